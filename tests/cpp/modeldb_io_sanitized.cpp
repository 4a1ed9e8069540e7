// Host code only: the files of the model database (csrc/modeldb_io.hpp).  Round trips of cloud.ply and tracks.ply, and the
// malformed files of tests/test_modeldb_io.py fed to the readers, every destination a heap block of exactly its capacity.
// Built with -fsanitize=address,undefined by tests/test_modeldb_io.py and run directly with a scratch directory as its
// argument; prints "ok <files read> <refused>" or the first thing that went wrong.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../multimotionfusion_amd/csrc/modeldb_io.hpp"

namespace {

namespace db = mmf::modeldb;
std::mt19937 rng(4321);
float uni(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }
int n_read = 0, n_refused = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            return false;                                                \
        }                                                                \
    } while (0)

bool put(const std::string& path, const std::vector<unsigned char>& bytes) {
    std::FILE* fp = std::fopen(path.c_str(), "wb");
    if (!fp) return false;
    const bool ok = bytes.empty() || std::fwrite(bytes.data(), 1, bytes.size(), fp) == bytes.size();
    return (std::fclose(fp) == 0) && ok;
}

bool replace(std::vector<unsigned char>& bytes, const std::string& from, const std::string& to) {
    const std::string s(bytes.begin(), bytes.end());
    const size_t at = s.find(from);
    if (at == std::string::npos) return false;
    const std::string r = s.substr(0, at) + to + s.substr(at + from.size());
    bytes.assign(r.begin(), r.end());
    return true;
}

bool cloud(const std::string& dir) {
    for (unsigned n : {0u, 1u, 5u}) {
        std::vector<unsigned char> rec((size_t)n * db::kCloudRecord);
        for (unsigned char& b : rec) b = (unsigned char)(rng() & 255u);
        const std::string path = dir + "/cloud.ply";
        std::string err;
        CHECK(db::write_cloud(path.c_str(), rec.data(), n, &err) == db::kOk);
        std::vector<unsigned char> file;
        CHECK(db::read_file(path.c_str(), &file));
        CHECK(file.size() == db::cloud_header(n).size() + rec.size());
        std::vector<unsigned char> back(rec.size());  // capacity == n exactly
        unsigned got = 99;
        CHECK(db::read_cloud(path.c_str(), back.data(), n, &got, &err) == db::kOk && got == n && back == rec);
        ++n_read;
        if (n == 0) continue;
        std::vector<unsigned char> small((size_t)(n - 1) * db::kCloudRecord);  // capacity < n
        CHECK(db::read_cloud(path.c_str(), small.data(), n - 1, &got, &err) == db::kInvalid && got == n);
        ++n_refused;
        std::vector<std::vector<unsigned char>> bad;
        bad.push_back(file), bad.back().pop_back();
        bad.push_back(file), bad.back().push_back(0);
        bad.push_back(file);
        CHECK(replace(bad.back(), "element vertex " + std::to_string(n), "element vertex " + std::to_string(n + 1)));
        bad.push_back(file);
        CHECK(replace(bad.back(), "property uchar green", "property uchar greem"));
        bad.push_back(file);
        CHECK(replace(bad.back(), "element vertex " + std::to_string(n), "element vertex 4294967295"));
        bad.push_back(std::vector<unsigned char>(file.begin(), file.begin() + 20));
        bad.push_back({});
        for (const auto& b : bad) {
            CHECK(put(path, b));
            CHECK(db::read_cloud(path.c_str(), back.data(), n, &got, &err) == db::kInvalid && !err.empty());
            ++n_refused;
        }
    }
    return true;
}

bool tracks(const std::string& dir) {
    const std::vector<std::vector<int>> cases = {{3, 0, 5}, {4}, {0, 0, 0}, {}, {33, 1}};
    for (const std::vector<int>& counts : cases) {
        size_t rows = 0, longest = 0;
        for (int c : counts) rows += (size_t)c, longest = std::max(longest, (size_t)c);
        std::vector<float> desc(rows * db::kDescDim), coord(rows * 3);
        for (float& v : desc) v = uni(-1, 1);
        for (float& v : coord) v = uni(-2, 2);
        const float pose[16] = {1, 0, 0, 0.5f, 0, 1, 0, -2.f, 0, 0, 1, 4.f, 0, 0, 0, 1};  // exact: the rows come back shifted
        const std::string path = dir + "/tracks.ply";
        std::string err;
        CHECK(db::write_tracks(path.c_str(), (int)counts.size(), counts.data(), desc.data(), coord.data(), pose, &err) == db::kOk);
        int nv = -1, nr = -1;
        CHECK(db::read_tracks(path.c_str(), 0, &nv, nullptr, 0, &nr, nullptr, nullptr, &err) == db::kOk);
        CHECK(nv == (longest ? (int)counts.size() : 0) && nr == (int)rows);
        std::vector<int> got_counts((size_t)nv);  // capacities == the sizes exactly
        std::vector<float> got_desc((size_t)nr * db::kDescDim), got_coord((size_t)nr * 3);
        CHECK(db::read_tracks(path.c_str(), nv, &nv, got_counts.data(), nr, &nr, got_desc.data(), got_coord.data(), &err) == db::kOk);
        ++n_read;
        if (longest) CHECK(got_counts == counts);
        CHECK(got_desc == desc);
        for (size_t r = 0; r < rows; ++r) {
            float p[3];
            db::apply_pose(pose, coord.data() + 3 * r, p);
            CHECK(std::memcmp(p, got_coord.data() + 3 * r, 12) == 0);
        }
        if (rows == 0) continue;
        std::vector<float> small_desc((size_t)(nr - 1) * db::kDescDim), small_coord((size_t)(nr - 1) * 3);
        CHECK(db::read_tracks(path.c_str(), nv, &nv, got_counts.data(), nr - 1, &nr, small_desc.data(), small_coord.data(), &err) == db::kInvalid);
        std::vector<int> small_counts((size_t)nv);  // (only nv - 1 of them are offered)
        CHECK(db::read_tracks(path.c_str(), nv - 1, &nv, small_counts.data(), nr, &nr, got_desc.data(), got_coord.data(), &err) == db::kInvalid);
        n_refused += 2;

        std::vector<unsigned char> file;
        CHECK(db::read_file(path.c_str(), &file));
        const size_t hdr = db::tracks_header((uint32_t)rows, (uint32_t)longest).size();
        const size_t tracks_at = hdr + rows * db::kTrackVertex;
        auto patch16 = [&](size_t at, uint16_t v) { auto b = file; std::memcpy(b.data() + at, &v, 2); return b; };
        auto patch32 = [&](size_t at, uint32_t v) { auto b = file; std::memcpy(b.data() + at, &v, 4); return b; };
        std::vector<std::vector<unsigned char>> bad;
        bad.push_back(patch16(hdr + 12, 255));
        bad.push_back(patch16(hdr + (rows - 1) * db::kTrackVertex + 12, 257));
        bad.push_back(patch16(hdr + 12, 65535));
        bad.push_back(patch32(tracks_at, (uint32_t)counts.size() + 1));
        bad.push_back(patch32(tracks_at, 0xFFFFFFF0u));
        bad.push_back(patch32(tracks_at + 4, (uint32_t)rows));
        bad.push_back(patch32(tracks_at + 4, 0xFFFFFFFEu));
        bad.push_back(std::vector<unsigned char>(file.begin(), file.begin() + hdr + 500));
        bad.push_back(std::vector<unsigned char>(file.begin(), file.begin() + hdr + 6));
        bad.push_back(std::vector<unsigned char>(file.begin(), file.begin() + tracks_at + 6));
        bad.push_back(std::vector<unsigned char>(file.begin(), file.begin() + tracks_at + 2));
        bad.push_back(file), bad.back().pop_back();
        bad.push_back(file), bad.back().push_back(0);
        bad.push_back(file);
        CHECK(replace(bad.back(), "element vertex " + std::to_string(rows), "element vertex " + std::to_string(rows + 1)));
        bad.push_back(file);
        CHECK(replace(bad.back(), "element vertex " + std::to_string(rows), "element vertex 4294967295"));
        bad.push_back(file);
        CHECK(replace(bad.back(), "element track " + std::to_string(longest), "element track " + std::to_string(longest + 1)));
        bad.push_back(file);
        CHECK(replace(bad.back(), "element edge 0", "element edge 1"));
        bad.push_back({});
        for (const auto& b : bad) {
            CHECK(put(path, b));
            CHECK(db::read_tracks(path.c_str(), nv, &nv, got_counts.data(), nr, &nr, got_desc.data(), got_coord.data(), &err) == db::kInvalid &&
                  !err.empty());
            nv = (int)got_counts.size(), nr = (int)rows;  // (a refusal says 0 / 0)
            ++n_refused;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: modeldb_io_sanitized <scratch directory>\n");
        return 2;
    }
    if (!cloud(argv[1]) || !tracks(argv[1])) return 1;
    std::printf("ok %d %d\n", n_read, n_refused);
    return 0;
}
