// modeldb_io.hpp -- the files of the model database: `cloud.ply`, a model's stable surfels as
// Model::exportModelPLY writes them (Core/Model/Model.cpp:1510-1598), and `tracks.ply`, its keypoint views in the binary layout
// of Model::exportTracksPLY with descriptors (:1386-1498) that Model::load reads back (:1658-1691).  Host code only: plain
// C++17, no HIP include -- g++ alone compiles it (tests/cpp/modeldb_io_sanitized.cpp); mmf_hip.hip includes it for the C ABI
// (mmf_ply_write_cloud, mmf_ply_read_cloud, mmf_tracks_ply_write, mmf_tracks_ply_read).
//
// Every reader takes the file as one byte buffer and moves a cursor that refuses to pass the end; no length found in a file
// sizes a copy before it has been checked against the format (256 floats per descriptor, one entry per view per track) and
// against what is left of the file.  Little-endian hosts only, like the reference (it writes its floats' bytes as they lie).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mmf {
namespace modeldb {

constexpr int kOk = 0, kInvalid = -1;  // MMF_OK, MMF_ERR_INVALID
constexpr size_t kCloudRecord = 31;    // x y z f32 | r g b u8 | nx ny nz f32 | radius f32
constexpr int kDescDim = 256;          // SuperPoint descriptors
constexpr size_t kTrackVertex = 12 + 2 + 4 * (size_t)kDescDim;  // x y z | uint16 list length | 256 f32
constexpr uint32_t kNoKeypoint = 0xFFFFFFFFu;                   // a track's entry where the view has no such row

inline int refuse(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return kInvalid;
}

// the product rounded to float before anything is added to it: no fused multiply-add, whatever the compiler's default
inline float rounded_product(float a, float b) {
    volatile float p = a * b;
    return p;
}
// ((p0 x + p1 y) + p2 z) + p3 per row p of the row-major 4 x 4 (the order of export_kernels.hpp)
inline void apply_pose(const float pose[16], const float c[3], float out[3]) {
    for (int r = 0; r < 3; ++r) {
        const float* p = pose + 4 * r;
        float s = rounded_product(p[0], c[0]) + rounded_product(p[1], c[1]);
        s = s + rounded_product(p[2], c[2]);
        out[r] = s + p[3];
    }
}

inline bool read_file(const char* path, std::vector<unsigned char>* bytes) {
    std::FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    bytes->clear();
    unsigned char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), fp)) > 0) bytes->insert(bytes->end(), chunk, chunk + got);
    const bool ok = std::ferror(fp) == 0;
    std::fclose(fp);
    return ok;
}
inline bool write_file(const char* path, const std::string& header, const void* body, size_t body_bytes) {
    std::FILE* fp = std::fopen(path, "wb");
    if (!fp) return false;
    bool ok = std::fwrite(header.data(), 1, header.size(), fp) == header.size();
    if (ok && body_bytes) ok = std::fwrite(body, 1, body_bytes, fp) == body_bytes;
    return (std::fclose(fp) == 0) && ok;
}

// a cursor over a file's bytes that never passes the end
struct Cursor {
    const unsigned char* p;
    size_t left;
    bool take(void* dst, size_t n) {
        if (n > left) return false;
        std::memcpy(dst, p, n);
        p += n, left -= n;
        return true;
    }
    // the literal text `s`, or nothing
    bool expect(const std::string& s) {
        if (s.size() > left || std::memcmp(p, s.data(), s.size()) != 0) return false;
        p += s.size(), left -= s.size();
        return true;
    }
    // a decimal number of at most 10 digits that fits 32 bits, written without sign, space or leading zero
    bool number(uint32_t* v) {
        unsigned long long acc = 0;
        size_t digits = 0;
        while (digits < left && digits < 10 && p[digits] >= '0' && p[digits] <= '9') acc = acc * 10 + (p[digits] - '0'), ++digits;
        if (digits == 0 || (digits > 1 && p[0] == '0') || acc > 0xFFFFFFFFull) return false;
        if (digits < left && p[digits] >= '0' && p[digits] <= '9') return false;
        p += digits, left -= digits;
        *v = (uint32_t)acc;
        return true;
    }
};

// ---- cloud.ply ---------------------------------------------------------------------------------------------------------------
inline std::string cloud_header(unsigned n) {  // Model.cpp:1516-1537, byte for byte
    return "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) +
           "\nproperty float x\nproperty float y\nproperty float z"
           "\nproperty uchar red\nproperty uchar green\nproperty uchar blue"
           "\nproperty float nx\nproperty float ny\nproperty float nz"
           "\nproperty float radius\nend_header\n";
}

inline int write_cloud(const char* path, const void* records, unsigned n, std::string* err) {
    if (!path || (!records && n)) return refuse(err, "mmf_ply_write_cloud: null argument");
    if (!write_file(path, cloud_header(n), records, (size_t)n * kCloudRecord))
        return refuse(err, std::string("mmf_ply_write_cloud: cannot write ") + path);
    return kOk;
}

// accepts exactly what write_cloud writes.  *n = the file's count whenever the header parses; records are copied only when
// the whole file is right and capacity >= *n
inline int read_cloud(const char* path, void* records, unsigned capacity, unsigned* n, std::string* err) {
    if (!path || !n || (!records && capacity)) return refuse(err, "mmf_ply_read_cloud: null argument");
    *n = 0;
    std::vector<unsigned char> bytes;
    if (!read_file(path, &bytes)) return refuse(err, std::string("mmf_ply_read_cloud: cannot read ") + path);
    Cursor c{bytes.data(), bytes.size()};
    uint32_t count = 0;
    if (!c.expect("ply\nformat binary_little_endian 1.0\nelement vertex ") || !c.number(&count))
        return refuse(err, "mmf_ply_read_cloud: not a binary little-endian PLY cloud");
    const std::string rest = cloud_header(0).substr(std::strlen("ply\nformat binary_little_endian 1.0\nelement vertex 0"));
    if (!c.expect(rest)) return refuse(err, "mmf_ply_read_cloud: unexpected header (the ten properties of a surfel cloud)");
    *n = count;
    if (c.left / kCloudRecord != count || c.left % kCloudRecord != 0)
        return refuse(err, "mmf_ply_read_cloud: the body does not hold exactly `element vertex` records");
    if (capacity < count) return refuse(err, "mmf_ply_read_cloud: capacity below the file's count");
    if (count) std::memcpy(records, c.p, (size_t)count * kCloudRecord);
    return kOk;
}

// ---- tracks.ply --------------------------------------------------------------------------------------------------------------
inline std::string tracks_header(uint32_t vertices, uint32_t tracks) {  // Model.cpp:1463-1482 with descriptors, binary
    return "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(vertices) +
           "\nproperty float32 x\nproperty float32 y\nproperty float32 z\nproperty list uint16 float32 descriptor"
           "\nelement edge 0\nproperty uint32 vertex1\nproperty uint32 vertex2\nelement track " +
           std::to_string(tracks) + "\nproperty list uint32 uint32 vertex_index\nend_header\n";
}

// The views of a model (the mmf_viewstore_store layout: counts[n_views], then the views' rows one after the other) as tracks:
// the store keeps no track identities, so track t is row t of every view that has one -- T = the largest count, entry i of
// track t = the vertex of row t of view i, or kNoKeypoint.  Vertices are numbered as the reference's loop meets them: track by
// track, inside a track by time index.  A vertex is pose * coordinate, the list length 256, the descriptor.  No edges: the
// rows of different views are not one physical point.
inline int write_tracks(const char* path, int n_views, const int* counts, const float* descriptor, const float* coordinate,
                        const float pose[16], std::string* err) {
    if (!path || !pose || n_views < 0 || (!counts && n_views)) return refuse(err, "mmf_tracks_ply_write: bad argument");
    size_t rows = 0, longest = 0;
    std::vector<size_t> first((size_t)n_views);
    for (int i = 0; i < n_views; ++i) {
        if (counts[i] < 0) return refuse(err, "mmf_tracks_ply_write: negative view size");
        first[(size_t)i] = rows;
        rows += (size_t)counts[i];
        if ((size_t)counts[i] > longest) longest = (size_t)counts[i];
    }
    if (rows && (!descriptor || !coordinate)) return refuse(err, "mmf_tracks_ply_write: null descriptors or coordinates");
    if (rows >= kNoKeypoint) return refuse(err, "mmf_tracks_ply_write: too many keypoints");
    std::vector<unsigned char> body(rows * kTrackVertex + longest * 4 * ((size_t)n_views + 1));
    unsigned char* v = body.data();
    unsigned char* t = body.data() + rows * kTrackVertex;
    const uint16_t nd = (uint16_t)kDescDim;
    uint32_t vertex = 0;
    for (size_t k = 0; k < longest; ++k) {
        const uint32_t nk = (uint32_t)n_views;
        std::memcpy(t, &nk, 4), t += 4;
        for (int i = 0; i < n_views; ++i) {
            uint32_t id = kNoKeypoint;
            if (k < (size_t)counts[i]) {
                const size_t row = first[(size_t)i] + k;
                float p[3];
                apply_pose(pose, coordinate + 3 * row, p);
                std::memcpy(v, p, 12), v += 12;
                std::memcpy(v, &nd, 2), v += 2;
                std::memcpy(v, descriptor + (size_t)kDescDim * row, 4 * (size_t)kDescDim), v += 4 * (size_t)kDescDim;
                id = vertex++;
            }
            std::memcpy(t, &id, 4), t += 4;
        }
    }
    if (!write_file(path, tracks_header(vertex, (uint32_t)longest), body.data(), body.size()))
        return refuse(err, std::string("mmf_tracks_ply_write: cannot write ") + path);
    return kOk;
}

// What Model::load rebuilds from the file: view i = the tracks with a keypoint at time index i, in track order.  *n_views
// and *n_rows are written whenever the file is right (a file without tracks says nothing of its views: 0 of them); counts
// (capacity cap_views) and the rows (capacity cap_rows) are written when they are not NULL and large enough, else refused.
// Coordinates come back as the file holds them: the writer's pose applied.
inline int read_tracks(const char* path, int cap_views, int* n_views, int* counts, int cap_rows, int* n_rows, float* descriptor,
                       float* coordinate, std::string* err) {
    if (!path || !n_views || !n_rows || cap_views < 0 || cap_rows < 0) return refuse(err, "mmf_tracks_ply_read: bad argument");
    *n_views = 0, *n_rows = 0;
    std::vector<unsigned char> bytes;
    if (!read_file(path, &bytes)) return refuse(err, std::string("mmf_tracks_ply_read: cannot read ") + path);
    Cursor c{bytes.data(), bytes.size()};
    uint32_t V = 0, T = 0;
    if (!c.expect("ply\nformat binary_little_endian 1.0\nelement vertex ") || !c.number(&V) ||
        !c.expect("\nproperty float32 x\nproperty float32 y\nproperty float32 z\nproperty list uint16 float32 descriptor"
                  "\nelement edge 0\nproperty uint32 vertex1\nproperty uint32 vertex2\nelement track ") ||
        !c.number(&T) || !c.expect("\nproperty list uint32 uint32 vertex_index\nend_header\n"))
        return refuse(err, "mmf_tracks_ply_read: unexpected header (binary tracks with descriptors, no edges)");
    // the vertices: every list length is checked where it stands, before the next vertex is looked for
    const unsigned char* vertices = c.p;
    for (uint32_t v = 0; v < V; ++v) {
        float xyz[3];
        uint16_t nd = 0;
        if (!c.take(xyz, 12) || !c.take(&nd, 2)) return refuse(err, "mmf_tracks_ply_read: the file ends inside a vertex");
        if (nd != kDescDim) return refuse(err, "mmf_tracks_ply_read: a descriptor that does not have 256 entries");
        if (c.left < 4 * (size_t)kDescDim) return refuse(err, "mmf_tracks_ply_read: the file ends inside a descriptor");
        c.p += 4 * (size_t)kDescDim, c.left -= 4 * (size_t)kDescDim;
    }
    // the tracks, first pass: the lengths, the indices, the views' sizes
    const Cursor tracks = c;
    uint32_t views = 0;
    std::vector<size_t> size;
    size_t rows = 0;
    for (uint32_t t = 0; t < T; ++t) {
        uint32_t nk = 0;
        if (!c.take(&nk, 4)) return refuse(err, "mmf_tracks_ply_read: the file ends inside a track");
        if (t == 0) {
            if (nk > c.left / 4) return refuse(err, "mmf_tracks_ply_read: the file ends inside a track");
            views = nk;
            size.assign(views, 0);
        }
        if (nk != views) return refuse(err, "mmf_tracks_ply_read: a track whose length is not the number of views");
        for (uint32_t i = 0; i < views; ++i) {
            uint32_t id = 0;
            if (!c.take(&id, 4)) return refuse(err, "mmf_tracks_ply_read: the file ends inside a track");
            if (id == kNoKeypoint) continue;
            if (id >= V) return refuse(err, "mmf_tracks_ply_read: a vertex index beyond the vertices");
            ++size[i], ++rows;
        }
    }
    if (c.left != 0) return refuse(err, "mmf_tracks_ply_read: bytes behind the last track");
    if (views > 0x7FFFFFFFu || rows > 0x7FFFFFFFu) return refuse(err, "mmf_tracks_ply_read: too many views or keypoints");
    *n_views = (int)views, *n_rows = (int)rows;
    if (counts) {
        if ((uint32_t)cap_views < views) return refuse(err, "mmf_tracks_ply_read: cap_views below the file's views");
        for (uint32_t i = 0; i < views; ++i) counts[i] = (int)size[i];
    }
    if (!descriptor && !coordinate) return kOk;
    if ((size_t)cap_rows < rows) return refuse(err, "mmf_tracks_ply_read: cap_rows below the file's keypoints");
    // second pass: row k of view i goes behind the rows of the views before it (every index and length has been checked)
    std::vector<size_t> next(views, 0);
    for (uint32_t i = 1; i < views; ++i) next[i] = next[i - 1] + size[i - 1];
    c = tracks;
    for (uint32_t t = 0; t < T; ++t) {
        uint32_t nk = 0;
        c.take(&nk, 4);
        for (uint32_t i = 0; i < views; ++i) {
            uint32_t id = 0;
            c.take(&id, 4);
            if (id == kNoKeypoint) continue;
            const unsigned char* src = vertices + (size_t)id * kTrackVertex;
            const size_t row = next[i]++;
            if (coordinate) std::memcpy(coordinate + 3 * row, src, 12);
            if (descriptor) std::memcpy(descriptor + (size_t)kDescDim * row, src + 14, 4 * (size_t)kDescDim);
        }
    }
    return kOk;
}

}  // namespace modeldb
}  // namespace mmf
