// What a front end pays on the host today for a frame that brings its label image: Segmentation.cpp:89-147 as a plain loop
// (one thread, three passes over the frame), built -O2 by tools/mask_probe.py and timed beside the device path.
#include <cmath>
#include <cstdint>
#include <cstring>

extern "C" int mask_host_loop(const uint8_t* labels, const float* depth, int n, const unsigned* ids, int n_models, unsigned next_id,
                              int allow_new, uint8_t* mapping, uint8_t* mask_out, unsigned* count_out, float* mean_out, float* std_out) {
    unsigned char index_of[256];
    std::memset(index_of, 0, sizeof(index_of));
    for (int i = 0; i < n_models; ++i) index_of[ids[i]] = (unsigned char)i;
    index_of[next_id] = (unsigned char)n_models;
    unsigned out_ids[256];
    std::memset(out_ids, 0, sizeof(out_ids));
    int has_new = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t v = labels[i];
        uint8_t o = 0;
        if (v) {
            if (mapping[v] != 0) {
                o = mapping[v];
                out_ids[o]++;
            } else if (allow_new && !has_new) {
                o = (uint8_t)next_id;
                mapping[v] = o;
                has_new = 1;
                out_ids[o]++;
            }
        } else {
            out_ids[0]++;
        }
        mask_out[i] = o;
    }
    const int entries = n_models + has_new;
    unsigned cnt[256];  // (entries: at most 255 models + the new label; ids and labels are bytes, hence every 256 here)
    for (int e = 0; e < entries; ++e) cnt[e] = 0, mean_out[e] = 0.f, std_out[e] = 0.f;
    for (int i = 0; i < n; ++i) {
        const int e = index_of[mask_out[i]];
        mean_out[e] += depth[i];
        cnt[e]++;
    }
    for (int e = 0; e < entries; ++e) mean_out[e] /= cnt[e] ? cnt[e] : 1;
    for (int i = 0; i < n; ++i) {
        const int e = index_of[mask_out[i]];
        std_out[e] += std::fabs(mean_out[e] - depth[i]);
    }
    for (int e = 0; e < entries; ++e) {
        std_out[e] /= cnt[e] ? cnt[e] : 1;
        count_out[e] = out_ids[e < n_models ? ids[e] : next_id] / 256;
        if (e >= n_models && count_out[e] < 1) count_out[e] = 1;
    }
    return has_new;
}
