// Ferns.h -- C++ shim with the class name and the members of the reference's keyframe database (Core/Ferns.h:32-135,
// Ferns.cpp), forwarding to the C ABI of include/mmf_hip.h (mmf_ferns_*).  Stage one of relocalisation: the
// database, addFrame and the search of findFrame up to the keyframe it would hand its odometry.  findFrame itself -- the fern
// odometry, its acceptance rule, photometricCheck, the surface constraints -- belongs to stage two and is not declared;
// findCandidate is new here.  Differences a maintainer has to bridge:
//   * the constructor takes the context and the frame size (the reference reads the Resolution singleton) and the table of
//     ferns (the reference seeds std::mt19937 with time(0)); an empty table is mmf_ferns_make_table's with `seed`;
//   * the database has a capacity: addFrame returns false for a frame that was dropped because it is full (dropped());
//   * poses are 16 floats, row major; images are GPUTexture views of DEVICE images of the frame's size (a model's fill-in
//     images); every call here waits for its result, as the reference's does.
#pragma once
#include <cstdint>
#include <vector>

#include "GPUTexture.h"
#include "cudafuncs.h"

class Ferns {
   public:
    struct Candidate {  // what findCandidate found: findFrame's minId, its blockHDAware and whether it is above 0.3
        int id = -1;
        float dissim = 0.f, similarity = 0.f;
        bool candidate = false;
        float pose[16] = {0};
        int srcTime = 0;
    };
    struct Frame {  // Ferns::Frame (Ferns.h:49-79): the images stay on the device
        int id = -1, srcTime = 0, goodCodes = 0;
        float pose[16] = {0};
        const void *initRgb = nullptr, *initVerts = nullptr, *initNorms = nullptr;  // rgba8 / f32 x 4 / f32 x 4, [height][width]
    };

    Ferns(mmf::Context& ctx, int frameWidth, int frameHeight, int n, int maxDepth, const float photoThresh, const std::vector<int>& table = {},
          unsigned long long seed = 0, int capacity = 1024)
        : num(n), factor(8), width(frameWidth / factor), height(frameHeight / factor), maxDepth(maxDepth), photoThresh(photoThresh), owned_(true) {
        mmf_ferns_config c;
        mmf::check(mmf_ferns_default_config(&c), "mmf_ferns_default_config");
        c.num = n, c.max_depth_mm = maxDepth, c.capacity = capacity;
        std::vector<int> own(table);
        if (own.empty()) {
            own.resize((size_t)(n > 0 ? n : 0) * 6);
            mmf::check(mmf_ferns_make_table(seed, n, width, height, maxDepth, own.data()), "mmf_ferns_make_table");
        }
        mmf::check(own.size() == (size_t)n * 6 ? MMF_OK : MMF_ERR_INVALID, "Ferns: the table must hold n ferns of six integers");
        mmf::check(mmf_ferns_create(ctx.get(), frameWidth, frameHeight, &c, own.data(), &e_), "mmf_ferns_create");
    }
    // a view of an engine someone else owns (MultiMotionFusion::getFerns)
    Ferns(mmf_ferns* engine, int frameWidth, int frameHeight, int n, int maxDepth)
        : num(n), factor(8), width(frameWidth / factor), height(frameHeight / factor), maxDepth(maxDepth), photoThresh(0.f), e_(engine) {}
    Ferns(const Ferns&) = delete;
    Ferns& operator=(const Ferns&) = delete;
    virtual ~Ferns() {
        if (owned_) mmf_ferns_destroy(e_);
    }

    // Ferns.cpp:72-143: true when the frame became a keyframe
    bool addFrame(GPUTexture* imageTexture, GPUTexture* vertexTexture, GPUTexture* normalTexture, const float pose[16], int srcTime,
                  const float threshold) {
        mmf::check(mmf_ferns_set_threshold(e_, threshold), "mmf_ferns_set_threshold");
        return process(imageTexture, vertexTexture, normalTexture, pose, srcTime, MMF_FERNS_ADD).added != 0;
    }
    // Ferns.cpp:145-203 up to the decision to run the fern odometry: the closest keyframe older than the time gap
    Candidate findCandidate(GPUTexture* vertexTexture, GPUTexture* normalTexture, GPUTexture* imageTexture, const int time) {
        const float none[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const mmf_ferns_result_t r = process(imageTexture, vertexTexture, normalTexture, none, time, MMF_FERNS_FIND);
        Candidate c;
        c.id = r.closest, c.dissim = r.closest_dissim, c.similarity = r.closest_similarity, c.candidate = r.candidate != 0;
        for (int k = 0; k < 16; ++k) c.pose[k] = r.closest_pose[k];
        c.srcTime = r.closest_time;
        lastClosest = c.candidate ? c.id : -1;
        return c;
    }
    // frames.size() / frames.at(id) of the reference
    int frames() const { return last().count; }
    Frame frame(int id) const {
        Frame f;
        f.id = id;
        mmf::check(mmf_ferns_keyframe(e_, id, &f.initRgb, &f.initVerts, &f.initNorms, f.pose, &f.srcTime, &f.goodCodes), "mmf_ferns_keyframe");
        return f;
    }
    int dropped() const { return last().dropped_total; }
    mmf_ferns_result_t lastResult() const { return last(); }
    std::vector<uint8_t> lastCodes() const {
        std::vector<uint8_t> codes((size_t)num);
        mmf::check(mmf_ferns_download(e_, "codes", codes.data(), codes.size()), "mmf_ferns_download");
        return codes;
    }
    // Ferns.cpp:322-337 on two rows of codes (host arithmetic)
    static float blockHDAware(const std::vector<uint8_t>& f1, const std::vector<uint8_t>& f2) {
        int count = 0;
        float val = 0;
        for (size_t i = 0; i < f1.size() && i < f2.size(); ++i)
            if (f1[i] != badCode && f2[i] != badCode) {
                count++;
                if (f1[i] == f2[i]) val += 1.0f;
            }
        return val / (float)count;
    }
    void reset() { mmf::check(mmf_ferns_reset(e_), "mmf_ferns_reset"), processed_ = false; }
    mmf_ferns* handle() const { return e_; }

    const int num, factor, width, height, maxDepth;
    const float photoThresh;  // (stage two's photometricCheck)
    int lastClosest = -1;
    static const uint8_t badCode = 255;

   private:
    mmf_ferns_result_t process(GPUTexture* image, GPUTexture* vertex, GPUTexture* normal, const float pose[16], int time, int flags) {
        mmf::check(image && vertex && normal ? MMF_OK : MMF_ERR_INVALID, "Ferns: null texture");
        mmf::check(mmf_ferns_process(e_, image->data(), vertex->data(), normal->data(), pose, time, flags), "mmf_ferns_process");
        processed_ = true;
        return last();
    }
    mmf_ferns_result_t last() const {
        mmf_ferns_result_t r;
        std::memset(&r, 0, sizeof(r));
        r.closest = -1;
        if (owned_ && !processed_) return r;  // (an engine that has not run has no record: an empty database)
        const int rc = mmf_ferns_result(e_, &r);
        if (rc == MMF_ERR_STATE) {  // (a borrowed engine before its first frame)
            std::memset(&r, 0, sizeof(r));
            r.closest = -1;
            return r;
        }
        mmf::check(rc, "mmf_ferns_result");
        return r;
    }
    mmf_ferns* e_ = nullptr;
    bool owned_ = false, processed_ = false;
};
