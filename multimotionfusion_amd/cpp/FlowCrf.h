// FlowCrf.h -- C++ shim of the flow-CRF inference engine (mmf_flowcrf_* of include/mmf_hip.h): the stage of
// the reference's flow_crf segmentation between its optical flow and its contours (Core/Segmentation/Segmentation.cpp:819-1263),
// for a front end that builds the rest.  Differences a maintainer has to bridge:
//   * every image is a DEVICE pointer (the frame's depth in metres, each model's vertex-confidence projection, the flow engine's
//     flow and motion images), the transformations are host matrices; everything runs on the context's stream, the getters
//     that return host data synchronise;
//   * the tracks come from a device tracker (PointTracker.h) or as plain device arrays;
//   * what the reference does with the id image afterwards (contours, the largest blob, ModelData) is not here.
#pragma once
#include <vector>

#include "cudafuncs.h"

class FlowCrf {
   public:
    FlowCrf() {}
    // fx .. cy: the camera of the frames; max_labels: models and the new label; max_tracks: a tracker's capacity
    FlowCrf(mmf::Context& ctx, int width, int height, float fx, float fy, float cx, float cy, int max_labels = 32, int max_tracks = 4096,
            const mmf_flowcrf_config* config = nullptr)
        : ctx_(&ctx), width_(width), height_(height) {
        mmf_flowcrf_config c;
        mmf::check(mmf_flowcrf_default_config(&c), "mmf_flowcrf_default_config");
        if (config) c = *config;
        mmf::check(mmf_flowcrf_create(ctx.get(), width, height, max_labels, max_tracks, fx, fy, cx, cy, &c, &engine_), "mmf_flowcrf_create");
    }
    FlowCrf(const FlowCrf&) = delete;
    FlowCrf& operator=(const FlowCrf&) = delete;
    virtual ~FlowCrf() {
        if (engine_) mmf_flowcrf_destroy(engine_);
    }

    bool isValid() const { return engine_ != nullptr; }
    int crfWidth() const { return width_ / 4; }
    int crfHeight() const { return height_ / 4; }

    // one inference from a tracker's table (nullptr: no tracks); asynchronous
    void infer(const mmf_flowcrf_input& in, mmf_tracker* tracker) {
        mmf::check(mmf_flowcrf_infer_tracker(engine_, &in, tracker), "mmf_flowcrf_infer_tracker");
    }
    // ... and from plain device arrays (nullptr: no tracks)
    void infer(const mmf_flowcrf_input& in, const mmf_flowcrf_tracks* tracks) {
        mmf::check(mmf_flowcrf_infer(engine_, &in, tracks), "mmf_flowcrf_infer");
    }

    // DEVICE pointers, valid until the next inference: the id image [h][w] and its x4 copy [height][width] (mmf_mask_segment's input)
    const unsigned char* getSegmentation() const { return result().ids; }
    const unsigned char* getSegmentationFull() const { return result().ids_full; }
    // the fused probabilities and the mean field's Q, f32 [labels][h][w]
    const float* getProbabilities(int* n_labels = nullptr) const {
        const Result r = result();
        if (n_labels) *n_labels = r.n_labels;
        return r.prob;
    }
    // a host copy of the id image (what the reference's model_segm holds)
    std::vector<unsigned char> downloadSegmentation() const {
        std::vector<unsigned char> host((size_t)crfWidth() * crfHeight());
        mmf::check(mmf_flowcrf_download(engine_, "ids", host.data(), host.size()), "mmf_flowcrf_download");
        return host;
    }
    int lastLaunches() const { return mmf_flowcrf_last_launches(engine_); }
    mmf_flowcrf* get() const { return engine_; }

   private:
    struct Result {
        const unsigned char *ids = nullptr, *ids_full = nullptr;
        const float *prob = nullptr, *q = nullptr;
        int n_labels = 0;
    };
    Result result() const {
        Result r;
        mmf::check(mmf_flowcrf_result(engine_, &r.ids, &r.ids_full, &r.prob, &r.q, nullptr, nullptr, &r.n_labels), "mmf_flowcrf_result");
        return r;
    }
    mmf::Context* ctx_ = nullptr;
    mmf_flowcrf* engine_ = nullptr;
    int width_ = 0, height_ = 0;
};
