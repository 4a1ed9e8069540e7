// FlowSegmentation.h -- C++ shim of the blob stage of the flow_crf segmentation (mmf_flowseg_* of include/mmf_hip.h; DESIGN.md
// 4.10): what the reference does with the MAP id image of its flow CRF (Core/Segmentation/Segmentation.cpp:1270-1324) -- the
// largest blob per model, the filled contours, the resize, ModelData and hasNewLabel -- for a front end that runs the
// stages itself (FlowCrf.h hands out the id image).  Differences a maintainer has to bridge:
//   * the id image and the depth are DEVICE pointers, the label table is a host array; run() is asynchronous on the
//     context's stream, result() waits for it;
//   * the contours are never materialised: the engine follows each border on the device and keeps the area and the fill.
#pragma once
#include <vector>

#include "cudafuncs.h"

class FlowSegmentation {
   public:
    FlowSegmentation() {}
    FlowSegmentation(mmf::Context& ctx, int width, int height, int max_labels = 32, const mmf_flowseg_config* config = nullptr)
        : width_(width), height_(height) {
        mmf_flowseg_config c;
        mmf::check(mmf_flowseg_default_config(&c), "mmf_flowseg_default_config");
        if (config) c = *config;
        mmf::check(mmf_flowseg_create(ctx.get(), width, height, max_labels, &c, &engine_), "mmf_flowseg_create");
    }
    FlowSegmentation(const FlowSegmentation&) = delete;
    FlowSegmentation& operator=(const FlowSegmentation&) = delete;
    virtual ~FlowSegmentation() {
        if (engine_) mmf_flowseg_destroy(engine_);
    }

    bool isValid() const { return engine_ != nullptr; }
    int crfWidth() const { return width_ / 4; }
    int crfHeight() const { return height_ / 4; }

    // ids [h][w] u8 and depth [height][width] f32 on the device; model_ids: the models' ids in list order
    void run(const unsigned char* ids_dev, const float* depth_dev, const std::vector<unsigned char>& model_ids, bool allow_new, unsigned new_id) {
        mmf::check(mmf_flowseg_run(engine_, ids_dev, depth_dev, model_ids.data(), (int)model_ids.size(), allow_new ? 1 : 0, new_id), "mmf_flowseg_run");
    }
    // waits for the run.  DEVICE pointers, valid until the next run: the id image at CRF size and at frame size
    struct Result {
        const unsigned char* segm = nullptr;
        const unsigned char* full = nullptr;
        mmf_flowseg_summary summary{};
    };
    Result result() const {
        Result r;
        mmf::check(mmf_flowseg_result(engine_, &r.segm, &r.full, &r.summary, nullptr, nullptr), "mmf_flowseg_result");
        return r;
    }
    // a host copy of the id image at CRF size (what the reference's model_segm holds after drawContours)
    std::vector<unsigned char> downloadSegmentation() const {
        std::vector<unsigned char> host((size_t)crfWidth() * crfHeight());
        mmf::check(mmf_flowseg_download(engine_, "segm", host.data(), host.size()), "mmf_flowseg_download");
        return host;
    }
    int lastLaunches() const { return mmf_flowseg_last_launches(engine_); }
    mmf_flowseg* handle() const { return engine_; }

   private:
    mmf_flowseg* engine_ = nullptr;
    int width_ = 0, height_ = 0;
};
