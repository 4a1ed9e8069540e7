// Slic.h -- C++ shim with the class name and the members the reference's segmentation uses (Core/Segmentation/Slic.h:28-146,
// Slic.cpp:23-112; callers: Segmentation.cpp:173-178, 218-221, 683), forwarding to the C ABI of include/mmf_hip.h: the
// super-pixel engine (mmf_slic_segment) in place of gSLICr, and the resampling calls (mmf_slic_downsample*,
// mmf_slic_upsample_u8).  Differences a maintainer has to bridge:
//   * images are DEVICE pointers (cv::Mat::data after an upload), results are DeviceArray / std::vector, as OpenCV is not
//     part of this repository's dependencies; everything runs on the context's stream, the getters that return host data
//     synchronise;
//   * the engine's colour space is RGB (what the reference's caller passes); the channels take part symmetrically, so
//     setInputImage's swapRedBlue changes nothing and is accepted for the call shape only;
//   * spixelSize must divide width and height (the reference reads past its arrays otherwise): the constructor's
//     arguments are checked at the first processFrame, which reports MMF_ERR_INVALID through mmf::check.
#pragma once
#include <vector>

#include "cudafuncs.h"

class Slic {
   public:
    Slic() {}
    Slic(mmf::Context& ctx, unsigned width, unsigned height, int spixelSize)
        : ctx_(&ctx), width_((int)width), height_((int)height), spixelSize_(spixelSize) {
        spixelX_ = width_ / spixelSize_, spixelY_ = height_ / spixelSize_, spixelNum_ = spixelX_ * spixelY_;
        labels_.create((size_t)width_ * height_);
        counts_dev_.create((size_t)spixelNum_);
        spixelCounts_.assign((size_t)spixelNum_, 0);
        zeros_.create((size_t)width_ * height_), mean_.create((size_t)spixelNum_);
        mmf::hip_check(hipMemset(zeros_.ptr(), 0, (size_t)width_ * height_ * sizeof(float)), "hipMemset");
    }
    virtual ~Slic() {}

    bool isValid() const { return ctx_ != nullptr && input_ != nullptr; }
    unsigned getSuperpixelSize(unsigned index) const { return (unsigned)spixelCounts_[index]; }
    const std::vector<int>& getSpixelCounts() const { return spixelCounts_; }
    unsigned getSpixelNum() const { return (unsigned)spixelNum_; }
    unsigned getSpixelX() const { return (unsigned)spixelX_; }
    unsigned getSpixelY() const { return (unsigned)spixelY_; }

    // DEVICE pointer of the label image (int32 [height][width]); valid until the next processFrame
    const int* getResult() const { return labels_.ptr(); }
    // ... and a host copy (what the reference's getResult returns)
    std::vector<int> downloadResult() const {
        ctx_->synchronize();
        std::vector<int> host;
        labels_.download(host);
        return host;
    }

    // u8 x 3 interleaved, DEVICE; it must stay unchanged until processFrame has run
    void setInputImage(const unsigned char* rgb_dev, bool swapRedBlue = true) {
        (void)swapRedBlue;
        input_ = rgb_dev;
    }

    // engine->Process_Frame + Get_Seg_Mask, and spixelCounts when countSizes (Slic.cpp:72-80)
    void processFrame(bool countSizes = true) {
        mmf::check(mmf_slic_segment(ctx_->get(), input_, width_, height_, spixelSize_, 5, nullptr, labels_.ptr(), nullptr,
                                    nullptr),
                   "mmf_slic_segment");
        if (!countSizes) return;
        // the sizes of the FINAL labels (the engine's own counts are those of its last update): the census of a resampling
        mmf::check(mmf_slic_downsample(ctx_->get(), labels_.ptr(), width_, height_, spixelSize_, zeros_.ptr(), 1, 0, 0, 0.f,
                                       mean_.ptr(), counts_dev_.ptr()),
                   "mmf_slic_downsample");
        ctx_->synchronize();
        counts_dev_.download(spixelCounts_);
    }

    // downsample<float>(image, channel): DEVICE float32 [height][width][channels] -> [spixelY][spixelX] (device)
    template <typename T>
    DeviceArray<T> downsample(const T* image_dev, int channels = 1, int channel = 0) const {
        static_assert(sizeof(T) == sizeof(float), "Slic::downsample<T>: float images (Slic.h:51-54 excludes the 8-bit ones)");
        DeviceArray<T> out((size_t)spixelNum_);
        mmf::check(mmf_slic_downsample(ctx_->get(), labels_.ptr(), width_, height_, spixelSize_, image_dev, channels, channel, 0, 0.f,
                                       out.ptr(), nullptr),
                   "mmf_slic_downsample");
        return out;
    }
    template <typename T>
    DeviceArray<T> downsampleThresholded(const T* image_dev, T minThreshold) const {
        static_assert(sizeof(T) == sizeof(float), "Slic::downsampleThresholded<T>: float images");
        DeviceArray<T> out((size_t)spixelNum_);
        mmf::check(mmf_slic_downsample(ctx_->get(), labels_.ptr(), width_, height_, spixelSize_, image_dev, 1, 0, 1, minThreshold,
                                       out.ptr(), nullptr),
                   "mmf_slic_downsample");
        return out;
    }
    // downsample(): integer means of the input image's channels (2, 1, 0), u8 x 3 per super-pixel
    DeviceArray<unsigned char> downsample() const {
        DeviceArray<unsigned char> out((size_t)spixelNum_ * 3);
        mmf::check(mmf_slic_downsample_rgb(ctx_->get(), labels_.ptr(), width_, height_, spixelSize_, input_, 3, out.ptr()),
                   "mmf_slic_downsample_rgb");
        return out;
    }
    // upsample<unsigned char>(map): DEVICE u8 [spixelNum] -> [height][width]
    template <typename T>
    DeviceArray<T> upsample(const T* map_dev) const {
        static_assert(sizeof(T) == 1, "Slic::upsample<T>: 8-bit maps (the segmentation's)");
        DeviceArray<T> out((size_t)width_ * height_);
        mmf::check(mmf_slic_upsample_u8(ctx_->get(), labels_.ptr(), width_, height_, map_dev, spixelNum_, out.ptr()),
                   "mmf_slic_upsample_u8");
        return out;
    }

   private:
    mmf::Context* ctx_ = nullptr;
    const unsigned char* input_ = nullptr;
    int width_ = 0, height_ = 0, spixelSize_ = 0, spixelX_ = 0, spixelY_ = 0, spixelNum_ = 0;
    DeviceArray<int> labels_, counts_dev_;
    DeviceArray<float> zeros_, mean_;  // the census's image and result (processFrame(countSizes))
    std::vector<int> spixelCounts_;
};
