// SuperPoint.h -- C++ shim with the class name and call shape the reference takes from the un-vendored
// super_point_inference package (Core/MultiMotionFusion.h:46,366; MultiMotionFusion.cpp:78,233):
//     kp_predictor = std::make_shared<SuperPoint>(keypoint_predictor_path);
//     std::tie(coordinates[i], descriptors[i]) = kp_predictor->getFeatures(img);
// forwarding to the C ABI of include/mmf_hip.h.  Differences a maintainer has to bridge:
//   * the constructor takes the 12 {weight, bias} arrays of SuperPointNet's state dict, not the path of the
//     TorchScript archive (reading that file needs libtorch, which stays on the reference's side);
//   * the image is a device pointer to interleaved u8 (cv::Mat::data after an upload), Eigen::MatrixX2d /
//     MatrixXd become row-major std::vector<double> (n x 2, n x 256), as the reference's Eigen types are not
//     part of this repository's dependencies.
#pragma once
#include <tuple>
#include <vector>

#include "RGBDOdometry.h"

class SuperPoint {
   public:
    // weights[24]: {w, b} of conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb
    // precision: F32 (the default) or F16 -- f16 operands, f32 accumulation; keypoints and descriptors stay f32
    enum Precision { F32 = MMF_SP_F32, F16 = MMF_SP_F16 };
    SuperPoint(mmf::Context& ctx, const float* const* weights, int max_width, int max_height, int max_keypoints = 4096,
               Precision precision = F32) {
        mmf::check(mmf_superpoint_create_ex(ctx.get(), weights, max_width, max_height, max_keypoints, (int)precision, &sp_),
                   "mmf_superpoint_create_ex");
        max_kp_ = max_keypoints;
    }
    Precision precision() const { return (Precision)mmf_superpoint_precision(sp_); }
    ~SuperPoint() { mmf_superpoint_destroy(sp_); }
    SuperPoint(const SuperPoint&) = delete;
    SuperPoint& operator=(const SuperPoint&) = delete;

    // (coordinates normalised by (width, height), descriptors), strongest keypoint first
    std::tuple<std::vector<double>, std::vector<double>> getFeatures(const unsigned char* image_dev, int width, int height,
                                                                     int channels, float conf_thresh = 0.015f, int nms_dist = 4,
                                                                     int border = 4) {
        std::vector<int> xy((size_t)max_kp_ * 2);
        std::vector<float> conf((size_t)max_kp_), desc((size_t)max_kp_ * 256);
        int n = 0;
        mmf::check(mmf_superpoint_get_features(sp_, image_dev, width, height, channels, conf_thresh, nms_dist, border, xy.data(),
                                               conf.data(), desc.data(), &n),
                   "mmf_superpoint_get_features");
        std::vector<double> coordinates((size_t)n * 2), descriptors((size_t)n * 256);
        for (int k = 0; k < n; ++k) {
            coordinates[2 * k] = (double)xy[2 * k] / (double)width;
            coordinates[2 * k + 1] = (double)xy[2 * k + 1] / (double)height;
        }
        for (size_t k = 0; k < descriptors.size(); ++k) descriptors[k] = (double)desc[k];
        return std::make_tuple(std::move(coordinates), std::move(descriptors));
    }

    // getFeatures without the host: enqueued on the context's stream, nothing awaited or read back.  The keypoints stay on
    // the device (deviceFeatures: pointers owned by this object, rows from *count on unspecified)
    void getFeaturesDevice(const unsigned char* image_dev, int width, int height, int channels, float conf_thresh = 0.015f,
                           int nms_dist = 4, int border = 4) {
        mmf::check(mmf_superpoint_get_features_device(sp_, image_dev, width, height, channels, conf_thresh, nms_dist, border),
                   "mmf_superpoint_get_features_device");
    }
    struct DeviceFeatures {
        const int *count, *status, *xy;  // status: 0 = the suppression converged, 1 = it did not (then *count is 0)
        const float *conf, *desc;
    };
    DeviceFeatures deviceFeatures() {
        DeviceFeatures d{};
        mmf::check(mmf_superpoint_device_features(sp_, &d.count, &d.xy, &d.conf, &d.desc, nullptr), "mmf_superpoint_device_features");
        mmf::check(mmf_superpoint_device_status(sp_, &d.status), "mmf_superpoint_device_status");
        return d;
    }
    int maxKeypoints() const { return max_kp_; }
    mmf_superpoint* handle() const { return sp_; }

   private:
    mmf_superpoint* sp_ = nullptr;
    int max_kp_ = 0;
};
