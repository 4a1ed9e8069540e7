// PointTracker.h -- C++ shim with the reference's class name (Core/Utils/PointTracker.h, .cpp:27-226) over the
// device-resident track table of the C ABI (include/mmf_hip.h, mmf_tracker_*).  The tracks live on the device: there is
// no getTracks(); what the reference's consumers read from the tracks is asked of the table (getLastTrackTransform,
// getVisible, the association inside processFrame).  Differences a maintainer has to bridge:
//   * Eigen::MatrixX2d / MatrixXd become row-major std::vector<double> (n x 2 normalised, n x 256), the types of
//     cpp/SuperPoint.h; the depth image is a DEVICE pointer to float32 metres [height][width] (cv::Mat after an upload);
//   * the table holds at most `capacity` tracks (a track that does not fit is dropped and counted: dropped()), a keypoint
//     outside the image gets NaN coordinates, pyramid level 0 only;
//   * Model::getLastTrackTransform(tracks) is a member here: the model's track set is the table's (modelId).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "RigidRANSAC.h"

namespace tracker {

class PointTracker {
   public:
    // intrinsics of pyramid level 0 (CameraModel::operator()(0))
    PointTracker(mmf::Context& ctx, int width, int height, float fx, float fy, float cx, float cy, int capacity = 4096,
                 int max_keypoints = 4096)
        : PointTracker(ctx.get(), width, height, fx, fy, cx, cy, capacity, max_keypoints) {}
    PointTracker(mmf_ctx* ctx, int width, int height, float fx, float fy, float cx, float cy, int capacity, int max_keypoints)
        : ctx_(ctx), width_(width), height_(height), capacity_(capacity), max_kp_(max_keypoints) {
        mmf::check(mmf_tracker_create(ctx_, width, height, fx, fy, cx, cy, capacity, max_keypoints, &t_), "mmf_tracker_create");
        if (hipMalloc(reinterpret_cast<void**>(&xy_dev_), (size_t)max_kp_ * 2 * sizeof(int)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&desc_dev_), (size_t)max_kp_ * 256 * sizeof(float)) != hipSuccess)
            mmf::check(MMF_ERR_HIP, "PointTracker: hipMalloc");
    }
    virtual ~PointTracker() {
        mmf_tracker_destroy(t_);  // (waits for the stream: nothing reads the staging buffers any more)
        (void)hipFree(xy_dev_);
        (void)hipFree(desc_dev_);
    }
    PointTracker(const PointTracker&) = delete;
    PointTracker& operator=(const PointTracker&) = delete;

    // addKeypoints(coordinates, descriptors, timestamp, depth, min_feature_distance, history) (:27-131)
    void addKeypoints(const std::vector<double>& coordinates, const std::vector<double>& descriptors, int64_t timestamp,
                      const float* depth_dev, float min_feature_distance = 0.7f, int history = 30) {
        const int n = (int)(coordinates.size() / 2);
        if (n > max_kp_ || descriptors.size() != (size_t)n * 256) mmf::check(MMF_ERR_INVALID, "PointTracker::addKeypoints: bad sizes");
        xy_.resize((size_t)n * 2), desc_.resize((size_t)n * 256);
        for (int k = 0; k < n; ++k) {  // cv::Point(cv::Vec2d): cvRound, half to even (:38)
            xy_[2 * k] = (int)std::lrint(coordinates[2 * k] * (double)width_);
            xy_[2 * k + 1] = (int)std::lrint(coordinates[2 * k + 1] * (double)height_);
        }
        for (size_t k = 0; k < desc_.size(); ++k) desc_[k] = (float)descriptors[k];
        mmf::check(mmf_ctx_synchronize(ctx_), "mmf_ctx_synchronize");  // the last add has read the staging buffers
        if (n > 0 && (hipMemcpy(xy_dev_, xy_.data(), xy_.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(desc_dev_, desc_.data(), desc_.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))
            mmf::check(MMF_ERR_HIP, "PointTracker::addKeypoints: hipMemcpy");
        mmf::check(mmf_tracker_add_keypoints(t_, n, xy_dev_, desc_dev_, depth_dev, (long long)timestamp, min_feature_distance, history),
                   "mmf_tracker_add_keypoints");
    }

    // the same with everything on the DEVICE, the number of keypoints included (SuperPoint::deviceFeatures): nothing waits;
    // rows from *n_dev on are not read
    void addKeypointsDevice(const int* n_dev, const int* xy_dev, const float* descriptor_dev, int64_t timestamp, const float* depth_dev,
                            float min_feature_distance = 0.7f, int history = 30) {
        mmf::check(mmf_tracker_add_keypoints_device(t_, n_dev, xy_dev, descriptor_dev, depth_dev, (long long)timestamp,
                                                    min_feature_distance, history),
                   "mmf_tracker_add_keypoints_device");
    }

    // prune(min_kps, min_time) (:170-203)
    void prune(size_t min_kps, uint64_t min_time) {
        mmf::check(mmf_tracker_prune(t_, (int)min_kps, (long long)min_time), "mmf_tracker_prune");
    }

    // Model::getLastTrackTransform (Model.cpp:739-775) of the model's tracks; fewer than 3 pairs: identity, no inliers
    RigidRANSAC::Result getLastTrackTransform(int modelId, const RigidRANSAC::Config& config = {10, 0.03f, 0.6f}) {
        RigidRANSAC::Result res;
        res.inlier.assign((size_t)capacity_, 0);
        const mmf_ransac_config cfg = {config.iterations, config.inlier_threshold, config.inlier_fraction};
        int has = 0;
        mmf::check(mmf_tracker_last_track_transform(t_, modelId, &cfg, res.transformation, &res.error, res.inlier.data(), &has),
                   "mmf_tracker_last_track_transform");
        if (!has) res.inlier.clear();
        return res;
    }

    size_t numTracks() {
        int n = 0;
        mmf::check(mmf_tracker_status(t_, &n, nullptr, nullptr), "mmf_tracker_status");
        return (size_t)n;
    }
    size_t length() {  // the common length of the reference's tracks
        int l = 0;
        mmf::check(mmf_tracker_status(t_, nullptr, &l, nullptr), "mmf_tracker_status");
        return (size_t)l;
    }
    size_t dropped() {
        int d = 0;
        mmf::check(mmf_tracker_status(t_, nullptr, nullptr, &d), "mmf_tracker_status");
        return (size_t)d;
    }
    // track->back() of every visible track (MultiMotionFusion.cpp:428-431): xy [n][2], coordinate [n][3], descriptor [n][256]
    int getVisible(std::vector<int>& xy, std::vector<float>& coordinate, std::vector<float>& descriptor) {
        xy.resize((size_t)capacity_ * 2), coordinate.resize((size_t)capacity_ * 3), descriptor.resize((size_t)capacity_ * 256);
        int n = 0;
        mmf::check(mmf_tracker_visible(t_, capacity_, &n, xy.data(), coordinate.data(), descriptor.data(), nullptr), "mmf_tracker_visible");
        xy.resize((size_t)n * 2), coordinate.resize((size_t)n * 3), descriptor.resize((size_t)n * 256);
        return n;
    }
    // the models' track sets (Model::updateTracks with every track: :622-627, initGlobalTracks); inside processFrame the
    // library associates by the frame's id image itself
    void associateAll(const std::vector<int>& modelIds) {
        mmf::check(mmf_tracker_associate_all(t_, modelIds.data(), (int)modelIds.size()), "mmf_tracker_associate_all");
    }
    // ----- the view log: the visible sets of the last `frames` adds stay on the device (0: off, the default), and
    // Model::store's views (Model.cpp:1617-1644, 508-522) are built from it -- no history kept by the caller
    void setViewLog(int frames) { mmf::check(mmf_tracker_set_view_log(t_, frames), "mmf_tracker_set_view_log"); }
    int frame() const { return mmf_tracker_frame(t_); }  // adds so far = the stamp of the newest frame
    struct ModelViews {
        std::vector<int> counts;             // keypoints per view
        const float* descriptor = nullptr;   // DEVICE [rows][256], the views one after the other; the tracker's, valid until
        const float* coordinate = nullptr;   // DEVICE [rows][3]                                  its next call
        int missing = 0;                     // views whose frame is not in the log (they are empty)
    };
    // view v = the logged keypoints of frame frames[v] that belong to the model now, in the frame poses[16 v ..] (row-major
    // 4 x 4, camera -> model at that frame) maps to; Model::storeDevice takes the result
    ModelViews modelViews(int modelId, const std::vector<int>& frames, const std::vector<float>& poses) {
        if (poses.size() != frames.size() * 16) mmf::check(MMF_ERR_INVALID, "PointTracker::modelViews: one pose per frame");
        ModelViews out;
        const int* counts = nullptr;
        mmf::check(mmf_tracker_model_views(t_, modelId, (int)frames.size(), frames.data(), poses.data(), &counts, &out.descriptor,
                                           &out.coordinate, &out.missing),
                   "mmf_tracker_model_views");
        out.counts.assign(counts, counts + frames.size());
        return out;
    }
    // ----- back-dating: Model::refineTrackSubset(tracks, parent, history) (Model.cpp:649-737) for the tracks that carry
    // `label` after this frame's association, from the table and the view log.  The entries are the reference's `poses`
    // (oldest first, the last one exactly the identity) with each pair's counts and estimate beside them.  `batch` is a
    // mmf_ransac_batch of this context with the reference's {10, 0.03, 0.6} (mmf_ransac_batch_create); frames are paired by
    // stamp, every pair gets a fresh engine, the window is bounded by the log.
    void reserveBackdate(int history) { mmf::check(mmf_tracker_reserve_backdate(t_, history), "mmf_tracker_reserve_backdate"); }
    std::vector<mmf_backdated_pose> backdate(int label, mmf_ransac_batch* batch, int history = 2) {
        std::vector<mmf_backdated_pose> out((size_t)(history > 0 ? history : 0));
        int n = 0;
        mmf::check(mmf_tracker_backdate(t_, label, history, batch, out.data(), (int)out.size(), &n), "mmf_tracker_backdate");
        out.resize((size_t)n);
        return out;
    }
    mmf_tracker* handle() const { return t_; }

   private:
    mmf_ctx* ctx_;
    mmf_tracker* t_ = nullptr;
    int width_, height_, capacity_, max_kp_;
    int* xy_dev_ = nullptr;
    float* desc_dev_ = nullptr;
    std::vector<int> xy_;
    std::vector<float> desc_;
};

}  // namespace tracker
