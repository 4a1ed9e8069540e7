// MultiMotionFusion.h -- C++ shims with the reference's class and method names for the surfel model
// (Core/Model/Model.h:120-360 + Core/Model/ModelProjection.h:37-77) and the orchestrator
// (Core/MultiMotionFusion.h:50-300), forwarding to the C ABI of include/mmf_hip.h.
//
// GPUTexture* arguments / getters keep their place in the signatures (GPUTexture.h: a view of a dense device image
// instead of an OpenGL texture).  Eigen / OpenCV types of the reference become plain arrays: poses are row-major
// float[16], FrameData carries raw pointers.  What the front-end pushes per GUI tick (GUI/MainController.cpp:641-670)
// and per frame (:588) compiles against this header; setters of subsystems that stay in the reference (redetection,
// ferns) are kept as recorded no-ops so those call sites need no #ifdef; the CRF and spawn setters are recorded and
// forwarded to the built-in dense-CRF segmentation.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "GPUTexture.h"
#include "RGBDOdometry.h"
#include "RigidRANSAC.h"
#include "PointTracker.h"
#include "SuperPoint.h"
#include "Ferns.h"

// FrameData (Core/FrameData.h:25-43) without OpenCV: one frame in HOST memory, as the log readers deliver it
struct FrameData {
    int64_t timestamp = 0;
    const uint8_t* rgb = nullptr;   // CV_8UC3, width x height
    const float* depth = nullptr;   // CV_32FC1 metres, 0 = invalid
    // optional CV_8UC1 image.  With setMaskSegmentation(true): the frame's raw labels as the reference's log readers deliver
    // them (Segmentation.cpp:89-147 runs inside processFrame; hasNewLabel is ignored).  Otherwise: an id image already mapped
    // to model ids, and hasNewLabel = SegmentationResult::hasNewLabel of it.
    const uint8_t* mask = nullptr;
    bool hasNewLabel = false;
};
// the same frame already resident in HBM (no upload inside processFrame)
struct FrameDataDevice {
    long long timestamp = 0;
    const uint8_t* rgb = nullptr;  // u8 x 3, interleaved, width x height
    const float* depth = nullptr;  // float32 metres, 0 = invalid
    const uint8_t* mask = nullptr;
    bool hasNewLabel = false;
    // not in the reference (a LogReader knows its next frame): the buffers the NEXT call will be given; their
    // sensor-side preparation is then enqueued while this call waits for its pose (mmf_frame::next_rgb / next_depth)
    const uint8_t* nextRgb = nullptr;
    const float* nextDepth = nullptr;
};

// The frame geometry the reference keeps in two process-wide singletons (Core/Utils/Resolution.h:26-67,
// Core/Utils/Intrinsics.h:24-66): set once by the front-end (GUI/MainController.cpp:147-148), read by the constructors.
class Resolution {
   public:
    static const Resolution& getInstance() { return instance(); }
    static void setResolution(int width, int height) { instance().w_ = width, instance().h_ = height; }
    const int& width() const { return check(), w_; }
    const int& height() const { return check(), h_; }
    const int& cols() const { return check(), w_; }
    const int& rows() const { return check(), h_; }
    int numPixels() const { return check(), w_ * h_; }

   private:
    static Resolution& instance() {
        static Resolution r;
        return r;
    }
    void check() const {
        if (w_ <= 0 || h_ <= 0) {
            std::fprintf(stderr, "You haven't initialised the Resolution class!\n");
            std::exit(-1);
        }
    }
    int w_ = 0, h_ = 0;
};
class Intrinsics {
   public:
    static const Intrinsics& getInstance() { return instance(); }
    static void setIntrinics(float fx = 0, float fy = 0, float cx = 0, float cy = 0) {  // (sic: the reference's spelling)
        Intrinsics& i = instance();
        i.fx_ = fx, i.fy_ = fy, i.cx_ = cx, i.cy_ = cy;
        i.check();
    }
    const float& fx() const { return check(), fx_; }
    const float& fy() const { return check(), fy_; }
    const float& cx() const { return check(), cx_; }
    const float& cy() const { return check(), cy_; }

   private:
    static Intrinsics& instance() {
        static Intrinsics i;
        return i;
    }
    void check() const {
        if (fx_ == 0 || fy_ == 0) {
            std::fprintf(stderr, "You haven't initialised the Intrinsics class!\n");
            std::exit(-1);
        }
    }
    float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
};

struct OdometryConfig {  // Core/Model/Model.h:45-61
    std::string init;
    std::string init_frame;
    int init_lvl = 0;
    bool icp_refine = false;
    int segm_lvl = 0;
};
struct SegmentationConfiguration {  // Core/Segmentation/Segmentation.h:72-80 ("": the built-in dense CRF; "flow_crf": flow + tracks + blobs)
    std::string mode;
    int sp_size = 16;
};

// Model::getModel()'s return type (Core/Model/Buffers.h:3-6).  The reference hands out the GL names of the vertex buffer that
// holds the surfels (48-byte Vertex records); here the store is three float4 arrays in HBM, handed out in place.
struct OutputBuffer {
    const float* positionConfidence = nullptr;  // device, [count][4]: x y z confidence
    const float* colourTime = nullptr;          // device, [count][4]: colour24-as-float, unused, initTime, timestamp
    const float* normalRadius = nullptr;        // device, [count][4]: nx ny nz radius
    unsigned count = 0;
};

class ModelProjection;

class Model {
   public:
    static const int MAX_VERTICES = 1024 * 1024;  // Model.cpp:119-126
    enum class MatchingType { Drost };            // Model.h:112 (model matching stays in the reference)

    struct surfel_t {  // Model.h:247-264, Vertex::SIZE = 48
        float position[3], confidence;
        float colour24, unused, initTime, timestamp;
        float normal[3], radius;
    };

    // Model(id, confidenceThresh, odom_cfg, enableFillIn, ...) (Model.cpp:147-262): a stand-alone model with its own
    // frame-to-model odometry
    Model(mmf::Context& ctx, int width, int height, float cx, float cy, float fx, float fy, unsigned char id,
          float confidenceThresh, bool enableFillIn = true, int maxSurfels = MAX_VERTICES)
        : width_(width), height_(height), fill_in_(enableFillIn) {
        mmf::check(mmf_model_create(ctx.get(), width, height, cx, cy, fx, fy, id, confidenceThresh, maxSurfels, &m_),
                   "mmf_model_create");
        mmf::check(mmf_odom_create(ctx.get(), width, height, cx, cy, fx, fy, 0.10f, std::sin(20.f * 3.14159254f / 180.f), &o_),
                   "mmf_odom_create");
        owned_ = true;
        identity(lastPose_);
    }
    // a model (and its odometry) owned by a MultiMotionFusion object
    Model(mmf_model* borrowed, mmf_odom* odom, int width, int height, bool fillIn)
        : m_(borrowed), o_(odom), owned_(false), width_(width), height_(height), fill_in_(fillIn) {
        identity(lastPose_);
    }
    ~Model() {
        if (owned_) {
            mmf_model_destroy(m_);
            mmf_odom_destroy(o_);
        }
    }
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;

    // ----- first frame
    void initialise(GPUTexture* rgb, GPUTexture* depthRaw, GPUTexture* depthFiltered, int time, float maxDepth) {
        mmf::check(mmf_model_initialise(m_, rgb->ptr<uint8_t>(), depthRaw->ptr<float>(), depthFiltered->ptr<float>(), time, maxDepth),
                   "mmf_model_initialise");
    }

    // ----- tracking (Model.h:150-157, Model.cpp:359-433)
    // generateCUDATextures(depth, mask): the filtered depth every model's initICP builds its pyramid from
    // (Model::GPUSetup::depth_tmp; the mask pyramid is never read by the tracker)
    static void generateCUDATextures(GPUTexture* depth, GPUTexture* /*mask*/) { shared_depth() = depth->ptr<float>(); }

    void initICP(bool doFillIn, bool frameToFrameRGB, float depthCutoff, GPUTexture* rgb) {
        float pose[16];
        getPose(pose);
        const bool fill = doFillIn;
        mmf::check(mmf_odom_init_icp_model(o_, (const float*)texture(fill ? "fillVertex" : "vertexConf"),
                                           (const float*)texture(fill ? "fillNormal" : "normalRadius"), depthCutoff, pose),
                   "mmf_odom_init_icp_model");
        const bool fillImage = fill || (frameToFrameRGB && allowsFillIn());
        mmf::check(mmf_odom_init_rgb_model(o_, (const uint8_t*)texture(fillImage ? "fillImage" : "image"), 0, 4),
                   "mmf_odom_init_rgb_model");
        mmf::check(mmf_odom_build_depth_pyramid(o_, shared_depth(), 0), "mmf_odom_build_depth_pyramid");
        mmf::check(mmf_odom_init_icp(o_, nullptr, nullptr, depthCutoff), "mmf_odom_init_icp");
        mmf::check(mmf_odom_init_rgb(o_, rgb->ptr<uint8_t>(), 0, 3), "mmf_odom_init_rgb");
    }

    void performTracking(bool frameToFrameRGB, bool rgbOnly, float icpWeight, bool pyramid, bool fastOdom, bool so3,
                         float maxDepthProcessed, GPUTexture* rgb, int64_t logTimestamp, bool tryFillIn = false) {
        float pose[16];
        getPose(pose);
        std::memcpy(lastPose_, pose, sizeof(pose));  // lastPose = pose (Model.cpp:412)
        initICP(tryFillIn, frameToFrameRGB, maxDepthProcessed, rgb);
        float trans[3] = {pose[3], pose[7], pose[11]};
        float rot[9] = {pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10]};
        // enableErrorRecording (every Model of the reference is created with it): icpError / rgbError are written
        mmf::check(mmf_odom_get_incremental_transformation(o_, trans, rot, rgbOnly, icpWeight, pyramid, fastOdom, so3,
                                                           const_cast<float*>(getICPErrorTexture()->ptr<float>()),
                                                           const_cast<float*>(getRGBErrorTexture()->ptr<float>())),
                   "mmf_odom_get_incremental_transformation");
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) pose[4 * r + c] = rot[3 * r + c];
            pose[4 * r + 3] = trans[r];
        }
        mmf::check(mmf_model_set_pose(m_, pose), "mmf_model_set_pose");
        timestamp_ns_.push_back(logTimestamp);
    }

    // ----- fusion (Model.h:196-207)
    float computeFusionWeight(float weightMultiplier) const {
        float pose[16], w = 0.f;
        getPose(pose);
        mmf::check(mmf_compute_fusion_weight(pose, lastPose_, weightMultiplier, &w), "mmf_compute_fusion_weight");
        return w;
    }
    void fuse(const int& time, GPUTexture* rgb, GPUTexture* mask, GPUTexture* depthRaw, GPUTexture* depthFiltered,
              const float depthCutoff, const float weightMultiplier) {
        mmf::check(mmf_model_fuse(m_, time, rgb->ptr<uint8_t>(), mask->ptr<uint8_t>(), depthRaw->ptr<float>(),
                                  depthFiltered->ptr<float>(), depthCutoff, computeFusionWeight(weightMultiplier)),
                   "mmf_model_fuse");
    }
    void clean(const int& time, std::vector<float>& graph, const int timeDelta, const float depthCutoff, const bool /*isFern*/,
               GPUTexture* depthFiltered, GPUTexture* mask, float outlierCoefficient = 3.0f) {
        if (!graph.empty()) {  // deformation graph: loop closure stays in the reference
            std::fprintf(stderr, "Model::clean: deformation graphs are not supported on this path\n");
            std::exit(-1);
        }
        mmf::check(mmf_model_clean(m_, time, timeDelta, depthCutoff, depthFiltered->ptr<float>(), mask->ptr<uint8_t>(), outlierCoefficient),
                   "mmf_model_clean");
    }

    // ----- prediction and fill-in (Model.h:208-220)
    bool allowsFillIn() const { return fill_in_; }
    void performFillIn(GPUTexture* rawRGB, GPUTexture* rawDepth, bool frameToFrameRGB, bool lost) {
        if (!fill_in_) return;
        mmf::check(mmf_model_perform_fill_in(m_, rawRGB->ptr<uint8_t>(), rawDepth->ptr<float>(), frameToFrameRGB, lost),
                   "mmf_model_perform_fill_in");
    }
    void combinedPredict(float depthCutoff, int time, int maxTime, int timeDelta, int /*ModelProjection::Prediction*/ = 0) {
        mmf::check(mmf_model_combined_predict(m_, depthCutoff, time, maxTime, timeDelta), "mmf_model_combined_predict");
    }
    void predictIndices(int time, float depthCutoff, int timeDelta) {
        mmf::check(mmf_model_predict_indices(m_, time, depthCutoff, timeDelta), "mmf_model_predict_indices");
    }
    // ModelProjection::synthesizeDepth (ModelProjection.h:49-50); result: texture("depth")
    void synthesizeDepth(float depthCutoff, float confThreshold, int time, int maxTime, int timeDelta) {
        mmf::check(mmf_model_synthesize_depth(m_, depthCutoff, confThreshold, time, maxTime, timeDelta), "mmf_model_synthesize_depth");
    }
    bool requiresFillIn(float ratio = 0.75f) {  // MultiMotionFusion::requiresFillIn(model, ratio)
        if (!fill_in_) return false;
        int r = 0;
        mmf::check(mmf_model_requires_fill_in(m_, ratio, &r), "mmf_model_requires_fill_in");
        return r != 0;
    }

    // ----- getters (Model.h:222-312)
    float getConfidenceThreshold() const { return mmf_model_confidence_threshold(m_); }
    void setConfidenceThreshold(float confThresh) { mmf::check(mmf_model_set_confidence_threshold(m_, confThresh), "setConfidenceThreshold"); }
    void setMaxDepth(float d) { mmf::check(mmf_model_set_max_depth(m_, d), "setMaxDepth"); }
    unsigned int getID() const { return (unsigned)mmf_model_id(m_); }
    unsigned lastCount() const {
        unsigned n = 0;
        mmf::check(mmf_model_count(m_, &n), "mmf_model_count");
        return n;
    }
    void overridePose(const float pose[16]) {  // pose = lastPose = p (Model.h:301-304)
        mmf::check(mmf_model_set_pose(m_, pose), "mmf_model_set_pose");
        std::memcpy(lastPose_, pose, sizeof(lastPose_));
    }
    void getPose(float pose[16]) const { mmf::check(mmf_model_get_pose(m_, pose), "mmf_model_get_pose"); }
    const float* getLastPose() const { return lastPose_; }
#ifdef MMF_HAVE_EIGEN
    Eigen::Matrix4f getPose() const {  // Model.h:292
        Eigen::Matrix<float, 4, 4, Eigen::RowMajor> p;
        getPose(p.data());
        return p;
    }
    void overridePose(const Eigen::Matrix4f& pose) {  // Model.h:301-304
        const Eigen::Matrix<float, 4, 4, Eigen::RowMajor> p = pose;
        overridePose(p.data());
    }
#endif
    std::vector<surfel_t> downloadMap() const {  // Model.cpp:1353-1384
        std::vector<surfel_t> out(lastCount());
        unsigned got = 0;
        if (!out.empty())
            mmf::check(mmf_model_download_map(m_, reinterpret_cast<float*>(out.data()), (unsigned)out.size(), &got),
                       "mmf_model_download_map");
        out.resize(got);
        return out;
    }
    // Model::exportModelPLY(export_dir, global_pose) (Model.cpp:1600-1605): the stable surfels under global_pose * pose^-1 as
    // `<export_dir>cloud-<id>.ply` (export_dir ends in '/', as the reference's).  The inverse is the rigid one, [R^T | -R^T t]
    // (MultiMotionFusion::savePly computes the product inside the library).
    void exportModelPLY(const std::string& export_dir, const float global_pose[16]) const {
        float p[16], inv[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, P[16];
        getPose(p);
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) inv[4 * r + q] = p[4 * q + r];
            inv[4 * r + 3] = -((p[r] * p[3] + p[4 + r] * p[7]) + p[8 + r] * p[11]);
        }
        for (int r = 0; r < 4; ++r)
            for (int q = 0; q < 4; ++q) {
                float acc = global_pose[4 * r] * inv[q];
                for (int k = 1; k < 4; ++k) acc = acc + global_pose[4 * r + k] * inv[4 * k + q];
                P[4 * r + q] = acc;
            }
        mmf::check(mmf_model_export_ply(m_, (export_dir + "cloud-" + std::to_string(getID()) + ".ply").c_str(), P), "mmf_model_export_ply");
    }
    // Ours (the reference restores no surfels): n packed 31-byte records {x y z f32 | r g b u8 | nx ny nz f32 | radius f32}
    // become the store's surfels under `pose` (nullptr: identity) with the given confidence and initTime = timestamp = time
    // (mmf_model_import_cloud: the store's content is replaced); the same from a PLY cloud; and every surfel's timestamp set
    // to `time`, into the prediction window of the frame that uses a restored map
    void importCloud(const void* records, unsigned n, const float* pose, float confidence, int time) {
        mmf::check(mmf_model_import_cloud(m_, pose, records, n, confidence, time), "mmf_model_import_cloud");
    }
    void importPly(const std::string& path, const float* pose, float confidence, int time) {
        mmf::check(mmf_model_import_ply(m_, path.c_str(), pose, confidence, time), "mmf_model_import_ply");
    }
    void setTimestamps(int time) { mmf::check(mmf_model_set_timestamps(m_, time), "mmf_model_set_timestamps"); }
    // Model.h:297: the surfel store the last fuse / clean left, in place (valid until this model's next fuse / clean)
    const OutputBuffer& getModel() {
        mmf::check(mmf_model_surfel_arrays(m_, &vbo_.positionConfidence, &vbo_.colourTime, &vbo_.normalRadius, &vbo_.count),
                   "mmf_model_surfel_arrays");
        return vbo_;
    }
    // Model.h:278-284: the error images of the last tracking (R32F, written on the last level-0 iteration) and the
    // confidence-carrying vertex image of the splat -- what Segmentation.cpp:218-219 reads of every model
    GPUTexture* getICPErrorTexture() { return error_texture(icp_tex_, "icp_error"); }
    GPUTexture* getRGBErrorTexture() { return error_texture(rgb_tex_, "rgb_error"); }
    std::vector<float> downloadICPErrorTexture() { return download_f32(getICPErrorTexture()->ptr<float>(), (size_t)width_ * height_); }
    std::vector<float> downloadRGBErrorTexture() { return download_f32(getRGBErrorTexture()->ptr<float>(), (size_t)width_ * height_); }
    std::vector<float> downloadVertexConfTexture() {  // RGBA32F: x y z confidence
        return download_f32(static_cast<const float*>(texture("vertexConf")), (size_t)width_ * height_ * 4);
    }
    RGBDOdometry::Stats getFrameOdometryStats() const {
        RGBDOdometry::Stats s;
        mmf::check(mmf_odom_get_stats(o_, &s), "mmf_odom_get_stats");
        return s;
    }
    // the GPUTexture getters of Model / ModelProjection (Model.h:232-244, ModelProjection.h:52-77) by name:
    // index vertConf colorTime normRad | image vertexConf normalRadius time | depth | fillVertex fillNormal fillImage
    const void* texture(const char* name, size_t* bytes = nullptr) const {
        void* p = nullptr;
        size_t b = 0;
        mmf::check(mmf_model_texture(m_, name, &p, &b), "mmf_model_texture");
        if (bytes) *bytes = b;
        return p;
    }
    size_t getSplatVertexConfTexBytes() const {
        size_t b = 0;
        (void)texture("vertexConf", &b);
        return b;
    }
    GPUTexture getRGBProjection() const { return GPUTexture(texture("image"), width_, height_, GPUTexture::RGBA8, "image"); }
    GPUTexture getVertexConfProjection() const { return GPUTexture(texture("vertexConf"), width_, height_, GPUTexture::RGBA32F, "vertexConf"); }
    GPUTexture getNormalProjection() const { return GPUTexture(texture("normalRadius"), width_, height_, GPUTexture::RGBA32F, "normalRadius"); }
    GPUTexture getTimeProjection() const { return GPUTexture(texture("time"), width_, height_, GPUTexture::R16UI, "time"); }
    GPUTexture getFillInImageTexture() const { return GPUTexture(texture("fillImage"), width_, height_, GPUTexture::RGBA8, "fillImage"); }
    GPUTexture getFillInVertexTexture() const { return GPUTexture(texture("fillVertex"), width_, height_, GPUTexture::RGBA32F, "fillVertex"); }
    GPUTexture getFillInNormalTexture() const { return GPUTexture(texture("fillNormal"), width_, height_, GPUTexture::RGBA32F, "fillNormal"); }
    GPUTexture getSparseIndexTex() const { return GPUTexture(texture("index"), width_, height_, GPUTexture::R32UI, "index"); }
    GPUTexture getSparseVertConfTex() const { return GPUTexture(texture("vertConf"), width_, height_, GPUTexture::RGBA32F, "vertConf"); }
    GPUTexture getSparseColorTimeTex() const { return GPUTexture(texture("colorTime"), width_, height_, GPUTexture::RGBA32F, "colorTime"); }
    GPUTexture getSparseNormalRadTex() const { return GPUTexture(texture("normRad"), width_, height_, GPUTexture::RGBA32F, "normRad"); }
    // ----- keypoint redetection (Model.cpp:781-874, 1617-1656).  tracker::KeypointPtr lists become host arrays: n keypoints with
    // descriptor [n][256] and coordinate [n][3].  The views live in a view store (mmf_viewstore: the fusion's for a model of a
    // MultiMotionFusion object, set by getModels / getInactiveModels; setViewStore for a stand-alone model).
    void setViewStore(mmf_viewstore* vs) { views_ = vs; }
    // Model::store(model_db_path, pose, clear) without the files: the views of tracks_local = computeTrackProjectionFirstFrame(),
    // n_views time indices with counts[v] valid keypoints each, rows one after the other, coordinates in the model's frame.
    // false: stored before, skipped (:1618-1621)
    bool store(int n_views, const int* counts, const float* descriptor, const float* coordinate) {
        int stored = 0;
        mmf::check(mmf_viewstore_store(need_views(), (int)getID(), n_views, counts, descriptor, coordinate, &stored), "mmf_viewstore_store");
        return stored != 0;
    }
    // the same with the rows on the DEVICE (tracker::PointTracker::modelViews): nothing passes through the host
    bool storeDevice(int n_views, const int* counts, const float* descriptor_dev, const float* coordinate_dev) {
        int stored = 0;
        mmf::check(mmf_viewstore_store_device(need_views(), (int)getID(), n_views, counts, descriptor_dev, coordinate_dev, &stored),
                   "mmf_viewstore_store_device");
        return stored != 0;
    }
    struct BestMatch : RigidRANSAC::Result {
        int view = -1;  // the time index of the winning view (-1: no estimate; transformation identity, error +inf)
    };
    // Model::getBestMatch(keypoints, config): the config must be the one the reference passes, {10, 0.03, 0.8}
    // (MultiMotionFusion.cpp:513): the library constructs that RigidRANSAC itself
    BestMatch getBestMatch(const float* descriptor, const float* coordinate, int n, const RigidRANSAC::Config& config) const {
        if (config.iterations != 10 || config.inlier_threshold != 0.03f || config.inlier_fraction != 0.8f)
            mmf::check(MMF_ERR_INVALID, "Model::getBestMatch: only RigidRANSAC::Config{10, 0.03, 0.8}");
        float* dev = nullptr;
        if (n > 0 && (hipMalloc(reinterpret_cast<void**>(&dev), (size_t)n * 256 * sizeof(float)) != hipSuccess ||
                      hipMemcpy(dev, descriptor, (size_t)n * 256 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
            (void)hipFree(dev);
            mmf::check(MMF_ERR_HIP, "Model::getBestMatch: upload of the descriptors");
        }
        BestMatch best;
        best.inlier.assign((size_t)(n > 0 ? n : 1), 0);
        int inliers = 0, n_matches = 0, found = 0;
        const int rc = mmf_viewstore_best_match(need_views(), (int)getID(), dev, coordinate, n, best.transformation, &best.error, &inliers,
                                                &best.view, &n_matches, best.inlier.data(), &found);
        (void)hipFree(dev);
        mmf::check(rc, "mmf_viewstore_best_match");
        best.inlier.resize(found ? (size_t)n_matches : 0);
        return best;
    }
    // Model::activate(pose, timestamp): overridePose and a pose list of one entry.  (Inside processFrame the library activates a
    // re-detected model itself: mmf_fusion_set_redetection.)
    void activate(const float pose[16], const int64_t& timestamp) {
        overridePose(pose);
        timestamp_ns_.assign(1, timestamp);
    }
    mmf_model* handle() const { return m_; }
    mmf_odom* odometryHandle() const { return o_; }

   private:
    static const float*& shared_depth() {
        static const float* d = nullptr;
        return d;
    }
    static void identity(float* m) {
        for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
    }
    GPUTexture* error_texture(std::unique_ptr<GPUTexture>& t, const char* name) {
        void* p = nullptr;
        size_t b = 0;
        mmf::check(mmf_odom_buffer(o_, name, 0, &p, &b), "mmf_odom_buffer");
        if (!t)
            t.reset(new GPUTexture(p, width_, height_, GPUTexture::R32F, name));
        else
            t->rebind(p);
        return t.get();
    }
    static std::vector<float> download_f32(const float* dev, size_t n) {  // GPUTexture::downloadTexture (cv::Mat in the reference)
        std::vector<float> host(n);
        if (hipMemcpy(host.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) host.clear();
        return host;
    }
    mmf_viewstore* need_views() const {
        if (!views_) mmf::check(MMF_ERR_STATE, "Model: no view store (setViewStore)");
        return views_;
    }
    mmf_viewstore* views_ = nullptr;
    mmf_model* m_ = nullptr;
    mmf_odom* o_ = nullptr;
    bool owned_ = false;
    int width_ = 0, height_ = 0;
    bool fill_in_ = false;
    float lastPose_[16];
    std::vector<int64_t> timestamp_ns_;
    OutputBuffer vbo_;
    std::unique_ptr<GPUTexture> icp_tex_, rgb_tex_;
};

typedef std::shared_ptr<Model> ModelPointer;
typedef std::list<ModelPointer> ModelList;

class MultiMotionFusion {
   public:
    // MultiMotionFusion::MultiMotionFusion (MultiMotionFusion.cpp:21-97); unset options keep the
    // GUI defaults of GUI/MainController.cpp:333-345, 514-517
    MultiMotionFusion(mmf::Context& ctx, int width, int height, float cx, float cy, float fx, float fy,
                      const mmf_fusion_config* cfg = nullptr)
        : width_(width), height_(height), ctx_(ctx.get()), fx_(fx), fy_(fy), cx_(cx), cy_(cy) {
        mmf::check(mmf_fusion_create(ctx.get(), width, height, cx, cy, fx, fy, cfg, &f_), "mmf_fusion_create");
        mmf::check(mmf_fusion_get_config(f_, &cfg_), "mmf_fusion_get_config");
        mmf::check(mmf_crf_default_config(&crf_), "mmf_crf_default_config");
        mmf::check(mmf_flowseg_default_config(&flowseg_), "mmf_flowseg_default_config");
        pushCrf();
    }
    // The reference's own argument list (Core/MultiMotionFusion.h:54-61, .cpp:21-97): the frame geometry comes from the
    // Resolution / Intrinsics singletons, the device context is the process-wide default one (device 0, like the reference's
    // cudaGetDeviceProperties(&prop, 0)).  Arguments of subsystems that stay in the reference (loop closure, relocalisation,
    // ferns, model matching, keypoint predictor path, segmentation mode) are recorded; closeLoops must be false, as the
    // front-end passes it (GUI/MainController.cpp:361, 514-515: openLoop is hard-wired).
    MultiMotionFusion(const int timeDelta = 200, const int countThresh = 35000, const float errThresh = 5e-05f, const float covThresh = 1e-05f,
                      const bool closeLoops = false, const bool iclnuim = false, const bool reloc = false, const float photoThresh = 115,
                      const float initConfidenceGlobal = 4, const float initConfidenceObject = 2, const float depthCut = 3,
                      const float icpThresh = 10, const bool fastOdom = false, const float fernThresh = 0.3095f, const bool so3 = true,
                      const bool frameToFrameRGB = false, const unsigned modelSpawnOffset = 20,
                      const Model::MatchingType /*matchingType*/ = Model::MatchingType::Drost, const std::string& exportDirectory = "",
                      const bool exportSegmentationResults = false, const std::string keypoint_predictor_path = {},
                      const OdometryConfig& odom_cfg = {}, const SegmentationConfiguration& segm_cfg = {})
        : width_(Resolution::getInstance().width()), height_(Resolution::getInstance().height()), odom_cfg_(odom_cfg), segm_cfg_(segm_cfg),
          exportDirectory_(exportDirectory) {
        if (closeLoops) {
            std::fprintf(stderr, "MultiMotionFusion: loop closure is not part of this path (the front-end runs with openLoop)\n");
            std::exit(-1);
        }
        mmf_fusion_config cfg;
        mmf::check(mmf_fusion_default_config(&cfg), "mmf_fusion_default_config");
        cfg.time_delta = timeDelta, cfg.conf_global_init = initConfidenceGlobal, cfg.conf_object_init = initConfidenceObject;
        cfg.depth_cutoff = depthCut, cfg.icp_weight = icpThresh, cfg.fast_odom = fastOdom, cfg.so3 = so3;
        cfg.frame_to_frame_rgb = frameToFrameRGB;
        other_["countThresh"] = (float)countThresh, other_["errThresh"] = errThresh, other_["covThresh"] = covThresh;
        other_["iclnuim"] = iclnuim, other_["reloc"] = reloc, other_["photoThresh"] = photoThresh, other_["fernThresh"] = fernThresh;
        other_["modelSpawnOffset"] = (float)modelSpawnOffset, other_["exportSegmentationResults"] = exportSegmentationResults;
        other_["hasKeypointPredictor"] = !keypoint_predictor_path.empty();
        const Intrinsics& K = Intrinsics::getInstance();
        ctx_ = defaultContext().get(), fx_ = K.fx(), fy_ = K.fy(), cx_ = K.cx(), cy_ = K.cy();
        mmf::check(mmf_fusion_create(defaultContext().get(), width_, height_, K.cx(), K.cy(), K.fx(), K.fy(), &cfg, &f_), "mmf_fusion_create");
        mmf::check(mmf_fusion_get_config(f_, &cfg_), "mmf_fusion_get_config");
        // the segmentation of a maskless multi-model frame: the built-in dense CRF in the default mode (""); "flow_crf":
        // Farneback flow, the flow-CRF inference on the keypoint tracks and the blob stage (Segmentation.cpp:779-1324); any
        // other mode keeps the error of a missing segmentation
        mmf::check(mmf_crf_default_config(&crf_), "mmf_crf_default_config");
        mmf::check(mmf_flowseg_default_config(&flowseg_), "mmf_flowseg_default_config");
        crf_.model_spawn_offset = (int)modelSpawnOffset, crf_.spixel_size = segm_cfg.sp_size;
        mask_.model_spawn_offset = (int)modelSpawnOffset, flowseg_.model_spawn_offset = (int)modelSpawnOffset;
        pushCrf();
        if (segm_cfg_.mode == "flow_crf") {
            setOpticalFlow(true);
            setFlowInference(true);
            pushFlowSeg();
        }
    }
    static mmf::Context& defaultContext() {
        static mmf::Context ctx(0);
        return ctx;
    }
    const OdometryConfig& getOdometryConfig() const { return odom_cfg_; }
    const SegmentationConfiguration& getSegmentationConfiguration() const { return segm_cfg_; }

    virtual ~MultiMotionFusion() {
        for (auto& kv : textures_) delete kv.second;
        models_.clear();
        mmf_fusion_destroy(f_);
        tracker_.reset();  // (after the fusion, which holds its handle)
        (void)hipFree(kp_rgb_);
        (void)hipFree(kp_depth_);
    }
    MultiMotionFusion(const MultiMotionFusion&) = delete;
    MultiMotionFusion& operator=(const MultiMotionFusion&) = delete;

    void preallocateModels(unsigned count) { mmf::check(mmf_fusion_preallocate_models(f_, count), "mmf_fusion_preallocate_models"); }

    // bool processFrame(const FrameData&, const Eigen::Matrix4f* inPose = 0, float weightMultiplier = 1,
    //                   GroundTruthOdometryInterface* = nullptr, bool bootstrap = false)  (MultiMotionFusion.h:78-80).
    // Like the reference it prints "invalid image data" and returns false for a bad frame and
    // returns false after a regular frame (MultiMotionFusion.cpp:209-212, 853).  The frame is uploaded inside (:221, :261).
    bool processFrame(const FrameData& frame, const float* inPose = nullptr, const float weightMultiplier = 1.f,
                      void* /*GroundTruthOdometryInterface*/ = nullptr, const bool bootstrap = false) {
        const FrameData next = next_;  // announced by announceNextFrame (one call only)
        next_ = FrameData();
        if (kp_predictor_ && !kp_on_device_ && frame.rgb && frame.depth && frame.timestamp >= 0 && !addFrameKeypoints(frame)) return false;
        return finish(mmf_fusion_process_frame_host_next(f_, frame.rgb, frame.depth, frame.mask, frame.hasNewLabel, frame.timestamp, inPose,
                                                         weightMultiplier, bootstrap, next.rgb, next.depth),
                      "mmf_fusion_process_frame_host");
    }
    // not in the reference: a front-end whose reader is one frame ahead (GUI/MainController.cpp:547-590) announces the frame
    // the NEXT processFrame call will bring (same buffers, unchanged until then): it is uploaded while this one is tracked
    // and prepared while this one is fused.  Optional; a frame that was announced and never comes costs nothing but the copy.
    void announceNextFrame(const FrameData& next) { next_ = next; }
#ifdef MMF_HAVE_EIGEN
    // the reference's exact signature (MultiMotionFusion.h:78-80) and pose getter (:196)
    bool processFrame(const FrameData& frame, const Eigen::Matrix4f* inPose, const float weightMultiplier = 1.f,
                      void* gt_pose = nullptr, const bool bootstrap = false) {
        if (!inPose) return processFrame(frame, static_cast<const float*>(nullptr), weightMultiplier, gt_pose, bootstrap);
        const Eigen::Matrix<float, 4, 4, Eigen::RowMajor> p = *inPose;
        return processFrame(frame, p.data(), weightMultiplier, gt_pose, bootstrap);
    }
    Eigen::Matrix4f getCurrPose() const {
        Eigen::Matrix<float, 4, 4, Eigen::RowMajor> p;
        mmf::check(mmf_fusion_get_pose(f_, p.data()), "mmf_fusion_get_pose");
        return p;
    }
#endif
    bool processFrame(const FrameDataDevice& frame, const float* inPose = nullptr, const float weightMultiplier = 1.f,
                      const bool bootstrap = false) {
        mmf_segmentation seg;
        std::memset(&seg, 0, sizeof(seg));
        seg.mask = frame.mask, seg.has_new_label = frame.hasNewLabel;
        mmf_frame fr;
        std::memset(&fr, 0, sizeof(fr));
        fr.rgb = frame.rgb, fr.depth = frame.depth, fr.timestamp = frame.timestamp;
        fr.in_pose = inPose, fr.weight_multiplier = weightMultiplier, fr.bootstrap = bootstrap, fr.icp_refine = 1;
        fr.segmentation = frame.mask ? &seg : nullptr;
        fr.next_rgb = frame.nextRgb, fr.next_depth = frame.nextDepth;
        return finish(mmf_fusion_process_frame_ex(f_, &fr), "mmf_fusion_process_frame_ex");
    }
    // the same frame step with odom_cfg.init == "kp" (MultiMotionFusion.cpp:312-384): trackTransform is
    // RigidRANSAC::Result::transformation of Model::getLastTrackTransform (row-major 4x4), icpRefine is
    // odom_cfg.icp_refine.  In the reference this is selected by the OdometryConfig passed to the constructor.
    bool processFrame(const FrameDataDevice& frame, const float trackTransform[16], const bool icpRefine,
                      const float weightMultiplier = 1.f) {
        return finish(mmf_fusion_process_frame_init(f_, frame.rgb, frame.depth, frame.timestamp, trackTransform, icpRefine, weightMultiplier),
                      "mmf_fusion_process_frame_init");
    }
    // not in the reference: start the next frame's input-side work (filter, pyramids, gradients) on a second
    // stream while the current frame is still being fused; pass the same frame to processFrame afterwards
    void prefetchFrame(const FrameDataDevice& next) {
        mmf::check(mmf_fusion_prefetch_frame(f_, next.rgb, next.depth), "mmf_fusion_prefetch_frame");
    }

    void predict() { mmf::check(mmf_fusion_predict(f_), "mmf_fusion_predict"); }  // MultiMotionFusion.h:86

    // getIndexMap() (:92): the global model's projections (ModelProjection's getters live on Model here)
    Model& getIndexMap() { return *getBackgroundModel(); }
    ModelPointer getBackgroundModel() { return getModels().front(); }
    ModelList& getModels() {  // :107 -- rebuilt from the native list when it changed
        const int n = mmf_fusion_num_models(f_);
        bool same = (int)models_.size() == n;
        int i = 0;
        for (auto it = models_.begin(); same && it != models_.end(); ++it, ++i) same = (*it)->handle() == mmf_fusion_model_at(f_, i);
        if (!same) {
            models_.clear();
            for (int k = 0; k < n; ++k)
                models_.push_back(std::make_shared<Model>(mmf_fusion_model_at(f_, k), mmf_fusion_odometry_at(f_, k), width_, height_,
                                                          k == 0 && cfg_.fill_in));
            for (auto& m : models_) m->setViewStore(mmf_fusion_viewstore(f_));
        }
        return models_;
    }
    ModelList& getInactiveModels() {  // inactiveModels (MultiMotionFusion.h:351): rebuilt from the native list
        inactive_.clear();
        for (int k = 0; k < mmf_fusion_num_inactive_models(f_); ++k) {
            inactive_.push_back(std::make_shared<Model>(mmf_fusion_inactive_model_at(f_, k), nullptr, width_, height_, false));
            inactive_.back()->setViewStore(mmf_fusion_viewstore(f_));
        }
        return inactive_;
    }
    // getTextures() (:124): the raw input images of the current frame
    std::map<std::string, GPUTexture*>& getTextures() {
        struct Spec { const std::string* name; GPUTexture::Format fmt; };
        const Spec specs[] = {{&GPUTexture::RGB, GPUTexture::RGB8}, {&GPUTexture::DEPTH_METRIC, GPUTexture::R32F},
                              {&GPUTexture::DEPTH_METRIC_FILTERED, GPUTexture::R32F}, {&GPUTexture::MASK, GPUTexture::R8UI}};
        for (const Spec& s : specs) {
            const void* p = nullptr;
            size_t b = 0;
            mmf::check(mmf_fusion_texture(f_, s.name->c_str(), &p, &b), "mmf_fusion_texture");
            auto it = textures_.find(*s.name);
            if (it == textures_.end())
                textures_[*s.name] = new GPUTexture(p, width_, height_, s.fmt, *s.name);
            else
                it->second->rebind(p);
        }
        return textures_;
    }
    // getModelToModel() (:136): the front-end only reads lastICPError / lastICPCount of it for its plots
    // (GUI/MainController.cpp:627-640); here they are the global model's frame-to-model statistics
    RGBDOdometry::Stats getModelToModel() {
        RGBDOdometry::Stats s;
        mmf::check(mmf_odom_get_stats(mmf_fusion_odometry(f_), &s), "mmf_odom_get_stats");
        return s;
    }
    float getConfidenceThreshold() { return mmf_model_confidence_threshold(mmf_fusion_model(f_)); }

    // ----- the setters of GUI/MainController.cpp:641-670
    void setRgbOnly(const bool& v) { mmf::check(mmf_fusion_set_rgb_only(f_, v), "setRgbOnly"); }
    void setIcpWeight(const float& v) { mmf::check(mmf_fusion_set_icp_weight(f_, v), "setIcpWeight"); }
    void setOutlierCoefficient(const float& v) { mmf::check(mmf_fusion_set_outlier_coefficient(f_, v), "setOutlierCoefficient"); }
    void setPyramid(const bool& v) { mmf::check(mmf_fusion_set_pyramid(f_, v), "setPyramid"); }
    void setFastOdom(const bool& v) { mmf::check(mmf_fusion_set_fast_odom(f_, v), "setFastOdom"); }
    void setSo3(const bool& v) { mmf::check(mmf_fusion_set_so3(f_, v), "setSo3"); }
    void setFrameToFrameRGB(const bool& v) { mmf::check(mmf_fusion_set_frame_to_frame_rgb(f_, v), "setFrameToFrameRGB"); }
    void setConfidenceThreshold(const float& v) { mmf::check(mmf_fusion_set_confidence_threshold(f_, v), "setConfidenceThreshold"); }
    void setDepthCutoff(const float& v) { mmf::check(mmf_fusion_set_depth_cutoff(f_, v), "setDepthCutoff"); }
    void setEnableMultipleModels(bool v) { mmf::check(mmf_fusion_set_enable_multiple_models(f_, v), "setEnableMultipleModels"); }
    void setTick(const int& v) { mmf::check(mmf_fusion_set_tick(f_, v), "setTick"); }
    void scheduleDeactivation(const ModelPointer& m) { mmf::check(mmf_fusion_schedule_deactivation(f_, (int)m->getID()), "scheduleDeactivation"); }
    // settings of subsystems that stay in the reference's front-end (spawning policy beyond the CRF, redetection):
    // recorded, not interpreted here.  The CRF and spawn settings are recorded too and forwarded to the built-in
    // segmentation (mmf_fusion_set_crf_segmentation).
    // fernThresh: recorded, and handed to the fern database while that hook is on (setFernDatabase)
    void setFernThresh(const float& v) {
        other_["fernThresh"] = v;
        if (fern_on_) mmf::check(mmf_ferns_set_threshold(mmf_fusion_fern_database(f_), v), "mmf_ferns_set_threshold");
    }
    // The fern keyframe database behind every frame's final predict(), where the reference's processFerns() stands
    // (MultiMotionFusion.cpp:824; mmf_fusion_set_fern_database): ferns(500, depthCut * 1000, ..) (:33) with the
    // recorded fernThresh, on the camera model's fill-in images.  Observational -- stage one of relocalisation: no pose, map or
    // mask depends on it, getLost() stays false.  Off until switched on; setFernDatabase(true) again starts an empty database.
    void setFernDatabase(bool v) {
        mmf_ferns_config c;
        mmf::check(mmf_ferns_default_config(&c), "mmf_ferns_default_config");
        const int depth_mm = (int)(refresh().depth_cutoff * 1000.f);
        c.max_depth_mm = depth_mm > 400 ? depth_mm : 400;
        if (other_.count("fernThresh")) c.threshold = other_["fernThresh"];
        ferns_.reset();
        mmf::check(mmf_fusion_set_fern_database(f_, v ? &c : nullptr, nullptr), "mmf_fusion_set_fern_database");
        other_["fernDatabase"] = v, fern_on_ = v;
        if (v) ferns_.reset(new Ferns(mmf_fusion_fern_database(f_), width_, height_, c.num, c.max_depth_mm));
    }
    // getFerns() (MultiMotionFusion.h:106): the hook's database; only while the hook is on
    Ferns& getFerns() {
        if (!ferns_) mmf::check(MMF_ERR_STATE, "getFerns: the fern database is off (setFernDatabase)");
        return *ferns_;
    }
    // the database's record of the last frame (mmf_fusion_last_fern_result); `valid` false while the hook is off and before
    // the first frame
    struct FernResult {
        bool valid = false;
        mmf_ferns_result_t record{};
    };
    FernResult getLastFernResult() {
        FernResult out;
        if (!fern_on_) return out;
        const int rc = mmf_fusion_last_fern_result(f_, &out.record);
        if (rc == MMF_ERR_STATE) return out;
        mmf::check(rc, "mmf_fusion_last_fern_result");
        out.valid = true;
        return out;
    }
    void setModelSpawnOffset(const unsigned& v) {
        other_["modelSpawnOffset"] = (float)v, crf_.model_spawn_offset = (int)v, mask_.model_spawn_offset = (int)v;
        flowseg_.model_spawn_offset = (int)v;
        pushCrf(), pushMask(), pushFlowSeg();
    }
    void setModelDeactivateCount(const unsigned& v) { other_["modelDeactivateCount"] = (float)v; }
    void setCrfPairwiseSigmaRGB(const float& v) { other_["crfPairwiseSigmaRGB"] = v, crf_.sigma_rgb = v, pushCrf(); }
    void setCrfPairwiseSigmaPosition(const float& v) { other_["crfPairwiseSigmaPosition"] = v, crf_.sigma_pos = v, pushCrf(); }
    void setCrfPairwiseSigmaDepth(const float& v) { other_["crfPairwiseSigmaDepth"] = v, crf_.sigma_depth = v, pushCrf(); }
    void setCrfPairwiseWeightAppearance(const float& v) { other_["crfPairwiseWeightAppearance"] = v, crf_.weight_appearance = v, pushCrf(); }
    void setCrfPairwiseWeightSmoothness(const float& v) { other_["crfPairwiseWeightSmoothness"] = v, crf_.weight_smoothness = v, pushCrf(); }
    void setCrfThresholdNew(const float& v) { other_["crfThresholdNew"] = v, crf_.threshold_new = v, pushCrf(); }
    void setCrfUnaryWeightError(const float& v) { other_["crfUnaryWeightError"] = v, crf_.unary_weight_error = v, pushCrf(); }
    void setCrfIteration(const unsigned& v) { other_["crfIteration"] = (float)v, crf_.iterations = (int)v, pushCrf(); }
    void setCrfUnaryKError(const float& v) { other_["crfUnaryKError"] = v, crf_.unary_k_error = v, pushCrf(); }
    void setNewModelMinRelativeSize(const float& v) { other_["newModelMinRelativeSize"] = v, crf_.min_rel_size_new = v, pushCrf(); }
    void setNewModelMaxRelativeSize(const float& v) { other_["newModelMaxRelativeSize"] = v, crf_.max_rel_size_new = v, pushCrf(); }
    // the built-in segmentation's super-pixels from the frame's RGB on the device (the engine that replaces gSLICr,
    // cpp/Slic.h) instead of the regular grid; sp_size must divide the frame size
    void setSuperpixelEngine(bool v) { other_["superpixelEngine"] = v, mmf::check(mmf_fusion_set_superpixel_engine(f_, v ? 1 : 0), "mmf_fusion_set_superpixel_engine"); }
    // Every frame's dense optical flow from the frame before it (the flow stage of "flow_crf", Segmentation.cpp:779-804:
    // Farneback on the pair scaled down by four, the reference's settings), computed beside the tracking; off until
    // switched on (SegmentationConfiguration::mode == "flow_crf" switches it on).  getLastFlow(): the last frame's
    // field in host memory, `valid` false after the first frame of a sequence (creation, reset) and while the hook is off.
    struct OpticalFlow {
        bool valid = false;
        int width = 0, height = 0;            // the flow image: the frame's size / 4
        std::vector<float> flow;              // [height][width][2] = {x, y}: prev(y, x) ~ next(y + flow.y, x + flow.x)
        std::vector<float> magnitude, motion; // [height][width]; motion = clamp((magnitude - 0.2) / 4.8, 0, 1) (:1193-1197)
    };
    void setOpticalFlow(bool v) {
        mmf_flow_config c;
        mmf::check(mmf_flow_default_config(&c), "mmf_flow_default_config");
        mmf::check(mmf_fusion_set_optical_flow(f_, v ? &c : nullptr), "mmf_fusion_set_optical_flow");
        other_["opticalFlow"] = v, flow_on_ = v;
        // (the inference reads the flow: off with it; setOpticalFlow(true) again replaces the flow engine -- a new sequence --
        // and the library switches the inference back on with it, so the flag stands)
        if (!v && flow_inference_on_) other_["flowInference"] = false, flow_inference_on_ = false;
        flow_seg_on_ = false;  // (the library ends the flow_crf mode with the flow engine it read)
    }
    OpticalFlow getLastFlow() {
        OpticalFlow out;
        if (!flow_on_) return out;
        const float *flow = nullptr, *magnitude = nullptr, *motion = nullptr;
        int has = 0;
        mmf::check(mmf_fusion_last_flow(f_, &flow, &magnitude, &motion, &out.width, &out.height, &has), "mmf_fusion_last_flow");
        if (!has) return out;
        mmf::check(mmf_ctx_synchronize(ctx_), "mmf_ctx_synchronize");  // (the fusion's stream has joined the flow's)
        const size_t px = (size_t)out.width * out.height;
        out.flow.resize(2 * px), out.magnitude.resize(px), out.motion.resize(px);
        if (hipMemcpy(out.flow.data(), flow, 2 * px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out.magnitude.data(), magnitude, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out.motion.data(), motion, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            mmf::check(MMF_ERR_HIP, "getLastFlow: download");
        out.valid = true;
        return out;
    }
    // The inference of flow_crf (Segmentation.cpp:819-1263; mmf_fusion_set_flow_inference) on every tracked frame
    // that has a flow; it needs setOpticalFlow(true).  Observational: the id image is handed out, the models do not use it.
    // getLastFlowInference(): the last frame's id images in host memory, `valid` false after the first frame of a sequence,
    // after a frame that was not tracked and while the hook is off.
    struct FlowInference {
        bool valid = false;
        int width = 0, height = 0, labels = 0;  // the CRF image: the frame's size / 4
        std::vector<unsigned char> ids;       // [height][width] model ids (the new label's: the next model id)
        std::vector<unsigned char> ids_full;  // [4 height][4 width]: the same scaled up by 4
    };
    void setFlowInference(bool v) {
        mmf_flowcrf_config c;
        mmf::check(mmf_flowcrf_default_config(&c), "mmf_flowcrf_default_config");
        mmf::check(mmf_fusion_set_flow_inference(f_, v ? &c : nullptr), "mmf_fusion_set_flow_inference");
        other_["flowInference"] = v, flow_inference_on_ = v;
        if (!v) flow_seg_on_ = false;
    }
    // What the flow_crf mode (SegmentationConfiguration::mode == "flow_crf"; mmf_fusion_set_flow_segmentation)
    // made of the last frame it segmented: the SegmentationResult's model data, hasNewLabel as processFrame used it, and per
    // label the winning blob.  `valid` false while the mode is off and before its first frame; `has_result` false for a frame
    // without an inference result (a zero mask, no entries).
    struct FlowSegmentation {
        bool valid = false, has_result = false;
        mmf_flowseg_summary summary{};
    };
    FlowSegmentation getLastFlowSegmentation() {
        FlowSegmentation out;
        if (!flow_seg_on_) return out;
        int has = 0;
        if (mmf_fusion_last_flow_segmentation(f_, &out.summary, &has) != MMF_OK) return out;  // (no frame yet)
        out.valid = true, out.has_result = has != 0;
        return out;
    }
    FlowInference getLastFlowInference() {
        FlowInference out;
        if (!flow_inference_on_) return out;
        const uint8_t *ids = nullptr, *full = nullptr;
        int has = 0;
        mmf::check(mmf_fusion_last_flow_inference(f_, &ids, &full, &out.width, &out.height, &out.labels, &has), "mmf_fusion_last_flow_inference");
        if (!has) return out;
        mmf::check(mmf_ctx_synchronize(ctx_), "mmf_ctx_synchronize");  // (the fusion's stream has joined the flow's)
        const size_t px = (size_t)out.width * out.height;
        out.ids.resize(px), out.ids_full.resize(16 * px);
        if (hipMemcpy(out.ids.data(), ids, px, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out.ids_full.data(), full, 16 * px, hipMemcpyDeviceToHost) != hipSuccess)
            mmf::check(MMF_ERR_HIP, "getLastFlowInference: download");
        out.valid = true;
        return out;
    }
    // redetection of inactive models by their stored keypoint views (:489-559), inside processFrame; off until switched on
    void setEnableRedetection(bool v) { other_["enableRedetection"] = v, mmf::check(mmf_fusion_set_redetection(f_, v ? 1 : 0), "mmf_fusion_set_redetection"); }
    // where the redetection candidates are verified: 0 = host (default), 1 = device, a fresh RigidRANSAC per view (mmf_hip.h)
    void setRedetectionVerifier(int mode) { mmf::check(mmf_fusion_set_redetection_verifier(f_, mode), "mmf_fusion_set_redetection_verifier"); }
    int getRedetectionHostVerified() { return mmf_fusion_redetection_host_verified(f_); }
    // the last keypoint of every visible track (track->back(), :428-436) for the next processFrame: xy [n][2] pixels,
    // coordinate [n][3] camera frame, descriptor [n][256]
    void setKeypoints(int n, const int* xy, const float* coordinate, const float* descriptor) {
        mmf::check(mmf_fusion_set_keypoints(f_, n, xy, coordinate, descriptor), "mmf_fusion_set_keypoints");
    }
    std::vector<mmf_redetection> getLastRedetections() {
        int n = 0;
        mmf::check(mmf_fusion_last_redetections(f_, nullptr, 0, &n), "mmf_fusion_last_redetections");
        std::vector<mmf_redetection> out((size_t)n);
        if (n) mmf::check(mmf_fusion_last_redetections(f_, out.data(), n, &n), "mmf_fusion_last_redetections");
        return out;
    }
    // what the last processFrame stored when a model left the active list (a tracker with a view log, redetection on)
    struct StoredViews {
        int model_id, n_views, rows;
    };
    std::vector<StoredViews> getLastStoredViews() {
        int n = 0;
        mmf::check(mmf_fusion_last_stored_views(f_, nullptr, nullptr, nullptr, 0, &n), "mmf_fusion_last_stored_views");
        std::vector<int> ids((size_t)n), views((size_t)n), rows((size_t)n);
        if (n) mmf::check(mmf_fusion_last_stored_views(f_, ids.data(), views.data(), rows.data(), n, &n), "mmf_fusion_last_stored_views");
        std::vector<StoredViews> out;
        for (int k = 0; k < n; ++k) out.push_back(StoredViews{ids[(size_t)k], views[(size_t)k], rows[(size_t)k]});
        return out;
    }
    // refineTrackSubset(segm_tracks[uid], globalModel, 2) (:596-599) inside processFrame: history 0 = off (the default), the
    // reference's value is 2.  The frame that spawns a model back-dates its poses from the tracks of its segment (an attached
    // tracker with a view log); with redetection on the views it stores on deactivation reach back before the spawn.  The
    // model's pose is not overridden.
    void setTrackBackdating(int history) { mmf::check(mmf_fusion_set_track_backdating(f_, history), "mmf_fusion_set_track_backdating"); }
    // what the last processFrame back-dated: the model's id (-1: nothing) and its entries, oldest first
    std::vector<mmf_backdated_pose> getLastBackdatedPoses(int* modelId = nullptr) {
        int n = 0, id = -1;
        mmf::check(mmf_fusion_last_backdated_poses(f_, &id, nullptr, 0, &n), "mmf_fusion_last_backdated_poses");
        std::vector<mmf_backdated_pose> out((size_t)n);
        if (n) mmf::check(mmf_fusion_last_backdated_poses(f_, &id, out.data(), n, &n), "mmf_fusion_last_backdated_poses");
        if (modelId) *modelId = id;
        return out;
    }
    // ----- keypoint tracks (MultiMotionFusion.h:307-309, 366; .cpp:223-248, 312-335): with a predictor set, processFrame(FrameData)
    // runs getFeatures on the frame, adds its keypoints to the tracker (0.7, 30) and prunes it (30, 1 s) before the library
    // call, which initialises every model from its own tracks when odom_cfg.init == "kp" and keeps the models' track sets
    void setOdomInit(const std::string& init) { odom_cfg_.init = init, pushTracker(); }  // "kp" or ""
    void setOdomRefine(bool icp_refine) { odom_cfg_.icp_refine = icp_refine, pushTracker(); }
    // not owned; nullptr detaches the tracker.  max_tracks bounds the table (dropped appends are counted: getTracker()->dropped())
    void setKeypointPredictor(SuperPoint* predictor, int max_tracks = 4096, int max_keypoints = 4096) {
        kp_predictor_ = predictor;
        if (predictor && !tracker_)
            tracker_.reset(new tracker::PointTracker(ctx_, width_, height_, fx_, fy_, cx_, cy_, max_tracks, max_keypoints));
        pushTracker();
    }
    tracker::PointTracker* getTracker() { return tracker_.get(); }
    // not in the reference: with it on, features, add and prune run INSIDE the library call on the frame it uploads (once),
    // enqueued and not awaited (mmf_fusion_set_keypoint_frontend); addFrameKeypoints -- its wait, its second upload and
    // the conversions to double and back -- is skipped.  The predictor must return no more keypoints than max_keypoints.
    void setKeypointFrontEndOnDevice(bool v) { kp_on_device_ = v, pushTracker(); }
    // the transformations the last frame's models were initialised with, list order (row-major 4x4 each)
    std::vector<float> getLastTrackTransforms() {
        int n = 0;
        mmf::check(mmf_fusion_last_track_transforms(f_, nullptr, 0, &n), "mmf_fusion_last_track_transforms");
        std::vector<float> out((size_t)n * 16);
        if (n) mmf::check(mmf_fusion_last_track_transforms(f_, out.data(), n, &n), "mmf_fusion_last_track_transforms");
        return out;
    }
    void setSetInhibit(bool v) {
        other_["inhibitModels"] = v, crf_.inhibit_new = v ? 1 : 0, mask_.inhibit_new = v ? 1 : 0, flowseg_.inhibit_new = v ? 1 : 0;
        pushCrf(), pushMask(), pushFlowSeg();
    }
    // not in the reference, where a frame with a mask always takes this branch (Segmentation.cpp:89): with it on,
    // FrameData::mask / FrameDataDevice::mask are RAW labels; processFrame maps them to model ids through a table it keeps,
    // spawns a model for the raster-first new label (modelSpawnOffset, inhibitModels) and computes the model data
    // (unseen counts, confidence 0.4, max depth).  Off (default): the mask is an id image mapped by the caller.
    void setMaskSegmentation(bool v) { mask_on_ = v, other_["maskSegmentation"] = v, pushMask(true); }
    std::vector<uint8_t> getMaskMapping() {
        std::vector<uint8_t> out(256);
        mmf::check(mmf_fusion_mask_mapping(f_, out.data()), "mmf_fusion_mask_mapping");
        return out;
    }
    void setEnableSmartModelDelete(bool v) { other_["enableSmartModelDelete"] = v; }
    const std::map<std::string, float>& frontEndSettings() const { return other_; }

    // ----- getters (:186-216)
    const bool& getLost() { return lost_; }  // loss detection and pose recovery stay in the reference: never lost here
    int getTick() const { return mmf_fusion_tick(f_); }
    int getTimeDelta() { return refresh().time_delta; }
    float getMaxDepthProcessed() { return refresh().max_depth_processed; }
    void getCurrPose(float pose[16]) const { mmf::check(mmf_fusion_get_pose(f_, pose), "mmf_fusion_get_pose"); }
    void exportPoses(const std::string& exportDir = "") {  // (the reference writes into the constructor's exportDirectory)
        mmf::check(mmf_fusion_export_poses(f_, (exportDir.empty() ? exportDirectory_ : exportDir).c_str()), "mmf_fusion_export_poses");
    }
    // savePly() (:1001-1018) into the constructor's exportDirectory: cloud-<id>.ply per model and the model database under
    // model_db/ (mmf_fusion_save_models); loadModels() (:131-145, -restore) from the same place -> the models restored
    void savePly() { mmf::check(mmf_fusion_save_models(f_, exportDirectory_.c_str()), "mmf_fusion_save_models"); }
    // setRestoreDense(true) (ours, default false): loadModels() also restores every model's surfels from its cloud.ply
    void setRestoreDense(bool val) { restoreDense_ = val; }
    int loadModels() {
        int n = 0;
        mmf::check(mmf_fusion_load_models_ex(f_, exportDirectory_.c_str(), restoreDense_ ? MMF_LOAD_DENSE : 0u, &n), "mmf_fusion_load_models");
        return n;
    }
    mmf_odom* getFrameOdometryHandle() { return mmf_fusion_odometry(f_); }
    mmf_fusion* handle() const { return f_; }

   private:
    bool finish(int rc, const char* what) {
        if (rc == MMF_ERR_INVALID) {
            std::fprintf(stderr, "%s\n", mmf_last_error());
            return false;
        }
        mmf::check(rc, what);
        return false;
    }
    void pushCrf() {
        mmf::check(mmf_fusion_set_crf_segmentation(f_, segm_cfg_.mode.empty() ? &crf_ : nullptr), "mmf_fusion_set_crf_segmentation");
    }
    void pushFlowSeg() {
        if (segm_cfg_.mode != "flow_crf" || !flow_inference_on_) return;
        mmf::check(mmf_fusion_set_flow_segmentation(f_, &flowseg_), "mmf_fusion_set_flow_segmentation");
        flow_seg_on_ = true;
    }
    void pushTracker() {
        other_["odomInitKp"] = odom_cfg_.init == "kp", other_["hasKeypointPredictor"] = kp_predictor_ != nullptr;
        mmf::check(mmf_fusion_set_tracker(f_, kp_predictor_ && tracker_ ? tracker_->handle() : nullptr, odom_cfg_.init == "kp" ? 1 : 0,
                                          odom_cfg_.icp_refine ? 1 : 0),
                   "mmf_fusion_set_tracker");
        other_["keypointFrontEndOnDevice"] = kp_on_device_;
        if (kp_on_device_ && kp_predictor_ && tracker_) {  // (set_tracker switched it off)
            mmf_keypoint_frontend_config k;
            mmf::check(mmf_keypoint_frontend_default_config(&k), "mmf_keypoint_frontend_default_config");
            mmf::check(mmf_fusion_set_keypoint_frontend(f_, kp_predictor_->handle(), &k), "mmf_fusion_set_keypoint_frontend");
        }
    }
    // MultiMotionFusion.cpp:223-248 at level 0: the frame's features into the tracker (device copies of rgb and depth of its own)
    bool addFrameKeypoints(const FrameData& frame) {
        const size_t npix = (size_t)width_ * height_;
        if (!kp_rgb_ && (hipMalloc(reinterpret_cast<void**>(&kp_rgb_), npix * 3) != hipSuccess ||
                         hipMalloc(reinterpret_cast<void**>(&kp_depth_), npix * sizeof(float)) != hipSuccess)) {
            std::fprintf(stderr, "MultiMotionFusion: hipMalloc of the keypoint images failed\n");
            return false;
        }
        mmf::check(mmf_ctx_synchronize(ctx_), "mmf_ctx_synchronize");  // (the last frame's add has read the depth copy)
        if (hipMemcpy(kp_rgb_, frame.rgb, npix * 3, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(kp_depth_, frame.depth, npix * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "MultiMotionFusion: upload of the keypoint images failed\n");
            return false;
        }
        std::vector<double> coordinates, descriptors;
        std::tie(coordinates, descriptors) = kp_predictor_->getFeatures(kp_rgb_, width_, height_, 3);
        tracker_->addKeypoints(coordinates, descriptors, frame.timestamp, kp_depth_, 0.7f, 30);
        const int64_t old = (int64_t)frame.timestamp - 1000000000LL;
        tracker_->prune(30, (uint64_t)(old > 0 ? old : 0));  // tracks older than 1 s with fewer than 30 keypoints (:246)
        return true;
    }
    void pushMask(bool always = false) {  // (the settings are pushed while the mode is on)
        if (mask_on_ || always) mmf::check(mmf_fusion_set_mask_segmentation(f_, mask_on_ ? &mask_ : nullptr), "mmf_fusion_set_mask_segmentation");
    }
    const mmf_fusion_config& refresh() {
        mmf::check(mmf_fusion_get_config(f_, &cfg_), "mmf_fusion_get_config");
        return cfg_;
    }
    mmf_fusion* f_ = nullptr;
    mmf_fusion_config cfg_;
    int width_, height_;
    mmf_ctx* ctx_ = nullptr;
    float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
    SuperPoint* kp_predictor_ = nullptr;
    bool kp_on_device_ = false;
    bool flow_on_ = false;
    bool flow_inference_on_ = false;
    bool flow_seg_on_ = false;
    bool fern_on_ = false;
    std::unique_ptr<Ferns> ferns_;  // a view of the hook's engine
    mmf_flowseg_config flowseg_{};
    std::unique_ptr<tracker::PointTracker> tracker_;
    unsigned char* kp_rgb_ = nullptr;
    float* kp_depth_ = nullptr;
    OdometryConfig odom_cfg_;
    SegmentationConfiguration segm_cfg_;
    std::string exportDirectory_;
    bool restoreDense_ = false;
    ModelList models_, inactive_;
    std::map<std::string, GPUTexture*> textures_;
    std::map<std::string, float> other_;
    mmf_crf_config crf_;
    mmf_mask_config mask_ = {22, 0};  // (mmf_mask_default_config)
    bool mask_on_ = false;
    bool lost_ = false;
    FrameData next_;
};
