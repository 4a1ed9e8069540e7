/*
 * mmf_hip.h -- C ABI of the MI355X (gfx950) dense-tracking hot path of MultiMotionFusion.
 *
 * This is the drop-in boundary: plain C, raw device/host pointers and sizes, no C++ / torch /
 * Eigen / OpenCV types.  Each entry point names the reference interface it replaces
 * (paths relative to the reference tree).  The C++ shim classes with the reference's own
 * names (multimotionfusion_amd/cpp/) and the Python ctypes mirror
 * (multimotionfusion_amd/_capi.py) are thin forwards onto this header.
 *
 * Conventions
 *   - every `*_dev` / "device" pointer is HBM memory of the context's device; everything else
 *     is host memory.  2-D images are passed as (pointer, step_bytes) like the reference's
 *     DeviceArray2D / PtrStep (Core/Cuda/containers/kernel_containers.hpp:48-91); step 0
 *     means dense (step = cols * sizeof(element)).
 *   - vertex / normal maps are planar float32 [3*rows][cols] (x plane, y plane, z plane;
 *     Core/Cuda/reduce.cu:261-263), invalid = NaN in the x plane.
 *   - 3x3 matrices are row major float[9] (types.cuh:61-73), poses row major float[16].
 *   - all work is enqueued on the context's stream; functions that return results in host
 *     memory synchronise that stream before returning (the reference's *Step functions do the
 *     same, reduce.cu:452-456); the others are asynchronous on the stream -- call
 *     mmf_ctx_synchronize() (the reference relies on the default stream's ordering).
 *   - return value: MMF_OK (0) or a negative mmf_status; mmf_last_error() gives the message for
 *     the calling thread.  (The reference prints and exit(-1)s, convenience.cuh:74-83; the C++
 *     shims reproduce that on a non-zero status.)
 */
#ifndef MMF_HIP_H_
#define MMF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_ABI_VERSION 3

typedef enum {
    MMF_OK = 0,
    MMF_ERR_INVALID = -1, /* bad argument (null pointer, size, alignment) */
    MMF_ERR_HIP = -2,     /* a HIP runtime call failed                     */
    MMF_ERR_NO_DEVICE = -3,
    MMF_ERR_STATE = -4 /* call order violated (e.g. initRGB before initICP) */
} mmf_status;

typedef struct mmf_ctx mmf_ctx;   /* device + stream + reduction scratch              */
typedef struct mmf_odom mmf_odom; /* replaces class RGBDOdometry (RGBDOdometry.h:31)  */

/* types.cuh:75-81 (DataTerm), 16 bytes */
typedef struct {
    int16_t zero_x, zero_y;
    int16_t one_x, one_y;
    float diff;
    uint8_t valid;
    uint8_t pad_[3];
} mmf_dataterm;

/* types.cuh:83-99 (CameraModel) */
typedef struct {
    float fx, fy, cx, cy;
} mmf_camera;

int mmf_abi_version(void);
const char *mmf_last_error(void);

/* private_stream != 0: create and own a non-blocking stream (`stream` is ignored).
 * private_stream == 0: run on the caller's hipStream_t `stream`; NULL is the device's default
 * (null) stream, which is what the reference uses throughout. */
int mmf_ctx_create(int device, void *stream, int private_stream, mmf_ctx **out);
void mmf_ctx_destroy(mmf_ctx *ctx);
int mmf_ctx_synchronize(mmf_ctx *ctx);
void *mmf_ctx_stream(mmf_ctx *ctx);
/* name of the device the context runs on, e.g. "gfx950:sramecc+:xnack-" */
int mmf_ctx_device_name(mmf_ctx *ctx, char *buf, size_t buflen);

/* ---------------------------------------------------------------------------------------
 * Device entry points: one per host function of Core/Cuda/cudafuncs.cuh:64-193.
 * (`pyrDown(ushort)` cudafuncs.cuh:167 has no caller in the reference and is not provided.)
 * `threads, blocks` of the reference signatures are chosen internally for gfx950.
 * ------------------------------------------------------------------------------------- */

/* icpStep, cudafuncs.cuh:64-82 / reduce.cu:399-473.
 * A_host[36] row major symmetric, b_host[6], residual_host[2] = {sum r^2, inliers}.
 * err_map_dev: optional cols x rows float32 image standing in for icpErrorSurface. */
int mmf_icp_step(mmf_ctx *ctx, const float Rcurr[9], const float tcurr[3], const float *vmap_curr,
                 size_t vmap_curr_step, const float *nmap_curr, size_t nmap_curr_step,
                 const float Rprev_inv[9], const float tprev[3], const mmf_camera *intr,
                 const float *vmap_g_prev, size_t vmap_g_prev_step, const float *nmap_g_prev,
                 size_t nmap_g_prev_step, float dist_thres, float angle_thres, int cols, int rows,
                 float *A_host, float *b_host, float *residual_host, float *err_map_dev,
                 size_t err_map_step);

/* computeRgbResidual, cudafuncs.cuh:113-132 / reduce.cu:867-945.  last/next masks are not
 * read by the reference (MASK_RGB_RESIDUAL undefined) and are not taken. */
int mmf_compute_rgb_residual(mmf_ctx *ctx, float min_scale, const int16_t *dIdx, size_t dIdx_step,
                             const int16_t *dIdy, size_t dIdy_step, const float *last_depth,
                             size_t last_depth_step, const float *next_depth,
                             size_t next_depth_step, const uint8_t *last_image,
                             size_t last_image_step, const uint8_t *next_image,
                             size_t next_image_step, mmf_dataterm *corres_dev,
                             float max_depth_delta, const float kt[3], const float krkinv[9],
                             int cols, int rows, int *sigma_sum_host, int *count_host,
                             float *err_map_dev, size_t err_map_step);

/* rgbStep, cudafuncs.cuh:84-97 / reduce.cu:609-661.  cloud = AoS float3 (dense). */
int mmf_rgb_step(mmf_ctx *ctx, const mmf_dataterm *corres_dev, float sigma, const float *cloud_dev,
                 float fx, float fy, const int16_t *dIdx, size_t dIdx_step, const int16_t *dIdy,
                 size_t dIdy_step, float sobel_scale, int cols, int rows, float *A_host,
                 float *b_host);

/* so3Step, cudafuncs.cuh:99-110 / reduce.cu:1092-1150.  A_host[9], b_host[3], residual[2]. */
int mmf_so3_step(mmf_ctx *ctx, const uint8_t *last_image, size_t last_image_step,
                 const uint8_t *next_image, size_t next_image_step, const float image_basis[9],
                 const float kinv[9], const float krlr[9], int cols, int rows, float *A_host,
                 float *b_host, float *residual_host);

/* createVMap / createNMap, cudafuncs.cuh:134-142 / cudafuncs.cu:136-205 (mask unused, :119) */
int mmf_create_vmap(mmf_ctx *ctx, const mmf_camera *intr, const float *depth, size_t depth_step,
                    int cols, int rows, float *vmap, size_t vmap_step, float depth_cutoff);
int mmf_create_nmap(mmf_ctx *ctx, const float *vmap, size_t vmap_step, int cols, int rows,
                    float *nmap, size_t nmap_step);
/* tranformMaps (sic), cudafuncs.cuh:144-149; src may equal dst */
int mmf_transform_maps(mmf_ctx *ctx, const float *vmap_src, const float *nmap_src, size_t src_step,
                       int cols, int rows, const float R[9], const float t[3], float *vmap_dst,
                       float *nmap_dst, size_t dst_step);
/* copyMaps, cudafuncs.cuh:151-154: RGBA32F interleaved (dense) -> planar */
int mmf_copy_maps(mmf_ctx *ctx, const float *vmap_rgba, const float *nmap_rgba, int cols, int rows,
                  float *vmap_dst, float *nmap_dst, size_t dst_step);
/* resizeVMap / resizeNMap, cudafuncs.cuh:156-160; output is (in_cols/2) x (in_rows/2) */
int mmf_resize_vmap(mmf_ctx *ctx, const float *in, size_t in_step, int in_cols, int in_rows,
                    float *out, size_t out_step);
int mmf_resize_nmap(mmf_ctx *ctx, const float *in, size_t in_step, int in_cols, int in_rows,
                    float *out, size_t out_step);
/* imageBGRToIntensity, cudafuncs.cuh:162-163; `channels` = 3 or 4 interleaved u8 */
int mmf_image_bgr_to_intensity(mmf_ctx *ctx, const uint8_t *img, size_t img_step, int channels,
                               int cols, int rows, uint8_t *dst, size_t dst_step);
/* verticesToDepth, cudafuncs.cuh:165-167; vmap_rgba dense RGBA32F */
int mmf_vertices_to_depth(mmf_ctx *ctx, const float *vmap_rgba, int cols, int rows, float cutoff,
                          float *dst, size_t dst_step);
/* projectToPointCloud, cudafuncs.cuh:170-173; cloud dense AoS float3 */
int mmf_project_to_point_cloud(mmf_ctx *ctx, const float *depth, size_t depth_step, int cols,
                               int rows, const mmf_camera *intr, int level, float *cloud);
/* pyrDownGaussF / pyrDownUcharGauss, cudafuncs.cuh:182-186; dst is (cols/2) x (rows/2) */
int mmf_pyr_down_gauss_f(mmf_ctx *ctx, const float *src, size_t src_step, int src_cols,
                         int src_rows, float *dst, size_t dst_step);
int mmf_pyr_down_uchar_gauss(mmf_ctx *ctx, const uint8_t *src, size_t src_step, int src_cols,
                             int src_rows, uint8_t *dst, size_t dst_step);
/* computeDerivativeImages, cudafuncs.cuh:191-193 */
int mmf_compute_derivative_images(mmf_ctx *ctx, const uint8_t *src, size_t src_step, int cols,
                                  int rows, int16_t *dx, size_t dx_step, int16_t *dy,
                                  size_t dy_step);

/* ---------------------------------------------------------------------------------------
 * RGBDOdometry (Core/Utils/RGBDOdometry.h:31-137).  GPUTexture* arguments of the reference
 * become dense device images; Eigen types become float arrays.
 * ------------------------------------------------------------------------------------- */
#define MMF_NUM_PYRS 3 /* RGBDOdometry.h:72 */

/* RGBDOdometry::RGBDOdometry, RGBDOdometry.h:34-36 (maskID is unused by the kernels) */
int mmf_odom_create(mmf_ctx *ctx, int width, int height, float cx, float cy, float fx, float fy,
                    float dist_thresh, float angle_thresh, mmf_odom **out);
void mmf_odom_destroy(mmf_odom *o);

/* Model::generateCUDATextures (Core/Model/Model.cpp:359-388): level-0 filtered depth ->
 * 3-level pyramid owned by the odometry object (returned for sharing between models). */
int mmf_odom_build_depth_pyramid(mmf_odom *o, const float *depth_l0, size_t step);
/* RGBDOdometry::initICP(depthPyramid, maskPyramid, cutoff), RGBDOdometry.h:41-43.  depth_pyr
 * may be NULL to use the pyramid built by mmf_odom_build_depth_pyramid. */
int mmf_odom_init_icp(mmf_odom *o, const float *const depth_pyr[MMF_NUM_PYRS],
                      const size_t steps[MMF_NUM_PYRS], float depth_cutoff);
/* RGBDOdometry::initICP(GPUTexture*,GPUTexture*,cutoff), RGBDOdometry.h:44 */
int mmf_odom_init_icp_from_prediction(mmf_odom *o, const float *vert_rgba, const float *norm_rgba,
                                      float depth_cutoff);
/* RGBDOdometry::initICPModel, RGBDOdometry.h:47 */
int mmf_odom_init_icp_model(mmf_odom *o, const float *vert_rgba, const float *norm_rgba,
                            float depth_cutoff, const float pose[16]);
/* RGBDOdometry::initRGB / initRGBModel / initFirstRGB, RGBDOdometry.h:49-53.
 * Must follow the matching initICP* call (RGBDOdometry.cpp:197,202). */
int mmf_odom_init_rgb(mmf_odom *o, const uint8_t *rgb, size_t step, int channels);
int mmf_odom_init_rgb_model(mmf_odom *o, const uint8_t *rgb, size_t step, int channels);
int mmf_odom_init_first_rgb(mmf_odom *o, const uint8_t *rgb, size_t step, int channels);

/* RGBDOdometry::getIncrementalTransformation, RGBDOdometry.h:56-58.
 * trans[3] / rot[9] in-out (host).  icp_err_dev / rgb_err_dev: width x height float32 device
 * images (dense) standing in for the two cudaSurfaceObject_t, or NULL.
 * The whole Gauss-Newton schedule runs device-resident (no host round trip per iteration);
 * the call returns after the stream has drained and trans/rot/stats are valid. */
int mmf_odom_get_incremental_transformation(mmf_odom *o, float trans[3], float rot[9],
                                            int rgb_only, float icp_weight, int pyramid,
                                            int fast_odom, int so3, float *icp_err_dev,
                                            float *rgb_err_dev);

/* public result members, RGBDOdometry.h:62-69 */
typedef struct {
    float lastICPError, lastICPCount, lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count;
    double lastA[36];
    double lastb[6];
    int iterations_run;
    int so3_iterations_run;
} mmf_odom_stats;
int mmf_odom_get_stats(mmf_odom *o, mmf_odom_stats *out);
/* RGBDOdometry::getCovariance, RGBDOdometry.h:60: inverse of lastA (6x6, row major) */
int mmf_odom_get_covariance(mmf_odom *o, double cov[36]);

/* Introspection for parity tests: device pointer of an internal pyramid buffer.
 * names: vmaps_curr nmaps_curr vmaps_g_prev nmaps_g_prev last_depth next_depth depth_pyr cloud
 *        last_image next_image last_next_image dIdx dIdy corres; for tests only (level ignored): extent (the 20 64-bit words of
 *        csrc/extent.hpp) and prep_box (two slots of four ints: the boxes an object model's last two boxed preparations stored) */
int mmf_odom_buffer(mmf_odom *o, const char *name, int level, void **dev_ptr, size_t *bytes);
/* synchronous copy of that buffer into host memory (host_bytes must equal its size) */
int mmf_odom_download(mmf_odom *o, const char *name, int level, void *host_dst, size_t host_bytes);

/* Timing hook for bench.py: enqueue `reps` back-to-back launches of the level-`level` ICP
 * reduction kernel on the odometry object's current maps and pose (no host work in
 * between), bracketed by HIP events on the context's stream; returns the mean time per launch.
 * variant: must be 0 (the shipped launch geometry); any other value returns MMF_ERR_INVALID. */
int mmf_odom_time_icp_kernel(mmf_odom *o, int level, int reps, int variant, float *mean_us_out);
/* Measurement mode for bench.py: while on, every launch of the Gauss-Newton loop's two kernels -- the producer
 * (ICP J^T J reduction + photometric correspondence pass of one iteration) and the photometric Jacobian /
 * solve step -- carries its own start / stop HIP events (the dispatch's begin / end timestamps, the same
 * ones a kernel trace reports), and the whole chain of a getIncrementalTransformation two more.  Sums, minima and
 * launch counts accumulate per pyramid level until the mode is switched (which also clears them). */
typedef struct {
    double producer_us_sum[MMF_NUM_PYRS], producer_us_min[MMF_NUM_PYRS];
    double rgb_step_us_sum[MMF_NUM_PYRS], rgb_step_us_min[MMF_NUM_PYRS];
    int producer_launches[MMF_NUM_PYRS], rgb_step_launches[MMF_NUM_PYRS];
    double chain_us_sum; /* odom_begin .. last step of one tracking call, on the device */
    int chains;
} mmf_odom_timing;
int mmf_odom_enable_timing(mmf_odom *o, int mode); /* 0 off, 1 the chain only (two events per call), 2 every kernel too */
int mmf_odom_get_timing(mmf_odom *o, mmf_odom_timing *out);

/* ---------------------------------------------------------------------------------------
 * Surfel model: Core/Model/Model.{h,cpp} (store, fuse, clean, initialise) and
 * Core/Model/ModelProjection.{h,cpp} (index map, splat prediction), without OpenGL.
 * The surfel store is a structure of float4 arrays in HBM; "textures" are dense device images.
 * All images are cols x rows, dense; rgb is interleaved u8 x 3 as uploaded from FrameData.rgb,
 * depth is float32 metres (0 = invalid), mask is u8.
 * ------------------------------------------------------------------------------------- */
typedef struct mmf_model mmf_model; /* replaces class Model + its ModelProjection */

/* Model::Model (Model.h:120-130): id doubles as the mask value of the model's pixels;
 * conf_threshold = confGlobalInit (10) / confObjectInit (0.01); max_surfels 0 = 1024*1024
 * (Model::MAX_VERTICES, Model.cpp:119-126). */
int mmf_model_create(mmf_ctx *ctx, int width, int height, float cx, float cy, float fx, float fy,
                     unsigned char id, float conf_threshold, int max_surfels, mmf_model **out);
void mmf_model_destroy(mmf_model *m);
/* Model::overridePose / getPose (Model.h:196-205): row-major camera-to-world 4x4 */
int mmf_model_set_pose(mmf_model *m, const float pose[16]);
int mmf_model_get_pose(mmf_model *m, float pose[16]);
/* Model::lastCount (Model.h:227) */
int mmf_model_count(mmf_model *m, unsigned *count);

/* MultiMotionFusion::filterDepth (MultiMotionFusion.cpp:897-904, depth_bilateral_metric.frag) */
int mmf_filter_depth(mmf_ctx *ctx, const float *depth, int cols, int rows, float max_depth, float *out);

/* computeFeedbackBuffers + Model::initialise (MultiMotionFusion.cpp:197-205, Model.cpp:267-312) */
int mmf_model_initialise(mmf_model *m, const uint8_t *rgb, const float *depth_raw,
                         const float *depth_filtered, int time, float max_depth);
/* Model::predictIndices -> ModelProjection::predictIndices (ModelProjection.cpp:94-143) */
int mmf_model_predict_indices(mmf_model *m, int time, float depth_cutoff, int time_delta);
/* Model::combinedPredict(ACTIVE) -> ModelProjection::combinedPredict (ModelProjection.cpp:187-269) */
int mmf_model_combined_predict(mmf_model *m, float depth_cutoff, int time, int max_time, int time_delta);
/* ModelProjection::synthesizeDepth (ModelProjection.cpp:275-335, depth_splat.frag): the splat's depth
 * only, into the model's "depth" image (float32 metres, 0 where no surfel lands); conf_threshold is
 * an argument here as in the reference (MultiMotionFusion.cpp:809-810 passes initConfThresGlobal) */
int mmf_model_synthesize_depth(mmf_model *m, float depth_cutoff, float conf_threshold, int time, int max_time,
                               int time_delta);
/* Model::fuse (Model.cpp:893-1048); weighting = Model::computeFusionWeight(weightMultiplier) */
int mmf_model_fuse(mmf_model *m, int time, const uint8_t *rgb, const uint8_t *mask, const float *depth_raw,
                   const float *depth_filtered, float depth_cutoff, float weighting);
/* Model::clean (Model.cpp:1050-1182); outlier_coeff = GPUSetup::outlierCoefficient (GUI default 3) */
int mmf_model_clean(mmf_model *m, int time, int time_delta, float depth_cutoff, const float *depth_filtered,
                    const uint8_t *mask, float outlier_coeff);
/* Model::performFillIn (Model.cpp:1607-1616) and MultiMotionFusion::requiresFillIn (:877-895) */
int mmf_model_perform_fill_in(mmf_model *m, const uint8_t *rgb, const float *depth_filtered,
                              int frame_to_frame_rgb, int lost);
int mmf_model_requires_fill_in(mmf_model *m, float ratio, int *result);
/* Model::downloadMap (Model.cpp:1353-1384): count_out surfels of 12 floats
 * {x y z conf | colour24 unused initTime timestamp | nx ny nz radius} (Vertex::SIZE = 48) */
int mmf_model_download_map(mmf_model *m, float *host_aos, unsigned max_surfels, unsigned *count_out);
/* Model::getModel() (Model.h:297; OutputBuffer of Core/Model/Buffers.h:3-6): the surfel store as it stands, in place --
 * three device arrays of float4 {xyz, confidence}, {colour24, unused, initTime, timestamp}, {normal xyz, radius} and the
 * number of surfels; valid until this model's next fuse / clean / initialise. */
int mmf_model_surfel_arrays(mmf_model *m, const float **pos_conf, const float **colour_time, const float **normal_radius,
                            unsigned *count);
/* inverse of download (tests, -restore) */
int mmf_model_upload_map(mmf_model *m, const float *host_aos, unsigned count);
/* device image behind a GPUTexture getter (ModelProjection.h:52-77, Model.h:232-244).
 * names: index(u32) vertConf colorTime normRad (float4) -- sparse index map;
 *        image(rgba8) vertexConf normalRadius (float4) time(u16) -- splat prediction;
 *        fillVertex fillNormal (float4) fillImage (rgba8) -- fill-in */
int mmf_model_texture(mmf_model *m, const char *name, void **dev_ptr, size_t *bytes);
/* Model::setMaxDepth / setConfidenceThreshold / getConfidenceThreshold / getID (Model.h:222-230, 307) */
int mmf_model_set_max_depth(mmf_model *m, float max_depth);
int mmf_model_set_confidence_threshold(mmf_model *m, float conf_threshold);
float mmf_model_confidence_threshold(mmf_model *m);
int mmf_model_id(mmf_model *m);

/* ---------------------------------------------------------------------------------------
 * Orchestrator: MultiMotionFusion::processFrame / predict (Core/MultiMotionFusion.h:78-86,
 * .cpp:207-854, 863-875): the global (camera) model plus the object models of the `models` list, each
 * with its own RGBDOdometry, tracked / predicted / fused / cleaned per frame.  With
 * enable_multiple_models == 0 this is the static-scene configuration (all-zero mask, :268-275).
 * The segmentation RESULT is handed in per frame (mmf_segmentation: gSLICr + dense CRF of the reference's
 * front-end), pulled through a callback at the point where the reference calls performSegmentation (:412), computed
 * from the frame's raw label image (Segmentation.cpp:89-147: mmf_fusion_set_mask_segmentation, below) or by the built-in
 * dense CRF (mmf_fusion_set_crf_segmentation, below).  Of relocalisation the fern keyframe database is here
 * (mmf_fusion_set_fern_database, below: stage one, observational); pose recovery, loss detection and loop closure stay in the
 * reference's front-end.
 * Every model runs on its own stream ("lane"); every public call returns with the fusion's own
 * stream (the context's) ordered after all lanes.
 * ------------------------------------------------------------------------------------- */
typedef struct mmf_fusion mmf_fusion;

typedef struct {
    int time_delta;            /* MultiMotionFusion ctor timeDelta (GUI default 200) */
    float conf_global_init;    /* confGlobalInit, GUI default 10 */
    float icp_weight;          /* GUI default 10 */
    float depth_cutoff;        /* bilateral filter maxD, GUI default */
    float max_depth_processed; /* 20 (MultiMotionFusion.cpp:53) */
    int rgb_only, pyramid, fast_odom, so3, frame_to_frame_rgb;
    float outlier_coeff;       /* GPUSetup::outlierCoefficient, GUI default 3 */
    int fill_in;               /* global model is created with fill-in enabled */
    int max_surfels;           /* 0 = Model::MAX_VERTICES */
    float conf_object_init;    /* confObjectInit, GUI default 0.01 (-confO) */
    int enable_multiple_models; /* setEnableMultipleModels (MultiMotionFusion.h:262) */
    int preallocated_models;   /* preallocateModels(count) (:125-131; -a) */
    int error_recording;       /* Model(..., enableErrorRecording): per-model ICP / RGB error images */
    int pose_logging;          /* enablePoseLogging: Model::poseLog, exportPoses */
    int max_object_surfels;    /* capacity of an object model's store, 0 = max_surfels */
    int batch_tracking;        /* 1: the Gauss-Newton chains of all models of a frame run as ONE chain of launches with
                                  gridDim.y = model (default); 0: one chain per model on the model's own stream */
} mmf_fusion_config;

/* SegmentationResult (Core/Segmentation/Segmentation.h:32-70) as far as processFrame consumes it */
typedef struct {
    unsigned id;                /* ModelData::id */
    unsigned super_pixel_count; /* 0: the model was not seen in this frame (:607) */
    float avg_confidence;       /* raises the object's confidence threshold, capped at 9 (:616-620) */
    float depth_mean, depth_std; /* Model::setMaxDepth(depth_mean + 1.2 depth_std) (:409, :486, :586) */
} mmf_segmentation_model;

typedef struct {
    const uint8_t *mask;  /* DEVICE, width*height u8: fullSegmentation = model id per pixel */
    int has_new_label;    /* hasNewLabel: spawn an object model for the id mmf_fusion_next_model_id() (:469-487) */
    int n_models;         /* entries of model_data: the active models in list order, then the new label's */
    const mmf_segmentation_model *model_data; /* HOST; NULL: no max-depth / confidence / unseen updates -- or, with
                                                 mmf_fusion_set_mask_segmentation on, mask = RAW LABELS to be segmented */
} mmf_segmentation;

/* one processFrame call (MultiMotionFusion.h:78-80): FrameData + the optional arguments */
typedef struct {
    const uint8_t *rgb;  /* DEVICE u8 x 3 interleaved (FrameData::rgb) */
    const float *depth;  /* DEVICE float32 metres (FrameData::depth) */
    long long timestamp;
    const float *in_pose; /* HOST 4x4 or NULL */
    float weight_multiplier;
    int bootstrap;
    /* odom_cfg.init == "kp" (:312-384): one 4x4 (HOST) per active model in list order = the
     * RigidRANSAC transformation of Model::getLastTrackTransform; NULL = no pose initialisation */
    const float *init_transforms;
    int n_init_transforms;
    int icp_refine; /* odom_cfg.icp_refine */
    /* enable_multiple_models: the result of performSegmentation(frame) for THIS frame; NULL = ask the callback */
    const mmf_segmentation *segmentation;
    /* optional hint (both or neither): the buffers the NEXT processFrame call will be given.  Their sensor-side
     * preparation (mmf_fusion_prefetch_frame) is then enqueued inside this call, while the host waits for this frame's
     * pose, instead of by a separate call afterwards.  Same contract: the next call gets these buffers, unchanged. */
    const uint8_t *next_rgb;
    const float *next_depth;
} mmf_frame;

/* called where the reference calls performSegmentation (:412): every model of this frame has been tracked
 * (poses, ICP / RGB error images and predictions of the previous fusion are readable); fill *out. */
typedef int (*mmf_segmentation_fn)(void *user, mmf_fusion *f, const mmf_frame *frame, mmf_segmentation *out);

int mmf_fusion_default_config(mmf_fusion_config *cfg);
int mmf_fusion_create(mmf_ctx *ctx, int width, int height, float cx, float cy, float fx, float fy,
                      const mmf_fusion_config *cfg, mmf_fusion **out);
void mmf_fusion_destroy(mmf_fusion *f);
int mmf_fusion_preallocate_models(mmf_fusion *f, unsigned count); /* preallocateModels (:125-131) */
/* processFrame(frame, inPose, weightMultiplier, gt_pose, bootstrap): rgb = u8 x 3 interleaved and
 * depth = float32 metres, both already in HBM (the reference uploads FrameData to GL textures
 * here, :221,261); in_pose may be NULL.  Returns MMF_ERR_INVALID with "invalid image data" where
 * the reference returns false (:209-212). */
int mmf_fusion_process_frame(mmf_fusion *f, const uint8_t *rgb, const float *depth, long long timestamp,
                             const float *in_pose, float weight_multiplier, int bootstrap);
/* processFrame with every optional input (multiple models, pose initialisation of every model) */
int mmf_fusion_process_frame_ex(mmf_fusion *f, const mmf_frame *frame);
/* processFrame(const FrameData&) with the frame in HOST memory: rgb, depth and the optional id image
 * (mask_host != NULL: FrameData::mask, already mapped to model ids -- raw labels with
 * mmf_fusion_set_mask_segmentation on) are staged through pinned double buffers
 * and uploaded on the fusion's stream (:221, :261, :416). */
int mmf_fusion_process_frame_host(mmf_fusion *f, const uint8_t *rgb_host, const float *depth_host,
                                  const uint8_t *mask_host, int has_new_label, long long timestamp,
                                  const float *in_pose, float weight_multiplier, int bootstrap);
/* The same with the NEXT call's host frame announced (both pointers or neither; the next call must be given exactly these
 * pointers, contents unchanged): the host-memory form of mmf_frame::next_rgb / next_depth.  That frame is staged and
 * uploaded on a stream of its own while this frame is tracked, and its sensor-side preparation overlaps this frame's
 * fusion -- what a front-end that reads frames ahead (GUI/MainController.cpp:547-590: logReader->getNext()) gets for free. */
int mmf_fusion_process_frame_host_next(mmf_fusion *f, const uint8_t *rgb_host, const float *depth_host,
                                       const uint8_t *mask_host, int has_new_label, long long timestamp,
                                       const float *in_pose, float weight_multiplier, int bootstrap,
                                       const uint8_t *next_rgb_host, const float *next_depth_host);
/* processFrame with the tracker initialised from keypoint tracks: odom_cfg.init == "kp"
 * (MultiMotionFusion.cpp:312-384).  init_transform = RigidRANSAC::Result::transformation of
 * Model::getLastTrackTransform (row-major 4x4, mmf_ransac_estimate): the camera model's pose becomes
 * pose * init_transform (:331), the map is predicted / fused / cleaned once at that pose with
 * Model::computeFusionWeight(weight_multiplier) (:352-366, Model.cpp:918), then the dense tracker refines the
 * pose when icp_refine != 0 (:377-381; odom_cfg.icp_refine), else the initial pose is kept (:382-385).  On the
 * first frame (tick 1) the transformation is ignored, as in the reference.  Fails in frame-to-frame RGB mode (:370). */
int mmf_fusion_process_frame_init(mmf_fusion *f, const uint8_t *rgb, const float *depth, long long timestamp,
                                  const float *init_transform, int icp_refine, float weight_multiplier);
/* Overlap across frames: enqueue the work of the NEXT frame that depends on the sensor frame only -- the depth
 * filter, vertex / normal maps and the depth pyramid on one side stream; the intensity pyramid, the gradients and
 * the SO3 pre-alignment (last frame's image against this one's) on another -- where they run while the current
 * frame is still being fused.  The following
 * mmf_fusion_process_frame* call with the SAME rgb / depth pointers picks the results up instead of
 * recomputing them (same kernels, same bits); with other pointers the prefetch is discarded.  rgb / depth must
 * stay unchanged until that call.  Optional: without it every frame is processed on its own. */
int mmf_fusion_prefetch_frame(mmf_fusion *f, const uint8_t *rgb, const float *depth);
/* predict() (MultiMotionFusion.h:86, .cpp:863-875): re-render every model's prediction at its current pose */
int mmf_fusion_predict(mmf_fusion *f);
/* getCurrPose / getTick / setTick / getBackgroundModel / getModels (MultiMotionFusion.h:100-216) */
int mmf_fusion_reset(mmf_fusion *f); /* empty maps, identity poses, tick = 1, only the global model active */
int mmf_fusion_get_pose(mmf_fusion *f, float pose[16]);
int mmf_fusion_tick(mmf_fusion *f);
int mmf_fusion_set_tick(mmf_fusion *f, int tick);
mmf_model *mmf_fusion_model(mmf_fusion *f);   /* getBackgroundModel(), = getIndexMap()'s owner */
mmf_odom *mmf_fusion_odometry(mmf_fusion *f); /* its frameToModel */
int mmf_fusion_num_models(mmf_fusion *f);     /* getModels().size() */
mmf_model *mmf_fusion_model_at(mmf_fusion *f, int index);
mmf_odom *mmf_fusion_odometry_at(mmf_fusion *f, int index);
int mmf_fusion_num_inactive_models(mmf_fusion *f);
mmf_model *mmf_fusion_inactive_model_at(mmf_fusion *f, int index);
int mmf_fusion_next_model_id(mmf_fusion *f); /* getNextModelID(false): the id a new label must carry in the mask */
int mmf_fusion_schedule_deactivation(mmf_fusion *f, int id); /* scheduleDeactivation: applied at the next frame */
/* Model::getICPErrorTexture (which = 0) / getRGBErrorTexture (which = 1) of the index-th active model:
 * width*height float32, written by the last level-0 iteration of its tracking */
int mmf_fusion_error_texture(mmf_fusion *f, int index, int which, float **dev_ptr);
/* getTextures() (MultiMotionFusion.h:124): "RGB" (u8 x 3), "DEPTH_METRIC", "DEPTH_METRIC_FILTERED" (float32),
 * "MASK" (u8) of the current frame as device images */
int mmf_fusion_texture(mmf_fusion *f, const char *name, const void **dev_ptr, size_t *bytes);
const float *mmf_fusion_depth_filtered(mmf_fusion *f);
/* the runtime setters the front-end pushes every GUI tick (MultiMotionFusion.cpp:1064-1116,
 * GUI/MainController.cpp:641-670); they take effect at the next processFrame */
int mmf_fusion_set_rgb_only(mmf_fusion *f, int val);
int mmf_fusion_set_icp_weight(mmf_fusion *f, float val);
int mmf_fusion_set_outlier_coefficient(mmf_fusion *f, float val);
int mmf_fusion_set_pyramid(mmf_fusion *f, int val);
int mmf_fusion_set_fast_odom(mmf_fusion *f, int val);
int mmf_fusion_set_so3(mmf_fusion *f, int val);
int mmf_fusion_set_frame_to_frame_rgb(mmf_fusion *f, int val);
int mmf_fusion_set_depth_cutoff(mmf_fusion *f, float val);
int mmf_fusion_set_confidence_threshold(mmf_fusion *f, float val);
int mmf_fusion_set_enable_multiple_models(mmf_fusion *f, int val);
int mmf_fusion_get_config(mmf_fusion *f, mmf_fusion_config *out);
/* Per-rigid-body shard (one process per GPU): this process runs the GPU work of the models whose id has
 * id % world == rank (fixed when the model is created: a model leaving the list moves nobody else); the other models exist
 * as bookkeeping only (ids, thresholds, poses).  The sensor-side
 * preparation of a frame runs on every rank.  Poses of remote models are handed in by the caller (the all-gather
 * of mmf_shard_* or of the host framework). */
int mmf_fusion_set_shard(mmf_fusion *f, int rank, int world);
int mmf_fusion_owns_model(mmf_fusion *f, int index);
int mmf_fusion_set_model_pose(mmf_fusion *f, int index, const float pose[16]);
/* The shard's two exchanges over RCCL, for a front-end that runs one process per GPU (the reference is
 * single GPU and walks its Model list serially, MultiMotionFusion.cpp:312, 793-816).  RCCL is bound at run time
 * (dlopen of librccl.so.1); all collectives run, in program order, on a stream the shard owns, tied to the context's
 * stream by events where data crosses.
 *   mmf_shard_unique_id  rank 0: ncclGetUniqueId; ship the 128 bytes to the other ranks by any means
 *   mmf_shard_create     ncclCommInitRank(world, id, rank) on the context's device
 *   mmf_shard_attach     use the caller's ncclComm_t instead (not destroyed by mmf_shard_destroy)
 *   mmf_shard_broadcast_frame  the root's rgb (u8 x 3) / depth (f32) / id image (u8, may be NULL) into the same
 *                        buffers of every rank: 8 B/px, stream ordered on the context's stream -- call before processFrame
 *   mmf_shard_post_frame / mmf_shard_wait_frame   the same exchange in two halves: post starts it on the shard's own stream
 *                        (behind what the context's stream holds now) so that it overlaps the frame being processed, wait
 *                        makes the context's stream wait for the exchange posted into that slot (0 .. 7)
 *   mmf_shard_gather_poses     after processFrame: all-gather of {pose, lastICPError, lastICPCount} (18 floats per
 *                        model slot); the poses of models other ranks own land in this rank's bookkeeping.  Blocking.
 *   mmf_shard_gather_poses_begin / _end   the same exchange without stalling a frame: _begin enqueues it (pinned
 *                        buffers, an event, no synchronisation), _end waits for the OLDEST one in flight and applies it
 *                        (call it one or two frames later; up to three may be in flight)
 *                        STALENESS CONTRACT: a rank's copy of a model it does not own carries the pose of the newest
 *                        exchange that rank has applied -- the current frame's under the blocking form, one to three frames
 *                        old under _begin / _end.  Nothing on the data path reads those copies (a rank tracks and fuses its
 *                        own models only).  The pose log (mmf_fusion_pose_log / export_poses) is written by a model's OWNER
 *                        only; an object model's entry is global_pose * inverse(pose) (MultiMotionFusion.cpp:829-846) with
 *                        the global pose as that rank holds it, so on ranks other than the global model's it is exact only
 *                        under the blocking form.
 *   mmf_shard_gather_maps      what the segmentation reads of every model (Segmentation.cpp:214-223): the ICP-error image
 *                        and the confidence channel of the splat's vertex image, averaged per super-pixel
 *                        (mmf_slic_downsample) where the model lives and all-gathered: out_dev[n_models][2][nspix] on every
 *                        rank, list order, {icp, confidence}; labels = device int32 super-pixel index image
 * A model belongs to rank (id % world), whatever its position in the list. */
typedef struct mmf_shard mmf_shard;
int mmf_shard_unique_id(char id[128]);
int mmf_shard_create(mmf_ctx *ctx, int rank, int world, const char id[128], mmf_shard **out);
int mmf_shard_attach(mmf_ctx *ctx, int rank, int world, void *nccl_comm, mmf_shard **out);
void mmf_shard_destroy(mmf_shard *s);
int mmf_shard_broadcast_frame(mmf_shard *s, uint8_t *rgb, float *depth, uint8_t *mask, int width, int height, int root);
int mmf_shard_post_frame(mmf_shard *s, uint8_t *rgb, float *depth, uint8_t *mask, int width, int height, int root, int slot);
int mmf_shard_wait_frame(mmf_shard *s, int slot);
int mmf_shard_gather_poses(mmf_shard *s, mmf_fusion *f);
int mmf_shard_gather_poses_begin(mmf_shard *s, mmf_fusion *f);
int mmf_shard_gather_poses_end(mmf_shard *s, mmf_fusion *f);
int mmf_shard_gather_maps(mmf_shard *s, mmf_fusion *f, const int *labels, int spixel_size, float *out_dev);
/* host wall clock of the last processFrame call: the tracking phase (first enqueue .. last result) and the whole call */
int mmf_fusion_last_timings(mmf_fusion *f, double *tracking_s, double *frame_s);
int mmf_fusion_set_segmentation_callback(mmf_fusion *f, mmf_segmentation_fn fn, void *user);
/* exportPoses() (:1020-1045): `poses-<id>.txt` per pose-logging model under export_dir (which ends in '/') */
int mmf_fusion_export_poses(mmf_fusion *f, const char *export_dir);
/* Model::getPoseLog() of the index-th active model: ts[i], p7[7 i ..] = x y z qx qy qz qw */
int mmf_fusion_pose_log(mmf_fusion *f, int index, long long *ts, float *p7, int max_entries, int *n_out);
/* test hook: the device build's mmf_expf and the packed exponential of the two-pixel bilateral filter on n arguments
 * (the packed one is defined for x <= 0 or NaN only) */
int mmf_debug_expf(mmf_ctx *ctx, const float *x_dev, int n, float *out_mmf_dev, float *out_packed_dev);
/* test / A-B hook: 1 = run the Gauss-Newton chain as one launch per iteration where it applies (the default), 0 = always as
 * producer + step launches, -1 = what the environment says (MMF_GN_FUSED=0 turns it off).  Process wide. */
int mmf_debug_set_gn_fused(int on);
/* test hook: the pixels per lane (1, 2, 4 or 5) of the one-launch chain's launches at pyramid levels 0, 1 and 2; 0 leaves a
 * level to the launch geometry's own choice.  A value the level's width does not allow (cols % px != 0) keeps that chain from
 * running.  Any negative argument clears all three: what the environment says (MMF_GN_PX), else by geometry.  Process wide. */
int mmf_debug_set_gn_px(int p0, int p1, int p2);
/* The one-launch chain spins on its own workgroups (a count barrier inside every launch); the library checks the launch's
 * occupancy before it uses that chain, but another process on the same GPU can still keep a launch from becoming resident as
 * a whole.  A launch that gives up marks the chain's result void; the call that waits for it tracks the frame again on the
 * two-launch chain from the pose it started with (RGBDOdometry.cpp:464-467: the call returns a pose, it never aborts) and the
 * process stops using the one-launch chain.  A launch whose sums leave the 64-bit fixed-point range its workgroups add them
 * up in (an ICP partial beyond 2^23: a scene some hundred metres deep) gives up in the same way, with the same consequence: the
 * next frames of such a scene would give up as well.  recoveries: how often that happened; one_launch_chain_in_use: 0 afterwards.
 * Either pointer may be NULL. */
int mmf_gn_chain_status(int *recoveries, int *one_launch_chain_in_use);
/* test hook: the next n one-launch chains of this process give up at their third launch */
int mmf_debug_force_gn_fault(int n);
/* test hook (process wide): the next one-launch chain runs n launches of its per-iteration kernel at pyramid level first_level
 * and nothing else (n = 0 disarms).  It ends like any chain (the divergence guard, the pose handed out), after n - 1 solves.
 * The call fails if it cannot take the one-launch chain.  mmf_debug_gn_truncated then gives, for that odometry: the 58 totals of
 * the last launch as the next launch would have decoded them ([0, 29) ICP, [29, 58) photometric), that pass's
 * {count, sum diff^2 mod 2^32}, and what the last solve left (n = 1: what the chain began with): the running transform's three
 * rows and Rcurr[9], tcurr[3], K R K^-1 [9], K t [3] (at first_level's intrinsics).  Of the call's results only the pose and
 * iterations_run (n - 1) mean anything: the other statistics stay as the odometry's last full chain left them. */
int mmf_debug_gn_truncate(int n, int first_level);
int mmf_debug_gn_truncated(mmf_odom *o, double totals[58], unsigned count_sumsq[2], double rt[12], float pose[24]);
/* test hook: the one-launch chain's solve and pose update (one wave, a row per lane) on n systems in device memory:
 * sys = n x {A[36], b[6]} and rt = n x 16 (the running transform) as doubles, prev = n x {Rprev[9], tprev[3]} floats, the level's
 * intrinsics; rt_out = n x 12 doubles (the new running transform's three rows), pose_out = n x 24 floats (as above). */
int mmf_debug_gn_solve(mmf_ctx *ctx, const double *sys_dev, const double *rt_dev, const float *prev_dev, float fx, float fy,
                       float cx, float cy, int n, double *rt_out_dev, float *pose_out_dev);
/* test hooks of the object models' walk in the one-launch chain (csrc/gn_fused.hpp: an object model's ICP term covers only the
 * rectangle of sensor pixels its prediction can reach under the iteration's pose).  Checking mode (process wide): such models
 * walk the WHOLE image and count the correspondences icpStep accepts outside that rectangle.  mmf_debug_odom_sparse_outside:
 * that count over the last chain of an odometry (0 or the rectangle is wrong), whether the chain walked it by its extents, and
 * rect = the level-0 rectangle of the chain's last launch {x0, y0, width, rows}, the most passes a level-0 rectangle took, and
 * whether the rectangles were derived (1) or the whole image (0), then the lanes the box of the model's own depth needed at
 * levels 0 / 1 / 2 (what its next chain is sized by).  Any pointer may be NULL. */
int mmf_debug_set_sparse_check(int on);
/* test hook: object models get n workgroups per launch of the one-launch chain at every level (0: the default, 32 / 24 / 16);
 * with n = 1 no object's extent fits, the chain reports it, the frame is tracked again on the two-launch chain and the model's
 * next chain is sized by what its box needed -- the one-launch chain stays in use (mmf_gn_chain_status) */
int mmf_debug_set_sparse_groups(int n);
int mmf_debug_odom_sparse_outside(mmf_odom *o, unsigned *outside, int *walked_by_extent, int rect[9]);
/* test / A-B hook: 1 = enqueue the reference's first predict() of a frame (MultiMotionFusion.cpp:675) although nothing
 * inside this library reads its images before the frame's second predict() (:821) overwrites them, 0 = leave it out (the
 * default; -1 = the default).  Process wide. */
int mmf_debug_set_mid_predict(int on);
/* test / A-B hook: the early depth test of combinedPredict (splat_kernel<true>: the rasterising pass reads a pixel's key before it
 * evaluates a fragment there and skips what cannot win; same images).  1 = always, 0 = never, -1 = when the store holds two
 * surfels per pixel or more (the default).  Process wide. */
int mmf_debug_set_splat_bound(int mode);
/* test / A-B hook: the projection / fuse / clean / predict passes of the OBJECT models of a frame: 0 = model by model on the models' own
 * streams, 2 = one launch per pass for all of them, restricted to where each model is (csrc/pass_rect.hpp: the boxes of its
 * key-image writes, of its non-zero images and of its id in the id image), -1 = the default (MMF_PASS_BATCH, or by the number
 * of object models a GPU runs: 2 from four on, 0 below).  Any other mode is MMF_ERR_INVALID and leaves the mode as it was.
 * Same maps and images, bit for bit, in both, also across a frame in which the mode changes.  Process wide. */
int mmf_debug_set_pass_batch(int mode);
/* test / A-B hook: an OBJECT model's model-side preparation (Model::initICPModel / initRGBModel's pyramids, records and point
 * clouds) covers only the box its prediction is non-zero in -- the hull of that box now and at its previous preparation, so
 * that every buffer stays what a whole-frame preparation writes (1, the default) -- or the whole frame (0); -1 = the default
 * (MMF_PREP_RECT).  Same buffers, bit for bit.  Process wide. */
int mmf_debug_set_prep_rect(int on);
/* test hook: from how many destination pixels on a preparation job's workgroups take four 64 x 4 tiles each, one below the other
 * (csrc/prep_batch.hpp: PrepJob::reps).  n > 0 = that many pixels (1: every job), 0 = never, -1 = the default (MMF_PREP_BIG, else
 * 200 000).  Same buffers, bit for bit.  Process wide. */
int mmf_debug_set_prep_big(int n);
/* test entry: the batched frame preparation (csrc/prep_batch.hpp) on n >= 1 stand-alone odometries of one context and size, as ONE
 * set of four stages filled by the collectors the orchestrator uses, launched on the context's stream; the gradients it wrote
 * are adopted, so that "dIdx" / "dIdy" download them.  preds[k] is odometry k's prediction: RGBA32F vertex / normal images, an
 * interleaved 8-bit image of `channels` (3 or 4) bytes per pixel, the pose (HOST, row-major 4 x 4), all dense; optionally the
 * source choice taken on the device (sel != NULL, a DEVICE int: the alt_* images are read when *sel != 0 or, with sel_total
 * != 0, when *sel / sel_total < sel_ratio); ext_gen != 0: the extent words are noted under that generation; pred_box != NULL
 * (DEVICE, four ints {x0, y0, x1, y1}; only without sel): the box the prediction is non-zero in -- the jobs cover the hull of
 * that box and of the previous preparation's (mmf_debug_set_prep_rect).  depth_filtered / rgb (device; either may be NULL)
 * with `sides` (1 = image side, 2 = depth side) are the sensor frame, prepared into odoms[0]: with n = 1 and both sides the
 * model side shares its four launches (prep_collect_all), otherwise the sensor side's jobs come first in each stage and every
 * odometry's model side follows (prep_collect_sensor, prep_collect_model).  No sensor frame: depth_filtered = rgb = NULL.
 * Nothing of this runs outside tests. */
typedef struct mmf_debug_prep_prediction {
    const float *vertex, *normal;
    const unsigned char *image;
    int channels;
    const float *pose;
    const int *sel;
    const float *alt_vertex, *alt_normal;
    const unsigned char *alt_image;
    int sel_total;
    float sel_ratio;
    unsigned ext_gen;
    const int *pred_box;
} mmf_debug_prep_prediction;
int mmf_debug_odom_prepare(mmf_odom *const *odoms, const mmf_debug_prep_prediction *preds, int n, const float *depth_filtered,
                           float depth_cutoff, const unsigned char *rgb, int rgb_channels, int sides);
/* test / A-B hook: when a frame's model side is prepared at the end of the call before it (one model per process, the next frame
 * handed in), the beginning of its tracking (odom_begin_kernel: RGBDOdometry.cpp:221-228, 237, 252-255, 316-328) rides the
 * preparation's last launch on one more workgroup (1, the default: csrc/track_kernels.hpp, prep_batch_begin_kernel) or is a launch
 * of its own in front of the first Gauss-Newton iteration (0); -1 = the default (MMF_BEGIN_RIDER).  Same bits.  Process wide.
 * mmf_debug_begin_rider_count: chains of this process that found their beginning done. */
/* test / A-B hook: every XCD works on one contiguous eighth of a surfel pass's blocks (1, the default: csrc/surfel_kernels.hpp,
 * xcd_block) or the blocks are dealt round-robin as the workgroups are (0); -1 = the default (MMF_XCD).  Same bits.  Synchronises
 * the device; process wide. */
int mmf_debug_set_xcd(int on);
/* the block workgroup `block` of a launch of `blocks` works on under that mapping (a host function: needs no device) */
unsigned mmf_debug_xcd_block(unsigned block, unsigned blocks);
int mmf_debug_set_begin_rider(int on);
int mmf_debug_begin_rider_count(void);
/* test / A-B hook: object models in the producer + step chain (csrc/extent.hpp, ChainGeom: their passes skip the blocks outside
 * the model's own depth and walk the images with a quarter of the workgroups).  1 = on, 0 = every model is tracked like the
 * camera model, -1 = the default (MMF_TRACK_CULL, on).  Process wide. */
int mmf_debug_set_track_cull(int mode);
/* test hook: the 24-bit depth key of combo_splat.frag's gl_FragDepth for n depths, as the rasterising pass computes it (the
 * division by 2 max_depth as three multiply-adds, csrc/surfel_kernels.hpp: splat_depth24_fast) and with the division */
int mmf_debug_depth_keys(mmf_ctx *ctx, const float *z_dev, int n, float max_depth, unsigned *fast_dev, unsigned *divided_dev);
/* Model::computeFusionWeight (Model.cpp:876-891) for pose / lastPose (host 4x4), exported for tests */
int mmf_compute_fusion_weight(const float pose[16], const float last_pose[16], float multiplier, float *out);

/* ---- keypoint descriptor matching ------------------------------------
 * PointTracker::addKeypoints, Core/Utils/PointTracker.cpp:100-114:
 *     cv::BFMatcher(cv::NORM_L2, true).match(current, previous, matches);   // query, train
 *     keep when min_feature_distance < epsilon || match.distance <= min_feature_distance
 * query [nq x dim], train [nt x dim]: dense float32 rows on the device (SuperPoint: dim = 256);
 * dim must be a multiple of 8.  train_idx [nq] receives the matched train row or -1, distance [nq]
 * the L2 distance of a match (0 when unmatched); both on the device.  The nq x nt Gram matrix runs
 * on the f32 matrix cores (csrc/match_kernels.hpp).  Asynchronous on the context's stream. */
int mmf_match_descriptors(mmf_ctx *ctx, const float *query, int nq, const float *train, int nt, int dim,
                          float max_distance, int *train_idx, float *distance);

/* ---- SuperPoint keypoint network --------------------------------------------
 * Replaces the un-vendored super_point_inference package as the reference uses it:
 *     kp_predictor = std::make_shared<SuperPoint>(keypoint_predictor_path);       Core/MultiMotionFusion.cpp:78
 *     std::tie(coordinates[i], descriptors[i]) = kp_predictor->getFeatures(img);  Core/MultiMotionFusion.cpp:233
 * weights: 24 HOST arrays {weight, bias} of conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa
 * convPb convDa convDb in PyTorch layout [Cout][Cin][k][k] / [Cout] (the state dict of SuperPointNet.pt;
 * reading the file is the caller's business).  The object serves images up to max_width x max_height
 * (sides multiples of 8) and returns at most max_keypoints keypoints.  The 3x3 and 1x1 convolutions run
 * on the f32 matrix cores (csrc/superpoint_kernels.hpp). */
typedef struct mmf_superpoint mmf_superpoint;
int mmf_superpoint_create(mmf_ctx *ctx, const float *const *weights, int max_width, int max_height,
                          int max_keypoints, mmf_superpoint **out);
void mmf_superpoint_destroy(mmf_superpoint *sp);
/* The precision of the forward pass is a property of the object.  MMF_SP_F32: the path above, and what
 * mmf_superpoint_create makes.  MMF_SP_F16: conv1a keeps f32 weights and arithmetic and stores f16; the weights of every
 * other layer are rounded to f16 (nearest, ties to even) when they are packed, activations between layers are f16, every
 * output has one f32 accumulator on v_mfma_f32_32x32x16_f16 (csrc/superpoint_f16_kernels.hpp); logits and descriptors
 * leave the two 1x1 heads as f32, and everything behind them is the same code on the same buffers.  A weight of conv1b ...
 * convDb that is not finite, or not finite after the rounding (|w| >= 65520), makes an f16 creation MMF_ERR_INVALID.
 * With precision MMF_SP_F32, mmf_superpoint_create_ex is mmf_superpoint_create. */
enum { MMF_SP_F32 = 0, MMF_SP_F16 = 1 };
int mmf_superpoint_create_ex(mmf_ctx *ctx, const float *const *weights, int max_width, int max_height,
                             int max_keypoints, int precision, mmf_superpoint **out);
int mmf_superpoint_precision(mmf_superpoint *sp); /* MMF_SP_F32 / MMF_SP_F16; -1 for NULL */
/* the rounding of that packing: src[n] f32 -> dst[n] f16 bits, nearest-even, |x| >= 65520 to inf, NaN kept.  Host only. */
int mmf_f16_round(const float *src, size_t n, uint16_t *dst);
/* the network alone: image = DEVICE pointer to interleaved u8 (1 = grey, 3 / 4 = RGB[A]); leaves the detector
 * logits [H/8][W/8][65], the normalised coarse descriptors [H/8][W/8][256] and the heat map [H][W] on the
 * device.  Asynchronous on the context's stream. */
int mmf_superpoint_forward(mmf_superpoint *sp, const uint8_t *image, int width, int height, int channels);
/* copy a result of the last forward pass to the host: which = 0 logits, 1 coarse descriptors, 2 heat map;
 * count must be the exact number of floats.  Synchronous. */
int mmf_superpoint_download(mmf_superpoint *sp, int which, float *host, size_t count);
/* SuperPoint::getFeatures: forward pass, heat >= conf_thresh, greedy non-maximum suppression (Chebyshev
 * radius nms_dist, strongest first), border band removed, descriptors sampled bilinearly and normalised.
 * xy [max_keypoints][2] (pixels), conf [max_keypoints], desc [max_keypoints][256]: HOST arrays, strongest
 * keypoint first; *count = keypoints written.  The reference's `coordinates` are xy / (width, height)
 * (PointTracker.cpp:40-41).  Synchronous. */
int mmf_superpoint_get_features(mmf_superpoint *sp, const uint8_t *image, int width, int height, int channels,
                                float conf_thresh, int nms_dist, int border, int *xy, float *conf, float *desc,
                                int *count);
/* The same WITHOUT the host: enqueues on the context's stream and returns -- no wait, nothing read back, no
 * host memory a second call could overwrite, and a number of launches (mmf_superpoint_last_launches) that depends on
 * (width, height) alone.  The suppression compacts the candidates, runs a fixed few passes over that list and lets ONE
 * workgroup walk what is left to the fixed point under a trip cap of listed + 1; the kept set is ranked by counting on the key
 * (~bits(conf), row-major index) and the strongest max_keypoints go to slot `rank`; max_keypoints workgroups sample the
 * descriptors, workgroup k leaving when k >= count.  Results equal mmf_superpoint_get_features' bit for bit.  (A heat map
 * of ties across the whole image leaves nearly everything to that one workgroup: 2.2 s at 640x480 where the host-facing call
 * needs 28 ms)
 *   mmf_superpoint_device_features   where they are: DEVICE pointers owned by sp, rewritten by its next call.  *count one int,
 *                       *xy [max_keypoints][2], *conf [max_keypoints], *desc [max_keypoints][256] (rows 16-byte aligned);
 *                       rows at or beyond *count are unspecified.
 *   mmf_superpoint_device_status     the suppression's status word, one DEVICE int owned by sp: 0 = converged, 1 = the cap
 *                       was hit -- then *count is 0 and no keypoint is handed on (mmf_tracker_set_keypoint_status takes it).
 *   mmf_superpoint_last_features     waits; the same into HOST arrays (any of xy / conf / desc may be NULL); tests, tools */
int mmf_superpoint_get_features_device(mmf_superpoint *sp, const uint8_t *image, int width, int height, int channels,
                                       float conf_thresh, int nms_dist, int border);
int mmf_superpoint_device_features(mmf_superpoint *sp, const int **count, const int **xy, const float **conf,
                                   const float **desc, int *max_keypoints);
int mmf_superpoint_device_status(mmf_superpoint *sp, const int **status);
int mmf_superpoint_last_features(mmf_superpoint *sp, int *count, int *status, int *xy, float *conf, float *desc);
int mmf_superpoint_last_launches(mmf_superpoint *sp);
/* one convolution layer (tests / tools): in [H][W][cin], out [H][W][cout] (or [H/2][W/2][cout] with pool) on
 * the device, channels-last; w [cout][cin][k][k], bias [cout] on the HOST; taps = 9 (3x3, zero pad 1) or 1;
 * cin a multiple of 32; nt = output-channel tiles of 32 per workgroup (1, 2, 4; 0 = automatic). Synchronous. */
int mmf_superpoint_conv(mmf_ctx *ctx, const float *in, int height, int width, int cin, const float *w,
                        const float *bias, int cout, int taps, int relu, int pool, int nt, float *out);
/* one layer of the f16 path (tests / tools): in [H][W][cin] f16 bits on the device; w, bias f32 on the HOST, w rounded as an
 * f16 creation rounds it (and refused like there); out f16 bits or, with out_is_f32, the unrounded f32 value (the two 1x1
 * heads).  Sizes, taps, nt and refusals as mmf_superpoint_conv.  Synchronous. */
int mmf_superpoint_conv_f16(mmf_ctx *ctx, const uint16_t *in, int height, int width, int cin, const float *w,
                            const float *bias, int cout, int taps, int relu, int pool, int nt, int out_is_f32, void *out);
/* (tests / tools) the first `layers` launches of mmf_superpoint_forward -- 1 = conv1a, 2 = conv1b + pool, 3 = conv2a, 4 = conv2b +
 * pool, 5 = conv3a, 6 = conv3b + pool, 7 = conv4a, 8 = conv4b, 9 = convPa | convDa -- and that launch's output [h][w][cout] copied
 * to the HOST: f16 bits on an MMF_SP_F16 object, f32 on an MMF_SP_F32 one; bytes = its exact size.  Synchronous. */
int mmf_debug_superpoint_forward_prefix(mmf_superpoint *sp, const uint8_t *image, int width, int height, int channels,
                                        int layers, void *host_out, size_t bytes);
/* the post-processing by itself (tests / tools): the code behind the two feature calls above, on maps given from outside.
 *   mmf_superpoint_set_maps       installs maps as if a forward pass of width x height had produced them.  Exactly one of
 *                       semi_dev (logits [H/8][W/8][65]; the heat map is then computed from them) and heat_dev ([H][W]);
 *                       desc_dev [H/8][W/8][256] or NULL (a zero map), L2-normalised per cell when normalize_desc != 0.  DEVICE
 *                       pointers, copied into the object's own buffers on the context's stream.  Sizes as mmf_superpoint_forward.
 *                       With heat_dev the logits mmf_superpoint_download(0) returns are unspecified.
 *   mmf_superpoint_select         mmf_superpoint_get_features without its forward pass (HOST outputs, synchronous).
 *   mmf_superpoint_select_device  mmf_superpoint_get_features_device without its forward pass; results by
 *                       mmf_superpoint_last_features, mmf_superpoint_last_launches counts the selection's kernels alone.
 * Both selections: MMF_ERR_STATE before any maps or forward pass exist.
 * Contract of a heat map: its values are softmax outputs, that is in [0, 1], +inf or NaN (NaN is never a candidate and never
 * suppresses).  Negative values and -0.0 are outside it: the ranking (sp_rank_key) orders confidences by bit pattern. */
int mmf_superpoint_set_maps(mmf_superpoint *sp, int width, int height, const float *semi_dev, const float *heat_dev,
                            const float *desc_dev, int normalize_desc);
int mmf_superpoint_select(mmf_superpoint *sp, float conf_thresh, int nms_dist, int border, int *xy, float *conf, float *desc,
                          int *count);
int mmf_superpoint_select_device(mmf_superpoint *sp, float conf_thresh, int nms_dist, int border);

/* ---- super-pixel resampling for the segmentation ------------------------------
 * Slic::downsample<float>(image, channel) (Core/Segmentation/Slic.h:48-83), Slic::downsampleThresholded<float>
 * (:87-126), Slic::downsample() (Slic.cpp:82-112) and Slic::upsample<unsigned char> (Slic.h:133-146), which
 * Segmentation.cpp:177-178,218-221,683 runs on the CPU after downloading the full-resolution ICP-error and
 * vertex-confidence textures of every model.  labels = gSLICr's segmentation mask (int32 [height][width],
 * values in [0, n), n = (width / spixel_size) * (height / spixel_size)); everything is a DEVICE pointer and
 * the calls are asynchronous on the context's stream.  Results are those of the reference's loops bit for
 * bit: float sums run in pixel order, the in-place division and the empty-super-pixel substitution
 * (resampleEmptyIndex, including its spixelY quirk) are reproduced.
 *   image [height][width][channels] float32, `channel` selected (the ICP-error map: channels 1; the
 *   vertex-confidence map: channels 4, channel 3); thresholded != 0: only values > min_threshold count
 *   (the depth map with 0.02); out [n] float32; counts_out (optional) [n] int32 = spixelCounts. */
int mmf_slic_downsample(mmf_ctx *ctx, const int *labels, int width, int height, int spixel_size, const float *image,
                        int channels, int channel, int thresholded, float min_threshold, float *out, int *counts_out);
/* rgb [height][width][channels] u8 (3 or 4); out [n][3] u8 = integer means of input channels (2, 1, 0) */
int mmf_slic_downsample_rgb(mmf_ctx *ctx, const int *labels, int width, int height, int spixel_size, const uint8_t *rgb,
                            int channels, uint8_t *out);
/* out[i] = map[labels[i]] */
int mmf_slic_upsample_u8(mmf_ctx *ctx, const int *labels, int width, int height, const uint8_t *map, int nspix,
                         uint8_t *out);

/* ---- the super-pixel engine (csrc/slic_engine_kernels.hpp) -------------------------------------------
 * The label image the calls above take, computed on the device: SLIC as the reference configures gSLICr
 * (Core/Segmentation/Slic.cpp:33-43: RGB colour space, GIVEN_SIZE, coh_weight 0.6, 5 iterations, no connectivity
 * enforcement).  rgb = DEVICE u8 [height][width][3] (the channels take part symmetrically, in memory order);
 * spixel_size S in (10, 256) and it must DIVIDE width and height (MMF_ERR_INVALID otherwise: gSLICr's map is
 * ceil(W/S) x ceil(H/S), Slic.h sizes its arrays by (W/S)(H/S)); n = (width / S) * (height / S).
 * initialise; iterations x (associate, update); associate -- iterations = 5 is the reference's, 0 = one association.
 *   centres_in   optional DEVICE [n][5] float32 {x, y, c0, c1, c2}: replaces the initialisation
 *   labels_out   DEVICE int32 [height][width], values in [0, n)
 *   centres_out  optional DEVICE [n][5] float32: the centres the last association used
 *   counts_out   optional DEVICE [n] int32: the pixels per centre at the last update (zeros when iterations == 0)
 * Asynchronous on the context's stream; 2 + 2 * iterations launches (+ 1 with centres_out).  Integer sums, float32 in
 * a fixed order: the results do not depend on the order the pixels are visited in. */
int mmf_slic_segment(mmf_ctx *ctx, const uint8_t *rgb, int width, int height, int spixel_size, int iterations,
                     const float *centres_in, int *labels_out, float *centres_out, int *counts_out);

/* ---- dense-CRF motion segmentation (Core/Segmentation/Segmentation.cpp:159-740, performSegmentationCRF) ----------
 * The segmentation that spawns object models, on the device (csrc/crf_kernels.hpp): super-pixel
 * means of the raw depth and of every model's ICP-error image and splat confidence, unaries from the ICP error, a
 * fully connected CRF (two Potts kernels, symmetric normalisation) by mean field, then the reference's post-processing
 * (largest connected component per label, size and border rules, depth statistics).  The Gaussian sums are EXACT
 * (densecrf's permutohedral lattice approximates them: DESIGN.md B1).  Labels are gSLICr-like super-pixel indices
 * (int32 [height][width], values in [0, n)); without them the regular grid min(y/S, H/S-1) * (W/S) + min(x/S, W/S-1)
 * is used (B3).  When the depth range of the frame is not a finite positive number every cell is background and no
 * new label is proposed (range_invalid, B4).
 *   mmf_crf_default_config   the GUI's settings (GUI/Tools/GUI.h:211-226 pushed by MainController.cpp:658-670); the
 *                        header defaults of Segmentation.h:140-159 are replaced by these before any segmentation runs.
 *                        Needs no device.
 *   mmf_crf_segment          stand-alone, synchronous: low_maps = DEVICE [n_models][2][n] {icp, conf} per super-pixel
 *                        as mmf_shard_gather_maps writes them (model list order); rgb / depth = DEVICE full-resolution
 *                        frame (u8 x 3, float32 metres); ids = HOST model ids in list order (< 255), next_id = the new
 *                        label's id, allow_new = spawnOffset >= modelSpawnOffset.  Writes the DEVICE mask_out
 *                        (width*height u8, fullSegmentation: model id or 255 per pixel), the HOST models_out (capacity
 *                        n_models + 1: the existing models, then the new label's entry when it survived), *n_models_out
 *                        and *has_new_label.  At most 32 labels and 16384 super-pixels.
 *   mmf_crf_last             what the last segmentation on this context computed (for tests and GUIs): the info
 *                        below, the model data, and optionally (DEVICE pointers, NULL to skip) the unaries [L][n], the
 *                        final marginals Q [L][n], the raw argmax map and the filtered map [n] (model ids, 255 =
 *                        removed).  Synchronous. */
typedef struct {
    float sigma_rgb, sigma_depth, sigma_pos;   /* pairwise standard deviations: 10, 0.9, 1.8 */
    float weight_appearance, weight_smoothness; /* 7, 2 */
    float threshold_new;       /* unaryThresholdNew: 5.5 */
    float unary_weight_error;  /* 75 */
    float unary_k_error;       /* 0.0375 */
    int iterations;            /* mean-field iterations: 10 */
    float min_rel_size_new, max_rel_size_new; /* 0.005, 0.4 of the super-pixels */
    int spixel_size;           /* SegmentationConfiguration::sp_size: 16, in (10, 256) */
    int model_spawn_offset;    /* fusion only: frames between spawns (22) */
    int inhibit_new;           /* fusion only: setSetInhibit (hasNewLabel forced to 0) */
} mmf_crf_config;

typedef struct {
    int n_cells, cells_x, cells_y; /* n = (W/S) (H/S) */
    int n_labels;       /* L = models + allow_new */
    int n_models;       /* entries of the model data */
    int allow_new, has_new_label, range_invalid, n_components;
    float range;        /* depth range of the super-pixel depth */
} mmf_crf_info;

int mmf_crf_default_config(mmf_crf_config *cfg);
int mmf_crf_segment(mmf_ctx *ctx, const mmf_crf_config *cfg, const int *labels, int width, int height, const uint8_t *rgb,
                    const float *depth, const float *low_maps, const unsigned *ids, int n_models, unsigned next_id,
                    int allow_new, uint8_t *mask_out, mmf_segmentation_model *models_out, int *n_models_out,
                    int *has_new_label);
int mmf_crf_last(mmf_ctx *ctx, mmf_crf_info *info, mmf_segmentation_model *models, int capacity, float *unaries,
                 float *q, uint8_t *raw_map, uint8_t *map);

/* The built-in segmentation (mmf_crf_segment) for enable_multiple_models, where the reference calls performSegmentation
 * (:412): precedence mmf_frame::segmentation, then the callback, then this; cfg == NULL switches it off (default).
 * It reads every model's ICP-error image (error_recording) and the splat of the previous frame, runs on the fusion's
 * stream behind every model's tracking, and needs world == 1 (MMF_ERR_STATE otherwise; sharded front ends call
 * mmf_crf_segment in their callback).  spawnOffset (:148, :410, :484) counts the multi-model tracked frames up to
 * cfg->model_spawn_offset and restarts at every spawn; a new label is proposed only once it has reached it.
 * mmf_fusion_set_superpixels: DEVICE int32 label image (width x height) for the NEXT frame only (copied); NULL: grid.
 * mmf_fusion_last_segmentation: mmf_crf_last of the fusion's context.
 * mmf_fusion_set_superpixel_engine: mode 0 = off (default), 1 = the label image of every frame the built-in segmentation
 *   handles is computed from that frame's RGB by mmf_slic_segment's engine (5 iterations, spixel_size of the CRF
 *   configuration), on a stream of its own beside the tracking.  Precedence per frame: labels handed in through
 *   mmf_fusion_set_superpixels, then the engine, then the grid.  MMF_ERR_INVALID when spixel_size does not divide the frame
 *   size -- here, and at the frame when the CRF configuration changed since; never a silent fall back to the grid.
 * mmf_fusion_last_superpixels: the label image the last segmentation used, whichever of the three it was, copied to the
 *   DEVICE int32 [height][width] labels_out.  Synchronous.  MMF_ERR_STATE before the first segmentation. */
int mmf_fusion_set_crf_segmentation(mmf_fusion *f, const mmf_crf_config *cfg);
int mmf_fusion_set_superpixels(mmf_fusion *f, const int *labels);
int mmf_fusion_set_superpixel_engine(mmf_fusion *f, int mode);
int mmf_fusion_last_superpixels(mmf_fusion *f, int *labels_out);
int mmf_fusion_last_segmentation(mmf_fusion *f, mmf_crf_info *info, mmf_segmentation_model *models, int capacity,
                                 float *unaries, float *q, uint8_t *raw_map, uint8_t *map);

/* ---- segmentation from a frame's GIVEN label image (Core/Segmentation/Segmentation.cpp:89-147: the branch of
 * performSegmentation for `frame.mask.total() != 0`, tested before the segmentation mode) -----------------------------------
 * What a mask dataset (Mask####.png, -maskdir), ground-truth ids or an external instance segmenter hand in: arbitrary labels
 * per pixel.  On the device (csrc/mask_kernels.hpp): labels are mapped to model ids through a 256-entry
 * table that persists from frame to frame (label 0 is background and never reads it); with allow_new the unmapped non-zero label
 * whose first pixel comes first in raster order becomes the new model's (table[label] = next_id); pixels of labels that stay
 * unmapped get id 0, are NOT counted for id 0 and DO enter the depth statistics of the global model.  Model data: the active
 * models in list order, then the new label's entry; super_pixel_count = pixels / 256 (the new entry: at least 1),
 * avg_confidence = 0.4, depth_mean / depth_std = mean and mean absolute deviation of the raw depth over the pixels of the id,
 * zero depth included, summed in float64 in a fixed order (B7: same input, same bits).  A label mapped to an id that is
 * neither in `ids` nor the new label's keeps that id in the mask and enters no entry (B7).
 *   mmf_mask_default_config  model_spawn_offset 22, inhibit_new 0.  Needs no device.
 *   mmf_mask_segment         stand-alone, synchronous: labels (u8) / depth (f32 metres) = DEVICE width*height images; ids =
 *                        HOST model ids in list order (ids[0] == 0, all <= 255, at most 255), next_id <= 255; mapping = HOST
 *                        table, in / out; mask_out = DEVICE width*height u8 (must not overlap labels); models_out = HOST,
 *                        capacity n_models + 1; *new_label = the input label that became new, or -1.  Two passes over the
 *                        image and two one-workgroup launches.
 * Inside processFrame (off by default; MMF_ERR_STATE with world > 1 -- a sharded front end calls mmf_mask_segment in its
 * segmentation callback):
 *   mmf_fusion_set_mask_segmentation   cfg == NULL switches it off.  With it on, a frame whose mmf_segmentation has
 *                        model_data == NULL -- and the mask_host of mmf_fusion_process_frame_host[_next] -- carries RAW LABELS and
 *                        has_new_label is ignored: the frame is segmented here, on the fusion's stream, before the callback and
 *                        the built-in CRF are considered; allow_new = spawnOffset >= cfg->model_spawn_offset (the counter of
 *                        mmf_fusion_set_crf_segmentation), inhibit_new clears has_new_label afterwards (the mask and the table
 *                        entry stay, MultiMotionFusion.cpp:413-415).  One host wait for the summary.  A mmf_segmentation that
 *                        brings model_data keeps its meaning; a frame without a mask goes to the callback / the CRF.
 *                        The labels must not be the fusion's own "MASK" texture (mmf_fusion_texture), which the id image
 *                        is written to: MMF_ERR_INVALID, as for any mask_out that overlaps the labels.
 *   mmf_fusion_mask_mapping  the fusion's table (cleared by mmf_fusion_reset)
 *   mmf_fusion_last_mask_segmentation  what the last frame this path handled computed; has_new_label as processFrame used it
 *                        (after inhibit_new).  MMF_ERR_STATE before the first such frame. */
typedef struct {
    int model_spawn_offset; /* frames between spawns (22) */
    int inhibit_new;        /* setSetInhibit (hasNewLabel forced to 0) */
} mmf_mask_config;
typedef struct {
    int n_models;      /* entries of the model data */
    int allow_new, has_new_label;
    int new_label;     /* the input label that became new, or -1 */
} mmf_mask_info;
int mmf_mask_default_config(mmf_mask_config *cfg);
int mmf_mask_segment(mmf_ctx *ctx, int width, int height, const uint8_t *labels, const float *depth, const unsigned *ids,
                     int n_models, unsigned next_id, int allow_new, uint8_t mapping[256], uint8_t *mask_out,
                     mmf_segmentation_model *models_out, int *n_models_out, int *has_new_label, int *new_label);
int mmf_fusion_set_mask_segmentation(mmf_fusion *f, const mmf_mask_config *cfg);
int mmf_fusion_mask_mapping(mmf_fusion *f, uint8_t mapping_out[256]);
int mmf_fusion_last_mask_segmentation(mmf_fusion *f, mmf_mask_info *info, mmf_segmentation_model *models, int capacity);

/* ---- keypoint redetection of inactive models (Core/MultiMotionFusion.cpp:425-436, 489-559; Model::getBestMatch,
 * Core/Model/Model.cpp:781-874; Model::store / activate, :1617-1656) -------------------------------------------------
 * A VIEW is what one time index of a model's stored local tracks holds (tracks_local = the result of
 * computeTrackProjectionFirstFrame, Model.cpp:508-522): n valid keypoints -- null and non-finite ones dropped, :806-811 --
 * with descriptor [n][256] float32 and coordinate [n][3] in the model's local frame.  The view store keeps the views of
 * all models in one device buffer; a query set (the keypoints of one segment) is matched against EVERY view of the store
 * in three launches, whatever the number of views (csrc/redetect_kernels.hpp): per view what
 * cv::BFMatcher(NORM_L2, true).match(query, view) returns, no distance gate, distances the fmaf chains of
 * mmf_match_descriptors.  Views are processed in ascending index and one RigidRANSAC{10, 0.03, 0.8} is constructed per
 * best-match call.
 *   mmf_viewstore_store       HOST arrays: counts[n_views] valid keypoints per view (0 allowed), the views' descriptors and
 *                         coordinates one after the other.  Like Model::store (:1618-1621) a model that has stored views
 *                         ignores a second store: *stored = 0.  Synchronous.  The store only grows; growing never frees a
 *                         buffer before mmf_viewstore_destroy.
 *   mmf_viewstore_store_device   the same with the rows on the DEVICE (what mmf_tracker_model_views returns): counts = HOST,
 *                         descriptor (16-byte aligned) / coordinate = DEVICE, the views' rows one after the other.  A kernel
 *                         scatters the rows to their padded places; the coordinates come back through pinned memory.  One
 *                         wait.  The store is then what mmf_viewstore_store leaves with the same views downloaded.
 *   mmf_viewstore_forget      the model is gone: its views stay in place, belong to nobody and match nothing of interest
 *   mmf_viewstore_num_views / _view   the views in store order (models in the order they were stored, a model's views ascending)
 *   mmf_viewstore_match       query = DEVICE [nq][256] (16-byte aligned); HOST train_idx / distance [views][nq]: the row of the
 *                         view that query row matched or -1, and the distance (0 when unmatched).  Synchronous.
 *   mmf_viewstore_best_match  Model::getBestMatch for one model: coordinate = HOST [nq][3] of the query keypoints; views with at
 *                         least 3 matches (:839), estimate(query, train) per view, estimates without inliers dropped (:859), the
 *                         smallest error wins, the first of equals (:870-873).  *found = 0: no estimate (T identity, error +inf).
 *                         T = Result::transformation (query ~ T train), *view = index of the winning view inside the model,
 *                         *n_matches its matches, inlier (optional, capacity nq) = Result::inlier over the hash-sorted matches.
 *   mmf_viewstore_last_launches   kernel launches the last match enqueued (3 per query set; 0 with an empty store)
 * Inside processFrame (off by default; MMF_ERR_STATE with world > 1):
 *   mmf_fusion_set_redetection   setEnableRedetection.  With it on, a frame that has keypoints, inactive models and stored views
 *                         labels the keypoints by the id image, and per label other than 0 / 255 with at least 3 finite
 *                         keypoints (labels ascending) and per inactive model (list order) accepts the best match when
 *                         error < 0.01 and inliers > 5 (:516): a pending new label is cancelled (no model is spawned, no id
 *                         consumed), an active model carrying the label is dropped and freed unless it is older (smaller id)
 *                         than the inactive one -- then nothing happens for the pair --, and the inactive model joins the active
 *                         list with pose = transformation^-1 (Model::activate), its map and its id.  Two host waits per such
 *                         frame (labels, matches); otherwise nothing is enqueued and nothing awaited.
 *   mmf_fusion_set_keypoints     the last keypoint of every currently visible track (track->back(), :428-436) for the NEXT
 *                         processFrame only: HOST xy [n][2] int pixels (outside the image: dropped, :432), coordinate [n][3]
 *                         camera frame (non-finite allowed), descriptor [n][256].  Copied.
 *   mmf_fusion_viewstore         the fusion's store (owned by the fusion): store a model's views there when it turns up in the
 *                         inactive list
 *   mmf_fusion_last_redetections what the last frame did, accepted matches in order (also the refused older / newer pairs:
 *                         activated = 0) */
typedef struct mmf_viewstore mmf_viewstore;
typedef struct {
    int label;      /* the segment's label in the id image */
    int model_id;   /* the inactive model whose view matched */
    int removed_id; /* the active model that carried the label and was dropped, or -1 */
    int activated;  /* 0: refused, an older active model carries the label (:536-541) */
    float error;    /* RigidRANSAC::Result::error of the best view */
    int inliers, view;
    float transformation[16]; /* Result::transformation; the model's new pose is its inverse */
} mmf_redetection;
int mmf_viewstore_create(mmf_ctx *ctx, mmf_viewstore **out);
void mmf_viewstore_destroy(mmf_viewstore *vs);
int mmf_viewstore_store(mmf_viewstore *vs, int model_id, int n_views, const int *counts, const float *descriptor,
                        const float *coordinate, int *stored);
int mmf_viewstore_store_device(mmf_viewstore *vs, int model_id, int n_views, const int *counts, const float *descriptor,
                               const float *coordinate, int *stored);
int mmf_viewstore_forget(mmf_viewstore *vs, int model_id);
int mmf_viewstore_num_views(mmf_viewstore *vs);
int mmf_viewstore_view(mmf_viewstore *vs, int view, int *model_id, int *index, int *rows);
int mmf_viewstore_match(mmf_viewstore *vs, const float *query, int nq, int *train_idx, float *distance);
int mmf_viewstore_best_match(mmf_viewstore *vs, int model_id, const float *query, const float *coordinate, int nq,
                             float T[16], float *error, int *inliers, int *view, int *n_matches, unsigned char *inlier,
                             int *found);
int mmf_viewstore_last_launches(mmf_viewstore *vs);
int mmf_fusion_set_redetection(mmf_fusion *f, int on);
int mmf_fusion_set_keypoints(mmf_fusion *f, int n, const int *xy, const float *coordinate, const float *descriptor);
mmf_viewstore *mmf_fusion_viewstore(mmf_fusion *f);
int mmf_fusion_last_redetections(mmf_fusion *f, mmf_redetection *out, int capacity, int *n_out);

/* ---- keypoint-based pose initialisation: RigidRANSAC (Core/Utils/RigidRANSAC.h:6-32, .cpp:73-180) ----
 * Host code, like the reference's (a few dozen keypoint tracks): p0, p1 are HOST arrays of n 3-D points
 * (row-major n x 3), mask an optional n-byte selection; T receives the row-major 4x4 of T_01 with
 * p0 ~ T_01 p1.  mmf_rigid_fit = the free function fit() (RigidRANSAC.cpp:73-120).  A mmf_ransac object owns
 * the std::default_random_engine of the reference's class, so successive estimates continue its sequence.
 * estimate(): error = mean inlier distance of the best model (+inf when none beat the initial all-points
 * fit); inlier (optional, n bytes) flags the rows of the HASH-SORTED correspondence order used internally
 * (RigidRANSAC.cpp:36-58), exactly what Result::inlier holds in the reference; *has_inlier = 0 when empty. */
typedef struct mmf_ransac mmf_ransac;
int mmf_rigid_fit(const float *p0, const float *p1, int n, const unsigned char *mask, float T[16]);
int mmf_rigid_apply(const float T[16], const float *p0, const float *p1, int n, float *distance);
int mmf_ransac_create(int iterations, float inlier_threshold, float inlier_fraction, mmf_ransac **out);
void mmf_ransac_destroy(mmf_ransac *r);
int mmf_ransac_estimate(mmf_ransac *r, const float *p0, const float *p1, int n, const unsigned char *mask,
                        float T[16], float *error, unsigned char *inlier, int *has_inlier);

/* ---- keypoint tracks on the device: tracker::PointTracker (Core/Utils/PointTracker.cpp:27-226), the per-model track sets
 * (Model::tracks, Model::updateTracks, Core/Model/Model.cpp:630-640; MultiMotionFusion.cpp:425-436, 584-604, 622-627) and
 * Model::getLastTrackTransform (Model.cpp:739-775) -------------------------------------------------------------------------
 * A TRACKER is a table of at most `capacity` tracks in the order of the reference's `tracks` vector (csrc/tracker_kernels.hpp).
 * Per track it keeps what the reference's consumers read, not the history: the descriptor of the last non-null keypoint, the
 * last two slots `cur` = end()[-1] and `prev` = end()[-2] (xy, coordinate, timestamp, non-null flag; a null slot holds zeros),
 * age (frames since the last non-null keypoint, 0 = this frame), nvalid (non-null keypoints so far), last_stamp, a uid that is
 * never reused, this frame's label and `member`, a 256-bit set of model ids: bit m = the track is in Model m's `tracks`.
 * `length` is the common length of the reference's tracks: frames since the table was last empty (0 when empty).
 * Pyramid level 0 only.  Every call enqueues a fixed number of launches on the context's stream, whatever the number of
 * keypoints and tracks, and returns; the calls marked "waits" wait for the stream once.  Differences from the reference:
 * a track that does not fit is dropped and counted (the reference's vector grows without bound), and a keypoint outside
 * the image gets NaN coordinates (the reference reads the depth image out of bounds there).
 *   mmf_tracker_create      intrinsics of level 0; max_keypoints bounds n of an add
 *   mmf_tracker_add_keypoints   addKeypoints (:27-131): DEVICE xy [n][2] int pixels (cvRound(normalised * (cols, rows)), :38),
 *                       DEVICE descriptor [n][256] (16-byte aligned), DEVICE depth [height][width] f32; all three are read
 *                       by the enqueued work.  coordinate = z * (x - cx) / fx, ... in float, NaN where z <= 0.  The active
 *                       tracks (age < history before this frame; history 0: all) are matched with the kernels of
 *                       mmf_match_descriptors (cross check, distance <= min_feature_distance unless that is < epsilon); every
 *                       track is extended by a null keypoint, matched tracks get theirs, unmatched keypoints start tracks in
 *                       ascending index.  An empty table adds without matching and restarts `length` at 1 (:61-66).
 *   mmf_tracker_prune       prune (:170-203): tracks with nvalid < min_kps AND last_stamp < min_time go, the rest close up in order
 *   mmf_tracker_associate   mask = DEVICE u8 id image [height][width].  label = mask at cur.xy for tracks whose cur is non-null
 *                       and inside the image, else -1.  For every listed model m that is some track's label: bit m of every
 *                       LABELLED track becomes (label == m); unlabelled tracks keep their sets (updateTracks(segm_tracks[m],
 *                       the other segments' tracks), :584-604)
 *   mmf_tracker_associate_all   every track joins every listed model (:622-627; initGlobalTracks at the first frame)
 *   mmf_tracker_forget_model    the model is gone: its bit is cleared everywhere
 *   mmf_tracker_last_pairs  waits.  For every listed model, in ONE launch: the tracks of the model, in table order, whose prev and
 *                       cur are non-null with finite coordinates (Model.cpp:747-761).  *p0 (prev) / *p1 (cur) = pinned HOST
 *                       [n_models][*stride][3], *counts = pinned HOST [n_models]; valid until the tracker's next call
 *   mmf_tracker_last_track_transform   waits.  getLastTrackTransform of one model: a fresh RigidRANSAC(cfg; NULL = {10, 0.03, 0.6})
 *                       on its pairs, p0 ~ T p1; fewer than 3 pairs: identity, error +inf, *has_inlier = 0.  inlier (optional)
 *                       holds at least `capacity` bytes: Result::inlier over the hash-sorted pairs
 *   mmf_tracker_visible     waits.  The tracks with a non-null cur, in order (track->back(), MultiMotionFusion.cpp:428-431): HOST xy
 *                       [*n][2], coordinate [*n][3], descriptor [*n][256], uid [*n]; arrays of `capacity` rows, any may be NULL
 *   mmf_tracker_status      waits.  Tracks, length, and the appends dropped since creation / reset
 *   mmf_tracker_download    waits.  The whole table into HOST arrays of `capacity` rows (tests and tools): the two-slot arrays
 *                       hold cur at row 0 and prev at row `capacity`; any array may be NULL
 *   mmf_tracker_last_launches   kernel launches of the tracker's last call
 *   mmf_tracker_reset       empty table, uid and counters from 0; the view log is emptied and its stamps restart
 * The VIEW LOG (off by default) is what Model::store's views are built from without a history kept by the caller:
 *   mmf_tracker_set_view_log    frames = 0: off, the ring is freed and an add stays 7 launches.  Otherwise a ring of `frames`
 *                       slots is allocated here, behind a wait for the stream, and starts empty.  With it on every add also
 *                       writes the frame's visible set -- count, uid, camera-frame coordinate and the descriptor of THAT
 *                       frame's keypoint, in table order -- into slot stamp % frames: two more launches, nothing read back.
 *   mmf_tracker_frame       adds since creation / reset = the stamp of the newest frame (host-known, no wait)
 *   mmf_tracker_model_views waits once.  View v = the logged keypoints of frame frames[v], in log order (uid ascending), whose
 *                       uid is in the table NOW (a pruned track has left), whose track has bit model_id NOW (a track that
 *                       joined later brings its earlier keypoints, one that left brings none) and whose coordinate in the
 *                       frame of poses[v] (HOST [n_views][16], row-major, camera -> model) is finite: project_kp
 *                       (Model.cpp:130-141), floats widened to double, ((r0 x + r1 y) + r2 z) + t per row with every product
 *                       and sum rounded on its own, rounded to float.  A frame that is not in the ring (older than `frames`
 *                       adds, newer than the newest, before the last reset or the switching on) gives an empty view and
 *                       counts in *missing.  *counts = pinned HOST [n_views]; *descriptor / *coordinate = DEVICE, the views'
 *                       rows one after the other ([rows][256], [rows][3]); they belong to the tracker and stay valid until
 *                       its next call.  Two launches whatever n_views is (0 allowed).
 * Differences from the reference: the history is bounded by the log (Model::store has poses.size() views, this the last
 * `frames` of them), and a caller pairs poses with frames BY STAMP (the reference pairs from the end of the lists, which
 * shifts every keypoint against its pose by one frame when a deactivation is scheduled).  The on-disk files are out of
 * scope.
 * BACK-DATING (Model::refineTrackSubset, Model.cpp:649-737; csrc/backdate_kernels.hpp): how the tracks of
 * one segment moved in the frames before it was segmented, as a pose list whose end is the identity.
 *   mmf_tracker_backdate    waits twice (counts, estimates).  S = the table rows with label[i] == label (after this frame's
 *                       mmf_tracker_associate), in table order.  len = max(1, min(length, history, the frames newest, newest
 *                       - 1, ... the ring holds)); entry j = the frame with stamp newest - len + 1 + j.  A track's keypoint in
 *                       a frame is the entry of that frame's slot with its uid.  ik = 0; for jk = 1 .. len - 1: both = rows of
 *                       S with a keypoint at ik and at jk, nvalid = those finite at both, from = ik; nvalid < 3: rel[jk] =
 *                       rel[ik], status TOO_FEW, ik stays; else T = the estimate of a FRESH RigidRANSAC{cfg of `batch`} for
 *                       the nvalid rows in table order (p0 at ik, p1 at jk), rel[jk] = rel[ik] T, ik = jk.  pose[j] =
 *                       inverse(rel[len - 1]) rel[j]; pose[len - 1] is exactly the identity.  Three launches whatever len, the
 *                       tracks and the slots are, then the batch object's one (none without a problem, and then one wait).
 *                       A problem with more than max_points rows is estimated by the same core on the host and flagged
 *                       (more than 65535: status TOO_MANY, T identity).  out = HOST [capacity], capacity >= min(history, the
 *                       frames in the ring) (MMF_ERR_INVALID otherwise); *n_out = len.  2 <= history <= 256 and label 0 .. 255
 *                       (MMF_ERR_INVALID), a tracker without a view log: MMF_ERR_STATE, a batch object of another context:
 *                       MMF_ERR_INVALID.  The table and the log are not written.  Frames are paired BY STAMP (the reference
 *                       indexes the tracks by the camera's pose count, which is wrong once the table was ever empty), every
 *                       pair gets a fresh engine (the reference runs one on; the same for its only history, 2), and every
 *                       entry carries its frame's stamp and its add's timestamp, kept on the host (the reference: 0 without
 *                       a common track)
 *   mmf_tracker_reserve_backdate   the workspace for windows of up to `history` frames, allocated HERE behind a wait for the
 *                       stream (0 frees it); a mmf_tracker_backdate that needs more than is reserved reserves it itself
 *   mmf_tracker_backdate_rows      test accessor: the p0 / p1 rows ([*n][3], HOST arrays of `capacity` rows) the last
 *                       mmf_tracker_backdate handed the batch object for entry `entry` (none: *n = 0)
 * Inside processFrame (off by default; MMF_ERR_STATE with world > 1; the fusion does not own the tracker, which must share
 * its context and image size):
 *   mmf_fusion_set_tracker      tracker = NULL detaches.  The caller adds and prunes a frame's keypoints BEFORE processFrame
 *                       (MultiMotionFusion.cpp:223-248).  First frame: every track joins model 0.  Later tracked frames with
 *                       odom_init_kp: one pairs call for all active models, one transformation per model in list order,
 *                       handed to the init_transforms path with the setter's icp_refine (a frame that brings init_transforms
 *                       of its own: MMF_ERR_INVALID).  After the frame's segmentation, redetection and spawn: associate against
 *                       textures[MASK] with the active ids (associate_all without enable_multiple_models); a model that left
 *                       the active list is forgotten.  With redetection on, a frame without mmf_fusion_set_keypoints takes
 *                       the tracker's visible set as its keypoints.  With redetection on AND a view log, every active
 *                       object model gets one (stamp, pose after tracking) entry per tracked frame (a spawned model at the end
 *                       of its first frame; a re-activated one restarts with the activation pose, Model::activate), trimmed
 *                       to the log's length, and a model that leaves the active list -- lost or scheduled -- stores its
 *                       views from the log (mmf_tracker_model_views -> mmf_viewstore_store_device), entries paired with frames
 *                       by stamp, before the tracker forgets it, once.  Otherwise nothing is recorded, enqueued or awaited.
 *   mmf_fusion_last_stored_views    what the last frame stored: per model its id, its views and their rows in all
 *   mmf_fusion_last_track_transforms   the transformations the last frame's models were initialised with (list order) */
typedef struct mmf_tracker mmf_tracker;
typedef struct {
    int iterations;
    float inlier_threshold, inlier_fraction;
} mmf_ransac_config;
int mmf_tracker_create(mmf_ctx *ctx, int width, int height, float fx, float fy, float cx, float cy, int capacity,
                       int max_keypoints, mmf_tracker **out);
void mmf_tracker_destroy(mmf_tracker *t);
int mmf_tracker_add_keypoints(mmf_tracker *t, int n, const int *xy, const float *descriptor, const float *depth,
                              long long timestamp, float min_feature_distance, int history);
int mmf_tracker_prune(mmf_tracker *t, int min_kps, long long min_time);
int mmf_tracker_associate(mmf_tracker *t, const uint8_t *mask, const int *model_ids, int n_models);
int mmf_tracker_associate_all(mmf_tracker *t, const int *model_ids, int n_models);
int mmf_tracker_forget_model(mmf_tracker *t, int model_id);
int mmf_tracker_last_pairs(mmf_tracker *t, const int *model_ids, int n_models, const float **p0, const float **p1,
                           const int **counts, int *stride);
int mmf_tracker_last_track_transform(mmf_tracker *t, int model_id, const mmf_ransac_config *cfg, float T[16], float *error,
                                     unsigned char *inlier, int *has_inlier);
int mmf_tracker_visible(mmf_tracker *t, int capacity, int *n, int *xy, float *coordinate, float *descriptor, long long *uid);
int mmf_tracker_status(mmf_tracker *t, int *n_tracks, int *length, int *dropped);
int mmf_tracker_download(mmf_tracker *t, int capacity, int *n_tracks, float *descriptor, int *age, int *nvalid,
                         long long *last_stamp, long long *uid, int *xy, float *coordinate, long long *timestamp, int *nonnull,
                         unsigned *member, int *label);
int mmf_tracker_last_launches(mmf_tracker *t);
int mmf_tracker_reset(mmf_tracker *t);
int mmf_tracker_set_view_log(mmf_tracker *t, int frames);
int mmf_tracker_frame(mmf_tracker *t);
int mmf_tracker_model_views(mmf_tracker *t, int model_id, int n_views, const int *frames, const float *poses,
                            const int **counts, const float **descriptor, const float **coordinate, int *missing);
int mmf_fusion_set_tracker(mmf_fusion *f, mmf_tracker *tracker, int odom_init_kp, int icp_refine);
int mmf_fusion_last_track_transforms(mmf_fusion *f, float *T, int capacity, int *n_out);
int mmf_fusion_last_stored_views(mmf_fusion *f, int *model_ids, int *n_views, int *rows, int capacity, int *n_out);
/* The add with the number of keypoints on the DEVICE: semantics and launches (7, 9 with the view log) of
 * mmf_tracker_add_keypoints, but the kernels read n from *n_dev, clamped to [0, max_keypoints]; nothing waits.  Grids and the
 * search's layouts are those of max_keypoints keypoints; rows k >= n of xy / descriptor (stale data of earlier frames)
 * enter no minimum, start no track and are not scattered: the table afterwards equals the host-n call's bit for bit.  The
 * host's bound of the track count grows by max_keypoints per such add (tightened by every call that waits); the padding
 * rows are fillers nothing matches.
 *   mmf_tracker_set_keypoint_status  a DEVICE int the device-count adds read from now on (NULL: none): while it is not 0 --
 *                       the keypoint source did not converge -- an add is a frame WITHOUT keypoints and counts as failed
 *   mmf_tracker_keypoint_failures    waits; such adds since creation / reset */
int mmf_tracker_add_keypoints_device(mmf_tracker *t, const int *n_dev, const int *xy, const float *descriptor,
                                     const float *depth, long long timestamp, float min_feature_distance, int history);
int mmf_tracker_set_keypoint_status(mmf_tracker *t, const int *status_dev);
int mmf_tracker_keypoint_failures(mmf_tracker *t, int *failures);
/* The keypoint front end INSIDE processFrame (MultiMotionFusion.cpp:223-248; off by default, sp = NULL switches it off, and
 * so does every mmf_fusion_set_tracker).  Needs an attached tracker (MMF_ERR_STATE otherwise, and with world > 1), a network
 * of the fusion's context that serves the frame size and returns no more keypoints than the tracker takes (MMF_ERR_INVALID).
 * With it on every mmf_fusion_process_frame* call first runs, on the frame's own device rgb (u8 x 3) and raw depth,
 * mmf_superpoint_get_features_device, the device-count add with the frame's timestamp (the network's status word attached)
 * and mmf_tracker_prune(prune_min_kps, max(timestamp - prune_window_ns, 0)): all enqueued, none awaited -- the frame's
 * first wait stays the pairs call of `-init kp`.  A frame for which the caller added keypoints itself: MMF_ERR_INVALID.
 * Off: nothing is enqueued, allocated or waited for.  Pyramid level 0 only, as the tracker. */
typedef struct {
    float conf_thresh;
    int nms_dist, border;
    float min_feature_distance;
    int history;
    int prune_min_kps;
    long long prune_window_ns;
} mmf_keypoint_frontend_config; /* defaults 0.015, 4, 4, 0.7, 30, 30, 1e9 */
int mmf_keypoint_frontend_default_config(mmf_keypoint_frontend_config *cfg);
int mmf_fusion_set_keypoint_frontend(mmf_fusion *f, mmf_superpoint *sp, const mmf_keypoint_frontend_config *cfg);

/* ---- RigidRANSAC for batches of independent problems on the device (csrc/ransac_kernels.hpp) ----
 * The contract, per problem and bit for bit: mmf_ransac_create(cfg); mmf_ransac_estimate(p0, p1, n, NULL, ...);
 * mmf_ransac_destroy -- a FRESH object per problem, no mask.  One wave per problem runs the arithmetic of the host class
 * (one source, csrc/rigid_ransac.hpp); the rows a hypothesis is fitted to come from a table the host builds at creation
 * with the class's own std::shuffle, so the device draws no random numbers.
 *   mmf_ransac_batch_create    3 <= max_points <= 1024, 1 <= cfg->iterations <= 32.  Builds and uploads the table (about
 *                         30 ms at 1024 points and 10 iterations: at creation, never per frame), allocates the results in
 *                         pinned memory.  Waits for the stream.
 *   mmf_ransac_batch_estimate  p0 / p1 = DEVICE [offsets[n_problems]][3], problem p = rows offsets[p] .. offsets[p + 1]
 *                         (HOST, offsets[0] = 0, ascending); results = HOST [n_problems]; inlier (optional) = HOST
 *                         [offsets[n_problems]], per problem over its HASH-SORTED rows like mmf_ransac_estimate's.  Sizes
 *                         are checked before anything is launched; a problem with fewer than 3 or more than max_points
 *                         rows gets its status (T identity, error +inf, no inliers) and leaves its neighbours alone.
 *                         One launch, one wait.
 *   mmf_ransac_batch_max_points / _last_launches   what the object was created with; launches of the last estimate
 * Test hooks: mmf_debug_hash_float = the restated std::hash<float> beside the library's; mmf_debug_ransac_core_host = one
 * problem through table + hash + sort + core on the host, outputs as mmf_ransac_estimate; mmf_debug_rounded_ops = out[i] =
 * op(a[i], b[i]) on the DEVICE as the core spells it: 0 sqrt (double), 1 / (double), 2 sqrt (float), 3 rintf, 4 / (float),
 * 5 float / int. */
#define MMF_RANSAC_OK 0
#define MMF_RANSAC_TOO_FEW 1  /* fewer than 3 correspondences */
#define MMF_RANSAC_TOO_MANY 2 /* more than max_points */
typedef struct mmf_ransac_batch mmf_ransac_batch;
typedef struct {
    float T[16];    /* row-major 4x4 of T_01; the all-points fit when no hypothesis was accepted */
    float error;    /* mean inlier distance of the best hypothesis, +inf when none was accepted */
    int n_inliers;  /* inliers of the best hypothesis, 0 when none */
    int has_inlier; /* 0: Result::inlier is empty */
    int status;     /* MMF_RANSAC_* */
} mmf_ransac_result;
int mmf_ransac_batch_create(mmf_ctx *ctx, const mmf_ransac_config *cfg, int max_points, mmf_ransac_batch **out);
void mmf_ransac_batch_destroy(mmf_ransac_batch *b);
int mmf_ransac_batch_estimate(mmf_ransac_batch *b, const float *p0_dev, const float *p1_dev, const int *offsets, int n_problems,
                              mmf_ransac_result *results, unsigned char *inlier);
int mmf_ransac_batch_max_points(mmf_ransac_batch *b);
int mmf_ransac_batch_last_launches(mmf_ransac_batch *b);
/* Back-dating (the tracker section above describes the calls): one entry of the pose list, oldest first.
 * Inside processFrame (off by default):
 *   mmf_fusion_set_track_backdating   history = 0 switches it off and frees what the setter made; 2 .. 256: the fusion creates
 *                         its batch object {10, 0.03, 0.6}, max_points 1024, HERE (never per frame) and, when a tracker is
 *                         attached, reserves its workspace.  MMF_ERR_STATE with world > 1.  With it on, a tracked frame whose
 *                         segmentation spawned a model this rank owns, with an attached tracker that keeps a view log, runs
 *                         mmf_tracker_backdate(new model's id, history) directly behind the frame's association (refineTrack-
 *                         Subset(segm_tracks[uid], globalModel, 2), MultiMotionFusion.cpp:596-599).  When the models' view-pose
 *                         lists are kept (redetection on), entries 0 .. len - 2 go in front of the spawn frame's own entry
 *                         and the list is trimmed to the log's length as before: the views the model stores on deactivation
 *                         reach back before the spawn.  The model's pose is NOT touched (the reference overrides it with a
 *                         near-identity; a spawned model's pose is the identity already).  Every other frame: nothing is
 *                         enqueued or awaited.
 *   mmf_fusion_last_backdated_poses   what the last mmf_fusion_process_frame* call back-dated: *model_id (-1: nothing) and its
 *                         entries; cleared at the start of every call */
typedef struct {
    int stamp;           /* the frame (mmf_tracker_frame counts them) */
    long long timestamp; /* of the add that logged it; 0 when the frame is not in the ring */
    int from;            /* ik: the entry this one is chained to (-1: entry 0) */
    int both;            /* tracks of the segment with a keypoint in both frames */
    int nvalid;          /* ... that are finite in both */
    int status;          /* MMF_RANSAC_* (entry 0: OK) */
    int host_estimated;  /* 1: more rows than the batch object takes, estimated by the same core on the host */
    float error;         /* as mmf_ransac_result's; +inf without an estimate */
    int n_inliers;
    float T[16];         /* T_01 of (from, this entry), p0 ~ T p1; identity without an estimate */
    float pose[16];      /* inverse(rel[len - 1]) rel[j]; the last entry's is exactly the identity */
} mmf_backdated_pose;
int mmf_tracker_backdate(mmf_tracker *t, int label, int history, mmf_ransac_batch *batch, mmf_backdated_pose *out, int capacity,
                         int *n_out);
int mmf_tracker_reserve_backdate(mmf_tracker *t, int history);
int mmf_tracker_backdate_rows(mmf_tracker *t, int entry, float *p0, float *p1, int capacity, int *n);
int mmf_fusion_set_track_backdating(mmf_fusion *f, int history);
int mmf_fusion_last_backdated_poses(mmf_fusion *f, int *model_id, mmf_backdated_pose *out, int capacity, int *n_out);
/* The view store with a verifier (keypoint redetection, above):
 *   mmf_viewstore_set_verifier   attaches a batch object (NULL detaches it; it belongs to the caller, shares the store's context
 *                         and outlives its attachment).  With one attached the store keeps its coordinates and its view table
 *                         on the device as well -- views stored before the call are uploaded here, growth copies them like the
 *                         descriptors and old buffers are kept until destroy -- and the match writes its rows to device memory
 *                         too.  Without one nothing of this is allocated, written or launched, and a match stays 3 launches.
 *   mmf_viewstore_best_match_device   the outputs of mmf_viewstore_best_match with coordinate = DEVICE [nq][3], nq <= max_points,
 *                         under the PER-VIEW rule: every view's estimate is that of a fresh RigidRANSAC{cfg of the batch
 *                         object} (mmf_viewstore_best_match runs ONE object's engine on from view to view).  The three match
 *                         launches, then a verify launch with grid = sets x views (views with fewer than 3 matches, empty
 *                         views and views of other models return at once) and a launch that picks per (set, model) the
 *                         smallest error over the model's views in ascending index, the first of equals, estimates without
 *                         inliers dropped: 5 launches whatever the store holds, one record through pinned memory, one wait.
 *                         MMF_ERR_STATE without a verifier.
 * Inside processFrame:
 *   mmf_fusion_set_redetection_verifier   mode 0 = host (default: the path of mmf_fusion_set_redetection, untouched), 1 =
 *                         device: the fusion creates a batch object {10, 0.03, 0.8}, max_points 1024, and attaches it to its
 *                         store.  A frame then stages the segments' coordinates with their descriptors and enqueues, behind
 *                         the matches of all segments, the two verification launches for ALL (segment, inactive model)
 *                         pairs before the one wait for the matches; the unchanged decision block reads the records (a model
 *                         that an earlier segment of the frame activated is skipped).  Still two waits per such frame.  A
 *                         segment with more than max_points finite keypoints is verified by the host core under the same
 *                         per-view rule and counted.  MMF_ERR_STATE with world > 1.
 *   mmf_fusion_redetection_host_verified  segments verified on the host in mode 1 since creation (-1: null) */
int mmf_viewstore_set_verifier(mmf_viewstore *vs, mmf_ransac_batch *b);
int mmf_viewstore_best_match_device(mmf_viewstore *vs, int model_id, const float *query, const float *coordinate, int nq,
                                    float T[16], float *error, int *inliers, int *view, int *n_matches, unsigned char *inlier,
                                    int *found);
int mmf_fusion_set_redetection_verifier(mmf_fusion *f, int mode);
int mmf_fusion_redetection_host_verified(mmf_fusion *f);
int mmf_debug_set_redetect_max_points(int max_points); /* the max_points of verifiers created from now on by the setter above (tests) */
/* The batch a frame's redetection runs (csrc/redetect_host.hpp: viewstore_batch_run, viewstore_batch_best), for the tests:
 * n_sets query sets of nq[s] rows, descriptor HOST [sum nq][256] / coordinate HOST [sum nq][3] with the sets behind one
 * another, against the n_asked models asked[].  rule 0 = host, one engine per (set, model); 1 = the device verifier
 * (MMF_ERR_STATE without one; a set beyond its max_points is verified by the host core and counted in *host_verified).
 * records OUT [n_sets * n_asked], pair (s, a) at s * n_asked + a, model_id = asked[a]; inlier OUT (optional)
 * [n_sets * n_asked][inlier_stride] over the hash-sorted matches, inlier_stride >= the largest set.  Launches as a frame's:
 * 3 per set, and 2 more under rule 1.  Synchronous. */
typedef struct {
    float T[16];
    float error;
    int inliers, view, n_matches, found, model_id;
} mmf_debug_redetect_record;
int mmf_debug_viewstore_best_match_batch(mmf_viewstore *vs, int n_sets, const int *nq, const float *descriptor,
                                         const float *coordinate, int n_asked, const int *asked, int rule,
                                         mmf_debug_redetect_record *records, unsigned char *inlier, int inlier_stride,
                                         int *host_verified);
int mmf_debug_hash_float(const float *x, int n, unsigned long long *restated, unsigned long long *libstdcxx);
int mmf_debug_ransac_core_host(const mmf_ransac_config *cfg, const float *p0, const float *p1, int n, float T[16], float *error,
                               unsigned char *inlier, int *has_inlier);
int mmf_debug_rounded_ops(mmf_ctx *ctx, int op, const void *a_dev, const void *b_dev, size_t n, void *out_dev);

/* ---- dense optical flow after Farneback (csrc/flow_kernels.hpp, csrc/flow_host.hpp) ------------------
 * The stage of the reference's flow_crf segmentation that turns a frame pair into a dense flow field
 * (Core/Segmentation/Segmentation.cpp:779-804: both frames scaled down by 4, cv::calcOpticalFlowFarneback(.., 0.2, 1, 20, 2,
 * 5, 15/50.0, 0)), as an engine of its own.  The flow_crf mode itself is NOT here.  The arithmetic is the one DESIGN.md 4.8
 * writes out -- Farneback's algorithm, one level, box window -- and tests/flow_oracle.py restates; parity with OpenCV is not
 * pinned.  Frames are DEVICE interleaved u8 RGB [height][width][3]; the flow image has w = width / div by h = height / div
 * pixels; prev(y, x) ~ next(y + flow.y, x + flow.x), in flow-image pixels.
 *   mmf_flow_default_config  div 4, levels 1, winsize 20, iterations 2, poly_n 5, poly_sigma 0.3
 *   mmf_flow_create          MMF_ERR_INVALID -- before any device is touched, never a fall back -- for levels != 1, div not in
 *                        {1, 2, 4}, a width or height div does not divide, a flow image under 8 x 8, winsize outside [2, 33],
 *                        poly_n outside [3, 7], iterations outside [1, 10], poly_sigma <= 0
 *   mmf_flow_compute         a stateless pair (it ends the sequence of mmf_flow_next: the buffers are shared)
 *   mmf_flow_next            the next frame of a sequence: the first call after create / reset / compute yields no flow
 *                        (*has_flow = 0), every later one the flow from the frame before it.  The engine keeps the last
 *                        frame's expansion: a frame pays stages 1-4 once.
 *   mmf_flow_result          DEVICE pointers: flow [h][w][2] = {x, y}, magnitude [h][w] = sqrtf(x x + y y), motion [h][w] =
 *                        clamp((magnitude - 0.2) / 4.8, 0, 1) (Segmentation.cpp:1193-1197); valid until the next compute /
 *                        next.  w, h are written in any case; MMF_ERR_STATE while there is no flow.
 *   mmf_flow_download        a stage image to HOST memory, for tests: "gray" / "smooth" (the latest frame; "gray0" / "smooth0":
 *                        the pair's first frame) u8 / f32 [h][w]; "R0" / "R1" (the pair's expansions) and "M" (the matrices
 *                        the last iteration read) f32 [h][w][5]; "flow_<i>" (behind iteration i) f32 [h][w][2]; "magnitude",
 *                        "motion".  bytes must be the image's size.  Synchronous.
 *   mmf_flow_tables          the tables the kernels read: g, xg, xxg [poly_n + 1], ig [4] = {ig11, ig03, ig33, ig55}
 *   mmf_flow_make_tables     the tables of an engine with (poly_n, poly_sigma): host arithmetic, no device
 *   mmf_flow_last_launches   kernel launches of the last compute / next: 1 + 2 * iterations for a pair (1 for the first frame
 *                        of a sequence), whatever the size
 * compute and next are asynchronous on the context's stream.
 * Inside processFrame:
 *   mmf_fusion_set_optical_flow   cfg != NULL: every frame's flow from the frame before it is computed from the frame's RGB by
 *                        an engine of the fusion's own (mmf_flow_next), on a stream of its own beside the tracking, behind the
 *                        point of the fusion's stream where the frame's RGB is on the device, and joined by the fusion's stream
 *                        before the call returns.  NULL (the default): off -- the engine, its stream and events are freed, and
 *                        no frame allocates, enqueues or waits for anything.  Poses, maps and masks are the same bits either
 *                        way.  mmf_fusion_reset starts a new sequence.  MMF_ERR_INVALID as mmf_flow_create; MMF_ERR_STATE on a
 *                        sharded fusion (world > 1).
 *   mmf_fusion_last_flow          the last call's flow (as mmf_flow_result; pointers into the fusion's engine, valid until the
 *                        next frame); *has_flow = 0 and null pointers after the first frame of a sequence.  MMF_ERR_STATE
 *                        while the hook is off. */
typedef struct mmf_flow mmf_flow;
typedef struct {
    int div;          /* the flow image is the frame scaled down by 1, 2 or 4 (area mean) */
    int levels;       /* 1 */
    int winsize;      /* the averaging window is (2 (winsize / 2) + 1)^2 */
    int iterations;
    int poly_n;       /* radius of the polynomial expansion */
    float poly_sigma; /* its Gaussian's standard deviation */
} mmf_flow_config;
int mmf_flow_default_config(mmf_flow_config *cfg);
int mmf_flow_create(mmf_ctx *ctx, int width, int height, const mmf_flow_config *cfg, mmf_flow **out);
void mmf_flow_destroy(mmf_flow *flow);
int mmf_flow_compute(mmf_flow *flow, const uint8_t *prev_rgb, const uint8_t *next_rgb);
int mmf_flow_next(mmf_flow *flow, const uint8_t *rgb, int *has_flow);
int mmf_flow_reset(mmf_flow *flow);
int mmf_flow_result(mmf_flow *flow, const float **flow_dev, const float **magnitude_dev, const float **motion_dev, int *w, int *h);
int mmf_flow_download(mmf_flow *flow, const char *name, void *host_dst, size_t bytes);
int mmf_flow_tables(mmf_flow *flow, float *g, float *xg, float *xxg, float *ig);
int mmf_flow_make_tables(int poly_n, float poly_sigma, float *g, float *xg, float *xxg, float *ig);
int mmf_flow_last_launches(mmf_flow *flow);
int mmf_fusion_set_optical_flow(mmf_fusion *f, const mmf_flow_config *cfg);
int mmf_fusion_last_flow(mmf_fusion *f, const float **flow_dev, const float **magnitude_dev, const float **motion_dev, int *w,
                         int *h, int *has_flow);

/* ---- the inference of the flow CRF (csrc/flowcrf_kernels.hpp, csrc/flowcrf_host.hpp) -----------------------
 * The stage of the reference's flow_crf segmentation that turns tracks, flow, depth and the models' predictions into fused label
 * probabilities and the MAP id image (Core/Segmentation/Segmentation.cpp:819-1263), as an engine of its own.  What follows it
 * in the reference (contours, the largest blob, ModelData, hasNewLabel; :1270-1324) is mmf_flowseg_*, the "flow_crf" mode
 * mmf_fusion_set_flow_segmentation (both below).  The arithmetic is the one DESIGN.md 4.9 writes out and tests/flowcrf_oracle.py restates.  The CRF image has
 * w = width / 4 by h = height / 4 cells, N = w h, and L = n_models + (allow_new ? 1 : 0) <= 32 labels, the new label last.
 *   (a) track errors   per model m and track k (Model::computeTrackProjectionStartEnd with length 2, Model.cpp:524-579): the
 *       start keypoint is the track's `prev` slot, the end its `cur` slot; a slot that is null, has stamp 0 or a non-finite
 *       coordinate gives no keypoint.  T_start[m] / T_end[m] (the reference's poses[-2] pose^-1 and poses.back() pose^-1) are
 *       widened to double and applied as ((r0 x + r1 y) + r2 z) + t; the pixel is round-half-away(c + (p.xy / p.z) f) in double.
 *       A track with a keypoint missing, a non-finite transformed coordinate or a pixel outside the frame is skipped (a pixel
 *       that is no number counts as outside).  v = |xy_end - xy_start| / ((t_end - t_start) 1e-9), the difference of the stamps
 *       as uint64_t, in double, rounded to float.  Its cell is (rint(x_end / 4), rint(y_end / 4)), half to even, its index
 *       cy w + cx AS THE REFERENCE WRITES IT: a column equal to w wraps into the next row, an index >= N is dropped (the
 *       reference writes out of bounds there).  Several tracks on a cell: the highest table index wins.  E [L][N] starts at +inf.
 *   (b) unaries        an active row's finite v becomes v > threshold ? 1 : 0; with allow_new the last row is any(v < threshold)
 *       over the active rows where all of them are finite, +inf elsewhere.  p = softmax(-E) per cell; a cell whose exp sum is
 *       not > 0 (all +inf, or a NaN from equal stamps) gets 1 / L.  U = -log p; +inf is legal and gives Q = 0.
 *   (c) projection     per model |depth - z| at (4x, 4y) (z = channel 2 of the model's [height][width][4] vertex image), min(.,
 *       max_err) (a NaN becomes max_err), exp(-d / max_err), divided by the sum over the models; 0 where depth < 1e-6 && z < 1e-6
 *       for any model, 0 where < min_proj_prob.  The new label's row is 0 (the reference leaves it uninitialised).
 *   (d) mean field     Q = softmax(-U); iterations x Q = softmax(-U + 4 weight_smoothness D_s K_s D_s Q + weight_appearance D_a K_a
 *       D_a Q), K = exp(-|f_i - f_j|^2 / 2) over EVERY pair (j = i included), D = 1 / sqrt(sum_j K_ij + 1e-20); smoothness
 *       features (x / 3, y / 3), appearance features ((float)(x / 40), (float)(y / 40)) -- integer divisions -- and 10 flow.
 *       The smoothness sum is evaluated separably and skips factors that are exactly 0 in float (|dx| or |dy| >= 44).
 *   (e) fusion         prob = 1 - (1 - Q motion)(1 - proj); label = the first maximum; ids [h][w] u8 = ids[label];
 *       ids_full [height][width] u8 = ids scaled up by 4, nearest (what mmf_mask_segment takes).
 *   mmf_flowcrf_default_config  div 4, iterations 10, weight_smoothness 40, weight_appearance 40, threshold 20 px/s, max_err 0.03 m,
 *                        min_proj_prob 0.3
 *   mmf_flowcrf_create       MMF_ERR_INVALID -- before any device is touched -- for div != 4, a width or height 4 does not divide,
 *                        max_labels outside [1, 32], iterations outside [0, 50], weights, threshold or max_err that are not
 *                        positive.  max_tracks: the most tracks (a tracker's capacity) an inference may be given.  fx .. cy: the
 *                        camera of the frame.  The image need not fit in LDS (1280 x 960 works).
 *   mmf_flowcrf_infer        one inference from plain DEVICE arrays of `count` tracks (tracks == NULL or count 0: no tracks, every
 *                        unary is log L).  Asynchronous on the context's stream; every input is read by the enqueued work.
 *   mmf_flowcrf_infer_tracker  the same from a tracker's table (its `cur` / `prev` slots: xy, coordinate, stamp, non-null flag;
 *                        the number of tracks is read on the device).  NULL: no tracks.
 *   mmf_flowcrf_result       DEVICE pointers, valid until the next inference: ids [h][w] u8, ids_full [height][width] u8, prob and
 *                        Q f32 [L][N].  w, h are written in any case; MMF_ERR_STATE before the first inference.
 *   mmf_flowcrf_download     a stage image to HOST memory, for tests: "E", "U", "proj", "Q", "prob" f32 [L][N]; "label" i32 [N];
 *                        "ids", "invalid" u8 [N]; "ids_full" u8 [height][width]; "cell" i32 [n_models][max_tracks] (a track's cell
 *                        index per model, -1: no sample).  Synchronous.
 *   mmf_flowcrf_last_launches  kernel launches of the last inference: 5 + 3 iterations (4 at iterations 0), plus one memset,
 *                        whatever the image size, the labels and the tracks.
 * Inside processFrame:
 *   mmf_fusion_set_flow_inference  cfg != NULL: every TRACKED frame that has a flow runs the inference where the reference
 *                        segments -- behind the tracking, on the predictions the frame was tracked against -- with the active
 *                        models in list order, the new label (id = the next model id) when enable_multiple_models is set (with
                        mmf_fusion_set_flow_segmentation on: when a model may spawn, see there),
 *                        T_start = prev pose^-1 and T_end = pose pose^-1 per model, and the attached tracker's table
 *                        (mmf_fusion_set_tracker; none: every unary is log L).  pose is the model's pose of this frame
 *                        (poses.back(): tracked, or with the tracker's icp_refine off the keypoint-initialised one), prev the
 *                        pose the frame before left it (poses[-2]) -- NOT Model::lastPose, which a keypoint initialisation
 *                        overrides with this frame's initial pose.  A model's first tracked frame has prev = the pose it
 *                        was created with.  It runs on the flow's stream behind the flow; the fusion's stream joins it before
 *                        the call returns.  Observational: poses, maps and masks are the same bits with it on or off, and it
 *                        fails no frame: one with more than 32 labels has no result.  NULL (the default): off -- the engine
 *                        and its events are freed and no frame allocates, enqueues or waits for anything.  MMF_ERR_INVALID
 *                        as mmf_flowcrf_create; MMF_ERR_STATE while the optical-flow hook is off, when it does not run at
 *                        div 4, and on a sharded fusion.  mmf_fusion_set_optical_flow(NULL) switches this hook off too; a
 *                        call that replaces the flow engine switches it on again with its configuration if the new engine
 *                        runs at div 4 (no result until the second frame), else leaves it off.
 *   mmf_fusion_last_flow_inference  the last call's id images (DEVICE pointers into the fusion's engine, valid until the next
 *                        frame): ids [h][w], ids_full [height][width]; *has_result = 0 and null pointers after the first frame
 *                        of a sequence, a frame that was not tracked or one with more than 32 labels.  MMF_ERR_STATE while
 *                        the hook is off.
 *   mmf_fusion_flow_inference_download  a stage image of that inference to HOST memory, as mmf_flowcrf_download, for tests.
 *                        MMF_ERR_STATE while the hook is off and after a frame without a result. */
typedef struct mmf_flowcrf mmf_flowcrf;
typedef struct {
    int div;        /* 4 */
    int iterations; /* mean-field updates */
    float weight_smoothness, weight_appearance;
    float threshold;     /* pixels per second: a track faster than this in a model's frame is that model's outlier */
    float max_err;       /* metres: the projection error is truncated here */
    float min_proj_prob; /* projection probabilities under this become 0 */
} mmf_flowcrf_config;
typedef struct {
    int n_models;             /* the active models, in list order; >= 1 */
    int allow_new;            /* append the new label */
    unsigned new_id;          /* its id */
    const unsigned char *ids; /* HOST [n_models] */
    const float *T_start;     /* HOST [n_models][16], row-major 4 x 4 */
    const float *T_end;       /* HOST [n_models][16] */
    const float *const *vertex; /* HOST array of n_models DEVICE pointers, f32 [height][width][4] each */
    const float *depth;       /* DEVICE f32 [height][width], metres */
    const float *flow;        /* DEVICE f32 [h][w][2] */
    const float *motion;      /* DEVICE f32 [h][w] (mmf_flow_result's third image) */
} mmf_flowcrf_input;
typedef struct {
    const int *xy_cur;         /* DEVICE [count][2] */
    const float *co_cur;       /* DEVICE [count][3] */
    const long long *ts_cur;   /* DEVICE [count] */
    const int *ok_cur;         /* DEVICE [count], 0: a null slot */
    const int *xy_prev;
    const float *co_prev;
    const long long *ts_prev;
    const int *ok_prev;
    int count;
} mmf_flowcrf_tracks;
int mmf_flowcrf_default_config(mmf_flowcrf_config *cfg);
int mmf_flowcrf_create(mmf_ctx *ctx, int width, int height, int max_labels, int max_tracks, float fx, float fy, float cx, float cy,
                       const mmf_flowcrf_config *cfg, mmf_flowcrf **out);
void mmf_flowcrf_destroy(mmf_flowcrf *fc);
int mmf_flowcrf_infer(mmf_flowcrf *fc, const mmf_flowcrf_input *in, const mmf_flowcrf_tracks *tracks);
int mmf_flowcrf_infer_tracker(mmf_flowcrf *fc, const mmf_flowcrf_input *in, mmf_tracker *tracker);
int mmf_flowcrf_result(mmf_flowcrf *fc, const uint8_t **ids_dev, const uint8_t **ids_full_dev, const float **prob_dev,
                       const float **q_dev, int *w, int *h, int *n_labels);
int mmf_flowcrf_download(mmf_flowcrf *fc, const char *name, void *host_dst, size_t bytes);
int mmf_flowcrf_last_launches(mmf_flowcrf *fc);
/* test hook: how the pair pass of (d) splits a cell's sum over j for an image of n_cells cells at a padded label width (1, 2,
 * 4, 8, 16 or 32): *nsplit ranges (the launch's grid.y), *nchunk chunks of 256 cells j, *per = ceil(nchunk / nsplit) chunks per
 * range; range s takes the chunks [s per, min(nchunk, (s + 1) per)) and is empty from s per >= nchunk on.  The launch's own
 * policy, not a copy of it; a host function: needs no device.  MMF_ERR_INVALID for any other width or n_cells < 1. */
int mmf_debug_flowcrf_pair_geometry(int n_cells, int padded_labels, int *nsplit, int *nchunk, int *per);
int mmf_fusion_set_flow_inference(mmf_fusion *f, const mmf_flowcrf_config *cfg);
int mmf_fusion_last_flow_inference(mmf_fusion *f, const uint8_t **ids_dev, const uint8_t **ids_full_dev, int *w, int *h,
                                   int *n_labels, int *has_result);
int mmf_fusion_flow_inference_download(mmf_fusion *f, const char *name, void *host_dst, size_t bytes);

/* ---- the blob stage of the flow_crf segmentation (csrc/flowseg_kernels.hpp, csrc/flowseg_host.hpp) ----------
 * What the reference does with the MAP id image of the inference (Core/Segmentation/Segmentation.cpp:1270-1324): the largest
 * blob per model, the filled contours, the resize, ModelData and hasNewLabel.  ids [h][w] u8 is what mmf_flowcrf_result hands
 * out (w = width / 4, h = height / 4), the label table is the models' ids in list order, then the new id with allow_new.
 *   (a) components     per id of the table the 8-connected components of ids == id; "component" = the raster index of a
 *       component's first cell, -1 for a cell whose id is not in the table (such a cell is never drawn).
 *   (b) area           area2 = 2 cv::contourArea of the component's outer border as cv::findContours(RETR_EXTERNAL,
 *       CHAIN_APPROX_NONE) follows it from that first cell: an integer.
 *   (c) winner         per id the component of maximal (area2, first cell): a tie -- all areas 0 included -- goes to the
 *       component found LAST in raster order, which is the first of OpenCV's contour list (not pinned).
 *       segm_count = rint(area2 / 2), half to even; an id without a cell has count 0 and draws nothing.
 *   (d) fill           the winner's cells and every cell its border polygon winds around (its holes and what lies in them); ids
 *       in ascending order onto a zero image, so a cell takes the highest id that covers it: segm [h][w] u8.
 *   (e) full           full [height][width] u8 = segm scaled by 4, nearest.
 *   (f) model data     per table entry: super_pixel_count = (unsigned)((float)segm_count 16.0f), avg_confidence, depth_mean =
 *       sum d / n and depth_std = sqrt(max(sum d^2 / n - mean^2, 0)) over the pixels full == id, zero depth included, in
 *       float64 and a fixed order (same input, same bits); both 0 for n = 0.
 *   (g) new label      has_new_label = allow_new && (float)count(segm == new_id) / (float)(w h) > new_model_size; when it is
 *       not, the new label's entry is dropped (n_entries = n_models).
 *   mmf_flowseg_default_config  div 4, new_model_size 0.05, avg_confidence 0.4, model_spawn_offset 22, inhibit_new 0
 *   mmf_flowseg_create       MMF_ERR_INVALID -- before any device is touched -- for div != 4, a width or height 4 does not
 *                        divide, max_labels outside [1, 32], new_model_size outside [0, 1), a negative model_spawn_offset.
 *   mmf_flowseg_run          asynchronous on the context's stream: ids_dev [h][w] u8 and depth_dev [height][width] f32 are
 *                        DEVICE images read by the enqueued work; ids_host = the n_models >= 1 model ids (HOST, distinct,
 *                        new_id not among them, new_id <= 255).  Eight kernel launches and two memsets whatever the image holds.
 *   mmf_flowseg_result       waits for the run; segm / full: DEVICE pointers valid until the next run; *summary: a copy of the
 *                        one pinned read.  w, h are written in any case; MMF_ERR_STATE before the first run.
 *   mmf_flowseg_download     a stage image to HOST memory, for tests: "component", "area2" (of the cell's component) i32 [h][w];
 *                        "winner" (1: the cell is of its id's winning component), "segm" u8 [h][w]; "full" u8 [height][width].
 *   mmf_flowseg_last_launches  kernel launches of the last run.
 * Inside processFrame (the reference's -segm_mode flow_crf):
 *   mmf_fusion_set_flow_segmentation  cfg != NULL: a frame that brings no segmentation of its own is segmented from the
 *                        flow-inference hook's id image, on the fusion's stream behind the inference, into the fusion's mask;
 *                        one host wait for the summary.  The inference then runs with allow_new = spawnOffset >=
 *                        cfg->model_spawn_offset (MultiMotionFusion.cpp:148) instead of enable_multiple_models; inhibit_new
 *                        clears has_new_label afterwards.  A frame without an inference result (an untracked frame, one
 *                        without a flow, one with more than 32 labels) gets a zero mask, no entries and no new label: nobody
 *                        is counted unseen, no max depth or confidence threshold moves (the reference reads modelData out of
 *                        bounds there).  NULL (the default): off, everything freed.  MMF_ERR_STATE while the flow-inference
 *                        hook is off and on a sharded fusion; switching the flow or the inference hook off -- or replacing the
 *                        flow engine -- switches this off too.
 *   mmf_fusion_last_flow_segmentation  what the last frame this path handled computed: *summary (has_new_label as
 *                        processFrame used it, after inhibit_new), *has_result = 0 for a frame without an inference result.
 *                        MMF_ERR_STATE before the first such frame. */
typedef struct mmf_flowseg mmf_flowseg;
typedef struct {
    int div;                /* 4 */
    float new_model_size;   /* the new label's share of the cells above which it spawns (0.05) */
    float avg_confidence;   /* every entry's avg_confidence (0.4) */
    int model_spawn_offset; /* frames between spawns (22); processFrame only */
    int inhibit_new;        /* setSetInhibit; processFrame only */
} mmf_flowseg_config;
typedef struct {
    int n_entries;          /* entries of models: the table's, without the new label's when has_new_label == 0 */
    int allow_new, has_new_label;
    unsigned new_cells;     /* count(segm == new_id); 0 without allow_new */
    mmf_segmentation_model models[32];
    int area2[32];          /* per table entry: the winner's 2 x contour area; 0: none */
    int first_cell[32];     /* ... and the raster index of its first cell; -1: the id has no cell */
} mmf_flowseg_summary;
int mmf_flowseg_default_config(mmf_flowseg_config *cfg);
int mmf_flowseg_create(mmf_ctx *ctx, int width, int height, int max_labels, const mmf_flowseg_config *cfg, mmf_flowseg **out);
void mmf_flowseg_destroy(mmf_flowseg *fs);
int mmf_flowseg_run(mmf_flowseg *fs, const uint8_t *ids_dev, const float *depth_dev, const unsigned char *ids_host, int n_models,
                    int allow_new, unsigned new_id);
int mmf_flowseg_result(mmf_flowseg *fs, const uint8_t **segm_dev, const uint8_t **full_dev, mmf_flowseg_summary *summary, int *w,
                       int *h);
int mmf_flowseg_download(mmf_flowseg *fs, const char *name, void *host_dst, size_t bytes);
int mmf_flowseg_last_launches(mmf_flowseg *fs);
int mmf_fusion_set_flow_segmentation(mmf_fusion *f, const mmf_flowseg_config *cfg);
int mmf_fusion_last_flow_segmentation(mmf_fusion *f, mmf_flowseg_summary *summary, int *has_result);

/* ---- the model database: savePly, cloud.ply / tracks.ply, -restore ----
 * Nothing here runs inside processFrame; every call is synchronous.
 *   mmf_model_export_cloud   Model::exportModelPLY's loop (Core/Model/Model.cpp:1547-1594) on the device: the surfels with
 *                         conf > conf_threshold (strict: NaN is dropped) in ascending index, each one packed little-endian
 *                         31-byte record {x y z f32 | r g b u8 | nx ny nz f32 | radius f32} in HOST memory.  Position =
 *                         ((p0 x + p1 y) + p2 z) + p3 per row p of the row-major pose, f32, no fused multiply-add; colour
 *                         c = (int)colour24, r = c >> 16 & 255, g = c >> 8 & 255, b = c & 255; normal =
 *                         -((r0 nx + r1 ny) + r2 nz) per row r of the pose's 3 x 3; radius copied.  *n_valid is always
 *                         written; capacity < *n_valid: MMF_ERR_INVALID and nothing is copied (mmf_model_count bounds
 *                         n_valid).  Reads the store only.  Three launches whatever the count:
 *   mmf_model_export_last_launches   the launches of the model's last export.
 *   mmf_model_export_ply     the same records, with the model's own confidence threshold, as a PLY file at `path`.
 *   mmf_ply_write_cloud / mmf_ply_read_cloud   the file: the reference's header byte for byte (:1516-1537), then n records.
 *                         The reader takes exactly that: any other header, a body that is not n records long, or
 *                         capacity < n is MMF_ERR_INVALID (*n is the file's count once the header has parsed).
 *   mmf_tracks_ply_write     a model's keypoint views (the mmf_viewstore_store layout) in the reference's binary tracks layout
 *                         with descriptors (:1386-1498), which Model::load reads (:1658-1691): track t = row t of every view
 *                         (entry i = the vertex of view i's row t, or 0xFFFFFFFF), vertices numbered track by track, then by
 *                         time index, each pose * coordinate in the arithmetic above, uint16 256, 256 f32; no edges.
 *   mmf_tracks_ply_read      what Model::load rebuilds: view i = the tracks with a keypoint at i, in track order.  *n_views
 *                         and *n_rows are always written for a well-formed file (a file without tracks has no views); NULL
 *                         destinations give the sizes only; too small a capacity, a list length other than 256 / n_views, a
 *                         vertex index >= the vertex count, a short file or trailing bytes: MMF_ERR_INVALID.
 *   mmf_viewstore_download_view   a view's rows back: HOST [rows][256] and [rows][3] (either may be NULL), without padding;
 *                         a bad index or capacity_rows < rows: MMF_ERR_INVALID.
 *   mmf_fusion_save_models   savePly (Core/MultiMotionFusion.cpp:1001-1018): for every active, then every inactive model,
 *                         with P = global pose * pose^-1: export_dir/cloud-<id>.ply, export_dir/model_db/model-<id>/cloud.ply
 *                         and, for a model with views in the fusion's store, .../tracks.ply.  Directories are created.
 *   mmf_fusion_load_models   loadModels (:131-145): for id = 1..255 ascending with a model_db/model-<id>/tracks.ply, an object
 *                         model with the next model id and conf_object_init, the file's views stored under that id, unseen
 *                         count -5, appended to the inactive list; no dense surfels.  A file that does not parse is skipped
 *                         and named by mmf_last_error.  MMF_ERR_STATE with world > 1.
 * Restoring a model's dense surfels (ours: the reference restores none):
 *   mmf_model_import_cloud   the inverse of mmf_model_export_cloud: record i of `host_records` (n records of 31 bytes, HOST
 *                         memory) becomes surfel i of the store, in file order.  With the row-major pose Q (NULL = identity,
 *                         the same arithmetic): position = ((q0 x + q1 y) + q2 z) + q3 per row q, normal =
 *                         -((r0 nx + r1 ny) + r2 nz) per row r of Q's 3 x 3 (the export negates, the import negates back),
 *                         f32, no fused multiply-add; radius copied; colour24 = (float)(r << 16 | g << 8 | b), the colour
 *                         vector's second component 0; confidence = `confidence`; initTime = timestamp = (float)time.
 *                         REPLACES the store's content (count = n; n = 0 empties it) and leaves the model as
 *                         mmf_model_upload_map leaves it for the same surfels.  n > the model's capacity: MMF_ERR_INVALID,
 *                         the store is untouched.  Synchronous (it first lets an in-flight count land); one launch whatever n:
 *   mmf_model_import_last_launches   the launches of the model's last import.
 *   mmf_model_import_ply     the file at `path` through mmf_ply_read_cloud, then the above.  A file that does not parse or holds
 *                         more records than the model holds surfels: MMF_ERR_INVALID, the store is untouched.
 *   mmf_model_set_timestamps   timestamp = (float)time for every surfel of the store; initTime and everything else stay.
 *                         Synchronous; one launch.  (combinedPredict / predictIndices drop a surfel with time - timestamp >
 *                         timeDelta: restored surfels are brought into the window of the frame that uses them; their initTime
 *                         still says when they were loaded.)
 *   mmf_fusion_load_models_ex   mmf_fusion_load_models with flags.  MMF_LOAD_DENSE: every model loaded from a tracks.ply also
 *                         gets the records of model_db/model-<id>/cloud.ply as surfels: Q = identity, confidence = the model's
 *                         threshold + 1, time = the fusion's tick at the call.  A missing cloud.ply, one that does not parse or
 *                         one with more records than the model holds leaves the model without surfels; it is loaded all the
 *                         same and mmf_last_error names the file.  When redetection activates such a model for the first time
 *                         its timestamps are set to the activating frame's tick: one launch on the model's stream, no wait.
 *                         mmf_fusion_load_models = flags 0.  Any other flag: MMF_ERR_INVALID.
 *   mmf_fusion_last_dense_restores   per model of the last load call with MMF_LOAD_DENSE, in load order.  *n is always the
 *                         number of entries, at most `capacity` are written.  Observational. */
#define MMF_LOAD_DENSE 1u
enum { MMF_DENSE_RESTORED = 0, MMF_DENSE_NO_FILE = 1, MMF_DENSE_NO_PARSE = 2, MMF_DENSE_TOO_LARGE = 3 };
typedef struct mmf_dense_restore {
    int model_id;      /* the id the model got in this fusion */
    unsigned surfels;  /* the surfels it got: the file's records, or 0 */
    int status;        /* MMF_DENSE_* */
} mmf_dense_restore;
int mmf_model_export_cloud(mmf_model *m, const float pose[16], float conf_threshold, void *host_records, unsigned capacity,
                           unsigned *n_valid);
int mmf_model_export_last_launches(mmf_model *m);
int mmf_model_export_ply(mmf_model *m, const char *path, const float pose[16]);
int mmf_ply_write_cloud(const char *path, const void *records, unsigned n);
int mmf_ply_read_cloud(const char *path, void *records, unsigned capacity, unsigned *n);
int mmf_tracks_ply_write(const char *path, int n_views, const int *counts, const float *descriptor, const float *coordinate,
                         const float pose[16]);
int mmf_tracks_ply_read(const char *path, int cap_views, int *n_views, int *counts, int cap_rows, int *n_rows, float *descriptor,
                        float *coordinate);
int mmf_viewstore_download_view(mmf_viewstore *vs, int view, int capacity_rows, float *descriptor, float *coordinate);
int mmf_fusion_save_models(mmf_fusion *f, const char *export_dir);
int mmf_fusion_load_models(mmf_fusion *f, const char *export_dir, int *n_loaded);
int mmf_model_import_cloud(mmf_model *m, const float pose[16], const void *host_records, unsigned n, float confidence, int time);
int mmf_model_import_last_launches(mmf_model *m);
int mmf_model_import_ply(mmf_model *m, const char *path, const float pose[16], float confidence, int time);
int mmf_model_set_timestamps(mmf_model *m, int time);
int mmf_fusion_load_models_ex(mmf_fusion *f, const char *export_dir, unsigned flags, int *n_loaded);
int mmf_fusion_last_dense_restores(mmf_fusion *f, mmf_dense_restore *out, int capacity, int *n);

/* ---- the fern keyframe database (csrc/ferns_kernels.hpp, csrc/ferns_host.hpp) ------------------------------
 * Stage one of relocalisation: ElasticFusion's randomised ferns (Core/Ferns.{h,cpp}) as an engine of its own -- the encoding
 * of a frame into fern codes, the database of keyframes, the rule that adds a frame (addFrame, Ferns.cpp:72-143) and the
 * search for the closest keyframe that is old enough (findFrame up to :203, with blockHDAware, :322-337).  What findFrame does
 * with that keyframe -- the fern odometry and its acceptance rule (:201-238), photometricCheck, the surface constraints --,
 * loss detection, the override of the pose, persistence and a sharded fusion are NOT here.  The arithmetic is the one
 * DESIGN.md 4.13 writes out and tests/ferns_oracle.py restates; the engine equals it bit for bit.
 * The inputs are a model's fill-in images as DEVICE images of the frame's size: image rgba8 [height][width][4], vert and norm
 * f32 [height][width][4] (mmf_model_texture "fillImage", "fillVertex", "fillNormal").  The small images have w = width / 8 by
 * h = height / 8 pixels; small pixel (i, j) is the source texel (texel((i + 0.5f) / w, width), texel((j + 0.5f) / h, height))
 * with texel(c, n) = clamp((int)floorf(c * (float)n), 0, n - 1) (GPUResize as DESIGN.md A3 restates it; rows are not flipped:
 * A7).  A fern is six int32 {x, y, t_r, t_g, t_b, t_d}: x in [0, w - 1], y in [0, h - 1], t_r, t_g, t_b in [0, 255], t_d in
 * [400, max_depth_mm] (millimetres; Ferns.cpp:21-70).  With v and p the small vertex and colour at (x, y) its code is
 *   (p.r > t_r) << 3 | (p.g > t_g) << 2 | (p.b > t_b) << 1 | (int(v.z * 1000.0f) > t_d)   when v.z > 0 (a NaN is not), else 255
 * -- one float multiplication, a truncating conversion; a product of 2^31 or more, where the reference's conversion is
 * undefined, counts as greater.  good = the number of codes that are not 255.  For a stored keyframe j
 *   co[j] = #{i : cur[i] != 255 and db[j][i] == cur[i]},   maxCo = (float)min(good_cur, good_j),
 *   dissim[j] = (maxCo - (float)co[j]) / maxCo   (one subtraction, one correctly rounded division; 0 / 0 is NaN, which no
 *   comparison accepts).
 * add:  minimum = FLT_MAX, lowered by strict < over every j in ascending order, and only if good_cur > 0; the frame becomes
 *   keyframe n iff (minimum > threshold || n == 0) && good_cur > 0, with its codes, good, pose, time and small images.
 * find: the same minimum over the j with time - time_j > min_time_gap; the lowest such j on a tie, -1 if there is none;
 *   similarity = (codes equal among the ferns good in both) / (float)(ferns good in both), NaN when there are none; the
 *   keyframe is a candidate iff similarity > min_similarity.
 * Unlike the reference's the database has a capacity: a frame the add rule accepts while it is full is dropped and counted.
 * The reference seeds its ferns with time(0): there is nothing to be equal to, so the table comes from the caller.
 *   mmf_ferns_default_config num 500 (MultiMotionFusion.cpp:33), max_depth_mm 15000 (:33: depthCut * 1000, with the GUI's depth
 *                        cutoff of 15 m, GUI/Tools/GUI.h:203, MainController.cpp:515), capacity 1024, min_time_gap 300
 *                        (Ferns.cpp:193), threshold 0.3095 (MultiMotionFusion.h:57), min_similarity 0.3 (Ferns.cpp:203)
 *   mmf_ferns_make_table a table of num ferns for w x h small images from `seed`, deterministically (a splitmix64 sequence,
 *                        per fern x, y, t_r, t_g, t_b, t_d, each lo + next % (hi - lo + 1)): host arithmetic, no device
 *   mmf_ferns_create     MMF_ERR_INVALID -- before any device is touched -- for a width or height under 8, num outside
 *                        [1, 16384], max_depth_mm < 400, capacity < 1, a NaN threshold, a null table or a fern outside its
 *                        ranges.  The table is copied.  Device memory: capacity * (num + w h 36) bytes and change.
 *   mmf_ferns_reset      empties the database and zeroes the drop count
 *   mmf_ferns_set_threshold   the threshold of the add rule from the next process call on (the reference hands it to every
 *                        addFrame call)
 *   mmf_ferns_process    flags MMF_FERNS_FIND, MMF_FERNS_ADD or both; with both the frame is encoded and searched once and find
 *                        sees the database before this frame's add.  Asynchronous on the context's stream: three launches
 *                        whatever num, the number of keyframes and the size, no host wait, no copy to the host; the number of
 *                        keyframes and the drop count live on the device and the decision to append is taken there.  pose: 16
 *                        floats, row major.  MMF_ERR_INVALID for a null image or pose and for flags outside {1, 2, 3}.
 *   mmf_ferns_result     the last process call's record, through pinned memory; waits for the stream.  Without MMF_FERNS_ADD
 *                        add_minimum is FLT_MAX and added 0; without MMF_FERNS_FIND closest is -1.  closest_dissim is FLT_MAX
 *                        and closest_similarity, closest_pose and closest_time are 0 while closest is -1.  MMF_ERR_STATE before
 *                        the first process call (and after a reset).
 *   mmf_ferns_keyframe   keyframe id: DEVICE pointers to its small images -- image rgba8 [h][w][4], vert and norm dense f32
 *                        [h][w][4], as mmf_odom_init_icp_model / mmf_odom_init_icp_from_prediction take them -- its pose,
 *                        time and good codes.  Any out pointer may be NULL.  Waits for the stream; MMF_ERR_INVALID for an id
 *                        that is not stored.  The pointers stay valid until the engine is destroyed.
 *   mmf_ferns_download   to HOST memory, for tests: "image" u8 [h][w][4], "vert" / "norm" f32 [h][w][4], "codes" u8 [num] (the
 *                        current frame); "co" i32 / "dissim" f32 [capacity] (the last search: entries from the count at that
 *                        search on are stale); "db_codes" u8 [capacity][num], "db_times" / "db_good" i32 [capacity].  bytes
 *                        must be the array's size.  Synchronous.
 *   mmf_ferns_last_launches   kernel launches of the last process call: 3
 * Inside processFrame (off by default):
 *   mmf_fusion_set_fern_database  cfg != NULL: behind the end-of-frame predict(), where the reference's processFerns() stands
 *                        (MultiMotionFusion.cpp:824; commented out there), every frame runs process(FIND | ADD) on the camera
 *                        model's fill-in images, its pose and the frame's tick, in an engine of the fusion's own (a second call
 *                        replaces it), on a stream of its own behind the point of the camera model's stream where those images
 *                        are complete, joined by the fusion's stream before the call returns.  table == NULL: the table of
 *                        mmf_ferns_make_table with seed 0.  The reference's findFrame reads the images of the mid-frame predict()
 *                        (:675-685), which this library does not enqueue: the hook queries the end-of-frame images instead.
 *                        Observational: poses, maps and masks are the same bits either way.  NULL (the default): off -- the
 *                        engine, its stream and events are freed and no frame allocates, enqueues or waits for anything.
 *                        mmf_fusion_reset empties the database.  MMF_ERR_INVALID as mmf_ferns_create; MMF_ERR_STATE on a
 *                        sharded fusion (world > 1; mmf_fusion_set_shard refuses a fusion with the hook on) and on a fusion
 *                        whose camera model has no fill-in.
 *   mmf_fusion_last_fern_result   as mmf_ferns_result, for the last frame.  MMF_ERR_STATE while the hook is off and before the
 *                        first frame.
 *   mmf_fusion_fern_database      the hook's engine (for mmf_ferns_keyframe, mmf_ferns_download), NULL while the hook is off */
#define MMF_FERNS_FIND 1
#define MMF_FERNS_ADD 2
typedef struct mmf_ferns mmf_ferns;
typedef struct {
    int num;              /* ferns */
    int max_depth_mm;     /* the upper end of a fern's depth threshold, millimetres */
    int capacity;         /* keyframes */
    int min_time_gap;     /* find: only keyframes with time - time_j > min_time_gap */
    float threshold;      /* add: the frame is kept when its lowest dissimilarity is above this */
    float min_similarity; /* find: the closest keyframe is a candidate above this */
} mmf_ferns_config;
typedef struct {
    int added;           /* this frame became keyframe count - 1 */
    int dropped_total;   /* frames the add rule accepted while the database was full, since creation / reset */
    int count;           /* keyframes stored, behind this call */
    int good_codes;      /* of the current frame */
    float add_minimum;   /* add's minimum; FLT_MAX when no keyframe lowered it */
    int closest;         /* find's keyframe, -1: none */
    float closest_dissim;
    float closest_similarity;
    int candidate;       /* closest >= 0 and closest_similarity > min_similarity */
    float closest_pose[16];
    int closest_time;
} mmf_ferns_result_t;
int mmf_ferns_default_config(mmf_ferns_config *cfg);
int mmf_ferns_make_table(unsigned long long seed, int num, int w, int h, int max_depth_mm, int *table_out);
int mmf_ferns_create(mmf_ctx *ctx, int width, int height, const mmf_ferns_config *cfg, const int *table, mmf_ferns **out);
void mmf_ferns_destroy(mmf_ferns *ferns);
int mmf_ferns_reset(mmf_ferns *ferns);
int mmf_ferns_set_threshold(mmf_ferns *ferns, float threshold);
int mmf_ferns_process(mmf_ferns *ferns, const void *image_rgba_dev, const void *vert_dev, const void *norm_dev, const float pose[16],
                      int time, int flags);
int mmf_ferns_result(mmf_ferns *ferns, mmf_ferns_result_t *out);
int mmf_ferns_keyframe(mmf_ferns *ferns, int id, const void **image_dev, const void **vert_dev, const void **norm_dev, float pose[16],
                       int *time, int *good_codes);
int mmf_ferns_download(mmf_ferns *ferns, const char *name, void *host_dst, size_t bytes);
int mmf_ferns_last_launches(mmf_ferns *ferns);
int mmf_fusion_set_fern_database(mmf_fusion *f, const mmf_ferns_config *cfg, const int *table);
int mmf_fusion_last_fern_result(mmf_fusion *f, mmf_ferns_result_t *out);
mmf_ferns *mmf_fusion_fern_database(mmf_fusion *f);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HIP_H_ */
