/*
 * vislam_hip.h -- C ABI of the MI355X-native visual front-end (libvislam_hip.so).
 *
 * This is the drop-in boundary for the Camera/Matcher/RANSAC hot path of
 * MecatronicaUSB/vi-slam.  The reference has no FFI of its own: its "GPU path" is
 * three C++ classes that call OpenCV's CUDA module.  Every entry point below
 * replaces one of those OpenCV(-CUDA) call sites; the reference file:line it
 * replaces is cited next to it.  The C++ adapter classes in vi-slam_amd/host/ keep
 * the reference's CameraGPU / MatcherGPU / VISystemGPU surface on top of this ABI.
 *
 * Conventions
 *   - plain C, no torch / OpenCV types; pointers + sizes only.
 *   - return value: VIS_OK (0) or a negative VIS_E_* code; never throws, never exits
 *     (reference convention is cout+exit / cv::Exception; adapters decide).
 *   - a vis_ctx is bound to ONE device and is NOT thread-safe (the reference is
 *     single-threaded, one frame in flight: src/main_vi_slamGPU.cpp:118-123).
 *   - "host" pointers are ordinary CPU memory; "dev" pointers are HIP device
 *     memory on the context's device (e.g. torch tensor .data_ptr()).
 *   - all functions are synchronous w.r.t. their host outputs unless they say
 *     "async": those enqueue on the context stream (vis_set_stream) and return.
 */
#ifndef VISLAM_HIP_H_
#define VISLAM_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIS_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------- */
enum {
    VIS_OK = 0,
    VIS_E_INVALID = -1,     /* bad argument / shape                            */
    VIS_E_NODEVICE = -2,    /* no HIP device (reference: main_vi_slamGPU.cpp:44-48 returns -1) */
    VIS_E_HIP = -3,         /* a HIP runtime call failed (see vis_last_error)  */
    VIS_E_CAPACITY = -4,    /* caller buffer too small / internal cap exceeded */
    VIS_E_STATE = -5,       /* call order wrong (e.g. slot empty, no plan)     */
    VIS_E_NOMEM = -6
};

/* ---- POD layouts crossing the ABI --------------------------------------- */
/* same field order and size (28 B) as cv::KeyPoint (Frame::keypoints, include/Camera.hpp:50) */
typedef struct vis_keypoint {
    float x, y;          /* level-0 pixel coordinates                            */
    float size;          /* 31 * scale(octave)                                   */
    float angle;         /* degrees [0,360)                                      */
    float response;      /* Harris response                                      */
    int32_t octave;      /* pyramid level                                        */
    int32_t class_id;    /* -1                                                   */
} vis_keypoint;

/* same field order and size (16 B) as cv::DMatch (Matcher::matches, include/Matcher.hpp:52) */
typedef struct vis_dmatch {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;      /* Hamming distance as float, like BFMatcher           */
} vis_dmatch;

enum { VIS_SYM_REFERENCE_EFFECTIVE = 0,  /* mutual best + ratio on direction 1 only:
                                            what src/Matcher.cpp:96-144 effectively does */
       VIS_SYM_INTENDED = 1 };           /* ratio on both directions + mutual best      */

enum { VIS_DESC_BYTES = 32, VIS_MAX_LEVELS = 16, VIS_MAX_GRID_ROOT = 32 };

/* One POD with every knob of the path.  Defaults (vis_default_params) are the
 * reference's hard-coded constants; see SURVEY.md section 5 "Config / flags". */
typedef struct vis_params {
    /* ORB -- cv::ORB::create(nfeatures) defaults; src/Camera.cpp:127 (200), src/CameraGPU.cpp:99 (1000) */
    int32_t nfeatures;        /* 1000 */
    int32_t nlevels;          /* 8    */
    float   scale_factor;     /* 1.2f */
    int32_t edge_threshold;   /* 31   */
    int32_t patch_size;       /* 31   */
    int32_t fast_threshold;   /* 20   */
    /* matcher post-filters -- src/Matcher.cpp:103 (0.8f), calibration/calibrationEUROC.xml:54 (49) */
    /* ratio: any float, taken as written -- a match survives iff !(d0 > (double)ratio * d1), so 0 keeps only d0 = 0, a negative ratio
     * only d0 = d1 = 0, NaN and +inf every match that has two neighbours (tests/match_param_cases.py).
     * n_cells: the grid is floor(sqrt(n_cells)) squared and that root is at most VIS_MAX_GRID_ROOT, i.e. 1 <= n_cells <=
     * 1088; a larger n_cells is refused by vis_set_params (VIS_E_INVALID, vis_last_error names the limit), never clamped to another
     * grid.  sym_mode: one of VIS_SYM_*, anything else is refused. */
    float   ratio;            /* 0.8f */
    int32_t n_cells;          /* 49   */
    int32_t w_size, h_size;   /* Matcher::setImageDimensions, src/Matcher.cpp:30-34; >= 1 */
    int32_t sym_mode;         /* VIS_SYM_* */
    /* essential RANSAC -- src/VISystem.cpp:1680 (prob 0.999, thr 1.0); OpenCV 3.2 maxIters = 1000 */
    double  ransac_prob;      /* 0.999 */
    double  ransac_threshold; /* 1.0 px; 1e-18 <= ransac_threshold / fx <= 1e18, else vis_set_params refuses it: 0 and NaN accept
                               * nothing, +inf everything, a negative value is its positive twin squared (tests/test_ransac_params_ref.py) */
    int32_t ransac_max_iters; /* 1000 */
    int32_t ransac_adaptive;  /* 1 = OpenCV adaptive stop, 0 = always max_iters (timing runs) */
    uint64_t ransac_seed;     /* 0xFFFFFFFFFFFFFFFF = cv::RNG((uint64)-1) */
    /* intrinsics -- calibration/calibrationEUROC.xml:20 */
    double  fx, fy, cx, cy;
    /* F2FRansac -- src/VISystem.cpp:709 (1000 iterations), :523 (threshold 370) */
    int32_t f2f_iters;        /* 1000 */
    double  f2f_threshold;    /* 370; any double, compared as written (error < threshold): NaN counts nothing, 0 and a negative value only an
                               * |x| that rounding left above 1, +inf every correspondence with a usable normal (tests/test_ransac_params_gpu.py) */
    /* which correspondences the batched pose stage consumes: the reference pipeline feeds the grid-filtered good
     * matches (Frame::next/prevGoodMatches, src/VISystem.cpp:1673-1674); BASELINE config 3 asks for RANSAC on the
     * un-gridded symmetric matches (M up to N) */
    int32_t pose_input;       /* VIS_POSE_GOOD */
    /* Device capacity for the keypoints of ONE frame; 0 = the default, sum over the levels of quota + quota/8 + 32.
     * KeyPointsFilter::retainBest keeps EVERY keypoint tied at its cut, so an image of identical corners (a calibration
     * checkerboard) yields more than nfeatures keypoints.  Beyond the capacity a call returns VIS_E_CAPACITY (never a silent cut);
     * the single-frame entry vis_orb_detect_compute grows the capacity itself up to the `cap` its caller passes. <= 65535. */
    int32_t keypoint_capacity;
    /* Keyframe gate of the batched stream path (vis_batch_run; the frame-at-a-time entry points ignore it).  0 = off: frame i is
     * matched against frame i-1 whatever it detected.  K >= 1: a frame is SAVED (CameraGPU::addGPUKeyframe, src/CameraGPU.cpp:138-173)
     * when its keypoint count is > K -- > 1 for the first frame saved after vis_batch_plan / vis_batch_reset (src/Camera.cpp:225,
     * src/CameraGPU.cpp:164) -- and every saved frame is matched against the last saved one (frameList.back(), :128-129).  K = 1 is
     * the GPU main's rule, K = 10 the CPU main's (Camera::addKeyframe, src/Camera.cpp:197-235).  0 ... 65535. */
    int32_t keyframe_min_points;  /* 0 */
} vis_params;
enum { VIS_POSE_GOOD = 0, VIS_POSE_SYM = 1 };

/* wall-clock of the last call's device work, from hipEvents on the context stream
 * (mirrors the elapsed_* members, include/Camera.hpp:121-126, include/Matcher.hpp:63-66) */
typedef struct vis_timings {
    float ms_total;
    float ms_pyramid;      /* resize chain                     */
    float ms_fast;         /* FAST score + NMS, all levels     */
    float ms_select;       /* histogram cut + Harris + top-N   */
    float ms_describe;     /* IC angle + blur + rBRIEF         */
    float ms_knn;          /* both knn directions              */
    float ms_filter;       /* ratio/sym/sort/grid              */
    float ms_pose;         /* essential RANSAC + recoverPose   */
    int32_t launches_fast; /* number of FAST kernel launches in the last call */
    int32_t launches_total;
    float ms_update;       /* Camera::Update half pyramid (VIS_STAGE_UPDATE), 0 when the stage did not run */
    float reserved_;
} vis_timings;

typedef struct vis_ctx vis_ctx;

/* ---- lifetime ------------------------------------------------------------ */
const char* vis_version(void);
const char* vis_strerror(int code);
/* replaces cv::cuda::getCudaEnabledDeviceCount(), src/main_vi_slamGPU.cpp:41 */
int  vis_device_count(void);
/* PCI address "dddd:bb:dd.f" of HIP device `device` (len >= 16): the multi-GPU launchers gather it per rank (generalises the device
 * selection of src/main_vi_slamGPU.cpp:41-43: N ranks must sit on N different devices) */
int  vis_device_pci_bus_id(int device, char* out, int len);
/* replaces cv::cuda::setDevice(0), src/main_vi_slamGPU.cpp:43, plus object construction */
int  vis_create(int device, vis_ctx** out);
void vis_destroy(vis_ctx* ctx);
const char* vis_last_error(vis_ctx* ctx);
void vis_default_params(vis_params* p);
/* replaces cuda::ORB::create(1000) (src/CameraGPU.cpp:99), createBFMatcher(NORM_HAMMING)
 * (src/MatcherGPU.cpp:30), Matcher::setImageDimensions (src/Matcher.cpp:30-34) */
int  vis_set_params(vis_ctx* ctx, const vis_params* p);
int  vis_get_params(vis_ctx* ctx, vis_params* p);
/* Enqueue on this hipStream_t from now on (e.g. the cuda_stream handle of a torch.cuda.Stream() the caller produces its inputs on).
 * NULL -- the handle 0 -- selects the context's OWN stream, which is created hipStreamNonBlocking: it is ordered with NOTHING of the
 * caller's, in particular not with the legacy default stream, whose handle is 0 too.  The default stream (torch.cuda.default_stream(),
 * what torch.cuda.current_stream() is unless the caller changed it) can therefore NOT be passed: a caller that works on it either moves
 * its producers and consumers to a stream of its own and passes that one, or synchronises the host around the library's calls.
 * Synchronises: everything queued through the stream set before, and on the context's other streams, is complete when this returns.
 * The stream must outlive the context (vis_destroy synchronises it) or be unset first (vis_set_stream(ctx, NULL)).
 *
 * Streams.  "The context's stream" below is the stream set here (or the own one).  The context has three more, all non-blocking:
 * an update stream (half pyramid / gradients of vis_batch_run), the match stream and the pose stream.  Every asynchronous call falls
 * into one of three classes (DESIGN.md has the table, one row per entry point; tests/test_caller_stream_gpu.py checks it):
 *   1. Calls on the context's stream -- vis_gradient_batch, vis_align_batch, vis_klt_batch, vis_f2f_batch, vis_filter_keypoints_batch,
 *      vis_homography_batch / _pose_batch / _polish_batch, vis_pnp_batch, vis_essential_batch / _refine_batch / _polish_batch,
 *      vis_ftrack_link_rows, vis_ftrack_triangulate_rows, vis_scale_link_rows, vis_trajectory_rows, vis_imu_preintegrate_rows, vis_rectify_batch (and vis_synth_frames_device, which is ordered the same way
 *      but blocks the host: see there).  They run in stream order: they wait
 *      for whatever the caller queued on that stream before the call (the producers of their device inputs), and their outputs may be
 *      read by anything queued on that stream after the call -- no host synchronisation on either side.  Those that write buffers an
 *      alignment on the pose stream may still read (vis_gradient_batch, vis_rectify_batch) wait for it first.
 *   2. vis_batch_run / vis_batch_run_guided.  The detect chain runs on the context's stream, so d_frames may be produced on that stream
 *      right before the call; the half pyramid and the gradients run on the update stream, which forks from the context's stream and
 *      is joined by it before the call returns, so d_frames may be overwritten by work queued on the context's stream after the call.
 *      The matcher (match stream; it reads vis_batch_run_guided's d_rot) and the pose stage (pose stream) are ordered behind the detect
 *      chain, hence behind what the caller queued before, and are NOT joined: results, vis_batch_half_pyramid, vis_batch_gradients and
 *      every getter are read after vis_batch_sync (or through a getter, which synchronises); d_rot is in use until then.
 *   3. Follow-ups of the last vis_batch_run on the pose stream.  vis_batch_align, vis_batch_track, vis_batch_klt, vis_batch_f2f,
 *      vis_batch_filter_keypoints, vis_batch_homography / _pose / _polish, vis_batch_pnp, vis_batch_essential_refine / _polish,
 *      vis_batch_ftrack_triangulate, vis_batch_scale_links, vis_batch_trajectory, vis_batch_imu, and vis_batch_ftrack when it is given a d_mask, FORK from the context's stream: they wait for what
 *      was queued on it before the call, so their caller device inputs may be produced there.  vis_batch_triangulate,
 *      vis_batch_triangulate_from and vis_batch_ftrack without a mask do NOT wait for the context's stream: what they read from caller
 *      buffers must be complete (or have been written by an earlier follow-up, which the pose stream orders).  None of them is joined
 *      back: caller buffers are in use, and outputs are read, after vis_batch_sync.  vis_batch_results_async likewise. */
int  vis_set_stream(vis_ctx* ctx, void* hip_stream);
int  vis_last_timings(vis_ctx* ctx, vis_timings* t);
/* per-level geometry the context derived from params for a w x h input
 * (ORB_Impl::detectAndCompute level sizes / quotas) */
int  vis_level_geometry(vis_ctx* ctx, int w, int h, int32_t* widths, int32_t* heights,
                        float* scales, int32_t* quotas);

/* ---- single-frame API: one call per OpenCV(-CUDA) call site --------------- */
/* Sizes of Camera::Update's levels (src/Camera.cpp:68-70: resize(prev, next, Size(), 0.5, 0.5)): cv::resize takes
 * dsize = cvRound(size * 0.5) -- round half to EVEN: 135 -> 68, 137 -> 68 -- so a level can be one row / column larger than the
 * reference's own bookkeeping `w_size[0] >> lvl` (src/Camera.cpp:42-47; 1080 -> 540, 270, 135, 68 against 67).  Both exist
 * here as they do there: buffers, strides, the gradients and the alignment's test of a WARPED point (src/VISystem.cpp:1299:
 * `y2 < image2.rows && x2 < image2.cols`) follow these sizes; the patch builders bound the candidate points they emit by `>> lvl`
 * like the reference.  For sizes that halve exactly four times (752x480) they coincide. */
void vis_half_pyramid_dims(int w, int h, int32_t lw[5], int32_t lh[5]);
/* Camera::Update, src/Camera.cpp:63-72: copy + 4x half-resolution levels.
 * out_levels[l] (l=1..4) receives lw[l]*lh[l] bytes (vis_half_pyramid_dims), tightly packed; out_levels[0] may be NULL.
 * With scale exactly 2 cv::resize(INTER_LINEAR) runs its area-fast path: (a+b+c+d+2)>>2 over every complete 2x2 block; where a
 * level is one larger than half of an odd source size, the last column / row averages the pixels that exist
 * (saturate_cast<uchar>((float)sum / count), round half to even).  16 <= w, h <= 4095 (a level may be one pixel wide or high:
 * 16 -> 8 -> 4 -> 2 -> 1); outside that VIS_E_INVALID, with a text in vis_last_error. */
int  vis_camera_update(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride,
                       uint8_t* const out_levels[5]);
/* replaces frameGPU.upload + cuda::ORB::detectAndCompute + descriptorsGPU.download,
 * src/CameraGPU.cpp:81,99-103 (CPU twin: src/Camera.cpp:87).  Keypoints/descriptors stay
 * resident in device slot `frame_slot` for the matcher (Frame list, include/Camera.hpp:104). */
int  vis_orb_detect_compute(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride,
                            int frame_slot, vis_keypoint* kps_out, uint8_t* desc_out,
                            int cap, int* n_out);
/* replaces descriptorsGPU[0/1].upload + 2x cuda knnMatch(k=2), src/MatcherGPU.cpp:49-56
 * (CPU twin src/Matcher.cpp:86,88).  out12: n_q x 2, out21: n_t x 2 (missing neighbours:
 * trainIdx = -1).  n_q/n_t are the slots' keypoint counts. */
int  vis_bf_knn2_hamming(vis_ctx* ctx, int slot_q, int slot_t,
                         vis_dmatch* out12, vis_dmatch* out21);
/* same, on caller-provided host descriptor arrays (n x 32 bytes) */
int  vis_bf_knn2_hamming_host(vis_ctx* ctx, const uint8_t* desc_q, int n_q,
                              const uint8_t* desc_t, int n_t,
                              vis_dmatch* out12, vis_dmatch* out21);
/* fused Matcher::computeBestMatches (ratio, symmetry, y-sort, grid-cell best),
 * src/Matcher.cpp:353-367 -> 96-244; writes goodMatches (<= root^2).  Also returns the
 * symmetric matches when sym_out != NULL (Matcher::matches, capacity sym_cap). */
int  vis_good_matches(vis_ctx* ctx, int slot_prev, int slot_cur,
                      vis_dmatch* good, int cap, int* n_good,
                      vis_dmatch* sym_out, int sym_cap, int* n_sym);
/* same filter chain on host-provided knn results + keypoints (unit-testable piece) */
int  vis_good_matches_host(vis_ctx* ctx, const vis_keypoint* kps1, int n1,
                           const vis_keypoint* kps2, int n2,
                           const vis_dmatch* knn12, const vis_dmatch* knn21,
                           vis_dmatch* good, int cap, int* n_good,
                           vis_dmatch* sym_out, int sym_cap, int* n_sym);
/* replaces cv::findEssentialMat(p1,p2,focal,pp,RANSAC,0.999,1.0), src/VISystem.cpp:1679-1680.
 * p1xy/p2xy: m x 2 floats (pixels).  E row-major. mask may be NULL.
 * Per-point test: (float)(s s / den) <= (float)thr^2 (s = x2^T E x1, den the Sampson denominator).  A correspondence with a NaN or an infinite
 * coordinate is no inlier of any model (s s / den is NaN: a NaN fails; the kernel's division-free shortcut asks for a finite right-hand side,
 * so inf <= inf does not pass); rows made of such correspondences alone give no model: E all zero, n_inliers 0, iters_run = the cap. */
int  vis_essential_ransac(vis_ctx* ctx, const float* p1xy, const float* p2xy, int m,
                          double E[9], uint8_t* mask, int* n_inliers, int* iters_run);
/* replaces cv::recoverPose(E,p1,p2,R,t,focal,pp), src/VISystem.cpp:1701.
 * A zero or rank-1 E -- such as the E vis_essential_ransac returns when it finds no model -- yields
 * NaN R, NaN t and n_good = 0 (the return code is still VIS_OK). */
int  vis_recover_pose(vis_ctx* ctx, const double E[9], const float* p1xy, const float* p2xy,
                      int m, double R[9], double t[3], int* n_good);
/* VISystem::F2FRansac, src/VISystem.cpp:612-769.  rot: 3x3 row-major f32 (IMU rotation),
 * sample_idx: 2*iters explicit sample indices (the reference uses unseeded rand(), :712-713),
 * scale: |t_GT|.  out: 3 floats. */
int  vis_f2f_ransac(vis_ctx* ctx, const vis_keypoint* pts1, const vis_keypoint* pts2, int m,
                    const float rot[9], const int32_t* sample_idx, int iters,
                    float scale, float out_t[3], int* count_max);

/* ---- the step after matching in CameraGPU::addGPUKeyframe (src/CameraGPU.cpp:154-157) ---- */
/* Camera::Update's half pyramid (src/Camera.cpp:63-72) + Camera::computeGradient (src/Camera.cpp:167-184) for n
 * frames resident in HBM.  Per frame and per level l = 0..4 of lw[l] x lh[l] pixels (vis_half_pyramid_dims): Scharr dx and dy as
 * CV_16S with OpenCV's `scale` argument (the reference call Scharr(img, g, CV_16S, 1, 0, 3, 0, BORDER_DEFAULT)
 * passes scale = 3, delta = 0), and gradient = addWeighted(|dx| sat u8, 0.5, |dy| sat u8, 0.5, 0).
 * All outputs are caller-owned DEVICE buffers of n * vis_gradient_frame_elems(w, h) elements: inside a frame the
 * levels are dense and back to back (level l starts at sum_{k<l} lw[k] lh[k]); d_gray receives levels 1..4 of
 * the half pyramid (its level-0 part is left untouched: level 0 is the frame itself).  16 <= w, h <= 4095 (the limit of the
 * alignment that reads these buffers; vis_gradient_frame_elems returns 0 outside it), stride >= w and stride % 4 == 0,
 * 1 <= scale <= 8 (int16 cannot overflow), output buffers 16-byte aligned (d_frames needs no alignment).  A level that is one pixel
 * wide or high (every side of 16 ... 21 ends in one) is a level like any other: BORDER_REFLECT_101 of a single pixel repeats it, so
 * the response across it is 0.  vis_gradient_batch is asynchronous on the context's stream (both of its launches, csrc/api.hip), behind an
 * alignment of the pose stream that still reads gradient buffers. */
size_t vis_gradient_frame_elems(int w, int h);
int  vis_gradient_batch(vis_ctx* ctx, const uint8_t* d_frames, int w, int h, int stride, int n, int scale,
                        uint8_t* d_gray, int16_t* d_gx, int16_t* d_gy, uint8_t* d_g);
/* one host frame; out pointers per level may be NULL; level l receives lw[l]*lh[l] elements (vis_half_pyramid_dims -- NOT (w>>l)*(h>>l):
 * 150 x 110 has a 38 x 28 level 2).  16 <= w, h <= 4095, stride >= w, 1 <= scale <= 8. */
int  vis_compute_gradient(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride, int scale,
                          int16_t* const gx[5], int16_t* const gy[5], uint8_t* const g[5]);
/* Camera::ObtainPatchesPointsPreviousFrame (src/Camera.cpp:358-410) and ObtainDebugPointsPreviousFrame
 * (:413-445): per level l the candidate list as rows (x, y, 1, 1) in the reference's push_back order, built from
 * at most 200 matched keypoints of the previous keyframe.  patch[l] / debug[l] receive up to `cap` rows
 * (VIS_E_CAPACITY if a level has more; n_patch[l] then holds the required count).  Level sizes come from
 * params.w_size >> l, params.h_size >> l (CameraModel w_size[lvl], h_size[lvl]).
 *   The candidate window, for EVERY float a keypoint can hold.  On level l, with cols x rows the level's size, sp = patch_size[l]
 *   (5, 3, 2, 5, 5: `patch_size - 1 / 2` in integers) and the level coordinates x = (float)(((double)kp.x + 0.5) * 2^-l - 0.5), y likewise,
 *   the candidate columns are the integers i with
 *       0 < i < cols,   i >= trunc(x - sp),   (float)i <= x + sp
 *   where x - sp and x + sp are the float difference and sum and the comparisons are taken on their values; the rows j likewise with y
 *   and rows.  The list holds (i, j, 1, 1) for every such column (outer, ascending) and row (inner, ascending), keypoint after keypoint.
 *   A keypoint whose level coordinate is NaN or infinite contributes none, and so does any whose window cannot touch the level, however
 *   large the coordinate (the reference's loop `for (int i = (int)(x - sp); (float)i <= x + sp; i++)` converts such a float to int, which
 *   is undefined, and never ends once x + sp >= 2^31).  Where that loop ends the list is its list.  No float outside [1, size) is
 *   converted to an integer on this path (csrc/patch_window.h). */
int  vis_patch_points(vis_ctx* ctx, const vis_keypoint* good, int n, int cap,
                      float* const patch[5], int n_patch[5], float* const debug[5], int n_debug[5]);

/* ---- the pose step the GPU main calls: VISystem::EstimatePoseFeatures (src/VISystem.cpp:1113-1448), called from
 * VISystemGPU::AddFrameGPU (src/VISystemGPU.cpp:167) -- SURVEY 8(f) N4 --------------------------------------- */
/* Gauss-Newton photometric alignment of the candidate points of the previous keyframe (ObtainPatchesPoints...) to the
 * current frame, coarse to fine over the half pyramid; pose = Sophus::SE3f (unit quaternion + translation). */
typedef struct vis_se3f { float qx, qy, qz, qw; float tx, ty, tz; } vis_se3f;   /* Sophus::SE3f storage order */
typedef struct vis_align_params {
    float fx, fy, cx, cy;        /* level-0 intrinsics, the float members of VISystem (include/VISystem.hpp:82) */
    int32_t first_level;         /* 3      src/VISystem.cpp:1119 */
    int32_t last_level;          /* 0      :1120 */
    int32_t max_iterations;      /* 10     :1117 */
    float   epsilon;             /* 0.001f :1115 */
    float   z_factor;            /* 0.002f :1121 */
} vis_align_params;
typedef struct vis_align_result {
    vis_se3f pose;               /* current_pose after the last level (Frame::rigid_transformation_, :1445) */
    float matrix[16];            /* pose.matrix(), row-major 4x4 */
    float error[5];              /* last mean squared residual per level */
    float initial_error;
    int32_t iterations[5];       /* iteration index k at which the level stopped */
    int32_t n_residuals[5];      /* valid residuals in the last iteration of the level */
} vis_align_result;
void vis_default_align_params(vis_align_params* ap);
/* Sophus::SE3f value operations on the host (thirdparty/sophus/se3.hpp:723-744 exp, :317-321 product, :253-259 matrix,
 * SE3(Matrix3, Point)): what VISystem::Track / EstimatePoseFeatures compose poses with (src/VISystem.cpp:1413,1607);
 * the same code the alignment kernel runs.  a = (upsilon, omega); matrices row-major. */
void vis_se3_exp(const float a[6], vis_se3f* out);
void vis_se3_mul(const vis_se3f* a, const vis_se3f* b, vis_se3f* out);
void vis_se3_from_rt(const float R[9], const float t[3], vis_se3f* out);
void vis_se3_matrix(const vis_se3f* a, float M[16]);
/* One pair, HOST pointers.  Level l images are dense lw[l] x lh[l] (vis_half_pyramid_dims: what vis_camera_update and
 * vis_compute_gradient write; up to one row / column more than (w>>l) x (h>>l)); 16 <= w, h <= 4095: gray1/gx1/gy1 of the previous keyframe
 * (Frame::grayImage / gradientX / gradientY), gray2 of the current frame, cand1[l] = n_cand[l] rows (x, y, z, 1) as
 * Frame::candidatePoints[l] holds them.  Levels outside [last_level, first_level] may be NULL.  init may be NULL
 * (identity); the reference seeds it from the IMU rotation residual and the ground-truth translation (:1133-1166).
 *   VIS_E_INVALID: fx, fy not finite and > 0; cx, cy, epsilon or z_factor not finite.
 *   A candidate row may hold any float.  Its source pixel is column (int)x, row (int)y where those lie inside the level, that is for
 *   -1 < x < (w >> l) and -1 < y < (h >> l) ((int)(-0.5) == 0); for every other x or y, NaN included, the row is skipped and the value is
 *   not converted.  A row whose warped point is NaN, infinite, outside the level, or whose depth P2 is 0 is skipped as well; init is
 *   taken as given: a NaN in it makes every warped point NaN (the record of a pair without residuals, with that pose), an infinite or
 *   huge translation is arithmetic like any other (tz = +inf projects every point onto (cx, cy)). */
int  vis_estimate_pose_features(vis_ctx* ctx, const vis_align_params* ap, int w, int h,
                                const uint8_t* const gray1[5], const uint8_t* const gray2[5],
                                const int16_t* const gx1[5], const int16_t* const gy1[5],
                                const float* const cand1[5], const int32_t n_cand[5],
                                const vis_se3f* init, vis_align_result* out);
/* Batched, DEVICE pointers: n consecutive frames resident in HBM and the outputs of vis_gradient_batch for the same
 * frames (d_gray levels 1..4, d_gx, d_gy).  Pair i = (frame i-1 -> frame i), i = 1..n-1; d_out[0] is zeroed.  The
 * candidate points of pair i are generated on the fly from d_pts: max_pts (x, y) floats per pair = the matched
 * keypoints of frame i-1 (Frame::nextGoodMatches, at most 200 are used like the reference), d_npts[i] of them valid; a d_npts[i]
 * above max_pts is clamped to max_pts (below 1: no candidates, the record of a pair without residuals).
 * d_init: n poses or NULL.  Asynchronous on the context's stream.  16 <= w, h <= 4095, stride >= w (any alignment).
 *   The rows of d_pts are device memory the call cannot validate: the candidates of a keypoint are vis_patch_points' window (above),
 *   which is defined for every float -- a NaN, an infinity or a coordinate of any size whose window does not touch the level contributes no
 *   candidate, so such an entry among the first min(d_npts[i], max_pts, 200) gives the record of the row without it; entries past that count
 *   are not read.  d_npts[i] may be any int32.  d_init is taken as given, like vis_estimate_pose_features' init; alignment parameters that
 *   are not finite are refused (VIS_E_INVALID) before anything is queued. */
int  vis_align_batch(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int w, int h, int stride, int n,
                     const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                     const float* d_pts, const int32_t* d_npts, int max_pts,
                     const vis_se3f* d_init, vis_align_result* d_out);
/* the same on the pairs of the last vis_batch_run (stages must have included MATCH): the matched points come from the
 * plan (the grid-filtered good matches of every pair).  Gate off: pair i = (frame i-1 -> frame i); pair 0 (frame 0 against the
 * carried frame) is skipped and d_out[0] is zeroed.  Gate on (keyframe_min_points > 0): pair i = (frame prev -> frame i) with prev =
 * vis_batch_get_keyframes' entry i when that is >= 0 (its gradients are in the same launch's set); a pair linked to the carried
 * frame is skipped like pair 0, and every pair that is skipped or has no pair (VIS_KF_*) gets a zeroed record.
 * Runs on the context's POSE stream, ordered behind everything queued on the context's stream so far (the gradients) and
 * behind the matcher, so that it overlaps the next vis_batch_run: d_frames, the gradient buffers and d_out are in use until
 * vis_batch_sync -- or until a later vis_gradient_batch / vis_batch_align / vis_feeder_submit of this context, which wait for it. */
int  vis_batch_align(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int n,
                     const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                     const vis_se3f* d_init, vis_align_result* d_out);
/* The weighting of the Gauss-Newton step (src/VISystem.cpp:1342-1344): the reference wrote two, IdentityWeights (live) and
 * TukeyFunctionWeights (:1797-1870, commented out at the call site).  Context state like vis_params, IDENTITY by default; read when
 * an alignment is enqueued (vis_estimate_pose_features, vis_align_batch, vis_batch_align, vis_batch_track -- the pair against the
 * carried keyframe included) and passed to it by value: a later vis_set_align_weights does not touch work already queued.
 * Per iteration, over the n valid residuals r (integers -255 ... 255):  med = MedianMat(r);  MAD = mad_scale * MedianMat(|r - med|),
 * 0 -> 1;  x = r / MAD;  w = (1 - x^2 / b^2)^2 for |x| <= b, else 0.  The step solves (WJ)^T (WJ) delta = -(WJ)^T (W r) and the error
 * is mean(r * W r) over all n (weight-0 residuals count in n), :1346-1409.  MedianMat takes the first bin whose running count exceeds
 * n / 2 -- after converting to CV_8U, which turns every negative residual into 0 and every deviation above 255 into 255:
 * VIS_W_TUKEY keeps that, VIS_W_TUKEY_SIGNED takes both medians over the values themselves (cf. VIS_SYM_*). */
enum { VIS_W_IDENTITY = 0,       /* IdentityWeights, :1343 */
       VIS_W_TUKEY = 1,          /* TukeyFunctionWeights exactly as written, MedianMat's 8-bit saturation included */
       VIS_W_TUKEY_SIGNED = 2 }; /* the same with medians over the signed residuals (what MedianMat evidently meant) */
typedef struct vis_align_weights {
    int32_t mode;                /* VIS_W_* */
    float   tukey_b;             /* 4.6851f :1800 */
    float   mad_scale;           /* 1.4826f :1831 */
    int32_t reserved_;           /* 0 */
} vis_align_weights;
void vis_default_align_weights(vis_align_weights* aw);
/* aw == NULL: the defaults.  VIS_E_INVALID (the setting stays as it was): mode outside VIS_W_*, tukey_b or mad_scale not finite and > 0,
 * reserved_ != 0, ctx == NULL. */
int  vis_set_align_weights(vis_ctx* ctx, const vis_align_weights* aw);
int  vis_get_align_weights(vis_ctx* ctx, vis_align_weights* aw);

/* ---- frame ingest (src/ImageReader.cpp) ------------------------------------- */
/* ImageReader::searchImages (src/ImageReader.cpp:49-74): the .pgm / .raw / .png files of `dir` in byte order, names
 * separated by '\n' in names_out (cap_bytes); *count = number of files.  names_out may be NULL to only count.
 * ("." and ".." are skipped by name; the reference erases the first two sorted entries.) */
int  vis_image_list(const char* dir, char* names_out, int cap_bytes, int* count);
/* ImageReader::getImageTime (:41-47): atol of the file name's stem (EuRoC names its images <timestamp ns>.ext) */
long vis_image_time(const char* file_name);
/* stand-in for imread(..., CV_LOAD_IMAGE_GRAYSCALE) (:80-82) on the formats this build reads: binary PGM
 * (P5, maxval <= 255, '#' comments allowed), headerless raw (w*h bytes) and greyscale PNG (what EuRoC ships: colour
 * type 0 or 4, 8 or 16 bit -- the high byte --, non-interlaced; chunk CRCs checked; colour / interlaced PNGs are
 * refused with VIS_E_INVALID).  vis_image_info tells PGM from PNG by the magic bytes. */
int  vis_pgm_info(const char* path, int* w, int* h);
int  vis_image_info(const char* path, int* w, int* h);
int  vis_image_read(const char* path, uint8_t* out, int out_stride, int w, int h);
/* Pinned-host double-buffered H2D feeder for vis_batch_run: fill vis_feeder_host_buffer(f, k) (batch x h x w,
 * dense; blocks while an earlier copy out of it is in flight), vis_feeder_submit(f, k, n, &d) enqueues the copy on a
 * copy stream and orders the context's detect stream after it, run vis_batch_run(ctx, d, n, ...), then
 * vis_feeder_release(f, k).  Alternating k = 0, 1 overlaps the copy of batch i+1 with the processing of batch i. */
typedef struct vis_feeder vis_feeder;
int  vis_feeder_create(vis_ctx* ctx, int w, int h, int batch, vis_feeder** out);
void vis_feeder_destroy(vis_feeder* f);
uint8_t* vis_feeder_host_buffer(vis_feeder* f, int which);
int  vis_feeder_submit(vis_feeder* f, int which, int n, const uint8_t** d_frames);
int  vis_feeder_release(vis_feeder* f, int which);

/* ---- batched stream API (throughput path) --------------------------------- */
/* Plan device buffers for batches of up to `max_frames` w x h frames.  Frames in a batch are consecutive frames of ONE camera
 * stream, matched against the last SAVED frame before them (Camera::computeGoodMatches: query = frameList.back(),
 * src/Camera.cpp:146-157).  The plan takes params.keyframe_min_points as it is at this call:
 *   0 (gate off): every frame is saved; frame i is matched against frame i-1, frame 0 against the last frame of the previous
 *     vis_batch_run call (carried on device), or not at all after vis_batch_reset.
 *   K >= 1 (gate on): frame i is saved when it has > K keypoints (> 1 until the first frame is saved after vis_batch_plan /
 *     vis_batch_reset).  A saved frame is matched against the last saved frame before it -- in the same batch, or the record
 *     carried from an earlier call; a frame that is not saved, or the first saved frame of a stream, has no pair (n_sym = n_good = 0,
 *     the pose record of a pair without correspondences).  The carried record is the last saved frame: a batch that saves nothing
 *     carries the earlier one forward.  Decided on the device, with no host round trip (vis_batch_get_keyframes reports it). */
int  vis_batch_plan(vis_ctx* ctx, int w, int h, int stride, int max_frames);
int  vis_batch_reset(vis_ctx* ctx);
enum { VIS_STAGE_DETECT = 1, VIS_STAGE_MATCH = 2, VIS_STAGE_POSE = 4, VIS_STAGE_ALL = 7,
       /* Camera::Update (src/Camera.cpp:63-72) for every frame of the batch: the 4 half-resolution levels into a plan-owned
        * buffer (vis_batch_half_pyramid), on a side stream that starts behind the pyramid launches of the detect chain and is joined
        * by the detect stream at the end of its chain. */
       VIS_STAGE_UPDATE = 8, VIS_STAGE_FRAME = 15,
       /* Camera::computeGradient (src/Camera.cpp:167-184; inside addGPUKeyframe, src/CameraGPU.cpp:154) for every frame of the
        * batch: Scharr dx / dy (CV_16S, scale 3) and the blended magnitude on the 5 half-pyramid levels, into plan-owned buffers
        * (vis_batch_gradients), on the same side stream as Camera::Update -- pure streaming work beside the detect chain.
        * Implies VIS_STAGE_UPDATE.  Overwrites the previous batch's gradients: it waits for a vis_batch_align still reading them. */
       VIS_STAGE_GRADIENT = 16 };
/* Asynchronous: d_frames = n_frames images resident in HBM (dev ptr, row stride from the plan, frame stride =
 * stride*h).  The context runs three streams: the detect chain (the stream set with vis_set_stream / the context's
 * own), the matcher, and the RANSAC/pose stage; consecutive calls overlap (detect of batch i+1 with match and pose of
 * batch i).  d_frames may be reused once the detect chain of this call has finished (vis_batch_sync, or an event
 * recorded on the detect stream after the call; vis_feeder_release does exactly that). */
int  vis_batch_run(vis_ctx* ctx, const uint8_t* d_frames, int n_frames, int stages);
int  vis_batch_sync(vis_ctx* ctx);
/* the half pyramids the last vis_batch_run(... | VIS_STAGE_UPDATE) wrote: DEVICE pointer to n * *frame_elems bytes, laid out
 * like d_gray of vis_gradient_batch (levels dense and back to back inside a frame, level 0's part untouched);
 * VIS_E_STATE if the stage has not run.  Valid until the next vis_batch_run / vis_batch_plan. */
int  vis_batch_half_pyramid(vis_ctx* ctx, const uint8_t** d_half, size_t* frame_elems);
/* the gradients the last vis_batch_run(... | VIS_STAGE_GRADIENT) wrote: DEVICE pointers laid out like the outputs of
 * vis_gradient_batch (d_gray = the half pyramid of vis_batch_half_pyramid); any pointer may be NULL.  VIS_E_STATE if the
 * stage has not run.  Valid until the next vis_batch_run / vis_batch_plan (the plan owns two sets and fills them in turn, so
 * that a vis_batch_align still reading one does not hold up the next step's gradients).  vis_batch_align takes them when its
 * three gradient arguments are NULL. */
int  vis_batch_gradients(vis_ctx* ctx, const uint8_t** d_gray, const int16_t** d_gx, const int16_t** d_gy, const uint8_t** d_g,
                         size_t* frame_elems);
/* copy results of the last batch to host (synchronises). Any pointer may be NULL. */
int  vis_batch_get_keypoints(vis_ctx* ctx, int frame, vis_keypoint* kps, uint8_t* desc,
                             int cap, int* n_out);
int  vis_batch_get_knn(vis_ctx* ctx, int frame, vis_dmatch* out12, int cap12, int* n12,
                       vis_dmatch* out21, int cap21, int* n21);
int  vis_batch_get_matches(vis_ctx* ctx, int frame, vis_dmatch* good, int cap, int* n_good,
                           int* n_sym);
int  vis_batch_get_pose(vis_ctx* ctx, int frame, double E[9], double R[9], double t[3],
                        int* n_inliers, int* n_pose_good, int* iters_run);
/* diagnostics: out[0] = kernel launches of this process so far, out[1] = times a single-frame entry point of this context blocked on the
 * device, out[2] = asynchronous copies those entry points queued (bench.py `single_frame_api`: per-frame differences), out[3] = the largest
 * vis_pose_result::undecided_max of any vis_essential_ransac call of this context. */
int  vis_debug_counters(vis_ctx* ctx, unsigned long long out[4]);
/* diagnostic (tests read the pyramid with it; no product path needs it): copy level `level` >= 1 of frame `frame` of the last
 * detection -- of the single-frame plan (batch == 0: vis_orb_detect_compute, frame 0) or of the batch plan (batch != 0: the last
 * vis_batch_run with VIS_STAGE_DETECT) -- to `out`, h_level rows of w_level bytes (vis_level_geometry) at out_stride >= w_level.
 * Read only: it launches nothing and changes nothing.  Synchronises the context's stream.  VIS_E_STATE if that plan has not
 * detected yet (also after vis_set_params / vis_batch_plan / vis_batch_reset); VIS_E_INVALID for level 0 (the caller's own
 * frame), a level >= nlevels or a frame outside the last detection. */
int  vis_debug_pyramid_level(vis_ctx* ctx, int batch, int frame, int level, uint8_t* out, int out_stride);
/* the inlier mask of findEssentialMat (src/VISystem.cpp:1680, the `mask` argument) for pair `frame` of the last batch: one byte per
 * correspondence the pose stage saw, in the order it saw them (good matches, or the symmetric matches with VIS_POSE_SYM).
 * VIS_E_CAPACITY if cap < *n_points (which is still returned). */
int  vis_batch_get_inlier_mask(vis_ctx* ctx, int frame, uint8_t* mask, int cap, int* n_points);
/* the pairing of the last vis_batch_run: prev[i] = the batch index of the frame that frame i was matched against, or one of
 * VIS_KF_CARRIED (the record carried from an earlier call), VIS_KF_NOT_SAVED (frame i failed the keyframe gate: no pair),
 * VIS_KF_FIRST (saved, with no earlier saved frame to match against).  Gate off: i-1, and VIS_KF_CARRIED or VIS_KF_FIRST for
 * frame 0.  *n_out = frames of the last batch; VIS_E_CAPACITY if cap < *n_out.  Synchronises. */
enum { VIS_KF_CARRIED = -1, VIS_KF_NOT_SAVED = -2, VIS_KF_FIRST = -3 };
int  vis_batch_get_keyframes(vis_ctx* ctx, int32_t* prev, int cap, int* n_out);
/* ---- batched camera tracking (VISystemGPU::AddFrameGPU after detection, src/VISystemGPU.cpp:137-175) --------------------
 * For every frame of the last vis_batch_run: the alignment of the frame's keyframe pair (VISystem::EstimatePoseFeatures) and
 * VISystem::Track (src/VISystem.cpp:1567-1635), final_poseCam = final_poseCam * SE3(matrix(pose).R, pose.t) -- the pose the GPU main
 * writes to its CSV (positionCam = pose.t, qOrientationCam = pose.q, src/main_vi_slamGPU.cpp:123-150).
 *   Preconditions (else VIS_E_STATE): the last vis_batch_run had VIS_STAGE_MATCH | VIS_STAGE_GRADIENT, pose_input == VIS_POSE_GOOD,
 *     n == the frames of that run, and EVERY vis_batch_run since vis_batch_plan / vis_batch_reset was tracked, once (the pair to the
 *     carried keyframe reads the snapshot the call for the launch before took: a launch that was not tracked leaves none).
 *   d_align[i] (n records): the alignment of frame i's pair, with vis_batch_get_keyframes' pairing -- gate off (i-1 -> i), gate on
 *     (prev[i] -> i) -- INCLUDING the pair to the keyframe carried from an earlier launch (VIS_KF_CARRIED), which vis_batch_align
 *     skips.  A frame without a pair gets a zeroed record.  d_init: n poses or NULL, as for vis_batch_align.
 *   d_track[i] (n records): final_poseCam after frame i.  A saved frame with a pair composes its own residual; a frame the gate
 *     refused composes the last residual again once two frames have been saved (AddFrameGPU re-estimates the unchanged last pair,
 *     frameList.size() > 1) -- that residual may come from an earlier launch; otherwise the pose is unchanged.
 *   The chain continues across launches.  vis_batch_reset restarts it at the pose last given to vis_batch_track_init and forgets
 *   the last residual; vis_batch_plan restarts it at identity.
 *   Asynchronous on the POSE stream with vis_batch_align's ordering (it overlaps the next vis_batch_run the same way): d_frames,
 *   the plan's gradients, d_align and d_track are in use until vis_batch_sync.  Host and device compose with the same code, so
 *   d_track equals vis_se3_mul / vis_se3_from_rt / vis_se3_matrix applied in frame order byte for byte. */
enum { VIS_TRACK_NONE = -4 };
typedef struct vis_track_result {
    vis_se3f pose;               /* final_poseCam after this frame */
    int32_t  composed;           /* the pair whose residual Track composed for this frame: the frame's own batch index (a saved
                                    frame with a pair); the batch index of the last saved frame (a frame the gate refused);
                                    VIS_KF_CARRIED (that saved frame is in an earlier launch); VIS_TRACK_NONE: Track did not run
                                    (fewer than two frames saved since vis_batch_plan / vis_batch_reset) */
} vis_track_result;              /* 32 bytes */
/* final_poseCam to continue from (InitializeSystemGPU's initial camera pose, src/VISystemGPU.cpp:107-115); NULL = identity.  Sets
 * the current pose of the chain (the last residual is kept) and the pose vis_batch_reset restarts at.  Needs a plan; synchronises.
 * The pose is taken as given -- not normalised, not tested: a component that is NaN or infinite stays in the chain, and every
 * final_poseCam composed from it carries what Sophus' product makes of it (d_align is not affected: the alignments do not read it). */
int  vis_batch_track_init(vis_ctx* ctx, const vis_se3f* pose);
int  vis_batch_track(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int n,
                     const vis_se3f* d_init, vis_align_result* d_align, vis_track_result* d_track);
/* what the pose stage leaves per pair on the device (vis_batch_results_async copies these records) */
typedef struct vis_pose_result {
    double E[9], R[9], t[3];
    int32_t n_inliers, n_pose_good, iters_run, n_points;
    int32_t n_models;          /* candidate essential matrices scored against the n_points correspondences (SURVEY 8(d):
                                  point evaluations = n_models x n_points) */
    int32_t undecided_max;     /* diagnostic: the most (model, point) inlier decisions that single precision left open in any group of 16
                                  hypotheses of this problem (settled in double precision: up to 4096 from a list, beyond that by
                                  recounting the group); 0 for up to 256 correspondences, which never use that form */
} vis_pose_result;
/* Queue the device-to-host copy of the last batch's results -- n pose records, the good matches (n x root^2, dense
 * rows) and their counts, one entry per frame of the batch: the pair (vis_batch_get_keyframes' prev[i] -> frame i); a frame
 * without a pair (frame 0 after vis_batch_reset; with the keyframe gate on, any VIS_KF_NOT_SAVED / VIS_KF_FIRST frame) has
 * count 0 and the pose record of zero correspondences -- behind the batch's own work; any pointer may be NULL; pinned host memory makes the copy
 * overlap the next vis_batch_run (pinned = device-accessible, e.g. hipHostMalloc: such destinations are written by one
 * small kernel of the library, which costs the pipeline nothing; anything else goes through hipMemcpyAsync).  n_cap = the number of frames the caller's buffers hold: VIS_E_CAPACITY (nothing is
 * copied) if the last batch had more.  The reference downloads its results every frame (src/CameraGPU.cpp:103, the
 * DMatch vectors of src/MatcherGPU.cpp:54-56).  The copies are only QUEUED: the host may read the buffers after
 * vis_batch_sync() (or after waiting for an event recorded behind this call); a later vis_batch_results_async is
 * ordered behind this one on the device but does not make this one visible to the host by itself. */
int  vis_batch_results_async(vis_ctx* ctx, vis_pose_result* h_pose, vis_dmatch* h_good, int32_t* h_ngood, int n_cap);
/* Batched streams run FAST at a per-level threshold tau >= fast_threshold predicted from the previous batch: retainBest(2 * quota)
 * only keeps corners whose score reaches a cut far above fast_threshold, and a corner below the cut can neither be kept nor
 * suppress a kept one, so any tau <= cut gives the identical keypoints.  The prediction is verified per (frame, level) on the
 * device and whatever it got wrong is redone at fast_threshold inside the same vis_batch_run: results never depend on it.
 * tau_next (nlevels ints, may be NULL) = the thresholds the NEXT batch will start from; *n_redone = (frame, level) pairs the last
 * batch had to redo.  Synchronises.  vis_batch_reset() forgets the prediction. */
int  vis_batch_fast_thresholds(vis_ctx* ctx, int32_t* tau_next, int32_t* n_redone);
/* device-side error/overflow flags of the last batch (0 = clean) */
int  vis_batch_status(vis_ctx* ctx, int* flags);

/* ---- map points: VISystem::Triangulate (src/VISystem.cpp:862-923) and VISystem::Disparity (:422-471) --------------------------------
 * The 3-D points of matched keypoints under a known relative pose (x2 = R x1 + t, as vis_pose_result holds it), per correspondence i:
 *   X            DLT triangulation in the pose stage's normalised coordinates ((double)p - c) * (1 / fx) -- the single focal of
 *                findEssentialMat(focal, pp) -- by the device code of recoverPose's cheirality vote (4 x 4 Jacobi eigen-decomposition of
 *                A^T A, eigenvector of the smallest eigenvalue): the point in the FIRST camera's frame, in units of the baseline (|t| = 1).
 *   VIS_MP_FRONT the cheirality test of recoverPose, the vote's own expression: for a pair of the batch the number of FRONT points under
 *                the record's (R, t) equals n_pose_good exactly.
 *   VIS_MP_INLIER  the mask byte of findEssentialMat when a mask is given, else set.
 *   reproj_px    |(u1, v1) - (fx X[0] / X[2] + cx, fx X[1] / X[2] + cy)| in double, rounded to float once (:913-915, with the focal the
 *                point was triangulated with).
 *   parallax_px  Disparity's per-point term (:440-462) in its own single precision and operation order with RotationResCam = (float)R^T:
 *                a = (u2 - cx) / fx, b = (v2 - cy) / fy, o = Rres (a, b, 1), |(u1, v1) - (fx o.x / o.z + cx, fy o.y / o.z + cy)|.
 *   VIS_MP_REPROJ_OK = reproj_px <= max_reproj_px, VIS_MP_PARALLAX_OK = parallax_px >= min_parallax_px, VIS_MP_KEPT = all four.
 *   inliers_only != 0: a correspondence whose mask byte is 0 is not decomposed; its record and flags are zero.
 * Summary per pair: the counts and mean_parallax_px = Disparity's return value, the float sum of parallax_px over all n_points in index
 * order divided by (float)n_points.  A pair without correspondences or without a pose (R all zero: what the pose stage leaves where
 * RANSAC found no model, for frame 0 after vis_batch_reset and for VIS_KF_NOT_SAVED / VIS_KF_FIRST frames) gets a zero summary and
 * its rows are left untouched.  A metric scale is the caller's multiplication. */
enum { VIS_MP_INLIER = 1, VIS_MP_FRONT = 2, VIS_MP_REPROJ_OK = 4, VIS_MP_PARALLAX_OK = 8, VIS_MP_KEPT = 16 };
typedef struct vis_tri_params { float max_reproj_px, min_parallax_px; int32_t inliers_only, reserved_; } vis_tri_params;   /* 16 bytes */
typedef struct vis_map_point { double X[3]; float reproj_px, parallax_px; } vis_map_point;                                /* 32 bytes */
typedef struct vis_tri_summary { int32_t n_points, n_front, n_kept; float mean_parallax_px; } vis_tri_summary;            /* 16 bytes */
/* 2.0 px, 0 px, 0.  These are THIS LIBRARY's defaults: the reference has no such constants (Triangulate only draws its points, and the
 * 22 px disparity threshold of its keyframe decision is commented out, src/VISystem.cpp:322). */
void vis_default_tri_params(vis_tri_params* tp);
/* One pair, HOST pointers; blocks once like the other single-frame entry points.  p1xy / p2xy: m x 2 floats (pixels); mask (m bytes) may
 * be NULL; points / flags receive m entries.  m = 0: a zero summary. */
int  vis_triangulate(vis_ctx* ctx, const vis_tri_params* tp, const double R[9], const double t[3],
                     const float* p1xy, const float* p2xy, int m, const uint8_t* mask,
                     vis_map_point* points, uint8_t* flags, vis_tri_summary* summary);
/* Every pair of the last vis_batch_run (which must have included VIS_STAGE_POSE; n = its frames), DEVICE pointers: d_points / d_flags hold
 * n rows of row_cap entries (d_points 16-byte aligned), d_summary n records.  Pair i is the pose stage's: its correspondences in the order
 * the stage saw them (vis_batch_get_inlier_mask), its mask, its (R, t).  Asynchronous on the POSE stream behind that pose stage, and it
 * overlaps the next vis_batch_run like vis_batch_align: the caller's buffers are in use until vis_batch_sync.  VIS_E_STATE without
 * context / plan / pose stage or when n differs; VIS_E_CAPACITY when row_cap is smaller than the plan's correspondences per pair
 * (root^2, or the keypoint capacity with VIS_POSE_SYM); VIS_E_INVALID for NULL or misaligned outputs. */
int  vis_batch_triangulate(vis_ctx* ctx, const vis_tri_params* tp, int n, int row_cap,
                           vis_map_point* d_points, uint8_t* d_flags, vis_tri_summary* d_summary);

/* ---- IMU-aided translation and epipolar keypoint filter: VISystem::F2FRansac (src/VISystem.cpp:612-769) and VISystem::FilterKeypoints
 * (:542-610) for the pairs of a batch -- the pose steps of the ground-truth main's AddFrame (:358-359, :523-527).  The rotation of every
 * pair is an INPUT (the reference integrates the IMU for it; vis_batch_imu / vis_imu_preintegrate_rows below write it on the device).  Both use one test per correspondence:
 *     -1000 / log10(|dir . normal|) < threshold,   normal = bearing1 x (R bearing2),  bearings ((u - cx) / fx, (v - cy) / fy, 1) normalised
 * with dir = a RANSAC hypothesis (F2FRansac) or the given translation's direction (FilterKeypoints).  The device decides it by two compares
 * and evaluates the expression itself only in a narrow band around 10^(-1000 / threshold): the result is that of the expression for every input
 * (DESIGN.md).  Rows: d_p1 / d_p2 hold n rows of max_pts (x, y) float points (8-byte aligned), d_npts[i] of them valid (clamped to max_pts).
 * F2FRansac per pair with m correspondences: iteration j of params.f2f_iters samples i1 = (d_draws[2j] & 0x7fffffff) % (m - 1) and i2 likewise from
 * d_draws[2j + 1] (rand() % (sizeNewGroup - 1), :712-713; ONE table of f2f_iters x 2 draws serves every pair, so a stream's records do not depend on
 * how it is cut into batches), d = normalize(n_i1 x n_i2), a zero cross product is skipped (:716), the count runs over all m correspondences with
 * params.f2f_threshold, and the first iteration with the largest count > 0 wins (:737-741).  t = scale * (float)d; with a reference translation g
 * (d_tref, 3 floats per pair; the ground-truth translation of :524-527 and :639-642) scale = |g| in float and t is negated when t . g < 0; without
 * (NULL): scale 1, no flip.  m < 2, f2f_iters == 0 or a frame without a pair: a zero record with best_iter = -1. */
enum { VIS_F2F_TILE = 512 };   /* correspondences per LDS tile of the kernel: rows longer than this are walked in several tiles */
typedef struct vis_f2f_result {          /* 32 bytes */
    float   t[3];                        /* scale * direction, sign-fixed; 0 when no hypothesis won */
    int32_t count_max, n_points;
    int32_t best_iter;                   /* -1: none */
    int32_t n_degenerate;                /* iterations skipped for a zero cross product, :716 */
    int32_t flipped;
} vis_f2f_result;
/* DEVICE pointers; d_rot: n x 9 floats (row-major 3x3 per pair), d_out: n records.  Asynchronous on the context's stream.  VIS_E_INVALID for a NULL
 * or misaligned argument (d_tref may be NULL) or n, max_pts < 0; VIS_E_STATE without a context. */
int  vis_f2f_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts,
                   const float* d_rot, const float* d_tref, const int32_t* d_draws, vis_f2f_result* d_out);
/* The same on the pairs of the last vis_batch_run (which must have included VIS_STAGE_MATCH; VIS_STAGE_POSE is not needed; n = its frames): the
 * correspondences the pose stage would see, in the order of vis_batch_get_inlier_mask (the good matches, or the symmetric matches with
 * VIS_POSE_SYM), with vis_batch_get_keyframes' pairing, the pair to the carried frame included; frame i's rotation is d_rot[9 i].  Asynchronous
 * on the POSE stream behind the match filter (and behind what is queued on the context's stream so far), overlapping the next vis_batch_run like
 * vis_batch_align: the caller's buffers are in use until vis_batch_sync.  VIS_E_STATE without context / plan / match stage or when n differs;
 * VIS_E_INVALID for NULL d_rot, d_draws or d_out. */
int  vis_batch_f2f(vis_ctx* ctx, int n, const float* d_rot, const float* d_tref, const int32_t* d_draws, vis_f2f_result* d_out);
/* FilterKeypoints: d_keep[i * row_cap + k] = 1 when correspondence k of pair i passes the test with dir = d_t[3 i ..] / |d_t[3 i ..]| (the three
 * floats widened to double, :565-568) under the rotation d_rot[9 i ..] (RotationResidual, :594), else 0; bytes beyond the pair's correspondences
 * are left untouched; d_nkeep[i] = the number kept.  A zero translation makes every dot product NaN: nothing is kept, as in the reference.  The
 * reference passes threshold 500.0 at its only call site (:358).  Asynchronous like vis_f2f_batch / vis_batch_f2f.  VIS_E_CAPACITY when row_cap is
 * smaller than max_pts (the plan's correspondences per pair); VIS_E_INVALID when threshold is not finite. */
int  vis_filter_keypoints_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts,
                                const float* d_rot, const float* d_t, double threshold, int row_cap, uint8_t* d_keep, int32_t* d_nkeep);
int  vis_batch_filter_keypoints(vis_ctx* ctx, int n, const float* d_rot, const float* d_t, double threshold, int row_cap,
                                uint8_t* d_keep, int32_t* d_nkeep);
/* One pair, HOST pointers (vis_keypoint arrays like vis_f2f_ransac); blocks once.  keep receives m bytes; m = 0: *n_keep = 0. */
int  vis_filter_keypoints(vis_ctx* ctx, const vis_keypoint* pts1, const vis_keypoint* pts2, int m, const float rot[9], const float t[3],
                          double threshold, uint8_t* keep, int* n_keep);

/* ---- homography RANSAC and the H-or-E model choice: the other half of a two-view initialiser (Mur-Artal, Montiel, Tardos: ORB-SLAM, 2015,
 * section IV; the reference has neither).  For a standing or purely rotating camera, a planar scene or points at infinity the essential
 * matrix of the pose stage is not determined by the correspondences; a homography explains such a pair, and
 * comparing the two models' scores flags it; the section after this one turns a flagged pair's H into a pose.
 * Coordinates: the pose stage's, x = ((double)u - cx) * (1 / fx), y = ((double)v - cy) * (1 / fx) with the single focal of findEssentialMat,
 * so H is the Euclidean homography R + t n^T / d up to scale.  Thresholds, once on the host in double: s2 = (sigma_px * (1 / fx))^2,
 * t_h = chi2_h * s2, t_e = chi2_e * s2.  No multiply-add is contracted; dot products are summed left to right.
 * Hypothesis j of hp.iters samples i_k = (d_draws[4 j + k] & 0x7fffffff) % m, k = 0 ... 3 (ONE table of iters x 4 draws serves every pair, so a
 * stream's records do not depend on how it is cut into batches).  Minimal solver, closed form over projective bases: with p_k = (x_k, y_k, 1)
 * the four source points, l0 = (p1 x p2) . p3, l1 = (p2 x p0) . p3, l2 = (p0 x p1) . p3, A = [l0 p0 | l1 p1 | l2 p2], B likewise from the
 * target points, H = B adj(A) (adj: rows c1 x c2, c2 x c0, c0 x c1 of the columns).  The iteration is skipped and counted in n_degenerate
 * when two indices are equal, when an l or (p0 x p1) . p2 of either side is zero or not finite, or when H does not reproduce its own
 * sample: one of the eight transfer tests below of the four sample points fails at t_h * 2^-20.
 * Per-point test, division-free: (U, V, w) = H (x1, y1, 1), e12 = (U - x2 w)^2 + (V - y2 w)^2, forward iff e12 <= t_h (w w); backward the
 * same with G = adj(H) on (x2, y2, 1) against (x1, y1); an inlier passes both; a NaN fails.  The first iteration with the largest count > 0
 * wins.  mask receives the winner's inlier bytes (zeros when no iteration won); bytes beyond the pair's correspondences are left untouched.
 * Scores of the winner -- ORB-SLAM's CheckHomography / CheckFundamental, restated from the paper, not from its code: with d = e12 / (w w),
 * score_h = sum over the points and both directions of (d <= t_h ? chi2_h - d / s2 : 0).  With an E: l2 = E x1, l1 = E^T x2, r = x2 . l2;
 * each direction adds chi2_h - d / s2, d = r^2 / (l_a^2 + l_b^2), when l_a^2 + l_b^2 > 0 and r^2 <= t_e (l_a^2 + l_b^2); n_inliers_e counts
 * the points that pass both; a zero or NaN E scores 0.  E is scored whether or not an H won.  Both sums are taken in one fixed order (64
 * partial sums over i mod 64 in rising i, then a fixed tree), without floating-point atomics: two runs are byte-identical.
 * Decision: H is offered when n_inliers >= min_inliers, E when it is given and n_inliers_e >= min_inliers; model = VIS_MODEL_HOMOGRAPHY when H
 * is offered and either E is not or score_h > h_ratio (score_h + score_e); else VIS_MODEL_ESSENTIAL when E is offered; else VIS_MODEL_NONE.
 * H is normalised last (unit Frobenius norm, negated when its determinant is negative; a determinant of exactly 0 keeps the sign): everything
 * above is computed from the unnormalised winner.  m < 4 or iters == 0: a zero record with best_iter = -1 (mask bytes of the pair zero). */
enum { VIS_MODEL_NONE = 0, VIS_MODEL_HOMOGRAPHY = 1, VIS_MODEL_ESSENTIAL = 2 };
enum { VIS_H_TILE = 512 };               /* correspondences per LDS tile of the kernel: rows longer than this are walked in several tiles */
typedef struct vis_homography_params {   /* 40 bytes */
    int32_t iters;                       /* 200    hypotheses per pair */
    int32_t min_inliers;                 /* 8      below it a model is not offered */
    double  chi2_h;                      /* 5.991  two-sided transfer error, 2 degrees of freedom, 95 % */
    double  chi2_e;                      /* 3.841  point-to-epipolar-line distance, 1 degree of freedom, 95 % */
    double  sigma_px;                    /* 1.0 */
    double  h_ratio;                     /* 0.40   ORB-SLAM2's value (the paper's 0.45 does not separate the test scenes: DESIGN.md section 4.10) */
} vis_homography_params;
typedef struct vis_homography_result {   /* 112 bytes */
    double  H[9];                        /* row-major, x2 ~ H x1; unit Frobenius norm, det >= 0; zeros when no iteration won */
    double  score_h, score_e;
    int32_t n_inliers, n_points;
    int32_t best_iter;                   /* -1: none */
    int32_t n_degenerate;
    int32_t n_inliers_e;
    int32_t model;                       /* VIS_MODEL_* */
} vis_homography_result;
void vis_default_homography_params(vis_homography_params* hp);
/* One pair, HOST pointers; blocks once like the other single-frame entry points.  p1xy / p2xy: m x 2 floats (pixels); draws: hp.iters x 4;
 * E: 9 doubles row-major or NULL; mask: m bytes or NULL. */
int  vis_find_homography(vis_ctx* ctx, const vis_homography_params* hp, const float* p1xy, const float* p2xy, int m,
                         const int32_t* draws, const double* E, uint8_t* mask, vis_homography_result* out);
/* DEVICE pointers, asynchronous on the context's stream.  d_p1 / d_p2: n rows of max_pts (x, y) float points, d_npts[i] of them valid
 * (clamped to max_pts); d_E: n x 9 doubles or NULL; d_mask: n rows of row_cap bytes or NULL; d_out: n records. */
int  vis_homography_batch(vis_ctx* ctx, const vis_homography_params* hp, int n, const float* d_p1, const float* d_p2,
                          const int32_t* d_npts, int max_pts, const int32_t* d_draws, const double* d_E,
                          int row_cap, uint8_t* d_mask, vis_homography_result* d_out);
/* The same on the pairs of the last vis_batch_run (which must have included VIS_STAGE_MATCH; n = its frames): the correspondences the pose
 * stage would see, in the order of vis_batch_get_inlier_mask, with vis_batch_get_keyframes' pairing, the pair to the carried frame
 * included.  E is the pair's pose record's when that run included VIS_STAGE_POSE; otherwise there is none.  A frame without a pair gets the
 * zero record.  Asynchronous on the POSE stream behind the pose stage, overlapping the next vis_batch_run like vis_batch_f2f: the caller's
 * buffers are in use until vis_batch_sync.
 * Refusals of the three calls, in this order.  VIS_E_INVALID: a NULL or misaligned pointer (8 bytes for points, E and records; E and the
 * mask may be NULL), a negative size, hp.iters < 0, hp.min_inliers < 4, a chi2 or sigma_px that is not finite and positive, h_ratio outside
 * (0, 1).  vis_homography_batch: VIS_E_STATE without a context, then VIS_E_CAPACITY when a mask is given and row_cap < max_pts.
 * vis_batch_homography: VIS_E_CAPACITY when a mask is given and row_cap is below the plan's correspondences per pair, then VIS_E_STATE
 * without context / plan / match stage or when n differs. */
int  vis_batch_homography(vis_ctx* ctx, const vis_homography_params* hp, int n, const int32_t* d_draws,
                          int row_cap, uint8_t* d_mask, vis_homography_result* d_out);

/* ---- the pose of a homography: the second half of that two-view initialiser (Faugeras & Lustman, "Motion and structure from motion in a
 * piecewise planar environment", 1988; ORB-SLAM section IV's ReconstructH -- both restated from the papers; the reference has neither).  For a
 * pair flagged VIS_MODEL_HOMOGRAPHY the (R, t) of vis_pose_result is undetermined; this turns the pair's H into (R, t / d, n): x2 = R x1 + t
 * for points of the plane n . X = d of the first camera, t in units of d -- NOT of unit norm like vis_pose_result's.  Accuracy is that of the
 * H it is given: the unrefitted four-point H of vis_*_homography, or that H refined over its inliers by vis_*_homography_polish (below), whose
 * record and mask this call reads unchanged.
 * All arithmetic is double, nothing is contracted, the only operations are + - * / sqrt; dot3(a, b) = a0 b0 + a1 b1 + a2 b2 and every sum of a
 * 3 x 3 product run left to right from 0 (tests/homography_pose_ref.py restates every step in this order, bit for bit).
 * Input: the record's H and best_iter, the pair's correspondences in pixels, an optional mask (the one vis_*_homography wrote; NULL = every
 * correspondence votes) and an optional rotation hint.  best_iter < 0, an H entry that is not finite, m < 1, or a t_norm (below) that is
 * not finite (a rank-deficient H: d2 == 0): the zero record with kind = VIS_HP_NONE, solution = second = -1.
 * Singular values: H = U diag(d1, d2, d3) V^T by the pose stage's Jacobi path (eigenvectors v0, v1 of H^T H by descending eigenvalue, v2 = v0 x
 * v1; u0 = H v0 / |H v0|, u1 = H v1 made orthogonal to u0 and normalised, u2 = u0 x u1: U and V are proper rotations, and det H >= 0 makes
 * d3 >= 0); sv[k] = d_k = sqrt(dot3(w, w)) with w = H v_k.  t_norm = (d1 - d3) / d2 = |t| / d.  q_k = d_k d_k, den = q1 - q3.
 * VIS_HP_ROTATION when t_norm <= min_t_over_d, den == 0 or den is not finite: R = U V^T, t = n = 0, no vote, solution = 0, second = -1.
 * Otherwise VIS_HP_PLANE, with the branch d' = +d2 only (det H >= 0: both cameras on one side of the plane):
 *   x1 = sqrt(max((q1 - q2) / den, 0)), x3 = sqrt(max((q2 - q3) / den, 0)), dd = (d1 + d3) d2,
 *   S = sqrt(max((q1 - q2) (q2 - q3), 0)) / dd, c = (q2 + d1 d3) / dd;   rotation 0: s = S, x3' = x3;  rotation 1: s = -S, x3' = -x3;
 *   R' = [[c, 0, -s], [0, 1, 0], [s, 0, c]], R = (U R') V^T, t' = ((d1 - d3) x1, 0, (d1 - d3) (-x3')), t_i = dot3(row i of U, t') / d2,
 *   n_i = (V_i0 x1 + V_i1 0) + V_i2 x3'.
 * Candidates k = 0 ... 3 for (e1, e3) = (+,+), (+,-), (-,+), (-,-): 0 = rotation 0, 1 = rotation 1, 2 = candidate 1 with -t, -n, 3 = candidate 0
 * with -t, -n (exactly).
 * Vote: a voting correspondence, in the pose stage's coordinates ((double)u - cx) * (1 / fx), votes for candidate k when the DLT triangulation
 * and depth test of recoverPose (the one behind n_pose_good and VIS_MP_FRONT) passes under (R_k, t_k) -> n_good[k]; a passing voter counts in
 * candidate k's parallax count when, with X its triangulated point, r1 = X, r2 = X + R_k^T t_k ((R^T t)_j = (R_0j t_0 + R_1j t_1) + R_2j t_2),
 * dot3(r1, r2) < max_cos_parallax * sqrt(dot3(r1, r1) * dot3(r2, r2)).  Integer sums: the order does not matter.  n_tested = the voters.
 * Choice: candidates ordered by (n_good descending, index ascending); best = the first; rivals = the others with (double)n_good[k] >=
 * ambiguity_ratio * (double)n_good[best].  Without a hint solution = best.  With a hint rot (9 floats row-major, the matrix vis_batch_f2f
 * takes: current-frame rays -> previous frame, i.e. ~ R^T) solution = the one of best and rivals, walked in that order, with the largest
 * trace(R_k (double)rot) = sum over i, j in row order of R_ij * rot_ji from 0; the first wins ties.  second = the first of the order that
 * is not solution.  The record carries both; whether to trust it is the caller's decision, as with `model`.
 * Flags: AMBIGUOUS = a rival and no hint; HINTED = a hint chose among two or more; FEW = (double)n_good[solution] < max((double)min_good,
 * good_share * (double)n_tested); LOW_PARALLAX = (double)n_parallax < parallax_share * (double)n_good[solution], n_parallax = the parallax
 * count of solution.  Two runs are byte-identical (no floating-point atomics). */
enum { VIS_HP_NONE = 0, VIS_HP_ROTATION = 1, VIS_HP_PLANE = 2 };
enum { VIS_HPF_AMBIGUOUS = 1, VIS_HPF_HINTED = 2, VIS_HPF_FEW = 4, VIS_HPF_LOW_PARALLAX = 8 };
typedef struct vis_hpose_params {        /* 48 bytes */
    double  min_t_over_d;                /* 0.05   below it the pair is a rotation (the measured separation of the test scenes) */
    double  max_cos_parallax;            /* 0.9998476951563913 = cos 1 deg, the paper's value */
    double  ambiguity_ratio;             /* 0.75   the paper's */
    double  good_share;                  /* 0.9    the paper's */
    double  parallax_share;              /* 0.5    this library's */
    int32_t min_good;                    /* 8      = vis_homography_params.min_inliers */
    int32_t reserved_;
} vis_hpose_params;
typedef struct vis_hpose_result {        /* 320 bytes */
    double  R[9], t[3], n[3];            /* the chosen candidate: x2 = R x1 + t, t in units of d, |n| = 1 */
    double  R2[9], t2[3], n2[3];         /* `second`; zeros when there is none */
    double  sv[3], t_norm;               /* d1, d2, d3; (d1 - d3) / d2 */
    int32_t n_good[4];                   /* votes of the four candidates */
    int32_t kind, flags, solution, second;   /* VIS_HP_*, VIS_HPF_*, candidate indices (-1: none) */
    int32_t n_tested, n_parallax, n_points, reserved_;
} vis_hpose_result;
void vis_default_hpose_params(vis_hpose_params* hq);
/* One pair, HOST pointers; blocks once.  h: the pair's homography record; p1xy / p2xy: m x 2 floats (pixels); mask: m bytes or NULL;
 * rot_hint: 9 floats or NULL. */
int  vis_homography_pose(vis_ctx* ctx, const vis_hpose_params* hq, const vis_homography_result* h, const float* p1xy, const float* p2xy, int m,
                         const uint8_t* mask, const float* rot_hint, vis_hpose_result* out);
/* DEVICE pointers, asynchronous on the context's stream, rows like vis_homography_batch's.  d_h: n homography records; d_mask: n rows of
 * row_cap bytes or NULL; d_rot: n x 9 floats or NULL; d_out: n records (a PLANE pair's record is the kernels' workspace until the call has
 * run: no scratch memory is taken). */
int  vis_homography_pose_batch(vis_ctx* ctx, const vis_hpose_params* hq, int n, const vis_homography_result* d_h, const float* d_p1,
                               const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask, const float* d_rot,
                               vis_hpose_result* d_out);
/* The same on the pairs of the last vis_batch_run, with d_h and d_mask as vis_batch_homography wrote them: on the POSE stream behind that call,
 * overlapping the next vis_batch_run like it; the caller's buffers are in use until vis_batch_sync.
 * Refusals of the three calls, in this order.  VIS_E_INVALID: a NULL pointer (the mask and the hint may be NULL), on the two device-pointer
 * calls a misaligned one (8 bytes for records and points, 4 for d_npts and d_rot; host pointers are copied and need none), a negative size, a parameter that is not finite, min_t_over_d < 0, max_cos_parallax, ambiguity_ratio, good_share or
 * parallax_share outside (0, 1], min_good < 1.  vis_homography_pose_batch: VIS_E_STATE without a context, then VIS_E_CAPACITY when a mask is
 * given and row_cap < max_pts or when max_pts > 2^29.  vis_batch_homography_pose: VIS_E_CAPACITY when a mask is given and row_cap is below the
 * plan's correspondences per pair, then VIS_E_STATE without context / plan / match stage or when n differs. */
int  vis_batch_homography_pose(vis_ctx* ctx, const vis_hpose_params* hq, int n, const vis_homography_result* d_h, int row_cap,
                               const uint8_t* d_mask, const float* d_rot, vis_hpose_result* d_out);

/* ---- homography polish: the RANSAC winner refined over its inliers, the set RE-SELECTED under the H it reached (OpenCV's findHomography refines
 * the same one-sided cost behind its RANSAC; the reference has no homography).  The call sits between vis_*_homography and vis_*_homography_pose:
 * it reads the record and mask the first wrote and writes a record and a mask the second reads unchanged, so homography -> polish ->
 * homography_pose chains on one stream with no host round trip (tests/homography_polish_ref.py restates every step, bit for bit).
 * All arithmetic is double, nothing is contracted, the only operations are + - * / sqrt and comparisons; every sum written with parentheses runs
 * in that order.  Coordinates: the pose stage's, x = ((double)u - cx) * (1 / fx), y likewise; (x, y) of the first image, (x2, y2) of the second.
 * t_sel = select_chi2 * (sigma_px * (1 / fx))^2 once on the host: with the defaults it is vis_*_homography's t_h.
 * Start: the record's H.  best_iter < 0, an entry that is not finite, or ss = H0 H0 + ... + H8 H8 (from k = 0, left to right) that is not > 0 or
 * not finite gives the ZERO record with flags = VIS_HPOL_NO_MODEL -- then the output mask row is left untouched and h_out receives the input
 * record unchanged.  Otherwise H <- H / sqrt(ss), entry by entry.
 * Per point under the current H:  U = (H0 x + H1 y) + H2, V = (H3 x + H4 y) + H5, w = (H6 x + H7 y) + H8;  iw = 1 / w, u = U iw, v = V iw;
 * ru = u - x2, rv = v - y2 (the forward transfer error);  a = x iw, b = y iw;  q = (a, b, iw), j0 = (-(a u), -(b u), -(iw u)),
 * j1 = (-(a v), -(b v), -(iw v)).  The Jacobian rows are J0 = (q, 0, j0) and J1 = (0, q, j1) in the nine entries of H.  A point outside the
 * set, or whose iw, u, v, ru or rv is not finite, adds +0.0 to every sum (ru, rv: a caller's mask may put a correspondence whose second point
 * is NaN or infinite into set 0; its NaN would reach the right-hand side through a finite Jacobian and the step would be NaN).
 * Sums, each under the summation contract "T" of vis_essential_polish (below: 256 partial sums over i mod 256, four wave totals added in rising
 * order), exactly as stated there.  Only the structurally non-zero products are formed -- a product with a zero of J0 or J1 is not:
 *   rows / columns 0 ... 2:  A_ab = sum q_a q_b (a <= b);  rows / columns 3 ... 5: the same six sums;  rows 0 ... 2 x columns 3 ... 5: +0.0;
 *   rows 0 ... 2 x columns 6 ... 8:  sum q_a j0_b;  rows 3 ... 5 x columns 6 ... 8:  sum q_a j1_b;
 *   rows / columns 6 ... 8:  sum j0_a j0_b + j1_a j1_b (a <= b);
 *   g_a = sum q_a ru (a = 0 ... 2), g_3+a = sum q_a rv, g_6+a = sum j0_a ru + j1_a rv;  the cost = sum ru ru + rv rv.
 * Gauge: p = the index of the largest |H_k| of the current iterate, the lowest on a tie (k rising from 0, replaced on > only).  Row and column p
 * are struck; the eight remaining unknowns keep their rising order.
 * Step: d = -A^-1 g by LDL^T without pivoting, exactly the PnP refinement's solve written for eight unknowns; a pivot that is not > 0 or not
 * finite ends the round's iteration (the iterates costed so far still compete).  Update: H_k <- H_k + d for k != p, then H <- H / sqrt(ss) as at
 * the start.
 * Passes, rounds and selection are vis_essential_polish's (below), word for word -- set 0 from the input mask's non-zero bytes (every point
 * without a mask), written to the output mask row as 0 / 1 where the current set lives from then on; n_set_first < min_inliers: VIS_HPOL_FEW, the
 * start reported with cost_first = cost0 = cost1; passes 0 ... refine_iters per round, the round reporting its iterate of least finite cost, the
 * earliest on a tie, costs compared within a round only; rounds 0 ... rounds with (1) the new set, (2) n_changed == 0: stop, (3) fewer than
 * min_inliers: stop with VIS_HPOL_SHRANK, (4) adopt -- with this re-selection test: G = adj(H) of the iterate the last round reported; the point
 * passes vis_*_homography's two-sided division-free transfer test at t_sel, e12 <= t_sel (w w) forward under H and backward under G, AND
 * t_sel (w w) is finite in both directions (inf <= inf would pass); a NaN fails.
 * Record: H = the last round's reported iterate, every entry negated when det = (H0 G0 + H1 G3) + H2 G6 < 0 (G = adj of it): unit Frobenius
 * norm, det >= 0, like vis_homography_result's.  cost_first, cost0, cost1, the counts and the flags have the meanings of vis_epolish_result's.
 * h_out (optional): the input vis_homography_result with H replaced by the reported H and n_inliers by n_set_last.  score_h, score_e, model,
 * best_iter, n_degenerate and n_inliers_e stay the input's: the scores and the H-or-E decision are those of the RANSAC winner, deliberately --
 * re-scoring under the refined H is not built.
 * The input record and the input mask are never modified.  Two runs are byte-identical.  Nothing is written into a plan. */
enum { VIS_HPOL_POLISHED = 1, VIS_HPOL_REJECTED = 2, VIS_HPOL_FEW = 4, VIS_HPOL_NO_MODEL = 8, VIS_HPOL_SHRANK = 16 };
typedef struct vis_hpolish_params {      /* 32 bytes; the defaults are this library's own */
    int32_t rounds;                      /* 3      re-selections, 0 ... 8; 0 = the refinement over set 0 alone */
    int32_t refine_iters;                /* 5      Gauss-Newton steps per round, 1 ... 64 */
    int32_t min_inliers;                 /* 8      a smaller set is not refined; refused below 5 */
    int32_t reserved_;                   /* 0 */
    double  select_chi2;                 /* 5.991  the re-selection's threshold: vis_homography_params.chi2_h; finite and > 0 */
    double  sigma_px;                    /* 1.0    finite and > 0 */
} vis_hpolish_params;
typedef struct vis_hpolish_result {      /* 128 bytes, 8-byte aligned, no implicit padding */
    double  H[9];                        /* the reported H: row-major, x2 ~ H x1; unit Frobenius norm, det >= 0 */
    double  cost_first;                  /* iterate 0 of round 0: the start's cost over set 0 */
    double  cost0, cost1;                /* of the last round run: its iterate 0 and its reported iterate, over that round's set */
    int32_t n_points, n_set_first, n_set_last;
    int32_t n_changed;
    int32_t rounds_run, steps_run, best_step;
    int32_t flags;                       /* VIS_HPOL_* */
} vis_hpolish_result;
void vis_default_hpolish_params(vis_hpolish_params* hp);
/* One pair, HOST pointers; blocks once like the other single-frame entry points.  h: the pair's homography record; p1xy / p2xy: m x 2 floats
 * (pixels); mask: m bytes or NULL; mask_out: m bytes; h_out: one record or NULL.
 * Refusals, in this order.  VIS_E_INVALID: a NULL out or h, m < 0, NULL points or a NULL mask_out with m > 0, hp NULL, hp.rounds < 0 or > 8,
 * hp.refine_iters < 1 or > 64, hp.min_inliers < 5, a select_chi2 or sigma_px that is not finite and positive, a reserved field that is not 0.
 * Then VIS_E_STATE without a context.  A refused call writes nothing. */
int  vis_homography_polish(vis_ctx* ctx, const vis_hpolish_params* hp, const vis_homography_result* h, const float* p1xy, const float* p2xy, int m,
                           const uint8_t* mask, vis_hpolish_result* out, uint8_t* mask_out, vis_homography_result* h_out);
/* DEVICE pointers, asynchronous on the context's stream: vis_homography_pose_batch's rows -- d_h: n records, d_mask: n rows of row_cap bytes or
 * NULL -- and d_mask_out: n rows of row_cap bytes (required), d_out: n records, d_h_out: n records or NULL.  One kernel in two shapes, chosen per
 * LAUNCH and without effect on a bit: one wave per pair when max_pts <= 64, four waves otherwise.  Rows may be as long as memory allows.
 * Refusals, in this order.  VIS_E_INVALID: what vis_homography_polish refuses of hp, a NULL or misaligned pointer (8 bytes for records and points,
 * 4 for counts; d_mask and d_h_out may be NULL), a negative size, d_mask_out overlapping d_mask or d_h_out overlapping d_h.  Then VIS_E_STATE
 * without a context.  Then VIS_E_CAPACITY when row_cap < max_pts. */
int  vis_homography_polish_batch(vis_ctx* ctx, const vis_hpolish_params* hp, int n, const vis_homography_result* d_h, const float* d_p1,
                                 const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask, uint8_t* d_mask_out,
                                 vis_hpolish_result* d_out, vis_homography_result* d_h_out);
/* The same on the pairs of the last vis_batch_run, with d_h and d_mask (n rows of mask_cap bytes, or NULL) as vis_batch_homography wrote them for
 * the same run -- caller buffers, like vis_batch_homography_pose's -- on the POSE stream behind that call, overlapping the next vis_batch_run; the
 * caller's buffers are in use until vis_batch_sync.  d_mask_out: n rows of row_cap bytes.  A frame without a pair (its record has best_iter =
 * -1) gets the NO_MODEL record.  vis_batch_homography_pose fed d_h_out and d_mask_out (at row_cap) then decomposes the polished H.
 * Refusals, in this order.  VIS_E_INVALID: what vis_homography_polish refuses of hp, a NULL d_h, d_mask_out or d_out, a misaligned (8 bytes) d_h,
 * d_out or d_h_out, n < 0, mask_cap < 0 or row_cap < 0, d_mask_out overlapping d_mask or d_h_out overlapping d_h.  Then VIS_E_STATE without
 * context / plan / match stage, or when n differs.  Then VIS_E_CAPACITY when row_cap, or with a mask mask_cap, is below the plan's
 * correspondences per pair. */
int  vis_batch_homography_polish(vis_ctx* ctx, const vis_hpolish_params* hp, int n, const vis_homography_result* d_h, int mask_cap,
                                 const uint8_t* d_mask, int row_cap, uint8_t* d_mask_out, vis_hpolish_result* d_out, vis_homography_result* d_h_out);

/* ---- PnP: the pose of a frame against map points, P3P RANSAC and Gauss-Newton refinement (Grunert 1841 as restated by Haralick, Lee,
 * Ottenberg, Noelle: "Review and analysis of solutions of the three point perspective pose estimation problem", 1994; the reference has
 * none).  A pose is (R, t) with x_cam = R X + t, X in the map's frame and units -- for the rows of vis_triangulate / vis_batch_triangulate,
 * the first camera of the pair in units of its baseline -- so t, unlike every two-view result above, has a scale.
 * Coordinates: the pose stage's, x = ((double)u - cx) * (1 / fx), y = ((double)v - cy) * (1 / fx) with the single focal the map points live in;
 * thr2 = (threshold_px * (1 / fx))^2 once on the host.  All arithmetic is double, nothing is contracted, the only operations are + - * / sqrt;
 * dot3(a, b) = a0 b0 + a1 b1 + a2 b2 and every sum of a 3 x 3 product run left to right (tests/pnp_ref.py restates every step in this order, bit
 * for bit).
 * Sample j of pp.iters takes i_k = (d_draws[3 j + k] & 0x7fffffff) % m, k = 0 ... 2 (ONE table of iters x 3 draws serves every problem).
 * Minimal solver.  Bearings f_k = (x / n, y / n, 1 / n), n = sqrt((x x + y y) + 1); world points P_k; p01 = P1 - P0, p02 = P2 - P0, p12 = P2 - P1;
 *   c2 = |p01|^2, b2 = |p02|^2, a2 = |p12|^2; ca = f1 . f2, cb = f0 . f2, cg = f0 . f1; p = (a2 - c2) / b2, q = (a2 + c2) / b2;
 *   A4 = (p - 1)^2 - 4 (c2 / b2) ca^2
 *   A3 = 4 [p (1 - p) cb - (1 - q) ca cg + 2 (c2 / b2) ca^2 cb]
 *   A2 = 2 [p^2 - 1 + 2 p^2 cb^2 + 2 ((b2 - c2) / b2) ca^2 - 4 q ca cb cg + 2 ((b2 - a2) / b2) cg^2]
 *   A1 = 4 [-p (1 + p) cb + 2 (a2 / b2) cg^2 cb - (1 - q) ca cg]
 *   A0 = (1 + p)^2 - 4 (a2 / b2) cg^2
 * (each bracket summed left to right, each product left to right).  Real roots v of A0 + ... + A4 v^4 in (0, B), B = 1 + max_k |A_k / A4|, by
 * derivative interlacing: the roots of the third, second and first derivative, found in turn, cut (0, B) into intervals with at most one
 * root each; an interval whose end values differ in sign (f < 0 against f >= 0) is halved, 40 times for a derivative and 100 times for the
 * quartic, an interval whose midpoint is not strictly inside staying as it is; the root is the last midpoint.  Ascending, at most four; the
 * root's place r is its slot.  For a root: den = 2 (cg - v ca); u = ((((p - 1) v^2 - 2 p cb v) + 1) + p) / den; w = (1 + v^2) - 2 v cb;
 * s0 = sqrt(b2 / w), s1 = u s0, s2 = v s0, Q_k = s_k f_k.  Rotation from two orthonormal triads: e1 = p01 / |p01|, e3 = (p01 x p02) / |p01 x p02|,
 * e2 = e3 x e1, g1, g2, g3 the same from Q1 - Q0 and Q2 - Q0; R_ij = (g1_i e1_j + g2_i e2_j) + g3_i e3_j; t = Q0 - R P0.
 * A sample is skipped and counted in n_degenerate when two of its indices are equal, when b2 is zero, when a coefficient is not finite or A4 is
 * zero, when |p01 x p02|^2 <= 2^-40 |p01|^2 |p02|^2, when B is not finite, or when no root yields a pose.  A root is dropped (its slot stays
 * empty) when den is zero or not finite, when v, u or w is not > 0, or when the camera triad fails the same collinearity test.  n_solutions
 * counts the poses of all samples.
 * Per-point test, division-free: (U, V, W) = R X + t (each row ((R_i0 X0 + R_i1 X1) + R_i2 X2) + t_i); an inlier iff W > 0, thr2 (W W) is
 * finite and (U - x W)^2 + (V - y W)^2 <= thr2 (W W); a NaN fails, and so does a point whose W W overflows or is infinite (inf <= inf would
 * otherwise pass under every pose).  Hypothesis h = 4 j + r: the largest count > 0 wins, ties go to the smallest h.  mask
 * receives the winner's inlier bytes (zeros when nothing won); bytes beyond the problem's points are left untouched.
 * Refinement: when refine_iters > 0 and n_inliers >= min_inliers, refine_iters Gauss-Newton steps over the winner's inliers (the set is
 * fixed).  Per point, with (U, V, W) under the current pose: iw = 1 / W, un = U / W, vn = V / W, residual (un - x, vn - y), j02 = -(un iw),
 * j12 = -(vn iw), Jacobian rows (rotation, then translation; the update is applied on the camera side)
 *   J0 = (j02 V, iw W - j02 U, -(iw V), iw, 0, j02),   J1 = (j12 V - iw W, -(j12 U), iw U, 0, iw, j12).
 * The 21 sums of J0_a J0_b + J1_a J1_b (a <= b), the 6 of J0_a rx + J1_a ry and the cost rx^2 + ry^2 are each taken in ONE fixed order (64 partial
 * sums over i mod 64 in rising i, a point outside the set adding 0, then the tree v = v + v[lane ^ off], off = 32 ... 1), without floating-point
 * atomics.  The step d = -(J^T J)^-1 J^T r by LDL^T without pivoting (D_j = A_jj - sum_c (L_jc L_jc) D_c, L_ij = (A_ij - sum_c (L_ic L_jc) D_c) / D_j,
 * c rising; z_i = -g_i - sum_c L_ic z_c; d_i = z_i / D_i - sum_{c > i} L_ci d_c, c rising); a pivot that is not > 0 or not finite ends the
 * refinement.  Update with the Cayley map: h = d_0..2 / 2, hh = h . h, s = 2 / (1 + hh), C_ij = delta_ij + s ([h]x_ij + (h_i h_j - delta_ij hh)),
 * R <- C R, t <- C t + d_3..5.  cost0 / cost1: the cost over the set under the winner and under the last pose reached (equal when no
 * refinement ran).  The refined pose is reported with VIS_PNP_REFINED iff cost1 is finite, cost1 <= cost0 and no pivot failed; otherwise the
 * winner with VIS_PNP_REFINE_REJECTED.  VIS_PNP_FEW: a winner below min_inliers, reported unrefined.  n_inliers_refined: the per-point test
 * under the reported pose over all points.  m < 4 or iters == 0: a zero record with best_iter = -1 (mask bytes of the problem zero).
 * Two runs are byte-identical. */
enum { VIS_PNP_REFINED = 1, VIS_PNP_REFINE_REJECTED = 2, VIS_PNP_FEW = 4 };
enum { VIS_PNP_TILE = 512 };             /* points per LDS tile of the kernel: rows longer than this are walked in several tiles */
typedef struct vis_pnp_params {          /* 24 bytes; the defaults are this library's own */
    int32_t iters;                       /* 200    three-point samples per problem (at most 2^29) */
    int32_t min_inliers;                 /* 8      below it the winner is not refined; refused below 4 */
    double  threshold_px;                /* 2.0    vis_default_tri_params' reprojection bound */
    int32_t refine_iters;                /* 5      Gauss-Newton steps; 0 = none */
    int32_t reserved_;
} vis_pnp_params;
typedef struct vis_pnp_result {          /* 240 bytes */
    double  R[9], t[3];                  /* the reported pose: x_cam = R X + t */
    double  R_ransac[9], t_ransac[3];    /* the winning P3P pose, always; zeros when nothing won */
    double  cost0, cost1;                /* sum of squared residuals (normalised coordinates) over the mask, before and after */
    int32_t n_inliers, n_points;
    int32_t best_iter, best_root;        /* the winning sample (-1: none) and its root's place */
    int32_t n_degenerate, n_solutions;
    int32_t n_inliers_refined;
    int32_t flags;                       /* VIS_PNP_* */
} vis_pnp_result;
void vis_default_pnp_params(vis_pnp_params* pp);
/* One problem, HOST pointers; blocks once like the other single-frame entry points.  X: m x 3 doubles; xy: m x 2 floats (pixels); draws:
 * pp.iters x 3; mask: m bytes or NULL. */
int  vis_pnp_ransac(vis_ctx* ctx, const vis_pnp_params* pp, const double* X, const float* xy, int m, const int32_t* draws, uint8_t* mask,
                    vis_pnp_result* out);
/* DEVICE pointers, asynchronous on the context's stream.  d_X: n rows of max_pts points, x_stride doubles from one point to the next (>= 3; 4
 * reads a row of vis_map_point in place); d_xy: n rows of max_pts (x, y) float pixels; d_npts[i] of them valid (clamped to max_pts); d_mask: n
 * rows of row_cap bytes or NULL; d_out: n records.
 * Refusals of these two calls, in this order.  VIS_E_INVALID: a NULL pointer (the mask may be NULL), on the device-pointer call a misaligned one
 * (8 bytes for d_X, d_xy and records, 4 for d_npts and d_draws), a negative size, x_stride < 3, pp.iters < 0 or > 2^29, pp.min_inliers < 4,
 * pp.refine_iters < 0, a threshold_px that is not finite and positive.  Then VIS_E_STATE without a context.  Then, vis_pnp_batch only,
 * VIS_E_CAPACITY when a mask is given and row_cap < max_pts. */
int  vis_pnp_batch(vis_ctx* ctx, const vis_pnp_params* pp, int n, const double* d_X, int x_stride, const float* d_xy, const int32_t* d_npts,
                   int max_pts, const int32_t* d_draws, int row_cap, uint8_t* d_mask, vis_pnp_result* d_out);

/* The same for every frame of the last vis_batch_run (which must have included VIS_STAGE_MATCH and VIS_STAGE_POSE; n = its frames) against the map
 * points vis_batch_triangulate wrote for that run: d_points / d_flags are its rows of row_cap entries.  For frame i, with q its keyframe
 * (vis_batch_get_keyframes) and p the keyframe of q: correspondence c of pair (q -> i) is linked to the FIRST correspondence k of pair (p -> q)
 * whose keypoint in frame q is the same (vis_dmatch.trainIdx of k == vis_dmatch.queryIdx of c, the lists the pose stage saw) and whose flags
 * contain every bit of `require` (VIS_MP_KEPT is the usual choice; 0 links every triangulated row).  The problem is X = d_points[q][k].X against
 * c's pixel in frame i, in rising c, solved like a row of vis_pnp_batch with the same d_draws for every frame: d_out[i] is the pose of frame i in
 * the frame of p, in units of the baseline p -> q; d_mask (rows of mask_cap bytes, or NULL) receives the inlier bytes of the n_linked rows.
 * d_link[i] always carries n_linked and q and p as vis_batch_get_keyframes numbers them (VIS_KF_* where there is none; p = q when q is no frame
 * of this launch), and where d_out[i] has a winner the motion q -> i in the same units: R_rel = R R_pq^T ((R_i0 Rpq_j0 + R_i1 Rpq_j1) + R_i2 Rpq_j2),
 * t_rel = t - R_rel t_pq, scale = sqrt(dot3(t_rel, t_rel)) -- this pair's baseline in units of the previous one -- with (R_pq, t_pq) the pose
 * record of pair q; zeros otherwise.  There is no problem (n_linked = 0, d_out[i] the zero record) when the frame has no pair, when q's pair has
 * no pose (R all zero), or when q lies in an earlier launch (frame 0, and whatever else the gate carries): the last case sets VIS_PNPL_NO_MAP --
 * joining across launches needs the carried pair's match list, which the plan does not keep.  Asynchronous on the POSE stream behind
 * vis_batch_triangulate of the same run, overlapping the next vis_batch_run like it; the caller's buffers are in use until vis_batch_sync.  The
 * workspace (a keypoint table and the linked rows per frame) is allocated by the first call of a plan.
 * Refusals, in this order.  VIS_E_INVALID: what vis_pnp_batch refuses of pp, a NULL d_draws / d_points / d_flags / d_out / d_link, d_points not
 * 16-byte or records not 8-byte aligned, a negative size, require outside 0 ... 255.  VIS_E_CAPACITY: row_cap, or with a mask mask_cap, below
 * the plan's correspondences per pair.  VIS_E_STATE: no context / plan / match stage / pose stage, or n differs. */
enum { VIS_PNPL_NO_MAP = 1 };
typedef struct vis_pnp_link {            /* 120 bytes */
    double  R_rel[9], t_rel[3];          /* frame q -> frame i: x_i = R_rel x_q + t_rel */
    double  scale;                       /* |t_rel|: the baseline q -> i in units of the baseline p -> q */
    int32_t n_linked;
    int32_t q, p;                        /* frame indices of this launch, or VIS_KF_* */
    int32_t flags;                       /* VIS_PNPL_* */
} vis_pnp_link;
int  vis_batch_pnp(vis_ctx* ctx, const vis_pnp_params* pp, int n, const int32_t* d_draws, const vis_map_point* d_points, const uint8_t* d_flags,
                   int row_cap, int require, int mask_cap, uint8_t* d_mask, vis_pnp_result* d_out, vis_pnp_link* d_link);

/* ---- the essential-matrix pose on device rows, and its refinement (the reference has neither: its findEssentialMat / recoverPose run once per
 * frame on host vectors, src/VISystem.cpp:1679-1701, and the five-point winner is never touched again) ---- */
/* The pose stage of vis_batch_run on caller-made rows: DEVICE pointers, asynchronous on the context's stream.  d_p1 / d_p2: n rows of max_pts
 * (x, y) float pixels, d_npts[i] of them valid (clamped to max_pts); d_mask: n rows of row_cap bytes, or NULL; d_out: n records, the layout
 * vis_batch_results_async writes.  Row i is what vis_essential_ransac followed by vis_recover_pose give for that row alone with the context's
 * parameters -- the same sample stream from (ransac_seed, M), the same adaptive stop, mask, E, R, t and counts -- except that a row without a
 * model (E all zero) has R = 0 and t = 0 as the batch path's records do, where vis_recover_pose on a zero E reports NaN.  Mask bytes beyond a
 * row's correspondences are left untouched.  The workspace (what a single call carves for one pair, times n) belongs to the context, is sized by
 * n, max_pts and ransac_max_iters and only grows: the first call, and any call that grows it, drains every stream of the context before the old
 * block is freed, so such a call SYNCHRONISES; VIS_E_NOMEM when the block cannot be allocated.
 * Refusals, in this order.  VIS_E_INVALID: a NULL or misaligned pointer (8 bytes for points and records, 4 for counts; the mask may be NULL) or
 * a negative size.  VIS_E_STATE without a context.  VIS_E_CAPACITY when max_pts > 8192 (the limit of every RANSAC problem), or when a mask is
 * given and row_cap < max_pts. */
int  vis_essential_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts,
                         int row_cap, uint8_t* d_mask, vis_pose_result* d_out);

/* Two-view refinement: Gauss-Newton on the Sampson distance over a fixed set of correspondences, from the (R, t) of a pose record.
 * Coordinates: the pose stage's, x = ((double)u - cx) * (1 / fx), y = ((double)v - cy) * (1 / fx), x1 = (x, y, 1) of the first image and x2 of the
 * second; thr = threshold_px / fx and thr2 = thr thr once on the host.  All arithmetic is double, nothing is contracted, the only operations are
 * + - * / sqrt and comparisons; dot3(a, b) = a0 b0 + a1 b1 + a2 b2, cross3 the usual (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), both left to right
 * (tests/essential_refine_ref.py restates every step in this order, bit for bit).
 * Start: the record's (R, t).  An all-zero R (what the pose stage leaves where there is no model or no pair), any entry of R or t that is not
 * finite, or |t|^2 = dot3(t, t) that is not > 0 or not finite gives the ZERO record with flags = VIS_ER_NO_POSE.  Otherwise t <- t / sqrt(|t|^2).
 * Set: the points i < m (m = the row's count clamped to 0 ... max_pts) whose mask byte is non-zero, every point when there is no mask; fixed for
 * the whole refinement; n_used counts it.  refine_iters == 0 or n_used < min_inliers: no refinement; the start is reported with best_step = 0,
 * steps_run = 0, cost1 = cost0, and VIS_ER_FEW when n_used < min_inliers.
 * For a matrix M (row-major) and x1 = (a, b, 1), x2 = (c, d, 1):  l_k(M) = (M_k0 a + M_k1 b) + M_k2;  m_k(M) = (M_0k c + M_1k d) + M_2k;
 * s(M) = (c l_0 + d l_1) + l_2.  "v x M" is the matrix whose column j is cross3(v, column j of M).
 * Model: E = t x R.  Residual of a point: r = s / sd with s = s(E), den = ((l_0^2 + l_1^2) + m_0^2) + m_1^2 (l, m of E), sd = sqrt(den): the signed
 * Sampson distance.  A point outside the set, or with den not > 0 or not finite, adds 0 to every sum below.
 * Parameters: rotation w (3), applied on the left of R, and a move (d_0, d_1) in the tangent plane of t.  Tangent basis of t: e = the unit axis of
 * t's smallest |component| (the lowest index on a tie), c = cross3(t, e), b1 = c / sqrt(dot3(c, c)), b2 = cross3(t, b1).  Derivative matrices
 * G_a = t x (e_a x R), a = 0, 1, 2 (e_a x R written out: rows (0, -R_2, R_1), (R_2, 0, -R_0), (-R_1, R_0, 0) of R's rows), G_3 = b1 x R, G_4 = b2 x R.
 * Jacobian, complete (the denominator is differentiated): with g = s(G_a), l', m' of G_a:  dd = 2 (((l_0 l'_0 + l_1 l'_1) + m_0 m'_0) + m_1 m'_1),
 * J_a = g / sd - ((0.5 s) dd) / (den sd).
 * Sums: the 15 of J_a J_b (a <= b, row order), the 5 of J_a r and the cost r r, each in ONE fixed order: 64 partial sums over i mod 64 in rising i, then
 * the tree v = v + v[lane ^ off], off = 32 ... 1; no floating-point atomics.
 * Step: (w, d) = -(J^T J)^-1 J^T r by LDL^T without pivoting, exactly the PnP refinement's solve above for five unknowns; a pivot that is not > 0 or
 * not finite ends the iteration (the poses costed so far still compete).  Update: R <- C(w) R with the PnP refinement's Cayley map;
 * v_k = (t_k + b1_k d_0) + b2_k d_1, t <- v / sqrt(dot3(v, v)) (b1, b2 of the t before the move).
 * Iterates: pass k = 0 ... refine_iters costs the current pose (iterate k) and, for k < refine_iters, solves and updates.  THE REPORTED POSE IS THE
 * ITERATE OF LEAST FINITE COST, the earliest on a tie (plain Gauss-Newton is not monotone here); iterate 0 is reported when no cost is finite.
 * best_step = its index, steps_run = the updates applied; cost0 = iterate 0's cost, cost1 = the reported one's, so cost1 <= cost0.  When a refinement
 * ran: VIS_ER_REFINED iff best_step > 0, else VIS_ER_REJECTED.  E = t x R of the reported pose.
 * n_inliers0 / n_inliers_refined: the points of the WHOLE row (not only the set) with thr2 den finite and s s <= thr2 den under the start and under
 * the reported pose (a NaN fails, and so does a point whose den is infinite: inf <= inf would pass); reported, not used.  The input mask is never modified, and the set is not re-selected after the refinement.
 * The refined pose is NOT written back: vis_batch_triangulate, vis_batch_pnp and vis_batch_track keep reading the pose stage's record.
 * Two runs are byte-identical. */
enum { VIS_ER_REFINED = 1, VIS_ER_REJECTED = 2, VIS_ER_FEW = 4, VIS_ER_NO_POSE = 8 };
typedef struct vis_eref_params {         /* 16 bytes; the defaults are this library's own */
    int32_t refine_iters;                /* 5      Gauss-Newton steps, 0 ... 64; 0 = none */
    int32_t min_inliers;                 /* 8      a smaller set is not refined; refused below 6 */
    double  threshold_px;                /* 1.0    of the reported inlier counts only (vis_params.ransac_threshold's default) */
} vis_eref_params;
typedef struct vis_eref_result {         /* 216 bytes, 8-byte aligned */
    double  R[9], t[3];                  /* the reported pose, |t| = 1 */
    double  E[9];                        /* t x R of the reported pose */
    double  cost0, cost1;                /* sum of squared Sampson distances (normalised coordinates) over the set: iterate 0, reported iterate */
    int32_t n_used, n_points;
    int32_t n_inliers0, n_inliers_refined;
    int32_t best_step, steps_run;
    int32_t flags;                       /* VIS_ER_* */
    int32_t reserved_;
} vis_eref_result;
void vis_default_eref_params(vis_eref_params* ep);
/* One pair, HOST pointers; blocks once like the other single-frame entry points.  R: 9 doubles row-major, t: 3; p1xy / p2xy: m x 2 floats (pixels);
 * mask: m bytes or NULL.
 * Refusals, in this order.  VIS_E_INVALID: a NULL out, R or t, m < 0, NULL points with m > 0, ep NULL, ep.refine_iters < 0 or > 64,
 * ep.min_inliers < 6, a threshold_px that is not finite and positive.  Then VIS_E_STATE without a context. */
int  vis_essential_refine(vis_ctx* ctx, const vis_eref_params* ep, const double R[9], const double t[3], const float* p1xy, const float* p2xy,
                          int m, const uint8_t* mask, vis_eref_result* out);
/* DEVICE pointers, asynchronous on the context's stream: exactly what vis_essential_batch writes and reads -- d_pose: n records; d_p1 / d_p2: n rows
 * of max_pts (x, y) float pixels, d_npts[i] of them valid (clamped); d_mask: n rows of row_cap bytes or NULL; d_out: n records -- so that
 * vis_batch_klt -> vis_essential_batch -> vis_essential_refine_batch runs without a host round trip.
 * Refusals, in this order.  VIS_E_INVALID: what vis_essential_refine refuses of ep, a NULL or misaligned pointer (8 bytes for records and points,
 * 4 for counts; the mask may be NULL), a negative size.  Then VIS_E_STATE without a context.  Then VIS_E_CAPACITY when a mask is given and
 * row_cap < max_pts. */
int  vis_essential_refine_batch(vis_ctx* ctx, const vis_eref_params* ep, int n, const vis_pose_result* d_pose, const float* d_p1, const float* d_p2,
                                const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask, vis_eref_result* d_out);
/* The same on the pairs of the last vis_batch_run (which must have included VIS_STAGE_MATCH and VIS_STAGE_POSE; n = its frames): the correspondences
 * the pose stage saw, its inlier mask (vis_batch_get_inlier_mask) and its pose records.  A frame without a pair gets the zero record with
 * VIS_ER_NO_POSE.  Asynchronous on the POSE stream behind the pose stage, overlapping the next vis_batch_run like vis_batch_homography: d_out is in
 * use until vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: what vis_essential_refine refuses of ep, a NULL or misaligned (8 bytes) d_out, n < 0.  Then VIS_E_STATE
 * without context / plan / match stage / pose stage, or when n differs. */
int  vis_batch_essential_refine(vis_ctx* ctx, const vis_eref_params* ep, int n, vis_eref_result* d_out);

/* Two-view polish: the refinement above with its set RE-SELECTED under the pose it reached, and the result in a pose record that
 * vis_batch_triangulate_from reads (tests/essential_polish_ref.py restates every step on essential_refine_ref's functions, bit for bit).
 * Everything the refinement's contract states holds here -- coordinates, residual, Jacobian, solve, updates -- except the order of the sums:
 * Summation contract "T" (tiled), for each of the 21 sums:
 *   partial sum j, j = 0 ... 255, adds the terms of the points i = j (mod 256) in rising i, starting from +0.0;
 *   W_w, w = 0 ... 3, is the tree v = v + v[lane ^ off], off = 32 ... 1, over the partial sums 64 w ... 64 w + 63;
 *   the sum is ((W_0 + W_1) + W_2) + W_3.  No floating-point atomics; every thread ends with the same bits; integer counts in any order.
 * A partial sum is never -0.0 (it starts at +0.0), so neither is a W.  A row of at most 64 points has W_1 = W_2 = W_3 = +0.0 and its sum is W_0
 * bit for bit: the one-wave contract of vis_essential_refine.  The device therefore runs one kernel in two shapes, chosen per LAUNCH and without
 * effect on a bit: one wave per pair when max_pts <= 64, four waves (thread tid owns the residue tid, the wave totals added in rising w) otherwise.
 * Start: vis_essential_refine's, from the record's (R, t): the same tests give the ZERO record with flags = VIS_EP_NO_POSE -- then the output mask row
 * is left untouched and pose_out receives the input record unchanged -- and otherwise t <- t / sqrt(|t|^2), once.
 * Set 0: the points i < m (m = the row's count clamped to 0 ... max_pts) whose input mask byte is non-zero, every point without a mask; it is written
 * to the output mask row, bytes 0 / 1 for i < m, and the current set lives there from then on; n_set_first counts it.  thr = select_px / fx and
 * thr2 = thr thr once on the host.
 * n_set_first < min_inliers: VIS_EP_FEW; the start is reported with cost_first = cost0 = cost1 = its cost over set 0, n_set_last = n_set_first and
 * rounds_run = steps_run = best_step = n_changed = 0.
 * Otherwise round k = 0 ... rounds:
 *   k >= 1: (1) the NEW set = the points of the whole row with thr2 den finite and s s <= thr2 den under the pose reported by round k - 1 (a NaN
 *           fails, and so does a point whose den is infinite: inf <= inf would pass); n_changed = the bytes in which it differs from the current set.
 *           (2) n_changed == 0: stop.  (3) the new set has fewer than min_inliers points: stop with VIS_EP_SHRANK; the current set and pose stay.
 *           (4) otherwise the new set becomes the current one.
 *   then vis_essential_refine's passes 0 ... refine_iters over the current set, from the pose reported by round k - 1 (round 0: from the start): the
 *   round reports its iterate of least finite cost, the earliest on a tie.  Costs are compared within a round only -- two sets' costs do not compare.
 * Record: the pose reported by the last round run and E = t x R of it; cost_first = iterate 0 of round 0; cost0 / cost1 / best_step = the last round
 * run's iterate 0, reported iterate and its index, so cost1 <= cost0; n_set_last = the current set at the end; n_changed = of the last selection made
 * (0 when none was); rounds_run = the rounds run, round 0 included; steps_run = the updates applied in all rounds.  VIS_EP_POLISHED iff some round
 * reported an iterate other than its first (the pose moved), else VIS_EP_REJECTED.
 * Output mask: the set the reported pose was fitted on (n_set_last bytes are 1); bytes beyond a row's points are left untouched.  The input mask is
 * never modified.  pose_out (optional): the input record with E, R, t replaced by the reported pose and n_inliers by n_set_last.
 * rounds = 0 on a row of at most 64 points: R, t, E, cost0, cost1, best_step are vis_essential_refine's, byte for byte.  Two runs are byte-identical.
 * Nothing is written into a plan: vis_batch_track and vis_batch_pnp's links (vis_pnp_link) still read the pose stage's record. */
enum { VIS_EP_POLISHED = 1, VIS_EP_REJECTED = 2, VIS_EP_FEW = 4, VIS_EP_NO_POSE = 8, VIS_EP_SHRANK = 16 };
typedef struct vis_epolish_params {      /* 32 bytes; the defaults are this library's own */
    int32_t rounds;                      /* 3      re-selections, 0 ... 8; 0 = the refinement over set 0 alone */
    int32_t refine_iters;                /* 5      Gauss-Newton steps per round, 1 ... 64 */
    int32_t min_inliers;                 /* 8      a smaller set is not refined; refused below 6 */
    int32_t reserved_;                   /* 0 */
    double  select_px;                   /* 2.0    the re-selection's threshold in pixels, finite and > 0 */
    int32_t reserved2_[2];               /* 0 */
} vis_epolish_params;
typedef struct vis_epolish_result {      /* 224 bytes, 8-byte aligned, no implicit padding */
    double  R[9], t[3];                  /* the reported pose, |t| = 1 */
    double  E[9];                        /* t x R of the reported pose */
    double  cost_first;                  /* iterate 0 of round 0: the start's cost over set 0 */
    double  cost0, cost1;                /* of the last round run: its iterate 0 and its reported iterate, over that round's set */
    int32_t n_points, n_set_first, n_set_last;
    int32_t n_changed;
    int32_t rounds_run, steps_run, best_step;
    int32_t flags;                       /* VIS_EP_* */
} vis_epolish_result;
void vis_default_epolish_params(vis_epolish_params* ep);
/* One pair, HOST pointers; blocks once like the other single-frame entry points.  R, t, p1xy, p2xy, m, mask as for vis_essential_refine; mask_out:
 * m bytes; pose_out: one record or NULL -- its input record is all zero but for R, t and n_points = m.
 * Refusals, in this order.  VIS_E_INVALID: a NULL out, R or t, m < 0, NULL points or a NULL mask_out with m > 0, ep NULL, ep.rounds < 0 or > 8,
 * ep.refine_iters < 1 or > 64, ep.min_inliers < 6, a select_px that is not finite and positive, a reserved field that is not 0.  Then VIS_E_STATE
 * without a context.  A refused call writes nothing. */
int  vis_essential_polish(vis_ctx* ctx, const vis_epolish_params* ep, const double R[9], const double t[3], const float* p1xy, const float* p2xy,
                          int m, const uint8_t* mask, vis_epolish_result* out, uint8_t* mask_out, vis_pose_result* pose_out);
/* DEVICE pointers, asynchronous on the context's stream: vis_essential_refine_batch's rows -- d_mask: n rows of row_cap bytes or NULL -- and
 * d_mask_out: n rows of row_cap bytes (required), d_out: n records, d_pose_out: n records or NULL.  Rows may be as long as memory allows: the 8192
 * of a RANSAC problem does not apply.
 * Refusals, in this order.  VIS_E_INVALID: what vis_essential_polish refuses of ep, a NULL or misaligned pointer (8 bytes for records and points,
 * 4 for counts; d_mask and d_pose_out may be NULL), a negative size, d_mask_out overlapping d_mask or d_pose_out overlapping d_pose.  Then
 * VIS_E_STATE without a context.  Then VIS_E_CAPACITY when row_cap < max_pts. */
int  vis_essential_polish_batch(vis_ctx* ctx, const vis_epolish_params* ep, int n, const vis_pose_result* d_pose, const float* d_p1, const float* d_p2,
                                const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask, uint8_t* d_mask_out,
                                vis_epolish_result* d_out, vis_pose_result* d_pose_out);
/* The same on the pairs of the last vis_batch_run (which must have included VIS_STAGE_MATCH and VIS_STAGE_POSE; n = its frames), as
 * vis_batch_essential_refine: the pose stage's correspondences, mask (read, never written) and records.  d_mask_out: n rows of row_cap bytes with
 * row_cap >= the plan's correspondences per pair (root^2, or the keypoint capacity with VIS_POSE_SYM).  A frame without a pair gets the NO_POSE
 * record.  Asynchronous on the POSE stream behind the pose stage, overlapping the next vis_batch_run: the caller's buffers are in use until
 * vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: what vis_essential_polish refuses of ep, a NULL d_mask_out or d_out, a misaligned (8 bytes) d_out or
 * d_pose_out, n < 0 or row_cap < 0.  Then VIS_E_STATE without context / plan / match stage / pose stage, or when n differs.  Then VIS_E_CAPACITY
 * when row_cap is below the plan's correspondences per pair. */
int  vis_batch_essential_polish(vis_ctx* ctx, const vis_epolish_params* ep, int n, int row_cap, uint8_t* d_mask_out, vis_epolish_result* d_out,
                                vis_pose_result* d_pose_out);
/* vis_batch_triangulate with the pose records (R, t, n_points are read) and the mask rows taken from CALLER device buffers -- those
 * vis_batch_essential_polish wrote for the same run -- instead of the plan's; the correspondences are still the plan's.  d_pose: n records, 8-byte
 * aligned; d_mask: n rows EXACTLY the plan's correspondences per pair apart (mask_cap states the distance; the triangulation reads its mask at the
 * row length of its points), or NULL for every point an inlier.  Fed the plan's own records and mask it gives vis_batch_triangulate's bytes.  Same
 * stream, ordering and buffer lifetimes as vis_batch_triangulate, which is also what orders it behind a vis_batch_essential_polish queued before it.
 * Records or mask rows that anything else wrote must be complete before the call: like vis_batch_triangulate it does not wait for the context's stream.
 * vis_batch_pnp takes its points from the caller already, so polish -> triangulate_from -> pnp chains with nothing more; vis_batch_pnp's links
 * (vis_pnp_link) and vis_batch_track still read the plan's record.
 * Refusals, in this order.  VIS_E_INVALID: what vis_batch_triangulate refuses, a NULL or misaligned d_pose, mask_cap < 0.  Then VIS_E_STATE as
 * vis_batch_triangulate.  Then VIS_E_CAPACITY when row_cap is below the plan's correspondences per pair, or d_mask is given and mask_cap differs
 * from it. */
int  vis_batch_triangulate_from(vis_ctx* ctx, const vis_tri_params* tp, int n, const vis_pose_result* d_pose, int mask_cap, const uint8_t* d_mask,
                                int row_cap, vis_map_point* d_points, uint8_t* d_flags, vis_tri_summary* d_summary);

/* ---- rotation-guided matching ("search by projection"): the 2-NN search of the matcher restricted to a window around the position the
 * pair's rotation predicts -- VISystem::WarpFunctionRT (src/VISystem.cpp:771-860; its call sites :500-504 are commented out in the reference)
 * put in front of the matcher.  rot: row-major 3x3 f32, the matrix vis_batch_f2f takes (current-frame rays -> previous frame, :1031-1033).
 * Prediction of a keypoint (u, v) of the CURRENT frame, with fx, fy, cx, cy = params narrowed to float once:
 *     a = (u - cx) / fx, b = (v - cy) / fy                                     (float)
 *     X_k = (float)((double)r_k0 a + (double)r_k1 b + (double)r_k2), k = 0..2  (summed left to right in double: OpenCV's float Mat * Mat,
 *                                                                               restated from memory, UNPINNED -- DESIGN.md section 2)
 *     x' = fx X_0 / X_2 + cx,  y' = fy X_1 / X_2 + cy                          (float, every operation rounded, in this order, no FMA)
 * Deviation from the reference, which divides by whatever X_2 is: (x', y') = (NaN, NaN) when !(X_2 > 0).
 * Window: previous keypoint i at (x_i, y_i) and current keypoint j may be matched iff
 *     fabsf(x'_j - x_i) <= radius && fabsf(y'_j - y_i) <= radius               (square; false for a NaN; the same test in both directions)
 * out12[i] = the two nearest admissible j (ascending distance, ties -> lower index), out21[j] likewise over admissible i; a row with fewer
 * than two admissible candidates has trainIdx = -1 in the missing places, exactly what the unguided matcher returns when the other set has
 * fewer than two rows, so the filters (fewer than 2 neighbours -> dropped, src/Matcher.cpp:162-165) apply unchanged.
 * Every call: VIS_E_INVALID for a NULL rot / d_rot, a radius that is negative or not finite, a non-finite entry of a HOST rot (and what the
 * unguided twin refuses); then VIS_E_STATE without a context or plan.  vis_timings.ms_knn of a guided call includes the prediction kernel. */
/* predictions of one set of keypoints, HOST pointers: out_xy receives n x 2 floats.  Blocks once. */
int  vis_warp_keypoints(vis_ctx* ctx, const vis_keypoint* kps, int n, const float rot[9], float* out_xy);
/* vis_bf_knn2_hamming inside the window; slot_q = previous frame, slot_t = current frame */
int  vis_bf_knn2_hamming_guided(vis_ctx* ctx, int slot_q, int slot_t, const float rot[9], float radius,
                                vis_dmatch* out12, vis_dmatch* out21);
/* vis_bf_knn2_hamming_host with the keypoints of both sets (q = previous, t = current).  The device rows are as long as the larger set, or
 * as params.keypoint_capacity when that is larger (above 16384 the popcount kernel runs, as for slots of such a context). */
int  vis_bf_knn2_hamming_guided_host(vis_ctx* ctx, const uint8_t* desc_q, const vis_keypoint* kps_q, int n_q,
                                     const uint8_t* desc_t, const vis_keypoint* kps_t, int n_t, const float rot[9], float radius,
                                     vis_dmatch* out12, vis_dmatch* out21);
/* vis_good_matches on the windowed 2-NN */
int  vis_good_matches_guided(vis_ctx* ctx, int slot_prev, int slot_cur, const float rot[9], float radius,
                             vis_dmatch* good, int cap, int* n_good, vis_dmatch* sym_out, int sym_cap, int* n_sym);
/* vis_batch_run whose match stage is windowed (stages without VIS_STAGE_MATCH: VIS_E_INVALID).  d_rot: DEVICE pointer, n_frames x 9 floats;
 * frame i's pair -- in vis_batch_get_keyframes' pairing, keyframe gate off or on, the pair to the carried frame included -- uses d_rot[9 i]
 * (vis_batch_f2f's convention).  d_rot is read on the match stream, behind what is queued on the context's stream so far, and is in use
 * until vis_batch_sync.  Everything downstream (filters, pose, vis_batch_f2f, triangulation, tracking, vis_batch_results_async) consumes
 * the matches as it does vis_batch_run's.  Nothing is remembered: a later vis_batch_run is unguided.  The prediction buffer (n_pairs x
 * keypoint capacity x 8 bytes) is allocated by the first guided call of a plan. */
int  vis_batch_run_guided(vis_ctx* ctx, const uint8_t* d_frames, int n_frames, int stages, const float* d_rot, float radius);

/* ---- pyramidal KLT: follow keypoints from one frame into the next by their image patch (Lucas-Kanade, coarse to fine) -----------------
 * Beyond the reference, off unless called.  Reads what the gradient stage leaves on the device: the half pyramid (vis_half_pyramid_dims) and
 * its Scharr gx / gy (int16, made with OpenCV's `scale` = scharr_scale).  The arithmetic is part of the contract (tests/klt_ref.py restates it
 * and the device reproduces it byte for byte): every inner sum is an integer, everything else is double arithmetic with + - * / sqrt in the
 * order written here, never contracted.
 *   Level geometry.  A level-0 position maps to level l as x_l = (x_0 + 0.5) / 2^l - 0.5 (pixel i of level l+1 is the mean of pixels 2i, 2i+1).
 *   Window fit.  With r = win_radius and n = (2r+1)^2, a window fits at (x, y) on a level of lw x lh pixels iff x, y are finite,
 *     floor(x) - r >= 0, floor(y) - r >= 0, floor(x) + r + 1 <= lw - 1, floor(y) + r + 1 <= lh - 1 -- tested in double before any
 *     conversion to an integer.  Nothing outside a level's lw x lh pixels is ever read; there is no border mode.
 *   Sampling.  X = floor(x), Y = floor(y), a = x - X, b = y - Y; w00 = rint(((1-a)(1-b)) 16384.0), w01 = rint((a (1-b)) 16384.0),
 *     w10 = rint(((1-a) b) 16384.0), w11 = 16384 - w00 - w01 - w10 (rint: half to even; w11 may be -1).  For window offset (i, j) in [-r, r]^2:
 *     S = w00 img[Y+j][X+i] + w01 img[Y+j][X+i+1] + w10 img[Y+j+1][X+i] + w11 img[Y+j+1][X+i+1];
 *     intensities T, J = (S + 256) >> 9 (1/32 grey level); gradients D = (S + 8192) >> 14 (int16 Scharr units); arithmetic shifts.
 *   One pass (template frame A, target frame B, start p0 in double, optional guess g).  d = 0, or (g - p0) / 2^first_level when both
 *   components of g are finite.  For l = first_level ... last_level: d <- 2 d when l < first_level; p_l = the level position of p0;
 *     (a) the template window at p_l does not fit: the level is skipped; at last_level the point is lost, VIS_KLT_OOB;
 *     (b) T, Dx, Dy from A's level l; Gxx = sum Dx^2, Gxy = sum Dx Dy, Gyy = sum Dy^2 (int64) -> doubles fxx, fxy, fyy;
 *         det = fxx fyy - fxy fxy;  lam = ((fxx + fyy) - sqrt((fxx - fyy)(fxx - fyy) + 4.0 (fxy fxy))) / (((2.0 n)(32.0 s))(32.0 s));
 *         !(det > 0 && lam >= min_eig): the level is skipped; at last_level the point is lost, VIS_KLT_FLAT;
 *     (c) up to max_iters times: the window at p_l + d does not fit in B: the level ends; at last_level the point is lost, VIS_KLT_OOB.
 *         Else J from B, e = J - T, bx = sum Dx e, by = sum Dy e (int64), ux = -(s (fyy bx - fxy by)) / det, uy = -(s (fxx by - fxy bx)) / det,
 *         d += u, one iteration counted; stop when ux ux + uy uy <= epsilon epsilon.
 *   Behind last_level: one more sample of B at p_last + d (same fit rule, VIS_KLT_OOB), sad = sum |J - T|; the pass ends at
 *   p0 + d 2^last_level.
 *   A point.  p0 = the float input widened; a non-finite input gives VIS_KLT_INVALID, reads no image and leaves a zero record otherwise.
 *     Forward pass A = frame 1, B = frame 2.  A lost point reports x, y = its input; else x, y = (float)(p0 + d 2^last_level), and VIS_KLT_ERR
 *     is set when max_err > 0 and (double)sad > (max_err 32.0) n.  Forward-backward, when fb_max_px > 0 and no flag is set so far: the same
 *     pass with the frames swapped from the float result, with p0 as its guess, ending at q: dx, dy = q - p0 in double,
 *     fb = (float)sqrt(dx dx + dy dy), VIS_KLT_FB when dx dx + dy dy > fb_max_px fb_max_px; a lost backward pass gives fb = -1 and VIS_KLT_FB.
 *     VIS_KLT_TRACKED is set iff no other flag is.  min_eig = (float)lam of last_level when (b) was reached there; iters = the forward
 *     pass's iterations over all levels; levels = bit l for every level that reached (c) in the forward pass. */
enum { VIS_KLT_TRACKED = 1, VIS_KLT_OOB = 2, VIS_KLT_FLAT = 4, VIS_KLT_ERR = 8, VIS_KLT_FB = 16, VIS_KLT_INVALID = 32 };
enum { VIS_KLT_NO_PAIR = 1 };
typedef struct vis_klt_params {          /* 56 bytes */
    int32_t win_radius;                  /* 7     2 ... 10: the window is (2r+1)^2 pixels */
    int32_t first_level;                 /* 3     last_level ... 4 */
    int32_t last_level;                  /* 0     0 ... first_level */
    int32_t max_iters;                   /* 10    1 ... 30, per level */
    double  epsilon;                     /* 0.01  px, finite and >= 0; 0 = never stop early */
    double  min_eig;                     /* 0.1   grey^2 / px^2 per pixel, finite and >= 0 (the order of OpenCV's 1e-4 in these units) */
    double  max_err;                     /* 0     mean absolute grey-level residual, finite and >= 0; 0 = off */
    double  fb_max_px;                   /* 0     forward-backward bound in px, finite and >= 0; 0 = off */
    int32_t scharr_scale;                /* 3     1 ... 8: what the gradients were made with (the plan's stage always uses 3) */
    int32_t reserved_;                   /* 0 */
} vis_klt_params;
typedef struct vis_klt_point {           /* 32 bytes */
    float    x, y;                       /* the point in frame 2 (a lost point: its input) */
    float    fb;                         /* forward-backward distance in px; 0 when it did not run, -1 when the backward pass was lost */
    float    min_eig;
    int32_t  sad;
    int32_t  flags;                      /* VIS_KLT_* */
    uint16_t iters;
    uint8_t  levels;
    uint8_t  pad_[5];                    /* 0 */
} vis_klt_point;
typedef struct vis_klt_pair {            /* 32 bytes */
    int32_t n_points, n_tracked, n_oob, n_flat, n_err, n_fb, n_invalid;
    int32_t flags;                       /* VIS_KLT_NO_PAIR */
} vis_klt_pair;
void vis_default_klt_params(vis_klt_params* kp);
/* Refusals of the three calls that need no device, in this order.  VIS_E_INVALID: a NULL pointer that is not optional; a negative size;
 * a parameter outside the ranges above or reserved_ != 0; w, h outside 16 ... 4095 or stride < w; on the device-pointer calls a record
 * pointer that is not 8-byte or a point / count pointer that is not 4-byte aligned.  Then VIS_E_STATE without a context (vis_batch_klt:
 * or without a plan, a run, its DETECT and GRADIENT stages, or with another n).
 * One pair, HOST pointers, shaped like vis_estimate_pose_features: level l images are dense lw[l] x lh[l]; levels outside
 * [last_level, first_level] may be NULL; gx2 / gy2 (or their level pointers) may be NULL when fb_max_px == 0.  pts: m x 2 floats;
 * guess: m x 2 floats or NULL; out: m records; pair: one record (n_points = m).  Blocks once. */
int  vis_klt_track(vis_ctx* ctx, const vis_klt_params* kp, int w, int h,
                   const uint8_t* const gray1[5], const int16_t* const gx1[5], const int16_t* const gy1[5],
                   const uint8_t* const gray2[5], const int16_t* const gx2[5], const int16_t* const gy2[5],
                   const float* pts, const float* guess, int m, vis_klt_point* out, vis_klt_pair* pair);
/* DEVICE pointers, shaped like vis_align_batch: n frames and the outputs of vis_gradient_batch for them.  Pair i = (frame i-1 -> frame i),
 * i = 1 ... n-1, tracks the first d_npts[i] (clamped to 0 ... max_pts) of d_pts' row i (max_pts x 2 floats per pair); d_guess: rows like
 * d_pts or NULL.  d_out: n rows of max_pts records, of which the pair's n_points are written; d_pair: n records.  Row 0 has no pair: its
 * max_pts records are zeroed and its pair record is zero but for VIS_KLT_NO_PAIR.  d_p1 / d_p2 / d_ntracked (all three or none): per pair the
 * VIS_KLT_TRACKED points in rising index, frame-1 input and frame-2 result, as rows of max_pts x 2 floats -- the layout vis_homography_batch,
 * vis_f2f_batch, vis_filter_keypoints_batch and vis_pnp_batch read -- and their count (0 for row 0); places behind the count are left alone.
 * Any stride >= w; a level too small for any window is skipped by the fit rule, not refused.  Asynchronous on the context's stream. */
int  vis_klt_batch(vis_ctx* ctx, const vis_klt_params* kp, const uint8_t* d_frames, int w, int h, int stride, int n,
                   const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                   const float* d_pts, const int32_t* d_npts, int max_pts, const float* d_guess,
                   vis_klt_point* d_out, vis_klt_pair* d_pair, float* d_p1, float* d_p2, int32_t* d_ntracked);
/* The same on the pairs of the last vis_batch_run, whose stages must have included DETECT and GRADIENT (n = its frames; kp->scharr_scale must
 * be 3): the points of pair i are ALL keypoints of frame prev[i], in vis_batch_get_keyframes' pairing with the gate off or on, tracked into
 * frame i.  Rows have the plan's keypoint capacity (row_cap >= it, else VIS_E_CAPACITY): d_out n x row_cap records, d_guess / d_p1 / d_p2
 * n x row_cap x 2 floats.  A frame without a pair, and a pair to the carried frame (whose gradients are not in this launch's set: what
 * vis_batch_align does with pair 0), gets the records of its row zeroed (the plan's keypoint capacity of them), n_tracked 0 and a pair record
 * that is zero but for VIS_KLT_NO_PAIR.
 * Runs on the context's POSE stream with vis_batch_align's ordering and buffer-lifetime rules: behind everything queued on the context's
 * stream so far (the gradients, the detection), overlapping the next vis_batch_run; d_frames, the plan's gradients and keypoints and the
 * caller's buffers are in use until vis_batch_sync -- or until the later vis_batch_run / vis_gradient_batch / vis_feeder_submit /
 * vis_rectify_batch that would overwrite them, which wait for it. */
int  vis_batch_klt(vis_ctx* ctx, const vis_klt_params* kp, const uint8_t* d_frames, int n, const float* d_guess, int row_cap,
                   vis_klt_point* d_out, vis_klt_pair* d_pair, float* d_p1, float* d_p2, int32_t* d_ntracked);

/* ---- rectification (vi::CameraModel, src/CameraModel.cpp:84-105; VISystem::CalculateROI, src/VISystem.cpp:162-205) -------------
 * Opt-in: nothing else in this header remaps a frame (the reference's GPU main hands frames on un-remapped, src/VISystemGPU.cpp:137-146).
 * Restatements of OpenCV 3.2 written from the published algorithm; parity with real OpenCV is UNPINNED.
 * K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2); sizes 1 ... 4095; fx, fy (and fx', fy') finite and > 0, else VIS_E_INVALID. */
/* cv::getOptimalNewCameraMatrix(K, dist, Size(in_w, in_h), alpha = 1, Size(out_w, out_h)) -> Knew = (fx', fy', cx', cy').  Host only. */
int  vis_optimal_new_camera_matrix(const float K[4], const float dist[4], int in_w, int in_h, int out_w, int out_h, float Knew[4]);
/* cv::initUndistortRectifyMap(K, dist, R = I, Knew, Size(out_w, out_h), CV_16SC2, map1, map2).  Host only.
 * map1: out_h x out_w x 2 int16 (source pixel x, y = floor(32 u) >> 5), map2: out_h x out_w uint16 ((v & 31) * 32 + (u & 31) in 1/32 px). */
int  vis_undistort_rectify_map(const float K[4], const float dist[4], const float Knew[4], int out_w, int out_h,
                               int16_t* map1, uint16_t* map2);
/* Device tables of one calibration: built once on the host (vis_undistort_rectify_map) and uploaded.  A vis_rectify belongs to its
 * context and is destroyed before it.  VIS_E_NODEVICE without a GPU (no context can exist then). */
typedef struct vis_rectify vis_rectify;
int  vis_rectify_create(vis_ctx* ctx, const float K[4], const float dist[4], const float Knew[4], int in_w, int in_h,
                        int out_w, int out_h, vis_rectify** out);
void vis_rectify_destroy(vis_rectify* r);
/* the tables, copied to the host (either pointer may be NULL); equal to vis_undistort_rectify_map's.  Synchronises. */
int  vis_rectify_maps(vis_rectify* r, int16_t* map1, uint16_t* map2);
/* remap(INTER_LINEAR, BORDER_CONSTANT, 0) of n frames, bit-exact to OpenCV 3.2's fixed-point 8U path with these tables: per output
 * pixel (sx, sy) = map1, a = map2 & 1023, fractions i = a >> 5 (y), j = a & 31 (x), D = (S00 32(32-i)(32-j) + S01 32(32-i)j +
 * S10 32 i(32-j) + S11 32 i j + 16384) >> 15, a tap outside the in_w x in_h source reading 0.
 *   d_in: n dense frames of in_h rows x in_stride bytes (in_stride >= in_w).  d_out: the window (x0, y0, w, h) of the rectified
 *   out_w x out_h image (remap, then crop: VISystem::CalculateROI's frame without a copy), n frames of h rows x out_stride bytes
 *   (out_stride >= w; the frame stride is out_stride * h -- a vis_batch_plan(ctx, w, h, out_stride, n) reads it as it is).
 *   Asynchronous on the context's detect stream (the stream of vis_set_stream / its own): a vis_batch_run on d_out that follows is
 *   ordered behind it, and a vis_feeder_release after that run also covers this read of the feeder's buffer.  d_out follows the
 *   reuse rules of vis_batch_run's d_frames for whatever call reads it last: vis_batch_align / vis_batch_track read their frames
 *   on the pose stream until vis_batch_sync.  This call orders itself behind the alignment that read d_out's range (the detect stream
 *   waits for it, as vis_feeder_submit's copy does), so rewriting d_out is safe; a pipelined caller double-buffers d_out (alternates
 *   two buffers) so that the wait is for the alignment of two steps back, not the last one. */
int  vis_rectify_batch(vis_rectify* r, const uint8_t* d_in, int in_stride, int n, int x0, int y0, int w, int h,
                       uint8_t* d_out, int out_stride);
/* one host frame (in_h rows x in_stride bytes) -> the full out_w x out_h rectified frame (out_stride >= out_w): CameraModel::Undistort
 * (src/CameraModel.cpp:103-105).  Through the context's staging block like the other single-frame entry points; blocks once. */
int  vis_rectify_host(vis_rectify* r, const uint8_t* img, int in_stride, uint8_t* out, int out_stride);

/* ---- feature tracks: the matches of a stream linked over any number of frames, and their N-view triangulation (the reference has neither:
 * its matcher, like everything above, knows one frame and its keyframe).  "ftrack" because vis_batch_track means CAMERA tracking.
 * The track contract (tests/ftrack_ref.py restates it; every result below is integer arithmetic and equals it byte for byte).
 * A LINK LIST of frame i is a list of vis_dmatch whose queryIdx is a keypoint of frame prev[i] and whose trainIdx is a keypoint of frame i
 * (vis_batch_pnp's orientation).  prev[i] is an index < i or a VIS_KF_* value; any other value counts as VIS_KF_FIRST.  A frame takes part with
 * nk(i) keypoints: 0 when prev[i] == VIS_KF_NOT_SAVED, else its count clamped to [0, row capacity].  The parent frame of i is frame prev[i] when
 * that is an index, the carried row when prev[i] == VIS_KF_CARRIED and a row is given (its keypoints are the entries with len > 0), else none.
 * Correspondence c of the first m entries (m = the list's count clamped to [0, link_cap], with a mask also to mask_cap) is a CANDIDATE iff the
 * frame has a parent, trainIdx < nk(i) and queryIdx is a keypoint of the parent (both compared unsigned: a negative index is out of range), and
 * its mask byte, when a mask is given, is non-zero.  A candidate LINKS keypoint trainIdx of frame i to keypoint queryIdx of the parent iff no
 * candidate earlier in the list has the same trainIdx and none has the same queryIdx: the first in list order wins on BOTH sides, so a track
 * never forks and never merges.  (A candidate that loses on one side still occupies the other: of (q0, t0), (q0, t1), (q1, t1) only the first
 * links.  That is what makes the rule one atomic minimum per side and independent of scheduling; the plan's own lists are one-to-one already.)
 * A linked keypoint continues its parent's track, every other keypoint k < nk(i) starts one.
 * Per keypoint a vis_ftrack_obs: birth_seq = the stream number of the frame the track started in (frame i of a call is seq0 + i; the plan counts
 * the frames of every vis_batch_run with VIS_STAGE_DETECT since vis_batch_plan / vis_batch_reset), birth_kp = the keypoint index of its first
 * observation -- (birth_seq, birth_kp) is the track's identity: unique, no counter, the same however a stream is cut into launches -- len = the
 * observations up to and including this one (>= 1), prev_kp = the parent's keypoint, or -1 where the track starts.  Entries k >= nk(i) of a
 * row, up to its capacity, are (-1, -1, 0, -1).
 * Per frame a vis_ftrack_frame: seq, n_keypoints = nk(i), n_continued, n_started, n_ended = the parent's keypoints that no keypoint of i
 * continues (0 without a parent), max_len, sum_len (the caller divides; wraps beyond 2^31), flags: VIS_FT_NO_PAIR = no parent (VIS_KF_FIRST,
 * VIS_KF_NOT_SAVED, frame 0 after a reset), VIS_FT_NO_CARRY = prev[i] is VIS_KF_CARRIED but no row is held (rows form: d_carry_in NULL; plan form:
 * the launch before was not linked) -- every keypoint of such a frame starts a track; not an error. */
enum { VIS_FT_NO_PAIR = 1, VIS_FT_NO_CARRY = 2 };
enum { VIS_FT_SYM = 0, VIS_FT_GOOD = 1 };
typedef struct vis_ftrack_obs { int32_t birth_seq, birth_kp, len, prev_kp; } vis_ftrack_obs;                               /* 16 bytes */
typedef struct vis_ftrack_frame { int32_t seq, n_keypoints, n_continued, n_started, n_ended, max_len, sum_len, flags; } vis_ftrack_frame;   /* 32 bytes */
/* Caller-made rows, DEVICE pointers, asynchronous on the context's stream, no plan.  d_prev, d_nkp, d_nlinks: n entries; d_links: n rows of
 * link_cap entries; d_mask: NULL or n rows of mask_cap bytes; d_carry_in: NULL or ONE row of row_cap observations, those of the frame
 * VIS_KF_CARRIED refers to; d_obs: n rows of row_cap records; d_frame: n records.  Every entry of d_obs and d_frame is written.  The workspace
 * (24 bytes per entry of d_obs) belongs to the context and only grows; a call that grows it SYNCHRONISES.  On the device: the candidates take an
 * atomic minimum of their list position per side, one pass writes every keypoint's parent, ceil(log2 n) rounds of pointer doubling between two
 * buffers replace every keypoint's (ancestor, distance) by its ancestor's -- no kernel loops over the frames -- and one workgroup per frame
 * writes the records and reduces the summary in integers.
 * Refusals, in this order.  VIS_E_INVALID: a NULL d_prev, d_nkp, d_nlinks, d_obs or d_frame, a NULL d_links with link_cap > 0, a pointer that is
 * not aligned (16 bytes for d_links, d_carry_in and d_obs, 4 for the rest), n, link_cap, mask_cap, row_cap or seq0 negative.  VIS_E_STATE without a
 * context.  VIS_E_CAPACITY when n x row_cap exceeds 2^28 entries. */
int  vis_ftrack_link_rows(vis_ctx* ctx, int n, const int32_t* d_prev, const int32_t* d_nkp, const vis_dmatch* d_links, const int32_t* d_nlinks,
                          int link_cap, const uint8_t* d_mask, int mask_cap, const vis_ftrack_obs* d_carry_in, int seq0, int row_cap,
                          vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame);
/* The pairs of the last vis_batch_run (which must have included VIS_STAGE_MATCH; n = its frames), with vis_batch_get_keyframes' pairing, keyframe
 * gate off or on.  source: VIS_FT_SYM = every symmetric match of a pair, VIS_FT_GOOD = the grid-filtered good matches.  d_mask: NULL or caller rows
 * of mask_cap bytes aligned with that list (a polish's mask); pose_inliers != 0 uses the pose stage's own mask instead (vis_batch_get_inlier_mask,
 * its first n_points bytes) and excludes a d_mask.  d_obs: n rows of row_cap >= the plan's keypoint capacity; only the first keypoint-capacity
 * entries of a row are written.  The plan keeps a copy of the row of the last SAVED frame of the launch (beside the keyframe gate's carried
 * record) and the stream number of frame 0: the next call continues those tracks across the launch boundary, a launch that saved nothing carries
 * the earlier row forward, vis_batch_plan / vis_batch_reset forget the row and restart seq at 0, and a launch that was not linked makes the frames
 * of the next one whose pair is the carried keyframe VIS_FT_NO_CARRY.  Calling it again for the same run repeats the result: every call of a run
 * continues the row the run was given, and a vis_batch_run without VIS_STAGE_DETECT in between does not begin a new run.  When the calls of one
 * run differ (another source, another mask), the row of the LAST call is the one the next run continues.  Asynchronous on the
 * POSE stream behind the matcher of that run (and, when a d_mask is given, behind the context's stream), overlapping the next vis_batch_run like
 * vis_batch_triangulate; the caller's buffers are in use until vis_batch_sync.  The workspace is allocated by the first call of a plan.
 * Refusals, in this order.  VIS_E_INVALID: a NULL or misaligned d_obs (16 bytes) or d_frame (4), n, mask_cap or row_cap negative, a source that is
 * neither VIS_FT_SYM nor VIS_FT_GOOD, pose_inliers together with a d_mask.  VIS_E_CAPACITY: row_cap below the plan's keypoint capacity, or with a
 * d_mask mask_cap below the list's row length (the keypoint capacity, or root^2 for VIS_FT_GOOD).  VIS_E_STATE: no context / plan / match stage, or n
 * differs.  Then VIS_E_INVALID when pose_inliers is set and the last run had no VIS_STAGE_POSE or source is not the list the pose stage saw. */
int  vis_batch_ftrack(vis_ctx* ctx, int source, int pose_inliers, int n, const uint8_t* d_mask, int mask_cap, int row_cap,
                      vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame);

/* N-view triangulation of the tracks.  d_poses: n x 12 doubles per frame, R row-major then t, x_cam = R X + t in ONE common frame and scale; a
 * frame whose 12 numbers are not all finite or whose R is all zero has no pose (the pose record's convention).  The poses are the caller's (a
 * VIO, a chained and scaled PnP, ground truth) or the d_poses of vis_trajectory_rows / vis_batch_trajectory below, which chain the two-view poses
 * of a stream under the common scale of vis_scale_link_rows / vis_batch_scale_links without a host step.
 * A point is computed for every keypoint (i, k), k < nk(i), that is the LAST observation of its track inside the call: no keypoint of a later
 * frame names it as its parent (prev[] index and prev_kp < nk of that frame).  Every other entry k < nk(i) gets the zero record and flags 0; entries
 * k >= nk(i) are left untouched.  The lane walks back from (i, k) along prev_kp / prev[] through at most max_views observations of this call --
 * observations of earlier launches are not held: a limitation -- and USES those whose frame has a pose and whose pixel (u, v) is finite (a
 * non-finite pixel drops the view; a finite one, however large, is used as it stands and ends in flags that fail).  Fewer than min_views used
 * views: VIS_FTP_FEW, n_views set, everything else zero.  Otherwise, all in double, nothing contracted, only + - * / sqrt, sums in view order
 * from the newest to the oldest, with (fx, fy, cx, cy) of the context's parameters and x = (u - cx) / fx, y = (v - cy) / fy:
 *   1. DLT: per view the rows r = x P_2 - P_0 and s = y P_2 - P_1 of P = [R | t]; the ten sums A_ab += r_a r_b + s_a s_b (a <= b), mirrored.
 *   2. The eigenvector of the smallest eigenvalue (the first on ties) by the Jacobi iteration of vis_triangulate; X = (v_0, v_1, v_2) / v_3.
 *      v_3 == 0, a quotient that is not finite, or a cost of that point (step 3) that is not finite -- the point lies in a camera's plane, or
 *      something overflowed: VIS_FTP_SINGULAR, n_views set, everything else zero.  No reported number is ever a NaN or an infinity.
 *   3. Up to gn_iters Gauss-Newton steps on the pixel error.  Per view (U, V, W) = R X + t (each row ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i),
 *      iw = 1 / W, un = U iw, vn = V iw, residual ru = (fx un + cx) - u, rv = (fy vn + cy) - v, Jacobian rows Ju_j = (fx iw) (R_0j - un R_2j),
 *      Jv_j = (fy iw) (R_1j - vn R_2j); H_ab += Ju_a Ju_b + Jv_a Jv_b (a <= b), g_a += Ju_a ru + Jv_a rv, cost += ru ru + rv rv.  Step by LDL^T
 *      without pivoting: D0 = H00, L10 = H01 / D0, L20 = H02 / D0, D1 = H11 - (L10 L10) D0, L21 = (H12 - (L20 L10) D0) / D1,
 *      D2 = (H22 - (L20 L20) D0) - (L21 L21) D1; z0 = -g0, z1 = -g1 - L10 z0, z2 = (-g2 - L20 z0) - L21 z1; d2 = z2 / D2, d1 = z1 / D1 - L21 d2,
 *      d0 = (z0 / D0 - L10 d1) - L20 d2; X <- X + d.  A pivot that is not > 0 or not finite ends the steps.  EVERY iterate is costed, the DLT point
 *      included, and the first of least cost is reported (an iterate replaces the best only with cost < best): the cost never rises above the DLT
 *      point's and a NaN iterate cannot win.
 *   4. vis_ftrack_point: X, rms_reproj_px = (float)sqrt(cost / n_views), parallax_cos = (float) of a . b / sqrt((a . a)(b . b)) with a, b the
 *      vectors from X to the centres -R^T t of the newest and the oldest used camera (the COSINE: the device's atan2 and a host's need not agree
 *      bit for bit, so no angle is formed and the threshold is a cosine, like vis_hpose_params.max_cos_parallax; a quotient that is not finite is
 *      reported as 1 and fails the threshold), n_views, flags:
 *      VIS_FTP_FRONT W > 0 in every used view, VIS_FTP_REPROJ_OK ru ru + rv rv <= max_reproj_px^2 in every used view, VIS_FTP_PARALLAX_OK
 *      parallax_cos (before rounding) <= max_parallax_cos, VIS_FTP_KEPT all three.
 * d_flags: the flags as bytes, rows of row_cap.  d_summary[i]: the counts of frame i.  Two runs are byte-identical. */
enum { VIS_FTP_FRONT = 1, VIS_FTP_REPROJ_OK = 2, VIS_FTP_PARALLAX_OK = 4, VIS_FTP_KEPT = 8, VIS_FTP_FEW = 16, VIS_FTP_SINGULAR = 32 };
typedef struct vis_ftrack_tri_params {   /* 32 bytes; the defaults are this library's own */
    int32_t max_views;                   /* 16     observations walked back from a track's end, 2 ... 32 */
    int32_t min_views;                   /* 2      used views below which no point is formed, 2 ... max_views */
    int32_t gn_iters;                    /* 5      Gauss-Newton steps, 0 ... 10 */
    int32_t reserved_;                   /* 0 */
    double  max_reproj_px;               /* 2.0    finite, > 0, at most 1e6 */
    double  max_parallax_cos;            /* cos(1 degree) = 0.9998476951563913; in (-1, 1] */
} vis_ftrack_tri_params;
typedef struct vis_ftrack_point { double X[3]; float rms_reproj_px, parallax_cos; int32_t n_views, flags; } vis_ftrack_point;   /* 40 bytes */
typedef struct vis_ftrack_tri_summary { int32_t n_ends, n_points, n_kept, n_front, n_reproj_ok, n_parallax_ok, n_few, n_singular; } vis_ftrack_tri_summary;   /* 32 bytes; n_points = ends with neither FEW nor SINGULAR */
void vis_default_ftrack_tri_params(vis_ftrack_tri_params* tp);
/* Caller-made rows, DEVICE pointers, asynchronous on the context's stream.  d_prev, d_nkp: n entries; d_obs: n rows of row_cap observations (only
 * prev_kp is read, and checked against nk of the parent frame); d_xy: n rows of row_cap (u, v) float pixels; d_poses: n x 12 doubles; d_points /
 * d_flags: n rows of row_cap entries; d_summary: n records.
 * Refusals, in this order.  VIS_E_INVALID: tp NULL or outside the ranges above, a NULL pointer, a pointer that is not aligned (16 bytes for d_obs, 8
 * for d_xy, d_poses and d_points, 4 for d_prev, d_nkp and d_summary), n or row_cap negative.  VIS_E_STATE without a context.  VIS_E_CAPACITY when
 * n x row_cap exceeds 2^28 entries. */
int  vis_ftrack_triangulate_rows(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, const int32_t* d_prev, const int32_t* d_nkp,
                                 const vis_ftrack_obs* d_obs, int row_cap, const float* d_xy, const double* d_poses, vis_ftrack_point* d_points,
                                 uint8_t* d_flags, vis_ftrack_tri_summary* d_summary);
/* The keypoints of the last vis_batch_run (n = its frames) with the observations vis_batch_ftrack wrote for it (d_obs, rows of row_cap) and
 * vis_batch_get_keyframes' pairing: on the POSE stream behind vis_batch_ftrack of the same run and behind the context's stream (where d_poses may
 * have been produced), overlapping the next vis_batch_run; the caller's buffers are in use until vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: what vis_ftrack_triangulate_rows refuses of tp, a NULL or misaligned d_obs, d_poses, d_points, d_flags or
 * d_summary, n or row_cap negative.  VIS_E_CAPACITY: row_cap below the plan's keypoint capacity.  VIS_E_STATE: no context / plan / match stage, or n
 * differs. */
int  vis_batch_ftrack_triangulate(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, const vis_ftrack_obs* d_obs, int row_cap,
                                  const double* d_poses, vis_ftrack_point* d_points, uint8_t* d_flags, vis_ftrack_tri_summary* d_summary);

/* ---- a scaled trajectory: consecutive two-view poses given one scale, and chained (the reference has neither: its monocular poses stay
 * pairwise, |t| = 1).  Two steps, each on caller rows and on the plan; tests/scale_link_ref.py and tests/trajectory_ref.py restate them, and every
 * record equals its restatement byte for byte: double arithmetic, + - * / and comparisons only, nothing contracted.
 * FRAMES.  prev[i] is an index < i, VIS_KF_CARRIED or VIS_KF_NOT_SAVED; any other value counts as VIS_KF_FIRST (the q / parent fields report the
 * value so normalised).  A frame HAS A PAIR when prev[i] is an index or VIS_KF_CARRIED; its pose record (R, t, x_i = R x_q + t) is USABLE when its 12
 * numbers are finite, R is not all zero and (t0 t0 + t1 t1) + t2 t2 is finite and > 0 (vis_essential_refine's convention).
 *
 * 1. SCALE LINKS.  Frame i with keyframe q = prev[i]: the length of baseline q -> i in units of the baseline of q's own pair p -> q, from the map
 * points both pairs share through a keypoint of frame q.  The list of frame i holds vis_dmatch entries with queryIdx a keypoint of q and trainIdx
 * a keypoint of i (vis_batch_pnp's orientation); its first m entries count, m = the list's count clamped to [0, min(link_cap, pts_cap)]; entry k
 * has the map point d_points[i][k] and the flag byte d_flags[i][k] of vis_batch_triangulate's layout (X in camera q, in units of baseline q -> i).
 * An entry QUALIFIES when its flag byte contains every bit of `require`.
 *   DEPTH ROW of frame i, row_cap doubles, one per keypoint of i: zero throughout unless i has a pair and a usable pose record.  Else keypoint kp
 *   gets the depth of the FIRST qualifying entry k in list order with trainIdx == kp (an integer minimum of k, as k_pnp_link does; trainIdx is
 *   compared unsigned against row_cap: a negative index is out of range): z2 = ((R[6] X0 + R[7] X1) + R[8] X2) + t[2] -- the depth in camera i in
 *   units of i's baseline -- when z2 is finite and > 0, else 0; a keypoint without a qualifying entry gets 0.
 *   RATIOS of frame i: every qualifying entry c whose queryIdx (unsigned < row_cap) has an entry z2 in q's depth row that is finite and > 0 and
 *   whose own z1 = X[2] is finite and > 0 gives rho = z2 / z1, kept when finite and > 0; n_shared counts them.  q's row is row q of this call, or
 *   d_depth_carry_in when q is VIS_KF_CARRIED.
 *   RECORD: scale = the lower median of the ratios, element (n_shared - 1) / 2 of their ascending order; q25 and q75 = elements (n_shared - 1) / 4
 *   and 3 (n_shared - 1) / 4 (integer divisions) -- order statistics, defined by value; with n_shared == 0 all three are 0.  flags:
 *   VIS_SL_NO_PAIR (i has no pair) and VIS_SL_NO_DEPTH (q is VIS_KF_CARRIED without a carried row, or q's row has no entry that is finite and > 0:
 *   q had no pair, no usable pose or no qualifying point -- a test of the row alone, so a carried row answers as the frame itself would) stand
 *   alone, with n_shared = 0; otherwise VIS_SL_FEW (n_shared < min_shared), VIS_SL_SPREAD (q75 - q25 > max_rel_spread * scale) and VIS_SL_RANGE (scale not
 *   inside [min_scale, max_scale]) in any combination, and VIS_SL_OK = 0 when none applies.  No reported number is ever a NaN or an infinity.
 * On the device: one workgroup per frame and two passes.  The depth pass settles the winner by a 64-bit atomic minimum in the row itself.  The
 * ratio pass keeps the ratios' bit patterns (a positive finite double orders like its 64-bit pattern; an entry without a ratio is the pattern 0,
 * which orders first) in LDS when m <= 1024 and in the workspace beyond that, and SELECTS the three ranks in one walk of eight 8-bit digits, an LDS
 * histogram per rank and digit, integers only, the pass count independent of the data.  Nothing is sorted. */
enum { VIS_SL_OK = 0, VIS_SL_NO_PAIR = 1, VIS_SL_NO_DEPTH = 2, VIS_SL_FEW = 4, VIS_SL_SPREAD = 8, VIS_SL_RANGE = 16 };
typedef struct vis_scale_link_params {   /* 32 bytes; the defaults are this library's own */
    int32_t require;                     /* VIS_MP_KEPT   flag bits an entry must carry, 0 ... 255 */
    int32_t min_shared;                  /* 8             ratios below which the link is VIS_SL_FEW, 1 ... 2^20 */
    double  max_rel_spread;              /* 1.0           (q75 - q25) / scale above which it is VIS_SL_SPREAD; finite, >= 0, at most 1e6 (loose on
                                                          purpose: DESIGN.md 4.19 has the spreads measured at 0.3 px and 1 px of noise) */
    double  min_scale, max_scale;        /* 1/64, 64      finite, 0 < min_scale <= max_scale */
} vis_scale_link_params;
typedef struct vis_scale_link { double scale, q25, q75; int32_t n_shared, q, flags, reserved_; } vis_scale_link;           /* 40 bytes */
void vis_default_scale_link_params(vis_scale_link_params* sp);
/* Caller-made rows, DEVICE pointers, asynchronous on the context's stream, no plan.  d_prev, d_nlinks: n entries; d_links: n rows of link_cap;
 * d_pose: n pose records (only R and t are read); d_points / d_flags: n rows of pts_cap; d_depth_carry_in: NULL or ONE row of row_cap doubles, the
 * depth row of the frame VIS_KF_CARRIED refers to; d_depth: n rows of row_cap doubles -- a pointer to one of its rows is a later call's carried
 * row, as vis_ftrack_link_rows chains through d_obs; d_link: n records.  Every entry of d_depth and d_link is written.  The workspace (8 bytes per
 * list entry, only when min(link_cap, pts_cap) > 1024) belongs to the context and only grows; a call that grows it SYNCHRONISES.
 * Refusals, in this order.  VIS_E_INVALID: sp NULL or outside the ranges above, a NULL d_prev, d_nlinks, d_pose, d_depth or d_link, a NULL d_links,
 * d_points or d_flags with min(link_cap, pts_cap) > 0, a pointer that is not aligned (16 bytes for d_links and d_points, 8 for d_pose, d_depth,
 * d_depth_carry_in and d_link, 4 for d_prev and d_nlinks), n, link_cap, pts_cap or row_cap negative.  VIS_E_STATE without a context.
 * VIS_E_CAPACITY when n x row_cap or n x link_cap exceeds 2^28 entries. */
int  vis_scale_link_rows(vis_ctx* ctx, const vis_scale_link_params* sp, int n, const int32_t* d_prev, const vis_dmatch* d_links,
                         const int32_t* d_nlinks, int link_cap, const vis_pose_result* d_pose, const vis_map_point* d_points, const uint8_t* d_flags,
                         int pts_cap, const double* d_depth_carry_in, int row_cap, double* d_depth, vis_scale_link* d_link);
/* The pairs of the last vis_batch_run (which must have included VIS_STAGE_POSE; n = its frames) with vis_batch_get_keyframes' pairing, the pose
 * stage's lists and records, and d_points / d_flags as vis_batch_triangulate wrote them for that run (rows of row_cap >= the plan's
 * correspondences per pair), as vis_batch_pnp reads them.  The depth rows (keypoint capacity doubles each) live in the plan's workspace, allocated by
 * the first call.  The plan keeps the row of the last SAVED frame of the launch, so the pair to the keyframe carried from the launch before has
 * its depth row -- what vis_batch_pnp cannot do (VIS_PNPL_NO_MAP) -- and the links of a stream are the same bytes however it is cut into
 * launches.  It keeps TWO rows and uses them in turn: a call repeated for the same run reads the row the run was given.  A launch that saved nothing
 * carries the earlier row forward; vis_batch_plan / vis_batch_reset forget the row; a run that was not linked makes the next run's carried pairs
 * VIS_SL_NO_DEPTH.  Asynchronous on the POSE stream behind vis_batch_triangulate of the same run; the caller's buffers are in use until
 * vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: sp as above, a NULL or misaligned d_points (16), d_flags or d_link (8), n or row_cap negative.
 * VIS_E_CAPACITY: row_cap below the plan's correspondences per pair.  VIS_E_STATE: no context / plan / pose stage, or n differs. */
int  vis_batch_scale_links(vis_ctx* ctx, const vis_scale_link_params* sp, int n, const vis_map_point* d_points, const uint8_t* d_flags, int row_cap,
                           vis_scale_link* d_link);

/* 2. THE CHAIN.  Frame i is NOT SAVED when prev[i] == VIS_KF_NOT_SAVED: the zero record with VIS_TJ_NOT_SAVED.  It HAS A PARENT when prev[i] is an
 * index q of a frame that is not NOT SAVED, or VIS_KF_CARRIED with a carried record (d_carry_in not NULL and its flags without VIS_TJ_NOT_SAVED and
 * VIS_TJ_OVERFLOW).  A saved frame with a parent and a usable pose record has an EDGE x_i = R_i x_q + sigma_i t_i, sigma_i = sigma_q s_i; every
 * other saved frame is a ROOT: identity pose, sigma = 1, the start of a segment (flags VIS_TJ_ROOT, with VIS_TJ_NO_POSE when it has a parent but no
 * usable pose, VIS_TJ_NO_CARRY when prev[i] == VIS_KF_CARRIED without a carried record).  s_i = d_link[i].scale when d_link[i].flags == VIS_SL_OK,
 * the scale is finite and > 0 and the parent is not a root (a root of this call, or a carried record with VIS_TJ_ROOT); else s_i = 1 and the edge is a UNIT edge (VIS_TJ_UNIT_EDGE): a gauge edge
 * -- the first edge below a root always is one, its parent has no pair and so no depth row -- or a held scale.
 * vis_traj_pose: R, t with x_i = R X + t, X in the root's frame (the layout d_poses of the N-view triangulation reads); sigma; segment_seq = the
 * root's stream number (frame i of a call is seq0 + i); epoch_seq = the stream number of the frame of the LAST unit edge on the way from the root
 * to i, for a root its own; hops = edges from the root; unit_edges = unit edges among them (1 = scaled throughout); parent = prev[i] normalised;
 * flags.  Through the carried record the segment is inherited, hops and unit_edges add, and epoch_seq is the carried one when the path inside the
 * call has no unit edge.  When any of R, t, sigma would not be finite, or sigma would not be > 0, the record is zero with VIS_TJ_OVERFLOW: no NaN
 * ever reaches a record.  Orthonormality of R is not repaired (DESIGN.md 4.19 has the measured deviation).
 * COMPOSITION, division-free.  The state (S, R, U) of a path i -> a means x_i = R x_a + sigma_a U and sigma_i = sigma_a S; an edge is
 * (s_i, R_i, s_i t_i) (each s_i * t_i[r]); path i -> m (S1, R1, U1) followed by m -> a (S2, R2, U2) is S = S1 S2,
 * R[3r + c] = (R1[3r] R2[c] + R1[3r + 1] R2[3 + c]) + R1[3r + 2] R2[6 + c], U[r] = (((R1[3r] U2[0] + R1[3r + 1] U2[1]) + R1[3r + 2] U2[2]) + S2 U1[r]);
 * hops and unit_edges add; the epoch is the first path's when that has a unit edge, else the second's.  At a root the record is (R, U, S).  At the
 * carried record (Rc, tc, sigma_c): R Rc by the product above, t[r] = (((R[3r] tc[0] + R[3r + 1] tc[1]) + R[3r + 2] tc[2]) + sigma_c U[r]),
 * sigma = sigma_c S.  The frames are chained by pointer doubling: ceil(log2 n) rounds (reach = 1, 2, 4 ... < n), in each of which every frame whose
 * ancestor is neither itself nor final replaces its state by the composition with its ancestor's state OF THE ROUND BEFORE -- so the rounding of
 * a record depends on the frame's position in its call, and two cuts of a stream agree within a bound, not byte for byte.
 * On the device all rounds run inside ONE launch of one workgroup: every thread keeps up to four frames' states in registers, reads the ancestor's,
 * and workgroup barriers separate reading from writing; the states live in LDS up to 256 frames and in the workspace beyond.  No loop over frames
 * depends on data.
 * d_poses (may be NULL): n x 12 doubles, R then t, of the frames whose epoch_seq (same_epoch_only != 0) or segment_seq (== 0) equals that of the
 * NEWEST frame with a pose (the largest i whose record is neither NOT_SAVED nor OVERFLOW); every other frame gets a zero row = "no pose", which
 * vis_batch_ftrack_triangulate skips.  Within one epoch all relative poses share one scale, so no track is triangulated across a held scale. */
enum { VIS_TJ_ROOT = 1, VIS_TJ_NO_POSE = 2, VIS_TJ_NO_CARRY = 4, VIS_TJ_NOT_SAVED = 8, VIS_TJ_UNIT_EDGE = 16, VIS_TJ_OVERFLOW = 32 };
enum { VIS_TJ_MAX_FRAMES = 1024 };
typedef struct vis_traj_pose {           /* 128 bytes */
    double  R[9], t[3], sigma;
    int32_t segment_seq, epoch_seq, hops, unit_edges, parent, flags;
} vis_traj_pose;
/* Caller-made rows, DEVICE pointers, asynchronous on the context's stream.  d_prev, d_pose, d_link, d_traj: n entries; d_carry_in: NULL or ONE record,
 * that of the frame VIS_KF_CARRIED refers to.  The workspace (120 bytes per frame, only when n > 256) belongs to the context and only grows; a
 * call that grows it SYNCHRONISES.
 * Refusals, in this order.  VIS_E_INVALID: a NULL d_prev, d_pose, d_link or d_traj, a pointer that is not aligned (8 bytes for d_pose, d_link,
 * d_carry_in, d_traj and d_poses, 4 for d_prev), n or seq0 negative.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_TJ_MAX_FRAMES. */
int  vis_trajectory_rows(vis_ctx* ctx, int n, const int32_t* d_prev, const vis_pose_result* d_pose, const vis_scale_link* d_link,
                         const vis_traj_pose* d_carry_in, int seq0, int same_epoch_only, vis_traj_pose* d_traj, double* d_poses);
/* The frames of the last vis_batch_run (with VIS_STAGE_POSE; n = its frames) with the pose stage's records, vis_batch_get_keyframes' pairing and
 * the links vis_batch_scale_links wrote for that run (d_link), on the POSE stream behind it; seq is the plan's frame counter, the one the feature
 * tracks use.  The plan carries the record of the last SAVED frame across launches, two records used in turn under the rules of the depth row
 * above (a run that was not chained makes the next run's carried pairs roots with VIS_TJ_NO_CARRY).  The caller's buffers are in use until
 * vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: a NULL or misaligned d_link, d_traj or d_poses (8; d_poses may be NULL), n negative.  VIS_E_STATE: no
 * context / plan / pose stage, or n differs.  VIS_E_CAPACITY: n > VIS_TJ_MAX_FRAMES. */
int  vis_batch_trajectory(vis_ctx* ctx, int n, const vis_scale_link* d_link, int same_epoch_only, vis_traj_pose* d_traj, double* d_poses);
/* The record the NEXT run's vis_batch_trajectory continues from where a frame's pair is the carried keyframe (rec NULL: none).  HOST pointer;
 * SYNCHRONISES, like vis_batch_track_init.  VIS_E_STATE without a context or plan. */
int  vis_batch_trajectory_init(vis_ctx* ctx, const vis_traj_pose* rec);
/* Out of scope: bundle adjustment, loop closure, feeding the trajectory into vis_batch_track or vis_batch_pnp (the metric scale is
 * vis_batch_vi_align's, which reads these records and changes none), and a scale between
 * siblings of one root in tree-shaped caller rows (each sibling is its own unit edge; the plan's pairing is a chain and never makes them). */

/* ---- IMU preintegration: the rotation of every pair (the d_rot of vis_batch_f2f, vis_batch_filter_keypoints, vis_batch_run_guided and the hint of
 * vis_batch_homography_pose) and the pair's motion deltas, on the device, with the plan's own pairing.  The reference computes the same quantity,
 * RotationResCam = imu2camRotation^T R(t_keyframe)^T R(t_frame) imu2camRotation, from the orientation of an external filter node; here standard
 * preintegration (Lupton & Sukkarieh 2012; Forster et al. 2017, restated from the papers) takes the filter's place.  tests/imu_ref.py restates every
 * operation below, and every record equals the restatement byte for byte: double arithmetic, + - * / and comparisons only (no sin, cos, sqrt),
 * nothing contracted.  "finite(x)" is |x| <= DBL_MAX.
 * PRODUCTS, summed left to right as in the trajectory's composition: (A B)[3r + c] = (A[3r] B[c] + A[3r + 1] B[3 + c]) + A[3r + 2] B[6 + c];
 * (A^T B)[3r + c] = (A[r] B[c] + A[3 + r] B[3 + c]) + A[6 + r] B[6 + c]; (A x)[r] = (A[3r] x[0] + A[3r + 1] x[1]) + A[3r + 2] x[2].
 * SAMPLES: t in seconds, rising; w in rad/s and a in m/s^2 in the IMU frame.  ub(x) = the first sample index with t > x and lb(x) = the first
 * with t >= x, by binary search (lo = 0, hi = n_samples; mid = (lo + hi) >> 1; `t[mid] <= x` resp. `t[mid] < x` moves lo to mid + 1, else hi to mid),
 * so a launch's sample array may overlap the one before.
 * 1. INTERVALS.  Interval i is (ta, tb] = (t_{i-1}, t_i] of d_tframe, t_{-1} = the carry's t_last.  Its delta starts as the identity (R = I, v = p = 0,
 * JRg = 0, n_steps = 0, flags = 0) with dt = tb - ta (0 when that is not finite).  Interval 0 without a carried time: VIS_IMU_NO_START, dt = 0,
 * nothing more.  ta or tb not finite: VIS_IMU_NONFINITE.  n_samples == 0: VIS_IMU_EMPTY | VIS_IMU_EXTRAPOLATED.  Else the VALUE at a breakpoint x
 * (ta, then tb), with j = ub(x): j == 0 holds sample 0 and j == n_samples holds the last sample, each VIS_IMU_EXTRAPOLATED unless that sample's t
 * equals x; otherwise u = (x - t[j-1]) / (t[j] - t[j-1]) and every component is s[j-1] + u (s[j] - s[j-1]).  The samples strictly inside are
 * [ub(ta), lb(tb)); none: VIS_IMU_EMPTY.  Every sample so used (held, bracketing or inside) must have finite t, w and a, else VIS_IMU_NONFINITE and
 * no sub-step is taken.  The sub-steps run from (ta, value) over the inside samples to (tb, value); one from (t0, w0, a0) to (t1, w1, a1):
 *   h = t1 - t0; not h > 0: VIS_IMU_ORDER, skipped.  Else n_steps += 1; h > max_gap_s: VIS_IMU_GAP;
 *   phi[k] = (0.5 (w0[k] + w1[k]) - bg[k]) h; xx = phi0 phi0, yy, zz, xy = phi0 phi1, xz, yz alike; th2 = (xx + yy) + zz;
 *   th2 > max_angle max_angle: VIS_IMU_FAST;
 *   A, B, C = the Horner sums c[0] + th2 (c[1] + th2 (... + th2 c[9])) of VIS_IMU_COEF_A / _B / _C: sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3;
 *   dR = Exp(phi) = { 1 - B (yy + zz), B xy - A phi2, B xz + A phi1;  B xy + A phi2, 1 - B (xx + zz), B yz - A phi0;  B xz - A phi1, B yz + A phi0, 1 - B (xx + yy) };
 *   Jr(phi)       = { 1 - C (yy + zz), C xy + B phi2, C xz - B phi1;  C xy - B phi2, 1 - C (xx + zz), C yz + B phi0;  C xz + B phi1, C yz - B phi0, 1 - C (xx + yy) };
 *   R' = R dR; am[r] = 0.5 ((R (a0 - ba))[r] + (R' (a1 - ba))[r]); p[r] = p[r] + (v[r] h + (0.5 am[r]) (h h)); then v[r] = v[r] + am[r] h;
 *   JRg[k] = (dR^T JRg)[k] - Jr[k] h; R = R'.
 * Ten terms: the first dropped term bounds the truncation, th^20 / 21! (A), / 22! (B), / 23! (C) -- 2e-20 at th = 1, below half an ulp of the sums,
 * and 2.1e-14 at th = 2.  max_angle defaults to 1; a sub-step beyond it is integrated all the same and says so (VIS_IMU_FAST).  The scheme is the
 * midpoint rule, second order in the sample period.  At the end any number of the delta that is not finite, or VIS_IMU_NONFINITE from above, gives
 * the identity again with dt, n_steps and the flags kept and VIS_IMU_NONFINITE set: no NaN or infinity reaches a record.
 * 2. PAIRS.  prev[i] as for vis_trajectory_rows.  The pair of frame i with keyframe q = prev[i] is the COMPOSITION of the intervals q + 1 ... i -- by
 * definition; a direct integration over (t_q, t_i] differs at the discretisation level, because a frame time inside a sample gap adds a breakpoint
 * (DESIGN.md 4.20).  X o Y (X earlier) = (R1 R2, v1[r] + (R1 v2)[r], (p1[r] + v1[r] dt2) + (R1 p2)[r], dt1 + dt2, (R2^T JRg1)[k] + JRg2[k]), n_steps added, flags
 * OR-ed; a composition with a number that is not finite is the identity with dt (0 when not finite), n_steps, flags kept and VIS_IMU_NONFINITE.
 * TABLE: T_0[i] = interval i, T_k[i] = T_{k-1}[i - 2^{k-1}] o T_{k-1}[i] for i >= 2^k - 1.  A pair of L = i - q intervals takes the set bits k of L
 * in rising order from pos = i: the first gives acc = T_k[pos], every later one acc = T_k[pos] o acc, and pos -= 2^k after each.  So a record depends
 * on its own intervals alone, not on the frame's place in the call, and with the gate off a stream's records are the same bytes however it is cut.
 * prev[i] == VIS_KF_CARRIED: L = i + 1 (intervals 0 ... i) and, when the carry has VIS_IMU_CARRY_OPEN, record = carry.open o acc.  Without a carry
 * (NULL, or without VIS_IMU_CARRY_TIME): the identity, dt = 0, VIS_IMU_NO_CARRY.  VIS_KF_NOT_SAVED / VIS_KF_FIRST: the identity, dt = 0, VIS_IMU_NO_PAIR.
 * q = prev[i] normalised.  CARRY OUT: t_last = t_{n-1}; with `last` the largest i that is not VIS_KF_NOT_SAVED, open = the L = n - 1 - last intervals
 * last + 1 ... n - 1 (L = 0: the identity, dt = 0, and no VIS_IMU_CARRY_OPEN); when no frame was saved, L = n and open = carry.open o acc where the
 * carry has VIS_IMU_CARRY_OPEN.  valid = VIS_IMU_CARRY_TIME, with VIS_IMU_CARRY_OPEN when open spans an interval.
 * d_rot[9 i] = (float)(r_ic^T R r_ic): (r_ic^T R) first, then times r_ic, in double, each entry narrowed once -- "current-frame rays -> previous
 * frame", RotationResCam.  The identity for a frame flagged VIS_IMU_NO_PAIR, VIS_IMU_NO_CARRY or VIS_IMU_NONFINITE, or when an entry exceeds FLT_MAX.
 * On the device: k_imu_intervals, one lane per interval, a serial loop over its sub-steps; k_imu_pairs, ONE launch of one workgroup that builds
 * every level (workgroup barriers between them; levels above the call's longest pair are not built, which no result depends on), composes the
 * pairs and writes d_delta, d_rot and the carry.  No loop's length depends on the gate's decisions. */
enum { VIS_IMU_OK = 0, VIS_IMU_NO_PAIR = 1, VIS_IMU_NO_CARRY = 2, VIS_IMU_NO_START = 4, VIS_IMU_EMPTY = 8, VIS_IMU_EXTRAPOLATED = 16, VIS_IMU_GAP = 32,
       VIS_IMU_FAST = 64, VIS_IMU_ORDER = 128, VIS_IMU_NONFINITE = 256 };
enum { VIS_IMU_CARRY_TIME = 1, VIS_IMU_CARRY_OPEN = 2 };
enum { VIS_IMU_MAX_FRAMES = 1024, VIS_IMU_EXP_TERMS = 10 };
/* (-1)^k / (2k + 1)!, / (2k + 2)!, / (2k + 3)!, k = 0 ... 9, each the double nearest to the quotient */
#define VIS_IMU_COEF_A { 1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15, -8.22063524662433e-18 }
#define VIS_IMU_COEF_B { 0.5, -0.041666666666666664, 0.001388888888888889, -2.48015873015873e-05, 2.755731922398589e-07, -2.08767569878681e-09, 1.1470745597729725e-11, -4.779477332387385e-14, 1.5619206968586225e-16, -4.110317623312165e-19 }
#define VIS_IMU_COEF_C { 0.16666666666666666, -0.008333333333333333, 0.0001984126984126984, -2.7557319223985893e-06, 2.505210838544172e-08, -1.6059043836821613e-10, 7.647163731819816e-13, -2.8114572543455206e-15, 8.22063524662433e-18, -1.9572941063391263e-20 }
typedef struct vis_imu_sample { double t, w[3], a[3]; } vis_imu_sample;                                                  /* 56 bytes */
typedef struct vis_imu_params {          /* 136 bytes; every field finite */
    double bg[3], ba[3];                 /* 0             the biases subtracted from w and a */
    double r_ic[9];                      /* identity      the reference's imu2camRotation, row-major */
    double max_gap_s;                    /* 0.05          a sub-step longer than this flags the interval VIS_IMU_GAP; > 0 */
    double max_angle;                    /* 1.0           a sub-step turning further (rad) flags it VIS_IMU_FAST; > 0 */
} vis_imu_params;
/* R: vectors of the IMU frame at the later time -> the IMU frame at the earlier time (R_q^T R_i); v, p: the preintegrated velocity and position
 * increments in the earlier frame, gravity NOT subtracted; dt; JRg = d(log R) / d(bg); n_steps = sub-steps taken; q = prev[i] normalised */
typedef struct vis_imu_delta { double R[9], v[3], p[3], dt, JRg[9]; int32_t n_steps, flags, q, reserved_; } vis_imu_delta;   /* 216 bytes */
/* t_last: the time of the last frame of the call before; open: the delta from the last SAVED frame to t_last; valid: VIS_IMU_CARRY_* */
typedef struct vis_imu_carry { double t_last; vis_imu_delta open; int32_t valid, reserved_; } vis_imu_carry;             /* 232 bytes */
void vis_default_imu_params(vis_imu_params* ip);
/* ONE interval (t_a, t_b], HOST pointers, blocks once: row 0 of vis_imu_preintegrate_rows for one frame at t_b whose pair is VIS_KF_CARRIED and whose
 * carry holds t_a alone.  rot (9 floats) may be NULL.
 * Refusals, in this order.  VIS_E_INVALID: ip NULL or out of range (a field not finite, a bound not > 0), delta NULL, n_samples negative, samples
 * NULL with n_samples > 0.  VIS_E_STATE without a context. */
int  vis_imu_preintegrate(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_sample* samples, int n_samples, double t_a, double t_b,
                          vis_imu_delta* delta, float* rot);
/* Caller rows, DEVICE pointers, asynchronous on the context's stream.  d_samples: n_samples records; d_tframe, d_prev, d_delta: n entries; d_rot: NULL or
 * n x 9 floats; d_carry_in: NULL or one record; d_carry_out: NULL or one record (it may not be d_carry_in).  Every entry of d_delta (and d_rot) is
 * written.  The workspace (208 bytes x frames x levels, levels = the bits of n: 25 doubles and the two integers of a table entry) belongs to the
 * context and only grows; a call that grows it SYNCHRONISES.
 * GUIDED MATCHING.  vis_batch_run_guided reads d_rot before the gate of its own run has paired the frames.  With the gate OFF the pairing is known
 * beforehand -- prev[i] = i - 1, frame 0 VIS_KF_CARRIED (VIS_KF_FIRST for the first launch of a stream) -- so this call with such a d_prev, queued on the
 * context's stream ahead of vis_batch_run_guided, feeds it with no host step; pass each call's d_carry_out as the next call's d_carry_in (two
 * records in turn).  With the gate ON a guided run driven by the IMU needs the integration between the gate and the matcher inside the run: out of scope.
 * Refusals, in this order.  VIS_E_INVALID: ip as above; a NULL d_tframe, d_prev or d_delta; d_samples NULL with n_samples > 0; a pointer that is not
 * aligned (8 bytes for d_samples, d_tframe, d_carry_in, d_delta, d_carry_out; 4 for d_prev and d_rot); n or n_samples negative; d_carry_out equal to
 * d_carry_in and not NULL.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_IMU_MAX_FRAMES. */
int  vis_imu_preintegrate_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                               const int32_t* d_prev, const vis_imu_carry* d_carry_in, vis_imu_delta* d_delta, float* d_rot, vis_imu_carry* d_carry_out);
/* The frames of the last vis_batch_run (with VIS_STAGE_MATCH; n = its frames) with vis_batch_get_keyframes' pairing, on the POSE stream through the
 * scaffold every follow-up uses: it FORKS from the context's stream, so d_samples and d_tframe may be produced there, and vis_batch_f2f,
 * vis_batch_filter_keypoints and vis_batch_homography_pose queued after it read its d_rot with no host step.  The plan keeps TWO carry records and
 * uses them in turn under the rules of the depth row of vis_batch_scale_links: a repeated call reads the record the run was given; vis_batch_plan /
 * vis_batch_reset forget it; a run that was not integrated makes the next run's carried pairs VIS_IMU_NO_CARRY.  The caller's buffers are in use until
 * vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: ip as above; a NULL d_tframe or d_delta; d_samples NULL with n_samples > 0; a misaligned pointer (8; d_rot 4);
 * n or n_samples negative.  VIS_E_STATE: no context / plan / match stage, or n differs.  VIS_E_CAPACITY: n > VIS_IMU_MAX_FRAMES. */
int  vis_batch_imu(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                   vis_imu_delta* d_delta, float* d_rot);
/* The carry the NEXT run's vis_batch_imu continues from (rec NULL: none).  HOST pointer; SYNCHRONISES, like vis_batch_trajectory_init.
 * VIS_E_STATE without a context or plan. */
int  vis_batch_imu_init(vis_ctx* ctx, const vis_imu_carry* rec);
/* Out of scope: a guided run with the gate on, and the adapters' IMU arguments (still accepted and ignored).  (The bias Jacobians of v and p and the
 * 9 x 9 covariance are the blocks below; the gyro bias, gravity, the metric scale and the lever arm are vis_vi_align_rows / vis_batch_vi_align.) */

/* ---- Bias Jacobians of the deltas and the first-order bias correction.  The three calls below are vis_imu_preintegrate, vis_imu_preintegrate_rows
 * and vis_batch_imu with one more output row, d_jac: Jvg = dv / dbg, Jva = dv / dba, Jpg = dp / dbg, Jpa = dp / dba (3 x 3 row-major), the derivatives
 * of the SCHEME above (midpoint rule, ten-term Exp), which is what a finite difference of tests/imu_ref.py measures.  d_delta, d_rot and the carried
 * delta are the sibling's BYTE FOR BYTE on every input: the delta's operations are the same ones in the same order, and a Jacobian never changes a
 * delta.  tests/imu_jac_ref.py restates every operation below; every record equals it byte for byte.  Double arithmetic, + - * / only, nothing
 * contracted.  ([u]x M)[c] = u[1] M[6 + c] - u[2] M[3 + c], [3 + c] = u[2] M[c] - u[0] M[6 + c], [6 + c] = u[0] M[3 + c] - u[1] M[c], c = 0, 1, 2.
 * SUB-STEP, with R, J = JRg before it, R', J' after it, u0 = a0 - ba, u1 = a1 - ba, all from the sub-step above, and k = 0 ... 8:
 *   G0 = R ([u0]x J), G1 = R' ([u1]x J') (products as above); Dg[k] = -0.5 (G0[k] + G1[k]); Da[k] = -0.5 (R[k] + R'[k]);
 *   Jpg[k] = Jpg[k] + (Jvg[k] h + (0.5 Dg[k]) (h h)); then Jvg[k] = Jvg[k] + Dg[k] h; Jpa, Jva alike with Da (the p lines use the old v Jacobians).
 * An interval starts with zero Jacobians and flags 0.  SETTLE, the rule every Jacobian record ends on, with the flags of ITS delta: zero matrices when
 * the delta's flags have any of VIS_IMU_NO_PAIR | NO_CARRY | NO_START | NONFINITE (a voided delta has zero Jacobians) or the record's flags already
 * have VIS_IMU_JAC_NONFINITE; else, when one of the 36 numbers is not finite: VIS_IMU_JAC_NONFINITE and zero matrices.  The flag is sticky: flags are
 * OR-ed through compositions.  No NaN or infinity reaches a record or a carry.  An interval settles after the delta's own finite() rule.
 * COMPOSITION X o Y (X earlier), after the delta's O = X o Y, with Wv = X.R ([Y.v]x X.JRg), Wp = X.R ([Y.p]x X.JRg):
 *   Jpa[k] = (X.Jpa[k] + X.Jva[k] Y.dt) + (X.R Y.Jpa)[k];                 Jva[k] = X.Jva[k] + (X.R Y.Jva)[k];
 *   Jpg[k] = ((X.Jpg[k] + X.Jvg[k] Y.dt) + (X.R Y.Jpg)[k]) - Wp[k];       Jvg[k] = (X.Jvg[k] + (X.R Y.Jvg)[k]) - Wv[k];
 * flags = X.flags | Y.flags; then SETTLE with O's flags.  TABLE, PAIRS and CARRY are the delta's, entry for entry: the same levels, the same set
 * bits, the carried open delta composed in front where the delta's is; so with the gate off a stream's Jacobians are the same bytes however it is
 * cut, and with the gate on two cuts agree within a bound.  A frame without a pair has zero Jacobians and flags 0.  q = the delta's q
 * (0 in a carry).  The table is a separate one of 496 bytes x frames x levels (62 slots: the 26 of vis_imu_preintegrate_rows, then the four blocks);
 * vis_imu_preintegrate_rows, vis_batch_imu and vis_imu_preintegrate keep their table, their kernels' work and their results.
 * On the device: k_imu_intervals<true> and k_imu_pairs<true>, the launches of the siblings; a composition folds one block at a time. */
enum { VIS_IMU_JAC_OK = 0, VIS_IMU_JAC_NONFINITE = 1 };
typedef struct vis_imu_bias_jac { double Jvg[9], Jva[9], Jpg[9], Jpa[9]; int32_t flags, q; } vis_imu_bias_jac;           /* 296 bytes */
/* vis_imu_carry and the Jacobians of its open delta */
typedef struct vis_imu_jac_carry { vis_imu_carry carry; vis_imu_bias_jac open_jac; } vis_imu_jac_carry;                   /* 528 bytes */
/* vis_imu_preintegrate with the Jacobians of the interval.  Refusals in its order, jac NULL beside delta NULL. */
int  vis_imu_preintegrate_jac(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_sample* samples, int n_samples, double t_a, double t_b,
                              vis_imu_delta* delta, vis_imu_bias_jac* jac, float* rot);
/* vis_imu_preintegrate_rows with d_jac (n records, 8-byte aligned, not NULL) and carries that hold the open delta's Jacobians.  The workspace is a
 * block of the context's own, apart from vis_imu_preintegrate_rows', under the same rule: it only grows, and a call that grows it SYNCHRONISES.
 * Refusals in the sibling's order and codes, d_jac beside d_delta. */
int  vis_imu_preintegrate_jac_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                                   const int32_t* d_prev, const vis_imu_jac_carry* d_carry_in, vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac, float* d_rot,
                                   vis_imu_jac_carry* d_carry_out);
/* vis_batch_imu with d_jac, on the POSE stream through the follow-up scaffold, with TWO carried vis_imu_jac_carry records of its own under the same
 * turn rule -- apart from vis_batch_imu's, so that either may be called for a run, or both.  Refusals in vis_batch_imu's order and codes. */
int  vis_batch_imu_jac(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                       vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac, float* d_rot);
/* The carry the NEXT run's vis_batch_imu_jac continues from (rec NULL: none).  HOST pointer; SYNCHRONISES.  VIS_E_STATE without a context or plan. */
int  vis_batch_imu_jac_init(vis_ctx* ctx, const vis_imu_jac_carry* rec);
/* THE CORRECTION: the records of a bias step (dbg, dba) to first order, with no second pass over the samples.  d_dbg: THREE doubles on the device --
 * the first 24 bytes of a vis_vi_align record are its dbg, so the alignment's result is passed as it is, with no host step; d_dba: three doubles or
 * NULL for (0, 0, 0).  Of ip, r_ic and max_angle are used.  Per frame, with (R, v, p, JRg) of d_delta[i] and the blocks of d_jac[i], in this order:
 *   flags with any of VIS_IMU_NO_PAIR | NO_CARRY | NO_START | NONFINITE, or one of the delta's 25 numbers not finite: VIS_IMC_UNUSABLE;
 *   d_jac[i].flags has VIS_IMU_JAC_NONFINITE: VIS_IMC_JAC;  one of the six bias numbers not finite: VIS_IMC_BIAS;
 *   phi = JRg dbg, xx ... th2 as in the sub-step; th2 > max_angle max_angle: VIS_IMC_ANGLE;
 *   R' = R Exp(phi) (A, B by the ten-term sums, dR as in the sub-step); v'[r] = v[r] + ((Jvg dbg)[r] + (Jva dba)[r]); p'[r] = p[r] + ((Jpg dbg)[r] +
 *   (Jpa dba)[r]); one of the 15 numbers not finite: VIS_IMC_NONFINITE; else VIS_IMC_OK.
 * VIS_IMC_OK writes the record with R', v', p' in the place of R, v, p and dt, JRg, n_steps, flags, q, reserved_ kept; every other status copies the
 * record unchanged.  d_status[i] (NULL or n int32) = the status.  d_rot_out (NULL or n x 9 floats) = d_rot's rule on the record written.  The
 * Jacobians are those of the OLD biases: after the step they are first-order stale, like JRg.  d_delta_out may not alias d_delta.  k_imu_correct, one
 * lane per frame, asynchronous on the context's stream, no workspace.
 * Refusals, in this order.  VIS_E_INVALID: ip as above; a NULL d_delta, d_jac, d_dbg or d_delta_out; a pointer that is not aligned (8 bytes; d_rot_out
 * and d_status 4); n negative; d_delta_out equal to d_delta.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_IMU_MAX_FRAMES. */
enum { VIS_IMC_OK = 0, VIS_IMC_UNUSABLE = 1, VIS_IMC_JAC = 2, VIS_IMC_BIAS = 4, VIS_IMC_ANGLE = 8, VIS_IMC_NONFINITE = 16 };
int  vis_imu_correct_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                          const double* d_dba, vis_imu_delta* d_delta_out, float* d_rot_out, int32_t* d_status);
/* The same for the frames of the last vis_batch_run, on the POSE stream through the follow-up scaffold: queued behind vis_batch_vi_align, it reads
 * that call's d_result as d_dbg, and a second vis_batch_vi_align queued behind it reads d_delta_out -- align, correct, align again with no host step.
 * (The second alignment of a run is a repeated call: it reads the carry the first one read.)  The caller's buffers are in use until vis_batch_sync.
 * Behind vis_batch_vi_align_ba, d_dbg = d_result and d_dba = &d_result->dba (byte 160 of that record) pass both estimated steps the same way.
 * Refusals as above; VIS_E_STATE: no context / plan / match stage, or n differs. */
int  vis_batch_imu_correct(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                           const double* d_dba, vis_imu_delta* d_delta_out, float* d_rot_out, int32_t* d_status);
/* Out of scope: the host adapters' IMU arguments, a guided run with the gate on.  (The accelerometer-bias estimate that reads Jva and Jpa is
 * vis_batch_vi_align_ba; the covariance is the block below.) */

/* ---- THE COVARIANCE of a delta.  The three calls below are vis_imu_preintegrate, vis_imu_preintegrate_rows and vis_batch_imu with one more output
 * row, d_cov: the 9 x 9 covariance of the error (dphi, dv, dp) of the delta, the error defined by R Exp(dphi), v + dv, p + dp, driven by white gyro and
 * accelerometer noise of the densities of vis_imu_noise (Forster et al. 2017, restated from the equations for THIS scheme: the linear map is the one
 * the bias Jacobians above follow, driven by noise in the place of a constant bias).  The bias Jacobians are NOT computed by these calls (a caller
 * who wants both queues both; k_imu_pairs<true> has no registers to spare).  d_delta, d_rot and the carried delta are the sibling's BYTE FOR BYTE on
 * every input.  tests/imu_cov_ref.py restates every operation below; every record equals it byte for byte.  Double arithmetic, + - * / only, nothing
 * contracted; products (A B), (A^T B), (A x) as in the IMU block, and (A B^T)[3r + c] = (A[3r] B[3c] + A[3r + 1] B[3c + 1]) + A[3r + 2] B[3c + 2];
 * (M [u]x)[3r] = M[3r + 1] u[2] - M[3r + 2] u[1], [3r + 1] = M[3r + 2] u[0] - M[3r] u[2], [3r + 2] = M[3r] u[1] - M[3r + 1] u[0].
 * BLOCKS.  S is kept as six 3 x 3 blocks, named by (row, column): A = phi-phi, B = v-phi, C = v-v, D = p-phi, E = p-v, F = p-p.  A, C and F are computed
 * as their UPPER TRIANGLES only (entries 00 01 02 11 12 22; where a product below reads one of them in full, the lower entries are copies), so the
 * matrix is symmetric by construction.  vis_imu_cov.S is the upper triangle of the 9 x 9 in row order, entry (r, c), r <= c, at r 9 - r (r - 1) / 2 +
 * (c - r): rows 0 - 2 hold A's triangle, B^T and D^T, rows 3 - 5 C's triangle and E^T, rows 6 - 8 F's triangle.
 * PROPAGATION by F = [a 0 0; b I 0; c t I] (3 x 3 blocks; a = M^T for a given M), P(X; M, b, c, t) = F X F^T, block by block and in this order:
 *   A'  = M^T (X.A M);                                       U = (b X.A) + X.B;         B' = U M;
 *   C'  = (U b^T) + ((b X.B^T) + X.C);                       V = ((c X.A) + t X.B) + X.D;   D' = V M;
 *   Y   = ((c X.B^T) + t X.C) + X.E;                         E' = (V b^T) + Y;
 *   Z   = ((c X.D^T) + t X.E^T) + X.F;                       F' = ((V c^T) + t Y) + Z;            (each line entry by entry; t X.B is t times the entry)
 * SUB-STEP, with R, dR, Jr, R', u0, u1, h of the sub-step above, hh = 0.5 h, qg = (sigma_g sigma_g) / h, qa = (sigma_a sigma_a) / h -- a sub-step is ONE
 * measurement of the mean rate and the mean specific force, each with independent noise of covariance (sigma^2 / h) I:
 *   S1 = R' [u1]x;  W = (R [u0]x) + (S1 dR^T);  b[k] = -(hh W[k]);  c[k] = hh b[k];  K1[k] = Jr[k] h;  K2[k] = -(hh (S1 K1)[k]);  K3[k] = (R[k] + R'[k]) hh;
 *   N.A = qg (K1 K1^T);  N.B = qg (K2 K1^T);  N.C = qg (K2 K2^T) + qa (K3 K3^T);  N.D = hh N.B;  N.E = hh N.C;  N.F = hh N.E  (entry by entry);
 *   S = P(S; dR, b, c, h) + N  (each entry: the propagated term first).
 * That is F S F^T + G diag(qg I, qa I) G^T with F = [dR^T 0 0; -h/2 W I 0; -h^2/4 W h I I] and G = [Jr h 0; -h/2 R' [u1]x Jr h, (R + R') h/2; h/2 times
 * that row].  An interval starts with S = 0 and flags 0.
 * COMPOSITION X o Y (X earlier), after the delta's O = X o Y:  b[k] = -(X.R [Y.v]x)[k];  c[k] = -(X.R [Y.p]x)[k];
 *   G-term: A = Y.A;  B = X.R Y.B;  C = (X.R Y.C) X.R^T;  D = X.R Y.D;  E = (X.R Y.E) X.R^T;  F = (X.R Y.F) X.R^T;
 *   S = P(X.S; Y.R, b, c, Y.dt) + G-term  (each entry: the propagated term first);  flags = X.flags | Y.flags; then SETTLE with O's flags.
 * SETTLE is the Jacobians' rule with VIS_IMU_COV_NONFINITE and the 45 numbers: S = 0 beside a voided delta or in a flagged record; else a number that
 * is not finite zeroes S and sets the flag, which is sticky.  No NaN or infinity reaches a record or a carry.  TABLE, PAIRS and CARRY are the delta's,
 * entry for entry; so with the gate off a stream's covariances are the same bytes however it is cut, and with the gate on two cuts agree within a
 * bound.  A frame without a pair has S = 0 and flags 0.  q = the delta's q (0 in a carry).  The table is a separate one of 568 bytes x
 * frames x levels (71 slots: the 26 of vis_imu_preintegrate_rows, then A's six, B, C's six, D, E, F's six).
 * On the device: k_imu_cov_intervals and k_imu_cov_pairs, the launches of the siblings and their bodies; a composition folds one block at a time.
 * Out of scope: bias random-walk states (a 15 x 15 covariance), the covariance of the bias-corrected records of vis_imu_correct_rows. */
enum { VIS_IMU_COV_OK = 0, VIS_IMU_COV_NONFINITE = 1 };
typedef struct vis_imu_noise {           /* 16 bytes; both finite and >= 0 */
    double sigma_g;                      /* 1.6968e-4     gyro noise density, rad/s/sqrt(Hz) (EuRoC's ADIS16448) */
    double sigma_a;                      /* 2.0e-3        accelerometer noise density, m/s^2/sqrt(Hz) */
} vis_imu_noise;
typedef struct vis_imu_cov { double S[45]; int32_t flags, q; } vis_imu_cov;                                              /* 368 bytes */
/* vis_imu_carry and the covariance of its open delta */
typedef struct vis_imu_cov_carry { vis_imu_carry carry; vis_imu_cov open_cov; } vis_imu_cov_carry;                       /* 600 bytes */
void vis_default_imu_noise(vis_imu_noise* np);
/* vis_imu_preintegrate with the covariance of the interval.  Refusals in its order: np NULL or out of range directly after ip, cov NULL beside delta NULL. */
int  vis_imu_preintegrate_cov(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, const vis_imu_sample* samples, int n_samples, double t_a,
                              double t_b, vis_imu_delta* delta, vis_imu_cov* cov, float* rot);
/* vis_imu_preintegrate_rows with d_cov (n records, 8-byte aligned, not NULL) and carries that hold the open delta's covariance.  The workspace is a
 * block of the context's own, apart from the siblings', under the same rule: it only grows, and a call that grows it SYNCHRONISES.
 * Refusals in the sibling's order and codes, np directly after ip, d_cov beside d_delta. */
int  vis_imu_preintegrate_cov_rows(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, const vis_imu_sample* d_samples, int n_samples,
                                   const double* d_tframe, const int32_t* d_prev, const vis_imu_cov_carry* d_carry_in, vis_imu_delta* d_delta,
                                   vis_imu_cov* d_cov, float* d_rot, vis_imu_cov_carry* d_carry_out);
/* vis_batch_imu with d_cov, on the POSE stream through the follow-up scaffold, with TWO carried vis_imu_cov_carry records of its own under the same
 * turn rule -- apart from vis_batch_imu's and vis_batch_imu_jac's, so that any of the three may follow a run, or all.  Refusals in vis_batch_imu's
 * order and codes, np directly after ip. */
int  vis_batch_imu_cov(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, const vis_imu_sample* d_samples, int n_samples,
                       const double* d_tframe, vis_imu_delta* d_delta, vis_imu_cov* d_cov, float* d_rot);
/* The carry the NEXT run's vis_batch_imu_cov continues from (rec NULL: none).  HOST pointer; SYNCHRONISES.  VIS_E_STATE without a context or plan. */
int  vis_batch_imu_cov_init(vis_ctx* ctx, const vis_imu_cov_carry* rec);

/* ---- visual-inertial alignment: the gyro bias, gravity in the root's frame, the factor from trajectory units to metres and a velocity per frame,
 * from the records of vis_batch_trajectory and vis_batch_imu (after Mur-Artal & Tardos 2017 and Qin et al. 2018, restated from the equations; the
 * reference has no such step).  tests/vi_align_ref.py restates every operation below and every record equals it byte for byte: double arithmetic,
 * + - * / sqrt and comparisons only, nothing contracted; products and finite() as in the IMU block; Exp is its ten-term series.
 * (A^T x)[r] = (A[r] x[0] + A[3 + r] x[1]) + A[6 + r] x[2]; a.b = (a[0] b[0] + a[1] b[1]) + a[2] b[2].
 * FRAMES.  q_i = prev[i] normalised as for vis_trajectory_rows.  The TAIL of frame i from its trajectory record T (x = R X + t): zero when T.flags has
 * VIS_TJ_NOT_SAVED or VIS_TJ_OVERFLOW; else C = -(R^T t) (the camera centre), M = r_ic R and Rw[3r + c] = M[3c + r] (IMU -> root, so that
 * Rw_q^T Rw_i = r_ic (R_q R_i^T) r_ic^T is the delta's R), L = R^T p_ci (the lever term; the metric IMU position is s C + L); zero again when one of
 * the 15 numbers is not finite; else segment_seq and epoch_seq of T and VIS_VIT_POSED, with VIS_VIT_EDGE when T.flags lacks VIS_TJ_ROOT, T.parent == q_i
 * and q_i is an index or VIS_KF_CARRIED.  The delta of frame i is USABLE when its flags have none of VIS_IMU_NO_PAIR | NO_CARRY | NO_START | NONFINITE
 * nor of `reject`, its 25 numbers are finite, dt > 0 and its q equals T.parent.  The PARENT of frame i is frame q_i (its tail, its delta) or, for
 * VIS_KF_CARRIED, the carry's `last` tail with `last_delta`, usable when that tail has VIS_VIT_DELTA; the GRANDPARENT is the parent's parent, the
 * carry's `parent` tail when the parent is the carried frame, the carry's `last` when the parent's pair is VIS_KF_CARRIED.  Without a carry those
 * tails are zero.  (S, E) = segment_seq and epoch_seq of the newest posed frame of the call, the carry's when the call has none, else (-1, -1).
 * 1. GYRO BIAS.  Frame i is a PAIR when it has an edge, a posed parent b and a usable delta (R, JRg = J): V = Rw_b^T Rw_i, Er = R^T V,
 * e = (0.5 (Er[7] - Er[5]), 0.5 (Er[2] - Er[6]), 0.5 (Er[3] - Er[1])) (sin(angle) axis: no inverse function); ten terms: (J^T J)[a][b] =
 * (J[a] J[b] + J[3 + a] J[3 + b]) + J[6 + a] J[6 + b] for a <= b in row order, (J^T e)[a] = (J[a] e0 + J[3 + a] e1) + J[6 + a] e2, e.e; a pair with
 * a term that is not finite does not count.  Pairs of every segment and epoch count.  With the totals H, b, c0 and n_pairs: n_pairs < min_pairs gives
 * VIS_VIA_GYRO_FEW; else H dbg = b by LDL^T (below), a failure VIS_VIA_GYRO_SINGULAR; both leave dbg = 0.  c1 = the sum over THIS CALL's pairs of e.e
 * with R Exp(J dbg) in the place of R (c0_call is the same sum before the step).
 * 2. SCALE AND GRAVITY.  Frame c is a TRIPLE with parent b and grandparent a when c and b have edges and (segment_seq, epoch_seq) = (S, E), a is
 * posed (it may be the tail of the epoch's unit edge) and both deltas, b's (a -> b, dt1, dv, dp) and c's (b -> c, dt2, dp'), are usable:
 *   lam[r] = (C_c[r] - C_b[r]) dt1 - (C_b[r] - C_a[r]) dt2;  beta = -(((0.5 dt1) dt2) (dt1 + dt2));
 *   gam[r] = (((Rw_b dp')[r] dt1 - (Rw_a dp)[r] dt2) + (Rw_a dv)[r] (dt1 dt2)) - ((L_c[r] - L_b[r]) dt1 - (L_b[r] - L_a[r]) dt2);
 * with d1[r] = (C_c[r] - C_b[r]) dt1, d2[r] = (C_b[r] - C_a[r]) dt2 and lam[r] = d1[r] - d2[r] (the same roundings): lam s + beta g = gam.  Eleven
 * terms: lam.lam, lam[0] beta, lam[1] beta, lam[2] beta, beta beta, lam.gam, beta gam[0], beta gam[1], beta gam[2], gam.gam and the EXCITATION
 * SCALE d1.d1 + d2.d2 (what lam.lam is the small difference of); not all finite: no triple.  The carried `lin` is M = sum A^T A,
 * A = [lam | beta I], as the rows of its upper triangle (beta beta three times, +0.0 between them), then r = sum A^T gam (4), sum gam.gam and
 * the summed excitation scale (lin[15]).  n_triples < min_triples: VIS_VIA_FEW.  Else M x = r by LDL^T; a failure, or M[0][0] not >
 * VIS_VIA_EXCITATION_REL lin[15] -- the baselines' second differences are rounding noise of the baselines, as under a constant velocity, where
 * M[0][0] stays > 0 by accident -- or a |g_lin| that is not finite is VIS_VIA_SINGULAR, and s_lin, g_lin, g_lin_norm report 0; else s_lin = x[0],
 * g_lin = x[1 ... 3], g_lin_norm = sqrt(g_lin.g_lin); | g_lin_norm - G | > g_tol G sets VIS_VIA_GRAVITY_NORM (a lack of excitation; not a
 * failure); s_lin not > 0: VIS_VIA_SCALE.
 * 3. GRAVITY OF NORM G, from M and r alone.  gh = g_lin / g_lin_norm (each entry), s = s_lin; refine_iters times: k = the first index of the smallest
 * |gh[k]|; d[j] = (j == k) - gh[k] gh[j], b1 = d / sqrt(d.d), b2 = gh x b1; x0 = G gh; rr[i] = r[i] - ((M[i][1] x0[0] + M[i][2] x0[1]) + M[i][3] x0[2]);
 * q = (rr[0], b1.rr[1...3], b2.rr[1...3]); w1[i] = M[1 + i][1...3].b1, w2 alike; N = {M[0][0], M[0][1...3].b1, M[0][1...3].b2; ., b1.w1, b1.w2; ., .,
 * b2.w2}; N y = q by LDL^T; g[j] = (x0[j] + y[1] b1[j]) + y[2] b2[j]; gh = g / sqrt(g.g); s = y[0].  A failed solve or a norm that is not finite and
 * > 0: VIS_VIA_SINGULAR; s not finite and > 0: VIS_VIA_SCALE.  Reported: s and g = G gh; any of VIS_VIA_FEW | SINGULAR | SCALE reports s = 1, g = 0.
 * LDL^T without pivoting, vis_essential_refine's: D[j] = A[j][j] - sum_c (L[j][c] L[j][c]) D[c], a D[j] that is not finite and > 0 fails;
 * L[i][j] = (A[i][j] - sum_c (L[i][c] L[j][c]) D[c]) / D[j]; z[i] = b[i] - sum_c L[i][c] z[c]; x[i] = z[i] / D[i] - sum_{c > i} L[c][i] x[c], c rising,
 * every sum subtracted term by term; an x that is not finite fails.
 * 4. STATES under the reported (s, g).  p[r] = s C[r] + L[r] for a posed frame of (S, E) (VIS_VIS_HAS_P); for one that also has an edge, a usable
 * delta (dt, dv, dp) and a posed parent b of segment S: v[r] = (((p[r] - p_b[r]) / dt + (0.5 g[r]) dt) + (Rw_b z)[r]), z[k] = dv[k] - dp[k] / dt
 * (VIS_VIS_HAS_V); res = sqrt(rho.rho), rho[r] = (lam[r] s + beta g[r]) - gam[r], for a triple (VIS_VIS_HAS_TRIPLE); VIS_VIS_HAS_PAIR; q = q_i.
 * Numbers that are not finite stay 0 without their flag; rms = sqrt(sum rho.rho / n_triples_call).
 * SUMS: the per-frame terms, zero where a frame does not count, under the summation contract "T" of vis_essential_polish with frames in the place of
 * points; a total is carried + call, one addition per entry, the carried first.  The carried linear sums count only when the carry's (segment_seq,
 * epoch_seq) is (S, E) (else VIS_VIA_RESTART); the gyro sums always.  Gyro totals that are not all finite become zero sums and a zero count with
 * VIS_VIA_GYRO_SINGULAR, linear ones with VIS_VIA_SINGULAR; c0_call, c1 and the sum under rms report 0 when they are not finite.
 * CARRY OUT: the totals, (S, E), the tail of the last SAVED frame (q_i != VIS_KF_NOT_SAVED) with VIS_VIT_DELTA when its delta is usable, that delta
 * (else a zero record), its parent's tail (flags & VIS_VIT_POSED), valid = VIS_VIC_VALID; a call that saved nothing passes the three through.  A
 * carry counts when it has VIS_VIC_VALID and its 81 numbers are finite; one that is not finite is ignored with VIS_VIA_BAD_CARRY.  Two cuts of a
 * stream agree within a bound, not byte for byte.
 * On the device: k_via_align, ONE launch of one workgroup of 256 threads, each with at most four frames; tails are recomputed from the trajectory
 * records where they are needed, so there is no workspace; barriers separate the newest-frame search, the sums, the solves (on every thread, the same
 * bits), the second pass and the records.  No loop's length depends on the gate's decisions. */
enum { VIS_VIA_OK = 0, VIS_VIA_GYRO_FEW = 1, VIS_VIA_GYRO_SINGULAR = 2, VIS_VIA_FEW = 4, VIS_VIA_SINGULAR = 8, VIS_VIA_SCALE = 16,
       VIS_VIA_GRAVITY_NORM = 32, VIS_VIA_RESTART = 64, VIS_VIA_BAD_CARRY = 128 };
enum { VIS_VIS_HAS_P = 1, VIS_VIS_HAS_V = 2, VIS_VIS_HAS_TRIPLE = 4, VIS_VIS_HAS_PAIR = 8 };
enum { VIS_VIT_POSED = 1, VIS_VIT_EDGE = 2, VIS_VIT_DELTA = 4 };
enum { VIS_VIC_VALID = 1 };
enum { VIS_VIA_MAX_FRAMES = 1024 };
#define VIS_VIA_EXCITATION_REL 9.094947017729282e-13       /* 2^-40: a relative second difference of 1e-6, below any visual baseline's own error */
typedef struct vis_vi_align_params {     /* 128 bytes; every field finite */
    double  r_ic[9];                     /* identity      vis_imu_params' r_ic */
    double  p_ci[3];                     /* 0             the IMU origin in camera coordinates, metres */
    double  G;                           /* 9.81          the norm of gravity, m/s^2; > 0 */
    double  g_tol;                       /* 0.1           | |g_lin| - G | above g_tol G sets VIS_VIA_GRAVITY_NORM; >= 0 */
    int32_t min_pairs, min_triples;      /* 8, 8          >= 1 */
    int32_t refine_iters;                /* 4             0 ... 16 */
    int32_t reject;                      /* VIS_IMU_EMPTY | VIS_IMU_GAP   delta flags that make a delta unusable */
} vis_vi_align_params;
typedef struct vis_vi_state { double p[3], v[3], res; int32_t flags, q; } vis_vi_state;                                    /* 64 bytes */
typedef struct vis_vi_align {            /* 160 bytes */
    double  dbg[3], c0, c0_call, c1, s, g[3], s_lin, g_lin[3], g_lin_norm, rms;
    int32_t n_pairs, n_triples, n_pairs_call, n_triples_call, segment_seq, epoch_seq, flags, reserved_;
} vis_vi_align;
typedef struct vis_vi_tail { double C[3], Rw[9], L[3]; int32_t segment_seq, epoch_seq, flags, reserved_; } vis_vi_tail;    /* 136 bytes */
typedef struct vis_vi_carry {            /* 720 bytes */
    double  gyro[10], lin[16];
    int32_t n_pairs, n_triples, segment_seq, epoch_seq;
    vis_vi_tail last, parent;
    vis_imu_delta last_delta;
    int32_t valid, reserved_;
} vis_vi_carry;
void vis_default_vi_align_params(vis_vi_align_params* vp);
/* Caller rows, DEVICE pointers, asynchronous on the context's stream, no workspace.  d_prev, d_traj, d_delta: n entries; d_state: NULL or n records;
 * d_result: ONE record; d_carry_in, d_carry_out: NULL or one record each, and not the same one.  n = 0 writes the solution of the carried totals.
 * Refusals, in this order.  VIS_E_INVALID: vp NULL or out of range; a NULL d_prev, d_traj, d_delta or d_result; a pointer that is not aligned (8
 * bytes; d_prev 4); n negative; d_carry_out equal to d_carry_in and not NULL.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_VIA_MAX_FRAMES. */
int  vis_vi_align_rows(vis_ctx* ctx, const vis_vi_align_params* vp, int n, const int32_t* d_prev, const vis_traj_pose* d_traj, const vis_imu_delta* d_delta,
                       const vis_vi_carry* d_carry_in, vis_vi_state* d_state, vis_vi_align* d_result, vis_vi_carry* d_carry_out);
/* The frames of the last vis_batch_run (with VIS_STAGE_POSE; n = its frames) with vis_batch_get_keyframes' pairing, on the POSE stream through the
 * follow-up scaffold, behind vis_batch_trajectory and vis_batch_imu of the run, whose d_traj and d_delta it reads: run -> triangulate -> scale links ->
 * trajectory -> imu -> alignment queues with no host step.  The plan keeps TWO carry records used in turn under the rules of the depth row of
 * vis_batch_scale_links (a repeated call reads what the run was given; vis_batch_plan / vis_batch_reset forget it; a run that was not aligned leaves
 * the next one without a carry).  The caller's buffers are in use until vis_batch_sync.
 * Refusals, in this order.  VIS_E_INVALID: vp as above; a NULL or misaligned (8) d_traj, d_delta or d_result, a misaligned d_state; n negative.
 * VIS_E_STATE: no context / plan / pose stage, or n differs.  VIS_E_CAPACITY: n > VIS_VIA_MAX_FRAMES. */
int  vis_batch_vi_align(vis_ctx* ctx, const vis_vi_align_params* vp, int n, const vis_traj_pose* d_traj, const vis_imu_delta* d_delta,
                        vis_vi_state* d_state, vis_vi_align* d_result);
/* The carry the NEXT run's vis_batch_vi_align continues from (rec NULL: none).  HOST pointer; SYNCHRONISES, like vis_batch_imu_init.
 * VIS_E_STATE without a context or plan. */
int  vis_batch_vi_align_init(vis_ctx* ctx, const vis_vi_carry* rec);
/* Out of scope: this call does not estimate the accelerometer bias (vis_vi_align_ba_rows / vis_batch_vi_align_ba below do) and does not correct dv
 * and dp for dbg itself (vis_batch_imu_correct does, from d_result, and a second call of this one reads the corrected records; or pass bg + dbg to
 * the next vis_batch_imu); weights by the deltas' covariances; feeding anything back into the trajectory, vis_batch_track or vis_batch_pnp.
 * There is no host-pointer single form: one interval aligns nothing. */

/* ---- visual-inertial alignment WITH THE ACCELEROMETER BIAS: the sibling of the block above that also solves for the step dba of the accelerometer
 * bias (Mur-Artal & Tardos 2017, step 3, restated from the equations), from the same records and the Jacobian records of vis_batch_imu_jac.
 * tests/vi_align_ba_ref.py restates every operation below and every record equals it byte for byte; arithmetic, products, a.b, finite() and contract
 * "T" as above.  THE EMBEDDED RECORD `a`, and the embedded carry, EQUAL vis_vi_align_rows' BYTE FOR BYTE on every input (d_carry_in's `carry` in the
 * place of its d_carry_in): the same terms over all pairs and triples, the same contract, the same solves; nothing below changes them.
 * A Jacobian record is USABLE beside its delta when its flags lack VIS_IMU_JAC_NONFINITE, its 36 numbers are finite and its q equals the delta's q.
 * The Jacobian record of the carried frame is the carry's last_jac beside last_delta.  A BIAS TRIPLE is a triple a -> b -> c of step 2 above (its
 * eleven terms finite) whose two Jacobian records, b's and c's, are usable and whose 32 terms below are finite.  With lam, beta, gam, d1, d2 of step
 * 2 above, Jpa_c of c's record, Jpa_b and Jva_b of b's, (X Y)[3r + c] = (X[3r] Y[c] + X[3r + 1] Y[3 + c]) + X[3r + 2] Y[6 + c], and k = 0 ... 8:
 *   B[k] = ((Rw_b Jpa_c)[k] dt1 - (Rw_a Jpa_b)[k] dt2) + (Rw_a Jva_b)[k] (dt1 dt2);   nB[k] = -B[k];
 *   lam s + beta g + nB dba = gam                      (x = (s, g, dba), 7 unknowns, A = [lam | beta I | nB]);
 * dba is the step vis_imu_correct_rows applies (v + Jva dba, p + Jpa dba).  (nB^T v)[c] = (nB[c] v[0] + nB[3 + c] v[1]) + nB[6 + c] v[2].  The 32 TERMS,
 * in the order of the carried `ba`: [0] lam.lam; [1 + c] lam[c] beta; [4] beta beta; [5 + c] (nB^T lam)[c]; [8 + k] beta nB[k]; [17 ...] (nB^T nB)[a][b] =
 * (nB[a] nB[b] + nB[3 + a] nB[3 + b]) + nB[6 + a] nB[6 + b] for a <= b in row order (6); [23] lam.gam; [24 + r] beta gam[r]; [27 + c] (nB^T gam)[c];
 * [30] gam.gam; [31] the excitation scale d1.d1 + d2.d2.  They are summed over the bias triples of the call under contract T, apart from the 11 sums
 * of step 2; a total is carried + call, the carried first, and the carried ones count under the rule of the linear sums ((S, E) of the carry).  Totals
 * that are not all finite become zero sums and a zero count with VIS_VIAB_UNOBSERVABLE.  M7 (7 x 7, symmetric): [0][0] = ba[0]; [0][1 + c] = ba[1 + c];
 * [1 + r][1 + c] = ba[4] when r == c, else +0.0; [0][4 + c] = ba[5 + c]; [1 + r][4 + c] = ba[8 + 3r + c]; [4 + a][4 + b] = ba[17 ...]; r7 = ba[23 ... 29].
 * SOLVE.  n_ba_triples < min_ba_triples: VIS_VIAB_FEW.  Else M7 x = r7 by the LDL^T above WITH THE RELATIVE PIVOT TEST: a D[j] that is not finite, not
 * > 0 or not > pivot_rel A[j][j] fails (under a rotation about one fixed axis the bias along the axis is a copy of a gravity column, D[6] / M7[6][6]
 * is rounding noise of either sign, and D > 0 alone lets it through).  A failure, ba[0] not > VIS_VIA_EXCITATION_REL ba[31], or a
 * sqrt(x[1...3].x[1...3]) that is not finite: VIS_VIAB_UNOBSERVABLE and s_lin7, g_lin7, g_lin7_norm, dba_lin report 0; else they are x[0], x[1 ... 3],
 * that norm and x[4 ... 6]; s_lin7 not > 0: VIS_VIAB_SCALE.  Then refine_iters rounds of step 3 above with the bias columns appended, from gh = g_lin7 /
 * g_lin7_norm, s = s_lin7, dba = dba_lin: k, d, b1, b2, x0 as there; rr[i] = r7[i] - ((M7[i][1] x0[0] + M7[i][2] x0[1]) + M7[i][3] x0[2]), i = 0 ... 6;
 * q = (rr[0], b1.rr[1...3], b2.rr[1...3], rr[4], rr[5], rr[6]); w1[i] = M7[1 + i][1...3].b1, w2 alike; N (6 x 6, symmetric): [0][0] = M7[0][0], [0][1] =
 * M7[0][1...3].b1, [0][2] = M7[0][1...3].b2, [1][1] = b1.w1, [1][2] = b1.w2, [2][2] = b2.w2, [0][3 + c] = M7[0][4 + c], [1][3 + c] = b1.(M7[1][4 + c],
 * M7[2][4 + c], M7[3][4 + c]), [2][3 + c] the same with b2, [3 + a][3 + c] = M7[4 + a][4 + c]; N y = q by the same LDL^T with the same pivot test;
 * g[j] = (x0[j] + y[1] b1[j]) + y[2] b2[j]; gh = g / sqrt(g.g); s = y[0]; dba = y[3 ... 5].  A failed solve, a norm that is not finite and > 0, or a G gh
 * or dba that is not finite: VIS_VIAB_UNOBSERVABLE; s not finite and > 0: VIS_VIAB_SCALE.
 * REPORTED: s_ba = s, g_ba = G gh, dba.  FALLBACK: with any of VIS_VIAB_FEW | UNOBSERVABLE | SCALE, dba = 0, s_ba and g_ba are a.s and a.g, rms_ba = 0 and
 * the states are vis_vi_align_rows' byte for byte -- a correction queued behind a failed estimate changes nothing.  No NaN or infinity reaches a
 * record or a carry.
 * STATES without a fallback: those of step 4 above under (s_ba, g_ba), with dv[k] + (Jva dba)[k] and dp[k] + (Jpa dba)[k] of the frame's own Jacobian
 * record in the place of dv and dp, VIS_VIS_HAS_V only where that record is usable; VIS_VIS_HAS_TRIPLE and res for the BIAS triples, rho[r] = ((lam[r] s_ba
 * + beta g_ba[r]) + (nB dba)[r]) - gam[r] (which is - (B dba)[r], the same bits); rms_ba = sqrt(sum rho.rho / n_ba_triples_call).
 * CARRY: vis_vi_align_rows' carry, the 32 totals and their count, and the Jacobian record of last_delta where both are usable, else (and with no
 * saved frame and no carry) a zero record with VIS_IMU_JAC_NONFINITE; a call that saved nothing passes last_jac through.  The bias part of a carry
 * counts when the embedded carry counts and its 32 + 36 numbers are finite; else it is ignored -- no carried sums, a last_jac that is not usable --
 * with VIS_VIAB_BAD_CARRY.
 * THE CHAIN: dba is at byte 160 of the result, dbg at byte 0, so vis_batch_imu_jac -> vis_batch_vi_align_ba -> vis_batch_imu_correct(d_dbg = d_result,
 * d_dba = &d_result->dba) -> vis_batch_vi_align_ba on the corrected records queues with no host step.
 * On the device: k_via_align<true>, the sibling's ONE launch of one workgroup of 256 threads with the bias sums as a pass of their own between its
 * sums and its solves; no workspace, tails recomputed; k_via_align<false> is the sibling as it was. */
enum { VIS_VIAB_OK = 0, VIS_VIAB_FEW = 1, VIS_VIAB_UNOBSERVABLE = 2, VIS_VIAB_SCALE = 4, VIS_VIAB_BAD_CARRY = 8 };
enum { VIS_VIAB_SUMS = 32 };
#define VIS_VIAB_PIVOT_REL 9.313225746154785e-10           /* 2^-30: between the pivot ratios of one-axis (1e-16) and two-axis (> 1e-6) rotations */
typedef struct vis_vi_align_ba_params {  /* 32 bytes */
    double  pivot_rel;                   /* VIS_VIAB_PIVOT_REL   a pivot not > pivot_rel times its diagonal entry fails; finite, 0 <= pivot_rel < 1 */
    int32_t min_ba_triples;              /* 16            >= 1 */
    int32_t reserved_[5];                /* 0 */
} vis_vi_align_ba_params;
typedef struct vis_vi_align_ba {         /* 304 bytes; dba at byte 160 */
    vis_vi_align a;                      /* vis_vi_align_rows' record of the same inputs */
    double  dba[3], s_ba, g_ba[3], dba_lin[3], s_lin7, g_lin7[3], g_lin7_norm, rms_ba;
    int32_t n_ba_triples, n_ba_triples_call, ba_flags, reserved_;
} vis_vi_align_ba;
typedef struct vis_vi_ba_carry {         /* 1280 bytes */
    vis_vi_carry carry;
    double  ba[VIS_VIAB_SUMS];
    int32_t n_ba_triples, reserved_;
    vis_imu_bias_jac last_jac;           /* of carry.last_delta */
} vis_vi_ba_carry;
void vis_default_vi_align_ba_params(vis_vi_align_ba_params* bp);
/* vis_vi_align_rows with d_jac (n records) beside d_delta.  Refusals in the sibling's order and codes: VIS_E_INVALID for vp or bp NULL or out of
 * range; a NULL d_prev, d_traj, d_delta, d_jac or d_result; a pointer that is not aligned (8 bytes; d_prev 4); n negative; d_carry_out equal to
 * d_carry_in and not NULL.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_VIA_MAX_FRAMES. */
int  vis_vi_align_ba_rows(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, const int32_t* d_prev,
                          const vis_traj_pose* d_traj, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const vis_vi_ba_carry* d_carry_in,
                          vis_vi_state* d_state, vis_vi_align_ba* d_result, vis_vi_ba_carry* d_carry_out);
/* vis_batch_vi_align with d_jac, on the POSE stream through the follow-up scaffold, behind vis_batch_trajectory and vis_batch_imu_jac of the run, with
 * TWO carried vis_vi_ba_carry records of its own under the same turn rule -- apart from vis_batch_vi_align's, so that either may be called for a run,
 * or both.  &d_result->dba is a valid d_dba of vis_batch_imu_correct (THE CHAIN above).  Refusals in vis_batch_vi_align's order and codes. */
int  vis_batch_vi_align_ba(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, const vis_traj_pose* d_traj,
                           const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, vis_vi_state* d_state, vis_vi_align_ba* d_result);
/* The carry the NEXT run's vis_batch_vi_align_ba continues from (rec NULL: none).  HOST pointer; SYNCHRONISES.  VIS_E_STATE without a context or plan. */
int  vis_batch_vi_align_ba_init(vis_ctx* ctx, const vis_vi_ba_carry* rec);
/* Out of scope: folding dbg into dv and dp inside the same call (the queued correct -> align_ba does that); weights by the deltas' covariances (the
 * covariance itself is vis_batch_imu_cov, its whitened residual vis_batch_imu_factor below); a prior on the bias; feeding the result back into the
 * trajectory, vis_batch_track or PnP; more than 1024 frames per call; a host-pointer single form. */

/* ---- THE INERTIAL FACTOR of a pair: the residual of the pair's delta against the aligned states of the frame and its parent, whitened by the
 * delta's covariance -- what says how far a visual pose may disagree with the IMU before it is wrong.  It reads the records of vis_batch_trajectory,
 * vis_batch_imu_cov and vis_batch_vi_align (or vis_batch_vi_align_ba: the head of a vis_vi_align_ba record is a vis_vi_align record and is passed as it
 * is) and writes one vis_imu_factor a frame.  tests/imu_factor_ref.py restates every operation; every record equals it byte for byte.  Double
 * arithmetic, + - * / and comparisons only, nothing contracted; products, tails, "usable delta" and LDL^T are the alignment block's, finite() the IMU's.
 * Frame i with q = prev[i] normalised, T = d_traj[i], the tails of i (pair q) and of q (pair prev[q] normalised), in this order:
 *   q < 0 (no pair, or the parent is the carried frame), or the tail of i lacks VIS_VIT_EDGE, or the tail of q lacks VIS_VIT_POSED: VIS_IMF_NO_PARENT,
 *     and nothing more is looked at.  Else, OR-ed:
 *   d_state[i] or d_state[q] lacks VIS_VIS_HAS_P or VIS_VIS_HAS_V: VIS_IMF_NO_STATE;  d_result->flags has any of VIS_VIA_FEW | SINGULAR | SCALE:
 *     VIS_IMF_NO_ALIGN;  the delta is not usable (parent = T.parent), or d_cov[i].flags has VIS_IMU_COV_NONFINITE, or one of its 45 numbers is not
 *     finite, or its q is not the delta's: VIS_IMF_UNUSABLE.
 * With none of them, (R, dv, dp, dt) of the delta, b = q, g = d_result->g, p and v of d_state:
 *   r[0..2] = e of the alignment's step 1 (V = Rw_b^T Rw_i, Er = R^T V, the sine-axis vector: no inverse function);
 *   w[k] = (v_i[k] - v_b[k]) - g[k] dt;                                   r[3 + k] = (Rw_b^T w)[k] - dv[k];
 *   w[k] = ((p_i[k] - p_b[k]) - v_b[k] dt) - (0.5 g[k]) (dt dt);          r[6 + k] = (Rw_b^T w)[k] - dp[k];
 * a residual that is not finite: VIS_IMF_NONFINITE.  A = the 9 x 9 of d_cov[i].S with var_rot, var_v, var_p added to its diagonal by threes (one
 * addition an entry); A y = r by LDL^T (9) and A[0..2][0..2] y3 = r[0..2] by LDL^T (3); a failed solve: VIS_IMF_SINGULAR; chi2 = r[0] y[0] + r[1] y[1]
 * + ... + r[8] y[8] summed left to right, chi2_rot = (r[0] y3[0] + r[1] y3[1]) + r[2] y3[2]; one that is not finite: VIS_IMF_NONFINITE.  Every flagged
 * record is all zeros but for its flags and q.  For a calibrated covariance and exact states chi2 has mean 9 and chi2_rot mean 3.
 * k_imu_factor, one lane per frame, asynchronous, no workspace.  Out of scope: the factor of a pair whose parent is the carried frame (the parent's
 * state and tail would have to be carried across launches), covariance-weighted alignment, feeding anything back. */
enum { VIS_IMF_OK = 0, VIS_IMF_NO_PARENT = 1, VIS_IMF_NO_STATE = 2, VIS_IMF_NO_ALIGN = 4, VIS_IMF_UNUSABLE = 8, VIS_IMF_SINGULAR = 16, VIS_IMF_NONFINITE = 32 };
typedef struct vis_imu_factor_params {   /* 24 bytes; every field finite and >= 0 */
    double var_rot, var_v, var_p;        /* 0, 0, 0       added to the diagonal of S: the variance of the visual pose's own error in rad^2, (m/s)^2, m^2 */
} vis_imu_factor_params;
typedef struct vis_imu_factor { double r[9], chi2, chi2_rot; int32_t flags, q; } vis_imu_factor;                           /* 96 bytes */
void vis_default_imu_factor_params(vis_imu_factor_params* fp);
/* Caller rows, DEVICE pointers, asynchronous on the context's stream, no workspace.  d_prev, d_traj, d_delta, d_cov, d_state, d_factor: n entries;
 * d_result: ONE vis_vi_align record.  Of vp, r_ic, p_ci and reject are used.
 * Refusals, in this order.  VIS_E_INVALID: vp NULL or out of range; fp NULL or out of range; a NULL d_prev, d_traj, d_delta, d_cov, d_state, d_result
 * or d_factor; a pointer that is not aligned (8 bytes; d_prev 4); n negative.  VIS_E_STATE without a context.  VIS_E_CAPACITY when n > VIS_VIA_MAX_FRAMES. */
int  vis_imu_factor_rows(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, const int32_t* d_prev,
                         const vis_traj_pose* d_traj, const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state,
                         const vis_vi_align* d_result, vis_imu_factor* d_factor);
/* The frames of the last vis_batch_run (with VIS_STAGE_POSE; n = its frames) with vis_batch_get_keyframes' pairing, on the POSE stream through the
 * follow-up scaffold: queued behind vis_batch_trajectory, vis_batch_imu_cov and vis_batch_vi_align (or vis_batch_vi_align_ba) of the run, it reads
 * their buffers with no host step.  The caller's buffers are in use until vis_batch_sync.
 * Refusals as above without d_prev; VIS_E_STATE: no context / plan / pose stage, or n differs. */
int  vis_batch_imu_factor(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, const vis_traj_pose* d_traj,
                          const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state, const vis_vi_align* d_result,
                          vis_imu_factor* d_factor);

/* ---- windowed bundle adjustment over feature tracks (csrc/ba.hip; tests/ba_ref.py restates it and every record, flag byte and output pose equals
 * the restatement byte for byte).  Poses and points are refined TOGETHER by a Schur-complement Levenberg-Marquardt solve, one workgroup per window,
 * all windows in one launch; a second kernel chains the windows through the frames they share and a third moves the points.  Double precision,
 * + - * / sqrt only, nothing contracted, every sum in one fixed order, LDL^T without pivoting, no floating-point atomics: two runs are
 * byte-identical and nothing depends on the launch shape.  Additive: VIS_ABI_VERSION stays 5.
 * WINDOWS.  S = stride.  Window j covers frames first = j S ... last = min(first + S, n - 1); there are ceil((n - 1) / S) of them.  With n <= 1
 *   there is none: the poses are copied, nothing else is written.  A frame HAS A POSE under the rule of the N-view triangulation, on the INPUT
 *   poses.  anchor = the first posed frame of the window (-1: none), held fixed; the FREE frames are the posed frames after it, camera index c =
 *   their rank (n_free <= 16, so at most 96 unknowns after the points are eliminated).  Window j OWNS the slots (i, k < nk(i)) of frames
 *   first + 1 ... last, window 0 also those of frame 0; entries k >= nk(i) are left untouched.
 * POINTS, in slot order (frame rising, keypoint rising).  An owned slot that a keypoint of a later owned frame names as its parent (k_ftri_mark's
 *   rule inside the window) gets the zero record and flag byte 0.  Every other owned slot is a window-end: steps 1-3 of vis_ftrack_triangulate_rows
 *   (the same device functions) over its walk restricted to frames >= anchor, with max_views 17, min_views, gn_iters = tri_gn_iters,
 *   max_reproj_px = init_reproj_px, under the input poses.  VIS_FTP_FEW there -> VIS_BAP_FEW (n_views set, the rest zero); singular, not in front in
 *   every used view or a view's e2 above init_reproj_px^2 -> VIS_BAP_INIT_REJECTED (n_views, rms0_px when the cost was finite, X zero); else
 *   VIS_BAP_USED with X and rms0_px = rms1_px = the triangulation's rms.  A keypoint is a point of at most one window.
 *   n_points, n_obs: the used points and their views.  n_free == 0 or n_points < min_points: VIS_BA_FEW, nothing is solved, cost1 = cost0.
 * OBSERVATION at pose P and point X with pixel (u, v): U, V, W, iw, un, vn, ru, rv, Ju_k, Jv_k exactly as in step 3 of the N-view triangulation,
 *   fu = fx iw, fv = fy iw, e2 = ru ru + rv rv, e = sqrt(e2); w = 1 and term = e2 when huber_px == 0 or e <= huber_px, else w = huber_px / e and
 *   term = (2 huber_px) e - huber_px huber_px.  The camera rows belong to the PnP refinement's update R <- C(omega) R, t <- C(omega) t + dt
 *   (the projection Jacobian times [ -[x_cam]x | I ]):
 *     Cu = (-(fu (un V)), fu (W + un U), -(fu V), fu, 0, -(fu un)),   Cv = (-(fv (W + vn V)), fv (vn U), fv U, 0, fv, -(fv vn)).
 * ONE LINEARISATION at the current state, lambda the damping.
 *   Per point, views in walk order (newest to oldest): V_ab += w (Ju_a Ju_b + Jv_a Jv_b) (a <= b), g_a += w (Ju_a ru + Jv_a rv); the diagonal of V
 *   times (1 + lambda); D0 ... D2, L10, L20, L21 by the 3 x 3 LDL^T of the triangulation -- a pivot not > 0 or not finite: the point SITS THE
 *   LINEARISATION OUT (no term anywhere, its X stays).  Vi = the inverse: column j is the solution of e_j by z0 = b0, z1 = b1 - L10 z0,
 *   z2 = (b2 - L20 z0) - L21 z1, x2 = z2 / D2, x1 = z1 / D1 - L21 x2, x0 = (z0 / D0 - L10 x1) - L20 x2, and Vi_jk (j <= k) is read from column k.
 *   Per free view W_ak = w (Cu_a Ju_k + Cv_a Jv_k) (6 x 3) and Y_ak = (W_a0 Vi_0k + W_a1 Vi_1k) + W_a2 Vi_2k.
 *   Over the points in slot order, absent terms skipped, every accumulator from 0.0: U_ab += w (Cu_a Cu_b + Cv_a Cv_b) (a <= b) and
 *   b_a += w (Cu_a ru + Cv_a rv) per free camera; T[6 c1 + a][6 c2 + b] += (Y1_a0 W2_b0 + Y1_a1 W2_b1) + Y1_a2 W2_b2 for row <= column;
 *   Tg[6 c + a] += (Y_a0 g_0 + Y_a1 g_1) + Y_a2 g_2.  A = Ud - T, Ud = U inside the diagonal blocks with its diagonal entries times (1 + lambda), 0.0
 *   elsewhere; rhs = -(b - Tg).  LDL^T without pivoting by the PnP refinement's recurrences, terms in rising column order:
 *   D_j = A_jj - sum_c (L_jc L_jc) D_c, L_ij = (A_ij - sum_c (L_ic L_jc) D_c) / D_j, z_i = rhs_i - sum_{c<i} L_ic z_c,
 *   d_i = z_i / D_i - sum_{c>i} L_ci d_c.  A pivot not > 0 or not finite: the linearisation is a REJECTION.
 *   Candidate: the free poses by the PnP refinement's Cayley update with d_c; per point Q_k = the sum over its free views in walk order of
 *   ((((W_0k d_0 + W_1k d_1) + W_2k d_2) + W_3k d_3) + W_4k d_4) + W_5k d_5, s_k = -g_k - Q_k, dX_k = (Vi_k0 s_0 + Vi_k1 s_1) + Vi_k2 s_2, X + dX.
 *   cost = the sum over the points in slot order of (the sum over the views in walk order of term).  The candidate is ACCEPTED iff its cost is
 *   finite and < the current cost: lambda <- max(lambda / 10, 1e-12); else REJECTED: lambda <- min(10 lambda, 1e12), the state is kept.
 *   lm_iters counts linearisations, so cost1 <= cost0 always, and lm_iters == 0 returns the input bytes.
 * AFTER THE SOLVE.  rms1_px = (float) sqrt(sum e2 / n_views) at the final state.  With n_accepted > 0 the scale gauge: ca, cin, cout = the centres
 *   -R^T t of the anchor (input) and of the last posed frame (input, final); scale = sqrt(|cin - ca|^2) / sqrt(|cout - ca|^2); not finite or not
 *   > 0: scale = 1, VIS_BA_NO_SCALE, nothing applied; else c' = ca + scale (c - ca), t' = -(R c') for every free frame and X' = ca + scale (X - ca).
 * STITCH, in window order, one fixed sequence inside one launch.  A_in = the anchor's input pose.  A_out = A_in for window 0 and for a window
 *   whose anchor is not its first frame -- the previous window did not deliver it: VIS_BA_RESTART (j > 0) -- else the output pose of the shared
 *   frame.  A_out == A_in byte for byte: the window's poses and points ARE the output.  Else pose_i <- (pose_i o A_in^-1) o A_out (R_rel = R_i
 *   R_a^T, t_rel = t_i - R_rel t_a; R = R_rel R_out, t = R_rel t_out + t_rel; every dot product (a0 b0 + a1 b1) + a2 b2) and
 *   X <- R_out^T ((R_a X + t_a) - t_out).  An output pose that is not finite is replaced by the input pose, a moved point that is not finite keeps its X.  A VIS_BA_FEW window contributes its
 *   input relative poses; a frame without a pose, window 0's anchor and a restarted anchor get their input bytes.
 * A window's record (but for VIS_BA_RESTART) depends only on its own frames; the stitched poses depend on earlier windows by construction.  The
 * absolute pose after stitching is not reliably better than the input: the windows are joined through single frames and each window's scale is
 * normalised to the input's span.  No reported number is ever a NaN or an infinity.
 * Out of scope: observations older than the window, sweeps across windows or overlap by more than one frame, inertial factors, intrinsics as
 * unknowns, writing refined poses into the plan, loop closure. */
enum { VIS_BA_REFINED = 1, VIS_BA_FEW = 2, VIS_BA_RESTART = 4, VIS_BA_NO_SCALE = 8 };
enum { VIS_BAP_USED = 1, VIS_BAP_INIT_REJECTED = 2, VIS_BAP_FEW = 4 };
typedef struct vis_ba_params {   /* 48 bytes; the defaults are this library's own */
    int32_t stride;              /* 8      free frames per window S, 1 ... 16 (<= 96 unknowns) */
    int32_t min_views;           /* 2      used views below which a track is no point, 2 ... 17 */
    int32_t min_points;          /* 12     points below which a window is copied, >= 1 */
    int32_t lm_iters;            /* 10     linearisations, 0 ... 30 */
    int32_t tri_gn_iters;        /* 5      as vis_ftrack_tri_params.gn_iters, 0 ... 10 */
    int32_t reserved_;           /* 0 */
    double  huber_px;            /* 2.4477 (sqrt 5.991); 0 = plain squares; finite, >= 0 */
    double  init_reproj_px;      /* 16.0   gate on the initial point; finite, > 0, <= 1e6 */
    double  lambda0;             /* 1e-4;  in [1e-12, 1e12] */
} vis_ba_params;
typedef struct vis_ba_window {   /* 80 bytes */
    int32_t first, last, anchor, n_free, n_points, n_obs, n_lin, n_accepted, n_rejected, flags, reserved_[2];
    double  cost0, cost1, lambda, scale;
} vis_ba_window;
typedef struct vis_ba_point { double X[3]; float rms0_px, rms1_px; int32_t n_views, flags; } vis_ba_point;   /* 40 bytes */
void vis_default_ba_params(vis_ba_params* bp);
/* Caller-made rows, DEVICE pointers, asynchronous on the context's stream.  d_prev, d_nkp, d_obs, d_xy, d_poses as vis_ftrack_triangulate_rows
 * reads them; d_poses_out: n x 12 doubles (must not overlap d_poses); d_windows: ceil((n - 1) / stride) records; d_points / d_flags: n rows of
 * row_cap entries.
 * Refusals, in this order.  VIS_E_INVALID: bp NULL or outside the ranges above, a NULL pointer, a pointer that is not aligned (16 bytes for d_obs,
 * 8 for d_xy, d_poses, d_poses_out, d_windows and d_points, 4 for d_prev and d_nkp), n or row_cap negative.  VIS_E_STATE without a context.
 * VIS_E_CAPACITY when n x row_cap exceeds 2^28 entries. */
int  vis_ba_rows(vis_ctx* ctx, const vis_ba_params* bp, int n, const int32_t* d_prev, const int32_t* d_nkp, const vis_ftrack_obs* d_obs, int row_cap,
                 const float* d_xy, const double* d_poses, double* d_poses_out, vis_ba_window* d_windows, vis_ba_point* d_points, uint8_t* d_flags);
/* The keypoints and the pairing of the last vis_batch_run (n = its frames) with the observations vis_batch_ftrack wrote for it: on the POSE stream
 * through the follow-up scaffold, behind vis_batch_ftrack of the run and behind the context's stream (where d_poses may have been produced), exactly
 * as vis_batch_ftrack_triangulate is queued; the caller's buffers are in use until vis_batch_sync.  d_poses_out may be handed to
 * vis_batch_ftrack_triangulate, vis_batch_vi_align and vis_batch_imu_factor with no host step.  Nothing is written into the plan.
 * Refusals, in this order.  VIS_E_INVALID: what vis_ba_rows refuses of bp, a NULL or misaligned d_obs, d_poses, d_poses_out, d_windows, d_points or
 * d_flags, n or row_cap negative.  VIS_E_STATE: no context / plan / match stage, or n differs.  VIS_E_CAPACITY: row_cap below the plan's keypoint
 * capacity, or n x row_cap beyond 2^28 entries. */
int  vis_batch_ba(vis_ctx* ctx, const vis_ba_params* bp, int n, const vis_ftrack_obs* d_obs, int row_cap, const double* d_poses, double* d_poses_out,
                  vis_ba_window* d_windows, vis_ba_point* d_points, uint8_t* d_flags);

/* ---- loop-closure candidates: a keyframe database on the device and a brute-force scorer (csrc/kfdb.hip; tests/kfdb_ref.py restates it and every
 * output equals the restatement byte for byte: everything here is integer arithmetic).  Place recognition without a vocabulary: a query frame is
 * matched against EVERY stored keyframe with the matcher's own rules and the number of symmetric matches is the score.  Additive:
 * VIS_ABI_VERSION stays 5.
 * SCORE of a couple (entry E with nE descriptors, query Q with nQ): the length of the symmetric list vis_good_matches_host gives for the pair with E
 *   as the first frame (queryIdx) and Q as the second (trainIdx), ratio = lp.ratio and sym_mode = lp.sym_mode -- k_filter's computeSymMatches on the
 *   matcher's keys (Hamming << 16) | row: ties go to the lower row, a side with fewer than two neighbours fails the ratio test (so a couple with
 *   nE < 2 or nQ < 2 scores 0).  The MATCH LIST of a couple is that list in its order: queryIdx rising, imgIdx = the slot, distance = the Hamming
 *   distance as float.
 * THE DATABASE belongs to a context, not to a plan: it outlives vis_batch_plan and vis_batch_reset (vis_destroy does NOT free it: destroy it first).
 *   A ring of entry_cap slots of kp_cap keypoints.  Adding n rows takes the n slots head, head + 1 ... modulo entry_cap, in row order, and moves the
 *   head; the oldest entries are overwritten (with n > entry_cap a later row of the same call overwrites an earlier one).  The slot never depends
 *   on device data: a row with count <= 0 or id < 0 becomes an EMPTY entry (count 0) that is never scored.  Counts are clamped to
 *   [0, min(row_cap, kp_cap)].  Per entry the device keeps the descriptors as the matcher's FP4 operand (lossless), the pixel (x, y) of every
 *   keypoint, the count and the id.
 * ELIGIBLE: entry e may be scored for query q iff the entry is not empty, id_q >= 0 and (int64) id_e + lp.min_gap <= id_q.  Otherwise its score
 *   is -1.  A query with id_q < 0 or count <= 0 (counts clamped like an entry's) is SKIPPED: flags = VIS_LOOP_SKIPPED, every score -1, no candidate.
 *   A query sees exactly what EARLIER calls on that database added, so the answer is NOT independent of how a stream is cut into launches: query
 *   before add in every launch (tools/run_directory.py --loops), and with min_gap >= the launch length the cut cannot matter.
 * CANDIDATES per query: the lp.topk eligible entries with score >= lp.min_score, ordered by score falling, then id rising, then slot rising, as
 *   vis_loop_cand; rows with fewer are filled with (-1, -1, 0, 0).  vis_loop_query: the id as given, n_keypoints = the count the
 *   query took part with (clamped; 0 when it was skipped), n_scored = the eligible entries, n_cand, best_score = the largest score (-1 when nothing
 *   was scored), flags.
 * MATCHES of a chosen candidate: for query i the call reads ONE vis_loop_cand at d_cand + i * cand_stride records (the caller picks the rank by
 *   offsetting the pointer).  When slot is in [0, entry_cap), the slot is not empty and still holds that id, and query i has a count > 0: the first
 *   min(count, max_pts) entries of the couple's match list (when d_matches is given), d_p1 = the entry's pixels and d_p2 = the query's pixels of
 *   those entries, d_npts[i] = the FULL count (the consumers clamp it to max_pts, so a truncated row is visible).  Otherwise d_npts[i] = 0 and
 *   the rows are left untouched.  The rows are what vis_essential_batch, vis_homography_batch and vis_pnp_batch read.
 * ORDER.  The rows forms run on the context's stream; the batch forms on the POSE stream through the follow-up scaffold behind the matcher of the
 *   last vis_batch_run (like vis_batch_ftrack) and behind the context's stream.  A database carries its own reader events and a last-writer
 *   event: calls on one database take effect in CALL ORDER whichever stream they ride -- an add waits for the pending queries, a query for the
 *   last add.  The rows forms expand the query descriptors into a grow-only block of the context: a call that grows it SYNCHRONISES (every
 *   stream of the context is drained before the old block is freed).
 * LIMITS.  One workgroup per (query, slot) couple; its winner tables take 4 (nE + nQ) bytes of LDS beside 9 KB of tiles: 137 KB at kp_cap 16384
 *   (one workgroup per CU), 10 KB at 1300.  kp_cap <= 16384 is the MFMA matcher's ageing-key limit.  Brute force over entry_cap entries per
 *   query: DESIGN.md 4.27 has the measured cost.
 * Out of scope: a coarse prefilter or vocabulary, Sim(3) or pose-graph correction, feeding a verified loop into vis_batch_ba or
 * vis_batch_trajectory, host adapters, descriptors other than the 32-byte ORB rows. */
enum { VIS_LOOP_SKIPPED = 1 };
typedef struct vis_loop_params {     /* 24 bytes; the defaults are this library's own */
    float   ratio;                   /* 0.8f   taken as written, like vis_params.ratio */
    int32_t sym_mode;                /* VIS_SYM_INTENDED; one of VIS_SYM_* */
    int32_t min_gap;                 /* 30     ids between an entry and a query that may be scored against it, >= 0 */
    int32_t topk;                    /* 4      candidates per query, 1 ... 16 */
    int32_t min_score;               /* 30     any value (twice the score of unrelated views, an eighteenth of a revisit's) */
    int32_t reserved_;               /* 0 */
} vis_loop_params;
typedef struct vis_loop_cand { int32_t id, slot, score, n_keypoints; } vis_loop_cand;                                        /* 16 bytes */
typedef struct vis_loop_query { int32_t id, n_keypoints, n_scored, n_cand, best_score, flags, reserved_[2]; } vis_loop_query; /* 32 bytes */
typedef struct vis_kfdb vis_kfdb;
typedef struct vis_kfdb_info_t { int32_t entry_cap, kp_cap, head, reserved_; int64_t total_added; } vis_kfdb_info_t;        /* 24 bytes */
void vis_default_loop_params(vis_loop_params* lp);
/* Lifetime and bookkeeping.  Refusals, in this order: VIS_E_INVALID (the out pointer NULL, entry_cap outside 1 ... 65536, kp_cap outside
 * 1 ... 16384, cap negative, a NULL or misaligned (4 bytes) output); VIS_E_STATE without a context / database; VIS_E_INVALID for a slot outside
 * [0, entry_cap); VIS_E_NOMEM (create).  vis_kfdb_reset empties every slot and puts the head at 0 (queued as a writer on the context's stream);
 * vis_kfdb_get_entry blocks: id, count and the first min(count, cap) pixel pairs of one slot (HOST pointers; xy may be NULL with cap 0). */
int  vis_kfdb_create(vis_ctx* ctx, int entry_cap, int kp_cap, vis_kfdb** db);
void vis_kfdb_destroy(vis_kfdb* db);
int  vis_kfdb_reset(vis_kfdb* db);
int  vis_kfdb_info(vis_kfdb* db, vis_kfdb_info_t* info);
int  vis_kfdb_get_entry(vis_kfdb* db, int slot, int32_t* id, int32_t* count, float* xy, int cap);
/* Add n rows: DEVICE pointers, asynchronous on the context's stream.  d_kps: n rows of row_cap vis_keypoint; d_desc: n rows of row_cap x 32 bytes;
 * d_nkp, d_ids: n int32.
 * Refusals, in this order.  VIS_E_INVALID: a NULL pointer, a pointer that is not aligned (4 bytes; d_desc 4), n or row_cap negative.  VIS_E_STATE
 * without a database. */
int  vis_kfdb_add_rows(vis_kfdb* db, int n, const vis_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nkp, int row_cap, const int32_t* d_ids);
/* The frames i of the last vis_batch_run (n = its frames) with (seq0 + i) % step == 0, seq0 = the stream number of its frame 0 (frames counted
 * since vis_batch_plan / vis_batch_reset): the host knows seq0, so the slots are host-decided.  Id = seq0 + i; a frame the keyframe gate did not
 * save becomes an empty entry.
 * Refusals, in this order.  VIS_E_INVALID: n negative or step < 1.  VIS_E_STATE: no database / plan / detect stage in the last run, or n differs.
 * VIS_E_CAPACITY: the plan's keypoint capacity exceeds kp_cap -- never a silent cut. */
int  vis_batch_kfdb_add(vis_kfdb* db, int n, int step);
/* Score n query rows against the database: DEVICE pointers, asynchronous on the context's stream.  d_desc, d_nkp, d_ids as in vis_kfdb_add_rows;
 * d_scores: NULL, or n x entry_cap int32 (the whole score row, -1 where not scored); d_cand: n x lp.topk records; d_query: n records.
 * Refusals, in this order.  VIS_E_INVALID: lp NULL or outside its ranges, a NULL pointer (d_scores may be), a pointer that is not aligned (4 bytes),
 * n or row_cap negative.  VIS_E_STATE without a database.  VIS_E_CAPACITY when n x entry_cap exceeds 2^28 couples.
 * Without d_scores the score rows live in a grow-only block of the database: a call that grows it synchronises, and such a query is ordered like
 * an add (two of them never share the block). */
int  vis_kfdb_query_rows(vis_kfdb* db, const vis_loop_params* lp, int n, const uint8_t* d_desc, const int32_t* d_nkp, int row_cap, const int32_t* d_ids,
                         int32_t* d_scores, vis_loop_cand* d_cand, vis_loop_query* d_query);
/* The same for the frames of the last vis_batch_run: ids and counts are the run's, the operands the plan's expanded descriptors; a frame not on the
 * step, or one the keyframe gate did not save, is skipped; a frame off the step launches no work.  The last run must have included VIS_STAGE_MATCH (the expanded descriptors are the matcher's;
 * VIS_E_STATE otherwise), where vis_batch_kfdb_add needs the detect stage alone.  Refusals as vis_batch_kfdb_add, after lp and the pointers as above. */
int  vis_batch_kfdb_query(vis_kfdb* db, const vis_loop_params* lp, int n, int step, int32_t* d_scores, vis_loop_cand* d_cand, vis_loop_query* d_query);
/* The matches of one chosen candidate per query.  d_kps: n rows of row_cap vis_keypoint of the queries; d_matches: NULL, or n rows of max_pts
 * vis_dmatch; d_p1, d_p2: n rows of max_pts (x, y) floats; d_npts: n int32.
 * Refusals, in this order.  VIS_E_INVALID: lp as above, a NULL pointer (d_matches may be), a pointer that is not aligned (8 bytes for d_p1 / d_p2,
 * 4 otherwise), n, row_cap, cand_stride or max_pts negative.  VIS_E_STATE without a database. */
int  vis_kfdb_match_rows(vis_kfdb* db, const vis_loop_params* lp, int n, const vis_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nkp,
                         int row_cap, const vis_loop_cand* d_cand, int cand_stride, int max_pts, vis_dmatch* d_matches, float* d_p1, float* d_p2,
                         int32_t* d_npts);
/* The same for the frames of the last vis_batch_run (keypoints, operands and counts are the plan's; a frame the gate did not save has count 0).
 * Refusals as vis_batch_kfdb_add (step apart), after lp and the pointers as above. */
int  vis_batch_kfdb_match(vis_kfdb* db, const vis_loop_params* lp, int n, const vis_loop_cand* d_cand, int cand_stride, int max_pts,
                          vis_dmatch* d_matches, float* d_p1, float* d_p2, int32_t* d_npts);

/* ---- synthetic EuRoC-shaped stream ("S-752") -------- */
/* Integer-only generator, identical bytes on every machine.  canvas: canvas_dim^2 bytes. */
int  vis_synth_canvas(uint8_t* canvas, int canvas_dim, uint64_t seed);
int  vis_synth_frame(const uint8_t* canvas, int canvas_dim, uint64_t seed, int t,
                     int w, int h, uint8_t* out, int out_stride);
/* "S-752P": the same stream with a second depth layer (1.5x parallax, same direction) and independently moving objects
 * (outliers) on top of the static background: image motion that is NOT one planar shift, so the adaptive RANSAC stop
 * does not trigger after a handful of hypotheses.  Same integer-only rule on host and device. */
int  vis_synth_frame_parallax(const uint8_t* canvas, int canvas_dim, uint64_t seed, int t,
                              int w, int h, uint8_t* out, int out_stride);
/* n consecutive frames t0 .. t0+n-1 generated on the device into d_out (frame stride = stride*h); d_canvas = the canvas
 * of vis_synth_canvas in device memory.  mode 0 = S-752, 1 = S-752P.  Byte-identical to the host generators.
 * The kernel is queued on the context's stream, behind whatever produced d_canvas there, and d_out may be read by work queued on that
 * stream after the call -- but the call is NOT asynchronous for the host: it uploads a per-frame table from pageable memory and blocks
 * until the context's stream has drained, the caller's earlier work on it included.  (A test-stream generator, not a product path.) */
int  vis_synth_frames_device(vis_ctx* ctx, const uint8_t* d_canvas, int canvas_dim, uint64_t seed, int t0, int n,
                             int w, int h, int stride, int mode, uint8_t* d_out);

#ifdef __cplusplus
}
#endif
#endif /* VISLAM_HIP_H_ */
