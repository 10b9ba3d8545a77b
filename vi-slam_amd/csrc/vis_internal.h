// vis_internal.h -- internal declarations of libvislam_hip (MI355X / gfx950 only).
// Product code: never includes or links anything under oracle/.
#ifndef VIS_INTERNAL_H_
#define VIS_INTERNAL_H_

#include <atomic>
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/vislam_hip.h"

#define VIS_BATCH_SETS 2          // record sets of a batch plan (see Plan)
#define VIS_NSLOTS 32            // device keyframe slots of the single-frame API (Camera::frameList)
#define VIS_RANSAC_MAX_M 8192    // max correspondences per RANSAC problem
#define VIS_MAX_MODELS 10
#define VIS_MAX_SIDE 4095        // largest frame side of the half pyramid, the gradients and the alignment (rectify.hip's too)
// k_fast (detect.hip) works on ITEMS: a strip of 32 lanes x 4 pixels = 128 pixel columns (120 of them emit; 1 score halo + 3 ring
// columns on either side) marched down 8 score rows at a time, at most VIS_FS_NCH chunks = 8 * NCH - 2 emitting rows.  An item owns a
// candidate slot sized by the 3x3-NMS bound of its emit region (60 x 31 = 1860 <= 2048): a slot cannot overflow.
#define VIS_FS_EMIT_W 120
#define VIS_FS_NCH 8
#define VIS_FS_EMIT_H (8 * VIS_FS_NCH - 2)
#define VIS_TILE_CAND_CAP 2048
static_assert(((VIS_FS_EMIT_W + 1) / 2) * ((VIS_FS_EMIT_H + 1) / 2) <= VIS_TILE_CAND_CAP, "NMS bound of an item");

struct LevelInfo {
    int w, h, stride;            // stride: bytes per row of the level buffer (level 0: caller's)
    int quota;                   // nfeaturesPerLevel
    float scale;                 // layerScale
    size_t frame_bytes;          // stride*h
    int cand_cap;                // tiles * VIS_TILE_CAND_CAP: every FAST item owns a slot sized by the 3x3-NMS bound
    int tile_base;               // first global tile index of this level
    int surv_cap;                // survivors of the FAST cut (2*quota + ties), LDS sort size
    int keep_cap;                // kept per level (quota + ties)
    int tiles_x, tiles_y;        // FAST items: strips x segments
    int wave_base, nwaves;       // k_fast waves of this level (two items each) in the plan's FastWave table
};

// device-resident compact kNN entry: key = (dist << 16) | trainIdx, 0xFFFFFFFF = none
typedef vis_pose_result PoseOut;       // E, R, t (double) + n_inliers, n_pose_good, iters_run, n_points, n_models, undecided_max

// The pending readers of one buffer set of the batch path (sets used in turn: the writer of a set waits for the readers of its last use).
// Per stream, one slot per stream of a context (A, U, M, P): the event behind the LAST reader queued there, which stands for every earlier
// one (a stream runs in order).  note() and clear() are bookkeeping only (host/stage_selftest.cpp drives them on the CPU); wait() makes
// the HIP calls.  A held event that is recorded again stands for a later point: a false dependency at worst (vis_ctx), never a missed one.
struct ReaderGuard {
    hipStream_t stream[4] = {};
    hipEvent_t event[4] = {};
    void note(hipStream_t s, hipEvent_t e) { int i = 0; while (i < 3 && stream[i] && stream[i] != s) i++; stream[i] = s; event[i] = e; }
    hipError_t wait(hipStream_t writer) const {
        for (int i = 0; i < 4 && stream[i]; i++) { const hipError_t e = hipStreamWaitEvent(writer, event[i], 0); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    void clear() { *this = ReaderGuard(); }
};

// Which of a plan's TWO carried rows a follow-up launch continues (vis_batch_ftrack, _scale_links, _trajectory, _imu, _vi_align, _vi_align_ba: "the rules of the depth row",
// include/vislam_hip.h).  A launch reads row `slot` -- the row of the last saved frame of the launch before, beside the carried record of the keyframe
// gate -- and writes the other one, slot ^ 1: two rows, so that a call never reads the row it writes and a call repeated for the same run reads again
// the row it read itself.  in = the row the last committed launch read, run = its run_count (-1: none), have = whether it had a row to read.
// pick() changes nothing; the caller commits once its launch was queued.  A run that was skipped leaves nothing to read.  Bookkeeping only,
// like ReaderGuard::note (host/stage_selftest.cpp walks the table of cases on the CPU).
struct Turn {
    int in = 0, run = -1; bool have = false;
    struct Pick { int slot; bool have; };
    Pick pick(int run_count) const { return run == run_count ? Pick{in, have} : Pick{in ^ 1, run >= 0 && run == run_count - 1}; }
    void commit(Pick p, int run_count) { in = p.slot; have = p.have; run = run_count; }
    void forget() { run = -1; have = false; }                      // vis_batch_reset, an _init call without a record (`in` stays: either row will do)
    // an _init call's record takes the place of what a call for the current run would have left for the next one: copy it to seed_slot(), then seeded()
    int seed_slot() const { return in ^ 1; }
    void seeded(int run_count) { run = run_count; }
};

// a grow-only device block of the context (vis_grow_block)
struct DevBlock { void* p = nullptr; size_t bytes = 0; };

// vis_batch_track's keyframe snapshot: one frame in the layout of a gradient-set frame (vis_grad_frame_elems elements per array),
// level 0 of gray dense (w x h); valid = the pair to the carried keyframe may read it (set per call, not stored)
struct TrackSnapshot { uint8_t* gray = nullptr; int16_t* gx = nullptr; int16_t* gy = nullptr; bool valid = false; };
// the trajectory chain's device state: final_poseCam, the last residual Track composed and whether there is one (two frames saved)
struct TrackState { vis_se3f pose; vis_se3f last; int32_t have_last; int32_t pad_; };
struct Plan {
    int w = 0, h = 0, stride = 0, B = 0, L = 0;
    int fs_nch = VIS_FS_NCH;     // chunks (8 score rows) per k_fast segment of this plan: 8 for batches, fewer for a handful of frames (more, shorter waves)
    int nrec = 0;                // keypoint/descriptor records (batch: B+1, single: VIS_NSLOTS)
    int kcap = 0;                // keypoints per record (sum of keep_cap)
    int npairs = 0;              // pair result capacity
    int root = 0;                // grid root
    int pose_mcap = 0;           // correspondences per pair the pose stage is sized for (root^2, or kcap with VIS_POSE_SYM)
    LevelInfo lv[VIS_MAX_LEVELS];
    // ---- device buffers
    uint8_t* d_stage = nullptr;              // single-frame upload staging (stride x h)
    uint8_t* d_pyr[VIS_MAX_LEVELS] = {};     // level l >= 1: B x h_l x stride_l
    uint32_t* d_rs_tab[VIS_MAX_LEVELS] = {}; // level l >= 1: coefficient tables of the resize step l-1 -> l (detect.hip k_resize_tab; built on first use)
    uint32_t* d_cand[VIS_MAX_LEVELS] = {};   // B x tiles_l x VIS_TILE_CAND_CAP packed (score<<24 | y<<12 | x)
    int32_t* d_tile_cnt = nullptr;           // B x total_tiles candidates per tile
    int total_tiles = 0;
    void* d_fast_tiles = nullptr;            // total_waves x FastWave (detect.hip): per-wave record of k_fast (two items of one level)
    int total_waves = 0;
    int32_t* d_seg_cnt = nullptr;            // B x L kept counts
    float4*  d_seg_kp[VIS_MAX_LEVELS] = {};  // B x keep_cap (x, y, response, unused)
    int32_t* d_flags = nullptr;              // device error flags (1 word)
    uint32_t* d_angle_tab = nullptr;         // IC-angle byte weight/mask table for k_describe
    // speculative FAST threshold of batched streams (detect.hip fast_tile): per-level prediction, per-(frame, level) cuts of the
    // last batch, and the work list of the pairs whose prediction was too high
    bool speculate = false;
    int32_t* d_tau = nullptr;                // L
    int32_t* d_seg_cut = nullptr;            // B x L
    int32_t* d_fix = nullptr;                // 1 + B x L
    // VIS_STAGE_UPDATE: B x vis_grad_frame_elems(w, h) half pyramids; VIS_STAGE_GRADIENT: the Scharr gradients of the batch
    // (Camera::computeGradient) beside the detect chain.  Plan-owned, allocated on first use, TWO sets used in turn: vis_batch_align of
    // step i reads set i & 1 on the pose stream while the side stream of step i + 1 fills the other one (with one set the alignment, the
    // next step's gradients and -- through the detect stream's join -- the next matcher formed a serial chain as long as the step).
    // grad[grad_set] = the set the last vis_batch_run wrote; readers = the alignments that read the set (matched by pointer identity).
    struct GradSet { uint8_t* half = nullptr; int16_t* gx = nullptr; int16_t* gy = nullptr; uint8_t* g = nullptr; ReaderGuard readers; };
    GradSet grad[2];
    int grad_set = 0;
    bool half_valid = false;
    bool grad_valid = false;
    // records
    vis_keypoint* d_kps = nullptr;           // nrec x kcap
    uint8_t* d_desc = nullptr;               // nrec x kcap x 32
    int32_t* d_nkp = nullptr;                // nrec
    int8_t* d_descx = nullptr;               // nrec x kcap x 128: descriptor bits as FP4 (e2m1) +1/-1, two per byte (MFMA matcher operand)
    // guided matching (match.hip k_warp): npairs x kcap predictions + 16 floats (the rotation of a single-frame call); allocated by the
    // first guided call of the plan (ensure_warp), so a context that never asks for a window has the footprint it always had
    float2* d_warp = nullptr;
    // The follow-ups' blocks, each allocated ONCE by the first call of the plan that needs it and never replaced (api.hip plan_block: one list per
    // block, measured for the allocation and bound by every call into a work struct of its own; plan_destroy frees them), and the turns of the
    // carried rows that five of them hold (Turn).  A plan starts with the turns' defaults and nothing commits before the block exists.
    // vis_batch_pnp (PnpPlanWork): per frame the keypoint table of its keyframe's pair (npairs x kcap), the linked rows (npairs x pose_mcap map
    // points and pixels) and their counts
    void* d_pnp_ws = nullptr;
    // vis_batch_ftrack (FtPlanWork): FtWork for B frames of kcap keypoints and, behind it, the two carried observation rows (kcap records each).
    // seq_next counts the frames of every detecting vis_batch_run since plan / reset, seq0 = the stream number of frame 0 of the last run
    void* d_ft_ws = nullptr; Turn ft;
    int seq_next = 0, seq0 = 0;
    // vis_batch_scale_links / vis_batch_trajectory (TrajPlanWork), allocated by the first call of either: the depth rows (B x kcap doubles), the two
    // carried depth rows, SlWork for B pairs of pose_mcap entries, TjWork for B frames, the two carried records
    void* d_tj_ws = nullptr; Turn sl, tj;
    // vis_batch_imu (ImuPlanWork), allocated by the first call or by vis_batch_imu_init: the lifting table for B frames and the two carried records
    void* d_imu_ws = nullptr; Turn imu;
    // vis_batch_imu_jac (ImuJacPlanWork), allocated by the first call or by vis_batch_imu_jac_init: the 62-slot lifting table for B frames and the two
    // carried vis_imu_jac_carry records
    void* d_imuj_ws = nullptr; Turn imuj;
    // vis_batch_imu_cov (ImuCovPlanWork), allocated by the first call or by vis_batch_imu_cov_init: the 71-slot lifting table for B frames and the two
    // carried vis_imu_cov_carry records
    void* d_imuc_ws = nullptr; Turn imuc;
    // vis_batch_vi_align (ViaPlanWork), allocated by the first call or by vis_batch_vi_align_init: the two carried records
    void* d_via_ws = nullptr; Turn via;
    // vis_batch_vi_align_ba (ViabPlanWork), allocated by the first call or by vis_batch_vi_align_ba_init: its own two carried records
    void* d_viab_ws = nullptr; Turn viab;
    // pairs
    int32_t* d_pair_q = nullptr;             // npairs: query record index (-1 = no pair)
    int32_t* d_pair_t = nullptr;
    uint32_t* d_knn12 = nullptr;             // npairs x kcap x 2 keys
    uint32_t* d_knn21 = nullptr;
    // What k_filter writes (sym, good: npairs x kcap / root^2 matches, counts; p1, p2: npairs x pose_mcap x 2 points) and the pose stage
    // / vis_batch_align / the results download read.  A batch plan owns TWO sets, used in turn like the record sets: with one set the filter
    // of step i + 1 had to wait for the pose stage and the download of step i, and the pose stage of step i + 1 for that filter -- a serial
    // loop (pose chain + download + filter) that set the step's period as soon as it grew longer than the detect chain (results download:
    // - 8 %).  Single-frame plans have set 0 only.  out() = the set of the last vis_batch_run (or of the one queueing its launches).
    struct MatchOut { vis_dmatch* sym = nullptr; int32_t* nsym = nullptr; vis_dmatch* good = nullptr; int32_t* ngood = nullptr;
                      float* p1 = nullptr; float* p2 = nullptr; ReaderGuard readers; };
    MatchOut mo[2];
    int mo_cur = 0;
    MatchOut& out() { return mo[mo_cur]; }
    float* d_hf = nullptr;                   // root band limits (float accumulation on host)
    float* d_wf = nullptr;
    // pose
    double* d_n1 = nullptr;                  // npairs x root^2 x 2 normalised points
    double* d_n2 = nullptr;
    uint8_t* d_mask = nullptr;               // npairs x root^2 inlier mask of the winning E
    int32_t* d_samples = nullptr;            // npairs x max_iters x 5
    double* d_models = nullptr;              // npairs x max_iters x 10 x 9
    int32_t* d_counts = nullptr;             // npairs x max_iters x 10  (-1 = no model)
    int32_t* d_rstate = nullptr;             // npairs x 4: niters, maxGood, bestIter, bestModel
    PoseOut* d_pose = nullptr;               // npairs
    int32_t* d_worklist = nullptr;           // 2 + npairs: count, pairs that need RANSAC chunks beyond the first, item counter of the roots kernel
    double* d_hyp = nullptr;                 // npairs x max_iters hypothesis records (VIS_HYP_DOUBLES each, element-major)
    int max_iters = 0;
    bool have_prev = false;                  // batch: record 0 holds the previous batch's last frame
    int last_n = 0;                          // frames in the last batch
    int pyr_frames = 0;                      // frames whose levels >= 1 the last launch_detect of this plan wrote into d_pyr (0: it has not run)
    int carry_from = 0;                      // absolute record to copy into the next set's record 0 (0 = none)
    // batch plans keep VIS_BATCH_SETS sets of records (keypoints, descriptors, expanded descriptors) and walk them round-robin: the detect
    // chain of batch i + SETS waits for the matcher of batch i.  (Round 5: three sets instead of two change nothing -- in steady state the
    // low-priority matcher / pose streams progress only as fast as the detect chain leaves them room, and the detect stream ends up waiting
    // for them however far ahead it may run: 393.4 k frames/s with three sets against 395-400 k with two, same build.)
    int nsets = 1, rec_per_set = 0, run_count = 0, last_base = 0;
    bool pair0_valid = false;                // last run: frame 0 had a predecessor
    // Per record set: the pair tables (query / train record; pqn = pq with pair 0 disabled) and, with the keyframe gate
    // (vis_params.keyframe_min_points at vis_batch_plan; 0 = off, gq and kf_link do not exist), the gated query table the matcher reads
    // instead of pq / pqn and the link table (vis_batch_get_keyframes' prev[], the alignment's previous frames).  matcher: waited for
    // where launch_detect first writes the set; links (the alignments that read kf_link): waited for before k_keyframe_links.
    // d_kf_state = {last saved record (absolute, -1 = none), a frame has been saved since reset}: written by k_keyframe_links, read by
    // the next one (keyframe.hip) on the detect stream.
    struct RecordSet { int32_t* pq = nullptr; int32_t* pt = nullptr; int32_t* pqn = nullptr; int32_t* gq = nullptr; int32_t* kf_link = nullptr;
                       ReaderGuard matcher, links; };
    RecordSet rec[VIS_BATCH_SETS];
    RecordSet& last_set() { return rec[last_base / rec_per_set]; }   // the record set of the last vis_batch_run
    int kf_min = 0;
    int32_t* d_kf_state = nullptr;
    // vis_batch_track (track.hip), allocated on first use: the snapshot of the last saved frame of the last tracked launch (the
    // carried keyframe's images for the next launch's pair to it) and the trajectory state the chain kernel carries from launch to
    // launch.  run_seq counts the vis_batch_run calls since plan / reset, track_seq the one the last vis_batch_track consumed.
    int last_stages = 0, run_seq = 0, track_seq = 0;
    TrackSnapshot snap{};
    TrackState* d_track_state = nullptr;
    vis_se3f track_init = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};   // vis_batch_track_init's pose: where vis_batch_reset restarts the chain
};

#define VIS_POSE_TABLE_M 64                  // the frame-at-a-time pose entry points take their RANSAC samples from the table for M <= 64 (root^2 = 49 in the reference)
struct vis_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t pose_stream = nullptr;       // RANSAC/pose of batch i overlaps detect/match of batch i+1
    hipStream_t match_stream = nullptr;      // knn + filters of batch i overlap the detect chain of batch i+1
    hipStream_t update_stream = nullptr;     // VIS_STAGE_UPDATE (Camera::Update): streaming work beside the VALU-bound detect chain
    // Ordering events (api.hip ordering_events).  Forks / joins: ev_update_fork A -> U, ev_update_done U -> A, ev_detect_done A -> M,
    // ev_filter_done M -> P, ev_align_fork A -> P; ev_pose_done / _start and ev_match_start also time.  Reader events (ReaderGuard):
    // ev_match_done[record set], ev_pose_done_set / ev_results_done_set / ev_tri_done / ev_epi_done[matcher-output set], ev_align_done[] in turn.  Each is recorded
    // again only by the next reader of its kind -- normally of the same set two steps on, after that set's writer queued its wait.
    // The reader events of the follow-ups of a batch step (ev_tri_done, ev_epi_done, ev_align_done) are recorded in ONE place: on_pose_stream().
    hipEvent_t ev_filter_done = nullptr, ev_pose_done = nullptr, ev_pose_start = nullptr, ev_detect_done = nullptr, ev_match_start = nullptr;
    hipEvent_t ev_update_fork = nullptr, ev_update_done = nullptr, ev_align_fork = nullptr;
    hipEvent_t ev_match_done[VIS_BATCH_SETS] = {}, ev_pose_done_set[2] = {}, ev_results_done_set[2] = {}, ev_align_done[2] = {}, ev_tri_done[2] = {}, ev_epi_done[2] = {};
    bool pose_pending = false;
    // the last two vis_batch_align / vis_batch_track (align[align_last] the latest) and the caller frames each read: align_reader()
    struct AlignRead { hipEvent_t event = nullptr; const uint8_t* begin = nullptr; const uint8_t* end = nullptr; };
    AlignRead align[2]; int align_last = 0;
    bool pose_attr_set = false;              // > 64 KiB LDS opt-in of the RANSAC solver kernels done on this context's device
    bool pose_grids_set = false; int pose_grid[4] = {0, 0, 0, 0};   // resident-workgroup grids of the work-list pose kernels on this device (pose.hip pose_grids)
    vis_params p;
    vis_align_weights aw = {VIS_W_IDENTITY, 4.6851f, 1.4826f, 0};   // vis_set_align_weights: read where an alignment is enqueued
    std::string err;
    Plan* single = nullptr;
    Plan* batch = nullptr;
    vis_timings tm;
    hipEvent_t ev[12];
    bool ev_ok = false;
    // grow-only scratch for the *_host entry points
    void* d_scratch = nullptr; size_t scratch_bytes = 0;
    // The grow-only workspaces of the device-rows calls, grown by vis_grow_block alone (vis_carve_block where the call carves a list) and freed by
    // vis_destroy: vis_essential_batch (api.hip PoseWork: the pose stage's buffers for n rows), vis_ftrack_link_rows (FtWork for n rows of
    // row_cap), vis_scale_link_rows (SlWork), vis_trajectory_rows (TjWork), vis_imu_preintegrate_rows and vis_imu_preintegrate (the lifting
    // table), vis_imu_preintegrate_jac_rows and vis_imu_preintegrate_jac (the table with the Jacobians' blocks), vis_imu_preintegrate_cov_rows and
    // vis_imu_preintegrate_cov (the table with the covariance's blocks).  SEVEN blocks, apart from the scratch
    // block and from each other: a host-pointer call between two batches, or another of these calls, cannot move the block a queued call was given
    DevBlock ess_ws, ft_ws, sl_ws, tjr_ws, imu_ws, imuj_ws, imuc_ws;
    DevBlock kfdb_ws;                        // vis_kfdb_query_rows / vis_kfdb_match_rows (kfdb.hip): the queries' expanded descriptors
    // grow-only PINNED host block of the single-frame entry points: a caller's pageable buffer is copied through it, so that every
    // upload / download of a call is an asynchronous copy on the context's stream and the call blocks ONCE, at its end (HostStage, api.hip)
    void* h_pin = nullptr; size_t h_pin_bytes = 0; void* h_pin_dev = nullptr;   // (h_pin_dev: the block's device address; nullptr = not device-accessible)
    int stage_live = 0;                      // HostStage objects alive on this context: vis_ensure_pin refuses to replace the block under one (VIS_E_STATE)
    // diagnostics of the single-frame path (vis_debug_counters): times the host blocked on the device / copies queued since the context was made
    unsigned long long n_host_waits = 0, n_copies = 0;
    unsigned long long undecided_max = 0;    // largest vis_pose_result::undecided_max a pose call of this context downloaded
    int slot_valid[VIS_NSLOTS];
    // cv::RNG sample tables for M in [6, sample_max_m], built on the host for (seed, max_iters)
    int32_t* d_sample_table = nullptr; int sample_max_m = 0; int sample_iters = 0; unsigned long long sample_seed = 0;
};

// The alignment still queued on the pose stream that a write of caller memory [b, e) waits for: the latest if it read the range or the
// range is not known (b == nullptr: gradient buffers, feeder copies), else the one before it, which also stands for every older one (the
// pose stream runs them in order).  nullptr: none pending.
inline hipEvent_t align_reader(const vis_ctx* ctx, const void* b, const void* e) {
    const vis_ctx::AlignRead& last = ctx->align[ctx->align_last];
    if (!last.event || !b || (last.begin < (const uint8_t*)e && (const uint8_t*)b < last.end)) return last.event;
    return ctx->align[ctx->align_last ^ 1].event;
}
inline hipError_t wait_align_readers(const vis_ctx* ctx, hipStream_t s, const void* b = nullptr, const void* e = nullptr) {
    const hipEvent_t ev = align_reader(ctx, b, e);
    return ev ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
}

// roctx ranges around the stage families of a batched step (readable rocprofv3 --marker-trace timelines); compiled in only by
// `make ROCTX=1` (-DVIS_HAVE_ROCTX -lrocprofiler-sdk-roctx: a diagnostic build), otherwise no-ops
#ifdef VIS_HAVE_ROCTX
#include <rocprofiler-sdk-roctx/roctx.h>
struct VisRange { explicit VisRange(const char* n) { roctxRangePushA(n); } ~VisRange() { roctxRangePop(); } };
#else
struct VisRange { explicit VisRange(const char*) {} };
#endif

// every kernel launch of the library is counted (vis_debug_counters: launches per frame of the single-frame path, bench.py's
// single_frame_api leg): one relaxed atomic increment beside a launch that costs microseconds (contexts of different host threads
// launch concurrently: a plain global would be a data race)
extern std::atomic<unsigned long long> vis_g_launches;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    do { vis_g_launches.fetch_add(1, std::memory_order_relaxed); kernel<<<(grid), (block), (lds), (stream)>>>(__VA_ARGS__); } while (0)

#define HIPCHK(ctx, call)                                                          \
    do { hipError_t e_ = (call);                                                   \
         if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
                                 return VIS_E_HIP; } } while (0)

// Every launcher enqueues on ctx->stream: the batch path points it at one of the context's other streams for the length of a block.
// Restored however the block is left, so a failure between the launches cannot leave the context enqueueing on the wrong stream.
struct StreamScope {
    vis_ctx* ctx; hipStream_t saved;
    StreamScope(vis_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
    ~StreamScope() { ctx->stream = saved; }
    StreamScope(const StreamScope&) = delete; StreamScope& operator=(const StreamScope&) = delete;
};

// The alignments' ring (vis_ctx::align): two reader events in turn, so the one before stays valid for the sets and the caller frames it
// guards.  next = the event the next alignment records; commit, once that record succeeded = it is the latest and read frames [b, e)
// (what vis_rectify_batch must not overwrite before it).  Bookkeeping only, like ReaderGuard::note.
inline hipEvent_t align_ring_next(const vis_ctx* ctx) { return ctx->ev_align_done[ctx->align_last ^ 1]; }
inline void align_ring_commit(vis_ctx* ctx, const uint8_t* b, const uint8_t* e) {
    ctx->align_last ^= 1;
    ctx->align[ctx->align_last] = {ctx->ev_align_done[ctx->align_last], b, e};
}
inline void note_readers(std::initializer_list<ReaderGuard*> readers, hipStream_t s, hipEvent_t e) { for (ReaderGuard* g : readers) if (g) g->note(s, e); }

// A follow-up of the last vis_batch_run, queued on the pose stream (DESIGN.md has the table of what each entry point orders and notes):
// optionally behind the context's stream (FU_FORK: where the caller's inputs, the detect chain and the joined gradients were queued) and
// behind the matcher of the last record set (FU_MATCHER); run() launches under a StreamScope of the pose stream; then the reader event --
// `done`, or the next of the alignments' ring with the caller frames [frames, frames_end) -- is recorded behind it and noted on every
// guard of `readers` that is not null: the buffers the call read, whose next writer waits for it.  A failing run() records and notes nothing.
enum { FU_FORK = 1, FU_MATCHER = 2 };
struct FollowUp { unsigned order; hipEvent_t done; const uint8_t* frames = nullptr; const uint8_t* frames_end = nullptr; };
template <class Run> int on_pose_stream(vis_ctx* ctx, const FollowUp& fu, Run run, std::initializer_list<ReaderGuard*> readers) {
    (void)hipSetDevice(ctx->device);
    const hipStream_t sP = ctx->pose_stream;
    if (fu.order & FU_FORK) { HIPCHK(ctx, hipEventRecord(ctx->ev_align_fork, ctx->stream)); HIPCHK(ctx, hipStreamWaitEvent(sP, ctx->ev_align_fork, 0)); }
    if (fu.order & FU_MATCHER) HIPCHK(ctx, ctx->batch->last_set().matcher.wait(sP));
    { StreamScope on(ctx, sP); const int rc = run(); if (rc) return rc; }
    const hipEvent_t ev = fu.done ? fu.done : align_ring_next(ctx);
    HIPCHK(ctx, hipEventRecord(ev, sP));
    if (!fu.done) align_ring_commit(ctx, fu.frames, fu.frames_end);
    note_readers(readers, sP, ev);
    return VIS_OK;
}

// Carve typed, 256-byte aligned pieces out of the context scratch block.  With a null base the carver MEASURES: it hands out nullptr and
// only advances `off`, through the same offsets a bound carver walks.  A take that would end beyond `limit` sets `overflow` and hands out
// nullptr, and so does every take after it (HostStage::overflow's twin: vis_carve refuses the call before anything is queued).
struct Carver {
    char* base; size_t off; size_t limit;
    int n = 0; bool overflow = false;
    template <class T> T* take(size_t count) {
        const size_t at = (off + 255) & ~(size_t)255, bytes = count * sizeof(T);
        if (overflow || at > limit || bytes > limit - at) { overflow = true; return nullptr; }
        off = at + bytes; n++;
        return base ? (T*)(base + at) : nullptr;
    }
    // What a HostStage needs to pass every carved buffer through the pinned block once per direction, `ways` directions: a stage take is
    // 64-byte aligned and at least 4 bytes long, so the 256 bytes per buffer cover a buffer staged in up to three pieces.
    size_t pin_bound(int ways) const { return (size_t)ways * (off + (size_t)n * 256); }
};
int vis_ensure_scratch(vis_ctx* ctx, size_t bytes);

// ---- host staging of the single-frame entry points (api.hip explains; vis_ensure_pin grows the context's pinned block) ----
#include <cstring>
#include <algorithm>
int vis_ensure_pin(vis_ctx* ctx, size_t bytes);
int launch_copy_jobs(vis_ctx* ctx, hipStream_t st, int njobs, void* const* dst, const void* const* src, const size_t* bytes);
// The block may only be replaced (vis_ensure_pin frees and re-allocates it when it grows) while NO HostStage is alive: a stage hands out
// addresses inside the block (take / down) that the caller reads after wait().  Round 5's host SIGSEGV (gpurun_out/r5r_gdb.log: libc's copy
// faulting on its first destination byte, 0x7ff600c00000 = 2 MiB-aligned, unmapped, 360 960 bytes = the first up2d of a call, i.e. offset 0 of
// a block that was no longer there) was a stage built on a block that a later vis_ensure_pin of the same call freed; every entry point sizes
// the block BEFORE it builds its stage since f950f5e, and since round 6 the rule is enforced instead of kept by convention: the stage reads
// the block's address from the context at every use, counts itself in ctx->stage_live, and vis_ensure_pin answers VIS_E_STATE instead of
// freeing a block under a live stage (vi-slam_amd/host/stage_selftest.cpp drives both refusals on the CPU).
struct HostStage {
    vis_ctx* ctx; size_t off = 0; hipError_t err = hipSuccess; bool overflow = false;
    explicit HostStage(vis_ctx* c) : ctx(c) { ctx->stage_live++; }
    ~HostStage() { ctx->stage_live--; }
    HostStage(const HostStage&) = delete; HostStage& operator=(const HostStage&) = delete;
    char* base_now() const { return (char*)ctx->h_pin; }
    void* take(size_t bytes) {
        off = (off + 63) & ~(size_t)63;
        if (!ctx->h_pin || off + bytes > ctx->h_pin_bytes) { overflow = true; return nullptr; }
        void* p = base_now() + off; off += bytes; return p;
    }
    // host (pageable) -> device, asynchronous: through the pinned block.  Dword-granular uploads are collected like the downloads and
    // read out of the block by one kernel of the library per six of them -- at flush_ups(), which every entry point calls behind its
    // last upload, in front of its first kernel (down() and wait() flush too, so a forgotten call shows as a wrong result in the parity
    // tests, not as a missing transfer).
    void* up_dst[6]; const void* up_src[6]; size_t up_bytes[6]; int up_n = 0;
    void flush_ups() {
        if (!up_n) return;
        if (launch_copy_jobs(ctx, ctx->stream, up_n, up_dst, up_src, up_bytes) != VIS_OK && err == hipSuccess) err = hipErrorLaunchFailure;
        ctx->n_copies++;
        up_n = 0;
    }
    void up(void* d, const void* h, size_t bytes) {
        if (!bytes) return;
        void* p = take(bytes);
        if (!p) return;
        std::memcpy(p, h, bytes);
        if (!(bytes & 3) && !((uintptr_t)d & 3) && ctx->h_pin_dev) {
            if (up_n == 6) flush_ups();
            up_dst[up_n] = d; up_src[up_n] = (const char*)ctx->h_pin_dev + ((char*)p - base_now()); up_bytes[up_n] = bytes; up_n++;
            return;
        }
        flush_ups();                                               // (stream order among the uploads)
        const hipError_t e = hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess && err == hipSuccess) err = e;
        ctx->n_copies++;
    }
    // rows of an image with a host stride -> a device image with its own stride
    void up2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t height) {
        char* p = (char*)take(width * height);
        if (!p) return;
        for (size_t y = 0; y < height; y++) std::memcpy(p + y * width, (const char*)h + y * hpitch, width);
        if (dpitch == width && !((width * height) & 3) && !((uintptr_t)d & 3) && ctx->h_pin_dev) {      // dense on the device: one copy job
            if (up_n == 6) flush_ups();
            up_dst[up_n] = d; up_src[up_n] = (const char*)ctx->h_pin_dev + (p - base_now()); up_bytes[up_n] = width * height; up_n++;
            return;
        }
        flush_ups();
        const hipError_t e = hipMemcpy2DAsync(d, dpitch, p, width, width, height, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess && err == hipSuccess) err = e;
        ctx->n_copies++;
    }
    // device -> the pinned block, asynchronous; valid after wait().  Dword-granular downloads are collected and written by ONE kernel of
    // the library per six of them (launch_copy_jobs; the block is device-accessible) when wait() is called -- every call site requests
    // its downloads right in front of its wait(), behind the kernels that produce them -- instead of one runtime copy each.
    void* dn_dst[6]; const void* dn_src[6]; size_t dn_bytes[6]; int dn_n = 0;
    void flush_downs() {
        if (!dn_n) return;
        if (launch_copy_jobs(ctx, ctx->stream, dn_n, dn_dst, dn_src, dn_bytes) != VIS_OK && err == hipSuccess) err = hipErrorLaunchFailure;
        ctx->n_copies++;
        dn_n = 0;
    }
    void* down(const void* d, size_t bytes) {
        flush_ups();
        void* p = take(std::max(bytes, (size_t)4));
        if (!p || !bytes) return p;
        if (!(bytes & 3) && !((uintptr_t)d & 3) && ctx->h_pin_dev) {
            if (dn_n == 6) flush_downs();
            dn_dst[dn_n] = (char*)ctx->h_pin_dev + ((char*)p - base_now()); dn_src[dn_n] = d; dn_bytes[dn_n] = bytes; dn_n++;
            return p;
        }
        const hipError_t e = hipMemcpyAsync(p, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess && err == hipSuccess) err = e;
        ctx->n_copies++;
        return p;
    }
    // the one place a single-frame entry point blocks
    int wait() {
        if (overflow) { ctx->err = "host staging block too small (internal)"; return VIS_E_NOMEM; }
        flush_ups(); flush_downs();
        if (err != hipSuccess) { ctx->err = std::string("staged copy: ") + hipGetErrorString(err); return VIS_E_HIP; }
        ctx->n_host_waits++;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); return VIS_E_HIP; }
        return VIS_OK;
    }
};

// The buffers of one host-pointer call, declared ONCE: layout(Carver&) assigns the call's d_* pointers.  It runs twice -- measuring, which
// sizes the scratch block and, from the same list, the pinned block (Carver::pin_bound; ways = 2 where a buffer is staged up AND down or in
// many pieces), then bound to ctx->d_scratch.  Both blocks have their final size when this returns: build the HostStage after it.
template <class Layout> int vis_carve(vis_ctx* ctx, Layout&& layout, int ways = 1) {
    Carver measure{nullptr, 0, SIZE_MAX};
    layout(measure);
    int rc = vis_ensure_scratch(ctx, measure.off);
    if (!rc) rc = vis_ensure_pin(ctx, measure.pin_bound(ways));
    if (rc) return rc;
    Carver cv{(char*)ctx->d_scratch, 0, ctx->scratch_bytes};
    layout(cv);
    if (cv.overflow) { ctx->err = "device scratch block too small (internal)"; return VIS_E_NOMEM; }
    return VIS_OK;
}
// The grow rule of the context's device-rows workspaces, in ONE place (api.hip): a request that fits -- a zero-byte one always does -- changes
// nothing; otherwise every stream of the context is drained (work queued on any of them may still use the old block), the block is freed and a new
// one allocated, or the call refused: VIS_E_NOMEM, "<who>: out of device memory for the workspace".  *replaced = the block is a new one.
// (vis_ensure_scratch is the same rule written apart: it answers a failed allocation with VIS_E_HIP and the runtime's text.)
int vis_grow_block(vis_ctx* ctx, DevBlock& b, size_t bytes, const char* who, bool* replaced = nullptr);
// vis_carve's twin for such a block: the list runs measuring, the block grows to that size (at_least: a floor), the list runs bound to the block
template <class Layout> int vis_carve_block(vis_ctx* ctx, DevBlock& b, const char* who, Layout&& layout, size_t at_least = 0, bool* replaced = nullptr) {
    Carver measure{nullptr, 0, SIZE_MAX};
    layout(measure);
    if (measure.overflow) { ctx->err = std::string(who) + ": the workspace exceeds the address space"; return VIS_E_NOMEM; }
    const int rc = vis_grow_block(ctx, b, std::max(measure.off, at_least), who, replaced);
    if (rc) return rc;
    Carver cv{(char*)b.p, 0, b.bytes};
    layout(cv);
    if (cv.overflow) { ctx->err = std::string(who) + ": workspace too small (internal)"; return VIS_E_NOMEM; }
    return VIS_OK;
}
// a launch failed behind queued uploads: drain the stream (they read the pinned block, which the next call may refill), then report
inline int vis_drain(vis_ctx* ctx, int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }


// ---- host-side geometry / tables (geometry.cpp) ----
int  vis_compute_levels(const vis_params& p, int w, int h, int stride0, LevelInfo* lv, int fs_nch = VIS_FS_NCH);
void vis_grid_limits(const vis_params& p, int* root, std::vector<float>& hf, std::vector<float>& wf);

struct SynthOrigin;
int  vis_synth_origin(int dim, uint64_t seed, int t, int w, int h, SynthOrigin* o);

// ---- plan management (api.hip) ----
int  plan_create(vis_ctx* ctx, int w, int h, int stride, int B, int nrec, int npairs, Plan** out, int nsets = 1);
void plan_destroy(Plan* pl);

// ---- kernel launchers (each enqueues on ctx->stream) ----
int launch_copy_jobs(vis_ctx* ctx, hipStream_t st, int njobs, void* const* dst, const void* const* src, const size_t* bytes);   // detect.hip: <= 6 dword-granular copies in one launch
int launch_detect(vis_ctx* ctx, Plan* pl, const uint8_t* d_frames, int n, int rec0, int carry_rec = -1, hipEvent_t after_resize = nullptr, const ReaderGuard* records_free = nullptr);   // carry_rec >= 0: copy that record to rec0 - 1 before k_describe; after_resize: recorded behind the pyramid launches; records_free: waited for before the chain's first write to the record set
int build_fast_tiles(vis_ctx* ctx, Plan* pl);
int launch_expand(vis_ctx* ctx, Plan* pl, int rec_first, int rec_count);
struct MatchGuide { const float* d_rot; float radius; };             // 9 floats per pair (row-major), window half-side in pixels
int ensure_warp(vis_ctx* ctx, Plan* pl);                              // api.hip: pl->d_warp, allocated once per plan
int launch_warp(vis_ctx* ctx, Plan* pl, int npairs, const float* d_rot, float2* d_warp);
int launch_match(vis_ctx* ctx, Plan* pl, int npairs, const MatchGuide* guide = nullptr);   // guide: the windowed 2-NN (k_warp first; needs pl->d_warp)
int launch_filter(vis_ctx* ctx, Plan* pl, int npairs);
int launch_pose(vis_ctx* ctx, Plan* pl, int npairs);
int launch_keyframe_links(vis_ctx* ctx, Plan* pl, int set, int n);   // keyframe.hip: carry the last saved record into the set, gate + link the batch
int reset_keyframe_state(vis_ctx* ctx, Plan* pl);                     // keyframe.hip: nothing saved, nothing carried
int align_batch_links(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int w, int h, int stride, int n,
                      const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy, const float* d_pts, const int32_t* d_npts,
                      int max_pts, const int32_t* d_prev, const TrackSnapshot* snap, const vis_se3f* d_init,
                      vis_align_result* d_out);   // align.hip: vis_align_batch with pair i = (d_prev[i] -> i), nullptr = i-1; snap: vis_batch_track
int ensure_track_buffers(vis_ctx* ctx, Plan* pl);                     // track.hip: the snapshot + chain state, allocated and initialised once per plan
int reset_track_state(vis_ctx* ctx, Plan* pl, bool keep_last);        // track.hip: chain state = track_init (+ no last residual unless keep_last); synchronous
int launch_track_snapshot(vis_ctx* ctx, Plan* pl, const uint8_t* d_frames, const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                          const int32_t* links, int n);               // track.hip: the launch's last saved frame -> pl->snap (ctx->stream)
int launch_track_chain(vis_ctx* ctx, Plan* pl, const int32_t* links, int n, const vis_align_result* d_align,
                       vis_track_result* d_track);                    // track.hip: Track() over the launch (ctx->stream)
int launch_half_pyramid(vis_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, uint8_t* d_out[5]);
// gradient.hip: Camera::Update / computeGradient / patch builders, batched
size_t vis_grad_frame_elems(int w, int h);
// cvRound(n * 0.5), round half to even: the size cv::resize(src, dst, Size(), 0.5, 0.5) gives the next level (include/vislam_hip.h)
static inline int vis_half_dim(int n) { return (n >> 1) + ((n & 1) & ((n >> 1) & 1)); }
static inline void vis_half_dims(int w, int h, int lw[5], int lh[5]) {
    lw[0] = w; lh[0] = h;
    for (int l = 1; l < 5; l++) { lw[l] = vis_half_dim(lw[l - 1]); lh[l] = vis_half_dim(lh[l - 1]); }
}
int launch_half_pyramid_batch(vis_ctx* ctx, const uint8_t* d_frames, int w, int h, int stride, size_t frame_bytes, int n, uint8_t* d_pyr);
int launch_gradient(vis_ctx* ctx, const uint8_t* d_frames, int w, int h, int stride, size_t frame_bytes, int n,
                    const uint8_t* d_pyr, int scale, int16_t* d_gx, int16_t* d_gy, uint8_t* d_g);
int launch_patch_points(vis_ctx* ctx, const vis_keypoint* d_good, int n, int w, int h, float* d_patch, float* d_debug, int cap,
                        int32_t* d_counts);
#define VIS_HYP_DOUBLES 97                // 96 doubles + 2 int32 per (pair, iteration): see pose.hip HR_*
int pose_run(vis_ctx* ctx, int npairs, int mcap, int max_iters, const float* d_p1, const float* d_p2, const int32_t* d_npts,
             double* d_n1, double* d_n2, int32_t* d_samples, double* d_models, int32_t* d_counts, int32_t* d_rstate,
             const double* d_E_in, uint8_t* d_mask, PoseOut* d_pose, int do_ransac, int do_pose, int32_t* d_worklist, double* d_hyp);
// pose.hip: k_triangulate + k_tri_summary on ctx->stream.  d_pose: npairs records (R, t, n_points); d_p1 / d_p2 / d_mask (may be null): rows of
// in_stride correspondences; d_points / d_flags: rows of row_cap >= in_stride entries
int triangulate_run(vis_ctx* ctx, const vis_tri_params* tp, int npairs, int in_stride, int row_cap, const PoseOut* d_pose,
                    const float* d_p1, const float* d_p2, const uint8_t* d_mask, vis_map_point* d_points, uint8_t* d_flags,
                    vis_tri_summary* d_summary);
int  vis_build_sample_table(vis_ctx* ctx, int max_m);
// epipolar.hip: k_f2f_batch / k_epi_filter on ctx->stream over npairs rows of in_stride (x, y) points (d_npts valid, clamped); d_keep: rows of row_cap >= in_stride.
// d_draws: iters x 2 words -- point indices in [0, m) as they stand with `direct`, else raw draws reduced modulo m - 1
int f2f_batch_run(vis_ctx* ctx, int npairs, int in_stride, const float* d_p1, const float* d_p2, const int32_t* d_npts,
                  const float* d_rot, const float* d_tref, const int32_t* d_draws, int iters, bool direct, vis_f2f_result* d_out);
int epi_filter_run(vis_ctx* ctx, int npairs, int in_stride, const float* d_p1, const float* d_p2, const int32_t* d_npts,
                   const float* d_rot, const float* d_t, double threshold, int row_cap, uint8_t* d_keep, int32_t* d_nkeep);
// homography.hip: k_homography_batch on ctx->stream over npairs rows of in_stride (x, y) points; hp validated by the caller; d_E: records of e_stride
// doubles that begin with E, or null; d_mask: rows of row_cap >= in_stride bytes, or null
int homography_batch_run(vis_ctx* ctx, const vis_homography_params* hp, int npairs, int in_stride, const float* d_p1, const float* d_p2,
                         const int32_t* d_npts, const int32_t* d_draws, const double* d_E, int e_stride, int row_cap, uint8_t* d_mask,
                         vis_homography_result* d_out);
// pose.hip: k_hpose_svd + k_hpose_vote on ctx->stream; hq validated by the caller; d_mask: rows of row_cap >= in_stride bytes, or null; d_rot: npairs x 9
// floats, or null
int hpose_run(vis_ctx* ctx, const vis_hpose_params* hq, int npairs, int in_stride, const vis_homography_result* d_h, const float* d_p1,
              const float* d_p2, const int32_t* d_npts, int row_cap, const uint8_t* d_mask, const float* d_rot, vis_hpose_result* d_out);
// pnp.hip: k_pnp_batch + k_pnp_refine on ctx->stream over n rows of in_stride points (d_X: x_stride doubles apart; d_xy: pixels); pp validated by the
// caller; d_mask: rows of row_cap >= in_stride bytes, or null
int pnp_batch_run(vis_ctx* ctx, const vis_pnp_params* pp, int n, int in_stride, const double* d_X, int x_stride, const float* d_xy,
                  const int32_t* d_npts, const int32_t* d_draws, int row_cap, uint8_t* d_mask, vis_pnp_result* d_out);
// k_pnp_link + pnp_batch_run + k_pnp_rel on ctx->stream: vis_batch_pnp's body (api.hip has the arguments' origin)
int pnp_link_run(vis_ctx* ctx, const vis_pnp_params* pp, int n, const int32_t* d_links, int pair0_valid, int mcap, int mstride, int kcap,
                 const vis_dmatch* d_matches, const int32_t* d_npts, const float* d_p2, const PoseOut* d_pose, const vis_map_point* d_points,
                 const uint8_t* d_flags, int row_cap, int require, int32_t* d_table, double* d_X, float* d_xy, int32_t* d_cnt,
                 const int32_t* d_draws, int mask_cap, uint8_t* d_mask, vis_pnp_result* d_out, vis_pnp_link* d_link);
// refine.hip: k_essential_refine on ctx->stream over n rows of in_stride (x, y) points; ep validated by the caller; d_start: n records of rec_stride
// doubles with R at r_off and t at t_off; d_mask: rows of row_cap >= in_stride bytes, or null
int essential_refine_run(vis_ctx* ctx, const vis_eref_params* ep, int n, int in_stride, const double* d_start, int rec_stride, int r_off, int t_off,
                         const float* d_p1, const float* d_p2, const int32_t* d_npts, int row_cap, const uint8_t* d_mask, vis_eref_result* d_out);
// refine.hip: k_essential_polish on ctx->stream (one wave per pair for in_stride <= 64, else four); ep validated by the caller; d_mask: rows of mask_cap
// bytes or null; d_mask_out: rows of out_cap bytes; d_pose_out: n records or null
int essential_polish_run(vis_ctx* ctx, const vis_epolish_params* ep, int n, int in_stride, const PoseOut* d_pose, const float* d_p1, const float* d_p2,
                         const int32_t* d_npts, int mask_cap, const uint8_t* d_mask, int out_cap, uint8_t* d_mask_out, vis_epolish_result* d_out,
                         PoseOut* d_pose_out);
// homography_polish.hip: k_homography_polish on ctx->stream (one wave per pair for in_stride <= 64, else four); hp validated by the caller; d_mask:
// rows of mask_cap bytes or null, d_mask_out: rows of out_cap bytes (both >= in_stride); d_h_out: n records or null
int homography_polish_run(vis_ctx* ctx, const vis_hpolish_params* hp, int n, int in_stride, const vis_homography_result* d_h, const float* d_p1,
                          const float* d_p2, const int32_t* d_npts, int mask_cap, const uint8_t* d_mask, int out_cap, uint8_t* d_mask_out,
                          vis_hpolish_result* d_out, vis_homography_result* d_h_out);
// ftrack.hip.  The workspace of one linking call over n frames of R keypoints, declared once: win (2 x n x R: the smallest list position that claimed
// keypoint k of frame i, then of its parent, 0xFFFFFFFF = none), s0 / s1 (n x R (ancestor, distance) pairs, the two buffers of the pointer doubling), par
// (n x R parents).  24 bytes per keypoint.
struct FtWork {
    uint32_t* win = nullptr; int2* s0 = nullptr; int2* s1 = nullptr; int32_t* par = nullptr;
    void layout(Carver& cv, size_t n, size_t R) { win = cv.take<uint32_t>(2 * n * R); s0 = cv.take<int2>(n * R); s1 = cv.take<int2>(n * R); par = cv.take<int32_t>(n * R); }
};
// The frames' pairing and counts as both forms hold them: prev == nullptr is the gate-off pairing (i - 1; frame 0: the carried frame iff pair0);
// nkp[i] = keypoints of frame i.
struct FtFrames { const int32_t* prev; int pair0; const int32_t* nkp; };
// k_ft_claim + k_ft_parent + the doubling rounds + k_ft_finish (+ k_ft_carry when d_carry_out) on ctx->stream.  R: keypoints per frame the workspace
// and the counts are sized for; d_links: rows of link_cap; d_mask: rows of mask_cap or null; d_mcnt: null, or a further bound of every list's count
// (int32 at d_mcnt[i * mcnt_stride]); d_carry: a row of R records or null; d_obs: rows of ocap >= R records of which the first wcap <= ocap are written
int ftrack_link_run(vis_ctx* ctx, const FtWork& W, int n, int R, FtFrames fr, const vis_dmatch* d_links, const int32_t* d_nlinks, int link_cap,
                    const uint8_t* d_mask, int mask_cap, const int32_t* d_mcnt, int mcnt_stride, const vis_ftrack_obs* d_carry, int seq0, int ocap,
                    int wcap, vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame, vis_ftrack_obs* d_carry_out);
// k_ftri_clear + k_ftri_mark + k_ftri_points on ctx->stream.  d_xy: the pixel (u, v) of keypoint k of frame i is the two floats at byte
// i * xy_row + k * xy_step; tp validated by the caller
int ftrack_triangulate_run(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, int R, FtFrames fr, const vis_ftrack_obs* d_obs, int ocap,
                           const void* d_xy, size_t xy_row, int xy_step, const double* d_poses, vis_ftrack_point* d_points, uint8_t* d_flags,
                           vis_ftrack_tri_summary* d_summary);
// ba.hip.  The poses copied to d_poses_out, then k_ba_window (one workgroup per window) + k_ba_stitch + k_ba_points on ctx->stream, no workspace (a
// cache of every used point's views was built and measured: DESIGN.md 4.26 has why it is not here); bp validated by the caller; d_xy as above
int ba_run(vis_ctx* ctx, const vis_ba_params* bp, int n, int R, FtFrames fr, const vis_ftrack_obs* d_obs, int ocap, const void* d_xy, size_t xy_row,
           int xy_step, const double* d_poses, double* d_poses_out, vis_ba_window* d_windows, vis_ba_point* d_points, uint8_t* d_flags);
// trajectory.hip.  SL_LDS_CAP: list entries per pair up to which the ratio pass keeps its keys in LDS; TJ_LDS_N: frames per call up to which the chain
// keeps its elements in LDS.  The workspaces beyond those sizes, declared once: keys (n x mcap 64-bit patterns), D / I (13 doubles and 4 ints per
// frame, structure of arrays).
#define SL_LDS_CAP 1024
#define TJ_LDS_N 256
struct SlWork {
    unsigned long long* keys = nullptr;
    void layout(Carver& cv, size_t n, size_t mcap) { keys = mcap > SL_LDS_CAP ? cv.take<unsigned long long>(n * mcap) : nullptr; }
};
struct TjWork {
    double* D = nullptr; int32_t* I = nullptr;
    void layout(Carver& cv, size_t n) { D = n > TJ_LDS_N ? cv.take<double>(13 * n) : nullptr; I = n > TJ_LDS_N ? cv.take<int32_t>(4 * n) : nullptr; }
};
// k_sl_depth + k_sl_ratio (+ k_sl_carry when d_carry_out) on ctx->stream; sp validated by the caller.  d_links: rows of link_cap of which the first
// mcap <= min(link_cap, pts_cap) count; d_points / d_flags: rows of pts_cap; d_carry: a row of row_cap doubles or null; d_depth: n rows of row_cap
int scale_link_run(vis_ctx* ctx, const vis_scale_link_params* sp, int n, FtFrames fr, const vis_dmatch* d_links, const int32_t* d_nlinks, int link_cap,
                   int mcap, const PoseOut* d_pose, const vis_map_point* d_points, const uint8_t* d_flags, int pts_cap, const double* d_carry,
                   int row_cap, double* d_depth, unsigned long long* d_keys, vis_scale_link* d_link, double* d_carry_out);
// k_tj_chain on ctx->stream: one launch.  d_carry: one record or null; d_poses, d_carry_out: null or the outputs
int trajectory_run(vis_ctx* ctx, int n, FtFrames fr, const PoseOut* d_pose, const vis_scale_link* d_link, const vis_traj_pose* d_carry, int seq0,
                   int same_epoch_only, double* d_wsD, int32_t* d_wsI, vis_traj_pose* d_traj, double* d_poses, vis_traj_pose* d_carry_out);
// imu.hip.  The lifting table of n frames: 26 eight-byte slots x frames x levels, levels = the bits of n (imu_table_bytes).  k_imu_intervals +
// k_imu_pairs on ctx->stream; ip validated by the caller; d_carry, d_rot, d_carry_out: null or the record / rows
size_t imu_table_bytes(int n);
int imu_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
            const vis_imu_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, float* d_rot, vis_imu_carry* d_carry_out);
// the same with the bias Jacobians of v and p: a table of 62 slots (imu_jac_table_bytes), k_imu_intervals<true> + k_imu_pairs<true>; d_jac: n records
size_t imu_jac_table_bytes(int n);
int imu_jac_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                   const vis_imu_jac_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac, float* d_rot, vis_imu_jac_carry* d_carry_out);
// the same with the covariance: a table of 71 slots (imu_cov_table_bytes), k_imu_cov_intervals + k_imu_cov_pairs; np validated by the caller; d_cov: n records
size_t imu_cov_table_bytes(int n);
int imu_cov_launch(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples,
                   const double* d_tframe, const vis_imu_cov_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, vis_imu_cov* d_cov, float* d_rot,
                   vis_imu_cov_carry* d_carry_out);
// k_imu_correct on ctx->stream: the records of a bias step; d_dba, d_rot, d_status: null or the rows
int imu_correct_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                       const double* d_dba, vis_imu_delta* d_out, float* d_rot, int32_t* d_status);
// vi_align.hip.  k_via_align on ctx->stream: one launch, no workspace; vp validated by the caller; d_carry, d_state, d_carry_out: null or the records
// k_imu_factor on ctx->stream: the whitened inertial residual of every pair; vp, fp validated by the caller; d_result: one record
int imu_factor_launch(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, FtFrames fr, const vis_traj_pose* d_traj,
                      const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state, const vis_vi_align* d_result,
                      vis_imu_factor* d_factor);
int via_launch(vis_ctx* ctx, const vis_vi_align_params* vp, int n, FtFrames fr, const vis_traj_pose* d_traj, const vis_imu_delta* d_delta,
               const vis_vi_carry* d_carry, vis_vi_state* d_state, vis_vi_align* d_result, vis_vi_carry* d_carry_out);
// the same with the accelerometer bias: k_via_align<true>; bp validated by the caller; d_jac: n records
int via_ba_launch(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, FtFrames fr, const vis_traj_pose* d_traj,
                  const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const vis_vi_ba_carry* d_carry, vis_vi_state* d_state,
                  vis_vi_align_ba* d_result, vis_vi_ba_carry* d_carry_out);
// refine.hip: the first d_npts[i] (clamped) bytes of every row of in_stride bytes -> rows of row_cap bytes (vis_essential_batch's mask)
int mask_rows_run(vis_ctx* ctx, int n, int in_stride, int row_cap, const int32_t* d_npts, const uint8_t* d_src, uint8_t* d_dst);
#define VIS_RSTATE_WORDS 16

#endif
