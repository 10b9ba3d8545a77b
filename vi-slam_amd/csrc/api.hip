// api.hip -- the C ABI of libvislam_hip.so (include/vislam_hip.h): context, plans, single-frame
// entry points (one per OpenCV-CUDA call site of the reference) and the batched stream path.
// Host code only; kernels live in detect.hip / match.hip / pose.hip / epipolar.hip / homography.hip / pnp.hip.
#include "vis_internal.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>

static const char* VIS_VERSION_STR = "vislam_hip 0.1 (gfx950)";

extern "C" const char* vis_version(void) { return VIS_VERSION_STR; }

extern "C" const char* vis_strerror(int code) {
    switch (code) {
        case VIS_OK: return "ok";
        case VIS_E_INVALID: return "invalid argument";
        case VIS_E_NODEVICE: return "no HIP device";
        case VIS_E_HIP: return "HIP runtime error";
        case VIS_E_CAPACITY: return "capacity exceeded";
        case VIS_E_STATE: return "invalid state / call order";
        case VIS_E_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}

// "dddd:bb:dd.f" of a HIP device: what the multi-GPU launchers gather per rank to show that N ranks ran on N different devices
extern "C" int vis_device_pci_bus_id(int device, char* out, int len) {
    if (!out || len < 16) return VIS_E_INVALID;
    out[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return VIS_E_NODEVICE; }
    if (device < 0 || device >= n) return VIS_E_INVALID;
    if (hipDeviceGetPCIBusId(out, len, device) != hipSuccess) { (void)hipGetLastError(); return VIS_E_HIP; }
    return VIS_OK;
}

extern "C" int vis_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void vis_default_params(vis_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->nfeatures = 1000; p->nlevels = 8; p->scale_factor = 1.2f; p->edge_threshold = 31; p->patch_size = 31;
    p->fast_threshold = 20; p->ratio = 0.8f; p->n_cells = 49; p->w_size = 752; p->h_size = 480;
    p->sym_mode = VIS_SYM_REFERENCE_EFFECTIVE;
    p->ransac_prob = 0.999; p->ransac_threshold = 1.0; p->ransac_max_iters = 1000; p->ransac_adaptive = 1;
    p->ransac_seed = 0xFFFFFFFFFFFFFFFFULL;
    p->fx = 458.654; p->fy = 457.296; p->cx = 367.215; p->cy = 248.375;     // calibrationEUROC.xml:20
    p->f2f_iters = 1000; p->f2f_threshold = 370.0;
    p->pose_input = VIS_POSE_GOOD;
}

// why: what vis_last_error says of a refusal whose reason is not obvious from the header's ranges (left alone otherwise)
static int validate_params(const vis_params& p, std::string& why) {
    if (p.nfeatures < 1 || p.nlevels < 1 || p.nlevels > VIS_MAX_LEVELS) return VIS_E_INVALID;
    if (!(p.scale_factor > 1.0f) || p.scale_factor > 3.0f) return VIS_E_INVALID;   // k_resize fetches a 12-byte source window per 4 outputs
    if (p.patch_size != 31) return VIS_E_INVALID;                 // the rBRIEF pattern is learned for 31x31
    if (p.edge_threshold < 22 || p.edge_threshold > 255) return VIS_E_INVALID;   // 43x43 raw patch must stay inside
    if (p.fast_threshold < 1 || p.fast_threshold > 254) return VIS_E_INVALID;
    if (p.n_cells < 1 || p.w_size < 1 || p.h_size < 1) return VIS_E_INVALID;
    // bestMatchesFilter's grid is floor(sqrt(n_cells)) squared; the filter kernel holds at most VIS_MAX_GRID_ROOT^2 cells.  A larger root
    // is refused, not clamped: a clamped grid is another grid (other cell sizes, other survivors), and nothing would tell the caller
    if ((int)std::floor(std::sqrt((double)p.n_cells)) > VIS_MAX_GRID_ROOT) {
        why = "vis_set_params: n_cells " + std::to_string(p.n_cells) + ": floor(sqrt(n_cells)) must not exceed VIS_MAX_GRID_ROOT = " +
              std::to_string((int)VIS_MAX_GRID_ROOT) + " (n_cells <= " + std::to_string((VIS_MAX_GRID_ROOT + 1) * (VIS_MAX_GRID_ROOT + 1) - 1) + ")";
        return VIS_E_INVALID;
    }
    if (p.sym_mode != VIS_SYM_REFERENCE_EFFECTIVE && p.sym_mode != VIS_SYM_INTENDED) {
        why = "vis_set_params: sym_mode " + std::to_string(p.sym_mode) + " is none of VIS_SYM_*"; return VIS_E_INVALID;
    }
    if (p.ransac_max_iters < 1 || p.ransac_max_iters > 100000) return VIS_E_INVALID;
    if (!(p.ransac_prob > 0 && p.ransac_prob < 1) || !(p.fx > 0) || !(p.fy > 0)) return VIS_E_INVALID;
    // the essential RANSAC compares a float Sampson error with (float)((ransac_threshold / fx)^2) and the scorer takes the float above it:
    // both must be ordinary floats.  0 and NaN accept nothing (the reference then returns no model after max_iters iterations), +inf accepts
    // every correspondence under the first model, a negative value is squared into its positive twin: none of them is an estimate anybody asked
    // for, all are refused.  (f2f_threshold is compared as written, `error < threshold` in double: every double is taken, see the header.)
    {
        const double t = p.ransac_threshold / p.fx;
        if (!(t >= 1e-18 && t <= 1e18)) {
            why = "vis_set_params: ransac_threshold / fx must lie in [1e-18, 1e18] (finite and positive)"; return VIS_E_INVALID;
        }
    }
    if (p.f2f_iters < 0) return VIS_E_INVALID;
    if (p.pose_input != VIS_POSE_GOOD && p.pose_input != VIS_POSE_SYM) return VIS_E_INVALID;
    if (p.keypoint_capacity < 0 || p.keypoint_capacity > 65535) return VIS_E_INVALID;
    if (p.keyframe_min_points < 0 || p.keyframe_min_points > 65535) return VIS_E_INVALID;
    return VIS_OK;
}

// the context's ordering events (vis_internal.h, vis_ctx) and their flags: vis_create and vis_destroy walk this one list
template <class F> static void ordering_events(vis_ctx* ctx, F f) {
    const unsigned dt = hipEventDisableTiming;
    f(ctx->ev_filter_done, dt); f(ctx->ev_detect_done, dt); f(ctx->ev_update_fork, dt); f(ctx->ev_update_done, dt); f(ctx->ev_align_fork, dt);
    f(ctx->ev_pose_done, hipEventDefault); f(ctx->ev_pose_start, hipEventDefault); f(ctx->ev_match_start, hipEventDefault);   // (also time the stages)
    for (int i = 0; i < VIS_BATCH_SETS; i++) f(ctx->ev_match_done[i], dt);
    for (int i = 0; i < 2; i++) { f(ctx->ev_pose_done_set[i], dt); f(ctx->ev_results_done_set[i], dt); f(ctx->ev_align_done[i], dt); f(ctx->ev_tri_done[i], dt); f(ctx->ev_epi_done[i], dt); }
}

extern "C" int vis_create(int device, vis_ctx** out) {
    if (!out) return VIS_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VIS_E_NODEVICE;
    if (device < 0 || device >= n) return VIS_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return VIS_E_HIP;
    vis_ctx* ctx = new (std::nothrow) vis_ctx();
    if (!ctx) return VIS_E_NOMEM;
    ctx->device = device;
    vis_default_params(&ctx->p);
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    for (int i = 0; i < VIS_NSLOTS; i++) ctx->slot_valid[i] = 0;
    // Stream priorities of the batch pipeline.  Rounds 2-4: detect chain high, everything beside it low.  Round 5: with the streaming k_fast the
    // low-priority matcher / pose queues hardly got a turn (k_knn_mfma 1.4 ms of wall clock for 0.29 ms of work) and the detect stream ended
    // up waiting for them at the start of every chain; matcher and pose at the detect stream's priority: 397.1 k -> 402.7 k frames/s (three
    // alternations on one box; all four equal: 402.5 k).  Camera::Update's streaming side stream stays low.
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);            // lo = numerically largest = least urgent
    if (hipStreamCreateWithPriority(&ctx->own_stream, hipStreamNonBlocking, prio_hi) != hipSuccess) { delete ctx; return VIS_E_HIP; }
    ctx->stream = ctx->own_stream;
    const int prio_pose = prio_hi, prio_match = prio_hi;
    bool ok = hipStreamCreateWithPriority(&ctx->pose_stream, hipStreamNonBlocking, prio_pose) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->match_stream, hipStreamNonBlocking, prio_match) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->update_stream, hipStreamNonBlocking, prio_lo) == hipSuccess;
    ordering_events(ctx, [&](hipEvent_t& e, unsigned flags) { ok = ok && hipEventCreateWithFlags(&e, flags) == hipSuccess; });
    if (!ok) { delete ctx; return VIS_E_HIP; }
    ctx->ev_ok = true;
    for (int i = 0; i < 12; i++) if (hipEventCreate(&ctx->ev[i]) != hipSuccess) ctx->ev_ok = false;
    *out = ctx;
    return VIS_OK;
}

extern "C" void vis_destroy(vis_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->match_stream) (void)hipStreamSynchronize(ctx->match_stream);
    if (ctx->pose_stream) (void)hipStreamSynchronize(ctx->pose_stream);
    plan_destroy(ctx->single); plan_destroy(ctx->batch);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    for (const DevBlock* b : {&ctx->ess_ws, &ctx->ft_ws, &ctx->sl_ws, &ctx->tjr_ws, &ctx->imu_ws, &ctx->imuj_ws, &ctx->imuc_ws, &ctx->kfdb_ws}) if (b->p) (void)hipFree(b->p);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->d_sample_table) (void)hipFree(ctx->d_sample_table);
    for (int i = 0; i < 12; i++) (void)hipEventDestroy(ctx->ev[i]);
    for (hipStream_t st : {ctx->pose_stream, ctx->match_stream, ctx->update_stream})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    ordering_events(ctx, [](hipEvent_t& e, unsigned) { if (e) (void)hipEventDestroy(e); });
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

// every stream of the context has been synchronised: no reader of any buffer set is pending any more
static void clear_pending(vis_ctx* ctx) {
    ctx->pose_pending = false;
    ctx->align[0] = ctx->align[1] = vis_ctx::AlignRead{};
    if (Plan* pl = ctx->batch) {
        for (Plan::RecordSet& r : pl->rec) { r.matcher.clear(); r.links.clear(); }
        for (Plan::GradSet& g : pl->grad) g.readers.clear();
        for (Plan::MatchOut& o : pl->mo) o.readers.clear();
    }
}

static void sync_all(vis_ctx* ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->update_stream) (void)hipStreamSynchronize(ctx->update_stream);      // (joined by the detect stream in vis_batch_run -- unless that call failed half way, or the caller swapped ctx->stream since)
    if (ctx->match_stream) (void)hipStreamSynchronize(ctx->match_stream);
    if (ctx->pose_stream) (void)hipStreamSynchronize(ctx->pose_stream);
    clear_pending(ctx);
}

extern "C" const char* vis_last_error(vis_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// the fields that fix the per-record layout (keypoint capacity per level, descriptor pattern)
static bool same_record_geometry(const vis_params& a, const vis_params& b) {
    return a.nfeatures == b.nfeatures && a.nlevels == b.nlevels && a.scale_factor == b.scale_factor &&
           a.edge_threshold == b.edge_threshold && a.patch_size == b.patch_size && a.keypoint_capacity == b.keypoint_capacity;
}

extern "C" int vis_set_params(vis_ctx* ctx, const vis_params* p) {
    if (!ctx || !p) return VIS_E_INVALID;
    std::string why;
    int rc = validate_params(*p, why);
    if (rc) { if (!why.empty()) ctx->err = why; return rc; }
    sync_all(ctx);
    // The reference changes matcher / pose settings while its keyframes keep their keypoints and descriptors
    // (Matcher::setImageDimensions, computeBestMatches(n_cells)): when only such fields change, the device slots of the
    // single-frame API survive -- the records move into the re-created plan.  A change of the detector geometry drops them
    // (vis_bf_knn2_hamming / vis_good_matches on a dropped slot return VIS_E_STATE, never stale data).
    Plan* old = ctx->single;
    const bool keep = old && same_record_geometry(ctx->p, *p);
    ctx->p = *p;
    plan_destroy(ctx->batch); ctx->batch = nullptr;
    ctx->single = nullptr;
    // the cv::RNG sample table of the frame-at-a-time pose entry points, for every M they take from the table (<= VIS_POSE_TABLE_M): built
    // HERE, where parameters change, not inside the first vis_essential_ransac whose correspondence count exceeds the last one's (round 5's
    // single_frame_api leg: one call of 200 took 57 ms -- a table freed, rebuilt and re-uploaded when M grew from 33 to 39 -- against a
    // p50 of 0.14 ms).  A failure here is not fatal: the entry point asks again.
    (void)hipSetDevice(ctx->device);
    (void)vis_build_sample_table(ctx, VIS_POSE_TABLE_M);
    if (keep) {
        Plan* np = nullptr;
        rc = plan_create(ctx, old->w, old->h, old->stride, 1, VIS_NSLOTS, 1, &np);
        if (rc == VIS_OK && np->kcap == old->kcap && np->nrec == old->nrec) {
            std::swap(np->d_kps, old->d_kps); std::swap(np->d_desc, old->d_desc);
            std::swap(np->d_nkp, old->d_nkp); std::swap(np->d_descx, old->d_descx);
            ctx->single = np;
            plan_destroy(old);
            return VIS_OK;
        }
        plan_destroy(np);
        // the parameters are set, but the keyframe slots could not be carried over: say so (callers that rely on the slots see
        // VIS_E_STATE from the next matcher call; the reason is here)
        ctx->err = std::string("vis_set_params: keyframe slots dropped, re-planning failed (") + vis_strerror(rc) + ")" + (ctx->err.empty() ? "" : ": " + ctx->err);
    }
    plan_destroy(old);
    for (int i = 0; i < VIS_NSLOTS; i++) ctx->slot_valid[i] = 0;
    return VIS_OK;
}

extern "C" int vis_get_params(vis_ctx* ctx, vis_params* p) {
    if (!ctx || !p) return VIS_E_INVALID;
    *p = ctx->p;
    return VIS_OK;
}

extern "C" int vis_set_stream(vis_ctx* ctx, void* s) {
    if (!ctx) return VIS_E_INVALID;
    sync_all(ctx);
    ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
    return VIS_OK;
}

extern "C" int vis_last_timings(vis_ctx* ctx, vis_timings* t) {
    if (!ctx || !t) return VIS_E_INVALID;
    *t = ctx->tm;
    return VIS_OK;
}

extern "C" int vis_level_geometry(vis_ctx* ctx, int w, int h, int32_t* widths, int32_t* heights,
                                  float* scales, int32_t* quotas) {
    if (!ctx) return VIS_E_INVALID;
    LevelInfo lv[VIS_MAX_LEVELS];
    int rc = vis_compute_levels(ctx->p, w, h, w, lv);
    if (rc) return rc;
    for (int l = 0; l < ctx->p.nlevels; l++) {
        if (widths) widths[l] = lv[l].w;
        if (heights) heights[l] = lv[l].h;
        if (scales) scales[l] = lv[l].scale;
        if (quotas) quotas[l] = lv[l].quota;
    }
    return VIS_OK;
}

// ------------------------------------------------------------------------------------------------ plans
template <class T> static int dalloc(vis_ctx* ctx, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    HIPCHK(ctx, hipMalloc((void**)p, count * sizeof(T)));
    return VIS_OK;
}
#define DALLOC(ptr, count) do { int rc_ = dalloc(ctx, &(ptr), (count)); if (rc_) return rc_; } while (0)

void plan_destroy(Plan* pl) {
    if (!pl) return;
    auto F = [](void* p) { if (p) (void)hipFree(p); };
    F(pl->d_stage);
    for (int l = 0; l < VIS_MAX_LEVELS; l++) {
        F(pl->d_pyr[l]); F(pl->d_rs_tab[l]);
        F(pl->d_cand[l]); F(pl->d_seg_kp[l]);
    }
    F(pl->d_fast_tiles); F(pl->d_tile_cnt); F(pl->d_seg_cnt); F(pl->d_flags); F(pl->d_angle_tab); for (Plan::GradSet& g : pl->grad) { F(g.half); F(g.gx); F(g.gy); F(g.g); } F(pl->d_tau); F(pl->d_seg_cut); F(pl->d_fix);
    F(pl->d_kps); F(pl->d_desc); F(pl->d_nkp); F(pl->d_descx); F(pl->d_warp); F(pl->d_pnp_ws); F(pl->d_ft_ws); F(pl->d_tj_ws); F(pl->d_imu_ws); F(pl->d_imuj_ws); F(pl->d_imuc_ws); F(pl->d_via_ws); F(pl->d_viab_ws);
    for (Plan::RecordSet& r : pl->rec) { F(r.pq); F(r.pt); F(r.pqn); F(r.gq); F(r.kf_link); }
    F(pl->d_kf_state);
    F(pl->snap.gray); F(pl->d_track_state);
    F(pl->d_knn12); F(pl->d_knn21);
    for (Plan::MatchOut& o : pl->mo) { F(o.sym); F(o.nsym); F(o.good); F(o.ngood); F(o.p1); F(o.p2); }
    F(pl->d_hf); F(pl->d_wf);
    F(pl->d_n1); F(pl->d_n2); F(pl->d_mask); F(pl->d_samples); F(pl->d_models); F(pl->d_counts); F(pl->d_rstate); F(pl->d_pose); F(pl->d_worklist); F(pl->d_hyp);
    delete pl;
}

// plan_create's body: any failure returns, and plan_create frees whatever was allocated
static int plan_fill(vis_ctx* ctx, Plan* pl, int w, int h, int stride, int B, int nrec, int npairs, int nsets) {
    pl->w = w; pl->h = h; pl->stride = stride; pl->B = B; pl->L = ctx->p.nlevels; pl->npairs = npairs;
    pl->nsets = nsets; pl->rec_per_set = nrec; nrec *= nsets; pl->nrec = nrec;
    // k_fast segment height: a wave marches 8 fs_nch - 2 emitting rows.  Long segments amortise the prologue and the halo rows of a wave --
    // right for a batch, whose tens of thousands of waves fill the chip anyway; ONE frame has 68 such waves for 256 CUs and the kernel's
    // latency is a wave's lifetime, so the single-frame plan (and small batches) cut the same frame into more, shorter waves
    pl->fs_nch = B >= 32 ? VIS_FS_NCH : (B >= 8 ? 4 : 2);
    int rc = vis_compute_levels(ctx->p, w, h, stride, pl->lv, pl->fs_nch);
    if (rc) return rc;
    const int L = pl->L;
    int kcap = 0; for (int l = 0; l < L; l++) kcap += pl->lv[l].quota + pl->lv[l].quota / 8 + 32;      // default: every level's own slack
    kcap = std::max(kcap, ctx->p.keypoint_capacity);             // (the levels' keep_cap share whatever the caller asked for beyond it)
    if (kcap > 65535) return VIS_E_INVALID;                      // packed 16-bit indices in the matcher
    pl->kcap = kcap;
    std::vector<float> hf, wf; vis_grid_limits(ctx->p, &pl->root, hf, wf);
    const int ncell = pl->root * pl->root;
    // correspondences per pair the pose stage sees: the grid-filtered good matches (reference pipeline) or every symmetric match
    const int mcap = ctx->p.pose_input == VIS_POSE_SYM ? kcap : ncell;
    if (mcap > VIS_RANSAC_MAX_M) return VIS_E_INVALID;
    pl->pose_mcap = mcap;
    pl->max_iters = ctx->p.ransac_max_iters;
    DALLOC(pl->d_stage, (size_t)stride * h);
    for (int l = 1; l < L; l++) {
        const LevelInfo& V = pl->lv[l];
        DALLOC(pl->d_pyr[l], V.frame_bytes * B);
    }
    for (int l = 0; l < L; l++) {
        DALLOC(pl->d_cand[l], (size_t)pl->lv[l].cand_cap * B);
        DALLOC(pl->d_seg_kp[l], (size_t)pl->lv[l].keep_cap * B);
    }
    pl->total_tiles = pl->lv[L - 1].tile_base + pl->lv[L - 1].tiles_x * pl->lv[L - 1].tiles_y;
    DALLOC(pl->d_tile_cnt, (size_t)B * pl->total_tiles); DALLOC(pl->d_seg_cnt, (size_t)B * L + VIS_MAX_LEVELS);   // + padding: k_describe reads VIS_MAX_LEVELS counts per frame
    if (pl->total_tiles > 65535) return VIS_E_INVALID;          // k_fast: gridDim.y
    rc = build_fast_tiles(ctx, pl);
    if (rc) return rc;
    if (nsets > 1) {                                               // batched stream plans predict the FAST threshold from batch to batch
        pl->speculate = true;
        DALLOC(pl->d_tau, L); DALLOC(pl->d_seg_cut, (size_t)B * L); DALLOC(pl->d_fix, (size_t)B * L + 1);
        std::vector<int32_t> t0((size_t)L, ctx->p.fast_threshold);
        HIPCHK(ctx, hipMemcpy(pl->d_tau, t0.data(), (size_t)L * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemset(pl->d_fix, 0, ((size_t)B * L + 1) * 4));
    }
    DALLOC(pl->d_flags, 4);
    HIPCHK(ctx, hipMemset(pl->d_flags, 0, 16));
    DALLOC(pl->d_kps, (size_t)nrec * kcap); DALLOC(pl->d_desc, (size_t)nrec * kcap * 32); DALLOC(pl->d_nkp, nrec);
    HIPCHK(ctx, hipMemset(pl->d_nkp, 0, (size_t)nrec * 4));
    HIPCHK(ctx, hipMemset(pl->d_desc, 0, (size_t)nrec * kcap * 32));
    DALLOC(pl->d_descx, (size_t)nrec * kcap * 128);
    for (int sidx = 0; sidx < nsets; sidx++) {
        Plan::RecordSet& r = pl->rec[sidx];
        DALLOC(r.pq, npairs); DALLOC(r.pt, npairs); DALLOC(r.pqn, npairs);
        const int base = sidx * pl->rec_per_set;
        std::vector<int32_t> q(npairs), t(npairs), qn(npairs);
        for (int i = 0; i < npairs; i++) { q[i] = base + i; t[i] = base + i + 1; qn[i] = i == 0 ? -1 : base + i; }
        HIPCHK(ctx, hipMemcpy(r.pq, q.data(), (size_t)npairs * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(r.pt, t.data(), (size_t)npairs * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(r.pqn, qn.data(), (size_t)npairs * 4, hipMemcpyHostToDevice));
    }
    pl->d_pair_q = pl->rec[0].pq; pl->d_pair_t = pl->rec[0].pt;
    if (nsets > 1 && ctx->p.keyframe_min_points > 0) {             // keyframe gate of a batched stream (keyframe.hip): tables written on the device
        pl->kf_min = ctx->p.keyframe_min_points;
        for (int sidx = 0; sidx < nsets; sidx++) {
            Plan::RecordSet& r = pl->rec[sidx];
            DALLOC(r.gq, npairs); DALLOC(r.kf_link, npairs);
            HIPCHK(ctx, hipMemset(r.gq, 0xFF, (size_t)npairs * 4));       // -1: no pair until a run has written the set
            HIPCHK(ctx, hipMemset(r.kf_link, 0xFF, (size_t)npairs * 4));
        }
        DALLOC(pl->d_kf_state, 2);
        rc = reset_keyframe_state(ctx, pl);
        if (rc) return rc;
    }
    DALLOC(pl->d_knn12, (size_t)npairs * kcap * 2); DALLOC(pl->d_knn21, (size_t)npairs * kcap * 2);
    for (int s_ = 0; s_ < (nsets > 1 ? 2 : 1); s_++) {              // the matcher-output sets (vis_internal.h): two for plans that pipeline steps
        Plan::MatchOut& o = pl->mo[s_];
        DALLOC(o.sym, (size_t)npairs * kcap); DALLOC(o.nsym, npairs);
        DALLOC(o.good, (size_t)npairs * ncell); DALLOC(o.ngood, npairs);
        DALLOC(o.p1, (size_t)npairs * mcap * 2); DALLOC(o.p2, (size_t)npairs * mcap * 2);
        HIPCHK(ctx, hipMemset(o.nsym, 0, (size_t)npairs * 4));
        HIPCHK(ctx, hipMemset(o.ngood, 0, (size_t)npairs * 4));
        HIPCHK(ctx, hipMemset(o.p1, 0, (size_t)npairs * mcap * 2 * sizeof(float)));
        HIPCHK(ctx, hipMemset(o.p2, 0, (size_t)npairs * mcap * 2 * sizeof(float)));
    }
    DALLOC(pl->d_hf, pl->root); DALLOC(pl->d_wf, pl->root);
    HIPCHK(ctx, hipMemcpy(pl->d_hf, hf.data(), (size_t)pl->root * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(pl->d_wf, wf.data(), (size_t)pl->root * 4, hipMemcpyHostToDevice));
    DALLOC(pl->d_n1, (size_t)npairs * mcap * 2); DALLOC(pl->d_n2, (size_t)npairs * mcap * 2);
    DALLOC(pl->d_mask, (size_t)npairs * mcap);
    DALLOC(pl->d_samples, (size_t)npairs * pl->max_iters * 5);
    DALLOC(pl->d_models, (size_t)npairs * pl->max_iters * 90);
    DALLOC(pl->d_counts, (size_t)npairs * pl->max_iters * 10);
    DALLOC(pl->d_rstate, (size_t)npairs * VIS_RSTATE_WORDS);
    DALLOC(pl->d_pose, npairs);
    DALLOC(pl->d_worklist, (size_t)npairs + 2);        // count, pairs, k_hyp_roots_packed item counter
    DALLOC(pl->d_hyp, (size_t)npairs * pl->max_iters * VIS_HYP_DOUBLES);
    // defence in depth: nothing should read these before writing them, but a recycled allocation must never
    // turn a missed guard into an out-of-bounds index (see the inactive-lane fix in k_ransac_hyp)
    HIPCHK(ctx, hipMemset(pl->d_samples, 0, (size_t)npairs * pl->max_iters * 5 * sizeof(int32_t)));
    HIPCHK(ctx, hipMemset(pl->d_counts, 0xFF, (size_t)npairs * pl->max_iters * 10 * sizeof(int32_t)));
    HIPCHK(ctx, hipMemset(pl->d_rstate, 0, (size_t)npairs * VIS_RSTATE_WORDS * sizeof(int32_t)));
    HIPCHK(ctx, hipMemset(pl->d_worklist, 0, ((size_t)npairs + 2) * sizeof(int32_t)));
    HIPCHK(ctx, hipMemset(pl->d_knn12, 0xFF, (size_t)npairs * kcap * 2 * sizeof(uint32_t)));
    HIPCHK(ctx, hipMemset(pl->d_knn21, 0xFF, (size_t)npairs * kcap * 2 * sizeof(uint32_t)));
    HIPCHK(ctx, hipMemset(pl->d_pose, 0, (size_t)npairs * sizeof(PoseOut)));
    // cv::RNG sample tables only for small M (the reference pipeline: M <= root^2); larger M replays the stream on the device
    return vis_build_sample_table(ctx, std::min(mcap, 8192));
}

int plan_create(vis_ctx* ctx, int w, int h, int stride, int B, int nrec, int npairs, Plan** out, int nsets) {
    *out = nullptr;
    if (B < 1 || nrec < 1 || npairs < 1 || stride < w || (stride & 3)) return VIS_E_INVALID;
    Plan* pl = new (std::nothrow) Plan();
    if (!pl) return VIS_E_NOMEM;
    const int rc = plan_fill(ctx, pl, w, h, stride, B, nrec, npairs, nsets);
    if (rc) { plan_destroy(pl); return rc; }
    *out = pl;
    return VIS_OK;
}

// cv::RNG((uint64)seed) + getSubset replayed on the host for every M in [6, max_m]: the RANSAC sample
// stream depends only on (seed, M), so the per-pair sequential RNG walk is replaced by a table row.
int vis_build_sample_table(vis_ctx* ctx, int max_m) {
    const int iters = ctx->p.ransac_max_iters;
    // as many rows as fit in 256 MB (2000 iterations: M <= 6715, i.e. config 3's ~3100 symmetric matches come from the table; pairs with
    // more correspondences than the table has rows replay the stream on the device, one thread per pair: 0.43 ms at M = 3100)
    max_m = (int)std::min<size_t>((size_t)max_m, 5 + ((size_t)256 << 20) / ((size_t)std::max(iters, 1) * 20));
    if (ctx->d_sample_table && ctx->sample_max_m >= max_m && ctx->sample_iters == iters && ctx->sample_seed == ctx->p.ransac_seed) return VIS_OK;
    if (ctx->d_sample_table) { sync_all(ctx); (void)hipFree(ctx->d_sample_table); ctx->d_sample_table = nullptr; ctx->sample_max_m = 0; }
    if (max_m < 6) return VIS_OK;                                  // no table: device replay
    std::vector<int32_t> tab;                                      // up to 256 MB of host memory: an allocation failure is an error code, not an exception across the C ABI
    try { tab.resize((size_t)(max_m - 5) * iters * 5); } catch (...) { ctx->err = "sample table: host allocation failed"; return VIS_E_NOMEM; }
    for (int M = 6; M <= max_m; M++) {
        unsigned long long state = ctx->p.ransac_seed ? ctx->p.ransac_seed : 0xffffffffULL;
        int32_t* dst = tab.data() + (size_t)(M - 6) * iters * 5;
        for (int it = 0; it < iters; it++) {
            int idx[5];
            for (int i = 0; i < 5; i++) {
                for (;;) {
                    state = (unsigned long long)(unsigned)state * 4164903690ULL + (unsigned)(state >> 32);   // RNG::next
                    const int v = idx[i] = (int)((unsigned)state % (unsigned)M);                               // uniform(0, M)
                    int j = 0;
                    for (; j < i; j++) if (v == idx[j]) break;
                    if (j == i) break;
                }
            }
            for (int k = 0; k < 5; k++) dst[5 * it + k] = idx[k];
        }
    }
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_sample_table, tab.size() * 4));
    HIPCHK(ctx, hipMemcpy(ctx->d_sample_table, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    ctx->sample_max_m = max_m; ctx->sample_iters = iters; ctx->sample_seed = ctx->p.ransac_seed;
    return VIS_OK;
}

int launch_pose(vis_ctx* ctx, Plan* pl, int npairs) {
    if (npairs <= 0) return VIS_OK;
    return pose_run(ctx, npairs, pl->pose_mcap, pl->max_iters, pl->out().p1, pl->out().p2,
                    ctx->p.pose_input == VIS_POSE_SYM ? pl->out().nsym : pl->out().ngood, pl->d_n1, pl->d_n2,
                    pl->d_samples, pl->d_models, pl->d_counts, pl->d_rstate, nullptr, pl->d_mask, pl->d_pose, 1, 1, pl->d_worklist, pl->d_hyp);
}

// grow-only scratch of the host-pointer entry points.  Every stream of the context is drained before the old block is
// freed: batch work queued on the matcher / pose streams may still read buffers carved from it.
int vis_ensure_scratch(vis_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->scratch_bytes) return VIS_OK;
    sync_all(ctx);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    ctx->d_scratch = nullptr; ctx->scratch_bytes = 0;
    HIPCHK(ctx, hipMalloc(&ctx->d_scratch, bytes));
    ctx->scratch_bytes = bytes;
    return VIS_OK;
}
// the grow rule of the device-rows workspaces (vis_internal.h)
int vis_grow_block(vis_ctx* ctx, DevBlock& b, size_t bytes, const char* who, bool* replaced) {
    if (replaced) *replaced = false;
    if (bytes <= b.bytes) return VIS_OK;
    sync_all(ctx);                                                 // work queued on any stream may still use the old block
    if (b.p) (void)hipFree(b.p);
    b = DevBlock{};
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError(); b.p = nullptr;
        ctx->err = std::string(who) + ": out of device memory for the workspace"; return VIS_E_NOMEM;
    }
    b.bytes = bytes;
    if (replaced) *replaced = true;
    return VIS_OK;
}

std::atomic<unsigned long long> vis_g_launches{0};

// ---- host staging of the single-frame entry points --------------------------------------------------------------------------------
// The reference's main hands over pageable host memory (cv::Mat, std::vector) once per camera frame (src/main_vi_slamGPU.cpp:118-123).  A
// blocking hipMemcpy on such memory is a full host <-> device round trip each; round 4's vis_orb_detect_compute made four of them, the
// matcher entry six.  Here every transfer of a call goes through the context's pinned block as an ASYNCHRONOUS copy on the context's
// stream -- uploads are copied into the block first, downloads are copied out of it after the call's ONE wait -- so an entry point blocks
// once (twice when a result decides what else to fetch).
int vis_ensure_pin(vis_ctx* ctx, size_t bytes) {
    if (ctx->h_pin_bytes >= bytes) return VIS_OK;
    if (ctx->stage_live > 0) { ctx->err = "staging block would be replaced under a live HostStage (internal: size the block before building the stage)"; return VIS_E_STATE; }
    (void)hipStreamSynchronize(ctx->stream);                       // nothing queued may still use the old block
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    ctx->h_pin = nullptr; ctx->h_pin_bytes = 0; ctx->h_pin_dev = nullptr;
    const size_t want = std::max(bytes + bytes / 4, (size_t)1 << 20);
    if (hipHostMalloc(&ctx->h_pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->err = "hipHostMalloc of the staging block failed"; return VIS_E_NOMEM; }
    ctx->h_pin_bytes = want;
    if (hipHostGetDevicePointer(&ctx->h_pin_dev, ctx->h_pin, 0) != hipSuccess) { (void)hipGetLastError(); ctx->h_pin_dev = nullptr; }   // (downloads then go through the runtime's copies)
    return VIS_OK;
}
// diagnostics: out[0] = kernel launches of this process, out[1] = times a single-frame entry point of this context blocked on the device,
// out[2] = asynchronous copies it queued (bench.py `single_frame_api`: launches and round trips per frame), out[3] = largest undecided
// list of any pose call of this context (k_hyp_score)
extern "C" int vis_debug_counters(vis_ctx* ctx, unsigned long long out[4]) {
    if (!ctx || !out) return VIS_E_INVALID;
    out[0] = vis_g_launches.load(std::memory_order_relaxed); out[1] = ctx->n_host_waits; out[2] = ctx->n_copies; out[3] = ctx->undecided_max;
    return VIS_OK;
}

// diagnostic: level `level` >= 1 of frame `frame` as the last detection of the chosen plan left it in the plan's pyramid (read only: no
// launch, nothing of the plan changes).  The rows are copied without their stride padding.
extern "C" int vis_debug_pyramid_level(vis_ctx* ctx, int batch, int frame, int level, uint8_t* out, int out_stride) {
    if (!ctx || !out) return VIS_E_INVALID;
    const Plan* pl = batch ? ctx->batch : ctx->single;
    if (!pl || pl->pyr_frames < 1) return VIS_E_STATE;
    if (level < 1 || level >= pl->L || frame < 0 || frame >= pl->pyr_frames) return VIS_E_INVALID;     // (level 0 is the caller's own frame)
    const LevelInfo& V = pl->lv[level];
    if (out_stride < V.w) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy2D(out, (size_t)out_stride, pl->d_pyr[level] + (size_t)frame * V.frame_bytes, (size_t)V.stride, (size_t)V.w, (size_t)V.h,
                            hipMemcpyDeviceToHost));
    return VIS_OK;
}

__global__ void k_set_pair(int32_t* q, int32_t* t, int32_t vq, int32_t vt) { *q = vq; *t = vt; }

static int ensure_single(vis_ctx* ctx, int w, int h) {
    (void)hipSetDevice(ctx->device);
    if (ctx->single && ctx->single->w == w && ctx->single->h == h) return VIS_OK;
    (void)hipStreamSynchronize(ctx->stream);
    plan_destroy(ctx->single); ctx->single = nullptr;
    for (int i = 0; i < VIS_NSLOTS; i++) ctx->slot_valid[i] = 0;
    const int stride = ((w + 63) / 64) * 64;
    return plan_create(ctx, w, h, stride, 1, VIS_NSLOTS, 1, &ctx->single);
}

// re-create the single-frame plan with a larger per-frame keypoint capacity; the valid slots keep their records
static int grow_single(vis_ctx* ctx, int capacity) {
    Plan* old = ctx->single;
    if (!old) return VIS_E_STATE;
    sync_all(ctx);
    const int cap_before = ctx->p.keypoint_capacity;
    ctx->p.keypoint_capacity = capacity;
    Plan* np = nullptr;
    int rc = plan_create(ctx, old->w, old->h, old->stride, 1, VIS_NSLOTS, 1, &np);
    if (rc == VIS_OK && (np->kcap < old->kcap || np->nrec != old->nrec)) { plan_destroy(np); rc = VIS_E_STATE; }
    if (rc) { ctx->p.keypoint_capacity = cap_before; return rc; }       // (the old plan and its slots stay as they were)
    // every failure from here on leaves the context as it was: the new plan is destroyed, the capacity restored (the early
    // returns of HIPCHK leaked `np` and left ctx->p ahead of the live plan)
    auto copy_records = [&]() -> hipError_t {
        std::vector<int32_t> nk((size_t)old->nrec);
        hipError_t e = hipMemcpy(nk.data(), old->d_nkp, nk.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(np->d_nkp, nk.data(), nk.size() * 4, hipMemcpyHostToDevice);
        for (int r = 0; e == hipSuccess && r < old->nrec && r < VIS_NSLOTS; r++) {
            const size_t n = (size_t)std::min(std::max(nk[r], 0), old->kcap);
            if (!ctx->slot_valid[r] || !n) continue;
            e = hipMemcpy(np->d_kps + (size_t)r * np->kcap, old->d_kps + (size_t)r * old->kcap, n * sizeof(vis_keypoint), hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(np->d_desc + (size_t)r * np->kcap * 32, old->d_desc + (size_t)r * old->kcap * 32, n * 32, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(np->d_descx + (size_t)r * np->kcap * 128, old->d_descx + (size_t)r * old->kcap * 128, n * 128, hipMemcpyDeviceToDevice);
        }
        return e;
    };
    const hipError_t ce = copy_records();
    if (ce != hipSuccess) {
        ctx->err = std::string("grow_single: ") + hipGetErrorString(ce);
        plan_destroy(np); ctx->p.keypoint_capacity = cap_before;
        return VIS_E_HIP;
    }
    plan_destroy(old);
    ctx->single = np;
    // a batch plan was sized with the old parameters: it goes (sync_all above has drained its streams; results of a finished batch that
    // the caller has not fetched yet are lost with it -- vis_set_params documents the same for every parameter change)
    plan_destroy(ctx->batch); ctx->batch = nullptr;
    return VIS_OK;
}

static void key_to_dmatch(uint32_t key, int q, vis_dmatch* m) {
    m->queryIdx = q;
    if (key == 0xFFFFFFFFu) { m->trainIdx = -1; m->imgIdx = -1; m->distance = FLT_MAX; }
    else { m->trainIdx = (int)(key & 0xFFFF); m->imgIdx = 0; m->distance = (float)(key >> 16); }
}

static int check_flags(vis_ctx* ctx, Plan* pl) {
    int32_t fl = 0;
    HIPCHK(ctx, hipMemcpy(&fl, pl->d_flags, 4, hipMemcpyDeviceToHost));
    if (fl) {
        ctx->err = "device capacity flag set: " + std::to_string(fl) + ((fl & 12) ? " (more tied keypoints than vis_params.keypoint_capacity holds: " +
                   std::to_string(pl->kcap) + " per frame; raise it)" : "");
        HIPCHK(ctx, hipMemset(pl->d_flags, 0, 4)); return VIS_E_CAPACITY;
    }
    return VIS_OK;
}

// ------------------------------------------------------------------------------------------------ single-frame API
extern "C" int vis_camera_update(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride, uint8_t* const out_levels[5]) {
    if (!ctx) return VIS_E_INVALID;
    if (!img || !out_levels || w < 16 || h < 16 || w > VIS_MAX_SIDE || h > VIS_MAX_SIDE || stride < w) {
        ctx->err = "vis_camera_update: img and out_levels not NULL, 16 <= w, h <= 4095, stride >= w"; return VIS_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    int lw[5], lh[5]; vis_half_dims(w, h, lw, lh);
    size_t lvl_bytes[5];
    for (int l = 0; l < 5; l++) lvl_bytes[l] = (size_t)lw[l] * lh[l];
    uint8_t* d[5];
    int rc = vis_carve(ctx, [&](Carver& cv) { for (int l = 0; l < 5; l++) d[l] = cv.take<uint8_t>(lvl_bytes[l]); }, 2);   // (d[0] goes up and may come down)
    if (rc) return rc;
    HostStage hs(ctx);
    hs.up2d(d[0], w, img, stride, w, h);
    hs.flush_ups();
    rc = launch_half_pyramid(ctx, d[0], w, h, w, d);
    if (rc) return vis_drain(ctx, rc);
    const void* got[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < 5; l++) if (out_levels[l]) got[l] = hs.down(d[l], lvl_bytes[l]);
    rc = hs.wait();
    if (rc) return rc;
    for (int l = 0; l < 5; l++) if (out_levels[l]) std::memcpy(out_levels[l], got[l], lvl_bytes[l]);
    return VIS_OK;
}

extern "C" size_t vis_gradient_frame_elems(int w, int h) { return (w < 16 || h < 16 || w > VIS_MAX_SIDE || h > VIS_MAX_SIDE) ? 0 : vis_grad_frame_elems(w, h); }
extern "C" void vis_half_pyramid_dims(int w, int h, int32_t lw[5], int32_t lh[5]) { if (lw && lh) vis_half_dims(w, h, lw, lh); }

extern "C" int vis_gradient_batch(vis_ctx* ctx, const uint8_t* d_frames, int w, int h, int stride, int n, int scale,
                                  uint8_t* d_gray, int16_t* d_gx, int16_t* d_gy, uint8_t* d_g) {
    if (!ctx || !d_frames || !d_gray || !d_gx || !d_gy || !d_g) return VIS_E_INVALID;
    if (w < 16 || h < 16 || w > VIS_MAX_SIDE || h > VIS_MAX_SIDE || stride < w || (stride & 3) || n < 1 || scale < 1 || scale > 8) {
        ctx->err = "vis_gradient_batch: 16 <= w, h <= 4095, stride >= w and % 4 == 0, n >= 1, 1 <= scale <= 8"; return VIS_E_INVALID;
    }
    if (((uintptr_t)d_gx | (uintptr_t)d_gy | (uintptr_t)d_g | (uintptr_t)d_gray) & 15) { ctx->err = "vis_gradient_batch: output buffers must be 16-byte aligned"; return VIS_E_INVALID; }
    (void)hipSetDevice(ctx->device);
    // a vis_batch_align still in flight on the pose stream reads the previous gradients (usually these very buffers)
    HIPCHK(ctx, wait_align_readers(ctx, ctx->stream));
    const size_t frame_bytes = (size_t)stride * h;
    int rc = launch_half_pyramid_batch(ctx, d_frames, w, h, stride, frame_bytes, n, d_gray);
    if (rc) return rc;
    return launch_gradient(ctx, d_frames, w, h, stride, frame_bytes, n, d_gray, scale, d_gx, d_gy, d_g);
}

extern "C" int vis_compute_gradient(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride, int scale,
                                    int16_t* const gx[5], int16_t* const gy[5], uint8_t* const g[5]) {
    if (!ctx) return VIS_E_INVALID;
    if (!img || !gx || !gy || !g || w < 16 || h < 16 || w > VIS_MAX_SIDE || h > VIS_MAX_SIDE || stride < w || scale < 1 || scale > 8) {
        ctx->err = "vis_compute_gradient: img, gx, gy and g not NULL, 16 <= w, h <= 4095, stride >= w, 1 <= scale <= 8"; return VIS_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    const size_t fe = vis_grad_frame_elems(w, h);
    const int ws = (w + 15) & ~15;                              // device row stride of the copy (the batched entry wants % 4 == 0)
    uint8_t *d_img, *d_gray, *d_g; int16_t *d_gx, *d_gy;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_img = cv.take<uint8_t>((size_t)ws * h);
        d_gray = cv.take<uint8_t>(fe);
        d_gx = cv.take<int16_t>(fe); d_gy = cv.take<int16_t>(fe);
        d_g = cv.take<uint8_t>(fe);
    });
    if (rc) return rc;
    HostStage hs(ctx);
    hs.up2d(d_img, ws, img, stride, w, h);
    hs.flush_ups();
    rc = vis_gradient_batch(ctx, d_img, w, h, ws, 1, scale, d_gray, d_gx, d_gy, d_g);
    if (rc) return vis_drain(ctx, rc);
    int lw[5], lh[5]; vis_half_dims(w, h, lw, lh);
    // the three outputs are dense over the five levels: one copy each, cut into levels on the host
    const int16_t* h_gx = (const int16_t*)hs.down(d_gx, fe * 2);
    const int16_t* h_gy = (const int16_t*)hs.down(d_gy, fe * 2);
    const uint8_t* h_g = (const uint8_t*)hs.down(d_g, fe);
    rc = hs.wait();
    if (rc) return rc;
    size_t off = 0;
    for (int l = 0; l < 5; l++) {
        const size_t cnt = (size_t)lw[l] * lh[l];
        if (gx[l]) std::memcpy(gx[l], h_gx + off, cnt * 2);
        if (gy[l]) std::memcpy(gy[l], h_gy + off, cnt * 2);
        if (g[l]) std::memcpy(g[l], h_g + off, cnt);
        off += cnt;
    }
    return VIS_OK;
}

extern "C" int vis_patch_points(vis_ctx* ctx, const vis_keypoint* good, int n, int cap,
                                float* const patch[5], int n_patch[5], float* const debug[5], int n_debug[5]) {
    if (!ctx || (n > 0 && !good) || n < 0 || cap < 0 || !patch || !debug || !n_patch || !n_debug) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    const int m = std::min(n, 200);
    vis_keypoint* d_good; float *d_patch, *d_debug; int32_t* d_cnt;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_good = cv.take<vis_keypoint>(200);
        d_patch = cv.take<float>((size_t)5 * std::max(cap, 1) * 4);
        d_debug = cv.take<float>((size_t)5 * std::max(cap, 1) * 4);
        d_cnt = cv.take<int32_t>(10);
    }, 2);                                                         // (the two lists come down in five pieces each, one per level)
    if (rc) return rc;
    HostStage hs(ctx);
    hs.up(d_good, good, (size_t)m * sizeof(vis_keypoint));
    hs.flush_ups();
    rc = launch_patch_points(ctx, d_good, m, ctx->p.w_size, ctx->p.h_size, d_patch, d_debug, cap, d_cnt);
    if (rc) return vis_drain(ctx, rc);
    // counts and both point lists of all five levels behind the kernels.  The list lengths are not known before the wait, but their
    // bounds are: min(m, 200) keypoints x at most (2 sp + 2)^2 points of a level's window (sp = 5, 3, 2, 5, 5: k_patch_points) and one
    // debug point per keypoint -- that much of every level is fetched, not the caller's whole capacity (200 x 121 x 16 B x 5 levels x 2
    // lists = 3.9 MB per call for 49 good matches; the GPU main calls this twice per frame)
    const int32_t* cnt = (const int32_t*)hs.down(d_cnt, 40);
    const float* h_patch[5]; const float* h_debug[5]; int bp[5], bd[5];
    const int mk = std::min(m, 200);
    for (int l = 0; l < 5; l++) {
        const int sp = l == 1 ? 3 : (l == 2 ? 2 : 5);
        bp[l] = (int)std::min<long long>(cap, (long long)mk * (2 * sp + 2) * (2 * sp + 2)); bd[l] = std::min(cap, mk);
        h_patch[l] = bp[l] ? (const float*)hs.down(d_patch + (size_t)l * cap * 4, (size_t)bp[l] * 16) : nullptr;
        h_debug[l] = bd[l] ? (const float*)hs.down(d_debug + (size_t)l * cap * 4, (size_t)bd[l] * 16) : nullptr;
    }
    rc = hs.wait();
    if (rc) return rc;
    bool over = false;
    for (int l = 0; l < 5; l++) {
        n_patch[l] = cnt[l]; n_debug[l] = cnt[5 + l];
        over = over || cnt[l] > cap || cnt[5 + l] > cap;
        const int np = std::min(cnt[l], bp[l]), nd = std::min(cnt[5 + l], bd[l]);         // (the bounds hold by construction; never read past what was fetched)
        if (patch[l] && np) std::memcpy(patch[l], h_patch[l], (size_t)np * 16);
        if (debug[l] && nd) std::memcpy(debug[l], h_debug[l], (size_t)nd * 16);
    }
    return over ? VIS_E_CAPACITY : VIS_OK;
}

// elapsed time between two events, false when either was never recorded (a stage that did not run, a sync before the first run).
// The failed query must not stay behind as the thread's "last error": the launch checks (hipGetLastError after a kernel launch)
// would report it for the next, valid, call.
static bool ev_elapsed(float* ms, hipEvent_t a, hipEvent_t b) {
    if (hipEventElapsedTime(ms, a, b) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

static void collect_detect_timings(vis_ctx* ctx) {
    if (!ctx->ev_ok) return;
    float a = 0;
    if (ev_elapsed(&a, ctx->ev[0], ctx->ev[1])) ctx->tm.ms_pyramid = a;
    if (ev_elapsed(&a, ctx->ev[1], ctx->ev[2])) ctx->tm.ms_fast = a;
    if (ev_elapsed(&a, ctx->ev[2], ctx->ev[3])) ctx->tm.ms_select = a;
    if (ev_elapsed(&a, ctx->ev[3], ctx->ev[4])) ctx->tm.ms_describe = a;
}

extern "C" int vis_orb_detect_compute(vis_ctx* ctx, const uint8_t* img, int w, int h, int stride, int frame_slot,
                                      vis_keypoint* kps_out, uint8_t* desc_out, int cap, int* n_out) {
    if (!ctx || !img || !n_out || frame_slot < 0 || frame_slot >= VIS_NSLOTS || stride < w) return VIS_E_INVALID;
    int rc = ensure_single(ctx, w, h);
    if (rc) return rc;
    Plan* pl = ctx->single;
    // everything the call may hand back, fetched behind the detect chain in one go: count, device flags and as many keypoint /
    // descriptor records as the caller can take (the count is not known before the wait; a record set is a few tens of KB)
    const size_t nfetch = (size_t)std::max(0, std::min(cap, pl->kcap));
    rc = vis_ensure_pin(ctx, (size_t)w * h + nfetch * (sizeof(vis_keypoint) + 32) + 4096);
    if (rc) return rc;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    int grow_to = 0;                                               // > 0: more ties than the plan's records hold; grow and detect again (below, once the stage is gone)
    {
        HostStage hs(ctx);
        hs.up2d(pl->d_stage, pl->stride, img, stride, w, h);
        hs.flush_ups();
        if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[0], ctx->stream);
        rc = launch_detect(ctx, pl, pl->d_stage, 1, frame_slot);
        if (rc) return rc;
        const int32_t* h_n = (const int32_t*)hs.down(pl->d_nkp + frame_slot, 4);
        const int32_t* h_fl = (const int32_t*)hs.down(pl->d_flags, 4);
        const void* h_kps = kps_out && nfetch ? hs.down(pl->d_kps + (size_t)frame_slot * pl->kcap, nfetch * sizeof(vis_keypoint)) : nullptr;
        const void* h_desc = desc_out && nfetch ? hs.down(pl->d_desc + (size_t)frame_slot * pl->kcap * 32, nfetch * 32) : nullptr;
        rc = hs.wait();
        if (rc) return rc;
        collect_detect_timings(ctx);
        { float a = 0; if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[0], ctx->ev[4])) ctx->tm.ms_total = a; }
        const int32_t n = *h_n, fl = *h_fl;
        if (fl) {
            // More tied keypoints than the plan's records hold (KeyPointsFilter::retainBest keeps every tie at its cut: a checkerboard)?  The
            // caller's `cap` says how many it is prepared to take: grow the per-frame capacity towards it -- the other slots' records move
            // into the re-created plan -- and detect again.  Only what exceeds `cap` (or 65535) is an error.
            if ((fl & 12) && !(fl & ~12) && cap > pl->kcap && pl->kcap < 65535) grow_to = std::min(65535, std::max(cap, 2 * pl->kcap));
            else {
                rc = check_flags(ctx, pl);                         // (reads and clears the flags: the error path may block again)
                if (rc) return rc;
            }
        }
        if (!grow_to) {
            ctx->slot_valid[frame_slot] = 1;
            *n_out = n;
            if (n > cap && (kps_out || desc_out)) return VIS_E_CAPACITY;
            if (kps_out && n) std::memcpy(kps_out, h_kps, (size_t)n * sizeof(vis_keypoint));
            if (desc_out && n) std::memcpy(desc_out, h_desc, (size_t)n * 32);
            return VIS_OK;
        }
    }
    // The retry runs with NO stage alive: it sizes the staging block for the larger record count, which may replace the block (round 6: the
    // retry used to re-enter this function under the first pass's live stage -- harmless only because that stage was never touched again;
    // vis_ensure_pin now refuses it, tests/test_edge_cases_gpu.py::test_ties_beyond_the_default_slack_are_all_returned on a fresh context)
    HIPCHK(ctx, hipMemset(pl->d_flags, 0, 4));
    rc = grow_single(ctx, grow_to);
    if (rc) return rc;
    return vis_orb_detect_compute(ctx, img, w, h, stride, frame_slot, kps_out, desc_out, cap, n_out);
}

static int set_single_pair(vis_ctx* ctx, Plan* pl, int slot_q, int slot_t) {
    if (!pl) return VIS_E_STATE;
    if (slot_q < 0 || slot_q >= VIS_NSLOTS || slot_t < 0 || slot_t >= VIS_NSLOTS) return VIS_E_INVALID;
    if (!ctx->slot_valid[slot_q] || !ctx->slot_valid[slot_t]) return VIS_E_STATE;
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, ctx->stream, pl->d_pair_q, pl->d_pair_t, (int32_t)slot_q, (int32_t)slot_t);   // (two blocking 4-byte uploads before)
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

static void keys_to_dmatches(const uint32_t* k, int n, vis_dmatch* out) {
    if (!out) return;
    for (int q = 0; q < n; q++) { key_to_dmatch(k[2 * q], q, out + 2 * q); key_to_dmatch(k[2 * q + 1], q, out + 2 * q + 1); }
}

// ---- guided matching: the window of the *_guided entry points (match.hip k_warp, window_admits) ----
int ensure_warp(vis_ctx* ctx, Plan* pl) {
    if (pl->d_warp) return VIS_OK;
    HIPCHK(ctx, hipMalloc((void**)&pl->d_warp, ((size_t)pl->npairs * pl->kcap + 8) * sizeof(float2)));   // + 16 floats: a single-frame call's rotation
    return VIS_OK;
}
// what every guided entry point refuses before it looks at its context; host_rot: rot is host memory, its entries must be finite
static bool guide_args_ok(const float* rot, float radius, bool host_rot) {
    if (!rot || !std::isfinite(radius) || radius < 0.f) return false;
    if (host_rot) for (int i = 0; i < 9; i++) if (!std::isfinite(rot[i])) return false;
    return true;
}
// the single-frame plan's guide: the caller's rotation goes behind the plan's predictions (through the staging block, sized by the caller)
static int single_guide(vis_ctx* ctx, Plan* pl, const float* rot, float radius, MatchGuide* g) {
    int rc = ensure_warp(ctx, pl);
    if (rc) return rc;
    float* d_rot = reinterpret_cast<float*>(pl->d_warp + (size_t)pl->npairs * pl->kcap);
    HostStage up(ctx);
    up.up(d_rot, rot, 36);
    up.flush_ups();
    if (up.overflow || up.err != hipSuccess) { ctx->err = "guided match: staging the rotation failed"; return VIS_E_HIP; }
    g->d_rot = d_rot; g->radius = radius;
    return VIS_OK;
}

// vis_bf_knn2_hamming (rot == nullptr) and vis_bf_knn2_hamming_guided
static int knn2_slots(vis_ctx* ctx, int slot_q, int slot_t, const float* rot, float radius, vis_dmatch* out12, vis_dmatch* out21) {
    (void)hipSetDevice(ctx->device);
    Plan* pl = ctx->single;
    int rc = pl ? vis_ensure_pin(ctx, (size_t)pl->kcap * 16 + 4096) : VIS_E_STATE;
    if (!rc) rc = set_single_pair(ctx, pl, slot_q, slot_t);
    MatchGuide g = {nullptr, 0.f};
    if (!rc && rot) rc = single_guide(ctx, pl, rot, radius, &g);
    if (rc) return rc;
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[4], ctx->stream);
    rc = launch_expand(ctx, pl, slot_q, 1);
    if (!rc && slot_t != slot_q) rc = launch_expand(ctx, pl, slot_t, 1);
    if (!rc) rc = launch_match(ctx, pl, 1, rot ? &g : nullptr);
    if (rc) return rc;
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[5], ctx->stream);
    HostStage hs(ctx);
    const int32_t* h_nq = (const int32_t*)hs.down(pl->d_nkp + slot_q, 4);
    const int32_t* h_nt = (const int32_t*)hs.down(pl->d_nkp + slot_t, 4);
    const uint32_t* h12 = out12 ? (const uint32_t*)hs.down(pl->d_knn12, (size_t)pl->kcap * 8) : nullptr;
    const uint32_t* h21 = out21 ? (const uint32_t*)hs.down(pl->d_knn21, (size_t)pl->kcap * 8) : nullptr;
    rc = hs.wait();
    if (rc) return rc;
    { float a = 0; if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[4], ctx->ev[5])) ctx->tm.ms_knn = a; }
    keys_to_dmatches(h12, std::min(*h_nq, pl->kcap), out12);
    keys_to_dmatches(h21, std::min(*h_nt, pl->kcap), out21);
    return VIS_OK;
}

extern "C" int vis_bf_knn2_hamming(vis_ctx* ctx, int slot_q, int slot_t, vis_dmatch* out12, vis_dmatch* out21) {
    if (!ctx) return VIS_E_INVALID;
    return knn2_slots(ctx, slot_q, slot_t, nullptr, 0.f, out12, out21);
}

extern "C" int vis_bf_knn2_hamming_guided(vis_ctx* ctx, int slot_q, int slot_t, const float rot[9], float radius, vis_dmatch* out12, vis_dmatch* out21) {
    if (!guide_args_ok(rot, radius, true)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    return knn2_slots(ctx, slot_q, slot_t, rot, radius, out12, out21);
}

// One set of keypoints, host pointers: out_xy[2 j ..] = the prediction of kps[j] (k_warp).  Blocks once.
extern "C" int vis_warp_keypoints(vis_ctx* ctx, const vis_keypoint* kps, int n, const float rot[9], float* out_xy) {
    if (n < 0 || !guide_args_ok(rot, 0.f, true) || (n && (!kps || !out_xy))) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    Plan tp; tp.kcap = n;
    float* d_rot; float2* d_xy;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        tp.d_kps = cv.take<vis_keypoint>(n);
        tp.d_nkp = cv.take<int32_t>(1); tp.d_pair_t = cv.take<int32_t>(1);
        d_rot = cv.take<float>(9);
        d_xy = cv.take<float2>(n);
    });
    if (rc) return rc;
    const int32_t head[2] = {n, 0};                               // nkp[0] = n; pair 0's current record = 0
    HostStage hs(ctx);
    hs.up(tp.d_kps, kps, (size_t)n * sizeof(vis_keypoint));
    hs.up(tp.d_nkp, head, 4); hs.up(tp.d_pair_t, head + 1, 4);
    hs.up(d_rot, rot, 36);
    hs.flush_ups();
    rc = launch_warp(ctx, &tp, 1, d_rot, d_xy);
    tp = Plan();       // scratch-owned pointers: nothing to free
    if (rc) return vis_drain(ctx, rc);
    const void* h_xy = hs.down(d_xy, (size_t)n * 8);
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out_xy, h_xy, (size_t)n * 8);
    return VIS_OK;
}

// vis_bf_knn2_hamming_host with the keypoints of both sets and a window.  The rows are as long as the larger set -- or as the context's
// keypoint_capacity when that is larger, so a capacity above 16384 selects the popcount kernel here as it does for the slots.
extern "C" int vis_bf_knn2_hamming_guided_host(vis_ctx* ctx, const uint8_t* desc_q, const vis_keypoint* kps_q, int n_q,
                                               const uint8_t* desc_t, const vis_keypoint* kps_t, int n_t, const float rot[9], float radius,
                                               vis_dmatch* out12, vis_dmatch* out21) {
    if (n_q < 0 || n_t < 0 || (n_q && (!desc_q || !kps_q)) || (n_t && (!desc_t || !kps_t))) return VIS_E_INVALID;
    if (n_q > 65535 || n_t > 65535 || !guide_args_ok(rot, radius, true)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    const int kcap = std::max(std::max(std::max(n_q, n_t), 1), std::min(ctx->p.keypoint_capacity, 65535));
    const bool mfma = kcap <= 16384;
    Plan tp;
    tp.kcap = kcap; tp.npairs = 1;
    float* d_rot;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        tp.d_desc = cv.take<uint8_t>((size_t)kcap * 64);
        tp.d_kps = cv.take<vis_keypoint>((size_t)kcap * 2);
        tp.d_nkp = cv.take<int32_t>(2); tp.d_pair_q = cv.take<int32_t>(1); tp.d_pair_t = cv.take<int32_t>(1);
        tp.d_knn12 = cv.take<uint32_t>((size_t)kcap * 2); tp.d_knn21 = cv.take<uint32_t>((size_t)kcap * 2);
        tp.d_warp = cv.take<float2>(kcap);
        d_rot = cv.take<float>(9);
        if (mfma) tp.d_descx = cv.take<int8_t>((size_t)kcap * 256);
    });
    if (rc) return rc;
    const int32_t nk[2] = {n_q, n_t};
    const MatchGuide g = {d_rot, radius};
    HostStage hs(ctx);
    hs.up(tp.d_desc, desc_q, (size_t)n_q * 32);
    hs.up(tp.d_desc + (size_t)kcap * 32, desc_t, (size_t)n_t * 32);
    hs.up(tp.d_kps, kps_q, (size_t)n_q * sizeof(vis_keypoint));
    hs.up(tp.d_kps + kcap, kps_t, (size_t)n_t * sizeof(vis_keypoint));
    hs.up(tp.d_nkp, nk, 8);
    hs.up(d_rot, rot, 36);
    hs.flush_ups();
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, ctx->stream, tp.d_pair_q, tp.d_pair_t, 0, 1);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[4], ctx->stream);
    rc = launch_expand(ctx, &tp, 0, 2);
    if (!rc) rc = launch_match(ctx, &tp, 1, &g);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[5], ctx->stream);
    const uint32_t* h12 = out12 && n_q ? (const uint32_t*)hs.down(tp.d_knn12, (size_t)n_q * 8) : nullptr;
    const uint32_t* h21 = out21 && n_t ? (const uint32_t*)hs.down(tp.d_knn21, (size_t)n_t * 8) : nullptr;
    tp = Plan();       // scratch-owned pointers: nothing to free
    if (rc) return vis_drain(ctx, rc);
    rc = hs.wait();
    if (rc) return rc;
    { float a = 0; if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[4], ctx->ev[5])) ctx->tm.ms_knn = a; }
    if (h12) keys_to_dmatches(h12, n_q, out12);
    if (h21) keys_to_dmatches(h21, n_t, out21);
    return VIS_OK;
}

extern "C" int vis_bf_knn2_hamming_host(vis_ctx* ctx, const uint8_t* desc_q, int n_q, const uint8_t* desc_t, int n_t,
                                        vis_dmatch* out12, vis_dmatch* out21) {
    if (!ctx || n_q < 0 || n_t < 0 || (n_q && !desc_q) || (n_t && !desc_t)) return VIS_E_INVALID;
    if (n_q > 65535 || n_t > 65535) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    const int kcap = std::max(std::max(n_q, n_t), 1);
    Plan tp;
    tp.kcap = kcap;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        tp.d_desc = cv.take<uint8_t>((size_t)kcap * 64);
        tp.d_nkp = cv.take<int32_t>(2); tp.d_pair_q = cv.take<int32_t>(1); tp.d_pair_t = cv.take<int32_t>(1);
        tp.d_knn12 = cv.take<uint32_t>((size_t)kcap * 2); tp.d_knn21 = cv.take<uint32_t>((size_t)kcap * 2);
        tp.d_descx = cv.take<int8_t>((size_t)kcap * 256);
    });
    if (rc) return rc;
    const int32_t nk[2] = {n_q, n_t};
    HostStage hs(ctx);
    hs.up(tp.d_desc, desc_q, (size_t)n_q * 32);
    hs.up(tp.d_desc + (size_t)kcap * 32, desc_t, (size_t)n_t * 32);
    hs.up(tp.d_nkp, nk, 8);
    hs.flush_ups();
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, ctx->stream, tp.d_pair_q, tp.d_pair_t, 0, 1);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[4], ctx->stream);
    rc = launch_expand(ctx, &tp, 0, 2);
    if (!rc) rc = launch_match(ctx, &tp, 1);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[5], ctx->stream);
    const uint32_t* h12 = out12 && n_q ? (const uint32_t*)hs.down(tp.d_knn12, (size_t)n_q * 8) : nullptr;
    const uint32_t* h21 = out21 && n_t ? (const uint32_t*)hs.down(tp.d_knn21, (size_t)n_t * 8) : nullptr;
    tp = Plan();       // scratch-owned pointers: nothing to free
    if (rc) return vis_drain(ctx, rc);
    rc = hs.wait();
    if (rc) return rc;
    { float a = 0; if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[4], ctx->ev[5])) ctx->tm.ms_knn = a; }
    if (h12) keys_to_dmatches(h12, n_q, out12);
    if (h21) keys_to_dmatches(h21, n_t, out21);
    return VIS_OK;
}

// the filter results of one pair: queued behind the filter kernel, copied out after the call's wait
struct MatchFetch { const int32_t* ng; const int32_t* ns; const void* good; const void* sym; size_t ngood_cap, nsym_cap; };
static MatchFetch fetch_matches(HostStage& hs, Plan* pl, int pair, bool want_good, int cap, bool want_sym, int sym_cap) {
    MatchFetch f = {};
    f.ng = (const int32_t*)hs.down(pl->out().ngood + pair, 4);
    f.ns = (const int32_t*)hs.down(pl->out().nsym + pair, 4);
    f.ngood_cap = (size_t)std::max(0, std::min(cap, pl->root * pl->root));
    f.nsym_cap = (size_t)std::max(0, std::min(sym_cap, pl->kcap));
    if (want_good && f.ngood_cap) f.good = hs.down(pl->out().good + (size_t)pair * pl->root * pl->root, f.ngood_cap * sizeof(vis_dmatch));
    if (want_sym && f.nsym_cap) f.sym = hs.down(pl->out().sym + (size_t)pair * pl->kcap, f.nsym_cap * sizeof(vis_dmatch));
    return f;
}
static int deliver_matches(const MatchFetch& f, vis_dmatch* good, int cap, int* n_good, vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    const int ng = *f.ng, ns = *f.ns;
    if (n_good) *n_good = ng;
    if (n_sym) *n_sym = ns;
    if (good) {
        if (ng > cap) return VIS_E_CAPACITY;
        if (ng) std::memcpy(good, f.good, (size_t)ng * sizeof(vis_dmatch));
    }
    if (sym_out) {
        if (ns > sym_cap) return VIS_E_CAPACITY;
        if (ns) std::memcpy(sym_out, f.sym, (size_t)ns * sizeof(vis_dmatch));
    }
    return VIS_OK;
}

// vis_good_matches (rot == nullptr) and vis_good_matches_guided
static int good_matches_slots(vis_ctx* ctx, int slot_prev, int slot_cur, const float* rot, float radius, vis_dmatch* good, int cap, int* n_good,
                              vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    (void)hipSetDevice(ctx->device);
    Plan* pl = ctx->single;
    int rc = pl ? vis_ensure_pin(ctx, ((size_t)pl->kcap + (size_t)pl->root * pl->root) * sizeof(vis_dmatch) + 4096) : VIS_E_STATE;
    if (!rc) rc = set_single_pair(ctx, pl, slot_prev, slot_cur);
    MatchGuide g = {nullptr, 0.f};
    if (!rc && rot) rc = single_guide(ctx, pl, rot, radius, &g);
    if (rc) return rc;
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[4], ctx->stream);
    rc = launch_expand(ctx, pl, slot_prev, 1);
    if (!rc && slot_cur != slot_prev) rc = launch_expand(ctx, pl, slot_cur, 1);
    if (!rc) rc = launch_match(ctx, pl, 1, rot ? &g : nullptr);
    if (rc) return rc;
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[5], ctx->stream);
    rc = launch_filter(ctx, pl, 1);
    if (rc) return rc;
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[6], ctx->stream);
    HostStage hs(ctx);
    const MatchFetch f = fetch_matches(hs, pl, 0, good != nullptr, cap, sym_out != nullptr, sym_cap);
    rc = hs.wait();
    if (rc) return rc;
    { float a = 0;
      if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[4], ctx->ev[5])) ctx->tm.ms_knn = a;
      if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[5], ctx->ev[6])) ctx->tm.ms_filter = a; }
    return deliver_matches(f, good, cap, n_good, sym_out, sym_cap, n_sym);
}

extern "C" int vis_good_matches(vis_ctx* ctx, int slot_prev, int slot_cur, vis_dmatch* good, int cap, int* n_good,
                                vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    if (!ctx) return VIS_E_INVALID;
    return good_matches_slots(ctx, slot_prev, slot_cur, nullptr, 0.f, good, cap, n_good, sym_out, sym_cap, n_sym);
}

extern "C" int vis_good_matches_guided(vis_ctx* ctx, int slot_prev, int slot_cur, const float rot[9], float radius, vis_dmatch* good, int cap,
                                       int* n_good, vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    if (!guide_args_ok(rot, radius, true)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    return good_matches_slots(ctx, slot_prev, slot_cur, rot, radius, good, cap, n_good, sym_out, sym_cap, n_sym);
}

static uint32_t dmatch_to_key(const vis_dmatch& m) {
    if (m.trainIdx < 0) return 0xFFFFFFFFu;
    return ((uint32_t)m.distance << 16) | (uint32_t)(m.trainIdx & 0xFFFF);
}

extern "C" int vis_good_matches_host(vis_ctx* ctx, const vis_keypoint* kps1, int n1, const vis_keypoint* kps2, int n2,
                                     const vis_dmatch* knn12, const vis_dmatch* knn21,
                                     vis_dmatch* good, int cap, int* n_good,
                                     vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    if (!ctx || n1 < 0 || n2 < 0 || n1 > 65535 || n2 > 65535) return VIS_E_INVALID;
    if ((n1 && (!kps1 || !knn12)) || (n2 && (!kps2 || !knn21))) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    const int kcap = std::max(std::max(n1, n2), 1);
    int root; std::vector<float> hf, wf; vis_grid_limits(ctx->p, &root, hf, wf);
    const int ncell = root * root;
    Plan tp; tp.kcap = kcap; tp.root = root;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        tp.d_kps = cv.take<vis_keypoint>((size_t)kcap * 2);
        tp.d_nkp = cv.take<int32_t>(2); tp.d_pair_q = cv.take<int32_t>(1); tp.d_pair_t = cv.take<int32_t>(1);
        tp.d_knn12 = cv.take<uint32_t>((size_t)kcap * 2); tp.d_knn21 = cv.take<uint32_t>((size_t)kcap * 2);
        Plan::MatchOut& o = tp.out();
        o.sym = cv.take<vis_dmatch>(kcap); o.nsym = cv.take<int32_t>(1);
        o.good = cv.take<vis_dmatch>(ncell); o.ngood = cv.take<int32_t>(1);
        o.p1 = cv.take<float>((size_t)ncell * 2); o.p2 = cv.take<float>((size_t)ncell * 2);
        tp.d_hf = cv.take<float>(root); tp.d_wf = cv.take<float>(root);
    });
    if (rc) return rc;
    std::vector<uint32_t> k12(2 * (size_t)kcap, 0xFFFFFFFFu), k21(2 * (size_t)kcap, 0xFFFFFFFFu);
    for (int i = 0; i < 2 * n1; i++) k12[i] = dmatch_to_key(knn12[i]);
    for (int i = 0; i < 2 * n2; i++) k21[i] = dmatch_to_key(knn21[i]);
    const int32_t nk[2] = {n1, n2};
    HostStage hs(ctx);
    hs.up(tp.d_kps, kps1, (size_t)n1 * sizeof(vis_keypoint));
    hs.up(tp.d_kps + kcap, kps2, (size_t)n2 * sizeof(vis_keypoint));
    hs.up(tp.d_nkp, nk, 8);
    hs.flush_ups();
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, ctx->stream, tp.d_pair_q, tp.d_pair_t, 0, 1);
    hs.up(tp.d_knn12, k12.data(), k12.size() * 4);
    hs.up(tp.d_knn21, k21.data(), k21.size() * 4);
    hs.up(tp.d_hf, hf.data(), (size_t)root * 4);
    hs.up(tp.d_wf, wf.data(), (size_t)root * 4);
    hs.flush_ups();
    rc = launch_filter(ctx, &tp, 1);
    if (rc) return vis_drain(ctx, rc);
    const MatchFetch f = fetch_matches(hs, &tp, 0, good != nullptr, cap, sym_out != nullptr, sym_cap);
    tp = Plan();
    rc = hs.wait();
    if (rc) return rc;
    return deliver_matches(f, good, cap, n_good, sym_out, sym_cap, n_sym);
}

// The pose stage's working buffers (pose_run's arguments) for n rows of mc correspondences and `iters` hypotheses, declared ONCE: pose_host carves
// them from the scratch block for one pair, vis_essential_batch from the context's own workspace for n.
struct PoseWork {
    double *n1, *n2, *models, *hyp; int32_t *samples, *counts, *rstate, *worklist; uint8_t* mask;
    void layout(Carver& cv, size_t n, size_t mc, size_t iters) {
        n1 = cv.take<double>(n * mc * 2); n2 = cv.take<double>(n * mc * 2);
        samples = cv.take<int32_t>(n * iters * 5);
        models = cv.take<double>(n * iters * 90);
        counts = cv.take<int32_t>(n * iters * 10);
        rstate = cv.take<int32_t>(n * VIS_RSTATE_WORDS);
        mask = cv.take<uint8_t>(n * mc);
        worklist = cv.take<int32_t>(2 + n);
        hyp = cv.take<double>(n * iters * VIS_HYP_DOUBLES);
    }
};

// shared by vis_essential_ransac / vis_recover_pose
static int pose_host(vis_ctx* ctx, const float* p1xy, const float* p2xy, int m, const double* E_in,
                     int do_ransac, int do_pose, uint8_t* mask, PoseOut* out) {
    (void)hipSetDevice(ctx->device);
    if (m > VIS_RANSAC_MAX_M) return VIS_E_CAPACITY;
    const int mcap = std::max(m, 1);
    const int iters = ctx->p.ransac_max_iters;
    // scratch sized for a power-of-two correspondence count >= 256: a stream whose match count creeps up does not re-allocate per call
    int mroom = 256; while (mroom < mcap) mroom <<= 1;
    float *d_p1, *d_p2; double* d_E; int32_t* d_npts; PoseOut* d_pose; PoseWork W;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        const size_t mc = cv.base ? mcap : mroom;                  // measured with room, bound to what the call uses
        d_p1 = cv.take<float>(mc * 2); d_p2 = cv.take<float>(mc * 2);
        d_npts = cv.take<int32_t>(1);
        d_E = cv.take<double>(9);
        d_pose = cv.take<PoseOut>(1);
        W.layout(cv, 1, mc, (size_t)iters);
    });
    if (rc) return rc;
    double *d_n1 = W.n1, *d_n2 = W.n2, *d_models = W.models, *d_hyp = W.hyp; int32_t *d_samples = W.samples, *d_counts = W.counts, *d_rstate = W.rstate, *d_worklist = W.worklist;
    uint8_t* d_mask = W.mask;
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    const int32_t mm = m;
    hs.up(d_npts, &mm, 4);
    if (E_in) hs.up(d_E, E_in, 72);
    hs.flush_ups();
    rc = vis_build_sample_table(ctx, VIS_POSE_TABLE_M);           // (already there since vis_set_params / the first call: never rebuilt because M grew)
    if (rc) return vis_drain(ctx, rc);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[6], ctx->stream);
    rc = pose_run(ctx, 1, mcap, iters, d_p1, d_p2, d_npts, d_n1, d_n2, d_samples, d_models, d_counts, d_rstate,
                  E_in ? d_E : nullptr, d_mask, d_pose, do_ransac, do_pose, d_worklist, d_hyp);
    if (rc) return vis_drain(ctx, rc);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[7], ctx->stream);
    const void* h_pose = hs.down(d_pose, sizeof(PoseOut));
    const void* h_mask = mask && m ? hs.down(d_mask, (size_t)m) : nullptr;
    rc = hs.wait();
    if (rc) return rc;
    { float a = 0; if (ctx->ev_ok && ev_elapsed(&a, ctx->ev[6], ctx->ev[7])) ctx->tm.ms_pose = a; }
    std::memcpy(out, h_pose, sizeof(PoseOut));
    if (out->undecided_max > 0) ctx->undecided_max = std::max(ctx->undecided_max, (unsigned long long)out->undecided_max);
    if (h_mask) std::memcpy(mask, h_mask, (size_t)m);
    return VIS_OK;
}

extern "C" int vis_essential_ransac(vis_ctx* ctx, const float* p1xy, const float* p2xy, int m,
                                    double E[9], uint8_t* mask, int* n_inliers, int* iters_run) {
    if (!ctx || m < 0 || (m && (!p1xy || !p2xy)) || !E) return VIS_E_INVALID;
    PoseOut o;
    int rc = pose_host(ctx, p1xy, p2xy, m, nullptr, 1, 0, mask, &o);
    if (rc) return rc;
    std::memcpy(E, o.E, 72);
    if (n_inliers) *n_inliers = o.n_inliers;
    if (iters_run) *iters_run = o.iters_run;
    return VIS_OK;
}

extern "C" int vis_recover_pose(vis_ctx* ctx, const double E[9], const float* p1xy, const float* p2xy, int m,
                                double R[9], double t[3], int* n_good) {
    if (!ctx || !E || m < 0 || (m && (!p1xy || !p2xy)) || !R || !t) return VIS_E_INVALID;
    PoseOut o;
    int rc = pose_host(ctx, p1xy, p2xy, m, E, 0, 1, nullptr, &o);
    if (rc) return rc;
    std::memcpy(R, o.R, 72); std::memcpy(t, o.t, 24);
    if (n_good) *n_good = o.n_pose_good;
    return VIS_OK;
}

extern "C" int vis_f2f_ransac(vis_ctx* ctx, const vis_keypoint* pts1, const vis_keypoint* pts2, int m, const float rot[9],
                              const int32_t* sample_idx, int iters, float scale, float out_t[3], int* count_max) {
    if (!ctx || !out_t || m < 0 || iters < 0 || !rot || (iters && !sample_idx) || (m && (!pts1 || !pts2))) return VIS_E_INVALID;
    out_t[0] = out_t[1] = out_t[2] = 0.f;
    if (count_max) *count_max = 0;
    if (m < 2 || iters == 0) return VIS_OK;                       // SPEC: M < 2 -> zero vector
    for (int i = 0; i < 2 * iters; i++) if (sample_idx[i] < 0 || sample_idx[i] >= m) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    float *d_p1, *d_p2, *d_rot; int32_t *d_idx, *d_n; vis_f2f_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>((size_t)m * 2); d_p2 = cv.take<float>((size_t)m * 2);
        d_rot = cv.take<float>(9); d_idx = cv.take<int32_t>((size_t)iters * 2); d_n = cv.take<int32_t>(1);
        d_out = cv.take<vis_f2f_result>(1);
    });
    if (rc) return rc;
    std::vector<float> xy((size_t)m * 4);
    for (int i = 0; i < m; i++) { xy[2 * (size_t)i] = pts1[i].x; xy[2 * (size_t)i + 1] = pts1[i].y; xy[2 * ((size_t)m + i)] = pts2[i].x; xy[2 * ((size_t)m + i) + 1] = pts2[i].y; }
    const int32_t n1 = m;
    HostStage hs(ctx);
    hs.up(d_p1, xy.data(), (size_t)m * 8);
    hs.up(d_p2, xy.data() + (size_t)m * 2, (size_t)m * 8);
    hs.up(d_rot, rot, 36);
    hs.up(d_idx, sample_idx, (size_t)iters * 8);
    hs.up(d_n, &n1, 4);
    hs.flush_ups();
    // one pair of k_f2f_batch with the indices as given and no reference translation: the record's t is (float)d of the winner -- `if (count >
    // countMax)`, the first strictly larger count in iteration order (src/VISystem.cpp:737-741), degenerate samples never -- or zero
    rc = f2f_batch_run(ctx, 1, m, d_p1, d_p2, d_n, d_rot, nullptr, d_idx, iters, true, d_out);
    if (rc) return vis_drain(ctx, rc);
    const vis_f2f_result* r = (const vis_f2f_result*)hs.down(d_out, sizeof(vis_f2f_result));
    rc = hs.wait();
    if (rc) return rc;
    for (int k = 0; k < 3; k++) out_t[k] = scale * r->t[k];
    if (count_max) *count_max = r->count_max;
    return VIS_OK;
}

// blocking downloads of the batch getters (vis_batch_get_*: test / inspection entry points behind a full synchronisation)
static int download_knn(vis_ctx* ctx, const uint32_t* d_keys, int n, vis_dmatch* out) {
    if (!out || n <= 0) return VIS_OK;
    std::vector<uint32_t> k(2 * (size_t)n);
    HIPCHK(ctx, hipMemcpy(k.data(), d_keys, k.size() * 4, hipMemcpyDeviceToHost));
    keys_to_dmatches(k.data(), n, out);
    return VIS_OK;
}
static int download_matches(vis_ctx* ctx, Plan* pl, int pair, vis_dmatch* good, int cap, int* n_good,
                            vis_dmatch* sym_out, int sym_cap, int* n_sym) {
    int32_t ng = 0, ns = 0;
    HIPCHK(ctx, hipMemcpy(&ng, pl->out().ngood + pair, 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&ns, pl->out().nsym + pair, 4, hipMemcpyDeviceToHost));
    if (n_good) *n_good = ng;
    if (n_sym) *n_sym = ns;
    if (good) {
        if (ng > cap) return VIS_E_CAPACITY;
        if (ng) HIPCHK(ctx, hipMemcpy(good, pl->out().good + (size_t)pair * pl->root * pl->root, (size_t)ng * sizeof(vis_dmatch), hipMemcpyDeviceToHost));
    }
    if (sym_out) {
        if (ns > sym_cap) return VIS_E_CAPACITY;
        if (ns) HIPCHK(ctx, hipMemcpy(sym_out, pl->out().sym + (size_t)pair * pl->kcap, (size_t)ns * sizeof(vis_dmatch), hipMemcpyDeviceToHost));
    }
    return VIS_OK;
}

// ------------------------------------------------------------------------------------------------ batch API
extern "C" int vis_batch_plan(vis_ctx* ctx, int w, int h, int stride, int max_frames) {
    if (!ctx || max_frames < 1 || max_frames > 4096) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);
    plan_destroy(ctx->batch); ctx->batch = nullptr;
    return plan_create(ctx, w, h, stride, max_frames, max_frames + 1, max_frames, &ctx->batch, VIS_BATCH_SETS);
}

extern "C" int vis_batch_reset(vis_ctx* ctx) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    sync_all(ctx);
    ctx->batch->have_prev = false; ctx->batch->last_n = 0; ctx->batch->pyr_frames = 0; ctx->batch->carry_from = 0; ctx->batch->pair0_valid = false;
    { const int rc = reset_keyframe_state(ctx, ctx->batch); if (rc) return rc; }   // keyframe gate: nothing saved, nothing carried
    ctx->batch->seq_next = ctx->batch->seq0 = 0; ctx->batch->ft.forget();   // vis_batch_ftrack: no carried row, seq restarts at 0
    ctx->batch->sl.forget(); ctx->batch->tj.forget();              // scale links / trajectory: nothing carried
    ctx->batch->imuc.forget();                                     // vis_batch_imu_cov: the same
    ctx->batch->imuj.forget();                                     // vis_batch_imu_jac: the same
    ctx->batch->imu.forget();                                      // vis_batch_imu: no carried time, no open delta
    ctx->batch->via.forget();                                      // vis_batch_vi_align: no carried sums, no tails
    ctx->batch->viab.forget();                                     // vis_batch_vi_align_ba: the same
    ctx->batch->run_seq = ctx->batch->track_seq = 0;              // vis_batch_track: the chain restarts at vis_batch_track_init's pose
    { const int rc = reset_track_state(ctx, ctx->batch, false); if (rc) return rc; }
    if (ctx->batch->speculate) {                                   // a new stream: no prediction
        std::vector<int32_t> t0((size_t)ctx->batch->L, ctx->p.fast_threshold);
        HIPCHK(ctx, hipMemcpy(ctx->batch->d_tau, t0.data(), t0.size() * 4, hipMemcpyHostToDevice));
    }
    return VIS_OK;
}

// Four streams per context: A = detect chain (caller's / own stream), U = Camera::Update / gradients, M = expand + knn + filters,
// P = RANSAC + recoverPose (and vis_batch_align / _track).  Batch i+1's detect chain overlaps batch i's matcher (MFMA + LDS, little
// VALU) and pose (latency-bound FP64): the record, gradient and matcher-output sets are used in turn, and the writer of a set waits
// for the readers of its last use (ReaderGuard, vis_internal.h).
// guide != nullptr (vis_batch_run_guided): the match stage searches inside the window; nothing of it outlives the call
static int batch_run_impl(vis_ctx* ctx, const uint8_t* d_frames, int n, int stages, const MatchGuide* guide) {
    Plan* pl = ctx->batch;
    if (!pl) return VIS_E_STATE;
    if (n < 1 || n > pl->B || ((uintptr_t)d_frames & 3)) return VIS_E_INVALID;
    (void)hipSetDevice(ctx->device);
    if (guide) { const int rcw = ensure_warp(ctx, pl); if (rcw) return rcw; }
    hipStream_t sA = ctx->stream, sM = ctx->match_stream, sP = ctx->pose_stream;
    ctx->tm.launches_total = 0;
    const bool detect = (stages & VIS_STAGE_DETECT) != 0;
    const int cur = detect ? (pl->run_count % pl->nsets) : (pl->last_base / pl->rec_per_set);   // run_count is committed only when every launch succeeded
    const int base = cur * pl->rec_per_set;
    int rc = VIS_OK;
    bool have_prev = pl->have_prev;
    if (detect) {
        // this record set was last read by the matcher nsets batches ago: launch_detect waits for it where the chain first writes the set
        if (pl->carry_from > 0) have_prev = true;      // previous batch's last frame -> record 0 of this set: copied by launch_detect's first kernel
    }
    // Camera::Update (src/Camera.cpp:63-72): the half pyramid of every frame of the batch.  Nothing of the detect chain reads it
    // and it is pure streaming work, so it runs on a stream of its own beside the (vector-ALU bound) detect kernels; the detect
    // stream joins it at the end of its chain, so "the detect stream is done" still means "d_frames may be reused".
    Plan::RecordSet& rs = pl->rec[cur];
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[0], sA);
    // keyframe gate on: the carried record is the last SAVED one, known only on the device -- k_keyframe_links copies it, behind the
    // records of this batch (it reads their counts), launch_detect's wait for the matcher that last read this set and the alignments
    // that still read its links
    if (detect) { VisRange r_("vis: ORB detect + describe"); rc = launch_detect(ctx, pl, d_frames, n, base + 1, (pl->carry_from > 0 && !pl->kf_min) ? pl->carry_from : -1,
                                                                             (stages & (VIS_STAGE_UPDATE | VIS_STAGE_GRADIENT)) ? ctx->ev_update_fork : nullptr, &rs.matcher);
                  if (!rc && pl->kf_min) rc = rs.links.wait(sA) == hipSuccess ? launch_keyframe_links(ctx, pl, cur, n) : VIS_E_HIP;
                  if (rc) return rc; }
    else if (ctx->ev_ok) for (int i = 1; i <= 4; i++) (void)hipEventRecord(ctx->ev[i], sA);
    hipStream_t sU = ctx->update_stream;
    pl->half_valid = false; pl->grad_valid = false;
    bool update_queued = false;
    if (stages & (VIS_STAGE_UPDATE | VIS_STAGE_GRADIENT)) {
        VisRange r_("vis: Camera::Update half pyramid");
        // this step's half pyramid / gradient set: the one the step before last used.  The plan's view of it (grad_set) is switched only
        // once every launch of the stage has been queued; a failure leaves the last step's set in place
        const int gs = pl->grad_set ^ 1;
        Plan::GradSet& G = pl->grad[gs];
        const size_t fe = vis_grad_frame_elems(pl->w, pl->h);
        if (!G.half) HIPCHK(ctx, hipMalloc((void**)&G.half, (size_t)pl->B * fe));
        if ((stages & VIS_STAGE_GRADIENT) && !G.gx) {
            HIPCHK(ctx, hipMalloc((void**)&G.gx, (size_t)pl->B * fe * 2)); HIPCHK(ctx, hipMalloc((void**)&G.gy, (size_t)pl->B * fe * 2));
            HIPCHK(ctx, hipMalloc((void**)&G.g, (size_t)pl->B * fe));
        }
        // the frames were produced on the detect stream (or before the call): the side stream is ordered behind it -- behind the
        // PYRAMID launches of this batch's detect chain (launch_detect recorded the event there): the resize chain streams at HBM
        // speed itself, the kernels after it are vector-ALU bound, and that is where streaming work fits beside them
        if (!detect) HIPCHK(ctx, hipEventRecord(ctx->ev_update_fork, sA));
        HIPCHK(ctx, hipStreamWaitEvent(sU, ctx->ev_update_fork, 0));
        // an alignment two steps back (vis_batch_align on the pose stream) may still read THIS set's half pyramid / gradients
        HIPCHK(ctx, G.readers.wait(sU));
        if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[10], sU);
        { StreamScope on(ctx, sU);
          rc = launch_half_pyramid_batch(ctx, d_frames, pl->w, pl->h, pl->stride, (size_t)pl->stride * pl->h, n, G.half);
          if (!rc && (stages & VIS_STAGE_GRADIENT))
              rc = launch_gradient(ctx, d_frames, pl->w, pl->h, pl->stride, (size_t)pl->stride * pl->h, n, G.half, 3 /* the reference's Scharr scale, src/Camera.cpp:172 */,
                                   G.gx, G.gy, G.g); }
        if (rc) {
            // whatever was queued on the side stream before the failure still reads d_frames / writes set gs: the detect stream joins
            // it before this call returns, so "ctx->stream is done" keeps meaning "the batch's buffers are free"
            if (hipEventRecord(ctx->ev_update_done, sU) == hipSuccess) (void)hipStreamWaitEvent(sA, ctx->ev_update_done, 0);
            return rc;
        }
        pl->grad_set = gs;
        pl->grad_valid = (stages & VIS_STAGE_GRADIENT) != 0;
        if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[11], sU);
        HIPCHK(ctx, hipEventRecord(ctx->ev_update_done, sU));
        update_queued = true;
        pl->half_valid = true;
    }
    // the matcher needs the records (detect chain), not the side stream's half pyramid / gradients: its event comes BEFORE the join (with
    // the join in front, the matcher -- and through it the alignment and the next step's gradients -- waited for the gradient stage)
    HIPCHK(ctx, hipEventRecord(ctx->ev_detect_done, sA));
    if (update_queued) HIPCHK(ctx, hipStreamWaitEvent(sA, ctx->ev_update_done, 0));
    if (stages & (VIS_STAGE_MATCH | VIS_STAGE_POSE)) HIPCHK(ctx, hipStreamWaitEvent(sM, ctx->ev_detect_done, 0));
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev_match_start, sM);
    // pair i: query = record base+i (frame i-1, or the carried frame for i = 0), train = record base+i+1 (frame i); keyframe gate on:
    // query = the record of the last saved frame before i (or -1: no pair), from the table k_keyframe_links wrote for this set
    pl->d_pair_q = pl->kf_min ? rs.gq : (have_prev ? rs.pq : rs.pqn);
    pl->d_pair_t = rs.pt;
    // the matcher-output set of this step: a step that runs the matcher takes the next one, a pose-only step reads the last one
    const int last_mo = pl->mo_cur, mo = pl->mo[1].sym ? ((stages & VIS_STAGE_MATCH) ? (last_mo ^ 1) : last_mo) : 0;
    pl->mo_cur = mo;
    Plan::MatchOut& O = pl->out();
    if (stages & VIS_STAGE_MATCH) {
        VisRange r_("vis: knn + match filters");
        StreamScope on(ctx, sM);
        rc = launch_expand(ctx, pl, base, n + 1);
        if (!rc) rc = launch_match(ctx, pl, n, guide);
        if (!rc) {
            if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[5], sM);
            // the filter writes matcher-output set `mo` (sets in turn, like the records): wait for what still reads THAT set -- the pose
            // stage, the alignment and the results download of the step before last; those of the last step read the other set
            rc = O.readers.wait(sM) == hipSuccess ? launch_filter(ctx, pl, n) : VIS_E_HIP;
        }
        if (!rc && ctx->ev_ok) (void)hipEventRecord(ctx->ev[6], sM);
        if (!rc) { (void)hipEventRecord(ctx->ev_match_done[cur], sM); rs.matcher.note(sM, ctx->ev_match_done[cur]); }
    } else if (ctx->ev_ok) { (void)hipEventRecord(ctx->ev[5], sM); (void)hipEventRecord(ctx->ev[6], sM); }
    if (!rc && (stages & VIS_STAGE_POSE)) {
        (void)hipEventRecord(ctx->ev_filter_done, sM);
        (void)hipStreamWaitEvent(sP, ctx->ev_filter_done, 0);
        StreamScope on(ctx, sP);
        (void)hipEventRecord(ctx->ev_pose_start, sP);
        VisRange r_("vis: essential RANSAC + recoverPose");
        rc = launch_pose(ctx, pl, n);
        (void)hipEventRecord(ctx->ev_pose_done, sP);
        ctx->pose_pending = true;
        if (hipEventRecord(ctx->ev_pose_done_set[mo], sP) == hipSuccess) O.readers.note(sP, ctx->ev_pose_done_set[mo]);
    }
    if (rc) { pl->mo_cur = last_mo; pl->half_valid = pl->grad_valid = false; return rc; }   // nothing of the stream state (carried frame, record set, matcher-output set) has been committed
    pl->have_prev = have_prev; pl->pair0_valid = have_prev;
    if (detect) { pl->run_count++; pl->carry_from = base + n; pl->seq0 = pl->seq_next; pl->seq_next += n; }
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[8], sA);
    pl->last_n = n; pl->last_base = base;
    pl->last_stages = stages; pl->run_seq++;                      // (what vis_batch_track checks)
    return VIS_OK;
}

extern "C" int vis_batch_run(vis_ctx* ctx, const uint8_t* d_frames, int n, int stages) {
    if (!ctx || !d_frames) return VIS_E_INVALID;
    return batch_run_impl(ctx, d_frames, n, stages, nullptr);
}

extern "C" int vis_batch_run_guided(vis_ctx* ctx, const uint8_t* d_frames, int n, int stages, const float* d_rot, float radius) {
    if (!d_frames || !guide_args_ok(d_rot, radius, false) || !(stages & VIS_STAGE_MATCH)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    const MatchGuide g = {d_rot, radius};
    return batch_run_impl(ctx, d_frames, n, stages, &g);
}

extern "C" int vis_batch_track_init(vis_ctx* ctx, const vis_se3f* pose) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                // (a chain kernel in flight writes the state)
    Plan* pl = ctx->batch;
    pl->track_init = pose ? *pose : vis_se3f{0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    const int rc = ensure_track_buffers(ctx, pl);
    return rc ? rc : reset_track_state(ctx, pl, true);
}

extern "C" int vis_batch_sync(vis_ctx* ctx) {
    if (!ctx) return VIS_E_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->update_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->update_stream));
    if (ctx->match_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->match_stream));
    const bool had_pose = ctx->pose_pending;
    if (ctx->pose_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->pose_stream));
    clear_pending(ctx);
    if (ctx->ev_ok) {
        collect_detect_timings(ctx);
        float a = 0;
        if (ev_elapsed(&a, ctx->ev_match_start, ctx->ev[5])) ctx->tm.ms_knn = a;
        if (ev_elapsed(&a, ctx->ev[5], ctx->ev[6])) ctx->tm.ms_filter = a;
        ctx->tm.ms_pose = 0;
        if (had_pose && ev_elapsed(&a, ctx->ev_pose_start, ctx->ev_pose_done)) ctx->tm.ms_pose = a;
        ctx->tm.ms_update = 0;
        const bool upd = ctx->batch && ctx->batch->half_valid;
        if (upd && ev_elapsed(&a, ctx->ev[10], ctx->ev[11])) ctx->tm.ms_update = a;
        hipEvent_t e0 = ctx->ev[0];
        if (ev_elapsed(&a, e0, ctx->ev[8])) ctx->tm.ms_total = a;
        if (ev_elapsed(&a, e0, ctx->ev[6]) && a > ctx->tm.ms_total) ctx->tm.ms_total = a;
        if (had_pose && ev_elapsed(&a, e0, ctx->ev_pose_done) && a > ctx->tm.ms_total) ctx->tm.ms_total = a;
    }
    return VIS_OK;
}

extern "C" int vis_batch_half_pyramid(vis_ctx* ctx, const uint8_t** d_half, size_t* frame_elems) {
    if (!ctx || !ctx->batch || !d_half) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!pl->half_valid) return VIS_E_STATE;
    *d_half = pl->grad[pl->grad_set].half;
    if (frame_elems) *frame_elems = vis_grad_frame_elems(pl->w, pl->h);
    return VIS_OK;
}

extern "C" int vis_batch_gradients(vis_ctx* ctx, const uint8_t** d_gray, const int16_t** d_gx, const int16_t** d_gy, const uint8_t** d_g, size_t* frame_elems) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!pl->grad_valid) return VIS_E_STATE;
    const Plan::GradSet& G = pl->grad[pl->grad_set];
    if (d_gray) *d_gray = G.half;
    if (d_gx) *d_gx = G.gx;
    if (d_gy) *d_gy = G.gy;
    if (d_g) *d_g = G.g;
    if (frame_elems) *frame_elems = vis_grad_frame_elems(pl->w, pl->h);
    return VIS_OK;
}

extern "C" int vis_batch_results_async(vis_ctx* ctx, vis_pose_result* h_pose, vis_dmatch* h_good, int32_t* h_ngood, int n_cap) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    const int n = pl->last_n;
    if (n < 1) return VIS_E_STATE;
    if (n_cap < n) { ctx->err = "vis_batch_results_async: caller buffers hold fewer frames than the last batch"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    // the pose stream is ordered behind the matcher of the same batch (ev_filter_done); without a pose stage the matcher's own stream
    hipStream_t s = ctx->pose_pending ? ctx->pose_stream : ctx->match_stream;
    const int ncell = pl->root * pl->root;
    // Pinned (device-accessible) destinations are written by ONE small kernel of the library instead of three hipMemcpyAsync: every
    // device-to-host copy of the runtime ends in a system-scope release, and with one per step the whole pipeline lost 8 % (round 5:
    // 402 k -> 371 k frames/s with a single 196 KB copy per step).  The host reads after vis_batch_sync, which orders it.  Anything
    // else (pageable memory, unaligned pointers) goes through the runtime's copies as before.
    void* dsts[3]; const void* srcs[3]; size_t bytes[3]; int nj = 0; bool mapped = true;
    auto add = [&](void* h, const void* d, size_t b) {
        if (!h) return;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, h) != hipSuccess) { (void)hipGetLastError(); mapped = false; }
        else if (at.type != hipMemoryTypeHost || !at.devicePointer || ((uintptr_t)at.devicePointer & 3)) mapped = false;
        else { dsts[nj] = at.devicePointer; }
        if (!mapped) dsts[nj] = h;
        srcs[nj] = d; bytes[nj] = b; nj++;
    };
    add(h_pose, pl->d_pose, (size_t)n * sizeof(vis_pose_result));
    add(h_good, pl->out().good, (size_t)n * ncell * sizeof(vis_dmatch));
    add(h_ngood, pl->out().ngood, (size_t)n * sizeof(int32_t));
    if (nj && mapped) { const int rc = launch_copy_jobs(ctx, s, nj, dsts, srcs, bytes); if (rc) return rc; ctx->n_copies++; }
    else {
        if (h_pose) HIPCHK(ctx, hipMemcpyAsync(h_pose, pl->d_pose, (size_t)n * sizeof(vis_pose_result), hipMemcpyDeviceToHost, s));
        if (h_good) HIPCHK(ctx, hipMemcpyAsync(h_good, pl->out().good, (size_t)n * ncell * sizeof(vis_dmatch), hipMemcpyDeviceToHost, s));
        if (h_ngood) HIPCHK(ctx, hipMemcpyAsync(h_ngood, pl->out().ngood, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_results_done_set[pl->mo_cur], s));
    pl->out().readers.note(s, ctx->ev_results_done_set[pl->mo_cur]);
    return VIS_OK;
}

// ---- map points (VISystem::Triangulate / Disparity): pose.hip k_triangulate
extern "C" void vis_default_tri_params(vis_tri_params* tp) {
    if (!tp) return;
    tp->max_reproj_px = 2.0f; tp->min_parallax_px = 0.0f; tp->inliers_only = 0; tp->reserved_ = 0;
}

extern "C" int vis_triangulate(vis_ctx* ctx, const vis_tri_params* tp, const double R[9], const double t[3],
                               const float* p1xy, const float* p2xy, int m, const uint8_t* mask,
                               vis_map_point* points, uint8_t* flags, vis_tri_summary* summary) {
    if (!ctx || !tp || !R || !t || !summary || m < 0 || (m && (!p1xy || !p2xy || !points || !flags))) return VIS_E_INVALID;
    std::memset(summary, 0, sizeof(*summary));
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    float *d_p1, *d_p2; uint8_t *d_mask, *d_flags; PoseOut* d_pose; vis_map_point* d_points; vis_tri_summary* d_summary;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>((size_t)m * 2); d_p2 = cv.take<float>((size_t)m * 2);
        d_mask = cv.take<uint8_t>(m);
        d_pose = cv.take<PoseOut>(1);
        d_points = cv.take<vis_map_point>(m);
        d_flags = cv.take<uint8_t>(((size_t)m + 3) & ~(size_t)3);
        d_summary = cv.take<vis_tri_summary>(1);
    });
    if (rc) return rc;
    PoseOut o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(o.R, R, 72); std::memcpy(o.t, t, 24);
    o.n_points = m;
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    if (mask) hs.up(d_mask, mask, (size_t)m);
    hs.up(d_pose, &o, sizeof(o));
    hs.flush_ups();
    // (a pair without a pose leaves its rows untouched: the caller's buffers are then not written either, summary.n_points == 0 below)
    rc = triangulate_run(ctx, tp, 1, m, m, d_pose, d_p1, d_p2, mask ? d_mask : nullptr, d_points, d_flags, d_summary);
    if (rc) return vis_drain(ctx, rc);
    const void* h_sum = hs.down(d_summary, sizeof(vis_tri_summary));
    const void* h_pts = hs.down(d_points, (size_t)m * sizeof(vis_map_point));
    const void* h_fl = hs.down(d_flags, ((size_t)m + 3) & ~(size_t)3);
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(summary, h_sum, sizeof(*summary));
    if (summary->n_points > 0) { std::memcpy(points, h_pts, (size_t)m * sizeof(vis_map_point)); std::memcpy(flags, h_fl, (size_t)m); }
    return VIS_OK;
}

extern "C" int vis_batch_triangulate(vis_ctx* ctx, const vis_tri_params* tp, int n, int row_cap,
                                     vis_map_point* d_points, uint8_t* d_flags, vis_tri_summary* d_summary) {
    if (!tp || !d_points || !d_flags || !d_summary || ((uintptr_t)d_points & 15) || ((uintptr_t)d_summary & 3)) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_triangulate: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (row_cap < pl->pose_mcap) { ctx->err = "vis_batch_triangulate: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    // On the pose stream, behind the pose stage that wrote d_mask / d_pose (single-buffered, written on that stream only: the next
    // pose stage is queued behind this call) and that itself waited for the filter that wrote p1 / p2.  Those belong to the matcher-output
    // set of the last step, which the filter two steps on rewrites: it waits for the reader event noted here.  (No fork: that would order
    // the call behind the side stream's gradients, which the detect stream joins.)
    Plan::MatchOut& O = pl->out();
    return on_pose_stream(ctx, {0, ctx->ev_tri_done[pl->mo_cur]}, [&] {
        const int rc = triangulate_run(ctx, tp, n, pl->pose_mcap, row_cap, pl->d_pose, O.p1, O.p2, pl->d_mask, d_points, d_flags, d_summary);
        if (!rc) ctx->pose_pending = true;
        return rc;
    }, {&O.readers});
}

// ---- F2FRansac / FilterKeypoints for the pairs of a batch: epipolar.hip k_f2f_batch, k_epi_filter
extern "C" int vis_f2f_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts,
                             const float* d_rot, const float* d_tref, const int32_t* d_draws, vis_f2f_result* d_out) {
    if (n < 0 || max_pts < 0 || !d_npts || !d_rot || !d_draws || !d_out || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 3)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    return f2f_batch_run(ctx, n, max_pts, d_p1, d_p2, d_npts, d_rot, d_tref, d_draws, ctx->p.f2f_iters, false, d_out);
}

extern "C" int vis_filter_keypoints_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts,
                                          const float* d_rot, const float* d_t, double threshold, int row_cap, uint8_t* d_keep, int32_t* d_nkeep) {
    if (n < 0 || max_pts < 0 || !d_npts || !d_rot || !d_t || !d_keep || !d_nkeep || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_nkeep & 3) || !std::isfinite(threshold)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (row_cap < max_pts) { ctx->err = "vis_filter_keypoints_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return epi_filter_run(ctx, n, max_pts, d_p1, d_p2, d_npts, d_rot, d_t, threshold, row_cap, d_keep, d_nkeep);
}

// The plan's pairs: the rows k_filter wrote for the pose stage (p1 / p2 of the last step's matcher-output set, ngood or nsym).  On the pose
// stream, behind the matcher of that step (the record set's matcher event, recorded behind the filter: what vis_batch_align waits for) and
// behind the context's stream, where the caller's inputs may have been produced.  The filter two steps on rewrites the set: it waits for
// the reader event noted here; so does, with `links` (the call read the link table of the keyframe gate), the next gate kernel of the record set.
template <class F> static int batch_epi(vis_ctx* ctx, int n, const char* who, F run, bool links = false) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = std::string(who) + ": the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    Plan::MatchOut& O = pl->out();
    return on_pose_stream(ctx, {FU_FORK | FU_MATCHER, ctx->ev_epi_done[pl->mo_cur]},
                          [&] { return run(pl, O, ctx->p.pose_input == VIS_POSE_SYM ? O.nsym : O.ngood); },
                          {&O.readers, links && pl->kf_min ? &pl->last_set().links : nullptr});
}

extern "C" int vis_batch_f2f(vis_ctx* ctx, int n, const float* d_rot, const float* d_tref, const int32_t* d_draws, vis_f2f_result* d_out) {
    if (!d_rot || !d_draws || !d_out || ((uintptr_t)d_out & 3)) return VIS_E_INVALID;
    return batch_epi(ctx, n, "vis_batch_f2f", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return f2f_batch_run(ctx, n, pl->pose_mcap, O.p1, O.p2, d_npts, d_rot, d_tref, d_draws, ctx->p.f2f_iters, false, d_out);
    });
}

extern "C" int vis_batch_filter_keypoints(vis_ctx* ctx, int n, const float* d_rot, const float* d_t, double threshold, int row_cap,
                                          uint8_t* d_keep, int32_t* d_nkeep) {
    if (!d_rot || !d_t || !d_keep || !d_nkeep || ((uintptr_t)d_nkeep & 3) || !std::isfinite(threshold)) return VIS_E_INVALID;
    if (ctx && ctx->batch && row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_filter_keypoints: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    return batch_epi(ctx, n, "vis_batch_filter_keypoints", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return epi_filter_run(ctx, n, pl->pose_mcap, O.p1, O.p2, d_npts, d_rot, d_t, threshold, row_cap, d_keep, d_nkeep);
    });
}

extern "C" int vis_filter_keypoints(vis_ctx* ctx, const vis_keypoint* pts1, const vis_keypoint* pts2, int m, const float rot[9], const float t[3],
                                    double threshold, uint8_t* keep, int* n_keep) {
    if (m < 0 || !rot || !t || !n_keep || (m && (!pts1 || !pts2 || !keep)) || !std::isfinite(threshold)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    *n_keep = 0;
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const size_t mk = ((size_t)m + 3) & ~(size_t)3;
    float *d_p1, *d_p2, *d_rt; int32_t* d_cnt; uint8_t* d_keep;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>((size_t)m * 2); d_p2 = cv.take<float>((size_t)m * 2);
        d_rt = cv.take<float>(12); d_cnt = cv.take<int32_t>(2);                   // rot, t | m, count
        d_keep = cv.take<uint8_t>(mk);
    }, 2);                                                         // (d_cnt goes up and comes down)
    if (rc) return rc;
    std::vector<float> xy((size_t)m * 4);
    for (int i = 0; i < m; i++) { xy[2 * (size_t)i] = pts1[i].x; xy[2 * (size_t)i + 1] = pts1[i].y; xy[2 * ((size_t)m + i)] = pts2[i].x; xy[2 * ((size_t)m + i) + 1] = pts2[i].y; }
    float rt[12]; std::memcpy(rt, rot, 36); std::memcpy(rt + 9, t, 12);
    const int32_t cnt[2] = {m, 0};
    HostStage hs(ctx);
    hs.up(d_p1, xy.data(), (size_t)m * 8);
    hs.up(d_p2, xy.data() + (size_t)m * 2, (size_t)m * 8);
    hs.up(d_rt, rt, sizeof(rt));
    hs.up(d_cnt, cnt, sizeof(cnt));
    hs.flush_ups();
    rc = epi_filter_run(ctx, 1, m, d_p1, d_p2, d_cnt, d_rt, d_rt + 9, threshold, (int)mk, d_keep, d_cnt + 1);
    if (rc) return vis_drain(ctx, rc);
    const void* h_cnt = hs.down(d_cnt, sizeof(cnt));
    const void* h_keep = hs.down(d_keep, mk);
    rc = hs.wait();
    if (rc) return rc;
    *n_keep = ((const int32_t*)h_cnt)[1];
    std::memcpy(keep, h_keep, (size_t)m);
    return VIS_OK;
}

// ---- homography RANSAC and the H-or-E model choice: homography.hip k_homography_batch
extern "C" void vis_default_homography_params(vis_homography_params* hp) {
    if (!hp) return;
    hp->iters = 200; hp->min_inliers = 8;
    hp->chi2_h = 5.991; hp->chi2_e = 3.841; hp->sigma_px = 1.0; hp->h_ratio = 0.40;
}

static bool homography_params_ok(const vis_homography_params* hp) {
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    return hp && hp->iters >= 0 && hp->min_inliers >= 4 && pos(hp->chi2_h) && pos(hp->chi2_e) && pos(hp->sigma_px) &&
           hp->h_ratio > 0.0 && hp->h_ratio < 1.0;
}

static void homography_zero_record(vis_homography_result* r) { std::memset(r, 0, sizeof(*r)); r->best_iter = -1; }

extern "C" int vis_find_homography(vis_ctx* ctx, const vis_homography_params* hp, const float* p1xy, const float* p2xy, int m,
                                   const int32_t* draws, const double* E, uint8_t* mask, vis_homography_result* out) {
    if (!out || m < 0 || (m && (!p1xy || !p2xy)) || !homography_params_ok(hp) || (m && hp->iters && !draws)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    homography_zero_record(out);
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const size_t mk = ((size_t)m + 3) & ~(size_t)3, nd = (size_t)hp->iters * 4;
    float *d_p1, *d_p2; int32_t *d_draws, *d_n; double* d_E; uint8_t* d_mask; vis_homography_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>((size_t)m * 2); d_p2 = cv.take<float>((size_t)m * 2);
        d_draws = cv.take<int32_t>(nd ? nd : 4); d_n = cv.take<int32_t>(1);
        d_E = cv.take<double>(9);
        d_mask = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_homography_result>(1);
    });
    if (rc) return rc;
    const int32_t n1 = m;
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    if (nd) hs.up(d_draws, draws, nd * 4);
    hs.up(d_n, &n1, 4);
    if (E) hs.up(d_E, E, 72);
    hs.flush_ups();
    rc = homography_batch_run(ctx, hp, 1, m, d_p1, d_p2, d_n, d_draws, E ? d_E : nullptr, 9, (int)mk, d_mask, d_out);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out, sizeof(vis_homography_result));
    const void* h_mask = hs.down(d_mask, mk);
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(*out));
    if (mask) std::memcpy(mask, h_mask, (size_t)m);
    return VIS_OK;
}

extern "C" int vis_homography_batch(vis_ctx* ctx, const vis_homography_params* hp, int n, const float* d_p1, const float* d_p2,
                                    const int32_t* d_npts, int max_pts, const int32_t* d_draws, const double* d_E,
                                    int row_cap, uint8_t* d_mask, vis_homography_result* d_out) {
    if (n < 0 || max_pts < 0 || row_cap < 0 || !d_npts || !d_draws || !d_out || (max_pts && (!d_p1 || !d_p2)) || !homography_params_ok(hp)) return VIS_E_INVALID;
    if (((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_E & 7) || ((uintptr_t)d_out & 7)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (d_mask && row_cap < max_pts) { ctx->err = "vis_homography_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return homography_batch_run(ctx, hp, n, max_pts, d_p1, d_p2, d_npts, d_draws, d_E, 9, row_cap, d_mask, d_out);
}

extern "C" int vis_batch_homography(vis_ctx* ctx, const vis_homography_params* hp, int n, const int32_t* d_draws,
                                    int row_cap, uint8_t* d_mask, vis_homography_result* d_out) {
    if (n < 0 || row_cap < 0 || !d_draws || !d_out || ((uintptr_t)d_out & 7) || !homography_params_ok(hp)) return VIS_E_INVALID;
    if (ctx && ctx->batch && d_mask && row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_homography: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    // behind the pose stage of the last run on the pose stream (batch_epi queues there): its records are single-buffered and written on that
    // stream only, and the next pose stage is queued behind this call
    return batch_epi(ctx, n, "vis_batch_homography", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        const bool have_E = (pl->last_stages & VIS_STAGE_POSE) != 0;
        static_assert(sizeof(PoseOut) % 8 == 0 && offsetof(PoseOut, E) == 0, "the pose record begins with E");
        return homography_batch_run(ctx, hp, n, pl->pose_mcap, O.p1, O.p2, d_npts, d_draws, have_E ? (const double*)pl->d_pose : nullptr,
                                    (int)(sizeof(PoseOut) / 8), row_cap, d_mask, d_out);
    });
}

// ---- the pose of a homography: pose.hip k_hpose_svd + k_hpose_vote
extern "C" void vis_default_hpose_params(vis_hpose_params* hq) {
    if (!hq) return;
    hq->min_t_over_d = 0.05; hq->max_cos_parallax = 0.9998476951563913; hq->ambiguity_ratio = 0.75;
    hq->good_share = 0.9; hq->parallax_share = 0.5; hq->min_good = 8; hq->reserved_ = 0;
}

static bool hpose_params_ok(const vis_hpose_params* hq) {
    auto share = [](double v) { return std::isfinite(v) && v > 0.0 && v <= 1.0; };
    return hq && std::isfinite(hq->min_t_over_d) && hq->min_t_over_d >= 0.0 && share(hq->max_cos_parallax) && share(hq->ambiguity_ratio) &&
           share(hq->good_share) && share(hq->parallax_share) && hq->min_good >= 1;
}

extern "C" int vis_homography_pose(vis_ctx* ctx, const vis_hpose_params* hq, const vis_homography_result* h, const float* p1xy, const float* p2xy,
                                   int m, const uint8_t* mask, const float* rot_hint, vis_hpose_result* out) {
    if (!out || !h || m < 0 || (m && (!p1xy || !p2xy)) || !hpose_params_ok(hq)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    std::memset(out, 0, sizeof(*out)); out->solution = out->second = -1;
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const size_t mk = ((size_t)m + 3) & ~(size_t)3;
    float *d_p1, *d_p2, *d_rot; int32_t* d_n; vis_homography_result* d_h; uint8_t* d_mask; vis_hpose_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>((size_t)m * 2); d_p2 = cv.take<float>((size_t)m * 2);
        d_n = cv.take<int32_t>(1);
        d_rot = cv.take<float>(9);
        d_h = cv.take<vis_homography_result>(1);
        d_mask = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_hpose_result>(1);
    });
    if (rc) return rc;
    const int32_t n1 = m;
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    hs.up(d_n, &n1, 4);
    hs.up(d_h, h, sizeof(*h));
    if (rot_hint) hs.up(d_rot, rot_hint, 36);
    if (mask) hs.up(d_mask, mask, (size_t)m);
    hs.flush_ups();
    rc = hpose_run(ctx, hq, 1, m, d_h, d_p1, d_p2, d_n, (int)mk, mask ? d_mask : nullptr, rot_hint ? d_rot : nullptr, d_out);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out, sizeof(vis_hpose_result));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(*out));
    return VIS_OK;
}

extern "C" int vis_homography_pose_batch(vis_ctx* ctx, const vis_hpose_params* hq, int n, const vis_homography_result* d_h, const float* d_p1,
                                         const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask,
                                         const float* d_rot, vis_hpose_result* d_out) {
    if (n < 0 || max_pts < 0 || row_cap < 0 || !d_h || !d_npts || !d_out || (max_pts && (!d_p1 || !d_p2)) || !hpose_params_ok(hq)) return VIS_E_INVALID;
    if (((uintptr_t)d_h & 7) || ((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_npts & 3) || ((uintptr_t)d_rot & 3)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (d_mask && row_cap < max_pts) { ctx->err = "vis_homography_pose_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return hpose_run(ctx, hq, n, max_pts, d_h, d_p1, d_p2, d_npts, row_cap, d_mask, d_rot, d_out);
}

extern "C" int vis_batch_homography_pose(vis_ctx* ctx, const vis_hpose_params* hq, int n, const vis_homography_result* d_h, int row_cap,
                                         const uint8_t* d_mask, const float* d_rot, vis_hpose_result* d_out) {
    if (n < 0 || row_cap < 0 || !d_h || !d_out || ((uintptr_t)d_h & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_rot & 3) || !hpose_params_ok(hq)) return VIS_E_INVALID;
    if (ctx && ctx->batch && d_mask && row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_homography_pose: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    // on the pose stream behind vis_batch_homography of the same run (batch_epi queues there): d_h and d_mask are complete when the kernels read them
    return batch_epi(ctx, n, "vis_batch_homography_pose", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return hpose_run(ctx, hq, n, pl->pose_mcap, d_h, O.p1, O.p2, d_npts, row_cap, d_mask, d_rot, d_out);
    });
}

// ---- PnP: pnp.hip k_pnp_batch + k_pnp_refine
extern "C" void vis_default_pnp_params(vis_pnp_params* pp) {
    if (!pp) return;
    pp->iters = 200; pp->min_inliers = 8; pp->threshold_px = 2.0; pp->refine_iters = 5; pp->reserved_ = 0;
}

static bool pnp_params_ok(const vis_pnp_params* pp) {
    return pp && pp->iters >= 0 && pp->iters <= (1 << 29) && pp->min_inliers >= 4 && pp->refine_iters >= 0 &&
           std::isfinite(pp->threshold_px) && pp->threshold_px > 0.0;
}

extern "C" int vis_pnp_ransac(vis_ctx* ctx, const vis_pnp_params* pp, const double* X, const float* xy, int m, const int32_t* draws,
                              uint8_t* mask, vis_pnp_result* out) {
    if (!out || m < 0 || (m && (!X || !xy)) || !pnp_params_ok(pp) || (m && pp->iters && !draws)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    std::memset(out, 0, sizeof(*out)); out->best_iter = -1;
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const size_t mk = ((size_t)m + 3) & ~(size_t)3, nd = (size_t)pp->iters * 3;
    double* d_X; float* d_xy; int32_t *d_draws, *d_n; uint8_t* d_mask; vis_pnp_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_X = cv.take<double>((size_t)m * 3); d_xy = cv.take<float>((size_t)m * 2);
        d_draws = cv.take<int32_t>(nd ? nd : 3); d_n = cv.take<int32_t>(1);
        d_mask = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_pnp_result>(1);
    });
    if (rc) return rc;
    const int32_t n1 = m;
    HostStage hs(ctx);
    hs.up(d_X, X, (size_t)m * 24);
    hs.up(d_xy, xy, (size_t)m * 8);
    if (nd) hs.up(d_draws, draws, nd * 4);
    hs.up(d_n, &n1, 4);
    hs.flush_ups();
    rc = pnp_batch_run(ctx, pp, 1, m, d_X, 3, d_xy, d_n, d_draws, (int)mk, d_mask, d_out);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out, sizeof(vis_pnp_result));
    const void* h_mask = hs.down(d_mask, mk);
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(*out));
    if (mask) std::memcpy(mask, h_mask, (size_t)m);
    return VIS_OK;
}

extern "C" int vis_pnp_batch(vis_ctx* ctx, const vis_pnp_params* pp, int n, const double* d_X, int x_stride, const float* d_xy,
                             const int32_t* d_npts, int max_pts, const int32_t* d_draws, int row_cap, uint8_t* d_mask, vis_pnp_result* d_out) {
    if (n < 0 || max_pts < 0 || row_cap < 0 || x_stride < 3 || !d_npts || !d_draws || !d_out || (max_pts && (!d_X || !d_xy)) || !pnp_params_ok(pp)) return VIS_E_INVALID;
    if (((uintptr_t)d_X & 7) || ((uintptr_t)d_xy & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_npts & 3) || ((uintptr_t)d_draws & 3)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (d_mask && row_cap < max_pts) { ctx->err = "vis_pnp_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return pnp_batch_run(ctx, pp, n, max_pts, d_X, x_stride, d_xy, d_npts, d_draws, row_cap, d_mask, d_out);
}

// A plan's lazily allocated block (Plan::d_pnp_ws, d_ft_ws, d_tj_ws, d_imu_ws, d_imuj_ws, d_imuc_ws, d_via_ws, d_viab_ws), in ONE place: the list is measured and the block allocated by the
// first call of the plan that needs it; every call binds the list to the block, into a work struct of its own.  The block is never replaced.
template <class Layout> static int plan_block(vis_ctx* ctx, void*& block, const char* who, Layout&& layout) {
    if (!block) {
        Carver measure{nullptr, 0, SIZE_MAX};
        layout(measure);
        if (measure.overflow) { ctx->err = std::string(who) + ": the plan's workspace exceeds the address space"; return VIS_E_NOMEM; }
        if (hipMalloc(&block, measure.off + 256) != hipSuccess) {
            (void)hipGetLastError(); block = nullptr;
            ctx->err = std::string(who) + ": out of device memory for the plan's workspace"; return VIS_E_NOMEM;
        }
    }
    Carver cv{(char*)block, 0, SIZE_MAX};
    layout(cv);
    return VIS_OK;
}

struct PnpPlanWork { int32_t* tab; double* X; float* xy; int32_t* n; };
static int ensure_pnp(vis_ctx* ctx, Plan* pl, PnpPlanWork& W) {
    return plan_block(ctx, pl->d_pnp_ws, "vis_batch_pnp", [&](Carver& cv) {
        W.tab = cv.take<int32_t>((size_t)pl->npairs * pl->kcap);
        W.X = cv.take<double>((size_t)pl->npairs * pl->pose_mcap * 3);
        W.xy = cv.take<float>((size_t)pl->npairs * pl->pose_mcap * 2);
        W.n = cv.take<int32_t>((size_t)pl->npairs);
    });
}

extern "C" int vis_batch_pnp(vis_ctx* ctx, const vis_pnp_params* pp, int n, const int32_t* d_draws, const vis_map_point* d_points,
                             const uint8_t* d_flags, int row_cap, int require, int mask_cap, uint8_t* d_mask, vis_pnp_result* d_out,
                             vis_pnp_link* d_link) {
    if (n < 0 || row_cap < 0 || mask_cap < 0 || require < 0 || require > 255 || !d_draws || !d_points || !d_flags || !d_out || !d_link ||
        !pnp_params_ok(pp)) return VIS_E_INVALID;
    if (((uintptr_t)d_points & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_link & 7) || ((uintptr_t)d_draws & 3)) return VIS_E_INVALID;
    if (ctx && ctx->batch && row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_pnp: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    if (ctx && ctx->batch && d_mask && mask_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_pnp: mask_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    if (!(ctx->batch->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_pnp: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (ctx->batch->last_n < 1 || n != ctx->batch->last_n) return VIS_E_STATE;    // (before the workspace is allocated)
    (void)hipSetDevice(ctx->device);
    PnpPlanWork W;
    { const int rc = ensure_pnp(ctx, ctx->batch, W); if (rc) return rc; }
    // on the pose stream (batch_epi queues there) behind the pose stage that wrote the pose records and behind vis_batch_triangulate of the same
    // run, which wrote d_points / d_flags on that stream; the link table is read there too: the next gate kernel of the record set waits for it
    return batch_epi(ctx, n, "vis_batch_pnp", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        const bool sym = ctx->p.pose_input == VIS_POSE_SYM;
        return pnp_link_run(ctx, pp, n, pl->kf_min ? pl->last_set().kf_link : nullptr, pl->pair0_valid ? 1 : 0, pl->pose_mcap, sym ? pl->kcap : pl->root * pl->root,
                            pl->kcap, sym ? O.sym : O.good, d_npts, O.p2, pl->d_pose, d_points, d_flags, row_cap, require, W.tab, W.X,
                            W.xy, W.n, d_draws, mask_cap, d_mask, d_out, d_link);
    }, true);
}

// ---- feature tracks: ftrack.hip
static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int vis_ftrack_link_rows(vis_ctx* ctx, int n, const int32_t* d_prev, const int32_t* d_nkp, const vis_dmatch* d_links, const int32_t* d_nlinks,
                                    int link_cap, const uint8_t* d_mask, int mask_cap, const vis_ftrack_obs* d_carry_in, int seq0, int row_cap,
                                    vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame) {
    if (!d_prev || !d_nkp || !d_nlinks || !d_obs || !d_frame || (link_cap > 0 && !d_links)) return VIS_E_INVALID;
    if (!aligned(d_links, 16) || !aligned(d_carry_in, 16) || !aligned(d_obs, 16) || !aligned(d_prev, 4) || !aligned(d_nkp, 4) || !aligned(d_nlinks, 4) ||
        !aligned(d_frame, 4)) return VIS_E_INVALID;
    if (n < 0 || link_cap < 0 || mask_cap < 0 || row_cap < 0 || seq0 < 0) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28)) { ctx->err = "vis_ftrack_link_rows: n x row_cap exceeds 2^28 entries"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    FtWork W;
    const int rc = vis_carve_block(ctx, ctx->ft_ws, "vis_ftrack_link_rows", [&](Carver& cv) { W.layout(cv, (size_t)n, (size_t)row_cap); }, 256);
    if (rc) return rc;
    return ftrack_link_run(ctx, W, n, row_cap, FtFrames{d_prev, 0, d_nkp}, d_links, d_nlinks, link_cap, d_mask, mask_cap, nullptr, 0, d_carry_in, seq0,
                           row_cap, row_cap, d_obs, d_frame, nullptr);
}

// the plan's workspace: FtWork for B frames of kcap keypoints and, behind it, the two carried rows -- one list, measured and then bound
struct FtPlanWork { FtWork ft; vis_ftrack_obs* carry[2]; };
static int ensure_ftrack(vis_ctx* ctx, Plan* pl, FtPlanWork& W) {
    return plan_block(ctx, pl->d_ft_ws, "vis_batch_ftrack", [&](Carver& cv) {
        W.ft.layout(cv, (size_t)pl->B, (size_t)pl->kcap);
        W.carry[0] = cv.take<vis_ftrack_obs>((size_t)pl->kcap); W.carry[1] = cv.take<vis_ftrack_obs>((size_t)pl->kcap);
    });
}

// the pairing of the last run as the kernels read it: the gate's link table, or the gate-off rule; the counts of its frames
static FtFrames plan_frames(Plan* pl) {
    return FtFrames{pl->kf_min ? pl->last_set().kf_link : nullptr, pl->pair0_valid ? 1 : 0, pl->d_nkp + pl->last_base + 1};
}

extern "C" int vis_batch_ftrack(vis_ctx* ctx, int source, int pose_inliers, int n, const uint8_t* d_mask, int mask_cap, int row_cap,
                                vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame) {
    if (!d_obs || !d_frame || !aligned(d_obs, 16) || !aligned(d_frame, 4) || n < 0 || mask_cap < 0 || row_cap < 0 ||
        (source != VIS_FT_SYM && source != VIS_FT_GOOD) || (pose_inliers && d_mask)) return VIS_E_INVALID;
    if (ctx && ctx->batch) {
        Plan* pl = ctx->batch;
        if (row_cap < pl->kcap) { ctx->err = "vis_batch_ftrack: row_cap is smaller than the plan's keypoint capacity"; return VIS_E_CAPACITY; }
        if (d_mask && mask_cap < (source == VIS_FT_SYM ? pl->kcap : pl->root * pl->root)) { ctx->err = "vis_batch_ftrack: mask_cap is smaller than the list's row length"; return VIS_E_CAPACITY; }
    }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_ftrack: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    const bool pose_sym = ctx->p.pose_input == VIS_POSE_SYM;
    if (pose_inliers && (!(pl->last_stages & VIS_STAGE_POSE) || (source == VIS_FT_SYM) != pose_sym)) {
        ctx->err = "vis_batch_ftrack: pose_inliers needs VIS_STAGE_POSE and the list the pose stage saw"; return VIS_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    FtPlanWork W;
    { const int rc = ensure_ftrack(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick row = pl->ft.pick(pl->run_count);
    Plan::MatchOut& O = pl->out();
    // On the pose stream behind the matcher of the run (the lists and counts of its matcher-output set, the keypoint counts of its record set, the
    // gate's link table) and, with a caller's mask, behind the context's stream; the pose stage's mask and records are written on the pose stream
    // itself.  The writers of those buffers wait for the reader event noted here.
    const int rc = on_pose_stream(ctx, {(unsigned)(FU_MATCHER | (d_mask ? FU_FORK : 0)), ctx->ev_epi_done[pl->mo_cur]}, [&] {
        const bool sym = source == VIS_FT_SYM;
        static_assert(sizeof(PoseOut) % 4 == 0 && offsetof(PoseOut, n_points) % 4 == 0, "the pose record's n_points as a strided int32");
        const int rc2 = ftrack_link_run(ctx, W.ft, n, pl->kcap, plan_frames(pl), sym ? O.sym : O.good, sym ? O.nsym : O.ngood, sym ? pl->kcap : pl->root * pl->root,
                                        pose_inliers ? pl->d_mask : d_mask, pose_inliers ? pl->pose_mcap : mask_cap,
                                        pose_inliers ? (const int32_t*)((const char*)pl->d_pose + offsetof(PoseOut, n_points)) : nullptr, (int)(sizeof(PoseOut) / 4),
                                        row.have ? W.carry[row.slot] : nullptr, pl->seq0, row_cap, pl->kcap, d_obs, d_frame, W.carry[row.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, {&O.readers, &pl->last_set().matcher, pl->kf_min ? &pl->last_set().links : nullptr});
    if (rc) return rc;
    pl->ft.commit(row, pl->run_count);
    return VIS_OK;
}

extern "C" void vis_default_ftrack_tri_params(vis_ftrack_tri_params* tp) {
    if (!tp) return;
    tp->max_views = 16; tp->min_views = 2; tp->gn_iters = 5; tp->reserved_ = 0; tp->max_reproj_px = 2.0; tp->max_parallax_cos = 0.9998476951563913;
}

static bool ftrack_tri_params_ok(const vis_ftrack_tri_params* tp) {
    return tp && tp->max_views >= 2 && tp->max_views <= 32 && tp->min_views >= 2 && tp->min_views <= tp->max_views && tp->gn_iters >= 0 && tp->gn_iters <= 10 &&
           std::isfinite(tp->max_reproj_px) && tp->max_reproj_px > 0.0 && tp->max_reproj_px <= 1e6 && tp->max_parallax_cos > -1.0 && tp->max_parallax_cos <= 1.0;
}

extern "C" int vis_ftrack_triangulate_rows(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, const int32_t* d_prev, const int32_t* d_nkp,
                                           const vis_ftrack_obs* d_obs, int row_cap, const float* d_xy, const double* d_poses, vis_ftrack_point* d_points,
                                           uint8_t* d_flags, vis_ftrack_tri_summary* d_summary) {
    if (!ftrack_tri_params_ok(tp) || !d_prev || !d_nkp || !d_obs || !d_xy || !d_poses || !d_points || !d_flags || !d_summary) return VIS_E_INVALID;
    if (!aligned(d_obs, 16) || !aligned(d_xy, 8) || !aligned(d_poses, 8) || !aligned(d_points, 8) || !aligned(d_prev, 4) || !aligned(d_nkp, 4) ||
        !aligned(d_summary, 4) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28)) { ctx->err = "vis_ftrack_triangulate_rows: n x row_cap exceeds 2^28 entries"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return ftrack_triangulate_run(ctx, tp, n, row_cap, FtFrames{d_prev, 0, d_nkp}, d_obs, row_cap, d_xy, (size_t)row_cap * 8, 8, d_poses, d_points, d_flags,
                                  d_summary);
}

extern "C" int vis_batch_ftrack_triangulate(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, const vis_ftrack_obs* d_obs, int row_cap,
                                            const double* d_poses, vis_ftrack_point* d_points, uint8_t* d_flags, vis_ftrack_tri_summary* d_summary) {
    if (!ftrack_tri_params_ok(tp) || !d_obs || !d_poses || !d_points || !d_flags || !d_summary || !aligned(d_obs, 16) || !aligned(d_poses, 8) ||
        !aligned(d_points, 8) || !aligned(d_summary, 4) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (ctx && ctx->batch && row_cap < ctx->batch->kcap) { ctx->err = "vis_batch_ftrack_triangulate: row_cap is smaller than the plan's keypoint capacity"; return VIS_E_CAPACITY; }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_ftrack_triangulate: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28)) { ctx->err = "vis_batch_ftrack_triangulate: n x row_cap exceeds 2^28 entries"; return VIS_E_CAPACITY; }
    // on the pose stream behind vis_batch_ftrack of the run (queued there), behind the matcher that saw the keypoints and behind the context's
    // stream, where the caller's poses may have been produced; the keypoint records and the link table are read: their writers wait for the event
    static_assert(offsetof(vis_keypoint, x) == 0 && offsetof(vis_keypoint, y) == 4, "a keypoint record begins with its pixel");
    return on_pose_stream(ctx, {FU_FORK | FU_MATCHER, ctx->ev_epi_done[pl->mo_cur]}, [&] {
        const int rc2 = ftrack_triangulate_run(ctx, tp, n, pl->kcap, plan_frames(pl), d_obs, row_cap, pl->d_kps + (size_t)(pl->last_base + 1) * pl->kcap,
                                               (size_t)pl->kcap * sizeof(vis_keypoint), (int)sizeof(vis_keypoint), d_poses, d_points, d_flags, d_summary);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, {&pl->out().readers, &pl->last_set().matcher, pl->kf_min ? &pl->last_set().links : nullptr});
}

// ---- windowed bundle adjustment over the tracks: ba.hip
extern "C" void vis_default_ba_params(vis_ba_params* bp) {
    if (!bp) return;
    bp->stride = 8; bp->min_views = 2; bp->min_points = 12; bp->lm_iters = 10; bp->tri_gn_iters = 5; bp->reserved_ = 0;
    bp->huber_px = 2.4477; bp->init_reproj_px = 16.0; bp->lambda0 = 1e-4;
}

static bool ba_params_ok(const vis_ba_params* bp) {
    return bp && bp->stride >= 1 && bp->stride <= 16 && bp->min_views >= 2 && bp->min_views <= 17 && bp->min_points >= 1 && bp->lm_iters >= 0 &&
           bp->lm_iters <= 30 && bp->tri_gn_iters >= 0 && bp->tri_gn_iters <= 10 && std::isfinite(bp->huber_px) && bp->huber_px >= 0.0 &&
           std::isfinite(bp->init_reproj_px) && bp->init_reproj_px > 0.0 && bp->init_reproj_px <= 1e6 && bp->lambda0 >= 1e-12 && bp->lambda0 <= 1e12;
}

extern "C" int vis_ba_rows(vis_ctx* ctx, const vis_ba_params* bp, int n, const int32_t* d_prev, const int32_t* d_nkp, const vis_ftrack_obs* d_obs,
                           int row_cap, const float* d_xy, const double* d_poses, double* d_poses_out, vis_ba_window* d_windows, vis_ba_point* d_points,
                           uint8_t* d_flags) {
    if (!ba_params_ok(bp) || !d_prev || !d_nkp || !d_obs || !d_xy || !d_poses || !d_poses_out || !d_windows || !d_points || !d_flags) return VIS_E_INVALID;
    if (!aligned(d_obs, 16) || !aligned(d_xy, 8) || !aligned(d_poses, 8) || !aligned(d_poses_out, 8) || !aligned(d_windows, 8) || !aligned(d_points, 8) ||
        !aligned(d_prev, 4) || !aligned(d_nkp, 4) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28)) { ctx->err = "vis_ba_rows: n x row_cap exceeds 2^28 entries"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return ba_run(ctx, bp, n, row_cap, FtFrames{d_prev, 0, d_nkp}, d_obs, row_cap, d_xy, (size_t)row_cap * 8, 8, d_poses, d_poses_out, d_windows, d_points,
                  d_flags);
}

extern "C" int vis_batch_ba(vis_ctx* ctx, const vis_ba_params* bp, int n, const vis_ftrack_obs* d_obs, int row_cap, const double* d_poses,
                            double* d_poses_out, vis_ba_window* d_windows, vis_ba_point* d_points, uint8_t* d_flags) {
    if (!ba_params_ok(bp) || !d_obs || !d_poses || !d_poses_out || !d_windows || !d_points || !d_flags || !aligned(d_obs, 16) || !aligned(d_poses, 8) ||
        !aligned(d_poses_out, 8) || !aligned(d_windows, 8) || !aligned(d_points, 8) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_ba: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if (row_cap < pl->kcap) { ctx->err = "vis_batch_ba: row_cap is smaller than the plan's keypoint capacity"; return VIS_E_CAPACITY; }
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28)) { ctx->err = "vis_batch_ba: n x row_cap exceeds 2^28 entries"; return VIS_E_CAPACITY; }
    // queued exactly as vis_batch_ftrack_triangulate: on the pose stream behind vis_batch_ftrack of the run, behind the matcher that saw the keypoints
    // and behind the context's stream, where the caller's poses may have been produced; nothing of the plan is written
    return on_pose_stream(ctx, {FU_FORK | FU_MATCHER, ctx->ev_epi_done[pl->mo_cur]}, [&] {
        const int rc2 = ba_run(ctx, bp, n, pl->kcap, plan_frames(pl), d_obs, row_cap, pl->d_kps + (size_t)(pl->last_base + 1) * pl->kcap,
                               (size_t)pl->kcap * sizeof(vis_keypoint), (int)sizeof(vis_keypoint), d_poses, d_poses_out, d_windows, d_points, d_flags);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, {&pl->out().readers, &pl->last_set().matcher, pl->kf_min ? &pl->last_set().links : nullptr});
}

// ---- scale links and the chained trajectory: trajectory.hip
extern "C" void vis_default_scale_link_params(vis_scale_link_params* sp) {
    if (!sp) return;
    sp->require = VIS_MP_KEPT; sp->min_shared = 8; sp->max_rel_spread = 1.0; sp->min_scale = 1.0 / 64.0; sp->max_scale = 64.0;
}

static bool scale_link_params_ok(const vis_scale_link_params* sp) {
    return sp && sp->require >= 0 && sp->require <= 255 && sp->min_shared >= 1 && sp->min_shared <= (1 << 20) && std::isfinite(sp->max_rel_spread) &&
           sp->max_rel_spread >= 0.0 && sp->max_rel_spread <= 1e6 && std::isfinite(sp->min_scale) && std::isfinite(sp->max_scale) && sp->min_scale > 0.0 &&
           sp->min_scale <= sp->max_scale;
}

extern "C" int vis_scale_link_rows(vis_ctx* ctx, const vis_scale_link_params* sp, int n, const int32_t* d_prev, const vis_dmatch* d_links,
                                   const int32_t* d_nlinks, int link_cap, const vis_pose_result* d_pose, const vis_map_point* d_points,
                                   const uint8_t* d_flags, int pts_cap, const double* d_depth_carry_in, int row_cap, double* d_depth,
                                   vis_scale_link* d_link) {
    if (!scale_link_params_ok(sp) || !d_prev || !d_nlinks || !d_pose || !d_depth || !d_link) return VIS_E_INVALID;
    if (std::min(link_cap, pts_cap) > 0 && (!d_links || !d_points || !d_flags)) return VIS_E_INVALID;
    if (!aligned(d_links, 16) || !aligned(d_points, 16) || !aligned(d_pose, 8) || !aligned(d_depth, 8) || !aligned(d_depth_carry_in, 8) || !aligned(d_link, 8) ||
        !aligned(d_prev, 4) || !aligned(d_nlinks, 4)) return VIS_E_INVALID;
    if (n < 0 || link_cap < 0 || pts_cap < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if ((size_t)n * (size_t)row_cap > ((size_t)1 << 28) || (size_t)n * (size_t)link_cap > ((size_t)1 << 28)) {
        ctx->err = "vis_scale_link_rows: n x row_cap or n x link_cap exceeds 2^28 entries"; return VIS_E_CAPACITY;
    }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const int mcap = std::min(link_cap, pts_cap);
    SlWork W;
    const int rc = vis_carve_block(ctx, ctx->sl_ws, "vis_scale_link_rows", [&](Carver& cv) { W.layout(cv, (size_t)n, (size_t)mcap); });
    if (rc) return rc;
    return scale_link_run(ctx, sp, n, FtFrames{d_prev, 0, nullptr}, d_links, d_nlinks, link_cap, mcap, d_pose, d_points, d_flags, pts_cap, d_depth_carry_in,
                          row_cap, d_depth, W.keys, d_link, nullptr);
}

extern "C" int vis_trajectory_rows(vis_ctx* ctx, int n, const int32_t* d_prev, const vis_pose_result* d_pose, const vis_scale_link* d_link,
                                   const vis_traj_pose* d_carry_in, int seq0, int same_epoch_only, vis_traj_pose* d_traj, double* d_poses) {
    if (!d_prev || !d_pose || !d_link || !d_traj) return VIS_E_INVALID;
    if (!aligned(d_pose, 8) || !aligned(d_link, 8) || !aligned(d_carry_in, 8) || !aligned(d_traj, 8) || !aligned(d_poses, 8) || !aligned(d_prev, 4)) return VIS_E_INVALID;
    if (n < 0 || seq0 < 0) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_TJ_MAX_FRAMES) { ctx->err = "vis_trajectory_rows: more than VIS_TJ_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    TjWork W;
    const int rc = vis_carve_block(ctx, ctx->tjr_ws, "vis_trajectory_rows", [&](Carver& cv) { W.layout(cv, (size_t)n); });
    if (rc) return rc;
    return trajectory_run(ctx, n, FtFrames{d_prev, 0, nullptr}, d_pose, d_link, d_carry_in, seq0, same_epoch_only, W.D, W.I, d_traj, d_poses, nullptr);
}

// the plan's block: one list, measured and then bound
struct TrajPlanWork { double* depth; double* sl_carry[2]; SlWork sl; TjWork tj; vis_traj_pose* tj_carry[2]; };
static int ensure_traj(vis_ctx* ctx, Plan* pl, TrajPlanWork& W) {
    return plan_block(ctx, pl->d_tj_ws, "vis_batch_scale_links / vis_batch_trajectory", [&](Carver& cv) {
        W.depth = cv.take<double>((size_t)pl->B * pl->kcap);
        W.sl_carry[0] = cv.take<double>((size_t)pl->kcap); W.sl_carry[1] = cv.take<double>((size_t)pl->kcap);
        W.sl.layout(cv, (size_t)pl->B, (size_t)pl->pose_mcap);
        W.tj.layout(cv, (size_t)pl->B);
        W.tj_carry[0] = cv.take<vis_traj_pose>(1); W.tj_carry[1] = cv.take<vis_traj_pose>(1);
    });
}

extern "C" int vis_batch_scale_links(vis_ctx* ctx, const vis_scale_link_params* sp, int n, const vis_map_point* d_points, const uint8_t* d_flags,
                                     int row_cap, vis_scale_link* d_link) {
    if (!scale_link_params_ok(sp) || !d_points || !d_flags || !d_link || !aligned(d_points, 16) || !aligned(d_link, 8) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (ctx && ctx->batch && row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_scale_links: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_scale_links: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;        // (before the workspace is allocated)
    (void)hipSetDevice(ctx->device);
    TrajPlanWork W;
    { const int rc = ensure_traj(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick row = pl->sl.pick(pl->run_count);
    // on the pose stream behind the pose stage and vis_batch_triangulate of the run, like vis_batch_pnp; the link table is read there too
    const int rc = batch_epi(ctx, n, "vis_batch_scale_links", [&](Plan* pl_, Plan::MatchOut& O, const int32_t* d_npts) {
        const bool sym = ctx->p.pose_input == VIS_POSE_SYM;
        const int rc2 = scale_link_run(ctx, sp, n, plan_frames(pl_), sym ? O.sym : O.good, d_npts, sym ? pl_->kcap : pl_->root * pl_->root, pl_->pose_mcap, pl_->d_pose,
                                       d_points, d_flags, row_cap, row.have ? W.sl_carry[row.slot] : nullptr, pl_->kcap, W.depth, W.sl.keys, d_link, W.sl_carry[row.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->sl.commit(row, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_trajectory(vis_ctx* ctx, int n, const vis_scale_link* d_link, int same_epoch_only, vis_traj_pose* d_traj, double* d_poses) {
    if (!d_link || !d_traj || !aligned(d_link, 8) || !aligned(d_traj, 8) || !aligned(d_poses, 8) || n < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_trajectory: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_TJ_MAX_FRAMES) { ctx->err = "vis_batch_trajectory: more than VIS_TJ_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    TrajPlanWork W;
    { const int rc = ensure_traj(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->tj.pick(pl->run_count);
    // on the pose stream behind vis_batch_scale_links of the run, which wrote d_link there, and behind the pose stage
    const int rc = batch_epi(ctx, n, "vis_batch_trajectory", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = trajectory_run(ctx, n, plan_frames(pl_), pl_->d_pose, d_link, rec.have ? W.tj_carry[rec.slot] : nullptr, pl_->seq0, same_epoch_only, W.tj.D, W.tj.I,
                                       d_traj, d_poses, W.tj_carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->tj.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_trajectory_init(vis_ctx* ctx, const vis_traj_pose* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a chain kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    TrajPlanWork W;
    { const int rc = ensure_traj(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->tj.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.tj_carry[pl->tj.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->tj.seeded(pl->run_count);
    return VIS_OK;
}

// ---- IMU preintegration: imu.hip
extern "C" void vis_default_imu_params(vis_imu_params* ip) {
    if (!ip) return;
    for (int k = 0; k < 3; k++) ip->bg[k] = ip->ba[k] = 0.0;
    for (int k = 0; k < 9; k++) ip->r_ic[k] = (k & 3) == 0 ? 1.0 : 0.0;
    ip->max_gap_s = 0.05; ip->max_angle = 1.0;
}

static bool imu_params_ok(const vis_imu_params* ip) {
    if (!ip) return false;
    for (int k = 0; k < 3; k++) if (!std::isfinite(ip->bg[k]) || !std::isfinite(ip->ba[k])) return false;
    for (int k = 0; k < 9; k++) if (!std::isfinite(ip->r_ic[k])) return false;
    return std::isfinite(ip->max_gap_s) && std::isfinite(ip->max_angle) && ip->max_gap_s > 0.0 && ip->max_angle > 0.0;
}

extern "C" int vis_imu_preintegrate_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                                         const int32_t* d_prev, const vis_imu_carry* d_carry_in, vis_imu_delta* d_delta, float* d_rot,
                                         vis_imu_carry* d_carry_out) {
    if (!imu_params_ok(ip) || !d_tframe || !d_prev || !d_delta || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_carry_in, 8) || !aligned(d_delta, 8) || !aligned(d_carry_out, 8) || !aligned(d_prev, 4) ||
        !aligned(d_rot, 4)) return VIS_E_INVALID;
    if (n < 0 || n_samples < 0 || (d_carry_out && d_carry_out == d_carry_in)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES) { ctx->err = "vis_imu_preintegrate_rows: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const int rc = vis_grow_block(ctx, ctx->imu_ws, imu_table_bytes(n), "vis_imu_preintegrate_rows");
    if (rc) return rc;
    return imu_launch(ctx, ip, n, FtFrames{d_prev, 0, nullptr}, d_samples, n_samples, d_tframe, d_carry_in, ctx->imu_ws.p, d_delta, d_rot, d_carry_out);
}

extern "C" int vis_imu_preintegrate(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_sample* samples, int n_samples, double t_a, double t_b,
                                    vis_imu_delta* delta, float* rot) {
    if (!imu_params_ok(ip) || !delta || n_samples < 0 || (n_samples > 0 && !samples)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    int rc = vis_grow_block(ctx, ctx->imu_ws, imu_table_bytes(1), "vis_imu_preintegrate");
    if (rc) return rc;
    vis_imu_sample* d_s; double* d_t; int32_t* d_prev; vis_imu_carry* d_c; vis_imu_delta* d_d; float* d_r;
    rc = vis_carve(ctx, [&](Carver& cv) {
        d_s = cv.take<vis_imu_sample>((size_t)std::max(n_samples, 1)); d_t = cv.take<double>(1); d_prev = cv.take<int32_t>(1);
        d_c = cv.take<vis_imu_carry>(1); d_d = cv.take<vis_imu_delta>(1); d_r = cv.take<float>(9);
    });
    if (rc) return rc;
    vis_imu_carry c;
    std::memset(&c, 0, sizeof(c));
    c.t_last = t_a; c.valid = VIS_IMU_CARRY_TIME;
    const int32_t prev = VIS_KF_CARRIED;
    HostStage hs(ctx);
    hs.up(d_s, samples, (size_t)n_samples * sizeof(vis_imu_sample));
    hs.up(d_t, &t_b, sizeof(t_b));
    hs.up(d_prev, &prev, sizeof(prev));
    hs.up(d_c, &c, sizeof(c));
    hs.flush_ups();
    rc = imu_launch(ctx, ip, 1, FtFrames{d_prev, 0, nullptr}, d_s, n_samples, d_t, d_c, ctx->imu_ws.p, d_d, d_r, nullptr);
    if (rc) return vis_drain(ctx, rc);
    const void* h_d = hs.down(d_d, sizeof(vis_imu_delta));
    const void* h_r = hs.down(d_r, 9 * sizeof(float));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(delta, h_d, sizeof(vis_imu_delta));
    if (rot) std::memcpy(rot, h_r, 9 * sizeof(float));
    return VIS_OK;
}

// the plan's block: the lifting table for B frames and the two carried records
struct ImuPlanWork { void* table; vis_imu_carry* carry[2]; };
static int ensure_imu(vis_ctx* ctx, Plan* pl, ImuPlanWork& W) {
    return plan_block(ctx, pl->d_imu_ws, "vis_batch_imu", [&](Carver& cv) {
        W.table = cv.take<char>(imu_table_bytes(pl->B)); W.carry[0] = cv.take<vis_imu_carry>(1); W.carry[1] = cv.take<vis_imu_carry>(1);
    });
}

extern "C" int vis_batch_imu(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                             vis_imu_delta* d_delta, float* d_rot) {
    if (!imu_params_ok(ip) || !d_tframe || !d_delta || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_delta, 8) || !aligned(d_rot, 4) || n < 0 || n_samples < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_imu: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES || n > pl->B) { ctx->err = "vis_batch_imu: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    ImuPlanWork W;
    { const int rc = ensure_imu(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->imu.pick(pl->run_count);
    // on the pose stream behind the matcher of the run (the gate's link table) and behind the context's stream (the caller's samples and times)
    const int rc = batch_epi(ctx, n, "vis_batch_imu", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = imu_launch(ctx, ip, n, plan_frames(pl_), d_samples, n_samples, d_tframe, rec.have ? W.carry[rec.slot] : nullptr, W.table, d_delta, d_rot,
                                   W.carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->imu.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_imu_init(vis_ctx* ctx, const vis_imu_carry* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    ImuPlanWork W;
    { const int rc = ensure_imu(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->imu.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.carry[pl->imu.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->imu.seeded(pl->run_count);
    return VIS_OK;
}

// ---- the same three calls with the bias Jacobians of v and p (k_imu_intervals<true>, k_imu_pairs<true>, a table and carried records of their own), and
// the first-order bias correction of the records (k_imu_correct)
extern "C" int vis_imu_preintegrate_jac_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                                             const int32_t* d_prev, const vis_imu_jac_carry* d_carry_in, vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac,
                                             float* d_rot, vis_imu_jac_carry* d_carry_out) {
    if (!imu_params_ok(ip) || !d_tframe || !d_prev || !d_delta || !d_jac || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_carry_in, 8) || !aligned(d_delta, 8) || !aligned(d_jac, 8) || !aligned(d_carry_out, 8) ||
        !aligned(d_prev, 4) || !aligned(d_rot, 4)) return VIS_E_INVALID;
    if (n < 0 || n_samples < 0 || (d_carry_out && d_carry_out == d_carry_in)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES) { ctx->err = "vis_imu_preintegrate_jac_rows: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const int rc = vis_grow_block(ctx, ctx->imuj_ws, imu_jac_table_bytes(n), "vis_imu_preintegrate_jac_rows");
    if (rc) return rc;
    return imu_jac_launch(ctx, ip, n, FtFrames{d_prev, 0, nullptr}, d_samples, n_samples, d_tframe, d_carry_in, ctx->imuj_ws.p, d_delta, d_jac, d_rot, d_carry_out);
}

extern "C" int vis_imu_preintegrate_jac(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_sample* samples, int n_samples, double t_a, double t_b,
                                        vis_imu_delta* delta, vis_imu_bias_jac* jac, float* rot) {
    if (!imu_params_ok(ip) || !delta || !jac || n_samples < 0 || (n_samples > 0 && !samples)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    int rc = vis_grow_block(ctx, ctx->imuj_ws, imu_jac_table_bytes(1), "vis_imu_preintegrate_jac");
    if (rc) return rc;
    vis_imu_sample* d_s; double* d_t; int32_t* d_prev; vis_imu_jac_carry* d_c; vis_imu_delta* d_d; vis_imu_bias_jac* d_j; float* d_r;
    rc = vis_carve(ctx, [&](Carver& cv) {
        d_s = cv.take<vis_imu_sample>((size_t)std::max(n_samples, 1)); d_t = cv.take<double>(1); d_prev = cv.take<int32_t>(1);
        d_c = cv.take<vis_imu_jac_carry>(1); d_d = cv.take<vis_imu_delta>(1); d_j = cv.take<vis_imu_bias_jac>(1); d_r = cv.take<float>(9);
    });
    if (rc) return rc;
    vis_imu_jac_carry c;
    std::memset(&c, 0, sizeof(c));
    c.carry.t_last = t_a; c.carry.valid = VIS_IMU_CARRY_TIME;
    const int32_t prev = VIS_KF_CARRIED;
    HostStage hs(ctx);
    hs.up(d_s, samples, (size_t)n_samples * sizeof(vis_imu_sample));
    hs.up(d_t, &t_b, sizeof(t_b));
    hs.up(d_prev, &prev, sizeof(prev));
    hs.up(d_c, &c, sizeof(c));
    hs.flush_ups();
    rc = imu_jac_launch(ctx, ip, 1, FtFrames{d_prev, 0, nullptr}, d_s, n_samples, d_t, d_c, ctx->imuj_ws.p, d_d, d_j, d_r, nullptr);
    if (rc) return vis_drain(ctx, rc);
    const void* h_d = hs.down(d_d, sizeof(vis_imu_delta));
    const void* h_j = hs.down(d_j, sizeof(vis_imu_bias_jac));
    const void* h_r = hs.down(d_r, 9 * sizeof(float));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(delta, h_d, sizeof(vis_imu_delta));
    std::memcpy(jac, h_j, sizeof(vis_imu_bias_jac));
    if (rot) std::memcpy(rot, h_r, 9 * sizeof(float));
    return VIS_OK;
}

// the plan's block: the 62-slot lifting table for B frames and the two carried records
struct ImuJacPlanWork { void* table; vis_imu_jac_carry* carry[2]; };
static int ensure_imu_jac(vis_ctx* ctx, Plan* pl, ImuJacPlanWork& W) {
    return plan_block(ctx, pl->d_imuj_ws, "vis_batch_imu_jac", [&](Carver& cv) {
        W.table = cv.take<char>(imu_jac_table_bytes(pl->B)); W.carry[0] = cv.take<vis_imu_jac_carry>(1); W.carry[1] = cv.take<vis_imu_jac_carry>(1);
    });
}

extern "C" int vis_batch_imu_jac(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                                 vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac, float* d_rot) {
    if (!imu_params_ok(ip) || !d_tframe || !d_delta || !d_jac || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_delta, 8) || !aligned(d_jac, 8) || !aligned(d_rot, 4) || n < 0 || n_samples < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_imu_jac: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES || n > pl->B) { ctx->err = "vis_batch_imu_jac: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    ImuJacPlanWork W;
    { const int rc = ensure_imu_jac(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->imuj.pick(pl->run_count);
    // on the pose stream behind the matcher of the run (the gate's link table) and behind the context's stream (the caller's samples and times)
    const int rc = batch_epi(ctx, n, "vis_batch_imu_jac", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = imu_jac_launch(ctx, ip, n, plan_frames(pl_), d_samples, n_samples, d_tframe, rec.have ? W.carry[rec.slot] : nullptr, W.table, d_delta, d_jac,
                                       d_rot, W.carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->imuj.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_imu_jac_init(vis_ctx* ctx, const vis_imu_jac_carry* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    ImuJacPlanWork W;
    { const int rc = ensure_imu_jac(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->imuj.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.carry[pl->imuj.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->imuj.seeded(pl->run_count);
    return VIS_OK;
}

// ---- the same three calls with the 9 x 9 covariance of the delta (k_imu_cov_intervals, k_imu_cov_pairs, a table and carried records of their own)
extern "C" void vis_default_imu_noise(vis_imu_noise* np) {
    if (!np) return;
    np->sigma_g = 1.6968e-4; np->sigma_a = 2.0e-3;
}

static bool imu_noise_ok(const vis_imu_noise* np) {
    return np && std::isfinite(np->sigma_g) && std::isfinite(np->sigma_a) && np->sigma_g >= 0.0 && np->sigma_a >= 0.0;
}

extern "C" int vis_imu_preintegrate_cov_rows(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, const vis_imu_sample* d_samples, int n_samples,
                                             const double* d_tframe, const int32_t* d_prev, const vis_imu_cov_carry* d_carry_in, vis_imu_delta* d_delta,
                                             vis_imu_cov* d_cov, float* d_rot, vis_imu_cov_carry* d_carry_out) {
    if (!imu_params_ok(ip) || !imu_noise_ok(np) || !d_tframe || !d_prev || !d_delta || !d_cov || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_carry_in, 8) || !aligned(d_delta, 8) || !aligned(d_cov, 8) || !aligned(d_carry_out, 8) ||
        !aligned(d_prev, 4) || !aligned(d_rot, 4)) return VIS_E_INVALID;
    if (n < 0 || n_samples < 0 || (d_carry_out && d_carry_out == d_carry_in)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES) { ctx->err = "vis_imu_preintegrate_cov_rows: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    const int rc = vis_grow_block(ctx, ctx->imuc_ws, imu_cov_table_bytes(n), "vis_imu_preintegrate_cov_rows");
    if (rc) return rc;
    return imu_cov_launch(ctx, ip, np, n, FtFrames{d_prev, 0, nullptr}, d_samples, n_samples, d_tframe, d_carry_in, ctx->imuc_ws.p, d_delta, d_cov, d_rot, d_carry_out);
}

extern "C" int vis_imu_preintegrate_cov(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, const vis_imu_sample* samples, int n_samples, double t_a,
                                        double t_b, vis_imu_delta* delta, vis_imu_cov* cov, float* rot) {
    if (!imu_params_ok(ip) || !imu_noise_ok(np) || !delta || !cov || n_samples < 0 || (n_samples > 0 && !samples)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    int rc = vis_grow_block(ctx, ctx->imuc_ws, imu_cov_table_bytes(1), "vis_imu_preintegrate_cov");
    if (rc) return rc;
    vis_imu_sample* d_s; double* d_t; int32_t* d_prev; vis_imu_cov_carry* d_c; vis_imu_delta* d_d; vis_imu_cov* d_v; float* d_r;
    rc = vis_carve(ctx, [&](Carver& cv) {
        d_s = cv.take<vis_imu_sample>((size_t)std::max(n_samples, 1)); d_t = cv.take<double>(1); d_prev = cv.take<int32_t>(1);
        d_c = cv.take<vis_imu_cov_carry>(1); d_d = cv.take<vis_imu_delta>(1); d_v = cv.take<vis_imu_cov>(1); d_r = cv.take<float>(9);
    });
    if (rc) return rc;
    vis_imu_cov_carry c;
    std::memset(&c, 0, sizeof(c));
    c.carry.t_last = t_a; c.carry.valid = VIS_IMU_CARRY_TIME;
    const int32_t prev = VIS_KF_CARRIED;
    HostStage hs(ctx);
    hs.up(d_s, samples, (size_t)n_samples * sizeof(vis_imu_sample));
    hs.up(d_t, &t_b, sizeof(t_b));
    hs.up(d_prev, &prev, sizeof(prev));
    hs.up(d_c, &c, sizeof(c));
    hs.flush_ups();
    rc = imu_cov_launch(ctx, ip, np, 1, FtFrames{d_prev, 0, nullptr}, d_s, n_samples, d_t, d_c, ctx->imuc_ws.p, d_d, d_v, d_r, nullptr);
    if (rc) return vis_drain(ctx, rc);
    const void* h_d = hs.down(d_d, sizeof(vis_imu_delta));
    const void* h_v = hs.down(d_v, sizeof(vis_imu_cov));
    const void* h_r = hs.down(d_r, 9 * sizeof(float));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(delta, h_d, sizeof(vis_imu_delta));
    std::memcpy(cov, h_v, sizeof(vis_imu_cov));
    if (rot) std::memcpy(rot, h_r, 9 * sizeof(float));
    return VIS_OK;
}

// the plan's block: the 71-slot lifting table for B frames and the two carried records
struct ImuCovPlanWork { void* table; vis_imu_cov_carry* carry[2]; };
static int ensure_imu_cov(vis_ctx* ctx, Plan* pl, ImuCovPlanWork& W) {
    return plan_block(ctx, pl->d_imuc_ws, "vis_batch_imu_cov", [&](Carver& cv) {
        W.table = cv.take<char>(imu_cov_table_bytes(pl->B)); W.carry[0] = cv.take<vis_imu_cov_carry>(1); W.carry[1] = cv.take<vis_imu_cov_carry>(1);
    });
}

extern "C" int vis_batch_imu_cov(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, const vis_imu_sample* d_samples, int n_samples,
                                 const double* d_tframe, vis_imu_delta* d_delta, vis_imu_cov* d_cov, float* d_rot) {
    if (!imu_params_ok(ip) || !imu_noise_ok(np) || !d_tframe || !d_delta || !d_cov || (n_samples > 0 && !d_samples)) return VIS_E_INVALID;
    if (!aligned(d_samples, 8) || !aligned(d_tframe, 8) || !aligned(d_delta, 8) || !aligned(d_cov, 8) || !aligned(d_rot, 4) || n < 0 || n_samples < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_imu_cov: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES || n > pl->B) { ctx->err = "vis_batch_imu_cov: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    ImuCovPlanWork W;
    { const int rc = ensure_imu_cov(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->imuc.pick(pl->run_count);
    // on the pose stream behind the matcher of the run (the gate's link table) and behind the context's stream (the caller's samples and times)
    const int rc = batch_epi(ctx, n, "vis_batch_imu_cov", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = imu_cov_launch(ctx, ip, np, n, plan_frames(pl_), d_samples, n_samples, d_tframe, rec.have ? W.carry[rec.slot] : nullptr, W.table, d_delta, d_cov,
                                       d_rot, W.carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->imuc.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_imu_cov_init(vis_ctx* ctx, const vis_imu_cov_carry* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    ImuCovPlanWork W;
    { const int rc = ensure_imu_cov(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->imuc.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.carry[pl->imuc.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->imuc.seeded(pl->run_count);
    return VIS_OK;
}

static int imu_correct_args(const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg, const double* d_dba,
                            vis_imu_delta* d_delta_out, float* d_rot_out, int32_t* d_status) {
    if (!imu_params_ok(ip) || !d_delta || !d_jac || !d_dbg || !d_delta_out) return VIS_E_INVALID;
    if (!aligned(d_delta, 8) || !aligned(d_jac, 8) || !aligned(d_dbg, 8) || !aligned(d_dba, 8) || !aligned(d_delta_out, 8) || !aligned(d_rot_out, 4) ||
        !aligned(d_status, 4)) return VIS_E_INVALID;
    if (n < 0 || d_delta_out == d_delta) return VIS_E_INVALID;
    return VIS_OK;
}

extern "C" int vis_imu_correct_rows(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                                    const double* d_dba, vis_imu_delta* d_delta_out, float* d_rot_out, int32_t* d_status) {
    { const int rc = imu_correct_args(ip, n, d_delta, d_jac, d_dbg, d_dba, d_delta_out, d_rot_out, d_status); if (rc) return rc; }
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES) { ctx->err = "vis_imu_correct_rows: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return imu_correct_launch(ctx, ip, n, d_delta, d_jac, d_dbg, d_dba, d_delta_out, d_rot_out, d_status);
}

extern "C" int vis_batch_imu_correct(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                                     const double* d_dba, vis_imu_delta* d_delta_out, float* d_rot_out, int32_t* d_status) {
    { const int rc = imu_correct_args(ip, n, d_delta, d_jac, d_dbg, d_dba, d_delta_out, d_rot_out, d_status); if (rc) return rc; }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_imu_correct: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_IMU_MAX_FRAMES) { ctx->err = "vis_batch_imu_correct: more than VIS_IMU_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    // on the pose stream behind vis_batch_imu_jac and vis_batch_vi_align of the run, which wrote d_delta, d_jac and d_dbg there
    return batch_epi(ctx, n, "vis_batch_imu_correct", [&](Plan*, Plan::MatchOut&, const int32_t*) {
        const int rc2 = imu_correct_launch(ctx, ip, n, d_delta, d_jac, d_dbg, d_dba, d_delta_out, d_rot_out, d_status);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    });
}

// ---- visual-inertial alignment: vi_align.hip
extern "C" void vis_default_vi_align_params(vis_vi_align_params* vp) {
    if (!vp) return;
    for (int k = 0; k < 9; k++) vp->r_ic[k] = (k & 3) == 0 ? 1.0 : 0.0;
    for (int k = 0; k < 3; k++) vp->p_ci[k] = 0.0;
    vp->G = 9.81; vp->g_tol = 0.1;
    vp->min_pairs = 8; vp->min_triples = 8; vp->refine_iters = 4; vp->reject = VIS_IMU_EMPTY | VIS_IMU_GAP;
}

static bool vi_align_params_ok(const vis_vi_align_params* vp) {
    if (!vp) return false;
    for (int k = 0; k < 9; k++) if (!std::isfinite(vp->r_ic[k])) return false;
    for (int k = 0; k < 3; k++) if (!std::isfinite(vp->p_ci[k])) return false;
    if (!std::isfinite(vp->G) || !std::isfinite(vp->g_tol) || !(vp->G > 0.0) || !(vp->g_tol >= 0.0)) return false;
    return vp->min_pairs >= 1 && vp->min_triples >= 1 && vp->refine_iters >= 0 && vp->refine_iters <= 16;
}

extern "C" int vis_vi_align_rows(vis_ctx* ctx, const vis_vi_align_params* vp, int n, const int32_t* d_prev, const vis_traj_pose* d_traj,
                                 const vis_imu_delta* d_delta, const vis_vi_carry* d_carry_in, vis_vi_state* d_state, vis_vi_align* d_result,
                                 vis_vi_carry* d_carry_out) {
    if (!vi_align_params_ok(vp) || !d_prev || !d_traj || !d_delta || !d_result) return VIS_E_INVALID;
    if (!aligned(d_traj, 8) || !aligned(d_delta, 8) || !aligned(d_carry_in, 8) || !aligned(d_state, 8) || !aligned(d_result, 8) || !aligned(d_carry_out, 8) ||
        !aligned(d_prev, 4)) return VIS_E_INVALID;
    if (n < 0 || (d_carry_out && d_carry_out == d_carry_in)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_vi_align_rows: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return via_launch(ctx, vp, n, FtFrames{d_prev, 0, nullptr}, d_traj, d_delta, d_carry_in, d_state, d_result, d_carry_out);
}

// ---- the inertial factor of a pair (k_imu_factor, vi_align.hip)
extern "C" void vis_default_imu_factor_params(vis_imu_factor_params* fp) {
    if (!fp) return;
    fp->var_rot = fp->var_v = fp->var_p = 0.0;
}

// (rows: the caller-rows form, which also takes d_prev)
static int imu_factor_args(const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, bool rows, const int32_t* d_prev, const vis_traj_pose* d_traj,
                           const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state, const vis_vi_align* d_result,
                           const vis_imu_factor* d_factor) {
    if (!vi_align_params_ok(vp)) return VIS_E_INVALID;
    if (!fp || !std::isfinite(fp->var_rot) || !std::isfinite(fp->var_v) || !std::isfinite(fp->var_p) || fp->var_rot < 0.0 || fp->var_v < 0.0 || fp->var_p < 0.0)
        return VIS_E_INVALID;
    if ((rows && !d_prev) || !d_traj || !d_delta || !d_cov || !d_state || !d_result || !d_factor) return VIS_E_INVALID;
    if (!aligned(d_traj, 8) || !aligned(d_delta, 8) || !aligned(d_cov, 8) || !aligned(d_state, 8) || !aligned(d_result, 8) || !aligned(d_factor, 8) ||
        !aligned(d_prev, 4)) return VIS_E_INVALID;
    return n < 0 ? VIS_E_INVALID : VIS_OK;
}

extern "C" int vis_imu_factor_rows(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, const int32_t* d_prev,
                                   const vis_traj_pose* d_traj, const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state,
                                   const vis_vi_align* d_result, vis_imu_factor* d_factor) {
    { const int rc = imu_factor_args(vp, fp, n, true, d_prev, d_traj, d_delta, d_cov, d_state, d_result, d_factor); if (rc) return rc; }
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_imu_factor_rows: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return imu_factor_launch(ctx, vp, fp, n, FtFrames{d_prev, 0, nullptr}, d_traj, d_delta, d_cov, d_state, d_result, d_factor);
}

extern "C" int vis_batch_imu_factor(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, const vis_traj_pose* d_traj,
                                    const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state, const vis_vi_align* d_result,
                                    vis_imu_factor* d_factor) {
    { const int rc = imu_factor_args(vp, fp, n, false, nullptr, d_traj, d_delta, d_cov, d_state, d_result, d_factor); if (rc) return rc; }
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_imu_factor: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_batch_imu_factor: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    // on the pose stream behind vis_batch_trajectory, vis_batch_imu_cov and vis_batch_vi_align of the run, which wrote every input there
    return batch_epi(ctx, n, "vis_batch_imu_factor", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = imu_factor_launch(ctx, vp, fp, n, plan_frames(pl_), d_traj, d_delta, d_cov, d_state, d_result, d_factor);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    });
}

// the plan's block: the two carried records
struct ViaPlanWork { vis_vi_carry* carry[2]; };
static int ensure_via(vis_ctx* ctx, Plan* pl, ViaPlanWork& W) {
    return plan_block(ctx, pl->d_via_ws, "vis_batch_vi_align", [&](Carver& cv) { W.carry[0] = cv.take<vis_vi_carry>(1); W.carry[1] = cv.take<vis_vi_carry>(1); });
}

extern "C" int vis_batch_vi_align(vis_ctx* ctx, const vis_vi_align_params* vp, int n, const vis_traj_pose* d_traj, const vis_imu_delta* d_delta,
                                  vis_vi_state* d_state, vis_vi_align* d_result) {
    if (!vi_align_params_ok(vp) || !d_traj || !d_delta || !d_result) return VIS_E_INVALID;
    if (!aligned(d_traj, 8) || !aligned(d_delta, 8) || !aligned(d_state, 8) || !aligned(d_result, 8) || n < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_vi_align: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_batch_vi_align: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    ViaPlanWork W;
    { const int rc = ensure_via(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->via.pick(pl->run_count);
    // on the pose stream behind vis_batch_trajectory and vis_batch_imu of the run, which wrote d_traj and d_delta there
    const int rc = batch_epi(ctx, n, "vis_batch_vi_align", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = via_launch(ctx, vp, n, plan_frames(pl_), d_traj, d_delta, rec.have ? W.carry[rec.slot] : nullptr, d_state, d_result, W.carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->via.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_vi_align_init(vis_ctx* ctx, const vis_vi_carry* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    ViaPlanWork W;
    { const int rc = ensure_via(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->via.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.carry[pl->via.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->via.seeded(pl->run_count);
    return VIS_OK;
}

// ---- visual-inertial alignment with the accelerometer bias: k_via_align<true>
extern "C" void vis_default_vi_align_ba_params(vis_vi_align_ba_params* bp) {
    if (!bp) return;
    bp->pivot_rel = VIS_VIAB_PIVOT_REL; bp->min_ba_triples = 16;
    for (int k = 0; k < 5; k++) bp->reserved_[k] = 0;
}

static bool vi_align_ba_params_ok(const vis_vi_align_ba_params* bp) {
    return bp && std::isfinite(bp->pivot_rel) && bp->pivot_rel >= 0.0 && bp->pivot_rel < 1.0 && bp->min_ba_triples >= 1;
}

extern "C" int vis_vi_align_ba_rows(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, const int32_t* d_prev,
                                    const vis_traj_pose* d_traj, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac,
                                    const vis_vi_ba_carry* d_carry_in, vis_vi_state* d_state, vis_vi_align_ba* d_result, vis_vi_ba_carry* d_carry_out) {
    if (!vi_align_params_ok(vp) || !vi_align_ba_params_ok(bp) || !d_prev || !d_traj || !d_delta || !d_jac || !d_result) return VIS_E_INVALID;
    if (!aligned(d_traj, 8) || !aligned(d_delta, 8) || !aligned(d_jac, 8) || !aligned(d_carry_in, 8) || !aligned(d_state, 8) || !aligned(d_result, 8) ||
        !aligned(d_carry_out, 8) || !aligned(d_prev, 4)) return VIS_E_INVALID;
    if (n < 0 || (d_carry_out && d_carry_out == d_carry_in)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_vi_align_ba_rows: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return via_ba_launch(ctx, vp, bp, n, FtFrames{d_prev, 0, nullptr}, d_traj, d_delta, d_jac, d_carry_in, d_state, d_result, d_carry_out);
}

// the plan's block: the two carried records
struct ViabPlanWork { vis_vi_ba_carry* carry[2]; };
static int ensure_viab(vis_ctx* ctx, Plan* pl, ViabPlanWork& W) {
    return plan_block(ctx, pl->d_viab_ws, "vis_batch_vi_align_ba",
                      [&](Carver& cv) { W.carry[0] = cv.take<vis_vi_ba_carry>(1); W.carry[1] = cv.take<vis_vi_ba_carry>(1); });
}

extern "C" int vis_batch_vi_align_ba(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, const vis_traj_pose* d_traj,
                                     const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, vis_vi_state* d_state, vis_vi_align_ba* d_result) {
    if (!vi_align_params_ok(vp) || !vi_align_ba_params_ok(bp) || !d_traj || !d_delta || !d_jac || !d_result) return VIS_E_INVALID;
    if (!aligned(d_traj, 8) || !aligned(d_delta, 8) || !aligned(d_jac, 8) || !aligned(d_state, 8) || !aligned(d_result, 8) || n < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_vi_align_ba: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (n > VIS_VIA_MAX_FRAMES) { ctx->err = "vis_batch_vi_align_ba: more than VIS_VIA_MAX_FRAMES frames"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    ViabPlanWork W;
    { const int rc = ensure_viab(ctx, pl, W); if (rc) return rc; }
    const Turn::Pick rec = pl->viab.pick(pl->run_count);
    // on the pose stream behind vis_batch_trajectory and vis_batch_imu_jac (or vis_batch_imu_correct) of the run, which wrote d_traj, d_delta and d_jac there
    const int rc = batch_epi(ctx, n, "vis_batch_vi_align_ba", [&](Plan* pl_, Plan::MatchOut&, const int32_t*) {
        const int rc2 = via_ba_launch(ctx, vp, bp, n, plan_frames(pl_), d_traj, d_delta, d_jac, rec.have ? W.carry[rec.slot] : nullptr, d_state, d_result,
                                      W.carry[rec.slot ^ 1]);
        if (!rc2) ctx->pose_pending = true;
        return rc2;
    }, true);
    if (rc) return rc;
    pl->viab.commit(rec, pl->run_count);
    return VIS_OK;
}

extern "C" int vis_batch_vi_align_ba_init(vis_ctx* ctx, const vis_vi_ba_carry* rec) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    sync_all(ctx);                                                 // (a kernel in flight reads and writes the records)
    Plan* pl = ctx->batch;
    ViabPlanWork W;
    { const int rc = ensure_viab(ctx, pl, W); if (rc) return rc; }
    if (!rec) { pl->viab.forget(); return VIS_OK; }
    HIPCHK(ctx, hipMemcpy(W.carry[pl->viab.seed_slot()], rec, sizeof(*rec), hipMemcpyHostToDevice));
    pl->viab.seeded(pl->run_count);
    return VIS_OK;
}

// ---- the pose stage on device rows: pose_run on a workspace of the context's own
extern "C" int vis_essential_batch(vis_ctx* ctx, int n, const float* d_p1, const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap,
                                   uint8_t* d_mask, vis_pose_result* d_out) {
    if (n < 0 || max_pts < 0 || row_cap < 0 || !d_npts || !d_out || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_npts & 3)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (max_pts > VIS_RANSAC_MAX_M) { ctx->err = "vis_essential_batch: max_pts exceeds the limit of a RANSAC problem"; return VIS_E_CAPACITY; }
    if (d_mask && row_cap < max_pts) { ctx->err = "vis_essential_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    if (n == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    if (max_pts == 0) {                                            // rows without room for a point: the record of zero correspondences, which is all zeros
        HIPCHK(ctx, hipMemsetAsync(d_out, 0, (size_t)n * sizeof(vis_pose_result), ctx->stream));
        return VIS_OK;
    }
    const int iters = ctx->p.ransac_max_iters, mcap = max_pts;
    PoseWork W;
    bool fresh = false;
    int rc = vis_carve_block(ctx, ctx->ess_ws, "vis_essential_batch", [&](Carver& cv) { W.layout(cv, (size_t)n, (size_t)mcap, (size_t)iters); }, 0, &fresh);
    if (rc) return rc;
    // defence in depth, as plan_fill's: nothing reads these buffers before it writes them, but fresh memory must never hold an index.  On the
    // context's stream, in front of the kernels the caller queues next: that stream does not wait for the null stream (hipStreamNonBlocking), so a
    // plain hipMemset could still be clearing the block under them
    if (fresh) HIPCHK(ctx, hipMemsetAsync(ctx->ess_ws.p, 0, ctx->ess_ws.bytes, ctx->stream));
    rc = vis_build_sample_table(ctx, VIS_POSE_TABLE_M);            // (already there since vis_set_params: the single calls' table, the same sample stream)
    if (rc) return rc;
    rc = pose_run(ctx, n, mcap, iters, d_p1, d_p2, d_npts, W.n1, W.n2, W.samples, W.models, W.counts, W.rstate, nullptr, W.mask, d_out, 1, 1,
                  W.worklist, W.hyp);
    if (rc) return rc;
    static_assert(sizeof(PoseOut) == sizeof(vis_pose_result), "the pose stage writes the public record: nothing to convert");
    return d_mask ? mask_rows_run(ctx, n, mcap, row_cap, d_npts, W.mask, d_mask) : VIS_OK;
}

// ---- two-view refinement: refine.hip k_essential_refine
extern "C" void vis_default_eref_params(vis_eref_params* ep) {
    if (!ep) return;
    ep->refine_iters = 5; ep->min_inliers = 8; ep->threshold_px = 1.0;
}

static bool eref_params_ok(const vis_eref_params* ep) {
    return ep && ep->refine_iters >= 0 && ep->refine_iters <= 64 && ep->min_inliers >= 6 && std::isfinite(ep->threshold_px) && ep->threshold_px > 0.0;
}

extern "C" int vis_essential_refine(vis_ctx* ctx, const vis_eref_params* ep, const double R[9], const double t[3], const float* p1xy,
                                    const float* p2xy, int m, const uint8_t* mask, vis_eref_result* out) {
    if (!out || !R || !t || m < 0 || (m && (!p1xy || !p2xy)) || !eref_params_ok(ep)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    const size_t mc = (size_t)std::max(m, 1), mk = (mc + 3) & ~(size_t)3;
    float *d_p1, *d_p2; double* d_rt; int32_t* d_n; uint8_t* d_mask; vis_eref_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>(mc * 2); d_p2 = cv.take<float>(mc * 2);
        d_rt = cv.take<double>(12); d_n = cv.take<int32_t>(1);
        d_mask = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_eref_result>(1);
    });
    if (rc) return rc;
    double rt[12]; std::memcpy(rt, R, 72); std::memcpy(rt + 9, t, 24);
    const int32_t n1 = m;
    std::vector<uint8_t> mpad;
    if (mask && m) { mpad.assign(mk, 0); std::memcpy(mpad.data(), mask, (size_t)m); }
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    hs.up(d_rt, rt, sizeof(rt));
    hs.up(d_n, &n1, 4);
    if (!mpad.empty()) hs.up(d_mask, mpad.data(), mk);
    hs.flush_ups();
    rc = essential_refine_run(ctx, ep, 1, (int)mc, d_rt, 12, 0, 9, d_p1, d_p2, d_n, (int)mk, mask ? d_mask : nullptr, d_out);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out, sizeof(vis_eref_result));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(*out));
    return VIS_OK;
}

static_assert(sizeof(PoseOut) % 8 == 0 && offsetof(PoseOut, R) == 72 && offsetof(PoseOut, t) == 144, "where k_essential_refine finds R and t in a pose record");

extern "C" int vis_essential_refine_batch(vis_ctx* ctx, const vis_eref_params* ep, int n, const vis_pose_result* d_pose, const float* d_p1,
                                          const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask,
                                          vis_eref_result* d_out) {
    if (!eref_params_ok(ep) || n < 0 || max_pts < 0 || row_cap < 0 || !d_pose || !d_npts || !d_out || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_pose & 7) || ((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_npts & 3)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (d_mask && row_cap < max_pts) { ctx->err = "vis_essential_refine_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return essential_refine_run(ctx, ep, n, max_pts, (const double*)d_pose, (int)(sizeof(PoseOut) / 8), 9, 18, d_p1, d_p2, d_npts, row_cap, d_mask, d_out);
}

extern "C" int vis_batch_essential_refine(vis_ctx* ctx, const vis_eref_params* ep, int n, vis_eref_result* d_out) {
    if (!eref_params_ok(ep) || n < 0 || !d_out || ((uintptr_t)d_out & 7)) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    if (!(ctx->batch->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_essential_refine: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    // on the pose stream (batch_epi queues there) behind the pose stage of the last run: its mask and records are single-buffered and written on
    // that stream only, and the next pose stage is queued behind this call
    return batch_epi(ctx, n, "vis_batch_essential_refine", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return essential_refine_run(ctx, ep, n, pl->pose_mcap, (const double*)pl->d_pose, (int)(sizeof(PoseOut) / 8), 9, 18, O.p1, O.p2, d_npts,
                                    pl->pose_mcap, pl->d_mask, d_out);
    });
}

// ---- two-view polish: refine.hip k_essential_polish
extern "C" void vis_default_epolish_params(vis_epolish_params* ep) {
    if (!ep) return;
    std::memset(ep, 0, sizeof(*ep));
    ep->rounds = 3; ep->refine_iters = 5; ep->min_inliers = 8; ep->select_px = 2.0;
}

static bool epolish_params_ok(const vis_epolish_params* ep) {
    return ep && ep->rounds >= 0 && ep->rounds <= 8 && ep->refine_iters >= 1 && ep->refine_iters <= 64 && ep->min_inliers >= 6 &&
           std::isfinite(ep->select_px) && ep->select_px > 0.0 && !ep->reserved_ && !ep->reserved2_[0] && !ep->reserved2_[1];
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

extern "C" int vis_essential_polish(vis_ctx* ctx, const vis_epolish_params* ep, const double R[9], const double t[3], const float* p1xy,
                                    const float* p2xy, int m, const uint8_t* mask, vis_epolish_result* out, uint8_t* mask_out,
                                    vis_pose_result* pose_out) {
    if (!out || !R || !t || m < 0 || (m && (!p1xy || !p2xy || !mask_out)) || !epolish_params_ok(ep)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    const size_t mc = (size_t)std::max(m, 1), mk = (mc + 3) & ~(size_t)3;
    float *d_p1, *d_p2; int32_t* d_n; uint8_t *d_mask, *d_mask_out; PoseOut *d_pose, *d_pose_out; vis_epolish_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>(mc * 2); d_p2 = cv.take<float>(mc * 2);
        d_pose = cv.take<PoseOut>(1); d_n = cv.take<int32_t>(1);
        d_mask = cv.take<uint8_t>(mk); d_mask_out = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_epolish_result>(1); d_pose_out = cv.take<PoseOut>(1);
    });
    if (rc) return rc;
    PoseOut o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(o.R, R, 72); std::memcpy(o.t, t, 24);
    o.n_points = m;
    const int32_t n1 = m;
    std::vector<uint8_t> mpad;
    if (mask && m) { mpad.assign(mk, 0); std::memcpy(mpad.data(), mask, (size_t)m); }
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    hs.up(d_pose, &o, sizeof(o));
    hs.up(d_n, &n1, 4);
    if (!mpad.empty()) hs.up(d_mask, mpad.data(), mk);
    hs.flush_ups();
    rc = essential_polish_run(ctx, ep, 1, (int)mc, d_pose, d_p1, d_p2, d_n, (int)mk, mask ? d_mask : nullptr, (int)mk, d_mask_out, d_out, d_pose_out);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out, sizeof(vis_epolish_result));
    const void* h_mask = hs.down(d_mask_out, mk);
    const void* h_pose = hs.down(d_pose_out, sizeof(PoseOut));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(*out));
    if (m && !(out->flags & VIS_EP_NO_POSE)) std::memcpy(mask_out, h_mask, (size_t)m);    // (NO_POSE: the row is left untouched, the caller's too)
    if (pose_out) std::memcpy(pose_out, h_pose, sizeof(*pose_out));
    return VIS_OK;
}

extern "C" int vis_essential_polish_batch(vis_ctx* ctx, const vis_epolish_params* ep, int n, const vis_pose_result* d_pose, const float* d_p1,
                                          const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask,
                                          uint8_t* d_mask_out, vis_epolish_result* d_out, vis_pose_result* d_pose_out) {
    if (!epolish_params_ok(ep) || n < 0 || max_pts < 0 || row_cap < 0 || !d_pose || !d_npts || !d_out || !d_mask_out || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_pose & 7) || ((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_pose_out & 7) || ((uintptr_t)d_npts & 3)) return VIS_E_INVALID;
    if (ranges_overlap(d_mask, (size_t)n * row_cap, d_mask_out, (size_t)n * row_cap) ||
        ranges_overlap(d_pose, (size_t)n * sizeof(PoseOut), d_pose_out, (size_t)n * sizeof(PoseOut))) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (row_cap < max_pts) { ctx->err = "vis_essential_polish_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return essential_polish_run(ctx, ep, n, max_pts, d_pose, d_p1, d_p2, d_npts, row_cap, d_mask, row_cap, d_mask_out, d_out, d_pose_out);
}

extern "C" int vis_batch_essential_polish(vis_ctx* ctx, const vis_epolish_params* ep, int n, int row_cap, uint8_t* d_mask_out, vis_epolish_result* d_out,
                                          vis_pose_result* d_pose_out) {
    if (!epolish_params_ok(ep) || !d_mask_out || !d_out || ((uintptr_t)d_out & 7) || ((uintptr_t)d_pose_out & 7) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    if (!(ctx->batch->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_essential_polish: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (ctx->batch->last_n < 1 || n != ctx->batch->last_n || !(ctx->batch->last_stages & VIS_STAGE_MATCH)) return VIS_E_STATE;
    if (row_cap < ctx->batch->pose_mcap) { ctx->err = "vis_batch_essential_polish: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    // on the pose stream behind the pose stage of the last run, as vis_batch_essential_refine; the plan's mask and records are read only
    return batch_epi(ctx, n, "vis_batch_essential_polish", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return essential_polish_run(ctx, ep, n, pl->pose_mcap, pl->d_pose, O.p1, O.p2, d_npts, pl->pose_mcap, pl->d_mask, row_cap, d_mask_out, d_out, d_pose_out);
    });
}

// ---- homography polish: homography_polish.hip k_homography_polish
extern "C" void vis_default_hpolish_params(vis_hpolish_params* hp) {
    if (!hp) return;
    std::memset(hp, 0, sizeof(*hp));
    hp->rounds = 3; hp->refine_iters = 5; hp->min_inliers = 8; hp->select_chi2 = 5.991; hp->sigma_px = 1.0;
}

static bool hpolish_params_ok(const vis_hpolish_params* hp) {
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    return hp && hp->rounds >= 0 && hp->rounds <= 8 && hp->refine_iters >= 1 && hp->refine_iters <= 64 && hp->min_inliers >= 5 &&
           pos(hp->select_chi2) && pos(hp->sigma_px) && !hp->reserved_;
}

extern "C" int vis_homography_polish(vis_ctx* ctx, const vis_hpolish_params* hp, const vis_homography_result* h, const float* p1xy,
                                     const float* p2xy, int m, const uint8_t* mask, vis_hpolish_result* out, uint8_t* mask_out,
                                     vis_homography_result* h_out) {
    if (!out || !h || m < 0 || (m && (!p1xy || !p2xy || !mask_out)) || !hpolish_params_ok(hp)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    const size_t mc = (size_t)std::max(m, 1), mk = (mc + 3) & ~(size_t)3;
    float *d_p1, *d_p2; int32_t* d_n; uint8_t *d_mask, *d_mask_out; vis_homography_result *d_h, *d_h_out; vis_hpolish_result* d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_p1 = cv.take<float>(mc * 2); d_p2 = cv.take<float>(mc * 2);
        d_h = cv.take<vis_homography_result>(1); d_n = cv.take<int32_t>(1);
        d_mask = cv.take<uint8_t>(mk); d_mask_out = cv.take<uint8_t>(mk);
        d_out = cv.take<vis_hpolish_result>(1); d_h_out = cv.take<vis_homography_result>(1);
    });
    if (rc) return rc;
    const int32_t n1 = m;
    std::vector<uint8_t> mpad;
    if (mask && m) { mpad.assign(mk, 0); std::memcpy(mpad.data(), mask, (size_t)m); }
    HostStage hs(ctx);
    hs.up(d_p1, p1xy, (size_t)m * 8);
    hs.up(d_p2, p2xy, (size_t)m * 8);
    hs.up(d_h, h, sizeof(*h));
    hs.up(d_n, &n1, 4);
    if (!mpad.empty()) hs.up(d_mask, mpad.data(), mk);
    hs.flush_ups();
    rc = homography_polish_run(ctx, hp, 1, (int)mc, d_h, d_p1, d_p2, d_n, (int)mk, mask ? d_mask : nullptr, (int)mk, d_mask_out, d_out, d_h_out);
    if (rc) return vis_drain(ctx, rc);
    const void* r_out = hs.down(d_out, sizeof(vis_hpolish_result));
    const void* r_mask = hs.down(d_mask_out, mk);
    const void* r_h = hs.down(d_h_out, sizeof(vis_homography_result));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, r_out, sizeof(*out));
    if (m && !(out->flags & VIS_HPOL_NO_MODEL)) std::memcpy(mask_out, r_mask, (size_t)m);    // (NO_MODEL: the row is left untouched, the caller's too)
    if (h_out) std::memcpy(h_out, r_h, sizeof(*h_out));
    return VIS_OK;
}

extern "C" int vis_homography_polish_batch(vis_ctx* ctx, const vis_hpolish_params* hp, int n, const vis_homography_result* d_h, const float* d_p1,
                                           const float* d_p2, const int32_t* d_npts, int max_pts, int row_cap, const uint8_t* d_mask,
                                           uint8_t* d_mask_out, vis_hpolish_result* d_out, vis_homography_result* d_h_out) {
    if (!hpolish_params_ok(hp) || n < 0 || max_pts < 0 || row_cap < 0 || !d_h || !d_npts || !d_out || !d_mask_out || (max_pts && (!d_p1 || !d_p2))) return VIS_E_INVALID;
    if (((uintptr_t)d_h & 7) || ((uintptr_t)d_p1 & 7) || ((uintptr_t)d_p2 & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_h_out & 7) || ((uintptr_t)d_npts & 3)) return VIS_E_INVALID;
    if (ranges_overlap(d_mask, (size_t)n * row_cap, d_mask_out, (size_t)n * row_cap) ||
        ranges_overlap(d_h, (size_t)n * sizeof(vis_homography_result), d_h_out, (size_t)n * sizeof(vis_homography_result))) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    if (row_cap < max_pts) { ctx->err = "vis_homography_polish_batch: row_cap is smaller than max_pts"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    return homography_polish_run(ctx, hp, n, max_pts, d_h, d_p1, d_p2, d_npts, row_cap, d_mask, row_cap, d_mask_out, d_out, d_h_out);
}

extern "C" int vis_batch_homography_polish(vis_ctx* ctx, const vis_hpolish_params* hp, int n, const vis_homography_result* d_h, int mask_cap,
                                           const uint8_t* d_mask, int row_cap, uint8_t* d_mask_out, vis_hpolish_result* d_out,
                                           vis_homography_result* d_h_out) {
    if (!hpolish_params_ok(hp) || !d_h || !d_mask_out || !d_out || ((uintptr_t)d_h & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_h_out & 7) ||
        n < 0 || mask_cap < 0 || row_cap < 0) return VIS_E_INVALID;
    if (ranges_overlap(d_mask, (size_t)n * mask_cap, d_mask_out, (size_t)n * row_cap) ||
        ranges_overlap(d_h, (size_t)n * sizeof(vis_homography_result), d_h_out, (size_t)n * sizeof(vis_homography_result))) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    if (ctx->batch->last_n < 1 || n != ctx->batch->last_n || !(ctx->batch->last_stages & VIS_STAGE_MATCH)) return VIS_E_STATE;
    if (row_cap < ctx->batch->pose_mcap || (d_mask && mask_cap < ctx->batch->pose_mcap)) {
        ctx->err = "vis_batch_homography_polish: row_cap or mask_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY;
    }
    // on the pose stream behind vis_batch_homography of the same run (batch_epi queues there): d_h and d_mask are complete when the kernel reads
    // them, and a vis_batch_homography_pose queued behind this call finds d_h_out and d_mask_out complete
    return batch_epi(ctx, n, "vis_batch_homography_polish", [&](Plan* pl, Plan::MatchOut& O, const int32_t* d_npts) {
        return homography_polish_run(ctx, hp, n, pl->pose_mcap, d_h, O.p1, O.p2, d_npts, mask_cap, d_mask, row_cap, d_mask_out, d_out, d_h_out);
    });
}

extern "C" int vis_batch_triangulate_from(vis_ctx* ctx, const vis_tri_params* tp, int n, const vis_pose_result* d_pose, int mask_cap,
                                          const uint8_t* d_mask, int row_cap, vis_map_point* d_points, uint8_t* d_flags, vis_tri_summary* d_summary) {
    if (!tp || !d_points || !d_flags || !d_summary || ((uintptr_t)d_points & 15) || ((uintptr_t)d_summary & 3)) return VIS_E_INVALID;
    if (!d_pose || ((uintptr_t)d_pose & 7) || mask_cap < 0) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_POSE)) { ctx->err = "vis_batch_triangulate_from: the last vis_batch_run had no VIS_STAGE_POSE"; return VIS_E_STATE; }
    if (row_cap < pl->pose_mcap) { ctx->err = "vis_batch_triangulate_from: row_cap is smaller than the plan's correspondences per pair"; return VIS_E_CAPACITY; }
    if (d_mask && mask_cap != pl->pose_mcap) { ctx->err = "vis_batch_triangulate_from: mask rows must be the plan's correspondences per pair apart"; return VIS_E_CAPACITY; }
    // vis_batch_triangulate's place on the pose stream and its reader event (it reads the same p1 / p2 of the last step's matcher-output set); the
    // caller's records and mask were written on that stream (vis_batch_essential_polish) or are the caller's to order
    Plan::MatchOut& O = pl->out();
    return on_pose_stream(ctx, {0, ctx->ev_tri_done[pl->mo_cur]}, [&] {
        const int rc = triangulate_run(ctx, tp, n, pl->pose_mcap, row_cap, d_pose, O.p1, O.p2, d_mask, d_points, d_flags, d_summary);
        if (!rc) ctx->pose_pending = true;
        return rc;
    }, {&O.readers});
}

extern "C" int vis_batch_fast_thresholds(vis_ctx* ctx, int32_t* tau_next, int32_t* n_redone) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    sync_all(ctx);
    if (!pl->speculate) { if (n_redone) *n_redone = 0; if (tau_next) for (int l = 0; l < pl->L; l++) tau_next[l] = ctx->p.fast_threshold; return VIS_OK; }
    if (tau_next) HIPCHK(ctx, hipMemcpy(tau_next, pl->d_tau, (size_t)pl->L * 4, hipMemcpyDeviceToHost));
    if (n_redone) HIPCHK(ctx, hipMemcpy(n_redone, pl->d_fix, 4, hipMemcpyDeviceToHost));
    return VIS_OK;
}

extern "C" int vis_batch_status(vis_ctx* ctx, int* flags) {
    if (!ctx || !ctx->batch || !flags) return VIS_E_STATE;
    sync_all(ctx);
    int32_t fl = 0;
    HIPCHK(ctx, hipMemcpy(&fl, ctx->batch->d_flags, 4, hipMemcpyDeviceToHost));
    *flags = fl;
    return VIS_OK;
}

extern "C" int vis_batch_get_keypoints(vis_ctx* ctx, int frame, vis_keypoint* kps, uint8_t* desc, int cap, int* n_out) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (frame < 0 || frame >= pl->last_n) return VIS_E_INVALID;
    sync_all(ctx);
    int32_t n = 0;
    const int rbase = pl->last_base;
    HIPCHK(ctx, hipMemcpy(&n, pl->d_nkp + rbase + frame + 1, 4, hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    if ((kps || desc) && n > cap) return VIS_E_CAPACITY;
    if (kps && n) HIPCHK(ctx, hipMemcpy(kps, pl->d_kps + (size_t)(rbase + frame + 1) * pl->kcap, (size_t)n * sizeof(vis_keypoint), hipMemcpyDeviceToHost));
    if (desc && n) HIPCHK(ctx, hipMemcpy(desc, pl->d_desc + (size_t)(rbase + frame + 1) * pl->kcap * 32, (size_t)n * 32, hipMemcpyDeviceToHost));
    return VIS_OK;
}

extern "C" int vis_batch_get_knn(vis_ctx* ctx, int frame, vis_dmatch* out12, int cap12, int* n12,
                                 vis_dmatch* out21, int cap21, int* n21) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (frame < 0 || frame >= pl->last_n) return VIS_E_INVALID;
    sync_all(ctx);
    int32_t nq = 0, nt = 0, q = pl->last_base + frame;
    if (pl->kf_min) HIPCHK(ctx, hipMemcpy(&q, pl->last_set().gq + frame, 4, hipMemcpyDeviceToHost));   // keyframe gate: the query record of the pair, -1 = none
    if (q >= 0) HIPCHK(ctx, hipMemcpy(&nq, pl->d_nkp + q, 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&nt, pl->d_nkp + pl->last_base + frame + 1, 4, hipMemcpyDeviceToHost));
    if (q < 0 || (!pl->kf_min && frame == 0 && !pl->pair0_valid)) { nq = 0; nt = 0; }      // no pair: the first frame of a stream, or a frame the gate did not save
    if (n12) *n12 = nq;
    if (n21) *n21 = nt;
    if (out12) { if (2 * nq > cap12) return VIS_E_CAPACITY; int rc = download_knn(ctx, pl->d_knn12 + (size_t)frame * pl->kcap * 2, nq, out12); if (rc) return rc; }
    if (out21) { if (2 * nt > cap21) return VIS_E_CAPACITY; int rc = download_knn(ctx, pl->d_knn21 + (size_t)frame * pl->kcap * 2, nt, out21); if (rc) return rc; }
    return VIS_OK;
}

extern "C" int vis_batch_get_matches(vis_ctx* ctx, int frame, vis_dmatch* good, int cap, int* n_good, int* n_sym) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (frame < 0 || frame >= pl->last_n) return VIS_E_INVALID;
    sync_all(ctx);
    return download_matches(ctx, pl, frame, good, cap, n_good, nullptr, 0, n_sym);
}

// the inlier mask findEssentialMat left for pair `frame` (one byte per correspondence the pose stage saw: the grid-filtered good
// matches, or the symmetric matches in their list order with VIS_POSE_SYM)
extern "C" int vis_batch_get_inlier_mask(vis_ctx* ctx, int frame, uint8_t* mask, int cap, int* n_points) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (frame < 0 || frame >= pl->last_n) return VIS_E_INVALID;
    sync_all(ctx);
    PoseOut o;
    HIPCHK(ctx, hipMemcpy(&o, pl->d_pose + frame, sizeof(PoseOut), hipMemcpyDeviceToHost));
    const int n = std::min(std::max(o.n_points, 0), pl->pose_mcap);
    if (n_points) *n_points = n;
    if (mask) {
        if (n > cap) return VIS_E_CAPACITY;
        if (n) HIPCHK(ctx, hipMemcpy(mask, pl->d_mask + (size_t)frame * pl->pose_mcap, (size_t)n, hipMemcpyDeviceToHost));
    }
    return VIS_OK;
}

extern "C" int vis_batch_get_keyframes(vis_ctx* ctx, int32_t* prev, int cap, int* n_out) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    const int n = pl->last_n;
    if (n < 1) return VIS_E_STATE;
    if (n_out) *n_out = n;
    if (!prev) return VIS_OK;
    if (cap < n) return VIS_E_CAPACITY;
    sync_all(ctx);
    if (pl->kf_min) { HIPCHK(ctx, hipMemcpy(prev, pl->last_set().kf_link, (size_t)n * 4, hipMemcpyDeviceToHost)); return VIS_OK; }
    for (int i = 0; i < n; i++) prev[i] = i - 1;
    prev[0] = pl->pair0_valid ? VIS_KF_CARRIED : VIS_KF_FIRST;
    return VIS_OK;
}

extern "C" int vis_batch_get_pose(vis_ctx* ctx, int frame, double E[9], double R[9], double t[3],
                                  int* n_inliers, int* n_pose_good, int* iters_run) {
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (frame < 0 || frame >= pl->last_n) return VIS_E_INVALID;
    sync_all(ctx);
    PoseOut o;
    HIPCHK(ctx, hipMemcpy(&o, pl->d_pose + frame, sizeof(PoseOut), hipMemcpyDeviceToHost));
    if (E) std::memcpy(E, o.E, 72);
    if (R) std::memcpy(R, o.R, 72);
    if (t) std::memcpy(t, o.t, 24);
    if (n_inliers) *n_inliers = o.n_inliers;
    if (n_pose_good) *n_pose_good = o.n_pose_good;
    if (iters_run) *iters_run = o.iters_run;
    return VIS_OK;
}
