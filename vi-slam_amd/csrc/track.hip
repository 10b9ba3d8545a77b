// track.hip -- vis_batch_track's device work after the alignment (align.hip batch_align_stream): the keyframe snapshot and
// VISystem::Track (src/VISystem.cpp:1567-1635) over every frame of a launch, in the order VISystemGPU::AddFrameGPU
// (src/VISystemGPU.cpp:137-175) runs it.  Both kernels run on the pose stream behind the alignment of the same launch.
//
// Snapshot: the pair of the next launch's first saved frame links to this launch's last saved frame (gate off: frame n - 1), whose
// images are gone by then (the caller's frame buffer is reused, the gradient sets alternate -- and a launch that saves nothing carries
// the keyframe forward, so it can be several launches old).  One frame of images is copied into a plan-owned buffer: ~2.4 MB at
// 752 x 480, once per launch, at HBM speed.
//
// Chain: final_poseCam = final_poseCam * SE3(R, t) per frame.  Float products are not associative, so the composition is one
// dependent chain of SE3 products -- no parallel scan -- run by one lane with the SAME se3_mul / se3_from_rt code the host helpers
// (vis_se3_*) and the adapters run (-ffp-contract=off on both sides): the device trajectory equals the host's byte for byte.  The
// parallel part is around it: the lanes of the workgroup turn the records into residuals and decide per frame which residual applies.
#include "vis_internal.h"
#include "se3_core.h"

#define TS_THREADS 256
#define TS_BLOCKS 256
#define TC_THREADS 1024

// nbytes from src to dst by the grid, in the widest unit both addresses and the size allow
__device__ __forceinline__ void ts_copy(void* dst, const void* src, size_t nbytes, size_t t, size_t nt) {
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)nbytes;
    if ((a & 15) == 0) {
        uint4* d = (uint4*)dst; const uint4* s = (const uint4*)src;
        for (size_t e = t; e < nbytes / 16; e += nt) d[e] = s[e];
    } else if ((a & 3) == 0) {
        uint32_t* d = (uint32_t*)dst; const uint32_t* s = (const uint32_t*)src;
        for (size_t e = t; e < nbytes / 4; e += nt) d[e] = s[e];
    } else {
        uint8_t* d = (uint8_t*)dst; const uint8_t* s = (const uint8_t*)src;
        for (size_t e = t; e < nbytes; e += nt) d[e] = s[e];
    }
}

// The launch's last saved frame f: gate off n - 1; gate on the largest i with link[i] != VIS_KF_NOT_SAVED, read from THIS launch's
// link table (the keyframe state the next launch's gate kernel may already have rewritten is not read).  None: the snapshot keeps the
// earlier keyframe.  Then gray level 0 of frame f (strided) -> dense, gray levels 1..4 and gx / gy of all levels as they are laid out
// in the gradient set.  Every block finds f itself (n <= 4096 links, L2 hits): no second launch, no device-wide barrier.
__global__ __launch_bounds__(TS_THREADS) void k_track_snapshot(const uint8_t* __restrict__ frames, int w, int h, int stride,
                                                               const uint8_t* __restrict__ half, const int16_t* __restrict__ gx,
                                                               const int16_t* __restrict__ gy, size_t fe, const int32_t* __restrict__ link,
                                                               int n, uint8_t* __restrict__ sg, int16_t* __restrict__ sgx, int16_t* __restrict__ sgy) {
    __shared__ int s_f;
    int f = n - 1;
    if (link) {
        if (threadIdx.x == 0) s_f = -1;
        __syncthreads();
        for (int j0 = n - 1; j0 >= 0; j0 -= blockDim.x) {
            const int j = j0 - (int)threadIdx.x;
            if (j >= 0 && link[j] != VIS_KF_NOT_SAVED) atomicMax(&s_f, j);
            __syncthreads();
            const bool found = s_f >= 0;
            __syncthreads();                                  // (every lane has read s_f before a later round could write it)
            if (found) break;
        }
        f = s_f;
    }
    if (f < 0) return;                                        // (uniform)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    const size_t l0 = (size_t)w * h;
    const uint8_t* F = frames + (size_t)f * stride * h;
    if (((w | stride) & 3) == 0 && ((uintptr_t)F & 3) == 0) {
        const int w4 = w >> 2;
        for (size_t e = t; e < (size_t)w4 * h; e += nt) {
            const size_t y = e / w4, x = e - y * w4;
            ((uint32_t*)sg)[e] = ((const uint32_t*)(F + y * stride))[x];
        }
    } else {
        for (size_t e = t; e < l0; e += nt) { const size_t y = e / w, x = e - y * w; sg[e] = F[y * stride + x]; }
    }
    ts_copy(sg + l0, half + (size_t)f * fe + l0, fe - l0, t, nt);
    ts_copy(sgx, gx + (size_t)f * fe, fe * 2, t, nt);
    ts_copy(sgy, gy + (size_t)f * fe, fe * 2, t, nt);
}

enum { TK_NONE = 0, TK_OWN = 1, TK_LAST = 2 };       // what Track composes for a frame: nothing, its own residual, the last one again
enum { TC_NOT_SAVED = 0, TC_FIRST = 1, TC_PAIR = 2 }; // a frame: refused by the gate, saved without a pair, saved with a pair

// One workgroup, chunks of TC_THREADS frames.  Per chunk: (1) every lane classifies its frame from the pairing (link table, or gate
// off: i - 1 and pair 0 to the carried frame when there is one) and converts the alignment record of a saved frame with a pair into
// SE3(matrix(pose).R, pose.t) in LDS; (2) the last saved frame before each frame (wave ballots + the waves' last indices through
// LDS + the chunks before through running values) gives a refused frame its `composed` (that frame, when it has a pair; the last
// residual of an earlier launch, when there is one; else none); (3) lane 0 composes the chunk in frame order.  state = {pose, last
// residual, have_last}, carried from launch to launch.
__global__ __launch_bounds__(TC_THREADS) void k_track_chain(const vis_align_result* __restrict__ al, const int32_t* __restrict__ link, int pair0,
                                                            int n, TrackState* __restrict__ st, vis_track_result* __restrict__ out) {
    __shared__ vis_se3f s_res[TC_THREADS];
    __shared__ int8_t s_cls[TC_THREADS], s_kind[TC_THREADS];
    __shared__ int s_wlast[TC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const bool have0 = st->have_last != 0;
    Se3 pose = to_se3(st->pose), last = to_se3(st->last);     // (lane 0's)
    int have_last = have0 ? 1 : 0;
    int prev_chunk = -1;                                      // batch index of the last saved frame before the chunk (-1: none in this launch)
    bool prev_chunk_pair = false;
    for (int c0 = 0; c0 < n; c0 += blockDim.x) {
        const int i = c0 + tid;
        int L = VIS_KF_NOT_SAVED;
        if (i < n) L = link ? link[i] : (i > 0 ? i - 1 : (pair0 ? VIS_KF_CARRIED : VIS_KF_FIRST));
        const bool saved = L != VIS_KF_NOT_SAVED, paired = saved && L != VIS_KF_FIRST;
        s_cls[tid] = paired ? TC_PAIR : (saved ? TC_FIRST : TC_NOT_SAVED);
        if (paired) {                                         // SE3(RotationResCam, translationResEst), VISystemGPU::AddFrameGPU + Track
            const float* M = al[i].matrix;
            const float R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]}, tr[3] = {M[3], M[7], M[11]};
            se3_from_rt_f(R, tr, &s_res[tid]);
        }
        const unsigned long long sv = __builtin_amdgcn_ballot_w64(saved);
        if (lane == 0) s_wlast[wv] = sv ? wv * 64 + 63 - __clzll((long long)sv) : -1;
        __syncthreads();
        int kind = TK_NONE, composed = VIS_TRACK_NONE;
        if (paired) { kind = TK_OWN; composed = i; }
        else if (i < n && !saved) {
            const unsigned long long below = sv & ((1ull << lane) - 1ull);
            int p = below ? wv * 64 + 63 - __clzll((long long)below) : -1;
            for (int w_ = wv - 1; w_ >= 0 && p < 0; w_--) p = s_wlast[w_];
            bool has; int who;
            if (p >= 0) { has = s_cls[p] == TC_PAIR; who = c0 + p; }
            else if (prev_chunk >= 0) { has = prev_chunk_pair; who = prev_chunk; }
            else { has = have0; who = VIS_KF_CARRIED; }
            if (has) { kind = TK_LAST; composed = who; }
        }
        s_kind[tid] = (int8_t)kind;
        if (i < n) out[i].composed = composed;
        __syncthreads();
        if (tid == 0) {
            const int m = min(n - c0, (int)blockDim.x);
            for (int j = 0; j < m; j++) {
                const int k = s_kind[j];
                if (k == TK_OWN) { last = to_se3(s_res[j]); have_last = 1; }
                if (k != TK_NONE) pose = se3_mul(pose, last);
                from_se3(pose, &out[c0 + j].pose);
            }
        }
        int cl = -1;
        for (int w_ = 0; w_ < nw; w_++) cl = max(cl, s_wlast[w_]);
        if (cl >= 0) { prev_chunk = c0 + cl; prev_chunk_pair = s_cls[cl] == TC_PAIR; }
        __syncthreads();                                      // s_res / s_cls / s_kind / s_wlast are rewritten by the next chunk
    }
    if (tid == 0) { from_se3(pose, &st->pose); from_se3(last, &st->last); st->have_last = have_last; }
}

int launch_track_snapshot(vis_ctx* ctx, Plan* pl, const uint8_t* d_frames, const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                          const int32_t* links, int n) {
    if (!pl->snap.gray || n < 1) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_track_snapshot, dim3(TS_BLOCKS), dim3(TS_THREADS), 0, ctx->stream, d_frames, pl->w, pl->h, pl->stride, d_gray, d_gx, d_gy,
                       vis_grad_frame_elems(pl->w, pl->h), links, n, pl->snap.gray, pl->snap.gx, pl->snap.gy);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int launch_track_chain(vis_ctx* ctx, Plan* pl, const int32_t* links, int n, const vis_align_result* d_align, vis_track_result* d_track) {
    if (!pl->d_track_state || n < 1) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_track_chain, dim3(1), dim3(TC_THREADS), 0, ctx->stream, d_align, links, pl->pair0_valid ? 1 : 0, n, pl->d_track_state, d_track);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int reset_track_state(vis_ctx* ctx, Plan* pl, bool keep_last) {
    if (!pl->d_track_state) return VIS_OK;
    TrackState s{};
    s.pose = pl->track_init;
    s.last = vis_se3f{0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    s.have_last = 0;
    HIPCHK(ctx, hipMemcpy(pl->d_track_state, &s, keep_last ? sizeof(vis_se3f) : sizeof(s), hipMemcpyHostToDevice));
    return VIS_OK;
}

int ensure_track_buffers(vis_ctx* ctx, Plan* pl) {
    if (pl->d_track_state) return VIS_OK;
    const size_t fe = vis_grad_frame_elems(pl->w, pl->h);
    const size_t gbytes = (fe + 255) & ~(size_t)255, dbytes = (fe * 2 + 255) & ~(size_t)255;
    if (!pl->snap.gray) {                                     // (one allocation; plan_destroy frees snap.gray)
        uint8_t* base = nullptr;
        HIPCHK(ctx, hipMalloc((void**)&base, gbytes + 2 * dbytes));
        pl->snap.gray = base; pl->snap.gx = (int16_t*)(base + gbytes); pl->snap.gy = (int16_t*)(base + gbytes + dbytes);
    }
    TrackState* st = nullptr;
    if (hipMalloc((void**)&st, sizeof(TrackState)) != hipSuccess) { ctx->err = "hipMalloc"; return VIS_E_HIP; }
    pl->d_track_state = st;
    return reset_track_state(ctx, pl, false);
}
