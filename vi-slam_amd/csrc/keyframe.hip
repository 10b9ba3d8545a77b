// keyframe.hip -- the keyframe gate of the batched stream path (vis_params.keyframe_min_points > 0).
// CameraGPU::addGPUKeyframe (src/CameraGPU.cpp:138-173) saves a frame only when it detected more than one keypoint and matches
// it against frameList.back() (:128-129), the last frame it SAVED; Camera::addKeyframe (src/Camera.cpp:197-235) does the same with
// > 10 for every frame after the first.  The batch decides this for all its frames at once on the device: saved(i) depends only on
// frame i's count and on whether a frame has been saved before it, and "the last saved frame before i" is a prefix scan, so one
// workgroup of ballots replaces the reference's sequential walk and the host never waits for the counts.
#include "vis_internal.h"
#include <climits>

#define KF_MAX_WAVES 16

// block-wide dword copy with 8 loads in flight per thread before their stores (source and destination are records of one buffer:
// the compiler may not move a load above a store it cannot prove disjoint, so a plain loop waits a full memory latency per element)
__device__ __forceinline__ void kf_copy_dwords(uint32_t* dst, const uint32_t* src, uint32_t count) {
    for (uint32_t j0 = threadIdx.x; j0 < count; j0 += 8 * blockDim.x) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t j = j0 + u * blockDim.x; v[u] = j < count ? src[j] : 0u; }
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t j = j0 + u * blockDim.x; if (j < count) dst[j] = v[u]; }
    }
}

// One workgroup.  state = {last saved record (absolute, -1 = none), a frame has been saved since reset}.
// 1. the last saved record of the earlier launches -> record `base` of this set (the carried record the matcher reads for a
//    link VIS_KF_CARRIED), like launch_detect's host-indexed copy of the gate-off path (which this path does not run);
// 2. per frame i of the batch (record base + 1 + i): saved(i) = (i == first) || (i > first && nkp > K), first = the first frame
//    with nkp > 1 when nothing has been saved since reset (else no first: saved(i) = nkp > K; K >= 1, so > K implies > 1);
//    link[i] = the last saved frame before i (mask below the lane + clz inside a wave, the waves' last saved index through LDS,
//    the chunks before through a running value), gq[i] = its record (or -1: no pair) for the matcher;
// 3. the new state.
__global__ __launch_bounds__(64 * KF_MAX_WAVES) void k_keyframe_links(int32_t* nkp, vis_keypoint* kps, uint8_t* desc, int kcap,
                                                                     int base, int n, int K, int32_t* __restrict__ state,
                                                                     int32_t* __restrict__ gq, int32_t* __restrict__ link) {
    __shared__ int s_first[KF_MAX_WAVES], s_last[KF_MAX_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const int src = state[0];
    const bool carried = state[1] != 0;
    // (1) carry: the source is a record of the other set (or its record 0), never this set's.  Only its nkp valid entries: nothing
    // reads a record beyond its count
    if (src >= 0 && src != base) {
        static_assert(sizeof(vis_keypoint) % 4 == 0, "copied in dwords");
        const uint32_t m = (uint32_t)min(max(nkp[src], 0), kcap);
        kf_copy_dwords((uint32_t*)(kps + (size_t)base * kcap), (const uint32_t*)(kps + (size_t)src * kcap), m * (sizeof(vis_keypoint) / 4));
        kf_copy_dwords((uint32_t*)(desc + (size_t)base * kcap * 32), (const uint32_t*)(desc + (size_t)src * kcap * 32), m * 8);
        if (tid == 0) nkp[base] = nkp[src];
    }
    // (2) the gate, blockDim.x frames per chunk
    bool seen = carried;                                  // a frame has been saved: the first-frame rule no longer applies
    int last = carried ? VIS_KF_CARRIED : VIS_KF_FIRST;   // last saved frame before the chunk (batch index), or the carried record / none
    for (int c0 = 0; c0 < n; c0 += blockDim.x) {
        const int i = c0 + tid;
        const int k = i < n ? nkp[base + 1 + i] : 0;
        const unsigned long long pK = __builtin_amdgcn_ballot_w64(k > K);
        unsigned long long saved = pK;
        if (!seen) {                                      // (uniform)
            const unsigned long long p1 = __builtin_amdgcn_ballot_w64(k > 1);
            if (lane == 0) s_first[wv] = p1 ? wv * 64 + __ffsll((long long)p1) - 1 : INT_MAX;
            __syncthreads();
            int first = INT_MAX;
            for (int w = 0; w < nw; w++) first = min(first, s_first[w]);
            const int lo = first == INT_MAX ? 64 : first - wv * 64;          // position of `first` in this wave
            if (lo >= 64) saved = 0;
            else if (lo >= 0) saved = (1ull << lo) | (lo < 63 ? pK & (~0ull << (lo + 1)) : 0ull);
        }
        if (lane == 0) s_last[wv] = saved ? wv * 64 + 63 - __clzll((long long)saved) : -1;
        __syncthreads();
        const unsigned long long below = saved & ((1ull << lane) - 1ull);
        int prev;
        if (below) prev = c0 + wv * 64 + 63 - __clzll((long long)below);
        else {
            int j = -1;
            for (int w = wv - 1; w >= 0 && j < 0; w--) j = s_last[w];
            prev = j >= 0 ? c0 + j : last;
        }
        if (i < n) {
            const int L = ((saved >> lane) & 1ull) ? prev : VIS_KF_NOT_SAVED;
            link[i] = L;
            gq[i] = L >= 0 ? base + 1 + L : (L == VIS_KF_CARRIED ? base : -1);
        }
        int cl = -1;
        for (int w = 0; w < nw; w++) cl = max(cl, s_last[w]);
        if (cl >= 0) { last = c0 + cl; seen = true; }
        __syncthreads();                                  // s_first / s_last are rewritten by the next chunk
    }
    // (3) a launch that saves nothing carries the earlier record forward: it sits in this set's record `base` now
    if (tid == 0) {
        state[0] = last >= 0 ? base + 1 + last : (last == VIS_KF_CARRIED ? base : -1);
        state[1] = seen ? 1 : 0;
    }
}

// on the detect stream, behind k_describe of the batch (the counts) and behind launch_detect's wait for the matcher that last read
// this record set (the carried record is written into it); ahead of ev_detect_done, which the matcher waits for
int launch_keyframe_links(vis_ctx* ctx, Plan* pl, int set, int n) {
    if (!pl->kf_min || !pl->d_kf_state || n < 1 || n > pl->npairs) return VIS_E_INVALID;
    const int base = set * pl->rec_per_set;
    // 16 waves whatever n is: the carried record (up to kcap x 60 bytes) is copied by the whole workgroup; the gate needs a multiple of 64
    hipLaunchKernelGGL(k_keyframe_links, dim3(1), dim3(64 * KF_MAX_WAVES), 0, ctx->stream, pl->d_nkp, pl->d_kps,
                       pl->d_desc, pl->kcap, base, n, pl->kf_min, pl->d_kf_state, pl->rec[set].gq, pl->rec[set].kf_link);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int reset_keyframe_state(vis_ctx* ctx, Plan* pl) {
    if (!pl->d_kf_state) return VIS_OK;
    const int32_t s0[2] = {-1, 0};
    HIPCHK(ctx, hipMemcpy(pl->d_kf_state, s0, sizeof(s0), hipMemcpyHostToDevice));
    return VIS_OK;
}
