// ep_sums.h -- the workgroup half of the summation contract "T" (include/vislam_hip.h, vis_essential_polish): what k_essential_polish
// (refine.hip) and k_homography_polish (homography_polish.hip) share.  A thread of NT = 64 NW walks the points i = tid mod NT, a wave_sum
// per sum leaves wave w with W_w, and ep_totals adds the wave totals in rising w on every thread: the same bits everywhere, hence uniform
// control flow around the barriers.  NW = 1 is the one-wave order as it stands (W_1 = W_2 = W_3 = +0.0 and a W is never -0.0).
#pragma once
#include "ransac_lanes.h"

// v[k] <- ((W_0 + W_1) + W_2) + W_3 of the wave totals v[k], n <- the sum of the waves' n, on every thread.  Two barriers: every thread of the
// workgroup calls it, in uniform control flow
template <int NW, int K>
DEV void ep_totals(double (&v)[K], int& n) {
    if constexpr (NW > 1) {
        static_assert(NW == 4, "the contract names four wave totals");
        __shared__ double s_w[NW][K];
        __shared__ int s_n[NW];
        const int tid = threadIdx.x;
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < K; k++) s_w[tid >> 6][k] = v[k];
            s_n[tid >> 6] = n;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; k++) v[k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
        n = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
        __syncthreads();                                           // read by every wave before the next call writes
    }
}
// two integer counts of the workgroup, on every thread
template <int NW>
DEV void ep_counts(int& a, int& b) {
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if constexpr (NW > 1) {
        __shared__ int s_c[NW][2];
        const int tid = threadIdx.x;
        if ((tid & 63) == 0) { s_c[tid >> 6][0] = a; s_c[tid >> 6][1] = b; }
        __syncthreads();
        a = 0; b = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { a += s_c[w][0]; b += s_c[w][1]; }
        __syncthreads();
    }
}
