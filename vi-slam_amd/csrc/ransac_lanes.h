// ransac_lanes.h -- what the lane-parallel RANSAC kernels share: k_homography_batch (homography.hip) and k_pnp_batch (pnp.hip) are
// written on it; k_f2f_batch (epipolar.hip) has the same shape written out (its header comment says why) and takes cross3 only.
//
// The shape: one workgroup per problem.  The hypotheses are spread over the lanes, IPL slots per lane and NT * IPL per round (slot s of
// lane tid in the round that starts at j0 is iteration j0 + s NT + tid), and stay in registers.  The points are walked in LDS tiles of TILE
// records, every lane reading the same record -- a broadcast -- and counting it under each of its slots.  The winner is the maximum over
// the workgroup of the integer key (count << 32 | 0x7fffffff - slot number): the first slot among those with the largest count, whatever
// order the maximum is taken in, so a record does not depend on <NT, IPL>.  The model stays in the kernel: the point record, the
// hypothesis, the inlier test, the early zero-record exit and the winner's epilogue.
//
// rl_first_tile, rl_walk_tiles and rl_block_reduce contain workgroup barriers: EVERY thread of the workgroup must call them, in uniform
// control flow, a thread without a hypothesis included.
#pragma once
#include <type_traits>

#ifndef DEV
#define DEV __device__ __forceinline__
#endif

DEV void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
DEV double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
DEV double wave_sum(double v) {                                    // the fixed tree: every lane ends with the same sum
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

// ---- the winner key.  0 = no slot with a count > 0 (a live slot's key is never 0: its count is).  A lane must offer its slots in rising
// order or compare with > as rl_offer does; either way the larger key is the larger count, then the smaller slot number.
DEV unsigned long long rl_key(int count, int slot) { return ((unsigned long long)(unsigned)count << 32) | (unsigned)(0x7fffffff - slot); }
DEV int rl_key_slot(unsigned long long key) { return 0x7fffffff - (int)(unsigned)(key & 0xffffffffull); }
DEV int rl_key_count(unsigned long long key) { return (int)(key >> 32); }
// true: `best` took the key of this slot (a live slot with a count > 0 that beats what the lane held)
DEV bool rl_offer(unsigned long long& best, bool live, int count, int slot) {
    const unsigned long long key = rl_key(count, slot);
    const bool take = live && count > 0 && key > best;
    if (take) best = key;
    return take;
}

// ---- a round: the slots that hold an iteration on any lane (uniform), and whether this wave holds any (wave-uniform)
template <int NT, int IPL> DEV int rl_round_slots(int j0, int iters) { return min(IPL, (iters - j0 + NT - 1) / NT); }
DEV bool rl_wave_live(int j0, int iters) { return j0 + ((int)threadIdx.x & ~63) < iters; }

// ---- the tile walk.  fill(i) -> the record of point i; count(tile, nt) counts the nt records of the tile under the lane's slots.
// A row of at most one tile is filled once, before the rounds (rl_first_tile: true = single), and the walk then only counts; a longer
// row is filled again in every round, barrier - fill - barrier per tile.  The barriers stand outside `wave_live`: a wave whose lanes hold
// no iteration fills its share and keeps the barriers, and only skips the count.
template <int TILE, int NT, class Pt, class Fill>
DEV bool rl_first_tile(Pt* tile, int m, Fill&& fill) {
    const bool single = m <= TILE;
    if (single) {                                                  // (uniform)
        for (int i = threadIdx.x; i < m; i += NT) tile[i] = fill(i);
        __syncthreads();
    }
    return single;
}
template <int TILE, int NT, class Pt, class Fill, class Count>
DEV void rl_walk_tiles(Pt* tile, int m, bool single, bool wave_live, Fill&& fill, Count&& count) {
    for (int t0 = 0; t0 < m; t0 += TILE) {
        const int nt = min(TILE, m - t0);
        if (!single) {
            __syncthreads();                                       // the tile before has been read by every wave
            for (int i = threadIdx.x; i < nt; i += NT) tile[i] = fill(t0 + i);
            __syncthreads();
        }
        if (wave_live) count(tile, nt);
    }
}

// ---- the slot ladder: f(std::integral_constant<int, NS>) for NS = nslots in 1 ... IPL, so that the counting loop is unrolled over a
// compile-time number of slots.  nslots is uniform.  (A closure type per kernel instantiation: each gets a dispatch chain of its own.)
template <int NS, int IPL, class F>
DEV void rl_for_slots(int nslots, F&& f) {
    if constexpr (NS < IPL) { if (nslots > NS) { rl_for_slots<NS + 1, IPL>(nslots, f); return; } }
    f(std::integral_constant<int, NS>{});
}

// ---- the workgroup reduction: best <- the maximum key, sum[k] <- the integer sums, on EVERY thread (k_pnp_batch finds the winning lane
// by `mine == best`).  A 64-lane xor butterfly, then one word per wave through LDS.  Contains a barrier: every thread must call it, once.
template <int NT, int NSUM>
DEV void rl_block_reduce(unsigned long long& best, int (&sum)[NSUM]) {
    __shared__ unsigned long long s_key[NT / 64];
    __shared__ int s_sum[NSUM][NT / 64];
    const int tid = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
        for (int k = 0; k < NSUM; k++) sum[k] += __shfl_xor(sum[k], off);
    }
    if ((tid & 63) == 0) {
        s_key[tid >> 6] = best;
        for (int k = 0; k < NSUM; k++) s_sum[k][tid >> 6] = sum[k];
    }
    __syncthreads();
    best = s_key[0];
    for (int k = 0; k < NSUM; k++) sum[k] = s_sum[k][0];
    for (int w = 1; w < NT / 64; w++) {
        best = s_key[w] > best ? s_key[w] : best;
        for (int k = 0; k < NSUM; k++) sum[k] += s_sum[k][w];
    }
}
