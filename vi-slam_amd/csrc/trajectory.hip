// trajectory.hip -- a scaled trajectory from two-view poses: the scale links (the baseline of a pair in units of its keyframe's own baseline, the
// median depth ratio of the map points both pairs share) and the chain of the scaled poses by pointer doubling
// (include/vislam_hip.h has the contract, tests/scale_link_ref.py and tests/trajectory_ref.py restate it).
// Scale links: one workgroup per frame, two launches.  k_sl_depth settles "the first qualifying entry wins a keypoint" by a 64-bit atomic minimum
// of the list position in the depth row itself and then replaces the position by the depth.  k_sl_ratio forms the ratios -- their bit patterns:
// a positive finite double orders like its pattern, an entry without a ratio is 0 and orders first -- and selects the three order statistics in
// eight passes over 8-bit digits, one LDS histogram per rank, integers only; nothing is sorted and the pass count does not depend on the data.
// The chain: ONE launch of one workgroup.  A frame's state (S, R, U, ancestor, hops, unit edges, epoch) is one element; ceil(log2 n) rounds replace
// it by its composition with its ancestor's, every thread holding its (up to four) elements in registers, barriers between reading and writing;
// the elements live in LDS (structure of arrays: a chain's ancestors are a shifted, conflict-free read) up to 256 frames, in the workspace beyond.
#include "vis_internal.h"
#include <cmath>

#define SL_BLOCK 256
#define SL_NONE 0xFFFFFFFFFFFFFFFFull
#define TJ_BLOCK 256
#define TJ_EPT (VIS_TJ_MAX_FRAMES / TJ_BLOCK)
static_assert(TJ_EPT * TJ_BLOCK == VIS_TJ_MAX_FRAMES && TJ_LDS_N == TJ_BLOCK, "one LDS element per thread, four elements per thread at the most");

__device__ __forceinline__ bool tj_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf
// prev[i] normalised: an index < i, VIS_KF_CARRIED, VIS_KF_NOT_SAVED, else VIS_KF_FIRST
__device__ __forceinline__ int tj_prev(const FtFrames& fr, int i) {
    const int p = fr.prev ? fr.prev[i] : (i > 0 ? i - 1 : (fr.pair0 ? VIS_KF_CARRIED : VIS_KF_FIRST));
    if (p >= 0) return p < i ? p : VIS_KF_FIRST;
    return p == VIS_KF_CARRIED || p == VIS_KF_NOT_SAVED ? p : VIS_KF_FIRST;
}
__device__ __forceinline__ bool tj_pose_usable(const PoseOut* o) {
    bool fin = true, any = false;
#pragma unroll
    for (int k = 0; k < 9; k++) { fin = fin && tj_finite(o->R[k]); any = any || o->R[k] != 0.0; }
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && tj_finite(o->t[k]);
    const double tt = (o->t[0] * o->t[0] + o->t[1] * o->t[1]) + o->t[2] * o->t[2];
    return fin && any && tj_finite(tt) && tt > 0.0;
}
// whether frame i writes a depth row: it has a pair and a usable pose record
__device__ __forceinline__ bool sl_has_row(const FtFrames& fr, const PoseOut* pose, int i) {
    const int p = tj_prev(fr, i);
    return (p >= 0 || p == VIS_KF_CARRIED) && tj_pose_usable(pose + i);
}

struct SlArgs { int n, link_cap, mcap, pts_cap, row_cap, require, min_shared; double max_rel_spread, min_scale, max_scale; };

__global__ __launch_bounds__(SL_BLOCK) void k_sl_depth(SlArgs A, FtFrames fr, const vis_dmatch* __restrict__ links, const int32_t* __restrict__ nlinks,
                                                       const PoseOut* __restrict__ pose, const vis_map_point* __restrict__ points,
                                                       const uint8_t* __restrict__ flags, unsigned long long* __restrict__ depth) {
    const int i = blockIdx.x, tid = threadIdx.x;
    unsigned long long* row = depth + (size_t)i * A.row_cap;
    if (!sl_has_row(fr, pose, i)) {                                    // (uniform)
        for (int k = tid; k < A.row_cap; k += SL_BLOCK) row[k] = 0ull;   // (the pattern of +0.0)
        return;
    }
    for (int k = tid; k < A.row_cap; k += SL_BLOCK) row[k] = SL_NONE;
    __syncthreads();
    const int m = min(max(nlinks[i], 0), A.mcap);
    const vis_dmatch* L = links + (size_t)i * A.link_cap;
    for (int k = tid; k < m; k += SL_BLOCK) {
        const int kp = L[k].trainIdx;
        if ((uint32_t)kp < (uint32_t)A.row_cap && (flags[(size_t)i * A.pts_cap + k] & A.require) == A.require) atomicMin(&row[kp], (unsigned long long)k);
    }
    __syncthreads();
    const double r6 = pose[i].R[6], r7 = pose[i].R[7], r8 = pose[i].R[8], t2 = pose[i].t[2];
    for (int kp = tid; kp < A.row_cap; kp += SL_BLOCK) {
        const unsigned long long w = row[kp];
        double z = 0.0;
        if (w != SL_NONE) {
            const double* X = points[(size_t)i * A.pts_cap + w].X;
            const double z2 = ((r6 * X[0] + r7 * X[1]) + r8 * X[2]) + t2;
            if (tj_finite(z2) && z2 > 0.0) z = z2;
        }
        row[kp] = (unsigned long long)__double_as_longlong(z);
    }
}

__device__ __forceinline__ int sl_wave_incl(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(v, off, 64); if (lane >= off) v += u; }
    return v;
}

__global__ __launch_bounds__(SL_BLOCK) void k_sl_ratio(SlArgs A, FtFrames fr, const vis_dmatch* __restrict__ links, const int32_t* __restrict__ nlinks,
                                                       const PoseOut* __restrict__ pose, const vis_map_point* __restrict__ points,
                                                       const uint8_t* __restrict__ flags, const double* __restrict__ depth,
                                                       const double* __restrict__ carry, unsigned long long* __restrict__ ws,
                                                       vis_scale_link* __restrict__ link) {
    __shared__ unsigned long long s_keys[SL_LDS_CAP];
    __shared__ int s_hist[3][256];
    __shared__ int s_wsum[3][SL_BLOCK / 64];
    __shared__ int s_digit[3], s_rank[3], s_cnt[SL_BLOCK / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int p = tj_prev(fr, i);
    int fl = 0;
    const double* qrow = nullptr;
    if (p == VIS_KF_NOT_SAVED || p == VIS_KF_FIRST) fl = VIS_SL_NO_PAIR;
    else if (p == VIS_KF_CARRIED) { qrow = carry; if (!carry) fl = VIS_SL_NO_DEPTH; }
    else qrow = depth + (size_t)p * A.row_cap;
    if (!fl) {                                                         // (uniform) a row without a depth -- q had no pair, no pose, no point -- is no row
        int any = 0;
        for (int k = tid; k < A.row_cap; k += SL_BLOCK) { const double z = qrow[k]; any |= tj_finite(z) && z > 0.0; }
        if (!__syncthreads_or(any)) fl = VIS_SL_NO_DEPTH;
    }
    vis_scale_link out;
    out.scale = out.q25 = out.q75 = 0.0; out.n_shared = 0; out.q = p; out.flags = fl; out.reserved_ = 0;
    if (fl) { if (tid == 0) link[i] = out; return; }                   // (uniform)
    const int m = min(max(nlinks[i], 0), A.mcap);
    unsigned long long* keys = m <= SL_LDS_CAP ? s_keys : ws + (size_t)i * A.mcap;
    const vis_dmatch* L = links + (size_t)i * A.link_cap;
    int cnt = 0;
    for (int c = tid; c < m; c += SL_BLOCK) {
        unsigned long long key = 0ull;
        const int kp = L[c].queryIdx;
        if ((uint32_t)kp < (uint32_t)A.row_cap && (flags[(size_t)i * A.pts_cap + c] & A.require) == A.require) {
            const double z2 = qrow[kp], z1 = points[(size_t)i * A.pts_cap + c].X[2];
            if (tj_finite(z2) && z2 > 0.0 && tj_finite(z1) && z1 > 0.0) {
                const double rho = z2 / z1;
                if (tj_finite(rho) && rho > 0.0) { key = (unsigned long long)__double_as_longlong(rho); cnt++; }
            }
        }
        keys[c] = key;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    int ns = 0;
    for (int w = 0; w < SL_BLOCK / 64; w++) ns += s_cnt[w];
    if (ns > 0) {                                                      // (uniform)
        // rank j among all m keys: the m - ns zero keys order first
        int rank[3] = {(m - ns) + (ns - 1) / 4, (m - ns) + (ns - 1) / 2, (m - ns) + (3 * (ns - 1)) / 4};
        unsigned long long prefix[3] = {0ull, 0ull, 0ull};
        for (int pass = 0; pass < 8; pass++) {
            const int shift = 56 - 8 * pass;
#pragma unroll
            for (int j = 0; j < 3; j++) s_hist[j][tid] = 0;
            __syncthreads();
            for (int c = tid; c < m; c += SL_BLOCK) {
                const unsigned long long key = keys[c];
                const unsigned long long hi = pass ? key >> (shift + 8) : 0ull;
                const int d = (int)((key >> shift) & 255ull);
#pragma unroll
                for (int j = 0; j < 3; j++) if (hi == prefix[j]) atomicAdd(&s_hist[j][d], 1);
            }
            __syncthreads();
            int v[3], incl[3];
#pragma unroll
            for (int j = 0; j < 3; j++) { v[j] = s_hist[j][tid]; incl[j] = sl_wave_incl(v[j]); if ((tid & 63) == 63) s_wsum[j][tid >> 6] = incl[j]; }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 3; j++) {
                int base = 0;
                for (int w = 0; w < (tid >> 6); w++) base += s_wsum[j][w];
                const int hi_ = base + incl[j], lo_ = hi_ - v[j];
                if (lo_ <= rank[j] && rank[j] < hi_) { s_digit[j] = tid; s_rank[j] = rank[j] - lo_; }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 3; j++) { prefix[j] = (prefix[j] << 8) | (unsigned long long)s_digit[j]; rank[j] = s_rank[j]; }
        }
        out.q25 = __longlong_as_double((long long)prefix[0]);
        out.scale = __longlong_as_double((long long)prefix[1]);
        out.q75 = __longlong_as_double((long long)prefix[2]);
    }
    if (tid != 0) return;
    out.n_shared = ns;
    if (ns < A.min_shared) fl |= VIS_SL_FEW;
    if (out.q75 - out.q25 > A.max_rel_spread * out.scale) fl |= VIS_SL_SPREAD;
    if (!(out.scale >= A.min_scale && out.scale <= A.max_scale)) fl |= VIS_SL_RANGE;
    out.flags = fl;
    link[i] = out;
}

// the largest i of the call that satisfies pred, or -1 (one workgroup)
template <class P> __device__ __forceinline__ int tj_block_last(int n, int* s_red, P pred) {
    int last = -1;
    for (int i = threadIdx.x; i < n; i += blockDim.x) if (pred(i)) last = i;   // (rising i: the lane's largest)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
    __syncthreads();                                                   // (s_red may still be read from its last use)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = last;
    __syncthreads();
    last = -1;
    for (int w = 0; w < (int)blockDim.x / 64; w++) last = max(last, s_red[w]);
    return last;
}

// one workgroup: the depth row of the last saved frame of the launch -> the plan's next carried row; a launch that saved nothing carries the row
// it was given forward (or zeros)
__global__ __launch_bounds__(SL_BLOCK) void k_sl_carry(int n, int row_cap, FtFrames fr, const double* __restrict__ carry, const double* __restrict__ depth,
                                                       double* __restrict__ out) {
    __shared__ int s_red[SL_BLOCK / 64];
    const int last = tj_block_last(n, s_red, [&](int i) { return tj_prev(fr, i) != VIS_KF_NOT_SAVED; });
    const double* src = last >= 0 ? depth + (size_t)last * row_cap : carry;
    for (int k = threadIdx.x; k < row_cap; k += SL_BLOCK) out[k] = src ? src[k] : 0.0;
}

int scale_link_run(vis_ctx* ctx, const vis_scale_link_params* sp, int n, FtFrames fr, const vis_dmatch* d_links, const int32_t* d_nlinks, int link_cap,
                   int mcap, const PoseOut* d_pose, const vis_map_point* d_points, const uint8_t* d_flags, int pts_cap, const double* d_carry,
                   int row_cap, double* d_depth, unsigned long long* d_keys, vis_scale_link* d_link, double* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (row_cap < 0 || mcap < 0 || mcap > link_cap || mcap > pts_cap || (mcap > SL_LDS_CAP && !d_keys)) return VIS_E_INVALID;
    SlArgs A;
    A.n = n; A.link_cap = link_cap; A.mcap = mcap; A.pts_cap = pts_cap; A.row_cap = row_cap; A.require = sp->require; A.min_shared = sp->min_shared;
    A.max_rel_spread = sp->max_rel_spread; A.min_scale = sp->min_scale; A.max_scale = sp->max_scale;
    hipLaunchKernelGGL(k_sl_depth, dim3(n), dim3(SL_BLOCK), 0, ctx->stream, A, fr, d_links, d_nlinks, d_pose, d_points, d_flags, (unsigned long long*)d_depth);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sl_ratio, dim3(n), dim3(SL_BLOCK), 0, ctx->stream, A, fr, d_links, d_nlinks, d_pose, d_points, d_flags, d_depth, d_carry, d_keys, d_link);
    HIPCHK(ctx, hipGetLastError());
    if (d_carry_out) {
        hipLaunchKernelGGL(k_sl_carry, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, n, row_cap, fr, d_carry, d_depth, d_carry_out);
        HIPCHK(ctx, hipGetLastError());
    }
    return VIS_OK;
}

// ---------------------------------------------------------------------------------------------- the chain
struct TjState { double S, R[9], U[3]; int anc, hops, units, epoch; };   // anc: a frame of the call, TJ_CARRY, or the frame itself (final)
#define TJ_CARRY (-1)

__device__ __forceinline__ bool tj_carry_ok(const vis_traj_pose* c) { return c && !(c->flags & (VIS_TJ_NOT_SAVED | VIS_TJ_OVERFLOW)); }
__device__ __forceinline__ bool tj_has_parent(const FtFrames& fr, int i, bool have_carry) {
    const int p = tj_prev(fr, i);
    return p >= 0 ? tj_prev(fr, p) != VIS_KF_NOT_SAVED : (p == VIS_KF_CARRIED && have_carry);
}
// a saved frame with a parent and a usable pose record
__device__ __forceinline__ bool tj_is_edge(const FtFrames& fr, const PoseOut* pose, int i, bool have_carry) {
    return tj_prev(fr, i) != VIS_KF_NOT_SAVED && tj_has_parent(fr, i, have_carry) && tj_pose_usable(pose + i);
}

__device__ __forceinline__ void tj_store(double* D, int* I, int stride, int e, const TjState& s) {
    D[e] = s.S;
#pragma unroll
    for (int k = 0; k < 9; k++) D[(size_t)(1 + k) * stride + e] = s.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) D[(size_t)(10 + k) * stride + e] = s.U[k];
    I[e] = s.anc; I[stride + e] = s.hops; I[2 * stride + e] = s.units; I[3 * stride + e] = s.epoch;
}
__device__ __forceinline__ void tj_load(const double* D, const int* I, int stride, int e, TjState& s) {
    s.S = D[e];
#pragma unroll
    for (int k = 0; k < 9; k++) s.R[k] = D[(size_t)(1 + k) * stride + e];
#pragma unroll
    for (int k = 0; k < 3; k++) s.U[k] = D[(size_t)(10 + k) * stride + e];
    s.anc = I[e]; s.hops = I[stride + e]; s.units = I[2 * stride + e]; s.epoch = I[3 * stride + e];
}
// path (1) followed by path (2): R <- R1 R2, U <- R1 U2 + S2 U1, S <- S1 S2 (the header fixes the parentheses)
__device__ __forceinline__ void tj_mul(const double* R1, const double* R2, double* R) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (R1[3 * r] * R2[c] + R1[3 * r + 1] * R2[3 + c]) + R1[3 * r + 2] * R2[6 + c];
}
__device__ __forceinline__ void tj_compose(TjState& s, const TjState& a) {
    double R[9], U[3];
    tj_mul(s.R, a.R, R);
#pragma unroll
    for (int r = 0; r < 3; r++) U[r] = ((s.R[3 * r] * a.U[0] + s.R[3 * r + 1] * a.U[1]) + s.R[3 * r + 2] * a.U[2]) + a.S * s.U[r];
#pragma unroll
    for (int k = 0; k < 9; k++) s.R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) s.U[k] = U[k];
    s.S = s.S * a.S;
    s.epoch = s.units > 0 ? s.epoch : a.epoch;
    s.hops += a.hops; s.units += a.units;
    s.anc = a.anc;
}

__global__ __launch_bounds__(TJ_BLOCK) void k_tj_chain(int n, FtFrames fr, const PoseOut* __restrict__ pose, const vis_scale_link* __restrict__ link,
                                                       const vis_traj_pose* __restrict__ carry, int seq0, int same_epoch, double* __restrict__ wsD,
                                                       int* __restrict__ wsI, vis_traj_pose* __restrict__ traj, double* __restrict__ poses,
                                                       vis_traj_pose* __restrict__ carry_out) {
    __shared__ double s_D[13 * TJ_LDS_N];
    __shared__ int s_I[4 * TJ_LDS_N];
    __shared__ int s_red[TJ_BLOCK / 64];
    __shared__ int s_key;
    const int tid = threadIdx.x;
    const bool lds = n <= TJ_LDS_N;                                    // (uniform)
    double* D = lds ? s_D : wsD;
    int* I = lds ? s_I : wsI;
    const int stride = lds ? TJ_LDS_N : n;
    const bool have_carry = tj_carry_ok(carry);
    TjState st[TJ_EPT];
    int fl[TJ_EPT], par[TJ_EPT];
    // ---- the elements: a root or a frame that was not saved is its own, final ancestor; an edge points at its parent
#pragma unroll
    for (int e = 0; e < TJ_EPT; e++) {
        const int i = tid + e * TJ_BLOCK;
        if (i >= n) continue;
        TjState s;
        s.S = 1.0;
#pragma unroll
        for (int k = 0; k < 9; k++) s.R[k] = (k & 3) == 0 ? 1.0 : 0.0;
        s.U[0] = s.U[1] = s.U[2] = 0.0;
        s.anc = i; s.hops = 0; s.units = 0; s.epoch = seq0 + i;
        const int p = tj_prev(fr, i);
        int f = 0;
        if (p == VIS_KF_NOT_SAVED) f = VIS_TJ_NOT_SAVED;
        else if (!tj_is_edge(fr, pose, i, have_carry)) {
            f = VIS_TJ_ROOT;
            if (tj_has_parent(fr, i, have_carry)) f |= VIS_TJ_NO_POSE;
            else if (p == VIS_KF_CARRIED) f |= VIS_TJ_NO_CARRY;
        } else {
            double sc = link[i].scale;
            const bool below_root = p >= 0 ? !tj_is_edge(fr, pose, p, have_carry) : (carry->flags & VIS_TJ_ROOT) != 0;
            const bool ok = link[i].flags == VIS_SL_OK && tj_finite(sc) && sc > 0.0 && !below_root;
            if (!ok) { sc = 1.0; f = VIS_TJ_UNIT_EDGE; }
            s.S = sc;
#pragma unroll
            for (int k = 0; k < 9; k++) s.R[k] = pose[i].R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) s.U[k] = sc * pose[i].t[k];
            s.anc = p >= 0 ? p : TJ_CARRY; s.hops = 1; s.units = ok ? 0 : 1;
        }
        st[e] = s; fl[e] = f; par[e] = p;
        tj_store(D, I, stride, i, s);
    }
    __syncthreads();
    // ---- pointer doubling: read the ancestor's state of the round before, barrier, write
    for (int reach = 1; reach < n; reach *= 2) {
        bool moved[TJ_EPT];
#pragma unroll
        for (int e = 0; e < TJ_EPT; e++) {
            const int i = tid + e * TJ_BLOCK;
            moved[e] = false;
            if (i >= n || st[e].anc < 0 || st[e].anc == i) continue;
            TjState a;
            tj_load(D, I, stride, st[e].anc, a);
            if (a.anc == st[e].anc) continue;                          // the ancestor is a root: the state is final
            tj_compose(st[e], a);
            moved[e] = true;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < TJ_EPT; e++) if (moved[e]) tj_store(D, I, stride, tid + e * TJ_BLOCK, st[e]);
        __syncthreads();
    }
    // ---- the records
    vis_traj_pose rec[TJ_EPT];
#pragma unroll
    for (int e = 0; e < TJ_EPT; e++) {
        const int i = tid + e * TJ_BLOCK;
        if (i >= n) continue;
        vis_traj_pose o;
#pragma unroll
        for (int k = 0; k < 16; k++) reinterpret_cast<double*>(&o)[k] = 0.0;
        const TjState& s = st[e];
        if (fl[e] & VIS_TJ_NOT_SAVED) o.flags = VIS_TJ_NOT_SAVED;
        else {
            if (s.anc == TJ_CARRY) {
                tj_mul(s.R, carry->R, o.R);
#pragma unroll
                for (int r = 0; r < 3; r++) o.t[r] = ((s.R[3 * r] * carry->t[0] + s.R[3 * r + 1] * carry->t[1]) + s.R[3 * r + 2] * carry->t[2]) + carry->sigma * s.U[r];
                o.sigma = carry->sigma * s.S;
                o.segment_seq = carry->segment_seq; o.epoch_seq = s.units > 0 ? s.epoch : carry->epoch_seq;
                o.hops = carry->hops + s.hops; o.unit_edges = carry->unit_edges + s.units;
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) o.R[k] = s.R[k];
#pragma unroll
                for (int k = 0; k < 3; k++) o.t[k] = s.U[k];
                o.sigma = s.S;
                o.segment_seq = seq0 + s.anc; o.epoch_seq = s.units > 0 ? s.epoch : seq0 + s.anc;
                o.hops = s.hops; o.unit_edges = s.units;
            }
            o.parent = par[e]; o.flags = fl[e];
            bool fin = tj_finite(o.sigma) && o.sigma > 0.0;
#pragma unroll
            for (int k = 0; k < 12; k++) fin = fin && tj_finite(o.R[k]);   // (R and t are adjacent)
            if (!fin) {
#pragma unroll
                for (int k = 0; k < 16; k++) reinterpret_cast<double*>(&o)[k] = 0.0;
                o.flags = VIS_TJ_OVERFLOW;
            }
        }
        rec[e] = o;
        traj[i] = o;
    }
    // ---- the dense poses of the newest frame's epoch (or segment), and the record the plan carries
    if (poses) {
        const int newest = tj_block_last(n, s_red, [&](int i) {
            bool ok = false;
#pragma unroll
            for (int e = 0; e < TJ_EPT; e++) if (i == tid + e * TJ_BLOCK) ok = !(rec[e].flags & (VIS_TJ_NOT_SAVED | VIS_TJ_OVERFLOW));
            return ok;
        });
#pragma unroll
        for (int e = 0; e < TJ_EPT; e++) if (newest >= 0 && newest == tid + e * TJ_BLOCK) s_key = same_epoch ? rec[e].epoch_seq : rec[e].segment_seq;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < TJ_EPT; e++) {
            const int i = tid + e * TJ_BLOCK;
            if (i >= n) continue;
            const bool in = newest >= 0 && !(rec[e].flags & (VIS_TJ_NOT_SAVED | VIS_TJ_OVERFLOW)) && (same_epoch ? rec[e].epoch_seq : rec[e].segment_seq) == s_key;
#pragma unroll
            for (int k = 0; k < 12; k++) poses[(size_t)i * 12 + k] = in ? rec[e].R[k] : 0.0;
        }
    }
    if (carry_out) {
        const int last = tj_block_last(n, s_red, [&](int i) { return tj_prev(fr, i) != VIS_KF_NOT_SAVED; });
#pragma unroll
        for (int e = 0; e < TJ_EPT; e++) if (last >= 0 && last == tid + e * TJ_BLOCK) *carry_out = rec[e];
        if (last < 0 && tid == 0) {
            vis_traj_pose o;
#pragma unroll
            for (int k = 0; k < 16; k++) reinterpret_cast<double*>(&o)[k] = 0.0;
            o.flags = VIS_TJ_NOT_SAVED;
            *carry_out = carry ? *carry : o;
        }
    }
}

int trajectory_run(vis_ctx* ctx, int n, FtFrames fr, const PoseOut* d_pose, const vis_scale_link* d_link, const vis_traj_pose* d_carry, int seq0,
                   int same_epoch_only, double* d_wsD, int32_t* d_wsI, vis_traj_pose* d_traj, double* d_poses, vis_traj_pose* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (n > VIS_TJ_MAX_FRAMES || (n > TJ_LDS_N && (!d_wsD || !d_wsI))) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_tj_chain, dim3(1), dim3(TJ_BLOCK), 0, ctx->stream, n, fr, d_pose, d_link, d_carry, seq0, same_epoch_only ? 1 : 0, d_wsD, d_wsI, d_traj,
                       d_poses, d_carry_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
