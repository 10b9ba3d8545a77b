// ftrack.hip -- feature tracks: the match lists of a launch linked into tracks of any length, and the N-view triangulation of those tracks
// (include/vislam_hip.h has the contract, tests/ftrack_ref.py restates it).
// Linking never loops over the frames of a launch.  A keypoint has at most one parent (the first-wins rule, settled by an atomic minimum of
// the list position per side and a pass in which only the winner writes), the parent lies in an EARLIER frame, so the frames of a launch form
// chains of at most n - 1 hops: ceil(log2 n) rounds of pointer doubling -- every keypoint replaces its (ancestor, distance) by its ancestor's,
// from one buffer into the other, so no round reads a half-updated element -- reach the first observation of every track.  All of it is
// integer arithmetic on streams of 4-, 8- and 16-byte elements, one element per lane, rows walked with consecutive lanes on consecutive entries.
// The triangulation is one lane per keypoint that ends a track: double precision, + - * / sqrt only, ten fixed accumulators for A^T A and nine for the
// normal equations (no run-time index into a matrix: jacobi_eig.h has the reason), every sum in view order.
#include "vis_internal.h"
#include "ftri_core.h"   // ft_prev, ft_count and the triangulation of one track: shared with ba.hip
#include <climits>
#include <cmath>

#define FT_BLOCK 256
#define FT_NONE 0xFFFFFFFFu

// the parent of frame i: an index < i, VIS_KF_CARRIED when a row is held, else VIS_KF_FIRST (none)
__device__ __forceinline__ int ft_parent(const FtFrames& fr, int i, bool have_carry) {
    const int p = ft_prev(fr, i);
    if (p >= 0) return p < i ? p : VIS_KF_FIRST;
    return p == VIS_KF_CARRIED && have_carry ? VIS_KF_CARRIED : VIS_KF_FIRST;
}
__device__ __forceinline__ int ft_list_count(const int32_t* nlinks, int i, int link_cap, const uint8_t* mask, int mask_cap, const int32_t* mcnt, int mcnt_stride) {
    int m = min(max(nlinks[i], 0), link_cap);
    if (mask) m = min(m, mask_cap);
    if (mcnt) m = min(m, max(mcnt[(size_t)i * mcnt_stride], 0));
    return m;
}

// one lane per (frame, list entry): a candidate takes the minimum of its list position on its trainIdx and on its queryIdx
__global__ __launch_bounds__(FT_BLOCK) void k_ft_claim(int R, FtFrames fr, const vis_dmatch* __restrict__ links, const int32_t* __restrict__ nlinks,
                                                       int link_cap, const uint8_t* __restrict__ mask, int mask_cap, const int32_t* __restrict__ mcnt,
                                                       int mcnt_stride, const vis_ftrack_obs* __restrict__ carry, uint32_t* win_t, uint32_t* win_q) {
    const int i = blockIdx.y, c = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (c >= ft_list_count(nlinks, i, link_cap, mask, mask_cap, mcnt, mcnt_stride)) return;
    const int p = ft_parent(fr, i, carry != nullptr);
    if (p == VIS_KF_FIRST) return;
    if (mask && !mask[(size_t)i * mask_cap + c]) return;
    const vis_dmatch d = links[(size_t)i * link_cap + c];
    if ((uint32_t)d.trainIdx >= (uint32_t)ft_count(fr, i, R)) return;
    if (p >= 0) { if ((uint32_t)d.queryIdx >= (uint32_t)ft_count(fr, p, R)) return; }
    else if ((uint32_t)d.queryIdx >= (uint32_t)R || carry[d.queryIdx].len <= 0) return;
    atomicMin(&win_t[(size_t)i * R + d.trainIdx], (uint32_t)c);
    atomicMin(&win_q[(size_t)i * R + d.queryIdx], (uint32_t)c);
}

// one lane per (frame, keypoint): the parent (only the correspondence that won both sides links) and the first state of the doubling.
// (ancestor, distance): ancestor >= 0 = element i * R + k of this call, ancestor <= -2 = entry -(ancestor + 2) of the carried row (final);
// a keypoint without a parent is its own ancestor at distance 0
__global__ __launch_bounds__(FT_BLOCK) void k_ft_parent(int R, FtFrames fr, const vis_dmatch* __restrict__ links, int link_cap, bool have_carry,
                                                        const uint32_t* __restrict__ win_t, const uint32_t* __restrict__ win_q,
                                                        int2* __restrict__ s0, int32_t* __restrict__ par) {
    const int i = blockIdx.y, k = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (k >= R) return;
    const size_t e = (size_t)i * R + k;
    int2 s = make_int2((int)e, 0);
    int q = -1;
    if (k < ft_count(fr, i, R)) {
        const uint32_t c = win_t[e];
        if (c != FT_NONE) {
            const int cq = links[(size_t)i * link_cap + c].queryIdx;          // (a candidate: in range of the parent, so of win_q's row)
            if (win_q[(size_t)i * R + cq] == c) {
                q = cq;
                const int p = ft_parent(fr, i, have_carry);
                s = p >= 0 ? make_int2(p * R + q, 1) : make_int2(-(q + 2), 1);
            }
        }
    }
    s0[e] = s;
    par[e] = q;
}

// one round: (a, d) <- (ancestor of a, d + its distance) unless a is final (a carried entry, or its own ancestor)
__global__ __launch_bounds__(FT_BLOCK) void k_ft_round(int total, const int2* __restrict__ src, int2* __restrict__ dst) {
    const int e = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (e >= total) return;
    int2 s = src[e];
    if (s.x >= 0 && s.x != e) {
        const int2 a = src[s.x];
        if (a.x != s.x) s = make_int2(a.x, s.y + a.y);
    }
    dst[e] = s;
}

__device__ __forceinline__ int ft_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int ft_wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// one workgroup per frame: the records of its row from the roots (or the carried row), the summary by wave reductions in integers
__global__ __launch_bounds__(FT_BLOCK) void k_ft_finish(int R, FtFrames fr, const vis_ftrack_obs* __restrict__ carry, const int2* __restrict__ st,
                                                        const int32_t* __restrict__ par, int seq0, int ocap, int wcap,
                                                        vis_ftrack_obs* __restrict__ obs, vis_ftrack_frame* __restrict__ frame) {
    __shared__ int s_red[5][FT_BLOCK / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int nk = ft_count(fr, i, R), p = ft_parent(fr, i, carry != nullptr);
    int cont = 0, mx = 0, parent_n = 0;
    uint32_t sum = 0;
    for (int k = tid; k < wcap; k += FT_BLOCK) {
        int4 o = make_int4(-1, -1, 0, -1);
        if (k < nk) {
            const size_t e = (size_t)i * R + k;
            const int2 s = st[e];
            const int q = par[e];
            if (s.x >= 0) o = make_int4(seq0 + s.x / R, s.x % R, s.y + 1, q);
            else { const vis_ftrack_obs c = carry[-(s.x + 2)]; o = make_int4(c.birth_seq, c.birth_kp, c.len + s.y, q); }
            cont += q >= 0; mx = max(mx, o.z); sum += (uint32_t)o.z;
        }
        *reinterpret_cast<int4*>(&obs[(size_t)i * ocap + k]) = o;
    }
    if (p == VIS_KF_CARRIED) for (int k = tid; k < R; k += FT_BLOCK) parent_n += carry[k].len > 0;
    cont = ft_wave_sum(cont); mx = ft_wave_max(mx); sum = (uint32_t)ft_wave_sum((int)sum); parent_n = ft_wave_sum(parent_n);
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = cont; s_red[1][tid >> 6] = mx; s_red[2][tid >> 6] = (int)sum; s_red[3][tid >> 6] = parent_n; }
    __syncthreads();
    if (tid == 0) {
        cont = mx = parent_n = 0; sum = 0;
        for (int w = 0; w < FT_BLOCK / 64; w++) { cont += s_red[0][w]; mx = max(mx, s_red[1][w]); sum += (uint32_t)s_red[2][w]; parent_n += s_red[3][w]; }
        if (p >= 0) parent_n = ft_count(fr, p, R);
        const int raw = ft_prev(fr, i);
        vis_ftrack_frame f;
        f.seq = seq0 + i; f.n_keypoints = nk; f.n_continued = cont; f.n_started = nk - cont;
        f.n_ended = p == VIS_KF_FIRST ? 0 : parent_n - cont;
        f.max_len = mx; f.sum_len = (int32_t)sum;
        f.flags = p != VIS_KF_FIRST ? 0 : (raw == VIS_KF_CARRIED ? VIS_FT_NO_CARRY : VIS_FT_NO_PAIR);
        frame[i] = f;
    }
}

// one workgroup: the row of the last saved frame of the launch -> the plan's next carried row; a launch that saved nothing carries the row it
// was given forward (or an empty one)
__global__ __launch_bounds__(FT_BLOCK) void k_ft_carry(int n, int R, FtFrames fr, const vis_ftrack_obs* __restrict__ carry, int ocap,
                                                       const vis_ftrack_obs* __restrict__ obs, vis_ftrack_obs* __restrict__ out) {
    __shared__ int s_last[FT_BLOCK / 64];
    const int tid = threadIdx.x;
    int last = -1;
    for (int i = tid; i < n; i += FT_BLOCK) if (ft_prev(fr, i) != VIS_KF_NOT_SAVED) last = i;   // (rising i: the lane's largest)
    last = ft_wave_max(last);
    if ((tid & 63) == 0) s_last[tid >> 6] = last;
    __syncthreads();
    last = -1;
    for (int w = 0; w < FT_BLOCK / 64; w++) last = max(last, s_last[w]);
    const int4* src = last >= 0 ? reinterpret_cast<const int4*>(obs + (size_t)last * ocap) : reinterpret_cast<const int4*>(carry);
    for (int k = tid; k < R; k += FT_BLOCK) reinterpret_cast<int4*>(out)[k] = src ? src[k] : make_int4(-1, -1, 0, -1);
}

int ftrack_link_run(vis_ctx* ctx, const FtWork& W, int n, int R, FtFrames fr, const vis_dmatch* d_links, const int32_t* d_nlinks, int link_cap,
                    const uint8_t* d_mask, int mask_cap, const int32_t* d_mcnt, int mcnt_stride, const vis_ftrack_obs* d_carry, int seq0, int ocap,
                    int wcap, vis_ftrack_obs* d_obs, vis_ftrack_frame* d_frame, vis_ftrack_obs* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (R < 0 || wcap > ocap || (size_t)n * (size_t)R > ((size_t)1 << 28)) return VIS_E_INVALID;
    const int total = n * R;
    const int2* st = W.s0;
    if (total > 0) {
        uint32_t* win_t = W.win; uint32_t* win_q = W.win + total;
        HIPCHK(ctx, hipMemsetAsync(W.win, 0xFF, (size_t)total * 2 * sizeof(uint32_t), ctx->stream));
        if (link_cap > 0) {
            hipLaunchKernelGGL(k_ft_claim, dim3((link_cap + FT_BLOCK - 1) / FT_BLOCK, n), dim3(FT_BLOCK), 0, ctx->stream, R, fr, d_links, d_nlinks, link_cap,
                               d_mask, mask_cap, d_mcnt, mcnt_stride, d_carry, win_t, win_q);
            HIPCHK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_ft_parent, dim3((R + FT_BLOCK - 1) / FT_BLOCK, n), dim3(FT_BLOCK), 0, ctx->stream, R, fr, d_links, link_cap, d_carry != nullptr,
                           win_t, win_q, W.s0, W.par);
        HIPCHK(ctx, hipGetLastError());
        int2* a = W.s0; int2* b = W.s1;
        for (int reach = 1; reach < n; reach *= 2) {                      // after r rounds a state spans 2^r hops; a chain has at most n - 1
            hipLaunchKernelGGL(k_ft_round, dim3((total + FT_BLOCK - 1) / FT_BLOCK), dim3(FT_BLOCK), 0, ctx->stream, total, a, b);
            HIPCHK(ctx, hipGetLastError());
            int2* t = a; a = b; b = t;
        }
        st = a;
    }
    hipLaunchKernelGGL(k_ft_finish, dim3(n), dim3(FT_BLOCK), 0, ctx->stream, R, fr, d_carry, st, W.par, seq0, ocap, wcap, d_obs, d_frame);
    HIPCHK(ctx, hipGetLastError());
    if (d_carry_out) {
        hipLaunchKernelGGL(k_ft_carry, dim3(1), dim3(FT_BLOCK), 0, ctx->stream, n, R, fr, d_carry, ocap, d_obs, d_carry_out);
        HIPCHK(ctx, hipGetLastError());
    }
    return VIS_OK;
}

// ---------------------------------------------------------------------------------------------- N-view triangulation
#define FTRI_MARK 0x80                                             // d_flags byte of a keypoint that a later frame continues (between the passes only)

// the flags of every keypoint and the summaries cleared
__global__ __launch_bounds__(FT_BLOCK) void k_ftri_clear(int R, FtFrames fr, int ocap, uint8_t* __restrict__ flags, vis_ftrack_tri_summary* __restrict__ summary) {
    const int i = blockIdx.y, k = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (k < ft_count(fr, i, R)) flags[(size_t)i * ocap + k] = 0;
    if (k < 8) reinterpret_cast<int32_t*>(summary + i)[k] = 0;
}

__global__ __launch_bounds__(FT_BLOCK) void k_ftri_mark(FtriArgs a, uint8_t* __restrict__ flags) {
    const int i = blockIdx.y, k = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (k >= ft_count(a.fr, i, a.R)) return;
    int pk;
    const int p = ftri_parent(a, 0, i, k, &pk);
    if (p >= 0) flags[(size_t)p * a.ocap + pk] = FTRI_MARK;          // (several writers can only write the same byte)
}

// one lane per keypoint: a keypoint that is not a track's end writes the zero record (the divergence is accepted: DESIGN.md 4.18)
__global__ __launch_bounds__(64) void k_ftri_points(FtriArgs a, vis_ftrack_point* __restrict__ points, uint8_t* __restrict__ flags,
                                                    vis_ftrack_tri_summary* __restrict__ summary) {
    const int i0 = blockIdx.y, k0 = blockIdx.x * 64 + threadIdx.x;
    const bool live = k0 < ft_count(a.fr, i0, a.R);
    const size_t e0 = (size_t)i0 * a.ocap + (live ? k0 : 0);
    const bool end = live && flags[e0] != FTRI_MARK;
    vis_ftrack_point pt;
    pt.X[0] = pt.X[1] = pt.X[2] = 0.0; pt.rms_reproj_px = pt.parallax_cos = 0.f; pt.n_views = 0; pt.flags = 0;
    if (end) ftri_point(a, 0, i0, k0, pt);
    if (live) { points[e0] = pt; flags[e0] = (uint8_t)pt.flags; }
    // the summary: one integer atomic per counter and wave
    const int fl = pt.flags;
    const bool none = !(fl & (VIS_FTP_FEW | VIS_FTP_SINGULAR));
    const unsigned long long b_end = __ballot(end);
    if (!b_end) return;
    const int cnt[8] = {(int)__popcll(b_end), (int)__popcll(__ballot(end && none)), (int)__popcll(__ballot(end && (fl & VIS_FTP_KEPT))), (int)__popcll(__ballot(end && (fl & VIS_FTP_FRONT))),
                        (int)__popcll(__ballot(end && (fl & VIS_FTP_REPROJ_OK))), (int)__popcll(__ballot(end && (fl & VIS_FTP_PARALLAX_OK))),
                        (int)__popcll(__ballot(end && (fl & VIS_FTP_FEW))), (int)__popcll(__ballot(end && (fl & VIS_FTP_SINGULAR)))};
    if (threadIdx.x < 8) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) c = threadIdx.x == j ? cnt[j] : c;
        if (c) atomicAdd(reinterpret_cast<int32_t*>(summary + i0) + threadIdx.x, c);
    }
}

int ftrack_triangulate_run(vis_ctx* ctx, const vis_ftrack_tri_params* tp, int n, int R, FtFrames fr, const vis_ftrack_obs* d_obs, int ocap,
                           const void* d_xy, size_t xy_row, int xy_step, const double* d_poses, vis_ftrack_point* d_points, uint8_t* d_flags,
                           vis_ftrack_tri_summary* d_summary) {
    if (n < 1) return VIS_OK;
    if (R < 0 || R > ocap || (size_t)n * (size_t)ocap > ((size_t)1 << 28)) return VIS_E_INVALID;
    FtriArgs a;
    a.n = n; a.R = R; a.ocap = ocap; a.fr = fr; a.obs = d_obs; a.xy = (const char*)d_xy; a.xy_row = xy_row; a.xy_step = xy_step; a.poses = d_poses;
    a.max_views = tp->max_views; a.min_views = tp->min_views; a.gn_iters = tp->gn_iters;
    a.thr2 = tp->max_reproj_px * tp->max_reproj_px; a.max_cos = tp->max_parallax_cos;
    a.fx = ctx->p.fx; a.fy = ctx->p.fy; a.cx = ctx->p.cx; a.cy = ctx->p.cy;
    const int bx = (std::max(R, 8) + FT_BLOCK - 1) / FT_BLOCK;
    hipLaunchKernelGGL(k_ftri_clear, dim3(bx, n), dim3(FT_BLOCK), 0, ctx->stream, R, fr, ocap, d_flags, d_summary);
    HIPCHK(ctx, hipGetLastError());
    if (R == 0) return VIS_OK;
    hipLaunchKernelGGL(k_ftri_mark, dim3((R + FT_BLOCK - 1) / FT_BLOCK, n), dim3(FT_BLOCK), 0, ctx->stream, a, d_flags);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ftri_points, dim3((R + 63) / 64, n), dim3(64), 0, ctx->stream, a, d_points, d_flags, d_summary);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
