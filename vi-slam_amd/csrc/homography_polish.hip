// homography_polish.hip -- Gauss-Newton polish of the homography over its inliers for every pair of a batch on gfx950, FP64 VALU.
//
// vis_*_homography reports the four-point winner of its RANSAC as it stands.  k_homography_polish takes that H and the winner's inlier mask and
// minimises the sum of squared forward transfer errors u(H x1) - x2 over the set, re-selecting the set under the H each round reached -- the shape
// of k_essential_polish (refine.hip): rounds of Gauss-Newton passes, every sum in the tiled order "T", LDL^T without pivoting, the iterate of
// least cost reported.  The contract -- coordinates, residual, Jacobian, the sums and their order, the gauge, the solve, the update, the
// selection -- is stated in include/vislam_hip.h and restated operation for operation in tests/homography_polish_ref.py; this file must keep
// every product and sum parenthesised as written there (the library is built with -ffp-contract=off).
//
// One workgroup per pair, NW waves: thread tid of NT = 64 NW owns the points i = tid mod NT, wave_sum leaves wave w with W_w and ep_totals
// (ep_sums.h) adds the wave totals in rising w on every thread, so every thread holds the same sums and the control flow around the barriers
// is uniform.  The set lives in the caller's output mask row: byte i is read and written by thread i mod NT alone, so no barrier guards it.
// The point loop accumulates the NINE-parameter normal equations, 40 sums (the block of rows and columns 0 ... 2 serves 3 ... 5 too, and the
// block between them is zero); the gauge -- the entry of H that is held -- strikes its row and column at solve time with selects between
// constant indices, once per pass on uniform values: no register array is indexed by a run-time value, so nothing lives in scratch memory.
// The point loops are not unrolled: two points' worth of products next to the 40 accumulators of 8 bytes do not fit the register file, and the
// compiler's unrolled loop spills (DESIGN.md section 4.17 has the resource report).
#include "vis_internal.h"
#include "ransac_lanes.h"
#include "ep_sums.h"
#include "h_transfer.h"
#include <cmath>
#include <cfloat>

struct HQArgs {
    double cx, cy, fx_inv, t_sel;      // k_pose_prep's normalisation; select_chi2 (sigma_px / fx)^2
    int refine_iters, min_inliers, rounds;
    int in_stride, mask_cap, out_cap;  // points per row; bytes between two rows of the input mask and of the output mask
};

enum { HQ_Q = 0, HQ_P0 = 6, HQ_P1 = 15, HQ_T = 24, HQ_G = 30, HQ_COST = 39, HQ_SUMS = 40 };

DEV bool hq_finite(double v) { return fabs(v) <= DBL_MAX; }        // false for a NaN

struct HQPt { double x, y, x2, y2; };
DEV HQPt hq_point(const float* __restrict__ p1, const float* __restrict__ p2, int i, const HQArgs& A) {
    const float2 a = reinterpret_cast<const float2*>(p1)[i], b = reinterpret_cast<const float2*>(p2)[i];
    HQPt p;
    p.x = ((double)a.x - A.cx) * A.fx_inv; p.y = ((double)a.y - A.cy) * A.fx_inv;
    p.x2 = ((double)b.x - A.cx) * A.fx_inv; p.y2 = ((double)b.y - A.cy) * A.fx_inv;
    return p;
}

// the residual of a point under H and what its Jacobian is made of: q = (a, b, iw); false: iw, u, v, ru or rv is not finite
DEV bool hq_residual(const double (&H)[9], const HQPt& p, double& u, double& v, double& ru, double& rv, double (&q)[3]) {
    const double U = (H[0] * p.x + H[1] * p.y) + H[2], V = (H[3] * p.x + H[4] * p.y) + H[5], w = (H[6] * p.x + H[7] * p.y) + H[8];
    const double iw = 1.0 / w;
    u = U * iw; v = V * iw;
    ru = u - p.x2; rv = v - p.y2;
    q[0] = p.x * iw; q[1] = p.y * iw; q[2] = iw;
    return hq_finite(iw) && hq_finite(u) && hq_finite(v) && hq_finite(ru) && hq_finite(rv);
}

// one pass over the row at H: the 40 sums over the set (bit 0 of the row's bytes), this thread's WAVE total of each.  With q = (a, b, iw),
// j0 = -(q u), j1 = -(q v):  S[HQ_Q ..] = q_a q_b (a <= b), S[HQ_P0 + 3 a + b] = q_a j0_b, S[HQ_P1 + 3 a + b] = q_a j1_b,
// S[HQ_T ..] = j0_a j0_b + j1_a j1_b (a <= b), S[HQ_G ..] = q_a ru | q_a rv | j0_a ru + j1_a rv, S[HQ_COST] = ru ru + rv rv
template <int NT>
DEV void hq_pass(const double (&H)[9], const float* __restrict__ p1, const float* __restrict__ p2, const uint8_t* srow, int m, int tid,
                 const HQArgs& A, double (&S)[HQ_SUMS]) {
#pragma unroll
    for (int k = 0; k < HQ_SUMS; k++) S[k] = 0.0;
#pragma clang loop unroll(disable)
    for (int i = tid; i < m; i += NT) {
        const HQPt p = hq_point(p1, p2, i, A);
        double u, v, ru, rv, q[3];
        const bool fin = hq_residual(H, p, u, v, ru, rv, q);
        const bool in = (srow[i] & 1) != 0 && fin;
        const double j0[3] = {-(q[0] * u), -(q[1] * u), -(q[2] * u)}, j1[3] = {-(q[0] * v), -(q[1] * v), -(q[2] * v)};
        int k = HQ_Q;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++, k++) { const double w = q[a] * q[b]; S[k] = S[k] + (in ? w : 0.0); }
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const double w0 = q[a] * j0[b], w1 = q[a] * j1[b];
                S[HQ_P0 + 3 * a + b] = S[HQ_P0 + 3 * a + b] + (in ? w0 : 0.0);
                S[HQ_P1 + 3 * a + b] = S[HQ_P1 + 3 * a + b] + (in ? w1 : 0.0);
            }
        k = HQ_T;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++, k++) { const double w = j0[a] * j0[b] + j1[a] * j1[b]; S[k] = S[k] + (in ? w : 0.0); }
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double g0 = q[a] * ru, g1 = q[a] * rv, g2 = j0[a] * ru + j1[a] * rv;
            S[HQ_G + a] = S[HQ_G + a] + (in ? g0 : 0.0);
            S[HQ_G + 3 + a] = S[HQ_G + 3 + a] + (in ? g1 : 0.0);
            S[HQ_G + 6 + a] = S[HQ_G + 6 + a] + (in ? g2 : 0.0);
        }
        const double e2 = ru * ru + rv * rv;
        S[HQ_COST] = S[HQ_COST] + (in ? e2 : 0.0);
    }
#pragma unroll
    for (int k = 0; k < HQ_SUMS; k++) S[k] = wave_sum(S[k]);
}

// the last pass: nothing is solved behind it, so only the cost is taken -- the same operations on the same operands as hq_pass
template <int NT>
DEV double hq_cost(const double (&H)[9], const float* __restrict__ p1, const float* __restrict__ p2, const uint8_t* srow, int m, int tid,
                   const HQArgs& A) {
    double acc = 0.0;
#pragma clang loop unroll(disable)
    for (int i = tid; i < m; i += NT) {
        const HQPt p = hq_point(p1, p2, i, A);
        double u, v, ru, rv, q[3];
        const bool fin = hq_residual(H, p, u, v, ru, rv, q);
        const bool in = (srow[i] & 1) != 0 && fin;
        const double e2 = ru * ru + rv * rv;
        acc = acc + (in ? e2 : 0.0);
    }
    return wave_sum(acc);
}

// the gauge: the index of the largest |H_k|, the lowest on a tie
DEV int hq_gauge(const double (&H)[9]) {
    int p = 0; double am = fabs(H[0]);
#pragma unroll
    for (int k = 1; k < 9; k++) { const double a = fabs(H[k]); if (a > am) { p = k; am = a; } }
    return p;
}

// entry (a, b) of the symmetric 9 x 9 matrix of the sums; a and b are constants wherever it is called
DEV double hq_entry(const double (&S)[HQ_SUMS], int a, int b) {
    if (a > b) { const int c = a; a = b; b = c; }
    const int ba = a / 3, bb = b / 3, ia = a % 3, ib = b % 3;
    if (ba == 0 && bb == 1) return 0.0;
    if (ba == bb) return S[(ba == 2 ? HQ_T : HQ_Q) + (ia == 0 ? ib : ia == 1 ? 2 + ib : 5)];
    return S[(ba == 0 ? HQ_P0 : HQ_P1) + 3 * ia + ib];
}

// dH = the step of the nine entries with entry p held: row and column p struck, the eight unknowns left in rising order solved by LDL^T without
// pivoting (er_solve5 of refine.hip written for eight), dH[p] = 0.  false: a pivot that is <= 0 or not finite
DEV bool hq_solve(const double (&S)[HQ_SUMS], int p, double (&dH)[9]) {
    double Am[8][8], g[8], L[8][8], D[8], z[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        g[i] = i >= p ? S[HQ_G + i + 1] : S[HQ_G + i];
#pragma unroll
        for (int j = i; j < 8; j++) {
            const double lo = i >= p ? hq_entry(S, i + 1, j) : hq_entry(S, i, j), hi = i >= p ? hq_entry(S, i + 1, j + 1) : hq_entry(S, i, j + 1);
            Am[i][j] = Am[j][i] = j >= p ? hi : lo;
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        double s = Am[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (L[j][c] * L[j][c]) * D[c];
        D[j] = s;
        ok = ok && s > 0.0 && hq_finite(s);
#pragma unroll
        for (int i = j + 1; i < 8; i++) {
            double v = Am[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) v = v - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = v / s;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double v = -g[i];
#pragma unroll
        for (int c = 0; c < i; c++) v = v - L[i][c] * z[c];
        z[i] = v;
    }
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        double v = z[i] / D[i];
#pragma unroll
        for (int c = i + 1; c < 8; c++) v = v - L[c][i] * d[c];
        d[i] = v;
    }
    dH[0] = p == 0 ? 0.0 : d[0];
#pragma unroll
    for (int k = 1; k < 8; k++) dH[k] = k == p ? 0.0 : k > p ? d[k - 1] : d[k];
    dH[8] = p == 8 ? 0.0 : d[7];
    return ok;
}

// ss = H0 H0 + ... + H8 H8 from k = 0, left to right
DEV double hq_norm2(const double (&H)[9]) {
    double ss = H[0] * H[0];
#pragma unroll
    for (int k = 1; k < 9; k++) ss = ss + H[k] * H[k];
    return ss;
}

// the selection under H, G = adj(H): bit 1 of byte i <- point i passes the two-sided transfer test at t_sel with t_sel (w w) finite in both
// directions (an infinite right-hand side would let inf <= inf pass); bit 0 stays the current set.  nnew: the points that pass, nchg: the bytes
// the selection would flip (this thread's share of both)
template <int NT>
DEV void hq_select(const double (&H)[9], const float* __restrict__ p1, const float* __restrict__ p2, uint8_t* srow, int m, int tid, const HQArgs& A,
                   int& nnew, int& nchg) {
    double G[9];
    h_adj(H, G);
    nnew = 0; nchg = 0;
#pragma clang loop unroll(disable)
    for (int i = tid; i < m; i += NT) {
        const HQPt p = hq_point(p1, p2, i, A);
        double e, ww;
        h_transfer(H, p.x, p.y, p.x2, p.y2, e, ww);
        const double rf = A.t_sel * ww;
        const bool f = hq_finite(rf) && e <= rf;
        h_transfer(G, p.x2, p.y2, p.x, p.y, e, ww);
        const double rb = A.t_sel * ww;
        const int pass = (f && hq_finite(rb) && e <= rb) ? 1 : 0;
        const int cur = srow[i];
        srow[i] = (uint8_t)(cur | (pass << 1));
        nnew += pass; nchg += pass ^ cur;
    }
}

static_assert(sizeof(vis_hpolish_result) == 128 && offsetof(vis_hpolish_result, flags) == 124, "16 words of 8 bytes, flags in the high half of the last");
static_assert(sizeof(vis_homography_result) == 112 && offsetof(vis_homography_result, H) == 0 && offsetof(vis_homography_result, n_inliers) == 88 &&
              offsetof(vis_homography_result, best_iter) == 96, "the record k_homography_polish starts from and writes");

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_homography_polish(HQArgs A, const vis_homography_result* __restrict__ hin, const float* __restrict__ p1,
                                                               const float* __restrict__ p2, const int32_t* __restrict__ npts,
                                                               const uint8_t* __restrict__ mask, uint8_t* mask_out,
                                                               vis_hpolish_result* __restrict__ out, vis_homography_result* __restrict__ h_out) {
    constexpr int NT = 64 * NW;
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* rec = reinterpret_cast<const double*>(hin + row);
    double H[9];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) { H[k] = rec[k]; fin = fin && hq_finite(H[k]); }
    const double ss0 = hq_norm2(H);
    vis_hpolish_result* o = out + row;
    if (hin[row].best_iter < 0 || !fin || !(ss0 > 0.0) || !hq_finite(ss0)) {   // (uniform) no model to start from: the zero record, the input record as it is
        if (tid < 16) reinterpret_cast<unsigned long long*>(o)[tid] = tid == 15 ? (unsigned long long)VIS_HPOL_NO_MODEL << 32 : 0ull;
        if (h_out && tid < 14) reinterpret_cast<unsigned long long*>(h_out + row)[tid] = reinterpret_cast<const unsigned long long*>(rec)[tid];
        return;
    }
    {
        const double n0 = sqrt(ss0);
#pragma unroll
        for (int k = 0; k < 9; k++) H[k] = H[k] / n0;
    }
    const int m = min(max(npts[row], 0), A.in_stride);
    const float* r1 = p1 + (size_t)row * A.in_stride * 2;
    const float* r2 = p2 + (size_t)row * A.in_stride * 2;
    const uint8_t* mrow = mask ? mask + (size_t)row * A.mask_cap : nullptr;
    uint8_t* srow = mask_out + (size_t)row * A.out_cap;
    int nset = 0, nchg = 0;
    for (int i = tid; i < m; i += NT) {                            // set 0
        const int in = (mrow ? mrow[i] != 0 : true) ? 1 : 0;
        srow[i] = (uint8_t)in;
        nset += in;
    }
    ep_counts<NW>(nset, nchg);
    const int nfirst = nset;
    const bool run = nset >= A.min_inliers;
    const int passes = run ? A.refine_iters : 0, rounds = run ? A.rounds : 0;
    double Hb[9], S[HQ_SUMS];
    double cost_first = 0.0, cost0 = 0.0, cost1 = 0.0;
    int best = 0, steps = 0, rounds_run = 0;
    bool shrank = false, moved = false;
#pragma unroll
    for (int k = 0; k < 9; k++) Hb[k] = H[k];
    for (int round = 0; round <= rounds; round++) {                // (uniform: every thread holds the same sums and counts)
        if (round > 0) {
            int nnew;
            hq_select<NT>(Hb, r1, r2, srow, m, tid, A, nnew, nchg);
            ep_counts<NW>(nnew, nchg);
            const bool adopt = nchg != 0 && nnew >= A.min_inliers;
            for (int i = tid; i < m; i += NT) { const int v = srow[i]; srow[i] = (uint8_t)(adopt ? v >> 1 : v & 1); }
            if (nchg == 0) break;
            if (!adopt) { shrank = true; break; }
            nset = nnew;
#pragma unroll
            for (int k = 0; k < 9; k++) H[k] = Hb[k];
        }
        for (int step = 0; step <= passes; step++) {               // Gauss-Newton passes over the current set
            double cost[1];
            int none = 0;
            if (step == passes) { cost[0] = hq_cost<NT>(H, r1, r2, srow, m, tid, A); ep_totals<NW>(cost, none); }
            else { hq_pass<NT>(H, r1, r2, srow, m, tid, A, S); ep_totals<NW>(S, none); cost[0] = S[HQ_COST]; }
            const bool take = step == 0 || (hq_finite(cost[0]) && (!hq_finite(cost1) || cost[0] < cost1));
            if (step == 0) { cost0 = cost[0]; if (round == 0) cost_first = cost[0]; }
            if (take) {
                cost1 = cost[0]; best = step;
#pragma unroll
                for (int k = 0; k < 9; k++) Hb[k] = H[k];
            }
            if (step == passes) break;
            const int p = hq_gauge(H);
            double dH[9];
            if (!hq_solve(S, p, dH)) break;
#pragma unroll
            for (int k = 0; k < 9; k++) H[k] = k == p ? H[k] : H[k] + dH[k];
            const double nn = sqrt(hq_norm2(H));
#pragma unroll
            for (int k = 0; k < 9; k++) H[k] = H[k] / nn;
            steps++;
        }
        rounds_run += run ? 1 : 0;
        moved = moved || best > 0;
    }
    if (tid != 0) return;
    double G[9];
    h_adj(Hb, G);
    const double det = (Hb[0] * G[0] + Hb[1] * G[3]) + Hb[2] * G[6];
    vis_hpolish_result r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.H[k] = det < 0.0 ? -Hb[k] : Hb[k];
    r.cost_first = cost_first; r.cost0 = cost0; r.cost1 = cost1;
    r.n_points = m; r.n_set_first = nfirst; r.n_set_last = nset; r.n_changed = nchg;
    r.rounds_run = rounds_run; r.steps_run = steps; r.best_step = best;
    r.flags = (run ? (moved ? VIS_HPOL_POLISHED : VIS_HPOL_REJECTED) : VIS_HPOL_FEW) | (shrank ? VIS_HPOL_SHRANK : 0);
    *o = r;
    if (h_out) {
        vis_homography_result q = hin[row];
#pragma unroll
        for (int k = 0; k < 9; k++) q.H[k] = r.H[k];
        q.n_inliers = nset;
        h_out[row] = q;
    }
}

// hp has been validated by the entry point.  d_h: n homography records; d_p1 / d_p2: n rows of in_stride (x, y) pixels, d_npts of them valid
// (clamped); d_mask: rows of mask_cap >= in_stride bytes, or null; d_mask_out: rows of out_cap >= in_stride bytes; d_h_out: n records or null.
// On ctx->stream.
int homography_polish_run(vis_ctx* ctx, const vis_hpolish_params* hp, int n, int in_stride, const vis_homography_result* d_h, const float* d_p1,
                          const float* d_p2, const int32_t* d_npts, int mask_cap, const uint8_t* d_mask, int out_cap, uint8_t* d_mask_out,
                          vis_hpolish_result* d_out, vis_homography_result* d_h_out) {
    if (n <= 0) return VIS_OK;
    HQArgs A;
    A.cx = ctx->p.cx; A.cy = ctx->p.cy; A.fx_inv = 1. / ctx->p.fx;
    const double s = hp->sigma_px * A.fx_inv;
    A.t_sel = hp->select_chi2 * (s * s);
    A.refine_iters = hp->refine_iters; A.min_inliers = hp->min_inliers; A.rounds = hp->rounds;
    A.in_stride = in_stride; A.mask_cap = mask_cap; A.out_cap = out_cap;
    if (in_stride <= 64)
        hipLaunchKernelGGL(k_homography_polish<1>, dim3(n), dim3(64), 0, ctx->stream, A, d_h, d_p1, d_p2, d_npts, d_mask, d_mask_out, d_out, d_h_out);
    else
        hipLaunchKernelGGL(k_homography_polish<4>, dim3(n), dim3(256), 0, ctx->stream, A, d_h, d_p1, d_p2, d_npts, d_mask, d_mask_out, d_out, d_h_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
