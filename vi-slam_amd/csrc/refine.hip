// refine.hip -- Gauss-Newton refinement of the two-view pose for every pair of a batch on gfx950, FP64 VALU.
//
// The pose stage reports the five-point winner of its RANSAC as it stands (findEssentialMat does no more).  k_essential_refine takes that (R, t)
// and the winner's inlier mask and minimises the sum of squared Sampson distances over the mask in the five parameters of E = [t]x R: a rotation
// step and a step in the tangent plane of the unit translation.  The contract -- coordinates, residual, the complete Jacobian, the summation order,
// the LDL^T solve, the Cayley and tangent updates, the choice of the iterate of least cost -- is stated in include/vislam_hip.h and restated
// operation for operation in tests/essential_refine_ref.py; this file must keep every product and sum parenthesised as written there (the library
// is built with -ffp-contract=off).
//
// One wave per pair, as k_pnp_refine (pnp.hip): every sum over 64 partial sums (i mod 64, rising i) and the fixed butterfly of wave_sum; the
// 5 x 5 solve on every lane alike (they hold the same sums), which is the one-lane solve without a broadcast; lane 0 writes.  Every index into a
// matrix or a sum is a compile-time constant (pose.hip's comment on jacobi_eig has the reason).  The LDL^T solve and the Cayley map are p_solve6
// and p_update of pnp.hip cut down to five unknowns and to the rotation: a second copy, so that pnp.o stays what it was.
//
// k_essential_polish (below k_essential_refine) runs the same passes in rounds, re-selecting the set under the pose each round reached, with one or
// four waves per pair; it shares every er_* function, er_pass / er_cost through their thread count.
#include "vis_internal.h"
#include "ransac_lanes.h"
#include "ep_sums.h"
#include <cmath>
#include <cfloat>

struct ERArgs {
    double cx, cy, fx_inv, thr2;       // k_pose_prep's normalisation; (threshold_px / fx)^2
    int refine_iters, min_inliers, in_stride, row_cap;
    int rec_stride, r_off, t_off;      // the start of pair i: doubles rec_stride * i + r_off (R, 9) and + t_off (t, 3)
};

DEV bool er_finite(double v) { return fabs(v) <= DBL_MAX; }        // false for a NaN

// column j of out = v x column j of M
DEV void er_xmat(const double (&v)[3], const double (&M)[9], double (&out)[9]) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
        out[j] = v[1] * M[6 + j] - v[2] * M[3 + j];
        out[3 + j] = v[2] * M[j] - v[0] * M[6 + j];
        out[6 + j] = v[0] * M[3 + j] - v[1] * M[j];
    }
}

// what a point needs of a matrix M: the first two rows of M x1, the first two of M^T x2, and x2^T M x1
DEV void er_apply(const double (&M)[9], double a, double b, double c, double d, double& l0, double& l1, double& m0, double& m1, double& s) {
    l0 = (M[0] * a + M[1] * b) + M[2];
    l1 = (M[3] * a + M[4] * b) + M[5];
    const double l2 = (M[6] * a + M[7] * b) + M[8];
    m0 = (M[0] * c + M[3] * d) + M[6];
    m1 = (M[1] * c + M[4] * d) + M[7];
    s = (c * l0 + d * l1) + l2;
}

// the tangent basis of a unit t: e = the axis of t's smallest |component| (the lowest index on a tie), b1 = (t x e) / |t x e|, b2 = t x b1.  ONE copy:
// the Jacobian and the update must see the same bits
DEV void er_tangent_basis(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    int k = 0; double am = a0;
    if (a1 < am) { k = 1; am = a1; }
    if (a2 < am) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3];
    cross3(t, e, c);
    const double nb = sqrt(dot3(c, c));
    b1[0] = c[0] / nb; b1[1] = c[1] / nb; b1[2] = c[2] / nb;
    cross3(t, b1, b2);
}

// E and the five derivative matrices of the pose (R, t): G_a = [t]x [e_a]x R for the rotation, [b_a]x R for the tangent plane
DEV void er_matrices(const double (&R)[9], const double (&t)[3], double (&E)[9], double (&G)[5][9]) {
    er_xmat(t, R, E);
    const double A0[9] = {0.0, 0.0, 0.0, -R[6], -R[7], -R[8], R[3], R[4], R[5]};       // [e_0]x R
    const double A1[9] = {R[6], R[7], R[8], 0.0, 0.0, 0.0, -R[0], -R[1], -R[2]};
    const double A2[9] = {-R[3], -R[4], -R[5], R[0], R[1], R[2], 0.0, 0.0, 0.0};
    er_xmat(t, A0, G[0]); er_xmat(t, A1, G[1]); er_xmat(t, A2, G[2]);
    double b1[3], b2[3];
    er_tangent_basis(t, b1, b2);
    er_xmat(b1, R, G[3]); er_xmat(b2, R, G[4]);
}

// t <- (t + b1 d0 + b2 d1) / |...| with the tangent basis of the t before the move
DEV void er_move_t(double (&t)[3], double d0, double d1) {
    double b1[3], b2[3];
    er_tangent_basis(t, b1, b2);
    const double v[3] = {(t[0] + b1[0] * d0) + b2[0] * d1, (t[1] + b1[1] * d0) + b2[1] * d1, (t[2] + b1[2] * d0) + b2[2] * d1};
    const double n = sqrt(dot3(v, v));
    t[0] = v[0] / n; t[1] = v[1] / n; t[2] = v[2] / n;
}

// one pass over the row at pose (R, t): S[0..14] = the upper triangle of sum J^T J in row order, S[15..19] = sum J^T r, S[20] = sum r^2 over the
// set; returns the number of points of the whole row that pass the inlier test under the pose.  NT threads walk the row (thread `lane` of them
// the points i = lane mod NT): what comes back is the total of the caller's own WAVE, all there is for NT = 64
template <int NT = 64>
DEV int er_pass(const double (&R)[9], const double (&t)[3], const float* __restrict__ p1, const float* __restrict__ p2,
                const uint8_t* __restrict__ mrow, int m, int lane, const ERArgs& A, double (&S)[21]) {
    double E[9], G[5][9];
    er_matrices(R, t, E, G);
#pragma unroll
    for (int k = 0; k < 21; k++) S[k] = 0.0;
    int n = 0;
    for (int i = lane; i < m; i += NT) {
        const float2 q1 = reinterpret_cast<const float2*>(p1)[i], q2 = reinterpret_cast<const float2*>(p2)[i];
        const double a = ((double)q1.x - A.cx) * A.fx_inv, b = ((double)q1.y - A.cy) * A.fx_inv;
        const double c = ((double)q2.x - A.cx) * A.fx_inv, d = ((double)q2.y - A.cy) * A.fx_inv;
        double l0, l1, m0, m1, s;
        er_apply(E, a, b, c, d, l0, l1, m0, m1, s);
        const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
        const double rhs = A.thr2 * den;                           // an infinite rhs would let inf <= inf pass
        n += (er_finite(rhs) && s * s <= rhs) ? 1 : 0;
        const bool in = (mrow ? mrow[i] != 0 : true) && den > 0.0 && er_finite(den);
        const double sd = sqrt(den), r = s / sd, hs = 0.5 * s, dsd = den * sd;
        double J[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            double g0, g1, h0, h1, gs;
            er_apply(G[k], a, b, c, d, g0, g1, h0, h1, gs);
            const double dd = 2.0 * (((l0 * g0 + l1 * g1) + m0 * h0) + m1 * h1);
            J[k] = gs / sd - (hs * dd) / dsd;
        }
        int k = 0;
#pragma unroll
        for (int u = 0; u < 5; u++)
#pragma unroll
            for (int v = u; v < 5; v++, k++) { const double w = J[u] * J[v]; S[k] = S[k] + (in ? w : 0.0); }
#pragma unroll
        for (int u = 0; u < 5; u++) { const double w = J[u] * r; S[15 + u] = S[15 + u] + (in ? w : 0.0); }
        const double e2 = r * r;
        S[20] = S[20] + (in ? e2 : 0.0);
    }
#pragma unroll
    for (int k = 0; k < 21; k++) S[k] = wave_sum(S[k]);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    return n;
}

// the last pass: nothing is solved behind it, so only the cost and the count are taken -- the same operations on the same operands as er_pass
template <int NT = 64>
DEV int er_cost(const double (&R)[9], const double (&t)[3], const float* __restrict__ p1, const float* __restrict__ p2,
                const uint8_t* __restrict__ mrow, int m, int lane, const ERArgs& A, double& cost) {
    double E[9];
    er_xmat(t, R, E);
    double acc = 0.0;
    int n = 0;
    for (int i = lane; i < m; i += NT) {
        const float2 q1 = reinterpret_cast<const float2*>(p1)[i], q2 = reinterpret_cast<const float2*>(p2)[i];
        const double a = ((double)q1.x - A.cx) * A.fx_inv, b = ((double)q1.y - A.cy) * A.fx_inv;
        const double c = ((double)q2.x - A.cx) * A.fx_inv, d = ((double)q2.y - A.cy) * A.fx_inv;
        double l0, l1, m0, m1, s;
        er_apply(E, a, b, c, d, l0, l1, m0, m1, s);
        const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
        const double rhs = A.thr2 * den;                           // an infinite rhs would let inf <= inf pass
        n += (er_finite(rhs) && s * s <= rhs) ? 1 : 0;
        const bool in = (mrow ? mrow[i] != 0 : true) && den > 0.0 && er_finite(den);
        const double r = s / sqrt(den), e2 = r * r;
        acc = acc + (in ? e2 : 0.0);
    }
    cost = wave_sum(acc);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    return n;
}

// d = -(sum J^T J)^-1 sum J^T r by LDL^T without pivoting; false: a pivot that is <= 0 or not finite
DEV bool er_solve5(const double (&S)[21], double (&d)[5]) {
    double Am[5][5], L[5][5], D[5], z[5];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 5; a++)
#pragma unroll
        for (int b = a; b < 5; b++, k++) Am[a][b] = Am[b][a] = S[k];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double s = Am[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (L[j][c] * L[j][c]) * D[c];
        D[j] = s;
        ok = ok && s > 0.0 && er_finite(s);
#pragma unroll
        for (int i = j + 1; i < 5; i++) {
            double v = Am[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) v = v - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = v / s;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        double v = -S[15 + i];
#pragma unroll
        for (int c = 0; c < i; c++) v = v - L[i][c] * z[c];
        z[i] = v;
    }
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        double v = z[i] / D[i];
#pragma unroll
        for (int c = i + 1; c < 5; c++) v = v - L[c][i] * d[c];
        d[i] = v;
    }
    return ok;
}

// R <- C(w) R with the Cayley map C = I + 2 / (1 + |h|^2) ([h]x + [h]x^2), h = w / 2 (p_update of pnp.hip)
DEV void er_rotate(double (&R)[9], double w0, double w1, double w2) {
    const double h[3] = {0.5 * w0, 0.5 * w1, 0.5 * w2};
    const double hh = dot3(h, h), s = 2.0 / (1.0 + hh);
    const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
    double Cm[9], N[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double k2 = i == j ? h[i] * h[j] - hh : h[i] * h[j];
            Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + s * (K[3 * i + j] + k2);
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) N[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = N[k];
}

__global__ __launch_bounds__(64) void k_essential_refine(ERArgs A, const double* __restrict__ start, const float* __restrict__ p1,
                                                         const float* __restrict__ p2, const int32_t* __restrict__ npts,
                                                         const uint8_t* __restrict__ mask, vis_eref_result* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const double* rec = start + (size_t)row * A.rec_stride;
    double R[9], t[3];
    bool any = false, fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) { R[k] = rec[A.r_off + k]; any = any || R[k] != 0.0; fin = fin && er_finite(R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { t[k] = rec[A.t_off + k]; fin = fin && er_finite(t[k]); }
    const double tt = dot3(t, t);
    vis_eref_result* o = out + row;
    if (!any || !fin || !(tt > 0.0) || !er_finite(tt)) {           // (uniform) no pose to start from: the zero record
        static_assert(sizeof(vis_eref_result) == 216 && offsetof(vis_eref_result, flags) == 208, "27 words of 8 bytes, flags in the low half of the last");
        if (lane < 27) reinterpret_cast<unsigned long long*>(o)[lane] = lane == 26 ? (unsigned long long)VIS_ER_NO_POSE : 0ull;
        return;
    }
    const double nt = sqrt(tt);
    t[0] = t[0] / nt; t[1] = t[1] / nt; t[2] = t[2] / nt;
    const int m = min(max(npts[row], 0), A.in_stride);
    const float* r1 = p1 + (size_t)row * A.in_stride * 2;
    const float* r2 = p2 + (size_t)row * A.in_stride * 2;
    const uint8_t* mrow = mask ? mask + (size_t)row * A.row_cap : nullptr;
    int nused = 0;
    for (int i = lane; i < m; i += 64) nused += (mrow ? mrow[i] != 0 : true) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) nused += __shfl_xor(nused, off);
    const bool run = A.refine_iters > 0 && nused >= A.min_inliers;
    const int passes = run ? A.refine_iters : 0;
    double Rb[9], tb[3], S[21];
    double cost0 = 0.0, cost1 = 0.0;
    int nin0 = 0, nin1 = 0, best = 0, steps = 0;
    for (int step = 0; step <= passes; step++) {                   // (uniform: every lane holds the same sums)
        double cost;
        int nin;
        if (step == passes) nin = er_cost(R, t, r1, r2, mrow, m, lane, A, cost);
        else { nin = er_pass(R, t, r1, r2, mrow, m, lane, A, S); cost = S[20]; }
        const bool take = step == 0 || (er_finite(cost) && (!er_finite(cost1) || cost < cost1));
        if (step == 0) { cost0 = cost; nin0 = nin; }
        if (take) {
            cost1 = cost; nin1 = nin; best = step;
#pragma unroll
            for (int k = 0; k < 9; k++) Rb[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) tb[k] = t[k];
        }
        if (step == passes) break;
        double d[5];
        if (!er_solve5(S, d)) break;
        er_rotate(R, d[0], d[1], d[2]);
        er_move_t(t, d[3], d[4]);
        steps++;
    }
    if (lane != 0) return;
    vis_eref_result r;
    double Eb[9];
    er_xmat(tb, Rb, Eb);
#pragma unroll
    for (int k = 0; k < 9; k++) { r.R[k] = Rb[k]; r.E[k] = Eb[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) r.t[k] = tb[k];
    r.cost0 = cost0; r.cost1 = cost1;
    r.n_used = nused; r.n_points = m; r.n_inliers0 = nin0; r.n_inliers_refined = nin1;
    r.best_step = best; r.steps_run = steps;
    r.flags = run ? (best > 0 ? VIS_ER_REFINED : VIS_ER_REJECTED) : (nused < A.min_inliers ? VIS_ER_FEW : 0);
    r.reserved_ = 0;
    *o = r;
}

// ep has been validated by the entry point.  d_start: n records of rec_stride doubles that hold R at r_off and t at t_off; d_p1 / d_p2: n rows of
// in_stride (x, y) pixels, d_npts of them valid (clamped); d_mask: rows of row_cap >= in_stride bytes, or null.  On ctx->stream.
int essential_refine_run(vis_ctx* ctx, const vis_eref_params* ep, int n, int in_stride, const double* d_start, int rec_stride, int r_off, int t_off,
                         const float* d_p1, const float* d_p2, const int32_t* d_npts, int row_cap, const uint8_t* d_mask, vis_eref_result* d_out) {
    if (n <= 0) return VIS_OK;
    ERArgs A;
    A.cx = ctx->p.cx; A.cy = ctx->p.cy; A.fx_inv = 1. / ctx->p.fx;
    const double thr = ep->threshold_px / ctx->p.fx;
    A.thr2 = thr * thr;
    A.refine_iters = ep->refine_iters; A.min_inliers = ep->min_inliers; A.in_stride = in_stride; A.row_cap = row_cap;
    A.rec_stride = rec_stride; A.r_off = r_off; A.t_off = t_off;
    hipLaunchKernelGGL(k_essential_refine, dim3(n), dim3(64), 0, ctx->stream, A, d_start, d_p1, d_p2, d_npts, d_mask, d_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

// ---- k_essential_polish: the refinement with its set re-selected under the pose it reached (include/vislam_hip.h states the algorithm and the
// summation contract "T", tests/essential_polish_ref.py restates both).  NW waves walk a pair: thread tid of NT = 64 NW owns the points
// i = tid mod NT, so er_pass<NT> / er_cost<NT> leave wave w with W_w, and ep_totals (ep_sums.h) adds the wave totals in rising w on every thread: the same bits
// everywhere, hence uniform control flow around the barriers.  NW = 1 is the one-wave kernel's order as it stands (W_1 = W_2 = W_3 = +0.0 and a
// W is never -0.0); a row of at most 64 points gives the same bits under either NW.  The set lives in the caller's output mask row: byte i is
// read and written by thread i mod NT alone, so no barrier guards it.
struct EPArgs {
    ERArgs er;                         // thr2 = (select_px / fx)^2; row_cap: of the input mask
    int rounds, out_cap;               // out_cap: bytes between two rows of the output mask
};

// the selection under the pose (R, t): bit 1 of byte i <- point i passes (thr2 den finite and s s <= thr2 den: er_pass's count, point for point);
// bit 0 stays the current set.  nnew: the points that pass, nchg: the bytes the selection would flip (this thread's share of both)
template <int NT>
DEV void ep_select(const double (&R)[9], const double (&t)[3], const float* __restrict__ p1, const float* __restrict__ p2, uint8_t* srow, int m, int tid,
                   const ERArgs& A, int& nnew, int& nchg) {
    double E[9];
    er_xmat(t, R, E);
    nnew = 0; nchg = 0;
    for (int i = tid; i < m; i += NT) {
        const float2 q1 = reinterpret_cast<const float2*>(p1)[i], q2 = reinterpret_cast<const float2*>(p2)[i];
        const double a = ((double)q1.x - A.cx) * A.fx_inv, b = ((double)q1.y - A.cy) * A.fx_inv;
        const double c = ((double)q2.x - A.cx) * A.fx_inv, d = ((double)q2.y - A.cy) * A.fx_inv;
        double l0, l1, m0, m1, s;
        er_apply(E, a, b, c, d, l0, l1, m0, m1, s);
        const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
        const double rhs = A.thr2 * den;                           // an infinite rhs would let inf <= inf pass
        const int pass = (er_finite(rhs) && s * s <= rhs) ? 1 : 0;
        const int cur = srow[i];
        srow[i] = (uint8_t)(cur | (pass << 1));
        nnew += pass; nchg += pass ^ cur;
    }
}

static_assert(sizeof(vis_epolish_result) == 224 && offsetof(vis_epolish_result, flags) == 220, "28 words of 8 bytes, flags in the high half of the last");
static_assert(sizeof(PoseOut) == 192 && offsetof(PoseOut, E) == 0 && offsetof(PoseOut, R) == 72 && offsetof(PoseOut, t) == 144 &&
              offsetof(PoseOut, n_inliers) == 168, "the record k_essential_polish starts from and writes");

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_essential_polish(EPArgs P, const PoseOut* __restrict__ pose, const float* __restrict__ p1,
                                                              const float* __restrict__ p2, const int32_t* __restrict__ npts,
                                                              const uint8_t* __restrict__ mask, uint8_t* mask_out,
                                                              vis_epolish_result* __restrict__ out, PoseOut* __restrict__ pose_out) {
    constexpr int NT = 64 * NW;
    const ERArgs& A = P.er;
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* rec = reinterpret_cast<const double*>(pose + row);
    double R[9], t[3];
    bool any = false, fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) { R[k] = rec[9 + k]; any = any || R[k] != 0.0; fin = fin && er_finite(R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { t[k] = rec[18 + k]; fin = fin && er_finite(t[k]); }
    const double tt = dot3(t, t);
    vis_epolish_result* o = out + row;
    if (!any || !fin || !(tt > 0.0) || !er_finite(tt)) {           // (uniform) no pose to start from: the zero record, the input record as it is
        if (tid < 28) reinterpret_cast<unsigned long long*>(o)[tid] = tid == 27 ? (unsigned long long)VIS_EP_NO_POSE << 32 : 0ull;
        if (pose_out && tid < 24) reinterpret_cast<unsigned long long*>(pose_out + row)[tid] = reinterpret_cast<const unsigned long long*>(rec)[tid];
        return;
    }
    const double nt = sqrt(tt);
    t[0] = t[0] / nt; t[1] = t[1] / nt; t[2] = t[2] / nt;
    const int m = min(max(npts[row], 0), A.in_stride);
    const float* r1 = p1 + (size_t)row * A.in_stride * 2;
    const float* r2 = p2 + (size_t)row * A.in_stride * 2;
    const uint8_t* mrow = mask ? mask + (size_t)row * A.row_cap : nullptr;
    uint8_t* srow = mask_out + (size_t)row * P.out_cap;
    int nset = 0, nchg = 0;
    for (int i = tid; i < m; i += NT) {                            // set 0
        const int in = (mrow ? mrow[i] != 0 : true) ? 1 : 0;
        srow[i] = (uint8_t)in;
        nset += in;
    }
    ep_counts<NW>(nset, nchg);
    const int nfirst = nset;
    const bool run = nset >= A.min_inliers;
    const int passes = run ? A.refine_iters : 0, rounds = run ? P.rounds : 0;
    double Rb[9], tb[3], S[21];
    double cost_first = 0.0, cost0 = 0.0, cost1 = 0.0;
    int best = 0, steps = 0, rounds_run = 0;
    bool shrank = false, moved = false;
#pragma unroll
    for (int k = 0; k < 9; k++) Rb[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) tb[k] = t[k];
    for (int round = 0; round <= rounds; round++) {                // (uniform: every thread holds the same sums and counts)
        if (round > 0) {
            int nnew;
            ep_select<NT>(Rb, tb, r1, r2, srow, m, tid, A, nnew, nchg);
            ep_counts<NW>(nnew, nchg);
            const bool adopt = nchg != 0 && nnew >= A.min_inliers;
            for (int i = tid; i < m; i += NT) { const int v = srow[i]; srow[i] = (uint8_t)(adopt ? v >> 1 : v & 1); }
            if (nchg == 0) break;
            if (!adopt) { shrank = true; break; }
            nset = nnew;
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rb[k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = tb[k];
        }
        for (int step = 0; step <= passes; step++) {               // k_essential_refine's passes over the current set
            double cost[1];
            int nin;
            if (step == passes) { nin = er_cost<NT>(R, t, r1, r2, srow, m, tid, A, cost[0]); ep_totals<NW>(cost, nin); }
            else { nin = er_pass<NT>(R, t, r1, r2, srow, m, tid, A, S); ep_totals<NW>(S, nin); cost[0] = S[20]; }
            const bool take = step == 0 || (er_finite(cost[0]) && (!er_finite(cost1) || cost[0] < cost1));
            if (step == 0) { cost0 = cost[0]; if (round == 0) cost_first = cost[0]; }
            if (take) {
                cost1 = cost[0]; best = step;
#pragma unroll
                for (int k = 0; k < 9; k++) Rb[k] = R[k];
#pragma unroll
                for (int k = 0; k < 3; k++) tb[k] = t[k];
            }
            if (step == passes) break;
            double d[5];
            if (!er_solve5(S, d)) break;
            er_rotate(R, d[0], d[1], d[2]);
            er_move_t(t, d[3], d[4]);
            steps++;
        }
        rounds_run += run ? 1 : 0;
        moved = moved || best > 0;
    }
    if (tid != 0) return;
    vis_epolish_result r;
    double Eb[9];
    er_xmat(tb, Rb, Eb);
#pragma unroll
    for (int k = 0; k < 9; k++) { r.R[k] = Rb[k]; r.E[k] = Eb[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) r.t[k] = tb[k];
    r.cost_first = cost_first; r.cost0 = cost0; r.cost1 = cost1;
    r.n_points = m; r.n_set_first = nfirst; r.n_set_last = nset; r.n_changed = nchg;
    r.rounds_run = rounds_run; r.steps_run = steps; r.best_step = best;
    r.flags = (run ? (moved ? VIS_EP_POLISHED : VIS_EP_REJECTED) : VIS_EP_FEW) | (shrank ? VIS_EP_SHRANK : 0);
    *o = r;
    if (pose_out) {
        PoseOut q = pose[row];
#pragma unroll
        for (int k = 0; k < 9; k++) { q.E[k] = Eb[k]; q.R[k] = Rb[k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) q.t[k] = tb[k];
        q.n_inliers = nset;
        pose_out[row] = q;
    }
}

// ep has been validated by the entry point.  d_pose: n pose records; d_p1 / d_p2: n rows of in_stride (x, y) pixels, d_npts of them valid (clamped);
// d_mask: rows of mask_cap >= in_stride bytes, or null; d_mask_out: rows of out_cap >= in_stride bytes; d_pose_out: n records or null.  On ctx->stream.
int essential_polish_run(vis_ctx* ctx, const vis_epolish_params* ep, int n, int in_stride, const PoseOut* d_pose, const float* d_p1, const float* d_p2,
                         const int32_t* d_npts, int mask_cap, const uint8_t* d_mask, int out_cap, uint8_t* d_mask_out, vis_epolish_result* d_out,
                         PoseOut* d_pose_out) {
    if (n <= 0) return VIS_OK;
    EPArgs P;
    ERArgs& A = P.er;
    A.cx = ctx->p.cx; A.cy = ctx->p.cy; A.fx_inv = 1. / ctx->p.fx;
    const double thr = ep->select_px / ctx->p.fx;
    A.thr2 = thr * thr;
    A.refine_iters = ep->refine_iters; A.min_inliers = ep->min_inliers; A.in_stride = in_stride; A.row_cap = mask_cap;
    A.rec_stride = (int)(sizeof(PoseOut) / 8); A.r_off = 9; A.t_off = 18;
    P.rounds = ep->rounds; P.out_cap = out_cap;
    if (in_stride <= 64)
        hipLaunchKernelGGL(k_essential_polish<1>, dim3(n), dim3(64), 0, ctx->stream, P, d_pose, d_p1, d_p2, d_npts, d_mask, d_mask_out, d_out, d_pose_out);
    else
        hipLaunchKernelGGL(k_essential_polish<4>, dim3(n), dim3(256), 0, ctx->stream, P, d_pose, d_p1, d_p2, d_npts, d_mask, d_mask_out, d_out, d_pose_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

// vis_essential_batch's mask: the pose stage writes rows of in_stride bytes, the caller's rows are row_cap bytes apart; bytes beyond a row's points
// are left untouched
__global__ void k_mask_rows(int in_stride, int row_cap, const int32_t* __restrict__ npts, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
    const int row = blockIdx.x;
    const int m = min(max(npts[row], 0), in_stride);
    for (int i = threadIdx.x; i < m; i += blockDim.x) dst[(size_t)row * row_cap + i] = src[(size_t)row * in_stride + i];
}
int mask_rows_run(vis_ctx* ctx, int n, int in_stride, int row_cap, const int32_t* d_npts, const uint8_t* d_src, uint8_t* d_dst) {
    if (n <= 0 || in_stride <= 0) return VIS_OK;
    hipLaunchKernelGGL(k_mask_rows, dim3(n), dim3(256), 0, ctx->stream, in_stride, row_cap, d_npts, d_src, d_dst);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
