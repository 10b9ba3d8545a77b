// homography.hip -- homography RANSAC and the H-or-E model choice for every pair of a batch on gfx950, FP64 VALU.
//
// The other half of a two-view initialiser (Mur-Artal, Montiel, Tardos: ORB-SLAM, 2015, section IV): a four-point homography RANSAC next
// to the essential one of pose.hip and a score that says which model explains the correspondences.  The contract -- coordinates,
// thresholds, the closed-form solver, the division-free test, the scores and the decision -- is stated in include/vislam_hip.h and
// restated operation for operation in tests/homography_ref.py; this file must keep every product and sum parenthesised as written
// there (the library is built with -ffp-contract=off).
//
// k_homography_batch has the shape of ransac_lanes.h: one workgroup per pair, the hypotheses spread over the lanes (IPL per lane), the
// correspondences walked in LDS tiles of VIS_H_TILE normalised (x1, y1, x2, y2), the winner the maximum key over the workgroup (a slot
// is an iteration).  A lane holds H and adj(H) of its hypotheses in registers, 18 doubles per slot; the solver is a closed form whose
// every index is a constant (pose.hip's comment on jacobi_eig has the reason: a run-time index puts the matrices into scratch memory).
// The first wave then recomputes the winner from its draws -- the same expressions, so the same bits as the lane that counted it -- and
// computes mask, scores and the decision; the sums run over 64 partial sums (i mod 64, rising i) and a fixed butterfly, whatever <NT, IPL>
// the launch has, so the record does not depend on the shape.
#include "vis_internal.h"
#include "ransac_lanes.h"
#include "h_transfer.h"                // h_adj, h_transfer
#include <cmath>
#include <cfloat>

#define H_TILE VIS_H_TILE              // 512 points = 16 KiB of LDS (public: the tests size their rows around it)

struct HArgs {
    double cx, cy, fx_inv;             // k_pose_prep's normalisation
    double s2, t_h, t_e, t_self;       // (sigma_px fx_inv)^2, chi2_h s2, chi2_e s2, t_h 2^-20
    double chi2_h, h_ratio;
    int iters, min_inliers, in_stride, row_cap, e_stride;
};
struct alignas(32) HPt { double x1, y1, x2, y2; };

DEV bool h_bad(double v) { return !(v != 0.0) || !(fabs(v) <= DBL_MAX); }      // zero, NaN or infinite

DEV HPt h_point(const float* __restrict__ q1, const float* __restrict__ q2, int i, const HArgs& A) {
    const float2 a = reinterpret_cast<const float2*>(q1)[i], b = reinterpret_cast<const float2*>(q2)[i];
    HPt p;
    p.x1 = ((double)a.x - A.cx) * A.fx_inv; p.y1 = ((double)a.y - A.cy) * A.fx_inv;
    p.x2 = ((double)b.x - A.cx) * A.fx_inv; p.y2 = ((double)b.y - A.cy) * A.fx_inv;
    return p;
}

// the projective basis of four points (x_k, y_k, 1): M = [l0 p0 | l1 p1 | l2 p2] row-major; false: a zero or non-finite l or determinant
DEV bool h_basis(const double (&x)[4], const double (&y)[4], double (&M)[9]) {
    const double p0[3] = {x[0], y[0], 1.0}, p1[3] = {x[1], y[1], 1.0}, p2[3] = {x[2], y[2], 1.0}, p3[3] = {x[3], y[3], 1.0};
    double c12[3], c20[3], c01[3];
    cross3(p1, p2, c12); cross3(p2, p0, c20); cross3(p0, p1, c01);
    const double l0 = dot3(c12, p3), l1 = dot3(c20, p3), l2 = dot3(c01, p3), det = dot3(c01, p2);
    M[0] = l0 * p0[0]; M[1] = l1 * p1[0]; M[2] = l2 * p2[0];
    M[3] = l0 * p0[1]; M[4] = l1 * p1[1]; M[5] = l2 * p2[1];
    M[6] = l0 * p0[2]; M[7] = l1 * p1[2]; M[8] = l2 * p2[2];
    return !(h_bad(l0) || h_bad(l1) || h_bad(l2) || h_bad(det));
}

DEV bool h_inlier(const double (&H)[9], const double (&G)[9], const HPt& p, double t) {
    double e, ww;
    h_transfer(H, p.x1, p.y1, p.x2, p.y2, e, ww);
    const bool f = e <= t * ww;
    h_transfer(G, p.x2, p.y2, p.x1, p.y1, e, ww);
    return f && e <= t * ww;
}

// hypothesis of iteration j: H = B adj(A), G = adj(H); false: skipped (equal indices, a degenerate basis, or H misses its own sample)
DEV bool h_hypothesis(const int32_t* __restrict__ draws, int j, int m, const float* __restrict__ q1, const float* __restrict__ q2,
                      const HArgs& A, double (&H)[9], double (&G)[9]) {
    int idx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = (int)((unsigned)(draws[4 * (size_t)j + k] & 0x7fffffff) % (unsigned)m);
    if (idx[0] == idx[1] || idx[0] == idx[2] || idx[0] == idx[3] || idx[1] == idx[2] || idx[1] == idx[3] || idx[2] == idx[3]) return false;
    HPt s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = h_point(q1, q2, idx[k], A);
    const double x1[4] = {s[0].x1, s[1].x1, s[2].x1, s[3].x1}, y1[4] = {s[0].y1, s[1].y1, s[2].y1, s[3].y1};
    const double x2[4] = {s[0].x2, s[1].x2, s[2].x2, s[3].x2}, y2[4] = {s[0].y2, s[1].y2, s[2].y2, s[3].y2};
    double Am[9], Bm[9], Aa[9];
    const bool ok_a = h_basis(x1, y1, Am), ok_b = h_basis(x2, y2, Bm);
    if (!ok_a || !ok_b) return false;
    h_adj(Am, Aa);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) H[3 * r + c] = (Bm[3 * r] * Aa[c] + Bm[3 * r + 1] * Aa[3 + c]) + Bm[3 * r + 2] * Aa[6 + c];
    h_adj(H, G);
    bool own = true;
#pragma unroll
    for (int k = 0; k < 4; k++) own = own && h_inlier(H, G, s[k], A.t_self);
    return own;
}

template <int NS, int IPL>
DEV void h_count_tile(const HPt* s_pt, int nt, const double (&H)[IPL][9], const double (&G)[IPL][9], int (&cnt)[IPL], double t_h) {
    static_assert(NS <= IPL, "slots");
    for (int i = 0; i < nt; i++) {
        const HPt p = s_pt[i];
#pragma unroll
        for (int s = 0; s < NS; s++) cnt[s] += h_inlier(H[s], G[s], p, t_h) ? 1 : 0;
    }
}

template <int NT, int IPL>
__global__ __launch_bounds__(NT) void k_homography_batch(HArgs A, const float* __restrict__ p1, const float* __restrict__ p2,
                                                         const int32_t* __restrict__ npts, const int32_t* __restrict__ draws,
                                                         const double* __restrict__ Ein, uint8_t* __restrict__ mask,
                                                         vis_homography_result* __restrict__ out) {
    __shared__ HPt s_pt[H_TILE];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(npts[pair], 0), A.in_stride);
    uint8_t* mrow = mask ? mask + (size_t)pair * A.row_cap : nullptr;
    vis_homography_result r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.H[k] = 0.0;
    r.score_h = r.score_e = 0.0; r.n_inliers = 0; r.n_points = 0; r.best_iter = -1; r.n_degenerate = 0; r.n_inliers_e = 0; r.model = VIS_MODEL_NONE;
    if (m < 4 || A.iters <= 0) {                                   // (uniform: the whole workgroup leaves)
        if (mrow) for (int i = tid; i < m; i += NT) mrow[i] = 0;
        if (tid == 0) out[pair] = r;
        return;
    }
    const float* q1 = p1 + (size_t)pair * A.in_stride * 2;
    const float* q2 = p2 + (size_t)pair * A.in_stride * 2;
    const auto fill = [&](int i) { return h_point(q1, q2, i, A); };
    const bool single = rl_first_tile<H_TILE, NT>(s_pt, m, fill);
    unsigned long long best = 0;                                   // 0: no iteration with a count > 0 yet
    int ndeg = 0;
    for (int j0 = 0; j0 < A.iters; j0 += NT * IPL) {
        double H[IPL][9], G[IPL][9]; int cnt[IPL]; bool live[IPL];
#pragma unroll
        for (int s = 0; s < IPL; s++) {
            const int j = j0 + s * NT + tid;
            cnt[s] = 0;
            live[s] = j < A.iters;
            if (live[s]) { live[s] = h_hypothesis(draws, j, m, q1, q2, A, H[s], G[s]); if (!live[s]) ndeg++; }
            if (!live[s]) {
#pragma unroll
                for (int k = 0; k < 9; k++) H[s][k] = G[s][k] = 0.0;
            }
        }
        const int nslots = rl_round_slots<NT, IPL>(j0, A.iters);
        rl_walk_tiles<H_TILE, NT>(s_pt, m, single, rl_wave_live(j0, A.iters), fill, [&](const HPt* tile, int nt) {
            rl_for_slots<1, IPL>(nslots, [&](auto ns) { h_count_tile<decltype(ns)::value, IPL>(tile, nt, H, G, cnt, A.t_h); });
        });
#pragma unroll
        for (int s = 0; s < IPL; s++) (void)rl_offer(best, live[s], cnt[s], j0 + s * NT + tid);
    }
    int sums[1] = {ndeg};
    rl_block_reduce<NT>(best, sums);
    if (tid >= 64) return;
    r.n_points = m; r.n_degenerate = sums[0];
    // ---- the first wave: the winner again from its draws, then mask, scores and decision over the points in strides of 64
    double H[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] = G[k] = 0.0;
    const bool won = best != 0;
    int it = -1;
    if (won) {
        it = rl_key_slot(best);
        (void)h_hypothesis(draws, it, m, q1, q2, A, H, G);
    }
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = Ein ? Ein[(size_t)pair * A.e_stride + k] : 0.0;
    double sh = 0.0, se = 0.0;
    int nin = 0, nine = 0;
    for (int i = tid; i < m; i += 64) {
        const HPt p = h_point(q1, q2, i, A);
        if (won) {
            double e, ww;
            h_transfer(H, p.x1, p.y1, p.x2, p.y2, e, ww);
            const bool f = e <= A.t_h * ww;
            const double df = e / ww;
            h_transfer(G, p.x2, p.y2, p.x1, p.y1, e, ww);
            const bool b = e <= A.t_h * ww;
            const double db = e / ww;
            const double tf = df <= A.t_h ? A.chi2_h - df / A.s2 : 0.0, tb = db <= A.t_h ? A.chi2_h - db / A.s2 : 0.0;
            sh = sh + (tf + tb);
            nin += (f && b) ? 1 : 0;
            if (mrow) mrow[i] = (f && b) ? 1 : 0;
        } else if (mrow) mrow[i] = 0;
        if (Ein) {
            const double l2a = (E[0] * p.x1 + E[1] * p.y1) + E[2], l2b = (E[3] * p.x1 + E[4] * p.y1) + E[5], l2c = (E[6] * p.x1 + E[7] * p.y1) + E[8];
            const double l1a = (E[0] * p.x2 + E[3] * p.y2) + E[6], l1b = (E[1] * p.x2 + E[4] * p.y2) + E[7];
            const double rr = (p.x2 * l2a + p.y2 * l2b) + l2c, r2 = rr * rr;
            const double n2 = l2a * l2a + l2b * l2b, n1 = l1a * l1a + l1b * l1b;
            const bool i2 = n2 > 0.0 && r2 <= A.t_e * n2, i1 = n1 > 0.0 && r2 <= A.t_e * n1;
            const double t2 = i2 ? A.chi2_h - (r2 / n2) / A.s2 : 0.0, t1 = i1 ? A.chi2_h - (r2 / n1) / A.s2 : 0.0;
            se = se + (t2 + t1);
            nine += (i2 && i1) ? 1 : 0;
        }
    }
    sh = wave_sum(sh); se = wave_sum(se);
    for (int off = 32; off > 0; off >>= 1) { nin += __shfl_xor(nin, off); nine += __shfl_xor(nine, off); }
    if (tid != 0) return;
    r.score_h = sh; r.score_e = se; r.n_inliers = nin; r.n_inliers_e = nine; r.best_iter = it;
    const bool offer_h = won && nin >= A.min_inliers, offer_e = Ein != nullptr && nine >= A.min_inliers;
    r.model = offer_h && (!offer_e || sh > A.h_ratio * (sh + se)) ? VIS_MODEL_HOMOGRAPHY : offer_e ? VIS_MODEL_ESSENTIAL : VIS_MODEL_NONE;
    if (won) {
        const double det = (H[0] * G[0] + H[1] * G[3]) + H[2] * G[6];
        double ss = H[0] * H[0];
#pragma unroll
        for (int k = 1; k < 9; k++) ss = ss + H[k] * H[k];
        const double nrm = sqrt(ss), sg = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int k = 0; k < 9; k++) r.H[k] = (sg * H[k]) / nrm;
    }
    out[pair] = r;
}

// hp has been validated by the entry point.  d_p1 / d_p2: npairs rows of in_stride (x, y) points, d_npts of them valid (clamped); d_E: records of
// e_stride doubles whose first nine are E, or null; d_mask: rows of row_cap >= in_stride bytes, or null; d_draws: iters x 4.  On ctx->stream.
int homography_batch_run(vis_ctx* ctx, const vis_homography_params* hp, int npairs, int in_stride, const float* d_p1, const float* d_p2,
                         const int32_t* d_npts, const int32_t* d_draws, const double* d_E, int e_stride, int row_cap, uint8_t* d_mask,
                         vis_homography_result* d_out) {
    if (npairs <= 0) return VIS_OK;
    HArgs A;
    A.cx = ctx->p.cx; A.cy = ctx->p.cy; A.fx_inv = 1. / ctx->p.fx;
    const double s = hp->sigma_px * A.fx_inv;
    A.s2 = s * s; A.t_h = hp->chi2_h * A.s2; A.t_e = hp->chi2_e * A.s2; A.t_self = A.t_h * 0x1p-20;
    A.chi2_h = hp->chi2_h; A.h_ratio = hp->h_ratio;
    A.iters = hp->iters; A.min_inliers = hp->min_inliers; A.in_stride = in_stride; A.row_cap = row_cap; A.e_stride = e_stride;
    // rows of up to one tile (the good matches: thousands of small pairs beside the detect chain): two waves, two hypotheses per point read;
    // longer rows (VIS_POSE_SYM: tens of pairs of thousands of points): four waves per pair.  Either shape holds 256 hypotheses per round.
    if (in_stride > H_TILE) hipLaunchKernelGGL((k_homography_batch<256, 1>), dim3(npairs), dim3(256), 0, ctx->stream, A, d_p1, d_p2, d_npts, d_draws, d_E, d_mask, d_out);
    else hipLaunchKernelGGL((k_homography_batch<128, 2>), dim3(npairs), dim3(128), 0, ctx->stream, A, d_p1, d_p2, d_npts, d_draws, d_E, d_mask, d_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
