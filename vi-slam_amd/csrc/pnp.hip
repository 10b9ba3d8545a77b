// pnp.hip -- PnP for every problem of a batch on gfx950, FP64 VALU: P3P RANSAC against map points, then Gauss-Newton over the winner's inliers.
//
// The pose of a frame against points that are already triangulated (x_cam = R X + t, X in the map's frame and units).  The contract --
// coordinates, the quartic of Grunert's P3P, the root finder, the two triads, the division-free test, the winner, the refinement and its
// summation order -- is stated in include/vislam_hip.h and restated operation for operation in tests/pnp_ref.py; this file must keep every
// product and sum parenthesised as written there (the library is built with -ffp-contract=off).
//
// k_pnp_batch has the shape of ransac_lanes.h: one workgroup per problem, one three-point sample per lane with its up to four poses in
// registers (48 doubles; DESIGN.md section 4.12 has the resource table that decided against four lanes per sample: the root finder runs in
// lock step over a wave either way, so a lane per root only quarters the samples a wave's solver pass serves), the correspondences walked
// in LDS tiles of VIS_PNP_TILE (X, x, y), the winner the maximum key over the workgroup (a slot is 4 sample + root).  Every
// index into a pose, a root list or a matrix is a compile-time constant (pose.hip's comment on jacobi_eig has the reason).  A lane keeps
// the pose behind its own best key in LDS and the first wave reads the one of the lane that holds the workgroup's (solving the winner a second time,
// as k_homography_batch does, would double the kernel: the solver, not the test, is what a short row costs); the first wave then
// writes mask and counts.
// k_pnp_refine: one wave per problem; every sum over 64 partial sums (i mod 64, rising i) and a fixed butterfly; the 6 x 6 solve on every
// lane alike (they hold the same sums), which is the one-lane solve without a broadcast.
#include "vis_internal.h"
#include "ransac_lanes.h"
#include <cmath>
#include <cfloat>

#define P_TILE VIS_PNP_TILE            // 512 points = 24 KiB of LDS (public: the tests size their rows around it)
#define P_INNER 40                     // halvings that separate the roots of a derivative
#define P_FINAL 100                    // halvings of the quartic itself: the interval stops shrinking long before

struct PArgs {
    double cx, cy, fx_inv, thr2;       // k_pose_prep's normalisation; (threshold_px fx_inv)^2
    int iters, min_inliers, refine_iters, in_stride, x_stride, row_cap;
};
struct alignas(16) PPt { double X[3], x, y, pad_; };               // 48 bytes: the broadcast read is three aligned 16-byte loads

DEV bool p_finite(double v) { return fabs(v) <= DBL_MAX; }         // false for a NaN

DEV PPt p_point(const double* __restrict__ Xr, const float* __restrict__ xyr, int i, const PArgs& A) {
    const float2 a = reinterpret_cast<const float2*>(xyr)[i];
    const double* X = Xr + (size_t)i * A.x_stride;
    PPt p;
    p.X[0] = X[0]; p.X[1] = X[1]; p.X[2] = X[2];
    p.x = ((double)a.x - A.cx) * A.fx_inv; p.y = ((double)a.y - A.cy) * A.fx_inv;
    p.pad_ = 0.0;
    return p;
}

// (U, V, W) = R X + t of a pose P = (R row-major, t)
DEV void p_transform(const double (&P)[12], const double* X, double& U, double& V, double& W) {
    U = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[9];
    V = ((P[3] * X[0] + P[4] * X[1]) + P[5] * X[2]) + P[10];
    W = ((P[6] * X[0] + P[7] * X[1]) + P[8] * X[2]) + P[11];
}
DEV bool p_inlier(const double (&P)[12], const PPt& q, double thr2) {
    double U, V, W;
    p_transform(P, q.X, U, V, W);
    const double du = U - q.x * W, dv = V - q.y * W;
    const double rhs = thr2 * (W * W);                              // an overflowed rhs would let inf <= inf pass under every pose
    return W > 0.0 && p_finite(rhs) && (du * du + dv * dv) <= rhs;
}

// ---- the real roots of a polynomial of degree D in (0, B): derivative interlacing (oracle/pose.cpp real_roots), one level
template <int D> DEV double p_horner(const double (&q)[5], double x) {
    double r = q[D];
#pragma unroll
    for (int i = D - 1; i >= 0; i--) r = r * x + q[i];
    return r;
}
template <int D, int NIT> DEV int p_level(const double (&q)[5], double B, const double (&prev)[4], int nprev, double (&cur)[4]) {
    int ncur = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) {                                  // interval j of the nprev + 1 the previous level's roots cut (0, B) into
        double lo = j == 0 ? 0.0 : prev[j - 1];
        double hi = j == nprev ? B : prev[j];
        const double flo = p_horner<D>(q, lo), fhi = p_horner<D>(q, hi);
        const bool found = j <= nprev && ((flo < 0.0) != (fhi < 0.0));
        bool act = found;
        for (int it = 0; it < NIT; it++) {
            const double mid = 0.5 * (lo + hi);
            act = act && mid > lo && mid < hi;                     // an interval that cannot shrink stays as it is
            if (!__any(act)) break;                                // (no lane of the wave has anything left: the results do not depend on it)
            const double fm = p_horner<D>(q, mid);
            const bool left = (fm < 0.0) == (flo < 0.0);
            if (act) { if (left) lo = mid; else hi = mid; }
        }
        const double root = 0.5 * (lo + hi);
        if (found) {
#pragma unroll
            for (int k = 0; k < 4; k++) if (ncur == k) cur[k] = root;
            ncur++;
        }
    }
    return ncur;
}
// ascending real roots in (0, B) of c[0] + ... + c[4] v^4 (roots of even multiplicity are not reported)
DEV int p_quartic_roots(const double (&c)[5], double B, double (&roots)[4]) {
    const double q3[5] = {6.0 * c[3], 24.0 * c[4], 0.0, 0.0, 0.0};
    const double q2[5] = {2.0 * c[2], 6.0 * c[3], 12.0 * c[4], 0.0, 0.0};
    const double q1[5] = {c[1], 2.0 * c[2], 3.0 * c[3], 4.0 * c[4], 0.0};
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    double r3[4], r2[4], r1[4];
    const int n3 = p_level<1, P_INNER>(q3, B, none, 0, r3);
    const int n2 = p_level<2, P_INNER>(q2, B, r3, n3, r2);
    const int n1 = p_level<3, P_INNER>(q1, B, r2, n2, r1);
    return p_level<4, P_FINAL>(c, B, r1, n1, roots);
}

DEV void p_bearing(double x, double y, double* f) {
    const double n = sqrt((x * x + y * y) + 1.0);
    f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}

// the sample's geometry that every root shares
struct PSample {
    double P0[3], f0[3], f1[3], f2[3];
    double e1[3], e2[3], e3[3];                                    // the world triad
    double b2, p, pm1, ca, cb, cg;
};

// the pose of root v: false = dropped (u, the denominator or s0^2 fails its sign test, or the camera triad is collinear)
DEV bool p_solution(const PSample& S, double v, double (&P)[12]) {
    const double den = 2.0 * (S.cg - v * S.ca);
    if (!(den != 0.0) || !p_finite(den)) return false;
    const double u = (((S.pm1 * (v * v) - ((2.0 * S.p) * S.cb) * v) + 1.0) + S.p) / den;
    if (!(v > 0.0) || !(u > 0.0)) return false;
    const double w = (1.0 + v * v) - (2.0 * v) * S.cb;
    if (!(w > 0.0)) return false;
    const double s0 = sqrt(S.b2 / w), s1 = u * s0, s2 = v * s0;
    const double Q0[3] = {s0 * S.f0[0], s0 * S.f0[1], s0 * S.f0[2]};
    const double q01[3] = {s1 * S.f1[0] - Q0[0], s1 * S.f1[1] - Q0[1], s1 * S.f1[2] - Q0[2]};
    const double q02[3] = {s2 * S.f2[0] - Q0[0], s2 * S.f2[1] - Q0[1], s2 * S.f2[2] - Q0[2]};
    double nq[3];
    cross3(q01, q02, nq);
    const double l1 = dot3(q01, q01), l2 = dot3(q02, q02), nn = dot3(nq, nq);
    if (!(nn > (0x1p-40 * l1) * l2)) return false;
    const double n1 = sqrt(l1), n3 = sqrt(nn);
    const double g1[3] = {q01[0] / n1, q01[1] / n1, q01[2] / n1}, g3[3] = {nq[0] / n3, nq[1] / n3, nq[2] / n3};
    double g2[3];
    cross3(g3, g1, g2);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) P[3 * r + c] = (g1[r] * S.e1[c] + g2[r] * S.e2[c]) + g3[r] * S.e3[c];
        P[9 + r] = Q0[r] - ((P[3 * r] * S.P0[0] + P[3 * r + 1] * S.P0[1]) + P[3 * r + 2] * S.P0[2]);
    }
    return true;
}

// sample j: up to four poses, slot r = the root's place among the ascending roots (an empty slot is all zeros, which no point passes);
// returns the number of poses, 0 = the sample is skipped
DEV int p_hypothesis(const int32_t* __restrict__ draws, int j, int m, const double* __restrict__ Xr, const float* __restrict__ xyr,
                     const PArgs& A, double (&PR)[4][12], bool (&live)[4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        live[r] = false;
#pragma unroll
        for (int k = 0; k < 12; k++) PR[r][k] = 0.0;
    }
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) idx[k] = (int)((unsigned)(draws[3 * (size_t)j + k] & 0x7fffffff) % (unsigned)m);
    if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) return 0;
    const PPt s0 = p_point(Xr, xyr, idx[0], A), s1 = p_point(Xr, xyr, idx[1], A), s2 = p_point(Xr, xyr, idx[2], A);
    PSample S;
    p_bearing(s0.x, s0.y, S.f0); p_bearing(s1.x, s1.y, S.f1); p_bearing(s2.x, s2.y, S.f2);
    const double p01[3] = {s1.X[0] - s0.X[0], s1.X[1] - s0.X[1], s1.X[2] - s0.X[2]};
    const double p02[3] = {s2.X[0] - s0.X[0], s2.X[1] - s0.X[1], s2.X[2] - s0.X[2]};
    const double p12[3] = {s2.X[0] - s1.X[0], s2.X[1] - s1.X[1], s2.X[2] - s1.X[2]};
    const double c2 = dot3(p01, p01), b2 = dot3(p02, p02), a2 = dot3(p12, p12);
    if (!(b2 != 0.0)) return 0;
    const double ca = dot3(S.f1, S.f2), cb = dot3(S.f0, S.f2), cg = dot3(S.f0, S.f1);
    const double p = (a2 - c2) / b2, q = (a2 + c2) / b2, ra = a2 / b2, rc = c2 / b2, rbc = (b2 - c2) / b2, rba = (b2 - a2) / b2;
    const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg, pm1 = p - 1.0, pp1 = 1.0 + p, omq = 1.0 - q, p2 = p * p;
    double c[5];
    c[4] = pm1 * pm1 - (4.0 * rc) * ca2;
    c[3] = 4.0 * (((p * (1.0 - p)) * cb - (omq * ca) * cg) + ((2.0 * rc) * ca2) * cb);
    c[2] = 2.0 * (((((p2 - 1.0) + (2.0 * p2) * cb2) + (2.0 * rbc) * ca2) - (((4.0 * q) * ca) * cb) * cg) + (2.0 * rba) * cg2);
    c[1] = 4.0 * ((((-p) * pp1) * cb + ((2.0 * ra) * cg2) * cb) - (omq * ca) * cg);
    c[0] = pp1 * pp1 - (4.0 * ra) * cg2;
    if (!(p_finite(c[0]) && p_finite(c[1]) && p_finite(c[2]) && p_finite(c[3]) && p_finite(c[4])) || !(c[4] != 0.0)) return 0;
    double nw[3];
    cross3(p01, p02, nw);
    const double nnw = dot3(nw, nw);
    if (!(nnw > (0x1p-40 * c2) * b2)) return 0;
    double B = fabs(c[0] / c[4]);
#pragma unroll
    for (int k = 1; k < 4; k++) { const double v = fabs(c[k] / c[4]); B = v > B ? v : B; }
    B = B + 1.0;
    if (!p_finite(B)) return 0;
    double roots[4];
    const int nr = p_quartic_roots(c, B, roots);
    const double lc = sqrt(c2), lw = sqrt(nnw);
#pragma unroll
    for (int k = 0; k < 3; k++) { S.P0[k] = s0.X[k]; S.e1[k] = p01[k] / lc; S.e3[k] = nw[k] / lw; }
    cross3(S.e3, S.e1, S.e2);
    S.b2 = b2; S.p = p; S.pm1 = pm1; S.ca = ca; S.cb = cb; S.cg = cg;
    int nsol = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r < nr) {
            live[r] = p_solution(S, roots[r], PR[r]);
            if (live[r]) nsol++;
            else {
#pragma unroll
                for (int k = 0; k < 12; k++) PR[r][k] = 0.0;
            }
        }
    }
    return nsol;
}

DEV void p_count_tile(const PPt* s_pt, int nt, const double (&PR)[4][12], int (&cnt)[4], double thr2) {
    for (int i = 0; i < nt; i++) {
        const PPt q = s_pt[i];
#pragma unroll
        for (int r = 0; r < 4; r++) cnt[r] += p_inlier(PR[r], q, thr2) ? 1 : 0;
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_pnp_batch(PArgs A, const double* __restrict__ X, const float* __restrict__ xy,
                                                  const int32_t* __restrict__ npts, const int32_t* __restrict__ draws,
                                                  uint8_t* __restrict__ mask, vis_pnp_result* __restrict__ out) {
    __shared__ PPt s_pt[P_TILE];
    __shared__ double s_bp[12][NT];                                // per lane, the pose behind its best key (registers are what bounds the occupancy)
    __shared__ int s_wt;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(npts[row], 0), A.in_stride);
    uint8_t* mrow = mask ? mask + (size_t)row * A.row_cap : nullptr;
    if (m < 4 || A.iters <= 0) {                                   // (uniform: the whole workgroup leaves)
        if (mrow) for (int i = tid; i < m; i += NT) mrow[i] = 0;
        if (tid < (int)(sizeof(vis_pnp_result) / 8)) {
            double* o = reinterpret_cast<double*>(out + row);
            o[tid] = 0.0;
        }
        __syncthreads();
        if (tid == 0) out[row].best_iter = -1;
        return;
    }
    const double* Xr = X + (size_t)row * A.in_stride * A.x_stride;
    const float* xyr = xy + (size_t)row * A.in_stride * 2;
    const auto fill = [&](int i) { return p_point(Xr, xyr, i, A); };
    const bool single = rl_first_tile<P_TILE, NT>(s_pt, m, fill);
    unsigned long long best = 0;                                   // 0: no pose with a count > 0 yet
    int ndeg = 0, nsol = 0;
    for (int j0 = 0; j0 < A.iters; j0 += NT) {
        double PR[4][12]; bool live[4]; int cnt[4] = {0, 0, 0, 0};
        const int j = j0 + tid;
        if (j < A.iters) {
            const int ns = p_hypothesis(draws, j, m, Xr, xyr, A, PR, live);
            nsol += ns;
            if (ns == 0) ndeg++;
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                live[r] = false;
#pragma unroll
                for (int k = 0; k < 12; k++) PR[r][k] = 0.0;
            }
        }
        rl_walk_tiles<P_TILE, NT>(s_pt, m, single, rl_wave_live(j0, A.iters), fill,
                                  [&](const PPt* tile, int nt) { p_count_tile(tile, nt, PR, cnt, A.thr2); });
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (rl_offer(best, live[r], cnt[r], 4 * j + r)) {
#pragma unroll
                for (int k = 0; k < 12; k++) s_bp[k][tid] = PR[r][k];
            }
        }
    }
    const unsigned long long mine = best;
    int sums[2] = {ndeg, nsol};
    rl_block_reduce<NT>(best, sums);
    const bool won = best != 0;
    if (won && mine == best) s_wt = tid;                           // one lane: a key names its slot
    __syncthreads();
    if (tid >= 64) return;
    // ---- the first wave: mask and count under the winner over the points in strides of 64
    double Pw[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Pw[k] = won ? s_bp[k][s_wt] : 0.0;
    int it = -1, root = 0;
    if (won) {
        const int h = rl_key_slot(best);
        it = h >> 2; root = h & 3;
    }
    int nin = 0;
    for (int i = tid; i < m; i += 64) {
        const bool in = won && p_inlier(Pw, p_point(Xr, xyr, i, A), A.thr2);
        nin += in ? 1 : 0;
        if (mrow) mrow[i] = in ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) nin += __shfl_xor(nin, off);
    if (tid != 0) return;
    vis_pnp_result r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.R[k] = r.R_ransac[k] = Pw[k];
#pragma unroll
    for (int k = 0; k < 3; k++) r.t[k] = r.t_ransac[k] = Pw[9 + k];
    r.cost0 = r.cost1 = 0.0;
    r.n_inliers = nin; r.n_points = m; r.best_iter = it; r.best_root = root; r.n_degenerate = sums[0]; r.n_solutions = sums[1];
    r.n_inliers_refined = nin;
    r.flags = won && nin < A.min_inliers ? VIS_PNP_FEW : 0;
    out[row] = r;
}

// ---- the refinement

// one pass over the points at pose P: S[0..20] = the upper triangle of sum J^T J in row order, S[21..26] = sum J^T r, S[27] = sum |r|^2, over the
// inliers of the winner P0; returns the number of points that pass the per-point test under P
DEV int p_pass(const double (&P0)[12], const double (&P)[12], const double* __restrict__ Xr, const float* __restrict__ xyr, int m, int lane,
               const PArgs& A, double (&S)[28]) {
#pragma unroll
    for (int k = 0; k < 28; k++) S[k] = 0.0;
    int n = 0;
    for (int i = lane; i < m; i += 64) {
        const PPt q = p_point(Xr, xyr, i, A);
        const bool in = p_inlier(P0, q, A.thr2);
        n += p_inlier(P, q, A.thr2) ? 1 : 0;
        double U, V, W;
        p_transform(P, q.X, U, V, W);
        const double iw = 1.0 / W, un = U / W, vn = V / W;
        const double rx = un - q.x, ry = vn - q.y;
        const double j02 = -(un * iw), j12 = -(vn * iw);
        const double J0[6] = {j02 * V, iw * W - j02 * U, -(iw * V), iw, 0.0, j02};
        const double J1[6] = {j12 * V - iw * W, -(j12 * U), iw * U, 0.0, iw, j12};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++, k++) { const double v = J0[a] * J0[b] + J1[a] * J1[b]; S[k] = S[k] + (in ? v : 0.0); }
#pragma unroll
        for (int a = 0; a < 6; a++) { const double v = J0[a] * rx + J1[a] * ry; S[21 + a] = S[21 + a] + (in ? v : 0.0); }
        const double e = rx * rx + ry * ry;
        S[27] = S[27] + (in ? e : 0.0);
    }
#pragma unroll
    for (int k = 0; k < 28; k++) S[k] = wave_sum(S[k]);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    return n;
}

// d = -(sum J^T J)^-1 sum J^T r by LDL^T without pivoting; false: a pivot that is <= 0 or not finite
DEV bool p_solve6(const double (&S)[28], double (&d)[6]) {
    double Am[6][6], L[6][6], D[6], z[6];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++, k++) Am[a][b] = Am[b][a] = S[k];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = Am[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (L[j][c] * L[j][c]) * D[c];
        D[j] = s;
        ok = ok && s > 0.0 && p_finite(s);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = Am[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) v = v - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = v / s;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = -S[21 + i];
#pragma unroll
        for (int c = 0; c < i; c++) v = v - L[i][c] * z[c];
        z[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = z[i] / D[i];
#pragma unroll
        for (int c = i + 1; c < 6; c++) v = v - L[c][i] * d[c];
        d[i] = v;
    }
    return ok;
}

// R <- C(w) R, t <- C(w) t + dt with the Cayley map C = I + 2 / (1 + |h|^2) ([h]x + [h]x^2), h = w / 2
DEV void p_update(double (&P)[12], const double (&d)[6]) {
    const double h[3] = {0.5 * d[0], 0.5 * d[1], 0.5 * d[2]};
    const double hh = dot3(h, h), s = 2.0 / (1.0 + hh);
    const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
    double Cm[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double k2 = i == j ? h[i] * h[j] - hh : h[i] * h[j];
            Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + s * (K[3 * i + j] + k2);
        }
    double N[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) N[3 * i + j] = (Cm[3 * i] * P[j] + Cm[3 * i + 1] * P[3 + j]) + Cm[3 * i + 2] * P[6 + j];
        N[9 + i] = ((Cm[3 * i] * P[9] + Cm[3 * i + 1] * P[10]) + Cm[3 * i + 2] * P[11]) + d[3 + i];
    }
#pragma unroll
    for (int k = 0; k < 12; k++) P[k] = N[k];
}

__global__ __launch_bounds__(64) void k_pnp_refine(PArgs A, const double* __restrict__ X, const float* __restrict__ xy,
                                                   const int32_t* __restrict__ npts, vis_pnp_result* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    vis_pnp_result* o = out + row;
    if (o->best_iter < 0) return;                                  // (uniform) the zero record, or no winner
    const int m = min(max(npts[row], 0), A.in_stride);
    const double* Xr = X + (size_t)row * A.in_stride * A.x_stride;
    const float* xyr = xy + (size_t)row * A.in_stride * 2;
    double P0[12], P[12], S[28];
#pragma unroll
    for (int k = 0; k < 9; k++) P0[k] = P[k] = o->R_ransac[k];
#pragma unroll
    for (int k = 0; k < 3; k++) P0[9 + k] = P[9 + k] = o->t_ransac[k];
    const int nin = o->n_inliers;
    (void)p_pass(P0, P, Xr, xyr, m, lane, A, S);
    const double cost0 = S[27];
    double cost1 = cost0;
    int flags = o->flags, nref = nin;
    bool refined = false;
    if (A.refine_iters > 0 && nin >= A.min_inliers) {
        bool ok = true;
        for (int step = 0; step < A.refine_iters; step++) {
            if (step > 0) (void)p_pass(P0, P, Xr, xyr, m, lane, A, S);
            double d[6];
            ok = p_solve6(S, d);
            if (!ok) break;                                        // (uniform: every lane holds the same sums)
            p_update(P, d);
        }
        const int n1 = p_pass(P0, P, Xr, xyr, m, lane, A, S);
        cost1 = S[27];
        refined = ok && p_finite(cost1) && cost1 <= cost0;
        flags |= refined ? VIS_PNP_REFINED : VIS_PNP_REFINE_REJECTED;
        if (refined) nref = n1;
    }
    if (lane != 0) return;
    o->cost0 = cost0; o->cost1 = cost1; o->flags = flags; o->n_inliers_refined = nref;
    if (refined) {
#pragma unroll
        for (int k = 0; k < 9; k++) o->R[k] = P[k];
#pragma unroll
        for (int k = 0; k < 3; k++) o->t[k] = P[9 + k];
    }
}

// ---- the rows of vis_batch_pnp: frame i's correspondences joined to the map points of its keyframe's own pair
struct LArgs {
    int n, pair0_valid, mcap, mstride, row_cap, require, kcap;
};
DEV int p_keyframe(const int32_t* __restrict__ links, int i, int pair0_valid) {
    return links ? links[i] : (i > 0 ? i - 1 : (pair0_valid ? VIS_KF_CARRIED : VIS_KF_FIRST));
}
DEV bool p_has_pose(const PoseOut* o) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; k++) any = any || o->R[k] != 0.0;
    return any;
}

// One workgroup per frame i.  q = i's keyframe, p = q's.  table[kp] = the first correspondence k of pair (p -> q) whose keypoint in frame q is kp
// and whose flags contain `require` (an integer minimum: order independent, like the vote counters of k_hpose_vote); then the correspondences c of
// pair (q -> i) whose keypoint in q has an entry are appended in rising c: X from row q of the caller's map points, the pixel from frame i.
template <int NT>
__global__ __launch_bounds__(NT) void k_pnp_link(LArgs A, const int32_t* __restrict__ links, const vis_dmatch* __restrict__ matches,
                                                 const int32_t* __restrict__ npts, const float* __restrict__ p2, const PoseOut* __restrict__ pose,
                                                 const vis_map_point* __restrict__ points, const uint8_t* __restrict__ flags,
                                                 int32_t* __restrict__ table, double* __restrict__ Xout, float* __restrict__ xyout,
                                                 int32_t* __restrict__ nout, vis_pnp_link* __restrict__ link) {
    __shared__ int s_wave[NT / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int q = p_keyframe(links, i, A.pair0_valid);
    const int p = q >= 0 && q < A.n ? p_keyframe(links, q, A.pair0_valid) : q;
    const bool usable = q >= 0 && q < A.n && p_has_pose(pose + q);     // (uniform)
    int total = 0;
    if (usable) {
        int32_t* tab = table + (size_t)i * A.kcap;
        for (int k = tid; k < A.kcap; k += NT) tab[k] = 0x7fffffff;
        __syncthreads();
        const int mq = min(max(npts[q], 0), A.mcap), mi = min(max(npts[i], 0), A.mcap);
        const vis_dmatch* Mq = matches + (size_t)q * A.mstride;
        const vis_dmatch* Mi = matches + (size_t)i * A.mstride;
        for (int k = tid; k < mq; k += NT) {
            const int kp = Mq[k].trainIdx;
            if (kp >= 0 && kp < A.kcap && (flags[(size_t)q * A.row_cap + k] & A.require) == A.require) atomicMin(&tab[kp], k);
        }
        __syncthreads();
        for (int c0 = 0; c0 < mi; c0 += NT) {                          // rising c: a workgroup-wide exclusive count per chunk
            const int c = c0 + tid;
            int k = 0x7fffffff;
            if (c < mi) { const int kp = Mi[c].queryIdx; if (kp >= 0 && kp < A.kcap) k = tab[kp]; }
            const bool hit = k != 0x7fffffff;
            const unsigned long long b = __ballot(hit);
            const int before = __popcll(b & ((1ull << (tid & 63)) - 1ull));
            if ((tid & 63) == 0) s_wave[tid >> 6] = __popcll(b);
            __syncthreads();
            int base = total, all = 0;
            for (int w = 0; w < NT / 64; w++) { if (w < (tid >> 6)) base += s_wave[w]; all += s_wave[w]; }
            if (hit) {
                const size_t o = (size_t)i * A.mcap + base + before;
                const vis_map_point* mp = points + (size_t)q * A.row_cap + k;
                Xout[3 * o] = mp->X[0]; Xout[3 * o + 1] = mp->X[1]; Xout[3 * o + 2] = mp->X[2];
                xyout[2 * o] = p2[2 * ((size_t)i * A.mcap + c)]; xyout[2 * o + 1] = p2[2 * ((size_t)i * A.mcap + c) + 1];
            }
            total += all;
            __syncthreads();                                           // s_wave is rewritten by the next chunk
        }
    }
    if (tid < (int)(sizeof(vis_pnp_link) / 8)) reinterpret_cast<double*>(link + i)[tid] = 0.0;
    __syncthreads();
    if (tid != 0) return;
    nout[i] = total;
    link[i].n_linked = total; link[i].q = q; link[i].p = p; link[i].flags = q == VIS_KF_CARRIED ? VIS_PNPL_NO_MAP : 0;
}

// the relative motion q -> i of every frame with a result: R_rel = R R_pq^T, t_rel = t - R_rel t_pq, scale = |t_rel|
__global__ void k_pnp_rel(int n, const vis_pnp_result* __restrict__ rec, const PoseOut* __restrict__ pose, vis_pnp_link* __restrict__ link) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = link[i].q;
    if (rec[i].best_iter < 0 || q < 0 || q >= n) return;
    const double* R = rec[i].R; const double* t = rec[i].t;
    const double* Rq = pose[q].R; const double* tq = pose[q].t;
    double Rr[9], tr[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rr[3 * r + c] = (R[3 * r] * Rq[3 * c] + R[3 * r + 1] * Rq[3 * c + 1]) + R[3 * r + 2] * Rq[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) tr[r] = t[r] - ((Rr[3 * r] * tq[0] + Rr[3 * r + 1] * tq[1]) + Rr[3 * r + 2] * tq[2]);
#pragma unroll
    for (int k = 0; k < 9; k++) link[i].R_rel[k] = Rr[k];
#pragma unroll
    for (int k = 0; k < 3; k++) link[i].t_rel[k] = tr[k];
    link[i].scale = sqrt(dot3(tr, tr));
}

// vis_batch_pnp's body on ctx->stream: links (null: gate off), the pose stage's match list (mstride entries per pair) and counts, its p2 rows, the
// caller's map points / flags (rows of row_cap), the plan's workspace (table: n x kcap; X: n x mcap x 3; xy: n x mcap x 2; cnt: n)
int pnp_link_run(vis_ctx* ctx, const vis_pnp_params* pp, int n, const int32_t* d_links, int pair0_valid, int mcap, int mstride, int kcap,
                 const vis_dmatch* d_matches, const int32_t* d_npts, const float* d_p2, const PoseOut* d_pose, const vis_map_point* d_points,
                 const uint8_t* d_flags, int row_cap, int require, int32_t* d_table, double* d_X, float* d_xy, int32_t* d_cnt,
                 const int32_t* d_draws, int mask_cap, uint8_t* d_mask, vis_pnp_result* d_out, vis_pnp_link* d_link) {
    if (n <= 0) return VIS_OK;
    LArgs A;
    A.n = n; A.pair0_valid = pair0_valid; A.mcap = mcap; A.mstride = mstride; A.row_cap = row_cap; A.require = require; A.kcap = kcap;
    hipLaunchKernelGGL((k_pnp_link<256>), dim3(n), dim3(256), 0, ctx->stream, A, d_links, d_matches, d_npts, d_p2, d_pose, d_points, d_flags,
                       d_table, d_X, d_xy, d_cnt, d_link);
    HIPCHK(ctx, hipGetLastError());
    const int rc = pnp_batch_run(ctx, pp, n, mcap, d_X, 3, d_xy, d_cnt, d_draws, mask_cap, d_mask, d_out);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pnp_rel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, n, d_out, d_pose, d_link);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

// pp has been validated by the entry point.  d_X: n rows of in_stride points, x_stride doubles apart; d_xy: n rows of in_stride (x, y) pixels;
// d_npts of them valid (clamped); d_mask: rows of row_cap >= in_stride bytes, or null; d_draws: iters x 3.  On ctx->stream.
int pnp_batch_run(vis_ctx* ctx, const vis_pnp_params* pp, int n, int in_stride, const double* d_X, int x_stride, const float* d_xy,
                  const int32_t* d_npts, const int32_t* d_draws, int row_cap, uint8_t* d_mask, vis_pnp_result* d_out) {
    if (n <= 0) return VIS_OK;
    PArgs A;
    A.cx = ctx->p.cx; A.cy = ctx->p.cy; A.fx_inv = 1. / ctx->p.fx;
    const double s = pp->threshold_px * A.fx_inv;
    A.thr2 = s * s;
    A.iters = pp->iters; A.min_inliers = pp->min_inliers; A.refine_iters = pp->refine_iters;
    A.in_stride = in_stride; A.x_stride = x_stride; A.row_cap = row_cap;
    hipLaunchKernelGGL((k_pnp_batch<256>), dim3(n), dim3(256), 0, ctx->stream, A, d_X, d_xy, d_npts, d_draws, d_mask, d_out);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pnp_refine, dim3(n), dim3(64), 0, ctx->stream, A, d_X, d_xy, d_npts, d_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
