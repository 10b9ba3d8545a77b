// ftri_core.h -- the N-view triangulation of one track as device functions: the walk along prev_kp / prev[], the used views, the cost pass and
// steps 1-3 of vis_ftrack_triangulate_rows (include/vislam_hip.h has the contract, tests/ftrack_ref.py restates it).  One text for k_ftri_points
// (ftrack.hip) and for the initial points of the windowed bundle adjustment (ba.hip), so both round the same way.  `lo` is the oldest frame a walk
// may enter: 0 for the triangulation of a call (the compare folds into the existing p < 0), a window's anchor for the adjustment.
#pragma once
#include "vis_internal.h"
#include "jacobi_eig.h"

__device__ __forceinline__ int ft_prev(const FtFrames& fr, int i) {
    return fr.prev ? fr.prev[i] : (i > 0 ? i - 1 : (fr.pair0 ? VIS_KF_CARRIED : VIS_KF_FIRST));
}
// nk(i): the keypoints frame i takes part with
__device__ __forceinline__ int ft_count(const FtFrames& fr, int i, int R) {
    return ft_prev(fr, i) == VIS_KF_NOT_SAVED ? 0 : min(max(fr.nkp[i], 0), R);
}

struct FtriArgs {
    int n, R, ocap; FtFrames fr; const vis_ftrack_obs* obs; const char* xy; size_t xy_row; int xy_step; const double* poses;
    int max_views, min_views, gn_iters; double thr2, max_cos, fx, fy, cx, cy;
};

// the parent keypoint of (i, k) inside this call and not older than frame lo: its frame, or -1
__device__ __forceinline__ int ftri_parent(const FtriArgs& a, int lo, int i, int k, int* pk) {
    const int p = ft_prev(a.fr, i);
    if (p < lo || p >= i) return -1;
    const int q = a.obs[(size_t)i * a.ocap + k].prev_kp;
    if ((uint32_t)q >= (uint32_t)ft_count(a.fr, p, a.R)) return -1;
    *pk = q;
    return p;
}

__device__ __forceinline__ bool ftri_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf

// A view of the walk: the pose of its frame and its pixel; false when the frame has no pose or the pixel is not finite
__device__ __forceinline__ bool ftri_view(const FtriArgs& a, int i, int k, double* P, double* u, double* v) {
    const double* p = a.poses + (size_t)i * 12;
    bool fin = true, zero = true;
#pragma unroll
    for (int j = 0; j < 12; j++) { P[j] = p[j]; fin = fin && ftri_finite(P[j]); if (j < 9) zero = zero && P[j] == 0.0; }
    const float* px = reinterpret_cast<const float*>(a.xy + (size_t)i * a.xy_row + (size_t)k * a.xy_step);   // (a keypoint record is 4-byte aligned)
    *u = (double)px[0]; *v = (double)px[1];
    return fin && !zero && ftri_finite(*u) && ftri_finite(*v);
}

struct FtriPass { double H00, H01, H02, H11, H12, H22, g0, g1, g2, cost, c_new[3], c_old[3]; bool front, reproj; int views; };

// cost, normal equations, flags and the end cameras' centres of X over the used views, newest to oldest
__device__ __forceinline__ void ftri_pass(const FtriArgs& a, int lo, int i0, int k0, const double* X, FtriPass& r) {
    r.H00 = r.H01 = r.H02 = r.H11 = r.H12 = r.H22 = r.g0 = r.g1 = r.g2 = r.cost = 0.0;
    r.front = r.reproj = true; r.views = 0;
    int i = i0, k = k0;
    for (int w = 0; w < a.max_views; w++) {
        double P[12], u, v;
        if (ftri_view(a, i, k, P, &u, &v)) {
            const double U = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[9];
            const double V = ((P[3] * X[0] + P[4] * X[1]) + P[5] * X[2]) + P[10];
            const double Wd = ((P[6] * X[0] + P[7] * X[1]) + P[8] * X[2]) + P[11];
            const double iw = 1.0 / Wd, un = U * iw, vn = V * iw;
            const double ru = (a.fx * un + a.cx) - u, rv = (a.fy * vn + a.cy) - v;
            const double fu = a.fx * iw, fv = a.fy * iw;
            const double ju0 = fu * (P[0] - un * P[6]), ju1 = fu * (P[1] - un * P[7]), ju2 = fu * (P[2] - un * P[8]);
            const double jv0 = fv * (P[3] - vn * P[6]), jv1 = fv * (P[4] - vn * P[7]), jv2 = fv * (P[5] - vn * P[8]);
            r.H00 += ju0 * ju0 + jv0 * jv0; r.H01 += ju0 * ju1 + jv0 * jv1; r.H02 += ju0 * ju2 + jv0 * jv2;
            r.H11 += ju1 * ju1 + jv1 * jv1; r.H12 += ju1 * ju2 + jv1 * jv2; r.H22 += ju2 * ju2 + jv2 * jv2;
            r.g0 += ju0 * ru + jv0 * rv; r.g1 += ju1 * ru + jv1 * rv; r.g2 += ju2 * ru + jv2 * rv;
            const double e2 = ru * ru + rv * rv;
            r.cost += e2;
            r.front = r.front && Wd > 0.0;
            r.reproj = r.reproj && e2 <= a.thr2;
            // the centre -R^T t, each row ((R_0j t_0 + R_1j t_1) + R_2j t_2) negated
            const double c0 = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]), c1 = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]),
                         c2 = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]);
            if (r.views == 0) { r.c_new[0] = c0; r.c_new[1] = c1; r.c_new[2] = c2; }
            r.c_old[0] = c0; r.c_old[1] = c1; r.c_old[2] = c2;
            r.views++;
        }
        int pk;
        const int p = ftri_parent(a, lo, i, k, &pk);
        if (p < 0) break;
        i = p; k = pk;
    }
}

// steps 1-4 for the track that ends in (i0, k0); pt arrives as the zero record
__device__ __forceinline__ void ftri_point(const FtriArgs& a, int lo, int i0, int k0, vis_ftrack_point& pt) {
    // (1) DLT over the used views, newest to oldest
    double A00 = 0, A01 = 0, A02 = 0, A03 = 0, A11 = 0, A12 = 0, A13 = 0, A22 = 0, A23 = 0, A33 = 0;
    int views = 0, i = i0, k = k0;
    for (int w = 0; w < a.max_views; w++) {
        double P[12], u, v;
        if (ftri_view(a, i, k, P, &u, &v)) {
            const double x = (u - a.cx) / a.fx, y = (v - a.cy) / a.fy;
            const double r0 = x * P[6] - P[0], r1 = x * P[7] - P[1], r2 = x * P[8] - P[2], r3 = x * P[11] - P[9];
            const double s0 = y * P[6] - P[3], s1 = y * P[7] - P[4], s2 = y * P[8] - P[5], s3 = y * P[11] - P[10];
            A00 += r0 * r0 + s0 * s0; A01 += r0 * r1 + s0 * s1; A02 += r0 * r2 + s0 * s2; A03 += r0 * r3 + s0 * s3;
            A11 += r1 * r1 + s1 * s1; A12 += r1 * r2 + s1 * s2; A13 += r1 * r3 + s1 * s3;
            A22 += r2 * r2 + s2 * s2; A23 += r2 * r3 + s2 * s3; A33 += r3 * r3 + s3 * s3;
            views++;
        }
        int pk;
        const int p = ftri_parent(a, lo, i, k, &pk);
        if (p < 0) break;
        i = p; k = pk;
    }
    pt.n_views = views;
    if (views < a.min_views) { pt.flags = VIS_FTP_FEW; return; }
    double M[16] = {A00, A01, A02, A03, A01, A11, A12, A13, A02, A12, A22, A23, A03, A13, A23, A33}, V[16];
    jacobi_eig<4>(M, V);
    int mn = 0; double dmin = M[0];
#pragma unroll
    for (int j = 1; j < 4; j++) if (M[5 * j] < dmin) { dmin = M[5 * j]; mn = j; }
    double E[4];
#pragma unroll
    for (int j = 0; j < 4; j++) E[j] = mn == 0 ? V[4 * j] : mn == 1 ? V[4 * j + 1] : mn == 2 ? V[4 * j + 2] : V[4 * j + 3];
    double X[3] = {E[0] / E[3], E[1] / E[3], E[2] / E[3]};
    if (E[3] == 0.0 || !ftri_finite(X[0]) || !ftri_finite(X[1]) || !ftri_finite(X[2])) { pt.flags = VIS_FTP_SINGULAR; return; }
    // (3) Gauss-Newton: every iterate costed, the first of least cost kept with what its pass found
    FtriPass r, best;
    ftri_pass(a, lo, i0, k0, X, r);
    best = r;
    if (!ftri_finite(r.cost)) { pt.flags = VIS_FTP_SINGULAR; return; }  // (a point in a camera's plane, an overflow: nothing to refine or report)
    double B[3] = {X[0], X[1], X[2]};
    for (int it = 0; it < a.gn_iters; it++) {
        const double D0 = r.H00;
        if (!(D0 > 0.0) || !ftri_finite(D0)) break;
        const double L10 = r.H01 / D0, L20 = r.H02 / D0;
        const double D1 = r.H11 - (L10 * L10) * D0;
        if (!(D1 > 0.0) || !ftri_finite(D1)) break;
        const double L21 = (r.H12 - (L20 * L10) * D0) / D1;
        const double D2 = (r.H22 - (L20 * L20) * D0) - (L21 * L21) * D1;
        if (!(D2 > 0.0) || !ftri_finite(D2)) break;
        const double z0 = -r.g0, z1 = -r.g1 - L10 * z0, z2 = (-r.g2 - L20 * z0) - L21 * z1;
        const double d2 = z2 / D2, d1 = z1 / D1 - L21 * d2, d0 = (z0 / D0 - L10 * d1) - L20 * d2;
        X[0] = X[0] + d0; X[1] = X[1] + d1; X[2] = X[2] + d2;
        ftri_pass(a, lo, i0, k0, X, r);
        if (r.cost < best.cost) { best = r; B[0] = X[0]; B[1] = X[1]; B[2] = X[2]; }
    }
    const double a0 = best.c_new[0] - B[0], a1 = best.c_new[1] - B[1], a2 = best.c_new[2] - B[2];
    const double b0 = best.c_old[0] - B[0], b1 = best.c_old[1] - B[1], b2 = best.c_old[2] - B[2];
    const double dab = (a0 * b0 + a1 * b1) + a2 * b2, daa = (a0 * a0 + a1 * a1) + a2 * a2, dbb = (b0 * b0 + b1 * b1) + b2 * b2;
    double cs = dab / sqrt(daa * dbb);
    const bool cs_ok = ftri_finite(cs);
    if (!cs_ok) cs = 1.0;
    pt.X[0] = B[0]; pt.X[1] = B[1]; pt.X[2] = B[2];
    pt.rms_reproj_px = (float)sqrt(best.cost / (double)views);
    pt.parallax_cos = (float)cs;
    int f = (best.front ? VIS_FTP_FRONT : 0) | (best.reproj ? VIS_FTP_REPROJ_OK : 0) | (cs_ok && cs <= a.max_cos ? VIS_FTP_PARALLAX_OK : 0);
    if (f == (VIS_FTP_FRONT | VIS_FTP_REPROJ_OK | VIS_FTP_PARALLAX_OK)) f |= VIS_FTP_KEPT;
    pt.flags = f;
}
