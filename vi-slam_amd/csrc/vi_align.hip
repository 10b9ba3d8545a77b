// vi_align.hip -- visual-inertial alignment on the device: the gyro bias, gravity in the root's frame, the metric scale and a velocity per frame from
// the trajectory records and the IMU pair deltas.  include/vislam_hip.h has the contract operation for operation, tests/vi_align_ref.py restates it.
// k_via_align is ONE launch of one workgroup of 256 threads; thread tid owns the frames tid, tid + 256, tid + 512, tid + 768.  A frame's tail (camera
// centre, IMU-to-root rotation, lever term) is recomputed from the trajectory record wherever it is needed -- its own, its parent's, its grandparent's
// -- so nothing is staged and there is no workspace.  Sums under contract T (ep_sums.h), the small solves on every thread with the same bits.
#include "vis_internal.h"
#include "ransac_lanes.h"
#include "ep_sums.h"
#include <cmath>

#define VIA_BLOCK 256

struct ViaTail { double C[3], Rw[9], L[3]; int seg, epoch, flags; };

DEV bool via_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf
DEV double via_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
DEV int via_prev(const FtFrames& fr, int i) {
    const int p = fr.prev ? fr.prev[i] : (i > 0 ? i - 1 : (fr.pair0 ? VIS_KF_CARRIED : VIS_KF_FIRST));
    if (p >= 0) return p < i ? p : VIS_KF_FIRST;
    return p == VIS_KF_CARRIED || p == VIS_KF_NOT_SAVED ? p : VIS_KF_FIRST;
}
DEV void via_mul(const double* A, const double* B, double* M) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
DEV void via_tmul(const double* A, const double* B, double* M) {       // A^T B
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
DEV void via_mulv(const double* A, const double* x, double* y) {
#pragma unroll
    for (int r = 0; r < 3; r++) y[r] = (A[3 * r] * x[0] + A[3 * r + 1] * x[1]) + A[3 * r + 2] * x[2];
}
DEV void via_tmulv(const double* A, const double* x, double* y) {      // A^T x
#pragma unroll
    for (int r = 0; r < 3; r++) y[r] = (A[r] * x[0] + A[3 + r] * x[1]) + A[6 + r] * x[2];
}
DEV void via_zero_tail(ViaTail& o) {
#pragma unroll
    for (int k = 0; k < 9; k++) o.Rw[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) o.C[k] = o.L[k] = 0.0;
    o.seg = o.epoch = o.flags = 0;
}
// the tail of trajectory record T of a frame whose normalised pair is q
DEV void via_tail(const vis_vi_align_params& P, const vis_traj_pose* __restrict__ T, int q, ViaTail& o) {
    via_zero_tail(o);
    const int tf = T->flags;
    if (tf & (VIS_TJ_NOT_SAVED | VIS_TJ_OVERFLOW)) return;
    double R[9], t[3], M[9], Rt[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = T->R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = T->t[k];
    via_tmulv(R, t, Rt);
    via_mul(P.r_ic, R, M);
    ViaTail w;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        w.C[r] = -Rt[r];
#pragma unroll
        for (int c = 0; c < 3; c++) w.Rw[3 * r + c] = M[3 * c + r];
    }
    via_tmulv(R, P.p_ci, w.L);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && via_finite(w.Rw[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && via_finite(w.C[k]) && via_finite(w.L[k]);
    if (!fin) return;
    w.seg = T->segment_seq; w.epoch = T->epoch_seq; w.flags = VIS_VIT_POSED;
    if (!(tf & VIS_TJ_ROOT) && T->parent == q && (q >= 0 || q == VIS_KF_CARRIED)) w.flags |= VIS_VIT_EDGE;
    o = w;
}
DEV void via_tail_load(const vis_vi_tail* __restrict__ r, ViaTail& o) {
#pragma unroll
    for (int k = 0; k < 9; k++) o.Rw[k] = r->Rw[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { o.C[k] = r->C[k]; o.L[k] = r->L[k]; }
    o.seg = r->segment_seq; o.epoch = r->epoch_seq; o.flags = r->flags;
}
DEV void via_tail_store(const ViaTail& t, int flags, vis_vi_tail& o) {
#pragma unroll
    for (int k = 0; k < 9; k++) o.Rw[k] = t.Rw[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { o.C[k] = t.C[k]; o.L[k] = t.L[k]; }
    o.segment_seq = t.seg; o.epoch_seq = t.epoch; o.flags = flags; o.reserved_ = 0;
}
DEV bool via_delta_numbers_finite(const vis_imu_delta* __restrict__ D) {
    bool fin = via_finite(D->dt);
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && via_finite(D->R[k]) && via_finite(D->JRg[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && via_finite(D->v[k]) && via_finite(D->p[k]);
    return fin;
}
DEV bool via_usable(const vis_vi_align_params& P, const vis_imu_delta* __restrict__ D, int parent) {
    if (D->flags & (VIS_IMU_NO_PAIR | VIS_IMU_NO_CARRY | VIS_IMU_NO_START | VIS_IMU_NONFINITE | P.reject)) return false;
    if (!via_delta_numbers_finite(D)) return false;
    return D->dt > 0.0 && D->q == parent;
}

// LDL^T without pivoting, er_solve5's order; b is added, not subtracted.  false: a pivot that is not finite and > 0, or an x that is not finite
template <int N>
DEV bool via_ldl(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
    double L[N][N], D[N], z[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = A[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (L[j][c] * L[j][c]) * D[c];
        D[j] = s;
        ok = ok && s > 0.0 && via_finite(s);
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = A[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) v = v - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = v / s;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double v = b[i];
#pragma unroll
        for (int c = 0; c < i; c++) v = v - L[i][c] * z[c];
        z[i] = v;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double v = z[i] / D[i];
#pragma unroll
        for (int c = i + 1; c < N; c++) v = v - L[c][i] * x[c];
        x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < N; i++) ok = ok && via_finite(x[i]);
    return ok;
}

DEV void via_rot_error(const double* dR, const double* V, double* e) {
    double Er[9];
    via_tmul(dR, V, Er);
    e[0] = 0.5 * (Er[7] - Er[5]); e[1] = 0.5 * (Er[2] - Er[6]); e[2] = 0.5 * (Er[3] - Er[1]);
}
DEV double via_horner(const double* c, double x) {
    double acc = c[VIS_IMU_EXP_TERMS - 1];
#pragma unroll
    for (int k = VIS_IMU_EXP_TERMS - 2; k >= 0; k--) acc = c[k] + x * acc;
    return acc;
}
DEV void via_exp(const double* phi, double* dR) {
    constexpr double cA[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_A, cB[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_B;
    const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2], xy = phi[0] * phi[1], xz = phi[0] * phi[2], yz = phi[1] * phi[2];
    const double th2 = (xx + yy) + zz;
    const double A = via_horner(cA, th2), B = via_horner(cB, th2);
    dR[0] = 1.0 - B * (yy + zz); dR[1] = B * xy - A * phi[2]; dR[2] = B * xz + A * phi[1];
    dR[3] = B * xy + A * phi[2]; dR[4] = 1.0 - B * (xx + zz); dR[5] = B * yz - A * phi[0];
    dR[6] = B * xz - A * phi[1]; dR[7] = B * yz + A * phi[0]; dR[8] = 1.0 - B * (xx + yy);
}
DEV double via_normalise(const double* v, double* u) {
    const double n = sqrt(via_dot(v, v));
#pragma unroll
    for (int k = 0; k < 3; k++) u[k] = v[k] / n;
    return n;
}

// what a frame's terms are built from: its own tail, its parent's and grandparent's, and the two deltas' numbers
struct ViaFrame {
    ViaTail c, b, a;
    double dt1, dt2, dv1[3], dp1[3], dp2[3], dv2[3];       // 1: the parent's delta (a -> b); 2: the frame's own (b -> c)
    int q;
    bool use_c, use_b;
};
struct ViaCarryIn { const vis_vi_carry* rec; };            // null: none that counts
template <bool BA> struct ViaBaArgs {};                                           // k_via_align<true>'s own arguments; none for <false>
template <> struct ViaBaArgs<true> { vis_vi_align_ba_params bp; const vis_imu_bias_jac* jac; };

DEV void via_gather(const vis_vi_align_params& P, const FtFrames& fr, const vis_traj_pose* __restrict__ traj, const vis_imu_delta* __restrict__ delta,
                    const vis_vi_carry* __restrict__ carry, int i, ViaFrame& F) {
    const int q = via_prev(fr, i);
    F.q = q;
    via_tail(P, traj + i, q, F.c);
    F.use_c = via_usable(P, delta + i, traj[i].parent);
    F.dt2 = delta[i].dt;
#pragma unroll
    for (int k = 0; k < 3; k++) { F.dp2[k] = delta[i].p[k]; F.dv2[k] = delta[i].v[k]; }
    via_zero_tail(F.b); via_zero_tail(F.a);
    F.use_b = false; F.dt1 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) F.dv1[k] = F.dp1[k] = 0.0;
    const vis_imu_delta* db = nullptr;
    if (q >= 0) {
        const int qq = via_prev(fr, q);
        via_tail(P, traj + q, qq, F.b);
        F.use_b = via_usable(P, delta + q, traj[q].parent);
        db = delta + q;
        if (qq >= 0) via_tail(P, traj + qq, via_prev(fr, qq), F.a);
        else if (qq == VIS_KF_CARRIED && carry) { via_tail_load(&carry->last, F.a); }
    } else if (q == VIS_KF_CARRIED && carry) {
        via_tail_load(&carry->last, F.b);
        via_tail_load(&carry->parent, F.a);
        F.use_b = (F.b.flags & VIS_VIT_DELTA) != 0;
        db = &carry->last_delta;
    }
    if (db) {
        F.dt1 = db->dt;
#pragma unroll
        for (int k = 0; k < 3; k++) { F.dv1[k] = db->v[k]; F.dp1[k] = db->p[k]; }
    }
}
DEV void via_triple_parts(const ViaFrame& F, double* lam, double& beta, double* gam, double& exc) {
    const double dt1 = F.dt1, dt2 = F.dt2;
    double u1[3], u2[3], u3[3], d1[3], d2[3];
    via_mulv(F.b.Rw, F.dp2, u1); via_mulv(F.a.Rw, F.dp1, u2); via_mulv(F.a.Rw, F.dv1, u3);
    beta = -(((0.5 * dt1) * dt2) * (dt1 + dt2));
#pragma unroll
    for (int r = 0; r < 3; r++) {
        d1[r] = (F.c.C[r] - F.b.C[r]) * dt1; d2[r] = (F.b.C[r] - F.a.C[r]) * dt2;
        lam[r] = d1[r] - d2[r];
        gam[r] = ((u1[r] * dt1 - u2[r] * dt2) + u3[r] * (dt1 * dt2)) - ((F.c.L[r] - F.b.L[r]) * dt1 - (F.b.L[r] - F.a.L[r]) * dt2);
    }
    exc = via_dot(d1, d1) + via_dot(d2, d2);
}
DEV bool via_is_pair(const ViaFrame& F) { return (F.c.flags & VIS_VIT_EDGE) && (F.b.flags & VIS_VIT_POSED) && F.use_c; }
DEV bool via_is_triple(const ViaFrame& F, int S, int E) {
    return (F.c.flags & VIS_VIT_EDGE) && (F.b.flags & VIS_VIT_EDGE) && (F.a.flags & VIS_VIT_POSED) && F.use_c && F.use_b && F.c.seg == S && F.c.epoch == E &&
           F.b.seg == S && F.b.epoch == E;
}
// the ten gyro terms of frame i; false: one is not finite
DEV bool via_gyro_terms(const ViaFrame& F, const vis_imu_delta* __restrict__ D, double* t) {
    double R[9], J[9], V[9], e[3];
#pragma unroll
    for (int k = 0; k < 9; k++) { R[k] = D->R[k]; J[k] = D->JRg[k]; }
    via_tmul(F.b.Rw, F.c.Rw, V);
    via_rot_error(R, V, e);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++, k++) t[k] = (J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b];
#pragma unroll
    for (int a = 0; a < 3; a++) t[6 + a] = (J[a] * e[0] + J[3 + a] * e[1]) + J[6 + a] * e[2];
    t[9] = via_dot(e, e);
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 10; j++) fin = fin && via_finite(t[j]);
    return fin;
}
DEV bool via_linear_terms(const double* lam, double beta, const double* gam, double exc, double* t) {
    t[0] = via_dot(lam, lam); t[1] = lam[0] * beta; t[2] = lam[1] * beta; t[3] = lam[2] * beta; t[4] = beta * beta;
    t[5] = via_dot(lam, gam); t[6] = beta * gam[0]; t[7] = beta * gam[1]; t[8] = beta * gam[2]; t[9] = via_dot(gam, gam); t[10] = exc;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 11; j++) fin = fin && via_finite(t[j]);
    return fin;
}

// ---- the accelerometer bias (vis_vi_align_ba_rows): k_via_align<true>
// via_ldl with the relative pivot test: a D[j] that is not finite, not > 0 or not > rel A[j][j] fails
template <int N>
DEV bool via_ldl_rel(const double (&A)[N][N], const double (&b)[N], double (&x)[N], double rel) {
    double L[N][N], D[N], z[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = A[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (L[j][c] * L[j][c]) * D[c];
        D[j] = s;
        ok = ok && s > 0.0 && via_finite(s) && s > rel * A[j][j];
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = A[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) v = v - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = v / s;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double v = b[i];
#pragma unroll
        for (int c = 0; c < i; c++) v = v - L[i][c] * z[c];
        z[i] = v;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double v = z[i] / D[i];
#pragma unroll
        for (int c = i + 1; c < N; c++) v = v - L[c][i] * x[c];
        x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < N; i++) ok = ok && via_finite(x[i]);
    return ok;
}
DEV bool via_jac_usable(const vis_imu_bias_jac* __restrict__ J, int dq) {
    if (J->flags & VIS_IMU_JAC_NONFINITE) return false;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && via_finite(J->Jvg[k]) && via_finite(J->Jva[k]) && via_finite(J->Jpg[k]) && via_finite(J->Jpa[k]);
    return fin && J->q == dq;
}
// the Jacobian record of frame i's parent beside that parent's delta (null: none), and whether the two of the triple are usable
DEV const vis_imu_bias_jac* via_parent_jac(const ViaFrame& F, const vis_imu_delta* __restrict__ delta, const vis_imu_bias_jac* __restrict__ jac,
                                           const vis_vi_ba_carry* __restrict__ bcarry, bool& usable) {
    usable = false;
    if (F.q >= 0) { usable = via_jac_usable(jac + F.q, delta[F.q].q); return jac + F.q; }
    if (F.q == VIS_KF_CARRIED && bcarry) { usable = via_jac_usable(&bcarry->last_jac, bcarry->carry.last_delta.q); return &bcarry->last_jac; }
    return nullptr;
}
// nB = -B of the triple of F; Jc: the frame's own record, Jb: its parent's
DEV void via_neg_b(const ViaFrame& F, const vis_imu_bias_jac* __restrict__ Jc, const vis_imu_bias_jac* __restrict__ Jb, double* nB) {
    double X[9], P1[9], P2[9], P3[9];
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = Jc->Jpa[k];
    via_mul(F.b.Rw, X, P1);
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = Jb->Jpa[k];
    via_mul(F.a.Rw, X, P2);
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = Jb->Jva[k];
    via_mul(F.a.Rw, X, P3);
#pragma unroll
    for (int k = 0; k < 9; k++) nB[k] = -((P1[k] * F.dt1 - P2[k] * F.dt2) + P3[k] * (F.dt1 * F.dt2));
}
DEV double via_col(const double* nB, const double* v, int c) { return (nB[c] * v[0] + nB[3 + c] * v[1]) + nB[6 + c] * v[2]; }
// the 32 terms of a bias triple; false: one is not finite
DEV bool via_ba_terms(const double* lam, double beta, const double* gam, double exc, const double* nB, double* t) {
    t[0] = via_dot(lam, lam); t[1] = lam[0] * beta; t[2] = lam[1] * beta; t[3] = lam[2] * beta; t[4] = beta * beta;
#pragma unroll
    for (int c = 0; c < 3; c++) { t[5 + c] = via_col(nB, lam, c); t[27 + c] = via_col(nB, gam, c); t[24 + c] = beta * gam[c]; }
#pragma unroll
    for (int k = 0; k < 9; k++) t[8 + k] = beta * nB[k];
    int k = 17;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++, k++) t[k] = (nB[a] * nB[b] + nB[3 + a] * nB[3 + b]) + nB[6 + a] * nB[6 + b];
    t[23] = via_dot(lam, gam); t[30] = via_dot(gam, gam); t[31] = exc;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < VIS_VIAB_SUMS; j++) fin = fin && via_finite(t[j]);
    return fin;
}
// frame i as a bias triple: its parts and nB; false: it is none
DEV bool via_bias_triple(const ViaFrame& F, int S, int E, const vis_imu_delta* __restrict__ delta, const vis_imu_bias_jac* __restrict__ jac,
                         const vis_vi_ba_carry* __restrict__ bcarry, int i, double* lam, double& beta, double* gam, double& exc, double* nB) {
    if (!via_is_triple(F, S, E)) return false;
    double t11[11];
    via_triple_parts(F, lam, beta, gam, exc);
    if (!via_linear_terms(lam, beta, gam, exc, t11)) return false;
    bool jb_ok;
    const vis_imu_bias_jac* Jb = via_parent_jac(F, delta, jac, bcarry, jb_ok);
    if (!jb_ok || !via_jac_usable(jac + i, delta[i].q)) return false;
    via_neg_b(F, jac + i, Jb, nB);
    return true;
}
struct ViaBa { double s, g[3], dba[3], s_lin, g_lin[3], dba_lin[3], g_norm; int flags; };
// the 7 x 7 solve and the rounds on the tangent plane, from the 32 totals alone; o.s, o.g come in as the 4-unknown solution and stay on a fallback
DEV void via_ba_solve(const vis_vi_align_params& P, const vis_vi_align_ba_params& BP, const double* ba, int n_ba, ViaBa& o) {
#pragma unroll
    for (int k = 0; k < 3; k++) o.dba[k] = o.g_lin[k] = o.dba_lin[k] = 0.0;
    o.s_lin = 0.0; o.g_norm = 0.0;
    if (n_ba < BP.min_ba_triples) { o.flags |= VIS_VIAB_FEW; return; }
    double M[7][7], r[7], x[7];
    M[0][0] = ba[0];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        M[0][1 + c] = M[1 + c][0] = ba[1 + c];
        M[0][4 + c] = M[4 + c][0] = ba[5 + c];
#pragma unroll
        for (int rr = 0; rr < 3; rr++) {
            M[1 + rr][1 + c] = rr == c ? ba[4] : 0.0;
            M[1 + rr][4 + c] = M[4 + c][1 + rr] = ba[8 + 3 * rr + c];
        }
    }
    {
        int k = 17;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++, k++) M[4 + a][4 + b] = M[4 + b][4 + a] = ba[k];
    }
#pragma unroll
    for (int k = 0; k < 7; k++) r[k] = ba[23 + k];
    const bool ok7 = via_ldl_rel<7>(M, r, x, BP.pivot_rel);
    const double gn = sqrt(via_dot(x + 1, x + 1));
    if (!ok7 || !(ba[0] > VIS_VIA_EXCITATION_REL * ba[31]) || !via_finite(gn)) { o.flags |= VIS_VIAB_UNOBSERVABLE; return; }
    o.s_lin = x[0]; o.g_norm = gn;
#pragma unroll
    for (int k = 0; k < 3; k++) { o.g_lin[k] = x[1 + k]; o.dba_lin[k] = x[4 + k]; }
    if (!(o.s_lin > 0.0)) { o.flags |= VIS_VIAB_SCALE; return; }
    double gh[3], s3 = o.s_lin, d3[3] = {o.dba_lin[0], o.dba_lin[1], o.dba_lin[2]};
    double nn = via_normalise(o.g_lin, gh);
    bool ok = via_finite(nn) && nn > 0.0;
    for (int it = 0; it < P.refine_iters && ok; it++) {
        int k = 0;
        if (fabs(gh[1]) < fabs(gh[k])) k = 1;
        if (fabs(gh[2]) < fabs(k == 1 ? gh[1] : gh[0])) k = 2;
        const double ghk = k == 0 ? gh[0] : (k == 1 ? gh[1] : gh[2]);
        double d[3], b1[3], b2[3], x0[3], rr[7], w1[3], w2[3], q[6], y[6], N[6][6];
#pragma unroll
        for (int j = 0; j < 3; j++) d[j] = (j == k ? 1.0 : 0.0) - ghk * gh[j];
        (void)via_normalise(d, b1);
        cross3(gh, b1, b2);
#pragma unroll
        for (int j = 0; j < 3; j++) x0[j] = P.G * gh[j];
#pragma unroll
        for (int i = 0; i < 7; i++) rr[i] = r[i] - ((M[i][1] * x0[0] + M[i][2] * x0[1]) + M[i][3] * x0[2]);
        q[0] = rr[0]; q[1] = via_dot(b1, rr + 1); q[2] = via_dot(b2, rr + 1); q[3] = rr[4]; q[4] = rr[5]; q[5] = rr[6];
#pragma unroll
        for (int i = 0; i < 3; i++) { w1[i] = via_dot(&M[1 + i][1], b1); w2[i] = via_dot(&M[1 + i][1], b2); }
        N[0][0] = M[0][0];
        N[0][1] = N[1][0] = via_dot(&M[0][1], b1);
        N[0][2] = N[2][0] = via_dot(&M[0][1], b2);
        N[1][1] = via_dot(b1, w1); N[2][2] = via_dot(b2, w2);
        N[1][2] = N[2][1] = via_dot(b1, w2);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double col[3] = {M[1][4 + c], M[2][4 + c], M[3][4 + c]};
            N[0][3 + c] = N[3 + c][0] = M[0][4 + c];
            N[1][3 + c] = N[3 + c][1] = via_dot(b1, col);
            N[2][3 + c] = N[3 + c][2] = via_dot(b2, col);
#pragma unroll
            for (int a = 0; a < 3; a++) N[3 + a][3 + c] = M[4 + a][4 + c];
        }
        ok = via_ldl_rel<6>(N, q, y, BP.pivot_rel);
        if (!ok) break;
        double gg[3];
#pragma unroll
        for (int j = 0; j < 3; j++) gg[j] = (x0[j] + y[1] * b1[j]) + y[2] * b2[j];
        nn = via_normalise(gg, gh);
        ok = via_finite(nn) && nn > 0.0 && via_finite(gh[0]) && via_finite(gh[1]) && via_finite(gh[2]);
        s3 = y[0]; d3[0] = y[3]; d3[1] = y[4]; d3[2] = y[5];
    }
    const double g3[3] = {P.G * gh[0], P.G * gh[1], P.G * gh[2]};
    if (!ok || !via_finite(g3[0]) || !via_finite(g3[1]) || !via_finite(g3[2]) || !via_finite(d3[0]) || !via_finite(d3[1]) || !via_finite(d3[2]))
        o.flags |= VIS_VIAB_UNOBSERVABLE;
    else if (!(via_finite(s3) && s3 > 0.0)) o.flags |= VIS_VIAB_SCALE;
    else {
        o.s = s3;
#pragma unroll
        for (int k = 0; k < 3; k++) { o.g[k] = g3[k]; o.dba[k] = d3[k]; }
    }
}


template <bool BA>
__global__ __launch_bounds__(VIA_BLOCK) void k_via_align(vis_vi_align_params P, int n, FtFrames fr, const vis_traj_pose* __restrict__ traj,
                                                         const vis_imu_delta* __restrict__ delta, const vis_vi_carry* __restrict__ carry_in,
                                                         vis_vi_state* __restrict__ state, vis_vi_align* __restrict__ result,
                                                         vis_vi_carry* __restrict__ carry_out, ViaBaArgs<BA> X) {
    // BA: carry_in, result and carry_out are the heads of a vis_vi_ba_carry, a vis_vi_align_ba and a vis_vi_ba_carry; X has the rest
    __shared__ int s_posed, s_saved, s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) { s_posed = -1; s_saved = -1; s_bad = 0; }
    __syncthreads();
    // ---- phase 1: the carry's numbers, the newest posed frame and the last saved one
    const bool given = carry_in && (carry_in->valid & VIS_VIC_VALID);
    if (given) {
        const double* num = nullptr;                              // the 81 numbers: gyro 10 and lin 16, two tails of 15, the delta's 25, each group contiguous
        if (tid < 26) num = reinterpret_cast<const double*>(carry_in) + tid;
        else if (tid < 41) num = reinterpret_cast<const double*>(&carry_in->last) + (tid - 26);
        else if (tid < 56) num = reinterpret_cast<const double*>(&carry_in->parent) + (tid - 41);
        else if (tid < 81) num = reinterpret_cast<const double*>(&carry_in->last_delta) + (tid - 56);
        if (num && !via_finite(*num)) atomicOr(&s_bad, 1);
        if constexpr (BA) {                                       // the bias part: 32 sums and the 36 numbers of last_jac
            const vis_vi_ba_carry* bc = reinterpret_cast<const vis_vi_ba_carry*>(carry_in);
            num = nullptr;
            if (tid >= 81 && tid < 113) num = bc->ba + (tid - 81);
            else if (tid >= 113 && tid < 149) num = reinterpret_cast<const double*>(&bc->last_jac) + (tid - 113);
            if (num && !via_finite(*num)) atomicOr(&s_bad, 2);
        }
    }
    {
        int posed = -1, saved = -1;
        for (int i = tid; i < n; i += VIA_BLOCK) {
            const int q = via_prev(fr, i);
            ViaTail t;
            via_tail(P, traj + i, q, t);
            if (t.flags & VIS_VIT_POSED) posed = i;
            if (q != VIS_KF_NOT_SAVED) saved = i;
        }
        atomicMax(&s_posed, posed); atomicMax(&s_saved, saved);
    }
    __syncthreads();
    const bool bad_carry = BA ? (s_bad & 1) != 0 : s_bad != 0;
    const vis_vi_carry* carry = given && !bad_carry ? carry_in : nullptr;
    const int newest = s_posed, last = s_saved;
    int flags = bad_carry ? VIS_VIA_BAD_CARRY : 0;
    int S = -1, E = -1;
    if (newest >= 0) {
        ViaTail t;
        via_tail(P, traj + newest, via_prev(fr, newest), t);
        S = t.seg; E = t.epoch;
    } else if (carry) { S = carry->segment_seq; E = carry->epoch_seq; }
    // ---- phase 2: the terms and the sums
    double sums[21];
#pragma unroll
    for (int k = 0; k < 21; k++) sums[k] = 0.0;
    int np_call = 0, nt_call = 0;
    for (int i = tid; i < n; i += VIA_BLOCK) {
        ViaFrame F;
        via_gather(P, fr, traj, delta, carry, i, F);
        double t[11];
        if (via_is_pair(F) && via_gyro_terms(F, delta + i, t)) {
            np_call++;
#pragma unroll
            for (int k = 0; k < 10; k++) sums[k] = sums[k] + t[k];
        }
        if (via_is_triple(F, S, E)) {
            double lam[3], beta, gam[3], exc;
            via_triple_parts(F, lam, beta, gam, exc);
            if (via_linear_terms(lam, beta, gam, exc, t)) {
                nt_call++;
#pragma unroll
                for (int k = 0; k < 11; k++) sums[10 + k] = sums[10 + k] + t[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 21; k++) sums[k] = wave_sum(sums[k]);
    { int none = 0; ep_totals<4>(sums, none); }
    ep_counts<4>(np_call, nt_call);
    // ---- phase 2b (BA): the terms of the bias triples and their sums, a pass of its own
    [[maybe_unused]] const vis_vi_ba_carry* bcarry = nullptr;
    [[maybe_unused]] double ba[BA ? VIS_VIAB_SUMS : 1];
    [[maybe_unused]] int nb_call = 0, n_ba = 0, ba_flags = 0;
    if constexpr (BA) {
        if (carry) {
            if (s_bad & 2) ba_flags = VIS_VIAB_BAD_CARRY;
            else bcarry = reinterpret_cast<const vis_vi_ba_carry*>(carry_in);
        }
#pragma unroll
        for (int k = 0; k < VIS_VIAB_SUMS; k++) ba[k] = 0.0;
        for (int i = tid; i < n; i += VIA_BLOCK) {
            ViaFrame F;
            via_gather(P, fr, traj, delta, carry, i, F);
            double lam[3], beta, gam[3], exc, nB[9], t[VIS_VIAB_SUMS];
            if (via_bias_triple(F, S, E, delta, X.jac, bcarry, i, lam, beta, gam, exc, nB) && via_ba_terms(lam, beta, gam, exc, nB, t)) {
                nb_call++;
#pragma unroll
                for (int k = 0; k < VIS_VIAB_SUMS; k++) ba[k] = ba[k] + t[k];
            }
        }
#pragma unroll
        for (int k = 0; k < VIS_VIAB_SUMS; k++) ba[k] = wave_sum(ba[k]);
        { int none = 0; ep_totals<4>(ba, none); }
        { int none = 0; ep_counts<4>(nb_call, none); }
        n_ba = nb_call;
        if (bcarry && carry->segment_seq == S && carry->epoch_seq == E) {
#pragma unroll
            for (int k = 0; k < VIS_VIAB_SUMS; k++) ba[k] = bcarry->ba[k] + ba[k];
            n_ba = bcarry->n_ba_triples + nb_call;
        }
        bool fin = true;
#pragma unroll
        for (int k = 0; k < VIS_VIAB_SUMS; k++) fin = fin && via_finite(ba[k]);
        if (!fin) {
#pragma unroll
            for (int k = 0; k < VIS_VIAB_SUMS; k++) ba[k] = 0.0;
            n_ba = 0; ba_flags |= VIS_VIAB_UNOBSERVABLE;
        }
    }
    // ---- phase 3: the totals and the solves, on every thread
    double gyro[10], lin[16];
#pragma unroll
    for (int k = 0; k < 10; k++) gyro[k] = sums[k];
    {
        const double* t = sums + 10;
        const double ex[16] = {t[0], t[1], t[2], t[3], t[4], 0.0, 0.0, t[4], 0.0, t[4], t[5], t[6], t[7], t[8], t[9], t[10]};
#pragma unroll
        for (int k = 0; k < 16; k++) lin[k] = ex[k];
    }
    const double c0_call = gyro[9];
    int n_pairs = np_call, n_triples = nt_call;
    if (carry) {
#pragma unroll
        for (int k = 0; k < 10; k++) gyro[k] = carry->gyro[k] + gyro[k];
        n_pairs = carry->n_pairs + np_call;
        if (carry->segment_seq == S && carry->epoch_seq == E) {
#pragma unroll
            for (int k = 0; k < 16; k++) lin[k] = carry->lin[k] + lin[k];
            n_triples = carry->n_triples + nt_call;
        } else flags |= VIS_VIA_RESTART;
    }
    {
        bool gfin = true, lfin = true;                            // (finite terms can still overflow a sum)
#pragma unroll
        for (int k = 0; k < 10; k++) gfin = gfin && via_finite(gyro[k]);
#pragma unroll
        for (int k = 0; k < 16; k++) lfin = lfin && via_finite(lin[k]);
        if (!gfin) {
#pragma unroll
            for (int k = 0; k < 10; k++) gyro[k] = 0.0;
            n_pairs = 0; flags |= VIS_VIA_GYRO_SINGULAR;
        }
        if (!lfin) {
#pragma unroll
            for (int k = 0; k < 16; k++) lin[k] = 0.0;
            n_triples = 0; flags |= VIS_VIA_SINGULAR;
        }
    }
    double dbg[3] = {0.0, 0.0, 0.0};
    if (n_pairs < P.min_pairs) flags |= VIS_VIA_GYRO_FEW;
    else {
        const double H[3][3] = {{gyro[0], gyro[1], gyro[2]}, {gyro[1], gyro[3], gyro[4]}, {gyro[2], gyro[4], gyro[5]}};
        const double b[3] = {gyro[6], gyro[7], gyro[8]};
        double x[3];
        if (via_ldl<3>(H, b, x)) { dbg[0] = x[0]; dbg[1] = x[1]; dbg[2] = x[2]; }
        else flags |= VIS_VIA_GYRO_SINGULAR;
    }
    double s = 1.0, g[3] = {0.0, 0.0, 0.0}, s_lin = 0.0, g_lin[3] = {0.0, 0.0, 0.0}, g_norm = 0.0;
    if (n_triples < P.min_triples) flags |= VIS_VIA_FEW;
    else {
        double M[4][4], r[4], x[4];
        {
            int k = 0;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = a; b < 4; b++, k++) M[a][b] = M[b][a] = lin[k];
#pragma unroll
            for (int a = 0; a < 4; a++) r[a] = lin[10 + a];
        }
        if (!via_ldl<4>(M, r, x) || !(lin[0] > VIS_VIA_EXCITATION_REL * lin[15])) flags |= VIS_VIA_SINGULAR;
        else {
            s_lin = x[0]; g_lin[0] = x[1]; g_lin[1] = x[2]; g_lin[2] = x[3];
            g_norm = sqrt(via_dot(g_lin, g_lin));
            if (!via_finite(g_norm)) { flags |= VIS_VIA_SINGULAR; s_lin = 0.0; g_lin[0] = g_lin[1] = g_lin[2] = 0.0; g_norm = 0.0; }
            else {
                if (fabs(g_norm - P.G) > P.g_tol * P.G) flags |= VIS_VIA_GRAVITY_NORM;
                if (!(s_lin > 0.0)) flags |= VIS_VIA_SCALE;
                else {
                    // step 3: gravity of norm G from M and r alone
                    double gh[3], s3 = s_lin;
                    double nn = via_normalise(g_lin, gh);
                    bool ok = via_finite(nn) && nn > 0.0;
                    for (int it = 0; it < P.refine_iters && ok; it++) {
                        int k = 0;
                        if (fabs(gh[1]) < fabs(gh[k])) k = 1;
                        if (fabs(gh[2]) < fabs(k == 1 ? gh[1] : gh[0])) k = 2;
                        const double ghk = k == 0 ? gh[0] : (k == 1 ? gh[1] : gh[2]);
                        double d[3], b1[3], b2[3], x0[3], rr[4], w1[3], w2[3], y[3];
#pragma unroll
                        for (int j = 0; j < 3; j++) d[j] = (j == k ? 1.0 : 0.0) - ghk * gh[j];
                        (void)via_normalise(d, b1);
                        cross3(gh, b1, b2);
#pragma unroll
                        for (int j = 0; j < 3; j++) x0[j] = P.G * gh[j];
#pragma unroll
                        for (int i = 0; i < 4; i++) rr[i] = r[i] - ((M[i][1] * x0[0] + M[i][2] * x0[1]) + M[i][3] * x0[2]);
                        const double q[3] = {rr[0], via_dot(b1, rr + 1), via_dot(b2, rr + 1)};
#pragma unroll
                        for (int i = 0; i < 3; i++) { w1[i] = via_dot(&M[1 + i][1], b1); w2[i] = via_dot(&M[1 + i][1], b2); }
                        const double n01 = via_dot(&M[0][1], b1), n02 = via_dot(&M[0][1], b2), n12 = via_dot(b1, w2);
                        const double N[3][3] = {{M[0][0], n01, n02}, {n01, via_dot(b1, w1), n12}, {n02, n12, via_dot(b2, w2)}};
                        ok = via_ldl<3>(N, q, y);
                        if (!ok) break;
                        double gg[3];
#pragma unroll
                        for (int j = 0; j < 3; j++) gg[j] = (x0[j] + y[1] * b1[j]) + y[2] * b2[j];
                        nn = via_normalise(gg, gh);
                        ok = via_finite(nn) && nn > 0.0 && via_finite(gh[0]) && via_finite(gh[1]) && via_finite(gh[2]);
                        s3 = y[0];
                    }
                    const double g3[3] = {P.G * gh[0], P.G * gh[1], P.G * gh[2]};
                    if (!ok || !via_finite(g3[0]) || !via_finite(g3[1]) || !via_finite(g3[2])) flags |= VIS_VIA_SINGULAR;
                    else if (!(via_finite(s3) && s3 > 0.0)) flags |= VIS_VIA_SCALE;
                    else { s = s3; g[0] = g3[0]; g[1] = g3[1]; g[2] = g3[2]; }
                }
            }
        }
    }
    [[maybe_unused]] ViaBa bo;
    [[maybe_unused]] bool ba_ok = false;
    if constexpr (BA) {
        bo.s = s; bo.g[0] = g[0]; bo.g[1] = g[1]; bo.g[2] = g[2]; bo.flags = ba_flags;
        via_ba_solve(P, X.bp, ba, n_ba, bo);
        ba_ok = !(bo.flags & (VIS_VIAB_FEW | VIS_VIAB_UNOBSERVABLE | VIS_VIAB_SCALE));
    }
    // ---- phase 4: the second pass and the states
    double sums2[BA ? 3 : 2] = {0.0, 0.0};
    for (int i = tid; i < n; i += VIA_BLOCK) {
        ViaFrame F;
        via_gather(P, fr, traj, delta, carry, i, F);
        vis_vi_state st;
#pragma unroll
        for (int k = 0; k < 3; k++) st.p[k] = st.v[k] = 0.0;
        st.res = 0.0; st.q = F.q;
        int f = 0;
        const bool in_se = (F.c.flags & VIS_VIT_POSED) && F.c.seg == S && F.c.epoch == E;
        double pc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) pc[r] = s * F.c.C[r] + F.c.L[r];
        if (in_se && via_finite(pc[0]) && via_finite(pc[1]) && via_finite(pc[2])) { st.p[0] = pc[0]; st.p[1] = pc[1]; st.p[2] = pc[2]; f |= VIS_VIS_HAS_P; }
        if (in_se && (F.c.flags & VIS_VIT_EDGE) && F.use_c && (F.b.flags & VIS_VIT_POSED) && F.b.seg == S) {
            double z[3], w[3], v[3];
#pragma unroll
            for (int k = 0; k < 3; k++) z[k] = F.dv2[k] - F.dp2[k] / F.dt2;
            via_mulv(F.b.Rw, z, w);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double pb = s * F.b.C[r] + F.b.L[r];
                v[r] = ((pc[r] - pb) / F.dt2 + (0.5 * g[r]) * F.dt2) + w[r];
            }
            if (via_finite(v[0]) && via_finite(v[1]) && via_finite(v[2])) { st.v[0] = v[0]; st.v[1] = v[1]; st.v[2] = v[2]; f |= VIS_VIS_HAS_V; }
        }
        double t[11];
        if (via_is_pair(F) && via_gyro_terms(F, delta + i, t)) {
            f |= VIS_VIS_HAS_PAIR;
            double R[9], J[9], phi[3], X[9], R2[9], V[9], e[3];
#pragma unroll
            for (int k = 0; k < 9; k++) { R[k] = delta[i].R[k]; J[k] = delta[i].JRg[k]; }
            via_mulv(J, dbg, phi);
            via_exp(phi, X);
            via_mul(R, X, R2);
            via_tmul(F.b.Rw, F.c.Rw, V);
            via_rot_error(R2, V, e);
            const double e1 = via_dot(e, e);
            if (via_finite(e1)) sums2[0] = sums2[0] + e1;
        }
        if (via_is_triple(F, S, E)) {
            double lam[3], beta, gam[3], rho[3], exc;
            via_triple_parts(F, lam, beta, gam, exc);
            if (via_linear_terms(lam, beta, gam, exc, t)) {
                f |= VIS_VIS_HAS_TRIPLE;
#pragma unroll
                for (int r = 0; r < 3; r++) rho[r] = (lam[r] * s + beta * g[r]) - gam[r];
                const double rr = via_dot(rho, rho);
                if (via_finite(rr)) { sums2[1] = sums2[1] + rr; st.res = sqrt(rr); }
            }
        }
        if constexpr (BA) {
            if (ba_ok) {                                          // the states under (s_ba, g_ba, dba) in the place of those under (s, g)
#pragma unroll
                for (int k = 0; k < 3; k++) st.p[k] = st.v[k] = 0.0;
                st.res = 0.0; f &= VIS_VIS_HAS_PAIR;
                double pa[3];
#pragma unroll
                for (int r = 0; r < 3; r++) pa[r] = bo.s * F.c.C[r] + F.c.L[r];
                if (in_se && via_finite(pa[0]) && via_finite(pa[1]) && via_finite(pa[2])) { st.p[0] = pa[0]; st.p[1] = pa[1]; st.p[2] = pa[2]; f |= VIS_VIS_HAS_P; }
                if (in_se && (F.c.flags & VIS_VIT_EDGE) && F.use_c && (F.b.flags & VIS_VIT_POSED) && F.b.seg == S && via_jac_usable(X.jac + i, delta[i].q)) {
                    double Jv[9], Jp[9], ev[3], ep[3], z[3], w[3], v[3];
#pragma unroll
                    for (int k = 0; k < 9; k++) { Jv[k] = X.jac[i].Jva[k]; Jp[k] = X.jac[i].Jpa[k]; }
                    via_mulv(Jv, bo.dba, ev); via_mulv(Jp, bo.dba, ep);
#pragma unroll
                    for (int k = 0; k < 3; k++) z[k] = (F.dv2[k] + ev[k]) - (F.dp2[k] + ep[k]) / F.dt2;
                    via_mulv(F.b.Rw, z, w);
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const double pb = bo.s * F.b.C[r] + F.b.L[r];
                        v[r] = ((pa[r] - pb) / F.dt2 + (0.5 * bo.g[r]) * F.dt2) + w[r];
                    }
                    if (via_finite(v[0]) && via_finite(v[1]) && via_finite(v[2])) { st.v[0] = v[0]; st.v[1] = v[1]; st.v[2] = v[2]; f |= VIS_VIS_HAS_V; }
                }
                double lam[3], beta, gam[3], exc, nB[9], t32[VIS_VIAB_SUMS];
                if (via_bias_triple(F, S, E, delta, X.jac, bcarry, i, lam, beta, gam, exc, nB) && via_ba_terms(lam, beta, gam, exc, nB, t32)) {
                    f |= VIS_VIS_HAS_TRIPLE;
                    double Bd[3], rho[3];
                    via_mulv(nB, bo.dba, Bd);
#pragma unroll
                    for (int r = 0; r < 3; r++) rho[r] = ((lam[r] * bo.s + beta * bo.g[r]) + Bd[r]) - gam[r];
                    const double rr = via_dot(rho, rho);
                    if (via_finite(rr)) { sums2[2] = sums2[2] + rr; st.res = sqrt(rr); }
                }
            }
        }
        st.flags = f;
        if (state) state[i] = st;
    }
    sums2[0] = wave_sum(sums2[0]); sums2[1] = wave_sum(sums2[1]);
    if constexpr (BA) sums2[2] = wave_sum(sums2[2]);
    { int none = 0; ep_totals<4>(sums2, none); }
    // ---- phase 5: the result and the carry
    if (tid != 0) return;
    vis_vi_align res;
#pragma unroll
    for (int k = 0; k < 3; k++) { res.dbg[k] = dbg[k]; res.g[k] = g[k]; res.g_lin[k] = g_lin[k]; }
    res.c0 = gyro[9]; res.c0_call = via_finite(c0_call) ? c0_call : 0.0; res.c1 = via_finite(sums2[0]) ? sums2[0] : 0.0; res.s = s; res.s_lin = s_lin; res.g_lin_norm = g_norm;
    res.rms = nt_call > 0 && via_finite(sums2[1]) ? sqrt(sums2[1] / (double)nt_call) : 0.0;
    res.n_pairs = n_pairs; res.n_triples = n_triples; res.n_pairs_call = np_call; res.n_triples_call = nt_call;
    res.segment_seq = S; res.epoch_seq = E; res.flags = flags; res.reserved_ = 0;
    *result = res;
    if constexpr (BA) {
        vis_vi_align_ba* rb = reinterpret_cast<vis_vi_align_ba*>(result);
#pragma unroll
        for (int k = 0; k < 3; k++) { rb->dba[k] = bo.dba[k]; rb->g_ba[k] = bo.g[k]; rb->dba_lin[k] = bo.dba_lin[k]; rb->g_lin7[k] = bo.g_lin[k]; }
        rb->s_ba = bo.s; rb->s_lin7 = bo.s_lin; rb->g_lin7_norm = bo.g_norm;
        rb->rms_ba = ba_ok && nb_call > 0 && via_finite(sums2[2]) ? sqrt(sums2[2] / (double)nb_call) : 0.0;
        rb->n_ba_triples = n_ba; rb->n_ba_triples_call = nb_call; rb->ba_flags = bo.flags; rb->reserved_ = 0;
    }
    if (!carry_out) return;
    if constexpr (BA) {
        vis_vi_ba_carry* cb = reinterpret_cast<vis_vi_ba_carry*>(carry_out);
#pragma unroll
        for (int k = 0; k < VIS_VIAB_SUMS; k++) cb->ba[k] = ba[k];
        cb->n_ba_triples = n_ba; cb->reserved_ = 0;
        vis_imu_bias_jac zj;
#pragma unroll
        for (int k = 0; k < 9; k++) zj.Jvg[k] = zj.Jva[k] = zj.Jpg[k] = zj.Jpa[k] = 0.0;
        zj.flags = VIS_IMU_JAC_NONFINITE; zj.q = 0;
        if (last >= 0) {
            if (via_usable(P, delta + last, traj[last].parent) && via_jac_usable(X.jac + last, delta[last].q)) zj = X.jac[last];
        } else if (bcarry) zj = bcarry->last_jac;
        cb->last_jac = zj;
    }
#pragma unroll
    for (int k = 0; k < 10; k++) carry_out->gyro[k] = gyro[k];
#pragma unroll
    for (int k = 0; k < 16; k++) carry_out->lin[k] = lin[k];
    carry_out->n_pairs = n_pairs; carry_out->n_triples = n_triples; carry_out->segment_seq = S; carry_out->epoch_seq = E;
    carry_out->valid = VIS_VIC_VALID; carry_out->reserved_ = 0;
    vis_imu_delta zd;
    {
#pragma unroll
        for (int k = 0; k < 9; k++) zd.R[k] = zd.JRg[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) zd.v[k] = zd.p[k] = 0.0;
        zd.dt = 0.0; zd.n_steps = zd.flags = zd.q = zd.reserved_ = 0;
    }
    if (last >= 0) {
        ViaFrame F;
        via_gather(P, fr, traj, delta, carry, last, F);
        via_tail_store(F.c, F.c.flags | (F.use_c ? VIS_VIT_DELTA : 0), carry_out->last);
        via_tail_store(F.b, F.b.flags & VIS_VIT_POSED, carry_out->parent);
        if (F.use_c) { zd = delta[last]; zd.reserved_ = 0; }
        carry_out->last_delta = zd;
    } else if (carry) {
        vis_vi_tail a = carry->last, b = carry->parent;
        zd = carry->last_delta;
        a.reserved_ = 0; b.reserved_ = 0; zd.reserved_ = 0;
        carry_out->last = a; carry_out->parent = b; carry_out->last_delta = zd;
    } else {
        ViaTail z;
        via_zero_tail(z);
        via_tail_store(z, 0, carry_out->last); via_tail_store(z, 0, carry_out->parent);
        carry_out->last_delta = zd;
    }
}

// ---------------------------------------------------------------------------------------------- the inertial factor of a pair
// One lane per frame: the residual of the pair's delta against the aligned states of the frame and its parent, and its chi-square under the
// delta's covariance (include/vislam_hip.h "THE INERTIAL FACTOR"; tests/imu_factor_ref.py restates it).  No workspace; tails are recomputed.
#define VIF_BLOCK 64
__global__ __launch_bounds__(VIF_BLOCK) void k_imu_factor(vis_vi_align_params P, vis_imu_factor_params FP, int n, FtFrames fr, const vis_traj_pose* __restrict__ traj,
                                                          const vis_imu_delta* __restrict__ delta, const vis_imu_cov* __restrict__ cov,
                                                          const vis_vi_state* __restrict__ state, const vis_vi_align* __restrict__ result,
                                                          vis_imu_factor* __restrict__ out) {
    const int i = blockIdx.x * VIF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int q = via_prev(fr, i);
    vis_imu_factor o;
#pragma unroll
    for (int k = 0; k < 9; k++) o.r[k] = 0.0;
    o.chi2 = o.chi2_rot = 0.0; o.flags = 0; o.q = q;
    ViaTail tc, tb;
    if (q >= 0) {
        via_tail(P, traj + i, q, tc);
        via_tail(P, traj + q, via_prev(fr, q), tb);
    }
    if (q < 0 || !(tc.flags & VIS_VIT_EDGE) || !(tb.flags & VIS_VIT_POSED)) { o.flags = VIS_IMF_NO_PARENT; out[i] = o; return; }
    const int need = VIS_VIS_HAS_P | VIS_VIS_HAS_V;
    if ((state[i].flags & need) != need || (state[q].flags & need) != need) o.flags |= VIS_IMF_NO_STATE;
    if (result->flags & (VIS_VIA_FEW | VIS_VIA_SINGULAR | VIS_VIA_SCALE)) o.flags |= VIS_IMF_NO_ALIGN;
    const vis_imu_delta* D = delta + i;
    const vis_imu_cov* S = cov + i;
    bool sfin = true;
    for (int k = 0; k < 45; k++) sfin = sfin && via_finite(S->S[k]);
    if (!via_usable(P, D, traj[i].parent) || (S->flags & VIS_IMU_COV_NONFINITE) || !sfin || S->q != D->q) o.flags |= VIS_IMF_UNUSABLE;
    if (o.flags) { out[i] = o; return; }
    // the residual
    double r[9], V[9], dR[9], w[3], x[3], g[3];
    const double dt = D->dt;
#pragma unroll
    for (int k = 0; k < 9; k++) dR[k] = D->R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = result->g[k];
    via_tmul(tb.Rw, tc.Rw, V);
    via_rot_error(dR, V, r);
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = (state[i].v[k] - state[q].v[k]) - g[k] * dt;
    via_tmulv(tb.Rw, w, x);
#pragma unroll
    for (int k = 0; k < 3; k++) r[3 + k] = x[k] - D->v[k];
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = ((state[i].p[k] - state[q].p[k]) - state[q].v[k] * dt) - (0.5 * g[k]) * (dt * dt);
    via_tmulv(tb.Rw, w, x);
#pragma unroll
    for (int k = 0; k < 3; k++) r[6 + k] = x[k] - D->p[k];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && via_finite(r[k]);
    if (!fin) { o.flags = VIS_IMF_NONFINITE; out[i] = o; return; }
    // chi-square: (S + diag) y = r by LDL^T, the lower triangle read from the record's upper one
    double A[9][9], y[9], A3[3][3], r3[3], y3[3];
#pragma unroll
    for (int a = 0; a < 9; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) {
            const double s = S->S[b * 9 - b * (b - 1) / 2 + (a - b)];
            A[a][b] = a == b ? s + (a < 3 ? FP.var_rot : (a < 6 ? FP.var_v : FP.var_p)) : s;
            A[b][a] = A[a][b];
        }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r3[a] = r[a];
#pragma unroll
        for (int b = 0; b < 3; b++) A3[a][b] = A[a][b];
    }
    if (!via_ldl<9>(A, r, y) || !via_ldl<3>(A3, r3, y3)) { o.flags = VIS_IMF_SINGULAR; out[i] = o; return; }
    double c9 = r[0] * y[0];
#pragma unroll
    for (int k = 1; k < 9; k++) c9 = c9 + r[k] * y[k];
    const double c3 = (r[0] * y3[0] + r[1] * y3[1]) + r[2] * y3[2];
    if (!via_finite(c9) || !via_finite(c3)) { o.flags = VIS_IMF_NONFINITE; out[i] = o; return; }
#pragma unroll
    for (int k = 0; k < 9; k++) o.r[k] = r[k];
    o.chi2 = c9; o.chi2_rot = c3;
    out[i] = o;
}

int imu_factor_launch(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_imu_factor_params* fp, int n, FtFrames fr, const vis_traj_pose* d_traj,
                      const vis_imu_delta* d_delta, const vis_imu_cov* d_cov, const vis_vi_state* d_state, const vis_vi_align* d_result,
                      vis_imu_factor* d_factor) {
    if (n < 1) return VIS_OK;
    if (n > VIS_VIA_MAX_FRAMES) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_imu_factor, dim3((n + VIF_BLOCK - 1) / VIF_BLOCK), dim3(VIF_BLOCK), 0, ctx->stream, *vp, *fp, n, fr, d_traj, d_delta, d_cov, d_state, d_result,
                       d_factor);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int via_launch(vis_ctx* ctx, const vis_vi_align_params* vp, int n, FtFrames fr, const vis_traj_pose* d_traj, const vis_imu_delta* d_delta,
               const vis_vi_carry* d_carry, vis_vi_state* d_state, vis_vi_align* d_result, vis_vi_carry* d_carry_out) {
    if (n < 0 || n > VIS_VIA_MAX_FRAMES || !d_result) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_via_align<false>, dim3(1), dim3(VIA_BLOCK), 0, ctx->stream, *vp, n, fr, d_traj, d_delta, d_carry, d_state, d_result, d_carry_out,
                       ViaBaArgs<false>{});
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int via_ba_launch(vis_ctx* ctx, const vis_vi_align_params* vp, const vis_vi_align_ba_params* bp, int n, FtFrames fr, const vis_traj_pose* d_traj,
                  const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const vis_vi_ba_carry* d_carry, vis_vi_state* d_state,
                  vis_vi_align_ba* d_result, vis_vi_ba_carry* d_carry_out) {
    if (n < 0 || n > VIS_VIA_MAX_FRAMES || !d_result || !d_jac) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_via_align<true>, dim3(1), dim3(VIA_BLOCK), 0, ctx->stream, *vp, n, fr, d_traj, d_delta, d_carry ? &d_carry->carry : nullptr, d_state,
                       &d_result->a, d_carry_out ? &d_carry_out->carry : nullptr, ViaBaArgs<true>{*bp, d_jac});
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
