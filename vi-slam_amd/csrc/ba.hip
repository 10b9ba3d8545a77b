// ba.hip -- windowed bundle adjustment over feature tracks (include/vislam_hip.h has the contract, tests/ba_ref.py restates it).
// k_ba_window: one workgroup per window.  The reduced camera system (at most 96 unknowns) lives in LDS as a packed triangle in double; the points are
// never stored apart from their output records: a point's views are re-walked along d_obs in every pass.  A pass visits the owned slots in chunks
// of 256 (one slot per lane); the build pass compacts the used points of a chunk, in slot order, and stages BA_BP of them at a time in LDS (per
// view U, V, W, 1 / W, the weight and the residual; per point the inverse of its damped block and its gradient), then every lane owns entries of
// the system (a row of six of one 6 x 6 block pair) and adds the staged points' terms to them in slot order -- a fixed order per entry, no
// atomics, the same for any launch shape.  DESIGN.md 4.26 has what that order costs.
// The candidate's points are not stored either: the cost pass forms dX again from the old state and costs X + dX; an accepted step forms it a
// third time and writes it.  k_ba_stitch chains the windows through their shared frames in one workgroup; k_ba_points moves the points.
#include "vis_internal.h"
#include "ftri_core.h"
#include <cmath>

#define BA_BLOCK 256
#define BA_MAXF 17                                                 // frames of a window: stride + 1
#define BA_MAXC 16                                                 // free cameras
#define BA_NMAX (6 * BA_MAXC)
#define BA_BP 12                                                   // points staged at a time
#define BA_MARK 0x80                                               // flag byte of a slot that a later owned frame continues (inside the kernel only)

struct BaArgs {
    FtriArgs t; vis_ba_params bp; const double* poses; double* poses_out; vis_ba_window* win; vis_ba_point* pts; uint8_t* flags;
};

struct BaShared {
    double A[BA_NMAX * (BA_NMAX + 1) / 2];                         // T, then A, then L (below the diagonal); element (i, k <= i) at i (i + 1) / 2 + k
    double U[BA_MAXC][21], b[BA_NMAX], Tg[BA_NMAX], z[BA_NMAX], D[BA_NMAX];   // b holds the step d after the solve
    double Pin[BA_MAXF][12], Pc[BA_MAXF][12], Pn[BA_MAXF][12];
    union {
        struct { double ob[BA_BP][BA_MAXF][7], Vi[BA_BP][6], g[BA_BP][3]; } st;
        double cost[BA_BLOCK];
    } u;
    int list[BA_BLOCK];
    int nk[BA_MAXF], cidx[BA_MAXF], posed[BA_MAXF], prevf[BA_MAXF];   // of the window's frames: nk(i), camera index or -1, has a pose, ft_prev
    int nv[BA_BP], okp[BA_BP], wcnt[BA_BLOCK / 64], cnt[2];
    double bc[2];                                                  // broadcast of lane 0's sums
    signed char vfr[BA_BP][BA_MAXF], vpos[BA_BP][BA_MAXC];
};
static_assert(sizeof(BaShared) <= 64 * 1024, "k_ba_window's LDS stays under 64 KB");

struct BaK { double fx, fy, cx, cy, hub; };
struct BaObs { double U, V, W, iw, un, vn, ru, rv, fu, fv, e2, w, term; };

__device__ __forceinline__ void ba_observe(const BaK& K, const double* P, const double* X, double u, double v, BaObs& o) {
    o.U = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[9];
    o.V = ((P[3] * X[0] + P[4] * X[1]) + P[5] * X[2]) + P[10];
    o.W = ((P[6] * X[0] + P[7] * X[1]) + P[8] * X[2]) + P[11];
    o.iw = 1.0 / o.W; o.un = o.U * o.iw; o.vn = o.V * o.iw;
    o.ru = (K.fx * o.un + K.cx) - u; o.rv = (K.fy * o.vn + K.cy) - v;
    o.fu = K.fx * o.iw; o.fv = K.fy * o.iw;
    o.e2 = o.ru * o.ru + o.rv * o.rv;
    const double e = sqrt(o.e2);
    const bool quad = K.hub == 0.0 || e <= K.hub;
    o.w = quad ? 1.0 : K.hub / e;
    o.term = quad ? o.e2 : (2.0 * K.hub) * e - K.hub * K.hub;
}
__device__ __forceinline__ void ba_point_rows(const BaObs& o, const double* P, double* ju, double* jv) {
#pragma unroll
    for (int k = 0; k < 3; k++) { ju[k] = o.fu * (P[k] - o.un * P[6 + k]); jv[k] = o.fv * (P[3 + k] - o.vn * P[6 + k]); }
}
// entry a of the camera rows Cu, Cv: the same twelve formulas as ba_cam_rows below, which must agree with these to the letter
__device__ __forceinline__ void ba_cam_entry(const BaObs& o, int a, double& cu, double& cv) {
    switch (a) {
    case 0: cu = -(o.fu * (o.un * o.V)); cv = -(o.fv * (o.W + o.vn * o.V)); break;
    case 1: cu = o.fu * (o.W + o.un * o.U); cv = o.fv * (o.vn * o.U); break;
    case 2: cu = -(o.fu * o.V); cv = o.fv * o.U; break;
    case 3: cu = o.fu; cv = 0.0; break;
    case 4: cu = 0.0; cv = o.fv; break;
    default: cu = -(o.fu * o.un); cv = -(o.fv * o.vn); break;
    }
}
__device__ __forceinline__ void ba_cam_rows(const BaObs& o, double* cu, double* cv) {
    cu[0] = -(o.fu * (o.un * o.V)); cu[1] = o.fu * (o.W + o.un * o.U); cu[2] = -(o.fu * o.V); cu[3] = o.fu; cu[4] = 0.0; cu[5] = -(o.fu * o.un);
    cv[0] = -(o.fv * (o.W + o.vn * o.V)); cv[1] = o.fv * (o.vn * o.U); cv[2] = o.fv * o.U; cv[3] = 0.0; cv[4] = o.fv; cv[5] = -(o.fv * o.vn);
}

// the used views of the track that ends in (i0, k0), newest to oldest: f(local frame, u, v)
template <class F> __device__ __forceinline__ void ba_walk(const FtriArgs& a, const BaShared& s, int first, int lo, int i0, int k0, F&& f) {
    int i = i0, k = k0;
    for (int w = 0; w < BA_MAXF; w++) {
        const int l = i - first;
        if (s.posed[l]) {
            const float* px = reinterpret_cast<const float*>(a.xy + (size_t)i * a.xy_row + (size_t)k * a.xy_step);
            const double u = (double)px[0], v = (double)px[1];
            if (ftri_finite(u) && ftri_finite(v)) f(l, u, v);
        }
        // ftri_parent's rule with the window's own prev[] and nk() (LDS): one dependent global load per hop
        const int p = s.prevf[l];
        if (p < lo || p >= i) break;
        const int q = a.obs[(size_t)i * a.ocap + k].prev_kp;
        if ((uint32_t)q >= (uint32_t)s.nk[p - first]) break;
        i = p; k = q;
    }
}

// the 3 x 3 LDL^T of the damped V and its inverse Vi = (00, 01, 02, 11, 12, 22); false: a pivot failed
__device__ __forceinline__ void ba_solve3(double L10, double L20, double L21, double D0, double D1, double D2, double b0, double b1, double b2, double* x) {
    const double z0 = b0, z1 = b1 - L10 * z0, z2 = (b2 - L20 * z0) - L21 * z1;
    x[2] = z2 / D2; x[1] = z1 / D1 - L21 * x[2]; x[0] = (z0 / D0 - L10 * x[1]) - L20 * x[2];
}
__device__ __forceinline__ bool ba_invert3(const double* V, double lam1, double* Vi) {
    const double H00 = V[0] * lam1, H11 = V[3] * lam1, H22 = V[5] * lam1;
    const double D0 = H00, L10 = V[1] / D0, L20 = V[2] / D0;
    const double D1 = H11 - (L10 * L10) * D0;
    const double L21 = (V[4] - (L20 * L10) * D0) / D1;
    const double D2 = (H22 - (L20 * L20) * D0) - (L21 * L21) * D1;
    const bool ok = D0 > 0.0 && ftri_finite(D0) && D1 > 0.0 && ftri_finite(D1) && D2 > 0.0 && ftri_finite(D2);
    double c0[3], c1[3], c2[3];
    ba_solve3(L10, L20, L21, D0, D1, D2, 1.0, 0.0, 0.0, c0);
    ba_solve3(L10, L20, L21, D0, D1, D2, 0.0, 1.0, 0.0, c1);
    ba_solve3(L10, L20, L21, D0, D1, D2, 0.0, 0.0, 1.0, c2);
    Vi[0] = c0[0]; Vi[1] = c1[0]; Vi[2] = c2[0]; Vi[3] = c1[1]; Vi[4] = c2[1]; Vi[5] = c2[2];
    return ok;
}

// R <- C(w) R, t <- C(w) t + dt of the PnP refinement (p_update of pnp.hip)
__device__ __forceinline__ void ba_update(const double* P, const double* d, double* N) {
    const double h[3] = {0.5 * d[0], 0.5 * d[1], 0.5 * d[2]};
    const double hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2], s = 2.0 / (1.0 + hh);
    const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
    double Cm[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double k2 = i == j ? h[i] * h[j] - hh : h[i] * h[j];
            Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + s * (K[3 * i + j] + k2);
        }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) N[3 * i + j] = (Cm[3 * i] * P[j] + Cm[3 * i + 1] * P[3 + j]) + Cm[3 * i + 2] * P[6 + j];
        N[9 + i] = ((Cm[3 * i] * P[9] + Cm[3 * i + 1] * P[10]) + Cm[3 * i + 2] * P[11]) + d[3 + i];
    }
}

__device__ __forceinline__ void ba_centre(const double* P, double* c) {
    c[0] = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]); c[1] = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]);
    c[2] = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]);
}

struct BaWin { int first, last, own0, lo, R, NS; };                 // NS: the owned slots, frame-major rows of R

// slot s of the window -> (frame, keypoint); false past the frame's keypoints
__device__ __forceinline__ bool ba_slot(const BaWin& w, const BaShared& s, int slot, int* i, int* k) {
    if (slot >= w.NS) return false;
    *i = w.own0 + slot / w.R; *k = slot % w.R;
    return *k < s.nk[*i - w.first];
}

// X + dX of the point that ends in (i, k) for the step s.b at the state s.Pc (the point sits out: X)
__device__ __forceinline__ void ba_point_step(const FtriArgs& a, const BaShared& s, const BaWin& w, const BaK& K, double lam1, int i, int k,
                                              const double* X, double* Xn) {
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, Q[3] = {0, 0, 0};
    ba_walk(a, s, w.first, w.lo, i, k, [&](int l, double u, double v) {
        BaObs o; double ju[3], jv[3];
        ba_observe(K, s.Pc[l], X, u, v, o);
        ba_point_rows(o, s.Pc[l], ju, jv);
        V[0] = V[0] + o.w * (ju[0] * ju[0] + jv[0] * jv[0]); V[1] = V[1] + o.w * (ju[0] * ju[1] + jv[0] * jv[1]);
        V[2] = V[2] + o.w * (ju[0] * ju[2] + jv[0] * jv[2]); V[3] = V[3] + o.w * (ju[1] * ju[1] + jv[1] * jv[1]);
        V[4] = V[4] + o.w * (ju[1] * ju[2] + jv[1] * jv[2]); V[5] = V[5] + o.w * (ju[2] * ju[2] + jv[2] * jv[2]);
#pragma unroll
        for (int q = 0; q < 3; q++) g[q] = g[q] + o.w * (ju[q] * o.ru + jv[q] * o.rv);
        const int c = s.cidx[l];
        if (c >= 0) {
            double cu[6], cv[6];
            ba_cam_rows(o, cu, cv);
            const double* d = s.b + 6 * c;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double t = (o.w * (cu[0] * ju[q] + cv[0] * jv[q])) * d[0] + (o.w * (cu[1] * ju[q] + cv[1] * jv[q])) * d[1];
#pragma unroll
                for (int r = 2; r < 6; r++) t = t + (o.w * (cu[r] * ju[q] + cv[r] * jv[q])) * d[r];
                Q[q] = Q[q] + t;
            }
        }
    });
    double Vi[6];
    Xn[0] = X[0]; Xn[1] = X[1]; Xn[2] = X[2];
    if (!ba_invert3(V, lam1, Vi)) return;
    const double s0 = -g[0] - Q[0], s1 = -g[1] - Q[1], s2 = -g[2] - Q[2];
    Xn[0] = X[0] + ((Vi[0] * s0 + Vi[1] * s1) + Vi[2] * s2);
    Xn[1] = X[1] + ((Vi[1] * s0 + Vi[3] * s1) + Vi[4] * s2);
    Xn[2] = X[2] + ((Vi[2] * s0 + Vi[4] * s1) + Vi[5] * s2);
}

// the cost of the state (STEP: of the candidate s.Pn with X + dX) over the used points in slot order; every lane returns it
template <bool STEP> __device__ __forceinline__ double ba_cost(const BaArgs& A, BaShared& s, const BaWin& w, const BaK& K, double lam1) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int base = 0; base < w.NS; base += BA_BLOCK) {
        int i, k;
        const bool live = ba_slot(w, s, base + tid, &i, &k);
        const size_t e = live ? (size_t)i * A.t.ocap + k : 0;
        const bool used = live && A.flags[e] == VIS_BAP_USED;
        double c = 0.0;
        if (used) {
            const double X0[3] = {A.pts[e].X[0], A.pts[e].X[1], A.pts[e].X[2]};
            double X[3] = {X0[0], X0[1], X0[2]};
            if (STEP) ba_point_step(A.t, s, w, K, lam1, i, k, X0, X);
            ba_walk(A.t, s, w.first, w.lo, i, k, [&](int l, double u, double v) {
                BaObs o;
                ba_observe(K, STEP ? s.Pn[l] : s.Pc[l], X, u, v, o);
                c = c + o.term;
            });
        }
        s.u.cost[tid] = c; s.list[tid] = used ? 1 : 0;
        __syncthreads();
        if (tid == 0) for (int t = 0; t < BA_BLOCK; t++) if (s.list[t]) acc = acc + s.u.cost[t];
        __syncthreads();
    }
    if (tid == 0) s.bc[0] = acc;
    __syncthreads();
    acc = s.bc[0];
    __syncthreads();
    return acc;
}

// T, U, b, Tg of the state s.Pc: the used points of every chunk compacted in slot order, BA_BP staged at a time, every lane adding to its entries
__device__ __forceinline__ void ba_build(const BaArgs& A, BaShared& s, const BaWin& w, const BaK& K, double lam1, int F) {
    const int tid = threadIdx.x, N = 6 * F, NE = N * (N + 1) / 2;
    for (int e = tid; e < NE; e += BA_BLOCK) s.A[e] = 0.0;
    for (int e = tid; e < F * 21; e += BA_BLOCK) s.U[e / 21][e % 21] = 0.0;
    for (int e = tid; e < N; e += BA_BLOCK) { s.b[e] = 0.0; s.Tg[e] = 0.0; }
    const int n_item = (F * (F + 1) / 2) * 6, n_uitem = F * 33;
    for (int base = 0; base < w.NS; base += BA_BLOCK) {
        int i, k;
        const bool live = ba_slot(w, s, base + tid, &i, &k);
        const bool used = live && A.flags[(size_t)i * A.t.ocap + k] == VIS_BAP_USED;
        const unsigned long long bal = __ballot(used);
        if ((tid & 63) == 0) s.wcnt[tid >> 6] = __popcll(bal);
        __syncthreads();                                           // (also: the entry lanes of the chunk before are done with the stage)
        int pos = __popcll(bal & ((1ull << (tid & 63)) - 1ull)), np = 0;
        for (int q = 0; q < BA_BLOCK / 64; q++) { if (q < (tid >> 6)) pos += s.wcnt[q]; np += s.wcnt[q]; }
        if (used) s.list[pos] = base + tid;
        __syncthreads();
        for (int sb = 0; sb < np; sb += BA_BP) {
            const int nb = min(BA_BP, np - sb);
            if (tid < nb) {
                const int slot = s.list[sb + tid], pi = w.own0 + slot / w.R, pk = slot % w.R;
                const vis_ba_point* pt = A.pts + (size_t)pi * A.t.ocap + pk;
                const double X[3] = {pt->X[0], pt->X[1], pt->X[2]};
                double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
                int nv = 0;
#pragma unroll
                for (int c = 0; c < BA_MAXC; c++) s.vpos[tid][c] = -1;
                ba_walk(A.t, s, w.first, w.lo, pi, pk, [&](int l, double u, double v) {
                    BaObs o; double ju[3], jv[3];
                    ba_observe(K, s.Pc[l], X, u, v, o);
                    ba_point_rows(o, s.Pc[l], ju, jv);
                    V[0] = V[0] + o.w * (ju[0] * ju[0] + jv[0] * jv[0]); V[1] = V[1] + o.w * (ju[0] * ju[1] + jv[0] * jv[1]);
                    V[2] = V[2] + o.w * (ju[0] * ju[2] + jv[0] * jv[2]); V[3] = V[3] + o.w * (ju[1] * ju[1] + jv[1] * jv[1]);
                    V[4] = V[4] + o.w * (ju[1] * ju[2] + jv[1] * jv[2]); V[5] = V[5] + o.w * (ju[2] * ju[2] + jv[2] * jv[2]);
#pragma unroll
                    for (int q = 0; q < 3; q++) g[q] = g[q] + o.w * (ju[q] * o.ru + jv[q] * o.rv);
                    double* ob = s.u.st.ob[tid][nv];
                    ob[0] = o.U; ob[1] = o.V; ob[2] = o.W; ob[3] = o.iw; ob[4] = o.w; ob[5] = o.ru; ob[6] = o.rv;
                    s.vfr[tid][nv] = (signed char)l;
                    if (s.cidx[l] >= 0) s.vpos[tid][s.cidx[l]] = (signed char)nv;
                    nv++;
                });
                double Vi[6];
                s.okp[tid] = ba_invert3(V, lam1, Vi) ? 1 : 0;
#pragma unroll
                for (int q = 0; q < 6; q++) s.u.st.Vi[tid][q] = Vi[q];
#pragma unroll
                for (int q = 0; q < 3; q++) s.u.st.g[tid][q] = g[q];
                s.nv[tid] = nv;
            }
            __syncthreads();
            // the Schur items: (camera pair c1 <= c2, a) -> the six entries T[6 c1 + a][6 c2 + b], row <= column; W1's row and Y once per point
            for (int it = tid; it < n_item; it += BA_BLOCK) {
                const int pair = it / 6, ea = it % 6;
                int c2 = 0;
                while ((c2 + 1) * (c2 + 2) / 2 <= pair) c2++;
                const int c1 = pair - c2 * (c2 + 1) / 2, row = 6 * c1 + ea;
                double acc[6];
#pragma unroll
                for (int eb = 0; eb < 6; eb++) { const int col = 6 * c2 + eb; acc[eb] = col >= row ? s.A[col * (col + 1) / 2 + row] : 0.0; }
                for (int p = 0; p < nb; p++) {
                    if (!s.okp[p]) continue;
                    const int v1 = s.vpos[p][c1], v2 = s.vpos[p][c2];
                    if (v1 < 0 || v2 < 0) continue;
                    BaObs o;
                    double ju[3], jv[3], cu[6], cv[6], W1[3];
                    const double* ob = s.u.st.ob[p][v1];
                    o.U = ob[0]; o.V = ob[1]; o.W = ob[2]; o.iw = ob[3]; o.w = ob[4];
                    o.un = o.U * o.iw; o.vn = o.V * o.iw; o.fu = K.fx * o.iw; o.fv = K.fy * o.iw;
                    ba_point_rows(o, s.Pc[s.vfr[p][v1]], ju, jv);
                    ba_cam_rows(o, cu, cv);
                    const double cua = ea == 0 ? cu[0] : ea == 1 ? cu[1] : ea == 2 ? cu[2] : ea == 3 ? cu[3] : ea == 4 ? cu[4] : cu[5];
                    const double cva = ea == 0 ? cv[0] : ea == 1 ? cv[1] : ea == 2 ? cv[2] : ea == 3 ? cv[3] : ea == 4 ? cv[4] : cv[5];
#pragma unroll
                    for (int q = 0; q < 3; q++) W1[q] = o.w * (cua * ju[q] + cva * jv[q]);
                    const double* Vi = s.u.st.Vi[p];
                    const double Y0 = (W1[0] * Vi[0] + W1[1] * Vi[1]) + W1[2] * Vi[2], Y1 = (W1[0] * Vi[1] + W1[1] * Vi[3]) + W1[2] * Vi[4],
                                 Y2 = (W1[0] * Vi[2] + W1[1] * Vi[4]) + W1[2] * Vi[5];
                    ob = s.u.st.ob[p][v2];
                    o.U = ob[0]; o.V = ob[1]; o.W = ob[2]; o.iw = ob[3]; o.w = ob[4];
                    o.un = o.U * o.iw; o.vn = o.V * o.iw; o.fu = K.fx * o.iw; o.fv = K.fy * o.iw;
                    ba_point_rows(o, s.Pc[s.vfr[p][v2]], ju, jv);
                    ba_cam_rows(o, cu, cv);
#pragma unroll
                    for (int eb = 0; eb < 6; eb++) {
                        const double W20 = o.w * (cu[eb] * ju[0] + cv[eb] * jv[0]), W21 = o.w * (cu[eb] * ju[1] + cv[eb] * jv[1]),
                                     W22 = o.w * (cu[eb] * ju[2] + cv[eb] * jv[2]);
                        acc[eb] = acc[eb] + ((Y0 * W20 + Y1 * W21) + Y2 * W22);
                    }
                }
#pragma unroll
                for (int eb = 0; eb < 6; eb++) { const int col = 6 * c2 + eb; if (col >= row) s.A[col * (col + 1) / 2 + row] = acc[eb]; }
            }
            // the camera items: U (21), b (6), Tg (6) of every free camera
            for (int it = tid; it < n_uitem; it += BA_BLOCK) {
                const int c = it / 33, ent = it % 33;
                int ea = 0, eb = 0;
                if (ent < 21) { int r = ent; while (r >= 6 - ea) { r -= 6 - ea; ea++; } eb = ea + r; }
                else ea = (ent - 21) % 6;
                double* dst = ent < 21 ? &s.U[c][ent] : ent < 27 ? &s.b[6 * c + ea] : &s.Tg[6 * c + ea];
                double acc = *dst;
                for (int p = 0; p < nb; p++) {
                    if (!s.okp[p]) continue;
                    const int v1 = s.vpos[p][c];
                    if (v1 < 0) continue;
                    const double* ob = s.u.st.ob[p][v1];
                    BaObs o;
                    o.U = ob[0]; o.V = ob[1]; o.W = ob[2]; o.iw = ob[3]; o.w = ob[4]; o.ru = ob[5]; o.rv = ob[6];
                    o.un = o.U * o.iw; o.vn = o.V * o.iw; o.fu = K.fx * o.iw; o.fv = K.fy * o.iw;
                    double cua, cva;
                    ba_cam_entry(o, ea, cua, cva);
                    if (ent < 21) { double cub, cvb; ba_cam_entry(o, eb, cub, cvb); acc = acc + o.w * (cua * cub + cva * cvb); }
                    else if (ent < 27) acc = acc + o.w * (cua * o.ru + cva * o.rv);
                    else {
                        double ju[3], jv[3], W1[3];
                        ba_point_rows(o, s.Pc[s.vfr[p][v1]], ju, jv);
#pragma unroll
                        for (int q = 0; q < 3; q++) W1[q] = o.w * (cua * ju[q] + cva * jv[q]);
                        const double* Vi = s.u.st.Vi[p];
                        const double* g = s.u.st.g[p];
                        const double Y0 = (W1[0] * Vi[0] + W1[1] * Vi[1]) + W1[2] * Vi[2], Y1 = (W1[0] * Vi[1] + W1[1] * Vi[3]) + W1[2] * Vi[4],
                                     Y2 = (W1[0] * Vi[2] + W1[1] * Vi[4]) + W1[2] * Vi[5];
                        acc = acc + ((Y0 * g[0] + Y1 * g[1]) + Y2 * g[2]);
                    }
                }
                *dst = acc;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}

// A = Ud - T, rhs, LDL^T without pivoting, the step into s.b; false (for every lane): a pivot failed
__device__ __forceinline__ bool ba_solve(BaShared& s, double lam1, int F) {
    const int tid = threadIdx.x, N = 6 * F, NE = N * (N + 1) / 2;
    for (int e = tid; e < NE; e += BA_BLOCK) {
        int col = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
        while ((col + 1) * (col + 2) / 2 <= e) col++;
        while (col * (col + 1) / 2 > e) col--;
        const int row = e - col * (col + 1) / 2;
        double ud = 0.0;
        if (row / 6 == col / 6) {
            const int a = row % 6, b = col % 6;
            ud = s.U[col / 6][a * 6 - a * (a - 1) / 2 + (b - a)];
            if (row == col) ud = ud * lam1;
        }
        s.A[e] = ud - s.A[e];
    }
    for (int e = tid; e < N; e += BA_BLOCK) s.z[e] = -(s.b[e] - s.Tg[e]);
    bool ok = true;
    for (int j = 0; j < N; j++) {
        __syncthreads();
        const double d = s.A[j * (j + 1) / 2 + j];
        if (!(d > 0.0) || !ftri_finite(d)) { ok = false; break; }   // (uniform: every lane reads the same element)
        if (tid == 0) s.D[j] = d;
        for (int i = j + 1 + tid; i < N; i += BA_BLOCK) s.A[i * (i + 1) / 2 + j] = s.A[i * (i + 1) / 2 + j] / d;
        __syncthreads();
        for (int i = j + 1 + (tid >> 4); i < N; i += BA_BLOCK / 16) {
            const double Lij = s.A[i * (i + 1) / 2 + j];
            for (int k = j + 1 + (tid & 15); k <= i; k += 16) s.A[i * (i + 1) / 2 + k] = s.A[i * (i + 1) / 2 + k] - (Lij * s.A[k * (k + 1) / 2 + j]) * d;
        }
    }
    __syncthreads();
    if (!ok) return false;
    for (int c = 0; c < N; c++) {
        const double zc = s.z[c];
        __syncthreads();
        for (int i = c + 1 + tid; i < N; i += BA_BLOCK) s.z[i] = s.z[i] - s.A[i * (i + 1) / 2 + c] * zc;
        __syncthreads();
    }
    if (tid == 0)
        for (int i = N - 1; i >= 0; i--) {
            double v = s.z[i] / s.D[i];
            for (int c = i + 1; c < N; c++) v = v - s.A[c * (c + 1) / 2 + i] * s.b[c];
            s.b[i] = v;
        }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(BA_BLOCK) void k_ba_window(BaArgs A) {
    __shared__ BaShared s;
    const int tid = threadIdx.x, j = blockIdx.x;
    const vis_ba_params& bp = A.bp;
    BaWin w;
    w.first = j * bp.stride; w.last = min(w.first + bp.stride, A.t.n - 1); w.own0 = w.first + (j > 0 ? 1 : 0); w.R = A.t.R;
    const int nf = w.last - w.first + 1;
    w.NS = (w.last - w.own0 + 1) * w.R;
    const BaK K = {A.t.fx, A.t.fy, A.t.cx, A.t.cy, bp.huber_px};
    if (tid < nf) {
        const double* p = A.poses + (size_t)(w.first + tid) * 12;
        bool fin = true, zero = true;
#pragma unroll
        for (int q = 0; q < 12; q++) { const double v = p[q]; s.Pin[tid][q] = s.Pc[tid][q] = s.Pn[tid][q] = v; fin = fin && ftri_finite(v); if (q < 9) zero = zero && v == 0.0; }
        s.posed[tid] = fin && !zero ? 1 : 0;
        s.nk[tid] = ft_count(A.t.fr, w.first + tid, w.R);
        s.prevf[tid] = ft_prev(A.t.fr, w.first + tid);
    }
    if (tid < 2) s.cnt[tid] = 0;
    __syncthreads();
    int anchor = -1, F = 0, lastf = -1;                             // (every lane: 17 LDS reads)
    for (int l = 0; l < nf; l++) if (s.posed[l]) { if (anchor < 0) anchor = w.first + l; else { F++; lastf = l; } }
    if (tid < nf) {
        int c = -1;
        if (s.posed[tid] && w.first + tid > anchor) { c = 0; for (int l = anchor - w.first + 1; l < tid; l++) c += s.posed[l]; }
        s.cidx[tid] = c;
    }
    w.lo = anchor >= 0 ? anchor : w.first;
    // the owned slots: cleared, the continued ones marked, the ends triangulated under the input poses
    for (int base = 0; base < w.NS; base += BA_BLOCK) {
        int i, k;
        if (ba_slot(w, s, base + tid, &i, &k)) A.flags[(size_t)i * A.t.ocap + k] = 0;
    }
    __syncthreads();
    for (int base = 0; base < w.NS; base += BA_BLOCK) {
        int i, k, pk;
        if (!ba_slot(w, s, base + tid, &i, &k)) continue;
        const int p = ftri_parent(A.t, w.own0, i, k, &pk);
        if (p >= 0) A.flags[(size_t)p * A.t.ocap + pk] = BA_MARK;   // (several writers can only write the same byte)
    }
    __syncthreads();
    for (int base = 0; base < w.NS; base += BA_BLOCK) {
        int i, k;
        if (!ba_slot(w, s, base + tid, &i, &k)) continue;
        const size_t e = (size_t)i * A.t.ocap + k;
        vis_ba_point r;
        r.X[0] = r.X[1] = r.X[2] = 0.0; r.rms0_px = r.rms1_px = 0.f; r.n_views = 0; r.flags = 0;
        if (A.flags[e] != BA_MARK) {
            vis_ftrack_point pt;
            pt.X[0] = pt.X[1] = pt.X[2] = 0.0; pt.rms_reproj_px = pt.parallax_cos = 0.f; pt.n_views = 0; pt.flags = 0;
            ftri_point(A.t, w.lo, i, k, pt);
            r.n_views = pt.n_views;
            if (pt.flags & VIS_FTP_FEW) r.flags = VIS_BAP_FEW;
            else if ((pt.flags & VIS_FTP_SINGULAR) || !(pt.flags & VIS_FTP_FRONT) || !(pt.flags & VIS_FTP_REPROJ_OK)) { r.flags = VIS_BAP_INIT_REJECTED; r.rms0_px = pt.rms_reproj_px; }
            else {
                r.flags = VIS_BAP_USED; r.X[0] = pt.X[0]; r.X[1] = pt.X[1]; r.X[2] = pt.X[2]; r.rms0_px = r.rms1_px = pt.rms_reproj_px;
                atomicAdd(&s.cnt[0], 1); atomicAdd(&s.cnt[1], pt.n_views);
            }
        }
        A.pts[e] = r; A.flags[e] = (uint8_t)r.flags;
    }
    __syncthreads();
    const int n_points = s.cnt[0], n_obs = s.cnt[1];
    double lam = bp.lambda0, scale = 1.0;
    double cur = ba_cost<false>(A, s, w, K, 1.0);
    const double cost0 = cur;
    int nacc = 0, nrej = 0, n_lin = 0, wflags = VIS_BA_FEW;
    if (F > 0 && n_points >= bp.min_points) {
        wflags = VIS_BA_REFINED;
        n_lin = bp.lm_iters;
        for (int it = 0; it < bp.lm_iters; it++) {
            const double lam1 = 1.0 + lam;
            ba_build(A, s, w, K, lam1, F);
            bool accept = false;
            double c = 0.0;
            if (ba_solve(s, lam1, F)) {
                if (tid < nf) {
                    if (s.cidx[tid] >= 0) ba_update(s.Pc[tid], s.b + 6 * s.cidx[tid], s.Pn[tid]);
                    else for (int q = 0; q < 12; q++) s.Pn[tid][q] = s.Pc[tid][q];
                }
                __syncthreads();
                c = ba_cost<true>(A, s, w, K, lam1);
                accept = ftri_finite(c) && c < cur;
            }
            if (accept) {
                for (int base = 0; base < w.NS; base += BA_BLOCK) {
                    int i, k;
                    if (!ba_slot(w, s, base + tid, &i, &k)) continue;
                    const size_t e = (size_t)i * A.t.ocap + k;
                    if (A.flags[e] != VIS_BAP_USED) continue;
                    const double X[3] = {A.pts[e].X[0], A.pts[e].X[1], A.pts[e].X[2]};
                    double Xn[3];
                    ba_point_step(A.t, s, w, K, lam1, i, k, X, Xn);
                    A.pts[e].X[0] = Xn[0]; A.pts[e].X[1] = Xn[1]; A.pts[e].X[2] = Xn[2];
                }
                __syncthreads();
                if (tid < nf) for (int q = 0; q < 12; q++) s.Pc[tid][q] = s.Pn[tid][q];
                cur = c; nacc++;
                const double l = lam / 10.0;
                lam = l > 1e-12 ? l : 1e-12;
            } else {
                nrej++;
                const double l = 10.0 * lam;
                lam = l < 1e12 ? l : 1e12;
            }
            __syncthreads();
        }
        // the scale gauge, rms1_px, the scaled points
        double ca[3] = {0, 0, 0};
        bool apply = false;
        if (nacc > 0) {
            double cin[3], cout[3];
            ba_centre(s.Pin[anchor - w.first], ca); ba_centre(s.Pin[lastf], cin); ba_centre(s.Pc[lastf], cout);
            const double di[3] = {cin[0] - ca[0], cin[1] - ca[1], cin[2] - ca[2]}, dq[3] = {cout[0] - ca[0], cout[1] - ca[1], cout[2] - ca[2]};
            const double sc = sqrt((di[0] * di[0] + di[1] * di[1]) + di[2] * di[2]) / sqrt((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]);
            if (ftri_finite(sc) && sc > 0.0) { scale = sc; apply = true; } else wflags |= VIS_BA_NO_SCALE;
        }
        for (int base = 0; base < w.NS; base += BA_BLOCK) {
            int i, k;
            if (!ba_slot(w, s, base + tid, &i, &k)) continue;
            const size_t e = (size_t)i * A.t.ocap + k;
            if (A.flags[e] != VIS_BAP_USED) continue;
            double X[3] = {A.pts[e].X[0], A.pts[e].X[1], A.pts[e].X[2]};
            double s2 = 0.0; int nv = 0;
            ba_walk(A.t, s, w.first, w.lo, i, k, [&](int l, double u, double v) {
                BaObs o;
                ba_observe(K, s.Pc[l], X, u, v, o);
                s2 = s2 + o.e2; nv++;
            });
            A.pts[e].rms1_px = (float)sqrt(s2 / (double)nv);
            if (apply) {
#pragma unroll
                for (int q = 0; q < 3; q++) A.pts[e].X[q] = ca[q] + scale * (X[q] - ca[q]);
            }
        }
        __syncthreads();                                           // (every walk at the final poses is done)
        if (apply && tid < nf && s.cidx[tid] >= 0) {
            double* P = s.Pc[tid];
            double c[3];
            ba_centre(P, c);
#pragma unroll
            for (int q = 0; q < 3; q++) c[q] = ca[q] + scale * (c[q] - ca[q]);
#pragma unroll
            for (int q = 0; q < 3; q++) P[9 + q] = -((P[3 * q] * c[0] + P[3 * q + 1] * c[1]) + P[3 * q + 2] * c[2]);
        }
    }
    // the window's poses of its free frames (the stitch moves them into the output frame), the record
    if (tid < nf && s.cidx[tid] >= 0) {
        double* o = A.poses_out + (size_t)(w.first + tid) * 12;
#pragma unroll
        for (int q = 0; q < 12; q++) o[q] = s.Pc[tid][q];
    }
    if (tid == 0) {
        vis_ba_window r;
        r.first = w.first; r.last = w.last; r.anchor = anchor; r.n_free = F; r.n_points = n_points; r.n_obs = n_obs; r.n_lin = n_lin;
        r.n_accepted = nacc; r.n_rejected = nrej; r.flags = wflags; r.reserved_[0] = r.reserved_[1] = 0;
        r.cost0 = cost0; r.cost1 = cur; r.lambda = lam; r.scale = scale;
        A.win[j] = r;
    }
}

__device__ __forceinline__ double ba_dot(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ __forceinline__ bool ba_same_bytes(const double* a, const double* b) {
    bool same = true;
#pragma unroll
    for (int q = 0; q < 12; q++) same = same && __double_as_longlong(a[q]) == __double_as_longlong(b[q]);
    return same;
}
__device__ __forceinline__ bool ba_has_pose(const double* p) {
    bool fin = true, zero = true;
#pragma unroll
    for (int q = 0; q < 12; q++) { fin = fin && ftri_finite(p[q]); if (q < 9) zero = zero && p[q] == 0.0; }
    return fin && !zero;
}

// one workgroup: the windows in order, a lane per frame of the window
__global__ __launch_bounds__(64) void k_ba_stitch(int nwin, const double* __restrict__ poses, double* poses_out, vis_ba_window* win) {
    const int tid = threadIdx.x;
    for (int j = 0; j < nwin; j++) {
        __syncthreads();                                           // (the shared frame of window j - 1 is written)
        const int first = win[j].first, last = win[j].last, anchor = win[j].anchor;
        if (anchor < 0) continue;
        const bool restart = j > 0 && anchor != first;
        if (restart && tid == 0) win[j].flags |= VIS_BA_RESTART;
        const double* Ai = poses + (size_t)anchor * 12;
        double Ao[12];
#pragma unroll
        for (int q = 0; q < 12; q++) Ao[q] = (j == 0 || restart) ? Ai[q] : poses_out[(size_t)anchor * 12 + q];
        const int i = anchor + 1 + tid;
        if (ba_same_bytes(Ai, Ao) || i > last || !ba_has_pose(poses + (size_t)i * 12)) continue;   // (the barrier above is reached by every lane)
        double* o = poses_out + (size_t)i * 12;
        double Rr[9], tr[3], N[12];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) Rr[3 * a + b] = ba_dot(o[3 * a], o[3 * a + 1], o[3 * a + 2], Ai[3 * b], Ai[3 * b + 1], Ai[3 * b + 2]);
#pragma unroll
        for (int a = 0; a < 3; a++) tr[a] = o[9 + a] - ba_dot(Rr[3 * a], Rr[3 * a + 1], Rr[3 * a + 2], Ai[9], Ai[10], Ai[11]);
        bool fin = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++) N[3 * a + b] = ba_dot(Rr[3 * a], Rr[3 * a + 1], Rr[3 * a + 2], Ao[b], Ao[3 + b], Ao[6 + b]);
            N[9 + a] = ba_dot(Rr[3 * a], Rr[3 * a + 1], Rr[3 * a + 2], Ao[9], Ao[10], Ao[11]) + tr[a];
        }
#pragma unroll
        for (int q = 0; q < 12; q++) fin = fin && ftri_finite(N[q]);
#pragma unroll
        for (int q = 0; q < 12; q++) o[q] = fin ? N[q] : poses[(size_t)i * 12 + q];
    }
}

// one lane per slot: the used points of a window whose anchor moved go to the output frame
__global__ __launch_bounds__(BA_BLOCK) void k_ba_points(int R, FtFrames fr, int ocap, int stride, const double* __restrict__ poses,
                                                        const double* __restrict__ poses_out, const vis_ba_window* __restrict__ win,
                                                        vis_ba_point* __restrict__ pts, const uint8_t* __restrict__ flags) {
    const int i = blockIdx.y, k = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (k >= ft_count(fr, i, R)) return;
    const size_t e = (size_t)i * ocap + k;
    if (flags[e] != VIS_BAP_USED) return;
    const int j = i == 0 ? 0 : (i - 1) / stride;
    const int anchor = win[j].anchor;
    if (j == 0 || anchor < 0 || (win[j].flags & VIS_BA_RESTART)) return;
    const double* Ai = poses + (size_t)anchor * 12;
    const double* Ao = poses_out + (size_t)anchor * 12;
    if (ba_same_bytes(Ai, Ao)) return;
    const double X[3] = {pts[e].X[0], pts[e].X[1], pts[e].X[2]};
    double y[3];
#pragma unroll
    for (int a = 0; a < 3; a++) y[a] = (ba_dot(Ai[3 * a], Ai[3 * a + 1], Ai[3 * a + 2], X[0], X[1], X[2]) + Ai[9 + a]) - Ao[9 + a];
    double Z[3];
#pragma unroll
    for (int a = 0; a < 3; a++) Z[a] = ba_dot(Ao[a], Ao[3 + a], Ao[6 + a], y[0], y[1], y[2]);
    if (!ftri_finite(Z[0]) || !ftri_finite(Z[1]) || !ftri_finite(Z[2])) return;      // (an extreme A_out: the point stays in its window's frame)
#pragma unroll
    for (int a = 0; a < 3; a++) pts[e].X[a] = Z[a];
}

int ba_run(vis_ctx* ctx, const vis_ba_params* bp, int n, int R, FtFrames fr, const vis_ftrack_obs* d_obs, int ocap, const void* d_xy, size_t xy_row,
           int xy_step, const double* d_poses, double* d_poses_out, vis_ba_window* d_windows, vis_ba_point* d_points, uint8_t* d_flags) {
    if (n < 1) return VIS_OK;
    if (R < 0 || R > ocap || (size_t)n * (size_t)ocap > ((size_t)1 << 28)) return VIS_E_INVALID;
    // every frame starts from its input bytes: frames without a pose and the anchors keep them
    HIPCHK(ctx, hipMemcpyAsync(d_poses_out, d_poses, (size_t)n * 12 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    const int nwin = n > 1 ? (n - 1 + bp->stride - 1) / bp->stride : 0;
    if (nwin == 0) return VIS_OK;
    BaArgs A;
    A.t.n = n; A.t.R = R; A.t.ocap = ocap; A.t.fr = fr; A.t.obs = d_obs; A.t.xy = (const char*)d_xy; A.t.xy_row = xy_row; A.t.xy_step = xy_step;
    A.t.poses = d_poses; A.t.max_views = BA_MAXF; A.t.min_views = bp->min_views; A.t.gn_iters = bp->tri_gn_iters;
    A.t.thr2 = bp->init_reproj_px * bp->init_reproj_px; A.t.max_cos = 1.0;
    A.t.fx = ctx->p.fx; A.t.fy = ctx->p.fy; A.t.cx = ctx->p.cx; A.t.cy = ctx->p.cy;
    A.bp = *bp; A.poses = d_poses; A.poses_out = d_poses_out; A.win = d_windows; A.pts = d_points; A.flags = d_flags;
    hipLaunchKernelGGL(k_ba_window, dim3(nwin), dim3(BA_BLOCK), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ba_stitch, dim3(1), dim3(64), 0, ctx->stream, nwin, d_poses, d_poses_out, d_windows);
    HIPCHK(ctx, hipGetLastError());
    if (R > 0) {
        hipLaunchKernelGGL(k_ba_points, dim3((R + BA_BLOCK - 1) / BA_BLOCK, n), dim3(BA_BLOCK), 0, ctx->stream, R, fr, ocap, bp->stride, d_poses, d_poses_out,
                           d_windows, d_points, d_flags);
        HIPCHK(ctx, hipGetLastError());
    }
    return VIS_OK;
}
