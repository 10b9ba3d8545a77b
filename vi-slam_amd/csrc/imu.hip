// imu.hip -- IMU preintegration on the device: one delta per frame interval (k_imu_intervals, a lane per interval, a serial loop over its
// sub-steps) and the pair deltas by binary lifting (k_imu_pairs: ONE launch of one workgroup builds the levels T_k[i] = T_{k-1}[i - 2^{k-1}] o T_{k-1}[i]
// with a barrier between them, composes every pair from the set bits of its length, and writes the records, the camera-frame rotations and the
// carry).  include/vislam_hip.h has the contract operation for operation, tests/imu_ref.py restates it.  Double arithmetic, + - * / only.
// A table entry is 26 eight-byte slots (25 doubles, n_steps and flags packed into the last), structure of arrays: slot s of entry i of level k
// is ws[((size_t)k * 26 + s) * n + i], so consecutive frames read consecutive addresses.  Levels are separate arrays: a round reads level k - 1 and
// writes level k, nothing is read and written in one round, one barrier a round suffices.
// The Jacobian variants (k_imu_intervals<true>, k_imu_pairs<true>: vis_imu_preintegrate_jac_rows, vis_batch_imu_jac) are separate instantiations with a
// table of their own of 62 slots: the 26 above, then Jvg, Jva, Jpg, Jpa (9 doubles each); the Jacobian flags ride in bits 16 and up of the flags half
// of slot 25 (a table entry's delta flags come from intervals alone and stay below bit 9).  A composition folds one block at a time into the
// accumulator: two whole entries are never held.  k_imu_correct applies a bias step to the records, a lane per frame.
// The covariance variants (k_imu_cov_intervals, k_imu_cov_pairs: vis_imu_preintegrate_cov_rows, vis_batch_imu_cov) share the kernels' bodies
// (imu_intervals_body, imu_pairs_body) and carry the 9 x 9 covariance of (dphi, dv, dp) as six 3 x 3 blocks in a table of 71 slots: the 26, then
// A (6), B (9), C (6), D (9), E (9), F (6); the covariance flags ride where the Jacobian flags do.
#include "vis_internal.h"
#include <cmath>

#define IMU_BLOCK 256
#define IMU_IV_BLOCK 64

struct ImuDelta { double R[9], v[3], p[3], dt, J[9]; int n_steps, flags; };
struct ImuJac { double vg[9], va[9], pg[9], pa[9]; int flags; };
struct ImuNoJac {};
template <bool JAC> struct ImuJacOf { typedef ImuNoJac type; };
template <> struct ImuJacOf<true> { typedef ImuJac type; };
// what the Jacobian variants read and write beside the delta's rows: the carried open delta's Jacobians, the rows, the carry's
struct ImuJacIO { const vis_imu_bias_jac* cin; vis_imu_bias_jac* rows; vis_imu_bias_jac* cout; };
// the covariance of (dphi, dv, dp) by 3 x 3 blocks: A phi-phi, C v-v, F p-p (upper triangles 00 01 02 11 12 22), B v-phi, D p-phi, E p-v (full, row-major);
// sg2, sa2: the squared densities, carried beside the accumulator so that the sub-step's hook needs no further argument
struct ImuCov { double A[6], B[9], C[6], D[9], E[9], F[6]; int flags; double sg2, sa2; };
struct ImuCovIO { const vis_imu_cov* cin; vis_imu_cov* rows; vis_imu_cov* cout; };
#define IMU_VOID_FLAGS (VIS_IMU_NO_PAIR | VIS_IMU_NO_CARRY | VIS_IMU_NO_START | VIS_IMU_NONFINITE)

__device__ __forceinline__ bool imu_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf
__device__ __forceinline__ int imu_prev(const FtFrames& fr, int i) {
    const int p = fr.prev ? fr.prev[i] : (i > 0 ? i - 1 : (fr.pair0 ? VIS_KF_CARRIED : VIS_KF_FIRST));
    if (p >= 0) return p < i ? p : VIS_KF_FIRST;
    return p == VIS_KF_CARRIED || p == VIS_KF_NOT_SAVED ? p : VIS_KF_FIRST;
}
__device__ __forceinline__ void imu_identity(ImuDelta& d) {
#pragma unroll
    for (int k = 0; k < 9; k++) { d.R[k] = (k & 3) == 0 ? 1.0 : 0.0; d.J[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 3; k++) d.v[k] = d.p[k] = 0.0;
    d.dt = 0.0; d.n_steps = 0; d.flags = 0;
}
__device__ __forceinline__ void imu_mul(const double* A, const double* B, double* M) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void imu_tmul(const double* A, const double* B, double* M) {       // A^T B
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
__device__ __forceinline__ void imu_mulv(const double* A, const double* x, double* y) {
#pragma unroll
    for (int r = 0; r < 3; r++) y[r] = (A[3 * r] * x[0] + A[3 * r + 1] * x[1]) + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ bool imu_all_finite(const ImuDelta& d) {
    bool fin = imu_finite(d.dt);
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && imu_finite(d.R[k]) && imu_finite(d.J[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && imu_finite(d.v[k]) && imu_finite(d.p[k]);
    return fin;
}
// the identity with dt (0 when not finite), n_steps and flags kept, and VIS_IMU_NONFINITE
__device__ __forceinline__ void imu_void(ImuDelta& d) {
    const double dt = imu_finite(d.dt) ? d.dt : 0.0;
    const int ns = d.n_steps, fl = d.flags | VIS_IMU_NONFINITE;
    imu_identity(d);
    d.dt = dt; d.n_steps = ns; d.flags = fl;
}
// X o Y, X the earlier
__device__ __forceinline__ void imu_compose(const ImuDelta& X, const ImuDelta& Y, ImuDelta& O) {
    double Rv[3], Rp[3], M[9];
    imu_mul(X.R, Y.R, O.R);
    imu_mulv(X.R, Y.v, Rv);
    imu_mulv(X.R, Y.p, Rp);
#pragma unroll
    for (int r = 0; r < 3; r++) { O.v[r] = X.v[r] + Rv[r]; O.p[r] = (X.p[r] + X.v[r] * Y.dt) + Rp[r]; }
    O.dt = X.dt + Y.dt;
    imu_tmul(Y.R, X.J, M);
#pragma unroll
    for (int k = 0; k < 9; k++) O.J[k] = M[k] + Y.J[k];
    O.n_steps = X.n_steps + Y.n_steps; O.flags = X.flags | Y.flags;
    if (!imu_all_finite(O)) imu_void(O);
}

// ---- the bias Jacobians of v and p
__device__ __forceinline__ void imu_jac_zero(ImuJac& q) {
#pragma unroll
    for (int k = 0; k < 9; k++) q.vg[k] = q.va[k] = q.pg[k] = q.pa[k] = 0.0;
}
__device__ __forceinline__ void imu_jac_zero(ImuNoJac&) {}
__device__ __forceinline__ void imu_skmul(const double* u, const double* M, double* S) {      // [u]x M
#pragma unroll
    for (int c = 0; c < 3; c++) {
        S[c] = u[1] * M[6 + c] - u[2] * M[3 + c];
        S[3 + c] = u[2] * M[c] - u[0] * M[6 + c];
        S[6 + c] = u[0] * M[3 + c] - u[1] * M[c];
    }
}
// the rule every Jacobian record ends on: zero beside a voided delta or a flagged record; not finite beside a finite delta: zero and flagged
__device__ __forceinline__ void imu_jac_settle(int dflags, ImuJac& q) {
    bool zero = (dflags & IMU_VOID_FLAGS) || (q.flags & VIS_IMU_JAC_NONFINITE);
    if (!zero) {
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; k++) fin = fin && imu_finite(q.vg[k]) && imu_finite(q.va[k]) && imu_finite(q.pg[k]) && imu_finite(q.pa[k]);
        if (!fin) { q.flags |= VIS_IMU_JAC_NONFINITE; zero = true; }
    }
    if (zero) imu_jac_zero(q);
}
__device__ __forceinline__ void imu_jac_settle(int, ImuNoJac&) {}
// the Jacobians of X o Y folded into q (in: Y's, out: the composition's), one block at a time; X's blocks come through ldx(block, M) (0 Jvg, 1 Jva, 2 Jpg,
// 3 Jpa), Y is the delta BEFORE the composition and oflags the composed delta's flags
template <class LoadX> __device__ __forceinline__ void imu_jac_fold(const ImuDelta& X, int xflags, LoadX ldx, const ImuDelta& Y, int oflags, ImuJac& q) {
    double S[9], W[9], Xv[9], Xp[9], M[9];
    q.flags |= xflags;
    ldx(3, Xp); ldx(1, Xv);
    imu_mul(X.R, q.pa, M);
#pragma unroll
    for (int k = 0; k < 9; k++) q.pa[k] = (Xp[k] + Xv[k] * Y.dt) + M[k];
    imu_mul(X.R, q.va, M);
#pragma unroll
    for (int k = 0; k < 9; k++) q.va[k] = Xv[k] + M[k];
    ldx(2, Xp); ldx(0, Xv);
    imu_skmul(Y.p, X.J, S); imu_mul(X.R, S, W);
    imu_mul(X.R, q.pg, M);
#pragma unroll
    for (int k = 0; k < 9; k++) q.pg[k] = ((Xp[k] + Xv[k] * Y.dt) + M[k]) - W[k];
    imu_skmul(Y.v, X.J, S); imu_mul(X.R, S, W);
    imu_mul(X.R, q.vg, M);
#pragma unroll
    for (int k = 0; k < 9; k++) q.vg[k] = (Xv[k] + M[k]) - W[k];
    imu_jac_settle(oflags, q);
}

// SL = the slots of a table entry: 26, or 62 with the Jacobians; jflags = the Jacobian flags (0 without)
template <int SL> __device__ __forceinline__ void imu_ws_store(unsigned long long* ws, int n, int level, int i, const ImuDelta& d, int jflags = 0) {
    unsigned long long* b = ws + (size_t)level * SL * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) b[(size_t)k * n] = (unsigned long long)__double_as_longlong(d.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) { b[(size_t)(9 + k) * n] = (unsigned long long)__double_as_longlong(d.v[k]); b[(size_t)(12 + k) * n] = (unsigned long long)__double_as_longlong(d.p[k]); }
    b[(size_t)15 * n] = (unsigned long long)__double_as_longlong(d.dt);
#pragma unroll
    for (int k = 0; k < 9; k++) b[(size_t)(16 + k) * n] = (unsigned long long)__double_as_longlong(d.J[k]);
    b[(size_t)25 * n] = ((unsigned long long)(uint32_t)(d.flags | (jflags << 16)) << 32) | (unsigned long long)(uint32_t)d.n_steps;
}
// (jflags: where the Jacobian flags of the entry go; the delta's flags are the low 16 bits either way, which is all of them without Jacobians)
template <int SL> __device__ __forceinline__ void imu_ws_load(const unsigned long long* ws, int n, int level, int i, ImuDelta& d, int* jflags = nullptr) {
    const unsigned long long* b = ws + (size_t)level * SL * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) d.R[k] = __longlong_as_double((long long)b[(size_t)k * n]);
#pragma unroll
    for (int k = 0; k < 3; k++) { d.v[k] = __longlong_as_double((long long)b[(size_t)(9 + k) * n]); d.p[k] = __longlong_as_double((long long)b[(size_t)(12 + k) * n]); }
    d.dt = __longlong_as_double((long long)b[(size_t)15 * n]);
#pragma unroll
    for (int k = 0; k < 9; k++) d.J[k] = __longlong_as_double((long long)b[(size_t)(16 + k) * n]);
    const unsigned long long w = b[(size_t)25 * n];
    d.n_steps = (int)(uint32_t)(w & 0xFFFFFFFFull); d.flags = (int)(uint32_t)(w >> 32);
    if (jflags) { *jflags = (int)((uint32_t)d.flags >> 16); d.flags &= 0xFFFF; }
}
// block b (0 Jvg, 1 Jva, 2 Jpg, 3 Jpa) of entry i of a 62-slot table
__device__ __forceinline__ void imu_ws_load_block(const unsigned long long* ws, int n, int level, int i, int b, double* M) {
    const unsigned long long* p = ws + ((size_t)level * 62 + 26 + 9 * b) * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = __longlong_as_double((long long)p[(size_t)k * n]);
}
__device__ __forceinline__ void imu_ws_store_block(unsigned long long* ws, int n, int level, int i, int b, const double* M) {
    unsigned long long* p = ws + ((size_t)level * 62 + 26 + 9 * b) * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) p[(size_t)k * n] = (unsigned long long)__double_as_longlong(M[k]);
}
// a whole entry: the delta and, with Jacobians, the four blocks
__device__ __forceinline__ void imu_entry_store(unsigned long long* ws, int n, int level, int i, const ImuDelta& d, const ImuNoJac&) { imu_ws_store<26>(ws, n, level, i, d); }
__device__ __forceinline__ void imu_entry_store(unsigned long long* ws, int n, int level, int i, const ImuDelta& d, const ImuJac& q) {
    imu_ws_store<62>(ws, n, level, i, d, q.flags);
    imu_ws_store_block(ws, n, level, i, 0, q.vg); imu_ws_store_block(ws, n, level, i, 1, q.va);
    imu_ws_store_block(ws, n, level, i, 2, q.pg); imu_ws_store_block(ws, n, level, i, 3, q.pa);
}
__device__ __forceinline__ void imu_entry_load(const unsigned long long* ws, int n, int level, int i, ImuDelta& d, ImuNoJac&) { imu_ws_load<26>(ws, n, level, i, d); }
__device__ __forceinline__ void imu_entry_load(const unsigned long long* ws, int n, int level, int i, ImuDelta& d, ImuJac& q) {
    imu_ws_load<62>(ws, n, level, i, d, &q.flags);
    imu_ws_load_block(ws, n, level, i, 0, q.vg); imu_ws_load_block(ws, n, level, i, 1, q.va);
    imu_ws_load_block(ws, n, level, i, 2, q.pg); imu_ws_load_block(ws, n, level, i, 3, q.pa);
}
// acc = T_k[pos] o acc.  Without Jacobians the two deltas; with them the entry's delta and flags are loaded, its blocks one at a time
__device__ __forceinline__ void imu_entry_fold(const unsigned long long* ws, int n, int level, int pos, ImuDelta& acc, ImuNoJac&) {
    ImuDelta e, o;
    imu_ws_load<26>(ws, n, level, pos, e);
    imu_compose(e, acc, o);
    acc = o;
}
__device__ __forceinline__ void imu_entry_fold(const unsigned long long* ws, int n, int level, int pos, ImuDelta& acc, ImuJac& q) {
    ImuDelta e, o;
    int ef;
    imu_ws_load<62>(ws, n, level, pos, e, &ef);
    imu_compose(e, acc, o);
    imu_jac_fold(e, ef, [&](int b, double* M) { imu_ws_load_block(ws, n, level, pos, b, M); }, acc, o.flags, q);
    acc = o;
}
// acc = the carried open delta o acc
__device__ __forceinline__ void imu_carry_load(const vis_imu_carry* carry, ImuDelta& c) {
#pragma unroll
    for (int k = 0; k < 9; k++) { c.R[k] = carry->open.R[k]; c.J[k] = carry->open.JRg[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { c.v[k] = carry->open.v[k]; c.p[k] = carry->open.p[k]; }
    c.dt = carry->open.dt; c.n_steps = carry->open.n_steps; c.flags = carry->open.flags;
}
__device__ __forceinline__ void imu_carry_fold(const vis_imu_carry* carry, const ImuJacIO&, ImuDelta& acc, ImuNoJac&) {
    ImuDelta c, o;
    imu_carry_load(carry, c);
    imu_compose(c, acc, o);
    acc = o;
}
__device__ __forceinline__ void imu_carry_fold(const vis_imu_carry* carry, const ImuJacIO& io, ImuDelta& acc, ImuJac& q) {
    ImuDelta c, o;
    imu_carry_load(carry, c);
    imu_compose(c, acc, o);
    const vis_imu_bias_jac* cj = io.cin;
    imu_jac_fold(c, cj->flags, [&](int b, double* M) {
        const double* src = b == 0 ? cj->Jvg : (b == 1 ? cj->Jva : (b == 2 ? cj->Jpg : cj->Jpa));
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = src[k];
    }, acc, o.flags, q);
    acc = o;
}
__device__ __forceinline__ void imu_jac_record(const ImuJac& q, int prev, vis_imu_bias_jac* out) {
    vis_imu_bias_jac o;
#pragma unroll
    for (int k = 0; k < 9; k++) { o.Jvg[k] = q.vg[k]; o.Jva[k] = q.va[k]; o.Jpg[k] = q.pg[k]; o.Jpa[k] = q.pa[k]; }
    o.flags = q.flags; o.q = prev;
    *out = o;
}
__device__ __forceinline__ void imu_jac_record(const ImuNoJac&, int, vis_imu_bias_jac*) {}
__device__ __forceinline__ void imu_jac_clear(ImuJac& q) { imu_jac_zero(q); q.flags = 0; }
__device__ __forceinline__ void imu_jac_clear(ImuNoJac&) {}

// ---- the covariance of (dphi, dv, dp): include/vislam_hip.h "THE COVARIANCE", restated by tests/imu_cov_ref.py.  The overloads below carry the names of the
// Jacobians' (imu_jac_clear, _settle, _record, imu_entry_*, imu_carry_fold, imu_substep_jac) so that the sub-step, the lifting and the kernels' bodies are shared
#define IMU_COV_SLOTS 71
__device__ __forceinline__ void imu_mult(const double* A, const double* B, double* M) {       // A B^T
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[3 * r + c] = (A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1]) + A[3 * r + 2] * B[3 * c + 2];
}
__device__ __forceinline__ void imu_mskew(const double* M, const double* u, double* S) {      // M [u]x
#pragma unroll
    for (int r = 0; r < 3; r++) {
        S[3 * r] = M[3 * r + 1] * u[2] - M[3 * r + 2] * u[1];
        S[3 * r + 1] = M[3 * r + 2] * u[0] - M[3 * r] * u[2];
        S[3 * r + 2] = M[3 * r] * u[1] - M[3 * r + 1] * u[0];
    }
}
__device__ __forceinline__ constexpr int imu_up(int j) { return j < 3 ? j : (j < 5 ? j + 1 : 8); }             // entry j of an upper triangle in the full matrix
__device__ __forceinline__ constexpr int imu_sym(int i, int j) { return i * 3 - i * (i - 1) / 2 + (j - i); }    // i <= j
__device__ __forceinline__ constexpr int imu_idx9(int r, int c) { return r * 9 - r * (r - 1) / 2 + (c - r); }   // r <= c, the 45 of vis_imu_cov
__device__ __forceinline__ void imu_sym_full(const double* s, double* M) {
    M[0] = s[0]; M[1] = s[1]; M[2] = s[2]; M[3] = s[1]; M[4] = s[3]; M[5] = s[4]; M[6] = s[2]; M[7] = s[4]; M[8] = s[5];
}
__device__ __forceinline__ void imu_cov_zero(ImuCov& q) {
#pragma unroll
    for (int k = 0; k < 9; k++) q.B[k] = q.D[k] = q.E[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) q.A[k] = q.C[k] = q.F[k] = 0.0;
}
__device__ __forceinline__ void imu_jac_clear(ImuCov& q) { imu_cov_zero(q); q.flags = 0; }
__device__ __forceinline__ void imu_jac_settle(int dflags, ImuCov& q) {
    bool zero = (dflags & IMU_VOID_FLAGS) || (q.flags & VIS_IMU_COV_NONFINITE);
    if (!zero) {
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; k++) fin = fin && imu_finite(q.B[k]) && imu_finite(q.D[k]) && imu_finite(q.E[k]);
#pragma unroll
        for (int k = 0; k < 6; k++) fin = fin && imu_finite(q.A[k]) && imu_finite(q.C[k]) && imu_finite(q.F[k]);
        if (!fin) { q.flags |= VIS_IMU_COV_NONFINITE; zero = true; }
    }
    if (zero) imu_cov_zero(q);
}
// block blk (0 A, 1 B, 2 C, 3 D, 4 E, 5 F) as a full 3 x 3: of an accumulator, of a record's 45, of entry i of a 71-slot table
__device__ __forceinline__ void imu_cov_block(const ImuCov& q, int blk, double* M) {
    if (blk == 0) imu_sym_full(q.A, M);
    else if (blk == 2) imu_sym_full(q.C, M);
    else if (blk == 5) imu_sym_full(q.F, M);
    else {
        const double* s = blk == 1 ? q.B : (blk == 3 ? q.D : q.E);
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = s[k];
    }
}
__device__ __forceinline__ void imu_cov_rec_block(const double* S, int blk, double* M) {
    const int bi = blk == 0 ? 0 : (blk < 3 ? 1 : 2), bj = (blk == 0 || blk == 1 || blk == 3) ? 0 : (blk == 5 ? 2 : 1);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int r = 3 * bi + i, c = 3 * bj + j;
            M[3 * i + j] = S[imu_idx9(r < c ? r : c, r < c ? c : r)];
        }
}
__device__ __forceinline__ constexpr int imu_cov_off(int blk) { return 26 + (blk == 0 ? 0 : (blk == 1 ? 6 : (blk == 2 ? 15 : (blk == 3 ? 21 : (blk == 4 ? 30 : 39))))); }
__device__ __forceinline__ void imu_cov_ws_block(const unsigned long long* ws, int n, int level, int i, int blk, double* M) {
    const unsigned long long* p = ws + ((size_t)level * IMU_COV_SLOTS + imu_cov_off(blk)) * n + i;
    if (blk == 0 || blk == 2 || blk == 5) {
        double s[6];
#pragma unroll
        for (int k = 0; k < 6; k++) s[k] = __longlong_as_double((long long)p[(size_t)k * n]);
        imu_sym_full(s, M);
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = __longlong_as_double((long long)p[(size_t)k * n]);
    }
}
// F X F^T added to q, one block at a time, for F = [a 0 0; b I 0; c t I] with a = M^T; X's blocks come through ldx(blk, full 3 x 3)
template <class LoadX> __device__ __forceinline__ void imu_cov_fterm(const double* M, const double* b, const double* c, double t, LoadX ldx, ImuCov& q) {
    double A[9], B[9], U[9], V[9], Y[9], T[9], W[9];
    ldx(0, A); ldx(1, B);
    imu_mul(A, M, T); imu_tmul(M, T, W);
#pragma unroll
    for (int j = 0; j < 6; j++) q.A[j] = W[imu_up(j)] + q.A[j];
    imu_mul(b, A, T);
#pragma unroll
    for (int k = 0; k < 9; k++) U[k] = T[k] + B[k];
    imu_mul(U, M, W);
#pragma unroll
    for (int k = 0; k < 9; k++) q.B[k] = W[k] + q.B[k];
    {
        double C[9];
        ldx(2, C);
        imu_mult(U, b, W); imu_mult(b, B, T);
#pragma unroll
        for (int j = 0; j < 6; j++) q.C[j] = (W[imu_up(j)] + (T[imu_up(j)] + C[imu_up(j)])) + q.C[j];
        imu_mult(c, B, T);
#pragma unroll
        for (int k = 0; k < 9; k++) Y[k] = T[k] + t * C[k];
    }
    double D[9], E[9];
    ldx(3, D);
    imu_mul(c, A, T);
#pragma unroll
    for (int k = 0; k < 9; k++) V[k] = (T[k] + t * B[k]) + D[k];
    imu_mul(V, M, W);
#pragma unroll
    for (int k = 0; k < 9; k++) q.D[k] = W[k] + q.D[k];
    ldx(4, E);
#pragma unroll
    for (int k = 0; k < 9; k++) Y[k] = Y[k] + E[k];
    imu_mult(V, b, W);
#pragma unroll
    for (int k = 0; k < 9; k++) q.E[k] = (W[k] + Y[k]) + q.E[k];
    ldx(5, A);                                                     // (A is done with: the p-p block of X)
    imu_mult(c, D, T); imu_mult(V, c, W);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            const double Z = (T[3 * i + j] + t * E[3 * j + i]) + A[3 * i + j];
            q.F[imu_sym(i, j)] = ((W[3 * i + j] + t * Y[3 * i + j]) + Z) + q.F[imu_sym(i, j)];
        }
}
// the covariance's share of a sub-step, BEFORE R moves on: the noise of the step, then F S F^T added
__device__ __forceinline__ void imu_substep_jac(ImuCov& q, const double* R, const double*, const double* Rn, const double*, const double* dR, const double* Jr,
                                                const double* u0, const double* u1, double h) {
    const double hh = 0.5 * h, qg = q.sg2 / h, qa = q.sa2 / h;
    double S0[9], S1[9], T[9], b[9], c[9], K1[9], K2[9], K3[9], N1[9], N2[9], N3[9];
    imu_mskew(R, u0, S0); imu_mskew(Rn, u1, S1); imu_mult(S1, dR, T);
#pragma unroll
    for (int k = 0; k < 9; k++) { b[k] = -(hh * (S0[k] + T[k])); c[k] = hh * b[k]; K1[k] = Jr[k] * h; }
    imu_mul(S1, K1, T);
#pragma unroll
    for (int k = 0; k < 9; k++) { K2[k] = -(hh * T[k]); K3[k] = (R[k] + Rn[k]) * hh; }
    const ImuCov X = q;
    imu_mult(K1, K1, N1); imu_mult(K2, K1, N2); imu_mult(K2, K2, T); imu_mult(K3, K3, N3);
#pragma unroll
    for (int j = 0; j < 6; j++) { q.A[j] = qg * N1[imu_up(j)]; q.C[j] = qg * T[imu_up(j)] + qa * N3[imu_up(j)]; }
#pragma unroll
    for (int k = 0; k < 9; k++) { q.B[k] = qg * N2[k]; q.D[k] = hh * q.B[k]; }
    imu_sym_full(q.C, T);
#pragma unroll
    for (int k = 0; k < 9; k++) q.E[k] = hh * T[k];
#pragma unroll
    for (int j = 0; j < 6; j++) q.F[j] = hh * q.E[imu_up(j)];
    imu_cov_fterm(dR, b, c, h, [&](int blk, double* Mx) { imu_cov_block(X, blk, Mx); }, q);
}
// the covariance of X o Y folded into q (in: Y's, out: the composition's): G Y.S G^T in place, then F X.S F^T added block by block
template <class LoadX> __device__ __forceinline__ void imu_cov_fold(const ImuDelta& X, int xflags, LoadX ldx, const ImuDelta& Y, int oflags, ImuCov& q) {
    double b[9], c[9], T[9], W[9], Fl[9];
    q.flags |= xflags;
    imu_mul(X.R, q.B, T);
#pragma unroll
    for (int k = 0; k < 9; k++) q.B[k] = T[k];
    imu_mul(X.R, q.D, T);
#pragma unroll
    for (int k = 0; k < 9; k++) q.D[k] = T[k];
    imu_mul(X.R, q.E, T); imu_mult(T, X.R, W);
#pragma unroll
    for (int k = 0; k < 9; k++) q.E[k] = W[k];
    imu_sym_full(q.C, Fl); imu_mul(X.R, Fl, T); imu_mult(T, X.R, W);
#pragma unroll
    for (int j = 0; j < 6; j++) q.C[j] = W[imu_up(j)];
    imu_sym_full(q.F, Fl); imu_mul(X.R, Fl, T); imu_mult(T, X.R, W);
#pragma unroll
    for (int j = 0; j < 6; j++) q.F[j] = W[imu_up(j)];
    imu_mskew(X.R, Y.v, T); imu_mskew(X.R, Y.p, W);
#pragma unroll
    for (int k = 0; k < 9; k++) { b[k] = -T[k]; c[k] = -W[k]; }
    imu_cov_fterm(Y.R, b, c, Y.dt, ldx, q);
    imu_jac_settle(oflags, q);
}
__device__ __forceinline__ void imu_entry_store(unsigned long long* ws, int n, int level, int i, const ImuDelta& d, const ImuCov& q) {
    imu_ws_store<IMU_COV_SLOTS>(ws, n, level, i, d, q.flags);
    unsigned long long* p = ws + ((size_t)level * IMU_COV_SLOTS + 26) * n + i;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        p[(size_t)k * n] = (unsigned long long)__double_as_longlong(q.A[k]);
        p[(size_t)(15 + k) * n] = (unsigned long long)__double_as_longlong(q.C[k]);
        p[(size_t)(39 + k) * n] = (unsigned long long)__double_as_longlong(q.F[k]);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        p[(size_t)(6 + k) * n] = (unsigned long long)__double_as_longlong(q.B[k]);
        p[(size_t)(21 + k) * n] = (unsigned long long)__double_as_longlong(q.D[k]);
        p[(size_t)(30 + k) * n] = (unsigned long long)__double_as_longlong(q.E[k]);
    }
}
__device__ __forceinline__ void imu_entry_load(const unsigned long long* ws, int n, int level, int i, ImuDelta& d, ImuCov& q) {
    imu_ws_load<IMU_COV_SLOTS>(ws, n, level, i, d, &q.flags);
    const unsigned long long* p = ws + ((size_t)level * IMU_COV_SLOTS + 26) * n + i;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        q.A[k] = __longlong_as_double((long long)p[(size_t)k * n]);
        q.C[k] = __longlong_as_double((long long)p[(size_t)(15 + k) * n]);
        q.F[k] = __longlong_as_double((long long)p[(size_t)(39 + k) * n]);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        q.B[k] = __longlong_as_double((long long)p[(size_t)(6 + k) * n]);
        q.D[k] = __longlong_as_double((long long)p[(size_t)(21 + k) * n]);
        q.E[k] = __longlong_as_double((long long)p[(size_t)(30 + k) * n]);
    }
    q.sg2 = q.sa2 = 0.0;
}
__device__ __forceinline__ void imu_entry_fold(const unsigned long long* ws, int n, int level, int pos, ImuDelta& acc, ImuCov& q) {
    ImuDelta e, o;
    int ef;
    imu_ws_load<IMU_COV_SLOTS>(ws, n, level, pos, e, &ef);
    imu_compose(e, acc, o);
    imu_cov_fold(e, ef, [&](int blk, double* M) { imu_cov_ws_block(ws, n, level, pos, blk, M); }, acc, o.flags, q);
    acc = o;
}
__device__ __forceinline__ void imu_carry_fold(const vis_imu_carry* carry, const ImuCovIO& io, ImuDelta& acc, ImuCov& q) {
    ImuDelta c, o;
    imu_carry_load(carry, c);
    imu_compose(c, acc, o);
    const vis_imu_cov* cc = io.cin;
    imu_cov_fold(c, cc->flags, [&](int blk, double* M) { imu_cov_rec_block(cc->S, blk, M); }, acc, o.flags, q);
    acc = o;
}
__device__ __forceinline__ void imu_jac_record(const ImuCov& q, int prev, vis_imu_cov* out) {
    vis_imu_cov o;
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = r; c < 9; c++) {
            const int br = r / 3, bc = c / 3, i = r % 3, j = c % 3;
            o.S[imu_idx9(r, c)] = br == bc ? (br == 0 ? q.A : (br == 1 ? q.C : q.F))[imu_sym(i, j)] : (br == 0 ? (bc == 1 ? q.B : q.D) : q.E)[3 * j + i];
        }
    o.flags = q.flags; o.q = prev;
    *out = o;
}

// ---------------------------------------------------------------------------------------------- step 1: the intervals
struct ImuPoint { double t, w[3], a[3]; };
__device__ __forceinline__ void imu_read(const vis_imu_sample* s, int j, ImuPoint& o) {
    o.t = s[j].t;
#pragma unroll
    for (int k = 0; k < 3; k++) { o.w[k] = s[j].w[k]; o.a[k] = s[j].a[k]; }
}
__device__ __forceinline__ bool imu_point_finite(const ImuPoint& s) {
    bool fin = imu_finite(s.t);
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && imu_finite(s.w[k]) && imu_finite(s.a[k]);
    return fin;
}
__device__ __forceinline__ int imu_ub(const vis_imu_sample* s, int n, double x) {      // the first index with t > x
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s[mid].t <= x) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int imu_lb(const vis_imu_sample* s, int n, double x) {      // the first index with t >= x
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s[mid].t < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// the value at breakpoint x (n >= 1); false: a sample it uses is not finite
__device__ __forceinline__ bool imu_value(const vis_imu_sample* s, int n, double x, ImuPoint& o, int& flags) {
    const int j = imu_ub(s, n, x);
    if (j == 0 || j == n) {
        imu_read(s, j == 0 ? 0 : n - 1, o);
        if (!imu_point_finite(o)) return false;
        if (!(o.t == x)) flags |= VIS_IMU_EXTRAPOLATED;
        o.t = x;
        return true;
    }
    ImuPoint s0, s1;
    imu_read(s, j - 1, s0); imu_read(s, j, s1);
    if (!imu_point_finite(s0) || !imu_point_finite(s1)) return false;
    const double u = (x - s0.t) / (s1.t - s0.t);
    o.t = x;
#pragma unroll
    for (int k = 0; k < 3; k++) { o.w[k] = s0.w[k] + u * (s1.w[k] - s0.w[k]); o.a[k] = s0.a[k] + u * (s1.a[k] - s0.a[k]); }
    return true;
}
__device__ __forceinline__ double imu_horner(const double* c, double x) {
    double acc = c[VIS_IMU_EXP_TERMS - 1];
#pragma unroll
    for (int k = VIS_IMU_EXP_TERMS - 2; k >= 0; k--) acc = c[k] + x * acc;
    return acc;
}
// the Jacobians' share of a sub-step, BEFORE R and JRg move on: R, J the old ones, Rn, Jn the new; p's lines use the old v Jacobians, as p uses the old v
__device__ __forceinline__ void imu_substep_jac(ImuJac& q, const double* R, const double* J, const double* Rn, const double* Jn, const double*, const double*,
                                                const double* u0, const double* u1, double h) {
    double S[9], G0[9], G1[9];
    imu_skmul(u0, J, S); imu_mul(R, S, G0);
    imu_skmul(u1, Jn, S); imu_mul(Rn, S, G1);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double Dg = -0.5 * (G0[k] + G1[k]), Da = -0.5 * (R[k] + Rn[k]);
        q.pg[k] = q.pg[k] + (q.vg[k] * h + (0.5 * Dg) * (h * h));
        q.vg[k] = q.vg[k] + Dg * h;
        q.pa[k] = q.pa[k] + (q.va[k] * h + (0.5 * Da) * (h * h));
        q.va[k] = q.va[k] + Da * h;
    }
}
__device__ __forceinline__ void imu_substep_jac(ImuNoJac&, const double*, const double*, const double*, const double*, const double*, const double*, const double*,
                                                const double*, double) {}
template <class Jac> __device__ __forceinline__ void imu_substep(ImuDelta& d, Jac& q, const vis_imu_params& P, const ImuPoint& s0, const ImuPoint& s1) {
    constexpr double cA[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_A, cB[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_B, cC[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_C;
    const double h = s1.t - s0.t;
    if (!(h > 0.0)) { d.flags |= VIS_IMU_ORDER; return; }
    d.n_steps += 1;
    if (h > P.max_gap_s) d.flags |= VIS_IMU_GAP;
    double phi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) phi[k] = (0.5 * (s0.w[k] + s1.w[k]) - P.bg[k]) * h;
    const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2], xy = phi[0] * phi[1], xz = phi[0] * phi[2], yz = phi[1] * phi[2];
    const double th2 = (xx + yy) + zz;
    if (th2 > P.max_angle * P.max_angle) d.flags |= VIS_IMU_FAST;
    const double A = imu_horner(cA, th2), B = imu_horner(cB, th2), C = imu_horner(cC, th2);
    const double dR[9] = {1.0 - B * (yy + zz), B * xy - A * phi[2], B * xz + A * phi[1],
                          B * xy + A * phi[2], 1.0 - B * (xx + zz), B * yz - A * phi[0],
                          B * xz - A * phi[1], B * yz + A * phi[0], 1.0 - B * (xx + yy)};
    const double Jr[9] = {1.0 - C * (yy + zz), C * xy + B * phi[2], C * xz - B * phi[1],
                          C * xy - B * phi[2], 1.0 - C * (xx + zz), C * yz + B * phi[0],
                          C * xz + B * phi[1], C * yz - B * phi[0], 1.0 - C * (xx + yy)};
    double Rn[9], u0[3], u1[3], r0[3], r1[3], M[9];
    imu_mul(d.R, dR, Rn);
#pragma unroll
    for (int k = 0; k < 3; k++) { u0[k] = s0.a[k] - P.ba[k]; u1[k] = s1.a[k] - P.ba[k]; }
    imu_mulv(d.R, u0, r0);
    imu_mulv(Rn, u1, r1);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double am = 0.5 * (r0[r] + r1[r]);
        d.p[r] = d.p[r] + (d.v[r] * h + (0.5 * am) * (h * h));
        d.v[r] = d.v[r] + am * h;
    }
    imu_tmul(dR, d.J, M);
    double Jn[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Jn[k] = M[k] - Jr[k] * h;
    imu_substep_jac(q, d.R, d.J, Rn, Jn, dR, Jr, u0, u1, h);
#pragma unroll
    for (int k = 0; k < 9; k++) { d.J[k] = Jn[k]; d.R[k] = Rn[k]; }
}

// the body of the interval kernels; q: the cleared accumulator of the variant
template <class Jac, class Init> __device__ __forceinline__ void imu_intervals_body(const vis_imu_params& P, Init init, int n, const vis_imu_sample* __restrict__ samples, int n_samples,
                                                                        const double* __restrict__ tframe, const vis_imu_carry* __restrict__ carry,
                                                                        unsigned long long* __restrict__ ws) {
    const int i = blockIdx.x * IMU_IV_BLOCK + threadIdx.x;
    if (i >= n) return;
    ImuDelta d;
    Jac q;
    imu_identity(d);
    imu_jac_clear(q);
    init(q);
    const bool start = i > 0 || (carry && (carry->valid & VIS_IMU_CARRY_TIME));
    if (!start) { d.flags = VIS_IMU_NO_START; imu_entry_store(ws, n, 0, i, d, q); return; }
    const double ta = i > 0 ? tframe[i - 1] : carry->t_last, tb = tframe[i];
    d.dt = tb - ta;
    if (!imu_finite(d.dt)) d.dt = 0.0;
    bool bad = !imu_finite(ta) || !imu_finite(tb);
    if (!bad && n_samples < 1) d.flags |= VIS_IMU_EMPTY | VIS_IMU_EXTRAPOLATED;
    if (!bad && n_samples >= 1) {
        ImuPoint pa, pb;
        bad = !imu_value(samples, n_samples, ta, pa, d.flags);
        if (!bad) bad = !imu_value(samples, n_samples, tb, pb, d.flags);
        const int lo = imu_ub(samples, n_samples, ta), hi = imu_lb(samples, n_samples, tb);
        if (!bad) {
            if (hi <= lo) d.flags |= VIS_IMU_EMPTY;
            for (int j = lo; j < hi; j++) {                          // every inside sample is looked at before any sub-step is taken
                ImuPoint s; imu_read(samples, j, s);
                if (!imu_point_finite(s)) { bad = true; break; }
            }
        }
        if (!bad) {
            ImuPoint cur = pa;
            for (int j = lo; j < hi; j++) {
                ImuPoint s; imu_read(samples, j, s);
                imu_substep(d, q, P, cur, s);
                cur = s;
            }
            imu_substep(d, q, P, cur, pb);
        }
    }
    if (bad || !imu_all_finite(d)) imu_void(d);
    imu_jac_settle(d.flags, q);
    imu_entry_store(ws, n, 0, i, d, q);
}
template <bool JAC> __global__ __launch_bounds__(IMU_IV_BLOCK) void k_imu_intervals(vis_imu_params P, int n, const vis_imu_sample* __restrict__ samples, int n_samples,
                                                                const double* __restrict__ tframe, const vis_imu_carry* __restrict__ carry,
                                                                unsigned long long* __restrict__ ws) {
    typedef typename ImuJacOf<JAC>::type Jac;
    imu_intervals_body<Jac>(P, [](Jac&) {}, n, samples, n_samples, tframe, carry, ws);
}
// the covariance's: the same intervals with the 45 numbers beside the delta, a table of 71 slots
__global__ __launch_bounds__(IMU_IV_BLOCK) void k_imu_cov_intervals(vis_imu_params P, vis_imu_noise N, int n, const vis_imu_sample* __restrict__ samples, int n_samples,
                                                                    const double* __restrict__ tframe, const vis_imu_carry* __restrict__ carry,
                                                                    unsigned long long* __restrict__ ws) {
    imu_intervals_body<ImuCov>(P, [&](ImuCov& q) { q.sg2 = N.sigma_g * N.sigma_g; q.sa2 = N.sigma_a * N.sigma_a; }, n, samples, n_samples, tframe, carry, ws);
}

// ---------------------------------------------------------------------------------------------- step 2: the pairs
// the composition of the L intervals that end at frame i (the set bits of L, rising; pos walks back); L >= 1
template <class Jac> __device__ __forceinline__ void imu_lift(const unsigned long long* ws, int n, int i, int L, ImuDelta& acc, Jac& q) {
    int pos = i;
    bool first = true;
    for (int k = 0; (1 << k) <= L; k++) {
        if (!(L & (1 << k))) continue;
        if (first) { imu_entry_load(ws, n, k, pos, acc, q); first = false; }
        else imu_entry_fold(ws, n, k, pos, acc, q);
        pos -= 1 << k;
    }
}
__device__ __forceinline__ void imu_record(const ImuDelta& d, int q, vis_imu_delta& o) {
#pragma unroll
    for (int k = 0; k < 9; k++) { o.R[k] = d.R[k]; o.JRg[k] = d.J[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { o.v[k] = d.v[k]; o.p[k] = d.p[k]; }
    o.dt = d.dt; o.n_steps = d.n_steps; o.flags = d.flags; o.q = q; o.reserved_ = 0;
}

// d_rot's rule: (float)(r_ic^T R r_ic), the identity for a frame without a delta or an entry beyond FLT_MAX
__device__ __forceinline__ void imu_rot_row(const double* r_ic, const ImuDelta& d, float* rot) {
    double T[9], M[9];
    imu_tmul(r_ic, d.R, T);
    imu_mul(T, r_ic, M);
    bool ok = !(d.flags & (VIS_IMU_NO_PAIR | VIS_IMU_NO_CARRY | VIS_IMU_NONFINITE));
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && fabs(M[k]) <= 3.4028234663852886e38;
#pragma unroll
    for (int k = 0; k < 9; k++) rot[k] = ok ? (float)M[k] : ((k & 3) == 0 ? 1.0f : 0.0f);
}

// the body of the pairs kernels; JAC: the variant writes rows and a carried record of its own through jio
template <class Jac, bool JAC, class IO> __device__ __forceinline__ void imu_pairs_body(const vis_imu_params& P, int n, const FtFrames& fr, const double* __restrict__ tframe,
                                                                                const vis_imu_carry* __restrict__ carry, unsigned long long* __restrict__ ws,
                                                                                vis_imu_delta* __restrict__ delta, float* __restrict__ rot,
                                                                                vis_imu_carry* __restrict__ carry_out, const IO& jio) {
    __shared__ int s_maxL, s_last;
    const int tid = threadIdx.x;
    const bool have_carry = carry && (carry->valid & VIS_IMU_CARRY_TIME);
    if (tid == 0) { s_maxL = 0; s_last = -1; }
    __syncthreads();
    {
        int mL = 0, last = -1;
        for (int i = tid; i < n; i += IMU_BLOCK) {
            const int p = imu_prev(fr, i);
            const int L = p >= 0 ? i - p : (p == VIS_KF_CARRIED && have_carry ? i + 1 : 0);
            mL = max(mL, L);
            if (p != VIS_KF_NOT_SAVED) last = i;
        }
        atomicMax(&s_maxL, mL); atomicMax(&s_last, last);
    }
    __syncthreads();
    const int last = s_last;
    const int Lc = carry_out ? (last >= 0 ? n - 1 - last : n) : 0;      // the carry's open delta is one more composition of the call
    const int maxL = max(s_maxL, Lc);                                  // (uniform)
    // ---- the levels: T_k[i] = T_{k-1}[i - 2^{k-1}] o T_{k-1}[i], i >= 2^k - 1
    for (int k = 1; (1 << k) <= maxL; k++) {
        const int half = 1 << (k - 1);
        for (int i = tid; i < n; i += IMU_BLOCK) {
            if (i < (1 << k) - 1) continue;
            ImuDelta o;
            Jac q;
            imu_entry_load(ws, n, k - 1, i, o, q);
            imu_entry_fold(ws, n, k - 1, i - half, o, q);
            imu_entry_store(ws, n, k, i, o, q);
        }
        __syncthreads();
    }
    // ---- the pairs
    for (int i = tid; i < n; i += IMU_BLOCK) {
        const int p = imu_prev(fr, i);
        ImuDelta d;
        Jac q;
        imu_identity(d);
        imu_jac_clear(q);
        if (p == VIS_KF_NOT_SAVED || p == VIS_KF_FIRST) d.flags = VIS_IMU_NO_PAIR;
        else if (p == VIS_KF_CARRIED && !have_carry) d.flags = VIS_IMU_NO_CARRY;
        else {
            imu_lift(ws, n, i, p >= 0 ? i - p : i + 1, d, q);
            if (p == VIS_KF_CARRIED && (carry->valid & VIS_IMU_CARRY_OPEN)) imu_carry_fold(carry, jio, d, q);
        }
        vis_imu_delta o;
        imu_record(d, p, o);
        delta[i] = o;
        if (JAC) imu_jac_record(q, p, jio.rows + i);
        if (rot) imu_rot_row(P.r_ic, d, rot + (size_t)i * 9);
    }
    // ---- the carry
    if (carry_out && tid == 0) {
        ImuDelta d;
        Jac q;
        imu_identity(d);
        imu_jac_clear(q);
        int valid = VIS_IMU_CARRY_TIME;
        if (Lc > 0) {
            imu_lift(ws, n, n - 1, Lc, d, q);
            valid |= VIS_IMU_CARRY_OPEN;
            if (last < 0 && have_carry && (carry->valid & VIS_IMU_CARRY_OPEN)) imu_carry_fold(carry, jio, d, q);
        }
        vis_imu_carry co;
        co.t_last = tframe[n - 1];
        imu_record(d, 0, co.open);
        co.valid = valid; co.reserved_ = 0;
        *carry_out = co;
        if (JAC) imu_jac_record(q, 0, jio.cout);
    }
}
template <bool JAC> __global__ __launch_bounds__(IMU_BLOCK) void k_imu_pairs(vis_imu_params P, int n, FtFrames fr, const double* __restrict__ tframe,
                                                         const vis_imu_carry* __restrict__ carry, unsigned long long* __restrict__ ws,
                                                         vis_imu_delta* __restrict__ delta, float* __restrict__ rot, vis_imu_carry* __restrict__ carry_out,
                                                         ImuJacIO jio) {
    imu_pairs_body<typename ImuJacOf<JAC>::type, JAC>(P, n, fr, tframe, carry, ws, delta, rot, carry_out, jio);
}
__global__ __launch_bounds__(IMU_BLOCK) void k_imu_cov_pairs(vis_imu_params P, int n, FtFrames fr, const double* __restrict__ tframe,
                                                             const vis_imu_carry* __restrict__ carry, unsigned long long* __restrict__ ws,
                                                             vis_imu_delta* __restrict__ delta, float* __restrict__ rot, vis_imu_carry* __restrict__ carry_out,
                                                             ImuCovIO cio) {
    imu_pairs_body<ImuCov, true>(P, n, fr, tframe, carry, ws, delta, rot, carry_out, cio);
}

// ---------------------------------------------------------------------------------------------- the bias correction of the records
// One lane per frame: R' = R Exp(JRg dbg), v' = v + (Jvg dbg + Jva dba), p' = p + (Jpg dbg + Jpa dba); a record that cannot be corrected is copied
__global__ __launch_bounds__(IMU_IV_BLOCK) void k_imu_correct(vis_imu_params P, int n, const vis_imu_delta* __restrict__ delta, const vis_imu_bias_jac* __restrict__ jac,
                                                              const double* __restrict__ dbg, const double* __restrict__ dba, vis_imu_delta* __restrict__ out,
                                                              float* __restrict__ rot, int32_t* __restrict__ status) {
    constexpr double cA[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_A, cB[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_B;
    const int i = blockIdx.x * IMU_IV_BLOCK + threadIdx.x;
    if (i >= n) return;
    vis_imu_delta r = delta[i];
    ImuDelta d;
#pragma unroll
    for (int k = 0; k < 9; k++) { d.R[k] = r.R[k]; d.J[k] = r.JRg[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { d.v[k] = r.v[k]; d.p[k] = r.p[k]; }
    d.dt = r.dt; d.n_steps = r.n_steps; d.flags = r.flags;
    double bg[3], ba[3];
    bool bfin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) { bg[k] = dbg[k]; ba[k] = dba ? dba[k] : 0.0; bfin = bfin && imu_finite(bg[k]) && imu_finite(ba[k]); }
    int st = VIS_IMC_OK;
    if ((d.flags & IMU_VOID_FLAGS) || !imu_all_finite(d)) st = VIS_IMC_UNUSABLE;
    else if (jac[i].flags & VIS_IMU_JAC_NONFINITE) st = VIS_IMC_JAC;
    else if (!bfin) st = VIS_IMC_BIAS;
    else {
        double phi[3];
        imu_mulv(d.J, bg, phi);
        const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2], xy = phi[0] * phi[1], xz = phi[0] * phi[2], yz = phi[1] * phi[2];
        const double th2 = (xx + yy) + zz;
        if (th2 > P.max_angle * P.max_angle) st = VIS_IMC_ANGLE;
        else {
            const double A = imu_horner(cA, th2), B = imu_horner(cB, th2);
            const double dR[9] = {1.0 - B * (yy + zz), B * xy - A * phi[2], B * xz + A * phi[1],
                                  B * xy + A * phi[2], 1.0 - B * (xx + zz), B * yz - A * phi[0],
                                  B * xz - A * phi[1], B * yz + A * phi[0], 1.0 - B * (xx + yy)};
            double Rn[9], vg[3], va[3], pg[3], pa[3], vn[3], pn[3];
            imu_mul(d.R, dR, Rn);
            const vis_imu_bias_jac* j = jac + i;
            imu_mulv(j->Jvg, bg, vg); imu_mulv(j->Jva, ba, va); imu_mulv(j->Jpg, bg, pg); imu_mulv(j->Jpa, ba, pa);
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; k++) { vn[k] = d.v[k] + (vg[k] + va[k]); pn[k] = d.p[k] + (pg[k] + pa[k]); fin = fin && imu_finite(vn[k]) && imu_finite(pn[k]); }
#pragma unroll
            for (int k = 0; k < 9; k++) fin = fin && imu_finite(Rn[k]);
            if (!fin) st = VIS_IMC_NONFINITE;
            else {
#pragma unroll
                for (int k = 0; k < 9; k++) { d.R[k] = Rn[k]; r.R[k] = Rn[k]; }
#pragma unroll
                for (int k = 0; k < 3; k++) { r.v[k] = vn[k]; r.p[k] = pn[k]; }
            }
        }
    }
    out[i] = r;
    if (status) status[i] = st;
    if (rot) imu_rot_row(P.r_ic, d, rot + (size_t)i * 9);
}

static size_t imu_table_bytes_of(int n, int slots) {
    int levels = 1;
    while ((1 << levels) <= n) levels++;
    return (size_t)levels * slots * sizeof(unsigned long long) * (size_t)(n > 0 ? n : 1);
}
size_t imu_table_bytes(int n) { return imu_table_bytes_of(n, 26); }
size_t imu_jac_table_bytes(int n) { return imu_table_bytes_of(n, 62); }
size_t imu_cov_table_bytes(int n) { return imu_table_bytes_of(n, IMU_COV_SLOTS); }

int imu_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
            const vis_imu_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, float* d_rot, vis_imu_carry* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (n > VIS_IMU_MAX_FRAMES || !d_ws || n_samples < 0) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_imu_intervals<false>, dim3((n + IMU_IV_BLOCK - 1) / IMU_IV_BLOCK), dim3(IMU_IV_BLOCK), 0, ctx->stream, *ip, n, d_samples, n_samples, d_tframe,
                       d_carry, (unsigned long long*)d_ws);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_imu_pairs<false>, dim3(1), dim3(IMU_BLOCK), 0, ctx->stream, *ip, n, fr, d_tframe, d_carry, (unsigned long long*)d_ws, d_delta, d_rot, d_carry_out,
                       ImuJacIO{nullptr, nullptr, nullptr});
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int imu_jac_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
                   const vis_imu_jac_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, vis_imu_bias_jac* d_jac, float* d_rot, vis_imu_jac_carry* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (n > VIS_IMU_MAX_FRAMES || !d_ws || !d_jac || n_samples < 0) return VIS_E_INVALID;
    const vis_imu_carry* cin = d_carry ? &d_carry->carry : nullptr;
    vis_imu_carry* cout = d_carry_out ? &d_carry_out->carry : nullptr;
    hipLaunchKernelGGL(k_imu_intervals<true>, dim3((n + IMU_IV_BLOCK - 1) / IMU_IV_BLOCK), dim3(IMU_IV_BLOCK), 0, ctx->stream, *ip, n, d_samples, n_samples, d_tframe,
                       cin, (unsigned long long*)d_ws);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_imu_pairs<true>, dim3(1), dim3(IMU_BLOCK), 0, ctx->stream, *ip, n, fr, d_tframe, cin, (unsigned long long*)d_ws, d_delta, d_rot, cout,
                       ImuJacIO{d_carry ? &d_carry->open_jac : nullptr, d_jac, d_carry_out ? &d_carry_out->open_jac : nullptr});
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int imu_cov_launch(vis_ctx* ctx, const vis_imu_params* ip, const vis_imu_noise* np, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples,
                   const double* d_tframe, const vis_imu_cov_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, vis_imu_cov* d_cov, float* d_rot,
                   vis_imu_cov_carry* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (n > VIS_IMU_MAX_FRAMES || !d_ws || !d_cov || n_samples < 0) return VIS_E_INVALID;
    const vis_imu_carry* cin = d_carry ? &d_carry->carry : nullptr;
    vis_imu_carry* cout = d_carry_out ? &d_carry_out->carry : nullptr;
    hipLaunchKernelGGL(k_imu_cov_intervals, dim3((n + IMU_IV_BLOCK - 1) / IMU_IV_BLOCK), dim3(IMU_IV_BLOCK), 0, ctx->stream, *ip, *np, n, d_samples, n_samples, d_tframe,
                       cin, (unsigned long long*)d_ws);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_imu_cov_pairs, dim3(1), dim3(IMU_BLOCK), 0, ctx->stream, *ip, n, fr, d_tframe, cin, (unsigned long long*)d_ws, d_delta, d_rot, cout,
                       ImuCovIO{d_carry ? &d_carry->open_cov : nullptr, d_cov, d_carry_out ? &d_carry_out->open_cov : nullptr});
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int imu_correct_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, const vis_imu_delta* d_delta, const vis_imu_bias_jac* d_jac, const double* d_dbg,
                       const double* d_dba, vis_imu_delta* d_out, float* d_rot, int32_t* d_status) {
    if (n < 1) return VIS_OK;
    hipLaunchKernelGGL(k_imu_correct, dim3((n + IMU_IV_BLOCK - 1) / IMU_IV_BLOCK), dim3(IMU_IV_BLOCK), 0, ctx->stream, *ip, n, d_delta, d_jac, d_dbg, d_dba, d_out,
                       d_rot, d_status);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
