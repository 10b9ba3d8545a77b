// imu.hip -- IMU preintegration on the device: one delta per frame interval (k_imu_intervals, a lane per interval, a serial loop over its
// sub-steps) and the pair deltas by binary lifting (k_imu_pairs: ONE launch of one workgroup builds the levels T_k[i] = T_{k-1}[i - 2^{k-1}] o T_{k-1}[i]
// with a barrier between them, composes every pair from the set bits of its length, and writes the records, the camera-frame rotations and the
// carry).  include/vislam_hip.h has the contract operation for operation, tests/imu_ref.py restates it.  Double arithmetic, + - * / only.
// A table entry is 26 eight-byte slots (25 doubles, n_steps and flags packed into the last), structure of arrays: slot s of entry i of level k
// is ws[((size_t)k * 26 + s) * n + i], so consecutive frames read consecutive addresses.  Levels are separate arrays: a round reads level k - 1 and
// writes level k, nothing is read and written in one round, one barrier a round suffices.
#include "vis_internal.h"
#include <cmath>

#define IMU_BLOCK 256
#define IMU_IV_BLOCK 64

struct ImuDelta { double R[9], v[3], p[3], dt, J[9]; int n_steps, flags; };

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

__device__ __forceinline__ void imu_ws_store(unsigned long long* ws, int n, int level, int i, const ImuDelta& d) {
    unsigned long long* b = ws + (size_t)level * 26 * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) b[(size_t)k * n] = (unsigned long long)__double_as_longlong(d.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) { b[(size_t)(9 + k) * n] = (unsigned long long)__double_as_longlong(d.v[k]); b[(size_t)(12 + k) * n] = (unsigned long long)__double_as_longlong(d.p[k]); }
    b[(size_t)15 * n] = (unsigned long long)__double_as_longlong(d.dt);
#pragma unroll
    for (int k = 0; k < 9; k++) b[(size_t)(16 + k) * n] = (unsigned long long)__double_as_longlong(d.J[k]);
    b[(size_t)25 * n] = ((unsigned long long)(uint32_t)d.flags << 32) | (unsigned long long)(uint32_t)d.n_steps;
}
__device__ __forceinline__ void imu_ws_load(const unsigned long long* ws, int n, int level, int i, ImuDelta& d) {
    const unsigned long long* b = ws + (size_t)level * 26 * n + i;
#pragma unroll
    for (int k = 0; k < 9; k++) d.R[k] = __longlong_as_double((long long)b[(size_t)k * n]);
#pragma unroll
    for (int k = 0; k < 3; k++) { d.v[k] = __longlong_as_double((long long)b[(size_t)(9 + k) * n]); d.p[k] = __longlong_as_double((long long)b[(size_t)(12 + k) * n]); }
    d.dt = __longlong_as_double((long long)b[(size_t)15 * n]);
#pragma unroll
    for (int k = 0; k < 9; k++) d.J[k] = __longlong_as_double((long long)b[(size_t)(16 + k) * n]);
    const unsigned long long w = b[(size_t)25 * n];
    d.n_steps = (int)(uint32_t)(w & 0xFFFFFFFFull); d.flags = (int)(uint32_t)(w >> 32);
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
__device__ __forceinline__ void imu_substep(ImuDelta& d, const vis_imu_params& P, const ImuPoint& s0, const ImuPoint& s1) {
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
#pragma unroll
    for (int k = 0; k < 9; k++) { d.J[k] = M[k] - Jr[k] * h; d.R[k] = Rn[k]; }
}

__global__ __launch_bounds__(IMU_IV_BLOCK) void k_imu_intervals(vis_imu_params P, int n, const vis_imu_sample* __restrict__ samples, int n_samples,
                                                                const double* __restrict__ tframe, const vis_imu_carry* __restrict__ carry,
                                                                unsigned long long* __restrict__ ws) {
    const int i = blockIdx.x * IMU_IV_BLOCK + threadIdx.x;
    if (i >= n) return;
    ImuDelta d;
    imu_identity(d);
    const bool start = i > 0 || (carry && (carry->valid & VIS_IMU_CARRY_TIME));
    if (!start) { d.flags = VIS_IMU_NO_START; imu_ws_store(ws, n, 0, i, d); return; }
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
                imu_substep(d, P, cur, s);
                cur = s;
            }
            imu_substep(d, P, cur, pb);
        }
    }
    if (bad || !imu_all_finite(d)) imu_void(d);
    imu_ws_store(ws, n, 0, i, d);
}

// ---------------------------------------------------------------------------------------------- step 2: the pairs
// the composition of the L intervals that end at frame i (the set bits of L, rising; pos walks back); L >= 1
__device__ __forceinline__ void imu_lift(const unsigned long long* ws, int n, int i, int L, ImuDelta& acc) {
    int pos = i;
    bool first = true;
    for (int k = 0; (1 << k) <= L; k++) {
        if (!(L & (1 << k))) continue;
        ImuDelta e;
        imu_ws_load(ws, n, k, pos, e);
        if (first) { acc = e; first = false; }
        else { ImuDelta o; imu_compose(e, acc, o); acc = o; }
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

__global__ __launch_bounds__(IMU_BLOCK) void k_imu_pairs(vis_imu_params P, int n, FtFrames fr, const double* __restrict__ tframe,
                                                         const vis_imu_carry* __restrict__ carry, unsigned long long* __restrict__ ws,
                                                         vis_imu_delta* __restrict__ delta, float* __restrict__ rot, vis_imu_carry* __restrict__ carry_out) {
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
            ImuDelta a, b, o;
            imu_ws_load(ws, n, k - 1, i - half, a);
            imu_ws_load(ws, n, k - 1, i, b);
            imu_compose(a, b, o);
            imu_ws_store(ws, n, k, i, o);
        }
        __syncthreads();
    }
    // ---- the pairs
    for (int i = tid; i < n; i += IMU_BLOCK) {
        const int p = imu_prev(fr, i);
        ImuDelta d;
        imu_identity(d);
        if (p == VIS_KF_NOT_SAVED || p == VIS_KF_FIRST) d.flags = VIS_IMU_NO_PAIR;
        else if (p == VIS_KF_CARRIED && !have_carry) d.flags = VIS_IMU_NO_CARRY;
        else {
            imu_lift(ws, n, i, p >= 0 ? i - p : i + 1, d);
            if (p == VIS_KF_CARRIED && (carry->valid & VIS_IMU_CARRY_OPEN)) {
                ImuDelta c, o;
#pragma unroll
                for (int k = 0; k < 9; k++) { c.R[k] = carry->open.R[k]; c.J[k] = carry->open.JRg[k]; }
#pragma unroll
                for (int k = 0; k < 3; k++) { c.v[k] = carry->open.v[k]; c.p[k] = carry->open.p[k]; }
                c.dt = carry->open.dt; c.n_steps = carry->open.n_steps; c.flags = carry->open.flags;
                imu_compose(c, d, o);
                d = o;
            }
        }
        vis_imu_delta o;
        imu_record(d, p, o);
        delta[i] = o;
        if (rot) {
            double T[9], M[9];
            imu_tmul(P.r_ic, d.R, T);
            imu_mul(T, P.r_ic, M);
            bool ok = !(d.flags & (VIS_IMU_NO_PAIR | VIS_IMU_NO_CARRY | VIS_IMU_NONFINITE));
#pragma unroll
            for (int k = 0; k < 9; k++) ok = ok && fabs(M[k]) <= 3.4028234663852886e38;
#pragma unroll
            for (int k = 0; k < 9; k++) rot[(size_t)i * 9 + k] = ok ? (float)M[k] : ((k & 3) == 0 ? 1.0f : 0.0f);
        }
    }
    // ---- the carry
    if (carry_out && tid == 0) {
        ImuDelta d;
        imu_identity(d);
        int valid = VIS_IMU_CARRY_TIME;
        if (Lc > 0) {
            imu_lift(ws, n, n - 1, Lc, d);
            valid |= VIS_IMU_CARRY_OPEN;
            if (last < 0 && have_carry && (carry->valid & VIS_IMU_CARRY_OPEN)) {
                ImuDelta c, o;
#pragma unroll
                for (int k = 0; k < 9; k++) { c.R[k] = carry->open.R[k]; c.J[k] = carry->open.JRg[k]; }
#pragma unroll
                for (int k = 0; k < 3; k++) { c.v[k] = carry->open.v[k]; c.p[k] = carry->open.p[k]; }
                c.dt = carry->open.dt; c.n_steps = carry->open.n_steps; c.flags = carry->open.flags;
                imu_compose(c, d, o);
                d = o;
            }
        }
        vis_imu_carry co;
        co.t_last = tframe[n - 1];
        imu_record(d, 0, co.open);
        co.valid = valid; co.reserved_ = 0;
        *carry_out = co;
    }
}

size_t imu_table_bytes(int n) {
    int levels = 1;
    while ((1 << levels) <= n) levels++;
    return (size_t)levels * 26 * sizeof(unsigned long long) * (size_t)(n > 0 ? n : 1);
}

int imu_launch(vis_ctx* ctx, const vis_imu_params* ip, int n, FtFrames fr, const vis_imu_sample* d_samples, int n_samples, const double* d_tframe,
            const vis_imu_carry* d_carry, void* d_ws, vis_imu_delta* d_delta, float* d_rot, vis_imu_carry* d_carry_out) {
    if (n < 1) return VIS_OK;
    if (n > VIS_IMU_MAX_FRAMES || !d_ws || n_samples < 0) return VIS_E_INVALID;
    hipLaunchKernelGGL(k_imu_intervals, dim3((n + IMU_IV_BLOCK - 1) / IMU_IV_BLOCK), dim3(IMU_IV_BLOCK), 0, ctx->stream, *ip, n, d_samples, n_samples, d_tframe,
                       d_carry, (unsigned long long*)d_ws);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_imu_pairs, dim3(1), dim3(IMU_BLOCK), 0, ctx->stream, *ip, n, fr, d_tframe, d_carry, (unsigned long long*)d_ws, d_delta, d_rot, d_carry_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
