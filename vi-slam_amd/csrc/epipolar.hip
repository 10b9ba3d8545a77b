// epipolar.hip -- the reference's own F2FRansac (VISystem::F2FRansac, src/VISystem.cpp:612-769) and FilterKeypoints (:542-610) for every
// pair of a batch on gfx950, FP64 VALU: the epipolar-plane test both share, k_f2f_batch (the translation RANSAC with the rotation given)
// and k_epi_filter.  Restated operation for operation in tests/f2f_ref.py; compared with the oracle (oracle/pose.cpp f2f_ransac) as well.
// Built like pose.hip, without the SLP vectorizer (the Makefile has the reason).
#include "vis_internal.h"
#include "ransac_lanes.h"
#include <cmath>
#include <cfloat>

// ---- the epipolar-plane test F2FRansac (src/VISystem.cpp:729-731) and FilterKeypoints (:596-598) share:
//          -1000.0 / log10(fabs(x)) < threshold,      x = a unit direction . an epipolar-plane normal
// decided by two compares wherever the outcome cannot depend on rounding, and by the expression itself (as src/VISystem.cpp:729-731
// and oracle/pose.cpp:585-586 write it: -1000.0 / log10(fabs(x)) < threshold, all in double) inside a band c_lo <= |x| <= c_hi around c = 10^(-1000 / threshold).  The result equals the full expression for EVERY x.
//
// For threshold T > 0, in exact arithmetic E(a) = -1000 / log10(a) rises from +0 (a -> 0) to +inf (a -> 1-) and is negative for a > 1, so
// E(a) < T  <=>  a < c  or  a >= 1.  The special values of the expression as the libms compute it agree with that: a = 0 gives -1000 / -inf
// = +0 < T; a = 1 gives -1000 / +0 = -inf; a > 1 gives log10 >= +0 (a faithful log10 is never negative there) and a quotient <= -0; a = inf
// gives -0; a NaN gives NaN < T = false (a NaN fails both compares below and takes the full expression).
// For 0 < a < 1 the computed value is E(a) (1 + e) with |e| <= (u_log + u_div + small) 2^-53: u_div = 1/2 (IEEE division on both sides:
// no fast-math, and a relative error of log10 turns into the same relative error of the quotient), u_log = the ulp error of log10 --
// glibc and the ROCm device library both document a bound of a few ulp (<= 2 and <= 2).  EPI_BAND_ULPS = 32 covers both with a factor of
// ten to spare.  With r = EPI_BAND_ULPS 2^-53 the computed outcome can differ from the exact one only when T / (1 + r) <= E(a) <= T / (1 - r),
// i.e. when log10(a) is within a relative r' ~ r of log10(c), i.e. when a = c^(1 +- r') = c (1 +- |ln c| r').  The band is
//          k = 2 (|ln c| + 1) r,  c_lo = c (1 - k),  c_hi = c (1 + k)
// : the + 1 covers the host's own rounding of c (pow: <= 1 ulp; the quotient -1000 / T: 1/2 ulp of the exponent = |ln c| / 2 ulp of c), the
// factor 2 is margin on top.  For T = 370 (c = 1.98e-3, |ln c| = 6.2) k = 5.1e-14: about one dot product in 1e13 takes the full expression.
// Thresholds for which that reasoning does not hold -- T <= 0 or not finite, c below 1e-290 (T < 3.45: c_lo near the denormals),
// c_hi >= 1 -- get c_lo = 0, c_hi = +inf: no |x| is below 0 or above +inf, every x takes the full expression.
#define EPI_BAND_ULPS 32.0
static void epi_band(double threshold, double* c_lo, double* c_hi) {
    *c_lo = 0.0; *c_hi = HUGE_VAL;
    if (!(threshold > 0.0) || !std::isfinite(threshold)) return;
    const double c = std::pow(10.0, -1000.0 / threshold);
    if (!(c >= 1e-290)) return;
    const double k = 2.0 * (std::fabs(std::log(c)) + 1.0) * (EPI_BAND_ULPS * 0x1p-53);
    const double lo = c * (1.0 - k), hi = c * (1.0 + k);
    if (!(lo > 0.0) || !(hi < 1.0)) return;
    *c_lo = lo; *c_hi = hi;
}
DEV bool epi_inlier(double x, double threshold, double c_lo, double c_hi) {
    const double ax = fabs(x);
    if (ax < c_lo) return true;
    if (ax > c_hi) return ax >= 1.0;
    return -1000.0 / log10(ax) < threshold;
}

// the normal of correspondence i's epipolar plane (src/VISystem.cpp:651-668, oracle/pose.cpp:565-573), expression for expression: the
// pixels to float camera coordinates ((u - cx) / fx, (v - cy) / fy, 1), widened to double, both normalised by the square root of
// (x x + y y) + z z, the second rotated by R with each row summed as (r0 b0 + r1 b1) + r2 b2, and n = a x (R b)
struct EpiCam { float fx, fy, cx, cy; };
DEV void epi_normal(const float* __restrict__ q1, const float* __restrict__ q2, int i, const EpiCam& K, const double (&Rm)[9], double* nv) {
    const float2 pa = reinterpret_cast<const float2*>(q1)[i], pb = reinterpret_cast<const float2*>(q2)[i];
    const float u1 = pa.x, v1 = pa.y, u2 = pb.x, v2 = pb.y;
    double a[3] = {(double)((u1 - K.cx) / K.fx), (double)((v1 - K.cy) / K.fy), 1.0};
    double b[3] = {(double)((u2 - K.cx) / K.fx), (double)((v2 - K.cy) / K.fy), 1.0};
    const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    for (int k = 0; k < 3; k++) { a[k] /= na; b[k] /= nb; }
    const double rb[3] = {(Rm[0] * b[0] + Rm[1] * b[1]) + Rm[2] * b[2], (Rm[3] * b[0] + Rm[4] * b[1]) + Rm[5] * b[2],
                          (Rm[6] * b[0] + Rm[7] * b[1]) + Rm[8] * b[2]};
    cross3(a, rb, nv);
}

// ---- F2FRansac for every pair of a batch in the shape of ransac_lanes.h, written out: one workgroup per pair, one launch.  (On the
// header's helpers the long-row kernel measured 0.1 ... 1.2 % slower in the pipeline, four alternations of four, with a counting loop that
// is the same instructions in other registers -- DESIGN.md section 4.13 -- so this kernel keeps its own copy of the tile walk, the key
// and the reduction; a change to the barrier protocol or the tie rule has to be made here as well.)  The iterations are
// spread over the lanes (IPL at a time per lane: one LDS read of a normal serves that many dot products), the points are walked in tiles
// of F2F_TILE normals in LDS, and the winner is taken here: the smallest iteration among those with the largest count (`if (count >
// countMax)` in iteration order, :737-741) = the maximum of the integer key (count << 32 | ~iteration) over the workgroup, whatever <NT, IPL>:
// 256 lanes x 4 iterations for rows of up to one tile (the good matches: thousands of small pairs share the chip with the detect chain),
// 512 x 2 for longer rows (VIS_POSE_SYM: tens of pairs of thousands of points, where a second wave per SIMD hides the LDS and
// branch latency of the first) -- DESIGN.md section 4.7 has both shapes measured both ways.
// vis_f2f_ransac is one pair of the same kernel with DIRECT indices (the same choice of shape).
#define F2F_TILE VIS_F2F_TILE          // 512 normals = 16 KiB of LDS (public: the tests size their rows around it)
struct F2fArgs { EpiCam K; double threshold, c_lo, c_hi; int iters, in_stride; };
struct alignas(32) EpiNv { double x, y, z, pad_; };

// hypothesis of iteration j: d = normalize(n_i1 x n_i2) with i = (draw & 0x7fffffff) % (m - 1) (rand() % (sizeNewGroup - 1), :712-713) -- or,
// DIRECT, with i = the draw as it stands (vis_f2f_ransac's sample_idx, validated to [0, m): m - 1 included, which the modulo cannot give);
// false: the cross product is zero and the iteration is skipped (:716)
template <bool DIRECT>
DEV bool f2f_hypothesis(const int32_t* __restrict__ draws, int j, int m, const EpiNv* s_nv, bool from_lds, const float* q1, const float* q2,
                        const EpiCam& K, const double (&Rm)[9], double* d) {
    const int i1 = DIRECT ? draws[2 * j] : (int)((unsigned)(draws[2 * j] & 0x7fffffff) % (unsigned)(m - 1));
    const int i2 = DIRECT ? draws[2 * j + 1] : (int)((unsigned)(draws[2 * j + 1] & 0x7fffffff) % (unsigned)(m - 1));
    double n1[3], n2[3];
    if (from_lds) { n1[0] = s_nv[i1].x; n1[1] = s_nv[i1].y; n1[2] = s_nv[i1].z; n2[0] = s_nv[i2].x; n2[1] = s_nv[i2].y; n2[2] = s_nv[i2].z; }
    else { epi_normal(q1, q2, i1, K, Rm, n1); epi_normal(q1, q2, i2, K, Rm, n2); }
    cross3(n1, n2, d);
    if (!(d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0)) return false;
    const double dn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int k = 0; k < 3; k++) d[k] /= dn;
    return true;
}

template <int NS, int IPL>
DEV void f2f_count_tile(const EpiNv* s_nv, int nt, const double (&d)[IPL][3], int (&cnt)[IPL], const F2fArgs& A) {
    static_assert(NS <= IPL, "slots");
    for (int i = 0; i < nt; i++) {
        const double n0 = s_nv[i].x, n1 = s_nv[i].y, n2 = s_nv[i].z;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const double x = (d[s][0] * n0 + d[s][1] * n1) + d[s][2] * n2;
            cnt[s] += epi_inlier(x, A.threshold, A.c_lo, A.c_hi) ? 1 : 0;
        }
    }
}

// the count over one tile for the first `nslots` of a lane's IPL iterations (a uniform number: slots beyond it hold no iteration on any lane).
// DIRECT is not used here: it gives k_f2f_batch<.., true> a dispatch chain of its own, without which the compiler inlines the shared one in
// another order and schedules the counting loop of the <.., false> kernels differently (same instructions, four scalar adds moved).
template <int NS, int IPL, bool DIRECT>
DEV void f2f_count_slots(int nslots, const EpiNv* s_nv, int nt, const double (&d)[IPL][3], int (&cnt)[IPL], const F2fArgs& A) {
    if constexpr (NS < IPL) { if (nslots > NS) { f2f_count_slots<NS + 1, IPL, DIRECT>(nslots, s_nv, nt, d, cnt, A); return; } }
    f2f_count_tile<NS, IPL>(s_nv, nt, d, cnt, A);
}

template <int NT, int IPL, bool DIRECT = false>
__global__ __launch_bounds__(NT) void k_f2f_batch(F2fArgs A, const float* __restrict__ p1, const float* __restrict__ p2,
                                                  const int32_t* __restrict__ npts, const float* __restrict__ rot,
                                                  const float* __restrict__ tref, const int32_t* __restrict__ draws,
                                                  vis_f2f_result* __restrict__ out) {
    __shared__ EpiNv s_nv[F2F_TILE];
    __shared__ unsigned long long s_key[NT / 64];
    __shared__ int s_deg[NT / 64];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(npts[pair], 0), A.in_stride);
    vis_f2f_result r;
    r.t[0] = r.t[1] = r.t[2] = 0.f; r.count_max = 0; r.n_points = 0; r.best_iter = -1; r.n_degenerate = 0; r.flipped = 0;
    if (m < 2 || A.iters <= 0) { if (tid == 0) out[pair] = r; return; }             // (uniform: the whole workgroup leaves)
    const float* q1 = p1 + (size_t)pair * A.in_stride * 2;
    const float* q2 = p2 + (size_t)pair * A.in_stride * 2;
    double Rm[9];
    for (int i = 0; i < 9; i++) Rm[i] = (double)rot[9 * (size_t)pair + i];
    const bool single = m <= F2F_TILE;                             // one tile: filled once, and the hypotheses take their normals from it
    if (single) {
        for (int i = tid; i < m; i += NT) { double nv[3]; epi_normal(q1, q2, i, A.K, Rm, nv); s_nv[i].x = nv[0]; s_nv[i].y = nv[1]; s_nv[i].z = nv[2]; }
        __syncthreads();
    }
    unsigned long long best = 0;                                   // 0: no iteration with a count > 0 yet
    int ndeg = 0;
    for (int j0 = 0; j0 < A.iters; j0 += NT * IPL) {
        double d[IPL][3]; int cnt[IPL]; bool live[IPL];
#pragma unroll
        for (int s = 0; s < IPL; s++) {
            const int j = j0 + s * NT + tid;
            cnt[s] = 0; d[s][0] = d[s][1] = d[s][2] = 0.0;
            live[s] = j < A.iters;
            if (live[s]) { live[s] = f2f_hypothesis<DIRECT>(draws, j, m, s_nv, single, q1, q2, A.K, Rm, d[s]); if (!live[s]) { ndeg++; d[s][0] = d[s][1] = d[s][2] = 0.0; } }
        }
        const int nslots = min(IPL, (A.iters - j0 + NT - 1) / NT);      // slots that hold an iteration on any lane
        const bool wave_live = j0 + (tid & ~63) < A.iters;          // (wave-uniform) a wave whose lanes hold no iteration only keeps the barriers
        for (int t0 = 0; t0 < m; t0 += F2F_TILE) {
            const int nt = min(F2F_TILE, m - t0);
            if (!single) {
                __syncthreads();                                   // the tile before has been read by every wave
                for (int i = tid; i < nt; i += NT) { double nv[3]; epi_normal(q1, q2, t0 + i, A.K, Rm, nv); s_nv[i].x = nv[0]; s_nv[i].y = nv[1]; s_nv[i].z = nv[2]; }
                __syncthreads();
            }
            if (wave_live) {
                f2f_count_slots<1, IPL, DIRECT>(nslots, s_nv, nt, d, cnt, A);
            }
        }
#pragma unroll
        for (int s = 0; s < IPL; s++) {                        // a lane's iterations in rising order
            const int j = j0 + s * NT + tid;
            const unsigned long long key = ((unsigned long long)(unsigned)cnt[s] << 32) | (unsigned)(0x7fffffff - j);
            if (live[s] && cnt[s] > 0 && key > best) best = key;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
        ndeg += __shfl_xor(ndeg, off);
    }
    if ((tid & 63) == 0) { s_key[tid >> 6] = best; s_deg[tid >> 6] = ndeg; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NT / 64; w++) { best = s_key[w] > best ? s_key[w] : best; ndeg += s_deg[w]; }
    r.n_points = m; r.n_degenerate = ndeg;
    if (best != 0) {
        const int it = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
        double d[3];
        (void)f2f_hypothesis<DIRECT>(draws, it, m, s_nv, false, q1, q2, A.K, Rm, d);        // the same expression: the same bits as the lane that counted it
        float scale = 1.0f, g[3] = {0.f, 0.f, 0.f};
        if (tref) { for (int k = 0; k < 3; k++) g[k] = tref[3 * (size_t)pair + k]; scale = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]); }   // :639-642
        float t[3] = {scale * (float)d[0], scale * (float)d[1], scale * (float)d[2]};
        if (tref && (t[0] * g[0] + t[1] * g[1]) + t[2] * g[2] < 0.f) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; r.flipped = 1; }       // :524-527
        r.t[0] = t[0]; r.t[1] = t[1]; r.t[2] = t[2];
        r.count_max = (int)(best >> 32); r.best_iter = it;
    }
    out[pair] = r;
}

// ---- FilterKeypoints (src/VISystem.cpp:542-610) for every correspondence of every pair: keep[k] = the test above on tVec . normal_k.
// tVec = (double)t / sqrt of its double sum of squares (:565-568): a zero translation makes it NaN, every dot product NaN, nothing is kept.
__global__ __launch_bounds__(256) void k_epi_filter(F2fArgs A, int row_cap, const float* __restrict__ p1, const float* __restrict__ p2,
                                                    const int32_t* __restrict__ npts, const float* __restrict__ rot,
                                                    const float* __restrict__ tr, uint8_t* __restrict__ keep, int32_t* __restrict__ nkeep) {
    __shared__ int s_cnt[4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(npts[pair], 0), A.in_stride);
    const float* q1 = p1 + (size_t)pair * A.in_stride * 2;
    const float* q2 = p2 + (size_t)pair * A.in_stride * 2;
    double Rm[9];
    for (int i = 0; i < 9; i++) Rm[i] = (double)rot[9 * (size_t)pair + i];
    double tv[3] = {(double)tr[3 * (size_t)pair], (double)tr[3 * (size_t)pair + 1], (double)tr[3 * (size_t)pair + 2]};
    const double tn = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
    for (int k = 0; k < 3; k++) tv[k] /= tn;
    int cnt = 0;
    for (int i = tid; i < m; i += 256) {
        double nv[3];
        epi_normal(q1, q2, i, A.K, Rm, nv);
        const bool k = epi_inlier((tv[0] * nv[0] + tv[1] * nv[1]) + tv[2] * nv[2], A.threshold, A.c_lo, A.c_hi);
        keep[(size_t)pair * row_cap + i] = k ? 1 : 0;
        cnt += k ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) nkeep[pair] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

static F2fArgs epi_args(const vis_ctx* ctx, double threshold, int iters, int in_stride) {
    F2fArgs A;
    A.K = {(float)ctx->p.fx, (float)ctx->p.fy, (float)ctx->p.cx, (float)ctx->p.cy};
    A.threshold = threshold;
    epi_band(threshold, &A.c_lo, &A.c_hi);
    A.iters = iters; A.in_stride = in_stride;
    return A;
}

// d_p1 / d_p2: npairs rows of in_stride (x, y) points, d_npts of them valid (clamped to in_stride); d_rot: npairs x 9; d_tref: npairs x 3 or
// null; d_draws: iters x 2 (direct: point indices in [0, m), see f2f_hypothesis); d_out: npairs records.  On ctx->stream.
template <bool DIRECT>
static void f2f_launch(vis_ctx* ctx, const F2fArgs& A, int npairs, const float* d_p1, const float* d_p2, const int32_t* d_npts,
                       const float* d_rot, const float* d_tref, const int32_t* d_draws, vis_f2f_result* d_out) {
    if (A.in_stride > F2F_TILE) hipLaunchKernelGGL((k_f2f_batch<512, 2, DIRECT>), dim3(npairs), dim3(512), 0, ctx->stream, A, d_p1, d_p2, d_npts, d_rot, d_tref, d_draws, d_out);
    else hipLaunchKernelGGL((k_f2f_batch<256, 4, DIRECT>), dim3(npairs), dim3(256), 0, ctx->stream, A, d_p1, d_p2, d_npts, d_rot, d_tref, d_draws, d_out);
}
int f2f_batch_run(vis_ctx* ctx, int npairs, int in_stride, const float* d_p1, const float* d_p2, const int32_t* d_npts,
                  const float* d_rot, const float* d_tref, const int32_t* d_draws, int iters, bool direct, vis_f2f_result* d_out) {
    if (npairs <= 0) return VIS_OK;
    const F2fArgs A = epi_args(ctx, ctx->p.f2f_threshold, iters, in_stride);
    if (direct) f2f_launch<true>(ctx, A, npairs, d_p1, d_p2, d_npts, d_rot, d_tref, d_draws, d_out);
    else f2f_launch<false>(ctx, A, npairs, d_p1, d_p2, d_npts, d_rot, d_tref, d_draws, d_out);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

// the same rows; d_t: npairs x 3; d_keep: npairs rows of row_cap >= in_stride bytes; d_nkeep: npairs.  On ctx->stream.
int epi_filter_run(vis_ctx* ctx, int npairs, int in_stride, const float* d_p1, const float* d_p2, const int32_t* d_npts,
                   const float* d_rot, const float* d_t, double threshold, int row_cap, uint8_t* d_keep, int32_t* d_nkeep) {
    if (npairs <= 0) return VIS_OK;
    const F2fArgs A = epi_args(ctx, threshold, 0, in_stride);
    hipLaunchKernelGGL(k_epi_filter, dim3(npairs), dim3(256), 0, ctx->stream, A, row_cap, d_p1, d_p2, d_npts, d_rot, d_t, d_keep, d_nkeep);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
