// align.hip -- VISystem::EstimatePoseFeatures on gfx950 (MI355X): batched Gauss-Newton photometric alignment.
//
// Replaces the pose step VISystemGPU::AddFrameGPU calls (/root/reference/src/VISystemGPU.cpp:167):
//   VISystem::EstimatePoseFeatures  /root/reference/src/VISystem.cpp:1113-1448
//   VISystem::WarpFunctionSE3       /root/reference/src/VISystem.cpp:1495-1558
//   VISystem::InitializePyramid     /root/reference/src/VISystem.cpp:1451-1493
// (SURVEY.md 8(f) N4).  It consumes what the N2 stage already produces on the device: the half pyramid, the Scharr
// gradients and the matched keypoints of the previous keyframe.
//
// Design: the algorithm is a strictly sequential chain of <= 4 levels x <= 10 iterations per frame pair, each iteration
// a reduction over a few thousand candidate pixels.  ONE persistent workgroup (4 waves) owns a pair for the whole
// chain: no host round trip and no kernel boundary between iterations, the pose lives in registers, the 27 sums of
// the normal equations are reduced with wave shuffles + 864 bytes of LDS, thread 0 solves the 6x6 system in LDS.
// Pairs are independent -> grid = pairs (1023 workgroups per 1024-frame batch).  In the batched path the candidate
// pixels of a level (the (2p+1)^2 patches around the matched keypoints, src/Camera.cpp:358-410) are generated once
// per level into LDS as packed (y << 16 | x) words instead of being streamed from a 16-byte-per-point list in HBM
// (95 KB per pair and level, re-read every iteration).  Image / gradient reads are scattered 1-5 byte gathers inside
// small patches: L2 hits after the first iteration.  Bound: FP64/FP32 VALU latency of one workgroup per pair.
//
// Arithmetic (operation order, float/double widths, summation tree) mirrors oracle/align.cpp exactly; the results are
// bit-identical to it (tests/test_align_gpu.py).
#include "vis_internal.h"
#include <cfloat>
#include <cmath>
#include <cstring>

#define DEV __device__ __forceinline__
#define AL_THREADS 256
#define AL_MAXKP 200                     // min(num_max_keypoints, 200), src/Camera.cpp:377

struct AlignLevel {
    const uint8_t* i1; const uint8_t* i2;          // level image of frame 0 of the batch (previous / current use frame offsets)
    const int16_t* gx; const int16_t* gy;
    const float* cand;                             // explicit list (x, y, z, w) rows, or nullptr (generated)
    size_t img_fstride, grad_fstride;              // elements between consecutive frames
    int rowstride, cols, rows, ncand;              // cols, rows: the reference's bookkeeping w_[lvl], h_[lvl] = size >> lvl (bounds of the coordinates)
    int acols, arows;                              // the level's own size (Camera::Update: cvRound(size * 0.5)): stride of the dense gradients, clamp of the rounded index
    float fx, fy, cx, cy, invfx, invfy;
};
struct AlignArgs {
    AlignLevel lv[5];
    int first, last, max_it; float eps, zf;
    const float* pts; const int32_t* npts; int max_pts;   // generated mode: matched keypoints of the previous frame per pair
    const vis_se3f* init; vis_align_result* out;
    int f1_off, f2_off, out_off;                          // frame index of image 1 / image 2 / result slot = pair + offset
    const int32_t* prev;                                  // generated mode, keyframe gate: image 1 = frame prev[slot]; < 0: no pair (record left as cleared)
    // vis_batch_track: image 1 of a pair whose previous frame is VIS_KF_CARRIED (an earlier launch) is the plan's keyframe snapshot,
    // one frame in the layout of a gradient set with a dense level 0 (track.hip); nullptr: such a pair is skipped like any link < 0
    const uint8_t* c_gray; const int16_t* c_gx; const int16_t* c_gy;
    int wmode; float tukey_b, mad_scale;                  // vis_align_weights of the context when the call was made (k_align<*, true> reads them)
};

#include "se3_core.h"
#include "patch_window.h"

// hal::LU32f as cv::invert(DECOMP_LU) uses it: A (6x6, row-major, LDS) -> B = inverse; false = singular.  The matrices are
// held in registers for the factorisation (fully unrolled; a row exchange with the runtime pivot row is a chain of selects):
// the same operations in the same order as the in-place version, without ~800 dependent LDS round trips of one thread.
__device__ bool lu_invert6(const float* Ain, float* Bout) {
    constexpr int n = 6;
    float A[n][n], B[n][n];
#pragma unroll
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < n; j++) { A[i][j] = Ain[i * n + j]; B[i][j] = i == j ? 1.f : 0.f; }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < n; i++) {
        int k = i; float best = fabsf(A[i][i]);
#pragma unroll
        for (int j = i + 1; j < n; j++) { const float v = fabsf(A[j][i]); if (v > best) { best = v; k = j; } }
        if (best < FLT_EPSILON * 10) ok = false;
#pragma unroll
        for (int j = i + 1; j < n; j++)
            if (k == j) {
#pragma unroll
                for (int c = i; c < n; c++) { const float t = A[i][c]; A[i][c] = A[j][c]; A[j][c] = t; }
#pragma unroll
                for (int c = 0; c < n; c++) { const float t = B[i][c]; B[i][c] = B[j][c]; B[j][c] = t; }
            }
        const float d = -1.f / A[i][i];
#pragma unroll
        for (int j = i + 1; j < n; j++) {
            const float alpha = A[j][i] * d;
#pragma unroll
            for (int c = i + 1; c < n; c++) A[j][c] += alpha * A[i][c];
#pragma unroll
            for (int c = 0; c < n; c++) B[j][c] += alpha * B[i][c];
        }
    }
#pragma unroll
    for (int i = n - 1; i >= 0; i--)
#pragma unroll
        for (int j = 0; j < n; j++) {
            float s_ = B[i][j];
#pragma unroll
            for (int k = i + 1; k < n; k++) s_ -= A[i][k] * B[k][j];
            B[i][j] = s_ / A[i][i];
        }
#pragma unroll
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < n; j++) Bout[i * n + j] = B[i][j];
    return ok;
}

// sum over the 64 lanes of a wave in the oracle's tree order (stride 32, 16, ... 1): lane 0 holds the result
DEV double wave_tree_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
DEV unsigned long long wave_tree_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// k_align<*, true>, statistics pass: WarpFunctionSE3 and the validity tests of one candidate exactly as the accumulation loop of
// k_align runs them (the same operations in the same order: both passes of an iteration must see the same residual list) -> the
// offsets of its two intensities; false = the candidate is skipped.  M = rows 0..2 of pose.matrix().
template <bool GEN>
DEV bool warp_offsets(const AlignLevel& V, const uint32_t* plist, int i, const double M[12], int rs1, size_t& o1, size_t& o2) {
    float x1, y1, z1, w1;
    if (GEN) { const uint32_t pw = plist[i]; x1 = (float)(pw & 0xFFFFu); y1 = (float)(pw >> 16); z1 = 1.f; w1 = 1.f; }
    else { const float4 c = reinterpret_cast<const float4*>(V.cand)[i]; x1 = c.x; y1 = c.y; z1 = c.z; w1 = c.w; }
    const float X = ((x1 - V.cx) * V.invfx) * z1, Y = ((y1 - V.cy) * V.invfy) * z1;
    const float P0 = (float)(((M[0] * (double)X + M[1] * (double)Y) + M[2] * (double)z1) + M[3] * (double)w1);
    const float P1 = (float)(((M[4] * (double)X + M[5] * (double)Y) + M[6] * (double)z1) + M[7] * (double)w1);
    const float P2 = (float)(((M[8] * (double)X + M[9] * (double)Y) + M[10] * (double)z1) + M[11] * (double)w1);
    const float P3 = (float)(((0.0 * (double)X + 0.0 * (double)Y) + 0.0 * (double)z1) + 1.0 * (double)w1);
    float x2 = P0 * V.fx; x2 = x2 / P2; x2 = x2 + V.cx;
    float y2 = P1 * V.fy; y2 = y2 / P2; y2 = y2 + V.cy;
    x2 = x2 * P3; y2 = y2 * P3;
    int ix1 = 0, iy1 = 0;
    if (!((y2 > 0 && y2 < V.arows && x2 > 0 && x2 < V.acols) && (P2 != 0))) return false;
    if (!source_index(x1, V.cols, ix1) || !source_index(y1, V.rows, iy1)) return false;
    int rx = (int)roundf(x2), ry = (int)roundf(y2);
    if (rx > V.acols - 1) rx = V.acols - 1;
    if (ry > V.arows - 1) ry = V.arows - 1;
    o1 = (size_t)iy1 * rs1 + ix1; o2 = (size_t)ry * V.rowstride + rx;
    return true;
}

#define AL_WBINS 512                     // residuals are intensity2 - intensity1 = -255 ... 255: bin r + 255 (bin 511 stays empty)

// One workgroup per frame pair; GEN = candidate pixels generated from the matched keypoints (batched path),
// otherwise read from an explicit (x, y, z, w) list (single-pair entry point: Frame::candidatePoints as the caller holds it).
// WT = VISystem::TukeyFunctionWeights (src/VISystem.cpp:1797-1870) instead of IdentityWeights in the Gauss-Newton step
// (:1342-1409): every iteration first counts the residuals of its candidates (one warp pass, a 511-bin histogram per wave), takes
// both medians of MedianAbsoluteDeviation from the counts, and tabulates the weight of every possible residual; the accumulation
// pass that follows is the identity one with a table lookup per residual.  The identity instantiations hold none of this.
template <bool GEN, bool WT>
__global__ __launch_bounds__(AL_THREADS) void k_align(AlignArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* plist = reinterpret_cast<uint32_t*>(smem);                 // GEN: packed candidate pixels of the level
    __shared__ double s_red[4][28];
    __shared__ unsigned long long s_sq[4];
    __shared__ int s_cnt[4];
    __shared__ float s_A[36], s_Ainv[36], s_delta[6];
    __shared__ int s_pre[AL_THREADS + 1];
    __shared__ int s_ok;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pair = blockIdx.x;
    const int f1 = G.prev ? G.prev[pair + G.out_off] : pair + G.f1_off, f2 = pair + G.f2_off;
    const bool carried = f1 == VIS_KF_CARRIED && G.c_gray != nullptr;
    if (f1 < 0 && !carried) return;                                      // (uniform: the whole workgroup)
    Se3 pose = {{1.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (G.init) {
        const vis_se3f in = G.init[pair + G.out_off];
        pose.q.w = in.qw; pose.q.x = in.qx; pose.q.y = in.qy; pose.q.z = in.qz; pose.t[0] = in.tx; pose.t[1] = in.ty; pose.t[2] = in.tz;
    }
    vis_align_result res;
    if (tid == 0) {
        for (int l = 0; l < 5; l++) { res.error[l] = 0.f; res.iterations[l] = 0; res.n_residuals[l] = 0; }
        res.initial_error = 0.f;
    }
    float initial_error = 0.f;
    const int m = GEN ? min(min(G.npts[pair + G.out_off], G.max_pts), AL_MAXKP) : 0;
    const float* kp = GEN ? G.pts + (size_t)(pair + G.out_off) * G.max_pts * 2 : nullptr;
#pragma unroll 1
    for (int lvl = G.first; lvl >= G.last; lvl--) {
        const AlignLevel V = G.lv[lvl];
        const int cols = V.cols, rows = V.rows;
        int N = V.ncand;
        if (GEN) {
            // Camera::ObtainPatchesPointsPreviousFrame (src/Camera.cpp:358-410) for this level, into LDS
            const int patch_size = lvl == 1 ? 3 : (lvl == 2 ? 2 : 5);
            const int sp = patch_size - 1 / 2;                                      // :376, integer 1/2 == 0
            const float factor_lvl = (float)(1.0 / (double)(1 << lvl));
            // the window of a keypoint, clamped to the level before any float becomes an int (patch_window.h): a coordinate that is NaN,
            // infinite or beyond int's range gives an empty one, where the reference's loop would not end
            PatchSpan wx = {1, 0}, wy = {1, 0}; int cnt = 0;
            if (tid < m) {
                const float x = (float)(((double)kp[2 * tid] + 0.5) * (double)factor_lvl - 0.5);
                const float y = (float)(((double)kp[2 * tid + 1] + 0.5) * (double)factor_lvl - 0.5);
                wx = patch_span(x, sp, cols); wy = patch_span(y, sp, rows);
                cnt = patch_span_count(wx) * patch_span_count(wy);
            }
            __syncthreads();                                                         // previous level done with plist / s_pre
            // exclusive prefix of the per-keypoint counts: wave scans by shuffles + the three wave totals (one thread walking
            // the 256 entries was 256 dependent LDS round trips per level)
            {
                int v = cnt;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
                if (lane == 63) s_cnt[wv] = v;
                __syncthreads();
                int base = 0;
                for (int w = 0; w < wv; w++) base += s_cnt[w];
                s_pre[tid + 1] = base + v;
                if (tid == 0) s_pre[0] = 0;
                __syncthreads();
            }
            if (tid < m) {
                int o = s_pre[tid];
                if (cnt)
                    for (int i = wx.lo; i <= wx.hi; i++)
                        for (int j = wy.lo; j <= wy.hi; j++) plist[o++] = ((uint32_t)j << 16) | (uint32_t)i;
            }
            N = s_pre[AL_THREADS];
            __syncthreads();
        }
        const size_t coff = (size_t)(V.gx - G.lv[0].gx);                     // the level's place in a frame of the set (snapshot: the same)
        const uint8_t* I1 = carried ? G.c_gray + coff : V.i1 + (size_t)f1 * V.img_fstride;
        const uint8_t* I2 = V.i2 + (size_t)f2 * V.img_fstride;
        const int16_t* GX = carried ? G.c_gx + coff : V.gx + (size_t)f1 * V.grad_fstride;
        const int16_t* GY = carried ? G.c_gy + coff : V.gy + (size_t)f1 * V.grad_fstride;
        const int rs1 = carried ? V.acols : V.rowstride;                         // (the snapshot's level 0 is dense)
        const float fx = V.fx, fy = V.fy, cx = V.cx, cy = V.cy, invfx = V.invfx, invfy = V.invfy;
        float error = 0.f, last_error = 50000.f;
        int k = 0, nres = 0;
#pragma unroll 1
        for (k = 0; k < G.max_it; k++) {
            float R[9]; qmat(pose.q, R);
            // rows 0..2 of pose.matrix(); row 3 = (0 0 0 1)
            const double m00 = R[0], m01 = R[1], m02 = R[2], m03 = pose.t[0];
            const double m10 = R[3], m11 = R[4], m12 = R[5], m13 = pose.t[1];
            const double m20 = R[6], m21 = R[7], m22 = R[8], m23 = pose.t[2];
            constexpr int NS = WT ? 28 : 27;                                        // WT: + the weighted squared error (not a sum of integers any more)
            double S[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) S[s] = 0.0;
            unsigned long long sumsq = 0; int cnt = 0;
            [[maybe_unused]] const float* wtab = nullptr;
            if constexpr (WT) {
                __shared__ int s_hist[4][AL_WBINS];                                 // one histogram per wave: residuals pile up around 0
                __shared__ int s_cum[AL_WBINS];                                     // s_cum[j] = residuals <= j - 255
                __shared__ float s_wtab[AL_WBINS];
                __shared__ int s_wsum[4], s_stat[2];
                for (int j = tid; j < 4 * AL_WBINS; j += AL_THREADS) (&s_hist[0][0])[j] = 0;
                if (tid == 0) { s_stat[0] = 0; s_stat[1] = 0; }
                __syncthreads();
                const double M[12] = {m00, m01, m02, m03, m10, m11, m12, m13, m20, m21, m22, m23};
#pragma unroll 1
                for (int i0 = tid; i0 < N; i0 += 4 * AL_THREADS) {                  // four candidates per round, like the accumulation
                    bool ok[4]; int a1[4], a2[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int i = i0 + u * AL_THREADS;
                        size_t o1 = 0, o2 = 0;
                        ok[u] = i < N && warp_offsets<GEN>(V, plist, i, M, rs1, o1, o2);
                        a1[u] = I1[o1]; a2[u] = I2[o2];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) if (ok[u]) atomicAdd(&s_hist[wv][a2[u] - a1[u] + 255], 1);
                }
                __syncthreads();
                {   // the four histograms added and their running count (thread = two bins; wave scan + the wave totals)
                    const int h0 = (s_hist[0][2 * tid] + s_hist[1][2 * tid]) + (s_hist[2][2 * tid] + s_hist[3][2 * tid]);
                    const int h1 = (s_hist[0][2 * tid + 1] + s_hist[1][2 * tid + 1]) + (s_hist[2][2 * tid + 1] + s_hist[3][2 * tid + 1]);
                    int v = h0 + h1;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
                    if (lane == 63) s_wsum[wv] = v;
                    __syncthreads();
                    for (int w = 0; w < wv; w++) v += s_wsum[w];
                    s_cum[2 * tid] = v - h1; s_cum[2 * tid + 1] = v;
                    __syncthreads();
                }
                // MedianMat (:1846-1870): the first bin whose running count exceeds (float)(n / 2) -- counts are < 2^24, so the float
                // comparison is the integer one.  The running count rises with the bin: exactly one bin sees the crossing.
                const int half = s_cum[AL_WBINS - 1] / 2;
                const bool as_written = G.wmode == VIS_W_TUKEY;                     // CV_8U saturation of both MedianMat calls
#pragma unroll
                for (int j = 2 * tid; j < 2 * tid + 2; j++)
                    if (s_cum[j] > half && (j == 0 || s_cum[j - 1] <= half)) s_stat[0] = j - 255;
                __syncthreads();
                // as written every negative residual counts in bin 0: the median of max(r, 0) = max(signed median, 0)
                const int med = as_written ? max(s_stat[0], 0) : s_stat[0];
                // |r - med| <= d  <=>  med - d <= r <= med + d: the running count of the deviations from the one of the residuals
                auto dev_count = [&](int d) {
                    const int hi = min(med + d, 255) + 255, lo = max(med - d, -255) + 255;
                    return s_cum[hi] - (lo > 0 ? s_cum[lo - 1] : 0);
                };
#pragma unroll
                for (int d = 2 * tid; d < 2 * tid + 2; d++)
                    if (d <= 510 && dev_count(d) > half && (d == 0 || dev_count(d - 1) <= half)) s_stat[1] = d;
                __syncthreads();
                const int dev = as_written ? min(s_stat[1], 255) : s_stat[1];       // (deviations of 256 ... 510 saturate to 255)
                float MAD = G.mad_scale * (float)dev;
                if (MAD == 0) MAD = 1;
                const float b = G.tukey_b;
                const float inv_MAD = (float)(1.0 / MAD), inv_b2 = (float)(1.0 / (b * b));
                for (int j = tid; j < AL_WBINS; j += AL_THREADS) {
                    const float x = (float)(j - 255) * inv_MAD;
                    float w = 0.f;
                    if (fabsf(x) <= b) { const float t = (float)(1.0 - (double)((x * x) * inv_b2)); w = t * t; }
                    s_wtab[j] = w;
                }
                __syncthreads();
                wtab = s_wtab;
            }
            // Four candidates per thread per round: first the warp of all four and their image / gradient loads (clamped
            // addresses for the ones that will be skipped), then the accumulation in the original order i, i + T, i + 2T,
            // i + 3T -- the per-thread sums see the same operations in the same order, but a round costs one memory round
            // trip instead of four.
#pragma unroll 1
            for (int i0 = tid; i0 < N; i0 += 4 * AL_THREADS) {
                float x2a[4], y2a[4], iza[4]; bool ok[4]; int i1v[4], i2v[4]; float gxv[4], gyv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + u * AL_THREADS;
                    ok[u] = false; x2a[u] = y2a[u] = iza[u] = 0.f;
                    size_t o1 = 0, o2 = 0, go = 0;
                    if (i < N) {
                        float x1, y1, z1, w1;
                        if (GEN) { const uint32_t pw = plist[i]; x1 = (float)(pw & 0xFFFFu); y1 = (float)(pw >> 16); z1 = 1.f; w1 = 1.f; }
                        else { const float4 c = reinterpret_cast<const float4*>(V.cand)[i]; x1 = c.x; y1 = c.y; z1 = c.z; w1 = c.w; }
                        const float X = ((x1 - cx) * invfx) * z1, Y = ((y1 - cy) * invfy) * z1;
                        const float P0 = (float)(((m00 * (double)X + m01 * (double)Y) + m02 * (double)z1) + m03 * (double)w1);
                        const float P1 = (float)(((m10 * (double)X + m11 * (double)Y) + m12 * (double)z1) + m13 * (double)w1);
                        const float P2 = (float)(((m20 * (double)X + m21 * (double)Y) + m22 * (double)z1) + m23 * (double)w1);
                        const float P3 = (float)(((0.0 * (double)X + 0.0 * (double)Y) + 0.0 * (double)z1) + 1.0 * (double)w1);
                        float x2 = P0 * fx; x2 = x2 / P2; x2 = x2 + cx;
                        float y2 = P1 * fy; y2 = y2 / P2; y2 = y2 + cy;
                        x2 = x2 * P3; y2 = y2 * P3;
                        const float z2 = P2;
                        float inv_z2 = 1 / z2;
                        int ix1 = 0, iy1 = 0;
                        const bool src_in = source_index(x1, cols, ix1) && source_index(y1, rows, iy1);   // (int)x1, (int)y1 where they index the level
                        // the warped point is tested against the size of the Mat it indexes (src/VISystem.cpp:1299: image2.rows / image2.cols
                        // = Camera::Update's level size, up to one row / column MORE than the bookkeeping `size >> lvl`)
                        bool v = (y2 > 0 && y2 < V.arows && x2 > 0 && x2 < V.acols) && (z2 != 0);
                        if (inv_z2 < 0) inv_z2 = 0;
                        v = v && src_in;
                        if (v) {
                            int rx = (int)roundf(x2), ry = (int)roundf(y2);
                            if (rx > V.acols - 1) rx = V.acols - 1;
                            if (ry > V.arows - 1) ry = V.arows - 1;
                            o1 = (size_t)iy1 * rs1 + ix1; o2 = (size_t)ry * V.rowstride + rx; go = (size_t)iy1 * V.acols + ix1;   // gradients are dense
                        }
                        ok[u] = v; x2a[u] = x2; y2a[u] = y2; iza[u] = inv_z2;
                    }
                    i1v[u] = I1[o1]; i2v[u] = I2[o2]; gxv[u] = (float)GX[go]; gyv[u] = (float)GY[go];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!ok[u]) continue;
                    const float x2 = x2a[u], y2 = y2a[u], inv_z2 = iza[u];
                    float Jw0[6], Jw1[6];
                    Jw0[0] = fx * inv_z2; Jw0[1] = 0.f;
                    Jw0[2] = -(fx * x2 * inv_z2 * inv_z2) * G.zf;
                    Jw0[3] = -(fx * x2 * y2 * inv_z2 * inv_z2);
                    Jw0[4] = (fx * (1 + x2 * x2 * inv_z2 * inv_z2));
                    Jw0[5] = -fx * y2 * inv_z2;
                    Jw1[0] = 0.f; Jw1[1] = fy * inv_z2;
                    Jw1[2] = -(fy * y2 * inv_z2 * inv_z2) * G.zf;
                    Jw1[3] = -(fy * (1 + y2 * y2 * inv_z2 * inv_z2));
                    Jw1[4] = fy * x2 * y2 * inv_z2 * inv_z2;
                    Jw1[5] = -fy * x2 * inv_z2;
                    const int ri = i2v[u] - i1v[u];
                    const float resf = (float)ri;
                    const float jl0 = gxv[u], jl1 = gyv[u];
                    double J[6];
#pragma unroll
                    for (int c = 0; c < 6; c++) J[c] = (double)(float)((double)jl0 * (double)Jw0[c] + (double)jl1 * (double)Jw1[c]);
                    float rhs = resf;
                    if constexpr (WT) {                                             // W enters the row and the residual (:1346-1409)
                        const float wgt = wtab[ri + 255];
#pragma unroll
                        for (int c = 0; c < 6; c++) J[c] = (double)(wgt * (float)J[c]);
                        rhs = resf * wgt;
                        S[27] += (double)resf * (double)rhs;
                    }
                    int s = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int b = a; b < 6; b++) S[s++] += J[a] * J[b];
#pragma unroll
                    for (int a = 0; a < 6; a++) S[21 + a] += J[a] * (double)rhs;
                    if constexpr (!WT) sumsq += (unsigned long long)(ri * ri);
                    cnt++;
                }
            }
            // reduction in the oracle's order: inside a wave strides 32..1, then (W0 + W1) + (W2 + W3)
#pragma unroll
            for (int s = 0; s < NS; s++) { const double v = wave_tree_sum(S[s]); if (lane == 0) s_red[wv][s] = v; }
            if constexpr (!WT) { const unsigned long long q = wave_tree_sum_u64(sumsq); if (lane == 0) s_sq[wv] = q; }
            { int c = cnt; for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64); if (lane == 0) s_cnt[wv] = c; }
            __syncthreads();
            nres = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            unsigned long long tsq = 0;
            if constexpr (!WT) tsq = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
            if (nres == 0) { __syncthreads(); break; }
            const float inv_num = (float)(1.0 / nres);
            if constexpr (WT) error = (float)((double)inv_num * ((s_red[0][27] + s_red[1][27]) + (s_red[2][27] + s_red[3][27])));
            else error = (float)((double)inv_num * (double)tsq);
            if (k == 0) initial_error = error;
            if (error >= last_error || k == G.max_it - 1 || fabsf(error - last_error) < G.eps) { __syncthreads(); break; }
            last_error = error;
            if (tid == 0) {
                float b[6];
                int s = 0;
                for (int a = 0; a < 6; a++)
                    for (int c = a; c < 6; c++) { const float v = (float)((s_red[0][s] + s_red[1][s]) + (s_red[2][s] + s_red[3][s])); s_A[6 * a + c] = v; s_A[6 * c + a] = v; s++; }
                for (int a = 0; a < 6; a++) b[a] = (float)(-((s_red[0][21 + a] + s_red[1][21 + a]) + (s_red[2][21 + a] + s_red[3][21 + a])));
                if (!lu_invert6(s_A, s_Ainv)) for (int i = 0; i < 36; i++) s_Ainv[i] = 0.f;
                for (int a = 0; a < 6; a++) { double acc = 0; for (int c = 0; c < 6; c++) acc += (double)s_Ainv[6 * a + c] * (double)b[c]; s_delta[a] = (float)acc; }
            }
            __syncthreads();
            float delta[6];
#pragma unroll
            for (int a = 0; a < 6; a++) delta[a] = s_delta[a];
            pose = se3_mul(pose, se3_exp(delta));
            __syncthreads();                                                        // s_red / s_delta are rewritten next iteration
        }
        if (tid == 0) { res.iterations[lvl] = k; res.error[lvl] = error; res.n_residuals[lvl] = nres; }
    }
    if (tid == 0) {
        res.initial_error = initial_error;
        res.pose.qx = pose.q.x; res.pose.qy = pose.q.y; res.pose.qz = pose.q.z; res.pose.qw = pose.q.w;
        res.pose.tx = pose.t[0]; res.pose.ty = pose.t[1]; res.pose.tz = pose.t[2];
        float R[9]; qmat(pose.q, R);
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) res.matrix[4 * i + j] = R[3 * i + j]; res.matrix[4 * i + 3] = pose.t[i]; }
        res.matrix[12] = res.matrix[13] = res.matrix[14] = 0.f; res.matrix[15] = 1.f;
        G.out[pair + G.out_off] = res;
    }
    (void)s_ok;
}

// ------------------------------------------------------------------------------------------------ host side
// Sophus::SE3f value operations for the host adapters (VISystem::Track composes poses, src/VISystem.cpp:1567-1635): the same
// functions the kernel runs, evaluated on the host.
extern "C" void vis_se3_exp(const float a[6], vis_se3f* out) { const float v[6] = {a[0], a[1], a[2], a[3], a[4], a[5]}; from_se3(se3_exp(v), out); }
extern "C" void vis_se3_mul(const vis_se3f* a, const vis_se3f* b, vis_se3f* out) { from_se3(se3_mul(to_se3(*a), to_se3(*b)), out); }
extern "C" void vis_se3_matrix(const vis_se3f* a, float M[16]) {
    float R[9]; qmat(to_se3(*a).q, R);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[4 * i + j] = R[3 * i + j];
    M[3] = a->tx; M[7] = a->ty; M[11] = a->tz; M[12] = M[13] = M[14] = 0.f; M[15] = 1.f;
}
extern "C" void vis_se3_from_rt(const float R[9], const float t[3], vis_se3f* out) { se3_from_rt_f(R, t, out); }

extern "C" void vis_default_align_params(vis_align_params* ap) {
    if (!ap) return;
    std::memset(ap, 0, sizeof(*ap));
    ap->fx = 458.654f; ap->fy = 457.296f; ap->cx = 367.215f; ap->cy = 248.375f;     // calibrationEUROC.xml:20
    ap->first_level = 3; ap->last_level = 0; ap->max_iterations = 10;                // src/VISystem.cpp:1117,1119,1120
    ap->epsilon = 0.001f; ap->z_factor = 0.002f;                                      // :1115,1121
}

static int check_align_params(vis_ctx* ctx, const vis_align_params* ap, int w, int h) {
    if (!ap || ap->first_level < ap->last_level || ap->first_level > 4 || ap->last_level < 0 || ap->max_iterations < 1) {
        ctx->err = "alignment: 0 <= last_level <= first_level <= 4, max_iterations >= 1"; return VIS_E_INVALID;
    }
    if (w < 16 || h < 16 || w > VIS_MAX_SIDE || h > VIS_MAX_SIDE || !(ap->fx > 0) || !(ap->fy > 0)) {
        ctx->err = "alignment: 16 <= w, h <= 4095, fx, fy > 0"; return VIS_E_INVALID;
    }
    if (!std::isfinite(ap->fx) || !std::isfinite(ap->fy) || !std::isfinite(ap->cx) || !std::isfinite(ap->cy) || !std::isfinite(ap->epsilon) ||
        !std::isfinite(ap->z_factor)) {
        ctx->err = "alignment: fx, fy, cx, cy, epsilon and z_factor must be finite"; return VIS_E_INVALID;
    }
    return VIS_OK;
}

// VISystem::InitializePyramid, src/VISystem.cpp:1451-1493 (same IEEE operations as the oracle)
static void fill_level_intrinsics(const vis_align_params& ap, AlignArgs& G) {
    float fx[5], fy[5], cx[5], cy[5];
    fx[0] = ap.fx; fy[0] = ap.fy; cx[0] = ap.cx; cy[0] = ap.cy;
    for (int l = 1; l < 5; l++) {
        fx[l] = (float)((double)fx[l - 1] * 0.5);
        fy[l] = (float)((double)fy[l - 1] * 0.5);
        cx[l] = (float)(((double)cx[0] + 0.5) / (double)(1 << l) - 0.5);
        cy[l] = (float)(((double)cy[0] + 0.5) / (double)(1 << l) - 0.5);
    }
    for (int l = 0; l < 5; l++) {
        G.lv[l].fx = fx[l]; G.lv[l].fy = fy[l]; G.lv[l].cx = cx[l]; G.lv[l].cy = cy[l];
        G.lv[l].invfx = 1.f / fx[l]; G.lv[l].invfy = 1.f / fy[l];
    }
    G.first = ap.first_level; G.last = ap.last_level; G.max_it = ap.max_iterations; G.eps = ap.epsilon; G.zf = ap.z_factor;
}

// ---- vis_align_weights: context state, read where an alignment is enqueued and passed to the kernel by value
extern "C" void vis_default_align_weights(vis_align_weights* aw) {
    if (!aw) return;
    aw->mode = VIS_W_IDENTITY; aw->tukey_b = 4.6851f; aw->mad_scale = 1.4826f; aw->reserved_ = 0;   // src/VISystem.cpp:1343,1800,1831
}
extern "C" int vis_set_align_weights(vis_ctx* ctx, const vis_align_weights* aw) {
    if (!ctx) return VIS_E_INVALID;
    vis_align_weights v;
    if (aw) v = *aw; else vis_default_align_weights(&v);
    if (v.mode < VIS_W_IDENTITY || v.mode > VIS_W_TUKEY_SIGNED) { ctx->err = "vis_set_align_weights: mode is VIS_W_IDENTITY, VIS_W_TUKEY or VIS_W_TUKEY_SIGNED"; return VIS_E_INVALID; }
    if (!std::isfinite(v.tukey_b) || !(v.tukey_b > 0) || !std::isfinite(v.mad_scale) || !(v.mad_scale > 0)) {
        ctx->err = "vis_set_align_weights: tukey_b and mad_scale must be finite and > 0"; return VIS_E_INVALID;
    }
    if (v.reserved_ != 0) { ctx->err = "vis_set_align_weights: reserved_ must be 0"; return VIS_E_INVALID; }
    ctx->aw = v;
    return VIS_OK;
}
extern "C" int vis_get_align_weights(vis_ctx* ctx, vis_align_weights* aw) {
    if (!ctx || !aw) return VIS_E_INVALID;
    *aw = ctx->aw;
    return VIS_OK;
}
static void fill_weights(const vis_ctx* ctx, AlignArgs& G) { G.wmode = ctx->aw.mode; G.tukey_b = ctx->aw.tukey_b; G.mad_scale = ctx->aw.mad_scale; }

extern "C" int vis_estimate_pose_features(vis_ctx* ctx, const vis_align_params* ap, int w, int h,
                                          const uint8_t* const gray1[5], const uint8_t* const gray2[5],
                                          const int16_t* const gx1[5], const int16_t* const gy1[5],
                                          const float* const cand1[5], const int32_t n_cand[5],
                                          const vis_se3f* init, vis_align_result* out) {
    if (!ctx || !out || !gray1 || !gray2 || !gx1 || !gy1 || !cand1 || !n_cand) return VIS_E_INVALID;
    int rc = check_align_params(ctx, ap, w, h);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    int alw[5], alh[5]; vis_half_dims(w, h, alw, alh);
    for (int l = ap->last_level; l <= ap->first_level; l++) {
        const int N = n_cand[l];
        if (N < 0 || N > (1 << 24)) return VIS_E_INVALID;
        if (N && (!gray1[l] || !gray2[l] || !gx1[l] || !gy1[l] || !cand1[l])) return VIS_E_INVALID;
    }
    AlignArgs G; std::memset(&G, 0, sizeof(G));
    fill_level_intrinsics(*ap, G);
    vis_se3f* d_init = nullptr; vis_align_result* d_out;
    rc = vis_carve(ctx, [&](Carver& cv) {                          // (the caller's arrays are pageable: through the pinned block, one wait per call)
        for (int l = ap->last_level; l <= ap->first_level; l++) {
            const size_t px = (size_t)alw[l] * alh[l];
            AlignLevel& V = G.lv[l];
            V.cols = w >> l; V.rows = h >> l; V.acols = alw[l]; V.arows = alh[l]; V.rowstride = alw[l]; V.ncand = n_cand[l]; V.img_fstride = 0; V.grad_fstride = 0;
            if (!V.ncand) continue;
            V.i1 = cv.take<uint8_t>(px); V.i2 = cv.take<uint8_t>(px);
            V.gx = cv.take<int16_t>(px); V.gy = cv.take<int16_t>(px);
            V.cand = cv.take<float>((size_t)V.ncand * 4);
        }
        if (init) d_init = cv.take<vis_se3f>(1);
        d_out = cv.take<vis_align_result>(1);
    });
    if (rc) return rc;
    HostStage hs(ctx);
    hipStream_t st = ctx->stream;
    for (int l = ap->last_level; l <= ap->first_level; l++) {
        const AlignLevel& V = G.lv[l];
        const size_t px = (size_t)alw[l] * alh[l];
        if (!V.ncand) continue;
        hs.up((void*)V.i1, gray1[l], px); hs.up((void*)V.i2, gray2[l], px);
        hs.up((void*)V.gx, gx1[l], px * 2); hs.up((void*)V.gy, gy1[l], px * 2);
        hs.up((void*)V.cand, cand1[l], (size_t)V.ncand * 16);
    }
    if (init) hs.up(d_init, init, sizeof(vis_se3f));
    hs.flush_ups();
    G.init = d_init; G.out = d_out; G.f1_off = 0; G.f2_off = 0; G.out_off = 0;
    fill_weights(ctx, G);
    if (G.wmode == VIS_W_IDENTITY) hipLaunchKernelGGL((k_align<false, false>), dim3(1), dim3(AL_THREADS), 0, st, G);
    else hipLaunchKernelGGL((k_align<false, true>), dim3(1), dim3(AL_THREADS), 0, st, G);
    if (const hipError_t e = hipGetLastError()) { ctx->err = std::string("k_align launch: ") + hipGetErrorString(e); return vis_drain(ctx, VIS_E_HIP); }
    const void* h_out = hs.down(d_out, sizeof(vis_align_result));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, sizeof(vis_align_result));
    return VIS_OK;
}

extern "C" int vis_align_batch(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int w, int h, int stride, int n,
                               const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                               const float* d_pts, const int32_t* d_npts, int max_pts,
                               const vis_se3f* d_init, vis_align_result* d_out) {
    return align_batch_links(ctx, ap, d_frames, w, h, stride, n, d_gray, d_gx, d_gy, d_pts, d_npts, max_pts, nullptr, nullptr, d_init, d_out);
}

// d_prev (n entries, device): pair i aligns frame d_prev[i] -> frame i, d_prev[i] < 0 = no pair (a zeroed record); every record is
// cleared first.  The frames d_prev names are frames of the same batch (d_prev[i] < i: the keyframe links of vis_batch_run).
// snap (vis_batch_track): the snapshot of the keyframe carried from an earlier launch; pair 0 (gate off) and every pair linked to
// VIS_KF_CARRIED are aligned against it (one workgroup per frame instead of per pair 1..n-1).  nullptr: those pairs are skipped.
int align_batch_links(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int w, int h, int stride, int n,
                      const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy, const float* d_pts, const int32_t* d_npts,
                      int max_pts, const int32_t* d_prev, const TrackSnapshot* snap, const vis_se3f* d_init, vis_align_result* d_out) {
    if (!ctx || !d_frames || !d_gray || !d_gx || !d_gy || !d_pts || !d_npts || !d_out) return VIS_E_INVALID;
    int rc = check_align_params(ctx, ap, w, h);
    if (rc) return rc;
    if (stride < w || n < 1 || max_pts < 1) { ctx->err = "vis_align_batch: stride >= w, n >= 1, max_pts >= 1"; return VIS_E_INVALID; }
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    {   // frame 0 has no predecessor in this batch: its record is cleared (by a kernel of the library, not by the runtime's fill);
        // with a link table every record is, and the pairs without a link leave theirs so
        static_assert(sizeof(vis_align_result) % 4 == 0, "cleared in dwords");
        void* dsts[1] = {d_out}; const void* srcs[1] = {nullptr}; const size_t bytes[1] = {(d_prev ? (size_t)n : 1) * sizeof(vis_align_result)};
        const int rc0 = launch_copy_jobs(ctx, st, 1, dsts, srcs, bytes);
        if (rc0) return rc0;
    }
    const int pairs = snap ? n : n - 1;
    if (pairs < 1) return VIS_OK;
    AlignArgs G; std::memset(&G, 0, sizeof(G));
    fill_level_intrinsics(*ap, G);
    const size_t fe = vis_grad_frame_elems(w, h);
    int alw[5], alh[5]; vis_half_dims(w, h, alw, alh);
    size_t off = 0;
    for (int l = 0; l < 5; l++) {
        AlignLevel& V = G.lv[l];
        V.cols = w >> l; V.rows = h >> l; V.acols = alw[l]; V.arows = alh[l]; V.ncand = 0; V.cand = nullptr;
        if (l == 0) { V.i1 = d_frames; V.i2 = d_frames; V.rowstride = stride; V.img_fstride = (size_t)stride * h; }
        else { V.i1 = d_gray + off; V.i2 = d_gray + off; V.rowstride = V.acols; V.img_fstride = fe; }
        V.gx = d_gx + off; V.gy = d_gy + off; V.grad_fstride = fe;
        off += (size_t)V.acols * V.arows;
    }
    G.pts = d_pts; G.npts = d_npts; G.max_pts = max_pts; G.init = d_init; G.out = d_out;
    G.f1_off = 0; G.f2_off = 1; G.out_off = 1;                                       // workgroup q = pair (frame q -> frame q+1), result slot q+1
    G.prev = d_prev;                                                                 // (or frame d_prev[q+1] -> frame q+1)
    if (snap) {                                                                      // workgroup q = frame q: (frame q-1, or d_prev[q]) -> frame q
        G.f1_off = -1; G.f2_off = 0; G.out_off = 0;                                  // (frame -1 = VIS_KF_CARRIED: the snapshot, when there is one)
        if (snap->valid) { G.c_gray = snap->gray; G.c_gx = snap->gx; G.c_gy = snap->gy; }
    }
    const int used = std::min(max_pts, AL_MAXKP);
    const size_t lds = (size_t)used * 121 * 4;                                       // largest patch: (2*5+1)^2 pixels per keypoint
    fill_weights(ctx, G);
    if (G.wmode == VIS_W_IDENTITY) {
        if (lds > 65536 - 4096) HIPCHK(ctx, hipFuncSetAttribute((const void*)k_align<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_align<true, false>), dim3(pairs), dim3(AL_THREADS), lds, st, G);
    } else {                                                                          // (+ 12.3 KB of histograms and tables beside the list: 109 KB of 160)
        if (lds > 65536 - 16384) HIPCHK(ctx, hipFuncSetAttribute((const void*)k_align<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_align<true, true>), dim3(pairs), dim3(AL_THREADS), lds, st, G);
    }
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

// vis_batch_align and vis_batch_track: the alignment of the last vis_batch_run's pairs on the pose stream, with its ordering and
// reader events; d_track != nullptr = vis_batch_track (every frame's pair, then the keyframe snapshot and the trajectory chain)
static int batch_align_stream(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int n,
                              const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                              const vis_se3f* d_init, vis_align_result* d_out, vis_track_result* d_track) {
    if (!ctx) return d_track ? VIS_E_STATE : VIS_E_INVALID;
    Plan* pl = ctx->batch;
    if (!pl || pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (ctx->p.pose_input != VIS_POSE_GOOD) return VIS_E_STATE;                       // needs the grid-filtered matches in d_p1
    if (!d_gray && !d_gx && !d_gy) {                                                   // the plan's own gradients (VIS_STAGE_GRADIENT of the last vis_batch_run)
        if (!pl->grad_valid) { ctx->err = d_track ? "vis_batch_track: the last vis_batch_run had no VIS_STAGE_GRADIENT"
                                                  : "vis_batch_align: no gradient buffers given and the last vis_batch_run had no VIS_STAGE_GRADIENT"; return VIS_E_STATE; }
        const Plan::GradSet& G = pl->grad[pl->grad_set];
        d_gray = G.half; d_gx = G.gx; d_gy = G.gy;
    }
    if (d_track) {
        if (!d_frames || !d_out) return VIS_E_INVALID;
        if (!(pl->last_stages & VIS_STAGE_MATCH)) { ctx->err = "vis_batch_track: the last vis_batch_run had no VIS_STAGE_MATCH"; return VIS_E_STATE; }
        // the pair to the carried keyframe reads the snapshot the call for the launch before wrote: every launch since
        // vis_batch_plan / vis_batch_reset must have been tracked, once
        if (pl->run_seq != pl->track_seq + 1) {
            ctx->err = pl->run_seq == pl->track_seq ? "vis_batch_track: this launch has been tracked already"
                                                    : "vis_batch_track: a vis_batch_run since vis_batch_plan / vis_batch_reset was not tracked (its keyframe is gone)";
            return VIS_E_STATE;
        }
        const int rc = ensure_track_buffers(ctx, pl);
        if (rc) return rc;
    }
    // One persistent workgroup per pair, a chain of dependent iterations: latency-bound work that fits beside the next batch's
    // detect chain.  It runs on the pose stream, behind (a) everything queued on the context's stream so far -- the gradients of
    // these frames -- and (b) the matcher of the last batch; what may not overtake it (the next filter rewriting the matched
    // points, the next vis_gradient_batch, the feeder's next copy into these frames) waits for the reader events noted below.
    Plan::RecordSet& rs = pl->last_set();
    // d_p1 = the matched keypoints of the query frame of every pair (getGoodMatches, src/Matcher.cpp:295-303): pair i = (frame i-1, frame i),
    // or with the keyframe gate (frame link[i], frame i); links to the carried record (VIS_KF_CARRIED < 0) are skipped like pair 0 --
    // except by vis_batch_track, which aligns them against the snapshot of that keyframe (its matched points are in d_p1 like any other)
    const int32_t* links = pl->kf_min ? rs.kf_link : nullptr;
    // the side stream refills a gradient set two steps on: it waits for the last alignment that read THAT set.  Decided by pointer
    // identity, not by how the caller got the pointers: the ones vis_batch_gradients() / vis_batch_half_pyramid() hand out are the
    // plan's sets too (valid until the next vis_batch_run), and a caller passing them explicitly needs the same ordering.  Noted too: the
    // matcher-output set of the last step (the matched points) and the links, which the next gate kernel of that record set rewrites
    auto read = [&](Plan::GradSet& G) { return (G.half && d_gray == G.half) || (G.gx && d_gx == G.gx) || (G.gy && d_gy == G.gy) ? &G.readers : nullptr; };
    return on_pose_stream(ctx, {FU_FORK | FU_MATCHER, nullptr, d_frames, d_frames + (size_t)pl->stride * pl->h * n}, [&] {
        TrackSnapshot snap{};
        if (d_track) { snap = pl->snap; snap.valid = pl->kf_min ? pl->track_seq > 0 : pl->pair0_valid; }   // (gate on: only a link says whether it is used)
        int rc = align_batch_links(ctx, ap, d_frames, pl->w, pl->h, pl->stride, n, d_gray, d_gx, d_gy, pl->out().p1, pl->out().ngood, pl->root * pl->root,
                                   links, d_track ? &snap : nullptr, d_init, d_out);
        if (!rc && d_track) rc = launch_track_snapshot(ctx, pl, d_frames, d_gray, d_gx, d_gy, links, n);
        if (!rc && d_track) rc = launch_track_chain(ctx, pl, links, n, d_out, d_track);
        if (!rc && d_track) pl->track_seq = pl->run_seq;
        return rc;
    }, {read(pl->grad[0]), read(pl->grad[1]), &pl->out().readers, links ? &rs.links : nullptr});
}

extern "C" int vis_batch_align(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int n,
                               const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                               const vis_se3f* d_init, vis_align_result* d_out) {
    return batch_align_stream(ctx, ap, d_frames, n, d_gray, d_gx, d_gy, d_init, d_out, nullptr);
}

extern "C" int vis_batch_track(vis_ctx* ctx, const vis_align_params* ap, const uint8_t* d_frames, int n,
                               const vis_se3f* d_init, vis_align_result* d_align, vis_track_result* d_track) {
    if (!d_track) return ctx && ctx->batch ? VIS_E_INVALID : VIS_E_STATE;
    return batch_align_stream(ctx, ap, d_frames, n, nullptr, nullptr, nullptr, d_init, d_align, d_track);
}
