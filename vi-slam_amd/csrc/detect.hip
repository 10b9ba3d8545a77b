// detect.hip -- ORB detect + describe on gfx950 (MI355X), batched over frames.
//
// Replaces the OpenCV-CUDA call site  cuda::ORB::create(1000)->detectAndCompute(frameGPU, ...)
// (/root/reference/src/CameraGPU.cpp:99-103) and its CPU twin cv::ORB::detectAndCompute
// (/root/reference/src/Camera.cpp:87); results are bit-identical to the CPU path restated in
// oracle/orb.cpp (tests/test_detect_gpu.py).
//
// Kernel chain per batch of B frames (all on one stream, no host sync):
//   k_resize   (per level l>=1)  cv::resize INTER_LINEAR 8-bit fixed point, level l-1 -> l (k_resize_tab: its tables, once per plan)
//   k_fast     (1 launch)        all levels, all frames: 128x32 tile of the emit region + halo -> LDS, byte-SWAR
//                                pretest on every position, dense FAST-9/16 cornerScore on the survivors, 3x3 NMS +
//                                border cull; candidates into the tile's own slot (no global atomics)
//   k_select   (1 launch)        block per (frame,level): 256-bin score histogram = retainBest(2*quota) cut,
//                                Harris on survivors, LDS bitonic sort by (response desc, y, x) = canonical order,
//                                retainBest(quota)
//   k_describe (1 launch)        a wave walks over keypoints (software pipeline: the next keypoint's record and patch are in flight):
//                                43x43 raw patch -> LDS, IC angle, 7-tap blur rows on the matrix pipe (v_mfma_i32_16x16x64_i8, exact),
//                                blur columns only where rBRIEF samples, 256 tests packed with wave ballots
// HBM traffic model: every pyramid pixel is read once by k_fast and once as the
// next level's resize source; candidates/keypoints are O(N) and tiny.  k_resize streams at 84 % of the copy ceiling; k_fast is a chain of
// latency-bound phases with vector + scalar issue saturated; k_describe is bound by the LDS array with vector issue right behind it.
#include "vis_internal.h"
#include "resize_index.h"
#include <cfloat>
#include <cmath>
#include <vector>

// ------------------------------------------------------------------------------------------------
// k_resize: one thread = 4 horizontally adjacent destination pixels (one 32-bit store) x RS_ROWS rows.  Narrow variant (every
// ORB pyramid step): source rows as the three aligned dwords around the 8-byte window the four outputs touch, coefficient
// records from the per-level table of k_resize_tab.  Wide variant (scale up to 3, or levels narrower than 48 px): 12-byte
// windows as unaligned dwords, coefficients in registers, bytes picked with v_alignbyte.
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

// XCD-aware work mapping.  Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8), each
// with a private 4 MiB L2.  All work of one frame is given to ONE XCD so that halo rows, overlapping
// keypoint patches and resize source rows that neighbouring workgroups share are L2 hits instead of 8
// separate fabric fetches (rocprofv3 FETCH_SIZE was 4.1x the algorithmic bytes for k_fast before this).
// Speed only: results do not depend on the placement.  Grid = 8 * ceil(n/8) * per_frame blocks.
__device__ __forceinline__ bool xcd_frame_map(int b, int per_frame, int n, int& frame, int& inner) {
    const int xcd = b & 7, j = b >> 3;
    frame = (j / per_frame) * 8 + xcd;
    inner = j - (j / per_frame) * per_frame;
    return frame < n;
}
static inline int xcd_grid(int n, int per_frame) { return 8 * ((n + 7) / 8) * per_frame; }

__device__ __forceinline__ uint32_t pick_byte(uint32_t w0, uint32_t w1, uint32_t w2, int off) {
    // byte `off` (0..11) of the 12-byte little-endian string w0|w1|w2
    const uint32_t lo = off < 4 ? w0 : (off < 8 ? w1 : w2);
    return (lo >> ((off & 3) * 8)) & 0xFFu;
}

// cv::resize's per-column / per-row tables are recomputed in registers (same IEEE operations as the host
// builds them with: double for the source coordinate, float for the fraction, round-half-even for the
// Q11 coefficient), so the only memory dependency of a thread is its 2 x 12 source bytes -- the
// table-driven version chained three dependent loads (yofs -> xofs -> pixels) and was latency bound.
__device__ __forceinline__ void resize_coef(int d, double scale, int slen, int& s0, int& c0, int& c1) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= slen - 1) { fx = 0.f; sx = slen - 1; }
    s0 = sx;
    c0 = __float2int_rn((1.f - fx) * 2048.f);
    c1 = __float2int_rn(fx * 2048.f);
}

#define RS_ROWS 5            // destination rows per thread (10: 110 VGPRs = 4 waves per SIMD and 0.49 ms for the pyramid of 1024 frames; 5: 63 VGPRs = 8 waves, 0.455 ms)
typedef uint32_t u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned short us2_t __attribute__((ext_vector_type(2)));

// Loads + arithmetic of the RS_ROWS destination rows of a thread for a COMPILE-TIME row-sharing pattern SHARE (bit r: destination
// row r's first source row is the second source row of row r - 1).  Consecutive destination rows share a source row whenever the
// source index advances by one -- four times out of five at the pyramid's scale 1.2 -- and with the pattern known to the compiler
// the shared row is neither loaded nor horizontally interpolated twice (6 instead of 10 loads for five rows).  A run-time pattern
// does not pay: predicated or scalar-branched loads measured 0.66 ms for the pyramid of 1024 frames against 0.62 without any sharing
// and 0.51 with a compile-time pattern -- so k_resize tests the wave's pattern against the ones that occur at scale 1.2 and falls
// back to SHARE = 0 (everything loaded) for any other wave.  Same values in every case.
// FULL: every lane of the wave has all RS_ROWS rows inside the level (decided once per wave by k_resize), the stores carry no predicate;
// FULL = false keeps it (rows_left = the lane's rows inside the level).  A store goes to the frame base (SGPRs) + one 32-bit lane
// offset that advances by the stride, like the loads.
template <uint32_t SHARE, bool FULL>
__device__ __forceinline__ void resize_rows(const uint8_t* __restrict__ fbase, uint32_t wb, uint32_t asel, const uint32_t (&YX)[RS_ROWS], const uint32_t (&YY)[RS_ROWS],
                                            const uint4* __restrict__ yrow, const uint32_t (&sel)[4],
                                            const uint32_t (&coef)[4], uint8_t* __restrict__ dfbase, uint32_t doff, uint32_t dstride, int rows_left, uint32_t keep) {
    uint64_t W0[RS_ROWS], W1[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        // (frame base in SGPRs + one 32-bit lane offset: no 64-bit address pairs)
        // Byte-unaligned 8-byte loads run at about half the rate of dword-aligned ones in the texture addresser (measured: 0.57 ms
        // against 0.47 for the whole pyramid), so a row is fetched as the THREE aligned dwords that contain its 8-byte window and the
        // window is cut out with two v_perm_b32 (asel = bytes s .. s + 3, s = 0 .. 4: k_resize_tab keeps the 12 bytes inside the row).
        const u32x3_a4 d1 = *reinterpret_cast<const u32x3_a4*>(fbase + (wb + YY[r]));
        W1[r] = (uint64_t)__builtin_amdgcn_perm(d1.y, d1.x, asel) | ((uint64_t)__builtin_amdgcn_perm(d1.z, d1.y, asel) << 32);
        if (!((SHARE >> r) & 1u)) {
            const u32x3_a4 d0 = *reinterpret_cast<const u32x3_a4*>(fbase + (wb + YX[r]));
            W0[r] = (uint64_t)__builtin_amdgcn_perm(d0.y, d0.x, asel) | ((uint64_t)__builtin_amdgcn_perm(d0.z, d0.y, asel) << 32);
        }
    }
#pragma unroll
    for (int r = 1; r < RS_ROWS; r++) if ((SHARE >> r) & 1u) W0[r] = W1[r - 1];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        uint32_t v[4];                                      // the pixels x 4, + 2 for the rounding shift (<= 1022)
        const uint32_t B0 = yrow[r].z, B1 = yrow[r].w;      // the Q11 row weights (<< 16) stay in LDS until their row is due
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t p0 = __builtin_amdgcn_perm((uint32_t)(W0[r] >> 32), (uint32_t)W0[r], sel[k]);
            const uint32_t p1 = __builtin_amdgcn_perm((uint32_t)(W1[r] >> 32), (uint32_t)W1[r], sel[k]);
            const uint32_t r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, p0), __builtin_bit_cast(us2_t, coef[k]), 0u, false);
            const uint32_t r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, p1), __builtin_bit_cast(us2_t, coef[k]), 0u, false);
            // (B * (r >> 4)) >> 16 as ONE v_mul_hi_u32 with the weight pre-shifted by 16 (B <= 2048, r >> 4 <= 32640)
            v[k] = __umulhi(B0, r0 >> 4) + __umulhi(B1, r1 >> 4) + 2u;
        }
        // >> 2 on pixels 0 | 2 and 1 | 3 as halves of one register each (v_pk_lshrrev_b16: no carry between the halves, no rounding or
        // mask constants in registers), then the odd pair moves into the byte gaps of the even one
        const us2_t e02 = __builtin_bit_cast(us2_t, (v[2] << 16) + v[0]) >> (unsigned short)2;
        const us2_t e13 = __builtin_bit_cast(us2_t, (v[3] << 16) + v[1]) >> (unsigned short)2;
        const uint32_t out = (__builtin_bit_cast(uint32_t, e13) << 8) | __builtin_bit_cast(uint32_t, e02);
        if (FULL || r < rows_left) *reinterpret_cast<uint32_t*>(dfbase + doff) = out & keep;
        doff += dstride;
    }
}

// The coefficient tables of one pyramid step, built once per plan by the same IEEE operations cv::resize builds its own with:
// 12 words per 4-pixel column group (4 byte selectors, 4 packed Q11 pairs, window start, store mask, 2 unused) followed by 4 words
// per destination row (two source row offsets, two Q11 weights << 16).
__global__ void k_resize_tab(uint32_t* __restrict__ tab, int bx_count, int dw, int dh, int sw, int sh, int sstride, double scale_x, double scale_y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < bx_count) {
        const int dx4 = i * 4;
        int sxs[4], a0s[4], a1s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) resize_coef(min(dx4 + k, dw - 1), scale_x, sw, sxs[k], a0s[k], a1s[k]);
        // window start clamped so that the 8-byte fetch stays inside the row; at the right edge the second
        // byte of a pair may fall outside the window: its coefficient is 0 there, so any byte will do
        const int wb = min(sxs[0], sstride - 8);
        const int wa = min(wb & ~3, sstride - 12);           // the aligned 12 bytes fetched around the window (rows are >= 12 bytes, stride % 4 == 0)
        uint32_t* e = tab + 12 * i;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int o = sxs[k] - wb;
            e[k] = 0x0c000c00u | (uint32_t)o | ((uint32_t)min(o + 1, 7) << 16);
            e[4 + k] = (uint32_t)a0s[k] | ((uint32_t)a1s[k] << 16);
        }
        e[8] = (uint32_t)wa;
        // bytes of the 4-pixel store that lie inside the row (the rest is written as 0, as it always was)
        e[9] = dx4 + 3 < dw ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (8 * (dx4 + 4 - dw)));
        e[10] = 0x03020100u + 0x01010101u * (uint32_t)(wb - wa);      // v_perm selector of window byte 0 .. 3 within a dword pair
        e[11] = 0u;
    }
    if (i < dh) {
        // vertical: row indices are clamped, the coefficients are not (resizeGeneric_Invoker)
        float fy = (float)((i + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int sy0 = min(max(sy, 0), sh - 1), sy1 = min(max(sy + 1, 0), sh - 1);
        uint32_t* e = tab + 12 * bx_count + 4 * i;
        e[0] = (uint32_t)__umul24(sy0, sstride); e[1] = (uint32_t)__umul24(sy1, sstride);
        e[2] = (uint32_t)__float2int_rn((1.f - fy) * 2048.f) << 16; e[3] = (uint32_t)__float2int_rn(fy * 2048.f) << 16;
    }
}

// NARROW (scale <= 2, every ORB pyramid step): the 4 outputs of a thread touch <= 8 consecutive source bytes, so
// one 8-byte load per source row, one v_perm_b32 per output to pull (p[sx], p[sx+1]) out as a u16 pair and one
// v_dot2_u32_u16 against the packed (c0, c1) coefficients: ~13 VALU instructions per output pixel instead of ~35.
// The wide variant (scale <= 3) keeps the 12-byte window and picks bytes with v_alignbyte.
template <bool NARROW>
__global__ __launch_bounds__(256) void k_resize(const uint8_t* __restrict__ src, int sw, int sh, int sstride, size_t sframe,
                                                uint8_t* __restrict__ dst, int dw, int dh, int dstride, size_t dframe,
                                                double scale_x, double scale_y,
                                                int bx_count, int per_frame, int nframes, const uint32_t* __restrict__ tab, uint32_t magic) {
    int f, inner;
    if (!xcd_frame_map(blockIdx.x, per_frame, nframes, f, inner)) return;
    if (NARROW) {
        // Neither the row coefficients (two source row offsets, two Q11 weights: the same for every thread of a row) nor the column
        // coefficients (the same for every thread of a column group) are computed here: k_resize_tab tabulated them once per plan
        // (the kernel is VALU-issue bound and the double-precision coordinate arithmetic was a quarter of its instructions).  A
        // thread's dependency chain is table entry -> source bytes; the rows of the workgroup go through LDS.
        __shared__ uint4 yc[256];
        // flat (row group, 4-pixel column group) index (resize_index.h), decoded by one multiply-high with the level's magic number.
        // What depends on the workgroup or the wave alone is computed from uniform integers, i.e. on the scalar unit.
        const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
        const uint32_t idx_wg = (uint32_t)inner * 256u, idx_wave = idx_wg + wave * 64u;
        const uint32_t tid = wave * 64u + threadIdx.x;
        uint32_t rg, cg;
        resize_index_decode(idx_wave + threadIdx.x, magic, (uint32_t)bx_count, rg, cg);
        const uint32_t dy0 = rg * RS_ROWS;
        const uint32_t rg_first = resize_index_row_group(idx_wg, magic), rg_last = resize_index_row_group(idx_wg + 255u, magic);
        const uint32_t row_first = rg_first * RS_ROWS, nrows = (rg_last - rg_first + 1u) * RS_ROWS;
        // the wave's last lane has its largest row group: is any of the wave's rows outside the level?
        const bool partial = (resize_index_row_group(idx_wave + 63u, magic) + 1u) * RS_ROWS > (uint32_t)dh;
        // table records at the table base (SGPRs) + a 32-bit byte offset (the table is 48 bytes per column group + 16 per row: < 2^17)
        const uint8_t* tabb = reinterpret_cast<const uint8_t*>(tab);
        // (the column records are requested first: the row record has to come back before the barrier, the others travel with it)
        uint4 s4, c4, m4;
        if (dy0 < (uint32_t)dh) {
            const uint32_t o = __umul24(cg, 48u);
            s4 = *reinterpret_cast<const uint4*>(tabb + o); c4 = *reinterpret_cast<const uint4*>(tabb + (o + 16u)); m4 = *reinterpret_cast<const uint4*>(tabb + (o + 32u));
        }
        // nrows <= 256: the host sends narrower levels (< 12 groups per row) to the wide variant
        if (tid < nrows) yc[tid] = *reinterpret_cast<const uint4*>(tabb + (48u * (uint32_t)bx_count + 16u * min(row_first + tid, (uint32_t)dh - 1u)));
        __syncthreads();
        if (dy0 >= (uint32_t)dh) return;
        const uint32_t sel[4] = {s4.x, s4.y, s4.z, s4.w}, coef[4] = {c4.x, c4.y, c4.z, c4.w};
        const uint32_t wb = m4.x, keep = m4.y, asel = m4.z;
        uint8_t* dfbase = dst + (size_t)f * dframe;
        const uint32_t doff = __umul24(dy0, (uint32_t)dstride) + cg * 4u;     // (rows and strides are far below 2^24)
        const int rows_left = dh - (int)dy0;
        const uint8_t* fbase = src + (size_t)f * sframe;
        const uint4* yrow = yc + (dy0 - row_first);
        uint32_t YX[RS_ROWS], YY[RS_ROWS];
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) { YX[r] = yrow[r].x; YY[r] = yrow[r].y; }
        // the row-sharing pattern of the WAVE (one scalar bit per row: every lane's first source row is the row above's second)
        uint32_t share = 0;
#pragma unroll
        for (int r = 1; r < RS_ROWS; r++) share |= (__builtin_amdgcn_ballot_w64(YX[r] != YY[r - 1]) == 0 ? 1u : 0u) << r;
        // At scale 1.2 the source row advances by two once every five rows (at row p of a group of five).
        // Any pattern that is a SUBSET of the wave's is exact (an unshared row is simply loaded); the second list covers waves that
        // straddle two row groups whose phase differs by one, so that only waves at a clamped border or of another scale load every row.
        // The sharing cases store without a per-row predicate.  A wave with a partial row group (the last of a level whose height is no
        // multiple of RS_ROWS) goes, like a wave of no listed pattern, to the one instance that loads every row and predicates its stores.
#define RS_CASE(M) if ((M & ~share) == 0u) { resize_rows<M, true>(fbase, wb, asel, YX, YY, yrow, sel, coef, dfbase, doff, (uint32_t)dstride, rows_left, keep); return; }
        if (!partial) { RS_CASE(0x1Eu) RS_CASE(0x1Cu) RS_CASE(0x1Au) RS_CASE(0x16u) RS_CASE(0x0Eu) RS_CASE(0x18u) RS_CASE(0x12u) RS_CASE(0x06u) }
#undef RS_CASE
        resize_rows<0u, false>(fbase, wb, asel, YX, YY, yrow, sel, coef, dfbase, doff, (uint32_t)dstride, rows_left, keep);
        return;
    }
    // flat (row group, 4-pixel column group) index: rows are narrower than 256 px on most levels, a 2-D block
    // mapping leaves a quarter of the lanes idle
    const int idx = inner * 256 + threadIdx.y * 64 + threadIdx.x;
    int rg = (int)(((float)idx + 0.5f) * (1.0f / (float)bx_count));
    int cg = idx - rg * bx_count;
    if (cg < 0) { rg--; cg += bx_count; } else if (cg >= bx_count) { rg++; cg -= bx_count; }
    const int dx4 = cg * 4, dy0 = rg * RS_ROWS;
    if (dy0 >= dh) return;
    int sxs[4], a0s[4], a1s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) resize_coef(min(dx4 + k, dw - 1), scale_x, sw, sxs[k], a0s[k], a1s[k]);
    uint8_t* dbase = dst + (size_t)f * dframe + dx4;
    const uint32_t keep = dx4 + 3 < dw ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (8 * (dx4 + 4 - dw)));
    // the 4 outputs read source bytes sxs[0] .. sxs[3]+1 (span <= 12 for any down-scale factor < 3.6);
    // clamp the window start so the 12-byte fetch stays inside the row (rows are >= 12 bytes)
    const int wb = min(sxs[0], sstride - 12);
    int offs[4]; bool s1s[4], s2s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { const int o0 = sxs[k] - wb; offs[k] = o0 & 3; s1s[k] = o0 >= 4; s2s[k] = o0 >= 8; }
    const uint8_t* sbase = src + (size_t)f * sframe + wb;
    // issue the source loads of all RS_ROWS rows first (24 dwords in flight per thread), then compute
    uint32_t W[RS_ROWS][6]; int B0[RS_ROWS], B1[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        const int dy = min(dy0 + r, dh - 1);
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int sy0 = min(max(sy, 0), sh - 1), sy1 = min(max(sy + 1, 0), sh - 1);
        B0[r] = __float2int_rn((1.f - fy) * 2048.f); B1[r] = __float2int_rn(fy * 2048.f);
        const uint8_t* S0 = sbase + (size_t)sy0 * sstride;
        const uint8_t* S1 = sbase + (size_t)sy1 * sstride;
        W[r][0] = *reinterpret_cast<const u32_unaligned*>(S0);     W[r][1] = *reinterpret_cast<const u32_unaligned*>(S0 + 4);
        W[r][2] = *reinterpret_cast<const u32_unaligned*>(S0 + 8); W[r][3] = *reinterpret_cast<const u32_unaligned*>(S1);
        W[r][4] = *reinterpret_cast<const u32_unaligned*>(S1 + 4); W[r][5] = *reinterpret_cast<const u32_unaligned*>(S1 + 8);
    }
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // the two horizontally adjacent source bytes (sx, sx+1) as the low 16 bits of one funnel shift.
            // At the right edge (sx == sw-1) the second byte is a don't-care: its coefficient is 0.
            const uint32_t lo0 = s2s[k] ? W[r][2] : (s1s[k] ? W[r][1] : W[r][0]), hi0 = s2s[k] ? 0u : (s1s[k] ? W[r][2] : W[r][1]);
            const uint32_t lo1 = s2s[k] ? W[r][5] : (s1s[k] ? W[r][4] : W[r][3]), hi1 = s2s[k] ? 0u : (s1s[k] ? W[r][5] : W[r][4]);
            const uint32_t p0 = __builtin_amdgcn_alignbyte(hi0, lo0, (uint32_t)offs[k]);
            const uint32_t p1 = __builtin_amdgcn_alignbyte(hi1, lo1, (uint32_t)offs[k]);
            const int r0 = (int)(p0 & 0xFFu) * a0s[k] + (int)((p0 >> 8) & 0xFFu) * a1s[k];
            const int r1 = (int)(p1 & 0xFFu) * a0s[k] + (int)((p1 >> 8) & 0xFFu) * a1s[k];
            const int v = (((B0[r] * (r0 >> 4)) >> 16) + ((B1[r] * (r1 >> 4)) >> 16) + 2) >> 2;
            out |= (uint32_t)(v & 255) << (8 * k);
        }
        if (dy0 + r < dh) *reinterpret_cast<uint32_t*>(dbase + (uint32_t)__umul24(dy0 + r, dstride)) = out & keep;
    }
}

// ------------------------------------------------------------------------------------------------
// k_fast: streaming FAST-9/16 + 3x3 NMS, one WAVE per two strip segments ("items"), no workgroup barrier.
//
// An item is a strip of 32 lanes x 4 pixels (one dword per lane and row) that a half wave marches down, 8 score rows per chunk, at
// most VIS_FS_NCH chunks.  Everything between the image and the candidate slot is private to the wave:
//   * rows arrive as ONE coalesced dword load per lane and row, requested a whole chunk (8 rows) ahead; the raw dword goes into a
//     16-row LDS ring (for the score phase), its 7-bit reduction stays in registers: a row is reduced once and serves as the lower,
//     the centre and the upper row of the axis pretest of three different score rows (the tiled kernel read five LDS dwords and
//     reduced five operands per 4-pixel unit);
//   * the east / west operands of the pretest come from the neighbour lanes (DPP wave shifts) -- no LDS access in the pretest at all;
//   * the pass bits of a chunk (8 rows x 4 pixels, dark and bright polarity apart) are two 32-bit registers per lane; the set bits are
//     compacted into an LDS queue (wave-wide prefix sum, no atomics) and scored TWO entries per lane, ONE polarity each, in gfx950's
//     three-input packed half-precision min / max (fast_score16_pair) into a 10-row score ring; entries that score move on to the 3x3 NMS
//     + border cull, which runs one row behind the scores (the scored entries of a pass's last row are carried to the next pass).
// 10 KB of LDS and 88 VGPRs per wave: 16 one-wave workgroups per CU.  Measured against the tiled kernel of rounds 1-4 (512 frames of
// S-752 at the predicted thresholds, last dispatch, tools/pmc_kernel.sh): vector instructions 213 M -> 172.5 M, scalar 107 M -> 29 M,
// 376 -> 313 us alone (330 before the pass masks were skewed across the lanes); at 13 waves per CU (12 KB) 366 us, at 9 waves 440 us -- the kernel is a chain of LDS / global round trips per wave,
// occupancy is what hides them.
// Results are the tiled kernel's: the pretest is the same necessary condition, cornerScore and the NMS are unchanged, candidate
// order inside a slot is irrelevant (k_select sorts).
#define FS_LANES 32
#define FS_ROWB 264                              // bytes per ring row: 64 lanes x 4 pixels + 8 (66 dwords: vertically adjacent positions -- corners
                                                 // cluster -- fall into different LDS banks; with 64 the byte gathers of the score phase conflicted 3x as often)
#define FS_ROWD (FS_ROWB / 4)
#define FS_RING 16                               // pixel / score ring rows (two chunks of 8)
#define FS_MIRROR 6                              // ring rows 0..5 are stored a second time behind row 15: a 7-row window never wraps
#define FS_QCAP 512                              // queue entries per pass (a chunk with more passers is worked through row by row)
#define FS_PX_BYTES ((FS_RING + FS_MIRROR) * FS_ROWB)
#define FS_SCR 10                                // score ring rows: the NMS of a chunk sees score rows 8 c - 2 .. 8 c + 7 (slot = row mod 10)
#define FS_SC_BYTES (FS_SCR * FS_ROWB)
#define FS_Q_BYTES ((FS_QCAP + 64) * 2)          // + one scratch entry per lane (branch-free append)
#define FS_CAR_BYTES (2 * 256)                   // two carry lists (ping-pong) of one byte per entry (4 lane + j): the scored passers of one score row
#define FS_WAVE_LDS (FS_PX_BYTES + FS_SC_BYTES + FS_Q_BYTES + FS_CAR_BYTES)
#define TILE_CAND_CAP VIS_TILE_CAND_CAP
static_assert(FS_LANES * 4 - 8 == VIS_FS_EMIT_W, "strip geometry (geometry.cpp)");
static_assert(2 * 2 * 4 * FS_LANES <= FS_QCAP, "the passers of one row (both polarities) fit the queue");

// cornerScore<16> without the early exit (callers have already thinned the candidates): with X[k] = v - p_k the minimum over 9
// consecutive X is the dark-arc margin of the arc starting at k, the maximum over the 16 arcs is cv::cornerScore's a0; with
// X[k] = p_k - v the same chain gives -b0; score = max(a0, -b0) - 1.
typedef short pk16 __attribute__((ext_vector_type(2)));
// TWO queue entries per lane, ONE polarity each (the halves of a packed register hold entry A and entry B): the
// pretest knows which polarity passed, and a position cannot have a dark AND a bright 9-arc (18 > 16 ring pixels), so the other
// polarity's chain is wasted work -- 112 packed instructions per two entries instead of 96 per entry.  sg = (+1 | -1) per half
// (dark: v - p_k, bright: p_k - v); a position whose pretest passed both polarities is in the queue twice, at most one entry scores.
template <int S>
__device__ __forceinline__ pk16 fast_score16_pair(const uint8_t* a0, const uint8_t* b0, uint32_t nsg, int t) {
    const uint32_t va = a0[3 * S + 3], vb = b0[3 * S + 3];
#define RO(dy, dx) ((3 + (dy)) * S + 3 + (dx))
    const int off[16] = {RO(3, 0), RO(3, 1), RO(2, 2), RO(1, 3), RO(0, 3), RO(-1, 3), RO(-2, 2), RO(-3, 1),
                         RO(-3, 0), RO(-3, -1), RO(-2, -2), RO(-1, -3), RO(0, -3), RO(1, -3), RO(2, -2), RO(3, -1)};
#undef RO
    // X[k] = sg (v - p_k) = p_k * (-sg) + sg v per half: one pack (the two ring bytes into the halves of a register) and one
    // v_pk_mad_i16.  The addend also carries 0x6500 per half: the 16-bit pattern 0x6500 + X (|X| <= 255) IS the half-precision number
    // 1280 + X, so the integer result can go straight into gfx950's three-input packed half-precision minimum / maximum -- min over 9
    // consecutive X as min3 of min3 (32 instructions), max over the 16 arcs as a chain of max3 (8): 40 instead of 80 two-input ones.
    // Every value is a small integer, exact in half precision; min / max commute with the bias.
    const pk16 V2 = {(short)va, (short)vb};
    const pk16 SV = -(V2 * __builtin_bit_cast(pk16, nsg)) + pk16{(short)0x6500, (short)0x6500};     // sg v = -(nsg v); nsg = -sg = (-1 | +1) per half
    uint32_t X[16], m3[16], m9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t pk = (uint32_t)a0[off[k]] | ((uint32_t)b0[off[k]] << 16);     // (no ds_read_u8_d16_hi: with SRAM ECC on, gfx950's d16 loads do not preserve the other half)
        asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(X[k]) : "v"(pk), "v"(nsg), "v"(__builtin_bit_cast(uint32_t, SV)));
    }
#pragma unroll
    for (int k = 0; k < 16; k++) asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(m3[k]) : "v"(X[k]), "v"(X[(k + 1) & 15]), "v"(X[(k + 2) & 15]));
#pragma unroll
    for (int k = 0; k < 16; k++) asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(m9[k]) : "v"(m3[k]), "v"(m3[(k + 3) & 15]), "v"(m3[(k + 6) & 15]));
    uint32_t acc;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(acc) : "v"(m9[0]), "v"(m9[1]), "v"(m9[2]));
#pragma unroll
    for (int k = 3; k < 15; k += 2) asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(acc) : "v"(acc), "v"(m9[k]), "v"(m9[k + 1]));
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(acc) : "v"(acc), "v"(m9[15]), "v"(m9[15]));
    const int sa = (int)(acc & 0xFFFFu) - 0x6500 - 1, sb = (int)(acc >> 16) - 0x6500 - 1;
    return pk16{(short)(sa >= t ? sa : 0), (short)(sb >= t ? sb : 0)};
}

// LDS traffic inside ONE wave is processed in issue order; only the compiler must be kept from
// reordering the accesses (waves of a block use disjoint LDS regions).
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
                         __builtin_amdgcn_wave_barrier();                        \
                         __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// one record per k_fast wave (two items of one level; an odd item count leaves the last wave's second half idle: nch = 0), built
// once per plan: everything a wave needs arrives with one 64-byte scalar load
struct FastWave {
    const uint8_t* img;          // level image (nullptr: level 0 = the batch of the call)
    uint32_t* cand;              // level candidate slots
    uint32_t frame_bytes;        // bytes per frame of the level image
    int32_t stride;
    uint32_t wh;                 // w | h << 16
    int32_t x0[2];               // pixel column of lane 0 of the half (dword aligned; its first emitting column is x0 + 4)
    int32_t y0[2];               // first score row of the half (its first emitting row is y0 + 1)
    uint32_t nl;                 // chunks of half 0 | chunks of half 1 << 8 | level << 16
    uint32_t ntiles;             // items of the level
    uint32_t tile[2];            // item index inside the level
    uint32_t tile_base;          // first global item index of the level (tile_cnt)
};
static_assert(sizeof(FastWave) == 64, "FastWave is read as s_load_dwordx16");

// Speculative threshold (batched streams).  KeyPointsFilter::retainBest(2 * quota) keeps, per level, the corners whose score
// reaches a cut that is far above the FAST threshold t (S-752: 61..82 against t = 20) and moves little from frame to frame.  A
// corner below the cut is neither kept nor able to suppress a kept one in the 3x3 NMS (strict >), so FAST may run with ANY
// threshold tau <= cut and give the identical keypoints -- while scoring a quarter of the candidates.  tau[level] is predicted from
// the previous batch's cuts (k_tau_update: min over the frames - margin); k_select VERIFIES it per (frame, level): fewer than
// 2 * quota candidates at tau > t means the prediction was too high there -> that (frame, level) goes on a device work list and is
// redone at t by k_fast_fix / k_select_fix.  Exact for every input; only the speed depends on how coherent the stream is.
__device__ __forceinline__ void fast_wave(const FastWave& V, const uint8_t* __restrict__ frames0, int total_tiles, int f,
                                          int threshold, int edge, int32_t* __restrict__ tile_cnt, unsigned char* __restrict__ lds) {
    typedef __attribute__((address_space(3))) uint16_t lds_u16;
    const int lane = (int)(threadIdx.x & 63u);
    const int hh = lane >> 5, lq = lane & (FS_LANES - 1);
    const int w = (int)(V.wh & 0xFFFFu), h = (int)(V.wh >> 16), stride = V.stride;
    const int nch0 = (int)(V.nl & 0xFFu), nch1 = (int)((V.nl >> 8) & 0xFFu);
    const int nchunks = max(nch0, nch1);                                       // wave-uniform
    const int x0 = hh ? V.x0[1] : V.x0[0], y0 = hh ? V.y0[1] : V.y0[0], nch = hh ? nch1 : nch0;
    const uint8_t* base = (V.img ? V.img : frames0) + (size_t)f * V.frame_bytes;       // level 0 is the caller's batch
    const int xpix = x0 + 4 * lq;
    const uint32_t coff = (uint32_t)min(xpix, stride - 4);                     // (a lane beyond the row holds no valid position)
    // real scores are needed one pixel beyond the emit region (NMS neighbours), nowhere else
    const int lox = max(3, edge - 1), hix = min(w - 3, w - edge + 1);
    const int loy = max(3, edge - 1), hiy = min(h - 3, h - edge + 1);
    // valid positions of the lane: byte j of colbits is all ones when pixel j may be scored.  The west operand of the first lane's
    // pixels 0..2 and the east operand of the last lane's pixels 1..3 lie outside the strip.
    uint32_t colbits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool ok = xpix + j >= lox && xpix + j < hix && (lq > 0 || j == 3) && (lq < FS_LANES - 1 || j == 0);
        colbits |= ok ? (0xFFu << (8 * j)) : 0u;
    }
    const int rlo = max(0, loy - y0), rhi = min(hiy - y0, 8 * nch);            // valid score rows of the half: y0 + [rlo, rhi)
    // LDS of this wave
    uint32_t* const px32 = reinterpret_cast<uint32_t*>(lds);
    const uint8_t* const pxb = lds;
    uint8_t* const sc = lds + FS_PX_BYTES;
    uint16_t* const Q = reinterpret_cast<uint16_t*>(lds + FS_PX_BYTES + FS_SC_BYTES);
    uint8_t* const CAR = reinterpret_cast<uint8_t*>(Q + FS_QCAP + 64);
    auto sc_slot = [](int q) -> int { return q - FS_SCR * ((q * 205) >> 11); };         // q mod 10 for 0 <= q < 1024 / 15
    static_assert(8 * VIS_FS_NCH < 1000, "range of the multiply-shift quotient");
    // rows: load chunk k = rows y0 - 5 + 8 k .. + 7 of the half (ring slots 8 (k & 1) ..).  Score row q of chunk c (q = 8 c + r) has its
    // centre in ring row q + 5, i.e. it needs load chunks c (last 6 rows) and c + 1.
    // the last row this half needs: ring row 8 nchunks + 7 (the lower row of its last score row; the image's last row at most).  The two
    // load chunks requested behind it (the prefetch is unconditional) re-read THAT row instead of sixteen new ones: the first streaming
    // build fetched 88 rows per 70 it used -- FETCH_SIZE 1.26 x the algorithmic bytes
    const uint32_t voff_max = (uint32_t)(min(h - 1, y0 - 5 + 8 * nchunks + 7) * stride) + coff;
    uint32_t voff = (uint32_t)(max(y0 - 5, 0) * stride) + coff;
    auto ld = [&](uint32_t o) -> uint32_t {
        return *(const __attribute__((address_space(1))) uint32_t*)(uintptr_t)(base + (size_t)o);   // global, not flat: the level-0 select hides the address space
    };
    // (rows below the image -- the chunk requested behind a segment's last one, the shorter half of a wave -- repeat the last row:
    // one v_min per row; nothing reads them as a valid position)
    auto load8 = [&](uint32_t (&d)[8]) {
#pragma unroll
        for (int i = 0; i < 8; i++) { d[i] = ld(min(voff, voff_max)); voff += (uint32_t)stride; }
    };
    const uint32_t M7 = 0x7f7f7f7fu;
    uint32_t old[8], nw[8], nxt[8];
    load8(old);
    load8(nw);
    load8(nxt);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        px32[i * FS_ROWD + lane] = old[i];
        if (i < FS_MIRROR) px32[(FS_RING + i) * FS_ROWD + lane] = old[i];
        px32[(8 + i) * FS_ROWD + lane] = nw[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) { old[i] = (old[i] >> 1) & M7; nw[i] = (nw[i] >> 1) & M7; }
    // Byte-SWAR axis pretest on plain 32-bit integer instructions (4 pixels per instruction, the full-rate class).  Pixels are reduced
    // to 7 bits (p >> 1), so bit 7 of every byte is free to hold the sign of a per-byte difference.  With K = ceil(t / 2):
    //     ring pixel darker than c - t    =>  c7 - r7 >= K        ring pixel brighter than c + t  =>  r7 - c7 >= K
    // (necessary conditions: the test may pass more pixels than the exact one, never fewer; cornerScore decides.)
    //     cD = c7 + (128 - (K-1))   per byte, no carry        D = cD - r7:  bit 7 set <=> c7 - r7 >= K-1   ("dark")
    //     B' = ~(D + (2K-3)) = ~(2K-3) - D:  bit 7 SET <=> r7 - c7 >= K-1 + (0 or 1)                           ("bright")
    // A byte whose subtraction wraps (|difference| > 118) borrows 1 from / carries 1 into its left neighbour: the tests
    // use K-1 resp. 2K-3 instead of K and 2K-2, which absorbs exactly that unit, and the wrapped byte itself reads
    // "pass".  tests/test_independent_numpy.py replays these formulas in numpy exhaustively over (c, r, t).
    // The axis test: both opposite pairs (upper, lower) and (east, west) must show a dark pixel, or both a bright one.
    const int K = (threshold + 1) >> 1;
    const bool swar = K >= 3 && K <= 128;                                      // t < 5: every position goes to cornerScore
    const uint32_t kD = 0x80808080u - (uint32_t)(K - 1) * 0x01010101u;
    const uint32_t nkB = ~((uint32_t)(2 * K - 3) * 0x01010101u);
    const uint32_t lane5 = (uint32_t)lane << 5;
    const uint32_t q_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)Q;          // LDS byte address
    const uint32_t a_scr = q_base + 2u * (uint32_t)(FS_QCAP + lane);
    // candidate slots of the two items and their fill
    uint32_t* const candf = V.cand + (size_t)f * V.ntiles * TILE_CAND_CAP;
    int cnt0 = 0, cnt1 = 0;                                                     // wave-uniform
    int ncar = 0, qcar = 0, cur = 0;                                            // carried passers: count, their score row, list in use
    WAVE_SYNC();
    for (int c = 0; c < nchunks; c++) {
        // bit 8 j + r: pixel j of score row 8 c + r passes the dark (maskD) / the bright (maskB) axis test
        uint32_t maskD = 0xFFFFFFFFu, maskB = 0xFFFFFFFFu;
        if (swar) {
            maskD = 0; maskB = 0;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t Cc = r < 3 ? old[r + 5] : nw[r - 3];
                const uint32_t Up = r < 6 ? old[r + 2] : nw[r - 6];
                const uint32_t Lo = nw[r];
                const uint32_t cl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Cc, 0x138, 0xF, 0xF, true);    // wave_shr:1: lane i <- lane i - 1
                const uint32_t cr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Cc, 0x130, 0xF, 0xF, true);    // wave_shl:1: lane i <- lane i + 1
                const uint32_t Ee = __builtin_amdgcn_alignbyte(cr, Cc, 3);       // +3 px: bytes 3..6 of cr:Cc
                const uint32_t Ww = __builtin_amdgcn_alignbyte(Cc, cl, 1);       // -3 px: bytes 1..4 of Cc:cl
                const uint32_t cD = Cc + kD;
                const uint32_t dn = cD - Up, ds = cD - Lo, de = cD - Ee, dw = cD - Ww;
                const uint32_t bn = nkB - dn, bs = nkB - ds, be = nkB - de, bw = nkB - dw;
                const uint32_t dark = (dn | ds) & (de | dw);                      // bit 7 of byte j: pixel j passes
                const uint32_t bright = (bn | bs) & (be | bw);
                // (x & sel) | mask as ONE full-rate v_bitop3_b32 (the compiler's v_and_or_b32 issues at half rate: tools/dpp_rates.hip)
                maskD = __builtin_amdgcn_bitop3_b32(r == 7 ? dark : (dark >> (7 - r)), 0x01010101u << r, maskD, 0xEA);
                maskB = __builtin_amdgcn_bitop3_b32(r == 7 ? bright : (bright >> (7 - r)), 0x01010101u << r, maskB, 0xEA);
            }
        }
        {
            // rows of this chunk that may be scored: q = 8 c + r in [rlo, rhi)
            const int lo_ = min(max(rlo - 8 * c, 0), 8), hi_ = min(max(rhi - 8 * c, 0), 8);
            const uint32_t rb = ((1u << hi_) - 1u) & ~((1u << lo_) - 1u);
            const uint32_t valid = colbits & (rb * 0x01010101u);
            maskD &= valid; maskB &= valid;
        }
        // Skew the masks across the lanes of a 16-lane row: lane i takes the bits of score row r from lane (i - r) mod 16 (row_ror:r).
        // Passers cluster around corners -- a 4 x 8 block of one lane holds a whole cluster, and the append below runs as many rounds as the
        // fullest lane has bits (a timing build without the append: 0.574 -> 0.456 ms for the kernel, 38 % of it).  After the skew a lane
        // holds ONE row of eight different 4-pixel columns: a cluster spreads over as many lanes as it has rows.  The queue entry keeps the
        // consumer lane; the score phase undoes the rotation (src lane = (lane & 48) | ((lane - r) & 15)).
        {
            uint32_t sD = maskD & 0x01010101u, sB = maskB & 0x01010101u;
#define FS_SKEW(R) { const uint32_t sel_ = 0x01010101u << (R);                                                                                        \
                     sD = __builtin_amdgcn_bitop3_b32((uint32_t)__builtin_amdgcn_update_dpp(0, (int)maskD, 0x120 + (R), 0xF, 0xF, false), sel_, sD, 0xEA); \
                     sB = __builtin_amdgcn_bitop3_b32((uint32_t)__builtin_amdgcn_update_dpp(0, (int)maskB, 0x120 + (R), 0xF, 0xF, false), sel_, sB, 0xEA); }
            FS_SKEW(1) FS_SKEW(2) FS_SKEW(3) FS_SKEW(4) FS_SKEW(5) FS_SKEW(6) FS_SKEW(7)
#undef FS_SKEW
            maskD = sD; maskB = sB;
        }
        // the score rows of this chunk (ring slots (8 c) mod 10 .. + 7, wrapping) start at zero: positions that are not scored read 0 in the NMS
        const int sc0 = sc_slot(8 * c);                                         // wave-uniform
        {
            constexpr int RU = FS_ROWB / 8;                                     // 8-byte units per row
            unsigned long long* z = reinterpret_cast<unsigned long long*>(sc);
#pragma unroll
            for (int k = 0; k < (8 * RU + 63) / 64; k++) {
                int u = sc0 * RU + 64 * k + lane;
                u -= u >= FS_SCR * RU ? FS_SCR * RU : 0;
                if (64 * k + lane < 8 * RU) z[u] = 0ull;
            }
        }
        // passes over the rows of the chunk: all 8 at once, or row by row when the chunk has more passers than the queue holds
        uint32_t mD = maskD, mB = maskB;
        int n = __popc(mD) + __popc(mB);
        auto prefix = [&](int v) -> int {                                       // wave-wide inclusive prefix sum (DPP row shifts + row broadcasts)
            v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);      // row_shr:1
            v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);      // row_shr:2
            v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);      // row_shr:4
            v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);      // row_shr:8
            v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);      // row_bcast:15 -> rows 1, 3
            v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);      // row_bcast:31 -> rows 2, 3
            return v;
        };
        int incl = prefix(n);
        int tot = __builtin_amdgcn_readlane(incl, 63);
        const int step = tot > FS_QCAP ? 1 : 8;
        for (int a = 0; a < 8; a += step) {
            if (step != 8) {
                const uint32_t sel = 0x01010101u << a;
                mD = maskD & sel; mB = maskB & sel;
                n = __popc(mD) + __popc(mB);
                incl = prefix(n);
                tot = __builtin_amdgcn_readlane(incl, 63);
            }
            const int qlast = 8 * c + a + step - 1;                              // the row whose lower neighbours are not scored yet
            const uint8_t* const car_rd = CAR + cur * 256; uint8_t* const car_wr = CAR + (cur ^ 1) * 256;
            int nnew = 0, nR = 0;                                                // scored passers: of row qlast (carried on) / of the rows before it
            if (tot) {
                // (1) queue append without ballots or atomics: every lane writes its passers to consecutive entries behind the lanes before
                // it; entry = polarity << 11 | lane << 5 | bit = polarity << 11 | (4 lane + j) << 3 | r.  A lane that has run out of bits
                // stores into its scratch entry.
                {
                    uint32_t a_idx = q_base + 2u * (uint32_t)(incl - n);
                    uint32_t dD = mD, dB = mB;
                    // rounds = the fullest lane's larger count, known before the loop (DPP max over the rows + four v_readlane): the loop
                    // control is scalar -- a `while (ballot(bits left))` puts a vector compare -> vcc -> branch chain into every round
                    int nmax = max(__popc(mD), __popc(mB));
                    nmax = max(nmax, __builtin_amdgcn_update_dpp(0, nmax, 0xB1, 0xF, 0xF, false));     // quad_perm [1,0,3,2]
                    nmax = max(nmax, __builtin_amdgcn_update_dpp(0, nmax, 0x4E, 0xF, 0xF, false));     // quad_perm [2,3,0,1]
                    nmax = max(nmax, __builtin_amdgcn_update_dpp(0, nmax, 0x141, 0xF, 0xF, false));    // row_half_mirror
                    nmax = max(nmax, __builtin_amdgcn_update_dpp(0, nmax, 0x140, 0xF, 0xF, false));    // row_mirror
                    const int wmax = max(max(__builtin_amdgcn_readlane(nmax, 0), __builtin_amdgcn_readlane(nmax, 16)),
                                         max(__builtin_amdgcn_readlane(nmax, 32), __builtin_amdgcn_readlane(nmax, 48)));
                    for (int rnd = 0; rnd < wmax; rnd++) {
                        const bool hasD = dD != 0u, hasB = dB != 0u;
                        const uint32_t bD = (uint32_t)__builtin_ctz(dD | 0x80000000u), bB = (uint32_t)__builtin_ctz(dB | 0x80000000u);
                        dD &= dD - 1u; dB &= dB - 1u;
                        *(lds_u16*)(uintptr_t)(hasD ? a_idx : a_scr) = (uint16_t)(lane5 | bD);
                        a_idx += hasD ? 2u : 0u;
                        *(lds_u16*)(uintptr_t)(hasB ? a_idx : a_scr) = (uint16_t)(lane5 | bB | 0x800u);
                        a_idx += hasB ? 2u : 0u;
                    }
                }
                WAVE_SYNC();
                // (2) cornerScore on the queue, two entries per lane (A = entry i0 + lane, B = entry i0 + 64 + lane).  Entries that score
                // are written to the score ring and move on: row qlast to the carry list, the rows before it to the front of the queue
                // (the survivor list R of the NMS; it never overtakes the entries still to be read).
                for (int i0 = 0; i0 < tot; i0 += 128) {
                    const int iA = i0 + lane, iB = i0 + 64 + lane;
                    const bool actA = iA < tot, actB = iB < tot;
                    const uint32_t eA = Q[actA ? iA : i0], eB = Q[actB ? iB : i0];
                    // entry = polarity << 11 | consumer lane << 5 | j << 3 | r: the bits of row r came from lane (consumer - r) mod 16 of its row
                    const int rA = (int)(eA & 7u), rB = (int)(eB & 7u), lcA = (int)(eA >> 5) & 63, lcB = (int)(eB >> 5) & 63;
                    const int xlA = ((lcA & 48) | ((lcA - rA) & 15)) * 4 + ((int)(eA >> 3) & 3), qA = 8 * c + rA;
                    const int xlB = ((lcB & 48) | ((lcB - rB) & 15)) * 4 + ((int)(eB >> 3) & 3), qB = 8 * c + rB;
                    // 7 x 7 window: ring rows q + 2 .. q + 8 (the centre is ring row q + 5), columns xl - 3 .. xl + 3
                    const uint8_t* a0 = pxb + (((qA + 2) & (FS_RING - 1)) * FS_ROWB + xlA - 3);
                    const uint8_t* b0 = pxb + (((qB + 2) & (FS_RING - 1)) * FS_ROWB + xlB - 3);
                    const uint32_t nsg = ((eA & 0x800u) ? 0x0001u : 0xFFFFu) | ((eB & 0x800u) ? 0x00010000u : 0xFFFF0000u);
                    const pk16 sp = fast_score16_pair<FS_ROWB>(a0, b0, nsg, threshold);
                    const int sA = actA ? (int)sp.x : 0, sB = actB ? (int)sp.y : 0;
                    WAVE_SYNC();                                               // (every entry of this round has been read)
                    const int slA = sc0 + rA, slB = sc0 + rB;      // (8 c + r) mod 10
                    if (sA > 0) sc[(slA - (slA >= FS_SCR ? FS_SCR : 0)) * FS_ROWB + xlA] = (uint8_t)sA;
                    if (sB > 0) sc[(slB - (slB >= FS_SCR ? FS_SCR : 0)) * FS_ROWB + xlB] = (uint8_t)sB;
                    const bool cA = sA > 0 && qA == qlast, cB = sB > 0 && qB == qlast;
                    const bool keepA = sA > 0 && qA != qlast, keepB = sB > 0 && qB != qlast;
                    const unsigned long long bRA = __builtin_amdgcn_ballot_w64(keepA), bRB = __builtin_amdgcn_ballot_w64(keepB);
                    const unsigned long long bCA = __builtin_amdgcn_ballot_w64(cA), bCB = __builtin_amdgcn_ballot_w64(cB);
                    auto rank = [&](unsigned long long bm) -> int {
                        return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
                    };
                    if (keepA) Q[nR + rank(bRA)] = (uint16_t)((xlA << 3) | rA);                       // (decoded: position << 3 | row, what the NMS reads)
                    if (keepB) Q[nR + __popcll(bRA) + rank(bRB)] = (uint16_t)((xlB << 3) | rB);
                    nR += __popcll(bRA) + __popcll(bRB);
                    if (cA) car_wr[nnew + rank(bCA)] = (uint8_t)xlA;
                    if (cB) car_wr[nnew + __popcll(bCA) + rank(bCB)] = (uint8_t)xlB;
                    nnew += __popcll(bCA) + __popcll(bCB);
                    WAVE_SYNC();
                }
            }
            // (3) 3x3 NMS + border cull over the carried row and this pass's scored rows but the last (every entry here has a score > 0)
            const int ntotal = ncar + nR;
            for (int i0 = 0; i0 < ntotal; i0 += 64) {
                const int i = i0 + lane;
                const bool act = i < ntotal, isc = i < ncar;
                const uint32_t e = Q[act && !isc ? i - ncar : 0];
                const int xl = isc ? (int)car_rd[i] : (int)(e >> 3) & 0xFF;
                const int q = isc ? qcar : 8 * c + (int)(e & 7u);
                const int s1 = sc_slot(q), s0 = s1 == 0 ? FS_SCR - 1 : s1 - 1, s2 = s1 == FS_SCR - 1 ? 0 : s1 + 1;
                const uint8_t* p1 = sc + (s1 * FS_ROWB + xl);
                const uint8_t* p0 = sc + (s0 * FS_ROWB + xl);
                const uint8_t* p2 = sc + (s2 * FS_ROWB + xl);
                // all eight neighbours at once (a short-circuit chain is up to eight dependent LDS round trips, and this kernel runs at 3-4 waves per SIMD)
                const int s = p1[0];
                const int n0 = p0[-1], n1 = p0[0], n2 = p0[1], n3 = p1[-1], n4 = p1[1], n5 = p2[-1], n6 = p2[0], n7 = p2[1];
                const int nmax = max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
                const int half = xl >> 7, xi = xl & 127;
                const int gx = (half ? V.x0[1] : V.x0[0]) + xi, gy = (half ? V.y0[1] : V.y0[0]) + q;
                const int qmax = 8 * (half ? nch1 : nch0) - 2;
                const bool em = act && s > nmax && q >= 1 && q <= qmax && xi >= 4 && xi <= 4 * FS_LANES - 5 &&
                                gx >= edge && gx < w - edge && gy >= edge && gy < h - edge;
                const unsigned long long bm = __builtin_amdgcn_ballot_w64(em);
                if (bm) {
                    const unsigned long long b1 = __builtin_amdgcn_ballot_w64(em && half), b0 = bm & ~b1;
                    const unsigned long long mine = half ? b1 : b0;
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
                    const uint32_t o = (half ? V.tile[1] : V.tile[0]) * TILE_CAND_CAP + (uint32_t)((half ? cnt1 : cnt0) + rank);
                    if (em) *(__attribute__((address_space(1))) uint32_t*)(uintptr_t)(candf + o) = ((uint32_t)s << 24) | ((uint32_t)gy << 12) | (uint32_t)gx;   // global, not flat
                    cnt0 += __popcll(b0); cnt1 += __popcll(b1);
                }
            }
            WAVE_SYNC();
            cur ^= 1; ncar = nnew; qcar = qlast;
        }
        // the next chunk's rows: ring slots of the load chunk that is no longer needed, 7-bit copies into the register window, and the
        // request for the chunk after it.  Unconditional (behind the last chunk the rows are clamped and never used): a load under a
        // condition gets a register of its own and a copy at the loop's back edge -- which has to WAIT for the load just issued.
        {
            const int par = c & 1;
#pragma unroll
            for (int i = 0; i < 8; i++) px32[(8 * par + i) * FS_ROWD + lane] = nxt[i];
            if (par == 0) {
#pragma unroll
                for (int i = 0; i < FS_MIRROR; i++) px32[(FS_RING + i) * FS_ROWD + lane] = nxt[i];
            }
            // (the empty asm ties the row offset to the reduced values: the loads below cannot be scheduled in front of the last use of
            // the registers they are to land in -- otherwise they get registers of their own and a copy behind a vmcnt(0) at the back edge)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t t = (nxt[i] >> 1) & M7;
                asm volatile("" : "+v"(t), "+v"(voff));
                old[i] = nw[i]; nw[i] = t;
            }
            load8(nxt);
            WAVE_SYNC();
        }
    }
    if (lane == 0) {
        int32_t* tc = tile_cnt + (size_t)f * total_tiles + V.tile_base;
        if (nch0) tc[V.tile[0]] = cnt0;
        if (nch1) tc[V.tile[1]] = cnt1;
    }
}

#define FS_WPB 1                 // waves per workgroup (the waves of a workgroup share nothing)
// ONE launch for all pyramid levels of all frames.  Grid (8, waves / FS_WPB, ceil(frames / 8)): blockIdx.x is the XCD the workgroup
// lands on (workgroups are dealt to the 8 XCDs round-robin in x-fastest order), so all work of frame 8 z + x meets in one L2
// -- the same placement as xcd_frame_map() without its integer divisions.
__global__ __launch_bounds__(64 * FS_WPB) void k_fast(const FastWave* __restrict__ waves, const uint8_t* __restrict__ frames0, int total_tiles, int total_waves,
                                                       int threshold, int edge, int32_t* __restrict__ tile_cnt, int nframes, const int32_t* __restrict__ tau) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[FS_WPB * FS_WAVE_LDS];
    const int f = blockIdx.z * 8 + blockIdx.x;
    const int wi = blockIdx.y * FS_WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (f >= nframes || wi >= total_waves) return;
    const FastWave V = waves[wi];
    fast_wave(V, frames0, total_tiles, f, tau ? tau[V.nl >> 16] : threshold, edge, tile_cnt, lds + (threadIdx.x >> 6) * FS_WAVE_LDS);
}

// work list: fix[0] = number of (frame, level) entries, fix[1 + i] = frame * L + level.  A small fixed grid walks
// (entry, wave of that level) items; with an empty list (the normal case) every wave leaves at once.
struct FixLevels { int wave_base[VIS_MAX_LEVELS], nwaves[VIS_MAX_LEVELS], L, max_waves; };
__global__ __launch_bounds__(64 * FS_WPB) void k_fast_fix(const FastWave* __restrict__ waves, const uint8_t* __restrict__ frames0, int total_tiles,
                                                           int threshold, int edge, int32_t* __restrict__ tile_cnt, FixLevels X,
                                                           const int32_t* __restrict__ fix) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[FS_WPB * FS_WAVE_LDS];
    const int items = fix[0] * X.max_waves;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int wk = blockIdx.x * FS_WPB + wv; wk < items; wk += gridDim.x * FS_WPB) {
        const int e = fix[1 + wk / X.max_waves], j = wk % X.max_waves;
        const int f = e / X.L, l = e - f * X.L;
        if (j < X.nwaves[l]) {                                        // wave-uniform
            const FastWave V = waves[X.wave_base[l] + j];
            fast_wave(V, frames0, total_tiles, f, threshold, edge, tile_cnt, lds + wv * FS_WAVE_LDS);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_select
struct LevelArgs {
    const uint8_t* img; size_t frame_bytes;
    const uint32_t* cand; float4* seg_kp;
    int w, h, stride, quota, surv_cap, keep_cap, ntiles, tile_base; float scale;
};
struct DetLevels { LevelArgs lv[VIS_MAX_LEVELS]; int L; };

__device__ __forceinline__ uint32_t fmap(float f) {            // order-preserving float -> uint
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funmap(uint32_t m) {
    uint32_t u = (m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m;
    return __uint_as_float(u);
}

// HarrisResponses(blockSize 7, k 0.04) at integer (x,y) of one level
__device__ __forceinline__ float harris7(const uint8_t* __restrict__ img, int stride, int x, int y) {
    int a = 0, b = 0, c = 0;
    const uint8_t* p0 = img + (size_t)(y - 4) * stride + (x - 4);
    // 9 x 9 neighbourhood as 9 x 3 unaligned dwords (27 loads instead of 81 byte loads); every kept
    // candidate is >= edge_threshold (>= 22) pixels inside the image, so x-4 .. x+7 stays inside the row
    uint32_t w[9][3];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint8_t* pr = p0 + (size_t)i * stride;
        w[i][0] = *reinterpret_cast<const u32_unaligned*>(pr);
        w[i][1] = *reinterpret_cast<const u32_unaligned*>(pr + 4);
        w[i][2] = *reinterpret_cast<const u32_unaligned*>(pr + 8);
    }
#define HPX(i, j) ((int)((w[i][(j) >> 2] >> (8 * ((j) & 3))) & 0xFFu))
#pragma unroll
    for (int i = 1; i <= 7; i++) {
#pragma unroll
        for (int j = 1; j <= 7; j++) {
            const int Ix = (HPX(i, j + 1) - HPX(i, j - 1)) * 2 + (HPX(i - 1, j + 1) - HPX(i - 1, j - 1)) + (HPX(i + 1, j + 1) - HPX(i + 1, j - 1));
            const int Iy = (HPX(i + 1, j) - HPX(i - 1, j)) * 2 + (HPX(i + 1, j - 1) - HPX(i - 1, j - 1)) + (HPX(i + 1, j + 1) - HPX(i - 1, j + 1));
            a += Ix * Ix; b += Iy * Iy; c += Ix * Iy;
        }
    }
#undef HPX
    const float scale = 1.f / ((1 << 2) * 7 * 255.f);
    const float scale_sq_sq = scale * scale * scale * scale;
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float s = fa + fb;
    return (fa * fb - fc * fc - 0.04f * s * s) * scale_sq_sq;
}

// the same as a real function: the second walk of k_select's windowed mode (rare: saturated images) calls it, so that a second inlined
// copy of the 27 loads does not raise the register count of the whole kernel (64 VGPRs = 8 waves per SIMD on the common path)
__device__ __attribute__((noinline)) float harris7_call(const uint8_t* __restrict__ img, int stride, int x, int y) { return harris7(img, stride, x, y); }

#ifdef VIS_FAST_PROFILE
__device__ unsigned long long g_sel_stamps[VIS_MAX_LEVELS * 8];      // diagnostic build: cycles per (level, phase) summed over workgroups
extern "C" int vis_debug_select_stamps(unsigned long long out[VIS_MAX_LEVELS * 8]) {
    if (hipDeviceSynchronize() != hipSuccess) return VIS_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sel_stamps), sizeof(g_sel_stamps)) != hipSuccess) return VIS_E_HIP;
    unsigned long long z[VIS_MAX_LEVELS * 8] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_sel_stamps), z, sizeof(z)) == hipSuccess ? VIS_OK : VIS_E_HIP;
}
#endif
// tau / t_base / seg_cut / fix: the speculative threshold (fast_tile); tau == nullptr: plain FAST at t_base
#define SEL_ARGS DetLevels D, const int32_t* __restrict__ tile_cnt, int total_tiles, int32_t* __restrict__ seg_cnt, \
                 int32_t* __restrict__ flags, int max_surv, int nframes, const int32_t* __restrict__ tau, int t_base, \
                 int32_t* __restrict__ seg_cut, int32_t* fix
#define SEL_NT 256
__global__ __launch_bounds__(256) void k_select(SEL_ARGS) {
#include "select_body.inc"
}
#undef SEL_NT
// 1024 threads per (frame, level) when a level sorts thousands of survivors (N = 4000 / 8000): the LDS bitonic sort and the
// gather loops are the critical path of a launch that has only frames x levels workgroups
#define SEL_NT 1024
__global__ __launch_bounds__(1024) void k_select_1024(SEL_ARGS) {
#include "select_body.inc"
}
#undef SEL_NT
// the (frame, level) pairs whose predicted threshold was too high, after k_fast_fix redid their tiles at t
#define SEL_FIX
#define SEL_NT 256
__global__ __launch_bounds__(256) void k_select_fix(SEL_ARGS) {
#include "select_body.inc"
}
#undef SEL_NT
#define SEL_NT 1024
__global__ __launch_bounds__(1024) void k_select_fix_1024(SEL_ARGS) {
#include "select_body.inc"
}
#undef SEL_NT
#undef SEL_FIX

// next batch's prediction: per level the smallest cut of this batch's frames minus a margin, never below t
#define TAU_MARGIN 4
__global__ __launch_bounds__(256) void k_tau_update(const int32_t* __restrict__ seg_cut, int L, int nframes, int t_base, int32_t* __restrict__ tau) {
    __shared__ int smin[VIS_MAX_LEVELS];
    const int tid = threadIdx.x;
    if (tid < VIS_MAX_LEVELS) smin[tid] = 255;
    __syncthreads();
    for (int l = 0; l < L; l++) {
        int m = 255;
        for (int f = tid; f < nframes; f += 256) m = min(m, seg_cut[(size_t)f * L + l]);
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) atomicMin(&smin[l], m);
    }
    __syncthreads();
    if (tid < L) tau[tid] = max(t_base, smin[tid] - TAU_MARGIN);
}

// ------------------------------------------------------------------------------------------------
// k_describe: one wave per keypoint
#define PR 21                 // raw patch radius: 18 (max rotated sample offset) + 3 (blur taps)
#define PW 43
#define PS 48                 // raw patch LDS row stride: 16-byte rows, the MFMA A operand of the row pass is one aligned ds_read_b128
#define HW 40                 // horizontally blurred columns stored (patch cols 3..42; samples use 3..39)
#define HTS 46                // the row-blurred patch is stored TRANSPOSED: hbT[col][row], 46 u16 per column (odd dword
                              // stride): the 7 vertical taps of a sample are then 4 consecutive dwords
#define WAVE_LDS ((PW * PS + HW * HTS * 2 + 8 + 15) / 16 * 16)     // bytes per wave, multiple of 16 (>= 4 spare bytes behind the blur buffer)

// the rBRIEF pattern as floats (x0, y0, x1, y1 per bit): the rotation works on floats, and 1024 int8 -> float conversions
// per keypoint are not free
__device__ const float g_pattern[256 * 4] = {
#include "orb_pattern.inc"
};

struct DescArgs {
    int umax[16];
    int kq[7];                // 7-tap Gaussian, Q8
    uint32_t k0, k1;          // the same taps packed as bytes for v_dot4_u32_u8: (k0..k3), (k4..k6, 0)
    uint32_t kp[4];           // and as u16 pairs for v_dot2_u32_u16: (k0,k1) (k2,k3) (k4,k5) (k6,0)
    const uint32_t* angle_tab; // [31 rows][9 dwords][2]: byte weights (u+16 inside the disc, else 0) and byte mask (1/0)
    float rad_per_deg;        // (float)(CV_PI/180.f)
    int patch_size;
};

__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// deterministic double sin/cos: Cody-Waite by pi/2 + fdlibm kernels, IEEE + - * only (no FMA)
__device__ __forceinline__ void sincos_det(double x, double* s, double* c) {
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632673412561417e+00;
    const double PIO2_LO = 6.07710050650619224932e-11;
    const double kd = rint(x * TWO_OVER_PI);
    const int k = (int)kd;
    const double r = (x - kd * PIO2_HI) - kd * PIO2_LO;
    const double z = r * r;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
    const double sr = r + (r * z) * ps;
    const double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
    const double cr = (1.0 - 0.5 * z) + (z * z) * pc;
    switch (k & 3) {
        case 0: *s = sr;  *c = cr;  break;
        case 1: *s = cr;  *c = -sr; break;
        case 2: *s = -sr; *c = -cr; break;
        default: *s = -cr; *c = sr; break;
    }
}

// sum over the 64 lanes of a wave: 4 DPP adds (quad swaps, half-row and row mirrors) + 4 v_readlane
__device__ __forceinline__ int wave_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);    // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);    // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// Three wave sums at once (exact integers, any order): after the first two butterfly steps the lanes of a quad carry DIFFERENT sums
// (lane & 3 = 0: a, 1: b, 2 and 3: c), the remaining steps move whole quads -- row rotations by 4 and 8, then gfx950's
// v_permlane16_swap / v_permlane32_swap between the rows -- so every lane ends with the total of its own sum: 17 vector
// instructions + 3 v_readlane instead of 3 x (4 + 4 v_readlane + 3 scalar adds).
__device__ __forceinline__ void wave_sum3(int& a, int& b, int& c) {
    const int lane = (int)__lane_id();
    a += __builtin_amdgcn_update_dpp(0, a, 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]
    b += __builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, false);
    c += __builtin_amdgcn_update_dpp(0, c, 0xB1, 0xF, 0xF, false);
    int v = (lane & 1) ? b : a;
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
    c += __builtin_amdgcn_update_dpp(0, c, 0x4E, 0xF, 0xF, false);
    int w = (lane & 2) ? c : v;
    w += __builtin_amdgcn_update_dpp(0, w, 0x124, 0xF, 0xF, false);    // row_ror:4
    w += __builtin_amdgcn_update_dpp(0, w, 0x128, 0xF, 0xF, false);    // row_ror:8
    typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
    v2u_t r = __builtin_amdgcn_permlane16_swap((unsigned)w, (unsigned)w, false, false);   // rows (0,1) and (2,3)
    w = (int)(r.x + r.y);
    r = __builtin_amdgcn_permlane32_swap((unsigned)w, (unsigned)w, false, false);         // the two halves
    w = (int)(r.x + r.y);
    a = __builtin_amdgcn_readlane(w, 0); b = __builtin_amdgcn_readlane(w, 1); c = __builtin_amdgcn_readlane(w, 2);
}

// Everything that identifies the keypoint (level, index, patch origin) is wave-uniform and is kept in SGPRs
// (v_readfirstlane), so per-lane addresses are 32-bit offsets from scalar bases; lane -> (row, column)
// mappings are fixed per phase, so the unrolled loops only add constants.
// (at most 96 SGPRs: from 97 on the hardware admits one workgroup fewer per CU than the 7 that LDS and VGPRs allow)
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96), amdgpu_waves_per_eu(7, 8))) void k_describe(DetLevels D, DescArgs G, const int32_t* __restrict__ seg_cnt,
                                                  vis_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
                                                  int32_t* __restrict__ nkp, int kcap, int rec0,
                                                  int32_t* __restrict__ flags, int nframes) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * WAVE_LDS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // grid (8, keypoint groups, ceil(frames / 8)): blockIdx.x is the XCD (see k_fast)
    const int f = blockIdx.z * 8 + blockIdx.x, kb = blockIdx.y;
    if (f >= nframes) return;
    // all level counts of the frame arrive with ONE scalar load (the buffer is padded by VIS_MAX_LEVELS words)
    struct SegCounts { int c[VIS_MAX_LEVELS]; };
    const SegCounts SC = *reinterpret_cast<const SegCounts*>(seg_cnt + (size_t)f * D.L);
    int total = 0;
#pragma unroll
    for (int l = 0; l < VIS_MAX_LEVELS; l++) total += l < D.L ? SC.c[l] : 0;
    if (total > kcap) { total = kcap; if (kb == 0 && wv == 0 && lane == 0) atomicOr(flags, 8); }
    if (kb == 0 && wv == 0 && lane == 0) nkp[rec0 + f] = total;
    uint8_t* raw = lds + wv * WAVE_LDS;
    uint32_t* hb32 = reinterpret_cast<uint32_t*>(raw + PW * PS);
    // A wave walks over keypoints g, g + waves-per-frame, ...: the launch has a few ten thousand workgroups instead of one
    // per four keypoints.  (With 353 k workgroups per 1024 frames the kernel spent half its time in workgroup dispatch:
    // waves that returned right after the prologue still took 0.54 of its 1.11 ms.)
    // lane l < L holds the packed index at which level l starts (INT_MAX beyond the last level): locating a keypoint is then
    // one compare + ballot + popcount + v_readlane instead of a scalar search over the levels
    int vstart = 0x7FFFFFFF;
    {
        int run = 0;
#pragma unroll
        for (int l = 0; l < VIS_MAX_LEVELS; l++) {
            if (l < D.L && lane == l) vstart = run;
            run += l < D.L ? SC.c[l] : 0;
        }
    }
    // The patch is kept in LDS as SIGNED bytes (pixel - 128: the i8 matrix instruction has no unsigned form).  The IC moments do not
    // notice: sum u (I - 128) = sum u I and sum v (I - 128) = sum v I over the symmetric disc, in exact integers.
#define PATCH_BIAS 0x80808080u
#define PATCH_DOT4(p, w) (__builtin_amdgcn_sdot4((int)(p), (int)(w), 0, false))
    // B operand of the row pass (see there): dword q of lane (g, j) = taps e .. e + 3, e = 16 g + 4 q - j, taps outside 0 .. 6 = 0
    typedef int v4i_t0 __attribute__((ext_vector_type(4)));
    v4i_t0 hp_b;
    {
        const unsigned long long K = (unsigned long long)G.k0 | ((unsigned long long)G.k1 << 32);
        const int e0 = 16 * (lane >> 4) - (lane & 15);
        uint32_t bq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = e0 + 4 * q;
            bq[q] = (e >= 7 || e <= -4) ? 0u : (e >= 0 ? (uint32_t)(K >> (8 * (e & 7))) : (uint32_t)(K << (8 * ((-e) & 7))));
        }
        hp_b = v4i_t0{(int)bq[0], (int)bq[1], (int)bq[2], (int)bq[3]};
    }
    const int hp_c0 = 128 * (G.kq[0] + G.kq[1] + G.kq[2] + G.kq[3] + G.kq[4] + G.kq[5] + G.kq[6]);
    const int lrs = (lane * 47) >> 9, lc = lane - lrs * 11;          // patch map: lane = (row % 5 [+ spare rows], dword); lane / 11
    uint8_t* const lw = raw + lrs * PS + 4 * lc;
    const uint2* const ic_tb = reinterpret_cast<const uint2*>(G.angle_tab) + min(lane, 62);
    // The kept-keypoint record (x, y, response, y << 16 | x) is wave-uniform: it comes through the SCALAR cache, and the record of the
    // wave's NEXT keypoint is requested one iteration ahead, so its HBM latency runs beside this keypoint's work instead of in front
    // of the patch loads (a keypoint was a chain of four exposed memory round trips: record -> patch -> IC weights -> pattern).
    typedef uint32_t u32x4_s __attribute__((ext_vector_type(4)));
    auto rec_request = [&](int gq) -> u32x4_s {
        const int lq = __popcll(__builtin_amdgcn_ballot_w64(gq >= vstart)) - 1;
        const int iq = gq - __builtin_amdgcn_readlane(vstart, lq);
        const float4* p = D.lv[lq].seg_kp + ((size_t)f * D.lv[lq].keep_cap + iq);
        // a load through the CONSTANT address space with a wave-uniform address = s_load_dwordx4 that the compiler's own wait-count
        // bookkeeping tracks (k_select wrote the records in an earlier launch; nothing in this kernel writes them)
        return *(const __attribute__((address_space(4))) u32x4_s*)(uintptr_t)p;
    };
    const int gstride = (int)gridDim.y * 4;
    int g = kb * 4 + wv;
    if (g >= total) return;
    // the rBRIEF pattern of this lane's four bits stays in registers for all keypoints of the wave (it was re-read per keypoint:
    // 4 of a keypoint's 21 vector memory instructions and one more exposed round trip)
    float4 pat[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pat[k] = *reinterpret_cast<const float4*>(g_pattern + 4 * (lane + 64 * k));
    // Software pipeline over the wave's keypoints: the 9 patch dwords of the NEXT keypoint are requested in the middle of this one
    // (right after the row pass has read the patch out of LDS) and stay in registers until the top of the next iteration; the record
    // that gives their address was requested an iteration earlier through the scalar cache.  A keypoint was a chain of four exposed
    // memory round trips (record -> patch -> IC weights -> pattern); now none of them is in front of its arithmetic.
    uint32_t pv[9];
    auto patch_request = [&](const u32x4_s& r, int gq) {
        const int lq = __popcll(__builtin_amdgcn_ballot_w64(gq >= vstart)) - 1;
        const LevelArgs& Aq = D.lv[lq];
        const int sq = Aq.stride;
        const int xq = (int)(r.w & 0xFFFFu), yq = (int)(r.w >> 16);
        const uint8_t* img = Aq.img + (size_t)f * Aq.frame_bytes + (size_t)(yq - PR) * sq + (xq - PR);
        // 43 rows x 44 bytes as 11 unaligned dwords per row; lane = (row % 5, dword), 9 loads cover rows 0..44.  No predicates: the
        // spare lanes 55..63 copy rows 5, 10, .. 45 once more, rows beyond 42 repeat row 42, and what is stored beyond row 42 lands
        // in the first bytes of the blur buffer, which the row pass rewrites before anything reads it.
        const uint32_t goff = (uint32_t)(__mul24(lrs, sq) + 4 * lc);
        const int gstep = 5 * sq;
#pragma unroll
        for (int k = 0; k < 8; k++) pv[k] = *reinterpret_cast<const u32_unaligned*>((img + (size_t)k * gstep) + goff);
        // rows 40 .. 45: clamped to the last patch row (with the smallest legal edge_threshold, 22, rows 43 .. 45 may lie below the image)
        pv[8] = *reinterpret_cast<const u32_unaligned*>(img + (uint32_t)(__mul24(min(lrs + 40, PW - 1), sq) + 4 * lc));
    };
    u32x4_s rec = rec_request(g);
    u32x4_s rec_next = rec_request(min(g + gstride, total - 1));
    patch_request(rec, g);
    for (; g < total; g += gstride) {
    const int lev = __popcll(__builtin_amdgcn_ballot_w64(g >= vstart)) - 1;       // level-major packed index -> (level, index in level)
    const LevelArgs& A = D.lv[lev];
    struct { float x, y, z; } kpr = {__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z)};
    uint2 icw[5];
    {
#pragma unroll
        for (int k = 0; k < 5; k++) icw[k] = ic_tb[63 * k];
#pragma unroll
        for (int k = 0; k < 9; k++) *reinterpret_cast<uint32_t*>(lw + k * 5 * PS) = pv[k] ^ PATCH_BIAS;
    }
    WAVE_SYNC();
    // IC angle over the radius-15 disc: each (row, dword) item is two byte dot products against a
    // precomputed weight/mask table: m10 = sum (u+16) I - 16 sum I,  m01 = sum v I   (all exact integers).
    // lane = (row % 7, dword); the table is padded with zero rows up to 35.
    int sA = 0, sB = 0, sC = 0;
    if (lane < 63) {
        const int rs = (lane * 57) >> 9, dw = lane - rs * 9;          // lane / 9
        const uint8_t* pr = raw + (PR - 15 + rs) * PS + 4 + 4 * dw;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint32_t pixw = *reinterpret_cast<const uint32_t*>(pr + k * 7 * PS);
            const uint2 wm = icw[k];
            const int a = PATCH_DOT4(pixw, wm.x);
            const int b = PATCH_DOT4(pixw, wm.y);
            sA += a; sB += b; sC += __mul24(rs + 7 * k - 15, b);
        }
    }
    wave_sum3(sA, sB, sC);
    const int m10 = sA - 16 * sB, m01 = sC;
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    // Horizontal 7-tap pass on the MATRIX pipe: H = (patch - 128) x T + 128 * sum(w) with the banded constant T[k][c] = w[k - c],
    // exact in the i32 accumulators of v_mfma_i32_16x16x64_i8.  Tile (t, n) = rows 16t .. 16t+15, blur columns 16n .. 16n+15: the A
    // operand of lane (g, i) is the 16 patch bytes of row 16t + i from column 16n + 16g (one aligned ds_read_b128; only the first
    // 22 columns meet a non-zero weight), the B operand -- lane (g, j): w[16g + s - j], s = 0 .. 15 -- is the SAME for every tile
    // (the band only moves with the columns A starts at).  Lane (g, j) receives rows 16t + 4g .. + 3 of column 16n + j = two
    // dwords of the transposed blur buffer: 2 v_perm_b32 + one 8-byte LDS store per tile instead of 80 v_dot4 per keypoint.
    // Rows 43 .. 47 (beyond the patch: whatever follows it in LDS) only reach blur rows that no sample touches; the store of
    // lanes g = 3 of the tiles t = 2 runs two rows over the column's 46 -- into rows 0, 1 of the next column, which the t = 0
    // tile of that column writes AFTERWARDS (one wave's LDS stores execute in order; the last column runs into the spare bytes).
    {
        const int hi_ = lane & 15, hg = lane >> 4;
        // lanes g = 2, 3 only ever meet zero weights: they all read the patch's first bytes (one broadcast address per 16-lane
        // group instead of 16 more addresses for the bank arbiter: the LDS array is this kernel's busiest unit, SQ_LDS_IDX_ACTIVE 97 %)
        const uint8_t* abase = hg < 2 ? raw + hi_ * PS + 16 * hg : raw;
        uint32_t* wbase = hb32 + hi_ * (HTS / 2) + 2 * hg;
        typedef int v4i_t __attribute__((ext_vector_type(4)));
        const v4i_t cin = {hp_c0, hp_c0, hp_c0, hp_c0};
        const bool c2 = hi_ < HW - 32;           // the third column tile holds blur columns 32 .. 39 only (the matrix instruction itself always runs with every lane)
        // the three column tiles of a row tile together: loads, matrix instructions, packs (the accumulators stay in VGPRs:
        // -amdgpu-mfma-vgpr-form, Makefile); the store addresses of the second / third column tile are re-formed per keypoint
        // (two full-rate adds) instead of living in registers across the loop
        auto row_tiles = [&](int t) {
            v4i_t av[3], d[3];
#pragma unroll
            for (int n = 0; n < 3; n++) av[n] = *reinterpret_cast<const v4i_t*>(abase + t * 16 * PS + 16 * n);
#pragma unroll
            for (int n = 0; n < 3; n++) d[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[n], hp_b, cin, 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 3; n++) {
                const uint32_t lo = __builtin_amdgcn_perm((uint32_t)d[n].y, (uint32_t)d[n].x, 0x05040100u);
                const uint32_t hi = __builtin_amdgcn_perm((uint32_t)d[n].w, (uint32_t)d[n].z, 0x05040100u);
                uint32_t wofs = (uint32_t)(n * 16 * (HTS / 2) * 4);
                asm volatile("" : "+v"(wofs));                       // keep it an add in the loop, not nine hoisted addresses
                uint32_t* w = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(wbase) + wofs) + t * 8;
                if (n < 2 || c2) { w[0] = lo; w[1] = hi; }
            }
        };
        row_tiles(2);
        WAVE_SYNC();
        row_tiles(1);
        row_tiles(0);
    }
    // the patch has left LDS: request the next keypoint's (and the record of the one after it)
    rec = rec_next;
    patch_request(rec, min(g + gstride, total - 1));
    rec_next = rec_request(min(g + 2 * gstride, total - 1));
    WAVE_SYNC();
    float ang = angle;
    ang *= G.rad_per_deg;
    double sd, cd;
    sincos_det((double)ang, &sd, &cd);
    const float a = (float)cd, b = (float)sd;
    unsigned long long words[4];
    // LDS byte address of blur-buffer element (column PR-3, row PR-3) of this wave, as a float (< 2^24: exact)
    const float tap0_f = (float)((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)reinterpret_cast<unsigned char*>(hb32)
                                 + (uint32_t)((PR - 3) * (HTS * 2) + 2 * (PR - 3)));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float4 pt = pat[k];
        int val[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const float px = e ? pt.z : pt.x, py = e ? pt.w : pt.y;
            const float fx = px * a - py * b;
            const float fy = px * b + py * a;
            // cvRound of both coordinates stays in float (v_rndne), and the LDS byte address of the first vertical tap --
            // column (PR+ix-3) of the transposed blur buffer, row (PR+iy-3): 92 ix + 2 iy + constant -- is formed there too:
            // every term is a small integer, so the two fused multiply-adds are exact; one conversion instead of two plus
            // the integer address arithmetic.  The 7 taps are 4 consecutive dwords from the address rounded down to 4.
            const float rx = rintf(fx), ry = rintf(fy);
            const uint32_t ab = (uint32_t)(int)__fmaf_rn(rx, (float)(HTS * 2), __fmaf_rn(ry, 2.f, tap0_f));
            const uint32_t* cw = (const uint32_t*)(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)(ab & ~3u);
            const uint32_t sh = ab;                                  // v_alignbyte_b32 shifts by bits [1:0] of its third operand (0 or 2 here: the address is even)
            const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2], w3 = cw[3];
            typedef unsigned short us2 __attribute__((ext_vector_type(2)));
            const uint32_t t0 = __builtin_amdgcn_alignbyte(w1, w0, sh), t1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
            const uint32_t t2 = __builtin_amdgcn_alignbyte(w3, w2, sh), t3 = __builtin_amdgcn_alignbyte(0u, w3, sh);
            uint32_t su = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, t0), __builtin_bit_cast(us2, G.kp[0]), 0u, false);
            su = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, t1), __builtin_bit_cast(us2, G.kp[1]), su, false);
            su = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, t2), __builtin_bit_cast(us2, G.kp[2]), su, false);
            su = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, t3), __builtin_bit_cast(us2, G.kp[3]), su, false);
            int s = (int)((su + (1u << 15)) >> 16);
            val[e] = s > 255 ? 255 : s;
        }
        words[k] = __builtin_amdgcn_ballot_w64(val[0] < val[1]);
    }
    uint8_t* dout = desc + ((size_t)(rec0 + f) * kcap + g) * 32;
    if (lane < 4) reinterpret_cast<unsigned long long*>(dout)[lane] = words[lane];
    if (lane == 0) {
        vis_keypoint kp;
        kp.x = kpr.x * A.scale; kp.y = kpr.y * A.scale;
        kp.size = (float)G.patch_size * A.scale;
        kp.angle = angle; kp.response = kpr.z; kp.octave = lev; kp.class_id = -1;
        kps[(size_t)(rec0 + f) * kcap + g] = kp;
    }
    WAVE_SYNC();        // the next keypoint's patch overwrites this wave's LDS region
    }
}

// ------------------------------------------------------------------------------------------------
// Camera::Update half pyramid (src/Camera.cpp:68-70), single-frame entry: cv::resize's area-fast path -- (a+b+c+d+2)>>2 over a complete
// 2x2 block, the mean of the pixels that exist (round half to even) in the last column / row of a level that is one larger than half
// of an odd source size (see gradient.hip k_half4 / oracle/orb.cpp orc_half_pyramid)
__global__ void k_half(const uint8_t* __restrict__ src, int sw, int sh, int sstride, uint8_t* __restrict__ dst, int dw, int dh) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const uint8_t* s = src + (size_t)(2 * y) * sstride + 2 * x;
    const bool right = 2 * x + 1 < sw, below = 2 * y + 1 < sh;
    if (right && below) dst[(size_t)y * dw + x] = (uint8_t)((s[0] + s[1] + s[sstride] + s[sstride + 1] + 2) >> 2);
    else {
        const int sum = s[0] + (right ? s[1] : 0) + (below ? s[sstride] : 0), count = 1 + (right ? 1 : 0) + (below ? 1 : 0);
        dst[(size_t)y * dw + x] = (uint8_t)__float2int_rn((float)sum / (float)count);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
static void fill_det_levels(const Plan* pl, const uint8_t* d_frames, DetLevels& D) {
    D.L = pl->L;
    for (int l = 0; l < pl->L; l++) {
        LevelArgs& A = D.lv[l];
        A.img = l == 0 ? d_frames : pl->d_pyr[l];
        A.frame_bytes = pl->lv[l].frame_bytes;
        A.cand = pl->d_cand[l]; A.seg_kp = pl->d_seg_kp[l];
        A.w = pl->lv[l].w; A.h = pl->lv[l].h; A.stride = pl->lv[l].stride;
        A.quota = pl->lv[l].quota; A.surv_cap = pl->lv[l].surv_cap; A.keep_cap = pl->lv[l].keep_cap;
        A.ntiles = pl->lv[l].tiles_x * pl->lv[l].tiles_y; A.tile_base = pl->lv[l].tile_base; A.scale = pl->lv[l].scale;
    }
}

static void fill_desc_args(const vis_params& p, DescArgs& G, std::vector<uint32_t>* tab_out) {
    // ORB umax table for halfPatchSize = 15 (computed exactly as ORB_Impl does)
    const int hp = p.patch_size / 2;
    int umax[17] = {0};
    int v, v0, vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1);
    int vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
    for (v = 0; v <= vmax; ++v) umax[v] = (int)std::lrint(std::sqrt((double)hp * hp - v * v));
    for (v = hp, v0 = 0; v >= vmin; --v) { while (umax[v0] == umax[v0 + 1]) ++v0; umax[v] = v0; ++v0; }
    for (int i = 0; i < 16; i++) G.umax[i] = umax[i];
    // getGaussianKernel(7, 2, CV_32F) -> Q8 integers (cvRound(k*256))
    const int n = 7; const double sigma = 2.0;
    double scale2X = -0.5 / (sigma * sigma), sum = 0; float cf[7];
    for (int i = 0; i < n; i++) { double x = i - (n - 1) * 0.5; cf[i] = (float)std::exp(scale2X * x * x); sum += cf[i]; }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) { cf[i] = (float)(cf[i] * sum); G.kq[i] = (int)std::lrint((double)cf[i] * 256.0); }
    G.k0 = (uint32_t)G.kq[0] | ((uint32_t)G.kq[1] << 8) | ((uint32_t)G.kq[2] << 16) | ((uint32_t)G.kq[3] << 24);
    G.k1 = (uint32_t)G.kq[4] | ((uint32_t)G.kq[5] << 8) | ((uint32_t)G.kq[6] << 16);
    G.kp[0] = (uint32_t)G.kq[0] | ((uint32_t)G.kq[1] << 16); G.kp[1] = (uint32_t)G.kq[2] | ((uint32_t)G.kq[3] << 16);
    G.kp[2] = (uint32_t)G.kq[4] | ((uint32_t)G.kq[5] << 16); G.kp[3] = (uint32_t)G.kq[6];
    G.rad_per_deg = (float)(M_PI / 180.f);
    G.patch_size = p.patch_size;
    G.angle_tab = nullptr;
    if (tab_out) {
        // row rv (v = rv-15), dword dw covers patch columns 4+4dw .. 7+4dw, i.e. u = pc - 21
        tab_out->assign(35 * 9 * 2, 0u);       // 31 rows + 4 zero rows (k_describe's fixed lane mapping over-runs)
        for (int rv = 0; rv < 31; rv++)
            for (int dw = 0; dw < 9; dw++) {
                uint32_t wv = 0, mv = 0;
                for (int b = 0; b < 4; b++) {
                    const int u = 4 + 4 * dw + b - 21, v = rv - 15;
                    const int au = u < 0 ? -u : u, av = v < 0 ? -v : v;
                    if (au <= 15 && au <= umax[av]) { wv |= (uint32_t)(u + 16) << (8 * b); mv |= 1u << (8 * b); }
                }
                (*tab_out)[2 * (rv * 9 + dw)] = wv; (*tab_out)[2 * (rv * 9 + dw) + 1] = mv;
            }
    }
}

// the per-wave records of k_fast (levels >= 1 point into the plan's pyramid; level 0 is the batch of the call: img = nullptr).
// Item i of a level = (segment i / strips, strip i % strips); a wave takes items 2 j and 2 j + 1 of ONE level.
int build_fast_tiles(vis_ctx* ctx, Plan* pl) {
    std::vector<FastWave> t;
    const int e = ctx->p.edge_threshold;
    const int x00 = (e - 4) & ~3;                       // pixel column of lane 0 of the first strip (vis_compute_levels)
    const int emit_h = 8 * pl->fs_nch - 2;             // emitting rows per segment of this plan
    for (int l = 0; l < pl->L; l++) {
        LevelInfo& V = pl->lv[l];
        const int items = V.tiles_x * V.tiles_y;
        if (V.frame_bytes > 0xFFFFFFFFull || items > 65535) return VIS_E_INVALID;
        V.wave_base = (int)t.size(); V.nwaves = (items + 1) / 2;
        const int emit_rows = V.h - 2 * e;
        for (int j = 0; j < V.nwaves; j++) {
            FastWave r = {};
            r.img = l == 0 ? nullptr : pl->d_pyr[l]; r.cand = pl->d_cand[l]; r.frame_bytes = (uint32_t)V.frame_bytes;
            r.stride = V.stride; r.wh = (uint32_t)V.w | ((uint32_t)V.h << 16);
            r.ntiles = (uint32_t)items; r.tile_base = (uint32_t)V.tile_base;
            uint32_t nch[2] = {0, 0};
            for (int k = 0; k < 2; k++) {
                const int i = std::min(2 * j + k, items - 1);          // (an idle second half repeats the first one's geometry: its loads stay inside the image)
                const int seg = i / V.tiles_x, strip = i % V.tiles_x;
                r.x0[k] = x00 + strip * VIS_FS_EMIT_W; r.y0[k] = e - 1 + seg * emit_h; r.tile[k] = (uint32_t)i;
                // emitting rows of the segment -> chunks of 8 score rows (one halo row above and below)
                const int rows = std::max(0, std::min(emit_h, emit_rows - seg * emit_h));
                nch[k] = 2 * j + k < items ? (uint32_t)std::max(1, (rows + 2 + 7) / 8) : 0u;
            }
            r.nl = nch[0] | (nch[1] << 8) | ((uint32_t)l << 16);
            t.push_back(r);
        }
    }
    pl->total_waves = (int)t.size();
    if (pl->total_waves > 65535 * FS_WPB) return VIS_E_INVALID;          // k_fast: gridDim.y
    HIPCHK(ctx, hipMalloc((void**)&pl->d_fast_tiles, t.size() * sizeof(FastWave)));
    HIPCHK(ctx, hipMemcpy(pl->d_fast_tiles, t.data(), t.size() * sizeof(FastWave), hipMemcpyHostToDevice));
    return VIS_OK;
}

// The small clears and copies in front of a batch as ONE launch: every hipMemsetAsync / hipMemcpyAsync is a launch of its own
// (5 us each with its gaps) on the stream that carries the detect chain -- six of them were 1 % of the step.
struct SmallOps { uint32_t* dst[6]; const uint32_t* src[6]; uint32_t end[6]; int n; };     // job j: dwords [end[j-1], end[j]), src == nullptr: clear
__global__ __launch_bounds__(256) void k_small_ops(SmallOps J) {
    const uint32_t total = J.end[J.n - 1];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        int j = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) j += (k < J.n - 1 && i >= J.end[k]) ? 1 : 0;
        const uint32_t o = i - (j ? J.end[j - 1] : 0u);
        J.dst[j][o] = J.src[j] ? J.src[j][o] : 0u;
    }
}

// up to six dword-granular copies (src == nullptr: clear) in ONE launch on `st`; the destinations may be device-accessible host memory
int launch_copy_jobs(vis_ctx* ctx, hipStream_t st, int njobs, void* const* dst, const void* const* src, const size_t* bytes) {
    if (njobs < 1 || njobs > 6) return VIS_E_INVALID;
    SmallOps J = {}; uint32_t e = 0;
    for (int k = 0; k < njobs; k++) { J.dst[k] = (uint32_t*)dst[k]; J.src[k] = (const uint32_t*)src[k]; e += (uint32_t)(bytes[k] / 4); J.end[k] = e; }
    J.n = njobs;
    if (!e) return VIS_OK;
    hipLaunchKernelGGL(k_small_ops, dim3((unsigned)std::min<uint32_t>(1024u, (e + 255u) / 256u)), dim3(256), 0, st, J);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

int launch_detect(vis_ctx* ctx, Plan* pl, const uint8_t* d_frames, int n, int rec0, int carry_rec, hipEvent_t after_resize, const ReaderGuard* records_free) {
    hipStream_t st = ctx->stream;
    const int L = pl->L;
    {
        SmallOps J = {}; uint32_t e = 0; int k = 0;
        auto job = [&](void* d, const void* s, size_t bytes) { J.dst[k] = (uint32_t*)d; J.src[k] = (const uint32_t*)s; e += (uint32_t)(bytes / 4); J.end[k] = e; k++; };
        job(pl->d_tile_cnt, nullptr, sizeof(int32_t) * (size_t)pl->B * pl->total_tiles);
        job(pl->d_seg_cnt, nullptr, sizeof(int32_t) * (size_t)pl->B * L);
        if (pl->speculate) job(pl->d_fix, nullptr, sizeof(int32_t));
        J.n = k;
        hipLaunchKernelGGL(k_small_ops, dim3((unsigned)std::min<uint32_t>(1024u, (e + 255u) / 256u)), dim3(256), 0, st, J);
        HIPCHK(ctx, hipGetLastError());
    }
    DetLevels D; fill_det_levels(pl, d_frames, D);
    DescArgs G;
    if (!pl->d_angle_tab) {
        std::vector<uint32_t> tab; fill_desc_args(ctx->p, G, &tab);
        HIPCHK(ctx, hipMalloc((void**)&pl->d_angle_tab, tab.size() * 4));
        HIPCHK(ctx, hipMemcpy(pl->d_angle_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    } else fill_desc_args(ctx->p, G, nullptr);
    G.angle_tab = pl->d_angle_tab;
    int nfast = 0;
    for (int l = 1; l < L; l++) {
        const LevelInfo& V = pl->lv[l];
        const LevelInfo& U = pl->lv[l - 1];
        const int bxc = (V.w + 3) / 4, per_frame = resize_index_blocks(bxc, V.h, RS_ROWS);   // bxc = 4-px groups per row
        const uint32_t magic = resize_index_magic((uint32_t)bxc);                           // (only the narrow variant decodes with it)
        // scale exactly as cv::resize derives it: inv_scale = (double)dsize/ssize; scale = 1./inv_scale
        const double scale_x = 1. / ((double)V.w / U.w), scale_y = 1. / ((double)V.h / U.h);
        if (scale_x <= 2.0 && bxc >= 12) {       // (256 threads then span at most 23 row groups = 230 rows of coefficients)
            if (!pl->d_rs_tab[l]) {              // first use of the plan: tabulate the step's coefficients
                const size_t words = (size_t)12 * bxc + (size_t)4 * V.h;
                HIPCHK(ctx, hipMalloc((void**)&pl->d_rs_tab[l], words * 4));
                hipLaunchKernelGGL(k_resize_tab, dim3((std::max(bxc, V.h) + 255) / 256), dim3(256), 0, st, pl->d_rs_tab[l], bxc, V.w, V.h, U.w, U.h, U.stride, scale_x, scale_y);
                HIPCHK(ctx, hipStreamSynchronize(st));       // (once: later launches may come from another stream)
            }
            hipLaunchKernelGGL(k_resize<true>, dim3(xcd_grid(n, per_frame)), dim3(64, 4), 0, st, D.lv[l - 1].img, U.w, U.h, U.stride, U.frame_bytes,
                               pl->d_pyr[l], V.w, V.h, V.stride, V.frame_bytes, scale_x, scale_y, bxc, per_frame, n, (const uint32_t*)pl->d_rs_tab[l], magic);
        } else
            hipLaunchKernelGGL(k_resize<false>, dim3(xcd_grid(n, per_frame)), dim3(64, 4), 0, st, D.lv[l - 1].img, U.w, U.h, U.stride, U.frame_bytes,
                               pl->d_pyr[l], V.w, V.h, V.stride, V.frame_bytes, scale_x, scale_y, bxc, per_frame, n, (const uint32_t*)nullptr, magic);
    }
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[1], st);
    if (after_resize) HIPCHK(ctx, hipEventRecord(after_resize, st));      // the side stream's streaming work starts here (vis_batch_run); behind k_fast or k_select instead: same frames/s (round 5)
    const int t_base = ctx->p.fast_threshold;
    const int32_t* tau = pl->speculate ? pl->d_tau : nullptr;            // batched streams only (see fast_tile)
    {
        hipLaunchKernelGGL(k_fast, dim3(8, (pl->total_waves + FS_WPB - 1) / FS_WPB, (n + 7) / 8), dim3(64 * FS_WPB), 0, st, (const FastWave*)pl->d_fast_tiles, d_frames,
                           pl->total_tiles, pl->total_waves, t_base, ctx->p.edge_threshold, pl->d_tile_cnt, n, tau);
        nfast = 1;
    }
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[2], st);
    int max_surv = 0; for (int l = 0; l < L; l++) max_surv = std::max(max_surv, pl->lv[l].surv_cap);
    int max_nt = 0; for (int l = 0; l < L; l++) max_nt = std::max(max_nt, pl->lv[l].tiles_x * pl->lv[l].tiles_y);
    const size_t sel_lds = (size_t)max_surv * 8 + 16 + 1024 + ((size_t)max_nt + 2) * 4 + 1024;   // keys | flags | hist | tile prefix | suffix sums
    const bool big = max_surv > 1024;    // large quotas: 1024 threads per (frame, level)
    if (sel_lds > 65536) {   // > 64 KiB of dynamic LDS needs the opt-in attribute (160 KiB per CU on gfx950)
        HIPCHK(ctx, hipFuncSetAttribute(big ? (const void*)k_select_1024 : (const void*)k_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel_lds));
        if (pl->speculate)
            HIPCHK(ctx, hipFuncSetAttribute(big ? (const void*)k_select_fix_1024 : (const void*)k_select_fix, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel_lds));
    }
    int32_t* seg_cut = pl->speculate ? pl->d_seg_cut : nullptr;
    int32_t* fix = pl->speculate ? pl->d_fix : nullptr;
    if (big) hipLaunchKernelGGL(k_select_1024, dim3(xcd_grid(n, L)), dim3(1024), sel_lds, st, D, pl->d_tile_cnt, pl->total_tiles,
                                pl->d_seg_cnt, pl->d_flags, max_surv, n, tau, t_base, seg_cut, fix);
    else hipLaunchKernelGGL(k_select, dim3(xcd_grid(n, L)), dim3(256), sel_lds, st, D, pl->d_tile_cnt, pl->total_tiles,
                            pl->d_seg_cnt, pl->d_flags, max_surv, n, tau, t_base, seg_cut, fix);
    if (pl->speculate) {
        // redo what the prediction got wrong (normally nothing: both grids find an empty list and leave), then predict the next batch
        FixLevels X; X.L = L; X.max_waves = 1;
        for (int l = 0; l < VIS_MAX_LEVELS; l++) { X.wave_base[l] = l < L ? pl->lv[l].wave_base : 0; X.nwaves[l] = l < L ? pl->lv[l].nwaves : 0; X.max_waves = std::max(X.max_waves, X.nwaves[l]); }
        hipLaunchKernelGGL(k_fast_fix, dim3(4096 / FS_WPB), dim3(64 * FS_WPB), 0, st, (const FastWave*)pl->d_fast_tiles, d_frames, pl->total_tiles, t_base,
                           ctx->p.edge_threshold, pl->d_tile_cnt, X, (const int32_t*)pl->d_fix);
        const int fix_grid = n * L;                      // one workgroup per possible work-list entry (<= 4096 frames x 16 levels)
        if (big) hipLaunchKernelGGL(k_select_fix_1024, dim3(fix_grid), dim3(1024), sel_lds, st, D, pl->d_tile_cnt, pl->total_tiles,
                                    pl->d_seg_cnt, pl->d_flags, max_surv, n, tau, t_base, seg_cut, fix);
        else hipLaunchKernelGGL(k_select_fix, dim3(fix_grid), dim3(256), sel_lds, st, D, pl->d_tile_cnt, pl->total_tiles,
                                pl->d_seg_cnt, pl->d_flags, max_surv, n, tau, t_base, seg_cut, fix);
        hipLaunchKernelGGL(k_tau_update, dim3(1), dim3(256), 0, st, (const int32_t*)pl->d_seg_cut, L, n, t_base, pl->d_tau);
        HIPCHK(ctx, hipGetLastError());
    }
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[3], st);
    // The records of this batch (k_describe writes them; the previous batch's last frame is copied in front of them) are the first thing
    // of the chain that touches the record set the matcher of an earlier batch may still be reading: the detect stream waits for that
    // matcher HERE, not at the start of the chain (round 5 timeline: a quarter of a millisecond of idle detect stream per step) -- the
    // resize chain, k_fast and k_select of this batch run meanwhile.
    if (records_free) HIPCHK(ctx, records_free->wait(st));
    if (carry_rec >= 0) {              // the previous batch's last frame -> the record in front of this batch's first (rec0 - 1)
        SmallOps J = {}; uint32_t e = 0; int k = 0;
        auto job = [&](void* d, const void* s, size_t bytes) { J.dst[k] = (uint32_t*)d; J.src[k] = (const uint32_t*)s; e += (uint32_t)(bytes / 4); J.end[k] = e; k++; };
        const size_t d = (size_t)(rec0 - 1), c = (size_t)carry_rec;
        job(pl->d_kps + d * pl->kcap, pl->d_kps + c * pl->kcap, (size_t)pl->kcap * sizeof(vis_keypoint));
        job(pl->d_desc + d * pl->kcap * 32, pl->d_desc + c * pl->kcap * 32, (size_t)pl->kcap * 32);
        job(pl->d_nkp + d, pl->d_nkp + c, 4);
        J.n = k;
        hipLaunchKernelGGL(k_small_ops, dim3((unsigned)std::min<uint32_t>(1024u, (e + 255u) / 256u)), dim3(256), 0, st, J);
    }
    // workgroups per frame: enough to fill the chip for small batches, a wave walks over many keypoints for large ones
    const int desc_groups = std::max(1, std::min((pl->kcap + 3) / 4, (16384 + n - 1) / n));
    hipLaunchKernelGGL(k_describe, dim3(8, desc_groups, (n + 7) / 8), dim3(256), 0, st, D, G, pl->d_seg_cnt,
                       pl->d_kps, pl->d_desc, pl->d_nkp, pl->kcap, rec0, pl->d_flags, n);
    if (ctx->ev_ok) (void)hipEventRecord(ctx->ev[4], st);
    ctx->tm.launches_fast = nfast;
    ctx->tm.launches_total = (L - 1) + 1 + 2;
    HIPCHK(ctx, hipGetLastError());
    pl->pyr_frames = n;                 // (vis_debug_pyramid_level: the frames whose levels this chain writes)
    return VIS_OK;
}

int launch_half_pyramid(vis_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, uint8_t* d_out[5]) {
    const uint8_t* src = d_img; int sw = w, sh = h, ss = stride;
    for (int l = 1; l < 5; l++) {
        const int dw = vis_half_dim(sw), dh = vis_half_dim(sh);
        if (dw < 1 || dh < 1) return VIS_E_INVALID;
        dim3 block(64, 4), grid((dw + 63) / 64, (dh + 3) / 4);
        hipLaunchKernelGGL(k_half, grid, block, 0, ctx->stream, src, sw, sh, ss, d_out[l], dw, dh);
        src = d_out[l]; sw = dw; sh = dh; ss = dw;
    }
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}
