// resize_index.h -- the flat work index of k_resize and its exact integer decode, shared by host and device.
//
// A level of bx_count 4-pixel column groups and ceil(dh / rows) row groups is dealt to threads by a flat index
// idx = row group * bx_count + column group (rows are narrower than 256 pixels on most levels, a 2-D block mapping leaves a quarter of
// the lanes idle).  The decode back is floor(idx / bx_count), taken as the high word of a 32 x 32-bit product with
//     magic = ceil(2^32 / bx_count) = (2^32 + e) / bx_count,  0 <= e < bx_count:
//     idx * magic / 2^32 = idx / bx_count + idx * e / (bx_count * 2^32),
// and the second term stays below 1 / bx_count -- too small to carry the quotient over the next integer -- as long as idx * e < 2^32,
// for which idx * bx_count <= 2^32 suffices.  Image sides go up to 4095, so bx_count <= 1024 and idx < 1024 * 819 + 256 < 2^20: the
// decode is exact with no correction step (host/resize_index_check.cpp sweeps every legal pair against / and %).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RESIZE_INDEX_HD __host__ __device__ __forceinline__
#else
#define RESIZE_INDEX_HD inline
#endif

#define RESIZE_INDEX_MAX_SIDE 4095       // the largest image side a level can have
#define RESIZE_INDEX_MAX_GROUPS 1024     // (4095 + 3) / 4

// ceil(2^32 / d) for 2 <= d (d = 1 would need 33 bits; a level is never one column group wide)
RESIZE_INDEX_HD uint32_t resize_index_magic(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }

RESIZE_INDEX_HD uint32_t resize_index_row_group(uint32_t idx, uint32_t magic) { return (uint32_t)(((uint64_t)idx * magic) >> 32); }

RESIZE_INDEX_HD void resize_index_decode(uint32_t idx, uint32_t magic, uint32_t bx_count, uint32_t& rg, uint32_t& cg) {
    rg = resize_index_row_group(idx, magic);
    cg = idx - rg * bx_count;
}

// workgroups of 256 threads per frame of a level of bx_count column groups and dh rows, `rows` rows per thread
RESIZE_INDEX_HD int resize_index_blocks(int bx_count, int dh, int rows) { return (bx_count * ((dh + rows - 1) / rows) + 255) / 256; }
