// resize_index_check -- csrc/resize_index.h walked on the CPU: the multiply-high decode of k_resize's flat work index against plain / and %,
// exhaustively: every bx_count a level can have (3 ... 1024 column groups: image sides up to 4095) and, for each, every index a thread of
// the launch can hold -- 0 ... per_frame * 256 - 1 for the tallest level (4095 rows), the indices past the level's last row group
// included, since those threads decode too before they leave.  Also the values k_resize takes from its workgroup and its wave alone (first
// and last row group of 256 and of 64 consecutive indices) and the bound the header's comment states.  `make -C vi-slam_amd/csrc` builds it
// with -fsanitize=undefined,address where the compiler has the static runtimes; tests/test_resize_index.py runs it.  Host code only.
#include "../csrc/resize_index.h"
#include <cstdio>

int main() {
    const int rows = 5;                                  // RS_ROWS of csrc/detect.hip
    unsigned long long calls = 0, fails = 0;
    uint32_t largest = 0;
    for (uint32_t bxc = 3; bxc <= RESIZE_INDEX_MAX_GROUPS; bxc++) {
        const uint32_t magic = resize_index_magic(bxc);
        // magic = ceil(2^32 / bxc)
        const uint64_t two32 = 1ull << 32;
        if ((uint64_t)magic * bxc < two32 || (uint64_t)(magic - 1u) * bxc >= two32) { std::printf("FAIL  magic(%u) = %u\n", bxc, magic); fails++; }
        const uint32_t end = (uint32_t)resize_index_blocks((int)bxc, RESIZE_INDEX_MAX_SIDE, rows) * 256u;
        if (end > largest) largest = end;
        if ((uint64_t)end * bxc > two32) { std::printf("FAIL  bound: %u indices x %u groups\n", end, bxc); fails++; }
        for (uint32_t idx = 0; idx < end; idx++) {
            uint32_t rg, cg;
            resize_index_decode(idx, magic, bxc, rg, cg);
            if (rg != idx / bxc || cg != idx % bxc) {
                if (fails < 20) std::printf("FAIL  idx %u bx_count %u: (%u, %u), want (%u, %u)\n", idx, bxc, rg, cg, idx / bxc, idx % bxc);
                fails++;
            }
        }
        calls += end;
        // the uniform values: a workgroup's and a wave's first and last index
        for (uint32_t base = 0; base < end; base += 64u) {
            const uint32_t last = base + 63u, wg = base & ~255u;
            if (resize_index_row_group(last, magic) != last / bxc || resize_index_row_group(wg + 255u, magic) != (wg + 255u) / bxc ||
                resize_index_row_group(wg, magic) != wg / bxc) { std::printf("FAIL  uniform values at %u, bx_count %u\n", base, bxc); fails++; }
            // a workgroup spans at most 256 rows of coefficients (the LDS array of k_resize) once bx_count >= 12
            if (bxc >= 12 && ((wg + 255u) / bxc - wg / bxc + 1u) * rows > 256u) { std::printf("FAIL  %u rows in a workgroup, bx_count %u\n", ((wg + 255u) / bxc - wg / bxc + 1u) * rows, bxc); fails++; }
        }
    }
#if defined(__SANITIZE_ADDRESS__)
    const char* how = "address + undefined sanitizers";
#else
    const char* how = "no sanitizer";
#endif
    std::printf("%llu decodes, largest index %u, %llu failures (%s)\n", calls, largest - 1u, fails, how);
    if (fails) return 1;
    std::printf("resize_index_check passed\n");
    return 0;
}
