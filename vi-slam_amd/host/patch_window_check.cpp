// patch_window_check -- csrc/patch_window.h walked on the CPU: every hostile keypoint coordinate of tests/align_hostile_cases.py (and a
// sweep of ordinary ones) through patch_span() on every level, and hostile candidate coordinates through source_index().  Each answer
// is compared with the rule of include/vislam_hip.h evaluated the slow way -- every integer 1 ... size - 1 tested in double -- and every
// call must return, which the reference's loop does not for a coordinate of +inf or >= 2^31.  `make -C vi-slam_amd/csrc` builds it with
// -fsanitize=undefined,address where the compiler has the runtimes (a float -> int conversion out of range is a UBSan finding and ends
// the run); tests/test_align_hostile_ref.py runs it.  Host code only: no device, no library.
#include "../csrc/patch_window.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int fails = 0, calls = 0;

static void check_span(float kp, int level, int size0) {
    const int patch_size = level == 1 ? 3 : (level == 2 ? 2 : 5);
    const int sp = patch_size - 1 / 2;
    const int size = size0 >> level;
    const float factor_lvl = (float)(1.0 / (double)(1 << level));
    const float c = (float)(((double)kp + 0.5) * (double)factor_lvl - 0.5);       // as k_align / k_patch_points form it
    const PatchSpan s = patch_span(c, sp, size);
    calls++;
    // the rule, one integer at a time
    const float a = c - (float)sp, b = c + (float)sp;
    int lo = 1, hi = 0; bool any = false, holes = false;
    if (std::isfinite(c))
        for (int i = 1; i < size; i++) {
            const bool in = (double)i >= std::trunc((double)a) && (float)i <= b;
            if (in && !any) { lo = hi = i; any = true; }
            else if (in) { if (i != hi + 1) holes = true; hi = i; }
        }
    const bool same = any ? (s.lo == lo && s.hi == hi) : s.lo > s.hi;
    if (!same || holes || patch_span_count(s) != (any ? hi - lo + 1 : 0) || (s.lo <= s.hi && (s.lo < 1 || s.hi > size - 1))) {
        std::printf("FAIL  kp %.9g level %d size %d: span [%d, %d], rule [%d, %d]\n", (double)kp, level, size, s.lo, s.hi, lo, hi);
        fails++;
    }
}

static void check_index(float v, int size) {
    int got = -12345;
    const bool ok = source_index(v, size, got);
    calls++;
    const bool want = v > -1.f && v < (float)size;                                 // 0 <= trunc(v) < size
    if (ok != want || (ok && got != (int)std::trunc((double)v)) || (!ok && got != -12345)) {
        std::printf("FAIL  source_index(%.9g, %d) = %d, %d\n", (double)v, size, (int)ok, got);
        fails++;
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[] = {16, 23, 120, 160, 176, 752, 4095};
    for (const int size0 : sizes) {
        std::vector<float> v = {nan, -nan, inf, -inf, 3e38f, -3e38f, 1e30f, -1e30f, 3e9f, -3e9f, 4294967296.f, -4294967296.f, 1e9f, -1e9f,
                                std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), (float)size0 + 40.f, -40.f,
                                std::nextafterf(2147483648.f, 0.f), -2147483648.f, std::nextafterf(-2147483648.f, -inf), 0.f, -0.f, 1e-45f, -1e-38f};
        for (int l = 0; l <= 4; l++) {
            const float p = 2147483648.f * (float)(1 << l);
            v.push_back(p); v.push_back(std::nextafterf(p, 0.f)); v.push_back(-p); v.push_back(std::nextafterf(-p, 0.f));
        }
        for (float x = -48.f; x <= (float)size0 + 48.f; x += 0.25f) v.push_back(x);        // ordinary coordinates, windows clipped on both sides
        for (const float kp : v)
            for (int l = 0; l <= 4; l++) check_span(kp, l, size0);
        for (int l = 0; l <= 4; l++) {
            const int size = size0 >> l;
            const float w[] = {nan, inf, -inf, 3e38f, -3e38f, 3e9f, -3e9f, 2147483648.f, -2147483648.f, -1.f, std::nextafterf(-1.f, 0.f), -0.5f, -0.f, 0.f,
                               0.5f, (float)size - 0.5f, std::nextafterf((float)size, 0.f), (float)size, (float)size + 0.5f, 1e-45f, -1e-45f};
            for (const float x : w) check_index(x, size);
        }
    }
#if defined(__SANITIZE_ADDRESS__)
    const char* how = "address + undefined sanitizers";
#else
    const char* how = "no sanitizer";
#endif
    std::printf("%d calls, %d failures (%s)\n", calls, fails, how);
    if (fails) return 1;
    std::printf("patch_window_check passed\n");
    return 0;
}
