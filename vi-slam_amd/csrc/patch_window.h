// patch_window.h -- the candidate window of Camera::ObtainPatchesPointsPreviousFrame (src/Camera.cpp:358-410) along one axis, and the
// truncation of a candidate's source pixel, defined for EVERY float (include/vislam_hip.h at vis_patch_points states the rule).  Shared
// by k_align<GEN> (align.hip) and k_patch_points (gradient.hip); plain C++ as well, so that host/patch_window_check.cpp can walk it on the
// CPU under a sanitizer.  oracle/gradient.cpp restates the rule on its own and does not include this file.
//
// The reference's loop is  for (int i = (int)(c - sp); (float)i <= c + sp; i++) if (i > 0 && i < size) ...  With c = +inf, or c + sp at or
// above 2^31, the condition holds for every int: i++ overflows and the loop never ends; (int) of a float outside int's range is
// undefined before that.  Here both bounds are clamped to [1, size - 1] as floats first; a float is converted only when it lies inside
// (1, size), where size <= 4095.
#pragma once

#if defined(__HIPCC__)
#define PW_FN __host__ __device__ inline
#else
#define PW_FN inline
#endif

struct PatchSpan { int lo, hi; };        // the integers lo ... hi; lo > hi: none

// the integers i with 0 < i < size, i >= trunc(c - sp) and (float)i <= c + sp, the sum and the difference taken in float as the
// reference takes them.  c NaN or infinite: none (every comparison with NaN is false; +inf fails the first test, -inf the second).
PW_FN PatchSpan patch_span(float c, int sp, int size) {
    const float a = c - (float)sp, b = c + (float)sp;
    PatchSpan s = {1, 0};
    if (!(a < (float)size) || !(b >= 1.f)) return s;        // the window ends left of 1 or starts right of size - 1 (or c is NaN)
    s.lo = a > 1.f ? (int)a : 1;                            // 1 < a < size: trunc(a) = (int)a; a <= 1: trunc(a) <= 1
    s.hi = b < (float)(size - 1) ? (int)b : size - 1;       // 1 <= b < size - 1: the largest i with (float)i <= b is (int)b
    return s;
}
PW_FN int patch_span_count(const PatchSpan& s) { return s.hi >= s.lo ? s.hi - s.lo + 1 : 0; }

// at<uchar>(y1, x1) of a candidate row: the column / row (int)v where that is inside [0, size), which is -1 < v < size ((int)(-0.5) == 0);
// false for every other float, NaN included, without converting it
PW_FN bool source_index(float v, int size, int& out) {
    if (!(v > -1.f && v < (float)size)) return false;
    out = (int)v;
    return true;
}
