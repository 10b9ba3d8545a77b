// geometry.cpp -- host-side tables of the detector: pyramid level geometry, per-level feature
// quotas, grid-filter band limits, and the
// integer-only synthetic stream generator, the rectification tables.  Plain C++ (no device code).
//
// Follows what cv::ORB / cv::resize derive for the reference call site
// /root/reference/src/Camera.cpp:87 (cv::ORB::detectAndCompute) -- see SURVEY.md Appendix A.1
// items 2-3 -- and Matcher::bestMatchesFilter's window arithmetic (/root/reference/src/Matcher.cpp:171-216).
#include "vis_internal.h"
#include "synth_core.h"
#include <cfloat>
#include <cmath>
#include <cstring>

static inline int round_half_even(double v) { return (int)std::lrint(v); }

int vis_compute_levels(const vis_params& p, int w, int h, int stride0, LevelInfo* lv, int fs_nch) {
    if (fs_nch < 1 || fs_nch > VIS_FS_NCH) return VIS_E_INVALID;
    const int emit_h = 8 * fs_nch - 2;                 // emitting rows of a k_fast segment (a plan's choice: see plan_create)
    if (p.nlevels < 1 || p.nlevels > VIS_MAX_LEVELS || p.nfeatures < 1) return VIS_E_INVALID;
    if (w < 2 * p.edge_threshold + 8 || h < 2 * p.edge_threshold + 8 || w > 4095 || h > 4095) return VIS_E_INVALID;
    const double sf = (double)p.scale_factor;            // ORB keeps the float argument in a double member
    for (int l = 0; l < p.nlevels; l++) {
        float s = (float)std::pow(sf, (double)l);
        lv[l].scale = s;
        lv[l].w = round_half_even((double)((float)w / s));
        lv[l].h = round_half_even((double)((float)h / s));
        if (lv[l].w < 8 || lv[l].h < 8) return VIS_E_INVALID;
        lv[l].stride = (l == 0) ? stride0 : ((lv[l].w + 63) / 64) * 64;
        lv[l].frame_bytes = (size_t)lv[l].stride * lv[l].h;
        // FAST items (k_fast, detect.hip): a strip segment of VIS_FS_EMIT_W x (8 fs_nch - 2) emitting positions inside the region that can
        // emit keypoints, [edge, w-edge) x [edge, h-edge); the pixel window of the first strip starts at a dword-aligned column
        // (edge - 4 rounded down to 4; its first emitting column is 4 pixels further).  tiles_x = strips, tiles_y = segments.
        const int e = p.edge_threshold, ex0 = ((e - 4) & ~3) + 4;
        lv[l].tiles_x = std::max(1, (lv[l].w - e - ex0 + VIS_FS_EMIT_W - 1) / VIS_FS_EMIT_W);
        lv[l].tiles_y = std::max(1, (lv[l].h - 2 * e + emit_h - 1) / emit_h);
        lv[l].cand_cap = lv[l].tiles_x * lv[l].tiles_y * VIS_TILE_CAND_CAP;
        lv[l].tile_base = l == 0 ? 0 : lv[l - 1].tile_base + lv[l - 1].tiles_x * lv[l - 1].tiles_y;
    }
    float factor = (float)(1.0 / sf);
    float nd = p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)p.nlevels));
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; l++) {
        lv[l].quota = round_half_even((double)nd);
        sum += lv[l].quota;
        nd *= factor;
    }
    lv[p.nlevels - 1].quota = std::max(p.nfeatures - sum, 0);
    // vis_params.keypoint_capacity beyond the default total is slack that ANY level may use (ties at the Harris cut sit on one level)
    int def_total = 0;
    for (int l = 0; l < p.nlevels; l++) def_total += lv[l].quota + lv[l].quota / 8 + 32;
    const int extra = std::max(0, p.keypoint_capacity - def_total);
    for (int l = 0; l < p.nlevels; l++) {
        int q = lv[l].quota;
        // survivors of the FAST-score cut: 2*quota plus ties at the cut (FAST scores are small
        // integers, ties are common); kept after the Harris cut: quota plus ties.
        int sc = 2 * q + q / 2 + 256;
        int pw = 64; while (pw < sc) pw <<= 1;
        if (pw > 8192) return VIS_E_INVALID;             // LDS sort limit (64 KiB of keys)
        while (pw < sc + extra && pw < 8192) pw <<= 1;    // a raised capacity also widens the one-round sort (k_select's LDS), up to that limit
        lv[l].surv_cap = pw;
        lv[l].keep_cap = std::min(q + q / 8 + 32 + extra, pw);
    }
    return VIS_OK;
}

// Matcher::bestMatchesFilter window limits: winW = w_size/floor(sqrt(n)) stored as float, limits
// accumulated in float exactly like `h_final = h_final + winHSize` (src/Matcher.cpp:177-178,203,229).
void vis_grid_limits(const vis_params& p, int* root, std::vector<float>& hf, std::vector<float>& wf) {
    // 1 <= root <= VIS_MAX_GRID_ROOT: validate_params refuses every other n_cells, so the root that sizes the cells is the root that counts them
    const double rd = std::floor(std::sqrt((double)p.n_cells));
    const int r = (int)rd;
    *root = r;
    float winW = (float)(p.w_size / rd);
    float winH = (float)(p.h_size / rd);
    hf.resize(r); wf.resize(r);
    float a = winH, b = winW;
    for (int j = 0; j < r; j++) { hf[j] = a; wf[j] = b; a = a + winH; b = b + winW; }
}

// ------------------------------------------------------------------------------------------------
// Synthetic EuRoC-shaped stream ("S-752"); integer arithmetic only so the
// bytes are identical on every host.  PRNG = xorshift64*.
struct XorShift64s {
    uint64_t s;
    explicit XorShift64s(uint64_t seed) : s(seed ? seed : 0x9E3779B97F4A7C15ULL) {}
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1DULL; }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
};

extern "C" int vis_synth_canvas(uint8_t* canvas, int dim, uint64_t seed) {
    if (!canvas || dim < 64) return VIS_E_INVALID;
    XorShift64s rng(seed);
    const size_t n = (size_t)dim * dim;
    std::memset(canvas, 128, n);
    const double area_ratio = (double)n / (4096.0 * 4096.0);
    const int nrect = std::max(8, (int)(24000 * area_ratio));
    const int nblob = std::max(8, (int)(12000 * area_ratio));
    for (int i = 0; i < nrect; i++) {
        int rw = 6 + (int)rng.below(59), rh = 6 + (int)rng.below(59);      // 6..64
        int x = (int)rng.below((uint32_t)dim), y = (int)rng.below((uint32_t)dim);
        uint8_t v = (uint8_t)rng.below(256);
        for (int yy = y; yy < std::min(dim, y + rh); yy++) std::memset(canvas + (size_t)yy * dim + x, v, (size_t)std::min(rw, dim - x));
    }
    for (int i = 0; i < nblob; i++) {
        int s = 3 + (int)rng.below(5);                                    // 3..7
        int x = (int)rng.below((uint32_t)dim), y = (int)rng.below((uint32_t)dim);
        uint8_t v = (uint8_t)rng.below(256);
        for (int yy = y; yy < std::min(dim, y + s); yy++) std::memset(canvas + (size_t)yy * dim + x, v, (size_t)std::min(s, dim - x));
    }
    // one 3x3 box blur, replicate border, rounded integer mean
    std::vector<uint8_t> src(canvas, canvas + n);
    for (int y = 0; y < dim; y++) {
        int y0 = y > 0 ? y - 1 : 0, y1 = y < dim - 1 ? y + 1 : dim - 1;
        for (int x = 0; x < dim; x++) {
            int x0 = x > 0 ? x - 1 : 0, x1 = x < dim - 1 ? x + 1 : dim - 1;
            int s = src[(size_t)y0 * dim + x0] + src[(size_t)y0 * dim + x] + src[(size_t)y0 * dim + x1] +
                    src[(size_t)y * dim + x0] + src[(size_t)y * dim + x] + src[(size_t)y * dim + x1] +
                    src[(size_t)y1 * dim + x0] + src[(size_t)y1 * dim + x] + src[(size_t)y1 * dim + x1];
            canvas[(size_t)y * dim + x] = (uint8_t)((s + 4) / 9);
        }
    }
    return VIS_OK;
}

// origins of the layers at frame t (host side: the PRNG draws happen once per stream)
int vis_synth_origin(int dim, uint64_t seed, int t, int w, int h, SynthOrigin* o) {
    if (w < 1 || h < 1 || w >= dim || h >= dim || t < 0 || dim < 64) return VIS_E_INVALID;
    XorShift64s rng(seed ^ 0xD1B54A32D192ED03ULL);
    const int rx = dim - w, ry = dim - h;
    const int ox = (int)rng.below((uint32_t)rx), oy = (int)rng.below((uint32_t)ry);
    o->x0 = (int)(((int64_t)ox + 12LL * t) % rx); o->y0 = (int)(((int64_t)oy + 8LL * t) % ry);
    // the layer offsets stay non-negative for every t < 2^20 so that >> 6 and / 48 are plain floor divisions
    const int mx0 = (int)rng.below(4096), my0 = (int)rng.below(4096), ux0 = (int)rng.below(4096), uy0 = (int)rng.below(4096);
    o->mx = mx0 + 18 * t; o->my = my0 + 12 * t;
    o->ux = ux0 + 48 * 200000 - 7 * t; o->uy = uy0 + 15 * t;
    return VIS_OK;
}

static int synth_frame_mode(const uint8_t* canvas, int dim, uint64_t seed, int t, int w, int h, uint8_t* out, int out_stride, int mode) {
    if (!canvas || !out || out_stride < w) return VIS_E_INVALID;
    SynthOrigin o;
    const int rc = vis_synth_origin(dim, seed, t, w, h, &o);
    if (rc) return rc;
    for (int y = 0; y < h; y++) {
        uint8_t* d = out + (size_t)y * out_stride;
        for (int x = 0; x < w; x++) d[x] = synth_pixel(canvas, dim, seed, t, w, x, y, mode, o);
    }
    return VIS_OK;
}

extern "C" int vis_synth_frame(const uint8_t* canvas, int dim, uint64_t seed, int t,
                               int w, int h, uint8_t* out, int out_stride) {
    return synth_frame_mode(canvas, dim, seed, t, w, h, out, out_stride, 0);
}

extern "C" int vis_synth_frame_parallax(const uint8_t* canvas, int dim, uint64_t seed, int t,
                                        int w, int h, uint8_t* out, int out_stride) {
    return synth_frame_mode(canvas, dim, seed, t, w, h, out, out_stride, 1);
}

// ---- rectification (vi::CameraModel, src/CameraModel.cpp:84-90): the new camera matrix and the CV_16SC2 + CV_16UC1 tables ----------
// Both restate OpenCV 3.2 from the published algorithm (the source is not part of this project): PARITY UNPINNED, like every other
// OpenCV restatement here.  -ffp-contract=off (Makefile): no product is fused into a sum.
static bool rect_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 4095 && h <= 4095; }
static bool rect_focal_ok(const float K[4]) { return std::isfinite(K[0]) && std::isfinite(K[1]) && K[0] > 0.f && K[1] > 0.f; }

// cv::getOptimalNewCameraMatrix(alpha = 1, centerPrincipalPoint = false) as calib3d 3.2 computes it (calibration.cpp:
// cvGetOptimalNewCameraMatrix -> icvGetRectangles -> cvUndistortPoints):
//   1. a 9 x 9 grid of pixel positions (x * w / 8, y * h / 8), stored as float;
//   2. each is undistorted into normalised coordinates by 5 fixed-point iterations of the inverse Brown model (double);
//   3. outer = bounding box of the 81 results (float); with alpha = 1 the new projection maps it onto the output viewport:
//      fx' = (out_w - 1) / outer.width, cx' = -fx' * outer.x (same for y).
extern "C" int vis_optimal_new_camera_matrix(const float K[4], const float dist[4], int in_w, int in_h, int out_w, int out_h, float Knew[4]) {
    if (!K || !dist || !Knew || !rect_size_ok(in_w, in_h) || !rect_size_ok(out_w, out_h) || !rect_focal_ok(K)) return VIS_E_INVALID;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3];
    float oX0 = FLT_MAX, oX1 = -FLT_MAX, oY0 = FLT_MAX, oY1 = -FLT_MAX;
    const int N = 9;
    for (int y = 0; y < N; y++)
        for (int x = 0; x < N; x++) {
            const float u = (float)x * in_w / (N - 1), v = (float)y * in_h / (N - 1);
            double xn = ((double)u - cx) * (1.0 / fx), yn = ((double)v - cy) * (1.0 / fy);
            const double x0 = xn, y0 = yn;
            for (int j = 0; j < 5; j++) {
                const double r2 = xn * xn + yn * yn;
                const double icdist = 1.0 / (1 + (k2 * r2 + k1) * r2);
                const double dX = 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn);
                const double dY = p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn;
                xn = (x0 - dX) * icdist; yn = (y0 - dY) * icdist;
            }
            const float px = (float)xn, py = (float)yn;
            oX0 = std::min(oX0, px); oX1 = std::max(oX1, px); oY0 = std::min(oY0, py); oY1 = std::max(oY1, py);
        }
    const float ow = oX1 - oX0, oh = oY1 - oY0;                                       // cv::Rect_<float>(oX0, oY0, oX1 - oX0, oY1 - oY0)
    const double fx1 = (out_w - 1) / (double)ow, fy1 = (out_h - 1) / (double)oh;
    const double cx1 = -fx1 * oX0, cy1 = -fy1 * oY0;
    Knew[0] = (float)fx1; Knew[1] = (float)fy1; Knew[2] = (float)cx1; Knew[3] = (float)cy1;
    return VIS_OK;
}

// cvRound(double) on x86-64 (cvtsd2si): round half to even; NaN and results outside int32 give INT_MIN -- what saturate_cast<int>
// (double) is in OpenCV 3.2
static inline int rect_cvround(double v) {
    const double r = std::nearbyint(v);
    if (!(r >= -2147483648.0 && r < 2147483648.0)) return INT32_MIN;
    return (int)r;
}

// cv::initUndistortRectifyMap(K, dist, R = I, K', size, CV_16SC2, map1, map2) as imgproc 3.2 (undistort.cpp) computes it.  Everything in
// double; dist = (k1, k2, p1, p2), k3 ... k6, s1 ... s4 and the tilt are 0 (the tilt matrix is the identity).
//   iR = (K' R)^-1 by cv::invert(DECOMP_LU)'s closed form for a 3 x 3 double matrix (1 / det3, adjugate times it);
//   row i: _x = i ir[1] + ir[2], _y = i ir[4] + ir[5], _w = i ir[7] + ir[8]; column j: the three ACCUMULATE ir[0], ir[3], ir[6];
//   w = 1 / _w, x = _x w, y = _y w, r2 = x^2 + y^2, kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
//   xd = x kr + p1 2xy + p2 (r2 + 2x^2) + s1 r2 + s2 r2^2, yd likewise, tilt (xd, yd, 1) -> (xd', yd', z'), u = fx / z' xd' + u0;
//   iu = saturate_cast<int>(u * 32): map1 = (short)(iu >> 5), (short)(iv >> 5); map2 = (iv & 31) * 32 + (iu & 31).
extern "C" int vis_undistort_rectify_map(const float K[4], const float dist[4], const float Knew[4], int out_w, int out_h,
                                         int16_t* map1, uint16_t* map2) {
    if (!K || !dist || !Knew || !map1 || !map2 || !rect_size_ok(out_w, out_h) || !rect_focal_ok(K) || !rect_focal_ok(Knew)) return VIS_E_INVALID;
    const double A[9] = {(double)K[0], 0, (double)K[2], 0, (double)K[1], (double)K[3], 0, 0, 1};
    const double Ar[9] = {(double)Knew[0], 0, (double)Knew[2], 0, (double)Knew[1], (double)Knew[3], 0, 0, 1};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double S[9];                                                                      // Ar.colRange(0, 3) * R
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) S[3 * r + c] = Ar[3 * r] * I[c] + Ar[3 * r + 1] * I[3 + c] + Ar[3 * r + 2] * I[6 + c];
    auto m = [&](int r, int c) { return S[3 * r + c]; };
    double d = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) +
               m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0));
    if (d == 0.) return VIS_E_INVALID;                                                // (cv::invert leaves a zero matrix; K' > 0 cannot get here)
    d = 1. / d;
    const double ir[9] = {
        (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) * d, (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * d, (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * d,
        (m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)) * d, (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * d, (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * d,
        (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)) * d, (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * d, (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * d};
    const double u0 = A[2], v0 = A[5], fx = A[0], fy = A[4];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3];
    const double k3 = 0., k4 = 0., k5 = 0., k6 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0.;
    const double T[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};                                  // computeTiltProjectionMatrix(tauX = 0, tauY = 0)
    for (int i = 0; i < out_h; i++) {
        int16_t* m1 = map1 + (size_t)i * out_w * 2;
        uint16_t* m2 = map2 + (size_t)i * out_w;
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        for (int j = 0; j < out_w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double w = 1. / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
            const double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
            const double vt0 = T[0] * xd + T[1] * yd + T[2] * 1, vt1 = T[3] * xd + T[4] * yd + T[5] * 1, vt2 = T[6] * xd + T[7] * yd + T[8] * 1;
            const double invProj = vt2 ? 1. / vt2 : 1;
            const double u = fx * invProj * vt0 + u0, v = fy * invProj * vt1 + v0;
            const int iu = rect_cvround(u * 32), iv = rect_cvround(v * 32);               // INTER_TAB_SIZE = 32, INTER_BITS = 5
            m1[j * 2] = (int16_t)(iu >> 5);
            m1[j * 2 + 1] = (int16_t)(iv >> 5);
            m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return VIS_OK;
}
