// klt.hip -- pyramidal Lucas-Kanade tracking of keypoints on gfx950 (MI355X): vis_klt_track, vis_klt_batch, vis_batch_klt.
//
// Beyond the reference (it follows keypoints by descriptor only).  Per (pair, point) the work is a chain of at most
// levels x max_iters dependent Gauss-Newton steps over a window of n = (2r+1)^2 <= 441 pixels: latency, not bytes.
//
// Shape: ONE WAVE per (pair, point), four waves per workgroup, no workgroup barrier anywhere.  The template of a level (T, Dx, Dy of
// frame 1) lives in registers, PPL = ceil(n / 64) pixels per lane with compile-time indices (k_klt<4>: r <= 7, k_klt<7>: r <= 10); every
// sum is an integer, taken over the wave with an xor butterfly, so every lane holds the same sums and runs the same double arithmetic:
// the early exits are wave-uniform.  Frame 2's patch is read straight from memory (L2 after the first touch), not through LDS: the
// position changes with every step, so a staged patch would be written once and read once -- two dependent latencies (global -> LDS,
// LDS -> register) where the direct gather has one, for 4 bytes per pixel that neighbouring lanes share in the same cache lines.
// k_klt_pairs then counts the flags of a pair and compacts its tracked points in rising index with ballots (one wave per pair).
//
// The arithmetic is the contract of include/vislam_hip.h ("pyramidal KLT"); tests/klt_ref.py restates it, byte for byte.
#include "vis_internal.h"
#include <cmath>
#include <cstring>

#define DEV __device__ __forceinline__
#define KLT_WAVES 4

struct KltLevel {
    const uint8_t* img; const int16_t* gx; const int16_t* gy;     // level images of frame 0 of the batch
    size_t img_fstride, grad_fstride;                              // elements between consecutive frames
    int rowstride, lw, lh;                                         // row stride of img (the gradients are dense: lw)
};
struct KltArgs {
    KltLevel lv[5];
    int r, first, last, max_it, s;
    double eps2, min_eig, err_bound, fb2;                          // epsilon^2, min_eig, (max_err 32) n or 0, fb_max_px^2 or 0
    double lam_den;                                                // ((2 n)(32 s))(32 s)
    const float* pts; int pt_stride; size_t pts_row;              // point k of row q: pts[q pts_row + k pt_stride] (x), [+ 1] (y)
    const int32_t* npts; int rows_by_prev;                         // rows and counts are indexed by the pair (0) or by its previous frame (1)
    const float* guess; size_t guess_row;                          // rows of (x, y) indexed by the pair, or nullptr
    const int32_t* prev;                                           // pair i = (frame prev[i] -> frame i), < 0: none; nullptr: i - 1
    int max_pts; size_t out_row;                                   // records per output row
    vis_klt_point* out; vis_klt_pair* pair;
    float* p1; float* p2; int32_t* ntracked;                       // compacted rows (out_row x 2 floats) or nullptr
};

DEV long long wave_isum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
DEV int wave_isum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

DEV bool klt_fits(double x, double y, int r, int lw, int lh) {
    if (!(fabs(x) < INFINITY) || !(fabs(y) < INFINITY)) return false;
    const double fx = floor(x), fy = floor(y);
    return fx - (double)r >= 0.0 && fy - (double)r >= 0.0 && fx + (double)r + 1.0 <= (double)(lw - 1) && fy + (double)r + 1.0 <= (double)(lh - 1);
}

struct KltTaps { int X, Y, w00, w01, w10, w11; };
DEV KltTaps klt_taps(double x, double y) {
    KltTaps t;
    const double fx = floor(x), fy = floor(y);
    const double a = x - fx, b = y - fy;
    t.X = (int)fx; t.Y = (int)fy;
    t.w00 = (int)rint(((1.0 - a) * (1.0 - b)) * 16384.0);
    t.w01 = (int)rint((a * (1.0 - b)) * 16384.0);
    t.w10 = (int)rint(((1.0 - a) * b) * 16384.0);
    t.w11 = 16384 - t.w00 - t.w01 - t.w10;
    return t;
}
template <class T> DEV int klt_sample(const T* p, int rs, const KltTaps& t) {
    return t.w00 * (int)p[0] + t.w01 * (int)p[1] + t.w10 * (int)p[rs] + t.w11 * (int)p[rs + 1];
}

// the pair of frame i: its previous frame, or < 0
DEV int klt_prev(const KltArgs& G, int i) { return G.prev ? G.prev[i] : i - 1; }

template <int PPL>
__global__ __launch_bounds__(KLT_WAVES * 64) void k_klt(KltArgs G) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * KLT_WAVES + (threadIdx.x >> 6);     // the point of this wave
    const int i = blockIdx.y;                                      // the pair = its second frame
    if (k >= G.max_pts) return;
    vis_klt_point* rec = G.out + (size_t)i * G.out_row + k;
    const int f1 = klt_prev(G, i);
    if (f1 < 0) {                                                  // no pair: the whole row is zeroed
        if (lane < 8) reinterpret_cast<int32_t*>(rec)[lane] = 0;
        return;
    }
    const int q = G.rows_by_prev ? f1 : i;
    const int m = min(max(G.npts[q], 0), G.max_pts);
    if (k >= m) return;
    const float* pp = G.pts + (size_t)q * G.pts_row + (size_t)k * G.pt_stride;
    const float xin = pp[0], yin = pp[1];
    const int r = G.r, W = 2 * r + 1, n = W * W;
    // this lane's pixels of the window: offsets (ox, oy) in [-r, r]; a slot beyond n reads the centre and counts nothing
    int ox[PPL], oy[PPL]; bool live[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int p = lane + 64 * j;
        live[j] = p < n;
        ox[j] = live[j] ? p % W - r : 0;
        oy[j] = live[j] ? p / W - r : 0;
    }
    float rx = xin, ry = yin, fb = 0.f, lam_out = 0.f;
    int sad_out = 0, flags = 0, iters_out = 0, levels_out = 0;
    const double p0x = (double)xin, p0y = (double)yin;
    if (!(fabs(p0x) < INFINITY) || !(fabs(p0y) < INFINITY)) { flags = VIS_KLT_INVALID; rx = ry = 0.f; }
    else {
        double sx = p0x, sy = p0y;                                 // the start of the pass
        bool have_g = false; double gx0 = 0.0, gy0 = 0.0;
        if (G.guess) {
            const float* gp = G.guess + (size_t)i * G.guess_row + (size_t)k * 2;
            gx0 = (double)gp[0]; gy0 = (double)gp[1];
            have_g = fabs(gx0) < INFINITY && fabs(gy0) < INFINITY;
        }
        int fT = f1, fJ = i;
        const double s = (double)G.s;
        for (int dir = 0; dir < 2; dir++) {                        // 0: forward, 1: backward (frames swapped)
            double dx = 0.0, dy = 0.0;
            if (have_g) { const double sc = (double)(1 << G.first); dx = (gx0 - sx) / sc; dy = (gy0 - sy) / sc; }
            int lost = 0, iters = 0, levels = 0, sad = 0;
            double lam_last = 0.0; bool have_lam = false;
            int T[PPL], Dx[PPL], Dy[PPL];
#pragma unroll
            for (int j = 0; j < PPL; j++) { T[j] = 0; Dx[j] = 0; Dy[j] = 0; }
            for (int l = G.first; l >= G.last && !lost; l--) {
                const bool at_last = l == G.last;
                if (l < G.first) { dx = 2.0 * dx; dy = 2.0 * dy; }
                const KltLevel& V = G.lv[l];
                const double sc = (double)(1 << l);
                const double px = (sx + 0.5) / sc - 0.5, py = (sy + 0.5) / sc - 0.5;
                if (!klt_fits(px, py, r, V.lw, V.lh)) { if (at_last) lost = VIS_KLT_OOB; continue; }
                {   // (b) the template of this level
                    const KltTaps t = klt_taps(px, py);
                    const uint8_t* im = V.img + (size_t)fT * V.img_fstride;
                    const int16_t* gx = V.gx + (size_t)fT * V.grad_fstride;
                    const int16_t* gy = V.gy + (size_t)fT * V.grad_fstride;
                    long long gxx = 0, gxy = 0, gyy = 0;
#pragma unroll
                    for (int j = 0; j < PPL; j++) {
                        const size_t oi = (size_t)(t.Y + oy[j]) * V.rowstride + (t.X + ox[j]);
                        const size_t og = (size_t)(t.Y + oy[j]) * V.lw + (t.X + ox[j]);
                        const int tv = (klt_sample(im + oi, V.rowstride, t) + 256) >> 9;
                        const int dxv = (klt_sample(gx + og, V.lw, t) + 8192) >> 14;
                        const int dyv = (klt_sample(gy + og, V.lw, t) + 8192) >> 14;
                        T[j] = tv; Dx[j] = live[j] ? dxv : 0; Dy[j] = live[j] ? dyv : 0;
                        gxx += (long long)Dx[j] * Dx[j]; gxy += (long long)Dx[j] * Dy[j]; gyy += (long long)Dy[j] * Dy[j];
                    }
                    gxx = wave_isum(gxx); gxy = wave_isum(gxy); gyy = wave_isum(gyy);
                    const double fxx = (double)gxx, fxy = (double)gxy, fyy = (double)gyy;
                    const double det = fxx * fyy - fxy * fxy;
                    const double lam = ((fxx + fyy) - sqrt((fxx - fyy) * (fxx - fyy) + 4.0 * (fxy * fxy))) / G.lam_den;
                    if (at_last) { lam_last = lam; have_lam = true; }
                    if (!(det > 0.0 && lam >= G.min_eig)) { if (at_last) lost = VIS_KLT_FLAT; continue; }
                    levels |= 1 << l;
                    // (c) the steps
                    const uint8_t* jm = V.img + (size_t)fJ * V.img_fstride;
                    for (int it = 0; it < G.max_it; it++) {
                        const double qx = px + dx, qy = py + dy;
                        if (!klt_fits(qx, qy, r, V.lw, V.lh)) { if (at_last) lost = VIS_KLT_OOB; break; }
                        const KltTaps u = klt_taps(qx, qy);
                        long long bx = 0, by = 0;
#pragma unroll
                        for (int j = 0; j < PPL; j++) {
                            const size_t oi = (size_t)(u.Y + oy[j]) * V.rowstride + (u.X + ox[j]);
                            const int e = ((klt_sample(jm + oi, V.rowstride, u) + 256) >> 9) - T[j];
                            bx += (long long)Dx[j] * e; by += (long long)Dy[j] * e;
                        }
                        bx = wave_isum(bx); by = wave_isum(by);
                        const double fbx = (double)bx, fby = (double)by;
                        const double ux = -(s * (fyy * fbx - fxy * fby)) / det;
                        const double uy = -(s * (fxx * fby - fxy * fbx)) / det;
                        dx = dx + ux; dy = dy + uy;
                        iters++;
                        if (ux * ux + uy * uy <= G.eps2) break;
                    }
                }
                if (at_last && !lost) {                            // the residual at the final position (T is last_level's)
                    const double qx = px + dx, qy = py + dy;
                    if (!klt_fits(qx, qy, r, V.lw, V.lh)) lost = VIS_KLT_OOB;
                    else {
                        const KltTaps u = klt_taps(qx, qy);
                        const uint8_t* jm = V.img + (size_t)fJ * V.img_fstride;
                        int a = 0;
#pragma unroll
                        for (int j = 0; j < PPL; j++) {
                            const size_t oi = (size_t)(u.Y + oy[j]) * V.rowstride + (u.X + ox[j]);
                            const int e = ((klt_sample(jm + oi, V.rowstride, u) + 256) >> 9) - T[j];
                            a += live[j] ? abs(e) : 0;
                        }
                        sad = wave_isum(a);
                    }
                }
            }
            const double sl = (double)(1 << G.last);
            const double ex = sx + dx * sl, ey = sy + dy * sl;     // where the pass ended
            if (dir == 0) {
                flags = lost; iters_out = iters; levels_out = levels;
                if (have_lam) lam_out = (float)lam_last;
                if (!lost) {
                    rx = (float)ex; ry = (float)ey; sad_out = sad;
                    if (G.err_bound > 0.0 && (double)sad > G.err_bound) flags |= VIS_KLT_ERR;
                }
                if (flags || !(G.fb2 > 0.0)) break;
                gx0 = p0x; gy0 = p0y; have_g = true;               // backward: from the float result, with p0 as the guess
                sx = (double)rx; sy = (double)ry;
                fT = i; fJ = f1;
            } else {
                if (lost) { fb = -1.f; flags |= VIS_KLT_FB; }
                else {
                    const double ddx = ex - p0x, ddy = ey - p0y;
                    const double d2 = ddx * ddx + ddy * ddy;
                    fb = (float)sqrt(d2);
                    if (d2 > G.fb2) flags |= VIS_KLT_FB;
                }
            }
        }
        if (!flags) flags = VIS_KLT_TRACKED;
    }
    if (lane == 0) {
        vis_klt_point o;
        o.x = rx; o.y = ry; o.fb = fb; o.min_eig = lam_out; o.sad = sad_out; o.flags = flags;
        o.iters = (uint16_t)iters_out; o.levels = (uint8_t)levels_out;
        for (int j = 0; j < 5; j++) o.pad_[j] = 0;
        *rec = o;
    }
}

// one wave per pair: the counts of the pair record and the tracked points in rising index
__global__ __launch_bounds__(64) void k_klt_pairs(KltArgs G) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int f1 = klt_prev(G, i);
    vis_klt_pair pr = {};
    int nt = 0;
    if (f1 < 0) pr.flags = VIS_KLT_NO_PAIR;
    else {
        const int q = G.rows_by_prev ? f1 : i;
        const int m = min(max(G.npts[q], 0), G.max_pts);
        pr.n_points = m;
        for (int k0 = 0; k0 < m; k0 += 64) {
            const int k = k0 + lane;
            const vis_klt_point* rec = G.out + (size_t)i * G.out_row + k;
            const int fl = k < m ? rec->flags : 0;
            const unsigned long long bt = __ballot(fl & VIS_KLT_TRACKED);
            pr.n_oob += __popcll(__ballot(fl & VIS_KLT_OOB)); pr.n_flat += __popcll(__ballot(fl & VIS_KLT_FLAT));
            pr.n_err += __popcll(__ballot(fl & VIS_KLT_ERR)); pr.n_fb += __popcll(__ballot(fl & VIS_KLT_FB));
            pr.n_invalid += __popcll(__ballot(fl & VIS_KLT_INVALID));
            if (G.p1 && (fl & VIS_KLT_TRACKED)) {
                const int at = nt + __popcll(bt & ((1ull << lane) - 1ull));
                const float* pp = G.pts + (size_t)q * G.pts_row + (size_t)k * G.pt_stride;
                float* a = G.p1 + ((size_t)i * G.out_row + at) * 2; float* b = G.p2 + ((size_t)i * G.out_row + at) * 2;
                a[0] = pp[0]; a[1] = pp[1]; b[0] = rec->x; b[1] = rec->y;
            }
            nt += __popcll(bt);
        }
        pr.n_tracked = nt;
    }
    if (lane == 0) { G.pair[i] = pr; if (G.ntracked) G.ntracked[i] = nt; }
}

// ---------------------------------------------------------------------------------------------------------------- host side
extern "C" void vis_default_klt_params(vis_klt_params* kp) {
    if (!kp) return;
    std::memset(kp, 0, sizeof(*kp));
    kp->win_radius = 7; kp->first_level = 3; kp->last_level = 0; kp->max_iters = 10;
    kp->epsilon = 0.01; kp->min_eig = 0.1; kp->max_err = 0.0; kp->fb_max_px = 0.0; kp->scharr_scale = 3;
}

static bool klt_params_ok(const vis_klt_params* kp) {
    auto nonneg = [](double v) { return std::isfinite(v) && v >= 0.0; };
    return kp && kp->win_radius >= 2 && kp->win_radius <= 10 && kp->last_level >= 0 && kp->last_level <= kp->first_level && kp->first_level <= 4 &&
           kp->max_iters >= 1 && kp->max_iters <= 30 && nonneg(kp->epsilon) && nonneg(kp->min_eig) && nonneg(kp->max_err) && nonneg(kp->fb_max_px) &&
           kp->scharr_scale >= 1 && kp->scharr_scale <= 8 && kp->reserved_ == 0;
}
static bool klt_dims_ok(int w, int h, int stride) { return w >= 16 && h >= 16 && w <= VIS_MAX_SIDE && h <= VIS_MAX_SIDE && stride >= w; }

static void klt_fill_params(const vis_klt_params& kp, KltArgs& G) {
    const double n = (double)((2 * kp.win_radius + 1) * (2 * kp.win_radius + 1)), s = (double)kp.scharr_scale;
    G.r = kp.win_radius; G.first = kp.first_level; G.last = kp.last_level; G.max_it = kp.max_iters; G.s = kp.scharr_scale;
    G.eps2 = kp.epsilon * kp.epsilon; G.min_eig = kp.min_eig;
    G.err_bound = kp.max_err > 0.0 ? (kp.max_err * 32.0) * n : 0.0;
    G.fb2 = kp.fb_max_px > 0.0 ? kp.fb_max_px * kp.fb_max_px : 0.0;
    G.lam_den = ((2.0 * n) * (32.0 * s)) * (32.0 * s);
}

// the levels of a batch laid out like vis_gradient_batch's outputs; level 0 of the intensities is the frames themselves
static void klt_fill_levels(KltArgs& G, const uint8_t* d_frames, int w, int h, int stride, size_t frame_stride,
                            const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy) {
    const size_t fe = vis_grad_frame_elems(w, h);
    int lw[5], lh[5]; vis_half_dims(w, h, lw, lh);
    size_t off = 0;
    for (int l = 0; l < 5; l++) {
        KltLevel& V = G.lv[l];
        V.lw = lw[l]; V.lh = lh[l];
        if (l == 0) { V.img = d_frames; V.rowstride = stride; V.img_fstride = frame_stride; }
        else { V.img = d_gray + off; V.rowstride = lw[l]; V.img_fstride = fe; }
        V.gx = d_gx + off; V.gy = d_gy + off; V.grad_fstride = fe;
        off += (size_t)lw[l] * lh[l];
    }
}

// k_klt + k_klt_pairs over the n rows of G on ctx->stream
static int klt_run(vis_ctx* ctx, const KltArgs& G, int n) {
    if (n < 1) return VIS_OK;
    if (G.max_pts > 0) {
        const dim3 grid((unsigned)((G.max_pts + KLT_WAVES - 1) / KLT_WAVES), (unsigned)n);
        if (G.r <= 7) hipLaunchKernelGGL((k_klt<4>), grid, dim3(KLT_WAVES * 64), 0, ctx->stream, G);
        else hipLaunchKernelGGL((k_klt<7>), grid, dim3(KLT_WAVES * 64), 0, ctx->stream, G);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_klt_pairs, dim3((unsigned)n), dim3(64), 0, ctx->stream, G);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

extern "C" int vis_klt_track(vis_ctx* ctx, const vis_klt_params* kp, int w, int h,
                             const uint8_t* const gray1[5], const int16_t* const gx1[5], const int16_t* const gy1[5],
                             const uint8_t* const gray2[5], const int16_t* const gx2[5], const int16_t* const gy2[5],
                             const float* pts, const float* guess, int m, vis_klt_point* out, vis_klt_pair* pair) {
    if (!pair || m < 0 || (m && (!pts || !out)) || !gray1 || !gx1 || !gy1 || !gray2 || !klt_params_ok(kp) || !klt_dims_ok(w, h, w)) return VIS_E_INVALID;
    const bool fb = kp->fb_max_px > 0.0;
    if (fb && (!gx2 || !gy2)) return VIS_E_INVALID;
    for (int l = kp->last_level; l <= kp->first_level; l++)
        if (!gray1[l] || !gx1[l] || !gy1[l] || !gray2[l] || (fb && (!gx2[l] || !gy2[l]))) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    std::memset(pair, 0, sizeof(*pair));
    if (m == 0) return VIS_OK;
    (void)hipSetDevice(ctx->device);
    // the two frames as a batch of two in the layout of a gradient set, level 0 of the intensities dense in its place
    const size_t fe = vis_grad_frame_elems(w, h);
    int lw[5], lh[5]; vis_half_dims(w, h, lw, lh);
    uint8_t* d_gray; int16_t *d_gx, *d_gy; float *d_pts, *d_guess = nullptr; int32_t* d_n; vis_klt_point* d_out; vis_klt_pair* d_pair;
    int rc = vis_carve(ctx, [&](Carver& cv) {
        d_gray = cv.take<uint8_t>(2 * fe); d_gx = cv.take<int16_t>(2 * fe); d_gy = cv.take<int16_t>(2 * fe);
        d_pts = cv.take<float>((size_t)m * 4);                     // rows 0 (unused) and 1
        if (guess) d_guess = cv.take<float>((size_t)m * 4);
        d_n = cv.take<int32_t>(2);
        d_out = cv.take<vis_klt_point>((size_t)m * 2); d_pair = cv.take<vis_klt_pair>(2);
    }, 2);
    if (rc) return rc;
    HostStage hs(ctx);
    size_t off = 0;
    for (int l = 0; l < 5; l++) {
        const size_t px = (size_t)lw[l] * lh[l];
        if (l >= kp->last_level && l <= kp->first_level) {
            hs.up(d_gray + off, gray1[l], px); hs.up(d_gray + fe + off, gray2[l], px);
            hs.up(d_gx + off, gx1[l], px * 2); hs.up(d_gy + off, gy1[l], px * 2);
            if (fb) { hs.up(d_gx + fe + off, gx2[l], px * 2); hs.up(d_gy + fe + off, gy2[l], px * 2); }
        }
        off += px;
    }
    const int32_t cnt[2] = {0, m};
    hs.up(d_pts + (size_t)m * 2, pts, (size_t)m * 8);
    if (guess) hs.up(d_guess + (size_t)m * 2, guess, (size_t)m * 8);
    hs.up(d_n, cnt, sizeof(cnt));
    hs.flush_ups();
    KltArgs G; std::memset(&G, 0, sizeof(G));
    klt_fill_params(*kp, G);
    klt_fill_levels(G, d_gray, w, h, w, fe, d_gray, d_gx, d_gy);
    G.pts = d_pts; G.pt_stride = 2; G.pts_row = (size_t)m * 2; G.npts = d_n; G.rows_by_prev = 0;
    G.guess = d_guess; G.guess_row = (size_t)m * 2; G.prev = nullptr;
    G.max_pts = m; G.out_row = (size_t)m; G.out = d_out; G.pair = d_pair;
    rc = klt_run(ctx, G, 2);
    if (rc) return vis_drain(ctx, rc);
    const void* h_out = hs.down(d_out + m, (size_t)m * sizeof(vis_klt_point));
    const void* h_pair = hs.down(d_pair + 1, sizeof(vis_klt_pair));
    rc = hs.wait();
    if (rc) return rc;
    std::memcpy(out, h_out, (size_t)m * sizeof(vis_klt_point));
    std::memcpy(pair, h_pair, sizeof(vis_klt_pair));
    return VIS_OK;
}

extern "C" int vis_klt_batch(vis_ctx* ctx, const vis_klt_params* kp, const uint8_t* d_frames, int w, int h, int stride, int n,
                             const uint8_t* d_gray, const int16_t* d_gx, const int16_t* d_gy,
                             const float* d_pts, const int32_t* d_npts, int max_pts, const float* d_guess,
                             vis_klt_point* d_out, vis_klt_pair* d_pair, float* d_p1, float* d_p2, int32_t* d_ntracked) {
    if (!d_frames || !d_gray || !d_gx || !d_gy || !d_npts || !d_pair || n < 0 || max_pts < 0 || (max_pts && (!d_pts || !d_out))) return VIS_E_INVALID;
    if ((d_p1 || d_p2 || d_ntracked) && !(d_p1 && d_p2 && d_ntracked)) return VIS_E_INVALID;
    if (!klt_params_ok(kp) || !klt_dims_ok(w, h, stride)) return VIS_E_INVALID;
    if (((uintptr_t)d_out & 7) || ((uintptr_t)d_pair & 7) || ((uintptr_t)d_pts & 3) || ((uintptr_t)d_guess & 3) || ((uintptr_t)d_npts & 3) ||
        ((uintptr_t)d_p1 & 3) || ((uintptr_t)d_p2 & 3) || ((uintptr_t)d_ntracked & 3) || ((uintptr_t)d_gx & 1) || ((uintptr_t)d_gy & 1)) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    KltArgs G; std::memset(&G, 0, sizeof(G));
    klt_fill_params(*kp, G);
    klt_fill_levels(G, d_frames, w, h, stride, (size_t)stride * h, d_gray, d_gx, d_gy);
    G.pts = d_pts; G.pt_stride = 2; G.pts_row = (size_t)max_pts * 2; G.npts = d_npts; G.rows_by_prev = 0;
    G.guess = d_guess; G.guess_row = (size_t)max_pts * 2; G.prev = nullptr;
    G.max_pts = max_pts; G.out_row = (size_t)max_pts; G.out = d_out; G.pair = d_pair;
    G.p1 = d_p1; G.p2 = d_p2; G.ntracked = d_ntracked;
    return klt_run(ctx, G, n);
}

extern "C" int vis_batch_klt(vis_ctx* ctx, const vis_klt_params* kp, const uint8_t* d_frames, int n, const float* d_guess, int row_cap,
                             vis_klt_point* d_out, vis_klt_pair* d_pair, float* d_p1, float* d_p2, int32_t* d_ntracked) {
    if (!d_frames || !d_out || !d_pair || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if ((d_p1 || d_p2 || d_ntracked) && !(d_p1 && d_p2 && d_ntracked)) return VIS_E_INVALID;
    if (!klt_params_ok(kp) || kp->scharr_scale != 3) return VIS_E_INVALID;
    if (((uintptr_t)d_out & 7) || ((uintptr_t)d_pair & 7) || ((uintptr_t)d_guess & 3) || ((uintptr_t)d_p1 & 3) || ((uintptr_t)d_p2 & 3) ||
        ((uintptr_t)d_ntracked & 3)) return VIS_E_INVALID;
    if (!ctx || !ctx->batch) return VIS_E_STATE;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & VIS_STAGE_DETECT) || !pl->grad_valid) { ctx->err = "vis_batch_klt: the last vis_batch_run had no VIS_STAGE_DETECT | VIS_STAGE_GRADIENT"; return VIS_E_STATE; }
    if (row_cap < pl->kcap) { ctx->err = "vis_batch_klt: row_cap is smaller than the plan's keypoint capacity"; return VIS_E_CAPACITY; }
    // On the pose stream like vis_batch_align (align.hip batch_align_stream): behind everything queued on the context's stream so far -- the
    // detect chain that wrote the keypoints and the links, joined by the side stream that wrote the gradients.  What may not overtake it
    // waits for the reader events noted below.
    Plan::RecordSet& rs = pl->last_set();
    Plan::GradSet& GS = pl->grad[pl->grad_set];
    KltArgs G; std::memset(&G, 0, sizeof(G));
    klt_fill_params(*kp, G);
    klt_fill_levels(G, d_frames, pl->w, pl->h, pl->stride, (size_t)pl->stride * pl->h, GS.half, GS.gx, GS.gy);
    static_assert(sizeof(vis_keypoint) == 28 && offsetof(vis_keypoint, x) == 0 && offsetof(vis_keypoint, y) == 4, "a keypoint record begins with (x, y)");
    // frame f of the launch is record last_base + 1 + f; gate off: pair i = (i - 1 -> i), pair 0 (the carried frame) has no pair here
    G.pts = reinterpret_cast<const float*>(pl->d_kps + (size_t)(pl->last_base + 1) * pl->kcap); G.pt_stride = 7; G.pts_row = (size_t)pl->kcap * 7;
    G.npts = pl->d_nkp + pl->last_base + 1; G.rows_by_prev = 1;
    G.guess = d_guess; G.guess_row = (size_t)row_cap * 2;
    const int32_t* links = pl->kf_min ? rs.kf_link : nullptr;
    G.prev = links;
    G.max_pts = pl->kcap; G.out_row = (size_t)row_cap; G.out = d_out; G.pair = d_pair;
    G.p1 = d_p1; G.p2 = d_p2; G.ntracked = d_ntracked;
    // the reader event: the alignments' ring, so that every writer that waits for an alignment waits for this call too.  The gradient set
    // two steps on is refilled behind it, and so is the record set (launch_detect waits for the matcher guard)
    return on_pose_stream(ctx, {FU_FORK, nullptr, d_frames, d_frames + (size_t)pl->stride * pl->h * n}, [&] { return klt_run(ctx, G, n); },
                          {&GS.readers, &rs.matcher, links ? &rs.links : nullptr});
}
