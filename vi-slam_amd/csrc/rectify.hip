// rectify.hip -- vi::CameraModel's rectification on the device: the tables of cv::initUndistortRectifyMap (geometry.cpp, built once on the
// host) and cv::remap(INTER_LINEAR, BORDER_CONSTANT, 0) over a batch of frames (src/CameraModel.cpp:84-105, src/VISystem.cpp:162-205).
//
// remap of 8U with CV_16SC2 + CV_16UC1 tables (OpenCV 3.2 imgproc/imgwarp.cpp remapBilinear, restated from the published algorithm:
// PARITY UNPINNED).  Output pixel: source cell (sx, sy) = map1, a = map2 & 1023, i = a >> 5 (y fraction), j = a & 31 (x fraction); the
// 2-D table of initInterTab2D holds the exact weights 32 (32 - i)(32 - j), 32 (32 - i) j, 32 i (32 - j), 32 i j (sum 32768: its fix-up
// loop never runs), D = (sum S w + 16384) >> 15.  Every weight is a multiple of 32, so this is (sum S w' + 512) >> 10 with the 10-bit
// weights w' = (32 - i)(32 - j) ... -- what the kernel computes.  Border: the inlier branch ((unsigned)sx < in_w - 1, (unsigned)sy <
// in_h - 1: all four taps inside), the all-outside branch (sx >= in_w || sx + 1 < 0 || sy >= in_h || sy + 1 < 0: the border value 0)
// and the per-tap branch (a tap outside reads 0) are one rule: a tap contributes when it lies inside the source.
//
// Shape: one thread = 4 adjacent output pixels of one row (one dword store).  It reads their table entries once and applies them to
// RF_F frames of the batch, so the 6-byte table costs 6 / RF_F bytes per output pixel.  A tap outside the source gets weight 0 and the
// offset 0 of its frame (an address that exists), so the frame loop is 16 loads and 16 multiply-adds with no branch.  With 8 or more
// frame groups all workgroups of one group land on one XCD (blockIdx % 8, as detect.hip's xcd_frame_map): the group's RF_F source frames
// (8 x 361 KB at 752 x 480) stay in that XCD's 4 MiB L2 while its workgroups gather from them.  With fewer (n <= 56: vis_rectify_host,
// small batches) the workgroups of a group are dealt over all XCDs instead, so that every XCD has work.
#include "vis_internal.h"

#define RF_THREADS 256
#define RF_F 8

struct vis_rectify {
    vis_ctx* ctx = nullptr;
    int in_w = 0, in_h = 0, out_w = 0, out_h = 0;
    uint32_t* d_map1 = nullptr;              // out_h x out_w: the CV_16SC2 entry (x, y int16) as one little-endian word
    uint16_t* d_map2 = nullptr;              // out_h x out_w: the CV_16UC1 entry
    hipEvent_t ev_last = nullptr;            // behind the last launch that read the tables (vis_rectify_destroy waits for it)
};

template <bool DW>
__global__ __launch_bounds__(RF_THREADS) void k_remap(const uint8_t* __restrict__ in, int in_w, int in_h, int in_stride, size_t in_fstride,
                                                      const uint32_t* __restrict__ map1, const uint16_t* __restrict__ map2, int tab_w,
                                                      int x0, int y0, int w, int h, int qw, int tiles, int n, int xcd_groups,
                                                      uint8_t* __restrict__ out, int out_stride, size_t out_fstride) {
    const int b = blockIdx.x;
    int group, tile;
    if (xcd_groups) { const int j = b >> 3, jt = j / tiles; group = jt * 8 + (b & 7); tile = j - jt * tiles; }
    else { group = b / tiles; tile = b - group * tiles; }
    const int f0 = group * RF_F;
    if (f0 >= n) return;
    const int q = tile * RF_THREADS + (int)threadIdx.x;
    if (q >= qw * h) return;
    const int y = q / qw, x = (q - y * qw) * 4;
    int off[4][4], wt[4][4];
    const size_t t0 = (size_t)(y0 + y) * tab_w + (size_t)(x0 + x);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int sx = 0, sy = 0, a = 0;
        const bool px = x + k < w;
        if (px) {
            const uint32_t m = map1[t0 + k];
            sx = (int)(int16_t)(m & 0xFFFFu); sy = (int)(int16_t)(m >> 16);
            a = map2[t0 + k] & 1023;
        }
        const int fi = a >> 5, fj = a & 31;
        const int wy[2] = {32 - fi, fi}, wx[2] = {32 - fj, fj};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int tx = sx + (t & 1), ty = sy + (t >> 1);
            const bool inside = px && (unsigned)tx < (unsigned)in_w && (unsigned)ty < (unsigned)in_h;
            off[k][t] = inside ? ty * in_stride + tx : 0;
            wt[k][t] = inside ? wy[t >> 1] * wx[t & 1] : 0;
        }
    }
    const int fend = min(n, f0 + RF_F);
    for (int f = f0; f < fend; f++) {
        const uint8_t* S = in + (size_t)f * in_fstride;
        uint8_t* D = out + (size_t)f * out_fstride + (size_t)y * out_stride + x;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = S[off[k][0]] * wt[k][0] + S[off[k][1]] * wt[k][1] + S[off[k][2]] * wt[k][2] + S[off[k][3]] * wt[k][3];
            v[k] = (uint32_t)((s + 512) >> 10);
        }
        if (DW && x + 3 < w) {
            *(uint32_t*)D = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (x + k < w) D[k] = (uint8_t)v[k];
        }
    }
}

static int launch_remap(vis_rectify* r, hipStream_t st, const uint8_t* d_in, int in_stride, int n, int x0, int y0, int w, int h,
                        uint8_t* d_out, int out_stride) {
    vis_ctx* ctx = r->ctx;
    const int qw = (w + 3) / 4;
    const long long tiles = ((long long)qw * h + RF_THREADS - 1) / RF_THREADS;
    const long long groups = (n + RF_F - 1) / RF_F;
    const int xcd_groups = groups >= 8;
    const long long blocks = xcd_groups ? 8 * ((groups + 7) / 8) * tiles : groups * tiles;
    if (blocks > 0x7FFFFFFFLL) { ctx->err = "vis_rectify_batch: too many frames for one launch"; return VIS_E_INVALID; }
    const size_t in_fs = (size_t)in_stride * r->in_h, out_fs = (size_t)out_stride * h;
    const bool dw = !((uintptr_t)d_out & 3) && !(out_stride & 3);
    if (dw) hipLaunchKernelGGL(k_remap<true>, dim3((unsigned)blocks), dim3(RF_THREADS), 0, st, d_in, r->in_w, r->in_h, in_stride, in_fs,
                               r->d_map1, r->d_map2, r->out_w, x0, y0, w, h, qw, (int)tiles, n, xcd_groups, d_out, out_stride, out_fs);
    else hipLaunchKernelGGL(k_remap<false>, dim3((unsigned)blocks), dim3(RF_THREADS), 0, st, d_in, r->in_w, r->in_h, in_stride, in_fs,
                            r->d_map1, r->d_map2, r->out_w, x0, y0, w, h, qw, (int)tiles, n, xcd_groups, d_out, out_stride, out_fs);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(r->ev_last, st));
    return VIS_OK;
}

extern "C" int vis_rectify_create(vis_ctx* ctx, const float K[4], const float dist[4], const float Knew[4], int in_w, int in_h,
                                  int out_w, int out_h, vis_rectify** out) {
    if (vis_device_count() <= 0) return VIS_E_NODEVICE;
    if (!ctx || !out) return VIS_E_INVALID;
    *out = nullptr;
    if (in_w < 1 || in_h < 1 || in_w > 4095 || in_h > 4095) { ctx->err = "vis_rectify_create: input size outside 1 ... 4095"; return VIS_E_INVALID; }
    const size_t npx = (size_t)(out_w > 0 ? out_w : 0) * (size_t)(out_h > 0 ? out_h : 0);
    std::vector<int16_t> m1(2 * std::max(npx, (size_t)1));
    std::vector<uint16_t> m2(std::max(npx, (size_t)1));
    int rc = vis_undistort_rectify_map(K, dist, Knew, out_w, out_h, m1.data(), m2.data());
    if (rc) { ctx->err = "vis_rectify_create: invalid calibration or output size"; return rc; }
    (void)hipSetDevice(ctx->device);
    vis_rectify* r = new (std::nothrow) vis_rectify();
    if (!r) return VIS_E_NOMEM;
    r->ctx = ctx; r->in_w = in_w; r->in_h = in_h; r->out_w = out_w; r->out_h = out_h;
    if (hipMalloc(&r->d_map1, npx * 4) != hipSuccess || hipMalloc(&r->d_map2, npx * 2) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev_last, hipEventDisableTiming) != hipSuccess ||
        hipMemcpy(r->d_map1, m1.data(), npx * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(r->d_map2, m2.data(), npx * 2, hipMemcpyHostToDevice) != hipSuccess) {
        ctx->err = std::string("vis_rectify_create: ") + hipGetErrorString(hipGetLastError());
        vis_rectify_destroy(r);
        return VIS_E_HIP;
    }
    *out = r;
    return VIS_OK;
}

extern "C" void vis_rectify_destroy(vis_rectify* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    if (r->ev_last) { (void)hipEventSynchronize(r->ev_last); (void)hipEventDestroy(r->ev_last); }
    if (r->d_map1) (void)hipFree(r->d_map1);
    if (r->d_map2) (void)hipFree(r->d_map2);
    delete r;
}

extern "C" int vis_rectify_maps(vis_rectify* r, int16_t* map1, uint16_t* map2) {
    if (!r) return VIS_E_INVALID;
    vis_ctx* ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t npx = (size_t)r->out_w * r->out_h;
    if (map1) HIPCHK(ctx, hipMemcpy(map1, r->d_map1, npx * 4, hipMemcpyDeviceToHost));
    if (map2) HIPCHK(ctx, hipMemcpy(map2, r->d_map2, npx * 2, hipMemcpyDeviceToHost));
    return VIS_OK;
}

extern "C" int vis_rectify_batch(vis_rectify* r, const uint8_t* d_in, int in_stride, int n, int x0, int y0, int w, int h,
                                 uint8_t* d_out, int out_stride) {
    if (!r) return VIS_E_INVALID;
    vis_ctx* ctx = r->ctx;
    if (!d_in || !d_out || n < 1 || in_stride < r->in_w || (size_t)in_stride * r->in_h > 0x7FFFFFFFu) {
        ctx->err = "vis_rectify_batch: NULL frames, n < 1, or in_stride < in_w (or in_stride * in_h >= 2^31)"; return VIS_E_INVALID;
    }
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 > r->out_w - w || y0 > r->out_h - h || out_stride < w) {
        ctx->err = "vis_rectify_batch: the window must lie inside the out_w x out_h output, out_stride >= w"; return VIS_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    // d_out is a caller frame buffer: a vis_batch_align / vis_batch_track still running on the pose stream may read it (the frames of an
    // earlier step).  Wait for the alignment that read this range (align_reader, vis_internal.h).
    HIPCHK(ctx, wait_align_readers(ctx, ctx->stream, d_out, d_out + (size_t)out_stride * h * n));
    return launch_remap(r, ctx->stream, d_in, in_stride, n, x0, y0, w, h, d_out, out_stride);
}

extern "C" int vis_rectify_host(vis_rectify* r, const uint8_t* img, int in_stride, uint8_t* out, int out_stride) {
    if (!r) return VIS_E_INVALID;
    vis_ctx* ctx = r->ctx;
    if (!img || !out || in_stride < r->in_w || out_stride < r->out_w) {
        ctx->err = "vis_rectify_host: NULL image, in_stride < in_w or out_stride < out_w"; return VIS_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    const size_t in_bytes = (size_t)r->in_w * r->in_h, out_bytes = (size_t)r->out_w * r->out_h;
    uint8_t *d_in, *d_out;
    int rc = vis_carve(ctx, [&](Carver& cv) { d_in = cv.take<uint8_t>(in_bytes); d_out = cv.take<uint8_t>(out_bytes); });
    if (rc) return rc;
    HostStage hs(ctx);
    hs.up2d(d_in, r->in_w, img, in_stride, r->in_w, r->in_h);
    hs.flush_ups();
    rc = launch_remap(r, ctx->stream, d_in, r->in_w, 1, 0, 0, r->out_w, r->out_h, d_out, r->out_w);
    if (rc) return vis_drain(ctx, rc);
    const uint8_t* got = (const uint8_t*)hs.down(d_out, out_bytes);
    rc = hs.wait();
    if (rc) return rc;
    for (int yy = 0; yy < r->out_h; yy++) std::memcpy(out + (size_t)yy * out_stride, got + (size_t)yy * r->out_w, r->out_w);
    return VIS_OK;
}
