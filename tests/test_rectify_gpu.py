"""GPU: rectification on the device (vis_rectify_*): k_remap against the numpy restatement of OpenCV 3.2's remap(INTER_LINEAR,
BORDER_CONSTANT 0) in tests/rectify_ref.py, byte for byte -- EuRoC tables on 1024 synthetic frames, noise, a saturated frame, a strong
lens, an odd size, padded strides, n not a multiple of the kernel's frame group; the ROI window; identity tables; the host form; the
downloaded tables; rectify -> vis_batch_run pipelined against synchronised against host-rectified frames; the error states; and the
vi::CameraModel adapter (GetMap1 / GetMap2 / Undistort / GetK)."""
import json
import os
import subprocess

import numpy as np
import pytest

import rectify_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xE0C00001
W, H = 752, 480
EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
ROI = (29, 54, 711, 426)                                  # CameraModel::RectifiedROI of the EuRoC calibration (x1, y1, x2, y2)
STRONG_K, STRONG_D, STRONG_KN = (400.0, 410.0, 320.0, 240.0), (0.9, 0.4, 0.01, -0.02), (2.0, 2.5, 320.0, 240.0)


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()                              # (torch's copy and the library's non-blocking streams are not ordered)
    return t


def _empty(nbytes):
    torch = _torch()
    t = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _euroc_kn(vislam):
    return vislam.optimal_new_camera_matrix(EUROC_K, EUROC_D, (W, H), (736, H))


def _ref(frame, K, D, Kn, out_w, out_h):
    m1, m2 = rectify_ref.undistort_rectify_map(K, D, Kn, out_w, out_h)
    return rectify_ref.remap(frame, m1, m2)


def _run(ctx, r, frames, in_stride=None, out_stride=None, window=None):
    """n host frames (n, in_h, in_w) -> device (padded to in_stride) -> batch -> host (n, h, w)"""
    n, ih, iw = frames.shape
    in_stride = in_stride or iw
    x0, y0, w, h = window or (0, 0) + r.out_size
    out_stride = out_stride or w
    buf = np.full((n, ih, in_stride), 0xA5, np.uint8)
    buf[:, :, :iw] = frames
    d_in, d_out = _dev(buf), _empty(n * h * out_stride)
    r.batch(d_in.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride, (x0, y0, w, h))
    out = _host(d_out).reshape(n, h, out_stride)
    assert (out[:, :, w:] == 0x5A).all()                   # nothing written beside the window
    return out[:, :, :w]


def test_euroc_1024_synthetic_frames(vislam, ctx, canvas):
    torch = _torch()
    n, Kn = 1024, _euroc_kn(vislam)
    d_canvas = _dev(canvas)
    d_in = torch.empty(n * H * W, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.synth_frames_device(d_canvas.data_ptr(), canvas.shape[0], SEED, 0, n, W, H, W, d_in.data_ptr())
    r = ctx.rectify(EUROC_K, EUROC_D, Kn, (W, H), (736, H))
    try:
        d_out = _empty(n * H * 736)
        r.batch(d_in.data_ptr(), W, n, d_out.data_ptr(), 736)
        out = _host(d_out).reshape(n, H, 736)
        m1, m2 = rectify_ref.undistort_rectify_map(EUROC_K, EUROC_D, Kn, 736, H)
        for t in (0, 1, 7, 8, 511, 512, 1022, 1023):
            want = rectify_ref.remap(vislam.synth_frame(canvas, t, W, H, SEED), m1, m2)
            assert out[t].tobytes() == want.tobytes(), t
    finally:
        r.close()


@pytest.mark.parametrize("case", ["noise", "saturated", "strong", "odd"])
def test_against_the_numpy_remap(vislam, ctx, case):
    rng = np.random.default_rng(7)
    if case == "strong":
        K, D, Kn, (iw, ih), (ow, oh) = STRONG_K, STRONG_D, STRONG_KN, (640, 480), (640, 480)
    elif case == "odd":
        K, D, (iw, ih), (ow, oh) = EUROC_K, EUROC_D, (333, 217), (301, 199)
        Kn = vislam.optimal_new_camera_matrix(K, D, (iw, ih), (ow, oh))
    else:
        K, D, (iw, ih), (ow, oh) = EUROC_K, EUROC_D, (W, H), (736, H)
        Kn = _euroc_kn(vislam)
    n = 13                                                # not a multiple of the kernel's frame group (8)
    frames = rng.integers(0, 256, (n, ih, iw), dtype=np.uint8)
    if case == "saturated":
        frames[:] = 255
    r = ctx.rectify(K, D, Kn, (iw, ih), (ow, oh))
    try:
        for in_stride, out_stride in ((None, None), (iw + 13, ow + 7), (iw + 64, ow + 64)):
            got = _run(ctx, r, frames, in_stride, out_stride)
            for i in range(n):
                assert got[i].tobytes() == _ref(frames[i], K, D, Kn, ow, oh).tobytes(), (case, in_stride, i)
    finally:
        r.close()
    if case == "saturated":
        assert (got[0][ROI[1]:ROI[3], ROI[0]:ROI[2]] == 255).all()


def test_roi_window_is_the_full_image_sliced(vislam, ctx):
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (9, H, W), dtype=np.uint8)
    r = ctx.rectify(EUROC_K, EUROC_D, _euroc_kn(vislam), (W, H), (736, H))
    try:
        full = _run(ctx, r, frames)
        x1, y1, x2, y2 = ROI
        for window, stride in (((x1, y1, x2 - x1, y2 - y1), 704), ((x1, y1, x2 - x1, y2 - y1), 683), ((1, 2, 5, 3), 5), ((735, 479, 1, 1), 4)):
            x0, y0, w, h = window
            got = _run(ctx, r, frames, None, stride, window)
            assert got.tobytes() == np.ascontiguousarray(full[:, y0:y0 + h, x0:x0 + w]).tobytes(), window
    finally:
        r.close()


def test_identity_tables_reproduce_the_input(vislam, ctx):
    rng = np.random.default_rng(5)
    for (w, h) in ((W, H), (211, 163)):
        K = (300.5, 301.25, w / 2, h / 2)
        frames = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        r = ctx.rectify(K, (0, 0, 0, 0), K, (w, h), (w, h))
        try:
            assert _run(ctx, r, frames, w + 4, w + 8).tobytes() == frames.tobytes()
        finally:
            r.close()


def test_host_form_and_downloaded_tables(vislam, ctx, canvas):
    Kn = _euroc_kn(vislam)
    r = ctx.rectify(EUROC_K, EUROC_D, Kn, (W, H), (736, H))
    try:
        f = vislam.synth_frame(canvas, 5, W, H, SEED)
        big = np.zeros((H, W + 40), np.uint8); big[:, :W] = f
        host = r.host(big[:, :W])                         # a strided view: in_stride = W + 40
        assert host.tobytes() == _run(ctx, r, f[None])[0].tobytes()
        assert host.tobytes() == _ref(f, EUROC_K, EUROC_D, Kn, 736, H).tobytes()
        m1, m2 = r.maps()
        l1, l2 = vislam.undistort_rectify_map(EUROC_K, EUROC_D, Kn, (736, H))
        assert m1.tobytes() == l1.tobytes() and m2.tobytes() == l2.tobytes()
    finally:
        r.close()


def _results(poses, goods, ngood):
    """pose records, the good matches each pair has (the rows beyond a pair's count are not written) and the counts"""
    return poses.tobytes(), [goods[i, :ngood[i]].tobytes() for i in range(len(ngood))], ngood.tobytes()


def test_rectify_then_batch_run_pipelined(vislam, canvas):
    """rectify -> vis_batch_run(ALL) over two consecutive launches with double-buffered outputs, against the same run synchronised after
    every call and against frames rectified on the host (rectify_ref) and uploaded"""
    torch = _torch()
    B, launches = 16, 2
    x1, y1, x2, y2 = ROI
    w, h, stride = x2 - x1, y2 - y1, 704
    Kn = _euroc_kn(vislam)
    p = vislam.default_params()
    p.w_size, p.h_size = w, h
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in Kn)
    raw = np.stack([vislam.synth_frame(canvas, t, W, H, SEED) for t in range(B * launches)])
    d_raw = [_dev(raw[k * B:(k + 1) * B]) for k in range(launches)]

    def device_run(sync):
        c = vislam.Context(0, p)
        r = c.rectify(EUROC_K, EUROC_D, Kn, (W, H), (736, H))
        c.batch_plan(w, h, stride, B)
        outs = [_empty(B * h * stride) for _ in range(2)]
        hold = [(np.zeros(B, vislam.POSE_RESULT_DTYPE), np.zeros((B, 49), vislam.DMATCH_DTYPE), np.zeros(B, np.int32)) for _ in range(launches)]
        for k in range(launches):
            r.batch(d_raw[k].data_ptr(), W, B, outs[k & 1].data_ptr(), stride, (x1, y1, w, h))
            if sync:
                torch.cuda.synchronize()
            c.batch_run(outs[k & 1].data_ptr(), B, vislam.STAGE_ALL)
            if sync:
                c.batch_sync()
            c.batch_results_async(B, hold[k][0].ctypes.data, hold[k][1].ctypes.data, hold[k][2].ctypes.data)
            if sync:
                c.batch_sync()
        c.batch_sync()
        assert c.batch_status() == 0
        res = [_results(*x) for x in hold]
        kp = [c.batch_keypoints(i) for i in range(B)]
        rect = _host(outs[(launches - 1) & 1]).reshape(B, h, stride)[:, :, :w].copy()
        r.close(); c.close()
        return res, kp, rect

    piped, kp_piped, rect_piped = device_run(False)
    synced, kp_synced, _ = device_run(True)
    # host-rectified frames, uploaded
    m1, m2 = rectify_ref.undistort_rectify_map(EUROC_K, EUROC_D, Kn, 736, H)
    host_rect = np.zeros((B * launches, h, stride), np.uint8)
    for t in range(B * launches):
        host_rect[t, :, :w] = rectify_ref.remap(raw[t], m1, m2)[y1:y2, x1:x2]
    assert rect_piped.tobytes() == np.ascontiguousarray(host_rect[B * (launches - 1):, :, :w]).tobytes()
    c = vislam.Context(0, p)
    c.batch_plan(w, h, stride, B)
    ref, kp_ref = [], None
    for k in range(launches):
        d = _dev(host_rect[k * B:(k + 1) * B])
        c.batch_run(d.data_ptr(), B, vislam.STAGE_ALL)
        ref.append(_results(*c.batch_results(B)))
        if k == launches - 1:
            kp_ref = [c.batch_keypoints(i) for i in range(B)]
    c.close()
    assert piped == synced == ref
    assert int(np.frombuffer(ref[1][2], np.int32).min()) > 0     # every pair matched something: the comparison is not vacuous
    for a, b, e in zip(kp_piped, kp_synced, kp_ref):
        assert len(a[0]) > 0 and a[0].tobytes() == b[0].tobytes() == e[0].tobytes() and a[1].tobytes() == b[1].tobytes() == e[1].tobytes()


def test_error_states(vislam, ctx):
    import ctypes as C
    r = ctx.rectify(EUROC_K, EUROC_D, _euroc_kn(vislam), (W, H), (736, H))
    try:
        d_in, d_out = _empty(2 * H * W), _empty(2 * H * 736)
        lib, ri, ro = vislam.lib, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr())
        ok = (r._r, ri, W, 2, 0, 0, 736, H, ro, 736)
        assert lib.vis_rectify_batch(*ok) == 0
        for i, v in ((4, 1), (5, 1), (4, -1), (5, -1), (6, 737), (7, 481), (6, 0), (7, 0), (9, 735), (3, 0), (3, -4), (2, W - 1), (1, None), (8, None), (0, None)):
            args = list(ok); args[i] = v
            assert lib.vis_rectify_batch(*args) == -1, (i, v)
        img = np.zeros((H, W), np.uint8); out = np.zeros((H, 736), np.uint8)
        assert lib.vis_rectify_host(r._r, img.ctypes.data, W - 1, out.ctypes.data, 736) == -1
        assert lib.vis_rectify_host(r._r, img.ctypes.data, W, out.ctypes.data, 735) == -1
        assert lib.vis_rectify_host(r._r, None, W, out.ctypes.data, 736) == -1
        assert lib.vis_rectify_host(r._r, img.ctypes.data, W, None, 736) == -1
        K, D = (np.array(v, np.float32) for v in (EUROC_K, EUROC_D))
        h = C.c_void_p()
        assert lib.vis_rectify_create(ctx._h, K.ctypes.data, D.ctypes.data, None, W, H, 736, H, C.byref(h)) == -1 and not h.value
        assert lib.vis_rectify_create(ctx._h, K.ctypes.data, D.ctypes.data, K.ctypes.data, 0, H, 736, H, C.byref(h)) == -1
        assert lib.vis_rectify_create(ctx._h, K.ctypes.data, D.ctypes.data, K.ctypes.data, W, H, 736, 4096, C.byref(h)) == -1
        assert lib.vis_rectify_create(None, K.ctypes.data, D.ctypes.data, K.ctypes.data, W, H, 736, H, C.byref(h)) == -1
        _torch().cuda.synchronize()
    finally:
        r.close()


def test_camera_model_adapter(vislam, ctx, canvas, tmp_path):
    xml = os.path.join(ROOT, "tests", "golden", "calibrationEUROC.xml")
    frame = vislam.synth_frame(canvas, 3, W, H, SEED)
    raw = tmp_path / "frame.raw"
    raw.write_bytes(frame.tobytes())
    exe = os.path.join(ROOT, "vi-slam_amd", "lib", "undistort_probe")
    out = subprocess.run([exe, xml, str(raw), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    Kn = _euroc_kn(vislam)
    assert j["valid"] == 1 and j["map1"] == [H, 736, 11] and j["map2"] == [H, 736, 2] and j["undistort"] == [H, 736]
    assert np.array(j["K"], np.float32).tobytes() == Kn.tobytes()
    assert np.array(j["K"], np.float32).tolist() == np.array([326.878448, 332.678375, 358.490997, 248.256042], np.float32).tolist()
    l1, l2 = vislam.undistort_rectify_map(EUROC_K, EUROC_D, Kn, (736, H))
    assert (tmp_path / "map1.bin").read_bytes() == l1.tobytes() and (tmp_path / "map2.bin").read_bytes() == l2.tobytes()
    r = ctx.rectify(EUROC_K, EUROC_D, Kn, (W, H), (736, H))
    try:
        assert (tmp_path / "undistort.bin").read_bytes() == r.host(frame).tobytes()
    finally:
        r.close()


def test_run_directory_rectifies_a_png_directory(vislam, canvas, tmp_path):
    """tools/run_directory.py --rectify calibrationEUROC.xml --roi (VISystem::CalculateROI's window) on an EuRoC-named PNG directory:
    frames rectified on the device, K' as the intrinsics, the oracle checked on the frames the device rectified, a trajectory written"""
    import sys
    from test_ingest import _write_png
    d = tmp_path / "mav0" / "cam0" / "data"
    d.mkdir(parents=True)
    n = 10
    for t in range(n):
        _write_png(str(d / f"{1403636579763555584 + 50000000 * t}.png"), vislam.synth_frame(canvas, t, W, H)[:, :, None], filters=[0, 2] * 240, level=1)
    xml = os.path.join(ROOT, "tests", "golden", "calibrationEUROC.xml")
    csv = tmp_path / "track.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_directory.py"), str(d), "--batch", "4", "--check", str(n), "--rectify", xml,
                        "--roi", "29,54,711,426", "--track", str(csv)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["frames"] == n and (j["width"], j["height"]) == (682, 372) and j["rectified"]["window"] == [29, 54, 682, 372]
    assert np.array(j["rectified"]["K_new"], np.float32).tobytes() == _euroc_kn(vislam).tobytes()
    kn = [float(v) for v in _euroc_kn(vislam)]
    assert j["rectified"]["K_window"] == [kn[0], kn[1], kn[2] - 29, kn[3] - 54]         # the principal point inside the cropped window
    assert j["checked_frames"] == n and j["frames_differing_from_the_oracle"] == [] and j["good_matches_mean"] > 10
    assert len(csv.read_text().splitlines()) == n


def test_rectify_then_track_pipelined(vislam, canvas):
    """rectify -> vis_batch_run(ALL | GRADIENT) -> vis_batch_track over four launches with two output buffers used in turn and no sync:
    rectify of launch k + 2 rewrites the buffer that the tracking of launch k reads on the pose stream, so it has to wait for it.  Against
    the same calls synchronised after each one, and against a run whose every launch has a buffer of its own (nothing is rewritten)."""
    import ctypes as C
    torch = _torch()
    B, launches = 16, 4
    x1, y1, x2, y2 = ROI
    w, h, stride = x2 - x1, y2 - y1, 704
    Kn = [float(v) for v in _euroc_kn(vislam)]
    p = vislam.default_params()
    p.w_size, p.h_size = w, h
    p.fx, p.cx, p.cy = Kn[0], Kn[2] - x1, Kn[3] - y1
    p.fy = p.fx
    ap = vislam.default_align_params()
    ap.fx, ap.fy, ap.cx, ap.cy = Kn[0], Kn[1], Kn[2] - x1, Kn[3] - y1
    stages = vislam.STAGE_ALL | vislam.STAGE_GRADIENT
    raw = np.stack([vislam.synth_frame(canvas, t, W, H, SEED) for t in range(B * launches)])
    d_raw = [_dev(raw[k * B:(k + 1) * B]) for k in range(launches)]
    sa, st = C.sizeof(vislam.AlignResult), C.sizeof(vislam.TrackResult)

    def run(mode):
        c = vislam.Context(0, p)
        r = c.rectify(EUROC_K, EUROC_D, Kn, (W, H), (736, H))
        c.batch_plan(w, h, stride, B)
        nbuf = launches if mode == "own" else 2
        outs = [_empty(B * h * stride) for _ in range(nbuf)]
        d_align = [_empty(B * sa) for _ in range(launches)]
        d_track = [_empty(B * st) for _ in range(launches)]
        for k in range(launches):
            d = outs[k % nbuf].data_ptr()
            r.batch(d_raw[k].data_ptr(), W, B, d, stride, (x1, y1, w, h))
            if mode == "synced":
                torch.cuda.synchronize()
            c.batch_run(d, B, stages)
            if mode == "synced":
                c.batch_sync()
            c.batch_track(ap, d, B, 0, d_align[k].data_ptr(), d_track[k].data_ptr())
            if mode == "synced":
                c.batch_sync()
        c.batch_sync()
        assert c.batch_status() == 0
        out = [(_host(a).tobytes(), _host(t).tobytes()) for a, t in zip(d_align, d_track)]
        c.close()
        assert not r._r                                   # the context closed its rectifier first
        return out

    piped, synced, own = run("piped"), run("synced"), run("own")
    assert piped == synced == own
    last = vislam.TrackResult.from_buffer_copy(own[-1][1], (B - 1) * st)
    assert last.composed != vislam.TRACK_NONE and any(abs(v) > 0 for v in (last.pose.tx, last.pose.ty, last.pose.tz))   # not vacuous


def test_context_close_closes_its_rectifiers(vislam):
    c = vislam.Context(0)
    r = c.rectify(EUROC_K, EUROC_D, _euroc_kn(vislam), (W, H), (736, H))
    r2 = c.rectify(EUROC_K, EUROC_D, _euroc_kn(vislam), (W, H), (736, H))
    r2.close()
    c.close()
    assert not r._r and not r2._r and c._rectifiers == []
    r.close()                                             # (after the context: nothing left to free, no access to it)
