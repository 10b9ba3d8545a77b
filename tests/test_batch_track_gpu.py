"""GPU: batched camera tracking (vis_batch_track) -- for every frame of a vis_batch_run, the alignment of its keyframe pair (the pair
to the keyframe carried from the launch before included) and VISystem::Track, final_poseCam = final_poseCam * SE3(R, t), in the order
VISystemGPU::AddFrameGPU runs them.  752 x 480 synthetic stream, EuRoC cam0 intrinsics (the default alignment parameters, as in the
adapter test).  Expected values: the oracle's EstimatePoseFeatures on each pair and the oracle's SE3 chain; for the keyframe gate a
Python frameList walk; and the frame-at-a-time adapters (vislam_main_gpu) for the whole trajectory.  Comparisons are bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_cases
from batch_track_cases import Oracle as _Oracle, decode as _decode, residual as _residual

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vi-slam_amd", "lib", "vislam_main_gpu")
W, H = 752, 480
E_STATE = -5
INIT7 = [0.05, -0.1, 0.02, 0.9934, 0.3, -0.2, 1.5]      # a non-identity final_poseCam to start from (normalised below)


def _stages(vislam):
    return vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT


def _init_pose(vislam, orc):
    q = np.array(INIT7[:4], np.float64)
    q /= np.linalg.norm(q)
    e = vislam.Se3f(*[float(np.float32(x)) for x in list(q) + INIT7[4:]])
    M = orc.se3_matrix(e)                                 # a unit quaternion as the library rounds it
    return orc.se3_from_rt(M[:3, :3], M[:3, 3])


def _as_vis(vislam, e):
    return vislam.Se3f(*[float(x) for x in e.as_array()])


def _context(vislam, B, K=0, params=None):
    p = params or vislam.default_params()
    if params is None:
        p.fy = p.fx
    p.keyframe_min_points = K
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    return c


def _out(vislam, n, sync=True):
    import torch
    a = torch.zeros(n * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
    t = torch.zeros(n * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
    if sync:
        torch.cuda.synchronize()                          # (torch's fill and the library's non-blocking streams are not ordered)
    return a, t


def _track(vislam, c, ap, ptr, n, d_init=0, out=None):
    a, t = out or _out(vislam, n)
    c.batch_track(ap, ptr, n, d_init, a.data_ptr(), t.data_ptr())
    return a, t


@pytest.fixture(scope="module")
def plain(vislam, canvas):
    import torch
    frames = np.stack([vislam.synth_frame(canvas, t, W, H) for t in range(48)])
    return frames, torch.from_numpy(frames).cuda()


def _zero(rec):
    return bytes(rec) == bytes(C.sizeof(rec))


def test_gate_off_every_pair_and_the_chain(vislam, orc, plain):
    """three launches of 16: every frame's record equals the oracle's alignment of (previous frame -> frame), pair 0 of launches 2
    and 3 (against the carried frame) included; d_track equals the oracle chain from a non-identity pose; pairs 1..n-1 equal what
    vis_batch_align gives for the same launch"""
    import torch
    frames, dev = plain
    ap = vislam.default_align_params()
    init = _init_pose(vislam, orc)
    c = _context(vislam, 16)
    c.batch_track_init(_as_vis(vislam, init))
    oracle = _Oracle(orc, frames)
    final, kps, checked = init, {}, 0
    for li in range(3):
        ptr = dev.data_ptr() + li * 16 * W * H
        c.batch_run(ptr, 16, _stages(vislam))
        ref_out = torch.zeros(16 * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_align(ap, ptr, 16, 0, 0, 0, 0, ref_out.data_ptr())
        a, t = _track(vislam, c, ap, ptr, 16)
        c.batch_sync()
        assert c.batch_status() == 0
        al, tr, ra, _ = _decode(vislam, a, t, 16)
        rb = ref_out.cpu().numpy().tobytes()
        sa = C.sizeof(vislam.AlignResult)
        assert ra[sa:] == rb[sa:], li
        assert _zero(vislam.AlignResult.from_buffer_copy(rb, 0)), li                       # vis_batch_align still skips pair 0
        for i in range(16):
            g = li * 16 + i
            kps[g] = c.batch_keypoints(i)[0]
            if g == 0:
                assert _zero(al[i]) and tr[i].composed == vislam.TRACK_NONE
                assert tr[i].pose.as_array().tobytes() == final.as_array().tobytes()
                continue
            good = c.batch_matches(i)[0]
            ref = oracle.align(g - 1, g, kps[g - 1][good["queryIdx"]])
            assert align_cases.result_tuple(al[i]) == align_cases.result_tuple(ref), (li, i)
            assert al[i].n_residuals[0] > 0, (li, i)
            final = orc.se3_mul(final, _residual(orc, ref.pose))
            assert tr[i].composed == i, (li, i)
            assert tr[i].pose.as_array().tobytes() == final.as_array().tobytes(), (li, i)
            checked += 1
    assert checked == 47
    c.close()


def test_batch_size_independence(vislam, orc, plain):
    """48 frames in launches of 8, 16, 24 and 48: identical d_align and d_track poses (no pair is lost at a launch boundary); the
    `composed` field is the batch index of the frame's own pair"""
    frames, dev = plain
    ap = vislam.default_align_params()
    init = _as_vis(vislam, _init_pose(vislam, orc))
    got = {}
    for n in (8, 16, 24, 48):
        c = _context(vislam, 48)
        c.batch_track_init(init)
        ra, rt = b"", b""
        for s in range(0, 48, n):
            ptr = dev.data_ptr() + s * W * H
            c.batch_run(ptr, n, _stages(vislam))
            a, t = _track(vislam, c, ap, ptr, n)
            c.batch_sync()
            _, tr, x, _ = _decode(vislam, a, t, n)
            ra += x
            rt += b"".join(r.pose.as_array().tobytes() for r in tr)
            want = [vislam.TRACK_NONE if s + i == 0 else i for i in range(n)]
            assert [r.composed for r in tr] == want, (n, s)
        assert c.batch_status() == 0
        c.close()
        got[n] = (ra, rt)
    for n in (16, 24, 48):
        assert got[n][0] == got[8][0], n
        assert got[n][1] == got[8][1], n


# ---- keyframe gate: streams with featureless (flat) and sparse frames, restated from the gate's own test ----------------------------
FLAT, SPARSE, NORMAL = "F", "S", "N"
GATE_LAUNCHES = [
    # flat at stream position 0 (nothing saved yet), flat mid-batch, two in a row, a sparse frame, a flat LAST frame
    "F N N F N F F N S N N N N N N F",
    # only flat frames: the snapshot of the keyframe (frame 14 of the launch before) must survive it
    "F F F F F F F F F F F F F F F F",
    # frame 0 links to the keyframe carried over two launches
    "N N F N N N N N S N N N N N N N",
    # a flat frame 0: frame 1's pair is the one to the carried keyframe
    "F N N N N N N N N N N N N N N F",
    None,
    # after the reset: a sparse frame first (saved under both rules), a flat frame, then plain frames
    "S N N F N N N N N N N N N N N N",
]


def _sparse(t):
    f = np.full((H, W), 128, np.uint8)
    x, y = 160 + 37 * (t % 11), 120 + 23 * (t % 7)
    f[y:y + 5, x:x + 5] = 255
    return f


def _gate_stream(vislam, canvas):
    frames, launches, resets, reset_next = [], [], [], False
    for spec in GATE_LAUNCHES:
        if spec is None:
            reset_next = True
            continue
        idx = []
        for k in spec.split():
            t = len(frames)
            frames.append(np.full((H, W), 128, np.uint8) if k == FLAT else _sparse(t) if k == SPARSE else vislam.synth_frame(canvas, t, W, H))
            idx.append(t)
        launches.append(idx)
        resets.append(reset_next)
        reset_next = False
    return launches, resets, np.stack(frames)


@pytest.fixture(scope="module")
def gated(vislam, canvas):
    import torch
    launches, resets, frames = _gate_stream(vislam, canvas)
    return launches, resets, frames, torch.from_numpy(frames).cuda()


@pytest.mark.parametrize("K", [1, 10])
def test_gate_on_against_the_frame_list(vislam, orc, gated, K):
    """AddFrameGPU's rule per frame: a saved frame with a pair composes its own residual, a refused frame composes the last pair's
    residual again once two frames have been saved (it may be a launch or more old), nothing is composed before the second saved
    frame; vis_batch_reset restarts at the vis_batch_track_init pose"""
    launches, resets, frames, dev = gated
    ap = vislam.default_align_params()
    init = _init_pose(vislam, orc)
    c = _context(vislam, 16, K)
    c.batch_track_init(_as_vis(vislam, init))
    oracle = _Oracle(orc, frames)
    kps, saved, final, last = {}, [], init, None
    n_own = n_last = n_carried_pairs = n_carried_last = 0
    for li, (idx, reset) in enumerate(zip(launches, resets)):
        if reset:
            c.batch_reset()
            saved, final, last = [], init, None
        n, start = len(idx), idx[0]
        ptr = dev.data_ptr() + start * W * H
        c.batch_run(ptr, n, _stages(vislam))
        a, t = _track(vislam, c, ap, ptr, n)
        c.batch_sync()
        assert c.batch_status() == 0
        al, tr, _, _ = _decode(vislam, a, t, n)
        links = c.batch_get_keyframes()
        for i, g in enumerate(idx):
            kps[g] = c.batch_keypoints(i)[0]
        for i, g in enumerate(idx):
            if len(kps[g]) > (K if saved else 1):               # Camera.cpp:225 / CameraGPU.cpp:164: saved
                if saved:
                    j = saved[-1]
                    assert links[i] == (j - start if j >= start else vislam.KF_CARRIED), (li, i, links[i])
                    good = c.batch_matches(i)[0]
                    ref = oracle.align(j, g, kps[j][good["queryIdx"]])
                    assert align_cases.result_tuple(al[i]) == align_cases.result_tuple(ref), (li, i)
                    last = _residual(orc, ref.pose)
                    final = orc.se3_mul(final, last)
                    assert tr[i].composed == i, (li, i)
                    n_own += 1
                    n_carried_pairs += j < start
                else:
                    assert links[i] == vislam.KF_FIRST and _zero(al[i]) and tr[i].composed == vislam.TRACK_NONE, (li, i)
                saved.append(g)
            else:
                assert links[i] == vislam.KF_NOT_SAVED and _zero(al[i]), (li, i)
                if last is not None:                            # frameList.size() > 1: the last pair again
                    final = orc.se3_mul(final, last)
                    j = saved[-1]
                    assert tr[i].composed == (j - start if j >= start else vislam.KF_CARRIED), (li, i, tr[i].composed)
                    n_last += 1
                    n_carried_last += j < start
                else:
                    assert tr[i].composed == vislam.TRACK_NONE, (li, i)
            assert tr[i].pose.as_array().tobytes() == final.as_array().tobytes(), (li, i)
    c.close()
    # what the stream exercised: pairs to a carried keyframe (one two launches old), refused frames re-composing, across a launch too
    assert n_own >= 45 and n_carried_pairs >= 2 and n_last >= 20 and n_carried_last >= 16, (n_own, n_carried_pairs, n_last, n_carried_last)


CAL_XML = """<?xml version="1.0"?>
<!-- synthetic EuRoC-shaped calibration: ORB + GPU Hamming matcher, no distortion -->
<opencv_storage>
<in_width type_id="integer"> 752 </in_width>
<in_height type_id="integer"> 480 </in_height>
<out_width type_id="integer"> 752 </out_width>
<out_height type_id="integer"> 480 </out_height>
<calibration_values type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 458.654 457.296 367.215 248.375 </data></calibration_values>
<rectification type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 0 0 0 0 </data></rectification>
<imu2cam0Transformation type_id="opencv-matrix">
  <rows>4</rows> <cols>4</cols> <dt>f</dt>
  <data> 0.0148655429818 -0.999880929698 0.00414029679422 -0.0216401454975
         0.999557249008 0.0149672133247 0.025715529948 -0.064676986768
        -0.0257744366974 0.00375618835797 0.999660727178 0.00981073058949
         0.0 0.0 0.0 1.0 </data></imu2cam0Transformation>
<camera_frecuency type_id="float"> 20 </camera_frecuency>
<imu_frecuency type_id="float"> 200 </imu_frecuency>
<min_features type_id="integer"> 20</min_features>
<num_max_keyframes type_id="integer"> 10</num_max_keyframes>
<start_index type_id="integer"> 0 </start_index>
<use_gt type_id="integer">1</use_gt>
<use_ros type_id="integer">0</use_ros>
<num_cells type_id="integer"> 49</num_cells>
<length_patch type_id="integer"> 3</length_patch>
<detector type_id="integer">2</detector>
<matcher type_id="integer">4</matcher>
</opencv_storage>
"""


def _f32(line):
    return np.array([int(x, 16) for x in line.split()[1:]], np.uint32).view(np.float32)


def test_equal_to_the_adapters(vislam, orc, canvas, tmp_path):
    """the reference main's class surface (vislam_main_gpu, frame at a time) and vis_batch_run + vis_batch_track in launches of 16
    give the same final_poseCam for every one of 45 frames (stream frames 2, 3, ...)"""
    import torch
    nframes = 45
    f = tmp_path / "cal.xml"
    f.write_text(CAL_XML)
    out = subprocess.run([EXE, str(f), str(nframes), str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    init = _f32([l for l in lines if l.startswith("INITPOSE")][0])
    fposes = [_f32(l) for l in lines if l.startswith("FINALPOSE")]
    assert len(fposes) == nframes
    Kc = [458.654, 457.296, 367.215, 248.375]
    p = vislam.default_params()
    p.fx = p.fy = float(np.float32(Kc[0]))
    p.cx, p.cy = float(np.float32(Kc[2])), float(np.float32(Kc[3]))
    p.w_size, p.h_size = W, H
    c = _context(vislam, 16, 1, params=p)
    ap = vislam.default_align_params()
    ap.fx, ap.fy, ap.cx, ap.cy = [float(np.float32(x)) for x in Kc]
    c.batch_track_init(vislam.Se3f(*[float(x) for x in init]))
    seed = orc.se3_from_rt(np.eye(3, dtype=np.float32), np.array([-0.0, -0.0, -0.0], np.float32))     # the adapters' SE3(I, -TranslationResidual)
    seeds = torch.from_numpy(np.tile(seed.as_array(), (16, 1)).copy()).cuda()
    frames = torch.from_numpy(np.stack([vislam.synth_frame(canvas, i + 2, W, H) for i in range(nframes)])).cuda()
    torch.cuda.synchronize()
    got = []
    for s in range(0, nframes, 16):
        n = min(16, nframes - s)
        ptr = frames.data_ptr() + s * W * H
        c.batch_run(ptr, n, _stages(vislam))
        a, t = _track(vislam, c, ap, ptr, n, seeds.data_ptr())
        c.batch_sync()
        got += _decode(vislam, a, t, n)[1]
    assert c.batch_status() == 0
    c.close()
    for i in range(nframes):
        assert got[i].pose.as_array().tobytes() == fposes[i].tobytes(), (i, got[i].pose.as_array(), fposes[i])
    assert not np.array_equal(fposes[-1], init)


def test_pipelined_equals_synchronised(vislam):
    """the gpu_main_sequence call pattern -- batch_run(i + 1) queued right behind batch_track(i), no sync -- over 6 launches of 64
    frames gives what the same launches give with batch_sync() after every call"""
    import torch
    n, L, dim, seedc = 64, 6, 4096, 0xE0C00001
    ap = vislam.default_align_params()
    res = {}
    for piped in (True, False):
        c = _context(vislam, n)
        canvas = torch.from_numpy(vislam.synth_canvas(dim, seedc)).cuda()
        frames = torch.empty((n * L, H, W), dtype=torch.uint8, device="cuda")
        c.synth_frames_device(canvas.data_ptr(), dim, seedc, 0, n * L, W, H, W, frames.data_ptr())
        bufs = [_out(vislam, n, sync=False) for _ in range(L)]
        torch.cuda.synchronize()
        outs = []
        for li in range(L):
            ptr = frames.data_ptr() + li * n * W * H
            c.batch_run(ptr, n, _stages(vislam))
            if not piped:
                c.batch_sync()
            outs.append(_track(vislam, c, ap, ptr, n, out=bufs[li]))
            if not piped:
                c.batch_sync()
        c.batch_sync()
        torch.cuda.synchronize()
        assert c.batch_status() == 0
        res[piped] = [(a.cpu().numpy().tobytes(), t.cpu().numpy().tobytes()) for a, t in outs]
        c.close()
    for li in range(L):
        assert res[True][li][0] == res[False][li][0], li
        assert res[True][li][1] == res[False][li][1], li
    tr = vislam.TrackResult.from_buffer_copy(res[True][L - 1][1], (n - 1) * C.sizeof(vislam.TrackResult))
    assert tr.composed == n - 1 and tr.pose.as_array().tobytes() != vislam.Se3f(0, 0, 0, 1, 0, 0, 0).as_array().tobytes()


def _code(fn):
    try:
        fn()
    except Exception as e:                                  # noqa: BLE001
        return getattr(e, "code", repr(e))
    return 0


def test_errors(vislam, orc, plain):
    import torch
    frames, dev = plain
    ap = vislam.default_align_params()
    ptr = dev.data_ptr()
    a, t = _out(vislam, 16)
    trk = lambda c, n=8: (lambda: c.batch_track(ap, ptr, n, 0, a.data_ptr(), t.data_ptr()))   # noqa: E731
    # no plan
    c = vislam.Context(0)
    assert _code(trk(c)) == E_STATE and _code(lambda: c.batch_track_init(None)) == E_STATE
    c.close()
    # no VIS_STAGE_GRADIENT / no VIS_STAGE_MATCH / n != last_n
    c = _context(vislam, 16)
    c.batch_run(ptr, 8, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert _code(trk(c)) == E_STATE
    c.batch_reset()
    c.batch_run(ptr, 8, vislam.STAGE_DETECT | vislam.STAGE_GRADIENT)
    assert _code(trk(c)) == E_STATE
    c.batch_reset()
    c.batch_run(ptr, 8, _stages(vislam))
    assert _code(trk(c, 7)) == E_STATE
    assert _code(trk(c)) == 0                               # (the failed calls left the launch to be tracked)
    assert _code(trk(c)) == E_STATE                         # a launch is tracked once
    # a launch in the middle that was not tracked
    c.batch_run(ptr + 8 * W * H, 8, _stages(vislam))
    c.batch_run(ptr + 16 * W * H, 8, _stages(vislam))
    assert _code(trk(c)) == E_STATE
    c.batch_sync()
    c.close()
    # pose_input != VIS_POSE_GOOD
    p = vislam.default_params()
    p.fy = p.fx
    p.pose_input = 1
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, 16)
    c.batch_run(ptr, 8, _stages(vislam))
    assert _code(trk(c)) == E_STATE
    c.batch_sync()
    # ... and a later valid plan / run / track of the same context is right: equal to a fresh context's
    p.pose_input = 0
    c.set_params(p)
    got = {}
    for which, cc in (("reused", c), ("fresh", None)):
        if cc is None:
            cc = _context(vislam, 16)
        else:
            cc.batch_plan(W, H, W, 16)
        outs = b""
        for s in (0, 16):
            cc.batch_run(ptr + s * W * H, 16, _stages(vislam))
            a2, t2 = _track(vislam, cc, ap, ptr + s * W * H, 16)
            cc.batch_sync()
            outs += a2.cpu().numpy().tobytes() + t2.cpu().numpy().tobytes()
        assert cc.batch_status() == 0
        cc.close()
        got[which] = outs
    assert got["reused"] == got["fresh"]
    torch.cuda.synchronize()


def test_run_directory_writes_the_trajectory(vislam, plain, tmp_path):
    """tools/run_directory.py --track out.csv on an EuRoC-named directory (20 PGM frames, batches of 8): one row per frame, positionCam
    x, y, z and qOrientationCam x, y, z, w, equal to vis_batch_track's poses from the identity (GPU main's keyframe rule)"""
    import sys
    frames, dev = plain
    n = 20
    d = tmp_path / "data"
    d.mkdir()
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "track.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_directory.py"), str(d), "--frames", str(n), "--batch", "8",
                        "--nfeatures", "1000", "--track", str(csv)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [[float(x) for x in l.split(",")] for l in csv.read_text().strip().splitlines()]
    assert len(rows) == n and all(len(x) == 7 for x in rows)
    p = vislam.default_params()
    p.nfeatures, p.w_size, p.h_size = 1000, W, H
    p.fy = p.fx
    c = _context(vislam, 8, 1, params=p)
    ap = vislam.default_align_params()
    want = []
    for s in range(0, n, 8):
        nb = min(8, n - s)
        ptr = dev.data_ptr() + s * W * H
        c.batch_run(ptr, nb, vislam.STAGE_FRAME | vislam.STAGE_GRADIENT)
        a, t = _track(vislam, c, ap, ptr, nb)
        c.batch_sync()
        want += [e.pose for e in _decode(vislam, a, t, nb)[1]]
    c.close()
    for i, (row, e) in enumerate(zip(rows, want)):
        assert np.array(row, np.float32).tobytes() == np.array([e.tx, e.ty, e.tz, e.qx, e.qy, e.qz, e.qw], np.float32).tobytes(), i
    assert rows[0] == [0, 0, 0, 0, 0, 0, 1] and rows[-1] != rows[0]
