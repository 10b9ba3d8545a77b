"""GPU: the windowed bundle adjustment (vis_ba_rows / vis_batch_ba) against the restatement tests/ba_ref.py, BYTE FOR BYTE: every vis_ba_window,
vis_ba_point, flag byte and output pose.  The outputs are pre-filled with 0xEE and everything the contract leaves alone (entries k >= nk(i), the
guard entries behind every buffer, everything but the poses for n <= 1) must keep it.  Shapes: row_cap 64 ... 320, n <= 35."""
import ctypes as C

import numpy as np
import pytest

import ba_cases as bc
import ba_ref as br
import ftrack_ref as fr

pytestmark = pytest.mark.gpu
FILL = 0xEE


def _dev(torch, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).cuda()    # (never an empty allocation: n == 0 still passes pointers)
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def cam_ctx(vislam):
    p = vislam.default_params()
    p.fx, p.fy, p.cx, p.cy = bc.CAM.fx, bc.CAM.fy, bc.CAM.cx, bc.CAM.cy
    c = vislam.Context(0, p)
    yield c
    c.close()


def params(vislam, **kw):
    bp, bq = vislam.default_ba_params(), br.Params()
    for k, v in kw.items():
        setattr(bp, k, v)
        setattr(bq, k, v)
    return bp, bq


def on_device(vislam, c, bp, sc):
    """(poses_out, windows, points, flags) of one vis_ba_rows, the guard entries checked"""
    import torch
    n, R = sc["obs"].shape
    nw = vislam.ba_windows(n, bp.stride)
    d = [_dev(torch, a) for a in (np.asarray(sc["prev"], np.int32), np.asarray(sc["nkp"], np.int32), sc["obs"], np.asarray(sc["xy"], np.float32),
                                  np.asarray(sc["poses"], np.float64))]
    po, wi, pts, fl = _filled(torch, (n + 1) * 96), _filled(torch, (nw + 1) * 80), _filled(torch, (n * R + 2) * 40), _filled(torch, n * R + 16)
    c.ba_rows(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), R, d[3].data_ptr(), d[4].data_ptr(), po.data_ptr(), wi.data_ptr(), pts.data_ptr(),
              fl.data_ptr(), bp)
    c.batch_sync()
    rpo, rwi, rp, rf = po.cpu().numpy(), wi.cpu().numpy(), pts.cpu().numpy(), fl.cpu().numpy()
    assert (rpo[n * 96:] == FILL).all() and (rwi[nw * 80:] == FILL).all() and (rp[n * R * 40:] == FILL).all() and (rf[n * R:] == FILL).all()
    return (rpo[:n * 96].view(np.float64).reshape(n, 12), rwi[:nw * 80].view(vislam.BA_WINDOW_DTYPE), rp[:n * R * 40].view(vislam.BA_POINT_DTYPE).reshape(n, R),
            rf[:n * R].reshape(n, R))


def restated(bq, sc, log=None):
    n, R = sc["obs"].shape
    fill_p = np.full(n * R * 40, FILL, np.uint8).view(br.POINT_DTYPE).reshape(n, R)
    return br.ba_rows(bq, bc.CAM, sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"], fill_p, np.full((n, R), FILL, np.uint8), log)


def check(vislam, c, sc, where, log=None, **kw):
    bp, bq = params(vislam, **kw)
    got = on_device(vislam, c, bp, sc)
    want = restated(bq, sc, log)
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[3].tobytes() == want[3].tobytes(), (where, np.argwhere(got[3] != want[3])[:5])
    n, R = sc["obs"].shape
    bad = [(i, k) for i in range(n) for k in range(R) if got[2][i, k].tobytes() != want[2][i, k].tobytes()]
    assert not bad, (where, len(bad), bad[:3], got[2][bad[0]], want[2][bad[0]])
    assert got[0].tobytes() == want[0].tobytes(), (where, np.argwhere(got[0] != want[0])[:5])
    return got


@pytest.mark.parametrize("n,stride", [(0, 8), (1, 8), (2, 8), (3, 8), (4, 4), (5, 4), (6, 4), (9, 4), (5, 1)])
def test_window_edges(vislam, cam_ctx, n, stride):
    """no window, one free pose, n = S, S + 1, S + 2, 2 S + 1, and a stride of one frame"""
    sc = bc.scene(30 + n, n, 90, row_cap=96)
    _, win, pts, _ = check(vislam, cam_ctx, sc, (n, stride), stride=stride, min_points=4)
    assert len(win) == br.n_windows(n, stride)
    if n >= 4:
        assert (win["flags"] & br.BA_REFINED).all() and (win["cost1"] < win["cost0"]).all() and int(win["n_accepted"].sum()) > 0
        assert int((pts["flags"] == br.BAP_USED).sum()) == int(win["n_points"].sum()) > 0


def test_sixteen_free_frames(vislam, cam_ctx):
    """S = 16 with n = 33: two windows of 96 unknowns each"""
    sc = bc.scene(5, 33, 260)
    _, win, _, _ = check(vislam, cam_ctx, sc, "S = 16", stride=16, lm_iters=3)
    assert win["n_free"].tolist() == [16, 16] and int(win["n_accepted"].sum()) > 0


@pytest.mark.parametrize("K,row_cap", [(63, 64), (64, 64), (65, 72), (255, 256), (256, 320), (257, 320)])
def test_keypoint_counts_at_the_wave_and_batch_edges(vislam, cam_ctx, K, row_cap):
    sc = bc.chain(40 + K, 5, K, row_cap)
    _, win, _, _ = check(vislam, cam_ctx, sc, K, stride=4, lm_iters=2)
    assert K - 2 <= int(win[0]["n_points"]) <= K and int(win[0]["n_obs"]) == 5 * int(win[0]["n_points"])      # (the gate may reject a point or two)


@pytest.mark.parametrize("K", [0, 11, 12])
def test_few_points(vislam, cam_ctx, K):
    """a window with no point, with min_points - 1 and with min_points points"""
    sc = bc.chain(50 + K, 5, K, 64)
    out, win, _, _ = check(vislam, cam_ctx, sc, K, stride=4)
    assert int(win[0]["flags"]) == (br.BA_REFINED if K == 12 else br.BA_FEW) and int(win[0]["n_points"]) == K
    if K < 12:
        assert out.tobytes() == np.asarray(sc["poses"], np.float64).tobytes()


@pytest.mark.parametrize("lm_iters", [0, 1, 10])
@pytest.mark.parametrize("huber_px", [0.0, 2.4477])
def test_iterations_and_loss(vislam, cam_ctx, lm_iters, huber_px):
    sc = bc.scene(7, 9, 120, noise=1.0)
    out, win, _, _ = check(vislam, cam_ctx, sc, (lm_iters, huber_px), stride=4, lm_iters=lm_iters, huber_px=huber_px)
    assert (win["n_lin"] == lm_iters).all() and (win["cost1"] <= win["cost0"]).all()
    if lm_iters == 0:
        assert out.tobytes() == np.asarray(sc["poses"], np.float64).tobytes()


def test_the_prototype_scene_with_rejected_steps(vislam, cam_ctx):
    """24 cameras, 400 points, the defaults: accepted and rejected steps, and the accuracy the CPU file asserts"""
    sc = bc.scene(1, 24, 400)
    log = []
    out, win, _, _ = check(vislam, cam_ctx, sc, "prototype", log)
    assert any(w == "reject" for _, _, w in log) and any(w == "accept" for _, _, w in log)
    ein, eout = br.relative_errors(sc["poses"], sc["truth"]), br.relative_errors(out, sc["truth"])
    assert eout[0] <= 0.5 * ein[0] and eout[1] <= 0.5 * ein[1], (ein, eout)


def test_camera_pivot_failure(vislam, cam_ctx):
    sc = bc.pivot_case()
    log = []
    out, win, _, _ = check(vislam, cam_ctx, sc, "pivot", log)
    assert [w for _, _, w in log] == ["pivot"] * 10 and int(win[0]["n_rejected"]) == 10 and float(win[0]["cost1"]) == float(win[0]["cost0"])
    assert out.tobytes() == np.asarray(sc["poses"], np.float64).tobytes()


@pytest.mark.parametrize("kind", bc.HOSTILE)
def test_hostile_rows(vislam, cam_ctx, kind):
    sc, clean = bc.hostile(kind)
    out, win, pts, fl = check(vislam, cam_ctx, sc, kind, stride=4)
    live = np.arange(sc["row_cap"])[None, :] < sc["nkp"][:, None]
    assert bc.all_finite(sc["poses"], out, win, pts[live])
    base = on_device(vislam, cam_ctx, params(vislam, stride=4)[0], bc.scene(21, 9, 160))
    for j in clean:                                                 # a window whose own frames were left alone keeps its record
        assert win[j].tobytes() == base[1][j].tobytes(), (kind, j, win[j], base[1][j])


def test_two_runs_and_the_reach_of_a_pose(vislam, cam_ctx):
    sc = bc.scene(8, 9, 140)
    bp = params(vislam, stride=4)[0]
    a, b = on_device(vislam, cam_ctx, bp, sc), on_device(vislam, cam_ctx, bp, sc)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for frame, other in ((1, 1), (7, 0)):                           # a pose changed outside window `other` leaves its record unchanged
        moved = dict(sc)
        moved["poses"] = sc["poses"].copy()
        moved["poses"][frame, 9] += 0.01
        m = on_device(vislam, cam_ctx, bp, moved)
        assert m[1][other].tobytes() == a[1][other].tobytes() and m[1][1 - other].tobytes() != a[1][1 - other].tobytes()


@pytest.mark.parametrize("gate", [False, True])
def test_batch_ba_against_the_rows_form(vislam, canvas, gate):
    """vis_batch_ba on the keypoints and the pairing of a vis_batch_run equals vis_ba_rows on the same rows"""
    import torch
    W, H, B = 320, 240, 8
    frames = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(B)])
    if gate:
        frames[3] = 128                                             # flat: the gate does not save it
    p = vislam.default_params()
    p.fy = p.fx
    p.cx, p.cy = W / 2.0, H / 2.0
    if gate:
        p.keyframe_min_points = 10
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    KC = c.keypoint_capacity(W, H)
    CAP = KC + 3
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    obs, fr_ = _filled(torch, B * CAP * 16), _filled(torch, B * 32)
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_ALL)
    c.batch_ftrack(B, CAP, obs.data_ptr(), fr_.data_ptr())
    poses = np.zeros((B, 12))
    for i in range(B):
        a = 0.002 * i
        poses[i, :9] = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
        poses[i, 9:] = [-0.05 * i, 0.0, 0.0]
    if gate:
        poses[3] = 0.0                                              # (a posed frame without keypoints would fail the camera pivot every time)
    bp = vislam.default_ba_params()
    bp.stride, bp.init_reproj_px, bp.lm_iters = 4, 200.0, 3
    nw = vislam.ba_windows(B, 4)
    d_poses = _dev(torch, poses)
    po, wi, pts, fl = _filled(torch, B * 96), _filled(torch, nw * 80), _filled(torch, B * CAP * 40), _filled(torch, B * CAP)
    arg = lambda t: C.c_void_p(t.data_ptr())
    call = lambda n=B, cap=CAP, o=obs: vislam.lib.vis_batch_ba(c._h, C.byref(bp), n, arg(o), cap, arg(d_poses), arg(po), arg(wi), arg(pts), arg(fl))
    assert call(n=B - 1) == -5 and call(cap=KC - 1) == -4 and call(n=B - 1, cap=KC - 1) == -5         # VIS_E_STATE before VIS_E_CAPACITY
    c.batch_ba(B, obs.data_ptr(), CAP, d_poses.data_ptr(), po.data_ptr(), wi.data_ptr(), pts.data_ptr(), fl.data_ptr(), bp)
    c.batch_sync()
    assert c.batch_status() == 0
    prev = np.asarray(c.batch_get_keyframes(), np.int32)
    kps = [c.batch_keypoints(i)[0] for i in range(B)]
    xy = np.zeros((B, CAP, 2), np.float32)
    for i in range(B):
        xy[i, :len(kps[i]), 0], xy[i, :len(kps[i]), 1] = kps[i]["x"], kps[i]["y"]
    h_obs = obs.cpu().numpy().view(vislam.FTRACK_OBS_DTYPE).reshape(B, CAP)
    rows = dict(prev=prev, nkp=np.array([len(k) for k in kps], np.int32), obs=h_obs, xy=xy, poses=poses, row_cap=CAP)
    want = on_device(vislam, c, bp, rows)
    got = (po.cpu().numpy().view(np.float64).reshape(B, 12), wi.cpu().numpy().view(vislam.BA_WINDOW_DTYPE),
           pts.cpu().numpy().view(vislam.BA_POINT_DTYPE).reshape(B, CAP), fl.cpu().numpy().reshape(B, CAP))
    for g, w_, name in zip(got, want, ("poses", "windows", "points", "flags")):
        assert g.tobytes() == w_.tobytes(), (gate, name)
    assert int(got[1]["n_points"].sum()) > 0 and (gate is False or (prev == vislam.KF_NOT_SAVED).any())
    c.close()
