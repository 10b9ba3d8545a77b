"""GPU: vis_ba_rows / vis_batch_ba on the cases of tests/ba_branch_cases.py against the restatement tests/ba_ref.py, BYTE FOR BYTE as in
tests/test_ba_gpu.py (whose helpers and 0xEE guards are used): every output pose, vis_ba_window, vis_ba_point and flag byte.  What each case
reaches -- fx != fy, points sitting a linearisation out, VIS_BA_NO_SCALE, both damping clamps, the ends of every parameter, translations from
2^-600 to 2^1000 -- is asserted of the restatement in tests/test_ba_branches_ref.py; the same runs are the reference here.
Shapes: 9 frames, row_cap 112 ... 144, two windows (one case: 18 frames of 40 keypoints at row_cap 64, S = 16)."""
import numpy as np
import pytest

import ba_branch_cases as bb
from test_ba_gpu import FILL, _dev, _filled, on_device, params
from test_ftrack_gpu import check_tri

pytestmark = pytest.mark.gpu
assert FILL == bb.FILL


@pytest.fixture(scope="module")
def contexts(vislam):
    """a context per camera, made when a case first asks for it"""
    made = {}

    def get(cam):
        if cam not in made:
            p = vislam.default_params()
            p.fx, p.fy, p.cx, p.cy = cam
            made[cam] = vislam.Context(0, p)
        return made[cam]
    yield get
    for c in made.values():
        c.close()


def equal(got, want, sc, where):
    """test_ba_gpu.check's comparison against a restatement that is already there: (poses, windows, points, flags)"""
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[3].tobytes() == want[3].tobytes(), (where, np.argwhere(got[3] != want[3])[:5])
    n, R = sc["obs"].shape
    bad = [(i, k) for i in range(n) for k in range(R) if got[2][i, k].tobytes() != want[2][i, k].tobytes()]
    assert not bad, (where, len(bad), bad[:3], got[2][bad[0]], want[2][bad[0]])
    assert got[0].tobytes() == want[0].tobytes(), (where, np.argwhere(got[0] != want[0])[:5])


@pytest.mark.parametrize("name", list(bb.CASES))
def test_the_case_on_the_device(vislam, contexts, name):
    r = bb.restated(name)
    bp, bq = params(vislam, **r.kw)
    assert all(getattr(bq, k) == v for k, v in r.kw.items())
    got = on_device(vislam, contexts(r.cam), bp, r.sc)
    equal(got, (r.out, r.win, r.pts, r.fl), r.sc, name)


def test_triangulation_under_the_wide_camera(vislam, contexts):
    """vis_ftrack_triangulate_rows (csrc/ftri_core.h, the text the adjustment shares) on the rows of the camera (300, 600, 100, 400)"""
    sc = bb.restated("aniso_wide").sc
    pts, fl, sm = check_tri(vislam, contexts(bb.WIDE_CAM), bb.camera(bb.WIDE_CAM), sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"], "wide camera",
                            **bb.TRI_KW)
    assert int(sm["n_kept"].sum()) > 50


def test_batch_ba_against_the_rows_form_with_fx_not_fy(vislam, canvas):
    """test_ba_gpu.py's test_batch_ba_against_the_rows_form (ungated) with the library's own fx = 458.654, fy = 457.296: vis_batch_ba equals
    vis_ba_rows on the same rows, and vis_ba_rows equals the restatement under that camera"""
    import torch
    W, H, B = 320, 240, 8
    frames = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(B)])
    p = vislam.default_params()
    assert (p.fx, p.fy) == bb.DEFAULT_CAM[:2] and p.fx != p.fy
    p.cx, p.cy = W / 2.0, H / 2.0
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
    bp = vislam.default_ba_params()
    bp.stride, bp.init_reproj_px, bp.lm_iters = 4, 200.0, 3
    nw = vislam.ba_windows(B, 4)
    d_poses = _dev(torch, poses)
    po, wi, pts, fl = _filled(torch, B * 96), _filled(torch, nw * 80), _filled(torch, B * CAP * 40), _filled(torch, B * CAP)
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
        assert g.tobytes() == w_.tobytes(), name
    assert int(got[1]["n_points"].sum()) > 0
    r = bb.run(rows, (p.fx, p.fy, p.cx, p.cy), stride=4, init_reproj_px=200.0, lm_iters=3)
    equal(want, (r.out, r.win, r.pts, r.fl), rows, "rows form under fx != fy")
    c.close()
