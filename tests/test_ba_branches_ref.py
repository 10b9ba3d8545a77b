"""CPU: the restatement tests/ba_ref.py on the cases of tests/ba_branch_cases.py -- every case TAKES the branch it is named for (asserted from the
restatement's own records, log and sit-out counts), stays finite and does not raise the cost.  The device equals these runs byte for byte
(tests/test_ba_branches_gpu.py), so what is asserted here is asserted of the kernel.  Also: a swap of fx and fy changes the result under the two
planted anisotropic cameras (so those cases can see one), and the cost under the 1 : 2 camera against scipy's minimum."""
import numpy as np
import pytest

import ba_branch_cases as bb
import ba_cases as bc
import ba_ref as br
import ftrack_ref as fr
from test_ba_ref import _window_views


@pytest.mark.parametrize("name", list(bb.CASES) + list(bb.BASES))
def test_the_case_takes_its_branch(name):
    r = bb.restated(name)
    w = bb.whats(r)
    print(f"\n{name}: flags {r.win['flags'].tolist()}, points {r.win['n_points'].tolist()}, {w.count('accept')} accepts, {w.count('reject')} rejects, "
          f"{w.count('pivot')} pivots, {sum(bb.sitouts(r))} sit-outs, cost {r.win['cost0'].tolist()} -> {r.win['cost1'].tolist()}, "
          f"lambda {r.win['lambda_'].tolist()}, scale {r.win['scale'].tolist()}")
    assert (bb.CASES.get(name) or bb.BASES[name]).reached(r), name
    assert bb.finite(r) and (r.win["cost1"] <= r.win["cost0"]).all()
    assert (r.win["n_accepted"] + r.win["n_rejected"] == r.win["n_lin"]).all() and len(r.log) == len(r.stats) == int(r.win["n_lin"].sum())
    assert (r.pts.view(np.uint8).reshape(r.live.shape + (40,))[~r.live] == bb.FILL).all() and (r.fl[~r.live] == bb.FILL).all()


def test_the_sit_out_counts_do_not_change_the_log_form():
    """ba_rows' stats argument is optional and the log keeps its 3-tuples"""
    sc = bb.proto()
    log = []
    a = br.ba_rows(br.Params(stride=4), bc.CAM, sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"], log=log)
    r = bb.restated("wide_gate")
    assert all(len(e) == 3 for e in log) and len(log) == 20 and sum(bb.sitouts(r)) == 0
    b = bb.run(sc, bb.PROTO_CAM, stride=4)
    assert a[0].tobytes() == b.out.tobytes() and a[1].tobytes() == b.win.tobytes() and log == b.log


@pytest.mark.parametrize("name", ["aniso_default", "aniso_wide"])
def test_a_swap_of_fx_and_fy_is_seen(name):
    """the same rows under (fy, fx, cx, cy): another start cost and other output bytes, so the device comparison of this case fails on a swap"""
    r = bb.restated(name)
    s = bb.run(r.sc, bb.swapped(r.cam), **r.kw)
    assert (s.win["cost0"] != r.win["cost0"]).all() and s.out.tobytes() != r.out.tobytes() and s.pts.tobytes() != r.pts.tobytes()


def test_triangulation_sees_a_swap_of_fx_and_fy():
    """the N-view triangulation (csrc/ftri_core.h is one text for both) on the rows of the 1 : 2 camera"""
    sc = bb.restated("aniso_wide").sc
    tp = fr.TriParams(**bb.TRI_KW)
    a = fr.triangulate_rows(tp, bb.camera(bb.WIDE_CAM), sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"])
    b = fr.triangulate_rows(tp, bb.camera(bb.swapped(bb.WIDE_CAM)), sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"])
    assert int(a[2]["n_kept"].sum()) > 50 and a[0].tobytes() != b[0].tobytes() and a[1].tobytes() != b[1].tobytes()


GAP_WIDE = 1.3e-6  # measured: (cost1 - scipy minimum) / scipy minimum = +6.35e-8 at lm_iters = 10 under the camera (300, 600, 100, 400):
                   # 87.01274102 against scipy's 87.01273549.  Ten linearisations have not ended here as they have under fx = fy: at lm_iters = 30 the
                   # restatement reads 87.012735492355, scipy 87.012735492360.  The rule of tests/test_ba_ref.py GAP: one decade over twice the measured
                   # magnitude, 1.27e-7.  scipy runs with its default variable scaling: with x_scale="jac" it stops on xtol at 165.49, far above both


def test_cost_against_scipy_least_squares_under_the_wide_camera():
    """test_ba_ref.py's yardstick with fx != fy: plain squares, one window (9 frames, anchor 0), the same points and start, the anchor fixed; the
    residual function below is this test's own (fx on the first coordinate, fy on the second)"""
    import scipy.optimize as scipy_opt
    cam = bb.camera(bb.WIDE_CAM)
    sc = br.scene(13, cam, n_cam=9, n_pts=120, span=(3, 9))
    p0, f0 = bb.run(sc, bb.WIDE_CAM, lm_iters=0, huber_px=0.0)[5:7]
    win = bb.run(sc, bb.WIDE_CAM, huber_px=0.0).win
    X0, views = _window_views(sc, p0, f0)
    cam_i = np.array([f for vw in views for f, _, _ in vw])
    pt_i = np.array([p for p, vw in enumerate(views) for _ in vw])
    uv = np.array([[u, v] for vw in views for _, u, v in vw])
    P0 = sc["poses"]

    def residuals(x):
        Ps = [P0[0]] + [np.array(br.cayley_update(list(P0[c]), list(x[6 * (c - 1):6 * c]))) for c in range(1, 9)]
        Rm, t = np.array([p[:9].reshape(3, 3) for p in Ps]), np.array([p[9:] for p in Ps])
        xc = np.einsum("nij,nj->ni", Rm[cam_i], x[48:].reshape(-1, 3)[pt_i]) + t[cam_i]
        return np.concatenate([300.0 * (xc[:, 0] / xc[:, 2]) + 100.0 - uv[:, 0], 600.0 * (xc[:, 1] / xc[:, 2]) + 400.0 - uv[:, 1]])

    x0 = np.concatenate([np.zeros(48), X0.reshape(-1)])
    start = float((residuals(x0) ** 2).sum())
    assert len(win) == 1 and abs(start - float(win[0]["cost0"])) <= 1e-9 * start     # the same problem
    sol = scipy_opt.least_squares(residuals, x0, method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=200)
    best = 2.0 * float(sol.cost)
    gap = (float(win[0]["cost1"]) - best) / best
    print(f"\ncost0 {start:.3f}, restatement cost1 {float(win[0]['cost1']):.6f}, scipy {best:.6f}, gap {gap:.2e}")
    assert sol.status > 0 and gap <= GAP_WIDE, (float(win[0]["cost1"]), best)
