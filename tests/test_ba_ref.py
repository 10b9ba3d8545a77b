"""CPU: what the restatement tests/ba_ref.py of the windowed bundle adjustment computes -- the device equals it byte for byte
(tests/test_ba_gpu.py), so its accuracy, its invariants and the branches it takes are checked here, without a device.

The scene is the prototype's: 24 cameras, 400 points seen over 3 ... 12 consecutive frames, fx = 458, pixels rounded to float, poses perturbed by
0.3 degrees and 0.02 units per frame (tests/ba_ref.py scene, built the way tests/test_ftrack_ref.py plants its own)."""
import math

import numpy as np
import pytest

import ba_cases as bc
import ba_ref as br
import ftrack_ref as fr


def run(sc, log=None, **kw):
    bq = br.Params()
    for k, v in kw.items():
        setattr(bq, k, v)
    return br.ba_rows(bq, bc.CAM, sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"], log=log)


@pytest.fixture(scope="module")
def solved():
    """the six prototype runs, computed once: (seed, noise) -> (scene, outputs, log)"""
    res = {}
    for seed in (1, 2, 3):
        for noise in (0.3, 1.0):
            sc, log = bc.scene(seed, 24, 400, noise=noise), []
            res[seed, noise] = (sc, run(sc, log), log)
    return res


@pytest.mark.parametrize("noise", [0.3, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_relative_pose_error_halves(solved, seed, noise):
    sc, (out, win, pts, fl), log = solved[seed, noise]
    ein, eout = br.relative_errors(sc["poses"], sc["truth"]), br.relative_errors(out, sc["truth"])
    print(f"\nseed {seed}, noise {noise} px: median relative error in {ein[0]:.3f} deg / {ein[1]:.4f}, out {eout[0]:.3f} deg / {eout[1]:.4f}")
    assert eout[0] <= 0.5 * ein[0] and eout[1] <= 0.5 * ein[1], (ein, eout)
    assert (win["cost1"] <= win["cost0"]).all() and (win["flags"] == br.BA_REFINED).all() and len(win) == 3
    assert (win["n_accepted"] + win["n_rejected"] == win["n_lin"]).all() and (win["n_lin"] == 10).all()
    assert bc.all_finite(sc["poses"], out, win, pts)


def test_both_branches_of_the_step_test_are_taken(solved):
    whats = [w for _, (_, _, log) in solved.items() for _, _, w in log]
    assert whats.count("accept") > 50 and whats.count("reject") > 10 and "pivot" not in whats


def test_camera_pivot_failure_is_a_rejection():
    sc, log = bc.pivot_case(), []
    out, win, pts, fl = run(sc, log)
    assert [w for _, _, w in log] == ["pivot"] * 10                 # the branch is taken, so the case keeps its meaning
    assert int(win[0]["n_rejected"]) == 10 and int(win[0]["n_accepted"]) == 0 and float(win[0]["cost1"]) == float(win[0]["cost0"])
    assert float(win[0]["lambda_"]) == 1e-4 * 1e10 and out.tobytes() == sc["poses"].tobytes()


def test_no_linearisation_returns_the_input_bytes():
    sc = bc.scene(3, 24, 400)
    out, win, pts, fl = run(sc, lm_iters=0)
    assert out.tobytes() == sc["poses"].tobytes() and (win["cost1"] == win["cost0"]).all() and (win["n_lin"] == 0).all()
    used = pts[fl == br.BAP_USED]
    assert len(used) > 500 and (used["rms0_px"] == used["rms1_px"]).all()
    # and the points are the N-view triangulation's under the input poses, window by window
    tp = fr.TriParams(max_views=17, max_reproj_px=16.0, max_parallax_cos=1.0)
    w_pts, _, _ = fr.triangulate_rows(tp, bc.CAM, sc["prev"][:9], sc["nkp"][:9], sc["obs"][:9], sc["xy"][:9], sc["poses"][:9])
    sel = fl[:9] == br.BAP_USED
    assert sel.sum() > 100 and (pts[:9][sel]["X"] == w_pts[sel]["X"]).all()


def _window_views(sc, pts, fl):
    """the used points of a one-window case with their views (frame, u, v), walked as the restatement walks them"""
    n, R = sc["obs"].shape
    nk = fr.counts(sc["prev"], sc["nkp"], R)
    X0, views = [], []
    for i in range(n):
        for k in range(int(nk[i])):
            if fl[i, k] != br.BAP_USED:
                continue
            vw, cur = [], (i, k)
            while cur is not None:
                vw.append((cur[0], float(sc["xy"][cur][0]), float(sc["xy"][cur][1])))
                cur = br._parent(sc["prev"], nk, sc["obs"], cur[0], cur[1], 0)
            assert len(vw) == int(pts[i, k]["n_views"])
            X0.append(pts[i, k]["X"].copy())
            views.append(vw)
    return np.array(X0), views


GAP = 1e-12        # measured: (cost1 - scipy minimum) / scipy minimum = -4.0e-14 at lm_iters = 10: the restatement ends AT scipy's minimum
                   # to rounding.  Twice that magnitude, 8e-14, is a few hundred ulps of a sum of 1,200 squares formed by two different programs;
                   # the bound leaves one decade over it


def test_cost_against_scipy_least_squares():
    """plain squares, one window (9 frames, anchor 0): the same points, the same start, the anchor fixed; scipy's trust-region minimum is the yardstick"""
    import scipy.optimize as scipy_opt
    sc = bc.scene(13, 9, 120)
    _, _, p0, f0 = run(sc, lm_iters=0, huber_px=0.0)
    out, win, pts, fl = run(sc, huber_px=0.0)
    X0, views = _window_views(sc, p0, f0)
    cam_i = np.array([f for vw in views for f, _, _ in vw])
    pt_i = np.array([p for p, vw in enumerate(views) for _ in vw])
    uv = np.array([[u, v] for vw in views for _, u, v in vw])
    P0 = sc["poses"]

    def residuals(x):
        Ps = [P0[0]] + [np.array(br.cayley_update(list(P0[c]), list(x[6 * (c - 1):6 * c]))) for c in range(1, 9)]
        Rm, t = np.array([p[:9].reshape(3, 3) for p in Ps]), np.array([p[9:] for p in Ps])
        X = x[48:].reshape(-1, 3)
        xc = np.einsum("nij,nj->ni", Rm[cam_i], X[pt_i]) + t[cam_i]
        return np.concatenate([bc.CAM.fx * xc[:, 0] / xc[:, 2] + bc.CAM.cx - uv[:, 0], bc.CAM.fy * xc[:, 1] / xc[:, 2] + bc.CAM.cy - uv[:, 1]])

    x0 = np.concatenate([np.zeros(48), X0.reshape(-1)])
    start = float((residuals(x0) ** 2).sum())
    assert abs(start - float(win[0]["cost0"])) <= 1e-9 * start     # the same problem
    sol = scipy_opt.least_squares(residuals, x0, method="trf", x_scale="jac", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=200)
    best = 2.0 * float(sol.cost)
    gap = (float(win[0]["cost1"]) - best) / best
    print(f"\ncost0 {start:.3f}, restatement cost1 {float(win[0]['cost1']):.6f}, scipy {best:.6f}, gap {gap:.2e}")
    assert gap <= GAP, (float(win[0]["cost1"]), best)


def test_exact_poses_stay():
    """the true poses with pixels that are exact but for their rounding to float: the adjustment moves nothing further than that rounding carries.
    A float pixel near 500 is off by at most 2^-15 px = 3.1e-5 px, an angle of 3.1e-5 / 458 = 6.7e-8 rad; with a margin of 10 over what single
    pixels do: R entries within 1e-6, t within 1e-5 (depths up to 9 units)."""
    sc = bc.scene(2, 24, 400, noise=0.0)
    sc["poses"] = sc["truth"].copy()
    out, win, pts, fl = run(sc)
    dR, dt = np.abs(out[:, :9] - sc["truth"][:, :9]).max(), np.abs(out[:, 9:] - sc["truth"][:, 9:]).max()
    print(f"\nexact poses: max |dR| {dR:.2e}, max |dt| {dt:.2e}, cost {win['cost0'].tolist()} -> {win['cost1'].tolist()}")
    assert dR <= 1e-6 and dt <= 1e-5 and (win["cost1"] <= win["cost0"]).all()


@pytest.fixture(scope="module")
def hostile_base():
    return run(bc.scene(21, 9, 160), stride=4)


@pytest.mark.parametrize("kind", bc.HOSTILE)
def test_hostile_rows_stay_finite(hostile_base, kind):
    sc, clean = bc.hostile(kind)
    out, win, pts, fl = run(sc, stride=4)
    live = np.arange(sc["row_cap"])[None, :] < sc["nkp"][:, None]
    assert bc.all_finite(sc["poses"], out, win, pts[live]) and (win["cost1"] <= win["cost0"]).all()
    for j in clean:                                                 # a window whose own frames were left alone keeps its record
        assert win[j].tobytes() == hostile_base[1][j].tobytes(), (kind, j)
    unposed = ~np.isfinite(sc["poses"]).all(1) | (sc["poses"][:, :9] == 0).all(1)
    assert out[unposed].tobytes() == sc["poses"][unposed].tobytes()
    if kind.endswith("_shared"):
        assert int(win[1]["flags"]) & br.BA_RESTART and int(win[1]["anchor"]) == 5
    if kind.endswith("_anchor"):
        assert int(win[0]["anchor"]) == 1 and not int(win[0]["flags"]) & br.BA_RESTART


def test_the_restatement_is_the_shipped_interface(vislam):
    """what this file checks is what the library ships: the restatement's defaults, record layouts, flags and window count are the binding's"""
    bp, bq = vislam.default_ba_params(), br.Params()
    for f in ("stride", "min_views", "min_points", "lm_iters", "tri_gn_iters", "huber_px", "init_reproj_px", "lambda0"):
        assert getattr(bp, f) == getattr(bq, f), f
    assert vislam.BA_WINDOW_DTYPE == br.WINDOW_DTYPE and vislam.BA_POINT_DTYPE == br.POINT_DTYPE
    assert (vislam.BA_REFINED, vislam.BA_FEW, vislam.BA_RESTART, vislam.BA_NO_SCALE) == (br.BA_REFINED, br.BA_FEW, br.BA_RESTART, br.BA_NO_SCALE)
    assert (vislam.BAP_USED, vislam.BAP_INIT_REJECTED, vislam.BAP_FEW) == (br.BAP_USED, br.BAP_INIT_REJECTED, br.BAP_FEW)
    assert all(vislam.ba_windows(n, s_) == br.n_windows(n, s_) for n in range(40) for s_ in (1, 4, 8, 16))
    assert callable(vislam.Context.ba_rows) and callable(vislam.Context.batch_ba) and hasattr(vislam.lib, "vis_ba_rows")
