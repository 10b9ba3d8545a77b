"""CPU: what the restatements (tests/pnp_ref.py, homography_ref.py + homography_pose_ref.py, f2f_ref.py, triangulate_ref.py) and the CPU
oracle's essential RANSAC do with correspondences that are not usable numbers: the rows of tests/hostile_cases.py (every kind x layout that
applies, 40 points and one more than an LDS tile; the magnitude ladder of finite pixels on one image).  tests/test_hostile_inputs_gpu.py holds
the kernels to the same records.

The expected figures were measured on these restatements at the default parameters and are pinned here; the properties (no hostile entry in
a mask, counts equal mask sums, finite hc.orthonormal winners, masks equal to the predicate evaluated exactly with mpmath) are asserted on
every row."""
import numpy as np
import pytest

import essential_refine_ref as er
import f2f_ref as fr
import homography_pose_ref as hpr
import homography_ref as hr
import hostile_cases as hc
import pnp_ref as pr
import pose_degenerate_cases as pdc
import triangulate_ref as tr

# ---------------------------------------------------------------------------------------------- PnP
def test_pnp_rows():
    rows, clean = hc.pnp_rows()
    assert int(clean[hc.M][0]["n_inliers"]) == 40 and int(clean[hc.TILE + 1][0]["n_inliers"]) == hc.TILE + 1
    for (kind, lay), row in rows.items():
        hc.check_pnp_row(kind, lay, row, row["rec"], row["mask"])
    # the figures of the 8-of-40 rows: the hostile entries cost their eight inliers and nothing else
    for kind in hc.pnp_kinds():
        rec, mask = rows[kind, "stride5"]["rec"], rows[kind, "stride5"]["mask"]
        if kind in ("X:centre", "X:tiny"):
            # eight copies of one point under eight different pixels: one of them is explained by the pose (tiny: entry 0 is still itself)
            assert int(rec["n_inliers"]) == 33 and int(mask[rows[kind, "stride5"]["idx"]].sum()) == 1, (kind, rec)
            continue
        got = (int(rec["n_inliers"]), int(rec["n_inliers_refined"]), int(rec["best_iter"]), int(rec["flags"]), float(rec["cost0"]), float(rec["cost1"]))
        assert got == (32, 32, 0, pr.REFINED, 7.356578742685758e-05, 3.189373830276841e-05), (kind, got)
        assert rec["R"].tobytes() == rows["X:nan", "stride5"]["rec"]["R"].tobytes(), kind       # one pose, whatever made the eight unusable


def _counts(X, xy, draws):
    rec, mask = pr.pnp(pr.Camera(), pr.default_params(), X, xy, draws)
    return rec, mask


def test_pnp_overflowing_points_were_inliers():
    """Before the per-point test required a finite right-hand side, thr2 (W W) = +inf let inf <= inf pass: a map point whose depth squares
    past DBL_MAX (|X| > 1.34e154), or with an infinite coordinate that leaves W = +inf, was an inlier of EVERY pose.  It raised every
    hypothesis' count (40 of 40 with eight such points), entered the mask, and its residuals entered the Gauss-Newton sums: the `refined'
    pose kept 10 of the 32 true inliers, or cost0 was NaN and the refinement rejected.  With the rule, every such row gives the record of the
    32 usable points."""
    base, draws = hc.pnp_base(hc.M), hc.pnp_draws()
    idx = hc.layout("stride5", hc.M)
    mixed = base["X"].copy()
    mixed[idx[:4]] *= 1e200
    mixed[idx[4:], 0] = -np.inf
    rows = {k: hc.hostile(f"X:{k}", base, idx)["X"] for k in ("x1e200", "x1e160", "x1e150", "pinf")}
    rows["mixed"] = mixed
    for name, X in rows.items():
        rec, mask = _counts(X, base["xy"], draws)
        got = (int(rec["n_inliers"]), int(mask[idx].sum()), int(rec["n_inliers_refined"]), int(rec["flags"]), float(rec["cost0"]))
        assert got == (32, 0, 32, pr.REFINED, 7.356578742685758e-05), (name, got)
    # the predicate itself: under the true pose the overflowing points fail, the points below the overflow are judged as numbers
    cam, pp = pr.Camera(), pr.default_params()
    _, thr2 = pr.thresholds(cam, pp)
    x, y = pr.normalise(cam, base["xy"])
    P = [float(v) for v in np.asarray(base["R"]).reshape(9)] + [float(v) for v in base["t"]]
    assert pr.inliers(P, base["X"], x, y, thr2).all()
    for name in ("x1e200", "x1e160", "pinf"):
        assert not pr.inliers(P, rows[name], x, y, thr2)[idx].any(), name
    v150, _ = hc.exact_inlier_pnp(P, rows["x1e150"], base["xy"], cam.cx, cam.cy, 1.0 / cam.fx, thr2)
    assert (pr.inliers(P, rows["x1e150"], x, y, thr2) == v150).all() and not v150[idx].any()


# ---------------------------------------------------------------------------------------------- homography and its pose
def test_homography_rows_and_their_pose():
    rows, clean = hc.h_rows()
    assert int(clean[hc.M][0]["n_inliers"]) == 40
    kinds = set()
    for (kind, lay), row in rows.items():
        pose = hc.check_h_row(kind, lay, row, row["rec"], row["mask"])
        kinds.add(int(pose["kind"]))
    assert kinds >= {hpr.HP_NONE, hpr.HP_PLANE}
    for kind in hc.pair_kinds():
        rec = rows[kind, "stride5"]["rec"]
        got = (int(rec["n_inliers"]), int(rec["best_iter"]), float(rec["score_h"]), int(rows[kind, "stride5"]["mask"][::5].sum()))
        assert got == (32, 30, 341.3981345811111, 0), (kind, got)


# ---------------------------------------------------------------------------------------------- F2F and the epipolar filter
@pytest.fixture(scope="module")
def f2f_params(vislam):
    p = vislam.default_params()
    p.fy, p.f2f_iters = p.fx, hc.ITERS
    return p


def test_f2f_rows(f2f_params):
    rows, clean = hc.f2f_rows(f2f_params)
    c40 = clean[hc.M]["rec"]
    assert (int(c40["count_max"]), int(c40["best_iter"])) == (40, 7)
    for (kind, lay), row in rows.items():
        hc.check_f2f_row(kind, lay, row, row["rec"], row["keep"], row["nkeep"])
    want_ndeg = {"nan": 4, "pinf": 4, "ninf": 4, "inf_all": 4, "big": 6}
    for kind in hc.pair_kinds():
        target, name = kind.split(":")
        rec = rows[kind, "stride5"]["rec"]
        if name == "dup":                                              # a correspondence that did not move is data: one of the eight agrees
            assert (int(rec["count_max"]), int(rec["best_iter"]), int(rec["n_degenerate"])) == (33, 7, 6), (kind, rec)
            continue
        ndeg = 14 if kind == "both:big" else want_ndeg[name]          # both images at the same +-3e38: the normal is exactly zero
        assert (int(rec["count_max"]), int(rec["best_iter"]), int(rec["n_degenerate"])) == (32, 7, ndeg), (kind, rec)
        assert np.asarray(rec["t"], np.float32).tobytes() == np.asarray(c40["t"], np.float32).tobytes(), kind


# ---------------------------------------------------------------------------------------------- the essential RANSAC (CPU oracle)
@pytest.fixture(scope="module")
def oracle_params(vislam, orc):
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    op = orc.Params()
    for f, _ in p._fields_:
        setattr(op, f, getattr(p, f))
    return op


def test_essential_rows(orc, oracle_params):
    rows, clean = hc.essential_rows(orc, oracle_params)
    assert (clean[40]["n_inliers"], clean[40]["iters_run"]) == (39, 3)
    for (kind, lay, m), row in rows.items():
        hc.check_essential_row(kind, lay, m, row, row["E"], row["mask"], row["n_inliers"], row["iters_run"], row["R"], row["t"], row["n_pose_good"],
                            int(oracle_params.ransac_max_iters))
    for kind in hc.PAIR_NEVER:
        row = rows[kind, "stride5", 40]
        assert (row["n_inliers"], row["iters_run"]) == (31, 21), (kind, row["n_inliers"], row["iters_run"])
        # recoverPose votes over every correspondence, as the reference: a finite point at +-3e38 can triangulate in front (four of p1's do)
        assert row["n_pose_good"] == (32 if kind in hc.PAIR_NONFINITE else {"p1:big": 36}.get(kind, 32)), (kind, row["n_pose_good"])
    row = rows["both:nan", "all", 40]
    assert not row["E"].any() and row["iters_run"] == 1000 and np.isnan(row["R"]).all()
    # the magnitude ladder: a finite pixel, however large, on one image.  From k = 1e-6 up no ladder entry is in any winner's mask (cap: zero
    # rows left out; hc.check_essential_row asserted it above on every row -- the scene seed of hc.essential_base is the choice that makes it
    # true of the ORACLE, so a device mask that holds one is the device's doing), and the 32 clean points of the 8-of-40 rows keep the pose
    # that the non-finite kinds leave them
    mags = [k for k in rows if hc.mag_of(k[0]) is not None]
    assert len(mags) == len(hc.mag_pair_kinds()) * 2 * len(hc.ESSENTIAL_MAG_LENGTHS) and len(hc.MAG_LADDER) == 11
    left_out = [k for k in mags if hc.mag_of(k[0]) >= hc.MAG_NEVER_FROM and rows[k]["mask"][rows[k]["idx"]].any()]
    assert left_out == []
    ref = rows["both:nan", "stride5", 40]
    for kind in hc.mag_pair_kinds():
        row = rows[kind, "stride5", 40]
        assert (row["n_inliers"], row["iters_run"]) == (31, 21) and row["mask"].tobytes() == ref["mask"].tobytes(), (kind, row["n_inliers"], row["iters_run"])
        assert row["E"].tobytes() == ref["E"].tobytes() and row["R"].tobytes() == ref["R"].tobytes() and row["t"].tobytes() == ref["t"].tobytes(), kind


def test_essential_refine_count_needs_a_finite_bound():
    """the second place of the finite-side rule: n_inliers0 / n_inliers_refined of the refinement counted s s <= thr2 den without asking for a
    finite den, so a pixel with one infinite coordinate (s = den = +inf) was counted under every pose: 36 and 40 of 40 where 32 are usable"""
    base = hc.essential_base(hc.M)
    idx = hc.layout("stride5", hc.M)
    cam, ep = er.Camera(), er.default_params()
    clean = er.refine(cam, ep, base["R"], base["t"], base["p1"], base["p2"])
    assert int(clean["n_inliers0"]) == 40
    for kind in hc.PAIR_NONFINITE:
        h = hc.hostile(kind, base, idx)
        rec = er.refine(cam, ep, base["R"], base["t"], h["p1"], h["p2"])
        assert (int(rec["n_inliers0"]), int(rec["n_inliers_refined"])) == (32, 32), (kind, rec)
        assert np.isfinite(float(rec["cost0"])) and np.isfinite(float(rec["cost1"])) and hc.orthonormal(rec["R"]), (kind, rec)


# ---------------------------------------------------------------------------------------------- triangulation
def test_triangulation_rows():
    rows, clean = hc.tri_rows()
    s = clean["summary"]
    assert (s["n_front"], s["n_kept"]) == (40, 40) and np.isfinite(s["mean_parallax_px"])
    for (kind, lay), row in rows.items():
        hc.check_tri_row(kind, lay, row, row["pts"], row["flags"], row["summary"])
    for kind in hc.PAIR_NONFINITE:
        s = rows[kind, "stride5"]["summary"]
        assert (s["n_front"], s["n_kept"]) == (32, 32), (kind, s)
        assert not np.isfinite(s["mean_parallax_px"]), (kind, s)
    s = rows["p1:big", "stride5"]["summary"]
    assert (s["n_front"], s["n_kept"], s["mean_parallax_px"]) == (36, 32, np.float32(np.inf)), s       # four of the eight far points are FRONT
    s = rows["t:zero", "none"]["summary"]
    assert s["n_front"] == 0 and s["n_kept"] == 0


# ---------------------------------------------------------------------------------------------- the helpers themselves
def test_same_record_and_exact_inlier():
    a = pr.zero_record()
    b = a.copy()
    a["cost0"], b["cost0"] = np.nan, -np.nan                           # two NaNs of different sign are the same answer
    assert a.tobytes() != b.tobytes() and hc.same_record(a, b)
    b["cost1"] = 1.0
    assert not hc.same_record(a, b) and hc.differing_fields(a, b) == ["cost1"] and hc.same_record(a, b, skip=("cost1",))
    b = a.copy()
    b["R"][4] = -0.0                                                   # +0 and -0 are different bytes
    assert not hc.same_record(a, b)
    b = a.copy()
    b["flags"] = 1
    assert not hc.same_record(a, b)
    # exact_inlier: a point one part in 1000 inside / outside the threshold circle (float pixels resolve 3e-5 here), a NaN, a point behind the camera
    cam, pp = pr.Camera(), pr.default_params()
    fx_inv, thr2 = pr.thresholds(cam, pp)
    P = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]
    X = np.array([[0.0, 0.0, 5.0]] * 4)
    X[3, 2] = -5.0
    r = pp.threshold_px
    xy = np.array([[cam.cx + r * (1 - 1e-3), cam.cy], [cam.cx + r * (1 + 1e-3), cam.cy], [np.nan, cam.cy], [cam.cx, cam.cy]], np.float32)
    v, d = hc.exact_inlier_pnp(P, X, xy, cam.cx, cam.cy, fx_inv, thr2)
    assert v.tolist() == [True, False, False, False] and d[2] == np.inf and 1e-4 < d[0] < 1e-2 and 1e-4 < d[1] < 1e-2
    with pytest.raises(AssertionError):
        hc.check_exact(np.array([1, 1, 0, 0]), v, np.maximum(d, 1.0), "a mask that differs")
    with pytest.raises(AssertionError):
        hc.check_exact(v, v, np.array([1.0, 1e-10, 1.0, 1.0]), "a point within the margin")
    I = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    _, _, t_h, _, _ = hr.thresholds(hr.Camera(), hr.default_params())
    rh = np.sqrt(hr.default_params().chi2_h) * hr.default_params().sigma_px
    x1 = np.array([[100.0, 100.0]] * 3, np.float32)
    x2 = np.array([[100.0 + rh * 0.999, 100.0], [100.0 + rh * 1.001, 100.0], [np.inf, 100.0]], np.float32)
    v, d = hc.exact_inlier_h(I, x1, x2, cam.cx, cam.cy, fx_inv, t_h)
    assert v.tolist() == [True, False, False] and d[2] == np.inf
