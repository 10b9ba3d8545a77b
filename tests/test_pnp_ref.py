"""CPU: the restatement of PnP (tests/pnp_ref.py) on its own -- no library, no device.

Scenes: pnp_ref.table_cases(), 7 classes x M 40 / 300 x noise 0 / 0.3 px x 0 / 25 % of the pixels replaced, 200 samples of
default_rng(7) at the default 2 px threshold.  Every bound below is 100 x what an independent method reaches on the same data (the rule of
DESIGN.md sections 4.10 and 4.11), never a figure of the code under test:

* a P3P pose against the equations of its own sample: the independent method is numpy.roots on the quartic and numpy.linalg.svd (Kabsch)
  for the rotation between the two triples, on the same sample.  THE RULE HERE IS NOT THE ISSUE'S TO THE LETTER.  The issue's rule --
  every pose within 100 x the independent method's residual on the same sample -- cannot be met by any code: on five of the samples below the
  independent method's side residual is exactly 0, and in general the two methods' residuals on one sample are two draws of one
  amplified rounding error (Grunert's quartic loses up to three digits in its coefficients, the same three for both methods), whose
  ratio is heavy-tailed: some 0.6 % of the ratios of two equally distributed errors exceed 100.  Measured: 32 of 18 264 poses (0.18 %)
  are beyond 100 x their own sample's figure, the worst a `tilted` M 300 sample at 2.95e-10 against 1.5e-12; no conditioning
  criterion separates them (triangle side ratios 0.02 ... 0.8, root conditioning 0.02 ... 3e5, the population's own range).  So the test
  asserts (a) EVERY pose within 100 x the independent method's worst figure over the samples of the same case, and (b) the issue's
  per-sample rule for at least 99 % of the poses -- the share is asserted, and it follows from the 0.6 % above, not from the count
  found.  R^T R - I and det R - 1 do not depend on the sample and are held to the case's figure throughout.  There is no absolute floor.
* truth at noise 0: the independent method is that P3P over the same samples plus a Rodrigues / lstsq Gauss-Newton run to convergence.
* refinement at noise 0.3: the independent minimiser, 20 iterations from the TRUE pose over the same mask, against the same minimiser
  started from the winner.  The REPORTED pose (default parameters, five steps) is held to 100 x that figure, or, where the independent
  minimiser started from the winner is itself further than that from its limit after the same five steps (a Gauss-Newton on a problem
  with residuals converges linearly: `plane` M 40, `far`), to 100 x the independent minimiser's own five-step distance; a second record
  with 20 steps is held to the first figure alone."""
import numpy as np
import pytest

import pnp_ref as pr

CAM = pr.Camera()
EXCEPTION_SHARE = 0.01


@pytest.fixture(scope="module")
def draws():
    return pr.make_draws(7)


@pytest.fixture(scope="module")
def runs(draws):
    """case -> (scene, hypotheses, record, mask) at the default parameters, computed once"""
    out = {}
    pp = pr.default_params()
    for case in pr.table_cases():
        scene = pr.make_scene(*case)
        hyp = pr.hypotheses(CAM, pp, scene[0], scene[1], draws)
        rec, mask = pr.finish(CAM, pp, scene[0], scene[1], hyp, *pr.pick(hyp, 200))
        out[case] = (scene, hyp, rec, mask)
    return out


def test_every_solution_satisfies_the_equations_of_its_sample(runs):
    print()
    n_poses = n_exc = 0
    for case, ((X, xy, _, _, _), hyp, _, _) in runs.items():
        if case[0] == "line":
            assert not hyp["live"].any()
            continue
        f = pr.bearings(CAM, xy)
        live = np.flatnonzero(hyp["live"].any(1))
        ind = {}
        for j in live:                                             # the independent method on every sample of the case first
            idx = hyp["idx"][j]
            res = [np.array(pr.solution_residuals(R, t, X[idx], f[idx])) for R, t in pr.p3p_independent(X[idx], f[idx])]
            ind[int(j)] = np.max(res, 0) if res else None
        ind_w = np.max([v for v in ind.values() if v is not None], 0)
        mine_w, exc = np.zeros(4), 0
        for j in live:
            idx = hyp["idx"][j]
            P, fs = X[idx], f[idx]
            reach = ind_w if ind[int(j)] is None else np.array([ind[int(j)][0], ind[int(j)][1], ind_w[2], ind_w[3]])
            for r in np.flatnonzero(hyp["live"][j]):
                pose = hyp["poses"][j, r]
                res = np.array(pr.solution_residuals(pose[:9], pose[9:], P, fs))
                n_poses += 1
                assert (res <= 100.0 * ind_w).all(), (case, int(j), int(r), res, ind_w)
                exc += int(ind[int(j)] is None or bool((res > 100.0 * reach).any()))
                mine_w = np.maximum(mine_w, res)
        n_exc += exc
        print(f"{case}: sides / parallel / R^T R - I / det - 1   restated {mine_w[0]:.1e} {mine_w[1]:.1e} {mine_w[2]:.1e} {mine_w[3]:.1e}   "
              f"independent {ind_w[0]:.1e} {ind_w[1]:.1e} {ind_w[2]:.1e} {ind_w[3]:.1e}   poses beyond 100 x their own sample's figure: {exc}")
    print(f"{n_poses} poses, {n_exc} of them beyond 100 x the independent method's figure on their own sample")
    assert n_poses > 10000 and n_exc <= EXCEPTION_SHARE * n_poses


def test_root_finder_against_numpy_roots(runs):
    """every real root numpy.roots sees in (0, B) that is simple is found, in ascending order, to 100 x numpy's own residual"""
    worst = 0.0
    for case, (_, hyp, _, _) in runs.items():
        G = hyp["geo"]
        for j in np.flatnonzero(G["ok"])[:50]:
            c = [float(G["c"][k][j]) for k in range(5)]
            got = hyp["roots"][j, :int(hyp["nroots"][j])]
            assert (np.diff(got) > 0).all() and (got > 0).all() and (got < G["B"][j]).all()
            scale = sum(abs(c[k]) * max(got.max(initial=1.0), 1.0) ** k for k in range(5))
            ref = np.roots(c[::-1])
            ref = np.sort(ref[(np.abs(ref.imag) < 1e-7 * np.maximum(1.0, np.abs(ref.real))) & (ref.real > 0)].real)
            for v in got:                                              # each found root is a root: a sign change within one step of the bisection
                lo, hi = np.nextafter(v, 0.0), np.nextafter(v, np.inf)
                pv = [np.polyval(c[::-1], u) for u in (lo, v, hi)]
                assert min(pv) <= 0.0 <= max(pv) or min(abs(p) for p in pv) <= 64 * 2.0 ** -52 * scale, (case, j, v, pv)
                if len(ref):
                    worst = max(worst, float(np.abs(ref - v).min() / max(v, 1.0)))
            well = [v for v in ref if np.abs(np.polyval(np.polyder(c[::-1]), v)) > 1e-6 * scale]
            for v in well:                                             # and no well-separated root of numpy's is missed
                assert len(got) and np.abs(got - v).min() <= 1e-6 * max(v, 1.0), (case, j, v, got)
    print(f"\nlargest relative distance of a found root from numpy.roots' nearest: {worst:.2e}")


def test_every_planted_inlier_is_found(runs, draws):
    pp = pr.default_params()
    n = 0
    for case, ((X, xy, planted, _, _), _, rec, mask) in runs.items():
        if case[0] not in pr.REGULAR:
            continue
        n += 1
        assert (mask.astype(bool) | ~planted).all(), (case, int(mask.sum()), int(planted.sum()))
        assert int(rec["n_inliers"]) == int(mask.sum()) >= int(planted.sum()) and int(rec["n_points"]) == case[1]
        _, _, imask = pr.ransac_independent(CAM, pp, X, xy, draws)
        assert (imask | ~planted).all(), (case, "the scene does not hold for the independent method")
    assert n == 40                                                     # no case left out


def test_truth_at_noise_zero(runs, draws):
    pp = pr.default_params()
    print()
    for case, ((X, xy, _, R, t), _, rec, mask) in runs.items():
        if case[2] != 0.0 or case[0] == "line":
            continue
        Ri, ti, imask = pr.ransac_independent(CAM, pp, X, xy, draws)
        Rg, tg = pr.gn_independent(CAM, X, xy, imask, Ri, ti, 20)
        e_r, e_t = pr.rot_diff(rec["R"], R), float(np.abs(rec["t"] - t).max())
        i_r, i_t = pr.rot_diff(Rg, R), float(np.abs(tg - t).max())
        u_r, u_t = pr.rot_diff(rec["R_ransac"], R), float(np.abs(rec["t_ransac"] - t).max())
        print(f"{case}: |R R_true^T - I| / max |t - t_true|   unrefined {u_r:.1e} {u_t:.1e}   reported {e_r:.1e} {e_t:.1e}   independent {i_r:.1e} {i_t:.1e}")
        assert int(rec["flags"]) == pr.REFINED
        assert e_r <= 100.0 * i_r, (case, e_r, i_r)
        if case[0] != "far":                                           # points at 1e6 do not determine the translation: printed, not bounded
            assert e_t <= 100.0 * i_t, (case, e_t, i_t)


def test_refinement_at_noise(runs):
    pp20 = pr.default_params()
    pp20.refine_iters = 20
    slow = 0
    print()
    for case, ((X, xy, _, R, t), hyp, rec, mask) in runs.items():
        if case[2] == 0.0 or case[0] == "line":
            continue
        assert float(rec["cost1"]) <= float(rec["cost0"]) and int(rec["flags"]) == pr.REFINED, case
        rec20, mask20 = pr.finish(CAM, pp20, X, xy, hyp, *pr.pick(hyp, 200))
        assert mask20.tobytes() == mask.tobytes() and float(rec20["cost1"]) <= float(rec20["cost0"])
        Ra, ta = pr.gn_independent(CAM, X, xy, mask, R, t, 20)
        Rb, tb = pr.gn_independent(CAM, X, xy, mask, rec["R_ransac"], rec["t_ransac"], 20)
        i_r, i_t = pr.rot_diff(Ra, Rb), float(np.abs(ta - tb).max())
        Rc, tc = pr.gn_independent(CAM, X, xy, mask, rec["R_ransac"], rec["t_ransac"], 5)          # the independent minimiser after the same five steps
        j_r, j_t = pr.rot_diff(Ra, Rc), float(np.abs(ta - tc).max())
        d5 = (pr.rot_diff(rec["R"], Ra), float(np.abs(rec["t"] - ta).max()))
        d20 = (pr.rot_diff(rec20["R"], Ra), float(np.abs(rec20["t"] - ta).max()))
        slow += int(j_r > 100.0 * i_r or j_t > 100.0 * i_t)
        print(f"{case}: from the independent minimiser, |R Ra^T - I| / max |t - ta|   reported (5 steps) {d5[0]:.1e} {d5[1]:.1e}   20 steps {d20[0]:.1e} {d20[1]:.1e}   "
              f"independent from the winner, 20 steps {i_r:.1e} {i_t:.1e}, 5 steps {j_r:.1e} {j_t:.1e}   cost {float(rec['cost0']):.2e} -> {float(rec['cost1']):.2e}")
        # the REPORTED pose: the issue's bound, or where the independent minimiser itself has not converged after five steps, 100 x ITS distance
        assert d5[0] <= 100.0 * max(i_r, j_r), (case, d5, i_r, j_r)
        assert d20[0] <= 100.0 * i_r, (case, d20, i_r)
        if case[0] != "far":
            assert d5[1] <= 100.0 * max(i_t, j_t), (case, d5, i_t, j_t)
            assert d20[1] <= 100.0 * i_t, (case, d20, i_t)
    print(f"cases in which the independent minimiser is more than 100 x its converged figure away after five steps: {slow} of 24")
    assert slow <= 6                                                   # the five-step bound is the issue's own in three quarters of the cases at least


def test_line_is_the_zero_record(runs):
    for case, (_, hyp, rec, mask) in runs.items():
        if case[0] != "line":
            continue
        want = pr.zero_record()
        want["n_points"], want["n_degenerate"] = case[1], 200        # every sample counted degenerate
        assert rec.tobytes() == want.tobytes() and not mask.any(), case


def test_three_and_four_points(draws):
    X, xy, _, R, t = pr.make_scene("general", 40, 0.0, 0.0)
    pp = pr.default_params()
    rec, mask = pr.pnp(CAM, pp, X[:3], xy[:3], draws)
    assert rec.tobytes() == pr.zero_record().tobytes() and len(mask) == 3 and not mask.any()
    pp.min_inliers = 4
    rec, mask = pr.pnp(CAM, pp, X[:4], xy[:4], draws)
    assert int(rec["n_points"]) == 4 and int(rec["n_inliers"]) == 4 and mask.all() and int(rec["best_iter"]) >= 0
    assert int(rec["flags"]) & (pr.REFINED | pr.REFINE_REJECTED) and pr.rot_diff(rec["R"], R) < 1e-5
    pp.iters = 0
    rec, mask = pr.pnp(CAM, pp, X, xy, draws)
    assert rec.tobytes() == pr.zero_record().tobytes() and not mask.any()


def test_few_flag_and_no_refinement():
    """a winner below min_inliers is reported unrefined with VIS_PNP_FEW; refine_iters = 0 reports the winner with equal costs"""
    X, xy, _, _, _ = pr.make_scene("general", 40, 0.0, 0.0)
    rng = np.random.default_rng(5)
    xy = xy.copy()
    xy[5:] = rng.uniform(0, 400, (35, 2)).astype(np.float32)           # five correspondences survive
    table = np.array([[0, 1, 2], [1, 3, 4]], np.int32)
    pp = pr.default_params()
    pp.iters = 2
    rec, mask = pr.pnp(CAM, pp, X, xy, table)
    assert 5 <= int(rec["n_inliers"]) < 8 and int(rec["flags"]) == pr.FEW
    assert rec["R"].tobytes() == rec["R_ransac"].tobytes() and float(rec["cost0"]) == float(rec["cost1"])
    pp.min_inliers, pp.refine_iters = 4, 0
    rec, mask = pr.pnp(CAM, pp, X, xy, table)
    assert int(rec["flags"]) == 0 and rec["t"].tobytes() == rec["t_ransac"].tobytes() and float(rec["cost0"]) == float(rec["cost1"])


def test_a_sample_with_two_equal_indices():
    X, xy, _, _, _ = pr.make_scene("general", 40, 0.0, 0.0)
    table = np.array([[3, 3, 7], [43, 9, 3], [1, 2, -2 ** 31 + 41], [4, 5, 6]], np.int32)   # 43 % 40 == 3; the sign bit is masked: 41 % 40 == 1
    assert pr.sample_indices(table, 4, 40).tolist()[:3] == [[3, 3, 7], [3, 9, 3], [1, 2, 1]]
    pp = pr.default_params()
    pp.iters = 4
    hyp = pr.hypotheses(CAM, pp, X, xy, table)
    assert hyp["live"].any(1).tolist() == [False, False, False, True]
    h, ndeg, nsol = pr.pick(hyp, 4)
    assert h >> 2 == 3 and ndeg == 3 and nsol == int(hyp["live"][3].sum())


def test_tie_goes_to_the_smallest_slot():
    """the same sample twice: the earlier one wins; two roots of one sample with equal counts: the lower root wins"""
    X, xy, _, _, _ = pr.make_scene("general", 40, 0.0, 0.0)
    pp = pr.default_params()
    pp.iters = 3
    hyp = pr.hypotheses(CAM, pp, X, xy, np.array([[4, 4, 9], [10, 20, 30], [10, 20, 30]], np.int32))
    h, ndeg, _ = pr.pick(hyp, 3)
    assert h >> 2 == 1 and ndeg == 1
    live, cnt = np.array([[True, True, False, True]]), np.array([[5, 9, 99, 9]])
    assert pr.pick(dict(live=live, cnt=cnt), 1)[0] == 1


def test_singular_normal_matrix_fails_a_pivot():
    """every point the same: J^T J has rank 2, a pivot is <= 0 (or the step is not finite) and the solve reports it"""
    X, xy, _, R, t = pr.make_scene("general", 40, 0.0, 0.0)
    Xs, xys = np.repeat(X[:1], 12, 0), np.repeat(xy[:1], 12, 0)
    P = list(R.reshape(9)) + list(t)
    x, y = pr.normalise(CAM, xys)
    S, n = pr.gn_pass(P, P, Xs, x, y, 1.0)
    assert n == 12
    d, ok = pr.solve6(S)
    assert not ok
    good, _ = pr.gn_pass(P, P, X, *pr.normalise(CAM, xy), 1.0)
    d, ok = pr.solve6(good)
    assert ok and np.isfinite(d).all() and np.abs(d).max() < 1e-5


def test_cayley_update_keeps_a_rotation():
    P = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.1, 0.2, 0.3]
    for _ in range(50):
        P = pr.cayley_update(P, [0.3, -0.2, 0.25, 0.01, 0.0, -0.01])
    R = np.array(P[:9]).reshape(3, 3)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1.0) < 1e-13


def test_the_join():
    """a hand-made pair of match tables: a keypoint of frame q matched twice in pair (p -> q) (the first that has the flags wins), a point
    that lacks `require`, a correspondence of pair (q -> i) without a partner, and a frame without a pair"""
    dm = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
    mk = lambda rows: np.array([(a, b, 0, 0.0) for a, b in rows], dm)
    pq = mk([(5, 7), (6, 9), (8, 7), (2, 11), (3, 4)])              # (keypoint in p, keypoint in q): q's keypoint 7 twice (k = 0 and 2)
    qi = mk([(9, 0), (7, 1), (4, 2), (11, 3), (12, 4)])             # (keypoint in q, keypoint in i)
    KEPT = 16
    fl = np.array([1, KEPT | 3, KEPT, 15, KEPT], np.uint8)          # k = 0 lacks KEPT, k = 3 has everything but KEPT
    assert pr.join(qi, pq, fl, KEPT) == [(0, 1), (1, 2), (2, 4)]    # 7 -> k = 2 (k = 0 lacks the flag), 11 has no kept point, 12 no partner
    assert pr.join(qi, pq, fl, 0) == [(0, 1), (1, 0), (2, 4), (3, 3)]                 # no flag asked for: the FIRST of the two
    assert pr.join(qi, pq, fl, KEPT | 2) == [(0, 1)]                # every bit of require
    assert pr.join(qi[:0], pq, fl, KEPT) == [] and pr.join(qi, pq[:0], fl[:0], KEPT) == []
    # rows and link records: frames 0 (carried keyframe), 1 (keyframe 0), 2 (not saved), 3 (keyframe 1)
    prev = [pr.KF_CARRIED, 0, pr.KF_NOT_SAVED, 1]
    pose = np.zeros(4, [("R", "<f8", (9,)), ("t", "<f8", (3,))])
    pose["R"][0] = pose["R"][1] = np.eye(3).reshape(9)
    pose["t"][1] = (0.0, 0.0, 1.0)
    pts = np.zeros((4, 5), [("X", "<f8", (3,))])
    pts["X"][1] = np.arange(15).reshape(5, 3)
    matches = [pq[:0], pq, pq[:0], qi]
    flags = [fl[:0], fl, fl[:0], fl]
    xy2 = [np.zeros((0, 2), np.float32), np.zeros((5, 2), np.float32), np.zeros((0, 2), np.float32), np.arange(10, dtype=np.float32).reshape(5, 2)]
    X, xy, L = pr.link_rows(3, prev, matches, pose, pts, flags, xy2, KEPT)
    assert (int(L["q"]), int(L["p"]), int(L["n_linked"]), int(L["flags"])) == (1, 0, 3, 0)
    assert X.tolist() == pts["X"][1][[1, 2, 4]].tolist() and xy.tolist() == xy2[3][[0, 1, 2]].tolist()
    X, xy, L = pr.link_rows(0, prev, matches, pose, pts, flags, xy2, KEPT)
    assert (int(L["q"]), int(L["p"]), int(L["n_linked"]), int(L["flags"])) == (pr.KF_CARRIED, pr.KF_CARRIED, 0, pr.NO_MAP) and len(X) == 0
    X, xy, L = pr.link_rows(2, prev, matches, pose, pts, flags, xy2, KEPT)
    assert (int(L["q"]), int(L["n_linked"]), int(L["flags"])) == (pr.KF_NOT_SAVED, 0, 0) and len(X) == 0
    X, xy, L = pr.link_rows(1, prev, matches, pose, pts, flags, xy2, KEPT)      # keyframe 0's own pair is the carried one: no map in this launch ...
    assert (int(L["q"]), int(L["p"]), int(L["n_linked"])) == (0, pr.KF_CARRIED, 0)   # ... and here it has rows but none that frame 1's list meets
    # the relative motion: R = Rz(90) after R_pq = I, t_pq = e_z
    rec = pr.zero_record()
    rec["best_iter"], rec["R"], rec["t"] = 0, [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0]
    _, _, L = pr.link_rows(3, prev, matches, pose, pts, flags, xy2, KEPT)
    M = pr.link_motion(L, rec, pose[1])
    assert M["R_rel"].tolist() == rec["R"].tolist() and M["t_rel"].tolist() == [1.0, 2.0, 2.0] and float(M["scale"]) == 3.0
    rec["best_iter"] = -1
    assert pr.link_motion(L, rec, pose[1]).tobytes() == L.tobytes()
