"""CPU: the restatement of the homography polish (tests/homography_polish_ref.py) on its own -- no device, and no entry point of the library.

Asserted.  The analytic Jacobian against central differences of (ru, rv) in the nine entries of H; the solve and the strike of the gauge's row and
column against numpy's solver on the same normal equations; cost1 <= cost0 on every case of homography_pose_ref.table_cases(); a row of at most 64
points gives the same bytes under the one-wave order and the tiled one; the gauge with p != 8 (a start turned 90 degrees about the optical axis,
and a two-entry tie); noise-free planted planes stay at the truth; the rotation classes still decompose to a rotation; the accuracy of the chain
homography -> polish -> homography_pose against homography -> homography_pose on planted planes with a quarter of outliers; hostile rows."""
import numpy as np
import pytest

import homography_polish_ref as hq
import homography_pose_ref as hpr
import homography_ref as hr
import hostile_cases as hc

CAM = hr.Camera()
DRAWS = hr.make_draws(7)


def true_h(R, t, n):
    """R + t n^T of a planted plane (t in units of d), 9 doubles"""
    return (np.asarray(R, np.float64) + np.outer(t, n)).reshape(9)


def unit(H):
    H = [hq.F(v) for v in np.asarray(H, np.float64).reshape(9)]
    nn = np.sqrt(hq.norm2(H))
    return [h / nn for h in H]


def record_of(H, m):
    """a homography record that holds H as a winner would"""
    r = hr.zero_record()
    r["H"], r["best_iter"], r["n_points"] = H, 0, m
    return r


@pytest.fixture(scope="module")
def table():
    """{case: dict(x1, x2, rec, mask, out = polish(...), sets)} over homography_pose_ref.table_cases(), computed once"""
    out = {}
    hp, pq = hr.default_params(), hq.default_params()
    for case in hpr.table_cases():
        cls, m, nz, ol = case
        x1, x2, _ = hr.make_rows(cls, m, nz, ol)
        rec, mask = hr.homography(CAM, hp, x1, x2, DRAWS)
        sets = []
        out[case] = dict(x1=x1, x2=x2, rec=rec, mask=mask, out=hq.polish(CAM, pq, rec, x1, x2, mask, sets), sets=sets)
    return out


def test_jacobian_against_central_differences():
    h = 1e-6
    for seed in (0, 1, 2):
        R, t, n, x1, x2 = hpr.planted_plane(seed, 60, 0.5)
        H = unit(true_h(R, t, n))
        x, y, u2, v2 = hr.normalise(CAM, x1, x2)
        J0, J1 = hq.jacobian(H, x, y, u2, v2)
        for k in range(9):
            Hp, Hm = list(H), list(H)
            Hp[k], Hm[k] = H[k] + h, H[k] - h
            _, _, rup, rvp, _, _ = hq.residual(Hp, x, y, u2, v2)
            _, _, rum, rvm, _, _ = hq.residual(Hm, x, y, u2, v2)
            d0, d1 = (rup - rum) / (2 * h), (rvp - rvm) / (2 * h)
            scale = max(float(np.abs(J0[k]).max()), float(np.abs(J1[k]).max()))
            assert scale > 0 and float(np.abs(d0 - J0[k]).max()) <= 1e-6 * scale and float(np.abs(d1 - J1[k]).max()) <= 1e-6 * scale, (seed, k)


def test_sums_and_solve_against_numpy():
    """the 40 sums are the entries of J^T J, J^T r and r^T r; the step with entry p held is numpy's solution of the struck system"""
    R, t, n, x1, x2 = hpr.planted_plane(3, 300, 0.5)
    x, y, u2, v2 = hr.normalise(CAM, x1, x2)
    setmask = np.arange(300) % 7 != 0
    for turn in range(9):
        H = unit(true_h(R, t, n) + 0.01 * np.arange(9))
        H = unit([3.0 if k == turn else H[k] for k in range(9)])                  # entry `turn` is the largest: every gauge once
        J0, J1 = hq.jacobian(H, x, y, u2, v2)
        _, _, ru, rv, _, _ = hq.residual(H, x, y, u2, v2)
        J = np.concatenate([np.stack(J0, 1)[setmask], np.stack(J1, 1)[setmask]])
        r = np.concatenate([ru[setmask], rv[setmask]])
        S = hq.gn_sums(H, x, y, u2, v2, setmask, hq.epr.tiled_sums)
        A = np.array([[float(hq.entry(S, a, b)) for b in range(9)] for a in range(9)])
        g = np.array([float(S[hq.G + a]) for a in range(9)])
        assert np.abs(A - J.T @ J).max() <= 1e-12 * np.abs(A).max() and np.abs(g - J.T @ r).max() <= 1e-12 * (np.abs(J).T @ np.abs(r)).max()
        assert abs(float(S[hq.COST]) - float(r @ r)) <= 1e-12 * float(r @ r)
        p = hq.gauge(H)
        assert p == turn
        dH, ok = hq.solve(S, p)
        keep = [k for k in range(9) if k != p]
        want = np.linalg.solve((J.T @ J)[np.ix_(keep, keep)], -(J.T @ r)[keep])
        assert ok and float(dH[p]) == 0.0
        assert np.abs(np.array([float(dH[k]) for k in keep]) - want).max() <= 1e-7 * max(np.abs(want).max(), 1e-12), (turn, dH, want)


def test_cost_never_rises_and_the_invariants_of_every_case(table):
    flags = {}
    pq = hq.default_params()
    for case, run in table.items():
        rec, mo, ho = run["out"]
        f = int(rec["flags"])
        flags[f] = flags.get(f, 0) + 1
        if f == hq.NO_MODEL:
            assert int(run["rec"]["best_iter"]) < 0 and mo is None and ho.tobytes() == run["rec"].tobytes(), case
            continue
        assert float(rec["cost1"]) <= float(rec["cost0"]), case
        assert int(rec["n_points"]) == case[1] and int(rec["n_set_first"]) == int(run["mask"].sum()) == int(run["rec"]["n_inliers"]), case
        assert int(mo.sum()) == int(rec["n_set_last"]) == int(ho["n_inliers"]) and set(np.unique(mo)) <= {0, 1}, case
        assert (mo != 0).tobytes() == run["sets"][-1].tobytes() and len(run["sets"]) == max(int(rec["rounds_run"]), 1), case
        H = rec["H"]
        assert np.isfinite(H).all() and abs(float(np.linalg.norm(H)) - 1.0) < 1e-15 and float(np.linalg.det(H.reshape(3, 3))) >= 0.0, case
        assert ho["H"].tobytes() == H.tobytes(), case
        for k in ("score_h", "score_e", "model", "best_iter", "n_degenerate", "n_inliers_e", "n_points"):
            assert ho[k] == run["rec"][k], (case, k)
        if f & hq.FEW:
            assert int(rec["n_set_first"]) < pq.min_inliers and int(rec["rounds_run"]) == 0 and int(rec["steps_run"]) == 0, case
            continue
        assert bool(f & hq.POLISHED) != bool(f & hq.REJECTED) and 1 <= int(rec["rounds_run"]) <= pq.rounds + 1, case
        assert int(rec["n_set_last"]) >= pq.min_inliers, case
    print("\nflags -> cases:", dict(sorted(flags.items())))
    assert flags.get(hq.POLISHED, 0) > len(table) // 2


def test_short_rows_give_the_same_bytes_in_the_one_wave_order(table):
    n = 0
    pq = hq.default_params()
    for case, run in table.items():
        if case[1] > 64:
            continue
        rec, mo, ho = hq.polish(CAM, pq, run["rec"], run["x1"], run["x2"], run["mask"], None, hq.one_wave_sums)
        assert rec.tobytes() == run["out"][0].tobytes() and ho.tobytes() == run["out"][2].tobytes(), case
        assert (mo is None and run["out"][1] is None) or mo.tobytes() == run["out"][1].tobytes(), case
        n += int(bool(int(rec["flags"]) & hq.POLISHED))
    assert n >= 12, n
    # ... and a longer row does not: the orders differ from point 64 on
    rng = np.random.default_rng(5)
    terms = rng.normal(0, 1, (300, hq.SUMS))
    assert np.array(hq.epr.tiled_sums(terms)).tobytes() != np.array(hq.one_wave_sums(terms)).tobytes()
    terms = rng.normal(0, 1, (64, hq.SUMS)) * 10.0 ** rng.integers(-8, 8, (64, hq.SUMS))
    assert np.array(hq.epr.tiled_sums(terms)).tobytes() == np.array(hq.one_wave_sums(terms)).tobytes()


def _turned(seed, m, noise, scale):
    """a planted plane whose second image is turned 90 degrees about the optical axis and zoomed by `scale`: (Ht, x1, x2)"""
    R, t, n, x1, x2 = hpr.planted_plane(seed, m, 0.0)
    x, y, u2, v2 = hr.normalise(CAM, x1, x2)
    rng = np.random.default_rng([17, seed])
    a, b = scale * -v2, scale * u2
    px = np.stack([a * CAM.fx + CAM.cx, b * CAM.fx + CAM.cy], 1) + rng.normal(0, noise, (m, 2))
    T = np.array([[0.0, -scale, 0.0], [scale, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return (T @ true_h(R, t, n).reshape(3, 3)).reshape(9), x1, np.ascontiguousarray(px, np.float32)


def test_the_gauge_away_from_the_last_entry():
    pq = hq.default_params()
    # a start turned 90 degrees about the optical axis: the largest entries are H1 and H3
    for seed in (0, 1, 2):
        Ht, x1, x2 = _turned(seed, 120, 0.3, 1.5)
        start = unit(np.asarray(Ht) + 2e-3 * np.array([1, -1, 1, 1, -1, 1, -1, 1, 1.0]))
        p = hq.gauge(start)
        assert p in (1, 3), p
        sets = []
        rec, mo, _ = hq.polish(CAM, pq, record_of(start, 120), x1, x2, None, sets)
        # the cost falls to the noise's: 2 m residuals of variance (0.3 / fx)^2, eight of them fitted away; half as much again is the margin
        floor = 2 * 120 * (0.3 / CAM.fx) ** 2
        assert int(rec["flags"]) == hq.POLISHED and float(rec["cost1"]) < 1.5 * floor < 0.5 * float(rec["cost_first"]), (seed, rec, floor)
        assert hq.gauge([hq.F(v) for v in rec["H"]]) == p and hr.unit_diff(rec["H"], Ht) < 0.2 * hr.unit_diff(start, Ht), seed
    # a two-entry tie: |H1| == |H3| exactly, both the largest -> the lowest index is held
    H = [hq.F(v) for v in (0.0, -2.0 / 3.0, 0.0, 2.0 / 3.0, 0.0, 0.0, 0.0, 0.0, 1.0 / 3.0)]
    assert abs(H[1]) == abs(H[3]) and hq.gauge(H) == 1 and hq.gauge([-h for h in H]) == 1 and float(hq.norm2(H)) == 1.0
    assert hq.gauge([hq.F(v) for v in (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)]) == 0 and hq.gauge([hq.F(v) for v in (0, 0, 0, 0, 0, 0, 0, 0, 1.0)]) == 8
    rng = np.random.default_rng(3)
    x1 = np.stack([rng.uniform(50, 700, 80), rng.uniform(40, 440, 80)], 1).astype(np.float32)
    x, y, _, _ = hr.normalise(CAM, x1, x1)
    px = np.stack([(2.0 * -y) * CAM.fx + CAM.cx, (2.0 * x) * CAM.fx + CAM.cy], 1) + rng.normal(0, 0.3, (80, 2))
    x2 = np.ascontiguousarray(px, np.float32)
    S = hq.gn_sums(H, *hr.normalise(CAM, x1, x2), np.ones(80, bool), hq.epr.tiled_sums)
    dH, ok = hq.solve(S, 1)
    assert ok and float(dH[1]) == 0.0 and all(float(dH[k]) != 0.0 for k in range(9) if k != 1)
    rec, mo, _ = hq.polish(CAM, pq, record_of(H, 80), x1, x2)
    assert int(rec["flags"]) & (hq.POLISHED | hq.REJECTED) and float(rec["cost1"]) <= float(rec["cost0"]) and hr.unit_diff(rec["H"], H) < 1e-3


def test_noise_free_planes_stay_at_the_truth():
    hp, pq = hr.default_params(), hq.default_params()
    worst = 0.0
    for seed in range(8):
        for m in (40, 300):
            R, t, n, x1, x2 = hpr.planted_plane(seed, m, 0.0)
            Ht = true_h(R, t, n)
            rec, mask = hr.homography(CAM, hp, x1, x2, DRAWS)
            out, mo, ho = hq.polish(CAM, pq, rec, x1, x2, mask)
            before, after = hr.unit_diff(rec["H"], Ht), hr.unit_diff(out["H"], Ht)
            worst = max(worst, after / before)
            assert after <= before, (seed, m, before, after)
            assert int(out["flags"]) in (hq.POLISHED, hq.REJECTED) and int(out["n_set_first"]) == m == int(out["n_set_last"]) and mo.all(), (seed, m, out)
            assert int(out["n_changed"]) == 0 and int(out["rounds_run"]) == 1 and float(out["cost1"]) <= float(out["cost_first"]), (seed, m, out)
    print(f"\nnoise-free: the polished H's distance from the truth is at most {worst:.3f} of the four-point H's")


def test_rotation_classes_still_decompose_to_a_rotation(table):
    hqp = hpr.default_params()
    n = 0
    for case, run in table.items():
        if case[0] not in hpr.ROTATION_LIST or int(run["out"][0]["flags"]) & (hq.NO_MODEL | hq.FEW):
            continue
        before = hpr.hpose(CAM, hqp, run["rec"], run["x1"], run["x2"], run["mask"])
        after = hpr.hpose(CAM, hqp, run["out"][2], run["x1"], run["x2"], run["out"][1])
        assert int(before["kind"]) == hpr.HP_ROTATION == int(after["kind"]), (case, float(before["t_norm"]), float(after["t_norm"]))
        n += 1
    assert n == 32, n


def _chain_errors(noise, m=300, seeds=40):
    """median (rotation, translation direction, normal) errors in degrees of the unrefitted and of the polished chain"""
    hp, hqp, pq = hr.default_params(), hpr.default_params(), hq.default_params()
    plain, polished = [], []
    for seed in range(seeds):
        R, t, n, x1, x2 = hpr.planted_plane(seed, m, noise)
        k = m // 4
        rng = np.random.default_rng([99, seed, m])
        x2 = x2.copy()
        x2[:k] = np.stack([rng.uniform(0, hr.W_PX, k), rng.uniform(0, hr.H_PX, k)], 1).astype(np.float32)
        rec, mask = hr.homography(CAM, hp, x1, x2, DRAWS)
        out, mo, ho = hq.polish(CAM, pq, rec, x1, x2, mask)
        assert int(out["flags"]) & hq.POLISHED, (noise, seed, out)
        rot = R.T.astype(np.float32)
        for H, sel, into in ((rec, mask != 0, plain), (ho, mo != 0, polished)):
            r = hpr.hpose(CAM, hqp, H, x1[sel], x2[sel], None, rot)        # the voters alone: the same votes as the whole row under its mask
            assert int(r["kind"]) == hpr.HP_PLANE, (noise, seed)
            into.append(hpr.truth_errors((r["R"], r["t"], r["n"]), (R, t, n))[:3])
    return np.median(np.array(plain), 0), np.median(np.array(polished), 0)


@pytest.mark.parametrize("noise", [0.3, 1.0])
def test_the_polished_chain_halves_the_pose_errors(noise):
    plain, polished = _chain_errors(noise)
    print(f"\nnoise {noise} px, m 300, 25 % outliers, 40 seeds: median rotation / translation direction / normal error in degrees   "
          f"unrefitted {plain[0]:.3f} / {plain[1]:.2f} / {plain[2]:.2f}   polished {polished[0]:.3f} / {polished[1]:.2f} / {polished[2]:.2f}")
    assert (polished <= 0.5 * plain).all(), (noise, plain, polished)


def test_hostile_rows():
    pq = hq.default_params()
    rows, clean = hc.h_rows()
    seen = dict(no_model=0, polished=0, rows=0)
    for (kind, lay), row in rows.items():
        rec, mo, ho = hq.polish(CAM, pq, row["rec"], row["p1"], row["p2"], row["mask"])
        seen["rows"] += 1
        if int(rec["flags"]) == hq.NO_MODEL:
            seen["no_model"] += 1
            assert int(row["rec"]["best_iter"]) < 0 and mo is None and rec.tobytes() == hq.zero_record().tobytes(), (kind, lay)
            continue
        assert np.isfinite(rec["H"]).all() and abs(float(np.linalg.norm(rec["H"])) - 1.0) < 1e-12, (kind, lay, rec)
        bad = ~(np.isfinite(row["p1"]).all(1) & np.isfinite(row["p2"]).all(1))
        assert not mo[bad].any(), (kind, lay, np.flatnonzero(mo[bad]))
        if kind in hc.PAIR_NEVER:
            assert not mo[row["idx"]].any(), (kind, lay)
        assert int(mo.sum()) == int(rec["n_set_last"]) and float(rec["cost1"]) <= float(rec["cost0"]), (kind, lay, rec)
        seen["polished"] += int(bool(int(rec["flags"]) & hq.POLISHED))
    print("\nhostile rows:", seen)
    assert seen["rows"] == 64 + 3 * len(hc.mag_pair_kinds()) and seen["no_model"] >= 10 and seen["polished"] >= 30, seen     # (+ the magnitude ladder)
    # a non-finite point that the caller's mask puts INTO set 0 adds nothing to a sum whose iw, u or v it spoils, and the first re-selection drops it
    m = hc.M
    base = hc.h_base(m)
    rec, mask = clean[m]
    for kind in ("p1:nan", "p1:pinf", "both:inf_all", "p2:nan", "p2:ninf"):
        h = hc.hostile(kind, base, np.array([1, 7]))
        forced = mask.copy()
        forced[[1, 7]] = 1
        out, mo, _ = hq.polish(CAM, pq, rec, h["p1"], h["p2"], forced)
        assert np.isfinite(out["H"]).all() and int(out["rounds_run"]) >= 2 and not mo[[1, 7]].any(), (kind, out)
