"""CPU: the restatement of the two-view polish (tests/essential_polish_ref.py) on its own -- no device, and no entry point of the library.

Scenes: essential_refine_ref.make_scene, the five classes x M 8 / 49 / 300 x noise 0.3 / 1.0 px x 0 / 25 % of the second image's pixels replaced,
12 seeds a cell, EuRoC intrinsics.  Every start is the CPU oracle's RANSAC winner at 1 px (orc_essential_ransac + orc_recover_pose) and set 0 is its
mask; the defaults (three re-selections at 2 px, five steps a round), min_inliers 6 at M 8 as in tests/test_essential_refine_ref.py.

Asserted.  rounds = 0 on every scene of at most 64 points: R, t, E, cost0, cost1, best_step are essential_refine_ref.refine's byte for byte.
On every run: cost1 <= cost0, n_set_last >= min_inliers unless FEW, the mask is the last set adopted and has n_set_last bytes set, and where the
rounds ended on an equal set the mask IS the selection under the reported pose.  At 1 px, per moving class over M 49 and 300, both outlier shares
and 12 seeds (48 runs), the median rotation and the median direction error are below the ONE-SET refinement's on the same starts; at 0.3 px both
are below the RANSAC winner's.  rounds = 8 keeps R a rotation and t a unit vector to rounding.  SHRANK, FEW and the equal-set stop on a
noise-free scene, from the record's own fields.  M 8, static and dup cells are printed, not bounded."""
import numpy as np
import pytest

import essential_polish_ref as epr
import essential_refine_ref as er
import oracle_bind as orc
import pose_degenerate_cases as pdc
import vislam

CAM = er.Camera()
SIZES, NOISES, OUTLIERS, SEEDS = (8, 49, 300), (0.3, 1.0), (0.0, 0.25), 12


def oracle_params():
    p = vislam.default_params()
    p.fx = p.fy = pdc.FOCAL
    p.cx, p.cy = pdc.CX, pdc.CY
    return p


def params_for(m, rounds=3):
    ep, eq = epr.default_params(), er.default_params()
    ep.rounds = rounds
    if m == 8:
        ep.min_inliers = eq.min_inliers = 6
    return ep, eq


def start_of(p, x1, x2):
    E, mask, _, _ = orc.essential_ransac(p, x1, x2)
    R, t, _ = orc.recover_pose(p, E, x1, x2)
    return R.reshape(9), t, mask


@pytest.fixture(scope="module")
def runs():
    """{(cls, m, noise, outliers, seed): dict}: scene, start, the polished record with its mask and sets, the one-set record -- computed once"""
    p = oracle_params()
    out = {}
    for cls in er.CLASSES:
        for m in SIZES:
            for nz in NOISES:
                for ol in OUTLIERS:
                    for seed in range(SEEDS):
                        x1, x2, Rt, tt = er.make_scene(cls, m, nz, ol, seed)
                        R0, t0, mask = start_of(p, x1, x2)
                        ep, eq = params_for(m)
                        sets = []
                        rec, mo, pose = epr.polish(CAM, ep, R0, t0, x1, x2, mask, None, sets)
                        out[(cls, m, nz, ol, seed)] = dict(x1=x1, x2=x2, Rt=Rt, tt=tt, R0=R0, t0=t0, mask=mask, rec=rec, mo=mo, pose=pose, sets=sets,
                                                           one=er.refine(CAM, eq, R0, t0, x1, x2, mask))
    return out


def errors(run, R, t):
    return er.rot_err_deg(np.reshape(R, (3, 3)), run["Rt"]), er.dir_err_deg(t, run["tt"])


def test_tiled_sums_equal_the_one_wave_sums_up_to_64_points_and_are_restored():
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, 63, 64):
        terms = rng.normal(0, 1, (n, 21)) * 10.0 ** rng.integers(-8, 8, (n, 21))
        assert np.array(epr.tiled_sums(terms)).tobytes() == np.array(er.pr.wave_sums(terms)).tobytes(), n
    terms = rng.normal(0, 1, (65, 3))
    terms[64] = 1e-30                                              # point 64: lane 0 of the one-wave order, wave 1 of the tiled one
    assert np.abs(np.array(epr.tiled_sums(terms)) - terms.sum(0)).max() < 1e-13
    keep = er.pr.wave_sums
    with epr.tiled():
        assert er.pr.wave_sums is epr.tiled_sums
    assert er.pr.wave_sums is keep
    # a term of -0.0 alone: the partial sum starts at +0.0, so the total is +0.0 under both contracts
    z = np.full((3, 1), -0.0)
    assert np.signbit(epr.tiled_sums(z)[0]) == np.signbit(er.pr.wave_sums(z)[0]) == False  # noqa: E712


def test_rounds_0_is_the_one_set_refinement_byte_for_byte(runs):
    n = 0
    for key, run in runs.items():
        if key[1] > 64:
            continue
        ep, eq = params_for(key[1], rounds=0)
        rec, mo, pose = epr.polish(CAM, ep, run["R0"], run["t0"], run["x1"], run["x2"], run["mask"])
        one = run["one"]
        if int(one["flags"]) == er.NO_POSE:
            assert rec.tobytes() == epr.zero_record().tobytes() and mo is None, key
            continue
        for f in ("R", "t", "E", "cost0", "cost1", "best_step"):
            assert rec[f].tobytes() == one[f].tobytes(), (key, f)
        assert int(rec["n_set_first"]) == int(rec["n_set_last"]) == int(one["n_used"]) and int(rec["steps_run"]) == int(one["steps_run"]), key
        assert float(rec["cost_first"]) == float(rec["cost0"]) and int(rec["n_changed"]) == 0 and int(rec["rounds_run"]) == (0 if int(rec["flags"]) & epr.FEW else 1), key
        assert (mo != 0).tobytes() == (run["mask"] != 0).tobytes(), key
        n += 1
    assert n >= 400, n


def test_invariants_of_every_run(runs):
    flags, stops = {}, dict(equal=0, shrank=0, rounds=0)
    for key, run in runs.items():
        rec, mo, sets = run["rec"], run["mo"], run["sets"]
        ep, _ = params_for(key[1])
        f = int(rec["flags"])
        flags[f] = flags.get(f, 0) + 1
        if f == epr.NO_POSE:
            assert rec.tobytes() == epr.zero_record().tobytes() and mo is None and run["pose"]["R"].tobytes() == np.asarray(run["R0"], np.float64).tobytes(), key
            continue
        assert float(rec["cost1"]) <= float(rec["cost0"]), key
        assert int(rec["n_points"]) == key[1] and int(rec["n_set_first"]) == int((run["mask"] != 0).sum()), key
        assert int(mo.sum()) == int(rec["n_set_last"]) and set(np.unique(mo)) <= {0, 1}, key
        assert (mo != 0).tobytes() == sets[-1].tobytes() and len(sets) == max(int(rec["rounds_run"]), 1), key
        if f & epr.FEW:
            assert int(rec["n_set_first"]) < ep.min_inliers and int(rec["rounds_run"]) == 0 and int(rec["steps_run"]) == 0 and not f & ~epr.FEW, key
            continue
        assert int(rec["n_set_last"]) >= ep.min_inliers, key
        assert bool(f & epr.POLISHED) != bool(f & epr.REJECTED) and 1 <= int(rec["rounds_run"]) <= ep.rounds + 1, key
        a, b = er.pr.normalise(CAM, run["x1"])
        c, d = er.pr.normalise(CAM, run["x2"])
        thr = np.float64(ep.select_px) / np.float64(CAM.fx)
        sel = epr.select(CAM, [np.float64(v) for v in rec["R"]], [np.float64(v) for v in rec["t"]], a, b, c, d, thr * thr)
        if f & epr.SHRANK:
            stops["shrank"] += 1
            assert int(sel.sum()) < ep.min_inliers and int(rec["n_changed"]) == int((sel != (mo != 0)).sum()) > 0, key
        elif int(rec["rounds_run"]) <= ep.rounds:                      # ended before the last round: on an equal set
            stops["equal"] += 1
            assert int(rec["n_changed"]) == 0 and sel.tobytes() == (mo != 0).tobytes(), key
        else:
            stops["rounds"] += 1
            assert int(rec["n_changed"]) > 0, key
        # the pose record: the reported pose, the last set's size, the rest of the input record
        q = run["pose"]
        assert q["R"].tobytes() == rec["R"].tobytes() and q["t"].tobytes() == rec["t"].tobytes() and q["E"].tobytes() == rec["E"].tobytes(), key
        assert int(q["n_inliers"]) == int(rec["n_set_last"]) and int(q["n_points"]) == key[1], key
        R, t = rec["R"].reshape(3, 3), rec["t"]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and abs(np.linalg.norm(t) - 1.0) < 1e-14, key
    print("\nflags -> runs:", dict(sorted(flags.items())), "  how the rounds ended:", stops)
    assert flags.get(epr.POLISHED, 0) > len(runs) // 2 and stops["equal"] > 0 and stops["rounds"] > 0


def _medians(runs, cls, nz, sizes):
    w, o, p = [], [], []
    for key, run in runs.items():
        if key[0] == cls and key[2] == nz and key[1] in sizes:
            w.append(errors(run, run["R0"], run["t0"] / np.linalg.norm(run["t0"])))
            o.append(errors(run, run["one"]["R"], run["one"]["t"]))
            p.append(errors(run, run["rec"]["R"], run["rec"]["t"]))
    return [np.median(np.array(v), 0) for v in (w, o, p)], len(w)


def test_medians_beat_the_one_set_refinement_at_one_pixel_and_the_winner_at_a_third(runs):
    print()
    for cls in er.MOVING:
        for nz in NOISES:
            for m in SIZES:
                for ol in OUTLIERS:
                    sel = {k: v for k, v in runs.items() if k[3] == ol}
                    (w, o, p), n = _medians(sel, cls, nz, (m,))
                    print(f"{cls} noise {nz} M {m} outliers {ol}: median rotation / direction error in degrees   winner {w[0]:.3f} {w[1]:.2f}   "
                          f"refined {o[0]:.3f} {o[1]:.2f}   polished {p[0]:.3f} {p[1]:.2f}")
            (w, o, p), n = _medians(runs, cls, nz, (49, 300))
            print(f"{cls} noise {nz}, M 49 and 300, {n} runs: winner {w[0]:.3f} {w[1]:.2f}   refined {o[0]:.3f} {o[1]:.2f}   polished {p[0]:.3f} {p[1]:.2f}")
            assert n == 48
            if nz == 1.0:
                assert p[0] < o[0] and p[1] < o[1], (cls, nz, o, p)
            else:
                assert p[0] < w[0] and p[1] < w[1], (cls, nz, w, p)


def test_printed_only_cells(runs):
    print()
    for cls in ("static", "dup"):
        for nz in NOISES:
            sel = [run for key, run in runs.items() if key[0] == cls and key[2] == nz]
            fl = sorted({int(run["rec"]["flags"]) for run in sel})
            print(f"{cls} noise {nz}: {len(sel)} runs, flags {fl}, median n_set_first -> n_set_last "
                  f"{np.median([int(r['rec']['n_set_first']) for r in sel]):.0f} -> {np.median([int(r['rec']['n_set_last']) for r in sel]):.0f}")


def test_8_rounds_keep_a_rotation_and_a_unit_vector(runs):
    worst = [0.0, 0.0]
    for cls in er.MOVING:
        for m in (49, 300):
            run = runs[(cls, m, 1.0, 0.25, 0)]
            ep, _ = params_for(m, rounds=8)
            rec, mo, _ = epr.polish(CAM, ep, run["R0"], run["t0"], run["x1"], run["x2"], run["mask"])
            R = rec["R"].reshape(3, 3)
            worst = [max(worst[0], float(np.abs(R.T @ R - np.eye(3)).max())), max(worst[1], abs(float(np.linalg.norm(rec["t"])) - 1.0))]
            assert float(rec["cost1"]) <= float(rec["cost0"]) and int(rec["rounds_run"]) <= 9 and int(rec["steps_run"]) <= 45
            assert int(rec["n_set_last"]) >= ep.min_inliers and int(mo.sum()) == int(rec["n_set_last"])
    print(f"\nafter up to 9 rounds of 5 steps: |R^T R - I| {worst[0]:.1e}, ||t| - 1| {worst[1]:.1e}")
    assert worst[0] < 45 * 16 * 2.0 ** -52 and worst[1] < 4 * 2.0 ** -52    # a rounding or two per step (45 at the most); the norm is renewed every step


def test_equal_set_stop_shrank_and_few():
    p = oracle_params()
    x1, x2, Rt, tt = er.make_scene("general", 49, 0.0, 0.0, 0)
    R0, t0, mask = start_of(p, x1, x2)
    ep = epr.default_params()
    # noise-free: every point is in the winner's mask and every point passes at 2 px under the refined pose -- the first selection changes nothing
    rec, mo, pose = epr.polish(CAM, ep, R0, t0, x1, x2, mask)
    assert int(rec["n_set_first"]) == 49 == int(rec["n_set_last"]) and int(rec["n_changed"]) == 0 and int(rec["rounds_run"]) == 1
    assert int(rec["flags"]) in (epr.POLISHED, epr.REJECTED) and int(rec["steps_run"]) <= 5 and mo.all()
    assert float(rec["cost_first"]) == float(rec["cost0"]) >= float(rec["cost1"])
    # ... and rounds = 0 gives the same record: the selection that changed nothing left no trace but n_changed = 0
    ep0 = epr.default_params()
    ep0.rounds = 0
    assert epr.polish(CAM, ep0, R0, t0, x1, x2, mask)[0].tobytes() == rec.tobytes()
    # SHRANK: at 1 px of noise a selection at a millionth of a pixel keeps next to nothing; the earlier set and pose stay
    x1, x2, Rt, tt = er.make_scene("general", 49, 1.0, 0.0, 1)
    R0, t0, mask = start_of(p, x1, x2)
    tiny = epr.default_params()
    tiny.select_px = 1e-6
    rec, mo, pose = epr.polish(CAM, tiny, R0, t0, x1, x2, mask)
    one = epr.polish(CAM, ep0, R0, t0, x1, x2, mask)[0]
    assert int(rec["flags"]) & epr.SHRANK and int(rec["rounds_run"]) == 1 and int(rec["n_changed"]) > 0 and int(rec["n_set_last"]) == int(rec["n_set_first"])
    assert (mo != 0).tobytes() == (mask != 0).tobytes() and int(pose["n_inliers"]) == int(rec["n_set_first"])
    for f in ("R", "t", "E", "cost_first", "cost0", "cost1", "best_step", "steps_run"):
        assert rec[f].tobytes() == one[f].tobytes(), f
    # FEW: seven points in set 0; the start is reported, t normalised, the mask is set 0
    few = np.zeros(49, np.uint8)
    few[:7] = 3
    rec, mo, pose = epr.polish(CAM, ep, R0, 3.0 * t0, x1, x2, few)
    assert int(rec["flags"]) == epr.FEW and int(rec["n_set_first"]) == 7 == int(rec["n_set_last"]) and int(rec["rounds_run"]) == 0 and int(rec["steps_run"]) == 0
    assert (rec["R"] == R0).all() and np.abs(rec["t"] - t0 / np.linalg.norm(t0)).max() < 1e-15 and float(rec["cost_first"]) == float(rec["cost0"]) == float(rec["cost1"])
    assert mo.tolist() == [1] * 7 + [0] * 42 and int(pose["n_inliers"]) == 7
    # NO_POSE: the zero record, the mask row left alone, the input record unchanged
    for R, t in ((np.zeros(9), t0), (np.where(np.arange(9) == 4, np.nan, R0), t0), (R0, np.zeros(3)), (R0, np.array([np.inf, 0.0, 0.0]))):
        rec, mo, pose = epr.polish(CAM, ep, R, t, x1, x2, mask)
        assert rec.tobytes() == epr.zero_record().tobytes() and mo is None
        assert pose["R"].tobytes() == np.asarray(R, np.float64).tobytes() and pose["t"].tobytes() == np.asarray(t, np.float64).tobytes() and int(pose["n_inliers"]) == 0
