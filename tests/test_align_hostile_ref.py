"""CPU: the candidate window of the patch builders and of the alignment on hostile matched points (tests/align_hostile_cases.py).

  - oracle/gradient.cpp's orc_patch_points equals the rule of include/vislam_hip.h restated with integers and fractions, on all five
    levels, for clean keypoints and for every hostile value in x, in y and in both -- and returns (the loop it replaced did not, for a
    coordinate of +inf or of 2^31 and more);
  - for keypoints inside [-2^20, 2^20] the oracle's rows are the bytes the oracle gave before the rule was written down
    (tests/golden/patch_points_rows.npz: nothing changed for usable inputs);
  - csrc/patch_window.h, the helper both kernels share, walked by host/patch_window_check.cpp under the sanitizers;
  - the conditions that keep tests/test_align_hostile_gpu.py from passing vacuously hold on the oracle for the chosen frames."""
import os
import subprocess

import numpy as np
import pytest

import align_hostile_cases as ahc
import hostile_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kp(vislam, xy):
    kp = np.zeros(len(xy), vislam.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    return kp


def _same_lists(vislam, orc, xy, w, h, where):
    for l in range(5):
        got, want = orc.patch_points(_kp(vislam, xy), w, h, l), ahc.patch_rule(xy, w, h, l)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (where, l, got.shape, want.shape)


def test_oracle_equals_the_rule_on_clean_keypoints(vislam, orc):
    _same_lists(vislam, orc, ahc.points()[1], ahc.W, ahc.H, "clean")
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(-12, ahc.W + 12, 200), rng.uniform(-12, ahc.H + 12, 200)], 1).astype(np.float32)   # windows clipped on every side
    xy[:40] = np.round(xy[:40] * 2) / 2                                                                            # integer and .5 coordinates
    _same_lists(vislam, orc, xy, ahc.W, ahc.H, "clipped")


@pytest.mark.parametrize("lay", ("stride5", "all", "wave_edges"))
def test_oracle_equals_the_rule_on_every_hostile_kind(vislam, orc, lay):
    base, idx = ahc.points()[1], ahc.layout(lay)
    for kind in ahc.kinds():
        _same_lists(vislam, orc, ahc.apply_kind(kind, base, idx), ahc.W, ahc.H, (kind, lay))


def test_hostile_values_by_the_rule():
    """what the GPU suite relies on: on the levels the alignment runs (3 ... 0) every hostile value has an empty window, except w + 40 /
    h + 40, whose level-3 window (5 wide around 24.6 / 19.6) reaches the last column / row -- ahc.contributes says so"""
    for name in ahc.coordinate_values():
        for size, axis in ((ahc.W, "x"), (ahc.H, "y")):
            v = ahc.coordinate_values(size)[name]
            spans = [ahc.exact_span(ahc.level_coordinate(v, l), ahc.PATCH_SIZE[l], size >> l) for l in range(4)]
            assert any(s is not None for s in spans) == ahc.contributes(f"{axis}:{name}"), (name, axis, spans)
    assert [k for k in ahc.kinds() if ahc.contributes(k)] == ["x:w+40", "y:w+40", "xy:w+40"]


def test_usable_inputs_give_the_rows_recorded_before_the_rule(vislam, orc):
    g = np.load(os.path.join(ROOT, "tests", "golden", "patch_points_rows.npz"))
    for name in ("uniform320", "clipped160"):
        xy, w, h = g[f"{name}_xy"], int(g[f"{name}_wh"][0]), int(g[f"{name}_wh"][1])
        assert np.abs(xy).max() <= 2 ** 20
        for l in range(5):
            got = orc.patch_points(_kp(vislam, xy), w, h, l)
            assert got.tobytes() == g[f"{name}_L{l}"].tobytes(), (name, l, got.shape)
            # the fixture can be derived again: the loop as it was, walked in Python where it ends and its casts are representable
            assert ahc.old_loop_rows(xy, w, h, l).tobytes() == g[f"{name}_L{l}"].tobytes(), (name, l)
        _same_lists(vislam, orc, xy, w, h, name)
    # the first list is the one tests/test_align_gpu.py::test_align_batch_explicit_points_and_init draws
    rng = np.random.default_rng(0)
    pts = np.zeros((3, 230, 2), np.float32)
    pts[..., 0] = rng.uniform(-2, 320 + 2, (3, 230)); pts[..., 1] = rng.uniform(-2, 240 + 2, (3, 230))
    assert pts[1].tobytes() == g["uniform320_xy"].tobytes()


def test_shared_helper_under_the_sanitizers(built):
    exe = os.path.join(ROOT, "vi-slam_amd", "lib", "patch_window_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "patch_window_check passed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stdout + r.stderr, r.stderr[-2000:]
    if "(address + undefined sanitizers)" not in r.stdout:
        pytest.skip("this g++ has no static sanitizer runtimes: the helper was walked and compared with the rule, but without a sanitizer")


@pytest.mark.parametrize("lay", ("first", "stride5", "wave_edges"))
def test_oracle_record_of_a_hostile_row_is_the_one_of_the_row_without_it(vislam, orc, lay):
    """the property the GPU suite asserts of the device, on the oracle: keypoints that contribute no candidate may as well be deleted"""
    t, idx = 1, ahc.layout(lay)
    base = ahc.points()[t]
    row, count = ahc.deleted(base, idx)
    short = ahc.oracle_pair(vislam, orc, t, row, count)
    assert np.isfinite(short["pose"]).all() and (short["n_residuals"][:4] > 0).all()
    for kind in ahc.kinds():
        rec = ahc.oracle_pair(vislam, orc, t, ahc.apply_kind(kind, base, idx), ahc.MAX_PTS)
        assert (rec.tobytes() == short.tobytes()) == (not ahc.contributes(kind)), (kind, lay, rec["n_residuals"], short["n_residuals"])


def test_vacuity_guards_hold_on_the_oracle(vislam, orc):
    """Before any GPU run, on the oracle (identity weights) and its numpy restatement (Tukey): every hostile case of
    tests/test_align_hostile_gpu.py either meets a guard -- residuals on every level the alignment runs, or two or more iterations on
    level 0 -- or is named in align_hostile_cases.EXCEPT_*, and those lists name nothing else.  Every clean pair and every "every fifth"
    pair keeps residuals on every level; at least half of the hostile pairs run two or more iterations on level 0."""
    pts = ahc.points()
    for mode in (0, 1):
        two_plus, total, unmet = 0, 0, set()
        for t in range(1, ahc.N_FRAMES):
            clean = ahc.oracle_pair(vislam, orc, t, pts[t], ahc.MAX_PTS, mode=mode)
            assert (clean["n_residuals"][:4] > 0).all(), (mode, t, clean["n_residuals"])
            for lay in ahc.INSIDE_LAYOUTS:
                row, count = ahc.deleted(pts[t], ahc.layout(lay))
                rec = ahc.oracle_pair(vislam, orc, t, row, count, mode=mode)
                if not ahc.meets_a_guard(rec):
                    unmet.add(lay)
                    assert count == 0 and not rec["n_residuals"].any()
                    continue
                assert (rec["n_residuals"][:4] > 0).all(), (mode, t, lay, rec["n_residuals"])
                total += 1
                two_plus += int(rec["iterations"][0] >= 1)         # the index at which level 0 stopped: 1 = it ran twice
        assert unmet == set(ahc.EXCEPT_LAYOUTS), (mode, unmet)
        assert 2 * two_plus >= total, (mode, two_plus, total)


def test_vacuity_guards_of_the_hostile_poses(vislam, orc):
    """every hostile initial pose on every pair at INIT_COUNT matched points, both weightings: a guard, or one of the named exceptions --
    the poses with a NaN or an infinity in them, and three finite ones that leave nothing to align by plain arithmetic"""
    pts = ahc.points()
    allowed = set(ahc.EXCEPT_POSES) | set(ahc.EXCEPT_FINITE_POSES)
    names = [n for n, _ in ahc.hostile_inits(vislam, orc)]
    assert allowed <= set(names)
    for n in ahc.EXCEPT_POSES:
        assert not np.isfinite(dict(ahc.hostile_inits(vislam, orc))[n].as_array()).all(), n
    for n in ahc.EXCEPT_FINITE_POSES:
        assert np.isfinite(dict(ahc.hostile_inits(vislam, orc))[n].as_array()).all(), n
    for mode in (0, 1):
        unmet = {}
        for name, pose in ahc.hostile_inits(vislam, orc):
            met = [ahc.meets_a_guard(ahc.oracle_pair(vislam, orc, t, pts[t], ahc.INIT_COUNT, init=pose, mode=mode)) for t in range(1, ahc.N_FRAMES)]
            assert all(met) or not any(met), (mode, name, met)
            unmet[name] = not any(met)
        assert {n for n, u in unmet.items() if u} == allowed, (mode, unmet)


def test_vacuity_guards_of_the_hostile_candidate_rows(vislam, orc):
    """every candidate-row kind at both places, no initial pose, both weightings: a guard, or EXCEPT_ROWS (accepted rows whose inverse
    depth overflows the step).  After ONE iteration per level, where the pose never moves, every kind keeps residuals on every level."""
    import align_weighted_ref as ref
    (l0, gx, gy), (l1, _, _) = ahc.levels(vislam, orc, 0), ahc.levels(vislam, orc, 1)
    none = np.zeros((1, 2), np.float32)
    for mode in (0, 1):
        for place in ahc.LIST_PLACES:
            unmet = set()
            for kind in ahc.list_values():
                cand = ahc.hostile_list(kind, place)
                if not ahc.meets_a_guard(ahc.oracle_pair(vislam, orc, 1, none, 0, mode=mode, cand=cand)):
                    unmet.add(kind)
                one = ahc.record(ref.estimate_pose_features(orc, ahc.params(orc, 1), ahc.W, ahc.H, l0, l1, gx, gy, cand, None))
                assert (one["n_residuals"][:4] > 0).all(), (kind, place, one["n_residuals"])
                assert hc.same_record(one, ahc.record(orc.estimate_pose_features(ahc.params(orc, 1), ahc.W, ahc.H, l0, l1, gx, gy, cand, None))), (kind, place)
            assert unmet == set(ahc.EXCEPT_ROWS), (mode, place, unmet)
