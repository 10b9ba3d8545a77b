"""CPU: the numpy restatement of the weighted alignment (tests/align_weighted_ref.py) is a reference --
  - with identity weights it equals oracle/align.cpp's orc_estimate_pose_features bit for bit on every single-pair and generated case the
    GPU tests use (so the oracle's dealing of rows by residual index and the kernel's by candidate index do not reach these results);
  - its mode-1 weights with the default constants equal orc_tukey_weights bit for bit, its mode-2 medians a sort-based selection;
  - what the weights do to a pair with an occluder, measured with the restatement (the numbers DESIGN.md section 4.6 quotes)."""
import numpy as np
import pytest

import align_weighted_ref as ref
import align_weights_cases as awc


def test_identity_equals_the_oracle_on_every_gpu_case(vislam, orc, canvas):
    cases = awc.single_cases(vislam, orc, canvas)
    assert len(cases) >= 16
    for name, cs in cases.items():
        want = orc.estimate_pose_features(cs.params(orc), cs.w, cs.h, *cs.levels(), cs.init(orc))
        got = ref.estimate_pose_features(orc, cs.params(orc), cs.w, cs.h, *cs.levels(), cs.init(orc))
        try:
            awc.same(got, want)
        except AssertionError as e:
            raise AssertionError((name,) + e.args) from None
        assert sum(want.n_residuals) > 0, name
    g = awc.generated_case(vislam, orc, canvas)
    oap = orc.default_align_params()
    oap.fx, oap.fy, oap.cx, oap.cy = 200.0, 200.0, 160.0, 120.0
    for t, p in g["pairs"].items():
        lv = (p["gray1"], p["gray2"], p["gx"], p["gy"], p["cand"])
        awc.same(ref.estimate_pose_features(orc, oap, g["W"], g["H"], *lv), orc.estimate_pose_features(oap, g["W"], g["H"], *lv))


def _vectors():
    rng = np.random.default_rng(3)
    v = {f"random_{n}": rng.integers(-255, 256, n) for n in (1, 2, 3, 255, 256, 257, 24200)}
    v["narrow_24200"] = np.clip(np.rint(rng.normal(3, 6, 24200)), -255, 255)           # piled up around 0, like real residuals
    v["all_zero"] = np.zeros(100)                                                       # MAD = 0 -> 1
    v["all_minus_255"] = np.full(77, -255)
    v["all_plus_255"] = np.full(78, 255)
    v["most_equal"] = np.concatenate([np.full(60, 7), rng.integers(-255, 256, 40)])     # more than half of the values equal
    # half and half: the running count lands exactly on n / 2 at the first value, so `bin > n / 2` takes the second one (even n);
    # odd n: n / 2 rounds down and the larger half is taken at once
    v["half_even"] = np.concatenate([np.full(50, 10), np.full(50, 40)])
    v["half_odd_low"] = np.concatenate([np.full(51, 10), np.full(50, 40)])
    v["half_odd_high"] = np.concatenate([np.full(50, 10), np.full(51, 40)])
    v["half_even_signed"] = np.concatenate([np.full(50, -30), np.full(50, 200)])
    v["ends"] = np.concatenate([np.full(40, -255), np.full(41, 255)])
    return {k: rng.permutation(a).astype(np.float32) for k, a in v.items()}


def test_mode_1_weights_equal_the_oracle(orc):
    for name, r in _vectors().items():
        assert ref.tukey_weights(r, ref.W_TUKEY).tobytes() == orc.tukey_weights(r).tobytes(), name
    assert (ref.tukey_weights(_vectors()["all_zero"], ref.W_TUKEY) == 1).all()


def _select(sorted_vals, n):
    """the first value whose count of values <= it exceeds n / 2 (integer division)"""
    for v in np.unique(sorted_vals):
        if np.searchsorted(sorted_vals, v, side="right") > n // 2:
            return int(v)
    raise AssertionError


def test_mode_2_medians_equal_a_sorted_selection():
    for name, r in _vectors().items():
        n = len(r)
        med = _select(np.sort(r), n)
        med2 = _select(np.sort(np.abs(r - med)), n)
        assert ref.medians(r, ref.W_TUKEY_SIGNED) == (med, med2), name
        # mode 1: the same selection after MedianMat's CV_8U saturation of the residuals, then of the deviations
        m1 = _select(np.sort(np.clip(r, 0, 255)), n)
        m1b = _select(np.sort(np.clip(np.abs(r - m1), 0, 255)), n)
        assert ref.medians(r, ref.W_TUKEY) == (m1, m1b), name
    assert ref.medians(_vectors()["half_even"], 2)[0] == 40 and ref.medians(_vectors()["half_odd_low"], 2)[0] == 10
    assert ref.medians(_vectors()["ends"], 1) == (255, 0) and ref.medians(_vectors()["ends"], 2) == (255, 0)
    assert ref.medians(_vectors()["all_minus_255"], 1) == (0, 255) and ref.medians(_vectors()["all_minus_255"], 2) == (-255, 0)


def test_non_default_constants_change_the_weights():
    r = _vectors()["narrow_24200"]
    a, b = ref.tukey_weights(r, 2), ref.tukey_weights(r, 2, b=2.5, mad_scale=1.0)
    assert (b <= a).all() and (b < a).any() and (a > 0).sum() > (b > 0).sum()


def test_the_two_modes_differ_where_the_saturation_bites(vislam, orc, canvas):
    """a GPU case whose residuals are mostly negative: as written the median of max(r, 0) is 0, signed it is
    not -- the two modes give different results there, so the GPU test tells them apart"""
    cs = awc.single_cases(vislam, orc, canvas)["mostly_minus_255"]
    a = ref.estimate_pose_features(orc, cs.params(orc), cs.w, cs.h, *cs.levels(), weights=1)
    b = ref.estimate_pose_features(orc, cs.params(orc), cs.w, cs.h, *cs.levels(), weights=2)
    assert (list(a.error), a.pose.as_array().tobytes()) != (list(b.error), b.pose.as_array().tobytes())


def _distance(orc, a, b):
    """(translation distance, rotation angle in rad) between two poses"""
    Ma, Mb = orc.se3_matrix(a).astype(np.float64), orc.se3_matrix(b).astype(np.float64)
    R = Ma[:3, :3].T @ Mb[:3, :3]
    return float(np.linalg.norm(Ma[:3, 3] - Mb[:3, 3])), float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("size", ["320", "150x110"])
def test_occluder_behaviour(vislam, orc, canvas, size, capsys):
    """frame 2 with a quarter of the patches under a rectangle of 255: how far the estimated pose moves away from the clean pair's
    (identity weights) under each weighting.  The numbers are printed (DESIGN.md section 4.6 quotes them); asserted is only what the
    restatement shows on both sizes: the translation of both Tukey poses stays closer to the clean pose than the identity pose does."""
    cases = awc.single_cases(vislam, orc, canvas)
    clean, occ = cases[f"clean_{size}"], cases[f"occluded_{size}"]
    base = ref.estimate_pose_features(orc, clean.params(orc), clean.w, clean.h, *clean.levels())
    rows = {}
    for mode in (0, 1, 2):
        c = ref.estimate_pose_features(orc, clean.params(orc), clean.w, clean.h, *clean.levels(), weights=mode)
        o = ref.estimate_pose_features(orc, occ.params(orc), occ.w, occ.h, *occ.levels(), weights=mode)
        rows[mode] = _distance(orc, o.pose, base.pose) + _distance(orc, c.pose, base.pose)
    with capsys.disabled():
        print(f"\noccluder {size} ({occ.c['occluded_fraction']:.2f} of the patches): mode -> |t_occ - t_clean|, angle_occ, |t_cleanmode - t_clean|, angle")
        for mode, r in rows.items():
            print(f"  mode {mode}: {r[0]:.6f} {r[1]:.6f} {r[2]:.6f} {r[3]:.6f}")
    assert rows[1][0] < rows[0][0] and rows[2][0] < rows[0][0], rows
