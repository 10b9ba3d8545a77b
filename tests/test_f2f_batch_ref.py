"""CPU: tests/f2f_ref.py -- the numpy restatement of F2FRansac / FilterKeypoints that the GPU tests compare the batched kernels with --
against the oracle (orc.f2f_ransac), against a second restatement in plain Python floats, and the reasoning behind the device's
two-compare form of the inlier test (csrc/epipolar.hip epi_inlier) against the full expression.  Tolerance: the project's own for F2FRansac
(tests/test_pose_gpu.py): equal count_max, |dt| <= 1e-6."""
import numpy as np
import pytest

import f2f_ref as fr

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


@pytest.mark.parametrize("thr", [250.0, 370.0, 600.0])
@pytest.mark.parametrize("m", [2, 3, 15, 40, 120])
def test_restatement_against_the_oracle(vislam, orc, m, thr):
    p = vislam.default_params()
    p.f2f_threshold = thr
    a, b, rot, t = fr.pair_inputs(m, 7 * m + 1, 0.2, 0.3)
    draws = np.random.default_rng(m).integers(0, 2 ** 31, (1000, 2)).astype(np.int32)
    tref = (0.37 * t).astype(np.float32)
    rec = fr.f2f(p, a, b, rot, draws, tref)
    scale = np.float32(np.sqrt((tref[0] * tref[0] + tref[1] * tref[1]) + tref[2] * tref[2]))
    ref, co = orc.f2f_ransac(p, fr.keypoints(KP, a), fr.keypoints(KP, b), rot, fr.reduce_draws(draws, m), float(scale))
    assert rec["count_max"] == co, (rec, co)
    if rec["flipped"]:
        ref = -ref
    assert np.abs(rec["t"] - ref).max() <= 1e-6
    assert rec["n_points"] == m
    if m == 2:                                                     # both samples are correspondence 0: every cross product is zero
        assert rec["best_iter"] == -1 and rec["n_degenerate"] == 1000 and co == 0
    else:
        assert rec["best_iter"] >= 0 and rec["count_max"] >= 2
        # the winner is the FIRST iteration with the largest count
        _, (d, cnt, deg, nv) = fr.f2f(p, a, b, rot, draws, tref, detail=True)
        assert cnt[rec["best_iter"]] == cnt.max() and (cnt[:rec["best_iter"]] < cnt.max()).all()
    # without a reference translation: scale 1, no flip
    free = fr.f2f(p, a, b, rot, draws)
    ref1, co1 = orc.f2f_ransac(p, fr.keypoints(KP, a), fr.keypoints(KP, b), rot, fr.reduce_draws(draws, m), 1.0)
    assert free["count_max"] == co1 and free["flipped"] == 0 and np.abs(free["t"] - ref1).max() <= 1e-6


def test_zero_records(vislam):
    p = vislam.default_params()
    draws = np.zeros((1000, 2), np.int32)
    zero = fr.record_tuple(fr.ZERO_RECORD)
    for m in (0, 1):
        a, b, rot, t = fr.pair_inputs(m, 3, 0.0, 0.1)
        assert fr.record_tuple(fr.f2f(p, a, b, rot, draws)) == zero
    a, b, rot, t = fr.pair_inputs(40, 3, 0.0, 0.1)
    assert fr.record_tuple(fr.f2f(p, a, b, rot, draws[:0], iters=0)) == zero
    assert zero[3] == -1


def test_tie_inputs_give_the_first_live_iteration(vislam):
    """the inputs of tests/test_f2f_batch_gpu.py test_tie_goes_to_the_first_live_iteration: under the restatement the (c, c) draws are
    skipped, every other iteration has the count of the hypothesis run alone, which is > 0, and the winner is the first of them"""
    p = vislam.default_params()
    p.fy = p.fx
    for a, b, rot, t in fr.edge_rows(vislam.F2F_TILE):
        idx = fr.reduce_draws(fr.tie_draws(1), len(a))
        assert tuple(idx[1]) == fr.TIE_PAIR and tuple(idx[0]) == (fr.TIE_SKIP, fr.TIE_SKIP)
        alone = fr.f2f(p, a, b, rot, fr.tie_draws(0, 1), t, iters=1)
        assert alone["best_iter"] == 0 and alone["n_degenerate"] == 0 and 0 < alone["count_max"] < len(a)
        for first in fr.TIE_FIRSTS:
            rec, (d, cnt, deg, nv) = fr.f2f(p, a, b, rot, fr.tie_draws(first), t, iters=fr.TIE_ITERS, detail=True)
            assert deg[:first].all() and not deg[first:].any() and (cnt[first:] == alone["count_max"]).all()
            assert (rec["best_iter"], rec["n_degenerate"], rec["count_max"]) == (first, first, alone["count_max"])
            assert rec["t"].tobytes() == alone["t"].tobytes() and rec["flipped"] == alone["flipped"]


def test_filter_two_ways(vislam):
    """masks of the numpy restatement and of the plain-Python one agree for every pair of the GPU tests' batch, and the two thresholds
    cut on both sides (0 < kept < m) on at least 8 of the 10 pairs with m >= 2 -- the condition the GPU test relies on"""
    p = vislam.default_params()
    for thr in (500.0, 370.0):
        both = 0
        for (m, seed, outl, noise) in fr.batch_cases(vislam.F2F_TILE):
            a, b, rot, t = fr.pair_inputs(m, seed, outl, noise)
            k1, c1 = fr.filter_keypoints(p, a, b, rot, t, thr)
            k2, c2 = fr.filter_keypoints_plain(p, a, b, rot, t, thr)
            assert k1.tobytes() == k2.tobytes() and c1 == c2 == int(k1.sum()), (m, thr)
            both += int(m >= 2 and 0 < c1 < m)
            z, cz = fr.filter_keypoints(p, a, b, rot, np.zeros(3, np.float32), thr)
            assert cz == 0 and not z.any()                         # a zero translation: NaN, nothing kept
            assert fr.filter_keypoints_plain(p, a, b, rot, np.zeros(3, np.float32), thr)[1] == 0
        assert both >= 8, (thr, both)


@pytest.mark.parametrize("thr", [250.0, 370.0, 500.0, 600.0])
def test_two_compare_form_equals_the_full_expression(thr):
    """This checks the reasoning (the band's derivation), not the device."""
    rng = np.random.default_rng(int(thr))
    c = 10.0 ** (-1000.0 / thr)
    lo, hi = fr.band(thr)
    assert 0 < lo < c < hi < 1 and (hi - lo) / c < 1e-12
    wide = np.concatenate([rng.uniform(-1.5, 1.5, 500_000), 10.0 ** rng.uniform(-12, 0.5, 500_000) * rng.choice([-1.0, 1.0], 500_000)])
    near = c * (1.0 + rng.uniform(-1e-10, 1e-10, 1_000_000)) * rng.choice([-1.0, 1.0], 1_000_000)
    edge = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), -np.nextafter(1.0, 0.0), -np.nextafter(1.0, 2.0),
                     5e-324, 2.2e-308, -1e-310, np.nan, np.inf, -np.inf, c, lo, hi, np.nextafter(lo, 0.0), np.nextafter(hi, 1.0)])
    for x in (wide, near, edge):
        got, inside = fr.inlier_banded(x, thr)
        want = fr.inlier_full(x, thr)
        assert (got == want).all(), x[got != want][:5]
    # the pure compare |x| < c differs from the expression only inside the band, and the band is rarely entered
    pure = np.abs(near) < c
    full = fr.inlier_full(near, thr)
    _, inside = fr.inlier_banded(near, thr)
    assert (pure == full)[~inside].all()
    assert fr.inlier_banded(wide, thr)[1].mean() < 1e-4
    e = fr.inlier_full(edge, thr)
    assert e[0] and e[1] and e[2] and e[3] and not e[4] and e[5] and e[8] and not e[11] and e[12] and e[13]


@pytest.mark.parametrize("thr", [0.0, -5.0, np.inf, -np.inf, np.nan, 3.0, 1e19, 1e300])
def test_thresholds_outside_the_reasoning_take_the_full_expression(thr):
    lo, hi = fr.band(thr)
    if thr in (1e19,):                                             # c = 1 - 2.3e-16: no room for a band below 1
        assert (lo, hi) == (0.0, np.inf)
    if not (thr > 0) or not np.isfinite(thr) or thr == 3.0:
        assert (lo, hi) == (0.0, np.inf)
    x = np.array([0.0, 1e-300, 0.5, 1.0, 2.0, np.nan, np.nextafter(1.0, 0.0)])
    got, inside = fr.inlier_banded(x, thr)
    assert (got == fr.inlier_full(x, thr)).all()
    if (lo, hi) == (0.0, np.inf):
        assert inside.all()
