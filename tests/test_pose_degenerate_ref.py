"""CPU: the degenerate pose cases (tests/pose_degenerate_cases.py) on the oracle alone -- the recorded conditioning of every case is
well-formed and usable, the invariants tests/test_pose_degenerate_gpu.py will ask of the kernels' E hold for the oracle's own E with
the bounds stated there, the zero-theta fixture is what it says, and the invariants can fail: three deliberately wrong models are
each caught, by the assertion named in the test."""
import numpy as np
import pytest

import pose_degenerate_cases as pdc
from test_independent_numpy import _jacobi


@pytest.fixture(scope="module")
def spread():
    return pdc.load_spread()


@pytest.fixture(scope="module")
def oracle_runs(vislam, orc, spread):
    """every kept case once on the committed oracle: key -> (p, x1, x2, E, mask, n_inliers, iters)"""
    out = {}
    for c in pdc.kept_cases(spread):
        p = pdc.set_mode(vislam.default_params(), c[3])
        x1, x2 = pdc.make_case(*c[:3])
        out[pdc.case_key(*c)] = (p, x1, x2) + orc.essential_ransac(p, x1, x2)
    return out


def test_spread_record_covers_the_case_list(spread):
    assert set(spread) == {pdc.case_key(*c) for c in pdc.all_cases()} and len(spread) == 208
    for k, r in spread.items():
        assert r["dropped"] == (not r["agree"]), k
        assert r["dropped"] or (r["spread"] is not None and r["spread"] >= 0), k


def test_few_cases_dropped_and_no_class_emptied(spread):
    dropped = [k for k, r in spread.items() if r["dropped"]]
    assert len(dropped) <= pdc.MAX_DROPPED_SHARE * len(spread), dropped
    for cls in pdc.CLASSES:
        for m in pdc.SIZES:
            left = [1 for nz in pdc.NOISES for md in pdc.MODES if not spread[pdc.case_key(cls, m, nz, md)]["dropped"]]
            assert left, (cls, m)


def test_both_kinds_of_assertion_have_cases(spread):
    stable = sum(pdc.is_e_stable(r) for r in spread.values())
    unstable = sum((not r["dropped"]) and not pdc.is_e_stable(r) for r in spread.values())
    assert 3 * stable >= len(spread) and 3 * unstable >= len(spread), (stable, unstable)


def test_record_is_of_the_committed_oracle(spread, oracle_runs):
    """the integer outcomes the tool recorded are the ones the committed oracle gives today (a stale record would classify other runs)"""
    for k, (p, x1, x2, E, mask, ninl, iters) in oracle_runs.items():
        assert (spread[k]["n_inliers"], spread[k]["iters_run"]) == (ninl, iters), k


def test_invariants_hold_on_the_oracle(oracle_runs):
    """Section 4d with the oracle's own E: finite, mask == its own Sampson test with at most 2 % of the errors inside the 2^-20 band
    (measured: none inside it, no bit off, in any case, M == 5 included), and the essential-matrix residuals.  With E == oE the residual
    bound 100 x own is met by construction; what this pins down is where that bound means something.  Measured residuals of the
    oracle's E: <= 3e-11 for general, sideways, plane, line, dup, grid (bound <= 1e-8, two orders above the 1e-12 floor at most) and
    <= 3e-10 for forward, same; 1e-7 for tilted; but up to 6e-5 for shift, 1e-3 for far, 3e-3 for static and 4e-2 for noise-free pure
    rotation -- there the five-point solver returns models that are not essential matrices to better than that, the bound is 0.1 and
    above, and the constraint check is VACUOUS for static, rot, far and shift: those classes are held by the re-scoring and the integer
    outcomes only."""
    tight = {"general", "sideways", "plane", "line", "dup", "grid", "forward", "same"}
    for k, (p, x1, x2, E, mask, ninl, iters) in oracle_runs.items():
        assert ninl >= 5, k                                     # every kept case has a model
        fig = pdc.check_model(E, mask, ninl, x1, x2, p, E)
        assert fig["band"] == 0, k
        assert abs(np.linalg.norm(E) - 1.0) <= 1e-12, k
        if k.split("-")[0] in tight:
            assert max(fig["cubic"], fig["det"]) <= 1e-9, (k, fig)   # so the bound is <= 1e-7 there: a wrong model's O(0.1) fails it


# ---- the invariants can fail ----------------------------------------------------------------------------------------------------
def _first(oracle_runs, cls, m=40, noise=0.3, mode="adaptive"):
    return oracle_runs[pdc.case_key(cls, m, noise, mode)]


@pytest.mark.parametrize("cls", ["general", "sideways", "grid", "plane"])
def test_a_transposed_model_is_caught_by_the_rescoring(oracle_runs, cls):
    """E^T is an essential matrix too (the residuals cannot tell), but of the opposite motion: its own Sampson test disowns the mask"""
    p, x1, x2, E, mask, ninl, iters = _first(oracle_runs, cls, m=300)
    pdc.check_model(E, mask, ninl, x1, x2, p, E)
    with pytest.raises(AssertionError, match="^rescore:"):
        pdc.check_model(E.T.copy(), mask, ninl, x1, x2, p, E)


@pytest.mark.parametrize("cls", ["general", "static", "rot", "far", "same", "shift"])
def test_one_flipped_mask_bit_is_caught(oracle_runs, cls):
    """with the count kept as reported the count check fires; with the count adjusted to the flipped mask the re-scoring does"""
    p, x1, x2, E, mask, ninl, iters = _first(oracle_runs, cls, m=300, mode="fixed100")
    bad = mask.copy()
    i = int(np.flatnonzero(mask)[0])
    bad[i] = 0
    with pytest.raises(AssertionError, match="^count:"):
        pdc.check_model(E, bad, ninl, x1, x2, p, E)
    with pytest.raises(AssertionError, match="^rescore:"):
        pdc.check_model(E, bad, ninl - 1, x1, x2, p, E)


def test_a_perturbed_model_is_caught_by_the_constraints(oracle_runs):
    """1e-6 on one entry leaves the mask of a noisy problem alone but is not an essential matrix any more (where the bound bites)"""
    p, x1, x2, E, mask, ninl, iters = _first(oracle_runs, "general", m=40, noise=0.3)
    bad = E.copy()
    bad[2, 2] += 1e-6
    with pytest.raises(AssertionError, match="^constraint:"):
        pdc.check_model(bad, mask, ninl, x1, x2, p, E)


# ---- zero theta -----------------------------------------------------------------------------------------------------------------
def _votes(R, t, x1, y1, x2, y2):
    """oracle/pose.cpp cheirality() on _jacobi: (vote, zero theta met)"""
    A, V, z = _jacobi(pdc.dlt_ata(R, t, x1, y1, x2, y2))
    mn = 0
    for i in range(1, 4):
        if A[i][i] < A[mn][mn]:
            mn = i
    X = np.array([V[k][mn] for k in range(4)])
    with np.errstate(all="ignore"):
        ok = X[2] * X[3] > 0
        Xn = X[:3] / X[3]
        z2 = ((R[2][0] * Xn[0] + R[2][1] * Xn[1]) + R[2][2] * Xn[2]) + t[2]
        return bool(ok and Xn[2] < 50.0 and z2 > 0 and z2 < 50.0), z


def _select(g):
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]: return 0
    if g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]: return 1
    if g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]: return 2
    return 3


def _normalised(x1, x2):
    f = lambda a: (a.astype(np.float64) - pdc.ZT_C) * (1.0 / pdc.ZT_FOCAL)
    return np.concatenate([f(x1), f(x2)], 1)


def test_zero_theta_fixture_is_zero_theta():
    for name, R in zip(("I", "R2"), pdc.R_CANDS):
        qs = pdc.ZERO_THETA_Q[name]
        assert len(qs) == len(set(qs)) == 80
        for tz in (1.0, -1.0):
            for q in qs:
                assert _votes(R.tolist(), [0.0, 0.0, tz], *[v / 4.0 for v in q])[1], (name, tz, q)
    assert (-8, 0, 0, 4) in pdc.ZERO_THETA_Q["I"] and (-7, 0, 0, -4) in pdc.ZERO_THETA_Q["I"]     # (-2, 0, 0, 1), (-1.75, 0, 0, -1)
    # the pixels are those grid points exactly, and an ordinary correspondence is not zero-theta
    x1, x2 = pdc.quarters_to_pixels(pdc.ZERO_THETA_Q["I"])
    assert (_normalised(x1, x2) * 4 == np.array(pdc.ZERO_THETA_Q["I"])).all()
    g1, g2 = pdc.motion_rows(64, 11)
    assert not any(_votes(np.eye(3).tolist(), [0.0, 0.0, 1.0], *r)[1] for r in _normalised(g1, g2))


def test_rows_place_the_zero_theta_points_where_the_waves_are():
    rows = pdc.zero_theta_rows()
    Rs = [R.tolist() for R in pdc.R_CANDS]
    where = {}
    for name, (x1, x2) in rows.items():
        n = _normalised(x1, x2)
        where[name] = [i for i, r in enumerate(n) if any(_votes(R, [0.0, 0.0, 1.0], *r)[1] for R in Rs)] if len(n) < 200 else None
    assert where["one_in_wave_fwd"] == [37] and where["second_wave_back"] == [64]
    assert where["only_zero_theta_I"] == list(range(80)) and where["only_zero_theta_union"] == list(range(148))
    x1, x2 = rows["nsplit2_fwd"]
    assert len(x1) == 1100 and (4 * max(len(x1), 1) + 4095) // 4096 == 2                          # k_pose_final's nsplit
    n = _normalised(x1, x2)
    assert all(any(_votes(R, [0.0, 0.0, 1.0], *n[i])[1] for R in Rs) for i in (0, 255, 256, 1099))


@pytest.mark.parametrize("row", ["only_zero_theta_I", "only_zero_theta_union", "second_wave_back"])
def test_reusing_the_votes_for_the_negated_translation_is_caught(vislam, orc, row):
    """the oracle's recoverPose of E = [e_z]x is the vote of (I, e_z), (diag(-1, -1, 1), e_z), (I, -e_z), (diag(-1, -1, 1), -e_z) as
    restated here on _jacobi; a kernel that reused the votes of [R | t] unchanged for [R | -t] would pick another candidate or
    report another count -- the comparison of n_good / R / t with the oracle in the GPU test notices"""
    p = pdc.zt_params(vislam.default_params())
    x1, x2 = pdc.zero_theta_rows()[row]
    Ro, to, no = orc.recover_pose(p, pdc.E_Z, x1, x2)
    cands = [(R, [0.0, 0.0, tz]) for tz in (1.0, -1.0) for R in pdc.R_CANDS]
    n = _normalised(x1, x2)
    g = [sum(_votes(R.tolist(), t, *r)[0] for r in n) for R, t in cands]
    sel = _select(g)
    assert no == g[sel] and (Ro == cands[sel][0]).all() and (to == np.array(cands[sel][1])).all(), (g, no, to)
    gm = [g[0], g[1], g[0], g[1]]                               # the mutation
    selm = _select(gm)
    assert (gm[selm], selm) != (g[sel], sel), (g, gm)           # another count or another candidate: R / t / n_good differ


def test_fixture_breaks_the_equivariance_the_shortcut_rests_on():
    """what the fallback is FOR: off these points the decomposition under -t is the one under t with rows and columns 3 negated, bit
    for bit (test_independent_numpy); on every point of the fixture it is not.  (The VOTES derived from the first eigenvector happen to
    agree with the decomposed ones on this grid -- the eigenvectors differ in their last bits only -- so the GPU test shows that
    the second pass runs and returns the oracle's votes, in every wave shape; it cannot show that the shortcut would have been wrong.)"""
    D = [1.0, 1.0, 1.0, -1.0]
    for name, R in zip(("I", "R2"), pdc.R_CANDS):
        for q in pdc.ZERO_THETA_Q[name]:
            x = [v / 4.0 for v in q]
            Ap, Vp, z = _jacobi(pdc.dlt_ata(R.tolist(), [0.0, 0.0, 1.0], *x))
            An, Vn, _ = _jacobi(pdc.dlt_ata(R.tolist(), [0.0, 0.0, -1.0], *x))
            assert z and any(Vn[i][j] != D[i] * Vp[i][j] * D[j] for i in range(4) for j in range(4)), (name, q)


def test_rank_deficient_E_is_nan_on_the_oracle(vislam, orc):
    """the specification the header states: a zero or rank-1 E gives NaN R, t and n_good = 0"""
    p = pdc.zt_params(vislam.default_params())
    d = pdc.directed_E()
    for name in ("zero", "rank1"):
        E, x1, x2 = d[name]
        R, t, n = orc.recover_pose(p, E, x1, x2)
        assert n == 0 and np.isnan(R).all() and np.isnan(t).all(), (name, R, t, n)
    E, x1, x2 = d["identity"]
    R, t, n = orc.recover_pose(p, E, x1, x2)
    assert np.isfinite(R).all() and np.isfinite(t).all()
