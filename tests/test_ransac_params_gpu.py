"""GPU: the essential RANSAC and F2F at the ends of their parameters (tests/ransac_param_cases.py) against the CPU oracle and
tests/f2f_ref.py.  The yardstick is tests/test_limits_gpu.py::_ransac_case's: mask, inlier count and iterations equal, E within TOL up to
sign, recoverPose on the oracle's E within TOL, a second run identical.  What the oracle makes nothing sensible of is refused by
vis_set_params, and tests/test_ransac_params_ref.py records what the oracle does make of it."""
import ctypes as C

import numpy as np
import pytest

import f2f_ref as fr
import hostile_cases as hc
import ransac_param_cases as rc
from test_hostile_inputs_gpu import _dev, _f2f_dict, _f2f_launch
from test_pose_gpu import TOL, _cmpE

pytestmark = pytest.mark.gpu
E_INVALID = -1                                                         # VIS_E_INVALID


@pytest.mark.parametrize("m", rc.LENGTHS)
def test_essential_ransac_at_the_parameter_ends(vislam, orc, m):
    seen = {}
    for name, fields, mm, seed in rc.rows():
        if mm != m:
            continue
        p = rc.params(vislam.default_params(), fields)
        x1, x2 = rc.scene(p, m, seed)
        c = vislam.Context(0, p)
        try:
            E, mask, ninl, it = c.essential_ransac(x1, x2)
            E2, mask2, ninl2, it2 = c.essential_ransac(x1, x2)
            assert (ninl2, it2) == (ninl, it) and (mask2 == mask).all() and E2.tobytes() == E.tobytes(), name
            oE, omask, oninl, oiters = orc.essential_ransac(p, x1, x2)
            seen[name] = (oninl, oiters, ninl, it, float(_cmpE(E, oE)))
            assert (ninl, it) == (oninl, oiters), (name, seen[name])
            assert (mask == omask).all(), name
            assert _cmpE(E, oE) <= TOL, (name, seen[name])
            Rg, tg, ng = c.recover_pose(oE, x1, x2)
            Ro, to, no = orc.recover_pose(p, oE, x1, x2)
            assert ng == no and np.abs(Rg - Ro).max() <= TOL and np.abs(tg - to).max() <= TOL, name
        finally:
            c.close()
    print(f"m = {m}: (oracle inliers, iterations, device inliers, iterations, |dE|)", seen)
    assert seen["ransac_seed 0x0"] == seen["ransac_seed 0xffffffff"]      # one scene, one run: cv::RNG(0) is cv::RNG(0xffffffff)
    assert len(seen) == len(rc.CASES)


def test_refused_ransac_thresholds(vislam):
    c = vislam.Context(0)
    for v in rc.REFUSED_RANSAC_THRESHOLDS:
        p = vislam.default_params()
        p.ransac_threshold = v
        assert vislam.lib.vis_set_params(c._h, C.byref(p)) == E_INVALID, v
        assert "ransac_threshold" in vislam.lib.vis_last_error(c._h).decode(), v
    for v in (1e-18 * 458.654 * (1 + 1e-9), 1e18 * 458.654 * (1 - 1e-9)):      # the ends themselves are taken
        p = vislam.default_params()
        p.ransac_threshold = v
        c.set_params(p)
    c.close()


def _f2f(vislam, torch, p, m, seed):
    """(device record, restatement's record) of vis_f2f_batch on one pair of m correspondences at the setting p, as comparable dicts"""
    a, b, rot, t = fr.pair_inputs(m, seed, 0.2, 0.3)
    draws = np.random.default_rng(seed).integers(0, 2 ** 31, (max(int(p.f2f_iters), 1), 2)).astype(np.int32)
    with np.errstate(all="ignore"):
        want = fr.f2f(p, a, b, rot, draws, t)
    c = vislam.Context(0, p)
    try:
        recs, _, _ = _f2f_launch(vislam, torch, c, [dict(p1=a, p2=b, rot=rot, t=t)], m, _dev(torch, draws))
        again, _, _ = _f2f_launch(vislam, torch, c, [dict(p1=a, p2=b, rot=rot, t=t)], m, _dev(torch, draws))
        assert again.tobytes() == recs.tobytes()
    finally:
        c.close()
    return _f2f_dict(recs[0]), _f2f_dict(want)


@pytest.mark.parametrize("m", [40, 300])
def test_f2f_thresholds_and_iteration_ends(vislam, m):
    """f2f_threshold is compared as written, `error < threshold` in double: 0, a negative value, NaN and +inf are all taken and give the
    restatement's record (the device's two-compare shortcut has no band then: tests/f2f_ref.py band()); f2f_iters 0 and 1"""
    import torch
    counts = {}
    for thr in rc.F2F_THRESHOLDS + (370.0,):
        p = vislam.default_params()
        p.fy, p.f2f_iters, p.f2f_threshold = p.fx, 200, thr
        got, want = _f2f(vislam, torch, p, m, 3)
        assert hc.same_record(got, want), (thr, got, want)
        counts[repr(thr)] = want["count_max"]
    print("F2F counts per threshold:", counts)
    assert counts["nan"] == 0 and counts["inf"] == m and 0 < counts["370.0"] < m
    for iters in rc.F2F_ITERS:
        p = vislam.default_params()
        p.fy, p.f2f_iters = p.fx, iters
        got, want = _f2f(vislam, torch, p, m, 4)
        assert hc.same_record(got, want), (iters, got, want)
        assert (want["count_max"] > 0) == (iters == 1), (iters, want)
