"""CPU: what the oracle's essential RANSAC does at the ends of its parameters (tests/ransac_param_cases.py) -- the facts behind what
vis_set_params accepts and refuses, and the preconditions of tests/test_ransac_params_gpu.py."""
import numpy as np
import pytest

import ransac_param_cases as rc


def _oracle_params(vislam, orc, fields):
    p = rc.params(vislam.default_params(), fields)
    op = orc.Params()
    for f, _ in p._fields_:
        setattr(op, f, getattr(p, f))
    return op


def test_every_case_gives_the_oracle_something_to_decide(vislam, orc):
    got = {}
    for name, fields, m, seed in rc.rows():
        op = _oracle_params(vislam, orc, fields)
        x1, x2 = rc.scene(op, m, seed)
        E, mask, ninl, iters = orc.essential_ransac(op, x1, x2)
        got[name, m] = (ninl, iters)
        assert 1 <= iters <= int(op.ransac_max_iters) and ninl == int(mask.sum()), (name, m)
        assert ninl >= 5 or name == "ransac_threshold 0.0001", (name, m, ninl)       # (0.3 px of noise: a 1e-4 px band may hold the sample alone)
    print(got)
    for m in rc.LENGTHS:
        # the adaptive stop ends a budget of 100000 after a few hundred iterations; one iteration is one iteration
        assert 5 < got["ransac_max_iters 100000", m][1] < 1000, got["ransac_max_iters 100000", m]
        assert got["ransac_max_iters 1", m][1] == 1
        # a confidence next to 1 runs longer than one next to 0
        assert got["ransac_prob 1e-12", m][1] <= got["ransac_prob 0.5", m][1] <= got[f"ransac_prob {rc.ONE_BELOW!r}", m][1]
        assert got["ransac_threshold 1000.0", m][0] == m            # 1000 px: every correspondence


def test_seed_zero_is_the_seed_0xffffffff(vislam, orc):
    """cv::RNG(0) takes the state 0xffffffff: the oracle does, api.hip's sample table and pose.hip's replay do"""
    for m in rc.LENGTHS:
        a, b, c = (_oracle_params(vislam, orc, dict(ransac_seed=s)) for s in (0, 0xffffffff, 0xfffffffe))
        x1, x2 = rc.scene(a, m, 77)
        ra, rb, rd = (orc.essential_ransac(q, x1, x2) for q in (a, b, c))
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2:] == rb[2:], m
        assert rd[0].tobytes() != ra[0].tobytes(), m                # (another seed is another run)


def test_what_the_oracle_does_with_the_refused_thresholds(vislam, orc):
    """0 and NaN: no correspondence is ever accepted, every iteration runs, no model.  +inf: every correspondence under the first model.
    A negative threshold: the run of its absolute value (it is squared).  None is a setting anybody means: vis_set_params refuses all four
    (tests/test_ransac_params_gpu.py)."""
    m = 120
    base = _oracle_params(vislam, orc, {})
    x1, x2 = rc.scene(base, m, 78)
    want = orc.essential_ransac(base, x1, x2)
    for v in (0.0, float("nan")):
        E, mask, ninl, iters = orc.essential_ransac(_oracle_params(vislam, orc, dict(ransac_threshold=v)), x1, x2)
        assert not E.any() and ninl == 0 and not mask.any() and iters == rc.ITERS, v
    E, mask, ninl, iters = orc.essential_ransac(_oracle_params(vislam, orc, dict(ransac_threshold=float("inf"))), x1, x2)
    assert ninl == m and mask.all() and iters == 1
    neg = orc.essential_ransac(_oracle_params(vislam, orc, dict(ransac_threshold=-1.0)), x1, x2)
    assert neg[0].tobytes() == want[0].tobytes() and neg[1].tobytes() == want[1].tobytes() and neg[2:] == want[2:]
