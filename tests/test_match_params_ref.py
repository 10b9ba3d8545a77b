"""CPU: the cases of tests/match_param_cases.py on the oracle alone -- that they are sharp (a filter with `>=` for `>`, or with the ratio
narrowed another way, gives another list on them), that the oracle's ratio test is the numpy model's, and that the grid cases contain what
they are meant to (keypoints on, below and above the limits; ties inside a cell; an empty last band; grid roots up to 32 and, for the
oracle only, beyond).  tests/test_match_params_gpu.py holds the kernel to the oracle on the same cases."""
import numpy as np
import pytest

import match_param_cases as mc


def _oracle(vislam, orc, case):
    p = mc.apply(vislam.default_params(), case)
    return orc.good_matches(p, case["k1"], case["k2"], case["k12"], case["k21"])


def test_the_ratio_cases_are_sharp(vislam, orc):
    """per tie ratio at least one case on which `>=` differs from `>`; for 0.8f and the largest float below 1, which have no integer tie, a
    ratio narrowed to half precision differs; and the oracle equals the `>` model with the float ratio widened to double on every case.
    (A ratio of double 0.8 in place of 0.8f cannot be told apart on integer distances up to 256: shown here, not assumed.)"""
    ge_differs, half_differs = set(), set()
    for case in mc.ratio_cases():
        ratio = case["params"]["ratio"]
        good, sym = _oracle(vislam, orc, case)
        want = mc.model_sym(case)
        assert sym["queryIdx"].tolist() == want.tolist(), case["name"]
        assert good.tobytes() == sym.tobytes(), case["name"]            # one keypoint per cell, row-major: the grid keeps everything in order
        if mc.model_sym(case, strict=False).tolist() != want.tolist():
            ge_differs.add(ratio)
        if mc.model_sym(case, narrow=lambda r: float(np.float16(r))).tolist() != want.tolist():
            half_differs.add(ratio)
    assert ge_differs >= set(mc.TIE_RATIOS), ge_differs
    assert half_differs >= {float(np.float32(0.8)), mc.BELOW_ONE}, half_differs
    d1 = np.arange(0, 257, dtype=np.float64)[None, :]
    d0 = np.arange(0, 257, dtype=np.float64)[:, None]
    assert ((d0 > np.float64(np.float32(0.8)) * d1) == (d0 > 0.8 * d1)).all()


def test_what_the_special_ratios_keep(vislam, orc):
    """0 keeps d0 = 0; a negative ratio d0 = d1 = 0 only; NaN and +inf everything with two neighbours (include/vislam_hip.h says so)"""
    for ratio, rule in ((0.0, lambda a, b: a == 0), (-0.5, lambda a, b: (a == 0) & (b == 0)), (float("nan"), lambda a, b: a >= 0),
                        (float("inf"), lambda a, b: a >= 0)):
        case = mc.ratio_case(ratio, 0)
        _, sym = _oracle(vislam, orc, case)
        d = case["k12"]["distance"]
        assert sym["queryIdx"].tolist() == np.flatnonzero(rule(d[:, 0], d[:, 1])).tolist(), ratio
    both = [len(_oracle(vislam, orc, mc.ratio_case(0.75, mode))[1]) for mode in (0, 1)]
    assert 0 < both[1] < both[0]                                       # the second direction's ratio test is seen to act


def test_the_grid_cases_hold_what_they_claim(vislam, orc):
    roots, ties, dropped = set(), 0, 0
    for case in mc.grid_cases():
        q = case["params"]
        root, hf, wf = mc.grid_limits(q["n_cells"], q["w_size"], q["h_size"])
        assert 1 <= root <= mc.MAX_GRID_ROOT and len(case["k1"]) <= 300, case["name"]
        roots.add(root)
        good, sym = _oracle(vislam, orc, case)
        assert len(sym) == len(case["k1"]) and 0 < len(good) <= root * root, case["name"]
        x, y = case["k1"]["x"], case["k1"]["y"]
        if case["name"].startswith("grid n_cells"):
            assert np.isin(hf[[0, root - 1]], y).all() and np.isin(wf[[0, root - 1]], x).all(), case["name"]      # on the limits, and beside them
            assert np.isin(np.nextafter(hf[0], np.float32(np.inf)), y) and np.isin(np.nextafter(wf[0], np.float32(-np.inf)), x), case["name"]
            assert (x < 0).any() and (y < 0).any() and (x > q["w_size"]).any() and (y > q["h_size"]).any(), case["name"]
            dropped += int((y > hf[root - 1]).sum())
        # a cell's winner: the smallest distance, and among equals the first in the stable order by y
        gx, gy, gd = x[good["queryIdx"]], y[good["queryIdx"]], good["distance"]
        band = np.searchsorted(hf, gy, side="left")
        assert (band < root).all() and (np.diff(band) >= 0).all(), case["name"]
        order = np.argsort(y, kind="stable")
        for k in range(len(good)):
            col = min(int(np.searchsorted(wf, gx[k], side="left")), root - 1)
            cell = [i for i in order if y[i] <= hf[root - 1] and np.searchsorted(hf, y[i], side="left") == band[k]
                    and min(int(np.searchsorted(wf, x[i], side="left")), root - 1) == col]
            best = min(case["k12"]["distance"][i, 0] for i in cell)
            first = [i for i in cell if case["k12"]["distance"][i, 0] == best]
            ties += len(first) > 1
            assert good["queryIdx"][k] == first[0] and gd[k] == best, (case["name"], k)
    assert roots >= {1, 2, 6, 7, 31, 32} and ties > 20 and dropped > 20
    good, _ = _oracle(vislam, orc, mc.empty_last_band_case())
    assert (mc.empty_last_band_case()["k1"]["y"][good["queryIdx"]] <= 60.0).all()
    good, _ = _oracle(vislam, orc, mc.signed_zero_case())
    assert good["queryIdx"].tolist() == [0, 2]


def test_the_oracle_beyond_root_32_is_another_grid(vislam, orc):
    """n_cells = 1089 is a 33 x 33 grid in the reference and in the oracle.  The library's filter holds 32 x 32 cells, so vis_set_params
    refuses it; this is what a grid cut to 32 rows and columns WOULD lose, on the oracle: matches below row 32 and the identity of column 32"""
    case = mc.grid_case(1088, 752, 480)
    case["params"]["n_cells"] = 1089
    good33, _ = _oracle(vislam, orc, case)
    root, hf, wf = mc.grid_limits(1089, 752, 480)
    assert root == 33
    y, x = case["k1"]["y"][good33["queryIdx"]], case["k1"]["x"][good33["queryIdx"]]
    assert (y > hf[31]).any() and (x > wf[31]).any()
    for n in mc.REFUSED_N_CELLS:
        assert int(np.floor(np.sqrt(np.float64(n)))) > mc.MAX_GRID_ROOT
    assert int(np.floor(np.sqrt(np.float64(max(mc.GRID_N_CELLS))))) == mc.MAX_GRID_ROOT
