"""Hand-made inputs of the match filters (nnFilter's ratio test, computeSymMatches, bestMatchesFilter's grid) over the parameter range
vis_set_params accepts.  Not a test module: shared by tests/test_match_params_ref.py (CPU: the oracle, and a numpy model of the ratio test
that shows the cases to be sharp) and tests/test_match_params_gpu.py (the kernel against the oracle, byte for byte).

A case is a dict: name, params (the fields of vis_params it changes), k1, k2 (keypoints), k12, k21 (2-NN lists of both directions).  Every
case has at most a few hundred keypoints; query q's best neighbour is train q and the reverse, so the symmetric list is what the ratio test
leaves, and the keypoints of a ratio case sit in cells of their own, so the grid keeps all of it."""
import numpy as np

F32 = np.float32
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
MAX_GRID_ROOT = 32                                                     # VIS_MAX_GRID_ROOT

BELOW_ONE = float(np.nextafter(F32(1.0), F32(0.0)))
RATIOS = (0.0, 0.25, 0.5, 0.75, float(F32(0.8)), 1.0, 1.5, BELOW_ONE, -0.5, float("nan"), float("inf"))
TIE_RATIOS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5)                           # those with integer pairs d0 == ratio * d1 in 0 ... 256
# (d0, d1) with d0 == ratio * d1 exactly, whatever the ratio's width; each goes in with d0 - 1 and d0 + 1 beside it
TIES = {0.0: ((0, 1), (0, 7), (0, 256)), 0.25: ((1, 4), (16, 64), (64, 256)), 0.5: ((1, 2), (100, 200), (128, 256)),
        0.75: ((3, 4), (96, 128), (192, 256)), 1.0: ((1, 1), (17, 17), (255, 255), (256, 256)), 1.5: ((3, 2), (150, 100), (255, 170))}
# pairs every ratio sees: 0 / 0, 256 / 256, equal, far apart either way, and the pairs next to 0.8f * d1 (never an integer for d1 in 1 ... 256)
COMMON = ((0, 0), (256, 256), (0, 256), (256, 0), (4, 5), (3, 5), (5, 5), (204, 255), (205, 255), (203, 255), (8, 10), (9, 10), (1, 256), (255, 256))


def ratio_pairs(ratio):
    out = list(COMMON)
    for d0, d1 in TIES.get(ratio, ()):
        out += [(d0, d1)] + [(d, d1) for d in (d0 - 1, d0 + 1) if 0 <= d <= 256]
    return out


def keypoints(xy):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    k = np.zeros(len(xy), KEYPOINT)
    k["x"], k["y"], k["size"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, -1
    return k


def knn(best, second, d0, d1):
    n = len(best)
    o = np.zeros((n, 2), DMATCH)
    o["queryIdx"] = np.arange(n, dtype=np.int32)[:, None]
    o["trainIdx"][:, 0], o["trainIdx"][:, 1] = best, second
    o["distance"][:, 0], o["distance"][:, 1] = d0, d1
    return o


def identity_knn(d0, d1):
    n = len(d0)
    q = np.arange(n)
    return knn(q, (q + 1) % max(n, 2) if n > 1 else q, d0, d1)


def ratio_case(ratio, sym_mode):
    """one keypoint per distance pair, on a 32 x 32 grid of 8-pixel cells (row-major: the symmetric list and the grid output have the same
    order); direction 1 carries the pairs in order, direction 2 the same pairs rotated by 5, so the two modes differ wherever one survives
    and the other does not"""
    pairs = ratio_pairs(ratio)
    n = len(pairs)
    assert n <= 1024
    q = np.arange(n)
    xy = np.stack([8.0 * (q % 32) + 4.0, 8.0 * (q // 32) + 4.0], 1)
    d12 = np.array(pairs, F32)
    d21 = np.roll(d12, 5, axis=0)
    return dict(name=f"ratio {ratio!r} mode {sym_mode}", params=dict(ratio=ratio, sym_mode=sym_mode, n_cells=1024, w_size=256, h_size=256),
                k1=keypoints(xy), k2=keypoints(xy + 1.0), k12=identity_knn(d12[:, 0], d12[:, 1]), k21=identity_knn(d21[:, 0], d21[:, 1]))


def ratio_cases():
    return [ratio_case(r, mode) for r in RATIOS for mode in (0, 1)]


def model_sym(case, strict=True, narrow=lambda r: float(F32(r))):
    """numpy model of nnFilter + computeSymMatches on a case: the query indices that survive.  strict=False: `>=` in place of `>`;
    narrow: how the ratio reaches the comparison (the library: the float widened to double)"""
    r = np.float64(narrow(case["params"]["ratio"]))
    gt = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)

    def survives(two):
        with np.errstate(invalid="ignore"):
            return (two["trainIdx"][:, 0] >= 0) & (two["trainIdx"][:, 1] >= 0) & ~gt(two["distance"][:, 0].astype(np.float64), r * two["distance"][:, 1].astype(np.float64))
    ok = survives(case["k12"])
    t = case["k12"]["trainIdx"][:, 0]
    ok &= case["k21"]["trainIdx"][t, 0] == np.arange(len(t))
    if case["params"]["sym_mode"] == 1:
        ok &= survives(case["k21"])[t]
    return np.flatnonzero(ok)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
GRID_N_CELLS = (1, 2, 3, 4, 48, 49, 50, 1023, 1024, 1025, 1088)
REFUSED_N_CELLS = (1089, 1090, 4096, 2 ** 31 - 1)
GRID_SIZES = ((752, 480), (1, 1), (100, 70), (64, 64), (4000, 3000), (7, 1000))     # (w_size, h_size); the keypoints span about 100 x 70


def grid_limits(n_cells, w_size, h_size):
    """(root, hf, wf): bestMatchesFilter's limits as the reference accumulates them, `h_final = h_final + winHSize` in float"""
    root = int(np.floor(np.sqrt(np.float64(n_cells))))
    win_w, win_h = F32(np.float64(w_size) / np.floor(np.sqrt(np.float64(n_cells)))), F32(np.float64(h_size) / np.floor(np.sqrt(np.float64(n_cells))))
    hf, wf = np.zeros(root, F32), np.zeros(root, F32)
    a, b = win_h, win_w
    for j in range(root):
        hf[j], wf[j] = a, b
        a, b = F32(a + win_h), F32(b + win_w)
    return root, hf, wf


def _around(v):
    return [np.nextafter(F32(v), F32(-np.inf)), F32(v), np.nextafter(F32(v), F32(np.inf))]


def grid_case(n_cells, w_size, h_size, seed=0):
    """keypoints exactly on, one float below and one float above cell limits (the first two, a middle one and the last two of each axis),
    spread over the extent, negative (and -0.0), beyond w_size / h_size; distances from a set of four, so cells hold ties (the first in y
    order wins); every match mutual and past the ratio test.  The rows are shuffled: the sort by y is the filter's own work"""
    rng = np.random.default_rng(1000 * seed + n_cells % 997 + w_size)
    root, hf, wf = grid_limits(n_cells, w_size, h_size)
    pick = sorted(set(int(i) for i in (0, 1, root // 2, root - 2, root - 1) if 0 <= i < root))
    pts = []
    for i in pick:
        for j in pick:
            ymid = F32(hf[j] - (hf[0] * F32(0.5)))
            xmid = F32(wf[i] - (wf[0] * F32(0.5)))
            pts += [(x, ymid) for x in _around(wf[i])] + [(xmid, y) for y in _around(hf[j])] + [(wf[i], hf[j])]
    ext_w, ext_h = min(float(w_size), 100.0), min(float(h_size), 70.0)
    pts += [(rng.uniform(0, ext_w), rng.uniform(0, ext_h)) for _ in range(40)]
    pts += [(-3.5, 2.0), (2.0, -3.5), (-1e6, -1e6), (-0.0, 1.0), (0.0, 1.0), (1.0, -0.0), (1.0, 0.0), (1.5, 0.0), (0.5, -0.0), (0.0, 0.0),
            (w_size + 5.0, 1.0), (1.0, h_size + 5.0), (w_size + 5.0, h_size + 5.0), (float(w_size), float(h_size)), (1e9, 1.0), (1.0, 1e9)]
    pts += [(10.25, 20.5)] * 3 + [(10.25, 20.25)]                     # one cell, equal y and a smaller one: stable order decides among equal distances
    xy = np.array(pts, F32)[rng.permutation(len(pts))]
    assert len(xy) <= 300
    d0 = rng.integers(10, 14, len(xy)).astype(F32)
    return dict(name=f"grid n_cells {n_cells} size {w_size} x {h_size}", params=dict(n_cells=n_cells, w_size=w_size, h_size=h_size),
                k1=keypoints(xy), k2=keypoints(xy + 1.0), k12=identity_knn(d0, d0 + 100), k21=identity_knn(d0, d0 + 100))


def empty_last_band_case():
    """7 x 7 cells over 70 x 70, nothing below the sixth band: the filter's band loop ends with matches used up and bands left"""
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(0, 70, 60), rng.uniform(0, 59.9, 60)], 1).astype(F32)
    d0 = rng.integers(10, 14, len(xy)).astype(F32)
    return dict(name="grid, empty last band", params=dict(n_cells=49, w_size=70, h_size=70), k1=keypoints(xy), k2=keypoints(xy + 1.0),
                k12=identity_knn(d0, d0 + 100), k21=identity_knn(d0, d0 + 100))


def signed_zero_case():
    """two matches of equal distance in one cell at y = +0 and y = -0, the +0 first: equal in the reference's sort, so the first stays first"""
    xy = np.array([(1.0, 0.0), (2.0, -0.0), (60.0, 60.0)], F32)
    d0 = np.array([10, 10, 12], F32)
    return dict(name="grid, y = +0 before y = -0", params=dict(n_cells=4, w_size=100, h_size=100), k1=keypoints(xy), k2=keypoints(xy + 1.0),
                k12=identity_knn(d0, d0 + 100), k21=identity_knn(d0, d0 + 100))


def grid_cases():
    out = [grid_case(n, 752, 480) for n in GRID_N_CELLS]
    out += [grid_case(n, w, h, seed=1) for n in (1, 3, 49, 50, 1088) for w, h in GRID_SIZES[1:]]
    return out + [empty_last_band_case(), signed_zero_case()]


def apply(p, case):
    """the vis_params `p` with the case's fields set (returns p)"""
    for k, v in case["params"].items():
        setattr(p, k, v)
    return p
