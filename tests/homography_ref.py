"""The homography RANSAC and the H-or-E model choice of include/vislam_hip.h (vis_find_homography / vis_homography_batch /
vis_batch_homography), restated operation for operation; the case builder; an independent solver.  Not a test module: shared by
tests/test_homography_ref.py (CPU), tests/test_homography_gpu.py, tools/homography_probe.py.

The 3 x 3 work runs on plain Python floats (IEEE doubles, one rounding per operation, no contraction) in the kernel's parenthesisation
(csrc/homography.hip); the per-point work is element-wise float64 numpy, which does not contract either.  The two sums of the scores are
taken in the kernel's order: 64 partial sums over i mod 64 in rising i, then the butterfly v = v + v[lane ^ off], off = 32 ... 1.

The independent method (dlt_svd) is the textbook one: the null vector of the 8 x 9 DLT matrix of the same four points by
numpy.linalg.svd."""
import ctypes as C

import numpy as np

import pose_degenerate_cases as pdc

MODEL_NONE, MODEL_HOMOGRAPHY, MODEL_ESSENTIAL = 0, 1, 2
H_LIST = ("static", "rot", "plane", "tilted", "far", "shift")          # a homography explains the pair
E_LIST = ("general", "forward", "sideways", "grid")                    # only an essential matrix does
ROBUST_ONLY = ("line", "dup", "same")                                  # both models or neither: run, never classified
W_PX, H_PX = 752, 480                                                  # where the planted outliers are drawn

RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("score_h", "<f8"), ("score_e", "<f8"), ("n_inliers", "<i4"), ("n_points", "<i4"),
                         ("best_iter", "<i4"), ("n_degenerate", "<i4"), ("n_inliers_e", "<i4"), ("model", "<i4")])


class Params(C.Structure):
    """vis_homography_params with its defaults, for callers without the library (CPU tests)"""
    _fields_ = [("iters", C.c_int32), ("min_inliers", C.c_int32), ("chi2_h", C.c_double), ("chi2_e", C.c_double), ("sigma_px", C.c_double),
                ("h_ratio", C.c_double)]


def default_params():
    return Params(200, 8, 5.991, 3.841, 1.0, 0.40)


class Camera:
    def __init__(self, fx=pdc.FOCAL, cx=pdc.CX, cy=pdc.CY):
        self.fx, self.cx, self.cy = float(fx), float(cx), float(cy)


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["best_iter"] = -1
    return r


def make_draws(seed, iters=200):
    return np.random.default_rng(seed).integers(0, 2 ** 31, (iters, 4)).astype(np.int32)


def make_rows(cls, m, noise, outliers, seed=None):
    """(x1, x2, planted): pose_degenerate_cases.make_case with the first `outliers` share of x2 replaced by uniform pixels of a 752 x 480
    image; planted = the number of correspondences left alone"""
    x1, x2 = pdc.make_case(cls, m, noise, seed)
    k = int(outliers * m)
    if k:
        rng = np.random.default_rng([77, pdc.CLASSES.index(cls), m, int(round(10 * noise))])
        x2 = x2.copy()
        x2[:k] = np.stack([rng.uniform(0, W_PX, k), rng.uniform(0, H_PX, k)], 1).astype(np.float32)
    return x1, x2, m - k


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def thresholds(cam, hp):
    """(fx_inv, s2, t_h, t_e, t_self) as the host computes them, in double"""
    fx_inv = 1.0 / cam.fx
    s = hp.sigma_px * fx_inv
    s2 = s * s
    t_h = hp.chi2_h * s2
    return fx_inv, s2, t_h, hp.chi2_e * s2, t_h * 2.0 ** -20


def normalise(cam, x1, x2):
    """the pose stage's coordinates: ((double)u - c) * (1 / fx), four float64 arrays"""
    fx_inv = 1.0 / cam.fx
    a, b = np.asarray(x1, np.float32).astype(np.float64), np.asarray(x2, np.float32).astype(np.float64)
    return (a[:, 0] - cam.cx) * fx_inv, (a[:, 1] - cam.cy) * fx_inv, (b[:, 0] - cam.cx) * fx_inv, (b[:, 1] - cam.cy) * fx_inv


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _bad(v):
    return not (v != 0.0) or not (abs(v) <= 1.7976931348623157e308)


def adj(M):
    """rows c1 x c2, c2 x c0, c0 x c1 of the columns of a row-major 3 x 3"""
    c0, c1, c2 = [M[0], M[3], M[6]], [M[1], M[4], M[7]], [M[2], M[5], M[8]]
    return _cross3(c1, c2) + _cross3(c2, c0) + _cross3(c0, c1)


def basis(x, y):
    """(M, ok): M = [l0 p0 | l1 p1 | l2 p2] of the four points (x_k, y_k, 1)"""
    p = [[x[k], y[k], 1.0] for k in range(4)]
    c12, c20, c01 = _cross3(p[1], p[2]), _cross3(p[2], p[0]), _cross3(p[0], p[1])
    l = [_dot3(c12, p[3]), _dot3(c20, p[3]), _dot3(c01, p[3])]
    det = _dot3(c01, p[2])
    M = [l[0] * p[0][0], l[1] * p[1][0], l[2] * p[2][0],
         l[0] * p[0][1], l[1] * p[1][1], l[2] * p[2][1],
         l[0] * p[0][2], l[1] * p[1][2], l[2] * p[2][2]]
    return M, not (_bad(l[0]) or _bad(l[1]) or _bad(l[2]) or _bad(det))


def transfer(M, x, y, u, v):
    """(e, w w) of (x, y, 1) under M against (u, v); floats or arrays"""
    U = (M[0] * x + M[1] * y) + M[2]
    V = (M[3] * x + M[4] * y) + M[5]
    w = (M[6] * x + M[7] * y) + M[8]
    du, dv = U - u * w, V - v * w
    return du * du + dv * dv, w * w


def inliers(H, G, x1, y1, x2, y2, t):
    """forward and backward pass masks of the division-free test (a NaN fails)"""
    with np.errstate(all="ignore"):
        e, ww = transfer(H, x1, y1, x2, y2)
        f = e <= t * ww
        e, ww = transfer(G, x2, y2, x1, y1)
        return f, e <= t * ww


def solve4(s1x, s1y, s2x, s2y, t_self=None):
    """(H, G, ok) of four correspondences (lists of Python floats): H = B adj(A), G = adj(H); ok is False for a degenerate basis or, with
    t_self, when one of the eight transfer tests of the sample fails"""
    A, ok_a = basis(s1x, s1y)
    B, ok_b = basis(s2x, s2y)
    if not (ok_a and ok_b):
        return None, None, False
    Aa = adj(A)
    H = [(B[3 * r] * Aa[c] + B[3 * r + 1] * Aa[3 + c]) + B[3 * r + 2] * Aa[6 + c] for r in range(3) for c in range(3)]
    G = adj(H)
    if t_self is not None:
        for k in range(4):
            e, ww = transfer(H, s1x[k], s1y[k], s2x[k], s2y[k])
            if not e <= t_self * ww:
                return H, G, False
            e, ww = transfer(G, s2x[k], s2y[k], s1x[k], s1y[k])
            if not e <= t_self * ww:
                return H, G, False
    return H, G, True


def sample_indices(draws, j, m):
    return [int(int(draws[j, k]) & 0x7fffffff) % m for k in range(4)]


def hypothesis(n, draws, j, m, t_self):
    idx = sample_indices(draws, j, m)
    if len(set(idx)) < 4:
        return None, None, False
    g = lambda a: [float(a[i]) for i in idx]
    return solve4(g(n[0]), g(n[1]), g(n[2]), g(n[3]), t_self)


def iterations(cam, hp, x1, x2, draws, iters=None, self_check=True):
    """(live bool[iters], count int[iters]) of every iteration of the table on one pair (m >= 4)"""
    iters = int(hp.iters) if iters is None else iters
    m = len(x1)
    _, _, t_h, _, t_self = thresholds(cam, hp)
    n = normalise(cam, x1, x2)
    live, cnt = np.zeros(iters, bool), np.zeros(iters, np.int64)
    for j in range(iters):
        H, G, ok = hypothesis(n, draws, j, m, t_self if self_check else None)
        if ok:
            f, b = inliers(H, G, n[0], n[1], n[2], n[3], t_h)
            live[j], cnt[j] = True, int((f & b).sum())
    return live, cnt


def pick(live, cnt, iters):
    """(best_iter or -1, n_degenerate) of the first `iters` iterations: the first one with the largest count > 0"""
    l, c = live[:iters], np.where(live[:iters], cnt[:iters], 0)
    best = int(np.argmax(c)) if len(c) and c.max() > 0 else -1
    return best, int(iters - l.sum())


def wave_sum(terms):
    """the kernel's summation order over per-point terms"""
    n = len(terms)
    pad = np.zeros(((n + 63) // 64) * 64)
    pad[:n] = terms
    acc = np.zeros(64)
    for row in pad.reshape(-1, 64):
        acc = acc + row
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return float(acc[0])


def finish(cam, hp, x1, x2, draws, best, ndeg, E=None, self_check=True):
    """(record, mask) from the winning iteration: mask, scores, decision, normalisation"""
    m = len(x1)
    fx_inv, s2, t_h, t_e, t_self = thresholds(cam, hp)
    n = normalise(cam, x1, x2)
    r = zero_record()
    r["n_points"], r["n_degenerate"], r["best_iter"] = m, ndeg, best
    mask = np.zeros(m, np.uint8)
    sh = se = 0.0
    nin = nine = 0
    with np.errstate(all="ignore"):
        if best >= 0:
            H, G, _ = hypothesis(n, draws, best, m, t_self if self_check else None)
            e, ww = transfer(H, n[0], n[1], n[2], n[3])
            f, df = e <= t_h * ww, e / ww
            e, ww = transfer(G, n[2], n[3], n[0], n[1])
            b, db = e <= t_h * ww, e / ww
            tf = np.where(df <= t_h, hp.chi2_h - df / s2, 0.0)
            tb = np.where(db <= t_h, hp.chi2_h - db / s2, 0.0)
            sh = wave_sum(tf + tb)
            mask = (f & b).astype(np.uint8)
            nin = int(mask.sum())
        if E is not None:
            Ee = [float(v) for v in np.asarray(E, np.float64).reshape(9)]
            l2a = (Ee[0] * n[0] + Ee[1] * n[1]) + Ee[2]
            l2b = (Ee[3] * n[0] + Ee[4] * n[1]) + Ee[5]
            l2c = (Ee[6] * n[0] + Ee[7] * n[1]) + Ee[8]
            l1a = (Ee[0] * n[2] + Ee[3] * n[3]) + Ee[6]
            l1b = (Ee[1] * n[2] + Ee[4] * n[3]) + Ee[7]
            rr = (n[2] * l2a + n[3] * l2b) + l2c
            r2 = rr * rr
            n2, n1 = l2a * l2a + l2b * l2b, l1a * l1a + l1b * l1b
            i2, i1 = (n2 > 0.0) & (r2 <= t_e * n2), (n1 > 0.0) & (r2 <= t_e * n1)
            t2 = np.where(i2, hp.chi2_h - (r2 / n2) / s2, 0.0)
            t1 = np.where(i1, hp.chi2_h - (r2 / n1) / s2, 0.0)
            se = wave_sum(t2 + t1)
            nine = int((i2 & i1).sum())
        r["score_h"], r["score_e"], r["n_inliers"], r["n_inliers_e"] = sh, se, nin, nine
        offer_h = best >= 0 and nin >= hp.min_inliers
        offer_e = E is not None and nine >= hp.min_inliers
        r["model"] = MODEL_HOMOGRAPHY if offer_h and (not offer_e or sh > hp.h_ratio * (sh + se)) else MODEL_ESSENTIAL if offer_e else MODEL_NONE
        if best >= 0:
            det = (H[0] * G[0] + H[1] * G[3]) + H[2] * G[6]
            ss = H[0] * H[0]
            for k in range(1, 9):
                ss = ss + H[k] * H[k]
            nrm = np.sqrt(np.float64(ss))
            sg = -1.0 if det < 0.0 else 1.0
            r["H"] = np.array([sg * h for h in H], np.float64) / nrm
    return r, mask


def homography(cam, hp, x1, x2, draws, E=None, self_check=True):
    """(record, mask) of one pair: what vis_find_homography returns"""
    m = len(x1)
    if m < 4 or hp.iters == 0:
        return zero_record(), np.zeros(m, np.uint8)
    live, cnt = iterations(cam, hp, x1, x2, draws, self_check=self_check)
    best, ndeg = pick(live, cnt, int(hp.iters))
    return finish(cam, hp, x1, x2, draws, best, ndeg, E, self_check)


def ratio(rec):
    s = float(rec["score_h"]) + float(rec["score_e"])
    return float(rec["score_h"]) / s if s > 0 else float("nan")


def margin(rec, hp):
    s = float(rec["score_h"]) + float(rec["score_e"])
    return abs(float(rec["score_h"]) - hp.h_ratio * s) / s if s > 0 else float("nan")


# ---- the independent method -----------------------------------------------------------------------------------------------------
def dlt_svd(s1x, s1y, s2x, s2y):
    """H (9,) of four correspondences: the right singular vector of the smallest singular value of the 8 x 9 DLT matrix"""
    rows = []
    for x, y, u, v in zip(s1x, s1y, s2x, s2y):
        rows.append([-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u])
        rows.append([0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v])
    return np.linalg.svd(np.array(rows, np.float64))[2][-1]


def unit_diff(Ha, Hb):
    """largest element difference of two homographies scaled to unit norm, sign matched"""
    a, b = np.asarray(Ha, np.float64).reshape(9), np.asarray(Hb, np.float64).reshape(9)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    s = 1.0 if float((a * b).sum()) >= 0 else -1.0
    return float(np.abs(a - s * b).max())


def winner_sample(cam, x1, x2, draws, best):
    n = normalise(cam, x1, x2)
    idx = sample_indices(draws, best, len(x1))
    return [[float(a[i]) for i in idx] for a in n]


def transfer_residual_px2(cam, H, s):
    """the largest squared forward transfer residual (pixels^2) of a homography on four correspondences"""
    worst = 0.0
    for k in range(4):
        e, ww = transfer(H, s[0][k], s[1][k], s[2][k], s[3][k])
        worst = max(worst, e / ww * cam.fx * cam.fx)
    return worst


# ---- the case lists -------------------------------------------------------------------------------------------------------------
def table_cases():
    """(cls, m, noise, outliers) of the classification table: 13 classes x 2 x 2 x 2"""
    return [(c, m, nz, o) for c in pdc.CLASSES for m in (40, 300) for nz in (0.0, 0.3) for o in (0.0, 0.25)]


def gpu_rows(tile):
    """(cls, m) of the device rows: every class at the small sizes (below, at and above the four-point minimum), three classes around the
    tile"""
    return [(c, m) for m in (3, 4, 5, 8, 40) for c in pdc.CLASSES] + \
           [(c, m) for m in (tile - 1, tile, tile + 1, 2 * tile + 7) for c in ("general", "plane", "static")]
