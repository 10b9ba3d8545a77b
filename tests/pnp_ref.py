"""PnP of include/vislam_hip.h (vis_pnp_ransac / vis_pnp_batch), restated operation for operation; the scene builder; independent
methods.  Not a test module: shared by tests/test_pnp_ref.py (CPU), tests/test_pnp_abi.py and tests/test_pnp_gpu.py.

Everything runs on IEEE doubles with one rounding per operation and no contraction, in the kernels' parenthesisation (csrc/pnp.hip): the
solver is element-wise float64 numpy over the samples (the kernel's lanes), the per-point work element-wise numpy over the points, the
6 x 6 solve and the pose update plain Python floats.  The sums of the refinement are taken in the kernel's order: 64 partial sums over
i mod 64 in rising i, then the butterfly v = v + v[lane ^ off], off = 32 ... 1.

The independent methods are textbook ones: numpy.roots on the quartic and numpy.linalg.svd (Kabsch) for the rotation between the two point
triples; a Gauss-Newton with a Rodrigues update and numpy.linalg.lstsq for the refinement."""
import ctypes as C

import numpy as np

import pose_degenerate_cases as pdc

REFINED, REFINE_REJECTED, FEW = 1, 2, 4
INNER, FINAL = 40, 100
CLASSES = ("general", "plane", "tilted", "static", "dup", "far", "line")
REGULAR = ("general", "plane", "tilted", "static", "dup")             # every planted inlier must be found
W_PX, H_PX = 752, 480                                                  # where the planted outliers are drawn
DBL_MAX = 1.7976931348623157e308

RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("R_ransac", "<f8", (9,)), ("t_ransac", "<f8", (3,)), ("cost0", "<f8"),
                         ("cost1", "<f8"), ("n_inliers", "<i4"), ("n_points", "<i4"), ("best_iter", "<i4"), ("best_root", "<i4"),
                         ("n_degenerate", "<i4"), ("n_solutions", "<i4"), ("n_inliers_refined", "<i4"), ("flags", "<i4")])


class Params(C.Structure):
    """vis_pnp_params with its defaults, for callers without the library (CPU tests)"""
    _fields_ = [("iters", C.c_int32), ("min_inliers", C.c_int32), ("threshold_px", C.c_double), ("refine_iters", C.c_int32), ("reserved_", C.c_int32)]


def default_params():
    return Params(200, 8, 2.0, 5, 0)


class Camera:
    def __init__(self, fx=pdc.FOCAL, cx=pdc.CX, cy=pdc.CY):
        self.fx, self.cx, self.cy = float(fx), float(cx), float(cy)


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["best_iter"] = -1
    return r


def make_draws(seed, iters=200):
    return np.random.default_rng(seed).integers(0, 2 ** 31, (iters, 3)).astype(np.int32)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def make_scene(cls, m, noise, outliers, seed=None):
    """(X m x 3 float64 map points, xy m x 2 float32 pixels, planted bool[m], R, t): points in the style of pose_degenerate_cases.make_case
    seen from a camera posed by a random (R, t), |w| ~ 0.1 rad, |t| ~ 0.9 (`static`: the identity); noise in pixels; the first `outliers`
    share of the pixels replaced by uniform ones of a 752 x 480 image"""
    rng = np.random.default_rng([41, CLASSES.index(cls), m, int(round(10 * noise)), int(round(100 * outliers))] + ([] if seed is None else [int(seed)]))
    w = rng.normal(0, 1, 3)
    R = pdc._rodrigues(0.1 * w / np.linalg.norm(w))
    t = rng.normal(0, 1, 3)
    t *= 0.9 / np.linalg.norm(t)
    if cls == "static":
        R, t = np.eye(3), np.zeros(3)
    n = 6 if cls == "dup" else m
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4.0, 12.0, n)], 1)
    if cls == "plane":
        X[:, 2] = 6.0
    elif cls == "tilted":
        X[:, 2] = 6.0 + 0.4 * X[:, 0] + 0.2 * X[:, 1]
    elif cls == "line":
        s = rng.uniform(-1, 1, n)
        X = np.array([0.3, -0.2, 7.0]) + s[:, None] * np.array([2.5, 1.0, 2.0])
    elif cls == "far":
        X[:, 2] = 1e6
        X[:, :2] *= 1e6 / 8.0
    xy = pdc._project(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    if cls == "dup":                                                   # six correspondences, repeated
        pick6 = rng.integers(0, 6, m)
        X, xy = X[pick6], xy[pick6]
    k = int(outliers * m)
    planted = np.ones(m, bool)
    if k:
        xy[:k] = np.stack([rng.uniform(0, W_PX, k), rng.uniform(0, H_PX, k)], 1)
        planted[:k] = False
    return np.ascontiguousarray(X, np.float64), np.ascontiguousarray(xy, np.float32), planted, R, t


def table_cases():
    """(cls, m, noise, outliers): 7 classes x 2 x 2 x 2"""
    return [(c, m, nz, o) for c in CLASSES for m in (40, 300) for nz in (0.0, 0.3) for o in (0.0, 0.25)]


# ---- the restatement: solver ------------------------------------------------------------------------------------------------------
def thresholds(cam, pp):
    """(fx_inv, thr2) as the host computes them, in double"""
    fx_inv = 1.0 / cam.fx
    s = pp.threshold_px * fx_inv
    return fx_inv, s * s


def normalise(cam, xy):
    """the pose stage's coordinates: ((double)u - c) * (1 / fx), two float64 arrays"""
    fx_inv = 1.0 / cam.fx
    a = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    return (a[:, 0] - cam.cx) * fx_inv, (a[:, 1] - cam.cy) * fx_inv


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _finite(v):
    return np.abs(v) <= DBL_MAX


def _horner(q, D, x):
    r = q[D]
    for i in range(D - 1, -1, -1):
        r = r * x + q[i]
    return r


def _level(q, D, nit, B, prev, nprev, ok):
    """one level of the derivative-interlacing root finder over all samples: (cur[4], ncur)"""
    S = len(B)
    cur, ncur = [np.zeros(S) for _ in range(4)], np.zeros(S, np.int64)
    for j in range(D):
        lo = np.zeros(S) if j == 0 else prev[j - 1].copy()
        hi = np.where(nprev == j, B, prev[j])
        flo, fhi = _horner(q, D, lo), _horner(q, D, hi)
        found = ok & (j <= nprev) & ((flo < 0.0) != (fhi < 0.0))
        act = found.copy()
        for _ in range(nit):
            mid = 0.5 * (lo + hi)
            act = act & (mid > lo) & (mid < hi)
            if not act.any():
                break
            fm = _horner(q, D, mid)
            left = (fm < 0.0) == (flo < 0.0)
            lo, hi = np.where(act & left, mid, lo), np.where(act & ~left, mid, hi)
        root = 0.5 * (lo + hi)
        for k in range(4):
            cur[k] = np.where(found & (ncur == k), root, cur[k])
        ncur = ncur + found
    return cur, ncur


def quartic_roots(c, B, ok=None):
    """(roots[4], n): ascending real roots in (0, B) of c[0] + ... + c[4] v^4, arrays over the samples"""
    S = len(B)
    ok = np.ones(S, bool) if ok is None else ok
    z = np.zeros(S)
    q3 = [6.0 * c[3], 24.0 * c[4]]
    q2 = [2.0 * c[2], 6.0 * c[3], 12.0 * c[4]]
    q1 = [c[1], 2.0 * c[2], 3.0 * c[3], 4.0 * c[4]]
    with np.errstate(all="ignore"):
        r3, n3 = _level(q3, 1, INNER, B, [z, z, z, z], np.zeros(S, np.int64), ok)
        r2, n2 = _level(q2, 2, INNER, B, r3, n3, ok)
        r1, n1 = _level(q1, 3, INNER, B, r2, n2, ok)
        return _level(c, 4, FINAL, B, r1, n1, ok)


def sample_indices(draws, iters, m):
    d = np.asarray(draws, np.int32).reshape(-1, 3)[:iters].astype(np.int64)
    return (d & 0x7fffffff) % m


def coefficients(X, x, y, idx):
    """everything the roots share, arrays over the samples: a dict with the quartic c[5], the skip mask `ok` (before the root finder) and the
    sample's geometry"""
    P = [[X[idx[:, k], a] for a in range(3)] for k in range(3)]
    f = []
    for k in range(3):
        xs, ys = x[idx[:, k]], y[idx[:, k]]
        n = np.sqrt((xs * xs + ys * ys) + 1.0)
        f.append([xs / n, ys / n, 1.0 / n])
    p01 = [P[1][a] - P[0][a] for a in range(3)]
    p02 = [P[2][a] - P[0][a] for a in range(3)]
    p12 = [P[2][a] - P[1][a] for a in range(3)]
    c2, b2, a2 = _dot3(p01, p01), _dot3(p02, p02), _dot3(p12, p12)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (b2 != 0.0)
    ca, cb, cg = _dot3(f[1], f[2]), _dot3(f[0], f[2]), _dot3(f[0], f[1])
    p, q, ra, rc, rbc, rba = (a2 - c2) / b2, (a2 + c2) / b2, a2 / b2, c2 / b2, (b2 - c2) / b2, (b2 - a2) / b2
    ca2, cb2, cg2, pm1, pp1, omq, p2 = ca * ca, cb * cb, cg * cg, p - 1.0, 1.0 + p, 1.0 - q, p * p
    c = [None] * 5
    c[4] = pm1 * pm1 - (4.0 * rc) * ca2
    c[3] = 4.0 * (((p * (1.0 - p)) * cb - (omq * ca) * cg) + ((2.0 * rc) * ca2) * cb)
    c[2] = 2.0 * (((((p2 - 1.0) + (2.0 * p2) * cb2) + (2.0 * rbc) * ca2) - (((4.0 * q) * ca) * cb) * cg) + (2.0 * rba) * cg2)
    c[1] = 4.0 * ((((-p) * pp1) * cb + ((2.0 * ra) * cg2) * cb) - (omq * ca) * cg)
    c[0] = pp1 * pp1 - (4.0 * ra) * cg2
    ok = ok & _finite(c[0]) & _finite(c[1]) & _finite(c[2]) & _finite(c[3]) & _finite(c[4]) & (c[4] != 0.0)
    nw = _cross3(p01, p02)
    nnw = _dot3(nw, nw)
    ok = ok & (nnw > (2.0 ** -40 * c2) * b2)
    B = np.abs(c[0] / c[4])
    for k in range(1, 4):
        v = np.abs(c[k] / c[4])
        B = np.where(v > B, v, B)
    B = B + 1.0
    ok = ok & _finite(B)
    lc, lw = np.sqrt(c2), np.sqrt(nnw)
    e1, e3 = [p01[a] / lc for a in range(3)], [nw[a] / lw for a in range(3)]
    e2 = _cross3(e3, e1)
    return dict(c=c, B=B, ok=ok, P0=P[0], f=f, e=(e1, e2, e3), a2=a2, b2=b2, c2=c2, p=p, pm1=pm1, ca=ca, cb=cb, cg=cg)


def solution(G, v):
    """(pose[12] arrays, live) of root v (an array over the samples)"""
    den = 2.0 * (G["cg"] - v * G["ca"])
    live = (den != 0.0) & _finite(den)
    u = (((G["pm1"] * (v * v) - ((2.0 * G["p"]) * G["cb"]) * v) + 1.0) + G["p"]) / den
    live = live & (v > 0.0) & (u > 0.0)
    w = (1.0 + v * v) - (2.0 * v) * G["cb"]
    live = live & (w > 0.0)
    s0 = np.sqrt(G["b2"] / w)
    s1, s2 = u * s0, v * s0
    f0, f1, f2 = G["f"]
    Q0 = [s0 * f0[a] for a in range(3)]
    q01 = [s1 * f1[a] - Q0[a] for a in range(3)]
    q02 = [s2 * f2[a] - Q0[a] for a in range(3)]
    nq = _cross3(q01, q02)
    l1, l2, nn = _dot3(q01, q01), _dot3(q02, q02), _dot3(nq, nq)
    live = live & (nn > (2.0 ** -40 * l1) * l2)
    n1, n3 = np.sqrt(l1), np.sqrt(nn)
    g1, g3 = [q01[a] / n1 for a in range(3)], [nq[a] / n3 for a in range(3)]
    g2 = _cross3(g3, g1)
    e1, e2, e3 = G["e"]
    P = [None] * 12
    for r in range(3):
        for cc in range(3):
            P[3 * r + cc] = (g1[r] * e1[cc] + g2[r] * e2[cc]) + g3[r] * e3[cc]
        P[9 + r] = Q0[r] - ((P[3 * r] * G["P0"][0] + P[3 * r + 1] * G["P0"][1]) + P[3 * r + 2] * G["P0"][2])
    return P, live


def transform(P, X):
    """(U, V, W) = R X + t; P: 12 scalars or column arrays, X: m x 3"""
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    U = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[9]
    V = ((P[3] * X0 + P[4] * X1) + P[5] * X2) + P[10]
    W = ((P[6] * X0 + P[7] * X1) + P[8] * X2) + P[11]
    return U, V, W


def inliers(P, X, x, y, thr2):
    with np.errstate(all="ignore"):
        U, V, W = transform(P, X)
        du, dv = U - x * W, V - y * W
        rhs = thr2 * (W * W)
        return (W > 0.0) & _finite(rhs) & ((du * du + dv * dv) <= rhs)


def hypotheses(cam, pp, X, xy, draws, iters=None, count=True):
    """every sample of the table on one problem (m >= 4): dict(live (S, 4), cnt (S, 4), poses (S, 4, 12), ok (S,), roots (S, 4), nroots, geo)"""
    iters = int(pp.iters) if iters is None else iters
    X = np.asarray(X, np.float64).reshape(-1, 3)
    m = len(X)
    _, thr2 = thresholds(cam, pp)
    x, y = normalise(cam, xy)
    idx = sample_indices(draws, iters, m)
    S = len(idx)
    with np.errstate(all="ignore"):
        G = coefficients(X, x, y, idx)
        roots, nr = quartic_roots(G["c"], G["B"], G["ok"])
        live, cnt, poses = np.zeros((S, 4), bool), np.zeros((S, 4), np.int64), np.zeros((S, 4, 12))
        for r in range(4):
            P, lv = solution(G, roots[r])
            lv = lv & G["ok"] & (r < nr)
            live[:, r] = lv
            for k in range(12):
                poses[:, r, k] = np.where(lv, P[k], 0.0)
            if count:
                cnt[:, r] = inliers([poses[:, r, k][:, None] for k in range(12)], X, x[None, :], y[None, :], thr2).sum(1)
    return dict(live=live, cnt=cnt, poses=poses, ok=G["ok"], roots=np.stack(roots, 1), nroots=nr, geo=G, idx=idx)


def pick(hyp, iters):
    """(winning slot h = 4 j + r or -1, n_degenerate, n_solutions) of the first `iters` samples: the first slot with the largest count > 0"""
    live, cnt = hyp["live"][:iters], hyp["cnt"][:iters]
    c = np.where(live, cnt, 0).reshape(-1)
    h = int(np.argmax(c)) if len(c) and c.max() > 0 else -1
    return h, int((~live.any(1)).sum()), int(live.sum())


# ---- the restatement: refinement --------------------------------------------------------------------------------------------------
def wave_sums(terms):
    """the kernel's summation order over per-point rows of terms (m x K): K sums"""
    n, K = terms.shape
    pad = np.zeros((((n + 63) // 64) * 64, K))
    pad[:n] = terms
    acc = np.zeros((64, K))
    for blk in pad.reshape(-1, 64, K):
        acc = acc + blk
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return [float(v) for v in acc[0]]


def gn_pass(P0, P, X, x, y, thr2):
    """(28 sums, points that pass under P): the upper triangle of J^T J in row order, J^T r, the cost, over the inliers of P0"""
    with np.errstate(all="ignore"):
        inl = inliers(P0, X, x, y, thr2)
        n = int(inliers(P, X, x, y, thr2).sum())
        U, V, W = transform(P, X)
        iw, un, vn = 1.0 / W, U / W, V / W
        rx, ry = un - x, vn - y
        j02, j12 = -(un * iw), -(vn * iw)
        z = np.zeros(len(X))
        J0 = [j02 * V, iw * W - j02 * U, -(iw * V), iw, z, j02]
        J1 = [j12 * V - iw * W, -(j12 * U), iw * U, z, iw, j12]
        cols = [J0[a] * J0[b] + J1[a] * J1[b] for a in range(6) for b in range(a, 6)]
        cols += [J0[a] * rx + J1[a] * ry for a in range(6)]
        cols.append(rx * rx + ry * ry)
        terms = np.where(inl[:, None], np.stack(cols, 1), 0.0)
    return wave_sums(terms), n


def solve6(S):
    """(d[6], ok): d = -(J^T J)^-1 J^T r by LDL^T without pivoting, on Python floats"""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = S[k]
            k += 1
    L, D, z, d = [[0.0] * 6 for _ in range(6)], [0.0] * 6, [0.0] * 6, [0.0] * 6
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            s = np.float64(A[j][j])
            for c in range(j):
                s = s - (L[j][c] * L[j][c]) * D[c]
            D[j] = s
            ok = ok and bool(s > 0.0) and bool(abs(s) <= DBL_MAX)
            for i in range(j + 1, 6):
                v = np.float64(A[i][j])
                for c in range(j):
                    v = v - (L[i][c] * L[j][c]) * D[c]
                L[i][j] = v / s
        for i in range(6):
            v = np.float64(-S[21 + i])
            for c in range(i):
                v = v - L[i][c] * z[c]
            z[i] = v
        for i in range(5, -1, -1):
            v = z[i] / D[i]
            for c in range(i + 1, 6):
                v = v - L[c][i] * d[c]
            d[i] = v
    return [float(v) for v in d], ok


def cayley_update(P, d):
    """R <- C R, t <- C t + d[3:6] with C = I + 2 / (1 + |h|^2) ([h]x + [h]x^2), h = d[0:3] / 2"""
    h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    hh = _dot3(h, h)
    s = 2.0 / (1.0 + hh)
    K = [0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0]
    Cm = [0.0] * 9
    for i in range(3):
        for j in range(3):
            k2 = h[i] * h[j] - hh if i == j else h[i] * h[j]
            Cm[3 * i + j] = (1.0 if i == j else 0.0) + s * (K[3 * i + j] + k2)
    N = [0.0] * 12
    for i in range(3):
        for j in range(3):
            N[3 * i + j] = (Cm[3 * i] * P[j] + Cm[3 * i + 1] * P[3 + j]) + Cm[3 * i + 2] * P[6 + j]
        N[9 + i] = ((Cm[3 * i] * P[9] + Cm[3 * i + 1] * P[10]) + Cm[3 * i + 2] * P[11]) + d[3 + i]
    return N


def finish(cam, pp, X, xy, hyp, h, ndeg, nsol):
    """(record, mask) from the winning slot: mask, counts, refinement"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    m = len(X)
    _, thr2 = thresholds(cam, pp)
    x, y = normalise(cam, xy)
    r = zero_record()
    r["n_points"], r["n_degenerate"], r["n_solutions"] = m, ndeg, nsol
    mask = np.zeros(m, np.uint8)
    if h < 0:
        return r, mask
    P0 = [float(v) for v in hyp["poses"][h >> 2, h & 3]]
    mask = inliers(P0, X, x, y, thr2).astype(np.uint8)
    nin = int(mask.sum())
    r["best_iter"], r["best_root"], r["n_inliers"], r["n_inliers_refined"] = h >> 2, h & 3, nin, nin
    r["R"] = r["R_ransac"] = P0[:9]
    r["t"] = r["t_ransac"] = P0[9:]
    flags = FEW if nin < pp.min_inliers else 0
    S, _ = gn_pass(P0, P0, X, x, y, thr2)
    cost0 = cost1 = S[27]
    if pp.refine_iters > 0 and nin >= pp.min_inliers:
        P, ok = list(P0), True
        for step in range(int(pp.refine_iters)):
            if step > 0:
                S, _ = gn_pass(P0, P, X, x, y, thr2)
            d, ok = solve6(S)
            if not ok:
                break
            P = cayley_update(P, d)
        S, n1 = gn_pass(P0, P, X, x, y, thr2)
        cost1 = S[27]
        refined = ok and abs(cost1) <= DBL_MAX and cost1 <= cost0
        flags |= REFINED if refined else REFINE_REJECTED
        if refined:
            r["R"], r["t"], r["n_inliers_refined"] = P[:9], P[9:], n1
    r["cost0"], r["cost1"], r["flags"] = cost0, cost1, flags
    return r, mask


def pnp(cam, pp, X, xy, draws):
    """(record, mask) of one problem: what vis_pnp_ransac returns"""
    m = len(np.asarray(X).reshape(-1, 3))
    if m < 4 or pp.iters == 0:
        return zero_record(), np.zeros(m, np.uint8)
    hyp = hypotheses(cam, pp, X, xy, draws)
    return finish(cam, pp, X, xy, hyp, *pick(hyp, int(pp.iters)))


# ---- the join of vis_batch_pnp ------------------------------------------------------------------------------------------------------
NO_MAP = 1
KF_CARRIED, KF_NOT_SAVED, KF_FIRST = -1, -2, -3
LINK_DTYPE = np.dtype([("R_rel", "<f8", (9,)), ("t_rel", "<f8", (3,)), ("scale", "<f8"), ("n_linked", "<i4"), ("q", "<i4"), ("p", "<i4"),
                       ("flags", "<i4")])


def join(match_qi, match_pq, flags_q, require):
    """[(c, k)] in rising c: correspondence c of pair (q -> i) and the FIRST correspondence k of pair (p -> q) with the same keypoint in frame q
    (trainIdx of k == queryIdx of c) whose flags contain `require`"""
    first = {}
    for k, mk in enumerate(match_pq):
        kp = int(mk["trainIdx"])
        if (int(flags_q[k]) & require) == require and kp not in first:
            first[kp] = k
    return [(c, first[int(mc["queryIdx"])]) for c, mc in enumerate(match_qi) if int(mc["queryIdx"]) in first]


def link_rows(i, prev, matches, poses, points, flags, xy2, require):
    """(X, xy, link record) of frame i: prev = vis_batch_get_keyframes' table, matches[j] / poses[j] / points[j] / flags[j] = pair j's match list,
    pose record, map point rows and flag rows, xy2[j] = the pixels of pair j's correspondences in frame j"""
    L = np.zeros(1, LINK_DTYPE)[0]
    q = int(prev[i])
    p = int(prev[q]) if 0 <= q < len(prev) else q
    L["q"], L["p"], L["flags"] = q, p, NO_MAP if q == KF_CARRIED else 0
    X, xy = np.zeros((0, 3)), np.zeros((0, 2), np.float32)
    if q >= 0 and np.any(np.asarray(poses[q]["R"]) != 0):
        pairs = join(matches[i], matches[q], flags[q], require)
        if pairs:
            X = np.stack([points[q][k]["X"] for _, k in pairs]).astype(np.float64)
            xy = np.stack([xy2[i][c] for c, _ in pairs]).astype(np.float32)
        L["n_linked"] = len(pairs)
    return X, xy, L


def link_motion(L, rec, pose_q):
    """the link record with R_rel, t_rel and scale of a frame whose PnP record has a winner"""
    L = L.copy()
    if int(rec["best_iter"]) < 0 or int(L["q"]) < 0:
        return L
    R, t = [float(v) for v in rec["R"]], [float(v) for v in rec["t"]]
    Rq, tq = [float(v) for v in pose_q["R"]], [float(v) for v in pose_q["t"]]
    Rr = [(R[3 * r] * Rq[3 * c] + R[3 * r + 1] * Rq[3 * c + 1]) + R[3 * r + 2] * Rq[3 * c + 2] for r in range(3) for c in range(3)]
    tr = [t[r] - ((Rr[3 * r] * tq[0] + Rr[3 * r + 1] * tq[1]) + Rr[3 * r + 2] * tq[2]) for r in range(3)]
    L["R_rel"], L["t_rel"], L["scale"] = Rr, tr, np.sqrt(np.float64(_dot3(tr, tr)))
    return L


# ---- the independent methods ------------------------------------------------------------------------------------------------------
def p3p_independent(P, f):
    """poses [(R, t)] of one sample by numpy.roots on the quartic and Kabsch (numpy.linalg.svd) on the two triples; P: 3 x 3 world points,
    f: 3 x 3 unit bearings"""
    P, f = np.asarray(P, np.float64), np.asarray(f, np.float64)
    a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    p, q = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (p - 1) ** 2 - 4 * c2 / b2 * ca ** 2
    A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb)
    A2 = 2 * (p ** 2 - 1 + 2 * p ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * q * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2)
    A1 = 4 * (-p * (1 + p) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - q) * ca * cg)
    A0 = (1 + p) ** 2 - 4 * a2 / b2 * cg ** 2
    out = []
    for v in np.roots([A4, A3, A2, A1, A0]):
        if abs(v.imag) > 1e-9 * max(1.0, abs(v.real)) or v.real <= 0:
            continue
        v = v.real
        u = ((p - 1) * v * v - 2 * p * cb * v + 1 + p) / (2 * (cg - v * ca))
        w = 1 + v * v - 2 * v * cb
        if not (u > 0 and w > 0):
            continue
        s0 = np.sqrt(b2 / w)
        Q = np.stack([s0 * f[0], u * s0 * f[1], v * s0 * f[2]])
        Pc, Qc = P - P.mean(0), Q - Q.mean(0)
        n_p, n_q = np.cross(Pc[1] - Pc[0], Pc[2] - Pc[0]), np.cross(Qc[1] - Qc[0], Qc[2] - Qc[0])
        Pa, Qa = np.vstack([Pc, n_p / np.linalg.norm(n_p)]), np.vstack([Qc, n_q / np.linalg.norm(n_q)])   # the normals fix the reflection
        Uu, _, Vt = np.linalg.svd(Qa.T @ Pa)
        R = Uu @ np.diag([1.0, 1.0, np.linalg.det(Uu @ Vt)]) @ Vt
        out.append((R, Q.mean(0) - R @ P.mean(0)))
    return out


def solution_residuals(R, t, P, f):
    """how well a pose satisfies the equations of its own sample: (largest relative side error of |Q_i - Q_j|^2 against the world triangle,
    largest sine between R P_k + t and f_k, max |R^T R - I|, |det R - 1|)"""
    R, t, P, f = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64), np.asarray(P, np.float64), np.asarray(f, np.float64)
    Q = P @ R.T + t
    side = max(abs(((Q[i] - Q[j]) ** 2).sum() - ((P[i] - P[j]) ** 2).sum()) / ((P[i] - P[j]) ** 2).sum() for i, j in ((0, 1), (0, 2), (1, 2)))
    par = max(float(np.linalg.norm(np.cross(Q[k], f[k])) / np.linalg.norm(Q[k])) for k in range(3))
    return side, par, float(np.abs(R.T @ R - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))


def bearings(cam, xy):
    x, y = normalise(cam, xy)
    f = np.stack([x, y, np.ones_like(x)], 1)
    return f / np.linalg.norm(f, axis=1)[:, None]


def ransac_independent(cam, pp, X, xy, draws):
    """(R, t, mask) of the best pose the independent solver finds over the same samples, counted with a plain pixel-distance test"""
    X = np.asarray(X, np.float64)
    f, m = bearings(cam, xy), len(X)
    px = np.asarray(xy, np.float32).astype(np.float64)
    best = (None, None, np.zeros(m, bool))
    for idx in sample_indices(draws, int(pp.iters), m):
        if len(set(idx.tolist())) < 3:
            continue
        P = X[idx]
        nrm = np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0]))
        if not nrm > 2.0 ** -20 * np.linalg.norm(P[1] - P[0]) * np.linalg.norm(P[2] - P[0]):
            continue
        for R, t in p3p_independent(P, f[idx]):
            Y = X @ R.T + t
            with np.errstate(all="ignore"):
                e = np.hypot(cam.fx * Y[:, 0] / Y[:, 2] + cam.cx - px[:, 0], cam.fx * Y[:, 1] / Y[:, 2] + cam.cy - px[:, 1])
                msk = (Y[:, 2] > 0) & (e <= pp.threshold_px)
            if msk.sum() > best[2].sum():
                best = (R, t, msk)
    return best


def gn_independent(cam, X, xy, mask, R, t, iters=20):
    """(R, t) of a Gauss-Newton with a Rodrigues update and numpy.linalg.lstsq over the masked points (pixel residuals)"""
    X, px = np.asarray(X, np.float64)[mask.astype(bool)], np.asarray(xy, np.float32).astype(np.float64)[mask.astype(bool)]
    R, t = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    for _ in range(iters):
        Y = X @ R.T + t
        r = np.stack([cam.fx * Y[:, 0] / Y[:, 2] + cam.cx - px[:, 0], cam.fx * Y[:, 1] / Y[:, 2] + cam.cy - px[:, 1]], 1).reshape(-1)
        U, V, W = Y[:, 0], Y[:, 1], Y[:, 2]
        z = np.zeros(len(X))
        Jp = cam.fx * np.stack([np.stack([1 / W, z, -U / W ** 2], 1), np.stack([z, 1 / W, -V / W ** 2], 1)], 1)        # n x 2 x 3
        Yx = np.stack([np.stack([z, -W, V], 1), np.stack([W, z, -U], 1), np.stack([-V, U, z], 1)], 1)               # n x 3 x 3
        J = np.concatenate([-Jp @ Yx, Jp], 2).reshape(-1, 6)
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        dR = pdc._rodrigues(d[:3])
        R, t = dR @ R, dR @ t + d[3:]
    return R, t


def rot_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def rot_diff(Ra, Rb):
    """|Ra Rb^T - I| (Frobenius): a rotation distance that does not lose small angles to arccos"""
    return float(np.linalg.norm(np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T - np.eye(3)))
