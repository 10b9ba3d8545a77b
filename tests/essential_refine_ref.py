"""The two-view refinement of include/vislam_hip.h (vis_essential_refine / _batch / vis_batch_essential_refine), restated operation for
operation; the scene builder; an independent minimiser.  Not a test module: shared by tests/test_essential_refine_ref.py (CPU),
tests/test_essential_refine_abi.py, tests/test_essential_refine_gpu.py and tests/test_essential_batch_gpu.py.

Everything runs on IEEE doubles with one rounding per operation and no contraction, in the kernel's parenthesisation (csrc/refine.hip): the
per-point work is element-wise float64 numpy over the points, the matrices, the 5 x 5 solve and the updates numpy float64 scalars.  The sums are
taken in the kernel's order (pnp_ref.wave_sums): 64 partial sums over i mod 64 in rising i, then the butterfly v = v + v[lane ^ off].

The independent minimiser is a textbook one: Rodrigues rotation update, a tangent basis of t from numpy.linalg.svd, a central-difference
Jacobian of the Sampson distances written with numpy matrix products, numpy.linalg.lstsq for the step."""
import ctypes as C

import numpy as np

import pnp_ref as pr
import pose_degenerate_cases as pdc

REFINED, REJECTED, FEW, NO_POSE = 1, 2, 4, 8
DBL_MAX = 1.7976931348623157e308
CLASSES = ("general", "forward", "sideways", "static", "dup")
MOVING = ("general", "forward", "sideways")

RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("E", "<f8", (9,)), ("cost0", "<f8"), ("cost1", "<f8"), ("n_used", "<i4"),
                         ("n_points", "<i4"), ("n_inliers0", "<i4"), ("n_inliers_refined", "<i4"), ("best_step", "<i4"), ("steps_run", "<i4"),
                         ("flags", "<i4"), ("reserved_", "<i4")])
assert RESULT_DTYPE.itemsize == 216


class Params(C.Structure):
    """vis_eref_params with its defaults, for callers without the library (CPU tests)"""
    _fields_ = [("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("threshold_px", C.c_double)]


def default_params():
    return Params(5, 8, 1.0)


Camera = pr.Camera
F = np.float64


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["flags"] = NO_POSE
    return r


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def make_scene(cls, m, noise, outliers, seed=0):
    """(x1, x2 float32 pixels m x 2, R, t unit or zero): points of pose_degenerate_cases.make_case's box seen before and after a motion;
    general: |w| ~ 0.05 rad per axis and a random unit t; forward / sideways: R = I, t = e_z / e_x; static: no motion; dup: six points of
    a general motion repeated.  noise in pixels on both images; the first `outliers` share of the second image's pixels replaced by uniform
    ones of a 752 x 480 image"""
    rng = np.random.default_rng([53, CLASSES.index(cls), m, int(round(10 * noise)), int(round(100 * outliers)), int(seed)])
    R = pdc._rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    if cls == "forward":
        R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    elif cls == "sideways":
        R, t = np.eye(3), np.array([1.0, 0.0, 0.0])
    elif cls == "static":
        R, t = np.eye(3), np.zeros(3)
    n = 6 if cls == "dup" else m
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4.0, 12.0, n)], 1)
    x1 = pdc._project(X) + rng.normal(0, noise, (n, 2))
    x2 = pdc._project(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    if cls == "dup":
        idx = rng.integers(0, 6, m)
        x1, x2 = x1[idx], x2[idx]
    k = int(round(outliers * m))
    x2[:k] = np.stack([rng.uniform(0, 752, k), rng.uniform(0, 480, k)], 1)
    return np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32), R, t


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _finite(v):
    return bool(np.abs(v) <= DBL_MAX)


def xmat(v, M):
    """column j of the result = cross3(v, column j of M); 9 float64 scalars, row-major"""
    out = [F(0.0)] * 9
    for j in range(3):
        out[j] = v[1] * M[6 + j] - v[2] * M[3 + j]
        out[3 + j] = v[2] * M[j] - v[0] * M[6 + j]
        out[6 + j] = v[0] * M[3 + j] - v[1] * M[j]
    return out


def tangent_basis(t):
    a = [np.abs(t[0]), np.abs(t[1]), np.abs(t[2])]
    k, am = 0, a[0]
    if a[1] < am:
        k, am = 1, a[1]
    if a[2] < am:
        k = 2
    e = [F(1.0 if k == i else 0.0) for i in range(3)]
    c = pr._cross3(t, e)
    nb = np.sqrt(pr._dot3(c, c))
    b1 = [c[0] / nb, c[1] / nb, c[2] / nb]
    return b1, pr._cross3(t, b1)


def matrices(R, t):
    """E and the five derivative matrices of the pose"""
    z = F(0.0)
    E = xmat(t, R)
    A0 = [z, z, z, -R[6], -R[7], -R[8], R[3], R[4], R[5]]
    A1 = [R[6], R[7], R[8], z, z, z, -R[0], -R[1], -R[2]]
    A2 = [-R[3], -R[4], -R[5], R[0], R[1], R[2], z, z, z]
    b1, b2 = tangent_basis(t)
    return E, [xmat(t, A0), xmat(t, A1), xmat(t, A2), xmat(b1, R), xmat(b2, R)]


def apply(M, a, b, c, d):
    l0 = (M[0] * a + M[1] * b) + M[2]
    l1 = (M[3] * a + M[4] * b) + M[5]
    l2 = (M[6] * a + M[7] * b) + M[8]
    m0 = (M[0] * c + M[3] * d) + M[6]
    m1 = (M[1] * c + M[4] * d) + M[7]
    s = (c * l0 + d * l1) + l2
    return l0, l1, m0, m1, s


def gn_pass(R, t, a, b, c, d, setmask, thr2):
    """(21 sums, points of the whole row that pass under the pose)"""
    with np.errstate(all="ignore"):
        E, G = matrices(R, t)
        l0, l1, m0, m1, s = apply(E, a, b, c, d)
        den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        rhs = thr2 * den
        n = int(((np.abs(rhs) <= DBL_MAX) & (s * s <= rhs)).sum())
        inl = setmask & (den > 0.0) & (np.abs(den) <= DBL_MAX)
        sd = np.sqrt(den)
        r, hs, dsd = s / sd, 0.5 * s, den * sd
        J = []
        for k in range(5):
            g0, g1, h0, h1, gs = apply(G[k], a, b, c, d)
            dd = 2.0 * (((l0 * g0 + l1 * g1) + m0 * h0) + m1 * h1)
            J.append(gs / sd - (hs * dd) / dsd)
        cols = [J[u] * J[v] for u in range(5) for v in range(u, 5)]
        cols += [J[u] * r for u in range(5)]
        cols.append(r * r)
        terms = np.where(inl[:, None], np.stack(cols, 1), 0.0) if len(a) else np.zeros((0, 21))
    return [F(v) for v in pr.wave_sums(terms)], n


def solve5(S):
    """(d[5], ok): d = -(J^T J)^-1 J^T r by LDL^T without pivoting"""
    A = [[F(0.0)] * 5 for _ in range(5)]
    k = 0
    for a in range(5):
        for b in range(a, 5):
            A[a][b] = A[b][a] = F(S[k])
            k += 1
    L, D, z, d = [[F(0.0)] * 5 for _ in range(5)], [F(0.0)] * 5, [F(0.0)] * 5, [F(0.0)] * 5
    ok = True
    with np.errstate(all="ignore"):
        for j in range(5):
            s = A[j][j]
            for c in range(j):
                s = s - (L[j][c] * L[j][c]) * D[c]
            D[j] = s
            ok = ok and bool(s > 0.0) and _finite(s)
            for i in range(j + 1, 5):
                v = A[i][j]
                for c in range(j):
                    v = v - (L[i][c] * L[j][c]) * D[c]
                L[i][j] = v / s
        for i in range(5):
            v = -F(S[15 + i])
            for c in range(i):
                v = v - L[i][c] * z[c]
            z[i] = v
        for i in range(4, -1, -1):
            v = z[i] / D[i]
            for c in range(i + 1, 5):
                v = v - L[c][i] * d[c]
            d[i] = v
    return d, ok


def rotate(R, w):
    """R <- C(w) R with the Cayley map of pnp_ref.cayley_update"""
    with np.errstate(all="ignore"):
        h = [0.5 * w[0], 0.5 * w[1], 0.5 * w[2]]
        hh = pr._dot3(h, h)
        s = 2.0 / (1.0 + hh)
        z = F(0.0)
        K = [z, -h[2], h[1], h[2], z, -h[0], -h[1], h[0], z]
        Cm = [z] * 9
        for i in range(3):
            for j in range(3):
                k2 = h[i] * h[j] - hh if i == j else h[i] * h[j]
                Cm[3 * i + j] = F(1.0 if i == j else 0.0) + s * (K[3 * i + j] + k2)
        N = [z] * 9
        for i in range(3):
            for j in range(3):
                N[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j]
    return N


def move_t(t, d0, d1):
    with np.errstate(all="ignore"):
        b1, b2 = tangent_basis(t)
        v = [(t[k] + b1[k] * d0) + b2[k] * d1 for k in range(3)]
        n = np.sqrt(pr._dot3(v, v))
        return [v[0] / n, v[1] / n, v[2] / n]


def refine(cam, ep, R, t, x1, x2, mask=None, trace=None, poses=None):
    """one RESULT_DTYPE record; x1 / x2: the row's m valid points (pixels); mask: m bytes or None; trace / poses: lists that receive every
    costed iterate's cost and (R[9], t[3]) -- the last entry is what plain Gauss-Newton produced, whichever iterate is reported"""
    R = [F(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = [F(v) for v in np.asarray(t, np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        tt = pr._dot3(t, t)
        if not any(v != 0.0 for v in R) or not all(_finite(v) for v in R + t) or not bool(tt > 0.0) or not _finite(tt):
            return zero_record()
        nt = np.sqrt(tt)
        t = [t[0] / nt, t[1] / nt, t[2] / nt]
    x1 = np.asarray(x1, np.float32).reshape(-1, 2)
    x2 = np.asarray(x2, np.float32).reshape(-1, 2)
    m = len(x1)
    a, b = pr.normalise(cam, x1)
    c, d = pr.normalise(cam, x2)
    setmask = np.ones(m, bool) if mask is None else np.asarray(mask).reshape(-1)[:m] != 0
    nused = int(setmask.sum())
    thr = F(ep.threshold_px) / F(cam.fx)
    thr2 = thr * thr
    run = ep.refine_iters > 0 and nused >= ep.min_inliers
    passes = int(ep.refine_iters) if run else 0
    cost0 = cost1 = F(0.0)
    nin0 = nin1 = best = steps = 0
    Rb, tb = R, t
    for step in range(passes + 1):
        S, nin = gn_pass(R, t, a, b, c, d, setmask, thr2)
        cost = S[20]
        if trace is not None:
            trace.append(float(cost))
        if poses is not None:
            poses.append((np.array(R, np.float64), np.array(t, np.float64)))
        if step == 0:
            cost0, nin0 = cost, nin
        if step == 0 or (_finite(cost) and (not _finite(cost1) or bool(cost < cost1))):
            cost1, nin1, best, Rb, tb = cost, nin, step, list(R), list(t)
        if step == passes:
            break
        dlt, ok = solve5(S)
        if not ok:
            break
        R = rotate(R, dlt[:3])
        t = move_t(t, dlt[3], dlt[4])
        steps += 1
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["R"], r["t"], r["E"] = Rb, tb, xmat(tb, Rb)
    r["cost0"], r["cost1"] = cost0, cost1
    r["n_used"], r["n_points"], r["n_inliers0"], r["n_inliers_refined"] = nused, m, nin0, nin1
    r["best_step"], r["steps_run"] = best, steps
    r["flags"] = ((REFINED if best > 0 else REJECTED) if run else (FEW if nused < ep.min_inliers else 0))
    return r


def refine_rows(cam, ep, starts, p1, p2, npts, mask=None):
    """the batch: starts = n x (R[9], t[3]) rows, p1 / p2 = n x max_pts x 2, npts clamped to 0 ... max_pts, mask = n x row_cap bytes or None"""
    n, max_pts = len(npts), p1.shape[1]
    out = np.zeros(n, RESULT_DTYPE)
    for i in range(n):
        m = min(max(int(npts[i]), 0), max_pts)
        out[i] = refine(cam, ep, starts[i][:9], starts[i][9:12], p1[i, :m], p2[i, :m], None if mask is None else mask[i, :m])
    return out


# ---- independent methods ------------------------------------------------------------------------------------------------------------
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def sampson_independent(cam, R, t, x1, x2):
    """signed Sampson distances in normalised coordinates, with matrix products"""
    X1 = np.concatenate([(x1.astype(np.float64) - [cam.cx, cam.cy]) / cam.fx, np.ones((len(x1), 1))], 1)
    X2 = np.concatenate([(x2.astype(np.float64) - [cam.cx, cam.cy]) / cam.fx, np.ones((len(x2), 1))], 1)
    E = skew(t) @ R
    l, lt = X1 @ E.T, X2 @ E
    return np.einsum("ij,ij->i", X2, l) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)


def gn_independent(cam, R, t, x1, x2, mask, iters):
    """(R, t, cost) after `iters` plain Gauss-Newton steps: Rodrigues update on the left of R, t moved in its tangent plane (basis: numpy's SVD
    null space of t^T), central-difference Jacobian, numpy.linalg.lstsq"""
    sel = np.ones(len(x1), bool) if mask is None else np.asarray(mask).astype(bool)
    x1, x2 = np.asarray(x1, np.float32)[sel], np.asarray(x2, np.float32)[sel]
    R, t = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    t = t / np.linalg.norm(t)
    for _ in range(iters):
        r0 = sampson_independent(cam, R, t, x1, x2)
        R, t = _moved(R, t, np.linalg.lstsq(jacobian_independent(cam, R, t, x1, x2), -r0, rcond=None)[0])
    r0 = sampson_independent(cam, R, t, x1, x2)
    return R, t, float(r0 @ r0)


def _moved(R, t, p):
    B = np.linalg.svd(t[None, :])[2][1:].T                            # 3 x 2, orthonormal, perpendicular to t
    v = t + B @ p[3:]
    return pdc._rodrigues(p[:3]) @ R, v / np.linalg.norm(v)


def jacobian_independent(cam, R, t, x1, x2, h=1e-6):
    """central differences of the Sampson distances in the five parameters of gn_independent (len(x1) x 5)"""
    J = np.zeros((len(x1), 5))
    for k in range(5):
        p = np.zeros(5)
        p[k] = h
        J[:, k] = (sampson_independent(cam, *_moved(R, t, p), x1, x2) - sampson_independent(cam, *_moved(R, t, -p), x1, x2)) / (2 * h)
    return J


def rot_err_deg(Ra, Rb):
    return pr.rot_angle_deg(Ra, Rb)


def dir_err_deg(ta, tb):
    ta, tb = np.asarray(ta, np.float64), np.asarray(tb, np.float64)
    c = float(ta @ tb) / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def pose_dist(Ra, ta, Rb, tb):
    """|Ra Rb^T - I| (Frobenius) + max |ta - tb|"""
    return pr.rot_diff(Ra, Rb) + float(np.abs(np.asarray(ta, np.float64).reshape(3) - np.asarray(tb, np.float64).reshape(3)).max())
