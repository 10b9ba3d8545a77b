"""Restatements the triangulation tests compare the library against (not test modules; nothing here calls the code under test).

  jacobi_eig4 / triangulate_point   plain Python doubles, operation for operation the sequence of oracle/pose.cpp cheirality() +
                                    jacobi_eig(4): Python floats are IEEE binary64 and every +, -, *, / and math.sqrt rounds once,
                                    like code compiled with -ffp-contract=off.
  parallax_f32                      VISystem::Disparity's per-point term (src/VISystem.cpp:440-462) in numpy float32 scalars.
  triangulate                       the contract of vis_triangulate on top of the two: records, flags, summary.
  svd_point                         the independent method: numpy.linalg.svd of the 4 x 4 DLT matrix A (not of A^T A).
  scene                             seeded synthetic two-view scenes (EuRoC intrinsics)."""
import math

import numpy as np

MP_INLIER, MP_FRONT, MP_REPROJ_OK, MP_PARALLAX_OK, MP_KEPT = 1, 2, 4, 8, 16
MAP_POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("reproj_px", "<f4"), ("parallax_px", "<f4")])
INF, NAN = float("inf"), float("nan")


def _div(a, b):
    """IEEE double division (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def jacobi_eig4(A):
    """cyclic Jacobi on the symmetric 4 x 4 matrix A (list of 16, row-major; destroyed: diagonal = eigenvalues).  Returns (V, sweeps,
    rotations): V's columns are the eigenvectors."""
    n = 4
    V = [1.0 if i == j else 0.0 for i in range(n) for j in range(n)]
    sweeps = rotations = 0
    for _ in range(30):
        off = 0.0
        for i in range(n):
            for j in range(i + 1, n):
                off += A[i * n + j] * A[i * n + j]
        if off < 1e-300:
            break
        sweeps += 1
        for p in range(n):
            for q in range(p + 1, n):
                apq = A[p * n + q]
                if abs(apq) < 1e-300:
                    continue
                rotations += 1
                app, aqq = A[p * n + p], A[q * n + q]
                theta = (aqq - app) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp, akq = A[k * n + p], A[k * n + q]
                    A[k * n + p] = c * akp - s * akq
                    A[k * n + q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p * n + k], A[q * n + k]
                    A[p * n + k] = c * apk - s * aqk
                    A[q * n + k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k * n + p], V[k * n + q]
                    V[k * n + p] = c * vkp - s * vkq
                    V[k * n + q] = s * vkp + c * vkq
    return V, sweeps, rotations


def normalise(p, fx, cx, cy):
    """((double)p - c) * (1.0 / fx) for both axes (oracle/pose.cpp normalise_points)"""
    inv = 1.0 / fx
    return (float(p[0]) - cx) * inv, (float(p[1]) - cy) * inv


def dlt_matrix(R, t, x1, y1, x2, y2):
    """the 4 x 4 DLT matrix of cheirality(): rows of P0 = [I | 0] and P = [R | t]"""
    P = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    A = [-1.0, 0.0, x1, 0.0, 0.0, -1.0, y1, 0.0] + [0.0] * 8
    for c in range(4):
        A[8 + c] = x2 * P[8 + c] - P[c]
        A[12 + c] = y2 * P[8 + c] - P[4 + c]
    return A, P


def triangulate_point(R, t, x1, y1, x2, y2):
    """(X[3], front, sweeps, rotations) of one normalised correspondence: cheirality() with the point kept"""
    A, P = dlt_matrix(R, t, x1, y1, x2, y2)
    AtA = [0.0] * 16
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[4 * k + i] * A[4 * k + j]
            AtA[4 * i + j] = s
    V, sweeps, rotations = jacobi_eig4(AtA)
    mn = 0
    for i in range(1, 4):
        if AtA[5 * i] < AtA[5 * mn]:
            mn = i
    X = [V[mn], V[4 + mn], V[8 + mn], V[12 + mn]]
    ok = (X[2] * X[3]) > 0
    Xn = [_div(X[0], X[3]), _div(X[1], X[3]), _div(X[2], X[3])]
    ok = ok and (Xn[2] < 50.0)
    z2 = ((P[8] * Xn[0] + P[9] * Xn[1]) + P[10] * Xn[2]) + P[11]
    ok = ok and (z2 > 0) and (z2 < 50.0)
    return Xn, bool(ok), sweeps, rotations


def reproj_px(X, p1, fx, cx, cy):
    """reprojection error in the first image, double, rounded to float once"""
    du = float(p1[0]) - (fx * _div(X[0], X[2]) + cx)
    dv = float(p1[1]) - (fx * _div(X[1], X[2]) + cy)
    s = du * du + dv * dv
    return np.float32(math.sqrt(s) if s == s and s >= 0 else NAN)


def parallax_f32(R, p1, p2, fx, fy, cx, cy):
    """Disparity's per-point term with RotationResCam = (float)R^T, every operation in float32"""
    f = np.float32
    with np.errstate(all="ignore"):
        fxf, fyf, cxf, cyf = f(fx), f(fy), f(cx), f(cy)
        u1, v1, u2, v2 = f(p1[0]), f(p1[1]), f(p2[0]), f(p2[1])
        a = (u2 - cxf) / fxf
        b = (v2 - cyf) / fyf
        one = f(1.0)
        ox = (f(R[0]) * a + f(R[3]) * b) + f(R[6]) * one
        oy = (f(R[1]) * a + f(R[4]) * b) + f(R[7]) * one
        oz = (f(R[2]) * a + f(R[5]) * b) + f(R[8]) * one
        u = fxf * ox / oz + cxf
        v = fyf * oy / oz + cyf
        du, dv = u1 - u, v1 - v
        r = np.sqrt(du * du + dv * dv)
    assert r.dtype == np.float32
    return r


def parallax_f64(R, p1, p2, fx, fy, cx, cy):
    """the same quantity in float64 from float64 inputs (what parallax_f32 is pinned against)"""
    Rm = np.asarray(R, np.float64).reshape(3, 3)
    o = Rm.T @ np.array([(float(p2[0]) - cx) / fx, (float(p2[1]) - cy) / fy, 1.0])
    return math.hypot(float(p1[0]) - (fx * o[0] / o[2] + cx), float(p1[1]) - (fy * o[1] / o[2] + cy))


def triangulate(R, t, p1, p2, fx, fy, cx, cy, mask=None, max_reproj_px=2.0, min_parallax_px=0.0, inliers_only=0):
    """vis_triangulate's contract: (points MAP_POINT_DTYPE[m], flags uint8[m], summary dict, sweeps per point)"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    p1 = np.asarray(p1, np.float32).reshape(-1, 2)
    p2 = np.asarray(p2, np.float32).reshape(-1, 2)
    m = len(p1)
    pts = np.zeros(m, MAP_POINT_DTYPE)
    flags = np.zeros(m, np.uint8)
    sweeps = np.zeros(m, np.int32)
    total = np.float32(0.0)
    for i in range(m):
        inl = True if mask is None else bool(mask[i])
        if inliers_only and not inl:
            total = total + np.float32(0.0)
            continue
        x1, y1 = normalise(p1[i], fx, cx, cy)
        x2, y2 = normalise(p2[i], fx, cx, cy)
        X, front, sweeps[i], _ = triangulate_point(R, t, x1, y1, x2, y2)
        rp = reproj_px(X, p1[i], fx, cx, cy)
        px = parallax_f32(R, p1[i], p2[i], fx, fy, cx, cy)
        f = (MP_INLIER if inl else 0) | (MP_FRONT if front else 0) | (MP_REPROJ_OK if rp <= np.float32(max_reproj_px) else 0) | \
            (MP_PARALLAX_OK if px >= np.float32(min_parallax_px) else 0)
        if f == (MP_INLIER | MP_FRONT | MP_REPROJ_OK | MP_PARALLAX_OK):
            f |= MP_KEPT
        pts[i] = (X, rp, px)
        flags[i] = f
        with np.errstate(all="ignore"):
            total = np.float32(total + px)                    # Disparity's running float sum, index order
    with np.errstate(all="ignore"):
        mean = np.float32(total / np.float32(m)) if m else np.float32(0.0)
    summary = dict(n_points=m, n_front=int(((flags & MP_FRONT) != 0).sum()), n_kept=int(((flags & MP_KEPT) != 0).sum()), mean_parallax_px=mean)
    return pts, flags, summary, sweeps


def svd_point(R, t, x1, y1, x2, y2):
    """(X[3], front) from numpy.linalg.svd of the DLT matrix A itself: the right singular vector of the smallest singular value"""
    A, P = dlt_matrix([float(v) for v in np.asarray(R).reshape(9)], [float(v) for v in np.asarray(t).reshape(3)], x1, y1, x2, y2)
    Q = np.linalg.svd(np.array(A, np.float64).reshape(4, 4))[2][-1]
    ok = Q[2] * Q[3] > 0
    X = Q[:3] / Q[3]
    z2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]
    return X, bool(ok and X[2] < 50.0 and 0 < z2 < 50.0)


EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375)           # calibration/calibrationEUROC.xml:20


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def scene(seed, n=200, fx=EUROC["fx"], cx=EUROC["cx"], cy=EUROC["cy"], w=752, h=480, noise_px=0.3):
    """a two-view scene with fy = fx: n points uniform over the first image, depth uniform in 4 ... 40 baselines, rotation vector
    N(0, 0.03^2) rad per axis, unit t, Gaussian pixel noise on both images, coordinates rounded to float.
    Returns (R (3, 3), t (3,), p1 (n, 2) float32, p2 (n, 2) float32, X true (n, 3))."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, w, n)
    v = rng.uniform(0, h, n)
    z = rng.uniform(4.0, 40.0, n)
    X = np.column_stack([(u - cx) / fx * z, (v - cy) / fx * z, z])
    R = rodrigues(rng.normal(0, 0.03, 3))
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    X2 = X @ R.T + t
    p1 = np.column_stack([u, v]) + rng.normal(0, noise_px, (n, 2))
    p2 = np.column_stack([fx * X2[:, 0] / X2[:, 2] + cx, fx * X2[:, 1] / X2[:, 2] + cy]) + rng.normal(0, noise_px, (n, 2))
    return R, t, p1.astype(np.float32), p2.astype(np.float32), X
