"""The pose of a homography (vis_homography_pose / vis_homography_pose_batch / vis_batch_homography_pose of include/vislam_hip.h) restated
operation for operation; an independent method; planted-plane scenes with their truth.  Not a test module: shared by
tests/test_homography_pose_ref.py (CPU), tests/test_homography_pose_abi.py and tests/test_homography_pose_gpu.py.

  jacobi_eig3 / svd3 / decompose / vote_point / choose / hpose   plain Python floats (IEEE binary64, one rounding per +, -, *, / and
                                    math.sqrt, nothing contracted) in the parenthesisation of csrc/pose.hip (jacobi_eig<3>, svd3_decompose,
                                    k_hpose_svd, k_hpose_vote); the vote is triangulate_ref.triangulate_point, the restatement of
                                    cheirality().
  decompose_svd                     the independent method: numpy.linalg.svd and the closed form of Faugeras & Lustman (1988) in numpy.
  truth / planted_plane             the (R, t / d, n) behind the plane classes of pose_degenerate_cases, and seeded scenes of a plane of
                                    any normal and distance."""
import ctypes as C
import math

import numpy as np

import homography_ref as hr
import pose_degenerate_cases as pdc
import triangulate_ref as tr

HP_NONE, HP_ROTATION, HP_PLANE = 0, 1, 2
HPF_AMBIGUOUS, HPF_HINTED, HPF_FEW, HPF_LOW_PARALLAX = 1, 2, 4, 8
KIND_NAMES = ("none", "rotation", "plane")
DBL_MAX = 1.7976931348623157e308

RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n", "<f8", (3,)), ("R2", "<f8", (9,)), ("t2", "<f8", (3,)), ("n2", "<f8", (3,)),
                         ("sv", "<f8", (3,)), ("t_norm", "<f8"), ("n_good", "<i4", (4,)), ("kind", "<i4"), ("flags", "<i4"), ("solution", "<i4"),
                         ("second", "<i4"), ("n_tested", "<i4"), ("n_parallax", "<i4"), ("n_points", "<i4"), ("reserved_", "<i4")])


class Params(C.Structure):
    """vis_hpose_params with its defaults, for callers without the library (CPU tests)"""
    _fields_ = [("min_t_over_d", C.c_double), ("max_cos_parallax", C.c_double), ("ambiguity_ratio", C.c_double), ("good_share", C.c_double),
                ("parallax_share", C.c_double), ("min_good", C.c_int32), ("reserved_", C.c_int32)]


def default_params():
    return Params(0.05, 0.9998476951563913, 0.75, 0.9, 0.5, 8, 0)


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["solution"] = r["second"] = -1
    return r


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mat3_mul(A, B):
    out = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += A[3 * i + k] * B[3 * k + j]
            out[3 * i + j] = s
    return out


def jacobi_eig3(A):
    """cyclic Jacobi on the symmetric 3 x 3 matrix A (list of 9, row-major; destroyed: diagonal = eigenvalues): jacobi_eig<3> of pose.hip, the
    rotations of triangulate_ref.jacobi_eig4 in the same order.  Returns (V, sweeps): V's columns are the eigenvectors."""
    n = 3
    V = [1.0 if i == j else 0.0 for i in range(n) for j in range(n)]
    sweeps = 0
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
    return V, sweeps


def svd3(E):
    """(U, Vt) of svd3_decompose (pose.hip): eigenvectors of E^T E by descending eigenvalue, v2 = v0 x v1, u0 = E v0 / |E v0|, u1 = E v1
    made orthogonal to u0 and normalised, u2 = u0 x u1 -- both proper rotations"""
    A = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += E[3 * k + i] * E[3 * k + j]
            A[3 * i + j] = s
    V, _ = jacobi_eig3(A)
    o = [0, 1, 2]
    for i in range(3):
        for j in range(i + 1, 3):
            if A[4 * o[j]] > A[4 * o[i]] or (A[4 * o[j]] == A[4 * o[i]] and o[j] < o[i]):
                o[i], o[j] = o[j], o[i]
    v0 = [V[3 * k + o[0]] for k in range(3)]
    v1 = [V[3 * k + o[1]] for k in range(3)]
    v2 = _cross3(v0, v1)
    u0 = [_dot3(E[3 * r:3 * r + 3], v0) for r in range(3)]
    u1 = [_dot3(E[3 * r:3 * r + 3], v1) for r in range(3)]
    n0 = math.sqrt(_dot3(u0, u0))
    u0 = [tr._div(v, n0) for v in u0]
    pr = _dot3(u0, u1)
    u1 = [u1[r] - pr * u0[r] for r in range(3)]
    n1 = math.sqrt(_dot3(u1, u1))
    u1 = [tr._div(v, n1) for v in u1]
    u2 = _cross3(u0, u1)
    U = [0.0] * 9
    for r in range(3):
        U[3 * r], U[3 * r + 1], U[3 * r + 2] = u0[r], u1[r], u2[r]
    return U, v0 + v1 + v2


def _finite(v):
    return abs(v) <= DBL_MAX


def _clamped_sqrt(v):
    return math.sqrt(v if v > 0.0 else 0.0)


def decompose(H, min_t_over_d):
    """k_hpose_svd on one H (9 floats): dict(kind, sv, t_norm, R [2 rotations or 1], t, n [per rotation]).  Rotation 0 carries candidates 0
    (+t, +n) and 3 (-t, -n), rotation 1 candidates 1 and 2."""
    H = [float(v) for v in H]
    U, Vt = svd3(H)
    sv = []
    for k in range(3):
        w = [_dot3(H[3 * r:3 * r + 3], Vt[3 * k:3 * k + 3]) for r in range(3)]
        sv.append(math.sqrt(_dot3(w, w)))
    d1, d2, d3 = sv
    t_norm = tr._div(d1 - d3, d2)
    q1, q2, q3 = d1 * d1, d2 * d2, d3 * d3
    den = q1 - q3
    if not _finite(t_norm):                                           # a rank-deficient H (d2 == 0) or an overflow: no pose
        return dict(kind=HP_NONE, sv=[0.0] * 3, t_norm=0.0, R=[[0.0] * 9], t=[[0.0] * 3], n=[[0.0] * 3])
    if t_norm <= min_t_over_d or den == 0.0 or not _finite(den):
        return dict(kind=HP_ROTATION, sv=sv, t_norm=t_norm, R=[_mat3_mul(U, Vt)], t=[[0.0] * 3], n=[[0.0] * 3])
    x1 = _clamped_sqrt(tr._div(q1 - q2, den))
    x3 = _clamped_sqrt(tr._div(q2 - q3, den))
    dd = (d1 + d3) * d2
    S = tr._div(_clamped_sqrt((q1 - q2) * (q2 - q3)), dd)
    c = tr._div(q2 + d1 * d3, dd)
    base = d1 - d3
    Rs, ts, ns = [], [], []
    for r in range(2):
        s, x3p = (S, x3) if r == 0 else (-S, -x3)
        Rp = [c, 0.0, -s, 0.0, 1.0, 0.0, s, 0.0, c]
        Rs.append(_mat3_mul(_mat3_mul(U, Rp), Vt))
        tp = [base * x1, 0.0, base * -x3p]
        ts.append([tr._div(_dot3(U[3 * i:3 * i + 3], tp), d2) for i in range(3)])
        ns.append([(Vt[i] * x1 + Vt[3 + i] * 0.0) + Vt[6 + i] * x3p for i in range(3)])
    return dict(kind=HP_PLANE, sv=sv, t_norm=t_norm, R=Rs, t=ts, n=ns)


def candidate(dec, k):
    """(R, t, n) of candidate k = 0 ... 3 of a PLANE decomposition: (e1, e3) = (+,+), (+,-), (-,+), (-,-)"""
    r = 0 if k in (0, 3) else 1
    if k < 2:
        return dec["R"][r], list(dec["t"][r]), list(dec["n"][r])
    return dec["R"][r], [-v for v in dec["t"][r]], [-v for v in dec["n"][r]]


def rt_t(R, t):
    """R^T t, each entry summed left to right"""
    return [(R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2] for j in range(3)]


def vote_point(R, t, ct, x1, y1, x2, y2, max_cos):
    """(good, parallax) of one normalised correspondence under one candidate: cheirality(), then r1 = X, r2 = X + R^T t"""
    X, front, _, _ = tr.triangulate_point(R, t, x1, y1, x2, y2)
    if not front:
        return False, False
    r2 = [X[0] + ct[0], X[1] + ct[1], X[2] + ct[2]]
    return True, _dot3(X, r2) < max_cos * math.sqrt(_dot3(X, X) * _dot3(r2, r2))


def vote_table(dec, norm, max_cos):
    """(good, par): bool[4, m] of every correspondence under every candidate (norm: homography_ref.normalise's four arrays)"""
    m = len(norm[0])
    good, par = np.zeros((4, m), bool), np.zeros((4, m), bool)
    for k in range(4):
        R, t, _ = candidate(dec, k)
        ct = rt_t(R, t)
        for i in range(m):
            good[k, i], par[k, i] = vote_point(R, t, ct, float(norm[0][i]), float(norm[1][i]), float(norm[2][i]), float(norm[3][i]), max_cos)
    return good, par


def choose(dec, n_good, n_par, n_tested, hq, rot=None):
    """(solution, second, flags): the choice of k_hpose_vote's last workgroup"""
    order = sorted(range(4), key=lambda k: (-n_good[k], k))
    best = order[0]
    rivals = [k for k in order[1:] if float(n_good[k]) >= hq.ambiguity_ratio * float(n_good[best])]
    flags, sol = 0, best
    if rot is None:
        if rivals:
            flags |= HPF_AMBIGUOUS
    else:
        rot = [float(np.float32(v)) for v in np.asarray(rot).reshape(9)]
        top = None
        for k in [best] + rivals:
            R = candidate(dec, k)[0]
            s = 0.0
            for i in range(3):
                for j in range(3):
                    s = s + R[3 * i + j] * rot[3 * j + i]
            if top is None or s > top:
                top, sol = s, k
        if rivals:
            flags |= HPF_HINTED
    second = [k for k in order if k != sol][0]
    if float(n_good[sol]) < max(float(hq.min_good), hq.good_share * float(n_tested)):
        flags |= HPF_FEW
    if float(n_par[sol]) < hq.parallax_share * float(n_good[sol]):
        flags |= HPF_LOW_PARALLAX
    return sol, second, flags


def hpose(cam, hq, hrec, x1, x2, mask=None, rot=None, table=None):
    """the record of one pair: what vis_homography_pose returns.  hrec: a vis_homography_result-like record (H, best_iter); table: a
    vote_table of the same H and correspondences (computed when absent)"""
    r = zero_record()
    m = len(x1)
    H = [float(v) for v in np.asarray(hrec["H"], np.float64).reshape(9)]
    if int(hrec["best_iter"]) < 0 or not all(_finite(v) for v in H) or m < 1:
        return r
    dec = decompose(H, hq.min_t_over_d)
    if dec["kind"] == HP_NONE:
        return r
    r["sv"], r["t_norm"], r["kind"], r["n_points"] = dec["sv"], dec["t_norm"], dec["kind"], m
    if dec["kind"] == HP_ROTATION:
        r["R"], r["solution"] = dec["R"][0], 0
        return r
    if table is None:
        table = vote_table(dec, hr.normalise(cam, x1, x2), hq.max_cos_parallax)
    votes = np.ones(m, bool) if mask is None else np.asarray(mask)[:m] != 0
    n_good = [int((table[0][k] & votes).sum()) for k in range(4)]
    n_par = [int((table[1][k] & votes).sum()) for k in range(4)]
    n_tested = int(votes.sum())
    sol, second, flags = choose(dec, n_good, n_par, n_tested, hq, rot)
    r["R"], r["t"], r["n"] = candidate(dec, sol)
    r["R2"], r["t2"], r["n2"] = candidate(dec, second)
    r["n_good"], r["flags"], r["solution"], r["second"], r["n_tested"], r["n_parallax"] = n_good, flags, sol, second, n_tested, n_par[sol]
    return r


# ---- the independent method -----------------------------------------------------------------------------------------------------
def decompose_svd(H):
    """(sv, [(R, t, n)] * 4) from numpy.linalg.svd and the closed form for d' = +d2, candidates in the contract's order (an empty list
    when d1 == d3)"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    U, d, Vt = np.linalg.svd(H)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = d
    if d1 * d1 - d3 * d3 <= 0:
        return d, []
    x1 = math.sqrt(max(0.0, (d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)))
    x3 = math.sqrt(max(0.0, (d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3)))
    out = []
    for e1, e3 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        st = e1 * e3 * math.sqrt(max(0.0, (d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        Rp = np.array([[ct, 0, -st], [0, 1, 0], [st, 0, ct]])
        tp = (d1 - d3) * np.array([e1 * x1, 0, -e3 * x3])
        out.append((s * U @ Rp @ Vt, U @ tp / d2, Vt.T @ np.array([e1 * x1, 0, e3 * x3])))
    return d, out


def residuals(H, sv2, cands):
    """the largest of max|R^T R - I|, |det R - 1|, ||n| - 1| and max|d2 (R + t n^T) - H| over the candidates"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    worst = [0.0, 0.0, 0.0, 0.0]
    for R, t, n in cands:
        R, t, n = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64), np.asarray(n, np.float64)
        worst[0] = max(worst[0], float(np.abs(R.T @ R - np.eye(3)).max()))
        worst[1] = max(worst[1], abs(float(np.linalg.det(R)) - 1.0))
        worst[2] = max(worst[2], abs(float(np.linalg.norm(n)) - 1.0))
        worst[3] = max(worst[3], float(np.abs(sv2 * (R + np.outer(t, n)) - H).max()))
    return worst


def rot_angle_deg(Ra, Rb):
    Ra, Rb = np.asarray(Ra, np.float64).reshape(3, 3), np.asarray(Rb, np.float64).reshape(3, 3)
    d = Ra @ Rb.T
    # the angle from the skew part (sine) and the trace (cosine): atan2 keeps its precision near zero, where acos of the trace has none
    sk = np.array([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
    return math.degrees(math.atan2(float(np.linalg.norm(sk)), float(np.trace(d)) - 1.0))


def vec_angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.atan2(float(np.linalg.norm(np.cross(a, b))), float(a @ b)))


def truth_errors(cand, truth_):
    """(angle of R, angle of t, angle of n, relative |t| / d error) of a candidate (R, t, n) against (R, t / d, n)"""
    R, t, n = cand
    Rt, tt, nt = truth_
    return (rot_angle_deg(R, Rt), vec_angle_deg(t, tt), vec_angle_deg(n, nt),
            abs(float(np.linalg.norm(t)) - float(np.linalg.norm(tt))) / float(np.linalg.norm(tt)))


# ---- scenes with their truth ----------------------------------------------------------------------------------------------------
PLANE_LIST = ("plane", "tilted")                                      # the classes of homography_ref.H_LIST with a translation and a plane
ROTATION_LIST = ("static", "rot", "far", "shift")


def truth(cls, m, noise):
    """(R, t / d, n) behind pose_degenerate_cases.make_case(cls, m, noise): its generator replayed.  plane: Z = 6; tilted: Z = 6 + 0.4 X +
    0.2 Y, i.e. n . X = d with n = (-0.4, -0.2, 1) / |.|, d = 6 / |.|"""
    rng = np.random.default_rng([pdc.CLASSES.index(cls), m, int(round(10 * noise))])
    R = pdc._rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    if cls in ("static", "shift"):
        return np.eye(3), np.zeros(3), np.zeros(3)
    if cls in ("rot", "far"):
        return R, np.zeros(3), np.zeros(3)                            # (far: |t| / d ~ 1e-6, below every tolerance here)
    nv = np.array([0.0, 0.0, 1.0]) if cls == "plane" else np.array([-0.4, -0.2, 1.0])
    d = 6.0 / np.linalg.norm(nv)
    return R, t / d, nv / np.linalg.norm(nv)


def planted_plane(seed, m, noise=0.0, fx=pdc.FOCAL, cx=pdc.CX, cy=pdc.CY):
    """(R, t / d, n, x1, x2): m points of a plane of random normal (within ~25 degrees of the optical axis) and distance 4 ... 8 seen from
    two cameras, x2 ~ R X + t with |t| = 0.5 ... 1.5, float32 pixels"""
    rng = np.random.default_rng([4011, int(seed), int(m)])
    R = pdc._rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 1, 3)
    t *= rng.uniform(0.5, 1.5) / np.linalg.norm(t)
    nv = np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.45, 0.45), 1.0])
    nv /= np.linalg.norm(nv)
    d = rng.uniform(4.0, 8.0)
    xy = np.stack([rng.uniform(-0.7, 0.7, m), rng.uniform(-0.45, 0.45, m)], 1)       # rays of the first camera
    rays = np.column_stack([xy, np.ones(m)])
    X = rays * (d / (rays @ nv))[:, None]
    X2 = X @ R.T + t
    x1 = pdc._project(X, fx, cx, cy) + rng.normal(0, noise, (m, 2))
    x2 = pdc._project(X2, fx, cx, cy) + rng.normal(0, noise, (m, 2))
    return R, t / d, nv, np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)


def table_cases():
    """(cls, m, noise, outliers) of the 48 cases: homography_ref.H_LIST x M 40 / 300 x noise 0 / 0.3 x outliers 0 / 25 %"""
    return [(c, m, nz, o) for c in hr.H_LIST for m in (40, 300) for nz in (0.0, 0.3) for o in (0.0, 0.25)]
