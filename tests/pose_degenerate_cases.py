"""Degenerate two-view problems for the pose stage: the case list, the invariants an essential matrix and its inlier mask must
satisfy whatever its entries are, and the exact-arithmetic recoverPose fixtures (zero-theta correspondences, directed E).
numpy only, deterministic; shared by tests/test_pose_degenerate_ref.py (CPU), tests/test_pose_degenerate_gpu.py and
tools/stress_pose.py.

Which cases have an E that is stable under rounding, and which were dropped because even the integer outcomes are not, is
MEASURED, not assumed: tests/golden/pose_degenerate_spread.json records, per case, what two builds of the CPU oracle (the
committed one and one with contracted multiply-adds) made of it.  Regenerate it with

    python tools/pose_conditioning.py

(CPU only; the classification -- the dropped set and the E-stable set -- must come out the same)."""
import json
import os

import numpy as np

FOCAL, CX, CY = 458.654, 367.215, 248.375                      # the K of test_pose_gpu.two_view
CLASSES = ("general", "static", "rot", "forward", "sideways", "plane", "tilted", "line", "far", "dup", "shift", "grid", "same")
SIZES = (5, 6, 40, 300)                # single-solve shortcut / smallest sampled problem / small / more than one 256-point staging pass
NOISES = (0.0, 0.3)
MODES = ("adaptive", "fixed100")       # first chunk through k_ransac_hyp + 16-lane k_hyp_roots / everything through the list kernels
E_STABLE_SPREAD = 1e-11                # two decimal orders below TOL = 1e-9: one pair of roundings is one sample of the amplification
MAX_DROPPED_SHARE = 0.05
BAND_REL = 2.0 ** -20                  # Sampson errors this close to the threshold may fall on either side
BAND_SHARE = 0.02
SPREAD_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_degenerate_spread.json")


def case_key(cls, m, noise, mode):
    return f"{cls}-M{m}-n{noise:g}-{mode}"


def all_cases():
    return [(c, m, nz, md) for c in CLASSES for m in SIZES for nz in NOISES for md in MODES]


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _project(X, f=FOCAL, cx=CX, cy=CY):
    return np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy], 1)


def make_case(cls, m, noise, seed=None):
    """(x1, x2) float32 pixels, m x 2 each (seed: another draw of the same class, for tools/stress_pose.py; the case list uses none).  The noise is added to the projections BEFORE the step that makes a class exact, so
    static / shift / dup / same / grid are exact at both noise levels (x2 == x1 bit for bit, a constant float32 offset, ...)."""
    rng = np.random.default_rng([CLASSES.index(cls), m, int(round(10 * noise))] + ([] if seed is None else [int(seed)]))
    R = _rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    n = 6 if cls == "dup" else 1 if cls == "same" else m
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4.0, 12.0, n)], 1)
    if cls in ("static", "shift"):
        R, t = np.eye(3), np.zeros(3)
    elif cls == "rot":
        t = np.zeros(3)
    elif cls == "forward":
        R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    elif cls == "sideways":
        R, t = np.eye(3), np.array([1.0, 0.0, 0.0])
    elif cls == "plane":
        X[:, 2] = 6.0
    elif cls == "tilted":
        X[:, 2] = 6.0 + 0.4 * X[:, 0] + 0.2 * X[:, 1]
    elif cls == "line":
        s = rng.uniform(-1, 1, n)
        X = np.array([0.3, -0.2, 7.0]) + s[:, None] * np.array([2.5, 1.0, 2.0])
    elif cls == "far":
        X[:, 2] = 1e6
        X[:, :2] *= 1e6 / 8.0
    x1 = _project(X)
    x2 = _project(X @ R.T + t)
    x1 = (x1 + rng.normal(0, noise, x1.shape)).astype(np.float32)
    x2 = (x2 + rng.normal(0, noise, x2.shape)).astype(np.float32)
    if cls == "static":
        x2 = x1.copy()
    elif cls == "shift":
        x2 = x1 + np.array([7.0, -3.0], np.float32)
    elif cls == "grid":
        x1, x2 = np.rint(x1), np.rint(x2)
    elif cls == "dup":
        idx = rng.integers(0, 6, m)
        x1, x2 = x1[idx], x2[idx]
    elif cls == "same":
        x1, x2 = np.repeat(x1, m, 0), np.repeat(x2, m, 0)
    return np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)


def set_mode(p, mode):
    """the camera of make_case and one of the two RANSAC modes, on a vis_params-like object (in place, returned)"""
    p.fx = p.fy = FOCAL
    p.cx, p.cy = CX, CY
    if mode == "adaptive":
        p.ransac_adaptive = 1                                   # default iteration cap
    else:
        p.ransac_adaptive, p.ransac_max_iters = 0, 100
    return p


def load_spread():
    with open(SPREAD_JSON) as f:
        return json.load(f)["cases"]


def kept_cases(spread=None):
    spread = load_spread() if spread is None else spread
    return [c for c in all_cases() if not spread[case_key(*c)]["dropped"]]


def is_e_stable(rec):
    return (not rec["dropped"]) and rec["spread"] <= E_STABLE_SPREAD


def cmp_E(E, oE):
    """sign-normalised largest element difference (both of unit Frobenius norm, or both zero)"""
    s = 1.0 if float((E * oE).sum()) >= 0 else -1.0
    return float(np.abs(E - s * oE).max())


# ---- what an E claims, checked from E alone (float64 numpy; numpy's element-wise products and sums are not contracted) ----------
def sampson_err32(E, x1, x2, fx, cx, cy):
    """sampson_inlier of pose.hip / count_inliers of the oracle in their operation order: float32 error per correspondence"""
    E = np.asarray(E, np.float64).reshape(9)
    inv = 1.0 / fx
    a1, b1 = (x1[:, 0].astype(np.float64) - cx) * inv, (x1[:, 1].astype(np.float64) - cy) * inv
    a2, b2 = (x2[:, 0].astype(np.float64) - cx) * inv, (x2[:, 1].astype(np.float64) - cy) * inv
    with np.errstate(all="ignore"):
        Ex0 = (E[0] * a1 + E[1] * b1) + E[2]
        Ex1 = (E[3] * a1 + E[4] * b1) + E[5]
        Ex2 = (E[6] * a1 + E[7] * b1) + E[8]
        Et0 = (E[0] * a2 + E[3] * b2) + E[6]
        Et1 = (E[1] * a2 + E[4] * b2) + E[7]
        x2tEx1 = (a2 * Ex0 + b2 * Ex1) + Ex2
        den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1
        return (x2tEx1 * x2tEx1 / den).astype(np.float32)


def rescore(E, x1, x2, fx, cx, cy, thr_px):
    """(mask the model claims, points inside the undecidable band around the threshold)"""
    err = sampson_err32(E, x1, x2, fx, cx, cy)
    t = np.float32((thr_px / fx) * (thr_px / fx))
    with np.errstate(all="ignore"):
        band = np.abs(err.astype(np.float64) - float(t)) <= BAND_REL * float(t)
        return (err <= t).astype(np.uint8), band


def essential_residuals(E):
    """(max |2 E E^T E - tr(E E^T) E|, |det E|) of E scaled to unit Frobenius norm"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    EEt = E @ E.T
    return float(np.abs(2.0 * EEt @ E - np.trace(EEt) * E).max()), float(abs(np.linalg.det(E)))


def residual_bounds(oE):
    """the bound on each residual of a model of the same problem: 100 x the reference's own (one pair of roundings is one sample),
    floored at what an exact model reaches in double precision"""
    return tuple(max(1e-12, 100.0 * r) for r in essential_residuals(oE))


def check_model(E, mask, n_inl, x1, x2, p, oE):
    """Section-4d invariants of a model with inliers: E finite; its mask is its own Sampson test outside the band and the band is
    thin; E is an essential matrix as nearly as the reference's.  Raises AssertionError naming the invariant; returns the figures."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    m = len(x1)
    assert np.isfinite(E).all(), "finite: E has a non-finite entry"
    assert int(mask.sum()) == n_inl, f"count: mask has {int(mask.sum())} ones, n_inliers = {n_inl}"
    fig = dict(band=0, flips=0)
    want, band = rescore(E, x1, x2, p.fx, p.cx, p.cy, p.ransac_threshold)      # (M == 5: all ones by definition, and by this test too)
    fig["band"] = int(band.sum())
    fig["flips"] = int(((want != mask) & ~band).sum())
    assert fig["flips"] == 0, f"rescore: {fig['flips']} mask bits differ from the model's own Sampson test: {np.flatnonzero((want != mask) & ~band)[:8]}"
    assert fig["band"] <= BAND_SHARE * m, f"band: {fig['band']} of {m} errors within 2^-20 of the threshold"
    r = essential_residuals(E)
    b = residual_bounds(oE)
    fig.update(cubic=r[0], det=r[1], cubic_bound=b[0], det_bound=b[1])
    assert r[0] <= b[0], f"constraint: max|2EE'E - tr(EE')E| = {r[0]:.3e} > {b[0]:.3e}"
    assert r[1] <= b[1], f"constraint: |det E| = {r[1]:.3e} > {b[1]:.3e}"
    return fig


# ---- recoverPose in exact arithmetic --------------------------------------------------------------------------------------------
# fx = fy = 256, cx = cy = 512: pixel 512 + 64 q is the normalised coordinate q / 4 exactly.  E = [e_z]x is left untouched by the
# Jacobi SVD; its candidates are exactly R1 = I, R2 = diag(-1, -1, 1), t = e_z.
ZT_FOCAL, ZT_C = 256.0, 512.0
E_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])            # [e_z]x
E_X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])            # [e_x]x
RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
E_ROT = E_Z @ RZ90                                                              # diag(-1, -1, 0): [e_z]x after a quarter turn about z
R_CANDS = (np.eye(3), np.diag([-1.0, -1.0, 1.0]))

# Correspondences (x1, y1, x2, y2) in QUARTERS on the grid {-2, -1.75, ..., 2}^4 whose 4 x 4 DLT decomposition meets theta == 0 in a
# rotation with column 3 (tests/test_independent_numpy._jacobi): an exhaustive search of the 17^4 grid points
# (tools/pose_conditioning.py --zero-theta) finds 80 for each candidate rotation, the same 80 for t = e_z and t = -e_z.
_ZT_AXIS = [(x, 0, 0, y) for x in (-8, -7, -6, 6, 7, 8) for y in (-4, 4)]       # zero-theta under both rotations
ZERO_THETA_Q = {
    "I": sorted(_ZT_AXIS + [(s, y, -s, v) for s in (-4, 4) for y in range(-8, 9) for v in (-4, 4)]),
    "R2": sorted(_ZT_AXIS + [(s, y, s, v) for s in (-4, 4) for y in range(-8, 9) for v in (-4, 4)]),
}


def dlt_ata(R, t, x1, y1, x2, y2):
    """A^T A of the DLT matrix of one correspondence under P0 = [I | 0], P1 = [R | t], summed in the oracle's order (plain lists of
    Python floats: the input tests/test_independent_numpy._jacobi takes)"""
    P = [[float(R[r][c]) for c in range(3)] + [float(t[r])] for r in range(3)]
    A = [[-1.0, 0.0, float(x1), 0.0], [0.0, -1.0, float(y1), 0.0],
         [float(x2) * P[2][c] - P[0][c] for c in range(4)], [float(y2) * P[2][c] - P[1][c] for c in range(4)]]
    out = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[k][i] * A[k][j]
            out[i][j] = s
    return out


def zt_params(p):
    p.fx = p.fy = ZT_FOCAL
    p.cx = p.cy = ZT_C
    return p


def quarters_to_pixels(q):
    q = np.asarray(q, np.float64).reshape(-1, 4)
    px = (ZT_C + 64.0 * q).astype(np.float32)
    return np.ascontiguousarray(px[:, :2]), np.ascontiguousarray(px[:, 2:])


def motion_rows(n, seed, R=np.eye(3), t=(0.0, 0.0, 1.0), outliers=0.1):
    """n float32 pixel correspondences of a random cloud under x2 ~ R X + t at the exact camera, a tenth of them random"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(4.0, 12.0, n)], 1)
    x1 = _project(X, ZT_FOCAL, ZT_C, ZT_C)
    x2 = _project(X @ np.asarray(R).T + np.asarray(t, np.float64), ZT_FOCAL, ZT_C, ZT_C)
    k = int(outliers * n)
    x2[:k] = rng.uniform(0, 1024, (k, 2))
    return x1.astype(np.float32), x2.astype(np.float32)


def _splice(gen, zt, at):
    x1, x2 = gen
    for (a, b), i in zip(zip(*zt), at):
        x1[i], x2[i] = a, b
    return x1, x2


def zero_theta_rows():
    """name -> (x1, x2): the row shapes of the fallback, each for a cloud the camera approaches (t = +e_z wins: the votes of the first
    decomposition decide) and one it backs away from (t = -e_z wins: the votes of the SECOND decomposition decide)"""
    zt_all = quarters_to_pixels(ZERO_THETA_Q["I"] + [q for q in ZERO_THETA_Q["R2"] if q not in ZERO_THETA_Q["I"]])
    rows = {"only_zero_theta_I": quarters_to_pixels(ZERO_THETA_Q["I"]), "only_zero_theta_both": quarters_to_pixels(_ZT_AXIS),
            "only_zero_theta_union": zt_all}
    pick = quarters_to_pixels([(-8, 0, 0, 4), (-7, 0, 0, -4), (4, 3, -4, 4), (-4, -5, -4, -4)])
    for name, tz in (("fwd", 1.0), ("back", -1.0)):
        t = (0.0, 0.0, tz)
        rows[f"one_in_wave_{name}"] = _splice(motion_rows(64, 11, t=t), pick, [37])               # the whole wave takes the pass
        rows[f"second_wave_{name}"] = _splice(motion_rows(65, 12, t=t), pick, [64])               # one of two waves takes it
        rows[f"nsplit2_{name}"] = _splice(motion_rows(1100, 13, t=t), pick, [0, 255, 256, 1099])  # two workgroups, votes summed
    return rows


def directed_E():
    """name -> (E, x1, x2): exact essential matrices with equal singular values, scaled far down and up, and rank-deficient ones"""
    out = {}
    scenes = {"ez": (E_Z, motion_rows(70, 21)), "ex": (E_X, motion_rows(70, 22, t=(1.0, 0.0, 0.0))),
              "rot90": (E_ROT, motion_rows(70, 23, R=RZ90))}
    for name, (E, (x1, x2)) in scenes.items():
        for tag, s in (("", 1.0), ("_1e-12", 1e-12), ("_1e+12", 1e12)):
            out[name + tag] = (E * s, x1, x2)
    x1, x2 = motion_rows(70, 24)
    out["zero"] = (np.zeros((3, 3)), x1, x2)
    out["rank1"] = (np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), x1, x2)
    out["identity"] = (np.eye(3), x1, x2)
    return out
