"""The essential RANSAC and F2F at the ends of their parameters.  Not a test module: shared by tests/test_ransac_params_ref.py (CPU, the
oracle alone) and tests/test_ransac_params_gpu.py (the device against the oracle, the yardstick of tests/test_limits_gpu.py::_ransac_case).

A case: (name, {vis_params field: value}).  Scenes are generated with the case's own intrinsics (fx, fy, cx, cy), m = 120 (k_hyp_score's
staged form) and 300 (its ballot form), 0.3 px of noise, a quarter of the second image's points replaced by uniform ones."""
import numpy as np

LENGTHS = (120, 300)
ITERS = 400
ONE_BELOW = 1.0 - 2.0 ** -53

CASES = (
    [(f"ransac_threshold {v!r}", dict(ransac_threshold=v)) for v in (1e-4, 1e-2, 30.0, 1e3)] +
    [(f"ransac_prob {v!r}", dict(ransac_prob=v)) for v in (1e-12, 0.5, ONE_BELOW)] +
    [("ransac_max_iters 1", dict(ransac_max_iters=1)), ("ransac_max_iters 100000", dict(ransac_max_iters=100000, ransac_adaptive=1))] +
    [(f"ransac_seed {v:#x}", dict(ransac_seed=v)) for v in (0, 0xffffffff)] +
    [(f"cx = cy = {v!r}", dict(cx=v, cy=v)) for v in (0.0, -1e4, 1e6)] +
    [("fy != fx", dict(fx=458.654, fy=300.0))] +
    [(f"fx = fy = {v!r}", dict(fx=v, fy=v)) for v in (1.0, 1e5)]
)
# what vis_set_params refuses, and why (tests/test_ransac_params_ref.py shows the oracle's answer to each)
REFUSED_RANSAC_THRESHOLDS = (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-19 * 458.654, 1e19 * 458.654)
F2F_THRESHOLDS = (0.0, -370.0, float("nan"), float("inf"))            # all accepted: compared as written
F2F_ITERS = (0, 1)


def params(base, fields):
    """the vis_params `base` (a fresh default_params()) at the setting of a case: adaptive stop, ITERS iterations, fy = fx unless the case says"""
    base.fy = base.fx
    base.ransac_adaptive, base.ransac_max_iters = 1, ITERS
    for k, v in fields.items():
        setattr(base, k, v)
    return base


def scene(p, m, seed):
    """(x1, x2) float32 pixels of m points seen before and after a small motion by the camera of p"""
    rng = np.random.default_rng(seed)
    ang = rng.normal(0, 0.05, 3)
    th = np.linalg.norm(ang)
    k = ang / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-3, 3, m), rng.uniform(-2, 2, m), rng.uniform(4.0, 12.0, m)], 1)
    X2 = X @ R.T + t

    def project(Y):
        return np.stack([p.fx * Y[:, 0] / Y[:, 2] + p.cx, p.fy * Y[:, 1] / Y[:, 2] + p.cy], 1)
    x1, x2 = project(X), project(X2) + rng.normal(0, 0.3, (m, 2))
    nout = m // 4
    x2[:nout] = project(np.stack([rng.uniform(-3, 3, nout), rng.uniform(-2, 2, nout), rng.uniform(4.0, 12.0, nout)], 1))
    return x1.astype(np.float32), x2.astype(np.float32)


def rows():
    """(name, fields, m, scene seed) of every case at both lengths; the two ransac_seed cases share their scenes"""
    return [(name, fields, m, 500 + (0 if "ransac_seed" in fields else 10 * (i + 1)) + j) for i, (name, fields) in enumerate(CASES)
            for j, m in enumerate(LENGTHS)]
