"""numpy restatement of VISystem::F2FRansac (src/VISystem.cpp:612-769) and VISystem::FilterKeypoints (:542-610) with the rules of the
batched entry points (include/vislam_hip.h): one table of draws reduced per pair, the first iteration with the largest count wins,
n_degenerate, the float scale and sign flip against a reference translation, zero records.

Every product and sum is written in the order the reference (and oracle/pose.cpp, and the kernels) write them: float bearings widened to
double, sqrt((a0^2 + a1^2) + a2^2), rows of R summed left to right, cross products as differences of two products, dot products
(x x' + y y') + z z'.  numpy's element-wise double arithmetic is IEEE without fused multiply-adds, so these are the same operations.

The inlier test is the full expression -1000 / log10(|x|) < threshold here (`inlier_full`); `inlier_banded` restates the device helper's two
compares + band (csrc/epipolar.hip epi_inlier / epi_band) so that the reasoning behind it can be checked on the CPU."""
import math
import struct

import numpy as np

F32 = np.float32
ZERO_RECORD = dict(t=np.zeros(3, F32), count_max=0, n_points=0, best_iter=-1, n_degenerate=0, flipped=0)
EPI_BAND_ULPS = 32.0


# ---------------------------------------------------------------------------------------------- synthetic pairs
def two_view(n, seed, outliers=0.0, noise=0.0, depth=(4.0, 12.0)):
    """local copy of tests/test_pose_gpu.py two_view: n points seen from two EuRoC cameras, (x1, x2 float32 pixels, R, t)"""
    rng = np.random.default_rng(seed)
    K = np.array([[458.654, 0, 367.215], [0, 458.654, 248.375], [0, 0, 1]])
    ang = rng.normal(0, 0.05, 3)
    th = np.linalg.norm(ang)
    k = ang / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(*depth, n)], 1)
    x1 = (K @ X.T).T
    x1 = x1[:, :2] / x1[:, 2:]
    X2 = (R @ X.T).T + t
    x2 = (K @ X2.T).T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 += rng.normal(0, noise, x1.shape)
    x2 += rng.normal(0, noise, x2.shape)
    nout = int(outliers * n)
    x2[:nout] = rng.uniform(0, 480, (nout, 2))
    return x1.astype(np.float32), x2.astype(np.float32), R, t


def pair_inputs(m, seed, outliers, noise):
    """(p1 m x 2, p2 m x 2 float32, rot 3 x 3 float32 = R^T, t float32) like tests/test_pose_gpu.py _f2f_inputs; t = the true translation"""
    x1, x2, R, t = two_view(max(m, 5), seed, outliers, noise)
    return np.ascontiguousarray(x1[:m]), np.ascontiguousarray(x2[:m]), R.T.astype(np.float32), t.astype(np.float32)


def keypoints(dtype, xy):
    k = np.zeros(len(xy), dtype)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


def batch_cases(tile):
    """the 12 pairs of the device-pointer tests: (m, seed, outliers, noise).  Rows at the ends of the size range, around one LDS tile
    of the kernel and beyond two; every pair carries pixel noise and the larger ones some outliers, so that the filter thresholds
    500 and 370 cut on both sides (tests/test_f2f_batch_ref.py checks that on the CPU)."""
    ms = [0, 1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 5, 40, 120, 60, 90]
    out = []
    for k, m in enumerate(ms):
        out.append((m, 101 + k, 0.3 if k >= 10 else 0.1, 1.5))
    return out


def edge_rows(tile):
    """the two rows of the iteration-count and tie tests, one per workgroup shape of the kernel: 40 correspondences and one more than a tile"""
    return [pair_inputs(40, 211, 0.1, 1.5), pair_inputs(tile + 1, 212, 0.1, 1.5)]


TIE_ITERS = 1100                                                   # a second round of either workgroup shape (1024 iterations per round)
TIE_FIRSTS = (0, 70, 300, 1030)                                    # the first live iteration: lane 0, a second wave, a second slot, the second round
TIE_PAIR, TIE_SKIP = (3, 17), 5                                    # below 39: the same reduced indices for both rows


def tie_draws(first, iters=TIE_ITERS):
    """every iteration draws TIE_PAIR, so every live count is equal; the first `first` draw (TIE_SKIP, TIE_SKIP), whose cross product
    n x n is exactly zero (a b - b a of the same two doubles), so they are skipped"""
    d = np.empty((iters, 2), np.int32)
    d[:] = TIE_PAIR
    d[:first] = TIE_SKIP
    return d


# ---------------------------------------------------------------------------------------------- the predicate
def inlier_full(x, thr):
    """-1000.0 / log10(fabs(x)) < threshold, element-wise (x = 0: -1000 / -inf = +0; |x| = 1: -1000 / +0 = -inf; NaN: False)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-1000.0 / np.log10(np.abs(np.asarray(x, np.float64)))) < thr


def band(thr):
    """(c_lo, c_hi) of csrc/epipolar.hip epi_band; (0, inf) = the full expression for every x"""
    if not (thr > 0.0) or not math.isfinite(thr):
        return 0.0, math.inf
    c = math.pow(10.0, -1000.0 / thr)
    if not (c >= 1e-290):
        return 0.0, math.inf
    k = 2.0 * (abs(math.log(c)) + 1.0) * (EPI_BAND_ULPS * 2.0 ** -53)
    lo, hi = c * (1.0 - k), c * (1.0 + k)
    if not (lo > 0.0) or not (hi < 1.0):
        return 0.0, math.inf
    return lo, hi


def inlier_banded(x, thr):
    """the device helper: two compares outside the band, the full expression inside.  Returns (result, evaluated-in-full mask)."""
    x = np.asarray(x, np.float64)
    lo, hi = band(thr)
    ax = np.abs(x)
    with np.errstate(invalid="ignore"):
        below, above = ax < lo, ax > hi
    res = below | (above & (ax >= 1.0))
    inside = ~below & ~above
    res[inside] = inlier_full(x[inside], thr)
    return res, inside


# ---------------------------------------------------------------------------------------------- normals
def normals(p, p1, p2, rot):
    """m x 3 float64 epipolar-plane normals (:651-668): bearing1 x (R bearing2)"""
    fx, fy, cx, cy = F32(p.fx), F32(p.fy), F32(p.cx), F32(p.cy)
    p1, p2 = np.asarray(p1, F32).reshape(-1, 2), np.asarray(p2, F32).reshape(-1, 2)
    R = np.asarray(rot, F32).reshape(9).astype(np.float64)

    def bearing(q):
        a0 = ((q[:, 0] - cx) / fx).astype(np.float64)
        a1 = ((q[:, 1] - cy) / fy).astype(np.float64)
        a2 = np.ones(len(q))
        n = np.sqrt((a0 * a0 + a1 * a1) + a2 * a2)
        return a0 / n, a1 / n, a2 / n
    a0, a1, a2 = bearing(p1)
    b0, b1, b2 = bearing(p2)
    r0 = (R[0] * b0 + R[1] * b1) + R[2] * b2
    r1 = (R[3] * b0 + R[4] * b1) + R[5] * b2
    r2 = (R[6] * b0 + R[7] * b1) + R[8] * b2
    return np.stack([a1 * r2 - a2 * r1, a2 * r0 - a0 * r2, a0 * r1 - a1 * r0], 1)


def reduce_draws(draws, m):
    """iteration j samples (draws[2j] & 0x7fffffff) % (m - 1) and the same of draws[2j + 1]: rand() % (sizeNewGroup - 1), :712-713"""
    d = np.asarray(draws, np.int32).reshape(-1, 2)
    return ((d & 0x7FFFFFFF) % (m - 1)).astype(np.int32)


# ---------------------------------------------------------------------------------------------- F2FRansac
def f2f(p, p1, p2, rot, draws, tref=None, iters=None, thr=None, detail=False):
    """one pair's record (a dict like ZERO_RECORD).  draws: the call's table (iters x 2 int32); tref: 3 floats or None.
    detail=True also returns (unit directions iters x 3, counts, degenerate mask, normals)."""
    iters = int(p.f2f_iters) if iters is None else iters
    thr = float(p.f2f_threshold) if thr is None else thr
    m = len(p1)
    rec = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ZERO_RECORD.items()}
    if m < 2 or iters <= 0:
        return (rec, None) if detail else rec
    nv = normals(p, p1, p2, rot)
    idx = reduce_draws(draws, m)[:iters]
    n1, n2 = nv[idx[:, 0]], nv[idx[:, 1]]
    d = np.stack([n1[:, 1] * n2[:, 2] - n1[:, 2] * n2[:, 1], n1[:, 2] * n2[:, 0] - n1[:, 0] * n2[:, 2], n1[:, 0] * n2[:, 1] - n1[:, 1] * n2[:, 0]], 1)
    deg = ~((d[:, 0] != 0.0) | (d[:, 1] != 0.0) | (d[:, 2] != 0.0))                # :716
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d / dn[:, None]
        x = (d[:, 0:1] * nv[None, :, 0] + d[:, 1:2] * nv[None, :, 1]) + d[:, 2:3] * nv[None, :, 2]
    cnt = inlier_full(x, thr).sum(1).astype(np.int64)
    cnt[deg] = 0
    rec["n_points"], rec["n_degenerate"] = m, int(deg.sum())
    if cnt.max() > 0:
        best = int(np.argmax(cnt))                                 # the first of the largest: `if (count > countMax)` in order, :737-741
        g = None if tref is None else np.asarray(tref, F32).reshape(3)
        scale = F32(1.0) if g is None else F32(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))      # float, :639-642
        t = np.array([scale * F32(d[best, k]) for k in range(3)], F32)
        if g is not None and F32((t[0] * g[0] + t[1] * g[1]) + t[2] * g[2]) < 0:                         # :524-527
            t = -t
            rec["flipped"] = 1
        rec["t"], rec["count_max"], rec["best_iter"] = t, int(cnt[best]), best
    return (rec, (d, cnt, deg, nv)) if detail else rec


def record_tuple(r):
    """a record (dict, numpy record or ctypes struct) as a comparable tuple, t by its bytes"""
    get = (lambda k: r[k]) if isinstance(r, (dict, np.void)) else (lambda k: getattr(r, k))
    t = np.array([get("t")[k] for k in range(3)], F32)
    return (t.tobytes(), int(get("count_max")), int(get("n_points")), int(get("best_iter")), int(get("n_degenerate")), int(get("flipped")))


# ---------------------------------------------------------------------------------------------- FilterKeypoints
def filter_keypoints(p, p1, p2, rot, t, thr):
    """(keep uint8[m], count): tVec = (double)t / sqrt of its double sum of squares (:565-568); a zero t keeps nothing (NaN)"""
    m = len(p1)
    if m == 0:
        return np.zeros(0, np.uint8), 0
    nv = normals(p, p1, p2, rot)
    tv = np.asarray(t, F32).reshape(3).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = tv / np.sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2])
        x = (tv[0] * nv[:, 0] + tv[1] * nv[:, 1]) + tv[2] * nv[:, 2]
    keep = inlier_full(x, thr).astype(np.uint8)
    return keep, int(keep.sum())


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def filter_keypoints_plain(p, p1, p2, rot, t, thr):
    """the same a second way: plain Python floats, math.sqrt / math.log10, one correspondence at a time.  A float operation is the
    double operation rounded to float once (exact for + - * / of floats: 53 >= 2 * 24 + 2 bits)."""
    fx, fy, cx, cy = _f32(p.fx), _f32(p.fy), _f32(p.cx), _f32(p.cy)
    R = [float(_f32(float(v))) for v in np.asarray(rot).reshape(9)]
    tv = [float(_f32(float(v))) for v in np.asarray(t).reshape(3)]
    s = math.sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2])
    tv = [v / s if s != 0.0 else math.nan for v in tv]
    keep = []
    for (u1, v1), (u2, v2) in zip(np.asarray(p1, F32).tolist(), np.asarray(p2, F32).tolist()):
        a = [_f32(_f32(u1 - cx) / fx), _f32(_f32(v1 - cy) / fy), 1.0]
        b = [_f32(_f32(u2 - cx) / fx), _f32(_f32(v2 - cy) / fy), 1.0]
        na = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        nb = math.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        a = [v / na for v in a]
        b = [v / nb for v in b]
        rb = [(R[0] * b[0] + R[1] * b[1]) + R[2] * b[2], (R[3] * b[0] + R[4] * b[1]) + R[5] * b[2], (R[6] * b[0] + R[7] * b[1]) + R[8] * b[2]]
        n = [a[1] * rb[2] - a[2] * rb[1], a[2] * rb[0] - a[0] * rb[2], a[0] * rb[1] - a[1] * rb[0]]
        x = abs((tv[0] * n[0] + tv[1] * n[1]) + tv[2] * n[2])
        if math.isnan(x):
            keep.append(0)
        elif x == 0.0:
            keep.append(1 if 0.0 < thr else 0)                     # -1000 / -inf = +0
        else:
            lg = math.log10(x)
            err = -math.inf if lg == 0.0 else -1000.0 / lg         # |x| = 1: -1000 / +0
            keep.append(1 if err < thr else 0)
    return np.array(keep, np.uint8), int(sum(keep))
