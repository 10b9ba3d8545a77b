"""Restatement of the scale-link contract of include/vislam_hip.h (not a test module; nothing here calls the code under test).

Frame i with keyframe q = prev[i]: the baseline q -> i in units of the baseline of q's own pair, the lower median of the depth ratios of the map
points both pairs share through a keypoint of q.  Plain Python floats (IEEE binary64, one rounding per + - * /, nothing contracted); the order
statistics come from a sorted list -- they are defined by value, so how the device finds them does not matter.

  norm_prev          prev[i] normalised: an index < i, KF_CARRIED, KF_NOT_SAVED, else KF_FIRST
  pose_usable        the 12 numbers finite, R not all zero, (t0 t0 + t1 t1) + t2 t2 finite and > 0
  scale_link_rows    vis_scale_link_rows: (depth rows, records)
  carry_out          the row the plan keeps for the next launch"""
import math

import numpy as np

KF_CARRIED, KF_NOT_SAVED, KF_FIRST = -1, -2, -3
SL_OK, SL_NO_PAIR, SL_NO_DEPTH, SL_FEW, SL_SPREAD, SL_RANGE = 0, 1, 2, 4, 8, 16
MP_KEPT = 16
SL_LDS_CAP = 1024                                                   # list entries up to which the device keeps the ratios in LDS
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
POSE_DTYPE = np.dtype([("E", "<f8", (9,)), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_inliers", "<i4"), ("n_pose_good", "<i4"), ("iters_run", "<i4"),
                       ("n_points", "<i4"), ("n_models", "<i4"), ("undecided_max", "<i4")])
MAP_POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("reproj_px", "<f4"), ("parallax_px", "<f4")])
LINK_DTYPE = np.dtype([("scale", "<f8"), ("q25", "<f8"), ("q75", "<f8"), ("n_shared", "<i4"), ("q", "<i4"), ("flags", "<i4"), ("reserved_", "<i4")])


class Params:
    def __init__(self, require=MP_KEPT, min_shared=8, max_rel_spread=1.0, min_scale=1.0 / 64.0, max_scale=64.0):
        self.require, self.min_shared, self.max_rel_spread, self.min_scale, self.max_scale = require, min_shared, max_rel_spread, min_scale, max_scale


def norm_prev(prev, i):
    p = int(prev[i])
    if p >= 0:
        return p if p < i else KF_FIRST
    return p if p in (KF_CARRIED, KF_NOT_SAVED) else KF_FIRST


def pose_usable(R, t):
    R, t = [float(v) for v in R], [float(v) for v in t]
    if not all(math.isfinite(v) for v in R + t) or not any(v != 0.0 for v in R):
        return False
    tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    return math.isfinite(tt) and tt > 0.0


def has_row(prev, pose, i):
    p = norm_prev(prev, i)
    return (p >= 0 or p == KF_CARRIED) and pose_usable(pose[i]["R"], pose[i]["t"])


def _pos(v):
    return math.isfinite(v) and v > 0.0


def depth_row(sp, links, m, R, t, points, flags, row_cap):
    row = [0.0] * row_cap
    won = set()
    for k in range(m):
        kp = int(links[k]["trainIdx"])
        if not 0 <= kp < row_cap or (int(flags[k]) & sp.require) != sp.require or kp in won:
            continue
        won.add(kp)
        X = [float(v) for v in points[k]["X"]]
        z2 = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2]
        row[kp] = z2 if _pos(z2) else 0.0
    return row


def ratios(sp, links, m, points, flags, qrow, row_cap):
    out = []
    for c in range(m):
        kp = int(links[c]["queryIdx"])
        if not 0 <= kp < row_cap or (int(flags[c]) & sp.require) != sp.require:
            continue
        z2, z1 = float(qrow[kp]), float(points[c]["X"][2])
        if _pos(z2) and _pos(z1):
            rho = z2 / z1
            if _pos(rho):
                out.append(rho)
    return out


def record(sp, rho, q):
    """the LINK_DTYPE fields of a frame whose ratios are rho"""
    ns = len(rho)
    s = sorted(rho)
    scale, q25, q75 = (s[(ns - 1) // 2], s[(ns - 1) // 4], s[(3 * (ns - 1)) // 4]) if ns else (0.0, 0.0, 0.0)
    fl = 0
    if ns < sp.min_shared:
        fl |= SL_FEW
    if q75 - q25 > sp.max_rel_spread * scale:
        fl |= SL_SPREAD
    if not (sp.min_scale <= scale <= sp.max_scale):
        fl |= SL_RANGE
    return (scale, q25, q75, ns, q, fl, 0)


def scale_link_rows(sp, prev, links, nlinks, pose, points, flags, row_cap, carry=None):
    """links: (n, link_cap) DMATCH_DTYPE; pose: n POSE_DTYPE; points / flags: (n, pts_cap); carry: None or row_cap doubles.
    Returns (depth (n, row_cap) float64, link (n) LINK_DTYPE)."""
    n = len(prev)
    mcap = min(links.shape[1], points.shape[1]) if n else 0
    depth = np.zeros((n, row_cap), np.float64)
    link = np.zeros(n, LINK_DTYPE)
    ms = [min(max(int(nlinks[i]), 0), mcap) for i in range(n)]
    for i in range(n):
        if has_row(prev, pose, i):
            R, t = [float(v) for v in pose[i]["R"]], [float(v) for v in pose[i]["t"]]
            depth[i] = depth_row(sp, links[i], ms[i], R, t, points[i], flags[i], row_cap)
    for i in range(n):
        p = norm_prev(prev, i)
        if p in (KF_NOT_SAVED, KF_FIRST):
            link[i] = (0.0, 0.0, 0.0, 0, p, SL_NO_PAIR, 0)
        elif p == KF_CARRIED and carry is None:
            link[i] = (0.0, 0.0, 0.0, 0, p, SL_NO_DEPTH, 0)
        else:
            qrow = carry if p == KF_CARRIED else depth[p]
            if not any(_pos(float(z)) for z in qrow):               # a row without a depth: q had no pair, no usable pose or no point
                link[i] = (0.0, 0.0, 0.0, 0, p, SL_NO_DEPTH, 0)
                continue
            link[i] = record(sp, ratios(sp, links[i], ms[i], points[i], flags[i], qrow, row_cap), p)
    return depth, link


def carry_out(prev, depth, carry, row_cap):
    """the row the plan keeps for the next launch: that of the last saved frame, else the row it was given, else zeros"""
    saved = [i for i in range(len(prev)) if norm_prev(prev, i) != KF_NOT_SAVED]
    if saved:
        return depth[saved[-1]].copy()
    return np.array(carry, np.float64) if carry is not None else np.zeros(row_cap)
