"""Restatement of the feature-track contract of include/vislam_hip.h (not a test module; nothing here calls the code under test).

The track contract.  A LINK LIST of frame i holds vis_dmatch entries whose queryIdx is a keypoint of frame prev[i] and whose trainIdx is a
keypoint of frame i.  prev[i] is an index < i or a VIS_KF_* value (anything else counts as VIS_KF_FIRST).  Frame i takes part with nk(i)
keypoints: 0 when prev[i] == VIS_KF_NOT_SAVED, else its count clamped to [0, row_cap].  Its parent is frame prev[i], or the carried row when
prev[i] == VIS_KF_CARRIED and a row is given (its keypoints: the entries with len > 0), else none.  Of the first m entries of the list (the
count clamped to [0, link_cap], with a mask also to mask_cap) entry c is a CANDIDATE iff the frame has a parent, both indices are keypoints
of their frames (unsigned compares) and its mask byte, when there is a mask, is non-zero.  A candidate LINKS iff no earlier candidate has the
same trainIdx and none has the same queryIdx -- first in list order wins on both sides, a loser still occupies its other side.  A linked
keypoint continues its parent's track; every other keypoint k < nk(i) starts one.

  link_rows           vis_ftrack_link_rows: numpy, the device's own scheme (minimum list position per side, then pointer doubling)
  triangulate_track   one track's N-view point in plain Python floats (IEEE binary64, one rounding per + - * / sqrt, nothing contracted), in the
                      parenthesisation and view order of csrc/ftrack.hip
  triangulate_rows    vis_ftrack_triangulate_rows on top of it: the walk, the records, flag bytes and summaries"""
import math

import numpy as np

from triangulate_ref import _div, jacobi_eig4

KF_CARRIED, KF_NOT_SAVED, KF_FIRST = -1, -2, -3
FT_NO_PAIR, FT_NO_CARRY = 1, 2
FT_SYM, FT_GOOD = 0, 1
FTP_FRONT, FTP_REPROJ_OK, FTP_PARALLAX_OK, FTP_KEPT, FTP_FEW, FTP_SINGULAR = 1, 2, 4, 8, 16, 32
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
OBS_DTYPE = np.dtype([("birth_seq", "<i4"), ("birth_kp", "<i4"), ("len", "<i4"), ("prev_kp", "<i4")])
FRAME_DTYPE = np.dtype([("seq", "<i4"), ("n_keypoints", "<i4"), ("n_continued", "<i4"), ("n_started", "<i4"), ("n_ended", "<i4"),
                        ("max_len", "<i4"), ("sum_len", "<i4"), ("flags", "<i4")])
POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("rms_reproj_px", "<f4"), ("parallax_cos", "<f4"), ("n_views", "<i4"), ("flags", "<i4")])
TRI_SUMMARY_DTYPE = np.dtype([("n_ends", "<i4"), ("n_points", "<i4"), ("n_kept", "<i4"), ("n_front", "<i4"), ("n_reproj_ok", "<i4"),
                              ("n_parallax_ok", "<i4"), ("n_few", "<i4"), ("n_singular", "<i4")])
EMPTY_OBS = (-1, -1, 0, -1)
NONE = np.iinfo(np.int64).max


def counts(prev, nkp, row_cap):
    """nk(i)"""
    prev, nkp = np.asarray(prev, np.int64), np.asarray(nkp, np.int64)
    return np.where(prev == KF_NOT_SAVED, 0, np.clip(nkp, 0, row_cap))


def parent_of(prev, i, have_carry):
    p = int(prev[i])
    if p >= 0:
        return p if p < i else KF_FIRST
    return KF_CARRIED if p == KF_CARRIED and have_carry else KF_FIRST


def empty_row(row_cap):
    r = np.zeros(row_cap, OBS_DTYPE)
    r[:] = EMPTY_OBS
    return r


def link_rows(prev, nkp, links, nlinks, row_cap, mask=None, carry=None, seq0=0):
    """links: (n, link_cap) DMATCH_DTYPE; nlinks: n; mask: None or (n, mask_cap) uint8; carry: None or row_cap OBS_DTYPE.
    Returns (obs (n, row_cap) OBS_DTYPE, frames (n) FRAME_DTYPE)."""
    n, R = len(prev), row_cap
    link_cap = links.shape[1] if n else 0
    nk = counts(prev, nkp, R)
    have = carry is not None
    anc = np.arange(n * R, dtype=np.int64)                          # >= 0: element i * R + k; <= -2: entry -(a + 2) of the carried row
    dist = np.zeros(n * R, np.int64)
    par = np.full(n * R, -1, np.int64)
    for i in range(n):
        p = parent_of(prev, i, have)
        m = min(max(int(nlinks[i]), 0), link_cap)
        if mask is not None:
            m = min(m, mask.shape[1])
        if p == KF_FIRST or m == 0:
            continue
        q = links[i, :m]["queryIdx"].astype(np.int64)
        t = links[i, :m]["trainIdx"].astype(np.int64)
        ok = (t >= 0) & (t < nk[i])
        if p >= 0:
            ok &= (q >= 0) & (q < nk[p])
        else:
            ok &= (q >= 0) & (q < R)
            ok[ok] = carry["len"][q[ok]] > 0
        if mask is not None:
            ok &= mask[i, :m] != 0
        c = np.nonzero(ok)[0]
        win_t, win_q = np.full(R, NONE), np.full(R, NONE)
        np.minimum.at(win_t, t[c], c)
        np.minimum.at(win_q, q[c], c)
        w = c[(win_t[t[c]] == c) & (win_q[q[c]] == c)]
        e = i * R + t[w]
        par[e] = q[w]
        anc[e] = p * R + q[w] if p >= 0 else -(q[w] + 2)
        dist[e] = 1
    reach = 1
    while reach < n:                                                # ceil(log2 n) rounds, each from the state of the round before
        a = anc.copy()
        go = (a >= 0) & (a != np.arange(n * R))
        aa = np.where(go, anc[np.where(go, a, 0)], a)
        step = go & (aa != a)
        anc = np.where(step, aa, a)
        dist = np.where(step, dist + dist[np.where(go, a, 0)], dist)
        reach *= 2
    obs = np.zeros((n, R), OBS_DTYPE)
    obs[:] = EMPTY_OBS
    frames = np.zeros(n, FRAME_DTYPE)
    for i in range(n):
        k = np.arange(int(nk[i]))
        e = i * R + k
        a, d = anc[e], dist[e]
        root = a >= 0
        o = obs[i, :len(k)]
        o["birth_seq"] = np.where(root, seq0 + a // R, 0)
        o["birth_kp"] = np.where(root, a % R, 0)
        o["len"] = np.where(root, d + 1, 0)
        if (~root).any():
            cq = -(a[~root] + 2)
            sel = np.nonzero(~root)[0]
            o["birth_seq"][sel] = carry["birth_seq"][cq]
            o["birth_kp"][sel] = carry["birth_kp"][cq]
            o["len"][sel] = carry["len"][cq] + d[~root]
        o["prev_kp"] = par[e]
        p = parent_of(prev, i, have)
        cont = int((par[e] >= 0).sum())
        parent_n = 0 if p == KF_FIRST else int(nk[p]) if p >= 0 else int((carry["len"] > 0).sum())
        f = frames[i]
        f["seq"], f["n_keypoints"], f["n_continued"], f["n_started"] = seq0 + i, int(nk[i]), cont, int(nk[i]) - cont
        f["n_ended"] = 0 if p == KF_FIRST else parent_n - cont
        f["max_len"] = int(o["len"].max()) if len(k) else 0
        f["sum_len"] = np.int64(o["len"].astype(np.int64).sum()).astype(np.int32)
        f["flags"] = 0 if p != KF_FIRST else FT_NO_CARRY if int(prev[i]) == KF_CARRIED else FT_NO_PAIR
    return obs, frames


def carry_out(prev, obs, carry, row_cap):
    """the row the plan keeps for the next launch: that of the last saved frame, else the row it was given, else an empty one"""
    saved = [i for i in range(len(prev)) if int(prev[i]) != KF_NOT_SAVED]
    if saved:
        return obs[saved[-1]].copy()
    return carry.copy() if carry is not None else empty_row(row_cap)


# ---------------------------------------------------------------------------------------------- N-view triangulation
class TriParams:
    def __init__(self, max_views=16, min_views=2, gn_iters=5, max_reproj_px=2.0, max_parallax_cos=0.9998476951563913):
        self.max_views, self.min_views, self.gn_iters = max_views, min_views, gn_iters
        self.max_reproj_px, self.max_parallax_cos = max_reproj_px, max_parallax_cos


class Camera:
    def __init__(self, fx=458.654, fy=457.296, cx=367.215, cy=248.375):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)


def has_pose(P):
    return all(math.isfinite(v) for v in P) and any(v != 0.0 for v in P[:9])


def cost_pass(cam, views, X):
    """(H00, H01, H02, H11, H12, H22, g0, g1, g2, cost, front, reproj_e2_max_ok(thr2 applied by the caller): list of e2, c_new, c_old)"""
    H00 = H01 = H02 = H11 = H12 = H22 = g0 = g1 = g2 = cost = 0.0
    front, e2s, c_new, c_old = True, [], None, None
    for P, u, v in views:
        U = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[9]
        V = ((P[3] * X[0] + P[4] * X[1]) + P[5] * X[2]) + P[10]
        W = ((P[6] * X[0] + P[7] * X[1]) + P[8] * X[2]) + P[11]
        iw = _div(1.0, W)
        un, vn = U * iw, V * iw
        ru, rv = (cam.fx * un + cam.cx) - u, (cam.fy * vn + cam.cy) - v
        fu, fv = cam.fx * iw, cam.fy * iw
        ju0, ju1, ju2 = fu * (P[0] - un * P[6]), fu * (P[1] - un * P[7]), fu * (P[2] - un * P[8])
        jv0, jv1, jv2 = fv * (P[3] - vn * P[6]), fv * (P[4] - vn * P[7]), fv * (P[5] - vn * P[8])
        H00 += ju0 * ju0 + jv0 * jv0
        H01 += ju0 * ju1 + jv0 * jv1
        H02 += ju0 * ju2 + jv0 * jv2
        H11 += ju1 * ju1 + jv1 * jv1
        H12 += ju1 * ju2 + jv1 * jv2
        H22 += ju2 * ju2 + jv2 * jv2
        g0 += ju0 * ru + jv0 * rv
        g1 += ju1 * ru + jv1 * rv
        g2 += ju2 * ru + jv2 * rv
        e2 = ru * ru + rv * rv
        cost += e2
        front = front and W > 0.0
        e2s.append(e2)
        c = (-((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]), -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]),
             -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]))
        if c_new is None:
            c_new = c
        c_old = c
    return dict(H=(H00, H01, H02, H11, H12, H22), g=(g0, g1, g2), cost=cost, front=front, e2s=e2s, c_new=c_new, c_old=c_old)


def dlt_point(cam, views):
    """(X or None when singular) of the used views, newest first"""
    A = [0.0] * 10
    for P, u, v in views:
        x, y = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
        r = (x * P[6] - P[0], x * P[7] - P[1], x * P[8] - P[2], x * P[11] - P[9])
        s = (y * P[6] - P[3], y * P[7] - P[4], y * P[8] - P[5], y * P[11] - P[10])
        j = 0
        for a in range(4):
            for b in range(a, 4):
                A[j] += r[a] * r[b] + s[a] * s[b]
                j += 1
    M = [A[0], A[1], A[2], A[3], A[1], A[4], A[5], A[6], A[2], A[5], A[7], A[8], A[3], A[6], A[8], A[9]]
    V, _, _ = jacobi_eig4(M)
    mn = 0
    for j in range(1, 4):
        if M[5 * j] < M[5 * mn]:
            mn = j
    E = [V[mn], V[4 + mn], V[8 + mn], V[12 + mn]]
    X = [_div(E[0], E[3]), _div(E[1], E[3]), _div(E[2], E[3])]
    if E[3] == 0.0 or not all(math.isfinite(c) for c in X):
        return None
    return X


def _pivot_ok(D):
    return D > 0.0 and math.isfinite(D)


def gn_step(r):
    """the LDL^T step of one pass, or None when a pivot fails"""
    H00, H01, H02, H11, H12, H22 = r["H"]
    g0, g1, g2 = r["g"]
    D0 = H00
    if not _pivot_ok(D0):
        return None
    L10, L20 = H01 / D0, H02 / D0
    D1 = H11 - (L10 * L10) * D0
    if not _pivot_ok(D1):
        return None
    L21 = (H12 - (L20 * L10) * D0) / D1
    D2 = (H22 - (L20 * L20) * D0) - (L21 * L21) * D1
    if not _pivot_ok(D2):
        return None
    z0 = -g0
    z1 = -g1 - L10 * z0
    z2 = (-g2 - L20 * z0) - L21 * z1
    d2 = z2 / D2
    d1 = z1 / D1 - L21 * d2
    d0 = (z0 / D0 - L10 * d1) - L20 * d2
    return d0, d1, d2


def zero_point():
    return np.zeros(1, POINT_DTYPE)[0]


def triangulate_track(tp, cam, views, with_trace=False):
    """views: [(P (12 floats), u, v)] of the USED views, newest first.  Returns the POINT_DTYPE record (and, with_trace, the cost of every iterate)."""
    pt = zero_point()
    pt["n_views"] = len(views)
    trace = []
    if len(views) < tp.min_views:
        pt["flags"] = FTP_FEW
        return (pt, trace) if with_trace else pt
    X = dlt_point(cam, views)
    if X is None:
        pt["flags"] = FTP_SINGULAR
        return (pt, trace) if with_trace else pt
    r = cost_pass(cam, views, X)
    best, B = r, list(X)
    trace.append(r["cost"])
    if not math.isfinite(r["cost"]):                                # a point in a camera's plane, an overflow: nothing to refine or report
        pt["flags"] = FTP_SINGULAR
        return (pt, trace) if with_trace else pt
    for _ in range(tp.gn_iters):
        d = gn_step(r)
        if d is None:
            break
        X = [X[0] + d[0], X[1] + d[1], X[2] + d[2]]
        r = cost_pass(cam, views, X)
        trace.append(r["cost"])
        if r["cost"] < best["cost"]:
            best, B = r, list(X)
    a = [best["c_new"][j] - B[j] for j in range(3)]
    b = [best["c_old"][j] - B[j] for j in range(3)]
    dab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    daa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    dbb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    prod = daa * dbb
    cs = _div(dab, math.sqrt(prod) if prod == prod else float("nan"))
    cs_ok = math.isfinite(cs)
    if not cs_ok:
        cs = 1.0
    thr2 = tp.max_reproj_px * tp.max_reproj_px
    with np.errstate(all="ignore"):
        pt["X"] = B
        q = best["cost"] / float(len(views))
        pt["rms_reproj_px"] = np.float32(math.sqrt(q) if q == q else float("nan"))
        pt["parallax_cos"] = np.float32(cs)
    f = (FTP_FRONT if best["front"] else 0) | (FTP_REPROJ_OK if all(e2 <= thr2 for e2 in best["e2s"]) else 0) | \
        (FTP_PARALLAX_OK if cs_ok and cs <= tp.max_parallax_cos else 0)
    if f == (FTP_FRONT | FTP_REPROJ_OK | FTP_PARALLAX_OK):
        f |= FTP_KEPT
    pt["flags"] = f
    return (pt, trace) if with_trace else pt


def track_parent(prev, nk, obs, i, k):
    """(frame, keypoint) of the parent of (i, k) inside the call, or None"""
    p = int(prev[i])
    if p < 0 or p >= i:
        return None
    q = int(obs[i, k]["prev_kp"])
    if q < 0 or q >= int(nk[p]):
        return None
    return p, q


def triangulate_rows(tp, cam, prev, nkp, obs, xy, poses, points=None, flags=None):
    """obs: (n, row_cap) OBS_DTYPE; xy: (n, row_cap, 2) float32; poses: (n, 12).  points / flags: the buffers as they stand before the call
    (entries k >= nk(i) keep their bytes); returns (points (n, row_cap) POINT_DTYPE, flags (n, row_cap) uint8, summary (n) TRI_SUMMARY_DTYPE)."""
    n, R = obs.shape
    nk = counts(prev, nkp, R)
    points = np.zeros((n, R), POINT_DTYPE) if points is None else points.copy()
    flags = np.zeros((n, R), np.uint8) if flags is None else flags.copy()
    summary = np.zeros(n, TRI_SUMMARY_DTYPE)
    child = np.zeros((n, R), bool)
    for i in range(n):
        for k in range(int(nk[i])):
            pq = track_parent(prev, nk, obs, i, k)
            if pq is not None:
                child[pq] = True
    P = [[float(v) for v in poses[i]] for i in range(n)]
    ok_pose = [has_pose(P[i]) for i in range(n)]
    for i in range(n):
        for k in range(int(nk[i])):
            if child[i, k]:
                points[i, k], flags[i, k] = zero_point(), 0
                continue
            views, cur = [], (i, k)
            for _ in range(tp.max_views):
                f, kk = cur
                u, v = float(xy[f, kk, 0]), float(xy[f, kk, 1])
                if ok_pose[f] and math.isfinite(u) and math.isfinite(v):
                    views.append((P[f], u, v))
                cur = track_parent(prev, nk, obs, f, kk)
                if cur is None:
                    break
            pt = triangulate_track(tp, cam, views)
            points[i, k], flags[i, k] = pt, int(pt["flags"])
            fl, s = int(pt["flags"]), summary[i]
            s["n_ends"] += 1
            s["n_points"] += int(not fl & (FTP_FEW | FTP_SINGULAR))
            s["n_kept"] += int(bool(fl & FTP_KEPT))
            s["n_front"] += int(bool(fl & FTP_FRONT))
            s["n_reproj_ok"] += int(bool(fl & FTP_REPROJ_OK))
            s["n_parallax_ok"] += int(bool(fl & FTP_PARALLAX_OK))
            s["n_few"] += int(bool(fl & FTP_FEW))
            s["n_singular"] += int(bool(fl & FTP_SINGULAR))
    return points, flags, summary
