"""Restatement of the windowed bundle adjustment of include/vislam_hip.h (vis_ba_rows; not a test module, nothing here calls the code under test).

Everything is IEEE binary64 with one rounding per + - * / sqrt and nothing contracted.  numpy is used ELEMENTWISE only (one ufunc per operation,
so every element sees the same roundings as a Python float would); every sum runs in the order the contract fixes: a point's views in walk
order, newest to oldest; points in slot order (frame rising, keypoint rising); accumulators start at 0.0 and absent terms are skipped.

The contract, in the order the code below follows it.
  WINDOWS.  S = stride.  Window j covers frames first = j S ... last = min(first + S, n - 1); there are ceil((n - 1) / S) of them (none for n <= 1,
  where the poses are copied and nothing else is written).  A frame HAS A POSE under ftri_view's rule on the INPUT poses.  anchor = the first posed
  frame of the window (-1: none), the FREE frames are the posed frames after it (camera index c = their rank, rising), n_free <= 16.  Window j
  OWNS the slots (i, k < nk(i)) of frames first + 1 ... last, window 0 also those of frame 0.
  POINTS.  An owned slot that a keypoint of a later owned frame of the window names as its parent (ftri_parent, parent frame owned) gets the zero
  record and flag byte 0.  Every other owned slot is a window-end: steps 1-3 of the N-view triangulation (ftrack_ref.triangulate_track) over its walk
  restricted to frames >= anchor (>= first without an anchor), max_views 17, min_views, tri_gn_iters, max_reproj_px = init_reproj_px, under the
  input poses.  FEW -> VIS_BAP_FEW (n_views set, the rest zero); SINGULAR, not FRONT or not REPROJ_OK -> VIS_BAP_INIT_REJECTED (n_views, and
  rms0_px when the cost was finite; X zero); else VIS_BAP_USED with X, rms0_px = rms1_px = the triangulation's rms.
  n_points / n_obs count the used points and their views.  n_free == 0 or n_points < min_points: VIS_BA_FEW, nothing is solved.
  OBSERVATION at pose P and point X, pixel (u, v):  U, V, W, iw, un, vn, ru, rv, fu = fx iw, fv = fy iw, Ju_k, Jv_k as in the triangulation;
  e2 = ru ru + rv rv, e = sqrt(e2); w = 1, term = e2 when huber == 0 or e <= huber, else w = huber / e, term = (2 huber) e - huber huber;
  camera rows  Cu = (-(fu (un V)), fu (W + un U), -(fu V), fu, 0, -(fu un)),  Cv = (-(fv (W + vn V)), fv (vn U), fv U, 0, fv, -(fv vn)).
  LINEARISATION.  Per point V_ab += w (Ju_a Ju_b + Jv_a Jv_b), g_a += w (Ju_a ru + Jv_a rv); the diagonal times (1 + lambda); the 3 x 3 LDL^T of
  the triangulation (a pivot not > 0 or not finite: the point sits the linearisation out -- no term anywhere, its X stays); Vi = the inverse,
  column j = the LDL^T solution of e_j, the upper triangle read from (row <= column).  Per free view W_ak = w (Cu_a Ju_k + Cv_a Jv_k),
  Y_ak = (W_a0 Vi_0k + W_a1 Vi_1k) + W_a2 Vi_2k.  Over the points in slot order: U_ab += w (Cu_a Cu_b + Cv_a Cv_b) (a <= b), b_a += w (Cu_a ru +
  Cv_a rv), T[6 c1 + a][6 c2 + b] += (Y1_a0 W2_b0 + Y1_a1 W2_b1) + Y1_a2 W2_b2 (row <= column), Tg[6 c + a] += (Y_a0 g_0 + Y_a1 g_1) + Y_a2 g_2.
  A = Ud - T with Ud = U in the diagonal blocks (diagonal entries times (1 + lambda)) and 0.0 elsewhere; rhs = -(b - Tg).  LDL^T without
  pivoting (D_j = A_jj - sum_c (L_jc L_jc) D_c, L_ij = (A_ij - sum_c (L_ic L_jc) D_c) / D_j, c rising; z_i = rhs_i - sum_{c<i} L_ic z_c;
  d_i = z_i / D_i - sum_{c>i} L_ci d_c, c rising).  A pivot not > 0 or not finite: rejection.
  CANDIDATE.  Free poses by the PnP refinement's Cayley update; per point Q_k = the sum over its free views in walk order of
  ((((W_0k d_0 + W_1k d_1) + W_2k d_2) + W_3k d_3) + W_4k d_4) + W_5k d_5, s_k = -g_k - Q_k, dX_k = (Vi_k0 s_0 + Vi_k1 s_1) + Vi_k2 s_2; X + dX.
  cost = sum over points in slot order of (sum over views in walk order of term).  Accepted iff finite and < the current cost:
  lambda <- max(lambda / 10, 1e-12); else lambda <- min(10 lambda, 1e12).
  AFTER THE SOLVE (windows that solved).  rms1_px = (float) sqrt(sum e2 / n_views) at the final state.  With n_accepted > 0 the scale gauge:
  ca, cin, cout = centres of the anchor (input), the last posed frame (input, final); scale = sqrt(|cin - ca|^2) / sqrt(|cout - ca|^2); not
  finite or not > 0: scale 1, VIS_BA_NO_SCALE, nothing applied; else c' = ca + scale (c - ca), t' = -(R c') for every free frame and
  X' = ca + scale (X - ca) for every used point.
  STITCH, in window order.  A_in = the anchor's input pose; A_out = A_in for window 0 and for a window whose anchor is not its first frame (then
  VIS_BA_RESTART, for j > 0), else the output pose already written for the shared frame.  A_out == A_in byte for byte: the window's poses and
  points are the output.  Else pose_i <- (pose_i o A_in^-1) o A_out and X <- A_out^-1 (A_in X).  An output pose that is not finite is replaced
  by the input pose, a moved point that is not finite keeps its X.  Frames without a pose, window 0's anchor and a restarted anchor get their input bytes."""
import math

import numpy as np

import ftrack_ref as fr

BA_REFINED, BA_FEW, BA_RESTART, BA_NO_SCALE = 1, 2, 4, 8
BAP_USED, BAP_INIT_REJECTED, BAP_FEW = 1, 2, 4
WINDOW_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("anchor", "<i4"), ("n_free", "<i4"), ("n_points", "<i4"), ("n_obs", "<i4"),
                         ("n_lin", "<i4"), ("n_accepted", "<i4"), ("n_rejected", "<i4"), ("flags", "<i4"), ("reserved_", "<i4", (2,)),
                         ("cost0", "<f8"), ("cost1", "<f8"), ("lambda_", "<f8"), ("scale", "<f8")])
POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("rms0_px", "<f4"), ("rms1_px", "<f4"), ("n_views", "<i4"), ("flags", "<i4")])
MAXV = 17


class Params:
    def __init__(self, stride=8, min_views=2, min_points=12, lm_iters=10, tri_gn_iters=5, huber_px=2.4477, init_reproj_px=16.0, lambda0=1e-4):
        self.stride, self.min_views, self.min_points, self.lm_iters, self.tri_gn_iters = stride, min_views, min_points, lm_iters, tri_gn_iters
        self.huber_px, self.init_reproj_px, self.lambda0 = float(huber_px), float(init_reproj_px), float(lambda0)


def n_windows(n, stride):
    return (n - 1 + stride - 1) // stride if n > 1 else 0


def _parent(prev, nk, obs, i, k, lo):
    p = int(prev[i])
    if p < lo or p >= i:
        return None
    q = int(obs[i, k]["prev_kp"])
    if q < 0 or q >= int(nk[p]):
        return None
    return p, q


def centre(P):
    return np.array([-((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]), -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]),
                     -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11])])


def cayley_update(P, d):
    """R <- C(w) R, t <- C(w) t + dt of the PnP refinement, on 12 + 6 Python floats"""
    h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
    s = 2.0 / (1.0 + hh)
    K = [0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0]
    C = [0.0] * 9
    for i in range(3):
        for j in range(3):
            k2 = h[i] * h[j] - hh if i == j else h[i] * h[j]
            C[3 * i + j] = (1.0 if i == j else 0.0) + s * (K[3 * i + j] + k2)
    N = [0.0] * 12
    for i in range(3):
        for j in range(3):
            N[3 * i + j] = (C[3 * i] * P[j] + C[3 * i + 1] * P[3 + j]) + C[3 * i + 2] * P[6 + j]
        N[9 + i] = ((C[3 * i] * P[9] + C[3 * i + 1] * P[10]) + C[3 * i + 2] * P[11]) + d[3 + i]
    return N


class _Window:
    """the points of one window as padded arrays: vf (NP, 17) local frame of view position v or -1, vu / vv its pixel"""

    def __init__(self, first, slots, views):
        self.slots = slots
        NP = len(slots)
        self.vf = np.full((NP, MAXV), -1, np.int64)
        self.vu = np.zeros((NP, MAXV))
        self.vv = np.zeros((NP, MAXV))
        for p, vw in enumerate(views):
            for v, (f, u, w) in enumerate(vw):
                self.vf[p, v], self.vu[p, v], self.vv[p, v] = f - first, u, w
        self.pres = self.vf >= 0


def _observe(cam, bp, W, P, X):
    """every observation of the window at poses P (nf, 12) and points X (NP, 3): dict of (NP, 17) arrays (garbage where not present)"""
    with np.errstate(all="ignore"):
        Pv = P[np.maximum(W.vf, 0)]                                    # (NP, 17, 12)
        x0, x1, x2 = X[:, 0, None], X[:, 1, None], X[:, 2, None]
        U = ((Pv[..., 0] * x0 + Pv[..., 1] * x1) + Pv[..., 2] * x2) + Pv[..., 9]
        V = ((Pv[..., 3] * x0 + Pv[..., 4] * x1) + Pv[..., 5] * x2) + Pv[..., 10]
        Wd = ((Pv[..., 6] * x0 + Pv[..., 7] * x1) + Pv[..., 8] * x2) + Pv[..., 11]
        iw = 1.0 / Wd
        un, vn = U * iw, V * iw
        ru, rv = (cam.fx * un + cam.cx) - W.vu, (cam.fy * vn + cam.cy) - W.vv
        fu, fv = cam.fx * iw, cam.fy * iw
        e2 = ru * ru + rv * rv
        e = np.sqrt(e2)
        h = bp.huber_px
        quad = np.full(e.shape, True) if h == 0.0 else e <= h
        w = np.where(quad, 1.0, h / e)
        term = np.where(quad, e2, (2.0 * h) * e - h * h)
        ju = np.stack([fu * (Pv[..., k] - un * Pv[..., 6 + k]) for k in range(3)], -1)
        jv = np.stack([fv * (Pv[..., 3 + k] - vn * Pv[..., 6 + k]) for k in range(3)], -1)
        z = np.zeros_like(fu)
        cu = np.stack([-(fu * (un * V)), fu * (Wd + un * U), -(fu * V), fu, z, -(fu * un)], -1)
        cv = np.stack([-(fv * (Wd + vn * V)), fv * (vn * U), fv * U, z, fv, -(fv * vn)], -1)
    return dict(ru=ru, rv=rv, e2=e2, w=w, term=term, ju=ju, jv=jv, cu=cu, cv=cv)


def _ordered(pres, terms):
    """per point: the sum of terms (NP, 17, ...) over the present views in walk order, from 0.0"""
    acc = np.zeros(terms.shape[:1] + terms.shape[2:])
    with np.errstate(all="ignore"):
        for v in range(MAXV):
            m = pres[:, v].reshape((-1,) + (1,) * (terms.ndim - 2))
            acc = np.where(m, acc + terms[:, v], acc)
    return acc


def _cost(W, o):
    """sum over the points in slot order of their walk-order sums"""
    per = _ordered(W.pres, o["term"])
    c = 0.0
    for v in per:
        c = c + float(v)
    return c


def _solve3(L10, L20, L21, D0, D1, D2, b0, b1, b2):
    z0 = b0
    z1 = b1 - L10 * z0
    z2 = (b2 - L20 * z0) - L21 * z1
    x2 = z2 / D2
    x1 = z1 / D1 - L21 * x2
    x0 = (z0 / D0 - L10 * x1) - L20 * x2
    return x0, x1, x2


def _point_blocks(W, o, lam1):
    """V, g, the damped LDL^T, the inverse: (ok (NP), Vi (NP, 3, 3) symmetric, g (NP, 3), Wc (NP, 17, 6, 3))"""
    ju, jv, w = o["ju"], o["jv"], o["w"]
    with np.errstate(all="ignore"):
        idx = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        Vt = np.stack([w * (ju[..., a] * ju[..., b] + jv[..., a] * jv[..., b]) for a, b in idx], -1)
        gt = np.stack([w * (ju[..., a] * o["ru"] + jv[..., a] * o["rv"]) for a in range(3)], -1)
        V, g = _ordered(W.pres, Vt), _ordered(W.pres, gt)
        H00, H01, H02, H11, H12, H22 = V[:, 0] * lam1, V[:, 1], V[:, 2], V[:, 3] * lam1, V[:, 4], V[:, 5] * lam1
        piv = lambda D: (D > 0.0) & np.isfinite(D)
        D0 = H00
        L10, L20 = H01 / D0, H02 / D0
        D1 = H11 - (L10 * L10) * D0
        L21 = (H12 - (L20 * L10) * D0) / D1
        D2 = (H22 - (L20 * L20) * D0) - (L21 * L21) * D1
        ok = piv(D0) & piv(D1) & piv(D2)
        one, zero = np.ones_like(D0), np.zeros_like(D0)
        c0 = _solve3(L10, L20, L21, D0, D1, D2, one, zero, zero)
        c1 = _solve3(L10, L20, L21, D0, D1, D2, zero, one, zero)
        c2 = _solve3(L10, L20, L21, D0, D1, D2, zero, zero, one)
        Vi = np.empty((len(D0), 3, 3))
        Vi[:, 0, 0], Vi[:, 0, 1], Vi[:, 0, 2], Vi[:, 1, 1], Vi[:, 1, 2], Vi[:, 2, 2] = c0[0], c1[0], c2[0], c1[1], c2[1], c2[2]
        Vi[:, 1, 0], Vi[:, 2, 0], Vi[:, 2, 1] = Vi[:, 0, 1], Vi[:, 0, 2], Vi[:, 1, 2]
        cu, cv = o["cu"], o["cv"]
        Wc = w[..., None, None] * (cu[..., :, None] * ju[..., None, :] + cv[..., :, None] * jv[..., None, :])
    return ok, Vi, g, Wc


def _ldl_solve(A, rhs):
    """A: symmetric (N, N), destroyed.  Returns d or None when a pivot fails"""
    N = len(rhs)
    L, D = np.zeros((N, N)), np.zeros(N)
    with np.errstate(all="ignore"):
        for j in range(N):
            d = float(A[j, j])
            if not (d > 0.0 and math.isfinite(d)):
                return None
            D[j] = d
            l = A[j + 1:, j] / d
            L[j + 1:, j] = l
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - (l[:, None] * l[None, :]) * d
        z = rhs.copy()
        for c in range(N):
            z[c + 1:] = z[c + 1:] - L[c + 1:, c] * z[c]
        x = np.zeros(N)
        for i in range(N - 1, -1, -1):
            v = z[i] / D[i]
            for c in range(i + 1, N):
                v = v - L[c, i] * x[c]
            x[i] = v
    return x


def _linearise(cam, bp, W, cidx, P, X, lam):
    """one linearisation: (delta (6 F) or None, ok, Vi, g, Wc)"""
    F = int(cidx.max()) + 1
    N = 6 * F
    lam1 = 1.0 + lam
    o = _observe(cam, bp, W, P, X)
    ok, Vi, g, Wc = _point_blocks(W, o, lam1)
    U, b, T, Tg = np.zeros((N, N)), np.zeros(N), np.zeros((N, N)), np.zeros(N)
    cam_of = np.where(W.pres, cidx[np.maximum(W.vf, 0)], -1)            # (NP, 17)
    with np.errstate(all="ignore"):
        for p in range(len(W.slots)):
            if not ok[p]:
                continue
            vs = np.nonzero(cam_of[p] >= 0)[0]
            if len(vs) == 0:
                continue
            cs = cam_of[p, vs]
            cu, cv, w = o["cu"][p, vs], o["cv"][p, vs], o["w"][p, vs]
            Ub = w[:, None, None] * (cu[:, :, None] * cu[:, None, :] + cv[:, :, None] * cv[:, None, :])
            bb = w[:, None] * (cu * o["ru"][p, vs, None] + cv * o["rv"][p, vs, None])
            Wp, vi, gp = Wc[p, vs], Vi[p], g[p]
            Y = np.stack([(Wp[:, :, 0] * vi[0, k] + Wp[:, :, 1] * vi[1, k]) + Wp[:, :, 2] * vi[2, k] for k in range(3)], -1)
            Tb = (Y[:, :, None, None, 0] * Wp[None, None, :, :, 0] + Y[:, :, None, None, 1] * Wp[None, None, :, :, 1]) + \
                Y[:, :, None, None, 2] * Wp[None, None, :, :, 2]
            tg = (Y[:, :, 0] * gp[0] + Y[:, :, 1] * gp[1]) + Y[:, :, 2] * gp[2]
            rows = (6 * cs[:, None] + np.arange(6)[None, :]).reshape(-1)
            T[np.ix_(rows, rows)] += Tb.reshape(len(rows), len(rows))
            Tg[rows] += tg.reshape(-1)
            b[rows] += bb.reshape(-1)
            for j, c in enumerate(cs):
                U[6 * c:6 * c + 6, 6 * c:6 * c + 6] += Ub[j]
        Ud = U.copy()
        Ud[np.diag_indices(N)] = Ud[np.diag_indices(N)] * lam1
        A = np.triu(Ud - T)
        A = A + np.triu(A, 1).T                                         # the upper triangle (row <= column) mirrored
        rhs = -(b - Tg)
    return _ldl_solve(A, rhs), ok, Vi, g, Wc, cam_of


def _candidate(W, cidx, free, P, X, d, ok, Vi, g, Wc, cam_of):
    Pn = P.copy()
    for c, f in enumerate(free):
        Pn[f] = cayley_update([float(v) for v in P[f]], [float(v) for v in d[6 * c:6 * c + 6]])
    with np.errstate(all="ignore"):
        Q = np.zeros_like(g)
        for v in range(MAXV):
            m = cam_of[:, v] >= 0
            dc = d.reshape(-1, 6)[np.maximum(cam_of[:, v], 0)]          # (NP, 6)
            Wv = Wc[:, v]                                               # (NP, 6, 3)
            dot = ((((Wv[:, 0] * dc[:, 0, None] + Wv[:, 1] * dc[:, 1, None]) + Wv[:, 2] * dc[:, 2, None]) + Wv[:, 3] * dc[:, 3, None]) +
                   Wv[:, 4] * dc[:, 4, None]) + Wv[:, 5] * dc[:, 5, None]
            Q = np.where(m[:, None], Q + dot, Q)
        s = -g - Q
        dX = np.stack([(Vi[:, k, 0] * s[:, 0] + Vi[:, k, 1] * s[:, 1]) + Vi[:, k, 2] * s[:, 2] for k in range(3)], -1)
        Xn = np.where(ok[:, None], X + dX, X)
    return Pn, Xn


def ba_rows(bp, cam, prev, nkp, obs, xy, poses, points=None, flags=None, log=None, stats=None):
    """obs: (n, row_cap) fr.OBS_DTYPE; xy: (n, row_cap, 2) float32; poses: (n, 12) float64.  points / flags: the buffers as they stand before the
    call (entries k >= nk(i), and everything when n <= 1, keep their bytes).  log: a list that receives (window, linearisation, what) with what in
    "accept", "reject", "pivot".  stats: a list that receives (window, linearisation, the number of used points that sat it out).
    Returns (poses_out (n, 12), windows, points (n, row_cap) POINT_DTYPE, flags (n, row_cap) uint8)."""
    n, R = obs.shape
    poses = np.ascontiguousarray(poses, np.float64).reshape(n, 12)
    out = poses.copy()
    points = np.zeros((n, R), POINT_DTYPE) if points is None else points.copy()
    flags = np.zeros((n, R), np.uint8) if flags is None else flags.copy()
    nw = n_windows(n, bp.stride)
    windows = np.zeros(nw, WINDOW_DTYPE)
    if nw == 0:
        return out, windows, points, flags
    nk = fr.counts(prev, nkp, R)
    posed = [fr.has_pose([float(v) for v in poses[i]]) for i in range(n)]
    tp = fr.TriParams(max_views=MAXV, min_views=bp.min_views, gn_iters=bp.tri_gn_iters, max_reproj_px=bp.init_reproj_px, max_parallax_cos=1.0)
    zero = np.zeros(1, POINT_DTYPE)[0]
    wpts = []                                                           # per window: (slots, X (NP, 3)) in the window's frame
    for j in range(nw):
        first = j * bp.stride
        last = min(first + bp.stride, n - 1)
        own0 = first + (1 if j > 0 else 0)
        anchor = next((i for i in range(first, last + 1) if posed[i]), -1)
        free = [i for i in range(anchor + 1, last + 1) if posed[i]] if anchor >= 0 else []
        lo = anchor if anchor >= 0 else first
        rec = windows[j]
        rec["first"], rec["last"], rec["anchor"], rec["n_free"] = first, last, anchor, len(free)
        rec["lambda_"], rec["scale"] = bp.lambda0, 1.0
        child = set()
        for i in range(own0 + 1, last + 1):
            for k in range(int(nk[i])):
                pq = _parent(prev, nk, obs, i, k, own0)
                if pq is not None:
                    child.add(pq)
        slots, views = [], []
        for i in range(own0, last + 1):
            for k in range(int(nk[i])):
                if (i, k) in child:
                    points[i, k], flags[i, k] = zero, 0
                    continue
                vw, cur = [], (i, k)
                for _ in range(MAXV):
                    f, kk = cur
                    u, v = float(xy[f, kk, 0]), float(xy[f, kk, 1])
                    if posed[f] and math.isfinite(u) and math.isfinite(v):
                        vw.append((f, u, v))
                    cur = _parent(prev, nk, obs, f, kk, lo)
                    if cur is None:
                        break
                pt = fr.triangulate_track(tp, cam, [([float(x) for x in poses[f]], u, v) for f, u, v in vw])
                fl = int(pt["flags"])
                r = zero.copy()
                r["n_views"] = pt["n_views"]
                if fl & fr.FTP_FEW:
                    r["flags"] = BAP_FEW
                elif fl & fr.FTP_SINGULAR or not (fl & fr.FTP_FRONT and fl & fr.FTP_REPROJ_OK):
                    r["flags"], r["rms0_px"] = BAP_INIT_REJECTED, pt["rms_reproj_px"]
                else:
                    r["flags"], r["X"], r["rms0_px"], r["rms1_px"] = BAP_USED, pt["X"], pt["rms_reproj_px"], pt["rms_reproj_px"]
                    slots.append((i, k))
                    views.append(vw)
                points[i, k], flags[i, k] = r, int(r["flags"])
        rec["n_points"], rec["n_obs"] = len(slots), sum(len(v) for v in views)
        W = _Window(first, slots, views)
        P = poses[first:last + 1].copy()
        X = np.array([points[s]["X"] for s in slots]).reshape(-1, 3)
        cur = _cost(W, _observe(cam, bp, W, P, X)) if slots else 0.0
        rec["cost0"] = rec["cost1"] = cur
        if not free or len(slots) < bp.min_points:
            rec["flags"] = BA_FEW
            wpts.append((slots, X))
            continue
        cidx = np.full(last - first + 1, -1, np.int64)
        for c, f in enumerate(free):
            cidx[f - first] = c
        lf = [f - first for f in free]
        lam, nacc, nrej = bp.lambda0, 0, 0
        for it in range(bp.lm_iters):
            d, ok, Vi, g, Wc, cam_of = _linearise(cam, bp, W, cidx, P, X, lam)
            what = "pivot"
            if d is not None:
                Pn, Xn = _candidate(W, cidx, lf, P, X, d, ok, Vi, g, Wc, cam_of)
                c = _cost(W, _observe(cam, bp, W, Pn, Xn))
                what = "accept" if math.isfinite(c) and c < cur else "reject"
            if what == "accept":
                P, X, cur = Pn, Xn, c
                lam, nacc = max(lam / 10.0, 1e-12), nacc + 1
            else:
                lam, nrej = min(10.0 * lam, 1e12), nrej + 1
            if log is not None:
                log.append((j, it, what))
            if stats is not None:
                stats.append((j, it, int((~ok).sum())))
        rec["n_lin"], rec["n_accepted"], rec["n_rejected"], rec["cost1"], rec["lambda_"] = bp.lm_iters, nacc, nrej, cur, lam
        rec["flags"] = BA_REFINED
        o = _observe(cam, bp, W, P, X)
        s2 = _ordered(W.pres, o["e2"])
        with np.errstate(all="ignore"):
            for p, s in enumerate(slots):
                points[s]["rms1_px"] = np.float32(math.sqrt(float(s2[p]) / float(len(views[p]))))
            if nacc > 0:
                ca, cin, cout = centre(poses[anchor]), centre(poses[free[-1]]), centre(P[lf[-1]])
                di, do = cin - ca, cout - ca
                scale = math.sqrt((di[0] * di[0] + di[1] * di[1]) + di[2] * di[2]) / np.float64(math.sqrt((do[0] * do[0] + do[1] * do[1]) + do[2] * do[2]))
                if not (math.isfinite(scale) and scale > 0.0):
                    rec["flags"] |= BA_NO_SCALE
                else:
                    rec["scale"] = scale
                    for f in lf:
                        c = ca + scale * (centre(P[f]) - ca)
                        for i in range(3):
                            P[f, 9 + i] = -((P[f, 3 * i] * c[0] + P[f, 3 * i + 1] * c[1]) + P[f, 3 * i + 2] * c[2])
                    X = ca[None, :] + scale * (X - ca[None, :])
        for f in free:
            out[f] = P[f - first]
        wpts.append((slots, X))
    # the stitch
    with np.errstate(all="ignore"):
        for j in range(nw):
            rec = windows[j]
            first, last, anchor = int(rec["first"]), int(rec["last"]), int(rec["anchor"])
            slots, X = wpts[j]
            if anchor < 0:
                continue
            Ain = poses[anchor]
            Aout = Ain
            if j > 0:
                if anchor != first:
                    rec["flags"] |= BA_RESTART
                else:
                    Aout = out[anchor].copy()
            if Aout.tobytes() != Ain.tobytes():
                Ri, ti, Ro, to = Ain[:9].reshape(3, 3), Ain[9:], Aout[:9].reshape(3, 3), Aout[9:]
                dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                for f in range(anchor + 1, last + 1):
                    if not posed[f]:
                        continue
                    Rw, tw = out[f][:9].reshape(3, 3), out[f][9:]
                    Rr = np.array([[dot(Rw[a], Ri[b]) for b in range(3)] for a in range(3)])
                    tr = np.array([tw[a] - dot(Rr[a], ti) for a in range(3)])
                    N = np.concatenate([np.array([[dot(Rr[a], Ro[:, b]) for b in range(3)] for a in range(3)]).reshape(9),
                                        np.array([dot(Rr[a], to) + tr[a] for a in range(3)])])
                    out[f] = N if np.isfinite(N).all() else poses[f]
                for p in range(len(slots)):
                    y = np.array([dot(Ri[a], X[p]) + ti[a] for a in range(3)]) - to
                    Z = np.array([dot(Ro[:, a], y) for a in range(3)])
                    if np.isfinite(Z).all():                            # (else the point stays in its window's frame)
                        X[p] = Z
            for p, s in enumerate(slots):
                points[s]["X"] = X[p]
    return out, windows, points, flags


# ---------------------------------------------------------------------------------------------- a planted scene as rows
def cay(w):
    h = np.asarray(w, float) / 2
    hh = h @ h
    hx = np.array([[0, -h[2], h[1]], [h[2], 0, -h[0]], [-h[1], h[0], 0]])
    return np.eye(3) + (2 / (1 + hh)) * (hx + (np.outer(h, h) - np.eye(3) * hh))


def scene(seed, cam, n_cam=24, n_pts=400, noise=0.3, span=(3, 12), rot_deg=0.3, tr=0.02):
    """The prototype's scene as rows: cameras on a gentle arc, points seen over span consecutive frames, pixels rounded to float; the input poses are
    the true ones perturbed per frame (frame 0 exact).  Returns dict(prev, nkp, obs, xy, truth (n, 12), poses (n, 12), row_cap)."""
    rng = np.random.default_rng(seed)
    Rs, ts = [], []
    for j in range(n_cam):
        a, b = 0.012 * j, 0.004 * math.sin(0.5 * j)
        R = cay([b, a, 0.3 * b])
        C = np.array([0.1 * j, 0.02 * math.sin(0.4 * j), 0.03 * j])
        Rs.append(R)
        ts.append(-R @ C)
    Xw = np.stack([rng.uniform(-2, 5, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 9, n_pts)], 1)
    rows = [[] for _ in range(n_cam)]                                   # per frame: (u, v, prev_kp)
    for p in range(n_pts):
        L = int(rng.integers(span[0], span[1] + 1))
        L = min(L, n_cam)
        s = int(rng.integers(0, n_cam - L + 1))
        pk = -1
        for j in range(s, s + L):
            xc = Rs[j] @ Xw[p] + ts[j]
            u = cam.fx * xc[0] / xc[2] + cam.cx + noise * rng.standard_normal()
            v = cam.fy * xc[1] / xc[2] + cam.cy + noise * rng.standard_normal()
            rows[j].append((np.float32(u), np.float32(v), pk))
            pk = len(rows[j]) - 1
    truth = np.array([np.concatenate([Rs[j].reshape(9), ts[j]]) for j in range(n_cam)])
    poses = truth.copy()
    for j in range(1, n_cam):
        Cc = cay(np.radians(rot_deg) * rng.standard_normal(3))
        d = tr * rng.standard_normal(3)
        poses[j, :9], poses[j, 9:] = (Cc @ Rs[j]).reshape(9), Cc @ ts[j] + d
    R = max(max(len(r) for r in rows), 1)
    R = (R + 7) // 8 * 8
    obs = np.zeros((n_cam, R), fr.OBS_DTYPE)
    obs[:] = fr.EMPTY_OBS
    xy = np.zeros((n_cam, R, 2), np.float32)
    for j, r in enumerate(rows):
        for k, (u, v, pk) in enumerate(r):
            xy[j, k] = (u, v)
            obs[j, k]["prev_kp"] = pk
    prev = np.array([fr.KF_FIRST] + list(range(n_cam - 1)), np.int32)
    nkp = np.array([len(r) for r in rows], np.int32)
    return dict(prev=prev, nkp=nkp, obs=obs, xy=xy, truth=truth, poses=poses, row_cap=R)


def relative_errors(poses, truth):
    """median frame-to-frame rotation error (degrees) and translation error"""
    er, et = [], []
    rel = lambda A, B: (A[:9].reshape(3, 3) @ B[:9].reshape(3, 3).T, A[9:] - A[:9].reshape(3, 3) @ B[:9].reshape(3, 3).T @ B[9:])
    for j in range(1, len(poses)):
        Rr, tr = rel(poses[j], poses[j - 1])
        R0, t0 = rel(truth[j], truth[j - 1])
        er.append(math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Rr @ R0.T) - 1) / 2)))))
        et.append(float(np.linalg.norm(tr - t0)))
    return float(np.median(er)), float(np.median(et))
