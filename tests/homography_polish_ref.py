"""The homography polish of include/vislam_hip.h (vis_homography_polish / _batch / vis_batch_homography_polish), restated operation for
operation: the start, the per-point residual and Jacobian, the 40 sums under the summation contract "T" (essential_polish_ref.tiled_sums,
imported, not copied), the gauge, the LDL^T solve for eight unknowns, the update, the re-selection and the rounds.  Not a test module: shared
by tests/test_homography_polish_abi.py, tests/test_homography_polish_ref.py (CPU) and tests/test_homography_polish_gpu.py.

The 3 x 3 work and the solve run on numpy float64 scalars (IEEE doubles, one rounding per operation, no contraction) in the kernel's
parenthesisation (csrc/homography_polish.hip); the per-point work is element-wise float64 numpy, which does not contract either.  The
transfer test and the adjugate are homography_ref's own."""
import ctypes as C

import numpy as np

import essential_polish_ref as epr
import homography_ref as hr

POLISHED, REJECTED, FEW, NO_MODEL, SHRANK = 1, 2, 4, 8, 16
DBL_MAX = 1.7976931348623157e308
F = np.float64
Q, P0, P1, T, G, COST, SUMS = 0, 6, 15, 24, 30, 39, 40                # where the sums live (csrc/homography_polish.hip: HQ_*)

RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("cost_first", "<f8"), ("cost0", "<f8"), ("cost1", "<f8"), ("n_points", "<i4"), ("n_set_first", "<i4"),
                         ("n_set_last", "<i4"), ("n_changed", "<i4"), ("rounds_run", "<i4"), ("steps_run", "<i4"), ("best_step", "<i4"),
                         ("flags", "<i4")])
assert RESULT_DTYPE.itemsize == 128


class Params(C.Structure):
    """vis_hpolish_params with its defaults, for callers without the library"""
    _fields_ = [("rounds", C.c_int32), ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("reserved_", C.c_int32), ("select_chi2", C.c_double),
                ("sigma_px", C.c_double)]


def default_params():
    return Params(3, 5, 8, 0, 5.991, 1.0)


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["flags"] = NO_MODEL
    return r


def _finite(v):
    return np.abs(v) <= DBL_MAX


def t_sel(cam, hp):
    """select_chi2 (sigma_px (1 / fx))^2 as the host computes it"""
    s = hp.sigma_px * (1.0 / cam.fx)
    return hp.select_chi2 * (s * s)


def one_wave_sums(terms):
    """the one-wave order (homography_ref.wave_sum) over per-point rows of terms (m x K): what a row of at most 64 points must also give"""
    return [hr.wave_sum(terms[:, k]) for k in range(terms.shape[1])]


def norm2(H):
    ss = H[0] * H[0]
    for k in range(1, 9):
        ss = ss + H[k] * H[k]
    return ss


def residual(H, x, y, x2, y2):
    """(u, v, ru, rv, q, finite) of the points under H: q = (a, b, iw)"""
    U = (H[0] * x + H[1] * y) + H[2]
    V = (H[3] * x + H[4] * y) + H[5]
    w = (H[6] * x + H[7] * y) + H[8]
    iw = 1.0 / w
    u, v = U * iw, V * iw
    ru, rv = u - x2, v - y2
    return u, v, ru, rv, [x * iw, y * iw, iw], _finite(iw) & _finite(u) & _finite(v) & _finite(ru) & _finite(rv)


def jacobian(H, x, y, x2, y2):
    """(J0, J1): the two rows of a point's Jacobian in the nine entries of H, each a list of nine arrays"""
    with np.errstate(all="ignore"):
        u, v, _, _, q, _ = residual(H, x, y, x2, y2)
        z = np.zeros(len(x))
        return q + [z, z, z] + [-(q[a] * u) for a in range(3)], [z, z, z] + q + [-(q[a] * v) for a in range(3)]


def gn_sums(H, x, y, x2, y2, setmask, sum_fn):
    """the 40 sums over the set at H"""
    with np.errstate(all="ignore"):
        u, v, ru, rv, q, fin = residual(H, x, y, x2, y2)
        inn = setmask & fin
        j0, j1 = [-(q[a] * u) for a in range(3)], [-(q[a] * v) for a in range(3)]
        cols = [q[a] * q[b] for a in range(3) for b in range(a, 3)]
        cols += [q[a] * j0[b] for a in range(3) for b in range(3)]
        cols += [q[a] * j1[b] for a in range(3) for b in range(3)]
        cols += [j0[a] * j0[b] + j1[a] * j1[b] for a in range(3) for b in range(a, 3)]
        cols += [q[a] * ru for a in range(3)] + [q[a] * rv for a in range(3)] + [j0[a] * ru + j1[a] * rv for a in range(3)]
        cols.append(ru * ru + rv * rv)
        terms = np.where(inn[:, None], np.stack(cols, 1), 0.0) if len(x) else np.zeros((0, SUMS))
        return [F(s) for s in sum_fn(terms)]


def entry(S, a, b):
    """entry (a, b) of the symmetric 9 x 9 matrix of the sums"""
    if a > b:
        a, b = b, a
    ba, bb, ia, ib = a // 3, b // 3, a % 3, b % 3
    if ba == 0 and bb == 1:
        return F(0.0)
    if ba == bb:
        return S[(T if ba == 2 else Q) + (ib if ia == 0 else 2 + ib if ia == 1 else 5)]
    return S[(P0 if ba == 0 else P1) + 3 * ia + ib]


def gauge(H):
    """the index of the largest |H_k|, the lowest on a tie"""
    p, am = 0, abs(H[0])
    for k in range(1, 9):
        if abs(H[k]) > am:
            p, am = k, abs(H[k])
    return p


def solve(S, p):
    """(dH[9], ok): row and column p struck, d = -A^-1 g of the eight others by LDL^T without pivoting (pnp_ref.solve6 for eight), dH[p] = 0"""
    idx = [k for k in range(9) if k != p]
    n = 8
    A = [[entry(S, idx[i], idx[j]) for j in range(n)] for i in range(n)]
    g = [S[G + idx[i]] for i in range(n)]
    L, D, z, d = [[F(0.0)] * n for _ in range(n)], [F(0.0)] * n, [F(0.0)] * n, [F(0.0)] * n
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            s = F(A[j][j])
            for c in range(j):
                s = s - (L[j][c] * L[j][c]) * D[c]
            D[j] = s
            ok = ok and bool(s > 0.0) and bool(_finite(s))
            for i in range(j + 1, n):
                v = F(A[i][j])
                for c in range(j):
                    v = v - (L[i][c] * L[j][c]) * D[c]
                L[i][j] = v / s
        for i in range(n):
            v = F(-g[i])
            for c in range(i):
                v = v - L[i][c] * z[c]
            z[i] = v
        for i in range(n - 1, -1, -1):
            v = z[i] / D[i]
            for c in range(i + 1, n):
                v = v - L[c][i] * d[c]
            d[i] = v
    dH = [F(0.0)] * 9
    for i, k in enumerate(idx):
        dH[k] = d[i]
    return dH, ok


def step(H, S):
    """(H after one update, ok): the gauge, the solve, H_k + d for k != p, the norm renewed"""
    p = gauge(H)
    dH, ok = solve(S, p)
    if not ok:
        return H, False
    with np.errstate(all="ignore"):
        H = [H[k] if k == p else H[k] + dH[k] for k in range(9)]
        nn = np.sqrt(norm2(H))
        return [h / nn for h in H], True


def select(H, x, y, x2, y2, t):
    """the points of the whole row that pass the two-sided transfer test at t under H and G = adj(H), with t (w w) finite in both directions"""
    with np.errstate(all="ignore"):
        Gm = hr.adj(H)
        e, ww = hr.transfer(H, x, y, x2, y2)
        rf = t * ww
        f = _finite(rf) & (e <= rf)
        e, ww = hr.transfer(Gm, x2, y2, x, y)
        rb = t * ww
        return f & _finite(rb) & (e <= rb)


def _round(H, x, y, x2, y2, setmask, passes, sum_fn):
    """passes 0 ... passes over the set from H: (Hb, cost0, cost1, best, steps)"""
    cost0 = cost1 = F(0.0)
    best = steps = 0
    Hb = H
    for k in range(passes + 1):
        S = gn_sums(H, x, y, x2, y2, setmask, sum_fn)
        cost = S[COST]
        if k == 0:
            cost0 = cost
        if k == 0 or (bool(_finite(cost)) and (not bool(_finite(cost1)) or bool(cost < cost1))):
            cost1, best, Hb = cost, k, list(H)
        if k == passes:
            break
        H, ok = step(H, S)
        if not ok:
            break
        steps += 1
    return Hb, cost0, cost1, best, steps


def polish(cam, hp, hrec, x1, x2, mask=None, sets=None, sum_fn=None):
    """(RESULT_DTYPE record, output mask of m bytes or None when the row is left untouched, the homography record h_out); hrec: the input
    homography record (homography_ref.RESULT_DTYPE); x1 / x2: the row's m valid points; mask: m bytes or None; sets: a list that receives every
    set that was current, as bool arrays; sum_fn: the order of the sums (contract T when absent)"""
    sum_fn = epr.tiled_sums if sum_fn is None else sum_fn
    x1 = np.asarray(x1, np.float32).reshape(-1, 2)
    x2 = np.asarray(x2, np.float32).reshape(-1, 2)
    m = len(x1)
    h_out = np.frombuffer(np.asarray(hrec).tobytes(), hr.RESULT_DTYPE)[0].copy()
    H = [F(v) for v in np.asarray(hrec["H"], np.float64).reshape(9)]
    with np.errstate(all="ignore"):
        ss = norm2(H)
        if int(hrec["best_iter"]) < 0 or not all(bool(_finite(v)) for v in H) or not bool(ss > 0.0) or not bool(_finite(ss)):
            return zero_record(), None, h_out
        n0 = np.sqrt(ss)
        H = [h / n0 for h in H]
        x, y, u2, v2 = hr.normalise(cam, x1, x2)
    cur = np.ones(m, bool) if mask is None else np.asarray(mask).reshape(-1)[:m] != 0
    nfirst = int(cur.sum())
    t = t_sel(cam, hp)
    run = nfirst >= hp.min_inliers
    passes, rounds = (int(hp.refine_iters), int(hp.rounds)) if run else (0, 0)
    Hb = H
    cost_first = cost0 = cost1 = F(0.0)
    best = steps = rounds_run = nchg = 0
    shrank = moved = False
    if sets is not None:
        sets.append(cur.copy())
    for k in range(rounds + 1):
        if k > 0:
            new = select(Hb, x, y, u2, v2, t)
            nchg = int((new != cur).sum())
            if nchg == 0:
                break
            if int(new.sum()) < hp.min_inliers:
                shrank = True
                break
            cur = new
            if sets is not None:
                sets.append(cur.copy())
        Hb, cost0, cost1, best, st = _round(Hb, x, y, u2, v2, cur, passes, sum_fn)
        if k == 0:
            cost_first = cost0
        steps += st
        rounds_run += int(run)
        moved = moved or best > 0
    with np.errstate(all="ignore"):
        Gm = hr.adj(Hb)
        det = (Hb[0] * Gm[0] + Hb[1] * Gm[3]) + Hb[2] * Gm[6]
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["H"] = [-h for h in Hb] if bool(det < 0.0) else Hb
    r["cost_first"], r["cost0"], r["cost1"] = cost_first, cost0, cost1
    r["n_points"], r["n_set_first"], r["n_set_last"], r["n_changed"] = m, nfirst, int(cur.sum()), nchg
    r["rounds_run"], r["steps_run"], r["best_step"] = rounds_run, steps, best
    r["flags"] = ((POLISHED if moved else REJECTED) if run else FEW) | (SHRANK if shrank else 0)
    h_out["H"], h_out["n_inliers"] = r["H"], r["n_set_last"]
    return r, cur.astype(np.uint8), h_out


def polish_rows(cam, hp, hrecs, p1, p2, npts, mask, mask_out):
    """the batch: hrecs = n homography records, p1 / p2 = n x max_pts x 2, npts clamped to 0 ... max_pts, mask = n x row_cap bytes or None;
    mask_out = n x row_cap bytes as they were before the call -> (records, mask_out afterwards, homography records)"""
    n, max_pts = len(npts), p1.shape[1]
    out, mo, ho = np.zeros(n, RESULT_DTYPE), mask_out.copy(), np.zeros(n, hr.RESULT_DTYPE)
    for i in range(n):
        m = min(max(int(npts[i]), 0), max_pts)
        out[i], row, ho[i] = polish(cam, hp, hrecs[i], p1[i, :m], p2[i, :m], None if mask is None else mask[i, :m])
        if row is not None:
            mo[i, :m] = row
    return out, mo, ho
