"""The two-view polish of include/vislam_hip.h (vis_essential_polish / _batch / vis_batch_essential_polish), restated on the functions of
tests/essential_refine_ref.py: the start, the passes, the solve and the updates are that module's own (imported, not copied); what is new here is
the summation contract "T", the re-selection of the set and the rounds.  Not a test module: shared by tests/test_essential_polish_abi.py,
tests/test_essential_polish_ref.py (CPU) and tests/test_essential_polish_gpu.py.

Contract T: 256 partial sums over i mod 256 in rising i from +0.0; W_w = the butterfly v = v + v[lane ^ off], off = 32 ... 1, over the partial
sums 64 w ... 64 w + 63; the sum is ((W_0 + W_1) + W_2) + W_3.  essential_refine_ref.gn_pass takes its sums through pnp_ref.wave_sums; tiled()
puts tiled_sums in that place for the length of a polish and takes it out again, so nothing else of the pass is restated."""
import contextlib
import ctypes as C

import numpy as np

import essential_refine_ref as er

POLISHED, REJECTED, FEW, NO_POSE, SHRANK = 1, 2, 4, 8, 16
F = np.float64

RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("E", "<f8", (9,)), ("cost_first", "<f8"), ("cost0", "<f8"), ("cost1", "<f8"),
                         ("n_points", "<i4"), ("n_set_first", "<i4"), ("n_set_last", "<i4"), ("n_changed", "<i4"), ("rounds_run", "<i4"),
                         ("steps_run", "<i4"), ("best_step", "<i4"), ("flags", "<i4")])
assert RESULT_DTYPE.itemsize == 224
POSE_DTYPE = np.dtype([("E", "<f8", (9,)), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_inliers", "<i4"), ("n_pose_good", "<i4"), ("iters_run", "<i4"),
                       ("n_points", "<i4"), ("n_models", "<i4"), ("undecided_max", "<i4")])
assert POSE_DTYPE.itemsize == 192


class Params(C.Structure):
    """vis_epolish_params with its defaults, for callers without the library"""
    _fields_ = [("rounds", C.c_int32), ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("reserved_", C.c_int32), ("select_px", C.c_double),
                ("reserved2_", C.c_int32 * 2)]


def default_params():
    return Params(3, 5, 8, 0, 2.0)


def zero_record():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["flags"] = NO_POSE
    return r


def tiled_sums(terms):
    """contract T over per-point rows of terms (m x K): K sums"""
    n, K = terms.shape
    pad = np.zeros((((n + 255) // 256) * 256, K))
    pad[:n] = terms
    acc = np.zeros((256, K))
    for blk in pad.reshape(-1, 256, K):
        acc = acc + blk
    lane = np.arange(64)
    W = []
    for w in range(4):
        v = acc[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ off]
        W.append(v[0])
    return [float(v) for v in ((W[0] + W[1]) + W[2]) + W[3]]


@contextlib.contextmanager
def tiled():
    """essential_refine_ref's passes summed under contract T"""
    keep = er.pr.wave_sums
    er.pr.wave_sums = tiled_sums
    try:
        yield
    finally:
        er.pr.wave_sums = keep


def select(cam, R, t, a, b, c, d, thr2):
    """the points of the whole row that pass under the pose: thr2 den finite and s s <= thr2 den (gn_pass's count, point for point)"""
    with np.errstate(all="ignore"):
        l0, l1, m0, m1, s = er.apply(er.xmat(t, R), a, b, c, d)
        den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        rhs = thr2 * den
        return (np.abs(rhs) <= er.DBL_MAX) & (s * s <= rhs)


def _round(R, t, a, b, c, d, setmask, thr2, passes):
    """vis_essential_refine's passes 0 ... passes over the set from (R, t): (Rb, tb, cost0, cost1, best, steps) -- the loop of
    essential_refine_ref.refine, which cannot be called for it: it would normalise t again"""
    cost0 = cost1 = F(0.0)
    best = steps = 0
    Rb, tb = R, t
    for step in range(passes + 1):
        S, _ = er.gn_pass(R, t, a, b, c, d, setmask, thr2)
        cost = S[20]
        if step == 0:
            cost0 = cost
        if step == 0 or (er._finite(cost) and (not er._finite(cost1) or bool(cost < cost1))):
            cost1, best, Rb, tb = cost, step, list(R), list(t)
        if step == passes:
            break
        dlt, ok = er.solve5(S)
        if not ok:
            break
        R = er.rotate(R, dlt[:3])
        t = er.move_t(t, dlt[3], dlt[4])
        steps += 1
    return Rb, tb, cost0, cost1, best, steps


def polish(cam, ep, R, t, x1, x2, mask=None, pose_in=None, sets=None):
    """(RESULT_DTYPE record, output mask of m bytes or None when the row is left untouched, POSE_DTYPE record); x1 / x2: the row's m valid points;
    mask: m bytes or None; pose_in: the input pose record (None: zero but for R, t and n_points = m); sets: a list that receives every set
    that was current, as bool arrays"""
    x1 = np.asarray(x1, np.float32).reshape(-1, 2)
    x2 = np.asarray(x2, np.float32).reshape(-1, 2)
    m = len(x1)
    if pose_in is None:
        pose_in = np.zeros(1, POSE_DTYPE)[0]
        pose_in["R"], pose_in["t"], pose_in["n_points"] = np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), m
    pose = pose_in.copy()
    R = [F(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = [F(v) for v in np.asarray(t, np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        tt = er.pr._dot3(t, t)
        if not any(v != 0.0 for v in R) or not all(er._finite(v) for v in R + t) or not bool(tt > 0.0) or not er._finite(tt):
            return zero_record(), None, pose
        nt = np.sqrt(tt)
        t = [t[0] / nt, t[1] / nt, t[2] / nt]
    a, b = er.pr.normalise(cam, x1)
    c, d = er.pr.normalise(cam, x2)
    cur = np.ones(m, bool) if mask is None else np.asarray(mask).reshape(-1)[:m] != 0
    nfirst = int(cur.sum())
    thr = F(ep.select_px) / F(cam.fx)
    thr2 = thr * thr
    run = nfirst >= ep.min_inliers
    passes, rounds = (int(ep.refine_iters), int(ep.rounds)) if run else (0, 0)
    Rb, tb = R, t
    cost_first = cost0 = cost1 = F(0.0)
    best = steps = rounds_run = nchg = 0
    shrank = moved = False
    if sets is not None:
        sets.append(cur.copy())
    with tiled():
        for k in range(rounds + 1):
            if k > 0:
                new = select(cam, Rb, tb, a, b, c, d, thr2)
                nchg = int((new != cur).sum())
                if nchg == 0:
                    break
                if int(new.sum()) < ep.min_inliers:
                    shrank = True
                    break
                cur = new
                if sets is not None:
                    sets.append(cur.copy())
            Rb, tb, cost0, cost1, best, st = _round(Rb, tb, a, b, c, d, cur, thr2, passes)
            if k == 0:
                cost_first = cost0
            steps += st
            rounds_run += int(run)
            moved = moved or best > 0
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["R"], r["t"], r["E"] = Rb, tb, er.xmat(tb, Rb)
    r["cost_first"], r["cost0"], r["cost1"] = cost_first, cost0, cost1
    r["n_points"], r["n_set_first"], r["n_set_last"], r["n_changed"] = m, nfirst, int(cur.sum()), nchg
    r["rounds_run"], r["steps_run"], r["best_step"] = rounds_run, steps, best
    r["flags"] = ((POLISHED if moved else REJECTED) if run else FEW) | (SHRANK if shrank else 0)
    pose["E"], pose["R"], pose["t"], pose["n_inliers"] = r["E"], r["R"], r["t"], r["n_set_last"]
    return r, cur.astype(np.uint8), pose


def polish_rows(cam, ep, poses, p1, p2, npts, mask, mask_out):
    """the batch: poses = n POSE_DTYPE records, p1 / p2 = n x max_pts x 2, npts clamped to 0 ... max_pts, mask = n x row_cap bytes or None;
    mask_out = n x row_cap bytes as they were before the call -> (records, mask_out afterwards, pose records)"""
    n, max_pts = len(npts), p1.shape[1]
    out, mo, po = np.zeros(n, RESULT_DTYPE), mask_out.copy(), np.zeros(n, POSE_DTYPE)
    for i in range(n):
        m = min(max(int(npts[i]), 0), max_pts)
        out[i], row, po[i] = polish(cam, ep, poses[i]["R"], poses[i]["t"], p1[i, :m], p2[i, :m], None if mask is None else mask[i, :m], poses[i])
        if row is not None:
            mo[i, :m] = row
    return out, mo, po
