"""Restatement of the trajectory contract of include/vislam_hip.h (not a test module; nothing here calls the code under test).

Plain Python floats (IEEE binary64, one rounding per + - *, nothing contracted, no division), the parenthesisation of the header.

  trajectory_rows    vis_trajectory_rows: the device's own scheme -- one element per frame, ceil(log2 n) rounds of pointer doubling, each from the
                     state of the round before -- (records (n) TRAJ_DTYPE, d_poses (n, 12))
  sequential_rows    the same records by plain left-to-right composition (frame i from the finished record of its parent): what the doubling is
                     compared with, and what two cuts of a stream differ by
  carry_out          the record the plan keeps for the next launch"""
import math

import numpy as np

from scale_link_ref import KF_CARRIED, KF_FIRST, KF_NOT_SAVED, SL_OK, norm_prev, pose_usable

TJ_ROOT, TJ_NO_POSE, TJ_NO_CARRY, TJ_NOT_SAVED, TJ_UNIT_EDGE, TJ_OVERFLOW = 1, 2, 4, 8, 16, 32
TJ_MAX_FRAMES, TJ_LDS_N = 1024, 256
TRAJ_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("sigma", "<f8"), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("hops", "<i4"),
                       ("unit_edges", "<i4"), ("parent", "<i4"), ("flags", "<i4")])
CARRY = -1
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def carry_ok(carry):
    return carry is not None and not int(carry["flags"]) & (TJ_NOT_SAVED | TJ_OVERFLOW)


def has_parent(prev, i, have_carry):
    p = norm_prev(prev, i)
    return norm_prev(prev, p) != KF_NOT_SAVED if p >= 0 else (p == KF_CARRIED and have_carry)


def is_edge(prev, pose, i, have_carry):
    return norm_prev(prev, i) != KF_NOT_SAVED and has_parent(prev, i, have_carry) and pose_usable(pose[i]["R"], pose[i]["t"])


def mul(R1, R2):
    return [(R1[3 * r] * R2[c] + R1[3 * r + 1] * R2[3 + c]) + R1[3 * r + 2] * R2[6 + c] for r in range(3) for c in range(3)]


def apply(R1, U2, S2, U1):
    """R1 U2 + S2 U1"""
    return [((R1[3 * r] * U2[0] + R1[3 * r + 1] * U2[1]) + R1[3 * r + 2] * U2[2]) + S2 * U1[r] for r in range(3)]


def compose(s, a):
    """path s (i -> m) followed by path a (m -> a's ancestor)"""
    return dict(S=s["S"] * a["S"], R=mul(s["R"], a["R"]), U=apply(s["R"], a["U"], a["S"], s["U"]), anc=a["anc"], hops=s["hops"] + a["hops"],
                units=s["units"] + a["units"], epoch=s["epoch"] if s["units"] > 0 else a["epoch"])


def elements(prev, pose, link, have_carry, seq0, carry=None):
    """per frame (state, flags, parent): a root or a frame that was not saved is its own, final ancestor"""
    out = []
    for i in range(len(prev)):
        p = norm_prev(prev, i)
        s = dict(S=1.0, R=list(IDENTITY), U=[0.0, 0.0, 0.0], anc=i, hops=0, units=0, epoch=seq0 + i)
        f = 0
        if p == KF_NOT_SAVED:
            f = TJ_NOT_SAVED
        elif not is_edge(prev, pose, i, have_carry):
            f = TJ_ROOT | (TJ_NO_POSE if has_parent(prev, i, have_carry) else TJ_NO_CARRY if p == KF_CARRIED else 0)
        else:
            sc = float(link[i]["scale"])
            below_root = not is_edge(prev, pose, p, have_carry) if p >= 0 else bool(int(carry["flags"]) & TJ_ROOT)
            ok = int(link[i]["flags"]) == SL_OK and math.isfinite(sc) and sc > 0.0 and not below_root
            if not ok:
                sc, f = 1.0, TJ_UNIT_EDGE
            s = dict(S=sc, R=[float(v) for v in pose[i]["R"]], U=[sc * float(v) for v in pose[i]["t"]], anc=p if p >= 0 else CARRY, hops=1,
                     units=0 if ok else 1, epoch=seq0 + i)
        out.append((s, f, p))
    return out


def zero_record(flags):
    r = np.zeros(1, TRAJ_DTYPE)[0]
    r["flags"] = flags
    return r


def finish(s, f, p, carry, seq0):
    """the record of a frame whose state s is final"""
    if f & TJ_NOT_SAVED:
        return zero_record(TJ_NOT_SAVED)
    if s["anc"] == CARRY:
        Rc, tc, sc = [float(v) for v in carry["R"]], [float(v) for v in carry["t"]], float(carry["sigma"])
        R, t, sigma = mul(s["R"], Rc), apply(s["R"], tc, sc, s["U"]), sc * s["S"]
        seg, epoch = int(carry["segment_seq"]), s["epoch"] if s["units"] > 0 else int(carry["epoch_seq"])
        hops, units = int(carry["hops"]) + s["hops"], int(carry["unit_edges"]) + s["units"]
    else:
        R, t, sigma = s["R"], s["U"], s["S"]
        seg, epoch = seq0 + s["anc"], s["epoch"] if s["units"] > 0 else seq0 + s["anc"]
        hops, units = s["hops"], s["units"]
    if not (all(math.isfinite(v) for v in R + t) and math.isfinite(sigma) and sigma > 0.0):
        return zero_record(TJ_OVERFLOW)
    r = zero_record(f)
    r["R"], r["t"], r["sigma"] = R, t, sigma
    r["segment_seq"], r["epoch_seq"], r["hops"], r["unit_edges"], r["parent"] = seg, epoch, np.int32(hops), np.int32(units), p
    return r


def dense_poses(rec, same_epoch_only):
    n = len(rec)
    poses = np.zeros((n, 12))
    valid = [i for i in range(n) if not int(rec[i]["flags"]) & (TJ_NOT_SAVED | TJ_OVERFLOW)]
    if valid:
        f = "epoch_seq" if same_epoch_only else "segment_seq"
        key = int(rec[valid[-1]][f])
        for i in valid:
            if int(rec[i][f]) == key:
                poses[i, :9], poses[i, 9:] = rec[i]["R"], rec[i]["t"]
    return poses


def trajectory_rows(prev, pose, link, carry=None, seq0=0, same_epoch_only=True):
    """prev: n; pose: n POSE_DTYPE; link: n LINK_DTYPE; carry: None or one TRAJ_DTYPE element.  Returns (records (n) TRAJ_DTYPE, d_poses (n, 12))."""
    n = len(prev)
    have = carry_ok(carry)
    el = elements(prev, pose, link, have, seq0, carry)
    st = [e[0] for e in el]
    reach = 1
    while reach < n:                                                # every round from the state of the round before
        new = list(st)
        for i in range(n):
            a = st[i]["anc"]
            if a < 0 or a == i or st[a]["anc"] == a:
                continue
            new[i] = compose(st[i], st[a])
        st = new
        reach *= 2
    rec = np.zeros(n, TRAJ_DTYPE)
    for i in range(n):
        rec[i] = finish(st[i], el[i][1], el[i][2], carry, seq0)
    return rec, dense_poses(rec, same_epoch_only)


def sequential_rows(prev, pose, link, carry=None, seq0=0):
    """the records by composing every edge onto the finished record of its parent, in frame order (mathematically the same chain)"""
    n = len(prev)
    have = carry_ok(carry)
    el = elements(prev, pose, link, have, seq0, carry)
    rec = np.zeros(n, TRAJ_DTYPE)
    for i in range(n):
        s, f, p = el[i]
        if f & TJ_NOT_SAVED or s["anc"] == i:
            rec[i] = finish(s, f, p, carry, seq0)
            continue
        par = carry if s["anc"] == CARRY else rec[s["anc"]]
        if int(par["flags"]) & TJ_OVERFLOW:
            rec[i] = zero_record(TJ_OVERFLOW)
            continue
        rec[i] = finish(dict(s, anc=CARRY), f, p, par, seq0)        # the parent's finished record plays the carried record's part
    return rec


def carry_out(prev, rec, carry):
    """the record the plan keeps for the next launch: that of the last saved frame, else the one it was given, else none"""
    saved = [i for i in range(len(prev)) if norm_prev(prev, i) != KF_NOT_SAVED]
    if saved:
        return rec[saved[-1]].copy()
    return carry.copy() if carry is not None else zero_record(TJ_NOT_SAVED)
