"""The bias Jacobians of the IMU deltas and the first-order bias correction of include/vislam_hip.h restated operation for operation in plain
Python floats (IEEE doubles, no contraction), on top of tests/imu_ref.py: the sub-step, the composition, the lifting table, the pair records, the
carry and the correction.  vis_imu_preintegrate_jac_rows equals preintegrate_jac_rows() and vis_imu_correct_rows equals correct_rows() byte for
byte; the delta part is imu_ref's by construction of the same operations and is asserted to be (tests/test_imu_jac_ref.py)."""
import numpy as np

import imu_ref as ir

IMU_JAC_OK, IMU_JAC_NONFINITE = 0, 1
IMC_OK, IMC_UNUSABLE, IMC_JAC, IMC_BIAS, IMC_ANGLE, IMC_NONFINITE = 0, 1, 2, 4, 8, 16
VOID_FLAGS = ir.IMU_NO_PAIR | ir.IMU_NO_CARRY | ir.IMU_NO_START | ir.IMU_NONFINITE
BLOCKS = ("Jvg", "Jva", "Jpg", "Jpa")

JAC_DTYPE = np.dtype([("Jvg", "<f8", (9,)), ("Jva", "<f8", (9,)), ("Jpg", "<f8", (9,)), ("Jpa", "<f8", (9,)), ("flags", "<i4"), ("q", "<i4")])
JAC_CARRY_DTYPE = np.dtype([("carry", ir.CARRY_DTYPE), ("open_jac", JAC_DTYPE)])


class Jac:
    __slots__ = ("vg", "va", "pg", "pa", "flags")

    def __init__(self):
        self.vg, self.va, self.pg, self.pa, self.flags = [0.0] * 9, [0.0] * 9, [0.0] * 9, [0.0] * 9, 0

    def copy(self):
        q = Jac()
        q.vg, q.va, q.pg, q.pa, q.flags = list(self.vg), list(self.va), list(self.pg), list(self.pa), self.flags
        return q

    def numbers(self):
        return self.vg + self.va + self.pg + self.pa


def skmul(u, M):
    """[u]x M"""
    return [u[1] * M[6 + c] - u[2] * M[3 + c] for c in range(3)] + [u[2] * M[c] - u[0] * M[6 + c] for c in range(3)] + \
           [u[0] * M[3 + c] - u[1] * M[c] for c in range(3)]


def settle(d, q):
    """the rule every Jacobian record ends on: zero beside a voided delta or a flagged record; not finite beside a finite delta: zero and flagged"""
    zero = bool(d.flags & VOID_FLAGS) or bool(q.flags & IMU_JAC_NONFINITE)
    if not zero and not all(ir.finite(x) for x in q.numbers()):
        q.flags |= IMU_JAC_NONFINITE
        zero = True
    if zero:
        q.vg, q.va, q.pg, q.pa = [0.0] * 9, [0.0] * 9, [0.0] * 9, [0.0] * 9
    return q


def substep(d, q, P, s0, s1):
    """imu_ref.substep with the four Jacobians; the delta's operations are the same ones in the same order"""
    h = s1[0] - s0[0]
    if not h > 0.0:
        d.flags |= ir.IMU_ORDER
        return
    d.n_steps += 1
    if h > P.max_gap_s:
        d.flags |= ir.IMU_GAP
    phi = [(0.5 * (s0[1][k] + s1[1][k]) - P.bg[k]) * h for k in range(3)]
    dR, Jr, th2 = ir.exp_and_jr(phi)
    if th2 > P.max_angle * P.max_angle:
        d.flags |= ir.IMU_FAST
    Rn = ir.mul(d.R, dR)
    u0, u1 = [s0[2][k] - P.ba[k] for k in range(3)], [s1[2][k] - P.ba[k] for k in range(3)]
    r0, r1 = ir.mulv(d.R, u0), ir.mulv(Rn, u1)
    for r in range(3):
        am = 0.5 * (r0[r] + r1[r])
        d.p[r] = d.p[r] + (d.v[r] * h + (0.5 * am) * (h * h))
        d.v[r] = d.v[r] + am * h
    M = ir.tmul(dR, d.J)
    Jn = [M[k] - Jr[k] * h for k in range(9)]
    G0, G1 = ir.mul(d.R, skmul(u0, d.J)), ir.mul(Rn, skmul(u1, Jn))
    for k in range(9):
        Dg, Da = -0.5 * (G0[k] + G1[k]), -0.5 * (d.R[k] + Rn[k])
        q.pg[k] = q.pg[k] + (q.vg[k] * h + (0.5 * Dg) * (h * h))
        q.vg[k] = q.vg[k] + Dg * h
        q.pa[k] = q.pa[k] + (q.va[k] * h + (0.5 * Da) * (h * h))
        q.va[k] = q.va[k] + Da * h
    d.J = Jn
    d.R = Rn


def interval(P, S, ts, ta, tb):
    """imu_ref.interval with the Jacobians: (delta, jac)"""
    d, q = ir.Delta(), Jac()
    if ta is None:
        d.flags = ir.IMU_NO_START
        return d, q
    d.dt = tb - ta
    if not ir.finite(d.dt):
        d.dt = 0.0
    bad = not ir.finite(ta) or not ir.finite(tb)
    if not bad and len(ts) < 1:
        d.flags |= ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED
    if not bad and len(ts) >= 1:
        pa = ir._value(S, ts, ta, d)
        bad = pa is None
        if not bad:
            pb = ir._value(S, ts, tb, d)
            bad = pb is None
        lo, hi = ir._ub(ts, ta), ir._lb(ts, tb)
        if not bad:
            if hi <= lo:
                d.flags |= ir.IMU_EMPTY
            bad = not all(ir._point_finite(S[j]) for j in range(lo, hi))
        if not bad:
            cur = pa
            for j in range(lo, hi):
                substep(d, q, P, cur, S[j])
                cur = S[j]
            substep(d, q, P, cur, pb)
    if bad or not all(ir.finite(x) for x in d.numbers()):
        d = ir.void(d)
    return d, settle(d, q)


def compose(X, Y):
    """(X.delta, X.jac) o (Y.delta, Y.jac), X the earlier: imu_ref.compose for the delta, then the four blocks"""
    (Xd, Xq), (Yd, Yq) = X, Y
    O = ir.compose(Xd, Yd)
    q = Jac()
    q.flags = Xq.flags | Yq.flags
    Wv, Wp = ir.mul(Xd.R, skmul(Yd.v, Xd.J)), ir.mul(Xd.R, skmul(Yd.p, Xd.J))
    Rpa, Rva, Rpg, Rvg = ir.mul(Xd.R, Yq.pa), ir.mul(Xd.R, Yq.va), ir.mul(Xd.R, Yq.pg), ir.mul(Xd.R, Yq.vg)
    q.pa = [(Xq.pa[k] + Xq.va[k] * Yd.dt) + Rpa[k] for k in range(9)]
    q.va = [Xq.va[k] + Rva[k] for k in range(9)]
    q.pg = [((Xq.pg[k] + Xq.vg[k] * Yd.dt) + Rpg[k]) - Wp[k] for k in range(9)]
    q.vg = [(Xq.vg[k] + Rvg[k]) - Wv[k] for k in range(9)]
    return O, settle(O, q)


def _copy(e):
    return e[0].copy(), e[1].copy()


def lifting_table(T0, max_len):
    T = [list(T0)]
    n, k = len(T0), 1
    while (1 << k) <= max_len:
        half = 1 << (k - 1)
        T.append([compose(T[k - 1][i - half], T[k - 1][i]) if i >= (1 << k) - 1 else None for i in range(n)])
        k += 1
    return T


def lift(T, i, L):
    pos, acc, k = i, None, 0
    while (1 << k) <= L:
        if L & (1 << k):
            acc = _copy(T[k][pos]) if acc is None else compose(T[k][pos], acc)
            pos -= 1 << k
        k += 1
    return acc


def sequential(T0, i, L):
    """the same intervals composed left to right"""
    acc = _copy(T0[i - L + 1])
    for j in range(i - L + 2, i + 1):
        acc = compose(acc, T0[j])
    return acc


def _carry_parts(carry):
    """(t_last or None, (open delta, open jac) or None) of a JAC_CARRY record or None"""
    if carry is None:
        return None, None
    c = np.asarray(carry, JAC_CARRY_DTYPE).reshape(-1)[0]
    t_last, o = ir._carry_parts(c["carry"])
    if o is None:
        return t_last, None
    q, r = Jac(), c["open_jac"]
    q.vg, q.va, q.pg, q.pa = ([float(x) for x in r[f]] for f in BLOCKS)
    q.flags = int(r["flags"])
    return t_last, (o, q)


def _record(out, q, prev):
    out["Jvg"], out["Jva"], out["Jpg"], out["Jpa"], out["flags"], out["q"] = q.vg, q.va, q.pg, q.pa, q.flags, prev


def intervals(P, samples, tframe, carry=None):
    S, ts = ir._samples(samples)
    t_last, _ = _carry_parts(carry)
    tf = [float(t) for t in tframe]
    return [interval(P, S, ts, tf[i - 1] if i > 0 else t_last, tf[i]) for i in range(len(tf))]


def preintegrate_jac_rows(P, samples, tframe, prev, carry=None, gather=lift):
    """(d_delta (n), d_jac (n), d_rot (n, 9) float32, d_carry_out) of vis_imu_preintegrate_jac_rows; gather=sequential: the left-to-right order"""
    n = len(tframe)
    t_last, c_open = _carry_parts(carry)
    have_carry = t_last is not None
    T0 = intervals(P, samples, tframe, carry)
    pv = [ir.norm_prev(prev, i) for i in range(n)]
    lens = [i - p if p >= 0 else (i + 1 if p == ir.KF_CARRIED and have_carry else 0) for i, p in enumerate(pv)]
    saved = [i for i in range(n) if pv[i] != ir.KF_NOT_SAVED]
    last = saved[-1] if saved else -1
    Lc = n - 1 - last if last >= 0 else n
    T = lifting_table(T0, max(lens + [Lc])) if gather is lift else T0
    delta, jac, rot = np.zeros(n, ir.DELTA_DTYPE), np.zeros(n, JAC_DTYPE), np.zeros((n, 9), np.float32)
    for i, p in enumerate(pv):
        d, q = ir.Delta(), Jac()
        if p in (ir.KF_NOT_SAVED, ir.KF_FIRST):
            d.flags = ir.IMU_NO_PAIR
        elif p == ir.KF_CARRIED and not have_carry:
            d.flags = ir.IMU_NO_CARRY
        else:
            d, q = gather(T, i, lens[i])
            if p == ir.KF_CARRIED and c_open is not None:
                d, q = compose(c_open, (d, q))
        ir._record(delta[i], d, p)
        _record(jac[i], q, p)
        rot[i] = ir.camera_rotation(P, d)
    out = np.zeros(1, JAC_CARRY_DTYPE)
    d, q, valid = ir.Delta(), Jac(), ir.IMU_CARRY_TIME
    if Lc > 0:
        (d, q), valid = gather(T, n - 1, Lc), valid | ir.IMU_CARRY_OPEN
        if last < 0 and c_open is not None:
            d, q = compose(c_open, (d, q))
    out[0]["carry"]["t_last"], out[0]["carry"]["valid"] = float(tframe[n - 1]), valid
    ir._record(out[0]["carry"]["open"], d, 0)
    _record(out[0]["open_jac"], q, 0)
    return delta, jac, rot, out


def preintegrate_jac(P, samples, t_a, t_b):
    """vis_imu_preintegrate_jac: (the delta, the Jacobians, the 9 float32 of the rotation)"""
    c = np.zeros(1, JAC_CARRY_DTYPE)
    c[0]["carry"]["t_last"], c[0]["carry"]["valid"] = t_a, ir.IMU_CARRY_TIME
    delta, jac, rot, _ = preintegrate_jac_rows(P, samples, [t_b], [ir.KF_CARRIED], c)
    return delta[0], jac[0], rot[0]


def jac_carry(carry, open_jac=None):
    """a JAC_CARRY record from an imu_ref CARRY record and the open delta's Jacobians (None: zero)"""
    c = np.zeros(1, JAC_CARRY_DTYPE)
    c[0]["carry"] = np.asarray(carry, ir.CARRY_DTYPE).reshape(-1)[0]
    if open_jac is not None:
        c[0]["open_jac"] = open_jac
    return c


def correct_rows(P, delta, jac, dbg, dba=None):
    """(d_delta_out, d_rot_out (n, 9) float32, d_status) of vis_imu_correct_rows; P gives r_ic and max_angle"""
    delta, jac = np.asarray(delta, ir.DELTA_DTYPE).reshape(-1), np.asarray(jac, JAC_DTYPE).reshape(-1)
    n = len(delta)
    bg = [float(x) for x in dbg]
    ba = [0.0, 0.0, 0.0] if dba is None else [float(x) for x in dba]
    out, rot, status = delta.copy(), np.zeros((n, 9), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        r, j = delta[i], jac[i]
        d = ir.Delta()
        d.R, d.v, d.p, d.dt, d.J = [float(x) for x in r["R"]], [float(x) for x in r["v"]], [float(x) for x in r["p"]], float(r["dt"]), [float(x) for x in r["JRg"]]
        d.flags = int(r["flags"])
        st = IMC_OK
        if d.flags & VOID_FLAGS or not all(ir.finite(x) for x in d.numbers()):
            st = IMC_UNUSABLE
        elif int(j["flags"]) & IMU_JAC_NONFINITE:
            st = IMC_JAC
        elif not all(ir.finite(x) for x in bg + ba):
            st = IMC_BIAS
        else:
            dR, _, th2 = ir.exp_and_jr(ir.mulv(d.J, bg))
            if th2 > P.max_angle * P.max_angle:
                st = IMC_ANGLE
            else:
                Rn = ir.mul(d.R, dR)
                blk = {f: [float(x) for x in j[f]] for f in BLOCKS}
                vg, va, pg, pa = ir.mulv(blk["Jvg"], bg), ir.mulv(blk["Jva"], ba), ir.mulv(blk["Jpg"], bg), ir.mulv(blk["Jpa"], ba)
                vn = [d.v[k] + (vg[k] + va[k]) for k in range(3)]
                pn = [d.p[k] + (pg[k] + pa[k]) for k in range(3)]
                if all(ir.finite(x) for x in Rn + vn + pn):
                    out[i]["R"], out[i]["v"], out[i]["p"] = Rn, vn, pn
                    d.R = Rn
                else:
                    st = IMC_NONFINITE
        status[i] = st
        rot[i] = ir.camera_rotation(P, d)
    return out, rot, status
