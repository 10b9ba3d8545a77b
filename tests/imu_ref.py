"""The IMU preintegration of include/vislam_hip.h restated operation for operation in plain Python floats (IEEE doubles, no contraction): the
intervals, the composition, the binary-lifting table, the pair records, the camera-frame rotations and the carry.  vis_imu_preintegrate_rows
equals preintegrate_rows() byte for byte.  sequential_rows() composes the same intervals left to right instead: the independent order the
lifting table is measured against."""
import math

import numpy as np

KF_CARRIED, KF_NOT_SAVED, KF_FIRST = -1, -2, -3
IMU_OK, IMU_NO_PAIR, IMU_NO_CARRY, IMU_NO_START, IMU_EMPTY, IMU_EXTRAPOLATED, IMU_GAP, IMU_FAST, IMU_ORDER, IMU_NONFINITE = 0, 1, 2, 4, 8, 16, 32, 64, 128, 256
IMU_CARRY_TIME, IMU_CARRY_OPEN = 1, 2
IMU_MAX_FRAMES, IMU_EXP_TERMS = 1024, 10
COEF_A = [1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
          1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15, -8.22063524662433e-18]
COEF_B = [0.5, -0.041666666666666664, 0.001388888888888889, -2.48015873015873e-05, 2.755731922398589e-07, -2.08767569878681e-09,
          1.1470745597729725e-11, -4.779477332387385e-14, 1.5619206968586225e-16, -4.110317623312165e-19]
COEF_C = [0.16666666666666666, -0.008333333333333333, 0.0001984126984126984, -2.7557319223985893e-06, 2.505210838544172e-08,
          -1.6059043836821613e-10, 7.647163731819816e-13, -2.8114572543455206e-15, 8.22063524662433e-18, -1.9572941063391263e-20]
FLT_MAX = 3.4028234663852886e38

SAMPLE_DTYPE = np.dtype([("t", "<f8"), ("w", "<f8", (3,)), ("a", "<f8", (3,))])
DELTA_DTYPE = np.dtype([("R", "<f8", (9,)), ("v", "<f8", (3,)), ("p", "<f8", (3,)), ("dt", "<f8"), ("JRg", "<f8", (9,)), ("n_steps", "<i4"),
                        ("flags", "<i4"), ("q", "<i4"), ("reserved_", "<i4")])
CARRY_DTYPE = np.dtype([("t_last", "<f8"), ("open", DELTA_DTYPE), ("valid", "<i4"), ("reserved_", "<i4")])
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


class Params:
    def __init__(self, bg=(0.0, 0.0, 0.0), ba=(0.0, 0.0, 0.0), r_ic=None, max_gap_s=0.05, max_angle=1.0):
        self.bg, self.ba = [float(x) for x in bg], [float(x) for x in ba]
        self.r_ic = [float(x) for x in (EYE if r_ic is None else np.asarray(r_ic, np.float64).reshape(9))]
        self.max_gap_s, self.max_angle = float(max_gap_s), float(max_angle)


class Delta:
    __slots__ = ("R", "v", "p", "dt", "J", "n_steps", "flags")

    def __init__(self):
        self.R, self.v, self.p, self.dt, self.J, self.n_steps, self.flags = list(EYE), [0.0] * 3, [0.0] * 3, 0.0, [0.0] * 9, 0, 0

    def copy(self):
        d = Delta()
        d.R, d.v, d.p, d.dt, d.J, d.n_steps, d.flags = list(self.R), list(self.v), list(self.p), self.dt, list(self.J), self.n_steps, self.flags
        return d

    def numbers(self):
        return self.R + self.v + self.p + [self.dt] + self.J


def finite(x):
    return abs(x) <= 1.7976931348623157e308


def div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def mul(A, B):
    return [(A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def tmul(A, B):
    return [(A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c] for r in range(3) for c in range(3)]


def mulv(A, x):
    return [(A[3 * r] * x[0] + A[3 * r + 1] * x[1]) + A[3 * r + 2] * x[2] for r in range(3)]


def horner(c, x):
    acc = c[IMU_EXP_TERMS - 1]
    for k in range(IMU_EXP_TERMS - 2, -1, -1):
        acc = c[k] + x * acc
    return acc


def exp_and_jr(phi):
    """(Exp(phi), Jr(phi), th2) by the header's formulas"""
    xx, yy, zz, xy, xz, yz = phi[0] * phi[0], phi[1] * phi[1], phi[2] * phi[2], phi[0] * phi[1], phi[0] * phi[2], phi[1] * phi[2]
    th2 = (xx + yy) + zz
    A, B, C = horner(COEF_A, th2), horner(COEF_B, th2), horner(COEF_C, th2)
    dR = [1.0 - B * (yy + zz), B * xy - A * phi[2], B * xz + A * phi[1],
          B * xy + A * phi[2], 1.0 - B * (xx + zz), B * yz - A * phi[0],
          B * xz - A * phi[1], B * yz + A * phi[0], 1.0 - B * (xx + yy)]
    Jr = [1.0 - C * (yy + zz), C * xy + B * phi[2], C * xz - B * phi[1],
          C * xy - B * phi[2], 1.0 - C * (xx + zz), C * yz + B * phi[0],
          C * xz + B * phi[1], C * yz - B * phi[0], 1.0 - C * (xx + yy)]
    return dR, Jr, th2


def void(d):
    """the identity with dt (0 when not finite), n_steps and flags kept, and IMU_NONFINITE"""
    o = Delta()
    o.dt, o.n_steps, o.flags = (d.dt if finite(d.dt) else 0.0), d.n_steps, d.flags | IMU_NONFINITE
    return o


def compose(X, Y):
    """X o Y, X the earlier"""
    O = Delta()
    O.R = mul(X.R, Y.R)
    Rv, Rp = mulv(X.R, Y.v), mulv(X.R, Y.p)
    O.v = [X.v[r] + Rv[r] for r in range(3)]
    O.p = [(X.p[r] + X.v[r] * Y.dt) + Rp[r] for r in range(3)]
    O.dt = X.dt + Y.dt
    M = tmul(Y.R, X.J)
    O.J = [M[k] + Y.J[k] for k in range(9)]
    O.n_steps, O.flags = X.n_steps + Y.n_steps, X.flags | Y.flags
    return O if all(finite(x) for x in O.numbers()) else void(O)


def _ub(ts, x):
    lo, hi = 0, len(ts)
    while lo < hi:
        mid = (lo + hi) >> 1
        if ts[mid] <= x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _lb(ts, x):
    lo, hi = 0, len(ts)
    while lo < hi:
        mid = (lo + hi) >> 1
        if ts[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _point_finite(s):
    return finite(s[0]) and all(finite(s[1][k]) and finite(s[2][k]) for k in range(3))


def _value(S, ts, x, d):
    """the value (t, w, a) at breakpoint x, or None when a sample it uses is not finite"""
    n = len(ts)
    j = _ub(ts, x)
    if j == 0 or j == n:
        s = S[0 if j == 0 else n - 1]
        if not _point_finite(s):
            return None
        if not s[0] == x:
            d.flags |= IMU_EXTRAPOLATED
        return (x, list(s[1]), list(s[2]))
    s0, s1 = S[j - 1], S[j]
    if not _point_finite(s0) or not _point_finite(s1):
        return None
    u = div(x - s0[0], s1[0] - s0[0])
    return (x, [s0[1][k] + u * (s1[1][k] - s0[1][k]) for k in range(3)], [s0[2][k] + u * (s1[2][k] - s0[2][k]) for k in range(3)])


def substep(d, P, s0, s1):
    h = s1[0] - s0[0]
    if not h > 0.0:
        d.flags |= IMU_ORDER
        return
    d.n_steps += 1
    if h > P.max_gap_s:
        d.flags |= IMU_GAP
    phi = [(0.5 * (s0[1][k] + s1[1][k]) - P.bg[k]) * h for k in range(3)]
    dR, Jr, th2 = exp_and_jr(phi)
    if th2 > P.max_angle * P.max_angle:
        d.flags |= IMU_FAST
    Rn = mul(d.R, dR)
    u0, u1 = [s0[2][k] - P.ba[k] for k in range(3)], [s1[2][k] - P.ba[k] for k in range(3)]
    r0, r1 = mulv(d.R, u0), mulv(Rn, u1)
    for r in range(3):
        am = 0.5 * (r0[r] + r1[r])
        d.p[r] = d.p[r] + (d.v[r] * h + (0.5 * am) * (h * h))
        d.v[r] = d.v[r] + am * h
    M = tmul(dR, d.J)
    d.J = [M[k] - Jr[k] * h for k in range(9)]
    d.R = Rn


def _samples(samples):
    s = np.asarray(samples, SAMPLE_DTYPE).reshape(-1)
    S = [(float(r["t"]), [float(x) for x in r["w"]], [float(x) for x in r["a"]]) for r in s]
    return S, [r[0] for r in S]


def interval(P, S, ts, ta, tb):
    """the delta of (ta, tb]; ta None: interval 0 without a carried time"""
    d = Delta()
    if ta is None:
        d.flags = IMU_NO_START
        return d
    d.dt = tb - ta
    if not finite(d.dt):
        d.dt = 0.0
    bad = not finite(ta) or not finite(tb)
    if not bad and len(ts) < 1:
        d.flags |= IMU_EMPTY | IMU_EXTRAPOLATED
    if not bad and len(ts) >= 1:
        pa = _value(S, ts, ta, d)
        bad = pa is None
        if not bad:
            pb = _value(S, ts, tb, d)
            bad = pb is None
        lo, hi = _ub(ts, ta), _lb(ts, tb)
        if not bad:
            if hi <= lo:
                d.flags |= IMU_EMPTY
            bad = not all(_point_finite(S[j]) for j in range(lo, hi))
        if not bad:
            cur = pa
            for j in range(lo, hi):
                substep(d, P, cur, S[j])
                cur = S[j]
            substep(d, P, cur, pb)
    if bad or not all(finite(x) for x in d.numbers()):
        d = void(d)
    return d


def norm_prev(prev, i):
    p = int(prev[i])
    if p >= 0:
        return p if p < i else KF_FIRST
    return p if p in (KF_CARRIED, KF_NOT_SAVED) else KF_FIRST


def _carry_parts(carry):
    """(t_last or None, the open delta or None) of an IMU_CARRY record or None"""
    if carry is None:
        return None, None
    c = np.asarray(carry, CARRY_DTYPE).reshape(-1)[0]
    if not int(c["valid"]) & IMU_CARRY_TIME:
        return None, None
    o = None
    if int(c["valid"]) & IMU_CARRY_OPEN:
        o = Delta()
        r = c["open"]
        o.R, o.v, o.p, o.dt, o.J = [float(x) for x in r["R"]], [float(x) for x in r["v"]], [float(x) for x in r["p"]], float(r["dt"]), [float(x) for x in r["JRg"]]
        o.n_steps, o.flags = int(r["n_steps"]), int(r["flags"])
    return float(c["t_last"]), o


def intervals(P, samples, tframe, carry=None):
    S, ts = _samples(samples)
    t_last, _ = _carry_parts(carry)
    tf = [float(t) for t in tframe]
    return [interval(P, S, ts, tf[i - 1] if i > 0 else t_last, tf[i]) for i in range(len(tf))]


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
            acc = T[k][pos].copy() if acc is None else compose(T[k][pos], acc)
            pos -= 1 << k
        k += 1
    return acc


def sequential(T0, i, L):
    """the same intervals composed left to right"""
    acc = T0[i - L + 1].copy()
    for j in range(i - L + 2, i + 1):
        acc = compose(acc, T0[j])
    return acc


def _record(out, d, q):
    out["R"], out["v"], out["p"], out["dt"], out["JRg"] = d.R, d.v, d.p, d.dt, d.J
    out["n_steps"], out["flags"], out["q"], out["reserved_"] = d.n_steps, d.flags, q, 0


def camera_rotation(P, d):
    M = mul(tmul(P.r_ic, d.R), P.r_ic)
    ok = not d.flags & (IMU_NO_PAIR | IMU_NO_CARRY | IMU_NONFINITE) and all(abs(x) <= FLT_MAX for x in M)
    return np.asarray(M if ok else EYE, np.float64).astype(np.float32)


def preintegrate_rows(P, samples, tframe, prev, carry=None, gather=lift):
    """(d_delta (n), d_rot (n, 9) float32, d_carry_out) of vis_imu_preintegrate_rows; gather=sequential: the left-to-right order"""
    n = len(tframe)
    t_last, c_open = _carry_parts(carry)
    have_carry = t_last is not None
    T0 = intervals(P, samples, tframe, carry)
    pv = [norm_prev(prev, i) for i in range(n)]
    lens = [i - p if p >= 0 else (i + 1 if p == KF_CARRIED and have_carry else 0) for i, p in enumerate(pv)]
    saved = [i for i in range(n) if pv[i] != KF_NOT_SAVED]
    last = saved[-1] if saved else -1
    Lc = n - 1 - last if last >= 0 else n
    T = lifting_table(T0, max(lens + [Lc])) if gather is lift else T0
    delta, rot = np.zeros(n, DELTA_DTYPE), np.zeros((n, 9), np.float32)
    for i, p in enumerate(pv):
        d = Delta()
        if p in (KF_NOT_SAVED, KF_FIRST):
            d.flags = IMU_NO_PAIR
        elif p == KF_CARRIED and not have_carry:
            d.flags = IMU_NO_CARRY
        else:
            d = gather(T, i, lens[i])
            if p == KF_CARRIED and c_open is not None:
                d = compose(c_open, d)
        _record(delta[i], d, p)
        rot[i] = camera_rotation(P, d)
    out = np.zeros(1, CARRY_DTYPE)
    d, valid = Delta(), IMU_CARRY_TIME
    if Lc > 0:
        d, valid = gather(T, n - 1, Lc), valid | IMU_CARRY_OPEN
        if last < 0 and c_open is not None:
            d = compose(c_open, d)
    out[0]["t_last"], out[0]["valid"] = float(tframe[n - 1]), valid
    _record(out[0]["open"], d, 0)
    return delta, rot, out


def preintegrate(P, samples, t_a, t_b):
    """vis_imu_preintegrate: (the record, the 9 float32 of the rotation)"""
    c = np.zeros(1, CARRY_DTYPE)
    c[0]["t_last"], c[0]["valid"] = t_a, IMU_CARRY_TIME
    delta, rot, _ = preintegrate_rows(P, samples, [t_b], [KF_CARRIED], c)
    return delta[0], rot[0]
