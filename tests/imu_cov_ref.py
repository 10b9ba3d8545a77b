"""The covariance of the IMU deltas of include/vislam_hip.h ("THE COVARIANCE") restated operation for operation in plain Python floats (IEEE
doubles, no contraction), on top of tests/imu_ref.py: the propagation by blocks, the sub-step, the composition, the lifting table, the pair records
and the carry.  vis_imu_preintegrate_cov_rows equals preintegrate_cov_rows() byte for byte; the delta part is imu_ref's by construction of the same
operations and is asserted to be (tests/test_imu_cov_ref.py)."""
import numpy as np

import imu_ref as ir

IMU_COV_OK, IMU_COV_NONFINITE = 0, 1
VOID_FLAGS = ir.IMU_NO_PAIR | ir.IMU_NO_CARRY | ir.IMU_NO_START | ir.IMU_NONFINITE
SIGMA_G, SIGMA_A = 1.6968e-4, 2.0e-3                                 # vis_default_imu_noise (EuRoC)
UP = (0, 1, 2, 4, 5, 8)                                              # the upper triangle's entries in a full 3 x 3

NOISE_DTYPE = np.dtype([("sigma_g", "<f8"), ("sigma_a", "<f8")])
COV_DTYPE = np.dtype([("S", "<f8", (45,)), ("flags", "<i4"), ("q", "<i4")])
COV_CARRY_DTYPE = np.dtype([("carry", ir.CARRY_DTYPE), ("open_cov", COV_DTYPE)])


class Noise:
    def __init__(self, sigma_g=SIGMA_G, sigma_a=SIGMA_A):
        self.sigma_g, self.sigma_a = float(sigma_g), float(sigma_a)


class Cov:
    """the six blocks: A phi-phi, C v-v, F p-p (upper triangles, 6 numbers), B v-phi, D p-phi, E p-v (9 numbers, row-major)"""
    __slots__ = ("A", "B", "C", "D", "E", "F", "flags")

    def __init__(self):
        self.A, self.B, self.C, self.D, self.E, self.F, self.flags = [0.0] * 6, [0.0] * 9, [0.0] * 6, [0.0] * 9, [0.0] * 9, [0.0] * 6, 0

    def copy(self):
        q = Cov()
        q.A, q.B, q.C, q.D, q.E, q.F, q.flags = list(self.A), list(self.B), list(self.C), list(self.D), list(self.E), list(self.F), self.flags
        return q

    def numbers(self):
        return self.A + self.B + self.C + self.D + self.E + self.F

    def matrix(self):
        """the symmetric 9 x 9"""
        M = np.zeros((9, 9))
        M[np.triu_indices(9)] = pack(self)
        return M + np.triu(M, 1).T


def full(s):
    return [s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]]


def sym(i, j):
    return i * 3 - i * (i - 1) // 2 + (j - i)


def idx9(r, c):
    return r * 9 - r * (r - 1) // 2 + (c - r)


def mult(A, B):
    """A B^T"""
    return [(A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1]) + A[3 * r + 2] * B[3 * c + 2] for r in range(3) for c in range(3)]


def mskew(M, u):
    """M [u]x"""
    out = []
    for r in range(3):
        out += [M[3 * r + 1] * u[2] - M[3 * r + 2] * u[1], M[3 * r + 2] * u[0] - M[3 * r] * u[2], M[3 * r] * u[1] - M[3 * r + 1] * u[0]]
    return out


def pack(q):
    """the 45 of vis_imu_cov: the upper triangle of the 9 x 9 in row order"""
    S = [0.0] * 45
    for r in range(9):
        for c in range(r, 9):
            br, bc, i, j = r // 3, c // 3, r % 3, c % 3
            if br == bc:
                S[idx9(r, c)] = (q.A, q.C, q.F)[br][sym(i, j)]
            else:
                S[idx9(r, c)] = (q.B if bc == 1 else q.D)[3 * j + i] if br == 0 else q.E[3 * j + i]
    return S


def unpack(S, flags=0):
    q = Cov()
    q.flags = flags

    def blk(bi, bj):
        return [S[idx9(min(3 * bi + i, 3 * bj + j), max(3 * bi + i, 3 * bj + j))] for i in range(3) for j in range(3)]
    q.A, q.C, q.F = [blk(0, 0)[k] for k in UP], [blk(1, 1)[k] for k in UP], [blk(2, 2)[k] for k in UP]
    q.B, q.D, q.E = blk(1, 0), blk(2, 0), blk(2, 1)
    return q


def settle(d, q):
    """the rule every covariance record ends on: zero beside a voided delta or a flagged record; not finite beside a finite delta: zero and flagged"""
    zero = bool(d.flags & VOID_FLAGS) or bool(q.flags & IMU_COV_NONFINITE)
    if not zero and not all(ir.finite(x) for x in q.numbers()):
        q.flags |= IMU_COV_NONFINITE
        zero = True
    if zero:
        q.A, q.B, q.C, q.D, q.E, q.F = [0.0] * 6, [0.0] * 9, [0.0] * 6, [0.0] * 9, [0.0] * 9, [0.0] * 6
    return q


def propagate(X, M, b, c, t, N):
    """P(X; M, b, c, t) + N: F X F^T for F = [M^T 0 0; b I 0; c t I], block by block, the propagated term first; N's flags are kept"""
    A, B, C, D, E, F = full(X.A), X.B, full(X.C), X.D, X.E, full(X.F)
    o = Cov()
    o.flags = N.flags
    W = ir.tmul(M, ir.mul(A, M))
    o.A = [W[UP[j]] + N.A[j] for j in range(6)]
    T = ir.mul(b, A)
    U = [T[k] + B[k] for k in range(9)]
    W = ir.mul(U, M)
    o.B = [W[k] + N.B[k] for k in range(9)]
    W, T = mult(U, b), mult(b, B)
    o.C = [(W[UP[j]] + (T[UP[j]] + C[UP[j]])) + N.C[j] for j in range(6)]
    T = mult(c, B)
    Y = [T[k] + t * C[k] for k in range(9)]
    T = ir.mul(c, A)
    V = [(T[k] + t * B[k]) + D[k] for k in range(9)]
    W = ir.mul(V, M)
    o.D = [W[k] + N.D[k] for k in range(9)]
    Y = [Y[k] + E[k] for k in range(9)]
    W = mult(V, b)
    o.E = [(W[k] + Y[k]) + N.E[k] for k in range(9)]
    T, W = mult(c, D), mult(V, c)
    for i in range(3):
        for j in range(i, 3):
            Z = (T[3 * i + j] + t * E[3 * j + i]) + F[3 * i + j]
            o.F[sym(i, j)] = ((W[3 * i + j] + t * Y[3 * i + j]) + Z) + N.F[sym(i, j)]
    return o


def substep(d, q, P, noise, s0, s1):
    """imu_ref.substep with the covariance; the delta's operations are the same ones in the same order.  Returns the new covariance"""
    h = s1[0] - s0[0]
    if not h > 0.0:
        d.flags |= ir.IMU_ORDER
        return q
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
    # the covariance, before R moves on
    hh, qg, qa = 0.5 * h, ir.div(noise.sigma_g * noise.sigma_g, h), ir.div(noise.sigma_a * noise.sigma_a, h)
    S0, S1 = mskew(d.R, u0), mskew(Rn, u1)
    T = mult(S1, dR)
    b = [-(hh * (S0[k] + T[k])) for k in range(9)]
    c = [hh * b[k] for k in range(9)]
    K1 = [Jr[k] * h for k in range(9)]
    T = ir.mul(S1, K1)
    K2 = [-(hh * T[k]) for k in range(9)]
    K3 = [(d.R[k] + Rn[k]) * hh for k in range(9)]
    N1, N2, T, N3 = mult(K1, K1), mult(K2, K1), mult(K2, K2), mult(K3, K3)
    N = Cov()
    N.flags = q.flags
    N.A = [qg * N1[UP[j]] for j in range(6)]
    N.C = [qg * T[UP[j]] + qa * N3[UP[j]] for j in range(6)]
    N.B = [qg * N2[k] for k in range(9)]
    N.D = [hh * N.B[k] for k in range(9)]
    Cf = full(N.C)
    N.E = [hh * Cf[k] for k in range(9)]
    N.F = [hh * N.E[UP[j]] for j in range(6)]
    q = propagate(q, dR, b, c, h, N)
    d.J = Jn
    d.R = Rn
    return q


def interval(P, noise, S, ts, ta, tb):
    """imu_ref.interval with the covariance: (delta, cov)"""
    d, q = ir.Delta(), Cov()
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
                q = substep(d, q, P, noise, cur, S[j])
                cur = S[j]
            q = substep(d, q, P, noise, cur, pb)
    if bad or not all(ir.finite(x) for x in d.numbers()):
        d = ir.void(d)
    return d, settle(d, q)


def compose(X, Y):
    """(X.delta, X.cov) o (Y.delta, Y.cov), X the earlier: imu_ref.compose for the delta, then the six blocks"""
    (Xd, Xq), (Yd, Yq) = X, Y
    O = ir.compose(Xd, Yd)
    R = Xd.R
    G = Cov()
    G.flags = Yq.flags | Xq.flags
    G.A = list(Yq.A)
    G.B, G.D = ir.mul(R, Yq.B), ir.mul(R, Yq.D)
    G.E = mult(ir.mul(R, Yq.E), R)
    W = mult(ir.mul(R, full(Yq.C)), R)
    G.C = [W[k] for k in UP]
    W = mult(ir.mul(R, full(Yq.F)), R)
    G.F = [W[k] for k in UP]
    b, c = [-x for x in mskew(R, Yd.v)], [-x for x in mskew(R, Yd.p)]
    return O, settle(O, propagate(Xq, Yd.R, b, c, Yd.dt, G))


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
    """(t_last or None, (open delta, open cov) or None) of a COV_CARRY record or None"""
    if carry is None:
        return None, None
    c = np.asarray(carry, COV_CARRY_DTYPE).reshape(-1)[0]
    t_last, o = ir._carry_parts(c["carry"])
    if o is None:
        return t_last, None
    return t_last, (o, unpack([float(x) for x in c["open_cov"]["S"]], int(c["open_cov"]["flags"])))


def _record(out, q, prev):
    out["S"], out["flags"], out["q"] = pack(q), q.flags, prev


def intervals(P, noise, samples, tframe, carry=None):
    S, ts = ir._samples(samples)
    t_last, _ = _carry_parts(carry)
    tf = [float(t) for t in tframe]
    return [interval(P, noise, S, ts, tf[i - 1] if i > 0 else t_last, tf[i]) for i in range(len(tf))]


def preintegrate_cov_rows(P, noise, samples, tframe, prev, carry=None, gather=lift, table=None):
    """(d_delta (n), d_cov (n), d_rot (n, 9) float32, d_carry_out) of vis_imu_preintegrate_cov_rows; gather=sequential: the left-to-right order;
    table: lifting_table(intervals(...), n) of the same samples, times and carried time, when the caller has it already (its levels do not depend
    on the pairing, and a level the call would not build is not read)"""
    n = len(tframe)
    t_last, c_open = _carry_parts(carry)
    have_carry = t_last is not None
    T0 = intervals(P, noise, samples, tframe, carry) if table is None else table[0]
    pv = [ir.norm_prev(prev, i) for i in range(n)]
    lens = [i - p if p >= 0 else (i + 1 if p == ir.KF_CARRIED and have_carry else 0) for i, p in enumerate(pv)]
    saved = [i for i in range(n) if pv[i] != ir.KF_NOT_SAVED]
    last = saved[-1] if saved else -1
    Lc = n - 1 - last if last >= 0 else n
    T = (table if table is not None else lifting_table(T0, max(lens + [Lc]))) if gather is lift else T0
    delta, cov, rot = np.zeros(n, ir.DELTA_DTYPE), np.zeros(n, COV_DTYPE), np.zeros((n, 9), np.float32)
    for i, p in enumerate(pv):
        d, q = ir.Delta(), Cov()
        if p in (ir.KF_NOT_SAVED, ir.KF_FIRST):
            d.flags = ir.IMU_NO_PAIR
        elif p == ir.KF_CARRIED and not have_carry:
            d.flags = ir.IMU_NO_CARRY
        else:
            d, q = gather(T, i, lens[i])
            if p == ir.KF_CARRIED and c_open is not None:
                d, q = compose(c_open, (d, q))
        ir._record(delta[i], d, p)
        _record(cov[i], q, p)
        rot[i] = ir.camera_rotation(P, d)
    out = np.zeros(1, COV_CARRY_DTYPE)
    d, q, valid = ir.Delta(), Cov(), ir.IMU_CARRY_TIME
    if Lc > 0:
        (d, q), valid = gather(T, n - 1, Lc), valid | ir.IMU_CARRY_OPEN
        if last < 0 and c_open is not None:
            d, q = compose(c_open, (d, q))
    out[0]["carry"]["t_last"], out[0]["carry"]["valid"] = float(tframe[n - 1]), valid
    ir._record(out[0]["carry"]["open"], d, 0)
    _record(out[0]["open_cov"], q, 0)
    return delta, cov, rot, out


def preintegrate_cov(P, noise, samples, t_a, t_b):
    """vis_imu_preintegrate_cov: (the delta, the covariance, the 9 float32 of the rotation)"""
    c = np.zeros(1, COV_CARRY_DTYPE)
    c[0]["carry"]["t_last"], c[0]["carry"]["valid"] = t_a, ir.IMU_CARRY_TIME
    delta, cov, rot, _ = preintegrate_cov_rows(P, noise, samples, [t_b], [ir.KF_CARRIED], c)
    return delta[0], cov[0], rot[0]


def cov_carry(carry, open_cov=None):
    """a COV_CARRY record from an imu_ref CARRY record and the open delta's covariance (None: zero)"""
    c = np.zeros(1, COV_CARRY_DTYPE)
    c[0]["carry"] = np.asarray(carry, ir.CARRY_DTYPE).reshape(-1)[0]
    if open_cov is not None:
        c[0]["open_cov"] = open_cov
    return c


def matrix(rec):
    """the symmetric 9 x 9 of a COV_DTYPE record"""
    M = np.zeros((9, 9))
    M[np.triu_indices(9)] = np.asarray(rec["S"], np.float64)
    return M + np.triu(M, 1).T
