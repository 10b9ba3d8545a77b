"""The visual-inertial alignment of include/vislam_hip.h (vis_vi_align_rows) restated operation for operation in plain Python floats (IEEE
doubles, one rounding per + - * / sqrt, nothing contracted): the tails, the gyro and the linear terms, the sums under contract T, the LDL^T
solves, the gravity refinement, the per-frame states and the carry.  Not a test module; nothing here calls the code under test.
vis_vi_align_rows equals align_rows() byte for byte."""
import math

import numpy as np

import imu_ref as ir
from essential_polish_ref import tiled_sums
from imu_ref import KF_CARRIED, KF_NOT_SAVED, div, exp_and_jr, finite, mul, mulv, norm_prev, tmul
from trajectory_ref import TJ_NOT_SAVED, TJ_OVERFLOW, TJ_ROOT, TRAJ_DTYPE

VIA_GYRO_FEW, VIA_GYRO_SINGULAR, VIA_FEW, VIA_SINGULAR, VIA_SCALE, VIA_GRAVITY_NORM, VIA_RESTART, VIA_BAD_CARRY = 1, 2, 4, 8, 16, 32, 64, 128
VIA_FAILED = VIA_FEW | VIA_SINGULAR | VIA_SCALE
VIS_HAS_P, VIS_HAS_V, VIS_HAS_TRIPLE, VIS_HAS_PAIR = 1, 2, 4, 8
VIT_POSED, VIT_EDGE, VIT_DELTA = 1, 2, 4
VIC_VALID = 1
VIA_MAX_FRAMES = 1024
EXCITATION_REL = 2.0 ** -40                                            # VIS_VIA_EXCITATION_REL

STATE_DTYPE = np.dtype([("p", "<f8", (3,)), ("v", "<f8", (3,)), ("res", "<f8"), ("flags", "<i4"), ("q", "<i4")])
RESULT_DTYPE = np.dtype([("dbg", "<f8", (3,)), ("c0", "<f8"), ("c0_call", "<f8"), ("c1", "<f8"), ("s", "<f8"), ("g", "<f8", (3,)), ("s_lin", "<f8"),
                         ("g_lin", "<f8", (3,)), ("g_lin_norm", "<f8"), ("rms", "<f8"), ("n_pairs", "<i4"), ("n_triples", "<i4"),
                         ("n_pairs_call", "<i4"), ("n_triples_call", "<i4"), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("flags", "<i4"),
                         ("reserved_", "<i4")])
TAIL_DTYPE = np.dtype([("C", "<f8", (3,)), ("Rw", "<f8", (9,)), ("L", "<f8", (3,)), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("flags", "<i4"),
                       ("reserved_", "<i4")])
CARRY_DTYPE = np.dtype([("gyro", "<f8", (10,)), ("lin", "<f8", (16,)), ("n_pairs", "<i4"), ("n_triples", "<i4"), ("segment_seq", "<i4"),
                        ("epoch_seq", "<i4"), ("last", TAIL_DTYPE), ("parent", TAIL_DTYPE), ("last_delta", ir.DELTA_DTYPE), ("valid", "<i4"),
                        ("reserved_", "<i4")])
assert STATE_DTYPE.itemsize == 64 and RESULT_DTYPE.itemsize == 160 and TAIL_DTYPE.itemsize == 136 and CARRY_DTYPE.itemsize == 720


class Params:
    def __init__(self, r_ic=None, p_ci=(0.0, 0.0, 0.0), G=9.81, g_tol=0.1, min_pairs=8, min_triples=8, refine_iters=4,
                 reject=ir.IMU_EMPTY | ir.IMU_GAP):
        self.r_ic = [float(x) for x in (ir.EYE if r_ic is None else np.asarray(r_ic, np.float64).reshape(9))]
        self.p_ci = [float(x) for x in p_ci]
        self.G, self.g_tol = float(G), float(g_tol)
        self.min_pairs, self.min_triples, self.refine_iters, self.reject = int(min_pairs), int(min_triples), int(refine_iters), int(reject)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def tmulv(A, x):
    """A^T x"""
    return [(A[r] * x[0] + A[3 + r] * x[1]) + A[6 + r] * x[2] for r in range(3)]


class Tail:
    __slots__ = ("C", "Rw", "L", "seg", "epoch", "flags")

    def __init__(self):
        self.C, self.Rw, self.L, self.seg, self.epoch, self.flags = [0.0] * 3, [0.0] * 9, [0.0] * 3, 0, 0, 0

    def numbers(self):
        return self.C + self.Rw + self.L


def tail_of(P, T, q):
    """the tail of a trajectory record whose frame has the (normalised) pair q"""
    o = Tail()
    if int(T["flags"]) & (TJ_NOT_SAVED | TJ_OVERFLOW):
        return o
    R, t = [float(x) for x in T["R"]], [float(x) for x in T["t"]]
    Rt = tmulv(R, t)
    o.C = [-Rt[r] for r in range(3)]
    M = mul(P.r_ic, R)
    o.Rw = [M[3 * c + r] for r in range(3) for c in range(3)]
    o.L = tmulv(R, P.p_ci)
    if not all(finite(x) for x in o.numbers()):
        return Tail()
    o.seg, o.epoch, o.flags = int(T["segment_seq"]), int(T["epoch_seq"]), VIT_POSED
    if not int(T["flags"]) & TJ_ROOT and int(T["parent"]) == q and (q >= 0 or q == KF_CARRIED):
        o.flags |= VIT_EDGE
    return o


def tail_from_record(r):
    o = Tail()
    o.C, o.Rw, o.L = [float(x) for x in r["C"]], [float(x) for x in r["Rw"]], [float(x) for x in r["L"]]
    o.seg, o.epoch, o.flags = int(r["segment_seq"]), int(r["epoch_seq"]), int(r["flags"])
    return o


def tail_to_record(out, t):
    out["C"], out["Rw"], out["L"], out["segment_seq"], out["epoch_seq"], out["flags"], out["reserved_"] = t.C, t.Rw, t.L, t.seg, t.epoch, t.flags, 0


class Dl:
    """the numbers of a delta record the alignment reads"""
    __slots__ = ("R", "v", "p", "dt", "J")


def delta_of(D):
    d = Dl()
    d.R, d.v, d.p, d.dt, d.J = [float(x) for x in D["R"]], [float(x) for x in D["v"]], [float(x) for x in D["p"]], float(D["dt"]), [float(x) for x in D["JRg"]]
    return d


def delta_usable(P, D, parent):
    if int(D["flags"]) & (ir.IMU_NO_PAIR | ir.IMU_NO_CARRY | ir.IMU_NO_START | ir.IMU_NONFINITE | P.reject):
        return False
    d = delta_of(D)
    if not all(finite(x) for x in d.R + d.v + d.p + [d.dt] + d.J):
        return False
    return d.dt > 0.0 and int(D["q"]) == parent


def ldl(A, b, n):
    """(ok, x) of A x = b by LDL^T without pivoting, er_solve5's order of operations"""
    L = [[0.0] * n for _ in range(n)]
    D, z, x = [0.0] * n, [0.0] * n, [0.0] * n
    ok = True
    for j in range(n):
        s = A[j][j]
        for c in range(j):
            s = s - (L[j][c] * L[j][c]) * D[c]
        D[j] = s
        ok = ok and s > 0.0 and finite(s)
        for i in range(j + 1, n):
            v = A[i][j]
            for c in range(j):
                v = v - (L[i][c] * L[j][c]) * D[c]
            L[i][j] = div(v, s)
    for i in range(n):
        v = b[i]
        for c in range(i):
            v = v - L[i][c] * z[c]
        z[i] = v
    for i in range(n - 1, -1, -1):
        v = div(z[i], D[i])
        for c in range(i + 1, n):
            v = v - L[c][i] * x[c]
        x[i] = v
    return ok and all(finite(v) for v in x), x


def rot_error(dR, V):
    Er = tmul(dR, V)
    return [0.5 * (Er[7] - Er[5]), 0.5 * (Er[2] - Er[6]), 0.5 * (Er[3] - Er[1])]


def gyro_terms(d, V):
    """the ten terms of a pair: J^T J (6, rows), J^T e (3), e.e; None when one is not finite"""
    e, J = rot_error(d.R, V), d.J
    t = [(J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b] for a in range(3) for b in range(a, 3)]
    t += [(J[a] * e[0] + J[3 + a] * e[1]) + J[6 + a] * e[2] for a in range(3)]
    t.append(dot(e, e))
    return t if all(finite(x) for x in t) else None


def gyro_after(d, V, dbg):
    """e.e of the pair with dR Exp(J dbg)"""
    dR = mul(d.R, exp_and_jr(mulv(d.J, dbg))[0])
    e = rot_error(dR, V)
    return dot(e, e)


def triple_parts(ta, tb, tc, db, dc):
    """(lam, beta, gam, exc) of the triple a -> b -> c; db is b's delta (a -> b), dc is c's (b -> c)"""
    dt1, dt2 = db.dt, dc.dt
    d1, d2 = [(tc.C[r] - tb.C[r]) * dt1 for r in range(3)], [(tb.C[r] - ta.C[r]) * dt2 for r in range(3)]
    lam = [d1[r] - d2[r] for r in range(3)]
    beta = -(((0.5 * dt1) * dt2) * (dt1 + dt2))
    u1, u2, u3 = mulv(tb.Rw, dc.p), mulv(ta.Rw, db.p), mulv(ta.Rw, db.v)
    gam = [((u1[r] * dt1 - u2[r] * dt2) + u3[r] * (dt1 * dt2)) - ((tc.L[r] - tb.L[r]) * dt1 - (tb.L[r] - ta.L[r]) * dt2) for r in range(3)]
    return lam, beta, gam, dot(d1, d1) + dot(d2, d2)


def linear_terms(lam, beta, gam, exc):
    """the eleven terms: M00, M01, M02, M03, beta^2, r0 ... r3, gam.gam, the excitation scale; None when one is not finite"""
    t = [dot(lam, lam), lam[0] * beta, lam[1] * beta, lam[2] * beta, beta * beta, dot(lam, gam), beta * gam[0], beta * gam[1], beta * gam[2], dot(gam, gam), exc]
    return t if all(finite(x) for x in t) else None


def expand_linear(t):
    """the 16 carried linear sums from the eleven summed ones: M in rows of the upper triangle (10), r (4), gam.gam, the excitation scale"""
    return [t[0], t[1], t[2], t[3], t[4], 0.0, 0.0, t[4], 0.0, t[4], t[5], t[6], t[7], t[8], t[9], t[10]]


def matrix4(lin):
    M = [[0.0] * 4 for _ in range(4)]
    k = 0
    for a in range(4):
        for b in range(a, 4):
            M[a][b] = M[b][a] = lin[k]
            k += 1
    return M, list(lin[10:14])


def normalise(v):
    n = math.sqrt(dot(v, v))
    return n, [div(v[k], n) for k in range(3)]


def refine_gravity(M, r, g_lin, s_lin, G, iters):
    """step 3: (ok, s, gh)"""
    n, gh = normalise(g_lin)
    if not (finite(n) and n > 0.0):
        return False, 1.0, [0.0] * 3
    s = s_lin
    for _ in range(iters):
        k = 0
        for j in (1, 2):
            if abs(gh[j]) < abs(gh[k]):
                k = j
        d = [(1.0 if j == k else 0.0) - gh[k] * gh[j] for j in range(3)]
        _, b1 = normalise(d)
        b2 = [gh[1] * b1[2] - gh[2] * b1[1], gh[2] * b1[0] - gh[0] * b1[2], gh[0] * b1[1] - gh[1] * b1[0]]
        x0 = [G * gh[j] for j in range(3)]
        rr = [r[i] - ((M[i][1] * x0[0] + M[i][2] * x0[1]) + M[i][3] * x0[2]) for i in range(4)]
        q = [rr[0], dot(b1, rr[1:]), dot(b2, rr[1:])]
        w1 = [dot(M[1 + i][1:], b1) for i in range(3)]
        w2 = [dot(M[1 + i][1:], b2) for i in range(3)]
        n01, n02 = dot(M[0][1:], b1), dot(M[0][1:], b2)
        n12 = dot(b1, w2)
        N = [[M[0][0], n01, n02], [n01, dot(b1, w1), n12], [n02, n12, dot(b2, w2)]]
        ok, y = ldl(N, q, 3)
        if not ok:
            return False, 1.0, [0.0] * 3
        g = [(x0[j] + y[1] * b1[j]) + y[2] * b2[j] for j in range(3)]
        n, gh = normalise(g)
        if not (finite(n) and n > 0.0 and all(finite(x) for x in gh)):
            return False, 1.0, [0.0] * 3
        s = y[0]
    return True, s, gh


def carry_parts(carry):
    """(the record or None, bad): a carry counts when it is given, has VIC_VALID and every number of it is finite"""
    if carry is None:
        return None, False
    c = np.asarray(carry, CARRY_DTYPE).reshape(-1)[0]
    if not int(c["valid"]) & VIC_VALID:
        return None, False
    nums = list(c["gyro"]) + list(c["lin"])
    for t in (c["last"], c["parent"]):
        nums += list(t["C"]) + list(t["Rw"]) + list(t["L"])
    d = c["last_delta"]
    nums += list(d["R"]) + list(d["v"]) + list(d["p"]) + [d["dt"]] + list(d["JRg"])
    if not all(finite(float(x)) for x in nums):
        return None, True
    return c, False


def align_rows(P, prev, traj, delta, carry=None, want_carry=True, detail=None):
    """(states (n) STATE_DTYPE, the RESULT_DTYPE record, the CARRY_DTYPE record) of vis_vi_align_rows.  detail: a dict that receives the sums of the
    absolute terms of the call (gyro 10, lin 16), the scale a difference between two orders of summation is measured against"""
    n = len(prev)
    traj, delta = np.asarray(traj, TRAJ_DTYPE), np.asarray(delta, ir.DELTA_DTYPE)
    c_in, bad_carry = carry_parts(carry)
    flags = VIA_BAD_CARRY if bad_carry else 0
    c_last = tail_from_record(c_in["last"]) if c_in is not None else Tail()
    c_parent = tail_from_record(c_in["parent"]) if c_in is not None else Tail()
    c_delta = delta_of(c_in["last_delta"]) if c_in is not None else None
    q = [norm_prev(prev, i) for i in range(n)]
    tails = [tail_of(P, traj[i], q[i]) for i in range(n)]
    usable = [delta_usable(P, delta[i], int(traj[i]["parent"])) for i in range(n)]
    dl = [delta_of(delta[i]) for i in range(n)]

    def parent_of(i):
        """(tail, delta, delta usable, its own pair) of the parent of frame i"""
        if q[i] >= 0:
            return tails[q[i]], dl[q[i]], usable[q[i]], q[q[i]]
        if q[i] == KF_CARRIED:
            return c_last, c_delta, bool(c_last.flags & VIT_DELTA), None
        return Tail(), None, False, None

    def grandparent_of(i):
        if q[i] >= 0:
            return parent_of(q[i])[0]
        return c_parent if q[i] == KF_CARRIED else Tail()

    posed = [i for i in range(n) if tails[i].flags & VIT_POSED]
    if posed:
        S, E = tails[posed[-1]].seg, tails[posed[-1]].epoch
    elif c_in is not None:
        S, E = int(c_in["segment_seq"]), int(c_in["epoch_seq"])
    else:
        S, E = -1, -1

    # ---- the terms
    gterms, lterms = np.zeros((n, 10)), np.zeros((n, 11))
    pair, triple, parts = [False] * n, [False] * n, [None] * n
    for i in range(n):
        tc = tails[i]
        tb, db, ub, _ = parent_of(i)
        if tc.flags & VIT_EDGE and tb.flags & VIT_POSED and usable[i]:
            t = gyro_terms(dl[i], tmul(tb.Rw, tc.Rw))
            if t is not None:
                gterms[i], pair[i] = t, True
        ta = grandparent_of(i)
        if (tc.flags & VIT_EDGE and tb.flags & VIT_EDGE and ta.flags & VIT_POSED and usable[i] and ub and (tc.seg, tc.epoch) == (S, E)
                and (tb.seg, tb.epoch) == (S, E)):
            lam, beta, gam, exc = triple_parts(ta, tb, tc, db, dl[i])
            t = linear_terms(lam, beta, gam, exc)
            if t is not None:
                lterms[i], triple[i], parts[i] = t, True, (lam, beta, gam)
    gcall, lcall = tiled_sums(gterms) if n else [0.0] * 10, tiled_sums(lterms) if n else [0.0] * 11
    np_call, nt_call = sum(pair), sum(triple)
    lcall = expand_linear(lcall)
    if detail is not None:
        detail["gyro"], detail["lin"] = np.abs(gterms).sum(0), np.asarray(expand_linear(list(np.abs(lterms).sum(0))))

    # ---- the totals
    gyro, lin, n_pairs, n_triples = list(gcall), list(lcall), np_call, nt_call
    if c_in is not None:
        gyro = [float(c_in["gyro"][k]) + gcall[k] for k in range(10)]
        n_pairs = int(c_in["n_pairs"]) + np_call
        if (int(c_in["segment_seq"]), int(c_in["epoch_seq"])) == (S, E):
            lin = [float(c_in["lin"][k]) + lcall[k] for k in range(16)]
            n_triples = int(c_in["n_triples"]) + nt_call
        else:
            flags |= VIA_RESTART

    if not all(finite(x) for x in gyro):                             # (finite terms can still overflow a sum)
        gyro, n_pairs, flags = [0.0] * 10, 0, flags | VIA_GYRO_SINGULAR
    if not all(finite(x) for x in lin):
        lin, n_triples, flags = [0.0] * 16, 0, flags | VIA_SINGULAR

    # ---- step 1
    dbg = [0.0] * 3
    if n_pairs < P.min_pairs:
        flags |= VIA_GYRO_FEW
    else:
        H = [[gyro[0], gyro[1], gyro[2]], [gyro[1], gyro[3], gyro[4]], [gyro[2], gyro[4], gyro[5]]]
        ok, x = ldl(H, gyro[6:9], 3)
        if ok:
            dbg = x
        else:
            flags |= VIA_GYRO_SINGULAR

    # ---- steps 2 and 3
    s, g, s_lin, g_lin, g_norm = 1.0, [0.0] * 3, 0.0, [0.0] * 3, 0.0
    if n_triples < P.min_triples:
        flags |= VIA_FEW
    else:
        M, r = matrix4(lin)
        ok, x = ldl(M, r, 4)
        if not ok or not lin[0] > EXCITATION_REL * lin[15]:
            flags |= VIA_SINGULAR
        else:
            s_lin, g_lin = x[0], x[1:]
            g_norm = math.sqrt(dot(g_lin, g_lin))
            if not finite(g_norm):
                flags |= VIA_SINGULAR
                s_lin, g_lin, g_norm = 0.0, [0.0] * 3, 0.0
            else:
                if abs(g_norm - P.G) > P.g_tol * P.G:
                    flags |= VIA_GRAVITY_NORM
                if not s_lin > 0.0:
                    flags |= VIA_SCALE
                else:
                    ok, s3, gh = refine_gravity(M, r, g_lin, s_lin, P.G, P.refine_iters)
                    g3 = [P.G * gh[k] for k in range(3)]
                    if not ok or not all(finite(v) for v in g3):
                        flags |= VIA_SINGULAR
                    elif not (finite(s3) and s3 > 0.0):
                        flags |= VIA_SCALE
                    else:
                        s, g = s3, g3

    # ---- step 4
    states = np.zeros(n, STATE_DTYPE)
    c1_terms, res_terms = np.zeros((n, 2)), None
    for i in range(n):
        st = states[i]
        st["q"] = q[i]
        f = 0
        tc = tails[i]
        tb, db, ub, _ = parent_of(i)
        in_se = bool(tc.flags & VIT_POSED) and (tc.seg, tc.epoch) == (S, E)
        pc = [s * tc.C[r] + tc.L[r] for r in range(3)]
        if in_se and all(finite(x) for x in pc):
            st["p"], f = pc, f | VIS_HAS_P
        if in_se and tc.flags & VIT_EDGE and usable[i] and tb.flags & VIT_POSED and tb.seg == S:
            d = dl[i]
            pb = [s * tb.C[r] + tb.L[r] for r in range(3)]
            w = mulv(tb.Rw, [d.v[k] - div(d.p[k], d.dt) for k in range(3)])
            v = [(div(pc[r] - pb[r], d.dt) + (0.5 * g[r]) * d.dt) + w[r] for r in range(3)]
            if all(finite(x) for x in v):
                st["v"], f = v, f | VIS_HAS_V
        if pair[i]:
            f |= VIS_HAS_PAIR
            e1 = gyro_after(dl[i], tmul(tb.Rw, tc.Rw), dbg)
            c1_terms[i][0] = e1 if finite(e1) else 0.0
        if triple[i]:
            f |= VIS_HAS_TRIPLE
            lam, beta, gam = parts[i]
            rho = [(lam[r] * s + beta * g[r]) - gam[r] for r in range(3)]
            rr = dot(rho, rho)
            if finite(rr):
                c1_terms[i][1] = rr
                st["res"] = math.sqrt(rr)
        st["flags"] = f
    sums2 = tiled_sums(c1_terms) if n else [0.0, 0.0]

    res = np.zeros(1, RESULT_DTYPE)[0]
    res["dbg"], res["c0"], res["c0_call"], res["c1"] = dbg, gyro[9], gcall[9] if finite(gcall[9]) else 0.0, sums2[0] if finite(sums2[0]) else 0.0
    res["s"], res["g"], res["s_lin"], res["g_lin"], res["g_lin_norm"] = s, g, s_lin, g_lin, g_norm
    res["rms"] = math.sqrt(sums2[1] / nt_call) if nt_call > 0 and finite(sums2[1]) else 0.0
    res["n_pairs"], res["n_triples"], res["n_pairs_call"], res["n_triples_call"] = n_pairs, n_triples, np_call, nt_call
    res["segment_seq"], res["epoch_seq"], res["flags"] = S, E, flags

    out = np.zeros(1, CARRY_DTYPE)
    if want_carry:
        o = out[0]
        o["gyro"], o["lin"], o["n_pairs"], o["n_triples"], o["segment_seq"], o["epoch_seq"], o["valid"] = gyro, lin, n_pairs, n_triples, S, E, VIC_VALID
        saved = [i for i in range(n) if q[i] != KF_NOT_SAVED]
        if saved:
            i = saved[-1]
            t = tails[i]
            lt = Tail()
            lt.C, lt.Rw, lt.L, lt.seg, lt.epoch, lt.flags = t.C, t.Rw, t.L, t.seg, t.epoch, t.flags | (VIT_DELTA if usable[i] else 0)
            tail_to_record(o["last"], lt)
            tail_to_record(o["parent"], parent_of(i)[0])
            o["parent"]["flags"] &= VIT_POSED
            if usable[i]:
                o["last_delta"] = delta[i]
                o["last_delta"]["reserved_"] = 0
        elif c_in is not None:
            o["last"], o["parent"], o["last_delta"] = c_in["last"], c_in["parent"], c_in["last_delta"]
            o["last"]["reserved_"] = o["parent"]["reserved_"] = o["last_delta"]["reserved_"] = 0
    return states, res, out
