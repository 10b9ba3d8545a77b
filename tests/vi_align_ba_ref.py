"""The visual-inertial alignment with the accelerometer bias of include/vislam_hip.h (vis_vi_align_ba_rows) restated operation for operation in
plain Python floats, on top of vi_align_ref (the embedded 4-unknown record, its states and its carry ARE align_rows') and imu_jac_ref (the Jacobian
records): the usable-Jacobian rule, B, the 32 terms of a bias triple, their sums under contract T, the 7 x 7 and 6 x 6 LDL^T solves with the relative
pivot test, the fallback, the states under (s_ba, g_ba, dba) and the carry.  Not a test module; nothing here calls the code under test.
vis_vi_align_ba_rows equals align_ba_rows() byte for byte."""
import math

import numpy as np

import imu_ref as ir
import vi_align_ref as vr
from essential_polish_ref import tiled_sums
from imu_jac_ref import IMU_JAC_NONFINITE, JAC_DTYPE
from imu_ref import KF_CARRIED, KF_NOT_SAVED, div, finite, mul, mulv, norm_prev
from vi_align_ref import VIT_DELTA, VIT_EDGE, VIT_POSED, Tail, dot, normalise

VIAB_FEW, VIAB_UNOBSERVABLE, VIAB_SCALE, VIAB_BAD_CARRY = 1, 2, 4, 8
VIAB_FAILED = VIAB_FEW | VIAB_UNOBSERVABLE | VIAB_SCALE
PIVOT_REL = 2.0 ** -30                                                 # VIS_VIAB_PIVOT_REL
N_BA = 32

BA_RESULT_DTYPE = np.dtype([("a", vr.RESULT_DTYPE), ("dba", "<f8", (3,)), ("s_ba", "<f8"), ("g_ba", "<f8", (3,)), ("dba_lin", "<f8", (3,)),
                            ("s_lin7", "<f8"), ("g_lin7", "<f8", (3,)), ("g_lin7_norm", "<f8"), ("rms_ba", "<f8"), ("n_ba_triples", "<i4"),
                            ("n_ba_triples_call", "<i4"), ("ba_flags", "<i4"), ("reserved_", "<i4")])
BA_CARRY_DTYPE = np.dtype([("carry", vr.CARRY_DTYPE), ("ba", "<f8", (N_BA,)), ("n_ba_triples", "<i4"), ("reserved_", "<i4"), ("last_jac", JAC_DTYPE)])
assert BA_RESULT_DTYPE.itemsize == 304 and BA_RESULT_DTYPE.fields["dba"][1] == 160 and BA_CARRY_DTYPE.itemsize == 1280


class BaParams:
    def __init__(self, min_ba_triples=16, pivot_rel=PIVOT_REL):
        self.min_ba_triples, self.pivot_rel = int(min_ba_triples), float(pivot_rel)


def jac_blocks(J):
    """(Jva, Jpa) of a Jacobian record as lists"""
    return [float(x) for x in J["Jva"]], [float(x) for x in J["Jpa"]]


def jac_usable(J, dq):
    """a Jacobian record beside a delta whose q is dq"""
    if int(J["flags"]) & IMU_JAC_NONFINITE:
        return False
    if not all(finite(float(x)) for f in ("Jvg", "Jva", "Jpg", "Jpa") for x in J[f]):
        return False
    return int(J["q"]) == dq


def ldl_rel(A, b, n, rel):
    """vi_align_ref.ldl with the relative pivot test: a D[j] that is not finite, not > 0 or not > rel A[j][j] fails"""
    L = [[0.0] * n for _ in range(n)]
    D, z, x = [0.0] * n, [0.0] * n, [0.0] * n
    ok = True
    for j in range(n):
        s = A[j][j]
        for c in range(j):
            s = s - (L[j][c] * L[j][c]) * D[c]
        D[j] = s
        ok = ok and s > 0.0 and finite(s) and s > rel * A[j][j]
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
    return ok and all(finite(v) for v in x), x, D


def neg_b(ta, tb, Jpa_c, Jpa_b, Jva_b, dt1, dt2):
    """nB = -B, B[k] = ((Rw_b Jpa_c)[k] dt1 - (Rw_a Jpa_b)[k] dt2) + (Rw_a Jva_b)[k] (dt1 dt2)"""
    P1, P2, P3 = mul(tb.Rw, Jpa_c), mul(ta.Rw, Jpa_b), mul(ta.Rw, Jva_b)
    return [-((P1[k] * dt1 - P2[k] * dt2) + P3[k] * (dt1 * dt2)) for k in range(9)]


def ba_terms(lam, beta, gam, exc, nB):
    """the 32 terms of a bias triple, A = [lam | beta I | nB]; None when one is not finite"""
    def col(v, c):                                                    # (nB^T v)[c]
        return (nB[c] * v[0] + nB[3 + c] * v[1]) + nB[6 + c] * v[2]
    t = [dot(lam, lam), lam[0] * beta, lam[1] * beta, lam[2] * beta, beta * beta]
    t += [col(lam, c) for c in range(3)]
    t += [beta * nB[k] for k in range(9)]
    t += [(nB[a] * nB[b] + nB[3 + a] * nB[3 + b]) + nB[6 + a] * nB[6 + b] for a in range(3) for b in range(a, 3)]
    t += [dot(lam, gam), beta * gam[0], beta * gam[1], beta * gam[2]]
    t += [col(gam, c) for c in range(3)]
    t += [dot(gam, gam), exc]
    return t if all(finite(x) for x in t) else None


def matrix7(ba):
    M = [[0.0] * 7 for _ in range(7)]
    M[0][0] = ba[0]
    for c in range(3):
        M[0][1 + c] = M[1 + c][0] = ba[1 + c]
        M[1 + c][1 + c] = ba[4]
        M[0][4 + c] = M[4 + c][0] = ba[5 + c]
        for r in range(3):
            M[1 + r][4 + c] = M[4 + c][1 + r] = ba[8 + 3 * r + c]
    k = 17
    for a in range(3):
        for b in range(a, 3):
            M[4 + a][4 + b] = M[4 + b][4 + a] = ba[k]
            k += 1
    return M, list(ba[23:30])


def refine7(M, r, g_lin, s_lin, dba_lin, G, iters, rel, ratios=None):
    """the rounds on the tangent plane with the bias columns: (ok, s, gh, dba)"""
    n, gh = normalise(g_lin)
    if not (finite(n) and n > 0.0):
        return False, 1.0, [0.0] * 3, [0.0] * 3
    s, dba = s_lin, list(dba_lin)
    for _ in range(iters):
        k = 0
        for j in (1, 2):
            if abs(gh[j]) < abs(gh[k]):
                k = j
        d = [(1.0 if j == k else 0.0) - gh[k] * gh[j] for j in range(3)]
        _, b1 = normalise(d)
        b2 = [gh[1] * b1[2] - gh[2] * b1[1], gh[2] * b1[0] - gh[0] * b1[2], gh[0] * b1[1] - gh[1] * b1[0]]
        x0 = [G * gh[j] for j in range(3)]
        rr = [r[i] - ((M[i][1] * x0[0] + M[i][2] * x0[1]) + M[i][3] * x0[2]) for i in range(7)]
        q = [rr[0], dot(b1, rr[1:4]), dot(b2, rr[1:4]), rr[4], rr[5], rr[6]]
        w1 = [dot(M[1 + i][1:4], b1) for i in range(3)]
        w2 = [dot(M[1 + i][1:4], b2) for i in range(3)]
        N = [[0.0] * 6 for _ in range(6)]
        N[0][0] = M[0][0]
        N[0][1] = N[1][0] = dot(M[0][1:4], b1)
        N[0][2] = N[2][0] = dot(M[0][1:4], b2)
        N[1][1], N[2][2] = dot(b1, w1), dot(b2, w2)
        N[1][2] = N[2][1] = dot(b1, w2)
        for c in range(3):
            N[0][3 + c] = N[3 + c][0] = M[0][4 + c]
            col = [M[1][4 + c], M[2][4 + c], M[3][4 + c]]
            N[1][3 + c] = N[3 + c][1] = dot(b1, col)
            N[2][3 + c] = N[3 + c][2] = dot(b2, col)
            for a in range(3):
                N[3 + a][3 + c] = M[4 + a][4 + c]
        ok, y, D = ldl_rel(N, q, 6, rel)
        if ratios is not None:
            ratios.append([div(D[j], N[j][j]) if N[j][j] != 0.0 else 0.0 for j in range(6)])
        if not ok:
            return False, 1.0, [0.0] * 3, [0.0] * 3
        g = [(x0[j] + y[1] * b1[j]) + y[2] * b2[j] for j in range(3)]
        n, gh = normalise(g)
        if not (finite(n) and n > 0.0 and all(finite(x) for x in gh)):
            return False, 1.0, [0.0] * 3, [0.0] * 3
        s, dba = y[0], y[3:6]
    return True, s, gh, dba


def ba_carry(carry4=None):
    """a BA_CARRY record around a vi_align_ref CARRY record (None: zero): no bias sums, a last_jac that is not usable"""
    c = np.zeros(1, BA_CARRY_DTYPE)
    if carry4 is not None:
        c[0]["carry"] = np.asarray(carry4, vr.CARRY_DTYPE).reshape(-1)[0]
    c[0]["last_jac"]["flags"] = IMU_JAC_NONFINITE
    return c


def align_ba_rows(P, BP, prev, traj, delta, jac, carry=None, want_carry=True, detail=None):
    """(states (n) STATE_DTYPE, the BA_RESULT_DTYPE record, the BA_CARRY_DTYPE record) of vis_vi_align_ba_rows.  detail: a dict that receives "ba" (the
    summed absolute terms of the call), "ratios7" (D[j] / M7[j][j]) and "ratios6" (the same of every refinement round)"""
    n = len(prev)
    traj, delta, jac = np.asarray(traj, vr.TRAJ_DTYPE), np.asarray(delta, ir.DELTA_DTYPE), np.asarray(jac, JAC_DTYPE)
    full = None if carry is None else np.asarray(carry, BA_CARRY_DTYPE).reshape(-1)[0]
    inner = None if full is None else full["carry"]
    st4, res4, carry4 = vr.align_rows(P, prev, traj, delta, inner, want_carry)
    c_in, _ = vr.carry_parts(inner)
    ba_flags = 0
    c_ba = None                                                       # the bias part of a carry that counts, when it is finite
    if c_in is not None:
        nums = list(full["ba"]) + [x for f in ("Jvg", "Jva", "Jpg", "Jpa") for x in full["last_jac"][f]]
        if all(finite(float(x)) for x in nums):
            c_ba = full
        else:
            ba_flags |= VIAB_BAD_CARRY
    S, E = int(res4["segment_seq"]), int(res4["epoch_seq"])
    c_last = vr.tail_from_record(c_in["last"]) if c_in is not None else Tail()
    c_parent = vr.tail_from_record(c_in["parent"]) if c_in is not None else Tail()
    c_delta = vr.delta_of(c_in["last_delta"]) if c_in is not None else None
    c_jac_ok = c_ba is not None and jac_usable(c_ba["last_jac"], int(c_in["last_delta"]["q"]))
    q = [norm_prev(prev, i) for i in range(n)]
    tails = [vr.tail_of(P, traj[i], q[i]) for i in range(n)]
    usable = [vr.delta_usable(P, delta[i], int(traj[i]["parent"])) for i in range(n)]
    dl = [vr.delta_of(delta[i]) for i in range(n)]
    jok = [jac_usable(jac[i], int(delta[i]["q"])) for i in range(n)]

    def parent_of(i):
        """(tail, delta, delta usable, Jacobian record, Jacobian usable) of the parent of frame i"""
        if q[i] >= 0:
            return tails[q[i]], dl[q[i]], usable[q[i]], jac[q[i]], jok[q[i]]
        if q[i] == KF_CARRIED:
            return c_last, c_delta, bool(c_last.flags & VIT_DELTA), c_ba["last_jac"] if c_ba is not None else None, c_jac_ok
        return Tail(), None, False, None, False

    def grandparent_of(i):
        if q[i] >= 0:
            return parent_of(q[i])[0]
        return c_parent if q[i] == KF_CARRIED else Tail()

    # ---- the terms of the bias triples
    terms, parts = np.zeros((n, N_BA)), [None] * n
    for i in range(n):
        tc = tails[i]
        tb, db, ub, jb, jb_ok = parent_of(i)
        ta = grandparent_of(i)
        if not (tc.flags & VIT_EDGE and tb.flags & VIT_EDGE and ta.flags & VIT_POSED and usable[i] and ub and (tc.seg, tc.epoch) == (S, E)
                and (tb.seg, tb.epoch) == (S, E)):
            continue
        lam, beta, gam, exc = vr.triple_parts(ta, tb, tc, db, dl[i])
        if vr.linear_terms(lam, beta, gam, exc) is None or not (jok[i] and jb_ok):
            continue
        Jva_b, Jpa_b = jac_blocks(jb)
        nB = neg_b(ta, tb, jac_blocks(jac[i])[1], Jpa_b, Jva_b, db.dt, dl[i].dt)
        t = ba_terms(lam, beta, gam, exc, nB)
        if t is not None:
            terms[i], parts[i] = t, (lam, beta, gam, nB)
    call = tiled_sums(terms) if n else [0.0] * N_BA
    nb_call = sum(p is not None for p in parts)
    if detail is not None:
        detail["ba"] = np.abs(terms).sum(0)

    # ---- the totals
    ba, n_ba = list(call), nb_call
    if c_ba is not None and (int(c_in["segment_seq"]), int(c_in["epoch_seq"])) == (S, E):
        ba = [float(c_ba["ba"][k]) + call[k] for k in range(N_BA)]
        n_ba = int(c_ba["n_ba_triples"]) + nb_call
    if not all(finite(x) for x in ba):
        ba, n_ba, ba_flags = [0.0] * N_BA, 0, ba_flags | VIAB_UNOBSERVABLE

    # ---- the solves
    s4, g4 = float(res4["s"]), [float(x) for x in res4["g"]]
    s_ba, g_ba, dba = s4, g4, [0.0] * 3
    s_lin7, g_lin7, dba_lin, g7_norm = 0.0, [0.0] * 3, [0.0] * 3, 0.0
    if n_ba < BP.min_ba_triples:
        ba_flags |= VIAB_FEW
    else:
        M, r = matrix7(ba)
        ok, x, D = ldl_rel(M, r, 7, BP.pivot_rel)
        if detail is not None:
            detail["ratios7"] = [div(D[j], M[j][j]) if M[j][j] != 0.0 else 0.0 for j in range(7)]
            detail["ratios6"] = []
        gn = math.sqrt(dot(x[1:4], x[1:4]))
        if not ok or not ba[0] > vr.EXCITATION_REL * ba[31] or not finite(gn):
            ba_flags |= VIAB_UNOBSERVABLE
        else:
            s_lin7, g_lin7, dba_lin, g7_norm = x[0], x[1:4], x[4:7], gn
            if not s_lin7 > 0.0:
                ba_flags |= VIAB_SCALE
            else:
                ok, s3, gh, d3 = refine7(M, r, g_lin7, s_lin7, dba_lin, P.G, P.refine_iters, BP.pivot_rel,
                                         detail["ratios6"] if detail is not None else None)
                g3 = [P.G * gh[k] for k in range(3)]
                if not ok or not all(finite(v) for v in g3 + d3):
                    ba_flags |= VIAB_UNOBSERVABLE
                elif not (finite(s3) and s3 > 0.0):
                    ba_flags |= VIAB_SCALE
                else:
                    s_ba, g_ba, dba = s3, g3, d3
    ba_ok = not ba_flags & VIAB_FAILED

    # ---- the states: vi_align_ref's on a fallback, else under (s_ba, g_ba, dba)
    states = st4.copy()
    rr_terms = np.zeros((n, 1))
    if ba_ok:
        for i in range(n):
            st = states[i]
            f = int(st4[i]["flags"]) & (vr.VIS_HAS_PAIR)
            st["p"], st["v"], st["res"] = 0.0, 0.0, 0.0
            tc = tails[i]
            tb = parent_of(i)[0]
            in_se = bool(tc.flags & VIT_POSED) and (tc.seg, tc.epoch) == (S, E)
            pc = [s_ba * tc.C[r] + tc.L[r] for r in range(3)]
            if in_se and all(finite(x) for x in pc):
                st["p"], f = pc, f | vr.VIS_HAS_P
            if in_se and tc.flags & VIT_EDGE and usable[i] and tb.flags & VIT_POSED and tb.seg == S and jok[i]:
                d = dl[i]
                Jva, Jpa = jac_blocks(jac[i])
                ev, ep = mulv(Jva, dba), mulv(Jpa, dba)
                dv, dp = [d.v[k] + ev[k] for k in range(3)], [d.p[k] + ep[k] for k in range(3)]
                pb = [s_ba * tb.C[r] + tb.L[r] for r in range(3)]
                w = mulv(tb.Rw, [dv[k] - div(dp[k], d.dt) for k in range(3)])
                v = [(div(pc[r] - pb[r], d.dt) + (0.5 * g_ba[r]) * d.dt) + w[r] for r in range(3)]
                if all(finite(x) for x in v):
                    st["v"], f = v, f | vr.VIS_HAS_V
            if parts[i] is not None:
                f |= vr.VIS_HAS_TRIPLE
                lam, beta, gam, nB = parts[i]
                Bd = mulv(nB, dba)
                rho = [((lam[r] * s_ba + beta * g_ba[r]) + Bd[r]) - gam[r] for r in range(3)]
                rr = dot(rho, rho)
                if finite(rr):
                    rr_terms[i][0] = rr
                    st["res"] = math.sqrt(rr)
            st["flags"] = f
    sum_rr = tiled_sums(rr_terms)[0] if n else 0.0

    res = np.zeros(1, BA_RESULT_DTYPE)[0]
    res["a"] = res4
    res["dba"], res["s_ba"], res["g_ba"], res["dba_lin"], res["s_lin7"], res["g_lin7"], res["g_lin7_norm"] = dba, s_ba, g_ba, dba_lin, s_lin7, g_lin7, g7_norm
    res["rms_ba"] = math.sqrt(sum_rr / nb_call) if ba_ok and nb_call > 0 and finite(sum_rr) else 0.0
    res["n_ba_triples"], res["n_ba_triples_call"], res["ba_flags"] = n_ba, nb_call, ba_flags

    out = np.zeros(1, BA_CARRY_DTYPE)
    if want_carry:
        o = out[0]
        o["carry"], o["ba"], o["n_ba_triples"] = carry4[0], ba, n_ba
        o["last_jac"]["flags"] = IMU_JAC_NONFINITE
        saved = [i for i in range(n) if q[i] != KF_NOT_SAVED]
        if saved:
            i = saved[-1]
            if usable[i] and jok[i]:
                o["last_jac"] = jac[i]
        elif c_ba is not None:
            o["last_jac"] = c_ba["last_jac"]
    return states, res, out
