"""The inertial factor of include/vislam_hip.h ("THE INERTIAL FACTOR") restated operation for operation in plain Python floats, on top of
tests/vi_align_ref.py (tails, usable deltas, LDL^T, the rotation error) and tests/imu_cov_ref.py (the covariance record).  vis_imu_factor_rows
equals factor_rows() byte for byte."""
import numpy as np

import imu_cov_ref as cr
import imu_ref as ir
import vi_align_ref as vr

IMF_OK, IMF_NO_PARENT, IMF_NO_STATE, IMF_NO_ALIGN, IMF_UNUSABLE, IMF_SINGULAR, IMF_NONFINITE = 0, 1, 2, 4, 8, 16, 32
FACTOR_DTYPE = np.dtype([("r", "<f8", (9,)), ("chi2", "<f8"), ("chi2_rot", "<f8"), ("flags", "<i4"), ("q", "<i4")])
FACTOR_PARAMS_DTYPE = np.dtype([("var_rot", "<f8"), ("var_v", "<f8"), ("var_p", "<f8")])


class FactorParams:
    def __init__(self, var_rot=0.0, var_v=0.0, var_p=0.0):
        self.var_rot, self.var_v, self.var_p = float(var_rot), float(var_v), float(var_p)


def factor_rows(P, FP, prev, traj, delta, cov, state, result):
    """d_factor (n) of vis_imu_factor_rows; P: vi_align_ref.Params, result: one RESULT record (or the head of a BA one)"""
    n = len(prev)
    res = np.asarray(result).reshape(-1)[0]
    g, rflags = [float(x) for x in res["g"]], int(res["flags"])
    out = np.zeros(n, FACTOR_DTYPE)
    need = vr.VIS_HAS_P | vr.VIS_HAS_V
    for i in range(n):
        q = ir.norm_prev(prev, i)
        out[i]["q"] = q
        if q >= 0:
            tc, tb = vr.tail_of(P, traj[i], q), vr.tail_of(P, traj[q], ir.norm_prev(prev, q))
        if q < 0 or not tc.flags & vr.VIT_EDGE or not tb.flags & vr.VIT_POSED:
            out[i]["flags"] = IMF_NO_PARENT
            continue
        fl = 0
        if int(state[i]["flags"]) & need != need or int(state[q]["flags"]) & need != need:
            fl |= IMF_NO_STATE
        if rflags & vr.VIA_FAILED:
            fl |= IMF_NO_ALIGN
        S = [float(x) for x in cov[i]["S"]]
        if not vr.delta_usable(P, delta[i], int(traj[i]["parent"])) or int(cov[i]["flags"]) & cr.IMU_COV_NONFINITE or \
                not all(ir.finite(x) for x in S) or int(cov[i]["q"]) != int(delta[i]["q"]):
            fl |= IMF_UNUSABLE
        if fl:
            out[i]["flags"] = fl
            continue
        d = vr.delta_of(delta[i])
        dt = d.dt
        pi, vi = [float(x) for x in state[i]["p"]], [float(x) for x in state[i]["v"]]
        pb, vb = [float(x) for x in state[q]["p"]], [float(x) for x in state[q]["v"]]
        r = vr.rot_error(d.R, ir.tmul(tb.Rw, tc.Rw))
        x = vr.tmulv(tb.Rw, [(vi[k] - vb[k]) - g[k] * dt for k in range(3)])
        r += [x[k] - d.v[k] for k in range(3)]
        x = vr.tmulv(tb.Rw, [((pi[k] - pb[k]) - vb[k] * dt) - (0.5 * g[k]) * (dt * dt) for k in range(3)])
        r += [x[k] - d.p[k] for k in range(3)]
        if not all(ir.finite(v) for v in r):
            out[i]["flags"] = IMF_NONFINITE
            continue
        var = (FP.var_rot, FP.var_v, FP.var_p)
        A = [[0.0] * 9 for _ in range(9)]
        for a in range(9):
            for b in range(a + 1):
                s = S[cr.idx9(b, a)]
                A[a][b] = A[b][a] = s + var[a // 3] if a == b else s
        ok9, y = vr.ldl(A, r, 9)
        ok3, y3 = vr.ldl([row[:3] for row in A[:3]], r[:3], 3)
        if not ok9 or not ok3:
            out[i]["flags"] = IMF_SINGULAR
            continue
        c9 = r[0] * y[0]
        for k in range(1, 9):
            c9 = c9 + r[k] * y[k]
        c3 = (r[0] * y3[0] + r[1] * y3[1]) + r[2] * y3[2]
        if not ir.finite(c9) or not ir.finite(c3):
            out[i]["flags"] = IMF_NONFINITE
            continue
        out[i]["r"], out[i]["chi2"], out[i]["chi2_rot"] = r, c9, c3
    return out
