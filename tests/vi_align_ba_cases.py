"""The one case generator of the tests of the alignment with the accelerometer bias (CPU: test_vi_align_ba_ref.py; GPU: test_vi_align_ba_gpu.py and
the stream test): vi_align_cases' planted scene -- its positions, gravity, IMU-to-camera rotation, lever arm and scale -- under a rotation about TWO
axes (its own, composed with a second one), with body rates in closed form and a planted accelerometer bias; the deltas and Jacobians through
imu_jac_ref, or, for the large frame counts, from the closed-form motion (the Jacobians by Simpson's rule on the closed-form rotation); the pairings,
carries, segment breaks, epoch changes and cuts of vi_align_cases; the hostile rows.  axes=1 is vi_align_cases' fixed-axis motion, the unobservable case."""
import math

import numpy as np

import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr
from trajectory_ref import TJ_NOT_SAVED, TJ_ROOT, TJ_UNIT_EDGE, TRAJ_DTYPE

NS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1024)
PAIRINGS = vc.PAIRINGS
CARRIES = ("none", "sums", "foreign")
FPS, HZ, T0, HEAD = vc.FPS, vc.HZ, vc.T0, 24
AXIS2 = [6.0 / 7.0, -2.0 / 7.0, 3.0 / 7.0]
ACC_BIAS = (0.1, -0.05, 0.2)                                           # imu_cases.params()' ba, m/s^2
GYRO_BIAS = vc.BIAS
PHASES = (0.11, 0.61)


def theta2(t):
    """(angle, rate) of the second rotation: at most 0.5 rad, inside the ten-term series' range"""
    u = t - T0
    return 0.5 * math.sin(1.3 * u + 0.4), 0.65 * math.cos(1.3 * u + 0.4)


def rw(t, axes=2):
    R1 = vc.rw(t)
    return ir.mul(R1, ir.exp_and_jr([a * theta2(t)[0] for a in AXIS2])[0]) if axes == 2 else R1


def body_rate(gyro_bias=(0.0, 0.0, 0.0), acc_bias=(0.0, 0.0, 0.0), axes=2):
    """R = R1 R2 with fixed axes: the body rate is R2^T (n1 th1') + n2 th2'"""
    def rate(t):
        w = [a * vc.theta(t)[1] for a in vc.AXIS]
        if axes == 2:
            R2 = ir.exp_and_jr([a * theta2(t)[0] for a in AXIS2])[0]
            w1 = vr.tmulv(R2, w)
            w = [w1[k] + AXIS2[k] * theta2(t)[1] for k in range(3)]
        acc = vc.motion(t)[2]
        f = vr.tmulv(rw(t, axes), [acc[k] - vc.GRAVITY[k] for k in range(3)])
        return [w[k] + gyro_bias[k] for k in range(3)], [f[k] + acc_bias[k] for k in range(3)]
    return rate


def camera_pose(t, axes=2):
    R = ir.tmul(vc.R_IC, ir.tmul(rw(t, axes), ir.EYE))
    L = vr.tmulv(R, vc.P_CI)
    p = vc.motion(t)[0]
    return R, [p[k] - L[k] for k in range(3)]


def trajectory(times, prev, seq0=0, carry_from=None, breaks=(), epochs=(), scales=(vc.SCALE, 1.7, 3.1), axes=2):
    """vi_align_cases.trajectory under this module's rotation"""
    n = len(times)
    rec, info = np.zeros(n, TRAJ_DTYPE), [None] * n
    for i in range(n):
        q = ir.norm_prev(prev, i)
        if q == ir.KF_NOT_SAVED:
            rec[i]["flags"] = TJ_NOT_SAVED
            continue
        R, P = camera_pose(float(times[i]), axes)
        par = info[q] if q >= 0 else (carry_from if q == ir.KF_CARRIED else None)
        r = rec[i]
        if par is None or i in breaks:
            C, seg, epoch, si, fl = [P[k] / scales[0] for k in range(3)], seq0 + i, seq0 + i, 0, TJ_ROOT
        else:
            Cp, seg, epoch, si, Pp = par
            fl = 0
            if (q >= 0 and bool(int(rec[q]["flags"]) & TJ_ROOT)) or i in epochs:
                fl, epoch = TJ_UNIT_EDGE, seq0 + i
                si = si + 1 if i in epochs else si
            C = [Cp[k] + (P[k] - Pp[k]) / scales[si % len(scales)] for k in range(3)]
            r["hops"], r["unit_edges"] = 1, 1
        info[i] = (C, seg, epoch, si, P)
        t = ir.mulv(R, C)
        r["R"], r["t"], r["sigma"] = R, [-x for x in t], 1.0
        r["segment_seq"], r["epoch_seq"], r["parent"], r["flags"] = seg, epoch, q, fl
    return rec, info


def closed_records(times, prev, t_before=None, acc_bias=(0.0, 0.0, 0.0), axes=2, panels=4):
    """DELTA and JAC records from the planted motion, exact but for rounding and the quadrature: dv, dp in closed form; Jva = -int Ra^T R(t) dt and
    Jpa = -int (tb - t) Ra^T R(t) dt by Simpson's rule; a planted accelerometer bias b enters as dv - Jva b, dp - Jpa b"""
    n = len(times)
    out, jac = np.zeros(n, ir.DELTA_DTYPE), np.zeros(n, jr.JAC_DTYPE)
    for i in range(n):
        q = ir.norm_prev(prev, i)
        out[i]["R"], out[i]["q"], jac[i]["q"] = ir.EYE, q, q
        ta = float(times[q]) if q >= 0 else (t_before if q == ir.KF_CARRIED else None)
        if ta is None:
            out[i]["flags"] = ir.IMU_NO_CARRY if q == ir.KF_CARRIED else ir.IMU_NO_PAIR
            continue
        tb = float(times[i])
        dt = tb - ta
        Ra, Rb = rw(ta, axes), rw(tb, axes)
        pa, va, _ = vc.motion(ta)
        pb, vb, _ = vc.motion(tb)
        m = 2 * panels * min(max(1, int(round(dt * FPS))), 8)            # (long pairs: coarser, and still the Jacobian the planted bias enters with)
        Jva, Jpa = np.zeros(9), np.zeros(9)
        for k in range(m + 1):
            t = ta + dt * k / m
            w = (1.0 if k in (0, m) else (4.0 if k & 1 else 2.0)) * dt / (3.0 * m)
            M = np.asarray(ir.tmul(Ra, rw(t, axes)))
            Jva -= w * M
            Jpa -= w * (tb - t) * M
        b = np.asarray(acc_bias, np.float64)
        dv = np.asarray(vr.tmulv(Ra, [vb[k] - va[k] - vc.GRAVITY[k] * dt for k in range(3)])) - Jva.reshape(3, 3) @ b
        dp = np.asarray(vr.tmulv(Ra, [pb[k] - pa[k] - va[k] * dt - 0.5 * vc.GRAVITY[k] * dt * dt for k in range(3)])) - Jpa.reshape(3, 3) @ b
        J = [-dt * x for x in ir.exp_and_jr([0.01 * (i % 7), -0.02, 0.03])[1]]
        err = ir.exp_and_jr(ir.mulv(J, [-x for x in GYRO_BIAS]))[0]
        out[i]["R"], out[i]["v"], out[i]["p"], out[i]["dt"], out[i]["JRg"] = ir.mul(ir.tmul(Ra, Rb), err), dv, dp, dt, J
        out[i]["n_steps"] = 10
        jac[i]["Jva"], jac[i]["Jpa"] = Jva, Jpa
        jac[i]["Jvg"], jac[i]["Jpg"] = 0.3 * dt * Jva, 0.3 * dt * Jpa     # (of the right magnitude; the alignment does not read them)
    return out, jac


_cache = {}


def scene(n, pairing="chain", carry="none", integrate=False, gyro_bias=(0.0, 0.0, 0.0), acc_bias=ACC_BIAS, axes=2, breaks=(), epochs=(), phase=0.11):
    """a call of n frames: dict(P, BP, prev, traj, delta, jac, carry ...), as vi_align_cases.scene.  A carry other than "none" makes frame 0
    VIS_KF_CARRIED, continuing a call of HEAD chained frames whose carry-out it is ("foreign": its sums under another epoch)"""
    key = (n, pairing, carry, integrate, tuple(gyro_bias), tuple(acc_bias), axes, tuple(breaks), tuple(epochs), phase)
    if key in _cache:
        return _cache[key]
    P, BP = vc.params(), br.BaParams()
    t_first = T0 + 0.37 / FPS
    head_t = np.asarray([t_first + (i + 1) / FPS for i in range(HEAD)], np.float64)
    times = np.asarray([float(head_t[-1]) + (i + 1) / FPS for i in range(n)], np.float64)
    have = carry != "none"
    prev = ic.pairing(pairing, n, ir.KF_CARRIED if have else ir.KF_FIRST) if n else np.zeros(0, np.int32)
    samples = None
    if integrate:
        samples = ic.samples_between(T0, float(times[-1] if n else head_t[-1]) + 2.0 / HZ, HZ, body_rate(gyro_bias, acc_bias, axes), phase)
    ip = ir.Params()
    c_rec, carry_from, icarry = None, None, None
    if have:
        hprev = ic.pairing("chain", HEAD)
        htraj, hinfo = trajectory(head_t, hprev, 0, axes=axes)
        if integrate:
            hdelta, hjac, _, icarry = jr.preintegrate_jac_rows(ip, samples, head_t, hprev)
        else:
            hdelta, hjac = closed_records(head_t, hprev, None, acc_bias, axes)
        _, _, c_rec = br.align_ba_rows(P, BP, hprev, htraj, hdelta, hjac)
        if carry == "foreign":
            c_rec[0]["carry"]["epoch_seq"] += 1000
        carry_from = hinfo[-1]
    traj, info = trajectory(times, prev, HEAD, carry_from, breaks, epochs, axes=axes)
    if integrate:
        if n:
            delta, jac = jr.preintegrate_jac_rows(ip, samples, times, prev, icarry)[:2]
        else:
            delta, jac = np.zeros(0, ir.DELTA_DTYPE), np.zeros(0, jr.JAC_DTYPE)
    else:
        delta, jac = closed_records(times, prev, float(head_t[-1]) if have else None, acc_bias, axes)
    sc = dict(P=P, BP=BP, prev=prev, traj=traj, delta=delta, jac=jac, carry=c_rec, times=times, info=info, samples=samples, head_t=head_t)
    _cache[key] = sc
    return sc


def errors(res):
    """(scale, gravity, dba) errors of the 7-unknown result against the planted truth, and (scale, gravity) of the embedded 4-unknown one"""
    g7, g4 = np.asarray(res["g_ba"]) - vc.GRAVITY, np.asarray(res["a"]["g"]) - vc.GRAVITY
    return (abs(float(res["s_ba"]) / vc.SCALE - 1.0), float(np.abs(g7).max()), float(np.abs(np.asarray(res["dba"]) - ACC_BIAS).max()),
            abs(float(res["a"]["s"]) / vc.SCALE - 1.0), float(np.abs(g4).max()))


def run(sc, **kw):
    return br.align_ba_rows(sc["P"], kw.pop("BP", sc["BP"]), sc["prev"], sc["traj"], sc["delta"], sc["jac"], kw.pop("carry", sc["carry"]), **kw)


def localise(sc, a, b):
    """vi_align_cases.localise with the Jacobian rows"""
    prev, traj, delta = vc.localise(sc, a, b)
    jac = sc["jac"][a:b].copy()
    jac["q"] = delta["q"]
    return prev, traj, delta, jac


def run_cuts(sc, cuts, align=None):
    """the scene's frames in launches of the given lengths, each continuing the carry of the one before: (states, last result, last carry)"""
    align = align or (lambda P, BP, prev, traj, delta, jac, carry: br.align_ba_rows(P, BP, prev, traj, delta, jac, carry))
    carry, at, states = sc["carry"], 0, []
    for m in cuts:
        prev, traj, delta, jac = localise(sc, at, at + m)
        st, res, carry = align(sc["P"], sc["BP"], prev, traj, delta, jac, carry)
        states.append(st)
        at += m
    return np.concatenate(states), res, carry


def hostile():
    """(name, scene fields, ba_flags that must be set, ba_flags that must not be set): every number of every record must be finite"""
    out = []
    nan, inf, big = float("nan"), float("inf"), 3e38
    base = scene(40, "chain", "sums")

    def copy(sc=base):
        return dict(sc, traj=sc["traj"].copy(), delta=sc["delta"].copy(), jac=sc["jac"].copy(), carry=None if sc["carry"] is None else sc["carry"].copy(),
                    prev=sc["prev"].copy())
    for name, val in (("nan", nan), ("+inf", inf), ("-inf", -inf), ("+3e38", big), ("-3e38", -big)):
        for field in jr.BLOCKS:
            s = copy()
            s["jac"][9][field][1] = val
            out.append((f"jac.{field}={name}", s, 0, br.VIAB_FEW))
    s = copy()
    s["jac"][9]["flags"] = jr.IMU_JAC_NONFINITE
    out.append(("a flagged Jacobian", s, 0, br.VIAB_FEW))
    s = copy()
    s["jac"][6]["q"] = 2
    out.append(("a jac.q that is not the delta's", s, 0, br.VIAB_FEW))
    s = copy(scene(40, "chain", "none"))
    s["jac"]["flags"] = jr.IMU_JAC_NONFINITE
    out.append(("every Jacobian flagged", s, br.VIAB_FEW, 0))
    for f, val in (("ba", nan), ("ba", inf), ("last_jac", -inf)):
        s = copy()
        if f == "ba":
            s["carry"][0]["ba"][7] = val
        else:
            s["carry"][0]["last_jac"]["Jpa"][4] = val
        out.append((f"carry.{f} = {val}", s, br.VIAB_BAD_CARRY, br.VIAB_FEW))
    s = copy()
    s["carry"][0]["carry"]["lin"][3] = nan
    out.append(("the embedded carry not finite", s, 0, br.VIAB_BAD_CARRY))
    s = copy()
    s["carry"][0]["ba"][:] = 3e307
    out.append(("sums at the edge of the range", s, 0, 0))
    s = copy()
    s["carry"][0]["ba"][:] = 1.7e308
    out.append(("sums past the edge of the range", s, br.VIAB_UNOBSERVABLE, 0))
    s = copy()
    s["jac"]["Jpa"] *= 1e150
    s["jac"]["Jva"] *= 1e150
    out.append(("huge Jacobians", s, None, 0))
    for sc4 in (vc.scene(40, "chain", "none", still=True), vc.scene(40, "alternate", "none", still=True, integrate=True)):
        s = dict(sc4, BP=br.BaParams(), jac=zero_jac(sc4["delta"]))
        out.append(("a constant velocity", s, br.VIAB_UNOBSERVABLE, 0))
    return out


def zero_jac(delta):
    """usable Jacobian records of zero matrices beside the given deltas"""
    jac = np.zeros(len(delta), jr.JAC_DTYPE)
    jac["q"] = delta["q"]
    return jac


def all_finite(states, res, carry=None):
    ok = vc.all_finite(states, res["a"], None if carry is None else carry["carry"])
    ok = ok and all(np.isfinite(res[f]).all() for f in ("dba", "s_ba", "g_ba", "dba_lin", "s_lin7", "g_lin7", "g_lin7_norm", "rms_ba"))
    if carry is not None:
        ok = ok and np.isfinite(carry[0]["ba"]).all() and all(np.isfinite(carry[0]["last_jac"][f]).all() for f in jr.BLOCKS)
    return bool(ok)
