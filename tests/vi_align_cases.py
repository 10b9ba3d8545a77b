"""The one case generator of the visual-inertial alignment tests (CPU: test_vi_align_ref.py; GPU: test_vi_align_gpu.py and the stream tests): a planted
motion with closed forms -- a rotation about a fixed axis, sinusoidal positions, a gravity vector that is no axis, a non-trivial IMU-to-camera rotation
and lever arm -- sampled at 200 Hz and framed at 20 frames/s through imu_ref, camera records built from it with a planted scale; the same motion with
closed-form deltas for the large frame counts; the pairings of imu_cases, segment breaks and epoch changes, the carries and the hostile rows."""
import math

import numpy as np

import imu_cases as ic
import imu_ref as ir
import vi_align_ref as vr
from trajectory_ref import TJ_NOT_SAVED, TJ_ROOT, TJ_UNIT_EDGE, TRAJ_DTYPE

NS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1024)
PAIRINGS = ic.PAIRINGS
CARRIES = ("none", "tails", "sums", "foreign")
FPS, HZ, T0 = 20.0, 200.0, 100.0
G = 9.81
GRAVITY = [G * x for x in (0.36, -0.8, 0.48)]                          # norm G, no axis
AXIS = [2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0]
R_IC = ir.exp_and_jr([0.3, -0.5, 0.8])[0]
P_CI = [0.05, -0.03, 0.1]
SCALE = 2.5                                                           # metres per trajectory unit
BIAS = (0.01, -0.02, 0.005)
HEAD = 12                                                             # frames of the call a carry comes from


def theta(t, still=False):
    """(angle, rate); the angle stays inside the ten-term series' range over every stream here (at most 1.9 rad after 52 s)"""
    if still:
        return 0.3, 0.0
    u = t - T0
    return 0.4 * math.sin(0.9 * u) + 0.028 * u, 0.36 * math.cos(0.9 * u) + 0.028


def rw(t, still=False):
    th = theta(t, still)[0]
    return ir.exp_and_jr([a * th for a in AXIS])[0]


def motion(t, still=False):
    """(p, v, acc) of the IMU in the root frame, metres; still: a constant velocity (and, in theta, a constant rotation)"""
    if still:
        return [0.3 * t, -0.2 * t, 0.1 * t], [0.3, -0.2, 0.1], [0.0, 0.0, 0.0]
    w, A, ph = (1.1, 0.7, 1.6), (1.5, 1.0, 0.8), (0.0, 0.5, 1.1)
    p = [A[k] * math.sin(w[k] * t + ph[k]) for k in range(3)]
    v = [A[k] * w[k] * math.cos(w[k] * t + ph[k]) for k in range(3)]
    a = [-A[k] * w[k] * w[k] * math.sin(w[k] * t + ph[k]) for k in range(3)]
    return p, v, a


def body_rate(bias=(0.0, 0.0, 0.0), still=False):
    def rate(t):
        dth = theta(t, still)[1]
        acc = motion(t, still)[2]
        f = ir.tmul(rw(t, still), [acc[0] - GRAVITY[0], 0, 0, acc[1] - GRAVITY[1], 0, 0, acc[2] - GRAVITY[2], 0, 0])
        return [AXIS[k] * dth + bias[k] for k in range(3)], [f[0], f[3], f[6]]
    return rate


def params(**kw):
    return vr.Params(r_ic=R_IC, p_ci=P_CI, G=G, **kw)


def struct_params(vislam, P):
    vp = vislam.default_vi_align_params()
    for k in range(9):
        vp.r_ic[k] = P.r_ic[k]
    for k in range(3):
        vp.p_ci[k] = P.p_ci[k]
    vp.G, vp.g_tol, vp.min_pairs, vp.min_triples, vp.refine_iters, vp.reject = P.G, P.g_tol, P.min_pairs, P.min_triples, P.refine_iters, P.reject
    return vp


def camera_pose(t, still=False):
    """(R, P): the camera rotation x = R X + t of the record and the camera centre in metres"""
    R = ir.tmul(R_IC, ir.tmul(rw(t, still), ir.EYE))                        # R = r_ic^T Rw^T
    L = vr.tmulv(R, P_CI)
    p = motion(t, still)[0]
    return R, [p[k] - L[k] for k in range(3)]


def trajectory(times, prev, seq0=0, carry_from=None, breaks=(), epochs=(), scales=(SCALE, 1.7, 3.1), still=False):
    """TRAJ records of the frames at `times` under the pairing prev.  carry_from: None or the info entry (C, segment, epoch, scale index, P) of the
    frame VIS_KF_CARRIED refers to.  breaks: frames that become roots; epochs: frames whose edge is a unit edge with the next planted scale."""
    n = len(times)
    rec = np.zeros(n, TRAJ_DTYPE)
    info = [None] * n                                                 # (C, segment, epoch, scale index, P)
    for i in range(n):
        q = ir.norm_prev(prev, i)
        if q == ir.KF_NOT_SAVED:
            rec[i]["flags"] = TJ_NOT_SAVED
            continue
        R, P = camera_pose(float(times[i]), still)
        par = info[q] if q >= 0 else (carry_from if q == ir.KF_CARRIED else None)
        r = rec[i]
        if par is None or i in breaks:
            C, seg, epoch, si, fl = [P[k] / scales[0] for k in range(3)], seq0 + i, seq0 + i, 0, TJ_ROOT
            r["hops"], r["unit_edges"] = 0, 0
        else:
            Cp, seg, epoch, si, Pp = par
            fl = 0
            below_root = q >= 0 and bool(int(rec[q]["flags"]) & TJ_ROOT)    # (the carried frame of these scenes is never a root)
            if below_root or i in epochs:
                fl, epoch = TJ_UNIT_EDGE, seq0 + i
                si = si + 1 if i in epochs else si
            C = [Cp[k] + (P[k] - Pp[k]) / scales[si % len(scales)] for k in range(3)]
            r["hops"], r["unit_edges"] = 1, 1
        info[i] = (C, seg, epoch, si, P)
        t = ir.mulv(R, C)
        r["R"], r["t"], r["sigma"] = R, [-x for x in t], 1.0
        r["segment_seq"], r["epoch_seq"], r["parent"], r["flags"] = seg, epoch, q, fl
    return rec, info


def closed_deltas(times, prev, t_before=None, still=False):
    """DELTA records in closed form from the planted motion (exact but for rounding), with a small planted rotation error and a Jacobian of the
    magnitude the integration gives: what the large frame counts use in the place of imu_ref"""
    n = len(times)
    out = np.zeros(n, ir.DELTA_DTYPE)
    for i in range(n):
        q = ir.norm_prev(prev, i)
        out[i]["R"], out[i]["q"] = ir.EYE, q
        ta = float(times[q]) if q >= 0 else (t_before if q == ir.KF_CARRIED else None)
        if ta is None:
            out[i]["flags"] = ir.IMU_NO_CARRY if q == ir.KF_CARRIED else ir.IMU_NO_PAIR
            continue
        tb = float(times[i])
        dt = tb - ta
        Ra, Rb = rw(ta, still), rw(tb, still)
        pa, va, _ = motion(ta, still)
        pb, vb, _ = motion(tb, still)
        dv = vr.tmulv(Ra, [vb[k] - va[k] - GRAVITY[k] * dt for k in range(3)])
        dp = vr.tmulv(Ra, [pb[k] - pa[k] - va[k] * dt - 0.5 * GRAVITY[k] * dt * dt for k in range(3)])
        J = [-dt * x for x in ir.exp_and_jr([0.01 * (i % 7), -0.02, 0.03])[1]]
        err = ir.exp_and_jr(ir.mulv(J, [-b for b in BIAS]))[0]
        out[i]["R"], out[i]["v"], out[i]["p"], out[i]["dt"], out[i]["JRg"] = ir.mul(ir.tmul(Ra, Rb), err), dv, dp, dt, J
        out[i]["n_steps"] = 10
    return out


_cache = {}


def scene(n, pairing="chain", carry="none", integrate=False, bias=(0.0, 0.0, 0.0), still=False, breaks=(), epochs=(), phase=0.11):
    """a call of n frames: dict(P, prev, traj, delta, carry, times, info, truth ...).  integrate: the deltas through imu_ref (else closed forms).
    A carry other than "none" makes frame 0 VIS_KF_CARRIED, continuing a call of HEAD chained frames whose carry-out it is ("tails": its sums
    zeroed; "foreign": its sums under another epoch)."""
    key = (n, pairing, carry, integrate, tuple(bias), still, tuple(breaks), tuple(epochs), phase)
    if key in _cache:
        return _cache[key]
    P = params()
    t_first = T0 + 0.37 / FPS
    head_t = np.asarray([t_first + (i + 1) / FPS for i in range(HEAD)], np.float64)
    times = np.asarray([float(head_t[-1]) + (i + 1) / FPS for i in range(n)], np.float64)
    have = carry != "none"
    prev = ic.pairing(pairing, n, ir.KF_CARRIED if have else ir.KF_FIRST) if n else np.zeros(0, np.int32)
    samples = ic.samples_between(T0, float(times[-1] if n else head_t[-1]) + 2.0 / HZ, HZ, body_rate(bias, still), phase) if integrate else None
    ip = ir.Params()
    c_rec, carry_from = None, None
    if have:
        hprev = ic.pairing("chain", HEAD)
        htraj, hinfo = trajectory(head_t, hprev, 0, still=still)
        if integrate:
            hdelta, _, icarry = ir.preintegrate_rows(ip, samples, head_t, hprev)
        else:
            hdelta, icarry = closed_deltas(head_t, hprev, still=still), None
        _, _, c_rec = vr.align_rows(P, hprev, htraj, hdelta)
        if carry == "tails":
            c_rec[0]["gyro"], c_rec[0]["lin"], c_rec[0]["n_pairs"], c_rec[0]["n_triples"] = 0.0, 0.0, 0, 0
        if carry == "foreign":
            c_rec[0]["epoch_seq"] += 1000
        carry_from = hinfo[-1]
    else:
        icarry = None
    traj, info = trajectory(times, prev, HEAD, carry_from, breaks, epochs, still=still)
    if integrate:
        delta = ir.preintegrate_rows(ip, samples, times, prev, icarry)[0] if n else np.zeros(0, ir.DELTA_DTYPE)
    else:
        delta = closed_deltas(times, prev, float(head_t[-1]) if have else None, still)
    sc = dict(P=P, prev=prev, traj=traj, delta=delta, carry=c_rec, times=times, info=info, samples=samples, head_t=head_t)
    _cache[key] = sc
    return sc


def truth_velocity(t, still=False):
    return motion(t, still)[1]


def hostile():
    """(name, scene fields, result flags that must be set, result flags that must not be set): every number of every record must be finite"""
    out = []
    nan, inf, big = float("nan"), float("inf"), 3e38
    base = scene(24, "chain", "sums")

    def copy(sc=base):
        return dict(sc, traj=sc["traj"].copy(), delta=sc["delta"].copy(), carry=None if sc["carry"] is None else sc["carry"].copy(), prev=sc["prev"].copy())
    for name, val in (("nan", nan), ("+inf", inf), ("-inf", -inf), ("+3e38", big), ("-3e38", -big)):
        for field in ("R", "t"):
            s = copy()
            s["traj"][7][field][1] = val
            out.append((f"traj.{field}={name}", s, 0, vr.VIA_FEW))
        for field in ("R", "v", "p", "dt", "JRg"):
            s = copy()
            if field == "dt":
                s["delta"][9]["dt"] = val
            else:
                s["delta"][9][field][1] = val
            out.append((f"delta.{field}={name}", s, 0, vr.VIA_FEW))
    s = copy()
    s["delta"][5]["dt"] = 0.0
    out.append(("a zero dt", s, 0, vr.VIA_FEW))
    s = copy()
    s["delta"][6]["q"] = 2
    out.append(("a q that is not the record's parent", s, 0, vr.VIA_FEW))
    s = copy()
    s["traj"][6]["parent"] = 3
    out.append(("a parent that is not the pairing's", s, 0, vr.VIA_FEW))
    s = copy()
    s["prev"][:] = ir.KF_NOT_SAVED
    s["traj"][:] = 0
    s["traj"]["flags"] = TJ_NOT_SAVED
    out.append(("no frame saved", s, 0, vr.VIA_RESTART))
    s = copy(scene(24, "chain", "none"))
    s["prev"][:] = ir.KF_NOT_SAVED
    s["traj"][:] = 0
    s["traj"]["flags"] = TJ_NOT_SAVED
    out.append(("no frame saved and no carry", s, vr.VIA_FEW | vr.VIA_GYRO_FEW, 0))
    for f, val in (("gyro", nan), ("lin", inf), ("last", -inf), ("parent", nan), ("last_delta", inf)):
        s = copy()
        if f in ("gyro", "lin"):
            s["carry"][0][f][3] = val
        elif f == "last_delta":
            s["carry"][0][f]["p"][2] = val
        else:
            s["carry"][0][f]["Rw"][4] = val
        out.append((f"carry.{f} not finite", s, vr.VIA_BAD_CARRY, 0))
    s = copy()
    s["carry"][0]["lin"][:] = 3e307
    s["carry"][0]["gyro"][:] = -3e307
    out.append(("a carry at the edge of the range", s, 0, 0))
    s = copy(scene(40, "chain", "none", still=True))
    out.append(("a constant velocity", s, None, 0))                   # singular or GRAVITY_NORM: asserted by the test
    s = copy(scene(40, "alternate", "none", still=True, integrate=True))
    out.append(("a constant velocity, integrated", s, None, 0))
    s = copy(scene(24, "chain", "none"))
    s["traj"]["t"] *= 1e200
    out.append(("huge translations", s, 0, 0))
    return out


def all_finite(states, res, carry=None):
    ok = all(np.isfinite(states[f]).all() for f in ("p", "v", "res"))
    ok = ok and all(np.isfinite(res[f]).all() for f in ("dbg", "c0", "c0_call", "c1", "s", "g", "s_lin", "g_lin", "g_lin_norm", "rms"))
    if carry is not None:
        c = carry[0]
        ok = ok and np.isfinite(c["gyro"]).all() and np.isfinite(c["lin"]).all() and np.isfinite(c["last_delta"]["R"]).all()
        ok = ok and all(np.isfinite(c[t][f]).all() for t in ("last", "parent") for f in ("C", "Rw", "L"))
    return bool(ok)


def localise(sc, a, b):
    """frames a ... b - 1 of a scene as a call of their own: indices below a become VIS_KF_CARRIED where they name the last saved frame before a"""
    prev = sc["prev"]
    before = [i for i in range(a) if ir.norm_prev(prev, i) != ir.KF_NOT_SAVED]
    last = before[-1] if before else None

    def loc(q):
        q = int(q)
        if q >= a or q < 0:
            return q - a if q >= a else q
        return ir.KF_CARRIED if q == last else ir.KF_FIRST
    traj, delta = sc["traj"][a:b].copy(), sc["delta"][a:b].copy()
    traj["parent"] = [loc(q) if not int(f) & TJ_NOT_SAVED else 0 for q, f in zip(traj["parent"], traj["flags"])]
    delta["q"] = [loc(q) for q in delta["q"]]
    return np.asarray([loc(ir.norm_prev(prev, i)) for i in range(a, b)], np.int32), traj, delta


def run_cuts(sc, cuts, align=vr.align_rows):
    """the scene's frames aligned in launches of the given lengths, each continuing the carry of the one before: (states, last result, last carry)"""
    carry, at, states = sc["carry"], 0, []
    for m in cuts:
        prev, traj, delta = localise(sc, at, at + m)
        st, res, carry = align(sc["P"], prev, traj, delta, carry)
        states.append(st)
        at += m
    return np.concatenate(states), res, carry


def sum_differences(co, whole, scale):
    """the largest difference between two carries' sums relative to the summed absolute terms (gyro, lin)"""
    out = []
    for f in ("gyro", "lin"):
        sc_ = np.maximum(np.asarray(scale[f], np.float64), 1e-300)
        out.append(float((np.abs(co[0][f] - whole[0][f]) / sc_).max()))
    return out
