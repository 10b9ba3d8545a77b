"""The one case generator of the IMU preintegration tests (CPU: test_imu_ref.py; GPU: test_imu_gpu.py, test_imu_stream_gpu.py): a smooth body
motion sampled at a chosen rate, frame times that fall between samples, the pairings, carried records, non-trivial parameters and the hostile rows."""
import math

import numpy as np

import imu_ref as ir

NS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024)
PAIRINGS = ("chain", "alternate", "long", "straddle")
PAIR_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1020, 1023)
FPS = 20.0
T0 = 100.0                                                           # seconds: times are not small numbers, as on a real stream


def body_rate(t):
    """a smooth time-varying body rate (rad/s) and specific force (m/s^2)"""
    w = [0.6 * math.sin(1.3 * t) + 0.2, 0.5 * math.cos(0.9 * t + 0.4), 0.4 * math.sin(2.1 * t + 1.0) - 0.1]
    a = [0.8 * math.cos(1.7 * t), 9.81 + 0.5 * math.sin(0.7 * t), 0.3 * math.sin(1.1 * t + 0.3)]
    return w, a


def samples_between(t_a, t_b, hz, rate=body_rate, phase=0.0):
    """samples at t_a + (k + phase) / hz up to t_b"""
    m = int(math.floor((t_b - t_a) * hz - phase)) + 1
    s = np.zeros(max(m, 0), ir.SAMPLE_DTYPE)
    for k in range(len(s)):
        t = t_a + (k + phase) / hz
        s[k]["t"] = t
        s[k]["w"], s[k]["a"] = rate(t)
    return s


def stream(n, per_interval, fps=FPS, rate=body_rate):
    """(samples, tframe, t_before): n frame times between samples, `per_interval` samples in a frame interval (0: one in about three intervals),
    samples from before t_before, the time a carry would hold, to after the last frame"""
    hz = fps * per_interval if per_interval > 0 else fps / 3.0
    t_before = T0 + 0.37 / fps
    tframe = np.asarray([t_before + (i + 1) / fps for i in range(n)], np.float64)
    return samples_between(T0, float(tframe[-1]) + 2.0 / hz, hz, rate, phase=0.11), tframe, t_before


def pairing(name, n, first=ir.KF_FIRST):
    """prev[] of n frames.  chain: i - 1; alternate: every second frame fails the gate; long: frame 0, n - 2 unsaved frames and a saved last frame
    (pair length n - 1); straddle: frame i pairs with the frame L back, L walking over the lengths around the powers of two that fit"""
    prev = np.zeros(n, np.int32)
    prev[0] = first
    if name == "chain":
        prev[1:] = np.arange(n - 1)
    elif name == "alternate":
        for i in range(1, n):
            prev[i] = ir.KF_NOT_SAVED if i & 1 else i - 2
    elif name == "long":
        prev[1:] = ir.KF_NOT_SAVED
        if n > 1:
            prev[n - 1] = 0
    elif name == "straddle":
        lens = sorted({max(1, (1 << k) + d) for k in range(11) for d in (-1, 0, 1)})
        for i in range(1, n):
            fit = [L for L in lens if L <= i]
            prev[i] = i - fit[(i * 7) % len(fit)] if i % 5 else i - fit[-1]
    else:
        raise ValueError(name)
    return prev


def params():
    """non-trivial biases and an IMU-to-camera rotation that is no axis permutation"""
    R = ir.exp_and_jr([0.3, -0.5, 0.8])[0]
    return ir.Params(bg=(0.01, -0.02, 0.005), ba=(0.1, -0.05, 0.2), r_ic=R)


def carried(t_last, with_open=True):
    """a carry record: the time of the last frame of the call before and, with_open, a delta from an earlier saved frame to it"""
    c = np.zeros(1, ir.CARRY_DTYPE)
    c[0]["t_last"], c[0]["valid"] = t_last, ir.IMU_CARRY_TIME | (ir.IMU_CARRY_OPEN if with_open else 0)
    c[0]["open"]["R"] = ir.EYE
    if with_open:
        s = samples_between(t_last - 0.3, t_last + 0.1, 200.0)
        d = ir.preintegrate(params(), s, t_last - 0.21, t_last)[0]
        c[0]["open"] = d
        c[0]["open"]["q"] = 0
    return c


def struct_params(vislam, P):
    ip = vislam.default_imu_params()
    for k in range(3):
        ip.bg[k], ip.ba[k] = P.bg[k], P.ba[k]
    for k in range(9):
        ip.r_ic[k] = P.r_ic[k]
    ip.max_gap_s, ip.max_angle = P.max_gap_s, P.max_angle
    return ip


def hostile():
    """(name, samples, tframe, prev, carry, {frame: flags that must be set}, {frame: flags that must not be set}).  Every number of every record
    must be finite whatever the row holds."""
    out = []
    nan, inf, big = float("nan"), float("inf"), 3e38
    chain = lambda n: pairing("chain", n, ir.KF_CARRIED)
    base, tf, tb = stream(6, 10)
    for name, val in (("nan", nan), ("+inf", inf), ("-inf", -inf), ("+3e38", big), ("-3e38", -big)):
        for field in ("w", "a", "t"):
            if field == "t" and val in (big, -big):
                continue                                              # (a finite time out of order is the next case)
            s = base.copy()
            j = int(np.searchsorted(s["t"], tf[2])) + 3              # a sample strictly inside interval 3
            if field == "t":
                s[j]["t"] = val
            else:
                s[j][field][1] = val
            want = ir.IMU_NONFINITE if field == "t" or not math.isfinite(val) or field == "w" else 0
            # (a time that is not finite leaves the array unsorted: where the searches of the OTHER intervals land is defined, and not asserted here)
            clean = {} if field == "t" else {1: ir.IMU_NONFINITE, 5: ir.IMU_NONFINITE}
            out.append((f"{field}={name}", s, tf, chain(6), carried(tb, False), {3: want}, clean))
    s = base.copy()
    j = int(np.searchsorted(s["t"], tf[1])) + 2
    s[j + 1]["t"] = s[j]["t"]                                         # equal sample times
    s[j + 3]["t"] = s[j + 2]["t"] - 0.001                             # a falling sample time
    out.append(("equal and falling sample times", s, tf, chain(6), carried(tb, False), {2: ir.IMU_ORDER}, {4: ir.IMU_ORDER}))
    t2 = tf.copy()
    t2[3] = t2[2]                                                     # frames with equal time stamps
    out.append(("equal frame times", base, t2, chain(6), carried(tb, False), {3: ir.IMU_ORDER | ir.IMU_EMPTY}, {2: ir.IMU_ORDER}))
    t3 = tf.copy()
    t3[3] = t3[2] - 0.01                                              # a falling frame time
    out.append(("falling frame times", base, t3, chain(6), carried(tb, False), {3: ir.IMU_ORDER}, {2: ir.IMU_ORDER}))
    # 0, 1 and 2 samples inside an interval; frame times equal to a sample time at both ends
    s = samples_between(T0, T0 + 1.0, 40.0)                           # 25 ms apart
    ts = s["t"]
    t4 = np.asarray([ts[4], ts[4] + 0.010, ts[5] + 0.001, ts[7] + 0.001, ts[9], ts[12]], np.float64)
    out.append(("0, 1, 2 samples and frame times on samples", s, t4, chain(6), carried(float(ts[2]), False),
                {1: ir.IMU_EMPTY}, {0: ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED, 2: ir.IMU_EMPTY, 3: ir.IMU_EMPTY, 4: ir.IMU_EMPTY, 5: ir.IMU_EXTRAPOLATED}))
    # frame times before the first and after the last sample
    t5 = np.asarray([ts[0] - 0.02, ts[0] - 0.01, ts[1] + 0.001, ts[-1] - 0.001, ts[-1] + 0.01, ts[-1] + 0.02], np.float64)
    out.append(("frames outside the samples", s, t5, chain(6), carried(float(ts[0]) - 0.03, False),
                {0: ir.IMU_EXTRAPOLATED | ir.IMU_EMPTY, 1: ir.IMU_EXTRAPOLATED, 2: ir.IMU_EXTRAPOLATED, 4: ir.IMU_EXTRAPOLATED, 5: ir.IMU_EXTRAPOLATED | ir.IMU_EMPTY},
                {3: ir.IMU_EXTRAPOLATED}))
    out.append(("a last sample at the frame time is no extrapolation", s, np.asarray([ts[-3], ts[-1]], np.float64), chain(2), carried(float(ts[-5]), False),
                {}, {0: ir.IMU_EXTRAPOLATED, 1: ir.IMU_EXTRAPOLATED}))
    out.append(("no samples at all", s[:0], tf, chain(6), carried(tb, False), {i: ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED for i in range(6)}, {}))
    # a gap above max_gap_s (default 0.05 s): samples 25 ms apart with three taken out
    g = np.concatenate([s[:10], s[13:]])
    t6 = np.asarray([g["t"][8] + 0.001, g["t"][9] + 0.001, g["t"][10] + 0.001, g["t"][12] + 0.001], np.float64)
    out.append(("a gap", g, t6, chain(4), carried(float(g["t"][6]), False), {2: ir.IMU_GAP}, {0: ir.IMU_GAP, 1: ir.IMU_GAP, 3: ir.IMU_GAP}))
    # a rate above max_angle (default 1 rad a sub-step): 60 rad/s over 25 ms is 1.5 rad
    f = s.copy()
    f["w"][7:9, 2] = 60.0
    t7 = np.asarray([ts[5] + 0.001, ts[9] + 0.001, ts[14] + 0.001], np.float64)
    out.append(("a fast rotation", f, t7, chain(3), carried(float(ts[3]), False), {1: ir.IMU_FAST}, {0: ir.IMU_FAST, 2: ir.IMU_FAST}))
    # a carried record that holds a NaN and an infinity
    c = carried(tb, True)
    c[0]["open"]["v"][1], c[0]["open"]["R"][4] = nan, inf
    out.append(("a hostile carry", base, tf, chain(6), c, {0: ir.IMU_NONFINITE}, {1: ir.IMU_NONFINITE}))
    c = carried(nan, False)
    out.append(("a carried time that is NaN", base, tf, chain(6), c, {0: ir.IMU_NONFINITE}, {1: ir.IMU_NONFINITE}))
    return out


def all_finite(delta, rot, carry=None):
    recs = [delta] + ([carry["open"]] if carry is not None else [])
    return all(np.isfinite(r[f]).all() for r in recs for f in ("R", "v", "p", "dt", "JRg")) and np.isfinite(rot).all() and \
        (carry is None or np.isfinite(carry["t_last"]).all())
