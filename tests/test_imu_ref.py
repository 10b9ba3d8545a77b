"""CPU: the restatement tests/imu_ref.py against an independent numpy model -- Rodrigues' formula with np.sin / np.cos, 5 x 5 matrix composition
of (R, v, p, dt) -- and against itself in another order.

Measured on the restatement (printed by every run, asserted at 16 x):
  constant body rate, 1.6 s at 200 Hz, frame times between samples: max |R - Exp(w T)| = 6.6e-15 (CONSTANT_RATE_ERR)
  smooth rate, error of R against a 12.8 kHz integration at 100, 200, 400, 800 Hz: 1.4e-05, 3.4e-06, 8.6e-07, 2.1e-07 -- ratios 4.00, 4.00, 4.01
  lifting table against the left-to-right composition, n = 1024, pair lengths 1 ... 1023: max |dR| = 3.7e-15, relative v 3.3e-15, p 4.0e-15,
  JRg 2.2e-15 (LIFT_ERR); their 16-fold is the bound the cuts of a gated stream are held to (test_imu_stream_gpu.py)
  composition against the direct integration of the same pair at 200 Hz: 6.0e-08 in R, the discretisation difference (a frame time inside a sample gap adds
  a breakpoint), below the scheme's own error at that rate (3.5e-06)"""
import math

import numpy as np
import pytest

import imu_cases as ic
import imu_ref as ir

CONSTANT_RATE_ERR = 6.6e-15
LIFT_ERR = {"R": 3.7e-15, "v": 3.3e-15, "p": 4.0e-15, "JRg": 2.2e-15}
LIFT_BOUND = {k: 16 * v for k, v in LIFT_ERR.items()}


def rodrigues(phi):
    phi = np.asarray(phi, np.float64)
    th = float(np.linalg.norm(phi))
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def log_so3(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    th = math.acos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w * (0.5 if th < 1e-9 else th / (2 * math.sin(th)))


def model_integrate(rate, t_a, t_b, hz, bg=(0, 0, 0), ba=(0, 0, 0)):
    """the independent model: midpoint steps of 1 / hz from t_a to t_b on the analytic rate, 5 x 5 matrices [[R, v, p], [0, 1, dt], [0, 0, 1]]"""
    M = np.eye(5)
    m = int(round((t_b - t_a) * hz))
    h = (t_b - t_a) / m
    bg, ba = np.asarray(bg, np.float64), np.asarray(ba, np.float64)
    for k in range(m):
        t0, t1 = t_a + k * h, t_a + (k + 1) * h
        (w0, a0), (w1, a1) = rate(t0), rate(t1)
        dR = rodrigues((0.5 * (np.asarray(w0) + np.asarray(w1)) - bg) * h)
        am = 0.5 * ((np.asarray(a0) - ba) + dR @ (np.asarray(a1) - ba))
        S = np.eye(5)
        S[:3, :3], S[:3, 3], S[:3, 4], S[3, 4] = dR, am * h, 0.5 * am * h * h, h
        M = M @ S
    return M


def as_matrix(rec):
    M = np.eye(5)
    M[:3, :3], M[:3, 3], M[:3, 4], M[3, 4] = np.asarray(rec["R"]).reshape(3, 3), rec["v"], rec["p"], rec["dt"]
    return M


def test_composition_is_the_5x5_product():
    """(R, v, p, dt) compose like the matrices [[R, v, p], [0, 1, dt], [0, 0, 1]]"""
    s, tf, tb = ic.stream(8, 10)
    d, _, _ = ir.preintegrate_rows(ic.params(), s, tf, ic.pairing("chain", 8, ir.KF_CARRIED), ic.carried(tb, False))
    long, _, _ = ir.preintegrate_rows(ic.params(), s, tf, ic.pairing("long", 8, ir.KF_CARRIED), ic.carried(tb, False))
    M = np.eye(5)
    for i in range(1, 8):
        M = M @ as_matrix(d[i])
    assert np.abs(M - as_matrix(long[7])).max() < 1e-13 and int(long[7]["n_steps"]) == int(d["n_steps"][1:].sum()) and int(long[7]["q"]) == 0


def test_constant_body_rate_is_the_exponential():
    w = np.array([0.4, -0.7, 0.5])
    rate = lambda t: (list(w), [0.0, 9.81, 0.0])
    s = ic.samples_between(ic.T0, ic.T0 + 2.0, 200.0, rate)
    t_a, t_b = ic.T0 + 0.1013, ic.T0 + 0.1013 + 1.6                  # between samples at both ends
    d, _ = ir.preintegrate(ir.Params(), s, t_a, t_b)
    err = np.abs(np.asarray(d["R"]).reshape(3, 3) - rodrigues(w * float(d["dt"]))).max()
    print("constant rate: max |R - Exp(w T)| =", err)
    assert int(d["flags"]) == 0 and int(d["n_steps"]) == 321 and err <= 16 * CONSTANT_RATE_ERR


def test_second_order_in_the_sample_period():
    t_a, t_b = ic.T0 + 0.1013, ic.T0 + 0.1013 + 1.6
    fine = model_integrate(ic.body_rate, t_a, t_b, 12800.0)
    errs = []
    for hz in (100.0, 200.0, 400.0, 800.0):
        s = ic.samples_between(ic.T0, ic.T0 + 2.0, hz, ic.body_rate)
        d, _ = ir.preintegrate(ir.Params(), s, t_a, t_b)
        assert int(d["flags"]) == 0
        errs.append(np.abs(np.asarray(d["R"]).reshape(3, 3) - fine[:3, :3]).max())
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("smooth rate: errors", errs, "ratios", ratios)
    assert all(3.5 <= r <= 4.5 for r in ratios), (errs, ratios)
    # v and p of the independent model at the SAME rate and breakpoints are the restatement's up to rounding
    s = ic.samples_between(t_a, t_b + 0.01, 200.0, ic.body_rate)
    P = ic.params()
    d, _ = ir.preintegrate(P, s, t_a, t_a + 320 / 200.0)
    same = model_integrate(ic.body_rate, t_a, t_a + 320 / 200.0, 200.0, P.bg, P.ba)
    assert np.abs(as_matrix(d) - same).max() < 1e-11, np.abs(as_matrix(d) - same).max()


def test_bias_jacobian_against_a_finite_difference():
    s, tf, tb = ic.stream(4, 10)
    t_a, t_b = tb, float(tf[3])
    P = ic.params()
    d0, _ = ir.preintegrate(P, s, t_a, t_b)
    R0, J, eps = np.asarray(d0["R"]).reshape(3, 3), np.asarray(d0["JRg"]).reshape(3, 3), 1e-6
    for k in range(3):
        Q = ic.params()
        Q.bg[k] += eps
        d1, _ = ir.preintegrate(Q, s, t_a, t_b)
        fd = log_so3(R0.T @ np.asarray(d1["R"]).reshape(3, 3)) / eps
        assert np.abs(fd - J[:, k]).max() <= 1e-5 * np.abs(J[:, k]).max(), (k, fd, J[:, k])


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.fixture(scope="module")
def big_stream():
    s, tf, tb = ic.stream(1024, 2)
    P = ic.params()
    return P, ir.intervals(P, s, tf, ic.carried(tb, False))


def test_lifting_table_against_left_to_right(big_stream):
    P, T0 = big_stream
    T = ir.lifting_table(T0, 1024)
    worst = dict.fromkeys(LIFT_ERR, 0.0)
    for L in ic.PAIR_LENGTHS + (1024,):
        for i in sorted({L - 1, min(1023, L + 5), 1023}):
            if L > i + 1:
                continue
            a, b = ir.lift(T, i, L), ir.sequential(T0, i, L)
            assert a.n_steps == b.n_steps and a.flags == b.flags == 0 and a.dt == pytest.approx(b.dt, rel=1e-14)
            worst["R"] = max(worst["R"], float(np.abs(np.asarray(a.R) - np.asarray(b.R)).max()))
            for f, x, y in (("v", a.v, b.v), ("p", a.p, b.p), ("JRg", a.J, b.J)):
                worst[f] = max(worst[f], _rel(x, y))
            if L == 1:
                assert a.numbers() == b.numbers()
    print("lifting against left to right:", worst)
    assert all(worst[f] <= LIFT_BOUND[f] for f in worst), worst


@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_rows_in_both_orders(n, name):
    """every test stream: the records of the lifting table and of the left-to-right composition agree within the bound, integers and flags equal"""
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        a, ra, ca = ir.preintegrate_rows(ic.params(), s, tf, prev, carry)
        b, rb, cb = ir.preintegrate_rows(ic.params(), s, tf, prev, carry, gather=ir.sequential)
        for f in ("n_steps", "flags", "q"):
            assert (a[f] == b[f]).all() and ca["open"][f] == cb["open"][f]
        assert ca["valid"] == cb["valid"] and ca["t_last"] == cb["t_last"] == tf[-1]
        for x, y in ((a, b), (ca["open"], cb["open"])):
            assert np.abs(x["R"] - y["R"]).max() <= LIFT_BOUND["R"]
            for f in ("v", "p", "JRg"):
                assert _rel(x[f], y[f]) <= LIFT_BOUND[f] or np.abs(y[f]).max() == 0
        assert np.abs(ra.astype(np.float64) - rb).max() <= 2.0 ** -23 and ic.all_finite(a, ra, ca)
        if name == "chain":                                           # L = 1 everywhere: the interval itself, in either order
            assert a[1:].tobytes() == b[1:].tobytes()
            assert int(ca["valid"][0]) == ir.IMU_CARRY_TIME and int(ca["open"]["n_steps"][0]) == 0
        if name == "long" and n > 2:
            assert int(a[n - 1]["q"]) == 0 and int(a[n - 1]["n_steps"]) == int(ir.preintegrate_rows(ic.params(), s, tf, ic.pairing("chain", n), None)[0]["n_steps"][1:].sum())
        want0 = ir.IMU_NO_PAIR if carry is None else 0
        assert int(a[0]["flags"]) == want0


def test_carried_pairs_and_the_carry_record():
    s, tf, tb = ic.stream(6, 10)
    P = ic.params()
    chain = ic.pairing("chain", 6, ir.KF_CARRIED)
    d, rot, _ = ir.preintegrate_rows(P, s, tf, chain, None)
    assert int(d[0]["flags"]) == ir.IMU_NO_CARRY and (rot[0] == np.eye(3, dtype=np.float32).reshape(9)).all() and float(d[0]["dt"]) == 0.0
    none = np.zeros(1, ir.CARRY_DTYPE)                                 # a record without IMU_CARRY_TIME counts as none
    assert ir.preintegrate_rows(P, s, tf, chain, none)[0].tobytes() == d.tobytes()
    # cut into two calls, gate off: the same bytes as one call
    whole, wrot, wc = ir.preintegrate_rows(P, s, tf, chain, ic.carried(tb, False))
    a, arot, ac = ir.preintegrate_rows(P, s, tf[:2], chain[:2], ic.carried(tb, False))
    b, brot, bc = ir.preintegrate_rows(P, s, tf[2:], ic.pairing("chain", 4, ir.KF_CARRIED), ac)
    assert whole[:2].tobytes() == a.tobytes() and whole[2:]["R"].tobytes() == b["R"].tobytes() and wrot.tobytes() == arot.tobytes() + brot.tobytes()
    for f in ("v", "p", "dt", "JRg", "n_steps", "flags"):
        assert whole[2:][f].tobytes() == b[f].tobytes(), f
    assert bc.tobytes() == wc.tobytes()
    # nothing saved in a call: the open delta grows through it
    unsaved = np.full(3, ir.KF_NOT_SAVED, np.int32)
    _, _, c1 = ir.preintegrate_rows(P, s, tf[:3], unsaved, ic.carried(tb, False))
    assert int(c1["valid"][0]) == ir.IMU_CARRY_TIME | ir.IMU_CARRY_OPEN
    late, _, _ = ir.preintegrate_rows(P, s, tf[3:], ic.pairing("chain", 3, ir.KF_CARRIED), c1)
    direct, _, _ = ir.preintegrate_rows(P, s, tf, np.asarray([ir.KF_CARRIED, -2, -2, ir.KF_CARRIED, 3, 4], np.int32), ic.carried(tb, False))
    assert np.abs(late[0]["R"] - direct[3]["R"]).max() <= LIFT_BOUND["R"] and int(late[0]["n_steps"]) == int(direct[3]["n_steps"])
    # without a carried time the open delta of a call that saved nothing says so
    _, _, c2 = ir.preintegrate_rows(P, s, tf[:3], unsaved, None)
    assert int(c2["open"]["flags"][0]) & ir.IMU_NO_START


def test_composition_against_direct_integration():
    """the pair is DEFINED as the composition of its intervals; integrating (t_q, t_i] in one go has fewer breakpoints and differs below the scheme's
    own error at that rate"""
    s, tf, tb = ic.stream(33, 10)                                      # 200 Hz
    P = ir.Params()
    long, _, _ = ir.preintegrate_rows(P, s, tf, ic.pairing("long", 33, ir.KF_FIRST), None)
    direct, _ = ir.preintegrate(P, s, float(tf[0]), float(tf[32]))
    fine = model_integrate(ic.body_rate, float(tf[0]), float(tf[32]), 12800.0)
    diff = np.abs(long[32]["R"] - direct["R"]).max()
    scheme = np.abs(np.asarray(direct["R"]).reshape(3, 3) - fine[:3, :3]).max()
    print("composition against direct integration:", diff, "the scheme's error:", scheme)
    assert 0 < diff < scheme and int(long[32]["n_steps"]) == int(direct["n_steps"]) + 31


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(case):
    name, s, tf, prev, carry, must, must_not = case
    d, rot, c = ir.preintegrate_rows(ir.Params(), s, tf, prev, carry)
    assert ic.all_finite(d, rot, c), name
    for i, f in must.items():
        assert int(d[i]["flags"]) & f == f, (name, i, int(d[i]["flags"]))
    for i, f in must_not.items():
        assert not int(d[i]["flags"]) & f, (name, i, int(d[i]["flags"]))
    for i in range(len(tf)):
        if int(d[i]["flags"]) & ir.IMU_NONFINITE:
            assert d[i]["R"].tolist() == ir.EYE and not d[i]["v"].any() and not d[i]["JRg"].any() and (rot[i] == np.asarray(ir.EYE, np.float32)).all()


def test_exp_series_against_rodrigues_up_to_the_bound():
    """ten terms: the first dropped terms bound the truncation of A and B, th^20 / 21! and th^20 / 22!, which enter an entry of Exp times |phi_k| <= th
    and th^2: below rounding up to 1 rad, 4.6e-14 at 2 rad (measured 2.9e-14).  The rest of the bound is rounding: a few ulps of entries <= 1"""
    rng = np.random.default_rng(7)
    trunc = lambda th: th ** 21 / math.factorial(21) + th ** 22 / math.factorial(22)
    for th, bound in ((1e-9, 8e-16), (0.01, 8e-16), (1.0, 8e-16 + trunc(1.0)), (2.0, 8e-16 + trunc(2.0))):
        for _ in range(20):
            u = rng.normal(size=3)
            phi = list(u / np.linalg.norm(u) * th)
            dR, Jr, th2 = ir.exp_and_jr(phi)
            assert np.abs(np.asarray(dR).reshape(3, 3) - rodrigues(phi)).max() <= bound, th
            # Jr(phi) = integral of Exp(-s phi) over s in [0, 1]: Simpson on 64 panels
            x = np.linspace(0, 1, 129)
            wts = np.ones(129); wts[1:-1:2] = 4; wts[2:-1:2] = 2
            num = sum(wk * rodrigues(-xk * np.asarray(phi)) for wk, xk in zip(wts, x)) / (3 * 128)
            assert np.abs(np.asarray(Jr).reshape(3, 3) - num).max() <= 1e-9 + bound
