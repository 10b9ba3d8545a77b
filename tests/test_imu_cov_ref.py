"""CPU: the restatement tests/imu_cov_ref.py -- its delta part against imu_ref byte for byte, its covariance against an independent dense numpy
model, its calibration against the sample covariance of noisy integrations, its lifting table against the left-to-right order, the cuts of a
stream, the exact properties (zero densities, scaling by a power of two, no negative eigenvalue), the sticky flag and the hostile rows.

Measured on the restatement (printed by every run; asserted at 4 x, the lifting table at 16 x as in test_imu_ref.py):
  against the dense model (9 x 9 matrices, closed-form Exp and Jr, one recursion over every sub-step of the pair), 200 Hz, ic.params(), relative to
  the largest entry of each block, worst of the six blocks:
    pair of 1 frame 4.3e-16, 8 frames 2.2e-15, 32 frames 3.9e-15 (DENSE_ERR)
  calibration, 1000 noisy integrations (seeds 20242 and 20249), EuRoC densities, noise of standard deviation sigma sqrt(hz) a sample:
    1 frame (11 sub-steps): sample / model standard deviation 0.950 - 1.022 over the nine components, mean chi-square 8.39
    8 frames (88 sub-steps): 0.967 - 1.032, mean chi-square 8.92
    bands: [sqrt((n_steps - 1/2) / n_steps) - 4 / sqrt(2 N), 1 + 4 / sqrt(2 N)] and [9 (n_steps - 1/2) / n_steps - 4 sqrt(18 / N), 9 + 4 sqrt(18 / N)]
  lifting table against the left-to-right composition, n = 1024, every pair length 1 ... 1024 from frame 0 and ic.PAIR_LENGTHS ending at frame 1023,
  relative to the largest entry of each block:
    A 6.4e-15, B 9.3e-15, C 9.5e-15, D 1.3e-14, E 8.3e-15, F 6.6e-15 (LIFT_ERR); their 16-fold bounds the cuts of a gated stream"""
import math

import numpy as np
import pytest

import imu_cases as ic
import imu_cov_ref as cr
import imu_ref as ir

BLOCKS = ("A", "B", "C", "D", "E", "F")
SLICES = {"A": (0, 0), "B": (1, 0), "C": (1, 1), "D": (2, 0), "E": (2, 1), "F": (2, 2)}
DENSE_ERR = {1: 4.3e-16, 8: 2.2e-15, 32: 3.9e-15}
LIFT_ERR = {"A": 6.4e-15, "B": 9.3e-15, "C": 9.5e-15, "D": 1.3e-14, "E": 8.3e-15, "F": 6.6e-15}
LIFT_BOUND = {k: 16 * v for k, v in LIFT_ERR.items()}
CUTS = {"A": [8, 1, 4, 8, 3, 8, 5], "B": [37], "C": [8, 8, 8, 8, 5], "D": [1] * 37}
DRAWS, SEED = 1000, 20241
NOISE = cr.Noise()


def cc(carry):
    return cr.cov_carry(carry) if carry is not None else None


def block(M, name):
    bi, bj = SLICES[name]
    return np.asarray(M)[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3]


def block_errors(M, W):
    """the difference of two 9 x 9 matrices by blocks, relative to the largest entry of each block of W"""
    return {b: float(np.abs(block(M, b) - block(W, b)).max() / max(np.abs(block(W, b)).max(), 1e-300)) for b in BLOCKS}


def cov_finite(cov, carry=None):
    recs = [cov] + ([carry["open_cov"]] if carry is not None else [])
    return all(np.isfinite(r["S"]).all() for r in recs)


def zero_beside_a_voided_delta(delta, cov):
    void = (delta["flags"] & cr.VOID_FLAGS) != 0
    flagged = (cov["flags"] & cr.IMU_COV_NONFINITE) != 0
    return not cov["S"][void | flagged].any()


def no_negative_eigenvalue(cov):
    for r in cov:
        w = np.linalg.eigvalsh(cr.matrix(r))
        if not w[0] >= -1e-12 * max(w[-1], 0.0):
            return False
    return True


# ---------------------------------------------------------------------------------------------- (a) the delta part
@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_the_delta_part_is_imu_ref_byte_for_byte(n, name):
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for key, carry in (("none", None), ("open", ic.carried(tb, True)), ("time", ic.carried(tb, False))):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        a = ir.preintegrate_rows(ic.params(), s, tf, prev, carry)
        d, q, rot, c = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, prev, cc(carry))
        assert d.tobytes() == a[0].tobytes() and rot.tobytes() == a[1].tobytes() and c["carry"].tobytes() == a[2].tobytes(), (n, name, key)
        assert cov_finite(q, c) and zero_beside_a_voided_delta(d, q) and (q["q"] == d["q"]).all() and not q["flags"].any()
        paired = (d["flags"] & cr.VOID_FLAGS) == 0
        assert (np.abs(q["S"][paired]).max(axis=1) > 0).all() and no_negative_eigenvalue(q[paired][:8])       # a real pair has a covariance


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(case):
    name, s, tf, prev, carry, must, _ = case
    a = ir.preintegrate_rows(ir.Params(), s, tf, prev, carry)
    d, q, rot, c = cr.preintegrate_cov_rows(ir.Params(), NOISE, s, tf, prev, cc(carry))
    assert d.tobytes() == a[0].tobytes() and rot.tobytes() == a[1].tobytes() and c["carry"].tobytes() == a[2].tobytes(), name
    assert cov_finite(q, c) and zero_beside_a_voided_delta(d, q) and no_negative_eigenvalue(q), name
    for i, f in must.items():
        if f & ir.IMU_NONFINITE:
            assert not q[i]["S"].any(), (name, i)


# ---------------------------------------------------------------------------------------------- (b) the dense model
def _skew(u):
    return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])


def _exp_jr(phi):
    """closed forms (Rodrigues), not the header's series"""
    th = float(np.linalg.norm(phi))
    K = _skew(phi)
    if th < 1e-12:
        return np.eye(3) + K, np.eye(3) - 0.5 * K
    A, B, Cc = math.sin(th) / th, (1.0 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    return np.eye(3) + A * K + B * K @ K, np.eye(3) - B * K + Cc * K @ K


def dense_model(P, noise, samples, t_a, t_b, breaks):
    """the covariance of the delta over (t_a, t_b] with breakpoints at the frame times `breaks`: F S F^T + G Q G^T with 9 x 9 matrices a sub-step"""
    ts, w, a = samples["t"], samples["w"], samples["a"]
    grid = np.unique(np.concatenate([[t_a, t_b], ts[(ts > t_a) & (ts < t_b)], [t for t in breaks if t_a < t < t_b]]))
    W = np.stack([np.interp(grid, ts, w[:, k]) for k in range(3)], 1) - np.asarray(P.bg)
    U = np.stack([np.interp(grid, ts, a[:, k]) for k in range(3)], 1) - np.asarray(P.ba)
    R, S = np.eye(3), np.zeros((9, 9))
    I, Z = np.eye(3), np.zeros((3, 3))
    for k in range(len(grid) - 1):
        h = float(grid[k + 1] - grid[k])
        dR, Jr = _exp_jr(0.5 * (W[k] + W[k + 1]) * h)
        Rn = R @ dR
        Wm = R @ _skew(U[k]) + Rn @ _skew(U[k + 1]) @ dR.T
        F = np.block([[dR.T, Z, Z], [-0.5 * h * Wm, I, Z], [-0.25 * h * h * Wm, h * I, I]])
        g1, g2 = -0.5 * h * (Rn @ _skew(U[k + 1]) @ Jr) * h, (R + Rn) * (0.5 * h)
        G = np.block([[Jr * h, Z], [g1, g2], [0.5 * h * g1, 0.5 * h * g2]])
        Q = np.diag([noise.sigma_g ** 2 / h] * 3 + [noise.sigma_a ** 2 / h] * 3)
        S = F @ S @ F.T + G @ Q @ G.T
        R = Rn
    return S


@pytest.mark.parametrize("L", (1, 8, 32))
def test_covariance_against_the_dense_model(L):
    n = L + 1
    s, tf, _ = ic.stream(n, 10)                                        # 200 Hz
    prev = ic.pairing("long", n)
    d, q, _, _ = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, prev, None)
    want = dense_model(ic.params(), NOISE, s, float(tf[0]), float(tf[-1]), tf)
    err = block_errors(cr.matrix(q[n - 1]), want)
    print(f"\npair of {L} frames against the dense model: {err}")
    assert int(d[n - 1]["q"]) == 0 and int(d[n - 1]["flags"]) == 0 and int(q[n - 1]["flags"]) == 0
    assert max(err.values()) <= 4 * DENSE_ERR[L], err


# ---------------------------------------------------------------------------------------------- (c) calibration
def _delta_of(P, s, tf):
    T0 = ir.intervals(P, s, tf, None)
    acc = T0[1].copy()
    for j in range(2, len(T0)):
        acc = ir.compose(acc, T0[j])
    return acc


@pytest.mark.parametrize("L", (1, 8))
def test_calibration_against_noisy_integrations(L):
    n, hz = L + 1, 10 * ic.FPS
    s, tf, _ = ic.stream(n, 10)
    P = ic.params()
    d, q, _, _ = cr.preintegrate_cov_rows(P, NOISE, s, tf, ic.pairing("long", n), None)
    S, clean, ns = cr.matrix(q[n - 1]), _delta_of(P, s, tf), int(d[n - 1]["n_steps"])
    assert np.abs(np.asarray(clean.R) - d[n - 1]["R"]).max() < 1e-14    # (left to right: the table's record to rounding)
    Rc = np.asarray(clean.R).reshape(3, 3)
    rng = np.random.default_rng(SEED + L)
    E = np.zeros((DRAWS, 9))
    for k in range(DRAWS):
        z = s.copy()
        z["w"] += rng.normal(0.0, NOISE.sigma_g * math.sqrt(hz), z["w"].shape)
        z["a"] += rng.normal(0.0, NOISE.sigma_a * math.sqrt(hz), z["a"].shape)
        o = _delta_of(P, z, tf)
        Er = Rc.T @ np.asarray(o.R).reshape(3, 3)
        E[k, :3] = 0.5 * (Er[2, 1] - Er[1, 2]), 0.5 * (Er[0, 2] - Er[2, 0]), 0.5 * (Er[1, 0] - Er[0, 1])
        E[k, 3:6], E[k, 6:] = np.asarray(o.v) - np.asarray(clean.v), np.asarray(o.p) - np.asarray(clean.p)
    ratio = np.sqrt((E ** 2).mean(axis=0) / np.diag(S))
    chi2 = float(np.einsum("ki,ki->k", E, np.linalg.solve(S, E.T).T).mean())
    end = (ns - 0.5) / ns                                              # the half sample at each end of the midpoint rule
    se_sd, se_chi = 1.0 / math.sqrt(2 * DRAWS), math.sqrt(18.0 / DRAWS)
    print(f"\npair of {L} frames, {ns} sub-steps, {DRAWS} draws: sample / model standard deviation {ratio.min():.3f} - {ratio.max():.3f} "
          f"(band {math.sqrt(end) - 4 * se_sd:.3f} - {1 + 4 * se_sd:.3f}), mean chi-square {chi2:.2f} (band {9 * end - 4 * se_chi:.2f} - {9 + 4 * se_chi:.2f})")
    assert (ratio >= math.sqrt(end) - 4 * se_sd).all() and (ratio <= 1.0 + 4 * se_sd).all(), ratio
    assert 9.0 * end - 4 * se_chi <= chi2 <= 9.0 + 4 * se_chi, chi2


# ---------------------------------------------------------------------------------------------- (d) the lifting table
@pytest.fixture(scope="module")
def big_table():
    s, tf, tb = ic.stream(1024, 2)
    T0 = cr.intervals(ic.params(), NOISE, s, tf, cc(ic.carried(tb, False)))
    return T0, cr.lifting_table(T0, 1024)


def test_lifting_table_against_left_to_right(big_table):
    T0, T = big_table
    worst = dict.fromkeys(BLOCKS, 0.0)

    def measure(a, b, exact):
        (da, qa), (db, qb) = a, b
        assert qa.flags == qb.flags == 0 and da.flags == db.flags == 0
        for f, v in block_errors(qa.matrix(), qb.matrix()).items():
            worst[f] = max(worst[f], v)
        if exact:
            assert qa.numbers() == qb.numbers()

    acc = None
    for L in range(1, 1025):                                           # every length, from frame 0: ONE running left-to-right composition
        acc = cr._copy(T0[0]) if acc is None else cr.compose(acc, T0[L - 1])
        measure(cr.lift(T, L - 1, L), acc, L == 1)
    for L in ic.PAIR_LENGTHS:                                          # and the lengths around the powers of two, ending at the last frame
        measure(cr.lift(T, 1023, L), cr.sequential(T0, 1023, L), L == 1)
    print("\nlifting against left to right:", worst)
    assert all(worst[f] <= LIFT_BOUND[f] for f in worst), worst


# ---------------------------------------------------------------------------------------------- (e) the cuts of a stream
def run_cuts(P, noise, s, tf, prev, cuts):
    """the stream cut into calls: frames whose keyframe lies in an earlier call are VIS_KF_CARRIED; (delta, cov, rot, the last carry)"""
    out, carry, a = [], None, 0
    for m in cuts:
        local = np.asarray([p - a if p >= a else (ir.KF_CARRIED if p >= 0 else p) for p in prev[a:a + m]], np.int32)
        d, q, rot, carry = cr.preintegrate_cov_rows(P, noise, s, tf[a:a + m], local, carry)
        out.append((d, q, rot))
        a += m
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3)) + (carry,)


def within_the_lifting_bound(cov, whole):
    """every record of `cov` against `whole`, by blocks, within LIFT_BOUND of the block's largest entry"""
    for r, w in zip(cov, whole):
        err = block_errors(cr.matrix(r), cr.matrix(w))
        if not all(err[b] <= LIFT_BOUND[b] or not np.abs(w["S"]).any() for b in BLOCKS):
            return False, err
    return True, None


@pytest.mark.parametrize("name", ("chain", "alternate"))
def test_cuts_of_a_stream(name):
    """gate off (the chain): the same bytes however the stream is cut; gate on (every second frame unsaved): within 16 x the lifting table's error"""
    s, tf, _ = ic.stream(37, 10)
    prev, P = ic.pairing(name, 37), ic.params()
    runs = {k: run_cuts(P, NOISE, s, tf, prev, c) for k, c in CUTS.items()}
    whole = runs["B"]
    for k, (d, q, rot, carry) in runs.items():
        assert (d["flags"] == whole[0]["flags"]).all() and (d["n_steps"] == whole[0]["n_steps"]).all() and not q["flags"].any(), k
        if name == "chain":
            assert q["S"].tobytes() == whole[1]["S"].tobytes() and d["R"].tobytes() == whole[0]["R"].tobytes(), k
            assert carry["open_cov"].tobytes() == whole[3]["open_cov"].tobytes() and carry["carry"].tobytes() == whole[3]["carry"].tobytes(), k
        else:
            ok, err = within_the_lifting_bound(q, whole[1])
            assert ok, (k, err)


# ---------------------------------------------------------------------------------------------- (f) exact properties
def test_zero_densities_scaling_and_eigenvalues():
    s, tf, tb = ic.stream(37, 10)
    P = ic.params()
    for name in ("chain", "alternate", "straddle"):
        prev = ic.pairing(name, 37, ir.KF_CARRIED)
        carry = cc(ic.carried(tb, True))
        d0, q0, _, c0 = cr.preintegrate_cov_rows(P, cr.Noise(0.0, 0.0), s, tf, prev, carry)
        assert not q0["S"].any() and not c0["open_cov"]["S"].any() and not q0["flags"].any()
        d1, q1, _, c1 = cr.preintegrate_cov_rows(P, NOISE, s, tf, prev, carry)
        d2, q2, _, c2 = cr.preintegrate_cov_rows(P, cr.Noise(2 * cr.SIGMA_G, 2 * cr.SIGMA_A), s, tf, prev, carry)
        assert d0.tobytes() == d1.tobytes() == d2.tobytes()
        assert (q2["S"] == 4.0 * q1["S"]).all() and (c2["open_cov"]["S"] == 4.0 * c1["open_cov"]["S"]).all()       # a power of two: exact
        assert no_negative_eigenvalue(q1) and no_negative_eigenvalue(c1["open_cov"])
    # one density at a time: the gyro alone leaves no block empty (it turns the force), the accelerometer alone leaves every phi block zero
    prev = ic.pairing("chain", 37, ir.KF_FIRST)
    _, qg, _, _ = cr.preintegrate_cov_rows(P, cr.Noise(cr.SIGMA_G, 0.0), s, tf, prev, None)
    _, qa, _, _ = cr.preintegrate_cov_rows(P, cr.Noise(0.0, cr.SIGMA_A), s, tf, prev, None)
    Ma, Mg = cr.matrix(qa[5]), cr.matrix(qg[5])
    assert not Ma[:3].any() and Ma[3:, 3:].any() and all(np.abs(block(Mg, b)).max() > 0 for b in BLOCKS)
    assert no_negative_eigenvalue(qg[1:]) and no_negative_eigenvalue(qa[1:])


# ---------------------------------------------------------------------------------------------- (g) the sticky flag
def test_an_overflowing_covariance_beside_a_finite_delta_is_flagged_and_the_flag_is_sticky():
    s, tf, tb = ic.stream(6, 10)
    chain = ic.pairing("chain", 6, ir.KF_CARRIED)
    c = cc(ic.carried(tb, True))
    c[0]["open_cov"]["S"][:] = 1.79e308                               # M^T (A M) overflows; the delta does not
    d, q, rot, co = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, chain, c)
    want = ir.preintegrate_rows(ic.params(), s, tf, chain, c["carry"])
    assert d.tobytes() == want[0].tobytes() and int(d[0]["flags"]) == 0 and cov_finite(q, co)
    assert int(q[0]["flags"]) == cr.IMU_COV_NONFINITE and not q[0]["S"].any() and not q["flags"][1:].any() and q["S"][1:].any(axis=1).all()
    # a NaN in the carried covariance alike
    c[0]["open_cov"]["S"][:] = 0.0
    c[0]["open_cov"]["S"][17] = float("nan")
    d, q, _, _ = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, chain, c)
    assert d.tobytes() == want[0].tobytes() and int(q[0]["flags"]) == cr.IMU_COV_NONFINITE and cov_finite(q)
    # densities whose squares overflow: every covariance is flagged, every delta is its sibling's
    d, q, _, co = cr.preintegrate_cov_rows(ic.params(), cr.Noise(1e200, 1e200), s, tf, chain, cc(ic.carried(tb, True)))
    assert d.tobytes() == want[0].tobytes() and (q["flags"] == cr.IMU_COV_NONFINITE).all() and not q["S"].any() and cov_finite(q, co)
    # sticky: nothing saved, so the flagged open delta is carried on through the call and into the next one's first pair
    unsaved = np.full(3, ir.KF_NOT_SAVED, np.int32)
    _, _, _, c1 = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf[:3], unsaved, c)
    assert int(c1["open_cov"]["flags"][0]) == cr.IMU_COV_NONFINITE and cov_finite(q, c1) and int(c1["carry"]["open"]["flags"][0]) == 0
    d2, q2, _, _ = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf[3:], ic.pairing("chain", 3, ir.KF_CARRIED), c1)
    assert int(q2[0]["flags"]) == cr.IMU_COV_NONFINITE and int(d2[0]["flags"]) == 0 and not q2["flags"][1:].any() and not q2[0]["S"].any()
    # and in the table: a flagged entry flags every composition it enters, and only those
    T0 = cr.intervals(ic.params(), NOISE, s, tf, cc(ic.carried(tb, False)))
    T0[2][1].flags |= cr.IMU_COV_NONFINITE
    T = cr.lifting_table(T0, 6)
    for i in range(6):
        for L in range(1, i + 2):
            assert bool(cr.lift(T, i, L)[1].flags) == (i - L < 2 <= i) == bool(cr.sequential(T0, i, L)[1].flags), (i, L)


def test_pack_and_unpack_are_inverse_and_the_host_form_is_row_zero():
    s, tf, tb = ic.stream(4, 10)
    d, q, rot, co = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, ic.pairing("chain", 4, ir.KF_CARRIED), cc(ic.carried(tb, True)))
    for r in q:
        S = [float(x) for x in r["S"]]
        assert cr.pack(cr.unpack(S)) == S
        M = cr.matrix(r)
        assert (M == M.T).all() and M[np.triu_indices(9)].tolist() == S
    d1, q1, r1 = cr.preintegrate_cov(ic.params(), NOISE, s, tb, float(tf[0]))
    a = ir.preintegrate(ic.params(), s, tb, float(tf[0]))
    assert d1.tobytes() == a[0].tobytes() and r1.tobytes() == a[1].tobytes() and int(q1["q"]) == ir.KF_CARRIED and q1["S"].any()
