"""CPU: the restatement tests/imu_jac_ref.py -- its delta part against imu_ref byte for byte, its Jacobians against central differences of
imu_ref.preintegrate_rows, its lifting table against the left-to-right order, the cuts of a stream, the correction against integrating again, the
sticky flag, the correction's status codes and the closed loop align -> correct -> align on the planted motion of tests/vi_align_cases.py.

Measured on the restatement (printed by every run; asserted at 4 x, the lifting table at 16 x as in test_imu_ref.py):
  central differences (step 1e-5) of the composed pair at 200 Hz, ic.params(), relative to the block's largest entry, worst of the four blocks:
    pair of 1 frame 2.2e-9, 8 frames 3.3e-10, 32 frames 1.2e-10 (FD_ERR) -- the finite difference's own error
  correction by dbg = (0.01, -0.02, 0.005), dba = (0.1, -0.05, 0.2) against integrating again with the new biases (CORRECTED; uncorrected in brackets):
    1 frame   R 2.4e-9 (1.0e-3)  v 4.8e-6 (1.0e-2)  p 8.0e-8 (2.5e-4)
    8 frames  R 1.5e-6 (8.4e-3)  v 3.6e-4 (9.4e-2)  p 4.6e-5 (1.8e-2)
    32 frames R 7.0e-5 (3.0e-2)  v 7.3e-3 (0.50)    p 3.7e-3 (0.36)
    an accelerometer step alone: 6.9e-18, 1.2e-16, 1.8e-15 (ACC_ONLY) -- rounding, v and p are linear in ba
  lifting table against the left-to-right composition, n = 1024, pair lengths 1 ... 1023, relative to the block's largest entry:
    Jvg 3.4e-15, Jva 2.5e-15, Jpg 2.1e-15, Jpa 1.8e-15 (LIFT_ERR); their 16-fold bounds the cuts of a gated stream
  closed loop, 40 frames, planted gyro bias (0.01, -0.02, 0.005), phases 0.11 and 0.61: the second alignment against the UNBIASED run of the motion:
    scale 2.3e-8 relative, gravity 8.9e-7 m/s^2, c0_call 8.2e-16 (LOOP); against the truth: scale 9.0e-6 (uncorrected 6.7e-5), gravity 5.4e-6
    m/s^2 (uncorrected 2.2e-3)"""
import numpy as np
import pytest

import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import vi_align_cases as vc
import vi_align_ref as vr

FD_ERR = {1: 2.2e-9, 8: 3.3e-10, 32: 1.2e-10}
CORRECTED = {1: dict(R=2.4e-9, v=4.8e-6, p=8.0e-8), 8: dict(R=1.5e-6, v=3.6e-4, p=4.6e-5), 32: dict(R=7.0e-5, v=7.3e-3, p=3.7e-3)}
ACC_ONLY = {1: 6.9e-18, 8: 1.2e-16, 32: 1.8e-15}
LIFT_ERR = {"Jvg": 3.4e-15, "Jva": 2.5e-15, "Jpg": 2.1e-15, "Jpa": 1.8e-15}
LIFT_BOUND = {k: 16 * v for k, v in LIFT_ERR.items()}
LOOP = dict(scale=2.3e-8, gravity=8.9e-7, c0_call=8.2e-16)
DBG, DBA = (0.01, -0.02, 0.005), (0.1, -0.05, 0.2)
CUTS = {"A": [8, 1, 4, 8, 3, 8, 5], "B": [37], "C": [8, 8, 8, 8, 5], "D": [1] * 37}


def jc(carry):
    return jr.jac_carry(carry) if carry is not None else None


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def jac_finite(jac, carry=None):
    recs = [jac] + ([carry["open_jac"]] if carry is not None else [])
    return all(np.isfinite(r[f]).all() for r in recs for f in jr.BLOCKS)


def zero_beside_a_voided_delta(delta, jac):
    void = (delta["flags"] & jr.VOID_FLAGS) != 0
    flagged = (jac["flags"] & jr.IMU_JAC_NONFINITE) != 0
    return all(not jac[f][void | flagged].any() for f in jr.BLOCKS)


@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_the_delta_part_is_imu_ref_byte_for_byte(n, name):
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        a = ir.preintegrate_rows(ic.params(), s, tf, prev, carry)
        d, j, rot, c = jr.preintegrate_jac_rows(ic.params(), s, tf, prev, jc(carry))
        assert d.tobytes() == a[0].tobytes() and rot.tobytes() == a[1].tobytes() and c["carry"].tobytes() == a[2].tobytes(), (n, name)
        assert jac_finite(j, c) and zero_beside_a_voided_delta(d, j) and (j["q"] == d["q"]).all() and not j["flags"].any()
        paired = (d["flags"] & jr.VOID_FLAGS) == 0
        assert all(np.abs(j[f][paired]).max(axis=1).all() for f in jr.BLOCKS if paired.any())    # a real pair has no empty block


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(case):
    name, s, tf, prev, carry, must, _ = case
    a = ir.preintegrate_rows(ir.Params(), s, tf, prev, carry)
    d, j, rot, c = jr.preintegrate_jac_rows(ir.Params(), s, tf, prev, jc(carry))
    assert d.tobytes() == a[0].tobytes() and rot.tobytes() == a[1].tobytes() and c["carry"].tobytes() == a[2].tobytes(), name
    assert jac_finite(j, c) and zero_beside_a_voided_delta(d, j), name
    for i, f in must.items():
        if f & ir.IMU_NONFINITE:
            assert not any(j[i][b].any() for b in jr.BLOCKS), (name, i)


def central_differences(s, tf, prev, i, eps=1e-5):
    """the four blocks of frame i by central differences of imu_ref.preintegrate_rows (the rows form: the composed pair itself)"""
    out = {}
    for which, (bv, bp) in (("bg", ("Jvg", "Jpg")), ("ba", ("Jva", "Jpa"))):
        cv, cp = [], []
        for k in range(3):
            r = []
            for sign in (1.0, -1.0):
                P = ic.params()
                getattr(P, which)[k] += sign * eps
                r.append(ir.preintegrate_rows(P, s, tf, prev, None)[0][i])
            cv.append((r[0]["v"] - r[1]["v"]) / (2 * eps))
            cp.append((r[0]["p"] - r[1]["p"]) / (2 * eps))
        out[bv], out[bp] = np.stack(cv, 1).reshape(9), np.stack(cp, 1).reshape(9)
    return out


@pytest.mark.parametrize("L", (1, 8, 32))
def test_jacobians_against_central_differences(L):
    n = L + 1
    s, tf, _ = ic.stream(n, 10)                                        # 200 Hz
    prev = ic.pairing("long", n)
    d, j, _, _ = jr.preintegrate_jac_rows(ic.params(), s, tf, prev, None)
    fd = central_differences(s, tf, prev, n - 1)
    err = {b: _rel(j[n - 1][b], fd[b]) for b in jr.BLOCKS}
    print(f"\npair of {L} frames: {err}")
    assert int(d[n - 1]["q"]) == 0 and int(d[n - 1]["flags"]) == 0 and max(err.values()) <= 4 * FD_ERR[L], err


@pytest.mark.parametrize("L", (1, 8, 32))
def test_the_correction_against_integrating_again(L):
    n = L + 1
    s, tf, _ = ic.stream(n, 10)
    prev = ic.pairing("long", n)
    P = ic.params()
    d, j, _, _ = jr.preintegrate_jac_rows(P, s, tf, prev, None)

    def again(g, a):
        Q = ic.params()
        Q.bg, Q.ba = [P.bg[k] + g[k] for k in range(3)], [P.ba[k] + a[k] for k in range(3)]
        return ir.preintegrate_rows(Q, s, tf, prev, None)[0][n - 1]

    out, rot, st = jr.correct_rows(P, d, j, DBG, DBA)
    want = again(DBG, DBA)
    err = {f: float(np.abs(out[n - 1][f] - want[f]).max()) for f in ("R", "v", "p")}
    before = {f: float(np.abs(d[n - 1][f] - want[f]).max()) for f in ("R", "v", "p")}
    print(f"\npair of {L} frames: corrected {err}, uncorrected {before}")
    assert int(st[n - 1]) == jr.IMC_OK and int(st[0]) == jr.IMC_UNUSABLE and out[0].tobytes() == d[0].tobytes()
    assert all(err[f] <= 4 * CORRECTED[L][f] and err[f] < before[f] / 20 for f in err), (err, before)
    for f in ("dt", "JRg", "n_steps", "flags", "q", "reserved_"):
        assert out[n - 1][f].tobytes() == d[n - 1][f].tobytes(), f
    assert rot[n - 1].tobytes() == np.asarray(ir.mul(ir.tmul(P.r_ic, list(out[n - 1]["R"])), P.r_ic), np.float64).astype(np.float32).tobytes()
    # an accelerometer step alone is exact to rounding; None is (0, 0, 0)
    out, _, _ = jr.correct_rows(P, d, j, (0.0, 0.0, 0.0), DBA)
    want = again((0.0, 0.0, 0.0), DBA)
    acc = max(float(np.abs(out[n - 1][f] - want[f]).max()) for f in ("v", "p"))
    print(f"accelerometer step alone: {acc}")
    assert out[n - 1]["R"].tobytes() == d[n - 1]["R"].tobytes() == want["R"].tobytes() and acc <= 4 * ACC_ONLY[L]
    a, b = jr.correct_rows(P, d, j, DBG, None), jr.correct_rows(P, d, j, DBG, (0.0, 0.0, 0.0))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def big_table():
    s, tf, tb = ic.stream(1024, 2)
    T0 = jr.intervals(ic.params(), s, tf, jc(ic.carried(tb, False)))
    return T0, jr.lifting_table(T0, 1024)


def test_lifting_table_against_left_to_right(big_table):
    T0, T = big_table
    worst = dict.fromkeys(jr.BLOCKS, 0.0)
    for L in ic.PAIR_LENGTHS + (1024,):
        for i in sorted({L - 1, min(1023, L + 5), 1023}):
            if L > i + 1:
                continue
            (da, a), (db, b) = jr.lift(T, i, L), jr.sequential(T0, i, L)
            assert a.flags == b.flags == 0 and da.flags == db.flags == 0
            for f, x, y in (("Jvg", a.vg, b.vg), ("Jva", a.va, b.va), ("Jpg", a.pg, b.pg), ("Jpa", a.pa, b.pa)):
                worst[f] = max(worst[f], _rel(x, y))
            if L == 1:
                assert a.numbers() == b.numbers()
    print("\nlifting against left to right:", worst)
    assert all(worst[f] <= LIFT_BOUND[f] for f in worst), worst


def run_cuts(P, s, tf, prev, cuts):
    """the stream cut into calls: frames whose keyframe lies in an earlier call are VIS_KF_CARRIED; (delta, jac, rot, the last carry)"""
    out, carry, a = [], None, 0
    for m in cuts:
        local = np.asarray([p - a if p >= a else (ir.KF_CARRIED if p >= 0 else p) for p in prev[a:a + m]], np.int32)
        d, j, rot, carry = jr.preintegrate_jac_rows(P, s, tf[a:a + m], local, carry)
        out.append((d, j, rot))
        a += m
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3)) + (carry,)


@pytest.mark.parametrize("name", ("chain", "alternate"))
def test_cuts_of_a_stream(name):
    """gate off (the chain): the same bytes however the stream is cut; gate on (every second frame unsaved): within 16 x the lifting table's error"""
    s, tf, _ = ic.stream(37, 10)
    prev, P = ic.pairing(name, 37), ic.params()
    runs = {k: run_cuts(P, s, tf, prev, c) for k, c in CUTS.items()}
    whole = runs["B"]
    for k, (d, j, rot, carry) in runs.items():
        assert (d["flags"] == whole[0]["flags"]).all() and (d["n_steps"] == whole[0]["n_steps"]).all() and not j["flags"].any(), k
        if name == "chain":
            for f in jr.BLOCKS + ("flags",):
                assert j[f].tobytes() == whole[1][f].tobytes(), (k, f)
            assert d["R"].tobytes() == whole[0]["R"].tobytes() and carry["open_jac"].tobytes() == whole[3]["open_jac"].tobytes()
        else:
            for f in jr.BLOCKS:
                scale = np.abs(whole[1][f]).max(axis=1)
                diff = np.abs(j[f] - whole[1][f]).max(axis=1)
                assert (diff <= LIFT_BOUND[f] * scale).all(), (k, f, float((diff / np.maximum(scale, 1e-300)).max()))


def test_an_overflowing_jacobian_beside_a_finite_delta_is_flagged_and_the_flag_is_sticky():
    s, tf, tb = ic.stream(6, 10)
    chain = ic.pairing("chain", 6, ir.KF_CARRIED)
    c = jc(ic.carried(tb, True))
    c[0]["open_jac"]["Jpg"][:], c[0]["open_jac"]["Jvg"][:] = 1.79e308, 1.79e308      # X.Jpg + X.Jvg Y.dt overflows; the delta does not
    d, j, rot, co = jr.preintegrate_jac_rows(ic.params(), s, tf, chain, c)
    want = ir.preintegrate_rows(ic.params(), s, tf, chain, c["carry"])
    assert d.tobytes() == want[0].tobytes() and int(d[0]["flags"]) == 0 and jac_finite(j, co)
    assert int(j[0]["flags"]) == jr.IMU_JAC_NONFINITE and not any(j[0][b].any() for b in jr.BLOCKS) and not j["flags"][1:].any()
    # a NaN in the carried Jacobians alike
    c[0]["open_jac"]["Jpg"][:], c[0]["open_jac"]["Jvg"][:] = 0.0, 0.0
    c[0]["open_jac"]["Jva"][4] = float("nan")
    d, j, _, _ = jr.preintegrate_jac_rows(ic.params(), s, tf, chain, c)
    assert d.tobytes() == want[0].tobytes() and int(j[0]["flags"]) == jr.IMU_JAC_NONFINITE and jac_finite(j)
    # sticky: nothing saved, so the flagged open delta is carried on through the call and into the next one's first pair
    unsaved = np.full(3, ir.KF_NOT_SAVED, np.int32)
    _, _, _, c1 = jr.preintegrate_jac_rows(ic.params(), s, tf[:3], unsaved, c)
    assert int(c1["open_jac"]["flags"][0]) == jr.IMU_JAC_NONFINITE and jac_finite(j, c1) and int(c1["carry"]["open"]["flags"][0]) == 0
    d2, j2, _, _ = jr.preintegrate_jac_rows(ic.params(), s, tf[3:], ic.pairing("chain", 3, ir.KF_CARRIED), c1)
    assert int(j2[0]["flags"]) == jr.IMU_JAC_NONFINITE and int(d2[0]["flags"]) == 0 and not j2["flags"][1:].any() and not j2[0]["Jva"].any()
    # and in the table: a flagged entry flags every composition it enters, and only those
    T0 = jr.intervals(ic.params(), s, tf, jc(ic.carried(tb, False)))
    T0[2][1].flags |= jr.IMU_JAC_NONFINITE
    T = jr.lifting_table(T0, 6)
    for i in range(6):
        for L in range(1, i + 2):
            assert bool(jr.lift(T, i, L)[1].flags) == (i - L < 2 <= i) == bool(jr.sequential(T0, i, L)[1].flags), (i, L)


def correction_status_cases():
    """(delta, jac, dbg, dba, P, the statuses): one record per status code, in the order of the header's list"""
    s, tf, tb = ic.stream(8, 10)
    P = ic.params()
    d, j, _, _ = jr.preintegrate_jac_rows(P, s, tf, ic.pairing("chain", 8, ir.KF_CARRIED), jc(ic.carried(tb, False)))
    d, j = d.copy(), j.copy()
    d[1]["flags"] |= ir.IMU_NONFINITE                                 # unusable by its flags
    d[2]["v"][1] = float("inf")                                       # unusable by a number
    j[3]["flags"] = jr.IMU_JAC_NONFINITE                              # flagged Jacobians
    d[4]["JRg"][:] = [x * 1e4 for x in d[4]["JRg"]]                   # |JRg dbg| beyond max_angle
    j[5]["Jpg"][2] = 1.7e308                                          # a result that overflows
    j[5]["Jpa"][2] = 1.7e308
    j[6]["Jvg"][0] = float("nan")                                     # a Jacobian that is not a number (and not flagged): the result is not finite
    want = [jr.IMC_OK, jr.IMC_UNUSABLE, jr.IMC_UNUSABLE, jr.IMC_JAC, jr.IMC_ANGLE, jr.IMC_NONFINITE, jr.IMC_NONFINITE, jr.IMC_OK]
    return d, j, (3.0, -2.0, 5.0), (1e3, 1e3, 1e3), P, want                 # (|JRg dbg| about 0.3 rad over a 50 ms pair)


def test_the_status_codes_of_the_correction():
    d, j, dbg, dba, P, want = correction_status_cases()
    out, rot, st = jr.correct_rows(P, d, j, dbg, dba)
    assert st.tolist() == want
    for i, w in enumerate(want):
        assert (out[i].tobytes() == d[i].tobytes()) == (w != jr.IMC_OK), i
    assert np.isfinite(rot).all() and (rot[1] == np.asarray(ir.EYE, np.float32)).all()            # (d_rot's rule: the flags, not the status)
    for i in (2, 4):                                                  # a record copied for another reason keeps the rotation of its own R
        assert rot[i].tobytes() == np.asarray(ir.mul(ir.tmul(P.r_ic, list(d[i]["R"])), P.r_ic), np.float64).astype(np.float32).tobytes(), i
    for bad in (float("nan"), float("inf"), -float("inf")):
        for g, a in (((0.0, bad, 0.0), None), (DBG, (bad, 0.0, 0.0))):
            out, _, st = jr.correct_rows(P, d, j, g, a)
            assert st.tolist() == [jr.IMC_BIAS if w in (jr.IMC_OK, jr.IMC_ANGLE, jr.IMC_NONFINITE) else w for w in want] and out.tobytes() == d.tobytes()


@pytest.mark.parametrize("phase", (0.11, 0.61))
def test_the_closed_loop_align_correct_align(phase):
    """the planted gyro bias of vi_align_cases: the second alignment, on records corrected with the first one's dbg, lands on the unbiased run"""
    true_g = np.asarray(vc.GRAVITY)
    clean = vc.scene(40, "chain", "none", integrate=True, phase=phase)
    _, r0, _ = vr.align_rows(clean["P"], clean["prev"], clean["traj"], clean["delta"], None)
    sc = vc.scene(40, "chain", "none", integrate=True, bias=vc.BIAS, phase=phase)
    ip = ir.Params()
    d, j, _, _ = jr.preintegrate_jac_rows(ip, sc["samples"], sc["times"], sc["prev"], None)
    assert d.tobytes() == sc["delta"].tobytes()
    _, r1, _ = vr.align_rows(sc["P"], sc["prev"], sc["traj"], d, None)
    d2, _, st = jr.correct_rows(ip, d, j, np.asarray(r1["dbg"]).reshape(3))
    assert st.tolist() == [jr.IMC_UNUSABLE] + [jr.IMC_OK] * 39
    _, r2, _ = vr.align_rows(sc["P"], sc["prev"], sc["traj"], d2, None)
    truth = lambda r: (abs(float(r["s"]) - vc.SCALE) / vc.SCALE, float(np.abs(np.asarray(r["g"]).reshape(3) - true_g).max()))
    got = dict(scale=abs(float(r2["s"]) - float(r0["s"])) / vc.SCALE, gravity=float(np.abs(np.asarray(r2["g"]) - np.asarray(r0["g"])).max()),
               c0_call=abs(float(r2["c0_call"]) - float(r0["c0_call"])))
    print(f"\nphase {phase}: against the unbiased run {got}; against the truth: unbiased {truth(r0)}, uncorrected {truth(r1)}, corrected {truth(r2)}")
    assert int(r2["flags"]) == 0 and int(r2["n_pairs"]) == 39 and int(r2["n_triples"]) == 38
    assert all(got[k] <= 4 * LOOP[k] for k in got), got
    assert truth(r2)[0] < truth(r1)[0] and truth(r2)[1] < truth(r1)[1]
    assert float(np.abs(np.asarray(r2["dbg"])).max()) < 1e-8 < float(np.abs(np.asarray(r1["dbg"])).max())
