"""CPU: the restatement tests/vi_align_ref.py against the planted motion of tests/vi_align_cases.py and against an independent numpy model (the
stacked rows through np.linalg.lstsq, step 3 through np.linalg.solve), and the conventions it rests on against imu_ref and trajectory_ref.

Measured here (200 Hz samples through imu_ref, 40 frames at 20 frames/s, sample phases 0.11 and 0.61) and asserted at 4 x:
  without a gyro bias   scale 9.1e-6 relative, gravity 4.6e-6 m/s^2, velocities 1.1e-5 m/s
  planted bias (0.01, -0.02, 0.005) rad/s   recovered to 4.9e-8 in the one step, c0 5.1e-5 -> c1 8.9e-15; dv and dp are NOT corrected for it, which
                        moves the scale by 6.8e-5 relative and gravity by 2.3e-3 m/s^2 (the header's limit)
The numpy model differs from the restatement by MODEL (below), asserted at 16 x.  Four cuts of a 37-frame stream differ in the carried sums by
CUT_BOUND / 16 relative to the summed absolute terms; the GPU stream test asserts CUT_BOUND."""
import numpy as np
import pytest

import imu_ref as ir
import vi_align_cases as vc
import vi_align_ref as vr

MEASURED = dict(scale=9.1e-6, gravity=4.6e-6, velocity=1.1e-5, bias=4.9e-8, scale_biased=6.8e-5, gravity_biased=2.3e-3)
MODEL = dict(dbg=4.9e-17, s_lin=8.9e-16, g_lin=3.6e-15, s=8.9e-16, g=4.5e-16, restack=2.7e-15)   # |restatement - numpy model|, measured on the planted scene
CUT_BOUND = dict(gyro=16 * 5.0e-16, lin=16 * 3.9e-16)
CUTS = {"A": [8, 1, 4, 8, 3, 8, 5], "B": [37], "C": [8, 8, 8, 8, 5], "D": [1] * 37}
TRUE_G = np.asarray(vc.GRAVITY)


def run(sc, P=None, **kw):
    return vr.align_rows(sc["P"] if P is None else P, sc["prev"], sc["traj"], sc["delta"], sc["carry"], **kw)


def test_rotation_convention_against_imu_ref_and_trajectory_records():
    """r_ic^T dR r_ic (imu_ref's d_rot) is the camera-frame rotation R_q R_i^T of the trajectory records, and Rw_q^T Rw_i is dR, to the
    discretisation level of the midpoint rule at 200 Hz"""
    sc = vc.scene(40, "alternate", "none", integrate=True)
    ip = ir.Params(r_ic=vc.R_IC)
    worst = 0.0
    for i in range(40):
        q = ir.norm_prev(sc["prev"], i)
        if q < 0:
            continue
        d = ir.Delta()
        d.R = [float(x) for x in sc["delta"][i]["R"]]
        rot = np.asarray(ir.mul(ir.tmul(ip.r_ic, d.R), ip.r_ic)).reshape(3, 3)
        Rq, Ri = sc["traj"][q]["R"].reshape(3, 3), sc["traj"][i]["R"].reshape(3, 3)
        worst = max(worst, np.abs(rot - Rq @ Ri.T).max())
        tq, ti = vr.tail_of(sc["P"], sc["traj"][q], ir.norm_prev(sc["prev"], q)), vr.tail_of(sc["P"], sc["traj"][i], q)
        worst = max(worst, np.abs(np.asarray(ir.tmul(tq.Rw, ti.Rw)) - sc["delta"][i]["R"]).max())
        C = -(Ri.T @ sc["traj"][i]["t"])                                  # the camera centre and the metric IMU position s C + L
        p = vc.SCALE * C + Ri.T @ np.asarray(vc.P_CI)
        other = vc.SCALE * np.asarray(ti.C) + np.asarray(ti.L)
        assert np.abs(p - other).max() < 1e-14
    print(f"\n|r_ic^T dR r_ic - R_q R_i^T| <= {worst:.2e}")
    assert worst < 4 * 4e-8


@pytest.mark.parametrize("phase", (0.11, 0.61))
def test_the_planted_motion_is_recovered(phase):
    sc = vc.scene(40, "chain", "none", integrate=True, phase=phase)
    st, res, _ = run(sc)
    assert int(res["flags"]) == 0 and int(res["n_triples"]) == 38 and int(res["n_pairs"]) == 39
    err = dict(scale=abs(float(res["s"]) - vc.SCALE) / vc.SCALE, gravity=float(np.abs(res["g"] - TRUE_G).max()))
    has_v = [i for i in range(40) if int(st[i]["flags"]) & vr.VIS_HAS_V]
    err["velocity"] = max(float(np.abs(st[i]["v"] - np.asarray(vc.truth_velocity(float(sc["times"][i])))).max()) for i in has_v)
    pos = [i for i in range(40) if int(st[i]["flags"]) & vr.VIS_HAS_P]
    ptrue = np.asarray([vc.motion(float(sc["times"][i]))[0] for i in pos])
    err["position"] = float(np.abs((st["p"][pos] - st["p"][pos[0]]) - (ptrue - ptrue[0])).max())
    print(f"\nphase {phase}: {err}, rms {float(res['rms']):.2e}")
    assert len(has_v) == 39 and len(pos) == 39                         # (the root has an epoch of its own)
    for k in ("scale", "gravity", "velocity"):
        assert err[k] <= 4 * MEASURED[k], k
    assert err["position"] <= 4 * MEASURED["scale"] * 4.0              # positions span 4 m
    assert abs(float(np.sqrt((res["g"] ** 2).sum())) - vc.G) < 1e-13


@pytest.mark.parametrize("phase", (0.11, 0.61))
def test_a_planted_gyro_bias_is_recovered_in_one_step(phase):
    sc = vc.scene(40, "chain", "none", integrate=True, bias=vc.BIAS, phase=phase)
    _, res, _ = run(sc)
    err = float(np.abs(res["dbg"] - np.asarray(vc.BIAS)).max())
    print(f"\nphase {phase}: bias error {err:.2e}, c0 {float(res['c0']):.2e} -> c1 {float(res['c1']):.2e}, scale "
          f"{abs(float(res['s']) - vc.SCALE) / vc.SCALE:.2e}, gravity {float(np.abs(res['g'] - TRUE_G).max()):.2e}")
    assert err <= 4 * MEASURED["bias"] and float(res["c0"]) > 4e-5 and float(res["c1"]) < 1e-12 and float(res["c0"]) == float(res["c0_call"])
    assert abs(float(res["s"]) - vc.SCALE) / vc.SCALE <= 4 * MEASURED["scale_biased"]
    assert float(np.abs(res["g"] - TRUE_G).max()) <= 4 * MEASURED["gravity_biased"]
    # the other sign diverges: the step is H dbg = +J^T e
    d = sc["delta"].copy()
    for i in range(40):
        if ir.norm_prev(sc["prev"], i) >= 0:
            dl = vr.delta_of(d[i])
            d[i]["R"] = ir.mul(dl.R, ir.exp_and_jr(ir.mulv(dl.J, [-float(x) for x in res["dbg"]]))[0])
    _, res2, _ = vr.align_rows(sc["P"], sc["prev"], sc["traj"], d)
    assert float(res2["c0"]) > 3.5 * float(res["c0"])


def numpy_model(sc, P):
    """the same estimate by other means: numpy matrices, the stacked rows through lstsq, step 3 through solve"""
    n = len(sc["prev"])
    R = [sc["traj"][i]["R"].reshape(3, 3) for i in range(n)]
    r_ic, p_ci = np.asarray(P.r_ic).reshape(3, 3), np.asarray(P.p_ci)
    C = [-(R[i].T @ sc["traj"][i]["t"]) for i in range(n)]
    Rw = [(r_ic @ R[i]).T for i in range(n)]
    L = [R[i].T @ p_ci for i in range(n)]
    Jr, er, A, b = [], [], [], []
    for i in range(1, n):
        d = sc["delta"][i]
        Er = d["R"].reshape(3, 3).T @ (Rw[i - 1].T @ Rw[i])
        er.append(0.5 * np.array([Er[2, 1] - Er[1, 2], Er[0, 2] - Er[2, 0], Er[1, 0] - Er[0, 1]]))
        Jr.append(d["JRg"].reshape(3, 3))
    dbg = np.linalg.lstsq(np.vstack(Jr), np.concatenate(er), rcond=None)[0]
    for c in range(2, n):
        db, dc = sc["delta"][c - 1], sc["delta"][c]
        dt1, dt2 = float(db["dt"]), float(dc["dt"])
        lam = (C[c] - C[c - 1]) * dt1 - (C[c - 1] - C[c - 2]) * dt2
        gam = (Rw[c - 1] @ dc["p"]) * dt1 - (Rw[c - 2] @ db["p"]) * dt2 + (Rw[c - 2] @ db["v"]) * dt1 * dt2 \
            - ((L[c] - L[c - 1]) * dt1 - (L[c - 1] - L[c - 2]) * dt2)
        A.append(np.hstack([lam.reshape(3, 1), -0.5 * dt1 * dt2 * (dt1 + dt2) * np.eye(3)]))
        b.append(gam)
    A, b = np.vstack(A), np.concatenate(b)
    x = np.linalg.lstsq(A, b, rcond=None)[0]
    return dbg, x, A, b


def numpy_refine(M, r, x, G, iters, stacked=None):
    gh, s = x[1:] / np.linalg.norm(x[1:]), x[0]
    for _ in range(iters):
        k = int(np.argmin(np.abs(gh)))
        b1 = np.eye(3)[k] - gh[k] * gh
        b1 /= np.linalg.norm(b1)
        b2 = np.cross(gh, b1)
        Pm = np.zeros((4, 3))
        Pm[0, 0], Pm[1:, 1], Pm[1:, 2] = 1.0, b1, b2
        x0 = np.concatenate([[0.0], G * gh])
        if stacked is None:
            y = np.linalg.solve(Pm.T @ M @ Pm, Pm.T @ (r - M @ x0))
        else:
            A, b = stacked
            y = np.linalg.lstsq(A @ Pm, b - A @ x0, rcond=None)[0]
        g = G * gh + y[1] * b1 + y[2] * b2
        gh, s = g / np.linalg.norm(g), y[0]
    return s, G * gh


def test_against_the_independent_numpy_model():
    sc = vc.scene(40, "chain", "none", integrate=True, bias=vc.BIAS)
    P = sc["P"]
    _, res, co = run(sc)
    dbg, x, A, b = numpy_model(sc, P)
    M, r = vr.matrix4([float(v) for v in co[0]["lin"]])
    M, r = np.asarray(M), np.asarray(r)
    s_a, g_a = numpy_refine(M, r, x, P.G, P.refine_iters)
    s_b, g_b = numpy_refine(None, None, x, P.G, P.refine_iters, stacked=(A, b))
    diff = dict(dbg=float(np.abs(res["dbg"] - dbg).max()), s_lin=abs(float(res["s_lin"]) - x[0]), g_lin=float(np.abs(res["g_lin"] - x[1:]).max()),
                s=abs(float(res["s"]) - s_a), g=float(np.abs(res["g"] - g_a).max()))
    sums = max(float(np.abs(M - A.T @ A).max()), float(np.abs(r - A.T @ b).max()))
    restack = max(abs(s_a - s_b), float(np.abs(g_a - g_b).max()))
    print(f"\nrestatement - numpy model: {diff}; sums {sums:.2e}; step 3 from (M, r) - from the stacked rows {restack:.2e}")
    for k, v in diff.items():
        assert v <= 16 * MODEL[k], (k, v)
    assert sums < 1e-18 and restack <= 16 * MODEL["restack"]
    # the residual norms of the states are the stacked system's under the reported solution
    st = run(sc)[0]
    rho = (A @ np.concatenate([[float(res["s"])], res["g"]]) - b).reshape(-1, 3)
    assert np.abs(np.sqrt((rho ** 2).sum(1)) - st["res"][2:]).max() < 1e-15
    assert float(res["rms"]) == pytest.approx(float(np.sqrt((rho ** 2).sum() / len(rho))), rel=1e-9)


def test_refine_iters_zero_reports_the_linear_solution_at_norm_G():
    sc = vc.scene(40, "chain", "none", integrate=True)
    _, res, _ = run(sc, P=vc.params(refine_iters=0))
    assert float(res["s"]) == float(res["s_lin"])
    assert np.abs(res["g"] - vc.G * res["g_lin"] / float(res["g_lin_norm"])).max() < 1e-14
    _, r16, _ = run(sc, P=vc.params(refine_iters=16))
    _, r4, _ = run(sc)
    assert abs(float(r16["s"]) - float(r4["s"])) < 1e-12               # the iteration has converged after four rounds


@pytest.mark.parametrize("kw", (dict(), dict(epochs=(9,)), dict(breaks=(6,))), ids=("plain", "epoch", "break"))
@pytest.mark.parametrize("carry", ("none", "sums"))
@pytest.mark.parametrize("pairing", ("chain", "alternate"))
def test_cuts_of_a_stream(pairing, carry, kw):
    sc = vc.scene(37, pairing, carry, integrate=True, bias=vc.BIAS, **kw)
    scale = {}
    _, whole, cw = run(sc, detail=scale)
    if sc["carry"] is not None:
        scale = {f: scale[f] + np.abs(sc["carry"][0][f]) for f in scale}
    worst = [0.0, 0.0]
    for name, cut in CUTS.items():
        st, res, co = vc.run_cuts(sc, cut)
        for f in ("n_pairs", "n_triples", "segment_seq", "epoch_seq"):
            assert int(res[f]) == int(whole[f]), (name, f)
        for t in ("last", "parent"):                                  # the tails are the frames' own: the same bytes
            assert all(co[0][t][f].tobytes() == cw[0][t][f].tobytes() for f in ("C", "Rw", "L", "segment_seq", "epoch_seq", "flags")), (name, t)
        assert all(co[0]["last_delta"][f].tobytes() == cw[0]["last_delta"][f].tobytes() for f in ("R", "v", "p", "dt", "JRg")), name
        d = vc.sum_differences(co, cw, scale)
        worst = [max(worst[0], d[0]), max(worst[1], d[1])]
        assert int(((st["flags"] & vr.VIS_HAS_PAIR) != 0).sum()) == int(whole["n_pairs_call"])
        if name == "B":
            assert co.tobytes() == cw.tobytes()
    print(f"\n{pairing}, {carry}, {kw}: sums differ by {worst[0]:.2e} (gyro), {worst[1]:.2e} (linear) of the summed absolute terms")
    assert worst[0] <= CUT_BOUND["gyro"] / 4 and worst[1] <= CUT_BOUND["lin"] / 4    # (a quarter of the bound the GPU stream test asserts)


def test_a_foreign_epoch_restarts_the_linear_sums_and_keeps_the_gyro_sums():
    sc = vc.scene(24, "chain", "foreign")
    _, res, co = run(sc)
    own = run(dict(sc, carry=vc.scene(24, "chain", "tails")["carry"]))[1]
    assert int(res["flags"]) & vr.VIA_RESTART and int(res["n_triples"]) == int(res["n_triples_call"]) == 24
    assert int(res["n_pairs"]) == 24 + vc.HEAD - 1 and int(own["n_pairs"]) == 24
    assert float(res["s_lin"]) == float(own["s_lin"]) and int(co[0]["epoch_seq"]) == int(res["epoch_seq"]) == 1


@pytest.mark.parametrize("case", vc.hostile(), ids=lambda c: c[0])
def test_hostile_rows(case):
    name, sc, must, must_not = case
    st, res, co = run(sc)
    f = int(res["flags"])
    assert vc.all_finite(st, res, co), name
    if must is None:                                                  # a constant velocity: the scale cannot be observed
        assert f & (vr.VIA_SINGULAR | vr.VIA_GRAVITY_NORM), (name, f)
        assert float(res["s"]) == 1.0 and not res["g"].any()
    else:
        assert f & must == must and not f & must_not, (name, f)
    if name == "no frame saved":
        c = sc["carry"][0]
        assert all(co[0][k].tobytes() == c[k].tobytes() for k in ("gyro", "lin", "last", "parent", "last_delta", "n_pairs", "n_triples"))
        assert not st["flags"].any()


def test_every_scene_of_the_gpu_test_is_finite_and_flagged_as_expected():
    for n in (1, 2, 3, 4, 65):
        for pairing in vc.PAIRINGS:
            for carry in vc.CARRIES:
                st, res, co = run(vc.scene(n, pairing, carry))
                assert vc.all_finite(st, res, co), (n, pairing, carry)
                assert bool(int(res["flags"]) & vr.VIA_FEW) == (int(res["n_triples"]) < 8)
                assert bool(int(res["flags"]) & vr.VIA_RESTART) == (carry == "foreign")
    _, res, _ = run(vc.scene(3, "chain", "none"))
    assert int(res["n_triples"]) == 1 and int(res["n_pairs"]) == 2     # three frames: the first triple
