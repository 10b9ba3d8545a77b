"""GPU: vis_imu_preintegrate_cov_rows and vis_batch_imu_cov on a CALLER's stream, under the rules and with the rig of tests/stream_order_cases.py: the
producer of every device input is still pending on the stream S when the call is queued -- only stream order can make the call see the real inputs --
and the outputs are read by a consumer on S (the rows form, on the context's stream) or after vis_batch_sync (the plan form, on the pose stream).  Per
input a decoy run shows that a stale read would be seen."""
import numpy as np
import pytest

import imu_cases as ic
import imu_cov_ref as cr
import imu_ref as ir
import stream_order_cases as so
from test_imu_caller_stream_gpu import Env, _check, _inputs
from test_imu_cov_gpu import struct_noise
from test_imu_cov_ref import NOISE, cc

pytestmark = pytest.mark.gpu
B = so.B
P = ic.params()


def _cov_inputs():
    ins = _inputs()
    ins["carry"] = tuple(cc(c) for c in ins["carry"])
    return ins


def case_rows(vislam):
    ins = _cov_inputs()
    ip, nz = ic.struct_params(vislam, P), struct_noise(vislam, NOISE)
    n_s = len(ins["samples"][0])
    return so.Case("vis_imu_preintegrate_cov_rows", so.CTX, ins, dict(delta=B * 216, cov=B * 368, rot=B * 36, cout=600),
                   lambda c, p: c.imu_preintegrate_cov_rows(B, p("samples"), n_s, p("tframe"), p("prev"), p("delta"), p("cov"), p("rot"), p("carry"), p("cout"),
                                                            ip=ip, noise=nz))


def case_plan(vislam, frames):
    ins = _cov_inputs()
    del ins["prev"], ins["carry"]                                    # (the plan's own pairing and carry)
    ip, nz = ic.struct_params(vislam, P), struct_noise(vislam, NOISE)
    n_s = len(ins["samples"][0])
    return so.Case("vis_batch_imu_cov", so.POSE, ins, dict(delta=B * 216, cov=B * 368, rot=B * 36),
                   lambda c, p: c.batch_imu_cov(B, p("samples"), n_s, p("tframe"), p("delta"), p("cov"), p("rot"), ip=ip, noise=nz), so._two_launches(frames))


@pytest.fixture(scope="module")
def env(vislam, canvas):
    import torch
    E = Env()
    E.torch, E.S = torch, torch.cuda.Stream()
    E.cA, E.cP = vislam.Context(0), so.plan_context(vislam)
    E.cA.set_stream(E.S)
    E.cP.set_stream(E.S.cuda_stream)
    E.frames = so.PlanFrames(vislam, torch, canvas)
    E.delay = so.Delay(torch, E.S)
    E.delay.measure()
    rig = so.Rig(torch, case_rows(vislam))
    host = [so.run_sync(torch, E.cA, rig)[1] for _ in range(4)][2:]
    chain_ms, ok = E.delay.size(max(host))
    if not ok:
        pytest.fail(f"a chain of {so.FACTOR:g} x the host time {max(host):.3f} ms is {chain_ms:.1f} ms > {so.CHAIN_MAX_MS:g} ms")
    yield E
    torch.cuda.synchronize()
    E.cP.close()
    E.cA.close()


def test_rows_on_a_caller_stream(vislam, env):
    want = _check(env, env.cA, case_rows(vislam))
    ins = _cov_inputs()
    ref = cr.preintegrate_cov_rows(P, NOISE, ins["samples"][0], ins["tframe"][0], ins["prev"][0], ins["carry"][0])
    assert want["delta"] == ref[0].tobytes() and want["cov"] == ref[1].tobytes() and want["rot"] == ref[2].tobytes() and want["cout"] == ref[3].tobytes()


def test_the_plan_form_on_a_caller_stream(vislam, env):
    want = _check(env, env.cP, case_plan(vislam, env.frames))
    delta, cov = np.frombuffer(want["delta"], ir.DELTA_DTYPE), np.frombuffer(want["cov"], cr.COV_DTYPE)
    assert (delta["flags"][1:] == 0).all() and int(delta[0]["flags"]) == ir.IMU_NO_CARRY      # (launch 0 was not integrated)
    assert cov["S"][1:].any(axis=1).all() and not cov[0]["S"].any() and not cov["flags"].any()


# ---- the inertial factor, both forms
def _factor_inputs():
    """(real, decoy) per device input, from the planted motion of tests/test_imu_factor_ref.py: every decoy changes the records"""
    from test_imu_factor_ref import planted, turned
    pl = planted(B)
    prev2 = pl["prev"].copy()
    prev2[B // 2] = ir.KF_NOT_SAVED
    delta2, cov2, state2, result2 = pl["delta"].copy(), pl["cov"].copy(), pl["true_state"].copy(), pl["true_result"].copy()
    delta2["v"][:, 0] += 0.01
    cov2["S"] *= 4.0
    state2["v"][:, 1] += 0.1
    result2[0]["g"] = [0.0, 0.0, 9.81]
    return pl, dict(prev=(pl["prev"], prev2), traj=(pl["traj"], turned(pl["traj"], B - 1, 1.0)), delta=(pl["delta"], delta2), cov=(pl["cov"], cov2),
                    state=(pl["true_state"], state2), result=(pl["true_result"], result2))


def _case_factor(vislam, name, kind, setup=None):
    import vi_align_cases as vc
    pl, ins = _factor_inputs()
    vp = vc.struct_params(vislam, pl["P"])
    if kind == so.POSE:
        del ins["prev"]                                               # (the plan's own pairing: a chain whose first frame is carried)
        run = lambda c, p: c.batch_imu_factor(B, p("traj"), p("delta"), p("cov"), p("state"), p("result"), p("out"), vp=vp)
    else:
        run = lambda c, p: c.imu_factor_rows(B, p("prev"), p("traj"), p("delta"), p("cov"), p("state"), p("result"), p("out"), vp=vp)
    return so.Case(name, kind, ins, dict(out=B * 96), run, setup)


def _factor_reference(want, plan):
    import imu_factor_ref as ff
    pl, ins = _factor_inputs()
    prev = pl["prev"].copy()
    if plan:
        prev[0] = ir.KF_CARRIED
    ref = ff.factor_rows(pl["P"], ff.FactorParams(), prev, pl["traj"], pl["delta"], pl["cov"], pl["true_state"], pl["true_result"])
    assert want["out"] == ref.tobytes() and (ref["flags"][1:] == 0).all() and (ref["chi2"][1:] > 0).all()


def test_the_factor_on_a_caller_stream(vislam, env):
    _factor_reference(_check(env, env.cA, _case_factor(vislam, "vis_imu_factor_rows", so.CTX)), False)


def test_the_plan_form_of_the_factor_on_a_caller_stream(vislam, env):
    _factor_reference(_check(env, env.cP, _case_factor(vislam, "vis_batch_imu_factor", so.POSE, so._two_launches(env.frames))), True)
