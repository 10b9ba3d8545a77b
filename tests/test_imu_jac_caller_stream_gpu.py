"""GPU: vis_imu_preintegrate_jac_rows, vis_batch_imu_jac, vis_imu_correct_rows and vis_batch_imu_correct on a CALLER's stream, under the rules and
with the rig of tests/stream_order_cases.py: the producer of every device input is still pending on the stream S when the call is queued -- only
stream order can make the call see the real inputs -- and the outputs are read by a consumer on S (the rows forms, on the context's stream) or after
vis_batch_sync (the plan forms, on the pose stream).  Per input a decoy run shows that a stale read would be seen."""
import numpy as np
import pytest

import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import stream_order_cases as so
from test_imu_caller_stream_gpu import Env, _check, _inputs
from test_imu_jac_ref import DBA, DBG, jc

pytestmark = pytest.mark.gpu
B = so.B
P = ic.params()


def _jac_inputs():
    ins = _inputs()
    ins["carry"] = tuple(jc(c) for c in ins["carry"])
    return ins


def case_rows(vislam):
    ins = _jac_inputs()
    ip = ic.struct_params(vislam, P)
    n_s = len(ins["samples"][0])
    return so.Case("vis_imu_preintegrate_jac_rows", so.CTX, ins, dict(delta=B * 216, jac=B * 296, rot=B * 36, cout=528),
                   lambda c, p: c.imu_preintegrate_jac_rows(B, p("samples"), n_s, p("tframe"), p("prev"), p("delta"), p("jac"), p("rot"), p("carry"), p("cout"), ip=ip))


def case_plan(vislam, frames):
    ins = _jac_inputs()
    del ins["prev"], ins["carry"]                                    # (the plan's own pairing and carry)
    ip = ic.struct_params(vislam, P)
    n_s = len(ins["samples"][0])
    return so.Case("vis_batch_imu_jac", so.POSE, ins, dict(delta=B * 216, jac=B * 296, rot=B * 36),
                   lambda c, p: c.batch_imu_jac(B, p("samples"), n_s, p("tframe"), p("delta"), p("jac"), p("rot"), ip=ip), so._two_launches(frames))


def _correct_inputs():
    ins = _inputs()
    a = jr.preintegrate_jac_rows(P, ins["samples"][0], ins["tframe"][0], ins["prev"][0], jc(ins["carry"][0]))
    b = jr.preintegrate_jac_rows(P, ins["samples"][1], ins["tframe"][1], ins["prev"][0], jc(ins["carry"][0]))
    return dict(rows=(a[0], b[0]), jacs=(a[1], b[1]), dbg=(np.asarray(DBG), np.asarray([0.02, 0.01, -0.03])), dba=(np.asarray(DBA), np.asarray([-0.2, 0.1, 0.05])))


def _case_correct(vislam, name, kind, call, setup=None):
    ip = ic.struct_params(vislam, P)
    outs = dict(out=B * 216, rot=B * 36, status=B * 4)
    run = lambda c, p: getattr(c, call)(B, p("rows"), p("jacs"), p("dbg"), p("out"), p("dba"), p("rot"), p("status"), ip=ip)
    return so.Case(name, kind, _correct_inputs(), outs, run, setup)


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
    ins = _jac_inputs()
    ref = jr.preintegrate_jac_rows(P, ins["samples"][0], ins["tframe"][0], ins["prev"][0], ins["carry"][0])
    assert want["delta"] == ref[0].tobytes() and want["jac"] == ref[1].tobytes() and want["rot"] == ref[2].tobytes() and want["cout"] == ref[3].tobytes()


def test_the_plan_form_on_a_caller_stream(vislam, env):
    want = _check(env, env.cP, case_plan(vislam, env.frames))
    delta, jac = np.frombuffer(want["delta"], ir.DELTA_DTYPE), np.frombuffer(want["jac"], jr.JAC_DTYPE)
    assert (delta["flags"][1:] == 0).all() and int(delta[0]["flags"]) == ir.IMU_NO_CARRY      # (launch 0 was not integrated)
    assert jac["Jva"][1:].any(axis=1).all() and not jac[0]["Jva"].any() and not jac["flags"].any()


def _correct_reference(want):
    ins = _correct_inputs()
    ref = jr.correct_rows(P, ins["rows"][0], ins["jacs"][0], ins["dbg"][0], ins["dba"][0])
    assert want["out"] == ref[0].tobytes() and want["rot"] == ref[1].tobytes() and want["status"] == ref[2].tobytes()
    assert (ref[2] == jr.IMC_OK).sum() >= B // 2 - 1                   # (every second frame of the pairing has a pair)


def test_the_correction_on_a_caller_stream(vislam, env):
    _correct_reference(_check(env, env.cA, _case_correct(vislam, "vis_imu_correct_rows", so.CTX, "imu_correct_rows")))


def test_the_plan_form_of_the_correction_on_a_caller_stream(vislam, env):
    _correct_reference(_check(env, env.cP, _case_correct(vislam, "vis_batch_imu_correct", so.POSE, "batch_imu_correct", so._two_launches(env.frames))))
