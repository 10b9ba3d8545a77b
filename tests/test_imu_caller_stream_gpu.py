"""GPU: vis_imu_preintegrate_rows and vis_batch_imu on a CALLER's stream, under the rules and with the rig of tests/stream_order_cases.py: the
producer of every device input (samples, frame times, pairing, carry) is still pending on the stream S when the call is queued -- only stream
order can make the call see the real inputs -- and the outputs are read by a consumer on S (the rows form, which the header places on the
context's stream) or after vis_batch_sync (the plan form, on the pose stream).  Per input a decoy run shows that a stale read would be seen.
The delay chain is sized from the host time of the calls themselves, as the rig's own fixture does."""
import numpy as np
import pytest

import imu_cases as ic
import imu_ref as ir
import stream_order_cases as so

pytestmark = pytest.mark.gpu
B = so.B
P = ic.params()


class Env:
    pass


def _inputs():
    s, tf, tb = ic.stream(B, 10)
    other = ic.stream(B, 10, rate=lambda t: ([0.9, -0.4, 0.3], [0.0, 9.0, 1.0]))[0]
    prev = ic.pairing("alternate", B, ir.KF_CARRIED)
    return dict(samples=(s, other), tframe=(tf, tf + 0.013), prev=(prev, ic.pairing("chain", B, ir.KF_CARRIED)),
                carry=(ic.carried(tb, True), ic.carried(tb - 0.007, False)))


def case_rows(vislam):
    ins = _inputs()
    ip = ic.struct_params(vislam, P)
    n_s = len(ins["samples"][0])
    return so.Case("vis_imu_preintegrate_rows", so.CTX, ins, dict(delta=B * 216, rot=B * 36, cout=232),
                   lambda c, p: c.imu_preintegrate_rows(B, p("samples"), n_s, p("tframe"), p("prev"), p("delta"), p("rot"), p("carry"), p("cout"), ip=ip))


def case_plan(vislam, frames):
    ins = _inputs()
    del ins["prev"], ins["carry"]                                    # (the plan's own pairing and carry)
    ip = ic.struct_params(vislam, P)
    n_s = len(ins["samples"][0])
    return so.Case("vis_batch_imu", so.POSE, ins, dict(delta=B * 216, rot=B * 36),
                   lambda c, p: c.batch_imu(B, p("samples"), n_s, p("tframe"), p("delta"), p("rot"), ip=ip), so._two_launches(frames))


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


def _check(E, c, case):
    torch = E.torch
    rig = so.Rig(torch, case)
    want, _ = so.run_sync(torch, c, rig)
    got, late, host_ms = so.run_late(torch, c, E.S, E.delay, rig)
    print(f"\n{case.name}: host {host_ms:.3f} ms of the late call, chain {E.delay.chain_ms:.1f} ms")
    assert late, (case.name, "the producer had finished when the call returned", host_ms)
    for k in want:
        assert got[k] == want[k], (case.name, k, "differs from the synchronised run")
    for name in case.inputs:
        decoy, _ = so.run_sync(torch, c, rig, (name,))
        assert any(decoy[k] != want[k] for k in want), (case.name, name, "its decoy gives the bytes of the real input")
    return want


def test_rows_on_a_caller_stream(vislam, env):
    want = _check(env, env.cA, case_rows(vislam))
    ins = _inputs()
    ref = ir.preintegrate_rows(P, ins["samples"][0], ins["tframe"][0], ins["prev"][0], ins["carry"][0])
    assert want["delta"] == ref[0].tobytes() and want["rot"] == ref[1].tobytes() and want["cout"] == ref[2].tobytes()


def test_the_plan_form_on_a_caller_stream(vislam, env):
    want = _check(env, env.cP, case_plan(vislam, env.frames))
    delta = np.frombuffer(want["delta"], ir.DELTA_DTYPE)
    assert (delta["flags"][1:] == 0).all() and int(delta[0]["flags"]) == ir.IMU_NO_CARRY      # (launch 0 was not integrated)
