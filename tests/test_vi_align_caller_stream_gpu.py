"""GPU: vis_vi_align_rows and vis_batch_vi_align on a CALLER's stream, under the rules and with the rig of tests/stream_order_cases.py: the
producer of every device input (pairing, trajectory records, deltas, carry) is still pending on the stream S when the call is queued -- only
stream order can make the call see the real inputs -- and the outputs are read by a consumer on S (the rows form, which the header places on the
context's stream) or after vis_batch_sync (the plan form, on the pose stream).  Per input a decoy run shows that a stale read would be seen."""
import numpy as np
import pytest

import imu_ref as ir
import stream_order_cases as so
import vi_align_cases as vc
import vi_align_ref as vr

pytestmark = pytest.mark.gpu
B = so.B


class Env:
    pass


def _inputs():
    real, other = vc.scene(B, "chain", "sums"), vc.scene(B, "alternate", "tails", epochs=(3,), still=True)
    return dict(prev=(real["prev"], other["prev"]), traj=(real["traj"], other["traj"]), delta=(real["delta"], other["delta"]),
                carry=(real["carry"], other["carry"]))


def case_rows(vislam):
    vp = vc.struct_params(vislam, vc.params())
    return so.Case("vis_vi_align_rows", so.CTX, _inputs(), dict(state=B * 64, result=160, cout=720),
                   lambda c, p: c.vi_align_rows(B, p("prev"), p("traj"), p("delta"), p("result"), p("state"), p("carry"), p("cout"), vp=vp))


def case_plan(vislam, frames):
    ins = _inputs()
    del ins["prev"], ins["carry"]                                    # (the plan's own pairing and carry)
    vp = vc.struct_params(vislam, vc.params(min_triples=4, min_pairs=4))
    return so.Case("vis_batch_vi_align", so.POSE, ins, dict(state=B * 64, result=160),
                   lambda c, p: c.batch_vi_align(B, p("traj"), p("delta"), p("result"), p("state"), vp=vp), so._two_launches(frames))


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
    sc = vc.scene(B, "chain", "sums")
    ref = vr.align_rows(sc["P"], sc["prev"], sc["traj"], sc["delta"], sc["carry"])
    assert want["state"] == ref[0].tobytes() and want["result"] == ref[1].tobytes() and want["cout"] == ref[2].tobytes()
    assert int(ref[1]["flags"]) == 0 and int(ref[1]["n_triples"]) == B + vc.HEAD - 2


def test_the_plan_form_on_a_caller_stream(vislam, env):
    want = _check(env, env.cP, case_plan(vislam, env.frames))
    res = np.frombuffer(want["result"], vr.RESULT_DTYPE)[0]
    st = np.frombuffer(want["state"], vr.STATE_DTYPE)
    # launch 0 was not aligned: frame 0's carried parent has no tail, so B - 1 frames have a posed parent and B - 2 a posed grandparent too
    assert int(res["n_pairs"]) == B - 1 and int(res["n_triples"]) == B - 2 and int(st[0]["q"]) == ir.KF_CARRIED and not int(st[0]["flags"]) & vr.VIS_HAS_PAIR
