"""GPU: vis_vi_align_ba_rows and vis_batch_vi_align_ba on a CALLER's stream, under the rules and with the rig of tests/stream_order_cases.py: the
producer of every device input (pairing, trajectory records, deltas, Jacobian records, carry) is still pending on the stream S when the call is
queued -- only stream order can make the call see the real inputs -- and the outputs are read by a consumer on S (the rows form, on the context's
stream) or after vis_batch_sync (the plan form, on the pose stream).  Per input a decoy run shows that a stale read would be seen."""
import numpy as np
import pytest

import imu_ref as ir
import stream_order_cases as so
import vi_align_ba_cases as bc
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr
from test_vi_align_ba_gpu import struct_ba_params
from test_vi_align_caller_stream_gpu import Env, _check

pytestmark = pytest.mark.gpu
B = so.B


def _inputs():
    real, other = bc.scene(B, "chain", "sums"), bc.scene(B, "alternate", "sums", epochs=(3,), acc_bias=(0.0, 0.3, 0.0))
    decoy_jac = other["jac"].copy()
    decoy_jac["Jpa"] *= 1.5                                           # (usable where the pairing lets it be, and other numbers)
    return dict(prev=(real["prev"], other["prev"]), traj=(real["traj"], other["traj"]), delta=(real["delta"], other["delta"]), jac=(real["jac"], decoy_jac),
                carry=(real["carry"], other["carry"]))


def case_rows(vislam):
    vp, bp = vc.struct_params(vislam, vc.params()), struct_ba_params(vislam, br.BaParams())
    return so.Case("vis_vi_align_ba_rows", so.CTX, _inputs(), dict(state=B * 64, result=304, cout=1280),
                   lambda c, p: c.vi_align_ba_rows(B, p("prev"), p("traj"), p("delta"), p("jac"), p("result"), p("state"), p("carry"), p("cout"), vp=vp, bp=bp))


def case_plan(vislam, frames):
    ins = _inputs()
    del ins["prev"], ins["carry"]                                    # (the plan's own pairing and carry)
    vp, bp = vc.struct_params(vislam, vc.params(min_triples=4, min_pairs=4)), struct_ba_params(vislam, br.BaParams(min_ba_triples=4))
    return so.Case("vis_batch_vi_align_ba", so.POSE, ins, dict(state=B * 64, result=304),
                   lambda c, p: c.batch_vi_align_ba(B, p("traj"), p("delta"), p("jac"), p("result"), p("state"), vp=vp, bp=bp), so._two_launches(frames))


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
    sc = bc.scene(B, "chain", "sums")
    ref = bc.run(sc)
    assert want["state"] == ref[0].tobytes() and want["result"] == ref[1].tobytes() and want["cout"] == ref[2].tobytes()
    assert int(ref[1]["ba_flags"]) == 0 and int(ref[1]["n_ba_triples"]) == B + bc.HEAD - 2 and ref[1]["dba"].any()


def test_the_plan_form_on_a_caller_stream(vislam, env):
    want = _check(env, env.cP, case_plan(vislam, env.frames))
    res = np.frombuffer(want["result"], br.BA_RESULT_DTYPE)[0]
    st = np.frombuffer(want["state"], vr.STATE_DTYPE)
    # launch 0 was not aligned: frame 0's carried parent has no tail, so B - 1 frames have a posed parent and B - 2 a posed grandparent too
    assert int(res["a"]["n_pairs"]) == B - 1 and int(res["n_ba_triples"]) == B - 2 and int(st[0]["q"]) == ir.KF_CARRIED
