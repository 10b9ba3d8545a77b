"""GPU: vis_vi_align_rows against the restatement tests/vi_align_ref.py, BYTE FOR BYTE: d_state, d_result and d_carry_out.  Every output sits between
0xEE guards that must keep their bytes.

n = 1, 2, 3 (the first triple), 4, 63, 64, 65, 255, 256, 257 (the thread-stride edges of contract T), 1024 (1025 is refused) and 0 (the carried totals'
solution), each with the pairings of imu_cases and the four carries (none, tails only, tails and sums, sums of a foreign epoch); segment breaks and
an epoch change mid-call; deltas integrated by imu_ref; the hostile rows of tests/vi_align_cases.py; d_state NULL, no carry out; refine_iters 0 and 16."""
import numpy as np
import pytest

import imu_ref as ir
import vi_align_cases as vc
import vi_align_ref as vr

pytestmark = pytest.mark.gpu
FILL = 0xEE
GUARD = 64


def _dev(torch, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.from_numpy(a if len(a) else np.zeros(8, np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _guarded(torch, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _payload(t, nbytes):
    h = t.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all()
    return h[GUARD:GUARD + nbytes]


def prepare_rows(vislam, P, prev, traj, delta, carry=None, want_state=True, want_carry=True):
    """the inputs of one vis_vi_align_rows uploaded and its outputs filled (both synchronise the device); the answer is call(c), which queues the
    call on context c and synchronises nothing.  call(c) answers collect() -> (d_state, d_result, d_carry_out), for after a synchronise"""
    import torch
    n = len(prev)
    keep = [_dev(torch, np.asarray(prev, np.int32)), _dev(torch, np.asarray(traj, vr.TRAJ_DTYPE)), _dev(torch, np.asarray(delta, ir.DELTA_DTYPE))]
    d_carry = _dev(torch, np.asarray(carry, vr.CARRY_DTYPE).reshape(1)) if carry is not None else None
    state, result, cout = _guarded(torch, n * 64), _guarded(torch, 160), _guarded(torch, 720)

    def collect():
        return (_payload(state, n * 64 if want_state else 0).view(vislam.VI_STATE_DTYPE), _payload(result, 160).view(vislam.VI_ALIGN_DTYPE)[0],
                _payload(cout, 720 if want_carry else 0).view(vislam.VI_CARRY_DTYPE))

    def call(c):
        c.vi_align_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), result.data_ptr() + GUARD, state.data_ptr() + GUARD if want_state else 0,
                        d_carry.data_ptr() if carry is not None else 0, cout.data_ptr() + GUARD if want_carry else 0, vp=vc.struct_params(vislam, P))
        return collect
    return call


def rows_on_device(vislam, c, P, *rows, **kw):
    collect = prepare_rows(vislam, P, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, sc, P=None, where=None):
    P = sc["P"] if P is None else P
    got = rows_on_device(vislam, c, P, sc["prev"], sc["traj"], sc["delta"], sc["carry"])
    want = vr.align_rows(P, sc["prev"], sc["traj"], sc["delta"], sc["carry"])
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(sc["prev"])) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[2].tobytes() == want[2].tobytes(), (where, got[2], want[2])
    assert vc.all_finite(*want), where
    return want


@pytest.mark.parametrize("name", vc.PAIRINGS)
@pytest.mark.parametrize("n", vc.NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    for carry in vc.CARRIES:
        st, res, _ = check(vislam, ctx, vc.scene(n, name, carry), where=(n, name, carry))
        if name == "chain" and carry == "sums":
            assert int(res["n_triples"]) == n + vc.HEAD - 2 and int(res["n_triples_call"]) == n
        if name == "chain" and carry == "foreign":
            assert int(res["flags"]) & vr.VIA_RESTART and int(res["n_triples"]) == n
        if name == "chain" and carry == "none":
            assert int(res["n_triples_call"]) == max(n - 2, 0)      # n = 3 is the first triple


def test_more_than_the_maximum_is_refused_and_none_solves_the_carried_totals(vislam, ctx):
    import torch
    buf = _dev(torch, np.zeros(1025 * 216, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.vi_align_rows(1025, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4                                          # VIS_E_CAPACITY
    sc = vc.scene(0, "chain", "sums")
    _, res, co = check(vislam, ctx, sc, where="n = 0")
    assert int(res["n_triples"]) == vc.HEAD - 2 and int(res["flags"]) == 0 and abs(float(res["s"]) - vc.SCALE) < 1e-6
    assert co[0]["last"].tobytes() == sc["carry"][0]["last"].tobytes() and co[0]["last_delta"].tobytes() == sc["carry"][0]["last_delta"].tobytes()


@pytest.mark.parametrize("kind", ("integrated", "biased", "break", "epoch", "break and epoch, carried"))
def test_integrated_deltas_breaks_and_epochs(vislam, ctx, kind):
    sc = {"integrated": lambda: vc.scene(40, "chain", "none", integrate=True),
          "biased": lambda: vc.scene(40, "alternate", "sums", integrate=True, bias=vc.BIAS),
          "break": lambda: vc.scene(40, "chain", "sums", breaks=(17,)),
          "epoch": lambda: vc.scene(40, "chain", "sums", epochs=(21,)),
          "break and epoch, carried": lambda: vc.scene(70, "alternate", "tails", breaks=(20,), epochs=(40,))}[kind]()
    _, res, _ = check(vislam, ctx, sc, where=kind)
    if kind == "epoch":
        assert int(res["epoch_seq"]) == vc.HEAD + 21 and int(res["flags"]) & vr.VIA_RESTART and int(res["n_triples"]) == 40 - 21 - 1
    if kind == "break":
        assert int(res["segment_seq"]) == vc.HEAD + 17 and int(res["flags"]) & vr.VIA_RESTART


@pytest.mark.parametrize("iters", (0, 16))
def test_refine_iters_at_both_ends(vislam, ctx, iters):
    sc = vc.scene(40, "chain", "none", integrate=True)
    _, res, _ = check(vislam, ctx, sc, P=vc.params(refine_iters=iters), where=iters)
    g = np.asarray(res["g"])
    assert abs(float(np.sqrt((g * g).sum())) - vc.G) < 1e-12 and int(res["flags"]) == 0


def test_without_states_and_without_a_carry_out(vislam, ctx):
    sc = vc.scene(65, "alternate", "sums")
    want = vr.align_rows(sc["P"], sc["prev"], sc["traj"], sc["delta"], sc["carry"])
    got = rows_on_device(vislam, ctx, sc["P"], sc["prev"], sc["traj"], sc["delta"], sc["carry"], want_state=False, want_carry=False)
    assert got[1].tobytes() == want[1].tobytes() and got[0].size == 0 and got[2].size == 0
    none = np.zeros(1, vr.CARRY_DTYPE)                                 # a record without VIS_VIC_VALID counts as none
    sc2 = dict(sc, carry=none)
    _, res, _ = check(vislam, ctx, sc2)
    assert int(res["n_triples"]) == int(res["n_triples_call"])


@pytest.mark.parametrize("case", vc.hostile(), ids=lambda c: c[0])
def test_hostile_rows(vislam, ctx, case):
    name, sc, must, must_not = case
    _, res, _ = check(vislam, ctx, sc, where=name)
    f = int(res["flags"])
    if must is None:
        assert f & (vr.VIA_SINGULAR | vr.VIA_GRAVITY_NORM), name
    else:
        assert f & must == must and not f & must_not, (name, f)
