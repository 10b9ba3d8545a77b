"""GPU: vis_vi_align_ba_rows against the restatement tests/vi_align_ba_ref.py, BYTE FOR BYTE: d_state, d_result and d_carry_out.  Every output sits
between 0xEE guards that must keep their bytes.

n = 1, 2, 3 (the first triple), 4, 63, 64, 65, 255, 256, 257 (the thread-stride edges of contract T), 1024 (1025 is refused) and 0 (the carried totals'
solution), each with the pairings of imu_cases and the carries (none, tails and sums, sums of a foreign epoch) on the two-axis motion; the embedded
record against vis_vi_align_rows on the same inputs; the fixed-axis motion (unobservable); segment breaks and an epoch change mid-call; deltas and
Jacobians integrated by imu_jac_ref; the hostile rows of tests/vi_align_ba_cases.py; d_state NULL, no carry out; refine_iters 0 and 16."""
import numpy as np
import pytest

import imu_jac_ref as jr
import imu_ref as ir
import vi_align_ba_cases as bc
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr
from test_vi_align_gpu import FILL, GUARD, _dev, _guarded, _payload, rows_on_device

pytestmark = pytest.mark.gpu


def struct_ba_params(vislam, BP):
    bp = vislam.default_vi_align_ba_params()
    bp.pivot_rel, bp.min_ba_triples = BP.pivot_rel, BP.min_ba_triples
    return bp


def prepare_ba_rows(vislam, P, BP, prev, traj, delta, jac, carry=None, want_state=True, want_carry=True):
    """the inputs of one vis_vi_align_ba_rows uploaded and its outputs filled (both synchronise the device); call(c) queues the call on context c,
    synchronises nothing and answers collect() -> (d_state, d_result, d_carry_out), for after a synchronise"""
    import torch
    n = len(prev)
    keep = [_dev(torch, np.asarray(prev, np.int32)), _dev(torch, np.asarray(traj, vr.TRAJ_DTYPE)), _dev(torch, np.asarray(delta, ir.DELTA_DTYPE)),
            _dev(torch, np.asarray(jac, jr.JAC_DTYPE))]
    d_carry = _dev(torch, np.asarray(carry, br.BA_CARRY_DTYPE).reshape(1)) if carry is not None else None
    state, result, cout = _guarded(torch, n * 64), _guarded(torch, 304), _guarded(torch, 1280)

    def collect():
        return (_payload(state, n * 64 if want_state else 0).view(vislam.VI_STATE_DTYPE), _payload(result, 304).view(vislam.VI_ALIGN_BA_DTYPE)[0],
                _payload(cout, 1280 if want_carry else 0).view(vislam.VI_BA_CARRY_DTYPE))

    def call(c):
        c.vi_align_ba_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), result.data_ptr() + GUARD,
                           state.data_ptr() + GUARD if want_state else 0, d_carry.data_ptr() if carry is not None else 0,
                           cout.data_ptr() + GUARD if want_carry else 0, vp=vc.struct_params(vislam, P), bp=struct_ba_params(vislam, BP))
        return collect
    return call


def ba_rows_on_device(vislam, c, P, BP, *rows, **kw):
    collect = prepare_ba_rows(vislam, P, BP, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, sc, P=None, BP=None, where=None, sibling=False):
    P, BP = sc["P"] if P is None else P, sc["BP"] if BP is None else BP
    got = ba_rows_on_device(vislam, c, P, BP, sc["prev"], sc["traj"], sc["delta"], sc["jac"], sc["carry"])
    want = br.align_ba_rows(P, BP, sc["prev"], sc["traj"], sc["delta"], sc["jac"], sc["carry"])
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(sc["prev"])) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[2].tobytes() == want[2].tobytes(), (where, got[2], want[2])
    assert bc.all_finite(*want), where
    if sibling:                                                       # the embedded record and carry are vis_vi_align_rows' of the same inputs
        inner = None if sc["carry"] is None else sc["carry"][0]["carry"]
        sib = rows_on_device(vislam, c, P, sc["prev"], sc["traj"], sc["delta"], inner)
        assert got[1]["a"].tobytes() == sib[1].tobytes() and got[2][0]["carry"].tobytes() == sib[2][0].tobytes(), where
        if int(got[1]["ba_flags"]) & br.VIAB_FAILED:
            assert got[0].tobytes() == sib[0].tobytes(), where
    return want


@pytest.mark.parametrize("name", bc.PAIRINGS)
@pytest.mark.parametrize("n", bc.NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    for carry in bc.CARRIES:
        st, res, _ = check(vislam, ctx, bc.scene(n, name, carry), where=(n, name, carry), sibling=carry == "sums")
        if name == "chain" and carry == "sums":
            assert int(res["n_ba_triples"]) == n + bc.HEAD - 2 and int(res["n_ba_triples_call"]) == n and int(res["ba_flags"]) == 0
            assert bc.errors(res)[2] < 1e-6                            # (closed-form records: the planted bias to the quadrature's error)
        if name == "chain" and carry == "foreign":
            assert int(res["a"]["flags"]) & vr.VIA_RESTART and int(res["n_ba_triples"]) == n
        if name == "chain" and carry == "none":
            assert int(res["n_ba_triples_call"]) == max(n - 2, 0)      # n = 3 is the first triple
            assert bool(int(res["ba_flags"]) & br.VIAB_FEW) == (n - 2 < 16)


def test_more_than_the_maximum_is_refused_and_none_solves_the_carried_totals(vislam, ctx):
    import torch
    buf = _dev(torch, np.zeros(1025 * 296, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.vi_align_ba_rows(1025, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4                                          # VIS_E_CAPACITY
    sc = bc.scene(0, "chain", "sums")
    _, res, co = check(vislam, ctx, sc, where="n = 0", sibling=True)
    assert int(res["n_ba_triples"]) == bc.HEAD - 2 and int(res["ba_flags"]) == 0 and bc.errors(res)[2] < 1e-6
    assert co[0]["last_jac"].tobytes() == sc["carry"][0]["last_jac"].tobytes()


@pytest.mark.parametrize("n", (8, 12, 20, 40, 100))
def test_a_fixed_axis_is_unobservable(vislam, ctx, n):
    sc = bc.scene(n, "chain", "none", integrate=True, axes=1)
    _, res, _ = check(vislam, ctx, sc, BP=br.BaParams(min_ba_triples=1), where=n, sibling=True)
    assert int(res["ba_flags"]) == br.VIAB_UNOBSERVABLE and not res["dba"].any()
    assert res["s_ba"].tobytes() == res["a"]["s"].tobytes() and res["g_ba"].tobytes() == res["a"]["g"].tobytes()


@pytest.mark.parametrize("kind", ("integrated", "both biases", "break", "epoch", "break and epoch, carried"))
def test_integrated_records_breaks_and_epochs(vislam, ctx, kind):
    sc = {"integrated": lambda: bc.scene(40, "chain", "none", integrate=True),
          "both biases": lambda: bc.scene(40, "alternate", "sums", integrate=True, gyro_bias=bc.GYRO_BIAS),
          "break": lambda: bc.scene(40, "chain", "sums", breaks=(17,)),
          "epoch": lambda: bc.scene(40, "chain", "sums", epochs=(21,)),
          "break and epoch, carried": lambda: bc.scene(70, "alternate", "sums", breaks=(20,), epochs=(40,))}[kind]()
    _, res, _ = check(vislam, ctx, sc, where=kind, sibling=True)
    if kind == "integrated":
        e = bc.errors(res)
        assert int(res["ba_flags"]) == 0 and e[0] < 4 * 7.3e-6 and e[2] < 4 * 6.9e-6 and e[3] > 2e-2     # test_vi_align_ba_ref.MEASURED[40]
    if kind == "epoch":
        assert int(res["a"]["epoch_seq"]) == bc.HEAD + 21 and int(res["n_ba_triples"]) == 40 - 21 - 1
    if kind == "break":
        assert int(res["a"]["segment_seq"]) == bc.HEAD + 17 and int(res["a"]["flags"]) & vr.VIA_RESTART


@pytest.mark.parametrize("iters", (0, 16))
def test_refine_iters_at_both_ends(vislam, ctx, iters):
    sc = bc.scene(40, "chain", "none", integrate=True)
    _, res, _ = check(vislam, ctx, sc, P=vc.params(refine_iters=iters), where=iters)
    g = np.asarray(res["g_ba"])
    assert abs(float(np.sqrt((g * g).sum())) - vc.G) < 1e-12 and int(res["ba_flags"]) == 0
    if iters == 0:
        assert res["dba"].tobytes() == res["dba_lin"].tobytes() and float(res["s_ba"]) == float(res["s_lin7"])


def test_without_states_and_without_a_carry_out(vislam, ctx):
    sc = bc.scene(65, "alternate", "sums")
    want = bc.run(sc)
    got = ba_rows_on_device(vislam, ctx, sc["P"], sc["BP"], sc["prev"], sc["traj"], sc["delta"], sc["jac"], sc["carry"], want_state=False, want_carry=False)
    assert got[1].tobytes() == want[1].tobytes() and got[0].size == 0 and got[2].size == 0
    none = np.zeros(1, br.BA_CARRY_DTYPE)                              # a record without VIS_VIC_VALID counts as none
    _, res, _ = check(vislam, ctx, dict(sc, carry=none))
    assert int(res["n_ba_triples"]) == int(res["n_ba_triples_call"])


@pytest.mark.parametrize("case", bc.hostile(), ids=lambda c: c[0])
def test_hostile_rows(vislam, ctx, case):
    name, sc, must, must_not = case
    _, res, _ = check(vislam, ctx, sc, where=name, sibling=True)
    f = int(res["ba_flags"])
    if must is not None:
        assert f & must == must and not f & must_not, (name, f)
