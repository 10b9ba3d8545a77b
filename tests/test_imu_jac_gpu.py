"""GPU: vis_imu_preintegrate_jac_rows, vis_imu_preintegrate_jac and vis_imu_correct_rows against the restatement tests/imu_jac_ref.py, BYTE FOR
BYTE: d_delta, d_jac, d_rot, d_carry_out, d_delta_out, d_rot_out and d_status.  Every output sits between 0xEE guards that must keep their bytes.  The
delta row is also checked against vis_imu_preintegrate_rows on the same device inputs: a Jacobian never changes a delta.

n = 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024 (1025 is refused) with the four pairings of tests/imu_cases.py, each with a carry that has an open delta
(and its Jacobians), one that holds a time alone, and none; 0, 1, 2, 10 and 100 samples per interval; the hostile rows; an overflowing carried
Jacobian beside a finite delta; the host form; the correction at n = 1, 63, 64, 65, 1024 with d_dba NULL and not, every status code, and d_dbg
pointing into a vis_vi_align record."""
import numpy as np
import pytest

import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
from test_imu_gpu import GUARD, _dev, _guarded, _payload, rows_on_device
from test_imu_jac_ref import DBA, DBG, correction_status_cases, jac_finite, jc, zero_beside_a_voided_delta

pytestmark = pytest.mark.gpu


def prepare_jac_rows(vislam, P, samples, tframe, prev, carry=None, want_rot=True, want_carry=True):
    """test_imu_gpu.prepare_rows for vis_imu_preintegrate_jac_rows; carry: a JAC_CARRY record or None.  call(c) queues the call and answers
    collect() -> (d_delta, d_jac, d_rot (n, 9), d_carry_out), for after a synchronise"""
    import torch
    n = len(tframe)
    keep = [_dev(torch, np.asarray(samples, ir.SAMPLE_DTYPE)), _dev(torch, np.asarray(tframe, np.float64)), _dev(torch, np.asarray(prev, np.int32))]
    d_carry = _dev(torch, np.asarray(carry, jr.JAC_CARRY_DTYPE).reshape(1)) if carry is not None else None
    delta, jac, rot, cout = _guarded(torch, n * 216), _guarded(torch, n * 296), _guarded(torch, n * 36), _guarded(torch, 528)

    def collect():
        return (_payload(delta, n * 216).view(vislam.IMU_DELTA_DTYPE), _payload(jac, n * 296).view(vislam.IMU_BIAS_JAC_DTYPE),
                _payload(rot, n * 36 if want_rot else 0).view(np.float32).reshape(-1, 9), _payload(cout, 528 if want_carry else 0).view(vislam.IMU_JAC_CARRY_DTYPE))

    def call(c):
        c.imu_preintegrate_jac_rows(n, keep[0].data_ptr() if len(samples) else 0, len(samples), keep[1].data_ptr(), keep[2].data_ptr(), delta.data_ptr() + GUARD,
                                    jac.data_ptr() + GUARD, rot.data_ptr() + GUARD if want_rot else 0, d_carry.data_ptr() if carry is not None else 0,
                                    cout.data_ptr() + GUARD if want_carry else 0, ip=ic.struct_params(vislam, P))
        return collect
    return call


def jac_rows_on_device(vislam, c, P, *rows, **kw):
    collect = prepare_jac_rows(vislam, P, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, P, samples, tframe, prev, carry=None, where=None):
    got = jac_rows_on_device(vislam, c, P, samples, tframe, prev, carry)
    want = jr.preintegrate_jac_rows(P, samples, tframe, prev, carry)
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(prev)) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[1].tobytes() == want[1].tobytes(), (where, [i for i in range(len(prev)) if got[1][i].tobytes() != want[1][i].tobytes()][:5])
    assert got[2].tobytes() == want[2].tobytes(), (where, np.argwhere(got[2] != want[2])[:5])
    assert got[3].tobytes() == want[3].tobytes(), (where, got[3], want[3])
    # the sibling on the same device inputs: the same delta, rotation and carried delta
    sib = rows_on_device(vislam, c, P, samples, tframe, prev, carry["carry"] if carry is not None else None)
    assert sib[0].tobytes() == got[0].tobytes() and sib[1].tobytes() == got[2].tobytes() and sib[2].tobytes() == got[3]["carry"].tobytes(), where
    assert jac_finite(got[1], got[3]) and zero_beside_a_voided_delta(got[0], got[1])
    return want


@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        cj = jc(carry)
        if carry is not None and int(carry[0]["valid"]) & ir.IMU_CARRY_OPEN:       # the open delta's own Jacobians
            t = float(carry[0]["t_last"])
            cj[0]["open_jac"] = jr.preintegrate_jac(ic.params(), ic.samples_between(t - 0.3, t + 0.1, 200.0), t - 0.21, t)[1]
            cj[0]["open_jac"]["q"] = 0
        d, j, rot, c = check(vislam, ctx, ic.params(), s, tf, prev, cj, where=(n, name))
        assert not j["flags"].any() and (j["q"] == d["q"]).all()
    prev = ic.pairing(name, n, ir.KF_CARRIED)                          # a carried pair without a record
    d, j, _, _ = check(vislam, ctx, ic.params(), s, tf, prev, None, where=(n, name, "no carry"))
    assert int(d[0]["flags"]) == ir.IMU_NO_CARRY and not any(j[0][b].any() for b in jr.BLOCKS)


def test_more_than_the_maximum_is_refused(vislam, ctx):
    import torch
    buf = _dev(torch, np.zeros(1025 * 296, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_preintegrate_jac_rows(1025, buf.data_ptr(), 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4                                          # VIS_E_CAPACITY
    out = _dev(torch, np.zeros(1025 * 216, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_correct_rows(1025, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), out.data_ptr())
    assert e.value.code == -4


@pytest.mark.parametrize("per_interval", (0, 1, 2, 10, 100))
def test_samples_per_interval(vislam, ctx, per_interval):
    s, tf, tb = ic.stream(12, per_interval)
    for P in (ir.Params(), ic.params()):
        for name in ("chain", "alternate", "long"):
            check(vislam, ctx, P, s, tf, ic.pairing(name, 12, ir.KF_CARRIED), jc(ic.carried(tb, False)), where=(per_interval, name))


def test_without_rotations_and_without_a_carry_out(vislam, ctx):
    s, tf, tb = ic.stream(9, 10)
    prev = ic.pairing("alternate", 9, ir.KF_CARRIED)
    want = jr.preintegrate_jac_rows(ic.params(), s, tf, prev, jc(ic.carried(tb, True)))
    got = jac_rows_on_device(vislam, ctx, ic.params(), s, tf, prev, jc(ic.carried(tb, True)), want_rot=False, want_carry=False)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].size == 0 and got[3].size == 0
    unsaved = np.full(7, ir.KF_NOT_SAVED, np.int32)                    # nothing saved: the open delta and its Jacobians are carried on
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        d, j, _, c = check(vislam, ctx, ic.params(), s, tf[:7], unsaved, jc(carry))
        assert (d["flags"] == ir.IMU_NO_PAIR).all() and int(c["carry"]["valid"][0]) == ir.IMU_CARRY_TIME | ir.IMU_CARRY_OPEN
        assert bool(c["open_jac"]["Jva"].any()) == (carry is not None)  # (without a carried time the open delta is VIS_IMU_NO_START: zero Jacobians)


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(vislam, ctx, case):
    name, s, tf, prev, carry, must, _ = case
    d, j, rot, c = check(vislam, ctx, ir.Params(), s, tf, prev, jc(carry), where=name)
    assert ic.all_finite(d, rot, c["carry"])
    for i, f in must.items():
        assert int(d[i]["flags"]) & f == f, (name, i)


def test_an_overflowing_carried_jacobian_is_flagged_and_the_flag_is_sticky(vislam, ctx):
    s, tf, tb = ic.stream(6, 10)
    chain = ic.pairing("chain", 6, ir.KF_CARRIED)
    c = jc(ic.carried(tb, True))
    c[0]["open_jac"]["Jpg"][:], c[0]["open_jac"]["Jvg"][:] = 1.79e308, 1.79e308
    d, j, _, _ = check(vislam, ctx, ic.params(), s, tf, chain, c)
    assert int(d[0]["flags"]) == 0 and int(j[0]["flags"]) == jr.IMU_JAC_NONFINITE and not j["flags"][1:].any()
    c[0]["open_jac"]["Jpg"][:], c[0]["open_jac"]["Jvg"][:] = 0.0, 0.0
    c[0]["open_jac"]["Jva"][4] = float("nan")
    unsaved = np.full(3, ir.KF_NOT_SAVED, np.int32)
    _, _, _, c1 = check(vislam, ctx, ic.params(), s, tf[:3], unsaved, c)
    assert int(c1["open_jac"]["flags"][0]) == jr.IMU_JAC_NONFINITE and int(c1["carry"]["open"]["flags"][0]) == 0
    d2, j2, _, _ = check(vislam, ctx, ic.params(), s, tf[3:], ic.pairing("chain", 3, ir.KF_CARRIED), c1)
    assert int(j2[0]["flags"]) == jr.IMU_JAC_NONFINITE and int(d2[0]["flags"]) == 0 and not j2["flags"][1:].any()


def test_the_host_form_is_row_0_of_a_one_frame_call(vislam, ctx):
    s, tf, tb = ic.stream(3, 10)
    for P in (ir.Params(), ic.params()):
        for t_a, t_b in ((tb, float(tf[0])), (float(tf[0]), float(tf[2])), (float(tf[1]), float(tf[1])), (ic.T0 - 1.0, ic.T0 - 0.5)):
            d, j, rot = ctx.imu_preintegrate_jac(s, t_a, t_b, ip=ic.struct_params(vislam, P))
            want = jr.preintegrate_jac(P, s, t_a, t_b)
            sib = ctx.imu_preintegrate(s, t_a, t_b, ip=ic.struct_params(vislam, P))
            assert d.tobytes() == want[0].tobytes() == sib[0].tobytes() and j.tobytes() == want[1].tobytes()
            assert rot.tobytes() == want[2].tobytes() == sib[1].tobytes()
    d, j, rot = ctx.imu_preintegrate_jac(s[:0], 1.0, 2.0)
    assert int(d["flags"]) == ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED and float(d["dt"]) == 1.0 and not any(j[b].any() for b in jr.BLOCKS) and int(j["flags"]) == 0


# ---- the correction
def correct_on_device(vislam, c, P, delta, jac, dbg, dba=None, dbg_in_align_record=False, want_rot=True, want_status=True):
    import torch
    n = len(delta)
    d_delta, d_jac = _dev(torch, np.asarray(delta, jr.ir.DELTA_DTYPE)), _dev(torch, np.asarray(jac, jr.JAC_DTYPE))
    if dbg_in_align_record:                                            # the first 24 bytes of a vis_vi_align record are its dbg
        rec = np.zeros(1, vislam.VI_ALIGN_DTYPE)
        rec[0]["dbg"], rec[0]["c0"], rec[0]["s"] = dbg, 123.0, 2.5
        assert rec.dtype.fields["dbg"][1] == 0
        d_dbg = _dev(torch, rec)
    else:
        d_dbg = _dev(torch, np.asarray(dbg, np.float64))
    d_dba = _dev(torch, np.asarray(dba, np.float64)) if dba is not None else None
    out, rot, st = _guarded(torch, n * 216), _guarded(torch, n * 36), _guarded(torch, n * 4)
    c.imu_correct_rows(n, d_delta.data_ptr(), d_jac.data_ptr(), d_dbg.data_ptr(), out.data_ptr() + GUARD, d_dba.data_ptr() if dba is not None else 0,
                       rot.data_ptr() + GUARD if want_rot else 0, st.data_ptr() + GUARD if want_status else 0, ip=ic.struct_params(vislam, P))
    c.batch_sync()
    return (_payload(out, n * 216).view(vislam.IMU_DELTA_DTYPE), _payload(rot, n * 36 if want_rot else 0).view(np.float32).reshape(-1, 9),
            _payload(st, n * 4 if want_status else 0).view(np.int32))


@pytest.fixture(scope="module")
def records():
    """1024 records with pairs of every length around the powers of two, the status cases spliced in at the wave edges"""
    s, tf, tb = ic.stream(1024, 2)
    d, j, _, _ = jr.preintegrate_jac_rows(ic.params(), s, tf, ic.pairing("straddle", 1024, ir.KF_CARRIED), jc(ic.carried(tb, True)))
    sd, sj, dbg, dba, _, _ = correction_status_cases()
    for at in (0, 60, 1016):
        d[at:at + 8], j[at:at + 8] = sd, sj
    return d, j, dbg, dba


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1024))
def test_the_correction_against_the_restatement(vislam, ctx, records, n):
    d, j, big_dbg, big_dba = records
    P = ic.params()
    seen = set()
    for dbg, dba in ((DBG, None), (DBG, DBA), (big_dbg, big_dba), ((0.0, 0.0, 0.0), DBA)):
        want = jr.correct_rows(P, d[:n], j[:n], dbg, dba)
        got = correct_on_device(vislam, ctx, P, d[:n], j[:n], dbg, dba)
        for k in range(3):
            assert got[k].tobytes() == want[k].tobytes(), (n, dbg, dba, k, np.argwhere(got[2] != want[2])[:5])
        assert np.isfinite(got[1]).all()
        seen |= set(got[2].tolist())
    if n >= 63:
        assert seen == {jr.IMC_OK, jr.IMC_UNUSABLE, jr.IMC_JAC, jr.IMC_ANGLE, jr.IMC_NONFINITE}, seen


def test_the_correction_reads_dbg_from_an_alignment_record_and_refuses_to_alias(vislam, ctx, records):
    d, j, _, _ = records
    P = ic.params()
    want = jr.correct_rows(P, d[:65], j[:65], DBG, None)
    got = correct_on_device(vislam, ctx, P, d[:65], j[:65], DBG, None, dbg_in_align_record=True)
    assert all(got[k].tobytes() == want[k].tobytes() for k in range(3))
    got = correct_on_device(vislam, ctx, P, d[:65], j[:65], DBG, None, want_rot=False, want_status=False)
    assert got[0].tobytes() == want[0].tobytes() and got[1].size == 0 and got[2].size == 0
    for bad in (float("nan"), float("inf")):                           # a bias that is not finite copies every record
        want = jr.correct_rows(P, d[:65], j[:65], (0.0, bad, 0.0), DBA)
        got = correct_on_device(vislam, ctx, P, d[:65], j[:65], (0.0, bad, 0.0), DBA)
        assert all(got[k].tobytes() == want[k].tobytes() for k in range(3)) and got[0].tobytes() == d[:65].tobytes()
        assert set(got[2].tolist()) == {jr.IMC_BIAS, jr.IMC_UNUSABLE, jr.IMC_JAC}
    import torch
    buf = _dev(torch, np.zeros(4 * 296, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_correct_rows(4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -1                                          # VIS_E_INVALID: d_delta_out is d_delta
