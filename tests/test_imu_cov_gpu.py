"""GPU: vis_imu_preintegrate_cov_rows and vis_imu_preintegrate_cov against the restatement tests/imu_cov_ref.py, BYTE FOR BYTE: d_delta, d_cov, d_rot
and d_carry_out.  Every output sits between 0xEE guards that must keep their bytes.  The delta row is also checked against vis_imu_preintegrate_rows
on the same device inputs: a covariance never changes a delta.

n = 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024 (1025 is refused) with the four pairings of tests/imu_cases.py, each with a carry that has an open delta
(and its covariance), one that holds a time alone, and none; 0, 1, 2, 10 and 100 samples per interval at n = 12 and two an interval at n = 1024 (the
restatement is plain Python); the hostile rows; an overflowing carried covariance beside a finite delta; densities of zero; the host form."""
import numpy as np
import pytest

import imu_cases as ic
import imu_cov_ref as cr
import imu_ref as ir
from test_imu_cov_ref import NOISE, cc, cov_finite, zero_beside_a_voided_delta
from test_imu_gpu import GUARD, _dev, _guarded, _payload, rows_on_device

pytestmark = pytest.mark.gpu


def struct_noise(vislam, noise):
    z = vislam.default_imu_noise()
    z.sigma_g, z.sigma_a = noise.sigma_g, noise.sigma_a
    return z


def prepare_cov_rows(vislam, P, noise, samples, tframe, prev, carry=None, want_rot=True, want_carry=True):
    """test_imu_gpu.prepare_rows for vis_imu_preintegrate_cov_rows; carry: a COV_CARRY record or None.  call(c) queues the call and answers
    collect() -> (d_delta, d_cov, d_rot (n, 9), d_carry_out), for after a synchronise"""
    import torch
    n = len(tframe)
    keep = [_dev(torch, np.asarray(samples, ir.SAMPLE_DTYPE)), _dev(torch, np.asarray(tframe, np.float64)), _dev(torch, np.asarray(prev, np.int32))]
    d_carry = _dev(torch, np.asarray(carry, cr.COV_CARRY_DTYPE).reshape(1)) if carry is not None else None
    delta, cov, rot, cout = _guarded(torch, n * 216), _guarded(torch, n * 368), _guarded(torch, n * 36), _guarded(torch, 600)

    def collect():
        return (_payload(delta, n * 216).view(vislam.IMU_DELTA_DTYPE), _payload(cov, n * 368).view(vislam.IMU_COV_DTYPE),
                _payload(rot, n * 36 if want_rot else 0).view(np.float32).reshape(-1, 9), _payload(cout, 600 if want_carry else 0).view(vislam.IMU_COV_CARRY_DTYPE))

    def call(c):
        c.imu_preintegrate_cov_rows(n, keep[0].data_ptr() if len(samples) else 0, len(samples), keep[1].data_ptr(), keep[2].data_ptr(), delta.data_ptr() + GUARD,
                                    cov.data_ptr() + GUARD, rot.data_ptr() + GUARD if want_rot else 0, d_carry.data_ptr() if carry is not None else 0,
                                    cout.data_ptr() + GUARD if want_carry else 0, ip=ic.struct_params(vislam, P), noise=struct_noise(vislam, noise))
        return collect
    return call


def cov_rows_on_device(vislam, c, P, noise, *rows, **kw):
    collect = prepare_cov_rows(vislam, P, noise, *rows, **kw)(c)
    c.batch_sync()
    return collect()


_TABLES = {}


def big_table(n, carried_time):
    """the restatement's lifting table of ic.stream(n, 2) under ic.params() and NOISE, built once per module: it depends on the carried TIME alone"""
    key = (n, carried_time)
    if key not in _TABLES:
        s, tf, tb = ic.stream(n, 2)
        _TABLES[key] = cr.lifting_table(cr.intervals(ic.params(), NOISE, s, tf, cc(ic.carried(tb, False)) if carried_time else None), n)
    return _TABLES[key]


def check(vislam, c, P, samples, tframe, prev, carry=None, where=None, noise=NOISE, table=None):
    got = cov_rows_on_device(vislam, c, P, noise, samples, tframe, prev, carry)
    want = cr.preintegrate_cov_rows(P, noise, samples, tframe, prev, carry, table=table)
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(prev)) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[1].tobytes() == want[1].tobytes(), (where, [i for i in range(len(prev)) if got[1][i].tobytes() != want[1][i].tobytes()][:5])
    assert got[2].tobytes() == want[2].tobytes(), (where, np.argwhere(got[2] != want[2])[:5])
    assert got[3].tobytes() == want[3].tobytes(), (where, got[3], want[3])
    # the sibling on the same device inputs: the same delta, rotation and carried delta
    sib = rows_on_device(vislam, c, P, samples, tframe, prev, carry["carry"] if carry is not None else None)
    assert sib[0].tobytes() == got[0].tobytes() and sib[1].tobytes() == got[2].tobytes() and sib[2].tobytes() == got[3]["carry"].tobytes(), where
    assert cov_finite(got[1], got[3]) and zero_beside_a_voided_delta(got[0], got[1])
    return want


def open_carry(carry):
    """the COV_CARRY record of an imu_cases carry, with the open delta's own covariance"""
    c = cc(carry)
    if carry is not None and int(carry[0]["valid"]) & ir.IMU_CARRY_OPEN:
        t = float(carry[0]["t_last"])
        c[0]["open_cov"] = cr.preintegrate_cov(ic.params(), NOISE, ic.samples_between(t - 0.3, t + 0.1, 200.0), t - 0.21, t)[1]
        c[0]["open_cov"]["q"] = 0
    return c


@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        table = big_table(n, carry is not None) if n > 65 else None
        d, q, rot, c = check(vislam, ctx, ic.params(), s, tf, prev, open_carry(carry), where=(n, name), table=table)
        assert not q["flags"].any() and (q["q"] == d["q"]).all()
    prev = ic.pairing(name, n, ir.KF_CARRIED)                          # a carried pair without a record
    d, q, _, _ = check(vislam, ctx, ic.params(), s, tf, prev, None, where=(n, name, "no carry"), table=big_table(n, False) if n > 65 else None)
    assert int(d[0]["flags"]) == ir.IMU_NO_CARRY and not q[0]["S"].any()


def test_more_than_the_maximum_is_refused(vislam, ctx):
    import torch
    buf = _dev(torch, np.zeros(1025 * 368, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_preintegrate_cov_rows(1025, buf.data_ptr(), 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4                                          # VIS_E_CAPACITY


@pytest.mark.parametrize("per_interval", (0, 1, 2, 10, 100))
def test_samples_per_interval(vislam, ctx, per_interval):
    s, tf, tb = ic.stream(12, per_interval)
    for P in (ir.Params(), ic.params()):
        for name in ("chain", "alternate", "long"):
            check(vislam, ctx, P, s, tf, ic.pairing(name, 12, ir.KF_CARRIED), cc(ic.carried(tb, False)), where=(per_interval, name))


def test_without_rotations_and_without_a_carry_out(vislam, ctx):
    s, tf, tb = ic.stream(9, 10)
    prev = ic.pairing("alternate", 9, ir.KF_CARRIED)
    want = cr.preintegrate_cov_rows(ic.params(), NOISE, s, tf, prev, open_carry(ic.carried(tb, True)))
    got = cov_rows_on_device(vislam, ctx, ic.params(), NOISE, s, tf, prev, open_carry(ic.carried(tb, True)), want_rot=False, want_carry=False)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].size == 0 and got[3].size == 0
    unsaved = np.full(7, ir.KF_NOT_SAVED, np.int32)                    # nothing saved: the open delta and its covariance are carried on
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        d, q, _, c = check(vislam, ctx, ic.params(), s, tf[:7], unsaved, open_carry(carry))
        assert (d["flags"] == ir.IMU_NO_PAIR).all() and int(c["carry"]["valid"][0]) == ir.IMU_CARRY_TIME | ir.IMU_CARRY_OPEN
        assert bool(c["open_cov"]["S"].any()) == (carry is not None)   # (without a carried time the open delta is VIS_IMU_NO_START: no covariance)


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(vislam, ctx, case):
    name, s, tf, prev, carry, must, _ = case
    d, q, rot, c = check(vislam, ctx, ir.Params(), s, tf, prev, cc(carry), where=name)
    assert ic.all_finite(d, rot, c["carry"])
    for i, f in must.items():
        assert int(d[i]["flags"]) & f == f, (name, i)


def test_an_overflowing_carried_covariance_is_flagged_and_the_flag_is_sticky(vislam, ctx):
    s, tf, tb = ic.stream(6, 10)
    chain = ic.pairing("chain", 6, ir.KF_CARRIED)
    c = cc(ic.carried(tb, True))
    c[0]["open_cov"]["S"][:] = 1.79e308
    d, q, _, _ = check(vislam, ctx, ic.params(), s, tf, chain, c)
    assert int(d[0]["flags"]) == 0 and int(q[0]["flags"]) == cr.IMU_COV_NONFINITE and not q["flags"][1:].any()
    c[0]["open_cov"]["S"][:] = 0.0
    c[0]["open_cov"]["S"][17] = float("nan")
    unsaved = np.full(3, ir.KF_NOT_SAVED, np.int32)
    _, _, _, c1 = check(vislam, ctx, ic.params(), s, tf[:3], unsaved, c)
    assert int(c1["open_cov"]["flags"][0]) == cr.IMU_COV_NONFINITE and int(c1["carry"]["open"]["flags"][0]) == 0
    d2, q2, _, _ = check(vislam, ctx, ic.params(), s, tf[3:], ic.pairing("chain", 3, ir.KF_CARRIED), c1)
    assert int(q2[0]["flags"]) == cr.IMU_COV_NONFINITE and int(d2[0]["flags"]) == 0 and not q2["flags"][1:].any()
    # densities whose squares overflow flag every covariance of the call and leave every delta alone
    d, q, _, _ = check(vislam, ctx, ic.params(), s, tf, chain, cc(ic.carried(tb, True)), noise=cr.Noise(1e200, 1e200))
    assert (q["flags"] == cr.IMU_COV_NONFINITE).all() and not d["flags"].any()


def test_zero_densities_and_a_power_of_two(vislam, ctx):
    s, tf, tb = ic.stream(65, 10)
    prev = ic.pairing("straddle", 65, ir.KF_CARRIED)
    carry = open_carry(ic.carried(tb, True))
    _, q0, _, c0 = check(vislam, ctx, ic.params(), s, tf, prev, cc(ic.carried(tb, True)), noise=cr.Noise(0.0, 0.0))
    assert not q0["S"].any() and not c0["open_cov"]["S"].any()
    _, q1, _, _ = check(vislam, ctx, ic.params(), s, tf, prev, carry)
    _, q2, _, _ = check(vislam, ctx, ic.params(), s, tf, prev, carry, noise=cr.Noise(2 * cr.SIGMA_G, 2 * cr.SIGMA_A))
    assert (q2["S"][1:] == 4.0 * q1["S"][1:]).all() and q1["S"][1:].any(axis=1).all()        # (frame 0 holds the carried covariance, which was not scaled)


def test_the_host_form_is_row_0_of_a_one_frame_call(vislam, ctx):
    s, tf, tb = ic.stream(3, 10)
    for P in (ir.Params(), ic.params()):
        for t_a, t_b in ((tb, float(tf[0])), (float(tf[0]), float(tf[2])), (float(tf[1]), float(tf[1])), (ic.T0 - 1.0, ic.T0 - 0.5)):
            d, q, rot = ctx.imu_preintegrate_cov(s, t_a, t_b, ip=ic.struct_params(vislam, P))
            want = cr.preintegrate_cov(P, NOISE, s, t_a, t_b)
            sib = ctx.imu_preintegrate(s, t_a, t_b, ip=ic.struct_params(vislam, P))
            assert d.tobytes() == want[0].tobytes() == sib[0].tobytes() and q.tobytes() == want[1].tobytes()
            assert rot.tobytes() == want[2].tobytes() == sib[1].tobytes()
    d, q, rot = ctx.imu_preintegrate_cov(s[:0], 1.0, 2.0)
    assert int(d["flags"]) == ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED and float(d["dt"]) == 1.0 and not q["S"].any() and int(q["flags"]) == 0


# ---- the inertial factor
def factor_on_device(vislam, c, P, FP, prev, traj, delta, cov, state, result, ba_record=False):
    import torch
    import vi_align_cases as vc
    n = len(prev)
    keep = [_dev(torch, np.asarray(prev, np.int32)), _dev(torch, traj), _dev(torch, np.asarray(delta, ir.DELTA_DTYPE)), _dev(torch, np.asarray(cov, cr.COV_DTYPE)),
            _dev(torch, state)]
    if ba_record:                                                      # the head of a vis_vi_align_ba record is a vis_vi_align record
        rec = np.zeros(1, vislam.VI_ALIGN_BA_DTYPE)
        rec[0]["a"], rec[0]["dba"], rec[0]["g_ba"] = np.asarray(result).reshape(-1)[0], 7.0, 123.0
        assert rec.dtype.fields["a"][1] == 0
        d_res = _dev(torch, rec)
    else:
        d_res = _dev(torch, np.asarray(result).reshape(-1)[:1])
    out = _guarded(torch, n * 96)
    fp = vislam.default_imu_factor_params()
    fp.var_rot, fp.var_v, fp.var_p = FP.var_rot, FP.var_v, FP.var_p
    c.imu_factor_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), d_res.data_ptr(),
                      out.data_ptr() + GUARD, vp=vc.struct_params(vislam, P), fp=fp)
    c.batch_sync()
    return _payload(out, n * 96).view(vislam.IMU_FACTOR_DTYPE)


@pytest.fixture(scope="module")
def factor_rows_1024():
    """1024 chained frames of the planted motion: closed-form deltas, the covariances of the 40 integrated pairs repeated, the true states; every
    flag's constructed row among the first 40; and the restatement's records, without and with variances on the diagonal"""
    import imu_factor_ref as fr
    import vi_align_cases as vc
    import vi_align_ref as vr
    from test_imu_factor_ref import flag_cases, planted
    small, sc = planted(), vc.scene(1024, "chain", "none", integrate=False)
    cov = np.zeros(1024, cr.COV_DTYPE)
    state = np.zeros(1024, vr.STATE_DTYPE)
    for i in range(1024):
        cov[i] = small["cov"][1 + i % 39]
        cov[i]["q"] = sc["delta"][i]["q"]
        p, v, _ = vc.motion(float(sc["times"][i]))
        state[i]["p"], state[i]["v"], state[i]["flags"], state[i]["q"] = p, v, vr.VIS_HAS_P | vr.VIS_HAS_V, sc["delta"][i]["q"]
    cov[0]["S"], cov[0]["q"] = 0.0, sc["delta"][0]["q"]
    prev, traj, delta, cov, state, want = flag_cases(dict(sc, cov=cov, true_state=state))
    rows = dict(P=sc["P"], prev=prev, traj=traj, delta=delta, cov=cov, state=state, result=small["true_result"], want=want)
    fps = (fr.FactorParams(), fr.FactorParams(1e-8, 1e-6, 1e-8))
    rows["expected"] = [fr.factor_rows(sc["P"], FP, prev, traj, delta, cov, state, small["true_result"]) for FP in fps]
    rows["fps"] = fps
    return rows


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1024))
def test_the_factor_against_the_restatement(vislam, ctx, factor_rows_1024, n):
    import imu_factor_ref as fr
    R = factor_rows_1024
    seen = 0
    for FP, want in zip(R["fps"], R["expected"]):
        got = factor_on_device(vislam, ctx, R["P"], FP, *(R[k][:n] for k in ("prev", "traj", "delta", "cov", "state")), R["result"])
        assert got.tobytes() == want[:n].tobytes(), (n, [i for i in range(n) if got[i].tobytes() != want[i].tobytes()][:5])
        assert np.isfinite(got["r"]).all() and np.isfinite(got["chi2"]).all()
        for f in got["flags"]:
            seen |= int(f)
    if n >= 63:
        assert seen == fr.IMF_NO_PARENT | fr.IMF_NO_STATE | fr.IMF_UNUSABLE | fr.IMF_SINGULAR | fr.IMF_NONFINITE
        assert all(int(R["expected"][0][i]["flags"]) == f for i, f in R["want"].items()) and (R["expected"][0]["chi2"][40:n] > 0).all()


def test_the_factor_reads_a_ba_record_and_a_failed_alignment_flags_every_pair(vislam, ctx, factor_rows_1024):
    import imu_factor_ref as fr
    import vi_align_ref as vr
    R = factor_rows_1024
    rows = [R[k][:65] for k in ("prev", "traj", "delta", "cov", "state")]
    got = factor_on_device(vislam, ctx, R["P"], R["fps"][0], *rows, R["result"], ba_record=True)
    assert got.tobytes() == R["expected"][0][:65].tobytes()
    bad = R["result"].copy()
    bad[0]["flags"] = vr.VIA_SCALE
    got = factor_on_device(vislam, ctx, R["P"], R["fps"][0], *rows, bad)
    want = fr.factor_rows(R["P"], R["fps"][0], *rows, bad)
    assert got.tobytes() == want.tobytes() and not got["r"].any() and ((got["flags"] & fr.IMF_NO_ALIGN) != 0).sum() >= 60
    import torch
    buf = _dev(torch, np.zeros(1025 * 368, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_factor_rows(1025, *([buf.data_ptr()] * 7))
    assert e.value.code == -4                                          # VIS_E_CAPACITY
