"""GPU: vis_imu_preintegrate_rows and vis_imu_preintegrate against the restatement tests/imu_ref.py, BYTE FOR BYTE: d_delta, d_rot and
d_carry_out.  Every output sits between 0xEE guards that must keep their bytes.

n = 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024 (1025 is refused) with the chain, every second frame unsaved, one keyframe with n - 2 unsaved frames and
a saved last frame (pair length n - 1) and pair lengths straddling the powers of two; each with a carry that has an open delta, one that holds a
time alone, and none; 0, 1, 2, 10 and 100 samples per interval; non-trivial bg, ba and r_ic; the hostile rows of tests/imu_cases.py; the host
form against row 0 of a one-frame rows call."""
import numpy as np
import pytest

import imu_cases as ic
import imu_ref as ir

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


def prepare_rows(vislam, P, samples, tframe, prev, carry=None, want_rot=True, want_carry=True):
    """the inputs of one vis_imu_preintegrate_rows uploaded and its outputs filled (both synchronise the device); the answer is call(c), which queues
    the call on context c and synchronises nothing.  call(c) answers collect() -> (d_delta, d_rot (n, 9), d_carry_out), for after a synchronise: it
    checks the guards around all three"""
    import torch
    n = len(tframe)
    keep = [_dev(torch, np.asarray(samples, ir.SAMPLE_DTYPE)), _dev(torch, np.asarray(tframe, np.float64)), _dev(torch, np.asarray(prev, np.int32))]
    d_carry = _dev(torch, np.asarray(carry, ir.CARRY_DTYPE).reshape(1)) if carry is not None else None
    delta, rot, cout = _guarded(torch, n * 216), _guarded(torch, n * 36), _guarded(torch, 232)

    def collect():
        return (_payload(delta, n * 216).view(vislam.IMU_DELTA_DTYPE), _payload(rot, n * 36 if want_rot else 0).view(np.float32).reshape(-1, 9),
                _payload(cout, 232 if want_carry else 0).view(vislam.IMU_CARRY_DTYPE))

    def call(c):
        c.imu_preintegrate_rows(n, keep[0].data_ptr() if len(samples) else 0, len(samples), keep[1].data_ptr(), keep[2].data_ptr(), delta.data_ptr() + GUARD,
                                rot.data_ptr() + GUARD if want_rot else 0, d_carry.data_ptr() if carry is not None else 0,
                                cout.data_ptr() + GUARD if want_carry else 0, ip=ic.struct_params(vislam, P))
        return collect
    return call


def rows_on_device(vislam, c, P, *rows, **kw):
    """(d_delta, d_rot (n, 9), d_carry_out) of one vis_imu_preintegrate_rows, the guards around all three checked"""
    collect = prepare_rows(vislam, P, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, P, samples, tframe, prev, carry=None, where=None):
    got = rows_on_device(vislam, c, P, samples, tframe, prev, carry)
    want = ir.preintegrate_rows(P, samples, tframe, prev, carry)
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(prev)) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[1].tobytes() == want[1].tobytes(), (where, np.argwhere(got[1] != want[1])[:5])
    assert got[2].tobytes() == want[2].tobytes(), (where, got[2], want[2])
    return want


@pytest.mark.parametrize("name", ic.PAIRINGS)
@pytest.mark.parametrize("n", ic.NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    s, tf, tb = ic.stream(n, 2 if n > 65 else 10)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        prev = ic.pairing(name, n, ir.KF_CARRIED if carry is not None else ir.KF_FIRST)
        d, rot, c = check(vislam, ctx, ic.params(), s, tf, prev, carry, where=(n, name))
        assert ic.all_finite(d, rot, c) and not (d["flags"][1:] & ~ir.IMU_NO_PAIR).any()
        if name == "long" and n > 2:
            assert int(d[n - 1]["q"]) == 0 and int(d[n - 1]["n_steps"]) >= n - 1
    prev = ic.pairing(name, n, ir.KF_CARRIED)                          # a carried pair without a record
    d, rot, _ = check(vislam, ctx, ic.params(), s, tf, prev, None, where=(n, name, "no carry"))
    assert int(d[0]["flags"]) == ir.IMU_NO_CARRY


def test_more_than_the_maximum_is_refused(vislam, ctx):
    import torch
    buf = _dev(torch, np.zeros(1025 * 216, np.uint8))
    with pytest.raises(vislam.VisError) as e:
        ctx.imu_preintegrate_rows(1025, buf.data_ptr(), 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4                                          # VIS_E_CAPACITY


@pytest.mark.parametrize("per_interval", (0, 1, 2, 10, 100))
def test_samples_per_interval(vislam, ctx, per_interval):
    s, tf, tb = ic.stream(12, per_interval)
    for P in (ir.Params(), ic.params()):
        for name in ("chain", "alternate", "long"):
            d, _, _ = check(vislam, ctx, P, s, tf, ic.pairing(name, 12, ir.KF_CARRIED), ic.carried(tb, False), where=(per_interval, name))
    chain = ir.preintegrate_rows(ir.Params(), s, tf, ic.pairing("chain", 12, ir.KF_CARRIED), ic.carried(tb, False))[0]
    if per_interval == 0:
        assert (chain["flags"] & ir.IMU_EMPTY).sum() >= 6 and (chain["n_steps"] <= 2).all()   # (samples three frame intervals apart)
    else:
        assert (chain["n_steps"] == per_interval + 1).all() and not (chain["flags"] & ir.IMU_EMPTY).any()


def test_without_rotations_and_without_a_carry_out(vislam, ctx):
    s, tf, tb = ic.stream(9, 10)
    prev = ic.pairing("alternate", 9, ir.KF_CARRIED)
    want = ir.preintegrate_rows(ic.params(), s, tf, prev, ic.carried(tb, True))
    got = rows_on_device(vislam, ctx, ic.params(), s, tf, prev, ic.carried(tb, True), want_rot=False, want_carry=False)
    assert got[0].tobytes() == want[0].tobytes() and got[1].size == 0 and got[2].size == 0
    none = np.zeros(1, ir.CARRY_DTYPE)                                 # a record without VIS_IMU_CARRY_TIME counts as none
    d, _, _ = check(vislam, ctx, ic.params(), s, tf, prev, none)
    assert int(d[0]["flags"]) == ir.IMU_NO_CARRY


def test_nothing_saved_carries_the_open_delta_on(vislam, ctx):
    s, tf, tb = ic.stream(7, 10)
    unsaved = np.full(7, ir.KF_NOT_SAVED, np.int32)
    for carry in (None, ic.carried(tb, True), ic.carried(tb, False)):
        d, _, c = check(vislam, ctx, ic.params(), s, tf, unsaved, carry)
        assert (d["flags"] == ir.IMU_NO_PAIR).all() and int(c["valid"][0]) == ir.IMU_CARRY_TIME | ir.IMU_CARRY_OPEN


@pytest.mark.parametrize("case", ic.hostile(), ids=lambda c: c[0])
def test_hostile_rows(vislam, ctx, case):
    name, s, tf, prev, carry, must, _ = case
    d, rot, c = check(vislam, ctx, ir.Params(), s, tf, prev, carry, where=name)
    assert ic.all_finite(d, rot, c)
    for i, f in must.items():
        assert int(d[i]["flags"]) & f == f, (name, i)


def test_the_host_form_is_row_0_of_a_one_frame_call(vislam, ctx):
    s, tf, tb = ic.stream(3, 10)
    for P in (ir.Params(), ic.params()):
        for t_a, t_b in ((tb, float(tf[0])), (float(tf[0]), float(tf[2])), (float(tf[1]), float(tf[1])), (ic.T0 - 1.0, ic.T0 - 0.5)):
            d, rot = ctx.imu_preintegrate(s, t_a, t_b, ip=ic.struct_params(vislam, P))
            c = np.zeros(1, ir.CARRY_DTYPE)
            c[0]["t_last"], c[0]["valid"] = t_a, ir.IMU_CARRY_TIME
            rows = rows_on_device(vislam, ctx, P, s, [t_b], [ir.KF_CARRIED], c)
            want = ir.preintegrate(P, s, t_a, t_b)
            assert d.tobytes() == rows[0][0].tobytes() == want[0].tobytes() and rot.tobytes() == rows[1][0].tobytes() == want[1].tobytes()
    d, rot = ctx.imu_preintegrate(s[:0], 1.0, 2.0)
    assert int(d["flags"]) == ir.IMU_EMPTY | ir.IMU_EXTRAPOLATED and float(d["dt"]) == 1.0 and (rot == np.eye(3, dtype=np.float32)).all()
