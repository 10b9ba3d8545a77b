"""GPU: vis_trajectory_rows against the restatement tests/trajectory_ref.py, BYTE FOR BYTE: the records and the dense poses.  Output buffers are
pre-filled with 0xEE and everything behind the written extent must keep it.

n = 1, 2, 3, 4, 5, 33, 64, 65, 257 (every round count up to nine; 257 is beyond the 256 frames whose states fit in LDS) with a plain chain, a gated
pairing with VIS_KF_NOT_SAVED runs, a pose-less frame in the middle, a link in the middle that is not VIS_SL_OK, two children of one root; a
carried record and none; same_epoch_only 0 and 1; a sigma product that overflows; and the device's doubling against the sequential composition
within 16 x the bound tests/test_trajectory_ref.py measured."""
import numpy as np
import pytest

import scale_link_ref as sl
import trajectory_ref as tj
from test_trajectory_ref import DOUBLING_BOUND, NS, PAIRINGS, assert_same_but_rounding, carried_record, overflowing, pairing, path_lengths

pytestmark = pytest.mark.gpu
FILL = 0xEE


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def prepare_chain(vislam, prev, pose, link, carry=None, seq0=0, same_epoch_only=True, dense=True):
    """the inputs of one vis_trajectory_rows uploaded and its outputs filled (both synchronise the device); the answer is call(c), which queues the
    call on context c and synchronises nothing.  call(c) answers collect() -> (records (n), d_poses (n, 12) or None), for after a synchronise: it
    checks the guard bytes behind both outputs"""
    import torch
    n = len(prev)
    keep = [_dev(torch, a) for a in (np.asarray(prev, np.int32), pose, link)]
    d_carry = _dev(torch, np.asarray(carry, tj.TRAJ_DTYPE).reshape(1)) if carry is not None else None
    rec, poses = _filled(torch, (n + 2) * 128), _filled(torch, (n * 12 + 5) * 8)

    def collect():
        rr, rp = rec.cpu().numpy(), poses.cpu().numpy()
        assert (rr[n * 128:] == FILL).all() and (rp[n * 96 if dense else 0:] == FILL).all()
        return rr[:n * 128].view(vislam.TRAJ_POSE_DTYPE), rp[:n * 96].view(np.float64).reshape(n, 12) if dense else None

    def call(c):
        c.trajectory_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), rec.data_ptr(), poses.data_ptr() if dense else 0,
                          d_carry.data_ptr() if carry is not None else 0, seq0, same_epoch_only)
        return collect
    return call


def chain_on_device(vislam, c, *rows, **kw):
    """(records (n), d_poses (n, 12) or None) of one vis_trajectory_rows; the guard bytes behind both outputs checked"""
    collect = prepare_chain(vislam, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, prev, pose, link, carry=None, seq0=0, same_epoch_only=True, where=None):
    got = chain_on_device(vislam, c, prev, pose, link, carry, seq0, same_epoch_only)
    want = tj.trajectory_rows(prev, pose, link, carry, seq0, same_epoch_only)
    assert got[0].tobytes() == want[0].tobytes(), (where, [i for i in range(len(prev)) if got[0][i].tobytes() != want[0][i].tobytes()][:5])
    assert got[1].tobytes() == want[1].tobytes(), (where, np.argwhere(got[1] != want[1])[:5])
    return want


@pytest.mark.parametrize("name", PAIRINGS)
@pytest.mark.parametrize("n", NS)
def test_rows_against_the_restatement(vislam, ctx, n, name):
    for carry in (None, carried_record()):
        prev, pose, link = pairing(name, n, first=sl.KF_CARRIED if carry is not None else sl.KF_FIRST)
        for same in (True, False):
            rec, poses = check(vislam, ctx, prev, pose, link, carry, seq0=40, same_epoch_only=same, where=(n, name, carry is not None, same))
        seq = tj.sequential_rows(prev, pose, link, carry, seq0=40)
        assert_same_but_rounding(rec, seq, path_lengths(seq, carry), 16 * DOUBLING_BOUND)
        assert all(np.isfinite(rec[f]).all() for f in ("R", "t", "sigma")) and np.isfinite(poses).all()
    if n >= 33 and name in ("chain", "badlink"):
        assert int(rec[n - 1]["hops"]) == 9 + n                     # the chain is as long as the launch, and continues the carried one


def test_without_dense_poses_and_with_carried_records_that_count_as_none(vislam, ctx):
    prev, pose, link = pairing("chain", 5, first=sl.KF_CARRIED)
    want, _ = tj.trajectory_rows(prev, pose, link, carried_record(), seq0=3)
    got, none = chain_on_device(vislam, ctx, prev, pose, link, carried_record(), seq0=3, dense=False)
    assert none is None and got.tobytes() == want.tobytes()
    for c in (tj.zero_record(tj.TJ_OVERFLOW), tj.zero_record(tj.TJ_NOT_SAVED)):
        rec, _ = check(vislam, ctx, prev, pose, link, c, seq0=3)
        assert int(rec[0]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_CARRY


def test_a_sigma_product_that_overflows(vislam, ctx):
    prev, pose, up, down = overflowing()
    for link in (up, down):
        rec, poses = check(vislam, ctx, prev, pose, link)
        assert int(rec[-1]["flags"]) == tj.TJ_OVERFLOW and (poses[-1] == 0).all() and int(rec[2]["flags"]) == 0
    hostile = carried_record()                                      # a carried record with a NaN and an infinity: every frame below it overflows
    hostile["t"][1], hostile["sigma"] = float("nan"), float("inf")
    prev[0] = sl.KF_CARRIED
    rec, _ = check(vislam, ctx, prev, pose, pairing("chain", len(prev))[2], hostile)
    assert (rec["flags"] == tj.TJ_OVERFLOW).all()


def test_hostile_links_and_poses(vislam, ctx):
    """NaN, infinite, zero and negative scales on VIS_SL_OK links are unit edges; NaN and infinite pose entries make a root"""
    prev, pose, link = pairing("chain", 12)
    link["scale"][[2, 3, 4, 5]] = [float("nan"), float("inf"), 0.0, -1.0]
    pose[7]["t"][0], pose[9]["R"][3], pose[10]["t"][:] = float("inf"), float("nan"), 0.0
    rec, _ = check(vislam, ctx, prev, pose, link)
    assert all(int(rec[i]["flags"]) == tj.TJ_UNIT_EDGE for i in (2, 3, 4, 5)) and all(int(rec[i]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_POSE for i in (7, 9, 10))
