"""GPU: the host-pointer entry points size the context's two grow-only blocks (device scratch, pinned staging) from one buffer list
per call (csrc/vis_internal.h vis_carve).  ONE context runs the pair calls at m = 5, then 700, then 5 again, and an image call at
16 x 16 and 64 x 48: on the way up both blocks are replaced between calls, on the way down a call carves a block larger than it
needs.  Every result must be byte-identical to the same call on a context created fresh for it -- a list that measures differently from
how it binds, or a stage built on a block that was replaced afterwards, reads or writes the wrong bytes.
The device-rows calls keep a grow-only workspace each (vis_grow_block / vis_carve_block): they go through the same scheme, small, large, small,
QUEUED on one context back to back, every upload done beforehand and one host synchronise at the end -- the large step replaces a block that the
small step's kernels were given."""
import numpy as np
import pytest

import f2f_ref as fr
import ftrack_ref
import homography_ref as hr
import imu_cases as ic
import imu_ref as ir
import scale_link_ref as sl
from test_ftrack_gpu import prepare_link, random_carry
from test_ftrack_ref import random_stream
from test_imu_gpu import prepare_rows
from test_scale_link_gpu import prepare_links
from test_scale_link_ref import shared_case
from test_trajectory_gpu import prepare_chain
from test_trajectory_ref import carried_record, pairing

pytestmark = pytest.mark.gpu


def _blob(v):
    """any result (arrays, numpy records, ctypes structures, ints, nested tuples) as bytes"""
    if isinstance(v, (tuple, list)):
        return b"|".join(_blob(x) for x in v)
    if isinstance(v, (np.ndarray, np.generic)):
        return np.asarray(v).tobytes()
    if isinstance(v, (int, float)):
        return repr(v).encode()
    return bytes(v)


def _pair_calls(vislam, m):
    """[(name, call(context) -> result)] in the order of the shared context; inputs depend on m alone"""
    x1, x2, R, t = fr.two_view(m, 900 + m, 0.2, 0.5)
    ka, kb = fr.keypoints(vislam.KEYPOINT_DTYPE, x1), fr.keypoints(vislam.KEYPOINT_DTYPE, x2)
    rot, t32 = R.T.astype(np.float32), t.astype(np.float32)
    hdraws = hr.make_draws(m)
    idx = np.random.default_rng(m).integers(0, m, (300, 2)).astype(np.int32)

    def hpose(c):
        rec, mask = c.find_homography(x1, x2, hdraws)
        return c.homography_pose(rec, x1, x2, mask)

    def pose(c):
        E, mask, ninl, iters = c.essential_ransac(x1, x2)
        return (E, mask, ninl, iters) + tuple(c.recover_pose(E, x1, x2))

    return [("filter_keypoints", lambda c: c.filter_keypoints(ka, kb, rot, t32, 500.0)),
            ("find_homography", lambda c: c.find_homography(x1, x2, hdraws)),
            ("homography_pose", hpose),
            ("triangulate", lambda c: c.triangulate(R, t, x1, x2)),
            ("essential_ransac + recover_pose", pose),
            ("f2f_ransac", lambda c: c.f2f_ransac(ka, kb, rot, idx, 0.37))]


def _image_calls(vislam):
    rng = np.random.default_rng(5)
    return [(f"camera_update {w} x {h}", (lambda img: lambda c: c.camera_update(img))(rng.integers(0, 256, (h, w)).astype(np.uint8)))
            for w, h in ((16, 16), (64, 48))]


def test_one_context_through_growing_and_shrinking_calls(vislam):
    fresh = {}

    def want(key, call):
        if key not in fresh:                                       # (m = 5 comes twice: one reference)
            c = vislam.Context(0)
            fresh[key] = _blob(call(c))
            c.close()
        return fresh[key]

    shared = vislam.Context(0)
    for step, m in enumerate((5, 700, 5)):
        for name, call in _pair_calls(vislam, m) + (_image_calls(vislam) if step == 0 else []):
            got = _blob(call(shared))
            assert len(got) > 0 and got == want((name, m), call), (step, m, name)
    shared.close()
    assert len(fresh) == 14


def _ftrack_rows(n, row_cap):
    prev, nkp, links, nlinks, mask = random_stream(1000 + n + row_cap, n, row_cap, row_cap + 3, hostile=False, first_prev=ftrack_ref.KF_CARRIED)
    return lambda v: prepare_link(v, prev, nkp, links, nlinks, row_cap, mask, random_carry(n, row_cap), seq0=70)


def _scale_link_rows(m):
    (*case, row_cap, _), _ = shared_case(m - 2, extra=2)              # m list entries per pair
    assert case[1].shape[1] == m
    return lambda v: prepare_links(v, sl.Params(), *case, row_cap)


def _trajectory_rows(n):
    prev, pose, link = pairing("chain", n, first=sl.KF_CARRIED)
    return lambda v: prepare_chain(v, prev, pose, link, carried_record(), seq0=40)


def _imu_rows(n):
    s, tf, tb = ic.stream(n, 2)
    return lambda v: prepare_rows(v, ic.params(), s, tf, ic.pairing("long", n, ir.KF_CARRIED), ic.carried(tb, True))


# name: (builder, small, large); a builder answers prepare(vislam) -> call(context) -> collect().  The large step needs a larger block than the small
# one -- for the scale links and the trajectory it is the only one that needs a block at all (more than SL_LDS_CAP = 1024 entries per pair, more than
# TJ_LDS_N = 256 frames)
ROWS_CALLS = {"ftrack_link_rows": (_ftrack_rows, (2, 8), (9, 300)),
              "scale_link_rows": (_scale_link_rows, (8,), (sl.SL_LDS_CAP + 1,)),
              "trajectory_rows": (_trajectory_rows, (3,), (257,)),
              "imu_preintegrate_rows": (_imu_rows, (1,), (257,))}


def test_rows_calls_queued_through_growing_blocks(vislam):
    """every call small, every call large, every call small again on ONE context.  The uploads and the output fills of all twelve calls come FIRST
    (they synchronise the device); then the twelve library calls are issued back to back and the host synchronises once, at the end.  So a call that
    grows its block does so while whatever the calls before it queued may still be running: it must neither free a block under those kernels nor
    move another call's block.  (The kernels are short: how many are still in flight when a block grows is up to the device.)"""
    prepare = {name: (build(*small), build(*large)) for name, (build, small, large) in ROWS_CALLS.items()}
    want = {}
    for name, sizes in prepare.items():
        for size, prep in enumerate(sizes):
            c = vislam.Context(0)
            collect = prep(vislam)(c)
            c.batch_sync()
            want[name, size] = _blob(collect())
            c.close()
    shared = vislam.Context(0)
    ready = [(name, size, prepare[name][size](vislam)) for size in (0, 1, 0) for name in prepare]
    queued = [(name, size, call(shared)) for name, size, call in ready]  # nothing here but the library's calls
    shared.batch_sync()
    got = [(name, size, _blob(collect())) for name, size, collect in queued]
    shared.close()
    assert len(got) == 12
    for step, (name, size, blob) in enumerate(got):
        assert len(blob) > 0 and blob == want[name, size], (step // 4, name, "large" if size else "small")
    assert all(want[name, 0] != want[name, 1] for name in prepare)
