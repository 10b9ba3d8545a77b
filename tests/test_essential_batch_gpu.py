"""GPU: vis_essential_batch -- the pose stage on rows that already sit in device memory -- against the single calls.

The yardstick is vis_essential_ransac followed by vis_recover_pose on each row alone (tests/test_pose_gpu.py pins those to the CPU oracle):
E, the mask, n_inliers and iters_run of the first, R, t and n_pose_good of the second, byte for byte.  One documented difference: a row
without a model (E all zero: fewer than five points) has R = 0 and t = 0 in the batch, as the plan's pose records do, where
vis_recover_pose on a zero E answers NaN.  Rows of 0, 4, 5, 6, 64, 257 and 300 correspondences with different lengths in one launch: 5 is the
single-solve shortcut, 6 the first row of the sample table, 64 its last (VIS_POSE_TABLE_M; longer rows replay the stream on the device), 257
exceeds the 256-correspondence form of the scoring.  n = 1 first, then n = 17 on the same context, which grows the workspace.  Points beyond a
row's count are NaN and the output buffers are pre-filled with 0xEE: an over-read or a stray write shows."""
import numpy as np
import pytest

import essential_refine_ref as er
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC = 192
LENGTHS = (0, 4, 5, 6, 64, 257, 300)
MAX_PTS, ROW_CAP = 320, 323


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _scene(i, m):
    cls = ("general", "forward", "sideways")[i % 3]
    return er.make_scene(cls, m, 0.3, 0.25 if m >= 64 else 0.0, seed=100 + i)[:2]


def _rows(n):
    lens = [LENGTHS[(i + 3) % len(LENGTHS)] for i in range(n)] if n > 1 else [64]
    return [_scene(i, m) for i, m in enumerate(lens)]


def _single(c, x1, x2):
    """the record fields and the mask the single calls give for one row"""
    E, mask, ninl, iters = c.essential_ransac(x1, x2)
    R, t, ngood = c.recover_pose(E, x1, x2)
    return E.reshape(9), mask, ninl, iters, R.reshape(9), t, ngood


def _run(vislam, torch, c, rows, with_mask=True, npts=None):
    n = len(rows)
    p1 = np.full((n, MAX_PTS, 2), np.nan, np.float32)
    p2 = np.full((n, MAX_PTS, 2), np.nan, np.float32)
    for i, (a, b) in enumerate(rows):
        p1[i, :len(a)], p2[i, :len(b)] = a, b
    npts = np.array([len(a) for a, _ in rows], np.int32) if npts is None else np.asarray(npts, np.int32)
    d_p1, d_p2, d_n = _dev(torch, p1), _dev(torch, p2), _dev(torch, npts)
    out, mask = _filled(torch, (n + 1) * REC), _filled(torch, n * ROW_CAP + 64)
    c.essential_batch(n, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), MAX_PTS, ROW_CAP, mask.data_ptr() if with_mask else 0, out.data_ptr())
    c.batch_sync()
    raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
    assert (raw[n * REC:] == FILL).all() and (mraw[n * ROW_CAP:] == FILL).all()
    if not with_mask:
        assert (mraw == FILL).all()
    return raw[:n * REC].view(vislam.POSE_RESULT_DTYPE).copy(), mraw[:n * ROW_CAP].reshape(n, ROW_CAP)


def _compare(c, recs, masks, rows, where):
    models = 0
    for i, (x1, x2) in enumerate(rows):
        m = len(x1)
        E, mask, ninl, iters, R, t, ngood = _single(c, x1, x2)
        r = recs[i]
        assert r["E"].tobytes() == E.tobytes(), (where, i, m)
        assert (int(r["n_inliers"]), int(r["iters_run"]), int(r["n_points"])) == (ninl, iters, m), (where, i, m, r)
        assert masks[i, :m].tobytes() == mask.tobytes() and (masks[i, m:] == FILL).all(), (where, i, m)
        if E.any():
            models += 1
            assert r["R"].tobytes() == R.tobytes() and r["t"].tobytes() == t.tobytes() and int(r["n_pose_good"]) == ngood, (where, i, m, r)
            assert ninl >= 5 and abs(np.linalg.norm(t) - 1.0) < 1e-9
        else:                                                      # no model: the batch path's zero pose, where the single call answers NaN
            assert m <= 5 and not r["R"].any() and not r["t"].any() and int(r["n_pose_good"]) == 0 and ninl == 0, (where, i, m, r)
            assert np.isnan(R).all()
    return models


def test_rows_equal_the_single_calls(vislam):
    import torch
    c = vislam.Context(0, pdc.set_mode(vislam.default_params(), "adaptive"))
    one = _rows(1)
    recs1, masks1 = _run(vislam, torch, c, one)                    # n = 1: the smallest workspace
    assert _compare(c, recs1, masks1, one, "n = 1") == 1
    rows = _rows(17)                                               # n = 17 on the same context: the workspace grows
    assert sorted({len(a) for a, _ in rows}) == list(LENGTHS)
    recs, masks = _run(vislam, torch, c, rows)
    assert _compare(c, recs, masks, rows, "n = 17") >= sum(len(a) > 5 for a, _ in rows)       # (five points may have no solution)
    assert any(int(r["iters_run"]) > 16 for r in recs)             # some row went beyond the first chunk of hypotheses (the work-list kernels)
    # the smaller launch again, on the grown workspace; without a mask nothing but the records is written; a second run is byte-identical
    again1, _ = _run(vislam, torch, c, one)
    assert again1.tobytes() == recs1.tobytes()
    recs2, _ = _run(vislam, torch, c, rows, with_mask=False)
    recs3, masks3 = _run(vislam, torch, c, rows)
    assert recs2.tobytes() == recs.tobytes() and recs3.tobytes() == recs.tobytes() and masks3.tobytes() == masks.tobytes()
    # a count above max_pts is clamped
    big = er.make_scene("general", MAX_PTS, 0.3, 0.25, seed=7)[:2]
    recs_c, masks_c = _run(vislam, torch, c, [big], npts=[5000])
    assert _compare(c, recs_c, masks_c, [big], "clamped") == 1 and int(recs_c[0]["n_points"]) == MAX_PTS
    c.close()


def test_rows_without_room_for_a_point(vislam):
    """max_pts == 0 (the point pointers may be NULL): every record is the record of zero correspondences -- all zeros, what a row of 0 points gives
    at any max_pts -- the mask is not touched, and the refinement answers VIS_ER_NO_POSE for such records"""
    import torch
    c = vislam.Context(0, pdc.set_mode(vislam.default_params(), "adaptive"))
    n = 5
    d_n = _dev(torch, np.array([0, 3, -1, 700, 0], np.int32))
    out, mask, ref = _filled(torch, (n + 1) * REC), _filled(torch, 64), _filled(torch, (n + 1) * 216)
    c.essential_batch(n, 0, 0, d_n.data_ptr(), 0, 0, mask.data_ptr(), out.data_ptr())
    c.essential_refine_batch(n, out.data_ptr(), 0, 0, d_n.data_ptr(), 0, 0, mask.data_ptr(), ref.data_ptr())
    c.batch_sync()
    raw, rraw = out.cpu().numpy(), ref.cpu().numpy()
    assert not raw[:n * REC].any() and (raw[n * REC:] == FILL).all() and (mask.cpu().numpy() == FILL).all()
    empty, _ = _run(vislam, torch, c, [_scene(0, 0)])
    assert empty[0].tobytes() == raw[:REC].tobytes()               # the same record as an empty row of a launch that has room
    assert rraw[:n * 216].tobytes() == er.zero_record().tobytes() * n and (rraw[n * 216:] == FILL).all()
    c.close()


def test_fixed_iteration_mode_and_refusals(vislam):
    """the adaptive stop off (every hypothesis through the work-list kernels), and the refusals that need a context"""
    import ctypes as C
    import torch
    c = vislam.Context(0, pdc.set_mode(vislam.default_params(), "fixed100"))
    rows = [_scene(i, m) for i, m in enumerate((6, 40, 257))]
    recs, masks = _run(vislam, torch, c, rows)
    assert _compare(c, recs, masks, rows, "fixed100") == 3 and max(int(r["iters_run"]) for r in recs) == 100
    some = C.c_void_p(recs.ctypes.data & ~7)
    L = vislam.lib
    assert L.vis_essential_batch(c._h, 1, some, some, some, 8193, 8193, None, some) == -4          # VIS_E_CAPACITY: beyond a RANSAC problem
    assert L.vis_essential_batch(c._h, 1, some, some, some, 49, 48, some, some) == -4              # a mask with a short row (refused: nothing is read)
    ep = vislam.default_eref_params()
    assert L.vis_essential_refine_batch(c._h, C.byref(ep), 1, some, some, some, some, 49, 48, some, some) == -4
    c.close()
