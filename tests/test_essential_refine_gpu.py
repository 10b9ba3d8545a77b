"""GPU: the two-view refinement (vis_essential_refine_batch / vis_essential_refine / vis_batch_essential_refine) against the restatement
tests/essential_refine_ref.py.

Records are compared BYTE FOR BYTE, every integer and every double: the restatement takes every product and sum in the kernel's order.  Output
buffers are pre-filled with 0xEE; points beyond a row's count are NaN and mask bytes beyond it 0xFF, so an over-read shows as a different
record; max_pts (640) exceeds every row and row_cap (643) exceeds max_pts.  The start of a row is the CPU oracle's RANSAC winner of its scene
(every other row turned by a few milliradians, so that the refinement has work to do), the set its mask; the device reads it from a pose
record whose other fields are NaN / junk.

vis_batch_essential_refine runs on the parallax stream the PnP and KLT tests batch (vis_synth_frame_parallax, 752 x 480, fy = fx), two launches
of 16 frames, gate off, gate on and VIS_POSE_SYM; the rows are rebuilt from the getters."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import essential_refine_ref as er
import homography_ref as hr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC, PREC = 216, 192
CAM = er.Camera()
MAX_PTS, ROW_CAP = 640, 643
LENGTHS = (0, 5, 7, 8, 63, 64, 65, 129, 300)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _params(vislam):
    return pdc.set_mode(vislam.default_params(), "adaptive")      # the camera of the scenes


def _both(vislam, **kw):
    a, b = vislam.default_eref_params(), er.default_params()
    for k, v in kw.items():
        setattr(a, k, v)
        setattr(b, k, v)
    return a, b


def _problem(vislam, orc, cls, m, noise, outliers, seed, turn):
    """(x1, x2, start[12], mask) of a scene: the oracle's winner, optionally turned by `turn` radians about (1, -1, 1) / sqrt 3"""
    x1, x2 = er.make_scene(cls, m, noise, outliers, seed)[:2]
    p = _params(vislam)
    E, mask, _, _ = orc.essential_ransac(p, x1, x2)
    R, t, _ = orc.recover_pose(p, E, x1, x2)
    if turn and np.isfinite(R).all():
        R = pdc._rodrigues(turn * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)) @ R
    return x1, x2, np.concatenate([R.reshape(9), t]), mask


class _Rows:
    def __init__(self, vislam, torch, probs, npts=None, max_pts=MAX_PTS, row_cap=ROW_CAP):
        self.probs, self.n, self.max_pts, self.row_cap = probs, len(probs), max_pts, row_cap
        n = self.n
        self.p1 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.p2 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.mask = np.full((n, row_cap), 0xFF, np.uint8)
        pose = np.zeros(n, vislam.POSE_RESULT_DTYPE)
        pose["E"], pose["n_inliers"], pose["n_points"] = np.nan, -7, 1 << 20          # never read
        self.starts = np.zeros((n, 12))
        for i, (a, b, s, mk) in enumerate(probs):
            k = min(len(a), max_pts)
            self.p1[i, :k], self.p2[i, :k], self.mask[i, :k] = a[:k], b[:k], mk[:k]
            self.starts[i] = s
            pose[i]["R"], pose[i]["t"] = s[:9], s[9:]
        self.npts = np.array([len(a) for a, _, _, _ in probs], np.int32) if npts is None else np.asarray(npts, np.int32)
        self.d = [_dev(torch, v) for v in (pose.view(np.uint8), self.p1, self.p2, self.npts, self.mask)]

    def run(self, vislam, torch, c, ep, with_mask=True):
        n = self.n
        out = _filled(torch, (n + 2) * REC)
        d_pose, d_p1, d_p2, d_n, d_mask = self.d
        c.essential_refine_batch(n, d_pose.data_ptr(), d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), self.max_pts, self.row_cap,
                                 d_mask.data_ptr() if with_mask else 0, out.data_ptr(), ep)
        c.batch_sync()
        raw = out.cpu().numpy()
        assert (raw[n * REC:] == FILL).all()
        assert d_mask.cpu().numpy().tobytes() == self.mask.tobytes()       # the input mask is never modified
        return raw[:n * REC].view(vislam.EREF_RESULT_DTYPE).copy()

    def want(self, eq, with_mask=True):
        return er.refine_rows(CAM, eq, self.starts, self.p1, self.p2, self.npts, self.mask if with_mask else None)


def _same(got, want, where):
    assert len(got) == len(want)
    for i in range(len(got)):
        assert got[i].tobytes() == want[i].tobytes(), (where, i, got[i], want[i])


@pytest.fixture(scope="module")
def probs(vislam, orc):
    """63 problems: the row lengths of the list seven times over with classes, noise, outliers and the turn of the start varied, one row of 600"""
    out = []
    for i in range(63):
        m = 600 if i == 40 else LENGTHS[i % len(LENGTHS)]
        cls = "general" if i == 40 else er.CLASSES[(i // len(LENGTHS) + i) % len(er.CLASSES)]
        out.append(_problem(vislam, orc, cls, m, (0.0, 0.3, 1.0)[i % 3], (0.0, 0.25)[(i // 3) % 2], i, 0.004 if i % 2 else 0.0))
    return out


def test_records_against_the_restatement(vislam, probs):
    import torch
    c = vislam.Context(0, _params(vislam))
    ep, eq = _both(vislam)
    rows = _Rows(vislam, torch, probs)
    assert rows.n == 63 and set(LENGTHS) | {600} == {int(v) for v in rows.npts}
    recs = rows.run(vislam, torch, c, ep)
    want = rows.want(eq)
    _same(recs, want, "mask")
    flags = [int(r["flags"]) for r in recs]
    assert flags.count(vislam.ER_REFINED) >= 20 and vislam.ER_FEW in flags and vislam.ER_NO_POSE in flags, flags
    assert all(float(r["cost1"]) <= float(r["cost0"]) for r in recs if int(r["flags"]) & (vislam.ER_REFINED | vislam.ER_REJECTED))
    # without a mask every point of the row is in the set
    recs_n = rows.run(vislam, torch, c, ep, with_mask=False)
    _same(recs_n, rows.want(eq, with_mask=False), "no mask")
    assert any(int(a["n_used"]) != int(b["n_used"]) for a, b in zip(recs, recs_n))
    # two runs are identical
    assert rows.run(vislam, torch, c, ep).tobytes() == recs.tobytes()
    # counts above max_pts are clamped, negative ones are empty rows
    big = probs[40]
    edge = _Rows(vislam, torch, [big, big, big], npts=[1000, 0, -5], max_pts=300, row_cap=300)
    got = edge.run(vislam, torch, c, ep)
    _same(got, edge.want(eq), "edge")
    assert [int(r["n_points"]) for r in got] == [300, 0, 0] and int(got[1]["flags"]) == vislam.ER_FEW
    c.close()


def test_single_call_equals_its_row(vislam, probs):
    c = vislam.Context(0, _params(vislam))
    ep, eq = _both(vislam)
    for i in list(range(0, 63, 4)) + [40]:
        x1, x2, s, mk = probs[i]
        for mask in (mk, None):
            rec = c.essential_refine(s[:9], s[9:], x1, x2, mask, ep)
            assert rec.tobytes() == er.refine(CAM, eq, s[:9], s[9:], x1, x2, mask).tobytes(), (i, mask is None)
    c.close()


def test_refine_iters_and_flags(vislam, orc, probs):
    """refine_iters 0 | 1 | 2 | 5 | 64 on four rows; REJECTED: a first pivot that fails (one correspondence repeated: J^T J has rank one), and a start
    that already is the minimum as far as the cost in double tells (either flag: printed); a row whose every term is dropped (NaN pixels in the set:
    J^T J = 0, the first pivot fails, REJECTED for certain); FEW; NO_POSE of the all-zero, NaN and zero-t kinds"""
    import torch
    c = vislam.Context(0, _params(vislam))
    four = [_problem(vislam, orc, "general", 300, 0.3, 0.25, 1, 0.004), _problem(vislam, orc, "forward", 63, 0.3, 0.0, 2, 0.0),
            _problem(vislam, orc, "sideways", 129, 1.0, 0.25, 3, 0.004), probs[40]]
    rows = _Rows(vislam, torch, four)
    seen = {}
    for iters in (0, 1, 2, 5, 64):
        ep, eq = _both(vislam, refine_iters=iters)
        recs = rows.run(vislam, torch, c, ep)
        _same(recs, rows.want(eq), iters)
        for r in recs:
            assert int(r["steps_run"]) <= iters and int(r["best_step"]) <= int(r["steps_run"])
            assert (int(r["flags"]) == 0) == (iters == 0)
        seen[iters] = recs
    assert all(float(a["cost1"]) <= float(b["cost1"]) for a, b in zip(seen[64], seen[5]))          # more iterates to choose from
    # the special rows
    x1, x2, s, mk = four[0]
    ep, eq = _both(vislam)
    ep20, eq20 = _both(vislam, refine_iters=20)
    conv = er.refine(CAM, eq20, s[:9], s[9:], x1, x2, mk)
    at_min = (x1, x2, np.concatenate([conv["R"], conv["t"]]), mk)
    one = (np.repeat(x1[:1], 8, 0), np.repeat(x2[:1] + np.float32(0.5), 8, 0), s, np.ones(8, np.uint8))
    nan_pts = (np.full((8, 2), np.nan, np.float32), np.full((8, 2), np.nan, np.float32), s, np.ones(8, np.uint8))     # every term is dropped: J^T J = 0
    few = (x1, x2, s, (np.arange(300) < 7).astype(np.uint8))
    zero_R = (x1, x2, np.concatenate([np.zeros(9), s[9:]]), mk)
    nan_R = (x1, x2, np.where(np.arange(12) == 4, np.nan, s), mk)
    inf_t = (x1, x2, np.where(np.arange(12) == 10, np.inf, s), mk)
    zero_t = (x1, x2, np.concatenate([s[:9], np.zeros(3)]), mk)
    long_t = (x1, x2, np.concatenate([s[:9], 5.0 * s[9:]]), mk)
    special = _Rows(vislam, torch, [at_min, one, few, zero_R, nan_R, inf_t, zero_t, long_t, nan_pts])
    recs = special.run(vislam, torch, c, ep)
    _same(recs, special.want(eq), "special")
    fl = [int(r["flags"]) for r in recs]
    R_, J_, F_, N_ = vislam.ER_REFINED, vislam.ER_REJECTED, vislam.ER_FEW, vislam.ER_NO_POSE
    assert fl[2:] == [F_, N_, N_, N_, N_, R_, J_] and fl[0] in (R_, J_) and fl[1] in (R_, J_), fl
    # the failed first pivot: nothing was applied, the start is reported
    assert int(recs[8]["steps_run"]) == 0 and int(recs[8]["best_step"]) == 0 and float(recs[8]["cost1"]) == float(recs[8]["cost0"]) == 0.0
    assert int(recs[8]["n_used"]) == 8 and int(recs[8]["n_inliers0"]) == 0 and recs[8]["R"].tobytes() == s[:9].tobytes()
    assert recs[2]["R"].tobytes() == s[:9].tobytes() and int(recs[2]["n_used"]) == 7 and int(recs[2]["n_points"]) == 300
    for k in (3, 4, 5, 6):
        assert recs[k].tobytes() == er.zero_record().tobytes()
    assert abs(np.linalg.norm(recs[7]["t"]) - 1.0) < 1e-15 and np.abs(recs[7]["t"] - seen[5][0]["t"]).max() < 1e-9   # the start's t is normalised first
    # at the minimum the cost cannot fall by more than its rounding
    assert float(recs[0]["cost0"]) - float(recs[0]["cost1"]) <= 64 * 2.0 ** -52 * float(recs[0]["cost0"])
    print(f"\nstart at the minimum: flags {fl[0]}, best_step {int(recs[0]['best_step'])}, cost {float(recs[0]['cost0'])!r} -> {float(recs[0]['cost1'])!r}")
    c.close()


# ---------------------------------------------------------------------------------------------- the plan's frames
W, H, B = 752, 480, 16


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(2 * B)])
    g = f.copy()
    g[5] = g[B + 5] = 128                                          # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


def _stream_params(vislam, gate=False, sym=False):
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    if sym:
        p.pose_input, p.keypoint_capacity = 1, 2048
    return p


@pytest.mark.parametrize("gate,sym", [(False, False), (True, False), (False, True)])
def test_plan_pairs_over_two_launches(vislam, orc, stream, gate, sym):
    import torch
    p = _stream_params(vislam, gate, sym)
    cam = er.Camera(p.fx, p.cx, p.cy)
    ep, eq = _both(vislam, min_inliers=6)
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    dev = _dev(torch, stream[gate])
    carried = None
    seen = dict(pairs=0, refined=0, no_pose=0)
    for launch in range(2):
        out = _filled(torch, (B + 1) * REC)
        c.batch_run(dev.data_ptr() + launch * B * W * H, B, vislam.STAGE_ALL)
        if launch == 0:                                            # the refusals that need a plan, in the header's order
            bad = vislam.default_eref_params()
            bad.min_inliers = 5
            call = lambda ep_=ep, n=B, o=out.data_ptr(): vislam.lib.vis_batch_essential_refine(c._h, C.byref(ep_), n, C.c_void_p(o))
            assert call(ep_=bad, n=B - 1) == -1 and call(o=out.data_ptr() + 4) == -1 and call(n=B - 1) == -5
            assert (out.cpu().numpy() == FILL).all()
        c.batch_essential_refine(B, out.data_ptr(), ep)
        c.batch_sync()
        assert c.batch_status() == 0
        prev = c.batch_get_keyframes()
        poses, _, ngood = c.batch_results(B)
        kps = [c.batch_keypoints(i)[0] for i in range(B)]
        raw = out.cpu().numpy()
        assert (raw[B * REC:] == FILL).all()
        recs = raw[:B * REC].view(vislam.EREF_RESULT_DTYPE)
        for i in range(B):
            kq = kps[prev[i]] if prev[i] >= 0 else carried if prev[i] == vislam.KF_CARRIED else None
            if kq is None:
                assert recs[i].tobytes() == er.zero_record().tobytes(), (launch, i)
                seen["no_pose"] += 1
                continue
            mt = orc.good_matches(p, kq, kps[i], *c.batch_knn(i))[1] if sym else c.batch_matches(i)[0]
            assert len(mt) == int(poses[i]["n_points"]), (launch, i)
            x1 = np.stack([kq["x"][mt["queryIdx"]], kq["y"][mt["queryIdx"]]], 1).astype(np.float32)
            x2 = np.stack([kps[i]["x"][mt["trainIdx"]], kps[i]["y"][mt["trainIdx"]]], 1).astype(np.float32)
            mask = c.batch_inlier_mask(i)
            assert len(mask) == len(mt) and int(np.count_nonzero(mask)) == int(poses[i]["n_inliers"])
            want = er.refine(cam, eq, poses[i]["R"], poses[i]["t"], x1, x2, mask)
            assert recs[i].tobytes() == want.tobytes(), (launch, i, recs[i], want)
            seen["pairs"] += 1
            seen["refined"] += int(int(want["flags"]) == vislam.ER_REFINED)
            seen["no_pose"] += int(int(want["flags"]) == vislam.ER_NO_POSE)
        carried = kps[-1]
    # a run without the pose stage has nothing to refine
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert vislam.lib.vis_batch_essential_refine(c._h, C.byref(ep), B, C.c_void_p(out.data_ptr())) == -5
    c.batch_sync()
    c.close()
    print(f"\ngate {gate}, symmetric matches {sym}: {seen}")
    assert seen["pairs"] >= (28 if gate else 31) and seen["refined"] >= 16 and seen["no_pose"] >= 1, seen


def _pipelined(vislam, torch, dev, p, sync_each, order, steps=3, n=5):
    """three steps of five frames with the follow-ups queued in `order` (letters: R refinement, H homography, T triangulation)"""
    ep, hp = vislam.default_eref_params(), vislam.default_homography_params()
    ep.min_inliers = 6
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    c.batch_reset()
    d_draws = _dev(torch, hr.make_draws(7))
    outs = [dict(R=_filled(torch, n * REC), H=_filled(torch, n * 112), Hm=_filled(torch, n * 49), Tp=_filled(torch, n * 49 * 32), Tf=_filled(torch, n * 49),
                 Ts=_filled(torch, n * 16)) for _ in range(steps)]
    poses = [np.zeros(n, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        o = outs[k]
        c.batch_run(dev.data_ptr() + k * n * W * H, n, vislam.STAGE_ALL)
        for what in order:
            if sync_each:
                c.batch_sync()
            if what == "R":
                c.batch_essential_refine(n, o["R"].data_ptr(), ep)
            elif what == "H":
                c.batch_homography(n, d_draws.data_ptr(), 49, o["Hm"].data_ptr(), o["H"].data_ptr(), hp)
            else:
                c.batch_triangulate(n, 49, o["Tp"].data_ptr(), o["Tf"].data_ptr(), o["Ts"].data_ptr())
        c.batch_results_async(n, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    res = {key: b"".join(o[key].cpu().numpy().tobytes() for o in outs) for key in outs[0]}
    res["pose"] = b"".join(q.tobytes() for q in poses)
    c.close()
    return res


def test_pipelined_equals_synchronised_and_leaves_the_other_follow_ups_alone(vislam, stream):
    import torch
    p = _stream_params(vislam)
    dev = _dev(torch, stream[False][:15])
    base = _pipelined(vislam, torch, dev, p, False, "HT")          # without the refinement
    first = _pipelined(vislam, torch, dev, p, False, "RHT")
    last = _pipelined(vislam, torch, dev, p, False, "HTR")
    synced = _pipelined(vislam, torch, dev, p, True, "RHT")
    for key in ("H", "Hm", "Tp", "Tf", "Ts", "pose"):
        assert base[key] == first[key] == last[key] == synced[key], key
    assert first["R"] == last["R"] == synced["R"] and base["R"] == bytes([FILL]) * len(base["R"])
    recs = np.frombuffer(first["R"], vislam.EREF_RESULT_DTYPE)
    assert (recs["flags"] == vislam.ER_REFINED).sum() >= 8 and (recs["flags"] == vislam.ER_NO_POSE).sum() >= 1      # not a comparison of empty records


# ---------------------------------------------------------------------------------------------- the chain
def test_klt_rows_to_pose_to_refinement(vislam, canvas):
    """vis_batch_klt's compacted rows -> vis_essential_batch -> vis_essential_refine_batch, the last two queued back to back on the context's
    stream with nothing but device memory between them (vis_batch_klt itself runs on the pose stream: one vis_batch_sync orders the two), against
    the host-pointer calls on the downloaded rows"""
    import torch
    PW, PH, PB = 320, 240, 8
    p = vislam.default_params()
    p.w_size, p.h_size, p.fy, p.nfeatures = PW, PH, p.fx, 200
    p.cx, p.cy = PW / 2.0, PH / 2.0
    frames = np.stack([vislam.synth_frame(canvas, t, PW, PH, parallax=True) for t in range(PB)])
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, PB)
    cap = c.keypoint_capacity(PW, PH)
    dev = _dev(torch, frames)
    c.batch_run(dev.data_ptr(), PB, vislam.STAGE_DETECT | vislam.STAGE_GRADIENT)
    recs, pair = _filled(torch, PB * cap * 32), _filled(torch, PB * 32)
    p1, p2, nt = _filled(torch, PB * cap * 8), _filled(torch, PB * cap * 8), _filled(torch, PB * 4)
    c.batch_klt(dev.data_ptr(), PB, cap, recs.data_ptr(), pair.data_ptr(), 0, p1.data_ptr(), p2.data_ptr(), nt.data_ptr())
    c.batch_sync()
    pose, mask, out = _filled(torch, PB * PREC), _filled(torch, PB * cap), _filled(torch, PB * REC)
    ep, eq = _both(vislam)
    c.essential_batch(PB, p1.data_ptr(), p2.data_ptr(), nt.data_ptr(), cap, cap, mask.data_ptr(), pose.data_ptr())
    c.essential_refine_batch(PB, pose.data_ptr(), p1.data_ptr(), p2.data_ptr(), nt.data_ptr(), cap, cap, mask.data_ptr(), out.data_ptr(), ep)
    c.batch_sync()
    h1, h2 = p1.cpu().numpy().reshape(PB, cap * 8), p2.cpu().numpy().reshape(PB, cap * 8)
    cnt = nt.cpu().numpy().view(np.int32)
    poses, masks = pose.cpu().numpy().view(vislam.POSE_RESULT_DTYPE), mask.cpu().numpy().reshape(PB, cap)
    got = out.cpu().numpy().view(vislam.EREF_RESULT_DTYPE)
    cam = er.Camera(p.fx, p.cx, p.cy)
    refined = 0
    for i in range(PB):
        k = int(cnt[i])
        x1, x2 = h1[i, :k * 8].view(np.float32).reshape(k, 2), h2[i, :k * 8].view(np.float32).reshape(k, 2)
        E, m1, ninl, iters = c.essential_ransac(x1, x2)
        assert poses[i]["E"].tobytes() == E.reshape(9).tobytes() and masks[i, :k].tobytes() == m1.tobytes() and int(poses[i]["n_inliers"]) == ninl, i
        if E.any():
            R, t, ng = c.recover_pose(E, x1, x2)
            assert poses[i]["R"].tobytes() == R.reshape(9).tobytes() and poses[i]["t"].tobytes() == t.tobytes(), i
        single = c.essential_refine(poses[i]["R"], poses[i]["t"], x1, x2, masks[i, :k], ep)
        assert got[i].tobytes() == single.tobytes() == er.refine(cam, eq, poses[i]["R"], poses[i]["t"], x1, x2, masks[i, :k]).tobytes(), (i, got[i], single)
        refined += int(int(got[i]["flags"]) == vislam.ER_REFINED)
    assert int(got[0]["flags"]) == vislam.ER_NO_POSE and int(cnt[0]) == 0 and refined >= 5      # frame 0 has no pair
    c.close()


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_refined_poses(vislam, stream, tmp_path):
    """tools/run_directory.py --refined: one line per frame, holding what vis_batch_essential_refine gives for the same frames in the same batches"""
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    frames = stream[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "refined.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--refined", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    dev = _dev(torch, frames)
    recs = []
    for first in range(0, n, nb):
        out = _filled(torch, nb * REC)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_essential_refine(nb, out.data_ptr())
        c.batch_sync()
        recs += list(out.cpu().numpy().view(vislam.EREF_RESULT_DTYPE))
    c.close()
    assert len(rows) == n == len(recs)
    assert j["refined"]["refined"] == sum(int(r["flags"]) == vislam.ER_REFINED for r in recs) >= 6
    for k, (row, r) in enumerate(zip(rows, recs)):
        assert len(row) == 32 and int(row[0]) == k and int(row[1]) == 1403636579763555584 + 50000000 * k
        assert [int(v) for v in row[2:9]] == [int(r[f]) for f in ("flags", "n_used", "n_points", "n_inliers0", "n_inliers_refined", "best_step", "steps_run")]
        want = [r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(r["E"])
        assert np.array([float(v) for v in row[9:]]).tobytes() == np.array(want, np.float64).tobytes(), k
