"""GPU: feature tracks (vis_ftrack_link_rows / vis_batch_ftrack) and their N-view triangulation (vis_ftrack_triangulate_rows /
vis_batch_ftrack_triangulate) against the restatement tests/ftrack_ref.py, BYTE FOR BYTE: observations, frame summaries, points, flag bytes
and summaries.  Output buffers are pre-filled with 0xEE (the FILL convention of tests/test_pnp_gpu.py) and everything behind the written extent
must keep it.

Rows form: n in {1, 2, 3, 8, 9, 33, 65} (the doubling depth at 2^k and 2^k + 1) with row capacities 8, 64, 65 and 300 (wave edges), a track
as long as the launch, a track entering through d_carry_in, VIS_KF_NOT_SAVED frames in the middle and at both ends, VIS_KF_FIRST in the
middle.  Plan form: the parallax stream of tests/test_pnp_gpu.py (752 x 480, two launches of 16, frames 5 and 21 flat), gate off, gate on and
VIS_POSE_SYM, every list source, the same 32 frames as one launch, a launch that was not linked, the refusals that need a plan."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ftrack_ref as fr
from test_ftrack_ref import CAM, planted, random_stream

pytestmark = pytest.mark.gpu
FILL = 0xEE


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def prepare_link(vislam, prev, nkp, links, nlinks, row_cap, mask=None, carry=None, seq0=0):
    """the inputs of one vis_ftrack_link_rows uploaded and its outputs filled (both synchronise the device); the answer is call(c), which queues the
    call on context c and synchronises nothing.  call(c) answers collect() -> (obs (n, row_cap), frames (n)), for after a synchronise: it checks the
    guard entries behind both outputs"""
    import torch
    n, link_cap = len(prev), links.shape[1]
    keep = [_dev(torch, np.asarray(a)) for a in (np.asarray(prev, np.int32), np.asarray(nkp, np.int32), links.reshape(-1).view(np.uint8) if links.size else np.zeros(16, np.uint8),
                                                 np.asarray(nlinks, np.int32))]
    d_mask = _dev(torch, mask) if mask is not None else None
    d_carry = _dev(torch, carry.view(np.uint8)) if carry is not None else None
    obs, frames = _filled(torch, (n * row_cap + 3) * 16), _filled(torch, (n + 2) * 32)

    def collect():
        ro, rf = obs.cpu().numpy(), frames.cpu().numpy()
        assert (ro[n * row_cap * 16:] == FILL).all() and (rf[n * 32:] == FILL).all()
        return ro[:n * row_cap * 16].view(vislam.FTRACK_OBS_DTYPE).reshape(n, row_cap), rf[:n * 32].view(vislam.FTRACK_FRAME_DTYPE)

    def call(c):
        c.ftrack_link_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), link_cap, row_cap, obs.data_ptr(), frames.data_ptr(),
                           seq0, d_mask.data_ptr() if mask is not None else 0, mask.shape[1] if mask is not None else 0, d_carry.data_ptr() if carry is not None else 0)
        return collect
    return call


def link_on_device(vislam, c, *rows, **kw):
    """(obs (n, row_cap), frames (n)) of one vis_ftrack_link_rows; the guard entries behind both outputs checked"""
    collect = prepare_link(vislam, *rows, **kw)(c)
    c.batch_sync()
    return collect()


def check_link(vislam, c, prev, nkp, links, nlinks, row_cap, mask=None, carry=None, seq0=0, where=None):
    got = link_on_device(vislam, c, prev, nkp, links, nlinks, row_cap, mask, carry, seq0)
    want = fr.link_rows(prev, nkp, links, nlinks, row_cap, mask, carry, seq0)
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), (where, np.argwhere(got[0] != want[0])[:5])
    return want


def random_carry(seed, row_cap):
    rng = np.random.default_rng(seed)
    carry = fr.empty_row(row_cap)
    for k in rng.permutation(row_cap)[:max(row_cap // 2, 1)]:
        carry[k] = (int(rng.integers(0, 50)), int(rng.integers(0, row_cap)), int(rng.integers(1, 9)), -1)
    return carry


@pytest.mark.parametrize("n,row_cap", [(1, 8), (2, 64), (3, 65), (8, 300), (9, 8), (33, 65), (65, 64), (65, 300)])
def test_rows_against_the_restatement(vislam, ctx, n, row_cap):
    """random one-to-one lists with gated and restarting frames, without and with a mask and a carried row"""
    prev, nkp, links, nlinks, mask = random_stream(1000 + n + row_cap, n, row_cap, row_cap + 3, hostile=False, first_prev=fr.KF_CARRIED)
    carry = random_carry(n, row_cap)
    for m_, c_ in ((None, None), (mask, carry)):
        _, frames = check_link(vislam, ctx, prev, nkp, links, nlinks, row_cap, m_, c_, seq0=70, where=(n, row_cap, m_ is not None))
    assert n < 8 or frames["n_continued"].any()
    if int(prev[0]) == fr.KF_CARRIED:                               # a track entering through d_carry_in, and the frame that has no row to continue
        assert int(frames[0]["flags"]) == 0
        assert int(fr.link_rows(prev, nkp, links, nlinks, row_cap)[1][0]["flags"]) == fr.FT_NO_CARRY


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 33, 65])
def test_a_track_as_long_as_the_launch(vislam, ctx, n):
    """identity links through every frame (the last doubling round matters), NOT_SAVED frames at both ends and in the middle, FIRST in the middle"""
    R = 65
    links = np.zeros((n, R), fr.DMATCH_DTYPE)
    links["queryIdx"] = links["trainIdx"] = np.arange(R)
    nkp, nlinks = np.full(n, R, np.int32), np.full(n, R, np.int32)
    prev = np.arange(-1, n - 1).astype(np.int32)
    carry = fr.empty_row(R)
    carry[:] = [(3, (7 * k) % R, 5, -1) for k in range(R)]
    obs, frames = check_link(vislam, ctx, prev, nkp, links, nlinks, R, None, carry, seq0=9, where=("chain", n))
    assert (obs[n - 1]["len"] == 5 + n).all() and (obs[n - 1]["birth_seq"] == 3).all()
    prev[0] = fr.KF_FIRST
    obs, frames = check_link(vislam, ctx, prev, nkp, links, nlinks, R, where=("chain from FIRST", n))
    assert (obs[n - 1]["len"] == n).all() and (obs[n - 1]["birth_seq"] == 0).all() and int(frames[n - 1]["max_len"]) == n
    if n >= 8:
        gated = prev.copy()
        gated[0] = gated[3] = gated[n - 1] = fr.KF_NOT_SAVED       # both ends and the middle: the saved frames link across the gap
        gated[1], gated[4] = fr.KF_CARRIED, 2
        gated[6] = fr.KF_FIRST                                      # a restart in the middle
        obs, frames = check_link(vislam, ctx, gated, nkp, links, nlinks, R, None, carry, where=("gated", n))
        assert (obs[5]["len"] == 5 + 4).all() and (obs[6]["len"] == 1).all() and int(frames[3]["flags"]) == fr.FT_NO_PAIR
        assert (obs[3].tobytes() == fr.empty_row(R).tobytes()) and int(frames[n - 1]["n_keypoints"]) == 0


# ---------------------------------------------------------------------------------------------- N-view rows
def tri_on_device(vislam, c, tp, prev, nkp, obs, xy, poses):
    import torch
    n, R = obs.shape
    d = [_dev(torch, a) for a in (np.asarray(prev, np.int32), np.asarray(nkp, np.int32), obs.reshape(-1).view(np.uint8), np.asarray(xy, np.float32),
                                  np.asarray(poses, np.float64))]
    pts, fl, sm = _filled(torch, (n * R + 2) * 40), _filled(torch, n * R + 16), _filled(torch, (n + 2) * 32)
    c.ftrack_triangulate_rows(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), R, d[3].data_ptr(), d[4].data_ptr(), pts.data_ptr(), fl.data_ptr(),
                              sm.data_ptr(), tp)
    c.batch_sync()
    rp, rf, rs = pts.cpu().numpy(), fl.cpu().numpy(), sm.cpu().numpy()
    assert (rp[n * R * 40:] == FILL).all() and (rf[n * R:] == FILL).all() and (rs[n * 32:] == FILL).all()
    return rp[:n * R * 40].view(vislam.FTRACK_POINT_DTYPE).reshape(n, R), rf[:n * R].reshape(n, R), rs[:n * 32].view(vislam.FTRACK_TRI_SUMMARY_DTYPE)


def check_tri(vislam, c, cam, prev, nkp, obs, xy, poses, where, **kw):
    tp, tq = vislam.default_ftrack_tri_params(), fr.TriParams()
    for k, v in kw.items():
        setattr(tp, k, v)
        setattr(tq, k, v)
    n, R = obs.shape
    got = tri_on_device(vislam, c, tp, prev, nkp, obs, xy, poses)
    fill_p = np.full(n * R * 40, FILL, np.uint8).view(fr.POINT_DTYPE).reshape(n, R)
    want = fr.triangulate_rows(tq, cam, prev, nkp, obs, xy, poses, fill_p, np.full((n, R), FILL, np.uint8))
    assert got[2].tobytes() == want[2].tobytes(), (where, got[2], want[2])
    assert got[1].tobytes() == want[1].tobytes(), (where, np.argwhere(got[1] != want[1])[:5])
    bad = [(i, k) for i in range(n) for k in range(R) if got[0][i, k].tobytes() != want[0][i, k].tobytes()]
    assert not bad, (where, bad[:3], got[0][bad[0]], want[0][bad[0]])
    return want


@pytest.fixture(scope="module")
def cam_ctx(vislam):
    """a context whose camera is the planted scenes'"""
    p = vislam.default_params()
    p.fx, p.fy, p.cx, p.cy = CAM.fx, CAM.fy, CAM.cx, CAM.cy
    c = vislam.Context(0, p)
    yield c
    c.close()


def chain_scene(n, R, noise=0.3, seed=4):
    """n cameras seeing R points, keypoint k of every frame the same point; link lists of the identity"""
    X, poses, xy = planted(seed, noise, n_cam=n, n_pts=R)
    links = np.zeros((n, R), fr.DMATCH_DTYPE)
    links["queryIdx"] = links["trainIdx"] = np.arange(R)
    prev = np.arange(-1, n - 1).astype(np.int32)
    prev[0] = fr.KF_FIRST
    return X, np.array(poses), np.stack(xy), links, prev


@pytest.mark.parametrize("gn_iters", [0, 5, 10])
def test_nview_rows_against_the_restatement(vislam, cam_ctx, gn_iters):
    """tracks of 1 (FEW), 2, max_views and max_views + 1 views -- the window keeps the newest -- a frame without a pose in the middle, rows that are
    not track ends; R = 70 crosses a wave"""
    n, R = 6, 70
    X, poses, xy, links, prev = chain_scene(n, R)
    nkp = np.full(n, R, np.int32)
    nlinks = np.array([0, R, R, R, R - 6, R - 3], np.int32)        # keypoints R-6.. end at frame 3 (4 views) and restart; R-3.. have 1 view at frame 5
    obs, _ = fr.link_rows(prev, nkp, links, nlinks, R)
    poses[2] = np.nan                                               # no pose in the middle of every track
    want = check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, ("chains", gn_iters), gn_iters=gn_iters, max_views=5)
    pts, fl, sm = want
    assert sm["n_ends"].tolist() == [0, 0, 0, 6, 3, R] and int(sm[5]["n_few"]) == 3 and int(sm[4]["n_few"]) == 3
    assert int(pts[5, 0]["n_views"]) == 4 and int(pts[3, R - 1]["n_views"]) == 3 and int(pts[5, R - 4]["n_views"]) == 2      # 5 walked, one without a pose
    assert int(sm[5]["n_kept"]) >= R - 10 and not fl[:3].any()
    err = np.linalg.norm(pts[5, :R - 6]["X"] - X[:R - 6], axis=1)
    assert np.median(err) < 0.2, np.median(err)


def test_nview_rows_degenerate_geometry(vislam, cam_ctx):
    """a point behind one camera, two identical cameras, a NOT_SAVED frame inside a track, counts above the capacity and below zero"""
    n, R = 6, 12
    X, poses, xy, links, prev = chain_scene(n, R, noise=0.0)
    nkp = np.array([R, R + 9, R, R, R, -4], np.int32)
    prev = np.array([fr.KF_FIRST, 0, fr.KF_NOT_SAVED, 1, 3, 4], np.int32)
    nlinks = np.array([0, R, R, R - 4, R, R], np.int32)            # the last four keypoints of frame 1 end there: two views, frames 1 and 0
    obs, _ = fr.link_rows(prev, nkp, links, nlinks, R)
    poses[1] = poses[0]                                             # two identical cameras
    D = np.diag([-1.0, 1.0, -1.0])                                  # camera 4 turned half round about its y axis, its pixels mirrored to match:
    poses[4, :9], poses[4, 9:] = (D @ poses[4, :9].reshape(3, 3)).reshape(9), D @ poses[4, 9:]      # every point reprojects exactly and lies behind it
    xy = xy.copy()
    xy[4, :, 1] = np.float32(2.0 * CAM.cy) - xy[4, :, 1]
    pts, fl, sm = check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, "degenerate")
    assert sm["n_ends"].tolist() == [0, 4, 0, 0, R, 0] and pts[1, R - 4:]["n_views"].tolist() == [2] * 4 and int(pts[4, 0]["n_views"]) == 4
    assert all(int(f) & fr.FTP_SINGULAR or not int(f) & fr.FTP_PARALLAX_OK for f in fl[1, R - 4:])
    assert not (fl[4] & (fr.FTP_KEPT | fr.FTP_FRONT)).any() and (fl[4, R - 4:] & fr.FTP_REPROJ_OK).all()      # (frames 4 and 3 alone)


# ---------------------------------------------------------------------------------------------- the plan's frames
W, H, B = 752, 480, 16


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(2 * B)])
    g = f.copy()
    g[5] = g[B + 5] = 128                                          # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


def _launch_lists(vislam, orc, c, p, n, carried_kps, want_sym):
    """what the getters return for the last run: prev, keypoints, the good lists, the symmetric lists (the oracle's filter on the device's kNN rows,
    as tests/test_pnp_gpu.py rebuilds them), the pose stage's masks"""
    prev = c.batch_get_keyframes()
    kps = [c.batch_keypoints(i)[0] for i in range(n)]
    good = [c.batch_matches(i)[0] for i in range(n)]
    sym = None
    if want_sym:
        sym = []
        for i in range(n):
            kq = kps[prev[i]] if prev[i] >= 0 else carried_kps if prev[i] == vislam.KF_CARRIED else None
            sym.append(np.zeros(0, vislam.DMATCH_DTYPE) if kq is None else orc.good_matches(p, kq, kps[i], *c.batch_knn(i))[1])
    masks = [c.batch_inlier_mask(i) for i in range(n)]
    return prev, kps, good, sym, masks


def _as_rows(lists, cap):
    rows, cnt = np.zeros((len(lists), cap), fr.DMATCH_DTYPE), np.zeros(len(lists), np.int32)
    for i, l in enumerate(lists):
        rows[i, :len(l)], cnt[i] = l, len(l)
    return rows, cnt


@pytest.mark.parametrize("gate,sym", [(False, False), (True, False), (False, True)])
def test_batch_ftrack_over_two_launches(vislam, orc, stream, gate, sym):
    import torch
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    if sym:
        p.pose_input, p.keypoint_capacity = 1, 2048
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, 2 * B)
    KC = c.keypoint_capacity(W, H)
    CAP = KC + 5
    ROOT2 = int(np.floor(np.sqrt(p.n_cells))) ** 2
    dev = _dev(torch, stream[gate])
    arg = lambda t: C.c_void_p(t.data_ptr())
    # (source, pose_inliers) variants: every list, and the pose stage's mask on the list it saw
    variants = [(vislam.FT_SYM, False), (vislam.FT_GOOD, False), (vislam.FT_SYM if sym else vislam.FT_GOOD, True)]
    seen = dict(long=0, cross=0, continued=0)
    two_launch = {}
    for src, inl in variants:
        for cuts in ((B, B), (2 * B,)):
            if len(cuts) == 1 and (src, inl) != variants[0]:
                continue
            c.batch_reset()
            carry, carried_kps, at, rows_all = None, None, 0, []
            for launch, n in enumerate(cuts):
                obs, frames = _filled(torch, (n * CAP + 2) * 16), _filled(torch, (n + 2) * 32)
                c.batch_run(dev.data_ptr() + at * W * H, n, vislam.STAGE_ALL)
                call = lambda s=src, i_=int(inl), n_=n, m=None, mc=0, cap=CAP: vislam.lib.vis_batch_ftrack(c._h, s, i_, n_, m, mc, cap, arg(obs), arg(frames))
                if launch == 0 and len(cuts) == 2 and (src, inl) == variants[0]:        # the refusals that need a plan, in the header's order
                    assert call(s=2, cap=KC - 1, n_=n - 1) == -1   # VIS_E_INVALID before anything else
                    assert call(cap=KC - 1, n_=n - 1) == -4 and call(m=arg(obs), mc=KC - 1, n_=n - 1) == -4      # VIS_E_CAPACITY before VIS_E_STATE
                    assert call(s=vislam.FT_GOOD, m=arg(obs), mc=ROOT2 - 1, n_=n - 1) == -4 and call(n_=n - 1) == -5
                    assert call(s=vislam.FT_GOOD if sym else vislam.FT_SYM, i_=1) == -1                          # not the list the pose stage saw
                    assert (obs.cpu().numpy() == FILL).all() and (frames.cpu().numpy() == FILL).all()
                c.batch_ftrack(n, CAP, obs.data_ptr(), frames.data_ptr(), src, inl)
                c.batch_sync()
                assert c.batch_status() == 0
                prev, kps, good, syms, masks = _launch_lists(vislam, orc, c, p, n, carried_kps, src == vislam.FT_SYM)
                lists = syms if src == vislam.FT_SYM else good
                links, nl = _as_rows(lists, KC if src == vislam.FT_SYM else ROOT2)
                mask = None
                if inl:
                    mask = np.zeros((n, links.shape[1]), np.uint8)
                    for i in range(n):
                        mask[i, :len(masks[i])] = masks[i]
                        nl[i] = min(nl[i], len(masks[i]))          # (the pose stage's first n_points bytes)
                nkp = np.array([len(k) for k in kps], np.int32)
                w_obs, w_fr = fr.link_rows(prev, nkp, links, nl, KC, mask, carry, seq0=at)
                ro, rf = obs.cpu().numpy(), frames.cpu().numpy()
                assert (ro[n * CAP * 16:] == FILL).all() and (rf[n * 32:] == FILL).all()
                g_obs = ro[:n * CAP * 16].view(vislam.FTRACK_OBS_DTYPE).reshape(n, CAP)
                assert rf[:n * 32].tobytes() == w_fr.tobytes(), (src, inl, launch, rf[:n * 32].view(vislam.FTRACK_FRAME_DTYPE), w_fr)
                assert g_obs[:, :KC].tobytes() == w_obs.tobytes(), (src, inl, launch)
                assert (g_obs[:, KC:].view(np.uint8) == FILL).all()  # only the first keypoint-capacity entries of a row are written
                assert not (w_fr["flags"] & vislam.FT_NO_CARRY).any()
                carry, carried_kps = fr.carry_out(prev, w_obs, carry, KC), [k for i, k in enumerate(kps) if prev[i] != vislam.KF_NOT_SAVED][-1]
                rows_all.append(w_obs)
                if launch == 1:                                     # the second launch's tracks continue the first's
                    cross = (w_obs["birth_seq"] >= 0) & (w_obs["birth_seq"] < B) & (w_obs["len"] > 2)
                    assert cross.any(), (src, inl)
                    seen["cross"] += int(cross.sum())
                seen["continued"] += int(w_fr["n_continued"].sum())
                seen["long"] = max(seen["long"], int(w_fr["max_len"].max()))
                at += n
            if (src, inl) == variants[0]:
                two_launch[len(cuts)] = np.concatenate(rows_all)
    assert two_launch[2].tobytes() == two_launch[1].tobytes()       # the same 32 frames as one launch: the same observations
    # skipping the call on launch 0 sets VIS_FT_NO_CARRY on launch 1, on the frame whose pair is the carried keyframe and only there
    c.batch_reset()
    obs, frames = _filled(torch, B * CAP * 16), _filled(torch, B * 32)
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_ALL)
    c.batch_run(dev.data_ptr() + B * W * H, B, vislam.STAGE_ALL)
    c.batch_ftrack(B, CAP, obs.data_ptr(), frames.data_ptr())
    c.batch_sync()
    f = frames.cpu().numpy().view(vislam.FTRACK_FRAME_DTYPE)
    prev = c.batch_get_keyframes()
    assert [int(x) & vislam.FT_NO_CARRY for x in f["flags"]] == [vislam.FT_NO_CARRY if q == vislam.KF_CARRIED else 0 for q in prev] and int(prev[0]) == vislam.KF_CARRIED
    assert f["seq"].tolist() == list(range(B, 2 * B))               # the plan counted the frames of the launch that was not linked
    # N-view on the plan's keypoints with poses chained on the host (any finite poses do: the comparison is against the restatement)
    kps = [c.batch_keypoints(i)[0] for i in range(B)]
    nkp = np.array([len(k) for k in kps], np.int32)
    poses = np.zeros((B, 12))
    for i in range(B):
        a = 0.002 * i
        poses[i, :9] = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
        poses[i, 9:] = [-0.05 * i, 0.0, 0.0]
    poses[:8] = 0.0                                                 # R all zero: no pose (and the tracks that end in those frames are FEW at once)
    poses[11] = np.nan                                              # no pose in the middle of the tracks that are triangulated
    tp, tq = vislam.default_ftrack_tri_params(), fr.TriParams(max_views=8, gn_iters=2)
    tp.max_views, tp.gn_iters = 8, 2                                # (the restatement is plain Python: a few thousand points)
    pts, fl, sm = _filled(torch, (B * CAP + 1) * 40), _filled(torch, B * CAP + 8), _filled(torch, (B + 1) * 32)
    d_poses = _dev(torch, poses)
    c.batch_ftrack_triangulate(B, obs.data_ptr(), CAP, d_poses.data_ptr(), pts.data_ptr(), fl.data_ptr(), sm.data_ptr(), tp)
    c.batch_sync()
    assert c.batch_status() == 0
    h_obs = obs.cpu().numpy().view(vislam.FTRACK_OBS_DTYPE).reshape(B, CAP)
    xy = np.zeros((B, CAP, 2), np.float32)
    for i in range(B):
        xy[i, :len(kps[i]), 0], xy[i, :len(kps[i]), 1] = kps[i]["x"], kps[i]["y"]
    cam = fr.Camera(p.fx, p.fy, p.cx, p.cy)
    fill_p = np.full(B * CAP * 40, FILL, np.uint8).view(fr.POINT_DTYPE).reshape(B, CAP)
    # (the restatement clamps the counts to its row length CAP; the plan clamps to the keypoint capacity, which no count exceeds)
    w_pts, w_fl, w_sm = fr.triangulate_rows(tq, cam, prev, nkp, h_obs, xy, poses, fill_p, np.full((B, CAP), FILL, np.uint8))
    rp, rf, rs = pts.cpu().numpy(), fl.cpu().numpy(), sm.cpu().numpy()
    assert (rp[B * CAP * 40:] == FILL).all() and (rf[B * CAP:] == FILL).all() and (rs[B * 32:] == FILL).all()
    assert rs[:B * 32].tobytes() == w_sm.tobytes(), (rs[:B * 32].view(fr.TRI_SUMMARY_DTYPE), w_sm)
    assert rf[:B * CAP].tobytes() == w_fl.tobytes() and rp[:B * CAP * 40].tobytes() == w_pts.tobytes()
    assert int(w_sm["n_points"].sum()) > 100 and int(w_sm["n_ends"].sum()) == int(nkp[[i for i in range(B) if prev[i] != vislam.KF_NOT_SAVED]].sum()) - \
        int(f["n_continued"].sum())
    # a run without the match stage has no lists to link
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_DETECT)
    assert vislam.lib.vis_batch_ftrack(c._h, 0, 0, B, None, 0, CAP, arg(obs), arg(frames)) == -5
    c.batch_sync()
    c.close()
    # a join that links nothing shows nothing
    assert seen["cross"] >= 50 and seen["long"] > 2 and seen["continued"] >= 500, seen
    print(f"\ngate {gate}, symmetric pose input {sym}: {seen}")


def test_run_directory_writes_the_tracks(vislam, stream, tmp_path):
    """tools/run_directory.py --tracks: the CSV holds what vis_batch_ftrack gives for the same frames in the same batches, the tracks continuing
    across the batches"""
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    frames = stream[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "tracks.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--tracks", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [[int(v) for v in l.split(",")] for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    cap = c.keypoint_capacity(W, H)
    dev = _dev(torch, frames)
    recs, lens = [], []
    for first in range(0, n, nb):
        obs, fr_ = _filled(torch, nb * cap * 16), _filled(torch, nb * 32)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_ftrack(nb, cap, obs.data_ptr(), fr_.data_ptr())
        c.batch_sync()
        recs += list(fr_.cpu().numpy().view(vislam.FTRACK_FRAME_DTYPE))
        lens += list(obs.cpu().numpy().view(vislam.FTRACK_OBS_DTYPE).reshape(nb, cap)["len"])
    c.close()
    assert len(rows) == n == len(recs)
    bins = j["tracks"]["histogram_bins"]
    for k, (row, f) in enumerate(zip(rows, recs)):
        assert len(row) == 2 + 8 + len(bins) and row[0] == k and row[1] == 1403636579763555584 + 50000000 * k
        assert row[2:10] == [int(f[name]) for name in vislam.FTRACK_FRAME_DTYPE.names], k
        l = lens[k][:int(f["n_keypoints"])]
        assert row[10:] == [int(((l >= lo) & (l < hi)).sum()) for lo, hi in zip(bins, bins[1:] + [2 ** 31])] and sum(row[10:]) == int(f["n_keypoints"])
    assert j["tracks"]["no_carry"] == 0 and j["tracks"]["max_len"] == max(int(f["max_len"]) for f in recs) > nb      # a track crosses the batches
    assert j["tracks"]["continued"] == sum(int(f["n_continued"]) for f in recs) and j["tracks"]["observations"] == sum(int(f["n_keypoints"]) for f in recs)
