"""GPU: the feature-track kernels on hostile rows, BYTE FOR BYTE against tests/ftrack_ref.py with 0xEE-filled outputs (nothing behind the written
extent may change, and no index a caller controls may be followed out of a row).

Linking: duplicate trainIdx and duplicate queryIdx, indices at nkp, at -1 and at the ends of int32, list and keypoint counts above their
capacities and below zero, a mask shorter than the lists, a mask of all zeros, prev[] entries that name a later frame, the frame itself or no
VIS_KF_* value, a carried row with garbage behind its keypoints.
N-view: prev_kp out of range in either direction, prev[] that is no earlier frame, a non-finite pixel (the view is dropped), a +-3e38 pixel
(used as it stands: the flags fail), poses with NaN, infinity, an all-zero R (no pose) and entries of 1e200 (a pose, and whatever overflows ends
in flags that fail)."""
import numpy as np
import pytest

import ftrack_ref as fr
from test_ftrack_gpu import CAM, cam_ctx, chain_scene, check_link, check_tri, random_carry      # noqa: F401  (cam_ctx is a fixture)
from test_ftrack_ref import random_stream

pytestmark = pytest.mark.gpu
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.mark.parametrize("seed,n,row_cap,link_cap", [(0, 9, 8, 8), (1, 8, 64, 70), (2, 33, 65, 65), (3, 3, 300, 311), (4, 65, 64, 40)])
def test_hostile_lists(vislam, ctx, seed, n, row_cap, link_cap):
    """random_stream's hostile lists: duplicates on either side, indices at nkp / -1 / beyond, counts above the capacities and below zero"""
    prev, nkp, links, nlinks, mask = random_stream(seed, n, row_cap, link_cap, first_prev=fr.KF_CARRIED)
    carry = random_carry(seed, row_cap)
    carry[0] = (I32_MAX, I32_MIN, I32_MIN, 77)                      # len <= 0: not a keypoint of the carried frame, whatever else it holds
    carry[row_cap - 1] = (5, I32_MAX, 0, -9)
    short = np.ascontiguousarray(mask[:, :max(link_cap // 2, 1)])  # mask_cap < link_cap: the counts are clamped to it
    for m_, c_ in ((None, None), (mask, carry), (short, carry), (np.zeros_like(mask), carry), (None, carry)):
        want = check_link(vislam, ctx, prev, nkp, links, nlinks, row_cap, m_, c_, seq0=I32_MAX - n, where=(seed, None if m_ is None else m_.shape))
    assert not fr.link_rows(prev, nkp, links, nlinks, row_cap, np.zeros_like(mask), carry)[1]["n_continued"].any()
    assert n < 8 or want[1]["n_continued"].any()


def test_every_entry_hostile(vislam, ctx):
    """lists made of nothing but duplicates and out-of-range indices, counts at the ends of int32, prev[] that is no pairing"""
    n, R = 9, 65
    links = np.zeros((n, R), fr.DMATCH_DTYPE)
    bad = np.array([-1, R, R + 1, I32_MIN, I32_MAX, 64, 64, 0, 0], np.int64)
    for i in range(n):
        links[i]["queryIdx"] = bad[(np.arange(R) + i) % len(bad)]
        links[i]["trainIdx"] = bad[(np.arange(R) * 3 + i) % len(bad)]
    nkp = np.array([R, I32_MAX, I32_MIN, 64, 65, 0, -1, R, R], np.int32)
    nlinks = np.array([I32_MAX, I32_MAX, R, I32_MIN, R + 1, R, R, -1, R], np.int32)
    prev = np.array([7, 1, 5, fr.KF_CARRIED, I32_MIN, 3, -4, 6, I32_MAX], np.int32)   # a later frame, itself, a later one, carried, garbage ...
    carry = random_carry(3, R)
    for c_ in (None, carry):
        obs, frames = check_link(vislam, ctx, prev, nkp, links, nlinks, R, None, c_, where="every entry hostile")
    assert frames["flags"].tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1]


def test_hostile_observations_and_pixels(vislam, cam_ctx):
    n, R = 6, 16
    X, poses, xy, links, prev = chain_scene(n, R, noise=0.2)
    nkp = np.full(n, R, np.int32)
    obs, _ = fr.link_rows(prev, nkp, links, np.full(n, R, np.int32), R)
    obs = obs.copy()
    obs[5, 0]["prev_kp"], obs[5, 1]["prev_kp"], obs[5, 2]["prev_kp"], obs[4, 3]["prev_kp"] = R, I32_MAX, I32_MIN, -1       # out of range: the walk ends there
    obs[3, 4]["prev_kp"] = 5                                        # two keypoints name the same parent: both walk on through it
    nkp[1] = 10                                                     # keypoints 10 ... of frame 1 do not exist: the tracks through them end at frame 2
    xy = xy.copy()
    xy[4, 6, 0], xy[3, 7, 1], xy[5, 8] = np.nan, np.inf, (-np.inf, np.nan)      # the view is dropped
    xy[4, 9, 0], xy[2, 10, 1], xy[5, 11] = 3e38, -3e38, (3e38, 3e38)            # used as it stands
    want = check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, "hostile rows")
    pts, fl, sm = want
    assert int(pts[5, 6]["n_views"]) == 5 and int(pts[5, 7]["n_views"]) == 5 and int(pts[5, 8]["n_views"]) == 5      # one view of six dropped
    assert not (fl[5, 9:12] & fr.FTP_KEPT).any() and int(pts[5, 9]["n_views"]) == 6
    assert int(pts[5, 0]["n_views"]) == 1 and int(fl[5, 0]) == fr.FTP_FEW and int(pts[5, 12]["n_views"]) == 4        # frames 5 ... 2
    for hostile_prev in ([fr.KF_FIRST, 0, 5, 1, 4, I32_MAX], [I32_MIN, 0, 1, -7, fr.KF_NOT_SAVED, 4]):
        check_tri(vislam, cam_ctx, CAM, np.array(hostile_prev, np.int32), nkp, obs, xy, poses, ("hostile prev", hostile_prev[2]))


def test_hostile_poses(vislam, cam_ctx):
    n, R = 6, 8
    X, poses, xy, links, prev = chain_scene(n, R, noise=0.2)
    nkp = np.full(n, R, np.int32)
    obs, _ = fr.link_rows(prev, nkp, links, np.full(n, R, np.int32), R)
    poses = poses.copy()
    poses[1, 3] = np.nan                                            # no pose
    poses[2, 10] = np.inf                                           # no pose
    poses[3, :9] = 0.0                                              # R all zero: no pose
    pts, fl, sm = check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, "no pose")
    assert (pts[5]["n_views"] == 3).all() and (fl[5] & fr.FTP_KEPT).all()
    poses[4] = 1e200                                                # finite: a pose, and what overflows fails its flags
    poses[0, 9:] = -1e200
    pts, fl, sm = check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, "huge pose")
    assert not (fl[5] & fr.FTP_KEPT).any()
    for gn in (0, 10):
        check_tri(vislam, cam_ctx, CAM, prev, nkp, obs, xy, poses, ("huge pose", gn), gn_iters=gn, max_views=2, min_views=2)
