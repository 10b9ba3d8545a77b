"""GPU: the follow-ups of a batch step queued without a sync equal the same sequence synchronised after every call.

vis_batch_triangulate, vis_batch_pnp, vis_batch_filter_keypoints and vis_batch_klt each queue on the pose stream behind the last
vis_batch_run and note a reader event on the buffer sets they read (csrc/vis_internal.h on_pose_stream; DESIGN.md has the table).  A
missing wait or a missing note shows as a step that reads a set the next-but-one step already rewrites: four launches of 8 on a plan of
8, because a set is rewritten two steps after it was read, every launch into output buffers of its own.

The frames are those of tests/test_pnp_gpu.py (vis_synth_frame_parallax, 752 x 480, t = 0 ... 31, fy = fx, min_inliers 6), plain and with
the keyframe gate on and frames 5 and 21 flat, so that the link table has readers too.  Every output buffer of every launch is compared
byte for byte.  The filter's rotations are the identity and its translations arbitrary directions: what it keeps is not a motion estimate,
only rows that depend on every matched point they read."""
import numpy as np
import pytest

import pnp_ref as pr

pytestmark = pytest.mark.gpu
FILL = 0xEE
W, H, B, STEPS = 752, 480, 8, 4
CAP = 49
FILTER_T = 2000.0              # FilterKeypoints keeps |t . n| < 10^(-1000 / T) = 0.32: with arbitrary translations, rows of kept AND dropped points


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(STEPS * B)])
    g = f.copy()
    g[5] = g[21] = 128                                             # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


def _sequence(vislam, torch, frames, gate, sync_each):
    """{buffer name: [bytes of launch 0, ...]} of the four launches"""
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    pp = vislam.default_pnp_params()
    pp.min_inliers = 6
    kp = vislam.default_klt_params()
    kp.fb_max_px = 1.0
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    kcap = c.keypoint_capacity(W, H)
    dev = _dev(torch, frames)
    d_draws = _dev(torch, pr.make_draws(7))
    d_rot = _dev(torch, np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)))
    d_t = _dev(torch, np.random.default_rng(79).normal(0, 1, (B, 3)).astype(np.float32))
    sizes = dict(points=B * CAP * 32, flags=B * CAP, summary=B * 16,                                     # vis_batch_triangulate
                 pnp=B * vislam.PNP_RESULT_DTYPE.itemsize, link=B * vislam.PNP_LINK_DTYPE.itemsize, mask=B * CAP,
                 keep=B * CAP, nkeep=B * 4,                                                              # vis_batch_filter_keypoints
                 klt=B * kcap * vislam.KLT_POINT_DTYPE.itemsize, pair=B * vislam.KLT_PAIR_DTYPE.itemsize, p1=B * kcap * 8, p2=B * kcap * 8, ntracked=B * 4)
    outs = [{k: _filled(torch, v) for k, v in sizes.items()} for _ in range(STEPS)]
    poses = [np.zeros(B, vislam.POSE_RESULT_DTYPE) for _ in range(STEPS)]

    def step():
        if sync_each:
            c.batch_sync()

    for k, o in enumerate(outs):
        ptr = dev.data_ptr() + k * B * W * H
        c.batch_run(ptr, B, vislam.STAGE_ALL | vislam.STAGE_GRADIENT)
        step()
        c.batch_triangulate(B, CAP, o["points"].data_ptr(), o["flags"].data_ptr(), o["summary"].data_ptr())
        step()
        c.batch_pnp(B, d_draws.data_ptr(), o["points"].data_ptr(), o["flags"].data_ptr(), CAP, o["pnp"].data_ptr(), o["link"].data_ptr(), vislam.MP_KEPT,
                    CAP, o["mask"].data_ptr(), pp)
        step()
        c.batch_filter_keypoints(B, d_rot.data_ptr(), d_t.data_ptr(), FILTER_T, CAP, o["keep"].data_ptr(), o["nkeep"].data_ptr())
        step()
        c.batch_klt(ptr, B, kcap, o["klt"].data_ptr(), o["pair"].data_ptr(), 0, o["p1"].data_ptr(), o["p2"].data_ptr(), o["ntracked"].data_ptr(), kp)
        step()
        c.batch_results_async(B, poses[k].ctypes.data)
        step()
    c.batch_sync()
    assert c.batch_status() == 0
    got = {name: [o[name].cpu().numpy().tobytes() for o in outs] for name in sizes}
    got["poses"] = [q.tobytes() for q in poses]
    c.close()
    return got


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_queued_follow_ups_equal_synchronised_ones(vislam, stream, gate):
    import torch
    queued = _sequence(vislam, torch, stream[gate], gate, False)
    synced = _sequence(vislam, torch, stream[gate], gate, True)
    # not a comparison of empty records (conditions on the synchronised run)
    pnp = np.frombuffer(b"".join(synced["pnp"]), vislam.PNP_RESULT_DTYPE)
    nkeep = [np.frombuffer(b, np.int32) for b in synced["nkeep"]]
    pairs = np.frombuffer(b"".join(synced["pair"]), vislam.KLT_PAIR_DTYPE)
    winners, tracked = int((pnp["best_iter"] >= 0).sum()), int((pairs["n_tracked"] > 0).sum())
    print(f"\ngate {gate}: {winners} PnP winners, n_keep per launch {[v[v > 0].tolist() for v in nkeep]}, {tracked} KLT pairs with tracked points")
    assert winners >= 4
    assert all((v > 0).any() for v in nkeep)
    assert tracked >= 20
    for name in synced:
        for k in range(STEPS):
            assert queued[name][k] == synced[name][k], (name, k)
