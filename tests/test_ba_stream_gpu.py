"""GPU: the stream-ordering rules of the windowed bundle adjustment.

vis_ba_rows on a CALLER's stream S (vis_set_stream) with every input -- d_poses among them -- still being produced on S when the call is queued:
the late-producer rig of tests/stream_order_cases.py (sync run, late run with the lateness guard, a decoy per input).
vis_batch_ba inside the plan's chain vis_batch_ftrack -> vis_batch_trajectory -> vis_batch_ba -> vis_batch_ftrack_triangulate(d_poses_out), queued
with no host step, against the same calls with vis_batch_sync between them."""
import numpy as np
import pytest

import ba_ref as br
import ftrack_ref as fr
import stream_order_cases as so
from test_trajectory_stream_gpu import Stream, _filled, frames  # noqa: F401  (frames: the module fixture of the trajectory stream test)

pytestmark = pytest.mark.gpu


def case_ba_rows(vislam):
    prev, nkp, links, nlinks, xy, poses = so.ftrack_scene()
    n, K = so.FT_N, so.FT_K
    obs, _ = fr.link_rows(prev, nkp, links, nlinks, K)
    rng = np.random.default_rng(5)
    moved = poses.copy()
    moved[1:, 9:] += 0.01 * rng.standard_normal((n - 1, 3))           # something to refine
    alone = np.tile(np.array([-1, -1, 0, -1], np.int32), n * K)     # every keypoint a track of its own: no point
    ins = dict(prev=(prev, np.full_like(prev, -3)), nkp=(nkp, np.full_like(nkp, K // 2)), obs=(obs, alone), xy=(xy, xy[::-1].copy()),
               poses=(moved, so.zeros(moved)))
    bp = vislam.default_ba_params()
    bp.stride = 4
    outs = dict(poses_out=n * 96, windows=vislam.ba_windows(n, 4) * 80, points=n * K * 40, flags=n * K)
    return so.Case("vis_ba_rows", so.CTX, ins, outs,
                   lambda c, p: c.ba_rows(n, p("prev"), p("nkp"), p("obs"), K, p("xy"), p("poses"), p("poses_out"), p("windows"), p("points"), p("flags"), bp))


def test_ba_rows_reads_poses_that_are_still_being_produced(vislam):
    import torch
    S = torch.cuda.Stream()
    c = vislam.Context(0)
    c.set_stream(S)
    case = case_ba_rows(vislam)
    rig = so.Rig(torch, case)
    delay = so.Delay(torch, S)
    op_ms = delay.measure()
    host = [so.run_sync(torch, c, rig)[1] for _ in range(3)][1:]
    chain_ms, ok = delay.size(max(host))
    assert ok, (chain_ms, host)
    want, _ = so.run_sync(torch, c, rig)
    got, late, host_ms = so.run_late(torch, c, S, delay, rig)
    print(f"\nvis_ba_rows: chain op {op_ms:.4f} ms, host {host_ms:.3f} ms of the late call, chain {delay.chain_ms:.1f} ms")
    assert late, ("the producer had finished when the call returned", host_ms, delay.chain_ms)
    for k in want:
        assert got[k] == want[k], (k, "differs from the synchronised run")
    for name in case.inputs:
        decoy, _ = so.run_sync(torch, c, rig, (name,))
        assert any(decoy[k] != want[k] for k in want), (name, "its decoy gives the bytes of the real input")
    win = np.frombuffer(want["windows"], vislam.BA_WINDOW_DTYPE)
    assert int(win[0]["flags"]) == br.BA_REFINED and int(win[0]["n_accepted"]) > 0 and int(win[0]["n_points"]) > 40
    torch.cuda.synchronize()
    c.close()


def _sequence(vislam, torch, f, gate, sync_each):
    """three launches of 8: the two-view chain, the tracks, the trajectory, the adjustment of the trajectory's poses and the N-view points under
    the adjusted poses, every call into buffers of its own taken before the first call"""
    s = Stream(vislam, torch, f, gate, 8)
    KC, L = s.KC, 3
    bufs = [s.buffers(8) for _ in range(L)]
    nw = vislam.ba_windows(8, 4)
    ft = [dict(obs=_filled(torch, 8 * KC * 16), frames=_filled(torch, 8 * 32), pts=_filled(torch, 8 * KC * 40), fl=_filled(torch, 8 * KC),
               sm=_filled(torch, 8 * 32), ba_poses=_filled(torch, 8 * 96), ba_win=_filled(torch, nw * 80), ba_pts=_filled(torch, 8 * KC * 40),
               ba_fl=_filled(torch, 8 * KC)) for _ in range(L)]
    tp = vislam.default_ftrack_tri_params()
    tp.max_views, tp.gn_iters = 8, 2
    bp = vislam.default_ba_params()
    bp.stride, bp.lm_iters, bp.init_reproj_px = 4, 3, 64.0

    def step():
        if sync_each:
            s.c.batch_sync()

    for k in range(L):
        s.run(8)
        step()
        s.follow(bufs[k], True, False)
        step()
        s.c.batch_ftrack(8, KC, ft[k]["obs"].data_ptr(), ft[k]["frames"].data_ptr())
        step()
        s.follow(bufs[k], False, True, tri=False)                   # vis_batch_trajectory: d_poses
        step()
        s.c.batch_ba(8, ft[k]["obs"].data_ptr(), KC, bufs[k]["poses"].data_ptr(), ft[k]["ba_poses"].data_ptr(), ft[k]["ba_win"].data_ptr(),
                     ft[k]["ba_pts"].data_ptr(), ft[k]["ba_fl"].data_ptr(), bp)
        step()
        s.c.batch_ftrack_triangulate(8, ft[k]["obs"].data_ptr(), KC, ft[k]["ba_poses"].data_ptr(), ft[k]["pts"].data_ptr(), ft[k]["fl"].data_ptr(),
                                     ft[k]["sm"].data_ptr(), tp)
        step()
        s.at += 8
    s.c.batch_sync()
    assert s.c.batch_status() == 0
    got = {name: [b[name].cpu().numpy().tobytes() for b in bufs] for name in bufs[0]}
    got.update({name: [b[name].cpu().numpy().tobytes() for b in ft] for name in ft[0]})
    s.close()
    return got


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_queued_chain_equals_the_step_by_step_one(vislam, frames, gate):
    import torch
    f = frames[gate][:24]
    queued, synced = _sequence(vislam, torch, f, gate, False), _sequence(vislam, torch, f, gate, True)
    win = np.frombuffer(b"".join(synced["ba_win"]), vislam.BA_WINDOW_DTYPE)
    sm = np.frombuffer(b"".join(synced["sm"]), fr.TRI_SUMMARY_DTYPE)
    print(f"\ngate {gate}: windows {win['flags'].tolist()}, points {win['n_points'].tolist()}, accepted {win['n_accepted'].tolist()}, "
          f"{int(sm['n_points'].sum())} N-view points under the adjusted poses")
    assert int(win["n_points"].sum()) > 0 and int(sm["n_ends"].sum()) > 100       # not a comparison of empty records
    for name in synced:
        for k in range(3):
            assert queued[name][k] == synced[name][k], (name, k)


def test_run_directory_writes_the_adjusted_poses(vislam, frames, tmp_path):
    """tools/run_directory.py --trajectory --ba: one row per frame, the poses vis_batch_ba gives for the same frames in the same batches"""
    import json
    import os
    import subprocess
    import sys

    import torch
    from test_trajectory_stream_gpu import H, W, _dev
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    f = frames[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + f[t].tobytes())
    tcsv, csv = tmp_path / "trajectory.csv", tmp_path / "ba.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--trajectory", str(tcsv), "--ba", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    cap, kc = int(np.floor(np.sqrt(p.n_cells))) ** 2, c.keypoint_capacity(W, H)
    dev = _dev(torch, f)
    want, wins = [], []
    for first in range(0, n, nb):
        pts, fl, sm, link, traj, poses = (_filled(torch, b) for b in (nb * cap * 32, nb * cap, nb * 16, nb * 40, nb * 128, nb * 96))
        obs, fr_, bpo, bwi, bpt, bfl = (_filled(torch, b) for b in (nb * kc * 16, nb * 32, nb * 96, 80, nb * kc * 40, nb * kc))
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_triangulate(nb, cap, pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
        c.batch_scale_links(nb, pts.data_ptr(), fl.data_ptr(), cap, link.data_ptr())
        c.batch_trajectory(nb, link.data_ptr(), traj.data_ptr(), poses.data_ptr())
        c.batch_ftrack(nb, kc, obs.data_ptr(), fr_.data_ptr())
        c.batch_ba(nb, obs.data_ptr(), kc, poses.data_ptr(), bpo.data_ptr(), bwi.data_ptr(), bpt.data_ptr(), bfl.data_ptr())
        c.batch_sync()
        want += list(bpo.cpu().numpy().view(np.float64).reshape(nb, 12))
        wins += list(bwi.cpu().numpy().view(vislam.BA_WINDOW_DTYPE))
    c.close()
    assert len(rows) == n and j["ba_csv"] == str(csv) and j["ba"]["windows"] == 2 == len(wins)
    for i, row in enumerate(rows):
        assert [int(v) for v in row[:4]] == [i, 1403636579763555584 + 50000000 * i, int(wins[i // nb]["flags"]), int(wins[i // nb]["n_points"])], i
        assert [float(v) for v in row[4:]] == [float(v) for v in want[i]], i
    assert j["ba"]["points"] == sum(int(w["n_points"]) for w in wins) and j["ba"]["cost1"] <= j["ba"]["cost0"]
