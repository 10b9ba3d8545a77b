#!/usr/bin/env python3
"""Probe: what the windowed bundle adjustment costs behind every launch of the pipelined stream path.  The baseline ("chain") is the chain as it
was: vis_batch_run(VIS_STAGE_ALL) on 1024 S-752 frames per launch (752 x 480, no sync between launches) with vis_batch_triangulate,
vis_batch_scale_links, vis_batch_trajectory, vis_batch_ftrack and vis_batch_ftrack_triangulate (on the trajectory's own d_poses) queued behind
each; the variants "ba4", "ba8", "ba16" add vis_batch_ba at that stride between the trajectory and the N-view triangulation, which then reads the
adjusted poses.  The variants alternate in ONE process, each on a context of its own, so that clocks and placement drift hit all alike; the window
is closed by vis_batch_sync and a device synchronise.

  python3 tools/ba_probe.py [--rounds 5] [--steps 10] [--shape headline|config3] [--profile]

--shape config3: BASELINE config 3 (1920 x 1080, 4000 features on 4 levels, 64 frames per launch).
--profile then runs a short "ba8" leg in a fresh child process under `rocprofv3 --kernel-trace --stats` (no counters in the same run) and prints
the stats rows of the k_ba_* kernels.  One JSON line per measurement; the "ba" lines carry what the last launch adjusted: windows by flag, points,
observations, accepted and rejected steps, and how many of the device's compute units a launch of that many workgroups leaves without one."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
R, DIM = 2, 4096
SHAPES = {"headline": dict(w=752, h=480, B=1024, seed=0xE0C00001), "config3": dict(w=1920, h=1080, B=64, seed=0xE0C00003)}
KERNELS = ("k_ba_window", "k_ba_stitch", "k_ba_points")
VARIANTS = ("chain", "ba4", "ba8", "ba16")


def params(vislam, shape):
    p = vislam.default_params()
    p.fy = p.fx
    if shape == "config3":
        p.nfeatures, p.nlevels, p.w_size, p.h_size = 4000, 4, 1920, 1080
        p.ransac_adaptive, p.ransac_max_iters, p.pose_input = 0, 2000, 1
    return p


def frames_on_device(torch, vislam, ctx, S):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, S["seed"])).cuda()
    n, chunk = S["B"] * R, min(S["B"], 256)
    fr = torch.empty((n, S["h"], S["w"]), dtype=torch.uint8, device="cuda")
    for t0 in range(0, n, chunk):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, S["seed"], t0, chunk, S["w"], S["h"], S["w"], fr.data_ptr() + t0 * S["w"] * S["h"], parallax=True)
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    cap = c.keypoint_capacity(S["w"], S["h"])
    mcap = int(np.floor(np.sqrt(p.n_cells))) ** 2 if p.pose_input == 0 else cap
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    mp, mfl, msm, link, traj, poses = z(B * mcap * 32), z(B * mcap), z(B * 16), z(B * 40), z(B * 128), z(B * 96)
    obs, frm = z(B * cap * vislam.FTRACK_OBS_DTYPE.itemsize), z(B * vislam.FTRACK_FRAME_DTYPE.itemsize)
    pts, fl, sm = z(B * cap * vislam.FTRACK_POINT_DTYPE.itemsize), z(B * cap), z(B * vislam.FTRACK_TRI_SUMMARY_DTYPE.itemsize)
    stride = int(variant[2:]) if variant != "chain" else 0
    bp = vislam.default_ba_params()
    nw = 0
    if stride:
        bp.stride = stride
        nw = vislam.ba_windows(B, stride)
        ba_poses, ba_win, ba_pts, ba_fl = z(B * 96), z(nw * 80), z(B * cap * 40), z(B * cap)
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        c.batch_triangulate(B, mcap, mp.data_ptr(), mfl.data_ptr(), msm.data_ptr())
        c.batch_scale_links(B, mp.data_ptr(), mfl.data_ptr(), mcap, link.data_ptr())
        c.batch_trajectory(B, link.data_ptr(), traj.data_ptr(), poses.data_ptr())
        c.batch_ftrack(B, cap, obs.data_ptr(), frm.data_ptr())
        src = poses
        if stride:
            c.batch_ba(B, obs.data_ptr(), cap, poses.data_ptr(), ba_poses.data_ptr(), ba_win.data_ptr(), ba_pts.data_ptr(), ba_fl.data_ptr(), bp)
            src = ba_poses
        c.batch_ftrack_triangulate(B, obs.data_ptr(), cap, src.data_ptr(), pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
    for i in range(warmup):
        step(i)
    c.batch_sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    c.batch_sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = c.batch_status() == 0
    s = sm.cpu().numpy().view(vislam.FTRACK_TRI_SUMMARY_DTYPE)
    extra = {"keypoint_capacity": cap, "track_ends_per_launch": int(s["n_ends"].sum()), "nview_points_per_launch": int(s["n_points"].sum()),
             "nview_kept_per_launch": int(s["n_kept"].sum())}
    if stride:
        w = ba_win.cpu().numpy().view(vislam.BA_WINDOW_DTYPE)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        extra.update({"windows": nw, "refined": int((w["flags"] & vislam.BA_REFINED != 0).sum()), "few": int((w["flags"] & vislam.BA_FEW != 0).sum()),
                      "restart": int((w["flags"] & vislam.BA_RESTART != 0).sum()), "points": int(w["n_points"].sum()), "observations": int(w["n_obs"].sum()),
                      "max_points_of_a_window": int(w["n_points"].max()), "accepted": int(w["n_accepted"].sum()), "rejected": int(w["n_rejected"].sum()),
                      "compute_units": cus, "compute_units_without_a_window": max(0, cus - nw)})
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def profile(a):
    out = tempfile.mkdtemp(prefix="ba_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ba", "--",
           sys.executable, os.path.abspath(__file__), "--only", "ba8", "--rounds", "1", "--steps", "3", "--warmup", "1", "--shape", a.shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no bundle-adjustment kernel rows in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--only", choices=VARIANTS, default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    vs = (a.only,) if a.only else VARIANTS
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_launch": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    summary = {}
    for v in vs:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "median_ms_per_launch": round(S["B"] / statistics.median(res[v]) * 1e3, 3),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
    if "chain" in vs:
        for v in vs:
            if v != "chain":
                summary[f"{v}_adds_ms_per_launch"] = round(summary[v]["median_ms_per_launch"] - summary["chain"]["median_ms_per_launch"], 3)
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
