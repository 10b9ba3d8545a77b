#!/usr/bin/env python3
"""Probe: what the feature tracks cost behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752 frames
per launch (752 x 480, no sync between launches) without the calls ("plain": the baseline, the pipeline as it was), with vis_batch_ftrack
on the symmetric matches ("link") and with vis_batch_ftrack_triangulate behind it as well ("both"; poses of a camera stepping along x, made
on the host once -- the call only needs SOME finite poses).  The variants alternate in ONE process, each on a context of its own, so that
clocks and placement drift hit all alike; the window is closed by vis_batch_sync and a device synchronise.

  python3 tools/ftrack_probe.py [--rounds 5] [--steps 20] [--profile] [--shape headline|config3]

--shape config3: BASELINE config 3 (1920 x 1080, 4000 features on 4 levels, 64 frames per launch).
--profile then runs a short "both" leg in a fresh child process under `rocprofv3 --kernel-trace --stats` (no counters in the same run) and
prints the stats rows of the k_ft_* / k_ftri_* kernels.  One JSON line per measurement; the "link" lines carry what the last launch linked
and the streaming floor of the link step: the bytes its kernels move per launch / 8 TB/s."""
import argparse
import csv
import glob
import json
import math
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
KERNELS = ("k_ft_claim", "k_ft_parent", "k_ft_round", "k_ft_finish", "k_ft_carry", "k_ftri_clear", "k_ftri_mark", "k_ftri_points")
HBM_BYTES_PER_S = 8e12


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
        ctx.synth_frames_device(canvas.data_ptr(), DIM, S["seed"], t0, chunk, S["w"], S["h"], S["w"], fr.data_ptr() + t0 * S["w"] * S["h"])
    torch.cuda.synchronize()
    return fr


def link_bytes(B, cap, n_links):
    """bytes the link step's kernels move per launch: the clear of the two claim tables (8 per keypoint), the lists (16 per entry, read by the
    claim pass; the winners' entries again by the parent pass) and two 4-byte atomics per entry, the parent pass (4 + 4 read, 8 + 4 written),
    ceil(log2 B) rounds of 8 read + 8 gathered + 8 written, the last pass (8 + 4 read, 16 written)"""
    rounds = max(0, math.ceil(math.log2(B))) if B > 1 else 0
    return B * cap * (8 + 20 + 24 * rounds + 28) + n_links * (16 + 8 + 16)


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    cap = c.keypoint_capacity(S["w"], S["h"])
    obs = torch.zeros(B * cap * vislam.FTRACK_OBS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    frm = torch.zeros(B * vislam.FTRACK_FRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    pts = torch.zeros(B * cap * vislam.FTRACK_POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(B * cap, dtype=torch.uint8, device="cuda")
    sm = torch.zeros(B * vislam.FTRACK_TRI_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    poses = np.zeros((B, 12))
    poses[:, 0] = poses[:, 4] = poses[:, 8] = 1.0
    poses[:, 9] = -0.05 * np.arange(B)
    d_poses = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant in ("link", "both"):
            c.batch_ftrack(B, cap, obs.data_ptr(), frm.data_ptr())
        if variant == "both":
            c.batch_ftrack_triangulate(B, obs.data_ptr(), cap, d_poses.data_ptr(), pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
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
    extra = {}
    if variant in ("link", "both"):
        f = frm.cpu().numpy().view(vislam.FTRACK_FRAME_DTYPE)
        n_links = int(f["n_continued"].sum())
        nbytes = link_bytes(B, cap, n_links)
        extra = {"keypoint_capacity": cap, "keypoints_per_launch": int(f["n_keypoints"].sum()), "continued_per_launch": n_links,
                 "max_len": int(f["max_len"].max()), "no_carry_frames": int((f["flags"] & vislam.FT_NO_CARRY != 0).sum()),
                 "link_bytes_per_launch": nbytes, "link_streaming_floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 1)}
        if n_links == 0:
            raise RuntimeError("the last launch linked nothing")
    if variant == "both":
        s = sm.cpu().numpy().view(vislam.FTRACK_TRI_SUMMARY_DTYPE)
        extra.update({"track_ends_per_launch": int(s["n_ends"].sum()), "points_per_launch": int(s["n_points"].sum()), "kept_per_launch": int(s["n_kept"].sum())})
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def profile(a):
    out = tempfile.mkdtemp(prefix="ftrack_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ftrack", "--",
           sys.executable, os.path.abspath(__file__), "--only", "both", "--rounds", "1", "--steps", "5", "--warmup", "2", "--shape", a.shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    for line in r.stdout.splitlines():                                # the child's own lines: what a launch linked
        if '"continued_per_launch"' in line:
            print(line, flush=True)
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no feature-track kernel rows in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)      # Calls, TotalDurationNs, AverageNs, ... as rocprofv3 writes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--only", choices=("plain", "link", "both"), default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    vs = (a.only,) if a.only else ("plain", "link", "both")
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    summary = {}
    for v in vs:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
    if len(vs) == 3:
        for v in ("link", "both"):
            summary[f"{v}_vs_plain_median_pct"] = round(100.0 * (statistics.median(res[v]) / statistics.median(res["plain"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
