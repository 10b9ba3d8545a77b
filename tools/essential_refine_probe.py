#!/usr/bin/env python3
"""Probe: what vis_batch_essential_refine costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752
frames per launch (752 x 480, no sync between launches) with and without the two-view refinement of every pair (5 Gauss-Newton steps over the
pose stage's inlier mask) queued behind it.  The two variants alternate in ONE process, each on a context of its own, so that clocks and
placement drift hit both alike; the window is closed by vis_batch_sync and a device synchronise.  The "plain" variant is the baseline: the
run without the call.

  python3 tools/essential_refine_probe.py [--rounds 5] [--steps 20] [--profile] [--shape headline|config3]

--shape config3: BASELINE config 3's pose stage (1920 x 1080, 4000 features on 4 levels, RANSAC on the symmetric matches with the adaptive
stop off, 64 frames per launch): thousands of correspondences per pair -- rows walked in many strides of 64.
--profile then runs a short leg with the call in a fresh child process under `rocprofv3 --kernel-trace --stats` (no counters in the same run)
and prints the stats row of k_essential_refine next to k_pose_final's from that same session.  One JSON line per measurement; the records of
the last launch are counted in the "refine" lines."""
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
KERNELS = ("k_essential_refine", "k_pose_final", "k_pose_svd")


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


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    c = vislam.Context(0, params(vislam, shape))
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    ep = vislam.default_eref_params()
    rec = torch.zeros(B * vislam.EREF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant == "refine":
            c.batch_essential_refine(B, rec.data_ptr(), ep)
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
    if variant == "refine":
        r = rec.cpu().numpy().view(vislam.EREF_RESULT_DTYPE)
        ran = (r["flags"] & (vislam.ER_REFINED | vislam.ER_REJECTED)) != 0
        extra = {"points_per_launch": int(r["n_points"].sum()), "used_per_launch": int(r["n_used"].sum()),
                 "refined": int((r["flags"] & vislam.ER_REFINED != 0).sum()), "rejected": int((r["flags"] & vislam.ER_REJECTED != 0).sum()),
                 "few": int((r["flags"] & vislam.ER_FEW != 0).sum()), "no_pose": int((r["flags"] & vislam.ER_NO_POSE != 0).sum()),
                 "median_cost_ratio": float(np.median(r["cost1"][ran] / np.maximum(r["cost0"][ran], 1e-300))) if ran.any() else None}
        if not ran.any():
            raise RuntimeError("no pair of the last launch was refined")
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def profile(a):
    out = tempfile.mkdtemp(prefix="eref_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "eref", "--",
           sys.executable, os.path.abspath(__file__), "--only", "refine", "--rounds", "1", "--steps", "5", "--warmup", "2", "--shape", a.shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    for line in r.stdout.splitlines():                                # the child's own lines: correspondences per launch
        if '"points_per_launch"' in line:
            print(line, flush=True)
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no refinement kernel rows in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)      # Calls, TotalDurationNs, AverageNs, ... as rocprofv3 writes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--only", choices=("plain", "refine"), default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    vs = (a.only,) if a.only else ("plain", "refine")
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
    if len(vs) == 2:
        summary["refine_vs_plain_median_pct"] = round(100.0 * (statistics.median(res["refine"]) / statistics.median(res["plain"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
