#!/usr/bin/env python3
"""Probe: what the keyframe gate (vis_params.keyframe_min_points) costs on the headline workload -- S-752, 1024 frames per launch,
VIS_STAGE_FRAME, 20 launches per step over two steps' worth of resident frames, like bench.py.  K = 0 (off) and K = 1 (the GPU main's
rule) alternate in ONE process, each on a context of its own, so that clocks and placement drift hit both alike.  Every S-752 frame
passes the gate, so K = 1 does the same work as K = 0 plus k_keyframe_links (one workgroup per launch) and the carried record it copies.

  python3 tools/keyframe_gate_probe.py [--rounds 3] [--steps 10] [--profile]

--profile then runs a short K = 1 leg in a fresh child process under `rocprofv3 --kernel-trace --stats` and prints the stats row of
k_keyframe_links (calls, total / average / min / max ns, share of kernel time).  One JSON line per measurement."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
W, H, B, Q, R, SEED, DIM = 752, 480, 1024, 20, 2, 0xE0C00001, 4096


def frames_on_device(torch, vislam, ctx):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, SEED)).cuda()
    fr = torch.empty((B * Q * R, H, W), dtype=torch.uint8, device="cuda")
    for t0 in range(0, B * Q * R, 256):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, SEED, t0, 256, W, H, W, fr.data_ptr() + t0 * W * H)
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, K, steps, warmup):
    p = vislam.default_params()
    p.fy = p.fx
    p.keyframe_min_points = K
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)

    def step(i):
        for s in range(Q):
            c.batch_run(fr.data_ptr() + (((i % R) * Q + s) * B) * W * H, B, vislam.STAGE_FRAME)
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
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * Q * B / dt, dt / (steps * Q)


def profile(args):
    out = tempfile.mkdtemp(prefix="kf_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kf", "--",
           sys.executable, os.path.abspath(__file__), "--only", "1", "--rounds", "1", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if "k_keyframe_links" in row.get("Name", "")]
    if not rows:
        raise SystemExit(f"no k_keyframe_links row in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": "k_keyframe_links", "stats": row}), flush=True)      # Calls, TotalDurationNs, AverageNs, ... as rocprofv3 writes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="one value of K (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c)
    c.close()
    ks = (a.only,) if a.only is not None else (0, 1)
    res = {k: [] for k in ks}
    for rnd in range(a.rounds):
        for k in ks:
            fps, launch_s = timed(torch, vislam, fr, k, a.steps, a.warmup)
            res[k].append(fps)
            print(json.dumps({"round": rnd, "K": k, "frames_per_s": round(fps), "us_per_launch": round(launch_s * 1e6, 1)}), flush=True)
    if len(ks) == 2:
        m0, m1 = max(res[0]), max(res[1])
        print(json.dumps({"best_K0": round(m0), "best_K1": round(m1), "K1_vs_K0_pct": round(100.0 * (m1 / m0 - 1.0), 2),
                          "us_per_launch_K0": round(B / m0 * 1e6, 1), "us_per_launch_K1": round(B / m1 * 1e6, 1)}), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
