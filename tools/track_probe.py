#!/usr/bin/env python3
"""Probe: what batched camera tracking (vis_batch_track) costs against vis_batch_align in the GPU main's pipelined sequence --
bench.py's gpu_main_sequence step (S-752, 752 x 480, 1024 frames per launch, VIS_STAGE_DETECT | MATCH | GRADIENT, then the pose-stream
call, no sync between steps) with batch_align and with batch_track.  The two variants alternate in ONE process, each on a context of
its own, so that clocks and placement drift hit both alike.  batch_track does batch_align's work plus pair 0 of every launch (against
the keyframe snapshot), k_track_snapshot (one frame of images, ~2.4 MB) and k_track_chain (one workgroup, 1024 dependent SE3 products).

  python3 tools/track_probe.py [--rounds 3] [--steps 20] [--profile]

--profile then runs a short batch_track leg in a fresh child process under `rocprofv3 --kernel-trace --stats` and prints the stats
rows of k_track_chain, k_track_snapshot and k_align.  One JSON line per measurement."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
W, H, B, R, SEED, DIM = 752, 480, 1024, 2, 0xE0C00001, 4096
KERNELS = ("k_track_chain", "k_track_snapshot", "k_align")


def frames_on_device(torch, vislam, ctx):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, SEED)).cuda()
    fr = torch.empty((B * R, H, W), dtype=torch.uint8, device="cuda")
    for t0 in range(0, B * R, 256):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, SEED, t0, 256, W, H, W, fr.data_ptr() + t0 * W * H)
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, variant, steps, warmup):
    import ctypes as C
    p = vislam.default_params()
    p.fy = p.fx
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    ap = vislam.default_align_params()
    outa = torch.empty(B * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
    outt = torch.empty(B * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stages = vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT

    def step(i):
        d = fr.data_ptr() + (i % R) * B * W * H
        c.batch_run(d, B, stages)
        if variant == "track":
            c.batch_track(ap, d, B, 0, outa.data_ptr(), outt.data_ptr())
        else:
            c.batch_align(ap, d, B, 0, 0, 0, 0, outa.data_ptr())
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
    return steps * B / dt


def profile(args):
    out = tempfile.mkdtemp(prefix="track_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "tp", "--",
           sys.executable, os.path.abspath(__file__), "--only", "track", "--rounds", "1", "--steps", "5", "--warmup", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no tracking kernel rows in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)      # Calls, TotalDurationNs, AverageNs, ... as rocprofv3 writes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("align", "track"), default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c)
    c.close()
    vs = (a.only,) if a.only else ("align", "track")
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps = timed(torch, vislam, fr, v, a.steps, a.warmup)
            res[v].append(fps)
            print(json.dumps({"round": rnd, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(B / fps * 1e3, 3)}), flush=True)
    summary = {}
    for v in vs:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
    if len(vs) == 2:
        summary["track_vs_align_pct"] = round(100.0 * (max(res["track"]) / max(res["align"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
