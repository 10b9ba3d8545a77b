#!/usr/bin/env python3
"""Probe: what rectification on the device (vis_rectify_batch, k_remap) costs.

  1. The kernel alone: n = 1024 S-752 frames (752 x 480) through the EuRoC tables into 736 x 480, best of --reps calls (each call timed
     from the host to the end of a device-wide synchronisation).  Algorithmic bytes per frame = in_w in_h + out_w out_h (each source byte
     read once, each output byte written once; the tables not counted): GB/s and the fraction of 8 TB/s.
  2. The pipelined step, vis_batch_run(ALL) on 1024 frames of 736 x 480 per launch, no sync between steps: "plain" runs it on frames that
     are already 736 x 480; "rectify" puts vis_rectify_batch (752 x 480 -> 736 x 480, two output buffers used in turn) in front of it.
     The two alternate in ONE process (--rounds), each on a context of its own, so that clocks and placement drift hit both alike.

  python3 tools/rectify_probe.py [--rounds 3] [--steps 20] [--reps 20] [--profile]

--profile runs a short rectify leg in a fresh child process under `rocprofv3 --kernel-trace --stats` and prints the stats row of k_remap.
One JSON line per measurement."""
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
W, H, OW, B, R, SEED, DIM = 752, 480, 736, 1024, 2, 0xE0C00001, 4096
EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
HBM_TBS = 8.0


def frames_on_device(torch, vislam, ctx, w, h):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, SEED)).cuda()
    fr = torch.empty((B * R, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for t0 in range(0, B * R, 256):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, SEED, t0, 256, w, h, w, fr.data_ptr() + t0 * w * h)
    torch.cuda.synchronize()
    return fr


def kernel_alone(torch, vislam, raw, reps):
    c = vislam.Context(0)
    Kn = vislam.optimal_new_camera_matrix(EUROC_K, EUROC_D, (W, H), (OW, H))
    r = c.rectify(EUROC_K, EUROC_D, Kn, (W, H), (OW, H))
    out = torch.empty(B * H * OW, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    best = float("inf")
    for i in range(reps + 2):
        t0 = time.perf_counter()
        r.batch(raw.data_ptr(), W, B, out.data_ptr(), OW)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= 2:
            best = min(best, dt)
    r.close(); c.close()
    nbytes = B * (W * H + OW * H)
    gbs = nbytes / best / 1e9
    print(json.dumps({"measure": "k_remap_alone", "frames": B, "in": [W, H], "out": [OW, H], "best_us": round(best * 1e6, 1),
                      "algorithmic_GB": round(nbytes / 1e9, 3), "GB_per_s": round(gbs, 1), "fraction_of_8TBps": round(gbs / (HBM_TBS * 1e3), 3)}),
          flush=True)


def timed(torch, vislam, plain, raw, variant, steps, warmup):
    p = vislam.default_params()
    p.w_size, p.h_size = OW, H
    c = vislam.Context(0, p)
    c.batch_plan(OW, H, OW, B)
    r, outs = None, None
    if variant == "rectify":
        Kn = vislam.optimal_new_camera_matrix(EUROC_K, EUROC_D, (W, H), (OW, H))
        r = c.rectify(EUROC_K, EUROC_D, Kn, (W, H), (OW, H))
        outs = [torch.empty(B * H * OW, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()

    def step(i):
        if variant == "rectify":
            d = outs[i & 1].data_ptr()
            r.batch(raw.data_ptr() + (i % R) * B * W * H, W, B, d, OW)
        else:
            d = plain.data_ptr() + (i % R) * B * OW * H
        c.batch_run(d, B, vislam.STAGE_ALL)
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
    if r is not None:
        r.close()
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt


def profile(args):
    out = tempfile.mkdtemp(prefix="rectify_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rp", "--",
           sys.executable, os.path.abspath(__file__), "--only", "rectify", "--rounds", "1", "--steps", "5", "--warmup", "2", "--reps", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if "k_remap" in row.get("Name", "")]
    if not rows:
        raise SystemExit(f"no k_remap rows in the stats under {out}")
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls of the kernel-alone measurement (best of)")
    ap.add_argument("--only", choices=("plain", "rectify"), default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    c = vislam.Context(0)
    raw = frames_on_device(torch, vislam, c, W, H)
    plain = frames_on_device(torch, vislam, c, OW, H) if a.only != "rectify" else None
    c.close()
    kernel_alone(torch, vislam, raw, a.reps)
    vs = (a.only,) if a.only else ("plain", "rectify")
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps = timed(torch, vislam, plain, raw, v, a.steps, a.warmup)
            res[v].append(fps)
            print(json.dumps({"round": rnd, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(B / fps * 1e3, 3)}), flush=True)
    summary = {}
    for v in vs:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
    if len(vs) == 2:
        summary["rectify_vs_plain_pct"] = round(100.0 * (max(res["rectify"]) / max(res["plain"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)
    del raw, plain
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
