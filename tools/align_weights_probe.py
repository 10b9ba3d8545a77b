#!/usr/bin/env python3
"""Probe: what the Tukey / MAD weighting of the alignment (vis_set_align_weights) costs on the pipelined tracking path --
vis_batch_run(DETECT | MATCH | GRADIENT) + vis_batch_track on S-752 frames per launch, no sync between launches -- under each
weighting: identity, tukey (VIS_W_TUKEY) and tukey-signed (VIS_W_TUKEY_SIGNED).  The modes alternate in ONE process, each on a context
of its own, so that clocks and placement drift hit all alike; the window is closed by vis_batch_sync and a device synchronise.  The
weighted k_align warps every candidate twice per iteration (statistics pass, accumulation pass); the cost is reported against identity
in the same process.

  python3 tools/align_weights_probe.py [--rounds 3] [--steps 10] [--profile] [--shape headline|config3]

--shape config3: BASELINE config 3's frames (1920 x 1080, 4000 features on 4 levels, 64 frames per launch).
--profile then runs, per mode (or for the one of --only), a leg of 7 launches in a fresh child process under `rocprofv3 --kernel-trace
--stats` and prints best and average of k_align's launches from the kernel trace.  VISLAM_HIP_LIB=<another build> --only identity
measures a library without the entry point (the parent's).  One JSON line per measurement."""
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
R, DIM = 2, 4096
SHAPES = {"headline": dict(w=752, h=480, B=1024, seed=0xE0C00001), "config3": dict(w=1920, h=1080, B=64, seed=0xE0C00003)}
MODES = {"identity": 0, "tukey": 1, "tukey-signed": 2}


def params(vislam, shape):
    p = vislam.default_params()
    p.fy = p.fx
    if shape == "config3":
        p.nfeatures, p.nlevels, p.w_size, p.h_size = 4000, 4, 1920, 1080
    return p


def frames_on_device(torch, vislam, ctx, S):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, S["seed"])).cuda()
    n, chunk = S["B"] * R, min(S["B"], 256)
    fr = torch.empty((n, S["h"], S["w"]), dtype=torch.uint8, device="cuda")
    for t0 in range(0, n, chunk):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, S["seed"], t0, chunk, S["w"], S["h"], S["w"], fr.data_ptr() + t0 * S["w"] * S["h"])
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, S, shape, mode, steps, warmup):
    import ctypes as C
    c = vislam.Context(0, params(vislam, shape))
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    if hasattr(vislam.lib, "vis_set_align_weights"):                  # (an older A/B build: identity only)
        aw = vislam.default_align_weights()
        aw.mode = MODES[mode]
        c.set_align_weights(aw)
    elif mode != "identity":
        raise SystemExit("this library has no vis_set_align_weights")
    ap = vislam.default_align_params()
    al = torch.zeros(B * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
    tr = torch.zeros(B * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stages = vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT

    def step(i):
        d = fr.data_ptr() + (i % R) * B * S["w"] * S["h"]
        c.batch_run(d, B, stages)
        c.batch_track(ap, d, B, 0, al.data_ptr(), tr.data_ptr())
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
    raw = al.cpu().numpy().tobytes()
    sz = C.sizeof(vislam.AlignResult)
    iters = sum(sum(vislam.AlignResult.from_buffer_copy(raw, i * sz).iterations) for i in range(B))
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, iters


def profile(a):
    for mode in ((a.only,) if a.only else tuple(MODES)):
        out = tempfile.mkdtemp(prefix="align_weights_probe_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "aw", "--",
               sys.executable, os.path.abspath(__file__), "--only", mode, "--rounds", "1", "--steps", "7", "--warmup", "0", "--shape", a.shape]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
        ns = []
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                ns += [int(row["End_Timestamp"]) - int(row["Start_Timestamp"]) for row in csv.DictReader(fh) if "k_align" in row.get("Kernel_Name", "")]
        if not ns:
            raise SystemExit(f"no k_align rows in the kernel trace under {out}")
        print(json.dumps({"shape": a.shape, "mode": mode, "k_align_launches": len(ns), "best_ms": round(min(ns) / 1e6, 3),
                          "avg_ms": round(statistics.mean(ns) / 1e6, 3), "max_ms": round(max(ns) / 1e6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--only", choices=tuple(MODES), default=None, help="one mode (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    ms = (a.only,) if a.only else tuple(MODES)
    res = {m: [] for m in ms}
    for rnd in range(a.rounds):
        for m in ms:
            fps, iters = timed(torch, vislam, fr, S, a.shape, m, a.steps, a.warmup)
            res[m].append(fps)
            print(json.dumps({"round": rnd, "shape": a.shape, "mode": m, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3),
                              "iterations_last_launch": iters}), flush=True)
    summary = {}
    for m in ms:
        summary[m] = {"best": round(max(res[m])), "median": round(statistics.median(res[m])), "min": round(min(res[m])),
                      "spread_pct": round(100.0 * (max(res[m]) / min(res[m]) - 1.0), 2)}
    for m in ms:
        if m != "identity" and "identity" in res:
            summary[m + "_vs_identity_median_pct"] = round(100.0 * (statistics.median(res[m]) / statistics.median(res["identity"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
