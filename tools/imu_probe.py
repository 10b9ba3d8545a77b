#!/usr/bin/env python3
"""Probe: what the IMU preintegration costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752 frames
per launch (752 x 480, no sync between launches) without follow-ups ("plain"), with vis_batch_imu behind every launch ("imu": 200 Hz samples beside
20 frames a second, the launch's sample window of a stream-long array), and with vis_batch_imu and vis_batch_f2f reading its rotations ("imu_f2f")
against vis_batch_f2f on rotations that were there already ("f2f").  The variants alternate in ONE process, each on a context of its own, so that
clocks and placement drift hit all alike; the window is closed by vis_batch_sync and a device synchronise.  Measured as DESIGN.md 4.19 does.

  python3 tools/imu_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--out profiles/imu_probe_mi355x.txt]

--shape config3: BASELINE config 3 (1920 x 1080, 4000 features on 4 levels, 64 frames per launch, VIS_POSE_SYM).  One JSON line per measurement
and a summary line with medians, spread and the cost per launch (the step of a variant less that of the one it extends); every line is also
appended to --out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
R, DIM = 2, 4096
SHAPES = {"headline": dict(w=752, h=480, B=1024, seed=0xE0C00001), "config3": dict(w=1920, h=1080, B=64, seed=0xE0C00003)}
VARIANTS = ("plain", "imu", "f2f", "imu_f2f")
FPS, HZ = 20.0, 200.0


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


def imu_stream(vislam, n_frames):
    """a smooth body rate at HZ over n_frames frame times at FPS that fall between samples"""
    m = int(n_frames / FPS * HZ) + 8
    s = np.zeros(m, vislam.IMU_SAMPLE_DTYPE)
    t = 100.0 + np.arange(m) / HZ
    s["t"] = t
    s["w"] = np.stack([0.6 * np.sin(1.3 * t) + 0.2, 0.5 * np.cos(0.9 * t + 0.4), 0.4 * np.sin(2.1 * t + 1.0) - 0.1], 1)
    s["a"] = np.stack([0.8 * np.cos(1.7 * t), 9.81 + 0.5 * np.sin(0.7 * t), 0.3 * np.sin(1.1 * t + 0.3)], 1)
    return s, 100.0 + 0.0037 + (np.arange(n_frames) + 1) / FPS


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    total = (steps + warmup) * B
    samples, tframe = imu_stream(vislam, total)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
    d_s, d_t = up(samples), up(tframe)
    per_launch = int(B / FPS * HZ) + 16                              # the launch's window of the stream's samples; consecutive windows overlap
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    delta, rot, rec = z(B * 216), z(B * 36), z(B * 32)
    eye = up(np.tile(np.eye(3, dtype=np.float32).reshape(9), (B, 1)))
    draws = up(np.random.default_rng(1).integers(0, 2 ** 31, (p.f2f_iters, 2)).astype(np.int32))
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant in ("imu", "imu_f2f"):
            first = max(0, int(i * B / FPS * HZ) - 8)
            c.batch_imu(B, d_s.data_ptr() + 56 * first, min(per_launch, len(samples) - first), d_t.data_ptr() + 8 * i * B, delta.data_ptr(), rot.data_ptr())
        if variant in ("f2f", "imu_f2f"):
            c.batch_f2f(B, (rot if variant == "imu_f2f" else eye).data_ptr(), 0, draws.data_ptr(), rec.data_ptr())
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
    if variant in ("imu", "imu_f2f"):
        d = delta.cpu().numpy().view(vislam.IMU_DELTA_DTYPE)
        extra = {"samples_per_launch": per_launch, "flags_of_the_last_launch": sorted(set(int(f) for f in d["flags"])), "median_n_steps": int(np.median(d["n_steps"])),
                 "table_bytes": 208 * B * (int(math.log2(B)) + 1)}
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_probe_mi355x.txt"))
    a = ap.parse_args()
    import torch
    import vislam
    log = open(a.out, "a")

    def emit(line):
        print(json.dumps(line), flush=True)
        log.write(json.dumps(line) + "\n")
        log.flush()
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    res = {v: [] for v in VARIANTS}
    for rnd in range(a.rounds):
        for v in VARIANTS:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            emit(line)
    summary = {"shape": a.shape}
    for v in VARIANTS:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2), "median_ms_per_step": round(S["B"] / statistics.median(res[v]) * 1e3, 3)}
    ms = {v: summary[v]["median_ms_per_step"] for v in VARIANTS}
    summary["cost_ms_per_launch"] = {"imu": round(ms["imu"] - ms["plain"], 3), "imu_ahead_of_f2f": round(ms["imu_f2f"] - ms["f2f"], 3)}
    emit(summary)


if __name__ == "__main__":
    main()
