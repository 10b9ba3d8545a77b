#!/usr/bin/env python3
"""Probe: what the visual-inertial alignment costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752
frames per launch (752 x 480, no sync between launches) with vis_batch_imu behind every launch ("imu": 200 Hz samples beside 20 frames a second)
and with vis_batch_vi_align behind that ("imu_via").  The alignment reads the launch's own deltas and a chained trajectory made once on the host
(a smooth motion, every frame an edge of one epoch, so that every frame is a pair and a triple: the most work a launch can hold).  The variants
alternate in ONE process, each on a context of its own, so that clocks and placement drift hit all alike; the window is closed by vis_batch_sync
and a device synchronise.  Measured as tools/imu_probe.py does.

  python3 tools/vi_align_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--out profiles/vi_align_probe_mi355x.txt]

--shape config3: BASELINE config 3 (1920 x 1080, 4000 features on 4 levels, 64 frames per launch, VIS_POSE_SYM).  One JSON line per measurement
and a summary line with medians, spread and the cost per launch (the step of "imu_via" less that of "imu"); every line is also appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from imu_probe import FPS, HZ, R, SHAPES, frames_on_device, imu_stream, params  # noqa: E402

VARIANTS = ("imu", "imu_via")
TRAJ_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("sigma", "<f8"), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("hops", "<i4"),
                       ("unit_edges", "<i4"), ("parent", "<i4"), ("flags", "<i4")])


def trajectory(B):
    """B chained records of a smooth motion: a rotation about z, sinusoidal centres, frame i an edge below frame i - 1 (frame 0 below the carried one)"""
    t = np.arange(B) / FPS
    a = 0.3 * np.sin(0.9 * t)
    rec = np.zeros(B, TRAJ_DTYPE)
    c, s = np.cos(a), np.sin(a)
    Rm = np.zeros((B, 3, 3))
    Rm[:, 0, 0], Rm[:, 0, 1], Rm[:, 1, 0], Rm[:, 1, 1], Rm[:, 2, 2] = c, -s, s, c, 1.0
    C = np.stack([1.5 * np.sin(1.1 * t), np.sin(0.7 * t + 0.5), 0.8 * np.sin(1.6 * t + 1.1)], 1)
    rec["R"], rec["t"], rec["sigma"] = Rm.reshape(B, 9), -np.einsum("nij,nj->ni", Rm, C), 1.0
    rec["epoch_seq"], rec["hops"], rec["unit_edges"], rec["parent"] = 1, np.arange(B) + 1, 1, np.arange(B) - 1
    return rec


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    samples, tframe = imu_stream(vislam, (steps + warmup) * B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
    d_s, d_t, d_traj = up(samples), up(tframe), up(trajectory(B))
    per_launch = int(B / FPS * HZ) + 16
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    delta, state, result = z(B * 216), z(B * 64), z(160)
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        first = max(0, int(i * B / FPS * HZ) - 8)
        c.batch_imu(B, d_s.data_ptr() + 56 * first, min(per_launch, len(samples) - first), d_t.data_ptr() + 8 * i * B, delta.data_ptr())
        if variant == "imu_via":
            c.batch_vi_align(B, d_traj.data_ptr(), delta.data_ptr(), result.data_ptr(), state.data_ptr())
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
    if variant == "imu_via":
        r = result.cpu().numpy().view(vislam.VI_ALIGN_DTYPE)[0]
        extra = {"pairs_of_the_last_launch": int(r["n_pairs_call"]), "triples_of_the_last_launch": int(r["n_triples_call"]), "flags": int(r["flags"])}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vi_align_probe_mi355x.txt"))
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
    summary["cost_ms_per_launch"] = {"vi_align": round(summary["imu_via"]["median_ms_per_step"] - summary["imu"]["median_ms_per_step"], 3)}
    emit(summary)


if __name__ == "__main__":
    main()
