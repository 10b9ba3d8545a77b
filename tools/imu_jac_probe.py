#!/usr/bin/env python3
"""Probe: what the bias Jacobians and the correction cost behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024
S-752 frames per launch (752 x 480, no sync between launches) with vis_batch_imu behind every launch ("imu"), with vis_batch_imu_jac in its place
("imu_jac"), with vis_batch_imu and vis_batch_vi_align ("imu_via", tools/vi_align_probe.py's), and with the closed loop vis_batch_imu_jac ->
vis_batch_vi_align -> vis_batch_imu_correct -> vis_batch_vi_align ("loop").  The alignment reads a chained trajectory made once on the host, as in
tools/vi_align_probe.py.  The variants alternate in ONE process, each on a context of its own, so that clocks and placement drift hit all alike;
the window is closed by vis_batch_sync and a device synchronise.

  python3 tools/imu_jac_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--out profiles/imu_jac_probe_mi355x.txt]

One JSON line per measurement and a summary line with medians, spread and the cost per launch (the step of a variant less that of the one it
extends); every line is also appended to --out."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from imu_probe import FPS, HZ, R, SHAPES, frames_on_device, imu_stream, params  # noqa: E402
from vi_align_probe import trajectory  # noqa: E402

VARIANTS = ("imu", "imu_jac", "imu_via", "loop")


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
    delta, jac, delta2, status, state, result, result2 = z(B * 216), z(B * 296), z(B * 216), z(B * 4), z(B * 64), z(160), z(160)
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        first = max(0, int(i * B / FPS * HZ) - 8)
        args = (B, d_s.data_ptr() + 56 * first, min(per_launch, len(samples) - first), d_t.data_ptr() + 8 * i * B, delta.data_ptr())
        if variant in ("imu", "imu_via"):
            c.batch_imu(*args)
        else:
            c.batch_imu_jac(*args, jac.data_ptr())
        if variant in ("imu_via", "loop"):
            c.batch_vi_align(B, d_traj.data_ptr(), delta.data_ptr(), result.data_ptr(), state.data_ptr())
        if variant == "loop":
            c.batch_imu_correct(B, delta.data_ptr(), jac.data_ptr(), result.data_ptr(), delta2.data_ptr(), 0, 0, status.data_ptr())
            c.batch_vi_align(B, d_traj.data_ptr(), delta2.data_ptr(), result2.data_ptr(), state.data_ptr())
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
    if variant in ("imu_jac", "loop"):
        j = jac.cpu().numpy().view(vislam.IMU_BIAS_JAC_DTYPE)
        extra = {"jac_flags_of_the_last_launch": sorted(set(int(f) for f in j["flags"])), "table_bytes": 496 * B * (int(math.log2(B)) + 1)}
    if variant == "loop":
        st = status.cpu().numpy().view(np.int32)
        r1, r2 = (x.cpu().numpy().view(vislam.VI_ALIGN_DTYPE)[0] for x in (result, result2))
        extra.update(corrected=int((st == vislam.IMC_OK).sum()), c0_call=[float(r1["c0_call"]), float(r2["c0_call"])])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_jac_probe_mi355x.txt"))
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
    summary["cost_ms_per_launch"] = {"jacobians": round(ms["imu_jac"] - ms["imu"], 3), "correct_and_align_again": round(ms["loop"] - ms["imu_via"] - (ms["imu_jac"] - ms["imu"]), 3),
                                     "loop_over_imu_via": round(ms["loop"] - ms["imu_via"], 3)}
    emit(summary)


if __name__ == "__main__":
    main()
