#!/usr/bin/env python3
"""Probe: what the alignment with the accelerometer bias costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on
1024 S-752 frames per launch (752 x 480, no sync between launches) with vis_batch_imu_jac behind every launch and then the single alignment
vis_batch_vi_align ("via"), vis_batch_vi_align_ba in its place ("viab"), or the closed loop vis_batch_vi_align_ba -> vis_batch_imu_correct (dbg and dba
read from the record) -> vis_batch_vi_align_ba ("loop").  The alignment reads a chained trajectory made once on the host, as in
tools/vi_align_probe.py.  The variants alternate in ONE process, each on a context of its own, so that clocks and placement drift hit all alike;
the window is closed by vis_batch_sync and a device synchronise.

  python3 tools/vi_align_ba_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--out profiles/vi_align_ba_probe_mi355x.txt]

One JSON line per measurement and a summary line with medians, spread and the cost per launch (the step of a variant less that of "via"); every
line is also appended to --out."""
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
from vi_align_probe import trajectory  # noqa: E402

VARIANTS = ("via", "viab", "loop")


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
    delta, jac, delta2, status, state, result, result2 = z(B * 216), z(B * 296), z(B * 216), z(B * 4), z(B * 64), z(304), z(304)
    torch.cuda.synchronize()
    dba = result.data_ptr() + vislam.VI_ALIGN_BA_DBA_OFFSET

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        first = max(0, int(i * B / FPS * HZ) - 8)
        c.batch_imu_jac(B, d_s.data_ptr() + 56 * first, min(per_launch, len(samples) - first), d_t.data_ptr() + 8 * i * B, delta.data_ptr(), jac.data_ptr())
        if variant == "via":
            c.batch_vi_align(B, d_traj.data_ptr(), delta.data_ptr(), result.data_ptr(), state.data_ptr())
        else:
            c.batch_vi_align_ba(B, d_traj.data_ptr(), delta.data_ptr(), jac.data_ptr(), result.data_ptr(), state.data_ptr())
        if variant == "loop":
            c.batch_imu_correct(B, delta.data_ptr(), jac.data_ptr(), result.data_ptr(), delta2.data_ptr(), dba, 0, status.data_ptr())
            c.batch_vi_align_ba(B, d_traj.data_ptr(), delta2.data_ptr(), jac.data_ptr(), result2.data_ptr(), state.data_ptr())
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
    if variant != "via":
        r = result.cpu().numpy().view(vislam.VI_ALIGN_BA_DTYPE)[0]
        extra = {"ba_flags": int(r["ba_flags"]), "bias_triples": int(r["n_ba_triples"]), "flags": int(r["a"]["flags"])}
    if variant == "loop":
        extra["corrected"] = int((status.cpu().numpy().view(np.int32) == vislam.IMC_OK).sum())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vi_align_ba_probe_mi355x.txt"))
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
    summary["cost_ms_per_launch"] = {"viab_over_via": round(ms["viab"] - ms["via"], 3), "loop_over_via": round(ms["loop"] - ms["via"], 3)}
    emit(summary)


if __name__ == "__main__":
    main()
