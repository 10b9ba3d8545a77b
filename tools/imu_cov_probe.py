#!/usr/bin/env python3
"""Probe: what the covariance of the deltas costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752
frames per launch (752 x 480, no sync between launches) with vis_batch_imu behind every launch ("imu"), with vis_batch_imu_cov in its place
("imu_cov"), and with both vis_batch_imu_jac and vis_batch_imu_cov ("imu_jac_cov", what a caller who wants the Jacobians and the covariance queues), with vis_batch_imu and vis_batch_vi_align ("imu_via",
tools/vi_align_probe.py's) and with the chain vis_batch_imu_cov -> vis_batch_vi_align -> vis_batch_imu_factor ("cov_via_factor").  The alignment reads
a chained trajectory made once on the host, as in tools/vi_align_probe.py.
The variants alternate in ONE process, each on a context of its own, so that clocks and placement drift hit all alike; the window is closed by
vis_batch_sync and a device synchronise.

  python3 tools/imu_cov_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--out profiles/imu_cov_probe_mi355x.txt]

One JSON line per measurement and a summary line with medians, spread and the cost per launch (the step of a variant less that of "imu"); every
line is also appended to --out."""
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

VARIANTS = ("imu", "imu_cov", "imu_jac_cov", "imu_via", "cov_via_factor")


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
    delta, delta2, jac, cov, state, result, factor = z(B * 216), z(B * 216), z(B * 296), z(B * 368), z(B * 64), z(160), z(B * 96)
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        first = max(0, int(i * B / FPS * HZ) - 8)
        args = (B, d_s.data_ptr() + 56 * first, min(per_launch, len(samples) - first), d_t.data_ptr() + 8 * i * B)
        if variant in ("imu", "imu_via"):
            c.batch_imu(*args, delta.data_ptr())
        else:
            c.batch_imu_cov(*args, delta.data_ptr(), cov.data_ptr())
        if variant == "imu_jac_cov":
            c.batch_imu_jac(*args, delta2.data_ptr(), jac.data_ptr())
        if variant in ("imu_via", "cov_via_factor"):
            c.batch_vi_align(B, d_traj.data_ptr(), delta.data_ptr(), result.data_ptr(), state.data_ptr())
        if variant == "cov_via_factor":
            c.batch_imu_factor(B, d_traj.data_ptr(), delta.data_ptr(), cov.data_ptr(), state.data_ptr(), result.data_ptr(), factor.data_ptr())
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
    if variant in ("imu_cov", "imu_jac_cov", "cov_via_factor"):
        q = cov.cpu().numpy().view(vislam.IMU_COV_DTYPE)
        d = delta.cpu().numpy().view(vislam.IMU_DELTA_DTYPE)
        paired = (d["flags"] & (vislam.IMU_NO_PAIR | vislam.IMU_NO_CARRY | vislam.IMU_NO_START | vislam.IMU_NONFINITE)) == 0
        sd = np.sqrt(q["S"][paired][:, [0, 24, 39]].mean(axis=0)) if paired.any() else np.zeros(3)      # entries (0, 0), (3, 3), (6, 6)
        extra = {"cov_flags_of_the_last_launch": sorted(set(int(f) for f in q["flags"])), "table_bytes": 568 * B * (int(math.log2(B)) + 1),
                 "pairs_of_the_last_launch": int(paired.sum()), "rms_sd_phi_x_v_x_p_x": [float(x) for x in sd]}
    if variant == "imu_jac_cov":
        extra["deltas_equal"] = bool((delta.cpu() == delta2.cpu()).all())
    if variant == "cov_via_factor":
        f = factor.cpu().numpy().view(vislam.IMU_FACTOR_DTYPE)
        extra["factor_flags_of_the_last_launch"] = {str(k): int((f["flags"] == k).sum()) for k in sorted(set(int(x) for x in f["flags"]))}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_cov_probe_mi355x.txt"))
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
    summary["cost_ms_per_launch"] = {"covariance_in_the_place_of_imu": round(ms["imu_cov"] - ms["imu"], 3),
                                     "jacobians_and_covariance_over_imu": round(ms["imu_jac_cov"] - ms["imu"], 3),
                                     "covariance_and_factor_over_imu_via": round(ms["cov_via_factor"] - ms["imu_via"], 3)}
    emit(summary)


if __name__ == "__main__":
    main()
