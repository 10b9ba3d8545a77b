#!/usr/bin/env python3
"""Probe: what vis_batch_essential_polish costs behind every launch of the pipelined stream path, next to vis_batch_essential_refine and to the run
without either -- tools/essential_refine_probe.py's windows (vis_batch_run(VIS_STAGE_ALL) per launch, no sync between launches, closed by
vis_batch_sync and a device synchronise) with four variants that alternate in ONE process, each on a context of its own:

  plain     the run without a follow-up: the baseline
  refine    vis_batch_essential_refine (one wave a pair, the set fixed)
  polish0   vis_batch_essential_polish with rounds = 0: the same arithmetic as `refine` on the headline shape (49 correspondences a pair, one wave),
            and on config3's long rows the four-wave form of it
  polish    vis_batch_essential_polish with the defaults (three re-selections at 2 px, five steps a round), pose_out written

  python3 tools/essential_polish_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--variants plain,refine,polish0,polish]

--shape config3: BASELINE config 3's pose stage (1920 x 1080, 4000 features on 4 levels, RANSAC on the symmetric matches with the adaptive stop
off, 64 frames per launch): thousands of correspondences per pair.  One JSON line per measurement -- the records of the last launch are counted in
the polish lines -- and one summary line with every variant's median against `plain`."""
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
from essential_refine_probe import SHAPES, frames_on_device, params  # noqa: E402
R = 2
VARIANTS = ("plain", "refine", "polish0", "polish")


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    mcap = c.keypoint_capacity(S["w"], S["h"]) if p.pose_input == 1 else int(np.floor(np.sqrt(p.n_cells))) ** 2
    er, ep = vislam.default_eref_params(), vislam.default_epolish_params()
    if variant == "polish0":
        ep.rounds = 0
    rec = torch.zeros(B * max(vislam.EREF_RESULT_DTYPE.itemsize, vislam.EPOLISH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    mask = torch.zeros(B * mcap, dtype=torch.uint8, device="cuda")
    pose = torch.zeros(B * vislam.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant == "refine":
            c.batch_essential_refine(B, rec.data_ptr(), er)
        elif variant != "plain":
            c.batch_essential_polish(B, mcap, mask.data_ptr(), rec.data_ptr(), pose.data_ptr(), ep)
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
    if variant.startswith("polish"):
        r = rec.cpu().numpy()[:B * vislam.EPOLISH_RESULT_DTYPE.itemsize].view(vislam.EPOLISH_RESULT_DTYPE)
        ran = (r["flags"] & (vislam.EP_POLISHED | vislam.EP_REJECTED)) != 0
        if not ran.any():
            raise RuntimeError("no pair of the last launch was polished")
        extra = {"mask_cap": mcap, "points_per_launch": int(r["n_points"].sum()), "set_first_per_launch": int(r["n_set_first"].sum()),
                 "set_last_per_launch": int(r["n_set_last"].sum()), "rounds_run_mean": round(float(r["rounds_run"][ran].mean()), 2),
                 "steps_run_mean": round(float(r["steps_run"][ran].mean()), 2), "polished": int((r["flags"] & vislam.EP_POLISHED != 0).sum()),
                 "rejected": int((r["flags"] & vislam.EP_REJECTED != 0).sum()), "few": int((r["flags"] & vislam.EP_FEW != 0).sum()),
                 "shrank": int((r["flags"] & vislam.EP_SHRANK != 0).sum()), "no_pose": int((r["flags"] & vislam.EP_NO_POSE != 0).sum())}
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
    ap.add_argument("--variants", default=",".join(VARIANTS))
    a = ap.parse_args()
    vs = tuple(a.variants.split(","))
    if not vs or any(v not in VARIANTS for v in vs):
        raise SystemExit(f"--variants: a comma-separated choice of {VARIANTS}")
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    summary = {"shape": a.shape}
    for v in vs:
        ms = [S["B"] / f * 1e3 for f in res[v]]
        summary[v] = {"median_fps": round(statistics.median(res[v])), "min_fps": round(min(res[v])), "max_fps": round(max(res[v])),
                      "median_ms_per_step": round(statistics.median(ms), 3), "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
    if "plain" in vs:
        base = summary["plain"]
        for v in vs:
            if v != "plain":
                summary[v]["vs_plain_pct"] = round(100.0 * (summary[v]["median_fps"] / base["median_fps"] - 1.0), 2)
                summary[v]["ms_per_step_over_plain"] = round(summary[v]["median_ms_per_step"] - base["median_ms_per_step"], 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
