#!/usr/bin/env python3
"""Probe: what vis_batch_homography_polish costs inside the chain homography -> homography_pose behind every launch of the pipelined stream
path -- tools/essential_refine_probe.py's windows (vis_batch_run(VIS_STAGE_ALL) per launch, no sync between launches, closed by vis_batch_sync
and a device synchronise) with four variants that alternate in ONE process, each on a context of its own:

  plain     the run without a follow-up: the baseline
  hposes    vis_batch_homography with its mask, then vis_batch_homography_pose: what tools/run_directory.py --hposes queues
  polish0   the same chain with vis_batch_homography_polish between the two calls, rounds = 0 (one round over the RANSAC's inliers)
  polish    the same with the defaults (three re-selections at the RANSAC's threshold, five steps a round), h_out written

  python3 tools/homography_polish_probe.py [--rounds 5] [--steps 20] [--shape headline|config3] [--variants plain,hposes,polish0,polish]

--shape config3: BASELINE config 3's pose stage (1920 x 1080, 4000 features on 4 levels, RANSAC on the symmetric matches with the adaptive stop
off, 64 frames per launch): thousands of correspondences per pair, the four-wave form of the kernel.  One JSON line per measurement -- the records
of the last launch are counted in the polish lines -- and one summary line with every variant's median against `plain` and `hposes`."""
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
VARIANTS = ("plain", "hposes", "polish0", "polish")


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    mcap = c.keypoint_capacity(S["w"], S["h"]) if p.pose_input == 1 else int(np.floor(np.sqrt(p.n_cells))) ** 2
    hp, hq, hl = vislam.default_homography_params(), vislam.default_hpose_params(), vislam.default_hpolish_params()
    if variant == "polish0":
        hl.rounds = 0
    draws = torch.from_numpy(np.random.default_rng(7).integers(0, 2 ** 31, (hp.iters, 4)).astype(np.int32)).cuda()
    hrec, hrec2 = (torch.zeros(B * vislam.HOMOGRAPHY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
    mask, mask2 = (torch.zeros(B * mcap, dtype=torch.uint8, device="cuda") for _ in range(2))
    rec = torch.zeros(B * vislam.HPOLISH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    pose = torch.zeros(B * vislam.HPOSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant == "plain":
            return
        c.batch_homography(B, draws.data_ptr(), mcap, mask.data_ptr(), hrec.data_ptr(), hp)
        if variant == "hposes":
            c.batch_homography_pose(B, hrec.data_ptr(), mcap, mask.data_ptr(), 0, pose.data_ptr(), hq)
        else:
            c.batch_homography_polish(B, hrec.data_ptr(), mcap, mask.data_ptr(), mcap, mask2.data_ptr(), rec.data_ptr(), hrec2.data_ptr(), hl)
            c.batch_homography_pose(B, hrec2.data_ptr(), mcap, mask2.data_ptr(), 0, pose.data_ptr(), hq)
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
        r = rec.cpu().numpy().view(vislam.HPOLISH_RESULT_DTYPE)
        ran = (r["flags"] & (vislam.HPOL_POLISHED | vislam.HPOL_REJECTED)) != 0
        if not ran.any():
            raise RuntimeError("no pair of the last launch was polished")
        extra = {"mask_cap": mcap, "points_per_launch": int(r["n_points"].sum()), "set_first_per_launch": int(r["n_set_first"].sum()),
                 "set_last_per_launch": int(r["n_set_last"].sum()), "rounds_run_mean": round(float(r["rounds_run"][ran].mean()), 2),
                 "steps_run_mean": round(float(r["steps_run"][ran].mean()), 2), "polished": int((r["flags"] & vislam.HPOL_POLISHED != 0).sum()),
                 "rejected": int((r["flags"] & vislam.HPOL_REJECTED != 0).sum()), "few": int((r["flags"] & vislam.HPOL_FEW != 0).sum()),
                 "shrank": int((r["flags"] & vislam.HPOL_SHRANK != 0).sum()), "no_model": int((r["flags"] & vislam.HPOL_NO_MODEL != 0).sum())}
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
    for ref in ("plain", "hposes"):
        if ref in vs:
            base = summary[ref]
            for v in vs[vs.index(ref) + 1:] if ref == "hposes" else vs:
                if v != ref:
                    summary[v][f"vs_{ref}_pct"] = round(100.0 * (summary[v]["median_fps"] / base["median_fps"] - 1.0), 2)
                    summary[v][f"ms_per_step_over_{ref}"] = round(summary[v]["median_ms_per_step"] - base["median_ms_per_step"], 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
