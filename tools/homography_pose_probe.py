#!/usr/bin/env python3
"""Probe: what vis_batch_homography_pose costs behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL) +
vis_batch_homography (with its mask) per launch, with and without the pose of every pair's homography queued behind it (no rotation hint).
The protocol is tools/homography_probe.py's: the two variants alternate in ONE process, each on a context of its own, no sync between
launches, the window closed by vis_batch_sync and a device synchronise.  The "homography" variant is the baseline.

  python3 tools/homography_pose_probe.py [--rounds 5] [--steps 20] [--shape headline|config3]

One JSON line per measurement; the kinds and flags of the last launch are counted in the "hpose" lines."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_probe as base                                       # shapes, parameters, frames, row capacity


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = base.params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    cap = base.row_capacity(vislam, c, p, S)
    hp, hq = vislam.default_homography_params(), vislam.default_hpose_params()
    draws = torch.from_numpy(np.random.default_rng(7).integers(0, 2 ** 31, (hp.iters, 4)).astype(np.int32)).cuda()
    rec = torch.zeros(B * vislam.HOMOGRAPHY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(B * cap, dtype=torch.uint8, device="cuda")
    out = torch.zeros(B * vislam.HPOSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % base.R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        c.batch_homography(B, draws.data_ptr(), cap, mask.data_ptr(), rec.data_ptr(), hp)
        if variant == "hpose":
            c.batch_homography_pose(B, rec.data_ptr(), cap, mask.data_ptr(), 0, out.data_ptr(), hq)
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
    if variant == "hpose":
        r = out.cpu().numpy().view(vislam.HPOSE_RESULT_DTYPE)
        pl = r[r["kind"] == vislam.HP_PLANE]
        extra = {"kinds": {vislam.HP_KIND_NAMES[k]: int((r["kind"] == k).sum()) for k in range(3)}, "voters_per_launch": int(r["n_tested"].sum()),
                 "plane_flags": {n: int(((pl["flags"] & b) != 0).sum()) for n, b in (("ambiguous", 1), ("few", 4), ("low_parallax", 8))}}
        if not (r["kind"] != vislam.HP_NONE).any():
            raise RuntimeError("no pair of the last launch has a homography pose")
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=tuple(base.SHAPES), default="headline")
    a = ap.parse_args()
    import torch
    import vislam
    S = base.SHAPES[a.shape]
    c = vislam.Context(0)
    fr = base.frames_on_device(torch, vislam, c, S)
    c.close()
    vs = ("homography", "hpose")
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    summary = {v: {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                   "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)} for v in vs}
    summary["hpose_vs_homography_median_pct"] = round(100.0 * (statistics.median(res["hpose"]) / statistics.median(res["homography"]) - 1.0), 2)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
