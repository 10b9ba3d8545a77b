#!/usr/bin/env python3
"""Probe: the headline workload -- vis_batch_run(VIS_STAGE_ALL) on 1024 S-752 frames per launch (752 x 480, no sync between launches) --
with the rotation guide off (vis_batch_run) against on (vis_batch_run_guided) at window radii of 8, 16, 32 and 64 pixels.  The variants
alternate in ONE process, each on a context of its own; the window is closed by vis_batch_sync and a device synchronise.

The S-752 stream moves by image shifts: the crop origin advances (12, 8) pixels per frame (csrc/synth_core.h), so a point of the current
frame lies (12, 8) pixels further right / down in the previous one.  Every pair gets the rotation that predicts this shift at the
principal point: a turn of atan(12 / fx) about the camera's y axis and of -atan(8 / fy) about its x axis (away from the centre the
prediction of a rotation is not a constant shift: it is off by a few pixels towards the corners, which is what the radii are for).

Per variant: frames per second of the whole pipelined step, ms_knn of the last launch (vis_timings: expansion + prediction + both 2-NN
directions of all 1024 pairs), good matches per pair and the share of RANSAC inliers among the pose stage's correspondences.

  python3 tools/guided_match_probe.py [--rounds 3] [--steps 10] [--popcount] [--unguided-only]

--popcount adds the popcount kernel at the same frames: a context with keypoint_capacity 16385 (rows too long for the MFMA kernel),
256 frames per launch, detect + match stages.  The match filters refuse that capacity (VIS_E_CAPACITY) behind the 2-NN, so only
ms_knn is reported for it, per pair like the other variants' ms_knn_per_pair.  --unguided-only runs what a build without the guided
entry points has (VISLAM_HIP_LIB=<older library>: the parent's numbers).  One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
R, DIM, W, H, B, SEED = 2, 4096, 752, 480, 1024, 0xE0C00001
RADII = (8.0, 16.0, 32.0, 64.0)
SHIFT = (12.0, 8.0)


def params(vislam):
    p = vislam.default_params()
    p.fy = p.fx
    return p


def shift_rotation(p):
    ty, tx = np.arctan(SHIFT[0] / p.fx), -np.arctan(SHIFT[1] / p.fy)
    ry = np.array([[np.cos(ty), 0, np.sin(ty)], [0, 1, 0], [-np.sin(ty), 0, np.cos(ty)]])
    rx = np.array([[1, 0, 0], [0, np.cos(tx), -np.sin(tx)], [0, np.sin(tx), np.cos(tx)]])
    return (ry @ rx).astype(np.float32)


def frames_on_device(torch, vislam, ctx, n):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, SEED)).cuda()
    fr = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    for t0 in range(0, n, 256):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, SEED, t0, 256, W, H, W, fr.data_ptr() + t0 * W * H)
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, radius, steps, warmup):
    """radius None: unguided"""
    p = params(vislam)
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    rot = torch.from_numpy(np.tile(shift_rotation(p).reshape(9), (B, 1))).cuda()
    torch.cuda.synchronize()

    def step(i):
        ptr = fr.data_ptr() + (i % R) * B * W * H
        if radius is None:
            c.batch_run(ptr, B, vislam.STAGE_ALL)
        else:
            c.batch_run_guided(ptr, B, rot.data_ptr(), radius, vislam.STAGE_ALL)
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
    ms_knn = float(c.timings().ms_knn)
    poses, _, ngood = c.batch_results(B)
    if c.batch_status() != 0:
        raise RuntimeError("device capacity flag set")
    pts, inl = int(poses["n_points"][1:].sum()), int(poses["n_inliers"][1:].sum())
    c.close()
    return dict(frames_per_s=round(steps * B / dt), ms_knn=round(ms_knn, 4), ms_knn_per_pair=round(ms_knn / B, 6),
                good_per_pair=round(float(ngood[1:].mean()), 2), inlier_share=round(inl / max(pts, 1), 4))


def popcount_knn(torch, vislam, fr, radius, steps):
    """ms_knn of the popcount kernel (keypoint_capacity 16385) on 256 of the same frames per launch"""
    n = 256
    p = params(vislam)
    p.keypoint_capacity = 16385
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    rot = torch.from_numpy(np.tile(shift_rotation(p).reshape(9), (n, 1))).cuda()
    torch.cuda.synchronize()
    stages = vislam.STAGE_DETECT | vislam.STAGE_MATCH
    best = None
    for i in range(steps):
        ptr = C.c_void_p(fr.data_ptr() + (i % R) * n * W * H)
        if radius is None:
            rc = vislam.lib.vis_batch_run(c._h, ptr, n, stages)
        else:
            rc = vislam.lib.vis_batch_run_guided(c._h, ptr, n, stages, C.c_void_p(rot.data_ptr()), radius)
        if rc != -4:                                               # VIS_E_CAPACITY from the filters, behind the 2-NN that is timed here
            raise RuntimeError(f"expected the filters' VIS_E_CAPACITY, got {rc}")
        c.batch_sync()
        ms = float(c.timings().ms_knn)
        best = ms if best is None else min(best, ms)
    c.close()
    return dict(frames_per_launch=n, ms_knn=round(best, 4), ms_knn_per_pair=round(best / n, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--popcount", action="store_true")
    ap.add_argument("--unguided-only", action="store_true", help="only the variants an older build selected with VISLAM_HIP_LIB has")
    a = ap.parse_args()
    import torch
    import vislam
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, B * R)
    c.close()
    variants = [("off", None)] + ([] if a.unguided_only else [(f"r{int(r)}", r) for r in RADII])
    res = {v: [] for v, _ in variants}
    for rnd in range(a.rounds):
        for v, radius in variants:
            m = timed(torch, vislam, fr, radius, a.steps, a.warmup)
            res[v].append(m)
            print(json.dumps(dict(round=rnd, variant=v, **m)), flush=True)
    summary = {}
    for v, _ in variants:
        summary[v] = {k: round(statistics.median(m[k] for m in res[v]), 6) for k in res[v][0]}
        summary[v]["ms_knn_min"] = min(m["ms_knn"] for m in res[v])
        summary[v]["ms_knn_max"] = max(m["ms_knn"] for m in res[v])
    print(json.dumps(dict(summary=summary)), flush=True)
    if a.popcount:
        for v, radius in (("popcount_off", None),) + (() if a.unguided_only else (("popcount_r16", 16.0),)):
            print(json.dumps(dict(variant=v, **popcount_knn(torch, vislam, fr, radius, max(a.steps // 2, 3)))), flush=True)


if __name__ == "__main__":
    main()
