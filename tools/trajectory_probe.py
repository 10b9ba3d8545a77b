#!/usr/bin/env python3
"""Probe: what the scale links and the chained trajectory cost behind every launch of the pipelined stream path -- vis_batch_run(VIS_STAGE_ALL)
on 1024 S-752 frames per launch (752 x 480, no sync between launches) without follow-ups ("plain"), with vis_batch_triangulate ("tri": what the
links need anyway), with vis_batch_scale_links behind it ("links"), with vis_batch_trajectory behind that ("traj"), and -- the yardstick of
DESIGN.md 4.18 -- with vis_batch_ftrack alone ("ftrack").  The variants alternate in ONE process, each on a context of its own, so that clocks
and placement drift hit all alike; the window is closed by vis_batch_sync and a device synchronise.

  python3 tools/trajectory_probe.py [--rounds 5] [--steps 20] [--profile] [--shape headline|config3]

--shape config3: BASELINE config 3 (1920 x 1080, 4000 features on 4 levels, 64 frames per launch, VIS_POSE_SYM: lists beyond the LDS form).
--profile then runs a short "traj" leg in a fresh child process under `rocprofv3 --kernel-trace --stats` (no counters in the same run) and prints
the stats rows of the k_sl_* / k_tj_* kernels: k_tj_chain has ONE call per launch.  One JSON line per measurement; the "links" lines carry what
the last launch linked and the streaming floor of the depth and ratio passes: the bytes they move per launch / 8 TB/s."""
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
R, DIM = 2, 4096
SHAPES = {"headline": dict(w=752, h=480, B=1024, seed=0xE0C00001), "config3": dict(w=1920, h=1080, B=64, seed=0xE0C00003)}
KERNELS = ("k_sl_depth", "k_sl_ratio", "k_sl_carry", "k_tj_chain")
VARIANTS = ("plain", "tri", "links", "traj", "ftrack")
HBM_BYTES_PER_S = 8e12


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


def link_bytes(B, kcap, mcap):
    """bytes the two passes move per launch, counted from the shapes with every list full: the depth pass clears and rewrites a row of kcap doubles
    (8 + 8 + 8 read back), reads the list, its flag bytes and one 8-byte atomic per entry (16 + 1 + 8) and a 32-byte map point per winner; the
    ratio pass scans the keyframe's row (8 per keypoint), reads the list, flags, the point's sector and the gathered depth (16 + 1 + 32 + 8)"""
    return B * (kcap * (24 + 8) + mcap * (25 + 32 + 57))


def timed(torch, vislam, fr, S, shape, variant, steps, warmup):
    p = params(vislam, shape)
    c = vislam.Context(0, p)
    B = S["B"]
    c.batch_plan(S["w"], S["h"], S["w"], B)
    kcap = c.keypoint_capacity(S["w"], S["h"])
    mcap = kcap if p.pose_input == 1 else int(np.floor(np.sqrt(p.n_cells))) ** 2
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    pts, fl, sm = z(B * mcap * 32), z(B * mcap), z(B * 16)
    link, traj, poses = z(B * 40), z(B * 128), z(B * 96)
    obs, frm = z(B * kcap * 16 if variant == "ftrack" else 16), z(B * 32)
    sp = vislam.default_scale_link_params()
    torch.cuda.synchronize()

    def step(i):
        c.batch_run(fr.data_ptr() + (i % R) * B * S["w"] * S["h"], B, vislam.STAGE_ALL)
        if variant in ("tri", "links", "traj"):
            c.batch_triangulate(B, mcap, pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
        if variant in ("links", "traj"):
            c.batch_scale_links(B, pts.data_ptr(), fl.data_ptr(), mcap, link.data_ptr(), sp)
        if variant == "traj":
            c.batch_trajectory(B, link.data_ptr(), traj.data_ptr(), poses.data_ptr())
        if variant == "ftrack":
            c.batch_ftrack(B, kcap, obs.data_ptr(), frm.data_ptr())
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
    if variant in ("links", "traj"):
        l = link.cpu().numpy().view(vislam.SCALE_LINK_DTYPE)
        nbytes = link_bytes(B, kcap, mcap)
        extra = {"keypoint_capacity": kcap, "list_capacity": mcap, "links_ok": int((l["flags"] == vislam.SL_OK).sum()), "links_few": int((l["flags"] & vislam.SL_FEW != 0).sum()),
                 "links_no_depth": int((l["flags"] == vislam.SL_NO_DEPTH).sum()), "median_n_shared": int(np.median(l["n_shared"])),
                 "link_bytes_per_launch": nbytes, "link_streaming_floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2)}
    if variant == "traj":
        t = traj.cpu().numpy().view(vislam.TRAJ_POSE_DTYPE)
        extra.update({"max_hops": int(t["hops"].max()), "roots": int((t["flags"] & vislam.TJ_ROOT != 0).sum()), "unit_edges": int((t["flags"] & vislam.TJ_UNIT_EDGE != 0).sum()),
                      "overflow": int((t["flags"] & vislam.TJ_OVERFLOW != 0).sum()), "dense_poses": int((poses.cpu().numpy().view(np.float64).reshape(B, 12)[:, :9] != 0).any(1).sum())})
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return steps * B / dt, extra


def profile(a):
    out = tempfile.mkdtemp(prefix="trajectory_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trajectory", "--",
           sys.executable, os.path.abspath(__file__), "--only", "traj", "--rounds", "1", "--steps", "5", "--warmup", "2", "--shape", a.shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"rocprofv3 run failed: {r.returncode}")
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no scale-link / trajectory kernel rows in the stats under {out}")
    print(json.dumps({"profiled_launches": 7}), flush=True)          # (2 warm-up + 5 timed: k_tj_chain's Calls must equal it)
    for row in rows:
        print(json.dumps({"kernel": row.get("Name"), "stats": row}), flush=True)      # Calls, TotalDurationNs, AverageNs, ... as rocprofv3 writes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--only", choices=VARIANTS, default=None, help="one variant (the profiled child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import vislam
    S = SHAPES[a.shape]
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c, S)
    c.close()
    vs = (a.only,) if a.only else VARIANTS
    res = {v: [] for v in vs}
    for rnd in range(a.rounds):
        for v in vs:
            fps, extra = timed(torch, vislam, fr, S, a.shape, v, a.steps, a.warmup)
            res[v].append(fps)
            line = {"round": rnd, "shape": a.shape, "variant": v, "frames_per_s": round(fps), "ms_per_step": round(S["B"] / fps * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    summary = {}
    for v in vs:
        summary[v] = {"best": round(max(res[v])), "median": round(statistics.median(res[v])), "min": round(min(res[v])),
                      "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2),
                      "median_ms_per_step": round(S["B"] / statistics.median(res[v]) * 1e3, 3)}
    if len(vs) == len(VARIANTS):                                    # the cost of each call per launch: the step of a variant less that of the one before
        ms = {v: summary[v]["median_ms_per_step"] for v in vs}
        summary["cost_ms_per_launch"] = {"triangulate": round(ms["tri"] - ms["plain"], 3), "scale_links": round(ms["links"] - ms["tri"], 3),
                                         "trajectory": round(ms["traj"] - ms["links"], 3), "ftrack_link_step": round(ms["ftrack"] - ms["plain"], 3)}
    print(json.dumps(summary), flush=True)
    del fr
    if a.profile:
        profile(a)


if __name__ == "__main__":
    main()
