#!/usr/bin/env python3
"""Probe: what the loop-candidate calls cost behind every launch of the pipelined stream path.  The baseline ("run") is vis_batch_run(VIS_STAGE_ALL)
on 1024 S-752 frames per launch (752 x 480, no sync between launches).  The variants add, behind each launch,
  q<entry_cap>s<step>   vis_batch_kfdb_query against a FULL database of entry_cap entries, every `step`-th frame a query (256 / 1024 / 4096 x 1 / 8 / 32)
  add1                  vis_batch_kfdb_add of every frame into a database of 1024 entries
  q1024s8m              q1024s8 followed by vis_batch_kfdb_match of the rank-0 candidates (max_pts 512)
The database is filled before the window opens (vis_batch_kfdb_add, step 1, over as many launches as it takes) and is not changed inside it, and
min_gap is 0, so every entry is eligible for every query: couples per launch = queries x entry_cap.  The variants alternate in ONE process, each
on a context of its own, so that clocks and placement drift hit all alike; the window is closed by vis_batch_sync and a device synchronise.
One JSON line per measurement, then the medians, what each variant adds to the baseline's launch and the time per couple.

  python3 tools/kfdb_probe.py [--rounds 3] [--steps 3] [--only NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
R, DIM, W, H, B, SEED = 2, 4096, 752, 480, 1024, 0xE0C00001
VARIANTS = ("run",) + tuple(f"q{e}s{s}" for e in (256, 1024, 4096) for s in (1, 8, 32)) + ("add1", "q1024s8m")
MAXP = 512


def frames_on_device(torch, vislam, ctx):
    canvas = torch.from_numpy(vislam.synth_canvas(DIM, SEED)).cuda()
    fr = torch.empty((B * R, H, W), dtype=torch.uint8, device="cuda")
    for t0 in range(0, B * R, 256):
        ctx.synth_frames_device(canvas.data_ptr(), DIM, SEED, t0, 256, W, H, W, fr.data_ptr() + t0 * W * H, parallax=True)
    torch.cuda.synchronize()
    return fr


def timed(torch, vislam, fr, variant, steps, warmup):
    p = vislam.default_params()
    p.fy = p.fx
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    cap = c.keypoint_capacity(W, H)
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    lp = vislam.default_loop_params()
    lp.min_gap = 0
    entry_cap, step, match, add = 0, 0, False, False
    if variant == "add1":
        entry_cap, add = 1024, True
    elif variant != "run":
        match = variant.endswith("m")
        e, s = variant.rstrip("m")[1:].split("s")
        entry_cap, step = int(e), int(s)
    db = c.kfdb(entry_cap, cap) if entry_cap else None
    if step:
        sc, ca, qu = z(B * entry_cap * 4), z(B * lp.topk * 16), z(B * 32)
        if match:
            m, p1, p2, npts = z(B * MAXP * 16), z(B * MAXP * 8), z(B * MAXP * 8), z(B * 4)
    torch.cuda.synchronize()
    run = lambda i: c.batch_run(fr.data_ptr() + (i % R) * B * W * H, B, vislam.STAGE_ALL)
    filled = 0
    while step and filled < entry_cap:                              # a full database of older frames
        run(filled // B)
        db.batch_add(B, 1)
        filled += B

    def one(i):
        run(i)
        if step:
            db.batch_query(B, sc.data_ptr(), ca.data_ptr(), qu.data_ptr(), step, lp)
            if match:
                db.batch_match(B, ca.data_ptr(), lp.topk, MAXP, m.data_ptr(), p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), lp)
        if add:
            db.batch_add(B, 1)
    for i in range(warmup):
        one(i)
    c.batch_sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(warmup + i)
    c.batch_sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = c.batch_status() == 0
    extra = {"keypoint_capacity": cap}
    if step:
        q = qu.cpu().numpy().view(vislam.LOOP_QUERY_DTYPE)
        live = q[q["flags"] == 0]
        extra.update({"entry_cap": entry_cap, "step": step, "queries_per_launch": int(len(live)), "couples_per_launch": int(q["n_scored"].sum()),
                      "median_keypoints_of_a_query": int(np.median(live["n_keypoints"])) if len(live) else 0,
                      "median_best_score": int(np.median(live["best_score"])) if len(live) else 0, "candidates_per_launch": int(q["n_cand"].sum())})
        if match:
            extra["matches_emitted_per_launch"] = int(npts.cpu().numpy().view(np.int32).sum())
    if db is not None:
        extra["database_bytes"] = entry_cap * cap * 136
        db.close()
    c.close()
    if not ok:
        raise RuntimeError("device capacity flag set")
    return dt / steps * 1e3, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma-separated variants beside the baseline")
    a = ap.parse_args()
    import torch
    import vislam
    c = vislam.Context(0)
    fr = frames_on_device(torch, vislam, c)
    c.close()
    vs = ("run",) + tuple(v for v in a.only.split(",") if v != "run") if a.only else VARIANTS
    assert all(v in VARIANTS for v in vs), vs
    res, last = {v: [] for v in vs}, {}
    for rnd in range(a.rounds):
        for v in vs:
            ms, extra = timed(torch, vislam, fr, v, a.steps, a.warmup)
            res[v].append(ms)
            last[v] = extra
            line = {"round": rnd, "variant": v, "ms_per_launch": round(ms, 3), "frames_per_s": round(B / ms * 1e3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    base = statistics.median(res["run"])
    summary = {"run": {"median_ms_per_launch": round(base, 3), "spread_pct": round(100.0 * (max(res["run"]) / min(res["run"]) - 1.0), 2)}}
    for v in vs[1:]:
        med = statistics.median(res[v])
        s = {"median_ms_per_launch": round(med, 3), "adds_ms_per_launch": round(med - base, 3), "spread_pct": round(100.0 * (max(res[v]) / min(res[v]) - 1.0), 2)}
        couples = last[v].get("couples_per_launch", 0)
        if couples and not v.endswith("m"):
            s["us_per_couple"] = round((med - base) * 1e3 / couples, 4)
        summary[v] = s
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
