#!/usr/bin/env python3
"""bench.py -- frames/sec of the MI355X-native detect -> match -> pose hot path.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 the driver launches it
under torch.distributed.run, one rank per GPU.  One JSON line on rank 0.  Such a plain run sets up, warms up, times
the K steps and prints the line (metric, value, unit, ms_per_step, ...); `--dump-outputs DIR` also writes what the
last timed step computed (dump_outputs).  The side measurements listed further down are taken only with `--full`.

Headline workload (BASELINE.json configs[1]): synthetic 752x480 mono8 EuRoC-shaped stream ("S-752", integer-only
generator, vi-slam_amd/csrc/synth_core.h), ORB 1000 keypoints x 8 levels, BF-Hamming k=2 both directions +
ratio/symmetry/grid filter, essential RANSAC + recoverPose.  A "step" = one pass of the whole hot path over one batch of
4096 consecutive frames that are already resident in HBM, as 4 launches of 1024 frames (the plan's device buffers are sized
for 1024; `kernels_ms_per_step`, `roofline` and the counter figures are PER LAUNCH of 1024 frames).
Multi-GPU (configs[3]): rank r processes its own stream (seed + r); the only collective is one broadcast of the
parameter/intrinsics struct from rank 0 (RCCL); scaling is weak.

With `--full`, beside `value` the line carries (rank 0, N = 1 only, all OUTSIDE the timed region of `value`):
  legs.s752_fixed1000   the same stream with ransac_adaptive = 0: 1000 hypotheses per pair (the pose kernels loaded)
  legs.s752_parallax    "S-752P": two depth layers + independently moving objects (adaptive RANSAC does real work)
  legs.s752_results_d2h the headline step + a pinned, overlapped D2H copy of poses and good matches every step
  legs.s752_mispredicted_thresholds  alternating incoherent batches: the cost of wrong FAST threshold predictions (redone inside the step)
  legs.config3_s1080    BASELINE configs[2]: 1920x1080, 4 levels, 4000 kps, RANSAC 2000 fixed iterations on the symmetric matches
  legs.config5_s2160    BASELINE configs[4]: 3840x2160, 8000 kps, 8000 x 8000 all-pairs
  legs.align_n4         SURVEY 8(f) N4: half pyramid + gradients + batched Gauss-Newton photometric alignment
  cpu_baseline*         the oracle ('port' of the reference CPU path) on the host cores: config 2 single thread,
                        config 1 (ORB::create(200), first frames of S-752), and frame-parallel on all cores
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (device memory + torch.distributed plumbing; imported before the HIP library)
import vislam  # noqa: E402
from vislam import dist as vdist  # noqa: E402

W, H, NFEAT, LEVELS = 752, 480, 1000, 8
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable copy)
FAM = ("ms_update", "ms_pyramid", "ms_fast", "ms_select", "ms_describe", "ms_knn", "ms_filter", "ms_pose", "ms_total")
SIMD_ISSUE_PEAK = 256 * 4 * 2.4e9 / 2       # wave-instr/s: 256 CUs x 4 SIMD-32, one wave64 VALU instruction per 2 cycles (MI355X_MICROARCH.md)


# a synthetic EuRoC-shaped calibration (no distortion, ORB + GPU Hamming matcher) for the adapter-level leg (legs.single_frame_api.add_frame_gpu)
CAL_XML = """<?xml version="1.0"?>
<opencv_storage>
<in_width type_id="integer"> 752 </in_width>
<in_height type_id="integer"> 480 </in_height>
<out_width type_id="integer"> 752 </out_width>
<out_height type_id="integer"> 480 </out_height>
<calibration_values type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 458.654 457.296 367.215 248.375 </data></calibration_values>
<rectification type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 0 0 0 0 </data></rectification>
<imu2cam0Transformation type_id="opencv-matrix">
  <rows>4</rows> <cols>4</cols> <dt>f</dt>
  <data> 0.0148655429818 -0.999880929698 0.00414029679422 -0.0216401454975
         0.999557249008 0.0149672133247 0.025715529948 -0.064676986768
        -0.0257744366974 0.00375618835797 0.999660727178 0.00981073058949
         0.0 0.0 0.0 1.0 </data></imu2cam0Transformation>
<camera_frecuency type_id="float"> 20 </camera_frecuency>
<imu_frecuency type_id="float"> 200 </imu_frecuency>
<min_features type_id="integer"> 20</min_features>
<num_max_keyframes type_id="integer"> 10</num_max_keyframes>
<start_index type_id="integer"> 0 </start_index>
<use_gt type_id="integer">1</use_gt>
<use_ros type_id="integer">0</use_ros>
<num_cells type_id="integer"> 49</num_cells>
<length_patch type_id="integer"> 3</length_patch>
<detector type_id="integer">2</detector>
<matcher type_id="integer">4</matcher>
</opencv_storage>
"""


def algorithmic_bytes(px, n):
    """SURVEY.md section 8(d) per-frame figures, split per kernel family (DESIGN.md 'Roofline')."""
    ptot = sum(px)
    return {
        "k_fast": ptot,                                     # every pyramid pixel read once
        "k_resize": (ptot - px[-1]) + (ptot - px[0]),       # each level read once as source + levels>=1 written
        "k_describe": n * 1369 + n * 60,                    # 37x37 blurred footprint + 32 B desc + 28 B keypoint
        "total_detect_describe": ptot + (ptot - px[0]) + (ptot - px[-1]) + n * 1369 + n * 60,
    }


class Stream:
    """B*R frames of a synthetic stream generated on the device (byte-identical to the host generator,
    tests/test_synth_gpu.py), so no rank spends host time or PCIe on frame synthesis."""

    def __init__(self, ctx, dev, w, h, count, seed, canvas_dim=4096, parallax=False):
        self.w, self.h, self.count = w, h, count
        self.canvas = vislam.synth_canvas(canvas_dim, seed)
        d_canvas = torch.from_numpy(self.canvas).to(dev)
        self.frames = torch.empty((count, h, w), dtype=torch.uint8, device=dev)
        step = 256
        for t0 in range(0, count, step):
            n = min(step, count - t0)
            ctx.synth_frames_device(d_canvas.data_ptr(), canvas_dim, seed, t0, n, w, h, w, self.frames.data_ptr() + t0 * w * h, parallax)
        torch.cuda.synchronize()
        del d_canvas

    def ptr(self, first):
        return self.frames.data_ptr() + first * self.w * self.h

    def host(self, n):
        return self.frames[:n].cpu().numpy()


class ClockSampler:
    """shader clock / memory clock / package power of ONE device, sampled from sysfs by a side thread WHILE the timed region runs
    (the HBM-bound stages have two bandwidth states from lease to lease; the record now says which clocks a run saw).
    sysfs (pp_dpm_sclk / pp_dpm_mclk: the level marked '*'; hwmon power1_average or power1_input in microwatts) costs a few file reads
    per sample; no subprocess, no HIP call.  Missing files give nulls, never an exception."""

    def __init__(self, pci_bus_id, period_s=0.05):
        import threading
        self.base = f"/sys/bus/pci/devices/{(pci_bus_id or '').lower()}"
        self.period = period_s
        self.samples = []
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _level(path):
        try:
            for line in open(path):
                if "*" in line:
                    return float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
        except Exception:
            pass
        return None

    def _power(self):
        import glob
        for pat in ("hwmon/hwmon*/power1_average", "hwmon/hwmon*/power1_input"):
            for f in glob.glob(os.path.join(self.base, pat)):
                try:
                    return float(open(f).read()) / 1e6
                except Exception:
                    continue
        return None

    def _run(self):
        while not self._stop.is_set():
            self.samples.append((self._level(os.path.join(self.base, "pp_dpm_sclk")), self._level(os.path.join(self.base, "pp_dpm_mclk")), self._power()))
            self._stop.wait(self.period)

    def __enter__(self):
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._th.join(timeout=2)

    def summary(self):
        med = lambda v: float(np.median(v)) if v else None                       # noqa: E731
        cols = [[x[i] for x in self.samples if x[i] is not None] for i in range(3)]
        return {"sclk_mhz": med(cols[0]), "mclk_mhz": med(cols[1]), "watts": med(cols[2]), "samples": len(self.samples),
                "source": f"sysfs {self.base} (median over the timed region)"}


def timed_steps(ctx, stream, B, R, stages, steps, warmup, dist=None, dev=None, after_step=None, q=1):
    """a step = q consecutive launches of the pipeline over q * B consecutive frames of the stream (q = 1 for the legs)"""
    def step(i):
        for s_ in range(q):
            ctx.batch_run(stream.ptr(((i % R) * q + s_) * B), B, stages)
        if after_step is not None:
            after_step(i)
    for i in range(warmup):
        step(i)
    ctx.batch_sync()
    if ctx.batch_status() != 0:
        raise RuntimeError("device capacity flag set during warm-up")
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    ctx.batch_sync()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if ctx.batch_status() != 0:
        raise RuntimeError("device capacity flag set during the timed region")
    return dt, step


def family_times(ctx, step, nprof=6):
    """per-kernel-family durations from HIP events on the library's streams, one batch in flight"""
    fam = {k: 0.0 for k in FAM}
    launches_fast = 1
    for i in range(nprof):
        step(i)
        ctx.batch_sync()
        t = ctx.timings()
        for k in fam:
            fam[k] += getattr(t, k) / nprof
        launches_fast = t.launches_fast
    return fam, launches_fast


def pose_load(ctx, n):
    """RANSAC load of the LAST batch: iterations, correspondences, candidate models"""
    pose, good, ng = ctx.batch_results(n)
    it = pose["iters_run"][1:].astype(np.int64)
    return {"iters_run_mean": float(it.mean()), "iters_run_max": int(it.max()), "correspondences_mean": float(pose["n_points"][1:].mean()),
            "pose_good_mean": float(pose["n_pose_good"][1:].mean()), "inliers_mean": float(pose["n_inliers"][1:].mean()),
            "hypotheses": int(it.sum()), "point_evals": int((pose["n_models"].astype(np.int64) * pose["n_points"]).sum())}


def kernel_rooflines(fam, launches_fast, px, nfeat, B, nlevels):
    alg = algorithmic_bytes(px, nfeat)
    out = {}
    for key, (name, nl) in {"ms_fast": ("k_fast", launches_fast), "ms_pyramid": ("k_resize", max(nlevels - 1, 1)), "ms_describe": ("k_describe", 1)}.items():
        if fam[key] <= 0:
            continue
        gbs = alg[name] * B / (fam[key] * 1e-3) / 1e9
        out[name] = {"ms": round(fam[key], 4), "launches": nl, "algorithmic_bytes_per_frame": alg[name], "GBps": gbs, "frac": gbs / HBM_PEAK_GBS}
    tot = fam["ms_pyramid"] + fam["ms_fast"] + fam["ms_select"] + fam["ms_describe"]
    out["detect_describe_GBps"] = alg["total_detect_describe"] * B / (tot * 1e-3) / 1e9
    return out, alg


MFMA_FP4_PEAK_PFLOPS = 10.0      # MI355X_MICROARCH.md "Matrix cores": FP6/FP4 dense ~10 PFLOP/s (the 20 PF headline figure includes 2:1 sparsity)


def matcher_roofline(ms_knn, n_desc, pairs, counters="headline", pmc_path=None):
    """north_star: 'L2-hit / VALU utilisation for the matcher against the chip's roofline'.  The matcher is k_expand + k_knn_mfma
    (v_mfma_scale_f32_32x32x64_f8f6f4 on FP4 +-1 operands, exact).  Per frame pair the kernel computes TWO n x n distance matrices
    (query->train and its transpose: the grid has a direction dimension, each direction keeps the row-wise top-2 of its own matrix),
    256 multiply-accumulates per distance.  `achieved` = those MACs x 2 FLOP / ms_knn of THIS run (HIP events, k_expand included);
    busy / hit / traffic figures come from the committed counter passes of the SAME workload (profiles/pmc_traffic.json: the headline
    set at the top level, the other configurations under legs.<name>, each stamped with its descriptors per frame) -- a set taken on
    another workload is never quoted: the fields are null and `counters_from` says why."""
    if not ms_knn or ms_knn <= 0:
        return None
    macs = 2.0 * n_desc * n_desc * 256 * pairs
    pf = macs * 2 / (ms_knn * 1e-3) / 1e15
    out = {"bound": "mfma-fp4", "kernel": "k_expand + k_knn_mfma", "achieved_PFLOPs": pf, "achieved_PMACs": pf / 2, "peak": MFMA_FP4_PEAK_PFLOPS, "unit": "PFLOP/s",
           "frac": pf / MFMA_FP4_PEAK_PFLOPS, "ms_knn": ms_knn, "descriptors_per_frame": n_desc, "pairs_per_step": pairs,
           "distance_matrices_per_pair": 2, "macs_per_step": macs, "mfma_busy_frac": None, "l2_hit": None, "traffic_over_algorithmic": None}
    try:
        pj = json.load(open(pmc_path or os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        cs = pj if counters == "headline" else (pj.get("legs") or {}).get(counters)
        if cs is None:
            out["counters_from"] = f"not measured for this workload (profiles/pmc_traffic.json has no legs.{counters})"
            return out
        if int(cs.get("n_desc", 1000 if counters == "headline" else -1)) != int(n_desc):
            out["counters_from"] = f"not measured for this workload (the committed set is for {cs.get('n_desc')} descriptors per frame, this leg has {n_desc})"
            return out
        raw = cs["raw"]["k_knn_mfma"]
        hit, miss = raw["TCC_HIT_sum"]["mean"], raw["TCC_MISS_sum"]["mean"]
        out["l2_hit"] = hit / (hit + miss)
        # SQ_VALU_MFMA_BUSY_CYCLES counts cycles per SIMD; GRBM_GUI_ACTIVE is summed over the 8 XCDs: cycles x 1024 SIMDs
        out["mfma_busy_frac"] = raw["SQ_VALU_MFMA_BUSY_CYCLES"]["mean"] / (raw["GRBM_GUI_ACTIVE"]["mean"] / 8 * 1024)
        out["counters_from"] = (f"profiles/pmc_traffic.json {'top level' if counters == 'headline' else 'legs.' + counters} raw.k_knn_mfma (TCC_HIT_sum, TCC_MISS_sum, "
                                f"SQ_VALU_MFMA_BUSY_CYCLES, GRBM_GUI_ACTIVE; {cs['batch_frames']} frames of {n_desc} descriptors per launch, commit {cs.get('measured_at_commit')})")
        # HBM traffic of k_knn_mfma against what it must read: the expanded descriptors (128 B each) of both frames of every pair
        alg_b = 2.0 * n_desc * 128 * cs["batch_frames"]
        out["hbm_traffic_bytes_per_launch_at_pmc_batch"] = cs["k_knn_mfma"]["hbm_bytes_per_launch"]
        out["algorithmic_bytes_per_launch_at_pmc_batch"] = alg_b
        out["traffic_over_algorithmic"] = cs["k_knn_mfma"]["hbm_bytes_per_launch"] / alg_b
    except Exception as e:
        out["counters_error"] = repr(e)
    return out


def leg_detect_counters(label, leg, B):
    """counter figures of a side leg's OWN workload (profiles/pmc_traffic.json legs.<label>, written by tools/final_profile.sh from counter
    passes at that leg's image size and keypoint count): HBM traffic against the algorithmic bytes of SURVEY 8(d) per detect/describe kernel."""
    try:
        cs = (json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("legs") or {}).get(label)
        if cs is None:
            return {"counters_from": f"not measured for this workload (no legs.{label} in profiles/pmc_traffic.json)"}
        out = {"counters_from": f"profiles/pmc_traffic.json legs.{label} ({cs['batch_frames']} frames per launch, commit {cs.get('measured_at_commit')})"}
        for k in ("k_fast", "k_resize", "k_describe", "k_select", "k_select_1024"):
            if k not in cs:
                continue
            calls = cs["raw"][k]["FETCH_SIZE"]["calls"] / max(1, cs.get("steps_counted", 1))          # launches of the family per step
            hbm = cs[k]["hbm_bytes_per_launch"] * calls                                             # per step of batch_frames frames
            d = {"hbm_traffic_bytes_per_frame": hbm / cs["batch_frames"], "lds_busy_frac": cs[k].get("lds_busy_frac"),
                 "valu_wave_insts_per_frame": (cs[k].get("valu_wave_insts_per_launch") or 0) * calls / cs["batch_frames"]}
            ab = ((leg.get("kernels") or {}).get(k) or {}).get("algorithmic_bytes_per_frame")
            if ab:
                d["traffic_over_algorithmic"] = d["hbm_traffic_bytes_per_frame"] / ab
            out[k] = d
        return out
    except Exception as e:
        return {"counters_error": repr(e)}


def run_leg(dev, w, h, B, R, params, seed, canvas_dim, steps, warmup, stages=None, parallax=False, want_pose=True, d2h=False):
    if stages is None:                                   # every leg runs Camera::Update inside the step, like the headline (1080p included since round 4)
        stages = vislam.STAGE_FRAME
    ctx = vislam.Context(dev.index or 0, params)
    try:
        st = Stream(ctx, dev, w, h, B * R, seed, canvas_dim, parallax)
        ctx.batch_plan(w, h, w, B)
        after = None
        if d2h:
            root2 = int(np.floor(np.sqrt(params.n_cells))) ** 2
            hp = torch.empty(B * C.sizeof(vislam.PoseResult), dtype=torch.uint8).pin_memory()
            hg = torch.empty(B * root2 * 16, dtype=torch.uint8).pin_memory()
            hn = torch.empty(B, dtype=torch.int32).pin_memory()
            after = lambda i: ctx.batch_results_async(B, hp.data_ptr(), hg.data_ptr(), hn.data_ptr())   # noqa: E731
        dt, step = timed_steps(ctx, st, B, R, stages, steps, warmup, after_step=after)
        fam, lf = family_times(ctx, step, 4)
        ws, hs, sc, q = ctx.level_geometry(w, h)
        px = [int(a) * int(b) for a, b in zip(ws, hs)]
        roof, alg = kernel_rooflines(fam, lf, px, params.nfeatures, B, params.nlevels)
        out = {"frames_per_step": B, "steps": steps, "ms_per_step": dt / steps * 1e3, "frames_per_s": B * steps / dt,
               "kernels_ms_per_step": {k: round(v, 4) for k, v in fam.items()}, "kernels": roof}
        if want_pose and (stages & vislam.STAGE_POSE):
            step(0); ctx.batch_sync()
            ms_pose = ctx.timings().ms_pose               # before the results download re-syncs the streams
            pl = pose_load(ctx, B)
            pl["ms_pose_per_step"] = ms_pose
            pl["hypotheses_per_s"] = pl["hypotheses"] / (ms_pose * 1e-3) if ms_pose > 0 else None
            pl["point_evals_per_s"] = pl["point_evals"] / (ms_pose * 1e-3) if ms_pose > 0 else None
            out["ransac"] = pl
        return out
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def pose_kernels(leg):
    """the pose kernels of a loaded leg against the measured issue ceilings: instruction counts and standalone launch durations from the
    committed counter pass (profiles/pmc_pose.json: tools/final_profile.sh step 4, other run, same kernels and workload; a counter pass
    serialises the kernels), double-precision ceiling = tools/f64_rates.hip's Horner pair (v_mul_f64 + v_add_f64, 2 waves per SIMD) of the
    same lease, single-precision ceiling = valu_peak_measured.full_rate_class of profiles/pmc_traffic.json.  k_hyp_score decides in single
    precision (its double fallback is a fraction of a percent of the decisions) and is priced against the single-precision ceiling; in
    the few-correspondences form of the fixed-1000 leg it is bound by model staging and LDS adds, not by the arithmetic.  Everything
    else is double precision."""
    try:
        pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_pose.json")))
        ks = pj["legs"][leg]
        f64 = pj["f64_issue_ceiling"]["by_instruction_2_waves_per_simd_4_chains"]["v_mul_f64 + v_add_f64 (Horner step, 2 instr)"]
        f32 = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["valu_peak_measured"]["full_rate_class"]
        out = {"counters_from": f"profiles/pmc_pose.json legs.{leg} (commit {pj.get('measured_at_commit')})", "f64_issue_ceiling": f64, "f32_full_rate_ceiling": f32,
               "unit": "wave-instr/s", "kernels": {}}
        for k, v in ks.items():
            if v.get("SQ_INSTS_VALU", 0) < 1e6:
                continue
            single = (k == "k_hyp_score")
            out["kernels"][k] = {"ms_standalone": v["ms"], "valu_wave_insts": v["SQ_INSTS_VALU"], "salu_wave_insts": v.get("SQ_INSTS_SALU"),
                                 "achieved": v["valu_wave_insts_per_s"], "ceiling": "f32 full rate" if single else "f64",
                                 "frac": v["valu_wave_insts_per_s"] / (f32 if single else f64)}
        return out
    except Exception as e:
        return {"error": f"profiles/pmc_pose.json unusable: {e!r}"}


def usable_cpus():
    """host threads this process may really use: the scheduler affinity mask, capped by the cgroup CPU quota (a GPU box
    hands one GPU's share of a 256-thread host to the job)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                if q > 0:
                    quota = q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            break
        except Exception:
            continue
    if quota:
        n = max(1, min(n, int(quota + 0.5)))
    return n, quota


def cpu_baseline(p, frames, budget_s, what):
    """oracle ('port' of the reference CPU path) timed on this host, 1 thread, bounded sample"""
    import oracle_bind as orc
    prev = None
    n = 0
    for t in range(3):                                   # warm-up
        k, d, r = orc.pipeline_frame(p, frames[t], prev)
        prev = (k, d)
    t0 = time.perf_counter()
    for t in range(3, len(frames)):
        k, d, r = orc.pipeline_frame(p, frames[t], prev)
        prev = (k, d)
        n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port", "sample_short": f"{n} S-752 frames, oracle pipeline_frame, g++ -O2, 1 thread",
            "sample": f"{n} consecutive S-752 frames ({what}), oracle pipeline_frame: Camera::Update + ORB + knn x2 + filters + essential RANSAC + "
                      f"recoverPose, g++ -O2, 1 thread; host has {os.cpu_count()} logical CPUs"}


def headline(a, world, B, Q, dt, ranks):
    """the fields of the result line that the timed steps alone decide (a plain run prints these and nothing else)"""
    return {
        "metric": "frames/sec detect+match+pose, 752x480 mono8", "value": vdist.aggregate_fps(world, a.steps, B * Q, dt), "unit": "frames/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        "ranks": ranks, **({"rehearsal": "N ranks on ONE device over gloo: exercises the N > 1 code path, not a scaling measurement"} if a.rehearse_on_one_gpu else {}),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload_short": "S-752 synthetic 752x480 mono8 resident in HBM; ORB 1000 kps x 8 levels, knn2 both ways + filters, essential RANSAC + recoverPose",
                   "workload": "S-752: synthetic 752x480 mono8 EuRoC-shaped stream (frames resident in HBM), 1000 ORB kps x 8 levels, BF-Hamming k=2 "
                               "both directions + ratio/sym/grid filter, essential RANSAC (adaptive, max 1000) + recoverPose.  S-752 is a planar "
                               "crop under pure image translation: every grid match is an exact inlier, the adaptive stop ends RANSAC after "
                               "<= 4 hypotheses (see pose_load) and the recovered pose is degenerate; legs.s752_fixed1000 / legs.s752_parallax load "
                               "the pose kernels.  Results stay on the device inside the timed region (legs.s752_results_d2h adds the download); "
                               "Camera::Update's half pyramid (4 levels per frame) is part of the step, as it is of the CPU baseline.  "
                               "FAST runs at a per-level threshold predicted from the previous batch's retainBest cuts (a corner below the cut "
                               "is neither kept nor able to suppress a kept one), verified per (frame, level) on the device, mispredictions redone "
                               "at fast_threshold inside the step: keypoints identical to FAST at 20 for every input (fast_threshold_prediction)",
                   "frames_per_step_per_gpu": B * Q, "launches_per_step": Q, "frames_per_launch": B,
                   "parallelism": f"stream-per-gpu x{world}" if world > 1 else "single-gpu"},
    }


DUMP_SAMPLE_FRAMES, DUMP_SAMPLE_SEED = 16, 0xD0      # keypoints / descriptors of this many frames of the last launch, chosen by this seed


def dump_outputs(ctx, B, out_dir, first_frame, stages):
    """what every stage of the timed path wrote in its last step, as the library's accessors hand it to a caller: for the step's last
    launch of B frames (stream frames first_frame ...) the pose records, good matches and counts of vis_batch_results_async, and for a
    fixed, seeded sample of that launch's frames the keypoints + descriptors (vis_batch_get_keypoints) and Camera::Update's half
    pyramid levels 1-4 (vis_batch_half_pyramid; level 0 is the frame itself and is not part of the stage's output).  Integers are
    stored as float64 (exact); good-match slots past a frame's count are set to -1.  About 12 MB in all."""
    os.makedirs(out_dir, exist_ok=True)
    pose, good, ng = ctx.batch_results(B)                 # synchronises every stream of the context
    valid = np.arange(good.shape[1])[None, :] < ng[:, None]
    arrays = {"pose_E": pose["E"], "pose_R": pose["R"], "pose_t": pose["t"],
              "pose_counts": np.stack([pose[k] for k in ("n_inliers", "n_pose_good", "iters_run", "n_points", "n_models")], 1).astype(np.float64),
              "good_count": ng.astype(np.float64),
              "good_query": np.where(valid, good["queryIdx"], -1).astype(np.float64),
              "good_train": np.where(valid, good["trainIdx"], -1).astype(np.float64),
              "good_distance": np.where(valid, good["distance"], -1).astype(np.float32)}
    frames = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(B, size=min(DUMP_SAMPLE_FRAMES, B), replace=False))
    kps, descs = [], []
    for f in frames:
        k, d = ctx.batch_keypoints(int(f))
        kps.append(np.stack([np.full(len(k), f, np.float32)] + [k[n].astype(np.float32) for n in vislam.KEYPOINT_DTYPE.names], 1))
        descs.append(d.astype(np.float32))
    arrays["keypoints"] = np.concatenate(kps).reshape(-1, 1 + len(vislam.KEYPOINT_DTYPE.names))    # frame, x, y, size, angle, response, octave, class_id
    arrays["descriptors"] = np.concatenate(descs).reshape(-1, 32)                                    # one byte per column
    arrays["sample_stream_frames"] = (first_frame + frames).astype(np.float64)                       # which stream frames the sample holds
    if not stages & (vislam.STAGE_UPDATE | vislam.STAGE_GRADIENT):      # a --stages run without Camera::Update has no half pyramid
        return _save(out_dir, arrays)
    d_half, fe = ctx.batch_half_pyramid()
    lw, lh = vislam.half_pyramid_dims(W, H)
    o1, n14 = lw[0] * lh[0], sum(lw[l] * lh[l] for l in range(1, 5))

    class _Half:                                          # the plan's half pyramid buffer of this launch as a torch view
        __cuda_array_interface__ = {"data": (d_half, False), "shape": (B, fe), "typestr": "|u1", "version": 2}
    half = torch.as_tensor(_Half(), device="cuda")
    arrays["half_pyramid"] = half[torch.from_numpy(frames).to(half.device), o1:o1 + n14].cpu().numpy().astype(np.float32)   # levels 1..4, row-major, concatenated
    _save(out_dir, arrays)


def _save(out_dir, arrays):
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)   # 200 x 3.7 ms: a timed region long enough for an outside observer (rocm-smi) to see
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="frames per LAUNCH of the pipeline (the plan's device buffers are sized for it)")
    ap.add_argument("--launches-per-step", type=int, default=20,
                    help="a step = this many consecutive launches over consecutive frames of the stream (20 x 1024 = 20480 frames per step, 15 GB of resident "
                         "frames with --ring 2): the driver's --steps 20 is then 400 launches = 1 s of steady state that an outside sampler (rocm-smi) can see "
                         "(4 launches per step in round 4: 0.2 s, every busy sample read 0 %%)")
    ap.add_argument("--ring", type=int, default=2, help="distinct steps' worth of frames resident in HBM")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="REHEARSAL of the N > 1 code path on a box with ONE GPU: every rank uses device 0 and the ranks talk over gloo (RCCL refuses "
                         "two ranks on one device).  The line says so (\"rehearsal\") and is not a scaling measurement")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, measure everything else: clocks, per-kernel times, rooflines, pose load, side legs, CPU baselines; the "
                         "full record goes to --full-out.  A plain run only sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what every stage wrote in the last launch of the last timed step (pose records, good "
                         "matches and their counts; keypoints, descriptors and half pyramid of a fixed sample of its frames) as DIR/<name>.npy, "
                         "float32 / float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the side legs (profiling runs)")
    ap.add_argument("--full-out", default=None, help="where the FULL record (legs, counter tables, prose) is written; default gpurun_out/bench_full.json. stdout carries "
                                                     "only the compact line (benchline.py)")
    ap.add_argument("--stages", type=int, default=vislam.STAGE_FRAME, help="debug: bitmask of stages (1 detect, 2 match, 4 pose, 8 Camera::Update); the reported metric needs all 15")
    a = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.rehearse_on_one_gpu:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="gloo" if a.rehearse_on_one_gpu else "nccl", world_size=world, rank=rank)   # "nccl" == RCCL on ROCm
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    ddev = torch.device("cpu") if (world > 1 and a.rehearse_on_one_gpu) else dev      # where the collectives' tensors live

    # ---- parameters: rank 0 owns them; one RCCL broadcast of the POD struct ("intrinsics only")
    p = vislam.default_params()
    if rank == 0:
        p.nfeatures, p.nlevels, p.w_size, p.h_size = NFEAT, LEVELS, W, H
        p.fy = p.fx
    p = vdist.broadcast_params(p, dist, ddev, rank)

    ctx = vislam.Context(local_rank if world > 1 else 0, p)
    B, R, Q = a.batch, a.ring, max(1, a.launches_per_step)
    seed = vdist.stream_seed(rank, world)
    stream = Stream(ctx, dev, W, H, B * Q * R, seed)      # generated on the device: no host synthesis, no H2D
    ctx.batch_plan(W, H, W, B)
    clocks = ClockSampler(vislam.device_pci_bus_id(local_rank if world > 1 else 0)) if a.full else contextlib.nullcontext()
    with clocks:
        dt, step_q = timed_steps(ctx, stream, B, R, a.stages, a.steps, a.warmup, dist, dev, q=Q)
    dt_rank = dt
    dt = vdist.max_over_ranks(dt, dist, ddev)
    # who ran where: one all_gather of a small POD per rank behind the timed region (N ranks must sit on N different devices)
    dev_index = local_rank if world > 1 else 0
    ranks = vdist.gather_rank_records(vdist.pack_rank_record(rank, dev_index, a.steps * B * Q / dt_rank, dt_rank, vislam.device_pci_bus_id(dev_index)),
                                      dist, ddev, world)
    if not a.rehearse_on_one_gpu:
        vdist.check_distinct_devices(ranks)
    if rank == 0 and a.dump_outputs:
        dump_outputs(ctx, B, a.dump_outputs, ((a.warmup + a.steps - 1) % R * Q + Q - 1) * B, a.stages)     # the frames timed_steps' last launch read
    if not a.full:
        if rank == 0:
            import benchline
            print(benchline.compact_line(headline(a, world, B, Q, dt, ranks)), flush=True)
        ctx.close()
        del stream
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    def step(i):                                          # ONE launch (per-kernel timings, pose load: per launch of B frames)
        ctx.batch_run(stream.ptr((i % (R * Q)) * B), B, a.stages)
    fam, launches_fast = family_times(ctx, step, 8)
    tau_next, redone = ctx.batch_fast_thresholds()       # the speculative FAST thresholds (exact by construction; see include/vislam_hip.h)
    headline_pose = None
    if rank == 0 and (a.stages & vislam.STAGE_POSE):
        step(0); ctx.batch_sync()
        ms_pose = ctx.timings().ms_pose                   # before the results download re-syncs the streams
        headline_pose = pose_load(ctx, B)
        headline_pose["ms_pose_per_step"] = ms_pose

    # ---- SURVEY 8(f) N2 + N4 (outside the timed region, not part of `value`)
    aux, legs = None, None
    if rank == 0 and not a.no_legs:
        aux, legs = {}, {}
        try:
            fe = vislam.gradient_frame_elems(W, H)
            gray = torch.empty(B * fe, dtype=torch.uint8, device=dev)
            gxb = torch.empty(B * fe, dtype=torch.int16, device=dev); gyb = torch.empty_like(gxb)
            gb = torch.empty(B * fe, dtype=torch.uint8, device=dev)
            d0 = stream.ptr(0)
            def grad():
                ctx.gradient_batch(d0, W, H, W, B, gray.data_ptr(), gxb.data_ptr(), gyb.data_ptr(), gb.data_ptr())
            for _ in range(3):
                grad()
            torch.cuda.synchronize()
            tg = time.perf_counter()
            KG = 20
            for _ in range(KG):
                grad()
            torch.cuda.synchronize()
            tg = (time.perf_counter() - tg) / KG
            pg = sum((W >> l) * (H >> l) for l in range(5))
            p_half = sum((W >> l) * (H >> l) for l in range(4)) + sum((W >> l) * (H >> l) for l in range(1, 5))
            gbytes = 6 * pg + p_half                     # gradient: 1 B read + 5 B written per pixel; pyramid: read 4 levels, write 4
            aux["gradient_batch"] = {"what": "Camera::Update half pyramid + Camera::computeGradient (Scharr x/y int16 + blended u8), 5 levels",
                                     "ms_per_batch": tg * 1e3, "frames": B, "algorithmic_bytes_per_frame": gbytes,
                                     "achieved_GBps": gbytes * B / tg / 1e9, "peak_GBps": HBM_PEAK_GBS,
                                     "frac": gbytes * B / tg / 1e9 / HBM_PEAK_GBS, "frames_per_s": B / tg}
            # N4: VISystem::EstimatePoseFeatures on every consecutive pair of the batch (good matches from the plan)
            ctx.batch_reset()
            ctx.batch_run(d0, B, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
            ctx.batch_sync()
            outb = torch.empty(B * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device=dev)
            apar = vislam.default_align_params()
            def align():
                ctx.batch_align(apar, d0, B, gray.data_ptr(), gxb.data_ptr(), gyb.data_ptr(), 0, outb.data_ptr())
            for _ in range(2):
                align()
            ctx.batch_sync(); torch.cuda.synchronize()
            ta = time.perf_counter()
            KA = 10
            for _ in range(KA):
                align()
            ctx.batch_sync(); torch.cuda.synchronize()
            ta = (time.perf_counter() - ta) / KA
            raw = np.frombuffer(outb.cpu().numpy().tobytes(), dtype=np.uint8).reshape(B, -1)
            its = np.frombuffer(raw[:, 28 + 64 + 20 + 4:28 + 64 + 20 + 4 + 20].tobytes(), np.int32).reshape(B, 5)
            nres = np.frombuffer(raw[:, 28 + 64 + 20 + 4 + 20:].tobytes(), np.int32).reshape(B, 5)
            evals = int(((its[:, :4] + 1) * nres[:, :4]).sum())        # iterations evaluated x residuals of the level
            legs["align_n4"] = {"what": "VISystem::EstimatePoseFeatures (Gauss-Newton photometric alignment, levels 3..0, <= 10 iterations) on the "
                                        f"{B - 1} consecutive pairs of one batch, one persistent workgroup per pair; inputs = the N2 stage outputs",
                                "ms_per_batch": ta * 1e3, "pairs_per_s": (B - 1) / ta, "iterations_mean_per_level": [float(x) for x in its[1:, :4].mean(0)],
                                "residual_evals_per_s": evals / ta}
            # the per-frame sequence of the GPU main, src/VISystemGPU.cpp:137-175, as one pipelined step: Camera::Update +
            # addGPUKeyframe (detect, match + filters, computeGradient, patch points) + EstimatePoseFeatures, for every frame of the batch
            def main_step(i):
                d = stream.ptr((i % R) * B)
                # half pyramid + gradients into the plan's buffers on the side stream (beside the detect chain), alignment on the
                # pose stream (beside the next batch's detect chain)
                ctx.batch_run(d, B, vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT)
                ctx.batch_align(apar, d, B, 0, 0, 0, 0, outb.data_ptr())
            for i in range(3):
                main_step(i)
            ctx.batch_sync(); torch.cuda.synchronize()
            tm = time.perf_counter()
            KM = 20
            for i in range(KM):
                main_step(3 + i)
            ctx.batch_sync(); torch.cuda.synchronize()
            tm = (time.perf_counter() - tm) / KM
            legs["gpu_main_sequence"] = {"what": "the GPU main's per-frame sequence (VISystemGPU::AddFrameGPU, src/VISystemGPU.cpp:137-175) for every frame of a batch: half pyramid, "
                                                 "ORB detect + describe, knn + filters against the previous frame, Scharr gradients, patch points, Gauss-Newton alignment "
                                                 "(the pose estimator that main calls, instead of the essential-matrix RANSAC of the headline); frames resident in HBM",
                                         "ms_per_step": tm * 1e3, "frames_per_s": B / tm, "frames_per_step": B}
            del gray, gxb, gyb, gb, outb
        except Exception as e:                            # never let a side measurement break the contract line
            aux["gradient_batch_or_align"] = {"error": repr(e)}
        # N3: the same pipeline fed from pinned HOST memory through the double-buffered feeder -- the PCIe-inclusive rate
        try:
            hostf = stream.host(min(B * R, 2 * B))
            feed = vislam.Feeder(ctx, W, H, B)
            for k in range(2):
                feed.host_buffer(k)[:] = hostf[(k % R) * B:(k % R + 1) * B]
            def fed_step(i):
                k = i & 1
                feed.host_buffer(k)                       # waits until the previous copy out of this buffer is done
                d = feed.submit(k, B)
                ctx.batch_run(d, B, a.stages)
                feed.release(k)
            ctx.batch_reset()
            for i in range(4):
                fed_step(i)
            ctx.batch_sync(); torch.cuda.synchronize()
            tf = time.perf_counter()
            KF = 20
            for i in range(KF):
                fed_step(i)
            ctx.batch_sync(); torch.cuda.synchronize()
            tf = (time.perf_counter() - tf) / KF
            aux["host_fed_pipeline"] = {"what": "same step, frames copied from pinned host memory by the double-buffered feeder (H2D overlapped with compute)",
                                        "frames_per_s": B / tf, "ms_per_step": tf * 1e3, "h2d_GBps": B * W * H / tf / 1e9}
            feed.close()
            del hostf
        except Exception as e:
            aux["host_fed_pipeline"] = {"error": repr(e)}

    px = None
    if rank == 0:
        ws, hs, sc, q = ctx.level_geometry(W, H)
        px = [int(x) * int(y) for x, y in zip(ws, hs)]
    host_frames = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        host_frames = stream.host(min(B * R, max(400, 6 * usable_cpus()[0] + 8)))
    ctx.close()
    del stream
    torch.cuda.empty_cache()

    # ---- the other configurations BASELINE.json names + the loaded-RANSAC / results-download variants of the headline
    if rank == 0 and legs is not None and world == 1:
        def guarded(name, fn):
            try:
                legs[name] = fn()
            except Exception as e:
                legs[name] = {"error": repr(e)}
        q1 = p.copy(); q1.ransac_adaptive = 0
        guarded("s752_fixed1000", lambda: dict(run_leg(dev, W, H, B, R, q1, vdist.SINGLE_SEED, 4096, 24, 3), pose_kernels=pose_kernels("f1000"),
                what="headline step with ransac_adaptive = 0: 1000 five-point hypotheses per frame pair, every candidate E scored on every match"))
        guarded("s752_parallax", lambda: dict(run_leg(dev, W, H, B, R, p, vdist.SINGLE_SEED, 4096, 60, 3, parallax=True),
                what="S-752P: two depth layers (1.5x parallax) + independently moving objects; adaptive RANSAC, same parameters as the headline"))
        guarded("s752_results_d2h", lambda: dict(run_leg(dev, W, H, B, R, p, vdist.SINGLE_SEED, 4096, 60, 3, d2h=True, want_pose=False),
                what="headline step + D2H of 1024 pose records (192 B), good matches (49 x 16 B) and counts into pinned memory every step, overlapped with the next step"))
        def leg_mispredict():
            """the cost of a WRONG threshold prediction (the headline stream is the most coherent input there is: 0 pairs redone).  Three
            batches of different content alternate -- S-752, the same frames at quarter contrast, uniform noise -- so every step starts
            from thresholds predicted on other content; whatever (frame, level) the prediction was too high for is redone inside the step."""
            ctx = vislam.Context(dev.index or 0, p)
            try:
                Bm = 512
                st = Stream(ctx, dev, W, H, Bm, vdist.SINGLE_SEED)
                low = (st.frames // 4 + 96).contiguous()
                g = torch.Generator(device=dev); g.manual_seed(7)
                noise = torch.randint(0, 256, (Bm, H, W), dtype=torch.uint8, device=dev, generator=g)
                bufs = [st.frames, low, noise]
                ctx.batch_plan(W, H, W, Bm)
                redone, taus = [], []
                def stepm(i):
                    ctx.batch_run(bufs[i % 3].data_ptr(), Bm, vislam.STAGE_FRAME)
                for i in range(3):
                    stepm(i)
                ctx.batch_sync()
                for i in range(3, 9):                       # counted separately from the timing: the read-back syncs
                    stepm(i); ctx.batch_sync()
                    t_, r_ = ctx.batch_fast_thresholds()
                    redone.append(int(r_)); taus.append([int(x) for x in t_])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                K = 12
                for i in range(9, 9 + K):
                    stepm(i)
                ctx.batch_sync(); torch.cuda.synchronize()
                dtm = (time.perf_counter() - t0) / K
                fam_m, _ = family_times(ctx, stepm, 6)
                return {"what": "headline step on alternating incoherent batches (S-752 / quarter contrast / uniform noise, 512 frames each): the "
                                "speculative FAST thresholds are predicted on OTHER content; mispredicted (frame, level) pairs are redone at "
                                "fast_threshold by k_fast_fix / k_select_fix inside the step; consecutive batches are not consecutive frames, so the "
                                "matcher / pose stages see unrelated pairs (their cost is what it is)",
                        "frames_per_step": Bm, "ms_per_step": dtm * 1e3, "frames_per_s": Bm / dtm, "frame_level_pairs_per_step": Bm * LEVELS,
                        "frame_level_pairs_redone_per_step": redone, "tau_next_per_level_after_each_step": taus,
                        "kernels_ms_per_step": {k: round(v, 4) for k, v in fam_m.items()}}
            finally:
                ctx.close()
                torch.cuda.empty_cache()
        guarded("s752_mispredicted_thresholds", leg_mispredict)
        def leg_single_frame():
            """the path the drop-in boundary exists for (/root/reference/src/main_vi_slamGPU.cpp:118-123 -> src/VISystemGPU.cpp:137-175): ONE frame
            per call, handed over in pageable host memory, results handed back to the host -- latency per frame, not batch throughput"""
            import subprocess, tempfile
            ctx = vislam.Context(dev.index or 0, p)
            try:
                cvs = vislam.synth_canvas(2048, vdist.SINGLE_SEED)
                n, warm = 200, 6
                fr = [vislam.synth_frame(cvs, t, W, H, vdist.SINGLE_SEED) for t in range(n + warm + 1)]     # numpy arrays: pageable host memory
                names = ("vis_camera_update", "vis_orb_detect_compute", "vis_good_matches", "vis_essential_ransac", "vis_recover_pose")
                per = {k: [] for k in names}
                tot, trace = [], []
                k_prev, _ = ctx.orb_detect_compute(fr[0], slot=0)
                c0 = None
                for t in range(1, n + warm + 1):
                    if t == warm + 1:
                        per = {k: [] for k in names}; tot = []; trace = []; c0 = ctx.debug_counters()
                    cc0 = ctx.debug_counters()
                    ts = [time.perf_counter()]
                    ctx.camera_update(fr[t]); ts.append(time.perf_counter())
                    k_cur, _d = ctx.orb_detect_compute(fr[t], slot=t & 1); ts.append(time.perf_counter())
                    g, _s = ctx.good_matches((t - 1) & 1, t & 1); ts.append(time.perf_counter())
                    p1 = np.stack([k_prev["x"][g["queryIdx"]], k_prev["y"][g["queryIdx"]]], 1)
                    p2 = np.stack([k_cur["x"][g["trainIdx"]], k_cur["y"][g["trainIdx"]]], 1)
                    tb = time.perf_counter()
                    E, _m, _ni, _it = ctx.essential_ransac(p1, p2); te = time.perf_counter()
                    ctx.recover_pose(E, p1, p2); tr = time.perf_counter()
                    for k, dt_ in zip(names, (ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2], te - tb, tr - te)):
                        per[k].append(dt_ * 1e3)
                    tot.append((ts[3] - ts[0] + tr - tb) * 1e3)
                    cc1 = ctx.debug_counters()
                    trace.append((len(tot) - 1, tot[-1], [per[k][-1] for k in names], cc1[0] - cc0[0], cc1[1] - cc0[1], cc1[2] - cc0[2], len(g)))
                    k_prev = k_cur
                c1 = ctx.debug_counters()
                pct = lambda v, q: float(np.percentile(np.array(v), q))
                out = {"what": "per frame, from pageable host memory through the C ABI (ctypes): vis_camera_update + vis_orb_detect_compute + vis_good_matches "
                               "(knn both directions + filters) + vis_essential_ransac + vis_recover_pose, 752x480 / N = 1000, 200 consecutive S-752 frames; every "
                               "call returns its results to the host.  Includes the ctypes / numpy wrapper (result arrays are allocated per call).  A 20 Hz camera "
                               "leaves 50 ms per frame; the CPU oracle needs 1000 / cpu_baseline.value ms",
                       "frames": n, "ms_per_frame_p50": pct(tot, 50), "ms_per_frame_p95": pct(tot, 95), "ms_per_frame_p99": pct(tot, 99),
                       "ms_per_frame_max": float(np.max(tot)), "slowest_frame_index": int(np.argmax(tot)), "ms_per_frame_mean": float(np.mean(tot)),
                       "ms_max_per_entry_point": {k: float(np.max(v)) for k, v in per.items()},
                       "slowest_call_index_per_entry_point": {k: int(np.argmax(v)) for k, v in per.items()},
                       # the five slowest frames: which entry point the time went to and what the frame did (launches / host waits / copies)
                       "slowest_frames": [{"index": i_, "ms": round(m_, 4), "ms_per_entry_point": {k: round(x, 4) for k, x in zip(names, e_)}, "launches": int(l_),
                                           "host_waits": int(w_), "copies": int(c_), "good_matches": int(g_)}
                                          for i_, m_, e_, l_, w_, c_, g_ in sorted(trace, key=lambda r_: -r_[1])[:5]],
                       "frames_per_s_one_at_a_time": 1e3 / float(np.mean(tot)),
                       "ms_p50_per_entry_point": {k: pct(v, 50) for k, v in per.items()}, "ms_p95_per_entry_point": {k: pct(v, 95) for k, v in per.items()},
                       "kernel_launches_per_frame": (c1[0] - c0[0]) / n, "host_waits_per_frame": (c1[1] - c0[1]) / n, "async_copies_per_frame": (c1[2] - c0[2]) / n,
                       "host_waits_per_entry_point": 1}
            finally:
                ctx.close()
                torch.cuda.empty_cache()
            # the reference's own call: VISystemGPU::AddFrameGPU on the adapter classes (C++, cv::Mat in pageable memory)
            exe = os.path.join(ROOT, "vi-slam_amd", "lib", "addframe_bench")
            try:
                with tempfile.NamedTemporaryFile("w", suffix=".xml", delete=False) as f:
                    f.write(CAL_XML)
                r = subprocess.run([exe, f.name, "200", "6"], capture_output=True, text=True, timeout=300)
                os.unlink(f.name)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                out["add_frame_gpu"] = dict(json.loads(line[-1]), what="VISystemGPU::AddFrameGPU per call on the adapter classes (vi-slam_amd/host/addframe_bench.cpp): Camera::Update, "
                                            "detect + describe, knn + filters against the last keyframe, Scharr gradients, patch points, Gauss-Newton alignment, Track") if line \
                    else {"error": (r.stdout + r.stderr)[-400:]}
            except Exception as e:
                out["add_frame_gpu"] = {"error": repr(e)}
            return out
        guarded("single_frame_api", leg_single_frame)
        q3 = vislam.default_params()
        q3.nfeatures, q3.nlevels, q3.w_size, q3.h_size = 4000, 4, 1920, 1080
        q3.fy = q3.fx
        q3.ransac_adaptive, q3.ransac_max_iters, q3.pose_input = 0, 2000, 1
        def leg3():
            r = run_leg(dev, 1920, 1080, 128, 2, q3, 0xE0C00003, 8192, 24, 2)
            r["pose_kernels"] = pose_kernels("c3")
            r["matcher_roofline"] = matcher_roofline(r["kernels_ms_per_step"]["ms_knn"], 4000, 127, counters="c3")
            r["detect_counters"] = leg_detect_counters("c3", r, 128)
            return r
        guarded("config3_s1080", lambda: dict(leg3(),
                what="BASELINE configs[2]: 1920x1080, 4-level pyramid, 4000 kps/frame, 4000x4000 knn both directions, essential RANSAC with a FIXED "
                     "2000 iterations on the un-gridded symmetric matches (pose_input = SYM) + recoverPose; 128 frames per step"))
        q5 = vislam.default_params()
        q5.nfeatures, q5.nlevels, q5.w_size, q5.h_size = 8000, 8, 3840, 2160
        q5.fy = q5.fx
        def leg5():
            r = run_leg(dev, 3840, 2160, 32, 2, q5, 0xE0C00005, 8192, 40, 2)
            n5 = 8000
            kn = r["kernels_ms_per_step"]["ms_knn"]
            r["matcher"] = {"pairs_per_distance_matrix": n5 * n5, "valu_lane_ops_per_matrix": 16 * n5 * n5,
                            "distance_matrices_per_s": 32 / (kn * 1e-3) if kn > 0 else None,
                            "equivalent_popcount_lane_ops_per_s": 16.0 * n5 * n5 * 32 / (kn * 1e-3) if kn > 0 else None,
                            "note": "the kernel computes TWO 8000 x 8000 matrices per pair (query->train and the transposed one, each reduced row-wise to its "
                                    "top-2), as the reference's two knnMatch calls do; the RATE reported here counts one matrix per pair, the unit SURVEY 8(d) "
                                    "prices (16 N1 N2 xor+popcount lane-ops); computed on the FP4 matrix cores (e2m1 +-1, exact)"}
            r["matcher_roofline"] = matcher_roofline(kn, n5, 31, counters="c5")
            r["detect_counters"] = leg_detect_counters("c5", r, 32)
            r["what"] = "BASELINE configs[4]: 3840x2160, 8 levels, 8000 kps/frame, 8000x8000 BF-Hamming all-pairs, filters, pose; 32 frames per step"
            return r
        guarded("config5_s2160", leg5)

    if rank == 0:
        alg = algorithmic_bytes(px, NFEAT)
        fam_bytes = {"ms_fast": ("k_fast", alg["k_fast"], launches_fast), "ms_pyramid": ("k_resize", alg["k_resize"], LEVELS - 1),
                     "ms_describe": ("k_describe", alg["k_describe"], 1)}
        dom = max(fam_bytes, key=lambda k: fam[k])
        kname, bytes_per_frame, nlaunch = fam_bytes[dom]
        per_launch_bytes = bytes_per_frame * B / nlaunch
        per_launch_s = fam[dom] * 1e-3 / nlaunch
        achieved = per_launch_bytes / per_launch_s / 1e9
        # Counter-side figures come from the committed rocprofv3 --pmc passes (tools/final_profile.sh -> tools/pmc_summarize.py ->
        # profiles/pmc_traffic.json: FETCH_SIZE / WRITE_SIZE in separate runs with the gfx950 FETCH_SIZE correction calibrated on
        # a 256 MiB copy, SQ instruction counts, LDS conflict cycles, and the VALU issue ceilings tools/valu_peak.hip measured in
        # the same lease), taken at pj["batch_frames"] frames per launch and scaled linearly to this run's batch; the TIMES are
        # this run's HIP events.  A missing or stale file is reported in the line, never silently skipped.
        traffic, valu, detect_kernels, pmc_commit, limited_by = None, None, None, None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        try:
            pj = json.load(open(pmc))
            pmc_commit = pj.get("measured_at_commit")
            scale = B / pj["batch_frames"]
            peaks = pj["valu_peak_measured"]
            detect_kernels = {}
            fam_of = {"k_fast": ("ms_fast", launches_fast, alg["k_fast"]), "k_resize": ("ms_pyramid", LEVELS - 1, alg["k_resize"]),
                      "k_describe": ("ms_describe", 1, alg["k_describe"]), "k_select": ("ms_select", 1, None)}
            for kn, (fk, nl, ab) in fam_of.items():
                r = pj[kn]
                t = fam[fk] * 1e-3                                   # all launches of the family, this run
                calls = nl                                           # per-launch counter means x launches of the family
                vi = r["valu_wave_insts_per_launch"] * scale * calls
                hbm = r["hbm_bytes_per_launch"] * scale * calls
                d = {"ms": round(fam[fk], 4), "launches": nl,
                     "hbm_traffic_bytes": hbm, "hbm_traffic_frac": hbm / t / 1e9 / HBM_PEAK_GBS,
                     "valu_wave_insts": vi, "valu_issue_frac": vi / t / SIMD_ISSUE_PEAK,
                     "valu_frac_of_half_rate_ceiling": vi / t / peaks["half_rate_class"],
                     "valu_frac_of_full_rate_ceiling": vi / t / peaks["full_rate_class"],
                     "salu_wave_insts": (r.get("salu_wave_insts_per_launch") or 0) * scale * calls,
                     "lds_bank_conflict_cycles": (r.get("lds_bank_conflict_cycles") or 0) * scale * calls,
                     # fraction of the launch during which a CU's LDS array is busy (SQ_LDS_IDX_ACTIVE / CU-cycles of the counter run)
                     "lds_busy_frac": r.get("lds_busy_frac")}
                if ab is not None:
                    d["algorithmic_bytes"] = ab * B
                    d["hbm_frac"] = ab * B / t / 1e9 / HBM_PEAK_GBS
                    d["traffic_over_algorithmic"] = hbm / (ab * B)
                # what the counters say limits the kernel: the larger of (HBM traffic / peak) and (VALU issue / measured ceiling of
                # the half-rate class, the class most of these kernels' instructions belong to) -- or the LDS array, when that is busier
                d["limited_by"] = "valu-issue" if d["valu_frac_of_half_rate_ceiling"] > d["hbm_traffic_frac"] else "hbm"
                if (d["lds_busy_frac"] or 0) > max(d["valu_frac_of_half_rate_ceiling"], d["hbm_traffic_frac"]):
                    d["limited_by"] = "lds"
                elif (d["lds_busy_frac"] or 0) >= 0.85 and d["limited_by"] == "valu-issue":
                    # round 4: k_describe's LDS array is busy ~90 % of the launch (57 % of that bank conflicts of the sample gathers) while vector
                    # issue sits at its half-rate ceiling: removing a fifth of its vector instructions moved it by 2 % (DESIGN_history.md section 4, Round 4)
                    d["limited_by"] = "lds + valu-issue"
                detect_kernels[kn] = d
            dk = detect_kernels[kname]
            traffic = pj[kname]["hbm_bytes_per_launch"] * scale
            limited_by = dk["limited_by"]
            valu = {"kernel": kname, "wave_insts_per_launch": dk["valu_wave_insts"] / nlaunch, "achieved": dk["valu_wave_insts"] / (fam[dom] * 1e-3),
                    "unit": "wave-instr/s", "peak_issue": SIMD_ISSUE_PEAK, "frac_of_issue_peak": dk["valu_issue_frac"],
                    "peak_measured_half_rate_class": peaks["half_rate_class"], "frac_of_half_rate_ceiling": dk["valu_frac_of_half_rate_ceiling"],
                    "peak_measured_full_rate_class": peaks["full_rate_class"], "frac_of_full_rate_ceiling": dk["valu_frac_of_full_rate_ceiling"],
                    "peak_measured_by": peaks.get("what"), "pmc_measured_at_commit": pmc_commit,
                    "note": "instruction counts from the committed SQ_INSTS_VALU pass (same kernels, same workload, other run); "
                            "times from this run; a kernel made of both instruction classes sits between the two measured ceilings"}
        except Exception as e:                                  # loud: the record says what is missing
            valu = {"error": f"profiles/pmc_traffic.json unusable: {e!r}"}
        # the bound that explains the headline: every vector instruction of the step (all kernels, counter passes) against the time a step takes
        issue = None
        try:
            pj2 = json.load(open(pmc))
            st_ = pj2["step"]
            vi_launch = st_["valu_wave_insts_per_step"] * (B / pj2["batch_frames"])
            t_launch = dt / a.steps / Q
            pk = pj2["valu_peak_measured"]
            issue = {"what": "whole step: sum of SQ_INSTS_VALU over every kernel of one launch of frames_per_launch frames (committed counter passes, scaled "
                             "linearly from their batch) / this run's time per launch", "valu_wave_insts_per_launch": vi_launch,
                     "salu_wave_insts_per_launch": st_["salu_wave_insts_per_step"] * (B / pj2["batch_frames"]),
                     "ms_per_launch": t_launch * 1e3, "achieved": vi_launch / t_launch, "unit": "wave-instr/s",
                     "peak_measured_half_rate_class": pk["half_rate_class"], "peak_measured_full_rate_class": pk["full_rate_class"],
                     "frac_of_half_rate_ceiling": vi_launch / t_launch / pk["half_rate_class"], "frac_of_full_rate_ceiling": vi_launch / t_launch / pk["full_rate_class"],
                     "frac": vi_launch / t_launch / pk["half_rate_class"], "valu_wave_insts_per_kernel_at_pmc_batch": st_["valu_wave_insts_per_kernel"],
                     "pmc_measured_at_commit": pmc_commit}
        except Exception as e:
            issue = {"error": f"profiles/pmc_traffic.json has no step totals: {e!r}"}
        out = {
            **headline(a, world, B, Q, dt, ranks),
            "clocks": clocks.summary(),
            # `bound` names the roofline `frac` is priced against (north_star asks for the HBM roofline of detect/describe);
            # `limited_by` is what the counters say actually limits this kernel (see valu_roofline / detect_kernels)
            "roofline": {"bound": "hbm", "limited_by": limited_by, "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "algorithmic_bytes_per_launch": per_launch_bytes, "avg_launch_ms": per_launch_s * 1e3},
            "valu_roofline": valu,
            "issue_roofline": issue,
            "fast_threshold_prediction": {"tau_next_per_level": [int(x) for x in tau_next], "fast_threshold": int(p.fast_threshold),
                                          "frame_level_pairs_redone_in_the_last_step": int(redone),
                                          "what": "thresholds the next batch's k_fast starts from (min over the last batch's frames of the "
                                                  "retainBest(2*quota) cut per level, minus 4); 0 pairs redone = every prediction of the last step held"},
            "detect_kernels": detect_kernels,
            "matcher_roofline": matcher_roofline(fam["ms_knn"], NFEAT, B),
            "pose_load": headline_pose,
            "aux_kernels": aux,
            "legs": legs,
            "kernels_ms_per_step": {k: round(v, 4) for k, v in fam.items()},       # per LAUNCH of frames_per_launch frames (one batch in flight)
            "kernels_ms_per_launch": {k: round(v, 4) for k, v in fam.items()},
            "detect_describe_GBps": alg["total_detect_describe"] * B / ((fam["ms_pyramid"] + fam["ms_fast"] + fam["ms_select"] + fam["ms_describe"]) * 1e-3) / 1e9,
        }
        if host_frames is not None:
            out["cpu_baseline"] = cpu_baseline(p, host_frames, 10.0, "752x480, N=1000, 8 levels: BASELINE configs[1]")
            p200 = p.copy(); p200.nfeatures = 200
            out["cpu_baseline_config1"] = cpu_baseline(p200, host_frames[:203], 8.0, "752x480, ORB::create(200) as the reference CPU main, src/Camera.cpp:127: "
                                                       "BASELINE configs[0], synthetic stand-in for EuRoC MH_01 which is not in the image")
            # the same port frame-parallel on ALL host cores (OpenCV itself would run TBB inside its calls);
            # informational, `cpu_baseline` stays the single-thread figure of the reference's own single-threaded code
            try:
                import oracle_bind as orc
                th, quota = usable_cpus()
                best = None
                for tt in sorted({th, min(th, 16)}):         # all usable threads, and the documented 16-core share of one GPU
                    ns = min(len(host_frames), max(48, 6 * tt))
                    sec, _ = orc.pipeline_stream_mt(p, host_frames[:ns], tt)
                    cand = {"value": ns / sec, "unit": "frames/s", "cores": tt, "kind": "port",
                            "sample": f"{ns} consecutive S-752 frames, frame-parallel std::thread pool over the same oracle pipeline on {tt} threads "
                                      f"(nproc = {os.cpu_count()}, affinity = {len(os.sched_getaffinity(0))}, cgroup cpu quota = {quota})"}
                    if best is None or cand["value"] > best["value"]:
                        best = cand
                out["cpu_baseline_multicore"] = best
            except Exception as e:
                out["cpu_baseline_multicore"] = {"error": repr(e)}
        # the full record goes to a FILE (and nowhere on stdout: BENCH_r05.json could not parse the 23 KB line of round 5); the LAST line of
        # stdout is the compact strict-JSON line of benchline.py, numbers only, < 1900 bytes
        full_path = a.full_out
        if full_path is None:
            d_ = os.path.join(ROOT, "gpurun_out")
            try:
                os.makedirs(d_, exist_ok=True)
                full_path = os.path.join(d_, "bench_full.json")
            except OSError:
                full_path = os.path.join(ROOT, "bench_full.json")
        try:
            with open(full_path, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        except OSError as e:
            print(f"bench.py: could not write the full record to {full_path}: {e!r}", file=sys.stderr)
            full_path = None
        import benchline
        print(benchline.compact_line(out, os.path.relpath(full_path, ROOT) if full_path else None), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
