"""The compact LAST line of bench.py (benchline.py): short enough for a 2000-byte tail, strict JSON, the contract keys present.
BENCH_r05.json: the driver could not parse round 5's 23 KB line (`parsed: null`); the CPU half of this file runs the formatter on every
committed full record, the GPU half on the real stdout of a short bench run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchline  # noqa: E402


def strict(s):
    def bad(x):
        raise ValueError(f"non-finite constant {x} in the line")
    return json.loads(s, parse_constant=bad)


def check_line(s, full):
    assert "\n" not in s and len(s.encode()) < 1900, len(s.encode())
    c = strict(s)
    for k in benchline.REQUIRED:
        if k in full:
            assert k in c, k
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "scaling", "dtype", "data", "higher_is_better", "vs_baseline"):
        assert c[k] == full[k], k
    assert abs(c["value"] - full["value"]) <= 1e-5 * full["value"] and abs(c["ms_per_step"] - full["ms_per_step"]) <= 1e-5 * full["ms_per_step"]
    assert set(c["config"]) >= {"workload", "parallelism"} and len(c["config"]["workload"]) <= 200 and "model" not in c["config"]
    r = c["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # numbers only below the top level: no prose fields
    for blk in ("roofline", "issue_roofline", "matcher_roofline", "t1", "legs", "latency_ms", "clocks", "aux", "ms"):
        for k, v in (c.get(blk) or {}).items():
            assert v is None or isinstance(v, (int, float)) or k in ("bound", "kernel", "unit", "limited_by"), (blk, k, v)
    return c


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench*.json"))))
def test_committed_records_format(path):
    txt = open(path).read()
    full = strict(txt if txt.lstrip().startswith("{") else [l for l in txt.splitlines() if l.startswith("{")][-1])
    if "full" in full and len(txt) < 2500:
        # a committed COMPACT line (the stdout of a bench run, profiles/r06_bench.json): it must itself satisfy the contract, and the full
        # record it names travels beside it
        c = check_line(txt.strip(), full)
        assert c["roofline"]["kernel"].startswith("k_") and c["cpu_baseline"]["kind"] == "port" and c["t1"]["target"] == 0.4
        beside = os.path.join(os.path.dirname(path), os.path.basename(path).replace(".json", "_full.json"))
        assert os.path.exists(beside), beside
        fr = strict(open(beside).read())
        assert abs(fr["value"] - c["value"]) <= 1e-5 * fr["value"] and benchline.compact_line(fr, c["full"]) == txt.strip()
        return
    c = check_line(benchline.compact_line(full, "gpurun_out/bench_full.json"), full)
    if "cpu_baseline" in full:
        assert c["cpu_baseline"]["kind"] in ("port", "reference") and c["cpu_baseline"]["cores"] >= 1 and len(c["cpu_baseline"]["sample"]) <= 80
    if "detect_kernels" in full and full["detect_kernels"]:
        assert c["t1"]["target"] == 0.4 and c["t1"]["k_describe_frac"] is not None


def test_eight_ranks_and_every_block_fit():
    full = strict(open(os.path.join(ROOT, "profiles", "r05_bench.json")).read())
    full["n_gpus"] = 8
    full["ranks"] = [dict(full["ranks"][0], rank=i, device=i) for i in range(8)]
    full["clocks"] = {"sclk_mhz": 2345.0, "mclk_mhz": 2000.0, "watts": 1255.5, "samples": 9, "source": "x"}
    sf = full["legs"]["single_frame_api"]
    sf.update(ms_per_frame_p99=1.234, ms_per_frame_max=31.23)
    sf["add_frame_gpu"].update(ms_p99=2.25, ms_max=3.31)
    c = check_line(benchline.compact_line(full, "gpurun_out/bench_full.json"), full)
    assert len(c["ranks"]) == 8 and c["roofline"] and c["cpu_baseline"]            # the contract blocks survive whatever is dropped


def test_non_finite_values_become_null_and_overflow_is_an_error():
    full = strict(open(os.path.join(ROOT, "profiles", "r05_bench.json")).read())
    full["roofline"]["traffic"] = float("nan")
    full["legs"]["config3_s1080"]["frames_per_s"] = float("inf")
    c = strict(benchline.compact_line(full))
    assert c["roofline"]["traffic"] is None and c["legs"]["c3"] is None
    with pytest.raises(ValueError):
        benchline.compact_line(full, limit=300)


@pytest.mark.gpu
def test_real_bench_stdout_is_one_compact_line(built, tmp_path):
    fp = tmp_path / "full.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--launches-per-step", "4", "--full", "--no-legs",
                        "--no-cpu-baseline", "--full-out", str(fp)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = r.stdout.rstrip("\n").splitlines()
    assert out and out[-1].startswith("{") and sum(l.startswith("{") for l in out) == 1, r.stdout[-2000:]
    full = strict(open(fp).read())
    c = check_line(out[-1], full)
    assert c["roofline"]["kernel"].startswith("k_") and c["t1"]["chain_frac"] > 0 and c["clocks"] is not None
    assert c["ranks"][0][:2] == [0, 0]


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(orc, tmp_path):
    """a plain run (no --full): the headline fields alone, --steps timed steps; --dump-outputs writes the same arrays on every run, and
    they are what the oracle computes for the frames of the last timed launch (keypoints, descriptors, half pyramid, good matches, pose)"""
    def run(d):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--launches-per-step", "2",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        out = r.stdout.rstrip("\n").splitlines()
        assert out and sum(l.startswith("{") for l in out) == 1 and out[-1].startswith("{"), r.stdout[-2000:]
        return strict(out[-1])
    c = run(tmp_path / "a")
    assert c["metric"] == "frames/sec detect+match+pose, 752x480 mono8" and c["unit"] == "frames/s" and c["higher_is_better"] is True and c["dtype"] == "u8"
    assert c["steps"] == 3 and c["warmup"] == 1 and c["ms_per_step"] > 0 and c["config"]["frames_per_step_per_gpu"] == 2048
    assert abs(c["value"] - 2048 / (c["ms_per_step"] * 1e-3)) <= 1e-4 * c["value"]
    for k in ("roofline", "cpu_baseline", "legs", "ms", "clocks", "full"):                # measured only with --full
        assert k not in c, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"pose_E.npy", "pose_R.npy", "pose_t.npy", "good_count.npy", "keypoints.npy", "descriptors.npy", "half_pyramid.npy",
            "sample_stream_frames.npy"} <= set(names), names
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["pose_E"].shape == (1024, 9) and a["good_count"].shape == (1024,) and a["good_count"].max() > 0 and len(a["keypoints"]) > 0
    # the last timed launch: step warmup + steps - 1 = 3 of a ring of 2 steps of 2 launches -> its second launch, stream frames 3072 ...
    first = ((1 + 3 - 1) % 2 * 2 + 1) * 1024
    sample = np.unique(a["keypoints"][:, 0]).astype(np.int64)
    assert len(sample) == 16 and (a["sample_stream_frames"] == first + sample).all()
    f = int(sample[sample > 0][0])                                                        # a sampled frame with its predecessor in the launch
    import vislam
    from vislam import dist as vdist
    p = vislam.default_params()
    p.nfeatures, p.nlevels, p.w_size, p.h_size = 1000, 8, 752, 480                        # bench.py's headline parameters
    p.fy = p.fx
    cv = vislam.synth_canvas(4096, vdist.SINGLE_SEED)
    img0, img1 = (vislam.synth_frame(cv, first + f + d, 752, 480, vdist.SINGLE_SEED) for d in (-1, 0))
    k0, d0 = orc.orb_detect_compute(p, img0)
    k1, d1 = orc.orb_detect_compute(p, img1)
    r1 = orc.pipeline_frame(p, img1, orc.pipeline_frame(p, img0)[:2])[2]                # the per-frame pipeline: matches + pose of the pair
    rows = a["keypoints"][:, 0] == f
    assert rows.sum() == len(k1) > 0 and (a["keypoints"][rows, 1:] == np.stack([k1[n].astype(np.float32) for n in vislam.KEYPOINT_DTYPE.names], 1)).all()
    assert (a["descriptors"][rows] == d1).all()
    half = np.concatenate([lv.reshape(-1) for lv in orc.half_pyramid(img1)[1:5]]).astype(np.float32)
    assert (a["half_pyramid"][list(sample).index(f)] == half).all()
    o12, o21 = orc.knn2_hamming(d0, d1)
    og, _ = orc.good_matches(p, k0, k1, o12, o21)
    n = len(og)
    assert a["good_count"][f] == n == r1.n_good > 0 and (a["good_query"][f, n:] == -1).all()
    assert (a["good_query"][f, :n] == og["queryIdx"]).all() and (a["good_train"][f, :n] == og["trainIdx"]).all()
    assert (a["good_distance"][f, :n] == og["distance"]).all()
    assert a["pose_counts"][f, 0] == r1.n_inliers and a["pose_counts"][f, 2] == r1.iters_run
    if r1.n_inliers:
        assert a["pose_counts"][f, 1] == r1.n_pose_good
        oE = np.array(r1.E)
        s = 1.0 if float((a["pose_E"][f] * oE).sum()) >= 0 else -1.0
        assert np.abs(a["pose_E"][f] - s * oE).max() <= 1e-9
        assert np.abs(a["pose_R"][f] - np.array(r1.R)).max() <= 1e-7 and np.abs(a["pose_t"][f] - np.array(r1.t)).max() <= 1e-7
    run(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == names
    for name in a:                                                                        # same arguments: same inputs, same outputs
        assert np.array_equal(a[name], np.load(tmp_path / "b" / (name + ".npy"))), name
