"""Inputs shared by tests/test_align_weights_ref.py (CPU: the restatement against the oracle) and tests/test_align_weights_gpu.py (the
library against the restatement): every single-pair case the GPU tests run is built here, so that the CPU test can show the restatement
equal to the oracle, with identity weights, on exactly those inputs."""
import numpy as np

import align_cases

FIXED_K = (200.0, 200.0)          # fx, fy of the small cases; cx, cy = the image centre


class Case:
    def __init__(self, name, w, h, c, first=3, last=0, iters=10, init6=None):
        self.name, self.w, self.h, self.c = name, w, h, c
        self.first, self.last, self.iters, self.init6 = first, last, iters, init6

    def params(self, mod):
        """mod = vislam or the oracle binding: its default alignment parameters with this case's intrinsics and options"""
        ap = mod.default_align_params()
        ap.fx, ap.fy, ap.cx, ap.cy = FIXED_K[0], FIXED_K[1], self.w / 2.0, self.h / 2.0
        ap.first_level, ap.last_level, ap.max_iterations = self.first, self.last, self.iters
        return ap

    def init(self, orc):
        return None if self.init6 is None else orc.se3_exp(self.init6)

    def levels(self):
        c = self.c
        return c["gray1"], c["gray2"], c["gx"], c["gy"], c["cand"]


def with_frame2(orc, c, f1):
    """the case with another second frame (its half pyramid; frame 1, its gradients and the candidates stay)"""
    d = dict(c)
    d["f1"] = f1
    d["gray2"] = orc.half_pyramid(f1)
    return d


def occlude(orc, c):
    """frame 2 with a rectangle of 255 from the top-left corner to the median keypoint: about a quarter of the patches"""
    f1 = c["f1"].copy()
    mx, my = int(np.median(c["kps"]["x"])), int(np.median(c["kps"]["y"]))
    f1[:my, :mx] = 255
    d = with_frame2(orc, c, f1)
    inside = (c["kps"]["x"] < mx) & (c["kps"]["y"] < my)
    d["occluded_fraction"] = float(inside.mean())
    return d


def from_frames(orc, f0, f1, kps, w, h, div=8):
    l0, l1 = orc.half_pyramid(f0), orc.half_pyramid(f1)
    gx, gy = [], []
    for lv in l0:
        a, b, _ = orc.scharr_gradient(lv, 3)
        gx.append((a // div).astype(np.int16)); gy.append((b // div).astype(np.int16))
    return dict(gray1=l0, gray2=l1, gx=gx, gy=gy, cand=[orc.patch_points(kps, w, h, l) for l in range(5)], kps=kps, f0=f0, f1=f1)


def truncated(c, n):
    d = dict(c)
    d["cand"] = [a[:n].copy() for a in c["cand"]]
    return d


_cache = {}


def single_cases(vislam, orc, canvas):
    """name -> Case; built once per session"""
    if "single" in _cache:
        return _cache["single"]
    out = {}
    clean = align_cases.case(vislam, orc, canvas, w=320, h=240, dx=2, dy=1, n=49, grad_div=8)
    out["clean_320"] = Case("clean_320", 320, 240, clean)
    out["occluded_320"] = Case("occluded_320", 320, 240, occlude(orc, clean))
    odd = align_cases.case(vislam, orc, canvas, w=150, h=110, dx=1, dy=1, n=20, grad_div=8)
    out["clean_150x110"] = Case("clean_150x110", 150, 110, odd)              # 150 x 110 does not halve exactly
    out["occluded_150x110"] = Case("occluded_150x110", 150, 110, occlude(orc, odd))
    out["init_levels_2_1"] = Case("init_levels_2_1", 320, 240, clean, first=2, last=1, iters=4, init6=[0.002, -0.001, 0, 0, 0, 0.001])
    out["init_level_0"] = Case("init_level_0", 320, 240, occlude(orc, clean), first=0, last=0, iters=25, init6=[0.01, 0.01, 0, 0, 0, 0])
    for n in (1, 255, 256, 257, 1024, 1025):                                 # the lane and four-per-thread round boundaries
        out[f"list_{n}"] = Case(f"list_{n}", 320, 240, truncated(out["occluded_320"].c, n))
    z = dict(clean)
    z["cand"] = []
    for a in clean["cand"]:
        a = a.copy()
        a[:, 2] = 0.5 + 0.25 * (np.arange(len(a)) % 7)                       # z = 0.5 ... 2.0
        z["cand"].append(a)
    out["z_not_1"] = Case("z_not_1", 320, 240, z, init6=[0.004, -0.003, 0.01, 0, 0, 0.002])
    # frame 2 = 255 where frame 1 = 0 and the reverse: residuals of -255 and +255, both ends of MedianMat's saturation
    f0 = np.where(clean["f0"] >= np.median(clean["f0"]), 255, 0).astype(np.uint8)
    bw = from_frames(orc, f0, (255 - f0).astype(np.uint8), clean["kps"], 320, 240)
    out["inverted"] = Case("inverted", 320, 240, bw)
    dark = f0.copy(); dark[:, :200] = 0                                        # mostly -255 (frame 1 bright, frame 2 black) ...
    out["mostly_minus_255"] = Case("mostly_minus_255", 320, 240, from_frames(orc, np.full_like(f0, 255) - dark // 4, dark, clean["kps"], 320, 240))
    out["mostly_plus_255"] = Case("mostly_plus_255", 320, 240, from_frames(orc, dark, np.full_like(f0, 255), clean["kps"], 320, 240))
    _cache["single"] = out
    return out


# weight settings the single-pair GPU test runs every case under: (mode, tukey_b, mad_scale)
DEFAULTS = (4.6851, 1.4826)
SETTINGS = [(1,) + DEFAULTS, (2,) + DEFAULTS]
CUSTOM = [(1, 2.5, 1.0), (2, 3.0, 2.0)]                                        # run on clean_320 and occluded_320


def generated_case(vislam, orc, canvas):
    """vis_align_batch: 4 frames of 320 x 240, 200 matched points for pairs 1 and 2 with every patch inside the frame (200 x 121 = 24 200
    candidates at level 0, the most the generated path holds) and 3 points for pair 3; frame 2 carries an occluder"""
    if "gen" in _cache:
        return _cache["gen"]
    W, H, n = 320, 240, 4
    cv = vislam.synth_canvas(1024, 5)
    frames = np.stack([vislam.synth_frame(cv, t, W, H, 5) for t in range(n)])
    frames[2, 40:140, 60:200] = 255
    rng = np.random.default_rng(11)
    max_pts = 200
    pts = np.zeros((n, max_pts, 2), np.float32)
    pts[..., 0] = rng.uniform(8, W - 9, (n, max_pts)); pts[..., 1] = rng.uniform(8, H - 9, (n, max_pts))
    npts = np.array([0, 200, 200, 3], np.int32)
    pairs = {}
    for t in range(1, n):
        kp = np.zeros(npts[t], vislam.KEYPOINT_DTYPE); kp["x"], kp["y"] = pts[t, :npts[t], 0], pts[t, :npts[t], 1]
        l0, l1 = orc.half_pyramid(frames[t - 1]), orc.half_pyramid(frames[t])
        gx, gy = [], []
        for lv in l0:
            a, b, _ = orc.scharr_gradient(lv, 3)
            gx.append(a); gy.append(b)
        pairs[t] = dict(gray1=l0, gray2=l1, gx=gx, gy=gy, cand=[orc.patch_points(kp, W, H, l) for l in range(5)])
    assert len(pairs[1]["cand"][0]) == 200 * 121
    _cache["gen"] = dict(W=W, H=H, n=n, frames=frames, pts=pts, npts=npts, max_pts=max_pts, pairs=pairs)
    return _cache["gen"]


def same(a, b):
    """bit-exact: pose, matrix, error[], initial_error, iterations[], n_residuals[]"""
    assert list(a.iterations) == list(b.iterations), ("iterations", list(a.iterations), list(b.iterations))
    assert list(a.n_residuals) == list(b.n_residuals), ("n_residuals", list(a.n_residuals), list(b.n_residuals))
    f = lambda v: np.array(list(v), np.float32).tobytes()                     # noqa: E731
    assert f(a.error) == f(b.error), ("error", list(a.error), list(b.error))
    assert f([a.initial_error]) == f([b.initial_error]), ("initial_error", a.initial_error, b.initial_error)
    assert a.pose.as_array().tobytes() == b.pose.as_array().tobytes(), ("pose", a.pose.as_array(), b.pose.as_array())
    assert f(a.matrix) == f(b.matrix), ("matrix", list(a.matrix), list(b.matrix))
