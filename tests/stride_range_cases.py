"""The shapes, strides, candidate counts and inputs that walk Camera::Update's half pyramid, Camera::computeGradient, the patch
builders, the photometric alignment and the tracking chain over padded row strides and both ends of the accepted size range
(16 ... 4095 per side).  Shared by the CPU yardstick (tests/test_stride_range_ref.py: the cases are sound on the oracle alone) and the
GPU tests (tests/test_stride_range_gpu.py), so that both run the same inputs.

  family A  sides 16 ... 24: level 4 is 1 or 2 pixels wide / high (16 -> 8 -> 4 -> 2 -> 1, 19 -> 10 -> 5 -> 2 -> 1, 23 -> 12 -> 6 -> 3 -> 2)
  family B  sides of 4095 / 4094: the 4095 -> 2048 -> 1024 -> 512 -> 256 chain against the bookkeeping 4095 >> 4 = 255
  family C  row strides larger than the width, against the oracle run on the dense frames
  family D  a 64 x 48 pair: candidate counts at the four-per-thread round boundaries, candidate values patch_points never emits
  family E  the patch builders at four (w_size, h_size), 199 / 200 / 201 keypoints on and beside every border
"""
import numpy as np

import align_cases

PAD = 0xA5                       # what the bytes between a row's width and its stride hold
SCALES = (1, 3, 8)
SMALL_SIZES = [(16, 16), (17, 19), (18, 16), (19, 21), (20, 17), (21, 21), (22, 16), (23, 23), (16, 40), (40, 16), (24, 24)]
LARGE_SIZES = [(4095, 16), (16, 4095), (4095, 33), (4094, 18)]
SMALL_N, LARGE_N = 9, 2          # 9: not a multiple of the 8-frame XCD group
# family C, gradients: (width, stride, byte offset of frame 0 inside its allocation); 48 rows
GRAD_H = 48
GRAD_STRIDES = [(64, 64, 0), (64, 68, 0), (64, 80, 0), (64, 96, 0), (64, 80, 4), (72, 72, 0), (72, 76, 0), (70, 72, 0), (70, 76, 0)]
GRAD_N = (1, 8, 9)
ALIGN_STRIDES = (320, 324, 336)  # vis_align_batch on 320 x 240
PLAN_SHAPES = [(320, 336), (318, 320)]       # (w, stride): k_track_snapshot's dword path and its byte path; 240 rows, launches of 8
PLAN_H, PLAN_B, PLAN_LAUNCHES = 240, 8, 3
WEIGHT_MODES = (0, 1, 2)


def min_stride(w):
    return (w + 3) & ~3


def frames_of(kind, w, h, n, seed=1):
    """n different frames: uniform noise, or 0 / 255 checkers with a block size per frame -- blocks of at least 2 x 3 pixels, so that a
    3 x 3 window can hold a whole step edge (the largest Scharr response, 16 * 255 * scale; one-pixel squares give none at all)"""
    if kind == "noise":
        return np.random.default_rng(seed * 1000003 + w * 4099 + h).integers(0, 256, (n, h, w), dtype=np.uint8)
    assert kind == "checker"
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(((xx // (2 + f % 4) + yy // (3 + f // 4) + f) & 1) * 255).astype(np.uint8) for f in range(n)])


def smooth_frame(w, h, seed=0):
    """a frame without fine texture (long waves in both directions plus +-3 of noise): a one-pixel shift of it is a small residual on
    every level, so the Gauss-Newton steps of a pair made from it stay small"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 128 + 45 * np.sin(xx / 23.0 + yy / 31.0 + seed) + 45 * np.cos(yy / 19.0 - xx / 41.0) + 25 * np.sin((xx + yy) / 7.0)
    v += np.random.default_rng(seed * 7919 + w * 4099 + h).integers(-3, 4, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def padded(frames, stride, offset=0):
    """the frames at row stride `stride`, `offset` bytes into a flat buffer; every byte that is not a pixel is PAD"""
    n, h, w = frames.shape
    buf = np.full(offset + n * h * stride, PAD, np.uint8)
    view = buf[offset:].reshape(n, h, stride)
    view[:, :, :w] = frames
    return buf


_grad_cache = {}


def gradient_ref(orc, frame, scale):
    """the oracle on one dense frame -> (half pyramid levels, [(gx, gy, g) per level])"""
    key = (frame.shape, frame.tobytes(), scale)
    if key not in _grad_cache:
        if len(_grad_cache) > 256:
            _grad_cache.clear()
        pyr = orc.half_pyramid(frame)
        _grad_cache[key] = (pyr, [orc.scharr_gradient(lv, scale) for lv in pyr])
    return _grad_cache[key]


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
class Pair:
    """one explicit-list alignment: per-level images, gradients and candidate rows (x, y, z, w), parameters and initial pose"""
    def __init__(self, name, w, h, gray1, gray2, gx, gy, cand, k, first=3, last=0, iters=10, init6=None):
        self.name, self.w, self.h = name, w, h
        self.gray1, self.gray2, self.gx, self.gy, self.cand = gray1, gray2, gx, gy, cand
        self.k, self.first, self.last, self.iters, self.init6 = k, first, last, iters, init6

    def params(self, mod, first=None, last=None, iters=None):
        ap = mod.default_align_params()
        ap.fx, ap.fy, ap.cx, ap.cy = self.k
        ap.first_level = self.first if first is None else first
        ap.last_level = self.last if last is None else last
        ap.max_iterations = self.iters if iters is None else iters
        return ap

    def init(self, orc):
        return None if self.init6 is None else orc.se3_exp(self.init6)

    def levels(self, cand=None):
        return self.gray1, self.gray2, self.gx, self.gy, self.cand if cand is None else cand

    def with_cand(self, name, cand, **kw):
        q = Pair(name, self.w, self.h, self.gray1, self.gray2, self.gx, self.gy, cand, self.k, self.first, self.last, self.iters, self.init6)
        for a, v in kw.items():
            setattr(q, a, v)
        return q


def _levels_of(orc, f0, f1, div):
    l0, l1 = orc.half_pyramid(f0), orc.half_pyramid(f1)
    gx, gy = [], []
    for lv in l0:
        a, b, _ = orc.scharr_gradient(lv, 3)
        gx.append((a // div).astype(np.int16)); gy.append((b // div).astype(np.int16))
    return l0, l1, gx, gy


_cache = {}

# family B, explicit list.  fx = fy = 256 and z = 2^-l on level l make a translation (tx, ty, 0) move every candidate of every level by
# the same 256 * tx pixels (fx_l * tx / z = (256 / 2^l) * tx * 2^l): 1.2 px along the long side, towards the extra column / row, and 0.3 px
# along the short one (a level one row high keeps 0 < y2 < 1).
LARGE_FOCAL, LARGE_SHIFT_LONG, LARGE_SHIFT_SHORT = 256.0, 1.2, 0.3


def large_shift(w, h):
    return (LARGE_SHIFT_LONG, LARGE_SHIFT_SHORT) if w >= h else (LARGE_SHIFT_SHORT, LARGE_SHIFT_LONG)


def large_edge_points(w, h, lvl):
    """candidates in the last valid column (w >= h) or row (h > w) of level `lvl`, (cols - 1 / rows - 1 of the bookkeeping size)"""
    cols, rows = w >> lvl, h >> lvl
    z = 2.0 ** -lvl
    if w >= h:
        return np.array([[cols - 1, y, z, 1] for y in sorted({0, rows // 2, rows - 1})], np.float32)
    return np.array([[x, rows - 1, z, 1] for x in sorted({0, cols // 2, cols - 1})], np.float32)


def large_explicit_pair(orc, w, h):
    """a smooth frame and the same moved by one pixel along its long side; levels 4 ... 0 (every level of these sizes holds a point);
    per level the edge points of large_edge_points, the far corner, the other border and a few interior points"""
    key = ("large", w, h)
    if key in _cache:
        return _cache[key]
    f0 = smooth_frame(w, h, 5)
    f1 = np.roll(f0, 1, axis=1 if w >= h else 0)
    # the Scharr response undivided (96 x the intensity slope: small Gauss-Newton steps, align_cases.case): across a side of 16 pixels
    # the step is badly conditioned, and a larger one throws the candidates of the finer levels out of the frame (16 x 4095 with the
    # response divided by 2 leaves level 1 without residuals)
    l0, l1, gx, gy = _levels_of(orc, f0, f1, 1)
    cand = []
    for lvl in range(5):
        cols, rows = w >> lvl, h >> lvl
        assert cols >= 1 and rows >= 1
        z = 2.0 ** -lvl
        xs = sorted({0, cols // 4, cols // 2, (3 * cols) // 4, max(cols - 2, 0), cols - 1})
        ys = sorted({0, rows // 2, max(rows - 2, 0), rows - 1})
        pts = [[x, y, z, 1] for y in ys for x in xs]
        cand.append(np.concatenate([large_edge_points(w, h, lvl), np.array(pts, np.float32)]))
    sx, sy = large_shift(w, h)
    _cache[key] = Pair(f"large_{w}x{h}", w, h, l0, l1, gx, gy, cand, (LARGE_FOCAL, LARGE_FOCAL, w / 2.0, h / 2.0), first=4, last=0, iters=3,
                       init6=[sx / LARGE_FOCAL, sy / LARGE_FOCAL, 0, 0, 0, 0])
    return _cache[key]


def large_generated(orc, vislam):
    """vis_align_batch on 4095 x 33, two frames: keypoints along x = 4080 ... 4094, so that the packed (y << 16) | x words of the generated
    candidate list reach x = 4094"""
    if "large_gen" in _cache:
        return _cache["large_gen"]
    W, H, n = 4095, 33, 2
    f0 = smooth_frame(W, H, 6)
    frames = np.stack([f0, np.roll(f0, 1, axis=1)])
    max_pts = 16
    pts = np.zeros((n, max_pts, 2), np.float32)
    pts[1, :15, 0] = np.arange(4080, 4095); pts[1, :15, 1] = 10 + (np.arange(15) % 13)
    npts = np.array([0, 15], np.int32)
    kp = np.zeros(15, vislam.KEYPOINT_DTYPE); kp["x"], kp["y"] = pts[1, :15, 0], pts[1, :15, 1]
    l0, l1, gx, gy = _levels_of(orc, frames[0], frames[1], 1)
    cand = [orc.patch_points(kp, W, H, l) for l in range(5)]
    # (a focal length of the frame's width: the points sit at the right edge, and a wide angle makes every step there a large one)
    pair = Pair("large_generated", W, H, l0, l1, gx, gy, cand, (4000.0, 4000.0, W / 2.0, H / 2.0))
    _cache["large_gen"] = dict(W=W, H=H, n=n, stride=4096, frames=frames, pts=pts, npts=npts, max_pts=max_pts, pair=pair)
    return _cache["large_gen"]


def align_320(orc, vislam):
    """the recipe of test_align_gpu.test_align_batch_explicit_points_and_init: 3 frames of 320 x 240, 230 and 17 matched points (some
    patches clipped by the border), an initial pose for pair 2 -> the inputs and the oracle's record of pairs 1 and 2"""
    if "a320" in _cache:
        return _cache["a320"]
    W, H, n = 320, 240, 3
    cv = vislam.synth_canvas(1024, 5)
    frames = np.stack([vislam.synth_frame(cv, t, W, H, 5) for t in range(n)])
    rng = np.random.default_rng(0)
    max_pts = 230
    pts = np.zeros((n, max_pts, 2), np.float32)
    pts[..., 0] = rng.uniform(-2, W + 2, (n, max_pts)); pts[..., 1] = rng.uniform(-2, H + 2, (n, max_pts))
    npts = np.array([0, 230, 17], np.int32)
    inits = np.zeros((n, 7), np.float32); inits[:, 3] = 1
    i2 = orc.se3_exp([0.001, 0, 0, 0, 0, 0.002]); inits[2] = i2.as_array()
    k = (200.0, 200.0, 160.0, 120.0)
    want = {}
    for t in (1, 2):
        kp = np.zeros(npts[t], vislam.KEYPOINT_DTYPE); kp["x"], kp["y"] = pts[t, :npts[t], 0], pts[t, :npts[t], 1]
        l0, l1, gx, gy = _levels_of(orc, frames[t - 1], frames[t], 1)
        pair = Pair(f"a320_{t}", W, H, l0, l1, gx, gy, [orc.patch_points(kp, W, H, l) for l in range(5)], k)
        want[t] = orc.estimate_pose_features(pair.params(orc), W, H, *pair.levels(), None if t == 1 else i2)
    _cache["a320"] = dict(W=W, H=H, n=n, frames=frames, pts=pts, npts=npts, max_pts=max_pts, inits=inits, k=k, want=want)
    return _cache["a320"]


# ---- family C, plan path: a stream of 24 frames in launches of 8 --------------------------------------------------------------------
def plan_params(vislam, w, h, gate):
    p = vislam.default_params()
    p.w_size, p.h_size = w, h
    p.fy = p.fx
    p.keyframe_min_points = 1 if gate else 0
    return p


def plan_frames(vislam, canvas, w, gate):
    """24 frames of the synthetic stream at w x 240; gate: the last frame of the first launch is flat (no keypoints: the gate refuses it,
    and the keyframe carried into the second launch is frame 6, not frame 7)"""
    key = ("plan", w, gate)
    if key not in _cache:
        frames = np.stack([vislam.synth_frame(canvas, t, w, PLAN_H) for t in range(PLAN_B * PLAN_LAUNCHES)])
        if gate:
            frames[PLAN_B - 1] = 128
        _cache[key] = frames
    return _cache[key]


def plan_walk(vislam, gate, n_kp, n_frames):
    """the keyframe pairing of the stream: per frame the stream index of the frame it is aligned against, or None (no pair); a frame is saved
    when the gate is off, or when it has more than 1 keypoint (K = 1: both of the gate's rules, Camera.cpp:225 / CameraGPU.cpp:164)"""
    prev, saved = [], []
    for g in range(n_frames):
        if not gate or n_kp[g] > 1:
            prev.append(saved[-1] if saved else None)
            saved.append(g)
        else:
            prev.append(None)
    return prev


# ---- family D: 64 x 48 --------------------------------------------------------------------------------------------------------------
SMALL_W, SMALL_H, SMALL_DIV = 64, 48, 2     # grad_div 2: every count keeps residuals on every level, a level runs 3+ iterations
SMALL_K = (200.0, 200.0, SMALL_W / 2.0, SMALL_H / 2.0)
LIST_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 100000)
LIST_LEVELS = ((1, 1), (3, 0))   # (first_level, last_level)
# generated path, 160 x 120, 7 frames: pair i + 1 takes row i's (max_pts is per call: one call per distinct max_pts)
GEN_ROWS = [(230, 0), (230, 1), (230, 199), (230, 200), (230, 201), (230, 230), (20, 50), (1, 1)]
GEN_W, GEN_H, GEN_N = 160, 120, 7
GEN_ITERS = 4                    # iterations per level: the numpy restatement of a 24 200-candidate pair costs ~50 ms each


def small_pair(vislam, orc, canvas):
    if "small" in _cache:
        return _cache["small"]
    f0, f1 = align_cases.two_frames(vislam, canvas, SMALL_W, SMALL_H, 1, 1)
    l0, l1, gx, gy = _levels_of(orc, f0, f1, SMALL_DIV)
    _cache["small"] = Pair("small", SMALL_W, SMALL_H, l0, l1, gx, gy, [np.zeros((0, 4), np.float32)] * 5, SMALL_K, iters=5)
    return _cache["small"]


def interior_list(w, h, n):
    """per level the interior pixels (1 ... cols - 2, 1 ... rows - 2) in row order, repeated until there are n of them"""
    out = []
    for lvl in range(5):
        cols, rows = w >> lvl, h >> lvl
        if cols < 3 or rows < 3:
            out.append(np.zeros((0, 4), np.float32)); continue
        yy, xx = np.mgrid[1:rows - 1, 1:cols - 1]
        base = np.stack([xx.ravel(), yy.ravel(), np.ones(xx.size), np.ones(xx.size)], 1).astype(np.float32)
        out.append(np.ascontiguousarray(np.resize(base, (n, 4))))
    return out


def count_pair(vislam, orc, canvas, n, first, last):
    return small_pair(vislam, orc, canvas).with_cand(f"list_{n}_L{first}-{last}", interior_list(SMALL_W, SMALL_H, n), first=first, last=last)


# Special values, level by level (cols, rows = the level's size; 64 x 48 halves exactly, so the level's own size is the same).  The
# initial pose is a translation of SPECIAL_SHIFT / fx along x and y, and the z of level l's rows is in units of 2^-l like family B's:
# a row with z = 1, w = 1 moves by +0.75 px in x and y on every level (fx_l * t / (z 2^-l) = 0.75 / z).
SPECIAL_SHIFT = 0.75


def special_rows(cols, rows):
    """-> [(kind, x, y, z, w, accepted at the initial pose)]: z and w as multiples of the level's unit z (1 on level 0).  The shift of a
    row is SPECIAL_SHIFT * w / z in x and y before the multiplication by w:  x2 = ((x - cx) + 0.75 * w / z + cx) * w."""
    mx, my = float(cols // 2), float(rows // 2)
    return [
        ("ordinary", mx, my, 1, 1, True), ("ordinary", 3.0, 2.0, 1, 1, True), ("ordinary", cols - 3.0, rows - 3.0, 1, 1, True),
        # (int)(-0.5) = 0: pixel 0 is read; the warped -0.5 + 0.75 is inside, with z = 4 the shift is 0.19 and -0.31 is outside
        ("x=-0.5", -0.5, my, 1, 1, True), ("x=-0.5", -0.5, my, 4, 1, False),
        ("y=-0.5", mx, -0.5, 1, 1, True), ("y=-0.5", mx, -0.5, 4, 1, False),
        ("x=0.5", 0.5, my, 1, 1, True), ("x=0.5", 0.5, my, -1, 1, False),           # z < 0 turns the shift round: 0.5 - 0.75 < 0
        ("y=0.5", mx, 0.5, 1, 1, True), ("y=0.5", mx, 0.5, -1, 1, False),
        # cols - 0.5 + 0.75 >= cols: outside; with z = -1 it moves left to cols - 1.25 and is read from column cols - 1
        ("x=cols-0.5", cols - 0.5, my, 1, 1, False), ("x=cols-0.5", cols - 0.5, my, -1, 1, True),
        ("y=rows-0.5", mx, rows - 0.5, 1, 1, False), ("y=rows-0.5", mx, rows - 0.5, -1, 1, True),
        ("x=cols", float(cols), my, 1, 1, False), ("x=cols", float(cols), my, -1, 1, False),      # (int)x1 >= cols, wherever it lands
        ("y=rows", mx, float(rows), 1, 1, False), ("y=rows", mx, float(rows), -1, 1, False),
        ("x=-1", -1.0, my, 1, 1, False), ("y=-1", mx, -1.0, 1, 1, False),
        ("z=0.5", mx, my, 0.5, 1, True), ("z=0.5", cols - 1.0, my, 0.5, 1, False),          # shift 1.5: cols - 1 + 1.5 >= cols
        ("z=2", mx, my, 2, 1, True), ("z=2", -0.5, my, 2, 1, False),                      # shift 0.375: -0.5 + 0.375 < 0
        ("z=0", mx, my, 0, 1, False), ("z=0", 3.0, 2.0, 0, 1, False),                     # P2 = 0: the quotient is infinite (or 0 / 0)
        ("z=-1", mx, my, -1, 1, True), ("z=-1", 0.5, my, -1, 1, False),
        # w = 0.5: x2 = (x + 0.375) * 0.5 -- inside for any x inside; outside needs another reason (the source pixel)
        ("w=0.5", mx, my, 1, 0.5, True), ("w=0.5", float(cols), my, 1, 0.5, False),
        ("w=0", mx, my, 1, 0, False), ("w=0", 3.0, 2.0, 1, 0, False),                     # x2 * 0 = 0 fails x2 > 0
    ]


def special_pair(vislam, orc, canvas):
    base = small_pair(vislam, orc, canvas)
    cand = []
    for lvl in range(5):
        zu = 2.0 ** -lvl
        rows_ = special_rows(SMALL_W >> lvl, SMALL_H >> lvl)
        cand.append(np.array([[x, y, z * zu, w] for _, x, y, z, w, _ in rows_], np.float32))
    t = SPECIAL_SHIFT / SMALL_K[0]
    return base.with_cand("special", cand, first=3, last=0, init6=[t, t, 0, 0, 0, 0])


def generated_small(vislam, orc):
    """-> {max_pts: dict(frames, pts (n, max_pts, 2), npts (n,), pairs {i: Pair})}: vis_align_batch on 160 x 120, 7 frames per call; the
    matched points are inside the frame by 8 px, so that 200 of them give the full 200 x 121 level-0 list"""
    if "gen_small" in _cache:
        return _cache["gen_small"]
    cv = vislam.synth_canvas(1024, 5)
    frames = np.stack([vislam.synth_frame(cv, t, GEN_W, GEN_H, 5) for t in range(GEN_N)])
    lev = [_levels_of(orc, frames[t], frames[t], 1) for t in range(GEN_N)]
    k = (150.0, 150.0, GEN_W / 2.0, GEN_H / 2.0)
    out = {}
    for max_pts in sorted({m for m, _ in GEN_ROWS}):
        rows_ = [r for r in GEN_ROWS if r[0] == max_pts]
        assert len(rows_) <= GEN_N - 1
        rng = np.random.default_rng(100 + max_pts)
        pts = np.zeros((GEN_N, max_pts, 2), np.float32)
        pts[..., 0] = rng.uniform(8, GEN_W - 9, (GEN_N, max_pts)); pts[..., 1] = rng.uniform(8, GEN_H - 9, (GEN_N, max_pts))
        npts = np.zeros(GEN_N, np.int32)
        pairs = {}
        for i, (_, np_) in enumerate(rows_):
            t = i + 1
            npts[t] = np_
            used = min(np_, max_pts, 200)                       # d_npts above max_pts is clamped; at most 200 are used
            kp = np.zeros(used, vislam.KEYPOINT_DTYPE); kp["x"], kp["y"] = pts[t, :used, 0], pts[t, :used, 1]
            pairs[t] = Pair(f"gen_{max_pts}_{np_}", GEN_W, GEN_H, lev[t - 1][0], lev[t][0], lev[t - 1][2], lev[t - 1][3],
                            [orc.patch_points(kp, GEN_W, GEN_H, l) for l in range(5)], k, iters=GEN_ITERS)
            pairs[t].npts = np_
        out[max_pts] = dict(frames=frames, pts=pts, npts=npts, pairs=pairs, k=k)
    _cache["gen_small"] = out
    return out


# ---- family E -----------------------------------------------------------------------------------------------------------------------
PATCH_SIZES = [(16, 16), (150, 110), (1080, 540), (4095, 4095)]
PATCH_COUNTS = (199, 200, 201)


def patch_keypoints(vislam, w, h, n):
    """n keypoints: on and one pixel outside every border and corner, at .5 coordinates beside them, the rest spread over the frame at
    integer and .5 coordinates (a fixed sequence: the first 199 of the 201 are the 199)"""
    edge_x = [0, 0.5, -1, -0.5, w - 1, w - 0.5, w, w + 1, w / 2.0, (w >> 1) + 0.5]
    edge_y = [0, 0.5, -1, -0.5, h - 1, h - 0.5, h, h + 1, h / 2.0, (h >> 1) + 0.5]
    pts = [(x, y) for y in edge_y for x in edge_x]
    rng = np.random.default_rng(w * 8191 + h)
    while len(pts) < 201:
        x, y = rng.integers(0, 2 * w) / 2.0, rng.integers(0, 2 * h) / 2.0
        pts.append((x, y))
    good = np.zeros(n, vislam.KEYPOINT_DTYPE)
    good["x"] = [p[0] for p in pts[:n]]; good["y"] = [p[1] for p in pts[:n]]
    return good
