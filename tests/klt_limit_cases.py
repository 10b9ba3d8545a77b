"""Scenes and point lists that take pyramidal KLT (csrc/klt.hip against tests/klt_ref.py) to its limits.  Shared by the CPU test
(tests/test_klt_limits_ref.py: the cases are what they claim, on the oracle's frames and the restatement alone) and the GPU test
(tests/test_klt_limits_gpu.py: the device against the restatement, byte for byte).

  full contrast   random fields of 0 / 255 blocks (and uniform noise), 160 x 120, frame 2 = frame 1 moved by SHIFT (whole pixels, exact):
                  the Scharr responses reach 16 * 255 * scale (32 640 at scale 8, the int16 end) and the five integer sums of a window
                  pass 2^31 -- the scenes of tests/test_klt_gpu.py stay below it, so an int accumulator would go unseen there
  saturated       all-255 and all-0 pairs: every gradient is 0, every point VIS_KLT_FLAT
  window edges    the exact ends of the window-fit rule at level 0, on both axes, for every radius
  alternating     a point list in which trackable and untrackable points alternate (the compaction's prefix over a partly set ballot)
  backward lost   a pair whose forward pass ends on a flat patch of frame 2: the backward template is flat, fb = -1
  plan guess      the guess rows of vis_batch_klt (indexed by the pair, at the caller's row stride) from the keypoints of a run

Measured on the oracle's pyramids and gradients, 64 grid points, forward-backward bound 1 px (test_klt_limits_ref.py prints these and
asserts the conditions; "above" = points of 64 whose sum of the first step at level 0 is beyond 2^31; the median distance of the
tracked results from the planted shift is without / with a guess, and the tests hold it to 4 x MEASURED_MEDIAN_ERR):

  case                  max |g|  max gxx  above  max |bx|  above  gxy above  tracked  median error px
  blocks_s8_r7           32 640  9.73e10     64   1.07e10     64         44       64  0.0033 / 0.0032
  blocks_s8_r10          32 640  1.94e11     64   1.94e10     64         47       64  0.0090 / 0.0091
  blocks_s3_r7_pyramid   12 240  1.37e10     64   4.01e9      21          0       64  0.0028 / 0.0030   (levels 2, 1, 0 run)
  blocks_s8_r2           32 640  2.06e10     61   2.08e9       0          8       64  0.0096 / 0.0114
  noise_s8_r7            30 688  2.58e10     64   1.61e9       0          2       64  0.334  / 0.332    (white noise has no slope to follow)

Records of 64 that change when one sum is wrapped to 32 bits (gxx, gxy, gyy, bx, by): 64 44 64 64 64; 64 47 64 64 64; 64 0 64 23 37;
61 8 63 0 1; 64 2 64 0 0.  On the blob scene of tests/test_klt_gpu.py: none at scale 3, r = 7; at scale 8, r = 10 (a combination no
test runs) 9 for gxx and 14 for gyy of 96.
"""
import numpy as np

import klt_ref as kr

W, H = 160, 120
SHIFT = (1, -1)                    # frame 2 shows frame 1 moved by this: a point p of frame 1 is at p + SHIFT in frame 2
TWO31 = float(2 ** 31)
NPOINTS = 64

# name -> (scene kind, block size, Scharr scale, win_radius, first_level)
FULL_CONTRAST = {
    "blocks_s8_r7": ("blocks", 2, 8, 7, 0),
    "blocks_s8_r10": ("blocks", 2, 8, 10, 0),
    "blocks_s3_r7_pyramid": ("blocks", 2, 3, 7, 3),
    "blocks_s8_r2": ("blocks", 2, 8, 2, 0),
    "noise_s8_r7": ("noise", 1, 8, 7, 0),
}
SATURATED = {"white": 255, "black": 0}
# median distance of the tracked results from the planted shift, measured (see the table above); the tests assert 4 x these
MEASURED_MEDIAN_ERR = {"blocks_s8_r7": 0.0033, "blocks_s8_r10": 0.0091, "blocks_s3_r7_pyramid": 0.0030, "blocks_s8_r2": 0.0114, "noise_s8_r7": 0.334}
# The cases whose first step has |bx| beyond 2^31 for at least half of the grid.  Near the solution e = -(Dx dx + Dy dy) / s, so
# bx = -(gxx dx + gxy dy) / s: one eighth of gxx for the one-pixel shift at scale 8.  The 441- and 225-pixel windows have gxx of 1e11
# and 5e10; a 25-pixel window cannot have more than 25 * 32640^2 = 2.7e10 (2^31 needs 1.7e10 at half of the points, random blocks give
# a median of 1e10), and noise has a quarter of the blocks' gxx.  Those two cases still take gxx, gxy and gyy beyond 32 bits.
BX_BEYOND = ("blocks_s8_r7", "blocks_s8_r10")


def moved_pair(kind, block, w=W, h=H, shift=SHIFT, seed=11):
    """(frame 1, frame 2) cut from one larger random field, so that frame 2 is frame 1 moved by `shift` with new content at the borders:
    kind "blocks": 0 / 255 squares of `block` pixels a side; "noise": uniform bytes"""
    m = 8
    rng = np.random.default_rng(seed)
    bh, bw = h + 2 * m, w + 2 * m
    if kind == "blocks":
        cells = rng.integers(0, 2, ((bh + block - 1) // block, (bw + block - 1) // block), dtype=np.uint8) * np.uint8(255)
        big = np.repeat(np.repeat(cells, block, 0), block, 1)[:bh, :bw]
    else:
        assert kind == "noise"
        big = rng.integers(0, 256, (bh, bw), dtype=np.uint8)
    sx, sy = shift
    assert abs(sx) <= m and abs(sy) <= m
    return np.ascontiguousarray(big[m:m + h, m:m + w]), np.ascontiguousarray(big[m - sy:m - sy + h, m - sx:m - sx + w])


def full_contrast_frames(name):
    if name in SATURATED:
        f = np.full((H, W), SATURATED[name], np.uint8)
        return f, f.copy()
    kind, block = FULL_CONTRAST[name][:2]
    return moved_pair(kind, block)


def full_contrast_params(name):
    if name in SATURATED:
        return kr.copy_params(kr.default_params(), scharr_scale=8, fb_max_px=1.0)
    _, _, scale, r, first = FULL_CONTRAST[name]
    return kr.copy_params(kr.default_params(), scharr_scale=scale, win_radius=r, first_level=first, fb_max_px=1.0)


def grid_points(r, count=NPOINTS, w=W, h=H):
    """`count` points whose window fits at level 0 with room for SHIFT and a few steps: two of three fractional, one on whole pixels"""
    pts, k, m = [], 0, r + 4
    while len(pts) < count:
        gx, gy = (k * 37) % 23, (k * 17) % 19
        x, y = m + (w - 2 * m - 1) * gx / 22.0, m + (h - 2 * m - 1) * gy / 18.0
        pts.append((float(np.floor(x)), float(np.floor(y))) if k % 3 == 0 else (float(np.floor(x)) + 0.31, float(np.floor(y)) + 0.77))
        k += 1
    return np.array(pts, np.float32)


def guess_for(pts, shift=SHIFT):
    """a guess 0.4 px beside the truth; every fifth x is NaN (a non-finite guess is treated as absent)"""
    g = (pts + np.array(shift, np.float32) + np.float32(0.4)).astype(np.float32)
    g[2::5, 0] = np.nan
    return g


def first_sums(kp, f1, f2, pts):
    """the five integer sums of the first step at last_level with d = 0 (int64 arrays over the points): what the accumulators hold"""
    l, r = kp.last_level, kp.win_radius
    p = kr.level_pos(pts.astype(np.float64), l)
    T = kr.intensity(f1[0][l], p[:, 0], p[:, 1], r)
    Dx, Dy = kr.gradient(f1[1][l], p[:, 0], p[:, 1], r), kr.gradient(f1[2][l], p[:, 0], p[:, 1], r)
    e = kr.intensity(f2[0][l], p[:, 0], p[:, 1], r) - T
    return dict(gxx=(Dx * Dx).sum((1, 2)), gxy=(Dx * Dy).sum((1, 2)), gyy=(Dy * Dy).sum((1, 2)), bx=(Dx * e).sum((1, 2)), by=(Dy * e).sum((1, 2)))


def truth_error(pts, rec, shift=SHIFT):
    """distances of the tracked results from pts + shift"""
    t = (rec["flags"] & kr.TRACKED) != 0
    got = np.stack([rec["x"], rec["y"]], 1).astype(np.float64)[t]
    return np.hypot(*(got - (pts.astype(np.float64)[t] + np.array(shift, np.float64))).T)


# ---- the blob scene and the point list of tests/test_klt_gpu.py ----------------------------------------------------------------------
BLOB_SHIFT = (3.3, -2.2)
FLAT_BOX = (96, 20, 136, 60)                                       # x0, y0, x1, y1 at 160 x 120 (scaled with the frame)
_frames_cache = {}


def blob_frames(w, h, n):
    """A, B, A, B ...: every pair is a shift by BLOB_SHIFT one way or the other"""
    if (w, h) not in _frames_cache:
        sx, sy = w / 160.0, h / 120.0
        box = None if w < 64 else (FLAT_BOX[0] * sx, FLAT_BOX[1] * sy, FLAT_BOX[2] * sx, FLAT_BOX[3] * sy)
        s = BLOB_SHIFT if w >= 64 else (0.6, -0.4)
        _frames_cache[(w, h)] = kr.blob_frames(w, h, [(0.0, 0.0), s], nblobs=160 if w >= 64 else 2000, flat_box=box)
    a, b = _frames_cache[(w, h)]
    return np.stack([a if i % 2 == 0 else b for i in range(n)])


def blob_points(w, h, r, count):
    """`count` points: a fractional and an integer grid, points whose window leaves each level on each side (and just stays inside), the
    textureless box, and coordinates that are not finite or absurdly large"""
    lw, lh = kr.half_dims(w, h)
    pts = []
    for l in range(4):
        back = lambda v: (v + 0.5) * (1 << l) - 0.5                # a level-l position at level 0
        for xl in (r - 0.5, r + 0.25, lw[l] - r - 2 + 0.5, lw[l] - r - 1 + 0.1):
            pts.append((back(xl), h * 0.5 + l))
        for yl in (r - 0.5, r + 0.25, lh[l] - r - 2 + 0.5, lh[l] - r - 1 + 0.1):
            pts.append((w * 0.45 + l, back(yl)))
    sx, sy = w / 160.0, h / 120.0
    pts += [((FLAT_BOX[0] + FLAT_BOX[2]) * 0.5 * sx + i, (FLAT_BOX[1] + FLAT_BOX[3]) * 0.5 * sy - i) for i in range(3)]
    nan, inf = np.nan, np.inf
    pts += [(nan, 20.0), (20.0, nan), (inf, 20.0), (20.0, -inf), (1e30, 20.0), (20.0, -1e30), (1e9, 1e9), (-5.0, 20.0), (w + 40.0, h + 40.0)]
    k = 0
    while len(pts) < count:                                        # the grid: every third point on whole pixels
        gx, gy = (k * 37) % 23, (k * 17) % 19
        x, y = w * (0.12 + 0.76 * gx / 22.0), h * (0.14 + 0.72 * gy / 18.0)
        pts.append((float(np.floor(x)), float(np.floor(y))) if k % 3 == 0 else (x + 0.31, y + 0.77))
        k += 1
    return np.array(pts[:count], np.float32)


def radius_points(r, count=64, w=W, h=H):
    """the point list of blob_points with the ten exact window edges of edge_points behind it"""
    return np.concatenate([blob_points(w, h, r, count), edge_points(r, w, h)])


# ---- window edges ---------------------------------------------------------------------------------------------------------------------
EDGE_OOB = (False, True, False, False, True)      # per axis: which of edge_values' five leave the level


def edge_values(r, size):
    """the ends of the fit rule floor(v) - r >= 0, floor(v) + r + 1 <= size - 1, as float32: r (fits), the float below r (floor r - 1:
    out), size - r - 2 (fits exactly), the float below size - r - 1 (still floor size - r - 2: fits), size - r - 1 (out)"""
    f = np.float32
    return [f(r), np.nextafter(f(r), f(0)), f(size - r - 2), np.nextafter(f(size - r - 1), f(0)), f(size - r - 1)]


def edge_points(r, w=W, h=H):
    """ten points: the five edge values in x at a textured row, then in y at a textured column (tests/test_klt_gpu.py's blob scene has
    its textureless zone at x > 71, y < 85)"""
    return np.array([(x, np.float32(h * 0.8)) for x in edge_values(r, w)] + [(np.float32(w * 0.3), y) for y in edge_values(r, h)], np.float32)


# ---- alternating points ---------------------------------------------------------------------------------------------------------------
def alternating_points(count, r=7, w=W, h=H):
    """even places: grid points in the left 72 columns, away from the blob scene's textureless zone (x > 71, y < 85) and the borders;
    odd places: points that cannot be tracked (beside the border, NaN, outside)"""
    good = grid_points(r + 4, (count + 1) // 2, 72, h)
    bad = [(1.5, 30.0), (np.nan, 40.0), (w - 2.0, 50.0), (60.0, 0.25), (70.0, h - 1.5), (-30.0, 20.0), (40.0, np.inf), (1e30, 1e30)]
    out = np.zeros((count, 2), np.float32)
    out[0::2] = good[:len(out[0::2])]
    out[1::2] = np.array([bad[k % len(bad)] for k in range(len(out[1::2]))], np.float32).reshape(-1, 2)
    return out


COUNT_CASES = {1: [0, 1, 0, 4], 2: [0, 2, 1, 5], 3: [0, 3, 2, 1], 5: [0, 5, 4, 9], 67: [0, 67, 66, 65, 64, 63, 1, 90]}     # max_pts -> d_npts


# ---- the backward pass lost -----------------------------------------------------------------------------------------------------------
PATCH = (58, 38, 106, 86)          # x0, y0, x1, y1 (exclusive) of the flat patch in frame 2: 48 px a side >= 2 r + 31 at r = 7


def backward_lost_case():
    """(frame 1, frame 2, params, pts, guess): frame 1 is a field of 6-px blocks, frame 2 the same with a flat patch of 128 laid over
    it.  One step per level from a guess at the patch centre ends inside the patch; from there the backward template is flat on
    every level (all gradients 0), so the backward pass is lost at last_level: fb = -1, VIS_KLT_FB, x / y the forward result"""
    f1, _ = moved_pair("blocks", 6, seed=21)
    f2 = f1.copy()
    x0, y0, x1, y1 = PATCH
    f2[y0:y1, x0:x1] = 128
    kp = kr.copy_params(kr.default_params(), max_iters=1, fb_max_px=1.0, max_err=0.0)
    cx, cy = (x0 + x1 - 1) * 0.5, (y0 + y1 - 1) * 0.5
    pts = np.array([(cx + dx, cy + dy) for dy in (-6.0, 0.25, 5.5) for dx in (-7.0, -2.5, 0.0, 3.75, 8.0)] + [(20.3, 100.6), (140.0, 20.0)], np.float32)
    guess = np.tile(np.array([cx, cy], np.float32), (len(pts), 1))
    guess[-2:] = np.nan                                            # two ordinary points outside the patch, without a guess
    return f1, f2, kp, pts, guess


# ---- the plan's guess rows -------------------------------------------------------------------------------------------------------------
def plan_guess(links, kps, row_cap):
    """guess rows for vis_batch_klt, indexed by the PAIR i: keypoint k of frame links[i] + (0.3 + 0.05 i, -0.2 - 0.05 i); NaN in every
    fifth entry and behind the row's count; the rows of frames without a pair hold 1e30"""
    n = len(links)
    g = np.full((n, row_cap, 2), np.nan, np.float32)
    for i in range(n):
        q = int(links[i])
        if q < 0:
            g[i] = np.float32(1e30)
            continue
        m = len(kps[q])
        g[i, :m, 0] = kps[q]["x"] + np.float32(0.3 + 0.05 * i)
        g[i, :m, 1] = kps[q]["y"] + np.float32(-0.2 - 0.05 * i)
        g[i, 4::5] = np.nan
    return g
