"""Hostile matched points, candidate rows and poses for the photometric alignment and the patch builders: values that are no usable
numbers (NaN, +-inf), that overflow `int` (2^31 ... 2^35 and their float predecessors, +-3e9, +-1e30, +-3e38), or that are merely far
outside the frame.  Not a test module: shared by tests/test_align_hostile_ref.py (CPU) and tests/test_align_hostile_gpu.py.

  exact_span / patch_rule     the candidate window of include/vislam_hip.h (vis_patch_points) restated with integers and fractions: no
                              float is ever converted to an int, so the restatement has a value for every float
  coordinate_values / kinds   the hostile coordinates, in x, in y and in both
  LAYOUTS / layout            where in a row of MAX_PTS matched points they sit
  frames / levels / points    160 x 120 synthetic frames, the oracle's pyramid and gradients, clean matched points
  deleted                     a row with the keypoints of a layout taken out: by the rule a hostile keypoint contributes no candidate, so a
                              row that holds them must give the record of the row without them
  old_loop_rows               the reference's loop as it was, for coordinates on which it ends (what tests/golden/patch_points_rows.npz records)
  hostile_inits               poses no alignment should be started from
  meets_a_guard / EXCEPT_*    the vacuity guards of the GPU suite and, by name, every case that meets none
  list_rows / hostile_list    explicit candidate rows (x, y, z, w) with one hostile component each"""
import math
from fractions import Fraction

import numpy as np

import stride_range_cases as src

F32 = np.float32
W, H = 160, 120
STRIDES = (160, 176)
N_FRAMES = 8                          # seven pairs per launch
MAX_PTS = 230
USED = 200                            # min(num_max_keypoints, 200), src/Camera.cpp:377
ITERS = 4                             # iterations per level (the numpy restatement of the Tukey modes costs ~50 ms per 24 200 candidates)
K = (150.0, 150.0, W / 2.0, H / 2.0)
FILL = 0xEE                           # what every output buffer holds before a call
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

ALIGN_DTYPE = np.dtype([("pose", "<f4", 7), ("matrix", "<f4", 16), ("error", "<f4", 5), ("initial_error", "<f4"), ("iterations", "<i4", 5),
                        ("n_residuals", "<i4", 5)])
TRACK_DTYPE = np.dtype([("pose", "<f4", 7), ("composed", "<i4")])


# ---- the rule, exactly ----------------------------------------------------------------------------------------------------------------
PATCH_SIZE = (5, 3, 2, 5, 5)          # start_point = patch_size - 1 / 2 with integer 1 / 2 == 0 (src/Camera.cpp:376)


def level_coordinate(v, level):
    """the keypoint coordinate on a level as the builders form it: float32(((double)v + 0.5) * (double)factor - 0.5)"""
    with np.errstate(all="ignore"):
        return F32((np.float64(F32(v)) + 0.5) * np.float64(F32(1.0 / (1 << level))) - 0.5)


def exact_span(c, sp, size):
    """the integers i with 0 < i < size, i >= trunc(c - sp) and i <= c + sp, sum and difference in float32 and compared as the rationals
    they are -> (lo, hi) or None.  A NaN or infinite c has none."""
    c = F32(c)
    if not math.isfinite(float(c)):
        return None
    with np.errstate(all="ignore"):
        a, b = c - F32(sp), c + F32(sp)                    # float32 arithmetic (finite: |c| <= FLT_MAX and sp <= 5 cannot overflow)
    a, b = Fraction(float(a)), Fraction(float(b))
    lo = max(math.trunc(a), 1)                             # Fraction -> int: towards zero, exact for any magnitude
    hi = min(math.floor(b), size - 1)
    return (lo, hi) if lo <= hi else None


def patch_rule(xy, w, h, level):
    """vis_patch_points' list of one level for the keypoints xy (m x 2 float32, at most USED are read) -> rows (x, y, 1, 1) float32"""
    sp = PATCH_SIZE[level]
    rows = []
    for x, y in np.asarray(xy, F32).reshape(-1, 2)[:USED]:
        sx = exact_span(level_coordinate(x, level), sp, w >> level)
        sy = exact_span(level_coordinate(y, level), sp, h >> level)
        if sx is None or sy is None:
            continue
        ii, jj = np.meshgrid(np.arange(sx[0], sx[1] + 1), np.arange(sy[0], sy[1] + 1), indexing="ij")    # column outer, row inner
        rows.append(np.stack([ii.ravel(), jj.ravel(), np.ones(ii.size, np.int64), np.ones(ii.size, np.int64)], 1))
    return np.concatenate(rows).astype(F32) if rows else np.zeros((0, 4), F32)


def old_loop_rows(xy, w, h, level):
    """the reference's loop as it was (src/Camera.cpp:381-384), for coordinates on which it ends and every cast is representable
    (|coordinate| <= 2^20): for (i = (int)(x - sp); (float)i <= x + sp; i++) for (j ...) if (i > 0 && i < cols && j > 0 && j < rows)"""
    sp, cols, rows = F32(PATCH_SIZE[level]), w >> level, h >> level
    out = []
    for x, y in np.asarray(xy, F32).reshape(-1, 2)[:USED]:
        assert abs(float(x)) <= 2 ** 20 and abs(float(y)) <= 2 ** 20
        cx, cy = level_coordinate(x, level), level_coordinate(y, level)
        i = int(cx - sp)                                   # (int) of a float inside int's range: towards zero
        while F32(i) <= cx + sp:
            j = int(cy - sp)
            while F32(j) <= cy + sp:
                if 0 < i < cols and 0 < j < rows:
                    out.append((i, j, 1, 1))
                j += 1
            i += 1
    return np.array(out, F32).reshape(-1, 4)


# ---- hostile coordinates --------------------------------------------------------------------------------------------------------------
def _below(v):
    return F32(np.nextafter(F32(v), F32(0)))


def coordinate_values(w=W):
    """{name: float32}: the values a keypoint coordinate is replaced by.  Every one is NaN, infinite, or so far from [0, w) that its window
    cannot touch a level; three of them (3e9, the powers of two from 2^31 and 3e38 / 1e30 / +inf) made the reference's loop endless"""
    v = {"nan": F32(np.nan), "pinf": F32(np.inf), "ninf": F32(-np.inf), "p3e38": F32(3e38), "n3e38": F32(-3e38), "p1e30": F32(1e30),
         "n1e30": F32(-1e30), "p3e9": F32(3e9), "n3e9": F32(-3e9), "p1e9": F32(1e9), "w+40": F32(w + 40), "m40": F32(-40)}
    for l in range(5):
        v[f"2^{31 + l}"] = F32(2.0 ** (31 + l))            # 2^31 * 2^l: the level-l coordinate of it is 2^31 (l = 1 is 2^32)
        v[f"2^{31 + l}-"] = _below(2.0 ** (31 + l))        # its float predecessor (l = 0: the largest float below 2^31)
    return v


AXES = ("x", "y", "xy")


def kinds():
    """"axis:name" for every hostile value in x, in y and in both"""
    return [f"{a}:{n}" for n in coordinate_values() for a in AXES]


def contributes(kind, w=W, h=H):
    """True iff a keypoint of this kind still has candidates on a level the alignment runs (3 ... 0).  By the rule that takes a non-empty
    window in x AND in y; the coordinate that is not replaced is a clean one, inside the frame.  Only w + 40 / h + 40 does: on level 3
    its window reaches the last column / row.  Such a keypoint is ordinary data: the reference is the oracle on the row as it is"""
    axis, name = kind.split(":")
    for l in range(4):
        ok = True
        if "x" in axis:
            ok = ok and exact_span(level_coordinate(coordinate_values(w)[name], l), PATCH_SIZE[l], w >> l) is not None
        if "y" in axis:
            ok = ok and exact_span(level_coordinate(coordinate_values(h)[name], l), PATCH_SIZE[l], h >> l) is not None
        if ok:
            return True
    return False


def apply_kind(kind, pts, idx, w=W, h=H):
    """a copy of the row pts (m x 2 float32) with the entries at idx replaced (w + 40 means h + 40 in y)"""
    axis, name = kind.split(":")
    out = np.array(pts, F32)
    idx = np.asarray(idx, np.int64)
    if "x" in axis:
        out[idx, 0] = coordinate_values(w)[name]
    if "y" in axis:
        out[idx, 1] = coordinate_values(h)[name]
    return out


# layouts over the USED keypoints of a row of MAX_PTS; "inside" ones replace keypoints that are read, "past" ones entries that are not
INSIDE_LAYOUTS = ("first", "stride5", "first3", "all", "wave_edges", "last")
PAST_LAYOUTS = ("past_used", "past_count")
PAST_COUNT = 150                      # d_npts of the "past_count" rows: entries 150 ... 229 are beyond the row's count


def layout(name):
    return {"first": np.array([0]), "stride5": np.arange(0, USED, 5), "first3": np.arange(3), "all": np.arange(USED),
            # the prefix of the per-keypoint counts crosses the waves of the workgroup here
            "wave_edges": np.array([63, 64, 127, 128, 191, 192]), "last": np.array([USED - 1]),
            "past_used": np.array([USED, USED + 1]), "past_count": np.arange(PAST_COUNT, MAX_PTS)}[name]


def deleted(pts, idx):
    """the USED keypoints a row of MAX_PTS reads, with those at idx taken out -> (row padded to MAX_PTS with zeros, count)"""
    keep = np.setdiff1d(np.arange(USED), idx)
    out = np.zeros((MAX_PTS, 2), F32)
    out[:len(keep)] = np.asarray(pts, F32)[keep]
    return out, len(keep)


# ---- frames and clean rows --------------------------------------------------------------------------------------------------------------
_cache = {}


def frames(vislam):
    if "frames" not in _cache:
        cv = vislam.synth_canvas(1024, 5)
        _cache["frames"] = np.stack([vislam.synth_frame(cv, t, W, H, 5) for t in range(N_FRAMES)])
    return _cache["frames"]


def levels(vislam, orc, t):
    """the oracle's half pyramid and gradients of frame t -> (levels, gx, gy)"""
    if ("lev", t) not in _cache:
        l0, _, gx, gy = src._levels_of(orc, frames(vislam)[t], frames(vislam)[t], 1)
        _cache["lev", t] = (l0, gx, gy)
    return _cache["lev", t]


def points():
    """(N_FRAMES, MAX_PTS, 2) clean matched points, inside the frame by 8 px: 200 of them give the full 200 x 121 level-0 list"""
    if "pts" not in _cache:
        rng = np.random.default_rng(20260)
        pts = np.zeros((N_FRAMES, MAX_PTS, 2), F32)
        pts[..., 0] = rng.uniform(8, W - 9, (N_FRAMES, MAX_PTS)); pts[..., 1] = rng.uniform(8, H - 9, (N_FRAMES, MAX_PTS))
        _cache["pts"] = pts
    return _cache["pts"]


def params(mod, iters=ITERS):
    ap = mod.default_align_params()
    ap.fx, ap.fy, ap.cx, ap.cy = K
    ap.max_iterations = iters
    return ap


def record(res):
    """a vislam.AlignResult (or the oracle's) as one ALIGN_DTYPE record"""
    return np.frombuffer(bytes(res), ALIGN_DTYPE)[0]


def oracle_pair(vislam, orc, t, row, count, init=None, mode=0, iters=ITERS, cand=None):
    """the record of pair t (frame t-1 -> frame t) for the matched points row[:count]: the oracle (mode 0) or its numpy restatement with
    Tukey weights (tests/align_weighted_ref.py); cached.  cand: explicit per-level candidate rows instead of the patches of the points"""
    key = ("orc", t, np.asarray(row, F32).tobytes(), count, None if init is None else bytes(init), mode, iters,
           None if cand is None else tuple(c.tobytes() for c in cand))
    if key not in _cache:
        used = max(0, min(count, MAX_PTS, USED))
        kp = np.zeros(used, vislam.KEYPOINT_DTYPE)
        kp["x"], kp["y"] = row[:used, 0], row[:used, 1]
        (l0, gx, gy), (l1, _, _) = levels(vislam, orc, t - 1), levels(vislam, orc, t)
        if cand is None:
            cand = [orc.patch_points(kp, W, H, l) for l in range(5)]
        if mode == 0:
            res = orc.estimate_pose_features(params(orc, iters), W, H, l0, l1, gx, gy, cand, init)
        else:
            import align_weighted_ref as ref
            res = ref.estimate_pose_features(orc, params(orc, iters), W, H, l0, l1, gx, gy, cand, init, weights=mode)
        _cache[key] = record(res)
    return _cache[key]


# ---- hostile poses ----------------------------------------------------------------------------------------------------------------------
def hostile_inits(vislam, orc):
    """[(name, Se3f)]: quaternion (x, y, z, w) and translation an alignment is started from"""
    nan, inf = float("nan"), float("inf")
    # a small rotation's unit quaternion times 1e3: the product is formed in float64 and rounded to float32 once, below
    rot = orc.se3_exp([0, 0, 0, 0.01, -0.02, 0.015]).as_array()[:4].astype(np.float64) * 1e3
    rows = [("q_nan_one", [0, nan, 0, 1, 0, 0, 0]), ("q_nan_all", [nan, nan, nan, nan, 0, 0, 0]), ("q_zero", [0, 0, 0, 0, 0, 0, 0]),
            ("q_norm_1e3", list(rot) + [0, 0, 0]),         # R = I - 2 (...) has entries of 1e4: every point leaves the frame
            ("q_norm_1e3_w", [0, 0, 0, 1e3, 0, 0, 0]),     # norm 1e3 with x = y = z = 0: toRotationMatrix gives I, the step renormalises
            ("tz_p3e38", [0, 0, 0, 1, 0, 0, 3e38]),        # a finite depth of 3e38: every point projects onto (cx, cy)
            ("t_pinf", [0, 0, 0, 1, inf, 0, 0]), ("t_ninf", [0, 0, 0, 1, 0, -inf, 0]),
            ("t_inf_z", [0, 0, 0, 1, 0, 0, inf]), ("t_p3e38", [0, 0, 0, 1, 3e38, 0, 0]), ("t_n3e38", [0, 0, 0, 1, 0, 0, -3e38]),
            ("t_all_nan", [0, 0, 0, 1, nan, nan, nan]),
            ("tz_m2", [0, 0, 0, 1, 0, 0, -2.0]),           # P2 = z + tz w = -1 for the generated rows (z = w = 1): every depth negative
            ("tz_m1", [0, 0, 0, 1, 0, 0, -1.0])]           # P2 = 1 - 1 = 0 exactly: x2 = P0 fx / 0
    return [(n, vislam.Se3f(*[float(F32(v)) for v in r])) for n, r in rows]


CLEAN_INIT6 = [0.001, 0, 0, 0, 0, 0.002]
INIT_COUNT = 40                       # matched points per pair in the launches with hostile poses


# ---- vacuity guards ---------------------------------------------------------------------------------------------------------------------
def meets_a_guard(rec):
    """a record shows that the alignment worked on something: residuals on every level it ran (3 ... 0), or two or more iterations on
    level 0 (iterations[0] is the index at which the level stopped)"""
    return bool((rec["n_residuals"][:4] > 0).all()) or int(rec["iterations"][0]) >= 1


# Every hostile case that meets no guard on the oracle, by name; tests/test_align_hostile_ref.py asserts that these are exactly the ones.
# Nothing is left to align in them: all keypoints hostile; a pose with a NaN or an infinity in it.
EXCEPT_LAYOUTS = ("all",)
EXCEPT_POSES = ("q_nan_one", "q_nan_all", "t_pinf", "t_ninf", "t_all_nan")
# ... and four that are neither, each for a reason of arithmetic that holds for oracle and device alike:
EXCEPT_FINITE_POSES = ("q_norm_1e3",  # rotation entries of 1e4 move every point out of the frame
                       "t_p3e38",     # tx = 3e38: P0 * fx overflows to inf, x2 < cols fails for every point
                       "tz_m1")       # P2 = 1 - 1 = 0 exactly (the case the depth test `z2 != 0` exists for): every point is skipped
EXCEPT_ROWS = ("z:1e-38", "z:1e-45")  # ACCEPTED rows (x2 = x1) whose 1 / z2 = 1e38 / inf overflows the Jacobian: the first step is NaN, and a
                                      # NaN pose warps nothing on any later iteration or level


# ---- explicit candidate rows ------------------------------------------------------------------------------------------------------------
LIST_N = 1100                         # rows 255 / 256 end the first round of 256 threads, rows 1023 / 1024 the first round of 4 x 256
LIST_EDGES = (255, 256, 1023, 1024)


def list_rows(level):
    """LIST_N clean rows (x, y, 1, 1) of a level: interior pixels in row order, repeated"""
    return src.interior_list(W, H, LIST_N)[level]


def list_values():
    """{"component:name": (column of the row, value or None where it depends on the level's size, name)}"""
    nan, inf = np.nan, np.inf
    v = {}
    for c, comp in ((0, "x"), (1, "y")):
        for name, val in (("nan", nan), ("pinf", inf), ("ninf", -inf), ("p3e38", 3e38), ("n3e38", -3e38), ("m0.5", -0.5), ("m1", -1.0),
                          ("size-0.5", None), ("size", None)):
            v[f"{comp}:{name}"] = (c, val, name)
    for name, val in (("zero", 0.0), ("neg", -1.0), ("1e-38", 1e-38), ("1e-45", 1e-45), ("nan", nan), ("inf", inf)):
        v[f"z:{name}"] = (2, val, name)
    for name, val in (("zero", 0.0), ("nan", nan), ("two", 2.0)):
        v[f"w:{name}"] = (3, val, name)
    return v


LIST_PLACES = ("stride5", "edges")


def hostile_list(kind, place):
    """per level 0 ... 4 (the alignment runs 3 ... 0) the clean rows with the component of `kind` replaced at every fifth row or at
    LIST_EDGES"""
    col, val, name = list_values()[kind]
    idx = np.arange(0, LIST_N, 5) if place == "stride5" else np.array(LIST_EDGES)
    out = []
    for lvl in range(5):
        rows = list_rows(lvl).copy()
        size = (W >> lvl) if col == 0 else (H >> lvl)
        rows[idx, col] = F32(size - 0.5 if name == "size-0.5" else size if name == "size" else val)
        out.append(rows)
    return out
