"""Hostile correspondences for the geometry entry points: rows whose entries are not usable numbers (NaN, +-inf), overflow the arithmetic
(+-3e38 pixels, map points scaled past sqrt(DBL_MAX)) or are degenerate (duplicates, points behind or at the camera centre).  Not a test
module: shared by tests/test_hostile_inputs_ref.py (CPU) and tests/test_hostile_inputs_gpu.py.

  hostile(kind, arrays, idx)   copies of a finite row with the entries at idx replaced
  layout(name, m, tile)        the index sets: every fifth point, the first three, all, the two sides of an LDS tile's end
  same_record(a, b)            records equal field by field; a float is byte-equal or NaN on both sides (x86 and the device do not produce
                               the same NaN sign or payload, so a byte comparison of a NaN proves nothing either way)
  exact_inlier_pnp / _h        the stated per-point predicate of PnP / of the homography transfer test evaluated with mpmath at 200 bits on
                               the float / double inputs taken exactly: (verdict, relative distance from the threshold)

Kinds are written "target:name".  The target names the array of `arrays` (a dict) that is changed; "both" = "p1" and "p2".
  pixel kinds (float32 m x 2): nan (x), pinf (y = +inf), ninf (x = -inf), inf_all (both coordinates +inf), big (+-3e38, signs alternating),
                               dup (p2 = p1 whatever the target: a correspondence that did not move),
                               mag+<k> / mag-<k> (targets p1, p2, xy only): ONE coordinate of each entry -- x of the even entries of idx, y of
                               the odd ones -- becomes c +- fx k sqrt(FLT_MAX) rounded to float (c = cx or cy): a finite pixel whose NORMALISED
                               coordinate is +-k sqrt(FLT_MAX) = +-k 1.84e19, k on MAG_LADDER: from ordinary numbers through the magnitude whose
                               square overflows a float (where single-precision error radii become +inf) to a pixel of 8e36, a factor 40
                               below FLT_MAX.  Never on both images: no hole was seen there, and "both:" keeps its six kinds.  Layouts
                               stride5, first3 and tile_edge
  point kinds (float64 m x 3, target "X"): nan (x), pinf (z = +inf), ninf (x = -inf), inf_all, x1e200, x1e160 (just above sqrt(DBL_MAX) =
                               1.34e154 in camera depth), x1e150 (just below: an ordinary, wrong, finite point), mirror (through the camera
                               centre: the same pixel, W < 0), centre (at the camera centre: W = 0 up to rounding), tiny (every entry becomes
                               X[idx[0]] + 1e-300 = X[idx[0]]: entry idx[0] stays a true correspondence, the others are duplicates of its
                               point under their own pixels).  mirror and centre need the true pose as arrays["R"], arrays["t"]."""
import numpy as np

import homography_pose_ref as hpr
import homography_ref as hr
import pnp_ref as pr
import pose_degenerate_cases as pdc
import triangulate_ref as tr

PIXEL_KINDS = ("nan", "pinf", "ninf", "inf_all", "big", "dup")
POINT_KINDS = ("nan", "pinf", "ninf", "inf_all", "x1e200", "x1e160", "x1e150", "mirror", "centre", "tiny")
NONFINITE = ("nan", "pinf", "ninf", "inf_all")
LAYOUTS = ("stride5", "first3", "all", "tile_edge")
DBL_MAX = 1.7976931348623157e308
FLT_MAX = float(np.finfo(np.float32).max)
ROOT_FLT_MAX = float(np.sqrt(np.float64(FLT_MAX)))                     # 1.8446743e19
# the normalised magnitudes of the mag kinds, in units of sqrt(FLT_MAX); a step whose pixel fx k sqrt(FLT_MAX) would pass FLT_MAX is dropped
MAG_LADDER = tuple(k for k in (1e-12, 1e-6, 0.5, 0.99, 1.1, 1.6, 2.7, 5.4, 54.0, 1e6, 1e15) if pdc.FOCAL * k * ROOT_FLT_MAX < FLT_MAX)
MAG_NAMES = tuple(f"mag{s}{k:g}" for k in MAG_LADDER for s in "+-")
MAG_LAYOUTS = ("stride5", "first3", "tile_edge")
MAG_NEVER_FROM = 1e-6                                                  # from this step up a ladder entry may be in no essential-matrix mask
MARGIN = 1e-9                                                          # exact_inlier's verdict is compared where the point is farther than this


def layout(name, m, tile=None):
    if name == "stride5":
        return np.arange(0, m, 5)
    if name == "first3":
        return np.arange(3)
    if name == "all":
        return np.arange(m)
    if name == "tile_edge":
        assert m == tile + 1
        return np.array([tile - 1, tile])
    raise ValueError(name)


def mag_pixel(name, axis):
    """the float32 pixel coordinate (axis 0 = x, 1 = y) of the ladder step "mag+<k>" / "mag-<k>": c +- fx k sqrt(FLT_MAX), finite"""
    v = np.float32((pdc.CX, pdc.CY)[axis] + float(name[3:]) * ROOT_FLT_MAX * pdc.FOCAL)     # (the sign is part of the number)
    assert name in MAG_NAMES and np.isfinite(v)
    return v


def _pixels(name, a, idx):
    a = np.array(a, np.float32)
    if name == "nan":
        a[idx, 0] = np.nan
    elif name == "pinf":
        a[idx, 1] = np.inf
    elif name == "ninf":
        a[idx, 0] = -np.inf
    elif name == "inf_all":
        a[idx] = np.inf
    elif name == "big":
        sgn = np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0).astype(np.float32)
        a[idx, 0], a[idx, 1] = np.float32(3e38) * sgn, -np.float32(3e38) * sgn
    elif name.startswith("mag"):
        a[idx[0::2], 0], a[idx[1::2], 1] = mag_pixel(name, 0), mag_pixel(name, 1)
    else:
        raise ValueError(name)
    return a


def _points(name, arrays, idx):
    X = np.array(arrays["X"], np.float64)
    if name == "nan":
        X[idx, 0] = np.nan
    elif name == "pinf":
        X[idx, 2] = np.inf
    elif name == "ninf":
        X[idx, 0] = -np.inf
    elif name == "inf_all":
        X[idx] = np.inf
    elif name in ("x1e200", "x1e160", "x1e150"):
        X[idx] = X[idx] * float(name[1:])
    elif name in ("mirror", "centre"):
        R, t = np.asarray(arrays["R"], np.float64).reshape(3, 3), np.asarray(arrays["t"], np.float64).reshape(3)
        C = -R.T @ t
        X[idx] = 2.0 * C - X[idx] if name == "mirror" else C
    elif name == "tiny":
        X[idx] = X[idx[0]] + 1e-300
    else:
        raise ValueError(name)
    return X


def hostile(kind, arrays, idx):
    """a copy of the dict `arrays` with the entries at idx of the kind's target replaced (the other arrays are shared, not copied)"""
    target, name = kind.split(":")
    idx = np.asarray(idx, np.int64)
    out = dict(arrays)
    if name == "dup":
        assert name in PIXEL_KINDS
        p2 = np.array(arrays["p2"], np.float32)
        p2[idx] = np.asarray(arrays["p1"], np.float32)[idx]
        out["p2"] = p2
    elif target == "X":
        assert name in POINT_KINDS
        out["X"] = _points(name, arrays, idx)
    else:
        assert name in PIXEL_KINDS or (name in MAG_NAMES and target != "both")
        for key in (("p1", "p2") if target == "both" else (target,)):
            out[key] = _pixels(name, arrays[key], idx)
    return out


def pair_kinds():
    """the pixel kinds of a two-image row: every name on image 1, image 2 and both (dup once)"""
    return [f"{t}:{k}" for k in PIXEL_KINDS[:-1] for t in ("p1", "p2", "both")] + ["p2:dup"]


def mag_pair_kinds():
    """the magnitude ladder of a two-image row: every step with both signs on image 1 and on image 2 (never both: see the module text)"""
    return [f"{t}:{n}" for n in MAG_NAMES for t in ("p1", "p2")]


def mag_pnp_kinds():
    return [f"xy:{n}" for n in MAG_NAMES]


def mag_of(kind):
    """the |k| of a mag kind, None of any other"""
    name = kind.split(":")[1]
    return abs(float(name[3:])) if name.startswith("mag") else None


def pnp_kinds():
    """the kinds of a PnP row: every point kind, and the pixel kinds on its one image"""
    return [f"X:{k}" for k in POINT_KINDS] + [f"xy:{k}" for k in PIXEL_KINDS[:-1]]


# ---- records ----------------------------------------------------------------------------------------------------------------------
def same_value(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.reshape(-1), b.reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    bits = a.view(f"u{a.dtype.itemsize}") == b.view(f"u{b.dtype.itemsize}")
    return bool((both_nan | bits).all())


def same_record(a, b, skip=()):
    """True iff two numpy records (or dicts of values) agree: an integer field is equal, a float field byte-equal or NaN on both sides;
    the fields named in `skip` are not compared"""
    if isinstance(a, dict) or isinstance(b, dict):
        if set(a.keys()) != set(b.keys()):
            return False
        names = list(a.keys())
    else:
        if a.dtype != b.dtype:
            return False
        names = a.dtype.names
    return all(same_value(a[k], b[k]) for k in names if k not in skip)


def differing_fields(a, b):
    names = list(a.keys()) if isinstance(a, dict) else a.dtype.names
    return [k for k in names if not same_value(a[k], b[k])]


# ---- the predicates, exactly --------------------------------------------------------------------------------------------------------
_exact = {}


def _mp():
    import mpmath
    mpmath.mp.prec = 200
    return mpmath


def _rel(mp, lhs, rhs):
    if rhs == 0:
        return 0.0 if lhs == 0 else float("inf")
    return float(abs(lhs - rhs) / rhs)


def exact_inlier_pnp(P, X, xy, cx, cy, fx_inv, thr2):
    """(verdict bool[m], distance float[m]) of include/vislam_hip.h's PnP per-point test under the pose P = (R row-major, t): W > 0,
    thr2 (W W) finite (as a double: <= DBL_MAX) and (U - x W)^2 + (V - y W)^2 <= thr2 (W W), with x = (u - cx) fx_inv.  A point with a
    non-finite coordinate does not pass (distance inf).  distance = the smaller of |lhs - rhs| / rhs and |W| / (|R_2| |X| + |t_2|) (how far
    W is from changing sign)"""
    mp = _mp()
    f = lambda v: mp.mpf(float(v))
    Pm = [f(v) for v in np.asarray(P, np.float64).reshape(12)]
    X, xy = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(xy, np.float32).reshape(-1, 2)
    verdict, dist = np.zeros(len(X), bool), np.full(len(X), np.inf)
    head = ("pnp", np.asarray(P, np.float64).tobytes(), float(cx), float(cy), float(fx_inv), float(thr2))
    for i in range(len(X)):
        if not (np.isfinite(X[i]).all() and np.isfinite(xy[i]).all()):
            continue
        key = head + (X[i].tobytes(), xy[i].tobytes())                 # (the rows of one scene share most points and often the pose)
        if key in _exact:
            verdict[i], dist[i] = _exact[key]
            continue
        Xi = [f(v) for v in X[i]]
        x, y = (f(xy[i, 0]) - f(cx)) * f(fx_inv), (f(xy[i, 1]) - f(cy)) * f(fx_inv)
        U = Pm[0] * Xi[0] + Pm[1] * Xi[1] + Pm[2] * Xi[2] + Pm[9]
        V = Pm[3] * Xi[0] + Pm[4] * Xi[1] + Pm[5] * Xi[2] + Pm[10]
        W = Pm[6] * Xi[0] + Pm[7] * Xi[1] + Pm[8] * Xi[2] + Pm[11]
        lhs, rhs = (U - x * W) ** 2 + (V - y * W) ** 2, f(thr2) * W * W
        verdict[i] = bool(W > 0 and rhs <= f(DBL_MAX) and lhs <= rhs)
        wscale = mp.sqrt(Pm[6] ** 2 + Pm[7] ** 2 + Pm[8] ** 2) * mp.sqrt(Xi[0] ** 2 + Xi[1] ** 2 + Xi[2] ** 2) + abs(Pm[11])
        dist[i] = min(_rel(mp, lhs, rhs), float(abs(W) / wscale) if wscale != 0 else 0.0)
        _exact[key] = (verdict[i], dist[i])
    return verdict, dist


def exact_inlier_h(H, x1, x2, cx, cy, fx_inv, t_h):
    """(verdict bool[m], distance float[m]) of the homography transfer test under H (9 doubles, any scale): (U - u w)^2 + (V - v w)^2 <= t_h (w w)
    with (U, V, w) = H (x, y, 1), and the same with G = adj(H) on the second image's point against the first's; an inlier passes both.
    Coordinates are (u - c) fx_inv.  A correspondence with a non-finite coordinate does not pass (distance inf).  distance = the smaller
    |lhs - rhs| / rhs of the two tests"""
    mp = _mp()
    f = lambda v: mp.mpf(float(v))
    Hm = [f(v) for v in np.asarray(H, np.float64).reshape(9)]
    c = [[Hm[0], Hm[3], Hm[6]], [Hm[1], Hm[4], Hm[7]], [Hm[2], Hm[5], Hm[8]]]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    Gm = cross(c[1], c[2]) + cross(c[2], c[0]) + cross(c[0], c[1])
    x1, x2 = np.asarray(x1, np.float32).reshape(-1, 2), np.asarray(x2, np.float32).reshape(-1, 2)
    verdict, dist = np.zeros(len(x1), bool), np.full(len(x1), np.inf)

    def one(M, x, y, u, v):
        U, V, w = M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5], M[6] * x + M[7] * y + M[8]
        return (U - u * w) ** 2 + (V - v * w) ** 2, f(t_h) * w * w
    head = ("h", np.asarray(H, np.float64).tobytes(), float(cx), float(cy), float(fx_inv), float(t_h))
    for i in range(len(x1)):
        if not (np.isfinite(x1[i]).all() and np.isfinite(x2[i]).all()):
            continue
        key = head + (x1[i].tobytes(), x2[i].tobytes())
        if key in _exact:
            verdict[i], dist[i] = _exact[key]
            continue
        a, b = (f(x1[i, 0]) - f(cx)) * f(fx_inv), (f(x1[i, 1]) - f(cy)) * f(fx_inv)
        u, v = (f(x2[i, 0]) - f(cx)) * f(fx_inv), (f(x2[i, 1]) - f(cy)) * f(fx_inv)
        lf, rf = one(Hm, a, b, u, v)
        lb, rb = one(Gm, u, v, a, b)
        verdict[i] = bool(lf <= rf and lb <= rb)
        dist[i] = min(_rel(mp, lf, rf), _rel(mp, lb, rb))
        _exact[key] = (verdict[i], dist[i])
    return verdict, dist


def check_exact(mask, verdict, dist, where):
    """the mask equals the exact verdict; no point of the row may lie within MARGIN of the threshold (change the seed, not the margin)"""
    near = np.flatnonzero(dist <= MARGIN)
    assert len(near) == 0, (where, "points within the margin of the threshold", near.tolist(), dist[near].tolist())
    bad = np.flatnonzero((np.asarray(mask) != 0) != verdict)
    assert len(bad) == 0, (where, "mask differs from the exact predicate at", bad.tolist(), dist[bad].tolist())


# ---- the rows of both suites --------------------------------------------------------------------------------------------------------
# Each family: one finite scene of 40 correspondences (layouts stride5, first3, all) and one of tile + 1 (layout tile_edge); the restatement
# runs once per (kind, layout) and both suites read the cached result.
TILE = 512                                                             # VIS_PNP_TILE = VIS_F2F_TILE = VIS_H_TILE (the GPU suite asserts it)
M = 40
ITERS = 200
_cache = {}


def row_layouts():
    """(layout, m) of every hostile row of a family"""
    return [("stride5", M), ("first3", M), ("all", M), ("tile_edge", TILE + 1)]


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pnp_base(m):
    import pnp_ref as pr
    X, xy, _, R, t = pr.make_scene("general", m, 0.3, 0.0)
    return dict(X=X, xy=xy, R=R, t=t)


def pnp_draws():
    import pnp_ref as pr
    return pr.make_draws(7, ITERS)


def pnp_rows():
    """{(kind, layout): dict(X, xy, idx, rec, mask)} and {m: (rec, mask)} of the clean rows: tests/pnp_ref.py at the default parameters"""
    def make():
        import pnp_ref as pr
        cam, pp, draws = pr.Camera(), pr.default_params(), pnp_draws()
        rows, clean = {}, {}
        for lay, m in row_layouts():
            base = _once(("pnp_base", m), lambda: pnp_base(m))
            if m not in clean:
                clean[m] = pr.pnp(cam, pp, base["X"], base["xy"], draws)
            idx = layout(lay, m, TILE)
            for kind in pnp_kinds():
                h = hostile(kind, base, idx)
                rec, mask = pr.pnp(cam, pp, h["X"], h["xy"], draws)
                rows[kind, lay] = dict(X=h["X"], xy=h["xy"], idx=idx, rec=rec, mask=mask)
            for kind in (mag_pnp_kinds() if lay in MAG_LAYOUTS else ()):
                h = hostile(kind, base, idx)
                with np.errstate(all="ignore"):
                    rec, mask = pr.pnp(cam, pp, h["X"], h["xy"], draws)
                rows[kind, lay] = dict(X=h["X"], xy=h["xy"], idx=idx, rec=rec, mask=mask)
        return rows, clean
    return _once("pnp_rows", make)


def h_base(m):
    import homography_ref as hr
    x1, x2, _ = hr.make_rows("plane", m, 0.3, 0.0)
    return dict(p1=x1, p2=x2)


def h_draws():
    import homography_ref as hr
    return hr.make_draws(7, ITERS)


def h_rows():
    """{(kind, layout): dict(p1, p2, idx, rec, mask)} and {m: (rec, mask)} of the clean rows: tests/homography_ref.py, no E"""
    def make():
        import homography_ref as hr
        cam, hp, draws = hr.Camera(), hr.default_params(), h_draws()
        rows, clean = {}, {}
        for lay, m in row_layouts():
            base = _once(("h_base", m), lambda: h_base(m))
            if m not in clean:
                clean[m] = hr.homography(cam, hp, base["p1"], base["p2"], draws)
            idx = layout(lay, m, TILE)
            for kind in pair_kinds() + (mag_pair_kinds() if lay in MAG_LAYOUTS else []):
                h = hostile(kind, base, idx)
                with np.errstate(all="ignore"):
                    rec, mask = hr.homography(cam, hp, h["p1"], h["p2"], draws)
                rows[kind, lay] = dict(p1=h["p1"], p2=h["p2"], idx=idx, rec=rec, mask=mask)
        return rows, clean
    return _once("h_rows", make)


def f2f_base(m):
    import f2f_ref as fr
    a, b, rot, t = fr.pair_inputs(m, 3, 0.0, 0.3)
    return dict(p1=a, p2=b, rot=rot, t=t)


def f2f_draws():
    return np.random.default_rng(5).integers(0, 2 ** 31, (ITERS, 2)).astype(np.int32)


FILTER_THRESHOLD = 500.0


def f2f_rows(p):
    """{(kind, layout): dict(p1, p2, rot, t, idx, rec, keep, nkeep)} and {m: the same of the clean row}: tests/f2f_ref.py with the true
    translation as reference (p: vis_params with fy = fx, f2f_iters = ITERS); keep = FilterKeypoints under (rot, t) at FILTER_THRESHOLD"""
    def make():
        import f2f_ref as fr
        assert int(p.f2f_iters) == ITERS and p.fy == p.fx
        draws = f2f_draws()
        rows, clean = {}, {}

        def one(a, b, base, idx):
            with np.errstate(all="ignore"):
                rec = fr.f2f(p, a, b, base["rot"], draws, base["t"])
                keep, nk = fr.filter_keypoints(p, a, b, base["rot"], base["t"], FILTER_THRESHOLD)
            return dict(p1=a, p2=b, rot=base["rot"], t=base["t"], idx=idx, rec=rec, keep=keep, nkeep=nk)
        for lay, m in row_layouts():
            base = _once(("f2f_base", m), lambda: f2f_base(m))
            if m not in clean:
                clean[m] = one(base["p1"], base["p2"], base, np.zeros(0, np.int64))
            idx = layout(lay, m, TILE)
            for kind in pair_kinds() + (mag_pair_kinds() if lay in MAG_LAYOUTS else []):
                h = hostile(kind, base, idx)
                rows[kind, lay] = one(h["p1"], h["p2"], base, idx)
        return rows, clean
    return _once("f2f_rows", make)


ESSENTIAL_LENGTHS = (40, 64, 257, 300)                                 # the work-list kernels carry hostile and clean rows together
ESSENTIAL_LAYOUTS = ("stride5", "first3", "all")
ESSENTIAL_MAG_LENGTHS = (40, 257, 300)


def essential_base(m):
    import essential_refine_ref as er
    x1, x2, R, t = er.make_scene("general", m, 0.3, 0.0, seed=100)
    return dict(p1=x1, p2=x2, R=R, t=t)


def essential_rows(orc, op):
    """{(kind, layout, m): dict(p1, p2, idx, E, mask, n_inliers, iters_run, R, t, n_pose_good)} and {m: the same of the clean row}: the CPU
    oracle's essential_ransac + recover_pose (op: the oracle's parameters, adaptive mode, the camera of the scenes).  Every kind at 40; at
    the longer lengths the kinds on both images, which is what the device suite interleaves"""
    def make():
        rows, clean = {}, {}

        def one(a, b, idx):
            E, mask, ninl, iters = orc.essential_ransac(op, a, b)
            R, t, ngood = orc.recover_pose(op, E, a, b)
            return dict(p1=a, p2=b, idx=idx, E=E.reshape(9).copy(), mask=mask.copy(), n_inliers=ninl, iters_run=iters, R=R.reshape(9).copy(),
                        t=t.copy(), n_pose_good=ngood)
        for m in ESSENTIAL_LENGTHS:
            base = _once(("essential_base", m), lambda: essential_base(m))
            clean[m] = one(base["p1"], base["p2"], np.zeros(0, np.int64))
            for lay in ESSENTIAL_LAYOUTS:
                idx = layout(lay, m)
                for kind in pair_kinds():
                    if m != M and not kind.startswith("both:"):
                        continue
                    h = hostile(kind, base, idx)
                    rows[kind, lay, m] = one(h["p1"], h["p2"], idx)
                # the magnitude ladder: on one image (where the single-precision scorer's radii overflowed alone), at 40 and at the
                # lengths above 256 -- the staged form and the ballot form of k_hyp_score
                for kind in (mag_pair_kinds() if lay in MAG_LAYOUTS and m in ESSENTIAL_MAG_LENGTHS else []):
                    h = hostile(kind, base, idx)
                    rows[kind, lay, m] = one(h["p1"], h["p2"], idx)
        return rows, clean
    return _once("essential_rows", make)


def tri_base():
    import triangulate_ref as tr
    R, t, p1, p2, _ = tr.scene(1, n=M)
    return dict(p1=p1, p2=p2, R=R, t=t)


def tri_rows():
    """{(kind, layout): dict(p1, p2, R, t, idx, pts, flags, summary)} and the clean row: tests/triangulate_ref.py, EuRoC camera with fy = fx"""
    def make():
        import triangulate_ref as tr
        K = tr.EUROC
        base = _once("tri_base", tri_base)

        def one(a, b, idx, t=None):
            t = base["t"] if t is None else t
            with np.errstate(all="ignore"):
                pts, fl, sm, _ = tr.triangulate(base["R"], t, a, b, K["fx"], K["fx"], K["cx"], K["cy"])
            return dict(p1=a, p2=b, R=base["R"], t=t, idx=idx, pts=pts, flags=fl, summary=sm)
        rows = {}
        clean = one(base["p1"], base["p2"], np.zeros(0, np.int64))
        for lay in ("stride5", "first3", "all"):
            idx = layout(lay, M)
            for kind in pair_kinds() + (mag_pair_kinds() if lay in MAG_LAYOUTS else []):
                h = hostile(kind, base, idx)
                rows[kind, lay] = one(h["p1"], h["p2"], idx)
        rows["t:zero", "none"] = one(base["p1"], base["p2"], np.zeros(0, np.int64), np.zeros(3))
        return rows, clean
    return _once("tri_rows", make)


# ---- the properties of a record on a hostile row: asserted on the restatements' output and on the device's alike -------------------------
# a hostile entry of these kinds is unusable whatever the pose: it may never be an inlier.  (A point at the camera centre or a duplicate of a
# true point, a correspondence that did not move, and an `all` row of finite wrong points are ordinary data: the exact predicate decides.)
PNP_NEVER = tuple(f"X:{k}" for k in NONFINITE + ("x1e200", "x1e160", "x1e150", "mirror")) + tuple(f"xy:{k}" for k in NONFINITE + ("big",))
PNP_NO_WINNER = tuple(f"X:{k}" for k in NONFINITE + ("x1e200", "x1e160")) + tuple(f"xy:{k}" for k in NONFINITE)
PAIR_NEVER = tuple(k for k in pair_kinds() if k.split(":")[1] in NONFINITE + ("big",))
PAIR_NONFINITE = tuple(k for k in pair_kinds() if k.split(":")[1] in NONFINITE)


def orthonormal(R):
    R = np.asarray(R, np.float64).reshape(3, 3)
    return bool(np.isfinite(R).all()) and float(np.abs(R @ R.T - np.eye(3)).max()) < 1e-9


def check_pnp_row(kind, lay, row, rec, mask):
    """the properties of one PnP record and mask (restatement's or device's) on a hostile row"""
    where = ("pnp", kind, lay)
    idx, m = row["idx"], len(row["X"])
    assert int(rec["n_points"]) == m and int(rec["n_inliers"]) == int(mask.sum()), where
    if kind in PNP_NEVER and not (lay == "all" and kind in ("X:x1e150", "X:mirror", "xy:big")):
        assert not mask[idx].any(), (where, np.flatnonzero(mask[idx]))
    if lay == "all" and kind in PNP_NO_WINNER:
        want = pr.zero_record()
        want["n_points"], want["n_degenerate"] = m, ITERS
        assert rec.tobytes() == want.tobytes() and not mask.any(), (where, rec)
    if int(rec["best_iter"]) < 0:
        assert not mask.any() and int(rec["n_inliers"]) == 0, where
        return
    assert orthonormal(rec["R"]) and orthonormal(rec["R_ransac"]) and np.isfinite(rec["t"]).all() and np.isfinite(rec["t_ransac"]).all(), where
    assert np.isfinite(float(rec["cost0"])) and np.isfinite(float(rec["cost1"])), (where, rec["cost0"], rec["cost1"])
    cam, pp = pr.Camera(), pr.default_params()
    fx_inv, thr2 = pr.thresholds(cam, pp)
    P = list(rec["R_ransac"]) + list(rec["t_ransac"])
    key = ("exact", where, np.asarray(P, np.float64).tobytes())        # (once per pose and row: the device's pose has the restatement's bytes)
    check_exact(mask, *_once(key, lambda: exact_inlier_pnp(P, row["X"], row["xy"], cam.cx, cam.cy, fx_inv, thr2)), where)


_votes = {}


def hpose_of(cam, rec, x1, x2, mask):
    """tests/homography_pose_ref.py's record of a homography record, its correspondences and mask; the votes of a correspondence under a
    candidate are computed once per (H, correspondence): the rows of one scene share most of both"""
    hq = hpr.default_params()
    table = None
    if int(rec["best_iter"]) >= 0 and len(x1) >= 1 and np.isfinite(rec["H"]).all():
        dec = hpr.decompose(rec["H"], hq.min_t_over_d)
        if dec["kind"] == hpr.HP_PLANE:
            with np.errstate(all="ignore"):
                norm = hr.normalise(cam, x1, x2)
            m = len(x1)
            good, par = np.zeros((4, m), bool), np.zeros((4, m), bool)
            cands = [(hpr.candidate(dec, k)[0], hpr.candidate(dec, k)[1]) for k in range(4)]
            head = np.asarray(rec["H"], np.float64).tobytes()
            for i in range(m):
                q = tuple(float(norm[j][i]) for j in range(4))
                if (head, q) not in _votes:
                    _votes[head, q] = [hpr.vote_point(R, t, hpr.rt_t(R, t), *q, hq.max_cos_parallax) for R, t in cands]
                for k in range(4):
                    good[k, i], par[k, i] = _votes[head, q][k]
            table = (good, par)
    return hpr.hpose(cam, hq, rec, x1, x2, mask, None, table)


def check_h_row(kind, lay, row, rec, mask):
    """the properties of one homography record and mask on a hostile row, and of the pose decomposed from the record"""
    where = ("homography", kind, lay)
    idx, m = row["idx"], len(row["p1"])
    assert int(rec["n_points"]) == m and int(rec["n_inliers"]) == int(mask.sum()), where
    if kind in PAIR_NEVER:
        assert not mask[idx].any(), (where, np.flatnonzero(mask[idx]))
    if lay == "all" and kind in PAIR_NEVER:
        want = hr.zero_record()
        want["n_points"], want["n_degenerate"] = m, ITERS
        assert rec.tobytes() == want.tobytes() and not mask.any(), (where, rec)
    cam = hr.Camera()
    key = ("hpose", where, np.asarray(rec["H"], np.float64).tobytes(), int(rec["best_iter"]), np.asarray(mask, np.uint8).tobytes())
    pose = _once(key, lambda: hpose_of(cam, rec, row["p1"], row["p2"], mask))
    if int(rec["best_iter"]) < 0:
        assert not mask.any() and pose.tobytes() == hpr.zero_record().tobytes(), where
        return pose
    assert np.isfinite(rec["H"]).all() and abs(float(np.linalg.norm(rec["H"])) - 1.0) < 1e-12, where
    if int(pose["kind"]) != hpr.HP_NONE:
        assert orthonormal(pose["R"]) and np.isfinite(pose["t"]).all() and np.isfinite(pose["n"]).all(), (where, pose)
        assert int(pose["n_tested"]) == int(mask.sum()) or int(pose["kind"]) == hpr.HP_ROTATION, (where, pose)
    fx_inv, _, t_h, _, _ = hr.thresholds(cam, hr.default_params())
    key = ("exact", where, np.asarray(rec["H"], np.float64).tobytes())
    check_exact(mask, *_once(key, lambda: exact_inlier_h(rec["H"], row["p1"], row["p2"], cam.cx, cam.cy, fx_inv, t_h)), where)
    return pose


def check_f2f_row(kind, lay, row, rec, keep, nkeep):
    where = ("f2f", kind, lay)
    idx, m = row["idx"], len(row["p1"])
    assert int(rec["n_points"]) == m and 0 <= int(rec["count_max"]) <= m and int(nkeep) == int(np.asarray(keep).sum()), where
    if kind in PAIR_NONFINITE:
        assert int(rec["count_max"]) <= m - len(idx) and not np.asarray(keep)[idx].any(), where     # a NaN normal is no inlier of any direction
        if lay == "all":
            assert int(rec["count_max"]) == 0 and int(rec["best_iter"]) == -1 and int(rec["flipped"]) == 0 and int(nkeep) == 0, where
            assert not np.asarray(rec["t"], np.float32).any(), where
    if int(rec["best_iter"]) >= 0:
        t = np.asarray(rec["t"], np.float64)
        assert np.isfinite(t).all() and abs(float(np.linalg.norm(t)) - float(np.linalg.norm(row["t"].astype(np.float64)))) < 1e-6, where


def check_tri_row(kind, lay, row, pts, flags, summary):
    where = ("triangulate", kind, lay)
    idx = row["idx"]
    get = (lambda k: summary[k]) if isinstance(summary, (dict, np.void)) else (lambda k: getattr(summary, k))
    assert int(get("n_points")) == len(row["p1"]), where
    assert int(get("n_front")) == int(((flags & tr.MP_FRONT) != 0).sum()) and int(get("n_kept")) == int(((flags & tr.MP_KEPT) != 0).sum()), where
    name = kind.split(":")[1]
    if kind in PAIR_NEVER:
        assert not (flags[idx] & tr.MP_KEPT).any(), (where, flags[idx])
    mean = np.float32(get("mean_parallax_px"))
    if name == "nan":                                                  # as the reference: Disparity sums every point, so one NaN makes the mean NaN
        assert np.isnan(mean) and (flags[idx] == tr.MP_INLIER).all(), (where, mean, flags[idx])
    if kind == "p1:big":                                               # as the reference: a finite float parallax of 1e38 sums to +inf
        assert mean == np.float32(np.inf) and (flags[idx] & tr.MP_FRONT).any(), (where, mean, flags[idx])
    clean = np.setdiff1d(np.arange(len(flags)), idx)
    assert (flags[clean] & tr.MP_KEPT).all() or kind == "t:zero", where       # the other points of the row are what they were


def check_essential_row(kind, lay, m, row, E, mask, ninl, iters, R, t, ngood, max_iters):
    where = ("essential", kind, lay, m)
    idx = row["idx"]
    E, R, t = np.asarray(E, np.float64).reshape(9), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)
    assert int(ninl) == int(np.asarray(mask).sum()) and np.isfinite(E).all(), where
    if kind in PAIR_NONFINITE or (kind in PAIR_NEVER and lay != "all"):   # (a whole row of +-3e38 is two finite points: a model may explain it)
        assert not np.asarray(mask)[idx].any(), (where, np.flatnonzero(np.asarray(mask)[idx]))
    if (mag_of(kind) or 0.0) >= MAG_NEVER_FROM:                        # (the scenes are chosen so that none lies on the winner's epipolar line)
        assert not np.asarray(mask)[idx].any(), (where, np.flatnonzero(np.asarray(mask)[idx]))
    if lay == "all" and kind in PAIR_NONFINITE:
        assert not E.any() and int(ninl) == 0 and int(iters) == max_iters and int(ngood) == 0, (where, ninl, iters)
    if E.any():
        assert orthonormal(R) and np.isfinite(t).all() and abs(float(np.linalg.norm(t)) - 1.0) < 1e-9, where
