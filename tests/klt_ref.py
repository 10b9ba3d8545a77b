"""The pyramidal KLT contract of include/vislam_hip.h restated in numpy, operation for operation: integer sums as int64, everything else
double arithmetic in the header's order.  Vectorised over the points of a pair (each point's arithmetic is independent of the others).

track(kp, f1, f2, pts, guess) -> records (POINT_DTYPE); pair_record(records) and compact(pts, records) restate k_klt_pairs.
A frame is (gray, gx, gy): three lists of five level arrays (uint8, int16, int16); gx / gy of frame 2 are only read by the backward pass."""
import ctypes as C

import numpy as np

TRACKED, OOB, FLAT, ERR, FB, INVALID = 1, 2, 4, 8, 16, 32
NO_PAIR = 1
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("fb", "<f4"), ("min_eig", "<f4"), ("sad", "<i4"), ("flags", "<i4"), ("iters", "<u2"),
                        ("levels", "u1"), ("pad_", "u1", (5,))])
PAIR_DTYPE = np.dtype([("n_points", "<i4"), ("n_tracked", "<i4"), ("n_oob", "<i4"), ("n_flat", "<i4"), ("n_err", "<i4"), ("n_fb", "<i4"),
                       ("n_invalid", "<i4"), ("flags", "<i4")])


class Params(C.Structure):
    _fields_ = [("win_radius", C.c_int32), ("first_level", C.c_int32), ("last_level", C.c_int32), ("max_iters", C.c_int32),
                ("epsilon", C.c_double), ("min_eig", C.c_double), ("max_err", C.c_double), ("fb_max_px", C.c_double),
                ("scharr_scale", C.c_int32), ("reserved_", C.c_int32)]


P_FIELDS = tuple(f for f, _ in Params._fields_)


def default_params():
    return Params(7, 3, 0, 10, 0.01, 0.1, 0.0, 0.0, 3, 0)


def copy_params(kp, **kw):
    q = Params(*[getattr(kp, f) for f in P_FIELDS])
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def half_dims(w, h):
    """vis_half_pyramid_dims: cvRound(n * 0.5), half to even"""
    half = lambda n: (n >> 1) + ((n & 1) & ((n >> 1) & 1))
    lw, lh = [w], [h]
    for _ in range(4):
        lw.append(half(lw[-1]))
        lh.append(half(lh[-1]))
    return lw, lh


def level_pos(p0, l):
    return (p0 + 0.5) / float(1 << l) - 0.5


def fits(x, y, r, lw, lh):
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        return fin & (fx - float(r) >= 0.0) & (fy - float(r) >= 0.0) & (fx + float(r) + 1.0 <= float(lw - 1)) & (fy + float(r) + 1.0 <= float(lh - 1))


def taps(x, y):
    """(X, Y, w00, w01, w10, w11) as int64 arrays"""
    fx, fy = np.floor(x), np.floor(y)
    a, b = x - fx, y - fy
    w00 = np.rint(((1.0 - a) * (1.0 - b)) * 16384.0).astype(np.int64)
    w01 = np.rint((a * (1.0 - b)) * 16384.0).astype(np.int64)
    w10 = np.rint(((1.0 - a) * b) * 16384.0).astype(np.int64)
    return fx.astype(np.int64), fy.astype(np.int64), w00, w01, w10, 16384 - w00 - w01 - w10


def sample(img, x, y, r):
    """S of every window pixel: (k, 2r+1, 2r+1) int64, rows j, columns i"""
    X, Y, w00, w01, w10, w11 = taps(x, y)
    o = np.arange(-r, r + 1)
    rows = (Y[:, None, None] + o[None, :, None])
    cols = (X[:, None, None] + o[None, None, :])
    im = img.astype(np.int64)
    assert rows.min(initial=0) >= 0 and cols.min(initial=0) >= 0 and rows.max(initial=0) + 1 < im.shape[0] and cols.max(initial=0) + 1 < im.shape[1]
    w = lambda v: v[:, None, None]
    return w(w00) * im[rows, cols] + w(w01) * im[rows, cols + 1] + w(w10) * im[rows + 1, cols] + w(w11) * im[rows + 1, cols + 1]


def intensity(img, x, y, r):
    return (sample(img, x, y, r) + 256) >> 9


def gradient(img, x, y, r):
    return (sample(img, x, y, r) + 8192) >> 14


SUMS = ("gxx", "gxy", "gyy", "bx", "by")


def _pass(kp, A, B_gray, start, guess, wrap=None):
    """one pass over the finite starts `start` (k x 2 float64): template frame A = (gray, gx, gy), target intensities B_gray.
    wrap = one of SUMS: that sum is taken modulo 2^32 (what an int accumulator would hold) -- a deliberately wrong variant, for the tests
    that prove a scene reaches beyond 32 bits (tests/test_klt_limits_ref.py)"""
    assert wrap is None or wrap in SUMS
    isum = lambda name, v: (v.astype(np.int32).astype(np.int64) if wrap == name else v).astype(np.float64)
    k = len(start)
    r, first, last = kp.win_radius, kp.first_level, kp.last_level
    n = (2 * r + 1) ** 2
    s = float(kp.scharr_scale)
    eps2 = kp.epsilon * kp.epsilon
    lam_den = ((2.0 * n) * (32.0 * s)) * (32.0 * s)
    d = np.zeros((k, 2))
    if guess is not None:
        hg = np.isfinite(guess).all(1)
        d[hg] = (guess[hg] - start[hg]) / float(1 << first)
    lost, iters, levels, sad = (np.zeros(k, np.int64) for _ in range(4))
    lam_last, have_lam = np.zeros(k), np.zeros(k, bool)
    for l in range(first, last - 1, -1):
        at_last = l == last
        if l < first:
            d = 2.0 * d
        p = level_pos(start, l)
        lh, lw = A[0][l].shape
        fit = fits(p[:, 0], p[:, 1], r, lw, lh)
        if at_last:
            lost[~fit] = OOB
        idx = np.nonzero(fit)[0]
        if not len(idx):
            continue
        T = intensity(A[0][l], p[idx, 0], p[idx, 1], r)
        Dx = gradient(A[1][l], p[idx, 0], p[idx, 1], r)
        Dy = gradient(A[2][l], p[idx, 0], p[idx, 1], r)
        fxx = isum("gxx", (Dx * Dx).sum((1, 2)))
        fxy = isum("gxy", (Dx * Dy).sum((1, 2)))
        fyy = isum("gyy", (Dy * Dy).sum((1, 2)))
        det = fxx * fyy - fxy * fxy
        lam = ((fxx + fyy) - np.sqrt((fxx - fyy) * (fxx - fyy) + 4.0 * (fxy * fxy))) / lam_den
        if at_last:
            lam_last[idx], have_lam[idx] = lam, True
        ok = (det > 0.0) & (lam >= kp.min_eig)
        if at_last:
            lost[idx[~ok]] = FLAT
        idx, T, Dx, Dy, fxx, fxy, fyy, det = idx[ok], T[ok], Dx[ok], Dy[ok], fxx[ok], fxy[ok], fyy[ok], det[ok]
        levels[idx] |= 1 << l
        active = np.ones(len(idx), bool)
        for _ in range(kp.max_iters):
            if not active.any():
                break
            q = p[idx] + d[idx]
            f = fits(q[:, 0], q[:, 1], r, lw, lh)
            if at_last:
                lost[idx[active & ~f]] = OOB
            active &= f
            a = np.nonzero(active)[0]
            if not len(a):
                break
            e = intensity(B_gray[l], q[a, 0], q[a, 1], r) - T[a]
            bx = isum("bx", (Dx[a] * e).sum((1, 2)))
            by = isum("by", (Dy[a] * e).sum((1, 2)))
            ux = -(s * (fyy[a] * bx - fxy[a] * by)) / det[a]
            uy = -(s * (fxx[a] * by - fxy[a] * bx)) / det[a]
            d[idx[a], 0] = d[idx[a], 0] + ux
            d[idx[a], 1] = d[idx[a], 1] + uy
            iters[idx[a]] += 1
            active[a[ux * ux + uy * uy <= eps2]] = False
        if at_last:
            keep = lost[idx] == 0
            idx, T = idx[keep], T[keep]
            q = p[idx] + d[idx]
            f = fits(q[:, 0], q[:, 1], r, lw, lh)
            lost[idx[~f]] = OOB
            g = np.nonzero(f)[0]
            if len(g):
                sad[idx[g]] = np.abs(intensity(B_gray[l], q[g, 0], q[g, 1], r) - T[g]).sum((1, 2))
    end = start + d * float(1 << last)
    return dict(lost=lost, end=end, sad=sad, lam=lam_last, have_lam=have_lam, iters=iters, levels=levels)


def track(kp, f1, f2, pts, guess=None, wrap=None):
    """records of the points `pts` (m x 2 float32) of frame f1 tracked into frame f2 (wrap: see _pass; None is the contract)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    m = len(pts)
    rec = np.zeros(m, POINT_DTYPE)
    p0_all = pts.astype(np.float64)
    valid = np.isfinite(p0_all).all(1)
    rec["flags"][~valid] = INVALID
    v = np.nonzero(valid)[0]
    if not len(v):
        return rec
    p0 = p0_all[v]
    g = None if guess is None else np.asarray(guess, np.float32).reshape(m, 2).astype(np.float64)[v]
    n = (2 * kp.win_radius + 1) ** 2
    fw = _pass(kp, f1, f2[0], p0, g, wrap)
    flags = fw["lost"].copy()
    res = np.where((flags == 0)[:, None], fw["end"], p0).astype(np.float32)
    sad = np.where(flags == 0, fw["sad"], 0)
    if kp.max_err > 0.0:
        flags[(flags == 0) & (sad.astype(np.float64) > (kp.max_err * 32.0) * float(n))] |= ERR
    fb = np.zeros(len(v), np.float32)
    if kp.fb_max_px > 0.0:
        b = np.nonzero(flags == 0)[0]
        if len(b):
            bw = _pass(kp, f2, f1[0], res[b].astype(np.float64), p0[b], wrap)
            dd = bw["end"] - p0[b]
            d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]
            lostb = bw["lost"] != 0
            fb[b] = np.where(lostb, -1.0, np.sqrt(d2)).astype(np.float32)
            flags[b[lostb | (d2 > kp.fb_max_px * kp.fb_max_px)]] |= FB
    flags[flags == 0] = TRACKED
    rec["x"][v], rec["y"][v] = res[:, 0], res[:, 1]
    rec["fb"][v] = fb
    rec["min_eig"][v] = np.where(fw["have_lam"], fw["lam"], 0.0).astype(np.float32)
    rec["sad"][v], rec["flags"][v] = sad, flags
    rec["iters"][v], rec["levels"][v] = fw["iters"], fw["levels"]
    return rec


def pair_record(rec, no_pair=False):
    out = np.zeros(1, PAIR_DTYPE)
    if no_pair:
        out["flags"] = NO_PAIR
        return out[0]
    out["n_points"] = len(rec)
    for name, bit in (("n_tracked", TRACKED), ("n_oob", OOB), ("n_flat", FLAT), ("n_err", ERR), ("n_fb", FB), ("n_invalid", INVALID)):
        out[name] = int(((rec["flags"] & bit) != 0).sum())
    return out[0]


def compact(pts, rec):
    """(p1, p2): the tracked points in rising index, frame-1 input and frame-2 result, float32"""
    t = (rec["flags"] & TRACKED) != 0
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    return pts[:len(rec)][t].copy(), np.stack([rec["x"][t], rec["y"][t]], 1).astype(np.float32)


def frame_from(orc, img, scale=3):
    """(gray, gx, gy) of one image by the CPU oracle's Camera::Update and Camera::computeGradient"""
    pyr = orc.half_pyramid(img)
    gr = [orc.scharr_gradient(lv, scale) for lv in pyr]
    return pyr, [g[0] for g in gr], [g[1] for g in gr]


# ---- analytic scenes: a sum of Gaussian blobs evaluated at shifted coordinates, so the true displacement is exact
def blob_frames(w, h, shifts, seed=5, nblobs=160, flat_box=None):
    """one uint8 image per entry of `shifts`: the scene moved by that shift (a point p of the unmoved scene is at p + shift).
    flat_box = (x0, y0, x1, y1): the blobs near that box are left out (a textureless region).  The blob count scales with the area."""
    rng = np.random.RandomState(seed)
    nblobs = max(4, int(round(nblobs * (w * h) / (160.0 * 120.0))))
    cx, cy = rng.uniform(-20, w + 20, nblobs), rng.uniform(-20, h + 20, nblobs)
    sg, am = rng.uniform(3.0, 8.0, nblobs), rng.uniform(25.0, 70.0, nblobs) * rng.choice([-1.0, 1.0], nblobs)
    if flat_box is not None:
        x0, y0, x1, y1 = flat_box
        keep = ~((cx > x0 - 25) & (cx < x1 + 25) & (cy > y0 - 25) & (cy < y1 + 25))
        cx, cy, sg, am = cx[keep], cy[keep], sg[keep], am[keep]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def render(dx, dy):
        f = np.full((h, w), 128.0)
        for k in range(len(cx)):
            f += am[k] * np.exp(-((xx - dx - cx[k]) ** 2 + (yy - dy - cy[k]) ** 2) / (2.0 * sg[k] * sg[k]))
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return [render(float(dx), float(dy)) for dx, dy in shifts]


def blob_scene(w, h, shift, seed=5, nblobs=160, flat_box=None):
    """(image 1, image 2): image 2 shows the scene of image 1 moved by `shift`"""
    a, b = blob_frames(w, h, [(0.0, 0.0), shift], seed, nblobs, flat_box)
    return a, b
