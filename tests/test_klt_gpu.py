"""GPU: pyramidal KLT (vis_klt_batch / vis_klt_track / vis_batch_klt) against the restatement tests/klt_ref.py, run on the pyramids and
gradients downloaded from the device: point records, pair records and compacted rows byte for byte.  Output buffers are pre-filled with
0xEE and everything the call must not write is checked to keep it.

Scenes: tests/klt_ref.py blob_frames (analytic, with a textureless box) at 160 x 120 (level 3 is 20 x 15: r = 7 fits nowhere, the level is
skipped for every point), 150 x 110 (half-to-even level sizes: level 2 is 38 x 28), both also at a padded stride, and 16 x 16 with r = 2."""
import ctypes as C

import numpy as np
import pytest

import homography_ref as hr
import klt_ref as kr
import stride_range_cases as src

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC = 32
SHIFT = (3.3, -2.2)
FLAT_BOX = (96, 20, 136, 60)                                       # x0, y0, x1, y1 at 160 x 120 (scaled with the frame)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((max(nbytes, 16),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _levels(flat, w, h):
    """one frame of a gradient set -> its five level arrays"""
    lw, lh = kr.half_dims(w, h)
    out, off = [], 0
    for l in range(5):
        out.append(flat[off:off + lw[l] * lh[l]].reshape(lh[l], lw[l]))
        off += lw[l] * lh[l]
    return out


class _Set:
    """n frames on the device at a row stride, their gradient set made by vis_gradient_batch, and the same as host frames for the restatement"""
    def __init__(self, vislam, torch, c, frames, stride, scale):
        self.n, self.h, self.w = frames.shape
        self.stride, self.scale = stride, scale
        fe = vislam.gradient_frame_elems(self.w, self.h)
        self.d_frames = _dev(torch, src.padded(frames, stride))
        self.d_gray = torch.zeros(self.n * fe, dtype=torch.uint8, device="cuda")
        self.d_gx = torch.zeros(self.n * fe, dtype=torch.int16, device="cuda")
        self.d_gy = torch.zeros(self.n * fe, dtype=torch.int16, device="cuda")
        d_g = torch.zeros(self.n * fe, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.gradient_batch(self.d_frames.data_ptr(), self.w, self.h, stride, self.n, self.d_gray.data_ptr(), self.d_gx.data_ptr(), self.d_gy.data_ptr(),
                         d_g.data_ptr(), scale)
        c.batch_sync()
        gray, gx, gy = self.d_gray.cpu().numpy(), self.d_gx.cpu().numpy(), self.d_gy.cpu().numpy()
        self.host = []
        for i in range(self.n):
            g = _levels(gray[i * fe:(i + 1) * fe], self.w, self.h)
            g[0] = frames[i]                                       # level 0 of the intensities is the frame itself
            self.host.append((g, _levels(gx[i * fe:(i + 1) * fe], self.w, self.h), _levels(gy[i * fe:(i + 1) * fe], self.w, self.h)))


_frames_cache, _want_cache = {}, {}


def _frames(w, h, n):
    """A, B, A, B ...: every pair is a shift by SHIFT one way or the other"""
    if (w, h) not in _frames_cache:
        sx, sy = w / 160.0, h / 120.0
        box = None if w < 64 else (FLAT_BOX[0] * sx, FLAT_BOX[1] * sy, FLAT_BOX[2] * sx, FLAT_BOX[3] * sy)
        s = SHIFT if w >= 64 else (0.6, -0.4)
        _frames_cache[(w, h)] = kr.blob_frames(w, h, [(0.0, 0.0), s], nblobs=160 if w >= 64 else 2000, flat_box=box)
    a, b = _frames_cache[(w, h)]
    return np.stack([a if i % 2 == 0 else b for i in range(n)])


def _points(w, h, r, count):
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


def _rows(w, h, r, n, max_pts, npts, seed=0):
    """per pair a different rotation of the point list; (pts n x max_pts x 2, npts, guess with NaN and useless entries mixed in)"""
    base = _points(w, h, r, max_pts)
    pts = np.stack([np.roll(base, 7 * i + seed, axis=0) for i in range(n)])
    sh = np.array(SHIFT if w >= 64 else (0.6, -0.4), np.float32)
    guess = pts + np.where((np.arange(n) % 2 == 1)[:, None, None], sh, -sh).astype(np.float32) + np.float32(0.4)
    guess[:, 2::5, 0] = np.nan                                     # a non-finite guess is treated as absent
    guess[:, 3::11] = np.float32(1e30)                             # a finite absurd one is used: the window leaves the level
    return pts, np.asarray(npts, np.int32), guess.astype(np.float32)


def _want(S, kp, pts, npts, guess, max_pts):
    want = []
    for i in range(1, S.n):
        m = min(max(int(npts[i]), 0), max_pts)
        want.append(kr.track(kp, S.host[i - 1], S.host[i], pts[i, :m], None if guess is None else guess[i, :m]))
    return want


def _launch(vislam, torch, c, S, kp, pts, npts, guess, max_pts, compacted=True):
    """one vis_klt_batch -> (record rows n x max_pts, pair records, p1 rows, p2 rows, ntracked); the guard bytes behind every buffer checked"""
    n = S.n
    d_pts, d_npts = _dev(torch, pts), _dev(torch, npts)
    d_guess = None if guess is None else _dev(torch, guess)
    out, pair = _filled(torch, (n * max_pts + 2) * REC), _filled(torch, (n + 2) * 32)
    p1, p2, nt = _filled(torch, n * max_pts * 8 + 64), _filled(torch, n * max_pts * 8 + 64), _filled(torch, n * 4 + 64)
    vkp = vislam.KltParams(*[getattr(kp, f) for f in kr.P_FIELDS])
    c.klt_batch(S.d_frames.data_ptr(), S.w, S.h, S.stride, n, S.d_gray.data_ptr(), S.d_gx.data_ptr(), S.d_gy.data_ptr(), d_pts.data_ptr(),
                d_npts.data_ptr(), max_pts, out.data_ptr(), pair.data_ptr(), 0 if d_guess is None else d_guess.data_ptr(),
                p1.data_ptr() if compacted else 0, p2.data_ptr() if compacted else 0, nt.data_ptr() if compacted else 0, vkp)
    c.batch_sync()
    raw, praw, r1, r2, rn = (t.cpu().numpy() for t in (out, pair, p1, p2, nt))
    assert (raw[n * max_pts * REC:] == FILL).all() and (praw[n * 32:] == FILL).all()
    assert (r1[n * max_pts * 8:] == FILL).all() and (r2[n * max_pts * 8:] == FILL).all() and (rn[n * 4:] == FILL).all()
    if not compacted:
        assert (r1 == FILL).all() and (r2 == FILL).all() and (rn == FILL).all()
    return (raw[:n * max_pts * REC].view(vislam.KLT_POINT_DTYPE).reshape(n, max_pts), praw[:n * 32].view(vislam.KLT_PAIR_DTYPE),
            r1[:n * max_pts * 8].reshape(n, max_pts * 8), r2[:n * max_pts * 8].reshape(n, max_pts * 8), rn[:n * 4].view(np.int32))


def _compare(got, want, pts, npts, max_pts, where, compacted=True):
    recs, pairs, r1, r2, rn = got
    n = len(recs)
    assert not recs[0].tobytes().strip(b"\0"), where               # row 0: zeroed records, the pair record of no pair
    assert pairs[0].tobytes() == kr.pair_record(None, no_pair=True).tobytes(), where
    flags = 0
    for i in range(1, n):
        m = min(max(int(npts[i]), 0), max_pts)
        w = want[i - 1]
        assert len(w) == m
        if recs[i, :m].tobytes() != w.tobytes():
            bad = [k for k in range(m) if recs[i, k].tobytes() != w[k].tobytes()]
            raise AssertionError((where, i, bad[:5], [(pts[i, k].tolist(), recs[i, k], w[k]) for k in bad[:3]]))
        assert (recs[i, m:].view(np.uint8) == FILL).all(), (where, i)     # records behind the pair's points are left alone
        assert pairs[i].tobytes() == kr.pair_record(w).tobytes(), (where, i, pairs[i])
        if compacted:
            a, b = kr.compact(pts[i, :m], w)
            k = len(a)
            assert int(rn[i]) == k == int(pairs[i]["n_tracked"]), (where, i)
            assert r1[i, :k * 8].tobytes() == a.tobytes() and r2[i, :k * 8].tobytes() == b.tobytes(), (where, i)
            assert (r1[i, k * 8:] == FILL).all() and (r2[i, k * 8:] == FILL).all(), (where, i)
        flags |= int(np.bitwise_or.reduce(w["flags"])) if m else 0
    if compacted:
        assert int(rn[0]) == 0 and (r1[0] == FILL).all() and (r2[0] == FILL).all(), where
    return flags


@pytest.fixture(scope="module")
def c(vislam):
    ctx = vislam.Context(0)
    yield ctx
    ctx.close()


_sets = {}


def _set(vislam, c, w, h, stride, n, scale=3):
    import torch
    key = (w, h, stride, n, scale)
    if key not in _sets:
        _sets[key] = _Set(vislam, torch, c, _frames(w, h, n), stride, scale)
    return _sets[key]


NPTS7 = [3, 96, 0, 1, 4, 5, 105]                                   # per frame; pair 1 has max_pts, the last one more than max_pts (clamped)


@pytest.mark.parametrize("w,h,stride", [(160, 120, 160), (160, 120, 176), (150, 110, 152), (150, 110, 172)], ids=lambda v: str(v))
def test_shapes_point_rows_and_flags(vislam, c, w, h, stride):
    """0, 1, 4, 5, max_pts points and a count above max_pts; integer and fractional coordinates; windows that leave each level on each
    side; the textureless box; NaN, inf and 1e30 coordinates; with a guess (NaN and absurd entries included); all checks on"""
    import torch
    S = _set(vislam, c, w, h, stride, 7)
    assert [a.shape for a in S.host[0][0]][2:4] == ([(30, 40), (15, 20)] if w == 160 else [(28, 38), (14, 19)])
    kp = kr.copy_params(kr.default_params(), fb_max_px=0.002, max_err=0.25)     # bounds inside what these clean scenes give: both flags occur
    pts, npts, guess = _rows(w, h, 7, 7, 96, NPTS7)
    key = (w, h)
    if key not in _want_cache:                                     # the stride changes nothing: one restatement per shape
        _want_cache[key] = _want(S, kp, pts, npts, guess, 96)
    want = _want_cache[key]
    got = _launch(vislam, torch, c, S, kp, pts, npts, guess, 96)
    seen = _compare(got, want, pts, npts, 96, (w, h, stride))
    assert seen == kr.TRACKED | kr.OOB | kr.FLAT | kr.ERR | kr.FB | kr.INVALID, seen
    full = want[0]
    assert (full["levels"] & 8 == 0).all() and (full["levels"] & 4).any() and (full["levels"] == 3).any()     # level 3 never ran; some points skip level 2
    assert (full["flags"] & kr.TRACKED).sum() >= 20
    # without the compacted rows nothing but the records is written
    got2 = _launch(vislam, torch, c, S, kp, pts, npts, guess, 96, compacted=False)
    assert got2[0].tobytes() == got[0].tobytes() and got2[1].tobytes() == got[1].tobytes()


SWEEP = [dict(win_radius=2), dict(win_radius=10), dict(first_level=0), dict(first_level=4), dict(last_level=1), dict(last_level=2, first_level=2),
         dict(max_iters=1), dict(max_iters=30, epsilon=0.0), dict(epsilon=0.0), dict(min_eig=0.0), dict(min_eig=40.0), dict(max_err=0.25),
         dict(fb_max_px=0.002), dict(fb_max_px=2.0, win_radius=10), dict(scharr_scale=1), dict(scharr_scale=8)]


# with a guess only where the parameter changes the levels or the steps: the guess sets where the first level starts, nothing else
CASES = [(ch, False) for ch in SWEEP] + [(ch, True) for ch in SWEEP if set(ch) & {"win_radius", "first_level", "last_level", "max_iters"}]


@pytest.mark.parametrize("change,with_guess", CASES, ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else ("guess" if v else "cold"))
def test_parameter_sweep(vislam, c, change, with_guess):
    import torch
    kp = kr.copy_params(kr.default_params(), **change)
    S = _set(vislam, c, 160, 120, 160, 3, kp.scharr_scale)
    pts, npts, guess = _rows(160, 120, kp.win_radius, 3, 64, [0, 64, 37], seed=3)
    g = guess if with_guess else None
    want = _want(S, kp, pts, npts, g, 64)
    seen = _compare(_launch(vislam, torch, c, S, kp, pts, npts, g, 64), want, pts, npts, 64, change)
    if change.get("min_eig", 0) > 1:                               # a bound no level-0 window of this scene reaches
        assert not seen & kr.TRACKED and seen & kr.FLAT and (want[0]["levels"] & 1 == 0).all() and (want[0]["levels"] & 6).any()
    else:
        assert seen & kr.TRACKED
    if "max_err" in change:
        assert seen & kr.ERR
    if "fb_max_px" in change:
        assert (want[0]["fb"] > 0).any() and (change["fb_max_px"] > 1 or seen & kr.FB)
    if change.get("last_level") == 1:
        assert (want[0]["levels"] & 1 == 0).all() and (want[0]["levels"] & 2).any()


def test_16x16_with_radius_2(vislam, c):
    """levels 16, 8, 4, 2, 1: a 5 x 5 window fits on levels 0 and 1 only; the smaller levels are skipped by the fit rule, not refused"""
    import torch
    kp = kr.copy_params(kr.default_params(), win_radius=2, first_level=4, min_eig=0.01)
    S = _set(vislam, c, 16, 16, 16, 3)
    g = np.array([(x + fx, y + fy) for y in range(1, 15, 2) for x in range(1, 15, 2) for fx, fy in ((0.0, 0.0), (0.4, 0.7))], np.float32)[:64]
    pts = np.stack([g, g, g[::-1]])
    npts = np.array([5, 64, 64], np.int32)
    want = _want(S, kp, pts, npts, None, 64)
    seen = _compare(_launch(vislam, torch, c, S, kp, pts, npts, None, 64), want, pts, npts, 64, "16x16")
    assert seen & kr.TRACKED and seen & kr.OOB
    assert (want[0]["levels"] & 0b11100 == 0).all() and (want[0]["levels"] & 2).any()


def test_single_call_equals_the_batch_row(vislam, c):
    import torch
    S = _set(vislam, c, 150, 110, 152, 7)
    for kp in (kr.default_params(), kr.copy_params(kr.default_params(), fb_max_px=0.002, max_err=0.25, win_radius=10, last_level=1)):
        pts, npts, guess = _rows(150, 110, kp.win_radius, 7, 96, NPTS7)
        recs, pairs = _launch(vislam, torch, c, S, kp, pts, npts, guess, 96)[:2]
        vkp = vislam.KltParams(*[getattr(kp, f) for f in kr.P_FIELDS])
        fb = kp.fb_max_px > 0
        for i in (1, 5, 6):
            m = min(int(npts[i]), 96)
            f1, f2 = S.host[i - 1], S.host[i]
            lo, hi = kp.last_level, kp.first_level
            only = lambda lv: [a if lo <= l <= hi else None for l, a in enumerate(lv)]     # levels outside [last, first] may be NULL
            rec, pair = c.klt_track(150, 110, only(f1[0]), only(f1[1]), only(f1[2]), only(f2[0]), pts[i, :m], only(f2[1]) if fb else None,
                                    only(f2[2]) if fb else None, guess[i, :m], vkp)
            assert rec.tobytes() == recs[i, :m].tobytes() and pair.tobytes() == pairs[i].tobytes(), (i, pair, pairs[i])
    rec, pair = c.klt_track(150, 110, *[S.host[0][k] for k in range(3)], S.host[1][0], np.zeros((0, 2), np.float32))
    assert len(rec) == 0 and not pair.tobytes().strip(b"\0")


# ---------------------------------------------------------------------------------------------- the plan's pairs
PW, PH, PB = 320, 240, 8


def _fetch(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    host = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0     # device to host
    return host


def _plan_launches(vislam, torch, frames, gate, kp):
    """two launches of 8 through vis_batch_run(DETECT | GRADIENT) + vis_batch_klt -> per launch what the call wrote, the pairing, the
    keypoints and the plan's pyramids and gradients as host frames"""
    p = src.plan_params(vislam, PW, PH, gate)
    p.nfeatures = 200
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, PB)
    cap = c.keypoint_capacity(PW, PH)
    dev = _dev(torch, frames)
    fe = vislam.gradient_frame_elems(PW, PH)
    vkp = vislam.KltParams(*[getattr(kp, f) for f in kr.P_FIELDS])
    out = []
    for li in range(2):
        ptr = dev.data_ptr() + li * PB * PW * PH
        c.batch_run(ptr, PB, vislam.STAGE_DETECT | vislam.STAGE_GRADIENT)
        recs, pair = _filled(torch, (PB * cap + 1) * REC), _filled(torch, (PB + 1) * 32)
        p1, p2, nt = _filled(torch, PB * cap * 8 + 16), _filled(torch, PB * cap * 8 + 16), _filled(torch, PB * 4 + 16)
        if li == 0:
            bad = vislam.default_klt_params()
            bad.scharr_scale = 1
            args = (C.c_void_p(ptr), PB, None, cap, C.c_void_p(recs.data_ptr()), C.c_void_p(pair.data_ptr()), None, None, None)
            assert vislam.lib.vis_batch_klt(c._h, C.byref(bad), *args) == -1                                   # the plan's gradients have scale 3
            assert vislam.lib.vis_batch_klt(c._h, C.byref(vkp), C.c_void_p(ptr), PB - 1, *args[2:]) == -5       # VIS_E_STATE: n differs
            assert vislam.lib.vis_batch_klt(c._h, C.byref(vkp), C.c_void_p(ptr), PB, None, cap - 1, *args[4:]) == -4   # VIS_E_CAPACITY
        c.batch_klt(ptr, PB, cap, recs.data_ptr(), pair.data_ptr(), 0, p1.data_ptr(), p2.data_ptr(), nt.data_ptr(), vkp)
        c.batch_sync()
        assert c.batch_status() == 0
        pg, px, py, _, pfe = c.batch_gradients()
        assert pfe == fe
        gray, gx, gy = _fetch(pg, PB * fe), _fetch(px, 2 * PB * fe).view(np.int16), _fetch(py, 2 * PB * fe).view(np.int16)
        host = []
        for i in range(PB):
            g = _levels(gray[i * fe:(i + 1) * fe], PW, PH)
            g[0] = frames[li * PB + i]
            host.append((g, _levels(gx[i * fe:(i + 1) * fe], PW, PH), _levels(gy[i * fe:(i + 1) * fe], PW, PH)))
        raw, praw, r1, r2, rn = (t.cpu().numpy() for t in (recs, pair, p1, p2, nt))
        assert (raw[PB * cap * REC:] == FILL).all() and (praw[PB * 32:] == FILL).all() and (rn[PB * 4:] == FILL).all()
        assert (r1[PB * cap * 8:] == FILL).all() and (r2[PB * cap * 8:] == FILL).all()
        out.append(dict(recs=raw[:PB * cap * REC].view(vislam.KLT_POINT_DTYPE).reshape(PB, cap), pairs=praw[:PB * 32].view(vislam.KLT_PAIR_DTYPE),
                        p1=r1[:PB * cap * 8].reshape(PB, cap * 8), p2=r2[:PB * cap * 8].reshape(PB, cap * 8), nt=rn[:PB * 4].view(np.int32),
                        links=c.batch_get_keyframes(), kps=[c.batch_keypoints(i)[0] for i in range(PB)], host=host, cap=cap))
    # a run without the gradient stage, or without detection, leaves nothing to track on
    c.batch_run(dev.data_ptr(), PB, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    args = (C.byref(vkp), C.c_void_p(dev.data_ptr()), PB, None, cap, C.c_void_p(recs.data_ptr()), C.c_void_p(pair.data_ptr()), None, None, None)
    assert vislam.lib.vis_batch_klt(c._h, *args) == -5
    c.batch_sync()
    c.close()
    return out


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_plan_pairs_equal_the_restatement(vislam, canvas, gate):
    """every keypoint of frame prev[i] tracked into frame i; the pair to the carried frame and the frames without a pair are zeroed rows
    with VIS_KLT_NO_PAIR.  Gate on: frame 7 of the first launch is flat, so frame 8 is paired with the carried frame 6 (no pair here)."""
    import torch
    frames = np.stack([vislam.synth_frame(canvas, t, PW, PH) for t in range(2 * PB)])
    if gate:
        frames[PB - 1] = 128
    kp = kr.copy_params(kr.default_params(), fb_max_px=1.0)
    launches = _plan_launches(vislam, torch, frames, gate, kp)
    n_pairs = n_tracked = 0
    for li, L in enumerate(launches):
        cap = L["cap"]
        for i in range(PB):
            q = int(L["links"][i])
            if q < 0:
                assert not L["recs"][i].tobytes().strip(b"\0"), (li, i)
                assert L["pairs"][i].tobytes() == kr.pair_record(None, no_pair=True).tobytes() and int(L["nt"][i]) == 0, (li, i)
                assert (L["p1"][i] == FILL).all() and (L["p2"][i] == FILL).all()
                continue
            k1 = L["kps"][q]
            m = len(k1)
            assert 0 < m <= cap
            pts = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
            want = kr.track(kp, L["host"][q], L["host"][i], pts)
            assert L["recs"][i, :m].tobytes() == want.tobytes(), (li, i)
            assert (L["recs"][i, m:].view(np.uint8) == FILL).all()
            assert L["pairs"][i].tobytes() == kr.pair_record(want).tobytes(), (li, i)
            a, b = kr.compact(pts, want)
            k = len(a)
            assert int(L["nt"][i]) == k and L["p1"][i, :k * 8].tobytes() == a.tobytes() and L["p2"][i, :k * 8].tobytes() == b.tobytes()
            assert (L["p1"][i, k * 8:] == FILL).all() and (L["p2"][i, k * 8:] == FILL).all()
            n_pairs += 1
            n_tracked += k
    links = [list(map(int, L["links"])) for L in launches]
    if gate:
        assert links[0] == [src_kf for src_kf in (vislam.KF_FIRST, 0, 1, 2, 3, 4, 5, vislam.KF_NOT_SAVED)] and links[1][0] == vislam.KF_CARRIED
    else:
        assert links[0][0] == vislam.KF_FIRST and links[1][0] == vislam.KF_CARRIED and links[0][1:] == list(range(PB - 1))
    assert n_pairs == (13 if gate else 14) and n_tracked >= 20 * n_pairs
    print(f"gate {gate}: {n_pairs} pairs, {n_tracked} tracked points")


def test_compacted_rows_feed_the_homography(vislam, canvas):
    """integration: the compacted rows of one launch, given to vis_homography_batch as they lie, yield the record tests/homography_ref.py
    gives on the same rows"""
    import torch
    frames = np.stack([vislam.synth_frame(canvas, t, PW, PH) for t in range(2 * PB)])
    L = _plan_launches(vislam, torch, frames, False, kr.default_params())[0]
    cap = L["cap"]
    p = src.plan_params(vislam, PW, PH, False)
    c = vislam.Context(0, p)
    draws = hr.make_draws(7)
    d_p1, d_p2, d_nt, d_draws = _dev(torch, L["p1"]), _dev(torch, L["p2"]), _dev(torch, L["nt"]), _dev(torch, draws)
    out = _filled(torch, PB * 112)
    hp = vislam.default_homography_params()
    c.homography_batch(PB, d_p1.data_ptr(), d_p2.data_ptr(), d_nt.data_ptr(), cap, d_draws.data_ptr(), 0, 0, 0, out.data_ptr(), hp)
    c.batch_sync()
    recs = out.cpu().numpy().view(vislam.HOMOGRAPHY_RESULT_DTYPE)
    cam = hr.Camera(p.fx, p.cx, p.cy)
    for i in (1, PB - 1):
        k = int(L["nt"][i])
        assert k >= 20
        x1, x2 = L["p1"][i, :k * 8].view(np.float32).reshape(k, 2), L["p2"][i, :k * 8].view(np.float32).reshape(k, 2)
        w_rec, _ = hr.homography(cam, hr.default_params(), x1, x2, draws, None)
        g, w = recs[i].copy(), w_rec.copy()
        for name in ("score_h", "score_e"):
            assert abs(float(g[name]) - float(w[name])) <= (k - 1) * 2.0 ** -52 * abs(float(w[name])), (i, name)
            g[name] = w[name] = 0.0
        assert g.tobytes() == w.tobytes(), (i, recs[i], w_rec)
        assert int(recs[i]["n_inliers"]) >= 0.8 * k                # one plane shifted: the tracks agree on a homography
    c.close()


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_tracks(vislam, canvas, tmp_path):
    """tools/run_directory.py --klt: the CSV holds what vis_batch_klt gives for the same frames in the same batches"""
    import json
    import os
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, B = 7, 4
    frames = np.stack([vislam.synth_frame(canvas, t, PW, PH) for t in range(n)])
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (PW, PH) + frames[t].tobytes())
    csv = tmp_path / "klt.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(B),
                        "--klt", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    # the same launches in this process (the tool's parameters: ORB::create(200), fy = fx; a forward-backward bound of 1 px)
    p = src.plan_params(vislam, PW, PH, False)
    p.nfeatures = 200
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, B)
    cap = c.keypoint_capacity(PW, PH)
    kp = vislam.default_klt_params()
    kp.fb_max_px = 1.0
    dev = _dev(torch, frames)
    want, totals = [], dict(pairs=0, points=0, tracked=0, oob=0, flat=0, fb=0)
    for first in range(0, n, B):
        nb = min(B, n - first)
        recs, pair = _filled(torch, B * cap * REC), _filled(torch, B * 32)
        c.batch_run(dev.data_ptr() + first * PW * PH, nb, vislam.STAGE_FRAME | vislam.STAGE_GRADIENT)
        c.batch_klt(dev.data_ptr() + first * PW * PH, nb, cap, recs.data_ptr(), pair.data_ptr(), kp=kp)
        c.batch_sync()
        rr, pp = recs.cpu().numpy().view(vislam.KLT_POINT_DTYPE).reshape(B, cap), pair.cpu().numpy().view(vislam.KLT_PAIR_DTYPE)
        links = c.batch_get_keyframes()
        for i in range(nb):
            if int(pp[i]["flags"]) & vislam.KLT_NO_PAIR:
                continue
            k1 = c.batch_keypoints(int(links[i]))[0]
            m = int(pp[i]["n_points"])
            assert m == len(k1)
            totals["pairs"] += 1
            for key, name in (("points", "n_points"), ("tracked", "n_tracked"), ("oob", "n_oob"), ("flat", "n_flat"), ("fb", "n_fb")):
                totals[key] += int(pp[i][name])
            want += [(first + i, jj, k1[jj], rr[i, jj].copy()) for jj in range(m)]
    c.close()
    assert totals["pairs"] == n - 2 and len(rows) == len(want) == totals["points"] > 500      # frame 0 and the second batch's first have no pair
    for row, (frame, jj, k1, rec) in zip(rows, want):
        assert int(row[0]) == frame and int(row[1]) == 1403636579763555584 + 50000000 * frame and int(row[2]) == jj
        assert np.array([float(v) for v in row[3:7] + row[8:10]], np.float32).tobytes() == \
            np.array([k1["x"], k1["y"], rec["x"], rec["y"], rec["fb"], rec["min_eig"]], np.float32).tobytes()
        assert [int(row[7])] + [int(v) for v in row[10:13]] == [int(rec[k]) for k in ("flags", "sad", "iters", "levels")]
    assert j["klt"] == totals and j["klt_csv"] == str(csv) and totals["tracked"] >= 0.8 * totals["points"]
