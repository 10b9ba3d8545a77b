"""GPU: the detector and its pyramid over the whole range vis_set_params accepts -- scale factors up to 3.0 (the wide k_resize variant
with its third-dword picks), the hand-over between the variants at ratio 2, steps at and next to ratio 1, sixteen levels, levels
smaller than the border, FAST thresholds 1 .. 5 (either side of the SWAR pretest switch) and 253 / 254, the largest border.

Two kinds of assertion, both exact (integer / byte data throughout):
  * pyramid parity: every level >= 1 read back (vis_debug_pyramid_level) equals the oracle's resize of the GPU level below it (a
    mismatch names the step), equals the same level of the oracle's own chain from the frame, and equals the numpy yardstick
    (tests/resize_ref.py, held equal to the oracle on these very steps by tests/test_resize_ref.py on the CPU);
  * detection parity: keypoint bytes and descriptors against orc.orb_detect_compute, with the conditions that keep a case from passing
    on nothing (param_range_cases.check_not_vacuous) asserted on the oracle's result alone.
The configurations and what each is the first to reach: tests/param_range_cases.py."""
import numpy as np
import pytest

import param_range_cases as prc
import resize_ref

pytestmark = pytest.mark.gpu

CASE_IDS = [c.id for c in prc.CASES]


def _assert_level(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        raise AssertionError((what, f"{len(ys)} of {got.size} bytes differ, first at (y, x) = ({ys[0]}, {xs[0]}): got {got[ys[0], xs[0]]}, "
                                    f"want {want[ys[0], xs[0]]}; columns {sorted(set(xs.tolist()))[:12]}, rows {sorted(set(ys.tolist()))[:12]}"))


def _check_pyramid(orc, ctx, img, ws, hs, what, batch=False, frame=0, yardstick_levels=None):
    """levels >= 1 of the last detection against (1) the oracle's step from the GPU level below, (2) the oracle's chain from the frame,
    (3) the numpy yardstick's step from the GPU level below (on yardstick_levels; None = all).  Only the w_l bytes of a row exist here."""
    L = len(ws)
    below, chain = img, img
    nbytes = 0
    for l in range(1, L):
        dw, dh = int(ws[l]), int(hs[l])
        got = ctx.pyramid_level(l, frame=frame, batch=batch, w=img.shape[1], h=img.shape[0])
        _assert_level(got, orc.resize_linear(below, dw, dh), (what, "step", l - 1, "->", l, below.shape[::-1], (dw, dh)))
        chain = orc.resize_linear(chain, dw, dh)
        _assert_level(got, chain, (what, "oracle chain", l))
        if yardstick_levels is None or l in yardstick_levels:
            _assert_level(got, resize_ref.resize_linear(below, dw, dh), (what, "numpy yardstick", l))
        below = got
        nbytes += got.size
    print(what, f"pyramid: {L - 1} levels, {nbytes} bytes equal to the oracle's", flush=True)


def _detect_both(vislam, orc, ctx, p, img, cap=None):
    ctx.set_params(p)
    k, d = ctx.orb_detect_compute(img, slot=0, cap=cap)
    ok, od = orc.orb_detect_compute(p, img, cap=cap)
    return k, d, ok, od


def _assert_same(k, d, ok, od, what=""):
    assert len(k) == len(ok), (what, len(k), len(ok))
    assert k.tobytes() == ok.tobytes(), what
    assert (d == od).all(), what


@pytest.fixture(scope="module")
def range_runs(vislam, orc, canvas):
    """per configuration, computed once and left unchanged: parameters, frame, the oracle's keypoints / descriptors and level sizes"""
    runs = {}
    for c in prc.CASES:
        p = c.params(vislam)
        img = c.image(vislam, canvas)
        ok, od = orc.orb_detect_compute(p, img)
        runs[c.id] = (c, p, img, ok, od)
    return runs


@pytest.mark.parametrize("cid", CASE_IDS)
def test_pyramid_and_detection_over_the_range(vislam, orc, ctx, range_runs, cid):
    c, p, img, ok, od = range_runs[cid]
    assert 2 * int(orc.level_geometry(p, c.w, c.h)[3][0]) * 1.25 + 256 <= 8192          # the plan's LDS sort holds level 0's survivors
    ctx.set_params(p)
    ws, hs, _, _ = ctx.level_geometry(c.w, c.h)
    ows, ohs, _, _ = orc.level_geometry(p, c.w, c.h)
    assert ws.tolist() == ows.tolist() and hs.tolist() == ohs.tolist()
    if c.sizes is not None:
        assert [(int(a), int(b)) for a, b in zip(ws, hs)][1:] == c.sizes                # the sizes the configuration was chosen for
    # not vacuous, by the oracle alone
    per = prc.check_not_vacuous(c, ws, hs, ok)
    k, d = ctx.orb_detect_compute(img, slot=0)
    print(cid, "oracle per octave", per.tolist(), "device per octave", np.bincount(k["octave"], minlength=len(ws)).tolist(), flush=True)
    # the pyramid first: a wrong level explains a wrong keypoint, not the other way round
    _check_pyramid(orc, ctx, img, ws, hs, cid, yardstick_levels=prc.YARDSTICK_LEVELS_16 if c.levels == 16 else None)
    _assert_same(k, d, ok, od, (cid, per.tolist()))


def test_pyramid_read_back_refusals(vislam, ctx, canvas):
    """vis_debug_pyramid_level: VIS_E_STATE before the plan has detected (a parameter change makes a new plan), VIS_E_INVALID for level 0,
    a level or frame out of range and a stride below the level's width; the batch plan is asked for separately"""
    p = vislam.default_params()
    p.w_size, p.h_size, p.nfeatures, p.nlevels = 320, 240, 300, 4
    ctx.set_params(p)

    def code(**kw):
        with pytest.raises(vislam.VisError) as ei:
            ctx.pyramid_level(**kw)
        return ei.value.code
    assert code(level=1) == -5                                       # VIS_E_STATE: nothing detected with these parameters
    ctx.orb_detect_compute(vislam.synth_frame(canvas, 0, 320, 240), slot=0)
    assert ctx.pyramid_level(1).shape == (200, 267)
    assert ctx.pyramid_level(3).shape == (139, 185)
    assert code(level=0) == -1 and code(level=4) == -1 and code(level=-1) == -1
    assert code(level=1, frame=1) == -1 and code(level=1, frame=-1) == -1
    assert code(level=1, batch=True) == -5                           # no batch plan
    out = np.zeros((200, 267), np.uint8)
    assert vislam.lib.vis_debug_pyramid_level(ctx._h, 0, 0, 1, out.ctypes.data, 266) == -1        # stride < w_1
    # a caller stride is honoured: the padding is left alone
    wide = np.full((200, 300), 7, np.uint8)
    assert vislam.lib.vis_debug_pyramid_level(ctx._h, 0, 0, 1, wide.ctypes.data, 300) == 0
    assert np.array_equal(wide[:, :267], ctx.pyramid_level(1)) and (wide[:, 267:] == 7).all()


@pytest.mark.parametrize("scale,levels", [(1.2, 8), (3.0, 4)])
def test_batch_pyramid_parity(vislam, orc, canvas, scale, levels):
    """nine frames of 752 x 480 through the batch plan -- one frame past the XCD group of eight -- frames 0, 7 and 8 read back"""
    import torch
    p = vislam.default_params()
    p.scale_factor, p.nlevels, p.nfeatures = scale, levels, 1000
    n = 9
    frames = np.stack([prc.make_image(vislam, canvas, "synth", 752, 480, 20 + t) for t in range(n)])
    c = vislam.Context(0, p)
    try:
        ws, hs, _, _ = c.level_geometry(752, 480)
        dev = torch.from_numpy(frames).cuda()
        c.batch_plan(752, 480, 752, n)
        with pytest.raises(vislam.VisError) as ei:
            c.pyramid_level(1, batch=True)
        assert ei.value.code == -5                                   # planned, not run
        c.batch_run(dev.data_ptr(), n, vislam.STAGE_DETECT)
        c.batch_sync()
        assert c.batch_status() == 0
        for f in (0, 7, 8):
            _check_pyramid(orc, c, frames[f], ws, hs, ("batch", scale, levels, "frame", f), batch=True, frame=f)
        with pytest.raises(vislam.VisError) as ei:
            c.pyramid_level(1, frame=n, batch=True)
        assert ei.value.code == -1
        k, d = c.batch_keypoints(8)
        ok, od = orc.orb_detect_compute(p, frames[8])
        assert len(ok) >= 50
        _assert_same(k, d, ok, od, ("batch", scale, "frame 8"))
    finally:
        c.close()


# ---- FAST thresholds at both ends of the accepted range, 320 x 240, one level and four
@pytest.fixture(scope="module")
def low_threshold_frame(vislam, canvas):
    return prc.make_image(vislam, canvas, "synth", 320, 240, 5, amp=6)


@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("thr", [1, 2, 4, 5])
def test_low_fast_thresholds(vislam, orc, ctx, low_threshold_frame, thr, levels):
    """k_fast runs its SWAR pretest for K = (threshold + 1) >> 1 >= 3 only: thresholds 1 .. 4 send every valid position to cornerScore,
    5 is the first that takes the pretest.  On the synthetic frame plus +-6 of noise FAST finds 5368 corners on level 0 at threshold 1 (one position in ten
    of the emit region) against 2385 at 5: the heaviest load the LDS queue and the carried-passer list get."""
    img = low_threshold_frame
    p = vislam.default_params()
    p.w_size, p.h_size, p.nlevels, p.nfeatures, p.fast_threshold = 320, 240, levels, 500, thr
    k, d, ok, od = _detect_both(vislam, orc, ctx, p, img, cap=20000)
    per = np.bincount(ok["octave"], minlength=levels)
    print("threshold", thr, "levels", levels, "oracle per octave", per.tolist(), "device", len(k), flush=True)
    assert len(ok) >= 50 and (per >= 1).all(), per.tolist()          # every level of 320 x 240 at 1.2^3 has an emit region far above 16 x 16
    if levels == 1:
        assert len(orc.fast_detect(img, thr)[0]) >= (3000 if thr <= 4 else 2000)       # the load the case is about
    _assert_same(k, d, ok, od, (thr, levels, per.tolist()))
    if levels == 4:
        ws, hs, _, _ = ctx.level_geometry(320, 240)
        _check_pyramid(orc, ctx, img, ws, hs, ("threshold", thr))


# level-0 floors of the dots image: one level keeps every corner (350 = 280 saturated + 70 at 254; 280 at threshold 254, where a
# difference of 254 is no corner); with four levels level 0's quota (258 of 800) is below the 280 tied saturated dots, which
# retainBest keeps together.  The upper levels blur isolated pixels away.
DOT_FLOORS = {(1, 253): 350, (1, 254): 280, (4, 253): 280, (4, 254): 280}


@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("thr", [253, 254])
def test_high_fast_thresholds(vislam, orc, ctx, thr, levels):
    """K = 127, the largest accepted, where the byte subtractions of the pretest wrap most often: isolated 255 on 0 and 0 on 255 are
    corners at every accepted threshold, dots of 254 on 0 at 253 only"""
    img, n_sat, n_254 = prc.dots_image()
    assert (n_sat, n_254) == (280, 70)
    p = vislam.default_params()
    p.w_size, p.h_size, p.nlevels, p.nfeatures, p.fast_threshold = 320, 240, levels, 800, thr
    k, d, ok, od = _detect_both(vislam, orc, ctx, p, img, cap=20000)
    n0 = int((ok["octave"] == 0).sum())
    print("threshold", thr, "levels", levels, "oracle", len(ok), "on level 0", n0, "device", len(k), flush=True)
    assert n0 >= DOT_FLOORS[(levels, thr)], (n0, len(ok))
    if levels == 1:
        assert n0 == (n_sat + n_254 if thr == 253 else n_sat)        # the 254-dots are corners at 253 and not at 254
    _assert_same(k, d, ok, od, (thr, levels, n0))


# ---- through the batch: the second of two consecutive launches runs on the predicted thresholds
def _two_batches(vislam, orc, p, frames, what, oracle_frame=4):
    import torch
    n = frames.shape[1]
    h, w = frames.shape[2:]
    single = vislam.Context(0, p)
    c = vislam.Context(0, p)
    try:
        c.batch_plan(w, h, w, n)
        taus = []
        for b in range(2):
            dev = torch.from_numpy(np.ascontiguousarray(frames[b])).cuda()
            c.batch_run(dev.data_ptr(), n, vislam.STAGE_DETECT)
            c.batch_sync()
            assert c.batch_status() == 0, (what, b)
            tau, redone = c.batch_fast_thresholds()
            print(what, "launch", b, "thresholds for the next launch", tau.tolist(), "redone", redone,
                  "keypoints per frame", [len(c.batch_keypoints(t, cap=20000)[0]) for t in range(n)], flush=True)
            # the prediction never goes below the configured threshold (nor beyond what FAST accepts): at threshold 1 there is no room below
            assert (tau >= p.fast_threshold).all() and (tau <= 254).all(), (what, b, tau.tolist())
            taus.append(tau.copy())
            for t in range(n):
                k, d = c.batch_keypoints(t, cap=20000)
                sk, sd = single.orb_detect_compute(frames[b, t], slot=0, cap=20000)
                _assert_same(k, d, sk, sd, (what, "batch", b, "frame", t, "against the single-frame call"))
                if t == oracle_frame:
                    ok, od = orc.orb_detect_compute(p, frames[b, t], cap=20000)
                    assert len(ok) >= 50, (what, len(ok))
                    _assert_same(k, d, ok, od, (what, "batch", b, "frame", t, "against the oracle"))
        return taus
    finally:
        c.close()
        single.close()


def test_speculative_threshold_at_fast_threshold_1(vislam, orc, canvas):
    p = vislam.default_params()
    p.w_size, p.h_size, p.nlevels, p.nfeatures, p.fast_threshold = 320, 240, 4, 500, 1
    p.keypoint_capacity = 4000                                       # headroom for ties at the cuts, as the tie tests give it
    frames = np.stack([prc.make_image(vislam, canvas, "synth", 320, 240, 40 + t) for t in range(18)]).reshape(2, 9, 240, 320)
    taus = _two_batches(vislam, orc, p, frames, "threshold 1")
    assert (taus[0] > 1).any(), taus                                 # the second launch did run on a prediction above the threshold


def test_speculative_threshold_at_fast_threshold_254(vislam, orc):
    """every corner of the dots image scores 254: the cut IS the threshold and the prediction has no room above it either"""
    p = vislam.default_params()
    p.w_size, p.h_size, p.nlevels, p.nfeatures, p.fast_threshold = 320, 240, 4, 800, 254
    p.keypoint_capacity = 4000
    img = prc.dots_image()[0]
    # eighteen different frames: the lattice shifted by whole pixels (the dots stay isolated and inside the border)
    frames = np.stack([np.roll(img, (t % 5, t % 7), axis=(0, 1)) for t in range(18)]).reshape(2, 9, 240, 320)
    taus = _two_batches(vislam, orc, p, frames, "threshold 254")
    assert all((t == 254).all() for t in taus), taus


def test_speculative_threshold_at_scale_3(vislam, orc, canvas):
    p = vislam.default_params()
    p.scale_factor, p.nlevels, p.nfeatures = 3.0, 4, 1000
    frames = np.stack([prc.make_image(vislam, canvas, "synth", 752, 480, 60 + t) for t in range(18)]).reshape(2, 9, 480, 752)
    _two_batches(vislam, orc, p, frames, "scale 3.0")


# ---- refusals at the ends of the range
def test_range_ends_are_refused_and_the_ends_themselves_accepted(vislam, ctx, canvas):
    p = vislam.default_params()
    above3 = float(np.nextafter(np.float32(3.0), np.float32(np.inf)))
    for field, val in (("scale_factor", above3), ("fast_threshold", 0), ("fast_threshold", 255), ("edge_threshold", 21), ("edge_threshold", 256)):
        q = p.copy()
        setattr(q, field, val)
        with pytest.raises(vislam.VisError) as ei:
            ctx.set_params(q)
        assert ei.value.code == -1, (field, val)
    for field, val in (("scale_factor", 3.0), ("fast_threshold", 1), ("fast_threshold", 254), ("edge_threshold", 22), ("edge_threshold", 255)):
        q = p.copy()
        setattr(q, field, val)
        ctx.set_params(q)
        assert getattr(ctx.params, field) == val
    # a last level under 8 pixels: 752 x 480 at 3.0 with 5 levels ends in 9 x 6.  The parameters are valid on their own; the detector
    # refuses the frame and the context goes on working
    q = p.copy()
    q.scale_factor, q.nlevels = 3.0, 5
    ctx.set_params(q)
    img = vislam.synth_frame(canvas, 1, 752, 480)
    with pytest.raises(vislam.VisError) as ei:
        ctx.orb_detect_compute(img, slot=0)
    assert ei.value.code == -1
    with pytest.raises(vislam.VisError) as ei:
        ctx.level_geometry(752, 480)
    assert ei.value.code == -1
    q.nlevels = 4
    ctx.set_params(q)
    assert len(ctx.orb_detect_compute(img, slot=0)[0]) >= 50
