"""GPU: Camera::Update's half pyramid, Camera::computeGradient, the patch builders, the photometric alignment and the tracking chain at
padded row strides and at both ends of the accepted size range, on the inputs of tests/stride_range_cases.py (which
tests/test_stride_range_ref.py shows sound on the CPU).  Every comparison is bytes: the integer stages against the oracle, the
alignment against the oracle (identity weights) or its numpy restatement (Tukey weights), the chain against the oracle's SE3 products.

  family A  sides 16 ... 24 (1- and 2-pixel levels) through vis_camera_update, vis_compute_gradient and vis_gradient_batch
  family B  sides of 4095 / 4094 through the same, the alignment at the last column / row of every level, and the refusal of 4096
  family C  stride > width: gradients, vis_align_batch, and the plan path (vis_batch_run + vis_batch_track) with the gate off and on
  family D  64 x 48: candidate counts at the round boundaries, candidate values patch_points never emits, d_npts / max_pts rows
  family E  vis_patch_points at four sizes and the capacity it reports"""
import ctypes as C

import numpy as np
import pytest

import align_weighted_ref as ref
import align_weights_cases as awc
import stride_range_cases as src
from test_batch_track_gpu import _Oracle, _decode, _residual, _zero

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
FILL8, FILL16 = 0x5A, 0x5A5A     # what the output buffers hold before a call


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def _gradient_batch(vislam, c, frames, stride, scale=3, offset=0):
    """vis_gradient_batch on the frames at `stride`, frame 0 `offset` bytes into its allocation -> host copies of d_gray, d_gx, d_gy,
    d_g with one guard record behind the n records, and the frame size in elements.  The frame buffer must come back as it went in."""
    import torch
    n, h, w = frames.shape
    buf = src.padded(frames, stride, offset)
    d = torch.from_numpy(buf).cuda()
    fe = vislam.gradient_frame_elems(w, h)
    assert fe > 0 and fe % 64 == 0
    gray = torch.full(((n + 1) * fe,), FILL8, dtype=torch.uint8, device="cuda"); g = gray.clone()
    gx = torch.full(((n + 1) * fe,), FILL16, dtype=torch.int16, device="cuda"); gy = gx.clone()
    torch.cuda.synchronize()
    c.gradient_batch(d.data_ptr() + offset, w, h, stride, n, gray.data_ptr(), gx.data_ptr(), gy.data_ptr(), g.data_ptr(), scale=scale)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), buf)
    return gray.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), g.cpu().numpy(), fe


def _check_records(orc, frames, scale, out, what):
    """every level of every frame against the oracle on the dense frame; level 0's part of d_gray, the elements between a frame's last
    level and the next frame, and the guard record hold the fill pattern"""
    gray, gx, gy, g, fe = out
    n, h, w = frames.shape
    for f in range(n):
        pyr, grads = src.gradient_ref(orc, frames[f], scale)
        off = f * fe
        for l in range(5):
            cnt = pyr[l].size
            ox, oy, og = grads[l]
            assert gx[off:off + cnt].tobytes() == ox.tobytes(), what + (f, l, "gx")
            assert gy[off:off + cnt].tobytes() == oy.tobytes(), what + (f, l, "gy")
            assert g[off:off + cnt].tobytes() == og.tobytes(), what + (f, l, "g")
            if l:
                assert gray[off:off + cnt].tobytes() == pyr[l].tobytes(), what + (f, l, "gray")
            else:
                assert (gray[off:off + cnt] == FILL8).all(), what + (f, "level 0 of d_gray")
            off += cnt
        end = (f + 1) * fe
        assert (gray[off:end] == FILL8).all() and (g[off:end] == FILL8).all(), what + (f, "pad")
        assert (gx[off:end] == FILL16).all() and (gy[off:end] == FILL16).all(), what + (f, "pad")
    for a, fill in ((gray, FILL8), (g, FILL8), (gx, FILL16), (gy, FILL16)):
        assert (a[n * fe:] == fill).all(), what + ("guard record",)


def _check_single_frame_entries(vislam, orc, c, frame, scales, what):
    got = c.camera_update(frame)
    pyr = orc.half_pyramid(frame)
    assert got[0].tobytes() == frame.tobytes(), what
    for l in range(1, 5):
        assert got[l].shape == pyr[l].shape and got[l].tobytes() == pyr[l].tobytes(), what + ("camera_update", l)
    for scale in scales:
        gx, gy, g = c.compute_gradient(frame, scale)
        _, grads = src.gradient_ref(orc, frame, scale)
        for l in range(5):
            assert gx[l].shape == grads[l][0].shape, what + (scale, l)
            assert gx[l].tobytes() == grads[l][0].tobytes(), what + (scale, l, "gx")
            assert gy[l].tobytes() == grads[l][1].tobytes(), what + (scale, l, "gy")
            assert g[l].tobytes() == grads[l][2].tobytes(), what + (scale, l, "g")


def _records(vislam, t, n):
    raw = t.cpu().numpy().tobytes()
    sz = C.sizeof(vislam.AlignResult)
    return [vislam.AlignResult.from_buffer_copy(raw, i * sz) for i in range(n)], raw


def _weights(vislam, mode):
    aw = vislam.default_align_weights()
    aw.mode = mode
    return aw


@pytest.fixture(scope="module")
def wctx(vislam):
    """a context of this module's own: the tests change its alignment weights and its parameters"""
    c = vislam.Context(0)
    yield c
    c.close()


def _expected(orc, pair, mode, first=None, last=None, iters=None):
    """identity weights: the oracle; Tukey weights: its numpy restatement (equal to the oracle under identity weights on these inputs,
    tests/test_stride_range_ref.py)"""
    ap = pair.params(orc, first=first, last=last, iters=iters)
    if mode == 0:
        return orc.estimate_pose_features(ap, pair.w, pair.h, *pair.levels(), pair.init(orc))
    return ref.estimate_pose_features(orc, ap, pair.w, pair.h, *pair.levels(), pair.init(orc), weights=mode)


def _explicit(vislam, orc, c, pair, mode):
    c.set_align_weights(_weights(vislam, mode))
    try:
        return c.estimate_pose_features(pair.params(vislam), pair.w, pair.h, *pair.levels(), pair.init(orc))
    finally:
        c.set_align_weights(None)


def _align_batch(vislam, c, frames, stride, k, pts, npts, max_pts, inits=None, iters=None, mode=0):
    """vis_gradient_batch + vis_align_batch on the frames at `stride` -> (records, their bytes)"""
    import torch
    n, h, w = frames.shape
    d = torch.from_numpy(src.padded(frames, stride)).cuda()
    fe = vislam.gradient_frame_elems(w, h)
    gray = torch.zeros(n * fe, dtype=torch.uint8, device="cuda"); g = torch.zeros_like(gray)
    gx = torch.zeros(n * fe, dtype=torch.int16, device="cuda"); gy = torch.zeros_like(gx)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda(); d_n = torch.from_numpy(npts).cuda()
    d_init = None if inits is None else torch.from_numpy(inits).cuda()
    out = torch.zeros(n * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
    ap = vislam.default_align_params()
    ap.fx, ap.fy, ap.cx, ap.cy = k
    if iters is not None:
        ap.max_iterations = iters
    torch.cuda.synchronize()
    c.set_align_weights(_weights(vislam, mode))
    try:
        c.gradient_batch(d.data_ptr(), w, h, stride, n, gray.data_ptr(), gx.data_ptr(), gy.data_ptr(), g.data_ptr())
        c.align_batch(ap, d.data_ptr(), w, h, stride, n, gray.data_ptr(), gx.data_ptr(), gy.data_ptr(), d_pts.data_ptr(), d_n.data_ptr(), max_pts,
                      0 if d_init is None else d_init.data_ptr(), out.data_ptr())
    finally:
        c.set_align_weights(None)
    torch.cuda.synchronize()
    return _records(vislam, out, n)


# ---- family A: the small end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", src.SMALL_SIZES, ids=lambda v: str(v))
def test_small_sizes_single_frame_entries(vislam, orc, ctx, w, h):
    """vis_camera_update and vis_compute_gradient (scales 1, 3, 8) where level 4 is 1 or 2 pixels wide or high.  Before 1-pixel levels
    were accepted, sides 16 ... 21 failed here with VIS_E_INVALID from the gradient launcher."""
    for kind in ("noise", "checker"):
        _check_single_frame_entries(vislam, orc, ctx, src.frames_of(kind, w, h, 1)[0], src.SCALES, (w, h, kind))


@pytest.mark.parametrize("w,h", src.SMALL_SIZES, ids=lambda v: str(v))
def test_small_sizes_gradient_batch(vislam, orc, ctx, w, h):
    """vis_gradient_batch, 9 frames, at the smallest stride the entry point takes and at 16 more"""
    for kind in ("noise", "checker"):
        frames = src.frames_of(kind, w, h, src.SMALL_N)
        for stride in (src.min_stride(w), src.min_stride(w) + 16):
            _check_records(orc, frames, 3, _gradient_batch(vislam, ctx, frames, stride), (w, h, kind, stride))


# ---- family B: the large end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", src.LARGE_SIZES, ids=lambda v: str(v))
def test_large_sizes_half_pyramid_and_gradients(vislam, orc, ctx, w, h):
    for kind in ("noise", "checker"):
        frames = src.frames_of(kind, w, h, src.LARGE_N)
        _check_single_frame_entries(vislam, orc, ctx, frames[1], src.SCALES, (w, h, kind))
        for stride in (src.min_stride(w), src.min_stride(w) + 16):
            _check_records(orc, frames, 3, _gradient_batch(vislam, ctx, frames, stride), (w, h, kind, stride))


@pytest.mark.parametrize("w,h", src.LARGE_SIZES, ids=lambda v: str(v))
def test_large_sizes_explicit_alignment_at_the_last_column_and_row(vislam, orc, wctx, w, h):
    """candidates in column cols - 1 / row rows - 1 of every level, moved by 1.2 px into the level's extra column / row where it has one
    (4095 >> 4 = 255 against 256 columns)"""
    pair = src.large_explicit_pair(orc, w, h)
    want = _expected(orc, pair, 0)
    assert all(want.n_residuals[l] > 0 for l in range(5))
    awc.same(_explicit(vislam, orc, wctx, pair, 0), want)
    lw, lh = vislam.half_pyramid_dims(w, h)
    for lvl in range(5):                                              # the edge points alone, per level: every one is counted
        if (w >> lvl, h >> lvl) == (lw[lvl], lh[lvl]):
            continue
        only = [np.zeros((0, 4), np.float32)] * 5
        only[lvl] = src.large_edge_points(w, h, lvl)
        q = pair.with_cand("edge", only, first=lvl, last=lvl, iters=1)
        got = _explicit(vislam, orc, wctx, q, 0)
        awc.same(got, _expected(orc, q, 0))
        assert got.n_residuals[lvl] == len(only[lvl])


@pytest.mark.parametrize("mode", src.WEIGHT_MODES)
def test_large_generated_alignment(vislam, orc, wctx, mode):
    """vis_align_batch on 4095 x 33 with keypoints up to x = 4094: the packed (y << 16) | x candidate words at their largest x"""
    g = src.large_generated(orc, vislam)
    res, _ = _align_batch(vislam, wctx, g["frames"], g["stride"], g["pair"].k, g["pts"], g["npts"], g["max_pts"], mode=mode)
    assert _zero(res[0])
    want = _expected(orc, g["pair"], mode)
    assert want.n_residuals[0] > 0
    awc.same(res[1], want)


def test_a_side_of_4096_is_refused_with_a_text(vislam, orc, wctx):
    import torch
    pair = src.large_explicit_pair(orc, 4095, 16)
    for w, h in ((4096, 16), (16, 4096)):
        with pytest.raises(vislam.VisError) as e:
            wctx.estimate_pose_features(pair.params(vislam), w, h, *pair.levels())
        assert e.value.code == E_INVALID and "4095" in str(e.value)
        # (a refusal reads and writes nothing; the buffer is large enough for every argument of a 4096 x 16 call all the same)
        room = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
        p = room.data_ptr()
        with pytest.raises(vislam.VisError) as e:
            wctx.align_batch(pair.params(vislam), p, w, h, 4096, 2, p, p, p, p, p, 1, 0, p)
        assert e.value.code == E_INVALID and "4095" in str(e.value)
        with pytest.raises(vislam.VisError) as e:
            wctx.gradient_batch(p, w, h, 4096, 1, p, p, p, p)
        assert e.value.code == E_INVALID and "4095" in str(e.value)
        assert vislam.gradient_frame_elems(w, h) == 0
        img = np.zeros((h, w), np.uint8)
        with pytest.raises(vislam.VisError) as e:
            wctx.compute_gradient(img)
        assert e.value.code == E_INVALID and "4095" in str(e.value)
        with pytest.raises(vislam.VisError) as e:
            wctx.camera_update(img)
        assert e.value.code == E_INVALID and "4095" in str(e.value)
    # the other side of the limit is family B itself; the lower limit says what it is as well
    assert vislam.gradient_frame_elems(4095, 4095) > 0
    with pytest.raises(vislam.VisError) as e:
        wctx.compute_gradient(np.zeros((15, 64), np.uint8))
    assert e.value.code == E_INVALID and "16" in str(e.value)
    with pytest.raises(vislam.VisError) as e:
        wctx.camera_update(np.zeros((64, 15), np.uint8))
    assert e.value.code == E_INVALID and "16" in str(e.value)


# ---- family C: padded strides ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,stride,offset", src.GRAD_STRIDES, ids=lambda v: str(v))
def test_padded_gradients(vislam, orc, ctx, w, stride, offset):
    """k_half_all takes a 16-aligned frame, stride and base; everything else goes level by level through k_half4.  The pad bytes hold
    0xA5 and the frames differ, so a row or frame stride mixed up with the width reads something else."""
    for n in src.GRAD_N:
        frames = src.frames_of("noise", w, src.GRAD_H, n, seed=2 + n)
        _check_records(orc, frames, 3, _gradient_batch(vislam, ctx, frames, stride, offset=offset), (w, stride, offset, n))


def test_align_batch_at_padded_strides(vislam, orc, wctx):
    a = src.align_320(orc, vislam)
    raws = []
    for stride in src.ALIGN_STRIDES:
        res, raw = _align_batch(vislam, wctx, a["frames"], stride, a["k"], a["pts"], a["npts"], a["max_pts"], inits=a["inits"])
        assert _zero(res[0])
        for t in (1, 2):
            assert a["want"][t].n_residuals[0] > 0
            awc.same(res[t], a["want"][t])
        raws.append(raw)
    assert raws[0] == raws[1] == raws[2]


def _fetch(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    host = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0     # device to host
    return host


def _run_plan(vislam, frames, w, stride, gate):
    """three launches of 8 through vis_batch_run(DETECT | MATCH | GRADIENT) + vis_batch_track on frames at `stride` -> per launch:
    alignment and track records (and their bytes), the pairing, keypoints, good matches, and the plan's gradients of frames 0 and 7"""
    import torch
    H, B = src.PLAN_H, src.PLAN_B
    c = vislam.Context(0, src.plan_params(vislam, w, H, gate))
    c.batch_plan(w, H, stride, B)
    dev = torch.from_numpy(src.padded(frames, stride)).cuda()
    ap = vislam.default_align_params()
    fe = vislam.gradient_frame_elems(w, H)
    launches = []
    for li in range(src.PLAN_LAUNCHES):
        ptr = dev.data_ptr() + li * B * stride * H
        c.batch_run(ptr, B, vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT)
        a = torch.zeros(B * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
        t = torch.zeros(B * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_track(ap, ptr, B, 0, a.data_ptr(), t.data_ptr())
        c.batch_sync()
        assert c.batch_status() == 0
        al, tr, ra, rt = _decode(vislam, a, t, B)
        pg, px, py, pgg, pfe = c.batch_gradients()
        assert pfe == fe
        grads = {}
        for i in (0, B - 1):
            grads[i] = (_fetch(pg + i * fe, fe), _fetch(px + 2 * i * fe, 2 * fe).view(np.int16), _fetch(py + 2 * i * fe, 2 * fe).view(np.int16),
                        _fetch(pgg + i * fe, fe))
        launches.append(dict(al=al, tr=tr, ra=ra, rt=rt, links=c.batch_get_keyframes(), kps=[c.batch_keypoints(i)[0] for i in range(B)],
                             good=[c.batch_matches(i)[0] for i in range(B)], grads=grads))
    c.close()
    return launches


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
@pytest.mark.parametrize("w,stride", src.PLAN_SHAPES, ids=lambda v: str(v))
def test_plan_path_at_padded_strides(vislam, orc, canvas, w, stride, gate):
    """(320, 336): k_track_snapshot's dword path; (318, 320): its byte path.  Every d_align record against the oracle's alignment of its
    pair -- the pairs against the carried keyframe (level 0 of the snapshot is dense, the frames are not) included --, d_track against
    the oracle chain, the plan's gradients of frames 0 and 7 against the oracle, and, where the width can be a stride (320), everything
    against the same stream planned at stride == w.  Gate on: frame 7 is flat, so the keyframe carried into launch 2 is frame 6."""
    H, B = src.PLAN_H, src.PLAN_B
    frames = src.plan_frames(vislam, canvas, w, gate)
    launches = _run_plan(vislam, frames, w, stride, gate)
    oracle = _Oracle(orc, frames, w, H)
    kps = {li * B + i: k for li, L in enumerate(launches) for i, k in enumerate(L["kps"])}
    saved, last, final = [], None, vislam.Se3f(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    n_pairs = n_carried = n_refused = 0
    for li, L in enumerate(launches):
        start = li * B
        for i in (0, B - 1):
            pyr, grads = src.gradient_ref(orc, frames[start + i], 3)
            gray, gx, gy, g = L["grads"][i]
            off = 0
            for l in range(5):
                cnt = pyr[l].size
                assert gx[off:off + cnt].tobytes() == grads[l][0].tobytes() and gy[off:off + cnt].tobytes() == grads[l][1].tobytes(), (li, i, l)
                assert g[off:off + cnt].tobytes() == grads[l][2].tobytes(), (li, i, l)
                assert l == 0 or gray[off:off + cnt].tobytes() == pyr[l].tobytes(), (li, i, l)
                off += cnt
        for i in range(B):
            g_ = start + i
            al, tr, link = L["al"][i], L["tr"][i], L["links"][i]
            if not gate or len(kps[g_]) > 1:
                if saved:
                    j = saved[-1]
                    assert link == (j - start if j >= start else vislam.KF_CARRIED), (li, i, link)
                    good = L["good"][i]
                    assert len(good) > 0, (li, i)
                    want = oracle.align(j, g_, kps[j][good["queryIdx"]])
                    assert want.n_residuals[0] > 0, (li, i)
                    awc.same(al, want)
                    last = _residual(orc, want.pose)
                    final = orc.se3_mul(final, last)
                    assert tr.composed == i, (li, i)
                    n_pairs += 1
                    n_carried += j < start
                else:
                    assert link == vislam.KF_FIRST and _zero(al) and tr.composed == vislam.TRACK_NONE, (li, i)
                saved.append(g_)
            else:
                assert link == vislam.KF_NOT_SAVED and _zero(al), (li, i)
                assert last is not None
                final = orc.se3_mul(final, last)
                j = saved[-1]
                assert tr.composed == (j - start if j >= start else vislam.KF_CARRIED), (li, i)
                n_refused += 1
            assert tr.pose.as_array().tobytes() == final.as_array().tobytes(), (li, i)
    assert n_pairs == (22 if gate else 23) and n_carried == 2 and n_refused == (1 if gate else 0)
    if gate:
        assert launches[1]["links"][0] == vislam.KF_CARRIED and saved[6:8] == [6, 8]
    if w % 4 == 0:
        used = sum(a * b for a, b in zip(*vislam.half_pyramid_dims(w, H)))
        dense = _run_plan(vislam, frames, w, w, gate)
        for a, b in zip(launches, dense):
            assert a["ra"] == b["ra"] and a["rt"] == b["rt"]
            for i in a["grads"]:
                # (the levels only: the elements between a frame's last level and the next frame are never written)
                for x, y in zip(a["grads"][i][1:], b["grads"][i][1:]):
                    assert x[:used].tobytes() == y[:used].tobytes()


# ---- family D: candidate counts and values on 64 x 48 -------------------------------------------------------------------------------
@pytest.mark.parametrize("first,last", src.LIST_LEVELS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", src.LIST_COUNTS)
def test_candidate_counts(vislam, orc, wctx, canvas, n, first, last):
    """k_align deals candidates four per thread per round of 1024; with Tukey weights both passes of an iteration must see the same list"""
    pair = src.count_pair(vislam, orc, canvas, n, first, last)
    for mode in src.WEIGHT_MODES:
        want = _expected(orc, pair, mode)
        # identity weights: residuals on every level (shown on the CPU); a Tukey step on ONE candidate can fling it out of the frame
        assert all(want.n_residuals[l] > 0 for l in range(last, first + 1)) if mode == 0 or n > 1 else want.n_residuals[first] > 0
        try:
            awc.same(_explicit(vislam, orc, wctx, pair, mode), want)
        except AssertionError as e:
            raise AssertionError((n, first, last, mode) + e.args) from None


@pytest.mark.parametrize("mode", src.WEIGHT_MODES)
def test_special_candidate_values(vislam, orc, wctx, canvas, mode):
    """fractional coordinates ((int)(-0.5) = 0), coordinates at cols - 0.5 and cols, z of 0.5, 2, 0 and -1, w of 0.5 and 0"""
    pair = src.special_pair(vislam, orc, canvas)
    want = _expected(orc, pair, mode)
    assert sum(want.n_residuals) > 0
    awc.same(_explicit(vislam, orc, wctx, pair, mode), want)
    if mode == 0:                                                    # and member by member at the initial pose: accepted as labelled
        for lvl in range(pair.last, pair.first + 1):
            for i, row in enumerate(src.special_rows(src.SMALL_W >> lvl, src.SMALL_H >> lvl)):
                only = [np.zeros((0, 4), np.float32)] * 5
                only[lvl] = pair.cand[lvl][i:i + 1]
                got = _explicit(vislam, orc, wctx, pair.with_cand("one", only, first=lvl, last=lvl, iters=1), 0)
                assert got.n_residuals[lvl] == int(row[-1]), (lvl, i, row)


@pytest.mark.parametrize("mode", src.WEIGHT_MODES)
@pytest.mark.parametrize("max_pts", sorted({m for m, _ in src.GEN_ROWS}))
def test_generated_point_counts(vislam, orc, wctx, max_pts, mode):
    """vis_align_batch with d_npts of 0, 1, 199, 200, 201 and 230 (at most 200 are used), d_npts above max_pts (clamped) and max_pts = 1
    (the smallest dynamic LDS block)"""
    g = src.generated_small(vislam, orc)[max_pts]
    res, _ = _align_batch(vislam, wctx, g["frames"], src.GEN_W, g["k"], g["pts"], g["npts"], max_pts, iters=src.GEN_ITERS, mode=mode)
    assert _zero(res[0])
    for t in range(1, src.GEN_N):
        if t not in g["pairs"]:
            assert list(res[t].n_residuals) == [0] * 5, (max_pts, t)  # d_npts = 0: the record of a pair without candidates
            continue
        try:
            awc.same(res[t], _expected(orc, g["pairs"][t], mode, iters=src.GEN_ITERS))
        except AssertionError as e:
            raise AssertionError((max_pts, g["pairs"][t].npts, mode) + e.args) from None


# ---- family E: the patch builders ---------------------------------------------------------------------------------------------------
def _patch_points_raw(vislam, c, good, cap):
    patch = [np.zeros((max(cap, 1), 4), np.float32) for _ in range(5)]
    debug = [np.zeros((max(cap, 1), 4), np.float32) for _ in range(5)]
    ap = (C.c_void_p * 5)(*[a.ctypes.data for a in patch]); ad = (C.c_void_p * 5)(*[a.ctypes.data for a in debug])
    npt = (C.c_int * 5)(); ndb = (C.c_int * 5)()
    rc = vislam.lib.vis_patch_points(c._h, good.ctypes.data_as(C.c_void_p), len(good), cap, ap, npt, ad, ndb)
    return rc, list(npt), list(ndb), patch, debug


@pytest.mark.parametrize("w,h", src.PATCH_SIZES, ids=lambda v: str(v))
def test_patch_builders(vislam, orc, w, h):
    p = vislam.default_params()
    p.w_size, p.h_size = w, h
    c = vislam.Context(0, p)
    for n in src.PATCH_COUNTS:
        good = src.patch_keypoints(vislam, w, h, n)
        want_p = [orc.patch_points(good, w, h, l) for l in range(5)]
        want_d = [orc.debug_points(good, l) for l in range(5)]
        need = max(max(len(a) for a in want_p), max(len(a) for a in want_d))
        rc, npt, ndb, patch, debug = _patch_points_raw(vislam, c, good, need)      # a capacity of exactly what is needed
        assert rc == 0, (n, rc)
        for l in range(5):
            assert npt[l] == len(want_p[l]) and ndb[l] == len(want_d[l]) == min(n, 200), (n, l)
            assert patch[l][:npt[l]].tobytes() == want_p[l].tobytes(), (n, l)
            assert debug[l][:ndb[l]].tobytes() == want_d[l].tobytes(), (n, l)
        rc, npt, ndb, _, _ = _patch_points_raw(vislam, c, good, need - 1)          # one below: the counts say what is needed
        assert rc == E_CAPACITY, (n, rc)
        assert npt == [len(a) for a in want_p] and ndb == [len(a) for a in want_d], n
    c.close()
