"""GPU: the photometric alignment and the patch builders on hostile matched points, candidate rows, counts and poses
(tests/align_hostile_cases.py; tests/test_align_hostile_ref.py shows the cases sound on the CPU).  These are the entry points that read
caller rows from device memory, where the host cannot validate them.

The candidate window has one rule for every float (include/vislam_hip.h at vis_patch_points): a keypoint whose level coordinate is NaN or
infinite, or whose window cannot touch the level, contributes no candidate.  So
  - vis_patch_points equals the oracle and the rule's exact restatement for every hostile value, layout and level;
  - a pair of vis_align_batch that holds hostile keypoints gives the bytes of the same pair with those keypoints deleted (the device's
    own launch of the shorter row, which in turn equals the oracle), clean pairs of the same launch give the bytes of a launch without
    hostile pairs, and nothing past min(d_npts, max_pts, 200) is read;
  - hostile d_npts, initial poses and explicit candidate rows (vis_estimate_pose_features) give the oracle's record: integers equal,
    floats byte-equal or NaN on both sides.
(w + 40 is far outside the frame but not outside the rule: on level 3 its window reaches the last column, align_hostile_cases.contributes.
Rows with it are compared with the oracle on the row as it is.)
Identity weights against oracle/align.cpp, VIS_W_TUKEY against its numpy restatement tests/align_weighted_ref.py.  Every output buffer
holds 0xEE before a call, and what a call must not write still does afterwards.  160 x 120 frames at strides 160 and 176."""
import ctypes as C

import numpy as np
import pytest

import align_hostile_cases as ahc
import hostile_cases as hc
import stride_range_cases as src

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
W, H, N, MAX_PTS = ahc.W, ahc.H, ahc.N_FRAMES, ahc.MAX_PTS
MODES = (0, 1)                        # VIS_W_IDENTITY, VIS_W_TUKEY
REC = ahc.ALIGN_DTYPE.itemsize


def _same(a, b, where):
    assert hc.same_record(a, b), (where, hc.differing_fields(a, b), [(k, a[k], b[k]) for k in hc.differing_fields(a, b)][:2])


def _no_nan(rec, where):
    for k in ("pose", "matrix", "error", "initial_error"):
        assert np.isfinite(rec[k]).all(), (where, k, rec[k])


class Rig:
    """the frames at one stride on the device with their vis_gradient_batch outputs, and vis_align_batch launches over them"""
    def __init__(self, vislam, stride):
        import torch
        assert C.sizeof(vislam.AlignResult) == REC
        self.vislam, self.stride, self.torch = vislam, stride, torch
        self.ctx = vislam.Context(0)
        self.dev = torch.from_numpy(src.padded(ahc.frames(vislam), stride)).cuda()
        fe = vislam.gradient_frame_elems(W, H)
        self.gray = torch.zeros(N * fe, dtype=torch.uint8, device="cuda")
        self.gx = torch.zeros(N * fe, dtype=torch.int16, device="cuda"); self.gy = torch.zeros_like(self.gx)
        self.g = torch.zeros(N * fe, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ctx.gradient_batch(self.dev.data_ptr(), W, H, stride, N, self.gray.data_ptr(), self.gx.data_ptr(), self.gy.data_ptr(), self.g.data_ptr())
        torch.cuda.synchronize()
        self.ap = ahc.params(vislam)
        self.cache = {}

    def set_mode(self, mode):
        aw = self.vislam.default_align_weights()
        aw.mode = mode
        self.ctx.set_align_weights(aw)

    def launch(self, mode, pts, npts, inits=None, max_pts=MAX_PTS, ap=None, raw=False):
        """one vis_align_batch over the N frames -> N records (record 0 is the cleared one); the record past the last one, the points,
        the counts and the poses must hold afterwards what they held before"""
        torch = self.torch
        pts = np.ascontiguousarray(pts, np.float32); npts = np.ascontiguousarray(npts, np.int32)
        assert pts.shape == (N, max_pts, 2) and npts.shape == (N,)
        d_pts, d_n = torch.from_numpy(pts).cuda(), torch.from_numpy(npts).cuda()
        d_init = None if inits is None else torch.from_numpy(np.ascontiguousarray(inits, np.float32)).cuda()
        out = torch.full(((N + 1) * REC,), ahc.FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.set_mode(mode)
        self.ctx.align_batch(ap or self.ap, self.dev.data_ptr(), W, H, self.stride, N, self.gray.data_ptr(), self.gx.data_ptr(), self.gy.data_ptr(),
                             d_pts.data_ptr(), d_n.data_ptr(), max_pts, d_init.data_ptr() if d_init is not None else 0, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[N * REC:] == ahc.FILL).all(), "vis_align_batch wrote past record n - 1"
        assert d_pts.cpu().numpy().tobytes() == pts.tobytes() and d_n.cpu().numpy().tobytes() == npts.tobytes()
        assert d_init is None or d_init.cpu().numpy().tobytes() == np.ascontiguousarray(inits, np.float32).tobytes()
        assert not got[:REC].any(), "record 0 is cleared"
        return got[:N * REC].tobytes() if raw else np.frombuffer(got[:N * REC].tobytes(), ahc.ALIGN_DTYPE)

    def clean(self, mode, count=MAX_PTS):
        """the launch of the clean rows with `count` points each (cached)"""
        key = ("clean", mode, count)
        if key not in self.cache:
            self.cache[key] = self.launch(mode, ahc.points(), np.full(N, count, np.int32))
        return self.cache[key]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=ahc.STRIDES, ids=lambda s: f"stride{s}")
def rig(vislam, request):
    r = Rig(vislam, request.param)
    yield r
    r.close()


def _chunks(items, k):
    return [items[i:i + k] for i in range(0, len(items), k)]


# ---- vis_patch_points -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pctx(vislam):
    p = vislam.default_params()
    p.w_size, p.h_size = W, H
    c = vislam.Context(0, p)
    yield c
    c.close()


def _patch_points_raw(vislam, c, good, cap):
    patch = [np.full((max(cap, 1), 4), np.nan, np.float32) for _ in range(5)]
    debug = [np.full((max(cap, 1), 4), np.nan, np.float32) for _ in range(5)]
    for a in patch + debug:
        a.view(np.uint8)[:] = ahc.FILL
    ap = (C.c_void_p * 5)(*[a.ctypes.data for a in patch]); ad = (C.c_void_p * 5)(*[a.ctypes.data for a in debug])
    npt = (C.c_int * 5)(); ndb = (C.c_int * 5)()
    rc = vislam.lib.vis_patch_points(c._h, good.ctypes.data_as(C.c_void_p), len(good), cap, ap, npt, ad, ndb)
    return rc, list(npt), list(ndb), patch, debug


def _kp(vislam, xy):
    kp = np.zeros(len(xy), vislam.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    return kp


@pytest.mark.parametrize("lay", ahc.INSIDE_LAYOUTS + ("past_used",))
def test_patch_points_on_hostile_keypoints(vislam, orc, pctx, lay):
    """230 keypoints, 200 read: counts and rows equal the oracle and the exact rule on all five levels; rows past the count keep 0xEE"""
    base, idx = ahc.points()[1], ahc.layout(lay)
    cap = ahc.USED * 121
    for kind in ahc.kinds():
        xy = ahc.apply_kind(kind, base, idx)
        rc, npt, ndb, patch, _ = _patch_points_raw(vislam, pctx, _kp(vislam, xy), cap)
        assert rc == 0, (kind, rc)
        for l in range(5):
            want = orc.patch_points(_kp(vislam, xy), W, H, l)
            rule = ahc.patch_rule(xy, W, H, l)
            assert want.tobytes() == rule.tobytes(), (kind, l)
            assert npt[l] == len(want) and patch[l][:npt[l]].tobytes() == want.tobytes(), (kind, l, npt[l], len(want))
            assert (patch[l][npt[l]:].view(np.uint8) == ahc.FILL).all(), (kind, l)
            assert ndb[l] == ahc.USED
        if lay == "all" and not kind.endswith("w+40") and not kind.endswith("m40"):
            assert npt == [0] * 5, (kind, npt)


def test_patch_points_capacity_among_hostile_keypoints(vislam, orc, pctx):
    """VIS_E_CAPACITY and the required counts are reported as before when hostile keypoints sit among clean ones"""
    for kind in ("x:pinf", "y:2^31", "xy:nan", "x:p3e9"):
        xy = ahc.apply_kind(kind, ahc.points()[2], ahc.layout("stride5"))
        want = [orc.patch_points(_kp(vislam, xy), W, H, l) for l in range(5)]
        need = max(len(a) for a in want)
        assert need > ahc.USED
        rc, npt, _, patch, _ = _patch_points_raw(vislam, pctx, _kp(vislam, xy), need)
        assert rc == 0 and npt == [len(a) for a in want], (kind, rc)
        rc, npt, _, patch, _ = _patch_points_raw(vislam, pctx, _kp(vislam, xy), need - 1)
        assert rc == E_CAPACITY and npt == [len(a) for a in want], (kind, rc, npt)
        for l in range(5):
            k = min(len(want[l]), need - 1)
            assert patch[l][:k].tobytes() == want[l][:k].tobytes() and (patch[l][k:].view(np.uint8) == ahc.FILL).all(), (kind, l)


# ---- vis_align_batch: hostile keypoints ---------------------------------------------------------------------------------------------------
def _expected_row(vislam, orc, mode, t, row, count):
    return ahc.oracle_pair(vislam, orc, t, row, count, mode=mode)


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
@pytest.mark.parametrize("lay", ahc.INSIDE_LAYOUTS)
def test_isolation_inside_a_pair(vislam, orc, rig, lay, mode):
    """every hostile kind at the layout's indices of every pair: the record is the one of the row with those keypoints deleted"""
    base, idx = ahc.points(), ahc.layout(lay)
    rows = [ahc.deleted(base[t], idx) for t in range(N)]
    short = rig.launch(mode, np.stack([r for r, _ in rows]), np.array([0] + [c for _, c in rows[1:]], np.int32))
    for t in range(1, N):
        _no_nan(short[t], (lay, t))
        _same(short[t], _expected_row(vislam, orc, mode, t, rows[t][0], rows[t][1]), ("deleted", lay, t))
        if lay == "all":
            assert not short[t]["n_residuals"].any() and not short[t]["iterations"].any()
        else:
            assert (short[t]["n_residuals"][:4] > 0).all(), (lay, t, short[t]["n_residuals"])
    for chunk in _chunks(ahc.kinds(), N - 1):
        pts = base.copy()
        for t, kind in enumerate(chunk, 1):
            pts[t] = ahc.apply_kind(kind, base[t], idx)
        got = rig.launch(mode, pts, np.full(N, MAX_PTS, np.int32))
        for t, kind in enumerate(chunk, 1):
            if ahc.contributes(kind):
                _same(got[t], _expected_row(vislam, orc, mode, t, pts[t], MAX_PTS), (kind, lay, t))
            else:
                assert got[t].tobytes() == short[t].tobytes(), (kind, lay, t, hc.differing_fields(got[t], short[t]))
        for t in range(len(chunk) + 1, N):                                     # the pairs of a short last chunk are clean ones
            assert got[t].tobytes() == rig.clean(mode)[t].tobytes(), (chunk, t)


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
def test_isolation_between_pairs(vislam, orc, rig, mode):
    """clean pairs (1, 3, 5, 7) interleaved with hostile pairs (2, 4, 6: every keypoint, or every fifth) in one launch: the clean ones are
    byte-identical to the launch of clean pairs alone, which equals the oracle"""
    base, clean = ahc.points(), rig.clean(mode)
    for t in range(1, N):
        _same(clean[t], _expected_row(vislam, orc, mode, t, base[t], MAX_PTS), ("clean", t))
        assert (clean[t]["n_residuals"][:4] > 0).all()
    nothing = rig.launch(mode, base, np.zeros(N, np.int32))
    for ci, chunk in enumerate(_chunks(ahc.kinds(), 3)):
        lay = "all" if ci % 2 == 0 else "stride5"
        pts = base.copy()
        for t, kind in zip((2, 4, 6), chunk):
            pts[t] = ahc.apply_kind(kind, base[t], ahc.layout(lay))
        got = rig.launch(mode, pts, np.full(N, MAX_PTS, np.int32))
        hostile_t = (2, 4, 6)[:len(chunk)]
        for t in range(1, N):
            if t not in hostile_t:
                assert got[t].tobytes() == clean[t].tobytes(), (chunk, lay, t, hc.differing_fields(got[t], clean[t]))
        for t, kind in zip(hostile_t, chunk):
            if lay == "all" and not ahc.contributes(kind):
                assert got[t].tobytes() == nothing[t].tobytes(), (kind, t)


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
def test_hostile_values_past_the_count_change_nothing(vislam, rig, mode):
    """entries 200 and 201 of a row of 230 (past the 200 that are read), and entries 150 ... 229 of a row whose d_npts is 150"""
    base = ahc.points()
    for lay, count in (("past_used", MAX_PTS), ("past_count", ahc.PAST_COUNT)):
        want = rig.clean(mode, count)
        for chunk in _chunks(ahc.kinds(), N - 1):
            pts = base.copy()
            for t, kind in enumerate(chunk, 1):
                pts[t] = ahc.apply_kind(kind, base[t], ahc.layout(lay))
            assert rig.launch(mode, pts, np.full(N, count, np.int32), raw=True) == want.tobytes(), (lay, chunk)


NPTS_VALUES = (ahc.INT_MIN, -1, 0, 1, 200, 201, MAX_PTS, MAX_PTS + 1, ahc.INT_MAX)


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
def test_hostile_npts(vislam, orc, rig, mode):
    """d_npts below 1: the record of a pair without residuals; above max_pts: clamped to max_pts (and 200 are read)"""
    base = ahc.points()
    for chunk in _chunks(NPTS_VALUES, N - 1):
        npts = np.zeros(N, np.int64)
        npts[1:1 + len(chunk)] = chunk
        got = rig.launch(mode, base, npts.astype(np.int32))
        for t, v in enumerate(chunk, 1):
            _same(got[t], _expected_row(vislam, orc, mode, t, base[t], max(0, min(v, MAX_PTS))), ("npts", v, t))
            assert bool(got[t]["n_residuals"].any()) == (v >= 1), (v, got[t]["n_residuals"])
            if v < 1:
                assert got[t]["pose"].tolist() == [0, 0, 0, 1, 0, 0, 0] and not got[t]["error"].any() and not got[t]["iterations"].any()


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
def test_hostile_initial_poses(vislam, orc, rig, mode):
    """hostile d_init on pairs 1, 3, 5, 7 and a clean one on 2, 4, 6: every hostile record equals the oracle's (floats byte-equal or NaN on
    both sides, n_residuals equal), the neighbours are the bytes of the launch with clean poses only"""
    base, count = ahc.points(), ahc.INIT_COUNT
    unmet = set(ahc.EXCEPT_POSES) | set(ahc.EXCEPT_FINITE_POSES)
    npts = np.full(N, count, np.int32)
    clean_init = orc.se3_exp(ahc.CLEAN_INIT6)
    clean_inits = np.tile(clean_init.as_array(), (N, 1))
    want_clean = rig.launch(mode, base, npts, clean_inits)
    for t in range(1, N):
        _same(want_clean[t], ahc.oracle_pair(vislam, orc, t, base[t], count, init=clean_init, mode=mode), ("clean init", t))
        assert (want_clean[t]["n_residuals"][:4] > 0).all()
    for chunk in _chunks(ahc.hostile_inits(vislam, orc), 4):
        inits = clean_inits.copy()
        for t, (_, pose) in zip((1, 3, 5, 7), chunk):
            inits[t] = pose.as_array()
        got = rig.launch(mode, base, npts, inits)
        again = rig.launch(mode, base, npts, inits, raw=True)
        assert again == got.tobytes(), [n for n, _ in chunk]
        hostile_t = (1, 3, 5, 7)[:len(chunk)]
        for t, (name, pose) in zip(hostile_t, chunk):
            _same(got[t], ahc.oracle_pair(vislam, orc, t, base[t], count, init=pose, mode=mode), (name, t))
            assert ahc.meets_a_guard(got[t]) == (name not in unmet), (name, t, got[t]["n_residuals"], got[t]["iterations"])
        for t in range(1, N):
            if t not in hostile_t:
                assert got[t].tobytes() == want_clean[t].tobytes(), ([n for n, _ in chunk], t)


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
def test_a_second_launch_is_byte_identical(vislam, orc, rig, mode):
    base = ahc.points()
    pts, npts = base.copy(), np.full(N, MAX_PTS, np.int32)
    inits = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (N, 1))
    for t, kind, lay in ((1, "x:nan", "stride5"), (2, "xy:pinf", "wave_edges"), (3, "y:2^31", "first3"), (4, "x:p3e38", "all"), (6, "xy:2^35-", "last")):
        pts[t] = ahc.apply_kind(kind, base[t], ahc.layout(lay))
    inits[5] = dict(ahc.hostile_inits(vislam, orc))["q_nan_one"].as_array()
    inits[7] = dict(ahc.hostile_inits(vislam, orc))["tz_m2"].as_array()
    npts[6] = ahc.INT_MAX
    first = rig.launch(mode, pts, npts, inits, raw=True)
    assert rig.launch(mode, pts, npts, inits, raw=True) == first


# ---- vis_estimate_pose_features: explicit candidate rows ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lctx(vislam):
    c = vislam.Context(0)
    yield c
    c.close()


LIST_INITS = (None, "tz_m2", "q_nan_one")


@pytest.mark.parametrize("mode", MODES, ids=["identity", "tukey"])
@pytest.mark.parametrize("place", ahc.LIST_PLACES)
def test_hostile_candidate_rows(vislam, orc, lctx, place, mode):
    """1100 rows per level, levels 3 ... 0, one hostile component at every fifth row or at rows 255 / 256 / 1023 / 1024 (the ends of the
    rounds of 256 threads and of 4 x 256 candidates): the oracle's record; after one iteration the residual count of the validity test
    as tests/align_weighted_ref.py states it; a second call gives the same bytes"""
    import align_weighted_ref as ref
    aw = vislam.default_align_weights(); aw.mode = mode
    lctx.set_align_weights(aw)
    t = 1
    (l0, gx, gy), (l1, _, _) = ahc.levels(vislam, orc, t - 1), ahc.levels(vislam, orc, t)
    inits = dict(ahc.hostile_inits(vislam, orc))
    clean = ahc.record(lctx.estimate_pose_features(ahc.params(vislam), W, H, l0, l1, gx, gy, [ahc.list_rows(l) for l in range(5)]))
    assert (clean["n_residuals"][:4] > 0).all()
    try:
        for kind in ahc.list_values():
            cand = ahc.hostile_list(kind, place)
            for iname in LIST_INITS:
                init = None if iname is None else inits[iname]
                where = (kind, place, iname)
                got = ahc.record(lctx.estimate_pose_features(ahc.params(vislam), W, H, l0, l1, gx, gy, cand, init))
                want = ahc.oracle_pair(vislam, orc, t, np.zeros((1, 2), np.float32), 0, init=init, mode=mode, cand=cand)
                _same(got, want, where)
                again = ahc.record(lctx.estimate_pose_features(ahc.params(vislam), W, H, l0, l1, gx, gy, cand, init))
                assert again.tobytes() == got.tobytes(), where
                # four of five rows are clean, so residuals remain on every level -- unless the hostile rows are ACCEPTED and poison the step:
                # z = 1e-38 / 1e-45 passes every validity test (x2 = x1), 1 / z2 = 1e38 / inf overflows the Jacobian, the normal equations
                # and the step are NaN, and a NaN pose warps nothing on any later iteration or level (oracle and device agree on that)
                # (ahc.EXCEPT_ROWS; tests/test_align_hostile_ref.py shows on the oracle that these are the only ones)
                if iname is None:
                    assert ahc.meets_a_guard(got) == (kind not in ahc.EXCEPT_ROWS), (where, got["n_residuals"], got["iterations"])
                one = ahc.record(lctx.estimate_pose_features(ahc.params(vislam, 1), W, H, l0, l1, gx, gy, cand, init))
                pred = ref.estimate_pose_features(orc, ahc.params(orc, 1), W, H, l0, l1, gx, gy, cand, init)
                assert one["n_residuals"].tolist() == list(pred.n_residuals), (where, one["n_residuals"], list(pred.n_residuals))
                if iname is None:                                                      # (one iteration per level: the pose never moves)
                    assert (one["n_residuals"][:4] > 0).all() and (one["n_residuals"][:4] <= ahc.LIST_N).all(), (where, one["n_residuals"])
    finally:
        lctx.set_align_weights(None)


# ---- parameters and the carried pose ------------------------------------------------------------------------------------------------------
def test_non_finite_alignment_parameters_are_refused(vislam, orc, rig, lctx):
    """fx, fy = inf and non-finite cx, cy, epsilon, z_factor: VIS_E_INVALID with an error text, nothing written"""
    t = 1
    (l0, gx, gy), (l1, _, _) = ahc.levels(vislam, orc, t - 1), ahc.levels(vislam, orc, t)
    cand = [ahc.list_rows(l) for l in range(5)]
    cases = [("fx", np.inf), ("fy", np.inf), ("fx", np.nan), ("fy", -np.inf)]
    cases += [(f, v) for f in ("cx", "cy", "epsilon", "z_factor") for v in (np.nan, np.inf, -np.inf)]
    for field, value in cases:
        ap = ahc.params(vislam)
        setattr(ap, field, float(value))
        with pytest.raises(vislam.VisError) as e:
            lctx.estimate_pose_features(ap, W, H, l0, l1, gx, gy, cand)
        assert e.value.code == E_INVALID and "alignment" in str(e.value), (field, value, str(e.value))
        import torch
        out = torch.full((N * REC,), ahc.FILL, dtype=torch.uint8, device="cuda")
        d_pts = torch.from_numpy(ahc.points()).cuda(); d_n = torch.full((N,), MAX_PTS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(vislam.VisError) as e:
            rig.ctx.align_batch(ap, rig.dev.data_ptr(), W, H, rig.stride, N, rig.gray.data_ptr(), rig.gx.data_ptr(), rig.gy.data_ptr(),
                                d_pts.data_ptr(), d_n.data_ptr(), MAX_PTS, 0, out.data_ptr())
        torch.cuda.synchronize()
        assert e.value.code == E_INVALID and "alignment" in str(e.value), (field, value, str(e.value))
        assert (out.cpu().numpy() == ahc.FILL).all(), (field, value)
    ok = ahc.params(vislam)
    ok.epsilon, ok.z_factor, ok.cx, ok.cy = 0.0, -0.5, -1e6, 1e6                         # finite values of any sign stay accepted
    lctx.estimate_pose_features(ok, W, H, l0, l1, gx, gy, cand)


def test_a_non_finite_carried_pose_propagates_down_the_chain(vislam, orc, canvas):
    """vis_batch_track_init takes the pose as given: a NaN component stays in every final_poseCam that is composed from it, exactly as the
    oracle's SE3 product composes it; the alignment records are untouched by it.  Three frames of 320 x 240."""
    import torch
    from batch_track_cases import Oracle as _Oracle, decode as _decode, residual as _residual
    w, h, n = 320, src.PLAN_H, 3
    frames = src.plan_frames(vislam, canvas, w, False)[:n]
    c = vislam.Context(0, src.plan_params(vislam, w, h, False))
    c.batch_plan(w, h, w, n)
    nan = float("nan")
    init = vislam.Se3f(0.0, nan, 0.0, 1.0, 0.5, nan, -0.25)
    c.batch_track_init(init)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    a = torch.full((n * C.sizeof(vislam.AlignResult),), ahc.FILL, dtype=torch.uint8, device="cuda")
    tr_ = torch.full((n * C.sizeof(vislam.TrackResult),), ahc.FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.batch_run(dev.data_ptr(), n, vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT)
    c.batch_track(vislam.default_align_params(), dev.data_ptr(), n, 0, a.data_ptr(), tr_.data_ptr())
    c.batch_sync()
    assert c.batch_status() == 0
    al, tr, ra, rt = _decode(vislam, a, tr_, n)
    oracle = _Oracle(orc, frames, w, h)
    kps = [c.batch_keypoints(i)[0] for i in range(n)]
    final = init
    assert hc.same_value(tr[0].pose.as_array(), final.as_array()) and tr[0].composed == vislam.TRACK_NONE
    for i in range(1, n):
        good = c.batch_matches(i)[0]
        assert len(good) > 0
        want = oracle.align(i - 1, i, kps[i - 1][good["queryIdx"]])
        _same(ahc.record(al[i]), ahc.record(want), ("align", i))
        assert want.n_residuals[0] > 0 and np.isfinite(want.pose.as_array()).all()
        final = orc.se3_mul(final, _residual(orc, want.pose))
        assert tr[i].composed == i
        assert hc.same_value(tr[i].pose.as_array(), final.as_array()), (i, tr[i].pose.as_array(), final.as_array())
        assert np.isnan(tr[i].pose.as_array()).any()
    c.close()
