"""GPU: the Tukey / MAD weighting of the photometric alignment (vis_set_align_weights; VISystem::TukeyFunctionWeights,
src/VISystem.cpp:1797-1870) through every alignment entry point against the numpy restatement tests/align_weighted_ref.py, which
tests/test_align_weights_ref.py ties to the oracle.  The arithmetic is specified exactly (integer residuals, a fixed summation tree), so
every comparison is of bits: pose, matrix, error[], initial_error, iterations[], n_residuals[]."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_weighted_ref as ref
import align_weights_cases as awc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vi-slam_amd", "lib", "vislam_main_gpu")
E_INVALID = -1


def _weights(vislam, mode, b=awc.DEFAULTS[0], s=awc.DEFAULTS[1]):
    aw = vislam.default_align_weights()
    aw.mode, aw.tukey_b, aw.mad_scale = mode, b, s
    return aw


@pytest.fixture()
def wctx(vislam):
    """a context of its own: the weighting is context state, and the session's shared context stays on identity"""
    c = vislam.Context(0)
    yield c
    c.close()


def _run_single(vislam, orc, c, cs, mode, b, s):
    c.set_align_weights(_weights(vislam, mode, b, s))
    got = c.estimate_pose_features(cs.params(vislam), cs.w, cs.h, *cs.levels(), cs.init(orc))
    want = ref.estimate_pose_features(orc, cs.params(orc), cs.w, cs.h, *cs.levels(), cs.init(orc), weights=mode, b=b, mad_scale=s)
    try:
        awc.same(got, want)
    except AssertionError as e:
        raise AssertionError((cs.name, mode, b, s) + e.args) from None
    return want


@pytest.mark.parametrize("mode", [1, 2])
def test_single_pair_every_case(vislam, orc, wctx, canvas, mode):
    """320 x 240 clean and occluded, 150 x 110 (does not halve exactly), an initial pose with a level subset, candidate lists of 1, 255,
    256, 257, 1024 and 1025 points, a list with z != 1, and pairs whose residuals are -255 and +255"""
    cases = awc.single_cases(vislam, orc, canvas)
    results = {name: _run_single(vislam, orc, wctx, cs, mode, *awc.DEFAULTS) for name, cs in cases.items()}
    assert all(sum(r.n_residuals) > 0 for r in results.values())
    # the weighting is in force: the occluded pair's result differs from the identity one
    occ = cases["occluded_320"]
    ident = orc.estimate_pose_features(occ.params(orc), occ.w, occ.h, *occ.levels())
    assert results["occluded_320"].pose.as_array().tobytes() != ident.pose.as_array().tobytes()


@pytest.mark.parametrize("mode,b,s", awc.CUSTOM)
def test_non_default_constants(vislam, orc, wctx, canvas, mode, b, s):
    cases = awc.single_cases(vislam, orc, canvas)
    for name in ("clean_320", "occluded_320", "z_not_1"):
        got = _run_single(vislam, orc, wctx, cases[name], mode, b, s)
        dflt = ref.estimate_pose_features(orc, cases[name].params(orc), 320, 240, *cases[name].levels(), cases[name].init(orc), weights=mode)
        assert (list(got.error), got.pose.as_array().tobytes()) != (list(dflt.error), dflt.pose.as_array().tobytes()), name


def test_degenerate_inputs(vislam, orc, wctx, canvas):
    cases = awc.single_cases(vislam, orc, canvas)
    cs = cases["clean_320"]
    same_frames = awc.with_frame2(orc, cs.c, cs.c["f0"])                      # every residual 0: MAD = 0 -> 1, every weight 1
    lv = (same_frames["gray1"], same_frames["gray2"], same_frames["gx"], same_frames["gy"], same_frames["cand"])
    empty = (cs.c["gray1"], cs.c["gray2"], cs.c["gx"], cs.c["gy"], [np.zeros((0, 4), np.float32)] * 5)
    outside = orc.se3_exp([50.0, 0, 0, 0, 0, 0])                              # every point leaves the image: zero residuals
    ap = cs.params(vislam)
    rec = {}
    for mode in (0, 1, 2):
        wctx.set_align_weights(_weights(vislam, mode))
        rec[mode] = [bytes(wctx.estimate_pose_features(ap, 320, 240, *lv)), bytes(wctx.estimate_pose_features(ap, 320, 240, *empty)),
                     bytes(wctx.estimate_pose_features(ap, 320, 240, *cs.levels(), outside))]
    assert rec[1] == rec[0] and rec[2] == rec[0]
    awc.same(vislam.AlignResult.from_buffer_copy(rec[1][0]), orc.estimate_pose_features(cs.params(orc), 320, 240, *lv))
    r = vislam.AlignResult.from_buffer_copy(rec[1][0])
    assert r.n_residuals[0] > 0 and list(r.error) == [0.0] * 5
    assert list(vislam.AlignResult.from_buffer_copy(rec[1][1]).n_residuals) == [0] * 5
    assert list(vislam.AlignResult.from_buffer_copy(rec[1][2]).n_residuals) == [0] * 5


def _records(vislam, buf, n):
    raw = buf.cpu().numpy().tobytes()
    sz = C.sizeof(vislam.AlignResult)
    return [vislam.AlignResult.from_buffer_copy(raw, i * sz) for i in range(n)]


@pytest.mark.parametrize("mode", [1, 2])
def test_generated_path(vislam, orc, wctx, canvas, mode):
    """vis_align_batch: two pairs at the 24 200-candidate level (the list fills 97 KB of LDS beside the histograms and tables) and a pair
    of 3 points, against the restatement fed with the oracle's patch points"""
    import torch
    g = awc.generated_case(vislam, orc, canvas)
    W, H, n = g["W"], g["H"], g["n"]
    dev = torch.from_numpy(g["frames"]).cuda()
    fe = vislam.gradient_frame_elems(W, H)
    gray = torch.zeros(n * fe, dtype=torch.uint8, device="cuda")
    gx = torch.zeros(n * fe, dtype=torch.int16, device="cuda"); gy = torch.zeros_like(gx)
    gg = torch.zeros(n * fe, dtype=torch.uint8, device="cuda")
    d_pts = torch.from_numpy(g["pts"]).cuda(); d_n = torch.from_numpy(g["npts"]).cuda()
    out = torch.zeros(n * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    wctx.gradient_batch(dev.data_ptr(), W, H, W, n, gray.data_ptr(), gx.data_ptr(), gy.data_ptr(), gg.data_ptr())
    ap = vislam.default_align_params(); oap = orc.default_align_params()
    for q in (ap, oap):
        q.fx, q.fy, q.cx, q.cy = 200.0, 200.0, 160.0, 120.0
    wctx.set_align_weights(_weights(vislam, mode))
    wctx.align_batch(ap, dev.data_ptr(), W, H, W, n, gray.data_ptr(), gx.data_ptr(), gy.data_ptr(), d_pts.data_ptr(), d_n.data_ptr(), g["max_pts"],
                     0, out.data_ptr())
    torch.cuda.synchronize()
    res = _records(vislam, out, n)
    assert bytes(res[0]) == bytes(C.sizeof(vislam.AlignResult))
    for t, p in g["pairs"].items():
        want = ref.estimate_pose_features(orc, oap, W, H, p["gray1"], p["gray2"], p["gx"], p["gy"], p["cand"], weights=mode)
        try:
            awc.same(res[t], want)
        except AssertionError as e:
            raise AssertionError((t,) + e.args) from None
    assert res[1].n_residuals[0] > 20000 and len(g["pairs"][3]["cand"][0]) == 3 * 121 and 0 < res[3].n_residuals[0] <= 3 * 121


# ---- the plan path: vis_batch_align / vis_batch_track on launches of 8 frames of 752 x 480 ------------------------------------------
PW, PH, PB = 752, 480, 8


def _stages(vislam):
    return vislam.STAGE_DETECT | vislam.STAGE_MATCH | vislam.STAGE_GRADIENT


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    import torch
    frames = np.stack([vislam.synth_frame(canvas, t, PW, PH) for t in range(2 * PB)])
    frames[3] = 128                                        # a featureless frame: refused by the keyframe gate (frame 4 pairs with frame 2)
    frames[PB] = 128                                       # ... and the first of launch 2: frame 1's pair is the one to the carried keyframe
    frames[5, 100:300, 200:500] = 255                      # an occluder
    return frames, torch.from_numpy(frames).cuda()


class _Pairs:
    """the restatement (prev -> cur) on the matched keypoints of prev, levels cached by frame"""
    def __init__(self, orc, frames):
        self.orc, self.frames, self.lv = orc, frames, {}

    def levels(self, g):
        if g not in self.lv:
            pyr = self.orc.half_pyramid(self.frames[g])
            gx, gy = [], []
            for lv in pyr:
                a, b, _ = self.orc.scharr_gradient(lv, 3)
                gx.append(a); gy.append(b)
            self.lv[g] = (pyr, gx, gy)
        return self.lv[g]

    def align(self, j, g, prev_kp, mode):
        (p0, gx, gy), (p1, _, _) = self.levels(j), self.levels(g)
        cand = [self.orc.patch_points(prev_kp, PW, PH, l) for l in range(5)]
        ap = self.orc.default_align_params()
        if mode == 0:                                       # (identity: the oracle itself, and the restatement equal to it on this pair)
            want = self.orc.estimate_pose_features(ap, PW, PH, p0, p1, gx, gy, cand)
            awc.same(ref.estimate_pose_features(self.orc, ap, PW, PH, p0, p1, gx, gy, cand), want)
            return want
        return ref.estimate_pose_features(self.orc, ap, PW, PH, p0, p1, gx, gy, cand, weights=mode)


def _plan_context(vislam, K):
    p = vislam.default_params()
    p.fy = p.fx
    p.keyframe_min_points = K
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, PB)
    return c


@pytest.mark.parametrize("K", [0, 1])
def test_plan_path_equals_the_restatement(vislam, orc, stream, K):
    """two launches of 8 under VIS_W_TUKEY, keyframe gate off (K = 0) and on: every record of vis_batch_track equals the restatement on
    the same pair -- the pair against the keyframe carried from launch 1 included -- and vis_batch_align gives the same records
    for the pairs inside the launch.  With identity weights on the same pairs the restatement equals the oracle."""
    import torch
    frames, dev = stream
    ap = vislam.default_align_params()
    c = _plan_context(vislam, K)
    c.set_align_weights(_weights(vislam, 1))
    pairs = _Pairs(orc, frames)
    sz = C.sizeof(vislam.AlignResult)
    kps, saved, n_pairs, n_carried = {}, [], 0, 0
    for li in range(2):
        ptr = dev.data_ptr() + li * PB * PW * PH
        a = torch.zeros(PB * sz, dtype=torch.uint8, device="cuda"); b = torch.zeros_like(a)
        t = torch.zeros(PB * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_run(ptr, PB, _stages(vislam))
        c.batch_align(ap, ptr, PB, 0, 0, 0, 0, b.data_ptr())
        c.batch_track(ap, ptr, PB, 0, a.data_ptr(), t.data_ptr())
        c.batch_sync()
        assert c.batch_status() == 0
        al, bl = _records(vislam, a, PB), _records(vislam, b, PB)
        links = c.batch_get_keyframes() if K else None
        for i in range(PB):
            kps[li * PB + i] = c.batch_keypoints(i)[0]
        for i in range(PB):
            g = li * PB + i
            if K:
                is_saved = len(kps[g]) > (K if saved else 1)
                j = saved[-1] if (is_saved and saved) else None
                if is_saved:
                    saved.append(g)
            else:
                j = g - 1 if g > 0 else None
            if j is None:
                assert bytes(al[i]) == bytes(sz), (li, i)
                continue
            if K:
                assert links[i] == (j - li * PB if j >= li * PB else vislam.KF_CARRIED), (li, i, links[i])
            good = c.batch_matches(i)[0]
            prev_kp = kps[j][good["queryIdx"]]
            want = pairs.align(j, g, prev_kp, 1)
            try:
                awc.same(al[i], want)
            except AssertionError as e:
                raise AssertionError((K, li, i, j) + e.args) from None
            pairs.align(j, g, prev_kp, 0)
            if j >= li * PB:
                assert bytes(bl[i]) == bytes(al[i]), (li, i)
            else:
                assert bytes(bl[i]) == bytes(sz), (li, i)              # vis_batch_align skips the pair to the carried keyframe
                n_carried += 1
            n_pairs += 1
    c.close()
    assert n_carried == 1 and n_pairs >= 11, (n_pairs, n_carried)


CAL_XML = """<?xml version="1.0"?>
<opencv_storage>
<in_width type_id="integer"> 752 </in_width>
<in_height type_id="integer"> 480 </in_height>
<out_width type_id="integer"> 752 </out_width>
<out_height type_id="integer"> 480 </out_height>
<calibration_values type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 458.654 457.296 367.215 248.375 </data></calibration_values>
<rectification type_id="opencv-matrix">
  <rows>1</rows> <cols>4</cols> <dt>f</dt>
  <data> 0 0 0 0 </data></rectification>
<imu2cam0Transformation type_id="opencv-matrix">
  <rows>4</rows> <cols>4</cols> <dt>f</dt>
  <data> 0.0148655429818 -0.999880929698 0.00414029679422 -0.0216401454975
         0.999557249008 0.0149672133247 0.025715529948 -0.064676986768
        -0.0257744366974 0.00375618835797 0.999660727178 0.00981073058949
         0.0 0.0 0.0 1.0 </data></imu2cam0Transformation>
<camera_frecuency type_id="float"> 20 </camera_frecuency>
<imu_frecuency type_id="float"> 200 </imu_frecuency>
<min_features type_id="integer"> 20</min_features>
<num_max_keyframes type_id="integer"> 10</num_max_keyframes>
<start_index type_id="integer"> 0 </start_index>
<use_gt type_id="integer">1</use_gt>
<use_ros type_id="integer">0</use_ros>
<num_cells type_id="integer"> 49</num_cells>
<length_patch type_id="integer"> 3</length_patch>
<detector type_id="integer">2</detector>
<matcher type_id="integer">4</matcher>
</opencv_storage>
"""


def _f32(line):
    return np.array([int(x, 16) for x in line.split()[1:]], np.uint32).view(np.float32)


def test_batch_track_equals_the_adapters_with_alignment_weights(vislam, orc, canvas, tmp_path):
    """the frame-at-a-time adapters with VISystem::alignmentWeights = VIS_W_TUKEY (vislam_main_gpu ... tukey) and vis_batch_run +
    vis_batch_track under vis_set_align_weights(VIS_W_TUKEY) give the same final_poseCam for every one of 18 frames (launches of 16
    and 2: the last launch's first pair is the one to the carried keyframe) -- and not the identity trajectory"""
    import torch
    nframes = 18
    f = tmp_path / "cal.xml"
    f.write_text(CAL_XML)
    runs = {}
    for name in ("tukey", "identity"):
        out = subprocess.run([EXE, str(f), str(nframes), str(tmp_path / "out.csv"), "synthetic", name], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        lines = out.stdout.splitlines()
        runs[name] = (_f32([l for l in lines if l.startswith("INITPOSE")][0]), [_f32(l) for l in lines if l.startswith("FINALPOSE")])
    init, fposes = runs["tukey"]
    assert len(fposes) == nframes
    assert fposes[-1].tobytes() != runs["identity"][1][-1].tobytes()
    Kc = [458.654, 457.296, 367.215, 248.375]
    p = vislam.default_params()
    p.fx = p.fy = float(np.float32(Kc[0]))
    p.cx, p.cy = float(np.float32(Kc[2])), float(np.float32(Kc[3]))
    p.w_size, p.h_size = PW, PH
    p.keyframe_min_points = 1
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, 16)
    c.set_align_weights(_weights(vislam, 1))
    ap = vislam.default_align_params()
    ap.fx, ap.fy, ap.cx, ap.cy = [float(np.float32(x)) for x in Kc]
    c.batch_track_init(vislam.Se3f(*[float(x) for x in init]))
    seed = orc.se3_from_rt(np.eye(3, dtype=np.float32), np.array([-0.0, -0.0, -0.0], np.float32))     # the adapters' SE3(I, -TranslationResidual)
    seeds = torch.from_numpy(np.tile(seed.as_array(), (16, 1)).copy()).cuda()
    frames = torch.from_numpy(np.stack([vislam.synth_frame(canvas, i + 2, PW, PH) for i in range(nframes)])).cuda()
    got = []
    for s in range(0, nframes, 16):
        n = min(16, nframes - s)
        ptr = frames.data_ptr() + s * PW * PH
        a = torch.zeros(n * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
        t = torch.zeros(n * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_run(ptr, n, _stages(vislam))
        c.batch_track(ap, ptr, n, seeds.data_ptr(), a.data_ptr(), t.data_ptr())
        c.batch_sync()
        raw = t.cpu().numpy().tobytes()
        got += [vislam.TrackResult.from_buffer_copy(raw, i * C.sizeof(vislam.TrackResult)) for i in range(n)]
    assert c.batch_status() == 0
    c.close()
    for i in range(nframes):
        assert got[i].pose.as_array().tobytes() == fposes[i].tobytes(), (i, got[i].pose.as_array(), fposes[i])


def test_state(vislam, orc, canvas, stream):
    import torch
    cs = awc.single_cases(vislam, orc, canvas)["occluded_320"]
    c = vislam.Context(0)
    d = c.get_align_weights()
    assert (d.mode, d.reserved_) == (0, 0) and bytes(d) == bytes(vislam.default_align_weights())
    # get returns what set stored
    c.set_align_weights(_weights(vislam, 2, 3.25, 1.75))
    g = c.get_align_weights()
    assert (g.mode, g.tukey_b, g.mad_scale, g.reserved_) == (2, 3.25, 1.75, 0)
    # a refused set leaves the previous setting in force
    bad = [_weights(vislam, 3), _weights(vislam, -1), _weights(vislam, 1, 0.0), _weights(vislam, 1, -1.0), _weights(vislam, 1, float("nan")),
           _weights(vislam, 1, float("inf")), _weights(vislam, 1, 4.0, 0.0), _weights(vislam, 1, 4.0, float("nan")), _weights(vislam, 1, 4.0, float("-inf"))]
    r = _weights(vislam, 1); r.reserved_ = 1
    for aw in bad + [r]:
        assert vislam.lib.vis_set_align_weights(c._h, C.byref(aw)) == E_INVALID
        assert bytes(c.get_align_weights()) == bytes(g)
    got = c.estimate_pose_features(cs.params(vislam), cs.w, cs.h, *cs.levels())
    awc.same(got, ref.estimate_pose_features(orc, cs.params(orc), cs.w, cs.h, *cs.levels(), weights=2, b=3.25, mad_scale=1.75))
    # set Tukey, run; set identity (NULL = the defaults), run: the second run is the oracle's
    c.set_align_weights(_weights(vislam, 1))
    first = c.estimate_pose_features(cs.params(vislam), cs.w, cs.h, *cs.levels())
    c.set_align_weights(None)
    second = c.estimate_pose_features(cs.params(vislam), cs.w, cs.h, *cs.levels())
    want = orc.estimate_pose_features(cs.params(orc), cs.w, cs.h, *cs.levels())
    awc.same(second, want)
    assert bytes(first) != bytes(second)
    c.close()
    # a setting changed between the enqueue and vis_batch_sync does not alter the queued result
    frames, dev = stream
    ap = vislam.default_align_params()
    sz = PB * C.sizeof(vislam.AlignResult)
    res = {}
    for flip in (False, True, None):
        c = _plan_context(vislam, 0)
        out = torch.zeros(sz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if flip is not None:
            c.set_align_weights(_weights(vislam, 1))
        c.batch_run(dev.data_ptr(), PB, _stages(vislam))
        c.batch_align(ap, dev.data_ptr(), PB, 0, 0, 0, 0, out.data_ptr())
        if flip:
            c.set_align_weights(None)
        c.batch_sync()
        res[flip] = out.cpu().numpy().tobytes()
        c.close()
    assert res[True] == res[False] and res[None] != res[False]
