"""CPU: the cases of tests/stride_range_cases.py are sound on the oracle alone, so that tests/test_stride_range_gpu.py compares the
library with something that means what the case says --
  (a) a numpy restatement of cv::Scharr and cv::addWeighted, written from their definitions (3 / 10 / 3 smoothing across, the central
      difference along, times `scale`, BORDER_REFLECT_101, rint(0.5 |dx|sat + 0.5 |dy|sat) with ties to even), equals
      orc.scharr_gradient on every level of every family A and family B size at scales 1, 3 and 8: the plain reference for levels
      that are 1 or 2 pixels wide;
  (b) non-vacuity: every alignment case shows, on the oracle, the condition it was built for (points accepted in the extra column,
      residuals on every level used, three or more iterations on a level, special values accepted AND rejected as labelled, ...);
  (c) the numpy restatement of the alignment (tests/align_weighted_ref.py) agrees with the oracle on the special-value list and on
      every candidate count.  The oracle's alignment has identity weights only; that is the mode compared here.  For the Tukey modes
      the restatement is the GPU tests' reference, and tests/test_align_weights_ref.py shows its weights equal to the oracle's."""
import numpy as np
import pytest

import align_weighted_ref as ref
import align_weights_cases as awc
import stride_range_cases as src
from test_batch_track_gpu import _Oracle


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def _reflect101_index(n):
    """indices -1 ... n of a line of n pixels under BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba); a line of one pixel repeats it"""
    i = np.arange(-1, n + 1)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def scharr_numpy(img, scale):
    """(dx, dy as int16 with saturation, addWeighted(|dx| sat u8, 0.5, |dy| sat u8, 0.5, 0))"""
    h, w = img.shape
    e = img.astype(np.int64)[_reflect101_index(h)][:, _reflect101_index(w)]              # (h + 2, w + 2): one pixel of border
    smooth_rows = 3 * e[:-2, :] + 10 * e[1:-1, :] + 3 * e[2:, :]                          # across the x derivative: 3 / 10 / 3 over rows
    smooth_cols = 3 * e[:, :-2] + 10 * e[:, 1:-1] + 3 * e[:, 2:]
    dx = (smooth_rows[:, 2:] - smooth_rows[:, :-2]) * scale
    dy = (smooth_cols[2:, :] - smooth_cols[:-2, :]) * scale
    dx16, dy16 = np.clip(dx, -32768, 32767).astype(np.int16), np.clip(dy, -32768, 32767).astype(np.int16)
    a, b = np.minimum(np.abs(dx16.astype(np.int64)), 255), np.minimum(np.abs(dy16.astype(np.int64)), 255)
    return dx16, dy16, np.rint(0.5 * a + 0.5 * b).astype(np.uint8)                        # np.rint: ties to even


@pytest.mark.parametrize("w,h", src.SMALL_SIZES + src.LARGE_SIZES, ids=lambda v: str(v))
def test_scharr_restatement_equals_the_oracle_on_every_level(orc, w, h):
    lw, lh = orc.half_pyramid_dims(w, h)
    seen_one = False
    for kind in ("noise", "checker"):
        for lv in orc.half_pyramid(src.frames_of(kind, w, h, 2)[1]):
            seen_one = seen_one or 1 in lv.shape
            for scale in src.SCALES:
                want, got = orc.scharr_gradient(lv, scale), scharr_numpy(lv, scale)
                for name, a, b in zip(("gx", "gy", "g"), want, got):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (kind, lv.shape, scale, name)
                if lv.shape == (1, 1):
                    assert not want[0].any() and not want[1].any() and not want[2].any()   # a 1 x 1 level: every response is 0
    assert seen_one == (min(lw[4], lh[4]) == 1)


def test_the_sizes_reach_what_they_were_chosen_for(orc):
    dims = {s: orc.half_pyramid_dims(*s) for s in src.SMALL_SIZES + src.LARGE_SIZES}
    assert dims[(16, 16)][0] == [16, 8, 4, 2, 1] and dims[(19, 21)] == ([19, 10, 5, 2, 1], [21, 10, 5, 2, 1])
    assert dims[(23, 23)][0][4] == 2 and dims[(22, 16)][0][4] == 2 and dims[(24, 24)][0][4] == 2
    for s in src.SMALL_SIZES[:6]:
        assert dims[s][0][4] == 1 or dims[s][1][4] == 1, s                                  # sides 16 ... 21: what the launcher refused
    assert dims[(4095, 16)][0] == [4095, 2048, 1024, 512, 256] and 4095 >> 4 == 255
    assert dims[(4094, 18)][0] == [4094, 2047, 1024, 512, 256]
    checker = src.frames_of("checker", 24, 24, 9)
    assert len({f.tobytes() for f in checker}) == 9                                        # the frames of a batch differ
    gx, gy, _ = orc.scharr_gradient(checker[0], 8)
    assert np.abs(gx).max() == 32640 or np.abs(gy).max() == 32640                          # 16 * 255 * 8: the largest response there is


def test_the_restatement_on_values_worked_by_hand():
    img = np.array([[0, 0, 255], [0, 0, 255], [0, 0, 255]], np.uint8)
    dx, dy, g = scharr_numpy(img, 1)
    assert dx[1, 1] == 16 * 255 and dy[1, 1] == 0 and g[1, 1] == 128                       # 127.5 -> 128 (even)
    assert dx[1, 0] == 0 and dx[1, 2] == 0                                                  # reflect 101: both neighbours are the same pixel
    dx, dy, g = scharr_numpy(np.array([[7], [9], [200]], np.uint8), 3)                      # one column: no response across it
    assert not dx.any() and dy[:, 0].tolist() == [0, 3 * 16 * 193, 0] and g[:, 0].tolist() == [0, 128, 0]
    assert scharr_numpy(np.array([[10, 13]], np.uint8), 1)[2].tolist() == [[0, 0]]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def _run(orc, pair, **kw):
    return orc.estimate_pose_features(pair.params(orc, **kw), pair.w, pair.h, *pair.levels(), pair.init(orc))


@pytest.mark.parametrize("w,h", src.LARGE_SIZES, ids=lambda v: str(v))
def test_large_explicit_pair_reaches_the_extra_column(orc, w, h):
    pair = src.large_explicit_pair(orc, w, h)
    full = _run(orc, pair)
    assert all(full.n_residuals[l] > 0 for l in range(5)), list(full.n_residuals)
    lw, lh = orc.half_pyramid_dims(w, h)
    sx, sy = src.large_shift(w, h)
    landed = 0
    for lvl in range(5):
        book, own = (w >> lvl, lw[lvl]) if w >= h else (h >> lvl, lh[lvl])
        if own == book:
            continue
        edge = src.large_edge_points(w, h, lvl)
        # the edge coordinate is book - 1 and the pose moves it by 1.2 px: past the bookkeeping size, inside the level's own
        assert book <= (book - 1) + src.LARGE_SHIFT_LONG < own
        only = [np.zeros((0, 4), np.float32)] * 5
        only[lvl] = edge
        q = pair.with_cand("edge", only)
        r = _run(orc, q, first=lvl, last=lvl, iters=1)
        assert r.n_residuals[lvl] == len(edge), (lvl, r.n_residuals[lvl], len(edge))       # all of them counted: they are in the extra column / row
        landed += len(edge)
    assert landed > 0
    assert sx > 0 and sy > 0


def test_large_generated_case(orc, vislam):
    g = src.large_generated(orc, vislam)
    r = _run(orc, g["pair"])
    assert r.n_residuals[0] > 0 and all(r.n_residuals[l] > 0 for l in range(4)), list(r.n_residuals)
    assert g["pair"].cand[0][:, 0].max() == 4094                                           # the largest x the packed word can hold a pixel at


def test_align_320_case(orc, vislam):
    a = src.align_320(orc, vislam)
    for t in (1, 2):
        assert a["want"][t].n_residuals[0] > 0, t
    assert a["want"][1].pose.as_array().tobytes() != a["want"][2].pose.as_array().tobytes()


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
@pytest.mark.parametrize("w,stride", src.PLAN_SHAPES, ids=lambda v: str(v))
def test_plan_stream_pairs_on_the_oracle(vislam, orc, canvas, w, stride, gate):
    """the oracle's own detection, matching and alignment over the stream: every pair has good matches and level-0 residuals; with the
    gate, frame 7 is refused and frame 8 pairs with frame 6 (the keyframe carried into the second launch is not the launch's last frame)"""
    assert stride % 4 == 0 and stride > w and ((w | stride) & 3 == 0) == (w == 320)
    frames = src.plan_frames(vislam, canvas, w, gate)
    p = src.plan_params(vislam, w, src.PLAN_H, gate)
    kd = [orc.orb_detect_compute(p, f) for f in frames]
    prev = src.plan_walk(vislam, gate, [len(k) for k, _ in kd], len(frames))
    if gate:
        assert prev[7] is None and prev[8] == 6 and len(kd[7][0]) == 0
    assert sum(q is not None for q in prev) == len(frames) - (2 if gate else 1)
    oracle = _Oracle(orc, frames, w, src.PLAN_H)
    for g, j in enumerate(prev):
        if j is None:
            continue
        o12, o21 = orc.knn2_hamming(kd[j][1], kd[g][1])
        good, _ = orc.good_matches(p, kd[j][0], kd[g][0], o12, o21)
        assert len(good) > 0, g
        assert oracle.align(j, g, kd[j][0][good["queryIdx"]]).n_residuals[0] > 0, g


def test_count_cases_on_the_oracle(vislam, orc, canvas):
    """every count: residuals on every level used, and the restatement equal to the oracle (identity weights); over the counts at least
    one level runs 3 or more iterations (what grad_div is for)"""
    most = 0
    for n in src.LIST_COUNTS:
        for first, last in src.LIST_LEVELS:
            pair = src.count_pair(vislam, orc, canvas, n, first, last)
            assert all(len(pair.cand[l]) == n for l in range(last, first + 1))
            want = _run(orc, pair)
            assert all(want.n_residuals[l] > 0 for l in range(last, first + 1)), (n, first, last, list(want.n_residuals))
            most = max(most, max(want.iterations))
            got = ref.estimate_pose_features(orc, pair.params(orc), pair.w, pair.h, *pair.levels(), pair.init(orc))
            awc.same(got, want)
    assert most >= 3, most
    small = src.count_pair(vislam, orc, canvas, 256, 3, 0)
    assert max(_run(orc, small).iterations) >= 3


def test_special_values_are_accepted_and_rejected_as_labelled(vislam, orc, canvas):
    pair = src.special_pair(vislam, orc, canvas)
    for lvl in range(pair.last, pair.first + 1):
        rows = src.special_rows(src.SMALL_W >> lvl, src.SMALL_H >> lvl)
        assert all(abs(v) < 2 ** 20 and np.isfinite(v) for r in pair.cand[lvl] for v in r)
        verdict = {}
        for i, (kind, *_, accepted) in enumerate(rows):
            only = [np.zeros((0, 4), np.float32)] * 5
            only[lvl] = pair.cand[lvl][i:i + 1]
            r = _run(orc, pair.with_cand("one", only), first=lvl, last=lvl, iters=1)
            assert r.n_residuals[lvl] == int(accepted), (lvl, i, kind, rows[i], r.n_residuals[lvl])
            verdict.setdefault(kind, set()).add(accepted)
        for kind, seen in verdict.items():
            if kind == "ordinary":
                assert seen == {True}
            elif kind in ("z=0", "x=cols", "y=rows", "x=-1", "y=-1", "w=0"):
                assert seen == {False}, kind                        # the rule allows no accepted member
            else:
                assert seen == {True, False}, kind
        assert {"x=-0.5", "y=-0.5", "x=0.5", "x=cols-0.5", "y=rows-0.5", "x=cols", "x=-1", "z=0.5", "z=2", "z=0", "z=-1", "w=0.5", "w=0"} <= set(verdict)
    full = _run(orc, pair)
    assert all(full.n_residuals[l] > 0 for l in range(4)) and max(full.iterations) >= 3, (list(full.n_residuals), list(full.iterations))


def test_generated_rows_on_the_oracle(vislam, orc):
    g = src.generated_small(vislam, orc)
    assert sorted(g) == [1, 20, 230]
    by_npts = {p.npts: p for p in g[230]["pairs"].values()}
    assert sorted(by_npts) == [0, 1, 199, 200, 201, 230]
    assert len(by_npts[200].cand[0]) == 200 * 121 and len(by_npts[199].cand[0]) == 199 * 121
    for np_, p in by_npts.items():
        r = _run(orc, p)
        # (one keypoint: the first level has residuals; what its 25 pixels do to the pose decides about the finer levels)
        assert (r.n_residuals[0 if np_ > 1 else 3] > 0) == (np_ > 0), (np_, list(r.n_residuals))
    # 201 and 230 use the first 200 points like 200 does -- of their own rows of points, so the lists have the same length only
    assert len(by_npts[201].cand[0]) == len(by_npts[230].cand[0]) == 200 * 121
    clamp = g[20]["pairs"][1]
    assert clamp.npts == 50 and len(clamp.cand[0]) == 20 * 121 and _run(orc, clamp).n_residuals[0] > 0
    one = g[1]["pairs"][1]
    assert one.npts == 1 and len(one.cand[0]) == 121 and _run(orc, one).n_residuals[3] > 0


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_on_the_special_values(vislam, orc, canvas):
    pair = src.special_pair(vislam, orc, canvas)
    want = _run(orc, pair)
    awc.same(ref.estimate_pose_features(orc, pair.params(orc), pair.w, pair.h, *pair.levels(), pair.init(orc)), want)
    # the Tukey modes run on the same list and are not the identity result (the GPU test can tell the modes apart)
    seen = {want.pose.as_array().tobytes()}
    for mode in (1, 2):
        r = ref.estimate_pose_features(orc, pair.params(orc), pair.w, pair.h, *pair.levels(), pair.init(orc), weights=mode)
        assert sum(r.n_residuals) > 0
        seen.add(r.pose.as_array().tobytes())
    assert len(seen) >= 2


def test_patch_keypoints_sit_on_and_beside_every_border(vislam, orc):
    for w, h in src.PATCH_SIZES:
        k199, k201 = src.patch_keypoints(vislam, w, h, 199), src.patch_keypoints(vislam, w, h, 201)
        assert k201[:199].tobytes() == k199.tobytes()
        for v, n in ((k201["x"], w), (k201["y"], h)):
            assert {0.0, 0.5, -1.0, -0.5, n - 1.0, n - 0.5, float(n), n + 1.0} <= set(v.tolist())
        for l in range(5):
            a, b = orc.patch_points(k199, w, h, l), orc.patch_points(k201, w, h, l)
            assert len(orc.patch_points(src.patch_keypoints(vislam, w, h, 200), w, h, l)) == len(b) >= len(a)
            assert len(orc.debug_points(k201, l)) == 200 and len(orc.debug_points(k199, l)) == 199
        assert len(orc.patch_points(k201, w, h, 0)) > 0
