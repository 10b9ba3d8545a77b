"""CPU: the cases of tests/klt_limit_cases.py are what they claim to be, on the oracle's pyramids and gradients and the restatement
tests/klt_ref.py alone -- the GPU test (tests/test_klt_limits_gpu.py) then only has to compare bytes.

  * the full-contrast scenes take the integer sums beyond 32 bits, saturate the int16 gradients at scale 8, and are still a fair
    tracking problem: at least half of the grid is tracked, the median error against the planted whole-pixel shift is within 4 x the
    figure measured when the cases were written (klt_limit_cases.MEASURED_MEDIAN_ERR);
  * a restatement with one of the five sums wrapped to 32 bits gives other records there -- and none on the blob scene of
    tests/test_klt_gpu.py (printed, not asserted: it documents why that scene could not see an int accumulator);
  * the window edges leave the level exactly where the fit rule says, for every radius;
  * the alternating list alternates, the backward-lost pair loses its backward pass, the guess rows are laid out by the pair."""
import numpy as np
import pytest

import klt_limit_cases as kc
import klt_ref as kr

_cache = {}


def _case(orc, name):
    """(kp, frame 1, frame 2, pts, first-step sums, records without a guess, records with one)"""
    if name not in _cache:
        a, b = kc.full_contrast_frames(name)
        kp = kc.full_contrast_params(name)
        f1, f2 = kr.frame_from(orc, a, kp.scharr_scale), kr.frame_from(orc, b, kp.scharr_scale)
        pts = kc.grid_points(kp.win_radius)
        _cache[name] = (kp, f1, f2, pts, kc.first_sums(kp, f1, f2, pts), kr.track(kp, f1, f2, pts), kr.track(kp, f1, f2, pts, kc.guess_for(pts)))
    return _cache[name]


@pytest.mark.parametrize("name", list(kc.FULL_CONTRAST))
def test_full_contrast_sums_pass_32_bits_and_the_scene_tracks(orc, name):
    kp, f1, f2, pts, s, cold, warm = _case(orc, name)
    m = len(pts)
    assert m == kc.NPOINTS
    gmax = max(int(np.abs(f1[k][0].astype(np.int64)).max()) for k in (1, 2))
    over = {k: int((np.abs(v) > kc.TWO31).sum()) for k, v in s.items()}
    line = f"{name}: max |g| {gmax}, max gxx {float(s['gxx'].max()):.3g}, max |bx| {float(np.abs(s['bx']).max()):.3g}, points above 2^31 {over} of {m}"
    for label, rec in (("cold", cold), ("guess", warm)):
        err = kc.truth_error(pts, rec)
        tracked = int(((rec["flags"] & kr.TRACKED) != 0).sum())
        line += f"; {label}: tracked {tracked}, median error {np.median(err):.5f} px, worst {err.max():.5f} px"
        assert 2 * tracked >= m, line                                                  # a fair tracking problem, not garbage in
        assert np.median(err) <= 4.0 * kc.MEASURED_MEDIAN_ERR[name], line
    print(line)
    assert 2 * over["gxx"] >= m, line
    if name in kc.BX_BEYOND:
        assert 2 * over["bx"] >= m, line
    if kp.scharr_scale == 8 and kc.FULL_CONTRAST[name][0] == "blocks":
        assert gmax == 32640, line                                                     # 16 * 255 * 8: the gradients saturate
    # the pyramid case runs its upper levels (level 3 of 160 x 120 holds no r = 7 window)
    assert int(np.bitwise_or.reduce(cold["levels"])) == (0b0111 if kp.first_level == 3 else 0b0001)


@pytest.mark.parametrize("name", list(kc.SATURATED))
def test_saturated_frames_are_flat_everywhere(orc, name):
    kp, f1, f2, pts, s, cold, warm = _case(orc, name)
    for rec in (cold, warm):
        assert (rec["flags"] == kr.FLAT).all() and (rec["min_eig"] == 0).all() and (rec["levels"] == 0).all()
        assert rec["x"].tobytes() == pts[:, 0].tobytes() and rec["y"].tobytes() == pts[:, 1].tobytes()
    assert all(int(np.abs(v).max()) == 0 for v in s.values())


def test_a_wrapped_sum_changes_records_there_and_none_on_the_blob_scene(orc):
    changed = {}
    for name in kc.FULL_CONTRAST:
        kp, f1, f2, pts, s, cold, _ = _case(orc, name)
        for w in kr.SUMS:
            rec = kr.track(kp, f1, f2, pts, wrap=w)
            changed[name, w] = sum(rec[k].tobytes() != cold[k].tobytes() for k in range(len(pts)))
        print(name, {w: changed[name, w] for w in kr.SUMS})
        # the sums of the template do not depend on the step: where one of them is beyond 32 bits at last_level, the record differs
        for w in ("gxx", "gxy", "gyy"):
            assert changed[name, w] >= 1 or not (np.abs(s[w]) > kc.TWO31).any(), (name, w)
        assert changed[name, "gxx"] >= 1 and changed[name, "gyy"] >= 1
    for w in kr.SUMS:
        assert all(changed[name, w] >= 1 for name in kc.BX_BEYOND), w                 # all five on the scale-8 windows of 225 and 441 pixels
    # the scene every other KLT test uses: nothing to see (the gap this file closes)
    blob = kc.blob_frames(kc.W, kc.H, 2)
    for scale, r in ((3, 7), (8, 10)):
        kp = kr.copy_params(kr.default_params(), scharr_scale=scale, win_radius=r, fb_max_px=1.0)
        f1, f2 = kr.frame_from(orc, blob[0], scale), kr.frame_from(orc, blob[1], scale)
        pts = kc.blob_points(kc.W, kc.H, r, 96)
        base = kr.track(kp, f1, f2, pts)
        print(f"blob scene, scale {scale}, r {r}: records changed by a wrapped sum:",
              {w: sum(a.tobytes() != b.tobytes() for a, b in zip(kr.track(kp, f1, f2, pts, wrap=w), base)) for w in kr.SUMS})


_blob = {}


def _blob_frames(orc):
    if not _blob:
        a, b = kc.blob_frames(kc.W, kc.H, 2)
        _blob["f"] = (kr.frame_from(orc, a), kr.frame_from(orc, b))
    return _blob["f"]


@pytest.mark.parametrize("r", range(2, 11))
def test_window_edges_leave_the_level_where_the_rule_says(orc, r):
    """level 0 only: of the five edge values per axis the second and the fifth are lost before any image is read; the others reach the
    steps at level 0, in both directions of the shift"""
    fa, fb = _blob_frames(orc)
    kp = kr.copy_params(kr.default_params(), win_radius=r, first_level=0, last_level=0)
    pts = kc.edge_points(r)
    lw, lh = kr.half_dims(kc.W, kc.H)
    fit = kr.fits(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64), r, lw[0], lh[0])
    assert fit.tolist() == [not o for o in kc.EDGE_OOB] * 2
    assert float(pts[1, 0]) < r and float(pts[3, 0]) < kc.W - r - 1 and float(pts[6, 1]) < r and float(pts[8, 1]) < kc.H - r - 1   # float32 keeps them apart
    for f1, f2 in ((fa, fb), (fb, fa)):
        rec = kr.track(kp, f1, f2, pts)
        out = np.array(kc.EDGE_OOB * 2)
        assert (rec["flags"][out] == kr.OOB).all() and (rec["levels"][out] == 0).all() and (rec["iters"][out] == 0).all() and (rec["min_eig"][out] == 0).all()
        assert (rec["levels"][~out] == 1).all() and (rec["iters"][~out] >= 1).all() and (rec["min_eig"][~out] > 0).all(), rec[~out]
    assert len(kc.radius_points(r)) == 74


def test_alternating_points_alternate(orc):
    fa, fb = _blob_frames(orc)
    pts = kc.alternating_points(67)
    kp = kr.default_params()
    for f1, f2 in ((fa, fb), (fb, fa)):
        t = (kr.track(kp, f1, f2, pts)["flags"] & kr.TRACKED) != 0
        assert not t[1::2].any() and t[0::2].all()                 # a half-set first ballot of 64, and tracked points behind it
    assert sorted(kc.COUNT_CASES) == [1, 2, 3, 5, 67] and kc.COUNT_CASES[67] == [0, 67, 66, 65, 64, 63, 1, 90]


def test_the_backward_pass_is_lost_on_a_flat_patch(orc):
    a, b, kp, pts, guess = kc.backward_lost_case()
    x0, y0, x1, y1 = kc.PATCH
    r = kp.win_radius
    assert min(x1 - x0, y1 - y0) >= 2 * r + 31 and kp.max_iters == 1 and kp.fb_max_px > 0 and kp.max_err == 0
    f1, f2 = kr.frame_from(orc, a), kr.frame_from(orc, b)
    rec = kr.track(kp, f1, f2, pts, guess)
    lost = rec["fb"] == -1
    print(f"backward pass lost for {lost.sum()} of {len(pts)} points; forward results {rec['x'][lost].min():.2f} ... {rec['x'][lost].max():.2f}, "
          f"{rec['y'][lost].min():.2f} ... {rec['y'][lost].max():.2f}")
    assert lost.sum() >= 10 and (rec["flags"][lost] == kr.FB).all()                    # the forward pass was not lost: FB is the only flag
    # the forward result is reported, and it lies so far inside the patch that the backward window sees nothing but 128 on every level
    fwd = kr.track(kr.copy_params(kp, fb_max_px=0.0), f1, f2, pts, guess)
    assert (fwd["flags"][lost] == kr.TRACKED).all()
    for name in ("x", "y", "sad", "iters", "levels", "min_eig"):
        assert rec[name].tobytes() == fwd[name].tobytes(), name
    m = r + 2 + 8                                                                      # the window, its bilinear neighbour, a level-3 pixel
    assert (rec["x"][lost] >= x0 + m).all() and (rec["x"][lost] <= x1 - 1 - m).all() and (rec["y"][lost] >= y0 + m).all() and (rec["y"][lost] <= y1 - 1 - m).all()
    assert (rec["x"][lost] != pts[lost, 0]).all() and (rec["iters"][lost] == 3).all() and (rec["levels"][lost] == 0b0111).all()
    # the two points outside the patch are tracked, with a forward-backward distance
    assert (rec["flags"][-2:] == kr.TRACKED).all() and (rec["fb"][-2:] >= 0).all()


def test_plan_guess_rows_are_laid_out_by_the_pair():
    kps = [np.zeros(n, [("x", "<f4"), ("y", "<f4")]) for n in (7, 0, 12, 3)]
    for q, k in enumerate(kps):
        k["x"], k["y"] = 100 * q + np.arange(len(k)), 50.0
    links = np.array([-3, 0, -2, 2], np.int32)
    g = kc.plan_guess(links, kps, 15)
    assert g.shape == (4, 15, 2) and g.dtype == np.float32
    assert (g[0] == np.float32(1e30)).all() and (g[2] == np.float32(1e30)).all()
    assert np.isnan(g[1, 7:]).all() and np.isnan(g[3, 12:]).all() and np.isnan(g[3, 4::5]).all() and np.isfinite(g[3, [0, 1, 2, 3, 5, 11]]).all()
    assert g[3, 5, 0] == np.float32(205.0) + np.float32(0.3 + 0.05 * 3) and g[1, 2, 1] == np.float32(50.0) + np.float32(-0.2 - 0.05)
