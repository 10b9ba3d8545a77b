"""GPU: pyramidal KLT (vis_klt_batch / vis_klt_track / vis_batch_klt) against the restatement tests/klt_ref.py, run on the pyramids and
gradients downloaded from the device: point records, pair records and compacted rows byte for byte.  Output buffers are pre-filled with
0xEE and everything the call must not write is checked to keep it.

Scenes: tests/klt_ref.py blob_frames (analytic, with a textureless box) at 160 x 120 (level 3 is 20 x 15: r = 7 fits nowhere, the level is
skipped for every point), 150 x 110 (half-to-even level sizes: level 2 is 38 x 28), both also at a padded stride, and 16 x 16 with r = 2."""
import numpy as np
import pytest

import homography_ref as hr
import klt_ref as kr
import stride_range_cases as src
from klt_device import FILL, PB, PH, PW, REC, Set as _Set, compare as _compare, dev as _dev, filled as _filled, launch as _launch
from klt_device import plan_launches as _plan_launches, want as _want
from klt_limit_cases import BLOB_SHIFT as SHIFT, blob_frames as _frames, blob_points as _points

pytestmark = pytest.mark.gpu
_want_cache = {}


def _rows(w, h, r, n, max_pts, npts, seed=0):
    """per pair a different rotation of the point list; (pts n x max_pts x 2, npts, guess with NaN and useless entries mixed in)"""
    base = _points(w, h, r, max_pts)
    pts = np.stack([np.roll(base, 7 * i + seed, axis=0) for i in range(n)])
    sh = np.array(SHIFT if w >= 64 else (0.6, -0.4), np.float32)
    guess = pts + np.where((np.arange(n) % 2 == 1)[:, None, None], sh, -sh).astype(np.float32) + np.float32(0.4)
    guess[:, 2::5, 0] = np.nan                                     # a non-finite guess is treated as absent
    guess[:, 3::11] = np.float32(1e30)                             # a finite absurd one is used: the window leaves the level
    return pts, np.asarray(npts, np.int32), guess.astype(np.float32)


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
