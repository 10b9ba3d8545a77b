"""GPU: pyramidal KLT at the limits of tests/klt_limit_cases.py -- integer sums beyond 32 bits, every window radius on both sides of the
k_klt<4> | k_klt<7> dispatch with the exact ends of the fit rule, point counts off the four waves of a workgroup and the 64 lanes of a
ballot, a lost backward pass, and vis_batch_klt with guess rows, a row_cap above the plan's capacity and a frame the gate skips.

Everything is compared with tests/klt_ref.py byte for byte: point records, pair records and compacted rows, behind 0xEE guard fills
(tests/klt_device.py).  tests/test_klt_limits_ref.py proves on the CPU that the cases reach what they are meant to reach."""
import numpy as np
import pytest

import klt_limit_cases as kc
import klt_ref as kr
from klt_device import FILL, PB, PH, PW, Set, compare, launch, plan_launches, want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c(vislam):
    ctx = vislam.Context(0)
    yield ctx
    ctx.close()


_sets = {}


def _set(vislam, c, key, frames, scale=3):
    import torch
    if (key, scale) not in _sets:
        _sets[key, scale] = Set(vislam, torch, c, frames, frames.shape[2], scale)
    return _sets[key, scale]


def _blob_set(vislam, c, n):
    return _set(vislam, c, ("blob", n), kc.blob_frames(kc.W, kc.H, n))


def _one_pair(pts, guess=None):
    """rows of a two-frame call: row 0 (no pair) holds other points than the pair's"""
    m = len(pts)
    rows = np.stack([pts[::-1], pts])
    return rows, np.array([m, m], np.int32), None if guess is None else np.stack([np.full_like(guess, 7.0), guess])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(kc.FULL_CONTRAST) + list(kc.SATURATED))
def test_full_contrast_sums(vislam, c, name):
    """gxx, gxy, gyy, bx, by beyond 2^31 (an int accumulator gives other records: test_klt_limits_ref.py), int16 gradients at their end,
    and frames without any gradient; with and without a guess, forward-backward on"""
    import torch
    kp = kc.full_contrast_params(name)
    S = _set(vislam, c, name, np.stack(kc.full_contrast_frames(name)), kp.scharr_scale)
    base = kc.grid_points(kp.win_radius)
    for guess in (None, kc.guess_for(base)):
        pts, npts, g = _one_pair(base, guess)
        w = want(S, kp, pts, npts, g, len(base))
        seen = compare(launch(vislam, torch, c, S, kp, pts, npts, g, len(base)), w, pts, npts, len(base), (name, guess is not None))
        if name in kc.SATURATED:
            assert seen == kr.FLAT
        else:
            assert seen & kr.TRACKED and 2 * int(((w[0]["flags"] & kr.TRACKED) != 0).sum()) >= len(base)
            if kc.FULL_CONTRAST[name][0] == "blocks" and kp.scharr_scale == 8:     # the device's own gradients reach the int16 end
                assert max(int(np.abs(S.host[0][k][0].astype(np.int64)).max()) for k in (1, 2)) == 32640


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("r", range(2, 11))
def test_every_window_radius(vislam, c, r):
    """49 ... 441 window pixels in the 256 slots of k_klt<4> (r <= 7) and the 448 of k_klt<7>, through the pyramid and at level 0 alone,
    where the exact ends of the fit rule are in the list: the float below r and lw - r - 1 itself are lost, their neighbours are not"""
    import torch
    S = _blob_set(vislam, c, 3)
    base = kc.radius_points(r)
    m = len(base)
    pts, npts = np.stack([base, base, np.roll(base, 5, axis=0)]), np.array([3, m, m], np.int32)
    for change in (dict(), dict(first_level=0, last_level=0)):
        kp = kr.copy_params(kr.default_params(), win_radius=r, **change)
        w = want(S, kp, pts, npts, None, m)
        seen = compare(launch(vislam, torch, c, S, kp, pts, npts, None, m), w, pts, npts, m, (r, change))
        assert seen & kr.TRACKED and seen & kr.OOB
        if change:
            edges = w[0][-10:]
            out = np.array(kc.EDGE_OOB * 2)
            assert (edges["flags"][out] == kr.OOB).all() and (edges["levels"][out] == 0).all() and (edges["levels"][~out] == 1).all(), edges


@pytest.mark.parametrize("r", [7, 8])
def test_window_radius_at_the_dispatch_on_blocks(vislam, c, r):
    """225 pixels in k_klt<4>, 289 in k_klt<7>, on full contrast: a window pixel dropped or counted twice changes every sum"""
    import torch
    kp = kr.copy_params(kr.default_params(), win_radius=r, fb_max_px=1.0)
    S = _set(vislam, c, "blocks6", np.stack(kc.moved_pair("blocks", 6)))
    pts, npts, _ = _one_pair(kc.grid_points(r))
    w = want(S, kp, pts, npts, None, kc.NPOINTS)
    seen = compare(launch(vislam, torch, c, S, kp, pts, npts, None, kc.NPOINTS), w, pts, npts, kc.NPOINTS, ("blocks6", r))
    assert seen & kr.TRACKED and 2 * int(((w[0]["flags"] & kr.TRACKED) != 0).sum()) >= kc.NPOINTS


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("max_pts", sorted(kc.COUNT_CASES))
def test_point_counts_off_the_wave_and_ballot_sizes(vislam, c, max_pts):
    """max_pts that is no multiple of the four waves of a workgroup (the k >= max_pts exit of a partly filled one), counts on both sides
    of the 64 lanes of k_klt_pairs' ballot, a count above max_pts; tracked and untracked points alternate"""
    import torch
    npts = np.array(kc.COUNT_CASES[max_pts], np.int32)
    n = len(npts)
    S = _blob_set(vislam, c, n)
    base = kc.alternating_points(max_pts)
    pts = np.stack([np.roll(base, i, axis=0) for i in range(n)])   # odd pairs: the untracked points come first
    kp = kr.default_params()
    w = want(S, kp, pts, npts, None, max_pts)
    got = launch(vislam, torch, c, S, kp, pts, npts, None, max_pts)
    seen = compare(got, w, pts, npts, max_pts, max_pts)
    assert seen & kr.TRACKED
    assert [int(v) for v in got[1]["n_points"]] == [0] + [min(int(v), max_pts) for v in npts[1:]]
    if max_pts == 67:
        t = (w[0]["flags"] & kr.TRACKED) != 0                      # pair 1, 67 points: a partly set first ballot, tracked points behind it
        assert 0 < t[:64].sum() < 64 and t[64:].any() and int(got[4][1]) == t.sum()
    # and without the compacted rows
    got2 = launch(vislam, torch, c, S, kp, pts, npts, None, max_pts, compacted=False)
    assert got2[0].tobytes() == got[0].tobytes() and got2[1].tobytes() == got[1].tobytes()


# ---------------------------------------------------------------------------------------------- 4
def test_backward_pass_lost(vislam, c):
    import torch
    a, b, kp, base, guess = kc.backward_lost_case()
    S = _set(vislam, c, "backward_lost", np.stack([a, b]))
    pts, npts, g = _one_pair(base, guess)
    m = len(base)
    w = want(S, kp, pts, npts, g, m)
    got = launch(vislam, torch, c, S, kp, pts, npts, g, m)
    compare(got, w, pts, npts, m, "backward lost")
    rec = got[0][1]
    lost = rec["fb"] == -1
    assert lost.sum() >= 10 and (rec["flags"][lost] == kr.FB).all() and int(got[1][1]["n_fb"]) >= lost.sum()
    fwd = launch(vislam, torch, c, S, kr.copy_params(kp, fb_max_px=0.0), pts, npts, g, m)[0][1]     # the forward pass alone
    assert (fwd["flags"][lost] == kr.TRACKED).all()
    assert rec["x"].tobytes() == fwd["x"].tobytes() and rec["y"].tobytes() == fwd["y"].tobytes() and (rec["x"][lost] != base[lost, 0]).all()


# ---------------------------------------------------------------------------------------------- 5, 6
_plan_cache = {}
ONE_STEP = dict(max_iters=1)


def _plan(vislam, canvas, gate):
    """the two launches, each with vis_batch_klt run on the same vis_batch_run without a guess (L itself: forward-backward on) and, in
    L["runs"], with the guess rows of klt_limit_cases.plan_guess at one step per level and at the defaults (gate on: also one step
    without a guess)"""
    import torch
    if gate not in _plan_cache:
        frames = np.stack([vislam.synth_frame(canvas, t, PW, PH) for t in range(2 * PB)])
        if gate:
            frames[3] = frames[PB + 3] = 128
        one = kr.copy_params(kr.default_params(), **ONE_STEP)
        runs = [(one, kc.plan_guess), (kr.default_params(), kc.plan_guess)] + ([(one, None)] if gate else [])
        _plan_cache[gate] = plan_launches(vislam, torch, frames, gate, kr.copy_params(kr.default_params(), fb_max_px=1.0), extra=5, runs=runs)
    return _plan_cache[gate]


_track_cache = {}


def _track(gate, li, i, R, guess_row):
    """the restatement of pair i of one run, with the guess row `guess_row` (None: without a guess)"""
    kp = R["kp"]
    key = (gate, li, i, kp.max_iters, kp.fb_max_px, None if R["guess"] is None else guess_row)
    if key not in _track_cache:
        q = int(R["links"][i])
        k1 = R["kps"][q]
        pts = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
        g = None if R["guess"] is None else R["guess"][guess_row, :len(k1)]
        _track_cache[key] = (pts, kr.track(kp, R["host"][q], R["host"][i], pts, g))
    return _track_cache[key]


def _check_plan_run(gate, li, R):
    """every row of one vis_batch_klt at the stride row_cap; -> (pairs, tracked points, pairs whose records differ from the restatement
    made with the guess row of the previous frame q instead of the pair i)"""
    cap, rc = R["cap"], R["row_cap"]
    assert rc == cap + 5 and R["recs"].shape == (PB, rc) and R["p1"].shape == (PB, rc * 8)
    n_pairs = n_tracked = by_q_differs = 0
    for i in range(PB):
        q = int(R["links"][i])
        assert (R["recs"][i, cap:].view(np.uint8) == FILL).all(), (li, i)              # the five records behind the plan's capacity
        if q < 0:
            assert not R["recs"][i, :cap].tobytes().strip(b"\0"), (li, i)
            assert R["pairs"][i].tobytes() == kr.pair_record(None, no_pair=True).tobytes() and int(R["nt"][i]) == 0, (li, i)
            assert (R["p1"][i] == FILL).all() and (R["p2"][i] == FILL).all()
            continue
        pts, w = _track(gate, li, i, R, i)
        m = len(pts)
        assert 0 < m <= cap
        if R["recs"][i, :m].tobytes() != w.tobytes():
            bad = [k for k in range(m) if R["recs"][i, k].tobytes() != w[k].tobytes()]
            raise AssertionError((li, i, q, bad[:5], [(pts[k].tolist(), R["recs"][i, k], w[k]) for k in bad[:3]]))
        assert (R["recs"][i, m:].view(np.uint8) == FILL).all(), (li, i)
        assert R["pairs"][i].tobytes() == kr.pair_record(w).tobytes(), (li, i)
        a, b = kr.compact(pts, w)
        k = len(a)
        assert int(R["nt"][i]) == k and R["p1"][i, :k * 8].tobytes() == a.tobytes() and R["p2"][i, :k * 8].tobytes() == b.tobytes(), (li, i)
        assert (R["p1"][i, k * 8:] == FILL).all() and (R["p2"][i, k * 8:] == FILL).all(), (li, i)
        n_pairs += 1
        n_tracked += k
        if R["guess"] is not None and R["kp"].max_iters == 1:
            by_q_differs += R["recs"][i, :m].tobytes() != _track(gate, li, i, R, q)[1].tobytes()
    return n_pairs, n_tracked, by_q_differs


def test_plan_guess_rows_and_row_cap(vislam, canvas):
    """vis_batch_klt with a guess: the points and counts are rows of the pair's PREVIOUS frame at the plan's stride, the guess and every
    output are rows of the PAIR at the caller's row_cap.  One step per level makes the result a function of the guess"""
    launches = _plan(vislam, canvas, False)
    for li, L in enumerate(launches):
        links = [int(v) for v in L["links"]]
        assert links == [vislam.KF_FIRST if li == 0 else vislam.KF_CARRIED] + list(range(PB - 1))
        assert _check_plan_run(False, li, L)[0] == PB - 1
        for R in L["runs"]:
            n_pairs, n_tracked, by_q = _check_plan_run(False, li, R)
            assert n_pairs == PB - 1 and n_tracked >= 20 * n_pairs
            if R["guess"] is not None:
                g = R["guess"]
                assert (g[0] == np.float32(1e30)).all() and np.isnan(g[1:, 4::5]).all() and np.isnan(g[1:, L["cap"]:]).all()
                if R["kp"].max_iters == 1:
                    assert by_q >= 1                               # the test can see which row the guess is read from


def test_plan_gate_skips_a_frame(vislam, canvas):
    """gate on, frame 3 of each launch flat: frame 4 is paired with frame 2, so the points of pair 4 are row 2 of the keypoints while its
    guess and outputs are row 4; the first frame of the second launch is paired with the carried frame (no pair here)"""
    launches = _plan(vislam, canvas, True)
    for li, L in enumerate(launches):
        links = [int(v) for v in L["links"]]
        assert links == [vislam.KF_FIRST if li == 0 else vislam.KF_CARRIED, 0, 1, vislam.KF_NOT_SAVED, 2, 4, 5, 6], (li, links)
        assert len(L["kps"][3]) == 0
        assert _check_plan_run(True, li, L)[0] == PB - 2
        by_q_seen = 0
        for R in L["runs"]:
            n_pairs, n_tracked, by_q = _check_plan_run(True, li, R)
            assert n_pairs == PB - 2 and n_tracked >= 20 * n_pairs
            by_q_seen += by_q
            # pair 4 tracks the keypoints of frame 2, which are not those of frame 3 (none) or of frame 4
            assert R["kps"][2].tobytes() != R["kps"][4].tobytes()
            assert int(R["pairs"][4]["n_points"]) == len(R["kps"][2]) and int(R["pairs"][3]["flags"]) == kr.NO_PAIR
        assert by_q_seen >= 1
        # one step from the guess and one step from nothing end elsewhere
        assert L["runs"][0]["recs"][4].tobytes() != L["runs"][2]["recs"][4].tobytes()
