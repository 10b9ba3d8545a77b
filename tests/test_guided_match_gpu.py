"""GPU: rotation-guided matching (vis_warp_keypoints, vis_bf_knn2_hamming_guided / _guided_host, vis_good_matches_guided,
vis_batch_run_guided) against tests/guided_match_ref.py -- exact equality everywhere.  The fixtures and what each of them exercises
are described, and their preconditions asserted on the CPU, in tests/guided_match_ref.py / tests/test_guided_match_ref.py."""
import numpy as np
import pytest

import guided_match_ref as gr

pytestmark = pytest.mark.gpu
F32 = np.float32
ROT, RADIUS = gr.SMALL_ROT, gr.RADIUS


@pytest.fixture(scope="module")
def pop_ctx(vislam):
    """keypoint_capacity 16385: rows beyond the MFMA kernel's 16384, so the popcount kernel runs (slots and host form alike)"""
    p = vislam.default_params()
    p.keypoint_capacity = 16385
    c = vislam.Context(0, p)
    yield c
    c.close()


def _run(c, case, rot=ROT, radius=RADIUS):
    d1, xy1, d2, xy2 = case[:4]
    return c.bf_knn2_hamming_guided_host(d1, gr.keypoints(xy1), d2, gr.keypoints(xy2), rot, radius)


def _check(c, case, rot=ROT, radius=RADIUS, what=""):
    d1, xy1, d2, xy2 = case[:4]
    k12, k21, _ = gr.knn2(d1, xy1, d2, xy2, rot, radius)
    g12, g21 = _run(c, case, rot, radius)
    w12, w21 = gr.dmatches(k12), gr.dmatches(k21)
    assert g12.tobytes() == w12.tobytes(), (what, "12", np.argwhere((g12["trainIdx"] != w12["trainIdx"]) | (g12["distance"] != w12["distance"]))[:4])
    assert g21.tobytes() == w21.tobytes(), (what, "21", np.argwhere((g21["trainIdx"] != w21["trainIdx"]) | (g21["distance"] != w21["distance"]))[:4])
    return g12, g21


# ---------------------------------------------------------------------------------------------------------------- the prediction
def test_warp_is_bit_equal_to_the_reference(ctx):
    pts = gr.warp_points()
    for k, rot in enumerate(gr.WARP_ROTS):
        got, want = ctx.warp_keypoints(gr.keypoints(pts), rot), gr.warp(pts, rot)
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), k
        assert got[~nan].tobytes() == want[~nan].tobytes(), (k, np.argwhere(got != want)[:4])
        if k == 2:
            assert nan.any() and (nan[:, 0] == nan[:, 1]).all()    # X_2 <= 0: (NaN, NaN)
    assert ctx.warp_keypoints(gr.keypoints(pts[:0]), gr.WARP_ROTS[1]).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------- MFMA kernel
@pytest.mark.parametrize("n_prev", gr.PREV_SIZES)
def test_mfma_kernel_sizes(ctx, n_prev):
    for n_cur in gr.CUR_SIZES:
        _check(ctx, gr.sized_case(n_prev, n_cur), what=(n_prev, n_cur))


def test_mfma_kernel_long_sweep(ctx):
    g12, g21 = _check(ctx, gr.long_sweep_case(), what="40 x 16384")
    t = g12["trainIdx"]
    assert ((t[:, 0] >= 0) & (t[:, 0] < 32)).any() and (t[:, 0] >= 16384 - 32).any()


# ---------------------------------------------------------------------------------------------------------------- popcount kernel
@pytest.mark.parametrize("nq", gr.POP_QUERIES)
def test_popcount_kernel_sizes(pop_ctx, nq):
    for ns in gr.POP_SWEPT:
        d1, xy1, d2, xy2 = gr.sized_case(nq, ns, seed=7000 + 100 * nq + ns)
        _check(pop_ctx, (d1, xy1, d2, xy2), what=("prev", nq, "cur", ns))
        _check(pop_ctx, (d2, xy2, d1, xy1), what=("prev", ns, "cur", nq))        # the sets exchanged: each direction sweeps each length


def test_both_kernels_agree(ctx, pop_ctx):
    case = gr.semantics_case()
    a12, a21 = _run(ctx, case)
    b12, b21 = _run(pop_ctx, case)
    assert a12.tobytes() == b12.tobytes() and a21.tobytes() == b21.tobytes()


# ---------------------------------------------------------------------------------------------------------------- window semantics
@pytest.fixture(scope="module")
def slots(vislam, canvas):
    """two frames of the synthetic stream in slots 0 (previous) and 1 (current) of a context of its own"""
    c = vislam.Context(0)
    ks = [c.orb_detect_compute(vislam.synth_frame(canvas, t, 752, 480), slot=s) for s, t in enumerate((3, 4))]
    assert min(len(k) for k, _ in ks) > 300
    yield c, ks
    c.close()


def test_everything_admissible_equals_the_unguided_matcher(slots):
    c, ((k1, _), (k2, _)) = slots
    u12, u21 = c.bf_knn2_hamming(0, 1, len(k1), len(k2))
    g12, g21 = c.bf_knn2_hamming_guided(0, 1, len(k1), len(k2), np.eye(3, dtype=F32), 1e30)
    assert g12.tobytes() == u12.tobytes() and g21.tobytes() == u21.tobytes()
    assert c.timings().ms_knn > 0


def test_nothing_admissible(slots):
    c, ((k1, d1), (k2, d2)) = slots
    rot = gr.rot_y(20.0).astype(F32)                               # every prediction lands hundreds of pixels away
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    assert not gr.admissible(xy1, gr.warp(xy2, rot), 0.0).any()
    g12, g21 = c.bf_knn2_hamming_guided(0, 1, len(k1), len(k2), rot, 0.0)
    assert (g12["trainIdx"] == -1).all() and (g21["trainIdx"] == -1).all()
    assert g12.tobytes() == gr.dmatches(np.full((len(k1), 2), gr.NONE)).tobytes()
    good, sym = c.good_matches_guided(0, 1, rot, 0.0)
    assert len(good) == 0 and len(sym) == 0


def test_slots_equal_the_reference_and_the_host_form(slots):
    c, ((k1, d1), (k2, d2)) = slots
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    for radius in (4.0, 16.0):
        k12, k21, adm = gr.knn2(d1, xy1, d2, xy2, ROT, radius)
        g12, g21 = c.bf_knn2_hamming_guided(0, 1, len(k1), len(k2), ROT, radius)
        assert g12.tobytes() == gr.dmatches(k12).tobytes() and g21.tobytes() == gr.dmatches(k21).tobytes()
        h12, h21 = c.bf_knn2_hamming_guided_host(d1, k1, d2, k2, ROT, radius)
        assert h12.tobytes() == g12.tobytes() and h21.tobytes() == g21.tobytes()
        assert adm.any() and not adm.all(1).any()


def test_one_and_two_candidates_edges_masked_winners_and_ties(ctx):
    case = gr.semantics_case()
    d1, xy1, d2, xy2, rows = case
    g12, g21 = _check(ctx, case, what="semantics")
    adm = gr.admissible(xy1, gr.warp(xy2, ROT), RADIUS)
    for g, a in ((g12, adm), (g21, adm.T)):                        # rows with exactly one and exactly two candidates (and none)
        counts = a.sum(1)
        have = (g["trainIdx"] >= 0).sum(1)
        assert (have[counts == 0] == 0).all() and (have[counts == 1] == 1).all() and (have[counts >= 2] == 2).all()
        assert (counts == 1).any() and (counts == 2).any()
        one = np.flatnonzero(counts == 1)
        assert (g["trainIdx"][one, 0] == a[one].argmax(1)).all() and (g["trainIdx"][one, 1] == -1).all()
    # exactly radius: admitted; the next float beyond it: not, although it is the closer descriptor
    e, at, beyond = rows["cur_edge"], rows["prev_at"], rows["prev_beyond"]
    assert g21["trainIdx"][e].tolist() == [at, -1] and g21["distance"][e, 0] == 9
    assert g12["trainIdx"][at].tolist() == [e, -1] and g12["trainIdx"][beyond].tolist() == [-1, -1]
    # the inadmissible row with the smaller distance and the lower index does not appear
    assert g21["trainIdx"][rows["cur_victim"]].tolist() == [rows["prev_ok"], -1] and g21["distance"][rows["cur_victim"], 0] == 5
    assert g12["trainIdx"][rows["prev_victim"]].tolist() == [rows["cur_ok"], -1] and g12["distance"][rows["prev_victim"], 0] == 5
    assert (g12["trainIdx"][rows["prev_far"]] == -1).all() and (g21["trainIdx"][rows["cur_far"]] == -1).all()
    # ties: the lower index first
    assert g21["trainIdx"][rows["tie_cur"]].tolist() == list(rows["tie_prev_pair"])
    assert g12["trainIdx"][rows["tie_prev"]].tolist() == list(rows["tie_cur_pair"])


def test_nan_predictions_match_nothing(ctx, pop_ctx):
    case = gr.nan_case()
    nan = np.isnan(gr.warp(case[3], gr.NAN_ROT)[:, 0])
    for c in (ctx, pop_ctx):
        g12, g21 = _check(c, case, rot=gr.NAN_ROT, what="nan")
        assert (g21["trainIdx"][nan] == -1).all()
        assert not np.isin(g12["trainIdx"], np.flatnonzero(nan)).any()
        assert (g21["trainIdx"][~nan, 0] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- filters
def test_good_matches_on_the_windowed_2nn(slots):
    c, ((k1, d1), (k2, d2)) = slots
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    sizes = []
    for radius in (6.0, 16.0):
        k12, k21, _ = gr.knn2(d1, xy1, d2, xy2, ROT, radius)
        want_good, want_sym = c.good_matches_host(k1, k2, gr.dmatches(k12), gr.dmatches(k21))
        good, sym = c.good_matches_guided(0, 1, ROT, radius)
        assert good.tobytes() == want_good.tobytes() and sym.tobytes() == want_sym.tobytes(), radius
        sizes.append((len(good), len(sym)))
    print(f"good / symmetric matches at radius 6 and 16: {sizes}")
    assert sizes[1][1] > 0


def test_state_refusals(vislam, slots):
    import ctypes as C
    c = vislam.Context(0)
    rot = np.eye(3, dtype=F32).reshape(9)
    R, out = rot.ctypes.data_as(C.c_void_p), np.zeros((8, 2), vislam.DMATCH_DTYPE)
    O = out.ctypes.data_as(C.c_void_p)
    n = C.c_int(0)
    L = vislam.lib
    assert L.vis_bf_knn2_hamming_guided(c._h, 0, 1, R, 8.0, O, O) == -5                            # no single-frame plan
    assert L.vis_good_matches_guided(c._h, 0, 1, R, 8.0, O, 8, C.byref(n), None, 0, None) == -5
    assert L.vis_batch_run_guided(c._h, C.c_void_p(64), 1, vislam.STAGE_ALL, C.c_void_p(64), 8.0) == -5   # no batch plan
    c.close()
    c = slots[0]
    assert L.vis_bf_knn2_hamming_guided(c._h, 0, 7, R, 8.0, O, O) == -5                            # an empty slot
    assert L.vis_bf_knn2_hamming_guided(c._h, 0, 32, R, 8.0, O, O) == -1                           # no such slot


# ---------------------------------------------------------------------------------------------------------------- batch
BW, BH, BN = 160, 120, 6


def _batch_params(vislam, **kw):
    p = vislam.default_params()
    p.w_size, p.h_size = BW, BH
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    """12 frames of the synthetic stream at 160 x 120, one small random rotation per frame"""
    frames = np.stack([vislam.synth_frame(canvas, t, BW, BH) for t in range(2 * BN)])
    rng = np.random.default_rng(21)
    rots = np.stack([gr.rodrigues(rng.normal(0, 0.01, 3)) for _ in range(2 * BN)]).astype(F32)
    return frames, rots


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _guided_stream(vislam, orc, torch, frames, rots, p, radius, stages):
    """the stream in guided launches of BN frames; every pair against the reference on the batch's own keypoints and descriptors.
    Returns per frame None (no pair) or (good matches, candidates-per-row histogram bits)"""
    c = vislam.Context(0, p)
    c.batch_plan(BW, BH, BW, BN)
    dev, d_rot = _dev(torch, frames), _dev(torch, rots)
    out, carried, first = [], None, 0
    while first < len(frames):
        c.batch_run_guided(dev.data_ptr() + first * BW * BH, BN, d_rot.data_ptr() + 36 * first, radius, stages)
        c.batch_sync()
        assert c.batch_status() == 0
        links = c.batch_get_keyframes()
        recs = [c.batch_keypoints(i) for i in range(BN)]
        for i in range(BN):
            prev = recs[links[i]] if links[i] >= 0 else (carried if links[i] == vislam.KF_CARRIED else None)
            o12, o21 = c.batch_knn(i)
            good, nsym = c.batch_matches(i)
            if prev is None:
                assert len(o12) == 0 and len(o21) == 0 and len(good) == 0 and nsym == 0, (first, i)
                out.append(None)
            else:
                (kq, dq), (kt, dt) = prev, recs[i]
                k12, k21, adm = gr.knn2(dq, np.stack([kq["x"], kq["y"]], 1), dt, np.stack([kt["x"], kt["y"]], 1), rots[first + i], radius,
                                        (p.fx, p.fy, p.cx, p.cy))
                w12, w21 = gr.dmatches(k12), gr.dmatches(k21)
                assert o12.tobytes() == w12.tobytes() and o21.tobytes() == w21.tobytes(), (first, i)
                wg, wsym = orc.good_matches(p, kq, kt, w12, w21)
                assert good.tobytes() == wg.tobytes() and nsym == len(wsym), (first, i)
                out.append((len(good), int(adm.sum()), adm.size))
            if links[i] != vislam.KF_NOT_SAVED:
                carried = recs[i]
        first += BN
    c.close()
    return out


def test_batch_gate_off(vislam, orc, stream):
    import torch
    frames, rots = stream
    out = _guided_stream(vislam, orc, torch, frames, rots, _batch_params(vislam), 12.0, vislam.STAGE_ALL)
    assert out[0] is None and all(o is not None for o in out[1:])      # frame 6 is paired with the carried frame 5
    print("good matches / admissible couples / all couples per pair:", out[1:])
    assert sum(o[0] for o in out[1:]) > 0 and all(0 < o[1] < o[2] for o in out[1:])


def test_batch_gate_refuses_a_frame(vislam, orc, stream):
    import torch
    frames, rots = stream
    frames = frames.copy()
    frames[3] = 128                                                # nothing to detect: the gate refuses it, frame 4 is paired with frame 2
    frames[6] = 128                                                # and the first frame of the second launch: frame 7 takes the carried frame 5
    out = _guided_stream(vislam, orc, torch, frames, rots, _batch_params(vislam, keyframe_min_points=10), 12.0,
                         vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert [o is None for o in out] == [i in (0, 3, 6) for i in range(2 * BN)]
    assert sum(o[0] for o in out if o) > 0


def test_a_plain_run_after_guided_ones_is_unguided(vislam, stream):
    import torch
    frames, rots = stream
    p = _batch_params(vislam)
    dev, d_rot = _dev(torch, frames), _dev(torch, rots)
    got = []
    for guided in (True, False):
        c = vislam.Context(0, p)
        c.batch_plan(BW, BH, BW, BN)
        for first in (0, BN):
            if guided:
                c.batch_run_guided(dev.data_ptr() + first * BW * BH, BN, d_rot.data_ptr() + 36 * first, 12.0)
            else:
                c.batch_run(dev.data_ptr() + first * BW * BH, BN)
            c.batch_sync()
        c.batch_run(dev.data_ptr(), BN)                            # frames 0 ... 5 again, frame 0 against the carried frame 11
        c.batch_sync()
        assert c.batch_status() == 0
        poses, goods, ngood = c.batch_results(BN)
        got.append(([tuple(x.tobytes() for x in c.batch_knn(i)) for i in range(BN)], [c.batch_matches(i)[0].tobytes() for i in range(BN)],
                    poses.tobytes(), ngood.tobytes()))
        c.close()
    assert got[0] == got[1]
