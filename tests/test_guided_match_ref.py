"""CPU: tests/guided_match_ref.py against tests/hamming_ref.py and against itself, and the preconditions of every fixture that
tests/test_guided_match_gpu.py runs on the device (planted ties, points exactly on and just beyond the window's edge, rows with exactly one
and exactly two candidates, masked winners, NaN predictions, the long sweep's first and last tile)."""
import numpy as np

import guided_match_ref as gr
import hamming_ref as hr

F32 = np.float32


def _as_idx_dist(keys):
    none = keys == gr.NONE
    idx = np.where(none, -1, (keys & np.uint32(0xFFFF)).astype(np.int32)).astype(np.int32)
    dist = np.where(none, np.inf, (keys >> np.uint32(16)).astype(F32)).astype(F32)
    return idx, dist


def test_identity_and_a_huge_window_give_the_unguided_2nn():
    for n_prev, n_cur in ((1, 1), (1, 9), (2, 1), (33, 65), (257, 300)):
        d1, xy1, d2, xy2 = gr.sized_case(n_prev, n_cur)
        k12, k21, adm = gr.knn2(d1, xy1, d2, xy2, np.eye(3, dtype=F32), 1e30)
        assert adm.all()
        (i12, s12), (i21, s21) = hr.knn2_both(d1, d2)
        for keys, idx, dist in ((k12, i12, s12), (k21, i21, s21)):
            gi, gd = _as_idx_dist(keys)
            assert (gi == idx).all() and (gd[idx >= 0] == dist[idx >= 0]).all(), (n_prev, n_cur)


def test_distances_agree_with_the_other_reference():
    d1, _, d2, _ = gr.sized_case(65, 33)
    assert (gr.hamming(d1, d2) == hr.distances(d1, d2).astype(np.int64)).all()
    assert gr.hamming(np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8))[0, 0] == 256


def test_admissibility_is_symmetric():
    d1, xy1, d2, xy2, _ = gr.semantics_case()
    pred = gr.warp(xy2, gr.SMALL_ROT)
    adm = gr.admissible(xy1, pred, gr.RADIUS)
    # the other direction evaluated with the roles of the operands exchanged: |a - b| and |b - a| are the same float
    with np.errstate(invalid="ignore"):
        other = (np.abs(xy1[None, :, 0] - pred[:, None, 0]) <= F32(gr.RADIUS)) & (np.abs(xy1[None, :, 1] - pred[:, None, 1]) <= F32(gr.RADIUS))
    assert (adm == other.T).all()
    k12, k21, _ = gr.knn2(d1, xy1, d2, xy2, gr.SMALL_ROT, gr.RADIUS)
    # whoever appears in a list is admissible, and a row's list is empty exactly when it has no candidate
    for keys, a in ((k12, adm), (k21, adm.T)):
        idx, _ = _as_idx_dist(keys)
        for q in range(len(idx)):
            assert all(a[q, t] for t in idx[q] if t >= 0)
            assert (idx[q] >= 0).sum() == min(2, int(a[q].sum()))


def test_float_warp_against_double():
    rng = np.random.default_rng(8)
    pts = gr.warp_points()
    assert len(pts) == 257 and (pts >= 0).all() and (pts[:, 0] < 752).all() and (pts[:, 1] < 480).all()
    worst = 0.0
    for _ in range(40):
        w = rng.normal(0, 1, 3)
        w *= np.deg2rad(rng.uniform(0, 10)) / np.linalg.norm(w)
        rot = gr.rodrigues(w).astype(F32)
        a, b = gr.warp(pts, rot), gr.warp_f64(pts, rot)
        assert not np.isnan(a).any()
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    print(f"float32 warp against float64, rotations <= 10 degrees: worst difference {worst:.3e} px")
    assert worst <= 1e-3


def test_warp_fixture_has_points_behind_the_camera():
    pts = gr.warp_points()
    assert np.array_equal(gr.warp(pts, gr.WARP_ROTS[0]).shape, (257, 2))
    for rot in gr.WARP_ROTS[:2]:
        assert not np.isnan(gr.warp(pts, rot)).any()
    nan = np.isnan(gr.warp(pts, gr.WARP_ROTS[2]))
    assert (nan[:, 0] == nan[:, 1]).all() and 20 < nan[:, 0].sum() < 237          # some, not all


def _has_tie(dist, adm):
    """a row whose two best admissible candidates are equally far (the lower index must come first)"""
    for q in range(len(dist)):
        c = np.sort(dist[q][adm[q]])
        if len(c) >= 2 and c[0] == c[1]:
            return True
    return False


def test_semantics_fixture_preconditions():
    d1, xy1, d2, xy2, rows = gr.semantics_case()
    pred = gr.warp(xy2, gr.SMALL_ROT)
    adm = gr.admissible(xy1, pred, gr.RADIUS)
    dist = gr.hamming(d1, d2)
    r = F32(gr.RADIUS)
    # candidate counts: 0, 1, 2 and more, in both directions
    for a in (adm, adm.T):
        counts = a.sum(1)
        assert (counts == 0).any() and (counts == 1).any() and (counts == 2).any() and (counts >= 3).any(), np.bincount(counts)
    assert _has_tie(dist, adm) and _has_tie(dist.T, adm.T)
    (a, b), t = rows["tie_prev_pair"], rows["tie_cur"]
    assert a < b and dist[a, t] == dist[b, t] == 3 and np.flatnonzero(adm[:, t]).tolist() == [a, b]
    (a, b), t = rows["tie_cur_pair"], rows["tie_prev"]
    assert a < b and dist[t, a] == dist[t, b] == 3 and np.flatnonzero(adm[t]).tolist() == [a, b]
    # the edge: exactly radius and the next float beyond it
    e, at, beyond = rows["cur_edge"], rows["prev_at"], rows["prev_beyond"]
    assert 8.0 <= pred[e, 0] < 16.0
    assert pred[e, 0] - xy1[at, 0] == r and pred[e, 1] - xy1[at, 1] == 0
    assert pred[e, 0] - xy1[beyond, 0] == np.nextafter(r, F32(np.inf)) and pred[e, 1] - xy1[beyond, 1] == 0
    assert adm[at, e] and not adm[beyond, e]
    assert adm[:, e].sum() == 1 and adm[at].sum() == 1 and adm[beyond].sum() == 0
    assert dist[beyond, e] == 0 and dist[at, e] == 9
    # masked winners: the far row has the smaller distance AND the lower index
    v, ok, far = rows["cur_victim"], rows["prev_ok"], rows["prev_far"]
    assert far == 0 < ok and dist[far, v] == 0 < dist[ok, v] == 5 and not adm[far, v] and adm[ok, v] and adm[:, v].sum() == 1
    assert adm[far].sum() == 0
    v, ok, far = rows["prev_victim"], rows["cur_ok"], rows["cur_far"]
    assert far == 0 < ok and dist[v, far] == 0 < dist[v, ok] == 5 and not adm[v, far] and adm[v, ok] and adm[v].sum() == 1
    assert adm[:, far].sum() == 0
    k12, k21, _ = gr.knn2(d1, xy1, d2, xy2, gr.SMALL_ROT, gr.RADIUS)
    assert k21[e].tolist() == [(9 << 16) | at, 0xFFFFFFFF] and k12[beyond].tolist() == [0xFFFFFFFF] * 2


def test_nan_fixture_preconditions():
    d1, xy1, d2, xy2 = gr.nan_case()
    pred = gr.warp(xy2, gr.NAN_ROT)
    nan = np.isnan(pred[:, 0])
    assert 5 < nan.sum() < 43
    adm = gr.admissible(xy1, pred, gr.RADIUS)
    assert not adm[:, nan].any() and adm[:, ~nan].any(0).all()       # every other current row has a candidate
    k12, k21, _ = gr.knn2(d1, xy1, d2, xy2, gr.NAN_ROT, gr.RADIUS)
    assert (k21[nan] == gr.NONE).all() and not np.isin(k12[k12 != gr.NONE] & 0xFFFF, np.flatnonzero(nan)).any()


def test_long_sweep_fixture_preconditions():
    d1, xy1, d2, xy2 = gr.long_sweep_case()
    assert len(d1) == 40 and len(d2) == 16384
    k12, k21, adm = gr.knn2(d1, xy1, d2, xy2, gr.SMALL_ROT, gr.RADIUS)
    cols = np.flatnonzero(adm.any(0))
    assert ((cols < 32) | (cols >= 16384 - 32)).all() and (cols < 32).any() and (cols >= 16384 - 32).any()
    idx, _ = _as_idx_dist(k12)
    first = (idx[:, 0] >= 0) & (idx[:, 0] < 32)
    assert first.any() and (idx[:, 0] >= 16384 - 32).any()           # best neighbours in the first tile (aged 511 times) and in the last
    assert (first & (idx[:, 1] >= 0) & (idx[:, 1] < 32)).any()       # a row whose two neighbours both come from the first tile
    assert (idx[:, 1] < 0).any()                                     # and rows with fewer than two candidates
    assert (k21[32:16384 - 32] == gr.NONE).all()


def test_sized_fixtures_have_empty_single_and_full_rows():
    seen12, seen21, ties = set(), set(), 0
    for n_prev in gr.PREV_SIZES:
        for n_cur in gr.CUR_SIZES:
            d1, xy1, d2, xy2 = gr.sized_case(n_prev, n_cur)
            assert len(d1) == len(xy1) == n_prev and len(d2) == len(xy2) == n_cur
            adm = gr.admissible(xy1, gr.warp(xy2, gr.SMALL_ROT), gr.RADIUS)
            seen12 |= set(np.minimum(adm.sum(1), 3).tolist())
            seen21 |= set(np.minimum(adm.sum(0), 3).tolist())
            ties += _has_tie(gr.hamming(d1, d2), adm)
    assert seen12 == seen21 == {0, 1, 2, 3} and ties > 20
    for nq in gr.POP_QUERIES:
        for ns in gr.POP_SWEPT:
            d1, xy1, d2, xy2 = gr.sized_case(nq, ns, seed=7000 + 100 * nq + ns)
            assert gr.admissible(xy1, gr.warp(xy2, gr.SMALL_ROT), gr.RADIUS).any()
