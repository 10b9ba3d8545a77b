"""GPU: the keyframe database at the ring, couple and LDS sizes tests/test_kfdb_gpu.py does not reach, against the restatement tests/kfdb_ref.py BYTE
FOR BYTE, guards included: the tie and second-neighbour ladder (every position pair across the row halves, the v_med3 pairs, the tile edge and the
tail tile), sets in which every distance ties, couples of 16384 x 40 ... 1 x 16384 and at kp_cap 4100, 2 and 1, rings of 255 ... 513 and 65536 slots,
add calls of more than 65535 rows, the candidate records and argument ends the contract defines, VIS_E_CAPACITY with a device, and (in a child
process of its own) the dynamic-LDS sizes between 48 KB and 128 KB.  tests/test_kfdb_ref.py checks every builder against the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr
from test_kfdb_gpu import FILL, INT_MAX, INT_MIN, Pair, _back, _dev, _filled, params

pytestmark = pytest.mark.gpu
F8 = kc.F8


def _fill(dt, shape):
    return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape(shape)


def emit(pr, lp, lq, kps, desc, nkp, cand, stride, max_pts, with_matches=True):
    """vis_kfdb_match_rows with the records as they lie in memory: cand is a flat record array and query i reads record i * stride (Pair.match
    cannot express stride 0 or a stride beyond the rows); everything the call writes or must leave alone against the restatement"""
    n, torch = len(nkp), pr.torch
    t = [_dev(torch, a) for a in (kps, desc, np.asarray(nkp, np.int32), cand)]
    m, p1, p2, npts = _filled(torch, n * max_pts * 16), _filled(torch, n * max_pts * 8), _filled(torch, n * max_pts * 8), _filled(torch, n * 4)
    pr.dev.match_rows(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), kps.shape[1], t[3].data_ptr(), stride, max_pts,
                      m.data_ptr() if with_matches else 0, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), lp)
    pr.c.batch_sync()
    got = (_back(m, n * max_pts * 16, kr.DMATCH_DTYPE).reshape(n, max_pts), _back(p1, n * max_pts * 8, np.float32).reshape(n, max_pts, 2),
           _back(p2, n * max_pts * 8, np.float32).reshape(n, max_pts, 2), _back(npts, n * 4, np.int32))
    want = pr.ref.match_rows(lq, kps, desc, nkp, cand[np.arange(n) * stride], max_pts, _fill(kr.DMATCH_DTYPE, (n, max_pts)),
                             _fill(np.float32, (n, max_pts, 2)), _fill(np.float32, (n, max_pts, 2)), _fill(np.int32, (n,)))
    assert got[3].tolist() == want[3].tolist(), (got[3], want[3])
    if with_matches:
        assert got[0].tobytes() == want[0].tobytes(), np.argwhere(got[0].view(np.uint8) != want[0].view(np.uint8))[:6]
    else:
        assert (got[0].view(np.uint8) == FILL).all()
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    return want


def own_cand(pr, slots):
    """the records a query would give for these slots: the id and the count each holds"""
    c = np.zeros(len(slots), kr.CAND_DTYPE)
    c["slot"], c["id"], c["n_keypoints"] = slots, pr.ref.id[slots], pr.ref.cnt[slots]
    return c


def same_ring_at(pr, slots):
    info = pr.dev.info()
    assert (info.entry_cap, info.kp_cap, info.head, info.total_added) == (pr.entry_cap, pr.kp_cap, pr.ref.head, pr.ref.total)
    for s in slots:
        i, n, xy = pr.dev.get_entry(int(s))
        ri, rn, rxy = pr.ref.get_entry(int(s))
        assert (i, n) == (ri, rn) and xy.tobytes() == rxy.tobytes(), (s, i, n, ri, rn)


def oracle_keys_of(orc):
    def keys(e, q):
        o12, o21 = orc.knn2_hamming(e, q)
        return kr.keys_from_dmatch(o12), kr.keys_from_dmatch(o21)
    return keys


# ---- A. the tie and second-neighbour ladder --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted_is_entry", [True, False], ids=["planted_entry", "planted_query"])
@pytest.mark.parametrize("ns", kc.LADDER_NS)
def test_tie_and_second_neighbour_ladder(vislam, ctx, ns, planted_is_entry):
    """one couple per query through vis_kfdb_match_rows: query i points at slot i with the id the slot holds (cand_stride 1), so every couple's whole
    match list is compared.  The tie (ratio 1.0) must name the lower row; 32 bits against 39 (ratio 0.8f) must DROP the planted row -- a kernel that
    lost the second neighbour would keep it; 32 against 40 keeps it."""
    cs = kc.ladder(ns)
    rng = np.random.default_rng(ns)
    sets = [kc.ladder_sets(c, planted_is_entry) for c in cs]
    pr = Pair(vislam, ctx, len(cs), kc.LADDER_ROW_CAP)
    kps, desc, nkp = kc.rows(rng, [e for e, _ in sets], kc.LADDER_ROW_CAP)
    pr.add(kps, desc, nkp, np.arange(len(cs)))
    qk, qd, qn = kc.rows(rng, [q for _, q in sets], kc.LADDER_ROW_CAP)
    cand = own_cand(pr, np.arange(len(cs)))
    seen = 0
    for ratio in (1.0, F8):                                         # the ratio is the call's: the couples of the other ratio ride along
        lp, lq = params(vislam, ratio=ratio)
        m, _, _, npts = emit(pr, lp, lq, qk, qd, qn, cand, 1, kc.LADDER_ROW_CAP)
        for i, c in enumerate(cs):
            if c["ratio"] == ratio:
                assert kc.ladder_match_of_f(c, planted_is_entry, m[i, :npts[i]]) == c["expect"], (c["kind"], c["a"], c["b"])
                seen += 1
        assert ratio != 1.0 or (npts > 0).all()                     # (at 1.0 every row with two neighbours passes the ratio test)
    assert seen == len(cs)
    pr.close()


@pytest.mark.parametrize("sym_mode", [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED])
@pytest.mark.parametrize("ratio", [F8, 1.0])
def test_sets_in_which_every_distance_ties(vislam, ctx, ratio, sym_mode):
    """n copies of one row against m copies of it (every distance 0) and all-zero against all-ones (every distance 256), n and m in 2, 33, 64, 257:
    the score row of all 8 x 8 couples and the list of every couple"""
    entries, queries = kc.all_equal_sets()
    rng = np.random.default_rng(8)
    pr = Pair(vislam, ctx, 8, 260)
    kps, desc, nkp = kc.rows(rng, entries, 260)
    pr.add(kps, desc, nkp, np.arange(8))
    qk, qd, qn = kc.rows(rng, queries, 260)
    lp, lq = params(vislam, ratio=ratio, sym_mode=sym_mode, min_gap=0, min_score=0, topk=8)
    scores, _, _ = pr.query(lp, lq, qd, qn, np.full(8, 50))
    assert (scores[:4, :4] == 1).all() and (scores[4:, 4:] == (1 if ratio == 1.0 else 0)).all()
    for s in range(8):
        emit(pr, lp, lq, qk, qd, qn, own_cand(pr, np.full(8, s)), 1, 4)
    pr.close()


# ---- B. couples at the sizes between ---------------------------------------------------------------------------------------------------------
def _planted_couple(seed, n_e, n_q, zeros=False):
    """random sets with hamming_ref.plant's ties and extremes and true correspondences a few bits apart on the rows plant() leaves alone"""
    import hamming_ref as hr
    rng = np.random.default_rng(seed)
    E = rng.integers(0, 256, (n_e, 32), dtype=np.uint8)
    Q = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    if zeros:                                                       # the matcher's limit case: the short set all zero, two all-ones rows in the long one
        Q[:] = 0
        E[[77, n_e - 5]] = 255
        return E, Q
    if min(n_e, n_q) < 9:
        return E, Q
    hr.plant(E, Q)
    small, big = min(n_e, n_q), max(n_e, n_q)
    for j in range(8, small - 1):
        i = 8 + (j * 409) % (big - 9)                              # (409 is prime: distinct rows of the long side for the rows of the short one)
        e, q = (i, j) if n_e >= n_q else (j, i)
        if j % 3 or small < 100:
            Q[q] = kc.flip(E[e], rng.choice(256, int(rng.integers(0, 12)), replace=False))
    return E, Q


def _couple_calls(vislam, pr, rng, Q_sets, row_cap, want_above=None):
    qk, qd, qn = kc.rows(rng, Q_sets, row_cap)
    lp, lq = params(vislam, min_gap=0, min_score=0, topk=1)
    scores, cand, _ = pr.query(lp, lq, qd, qn, np.full(len(Q_sets), 9))
    if want_above is not None:
        assert (scores > want_above).all(), scores
    cd = np.zeros(cand.shape, kr.CAND_DTYPE)
    cd[:] = cand
    for max_pts in (int(cand["score"][0, 0]), 7):
        want = emit(pr, lp, lq, qk, qd, qn, cd.reshape(-1), 1, max_pts)
    return scores, want


@pytest.mark.parametrize("n_e,n_q,zeros", [(16384, 40, False), (40, 16384, False), (16384, 1, False), (1, 16384, False), (16384, 33, True)],
                         ids=["16384x40", "40x16384", "16384x1", "1x16384", "16384x33_zero"])
def test_tall_and_short_couples_at_kp_cap_16384(vislam, orc, ctx, n_e, n_q, zeros):
    """the shapes of the matcher's limit tests (tests/test_limits_gpu.py protects k_knn_mfma, not the copy of its chain in loop_sweep): 512 tiles
    against 2, one row against 16384, and an all-zero short set against a long one with two all-ones rows.  The keys are the CPU oracle's."""
    E, Q = _planted_couple(1000 + n_e + n_q, n_e, n_q, zeros)
    rng = np.random.default_rng(4)
    pr = Pair(vislam, ctx, 1, 16384, oracle_keys_of(orc))
    kps, desc, nkp = kc.rows(rng, [E], 16384)
    pr.add(kps, desc, nkp, [0])
    degenerate = zeros or min(n_e, n_q) == 1
    scores, want = _couple_calls(vislam, pr, rng, [Q], 16384, None if degenerate else 20)
    print(f"score at {n_e} x {n_q}{' (all zero)' if zeros else ''}:", int(scores[0, 0]))
    if min(n_e, n_q) == 1:                                          # fewer than two neighbours in one direction: nothing passes the ratio test
        assert scores[0, 0] == 0 and want[3].tolist() == [0] and (want[0].view(np.uint8) == FILL).all() and (want[1].view(np.uint8) == FILL).all()
    pr.close()


def test_couples_at_kp_cap_4100(vislam, orc, ctx):
    """4097 x 2049 and 1000 x 777 (and the two couples across): 17 chunks of 256 fixed rows, the last of ONE row, 129 and 65 tiles with a tail of 1"""
    rng = np.random.default_rng(41)
    pr = Pair(vislam, ctx, 2, 4100, oracle_keys_of(orc))
    E0, Q0 = _planted_couple(4097, 4097, 2049)
    E1, Q1 = _planted_couple(1000, 1000, 777)
    Q0[1500:2000], Q1[300:700] = E1[:500], E0[:400]                  # (so that the couples across score too)
    kps, desc, nkp = kc.rows(rng, [E0, E1], 4100)
    pr.add(kps, desc, nkp, [0, 1])
    scores, _ = _couple_calls(vislam, pr, rng, [Q0, Q1], 4100, 20)
    print("scores at kp_cap 4100 (4097 | 1000 entries x 2049 | 777 queries):", scores.tolist())
    pr.close()


@pytest.mark.parametrize("kp_cap", [1, 2])
def test_kp_cap_1_and_2(vislam, ctx, kp_cap):
    """kp_cap 1: every couple has fewer than two neighbours, every score is 0; kp_cap 2: two copies score 2.  row_cap above and at kp_cap"""
    E, Q, _ = kc.planted_sets(5, 40, 40)
    rng = np.random.default_rng(kp_cap)
    for row_cap in (kp_cap, 5):
        pr = Pair(vislam, ctx, 3, kp_cap)
        kps, desc, nkp = kc.rows(rng, [E[:2], E[2:3], E[4:9]], row_cap)
        pr.add(kps, desc, nkp, [0, 1, 2])
        pr.same_ring()
        lp, lq = params(vislam, min_gap=0, min_score=0, topk=3)
        qk, qd, qn = kc.rows(rng, [E[:2], E[4:6], Q[:5]], row_cap)
        scores, _, _ = pr.query(lp, lq, qd, qn, [7, 7, 7])
        assert (scores >= 0).all() and scores[0, 0] == scores[1, 2] == (0 if kp_cap == 1 else 2) and (kp_cap == 2 or (scores == 0).all())
        for s in range(3):
            emit(pr, lp, lq, qk, qd, qn, own_cand(pr, np.full(3, s)), 1, 2)
        pr.close()


# ---- C. large rings and long adds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry_cap", kc.RING_CAPS)
def test_rings_around_256_slots(vislam, ctx, entry_cap):
    """k_loop_topk's 256-strided loops with a second and third turn, its reduction trees with every thread live, equal (score, id) in one thread,
    in neighbouring threads and 255 apart, 15 / 16 / 17 entries at or above min_score with topk 16, min_score at both ends of int32; the deal of
    k_loop_score over the XCDs at 32 and 65 slots an XCD"""
    pr = Pair(vislam, ctx, entry_cap, 32)
    kps, desc, nkp, ids = kc.ring_table(entry_cap)
    pr.add(kps, desc, nkp, ids)
    pr.same_ring()
    qk, qd, qn, qi = kc.ring_queries(entry_cap)
    for ms in (6, 5, 4, INT_MIN, INT_MAX):
        lp, lq = params(vislam, min_gap=0, topk=16, min_score=ms)
        scores, cand, query = pr.query(lp, lq, qd, qn, qi)
        assert query["n_cand"].tolist()[:2] == [min(kc.RING_MIN_SCORES.get(ms, 0 if ms > 0 else 16), 16), 0]
    lp, lq = params(vislam, min_gap=0, topk=3, min_score=1)
    pr.query(lp, lq, qd, qn, qi, with_scores=False)
    pr.add(kps[:5], desc[:5], nkp[:5], 3000 + np.arange(5))         # the head was back at 0: five slots turn over
    lp, lq = params(vislam, min_gap=10, topk=16, min_score=5)
    pr.query(lp, lq, qd, qn, qi)
    pr.close()


def test_ring_of_65536_slots_and_an_add_of_70000_rows(vislam, ctx):
    """entry_cap at its limit, kp_cap 8.  One add call of 70000 rows -- more than 65535, so blockIdx.x carries them, and the first 4464 are skipped
    because later rows of the call take their slots --, then one of 3.  The ring at the head, the 64 slots on either side of it and every 257th slot;
    a 3-query call in which a few hundred entries are eligible."""
    E = 65536
    pr = Pair(vislam, ctx, E, 8)
    kps, desc, nkp, ids = kc.scored_rows(70003, 8)
    pr.add(kps[:70000], desc[:70000], nkp[:70000], ids[:70000])
    pr.add(kps[70000:], desc[70000:], nkp[70000:], ids[70000:])
    head = pr.ref.head
    assert head == 70003 - E and pr.ref.total == 70003
    same_ring_at(pr, sorted({(head + d) % E for d in range(-64, 65)} | set(range(0, E, 257)) | {E - 1}))
    qk, qd, qn = kc.query_base(3)
    qk, qd, qn = qk[:, :8], np.ascontiguousarray(qd[:, :8]), np.array([8, 8, 8], np.int32)
    oldest = int(pr.ref.id[head]) if pr.ref.id[head] >= 0 else int(pr.ref.id[(head + 1) % E])
    lp, lq = params(vislam, min_gap=100, topk=16, min_score=3)
    _, cand, query = pr.query(lp, lq, qd, qn, [oldest + 100 + 400, -1, oldest + 100 + 550])
    print("ring of 65536: eligible", query["n_scored"].tolist(), "best", query["best_score"].tolist(), "top", cand["score"][0].tolist())
    assert 250 <= query["n_scored"][0] <= 550 and 250 <= query["n_scored"][2] <= 550 and query["flags"].tolist() == [0, 1, 0]
    assert query["best_score"][0] >= 6 and query["n_cand"][0] == 16
    pr.close()


def test_small_ring_lapped_thousands_of_times_by_one_add(vislam, ctx):
    """entry_cap 7, row_cap 4, one add call of 65536 + 7 * 3 + 2 rows: all but the last 7 are skipped"""
    n = 65536 + 7 * 3 + 2
    pr = Pair(vislam, ctx, 7, 8)
    kps, desc, nkp, ids = kc.scored_rows(n, 4)
    pr.add(kps[:3], desc[:3], nkp[:3], ids[:3])                      # (so that the long add starts off slot 0)
    pr.add(kps, desc, nkp, ids)
    pr.same_ring()
    assert (pr.ref.head, pr.ref.total) == ((3 + n) % 7, n + 3) and sorted(pr.ref.id.tolist()) == sorted(ids[n - 7:].tolist())
    qk, qd, qn = kc.query_base(2)
    lp, lq = params(vislam, min_gap=0, topk=7, min_score=0)
    scores, _, _ = pr.query(lp, lq, np.ascontiguousarray(qd[:, :4]), np.array([4, 4], np.int32), [n, n + 1])
    assert (scores >= 0).sum() >= 6 and scores.max() >= 2
    pr.close()


def test_capacity_refusal_with_a_device(vislam, ctx):
    """n x entry_cap = 4097 x 65536 is 65536 couples above 2^28: VIS_E_CAPACITY, nothing written (the score buffer is there in full, so even an
    accepted call would stay inside it), and the database answers an ordinary query afterwards.  The accepted end (n = 4096) is a gigabyte of
    scores and 2^28 workgroups: not run."""
    import torch
    E, n = 65536, 4097
    pr = Pair(vislam, ctx, E, 8)
    kps, desc, nkp, ids = kc.scored_rows(40, 8)
    pr.add(kps, desc, nkp, ids)
    qd = np.repeat(kc.BASE[None, :8], n, 0)
    t = [_dev(torch, a) for a in (qd, np.full(n, 8, np.int32), np.full(n, 1000, np.int32))]
    lp, lq = params(vislam, min_gap=0, topk=16, min_score=0)
    sc, ca, qu = _filled(torch, n * E * 4), _filled(torch, n * 16 * 16), _filled(torch, n * 32)
    for scores_ptr in (sc.data_ptr(), 0):
        with pytest.raises(vislam.VisError) as e:
            pr.dev.query_rows(n, t[0].data_ptr(), t[1].data_ptr(), 8, t[2].data_ptr(), scores_ptr, ca.data_ptr(), qu.data_ptr(), lp)
        assert e.value.code == -4 and "2^28" in str(e.value)
    ctx.batch_sync()
    assert all(bool((b == FILL).all().item()) for b in (sc, ca, qu))
    del sc
    scores, _, _ = pr.query(lp, lq, qd[:2], [8, 8], [1000, 1001])
    assert (scores >= 0).sum() >= 2 * 20 and scores.max() == 8
    pr.close()


# ---- D. candidate records and argument ends --------------------------------------------------------------------------------------------------
@pytest.fixture()
def four(vislam, ctx):
    """a ring of 5 slots: 4 entries of about 100 keypoints, slot 2 added empty, slot 4 never written (id -1); 3 different queries: query 0 holds noisy copies of rows of entries 0 and 1, query 1 of entries
    1 and 0, query 2 of entries 3 and 1"""
    rng = np.random.default_rng(21)
    E = rng.integers(0, 256, (300, 32), dtype=np.uint8)

    def noisy(rows_):
        q = rng.integers(0, 256, (len(rows_), 32), dtype=np.uint8)
        for i, r in enumerate(rng.permutation(rows_)):
            if i % 3:
                q[i] = kc.flip(E[r], rng.choice(256, int(rng.integers(0, 10)), replace=False))
        return q
    pr = Pair(vislam, ctx, 5, 160)
    kps, desc, nkp = kc.rows(rng, [E[:100], E[50:147], E[:0], E[200:300]], 152)
    pr.add(kps, desc, nkp, [10, 11, 12, 13])
    yield pr, kc.rows(rng, [noisy(np.arange(100)), noisy(np.arange(40, 150)), noisy(np.r_[110:147, 200:300])], 152), rng
    pr.close()


def test_candidate_records_the_contract_refuses_or_reads(vislam, four):
    pr, (qk, qd, qn), _ = four
    lp, lq = params(vislam, min_gap=0, min_score=0, topk=4)
    rec = lambda i, s: np.array([(i, s, 0, 0)], kr.CAND_DTYPE)
    for slot in (5, 6, INT_MAX, INT_MIN, -2, -1):                    # no such slot: d_npts 0, the rows untouched
        for i in (10, -1):
            want = emit(pr, lp, lq, qk, qd, qn, np.concatenate([rec(i, slot), rec(10, 0), rec(i, slot)]), 1, 152)
            assert want[3][0] == want[3][2] == 0 and want[3][1] > 20
    for d_id, live in ((0, True), (1, False), (-1, False)):            # a live slot with its id, one above, one below
        want = emit(pr, lp, lq, qk, qd, qn, np.concatenate([rec(10 + d_id, 0), rec(11 + d_id, 1), rec(13 + d_id, 3)]), 1, 152)
        assert ((want[3] > 20) == live).all() and (live or (want[3] == 0).all()), want[3]
    for i, slot in ((12, 2), (-1, 2), (-1, 4), (0, 4)):               # an empty slot, with the id it holds too: the one added empty, the one never written
        assert emit(pr, lp, lq, qk, qd, qn, np.concatenate([rec(i, slot)] * 3), 1, 152)[3].tolist() == [0, 0, 0]
    assert pr.ref.get_entry(4)[:2] == (-1, 0) and pr.ref.get_entry(2)[:2] == (12, 0)
    # cand_stride 0: every query reads record 0; the records behind it are never looked at
    want = emit(pr, lp, lq, qk, qd, qn, np.concatenate([rec(11, 1), rec(-7, INT_MAX), rec(-7, INT_MIN)]), 0, 152)
    assert (want[3] > 10).all() and len(set(want[3].tolist())) == 3
    # cand_stride 5 over the 4 records of a query and one record of padding
    _, cand, _ = pr.query(lp, lq, qd, qn, [20, 21, 22])
    padded = np.zeros((3, 5), kr.CAND_DTYPE)
    padded[:, :4], padded[:, 4] = cand, rec(-9, INT_MIN)[0]
    for rank in range(4):
        want = emit(pr, lp, lq, qk, qd, qn, padded.reshape(-1)[rank:], 5, 152)
        assert (want[3] == np.where(cand["slot"][:, rank] >= 0, cand["score"][:, rank], 0)).all()    # the list is as long as the score said


def test_max_pts_0(vislam, four):
    """d_npts is the full count and nothing else is written, with d_matches and without"""
    pr, (qk, qd, qn), _ = four
    lp, lq = params(vislam, min_gap=0, min_score=0)
    for with_matches in (True, False):
        want = emit(pr, lp, lq, qk, qd, qn, own_cand(pr, np.array([0, 1, 3])), 1, 0, with_matches)
        assert (want[3] > 20).all()


def test_row_cap_0(vislam, four):
    """rows without room for a keypoint: an add makes empty entries and moves the head, a query is skipped, a match gives d_npts 0"""
    pr, (qk, qd, qn), _ = four
    lp, lq = params(vislam, min_gap=0, min_score=0)
    cand = own_cand(pr, np.array([0, 1, 3]))
    _, _, query = pr.query(lp, lq, qd[:, :0], qn, [20, 21, 22])
    assert query["flags"].tolist() == [1, 1, 1]
    assert emit(pr, lp, lq, qk[:, :0], qd[:, :0], qn, cand, 1, 8)[3].tolist() == [0, 0, 0]
    pr.add(qk[:2, :0], qd[:2, :0], qn[:2], [14, 15])
    pr.same_ring()
    assert pr.ref.head == 1 and pr.ref.cnt.tolist() == [0, 97, 0, 100, 0] and pr.ref.id.tolist() == [15, 11, 12, 13, 14]
    scores, _, _ = pr.query(lp, lq, qd, qn, [20, 21, 22])
    assert (scores[:, [0, 2, 4]] == -1).all() and (scores[:, [1, 3]] >= 0).all()


def test_n_0(vislam, four):
    """calls without rows: nothing is written, head and total stay"""
    import torch
    pr, (qk, qd, qn), _ = four
    lp, lq = params(vislam, min_gap=0, min_score=0)
    pr.add(qk[:0], qd[:0], qn[:0], np.zeros(0, np.int32))
    pr.same_ring()
    assert (pr.ref.head, pr.ref.total) == (4, 4)
    t = [_dev(torch, a) for a in (qk, qd, qn, np.array([20, 21, 22], np.int32), own_cand(pr, np.array([0, 1, 3])))]
    out = [_filled(torch, 64) for _ in range(7)]
    pr.dev.query_rows(0, t[1].data_ptr(), t[2].data_ptr(), 152, t[3].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), lp)
    pr.dev.query_rows(0, t[1].data_ptr(), t[2].data_ptr(), 152, t[3].data_ptr(), 0, out[1].data_ptr(), out[2].data_ptr(), lp)
    pr.dev.match_rows(0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 152, t[4].data_ptr(), 1, 4, out[3].data_ptr(), out[4].data_ptr(), out[5].data_ptr(),
                      out[6].data_ptr(), lp)
    pr.c.batch_sync()
    for o in out:
        _back(o, 0, np.uint8)
    pr.same_ring()
    pr.query(lp, lq, qd, qn, [20, 21, 22])


@pytest.mark.parametrize("sym_mode", [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED])
def test_ratios_at_the_ends(vislam, ctx, sym_mode):
    """1.0, 2.0, +inf (inf * 0 is a NaN: the comparison is false, the match stays), -1.0 and the smallest float32 denormal, taken as written"""
    E, Q, _ = kc.planted_sets(1234, 300, 257)
    rng = np.random.default_rng(9)
    pr = Pair(vislam, ctx, 2, 320)
    kps, desc, nkp = kc.rows(rng, [E, E[:129]], 320)
    pr.add(kps, desc, nkp, [0, 1])
    qk, qd, qn = kc.rows(rng, [Q, Q[:65]], 320)
    seen = []
    for ratio in kc.RATIO_ENDS:
        lp, lq = params(vislam, ratio=ratio, sym_mode=sym_mode, min_gap=0, min_score=0)
        scores, _, _ = pr.query(lp, lq, qd, qn, [5, 6])
        emit(pr, lp, lq, qk, qd, qn, own_cand(pr, np.array([0, 1])), 1, 320)
        seen.append(int(scores[0, 0]))
    print("scores at the ratio ends", kc.RATIO_ENDS, seen)
    assert len(set(seen)) >= 2
    pr.close()


# ---- E. the LDS sizes between 48 KB and 128 KB, in a process that has not raised the limit yet -----------------------------------------------
def test_lds_ladder_in_a_fresh_process():
    """tests/kfdb_lds_ladder.py once, as a child: hipFuncAttributeMaxDynamicSharedMemorySize is process-wide, so a pytest process that has run a
    16384-keypoint database cannot tell whether a launch at 48 ... 96 KB is accepted on its own"""
    import kfdb_lds_ladder as ladder
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kfdb_lds_ladder.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, script], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("lds ladder:")]
    assert len(lines) == len(ladder.LADDER) == 7 and all(l.endswith(" ok") for l in lines), lines
    for (kp_cap, row_cap), l in zip(ladder.LADDER, lines):
        assert f" {kp_cap} + {row_cap} " in l, (kp_cap, row_cap, l)
