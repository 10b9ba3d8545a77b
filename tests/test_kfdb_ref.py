"""CPU: the restatement of the loop-candidate contract (tests/kfdb_ref.py) against the CPU oracle -- the score and the match list of a couple are
what orc.knn2_hamming + orc.good_matches(...)[1] give, existing and independent code --, place recognition on a planted out-and-back path with the
oracle alone, and the ring / eligibility / top-k / emission bookkeeping on hand-made tables."""
import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr

F8 = float(np.float32(0.8))


def oracle_list(orc, p, E, Q):
    """the symmetric list of the pair (E first, Q second) by the oracle; the keypoints do not enter it"""
    o12, o21 = orc.knn2_hamming(E, Q)
    rng = np.random.default_rng(0)
    return orc.good_matches(p, kc.keypoints(rng, len(E)), kc.keypoints(rng, len(Q)), o12, o21)[1]


def oracle_params(vislam, ratio, sym_mode):
    p = vislam.default_params()
    p.ratio, p.sym_mode = ratio, sym_mode
    return p


@pytest.mark.parametrize("sym_mode", [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED])
@pytest.mark.parametrize("ratio", [F8, 0.5, 0.75])
def test_restatement_equals_the_oracle(vislam, orc, ratio, sym_mode):
    p, lp = oracle_params(vislam, ratio, sym_mode), kr.Params(ratio=ratio, sym_mode=sym_mode)
    seen = 0
    for a, n_e in enumerate(kc.REF_COUNTS):
        for n_q in (kc.REF_COUNTS if ratio == F8 else (n_e, 300)):
            E, Q, plants = kc.planted_sets(1000 * a + n_q, n_e, n_q, ratio)
            got, want = kr.couple_list(E, Q, lp, slot=-1), oracle_list(orc, p, E, Q)
            assert got.tobytes() == want.tobytes(), (n_e, n_q, len(got), len(want))
            # the oracle's 2-NN lists and the restatement's keys are the same thing
            o12, o21 = orc.knn2_hamming(E, Q)
            k12, k21 = kr.couple_keys(E, Q)
            assert (kr.keys_from_dmatch(o12) == k12).all() and (kr.keys_from_dmatch(o21) == k21).all(), (n_e, n_q)
            if plants:
                q_of = dict(zip(got["queryIdx"].tolist(), got["trainIdx"].tolist()))
                d_of = dict(zip(got["queryIdx"].tolist(), got["distance"].tolist()))
                d1, on = kc.BOUNDARIES[ratio]
                assert plants["on"] in q_of and d_of[plants["on"]] == on and plants["below"] in q_of and plants["above"] not in q_of, (n_e, n_q)
                assert (plants["one_sided"] in q_of) == (sym_mode == kr.SYM_REFERENCE_EFFECTIVE), (n_e, n_q)
                e, q = plants["dup_query"]                                            # the tie goes to the lower row; a duplicate fails the ratio test
                assert int(k12[e, 0] & 0xFFFF) == q and int(k12[e, 1] & 0xFFFF) > q and k12[e, 0] >> 16 == k12[e, 1] >> 16 == 3 and e not in q_of
                e0, e1, q = plants["dup_entry"]
                assert [int(k21[q, j] & 0xFFFF) for j in (0, 1)] == [e0, e1] and e1 not in q_of
                assert (q_of.get(e0) == q) == (sym_mode == kr.SYM_REFERENCE_EFFECTIVE)
                e, q = plants["copy"]
                assert q_of[e] == q and d_of[e] == 0.0
                e, q = plants["complement"]
                assert int(kr.hamming(E[e:e + 1], Q[q:q + 1])[0, 0]) == 256 and q_of.get(e) != q
                seen += 1
    assert seen >= 9
    one = kr.couple_list(E[:1], Q[:1], lp)
    assert len(one) == 0 and len(oracle_list(orc, p, E[:1], Q[:1])) == 0            # fewer than two neighbours fail the ratio test


@pytest.fixture(scope="module")
def path(vislam, orc):
    """descriptors of the planted path by the oracle's detector, and the oracle's score of every (entry, query) couple"""
    p = kc.path_params(vislam.default_params())
    out, back, other = kc.path_frames(vislam.synth_canvas(1024))
    det = lambda f: orc.orb_detect_compute(p, f)
    E, Qb, Qo = [det(f) for f in out], [det(f) for f in back], [det(f) for f in other]

    def score(e, q):
        o12, o21 = orc.knn2_hamming(e[1], q[1])
        return len(orc.good_matches(p, e[0], q[0], o12, o21)[1])
    return dict(p=p, E=E, Qb=Qb, Qo=Qo, back=np.array([[score(e, q) for e in E] for q in Qb]), other=np.array([[score(e, q) for e in E] for q in Qo]))


def test_recognition_on_the_planted_path(path):
    """Back frame j revisits out frame 15 - j, shifted by (3, 2) pixels.  The figures of this run are printed and recorded in DESIGN.md 4.27; the
    assertions are conditions the oracle alone meets: the planted revisit is rank 1 for every query, and every crop from elsewhere on the canvas
    scores below the default min_score against every entry."""
    lp = kr.Params()
    back, other = path["back"], path["other"]
    n = kc.PATH_N
    revisit = np.array([back[j, n - 1 - j] for j in range(n)])
    far = np.array([back[j, e] for j in range(n) for e in range(n) if abs(e - (n - 1 - j)) >= 8])
    print("keypoints per frame", min(len(e[0]) for e in path["E"]), "-", max(len(e[0]) for e in path["E"]))
    print("revisit scores", revisit.min(), "-", revisit.max(), "| entries 8 or more frames away: at most", far.max(), "| elsewhere", other.min(), "-", other.max())
    for j in range(n):
        assert min(range(n), key=lambda e: (-int(back[j, e]), e)) == n - 1 - j, (j, back[j])      # the contract's order: score falling, then id rising
    assert other.max() < lp.min_score <= revisit.min(), (other.max(), revisit.min())


def test_restatement_ranks_the_path_like_the_oracle(path):
    """the restatement's database over the same descriptors: ids 0 ... 15 out, 16 ... 31 back, min_gap 1 (every entry is eligible)"""
    lp = kr.Params(min_gap=1)
    db = kr.KfDb(32, 2048)
    cap = max(len(k) for k, _ in path["E"] + path["Qb"])

    def pad(sets):
        kps, desc = np.zeros((len(sets), cap), kr.KEYPOINT_DTYPE), np.zeros((len(sets), cap, 32), np.uint8)
        for i, (k, d) in enumerate(sets):
            kps[i, :len(k)], desc[i, :len(k)] = k, d
        return kps, desc, np.array([len(k) for k, _ in sets], np.int32)
    kps, desc, nkp = pad(path["E"])
    db.add_rows(kps, desc, nkp, np.arange(16, dtype=np.int32))
    kps, desc, nkp = pad(path["Qb"])
    scores, cand, query = db.query_rows(lp, desc, nkp, np.arange(16, 32, dtype=np.int32))
    assert (scores[:, :16] == path["back"]).all() and (scores[:, 16:] == -1).all()
    assert cand["id"][:, 0].tolist() == [15 - j for j in range(16)] and (query["n_scored"] == 16).all() and (query["n_cand"] == lp.topk).all()


# ---- bookkeeping on hand-made tables: an entry that holds copies of s rows of the query beside random rows scores exactly s ---------------
table, query_base = kc.table, kc.query_base


def test_ring_wrap_and_empty_entries():
    db = kr.KfDb(4, 32)
    kps, desc, nkp = table([(3, 1), (4, 2), None, (5, 3), (6, 4), (7, 5)])
    ids = np.array([10, 11, 12, -5, 14, 15], np.int32)
    db.add_rows(kps[:3], desc[:3], nkp[:3], ids[:3])
    assert (db.head, db.total) == (3, 3) and db.id.tolist() == [10, 11, 12, -1] and db.cnt.tolist() == [24, 24, 0, 0]
    db.add_rows(kps[3:], desc[3:], nkp[3:], ids[3:])                  # slots 3, 0, 1: the two oldest entries are overwritten
    assert (db.head, db.total) == (2, 6) and db.id.tolist() == [14, 15, 12, -5] and db.cnt.tolist() == [24, 24, 0, 0]
    qk, qd, qn = query_base()
    scores, cand, query = db.query_rows(kr.Params(min_gap=0, min_score=1), qd, qn, np.array([100], np.int32))
    assert scores.tolist() == [[6, 7, -1, -1]]                        # the empty entry and the one with a negative id are never scored
    assert cand["slot"][0].tolist() == [1, 0, -1, -1] and cand[0, 2].tolist() == (-1, -1, 0, 0) and query[0].tolist()[:6] == (100, 24, 2, 2, 7, 0)
    one = kr.KfDb(4, 32)
    one.add_rows(kps, desc, nkp, ids)                                 # the same six rows in ONE call: the same ring
    assert one.id.tolist() == db.id.tolist() and one.cnt.tolist() == db.cnt.tolist() and (one.head, one.total) == (2, 6)
    db.reset()
    assert (db.head, db.total) == (0, 0) and db.get_entry(0)[:2] == (-1, 0)


def test_eligibility_topk_ties_and_min_score():
    db = kr.KfDb(8, 32)
    kps, desc, nkp = table([(5, 1), (5, 2), (9, 3), (5, 4), (2, 5), (9, 6)])
    db.add_rows(kps, desc, nkp, np.array([20, 7, 30, 7, 1, 31], np.int32))
    qk, qd, qn = query_base(3)
    lp = kr.Params(min_gap=10, topk=4, min_score=5)
    scores, cand, query = db.query_rows(lp, qd, qn, np.array([40, 41, 17], np.int32))
    assert scores[0].tolist() == [5, 5, 9, 5, 2, -1, -1, -1]          # id 30 + 10 == 40 is eligible, id 31 is not
    assert scores[1].tolist() == [5, 5, 9, 5, 2, 9, -1, -1]           # one above: id 31 + 10 == 41
    assert cand["slot"][0].tolist() == [2, 1, 3, 0]                   # score falling; the tie on score by id (7, 7, 20), the tie on id by slot
    assert cand["slot"][1].tolist() == [2, 5, 1, 3] and cand["id"][1].tolist() == [30, 31, 7, 7]
    assert scores[2].tolist() == [-1, 5, -1, 5, 2, -1, -1, -1] and cand["slot"][2].tolist() == [1, 3, -1, -1]      # topk above the eligible count
    assert query["n_scored"].tolist() == [5, 6, 3] and query["n_cand"].tolist() == [4, 4, 2] and query["best_score"].tolist() == [9, 9, 5]
    at, above = kr.Params(min_gap=10, topk=16, min_score=9), kr.Params(min_gap=10, topk=16, min_score=10)
    assert db.query_rows(at, qd, qn, np.array([40, 41, 17], np.int32))[2]["n_cand"].tolist() == [1, 2, 0]
    assert db.query_rows(above, qd, qn, np.array([40, 41, 17], np.int32))[2]["n_cand"].tolist() == [0, 0, 0]
    big = kr.Params(min_gap=2 ** 31 - 1, min_score=0)                 # id + min_gap beyond 32 bits: nothing wraps, nothing is eligible
    s, _, q = db.query_rows(big, qd[:1], qn[:1], np.array([2 ** 31 - 1], np.int32))
    assert (s == -1).all() and q[0]["n_scored"] == 0 and q[0]["best_score"] == -1 and q[0]["flags"] == 0


def test_skipped_queries():
    db = kr.KfDb(2, 32)
    kps, desc, nkp = table([(5, 1)])
    db.add_rows(kps, desc, nkp, np.array([0], np.int32))
    qk, qd, qn = query_base(4)
    qn[:] = [24, 0, -7, 24]
    scores, cand, query = db.query_rows(kr.Params(min_gap=0, min_score=0), qd, qn, np.array([5, 5, 5, -1], np.int32))
    assert scores.tolist() == [[5, -1], [-1, -1], [-1, -1], [-1, -1]]
    assert query["flags"].tolist() == [0, 1, 1, 1] and query["n_keypoints"].tolist() == [24, 0, 0, 0] and query["id"].tolist() == [5, 5, 5, -1]
    assert (cand["slot"][1:] == -1).all() and query["n_cand"].tolist() == [1, 0, 0, 0]


def test_match_rows_and_stale_candidates():
    db = kr.KfDb(2, 32)
    kps, desc, nkp = table([(5, 1), (3, 2)])
    db.add_rows(kps, desc, nkp, np.array([0, 1], np.int32))
    qk, qd, qn = query_base(5)
    lp = kr.Params(min_gap=0, min_score=0)
    cand = np.array([(0, 0, 5, 24), (1, 1, 3, 24), (-1, -1, 0, 0), (5, 0, 5, 24), (1, 2, 3, 24)], kr.CAND_DTYPE)      # live, live, none, stale id, slot out of range
    fill = lambda dt, shape: np.full(np.prod(shape) * np.dtype(dt).itemsize, 0xEE, np.uint8).view(dt).reshape(shape)
    m, p1, p2, npts = db.match_rows(lp, qk, qd, qn, cand, 4, fill(kr.DMATCH_DTYPE, (5, 4)), fill(np.float32, (5, 4, 2)), fill(np.float32, (5, 4, 2)), fill(np.int32, (5,)))
    assert npts.tolist() == [5, 3, 0, 0, 0]                           # the FULL count: row 0 is truncated to max_pts = 4 and says so
    assert m["queryIdx"][0].tolist() == [0, 1, 2, 3] and m["trainIdx"][1, :3].tolist() == [0, 1, 2] and (m["imgIdx"][0] == 0).all() and (m["imgIdx"][1, :3] == 1).all()
    assert (m["distance"][0] == 0).all() and p1[0, :, 0].tolist() == [100, 101, 102, 103] and p2[1, :3, 1].tolist() == [0.75, 1.75, 2.75]
    assert (m[1, 3:].view(np.uint8) == 0xEE).all() and (m[2:].view(np.uint8) == 0xEE).all() and (p1[2:].view(np.uint8) == 0xEE).all()
    kps2, desc2, nkp2 = table([(7, 9)])
    db.add_rows(kps2, desc2, nkp2, np.array([2], np.int32))           # slot 0 is overwritten: the candidate (0, 0, ...) is stale now
    _, _, _, npts = db.match_rows(lp, qk, qd, qn, cand, 4, None, fill(np.float32, (5, 4, 2)), fill(np.float32, (5, 4, 2)), fill(np.int32, (5,)))
    assert npts.tolist() == [0, 3, 0, 0, 0]


# ---- the builders of tests/test_kfdb_limits_gpu.py: the oracle agrees with the restatement on every one of them, and they discriminate ------
@pytest.fixture(scope="module")
def ladders():
    return {ns: kc.ladder(ns) for ns in kc.LADDER_NS}


def test_ladder_shape(ladders):
    """every position pair of the issue's list, f at every fixed index named, the random rows far from f"""
    for ns, cs in ladders.items():
        P = kc.ladder_positions(ns)
        assert set(kc.LADDER_P) <= set(P) and (ns == 64 or {64, 65} <= set(P)) and max(P) == ns - 1
        pairs = {(a, b) for i, a in enumerate(P) for b in P[i + 1:]}
        for kind in ("tie", "ab", "ba"):
            assert {(c["a"], c["b"]) for c in cs if c["kind"] == kind} == pairs
        assert {c["f"] for c in cs} == {0, 31, 32, 63, 64, 255, 256, 257} and {c["kind"] for c in cs} >= {"control_ab", "control_ba"}
        for c in cs:
            d = kr.hamming(c["fixed"][c["f"]][None], np.concatenate([c["fixed"], c["swept"]]))[0]
            d[c["f"]] = d[len(c["fixed"]) + c["a"]] = d[len(c["fixed"]) + c["b"]] = 999
            assert d.min() > 64 and len(c["swept"]) == ns and len(c["fixed"]) == dict(kc.LADDER_FIXED_BY_F)[c["f"]]
    assert sum(len(cs) for cs in ladders.values()) == 3 * (120 + 153) + 4


@pytest.mark.parametrize("planted_is_entry", [True, False], ids=["planted_entry", "planted_query"])
def test_ladder_restatement_equals_the_oracle(vislam, orc, ladders, planted_is_entry):
    """keys and list of every ladder couple; the plant decides the list as the builder says: the tie names the lower row, 32 against 39 drops f,
    32 against 40 keeps it"""
    for ns, cs in ladders.items():
        for c in cs:
            E, Q = kc.ladder_sets(c, planted_is_entry)
            p, lp = oracle_params(vislam, c["ratio"], kr.SYM_INTENDED), kr.Params(ratio=c["ratio"], sym_mode=kr.SYM_INTENDED)
            o12, o21 = orc.knn2_hamming(E, Q)
            k12, k21 = kr.couple_keys(E, Q)
            assert (kr.keys_from_dmatch(o12) == k12).all() and (kr.keys_from_dmatch(o21) == k21).all(), (ns, c["kind"], c["a"], c["b"])
            got = kr.sym_list(k12, k21, lp.ratio, lp.sym_mode)
            assert got.tobytes() == oracle_list(orc, p, E, Q).tobytes(), (ns, c["kind"], c["a"], c["b"])
            assert kc.ladder_match_of_f(c, planted_is_entry, got) == c["expect"], (ns, c["kind"], c["a"], c["b"])
            kf = (k12 if planted_is_entry else k21)[c["f"]]
            first, second = (c["b"], c["a"]) if c["kind"] in ("ba", "control_ba") else (c["a"], c["b"])
            assert (kf & 0xFFFF).tolist() == [first, second] and (kf >> 16).tolist() == {"tie": [3, 3], "ab": [32, 39], "ba": [32, 39]}.get(c["kind"], [32, 40])


@pytest.mark.parametrize("wrong", [kc.wrong_knn2_tie_to_the_higher_row, kc.wrong_knn2_second_is_the_third, kc.wrong_knn2_halves_merged_by_their_seconds])
def test_ladder_discriminates(ladders, wrong):
    """each deliberately wrong 2-NN changes the expected bytes of ladder couples, in both orientations -- and of none of the wrong kind: a tie
    does not notice a lost second neighbour, a first / second pair does not notice the tie rule"""
    changed = {(o, k): 0 for o in (True, False) for k in ("tie", "ab", "ba")}
    for cs in ladders.values():
        for c in cs[::5] + [x for x in cs if (x["a"], x["b"]) in ((3, 4), (31, 32), (0, 63))]:
            lp = kr.Params(ratio=c["ratio"], sym_mode=kr.SYM_INTENDED)
            for o in (True, False):
                E, Q = kc.ladder_sets(c, o)
                if kr.couple_list(E, Q, lp).tobytes() != kr.couple_list(E, Q, lp, keys_fn=kc.wrong_keys(wrong)).tobytes() and c["kind"] in ("tie", "ab", "ba"):
                    changed[(o, c["kind"])] += 1
    print(wrong.__name__, changed)
    tie_rule = wrong is kc.wrong_knn2_tie_to_the_higher_row
    for o in (True, False):
        assert (changed[(o, "tie")] > 0) == tie_rule and (changed[(o, "ab")] > 0) == (not tie_rule) and (changed[(o, "ba")] > 0) == (not tie_rule), changed


@pytest.mark.parametrize("sym_mode", [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED])
@pytest.mark.parametrize("ratio", [kc.F8, 1.0])
def test_all_equal_sets_against_the_oracle(vislam, orc, ratio, sym_mode):
    """every distance 0: entry 0 and query 0 take each other, the score is 1; every distance 256: 256 > 0.8f * 256 drops everything, ratio 1.0 keeps
    the same single match"""
    entries, queries = kc.all_equal_sets()
    p, lp = oracle_params(vislam, ratio, sym_mode), kr.Params(ratio=ratio, sym_mode=sym_mode)
    n4 = len(kc.ALL_EQUAL_COUNTS)
    for i, E in enumerate(entries):
        for j, Q in enumerate(queries):
            got = kr.couple_list(E, Q, lp)
            assert got.tobytes() == oracle_list(orc, p, E, Q).tobytes(), (i, j)
            if i < n4 and j < n4:
                assert got[["queryIdx", "trainIdx"]].tolist() == [(0, 0)] and got["distance"][0] == 0
            if i >= n4 and j >= n4:
                assert got["distance"].tolist() == ([256.0] if ratio == 1.0 else [])


@pytest.mark.parametrize("entry_cap", kc.RING_CAPS)
def test_ring_tables_tell_the_orders_apart(entry_cap):
    """the large-ring tables: the scores are the planted ones, 15 / 16 / 17 entries at or above the three min_scores, and a top-k ordered by
    (score, slot) instead of (score, id, slot) gives other bytes"""
    db = kr.KfDb(entry_cap, 32)
    kps, desc, nkp, ids = kc.ring_table(entry_cap)
    db.add_rows(kps, desc, nkp, ids)
    qk, qd, qn, qi = kc.ring_queries(entry_cap)
    for ms, count in kc.RING_MIN_SCORES.items():
        lp = kr.Params(min_gap=0, topk=16, min_score=ms)
        scores, cand, query = db.query_rows(lp, qd, qn, qi)
        assert [int(scores[0, s]) for g in kc.RING_GROUPS[entry_cap] for s in g] == [9 - i for i, g in enumerate(kc.RING_GROUPS[entry_cap]) for _ in g]
        assert (scores[0, [30, 40, 70, 71]] == [6, 6, 5, 4]).all() and scores[0].max() == 12 and (scores[0] >= ms).sum() == count
        assert query["n_cand"].tolist()[:2] == [min(count, 16), 0] and query["flags"].tolist() == [0, 1, 0]
        assert 0 < query["n_cand"][2] < 15                                 # (the entries of score 12 are too young for the last query)
        assert query["n_scored"].tolist()[0] == entry_cap and 17 < query["n_scored"][2] < entry_cap
        by_slot = db.query_rows(lp, qd, qn, qi, rank_key=lambda sc, i_, s_: (-sc, s_))
        assert by_slot[1].tobytes() != cand.tobytes() and by_slot[0].tobytes() == scores.tobytes()
        slots = cand["slot"][0, :count].tolist()
        assert slots.index(40) < slots.index(30)                           # id 800 before id 900
        for g in kc.RING_GROUPS[entry_cap]:
            at = [slots.index(s) for s in g]
            assert at == list(range(at[0], at[0] + len(g)))                # equal (score, id): slot rising, next to each other
    for ms, count in ((-2 ** 31, 16), (2 ** 31 - 1, 0)):
        assert db.query_rows(kr.Params(min_gap=0, topk=16, min_score=ms), qd, qn, qi)[2]["n_cand"].tolist() == [count, 0, count]


def test_long_adds_in_the_restatement():
    """one add call that laps a ring of 7 slots thousands of times leaves the last 7 rows, as adding them one call at a time does"""
    n = 65536 + 7 * 3 + 2
    kps, desc, nkp, ids = kc.scored_rows(n, 4)
    one, many = kr.KfDb(7, 8), kr.KfDb(7, 8)
    one.add_rows(kps, desc, nkp, ids)
    many.add_rows(kps[:n - 7], desc[:n - 7], nkp[:n - 7], ids[:n - 7])
    many.add_rows(kps[n - 7:], desc[n - 7:], nkp[n - 7:], ids[n - 7:])
    assert (one.head, one.total) == (many.head, many.total) == (n % 7, n) and one.id.tolist() == many.id.tolist() and one.cnt.tolist() == many.cnt.tolist()
    assert sorted(one.id.tolist()) == sorted(ids[n - 7:].tolist()) and (one.cnt > 0).sum() >= 3


def test_ratio_ends_give_different_scores():
    """ratios 1.0, 2.0, +inf, -1.0 and the smallest float32 denormal on a planted couple: the restatement evaluates !(d0 > (double)(float)ratio * d1)
    as written; at least two of them differ (they all do but 2.0 and +inf)"""
    E, Q, _ = kc.planted_sets(1234, 300, 257)
    for mode in (kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED):
        scores = [len(kr.couple_list(E, Q, kr.Params(ratio=r, sym_mode=mode))) for r in kc.RATIO_ENDS]
        print("ratio ends", kc.RATIO_ENDS, "mode", mode, "scores", scores)
        assert len(set(scores)) >= 2 and scores[0] > scores[3] and scores[4] >= 1 and scores[2] >= scores[0]


def test_rows_without_room_and_calls_without_rows():
    """row_cap 0 and n 0 in the restatement: empty entries and a moving head; nothing at all"""
    db = kr.KfDb(4, 32)
    kps, desc, nkp = kc.table([(5, 1), (3, 2)])
    db.add_rows(kps, desc, nkp, np.array([0, 1], np.int32))
    db.add_rows(kps[:0], desc[:0], nkp[:0], np.zeros(0, np.int32))
    assert (db.head, db.total) == (2, 2)
    db.add_rows(kps[:, :0], desc[:, :0], nkp, np.array([2, 3], np.int32))
    assert (db.head, db.total) == (0, 4) and db.cnt.tolist() == [24, 24, 0, 0] and db.id.tolist() == [0, 1, 2, 3]
    qk, qd, qn = kc.query_base(2)
    lp = kr.Params(min_gap=0, min_score=0)
    scores, cand, query = db.query_rows(lp, qd[:, :0], qn, np.array([9, 9], np.int32))
    assert (scores == -1).all() and query["flags"].tolist() == [1, 1] and query["n_keypoints"].tolist() == [0, 0]
    scores, cand, query = db.query_rows(lp, qd[:0], qn[:0], np.zeros(0, np.int32))
    assert scores.shape == (0, 4) and cand.shape == (0, 4) and query.shape == (0,)
