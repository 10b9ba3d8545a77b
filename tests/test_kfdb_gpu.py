"""GPU: the keyframe database and the loop scorer (vis_kfdb_*) against the restatement tests/kfdb_ref.py, BYTE FOR BYTE: the whole score row, the
candidates, the query records, the ring as vis_kfdb_get_entry reads it back, the match rows.  Outputs are pre-filled with 0xEE and what the
contract leaves alone (match rows beyond the list or of a stale candidate, the guard entries behind every buffer) must keep it.  Shapes: kp_cap 320
with counts on either side of the 32-row tile, the wave, the 256-descriptor chunk of a workgroup and a second chunk; entry_cap around the deal over
8 XCDs; one couple at the ageing-key limit of 16384 rows."""
import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr

pytestmark = pytest.mark.gpu
FILL = 0xEE
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
F8 = float(np.float32(0.8))


def _dev(torch, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).cuda()    # (never an empty allocation)
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes + 32,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _back(t, nbytes, dtype):
    raw = t.cpu().numpy()
    assert (raw[nbytes:] == FILL).all(), "the guard entries behind a buffer were written"
    return raw[:nbytes].view(dtype)


def params(vislam, **kw):
    lp, lq = vislam.default_loop_params(), kr.Params()
    for k, v in kw.items():
        setattr(lp, k, v)
        setattr(lq, k, v)
    return lp, lq


class Pair:
    """a device database and the restatement's, fed the same calls"""

    def __init__(self, vislam, c, entry_cap, kp_cap, keys_fn=kr.couple_keys):
        import torch
        self.v, self.c, self.torch = vislam, c, torch
        self.dev, self.ref = c.kfdb(entry_cap, kp_cap), kr.KfDb(entry_cap, kp_cap, keys_fn)
        self.entry_cap, self.kp_cap = entry_cap, kp_cap

    def close(self):
        self.dev.close()

    def add(self, kps, desc, nkp, ids, ref_nkp=None):
        t = [_dev(self.torch, a) for a in (kps, desc, np.asarray(nkp, np.int32), np.asarray(ids, np.int32))]
        self.dev.add_rows(len(nkp), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), kps.shape[1], t[3].data_ptr())
        self.c.batch_sync()
        self.ref.add_rows(kps, desc, nkp if ref_nkp is None else ref_nkp, ids)

    def same_ring(self):
        info = self.dev.info()
        assert (info.entry_cap, info.kp_cap, info.head, info.total_added) == (self.entry_cap, self.kp_cap, self.ref.head, self.ref.total)
        for s in range(self.entry_cap):
            i, n, xy = self.dev.get_entry(s)
            ri, rn, rxy = self.ref.get_entry(s)
            assert (i, n) == (ri, rn) and xy.tobytes() == rxy.tobytes(), (s, i, n, ri, rn)

    def query(self, lp, lq, desc, nkp, ids, with_scores=True):
        n, E, torch = len(nkp), self.entry_cap, self.torch
        t = [_dev(torch, a) for a in (desc, np.asarray(nkp, np.int32), np.asarray(ids, np.int32))]
        sc, ca, qu = _filled(torch, n * E * 4), _filled(torch, n * lp.topk * 16), _filled(torch, n * 32)
        self.dev.query_rows(n, t[0].data_ptr(), t[1].data_ptr(), desc.shape[1], t[2].data_ptr(), sc.data_ptr() if with_scores else 0, ca.data_ptr(),
                            qu.data_ptr(), lp)
        self.c.batch_sync()
        got = (_back(sc, n * E * 4 if with_scores else 0, np.int32).reshape(n, -1), _back(ca, n * lp.topk * 16, kr.CAND_DTYPE).reshape(n, lp.topk),
               _back(qu, n * 32, kr.QUERY_DTYPE))
        want = self.ref.query_rows(lq, desc, nkp, ids)
        if with_scores:
            assert got[0].tobytes() == want[0].tobytes(), (np.argwhere(got[0] != want[0])[:6], got[0][got[0] != want[0]][:6], want[0][got[0] != want[0]][:6])
        assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
        assert got[2].tobytes() == want[2].tobytes(), (got[2], want[2])
        return want

    def match(self, lp, lq, kps, desc, nkp, cand, stride, rank, max_pts, with_matches=True):
        """cand: (n, stride) records on the device; the call reads record `rank` of every row"""
        n, torch = len(nkp), self.torch
        t = [_dev(torch, a) for a in (kps, desc, np.asarray(nkp, np.int32), cand)]
        m, p1, p2, npts = _filled(torch, n * max_pts * 16), _filled(torch, n * max_pts * 8), _filled(torch, n * max_pts * 8), _filled(torch, n * 4)
        self.dev.match_rows(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), desc.shape[1], t[3].data_ptr() + 16 * rank, stride, max_pts,
                            m.data_ptr() if with_matches else 0, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), lp)
        self.c.batch_sync()
        got = (_back(m, n * max_pts * 16, kr.DMATCH_DTYPE).reshape(n, max_pts), _back(p1, n * max_pts * 8, np.float32).reshape(n, max_pts, 2),
               _back(p2, n * max_pts * 8, np.float32).reshape(n, max_pts, 2), _back(npts, n * 4, np.int32))
        fill = lambda dt, shape: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape(shape)
        want = self.ref.match_rows(lq, kps, desc, nkp, cand.reshape(n, stride)[:, rank], max_pts, fill(kr.DMATCH_DTYPE, (n, max_pts)),
                                   fill(np.float32, (n, max_pts, 2)), fill(np.float32, (n, max_pts, 2)), fill(np.int32, (n,)))
        assert got[3].tolist() == want[3].tolist(), (got[3], want[3])
        if with_matches:
            assert got[0].tobytes() == want[0].tobytes(), np.argwhere(got[0] != want[0])[:6]
        else:
            assert (got[0].view(np.uint8) == FILL).all()
        assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        return want


@pytest.fixture(scope="module")
def master():
    """one planted couple of 300 x 300; the sets of the count tests are its prefixes, so that every size has true correspondences"""
    return kc.planted_sets(77, 300, 300)


@pytest.mark.parametrize("row_cap", [352, 288], ids=["row_cap_above_kp_cap", "row_cap_below_kp_cap"])
@pytest.mark.parametrize("sym_mode", [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED])
def test_counts_on_either_side_of_a_couple(vislam, ctx, master, row_cap, sym_mode):
    """16 entries x 16 queries with every count of kfdb_cases.COUNTS on either side: the tile tail, the wave edges, the 256-descriptor chunk of a
    workgroup and a second chunk; kp_cap 320, and with row_cap 288 the count 300 is clamped"""
    E, Q, _ = master
    rng = np.random.default_rng(5)
    pr = Pair(vislam, ctx, 16, 320)
    kps, desc, nkp = kc.rows(rng, [E[:c] for c in kc.COUNTS], row_cap)
    pr.add(kps, desc, nkp, np.arange(16))
    pr.same_ring()
    qk, qd, qn = kc.rows(rng, [Q[:c] for c in kc.COUNTS], row_cap)
    lp, lq = params(vislam, sym_mode=sym_mode, min_gap=0, min_score=1, topk=16)
    scores, cand, query = pr.query(lp, lq, qd, qn, np.full(16, 100))
    assert query["flags"].tolist() == [1] + [0] * 15 and (scores[1:, 0] == -1).all() and (scores[1:, 1:] >= 0).all()
    assert scores[15, 15] >= 100 and scores[12, 12] > 50 and len(np.unique(scores)) > 30              # not a comparison of empty lists
    pr.close()


@pytest.mark.parametrize("entry_cap", [1, 7, 8, 9, 17])
def test_entry_caps_around_the_deal_over_the_xcds(vislam, ctx, master, entry_cap):
    """ring wrap inside one add call and across calls, an add of more rows than entry_cap; 1, 3 and 9 queries after each"""
    E, Q, _ = master
    rng = np.random.default_rng(entry_cap)
    pr = Pair(vislam, ctx, entry_cap, 64)
    lp, lq = params(vislam, min_gap=2, min_score=1, topk=3)
    next_id = 0
    for n_add, n_q in ((3, 1), (entry_cap + 2, 3), (2, 9), (max(entry_cap - 1, 1), 3)):
        sets = [E[o:o + 40 + (o % 9)] for o in rng.integers(0, 200, n_add)]
        kps, desc, nkp = kc.rows(rng, sets, 64)
        pr.add(kps, desc, nkp, np.arange(next_id, next_id + n_add))
        next_id += n_add
        pr.same_ring()
        qk, qd, qn = kc.rows(rng, [Q[o:o + 50] for o in rng.integers(0, 200, n_q)], 64)
        scores, _, _ = pr.query(lp, lq, qd, qn, next_id - 1 + np.arange(n_q))
        pr.query(lp, lq, qd, qn, next_id - 1 + np.arange(n_q), with_scores=False)
    assert (scores >= 0).any() or entry_cap == 1
    pr.dev.reset()
    pr.ref.reset()
    pr.same_ring()
    pr.close()


@pytest.mark.parametrize("ratio", [F8, 0.5, 0.75, 0.0, float("nan")])
def test_ratio_boundaries_duplicates_and_both_modes(vislam, ctx, ratio):
    E, Q, plants = kc.planted_sets(1234, 300, 257, ratio)
    rng = np.random.default_rng(9)
    pr = Pair(vislam, ctx, 2, 320)
    kps, desc, nkp = kc.rows(rng, [E, E[:129]], 320)
    pr.add(kps, desc, nkp, [0, 1])
    qk, qd, qn = kc.rows(rng, [Q, Q[:65]], 320)
    per_mode = []
    for mode in (kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED):
        lp, lq = params(vislam, ratio=ratio, sym_mode=mode, min_gap=0, min_score=0)
        scores, cand, _ = pr.query(lp, lq, qd, qn, [5, 6])
        cd = np.zeros((2, 4), kr.CAND_DTYPE)
        cd[:] = cand
        m = pr.match(lp, lq, qk, qd, qn, cd, 4, 0, 320)[0]
        per_mode.append((int(scores[0, 0]), set(m["queryIdx"][0, :scores[0, 0]].tolist())))
    if ratio in kc.BOUNDARIES:
        for _, got in per_mode:
            assert plants["on"] in got and plants["below"] in got and plants["above"] not in got
        # the query row of this plant has two entries at the same distance: direction 2 fails the ratio test, direction 1 does not
        assert plants["one_sided"] in per_mode[0][1] and plants["one_sided"] not in per_mode[1][1] and per_mode[0][0] > per_mode[1][0]
    pr.close()


def test_one_couple_at_the_ageing_key_limit(vislam, orc, ctx):
    """16384 x 16353 descriptors at kp_cap 16384: 512 tiles, the last of ONE row, 64 column chunks per direction, 128 KB of winner tables in LDS.
    Planted as tests/hamming_ref.py does for the matcher: ties between the first and the last row of either side.  The restatement takes its keys from
    the CPU oracle's 2-NN (the numpy product does not fit)."""
    import hamming_ref as hr
    rng = np.random.default_rng(16384)
    E = rng.integers(0, 256, (16384, 32), dtype=np.uint8)
    Q = rng.integers(0, 256, (16353, 32), dtype=np.uint8)
    rows = hr.plant(E, Q)
    for e in range(100, 4000, 3):                                 # true correspondences, or the list would be empty
        if (7 * e) % 16353 in (0, rows["zero_t"], rows["tie_t"], 16352):
            continue
        Q[(7 * e) % 16353] = kc.flip(E[e], rng.choice(256, int(rng.integers(0, 30)), replace=False))

    def oracle_keys(e, q):
        o12, o21 = orc.knn2_hamming(e, q)
        return kr.keys_from_dmatch(o12), kr.keys_from_dmatch(o21)
    pr = Pair(vislam, ctx, 1, 16384, oracle_keys)
    kps, desc, nkp = kc.rows(rng, [E], 16384)
    pr.add(kps, desc, nkp, [0])
    qk, qd, qn = kc.rows(rng, [Q], 16384)
    lp, lq = params(vislam, min_gap=0, min_score=0, topk=1)
    scores, cand, _ = pr.query(lp, lq, qd, qn, [1])
    k12, k21 = oracle_keys(E, Q)
    assert (k12[rows["tie_q"]] & 0xFFFF).tolist() == [0, 16352] and (k21[rows["tie_t"]] & 0xFFFF).tolist() == [0, 16383]
    print("score at 16384 x 16353:", int(scores[0, 0]))
    assert scores[0, 0] > 1000
    cd = np.zeros((1, 1), kr.CAND_DTYPE)
    cd[:] = cand
    pr.match(lp, lq, qk, qd, qn, cd, 1, 0, 2048)                 # truncated: d_npts says so
    pr.close()


def test_hostile_counts_and_ids(vislam, ctx, master):
    E, Q, _ = master
    rng = np.random.default_rng(3)
    pr = Pair(vislam, ctx, 8, 96)
    hostile = [-1, INT_MIN, INT_MAX, 97, 200, 0, 64, 50]        # (counts above row_cap = 80 or kp_cap = 96 are clamped to 80)
    kps, desc, nkp = kc.rows(rng, [E[:80]] * 8, 80, counts=hostile)
    ids = [0, 1, 2, 3, INT_MAX, 5, -1, INT_MAX - 1]
    pr.add(kps, desc, nkp, ids)
    pr.same_ring()
    assert pr.ref.cnt.tolist() == [0, 0, 80, 80, 80, 0, 0, 50]
    qk, qd, qn = kc.rows(rng, [Q[:80]] * 6, 80, counts=[INT_MAX, INT_MIN, -1, 81, 40, 80])
    for gap in (0, 1, INT_MAX):                                   # id + min_gap beyond 32 bits must not wrap into eligibility
        lp, lq = params(vislam, min_gap=gap, min_score=0, topk=8)
        scores, _, query = pr.query(lp, lq, qd, qn, [INT_MAX, 7, 7, INT_MAX - 1, INT_MAX, -1])
        assert query["flags"].tolist() == [0, 1, 1, 0, 0, 1] and query["n_keypoints"].tolist() == [80, 0, 0, 80, 40, 0]
    assert (scores[:, 4] == -1).all() and scores[0].tolist()[:4] == [-1, -1, -1, -1]
    pr.close()


def test_topk_and_eligibility_through_the_device(vislam, ctx):
    """the hand-made tables of tests/test_kfdb_ref.py: the tie on score and on id, topk above the eligible count, min_score at and above a score"""
    pr = Pair(vislam, ctx, 8, 32)
    kps, desc, nkp = kc.table([(5, 1), (5, 2), (9, 3), (5, 4), (2, 5), (9, 6)])
    pr.add(kps, desc, nkp, [20, 7, 30, 7, 1, 31])
    qk, qd, qn = kc.query_base(3)
    for kw in (dict(topk=4, min_score=5), dict(topk=16, min_score=9), dict(topk=16, min_score=10), dict(topk=1, min_score=-5), dict(topk=2, min_score=2)):
        lp, lq = params(vislam, min_gap=10, **kw)
        scores, cand, query = pr.query(lp, lq, qd, qn, [40, 41, 17])
    assert scores[1].tolist() == [5, 5, 9, 5, 2, 9, -1, -1] and cand["slot"][1].tolist() == [2, 5]
    pr.close()


def test_emission(vislam, ctx, master):
    """max_pts exactly the count, one below it and 1; d_matches NULL; a candidate of (-1, ...); a slot overwritten since the query; cand_stride of
    topk records read at rank 0 and rank 1"""
    E, Q, _ = master
    rng = np.random.default_rng(11)
    pr = Pair(vislam, ctx, 3, 320)
    kps, desc, nkp = kc.rows(rng, [E[:300], E[:200], E[40:260]], 320)
    pr.add(kps, desc, nkp, [0, 1, 2])
    qk, qd, qn = kc.rows(rng, [Q[:300], Q[:150], Q[:1], Q[:0]], 320)
    lp, lq = params(vislam, min_gap=0, min_score=20, topk=2)
    scores, cand, _ = pr.query(lp, lq, qd, qn, [9, 9, 9, 9])
    assert cand["slot"][2].tolist() == [-1, -1] and (cand["slot"][:2] >= 0).all()
    count = int(cand["score"][0, 0])
    for rank in (0, 1):
        for max_pts in (count, count - 1, 1, 320):
            pr.match(lp, lq, qk, qd, qn, cand, 2, rank, max_pts)
    pr.match(lp, lq, qk, qd, qn, cand, 2, 0, count, with_matches=False)
    victim = int(cand["slot"][0, 0])
    k2, d2, n2 = kc.rows(rng, [E[:100]] * (victim + 1), 320)
    pr.add(k2, d2, n2, 10 + np.arange(victim + 1))               # the ring comes round to the slot of query 0's best candidate: it is stale now
    want = pr.match(lp, lq, qk, qd, qn, cand, 2, 0, count)
    assert want[3][0] == 0
    pr.close()


def test_chained_verification_on_the_planted_path(vislam, orc):
    """two revisits of the planted path: vis_essential_batch on the rows the device emitted gives the records it gives on the restatement's rows"""
    import torch
    p = kc.path_params(vislam.default_params())
    c = vislam.Context(0, p)
    out, back, _ = kc.path_frames(vislam.synth_canvas(1024))
    ents, qrys = [orc.orb_detect_compute(p, out[i]) for i in (15, 12)], [orc.orb_detect_compute(p, back[j]) for j in (0, 3)]
    cap = 1024

    def pad(sets):
        kps, desc = np.zeros((len(sets), cap), kr.KEYPOINT_DTYPE), np.zeros((len(sets), cap, 32), np.uint8)
        for i, (k, d) in enumerate(sets):
            kps[i, :len(k)], desc[i, :len(k)] = k, d
        return kps, desc, np.array([len(k) for k, _ in sets], np.int32)
    pr = Pair(vislam, c, 4, cap)
    pr.add(*pad(ents), [15, 12])
    qk, qd, qn = pad(qrys)
    lp, lq = params(vislam, min_gap=1, topk=1)
    _, cand, _ = pr.query(lp, lq, qd, qn, [16, 19])
    assert cand["id"][:, 0].tolist() == [15, 12] and (cand["score"][:, 0] > 500).all()
    n, max_pts = 2, cap
    t = [_dev(torch, a) for a in (qk, qd, qn, cand)]
    p1, p2, npts = _filled(torch, n * max_pts * 8), _filled(torch, n * max_pts * 8), _filled(torch, n * 4)
    rec = [_filled(torch, n * vislam.POSE_RESULT_DTYPE.itemsize) for _ in range(2)]
    pr.dev.match_rows(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), cap, t[3].data_ptr(), 1, max_pts, 0, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), lp)
    c.essential_batch(n, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), max_pts, 0, 0, rec[0].data_ptr())     # queued behind the emission, no host step
    c.batch_sync()
    fill = lambda dt, shape: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape(shape)
    _, w1, w2, wn = pr.ref.match_rows(lq, qk, qd, qn, cand[:, 0], max_pts, None, fill(np.float32, (n, max_pts, 2)), fill(np.float32, (n, max_pts, 2)),
                                      fill(np.int32, (n,)))
    u = [_dev(torch, a) for a in (w1, w2, wn)]
    c.essential_batch(n, u[0].data_ptr(), u[1].data_ptr(), u[2].data_ptr(), max_pts, 0, 0, rec[1].data_ptr())
    c.batch_sync()
    nb = n * vislam.POSE_RESULT_DTYPE.itemsize
    got, want = _back(rec[0], nb, vislam.POSE_RESULT_DTYPE), _back(rec[1], nb, vislam.POSE_RESULT_DTYPE)
    assert got.tobytes() == want.tobytes()
    print("loop verification: matches", wn.tolist(), "inliers", got["n_inliers"].tolist())
    assert (got["n_inliers"] > 100).all()
    pr.close()
    c.close()
