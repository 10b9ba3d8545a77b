"""numpy restatement of the loop-candidate contract (include/vislam_hip.h, "loop-closure candidates"): the score and the match list of a couple, the
ring, eligibility, top-k and emission.  Not a test module: tests/test_kfdb_ref.py checks it against the CPU oracle, tests/test_kfdb_gpu.py and
tests/test_kfdb_stream_gpu.py compare the device with it BYTE FOR BYTE (everything is integer arithmetic).  Python ints where 32 bits could wrap."""
import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
CAND_DTYPE = np.dtype([("id", "<i4"), ("slot", "<i4"), ("score", "<i4"), ("n_keypoints", "<i4")])
QUERY_DTYPE = np.dtype([("id", "<i4"), ("n_keypoints", "<i4"), ("n_scored", "<i4"), ("n_cand", "<i4"), ("best_score", "<i4"), ("flags", "<i4"),
                        ("reserved_", "<i4", (2,))])
PARAM_FIELDS = ("ratio", "sym_mode", "min_gap", "topk", "min_score", "reserved_")
SYM_REFERENCE_EFFECTIVE, SYM_INTENDED = 0, 1
LOOP_SKIPPED = 1
NONE = 0xFFFFFFFF
MAX_ENTRY_CAP, MAX_KP_CAP, MAX_TOPK = 65536, 16384, 16


class Params:
    """vis_loop_params with vis_default_loop_params' values"""

    def __init__(self, **kw):
        self.ratio, self.sym_mode, self.min_gap, self.topk, self.min_score, self.reserved_ = float(np.float32(0.8)), SYM_INTENDED, 30, 4, 30, 0
        for k, v in kw.items():
            assert k in PARAM_FIELDS, k
            setattr(self, k, v)


def params_ok(lp):
    return lp.sym_mode in (SYM_REFERENCE_EFFECTIVE, SYM_INTENDED) and lp.min_gap >= 0 and 1 <= lp.topk <= MAX_TOPK


# ---- a couple -------------------------------------------------------------------------------------------------------------------------
def hamming(a, b):
    """(len(a), len(b)) Hamming distances of 32-byte rows"""
    A = np.unpackbits(np.ascontiguousarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)      # (sums of at most 256 ones: exact in float)
    B = np.unpackbits(np.ascontiguousarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (A @ (1 - B).T + (1 - A) @ B.T).astype(np.int32)


def knn2_keys(fixed, swept):
    """the matcher's keys: per row of `fixed` the two smallest (Hamming << 16) | row over `swept` (ties: the lower row), NONE where there is none"""
    nf, ns = len(fixed), len(swept)
    out = np.full((nf, 2), NONE, np.uint32)
    if nf and ns:
        keys = np.sort((hamming(fixed, swept).astype(np.int64) << 16) | np.arange(ns, dtype=np.int64)[None, :], axis=1)
        out[:, :min(ns, 2)] = keys[:, :2].astype(np.uint32)
    return out


def keys_from_dmatch(two):
    """the same keys from a 2-NN list in DMATCH form (the CPU oracle's): trainIdx < 0 = no neighbour"""
    t = two["trainIdx"].astype(np.int64)
    d = np.where(t < 0, 0.0, two["distance"]).astype(np.int64)
    return np.where(t < 0, NONE, (d << 16) | t).astype(np.uint32)


def ratio_survives(keys, ratio):
    """nnFilter on a key pair: two neighbours and !(d0 > (double)(float)ratio * d1)"""
    r = np.float64(np.float32(ratio))
    d0, d1 = (keys[:, 0] >> 16).astype(np.float64), (keys[:, 1] >> 16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (keys[:, 0] != NONE) & (keys[:, 1] != NONE) & ~(d0 > r * d1)


def sym_list(k12, k21, ratio, sym_mode, slot=-1):
    """computeSymMatches on the keys of both directions (k12: entry -> query): the match list, queryIdx rising"""
    n1 = len(k12)
    ok = ratio_survives(k12, ratio)
    t = (k12[:, 0] & 0xFFFF).astype(np.int64)
    t_ok = np.where(ok, t, 0)
    if len(k21):
        b0 = k21[t_ok, 0]
        ok &= (b0 != NONE) & ((b0 & 0xFFFF).astype(np.int64) == np.arange(n1))
        if sym_mode == SYM_INTENDED:
            ok &= ratio_survives(k21, ratio)[t_ok]
    else:
        ok[:] = False
    q = np.flatnonzero(ok)
    m = np.zeros(len(q), DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["imgIdx"], m["distance"] = q, t[q], slot, (k12[q, 0] >> 16).astype(np.float32)
    return m


def couple_keys(e_desc, q_desc):
    return knn2_keys(e_desc, q_desc), knn2_keys(q_desc, e_desc)


def couple_list(e_desc, q_desc, lp, slot=-1, keys_fn=couple_keys):
    k12, k21 = keys_fn(e_desc, q_desc)
    return sym_list(k12, k21, lp.ratio, lp.sym_mode, slot)


# ---- the database ---------------------------------------------------------------------------------------------------------------------
def clamp_count(n, row_cap, kp_cap):
    return min(max(int(n), 0), min(row_cap, kp_cap))


def row_cap_of(desc, n):
    """the row capacity of a call's padded descriptor rows; 0 for no rows or rows without room for a keypoint"""
    d = np.asarray(desc)
    return 0 if n == 0 or d.size == 0 else d.reshape(n, -1, 32).shape[1]


class KfDb:
    """the ring as the contract states it; keys_fn(e_desc, q_desc) -> (k12, k21) may be replaced (the CPU oracle's 2-NN for sets too large for numpy)"""

    def __init__(self, entry_cap, kp_cap, keys_fn=couple_keys):
        assert 1 <= entry_cap <= MAX_ENTRY_CAP and 1 <= kp_cap <= MAX_KP_CAP
        self.entry_cap, self.kp_cap, self.keys_fn = entry_cap, kp_cap, keys_fn
        self.reset()

    def reset(self):
        self.head, self.total = 0, 0
        self.id = np.full(self.entry_cap, -1, np.int32)
        self.cnt = np.zeros(self.entry_cap, np.int32)
        self.desc = [np.zeros((0, 32), np.uint8) for _ in range(self.entry_cap)]
        self.xy = [np.zeros((0, 2), np.float32) for _ in range(self.entry_cap)]

    def add_rows(self, kps, desc, nkp, ids):
        """kps (n, row_cap) KEYPOINT_DTYPE, desc (n, row_cap, 32), nkp / ids (n,): the n slots behind the head, in order"""
        n = len(nkp)
        row_cap = row_cap_of(desc, n)
        for i in range(n):
            s = (self.head + i) % self.entry_cap
            c = clamp_count(nkp[i], row_cap, self.kp_cap)
            if int(ids[i]) < 0:
                c = 0
            self.id[s], self.cnt[s] = ids[i], c
            self.desc[s] = np.array(desc[i][:c], np.uint8).reshape(c, 32)
            self.xy[s] = np.stack([kps[i]["x"][:c], kps[i]["y"][:c]], 1).astype(np.float32).reshape(c, 2)
        self.head, self.total = (self.head + n) % self.entry_cap, self.total + n

    def get_entry(self, slot):
        return int(self.id[slot]), int(self.cnt[slot]), self.xy[slot].copy()

    def eligible(self, slot, id_q, lp):
        return self.cnt[slot] > 0 and id_q >= 0 and int(self.id[slot]) + int(lp.min_gap) <= int(id_q)

    def query_rows(self, lp, desc, nkp, ids, rank_key=None):
        """-> (scores (n, entry_cap) int32, cand (n, topk) CAND_DTYPE, query (n,) QUERY_DTYPE); rank_key(score, id, slot): a sort key in place of
        the contract's (score falling, id rising, slot rising) -- for the tests that show a table tells the orders apart"""
        assert params_ok(lp)
        rank_key = rank_key or (lambda sc, i_, s_: (-sc, i_, s_))
        n = len(nkp)
        row_cap = row_cap_of(desc, n)
        scores = np.full((n, self.entry_cap), -1, np.int32)
        cand = np.zeros((n, lp.topk), CAND_DTYPE)
        cand["id"], cand["slot"] = -1, -1
        query = np.zeros(n, QUERY_DTYPE)
        for i in range(n):
            c = clamp_count(nkp[i], row_cap, self.kp_cap)
            if int(ids[i]) < 0:
                c = 0
            if c > 0:
                qd = np.asarray(desc[i][:c], np.uint8).reshape(c, 32)
                for s in range(self.entry_cap):
                    if self.eligible(s, int(ids[i]), lp):
                        scores[i, s] = len(couple_list(self.desc[s], qd, lp, s, self.keys_fn))
            order = sorted((s for s in range(self.entry_cap) if scores[i, s] >= 0 and scores[i, s] >= lp.min_score),
                           key=lambda s: rank_key(int(scores[i, s]), int(self.id[s]), s))[:lp.topk]
            for r, s in enumerate(order):
                cand[i, r] = (self.id[s], s, scores[i, s], self.cnt[s])
            query[i] = (ids[i], c, int((scores[i] >= 0).sum()), len(order), int(scores[i].max()), 0 if c > 0 else LOOP_SKIPPED, (0, 0))
        return scores, cand, query

    def match_rows(self, lp, kps, desc, nkp, cand, max_pts, matches, p1, p2, npts):
        """cand: ONE record per query; matches (n, max_pts) DMATCH_DTYPE or None, p1 / p2 (n, max_pts, 2) float32, npts (n,) int32: the caller's
        buffers as they were, returned with what the call writes"""
        assert params_ok(lp)
        n = len(nkp)
        row_cap = row_cap_of(desc, n)
        matches = None if matches is None else matches.copy()
        p1, p2, npts = p1.copy(), p2.copy(), npts.copy()
        for i in range(n):
            c = clamp_count(nkp[i], row_cap, self.kp_cap)
            s = int(cand[i]["slot"])
            if not (0 <= s < self.entry_cap and c > 0 and self.cnt[s] > 0 and int(self.id[s]) == int(cand[i]["id"])):
                npts[i] = 0
                continue
            m = couple_list(self.desc[s], np.asarray(desc[i][:c], np.uint8).reshape(c, 32), lp, s, self.keys_fn)
            k = min(len(m), max_pts)
            if matches is not None:
                matches[i, :k] = m[:k]
            p1[i, :k] = self.xy[s][m["queryIdx"][:k]]
            p2[i, :k, 0], p2[i, :k, 1] = kps[i]["x"][m["trainIdx"][:k]], kps[i]["y"][m["trainIdx"][:k]]
            npts[i] = len(m)
        return matches, p1, p2, npts
