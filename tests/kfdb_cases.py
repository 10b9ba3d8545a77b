"""Inputs of the loop-candidate tests (tests/test_kfdb_ref.py on the CPU, tests/test_kfdb_gpu.py and its stream twins on the device).  Not a test
module.  Descriptor sets with planted structure -- true correspondences a few bits apart, duplicates (the tie goes to the lower row), Hamming 0 and
256, and triples exactly on, one below and one above d0 == ratio * d1 --, the planted out-and-back path of the recognition test, and the builders
of tests/test_kfdb_limits_gpu.py: the tie and second-neighbour ladder, sets in which every distance ties, ring tables around 256 slots, long adds."""
import numpy as np

import kfdb_ref as kr

COUNTS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
REF_COUNTS = (1, 2, 31, 32, 33, 255, 256, 257, 300)
# (ratio, d1, the d0 exactly on ratio * d1): each goes in with d0 - 1 and d0 + 1; 0.8f * d1 is never an integer, so its pairs straddle it
BOUNDARIES = {0.5: (32, 16), 0.75: (32, 24), float(np.float32(0.8)): (40, 32)}


def flip(row, bits):
    """a copy of a 32-byte row with these bit positions inverted"""
    out = np.array(row, np.uint8)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def keypoints(rng, n):
    k = np.zeros(n, kr.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 320, n).astype(np.float32), rng.uniform(0, 240, n).astype(np.float32)
    k["size"], k["class_id"] = 31.0, -1
    return k


def planted_sets(seed, n_e, n_q, ratio=float(np.float32(0.8))):
    """(E, Q, plants): E (n_e, 32), Q (n_q, 32) uint8.  Rows of Q are rows of E a few bits apart (under a permutation), the rest random -- random
    rows are about 128 +- 8 bits from everything.  From 33 rows a side on, plants = {"on" | "below" | "above": entry row}: entry row r whose best
    query row is d0 away and whose second best is d1 away, d0 on / below / above ratio * d1 (for 0.8f: 32 is just below 0.8f * 40, 33 just above).
    Also planted where there is room: two identical query rows (the lower wins), two identical entry rows, an exact copy (Hamming 0) and a
    complement (Hamming 256)."""
    rng = np.random.default_rng(seed)
    E = rng.integers(0, 256, (n_e, 32), dtype=np.uint8)
    Q = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    m = min(n_e, n_q)
    perm = rng.permutation(n_q)[:m]
    for e in range(0, m, 2):                                   # every other entry has a true correspondence
        Q[perm[e]] = flip(E[e], rng.choice(256, int(rng.choice([0, 1, 2, 5, 20, 40])), replace=False))
    plants = {}
    if m >= 33:
        d1, on = BOUNDARIES.get(ratio, (40, 32))
        free = [int(perm[e]) for e in range(1, m, 2)]          # query rows that are still random
        for j, (name, d0) in enumerate((("on", on), ("below", on - 1), ("above", on + 1))):
            e, qa, qb = 1 + 2 * j, free[2 * j], free[2 * j + 1]
            bits = rng.permutation(256)
            Q[qa], Q[qb] = flip(E[e], bits[:d0]), flip(E[e], bits[d0:d0 + d1])
            plants[name] = e
        e = 7                                                  # INTENDED drops what REFERENCE_EFFECTIVE keeps: the query row has two near entries
        qa = free[6]
        bits = rng.permutation(256)
        Q[qa] = flip(E[e], bits[:4])
        E[9] = flip(Q[qa], bits[4:8])                          # (4 and 4: the tie goes to entry 7, and 4 > ratio * 4)
        plants["one_sided"] = e
        Q[free[7]] = Q[free[8]] = flip(E[11], bits[:3])        # identical query rows: entry 11 takes the lower one
        plants["dup_query"] = (11, min(free[7], free[8]))
        E[13] = E[15] = flip(Q[free[9]], bits[:2])             # identical entry rows: the query row takes entry 13, so 15 has no mutual match
        plants["dup_entry"] = (13, 15, free[9])
        Q[free[10]] = E[17]                                    # Hamming 0
        Q[free[11]] = ~E[19]                                   # Hamming 256 to entry 19
        plants["copy"], plants["complement"] = (17, free[10]), (19, free[11])
    return E, Q, plants


def rows(rng, sets, row_cap, counts=None):
    """padded rows for a call from descriptor sets: (kps (n, row_cap), desc (n, row_cap, 32), nkp (n,)); the entries beyond a set hold random
    data that must not matter; counts: what the call is told instead of the sets' sizes (hostile counts)"""
    n = len(sets)
    kps = keypoints(rng, n * row_cap).reshape(n, row_cap)
    desc = rng.integers(0, 256, (n, row_cap, 32), dtype=np.uint8)
    for i, d in enumerate(sets):
        c = min(len(d), row_cap)
        desc[i, :c] = d[:c]
    return kps, desc, np.asarray([len(d) for d in sets] if counts is None else counts, np.int32)


# ---- hand-made tables: an entry that holds copies of s rows of the query beside random rows scores exactly s --------------------------
BASE = np.random.default_rng(42).integers(0, 256, (24, 32), dtype=np.uint8)


def entry_scoring(s, seed):
    d = np.random.default_rng(seed).integers(0, 256, (24, 32), dtype=np.uint8)
    d[:s] = BASE[:s]
    return d


def table(entries, row_cap=24):
    """(kps, desc, nkp) rows of entries given as (score, seed) or None (a row with count 0)"""
    n = len(entries)
    kps, desc, nkp = np.zeros((n, row_cap), kr.KEYPOINT_DTYPE), np.zeros((n, row_cap, 32), np.uint8), np.zeros(n, np.int32)
    for i, e in enumerate(entries):
        if e is not None:
            desc[i], nkp[i] = entry_scoring(*e), 24
            kps[i]["x"], kps[i]["y"] = np.arange(24) + 100 * e[1], np.arange(24) + 0.5
    return kps, desc, nkp


def query_base(n=1):
    kps = np.zeros((n, 24), kr.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = np.arange(24) + 0.25, np.arange(24) + 0.75
    return kps, np.repeat(BASE[None], n, 0), np.full(n, 24, np.int32)


# ---- the tie and second-neighbour ladder (tests/test_kfdb_limits_gpu.py, CPU checks in tests/test_kfdb_ref.py) ------------------------------
# A row f of the FIXED set has its two nearest rows of the SWEPT set at chosen positions a < b.  The positions walk what the 2-NN merge of
# csrc/kfdb.hip depends on: the two row halves a lane pair holds (rows 4h + (r & 3) + 8 (r >> 2) of a 32-row tile: 0-3 | 4-7 | 8-11 ...), the
# pairwise v_med3 step (rows r, r + 1 of one lane), the tile edge (31 | 32, 63 | 64) and the masked tail tile (ns = 66: rows 64 and 65).
F8 = float(np.float32(0.8))
LADDER_NS = (64, 66)
LADDER_P = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 33, 35, 36, 63)
LADDER_TAIL_P = (64, 65)
# (rows of the fixed set, the index of f): the column, wave, column-group and chunk edges of the fixed side
LADDER_FIXED = ((33, 0), (40, 31), (33, 32), (64, 63), (65, 64), (256, 255), (258, 256), (258, 257))
LADDER_FIXED_BY_F = tuple((fi, nf) for nf, fi in LADDER_FIXED)
LADDER_ROW_CAP = 264
# ratios at the ends of what the contract takes as written: !(d0 > (double)(float)ratio * d1)
RATIO_ENDS = (1.0, 2.0, float("inf"), -1.0, float(np.float32(1e-45)))


def ladder_positions(ns):
    return LADDER_P + (LADDER_TAIL_P if ns > 64 else ())


def _ladder_pool(seed):
    """random rows for both sets, every one of them more than 64 bits from the planted f (the first row of the pool); the next seed if not"""
    while True:
        pool = np.random.default_rng(seed).integers(0, 256, (1 + 258 + 66, 32), dtype=np.uint8)
        if int(kr.hamming(pool[:1], pool[1:]).min()) > 64:
            return pool
        seed += 1


def ladder(ns, seed=2024):
    """the couples of one swept size: dicts of fixed (nf, 32), swept (ns, 32), f (index in fixed), a, b, kind, ratio and expect -- the swept row f
    must be matched with, or None where the ratio test must drop f.  Kinds per pair a < b of ladder_positions(ns):
      tie      swept[a] == swept[b] = f with 3 bits flipped, ratio 1.0: the lower row a
      ab       swept[a] 32 bits from f, swept[b] 39 bits (on other bits), ratio 0.8f: 32 > 0.8f * 39, so NO match -- a kernel that lost the
               second neighbour would see a random row (> 64 bits) there and keep it
      ba       the same with b first and a second
    and per ns two controls with the second neighbour at 40 bits (0.8f * 40 is just above 32): the match survives."""
    pool = _ladder_pool(seed)
    f_row, rnd_f, rnd_s = pool[0], pool[1:259], pool[259:259 + ns]
    bits = np.random.default_rng(seed + 1).permutation(256)
    near, first, second, control = flip(f_row, bits[:3]), flip(f_row, bits[:32]), flip(f_row, bits[32:71]), flip(f_row, bits[32:72])
    out = []

    def couple(kind, a, b, ratio, rows_ab, expect):
        nf, fi = LADDER_FIXED[len(out) % len(LADDER_FIXED)]
        fixed, swept = rnd_f[:nf].copy(), rnd_s.copy()
        fixed[fi], swept[a], swept[b] = f_row, rows_ab[0], rows_ab[1]
        out.append(dict(fixed=fixed, swept=swept, f=fi, a=a, b=b, kind=kind, ratio=ratio, expect=expect))
    P = ladder_positions(ns)
    for i, a in enumerate(P):
        for b in P[i + 1:]:
            couple("tie", a, b, 1.0, (near, near), a)
            couple("ab", a, b, F8, (first, second), None)
            couple("ba", a, b, F8, (second, first), None)
    couple("control_ab", 3, 4, F8, (first, control), 3)
    couple("control_ba", 31, P[-1], F8, (control, first), P[-1])
    return out


def ladder_sets(c, planted_is_entry):
    """(entry set, query set) of a ladder couple: the set that holds f as the entry (direction 1 carries the plant) or as the query (direction 2
    and the mutual test carry it)"""
    return (c["fixed"], c["swept"]) if planted_is_entry else (c["swept"], c["fixed"])


def ladder_match_of_f(c, planted_is_entry, m):
    """the swept row the list m matches f with, or None"""
    mine, other = ("queryIdx", "trainIdx") if planted_is_entry else ("trainIdx", "queryIdx")
    hit = m[other][m[mine] == c["f"]]
    return int(hit[0]) if len(hit) else None


# deliberately wrong 2-NN keys: each must change the list of at least one ladder couple (tests/test_kfdb_ref.py)
def _sorted_keys(fixed, swept):
    return np.sort((kr.hamming(fixed, swept).astype(np.int64) << 16) | np.arange(len(swept), dtype=np.int64)[None, :], axis=1)


def _pack(keys, nf, take=(0, 1)):
    out = np.full((nf, 2), kr.NONE, np.uint32)
    for j, t in enumerate(take):
        if t < keys.shape[1]:
            out[:, j] = keys[:, t].astype(np.uint32)
    return out


def wrong_knn2_tie_to_the_higher_row(fixed, swept):
    ns = len(swept)
    k = np.sort((kr.hamming(fixed, swept).astype(np.int64) << 16) | (ns - 1 - np.arange(ns, dtype=np.int64))[None, :], axis=1)
    return _pack((k & ~np.int64(0xFFFF)) | (ns - 1 - (k & 0xFFFF)), len(fixed))


def wrong_knn2_second_is_the_third(fixed, swept):
    return _pack(_sorted_keys(fixed, swept), len(fixed), (0, 2))


def wrong_knn2_halves_merged_by_their_seconds(fixed, swept):
    """the two row halves of a lane pair (bit 2 of the row) keep their own two best; merged as (min(a0, o0), min(a1, o1)) -- the larger of the two
    firsts is forgotten"""
    big = np.int64(kr.NONE)
    keys = (kr.hamming(fixed, swept).astype(np.int64) << 16) | np.arange(len(swept), dtype=np.int64)[None, :]
    half = ((np.arange(len(swept)) >> 2) & 1).astype(bool)
    best = []
    for h in (False, True):
        k = np.sort(np.where((half == h)[None, :], keys, big), axis=1)
        best.append(np.concatenate([k, np.full((len(fixed), 2), big)], 1)[:, :2])
    return np.stack([np.minimum(best[0][:, 0], best[1][:, 0]), np.minimum(best[0][:, 1], best[1][:, 1])], 1).astype(np.uint32)


def wrong_keys(knn2):
    """a couple's keys_fn from a wrong one-direction 2-NN"""
    return lambda e, q: (knn2(e, q), knn2(q, e))


ALL_EQUAL_COUNTS = (2, 33, 64, 257)


def all_equal_sets():
    """(entries, queries): sets in which every distance ties.  Entries: n copies of one row, then n all-zero rows; queries: m copies of the same
    row (every distance 0), then m all-ones rows (every distance to the zero rows 256); n and m over ALL_EQUAL_COUNTS"""
    row = np.random.default_rng(31).integers(0, 256, 32, dtype=np.uint8)
    rep = lambda r, n: np.repeat(np.asarray(r, np.uint8)[None], n, 0)
    entries = [rep(row, n) for n in ALL_EQUAL_COUNTS] + [np.zeros((n, 32), np.uint8) for n in ALL_EQUAL_COUNTS]
    queries = [rep(row, m) for m in ALL_EQUAL_COUNTS] + [np.full((m, 32), 255, np.uint8) for m in ALL_EQUAL_COUNTS]
    return entries, queries


# ---- rings above 256 slots: what k_loop_topk's 256-strided loops and its reduction trees depend on ------------------------------------------
RING_CAPS = (255, 256, 257, 513)
# slots that hold the SAME (score, id): e and e + 1, e and e + 255, e and e + 256 (one thread of k_loop_topk) -- where the ring has them.  Two of
# them put the LOWER slot on the far side of a step of the reduction tree, where only the tree's own slot comparison keeps it in front: 255 and 256
# (threads 255 and 0) and 130 and 258 (threads 130 and 2, which meet in the first step)
RING_GROUPS = {255: ((10, 11),), 256: ((10, 11), (0, 255)), 257: ((10, 11), (0, 255, 256)), 513: ((10, 11), (20, 275), (1, 257), (130, 258))}
RING_MIN_SCORES = {6: 15, 5: 16, 4: 17}                     # min_score: how many entries are at or above it (topk is 16)


def ring_table(entry_cap):
    """(kps, desc, nkp, ids) of entry_cap rows for an empty ring: background entries of score 1 ... 3 with id 1000 + slot; the groups of
    RING_GROUPS at scores 9, 8, 7 (6) with ids 5, 6, 7 (8); slots 30 and 40 at score 6 with ids 900 and 800 (the opposite order); entries of score 12 with
    falling ids from slot 50 on until 15 entries score 6 or more; slot 70 scores 5 and slot 71 scores 4"""
    spec = {s: (1 + s % 3, 1000 + s) for s in range(entry_cap)}
    for g, slots in enumerate(RING_GROUPS[entry_cap]):
        for s in slots:
            spec[s] = (9 - g, 5 + g)
    spec[30], spec[40] = (6, 900), (6, 800)
    s = 50
    while sum(sc >= 6 for sc, _ in spec.values()) < 15:
        spec[s] = (12, 2000 - s)
        s += 1
    assert s <= 70
    spec[70], spec[71] = (5, 950), (4, 951)
    for ms, count in RING_MIN_SCORES.items():
        assert sum(sc >= ms for sc, _ in spec.values()) == count
    kps, desc, nkp = table([(spec[s][0], 1000 + s) for s in range(entry_cap)])         # (seed 42 would be BASE itself)
    return kps, desc, nkp, np.array([spec[s][1] for s in range(entry_cap)], np.int32)


def ring_queries(entry_cap):
    """three queries, the middle one skipped; the last sees the groups and the lower half of the background only (with min_gap 0)"""
    qk, qd, qn = query_base(3)
    qn[1] = 0
    return qk, qd, qn, np.array([1000000, 1000000, 1000 + entry_cap // 2], np.int32)


def scored_rows(n, kp=8, seed=65536):
    """(kps, desc, nkp, ids) of n rows of kp keypoints for the long adds: row i holds i % (kp + 1) rows of BASE beside random ones and scores about
    that against BASE[:kp]; counts 0 ... kp with a few hostile ones; id = i, every 97th negative (an empty entry)"""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n, kp, 32), dtype=np.uint8)
    s = np.arange(n) % (kp + 1)
    for j in range(kp):
        desc[s > j, j] = BASE[j]
    kps = np.zeros((n, kp), kr.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = (np.arange(n)[:, None] % 4096) + 0.25 * np.arange(kp)[None, :], np.arange(kp)[None, :] + 0.5
    nkp = rng.integers(0, kp + 1, n).astype(np.int32)
    nkp[5::13] = kp
    nkp[7::1001], nkp[8::1001], nkp[9::1001] = -1, 2 ** 31 - 1, -2 ** 31
    ids = np.arange(n, dtype=np.int32)
    ids[96::97] = -1
    return kps, desc, nkp, ids


# ---- the planted out-and-back path (tests/test_kfdb_ref.py has the figures) ------------------------------------------------------------
PATH_W, PATH_H, PATH_N = 320, 240, 16
PATH_OUT = [(40 + 12 * i, 60 + 8 * i) for i in range(PATH_N)]
PATH_BACK = [(x + 3, y + 2) for x, y in reversed(PATH_OUT)]
PATH_ELSEWHERE = [(600, 100), (700, 500), (100, 700), (500, 650), (650, 300), (350, 450)]


def path_frames(canvas):
    """(out frames, back frames, crops from elsewhere): 320 x 240 crops of the canvas plus noise in -2 ... 2 from default_rng(7), drawn out-frames
    first, then back-frames in path order, then the crops from elsewhere"""
    rng = np.random.default_rng(7)

    def crop(o):
        x, y = o
        f = canvas[y:y + PATH_H, x:x + PATH_W].astype(np.int16) + rng.integers(-2, 3, (PATH_H, PATH_W)).astype(np.int16)
        return np.clip(f, 0, 255).astype(np.uint8)
    return [crop(o) for o in PATH_OUT], [crop(o) for o in PATH_BACK], [crop(o) for o in PATH_ELSEWHERE]


def path_params(p):
    """the detector / matcher parameters of the path: defaults, INTENDED, the frame size"""
    p.sym_mode, p.w_size, p.h_size = 1, PATH_W, PATH_H
    return p
