"""Inputs of the loop-candidate tests (tests/test_kfdb_ref.py on the CPU, tests/test_kfdb_gpu.py and its stream twins on the device).  Not a test
module.  Descriptor sets with planted structure -- true correspondences a few bits apart, duplicates (the tie goes to the lower row), Hamming 0 and
256, and triples exactly on, one below and one above d0 == ratio * d1 -- and the planted out-and-back path of the recognition test."""
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
