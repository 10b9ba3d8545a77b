"""Independent numpy reference of the brute-force Hamming 2-NN (TEST INFRASTRUCTURE ONLY).  It shares nothing with oracle/match.cpp:
no xor, no popcount, no packed key.  The descriptors are unpacked into 0 / 1 floats and the distance is |a| + |b| - 2 a.b^T with a
float32 matrix product -- exact, because every partial sum is an integer of at most 256 (far below 2^24).  The two nearest are the
two smallest (distance, train index) pairs, so the lower index wins a tie: the order of cv::batchDistance."""
import numpy as np


def _bits(d):
    d = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
    return np.unpackbits(d, axis=1).astype(np.float32)


def distances(dq, dt):
    """the full (len(dq), len(dt)) matrix of Hamming distances, float32 (small inputs only)"""
    a, b = _bits(dq), _bits(dt)
    return a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)


def knn2(dq, dt, chunk=None):
    """(trainIdx, distance): int32 and float32 arrays of shape (len(dq), 2); a missing neighbour is (-1, inf).  Chunked over query
    rows (by default so that one block of distances holds about 16 M entries)."""
    a, b = _bits(dq), _bits(dt)
    nq, nt = len(a), len(b)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), np.inf, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    if chunk is None:
        chunk = max(64, min(2048, (1 << 24) // nt))
    nb = b.sum(1)
    bt = np.ascontiguousarray(b.T)
    for q0 in range(0, nq, chunk):
        aq = a[q0:q0 + chunk]
        d = aq.sum(1)[:, None] + nb[None, :] - 2.0 * (aq @ bt)
        # argmin returns the FIRST minimum of a row: the lowest train index among equal distances
        rows = np.arange(len(aq))
        i0 = d.argmin(1)
        idx[q0:q0 + chunk, 0] = i0
        dist[q0:q0 + chunk, 0] = d[rows, i0]
        if nt > 1:
            d[rows, i0] = np.inf
            i1 = d.argmin(1)
            idx[q0:q0 + chunk, 1] = i1
            dist[q0:q0 + chunk, 1] = d[rows, i1]
    return idx, dist


def knn2_both(d1, d2, chunk=None):
    """both directions, like vis_bf_knn2_hamming_host: ((idx12, dist12), (idx21, dist21))"""
    return knn2(d1, d2, chunk), knn2(d2, d1, chunk)


def assert_same(dm, ref, what=""):
    """dm: an (n, 2) DMatch array of the library or the oracle; ref: knn2's (idx, dist).  A missing neighbour is trainIdx -1 there
    (its distance field is not compared)."""
    idx, dist = ref
    assert dm.shape == idx.shape, (what, dm.shape, idx.shape)
    assert (dm["queryIdx"] == np.arange(len(idx), dtype=np.int32)[:, None]).all(), what
    assert (dm["trainIdx"] == idx).all(), (what, np.argwhere(dm["trainIdx"] != idx)[:4])
    have = idx >= 0
    assert (dm["distance"][have] == dist[have]).all(), (what, np.argwhere(have & (dm["distance"] != dist))[:4])


def plant(d1, d2):
    """The ties and extremes of the limit tests, written into random descriptor sets in place (both sets need >= 9 rows).  Returns
    the planted row numbers: `tie_q` of d1 equals rows 0 and n2-1 of d2 (two neighbours at distance 0, as far apart as the set
    allows), `tie_t` of d2 equals rows 0 and n1-1 of d1 (the same in the other direction), `ones_q` of d1 is all ones and `zero_t`
    of d2 all zeros (Hamming 256 between them)."""
    n1, n2 = len(d1), len(d2)
    assert n1 >= 9 and n2 >= 9
    tie_q, ones_q = 5, 7
    tie_t, zero_t = 6, 3
    d2[n2 - 1] = d2[0]
    d1[tie_q] = d2[0]
    d1[n1 - 1] = d1[0]
    d2[tie_t] = d1[0]
    d1[ones_q] = 255
    d2[zero_t] = 0
    return dict(tie_q=tie_q, tie_t=tie_t, ones_q=ones_q, zero_t=zero_t)
