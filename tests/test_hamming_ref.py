"""CPU: the two yardsticks of the matcher tests against each other.  tests/hamming_ref.py (unpacked bits, float32 matrix product,
argmin) and the oracle's orc_knn2_hamming (xor + popcount, packed keys) must name the same two neighbours at the same distances, in
both directions, at the sizes the GPU limit tests use: one row past the MFMA matcher's range, exactly on it, and the largest
row count the packed 16-bit train index holds, with planted ties in the first and last row and an all-zero / all-ones pair."""
import numpy as np
import pytest

import hamming_ref as hr


def _sets(n1, n2, seed):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    return d1, d2, hr.plant(d1, d2)


@pytest.mark.parametrize("n1,n2", [(16385, 16385), (16384, 16384), (65535, 257), (257, 65535)])
def test_reference_and_oracle_agree(orc, n1, n2):
    d1, d2, rows = _sets(n1, n2, 7 * n1 + n2)
    o12, o21 = orc.knn2_hamming(d1, d2)
    r12, r21 = hr.knn2_both(d1, d2)                               # one numpy pass per direction
    hr.assert_same(o12, r12, "12")
    hr.assert_same(o21, r21, "21")
    # the plants are really there: both neighbours at distance 0, the lower index first, the other one in the LAST row
    assert list(r12[0][rows["tie_q"]]) == [0, n2 - 1] and list(r12[1][rows["tie_q"]]) == [0.0, 0.0]
    assert list(r21[0][rows["tie_t"]]) == [0, n1 - 1] and list(r21[1][rows["tie_t"]]) == [0.0, 0.0]
    assert list(o12["trainIdx"][rows["tie_q"]]) == [0, n2 - 1]
    assert list(o21["trainIdx"][rows["tie_t"]]) == [0, n1 - 1]


def test_reference_on_hand_made_rows():
    """the reference itself on rows whose answer is known without any code: distance 256, a three-way tie, a single row"""
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    h = o.copy()
    h[:16] = 0                                                   # 128 bits set
    dq = np.stack([z, o, h])
    dt = np.stack([o, h, h, z, h])
    assert (hr.distances(dq, dt) == np.array([[256, 128, 128, 0, 128], [0, 128, 128, 256, 128], [128, 0, 0, 128, 0]], np.float32)).all()
    idx, dist = hr.knn2(dq, dt)
    assert idx.tolist() == [[3, 1], [0, 1], [1, 2]]
    assert dist.tolist() == [[0.0, 128.0], [0.0, 128.0], [0.0, 0.0]]
    idx, dist = hr.knn2(dq, dt[:1])
    assert idx.tolist() == [[0, -1], [0, -1], [0, -1]] and dist[:, 0].tolist() == [256.0, 0.0, 128.0]
    idx, dist = hr.knn2(dq, dt[:0])
    assert (idx == -1).all() and idx.shape == (3, 2)
    # chunking does not change the answer
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    b = rng.integers(0, 4, (700, 32), dtype=np.uint8)            # few distinct bits: many equal distances
    one = hr.knn2(a, b, chunk=300)
    for c in (1, 7, 64):
        got = hr.knn2(a, b, chunk=c)
        assert (got[0] == one[0]).all() and (got[1] == one[1]).all()
    # ... and equals a brute-force popcount
    pc = np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2)
    for q in range(300):
        order = np.lexsort((np.arange(700), pc[q]))[:2]
        assert one[0][q].tolist() == order.tolist() and one[1][q].tolist() == [float(pc[q][order[0]]), float(pc[q][order[1]])]
