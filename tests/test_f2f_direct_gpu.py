"""vis_f2f_ransac with its sample indices taken as given (k_f2f_batch<.., DIRECT>, one pair), against the oracle (orc.f2f_ransac) with the
project's tolerance for F2FRansac (tests/test_pose_gpu.py): equal count_max, |dt| <= 1e-6.

The public contract allows sample_idx == m - 1, which rand() % (m - 1) never produces and no other test draws: here the indices come from
[0, m), every case contains m - 1 (asserted), and in some cases the winning sample does (asserted on the CPU, with the oracle).  Shapes:
m = 2, 3, F2F_TILE and F2F_TILE + 1 (one tile / two tiles of normals: where the kernel's 256 x 4 and 512 x 2 shapes switch) times
iters = 1, 256, 257, 1024, 1025 (the ends of a workgroup's lanes and of one round of NT x IPL = 1024 iterations of either shape).
The seeds were chosen on the CPU: the smallest seed whose indices contain m - 1."""
import numpy as np
import pytest

import f2f_ref as fr

TILE = 512                                                         # VIS_F2F_TILE (asserted against the library below)
MS = [2, 3, TILE, TILE + 1]
ITERS = [1, 256, 257, 1024, 1025]
SCALE = 0.37
# (m, iters) -> seed of the index table where seed 0 does not draw m - 1 (two draws out of 512 need a search: 588 is the first)
SEEDS = {(TILE, 1): 588, (TILE + 1, 1): 588, (TILE, 256): 1, (TILE, 257): 1, (TILE + 1, 256): 1, (TILE + 1, 257): 1}
_cache = {}


def _case(vislam, orc, m, iters):
    """inputs and the oracle's answer of one case, computed once: (ka, kb, rot, idx, oracle t, oracle count, winning iteration or -1)"""
    if (m, iters) not in _cache:
        p = vislam.default_params()
        a, b, rot, _ = fr.pair_inputs(m, 400 + m, 0.2, 0.5)
        ka, kb = fr.keypoints(vislam.KEYPOINT_DTYPE, a), fr.keypoints(vislam.KEYPOINT_DTYPE, b)
        idx = np.random.default_rng(SEEDS.get((m, iters), 0)).integers(0, m, (iters, 2)).astype(np.int32)
        ot, oc = orc.f2f_ransac(p, ka, kb, rot, idx, SCALE)
        # the winner: the first iteration whose own count is the largest (`if (count > countMax)` in order), by the oracle one iteration at a time
        counts = [orc.f2f_ransac(p, ka, kb, rot, idx[j:j + 1], SCALE)[1] for j in range(iters)]
        win = int(np.argmax(counts)) if oc > 0 else -1
        assert win < 0 or counts[win] == oc
        _cache[(m, iters)] = (ka, kb, rot, idx, ot, oc, win)
    return _cache[(m, iters)]


def test_cases_reach_the_last_point(vislam, orc):
    """CPU: every index table contains m - 1, and the winning sample of some case does -- also of a row longer than two points"""
    assert vislam.F2F_TILE == TILE
    winners = []
    for m in MS:
        for iters in ITERS:
            _, _, _, idx, _, oc, win = _case(vislam, orc, m, iters)
            assert idx.min() >= 0 and idx.max() == m - 1, (m, iters)
            if win >= 0 and (idx[win] == m - 1).any():
                winners.append((m, iters))
    print("cases whose winning sample holds m - 1:", winners)
    assert any(m == 2 for m, _ in winners) and any(m > 2 for m, _ in winners), winners


@pytest.mark.gpu
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("m", MS)
def test_direct_indices_against_the_oracle(vislam, orc, ctx, m, iters):
    ctx.set_params(vislam.default_params())
    ka, kb, rot, idx, ot, oc, _ = _case(vislam, orc, m, iters)
    assert (idx == m - 1).any()
    got, cg = ctx.f2f_ransac(ka, kb, rot, idx, SCALE)
    print(f"m {m} iters {iters}: count {cg} (oracle {oc}), max |dt| {np.abs(got - ot).max():.3g}")
    assert cg == oc, (cg, oc)
    assert np.abs(got - ot).max() <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("m", [3, TILE + 1])
def test_all_samples_degenerate_under_a_negative_scale(vislam, orc, ctx, m):
    """i1 == i2 throughout (m - 1 among them): every cross product is zero, nothing wins.  The oracle returns scale * 0.f = -0.0 three times
    and count 0 (checked on the CPU before this assertion was written); the library multiplies its zero record by the scale the same way."""
    p = vislam.default_params()
    ctx.set_params(p)
    a, b, rot, _ = fr.pair_inputs(m, 400 + m, 0.2, 0.5)
    ka, kb = fr.keypoints(vislam.KEYPOINT_DTYPE, a), fr.keypoints(vislam.KEYPOINT_DTYPE, b)
    idx = np.repeat(np.arange(257, dtype=np.int32)[::-1] % m, 2).reshape(-1, 2)
    idx[0] = m - 1
    assert (idx[:, 0] == idx[:, 1]).all() and (idx == m - 1).any()
    ot, oc = orc.f2f_ransac(p, ka, kb, rot, idx, -SCALE)
    assert oc == 0 and ot.tobytes() == np.full(3, -0.0, np.float32).tobytes()
    got, cg = ctx.f2f_ransac(ka, kb, rot, idx, -SCALE)
    assert cg == 0 and (got == 0).all()
    assert got.tobytes() == ot.tobytes()
