"""GPU parity AT the size limits DESIGN.md section 7 states (bit-exact vs the oracle unless a tolerance is given):
  matcher   16384 rows per side = the last size of the MFMA kernel (tile 511, age 8176: the 13 low key bits are full); above it the
            popcount kernel k_knn2 in both of its launch shapes, every residue of its unrolled loop, train indices up to 65534;
            the two kernels against each other on the same rows; 65536 rows refused
  RANSAC    64 | 65 (sample table | RNG replay on the device), 256 | 257 (the two forms of k_hyp_score), 1024 | 1025 and the row counts
            that do not divide evenly over their rounds (5 = 3 + 2, 13 = 4 + 3 + 3 + 3, 17 = 4 + 4 + 3 + 3 + 3), 8192 = the most a problem
            may hold, 8193 refused; the undecided list of k_hyp_score (vis_pose_result.undecided_max) on its list path and beyond its
            4096 entries, where the sub-item is recounted in double precision
  detector  image side 4095 = the most the packed FAST candidate (score << 24 | y << 12 | x) holds; 4096 refused.
Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest

import hamming_ref as hr
from test_pose_gpu import TOL, _cmpE, two_view

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4


# ------------------------------------------------------------------------------------------------ matcher
def _sets(n1, n2, seed, plant=True):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    rows = hr.plant(d1, d2) if plant and min(n1, n2) >= 9 else None
    return d1, d2, rows


def _plant_far(d1, d2):
    """row 11 of each set = the LAST BUT ONE row of the other: its first neighbour is that row (n - 2), alone at distance 0"""
    d1[11] = d2[len(d2) - 2]
    d2[11] = d1[len(d1) - 2]


def _plant_tail(fixed, swept, base=20):
    """rows base, base + 1 ... of `fixed` = the rows of `swept` beyond its last multiple of eight (the tail of k_knn2's unrolled loop):
    each of those rows is then somebody's first neighbour.  Returns them."""
    n = len(swept)
    tail = list(range(n & ~7, n))
    assert base + len(tail) < len(fixed) - 2 and (n & ~7) > base + 8
    for j, r in enumerate(tail):
        fixed[base + j] = swept[r]
    return tail


def _parity(ctx, orc, d1, d2, with_ref):
    g12, g21 = ctx.bf_knn2_hamming_host(d1, d2)
    o12, o21 = orc.knn2_hamming(d1, d2)
    assert g12.tobytes() == o12.tobytes(), np.argwhere(g12["trainIdx"] != o12["trainIdx"])[:4]
    assert g21.tobytes() == o21.tobytes(), np.argwhere(g21["trainIdx"] != o21["trainIdx"])[:4]
    if with_ref:
        r12, r21 = hr.knn2_both(d1, d2)
        hr.assert_same(g12, r12, "12")
        hr.assert_same(g21, r21, "21")
    return g12, g21


def _assert_plants(g12, g21, rows, n1, n2):
    """what hamming_ref.plant() wrote really comes back: two neighbours at distance 0, first and last row, the lower index first"""
    for g, q, last in ((g12, rows["tie_q"], n2 - 1), (g21, rows["tie_t"], n1 - 1)):
        assert g["trainIdx"][q].tolist() == [0, last] and g["distance"][q].tolist() == [0.0, 0.0], (q, g[q])


@pytest.mark.parametrize("n1,n2", [(16384, 16384), (16383, 16353), (16384, 40), (40, 16384)])
def test_mfma_matcher_full_key_range(vislam, orc, ctx, n1, n2):
    """k_knn_mfma where its running keys are oldest: a neighbour in row 0 has been aged 511 times (16 * 511 = 8176 of the 8191 the low
    bits hold) when the last tile is merged, and a neighbour in the last tile restores to tile index 511.  16353 rows end in a last
    tile of ONE row (the masked merge, at tile 511)."""
    d1, d2, rows = _sets(n1, n2, 1000 + n1 + n2)
    _plant_far(d1, d2)
    g12, g21 = _parity(ctx, orc, d1, d2, with_ref=min(n1, n2) == 40)
    _assert_plants(g12, g21, rows, n1, n2)
    assert g12["trainIdx"][11, 0] == n2 - 2 and g21["trainIdx"][11, 0] == n1 - 2
    assert g12["distance"][11, 0] == 0 and g21["distance"][11, 0] == 0


@pytest.mark.parametrize("ns", [1, 33])
@pytest.mark.parametrize("zeros", [False, True])
def test_mfma_matcher_one_row_and_one_row_past_a_tile(vislam, orc, ctx, ns, zeros):
    """16384 fixed rows against a swept set of 1 row (no second neighbour: trainIdx -1, as in test_knn2_empty) and of 33 rows (a second
    tile of one row).  With an all-zero swept set an all-ones fixed row has its only neighbours at Hamming 256, the top of the key's
    distance field, and every fixed row sees 33 equal distances: rows 0 and 1 win."""
    rng = np.random.default_rng(40 + ns)
    d1 = rng.integers(0, 256, (16384, 32), dtype=np.uint8)
    d1[7] = 255
    d1[16383] = 255
    d2 = np.zeros((ns, 32), np.uint8) if zeros else rng.integers(0, 256, (ns, 32), dtype=np.uint8)
    g12, g21 = _parity(ctx, orc, d1, d2, with_ref=True)
    if ns == 1:
        assert (g12["trainIdx"][:, 0] == 0).all() and (g12["trainIdx"][:, 1] == -1).all()
    if zeros:
        for q in (7, 16383):
            assert g12["distance"][q, 0] == 256.0 and g12["trainIdx"][q, 0] == 0
            if ns > 1:
                assert g12["distance"][q, 1] == 256.0 and g12["trainIdx"][q, 1] == 1
        if ns > 1:
            assert (g12["trainIdx"] == [0, 1]).all()
        # the other direction: every all-zero row finds the fixed rows with the fewest set bits, the same two for all of them
        assert (g21["trainIdx"] == g21["trainIdx"][0]).all()


@pytest.mark.parametrize("n1,n2", [(16385, 16385), (65535, 4099), (4099, 65535), (65281, 9)])
def test_popcount_matcher_both_launch_shapes(vislam, orc, ctx, n1, n2):
    """k_knn2 runs above 16384 rows per side: 16385 x 16385 in 64-thread blocks (ceil(16385 / 256) * 2 = 130 < 512), 65281 rows and
    more in 256-thread blocks (ceil(65281 / 256) * 2 = 512).  65535 rows: the packed 16-bit train index reaches 65534 (a planted tie
    between rows 0 and 65534) and 65533 (planted alone at distance 0).  (65535 x 65535 would take the oracle about 20 s; the two
    65535 x 4099 shapes sweep and fix the same 65535 rows.)"""
    d1, d2, rows = _sets(n1, n2, 2000 + n1 + n2)
    if min(n1, n2) > 13:
        _plant_far(d1, d2)
    g12, g21 = _parity(ctx, orc, d1, d2, with_ref=n1 != n2)
    _assert_plants(g12, g21, rows, n1, n2)
    if min(n1, n2) > 13:
        assert g12["trainIdx"][11, 0] == n2 - 2 and g21["trainIdx"][11, 0] == n1 - 2
    if n2 == 65535:
        assert g12["trainIdx"][rows["tie_q"]].tolist() == [0, 65534] and g12["trainIdx"][11, 0] == 65533
    if n1 == 65535:
        assert g21["trainIdx"][rows["tie_t"]].tolist() == [0, 65534] and g21["trainIdx"][11, 0] == 65533


@pytest.mark.parametrize("n1,n2", [(n, 16385) for n in range(9, 17)] + [(16385, 16386), (16387, 16388), (16389, 16390), (16391, 16392)])
def test_popcount_matcher_every_tail_length(vislam, orc, ctx, n1, n2):
    """k_knn2 sweeps eight rows per step and the rest one by one: swept sets of 9 ... 16 and of 16385 ... 16392 rows are every residue
    mod 8, small and large (both directions of one call sweep one set each; the larger side, above 16384, selects this kernel).  Every
    row of a tail is planted as somebody's exact neighbour, so a tail row that is skipped changes the answer."""
    d1, d2, rows = _sets(n1, n2, 3000 + n1 + n2)
    tail1 = _plant_tail(d2, d1) if n1 > 64 else list(range(n1 & ~7, n1))   # (a small d1: its tail row n1 - 1 is the planted tie, and
    tail2 = _plant_tail(d1, d2) if n1 > 64 else list(range(n2 & ~7, n2))   #  row 16384 of d2 is the other one)
    g12, g21 = _parity(ctx, orc, d1, d2, with_ref=n1 < 64)
    _assert_plants(g12, g21, rows, n1, n2)
    if n1 > 64:
        for g, tail in ((g21, tail1), (g12, tail2)):              # (a tail row may share its distance 0 with a planted tie: either place)
            for j, r in enumerate(tail):
                k = g["trainIdx"][20 + j].tolist()
                assert r in k and g["distance"][20 + j][k.index(r)] == 0, (r, g[20 + j])
    else:
        # every row of the small set is within the first two neighbours of some of the 16385 rows on the other side
        assert set(range(n1)) <= set(g21["trainIdx"].reshape(-1).tolist())
        assert tail2 == [16384] and g12["trainIdx"][rows["tie_q"], 1] == 16384


def test_mfma_and_popcount_matchers_agree(vislam, orc, ctx):
    """match.hip: "Results are bit-identical to k_knn2".  The same 16384 x 16384 rows once as they are (MFMA kernel) and once with one
    more row per side (16385: popcount kernel).  The added rows are 64 bits further from every row than anything else (all rows end in
    64 zero bits, the added ones in 64 one bits), so they are nobody's neighbour -- asserted on the oracle -- and the first 16384
    result rows of both runs must be the same bytes."""
    n = 16384
    rng = np.random.default_rng(77)
    d1 = rng.integers(0, 256, (n + 1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n + 1, 32), dtype=np.uint8)
    d1[:, 24:] = 0
    d2[:, 24:] = 0
    d2[n - 1] = d2[0]; d1[5] = d2[0]                              # ties between the first and the last row, both directions
    d1[n - 1] = d1[0]; d2[6] = d1[0]
    d1[9] = 0; d2[3] = 0
    d1[n, 24:] = 255
    d2[n, 24:] = 255
    a12, a21 = ctx.bf_knn2_hamming_host(d1[:n], d2[:n])           # kcap 16384: k_knn_mfma
    b12, b21 = ctx.bf_knn2_hamming_host(d1, d2)                   # kcap 16385: k_knn2
    o12, o21 = orc.knn2_hamming(d1, d2)
    assert (o12["trainIdx"][:n] != n).all() and (o21["trainIdx"][:n] != n).all()      # the added rows are nobody's neighbour
    assert b12.tobytes() == o12.tobytes() and b21.tobytes() == o21.tobytes()
    assert a12.tobytes() == b12[:n].tobytes() and a21.tobytes() == b21[:n].tobytes()
    assert a12["trainIdx"][5].tolist() == [0, n - 1] and a21["trainIdx"][6].tolist() == [0, n - 1]


def test_slots_above_16384_keypoints(vislam, orc, canvas):
    """keypoint_capacity = 16385: the slot matcher runs the popcount kernel with a few hundred real descriptors in rows of 16385 and
    must equal the oracle and a default-capacity context (MFMA kernel).  The match filters sort at most 16384 keypoints per frame in
    LDS: vis_good_matches and a vis_batch_run with the match stage refuse that capacity with VIS_E_CAPACITY and say so."""
    import torch
    p = vislam.default_params()
    frames = [vislam.synth_frame(canvas, t, 752, 480) for t in (3, 4)]
    small = vislam.Context(0, p)
    ks = [small.orb_detect_compute(f, slot=s) for s, f in enumerate(frames)]
    s12, s21 = small.bf_knn2_hamming(0, 1, len(ks[0][0]), len(ks[1][0]))
    small.close()
    p.keypoint_capacity = 16385
    big = vislam.Context(0, p)
    kb = [big.orb_detect_compute(f, slot=s) for s, f in enumerate(frames)]
    for (k, d), (k2, d2) in zip(ks, kb):
        assert len(k) > 300 and k.tobytes() == k2.tobytes() and d.tobytes() == d2.tobytes()
    g12, g21 = big.bf_knn2_hamming(0, 1, len(kb[0][0]), len(kb[1][0]))
    o12, o21 = orc.knn2_hamming(kb[0][1], kb[1][1])
    print(f"slot matcher at capacity 16385: {len(kb[0][0])} x {len(kb[1][0])} keypoints")
    assert g12.tobytes() == o12.tobytes() and g21.tobytes() == o21.tobytes()
    assert g12.tobytes() == s12.tobytes() and g21.tobytes() == s21.tobytes()
    with pytest.raises(vislam.VisError) as ei:
        big.good_matches(0, 1)
    print("vis_good_matches:", ei.value)
    assert ei.value.code == E_CAPACITY and "16385" in str(ei.value)
    dev = torch.from_numpy(np.stack(frames)).cuda()
    big.batch_plan(752, 480, 752, 2)
    with pytest.raises(vislam.VisError) as ei:
        big.batch_run(dev.data_ptr(), 2, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
        big.batch_sync()
    print("vis_batch_run:", ei.value)
    assert ei.value.code == E_CAPACITY and "16385" in str(ei.value)
    big.batch_sync()
    # the same plan still detects (the refusal left nothing half done)
    big.batch_run(dev.data_ptr(), 2, vislam.STAGE_DETECT)
    big.batch_sync()
    assert big.batch_status() == 0
    k0, d0 = big.batch_keypoints(0)
    assert k0.tobytes() == ks[0][0].tobytes() and d0.tobytes() == ks[0][1].tobytes()
    big.close()


def test_65536_descriptors_are_refused(vislam, ctx):
    big, one = np.zeros((65536, 32), np.uint8), np.zeros((1, 32), np.uint8)
    for a, b in ((big, one), (one, big)):
        with pytest.raises(vislam.VisError) as ei:
            ctx.bf_knn2_hamming_host(a, b)
        assert ei.value.code == E_INVALID


# ------------------------------------------------------------------------------------------------ RANSAC
def _ransac_case(vislam, orc, m, thr, fx, noise, adaptive, iters=400):
    """the generator of test_pose_gpu.test_many_correspondences_single_precision_scoring on a context of its own (the undecided-list
    mark of vis_debug_counters is a maximum over the context's calls).  Returns the oracle's inlier count and iterations and the mark."""
    p = vislam.default_params()
    p.fx = p.fy = fx
    p.ransac_threshold, p.ransac_adaptive, p.ransac_max_iters = thr, adaptive, iters
    rng = np.random.default_rng(m + int(10 * thr))
    x1, x2, R, t = two_view(m, 100 + m, 0.35, 0.0)
    x2 = (x2 + rng.normal(0, noise, x2.shape)).astype(np.float32)
    c = vislam.Context(0, p)
    try:
        assert c.undecided_max() == 0
        E, mask, ninl, it = c.essential_ransac(x1, x2)
        mark = c.undecided_max()
        E2, mask2, ninl2, it2 = c.essential_ransac(x1, x2)        # run to run: the same answer and the same mark (a maximum is order independent)
        assert (ninl2, it2) == (ninl, it) and (mask2 == mask).all() and E2.tobytes() == E.tobytes() and c.undecided_max() == mark
        oE, omask, oninl, oiters = orc.essential_ransac(p, x1, x2)
        print(f"ransac m={m} thr={thr} fx={fx} noise={noise} adaptive={adaptive}: oracle {oninl} inliers, {oiters} iterations; "
              f"gpu {ninl}, {it}; undecided_max {mark}; |dE| {_cmpE(E, oE):.3g}")
        assert (ninl, it) == (oninl, oiters)
        assert (mask == omask).all()
        assert _cmpE(E, oE) <= TOL
        Rg, tg, ng = c.recover_pose(oE, x1, x2)
        Ro, to, no = orc.recover_pose(p, oE, x1, x2)
        assert ng == no
        assert np.abs(Rg - Ro).max() <= TOL and np.abs(tg - to).max() <= TOL
        assert c.undecided_max() == mark                          # (vis_recover_pose scores nothing)
    finally:
        c.close()
    return oninl, oiters, mark


@pytest.mark.parametrize("m,adaptive", [(m, 1) for m in (64, 65, 255, 256, 257, 1024, 1025, 3100, 4096, 4097, 8191, 8192)] +
                         [(m, 0) for m in (65, 257, 1025, 8192)])
def test_ransac_size_boundaries(vislam, orc, m, adaptive):
    """Both sides of every size at which the pose stage changes form.  64 | 65: samples from the host-built table | replayed on the device;
    256 | 257: k_hyp_score's few-points form | rows of 256 points; 1024 | 1025: one round of 4 rows | two rounds of 3 + 2; 3100 and 4097:
    13 = 4 + 3 + 3 + 3 and 17 = 4 + 4 + 3 + 3 + 3 rows; 8192: the largest problem.  Threshold-sized noise, 35 % outliers: the oracle
    keeps 0.43 ... 0.55 of the points at every size (measured on the CPU oracle), so 0.3 m < inliers < 0.7 m rules out a degenerate case
    passing as parity."""
    oninl, oiters, mark = _ransac_case(vislam, orc, m, 1.0, 458.654, 1.0, adaptive)
    assert 0.3 * m < oninl < 0.7 * m
    assert oiters == 400 if not adaptive else oiters <= 400       # (the adaptive runs stop after 196 ... 356 iterations, 4097 points run all 400)
    assert 0 <= mark <= 4096
    if m <= 256:
        assert mark == 0                                          # the few-points form never lists anything
    else:
        assert mark > 0                                           # first run: 4, 5, 7, 16, 39, 15, 30, 87 (257 ... 8192 points); fixed iterations 4, 7, 87


def test_ransac_8193_points_are_refused_and_leave_nothing_behind(vislam, orc):
    p = vislam.default_params()
    p.fx = p.fy = 458.654
    p.ransac_threshold, p.ransac_adaptive, p.ransac_max_iters = 1.0, 1, 400
    x1, x2, R, t = two_view(8193, 5, 0.35, 0.5)
    c = vislam.Context(0, p)
    with pytest.raises(vislam.VisError) as ei:
        c.essential_ransac(x1, x2)
    assert ei.value.code == E_CAPACITY
    with pytest.raises(vislam.VisError) as ei:
        c.recover_pose(np.eye(3), x1, x2)
    assert ei.value.code == E_CAPACITY
    E, mask, ninl, it = c.essential_ransac(x1[:8192], x2[:8192])
    oE, omask, oninl, oiters = orc.essential_ransac(p, x1[:8192], x2[:8192])
    assert (ninl, it) == (oninl, oiters) and (mask == omask).all() and _cmpE(E, oE) <= TOL and oninl > 2000
    c.close()


# ---- the undecided list of k_hyp_score.  vis_pose_result.undecided_max (vis_debug_counters out[3] for the frame-at-a-time calls) is the
# most (model, point) decisions one sub-item (16 hypotheses) left to double precision: up to 4096 are settled from a list, more than
# that by recounting the sub-item.  Before this mark no test could tell which of the two had run.
MANY = [(300, 1.0, 458.654, 1.0, 1), (1000, 0.25, 458.654, 0.3, 1), (3000, 1.0, 150.0, 1.0, 1), (3000, 3.0, 458.654, 3.0, 0),
        (5000, 1.0, 458.654, 0.7, 1), (2049, 0.5, 90.0, 0.5, 0)]


@pytest.mark.parametrize("m,thr,fx,noise,adaptive", MANY)
def test_undecided_list_path(vislam, orc, m, thr, fx, noise, adaptive):
    """the cases of test_pose_gpu.test_many_correspondences_single_precision_scoring with the mark read: the list never overflows here
    (<= 4096) and is never empty -- the double-precision settle loop really decides something in these tests.  First run, in the
    order of MANY: 3, 6, 8, 29, 31, 2 entries: a few of the 10^5 ... 10^6 decisions of a sub-item, not the 0.1 % pose.hip once guessed."""
    oninl, oiters, mark = _ransac_case(vislam, orc, m, thr, fx, noise, adaptive)
    assert 100 < oninl < 0.95 * m
    assert 0 < mark <= 4096


@pytest.mark.parametrize("fx,thr", [(5000.0, 0.1), (5000.0, 0.25)])
def test_undecided_list_overflow_recounts_in_double(vislam, orc, fx, thr):
    """More than 4096 undecided decisions in one sub-item: k_hyp_score throws the sub-item's counts away and recounts it in double.
    The single-precision error radius of the Sampson numerator is relative to |s|, so against a threshold t (normalised: thr / fx)
    the undecided band is about 2^-20 * fx / thr of t wide: LONG focal lengths and small thresholds widen it, short ones do not
    (measured with 8192 points, 35 % outliers, noise = threshold, adaptive stop off, 400 iterations -- fx 40 ... 150: 7 ... 18 entries
    at any threshold; fx 458.654: 54 ... 263; fx 1500: 404 ... 1128; fx 5000: 4541 at thr 3, 6755 at 1, 10943 at 0.25, 13484 at 0.1).
    The two cases here overflow the list 3.3 and 2.7 times over (>= 1.5 x asked for, so a change of rounding does not bring them back
    under the cap).  Masks, counts and iterations must be the oracle's, E within TOL, as everywhere."""
    oninl, oiters, mark = _ransac_case(vislam, orc, 8192, thr, fx, thr, 0)
    assert oiters == 400 and oninl > 1000
    assert mark > 4096


# ------------------------------------------------------------------------------------------------ detector
def _noise_image(w, h, seed):
    """uniform noise under a 2 x 2 box (four taps): corners everywhere, up to the border"""
    n = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint32)
    return ((n + np.roll(n, 1, 0) + np.roll(n, 1, 1) + np.roll(np.roll(n, 1, 0), 1, 1)) // 4).astype(np.uint8)


def _detect_params(vislam, w, h, nfeatures):
    p = vislam.default_params()
    p.nfeatures, p.nlevels, p.w_size, p.h_size = nfeatures, 8, w, h
    return p


# (image seeds picked on the oracle's output alone: level-0 keypoints up to x = 4063 = side - 1 - 31, y = 4057 and 4061 / 4061)
@pytest.mark.parametrize("w,h,nfeatures,cap,seed", [(4095, 140, 1000, None, 7), (140, 4095, 1000, None, 3), (4095, 4095, 8000, 20000, 4095)])
def test_detector_at_image_side_4095(vislam, orc, w, h, nfeatures, cap, seed):
    """k_fast packs a candidate as score << 24 | y << 12 | x: 4095 is the largest side.  Level-0 keypoints must reach the last 64 columns /
    rows (x or y >= 4032 sets all of the six high bits of its field) -- asserted on the oracle's output."""
    img = _noise_image(w, h, seed)
    p = _detect_params(vislam, w, h, nfeatures)
    ok, od = orc.orb_detect_compute(p, img, cap=cap)
    l0 = ok[ok["octave"] == 0]
    print(f"detect {w} x {h}: {len(ok)} keypoints, level 0 reaches x = {l0['x'].max()}, y = {l0['y'].max()} (from {l0['x'].min()}, {l0['y'].min()})")
    assert len(ok) >= 500
    if w == 4095:
        assert l0["x"].max() >= 4032
    if h == 4095:
        assert l0["y"].max() >= 4032
    c = vislam.Context(0, p)
    k, d = c.orb_detect_compute(img, slot=0, cap=cap)
    c.close()
    assert len(k) == len(ok) and k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()


def test_detector_batched_at_width_4095_stride_4096(vislam, orc):
    """the batched path on 4095-wide frames in rows of 4096 bytes (the stride must be a multiple of 4, so it cannot equal this width:
    4095 as a stride is refused)"""
    import torch
    w, h = 4095, 140
    p = _detect_params(vislam, w, h, 1000)
    imgs = [_noise_image(w, h, seed) for seed in (7, 6, 9)]
    buf = np.full((3, h, 4096), 255, np.uint8)                    # the padding column is not zero: it must not be read as image
    for i, im in enumerate(imgs):
        buf[i, :, :w] = im
    dev = torch.from_numpy(buf).cuda()
    c = vislam.Context(0, p)
    with pytest.raises(vislam.VisError) as ei:
        c.batch_plan(w, h, 4095, 3)
    assert ei.value.code == E_INVALID
    c.batch_plan(w, h, 4096, 3)
    c.batch_run(dev.data_ptr(), 3, vislam.STAGE_DETECT)
    c.batch_sync()
    assert c.batch_status() == 0
    for i, im in enumerate(imgs):
        ok, od = orc.orb_detect_compute(p, im)
        k, d = c.batch_keypoints(i)
        assert len(ok) >= 500 and ok[ok["octave"] == 0]["x"].max() >= 4032
        assert len(k) == len(ok) and k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes(), i
    c.close()


@pytest.mark.parametrize("w,h", [(4096, 140), (140, 4096)])
def test_image_side_4096_is_refused(vislam, w, h):
    p = _detect_params(vislam, 752, 480, 1000)
    c = vislam.Context(0, p)
    with pytest.raises(vislam.VisError) as ei:
        c.orb_detect_compute(np.zeros((h, w), np.uint8), slot=0)
    assert ei.value.code == E_INVALID
    with pytest.raises(vislam.VisError) as ei:
        c.batch_plan(w, h, 4096, 2)
    assert ei.value.code == E_INVALID
    c.close()
