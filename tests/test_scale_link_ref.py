"""CPU: the restatement of the scale links (tests/scale_link_ref.py) against a plain numpy model -- a dictionary of first winners, a sorted array --
on random and hostile rows, and on a planted scene: 300 points at depth 4-8, 12 cameras whose baselines vary from 0.05 to 0.3, true relative
poses with unit t, 70 % of the points seen per pair, pixels rounded to float, every pair triangulated by the project's restated two-view
triangulation (tests/triangulate_ref.py).  Noise-free, every VIS_SL_OK link is within 1e-5 of the true baseline ratio.  The case builders here
are shared with the GPU tests."""
import functools
import math

import numpy as np
import pytest

import scale_link_ref as sl
import triangulate_ref as tri

NAN, INF = float("nan"), float("inf")


def rot(w):
    return tri.rodrigues(np.asarray(w, np.float64))


def pose_records(n, rng, zero=(), nan=()):
    """n pose records with a random small rotation and a unit t; `zero`: all-zero records, `nan`: a NaN in R"""
    pose = np.zeros(n, sl.POSE_DTYPE)
    for i in range(n):
        t = rng.normal(0, 1, 3)
        pose[i]["R"] = rot(rng.normal(0, 0.05, 3)).reshape(9)
        pose[i]["t"] = t / np.linalg.norm(t)
    for i in zero:
        pose[i]["R"], pose[i]["t"] = 0.0, 0.0
    for i in nan:
        pose[i]["R"][4] = NAN
    return pose


def random_case(seed, n, row_cap, link_cap, pts_cap, hostile=True, first_prev=sl.KF_FIRST):
    """a stream of n frames with gated, restarting and pose-less frames; lists with duplicate, negative and out-of-range indices, counts beyond
    the capacity, points with z of 0, negative, NaN and +-inf, flag bytes with and without VIS_MP_KEPT"""
    rng = np.random.default_rng(seed)
    prev = np.zeros(n, np.int32)
    last = first_prev
    for i in range(n):
        r = rng.random()
        if i and r < 0.12:
            prev[i] = sl.KF_NOT_SAVED
            continue
        prev[i] = sl.KF_FIRST if (i and r < 0.18) else last
        if hostile and i and r > 0.97:
            prev[i] = i + 3                                         # not an earlier frame: counts as VIS_KF_FIRST
        last = i
    pose = pose_records(n, rng, zero=[i for i in range(n) if rng.random() < 0.08], nan=[i for i in range(n) if hostile and rng.random() < 0.04])
    links = np.zeros((n, link_cap), sl.DMATCH_DTYPE)
    links["queryIdx"] = rng.integers(0, row_cap, (n, link_cap))
    links["trainIdx"] = rng.integers(0, row_cap, (n, link_cap))
    nlinks = rng.integers(0, link_cap + 1, n).astype(np.int32)
    points = np.zeros((n, pts_cap), sl.MAP_POINT_DTYPE)
    points["X"] = rng.normal(0, 1, (n, pts_cap, 3)) * [1.0, 1.0, 0.0] + [0.0, 0.0, 1.0] * rng.uniform(2.0, 9.0, (n, pts_cap, 1))
    flags = np.where(rng.random((n, pts_cap)) < 0.8, 31, rng.integers(0, 16, (n, pts_cap))).astype(np.uint8)
    if hostile:
        bad = rng.random((n, link_cap)) < 0.08
        links["queryIdx"][bad] = rng.choice([-1, -7, row_cap, row_cap + 5, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
        bad = rng.random((n, link_cap)) < 0.08
        links["trainIdx"][bad] = rng.choice([-1, -7, row_cap, row_cap + 5, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
        nlinks[rng.random(n) < 0.15] = link_cap + 9
        nlinks[rng.random(n) < 0.1] = -3
        bad = rng.random((n, pts_cap)) < 0.1
        points["X"][..., 2][bad] = rng.choice([0.0, -0.0, -3.0, NAN, INF, -INF, 1e308, 5e-324], int(bad.sum()))
        bad = rng.random((n, pts_cap)) < 0.03
        points["X"][..., 0][bad] = rng.choice([NAN, INF, 1e308], int(bad.sum()))
    return prev, links, nlinks, pose, points, flags


def shared_case(ns, extra=3, values=None, seed=0, carried=False):
    """three frames (or, carried, the last of them alone with the depth row of frame 1): frame 2 shares exactly ns points with frame 1's pair, among
    ns + extra list entries; values: the ratios to plant (None: random in 0.5 ... 2), in list order.  Returns the rows and the planted ratios."""
    rng = np.random.default_rng(1000 + ns + seed)
    m = ns + extra
    row_cap = m + 2
    values = rng.uniform(0.5, 2.0, ns) if values is None else np.asarray(values, np.float64)
    pose = pose_records(3, rng)
    pose[1]["R"], pose[1]["t"] = np.eye(3).reshape(9), [0.0, 0.0, 1.0]   # depth in camera 1 = X[2] + 1
    links = np.zeros((3, m), sl.DMATCH_DTYPE)
    points = np.zeros((3, m), sl.MAP_POINT_DTYPE)
    flags = np.full((3, m), 31, np.uint8)
    kp = rng.permutation(row_cap)[:m]
    links[1]["queryIdx"], links[1]["trainIdx"] = rng.integers(0, row_cap, m), kp
    z2 = rng.uniform(3.0, 9.0, m)
    points[1]["X"][:, 2] = z2 - 1.0
    order = rng.permutation(m)                                      # which entries of frame 2's list share a point: the first ns of a permutation
    links[2]["queryIdx"][order] = kp
    links[2]["trainIdx"] = rng.integers(0, row_cap, m)
    points[2]["X"][order[:ns], 2] = z2[:ns] / values
    flags[2][order[ns:]] = 15                                       # the others lack VIS_MP_KEPT
    nlinks = np.array([0, m, m], np.int32)
    prev = np.array([sl.KF_FIRST, 0, 1], np.int32)
    if carried:
        depth, _ = sl.scale_link_rows(sl.Params(), prev, links, nlinks, pose, points, flags, row_cap)
        return (np.array([sl.KF_CARRIED], np.int32), links[2:], nlinks[2:], pose[2:], points[2:], flags[2:], row_cap, depth[1].copy()), values
    return (prev, links, nlinks, pose, points, flags, row_cap, None), values


def model(sp, prev, links, nlinks, pose, points, flags, row_cap, carry=None):
    """the contract once more with numpy: np.unique's first index for the winners, a sorted array for the statistics"""
    n = len(prev)
    mcap = min(links.shape[1], points.shape[1])
    depth, link = np.zeros((n, row_cap)), np.zeros(n, sl.LINK_DTYPE)
    qual = (flags[:, :mcap] & sp.require) == sp.require
    pos = lambda v: np.isfinite(v) & (v > 0)
    rows = [sl.has_row(prev, pose, i) for i in range(n)]
    for i in range(n):
        m = min(max(int(nlinks[i]), 0), mcap)
        if not rows[i]:
            continue
        tr = links[i, :m]["trainIdx"].astype(np.int64)
        ks = np.nonzero(qual[i, :m] & (tr >= 0) & (tr < row_cap))[0]
        kps, first = np.unique(tr[ks], return_index=True)
        X = points[i]["X"][ks[first]]
        R, t = pose[i]["R"], pose[i]["t"]
        with np.errstate(all="ignore"):
            z = ((R[6] * X[:, 0] + R[7] * X[:, 1]) + R[8] * X[:, 2]) + t[2]
        depth[i, kps] = np.where(pos(z), z, 0.0)
    for i in range(n):
        p = sl.norm_prev(prev, i)
        link[i]["q"] = p
        if p in (sl.KF_NOT_SAVED, sl.KF_FIRST):
            link[i]["flags"] = sl.SL_NO_PAIR
            continue
        qrow = None if p == sl.KF_CARRIED and carry is None else np.asarray(carry if p == sl.KF_CARRIED else depth[p])
        if qrow is None or not pos(qrow).any():
            link[i]["flags"] = sl.SL_NO_DEPTH
            continue
        m = min(max(int(nlinks[i]), 0), mcap)
        qi = links[i, :m]["queryIdx"].astype(np.int64)
        ok = qual[i, :m] & (qi >= 0) & (qi < row_cap)
        z2, z1 = qrow[np.where(ok, qi, 0)], points[i]["X"][:m, 2]
        ok &= pos(z2) & pos(z1)
        with np.errstate(all="ignore"):
            rho = z2[ok] / z1[ok]
        rho = np.sort(rho[pos(rho)])
        ns = len(rho)
        if ns:
            link[i]["scale"], link[i]["q25"], link[i]["q75"] = rho[(ns - 1) // 2], rho[(ns - 1) // 4], rho[(3 * (ns - 1)) // 4]
        link[i]["n_shared"] = ns
        fl = (sl.SL_FEW if ns < sp.min_shared else 0) | (sl.SL_SPREAD if link[i]["q75"] - link[i]["q25"] > sp.max_rel_spread * link[i]["scale"] else 0)
        link[i]["flags"] = fl | (0 if sp.min_scale <= link[i]["scale"] <= sp.max_scale else sl.SL_RANGE)
    return depth, link


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_numpy_model(seed):
    n, row_cap, link_cap, pts_cap = [(9, 40, 37, 41), (17, 64, 70, 66), (5, 8, 30, 30), (33, 65, 64, 64), (12, 300, 120, 100), (3, 16, 0, 0)][seed]
    case = random_case(seed, n, row_cap, link_cap, pts_cap, first_prev=sl.KF_CARRIED if seed & 1 else sl.KF_FIRST)
    carry = np.where(np.random.default_rng(seed).random(row_cap) < 0.7, np.random.default_rng(seed + 1).uniform(2, 9, row_cap), 0.0)
    for sp, c in ((sl.Params(), None), (sl.Params(require=0, min_shared=3, max_rel_spread=0.2, min_scale=0.8, max_scale=1.25), carry)):
        want, got = model(sp, *case, row_cap, c), sl.scale_link_rows(sp, *case, row_cap, c)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), seed
        assert np.isfinite(got[0]).all() and all(np.isfinite(got[1][f]).all() for f in ("scale", "q25", "q75"))
    if n >= 9:                                                      # (the longer streams do form ratios)
        assert (got[1]["n_shared"] > 0).any()


@pytest.mark.parametrize("ns", [0, 1, 2, 7, 8, 63, 64, 65])
def test_the_order_statistics_of_a_planted_row(ns):
    (prev, links, nlinks, pose, points, flags, row_cap, _), values = shared_case(ns)
    _, link = sl.scale_link_rows(sl.Params(), prev, links, nlinks, pose, points, flags, row_cap)
    assert [int(f) for f in link["flags"][:2]] == [sl.SL_NO_PAIR, sl.SL_NO_DEPTH] and int(link[2]["n_shared"]) == ns and int(link[2]["q"]) == 1
    if ns:
        s = np.sort(values)
        want = np.array([s[(ns - 1) // 2], s[(ns - 1) // 4], s[(3 * (ns - 1)) // 4]])
        assert np.abs(np.array([link[2]["scale"], link[2]["q25"], link[2]["q75"]]) / want - 1).max() < 1e-14   # (z2 / (z2 / v) rounds twice)
    assert bool(int(link[2]["flags"]) & sl.SL_FEW) == (ns < 8)
    if ns == 0:
        assert int(link[2]["flags"]) == sl.SL_FEW | sl.SL_RANGE and float(link[2]["scale"]) == 0.0
    # the carried form of the same frame gives the same record but q
    (cprev, *crest, crow_cap, carry), _ = shared_case(ns, carried=True)
    _, clink = sl.scale_link_rows(sl.Params(), cprev, *crest, crow_cap, carry)
    a, b = link[2:3].copy(), clink.copy()
    assert int(b[0]["q"]) == sl.KF_CARRIED
    b["q"] = a["q"]
    assert a.tobytes() == b.tobytes()
    assert int(sl.scale_link_rows(sl.Params(), cprev, *crest, crow_cap, None)[1][0]["flags"]) == sl.SL_NO_DEPTH


def test_flags_spread_range_and_the_first_winner():
    (prev, links, nlinks, pose, points, flags, row_cap, _), _ = shared_case(9, values=[4.0, 1.0, 2.0, 1.0, 4.0, 2.0, 1.0, 2.0, 4.0])
    run = lambda **kw: sl.scale_link_rows(sl.Params(**kw), prev, links, nlinks, pose, points, flags, row_cap)[1][2]
    r = run()
    assert (float(r["q25"]), float(r["scale"]), float(r["q75"]), int(r["flags"])) == (1.0, 2.0, 4.0, sl.SL_SPREAD)       # 3 > 1.0 * 2
    assert int(run(max_rel_spread=1.5)["flags"]) == sl.SL_OK and int(run(max_rel_spread=1.5, max_scale=1.9)["flags"]) == sl.SL_RANGE
    assert int(run(max_rel_spread=1.5, min_scale=2.0, max_scale=2.0, min_shared=10)["flags"]) == sl.SL_FEW
    # a second entry on the same keypoint of frame 1 loses, whatever its depth; an earlier one that does not qualify does not win
    l2, p2, f2 = links.copy(), points.copy(), flags.copy()
    m = links.shape[1]
    l2[1]["trainIdx"][m - 1] = l2[1]["trainIdx"][0]
    p2[1]["X"][m - 1, 2] = 100.0
    d = sl.scale_link_rows(sl.Params(), prev, l2, nlinks, pose, p2, f2, row_cap)[0]
    assert d[1, l2[1]["trainIdx"][0]] == points[1]["X"][0, 2] + 1.0
    f2[1, 0] = 15
    d = sl.scale_link_rows(sl.Params(), prev, l2, nlinks, pose, p2, f2, row_cap)[0]
    assert d[1, l2[1]["trainIdx"][0]] == 101.0
    assert sl.scale_link_rows(sl.Params(require=0), prev, l2, nlinks, pose, p2, f2, row_cap)[0][1, l2[1]["trainIdx"][0]] == points[1]["X"][0, 2] + 1.0


# ---------------------------------------------------------------------------------------------- the planted scene
FX, CX, CY = 458.0, 376.0, 240.0
N_CAM, N_PTS = 12, 300


@functools.lru_cache(maxsize=None)
def planted(seed, noise):
    """the scene of the module's docstring.  Returns a dict: prev, links, nlinks, pose (true relative poses, unit t), points / flags (restated
    two-view triangulation), xy (n, N_PTS, 2) float32, base (the true baselines, base[0] = 0), Rw / C (the cameras), X (the points)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, N_PTS), rng.uniform(-1.5, 1.5, N_PTS), rng.uniform(4, 8, N_PTS)], 1)
    base = np.concatenate([[0.0], rng.uniform(0.05, 0.3, N_CAM - 1)])
    Rw, C = [], []
    c = np.zeros(3)
    for j in range(N_CAM):
        d = np.array([1.0, 0.0, 0.0]) + rng.normal(0, 0.3, 3)
        c = c + base[j] * d / np.linalg.norm(d)
        Rw.append(rot([0.0, 0.01 * j, 0.0]) @ rot(rng.normal(0, 0.01, 3)))
        C.append(c)
    xy = np.zeros((N_CAM, N_PTS, 2), np.float32)
    for j in range(N_CAM):
        Xc = (X - C[j]) @ Rw[j].T
        xy[j] = (np.stack([FX * Xc[:, 0] / Xc[:, 2] + CX, FX * Xc[:, 1] / Xc[:, 2] + CY], 1) + noise * rng.standard_normal((N_PTS, 2))).astype(np.float32)
    m = (7 * N_PTS) // 10
    prev = np.arange(-1, N_CAM - 1).astype(np.int32)
    prev[0] = sl.KF_FIRST
    links, nlinks = np.zeros((N_CAM, m), sl.DMATCH_DTYPE), np.full(N_CAM, m, np.int32)
    pose, points, flags = np.zeros(N_CAM, sl.POSE_DTYPE), np.zeros((N_CAM, m), sl.MAP_POINT_DTYPE), np.zeros((N_CAM, m), np.uint8)
    nlinks[0] = 0
    for j in range(1, N_CAM):
        seen = rng.permutation(N_PTS)[:m]
        links[j]["queryIdx"] = links[j]["trainIdx"] = seen          # keypoint k of every frame is point k
        R = Rw[j] @ Rw[j - 1].T
        t = Rw[j] @ (C[j - 1] - C[j])
        pose[j]["R"], pose[j]["t"] = R.reshape(9), t / np.linalg.norm(t)
        pts, fl, _, _ = tri.triangulate(pose[j]["R"], pose[j]["t"], xy[j - 1][seen], xy[j][seen], FX, FX, CX, CY)
        points[j], flags[j] = pts, fl
    return dict(prev=prev, links=links, nlinks=nlinks, pose=pose, points=points, flags=flags, xy=xy, base=base, Rw=Rw, C=C, X=X)


# VIS_MP_KEPT contains VIS_MP_FRONT, recoverPose's test, which also demands a depth below 50 baselines; this scene reaches 8 / 0.05 = 160.  The
# scene's links therefore require the other three bits, and leave the sign of the depth to the links' own z > 0 tests.
PLANTED_REQUIRE = 1 | 4 | 8


def planted_links(seed, noise):
    s = planted(seed, noise)
    return sl.scale_link_rows(sl.Params(require=PLANTED_REQUIRE), s["prev"], s["links"], s["nlinks"], s["pose"], s["points"], s["flags"], N_PTS)[1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_links_recover_the_baseline_ratios(seed):
    s, link = planted(seed, 0.0), planted_links(seed, 0.0)
    assert int(link[0]["flags"]) == sl.SL_NO_PAIR and int(link[1]["flags"]) == sl.SL_NO_DEPTH
    worst = 0.0
    for i in range(2, N_CAM):
        assert int(link[i]["flags"]) == sl.SL_OK and int(link[i]["n_shared"]) > 100, link[i]
        worst = max(worst, abs(float(link[i]["scale"]) / (s["base"][i] / s["base"][i - 1]) - 1.0))
    print(f"\nseed {seed}: worst baseline-ratio error {worst:.2e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("noise", [0.3, 1.0])
def test_noisy_links_and_their_spread(noise):
    """recorded, and asserted only as far as the defaults rely on it: every link of the scene stays VIS_SL_OK under max_rel_spread = 1.0"""
    worst, spread = 0.0, 0.0
    for seed in (1, 2, 3):
        s, link = planted(seed, noise), planted_links(seed, noise)
        for i in range(2, N_CAM):
            assert int(link[i]["flags"]) == sl.SL_OK, (seed, i, link[i])
            worst = max(worst, abs(float(link[i]["scale"]) / (s["base"][i] / s["base"][i - 1]) - 1.0))
            spread = max(spread, (float(link[i]["q75"]) - float(link[i]["q25"])) / float(link[i]["scale"]))
    print(f"\nnoise {noise} px: worst baseline-ratio error {worst:.3f}, largest (q75 - q25) / scale {spread:.3f}")
    assert spread < 1.0
