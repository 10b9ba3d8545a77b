"""CPU: the restatement tests/ftrack_ref.py against independent implementations.

Linking: a dictionary walk over the frames in order, written without pointer doubling, on random match lists with gated frames, duplicates on
either side, out-of-range indices, empty lists, a mask and a carried row; one stream of 40 frames cut into launches of 40, 16 + 24 and
1 + ... + 1 with the row carried gives identical observations.

N-view: a planted scene -- 300 points at depth 4 - 8, 8 cameras stepping 0.1 along x with 0.01 rad of yaw per frame, f = 458, pixels rounded
to float, seeds 1 - 3.  The median distance of the 8-view points from the truth is at most HALF that of the two-view DLT + the same refinement
on the last two frames, at 0.3 px and at 1 px of noise (the numpy prototype measured a ratio of 0.11 in all six cells: 0.021 - 0.024 against
0.20 - 0.22 at 0.3 px, 0.070 - 0.080 against 0.66 - 0.71 at 1 px; the factor two is margin, not a tuned bound).  With exact pixels the points
are exact to 1e-9, and the reported cost never exceeds the DLT point's."""
import math

import numpy as np
import pytest

import ftrack_ref as fr
from ftrack_stream_cases import walk_link


# ---------------------------------------------------------------------------------------------- linking
def random_stream(seed, n, row_cap, link_cap, gate=True, hostile=True, first_prev=fr.KF_FIRST):
    """(prev, nkp, links, nlinks, mask): mostly one-to-one lists with duplicates on either side, out-of-range indices, empty lists, counts beyond
    their capacities, gated and restarting frames"""
    rng = np.random.default_rng(seed)
    prev, nkp = np.zeros(n, np.int32), rng.integers(row_cap // 2, row_cap + 1, n).astype(np.int32)
    last = None
    for i in range(n):
        r = rng.random()
        if gate and r < 0.15:
            prev[i] = fr.KF_NOT_SAVED
            continue
        if gate and r < 0.2 and i:
            prev[i], last = fr.KF_FIRST, i
            continue
        prev[i] = first_prev if last is None else last
        last = i
    if hostile:
        nkp[rng.integers(0, n)] = row_cap + 7
        nkp[rng.integers(0, n)] = -3
    links = np.zeros((n, link_cap), fr.DMATCH_DTYPE)
    nlinks = np.zeros(n, np.int32)
    mask = (rng.random((n, link_cap)) < 0.8).astype(np.uint8)
    for i in range(n):
        m = int(rng.integers(0, link_cap + 1)) if rng.random() > 0.1 else 0
        q = rng.permutation(row_cap)[:m] if m <= row_cap else rng.integers(0, row_cap, m)
        t = rng.permutation(row_cap)[:m] if m <= row_cap else rng.integers(0, row_cap, m)
        if hostile and m > 4:
            d = rng.integers(0, m, 6)
            q[d[0]], t[d[1]] = q[d[2]], t[d[3]]                     # duplicates on either side
            q[d[4]], t[d[5]] = rng.choice([-1, row_cap, row_cap + 5, -2 ** 31]), rng.choice([-1, row_cap, 2 ** 31 - 1])
        links[i, :m]["queryIdx"], links[i, :m]["trainIdx"] = q, t
        nlinks[i] = m + (5 if hostile and rng.random() < 0.2 else 0)          # a count above the capacity is clamped
    return prev, nkp, links, nlinks, mask


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_dictionary_walk(seed):
    n, row_cap, link_cap = (1, 2, 3, 9, 33, 40)[seed], (8, 64, 65, 30, 20, 50)[seed], (8, 70, 65, 30, 16, 50)[seed]
    prev, nkp, links, nlinks, mask = random_stream(seed, n, row_cap, link_cap, first_prev=fr.KF_CARRIED if seed % 2 else fr.KF_FIRST)
    carry = fr.empty_row(row_cap)
    rng = np.random.default_rng(100 + seed)
    for k in rng.permutation(row_cap)[:row_cap // 2]:
        carry[k] = (int(rng.integers(0, 50)), int(rng.integers(0, row_cap)), int(rng.integers(1, 9)), -1)
    for m_, c_ in ((None, None), (mask, None), (None, carry), (mask, carry), (np.zeros_like(mask), carry)):
        got = fr.link_rows(prev, nkp, links, nlinks, row_cap, m_, c_, seq0=50)
        want = walk_link(prev, nkp, links, nlinks, row_cap, m_, c_, seq0=50)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (seed, m_ is not None, c_ is not None)
    f = fr.link_rows(prev, nkp, links, nlinks, row_cap, np.zeros_like(mask), carry, seq0=50)[1]
    assert not f["n_continued"].any()                               # a mask of all zeros links nothing


def test_first_in_list_order_wins_on_both_sides():
    links = np.zeros((2, 4), fr.DMATCH_DTYPE)
    links[1]["queryIdx"], links[1]["trainIdx"] = [0, 0, 1, 2], [0, 1, 1, 2]      # (q0, t0) links; (q0, t1) loses q0 but occupies t1; (q1, t1) loses
    obs, frames = fr.link_rows([fr.KF_FIRST, 0], [3, 3], links, [0, 4], 4)
    assert obs[1]["prev_kp"].tolist() == [0, -1, 2, -1] and obs[1]["len"].tolist() == [2, 1, 2, 0]
    assert frames[1].tolist() == (1, 3, 2, 1, 1, 2, 5, 0) and frames[0].tolist() == (0, 3, 0, 3, 0, 1, 3, fr.FT_NO_PAIR)


def test_a_stream_does_not_depend_on_how_it_is_cut_into_launches():
    n, row_cap, link_cap = 40, 24, 24
    prev, nkp, links, nlinks, mask = random_stream(11, n, row_cap, link_cap, hostile=False)
    assert (prev == fr.KF_NOT_SAVED).any()
    whole, _ = fr.link_rows(prev, nkp, links, nlinks, row_cap, mask)
    assert int(whole["len"].max()) >= 5
    for cuts in ([40], [16, 24], [1] * 40):
        carry, at, rows, flags = None, 0, [], []
        for m in cuts:
            p = prev[at:at + m].astype(np.int64) - at                # the launch's own numbering: an earlier launch's frame is the carried one
            local = np.where(prev[at:at + m] < 0, prev[at:at + m], np.where(p < 0, fr.KF_CARRIED, p)).astype(np.int32)
            # (the carried row is that of the last SAVED frame before the launch, which is what prev[] names: the gate links to nothing older)
            o, f = fr.link_rows(local, nkp[at:at + m], links[at:at + m], nlinks[at:at + m], row_cap, mask[at:at + m], carry, seq0=at)
            carry = fr.carry_out(local, o, carry, row_cap)
            rows.append(o)
            flags.append(f["flags"])
            at += m
        assert np.concatenate(rows).tobytes() == whole.tobytes(), cuts
        assert not (np.concatenate(flags) & fr.FT_NO_CARRY).any()


# ---------------------------------------------------------------------------------------------- N-view
CAM = fr.Camera(458.0, 458.0, 376.0, 240.0)


def planted(seed, noise, n_cam=8, n_pts=300):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 8, n_pts)], 1)
    poses, xy = [], []
    for j in range(n_cam):
        a = 0.01 * j
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        C = np.array([0.1 * j, 0.0, 0.0])
        t = -R @ C
        Xc = X @ R.T + t
        px = np.stack([CAM.fx * Xc[:, 0] / Xc[:, 2] + CAM.cx, CAM.fy * Xc[:, 1] / Xc[:, 2] + CAM.cy], 1) + noise * rng.standard_normal((n_pts, 2))
        poses.append([float(v) for v in np.concatenate([R.reshape(9), t])])
        xy.append(px.astype(np.float32))                            # pixels rounded to float
    return X, poses, xy


def solve(poses, xy, k, frames, tp):
    views = [(poses[j], float(xy[j][k, 0]), float(xy[j][k, 1])) for j in frames]      # newest first
    return fr.triangulate_track(tp, CAM, views, with_trace=True)


@pytest.mark.parametrize("noise", [0.3, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_eight_views_beat_the_last_two(seed, noise):
    X, poses, xy = planted(seed, noise)
    tp = fr.TriParams()
    e8, e2 = [], []
    for k in range(len(X)):
        p8, tr8 = solve(poses, xy, k, range(7, -1, -1), tp)
        p2, tr2 = solve(poses, xy, k, (7, 6), tp)
        assert int(p8["n_views"]) == 8 and int(p2["n_views"]) == 2
        for p, tr in ((p8, tr8), (p2, tr2)):                        # the least-cost rule: never above the DLT point's cost
            cost = float(p["rms_reproj_px"]) ** 2 * int(p["n_views"])
            assert min(tr) <= tr[0] and abs(cost - min(tr)) <= 1e-5 * max(min(tr), 1e-12)
        e8.append(np.linalg.norm(p8["X"] - X[k]))
        e2.append(np.linalg.norm(p2["X"] - X[k]))
    m8, m2 = float(np.median(e8)), float(np.median(e2))
    print(f"\nseed {seed}, noise {noise} px: median error 8 views {m8:.4f}, last two {m2:.4f}, ratio {m8 / m2:.3f}")
    assert m8 <= 0.5 * m2, (m8, m2)


def test_exact_pixels_give_exact_points():
    X, poses, _ = planted(5, 0.0, n_pts=60)
    tp = fr.TriParams()
    for k in range(len(X)):
        views = []
        for j in range(7, -1, -1):                                  # exact (double) pixels, not rounded to float
            P = poses[j]
            U = P[0] * X[k, 0] + P[1] * X[k, 1] + P[2] * X[k, 2] + P[9]
            V = P[3] * X[k, 0] + P[4] * X[k, 1] + P[5] * X[k, 2] + P[10]
            W = P[6] * X[k, 0] + P[7] * X[k, 1] + P[8] * X[k, 2] + P[11]
            views.append((P, CAM.fx * U / W + CAM.cx, CAM.fy * V / W + CAM.cy))
        p = fr.triangulate_track(tp, CAM, views)
        assert np.abs(p["X"] - X[k]).max() <= 1e-9 and int(p["flags"]) == fr.FTP_FRONT | fr.FTP_REPROJ_OK | fr.FTP_PARALLAX_OK | fr.FTP_KEPT, (k, p)


def test_flags_and_degenerate_tracks():
    X, poses, xy = planted(7, 0.0, n_pts=4)
    tp = fr.TriParams()
    v = lambda j, k=0: (poses[j], float(xy[j][k, 0]), float(xy[j][k, 1]))
    assert int(fr.triangulate_track(tp, CAM, [v(3)])["flags"]) == fr.FTP_FEW
    same = fr.triangulate_track(tp, CAM, [v(3), v(3)])             # two identical cameras: no baseline
    assert int(same["flags"]) & fr.FTP_SINGULAR or not int(same["flags"]) & fr.FTP_PARALLAX_OK
    behind = list(poses[0])
    behind[11] = -20.0                                              # the point lies behind this camera
    p = fr.triangulate_track(tp, CAM, [v(7), (behind, float(xy[0][0, 0]), float(xy[0][0, 1]))])
    assert not int(p["flags"]) & fr.FTP_KEPT
    big = fr.triangulate_track(tp, CAM, [v(7), (poses[6], 3e38, float(xy[6][0, 1]))])
    assert not int(big["flags"]) & fr.FTP_KEPT                      # a finite pixel, however large, is used and fails its flags
    near = fr.triangulate_track(fr.TriParams(max_parallax_cos=0.5), CAM, [v(7), v(0)])
    assert int(near["flags"]) & fr.FTP_REPROJ_OK and not int(near["flags"]) & (fr.FTP_PARALLAX_OK | fr.FTP_KEPT)


def test_rows_walk_window_and_ends():
    """the walk of triangulate_rows: only track ends get a point, the window keeps the newest max_views, a frame without a pose is skipped"""
    n, R = 6, 4
    X, poses, xy = planted(9, 0.0, n_cam=n, n_pts=R)
    prev = np.array([fr.KF_FIRST, 0, 1, 2, 3, 4], np.int32)
    nkp = np.full(n, R, np.int32)
    links = np.zeros((n, R), fr.DMATCH_DTYPE)
    links["queryIdx"] = links["trainIdx"] = np.arange(R)
    nl = np.array([0, R, R, R, 3, 3], np.int32)                    # keypoint 3 ends at frame 3
    obs, _ = fr.link_rows(prev, nkp, links, nl, R)
    P = np.array(poses)
    P[2] = np.nan                                                   # frame 2 has no pose
    pts, fl, sm = fr.triangulate_rows(fr.TriParams(max_views=4), CAM, prev, nkp, obs, np.stack(xy), P)
    assert not fl[:3].any() and not pts[:3]["n_views"].any()        # not ends: zero records
    assert int(pts[3, 3]["n_views"]) == 3 and not fl[3, :3].any()   # frames 3, (2 skipped), 1, 0
    assert pts[5, :3]["n_views"].tolist() == [3, 3, 3]              # the window 5, 4, 3, 2 keeps the newest four, of which frame 2 has no pose
    assert int(pts[4, 3]["n_views"]) == 1 and int(fl[4, 3]) == int(fl[5, 3]) == fr.FTP_FEW     # keypoint 3 starts anew in frames 4 and 5: one view each
    assert sm["n_ends"].tolist() == [0, 0, 0, 1, 1, 4] and sm["n_few"].tolist() == [0, 0, 0, 0, 1, 1] and int(sm[5]["n_kept"]) == 3
