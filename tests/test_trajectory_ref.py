"""CPU: the restatement of the chained trajectory (tests/trajectory_ref.py): its pointer doubling against its own plain left-to-right composition
and against a numpy 4 x 4 model, the flags, segments and epochs of every pairing the GPU tests use, and the planted scene of
tests/test_scale_link_ref.py -- the end point of the scaled chain against the same chain with every s = 1, and the trajectory's d_poses fed to the
restated N-view triangulation against the true poses.  The case builders here are shared with the GPU tests.

DOUBLING_BOUND is the largest difference between doubling and sequential composition measured over the streams below (R entries absolute -- they
are bounded by 1 --, sigma relative, t against the path length); two cuts of a stream differ by that kind of rounding, and the GPU tests allow 16
times it."""
import math

import numpy as np
import pytest

import ftrack_ref as fr
import scale_link_ref as sl
import trajectory_ref as tj
from test_scale_link_ref import FX, CX, CY, N_CAM, N_PTS, planted, planted_links, pose_records

DOUBLING_BOUND = 2.7e-15                                            # measured 2.66e-15 (|dR|; sigma 1.89e-15, t 6.2e-16): the test below prints it
NS = (1, 2, 3, 4, 5, 33, 64, 65, 257)
PAIRINGS = ("chain", "gated", "poseless", "badlink", "siblings")


def pairing(name, n, seed=0, first=sl.KF_FIRST):
    """(prev, pose, link) of n frames.  chain: i - 1.  gated: runs of VIS_KF_NOT_SAVED frames, the saved ones paired with the last saved.
    poseless: a frame in the middle has a zero pose record (a new segment).  badlink: a link in the middle is VIS_SL_FEW (a new epoch).
    siblings: frames 1 and 2 are both children of frame 0."""
    rng = np.random.default_rng(100 * n + seed)
    prev = np.arange(-1, n - 1).astype(np.int32)
    prev[0] = first
    pose = pose_records(n, rng)
    link = np.zeros(n, sl.LINK_DTYPE)
    link["scale"], link["n_shared"] = rng.uniform(0.5, 2.0, n), 50
    link["q25"], link["q75"] = link["scale"] * 0.9, link["scale"] * 1.1
    mid = n // 2
    if name == "gated":
        last = first
        for i in range(n):
            if rng.random() < 0.4 and i not in (1,):
                prev[i] = sl.KF_NOT_SAVED
            else:
                prev[i], last = last, i
    elif name == "poseless" and n > 2:
        pose[mid]["R"], pose[mid]["t"] = 0.0, 0.0
    elif name == "badlink" and n > 2:
        link[mid]["flags"] = sl.SL_FEW
    elif name == "siblings" and n > 2:
        prev[2] = 0
    link["q"] = [sl.norm_prev(prev, i) for i in range(n)]
    return prev, pose, link


def carried_record(seed=7):
    rng = np.random.default_rng(seed)
    c = tj.zero_record(tj.TJ_UNIT_EDGE)
    c["R"], c["t"], c["sigma"] = pose_records(1, rng)[0]["R"], rng.normal(0, 3, 3), 0.37
    c["segment_seq"], c["epoch_seq"], c["hops"], c["unit_edges"], c["parent"] = 11, 14, 9, 2, 5
    return c


def differences(a, b, path):
    """(max |dR|, max relative d sigma, max |dt| / path length) over the records both have"""
    ok = [i for i in range(len(a)) if not (int(a[i]["flags"]) | int(b[i]["flags"])) & (tj.TJ_NOT_SAVED | tj.TJ_OVERFLOW)]
    if not ok:
        return 0.0, 0.0, 0.0
    dR = max(float(np.abs(a[i]["R"] - b[i]["R"]).max()) for i in ok)
    dS = max(abs(float(a[i]["sigma"]) / float(b[i]["sigma"]) - 1.0) for i in ok)
    dt = max(float(np.abs(a[i]["t"] - b[i]["t"]).max()) / max(path[i], 1e-300) for i in ok)
    return dR, dS, dt


def path_lengths(rec, carry=None):
    """the length of the path from the root (or the carried record: |tc| stands for what lies before it) to every frame"""
    L = np.zeros(len(rec))
    for i in range(len(rec)):
        p = int(rec[i]["parent"])
        if int(rec[i]["flags"]) & (tj.TJ_ROOT | tj.TJ_NOT_SAVED | tj.TJ_OVERFLOW):
            continue
        L[i] = (L[p] if p >= 0 else float(np.linalg.norm(carry["t"]))) + float(rec[i]["sigma"])
    return L


def assert_same_but_rounding(a, b, path, bound):
    for f in ("segment_seq", "epoch_seq", "hops", "unit_edges", "parent", "flags"):
        assert (a[f] == b[f]).all(), f
    d = differences(a, b, path)
    assert max(d) <= bound, d
    return d


def stream_cases():
    for n in NS:
        for name in PAIRINGS:
            for carry in (None, carried_record()):
                yield n, name, carry


def test_doubling_against_sequential_composition():
    worst = (0.0, 0.0, 0.0)
    for n, name, carry in list(stream_cases()) + [(37, "chain", None), (37, "gated", carried_record())]:
        prev, pose, link = pairing(name, n, first=sl.KF_CARRIED if carry is not None else sl.KF_FIRST)
        rec, _ = tj.trajectory_rows(prev, pose, link, carry, seq0=40)
        seq = tj.sequential_rows(prev, pose, link, carry, seq0=40)
        d = assert_same_but_rounding(rec, seq, path_lengths(seq, carry), math.inf)   # (the integers; the bound is asserted on the whole below)
        worst = tuple(max(x, y) for x, y in zip(worst, d))
        assert all(np.isfinite(rec[f]).all() for f in ("R", "t", "sigma"))
    # the longest chain: how far R has drifted from a rotation (not repaired)
    prev, pose, link = pairing("chain", 257)
    rec, _ = tj.trajectory_rows(prev, pose, link)
    R = rec[256]["R"].reshape(3, 3)
    print(f"\ndoubling against sequential: max |dR| {worst[0]:.2e}, sigma {worst[1]:.2e}, t / path {worst[2]:.2e}; "
          f"max |R R^T - I| after 256 edges {np.abs(R @ R.T - np.eye(3)).max():.2e}")
    assert 0.0 < max(worst) <= DOUBLING_BOUND                       # (the two orders do round differently: the bound is not vacuous)


def test_against_a_4x4_model():
    """x_i = R_i x_q + sigma_i t_i chained with numpy matrices"""
    for name in PAIRINGS:
        prev, pose, link = pairing(name, 33)
        rec, _ = tj.trajectory_rows(prev, pose, link, seq0=5)
        T, sig = {}, {}
        for i in range(33):
            f = int(rec[i]["flags"])
            if f & tj.TJ_NOT_SAVED:
                assert rec[i].tobytes() == tj.zero_record(tj.TJ_NOT_SAVED).tobytes()
                continue
            if f & tj.TJ_ROOT:
                T[i], sig[i] = np.eye(4), 1.0
                assert int(rec[i]["segment_seq"]) == int(rec[i]["epoch_seq"]) == 5 + i and int(rec[i]["hops"]) == int(rec[i]["unit_edges"]) == 0
            else:
                q = int(prev[i])
                s = 1.0 if f & tj.TJ_UNIT_EDGE else float(link[i]["scale"])
                sig[i] = sig[q] * s
                E = np.eye(4)
                E[:3, :3], E[:3, 3] = pose[i]["R"].reshape(3, 3), sig[i] * pose[i]["t"]
                T[i] = E @ T[q]
                assert int(rec[i]["segment_seq"]) == int(rec[q]["segment_seq"]) and int(rec[i]["hops"]) == int(rec[q]["hops"]) + 1
                assert int(rec[i]["epoch_seq"]) == (5 + i if f & tj.TJ_UNIT_EDGE else int(rec[q]["epoch_seq"]))
                assert int(rec[i]["unit_edges"]) == int(rec[q]["unit_edges"]) + bool(f & tj.TJ_UNIT_EDGE)
                assert bool(f & tj.TJ_UNIT_EDGE) == (int(link[i]["flags"]) != sl.SL_OK or bool(int(rec[q]["flags"]) & tj.TJ_ROOT))
            assert np.abs(rec[i]["R"].reshape(3, 3) - T[i][:3, :3]).max() < 1e-13 and np.abs(rec[i]["t"] - T[i][:3, 3]).max() < 1e-12
            assert abs(float(rec[i]["sigma"]) / sig[i] - 1) < 1e-13


def test_segments_epochs_and_the_dense_poses():
    n = 9
    prev, pose, link = pairing("badlink", n)                        # frame 4 holds its scale: a new epoch
    rec, poses = tj.trajectory_rows(prev, pose, link, seq0=20)
    assert [int(v) for v in rec["epoch_seq"]] == [20, 21, 21, 21, 24, 24, 24, 24, 24] and (rec["segment_seq"] == 20).all()
    assert [int(v) for v in rec["unit_edges"]] == [0, 1, 1, 1, 2, 2, 2, 2, 2]
    assert (poses[:4] == 0).all() and (poses[4:, :9] == rec["R"][4:]).all() and (poses[4:, 9:] == rec["t"][4:]).all()
    _, poses = tj.trajectory_rows(prev, pose, link, seq0=20, same_epoch_only=False)
    assert (poses[:, :9] == rec["R"]).all()
    prev, pose, link = pairing("poseless", n)                       # frame 4 has no pose: a root, a new segment
    rec, poses = tj.trajectory_rows(prev, pose, link, seq0=20)
    assert int(rec[4]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_POSE and [int(v) for v in rec["segment_seq"]] == [20] * 4 + [24] * 5
    assert int(rec[5]["flags"]) == tj.TJ_UNIT_EDGE and (poses[:5] == 0).all() and (poses[5:, :9] == rec["R"][5:]).all()
    _, poses = tj.trajectory_rows(prev, pose, link, seq0=20, same_epoch_only=False)
    assert (poses[:4] == 0).all() and (poses[4, :9] == tj.IDENTITY).all()
    prev, pose, link = pairing("siblings", n)                       # two children of the root: each its own unit edge
    rec, _ = tj.trajectory_rows(prev, pose, link)
    assert int(rec[1]["flags"]) == int(rec[2]["flags"]) == tj.TJ_UNIT_EDGE and int(rec[2]["hops"]) == 1 and int(rec[3]["hops"]) == 2
    # a carried record: inherited segment, added counts; without it a root with NO_CARRY; a carried record that overflowed counts as none
    c = carried_record()
    prev, pose, link = pairing("chain", 4, first=sl.KF_CARRIED)
    rec, _ = tj.trajectory_rows(prev, pose, link, c, seq0=30)
    assert (rec["segment_seq"] == 11).all() and [int(v) for v in rec["hops"]] == [10, 11, 12, 13] and (rec["epoch_seq"] == 14).all() and (rec["unit_edges"] == 2).all()
    for none in (None, tj.zero_record(tj.TJ_OVERFLOW), tj.zero_record(tj.TJ_NOT_SAVED)):
        rec, _ = tj.trajectory_rows(prev, pose, link, none, seq0=30)
        assert int(rec[0]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_CARRY and int(rec[1]["flags"]) == tj.TJ_UNIT_EDGE and (rec["segment_seq"] == 30).all()


def overflowing(n=12):
    """a chain whose sigma product leaves the doubles: up past 1e308, and (the second) down to 0"""
    prev, pose, link = pairing("chain", n)
    link["scale"] = 1e60
    down = link.copy()
    down["scale"] = 1e-60
    return prev, pose, link, down


def test_a_sigma_product_that_overflows():
    prev, pose, up, down = overflowing()
    for link in (up, down):
        rec, poses = tj.trajectory_rows(prev, pose, link)
        bad = [bool(int(f) & tj.TJ_OVERFLOW) for f in rec["flags"]]
        assert bad[-1] and not bad[2] and bad == sorted(bad)       # from some frame on, every record
        for i in range(len(prev)):
            if bad[i]:
                assert rec[i].tobytes() == tj.zero_record(tj.TJ_OVERFLOW).tobytes() and (poses[i] == 0).all()
        assert all(np.isfinite(rec[f]).all() for f in ("R", "t", "sigma"))


# ---------------------------------------------------------------------------------------------- the planted scene
def end_point(rec):
    R, t = rec[-1]["R"].reshape(3, 3), rec[-1]["t"]
    return -R.T @ t


@pytest.mark.parametrize("noise", [0.3, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_scaled_chain_against_unit_baselines(seed, noise):
    s, link = planted(seed, noise), planted_links(seed, noise)
    b1 = s["base"][1]
    true = s["Rw"][0] @ (s["C"][-1] - s["C"][0]) / b1               # the last centre in the root's frame, in units of the first baseline
    path = s["base"].sum() / b1
    rec, _ = tj.trajectory_rows(s["prev"], s["pose"], link)
    assert (rec["unit_edges"][1:] == 1).all()                       # scaled throughout
    unit = link.copy()
    unit["flags"] = sl.SL_FEW
    rec1, _ = tj.trajectory_rows(s["prev"], s["pose"], unit)
    e, e1 = np.linalg.norm(end_point(rec) - true), np.linalg.norm(end_point(rec1) - true)
    print(f"\nseed {seed}, noise {noise} px: end-point error {e / path:.4f} of the path scaled, {e1 / path:.3f} with every s = 1, ratio {e / e1:.4f}")
    assert e <= 0.1 * e1


N_VIEW_RATIO = {}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_dense_poses_feed_the_n_view_triangulation(seed):
    """median point error under the chained poses against that under the true poses, at 0.3 px, over the track ends of the newest three frames.
    Measured: 2.785, 1.367 and 2.156 times (seeds 1, 2, 3); at most 3 is asserted."""
    s, link = planted(seed, 0.3), planted_links(seed, 0.3)
    _, poses = tj.trajectory_rows(s["prev"], s["pose"], link)
    assert (poses[0] == 0).all() and (poses[1:, :9] != 0).any(1).all()   # the root is its own epoch; frames 1 ... 11 share one
    b1 = s["base"][1]
    true = np.zeros((N_CAM, 12))
    for j in range(1, N_CAM):
        true[j, :9] = (s["Rw"][j] @ s["Rw"][0].T).reshape(9)
        true[j, 9:] = s["Rw"][j] @ (s["C"][0] - s["C"][j]) / b1
    Xtrue = (s["X"] - s["C"][0]) @ s["Rw"][0].T / b1
    nkp = np.full(N_CAM, N_PTS, np.int32)
    obs, _ = fr.link_rows(s["prev"], nkp, s["links"], s["nlinks"], N_PTS)
    cam, tp = fr.Camera(FX, FX, CX, CY), fr.TriParams()
    err = []
    for P in (poses, true):
        pts, flags, _ = triangulate_ends(tp, cam, s["prev"], obs, s["xy"], P, range(N_CAM - 3, N_CAM))
        kept = (flags & fr.FTP_KEPT) != 0
        assert kept.sum() > 200
        err.append(float(np.median(np.linalg.norm(pts["X"][kept] - Xtrue[np.nonzero(kept)[1]], axis=1))))
    N_VIEW_RATIO[seed] = err[0] / err[1]
    print(f"\nseed {seed}: median point error {err[0]:.4f} under the chained poses, {err[1]:.4f} under the true ones, ratio {err[0] / err[1]:.3f}")
    assert err[0] <= 3.0 * err[1]


def triangulate_ends(tp, cam, prev, obs, xy, poses, frames):
    """fr.triangulate_rows restricted to the track ends inside `frames` (the walk and the records are triangulate_rows' own)"""
    n, R = obs.shape
    nk = fr.counts(prev, np.full(n, R), R)
    child = np.zeros((n, R), bool)
    for i in range(n):
        for k in range(R):
            pq = fr.track_parent(prev, nk, obs, i, k)
            if pq is not None:
                child[pq] = True
    P = [[float(v) for v in poses[i]] for i in range(n)]
    ok = [fr.has_pose(p) for p in P]
    pts, flags = np.zeros((n, R), fr.POINT_DTYPE), np.zeros((n, R), np.uint8)
    for i in frames:
        for k in range(R):
            if child[i, k]:
                continue
            views, cur = [], (i, k)
            for _ in range(tp.max_views):
                f, kk = cur
                if ok[f]:
                    views.append((P[f], float(xy[f, kk, 0]), float(xy[f, kk, 1])))
                cur = fr.track_parent(prev, nk, obs, f, kk)
                if cur is None:
                    break
            pts[i, k] = fr.triangulate_track(tp, cam, views)
            flags[i, k] = int(pts[i, k]["flags"])
    return pts, flags, None
