"""GPU: PnP (vis_pnp_batch / vis_pnp_ransac) against the restatement tests/pnp_ref.py.

Records and masks are compared BYTE FOR BYTE, every integer and every double: the restatement takes every product and sum in the kernels'
order, the sums of the refinement included.  Output buffers are pre-filled with 0xEE and everything the call must not write is checked to
keep it; map points beyond a row's count and the fourth double of a point at x_stride 4 are NaN, so a read of either would show.

The build has one workgroup shape (256 lanes, one sample per lane, rows walked in tiles of VIS_PNP_TILE points): the rows of the CPU case
list (M 40 and 300, one tile) and the rows around one and two tiles all go through it in one launch.

A row whose normal matrix is singular because every inlier is the same point cannot be built: the three points of the winning sample
reproject exactly and are always among its inliers.  The failed pivot is checked on the restatement (tests/test_pnp_ref.py); here the
VIS_PNP_REFINE_REJECTED rows are two whose single Gauss-Newton step, taken at a threshold of 100 / 1000 px over gross outliers, raises the
cost.

vis_batch_pnp runs on the parallax stream tests/test_triangulate_gpu.py batches (vis_synth_frame_parallax, canvas 2048 / seed 0xE0C00001,
752 x 480, fy = fx), two launches of 16 frames, gate off and on (with the gate, frame 5 of each launch is flat and is not saved, so a link
skips it)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_ref as pr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC = 240
CAM = pr.Camera()


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _params(vislam):
    return pdc.set_mode(vislam.default_params(), "adaptive")      # the camera of the scenes


def _both(vislam, **kw):
    """the library's and the restatement's parameter blocks, set alike"""
    a, b = vislam.default_pnp_params(), pr.default_params()
    for k, v in kw.items():
        setattr(a, k, v)
        setattr(b, k, v)
    return a, b


class _Rows:
    """problems as device rows of max_pts points at a point stride of x_stride doubles"""
    def __init__(self, torch, probs, max_pts, x_stride=3, npts=None):
        self.probs, self.n, self.max_pts, self.x_stride = probs, len(probs), max_pts, x_stride
        X = np.full((self.n, max_pts, x_stride), np.nan)
        xy = np.full((self.n, max_pts, 2), np.nan, np.float32)
        for i, (a, b) in enumerate(probs):
            k = min(len(a), max_pts)
            X[i, :k, :3], xy[i, :k] = a[:k], b[:k]
        self.npts = np.array([len(a) for a, _ in probs], np.int32) if npts is None else np.asarray(npts, np.int32)
        self.d_X, self.d_xy, self.d_npts = _dev(torch, X), _dev(torch, xy), _dev(torch, self.npts)

    def m(self, i):
        return min(max(int(self.npts[i]), 0), self.max_pts)

    def run(self, vislam, torch, c, pp, d_draws, with_mask=True):
        """(records, mask rows) of one vis_pnp_batch; guard records / bytes checked"""
        n, cap = self.n, self.max_pts + 3
        out, mask = _filled(torch, (n + 2) * REC), _filled(torch, n * cap + 64)
        c.pnp_batch(n, self.d_X.data_ptr(), self.x_stride, self.d_xy.data_ptr(), self.d_npts.data_ptr(), self.max_pts, d_draws.data_ptr(), cap,
                    mask.data_ptr() if with_mask else 0, out.data_ptr(), pp)
        c.batch_sync()
        raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
        assert (raw[n * REC:] == FILL).all() and (mraw[n * cap:] == FILL).all()
        rows = mraw[:n * cap].reshape(n, cap)
        for i in range(n):
            assert (rows[i, self.m(i):] == FILL).all(), i          # bytes beyond the problem's points are left untouched
        if not with_mask:
            assert (mraw == FILL).all()
        return raw[:n * REC].view(vislam.PNP_RESULT_DTYPE).copy(), rows


def _check(recs, masks, rows, want, where):
    for i in range(rows.n):
        w_rec, w_mask = want[i]
        m = rows.m(i)
        assert recs[i].tobytes() == w_rec.tobytes(), (where, i, recs[i], w_rec)
        assert masks[i, :m].tobytes() == w_mask.tobytes(), (where, i)


@pytest.fixture(scope="module")
def draws():
    return pr.make_draws(7)


@pytest.fixture(scope="module")
def probs(vislam):
    """(X, xy) of the CPU case list, then the edge rows: m 3 | 4 | 5, one tile - 1 | one tile | one tile + 1, two tiles + 7"""
    T = vislam.PNP_TILE
    out = [pr.make_scene(*case)[:2] for case in pr.table_cases()]
    for m in (3, 4, 5):
        out.append(pr.make_scene("general", m, 0.0, 0.0)[:2])
    for k, m in enumerate((T - 1, T, T + 1, 2 * T + 7)):
        out.append(pr.make_scene(("general", "plane", "dup", "general")[k], m, 0.3, 0.25)[:2])
    return out


@pytest.fixture(scope="module")
def want(probs, draws):
    """per problem (record, mask) of the restatement at the default parameters"""
    pp = pr.default_params()
    return [pr.pnp(CAM, pp, X, xy, draws) for X, xy in probs]


@pytest.mark.parametrize("x_stride", [3, 4])
def test_records_and_masks_against_the_restatement(vislam, probs, want, draws, x_stride):
    import torch
    T = vislam.PNP_TILE
    c = vislam.Context(0, _params(vislam))
    d_draws = _dev(torch, draws)
    pp, pq = _both(vislam)
    # every problem in one launch, rows of two tiles + 7; then a row whose count is above max_pts (clamped), an empty row and a negative count
    rows = _Rows(torch, probs, 2 * T + 7, x_stride)
    recs, masks = rows.run(vislam, torch, c, pp, d_draws)
    _check(recs, masks, rows, want, ("all", x_stride))
    assert [int(r["n_points"]) for r in recs[-7:]] == [0, 4, 5, T - 1, T, T + 1, 2 * T + 7]
    assert all(int(r["best_iter"]) >= 0 and int(r["flags"]) & vislam.PNP_REFINED for r in recs[-4:])
    assert {int(r["best_root"]) for r in recs} >= {0, 1}           # more than one root's place wins somewhere
    big = probs[-1]
    edge = _Rows(torch, [big, big, big, probs[0]], 40, x_stride, [1000, 0, -5, 40])
    recs_e, masks_e = edge.run(vislam, torch, c, pp, d_draws)
    w40 = pr.pnp(CAM, pq, big[0][:40], big[1][:40], draws)
    _check(recs_e, masks_e, edge, [w40, (pr.zero_record(), np.zeros(0, np.uint8)), (pr.zero_record(), np.zeros(0, np.uint8)), want[0]], ("edge", x_stride))
    assert int(recs_e[0]["n_points"]) == 40
    # without a mask nothing but the records is written; a second run is byte-identical
    recs2, _ = rows.run(vislam, torch, c, pp, d_draws, with_mask=False)
    assert recs2.tobytes() == recs.tobytes()
    recs3, masks3 = rows.run(vislam, torch, c, pp, d_draws)
    assert recs3.tobytes() == recs.tobytes() and masks3.tobytes() == masks.tobytes()
    c.close()


def test_iteration_counts_at_wave_and_workgroup_edges(vislam):
    """one sample per lane, 256 lanes: the edges of a wave (64) and of a round (256); iters 0 gives zero records.  At 0.5 px the counts of the
    samples differ, so the winner moves as the table grows"""
    import torch
    T = vislam.PNP_TILE
    table = pr.make_draws(11, 257)
    three = [pr.make_scene(cls, 40, 0.3, 0.25)[:2] for cls in ("general", "plane", "dup")]
    three.append(pr.make_scene("tilted", T + 1, 0.3, 0.25)[:2])
    hyps = [pr.hypotheses(CAM, _both(vislam, threshold_px=0.5)[1], X, xy, table, 257) for X, xy in three]
    c = vislam.Context(0, _params(vislam))
    d_draws = _dev(torch, table)
    rows = _Rows(torch, three, T + 1)
    winners = set()
    for iters in (1, 63, 64, 65, 255, 256, 257, 200, 0):
        pp, pq = _both(vislam, iters=iters, threshold_px=0.5)
        recs, masks = rows.run(vislam, torch, c, pp, d_draws)
        if iters == 0:
            for i in range(rows.n):
                assert recs[i].tobytes() == pr.zero_record().tobytes() and not masks[i, :rows.m(i)].any()
            continue
        want = [pr.finish(CAM, pq, X, xy, hyps[i], *pr.pick(hyps[i], iters)) for i, (X, xy) in enumerate(three)]
        _check(recs, masks, rows, want, iters)
        winners |= {int(r["best_iter"]) for r in recs}
    assert max(winners) >= 64                                      # a winner beyond the first wave
    c.close()


def test_refine_iters_and_flags(vislam, draws):
    """refine_iters 0 | 1 | 5; a step that raises the cost (VIS_PNP_REFINE_REJECTED keeps the winner); a winner below min_inliers (VIS_PNP_FEW)"""
    import torch
    c = vislam.Context(0, _params(vislam))
    d_draws = _dev(torch, draws)
    scenes = [pr.make_scene(*case)[:2] for case in (("general", 40, 0.3, 0.25), ("dup", 40, 0.3, 0.25), ("tilted", 40, 0.0, 0.25), ("plane", 300, 0.3, 0.0))]
    rows = _Rows(torch, scenes, 300)
    seen = set()
    for kw in (dict(refine_iters=0), dict(refine_iters=1), dict(refine_iters=5), dict(refine_iters=1, threshold_px=100.0),
               dict(refine_iters=1, threshold_px=1000.0), dict(refine_iters=5, threshold_px=1000.0), dict(min_inliers=31), dict(min_inliers=4)):
        pp, pq = _both(vislam, **kw)
        recs, masks = rows.run(vislam, torch, c, pp, d_draws)
        _check(recs, masks, rows, [pr.pnp(CAM, pq, X, xy, draws) for X, xy in scenes], kw)
        for r in recs:
            fl = int(r["flags"])
            seen.add(fl)
            if kw.get("refine_iters") == 0:
                assert fl == 0 and float(r["cost0"]) == float(r["cost1"]) and r["R"].tobytes() == r["R_ransac"].tobytes()
            if fl & vislam.PNP_REFINE_REJECTED:
                assert not float(r["cost1"]) <= float(r["cost0"])
            if fl & (vislam.PNP_REFINE_REJECTED | vislam.PNP_FEW) or fl == 0:
                assert r["R"].tobytes() == r["R_ransac"].tobytes() and r["t"].tobytes() == r["t_ransac"].tobytes()
                assert int(r["n_inliers_refined"]) == int(r["n_inliers"])
            if fl & vislam.PNP_REFINED:
                assert float(r["cost1"]) <= float(r["cost0"]) and r["R"].tobytes() != r["R_ransac"].tobytes()
            if fl & vislam.PNP_FEW:
                assert int(r["n_inliers"]) < pp.min_inliers and fl == vislam.PNP_FEW
    assert seen == {0, vislam.PNP_REFINED, vislam.PNP_REFINE_REJECTED, vislam.PNP_FEW}
    c.close()


def test_tie_rule(vislam):
    """equal counts: the smallest slot 4 j + r wins -- between two copies of one sample whose first sits in the second wave, or in the second
    round of 256 with every sample before it skipped; and between two roots of one sample"""
    import torch
    X, xy = pr.make_scene("general", 40, 0.0, 0.0)[:2]
    c = vislam.Context(0, _params(vislam))
    rows = _Rows(torch, [(X, xy)], 40)
    for first, second, iters in ((70, 200, 256), (260, 290, 300), (255, 256, 257)):
        table = np.zeros((iters, 3), np.int32)                     # (0, 0, 0): skipped
        table[first] = table[second] = (10, 20, 30)
        pp, pq = _both(vislam, iters=iters)
        recs, masks = rows.run(vislam, torch, c, pp, _dev(torch, table))
        _check(recs, masks, rows, [pr.pnp(CAM, pq, X, xy, table)], (first, second))
        assert int(recs[0]["best_iter"]) == first and int(recs[0]["n_degenerate"]) == iters - 2 and int(recs[0]["n_inliers"]) == 40
    # two roots of one sample: the sample's three points and one correspondence nobody explains, so every pose counts exactly three
    pq = pr.default_params()
    hyp = pr.hypotheses(CAM, pq, X, xy, pr.make_draws(7))
    j = int(np.flatnonzero(hyp["live"].sum(1) >= 2)[0])
    idx = hyp["idx"][j]
    X4, xy4 = np.vstack([X[idx], [[0.0, 0.0, -5.0]]]), np.vstack([xy[idx], [[10.0, 10.0]]]).astype(np.float32)
    table = np.array([[0, 1, 2]], np.int32)
    pp, pq = _both(vislam, iters=1, min_inliers=4)
    h4 = pr.hypotheses(CAM, pq, X4, xy4, table)
    live = np.flatnonzero(h4["live"][0])
    assert len(live) >= 2 and set(h4["cnt"][0, live].tolist()) == {3}
    rows4 = _Rows(torch, [(X4, xy4)], 4)
    recs, masks = rows4.run(vislam, torch, c, pp, _dev(torch, table))
    _check(recs, masks, rows4, [pr.pnp(CAM, pq, X4, xy4, table)], "roots")
    assert int(recs[0]["best_root"]) == int(live[0]) and int(recs[0]["n_inliers"]) == 3 and int(recs[0]["flags"]) == vislam.PNP_FEW
    assert int(recs[0]["n_solutions"]) == len(live)
    c.close()


def test_single_call_equals_the_batch(vislam, probs, want, draws):
    """vis_pnp_ransac (host pointers, one problem) on EVERY row against what vis_pnp_batch gave, which is the restatement's"""
    c = vislam.Context(0, _params(vislam))
    for i in range(len(probs)):
        X, xy = probs[i]
        rec, mask = c.pnp_ransac(X, xy, draws)
        assert rec.tobytes() == want[i][0].tobytes() and mask.tobytes() == want[i][1].tobytes(), i
    pp = vislam.default_pnp_params()
    pp.iters = 0
    rec, mask = c.pnp_ransac(*probs[0], draws, pp)
    assert rec.tobytes() == pr.zero_record().tobytes() and not mask.any()
    rec, mask = c.pnp_ransac(np.zeros((0, 3)), np.zeros((0, 2), np.float32), draws)
    assert rec.tobytes() == pr.zero_record().tobytes() and len(mask) == 0
    c.close()


# ---------------------------------------------------------------------------------------------- the plan's frames
W, H, B = 752, 480, 16


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(2 * B)])
    g = f.copy()
    g[5] = g[B + 5] = 128                                          # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


@pytest.mark.parametrize("gate,sym", [(False, False), (True, False), (False, True)])
def test_batch_pnp_over_two_launches(vislam, orc, stream, draws, gate, sym):
    """sym: VIS_POSE_SYM -- the pose stage's list is the symmetric matches (stride = the keypoint capacity, hundreds of correspondences per
    pair), rebuilt here from the kNN getters by the oracle's filter"""
    import torch
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    CAP = 49
    if sym:
        p.pose_input, p.keypoint_capacity, CAP = 1, 2048, 2048
    MCAP = CAP + 3
    cam = pr.Camera(p.fx, p.cx, p.cy)
    pp, pq = _both(vislam, min_inliers=6)
    KEPT = vislam.MP_KEPT
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    carried = None
    dev = _dev(torch, stream[gate])
    d_draws = _dev(torch, draws)
    arg = lambda t: C.c_void_p(t.data_ptr())
    seen = dict(winners=0, linked=0, no_map=0, skipped=0, refined=0)
    for launch in range(2):
        pts, fl, sm = _filled(torch, B * CAP * 32), _filled(torch, B * CAP), _filled(torch, B * 16)
        out, link, mask = _filled(torch, (B + 1) * REC), _filled(torch, (B + 1) * 120), _filled(torch, B * MCAP + 64)
        c.batch_run(dev.data_ptr() + launch * B * W * H, B, vislam.STAGE_ALL)
        c.batch_triangulate(B, CAP, pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
        call = lambda pp_=pp, n=B, cap=CAP, mcap=MCAP, o=out: vislam.lib.vis_batch_pnp(c._h, C.byref(pp_), n, arg(d_draws), arg(pts), arg(fl), cap, KEPT, mcap,
                                                                                       arg(mask), arg(o), arg(link))
        if launch == 0:                                            # the refusals that need a plan, in the header's order
            bad = vislam.default_pnp_params()
            bad.min_inliers = 3
            assert call(pp_=bad, cap=CAP - 1, n=B - 1) == -1       # VIS_E_INVALID before anything else
            assert call(cap=CAP - 1, n=B - 1) == -4 and call(mcap=CAP - 1, n=B - 1) == -4          # VIS_E_CAPACITY before VIS_E_STATE
            assert call(n=B - 1) == -5                             # VIS_E_STATE: n differs
            assert (out.cpu().numpy() == FILL).all() and (link.cpu().numpy() == FILL).all()
        c.batch_pnp(B, d_draws.data_ptr(), pts.data_ptr(), fl.data_ptr(), CAP, out.data_ptr(), link.data_ptr(), KEPT, MCAP, mask.data_ptr(), pp)
        c.batch_sync()
        assert c.batch_status() == 0
        prev = c.batch_get_keyframes()
        poses, _, ngood = c.batch_results(B)
        kps = [c.batch_keypoints(i)[0] for i in range(B)]
        if sym:                                                    # the symmetric list of every pair: the oracle's filter on the device's kNN rows
            matches = []
            for i in range(B):
                kq = kps[prev[i]] if prev[i] >= 0 else carried if prev[i] == vislam.KF_CARRIED else None
                matches.append(np.zeros(0, vislam.DMATCH_DTYPE) if kq is None else orc.good_matches(p, kq, kps[i], *c.batch_knn(i))[1])
            assert max(len(m) for m in matches) > 49               # more than the grid filter would leave
        else:
            matches = [c.batch_matches(i)[0] for i in range(B)]
        carried = kps[-1]
        xy2 = [np.stack([kps[i]["x"][matches[i]["trainIdx"]], kps[i]["y"][matches[i]["trainIdx"]]], 1).astype(np.float32) for i in range(B)]
        h_pts = pts.cpu().numpy().view(vislam.MAP_POINT_DTYPE).reshape(B, CAP)
        h_fl = fl.cpu().numpy().reshape(B, CAP)
        raw_o, raw_l, raw_m = out.cpu().numpy(), link.cpu().numpy(), mask.cpu().numpy()
        assert (raw_o[B * REC:] == FILL).all() and (raw_l[B * 120:] == FILL).all() and (raw_m[B * MCAP:] == FILL).all()
        recs, links, masks = raw_o[:B * REC].view(vislam.PNP_RESULT_DTYPE), raw_l[:B * 120].view(vislam.PNP_LINK_DTYPE), raw_m[:B * MCAP].reshape(B, MCAP)
        rows = []
        for i in range(B):
            assert len(matches[i]) == (int(poses[i]["n_points"]) if sym else int(ngood[i])), (launch, i)
            X, xy, L = pr.link_rows(i, prev, matches, poses, h_pts, h_fl, xy2, KEPT)       # the numpy join of the getters and the triangulation rows
            rows.append((X, xy))
            w_rec, w_mask = pr.pnp(cam, pq, X, xy, draws)
            wL = pr.link_motion(L, w_rec, poses[int(L["q"])] if int(L["q"]) >= 0 else None)
            assert recs[i].tobytes() == w_rec.tobytes(), (launch, i, recs[i], w_rec)
            assert links[i].tobytes() == wL.tobytes(), (launch, i, links[i], wL)
            m = int(L["n_linked"])
            assert masks[i, :m].tobytes() == w_mask.tobytes() and (masks[i, m:] == FILL).all(), (launch, i)
            if int(w_rec["best_iter"]) >= 0:
                seen["winners"] += 1
                seen["refined"] += int(bool(int(w_rec["flags"]) & vislam.PNP_REFINED))
                R = np.asarray(wL["R_rel"]).reshape(3, 3)
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(float(wL["scale"]) - np.linalg.norm(wL["t_rel"])) <= 1e-12 * float(wL["scale"])
            seen["linked"] += int(m >= 4)
            seen["no_map"] += int(int(L["flags"]) == vislam.PNPL_NO_MAP)
            seen["skipped"] += int(0 <= int(L["q"]) < i - 1)
        assert (int(links[0]["flags"]) == vislam.PNPL_NO_MAP) == (launch == 1) and int(links[0]["n_linked"]) == 0
        # the records equal vis_pnp_batch on those rows
        again = _Rows(torch, rows, max(49, max(len(a) for a, _ in rows)))
        recs_b, masks_b = again.run(vislam, torch, c, pp, d_draws)
        assert recs_b.tobytes() == recs.tobytes()
    # a run without the pose stage has no map to join
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert call() == -5
    c.batch_sync()
    c.close()
    # a join that links nothing shows nothing: at least a quarter of the 32 frames must have a problem, a winner, and some a refined pose
    assert seen["no_map"] == 1 and seen["linked"] >= 8 and seen["winners"] >= 8 and seen["refined"] >= 1, seen
    assert (seen["skipped"] >= 1) == gate, seen
    print(f"\ngate {gate}, symmetric matches {sym}: {seen}")


def test_run_directory_writes_the_poses(vislam, stream, draws, tmp_path):
    """tools/run_directory.py --pnp: the CSV holds what vis_batch_triangulate + vis_batch_pnp give for the same frames in the same batches"""
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    frames = stream[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "pnp.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--pnp", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    dev, d_draws = _dev(torch, frames), _dev(torch, draws)
    recs, links = [], []
    for first in range(0, n, nb):
        pts, fl, sm = _filled(torch, nb * 49 * 32), _filled(torch, nb * 49), _filled(torch, nb * 16)
        out, link = _filled(torch, nb * REC), _filled(torch, nb * 120)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_triangulate(nb, 49, pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
        c.batch_pnp(nb, d_draws.data_ptr(), pts.data_ptr(), fl.data_ptr(), 49, out.data_ptr(), link.data_ptr())
        c.batch_sync()
        recs += list(out.cpu().numpy().view(vislam.PNP_RESULT_DTYPE))
        links += list(link.cpu().numpy().view(vislam.PNP_LINK_DTYPE))
    c.close()
    assert len(rows) == n == len(recs)
    posed = sum(int(r["best_iter"]) >= 0 for r in recs)
    assert j["pnp"]["posed"] == posed and j["pnp"]["no_map"] == 1 and j["pnp"]["linked"] == sum(int(l["n_linked"]) >= 4 for l in links)
    for k, (row, r, l) in enumerate(zip(rows, recs, links)):
        assert len(row) == 38 and int(row[0]) == k and int(row[1]) == 1403636579763555584 + 50000000 * k
        assert [int(v) for v in row[2:6]] == [int(l[f]) for f in ("q", "p", "n_linked", "flags")]
        assert [int(v) for v in row[7:12]] == [int(r[f]) for f in ("n_inliers", "n_inliers_refined", "best_iter", "best_root", "flags")]
        want = [l["scale"], r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(l["R_rel"]) + list(l["t_rel"])
        got = [row[6]] + row[12:]
        assert np.array([float(v) for v in got]).tobytes() == np.array(want, np.float64).tobytes(), k
