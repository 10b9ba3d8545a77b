"""GPU: homography RANSAC and the H-or-E model choice (vis_homography_batch / vis_find_homography / vis_batch_homography) against the
restatement tests/homography_ref.py.

Records and masks are compared byte for byte; score_h / score_e within relative (m - 1) 2^-52 (the terms are identical, and two
summation orders of m non-negative doubles differ by no more than that; the restatement sums in the kernel's order).  Output buffers are pre-filled with 0xEE and everything the call must not write is checked to keep it.

The stream of the plan tests: vis_synth_frame_parallax, canvas 2048 / seed 0xE0C00001, 752 x 480, fy = fx, frames 0 ... 15 (26 ... 42 good
matches per pair, tests/test_f2f_batch_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import homography_ref as hr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
W, H = 752, 480
FILL = 0xEE
REC = 112
E_SKEW = np.array([[0.0, -1.0, 0.2], [1.0, 0.0, -0.3], [-0.2, 0.3, 0.0]])      # rows too short for the oracle's RANSAC get this one


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _cam_params(vislam, **kw):
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _stream_params(vislam, **kw):
    p = vislam.default_params()
    p.fy = p.fx
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cam_of(p):
    return hr.Camera(p.fx, p.cx, p.cy)


def _same_but_scores(got, want, m, where):
    """one record against the restatement: everything but the scores byte for byte, the scores within (m - 1) 2^-52"""
    g, w = got.copy(), want.copy()
    for k in ("score_h", "score_e"):
        tol = max(m - 1, 0) * 2.0 ** -52 * abs(float(w[k]))
        assert abs(float(g[k]) - float(w[k])) <= tol, (where, k, float(g[k]), float(w[k]))
        g[k] = w[k] = 0.0
    assert g.tobytes() == w.tobytes(), (where, got, want)


class _Rows:
    """pairs as device rows of max_pts correspondences, with their E table"""
    def __init__(self, torch, pairs, max_pts, npts=None):
        self.pairs, self.n, self.max_pts = pairs, len(pairs), max_pts
        p1 = np.zeros((self.n, max_pts, 2), np.float32)
        p2 = np.zeros_like(p1)
        for i, (a, b, _) in enumerate(pairs):
            k = min(len(a), max_pts)
            p1[i, :k], p2[i, :k] = a[:k], b[:k]
        self.npts = np.array([len(a) for a, _, _ in pairs], np.int32) if npts is None else np.asarray(npts, np.int32)
        self.E = np.stack([np.asarray(e, np.float64).reshape(9) for _, _, e in pairs])
        self.d_p1, self.d_p2, self.d_npts, self.d_E = _dev(torch, p1), _dev(torch, p2), _dev(torch, self.npts), _dev(torch, self.E)

    def m(self, i):
        return min(max(int(self.npts[i]), 0), self.max_pts)

    def run(self, vislam, torch, c, hp, d_draws, with_E, with_mask=True):
        """(records, mask rows) of one vis_homography_batch; guard records / bytes checked"""
        n, cap = self.n, self.max_pts + 3
        out, mask = _filled(torch, (n + 2) * REC), _filled(torch, n * cap + 64)
        c.homography_batch(n, self.d_p1.data_ptr(), self.d_p2.data_ptr(), self.d_npts.data_ptr(), self.max_pts, d_draws.data_ptr(),
                           self.d_E.data_ptr() if with_E else 0, cap, mask.data_ptr() if with_mask else 0, out.data_ptr(), hp)
        c.batch_sync()
        raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
        assert (raw[n * REC:] == FILL).all() and (mraw[n * cap:] == FILL).all()
        rows = mraw[:n * cap].reshape(n, cap)
        for i in range(n):
            assert (rows[i, self.m(i):] == FILL).all(), i          # bytes beyond the pair's correspondences are left untouched
        if not with_mask:
            assert (mraw == FILL).all()
        return raw[:n * REC].view(vislam.HOMOGRAPHY_RESULT_DTYPE).copy(), rows


@pytest.fixture(scope="module")
def draws():
    return hr.make_draws(7)


@pytest.fixture(scope="module")
def pairs(vislam, orc):
    """(x1, x2, E) of hr.gpu_rows: outliers and noise on the rows of 8 and more, E from the oracle where it can run"""
    p = _cam_params(vislam)
    out = []
    for k, (cls, m) in enumerate(hr.gpu_rows(vislam.H_TILE)):
        x1, x2, _ = hr.make_rows(cls, m, 0.3 if k % 2 else 0.0, 0.25 if m >= 8 else 0.0)
        E = orc.essential_ransac(p, x1, x2)[0] if m >= 5 else E_SKEW
        out.append((x1, x2, np.asarray(E, np.float64).reshape(9)))
    n_small = 5 * len(pdc.CLASSES)
    out[n_small - 1] = out[n_small - 1][:2] + (np.zeros(9),)        # a zero E and a NaN E on two rows of 40
    out[n_small - 2] = out[n_small - 2][:2] + (np.full(9, np.nan),)
    return out


@pytest.fixture(scope="module")
def want(vislam, pairs, draws):
    """(with E, without E) -> per pair (record, mask) of the restatement at the default parameters, the iterations computed once per pair"""
    cam, hp = _cam_of(_cam_params(vislam)), hr.default_params()
    res = {True: [], False: []}
    for x1, x2, E in pairs:
        m = len(x1)
        if m < 4:
            for k in res:
                res[k].append((hr.zero_record(), np.zeros(m, np.uint8)))
            continue
        live, cnt = hr.iterations(cam, hp, x1, x2, draws)
        best, ndeg = hr.pick(live, cnt, 200)
        res[True].append(hr.finish(cam, hp, x1, x2, draws, best, ndeg, E))
        res[False].append(hr.finish(cam, hp, x1, x2, draws, best, ndeg, None))
    return res


@pytest.fixture(scope="module")
def launches(vislam, pairs):
    """the two row shapes: the rows of up to 40 as rows of 40 (one tile: the short-row kernel shape) with one count that must be clamped,
    and every row as rows of 2 tiles + 7 (the long-row shape)"""
    import torch
    T = vislam.H_TILE
    n_small = 5 * len(pdc.CLASSES)
    assert [len(a) for a, _, _ in pairs[n_small:]] == [T - 1] * 3 + [T] * 3 + [T + 1] * 3 + [2 * T + 7] * 3
    big = pairs[-3]                                                # general, 2 tiles + 7: its first 40 correspondences, announced as 1000
    short = _Rows(torch, pairs[:n_small] + [big], 40, [len(a) for a, _, _ in pairs[:n_small]] + [1000])
    long_ = _Rows(torch, pairs, 2 * T + 7)
    assert short.max_pts <= T < long_.max_pts
    return short, long_


@pytest.mark.parametrize("with_E", [True, False])
def test_records_and_masks_against_the_restatement(vislam, launches, want, draws, with_E):
    import torch
    short, long_ = launches
    p = _cam_params(vislam)
    cam, hp, hq = _cam_of(p), vislam.default_homography_params(), hr.default_params()
    c = vislam.Context(0, p)
    d_draws = _dev(torch, draws)
    models = set()
    for rows in (short, long_):
        recs, masks = rows.run(vislam, torch, c, hp, d_draws, with_E)
        for i in range(rows.n):
            m = rows.m(i)
            if rows is short and i == rows.n - 1:                  # the clamped row: the restatement on its first 40 correspondences
                x1, x2, E = rows.pairs[i]
                w_rec, w_mask = hr.homography(cam, hq, x1[:40], x2[:40], draws, E if with_E else None)
                assert m == 40
            else:
                w_rec, w_mask = want[with_E][i]
            _same_but_scores(recs[i], w_rec, m, (rows.max_pts, i))
            assert masks[i, :m].tobytes() == w_mask.tobytes(), (rows.max_pts, i)
            assert int(recs[i]["n_points"]) == (m if m >= 4 else 0)
            models.add(int(recs[i]["model"]))
        if rows is long_:
            assert all(int(r["best_iter"]) >= 0 for r in recs[-12:])
    assert models == ({0, 1, 2} if with_E else {0, 1})             # every outcome of the decision occurs
    # without a mask nothing but the records is written
    recs2, _ = long_.run(vislam, torch, c, hp, d_draws, with_E, with_mask=False)
    assert recs2.tobytes() == recs.tobytes()
    c.close()


def test_iteration_counts_at_lane_and_workgroup_edges(vislam, draws):
    """both kernel shapes hold 256 hypotheses per round (128 lanes x 2, 256 x 1)"""
    import torch
    p = _cam_params(vislam)
    cam = _cam_of(p)
    table = hr.make_draws(11, 257)
    three = [hr.make_rows(cls, 40, 0.3, 0.25)[:2] + (E_SKEW.reshape(9),) for cls in ("general", "plane", "static")]
    per_pair = [hr.iterations(cam, hr.default_params(), a, b, table, 257) for a, b, _ in three]
    c = vislam.Context(0, p)
    d_draws = _dev(torch, table)
    shapes = (_Rows(torch, three, 40), _Rows(torch, three, vislam.H_TILE + 1))
    for iters in (1, 63, 64, 65, 255, 256, 257, 200):
        hp, hq = vislam.default_homography_params(), hr.default_params()
        hp.iters = hq.iters = iters
        for rows in shapes:
            recs, masks = rows.run(vislam, torch, c, hp, d_draws, True)
            for i, (a, b, E) in enumerate(three):
                best, ndeg = hr.pick(*per_pair[i], iters)
                w_rec, w_mask = hr.finish(cam, hq, a, b, table, best, ndeg, E)
                _same_but_scores(recs[i], w_rec, 40, (iters, rows.max_pts, i))
                assert masks[i, :40].tobytes() == w_mask.tobytes(), (iters, rows.max_pts, i)
    c.close()


@pytest.mark.parametrize("first", [70, 130, 260])
def test_tie_goes_to_the_first_live_iteration(vislam, first):
    """static rows: every live hypothesis counts all m points.  The table's draws repeat an index up to iteration `first`, which lies in
    the second wave (70), in a lane's second slot of the short-row shape (130) and in the second round of either shape (260)"""
    import torch
    p = _cam_params(vislam)
    cam = _cam_of(p)
    table = hr.make_draws(13, 300)
    table[:first, 1] = table[:first, 0]
    hp, hq = vislam.default_homography_params(), hr.default_params()
    hp.iters = hq.iters = 300
    three = [hr.make_rows("static", m, 0.0, 0.0)[:2] + (np.zeros(9),) for m in (40, 41, 47)]
    c = vislam.Context(0, p)
    d_draws = _dev(torch, table)
    for rows in (_Rows(torch, three, 47), _Rows(torch, three, vislam.H_TILE + 1)):
        recs, _ = rows.run(vislam, torch, c, hp, d_draws, False)
        for i, (a, b, _) in enumerate(three):
            live, cnt = hr.iterations(cam, hq, a, b, table, 300)
            assert not live[:first].any() and live[first] and (cnt[live] == len(a)).all() and live.sum() > 1
            assert int(recs[i]["best_iter"]) == first and int(recs[i]["n_inliers"]) == len(a), (rows.max_pts, i, recs[i])
            assert int(recs[i]["n_degenerate"]) == int(300 - live.sum())
    c.close()


def test_single_call_equals_the_batch(vislam, launches, pairs, draws):
    import torch
    _, long_ = launches
    p = _cam_params(vislam)
    hp = vislam.default_homography_params()
    c = vislam.Context(0, p)
    d_draws = _dev(torch, draws)
    for with_E in (True, False):
        recs, masks = long_.run(vislam, torch, c, hp, d_draws, with_E)
        for i, (x1, x2, E) in enumerate(pairs):
            if not with_E and i % 7:
                continue
            rec, mask = c.find_homography(x1, x2, draws, E if with_E else None, hp)
            assert rec.tobytes() == recs[i].tobytes(), (with_E, i, rec, recs[i])
            assert mask.tobytes() == masks[i, :len(x1)].tobytes(), (with_E, i)
    rec, mask = c.find_homography(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), draws, None, hp)
    assert rec.tobytes() == hr.zero_record().tobytes() and len(mask) == 0
    c.close()


def test_two_runs_are_byte_identical(vislam, launches, draws):
    import torch
    p = _cam_params(vislam)
    hp = vislam.default_homography_params()
    d_draws = _dev(torch, draws)
    got = []
    for _ in range(2):
        c = vislam.Context(0, p)
        got.append([(r.tobytes(), m.tobytes()) for r, m in (rows.run(vislam, torch, c, hp, d_draws, True) for rows in launches)])
        c.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------------------------------------- the plan's pairs
@pytest.fixture(scope="module")
def frames16(vislam, canvas):
    return np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(16)])


def _plan_run(vislam, torch, frames, p, stages, d_draws, call=True):
    """one launch of the whole stream: (records, mask rows, pose records, per-frame correspondences rebuilt from the getters or None)"""
    n = len(frames)
    hp = vislam.default_homography_params()
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    c.batch_reset()
    dev = _dev(torch, frames)
    out, mask = _filled(torch, n * REC), _filled(torch, n * 49)
    poses = np.zeros(n, vislam.POSE_RESULT_DTYPE)
    c.batch_run(dev.data_ptr(), n, stages)
    if call:
        assert vislam.lib.vis_batch_homography(c._h, C.byref(hp), n - 1, C.c_void_p(d_draws.data_ptr()), 49, C.c_void_p(mask.data_ptr()),
                                               C.c_void_p(out.data_ptr())) == -5          # VIS_E_STATE: n differs
        assert vislam.lib.vis_batch_homography(c._h, C.byref(hp), n, C.c_void_p(d_draws.data_ptr()), 48, C.c_void_p(mask.data_ptr()),
                                               C.c_void_p(out.data_ptr())) == -4          # VIS_E_CAPACITY: below the plan's 49 per pair
        c.batch_homography(n, d_draws.data_ptr(), 49, mask.data_ptr(), out.data_ptr(), hp)
    if stages & vislam.STAGE_POSE:
        c.batch_results_async(n, poses.ctypes.data)
    c.batch_sync()
    assert c.batch_status() == 0
    links = c.batch_get_keyframes()
    kps = [c.batch_keypoints(i)[0] for i in range(n)]
    corr = []
    for i in range(n):
        if links[i] < 0:
            corr.append(None)                                      # one launch after a reset: no carried frame
            continue
        good, _ = c.batch_matches(i)
        kq, kt = kps[links[i]], kps[i]
        corr.append((np.stack([kq["x"][good["queryIdx"]], kq["y"][good["queryIdx"]]], 1).astype(np.float32),
                     np.stack([kt["x"][good["trainIdx"]], kt["y"][good["trainIdx"]]], 1).astype(np.float32)))
    c.close()
    return out.cpu().numpy().view(vislam.HOMOGRAPHY_RESULT_DTYPE), mask.cpu().numpy().reshape(n, 49), poses, corr


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("with_pose", [True, False])
def test_plan_pairs_equal_the_device_pointer_call(vislam, frames16, draws, gate, with_pose):
    import torch
    p = _stream_params(vislam, keyframe_min_points=1) if gate else _stream_params(vislam)
    frames = frames16.copy()
    if gate:
        frames[4] = 128                                            # a blank frame is refused: frame 5 is paired with frame 3
    stages = vislam.STAGE_DETECT | vislam.STAGE_MATCH | (vislam.STAGE_POSE if with_pose else 0)
    d_draws = _dev(torch, draws)
    recs, masks, poses, corr = _plan_run(vislam, torch, frames, p, stages, d_draws)
    no_pair = [i for i in range(16) if corr[i] is None]
    assert no_pair == ([0, 4] if gate else [0])
    rows = _Rows(torch, [(np.zeros((0, 2), np.float32),) * 2 + (np.zeros(9),) if cr is None else (cr[0], cr[1], poses[i]["E"])
                         for i, cr in enumerate(corr)], 49)
    c = vislam.Context(0, p)
    w_recs, w_masks = rows.run(vislam, torch, c, vislam.default_homography_params(), d_draws, with_pose)
    c.close()
    assert recs.tobytes() == w_recs.tobytes()
    for i in range(16):
        m = rows.m(i)
        assert masks[i, :m].tobytes() == w_masks[i, :m].tobytes() and (masks[i, m:] == FILL).all(), i
        if corr[i] is None:
            assert recs[i].tobytes() == hr.zero_record().tobytes(), i
        else:
            assert int(recs[i]["n_points"]) == m >= 4 and int(recs[i]["best_iter"]) >= 0, (i, recs[i])
            assert (int(recs[i]["n_inliers_e"]) > 0) == with_pose or int(poses[i]["n_inliers"]) == 0, (i, recs[i])
    print(f"gate {gate}, pose {with_pose}: models {[int(r['model']) for r in recs]}, ratios {[round(hr.ratio(r), 3) for r in recs[1:]]}")
    if with_pose:
        _, _, poses0, _ = _plan_run(vislam, torch, frames, p, stages, d_draws, call=False)
        assert poses.tobytes() == poses0.tobytes()                 # the pose records do not notice the call


def _pipelined(vislam, torch, dev, p, d_draws, sync_each, steps=3, B=5):
    hp = vislam.default_homography_params()
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    outs = [(_filled(torch, B * REC), _filled(torch, B * 49)) for _ in range(steps)]
    poses = [np.zeros(B, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        c.batch_run(dev.data_ptr() + k * B * W * H, B, vislam.STAGE_ALL)
        if sync_each:
            c.batch_sync()
        c.batch_homography(B, d_draws.data_ptr(), 49, outs[k][1].data_ptr(), outs[k][0].data_ptr(), hp)
        if sync_each:
            c.batch_sync()
        c.batch_results_async(B, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    recs = [(o.cpu().numpy().tobytes(), m.cpu().numpy().tobytes()) for o, m in outs]
    c.close()
    return recs, [q.tobytes() for q in poses]


def test_a_run_queued_before_the_sync_changes_nothing(vislam, frames16, draws):
    import torch
    p = _stream_params(vislam)
    dev = _dev(torch, frames16[:15])
    d_draws = _dev(torch, draws)
    qr, qp = _pipelined(vislam, torch, dev, p, d_draws, False)
    sr, sp = _pipelined(vislam, torch, dev, p, d_draws, True)
    assert qr == sr and qp == sp
    recs = np.frombuffer(b"".join(r for r, _ in qr), vislam.HOMOGRAPHY_RESULT_DTYPE)
    assert (recs["best_iter"] >= 0).sum() == 14 and (recs["n_inliers_e"] > 0).sum() >= 10      # not a comparison of empty records


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_models(vislam, frames16, tmp_path):
    """tools/run_directory.py --models: the CSV holds what vis_batch_homography gives for the same frames in the same batches"""
    import json
    import os
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, B = 12, 5
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames16[t].tobytes())
    csv = tmp_path / "models.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(B),
                        "--models", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    # the same launches in this process (the tool's parameters: ORB::create(200), fy = fx; its draws)
    c = vislam.Context(0, _stream_params(vislam, nfeatures=200, w_size=W, h_size=H))
    c.batch_plan(W, H, W, B)
    dev, d_draws = _dev(torch, frames16[:n]), _dev(torch, hr.make_draws(7))
    want = []
    for first in range(0, n, B):
        nb = min(B, n - first)
        out = _filled(torch, nb * REC)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_homography(nb, d_draws.data_ptr(), 0, 0, out.data_ptr())
        c.batch_sync()
        recs = out.cpu().numpy().view(vislam.HOMOGRAPHY_RESULT_DTYPE)
        want += [(first + i, recs[i].copy()) for i in range(nb) if int(recs[i]["n_points"]) > 0]
    c.close()
    assert len(rows) == len(want) == n - 1                         # every frame but the first has a pair (the second batch's first: the carried one)
    totals = {k: 0 for k in vislam.MODEL_NAMES}
    for row, (frame, rec) in zip(rows, want):
        assert int(row[0]) == frame and int(row[1]) == 1403636579763555584 + 50000000 * frame
        assert row[2] == vislam.MODEL_NAMES[int(rec["model"])]
        assert [int(v) for v in row[3:6] + row[8:10]] == [int(rec[k]) for k in ("n_points", "n_inliers", "n_inliers_e", "best_iter", "n_degenerate")]
        assert np.array([float(v) for v in row[6:8] + row[10:19]]).tobytes() == np.concatenate([[rec["score_h"], rec["score_e"]], rec["H"]]).tobytes()
        totals[row[2]] += 1
    assert j["models"] == totals and j["models_csv"] == str(csv)
