"""GPU: the pose of a homography (vis_homography_pose / vis_homography_pose_batch / vis_batch_homography_pose) against the restatement
tests/homography_pose_ref.py: whole records byte for byte -- every integer and every double.  Output buffers are pre-filled with 0xEE and
guard records on both sides of d_out must keep it.

H and mask of a row come from vis_find_homography (byte-identical to its own restatement, tests/test_homography_gpu.py); the rows that probe
the stride, workgroup and nsplit edges are prefixes of ONE plane scene of 1100 correspondences and share its H, so that a row of 1 or 3
correspondences still is a PLANE pair.  The stream of the plan tests is that of tests/test_homography_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import homography_pose_ref as hpr
import homography_ref as hr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
W, H = 752, 480
FILL = 0xEE
REC, HREC = 320, 112
EDGES = (1, 3, 63, 64, 65, 255, 256, 257, 513, 1100)     # a wave, the workgroup's 256, two strides, nsplit 2 (rows above 1024)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _cam_params(vislam):
    return pdc.set_mode(vislam.default_params(), "adaptive")


def _stream_params(vislam, **kw):
    p = vislam.default_params()
    p.fy = p.fx
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _small_rot(seed):
    return np.asarray(pdc._rodrigues(np.random.default_rng([909, seed]).normal(0, 0.03, 3)).T, np.float32)


class Row:
    """one pair: correspondences, homography record, mask, hint, and the restatement's decomposition and vote table (computed once)"""
    def __init__(self, cam, name, x1, x2, hrec, mask, rot, table=None):
        self.name, self.x1, self.x2, self.hrec, self.mask, self.rot = name, x1, x2, hrec, np.ascontiguousarray(mask, np.uint8), rot
        self.cam, self.m = cam, len(x1)
        self.table = table
        if table is None and int(hrec["best_iter"]) >= 0 and self.m >= 1 and np.isfinite(hrec["H"]).all():
            dec = hpr.decompose(hrec["H"], hpr.default_params().min_t_over_d)
            if dec["kind"] == hpr.HP_PLANE:
                self.table = hpr.vote_table(dec, hr.normalise(cam, x1, x2), hpr.default_params().max_cos_parallax)

    def want(self, with_mask, with_hint, m=None):
        m = self.m if m is None else m
        t = None if self.table is None else (self.table[0][:, :m], self.table[1][:, :m])
        return hpr.hpose(self.cam, hpr.default_params(), self.hrec, self.x1[:m], self.x2[:m], self.mask[:m] if with_mask else None,
                         self.rot if with_hint else None, t)


@pytest.fixture(scope="module")
def rows(vislam):
    """the class rows (13 classes at M 4, 40, 300; noise and outliers on every other one), the edge rows (prefixes of one plane scene), and
    rows whose homography record has best_iter = -1 in between"""
    p = _cam_params(vislam)
    cam = hr.Camera(p.fx, p.cx, p.cy)
    c = vislam.Context(0, p)
    draws = hr.make_draws(7)
    out = []
    for k, (m, cls) in enumerate((m, cls) for m in (4, 40, 300) for cls in pdc.CLASSES):
        noise = 0.3 if k % 2 else 0.0
        x1, x2, _ = hr.make_rows(cls, m, noise, 0.25 if m >= 40 and k % 3 else 0.0)
        hrec, mask = c.find_homography(x1, x2, draws)
        rot = np.asarray(hpr.truth(cls, m, noise)[0].T, np.float32) if cls in hr.H_LIST else _small_rot(k)
        out.append(Row(cam, f"{cls}-{m}", x1, x2, hrec, mask, rot))
        if k % 5 == 2:
            out.append(Row(cam, f"none-{k}", x1, x2, hr.zero_record(), mask, rot))
    x1, x2, _ = hr.make_rows("plane", EDGES[-1], 0.0, 0.25)
    hrec, mask = c.find_homography(x1, x2, draws)
    c.close()
    big = Row(cam, f"plane-{EDGES[-1]}", x1, x2, hrec, mask, np.asarray(hpr.truth("plane", EDGES[-1], 0.0)[0].T, np.float32))
    assert big.table is not None
    for m in EDGES[:-1]:
        out.append(Row(cam, f"plane-{m}", x1[:m], x2[:m], hrec, mask[:m], big.rot, (big.table[0][:, :m], big.table[1][:, :m])))
    out.append(big)
    return out


def _launch(vislam, torch, c, rows, max_pts, with_mask, with_hint, npts=None):
    """records of one vis_homography_pose_batch over `rows` as device rows of max_pts; the guard records on both sides are checked"""
    n, cap = len(rows), max_pts + 5
    p1, p2 = np.zeros((n, max_pts, 2), np.float32), np.zeros((n, max_pts, 2), np.float32)
    mk = np.full((n, cap), 1, np.uint8)
    for i, r in enumerate(rows):
        k = min(r.m, max_pts)
        p1[i, :k], p2[i, :k], mk[i, :k] = r.x1[:k], r.x2[:k], r.mask[:k]
    npts = np.array([r.m for r in rows], np.int32) if npts is None else np.asarray(npts, np.int32)
    hrecs = np.frombuffer(b"".join(r.hrec.tobytes() for r in rows), np.uint8).copy()
    assert len(hrecs) == n * HREC
    rot = np.stack([r.rot.reshape(9) for r in rows]).astype(np.float32)
    d = [_dev(torch, a) for a in (hrecs, p1, p2, npts, mk, rot)]
    out = _filled(torch, (n + 2) * REC)
    c.homography_pose_batch(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max_pts, cap,
                            d[4].data_ptr() if with_mask else 0, d[5].data_ptr() if with_hint else 0, out.data_ptr() + REC)
    c.batch_sync()
    raw = out.cpu().numpy()
    assert (raw[:REC] == FILL).all() and (raw[(n + 1) * REC:] == FILL).all()
    return raw[REC:(n + 1) * REC].view(vislam.HPOSE_RESULT_DTYPE).copy()


def _check(got, want, where):
    assert got.tobytes() == want.tobytes(), (where, got, want)


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("with_hint", [True, False])
def test_records_against_the_restatement(vislam, rows, with_mask, with_hint):
    import torch
    c = vislam.Context(0, _cam_params(vislam))
    kinds, flags = set(), 0
    # rows of 1100 (two workgroups per pair) hold every row; rows of 300 (one workgroup) hold the 1100-row clamped to its first 300
    for max_pts in (EDGES[-1], 300):
        sel = [r for r in rows if r.m <= max_pts or r.m == EDGES[-1]]
        recs = _launch(vislam, torch, c, sel, max_pts, with_mask, with_hint)
        for r, got in zip(sel, recs):
            m = min(r.m, max_pts)
            if r.name.split("-")[0] in hr.ROBUST_ONLY:             # both models or neither explain these: they only have to run clean
                assert int(got["kind"]) in (0, 1, 2) and -1 <= int(got["solution"]) <= 3 and int(got["n_points"]) in (0, m), (r.name, got)
                continue
            _check(got, r.want(with_mask, with_hint, m), (max_pts, r.name))
            kinds.add(int(got["kind"]))
            flags |= int(got["flags"])
            if r.name.startswith("none"):
                assert got.tobytes() == hpr.zero_record().tobytes()
    assert kinds == {0, 1, 2}
    assert flags & (hpr.HPF_HINTED if with_hint else hpr.HPF_AMBIGUOUS) and not flags & (hpr.HPF_AMBIGUOUS if with_hint else hpr.HPF_HINTED)
    c.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batches_equal_the_single_call(vislam, rows, n):
    """the lane-per-pair kernel's edges: every pair of a batch of n equals its single-call record (mask and hint given)"""
    import torch
    c = vislam.Context(0, _cam_params(vislam))
    small = [r for r in rows if r.m <= 65]
    assert len(small) >= 20 and any(r.table is not None for r in small)
    single = [c.homography_pose(r.hrec, r.x1, r.x2, r.mask, r.rot.reshape(3, 3)) for r in small]
    sel = [small[(7 * i) % len(small)] for i in range(n)]
    recs = _launch(vislam, torch, c, sel, 65, True, True)
    for i in range(n):
        _check(recs[i], single[(7 * i) % len(small)], (n, i, sel[i].name))
    # no mask, no hint, and no correspondences
    r = next(r for r in small if r.table is not None and r.m >= 40)
    _check(c.homography_pose(r.hrec, r.x1, r.x2), r.want(False, False), r.name)
    z = c.homography_pose(r.hrec, r.x1[:0], r.x2[:0])
    assert z.tobytes() == hpr.zero_record().tobytes()
    c.close()


def test_votes_are_the_front_flags_of_the_map_points(vislam, rows):
    """vis_triangulate under the record's (R, t) marks exactly n_good[solution] masked correspondences VIS_MP_FRONT: the same device function"""
    import torch
    c = vislam.Context(0, _cam_params(vislam))
    sel = rows                                                     # every row, the one of 1100 (votes summed over two workgroups) included
    recs = _launch(vislam, torch, c, sel, EDGES[-1], True, True)
    n_plane = 0
    for r, rec in zip(sel, recs):
        if int(rec["kind"]) != vislam.HP_PLANE:
            continue
        n_plane += 1
        for R, t, k in ((rec["R"], rec["t"], int(rec["solution"])), (rec["R2"], rec["t2"], int(rec["second"]))):
            _, fl, _ = c.triangulate(R, t, r.x1, r.x2, r.mask)
            front = int((((fl & vislam.MP_FRONT) != 0) & (r.mask != 0)).sum())
            assert front == int(rec["n_good"][k]), (r.name, k, front, rec["n_good"])
    assert n_plane >= 10 and int(recs[-1]["kind"]) == vislam.HP_PLANE and sel[-1].m == EDGES[-1]
    c.close()


def test_zero_theta_correspondences(vislam):
    """H = diag(1, 1, 2) = I + e_z e_z^T decomposes exactly into R = I, t / d = e_z, n = e_z (both rotations coincide), the candidates under
    which pose_degenerate_cases' grid correspondences meet theta == 0 in the 4 x 4 decomposition: there the twin with -t is decomposed on its
    own.  They are spliced into rows of that plane at the positions of pdc.zero_theta_rows (a wave of its own, the second wave, both
    workgroups of a split row); the votes must still be the restatement's, which decomposes every candidate separately.
    What this shows is that such rows run clean and match.  It cannot tell whether the fallback pass runs: for these correspondences the
    (good, parallax) bits taken from the first decomposition equal those of the twin decomposed on its own, so a kernel without the
    fallback would pass too -- the limit tests/test_pose_degenerate_ref.py states for the pose stage's own zero-theta rows."""
    import torch
    p = pdc.zt_params(vislam.default_params())
    cam = hr.Camera(p.fx, p.cx, p.cy)
    hrec = hr.zero_record()
    hrec["H"], hrec["best_iter"] = np.diag([1.0, 1.0, 2.0]).reshape(9), 0
    dec = hpr.decompose(hrec["H"], 0.05)
    assert dec["kind"] == hpr.HP_PLANE and dec["R"][0] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and dec["t"][0] == [0.0, 0.0, 1.0]
    pick = pdc.quarters_to_pixels([(-8, 0, 0, 4), (-7, 0, 0, -4), (4, 3, -4, 4), (-4, -5, -4, -4)])
    made = []
    for m, at, seed in ((64, [37], 1), (65, [64], 2), (1100, [0, 255, 256, 1099], 3)):
        q = np.random.default_rng([515, seed]).uniform(-2, 2, (m, 2))
        x1 = (pdc.ZT_C + 64.0 * q).astype(np.float32)
        x2 = (pdc.ZT_C + 32.0 * q).astype(np.float32)               # (x, y, 1) -> (x, y, 2): half the normalised coordinates
        x1, x2 = pdc._splice((x1, x2), pick, at)
        made.append(Row(cam, f"zt-{m}", x1, x2, hrec, np.ones(m, np.uint8), np.eye(3, dtype=np.float32)))
    for name in ("only_zero_theta_I", "only_zero_theta_union"):
        x1, x2 = pdc.zero_theta_rows()[name]
        made.append(Row(cam, name, x1, x2, hrec, np.ones(len(x1), np.uint8), np.eye(3, dtype=np.float32)))
    c = vislam.Context(0, p)
    recs = _launch(vislam, torch, c, made, 1100, True, False)
    for r, got in zip(made, recs):
        _check(got, r.want(True, False), r.name)
        assert int(got["kind"]) == hpr.HP_PLANE
    assert int(recs[0]["n_good"][0]) > 32 and int(recs[2]["n_good"][0]) > 550   # the plane's own points are in front under (I, +e_z)
    c.close()


def test_two_runs_are_byte_identical(vislam, rows):
    import torch
    got = []
    for _ in range(2):
        c = vislam.Context(0, _cam_params(vislam))
        got.append(_launch(vislam, torch, c, rows, EDGES[-1], True, True).tobytes())
        c.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------------------------------------- the plan's pairs
@pytest.fixture(scope="module")
def frames16(vislam, canvas):
    return np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(16)])


def _rots(n):
    return np.stack([_small_rot(100 + i).reshape(9) for i in range(n)]).astype(np.float32)


@pytest.mark.parametrize("gate", [False, True])
def test_plan_pairs_equal_the_device_pointer_call(vislam, frames16, gate):
    import torch
    p = _stream_params(vislam, keyframe_min_points=1) if gate else _stream_params(vislam)
    frames = frames16.copy()
    if gate:
        frames[4] = 128                                            # a blank frame is refused: frame 5 is paired with frame 3
    n = 16
    hp, hq = vislam.default_homography_params(), vislam.default_hpose_params()
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    c.batch_reset()
    dev, d_draws, d_rot = _dev(torch, frames), _dev(torch, hr.make_draws(7)), _dev(torch, _rots(n))
    hrec, mask, out = _filled(torch, n * HREC), _filled(torch, n * 49), _filled(torch, (n + 2) * REC)
    c.batch_run(dev.data_ptr(), n, vislam.STAGE_ALL)
    c.batch_homography(n, d_draws.data_ptr(), 49, mask.data_ptr(), hrec.data_ptr(), hp)
    v = lambda t: C.c_void_p(t.data_ptr())
    assert vislam.lib.vis_batch_homography_pose(c._h, C.byref(hq), n - 1, v(hrec), 49, v(mask), v(d_rot), v(out)) == -5   # VIS_E_STATE: n differs
    assert vislam.lib.vis_batch_homography_pose(c._h, C.byref(hq), n, v(hrec), 48, v(mask), v(d_rot), v(out)) == -4       # VIS_E_CAPACITY
    c.batch_homography_pose(n, hrec.data_ptr(), 49, mask.data_ptr(), d_rot.data_ptr(), out.data_ptr() + REC, hq)
    c.batch_sync()
    assert c.batch_status() == 0
    links = c.batch_get_keyframes()
    kps = [c.batch_keypoints(i)[0] for i in range(n)]
    p1, p2, npts = np.zeros((n, 49, 2), np.float32), np.zeros((n, 49, 2), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        if links[i] < 0:
            continue
        good, _ = c.batch_matches(i)
        kq, kt = kps[links[i]], kps[i]
        npts[i] = len(good)
        p1[i, :npts[i]] = np.stack([kq["x"][good["queryIdx"]], kq["y"][good["queryIdx"]]], 1)
        p2[i, :npts[i]] = np.stack([kt["x"][good["trainIdx"]], kt["y"][good["trainIdx"]]], 1)
    assert [i for i in range(n) if links[i] < 0] == ([0, 4] if gate else [0])
    raw = out.cpu().numpy()
    assert (raw[:REC] == FILL).all() and (raw[(n + 1) * REC:] == FILL).all()
    recs = raw[REC:(n + 1) * REC].view(vislam.HPOSE_RESULT_DTYPE)
    d = [_dev(torch, a) for a in (p1, p2, npts)]
    out2 = _filled(torch, n * REC)
    c.homography_pose_batch(n, hrec.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 49, 49, mask.data_ptr(), d_rot.data_ptr(),
                            out2.data_ptr(), hq)
    c.batch_sync()
    recs2 = out2.cpu().numpy().view(vislam.HPOSE_RESULT_DTYPE)
    assert recs.tobytes() == recs2.tobytes()
    for i in range(n):
        if links[i] < 0:
            assert recs[i].tobytes() == hpr.zero_record().tobytes(), i
        else:
            assert int(recs[i]["n_points"]) == npts[i] and int(recs[i]["kind"]) in (1, 2), (i, recs[i])
    print(f"gate {gate}: kinds {[int(r['kind']) for r in recs]}, t_norm {[round(float(r['t_norm']), 4) for r in recs]}")
    c.close()


def _pipelined(vislam, torch, dev, p, d_draws, d_rot, sync_each, steps=3, B=5):
    hp, hq = vislam.default_homography_params(), vislam.default_hpose_params()
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    outs = [(_filled(torch, B * HREC), _filled(torch, B * 49), _filled(torch, B * REC)) for _ in range(steps)]
    poses = [np.zeros(B, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        c.batch_run(dev.data_ptr() + k * B * W * H, B, vislam.STAGE_ALL)
        if sync_each:
            c.batch_sync()
        c.batch_homography(B, d_draws.data_ptr(), 49, outs[k][1].data_ptr(), outs[k][0].data_ptr(), hp)
        c.batch_homography_pose(B, outs[k][0].data_ptr(), 49, outs[k][1].data_ptr(), d_rot.data_ptr(), outs[k][2].data_ptr(), hq)
        if sync_each:
            c.batch_sync()
        c.batch_results_async(B, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    recs = [tuple(t.cpu().numpy().tobytes() for t in o) for o in outs]
    c.close()
    return recs, [q.tobytes() for q in poses]


def test_a_run_queued_before_the_sync_changes_nothing(vislam, frames16):
    import torch
    p = _stream_params(vislam)
    dev, d_draws, d_rot = _dev(torch, frames16[:15]), _dev(torch, hr.make_draws(7)), _dev(torch, _rots(5))
    qr, qp = _pipelined(vislam, torch, dev, p, d_draws, d_rot, False)
    sr, sp = _pipelined(vislam, torch, dev, p, d_draws, d_rot, True)
    assert qr == sr and qp == sp
    recs = np.frombuffer(b"".join(r[2] for r in qr), vislam.HPOSE_RESULT_DTYPE)
    assert (recs["kind"] > 0).sum() == 14                          # not a comparison of empty records


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_hposes(vislam, frames16, tmp_path):
    """tools/run_directory.py --hposes: one line per pair, holding what the two calls give for the same frames in the same batches"""
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
    csv = tmp_path / "hposes.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(B),
                        "--hposes", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    lines = [l.split(",") for l in csv.read_text().splitlines()]
    c = vislam.Context(0, _stream_params(vislam, nfeatures=200, w_size=W, h_size=H))
    c.batch_plan(W, H, W, B)
    dev, d_draws = _dev(torch, frames16[:n]), _dev(torch, hr.make_draws(7))
    want = []
    for first in range(0, n, B):
        nb = min(B, n - first)
        hrec, mask, out = _filled(torch, nb * HREC), _filled(torch, nb * 49), _filled(torch, nb * REC)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_homography(nb, d_draws.data_ptr(), 49, mask.data_ptr(), hrec.data_ptr())
        c.batch_homography_pose(nb, hrec.data_ptr(), 49, mask.data_ptr(), 0, out.data_ptr())
        c.batch_sync()
        recs = out.cpu().numpy().view(vislam.HPOSE_RESULT_DTYPE)
        want += [(first + i, recs[i].copy()) for i in range(nb) if int(recs[i]["kind"]) != vislam.HP_NONE]
    c.close()
    assert len(lines) == len(want) == n - 1                        # every frame but the first has a pair
    totals = {k: 0 for k in vislam.HP_KIND_NAMES}
    for row, (frame, rec) in zip(lines, want):
        assert int(row[0]) == frame and int(row[1]) == 1403636579763555584 + 50000000 * frame
        assert row[2] == vislam.HP_KIND_NAMES[int(rec["kind"])]
        ints = [int(rec[k]) for k in ("flags", "solution", "second", "n_points", "n_tested", "n_parallax")] + [int(v) for v in rec["n_good"]]
        assert [int(v) for v in row[3:13]] == ints
        dbl = np.concatenate([rec["sv"], [rec["t_norm"]], rec["R"], rec["t"], rec["n"], rec["R2"], rec["t2"], rec["n2"]])
        assert np.array([float(v) for v in row[13:]]).tobytes() == dbl.tobytes()
        totals[row[2]] += 1
    assert j["hposes"] == totals and j["hposes_csv"] == str(csv)
