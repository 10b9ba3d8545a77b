"""GPU: the two-view polish (vis_essential_polish_batch / vis_essential_polish / vis_batch_essential_polish) and vis_batch_triangulate_from
against the restatement tests/essential_polish_ref.py.

Records, pose records and masks are compared BYTE FOR BYTE, every integer and every double.  Output buffers are pre-filled with 0xEE; points beyond
a row's count are NaN and input mask bytes beyond it 0xFF, so an over-read shows as a different record and an over-write as a changed filler; the
pose records the device starts from hold NaN / junk outside R and t, which pose_out must carry over.  One list of 37 problems serves every
test: its rows run at max_pts 640 (four waves a pair) and, those of at most 64 points, again at max_pts 64 (one wave a pair); a restated row is
computed once per (row, parameters, mask) and shared.  The start of a row is the CPU oracle's RANSAC winner of its scene, every other row turned
by a few milliradians.

The plan path runs on 16 frames of the parallax stream (vis_synth_frame_parallax, 752 x 480, fy = fx), gate off and on."""
import ctypes as C

import numpy as np
import pytest

import essential_polish_ref as epr
import essential_refine_ref as er
import homography_ref as hr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC, PREC = 224, 192
CAM = er.Camera()
LENGTHS = (0, 5, 6, 8, 63, 64, 65, 255, 256, 257, 511, 513, 600)
N = 37


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
    a, b = vislam.default_epolish_params(), epr.default_params()
    for k, v in kw.items():
        setattr(a, k, v)
        setattr(b, k, v)
    return a, b


def _problem(vislam, orc, cls, m, noise, outliers, seed, turn):
    """(x1, x2, start[12], mask) of a scene: the oracle's winner, optionally turned by `turn` radians about (1, -1, 1) / sqrt 3"""
    x1, x2 = er.make_scene(cls, m, noise, outliers, seed)[:2]
    p = _params(vislam)
    E, mask, _, _ = orc.essential_ransac(p, x1, x2)
    R, t, _ = orc.recover_pose(p, E, x1, x2)
    if turn and np.isfinite(R).all():
        R = pdc._rodrigues(turn * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)) @ R
    return x1, x2, np.concatenate([R.reshape(9), t]), mask


@pytest.fixture(scope="module")
def probs(vislam, orc):
    """37 problems: the 13 row lengths with classes, noise, outliers and the turn of the start varied (rows 0 ... 25), then the special rows"""
    out = []
    for i in range(26):
        out.append(_problem(vislam, orc, er.MOVING[i % 3] if i % 13 > 2 else er.CLASSES[i % 5], LENGTHS[i % 13], (1.0, 0.3, 0.0)[(i // 2) % 3],
                            (0.0, 0.25)[i % 2], i, 0.004 if i % 2 else 0.0))
    x1, x2, s, mk = _problem(vislam, orc, "general", 300, 1.0, 0.25, 1, 0.004)
    y1, y2, u, mu = _problem(vislam, orc, "sideways", 60, 1.0, 0.0, 2, 0.0)
    inf1, nan2 = x1.copy(), x2.copy()
    inf1[100] = (np.inf, 100.0)                                    # a point whose den is not finite, in the set
    nan2[7] = np.nan
    inf60 = y1.copy()
    inf60[3] = (np.inf, -np.inf)
    out += [(x1, x2, s, (np.arange(300) < 7).astype(np.uint8)),                                   # 26 FEW
            (x1, x2, np.concatenate([np.zeros(9), s[9:]]), mk),                                   # 27 NO_POSE: R all zero
            (x1, x2, np.where(np.arange(12) == 4, np.nan, s), mk),                                # 28 NO_POSE: not finite
            (y1, y2, np.concatenate([u[:9], np.zeros(3)]), mu),                                   # 29 NO_POSE: t = 0
            (inf1, x2, s, np.where(np.arange(300) == 100, 1, mk).astype(np.uint8)),                # 30
            (x1, nan2, s, np.where(np.arange(300) == 7, 1, mk).astype(np.uint8)),                 # 31
            (inf60, y2, u, np.ones(60, np.uint8)),                                                # 32
            (y1, y2, np.concatenate([u[:9], 5.0 * u[9:]]), (mu * 7).astype(np.uint8)),            # 33 a long t, mask bytes of 7
            (y1[:8], y2[:8], u, np.arange(8, dtype=np.uint8) % 8 < 7),                            # 34 FEW at 8 points
            (np.repeat(x1[299:], 64, 0), np.repeat(x2[299:] + np.float32(0.5), 64, 0), s, np.ones(64, np.uint8)),   # 35 the first pivot fails
            (x1[:257], x2[:257], s, np.zeros(257, np.uint8))]                                     # 36 FEW: an empty set
    out[34] = (out[34][0], out[34][1], out[34][2], np.asarray(out[34][3], np.uint8))
    assert len(out) == N
    return out


class _Rows:
    """a launch: rows `idx` of the problems at (max_pts, row_cap), uploaded once"""

    def __init__(self, vislam, torch, probs, idx, max_pts, row_cap):
        self.probs, self.idx, self.n, self.max_pts, self.row_cap = probs, list(idx), len(idx), max_pts, row_cap
        n = self.n
        self.p1 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.p2 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.mask = np.full((n, row_cap), 0xFF, np.uint8)
        self.pose = np.zeros(n, vislam.POSE_RESULT_DTYPE)
        self.pose["E"], self.pose["n_inliers"], self.pose["n_pose_good"], self.pose["n_models"] = np.nan, -7, 11, 1 << 20    # never read, carried over
        for i, k in enumerate(self.idx):
            a, b, s, mk = probs[k]
            assert len(a) <= max_pts
            self.p1[i, :len(a)], self.p2[i, :len(a)], self.mask[i, :len(a)] = a, b, mk
            self.pose[i]["R"], self.pose[i]["t"], self.pose[i]["n_points"] = s[:9], s[9:], len(a)
        self.npts = np.array([len(probs[k][0]) for k in self.idx], np.int32)
        self.d = [_dev(torch, v) for v in (self.pose.view(np.uint8), self.p1, self.p2, self.npts, self.mask)]

    def run(self, vislam, torch, c, ep, with_mask=True, with_pose=True):
        """(records, output mask rows, pose records or None); everything beyond what the call may write is checked to be filler"""
        n, cap = self.n, self.row_cap
        out, mo, po = _filled(torch, (n + 1) * REC), _filled(torch, (n + 1) * cap), _filled(torch, (n + 1) * PREC)
        d_pose, d_p1, d_p2, d_n, d_mask = self.d
        c.essential_polish_batch(n, d_pose.data_ptr(), d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), self.max_pts, cap,
                                 d_mask.data_ptr() if with_mask else 0, mo.data_ptr(), out.data_ptr(), po.data_ptr() if with_pose else 0, ep)
        c.batch_sync()
        raw, rawm, rawp = out.cpu().numpy(), mo.cpu().numpy(), po.cpu().numpy()
        assert (raw[n * REC:] == FILL).all() and (rawm[n * cap:] == FILL).all() and (rawp[n * PREC if with_pose else 0:] == FILL).all()
        assert d_mask.cpu().numpy().tobytes() == self.mask.tobytes() and d_pose.cpu().numpy().tobytes() == self.pose.tobytes()      # inputs are never modified
        return (raw[:n * REC].view(vislam.EPOLISH_RESULT_DTYPE).copy(), rawm[:n * cap].reshape(n, cap).copy(),
                rawp[:n * PREC].view(vislam.POSE_RESULT_DTYPE).copy() if with_pose else None)

    def check(self, want, got, where, with_pose=True):
        recs, masks, poses = got
        for i, k in enumerate(self.idx):
            r, mrow, q = want(k)
            m = int(self.npts[i])
            assert recs[i].tobytes() == r.tobytes(), (where, i, k, recs[i], r)
            assert masks[i].tobytes() == (bytes([FILL]) * self.row_cap if mrow is None else mrow.tobytes() + bytes([FILL]) * (self.row_cap - m)), (where, i, k)
            if with_pose:
                junk = self.pose[i].copy()                         # the restated record started from zeros: give it the launch's junk
                if mrow is not None:
                    junk["E"], junk["R"], junk["t"], junk["n_inliers"] = q["E"], q["R"], q["t"], q["n_inliers"]
                assert poses[i].tobytes() == junk.tobytes(), (where, i, k, poses[i], junk)


@pytest.fixture(scope="module")
def wants(probs):
    """want(params, with_mask)(k) -> the restated (record, mask row, pose record) of problem k, computed once"""
    cache = {}

    def want(eq, with_mask=True):
        def of(k):
            key = (k, eq.rounds, eq.refine_iters, eq.min_inliers, eq.select_px, with_mask)
            if key not in cache:
                x1, x2, s, mk = probs[k]
                cache[key] = epr.polish(CAM, eq, s[:9], s[9:], x1, x2, mk if with_mask else None)
            return cache[key]
        return of
    return want


SHORT = [k for k in range(N) if k < 26 and LENGTHS[k % 13] <= 64] + [29, 32, 33, 34, 35]


def test_records_masks_and_poses_against_the_restatement(vislam, probs, wants):
    import torch
    c = vislam.Context(0, _params(vislam))
    long_rows = _Rows(vislam, torch, probs, range(N), 640, 643)                            # four waves a pair; row_cap > max_pts
    short_rows = _Rows(vislam, torch, probs, [SHORT[i % len(SHORT)] for i in range(N)], 64, 67)      # one wave a pair
    assert {int(v) for v in long_rows.npts} >= set(LENGTHS) and {int(v) for v in short_rows.npts} >= {0, 5, 6, 8, 63, 64}
    seen = {}
    for rounds in (0, 1, 3, 8):
        ep, eq = _both(vislam, rounds=rounds)
        got = long_rows.run(vislam, torch, c, ep)
        long_rows.check(wants(eq), got, ("640", rounds))
        short_rows.check(wants(eq), short_rows.run(vislam, torch, c, ep), ("64", rounds))
        seen[rounds] = got[0]
    fl = [int(r["flags"]) for r in seen[3]]
    P_, J_, F_, N_ = vislam.EP_POLISHED, vislam.EP_REJECTED, vislam.EP_FEW, vislam.EP_NO_POSE
    assert fl[26:30] == [F_, N_, N_, N_] and fl[34] == F_ and fl[36] == F_ and fl[35] & J_ and fl[33] & (P_ | J_), fl
    print("\nrounds run at rounds = 3:", [int(r["rounds_run"]) for r in seen[3]], " at rounds = 8:", [int(r["rounds_run"]) for r in seen[8]])
    assert fl.count(P_) >= 20 and max(int(r["rounds_run"]) for r in seen[8]) >= max(int(r["rounds_run"]) for r in seen[3]) >= 3
    assert all(int(r["rounds_run"]) <= 1 and int(r["n_changed"]) == 0 for r in seen[0])
    assert any(int(a["n_set_last"]) != int(a["n_set_first"]) for a in seen[1])
    # the point whose den is not finite never enters a set, whatever the mask said
    ep, eq = _both(vislam)
    _, masks, _ = long_rows.run(vislam, torch, c, ep)
    assert masks[30][100] == 0 and masks[30][:300].sum() == int(seen[3][30]["n_set_last"]) and int(seen[3][30]["rounds_run"]) >= 2
    # without a mask every point of the row is in set 0; without pose_out nothing else changes
    got = long_rows.run(vislam, torch, c, ep, with_mask=False, with_pose=False)
    long_rows.check(wants(eq, False), got, "no mask", with_pose=False)
    short_rows.check(wants(eq, False), short_rows.run(vislam, torch, c, ep, with_mask=False), "64, no mask")
    assert any(int(a["n_set_first"]) != int(b["n_set_first"]) for a, b in zip(seen[3], got[0]))
    # two runs are identical
    a, b = long_rows.run(vislam, torch, c, ep), long_rows.run(vislam, torch, c, ep)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].tobytes() == seen[3].tobytes()
    # one row a launch, both shapes; SHRANK: a selection at a millionth of a pixel keeps next to nothing of a noisy row
    ep, eq = _both(vislam, select_px=1e-6)
    for k, shape in ((12, (640, 640)), (18, (64, 64)), (18, (640, 641))):
        one = _Rows(vislam, torch, probs, [k], *shape)
        got = one.run(vislam, torch, c, ep)
        one.check(wants(eq), got, ("shrank", k, shape))
        assert int(got[0][0]["flags"]) & vislam.EP_SHRANK and int(got[0][0]["n_set_last"]) == int(got[0][0]["n_set_first"]) and int(got[0][0]["n_changed"]) > 0
        assert got[1][0][:len(probs[k][3])].tobytes() == (probs[k][3] != 0).astype(np.uint8).tobytes()
    # counts above max_pts are clamped, negative ones are empty rows
    edge = _Rows(vislam, torch, probs, [12, 12, 12], 640, 640)
    edge.npts[:] = [1000, 0, -5]
    edge.d[3] = _dev(torch, edge.npts)
    ep, eq = _both(vislam)
    recs, masks, _ = edge.run(vislam, torch, c, ep)
    assert [int(r["n_points"]) for r in recs] == [640, 0, 0] and int(recs[1]["flags"]) == F_ == int(recs[2]["flags"]) and (masks[1:] == FILL).all()
    c.close()


def test_a_short_row_is_the_same_in_both_shapes_and_the_refinement_at_rounds_0(vislam, probs):
    import torch
    c = vislam.Context(0, _params(vislam))
    a, b = _Rows(vislam, torch, probs, SHORT, 64, 64), _Rows(vislam, torch, probs, SHORT, 640, 640)
    for rounds in (0, 3):
        ep, _ = _both(vislam, rounds=rounds)
        ga, gb = a.run(vislam, torch, c, ep), b.run(vislam, torch, c, ep)
        assert ga[0].tobytes() == gb[0].tobytes() and ga[2].tobytes() == gb[2].tobytes()
        assert all(ga[1][i, :m].tobytes() == gb[1][i, :m].tobytes() for i, m in enumerate(a.npts))
    # rounds = 0 against vis_essential_refine_batch on the same buffers
    out = _filled(torch, a.n * 216)
    d_pose, d_p1, d_p2, d_n, d_mask = a.d
    c.essential_refine_batch(a.n, d_pose.data_ptr(), d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), 64, 64, d_mask.data_ptr(), out.data_ptr())
    c.batch_sync()
    ref = out.cpu().numpy().view(vislam.EREF_RESULT_DTYPE)
    ep, _ = _both(vislam, rounds=0)
    recs = a.run(vislam, torch, c, ep)[0]
    refined = 0
    for r, e in zip(recs, ref):
        if int(e["flags"]) == vislam.ER_NO_POSE:
            assert int(r["flags"]) == vislam.EP_NO_POSE
            continue
        for f in ("R", "t", "E", "cost0", "cost1", "best_step", "steps_run"):
            assert r[f].tobytes() == e[f].tobytes(), f
        assert int(r["n_set_first"]) == int(e["n_used"]) and int(r["n_points"]) == int(e["n_points"])
        refined += int(int(e["flags"]) == vislam.ER_REFINED)
    assert refined >= 5
    c.close()


def test_single_call_equals_its_row(vislam, probs, wants):
    c = vislam.Context(0, _params(vislam))
    ep, eq = _both(vislam)
    for k in (0, 1, 4, 5, 6, 9, 12, 26, 27, 29, 30, 33, 35):
        x1, x2, s, mk = probs[k]
        for with_mask in (True, False):
            rec, mo, pose = c.essential_polish(s[:9], s[9:], x1, x2, mk if with_mask else None, ep)
            r, mrow, q = wants(eq, with_mask)(k)
            assert rec.tobytes() == r.tobytes(), (k, with_mask, rec, r)
            assert mo.tobytes() == (np.zeros(len(x1), np.uint8) if mrow is None else mrow).tobytes(), (k, with_mask)     # NO_POSE: the binding's zeros, untouched
            assert pose.tobytes() == q.tobytes(), (k, with_mask, pose, q)
    c.close()


# ---------------------------------------------------------------------------------------------- the plan's frames
W, H, B, MC = 752, 480, 16, 49


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(B)])
    g = f.copy()
    g[5] = 128                                                     # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


def _stream_params(vislam, gate=False):
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    return p


@pytest.mark.parametrize("gate", [False, True])
def test_plan_pairs_and_triangulation_from_the_polished_pose(vislam, stream, gate):
    import torch
    p = _stream_params(vislam, gate)
    ep, _ = _both(vislam, min_inliers=6)
    tp = vislam.default_tri_params()
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    dev = _dev(torch, stream[gate])
    cap = MC + 3                                                   # the polish's mask rows may be longer than the plan's
    out, mo, po, mo49 = _filled(torch, (B + 1) * REC), _filled(torch, (B + 1) * cap), _filled(torch, (B + 1) * PREC), _filled(torch, (B + 1) * MC)
    tri = [dict(p=_filled(torch, B * MC * 32), f=_filled(torch, B * MC), s=_filled(torch, B * 16)) for _ in range(3)]
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_ALL)
    # the refusals that need a plan, in the header's order
    bad = vislam.default_epolish_params()
    bad.rounds = 9
    call = lambda ep_=ep, n=B, rc=cap, m=mo.data_ptr(), o=out.data_ptr(), q=po.data_ptr(): \
        vislam.lib.vis_batch_essential_polish(c._h, C.byref(ep_), n, rc, C.c_void_p(m), C.c_void_p(o), C.c_void_p(q))
    assert call(ep_=bad, n=B - 1) == -1 and call(o=out.data_ptr() + 4, rc=MC - 1) == -1 and call(n=B - 1, rc=MC - 1) == -5 and call(rc=MC - 1) == -4
    trif = lambda n=B, q=po.data_ptr(), mc=MC, m=mo49.data_ptr(), rc=MC: vislam.lib.vis_batch_triangulate_from(
        c._h, C.byref(tp), n, C.c_void_p(q), mc, C.c_void_p(m) if m else None, rc, C.c_void_p(tri[0]["p"].data_ptr()), C.c_void_p(tri[0]["f"].data_ptr()),
        C.c_void_p(tri[0]["s"].data_ptr()))
    assert trif(q=po.data_ptr() + 4, n=B - 1) == -1 and trif(n=B - 1, rc=MC - 1) == -5 and trif(rc=MC - 1) == -4 and trif(mc=MC + 1) == -4
    assert all((b.cpu().numpy() == FILL).all() for b in (out, mo, po, tri[0]["p"], tri[0]["f"], tri[0]["s"]))
    # the plan's pairs, twice: rows of 52 bytes, and rows of 49 that vis_batch_triangulate_from reads; then the three triangulations
    c.batch_essential_polish(B, cap, mo.data_ptr(), out.data_ptr(), po.data_ptr(), ep)
    c.batch_essential_polish(B, MC, mo49.data_ptr(), out.data_ptr(), po.data_ptr(), ep)
    c.batch_triangulate(B, MC, tri[0]["p"].data_ptr(), tri[0]["f"].data_ptr(), tri[0]["s"].data_ptr(), tp)
    c.batch_triangulate_from(B, po.data_ptr(), MC, mo49.data_ptr(), MC, tri[2]["p"].data_ptr(), tri[2]["f"].data_ptr(), tri[2]["s"].data_ptr(), tp)
    c.batch_sync()
    assert c.batch_status() == 0
    prev = c.batch_get_keyframes()
    poses, _, ngood = c.batch_results(B)
    kps = [c.batch_keypoints(i)[0] for i in range(B)]
    plan_mask = np.full((B, MC), 0xFF, np.uint8)
    p1, p2 = np.full((B, MC, 2), np.nan, np.float32), np.full((B, MC, 2), np.nan, np.float32)
    npts = np.zeros(B, np.int32)
    for i in range(B):
        if prev[i] < 0:
            assert int(poses[i]["n_points"]) == 0 and not poses[i]["R"].any(), i
            continue
        mt = c.batch_matches(i)[0]
        k = npts[i] = len(mt)
        assert k == int(poses[i]["n_points"]) <= MC
        p1[i, :k] = np.stack([kps[prev[i]]["x"][mt["queryIdx"]], kps[prev[i]]["y"][mt["queryIdx"]]], 1)
        p2[i, :k] = np.stack([kps[i]["x"][mt["trainIdx"]], kps[i]["y"][mt["trainIdx"]]], 1)
        plan_mask[i, :k] = c.batch_inlier_mask(i)
    # (a) the plan call equals the device-row call on the downloaded rows
    d_rows = [_dev(torch, v) for v in (poses.view(np.uint8), p1, p2, npts, plan_mask)]
    out2, mo2, po2 = _filled(torch, (B + 1) * REC), _filled(torch, (B + 1) * MC), _filled(torch, (B + 1) * PREC)
    c.essential_polish_batch(B, d_rows[0].data_ptr(), d_rows[1].data_ptr(), d_rows[2].data_ptr(), d_rows[3].data_ptr(), MC, MC, d_rows[4].data_ptr(),
                             mo2.data_ptr(), out2.data_ptr(), po2.data_ptr(), ep)
    # (b) vis_batch_triangulate_from fed the plan's own records and mask
    c.batch_triangulate_from(B, d_rows[0].data_ptr(), MC, d_rows[4].data_ptr(), MC, tri[1]["p"].data_ptr(), tri[1]["f"].data_ptr(), tri[1]["s"].data_ptr(), tp)
    c.batch_sync()
    h_out, h_mo, h_po, h_mo49 = (b.cpu().numpy() for b in (out, mo, po, mo49))
    assert h_out.tobytes() == out2.cpu().numpy().tobytes() and h_po.tobytes() == po2.cpu().numpy().tobytes() and h_mo49.tobytes() == mo2.cpu().numpy().tobytes()
    assert (h_out[B * REC:] == FILL).all() and (h_mo[B * cap:] == FILL).all() and (h_po[B * PREC:] == FILL).all()
    assert h_mo[:B * cap].reshape(B, cap)[:, :MC].tobytes() == h_mo49[:B * MC].tobytes() and (h_mo[:B * cap].reshape(B, cap)[:, MC:] == FILL).all()
    recs, pol = h_out[:B * REC].view(vislam.EPOLISH_RESULT_DTYPE), h_po[:B * PREC].view(vislam.POSE_RESULT_DTYPE)
    masks = h_mo49[:B * MC].reshape(B, MC)
    for key in ("p", "f", "s"):
        assert tri[0][key].cpu().numpy().tobytes() == tri[1][key].cpu().numpy().tobytes(), key
    # (c) fed the polished ones it is vis_triangulate of each pair
    hp = tri[2]["p"].cpu().numpy().view(vislam.MAP_POINT_DTYPE).reshape(B, MC)
    hf, hs = tri[2]["f"].cpu().numpy().reshape(B, MC), tri[2]["s"].cpu().numpy().view(vislam.TRI_SUMMARY_DTYPE)
    seen = dict(pairs=0, polished=0, no_pose=0, moved_sets=0)
    for i in range(B):
        k = int(npts[i])
        if int(recs[i]["flags"]) == vislam.EP_NO_POSE:
            seen["no_pose"] += 1
            assert pol[i].tobytes() == poses[i].tobytes() and (masks[i] == FILL).all() and not hs[i].tobytes().strip(b"\0"), i
            continue
        assert int(pol[i]["n_inliers"]) == int(recs[i]["n_set_last"]) == int(masks[i, :k].sum()) and pol[i]["R"].tobytes() == recs[i]["R"].tobytes(), i
        pts, fl, sm = c.triangulate(pol[i]["R"], pol[i]["t"], p1[i, :k], p2[i, :k], masks[i, :k], tp)
        assert hp[i, :k].tobytes() == pts.tobytes() and hf[i, :k].tobytes() == fl.tobytes(), i
        assert [int(hs[i][f]) for f in ("n_points", "n_front", "n_kept")] == [sm.n_points, sm.n_front, sm.n_kept], i
        seen["pairs"] += 1
        seen["polished"] += int(bool(int(recs[i]["flags"]) & vislam.EP_POLISHED))
        seen["moved_sets"] += int(masks[i, :k].tobytes() != (plan_mask[i, :k] != 0).astype(np.uint8).tobytes())
    print(f"\ngate {gate}: {seen}")
    assert seen["pairs"] >= (13 if gate else 15) and seen["polished"] >= 8 and seen["no_pose"] >= 1 and seen["moved_sets"] >= 1, seen
    # a run without the pose stage has nothing to polish or to triangulate
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert call() == -5 and trif() == -5
    c.batch_sync()
    c.close()


def _pipelined(vislam, torch, dev, p, sync_each, order, steps=3, n=5):
    """three steps of five frames with the follow-ups queued in `order` (letters: P polish, H homography, F triangulation from the polished pose)"""
    ep, hp = vislam.default_epolish_params(), vislam.default_homography_params()
    ep.min_inliers = 6
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    c.batch_reset()
    d_draws = _dev(torch, hr.make_draws(7))
    outs = [dict(P=_filled(torch, n * REC), Pm=_filled(torch, n * MC), Pq=_filled(torch, n * PREC), H=_filled(torch, n * 112), Hm=_filled(torch, n * MC),
                 Fp=_filled(torch, n * MC * 32), Ff=_filled(torch, n * MC), Fs=_filled(torch, n * 16)) for _ in range(steps)]
    poses = [np.zeros(n, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        o = outs[k]
        c.batch_run(dev.data_ptr() + k * n * W * H, n, vislam.STAGE_ALL)
        for what in order:
            if sync_each:
                c.batch_sync()
            if what == "P":
                c.batch_essential_polish(n, MC, o["Pm"].data_ptr(), o["P"].data_ptr(), o["Pq"].data_ptr(), ep)
            elif what == "H":
                c.batch_homography(n, d_draws.data_ptr(), MC, o["Hm"].data_ptr(), o["H"].data_ptr(), hp)
            else:
                c.batch_triangulate_from(n, o["Pq"].data_ptr(), MC, o["Pm"].data_ptr(), MC, o["Fp"].data_ptr(), o["Ff"].data_ptr(), o["Fs"].data_ptr())
        c.batch_results_async(n, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    res = {key: b"".join(o[key].cpu().numpy().tobytes() for o in outs) for key in outs[0]}
    res["pose"] = b"".join(q.tobytes() for q in poses)
    c.close()
    return res


def test_pipelined_equals_synchronised_before_and_behind_the_homography(vislam, stream):
    import torch
    p = _stream_params(vislam)
    dev = _dev(torch, stream[False][:15])
    base = _pipelined(vislam, torch, dev, p, False, "H")           # without the polish
    first = _pipelined(vislam, torch, dev, p, False, "PFH")
    last = _pipelined(vislam, torch, dev, p, False, "HPF")
    split = _pipelined(vislam, torch, dev, p, False, "PHF")
    synced = _pipelined(vislam, torch, dev, p, True, "PFH")
    for key in ("H", "Hm", "pose"):
        assert base[key] == first[key] == last[key] == split[key] == synced[key], key
    for key in ("P", "Pm", "Pq", "Fp", "Ff", "Fs"):
        assert first[key] == last[key] == split[key] == synced[key] and base[key] == bytes([FILL]) * len(base[key]), key
    recs = np.frombuffer(first["P"], vislam.EPOLISH_RESULT_DTYPE)
    assert ((recs["flags"] & vislam.EP_POLISHED) != 0).sum() >= 8 and (recs["flags"] == vislam.EP_NO_POSE).sum() >= 1      # not a comparison of empty records
    sums = np.frombuffer(first["Fs"], vislam.TRI_SUMMARY_DTYPE)
    assert (sums["n_points"] > 0).sum() >= 8


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_polished_poses(vislam, stream, tmp_path):
    """tools/run_directory.py --polished: one line per frame, holding what vis_batch_essential_polish gives for the same frames in the same batches"""
    import json
    import os
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    frames = stream[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "polished.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--polished", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    dev = _dev(torch, frames)
    recs = []
    for first in range(0, n, nb):
        out, mo = _filled(torch, nb * REC), _filled(torch, nb * MC)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_essential_polish(nb, MC, mo.data_ptr(), out.data_ptr())
        c.batch_sync()
        recs += list(out.cpu().numpy().view(vislam.EPOLISH_RESULT_DTYPE))
    c.close()
    assert len(rows) == n == len(recs)
    assert j["polished"]["polished"] == sum(bool(int(r["flags"]) & vislam.EP_POLISHED) for r in recs) >= 6
    for k, (row, r) in enumerate(zip(rows, recs)):
        assert len(row) == 34 and int(row[0]) == k and int(row[1]) == 1403636579763555584 + 50000000 * k
        assert [int(v) for v in row[2:10]] == [int(r[f]) for f in ("flags", "n_points", "n_set_first", "n_set_last", "n_changed", "rounds_run", "steps_run", "best_step")]
        want = [r["cost_first"], r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(r["E"])
        assert np.array([float(v) for v in row[10:]]).tobytes() == np.array(want, np.float64).tobytes(), k
