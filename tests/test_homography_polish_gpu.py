"""GPU: the homography polish (vis_homography_polish_batch / vis_homography_polish / vis_batch_homography_polish) against the restatement
tests/homography_polish_ref.py.

Records, output masks and h_out are compared BYTE FOR BYTE, every integer and every double.  Output buffers are pre-filled with 0xEE; points
beyond a row's count are NaN and input mask bytes beyond it 0xFF, so an over-read shows as a different record and an over-write as a changed
filler.  One list of problems serves every test: 42 scenes -- the row lengths 0 ... 1030, the classes of homography_ref.H_LIST and general
motion, noise 0 / 0.3 / 1 px, 0 / 25 % of outliers -- whose record and mask are the restated RANSAC's, then the special rows.  They run at max_pts
1100 (four waves a pair) and, those of at most 64 points, again at max_pts 64 (one wave a pair); a restated row is computed once per (row,
parameters, mask) and shared.

The plan path runs on 5 frames of the parallax stream (vis_synth_frame_parallax, 752 x 480, fy = fx), gate off and on."""
import ctypes as C

import numpy as np
import pytest

import homography_polish_ref as hq
import homography_pose_ref as hpr
import homography_ref as hr
import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
FILL = 0xEE
REC, HREC, PREC = 128, 112, 320
CAM = hr.Camera()
LENGTHS = (0, 3, 4, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300, 1030)
CLASSES = hr.H_LIST + ("general",)
NSCENES = 42
DRAWS = hr.make_draws(7)


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
    a, b = vislam.default_hpolish_params(), hq.default_params()
    for k, v in kw.items():
        setattr(a, k, v)
        setattr(b, k, v)
    return a, b


def _with(rec, **kw):
    r = rec.copy()
    for k, v in kw.items():
        r[k] = v
    return r


def make_problems():
    """(x1, x2, homography record, mask) of every problem: the scenes (0 ... 41), then the special rows"""
    hp = hr.default_params()
    out = []
    for i in range(NSCENES):
        cls, m = CLASSES[(i + i // 14) % 7], LENGTHS[i % 14]
        x1, x2, _ = hr.make_rows(cls, m, (0.0, 0.3, 1.0)[(i // 2) % 3], (0.0, 0.25)[i % 2], seed=i)
        rec, mask = hr.homography(CAM, hp, x1, x2, DRAWS)
        out.append((x1, x2, rec, mask))
    x1, x2, _ = hr.make_rows("plane", 300, 1.0, 0.25)
    rec, mask = hr.homography(CAM, hp, x1, x2, DRAWS)
    y1, y2, _ = hr.make_rows("tilted", 60, 0.3, 0.0)
    rec60, mask60 = hr.homography(CAM, hp, y1, y2, DRAWS)
    assert int(rec["best_iter"]) >= 0 and int(rec60["best_iter"]) >= 0
    inf1, nan2 = x1.copy(), x2.copy()
    inf1[100] = (np.inf, 100.0)                                    # points that spoil iw / ru, put into the set by the mask
    nan2[7] = np.nan
    H0 = np.zeros(9)
    # a second image turned 90 degrees about the optical axis and zoomed by two: H ~ (0, -2, 0; 2, 0, 0; 0, 0, 1), the gauge on a tie at the start
    a, b, _, _ = hr.normalise(CAM, y1, y1)
    rng = np.random.default_rng(3)
    z2 = np.ascontiguousarray(np.stack([(2.0 * -b) * CAM.fx + CAM.cx, (2.0 * a) * CAM.fx + CAM.cy], 1) + rng.normal(0, 0.3, (60, 2)), np.float32)
    out += [(x1, x2, rec, (np.arange(300) < 7).astype(np.uint8)),                                 # 42 FEW
            (x1, x2, _with(rec, best_iter=-1), mask),                                             # 43 NO_MODEL: no winner, H as it is
            (x1, x2, _with(rec, H=np.where(np.arange(9) == 4, np.nan, rec["H"])), mask),          # 44 NO_MODEL: not finite
            (y1, y2, _with(rec60, H=H0), mask60),                                                 # 45 NO_MODEL: H = 0
            (inf1, x2, rec, np.where(np.arange(300) == 100, 1, mask).astype(np.uint8)),            # 46
            (x1, nan2, rec, np.where(np.arange(300) == 7, 1, mask).astype(np.uint8)),             # 47
            (y1, y2, _with(rec60, H=-5.0 * rec60["H"]), (mask60 * 7).astype(np.uint8)),           # 48 a long H of negative determinant, mask bytes of 7
            (y1[:8], y2[:8], rec60, (np.arange(8) < 7).astype(np.uint8)),                         # 49 FEW at 8 points
            (np.repeat(x1[299:], 64, 0), np.repeat(x2[299:], 64, 0), rec, np.ones(64, np.uint8)),  # 50 one point 64 times: a pivot fails
            (x1[:257], x2[:257], rec, np.zeros(257, np.uint8)),                                   # 51 FEW: an empty set
            (y1, z2, _with(rec60, H=np.array([0.0, -2.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0])), np.ones(60, np.uint8))]   # 52 the gauge holds H1, not H8
    assert len(out) == NSCENES + 11
    return out


@pytest.fixture(scope="module")
def probs():
    return make_problems()


SHORT = [k for k in range(NSCENES) if LENGTHS[k % 14] <= 64] + [45, 48, 49, 50, 52]


class _Rows:
    """a launch: rows `idx` of the problems at (max_pts, row_cap), uploaded once"""

    def __init__(self, vislam, torch, probs, idx, max_pts, row_cap):
        self.probs, self.idx, self.n, self.max_pts, self.row_cap = probs, list(idx), len(idx), max_pts, row_cap
        n = self.n
        self.p1 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.p2 = np.full((n, max_pts, 2), np.nan, np.float32)
        self.mask = np.full((n, row_cap), 0xFF, np.uint8)
        self.h = np.zeros(n, vislam.HOMOGRAPHY_RESULT_DTYPE)
        for i, k in enumerate(self.idx):
            a, b, rec, mk = probs[k]
            assert len(a) <= max_pts
            self.p1[i, :len(a)], self.p2[i, :len(a)], self.mask[i, :len(a)] = a, b, mk
            self.h[i] = np.frombuffer(rec.tobytes(), vislam.HOMOGRAPHY_RESULT_DTYPE)[0]
        self.npts = np.array([len(probs[k][0]) for k in self.idx], np.int32)
        self.d = [_dev(torch, v) for v in (self.h.view(np.uint8), self.p1, self.p2, self.npts, self.mask)]

    def run(self, vislam, torch, c, hp, with_mask=True, with_h=True):
        """(records, output mask rows, homography records or None); everything beyond what the call may write is checked to be filler"""
        n, cap = self.n, self.row_cap
        out, mo, ho = _filled(torch, (n + 1) * REC), _filled(torch, (n + 1) * cap), _filled(torch, (n + 1) * HREC)
        d_h, d_p1, d_p2, d_n, d_mask = self.d
        c.homography_polish_batch(n, d_h.data_ptr(), d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), self.max_pts, cap,
                                  d_mask.data_ptr() if with_mask else 0, mo.data_ptr(), out.data_ptr(), ho.data_ptr() if with_h else 0, hp)
        c.batch_sync()
        raw, rawm, rawh = out.cpu().numpy(), mo.cpu().numpy(), ho.cpu().numpy()
        assert (raw[n * REC:] == FILL).all() and (rawm[n * cap:] == FILL).all() and (rawh[n * HREC if with_h else 0:] == FILL).all()
        assert d_mask.cpu().numpy().tobytes() == self.mask.tobytes() and d_h.cpu().numpy().tobytes() == self.h.tobytes()      # inputs are never modified
        return (raw[:n * REC].view(vislam.HPOLISH_RESULT_DTYPE).copy(), rawm[:n * cap].reshape(n, cap).copy(),
                rawh[:n * HREC].view(vislam.HOMOGRAPHY_RESULT_DTYPE).copy() if with_h else None)

    def check(self, want, got, where, with_h=True):
        recs, masks, hs = got
        for i, k in enumerate(self.idx):
            r, mrow, q = want(k)
            m = int(self.npts[i])
            assert recs[i].tobytes() == r.tobytes(), (where, i, k, recs[i], r)
            assert masks[i].tobytes() == (bytes([FILL]) * self.row_cap if mrow is None else mrow.tobytes() + bytes([FILL]) * (self.row_cap - m)), (where, i, k)
            if with_h:
                assert hs[i].tobytes() == q.tobytes(), (where, i, k, hs[i], q)


@pytest.fixture(scope="module")
def wants(probs):
    """want(params, with_mask)(k) -> the restated (record, mask row, homography record) of problem k, computed once"""
    cache = {}

    def want(hp, with_mask=True):
        def of(k):
            key = (k, hp.rounds, hp.refine_iters, hp.min_inliers, hp.select_chi2, hp.sigma_px, with_mask)
            if key not in cache:
                x1, x2, rec, mk = probs[k]
                cache[key] = hq.polish(CAM, hp, rec, x1, x2, mk if with_mask else None)
            return cache[key]
        return of
    return want


def test_records_masks_and_h_out_against_the_restatement(vislam, probs, wants):
    import torch
    N = len(probs)
    c = vislam.Context(0, _params(vislam))
    long_rows = _Rows(vislam, torch, probs, range(N), 1100, 1103)                          # four waves a pair; row_cap > max_pts
    short_rows = _Rows(vislam, torch, probs, SHORT, 64, 67)                                # one wave a pair
    assert {int(v) for v in long_rows.npts} >= set(LENGTHS) and {int(v) for v in short_rows.npts} >= {0, 3, 4, 7, 8, 9, 63, 64}
    seen = {}
    for rounds in (0, 3, 8):
        hp, hqp = _both(vislam, rounds=rounds)
        got = long_rows.run(vislam, torch, c, hp)
        long_rows.check(wants(hqp), got, ("1100", rounds))
        short_rows.check(wants(hqp), short_rows.run(vislam, torch, c, hp), ("64", rounds))
        seen[rounds] = got[0]
    fl = [int(r["flags"]) for r in seen[3]]
    P_, J_, F_, N_ = vislam.HPOL_POLISHED, vislam.HPOL_REJECTED, vislam.HPOL_FEW, vislam.HPOL_NO_MODEL
    assert fl[42:46] == [F_, N_, N_, N_] and fl[49] == F_ and fl[51] == F_ and fl[50] & (P_ | J_) and fl[48] & (P_ | J_) and fl[52] == P_, fl
    assert hq.gauge([hq.F(v) for v in seen[3][52]["H"]]) in (1, 3) and hr.unit_diff(seen[3][52]["H"], probs[52][2]["H"]) < 1e-2
    assert all(f == N_ for k, f in enumerate(fl[:NSCENES]) if LENGTHS[k % 14] < 4), fl         # rows below the four-point minimum have no winner
    print("\nflags at rounds = 3:", fl, "\nrounds run at rounds = 3:", [int(r["rounds_run"]) for r in seen[3]], " at rounds = 8:", [int(r["rounds_run"]) for r in seen[8]])
    assert sum(bool(f & P_) for f in fl) >= 25 and max(int(r["rounds_run"]) for r in seen[8]) >= max(int(r["rounds_run"]) for r in seen[3]) >= 3
    assert all(int(r["rounds_run"]) <= 1 and int(r["n_changed"]) == 0 for r in seen[0])
    assert any(int(a["n_set_last"]) != int(a["n_set_first"]) for a in seen[3])
    assert all(float(np.linalg.det(r["H"].reshape(3, 3))) >= 0.0 and abs(float(np.linalg.norm(r["H"])) - 1.0) < 1e-15 for r in seen[3] if int(r["flags"]) != N_)
    # the points that spoil iw or ru never stay in a set, whatever the mask said
    hp, hqp = _both(vislam)
    _, masks, _ = long_rows.run(vislam, torch, c, hp)
    assert masks[46][100] == 0 and masks[47][7] == 0 and masks[46][:300].sum() == int(seen[3][46]["n_set_last"]) and int(seen[3][46]["rounds_run"]) >= 2
    # without a mask every point of the row is in set 0; without h_out nothing else changes
    got = long_rows.run(vislam, torch, c, hp, with_mask=False, with_h=False)
    long_rows.check(wants(hqp, False), got, "no mask", with_h=False)
    short_rows.check(wants(hqp, False), short_rows.run(vislam, torch, c, hp, with_mask=False), "64, no mask")
    assert any(int(a["n_set_first"]) != int(b["n_set_first"]) for a, b in zip(seen[3], got[0]))
    # two runs are identical
    a, b = long_rows.run(vislam, torch, c, hp), long_rows.run(vislam, torch, c, hp)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].tobytes() == seen[3].tobytes()
    # one row a launch, both shapes; SHRANK: a selection at a millionth of the threshold keeps next to nothing of a noisy row
    hp, hqp = _both(vislam, select_chi2=5.991e-12)
    for k, shape in ((41, (1100, 1100)), (34, (64, 64)), (34, (1100, 1101))):          # "rot" at 1 px of noise, 1030 and 63 points
        one = _Rows(vislam, torch, probs, [k], *shape)
        got = one.run(vislam, torch, c, hp)
        one.check(wants(hqp), got, ("shrank", k, shape))
        assert int(got[0][0]["flags"]) & vislam.HPOL_SHRANK and int(got[0][0]["n_set_last"]) == int(got[0][0]["n_set_first"]) and int(got[0][0]["n_changed"]) > 0
        assert got[1][0][:len(probs[k][3])].tobytes() == (probs[k][3] != 0).astype(np.uint8).tobytes()
    # counts above max_pts are clamped, negative ones are empty rows
    edge = _Rows(vislam, torch, probs, [26, 26, 26], 300, 300)
    edge.npts[:] = [1000, 0, -5]
    edge.d[3] = _dev(torch, edge.npts)
    hp, hqp = _both(vislam)
    recs, masks, _ = edge.run(vislam, torch, c, hp)
    assert [int(r["n_points"]) for r in recs] == [300, 0, 0] and int(recs[1]["flags"]) == F_ == int(recs[2]["flags"]) and (masks[1:] == FILL).all()
    assert recs[0].tobytes() == seen[3][26].tobytes()
    c.close()


def test_a_short_row_is_the_same_in_both_shapes(vislam, probs):
    import torch
    c = vislam.Context(0, _params(vislam))
    a, b = _Rows(vislam, torch, probs, SHORT, 64, 64), _Rows(vislam, torch, probs, SHORT, 1100, 1100)
    for rounds in (0, 3):
        hp, _ = _both(vislam, rounds=rounds)
        ga, gb = a.run(vislam, torch, c, hp), b.run(vislam, torch, c, hp)
        assert ga[0].tobytes() == gb[0].tobytes() and ga[2].tobytes() == gb[2].tobytes()
        assert all(ga[1][i, :m].tobytes() == gb[1][i, :m].tobytes() for i, m in enumerate(a.npts))
        assert sum(bool(int(r["flags"]) & vislam.HPOL_POLISHED) for r in ga[0]) >= 8
    c.close()


def test_single_call_equals_its_row(vislam, probs, wants):
    c = vislam.Context(0, _params(vislam))
    hp, hqp = _both(vislam)
    for k in (0, 1, 4, 8, 9, 12, 13, 26, 42, 43, 45, 46, 48, 50, 52):
        x1, x2, rec, mk = probs[k]
        for with_mask in (True, False):
            out, mo, ho = c.homography_polish(rec, x1, x2, mk if with_mask else None, hp)
            r, mrow, q = wants(hqp, with_mask)(k)
            assert out.tobytes() == r.tobytes(), (k, with_mask, out, r)
            assert mo.tobytes() == (np.zeros(len(x1), np.uint8) if mrow is None else mrow).tobytes(), (k, with_mask)     # NO_MODEL: the binding's zeros, untouched
            assert ho.tobytes() == q.tobytes(), (k, with_mask, ho, q)
    c.close()


# ---------------------------------------------------------------------------------------------- the plan's frames
W, H, B, MC = 752, 480, 5, 49


@pytest.fixture(scope="module")
def stream(vislam, canvas):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(15)])
    g = f.copy()
    g[2] = 128                                                     # flat: no keypoints, the gate does not save it
    return {False: f, True: g}


def _stream_params(vislam, gate=False):
    p = vislam.default_params()
    p.fy = p.fx
    if gate:
        p.keyframe_min_points = 10
    return p


@pytest.mark.parametrize("gate", [False, True])
def test_plan_chain_equals_the_restatement_chain(vislam, stream, gate):
    import torch
    p = _stream_params(vislam, gate)
    cam = hr.Camera(p.fx, p.cx, p.cy)
    hp0, hqp0 = vislam.default_homography_params(), vislam.default_hpose_params()
    hp, hqp = _both(vislam)
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    dev, d_draws = _dev(torch, stream[gate][:B]), _dev(torch, DRAWS)
    cap = MC + 3                                                   # the polish's mask rows may be longer than the plan's
    hrec, hmask = _filled(torch, (B + 1) * HREC), _filled(torch, (B + 1) * MC)
    out, mo, ho = _filled(torch, (B + 1) * REC), _filled(torch, (B + 1) * cap), _filled(torch, (B + 1) * HREC)
    plain, pol = _filled(torch, (B + 1) * PREC), _filled(torch, (B + 1) * PREC)
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_ALL)
    c.batch_homography(B, d_draws.data_ptr(), MC, hmask.data_ptr(), hrec.data_ptr(), hp0)
    # the refusals that need a plan, in the header's order
    bad = vislam.default_hpolish_params()
    bad.rounds = 9
    call = lambda hp_=hp, n=B, h=hrec.data_ptr(), mc=MC, mk=hmask.data_ptr(), rc=cap, m=mo.data_ptr(), o=out.data_ptr(), q=ho.data_ptr(): \
        vislam.lib.vis_batch_homography_polish(c._h, C.byref(hp_), n, C.c_void_p(h), mc, C.c_void_p(mk) if mk else None, rc, C.c_void_p(m), C.c_void_p(o),
                                               C.c_void_p(q) if q else None)
    assert call(hp_=bad, n=B - 1) == -1 and call(o=out.data_ptr() + 4, rc=MC - 1) == -1 and call(m=hmask.data_ptr()) == -1 and call(q=hrec.data_ptr()) == -1
    assert call(n=B - 1, rc=MC - 1) == -5 and call(rc=MC - 1) == -4 and call(mc=MC - 1) == -4
    c.batch_sync()
    assert all((b.cpu().numpy() == FILL).all() for b in (out, mo, ho))                             # a refused call writes nothing
    # homography -> polish -> homography_pose on the polished record and mask, and the plain pose of the same run, nothing in between
    c.batch_homography_polish(B, hrec.data_ptr(), MC, hmask.data_ptr(), cap, mo.data_ptr(), out.data_ptr(), ho.data_ptr(), hp)
    c.batch_homography_pose(B, ho.data_ptr(), cap, mo.data_ptr(), 0, pol.data_ptr(), hqp0)
    c.batch_homography_pose(B, hrec.data_ptr(), MC, hmask.data_ptr(), 0, plain.data_ptr(), hqp0)
    c.batch_sync()
    assert c.batch_status() == 0
    prev = c.batch_get_keyframes()
    kps = [c.batch_keypoints(i)[0] for i in range(B)]
    raw = [b.cpu().numpy() for b in (hrec, hmask, out, mo, ho, plain, pol)]
    assert all((r[B * s:] == FILL).all() for r, s in zip(raw, (HREC, MC, REC, cap, HREC, PREC, PREC)))
    h_in, m_in = raw[0][:B * HREC].view(vislam.HOMOGRAPHY_RESULT_DTYPE), raw[1][:B * MC].reshape(B, MC)
    recs, masks, h_out = raw[2][:B * REC].view(vislam.HPOLISH_RESULT_DTYPE), raw[3][:B * cap].reshape(B, cap), raw[4][:B * HREC].view(vislam.HOMOGRAPHY_RESULT_DTYPE)
    plain_r, pol_r = raw[5][:B * PREC].view(vislam.HPOSE_RESULT_DTYPE), raw[6][:B * PREC].view(vislam.HPOSE_RESULT_DTYPE)
    seen = dict(pairs=0, polished=0, no_model=0, moved=0)
    for i in range(B):
        if prev[i] < 0:
            assert int(recs[i]["flags"]) == vislam.HPOL_NO_MODEL and recs[i].tobytes() == hq.zero_record().tobytes(), i
            assert h_out[i].tobytes() == h_in[i].tobytes() and (masks[i] == FILL).all() and pol_r[i].tobytes() == hpr.zero_record().tobytes(), i
            seen["no_model"] += 1
            continue
        mt = c.batch_matches(i)[0]
        k = len(mt)
        x1 = np.stack([kps[prev[i]]["x"][mt["queryIdx"]], kps[prev[i]]["y"][mt["queryIdx"]]], 1)
        x2 = np.stack([kps[i]["x"][mt["trainIdx"]], kps[i]["y"][mt["trainIdx"]]], 1)
        assert int(h_in[i]["n_points"]) == k <= MC
        r, mrow, q = hq.polish(cam, hqp, h_in[i], x1, x2, m_in[i, :k])
        assert recs[i].tobytes() == r.tobytes(), (i, recs[i], r)
        assert h_out[i].tobytes() == q.tobytes(), (i, h_out[i], q)
        assert masks[i].tobytes() == (bytes([FILL]) * cap if mrow is None else mrow.tobytes() + bytes([FILL]) * (cap - k)), i
        want_pol = hpr.hpose(cam, hpr.default_params(), q, x1, x2, mrow, None)
        want_plain = hpr.hpose(cam, hpr.default_params(), h_in[i], x1, x2, m_in[i, :k], None)
        assert pol_r[i].tobytes() == want_pol.tobytes(), (i, pol_r[i], want_pol)
        assert plain_r[i].tobytes() == want_plain.tobytes(), (i, plain_r[i], want_plain)                 # the plain call is what it was
        seen["pairs"] += 1
        seen["polished"] += int(bool(int(recs[i]["flags"]) & vislam.HPOL_POLISHED))
        seen["moved"] += int(pol_r[i]["R"].tobytes() != plain_r[i]["R"].tobytes())
    print(f"\ngate {gate}: {seen}, frames without a pair {[i for i in range(B) if prev[i] < 0]}")
    assert seen["no_model"] >= 1 and seen["pairs"] >= 3 and seen["polished"] >= 2 and seen["moved"] >= 2, seen
    # a run without the match stage has no pairs to polish
    c.batch_run(dev.data_ptr(), B, vislam.STAGE_DETECT)
    assert call() == -5
    c.batch_sync()
    c.close()


def _pipelined(vislam, torch, dev, p, sync_each, order, steps=3, n=B):
    """three steps of five frames with the follow-ups queued in `order` (letters: h homography, q its polish, o the pose of the polished record,
    E the two-view polish)"""
    hp0, hp, hqp0, ep = vislam.default_homography_params(), vislam.default_hpolish_params(), vislam.default_hpose_params(), vislam.default_epolish_params()
    ep.min_inliers = 6
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, n)
    c.batch_reset()
    d_draws = _dev(torch, DRAWS)
    outs = [dict(h=_filled(torch, n * HREC), hm=_filled(torch, n * MC), q=_filled(torch, n * REC), qm=_filled(torch, n * MC), qh=_filled(torch, n * HREC),
                 o=_filled(torch, n * PREC), E=_filled(torch, n * 224), Em=_filled(torch, n * MC)) for _ in range(steps)]
    poses = [np.zeros(n, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        o = outs[k]
        c.batch_run(dev.data_ptr() + k * n * W * H, n, vislam.STAGE_ALL)
        for what in order:
            if sync_each:
                c.batch_sync()
            if what == "h":
                c.batch_homography(n, d_draws.data_ptr(), MC, o["hm"].data_ptr(), o["h"].data_ptr(), hp0)
            elif what == "q":
                c.batch_homography_polish(n, o["h"].data_ptr(), MC, o["hm"].data_ptr(), MC, o["qm"].data_ptr(), o["q"].data_ptr(), o["qh"].data_ptr(), hp)
            elif what == "o":
                c.batch_homography_pose(n, o["qh"].data_ptr(), MC, o["qm"].data_ptr(), 0, o["o"].data_ptr(), hqp0)
            else:
                c.batch_essential_polish(n, MC, o["Em"].data_ptr(), o["E"].data_ptr(), 0, ep)
        c.batch_results_async(n, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    res = {key: b"".join(o[key].cpu().numpy().tobytes() for o in outs) for key in outs[0]}
    res["pose"] = b"".join(q.tobytes() for q in poses)
    c.close()
    return res


def test_pipelined_equals_synchronised_before_and_behind_the_two_view_polish(vislam, stream):
    import torch
    p = _stream_params(vislam)
    dev = _dev(torch, stream[False])
    first = _pipelined(vislam, torch, dev, p, False, "hqoE")
    last = _pipelined(vislam, torch, dev, p, False, "Ehqo")
    split = _pipelined(vislam, torch, dev, p, False, "hEqo")
    synced = _pipelined(vislam, torch, dev, p, True, "hqoE")
    for key in first:
        assert first[key] == last[key] == split[key] == synced[key], key
    recs = np.frombuffer(first["q"], vislam.HPOLISH_RESULT_DTYPE)
    assert ((recs["flags"] & vislam.HPOL_POLISHED) != 0).sum() >= 8 and (recs["flags"] == vislam.HPOL_NO_MODEL).sum() >= 1      # not a comparison of empty records
    assert (np.frombuffer(first["o"], vislam.HPOSE_RESULT_DTYPE)["kind"] > 0).sum() >= 8
    assert ((np.frombuffer(first["E"], vislam.EPOLISH_RESULT_DTYPE)["flags"] & vislam.EP_POLISHED) != 0).sum() >= 4


# ---------------------------------------------------------------------------------------------- the directory harness
def test_run_directory_writes_the_polished_hposes(vislam, stream, tmp_path):
    """tools/run_directory.py --hposes ... --hpolish: one line per pair, holding what the three calls give for the same frames in the same batches"""
    import json
    import os
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb_ = 10, 5
    frames = stream[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + frames[t].tobytes())
    csv = tmp_path / "hposes.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb_),
                        "--hposes", str(csv), "--hpolish"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    lines = [l.split(",") for l in csv.read_text().splitlines()]
    p = _stream_params(vislam)                                     # the tool's parameters: ORB::create(200), fy = fx
    p.nfeatures, p.w_size, p.h_size = 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb_)
    dev, d_draws = _dev(torch, frames), _dev(torch, DRAWS)
    want, flags = [], []
    for first in range(0, n, nb_):
        hrec, mask, out = _filled(torch, nb_ * HREC), _filled(torch, nb_ * MC), _filled(torch, nb_ * PREC)
        q, qm, qh = _filled(torch, nb_ * REC), _filled(torch, nb_ * MC), _filled(torch, nb_ * HREC)
        c.batch_run(dev.data_ptr() + first * W * H, nb_, vislam.STAGE_FRAME)
        c.batch_homography(nb_, d_draws.data_ptr(), MC, mask.data_ptr(), hrec.data_ptr())
        c.batch_homography_polish(nb_, hrec.data_ptr(), MC, mask.data_ptr(), MC, qm.data_ptr(), q.data_ptr(), qh.data_ptr())
        c.batch_homography_pose(nb_, qh.data_ptr(), MC, qm.data_ptr(), 0, out.data_ptr())
        c.batch_sync()
        recs, pol = out.cpu().numpy().view(vislam.HPOSE_RESULT_DTYPE), q.cpu().numpy().view(vislam.HPOLISH_RESULT_DTYPE)
        flags += [int(f) for f in pol["flags"]]
        want += [(first + i, recs[i].copy(), int(pol[i]["flags"])) for i in range(nb_) if int(recs[i]["kind"]) != vislam.HP_NONE]
    c.close()
    assert len(lines) == len(want) == n - 1                        # every frame but the first has a pair
    for row, (frame, rec, pf) in zip(lines, want):
        assert len(row) == 48 and int(row[0]) == frame and int(row[1]) == 1403636579763555584 + 50000000 * frame
        assert row[2] == vislam.HP_KIND_NAMES[int(rec["kind"])] and int(row[47]) == pf
        ints = [int(rec[k]) for k in ("flags", "solution", "second", "n_points", "n_tested", "n_parallax")] + [int(v) for v in rec["n_good"]]
        assert [int(v) for v in row[3:13]] == ints
        dbl = np.concatenate([rec["sv"], [rec["t_norm"]], rec["R"], rec["t"], rec["n"], rec["R2"], rec["t2"], rec["n2"]])
        assert np.array([float(v) for v in row[13:47]]).tobytes() == dbl.tobytes()
    assert j["hpolish"]["polished"] == sum(bool(f & vislam.HPOL_POLISHED) for f in flags) >= 5
    assert j["hpolish"]["no_model"] == sum(f == vislam.HPOL_NO_MODEL for f in flags) >= 1
