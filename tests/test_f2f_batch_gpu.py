"""GPU: F2FRansac and FilterKeypoints for the pairs of a batch (vis_f2f_batch / vis_batch_f2f, vis_filter_keypoints_batch /
vis_batch_filter_keypoints / vis_filter_keypoints; VISystem::F2FRansac, src/VISystem.cpp:612-769, VISystem::FilterKeypoints, :542-610).

Every F2F record is checked against the single call (ctx.f2f_ransac on the same pair with idx = draws % (m - 1) and the float scale: t
byte-identical, equal count), against the oracle (orc.f2f_ransac: equal count, |dt| <= 1e-6, the project's own tolerance,
tests/test_pose_gpu.py) and against tests/f2f_ref.py (best_iter, n_degenerate, flipped).  The single call and the batch now run the same
kernel template (k_f2f_batch: the single call is one pair of it with its indices taken as given, the batch reduces raw draws modulo
m - 1), so the first comparison only shows that the two index forms, the two row layouts and the host's scale agree; the independent
checks are the oracle and tests/f2f_ref.py, both asserted on every record below.  Filter masks and counts are compared byte for byte
with the restatement.  The plan's pairs are rebuilt from the batch getters.

The stream of the plan tests: vis_synth_frame_parallax, canvas 2048 / seed 0xE0C00001, 752 x 480, fy = fx, frames 0 ... 15; the oracle's
pipeline gives 26 ... 42 good matches on every pair of frames 0 ... 63 (tests/test_triangulate_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import f2f_ref as fr

pytestmark = pytest.mark.gpu
W, H = 752, 480
FILL = 0xEE


def _params(vislam, **kw):
    p = vislam.default_params()
    p.fy = p.fx
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _small_rots(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_rodrigues(rng.normal(0, 0.01, 3)) for _ in range(n)]).astype(np.float32)


def _vectors(n, seed, scale):
    v = np.random.default_rng(seed).normal(0, 1, (n, 3))
    return (scale * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _draws(seed, iters=1000):
    return np.random.default_rng(seed).integers(0, 2 ** 31, (iters, 2)).astype(np.int32)      # what rand() returns: 0 ... RAND_MAX


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _check_record(vislam, orc, single, p, rec, a, b, rot, draws, tref, where):
    """one record of a batch against the single call (the same kernel template), and -- independently -- the oracle and the restatement"""
    KP = vislam.KEYPOINT_DTYPE
    m, iters = len(a), int(p.f2f_iters)
    want = fr.f2f(p, a, b, rot, draws, tref)
    got = fr.record_tuple(rec)
    assert got[1:] == fr.record_tuple(want)[1:], (where, got, fr.record_tuple(want))
    if m < 2 or iters == 0:
        assert got == fr.record_tuple(fr.ZERO_RECORD), where
        return
    idx = fr.reduce_draws(draws, m)[:iters]
    g = None if tref is None else np.asarray(tref, np.float32)
    scale = np.float32(1.0) if g is None else np.float32(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
    ka, kb = fr.keypoints(KP, a), fr.keypoints(KP, b)
    st, sc = single.f2f_ransac(ka, kb, rot, idx, float(scale))
    sign = np.float32(-1.0 if int(rec["flipped"]) else 1.0)
    assert int(rec["count_max"]) == sc, (where, int(rec["count_max"]), sc)
    assert np.asarray(rec["t"], np.float32).tobytes() == (sign * st).astype(np.float32).tobytes(), (where, rec["t"], st)
    ot, oc = orc.f2f_ransac(p, ka, kb, rot, idx, float(scale))
    assert int(rec["count_max"]) == oc, (where, int(rec["count_max"]), oc)
    assert np.abs(np.asarray(rec["t"], np.float32) - sign * ot).max() <= 1e-6, (where, rec["t"], ot)
    if g is not None and int(rec["count_max"]) > 0:
        assert float(np.dot(np.asarray(rec["t"], np.float64), g.astype(np.float64))) >= -1e-6, where


# ---------------------------------------------------------------------------------------------- 1 - 3: device pointers, synthetic pairs
class _Synth:
    """pairs of fr.batch_cases as device rows of max_pts correspondences"""
    def __init__(self, vislam, torch, cases, pairs=None):
        self.cases = cases
        self.pairs = [fr.pair_inputs(*c) for c in cases] if pairs is None else pairs
        self.n = len(cases)
        self.max_pts = max(len(a) for a, _, _, _ in self.pairs)
        p1 = np.zeros((self.n, self.max_pts, 2), np.float32)
        p2 = np.zeros_like(p1)
        for i, (a, b, _, _) in enumerate(self.pairs):
            p1[i, :len(a)], p2[i, :len(b)] = a, b
        self.rots = np.stack([r for _, _, r, _ in self.pairs])
        self.ts = np.stack([t for _, _, _, t in self.pairs])
        self.trefs = (self.ts * np.linspace(-0.9, 1.3, self.n, dtype=np.float32)[:, None]).astype(np.float32)   # both signs, scales != 1
        self.npts = np.array([len(a) for a, _, _, _ in self.pairs], np.int32)
        self.d_p1, self.d_p2, self.d_npts = _dev(torch, p1), _dev(torch, p2), _dev(torch, self.npts)
        self.d_rot, self.d_t, self.d_tref = _dev(torch, self.rots), _dev(torch, self.ts), _dev(torch, self.trefs)


@pytest.fixture(scope="module")
def synth(vislam):
    import torch
    return _Synth(vislam, torch, fr.batch_cases(vislam.F2F_TILE))


@pytest.fixture(scope="module")
def synth_short(vislam, synth):
    """the eight pairs of up to 120 correspondences again, as rows of 120: rows of at most one tile take the kernel's other workgroup shape"""
    import torch
    keep = [i for i in range(synth.n) if synth.npts[i] <= 120]
    return _Synth(vislam, torch, [synth.cases[i] for i in keep], [synth.pairs[i] for i in keep])


@pytest.mark.parametrize("iters", [1000, 70, 0])
def test_device_rows_against_single_call_oracle_and_restatement(vislam, orc, synth, synth_short, iters):
    import torch
    T = vislam.F2F_TILE
    assert sorted(synth.npts.tolist()) == sorted([0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 5, 40, 120, 60, 90])
    assert synth.max_pts > T >= synth_short.max_pts == 120 and synth_short.n == 8
    p = _params(vislam, f2f_iters=iters)
    c, single = vislam.Context(0, p), vislam.Context(0, p)
    draws = _draws(5, max(iters, 1))
    d_draws = _dev(torch, draws)
    for synth, with_ref in ((synth, True), (synth, False), (synth_short, True)):
        n = synth.n
        out = _filled(torch, (n + 2) * 32)
        c.f2f_batch(n, synth.d_p1.data_ptr(), synth.d_p2.data_ptr(), synth.d_npts.data_ptr(), synth.max_pts, synth.d_rot.data_ptr(),
                    synth.d_tref.data_ptr() if with_ref else 0, d_draws.data_ptr(), out.data_ptr())
        c.batch_sync()
        raw = out.cpu().numpy()
        assert (raw[n * 32:] == FILL).all()                        # records beyond n keep their fill pattern
        recs = raw[:n * 32].view(vislam.F2F_RESULT_DTYPE)
        flipped = 0
        for i, (a, b, rot, _) in enumerate(synth.pairs):
            _check_record(vislam, orc, single, p, recs[i], a, b, rot, draws, synth.trefs[i] if with_ref else None, (iters, with_ref, i))
            flipped += int(recs[i]["flipped"])
        if iters and with_ref and n == 12:
            assert 0 < flipped < n                                 # the sign fix went both ways
        if not with_ref:
            assert flipped == 0
        if iters:
            assert int(recs[2]["n_degenerate"]) == iters and int(recs[2]["best_iter"]) == -1       # m = 2: both samples are point 0
            assert all(int(recs[i]["best_iter"]) >= 0 for i in range(3, n))
    c.close()
    single.close()


class _EdgeRows:
    """fr.edge_rows, each a one-pair batch of its own row length (40: the workgroup shape of short rows; F2F_TILE + 1: the other one)"""
    def __init__(self, vislam, torch):
        self.pairs = fr.edge_rows(vislam.F2F_TILE)
        assert [len(a) for a, _, _, _ in self.pairs] == [40, vislam.F2F_TILE + 1]
        self.dev = [(_dev(torch, a), _dev(torch, b), _dev(torch, np.array([len(a)], np.int32)), _dev(torch, rot), _dev(torch, t))
                    for a, b, rot, t in self.pairs]

    def run(self, vislam, torch, c, k, draws):
        d_p1, d_p2, d_n, d_rot, d_tref = self.dev[k]
        d_draws, out = _dev(torch, draws), _filled(torch, 2 * 32)
        c.f2f_batch(1, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), len(self.pairs[k][0]), d_rot.data_ptr(), d_tref.data_ptr(),
                    d_draws.data_ptr(), out.data_ptr())
        c.batch_sync()
        raw = out.cpu().numpy()
        assert (raw[32:] == FILL).all()
        return raw[:32].view(vislam.F2F_RESULT_DTYPE)[0]


def test_iteration_counts_at_slot_and_round_edges(vislam, orc):
    """iteration counts at the edges of a lane's slots, a wave, a workgroup and a round (256 x 4 and 512 x 2 lanes x slots: 1024 iterations
    per round): one lane, one wave, one more; one slot of the short shape, one more; inside the third slot; one round, one more; inside
    the second round's second slot"""
    import torch
    p = _params(vislam)
    c = vislam.Context(0, p)
    rows = _EdgeRows(vislam, torch)
    for iters in (1, 64, 65, 256, 257, 600, 1024, 1025, 1300):
        p.f2f_iters = iters
        c.set_params(p)
        draws = _draws(900 + iters, iters)
        for k, (a, b, rot, t) in enumerate(rows.pairs):
            rec = rows.run(vislam, torch, c, k, draws)
            _check_record(vislam, orc, c, p, rec, a, b, rot, draws, t, (iters, len(a)))
            assert int(rec["best_iter"]) >= 0, (iters, len(a))
    c.close()


def test_tie_goes_to_the_first_live_iteration(vislam):
    """every live iteration has the same count: the winner is the first of them, wherever it sits -- lane 0, a second wave, a later slot
    of a lane, the second round (tests/test_f2f_batch_ref.py checks the inputs against the restatement on the CPU)"""
    import torch
    p = _params(vislam)
    c = vislam.Context(0, p)
    rows = _EdgeRows(vislam, torch)
    for k, (a, b, rot, t) in enumerate(rows.pairs):
        p.f2f_iters = 1
        c.set_params(p)
        alone = rows.run(vislam, torch, c, k, fr.tie_draws(0, 1))
        assert int(alone["best_iter"]) == 0 and int(alone["count_max"]) > 0
        assert fr.record_tuple(alone) == fr.record_tuple(fr.f2f(p, a, b, rot, fr.tie_draws(0, 1), t))
        p.f2f_iters = fr.TIE_ITERS
        c.set_params(p)
        for first in fr.TIE_FIRSTS:
            draws = fr.tie_draws(first)
            rec = rows.run(vislam, torch, c, k, draws)
            where = (len(a), first)
            assert int(rec["best_iter"]) == first and int(rec["n_degenerate"]) == first, (where, rec)
            assert int(rec["count_max"]) == int(alone["count_max"]), (where, rec, alone)
            assert fr.record_tuple(rec) == fr.record_tuple(fr.f2f(p, a, b, rot, draws, t)), where
    c.close()


def test_counts_at_the_boundary_of_the_predicate(vislam, orc):
    """thresholds set exactly ON the error of a correspondence (and its two neighbours), where the band of the device helper is entered:
    count and winner must be the oracle's"""
    import torch
    p = _params(vislam)
    a, b, rot, _ = fr.pair_inputs(60, 33, 0.25, 0.4)
    draws = _draws(33)
    rec, (d, cnt, deg, nv) = fr.f2f(p, a, b, rot, draws, detail=True)
    best = rec["best_iter"]
    x = np.abs((d[best, 0] * nv[:, 0] + d[best, 1] * nv[:, 1]) + d[best, 2] * nv[:, 2])
    cc = 10.0 ** (-1000.0 / p.f2f_threshold)
    order = np.argsort(np.abs(np.log(np.where(x > 0, x, 1e-300)) - np.log(cc)))
    near = [int(k) for k in order if 0 < x[k] < 1][:3]
    assert (x[near] < cc).any() or (x[near] > cc).any()
    thresholds = []
    for k in near:
        t0 = float(-1000.0 / np.log10(x[k]))
        thresholds += [float(np.nextafter(t0, -np.inf)), t0, float(np.nextafter(t0, np.inf))]
    assert len(thresholds) == 9
    KP = vislam.KEYPOINT_DTYPE
    ka, kb = fr.keypoints(KP, a), fr.keypoints(KP, b)
    idx = fr.reduce_draws(draws, 60)
    c = vislam.Context(0, p)
    d_p1, d_p2, d_n = _dev(torch, a), _dev(torch, b), _dev(torch, np.array([60], np.int32))
    d_rot, d_draws = _dev(torch, rot), _dev(torch, draws)
    for thr in thresholds:
        p.f2f_threshold = thr
        c.set_params(p)
        out = _filled(torch, 32)
        c.f2f_batch(1, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), 60, d_rot.data_ptr(), 0, d_draws.data_ptr(), out.data_ptr())
        c.batch_sync()
        r = out.cpu().numpy().view(vislam.F2F_RESULT_DTYPE)[0]
        ot, oc = orc.f2f_ransac(p, ka, kb, rot, idx, 1.0)
        print(f"threshold {thr!r}: device count {int(r['count_max'])} iteration {int(r['best_iter'])}, oracle count {oc}")
        assert int(r["count_max"]) == oc, (thr, int(r["count_max"]), oc)
        assert np.abs(r["t"] - ot).max() <= 1e-6, (thr, r["t"], ot)
    c.close()


def test_threshold_sweep_on_eight_pairs(vislam, orc):
    import torch
    p = _params(vislam)
    pairs = [fr.pair_inputs(60, 33 + k, 0.25, 0.4) for k in range(8)]
    draws = _draws(33)
    KP = vislam.KEYPOINT_DTYPE
    d_p1 = _dev(torch, np.stack([a for a, _, _, _ in pairs]))
    d_p2 = _dev(torch, np.stack([b for _, b, _, _ in pairs]))
    d_n, d_rot, d_draws = _dev(torch, np.full(8, 60, np.int32)), _dev(torch, np.stack([r for _, _, r, _ in pairs])), _dev(torch, draws)
    idx = fr.reduce_draws(draws, 60)
    c = vislam.Context(0, p)
    seen = set()
    for thr in np.linspace(150.0, 900.0, 26):
        p.f2f_threshold = float(thr)
        c.set_params(p)
        out = _filled(torch, 8 * 32)
        c.f2f_batch(8, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), 60, d_rot.data_ptr(), 0, d_draws.data_ptr(), out.data_ptr())
        c.batch_sync()
        recs = out.cpu().numpy().view(vislam.F2F_RESULT_DTYPE)
        for k, (a, b, rot, _) in enumerate(pairs):
            ot, oc = orc.f2f_ransac(p, fr.keypoints(KP, a), fr.keypoints(KP, b), rot, idx, 1.0)
            assert int(recs[k]["count_max"]) == oc, (thr, k, int(recs[k]["count_max"]), oc)
            assert np.abs(recs[k]["t"] - ot).max() <= 1e-6
        seen.add(int(recs[0]["count_max"]))
    c.close()
    assert len(seen) >= 5                                          # the sweep really crossed count boundaries


def test_filter_rows(vislam, synth):
    import torch
    p = _params(vislam)
    c = vislam.Context(0, p)
    n, cap = synth.n, synth.max_pts + 3
    KP = vislam.KEYPOINT_DTYPE
    for thr in (500.0, 370.0):
        keep, nk = _filled(torch, n * cap), _filled(torch, (n + 1) * 4)
        c.filter_keypoints_batch(n, synth.d_p1.data_ptr(), synth.d_p2.data_ptr(), synth.d_npts.data_ptr(), synth.max_pts, synth.d_rot.data_ptr(),
                                 synth.d_t.data_ptr(), thr, cap, keep.data_ptr(), nk.data_ptr())
        c.batch_sync()
        rows, cnt = keep.cpu().numpy().reshape(n, cap), nk.cpu().numpy().view(np.int32)
        assert cnt[n] == np.frombuffer(bytes([FILL] * 4), np.int32)[0]
        both = 0
        for i, (a, b, rot, t) in enumerate(synth.pairs):
            m = len(a)
            wk, wc = fr.filter_keypoints(p, a, b, rot, t, thr)
            assert rows[i, :m].tobytes() == wk.tobytes() and int(cnt[i]) == wc, (thr, i)
            assert (rows[i, m:] == FILL).all(), (thr, i)           # bytes beyond the pair's correspondences are left untouched
            sk, sc = c.filter_keypoints(fr.keypoints(KP, a), fr.keypoints(KP, b), rot, t, thr)
            assert sk.tobytes() == wk.tobytes() and sc == wc, (thr, i)
            both += int(m >= 2 and 0 < wc < m)
        assert both >= 8, (thr, both)                              # the threshold cuts on both sides (checked on the CPU: test_f2f_batch_ref.py)
        # a zero translation keeps nothing
        keep, nk = _filled(torch, n * cap), _filled(torch, n * 4)
        zero_t = _dev(torch, np.zeros((n, 3), np.float32))
        c.filter_keypoints_batch(n, synth.d_p1.data_ptr(), synth.d_p2.data_ptr(), synth.d_npts.data_ptr(), synth.max_pts, synth.d_rot.data_ptr(),
                                 zero_t.data_ptr(), thr, cap, keep.data_ptr(), nk.data_ptr())
        c.batch_sync()
        rows, cnt = keep.cpu().numpy().reshape(n, cap), nk.cpu().numpy().view(np.int32)
        assert not cnt.any() and all(not rows[i, :synth.npts[i]].any() for i in range(n))
    a, b, rot, t = synth.pairs[8]
    assert c.filter_keypoints(fr.keypoints(KP, a), fr.keypoints(KP, b), rot, np.zeros(3, np.float32), 500.0)[1] == 0
    assert c.filter_keypoints(fr.keypoints(KP, a[:0]), fr.keypoints(KP, b[:0]), rot, t, 500.0)[1] == 0
    # row_cap one short
    keep, nk = _filled(torch, n * cap), _filled(torch, n * 4)
    rc = vislam.lib.vis_filter_keypoints_batch(c._h, n, C.c_void_p(synth.d_p1.data_ptr()), C.c_void_p(synth.d_p2.data_ptr()),
                                               C.c_void_p(synth.d_npts.data_ptr()), synth.max_pts, C.c_void_p(synth.d_rot.data_ptr()),
                                               C.c_void_p(synth.d_t.data_ptr()), 500.0, synth.max_pts - 1, C.c_void_p(keep.data_ptr()),
                                               C.c_void_p(nk.data_ptr()))
    assert rc == -4                                                # VIS_E_CAPACITY
    c.batch_sync()
    assert (keep.cpu().numpy() == FILL).all()
    c.close()


# ---------------------------------------------------------------------------------------------- 4 - 7: the plan's pairs
@pytest.fixture(scope="module")
def frames16(vislam, canvas):
    return np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(16)])


class _Inputs:
    """per-frame rotations / reference translations / filter translations of a 16-frame stream and the call's draw table, on the device"""
    def __init__(self, torch, n, identity, iters=1000):
        self.rots = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)) if identity else _small_rots(n, 77)
        self.trefs, self.ts, self.draws = _vectors(n, 78, 0.05), _vectors(n, 79, 0.3), _draws(80, iters)
        self.d_rot, self.d_tref, self.d_t, self.d_draws = _dev(torch, self.rots), _dev(torch, self.trefs), _dev(torch, self.ts), _dev(torch, self.draws)


class _Out:
    def __init__(self, torch, n, row_cap):
        self.n, self.row_cap = n, row_cap
        self.rec, self.keep, self.nk = _filled(torch, n * 32), _filled(torch, n * row_cap), _filled(torch, n * 4)

    def host(self, vislam):
        return (self.rec.cpu().numpy().view(vislam.F2F_RESULT_DTYPE), self.keep.cpu().numpy().reshape(self.n, self.row_cap),
                self.nk.cpu().numpy().view(np.int32))


def _queue(c, inp, out, first, n, thr=500.0):
    """vis_batch_f2f + vis_batch_filter_keypoints for n frames starting at stream frame `first`, into rows first ... of `out`"""
    c.batch_f2f(n, inp.d_rot.data_ptr() + 36 * first, inp.d_tref.data_ptr() + 12 * first, inp.d_draws.data_ptr(), out.rec.data_ptr() + 32 * first)
    c.batch_filter_keypoints(n, inp.d_rot.data_ptr() + 36 * first, inp.d_t.data_ptr() + 12 * first, thr, out.row_cap,
                             out.keep.data_ptr() + out.row_cap * first, out.nk.data_ptr() + 4 * first)


def _run_stream(vislam, torch, frames, cuts, p, inp, row_cap, stages):
    """the stream in launches of `cuts` frames; returns the host outputs and, per frame, the correspondences rebuilt from the getters
    (None: no pair)"""
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, max(cuts))
    c.batch_reset()
    dev = _dev(torch, frames)
    out = _Out(torch, len(frames), row_cap)
    pairs, first, carried = [], 0, None
    for n in cuts:
        c.batch_run(dev.data_ptr() + first * W * H, n, stages)
        _queue(c, inp, out, first, n)
        c.batch_sync()
        assert c.batch_status() == 0
        links = c.batch_get_keyframes()
        kps = [c.batch_keypoints(i)[0] for i in range(n)]
        for i in range(n):
            kq = kps[links[i]] if links[i] >= 0 else (carried if links[i] == vislam.KF_CARRIED else None)
            if kq is None:
                pairs.append(None)
            else:
                pairs.append(_correspondences(vislam, c, p, i, kq, kps[i]))
            if links[i] != vislam.KF_NOT_SAVED:
                carried = kps[i]
        first += n
    host = out.host(vislam)
    c.close()
    return host, pairs


def _correspondences(vislam, c, p, i, kq, kt):
    """(p1, p2) the pose stage would see for frame i of the last launch: the good matches, or the symmetric ones with VIS_POSE_SYM"""
    good, nsym = c.batch_matches(i)
    if p.pose_input == 1:
        import oracle_bind as orc
        o12, o21 = c.batch_knn(i)
        _, sym = orc.good_matches(p, kq, kt, o12, o21)      # the oracle's filter on the DEVICE's knn lists
        assert len(sym) == nsym, (i, len(sym), nsym)
        good = sym
    p1 = np.stack([kq["x"][good["queryIdx"]], kq["y"][good["queryIdx"]]], 1).astype(np.float32)
    p2 = np.stack([kt["x"][good["trainIdx"]], kt["y"][good["trainIdx"]]], 1).astype(np.float32)
    return p1, p2


def _check_stream(vislam, orc, p, host, pairs, inp, want_pair, thr=500.0):
    recs, keep, nk = host
    single = vislam.Context(0, p)
    ms = []
    for i, pr in enumerate(pairs):
        assert (pr is not None) == want_pair(i), i
        if pr is None:
            assert fr.record_tuple(recs[i]) == fr.record_tuple(fr.ZERO_RECORD) and int(recs[i]["best_iter"]) == -1, i
            assert int(nk[i]) == 0 and (keep[i] == FILL).all(), i
            continue
        a, b = pr
        m = len(a)
        ms.append(m)
        assert int(recs[i]["n_points"]) == m >= 2 and int(recs[i]["best_iter"]) >= 0 and int(recs[i]["count_max"]) > 0, (i, m, recs[i])
        _check_record(vislam, orc, single, p, recs[i], a, b, inp.rots[i], inp.draws, inp.trefs[i], i)
        wk, wc = fr.filter_keypoints(p, a, b, inp.rots[i], inp.ts[i], thr)
        assert keep[i, :m].tobytes() == wk.tobytes() and int(nk[i]) == wc, i
        assert (keep[i, m:] == FILL).all(), i
    single.close()
    return ms


@pytest.mark.parametrize("identity", [True, False])
def test_plan_pairs(vislam, orc, frames16, identity):
    import torch
    p = _params(vislam)
    inp = _Inputs(torch, 16, identity)
    host, pairs = _run_stream(vislam, torch, frames16, [16], p, inp, 49, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    ms = _check_stream(vislam, orc, p, host, pairs, inp, lambda i: i > 0)
    print(f"correspondences per pair: {min(ms)} ... {max(ms)}; kept by the filter: {host[2][1:].tolist()}")
    assert len(ms) == 15


def test_batch_cut_invariance(vislam, frames16):
    """the same 16 frames as two launches of 8: frame 8's pair is the carried one"""
    import torch
    p = _params(vislam)
    inp = _Inputs(torch, 16, False)
    stages = vislam.STAGE_DETECT | vislam.STAGE_MATCH
    (r1, k1, n1), pairs1 = _run_stream(vislam, torch, frames16, [16], p, inp, 49, stages)
    (r2, k2, n2), pairs2 = _run_stream(vislam, torch, frames16, [8, 8], p, inp, 49, stages)
    assert pairs2[8] is not None and pairs2[0] is None
    assert r1[1:].tobytes() == r2[1:].tobytes() and k1[1:].tobytes() == k2[1:].tobytes() and n1[1:].tobytes() == n2[1:].tobytes()
    assert r1[0].tobytes() == r2[0].tobytes()
    assert all(int(r["best_iter"]) >= 0 for r in r1[1:])


def test_pose_sym_rows(vislam, orc, frames16):
    """VIS_POSE_SYM: every symmetric match is a correspondence; the rows are longer than one tile of the kernel"""
    import torch
    p = _params(vislam, pose_input=1)
    inp = _Inputs(torch, 4, False)
    # the plan's correspondences per pair = its keypoint capacity: the sum over the levels of quota + quota / 8 + 32
    c = vislam.Context(0, p)
    kcap = int(sum(q + q // 8 + 32 for q in c.level_geometry(W, H)[3]))
    assert kcap > vislam.F2F_TILE
    c.batch_plan(W, H, W, 4)
    dev = _dev(torch, frames16[:4])
    c.batch_run(dev.data_ptr(), 4, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    o = _Out(torch, 4, kcap)
    call = lambda cap: vislam.lib.vis_batch_filter_keypoints(c._h, 4, C.c_void_p(inp.d_rot.data_ptr()), C.c_void_p(inp.d_t.data_ptr()), 500.0, cap,
                                                              C.c_void_p(o.keep.data_ptr()), C.c_void_p(o.nk.data_ptr()))
    assert call(kcap - 1) == -4 and call(kcap) == 0                # VIS_E_CAPACITY below the plan's row length
    c.batch_sync()
    c.close()
    host, pairs = _run_stream(vislam, torch, frames16[:4], [4], p, inp, kcap, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    ms = _check_stream(vislam, orc, p, host, pairs, inp, lambda i: i > 0)
    print(f"VIS_POSE_SYM: rows of {kcap}, correspondences per pair {ms}")
    assert len(ms) == 3 and min(ms) > 49


def test_keyframe_gate_pairing(vislam, orc, frames16):
    """keyframe_min_points = 1 with a blank frame in the middle: the refused frame gets a zero record, the frame after it is paired with
    the last saved one (vis_batch_get_keyframes)"""
    import torch
    p = _params(vislam, keyframe_min_points=1)
    frames = frames16[:8].copy()
    frames[4] = 128
    inp = _Inputs(torch, 8, False)
    host, pairs = _run_stream(vislam, torch, frames, [8], p, inp, 49, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    ms = _check_stream(vislam, orc, p, host, pairs, inp, lambda i: i not in (0, 4))
    assert len(ms) == 6
    # state and capacity refusals that need a plan
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, 8)
    o = _Out(torch, 8, 49)
    f2f = lambda n: vislam.lib.vis_batch_f2f(c._h, n, C.c_void_p(inp.d_rot.data_ptr()), None, C.c_void_p(inp.d_draws.data_ptr()), C.c_void_p(o.rec.data_ptr()))
    flt = lambda n, cap: vislam.lib.vis_batch_filter_keypoints(c._h, n, C.c_void_p(inp.d_rot.data_ptr()), C.c_void_p(inp.d_t.data_ptr()), 500.0, cap,
                                                                C.c_void_p(o.keep.data_ptr()), C.c_void_p(o.nk.data_ptr()))
    assert f2f(8) == -5 and flt(8, 49) == -5                       # VIS_E_STATE: nothing has run
    dev = _dev(torch, frames)
    c.batch_run(dev.data_ptr(), 8, vislam.STAGE_DETECT)
    assert f2f(8) == -5 and flt(8, 49) == -5                       # the last run had no VIS_STAGE_MATCH
    c.batch_run(dev.data_ptr(), 8, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    assert f2f(7) == -5 and flt(7, 49) == -5                       # n differs
    assert flt(8, 48) == -4                                        # VIS_E_CAPACITY
    assert f2f(8) == 0 and flt(8, 49) == 0
    c.batch_sync()
    assert c.batch_status() == 0
    c.close()


def _pipelined(vislam, torch, dev, p, inp, sync_each, steps=3, B=5):
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c.batch_reset()
    outs = [_Out(torch, B, 49) for _ in range(steps)]
    poses = [np.zeros(B, vislam.POSE_RESULT_DTYPE) for _ in range(steps)]
    for k in range(steps):
        c.batch_run(dev.data_ptr() + k * B * W * H, B, vislam.STAGE_ALL)
        if sync_each:
            c.batch_sync()
        c.batch_f2f(B, inp.d_rot.data_ptr() + 36 * B * k, inp.d_tref.data_ptr() + 12 * B * k, inp.d_draws.data_ptr(), outs[k].rec.data_ptr())
        if sync_each:
            c.batch_sync()
        c.batch_results_async(B, poses[k].ctypes.data)
        if sync_each:
            c.batch_sync()
    c.batch_sync()
    assert c.batch_status() == 0
    recs = [o.rec.cpu().numpy().tobytes() for o in outs]
    c.close()
    return recs, [q.tobytes() for q in poses]


def test_pipelined_steps_equal_synchronised_ones(vislam, frames16):
    import torch
    p = _params(vislam)
    inp = _Inputs(torch, 15, False)
    dev = _dev(torch, frames16[:15])
    qr, qp = _pipelined(vislam, torch, dev, p, inp, False)
    sr, sp = _pipelined(vislam, torch, dev, p, inp, True)
    assert qr == sr and qp == sp
    recs = np.frombuffer(b"".join(qr), vislam.F2F_RESULT_DTYPE)
    assert (recs["best_iter"] >= 0).sum() == 14                    # not a comparison of empty records
