"""GPU: the geometry entry points that take caller-supplied rows, on correspondences that are not usable numbers (tests/hostile_cases.py: NaN,
+-inf, +-3e38, overflowing or degenerate map points, duplicates; every fifth entry, the first three, all, the two sides of an LDS tile's end),
and on finite pixels of one image along a ladder of magnitudes through sqrt(FLT_MAX) in normalised coordinates (the "mag" kinds), which the
essential RANSAC's single-precision scorer once counted as certain inliers.

Per entry point: the hostile rows are interleaved with clean rows of the existing case lists in one launch, and the clean rows' records and
masks must be BYTE-IDENTICAL to a launch of the clean rows alone (one bad entry changes nothing for anybody else); every hostile row equals
the restatement (the CPU oracle for the essential RANSAC) under hostile_cases.same_record -- integers equal, floats byte-equal or NaN on
both sides -- with masks byte for byte; the properties tests/test_hostile_inputs_ref.py asserts on the restatements hold on the device's own
output (the exact mpmath predicate on the device's masks included); the single host-pointer call equals the batch row; a second identical
launch is byte-identical, NaNs included; and a draw table with INT_MIN, -1 and 0x7fffffff entries (masked and reduced modulo m by the
kernels) still gives the restatement's records.  Output buffers are pre-filled with 0xEE and everything a call must not write keeps it.

vis_triangulate has no device-pointer form over caller rows (vis_batch_triangulate reads the plan's own rows), so it is the single call."""
import numpy as np
import pytest

import essential_refine_ref as er
import f2f_ref as fr
import homography_pose_ref as hpr
import homography_ref as hr
import hostile_cases as hc
import pnp_ref as pr
import pose_degenerate_cases as pdc
import triangulate_ref as tr

pytestmark = pytest.mark.gpu
FILL = 0xEE
T = hc.TILE
INT_MIN = -2 ** 31


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def _interleave(hostile, clean):
    """hostile and clean rows in turn (the longer list's tail follows): [(row, is_hostile, index in its own list)]"""
    out = []
    for k in range(max(len(hostile), len(clean))):
        if k < len(hostile):
            out.append((hostile[k], True, k))
        if k < len(clean):
            out.append((clean[k], False, k))
    return out


def _hostile_draws(draws):
    """the table with INT_MIN, -1 and 0x7fffffff in place of some entries (every column, the first iteration included)"""
    d = np.array(draws, np.int32)
    flat = d.reshape(-1)
    flat[0::7], flat[3::11], flat[5::13] = INT_MIN, -1, 0x7fffffff
    return d


def _assert_same(got, want, where, skip=()):
    assert hc.same_record(got, want, skip), (where, hc.differing_fields(got, want), got, want)


# ---------------------------------------------------------------------------------------------- PnP
def _pnp_launch(vislam, torch, c, rows, max_pts, x_stride, d_draws):
    """(records, mask rows) of one vis_pnp_batch over rows [(X, xy)]: points beyond a row's count and the fourth double at x_stride 4 are NaN"""
    n, cap = len(rows), max_pts + 3
    X = np.full((n, max_pts, x_stride), np.nan)
    xy = np.full((n, max_pts, 2), np.nan, np.float32)
    for i, (a, b) in enumerate(rows):
        X[i, :len(a), :3], xy[i, :len(a)] = a, b
    npts = np.array([len(a) for a, _ in rows], np.int32)
    d_X, d_xy, d_n = _dev(torch, X), _dev(torch, xy), _dev(torch, npts)
    out, mask = _filled(torch, (n + 2) * 240), _filled(torch, n * cap + 64)
    c.pnp_batch(n, d_X.data_ptr(), x_stride, d_xy.data_ptr(), d_n.data_ptr(), max_pts, d_draws.data_ptr(), cap, mask.data_ptr(), out.data_ptr())
    c.batch_sync()
    raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
    assert (raw[n * 240:] == FILL).all() and (mraw[n * cap:] == FILL).all()
    mrows = mraw[:n * cap].reshape(n, cap)
    for i in range(n):
        assert (mrows[i, npts[i]:] == FILL).all(), i
    return raw[:n * 240].view(pr.RESULT_DTYPE).copy(), [mrows[i, :npts[i]].copy() for i in range(n)]


@pytest.mark.parametrize("x_stride", [3, 4])
def test_pnp_batch(vislam, x_stride):
    import torch
    assert vislam.PNP_TILE == T and vislam.PNP_RESULT_DTYPE == pr.RESULT_DTYPE
    rows, _ = hc.pnp_rows()
    cam, pq, draws = pr.Camera(), pr.default_params(), hc.pnp_draws()
    c = vislam.Context(0, pdc.set_mode(vislam.default_params(), "adaptive"))
    d_draws = _dev(torch, draws)
    clean40 = [pr.make_scene(*case)[:2] for case in pr.table_cases() if case[1] == 40]
    cleanT = [pr.make_scene(cls, m, 0.3, 0.25)[:2] for cls, m in (("general", T - 1), ("plane", T), ("dup", T + 1))]
    for max_pts, lays, clean in ((40, ("stride5", "first3", "all"), clean40), (T + 1, ("tile_edge",), cleanT)):
        keys = [(kind, lay) for lay in lays for kind in hc.pnp_kinds() + (hc.mag_pnp_kinds() if lay in hc.MAG_LAYOUTS else [])]
        mixed = _interleave([(rows[k]["X"], rows[k]["xy"]) for k in keys], clean)
        recs, masks = _pnp_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, x_stride, d_draws)
        alone_r, alone_m = _pnp_launch(vislam, torch, c, clean, max_pts, x_stride, d_draws)
        for i, (_, is_hostile, k) in enumerate(mixed):
            if not is_hostile:                                     # isolation: a clean row next to hostile ones is the clean row alone
                assert recs[i].tobytes() == alone_r[k].tobytes() and masks[i].tobytes() == alone_m[k].tobytes(), (max_pts, "clean", k)
                continue
            kind, lay = keys[k]
            row = rows[kind, lay]
            _assert_same(recs[i], row["rec"], ("pnp", kind, lay, x_stride))
            assert masks[i].tobytes() == row["mask"].tobytes(), ("pnp", kind, lay)
            hc.check_pnp_row(kind, lay, row, recs[i], masks[i])
            if lay == "stride5":                                   # the single host-pointer call on one row of every kind
                rec1, mask1 = c.pnp_ransac(row["X"], row["xy"], draws)
                _assert_same(np.frombuffer(rec1.tobytes(), pr.RESULT_DTYPE)[0], recs[i], ("pnp single", kind))
                assert mask1.tobytes() == masks[i].tobytes(), ("pnp single", kind)
        assert int(alone_r[0]["best_iter"]) >= 0 and sum(int(r["best_iter"]) >= 0 for r in recs) > len(mixed) // 2    # not a comparison of empty records
        recs2, masks2 = _pnp_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, x_stride, d_draws)
        assert recs2.tobytes() == recs.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(masks, masks2))    # NaNs included
        print(f"pnp, x_stride {x_stride}, rows of {max_pts}: {len(keys)} hostile and {len(clean)} clean rows, winners {sum(int(r['best_iter']) >= 0 for r in recs)}")
    # draws with INT_MIN, -1 and 0x7fffffff: masked and reduced modulo m, nothing is read out of range
    bad = _hostile_draws(draws)
    assert (bad == INT_MIN).any() and (bad == -1).any() and (bad == 0x7fffffff).any()
    sel = [("X:nan", "stride5"), ("X:x1e160", "stride5"), ("xy:pinf", "first3"), ("X:inf_all", "tile_edge")]
    some = [(rows[k]["X"], rows[k]["xy"]) for k in sel] + [clean40[0], cleanT[2]]
    recs, masks = _pnp_launch(vislam, torch, c, some, T + 1, x_stride, _dev(torch, bad))
    for i, (X, xy) in enumerate(some):
        w_rec, w_mask = pr.pnp(cam, pq, X, xy, bad)
        _assert_same(recs[i], w_rec, ("pnp draws", i))
        assert masks[i].tobytes() == w_mask.tobytes(), ("pnp draws", i)
    c.close()


# ---------------------------------------------------------------------------------------------- homography and its pose
HREC, PREC = 112, 320


def _h_launch(vislam, torch, c, rows, max_pts, d_draws):
    """(records, mask rows, the device buffers) of one vis_homography_batch without E over rows [(x1, x2)]"""
    n, cap = len(rows), max_pts + 3
    p1 = np.full((n, max_pts, 2), np.nan, np.float32)
    p2 = np.full((n, max_pts, 2), np.nan, np.float32)
    for i, (a, b) in enumerate(rows):
        p1[i, :len(a)], p2[i, :len(b)] = a, b
    npts = np.array([len(a) for a, _ in rows], np.int32)
    d_p1, d_p2, d_n = _dev(torch, p1), _dev(torch, p2), _dev(torch, npts)
    out, mask = _filled(torch, (n + 2) * HREC), _filled(torch, n * cap + 64)
    c.homography_batch(n, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), max_pts, d_draws.data_ptr(), 0, cap, mask.data_ptr(), out.data_ptr())
    c.batch_sync()
    raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
    assert (raw[n * HREC:] == FILL).all() and (mraw[n * cap:] == FILL).all()
    mrows = mraw[:n * cap].reshape(n, cap)
    for i in range(n):
        assert (mrows[i, npts[i]:] == FILL).all(), i
    return raw[:n * HREC].view(hr.RESULT_DTYPE).copy(), [mrows[i, :npts[i]].copy() for i in range(n)], (out, d_p1, d_p2, d_n, mask, cap)


def _same_h(got, want, m, where):
    """everything but the scores under same_record; the scores within (m - 1) 2^-52 relative (tests/test_homography_gpu.py: identical terms,
    two summation orders of m non-negative doubles)"""
    _assert_same(got, want, where, skip=("score_h", "score_e"))
    for k in ("score_h", "score_e"):
        assert abs(float(got[k]) - float(want[k])) <= max(m - 1, 0) * 2.0 ** -52 * abs(float(want[k])), (where, k, float(got[k]), float(want[k]))


def _h_sets(vislam):
    rows, _ = hc.h_rows()
    clean40 = [hr.make_rows(cls, 40, 0.3 if k % 2 else 0.0, 0.25)[:2] for k, cls in enumerate(pdc.CLASSES)]
    cleanT = [hr.make_rows(cls, T + 1, 0.3, 0.25)[:2] for cls in ("general", "plane", "static")]
    return rows, ((40, ("stride5", "first3", "all"), clean40), (T + 1, ("tile_edge",), cleanT))


def test_homography_batch(vislam):
    import torch
    assert vislam.H_TILE == T and vislam.HOMOGRAPHY_RESULT_DTYPE == hr.RESULT_DTYPE
    rows, sets = _h_sets(vislam)
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    cam, hq, draws = hr.Camera(p.fx, p.cx, p.cy), hr.default_params(), hc.h_draws()
    c = vislam.Context(0, p)
    d_draws = _dev(torch, draws)
    for max_pts, lays, clean in sets:
        keys = [(kind, lay) for lay in lays for kind in hc.pair_kinds() + (hc.mag_pair_kinds() if lay in hc.MAG_LAYOUTS else [])]
        mixed = _interleave([(rows[k]["p1"], rows[k]["p2"]) for k in keys], clean)
        recs, masks, _ = _h_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, d_draws)
        alone_r, alone_m, _ = _h_launch(vislam, torch, c, clean, max_pts, d_draws)
        for i, (_, is_hostile, k) in enumerate(mixed):
            if not is_hostile:
                assert recs[i].tobytes() == alone_r[k].tobytes() and masks[i].tobytes() == alone_m[k].tobytes(), (max_pts, "clean", k)
                continue
            kind, lay = keys[k]
            row = rows[kind, lay]
            _same_h(recs[i], row["rec"], len(row["p1"]), ("homography", kind, lay))
            assert masks[i].tobytes() == row["mask"].tobytes(), ("homography", kind, lay)
            hc.check_h_row(kind, lay, row, recs[i], masks[i])
            if lay == "stride5":
                rec1, mask1 = c.find_homography(row["p1"], row["p2"], draws)
                _assert_same(np.frombuffer(rec1.tobytes(), hr.RESULT_DTYPE)[0], recs[i], ("homography single", kind))
                assert mask1.tobytes() == masks[i].tobytes(), ("homography single", kind)
        assert any(int(r["best_iter"]) >= 0 for r in alone_r)
        recs2, masks2, _ = _h_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, d_draws)
        assert recs2.tobytes() == recs.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(masks, masks2))
        print(f"homography, rows of {max_pts}: {len(keys)} hostile and {len(clean)} clean rows, winners {sum(int(r['best_iter']) >= 0 for r in recs)}")
    bad = _hostile_draws(draws)
    sel = [("p1:nan", "stride5"), ("both:big", "stride5"), ("p2:pinf", "first3"), ("both:inf_all", "tile_edge")]
    some = [(rows[k]["p1"], rows[k]["p2"]) for k in sel] + [sets[0][2][2], sets[1][2][1]]
    recs, masks, _ = _h_launch(vislam, torch, c, some, T + 1, _dev(torch, bad))
    for i, (a, b) in enumerate(some):
        w_rec, w_mask = hr.homography(cam, hq, a, b, bad)
        _same_h(recs[i], w_rec, len(a), ("homography draws", i))
        assert masks[i].tobytes() == w_mask.tobytes(), ("homography draws", i)
    c.close()


def _hpose_launch(vislam, torch, c, n, bufs, max_pts):
    """records of one vis_homography_pose_batch on exactly the buffers a homography launch read and wrote (no hint)"""
    d_h, d_p1, d_p2, d_n, d_mask, cap = bufs
    out = _filled(torch, (n + 2) * PREC)
    c.homography_pose_batch(n, d_h.data_ptr(), d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), max_pts, cap, d_mask.data_ptr(), 0, out.data_ptr() + PREC)
    c.batch_sync()
    raw = out.cpu().numpy()
    assert (raw[:PREC] == FILL).all() and (raw[(n + 1) * PREC:] == FILL).all()
    return raw[PREC:(n + 1) * PREC].view(hpr.zero_record().dtype).copy()


def test_homography_pose_batch(vislam):
    """the pose of the homography on the records and masks vis_homography_batch gave for the hostile rows: the hostile correspondences are
    outside the mask, so they may not vote, and their NaNs may not reach the record"""
    import torch
    assert vislam.HPOSE_RESULT_DTYPE == hpr.zero_record().dtype
    rows, sets = _h_sets(vislam)
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    cam = hr.Camera(p.fx, p.cx, p.cy)
    c = vislam.Context(0, p)
    d_draws = _dev(torch, hc.h_draws())
    kinds = set()
    for max_pts, lays, clean in sets:
        keys = [(kind, lay) for lay in lays for kind in hc.pair_kinds() + (hc.mag_pair_kinds() if lay in hc.MAG_LAYOUTS else [])]
        mixed = _interleave([(rows[k]["p1"], rows[k]["p2"]) for k in keys], clean)
        hrecs, masks, bufs = _h_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, d_draws)
        poses = _hpose_launch(vislam, torch, c, len(mixed), bufs, max_pts)
        _, _, bufs_c = _h_launch(vislam, torch, c, clean, max_pts, d_draws)
        alone = _hpose_launch(vislam, torch, c, len(clean), bufs_c, max_pts)
        for i, ((a, b), is_hostile, k) in enumerate(mixed):
            if not is_hostile:
                assert poses[i].tobytes() == alone[k].tobytes(), (max_pts, "clean", k)
                continue
            kind, lay = keys[k]
            want = hc.check_h_row(kind, lay, rows[kind, lay], hrecs[i], masks[i])       # (the restatement's pose of that record and mask)
            _assert_same(poses[i], want, ("hpose", kind, lay))
            kinds.add(int(poses[i]["kind"]))
            if int(poses[i]["kind"]) != hpr.HP_NONE:
                assert hc.orthonormal(poses[i]["R"]) and np.isfinite(poses[i]["t"]).all(), ("hpose", kind, lay)
            if lay == "stride5":
                one = c.homography_pose(hrecs[i], a, b, masks[i])
                _assert_same(np.frombuffer(one.tobytes(), poses.dtype)[0], poses[i], ("hpose single", kind))
        assert poses.tobytes() == _hpose_launch(vislam, torch, c, len(mixed), bufs, max_pts).tobytes()
        print(f"homography pose, rows of {max_pts}: {len(keys)} hostile and {len(clean)} clean rows, kinds {sorted(int(q['kind']) for q in poses)}")
    assert kinds >= {hpr.HP_NONE, hpr.HP_PLANE}
    c.close()


# ---------------------------------------------------------------------------------------------- triangulation
def test_triangulate(vislam):
    rows, clean = hc.tri_rows()
    p = vislam.default_params()
    p.fy = p.fx
    assert (p.fx, p.cx, p.cy) == (tr.EUROC["fx"], tr.EUROC["cx"], tr.EUROC["cy"]) and vislam.MAP_POINT_DTYPE == tr.MAP_POINT_DTYPE
    c = vislam.Context(0, p)
    cp, cf, cs = c.triangulate(clean["R"], clean["t"], clean["p1"], clean["p2"])
    assert cp.tobytes() == clean["pts"].tobytes() and cf.tobytes() == clean["flags"].tobytes()
    n_rows = 0
    for (kind, lay), row in rows.items():
        where = ("triangulate", kind, lay)
        pts, fl, sm = c.triangulate(row["R"], row["t"], row["p1"], row["p2"])
        for i in range(len(pts)):
            _assert_same(pts[i], row["pts"][i], where + (i,))
        assert fl.tobytes() == row["flags"].tobytes(), where
        got = dict(n_points=sm.n_points, n_front=sm.n_front, n_kept=sm.n_kept, mean_parallax_px=np.float32(sm.mean_parallax_px))
        _assert_same(got, row["summary"], where)
        hc.check_tri_row(kind, lay, row, pts, fl, got)
        others = np.setdiff1d(np.arange(len(pts)), row["idx"])
        if kind != "t:zero":                                       # isolation inside the row: the other points are those of the clean row, byte for byte
            assert pts[others].tobytes() == cp[others].tobytes() and fl[others].tobytes() == cf[others].tobytes(), where
        n_rows += 1
        pts2, fl2, sm2 = c.triangulate(row["R"], row["t"], row["p1"], row["p2"])
        assert pts2.tobytes() == pts.tobytes() and fl2.tobytes() == fl.tobytes() and \
            np.float32(sm2.mean_parallax_px).tobytes() == np.float32(sm.mean_parallax_px).tobytes(), where
    print(f"triangulate: {n_rows} hostile rows of {hc.M}")
    c.close()


# ---------------------------------------------------------------------------------------------- F2F and the epipolar filter
def _f2f_dict(rec):
    return dict(t=np.asarray(rec["t"], np.float32).copy(), count_max=int(rec["count_max"]), n_points=int(rec["n_points"]), best_iter=int(rec["best_iter"]),
                n_degenerate=int(rec["n_degenerate"]), flipped=int(rec["flipped"]))


def _f2f_launch(vislam, torch, c, rows, max_pts, d_draws):
    """(F2F records, keep rows, keep counts) of one vis_f2f_batch and one vis_filter_keypoints_batch over rows [dict(p1, p2, rot, t)]"""
    n, cap = len(rows), max_pts + 3
    p1 = np.full((n, max_pts, 2), np.nan, np.float32)
    p2 = np.full((n, max_pts, 2), np.nan, np.float32)
    for i, r in enumerate(rows):
        p1[i, :len(r["p1"])], p2[i, :len(r["p2"])] = r["p1"], r["p2"]
    npts = np.array([len(r["p1"]) for r in rows], np.int32)
    rot, tt = np.stack([r["rot"].reshape(9) for r in rows]).astype(np.float32), np.stack([r["t"] for r in rows]).astype(np.float32)
    d = [_dev(torch, a) for a in (p1, p2, npts, rot, tt)]
    out, keep, nkeep = _filled(torch, (n + 2) * 32), _filled(torch, n * cap + 64), _filled(torch, (n + 2) * 4)
    c.f2f_batch(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), max_pts, d[3].data_ptr(), d[4].data_ptr(), d_draws.data_ptr(), out.data_ptr())
    c.filter_keypoints_batch(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), max_pts, d[3].data_ptr(), d[4].data_ptr(), hc.FILTER_THRESHOLD, cap,
                             keep.data_ptr(), nkeep.data_ptr())
    c.batch_sync()
    raw, kraw, nraw = out.cpu().numpy(), keep.cpu().numpy(), nkeep.cpu().numpy()
    assert (raw[n * 32:] == FILL).all() and (kraw[n * cap:] == FILL).all() and (nraw[n * 4:] == FILL).all()
    krows = kraw[:n * cap].reshape(n, cap)
    for i in range(n):
        assert (krows[i, npts[i]:] == FILL).all(), i
    return raw[:n * 32].view(vislam.F2F_RESULT_DTYPE).copy(), [krows[i, :npts[i]].copy() for i in range(n)], nraw[:n * 4].view(np.int32).copy()


def test_f2f_batch_and_filter(vislam):
    import torch
    assert vislam.F2F_TILE == T
    p = vislam.default_params()
    p.fy, p.f2f_iters = p.fx, hc.ITERS
    rows, _ = hc.f2f_rows(p)
    draws = hc.f2f_draws()
    c = vislam.Context(0, p)
    d_draws = _dev(torch, draws)
    KP = vislam.KEYPOINT_DTYPE

    def clean_rows(ms):
        out = []
        for case in fr.batch_cases(T):
            if case[0] in ms:
                a, b, rot, t = fr.pair_inputs(*case)
                out.append(dict(p1=a, p2=b, rot=rot, t=t))
        return out
    for max_pts, lays, clean in ((120, ("stride5", "first3", "all"), clean_rows((0, 1, 2, 3, 40, 60, 90, 120))),
                                 (T + 1, ("tile_edge",), clean_rows((T - 1, T, T + 1)))):
        keys = [(kind, lay) for lay in lays for kind in hc.pair_kinds() + (hc.mag_pair_kinds() if lay in hc.MAG_LAYOUTS else [])]
        mixed = _interleave([rows[k] for k in keys], clean)
        recs, keeps, nkeeps = _f2f_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, d_draws)
        alone = _f2f_launch(vislam, torch, c, clean, max_pts, d_draws)
        for i, (row, is_hostile, k) in enumerate(mixed):
            if not is_hostile:
                assert recs[i].tobytes() == alone[0][k].tobytes() and keeps[i].tobytes() == alone[1][k].tobytes() and nkeeps[i] == alone[2][k], (max_pts, k)
                continue
            kind, lay = keys[k]
            got = _f2f_dict(recs[i])
            want = _f2f_dict(row["rec"])
            _assert_same(got, want, ("f2f", kind, lay))
            assert keeps[i].tobytes() == row["keep"].tobytes() and int(nkeeps[i]) == row["nkeep"], ("filter", kind, lay)
            hc.check_f2f_row(kind, lay, row, got, keeps[i], nkeeps[i])
            if lay == "stride5":                                   # the single calls: indices reduced on the host, the float scale, no flip
                m = len(row["p1"])
                ka, kb = fr.keypoints(KP, row["p1"]), fr.keypoints(KP, row["p2"])
                g = row["t"].astype(np.float32)
                scale = np.float32(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
                st, sc = c.f2f_ransac(ka, kb, row["rot"], fr.reduce_draws(draws, m)[:hc.ITERS], float(scale))
                sign = np.float32(-1.0 if got["flipped"] else 1.0)
                assert sc == got["count_max"] and (sign * st).astype(np.float32).tobytes() == got["t"].tobytes(), ("f2f single", kind, st, got)
                k1, n1 = c.filter_keypoints(ka, kb, row["rot"], row["t"], hc.FILTER_THRESHOLD)
                assert k1.tobytes() == keeps[i].tobytes() and n1 == int(nkeeps[i]), ("filter single", kind)
        assert any(int(r["best_iter"]) >= 0 for r in alone[0])
        again = _f2f_launch(vislam, torch, c, [r for r, _, _ in mixed], max_pts, d_draws)
        assert again[0].tobytes() == recs.tobytes() and again[2].tobytes() == nkeeps.tobytes() and \
            all(a.tobytes() == b.tobytes() for a, b in zip(keeps, again[1]))
        print(f"f2f + filter, rows of {max_pts}: {len(keys)} hostile and {len(clean)} clean rows, winners {sum(int(r['best_iter']) >= 0 for r in recs)}, kept {int(nkeeps.sum())}")
    bad = _hostile_draws(draws)
    sel = [rows["p1:nan", "stride5"], rows["both:big", "stride5"], rows["p2:ninf", "first3"], rows["both:inf_all", "tile_edge"], clean_rows((T + 1,))[0]]
    recs, _, _ = _f2f_launch(vislam, torch, c, sel, T + 1, _dev(torch, bad))
    for i, row in enumerate(sel):
        with np.errstate(all="ignore"):
            want = fr.f2f(p, row["p1"], row["p2"], row["rot"], bad, row["t"])
        _assert_same(_f2f_dict(recs[i]), _f2f_dict(want), ("f2f draws", i))
    c.close()


# ---------------------------------------------------------------------------------------------- the essential RANSAC on device rows
MAX_PTS, ROW_CAP, EREC = 320, 323, 192


def _essential_launch(vislam, torch, c, rows):
    n = len(rows)
    p1 = np.full((n, MAX_PTS, 2), np.nan, np.float32)
    p2 = np.full((n, MAX_PTS, 2), np.nan, np.float32)
    for i, (a, b) in enumerate(rows):
        p1[i, :len(a)], p2[i, :len(b)] = a, b
    npts = np.array([len(a) for a, _ in rows], np.int32)
    d_p1, d_p2, d_n = _dev(torch, p1), _dev(torch, p2), _dev(torch, npts)
    out, mask = _filled(torch, (n + 1) * EREC), _filled(torch, n * ROW_CAP + 64)
    c.essential_batch(n, d_p1.data_ptr(), d_p2.data_ptr(), d_n.data_ptr(), MAX_PTS, ROW_CAP, mask.data_ptr(), out.data_ptr())
    c.batch_sync()
    raw, mraw = out.cpu().numpy(), mask.cpu().numpy()
    assert (raw[n * EREC:] == FILL).all() and (mraw[n * ROW_CAP:] == FILL).all()
    mrows = mraw[:n * ROW_CAP].reshape(n, ROW_CAP)
    for i in range(n):
        assert (mrows[i, npts[i]:] == FILL).all(), i
    return raw[:n * EREC].view(vislam.POSE_RESULT_DTYPE).copy(), [mrows[i, :npts[i]].copy() for i in range(n)]


def test_essential_batch(vislam, orc):
    import torch
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    op = orc.Params()
    for f, _ in p._fields_:
        setattr(op, f, getattr(p, f))
    rows, _ = hc.essential_rows(orc, op)
    c = vislam.Context(0, p)
    keys = list(rows.keys())
    assert sorted({k[2] for k in keys}) == list(hc.ESSENTIAL_LENGTHS)
    lens = (0, 4, 5, 6, 64, 257, 300)                              # the rows of tests/test_essential_batch_gpu.py
    clean = [er.make_scene(("general", "forward", "sideways")[i % 3], m, 0.3, 0.25 if m >= 64 else 0.0, seed=100 + i)[:2]
             for i, m in enumerate(lens[(i + 3) % len(lens)] for i in range(17))]
    mixed = _interleave([(rows[k]["p1"], rows[k]["p2"]) for k in keys], clean)
    recs, masks = _essential_launch(vislam, torch, c, [r for r, _, _ in mixed])
    alone_r, alone_m = _essential_launch(vislam, torch, c, clean)
    assert any(int(r["iters_run"]) > 16 for r in alone_r)          # the work-list kernels ran on clean and hostile rows together
    models = 0
    for i, ((a, b), is_hostile, k) in enumerate(mixed):
        if not is_hostile:
            assert recs[i].tobytes() == alone_r[k].tobytes() and masks[i].tobytes() == alone_m[k].tobytes(), ("clean", k)
            continue
        kind, lay, m = keys[k]
        where = ("essential", kind, lay, m)
        row, r = rows[kind, lay, m], recs[i]
        # the yardstick of tests/test_essential_batch_gpu.py: the single calls on the row alone (R, t are NaN there without a model, 0 here)
        E, mask1, ninl, iters = c.essential_ransac(a, b)
        R, t, ngood = c.recover_pose(E, a, b)
        assert hc.same_value(r["E"], E.reshape(9)) and (int(r["n_inliers"]), int(r["iters_run"]), int(r["n_points"])) == (ninl, iters, m), (where, r)
        assert masks[i].tobytes() == mask1.tobytes(), where
        if E.any():
            models += 1
            assert hc.same_value(r["R"], R.reshape(9)) and hc.same_value(r["t"], t) and int(r["n_pose_good"]) == ngood, (where, r, R, t)
        else:
            assert not r["R"].any() and not r["t"].any() and int(r["n_pose_good"]) == 0 and ninl == 0 and np.isnan(R).all(), (where, r)
        # the oracle, directly: counts, iterations and mask equal, E up to sign within the smoke check's 1e-6
        assert (int(r["n_inliers"]), int(r["iters_run"])) == (row["n_inliers"], row["iters_run"]) and masks[i].tobytes() == row["mask"].tobytes(), (where, r)
        sgn = 1.0 if float((r["E"] * row["E"]).sum()) >= 0 else -1.0
        assert np.abs(r["E"] - sgn * row["E"]).max() < 1e-6, where
        if E.any():
            assert int(r["n_pose_good"]) == row["n_pose_good"], (where, r)
        hc.check_essential_row(kind, lay, m, row, r["E"], masks[i], r["n_inliers"], r["iters_run"], R, t, r["n_pose_good"], int(p.ransac_max_iters))
    assert models >= len(keys) // 2
    print(f"essential: {len(keys)} hostile and {len(clean)} clean rows, {models} hostile rows with a model")
    recs2, masks2 = _essential_launch(vislam, torch, c, [r for r, _, _ in mixed])
    assert recs2.tobytes() == recs.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(masks, masks2))
    c.close()


def test_warp_and_guided_window_on_the_ladder(vislam):
    """vis_warp_keypoints and the window predicate of the guided 2-NN with keypoints at the magnitudes of hc.MAG_LADDER, in the current frame
    (whose prediction overflows to +-inf or to inf - inf = NaN) and in the previous one (whose difference from every prediction does): bit
    for bit the numpy restatement, and from k = 1e-6 up such a keypoint is nobody's neighbour"""
    import guided_match_ref as gr
    rng = np.random.default_rng(23)
    rot = gr.WARP_ROTS[1]
    xy_cur = gr.warp_points()[:120].copy()
    xy_prev = np.concatenate([gr.warp(xy_cur, rot), gr.warp(xy_cur[:40], rot) + np.float32(2.0)]).astype(np.float32)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    d_cur, d_prev = pool[rng.integers(0, 6, len(xy_cur))], pool[rng.integers(0, 6, len(xy_prev))]
    names = hc.MAG_NAMES
    lad_cur, lad_prev = 2 * np.arange(len(names)), 3 * np.arange(len(names)) + 1
    for j, name in enumerate(names):                               # one coordinate each: x and y in turn
        ax = (j // 2) % 2                                          # (the names alternate in sign)
        xy_cur[lad_cur[j], ax] = hc.mag_pixel(name, ax)
        xy_prev[lad_prev[j], 1 - ax] = hc.mag_pixel(name, 1 - ax)
    assert (np.abs(xy_cur[lad_cur]).max(1) > 1e9).all() and (np.abs(xy_prev[lad_prev]).max(1) > 1e9).all() and np.isfinite(xy_cur).all()
    far = np.array([hc.mag_of("p1:" + n) >= hc.MAG_NEVER_FROM for n in names])
    c = vislam.Context(0)
    got, want = c.warp_keypoints(gr.keypoints(xy_cur), rot), gr.warp(xy_cur, rot)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all() and got[~nan].tobytes() == want[~nan].tobytes(), np.argwhere(got != want)[:6]
    assert nan[lad_cur].any() and not nan[lad_cur].all()           # some turn behind the camera, the others project to an ordinary pixel
    k12, k21, adm = gr.knn2(d_prev, xy_prev, d_cur, xy_cur, rot, gr.RADIUS)
    assert not adm[:, lad_cur[far]].any() and not adm[lad_prev[far], :].any() and adm.any(1).sum() > 100
    g12, g21 = c.bf_knn2_hamming_guided_host(d_prev, gr.keypoints(xy_prev), d_cur, gr.keypoints(xy_cur), rot, gr.RADIUS)
    assert g12.tobytes() == gr.dmatches(k12).tobytes() and g21.tobytes() == gr.dmatches(k21).tobytes()
    assert (g21["trainIdx"][lad_cur[far]] == -1).all() and (g12["trainIdx"][lad_prev[far]] == -1).all()
    c.close()


def test_essential_refine_count(vislam):
    """the refinement's reported counts on pixels with an infinite coordinate: the finite-side rule's second place, against the restatement"""
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    base = hc.essential_base(hc.M)
    idx = hc.layout("stride5", hc.M)
    cam, ep = er.Camera(p.fx, p.cx, p.cy), er.default_params()
    c = vislam.Context(0, p)
    for kind in hc.PAIR_NONFINITE:
        h = hc.hostile(kind, base, idx)
        got = c.essential_refine(base["R"], base["t"], h["p1"], h["p2"])
        want = er.refine(cam, ep, base["R"], base["t"], h["p1"], h["p2"])
        _assert_same(np.frombuffer(got.tobytes(), want.dtype)[0], want, ("essential refine", kind))
        assert (int(got["n_inliers0"]), int(got["n_inliers_refined"])) == (32, 32), (kind, got)
    c.close()
