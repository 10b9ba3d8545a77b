"""Independent numpy reference of rotation-guided matching (TEST INFRASTRUCTURE ONLY): the prediction of VISystem::WarpFunctionRT
(src/VISystem.cpp:771-860) as include/vislam_hip.h restates it, Hamming distances from unpacked bits, the window predicate and the packed
top-2 keys (Hamming << 16 | index, 0xFFFFFFFF = no neighbour).  Nothing here calls the library.  The fixtures of
tests/test_guided_match_gpu.py are built here too, so that tests/test_guided_match_ref.py can assert their preconditions on the CPU."""
import numpy as np

F32 = np.float32
NONE = np.uint32(0xFFFFFFFF)
INTR = (458.654, 457.296, 367.215, 248.375)          # vis_default_params: fx, fy, cx, cy (calibrationEUROC.xml)
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rot_y(deg):
    return rodrigues([0.0, np.deg2rad(deg), 0.0])


def warp(xy, rot, intr=INTR):
    """(n, 2) float32 predictions: a, b and the projection in float32 (numpy rounds every float32 operation), the rows of rot (a, b, 1)
    summed left to right in float64 and narrowed once; (NaN, NaN) where !(X_2 > 0)"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    r = np.asarray(rot, F32).reshape(3, 3)
    fx, fy, cx, cy = (F32(v) for v in intr)
    a = (xy[:, 0] - cx) / fx
    b = (xy[:, 1] - cy) / fy
    assert a.dtype == F32 and b.dtype == F32
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    X = [((np.float64(r[k, 0]) * a64 + np.float64(r[k, 1]) * b64) + np.float64(r[k, 2])).astype(F32) for k in range(3)]
    with np.errstate(all="ignore"):
        x = fx * X[0] / X[2] + cx
        y = fy * X[1] / X[2] + cy
    assert x.dtype == F32 and y.dtype == F32
    out = np.stack([x, y], 1)
    out[~(X[2] > 0)] = np.nan
    return out


def warp_f64(xy, rot, intr=INTR):
    """the same expression evaluated in float64 throughout (rot, intrinsics and points narrowed to float32 first: the same inputs)"""
    xy = np.asarray(xy, F32).reshape(-1, 2).astype(np.float64)
    r = np.asarray(rot, F32).reshape(3, 3).astype(np.float64)
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    a, b = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
    X = [r[k, 0] * a + r[k, 1] * b + r[k, 2] for k in range(3)]
    return np.stack([fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy], 1)


def admissible(prev_xy, pred_xy, radius):
    """(n_prev, n_cur) bool: fabsf(x'_j - x_i) <= radius && fabsf(y'_j - y_i) <= radius in float32; a NaN makes it false"""
    p = np.asarray(prev_xy, F32).reshape(-1, 2)
    q = np.asarray(pred_xy, F32).reshape(-1, 2)
    r = F32(radius)
    with np.errstate(invalid="ignore"):
        dx = np.abs(q[None, :, 0] - p[:, None, 0])
        dy = np.abs(q[None, :, 1] - p[:, None, 1])
        assert dx.dtype == F32
        return (dx <= r) & (dy <= r)


def hamming(dq, dt):
    """(len(dq), len(dt)) int64 Hamming distances from the unpacked bits: the positions where exactly one of the two has a one"""
    a = np.unpackbits(np.ascontiguousarray(dq, np.uint8).reshape(-1, 32), axis=1).astype(F32)
    b = np.unpackbits(np.ascontiguousarray(dt, np.uint8).reshape(-1, 32), axis=1).astype(F32)
    d = a @ (1 - b).T + (1 - a) @ b.T                 # integers <= 256: exact in float32
    return d.astype(np.int64)


def top2_keys(dist, adm):
    """(n_q, 2) uint32: the two smallest (Hamming << 16) | j over the admissible j of every row, 0xFFFFFFFF in the missing places"""
    nq, nt = dist.shape
    keys = (dist.astype(np.uint32) << np.uint32(16)) | np.arange(nt, dtype=np.uint32)[None, :]
    keys = np.where(adm, keys, NONE)
    keys = np.concatenate([keys, np.full((nq, 2), NONE, np.uint32)], 1)
    keys.sort(axis=1)
    return np.ascontiguousarray(keys[:, :2])


def knn2(d_prev, xy_prev, d_cur, xy_cur, rot, radius, intr=INTR):
    """(keys12, keys21, adm): the windowed 2-NN of both directions, prev -> cur and cur -> prev"""
    adm = admissible(xy_prev, warp(xy_cur, rot, intr), radius)
    dist = hamming(d_prev, d_cur)
    return top2_keys(dist, adm), top2_keys(dist.T, adm.T), adm


def dmatches(keys):
    """the library's DMatch rows of a key array (api.hip key_to_dmatch): a missing neighbour is (q, -1, -1, FLT_MAX)"""
    n = len(keys)
    out = np.zeros((n, 2), DMATCH)
    out["queryIdx"] = np.arange(n, dtype=np.int32)[:, None]
    none = keys == NONE
    out["trainIdx"] = np.where(none, -1, (keys & np.uint32(0xFFFF)).astype(np.int32))
    out["imgIdx"] = np.where(none, -1, 0)
    out["distance"] = np.where(none, np.finfo(F32).max, (keys >> np.uint32(16)).astype(F32))
    return out


def keypoints(xy):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    k = np.zeros(len(xy), KEYPOINT)
    k["x"], k["y"], k["size"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, -1
    return k


# ------------------------------------------------------------------------------------------------------------------ fixtures
SMALL_ROT = rodrigues([0.004, -0.006, 0.003]).astype(F32)            # a few pixels of image motion
RADIUS = 8.0
PREV_SIZES = (1, 2, 3, 31, 32, 33, 64, 65, 255, 256, 257)
CUR_SIZES = (1, 2, 31, 32, 33, 65, 300)
POP_QUERIES = (1, 64, 65, 129)
POP_SWEPT = (7, 8, 9, 16, 17)


def _descriptors(rng, n, pool):
    """rows drawn from a small pool with up to three flipped bits: equal distances (ties) are everywhere"""
    d = pool[rng.integers(0, len(pool), n)].copy()
    for i in range(n):
        for _ in range(int(rng.integers(0, 4))):
            d[i, rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return d


def _quarter(rng, n, x0, y0, w, h):
    """n positions on the quarter-pixel grid inside [x0, x0 + w) x [y0, y0 + h)"""
    return np.stack([x0 + rng.integers(0, 4 * w, n) / 4.0, y0 + rng.integers(0, 4 * h, n) / 4.0], 1).astype(F32)


def sized_case(n_prev, n_cur, seed=None):
    """random sets of the given sizes in a region sized so that a row has about two candidates; returns (d_prev, xy_prev, d_cur, xy_cur)"""
    rng = np.random.default_rng(1000 * n_prev + n_cur if seed is None else seed)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    side = int(max(24, np.sqrt(128.0 * max(n_prev, n_cur))))
    return (_descriptors(rng, n_prev, pool), _quarter(rng, n_prev, 200, 150, side, side),
            _descriptors(rng, n_cur, pool), _quarter(rng, n_cur, 200, 150, side, side))


def long_sweep_case():
    """40 previous x 16384 current rows: only current rows of the first and of the last tile of 32 lie near the previous keypoints, every
    other one is hundreds of pixels away -- a key kept from the first tile is aged 511 times before it is written"""
    rng = np.random.default_rng(4242)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    n_prev, n_cur = 40, 16384
    xy_prev = _quarter(rng, n_prev, 100, 100, 48, 48)
    xy_cur = _quarter(rng, n_cur, 450, 250, 250, 200)
    near = np.r_[0:32, n_cur - 32:n_cur]
    xy_cur[near] = _quarter(rng, 64, 100, 100, 48, 48)
    return _descriptors(rng, n_prev, pool), xy_prev, _descriptors(rng, n_cur, pool), xy_cur


def semantics_case():
    """One pair of sets for the window's edge cases, under SMALL_ROT and RADIUS.  Returns (d_prev, xy_prev, d_cur, xy_cur, rows):
      random part      60 previous / 50 current rows in 160 x 120 pixels: rows with 0, 1, 2 and more candidates in both directions, ties
      boundary         current row `cur_edge` predicted at x' in [8, 16) (where a float32 resolves nextafter(8)); previous row `prev_at`
                       sits at exactly x' - 8, previous row `prev_beyond` at x' - nextafter(8), both at y'; prev_beyond has cur_edge's
                       descriptor (distance 0), prev_at differs from it in 9 bits
      masked winners   previous row 0 (`prev_far`) is far from everything and equals the descriptor of current row `cur_victim`, whose only
                       admissible candidate `prev_ok` is 5 bits away and has a higher index; the mirror image with current row 0
                       (`cur_far`), previous row `prev_victim` and current row `cur_ok`
      planted ties     current row `tie_cur` sees the two previous rows `tie_prev_pair` (equal descriptors, 3 bits away) and nothing else;
                       previous row `tie_prev` likewise the two current rows `tie_cur_pair`"""
    rng = np.random.default_rng(99)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    n_prev, n_cur = 60, 50
    d_prev, d_cur = _descriptors(rng, n_prev, pool), _descriptors(rng, n_cur, pool)
    xy_prev, xy_cur = _quarter(rng, n_prev, 200, 150, 160, 120), _quarter(rng, n_cur, 200, 150, 160, 120)
    rows = {}
    # masked winners: rows 0 of both sets move far away (nothing else lives there)
    xy_prev[0], xy_cur[0] = (700.25, 30.5), (30.25, 440.5)
    extra_prev_xy, extra_prev_d, extra_cur_xy, extra_cur_d = [], [], [], []
    fresh = rng.integers(0, 256, (6, 32), dtype=np.uint8)            # descriptors of the planted rows: nowhere near the pool

    def flipped(d, nbits):
        d = d.copy()
        for k in range(nbits):
            d[k] ^= np.uint8(1)
        return d

    # cur_victim at (600.5, 400.25): alone there, with prev_ok at its prediction
    cv = np.array([[600.5, 400.25]], F32)
    rows["cur_victim"] = n_cur + len(extra_cur_xy); extra_cur_xy.append(cv[0]); extra_cur_d.append(fresh[0])
    rows["prev_ok"] = n_prev + len(extra_prev_xy); extra_prev_xy.append(warp(cv, SMALL_ROT)[0] + F32(1.0)); extra_prev_d.append(flipped(fresh[0], 5))
    d_prev[0] = fresh[0]; rows["prev_far"] = 0
    # prev_victim at (650.5, 100.25): alone there, with cur_ok predicted within a pixel or two of it
    pv = np.array([650.5, 100.25], F32)
    rows["prev_victim"] = n_prev + len(extra_prev_xy); extra_prev_xy.append(pv); extra_prev_d.append(fresh[1])
    rows["cur_ok"] = n_cur + len(extra_cur_xy); extra_cur_xy.append(pv + F32(0.5)); extra_cur_d.append(flipped(fresh[1], 5))
    d_cur[0] = fresh[1]; rows["cur_far"] = 0
    # boundary
    ce = np.array([[14.25, 60.5]], F32)
    pe = warp(ce, SMALL_ROT)[0]
    rows["cur_edge"] = n_cur + len(extra_cur_xy); extra_cur_xy.append(ce[0]); extra_cur_d.append(fresh[2])
    r = F32(RADIUS)
    rows["prev_at"] = n_prev + len(extra_prev_xy); extra_prev_xy.append(np.array([pe[0] - r, pe[1]], F32)); extra_prev_d.append(flipped(fresh[2], 9))
    rows["prev_beyond"] = n_prev + len(extra_prev_xy)
    extra_prev_xy.append(np.array([pe[0] - np.nextafter(r, F32(np.inf)), pe[1]], F32)); extra_prev_d.append(fresh[2])
    # planted ties: two equal descriptors, both admissible, 3 bits from the row that sees them -- the lower index must come first
    tc = np.array([[500.5, 300.25]], F32)
    tp = warp(tc, SMALL_ROT)[0]
    rows["tie_cur"] = n_cur + len(extra_cur_xy); extra_cur_xy.append(tc[0]); extra_cur_d.append(fresh[3])
    rows["tie_prev_pair"] = (n_prev + len(extra_prev_xy), n_prev + len(extra_prev_xy) + 1)
    extra_prev_xy += [tp + F32(-1.0), tp + F32(2.0)]; extra_prev_d += [flipped(fresh[3], 3)] * 2
    tq = np.array([450.5, 60.25], F32)
    rows["tie_prev"] = n_prev + len(extra_prev_xy); extra_prev_xy.append(tq); extra_prev_d.append(fresh[4])
    rows["tie_cur_pair"] = (n_cur + len(extra_cur_xy), n_cur + len(extra_cur_xy) + 1)
    extra_cur_xy += [tq + F32(-1.0), tq + F32(1.5)]; extra_cur_d += [flipped(fresh[4], 3)] * 2
    xy_prev = np.concatenate([xy_prev, np.stack(extra_prev_xy)]).astype(F32)
    xy_cur = np.concatenate([xy_cur, np.stack(extra_cur_xy)]).astype(F32)
    d_prev = np.concatenate([d_prev, np.stack(extra_prev_d)])
    d_cur = np.concatenate([d_cur, np.stack(extra_cur_d)])
    return d_prev, xy_prev, d_cur, xy_cur, rows


NAN_ROT = rot_y(80.0).astype(F32)                                     # X_2 = -sin(80 deg) a + cos(80 deg): <= 0 right of u = cx + 81


def nan_case():
    """current keypoints across the whole frame under an 80 degree turn about the y axis: those with X_2 <= 0 predict (NaN, NaN); the
    previous keypoints sit on the predictions of the others (wherever those fall), plus a few at NaN-predicted rows' own positions"""
    rng = np.random.default_rng(31)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    xy_cur = _quarter(rng, 48, 20, 20, 700, 440)
    pred = warp(xy_cur, NAN_ROT)
    ok = ~np.isnan(pred[:, 0])
    xy_prev = np.concatenate([pred[ok], pred[ok] + F32(2.0), xy_cur[~ok][:6]]).astype(F32)
    return _descriptors(rng, len(xy_prev), pool), xy_prev, _descriptors(rng, 48, pool), xy_cur


def warp_points():
    """257 keypoints inside a 752 x 480 frame on the quarter-pixel grid (one workgroup of k_warp and one thread more)"""
    return _quarter(np.random.default_rng(5), 257, 0, 0, 752, 480)


WARP_ROTS = (np.eye(3, dtype=F32), rodrigues([0.05, -0.12, 0.09]).astype(F32), NAN_ROT)      # the third puts some X_2 <= 0
