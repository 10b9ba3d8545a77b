"""CPU: the KLT restatement tests/klt_ref.py against an independent float64 Lucas-Kanade and against truth, on analytic scenes (a sum of
Gaussian blobs evaluated at shifted coordinates and rounded to u8, 160 x 120, so the true displacement is known exactly).

The independent method: float pyramids (plain 2 x 2 means), plain bilinear sampling, Scharr / 32 gradients of the float level, the normal
equations solved by numpy.linalg.solve; same windows, levels, iteration limit and stop rule.

The rule, per point that the independent method puts within 0.5 px of truth: restated error <= max(2 x the independent error on the same
point, epsilon) -- 2 because both draw from the same u8 quantisation noise, epsilon because both stop once a step is below it.  Such points
are >= 90 % of the restatement's tracked points in every case, and for shifts <= 11 px >= 75 % of the grid is tracked."""
import numpy as np
import pytest

import klt_ref as kr

W, H = 160, 120
SHIFTS = [(0.37, -0.21), (3.3, -2.2), (9.6, 5.4), (12.1, 6.4)]          # |s| = 0.43, 3.97, 11.01, 13.69 px
GRID = np.array([(24.3 + 11.1 * i + 0.17 * j, 22.6 + 10.7 * j + 0.23 * i) for j in range(7) for i in range(10)], np.float32)   # 70 fractional points


@pytest.fixture(scope="module")
def scenes(orc):
    out = {}
    for s in SHIFTS:
        a, b = kr.blob_scene(W, H, s)
        out[s] = (a, b, kr.frame_from(orc, a), kr.frame_from(orc, b))
    return out


# ---- the independent method
def _float_pyramid(img):
    lv = [img.astype(np.float64)]
    for _ in range(3):
        a = lv[-1]
        a = a[:a.shape[0] // 2 * 2, :a.shape[1] // 2 * 2]
        lv.append((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4.0)
    return lv


def _scharr32(a):
    p = np.pad(a, 1, mode="reflect")
    gx = (3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])) / 32.0
    gy = (3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])) / 32.0
    return gx, gy


def _bilinear(a, x, y):
    X, Y = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - X, y - Y
    return (1 - fx) * (1 - fy) * a[Y, X] + fx * (1 - fy) * a[Y, X + 1] + (1 - fx) * fy * a[Y + 1, X] + fx * fy * a[Y + 1, X + 1]


def independent_lk(img1, img2, pts, r=7, first=3, last=0, max_iters=10, eps=0.01, guess=None):
    """-> (positions m x 2 float64, NaN where the window left a level at level 0 or the matrix was singular)"""
    p1, p2 = _float_pyramid(img1), _float_pyramid(img2)
    o = np.arange(-r, r + 1, dtype=np.float64)
    oy, ox = np.meshgrid(o, o, indexing="ij")
    out = np.full((len(pts), 2), np.nan)
    for k, p0 in enumerate(np.asarray(pts, np.float64)):
        d = np.zeros(2) if guess is None else (np.asarray(guess[k], np.float64) - p0) / 2.0 ** first
        ok = False
        for l in range(first, last - 1, -1):
            if l < first:
                d = 2.0 * d
            a, b = p1[l], p2[l]
            gx, gy = _scharr32(a)
            p = (p0 + 0.5) / 2.0 ** l - 0.5
            inside = lambda q: q[0] - r >= 0 and q[1] - r >= 0 and q[0] + r + 1 < a.shape[1] - 1 and q[1] + r + 1 < a.shape[0] - 1
            ok = False
            if not inside(p):
                continue
            T, Dx, Dy = _bilinear(a, p[0] + ox, p[1] + oy), _bilinear(gx, p[0] + ox, p[1] + oy), _bilinear(gy, p[0] + ox, p[1] + oy)
            G = np.array([[(Dx * Dx).sum(), (Dx * Dy).sum()], [(Dx * Dy).sum(), (Dy * Dy).sum()]])
            if np.linalg.cond(G) > 1e12:
                continue
            ok = True
            for _ in range(max_iters):
                q = p + d
                if not inside(q):
                    ok = False
                    break
                e = _bilinear(b, q[0] + ox, q[1] + oy) - T
                u = -np.linalg.solve(G, np.array([(Dx * e).sum(), (Dy * e).sum()]))
                d = d + u
                if u @ u <= eps * eps:
                    break
        if ok:
            out[k] = p0 + d * 2.0 ** last
    return out


@pytest.mark.parametrize("shift", SHIFTS)
def test_restatement_against_independent_lk_and_truth(scenes, shift):
    img1, img2, f1, f2 = scenes[shift]
    kp = kr.default_params()
    rec = kr.track(kp, f1, f2, GRID)
    ind = independent_lk(img1, img2, GRID)
    truth = GRID.astype(np.float64) + np.array(shift)
    tracked = (rec["flags"] & kr.TRACKED) != 0
    got = np.stack([rec["x"], rec["y"]], 1).astype(np.float64)
    err_r = np.hypot(*(got - truth).T)
    err_i = np.hypot(*(ind - truth).T)
    judged = tracked & np.isfinite(err_i) & (err_i <= 0.5)
    broke = judged & (err_r > np.maximum(2.0 * err_i, kp.epsilon))
    pair = kr.pair_record(rec)
    print(f"shift {shift} |{np.hypot(*shift):.2f}|: tracked {tracked.sum()} of {len(GRID)} (flat {pair['n_flat']}, oob {pair['n_oob']}), judged {judged.sum()}, "
          f"median restated error {np.median(err_r[judged]):.4f} px, worst {err_r[judged].max():.4f} px (independent: median "
          f"{np.median(err_i[judged]):.4f}, worst {err_i[judged].max():.4f}), rule broken by {broke.sum()}; "
          f"tracked but not judged: {[(int(i), round(float(err_r[i]), 2), round(float(err_i[i]), 2)) for i in np.nonzero(tracked & ~judged)[0]]}")
    assert not broke.any(), [(int(i), float(err_r[i]), float(err_i[i])) for i in np.nonzero(broke)[0]]
    assert judged.sum() >= 0.9 * tracked.sum()
    if np.hypot(*shift) <= 11.5:
        assert tracked.sum() >= 0.75 * len(GRID)
    assert tracked.sum() > 0 and pair["n_points"] == len(GRID) and pair["n_tracked"] == tracked.sum()


def test_every_flag_on_hand_made_inputs(scenes, orc):
    shift = SHIFTS[1]
    _, _, f1, f2 = scenes[shift]
    kp = kr.default_params()
    flat = np.full((H, W), 77, np.uint8)
    ff = kr.frame_from(orc, flat)
    pts = np.array([[80.25, 60.5], [3.0, 60.0], [80.0, 3.0], [157.0, 60.0], [80.0, 117.0], [np.nan, 5.0], [5.0, np.inf], [-np.inf, 5.0], [1e30, 60.0], [1e9, 1e9],
                    [151.2, 60.0]], np.float32)
    rec = kr.track(kp, f1, f2, pts)
    assert rec["flags"].tolist() == [kr.TRACKED] + [kr.OOB] * 4 + [kr.INVALID] * 3 + [kr.OOB] * 2 + [kr.OOB]
    assert rec[5].tobytes() == rec[6].tobytes() and rec["x"][5] == 0 and rec["iters"][5] == 0      # an invalid point: zero but for the flag
    assert rec["x"][8] == np.float32(1e30) and rec["y"][9] == np.float32(1e9)                         # a lost point reports its input
    assert rec["levels"][0] == 0b0111 and rec["iters"][0] >= 3 and rec["min_eig"][0] >= 0.1 and rec["sad"][0] > 0
    # the last point's template fits at level 0 but the window leaves frame 2 on the way (x + 3.3 + 8 > 159)
    assert rec["levels"][10] & 1 and rec["min_eig"][10] > 0
    # flat: every level is skipped, lost at last_level
    rf = kr.track(kp, ff, ff, pts[:1])
    assert rf["flags"][0] == kr.FLAT and rf["min_eig"][0] == 0 and rf["levels"][0] == 0 and (rf["x"][0], rf["y"][0]) == (pts[0, 0], pts[0, 1])
    # ERR: the same point against a frame of another brightness (the gradients agree, the residual does not)
    f2b = kr.frame_from(orc, np.clip(scenes[shift][1].astype(int) + 40, 0, 255).astype(np.uint8))
    re = kr.track(kr.copy_params(kp, max_err=10.0), f1, f2b, pts[:1])
    assert re["flags"][0] == kr.ERR and re["sad"][0] > 10 * 32 * 225
    assert kr.track(kr.copy_params(kp, max_err=10.0), f1, f2, pts[:1])["flags"][0] == kr.TRACKED
    # FB on a bound no sub-pixel tracker meets exactly, and off on a generous one
    r1 = kr.track(kr.copy_params(kp, fb_max_px=1e-9), f1, f2, pts[:1], )
    r2 = kr.track(kr.copy_params(kp, fb_max_px=0.5), f1, f2, pts[:1])
    assert r1["flags"][0] == kr.FB and r1["fb"][0] > 0 and r2["flags"][0] == kr.TRACKED and r2["fb"][0] == r1["fb"][0] < 0.1
    pr = kr.pair_record(rec)
    assert (pr["n_points"], pr["n_tracked"], pr["n_oob"], pr["n_invalid"], pr["flags"]) == (11, 1, 7, 3, 0)
    assert kr.pair_record(rec, no_pair=True).tobytes() == np.array([(0, 0, 0, 0, 0, 0, 0, 1)], kr.PAIR_DTYPE).tobytes()
    a, b = kr.compact(pts, rec)
    assert a.tolist() == [pts[0].tolist()] and b.tolist() == [[float(rec["x"][0]), float(rec["y"][0])]]


def test_a_negative_last_weight_occurs_and_is_exact():
    """a = b = 0.6 / 16384: the three rounded weights are 16383, 1, 1 and sum to 16385, so w11 = -1; the integer sum is still exact"""
    fr = (np.arange(0, 64) + 0.6) / 16384.0                       # a = b = 0.6 / 16384: 16383 + 1 + 1
    xs, ys = np.meshgrid(10.0 + fr, 10.0 + fr)
    _, _, a00, a01, a10, a11 = kr.taps(xs.ravel(), ys.ravel())
    assert (a00 + a01 + a10 + a11 == 16384).all()
    neg = np.nonzero(a11 < 0)[0]
    assert len(neg) > 0 and a11.min() == -1
    k = neg[0]
    img = np.arange(40 * 40, dtype=np.int64).reshape(40, 40) % 251
    S = kr.sample(img.astype(np.uint8), xs.ravel()[k:k + 1], ys.ravel()[k:k + 1], 2)
    Xk, Yk = int(np.floor(xs.ravel()[k])), int(np.floor(ys.ravel()[k]))
    want = a00[k] * img[Yk, Xk] + a01[k] * img[Yk, Xk + 1] + a10[k] * img[Yk + 1, Xk] + a11[k] * img[Yk + 1, Xk + 1]
    assert int(S[0, 2, 2]) == int(want)
    T = (S + 256) >> 9
    assert T.min() >= 0 and T.max() <= 255 * 32


def test_forward_backward_catches_a_planted_occlusion(scenes, orc):
    shift = SHIFTS[1]
    img1, img2, f1, _ = scenes[shift]
    occl = img2.copy()
    rng = np.random.RandomState(3)
    box = (slice(40, 80), slice(60, 110))                                   # rows, columns of frame 2 replaced by noise
    occl[box] = rng.randint(0, 256, (40, 50))
    f2 = kr.frame_from(orc, occl)
    kp = kr.copy_params(kr.default_params(), fb_max_px=0.5)
    rec = kr.track(kp, f1, f2, GRID)
    truth = GRID.astype(np.float64) + np.array(shift)
    inside = (truth[:, 0] > 68) & (truth[:, 0] < 102) & (truth[:, 1] > 48) & (truth[:, 1] < 72)     # windows wholly inside the planted box
    outside = (truth[:, 0] < 60 - 9) | (truth[:, 0] > 110 + 9) | (truth[:, 1] < 40 - 9) | (truth[:, 1] > 80 + 9)
    assert inside.sum() >= 4
    tr = (rec["flags"] & kr.TRACKED) != 0
    assert not tr[inside].any() and ((rec["flags"][inside] & (kr.FB | kr.OOB | kr.FLAT)) != 0).all()
    plain = kr.track(kr.default_params(), f1, f2, GRID)
    assert ((plain["flags"][inside] & kr.TRACKED) != 0).any()              # without the check some of them pass as tracked
    got = np.stack([rec["x"], rec["y"]], 1)[tr & outside]
    assert (tr & outside).sum() >= 20 and np.hypot(*(got - truth[tr & outside]).T).max() < 0.5


def test_a_guess_shortens_the_iterations(scenes):
    shift = SHIFTS[3]
    _, _, f1, f2 = scenes[shift]
    kp = kr.default_params()
    cold = kr.track(kp, f1, f2, GRID)
    guess = (GRID + np.array(shift, np.float32) + np.float32(0.3)).astype(np.float32)
    warm = kr.track(kp, f1, f2, GRID, guess)
    both = ((cold["flags"] & kr.TRACKED) != 0) & ((warm["flags"] & kr.TRACKED) != 0)
    assert both.sum() >= 30
    assert warm["iters"][both].sum() < cold["iters"][both].sum()
    nan_guess = np.full_like(guess, np.nan)
    assert kr.track(kp, f1, f2, GRID, nan_guess).tobytes() == cold.tobytes()   # a non-finite guess is treated as absent
    print(f"iterations over {both.sum()} points: {cold['iters'][both].sum()} cold, {warm['iters'][both].sum()} with a guess")
