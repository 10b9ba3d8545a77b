"""CPU: the yardstick of the triangulation tests checked where no GPU is needed -- tests/triangulate_ref.py's Jacobi path against
numpy.linalg.svd of the DLT matrix on the generator's scenes, its float32 parallax against a float64 evaluation, and the contract's
bookkeeping (flags, summary, inliers_only)."""
import numpy as np

import triangulate_ref as tr

FX, CX, CY = tr.EUROC["fx"], tr.EUROC["cx"], tr.EUROC["cy"]


def _compare(seeds):
    worst, n_all, n_cmp, max_sweeps = 0.0, 0, 0, 0
    for seed in seeds:
        R, t, p1, p2, _ = tr.scene(seed)
        Rl, tl = [float(v) for v in R.reshape(9)], [float(v) for v in t]
        for a, b in zip(p1, p2):
            x1, y1 = tr.normalise(a, FX, CX, CY)
            x2, y2 = tr.normalise(b, FX, CX, CY)
            X, front, sweeps, _ = tr.triangulate_point(Rl, tl, x1, y1, x2, y2)
            Xs, front_s = tr.svd_point(R, t, x1, y1, x2, y2)
            n_all += 1
            max_sweeps = max(max_sweeps, sweeps)
            if front_s:
                n_cmp += 1
                worst = max(worst, float(np.abs(np.array(X) - Xs).max() / np.linalg.norm(Xs)))
                assert front, (seed, X, Xs)                    # (no point of these scenes sits within rounding of the 50-unit cut)
    return worst, n_all, n_cmp, max_sweeps


def test_jacobi_path_against_numpy_svd():
    worst, n_all, n_cmp, max_sweeps = _compare(range(100, 110))
    print(f"restated Jacobi vs numpy SVD of A: max |X - X_svd| / |X_svd| = {worst:.3e} on {n_cmp} of {n_all} points, <= {max_sweeps} sweeps")
    assert n_all == 2000 and n_cmp >= 0.95 * n_all
    assert worst <= 1e-9                                        # the project's pose tolerance


def test_jacobi_eigenvectors():
    rng = np.random.default_rng(5)
    for _ in range(50):
        B = rng.normal(0, 1, (4, 4))
        S = B.T @ B
        A = [float(v) for v in S.reshape(16)]
        V, sweeps, _ = tr.jacobi_eig4(A)
        V = np.array(V).reshape(4, 4)
        lam = np.array([A[0], A[5], A[10], A[15]])
        assert 1 <= sweeps < 30
        assert np.abs(V.T @ V - np.eye(4)).max() < 1e-13
        assert np.abs(S @ V - V * lam).max() < 1e-12 * max(1.0, lam.max())
        assert np.allclose(np.sort(lam), np.linalg.eigvalsh(S), rtol=1e-12, atol=1e-13)


def test_parallax_f32_against_float64():
    worst = 0.0
    for seed in range(200, 205):
        R, t, p1, p2, _ = tr.scene(seed)
        Rf = R.astype(np.float32).astype(np.float64)           # the rotation Disparity sees
        for a, b in zip(p1, p2):
            got = tr.parallax_f32(R.reshape(9), a, b, FX, tr.EUROC["fy"], CX, CY)
            f = np.float32
            want = tr.parallax_f64(Rf, a, b, float(f(FX)), float(f(tr.EUROC["fy"])), float(f(CX)), float(f(CY)))
            worst = max(worst, abs(float(got) - want))
    print(f"float32 parallax vs float64: max |diff| = {worst:.3e} px")
    # about ten float32 operations on values below 1000 px: a few ulp of 2^-14 px (6.1e-5) each
    assert worst < 1e-3


def test_contract_bookkeeping():
    R, t, p1, p2, _ = tr.scene(300, n=40)
    k = dict(fx=FX, fy=FX, cx=CX, cy=CY)
    pts, fl, sm, _ = tr.triangulate(R, t, p1, p2, **k)
    assert sm["n_points"] == 40 and sm["n_front"] == int(((fl & tr.MP_FRONT) != 0).sum())
    assert ((fl & tr.MP_INLIER) != 0).all() and ((fl & tr.MP_PARALLAX_OK) != 0).all()
    kept = ((fl & 15) == 15)
    assert (((fl & tr.MP_KEPT) != 0) == kept).all() and sm["n_kept"] == int(kept.sum())
    total = np.float32(0)
    for v in pts["parallax_px"]:
        total = np.float32(total + v)
    assert sm["mean_parallax_px"].tobytes() == np.float32(total / np.float32(40)).tobytes()
    mask = (np.arange(40) % 3 != 0).astype(np.uint8)
    pts2, fl2, sm2, _ = tr.triangulate(R, t, p1, p2, mask=mask, inliers_only=1, **k)
    assert (fl2[mask == 0] == 0).all() and pts2[mask == 0].tobytes() == bytes(32 * int((mask == 0).sum()))
    assert pts2[mask == 1].tobytes() == pts[mask == 1].tobytes() and (fl2[mask == 1] == fl[mask == 1]).all()
    pts3, fl3, sm3, _ = tr.triangulate(R, t, p1, p2, mask=mask, **k)
    assert pts3.tobytes() == pts.tobytes() and (((fl3 & tr.MP_INLIER) != 0) == (mask != 0)).all() and sm3["n_front"] == sm["n_front"]
    assert tr.triangulate(R, t, p1[:0], p2[:0], **k)[2] == dict(n_points=0, n_front=0, n_kept=0, mean_parallax_px=np.float32(0))
