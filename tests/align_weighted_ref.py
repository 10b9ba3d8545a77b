"""numpy restatement of VISystem::EstimatePoseFeatures (src/VISystem.cpp:1113-1448) with the weighting of its Gauss-Newton step as an
argument: IdentityWeights (:1343) or TukeyFunctionWeights / MedianAbsoluteDeviation / MedianMat (:1797-1870).  It follows oracle/align.cpp
operation by operation -- float32 element operations, float64 products and sums where the oracle has them -- and calls the oracle for the
pieces it exports (se3_exp, se3_mul, se3_matrix, lu_invert6, half_pyramid_dims).  Two things are its own:
  - the weights, for every mode and any (tukey_b, mad_scale); mode 1 with the default constants is orc_tukey_weights;
  - candidates are dealt to the 256 partial sums by CANDIDATE index, as k_align deals them (a skipped candidate adds +0.0, which leaves a
    double partial as it was); the oracle deals by residual index.  tests/test_align_weights_ref.py shows that with identity weights the two
    give the same bits on every case the GPU tests use, which is what makes this file a reference for them."""
import numpy as np

from vislam import AlignResult, Se3f

W_IDENTITY, W_TUKEY, W_TUKEY_SIGNED = 0, 1, 2
DEFAULT_B, DEFAULT_MAD_SCALE = 4.6851, 1.4826
LANES = 256
f32, f64 = np.float32, np.float64


def _median_bin(hist, n):
    """MedianMat's rule: the first bin whose running count exceeds (float)(n / 2), integer division (:1851, :1863-1867)"""
    m = f32(n // 2)
    cum = np.cumsum(hist).astype(f32)
    hit = np.nonzero(cum > m)[0]
    return int(hit[0]) if len(hit) else -1


def medians(r, mode):
    """-> (median of the residuals, median of |r - median|) under `mode` (1: both through MedianMat's CV_8U saturation; 2: signed)"""
    r = np.asarray(r, f32)
    n = len(r)
    if mode == W_TUKEY:
        med = _median_bin(np.bincount(np.clip(np.rint(r.astype(f64)), 0, 255).astype(np.int64), minlength=256), n)
    else:
        med = _median_bin(np.bincount(np.rint(r.astype(f64)).astype(np.int64) + 255, minlength=511), n) - 255
    dev = np.abs(r - f32(med))
    if mode == W_TUKEY:
        med2 = _median_bin(np.bincount(np.clip(np.rint(dev.astype(f64)), 0, 255).astype(np.int64), minlength=256), n)
    else:
        med2 = _median_bin(np.bincount(np.rint(dev.astype(f64)).astype(np.int64), minlength=511), n)
    return med, med2


def tukey_weights(r, mode=W_TUKEY, b=DEFAULT_B, mad_scale=DEFAULT_MAD_SCALE):
    """TukeyFunctionWeights over the residuals r (float32, integer values -255 ... 255)"""
    r = np.asarray(r, f32)
    if len(r) == 0:
        return np.zeros(0, f32)
    b = f32(b)
    _, med2 = medians(r, mode)
    MAD = f32(mad_scale) * f32(med2)
    if MAD == 0:
        MAD = f32(1)
    inv_MAD = f32(1.0 / f64(MAD))
    inv_b2 = f32(1.0 / f64(b * b))
    x = r * inv_MAD
    t = (1.0 - ((x * x) * inv_b2).astype(f64)).astype(f32)
    return np.where(np.abs(x) <= b, t * t, f32(0)).astype(f32)


def _intrinsics(ap):
    fx, fy, cx, cy = [f32(ap.fx)], [f32(ap.fy)], [f32(ap.cx)], [f32(ap.cy)]
    for l in range(1, 5):
        fx.append(f32(f64(fx[l - 1]) * 0.5)); fy.append(f32(f64(fy[l - 1]) * 0.5))
        cx.append(f32((f64(cx[0]) + 0.5) / f64(1 << l) - 0.5)); cy.append(f32((f64(cy[0]) + 0.5) / f64(1 << l) - 0.5))
    return fx, fy, cx, cy


def _round_away(v):
    v = v.astype(f64)                                            # std::round: half away from zero
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def _tree(part):
    """256 partials -> one sum per column: inside each 64 strides 32 ... 1, then (G0 + G1) + (G2 + G3)"""
    part = part.copy()
    for g in range(0, LANES, 64):
        off = 32
        while off:
            part[g:g + off] += part[g + off:g + 2 * off]
            off >>= 1
    return (part[0] + part[64]) + (part[128] + part[192])


def estimate_pose_features(orc, ap, w, h, gray1, gray2, gx1, gy1, cand1, init=None, weights=W_IDENTITY, b=DEFAULT_B,
                           mad_scale=DEFAULT_MAD_SCALE):
    fxs, fys, cxs, cys = _intrinsics(ap)
    alw, alh = orc.half_pyramid_dims(w, h)
    pose = Se3f(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0) if init is None else init
    res = AlignResult()
    initial_error = f32(0)
    zf = f32(ap.z_factor)
    with np.errstate(all="ignore"):
        for lvl in range(ap.first_level, ap.last_level - 1, -1):
            cols, rows = w >> lvl, h >> lvl
            acols, arows = int(alw[lvl]), int(alh[lvl])
            c = None if cand1[lvl] is None else np.asarray(cand1[lvl], f32).reshape(-1, 4)
            N = 0 if c is None else len(c)
            fx, fy, cx, cy = fxs[lvl], fys[lvl], cxs[lvl], cys[lvl]
            invfx, invfy = f32(1) / fx, f32(1) / fy
            error, last_error = f32(0), f32(50000)
            k, nres = 0, 0
            for k in range(ap.max_iterations):
                M = orc.se3_matrix(pose).astype(f64)
                if N == 0:
                    nres = 0
                    break
                x1, y1, z1, w1 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
                X = ((x1 - cx) * invfx) * z1
                Y = ((y1 - cy) * invfy) * z1
                P = [(((M[a, 0] * X.astype(f64) + M[a, 1] * Y.astype(f64)) + M[a, 2] * z1.astype(f64)) + M[a, 3] * w1.astype(f64)).astype(f32)
                     for a in range(4)]
                x2 = P[0] * fx; x2 = x2 / P[2]; x2 = x2 + cx
                y2 = P[1] * fy; y2 = y2 / P[2]; y2 = y2 + cy
                x2 = x2 * P[3]; y2 = y2 * P[3]
                z2 = P[2]
                inv_z2 = f32(1) / z2
                valid = (y2 > 0) & (y2 < arows) & (x2 > 0) & (x2 < acols) & (z2 != 0)
                inv_z2 = np.where(inv_z2 < 0, f32(0), inv_z2).astype(f32)
                # 0 <= (int)x1 < cols is -1 < x1 < cols ((int)(-0.5) == 0): decided on the floats, so that no value outside the level -- NaN,
                # +-inf, +-3e38 -- is ever cast to an integer
                inside = (x1 > -1) & (x1 < cols) & (y1 > -1) & (y1 < rows)
                ix1 = np.trunc(np.where(inside, x1, 0)).astype(np.int64)
                iy1 = np.trunc(np.where(inside, y1, 0)).astype(np.int64)
                valid &= inside
                idx = np.nonzero(valid)[0]
                nres = len(idx)
                if nres == 0:
                    break
                x2, y2, iz = x2[idx], y2[idx], inv_z2[idx]
                ix1, iy1 = ix1[idx], iy1[idx]
                rx = np.minimum(_round_away(x2), acols - 1); ry = np.minimum(_round_away(y2), arows - 1)
                zero = np.zeros(nres, f32)
                Jw0 = [fx * iz, zero, -(fx * x2 * iz * iz) * zf, -(fx * x2 * y2 * iz * iz), fx * (f32(1) + x2 * x2 * iz * iz), -fx * y2 * iz]
                Jw1 = [zero, fy * iz, -(fy * y2 * iz * iz) * zf, -(fy * (f32(1) + y2 * y2 * iz * iz)), fy * x2 * y2 * iz * iz, -fy * x2 * iz]
                r = (gray2[lvl][ry, rx].astype(np.int64) - gray1[lvl][iy1, ix1].astype(np.int64)).astype(f32)
                jl0 = gx1[lvl][iy1, ix1].astype(f64); jl1 = gy1[lvl][iy1, ix1].astype(f64)
                J = [(jl0 * Jw0[q].astype(f64) + jl1 * Jw1[q].astype(f64)).astype(f32) for q in range(6)]
                inv_num = f32(1.0 / nres)
                if weights == W_IDENTITY:
                    rhs = r
                    ns = 27
                else:
                    wt = tukey_weights(r, weights, b, mad_scale)
                    rhs = r * wt
                    J = [wt * j for j in J]
                    ns = 28
                contrib = np.zeros((-(-N // LANES) * LANES, ns), f64)
                s = 0
                for a in range(6):
                    for q in range(a, 6):
                        contrib[idx, s] = J[a].astype(f64) * J[q].astype(f64); s += 1
                for a in range(6):
                    contrib[idx, 21 + a] = J[a].astype(f64) * rhs.astype(f64)
                if ns == 28:
                    contrib[idx, 27] = r.astype(f64) * rhs.astype(f64)
                part = np.zeros((LANES, ns), f64)
                for rnd in contrib.reshape(-1, LANES, ns):           # per lane: its candidates in increasing index
                    part += rnd
                S = _tree(part)
                if ns == 28:
                    error = f32(f64(inv_num) * S[27])
                else:
                    error = f32(f64(inv_num) * float(np.sum(r.astype(f64) * r.astype(f64))))   # (integers: exact in any order)
                if k == 0:
                    initial_error = error
                if error >= last_error or k == ap.max_iterations - 1 or abs(f32(error - last_error)) < f32(ap.epsilon):
                    break
                last_error = error
                A = np.zeros((6, 6), f32)
                s = 0
                for a in range(6):
                    for q in range(a, 6):
                        A[a, q] = A[q, a] = f32(S[s]); s += 1
                bb = (-S[21:27]).astype(f32)
                _, Ainv = orc.lu_invert6(A)
                delta = np.zeros(6, f32)
                for a in range(6):
                    acc = f64(0)
                    for q in range(6):
                        acc += f64(Ainv[a, q]) * f64(bb[q])
                    delta[a] = f32(acc)
                pose = orc.se3_mul(pose, orc.se3_exp(delta))
            res.iterations[lvl] = k; res.error[lvl] = error; res.n_residuals[lvl] = nres
    res.initial_error = initial_error
    res.pose = pose
    res.matrix[:] = [float(v) for v in orc.se3_matrix(pose).reshape(16)]
    return res
