"""cv::resize INTER_LINEAR for 8-bit single-channel images, restated in numpy from the published algorithm (OpenCV 3.2
modules/imgproc/src/imgwarp.cpp: resizeGeneric_ with HResizeLinear<uchar, int, short, 2048> and VResizeLinear<uchar, int, short,
FixedPtCast<int, uchar, 22>>).  An independent yardstick for the pyramid: it shares no code with oracle/orb.cpp (which is C++ and
walks pixel by pixel) -- whole-array numpy here, written from the formulas:

    scale  = 1 / (dsize / ssize)                      double, per axis
    f      = (float)((d + 0.5) * scale - 0.5)         source coordinate of destination index d
    s      = floor(f);  f -= s                        fraction in float
    horizontal: s < 0 -> (0, f = 0);  s >= sw - 1 -> (sw - 1, f = 0)          index AND fraction clamped
    vertical:   rows clip(s), clip(s + 1) to [0, sh - 1]                      only the indices; the fraction stays
    coefficients (Q11): round-half-even((1 - f) * 2048), round-half-even(f * 2048), each rounded on its own
    row    = S[sx] * a0 + S[sx + 1] * a1                                      int, < 2^19
    out    = (((b0 * (row0 >> 4)) >> 16) + ((b1 * (row1 >> 4)) >> 16) + 2) >> 2
"""
import numpy as np


def _coords(dlen, slen):
    """(index, fraction) of every destination index along one axis, before any clamp"""
    scale = 1.0 / (float(dlen) / float(slen))                     # double
    f = ((np.arange(dlen, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    return s.astype(np.int64), (f - s.astype(np.float32)).astype(np.float32)


def _q11(f):
    """the coefficient pair of a float32 fraction: each of (1 - f) * 2048 and f * 2048 in float, rounded half to even"""
    one = np.float32(1.0)
    k = np.float32(2048.0)
    return np.rint((one - f) * k).astype(np.int64), np.rint(f * k).astype(np.int64)


def resize_linear(src, dw, dh):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    sh, sw = src.shape
    sx, fx = _coords(dw, sw)
    lo, hi = sx < 0, sx >= sw - 1
    sx = np.where(lo, 0, np.where(hi, sw - 1, sx))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    a0, a1 = _q11(fx)
    sy, fy = _coords(dh, sh)
    b0, b1 = _q11(fy)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    S = src.astype(np.int64)
    # (at sx == sw - 1 the second tap has coefficient 0: any column will do)
    rows = S[:, sx] * a0[None, :] + S[:, np.minimum(sx + 1, sw - 1)] * a1[None, :]
    out = (((b0[:, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
