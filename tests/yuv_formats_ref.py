"""The chroma formats of the Y'CbCr boundary (include/pnpvcve.h, "Chroma formats") restated in numpy, both directions, 8 / 10 / 12 bit.

Written from the header's statement, not from the kernels.  A chroma format is a pair of subsampling factors (sx, sy): 4:2:0 (2, 2),
4:2:2 (2, 1), 4:4:4 (1, 1); the chroma planes are (h / sy) x (w / sx).  On an axis whose factor is 2 the chroma mode's taps (on the way
in) and filter (on the way out) of tests/yuv_chroma_ref.py apply; on an axis whose factor is 1 luma index k takes chroma index k with
weight 4 on the way in, and the sample is the pixel's own value on the way out.  Planes are integer SAMPLE VALUES; the constants and
the tap table are tests/yuv_chroma_ref.py's."""
import numpy as np

from yuv_chroma_ref import DEPTHS, MODES, F, constants, cosited, mode_index, taps  # noqa: F401

FORMATS = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}      # name -> (sx, sy); PNP_YUV_FORMAT_* = the index
FORMAT_NAMES = tuple(FORMATS)


def factors(fmt):
    return FORMATS[fmt] if isinstance(fmt, str) else tuple(fmt)


def chroma_shape(h, w, fmt):
    sx, sy = factors(fmt)
    assert h % sy == 0 and w % sx == 0, (h, w, fmt)
    return h // sy, w // sx


def axis_taps(n, factor, co, replicate):
    """one axis of n chroma samples -> (i0, w0, i1, w1) for each of its factor * n luma indices, weights in quarters"""
    if factor == 2:
        return taps(n, co, replicate)
    k = np.arange(n)
    return k, np.full(n, 4), k, np.zeros(n, int)


def upsample16(c, mode, fmt):
    """integer chroma (..., rows, cols), the midpoint already taken off -> (..., sy rows, sx cols) int64: 16 times the chroma at every
    luma position, the exact integer sum of wy * wx * c"""
    c = np.asarray(c).astype(np.int64)
    sx, sy = factors(fmt)
    m = mode_index(mode)
    yco, xco = cosited(m)
    i0, w0, i1, w1 = axis_taps(c.shape[-1], sx, xco, m == 0)
    c = w0 * c[..., i0] + w1 * c[..., i1]
    i0, w0, i1, w1 = axis_taps(c.shape[-2], sy, yco, m == 0)
    return w0[:, None] * c[..., i0, :] + w1[:, None] * c[..., i1, :]


def from_planes(Y, Cb, Cr, standard, depth=8, mode=0, fmt='420'):
    """sample values Y (..., h, w), Cb / Cr (..., h / sy, w / sx) -> (..., 3, h, w) float32 RGB clamped to [0, 1]"""
    k = constants(standard, depth)
    y = k['cy'] * (np.asarray(Y).astype(np.int32) - k['yoff']).astype(F)
    u16 = upsample16(np.asarray(Cb).astype(np.int64) - k['mid'], mode, fmt)
    v16 = upsample16(np.asarray(Cr).astype(np.int64) - k['mid'], mode, fmt)
    assert u16.shape == y.shape, (u16.shape, y.shape)
    u, v = u16.astype(F) * F(0.0625), v16.astype(F) * F(0.0625)
    r = y + k['crv'] * v
    g = (y - k['cgu'] * u) - k['cgv'] * v
    b = y + k['cbu'] * u
    out = np.stack([r, g, b], axis=-3)
    assert out.dtype == F
    return np.minimum(np.maximum(out, F(0)), F(1))


def _axis_down(p, factor, co):
    """the last axis: factor 1 the values themselves; factor 2 midway (p0 + p1) * 0.5, co-sited ((pL + pR) + (pC + pC)) * 0.25 with
    the clamped left tap"""
    if factor == 1:
        return p
    if not co:
        return (p[..., 0::2] + p[..., 1::2]) * F(0.5)
    n = p.shape[-1] // 2
    left = np.maximum(2 * np.arange(n) - 1, 0)
    pc, pr_, pl = p[..., 0::2], p[..., 1::2], p[..., left]
    return ((pl + pr_) + (pc + pc)) * F(0.25)


def downsample(p, mode, fmt):
    """float32 (..., h, w) per-pixel pb or pr -> (..., h / sy, w / sx).  4:2:0 is the 4:2:0 statement's own expression (the box mean
    of modes 0 and 1 is ONE expression over the 2x2 block, not two passes); with a factor of 1 on an axis there is one pass at most."""
    sx, sy = factors(fmt)
    m = mode_index(mode)
    yco, xco = cosited(m)
    p = np.asarray(p, F)
    if (sx, sy) == (2, 2) and not xco:
        return ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * F(0.25)
    a = np.swapaxes(_axis_down(p, sx, xco), -1, -2)          # rows last
    out = np.swapaxes(_axis_down(a, sy, yco), -1, -2)
    assert out.dtype == F
    return out


def to_planes(planes, standard, depth=8, mode=0, fmt='420'):
    """(..., 3, h, w) float32 -> the sample values y (..., h, w), cb, cr (..., h / sy, w / sx) as uint16"""
    k = constants(standard, depth)
    x = np.minimum(np.maximum(np.asarray(planes, F), F(0)), F(1))
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yl = (k['kr'] * r + k['kg'] * g) + k['kb'] * b
    pb, pr = (b - yl) * k['ipb'], (r - yl) * k['ipr']
    assert yl.dtype == F and pb.dtype == F
    code = lambda v: np.minimum(np.maximum(np.rint(v), F(0)), F(k['top'])).astype(np.uint16)      # np.rint: half to even  # noqa: E731
    return (code(F(k['yoff']) + k['sy'] * yl), code(F(k['mid']) + k['sc'] * downsample(pb, mode, fmt)),
            code(F(k['mid']) + k['sc'] * downsample(pr, mode, fmt)))
