"""The chroma modes of the 4:2:0 boundary (include/pnpvcve.h, "Chroma modes") restated in numpy, both directions, 8 / 10 / 12 bit.

Written from the header's statement, not from the kernels.  A mode says where chroma sample (j, i) lies among the luma samples and
selects the filter of each direction; mode 0 is the boundary tests/yuv_ref.py and tests/yuv16_ref.py pin (replicated in, box mean
out), and this file gives it from the same code path as the others so that it is tied to them.  Planes here are integer SAMPLE VALUES
(what tests/yuv16_ref.values reads out of a container); every constant comes from those two files."""
import numpy as np

import yuv16_ref
import yuv_ref

F = np.float32
MODES = ('replicate', 'center', 'left', 'topleft')      # PNP_YUV_CHROMA_* = the index
DEPTHS = (8, 10, 12)


def mode_index(mode):
    return MODES.index(mode) if isinstance(mode, str) else int(mode)


def cosited(mode):
    """-> (the y axis is co-sited, the x axis is co-sited): chroma lies ON the even luma indices of such an axis, midway otherwise"""
    m = mode_index(mode)
    return m == 3, m >= 2


def constants(standard, depth):
    """the float32 constants of tests/yuv_ref.py (depth 8) or tests/yuv16_ref.py, with `mid` and `top` at every depth"""
    if depth == 8:
        return dict(yuv_ref.constants(standard), mid=128, top=255)
    return yuv16_ref.constants(standard, depth)


def taps(n, co, replicate=False):
    """One axis, n chroma samples: for each luma index k < 2n the two chroma indices and their weights in quarters, (i0, w0, i1, w1).
    co-sited: even k (i: 4), odd k (i: 2, min(i+1, n-1): 2); midway: even k (i: 3, max(i-1, 0): 1), odd k (i: 3, min(i+1, n-1): 1);
    replication is (i: 4) for both."""
    k = np.arange(2 * n)
    i = k >> 1
    odd = (k & 1) == 1
    if replicate:
        return i, np.full(2 * n, 4), i, np.zeros(2 * n, int)
    other = np.where(odd, np.minimum(i + 1, n - 1), np.maximum(i - 1, 0))
    if co:
        return i, np.where(odd, 2, 4), np.where(odd, other, i), np.where(odd, 2, 0)
    return i, np.full(2 * n, 3), other, np.ones(2 * n, int)


def upsample16(c, mode):
    """integer chroma (..., rows, cols), the midpoint already taken off -> (..., 2 rows, 2 cols) int64: 16 times the chroma at every
    luma position, the exact integer sum of wy * wx * c"""
    c = np.asarray(c).astype(np.int64)
    m = mode_index(mode)
    yco, xco = cosited(m)
    i0, w0, i1, w1 = taps(c.shape[-1], xco, m == 0)
    c = w0 * c[..., i0] + w1 * c[..., i1]
    i0, w0, i1, w1 = taps(c.shape[-2], yco, m == 0)
    return w0[:, None] * c[..., i0, :] + w1[:, None] * c[..., i1, :]


def from_planes(Y, Cb, Cr, standard, depth=8, mode=0):
    """sample values Y (..., h, w), Cb / Cr (..., h/2, w/2) -> (..., 3, h, w) float32 RGB clamped to [0, 1]"""
    k = constants(standard, depth)
    y = k['cy'] * (np.asarray(Y).astype(np.int32) - k['yoff']).astype(F)
    u16 = upsample16(np.asarray(Cb).astype(np.int64) - k['mid'], mode)
    v16 = upsample16(np.asarray(Cr).astype(np.int64) - k['mid'], mode)
    u, v = u16.astype(F) * F(0.0625), v16.astype(F) * F(0.0625)
    r = y + k['crv'] * v
    g = (y - k['cgu'] * u) - k['cgv'] * v
    b = y + k['cbu'] * u
    out = np.stack([r, g, b], axis=-3)
    assert out.dtype == F
    return np.minimum(np.maximum(out, F(0)), F(1))


def _three(p):
    """the last axis co-sited: sample i from the taps max(2i - 1, 0), 2i, 2i + 1 as ((pL + pR) + (pC + pC)) * 0.25"""
    n = p.shape[-1] // 2
    left = np.maximum(2 * np.arange(n) - 1, 0)
    pc, pr_, pl = p[..., 0::2], p[..., 1::2], p[..., left]
    return ((pl + pr_) + (pc + pc)) * F(0.25)


def _two(p):
    """the last axis midway: (p0 + p1) * 0.5"""
    return (p[..., 0::2] + p[..., 1::2]) * F(0.5)


def downsample(p, mode):
    """float32 (..., h, w) per-pixel pb or pr -> (..., h/2, w/2): the box mean (modes 0, 1); each row across with the three taps, then
    the two rows of a sample combined (left) or the rows max(2j - 1, 0), 2j, 2j + 1 with the three taps again (topleft)"""
    m = mode_index(mode)
    p = np.asarray(p, F)
    if m < 2:
        return ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * F(0.25)
    a = np.swapaxes(_three(p), -1, -2)          # rows last
    out = np.swapaxes(_three(a) if m == 3 else _two(a), -1, -2)
    assert out.dtype == F
    return out


def to_planes(planes, standard, depth=8, mode=0):
    """(..., 3, h, w) float32 -> the sample values y (..., h, w), cb, cr (..., h/2, w/2) as uint16"""
    k = constants(standard, depth)
    x = np.minimum(np.maximum(np.asarray(planes, F), F(0)), F(1))
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yl = (k['kr'] * r + k['kg'] * g) + k['kb'] * b
    pb, pr = (b - yl) * k['ipb'], (r - yl) * k['ipr']
    assert yl.dtype == F and pb.dtype == F
    code = lambda v: np.minimum(np.maximum(np.rint(v), F(0)), F(k['top'])).astype(np.uint16)      # np.rint: half to even
    return (code(F(k['yoff']) + k['sy'] * yl), code(F(k['mid']) + k['sc'] * downsample(pb, mode)),
            code(F(k['mid']) + k['sc'] * downsample(pr, mode)))
