"""The 10 / 12-bit Y'CbCr 4:2:0 boundary's arithmetic (include/pnpvcve.h, pnp_yuv420_planes16) restated in numpy.

The reference has no such path, so the mode is pinned to this restatement: the library must be bit-equal to it.  The formulas are
tests/yuv_ref.py's with the constants of the depth d (s = 2^(d-8)): every constant is evaluated in double and rounded to float32
once; every product and sum after that is a float32 operation rounded on its own.  A sample lives in a 16-bit little-endian word,
low-aligned (value & (2^d - 1)) or high-aligned (word >> (16 - d)); written words carry zeros outside the value."""
import numpy as np

import yuv_ref

STANDARDS = yuv_ref.STANDARDS
DEPTHS = (10, 12)
F = np.float32
# layout name -> (plane order of tests/yuv_ref.pack, bit depth, msb_aligned)
LAYOUTS = {'p010': ('nv12', 10, True), 'p012': ('nv12', 12, True), 'yuv420p10le': ('i420', 10, False), 'yuv420p12le': ('i420', 12, False)}


def constants(standard, depth):
    """-> dict of the float32 constants (and yoff, mid, top) of PNP_YUV_* `standard` (an index or a name) at `depth` bits"""
    assert depth in DEPTHS
    i = STANDARDS.index(standard) if isinstance(standard, str) else int(standard)
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[i >> 1]
    kg = 1.0 - kr - kb
    s, top = float(1 << (depth - 8)), float((1 << depth) - 1)
    sy, sc, yoff = ((219.0 * s, 224.0 * s, 16 << (depth - 8)), (top, top, 0))[i & 1]
    return dict(yoff=yoff, mid=1 << (depth - 1), top=(1 << depth) - 1,
                cy=F(1.0 / sy), crv=F(2.0 * (1.0 - kr) / sc), cbu=F(2.0 * (1.0 - kb) / sc),
                cgu=F(2.0 * kb * (1.0 - kb) / (kg * sc)), cgv=F(2.0 * kr * (1.0 - kr) / (kg * sc)),
                kr=F(kr), kg=F(kg), kb=F(kb), sy=F(sy), sc=F(sc), ipb=F(0.5 / (1.0 - kb)), ipr=F(0.5 / (1.0 - kr)))


def values(words, depth, msb_aligned):
    """uint16 words of a container -> the sample values (int32): total, whatever the other bits hold"""
    w = np.asarray(words).view(np.uint16).astype(np.int32)
    return (w >> (16 - depth)) if msb_aligned else (w & ((1 << depth) - 1))


def words(vals, depth, msb_aligned):
    """sample values -> uint16 words of a container, the bits outside the value zero"""
    v = np.asarray(vals).astype(np.uint16)
    return (v << np.uint16(16 - depth)) if msb_aligned else v


def rgb_from_values(Y, Cb, Cr, standard, depth):
    """integer sample values of one shape (chroma already replicated) -> float32 (..., 3) RGB clamped to [0, 1]"""
    k = constants(standard, depth)
    y = k['cy'] * (Y.astype(np.int32) - k['yoff']).astype(F)
    u = (Cb.astype(np.int32) - k['mid']).astype(F)
    v = (Cr.astype(np.int32) - k['mid']).astype(F)
    r = y + k['crv'] * v
    g = (y - k['cgu'] * u) - k['cgv'] * v
    b = y + k['cbu'] * u
    out = np.stack([r, g, b], axis=-1)
    assert out.dtype == F
    return np.minimum(np.maximum(out, F(0)), F(1))


def from_yuv16(y, cb, cr, standard, depth, msb_aligned=False):
    """y (..., h, w), cb / cr (..., h/2, w/2) uint16 words -> (..., 3, h, w) float32: chroma replicated"""
    up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)
    Y, Cb, Cr = (values(p, depth, msb_aligned) for p in (y, cb, cr))
    return np.moveaxis(rgb_from_values(Y, up(Cb), up(Cr), standard, depth), -1, -3)


def pre_round(planes, standard, depth):
    """(..., 3, h, w) float32 -> the float32 values the three planes are rounded from: (y, cb, cr) before rint and the clamp"""
    k = constants(standard, depth)
    x = np.minimum(np.maximum(np.asarray(planes, F), F(0)), F(1))
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yl = (k['kr'] * r + k['kg'] * g) + k['kb'] * b
    pb, pr = (b - yl) * k['ipb'], (r - yl) * k['ipr']

    def box(p):      # ((p00 + p01) + (p10 + p11)) * 0.25: rows top then bottom, columns left then right
        return ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * F(0.25)

    out = F(k['yoff']) + k['sy'] * yl, F(k['mid']) + k['sc'] * box(pb), F(k['mid']) + k['sc'] * box(pr)
    assert all(o.dtype == F for o in out)
    return out


def to_yuv16(planes, standard, depth, msb_aligned=False):
    """(..., 3, h, w) float32 -> y (..., h, w), cb, cr (..., h/2, w/2) uint16 words of the container"""
    top = F((1 << depth) - 1)
    code = lambda x: np.minimum(np.maximum(np.rint(x), F(0)), top).astype(np.uint16)      # np.rint: half to even
    return tuple(words(code(p), depth, msb_aligned) for p in pre_round(planes, standard, depth))


def pack(y, cb, cr, order, pitch=None):
    """planes of words -> one packed uint16 buffer (..., 3h/2, pitch) with yuv_ref.pack's plane orders ('nv12' | 'nv21' | 'i420'),
    samples for bytes; the words of a row beyond the frame's width are 0"""
    h, w = y.shape[-2:]
    pitch = w if pitch is None else pitch
    buf = np.zeros(y.shape[:-2] + (h * 3 // 2, pitch), np.uint16)
    buf[..., :h, :w] = y
    if order in ('nv12', 'nv21'):
        a, b = (cb, cr) if order == 'nv12' else (cr, cb)
        buf[..., h:, 0:w:2] = a
        buf[..., h:, 1:w:2] = b
    else:
        assert pitch % 2 == 0
        flat = buf.reshape(y.shape[:-2] + (-1,))
        c0, n = h * pitch, (h // 2) * (pitch // 2)
        for j, c in enumerate((cb, cr)):
            rows = flat[..., c0 + j * n:c0 + (j + 1) * n].reshape(y.shape[:-2] + (h // 2, pitch // 2))
            rows[..., :w // 2] = c
    return buf


def ssim_plane(a, b, depth):
    """float64 SSIM of two (rows, cols) planes of sample values with the 11-tap Gaussian window (sigma 1.5), valid region only,
    L = 2^depth - 1: the definition pnp_ssim_partials_yuv420p16's sums are held to"""
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 * 1.5))
    g /= g.sum()
    L = float((1 << depth) - 1)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2

    def filt(x):
        rows = sum(g[k] * x[:, k:x.shape[1] - 10 + k] for k in range(11))
        return sum(g[k] * rows[k:rows.shape[0] - 10 + k, :] for k in range(11))

    a, b = a.astype(np.float64), b.astype(np.float64)
    mu1, mu2 = filt(a), filt(b)
    s11, s22, s12 = filt(a * a) - mu1 * mu1, filt(b * b) - mu2 * mu2, filt(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return float(m.mean())
