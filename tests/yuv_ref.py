"""The Y'CbCr 4:2:0 boundary's arithmetic (include/pnpvcve.h, pnp_frames_from_yuv420 / pnp_frames_to_yuv420) restated in numpy.

The reference has no YUV input path, so the mode is pinned to this restatement: the library must be bit-equal to it.  Every constant
is evaluated in double from Kr and Kb and rounded to float32 once; every product and sum after that is a float32 operation rounded on
its own (numpy never fuses a multiply with an add)."""
import numpy as np

STANDARDS = ('bt601-limited', 'bt601-full', 'bt709-limited', 'bt709-full')      # PNP_YUV_* = the index
F = np.float32


def constants(standard):
    """-> dict of the float32 constants (and yoff) of PNP_YUV_* `standard` (an index or a name)"""
    s = STANDARDS.index(standard) if isinstance(standard, str) else int(standard)
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[s >> 1]
    kg = 1.0 - kr - kb
    sy, sc, yoff = ((219.0, 224.0, 16), (255.0, 255.0, 0))[s & 1]
    return dict(kr64=kr, kb64=kb, kg64=kg, sy64=sy, sc64=sc, yoff=yoff,
                cy=F(1.0 / sy), crv=F(2.0 * (1.0 - kr) / sc), cbu=F(2.0 * (1.0 - kb) / sc),
                cgu=F(2.0 * kb * (1.0 - kb) / (kg * sc)), cgv=F(2.0 * kr * (1.0 - kr) / (kg * sc)),
                kr=F(kr), kg=F(kg), kb=F(kb), sy=F(sy), sc=F(sc), ipb=F(0.5 / (1.0 - kb)), ipr=F(0.5 / (1.0 - kr)))


def rgb_from_bytes(Y, Cb, Cr, standard, clamp=True):
    """uint8 arrays of one shape (chroma already replicated) -> float32 (..., 3) RGB, clamped to [0, 1] unless clamp=False"""
    k = constants(standard)
    y = k['cy'] * (Y.astype(np.int32) - k['yoff']).astype(F)
    u = (Cb.astype(np.int32) - 128).astype(F)
    v = (Cr.astype(np.int32) - 128).astype(F)
    r = y + k['crv'] * v
    g = (y - k['cgu'] * u) - k['cgv'] * v
    b = y + k['cbu'] * u
    out = np.stack([r, g, b], axis=-1)
    assert out.dtype == F
    return np.minimum(np.maximum(out, F(0)), F(1)) if clamp else out


def rgb_from_bytes_f64(Y, Cb, Cr, standard):
    """the definition in float64, unclamped"""
    k = constants(standard)
    kr, kb, kg, sy, sc = k['kr64'], k['kb64'], k['kg64'], k['sy64'], k['sc64']
    y = (Y.astype(np.float64) - k['yoff']) / sy
    u, v = Cb.astype(np.float64) - 128.0, Cr.astype(np.float64) - 128.0
    r = y + 2.0 * (1.0 - kr) / sc * v
    g = y - 2.0 * kb * (1.0 - kb) / (kg * sc) * u - 2.0 * kr * (1.0 - kr) / (kg * sc) * v
    b = y + 2.0 * (1.0 - kb) / sc * u
    return np.stack([r, g, b], axis=-1)


def frames_from_yuv420(y, cb, cr, standard):
    """y (..., h, w), cb / cr (..., h/2, w/2) uint8 -> (..., 3, h, w) float32: chroma replicated, pixel (yy, xx) reads (yy >> 1, xx >> 1)"""
    up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)
    return np.moveaxis(rgb_from_bytes(y, up(cb), up(cr), standard), -1, -3)


def _byte(x):
    return np.minimum(np.maximum(np.rint(x), F(0)), F(255)).astype(np.uint8)      # np.rint: half to even


def frames_to_yuv420(planes, standard):
    """(..., 3, h, w) float32 -> y (..., h, w), cb, cr (..., h/2, w/2) uint8"""
    k = constants(standard)
    x = np.minimum(np.maximum(np.asarray(planes, F), F(0)), F(1))
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yl = (k['kr'] * r + k['kg'] * g) + k['kb'] * b
    y = _byte(F(k['yoff']) + k['sy'] * yl)
    pb, pr = (b - yl) * k['ipb'], (r - yl) * k['ipr']

    def box(p):      # ((p00 + p01) + (p10 + p11)) * 0.25: rows top then bottom, columns left then right
        return ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * F(0.25)

    assert yl.dtype == F and pb.dtype == F
    return y, _byte(F(128) + k['sc'] * box(pb)), _byte(F(128) + k['sc'] * box(pr))


def pack(y, cb, cr, layout, pitch=None):
    """planes (..., h, w) / (..., h/2, w/2) -> one packed uint8 buffer (..., 3h/2, pitch) in `layout` ('nv12' | 'nv21' | 'i420'); the
    bytes of a row beyond the frame's width are 0.  I420's chroma rows are pitch/2 apart (pitch even)."""
    h, w = y.shape[-2:]
    pitch = w if pitch is None else pitch
    buf = np.zeros(y.shape[:-2] + (h * 3 // 2, pitch), np.uint8)
    buf[..., :h, :w] = y
    if layout in ('nv12', 'nv21'):
        a, b = (cb, cr) if layout == 'nv12' else (cr, cb)
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
