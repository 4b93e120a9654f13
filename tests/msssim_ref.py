"""MS-SSIM as include/pnpvcve.h states it (pnp_msssim_*), restated with scipy.ndimage -- independently of pnp_vcve_amd.metrics: it
shares no helper with it.  The window is applied with scipy.ndimage.correlate1d along both axes and the 'valid' region is cut out of
the result (5 samples from every side: there the border mode never enters); the pyramid is a reshape-mean.

    plane_scales(a, b, peak) -> (5, 2) float64: the raw (CS_s, S_s) of one plane pair
    value(scales)            -> prod_{s<4} max(CS_s, 0)^w_s * max(S_4, 0)^w_4
    level_shapes(h, w, crop) -> [(rows, cols)] * 5, or None below 176 x 176
"""
import numpy as np
from scipy import ndimage

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
MIN_SIZE = 176


def level_shapes(h, w, crop=0):
    h, w = h - 2 * crop, w - 2 * crop
    if crop < 0 or min(h, w) < MIN_SIZE:
        return None
    out = []
    for _ in range(5):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def blocks_of(rows, cols):
    """16 x 32 tiles of the (rows - 10) x (cols - 10) valid map"""
    return -(-(rows - 10) // 16) * -(-(cols - 10) // 32)


def pyramid(x, dtype=np.float32):
    """the five levels of a plane: 2 x 2 means formed in float64 and stored as `dtype`; an odd last row / column is dropped"""
    levels = [np.asarray(x).astype(dtype)]
    for _ in range(4):
        p = levels[-1]
        h, w = p.shape[0] // 2, p.shape[1] // 2
        q = p[:2 * h, :2 * w].astype(np.float64).reshape(h, 2, w, 2)
        # ((x00 + x01) + (x10 + x11)) * 0.25, in that order
        levels.append((((q[:, 0, :, 0] + q[:, 0, :, 1]) + (q[:, 1, :, 0] + q[:, 1, :, 1])) * 0.25).astype(dtype))
    return levels


def _window():
    k = np.exp(-0.5 * ((np.arange(11) - 5.0) / 1.5) ** 2)
    return k / k.sum()


def _filt(x, k):
    y = ndimage.correlate1d(x, k, axis=1, mode='constant', cval=0.0)
    y = ndimage.correlate1d(y, k, axis=0, mode='constant', cval=0.0)
    return y[5:-5, 5:-5]


def plane_scales(a, b, peak=255.0):
    k = _window()
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    out = np.zeros((5, 2))
    for s, (x, y) in enumerate(zip(pyramid(a), pyramid(b))):
        x, y = x.astype(np.float64), y.astype(np.float64)
        mx, my = _filt(x, k), _filt(y, k)
        vx, vy, cxy = _filt(x * x, k) - mx * mx, _filt(y * y, k) - my * my, _filt(x * y, k) - mx * my
        cs = (2.0 * cxy + c2) / (vx + vy + c2)
        lum = (2.0 * mx * my + c1) / (mx * mx + my * my + c1)
        out[s] = np.mean(cs), np.mean(lum * cs)
    return out


def value(scales):
    scales = np.asarray(scales, np.float64)
    f = np.concatenate([scales[..., :4, 0], scales[..., 4:5, 1]], axis=-1)
    return np.prod(np.maximum(f, 0.0) ** WEIGHTS, axis=-1)


def test_pair(h, w, seed, peak=255, planes=1):
    """(planes, h, w) integer planes a, b in [0, peak]: a smooth pattern plus noise, and `a` blended with its 8 x 8 block means plus a
    small offset (constant, plus one per 32 x 32 block) -- every level's CS_s and S_s then lies well inside (0.1, 0.999)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b = [], []
    for p in range(planes):
        smooth = 0.5 + 0.22 * np.sin(xx / (9.0 + 3 * p) + 0.3 * p) * np.cos(yy / (13.0 - 2 * p)) + 0.12 * np.sin((xx + 2 * yy) / 41.0)
        x = np.clip(smooth + 0.10 * rng.standard_normal((h, w)), 0.0, 1.0)
        hb, wb = -(-h // 8), -(-w // 8)
        pad = np.pad(x, ((0, hb * 8 - h), (0, wb * 8 - w)), mode='edge')
        means = pad.reshape(hb, 8, wb, 8).mean(axis=(1, 3)).repeat(8, axis=0).repeat(8, axis=1)[:h, :w]
        # an offset that differs from one 32 x 32 block to the next: a distortion that survives down to level 4
        coarse = rng.standard_normal((-(-h // 32), -(-w // 32))).repeat(32, axis=0).repeat(32, axis=1)[:h, :w]
        y = np.clip(0.45 * x + 0.55 * means + 0.03 + 0.04 * rng.standard_normal((h, w)) + 0.06 * coarse, 0.0, 1.0)
        a.append(np.rint(x * peak))
        b.append(np.rint(y * peak))
    return np.stack(a).astype(np.int64), np.stack(b).astype(np.int64)


test_pair.__test__ = False      # (a helper, not a test)
