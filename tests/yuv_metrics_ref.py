"""The plane metrics of two 8-bit 4:2:0 clips (include/pnpvcve.h, pnp_psnr_sse_yuv420) restated in numpy: per-plane SSE with the crop,
PSNR and the 6:1:1 mean.  Integer arithmetic up to the logarithm, so the library's SSE must equal this one exactly."""
import numpy as np


def crop_plane(p, crop):
    """(..., rows, cols) -> the plane without `crop` samples on every side"""
    return p[..., crop:p.shape[-2] - crop, crop:p.shape[-1] - crop] if crop else p


def plane_sse(a, b, crop):
    """two uint8 planes (..., rows, cols) -> int64 (...): the sum of squared byte differences inside the crop"""
    d = crop_plane(np.asarray(a), crop).astype(np.int64) - crop_plane(np.asarray(b), crop).astype(np.int64)
    return (d * d).sum(axis=(-2, -1))


def sse_yuv420(a, b, crop_border=0):
    """a, b: (y, cb, cr) uint8 arrays (..., h, w) / (..., h/2, w/2) -> int64 (..., 3) = SSE of Y, Cb, Cr: the Y plane cropped by
    crop_border (even), the chroma planes by crop_border / 2"""
    assert crop_border >= 0 and crop_border % 2 == 0
    crops = (crop_border, crop_border // 2, crop_border // 2)
    return np.stack([plane_sse(pa, pb, c) for pa, pb, c in zip(a, b, crops)], axis=-1)


def counts(h, w, crop_border=0):
    """samples of the cropped Y, Cb, Cr planes"""
    n_y = (h - 2 * crop_border) * (w - 2 * crop_border)
    n_c = (h // 2 - crop_border) * (w // 2 - crop_border)          # h/2 - 2 (crop/2)
    return np.array([n_y, n_c, n_c], np.float64)


def psnr_from_sse(sse, h, w, crop_border=0):
    """PSNR_p = 10 log10(255^2 N_p / SSE_p), float64 (..., 3); inf where SSE_p is 0"""
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide='ignore'):
        out = 10.0 * np.log10(255.0 ** 2 * counts(h, w, crop_border) / sse)
    out[sse == 0] = np.inf
    return out


def psnr_yuv420(a, b, crop_border=0):
    h, w = a[0].shape[-2:]
    return psnr_from_sse(sse_yuv420(a, b, crop_border), h, w, crop_border)


def psnr_611(psnr):
    """(..., 3) plane PSNRs -> the 6:1:1 mean (6 Y + U + V) / 8 per frame"""
    return (6.0 * psnr[..., 0] + psnr[..., 1] + psnr[..., 2]) / 8.0
