"""Evaluation metrics with the reference's definitions (host side, numpy).

tensor2img: mmedit/core/misc.py:9-74 ; psnr: mmedit/core/evaluation/metrics.py:170-215 ;
ssim: metrics.py:218-355 (11x11 Gaussian sigma 1.5, 'valid' window).  The reference computes
SSIM with cv2.filter2D; cv2 is not available here, the same window is applied with a separable
'valid' correlation in float64 (SSIM parity is unpinned against cv2 itself -- SURVEY.md section 8c --
but checked against an independent scipy.ndimage restatement of the reference formula,
tests/test_host_logic.py::test_ssim_against_independent_scipy_restatement).

Reference quirk kept: with crop_border != 0 the reference slices `img[cb:-cb, cb:-cb, None]`
(metrics.py:343-345), which turns an HWC image into (H', W', 1, 3); its channel loop then runs once
over `img[..., 0]`, i.e. SSIM is computed on channel 0 (B of the BGR image) only.  PSNR is a mean over
all elements and is unaffected.  The shipped configs use crop_border=0.

convert_to='y' (metrics.py:200-203, 338-343): `mmcv.bgr2ycbcr(img / 255., y_only=True) * 255.` on the float32 BGR image.  mmcv is
not available here; its arithmetic is restated from its published source (mmcv/image/colorspace.py: bgr2ycbcr with y_only and
_convert_input_type_range / _convert_output_type_range for a float32 image) in `bgr2y`; parity with an installed mmcv is unpinned,
like cv2's above.
"""
import numpy as np
import torch


def tensor2img(tensor, out_type=np.uint8, min_max=(0, 1)):
    """(1,3,H,W) / (3,H,W) RGB tensor in [0,1] -> (H,W,3) BGR uint8 (rounded)."""
    if not torch.is_tensor(tensor):
        raise TypeError(f'tensor expected, got {type(tensor)}')
    t = tensor.squeeze(0).squeeze(0).float().detach().cpu().clamp(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    if t.dim() == 3:
        img = np.transpose(t.numpy()[[2, 1, 0], :, :], (1, 2, 0))
    elif t.dim() == 2:
        img = t.numpy()
    else:
        raise ValueError(f'Only support 3D or 2D tensor here. But received with dimension: {t.dim()}')
    if out_type == np.uint8:
        img = (img * 255.0).round()
    return img.astype(out_type)


BGR2Y = [24.966, 128.553, 65.481]       # mmcv's bgr2ycbcr(y_only=True): 219 * (0.114, 0.587, 0.299), the BT.601 luma of B, G, R


def bgr2y(img):
    """mmcv.bgr2ycbcr(img, y_only=True) for a float32 (H,W,3) BGR image in [0,1] -> float32 (H,W) Y in [16/255, 235/255]: the dot
    product and the offset in float64 (np.dot with a list of Python floats), / 255., back to the input's float32."""
    out_img = np.dot(img, BGR2Y) + 16.0
    out_img /= 255.
    return out_img.astype(np.float32)


def _is_y(convert_to, quote_end):
    if isinstance(convert_to, str) and convert_to.lower() == 'y':
        return True
    if convert_to is not None:
        raise ValueError('Wrong color model. Supported values are "Y" and None' + quote_end)
    return False


def psnr(img1, img2, crop_border=0, input_order='HWC', convert_to=None):
    assert img1.shape == img2.shape, f'Image shapes are different: {img1.shape}, {img2.shape}.'
    if input_order == 'CHW':
        img1, img2 = img1.transpose(1, 2, 0), img2.transpose(1, 2, 0)
    a, b = img1.astype(np.float32), img2.astype(np.float32)
    if _is_y(convert_to, '.'):                   # metrics.py:201-206
        a, b = bgr2y(a / 255.) * 255., bgr2y(b / 255.) * 255.
    if crop_border != 0:
        a = a[crop_border:-crop_border, crop_border:-crop_border, None]
        b = b[crop_border:-crop_border, crop_border:-crop_border, None]
    mse = np.mean((a - b) ** 2)
    if mse == 0:
        return float('inf')
    return 20. * np.log10(255. / np.sqrt(mse))


def _gauss_valid(x, k):
    # separable 'valid' correlation with the symmetric 1-D kernel k along both axes
    n = len(k)
    h, w = x.shape
    tmp = np.zeros((h - n + 1, w), np.float64)
    for i in range(n):
        tmp += k[i] * x[i:i + h - n + 1, :]
    out = np.zeros((h - n + 1, w - n + 1), np.float64)
    for i in range(n):
        out += k[i] * tmp[:, i:i + w - n + 1]
    return out


def _ssim_channel(a, b):
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = a.astype(np.float64), b.astype(np.float64)
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    mu1, mu2 = _gauss_valid(a, g), _gauss_valid(b, g)
    s1 = _gauss_valid(a * a, g) - mu1 ** 2
    s2 = _gauss_valid(b * b, g) - mu2 ** 2
    s12 = _gauss_valid(a * b, g) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    return m.mean()


def ssim(img1, img2, crop_border=0, input_order='HWC', convert_to=None):
    assert img1.shape == img2.shape, f'Image shapes are different: {img1.shape}, {img2.shape}.'
    if input_order == 'CHW':
        img1, img2 = img1.transpose(1, 2, 0), img2.transpose(1, 2, 0)
    if _is_y(convert_to, ''):                    # metrics.py:338-346: one channel, the float32 Y
        img1, img2 = img1.astype(np.float32), img2.astype(np.float32)
        img1, img2 = bgr2y(img1 / 255.) * 255., bgr2y(img2 / 255.) * 255.
    if img1.ndim == 2:
        img1, img2 = img1[..., None], img2[..., None]
    if crop_border != 0:       # metrics.py:343-350: the `None` index leaves only channel 0 in the loop (see module docstring)
        img1 = img1[crop_border:-crop_border, crop_border:-crop_border, :1]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, :1]
    return float(np.mean([_ssim_channel(img1[..., i], img2[..., i]) for i in range(img1.shape[2])]))


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003, as published (sum 1.0001)
MSSSIM_MIN_SIZE = 176                                            # level 4 must hold one 11 x 11 window: 11 << 4


def _msssim_down(x):
    """the next level of the pyramid: 2 x 2 means formed in float64 and stored as float32, an odd last row / column dropped"""
    h, w = x.shape[0] // 2, x.shape[1] // 2
    x = x[:2 * h, :2 * w].astype(np.float64)
    return (((x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])) * 0.25).astype(np.float32)


def msssim_plane_scales(a, b, peak=255.0):
    """(5, 2) float64: the raw (CS_s, S_s) of one plane pair -- the means over the valid map of cs and of l * cs at the five levels"""
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    a, b = a.astype(np.float32), b.astype(np.float32)
    out = np.zeros((5, 2), np.float64)
    for s in range(5):
        if s:
            a, b = _msssim_down(a), _msssim_down(b)
        x, y = a.astype(np.float64), b.astype(np.float64)
        mu1, mu2 = _gauss_valid(x, g), _gauss_valid(y, g)
        s1 = _gauss_valid(x * x, g) - mu1 ** 2
        s2 = _gauss_valid(y * y, g) - mu2 ** 2
        s12 = _gauss_valid(x * y, g) - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        lum = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1)
        out[s] = cs.mean(), (lum * cs).mean()
    return out


def msssim_from_scales(scales):
    """(..., 5, 2) raw (CS_s, S_s) -> (...) MS-SSIM = prod_{s<4} max(CS_s, 0)^w_s * max(S_4, 0)^w_4 in float64"""
    scales = np.asarray(scales, np.float64)
    w = np.array(MSSSIM_WEIGHTS, np.float64)
    f = np.concatenate([scales[..., :4, 0], scales[..., 4:, 1]], axis=-1)
    return np.prod(np.maximum(f, 0.0) ** w, axis=-1)


def msssim(img1, img2, crop_border=0, input_order='HWC', convert_to=None):
    """Multi-scale SSIM (Wang, Simoncelli, Bovik 2003; five scales) of two uint8 BGR images, the definition of include/pnpvcve.h
    (pnp_msssim_*).  It is this project's own: the reference has no MS-SSIM and neither cv2 nor an HM / VTM / libvmaf build is available
    here, so parity with a particular external tool is unpinned; it is checked against the independent scipy restatement
    tests/msssim_ref.py.  Every level uses ssim()'s window; level s+1 is the 2 x 2 mean of level s.  convert_to='y': one plane, the
    float32 Y of ssim().  Several channels give the mean of the channels' values, with or without a crop (ssim()'s crop quirk is the
    reference's and is not carried over).  The cropped image must be at least 176 x 176."""
    assert img1.shape == img2.shape, f'Image shapes are different: {img1.shape}, {img2.shape}.'
    if input_order == 'CHW':
        img1, img2 = img1.transpose(1, 2, 0), img2.transpose(1, 2, 0)
    if _is_y(convert_to, ''):
        img1, img2 = img1.astype(np.float32), img2.astype(np.float32)
        img1, img2 = bgr2y(img1 / 255.) * 255., bgr2y(img2 / 255.) * 255.
    if img1.ndim == 2:
        img1, img2 = img1[..., None], img2[..., None]
    if crop_border != 0:
        img1 = img1[crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border]
    if min(img1.shape[:2]) < MSSSIM_MIN_SIZE:
        raise ValueError(f'MS-SSIM needs {MSSSIM_MIN_SIZE} x {MSSSIM_MIN_SIZE} samples after the crop (level 4 must hold one 11 x 11 '
                         f'window), got {img1.shape[0]} x {img1.shape[1]}')
    scales = np.stack([msssim_plane_scales(img1[..., i], img2[..., i]) for i in range(img1.shape[2])])
    return float(np.mean(msssim_from_scales(scales)))


ALLOWED_METRICS = {'PSNR': psnr, 'SSIM': ssim, 'MS-SSIM': msssim}
