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


# ---------------------------------------------------------------- PSNR-B (include/pnpvcve.h, pnp_psnrb_*: the one statement of the definition)
# The host path: the five sums of a plane by slicing (psnrb_plane_sums), the pair counts in closed form (psnrb_counts) and the fp64 part
# (psnrb_values), which ops.psnrb_* call on the device's sums too: that part exists once.
PSNRB_BLOCKS = (4, 8, 16, 32, 64)


def psnrb_block(block, chroma=False):
    """the block size of a plane: `block` (one of PSNRB_BLOCKS), half of it on the chroma planes of 4:2:0"""
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in PSNRB_BLOCKS:
        raise ValueError(f'block must be one of {PSNRB_BLOCKS}, got {block!r}')
    return int(block) // 2 if chroma else int(block)


def psnrb_counts(rows, cols, crop=0, plane_block=8):
    """(NBh, NNh, NBv, NNv): the horizontal boundary / other and the vertical boundary / other neighbour pairs inside the crop of a plane of
    rows x cols samples with blocks of plane_block (the plane's own: a power of two, 2 .. 64), the grid anchored at the uncropped origin"""
    bp = int(plane_block)
    if bp < 2 or bp > 64 or bp & (bp - 1):
        raise ValueError(f'a plane block is a power of two from 2 to 64, got {plane_block!r}')
    if rows < 1 or cols < 1 or crop < 0 or 2 * crop >= rows or 2 * crop >= cols:
        raise ValueError(f'a crop of {crop} leaves nothing of a {rows} x {cols} plane')
    h, w = rows - 2 * crop, cols - 2 * crop
    if min(h, w) < bp:
        raise ValueError(f'PSNR-B with blocks of {bp} needs {bp} x {bp} samples after the crop, got {h} x {w}')
    kx = (cols - crop - 1) // bp - crop // bp
    ky = (rows - crop - 1) // bp - crop // bp
    return h * kx, h * (w - 1 - kx), w * ky, w * (h - 1 - ky)


def psnrb_plane_sums(a, b, crop=0, plane_block=8):
    """(5,) sse, sbh, snh, sbv, snv of one plane of the test clip a against the reference b (None: sse = 0).  Integer planes give exact
    int64 sums; float32 planes (the Y of convert_to='y') are subtracted in float32, squared and added in float64."""
    psnrb_counts(a.shape[0], a.shape[1], crop, plane_block)
    y0, y1, x0, x1 = crop, a.shape[0] - crop, crop, a.shape[1] - crop
    exact = np.issubdtype(a.dtype, np.integer)
    wide = np.int64 if exact else np.float64

    def sq(d):
        d = d.astype(wide)
        return d * d

    a = a[y0:y1, x0:x1].astype(np.int64 if exact else np.float32)
    out = np.zeros(5, wide)
    if b is not None:
        out[0] = sq(a - b[y0:y1, x0:x1].astype(a.dtype)).sum()
    dh, dv = sq(a[:, :-1] - a[:, 1:]), sq(a[:-1, :] - a[1:, :])
    bh = (np.arange(x0, x1 - 1) + 1) % plane_block == 0
    bv = (np.arange(y0, y1 - 1) + 1) % plane_block == 0
    out[1], out[2] = dh[:, bh].sum(), dh[:, ~bh].sum()
    out[3], out[4] = dv[bv, :].sum(), dv[~bv, :].sum()
    return out


def psnrb_values(sums, counts, block, dims, peak):
    """The fp64 part.  sums (..., 5) = sse, sbh, snh, sbv, snv of a plane; counts = psnrb_counts of it; block: the PLANE's block size;
    dims = (h, w) of the region; peak P.  -> (PSNR-B, BEF), float64 arrays (...): D_B = (sbh + sbv) / (NBh + NBv), 0 without a boundary
    pair; D_N = (snh + snv) / (NNh + NNv); BEF = log2(block) / log2(min(h, w)) * (D_B - D_N) where D_B > D_N, else 0; PSNR-B = 10 log10(P^2
    / (sse / (h w) + BEF)), inf where the denominator is 0."""
    s = np.asarray(sums).astype(np.float64)
    nbh, nnh, nbv, nnv = (int(x) for x in counts)
    h, w = int(dims[0]), int(dims[1])
    zero = np.zeros(s.shape[:-1], np.float64)
    d_b = (s[..., 1] + s[..., 3]) / float(nbh + nbv) if nbh + nbv else zero
    d_n = (s[..., 2] + s[..., 4]) / float(nnh + nnv) if nnh + nnv else zero
    eta = np.log2(float(block)) / np.log2(float(min(h, w)))
    bef = np.where(d_b > d_n, eta * (d_b - d_n), 0.0)
    den = s[..., 0] / float(h * w) + bef
    with np.errstate(divide='ignore'):
        val = 10.0 * np.log10(float(peak) ** 2 / den)
    return np.where(den == 0, np.inf, val), bef


def _psnrb_planes(img, input_order, convert_to):
    if input_order == 'CHW':
        img = img.transpose(1, 2, 0)
    if _is_y(convert_to, '.'):
        return [bgr2y(img.astype(np.float32) / 255.) * 255.]
    if img.ndim == 2:
        img = img[..., None]
    return [img[..., i] for i in range(img.shape[2])]


def psnrb(img1, img2, crop_border=0, input_order='HWC', convert_to=None, block=8):
    """PSNR-B (Yim and Bovik 2011) of the test image img1 against the reference img2, two uint8 BGR images as psnr() takes them: PSNR
    with the blocking effect factor of img1 added to the mean squared error, the definition of include/pnpvcve.h (pnp_psnrb_*).  It is
    unpinned against any external port; it is checked against the independent pair-by-pair restatement tests/psnrb_ref.py.  The block
    grid is anchored at the uncropped image's origin.  convert_to='y': one plane, the float32 Y of psnr().  Several channels give the
    mean of the channels' values."""
    assert img1.shape == img2.shape, f'Image shapes are different: {img1.shape}, {img2.shape}.'
    bp = psnrb_block(block)
    pa, pb = _psnrb_planes(img1, input_order, convert_to), _psnrb_planes(img2, input_order, convert_to)
    rows, cols = pa[0].shape
    counts = psnrb_counts(rows, cols, crop_border, bp)
    dims = (rows - 2 * crop_border, cols - 2 * crop_border)
    sums = np.stack([psnrb_plane_sums(x, y, crop_border, bp) for x, y in zip(pa, pb)])
    return float(np.mean(psnrb_values(sums, counts, bp, dims, 255.0)[0]))


def bef(img, crop_border=0, input_order='HWC', convert_to=None, block=8):
    """The blocking effect factor of one image alone (the BEF of psnrb(): a no-reference blockiness figure), the mean over its channels"""
    bp = psnrb_block(block)
    pa = _psnrb_planes(img, input_order, convert_to)
    rows, cols = pa[0].shape
    counts = psnrb_counts(rows, cols, crop_border, bp)
    sums = np.stack([psnrb_plane_sums(x, None, crop_border, bp) for x in pa])
    return float(np.mean(psnrb_values(sums, counts, bp, (rows - 2 * crop_border, cols - 2 * crop_border), 255.0)[1]))


ALLOWED_METRICS = {'PSNR': psnr, 'SSIM': ssim, 'MS-SSIM': msssim, 'PSNR-B': psnrb}


# ---------------------------------------------------------------- XPSNR (include/pnpvcve.h, pnp_xpsnr_*: the one statement of the definition)
# A plane metric of 4:2:0 clips: it is not in ALLOWED_METRICS (RGB / Y clips refuse the name as they refuse any unknown one).  The
# functions below are the host path: integer sums from numpy planes (xpsnr_sums), and the fp64 part -- weights, weighted sums, decibels
# -- which ops.xpsnr_yuv420 calls on the device's sums too (xpsnr_weights, xpsnr_values): that part exists once.
XPSNR_K6 = ((0, -1, -1, -1, -1, 0), (-1, -2, -3, -3, -2, -1), (-1, -3, 12, 12, -3, -1),
            (-1, -3, 12, 12, -3, -1), (-1, -2, -3, -3, -2, -1), (0, -1, -1, -1, -1, 0))


def xpsnr_plan(h, w):
    """(N, rows, cols, b) of a cropped h x w luma plane: the block size, the block grid and the border of the activity filters"""
    n = max(4, 4 * int(np.floor(32.0 * np.sqrt(w * h / (3840.0 * 2160.0)) + 0.5)))
    return n, -(-h // n), -(-w // n), (2 if w * h > 2048 * 1152 else 1)


def xpsnr_regions(h, w):
    """the activity regions of every block: (ry0, ry1) of the block rows and (rx0, rx1) of the block columns, int64 arrays"""
    n, rows, cols, b = xpsnr_plan(h, w)

    def axis(size, count):
        lo = np.arange(count, dtype=np.int64) * n
        hi = np.minimum(lo + n, size)
        return np.where(lo > 0, lo, b), np.where(hi < size, hi, size - b)

    return axis(h, rows), axis(w, cols)


def xpsnr_areas(h, w):
    """(rows, cols) int64: area_k, 0 for an empty region"""
    (y0, y1), (x0, x1) = xpsnr_regions(h, w)
    return np.maximum(y1 - y0, 0)[:, None] * np.maximum(x1 - x0, 0)[None, :]


def _xpsnr_block_sums(x, n):
    """(..., h, w) integers -> (..., rows, cols): the sums over the N x N tiles, the last ones clipped at the edge"""
    h, w = x.shape[-2:]
    return np.add.reduceat(np.add.reduceat(x, np.arange(0, h, n), axis=-2), np.arange(0, w, n), axis=-1)


def xpsnr_sums(o, r, fps=30, planes='yuv'):
    """The integer part on the host: o (the original) and r (the test clip) as (y, u, v) triples of (T, rows, cols) integer arrays of
    sample values, already cropped -> (T, rows * cols, 5) int64 = sse_y, sse_u, sse_v, sa, ta of every frame and block, what
    pnp_xpsnr_sums_yuv420 leaves.  Only the planes named in `planes` are compared, the others' sums are 0.  Vectorised: the filters
    run over the whole picture's positions (the union of the regions is the picture without its border), the blocks add them up."""
    oy = np.asarray(o[0]).astype(np.int64)
    t, h, w = oy.shape
    n, rows, cols, b = xpsnr_plan(h, w)
    out = np.zeros((t, rows, cols, 5), np.int64)
    for k, name in enumerate('yuv'):
        if name in planes:
            d = np.asarray(o[k]).astype(np.int64) - np.asarray(r[k]).astype(np.int64)
            out[..., k] = _xpsnr_block_sums(d * d, n if k == 0 else n // 2)
    sa, ta = np.zeros((t, h, w), np.int64), np.zeros((t, h, w), np.int64)
    if h > 2 * b and w > 2 * b:
        if b == 1:
            c = oy[:, 1:-1, 1:-1]
            e = 12 * c - 2 * (oy[:, 1:-1, :-2] + oy[:, 1:-1, 2:] + oy[:, :-2, 1:-1] + oy[:, 2:, 1:-1]) \
                - (oy[:, :-2, :-2] + oy[:, :-2, 2:] + oy[:, 2:, :-2] + oy[:, 2:, 2:])
            sa[:, 1:-1, 1:-1] = np.abs(e)
            s, where = c, (slice(None), slice(1, -1), slice(1, -1))
        else:       # positions: the even rows and columns of [2, h - 2) x [2, w - 2)
            py, px = (h - 4) // 2, (w - 4) // 2
            e = np.zeros((t, py, px), np.int64)
            for q in range(6):
                for c in range(6):
                    if XPSNR_K6[q][c]:
                        e += XPSNR_K6[q][c] * oy[:, q:q + 2 * py:2, c:c + 2 * px:2]
            sa[:, 2:h - 2:2, 2:w - 2:2] = np.abs(e)
            s = oy[:, 2:h - 2:2, 2:w - 2:2] + oy[:, 2:h - 2:2, 3:w - 1:2] + oy[:, 3:h - 1:2, 2:w - 2:2] + oy[:, 3:h - 1:2, 3:w - 1:2]
            where = (slice(None), slice(2, h - 2, 2), slice(2, w - 2, 2))
        d = np.zeros_like(s)
        for i in range(1, t):
            d[i] = s[i] - 2 * s[i - 1] + s[i - 2] if (fps >= 32 and i >= 2) else s[i] - s[i - 1]
        ta[where] = np.abs(d)
    out[..., 3] = _xpsnr_block_sums(sa, n)
    out[..., 4] = _xpsnr_block_sums(ta, n)
    return out.reshape(t, rows * cols, 5)


def xpsnr_weights(sa, ta, area, t, fps, d, h, w):
    """The weights w_k of frame t, fp64: sa, ta, area are (rows, cols) arrays of the frame's block sums and region areas, d the bit
    depth, h x w the cropped luma plane.  act = max((sa + f ta) / area, 2^(d-6)) (the floor for an empty region), a = act^2, the
    minimum smoothing over the existing 8 neighbours, w = A / sqrt(a^)."""
    sa, ta, area = (np.asarray(x, np.float64) for x in (sa, ta, area))
    f = 1.0 if (fps >= 32 and t >= 2) else 2.0
    floor = 2.0 ** (d - 6)
    with np.errstate(divide='ignore', invalid='ignore'):
        act = np.where(area > 0, (sa + f * ta) / area, floor)
    a = np.maximum(act, floor) ** 2
    rows, cols = a.shape
    pad = np.full((rows + 2, cols + 2), np.inf)
    pad[1:-1, 1:-1] = a
    nb = np.full((rows, cols), np.inf)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                nb = np.minimum(nb, pad[dy:dy + rows, dx:dx + cols])
    smoothed = np.where(np.isfinite(nb), np.maximum(a, nb), a)      # (a block with no neighbour keeps a)
    big_a = np.sqrt(16.0 * 2.0 ** (2 * d - 9) * np.sqrt(3840.0 * 2160.0 / (w * h)))
    return big_a / np.sqrt(smoothed)


def xpsnr_values(sums, d, fps, h, w, planes='yuv'):
    """(T, rows * cols, 5) integer sums of a cropped h x w clip of depth d -> (wsse (T, len(planes)), per-frame dB (T, len(planes)), the
    clip's dB (len(planes),)), fp64: wsse_p(t) = sum_k w_k sse_{p,k} added in block index order; XPSNR_p(t) = 10 log10(P^2 H_p W_p /
    wsse_p(t)); the clip's value is the log of the mean, 10 log10(P^2 H_p W_p T / sum_t wsse_p(t)); +inf where the sum is 0."""
    sums = np.asarray(sums)
    n, rows, cols, _ = xpsnr_plan(h, w)
    t = sums.shape[0]
    assert sums.shape == (t, rows * cols, 5), (sums.shape, rows, cols)
    area = xpsnr_areas(h, w)
    wsse = np.zeros((t, len(planes)), np.float64)
    for i in range(t):
        g = sums[i].reshape(rows, cols, 5)
        wk = xpsnr_weights(g[..., 3], g[..., 4], area, i, fps, d, h, w).reshape(-1)
        for j, p in enumerate(planes):
            terms = wk * sums[i, :, 'yuv'.index(p)].astype(np.float64)
            wsse[i, j] = np.cumsum(terms)[-1]                       # sequential: block index order
    peak2 = float((1 << d) - 1) ** 2
    size = np.array([float(h * w) if p == 'y' else float((h // 2) * (w // 2)) for p in planes])
    total = np.cumsum(wsse, axis=0)[-1]
    with np.errstate(divide='ignore'):
        frames = np.where(wsse > 0, 10.0 * np.log10(peak2 * size / wsse), np.inf)
        clip = np.where(total > 0, 10.0 * np.log10(peak2 * size * t / total), np.inf)
    return wsse, frames, clip


def xpsnr(o, r, d, fps=30, crop_border=0):
    """XPSNR of a test clip r against the original o on the host: (y, u, v) triples of (T, rows, cols) integer arrays of sample values
    at bit depth d, the luma cropped by crop_border (even) and the chroma by half of it -> dict(sums (T, blocks, 5) int64, wsse and
    frames (T, 3) fp64 -- the weighted squared error and the dB of every frame, columns Y, U, V --, clip (3,) fp64: the metric).  The
    definition is include/pnpvcve.h's; what ops.xpsnr_yuv420 returns from the device's sums goes through the same xpsnr_values."""
    if crop_border < 0 or crop_border % 2:
        raise ValueError(f'crop_border must be even and >= 0 (the chroma planes are cropped by half of it), got {crop_border}')
    if d not in (8, 10, 12) or int(fps) != fps or fps < 1:
        raise ValueError(f'XPSNR takes a bit depth of 8, 10 or 12 and an integer fps >= 1, got {d} and {fps}')

    def cut(planes):
        out = []
        for k, p in enumerate(planes):
            c = crop_border if k == 0 else crop_border // 2
            p = np.asarray(p)
            out.append(p[:, c:p.shape[1] - c, c:p.shape[2] - c])
        return out

    o, r = cut(o), cut(r)
    t, h, w = o[0].shape
    if h < 2 or w < 2 or h % 2 or w % 2 or any(x.shape != (t, h // 2, w // 2) for x in o[1:]) or [x.shape for x in o] != [x.shape for x in r]:
        raise ValueError(f'XPSNR compares two 4:2:0 clips of one even size, got {[x.shape for x in o]} and {[x.shape for x in r]}')
    sums = xpsnr_sums(o, r, fps)
    wsse, frames, clip = xpsnr_values(sums, d, fps, h, w)
    return dict(sums=sums, wsse=wsse, frames=frames, clip=clip)


# ---------------------------------------------------------------- enhancement gain (include/pnpvcve.h, pnp_gain_*: the one statement of the definition)
# What the test clip a gained over the compressed input l, both against the original g.  The host path: the two squared-error sums of
# every gain cell by reshaping (gain_sums), a cell's sample count in closed form (gain_cell_counts), and the fp64 part (gain_values,
# gain_sd, gain_yuv, gain_report), which ops.gain_* and BasicVSR.evaluate call on the device's sums too: that part exists once.
GAIN_BLOCKS = (16, 32, 64, 128)
GAIN_METRICS = ('PSNR_LQ', 'SSIM_LQ', 'dPSNR', 'dSSIM', 'PSNR_SD', 'PSNR_SD_LQ')                   # served on every boundary
GAIN_PLANE_METRICS = ('dPSNR_U', 'dPSNR_V', 'PSNR_LQ_U', 'PSNR_LQ_V', 'dSSIM_U', 'dSSIM_V', 'SSIM_LQ_U', 'SSIM_LQ_V', 'dPSNR_YUV')      # clips of planes only
GAIN_FACTORS = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}      # chroma format -> (sx, sy)


def gain_block(block):
    """the gain block: one of GAIN_BLOCKS luma samples (64: the CTU of HEVC; 128: VVC's)"""
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in GAIN_BLOCKS:
        raise ValueError(f'block must be one of {GAIN_BLOCKS}, got {block!r}')
    return int(block)


def gain_grid(h, w, block=64):
    """(rows, cols) of the cell grid of h x w frames: anchored at the uncropped frame's origin, the same for every plane"""
    b = gain_block(block)
    if h < 1 or w < 1:
        raise ValueError(f'frames of {h} x {w}')
    return -(-int(h) // b), -(-int(w) // b)


def _gain_plane(h, w, crop, block, sx, sy):
    """-> (rows, cols, crop down, crop across, cell rows, cell columns) of the plane of h x w frames that (sx, sy) subsample"""
    b = gain_block(block)
    if isinstance(crop, bool) or int(crop) != crop or crop < 0 or 2 * crop >= h or 2 * crop >= w:
        raise ValueError(f'a crop of {crop!r} leaves nothing of {h} x {w} frames (or is no integer >= 0)')
    if h % sy or w % sx:
        raise ValueError(f'{h} x {w} frames cannot be subsampled by {sx} across and {sy} down')
    return h // sy, w // sx, int(crop) // sy, int(crop) // sx, b // sy, b // sx


def gain_cell_counts(h, w, crop_border=0, block=64, sx=1, sy=1):
    """(rows, cols) int64: the samples of every cell inside the region, in closed form -- the overlap of [i bh, (i + 1) bh) with
    [cy, rows - cy) times the overlap of [j bw, (j + 1) bw) with [cx, cols - cx); a cell inside the crop has 0"""
    rows, cols, cy, cx, bh, bw = _gain_plane(h, w, crop_border, block, sx, sy)
    gr, gc = gain_grid(h, w, block)

    def overlap(count, b, lo, hi):
        k = np.arange(count, dtype=np.int64)
        return np.maximum(np.minimum((k + 1) * b, hi) - np.maximum(k * b, lo), 0)

    return overlap(gr, bh, cy, rows - cy)[:, None] * overlap(gc, bw, cx, cols - cx)[None, :]


def _gain_cells(e, cy, cx, bh, bw, gr, gc):
    """(T, rows, cols) per-sample errors -> (T, gr, gc): zeros outside the region, the plane padded to whole cells, one reshape"""
    t, rows, cols = e.shape
    pad = np.zeros((t, gr * bh, gc * bw), e.dtype)
    pad[:, cy:rows - cy, cx:cols - cx] = e[:, cy:rows - cy, cx:cols - cx]
    return pad.reshape(t, gr, bh, gc, bw).sum(axis=(2, 4))


def _gain_errors(x, g):
    """per-sample squared error of two (T, rows, cols[, C]) arrays, a pixel's channels added: integers exactly (int64); float32 samples
    (the Y of convert_to='y') as one float32 subtraction squared in float64"""
    x, g = np.asarray(x), np.asarray(g)
    if x.shape != g.shape or x.ndim not in (3, 4):
        raise ValueError(f'clips of different shapes: {x.shape} and {g.shape}')
    if x.dtype == np.float32 and g.dtype == np.float32:
        d = (x - g).astype(np.float64)
    elif np.issubdtype(x.dtype, np.integer) and np.issubdtype(g.dtype, np.integer):
        d = x.astype(np.int64) - g.astype(np.int64)
    else:
        raise TypeError(f'samples must be integers, or float32 luma on both sides: got {x.dtype} and {g.dtype}')
    e = d * d
    return e.sum(axis=-1) if e.ndim == 4 else e


def gain_classes(par):
    """(T, 3, h, w) partition map -> (T, h, w) int64 classes: (par0 != 0) | (par1 != 0) << 1 | (par2 != 0) << 2"""
    par = np.asarray(par)
    if par.ndim != 4 or par.shape[1] != 3:
        raise ValueError(f'par must be (frames, 3, h, w), got {par.shape}')
    nz = (par != 0).astype(np.int64)
    return nz[:, 0] | (nz[:, 1] << 1) | (nz[:, 2] << 2)


def gain_sums(a, l, g, crop_border=0, block=64, fmt=None, par=None):
    """The sums of the enhancement gain on the host (include/pnpvcve.h).  a (the test clip), l (the compressed input), g (the original):
    three (y, u, v) triples of (T, rows, cols) integer arrays of a clip of planes in the chroma format fmt ('420' | '422' | '444'); or
    three (T, h, w, C) integer arrays of pixels (the channels of a pixel are added); or three (T, h, w) float32 luma arrays.  ->
    (grid (T, planes, rows, cols, 2) = E_a, E_l of every cell, int64 -- float64 for float32 samples --, classes (T, 8, 3) = N, E_a, E_l
    of every partition class on the Y plane / the pixels, or None without par (T, 3, h, w))."""
    if isinstance(a, (tuple, list)):
        if fmt not in GAIN_FACTORS:
            raise ValueError(f'a clip of planes needs its chroma format, one of {sorted(GAIN_FACTORS)}: got {fmt!r}')
        planes = [(a[k], l[k], g[k], (1, 1) if k == 0 else GAIN_FACTORS[fmt]) for k in range(3)]
    else:
        planes = [(a, l, g, (1, 1))]
    t, h, w = np.asarray(planes[0][0]).shape[:3]
    gr, gc = gain_grid(h, w, block)
    grid, classes = None, None
    for k, (pa, pl, pg, (sx, sy)) in enumerate(planes):
        rows, cols, cy, cx, bh, bw = _gain_plane(h, w, crop_border, block, sx, sy)
        ea, el = _gain_errors(pa, pg), _gain_errors(pl, pg)
        if ea.shape != (t, rows, cols) or el.shape != (t, rows, cols):
            raise ValueError(f'plane {k} must be {(t, rows, cols)}, got {ea.shape} and {el.shape}')
        if grid is None:
            grid = np.zeros((t, len(planes), gr, gc, 2), ea.dtype)
        grid[:, k, :, :, 0] = _gain_cells(ea, cy, cx, bh, bw, gr, gc)
        grid[:, k, :, :, 1] = _gain_cells(el, cy, cx, bh, bw, gr, gc)
        if k == 0 and par is not None:
            cls = gain_classes(par)
            if cls.shape != (t, h, w):
                raise ValueError(f'par must be {(t, 3, h, w)}, got {np.asarray(par).shape}')
            region = (slice(None), slice(cy, rows - cy), slice(cx, cols - cx))
            classes = np.zeros((t, 8, 3), ea.dtype)
            for c in range(8):
                m = cls[region] == c
                classes[:, c, 0] = m.sum(axis=(1, 2))
                classes[:, c, 1] = (ea[region] * m).sum(axis=(1, 2))
                classes[:, c, 2] = (el[region] * m).sum(axis=(1, 2))
    return grid, classes


def gain_frame_sums(grid):
    """grid (..., rows, cols, 2) -> (..., 2): a frame's E_a, E_l, its cells added in index order (row by row) -- ONE order for every
    caller, so the fp64 sums of convert_to='y' give the same bits wherever they are formed; integers are exact in any order"""
    g = np.asarray(grid)
    return g.reshape(g.shape[:-3] + (-1, 2)).cumsum(axis=-2)[..., -1, :]


def gain_values(e_a, e_l, n, peak=255.0):
    """The fp64 part.  e_a, e_l: arrays (...) of squared-error sums over n samples each (n: a number or an array that broadcasts), peak
    P -> (PSNR of a, PSNR of l, dPSNR), float64 arrays (...): PSNR(x) = 10 log10(P^2 n / E_x), +inf for E = 0; dPSNR = 10 log10(E_l /
    E_a), 0 for 0 / 0, +inf for E_a = 0 < E_l, -inf for E_l = 0 < E_a."""
    ea, el = np.asarray(e_a, np.float64), np.asarray(e_l, np.float64)
    n = np.asarray(n, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        pa = np.where(ea > 0, 10.0 * np.log10(float(peak) ** 2 * n / ea), np.inf)
        pl = np.where(el > 0, 10.0 * np.log10(float(peak) ** 2 * n / el), np.inf)
        d = np.where(ea > 0, np.where(el > 0, 10.0 * np.log10(el / ea), -np.inf), np.where(el > 0, np.inf, 0.0))
    return pa, pl, d


def gain_sd(per_frame):
    """the quality fluctuation of a clip: the population standard deviation (ddof 0) of the frames' values, fp64"""
    x = np.asarray(per_frame, np.float64).reshape(-1)
    return float(np.sqrt(np.mean((x - np.mean(x)) ** 2)))


def gain_yuv(dy, du, dv):
    """(6 dY + dU + dV) / 8 per frame, the weights of PSNR_YUV"""
    return (6.0 * np.asarray(dy, np.float64) + np.asarray(du, np.float64) + np.asarray(dv, np.float64)) / 8.0


def _gain_json(x):
    x = float(x)
    return x if np.isfinite(x) else ('inf' if x > 0 else ('-inf' if x < 0 else 'nan'))


def gain_report(grid, counts, peak=255.0, slices=None, qps=None, base_qps=None, classes=None, class_samples=1, ssim=None, ssim_lq=None, block=64):
    """One clip's gain as a JSON-ready dict.  grid (T, rows, cols, 2): the cells' E_a, E_l of the Y plane / the pixels; counts (rows,
    cols): the cells' samples (gain_cell_counts, times 3 for RGB sums); slices (T) letters or their codes ord('I' | 'P' | 'B'), qps and
    base_qps (T) numbers or None; classes (T, 8, 3) or None, class_samples the samples a pixel stands for (3 for RGB sums); ssim,
    ssim_lq (T) the SSIM of a and of l per frame or None.  ->
      frames:   per frame index, slice, qp, base_qp, PSNR, PSNR_LQ, dPSNR (and SSIM, SSIM_LQ, dSSIM);
      by_slice / by_qp: the means of those values over the frames of a slice type / a QP, with the number of frames;
      classes:  per partition class, summed over the clip: N, PSNR, PSNR_LQ, dPSNR (None without a partition map);
      grid:     dPSNR of every cell, frames summed, as nested lists (0 for a cell inside the crop);
      dPSNR:    the clip's value, the mean over frames.
    Infinite values are written as the strings 'inf' / '-inf' (JSON has no infinity)."""
    grid = np.asarray(grid)
    t = grid.shape[0]
    n = float(np.asarray(counts, np.float64).sum())
    e = gain_frame_sums(grid)
    pa, pl, dp = gain_values(e[:, 0], e[:, 1], n, peak)

    def letter(s):
        return s if isinstance(s, str) else chr(int(round(float(s))))

    sl = [None] * t if slices is None else [letter(s) for s in np.asarray(slices).reshape(-1)[:t].tolist()]
    qp = [None] * t if qps is None else [float(q) for q in np.asarray(qps, np.float64).reshape(-1)[:t]]
    bq = [None] * t if base_qps is None else [float(q) for q in np.asarray(base_qps, np.float64).reshape(-1)[:t]]
    cols = dict(PSNR=pa, PSNR_LQ=pl, dPSNR=dp)
    if ssim is not None and ssim_lq is not None:
        sa, sq = np.asarray(ssim, np.float64).reshape(-1), np.asarray(ssim_lq, np.float64).reshape(-1)
        cols.update(SSIM=sa, SSIM_LQ=sq, dSSIM=sa - sq)
    frames = [dict(index=i, slice=sl[i], qp=qp[i], base_qp=bq[i], **{k: _gain_json(v[i]) for k, v in cols.items()}) for i in range(t)]

    def groups(keys):
        out = {}
        for key in dict.fromkeys(k for k in keys if k is not None):
            idx = [i for i in range(t) if keys[i] == key]
            with np.errstate(invalid='ignore'):
                out[str(key) if isinstance(key, str) else repr(key)] = dict(frames=len(idx), **{k: _gain_json(np.mean(v[idx])) for k, v in cols.items()})
        return out

    table = None
    if classes is not None:
        c = np.asarray(classes).sum(axis=0)
        ca, cl, cd = gain_values(c[:, 1], c[:, 2], c[:, 0].astype(np.float64) * class_samples, peak)
        table = [dict(**{'class': k}, N=int(c[k, 0]), PSNR=_gain_json(ca[k]), PSNR_LQ=_gain_json(cl[k]), dPSNR=_gain_json(cd[k])) for k in range(8)]
    cells = gain_values(grid[..., 0].sum(axis=0), grid[..., 1].sum(axis=0), 1.0, peak)[2]
    with np.errstate(invalid='ignore'):
        return dict(block=int(block), frames=frames, by_slice=groups(sl), by_qp=groups(qp), classes=table,
                    grid=[[_gain_json(v) for v in row] for row in cells], dPSNR=_gain_json(np.mean(dp)))
