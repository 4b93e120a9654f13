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
