"""GPU: one clip source and one pair of group loaders (csrc/metric_src.h: ClipSrc, plane_load4, f32_load4; csrc/plane_src.h: clip_planes)
behind every device metric.  The same samples go through every entry that forms a squared error -- plane PSNR, PSNR-B, the enhancement
gain and XPSNR on Y'CbCr planes; PSNR-B and the gain on RGB frames -- in the layouts, pitches and base addresses where a loader can go
wrong (a short last group, cropped rows that start at an odd column, planes too small for a dword fetch at their end, an interleaved
pair in either order, high-aligned 16-bit words).  The sums are exact integers: they must be equal to each other and to numpy's int64
SSE, with no tolerance."""
import numpy as np
import pytest
import torch

import test_gpu_yuv16_frames as y16
import test_gpu_yuv_frames as yf
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
T = 2
# (h, w, crop): chroma planes of 27 x 35 (an odd width, a last group of three); chroma of 33 x 39 cropped by 1, so cropped rows start at
# column 1; one group a chroma row, so no group of the plane's end qualifies for the dword path
SHAPES = [(54, 70, 0), (66, 78, 2), (16, 16, 0)]
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def plane_pair(h, w, depth):
    """the Y, Cb, Cr sample values of two clips (CPU int32), the second the first plus noise of +-9: drawn once per shape and depth"""
    if (h, w, depth) not in _CACHE:
        g = torch.Generator().manual_seed(7100 + 100 * h + w + depth)
        top = (1 << depth) - 1
        a = [torch.randint(0, top + 1, (T, hh, ww), generator=g, dtype=torch.int32) for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        b = [(x + torch.randint(-9, 10, x.shape, generator=g, dtype=torch.int32)).clamp(0, top) for x in a]
        _CACHE[(h, w, depth)] = (a, b)
    return _CACHE[(h, w, depth)]


def numpy_sse(a, b, crop):
    """(T, 3) int64: the SSE of the planes, Y cropped by crop, chroma by crop / 2"""
    out = np.zeros((T, 3), np.int64)
    for k, (p, q) in enumerate(zip(a, b)):
        c = crop if k == 0 else crop // 2
        d = (p.numpy().astype(np.int64) - q.numpy().astype(np.int64))[:, c:p.shape[1] - c, c:p.shape[2] - c]
        out[:, k] = (d * d).sum(axis=(1, 2))
    return out


def layout_pairs(h, w):
    """(name, depth, the test clip's planes, the reference's): the constructors of the two containers"""
    yield 'nv12 off 1 pitch w+7 / i420', 8, lambda: yf.Planes(T, h, w, 'nv12', pitch=w + 7, off=1), lambda: yf.Planes(T, h, w, 'i420')
    yield 'nv12 off 3 pitch w+7 / i420', 8, lambda: yf.Planes(T, h, w, 'nv12', pitch=w + 7, off=3), lambda: yf.Planes(T, h, w, 'i420')
    yield 'nv21 / nv12', 8, lambda: yf.Planes(T, h, w, 'nv21'), lambda: yf.Planes(T, h, w, 'nv12')
    yield 'p010 pitch 2w+6 off 6 / yuv420p10le', 10, (lambda: y16.Planes16(T, h, w, 'nv12', 10, True, pitch=2 * w + 6, off=6)), \
        lambda: y16.Planes16(T, h, w, 'i420', 10, False)


@pytest.mark.parametrize('h,w,crop', SHAPES, ids=lambda v: str(v))
def test_every_plane_entry_forms_numpys_squared_error(h, w, crop):
    for name, depth, make_a, make_b in layout_pairs(h, w):
        a, b = plane_pair(h, w, depth)
        want = numpy_sse(a, b, crop)
        conv = (lambda p: [x.to(torch.uint8) for x in p]) if depth == 8 else (lambda p: p)
        va, vb = make_a().fill(*conv(a)).views, make_b().fill(*conv(b)).views
        got = {'psnr_sse_yuv': ops.psnr_sse_yuv(va, vb, crop).numpy(),
               'psnrb_sums_yuv420': ops.psnrb_sums_yuv420(va, vb, crop, 'yuv')[..., 0].numpy(),
               'xpsnr_sums_yuv420': ops.xpsnr_sums_yuv420(va, vb, crop, 'yuv')[..., :3].sum(dim=-2).numpy()}
        grid = ops.gain_sums_yuv(va, va, vb, crop, 'yuv', block=16)[0].numpy()           # lead + (3, rows, cols, 2)
        got['gain_sums_yuv E_a'], got['gain_sums_yuv E_l'] = grid[..., 0].sum(axis=(-2, -1)), grid[..., 1].sum(axis=(-2, -1))
        print(f'{(h, w, crop)} {name}: SSE of frame 0 {want[0].tolist()}')
        assert want.min() > 0
        for entry, v in got.items():
            assert v.dtype == np.int64 and v.shape == (T, 3), (name, entry, v.dtype, v.shape)
            assert np.array_equal(v, want), (name, entry, v.tolist(), want.tolist())


def byte_view(x, off):
    """the bytes of x in a device allocation of their own, `off` bytes from its start"""
    flat = torch.full((x.numel() + 8,), 0xA5, dtype=torch.uint8, device=dev())
    v = flat[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    return v


@pytest.mark.parametrize('h,w,crop', [(66, 79, 0), (66, 79, 3)], ids=lambda v: str(v))
def test_every_frame_entry_forms_numpys_squared_error(h, w, crop):
    g = torch.Generator().manual_seed(7300 + crop)
    a = torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)
    b = (a.int() + torch.randint(-9, 10, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    d = (a.numpy().astype(np.int64) - b.numpy().astype(np.int64))[:, crop:h - crop, crop:w - crop]
    want = (d * d).sum(axis=(1, 2, 3))
    assert want.min() > 0
    a1, b3 = byte_view(a, 1), byte_view(b, 3)
    fa, fb = ops.frames_from_rgb8(a1), ops.frames_from_rgb8(b3)     # (T,3,h,w) fp32 planes, byte / 255
    for name, x, y in (('u8 off 1 / u8 off 3', a1, b3), ('u8 / f32', a1, fb), ('f32 / f32', fa, fb)):
        pb = ops.psnrb_sums_frames(x, y, crop)[..., 0].sum(dim=-1).numpy()
        ga = ops.gain_sums_frames(x, x, y, crop, block=16)[0][..., 0].sum(dim=(-3, -2, -1)).numpy()
        print(f'{(h, w, crop)} {name}: SSE {want.tolist()}')
        for entry, v in (('psnrb_sums_frames', pb), ('gain_sums_frames', ga)):
            assert v.dtype == np.int64 and np.array_equal(v, want), (name, entry, v.tolist(), want.tolist())
