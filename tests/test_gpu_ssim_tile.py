"""GPU: one SSIM tile body (csrc/ssim_tile.h) behind every SSIM entry.  The same byte samples go through pnp_ssim_partials_f32, every
format pair of pnp_ssim_partials_io and the plane loader of pnp_ssim_partials_yuv (a 4:4:4 clip whose Y plane holds one channel's bytes;
at the 4:2:0 shape the Cb and Cr planes too, NV12 and I420) at the shapes where the tile logic can go wrong, and the raw partials must
be the same bits.  The sums are held to the host restatement (metrics.ssim) at the 1e-10 of tests/test_gpu_metrics_io.py; the 16-bit
sample path, at depth 10, to the float64 definition with L = 1023 (tests/yuv16_ref.ssim_plane) at the 1e-10 of
tests/test_gpu_yuv16_metrics.py."""
import ctypes

import numpy as np
import pytest
import torch

import yuv16_ref
from pnp_vcve_amd import _native, metrics, ops

pytestmark = pytest.mark.gpu
T = 2
# (h, w, crop): a 1 x 1 valid map; exactly one full tile; four tiles with 1-wide remainders; the one full tile behind a crop; two tiles
# across, whose 4:2:0 chroma planes are 22 x 43 (one tile, odd width, the plane loader's short last group)
SHAPES = [(11, 11, 0), (26, 42, 0), (27, 43, 0), (34, 50, 4), (44, 86, 2)]
SHAPES16 = [(27, 43, 0), (44, 86, 2)]
F32, U8, NONE = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC, _native.COLOR_NONE
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def byte_pair(h, w):
    """two byte clips (T,h,w,3) on the host, the second the first plus small noise: drawn once per shape"""
    if (h, w) not in _CACHE:
        g = torch.Generator().manual_seed(4200 + 100 * h + w)
        a = torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)
        b = (a.int() + torch.randint(-9, 10, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
        _CACHE[(h, w)] = (a, b)
    return _CACHE[(h, w)]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def partials_f32(pa, pb, crop):
    """pnp_ssim_partials_f32 of (T,c,h,w) fp32 planes -> (T, c, blocks)"""
    L = _native.lib()
    c, h, w = pa.shape[1:]
    nb = int(L.pnp_ssim_blocks(h, w, crop))
    out = torch.full((T, c, nb), float('nan'), dtype=torch.float64, device=dev())
    assert L.pnp_ssim_partials_f32(_vp(pa), _vp(pb), _vp(out), T, c, h, w, crop, _stream()) == 0
    return out


def partials_io(x, y, h, w, crop):
    L = _native.lib()
    nb = int(L.pnp_ssim_blocks(h, w, crop))
    out = torch.full((T, 3, nb), float('nan'), dtype=torch.float64, device=dev())
    fx, fy = (U8 if t.dtype == torch.uint8 else F32 for t in (x, y))
    assert L.pnp_ssim_partials_io(_vp(x), fx, _vp(y), fy, NONE, _vp(out), T, 3, h, w, crop, _stream()) == 0
    return out


def partials_yuv(a, b, plane, h, w, crop):
    """pnp_ssim_partials_yuv of one plane (a PNP_PLANE_* bit) of two 8-bit clips -> (T, blocks)"""
    L = _native.lib()
    fmt = _native.YUV_FORMAT[ops.yuv_format(a)]
    nb = int(L.pnp_ssim_blocks_yuv(h, w, crop, plane, fmt))
    assert nb >= 1
    out = torch.full((T, nb), float('nan'), dtype=torch.float64, device=dev())
    da, db = ops._yuv_clip_desc(a)[0], ops._yuv_clip_desc(b)[0]
    assert L.pnp_ssim_partials_yuv(ctypes.byref(da), ctypes.byref(db), plane, _vp(out), T, h, w, crop, fmt, _stream()) == 0
    return out


def f32_plane(p):
    """(T, rows, cols) bytes on the device -> (T, 1, rows, cols) fp32, byte / 255 through the table of frames_from_rgb8"""
    return ops.frames_from_rgb8(p[..., None].expand(p.shape + (3,)).contiguous())[:, :1].contiguous()


def yuv420_clip(y, cb, cr, layout):
    """device byte planes -> Yuv420Frames of a packed buffer in `layout`"""
    h, w = y.shape[-2:]
    v = ops.yuv420_views(torch.zeros((T, h * 3 // 2, w), dtype=torch.uint8, device=dev()), h, w, layout)
    for dst, src in zip(v, (y, cb, cr)):
        dst.copy_(src)
    return v


@pytest.mark.parametrize('h,w,crop', SHAPES, ids=lambda v: str(v))
def test_every_8_bit_ssim_entry_gives_the_same_partials(h, w, crop):
    a, b = (x.to(dev()) for x in byte_pair(h, w))
    pa, pb = ops.frames_from_rgb8(a), ops.frames_from_rgb8(b)
    ref = partials_f32(pa, pb, crop)
    assert not bool(torch.isnan(ref).any())
    for x, y in ((a, b), (a, pb), (pa, b)):
        assert torch.equal(partials_io(x, y, h, w, crop), ref), (x.dtype, y.dtype)
    for ch in range(3):                                             # a channel's bytes as the Y plane of a 4:4:4 clip
        ya, yb = a[..., ch].contiguous(), b[..., ch].contiguous()
        one = partials_f32(f32_plane(ya), f32_plane(yb), crop)[:, 0]
        assert torch.equal(one, ref[:, ch]), ch
        got = partials_yuv(ops.Yuv444Frames(ya, ya, ya), ops.Yuv444Frames(yb, yb, yb), _native.PLANE_Y, h, w, crop)
        assert torch.equal(got, one), ch
    if h % 2 == 0 and w % 2 == 0:                                   # the chroma planes of a 4:2:0 clip: channels 0 and 1, cut to h/2 x w/2
        ca, cb_ = [a[:, :h // 2, :w // 2, k].contiguous() for k in (0, 1)], [b[:, :h // 2, :w // 2, k].contiguous() for k in (0, 1)]
        want = [partials_f32(f32_plane(p), f32_plane(q), crop // 2)[:, 0] for p, q in zip(ca, cb_)]
        for la, lb in (('nv12', 'i420'), ('i420', 'nv12')):
            va, vb = yuv420_clip(a[..., 2], *ca, la), yuv420_clip(b[..., 2], *cb_, lb)
            for k, plane in enumerate((_native.PLANE_CB, _native.PLANE_CR)):
                assert torch.equal(partials_yuv(va, vb, plane, h, w, crop), want[k]), (la, lb, k)
    # the sums against the host restatement
    n = (h - 2 * crop - 10) * (w - 2 * crop - 10)
    got = (ref.sum(dim=2) / n).cpu().numpy()
    host = np.array([[metrics.ssim(a[i, ..., ch].cpu().numpy(), b[i, ..., ch].cpu().numpy(), crop) for ch in range(3)] for i in range(T)])
    err = float(np.abs(got - host).max())
    print(f'SSIM {(h, w, crop)}: device vs host restatement {err:.3e}; values {got.min():.4f} .. {got.max():.4f}')
    assert err <= 1e-10, err
    assert 0.0 < got.min() and got.max() < 1.0


def clip16(v, h, w):
    """(T,h,w,3) 10-bit values -> (the planes they make, the clip of those planes on the device): odd sizes a 4:4:4 clip, a channel a
    plane; even sizes a 4:2:0 clip, channel 2 its Y plane, channels 0 and 1 cut to h/2 x w/2 its chroma planes"""
    if h % 2 or w % 2:
        planes, cls = [v[..., k] for k in range(3)], ops.Yuv444Frames16
    else:
        planes, cls = [v[..., 2], v[:, :h // 2, :w // 2, 0], v[:, :h // 2, :w // 2, 1]], ops.Yuv420Frames16
    return planes, cls(*[p.to(torch.int16).contiguous().to(dev()) for p in planes], 10, False)


@pytest.mark.parametrize('h,w,crop', SHAPES16, ids=lambda v: str(v))
def test_the_16_bit_sample_path_is_the_float64_definition_at_depth_10(h, w, crop):
    a, b = byte_pair(h, w)
    va = a.int() * 4 + 1                                            # 10-bit values
    vb = (va + (b.int() - a.int())).clamp(0, 1023)
    (pa, ca), (pb, cb) = clip16(va, h, w), clip16(vb, h, w)
    got = ops.ssim_yuv(ca, cb, crop, 'yuv').numpy()

    def cut(p):                                                     # a plane of rows h / sy is cropped by crop / sy, likewise across
        cy, cx = crop * p.shape[1] // h, crop * p.shape[2] // w
        return p[:, cy:p.shape[1] - cy, cx:p.shape[2] - cx].numpy()

    want = np.array([[yuv16_ref.ssim_plane(cut(p)[i], cut(q)[i], 10) for p, q in zip(pa, pb)] for i in range(T)])
    err = float(np.abs(got - want).max())
    print(f'16-bit SSIM {(h, w, crop)}: device vs float64 definition {err:.3e}')
    assert got.shape == (T, 3) and err < 1e-10, err
    assert 0.0 < got.min() and got.max() < 1.0
