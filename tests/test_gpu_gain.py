"""GPU: the enhancement gain (include/pnpvcve.h, pnp_gain_*; csrc/gain.hip).  The grid of the cells' two squared-error sums and the
partition-class sums are held to the independent restatement tests/gain_ref.py: torch.equal on every boundary that scores integers
(8-bit planes of the three chroma formats in every layout, 10 / 12-bit words low- and high-aligned, RGB frames fp32 or uint8), 1e-12
relative -- the project's bound for two fp64 summations of the same terms -- and bit-equal between two runs for the fp32 Y.  Then
against code that exists (ops.psnr_sse_yuv, pnp_psnr_stat_io), canaries around the outputs, single differences on every seam, and the
names through BasicVSR.evaluate, multi_gpu_test and tools/test.py --gain-report."""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gain_ref as ref
import test_gpu_yuv16_frames as y16
import test_gpu_yuv_formats as tf
import test_gpu_yuv_frames as yf
import test_gpu_yuv_metrics as m8
from pnp_vcve_amd import _native, metrics, ops

pytestmark = pytest.mark.gpu
dev = yf.dev
T = 3
SIZES = [(64, 80), (66, 78), (130, 70)]
BLOCKS = (16, 64)
CROPS = (0, 2, 6)
_CACHE = {}


def rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def close(x, y):
    """two float64 tensors of finite dB values, one formula evaluated twice: 1e-12 relative"""
    return x.shape == y.shape and x.dtype == y.dtype == torch.float64 and float(((x - y).abs() / y.abs()).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ clips and their references, made once
def plane_values(h, w, fmt, depth):
    """(a, l, g): three (y, u, v) triples of (T, rows, cols) int32 arrays; a and l differ from g by a codec's errors, never by none"""
    key = ('values', h, w, fmt, depth)
    if key not in _CACHE:
        rng = np.random.RandomState(h * 7 + w + depth)
        sx, sy = ref.FORMATS[fmt]
        top = (1 << depth) - 1
        g = tuple(rng.randint(0, top + 1, (T, hh, ww)).astype(np.int32) for hh, ww in ((h, w), (h // sy, w // sx), (h // sy, w // sx)))
        near = lambda s: tuple(np.clip(p + rng.randint(-s, s + 1, p.shape), 0, top).astype(np.int32) for p in g)      # noqa: E731
        _CACHE[key] = (near(9 << (depth - 8)), near(14 << (depth - 8)), g)
    return _CACHE[key]


def plane_ref(h, w, fmt, depth, crop, block):
    key = ('ref', h, w, fmt, depth, crop, block)
    if key not in _CACHE:
        a, l, g = plane_values(h, w, fmt, depth)
        _CACHE[key] = torch.from_numpy(ref.gain_grid(a, l, g, crop, block, fmt))
        assert int(_CACHE[key].sum(dim=(1, 2, 3)).min()) > 0            # every frame has an E_a and an E_l
    return _CACHE[key]


def par_map(h, w):
    """(T, 3, h, w) fp32 whose planes overlap, values other than 1 among them"""
    key = ('par', h, w)
    if key not in _CACHE:
        rng = np.random.RandomState(h + w)
        par = np.zeros((T, 3, h, w), np.float32)
        for f in range(T):
            for c in range(3):
                for _ in range(6):
                    y, x = rng.randint(0, h - 8), rng.randint(0, w - 8)
                    par[f, c, y:y + rng.randint(4, 40), x:x + rng.randint(4, 40)] = rng.choice([1.0, 0.5, -2.0])
        _CACHE[key] = par
    return _CACHE[key]


def tt(vals):
    return [torch.from_numpy(np.ascontiguousarray(v)) for v in vals]


def clips8(h, w, fmt):
    """the three clips of 8-bit values, each in a layout of its own: a at an odd address and pitch, l interleaved the other way round or
    planar, g tight"""
    a, l, g = plane_values(h, w, fmt, 8)
    if fmt == '420':
        return (yf.Planes(T, h, w, 'nv12', w + 7, 1).fill(*[x.to(torch.uint8) for x in tt(a)]),
                yf.Planes(T, h, w, 'i420', w + 6, 3, w // 2 + 3).fill(*[x.to(torch.uint8) for x in tt(l)]),
                yf.Planes(T, h, w, 'nv21').fill(*[x.to(torch.uint8) for x in tt(g)]))
    names = {'422': ('nv16', 'yuv422p', 'nv16-crfirst'), '444': ('yuv444p', 'nv24', 'yuv444p')}[fmt]
    ca, cl, cg = (tf.BY_NAME[n] for n in names)
    return tf.planes_of(ca, T, h, w, True).fill(*tt(a)), tf.planes_of(cl, T, h, w, off=3).fill(*tt(l)), tf.planes_of(cg, T, h, w).fill(*tt(g))


def clips16(h, w, fmt, depth):
    """10 / 12-bit clips: low- and high-aligned words, interleaved and planar, an even address that is not 8-byte aligned"""
    a, l, g = plane_values(h, w, fmt, depth)
    if fmt == '420':
        return (y16.Planes16(T, h, w, 'nv12', depth, True, 2 * w + 6, 2).fill(*tt(a)), y16.Planes16(T, h, w, 'i420', depth, False).fill(*tt(l)),
                y16.Planes16(T, h, w, 'nv21', depth, False, 2 * w + 2, 6).fill(*tt(g)))
    lay = {('422', 10): ('p210', 'yuv422p10le'), ('422', 12): ('yuv422p12le', 'p212'), ('444', 10): ('p410', 'yuv444p10le')}[(fmt, depth)]
    cont = dict(tf.BY_NAME, yuv422p10le=('yuv422p10le', '422', 'i420', 10, False, 'bt601-limited'), p212=('p212', '422', 'nv12', 12, True, 'bt601-limited'))
    ca, cl = cont[lay[0]], cont[lay[1]]
    return tf.planes_of(ca, T, h, w, True).fill(*tt(a)), tf.planes_of(cl, T, h, w).fill(*tt(l)), tf.planes_of(ca, T, h, w, off=1).fill(*tt(g))


def unchanged(planes, values):
    return torch.equal(planes.flat.cpu(), planes.expect(*tt(values)) if not isinstance(planes, yf.Planes) else planes.expect(*[x.to(torch.uint8) for x in tt(values)]))


# ------------------------------------------------------------------------------------------------ planes against the restatement
@pytest.mark.parametrize('fmt', ['420', '422', '444'])
@pytest.mark.parametrize('h,w', SIZES)
def test_8_bit_planes_in_three_layouts_are_the_restatement(h, w, fmt):
    pa, pl, pg = clips8(h, w, fmt)
    par = torch.from_numpy(par_map(h, w)).to(dev())
    a, l, g = plane_values(h, w, fmt, 8)
    for block in BLOCKS:
        for crop in CROPS:
            want = plane_ref(h, w, fmt, 8, crop, block)
            got, classes = ops.gain_sums_yuv(pa.views, pl.views, pg.views, crop, 'yuv', block)
            assert classes is None and got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want), (block, crop)
            # against code that exists today: the grid summed over its cells is the plane PSNR's SSE, both halves
            assert torch.equal(got[..., 0].sum(dim=(2, 3)), ops.psnr_sse_yuv(pa.views, pg.views, crop))
            assert torch.equal(got[..., 1].sum(dim=(2, 3)), ops.psnr_sse_yuv(pl.views, pg.views, crop))
    # a subset of the planes in the order asked for, and the classes of the Y plane
    want = plane_ref(h, w, fmt, 8, 2, 16)
    got, classes = ops.gain_sums_yuv(pa.views, pl.views, pg.views, 2, 'vy', 16, par)
    assert torch.equal(got, want[:, [2, 0]])
    cw = torch.from_numpy(ref.gain_classes(a[0], l[0], g[0], par_map(h, w), 2))
    assert classes.dtype == torch.int64 and torch.equal(classes, cw) and int((cw[:, :, 0] > 0).sum()) >= 4 * T
    assert torch.equal(classes[:, :, 1:].sum(dim=1), want[:, 0].sum(dim=(1, 2)))
    assert torch.equal(ops.gain_sums_yuv(pa.views, pl.views, pg.views, 2, 'u', 16)[0], want[:, [1]])
    with pytest.raises(ValueError, match="'y'"):
        ops.gain_sums_yuv(pa.views, pl.views, pg.views, 2, 'uv', 16, par)
    # the per-frame values are the host's formula on those sums
    pa_, pl_, dp = ops.gain_yuv(pa.views, pl.views, pg.views, 2, 'yuv', 16)
    psnr = ops.psnr_yuv(pa.views, pg.views, 2)
    assert dp.shape == (T, 3) and close(pa_, psnr) and close(pl_, ops.psnr_yuv(pl.views, pg.views, 2))
    assert float((dp - (pa_ - pl_)).abs().max()) <= 1e-12 * float(pa_.max()) and bool((dp > 0).all())
    for p, v in zip((pa, pl, pg), (a, l, g)):
        assert unchanged(p, v)                                          # read only


@pytest.mark.parametrize('fmt,depth', [('420', 10), ('420', 12), ('422', 10), ('422', 12), ('444', 10)])
def test_16_bit_planes_low_and_high_aligned_are_the_restatement(fmt, depth):
    for h, w in SIZES:
        pa, pl, pg = clips16(h, w, fmt, depth)
        a, l, g = plane_values(h, w, fmt, depth)
        for block in BLOCKS:
            for crop in CROPS:
                want = plane_ref(h, w, fmt, depth, crop, block)
                got, _ = ops.gain_sums_yuv(pa.views, pl.views, pg.views, crop, 'yuv', block)
                assert got.dtype == torch.int64 and torch.equal(got, want), (h, w, block, crop)
                assert torch.equal(got[..., 0].sum(dim=(2, 3)), ops.psnr_sse_yuv(pa.views, pg.views, crop))
                assert torch.equal(got[..., 1].sum(dim=(2, 3)), ops.psnr_sse_yuv(pl.views, pg.views, crop))
        par = torch.from_numpy(par_map(h, w)).to(dev())
        _, classes = ops.gain_sums_yuv(pa.views, pl.views, pg.views, 6, 'y', 64, par)
        assert torch.equal(classes, torch.from_numpy(ref.gain_classes(a[0], l[0], g[0], par_map(h, w), 6)))
        pa_, _, _ = ops.gain_yuv(pa.views, pl.views, pg.views, 6, 'yuv', 64)
        assert close(pa_, ops.psnr_yuv(pa.views, pg.views, 6))            # the peak is 2^d - 1
        for p, v in zip((pa, pl, pg), (a, l, g)):
            assert unchanged(p, v)


# ------------------------------------------------------------------------------------------------ RGB frames and their luma
def rgb_values(h, w):
    key = ('rgb', h, w)
    if key not in _CACHE:
        rng = np.random.RandomState(h + 3 * w)
        g = rng.randint(0, 256, (T, h, w, 3)).astype(np.uint8)
        near = lambda s: np.clip(g.astype(np.int64) + rng.randint(-s, s + 1, g.shape), 0, 255).astype(np.uint8)      # noqa: E731
        _CACHE[key] = (near(9), near(14), g)
    return _CACHE[key]


def rgb_ref(h, w, crop, block, y):
    key = ('rgbref', h, w, crop, block, y)
    if key not in _CACHE:
        vals = rgb_values(h, w)
        if y:
            vals = tuple(ref.luma(x) for x in vals)
        _CACHE[key] = torch.from_numpy(ref.gain_grid(*vals, crop, block))
    return _CACHE[key]


def as_frames(x, kind):
    """(T,h,w,3) bytes -> the device clip: 'u8' as it is, 'f32' (T,3,h,w) planes byte / 255, 'off' fp32 planes off the byte grid that
    round to the same bytes (to_u8 rounds, and clamps what lies outside [0, 1])"""
    t = torch.from_numpy(x)
    if kind == 'u8':
        return t.to(dev())
    f = (torch.arange(256, dtype=torch.float32) / 255.0)[t.long()].permute(0, 3, 1, 2).contiguous()
    if kind == 'off':
        f = f + 0.3 / 255.0
        f = torch.where(torch.from_numpy(x).permute(0, 3, 1, 2) == 255, f + 0.5, f)
    return f.contiguous().to(dev())          # (torch.where may hand back the condition's permuted strides: the raw entries read memory)


@pytest.mark.parametrize('h,w', SIZES)
def test_rgb_frames_in_either_format_are_the_restatement(h, w):
    a, l, g = rgb_values(h, w)
    combos = list(itertools.product(('f32', 'u8'), repeat=3)) if (h, w) == SIZES[1] else [('u8', 'f32', 'u8'), ('off', 'u8', 'f32')]
    par = torch.from_numpy(par_map(h, w)).to(dev())
    L = _native.lib()
    for ka, kl, kg in combos:
        fa, fl, fg = as_frames(a, ka), as_frames(l, kl), as_frames(g, kg)
        keep = [x.clone() for x in (fa, fl, fg)]
        for block in BLOCKS:
            for crop in CROPS:
                want = rgb_ref(h, w, crop, block, False)
                got, classes = ops.gain_sums_frames(fa, fl, fg, crop, None, block)
                assert classes is None and got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want), (ka, kl, kg, block, crop)
                # the sums behind ops.psnr_frames: pnp_psnr_stat_io's integers on the same clips
                for q, (x, fx) in enumerate(((fa, ka), (fl, kl))):
                    stat = torch.empty(T, dtype=torch.int64, device=dev())
                    fmt = lambda k: _native.FRAMES_U8_HWC if k == 'u8' else _native.FRAMES_F32_NCHW      # noqa: E731
                    assert L.pnp_psnr_stat_io(ops._ptr(x), fmt(fx), ops._ptr(fg), fmt(kg), _native.COLOR_NONE, ops._ptr(stat), T, 3, h, w, crop,
                                              ops._stream()) == 0
                    assert torch.equal(got[:, 0, :, :, q].sum(dim=(1, 2)), stat.cpu()), (ka, kl, kg, block, crop, q)
        got, classes = ops.gain_sums_frames(fa, fl, fg, 2, None, 16, par)
        cw = torch.from_numpy(ref.gain_classes(a, l, g, par_map(h, w), 2))
        assert torch.equal(got, rgb_ref(h, w, 2, 16, False)) and classes.dtype == torch.int64 and torch.equal(classes, cw)
        assert bool((classes[:, :, 0].sum(dim=1) == (h - 4) * (w - 4)).all())
        pa_, pl_, dp = ops.gain_frames(fa, fl, fg, 2, None, 64)
        assert close(pa_, ops.psnr_frames(fa, fg, 2)) and close(pl_, ops.psnr_frames(fl, fg, 2)) and dp.shape == (T,)
        assert all(torch.equal(x, k) for x, k in zip((fa, fl, fg), keep))                       # read only
    # a leading shape of two dimensions
    two = ops.gain_sums_frames(as_frames(a, 'u8')[None], as_frames(l, 'f32')[None], as_frames(g, 'u8')[None], 2, None, 16, par[None])
    assert two[0].shape == (1, T) + tuple(rgb_ref(h, w, 2, 16, False).shape[1:]) and torch.equal(two[0][0], rgb_ref(h, w, 2, 16, False))
    assert two[1].shape == (1, T, 8, 3)


@pytest.mark.parametrize('h,w', SIZES)
def test_luma_sums_to_1e_12_and_the_same_bits_every_run(h, w):
    a, l, g = rgb_values(h, w)
    fa, fl, fg = as_frames(a, 'u8'), as_frames(l, 'f32'), as_frames(g, 'off')
    par = torch.from_numpy(par_map(h, w)).to(dev())
    worst = 0.0
    for block in BLOCKS:
        for crop in CROPS:
            want = rgb_ref(h, w, crop, block, True)
            got, _ = ops.gain_sums_frames(fa, fl, fg, crop, 'y', block)
            again, _ = ops.gain_sums_frames(fa, fl, fg, crop, 'Y', block)
            assert got.dtype == torch.float64 and got.shape == want.shape and torch.equal(got, again)
            err = ((got - want).abs() / want.clamp_min(1e-300)).where(want > 0, got.abs())
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= 1e-12, (block, crop, float(err.max()))
    print(f'{h}x{w}: luma grid, max relative difference {worst}')
    got, classes = ops.gain_sums_frames(fa, fl, fg, 2, 'y', 16, par)
    again = ops.gain_sums_frames(fa, fl, fg, 2, 'y', 16, par)
    assert torch.equal(got, again[0]) and torch.equal(classes, again[1]) and classes.dtype == torch.float64
    cw = torch.from_numpy(ref.gain_classes(*[ref.luma(x) for x in (a, l, g)], par_map(h, w), 2))
    assert torch.equal(classes[:, :, 0], cw[:, :, 0])
    err = ((classes - cw).abs() / cw.clamp_min(1e-300)).where(cw > 0, classes.abs())
    assert float(err.max()) <= 1e-12
    pa_, pl_, _ = ops.gain_frames(fa, fl, fg, 2, 'y', 16)
    assert close(pa_, ops.psnr_frames(fa, fg, 2, 'y')) and close(pl_, ops.psnr_frames(fl, fg, 2, 'y'))


# ------------------------------------------------------------------------------------------------ canaries and seams
def test_outputs_sit_between_untouched_canaries():
    h, w, crop, block = 66, 78, 2, 16
    L = _native.lib()
    rows, cols = metrics.gain_grid(h, w, block)
    CAN = 0x5A5A5A5A5A5A5A5A
    pad = 64

    def guarded(n):
        return torch.full((pad + n + pad,), CAN, dtype=torch.int64, device=dev())

    # planes: the grid of three planes and the class sums
    pa, pl, pg = clips8(h, w, '420')
    par = torch.from_numpy(par_map(h, w)).to(dev())
    ng, nc = T * 3 * rows * cols * 2, T * 24
    grid, cls = guarded(ng), guarded(nc)
    da, dl, dg = (ops._yuv_clip_desc(p.views, 'x')[0] for p in (pa, pl, pg))
    rc = L.pnp_gain_sums_yuv(ctypes.byref(da), ctypes.byref(dl), ctypes.byref(dg), 7, ops._ptr(par), ops._ptr(grid[pad:]), ops._ptr(cls[pad:]), T, h, w, crop,
                             block, 0, ops._stream())
    assert rc == 0
    want, wcls = ops.gain_sums_yuv(pa.views, pl.views, pg.views, crop, 'yuv', block, par)
    for buf, n, w_ in ((grid, ng, want), (cls, nc, wcls)):
        b = buf.cpu()
        assert bool((b[:pad] == CAN).all()) and bool((b[pad + n:] == CAN).all()) and torch.equal(b[pad:pad + n], w_.reshape(-1))
    # a mask of one plane leaves the others' cells written as zeros, and the canaries alone
    grid = guarded(ng)
    assert L.pnp_gain_sums_yuv(ctypes.byref(da), ctypes.byref(dl), ctypes.byref(dg), _native.PLANE_CB, None, ops._ptr(grid[pad:]), None, T, h, w, crop, block, 0,
                               ops._stream()) == 0
    b = grid.cpu()
    got = b[pad:pad + ng].reshape(T, 3, rows, cols, 2)
    assert bool((b[:pad] == CAN).all()) and bool((b[pad + ng:] == CAN).all()) and torch.equal(got[:, 1], want[:, 1]) and not bool(got[:, [0, 2]].any())
    # frames: integers, then the doubles of the luma with the class partials of every tile
    a, l, g = rgb_values(h, w)
    fa, fl, fg = as_frames(a, 'u8'), as_frames(l, 'f32'), as_frames(g, 'u8')
    for color, name in ((_native.COLOR_NONE, None), (_native.COLOR_Y, 'y')):
        tiles = int(L.pnp_gain_luma_tiles(h, w, crop, block))
        ng, nc = T * rows * cols * 2, T * 24 * (tiles if name else 1)
        grid, cls = guarded(ng), guarded(nc)
        rc = L.pnp_gain_sums_io(ops._ptr(fa), _native.FRAMES_U8_HWC, ops._ptr(fl), _native.FRAMES_F32_NCHW, ops._ptr(fg), _native.FRAMES_U8_HWC, color,
                                ops._ptr(par), ops._ptr(grid[pad:]), ops._ptr(cls[pad:]), T, 3, h, w, crop, block, ops._stream())
        assert rc == 0
        want, wcls = ops.gain_sums_frames(fa, fl, fg, crop, name, block, par)
        b, c = grid.cpu(), cls.cpu()
        assert bool((b[:pad] == CAN).all()) and bool((b[pad + ng:] == CAN).all()) and bool((c[:pad] == CAN).all()) and bool((c[pad + nc:] == CAN).all())
        if name:
            assert torch.equal(b[pad:pad + ng].view(torch.float64), want.reshape(-1))
            part = c[pad:pad + nc].view(torch.float64).reshape(T, tiles, 8, 3)
            assert torch.equal(torch.from_numpy(part.numpy().cumsum(axis=1)[:, -1].copy()), wcls)
        else:
            assert torch.equal(b[pad:pad + ng], want.reshape(-1)) and torch.equal(c[pad:pad + nc], wcls.reshape(-1))


def test_a_sample_on_a_seam_is_counted_once():
    """a single non-zero difference at a cell seam, a tile seam (columns 255 | 256 and 511 | 512 of the plane) and the crop's edge"""
    h, w, crop, block = 34, 530, 2, 16
    rows, cols = metrics.gain_grid(h, w, block)
    base = torch.full((1, h, w), 100, dtype=torch.uint8)
    half = torch.full((1, h // 2, w // 2), 100, dtype=torch.uint8)
    pg = yf.Planes(1, h, w, 'i420').fill(base, half, half)
    ug = torch.full((1, h, w, 3), 100, dtype=torch.uint8, device=dev())
    spots = [(15, 15), (15, 16), (16, 15), (16, 16), (20, 255), (20, 256), (21, 511), (21, 512), (31, 527), (32, 528),      # seams; the last two: cell 2 x 33
             (2, 2), (2, 527), (31, 2), (31, 300), (17, 527),                                                                 # the first and last rows and columns of the region
             (1, 40), (32, 40), (20, 1), (20, 528), (0, 0), (33, 529)]                                                        # in the crop: counted by nobody
    for y, x in spots:
        inside = crop <= y < h - crop and crop <= x < w - crop
        ya = base.clone()
        ya[0, y, x] = 107
        pa = yf.Planes(1, h, w, 'nv12', w + 1, 1).fill(ya, half, half)
        want = torch.zeros((1, 3, rows, cols, 2), dtype=torch.int64)
        if inside:
            want[0, 0, y // block, x // block, 0] = 49
        got, _ = ops.gain_sums_yuv(pa.views, pg.views, pg.views, crop, 'yuv', block)
        assert torch.equal(got, want), (y, x)
        # the chroma plane of 4:2:0: cells of 8 x 8, the crop 1, the same picture positions
        cy, cx = y // 2, x // 2
        ca = half.clone()
        ca[0, cy, cx] = 93
        pl = yf.Planes(1, h, w, 'i420').fill(base, half, ca)
        want = torch.zeros((1, 3, rows, cols, 2), dtype=torch.int64)
        if 1 <= cy < h // 2 - 1 and 1 <= cx < w // 2 - 1:
            want[0, 2, cy // 8, cx // 8, 1] = 49
        got, _ = ops.gain_sums_yuv(pg.views, pl.views, pg.views, crop, 'yuv', block)
        assert torch.equal(got, want), (cy, cx)
        # pixels: one channel of one pixel
        ua = ug.clone()
        ua[0, y, x, 1] = 90
        want = torch.zeros((1, 1, rows, cols, 2), dtype=torch.int64)
        if inside:
            want[0, 0, y // block, x // block, 0] = 100
        got, _ = ops.gain_sums_frames(ua, ug, ug, crop, None, block)
        assert torch.equal(got, want), (y, x)
    # 16-bit words at the same seams, block 128: two cells across a tile and a half
    w16 = torch.full((1, h, w), 400, dtype=torch.int32)
    h16 = torch.full((1, h // 2, w // 2), 400, dtype=torch.int32)
    qg = y16.Planes16(1, h, w, 'i420', 10, False).fill(w16, h16, h16)
    for y, x in ((20, 127), (20, 128), (20, 255), (20, 256), (20, 511), (20, 512)):
        v = w16.clone()
        v[0, y, x] = 1023
        qa = y16.Planes16(1, h, w, 'nv12', 10, True).fill(v, h16, h16)
        got, _ = ops.gain_sums_yuv(qa.views, qg.views, qg.views, 0, 'y', 128)
        want = torch.zeros((1, 1, 1, 5, 2), dtype=torch.int64)
        want[0, 0, 0, x // 128, 0] = 623 * 623
        assert torch.equal(got, want), (y, x)


# ------------------------------------------------------------------------------------------------ evaluate
def scorer(names, crop_border=0, **cfg):
    """one model for every case: evaluate() reads nothing of it but test_cfg (and whether its generator is a vsr one)"""
    if 'scorer' not in _CACHE:
        _CACHE['scorer'] = m8.restorer_model(['PSNR'])
    _CACHE['scorer'].test_cfg = dict(metrics=list(names), crop_border=crop_border, **cfg)
    return _CACHE['scorer']


def mean(x):
    """the mean over frames as evaluate() forms it for the gain names (numpy, fp64)"""
    return float(np.mean(x.numpy()))


def test_evaluate_returns_the_values_of_the_ops():
    h, w = 66, 78
    names = ['PSNR', 'SSIM', 'PSNR_LQ', 'SSIM_LQ', 'dPSNR', 'dSSIM', 'PSNR_SD', 'PSNR_SD_LQ']
    a, l, g = rgb_values(h, w)
    fa, fl, fg = as_frames(a, 'f32'), as_frames(l, 'u8'), as_frames(g, 'u8')
    par = torch.from_numpy(par_map(h, w)).to(dev())
    for convert_to in (None, 'y'):
        for crop, block in ((0, 64), (6, 16)):
            m = scorer(names, crop, convert_to=convert_to, gain_block=block)
            got = m.evaluate(fa[None], fg[None], lq=fl[None], par_map=par[None])
            pa_, pl_, dp = ops.gain_frames(fa, fl, fg, crop, convert_to, block)
            sa, sl = ops.ssim_frames(fa, fg, crop, convert_to), ops.ssim_frames(fl, fg, crop, convert_to)
            want = dict(PSNR=float(ops.psnr_frames(fa, fg, crop, convert_to).mean()), SSIM=float(sa.mean()), PSNR_LQ=mean(pl_),
                        SSIM_LQ=mean(sl), dPSNR=mean(dp), dSSIM=mean(sa - sl), PSNR_SD=metrics.gain_sd(pa_.numpy()),
                        PSNR_SD_LQ=metrics.gain_sd(pl_.numpy()))
            assert got == want and got['dPSNR'] > 0 and got['PSNR_SD'] > 0
            assert rel(got['PSNR_LQ'], float(ops.psnr_frames(fl, fg, crop, convert_to).mean())) <= 1e-12
            assert m.last_gain['classes'].shape == (T, 8, 3) and m.last_gain['grid'].shape == (T,) + metrics.gain_grid(h, w, block) + (2,)
            # the existing results are what they are without a gain name, and the host path agrees on the same bytes
            assert scorer(['PSNR', 'SSIM'], crop, convert_to=convert_to).evaluate(fa[None], fg[None]) == {k: got[k] for k in ('PSNR', 'SSIM')}
            host = scorer(['PSNR_LQ', 'dPSNR', 'PSNR_SD', 'PSNR_SD_LQ'], crop, convert_to=convert_to, gain_block=block).evaluate(
                fa[None].cpu(), as_frames(g, 'f32')[None].cpu(), lq=as_frames(l, 'f32')[None].cpu())
            for k in ('PSNR_LQ', 'dPSNR', 'PSNR_SD', 'PSNR_SD_LQ'):        # (the sums are equal integers; 'y': two fp64 summations)
                assert rel(host[k], got[k]) <= 1e-12, (k, host[k], got[k])
    with pytest.raises(KeyError):
        scorer(['PSNR', 'dPSNR_YUV']).evaluate(fa[None], fg[None], lq=fl[None])
    with pytest.raises(ValueError, match='lq'):
        scorer(['PSNR', 'dPSNR']).evaluate(fa[None], fg[None])
    # clips of planes, every name, on 4:2:0 8 bit, 4:2:2 8 bit and 4:2:0 10 bit
    all_names = ['PSNR', 'dPSNR', 'dPSNR_U', 'dPSNR_V', 'PSNR_LQ', 'PSNR_LQ_U', 'PSNR_LQ_V', 'dSSIM', 'dSSIM_U', 'dSSIM_V', 'SSIM_LQ', 'SSIM_LQ_U',
                 'SSIM_LQ_V', 'dPSNR_YUV', 'PSNR_SD', 'PSNR_SD_LQ', 'PSNR_YUV']
    lead = lambda v: type(v)(*[x[None] for x in v[:3]], *v[3:])      # noqa: E731
    for pa, pl, pg in (clips8(h, w, '420'), clips8(h, w, '422'), clips16(h, w, '420', 10)):
        for crop, block in ((0, 64), (2, 16)):
            m = scorer(all_names, crop, gain_block=block)
            got = m.evaluate(lead(pa.views), lead(pg.views), lq=pl.views, par_map=par[None])
            pa_, pl_, dp = ops.gain_yuv(pa.views, pl.views, pg.views, crop, 'yuv', block)
            sa, sl = ops.ssim_yuv(pa.views, pg.views, crop, 'yuv'), ops.ssim_yuv(pl.views, pg.views, crop, 'yuv')
            psnr = ops.psnr_yuv(pa.views, pg.views, crop)
            want = dict(PSNR=float(psnr[:, 0].mean()), PSNR_YUV=float(((6.0 * psnr[:, 0] + psnr[:, 1] + psnr[:, 2]) / 8.0).mean()),
                        PSNR_SD=metrics.gain_sd(pa_[:, 0].numpy()), PSNR_SD_LQ=metrics.gain_sd(pl_[:, 0].numpy()),
                        dPSNR_YUV=mean((6.0 * dp[:, 0] + dp[:, 1] + dp[:, 2]) / 8.0))
            for k, s in enumerate(('', '_U', '_V')):
                want.update({'dPSNR' + s: mean(dp[:, k]), 'PSNR_LQ' + s: mean(pl_[:, k]), 'SSIM_LQ' + s: mean(sl[:, k]), 'dSSIM' + s: mean(sa[:, k] - sl[:, k])})
            assert list(got) == all_names and got == {k: want[k] for k in all_names}
            assert torch.equal(torch.from_numpy(m.last_gain['classes']), ops.gain_sums_yuv(pa.views, pl.views, pg.views, crop, 'y', block, par)[1])
    with pytest.raises(ValueError, match='bit'):
        scorer(['dPSNR']).evaluate(clips8(h, w, '420')[0].views, clips8(h, w, '420')[2].views, lq=clips16(h, w, '420', 10)[1].views)


# ------------------------------------------------------------------------------------------------ the evaluation loop and the tool
NAMES = ('PSNR', 'dPSNR', 'PSNR_SD')


@pytest.fixture(scope='module')
def clip_tree(tmp_path_factory):
    """two synthetic 64 x 64 clips of 3 frames"""
    from pnp_vcve_amd import synthetic as syn
    return syn.write_clip_tree(str(tmp_path_factory.mktemp('gain') / 'data'), clips=['000', '011'], t=3, h=64, w=64, seed=6)


@pytest.mark.parametrize('switch', ['plain', 'byte_frames', 'byte_metrics'])
def test_multi_gpu_test_carries_the_names_with_and_without_the_byte_switches(clip_tree, switch):
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset
    lq, gt, qp = clip_tree
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    model = m8.restorer_model(NAMES, gain_block=32)
    seen, orig_eval = [], model.evaluate

    def spy_eval(output, gt, lq=None, par_map=None):
        seen.append((output.clone(), gt.clone(), lq.clone()))
        return orig_eval(output, gt, lq=lq, par_map=par_map)

    model.evaluate = spy_eval
    try:
        got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, metrics=NAMES, **({} if switch == 'plain' else {switch: True}))
    finally:
        model.evaluate = orig_eval
    assert len(got) == 2 and all(set(r['eval_result']) == set(NAMES) for r in got)
    assert all(np.isfinite(v) for r in got for v in r['eval_result'].values()) and got[0]['eval_result'] != got[1]['eval_result']
    want_lq = torch.float32 if switch == 'plain' else torch.uint8
    assert [x[2].dtype for x in seen] == [want_lq] * 2
    for r, (out, gt_, lq_) in zip(got, seen):                       # clip by clip: the ops' per-frame values behind it
        pa_, pl_, dp = ops.gain_frames(out[0], lq_[0], gt_[0], 0, None, 32)
        assert r['eval_result']['dPSNR'] == mean(dp) and r['eval_result']['PSNR_SD'] == metrics.gain_sd(pa_.numpy())
        assert r['eval_result']['PSNR'] == float(ops.psnr_frames(out[0], gt_[0]).mean())
    _CACHE[('loop', switch)] = [r['eval_result'] for r in got]
    if ('loop', 'plain') in _CACHE:                                 # the same bytes are scored whatever the switch: equal digits
        assert _CACHE[('loop', switch)] == _CACHE[('loop', 'plain')]
    # the gather of a distributed run carries them as it carries any name (one process: the identity)
    from pnp_vcve_amd import dist
    rows = [[r['eval_result'][k] for k in NAMES] for r in got]
    assert dist.gather_clip_metrics(rows, len(ds)).tolist() == rows


def test_multi_gpu_test_carries_the_names_with_yuv_frames(tmp_path):
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    names = ['PSNR', 'dPSNR', 'PSNR_SD', 'PSNR_LQ', 'dSSIM']      # (the tree's chroma planes may agree in a frame: E = 0 there, no finite dB)
    lq, gt, qp = m8.write_yuv_tree(tmp_path / 'data', 'i420', clips=('000', '011'), t=3, h=64, w=64)
    ds = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=64, layout='i420', qp_slice_file=qp))
    model = m8.restorer_model(metrics=names, gain_block=16)
    want_ = []
    for i in range(2):
        data = _to_device(collate([ds[i]]), dev())
        with torch.no_grad():
            buf = model.generator(data['lq'], *[data[k] for k in yf.SIDE], out_dtype='nv12')
        out = ops.yuv420_views(buf, 64, 64, 'nv12')
        want_.append(model.evaluate(out, data['gt'], lq=data['lq'], par_map=data['partitions']))
        one = lambda v: ops.Yuv420Frames(*[p[0] for p in v])      # noqa: E731
        pa_, pl_, dp = ops.gain_yuv(one(out), one(data['lq']), one(data['gt']), 0, 'yuv', 16)
        assert want_[-1]['dPSNR'] == mean(dp[:, 0]) and want_[-1]['PSNR_LQ'] == mean(pl_[:, 0])
        assert want_[-1]['PSNR_SD'] == metrics.gain_sd(pa_[:, 0].numpy()) and all(np.isfinite(v) for v in want_[-1].values())
    got = multi_gpu_test(model, ds, device=dev(), metrics=tuple(names), yuv_frames=True, yuv_out_layout='nv12')
    assert [r['eval_result'] for r in got] == want_                 # digit for digit


def _run_tools_test(tmp_path, tag, data_lines, names, *switches, extra=''):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfgp = tmp_path / f'cfg_{tag}.py'
    cfgp.write_text(f"_base_ = [{os.path.join(root, 'configs', 'REDS_folder_example.py')!r}]\n" + data_lines +
                    f"test_cfg = dict(metrics={names!r}, crop_border=0)\n" + extra)
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test.py'), str(cfgp), 'none', '--seed', '0', *switches],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    closing = [ln for ln in out.stdout.splitlines() if re.fullmatch(r'-?[0-9.naif]+(/-?[0-9.naif]+)+', ln.strip())]
    assert len(closing) == 1, out.stdout
    return closing[0].strip(), out.stdout


def _rgb_data(clip_tree):
    lq, gt, qp = clip_tree
    return (f"data = dict(test=dict(_delete_=True, type='SRREDSMultipleGTCompressDataset', lq_folder={lq!r}, gt_folder={gt!r},\n"
            f"                      num_input_frames=100, pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file={qp!r})], scale=1,\n"
            f"                      val_partition='REDS4', test_mode=True))\n")


def test_tools_test_writes_one_report_per_clip_and_prints_the_field(clip_tree, tmp_path):
    names = ['PSNR', 'SSIM', 'dPSNR', 'dSSIM', 'PSNR_SD', 'PSNR_SD_LQ']
    folder = tmp_path / 'gain'
    line, text = _run_tools_test(tmp_path, 'gain', _rgb_data(clip_tree), names, '--gain-report', str(folder), '--byte-metrics')
    assert re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}/-?\d+\.\d{4}', line)
    printed = float(re.search(r'Eval-dPSNR: (\S+)', text).group(1))
    assert f'{printed:.4f}' == line.rsplit('/', 1)[1] and np.isfinite(printed)
    assert sorted(os.listdir(folder)) == ['000.json', '011.json']
    docs = [json.load(open(folder / f)) for f in ('000.json', '011.json')]
    per_clip = []
    for d in docs:
        assert d['block'] == 64 and len(d['frames']) == 3 and np.array(d['grid']).shape == (1, 1)
        assert set(d['frames'][0]) == {'index', 'slice', 'qp', 'base_qp', 'PSNR', 'PSNR_LQ', 'dPSNR', 'SSIM', 'SSIM_LQ', 'dSSIM'}
        assert d['frames'][0]['slice'] == 'I' and all(f['slice'] in 'IPB' for f in d['frames']) and set(d['by_slice']) == {f['slice'] for f in d['frames']}
        assert len(d['classes']) == 8 and sum(row['N'] for row in d['classes']) == 3 * 64 * 64
        per_clip.append(sum(f['dPSNR'] for f in d['frames']) / 3)
        assert rel(d['dPSNR'], per_clip[-1]) <= 1e-12
    assert rel(printed, sum(per_clip) / 2) <= 1e-12                   # the per-frame dPSNR mean is the printed field


def test_tools_test_on_an_identity_enhancement_reports_a_gain_of_exactly_zero(clip_tree, tmp_path):
    """psnr_only scores the input frames: a is l"""
    names = ['PSNR', 'SSIM', 'dPSNR', 'PSNR_SD', 'PSNR_SD_LQ', 'PSNR_LQ']
    folder = tmp_path / 'gain'
    line, text = _run_tools_test(tmp_path, 'same', _rgb_data(clip_tree), names, '--gain-report', str(folder), extra='model = dict(psnr_only=True)\n')
    val = lambda k: float(re.search(r'Eval-' + k + r': (\S+)', text).group(1))      # noqa: E731
    assert val('dPSNR') == 0.0 and line.rsplit('/', 1)[1] in ('0.0000', '-0.0000') and val('PSNR_SD') == val('PSNR_SD_LQ')
    assert rel(val('PSNR_LQ'), val('PSNR')) <= 1e-12
    for f in ('000.json', '011.json'):
        d = json.load(open(folder / f))
        assert d['dPSNR'] == 0.0 and all(fr['dPSNR'] == 0.0 and fr['PSNR'] == fr['PSNR_LQ'] for fr in d['frames']) and not np.array(d['grid']).any()
