"""GPU: PSNR-B on the device (include/pnpvcve.h, pnp_psnrb_*; csrc/psnrb.hip).  On every boundary that scores bytes or d-bit samples the
kernel leaves integers only, so every check of it is torch.equal against the independent restatement tests/psnrb_ref.py, which
enumerates the pairs; the fp32 Y of convert_to='y' leaves fp64 partials, whose sum in index order is the restatement's to 1e-12
relative.  The fp64 part is the host path's own function, so the values of ops.psnrb_* are == metrics.psnrb_values of the same sums.
Then the names through BasicVSR.evaluate, multi_gpu_test and tools/test.py.

Clips are psnrb_ref.blocky_plane's: constant within the 8 x 8 blocks of a grid plus a little noise (the test clip) against a smoothed
copy (the reference), so the boundary sums dominate at block 8 and every sum is non-zero.  The restatement of a clip is computed once,
kept and left unchanged.  Shapes: 64 x 80 (one tile wide, two high) and 66 x 79 / 66 x 78 (odd byte addresses, ragged groups of four,
a ragged last tile row); the seam test uses 70 x 530."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import psnrb_ref as ref
import test_gpu_yuv16_frames as y16
import test_gpu_yuv_frames as yf
import test_gpu_yuv_metrics as m8
from pnp_vcve_amd import _native, metrics, ops

pytestmark = pytest.mark.gpu
dev = yf.dev
T = 3
BLOCKS = (4, 8, 16)
MASKS = ('y', 'u', 'yu', 'v', 'yv', 'uv', 'yuv')         # plane masks 1 .. 7
_CACHE = {}


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    return float(np.max(np.where(both_inf, 0.0, r)))


# ------------------------------------------------------------------------------------------------ clips and their restatement
def rgb_clip(h, w, t=T):
    """-> (a, b): uint8 (t, h, w, 3) CPU tensors, the test clip and the reference"""
    key = ('rgb', h, w, t)
    if key not in _CACHE:
        pl = [[ref.blocky_plane(h, w, 8, 8, seed=100 * f + c + h) for c in range(3)] for f in range(t)]
        _CACHE[key] = tuple(torch.from_numpy(np.stack([np.stack([pl[f][c][k] for c in range(3)], axis=-1) for f in range(t)]).astype(np.uint8))
                            for k in (0, 1))
    return _CACHE[key]


def lut(u8):
    """uint8 (t, h, w, 3) -> fp32 (t, 3, h, w) planes on the device whose rounding to bytes gives the bytes back"""
    return (u8.permute(0, 3, 1, 2).float() / 255.0).contiguous().to(dev())


def luma(u8):
    """the fp32 Y the definition names: pnp_luma_from_frames of the byte clip -> (t, h, w) float32 numpy"""
    key = ('luma', u8.data_ptr())
    if key not in _CACHE:
        _CACHE[key] = ops.luma_frames(u8.to(dev())).cpu().numpy()
    return _CACHE[key]


def want_planes(key, a_planes, b_planes, crop, bp):
    """the restatement's sums of a list of plane pairs, computed once: list of [sse, sbh, snh, sbv, snv]"""
    key = ('want',) + key + (crop, bp)
    if key not in _CACHE:
        _CACHE[key] = [ref.plane_sums(a, b, crop, bp) for a, b in zip(a_planes, b_planes)]
    return _CACHE[key]


def want_rgb(h, w, crop, block, t=T):
    a, b = rgb_clip(h, w, t)
    an, bn = a.numpy().astype(np.int64), b.numpy().astype(np.int64)
    s = want_planes(('rgb', h, w, t), [an[f, :, :, c] for f in range(t) for c in range(3)], [bn[f, :, :, c] for f in range(t) for c in range(3)],
                    crop, block)
    return torch.tensor(s, dtype=torch.int64).reshape(t, 3, 5)


def want_y(h, w, crop, block, t=T):
    a, b = rgb_clip(h, w, t)
    ya, yb = luma(a), luma(b)
    s = want_planes(('y', h, w, t), list(ya), list(yb), crop, block)
    return np.array(s, np.float64).reshape(t, 1, 5)


def yuv_clip(h, w, d=8, t=T):
    """-> (a, b): (y, u, v) triples of (t, rows, cols) int32 CPU tensors of sample values; the chroma blocks are half size"""
    key = ('yuv', h, w, d, t)
    if key not in _CACHE:
        out = ([], [])
        for k, (rows, cols, bp) in enumerate(((h, w, 8), (h // 2, w // 2, 4), (h // 2, w // 2, 4))):
            pl = [ref.blocky_plane(rows, cols, d, bp, seed=1000 * d + 10 * f + k + w) for f in range(t)]
            for side in (0, 1):
                out[side].append(torch.from_numpy(np.stack([p[side] for p in pl]).astype(np.int32)))
        _CACHE[key] = out
    return _CACHE[key]


def want_yuv(h, w, d, crop, block, planes='yuv', t=T):
    """(t, 3, 5) int64: the restatement of the planes named, 0 for the others -- what the entry writes"""
    a, b = yuv_clip(h, w, d, t)
    out = torch.zeros((t, 3, 5), dtype=torch.int64)
    for k, p in enumerate('yuv'):
        if p in planes:
            s = want_planes(('yuv', h, w, d, t, k), list(a[k].numpy().astype(np.int64)), list(b[k].numpy().astype(np.int64)),
                            crop if k == 0 else crop // 2, block if k == 0 else block // 2)
            out[:, k] = torch.tensor(s, dtype=torch.int64)
    return out


def planes8(h, w, layout, vals, t=T):
    """an 8-bit clip at an odd base offset with an odd pitch"""
    return yf.Planes(t, h, w, layout, w + 5, 1 if layout == 'i420' else 3).fill(*[v.to(torch.uint8) for v in vals])


def planes16(h, w, d, container, vals, t=T):
    """'planar': yuv420pXXle (low-aligned words, three planes); 'p01x': P010 / P012 (high-aligned, interleaved chroma) with a wider pitch
    behind an offset"""
    if container == 'planar':
        return y16.Planes16(t, h, w, 'i420', d, False).fill(*vals)
    return y16.Planes16(t, h, w, 'nv12', d, True, 2 * w + 6, 6).fill(*vals)


# ------------------------------------------------------------------------------------------------ 1. RGB and Y clips
@pytest.mark.parametrize('convert_to', [None, 'y'])
@pytest.mark.parametrize('h,w', [(64, 80), (66, 79)])
def test_rgb_clips_equal_the_restatement(h, w, convert_to):
    a, b = rgb_clip(h, w)
    forms = {'f32': (lut(a), lut(b)), 'u8': (a.to(dev()), b.to(dev()))}
    if w % 2:
        assert forms['u8'][0][0, 1].data_ptr() % 2 == 1                        # byte rows at odd addresses
    worst = 0.0
    for block in BLOCKS:
        for crop in (0, 3):
            want = want_rgb(h, w, crop, block) if convert_to is None else want_y(h, w, crop, block)
            assert (np.asarray(want) > 0).all()
            for fa, fb in (('f32', 'f32'), ('u8', 'u8'), ('f32', 'u8'), ('u8', 'f32')):
                got = ops.psnrb_sums_frames(forms[fa][0], forms[fb][1], crop, convert_to, block)
                if convert_to is None:
                    assert got.dtype == torch.int64 and got.shape == (T, 3, 5) and torch.equal(got, want), (block, crop, fa, fb)
                else:
                    assert got.dtype == torch.float64 and got.shape == (T, 1, 5)
                    r = rel(got.numpy(), want)
                    worst = max(worst, r)
                    assert r <= 1e-12, (block, crop, fa, fb, r)
            # the no-reference form: sse 0, the other four unchanged
            for fa in ('f32', 'u8'):
                alone = ops.psnrb_sums_frames(forms[fa][0], None, crop, convert_to, block)
                assert bool((alone[..., 0] == 0).all()) and torch.equal(alone[..., 1:], got[..., 1:]), (block, crop, fa)
    if convert_to is not None:
        print(f'{h}x{w} Y: max relative difference of the summed partials {worst}')


def test_fp32_planes_of_any_channel_count():
    """pnp_psnr_stat_io takes fp32 planes of any c: one plane a block column, the samples to_u8 of the floats (values off the byte grid,
    below 0 and above 1 among them)"""
    h, w, c = 66, 79, 2
    g = torch.Generator().manual_seed(3)
    a = torch.rand((T, c, h, w), generator=g) * 1.2 - 0.1
    b = torch.rand((T, c, h, w), generator=g)
    to_u8 = lambda x: np.rint(np.clip(x.numpy(), 0, 1).astype(np.float32) * np.float32(255)).astype(np.int64)
    an, bn = to_u8(a), to_u8(b)
    for block, crop in ((8, 0), (16, 3)):
        want = torch.tensor([[ref.plane_sums(an[f, k], bn[f, k], crop, block) for k in range(c)] for f in range(T)], dtype=torch.int64)
        assert torch.equal(ops.psnrb_sums_frames(a.to(dev()), b.to(dev()), crop, None, block), want)
        assert torch.equal(ops.psnrb_sums_frames(a.to(dev()), None, crop, None, block)[..., 1:], want[..., 1:])


# ------------------------------------------------------------------------------------------------ 2. 4:2:0 planes, 8 bit
@pytest.mark.parametrize('crop', [0, 2])
@pytest.mark.parametrize('h,w', [(64, 80), (66, 78)])
def test_8_bit_planes_equal_the_restatement(h, w, crop):
    a, b = yuv_clip(h, w)
    for la, lb in (('i420', 'nv12'), ('nv12', 'nv21'), ('nv21', 'i420')):      # test and reference in layouts of their own
        pa, pb = planes8(h, w, la, a), planes8(h, w, lb, b)
        assert pa.views.y.data_ptr() % 2 == 1 and pa.views.y.stride(1) == w + 5
        for block in BLOCKS:
            for planes in (MASKS if block == 8 else ('yuv', 'vy')):
                got = ops.psnrb_sums_yuv420(pa.views, pb.views, crop, planes, block)
                assert got.dtype == torch.int64 and got.shape == (T, 3, 5)
                assert torch.equal(got, want_yuv(h, w, 8, crop, block, planes)), (la, lb, block, planes)
            alone = ops.psnrb_sums_yuv420(pa.views, None, crop, 'yuv', block)
            assert bool((alone[..., 0] == 0).all()) and torch.equal(alone[..., 1:], want_yuv(h, w, 8, crop, block)[..., 1:])
        assert torch.equal(pa.flat.cpu(), pa.expect(*[v.to(torch.uint8) for v in a]))      # read only
    assert bool((want_yuv(h, w, 8, crop, 8) > 0).all())


# ------------------------------------------------------------------------------------------------ 3. 10 and 12 bit, both containers
@pytest.mark.parametrize('crop', [0, 2])
@pytest.mark.parametrize('d', [10, 12])
@pytest.mark.parametrize('h,w', [(64, 80), (66, 78)])
def test_16_bit_planes_equal_the_restatement_whatever_the_container(h, w, d, crop):
    a, b = yuv_clip(h, w, d)
    assert int(a[0].max()) > (1 << (d - 1))                                    # the depth is used
    for ca, cb in (('planar', 'p01x'), ('p01x', 'planar'), ('p01x', 'p01x')):
        pa, pb = planes16(h, w, d, ca, a), planes16(h, w, d, cb, b)
        for block in BLOCKS:
            for planes in (MASKS if (block, ca, cb) == (8, 'planar', 'p01x') else ('yuv', 'u')):
                got = ops.psnrb_sums_yuv420(pa.views, pb.views, crop, planes, block)
                assert torch.equal(got, want_yuv(h, w, d, crop, block, planes)), (ca, cb, block, planes)
        alone = ops.psnrb_sums_yuv420(pa.views, None, crop, 'yuv', 8)
        assert bool((alone[..., 0] == 0).all()) and torch.equal(alone[..., 1:], want_yuv(h, w, d, crop, 8)[..., 1:])
        assert torch.equal(pa.flat.cpu(), pa.expect(*a))                       # read only


# ------------------------------------------------------------------------------------------------ 4. tile seams
def test_pairs_across_tile_seams_are_counted_once():
    """The kernel's tile is 256 columns x 32 rows (a wave: 8 rows of it), anchored at the region's first sample.  70 x 530 is two tiles
    and a ragged remainder both ways (2 x 256 + 18 columns, 2 x 32 + 6 rows).  The planted clip is exactly constant within the 8 x 8
    blocks of the grid: uncropped, the grid lines ARE the seams between lanes, waves and tiles, so every non-zero pair straddles one and
    a pair dropped or counted twice at a seam changes sbh / sbv; with a crop of 3 (RGB) or 2 (planes) the tiles move and the seams fall
    inside blocks while the grid stays."""
    h, w = 70, 530
    planted = [ref.block_constant(h, w, 8, seed=40 + c) for c in range(3)]
    u8 = torch.from_numpy(np.stack(planted, axis=-1).astype(np.uint8))[None]
    zero = torch.zeros_like(u8)
    for crop in (0, 3):
        want = torch.tensor([[ref.plane_sums(p, np.zeros_like(p), crop, 8) for p in planted]], dtype=torch.int64)
        assert bool((want[..., 2] == 0).all()) and bool((want[..., 4] == 0).all()) and bool((want[..., [0, 1, 3]] > 0).all())
        assert torch.equal(ops.psnrb_sums_frames(u8.to(dev()), zero.to(dev()), crop, None, 8), want)
        assert torch.equal(ops.psnrb_sums_frames(lut(u8), lut(zero), crop, None, 8), want)
        # every other block size sees the same steps: shared out between boundary and other pairs, none lost
        for block in (4, 16):
            got = ops.psnrb_sums_frames(u8.to(dev()), None, crop, None, block)
            assert torch.equal(got[..., 1] + got[..., 2], want[..., 1]) and torch.equal(got[..., 3] + got[..., 4], want[..., 3])
        # Y of the planted clip: a grey clip (R = G = B) keeps the blocks constant
        grey = u8[..., :1].expand(-1, -1, -1, 3).contiguous()
        ya, yb = (ops.luma_frames(x.to(dev())).cpu().numpy()[0] for x in (grey, torch.zeros_like(grey)))       # (the Y of black is 16)
        wy = np.array(ref.plane_sums(ya, yb, crop, 8))
        gy = ops.psnrb_sums_frames(grey.to(dev()), torch.zeros_like(grey).to(dev()), crop, 'y', 8).numpy()[0, 0]
        assert gy[2] == 0 and gy[4] == 0 and rel(gy, wy) <= 1e-12
    # the plane path: Y with blocks of 8, chroma (35 x 265: two tiles wide, one and a bit high) with blocks of 4
    y = torch.from_numpy(planted[0].astype(np.int32))[None]
    c = [torch.from_numpy(ref.block_constant(h // 2, w // 2, 4, seed=50 + k).astype(np.int32))[None] for k in range(2)]
    for crop in (0, 2):
        want = torch.tensor([[ref.plane_sums(p[0].numpy().astype(np.int64), None, crop if k == 0 else crop // 2, 8 if k == 0 else 4)
                              for k, p in enumerate([y] + c)]], dtype=torch.int64)
        assert bool((want[..., 2] == 0).all()) and bool((want[..., 4] == 0).all()) and bool((want[..., [1, 3]] > 0).all())
        p8 = planes8(h, w, 'nv12', [y] + c, t=1)
        assert torch.equal(ops.psnrb_sums_yuv420(p8.views, None, crop, 'yuv', 8), want)
        p10 = planes16(h, w, 10, 'p01x', [4 * y] + [4 * x for x in c], t=1)
        assert torch.equal(ops.psnrb_sums_yuv420(p10.views, None, crop, 'yuv', 8), 16 * want)
    # and a noisy clip of that size, where every pair counts
    a, b = yuv_clip(h, w, 8, 1)
    pa, pb = planes8(h, w, 'i420', a, t=1), planes8(h, w, 'nv21', b, t=1)
    for crop in (0, 2):
        assert torch.equal(ops.psnrb_sums_yuv420(pa.views, pb.views, crop, 'yuv', 8), want_yuv(h, w, 8, crop, 8, t=1))


# ------------------------------------------------------------------------------------------------ 5. stray writes and determinism
def test_the_output_sits_between_untouched_canaries_and_two_runs_give_the_same_bits():
    h, w, crop, block = 66, 78, 2, 8
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    a, b = rgb_clip(66, 79)
    ua, ub = a.to(dev()), b.to(dev())
    ya, yb = yuv_clip(h, w)
    pa, pb = planes8(h, w, 'nv12', ya), planes8(h, w, 'i420', yb)
    y10a, y10b = yuv_clip(h, w, 10)
    qa, qb = planes16(h, w, 10, 'p01x', y10a), planes16(h, w, 10, 'planar', y10b)
    nb = int(L.pnp_psnrb_luma_blocks(66, 79, crop))
    assert nb == 2
    da, db = ops._yuv_clip_desc(pa.views, 'a')[0], ops._yuv_clip_desc(pb.views, 'b')[0]
    ea, eb = ops._yuv_clip_desc(qa.views, 'a')[0], ops._yuv_clip_desc(qb.views, 'b')[0]
    calls = {
        'rgb': (T * 3 * 5, lambda out: L.pnp_psnrb_sums_io(ptr(ua), _native.FRAMES_U8_HWC, ptr(ub), _native.FRAMES_U8_HWC, _native.COLOR_NONE, out, T, 3,
                                                           66, 79, crop, block, stream)),
        'y': (T * nb * 5, lambda out: L.pnp_psnrb_sums_io(ptr(ua), _native.FRAMES_U8_HWC, ptr(ub), _native.FRAMES_U8_HWC, _native.COLOR_Y, out, T, 3,
                                                          66, 79, crop, block, stream)),
        'planes8': (T * 3 * 5, lambda out: L.pnp_psnrb_sums_yuv420(ctypes.byref(da), ctypes.byref(db), 5, out, T, h, w, crop, block, stream)),
        'planes16': (T * 3 * 5, lambda out: L.pnp_psnrb_sums_yuv420p16(ctypes.byref(ea), ctypes.byref(eb), 7, out, T, h, w, crop, block, stream)),
    }
    band, canary = 64, 0x5A5A5A5A5A5A5A5A
    for name, (n, call) in calls.items():
        runs = []
        for _ in range(2):
            buf = torch.full((band + n + band,), canary, dtype=torch.int64, device=dev())
            assert call(ctypes.c_void_p(buf.data_ptr() + 8 * band)) == 0, name
            got = buf.cpu()
            assert bool((got[:band] == canary).all()) and bool((got[band + n:] == canary).all()), name
            runs.append(got[band:band + n])
        assert torch.equal(runs[0], runs[1]), name
        assert not bool((runs[0] == canary).any()), name                       # every slot was written
    # what they left is what the ops return
    mid = lambda n, call: (lambda buf: (call(ctypes.c_void_p(buf.data_ptr())), buf.cpu())[1])(torch.empty(n, dtype=torch.int64, device=dev()))
    assert torch.equal(mid(*calls['rgb']).reshape(T, 3, 5), ops.psnrb_sums_frames(ua, ub, crop, None, block))
    assert torch.equal(mid(*calls['planes8']).reshape(T, 3, 5), ops.psnrb_sums_yuv420(pa.views, pb.views, crop, 'yv', block))
    assert torch.equal(mid(*calls['planes16']).reshape(T, 3, 5), ops.psnrb_sums_yuv420(qa.views, qb.views, crop, 'yuv', block))


# ------------------------------------------------------------------------------------------------ 6. values
@pytest.mark.parametrize('convert_to', [None, 'y'])
def test_rgb_values_are_the_host_paths_on_the_same_sums(convert_to):
    h, w = 66, 79
    a, b = rgb_clip(h, w)
    ua, ub = a.to(dev()), b.to(dev())
    for block, crop in ((8, 0), (16, 3), (4, 3)):
        sums = ops.psnrb_sums_frames(ua, ub, crop, convert_to, block)
        counts = metrics.psnrb_counts(h, w, crop, block)
        val, bef = metrics.psnrb_values(sums.numpy(), counts, block, (h - 2 * crop, w - 2 * crop), 255.0)
        got = ops.psnrb_frames(ua, ub, crop, convert_to, block)
        assert got.dtype == torch.float64 and got.shape == (T,) and np.array_equal(got.numpy(), val.mean(axis=-1))          # ==, not close
        assert np.array_equal(ops.bef_frames(ua, crop, convert_to, block).numpy(), bef.mean(axis=-1))
        assert torch.equal(ops.psnrb_frames(lut(a), ub, crop, convert_to, block), got)
        # the restatement's value, and the numpy host path on the BGR images evaluate() would hand it
        want = want_rgb(h, w, crop, block).numpy() if convert_to is None else want_y(h, w, crop, block)
        cnt = ref.counts(h, w, crop, block)
        wv = np.array([[ref.value(s, cnt, block, h - 2 * crop, w - 2 * crop, 255.0)[0] for s in f] for f in want])
        assert rel(got.numpy(), wv.mean(axis=-1)) <= 1e-12
        host = [metrics.psnrb(a[f].numpy()[..., ::-1], b[f].numpy()[..., ::-1], crop, convert_to=convert_to, block=block) for f in range(T)]
        assert rel(got.numpy(), host) <= 1e-12
        assert 5 < float(got.min()) and float(got.max()) < 60
    # a blocky clip has a BEF at its own block size, and PSNR-B below PSNR; the BEF is the first clip's
    assert bool((ops.bef_frames(ua, 0, convert_to, 8) > 0).all())
    assert bool((ops.psnrb_frames(ua, ub, 0, convert_to, 8) < ops.psnr_frames(ua, ub, 0, convert_to)).all())
    assert not torch.equal(ops.psnrb_frames(ub, ua, 0, convert_to, 8), ops.psnrb_frames(ua, ub, 0, convert_to, 8))
    # a leading batch shape
    two = ops.psnrb_frames(ua[None].expand(2, -1, -1, -1, -1), ub[None].expand(2, -1, -1, -1, -1), 0, convert_to, 8)
    assert two.shape == (2, T) and torch.equal(two[0], two[1]) and torch.equal(two[0], ops.psnrb_frames(ua, ub, 0, convert_to, 8))


@pytest.mark.parametrize('d', [8, 10, 12])
def test_plane_values_are_the_host_paths_on_the_same_sums(d):
    h, w, crop, block = 66, 78, 2, 16
    a, b = yuv_clip(h, w, d)
    pa = planes8(h, w, 'nv12', a) if d == 8 else planes16(h, w, d, 'p01x', a)
    pb = planes8(h, w, 'i420', b) if d == 8 else planes16(h, w, d, 'planar', b)
    peak = float((1 << d) - 1)
    sums = ops.psnrb_sums_yuv420(pa.views, pb.views, crop, 'yuv', block).numpy()
    for planes in ('yuv', 'vy', 'u'):
        got, bef = ops.psnrb_yuv420(pa.views, pb.views, crop, planes, block), ops.bef_yuv420(pa.views, crop, planes, block)
        assert got.dtype == bef.dtype == torch.float64 and got.shape == bef.shape == (T, len(planes))
        for i, p in enumerate(planes):
            k = 'yuv'.index(p)
            rows, cols, c, bp = (h, w, crop, block) if k == 0 else (h // 2, w // 2, crop // 2, block // 2)
            hv, hb = metrics.psnrb_values(sums[:, k], metrics.psnrb_counts(rows, cols, c, bp), bp, (rows - 2 * c, cols - 2 * c), peak)
            assert np.array_equal(got[:, i].numpy(), hv) and np.array_equal(bef[:, i].numpy(), hb)          # ==, not close
            wv = [ref.psnrb_plane(a[k][f].numpy().astype(np.int64), b[k][f].numpy().astype(np.int64), c, bp, peak) for f in range(T)]
            assert rel(got[:, i].numpy(), [x['value'] for x in wv]) <= 1e-12 and rel(bef[:, i].numpy(), [x['bef'] for x in wv]) <= 1e-12
    # a == b: the BEF alone is left, and a clip without block edges and without error gives +inf
    same = ops.psnrb_yuv420(pa.views, pa.views, crop, 'yuv', block)
    assert np.array_equal(same.numpy(), 10.0 * np.log10(peak ** 2 / ops.bef_yuv420(pa.views, crop, 'yuv', block).numpy()))
    flat = [torch.full_like(x, 1 << (d - 1)) for x in a]
    pf = planes8(h, w, 'i420', flat) if d == 8 else planes16(h, w, d, 'planar', flat)
    assert bool(torch.isinf(ops.psnrb_yuv420(pf.views, pf.views, crop, 'yuv', block)).all())


def test_refusals_raise_before_any_gpu_work():
    h, w = 64, 80
    a, b = rgb_clip(h, w)
    ua, ub = a.to(dev()), b.to(dev())
    ya, yb = yuv_clip(h, w)
    pa, pb = planes8(h, w, 'nv12', ya), planes8(h, w, 'i420', yb)
    for block in (0, 3, 12, 128, 8.0, '8', True, None):
        for call in (lambda: ops.psnrb_frames(ua, ub, 0, None, block), lambda: ops.bef_frames(ua, 0, 'y', block),
                     lambda: ops.psnrb_sums_frames(ua, ub, block=block), lambda: ops.psnrb_yuv420(pa.views, pb.views, 0, 'y', block),
                     lambda: ops.bef_yuv420(pa.views, 0, 'uv', block), lambda: ops.psnrb_sums_yuv420(pa.views, pb.views, block=block)):
            with pytest.raises(ValueError, match='block'):
                call()
    with pytest.raises(ValueError, match='needs'):
        ops.psnrb_frames(ua, ub, 25, None, 16)                      # 14 rows left
    with pytest.raises(ValueError, match='needs'):
        ops.psnrb_yuv420(pa.views, pb.views, 2, 'u', 64)            # the chroma plane, cropped by 1 to 30 x 38, holds no block of 32
    with pytest.raises(ValueError, match='needs'):
        ops.psnrb_yuv420(pa.views, pb.views, 26, 'yu', 16)          # Y: 12 x 28 holds no block of 16
    with pytest.raises(ValueError, match='crop_border'):
        ops.psnrb_yuv420(pa.views, pb.views, 3, 'y', 8)
    with pytest.raises(ValueError, match='planes'):
        ops.psnrb_yuv420(pa.views, pb.views, 0, 'yy', 8)
    with pytest.raises(ValueError, match='color model'):
        ops.psnrb_frames(ua, ub, 0, 'ycbcr', 8)
    with pytest.raises(AssertionError, match='shapes'):
        ops.psnrb_frames(ua, ub[:, :-1], 0, None, 8)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.psnrb_frames(a, b)                                      # no fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.bef_frames(a)
    q10, q12 = planes16(h, w, 10, 'planar', yuv_clip(h, w, 10)[0]), planes16(h, w, 12, 'planar', yuv_clip(h, w, 12)[0])
    with pytest.raises(ValueError, match='both'):
        ops.psnrb_yuv420(pa.views, q10.views)
    with pytest.raises(ValueError, match='bit depth'):
        ops.psnrb_yuv420(q10.views, q12.views)


# ------------------------------------------------------------------------------------------------ 7. through the model
def model_with(metrics_, crop_border=0, **cfg):
    from pnp_vcve_amd import restorer, synthetic as syn      # noqa: F401
    from pnp_vcve_amd.registry import build_model
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **dict(syn.DEFAULT_GENERATOR_CFG))
    return build_model(dict(type='BasicVSR', generator=gen), train_cfg=None, test_cfg=dict(metrics=list(metrics_), crop_border=crop_border, **cfg))


def test_evaluate_returns_the_clip_value_of_the_ops():
    h, w = 66, 79
    a, b = rgb_clip(h, w)
    fa, fb, ua, ub = lut(a), lut(b), a.to(dev()), b.to(dev())
    for convert_to in (None, 'y'):
        for crop, cfg, block in ((0, {}, 8), (3, dict(psnrb_block=16), 16)):
            m = model_with(['PSNR', 'PSNR-B'], crop, convert_to=convert_to, **cfg)
            want = {'PSNR': float(ops.psnr_frames(fa, fb, crop, convert_to).mean()), 'PSNR-B': float(ops.psnrb_frames(fa, fb, crop, convert_to, block).mean())}
            assert m.evaluate(fa[None], fb[None]) == want               # the output is the test clip
            assert m.evaluate(ua[None], ub[None]) == want               # byte clips
            assert m.evaluate(ua[None], fb[None]) == want
            assert m.evaluate(fb[None], fa[None])['PSNR-B'] != want['PSNR-B'] and m.evaluate(fb[None], fa[None])['PSNR'] == want['PSNR']
            # the host path serves the name too: CPU tensors, a 5-D clip and a 4-D centre-frame pair
            host = m.evaluate(fa[None].cpu(), fb[None].cpu())['PSNR-B']
            assert abs(host - want['PSNR-B']) <= 1e-12 * want['PSNR-B']
            one = m.evaluate(fa[:1].cpu(), fb[:1].cpu())['PSNR-B']
            assert abs(one - float(ops.psnrb_frames(fa[:1], fb[:1], crop, convert_to, block)[0])) <= 1e-12 * one
        for name in ('PSNR-B_U', 'PSNR-B_V'):                           # plane metrics on the RGB path, as PSNR_YUV
            with pytest.raises(KeyError):
                model_with([name], convert_to=convert_to).evaluate(fa[None], fb[None])
            with pytest.raises(KeyError):
                model_with([name], convert_to=convert_to).evaluate(ua[None], ub[None])
        with pytest.raises(KeyError):
            model_with(['PSNR-B_U']).evaluate(fa[None].cpu(), fb[None].cpu())
    with pytest.raises(ValueError, match='block'):
        model_with(['PSNR-B'], psnrb_block=12).evaluate(fa[None], fb[None])
    # the plane path, every name
    h, w = 66, 78
    ya, yb = yuv_clip(h, w)
    pa, pb = planes8(h, w, 'nv12', ya), planes8(h, w, 'i420', yb)
    names = ['PSNR-B', 'PSNR-B_V', 'PSNR', 'PSNR-B_U', 'SSIM_U', 'PSNR_YUV']
    for crop, cfg, block in ((0, {}, 8), (2, dict(psnrb_block=16, convert_to='y'), 16)):
        got = model_with(names, crop, **cfg).evaluate(pa.views, pb.views)
        v = ops.psnrb_yuv420(pa.views, pb.views, crop, 'yuv', block)
        assert list(got) == names
        assert [got[k] for k in ('PSNR-B', 'PSNR-B_U', 'PSNR-B_V')] == [float(v[:, k].mean()) for k in range(3)]
        p = ops.psnr_yuv420(pa.views, pb.views, crop)
        assert got['PSNR'] == float(p[:, 0].mean()) and got['PSNR_YUV'] == float(((6.0 * p[:, 0] + p[:, 1] + p[:, 2]) / 8.0).mean())
        assert got['SSIM_U'] == float(ops.ssim_yuv420(pa.views, pb.views, crop, 'u').mean())
        assert got['PSNR-B'] < got['PSNR']
    assert model_with(['PSNR-B']).evaluate(pb.views, pa.views)['PSNR-B'] != model_with(['PSNR-B']).evaluate(pa.views, pb.views)['PSNR-B']
    assert model_with(['PSNR-B_U']).evaluate(pa.views, pb.views) == {'PSNR-B_U': float(ops.psnrb_yuv420(pa.views, pb.views, 0, 'u', 8).mean())}
    # a batch dimension of one, and 10 / 12 bit
    lead = lambda v: type(v)(*[x[None] for x in v[:3]], *v[3:])
    for d in (10, 12):
        za, zb = yuv_clip(h, w, d)
        qa, qb = planes16(h, w, d, 'p01x', za), planes16(h, w, d, 'planar', zb)
        got = model_with(['PSNR-B_V', 'PSNR-B']).evaluate(lead(qa.views), lead(qb.views))
        v = ops.psnrb_yuv420(qa.views, qb.views, 0, 'vy', 8)
        assert got == {'PSNR-B_V': float(v[:, 0].mean()), 'PSNR-B': float(v[:, 1].mean())}
    from pnp_vcve_amd.restorer import BasicVSR
    assert all(n in BasicVSR.YUV_METRICS for n in ('PSNR-B', 'PSNR-B_U', 'PSNR-B_V'))


def test_multi_gpu_test_carries_the_names_with_yuv_frames(tmp_path):
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    names = ['PSNR', 'PSNR-B', 'PSNR-B_U', 'PSNR-B_V']
    lq, gt, qp = m8.write_yuv_tree(tmp_path / 'data', 'i420', clips=('000', '011'), t=3, h=64, w=64)
    ds = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=64, layout='i420', qp_slice_file=qp))
    model = m8.restorer_model(metrics=names, psnrb_block=16)
    want_ = []
    for i in range(2):
        data = _to_device(collate([ds[i]]), dev())
        with torch.no_grad():
            buf = model.generator(data['lq'], *[data[k] for k in yf.SIDE], out_dtype='nv12')
        out = ops.yuv420_views(buf, 64, 64, 'nv12')
        want_.append(model.evaluate(out, data['gt']))
        v = ops.psnrb_yuv420(ops.Yuv420Frames(*[p[0] for p in out]), ops.Yuv420Frames(*[p[0] for p in data['gt']]), 0, 'yuv', 16)
        assert [want_[-1][k] for k in names[1:]] == [float(v[:, k].mean()) for k in range(3)]
        assert all(np.isfinite(want_[-1][k]) and want_[-1][k] > 0 for k in names[1:])      # (a seeded generator's output: any finite value)
    got = multi_gpu_test(model, ds, device=dev(), metrics=tuple(names), yuv_frames=True, yuv_out_layout='nv12')
    assert [r['eval_result'] for r in got] == want_                 # digit for digit
    # and the gather of a distributed run carries them as it carries any name (one process: the identity)
    from pnp_vcve_amd import dist
    rows = [[r['eval_result'][k] for k in names] for r in got]
    assert dist.gather_clip_metrics(rows, len(ds)).tolist() == rows


@pytest.fixture(scope='module')
def clip_tree(tmp_path_factory):
    """two synthetic 64 x 64 clips of 3 frames"""
    from pnp_vcve_amd import synthetic as syn
    return syn.write_clip_tree(str(tmp_path_factory.mktemp('psnrb') / 'data'), clips=['000', '011'], t=3, h=64, w=64, seed=6)


@pytest.mark.parametrize('switch', ['plain', 'byte_frames', 'byte_metrics'])
def test_multi_gpu_test_carries_the_name_with_and_without_the_byte_switches(clip_tree, switch):
    from pnp_vcve_amd import synthetic as syn
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset
    lq, gt, qp = clip_tree
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    model = model_with(['PSNR', 'PSNR-B'], psnrb_block=16)
    model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=9).items()})
    model = model.to(dev()).eval()
    seen, orig_eval = [], model.evaluate

    def spy_eval(output, gt):
        seen.append((output.clone(), gt.clone()))
        return orig_eval(output, gt)

    model.evaluate = spy_eval
    try:
        got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, metrics=('PSNR', 'PSNR-B'),
                             **({} if switch == 'plain' else {switch: True}))
    finally:
        model.evaluate = orig_eval
    assert len(got) == 2 and all(set(r['eval_result']) == {'PSNR', 'PSNR-B'} for r in got)
    assert all(np.isfinite(v) and v > 0 for r in got for v in r['eval_result'].values())
    assert got[0]['eval_result'] != got[1]['eval_result']
    want_dtype = torch.uint8 if switch == 'byte_metrics' else torch.float32
    assert [(o.dtype, g.dtype) for o, g in seen] == [(want_dtype, want_dtype)] * 2
    for r, (out, gt_) in zip(got, seen):                            # clip by clip: the ops' per-frame values behind it
        assert r['eval_result']['PSNR-B'] == float(ops.psnrb_frames(out[0], gt_[0], 0, None, 16).mean())
        assert r['eval_result']['PSNR'] == float(ops.psnr_frames(out[0], gt_[0]).mean())
    _CACHE[('loop', switch)] = [r['eval_result'] for r in got]
    if ('loop', 'plain') in _CACHE:                                 # the same bytes are scored whatever the switch
        assert _CACHE[('loop', switch)] == _CACHE[('loop', 'plain')]


def _run_tools_test(tmp_path, tag, data_lines, names, *switches):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfgp = tmp_path / f'cfg_{tag}.py'
    cfgp.write_text(f"_base_ = [{os.path.join(root, 'configs', 'REDS_folder_example.py')!r}]\n" + data_lines +
                    f"test_cfg = dict(metrics={names!r}, crop_border=0)\n")
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test.py'), str(cfgp), 'none', '--seed', '0', *switches],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    closing = [ln for ln in out.stdout.splitlines() if re.fullmatch(r'[0-9.naif]+(/[0-9.naif]+)+', ln.strip())]
    assert len(closing) == 1, out.stdout
    return closing[0].strip(), out.stdout


def _rgb_data(clip_tree):
    lq, gt, qp = clip_tree
    return (f"data = dict(test=dict(_delete_=True, type='SRREDSMultipleGTCompressDataset', lq_folder={lq!r}, gt_folder={gt!r},\n"
            f"                      num_input_frames=100, pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file={qp!r})], scale=1,\n"
            f"                      val_partition='REDS4', test_mode=True))\n")


def _printed_field(line, text):
    printed = float(re.search(r'Eval-PSNR-B: (\S+)', text).group(1))
    assert np.isfinite(printed) and printed > 0 and f'{printed:.4f}' == line.rsplit('/', 1)[1]
    assert printed <= float(re.search(r'Eval-PSNR: (\S+)', text).group(1))
    return printed


def test_tools_test_prints_a_psnrb_field_only_when_the_config_lists_it(clip_tree, tmp_path):
    """byte clips (--byte-metrics), with and without the name"""
    with_ = _run_tools_test(tmp_path, 'with', _rgb_data(clip_tree), ['PSNR', 'SSIM', 'PSNR-B'], '--byte-metrics')
    without = _run_tools_test(tmp_path, 'without', _rgb_data(clip_tree), ['PSNR', 'SSIM'], '--byte-metrics')
    print(with_[0], without[0])
    assert re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}/\d+\.\d{4}', with_[0]) and re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}', without[0])
    assert with_[0].rsplit('/', 1)[0] == without[0]                # the two fields of today, byte for byte
    assert 'PSNR-B' not in without[1]
    _CACHE['tools bytes'] = (with_[0], _printed_field(*with_))


def test_tools_test_prints_the_field_on_rgb_clips(clip_tree, tmp_path):
    """fp32 clips, no switch; the same bytes are scored as with --byte-metrics"""
    line, text = _run_tools_test(tmp_path, 'rgb', _rgb_data(clip_tree), ['PSNR', 'SSIM', 'PSNR-B'])
    assert re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}/\d+\.\d{4}', line)
    printed = _printed_field(line, text)
    if 'tools bytes' in _CACHE:
        assert (line, printed) == _CACHE['tools bytes']


def test_tools_test_prints_the_field_on_yuv_frames(tmp_path):
    lq, gt, qp = m8.write_yuv_tree(tmp_path / 'data', 'i420', clips=('000', '011'), t=3, h=64, w=64)
    data = (f"data = dict(test=dict(_delete_=True, type='Yuv420ClipFolderDataset', lq_folder={lq!r}, gt_folder={gt!r}, height=64, width=64,\n"
            f"                      layout='i420', qp_slice_file={qp!r}))\n")
    save = tmp_path / 'out'
    line, text = _run_tools_test(tmp_path, 'yuv', data, ['PSNR', 'SSIM', 'PSNR-B'], '--yuv-frames', '--save-path', str(save))
    assert re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}/\d+\.\d{4}', line)
    printed = float(re.search(r'Eval-PSNR-B: (\S+)', text).group(1))
    assert f'{printed:.4f}' == line.rsplit('/', 1)[1]
    # what it printed is the ops' value of the frames it wrote against the ground truth's, the mean over the clips
    vals = []
    for c in ('000', '011'):
        bufs = [torch.from_numpy(np.fromfile(os.path.join(folder, c + '.yuv'), np.uint8).reshape(3, 96, 64)).to(dev()) for folder in (str(save), gt)]
        a, b = (ops.yuv420_views(x, 64, 64, 'i420') for x in bufs)
        vals.append(float(ops.psnrb_yuv420(a, b, 0, 'y', 8).mean()))
    assert printed == sum(vals) / 2 and np.isfinite(printed) and printed > 0
