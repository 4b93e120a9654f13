"""GPU: plane PSNR / SSIM of 10 / 12-bit 4:2:0 clips.  The SSE is an integer and must equal numpy's int64 sum on the same sample values;
the SSIM kernel is the 8-bit one's body behind a 16-bit sample load, so clips that hold the same values give the same bits whatever
their container and layout, and against the float64 definition with L = 2^d - 1 (tests/yuv16_ref.ssim_plane) the difference stays
below the 1e-10 that tests/test_gpu_any_size.py holds the device SSIM to against metrics.ssim (the project's figure for this kernel
family's summation order against a differently ordered fp64 sum; not measured for this kernel)."""
import numpy as np
import pytest
import torch

import test_gpu_yuv16_frames as y16
import test_gpu_yuv_metrics as m8
import yuv16_ref
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
dev = y16.dev
T = 3
SHAPES = [(40, 56), (66, 70)]
CROPS = m8.CROPS      # the crops the 8-bit test uses
_CACHE = {}


def crop_planes(vals, crop):
    c2 = crop // 2
    y, cb, cr = vals
    return [y[:, crop:y.shape[1] - crop, crop:y.shape[2] - crop], cb[:, c2:cb.shape[1] - c2, c2:cb.shape[2] - c2],
            cr[:, c2:cr.shape[1] - c2, c2:cr.shape[2] - c2]]


def sse_ref(a, b, crop):
    """(T, 3) int64: numpy's exact sum of squared differences of the cropped Y, Cb and Cr planes"""
    return np.stack([((p.numpy().astype(np.int64) - q.numpy().astype(np.int64)) ** 2).reshape(T, -1).sum(axis=1)
                     for p, q in zip(crop_planes(a, crop), crop_planes(b, crop))], axis=1)


def psnr_ref(sse, h, w, crop, depth):
    n = np.array([(h - 2 * crop) * (w - 2 * crop)] + [(h // 2 - crop) * (w // 2 - crop)] * 2, np.float64)
    with np.errstate(divide='ignore'):
        out = 10.0 * np.log10(float((1 << depth) - 1) ** 2 * n / sse.astype(np.float64))
    out[sse == 0] = np.inf
    return out


def clip_pair(h, w, depth):
    """two clips of decoder-like sample values and their numpy SSE per crop, drawn and computed once per shape and depth"""
    if (h, w, depth) not in _CACHE:
        a, b = y16.random_values(1000 + h + depth, T, h, w, depth), y16.random_values(2000 + w + depth, T, h, w, depth)
        _CACHE[(h, w, depth)] = (a, b, {c: sse_ref(a, b, c) for c in CROPS})
    return _CACHE[(h, w, depth)]


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_sse_is_numpys_int64_sum_and_the_psnr_uses_the_depths_peak(h, w, depth):
    a, b, want = clip_pair(h, w, depth)
    assert all(int(v.min()) > 0 for v in want.values())
    tight_b = y16.Planes16(T, h, w, 'i420', depth, False).fill(*b)
    for msb in (False, True):
        for order, pitch, off, cpitch in y16.layouts(w):
            pa = y16.Planes16(T, h, w, order, depth, msb, pitch, off, cpitch).fill(*a)      # `a` in every layout and container against a tight planar `b`
            for crop in CROPS:
                got = ops.psnr_sse_yuv420(pa.views, tight_b.views, crop)
                assert got.dtype == torch.int64 and got.shape == (T, 3)
                assert np.array_equal(got.numpy(), want[crop]), (msb, order, pitch, off, crop, got.tolist(), want[crop].tolist())
            assert torch.equal(pa.flat.cpu(), pa.expect(*a))                                 # read only
    tight_a = y16.Planes16(T, h, w, 'nv12', depth, True).fill(*a)
    for crop in CROPS:      # the PSNR the host forms of it, and the 6:1:1 mean: peak 2^d - 1
        got = ops.psnr_yuv420(tight_a.views, tight_b.views, crop)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), psnr_ref(want[crop], h, w, crop, depth)), crop
    # a pair that differs by max in every sample: 4095^2 = 2^24 per sample -- a 32-bit accumulator wraps (12 bit, 66 x 70: 7.7e10 per Y plane)
    top = (1 << depth) - 1
    zero = [torch.zeros_like(x) for x in a]
    full = [torch.full_like(x, top) for x in a]
    pz, pf = y16.Planes16(T, h, w, 'nv21', depth, True).fill(*zero), y16.Planes16(T, h, w, 'i420', depth, False, 2 * w + 6, 2).fill(*full)
    got = ops.psnr_sse_yuv420(pz.views, pf.views, 0).numpy()
    assert np.array_equal(got, np.broadcast_to(np.array([h * w, h * w // 4, h * w // 4], np.int64) * top * top, (T, 3)))
    if depth == 12:
        assert got[0, 0] > 1 << 32
    assert np.array_equal(ops.psnr_yuv420(pz.views, pf.views, 0).numpy(), np.zeros((T, 3)))       # 10 log10(peak^2 / peak^2)
    # a batch: (n,t,...) views
    v2 = ops.Yuv420Frames16(*[torch.stack([x, x.flip(0)]) for x in tight_a.views[:3]], depth, True)
    g2 = ops.Yuv420Frames16(*[torch.stack([x, x.flip(0)]) for x in tight_b.views[:3]], depth, False)
    got = ops.psnr_sse_yuv420(v2, g2, 2)
    assert got.shape == (2, T, 3) and np.array_equal(got[0].numpy(), want[2]) and np.array_equal(got[1].numpy(), want[2][::-1])


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
def test_equal_clips_give_sse_0_an_infinite_psnr_and_an_ssim_of_1(depth):
    a, _, _ = clip_pair(40, 56, depth)
    pa, pb = y16.Planes16(T, 40, 56, 'nv12', depth, True, 118, 2).fill(*a), y16.Planes16(T, 40, 56, 'i420', depth, False).fill(*a)
    for crop in CROPS:
        assert not bool(ops.psnr_sse_yuv420(pa.views, pb.views, crop).any())
        assert bool(torch.isinf(ops.psnr_yuv420(pa.views, pb.views, crop)).all())
        s = ops.ssim_yuv420(pa.views, pb.views, crop, 'yuv')
        assert s.dtype == torch.float64 and s.shape == (T, 3) and float((s - 1.0).abs().max()) <= 1e-12, (crop, s.tolist())
    s = ops.ssim_yuv420(pa.views, pa.views, 0, 'y')
    assert float((s - 1.0).abs().max()) <= 1e-12


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_ssim_is_one_value_whatever_the_container_and_is_the_float64_definition(h, w, depth):
    a, b, _ = clip_pair(h, w, depth)
    # a structured pair as well (SSIM of two independent noise clips is near 0): b2 = a with small noise
    g = torch.Generator().manual_seed(h * w + depth)
    top = (1 << depth) - 1
    b2 = [(x + torch.randint(-(top // 32), top // 32 + 1, x.shape, generator=g, dtype=torch.int32)).clamp_(0, top) for x in a]
    for other in (b, b2):
        base = None
        for msb, order, pitch, off in ((False, 'i420', None, 0), (True, 'i420', 2 * w + 2, 2), (False, 'nv12', None, 0), (True, 'nv21', 2 * w + 6, 6)):
            pa = y16.Planes16(T, h, w, order, depth, msb, pitch, off).fill(*a)
            pb = y16.Planes16(T, h, w, 'nv12' if order == 'i420' else 'i420', depth, not msb).fill(*other)      # described each on its own
            got = {crop: ops.ssim_yuv420(pa.views, pb.views, crop, 'yuv') for crop in CROPS}
            if base is None:
                base = got
            assert all(torch.equal(got[c], base[c]) for c in CROPS), (msb, order, pitch, off)      # the same bits: containers, interleaved / planar
            assert torch.equal(ops.ssim_yuv420(pa.views, pb.views, 2, 'vy'), got[2][:, [2, 0]])
        for crop in CROPS:
            want = np.array([[yuv16_ref.ssim_plane(p[i].numpy(), q[i].numpy(), depth) for p, q in zip(crop_planes(a, crop), crop_planes(other, crop))]
                             for i in range(T)])
            err = float(np.abs(base[crop].numpy() - want).max())
            print(f'{h}x{w} {depth} bit crop {crop}: SSIM in [{want.min():.4f}, {want.max():.4f}], max |device - float64 definition| = {err:.3e}')
            assert err < 1e-10, (crop, err)


def test_refusals_raise_before_any_gpu_work():
    a, b, _ = clip_pair(40, 56, 10)
    pa = y16.Planes16(T, 40, 56, 'nv12', 10, True).fill(*a)
    p12 = y16.Planes16(T, 40, 56, 'nv12', 12, True).fill(*b)
    p8 = m8.yf.Planes(T, 40, 56, 'nv12').fill(*m8.yf.random_planes(3, T, 40, 56))
    for f in (ops.psnr_sse_yuv420, ops.psnr_yuv420, ops.ssim_yuv420):
        with pytest.raises(ValueError, match='bit depth'):
            f(pa.views, p12.views)
        with pytest.raises(ValueError, match='8-bit'):      # mixing with 8-bit frames
            f(pa.views, p8.views)
        with pytest.raises(ValueError, match='8-bit'):
            f(p8.views, pa.views)
        with pytest.raises(ValueError, match='crop_border'):
            f(pa.views, pa.views, 3)
        with pytest.raises(ValueError, match='bit_depth'):
            f(ops.Yuv420Frames16(*pa.views[:3], 14, False), ops.Yuv420Frames16(*pa.views[:3], 14, False))
    with pytest.raises(ValueError, match='11x11'):
        ops.ssim_yuv420(pa.views, pa.views, 10, 'yu')


def test_evaluate_on_two_16_bit_clips_returns_these_values_means():
    model = m8.restorer_model(crop_border=2)
    a, b, _ = clip_pair(66, 70, 10)
    out = y16.Planes16(T, 66, 70, 'i420', 10, False).fill(*a).views
    gt = y16.Planes16(T, 66, 70, 'nv12', 10, True, 146, 2).fill(*b).views
    res = model.evaluate(ops.Yuv420Frames16(*[x[None] for x in out[:3]], 10, False), gt)      # (1,t,...) or (t,...) views
    assert list(res) == m8.ALL_METRICS
    p, s = ops.psnr_yuv420(out, gt, 2), ops.ssim_yuv420(out, gt, 2, 'yuv')
    want = dict(PSNR=p[:, 0].mean(), SSIM=s[:, 0].mean(), PSNR_U=p[:, 1].mean(), PSNR_V=p[:, 2].mean(), SSIM_U=s[:, 1].mean(), SSIM_V=s[:, 2].mean(),
                PSNR_YUV=((6.0 * p[:, 0] + p[:, 1] + p[:, 2]) / 8.0).mean())
    assert res == {k: float(v) for k, v in want.items()}
    assert np.array_equal(p.numpy(), psnr_ref(sse_ref(a, b, 2), 66, 70, 2, 10))
    out8 = m8.yf.Planes(T, 66, 70, 'nv12').fill(*m8.yf.random_planes(3, T, 66, 70)).views
    with pytest.raises(ValueError, match='Yuv420Frames16'):
        model.evaluate(out8, gt)
