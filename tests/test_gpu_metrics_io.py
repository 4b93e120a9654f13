"""GPU: the metrics' format-independent front end (pnp_psnr_stat_io / pnp_ssim_partials_io / pnp_luma_from_frames): fp32 planes or
uint8 HWC frames for each input, optional luma (test_cfg.convert_to='y'), and the loop that evaluates on bytes (byte_metrics).

Shapes: 3 frames of 37x53 (h*w*3 = 5883 is odd: frames 1 and 2 start at odd addresses; the SSIM valid map is 27x43 = 2x2 tiles, both edge
tiles partial), 11x11 (a single SSIM position), 64x96; crops 0 and 3.  Every raw call writes into a NaN- / 0xFF-filled buffer with a
guard band behind it, which must stay untouched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pnp_vcve_amd import _native, metrics, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8 = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC
NONE, Y = _native.COLOR_NONE, _native.COLOR_Y
SHAPES = [(3, 37, 53), (2, 11, 11), (2, 64, 96)]
CROPS = [0, 3]
PAIRS = [('u8', 'u8'), ('u8', 'f32'), ('f32', 'u8')]
GUARD = 64


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def byte_pair(seed, frames, h, w):
    """two byte clips (frames,h,w,3) RGB that differ by small noise, with some pixels at 0 and 255"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8)
    a[:, 0, 0], a[:, -1, -1] = 0, 255
    b = (a.int() + torch.randint(-9, 10, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return a.to(dev()), b.to(dev())


def at_offset(u8, off):
    """the same bytes at byte address = off (mod 4), sliced out of a larger buffer"""
    flat = torch.full((u8.numel() + 8,), 0xEE, dtype=torch.uint8, device=u8.device)
    v = flat[off:off + u8.numel()].view(u8.shape)
    v.copy_(u8)
    assert v.data_ptr() % 4 == off and v.is_contiguous()
    return v


def as_fmt(u8, fmt):
    return u8 if fmt == 'u8' else ops.frames_from_rgb8(u8)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n, dtype):
    """n elements to be written + a guard band; float64 / float32: NaN, int64: 0xFF bytes"""
    buf = torch.full((n + GUARD,), -1 if dtype == torch.int64 else float('nan'), dtype=dtype, device=dev())
    return buf


def _check_guarded(buf, n, what):
    torch.cuda.synchronize()
    out, guard = buf[:n], buf[n:]
    if buf.dtype == torch.int64:
        assert bool((guard == -1).all()), (what, 'guard band written')
        assert bool((out >= 0).all()), (what, 'output not fully written')
    else:
        assert bool(torch.isnan(guard).all()), (what, 'guard band written')
        assert not bool(torch.isnan(out).any()), (what, 'output not fully written')
    return out.clone()


def _dims(t):
    if t.dtype == torch.uint8:
        return U8, t.shape[0], t.shape[1], t.shape[2]
    return F32, t.shape[0], t.shape[2], t.shape[3]


def raw_psnr(a, b, color, crop):
    """pnp_psnr_stat_io -> (frames) int64 SSE or (frames, blocks) float64 partials"""
    L = _native.lib()
    (fa, frames, h, w), fb = _dims(a), _dims(b)[0]
    nb = int(L.pnp_psnr_luma_blocks(h, w, crop)) if color == Y else 1
    assert nb >= 1
    buf = _guarded(frames * nb, torch.float64 if color == Y else torch.int64)
    rc = L.pnp_psnr_stat_io(_vp(a), fa, _vp(b), fb, color, _vp(buf), frames, 3, h, w, crop, _stream())
    assert rc == 0, rc
    out = _check_guarded(buf, frames * nb, ('psnr', fa, fb, color, crop))
    return out.reshape(frames, nb) if color == Y else out


def raw_ssim(a, b, color, crop):
    L = _native.lib()
    (fa, frames, h, w), fb = _dims(a), _dims(b)[0]
    nb = int(L.pnp_ssim_blocks(h, w, crop))
    planes = frames * (1 if color == Y else 3)
    buf = _guarded(planes * nb, torch.float64)
    rc = L.pnp_ssim_partials_io(_vp(a), fa, _vp(b), fb, color, _vp(buf), frames, 3, h, w, crop, _stream())
    assert rc == 0, rc
    return _check_guarded(buf, planes * nb, ('ssim', fa, fb, color, crop)).reshape(planes, nb)


# ------------------------------------------------------------------------------------------------ the numpy restatement
def ref_y(img_bgr_u8):
    """metrics.py:200-202 line by line, mmcv.bgr2ycbcr(y_only=True) restated from its published source: float32 image, np.dot with the
    list, + 16.0, / 255., astype(float32), * 255."""
    img = img_bgr_u8.astype(np.float32) / 255.
    out = np.dot(img, [24.966, 128.553, 65.481]) + 16.0
    out = out / 255.
    return out.astype(np.float32) * 255.


def bgr(u8_rgb_frame):
    return np.ascontiguousarray(u8_rgb_frame.cpu().numpy()[..., ::-1])


def crop2(x, c):
    return x[c:-c, c:-c] if c else x


# ------------------------------------------------------------------------------------------------ 1. luma, bit for bit
def test_luma_of_all_2_to_24_byte_triples_is_bit_equal_to_the_numpy_restatement():
    v = torch.arange(1 << 24, dtype=torch.int32)
    frame = torch.stack([v & 255, (v >> 8) & 255, v >> 16], dim=1).to(torch.uint8).reshape(1, 4096, 4096, 3)
    want = torch.from_numpy(ref_y(frame[0].numpy()[..., ::-1]))
    assert want.dtype == torch.float32 and want.shape == (4096, 4096)
    u8 = frame.to(dev())
    L = _native.lib()
    n = 4096 * 4096
    for src, fmt in ((u8, U8), (ops.frames_from_rgb8(u8), F32)):
        buf = _guarded(n, torch.float32)
        assert L.pnp_luma_from_frames(_vp(src), fmt, _vp(buf), 1, 4096, 4096, _stream()) == 0
        got = _check_guarded(buf, n, ('luma', fmt)).reshape(4096, 4096).cpu()
        assert torch.equal(got, want), (fmt, int((got != want).sum()))
        assert torch.equal(ops.luma_frames(src)[0].cpu(), want)
    assert abs(float(want.min()) - 16.0) < 1e-5 and abs(float(want.max()) - 235.0) < 1e-4


@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_luma_of_ragged_clips_at_every_byte_offset(off):
    """37x53: no frame is whole groups of four pixels' dwords, frames start at odd addresses; the plane's 16-byte stores only where aligned"""
    a, _ = byte_pair(3 + off, 3, 37, 53)
    want = torch.from_numpy(np.stack([ref_y(bgr(a[i])) for i in range(3)]))
    src = at_offset(a, off)
    buf = _guarded(3 * 37 * 53, torch.float32)
    assert _native.lib().pnp_luma_from_frames(_vp(src), U8, _vp(buf), 3, 37, 53, _stream()) == 0
    got = _check_guarded(buf, 3 * 37 * 53, ('luma', off)).reshape(3, 37, 53).cpu()
    assert torch.equal(got, want)
    assert torch.equal(ops.luma_frames(ops.frames_from_rgb8(a)).cpu(), want)
    assert ops.luma_frames(a[None]).shape == (1, 3, 37, 53)


# ------------------------------------------------------------------------------------------------ 2. bytes == planes
@pytest.mark.parametrize('crop', CROPS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_byte_frames_give_the_statistics_of_their_fp32_planes(shape, crop):
    frames, h, w = shape
    a, b = byte_pair(11 + h, frames, h, w)
    pa, pb = ops.frames_from_rgb8(a), ops.frames_from_rgb8(b)
    L = _native.lib()
    sse_ref = torch.empty(frames, dtype=torch.int64, device=dev())                     # the existing entry points on the planes
    assert L.pnp_psnr_sse_f32(_vp(pa), _vp(pb), _vp(sse_ref), frames, 3, h, w, crop, _stream()) == 0
    psnr_ref = ops.psnr_frames(pa, pb, crop)
    has_ssim = h - 2 * crop >= 11 and w - 2 * crop >= 11
    if has_ssim:
        nb = int(L.pnp_ssim_blocks(h, w, crop))
        part_ref = torch.empty((frames * 3, nb), dtype=torch.float64, device=dev())
        assert L.pnp_ssim_partials_f32(_vp(pa), _vp(pb), _vp(part_ref), frames, 3, h, w, crop, _stream()) == 0
        ssim_ref = ops.ssim_frames(pa, pb, crop)
    assert bool((sse_ref > 0).all())
    cases = [(as_fmt(a, fa), as_fmt(b, fb), (fa, fb)) for fa, fb in PAIRS]
    cases += [(at_offset(a, k), at_offset(b, (k + 1) % 4), ('off', k)) for k in (1, 2, 3)]
    cases += [(at_offset(a, 3), pb, ('off3', 'f32'))]
    for x, y, label in cases:
        assert torch.equal(raw_psnr(x, y, NONE, crop), sse_ref), (label, 'sse')
        assert torch.equal(ops.psnr_frames(x, y, crop), psnr_ref), (label, 'psnr')
        if has_ssim:
            assert torch.equal(raw_ssim(x, y, NONE, crop), part_ref), (label, 'ssim partials')
            assert torch.equal(ops.ssim_frames(x, y, crop), ssim_ref), (label, 'ssim')
        else:
            with pytest.raises(ValueError):
                ops.ssim_frames(x, y, crop)
    # leading dims and keyword use
    assert torch.equal(ops.psnr_frames(a[None], pb[None], crop_border=crop, convert_to=None), psnr_ref[None])


# ------------------------------------------------------------------------------------------------ 3. Y PSNR
@pytest.mark.parametrize('crop', CROPS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_luma_psnr_against_fp64_and_reference_style_float32(shape, crop):
    frames, h, w = shape
    a, b = byte_pair(21 + h, frames, h, w)
    want64, want32 = [], []
    for i in range(frames):
        ya, yb = crop2(ref_y(bgr(a[i])), crop), crop2(ref_y(bgr(b[i])), crop)
        d = ya - yb                                                                    # float32, as the reference subtracts
        assert d.dtype == np.float32
        want64.append(20. * np.log10(255. / np.sqrt(np.sum(d.astype(np.float64) ** 2) / d.size)))
        want32.append(float(metrics.psnr(bgr(a[i]), bgr(b[i]), crop, convert_to='y')))      # float32 np.mean, the reference's lines
    worst64 = worst32 = 0.0
    first = None
    for fa, fb in PAIRS + [('f32', 'f32')]:
        x, y = as_fmt(a, fa), as_fmt(b, fb)
        part = raw_psnr(x, y, Y, crop)
        got = ops.psnr_frames(x, y, crop, convert_to='y')
        assert got.dtype == torch.float64 and got.shape == (frames,)
        n = (h - 2 * crop) * (w - 2 * crop)
        assert torch.equal(got, 20.0 * torch.log10(255.0 / (torch.from_numpy(part.cpu().numpy().cumsum(axis=1)[:, -1].copy()) / n).sqrt()))
        first = got if first is None else first
        assert torch.equal(got, first), (fa, fb)                                       # every format pair: the same bits
        assert torch.equal(ops.psnr_frames(x, y, crop, 'Y'), got)                      # and again: identical from run to run
        assert torch.equal(raw_psnr(x, y, Y, crop), part)
        for i in range(frames):
            worst64 = max(worst64, abs(float(got[i]) - want64[i]))
            worst32 = max(worst32, abs(float(got[i]) - want32[i]))
    print(f'Y PSNR {shape} crop {crop}: device vs fp64 restatement {worst64:.3e} dB, vs the reference-style float32 mean {worst32:.3e} dB')
    assert worst64 <= 1e-9, worst64
    assert worst32 <= 5e-5, worst32
    # clips at other byte offsets: the same bits
    assert torch.equal(ops.psnr_frames(at_offset(a, 1), at_offset(b, 3), crop, 'y'), first)
    # identical frames
    same = ops.psnr_frames(a, ops.frames_from_rgb8(a), crop, 'y')
    assert bool(torch.isinf(same).all()) and bool((same > 0).all())
    with pytest.raises(ValueError, match='Wrong color model'):
        ops.psnr_frames(a, b, crop, 'ycbcr')


# ------------------------------------------------------------------------------------------------ 4. Y SSIM
@pytest.mark.parametrize('crop', CROPS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_luma_ssim_against_host_and_scipy_restatement(shape, crop):
    from test_host_logic import _ssim_scipy
    frames, h, w = shape
    a, b = byte_pair(31 + h, frames, h, w)
    if h - 2 * crop < 11:
        with pytest.raises(ValueError):
            ops.ssim_frames(a, b, crop, convert_to='y')
        return
    host = [float(metrics.ssim(bgr(a[i]), bgr(b[i]), crop, convert_to='y')) for i in range(frames)]
    sci = [float(_ssim_scipy(ref_y(bgr(a[i]))[..., None], ref_y(bgr(b[i]))[..., None], crop)) for i in range(frames)]
    first, worst = None, 0.0
    for fa, fb in PAIRS + [('f32', 'f32')]:
        x, y = as_fmt(a, fa), as_fmt(b, fb)
        part = raw_ssim(x, y, Y, crop)
        assert part.shape == (frames, int(_native.lib().pnp_ssim_blocks(h, w, crop)))
        got = ops.ssim_frames(x, y, crop, convert_to='Y')
        first = got if first is None else first
        assert torch.equal(got, first), (fa, fb)
        assert torch.equal(raw_ssim(x, y, Y, crop), part) and torch.equal(ops.ssim_frames(x, y, crop, 'y'), got)      # run to run
        for i in range(frames):
            worst = max(worst, abs(float(got[i]) - host[i]), abs(float(got[i]) - sci[i]))
    print(f'Y SSIM {shape} crop {crop}: device vs host / scipy {worst:.3e}')
    assert worst <= 1e-10, worst
    assert torch.equal(ops.ssim_frames(at_offset(a, 2), at_offset(b, 1), crop, 'y'), first)
    assert all(0.3 < v < 1.0 for v in host)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_bad_arguments_are_refused():
    L = _native.lib()
    BAD = 1001
    a, b = byte_pair(5, 2, 24, 24)
    pa, pb = ops.frames_from_rgb8(a), ops.frames_from_rgb8(b)
    out = torch.zeros(4096, dtype=torch.float64, device=dev())
    st = _stream()

    def psnr(x, fx, y, fy, color, c, h, w, crop):
        return L.pnp_psnr_stat_io(_vp(x), fx, _vp(y), fy, color, _vp(out), 2, c, h, w, crop, st)

    def ssim(x, fx, y, fy, color, c, h, w, crop):
        return L.pnp_ssim_partials_io(_vp(x), fx, _vp(y), fy, color, _vp(out), 2, c, h, w, crop, st)

    for fn in (psnr, ssim):
        assert fn(a, U8, b, U8, NONE, 3, 24, 24, 0) == 0
        assert fn(pa, F32, pb, F32, NONE, 1, 24, 24, 0) == 0                 # planes of any channel count, as the f32 entries
        for c in (1, 4):
            assert fn(a, U8, b, U8, NONE, c, 24, 24, 0) == BAD               # c != 3 with a byte format
            assert fn(pa, F32, b, U8, NONE, c, 24, 24, 0) == BAD
            assert fn(a, U8, pb, F32, NONE, c, 24, 24, 0) == BAD
            assert fn(pa, F32, pb, F32, Y, c, 24, 24, 0) == BAD              # c != 3 with Y
        assert fn(a, 2, b, U8, NONE, 3, 24, 24, 0) == BAD                    # unknown format
        assert fn(a, U8, b, -1, NONE, 3, 24, 24, 0) == BAD
        assert fn(a, U8, b, U8, 2, 3, 24, 24, 0) == BAD                      # unknown colour
        assert fn(a, U8, b, U8, -1, 3, 24, 24, 0) == BAD
        assert fn(a, U8, b, U8, NONE, 3, 24, 24, 12) == BAD                  # 2 crop >= h, w
        assert fn(a, U8, b, U8, Y, 3, 24, 30, 12) == BAD                     # 2 crop >= h
        assert fn(a, U8, b, U8, Y, 3, 30, 24, 12) == BAD                     # 2 crop >= w
        assert fn(a, U8, b, U8, NONE, 3, 24, 24, -1) == BAD
    assert psnr(a, U8, b, U8, Y, 3, 24, 24, 7) == 0                          # 10x10 inside the crop: PSNR runs,
    for color in (NONE, Y):
        assert ssim(a, U8, b, U8, color, 3, 24, 24, 7) == BAD                # SSIM has no 11x11 window
        assert ssim(a, U8, b, U8, color, 3, 10, 24, 0) == BAD
        assert ssim(a, U8, b, U8, color, 3, 24, 10, 0) == BAD
    assert L.pnp_luma_from_frames(_vp(a), 2, _vp(out), 2, 24, 24, st) == BAD
    assert L.pnp_luma_from_frames(_vp(a), U8, _vp(out), 0, 24, 24, st) == BAD
    assert L.pnp_psnr_luma_blocks(24, 24, 12) == 0 and L.pnp_psnr_luma_blocks(24, 24, 0) == 1
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match='Image shapes are different'):
        ops.psnr_frames(a, pb[:, :, :20], 0)
    with pytest.raises(TypeError):
        ops.psnr_frames(a, pb.half(), 0)
    with pytest.raises(ValueError):
        ops.ssim_frames(a.permute(0, 3, 1, 2).contiguous(), b, 0)           # uint8 planes: not the decoder's layout


# ------------------------------------------------------------------------------------------------ 6. wrapper and loop
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from pnp_vcve_amd import restorer, synthetic as syn  # noqa: F401
    from pnp_vcve_amd.datasets import build_dataset
    from pnp_vcve_amd.registry import build_model
    root = tmp_path_factory.mktemp('metrics_io')
    lq, gt, qp = syn.write_clip_tree(str(root / 'data'), clips=['000', '011'], t=3, h=64, w=96, seed=4)
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg)
    model = build_model(dict(type='BasicVSR', generator=gen, pixel_loss=dict(type='CharbonnierLoss')), train_cfg=None,
                        test_cfg=dict(metrics=['PSNR', 'SSIM'], crop_border=0))
    model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=9).items()})
    return root, (lq, gt, qp), ds, model.to(dev()).eval()


def test_byte_metrics_loop_equals_the_plain_loop(tree):
    from pnp_vcve_amd.apis import multi_gpu_test
    root, _, ds, model = tree
    model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=0)
    asked, gts = [], []
    orig_clips, orig_eval = model.generator.forward_clips, model.evaluate

    def spy(clips, out_dtype=None):
        asked.append((len(list(clips)), out_dtype, clips[0][0].dtype))
        return orig_clips(clips, out_dtype=out_dtype)

    def spy_eval(output, gt):
        gts.append((output.dtype, gt.dtype, tuple(gt.shape)))
        return orig_eval(output, gt)

    model.generator.forward_clips, model.evaluate = spy, spy_eval
    try:
        ref = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2)
        assert [g[:2] for g in gts] == [(torch.float32, torch.float32)] * 2
        got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_frames=True, byte_metrics=True)
        assert asked == [(2, torch.uint8, torch.uint8)]
        assert gts[2:] == [(torch.uint8, torch.uint8, (1, 3, 64, 96, 3))] * 2         # the metrics read two byte clips
        assert [r['eval_result'] for r in got] == [r['eval_result'] for r in ref]
        assert all(np.isfinite(v) and v > 0 for r in got for v in r['eval_result'].values())
        got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_metrics=True, save_image=True, save_path=str(root / 'a'))
        assert asked[-1] == (2, torch.uint8, torch.uint8)                              # the switch implies byte_frames
        assert [r['eval_result'] for r in got] == [r['eval_result'] for r in ref]
        ref1 = multi_gpu_test(model, ds, device=dev(), clips_in_flight=1, save_image=True, save_path=str(root / 'b'))
        assert [r['eval_result'] for r in ref1] == [r['eval_result'] for r in ref]
        for clip in ('000', '011'):
            for i in range(3):
                with open(root / 'a' / clip / f'{i:08d}.png', 'rb') as fa, open(root / 'b' / clip / f'{i:08d}.png', 'rb') as fb:
                    assert fa.read() == fb.read()
        # one clip at a time: the generator's own forward is asked for bytes as well
        one = multi_gpu_test(model, ds, device=dev(), clips_in_flight=1, byte_metrics=True)
        assert [r['eval_result'] for r in one] == [r['eval_result'] for r in ref]
    finally:
        model.generator.forward_clips, model.evaluate = orig_clips, orig_eval


@pytest.mark.parametrize('crop', CROPS)
def test_convert_to_y_through_the_loops_and_against_the_host(tree, crop):
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.metrics import tensor2img
    _, _, ds, model = tree
    model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=crop, convert_to='y')
    seen = []
    orig_eval = model.evaluate

    def spy_eval(output, gt):
        if output.dtype == torch.float32:
            seen.append((output.cpu(), gt.cpu()))
        return orig_eval(output, gt)

    model.evaluate = spy_eval
    try:
        plain = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2)
        byte = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_metrics=True)
    finally:
        model.evaluate = orig_eval
        model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=0)
    assert len(seen) == 2
    assert [r['eval_result'] for r in byte] == [r['eval_result'] for r in plain]
    for (out, gt), res in zip(seen, plain):
        host = {name: float(np.mean([fn(tensor2img(out[:, i]), tensor2img(gt[:, i]), crop, convert_to='y') for i in range(out.size(1))]))
                for name, fn in (('PSNR', metrics.psnr), ('SSIM', metrics.ssim))}
        dp, ds_ = abs(res['eval_result']['PSNR'] - host['PSNR']), abs(res['eval_result']['SSIM'] - host['SSIM'])
        print(f"convert_to=y crop {crop}: device {res['eval_result']} host {host}: |dPSNR| {dp:.3e} dB, |dSSIM| {ds_:.3e}")
        assert dp <= 5e-5 and ds_ <= 1e-10
    # 'Y' is the same switch; the three-channel values differ from it
    model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=crop, convert_to='Y')
    try:
        upper = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_metrics=True)
        model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=crop)
        rgb = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_metrics=True)
    finally:
        model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=0)
    assert [r['eval_result'] for r in upper] == [r['eval_result'] for r in byte]
    assert all(r['eval_result']['PSNR'] != q['eval_result']['PSNR'] for r, q in zip(rgb, byte))


def test_forward_test_evaluates_a_uint8_only_output_and_keeps_the_centre_frame_error(tree):
    from pnp_vcve_amd.apis import _to_device
    from pnp_vcve_amd.datasets import collate
    _, _, ds, model = tree
    model.test_cfg = dict(metrics=['PSNR', 'SSIM'], crop_border=0)
    data = _to_device(collate([ds.get_uint8(0)]), dev(), byte_frames=True, byte_metrics=True)
    assert data['lq'].dtype == torch.uint8 and data['gt'].dtype == torch.uint8
    planes = _to_device(collate([ds.get_uint8(0)]), dev(), byte_frames=True)
    assert planes['gt'].dtype == torch.float32 and torch.equal(ops.frames_from_rgb8(data['gt']), planes['gt'])
    with torch.no_grad():
        ref = model(test_mode=True, **planes)['eval_result']
        got = model(test_mode=True, out_dtype=torch.uint8, **data)['eval_result']
        mixed = model(test_mode=True, out_dtype=torch.uint8, **planes)['eval_result']           # byte output against fp32 gt
        assert got == ref and mixed == ref
        centre = dict(data, gt=planes['gt'][:, 1])
        with pytest.raises(ValueError, match='centre-frame'):
            model(test_mode=True, out_dtype=torch.uint8, **centre)


def test_tools_test_byte_metrics_with_convert_to_y_on_the_command_line(tree, tmp_path):
    _, (lq, gt, qp), _, _ = tree
    cfgp = tmp_path / 'folder_cfg.py'
    cfgp.write_text(
        f"_base_ = [{os.path.join(ROOT, 'configs', 'REDS_folder_example.py')!r}]\n"
        f"data = dict(test=dict(_delete_=True, type='SRREDSMultipleGTCompressDataset', lq_folder={lq!r}, gt_folder={gt!r},\n"
        f"                      num_input_frames=100, pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file={qp!r})], scale=1,\n"
        f"                      val_partition='REDS4', test_mode=True))\n")
    vals = {}
    for flag in ((), ('--byte-metrics',)):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), str(cfgp), 'none', '--seed', '0'] + list(flag) +
                             ['--cfg-options', 'test_cfg.convert_to=y'], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        vals[bool(flag)] = (re.search(r'Eval-PSNR: (\S+)', out.stdout).group(1), re.search(r'Eval-SSIM: (\S+)', out.stdout).group(1))
    print(vals)
    assert vals[True] == vals[False]
    p, s = float(vals[True][0]), float(vals[True][1])
    assert np.isfinite(p) and p > 0 and np.isfinite(s) and 0 < s <= 1
