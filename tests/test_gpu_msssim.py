"""GPU: multi-scale SSIM on the device (include/pnpvcve.h, pnp_msssim_*; csrc/msssim.hip) on every boundary SSIM is computed on, against
the independent restatement tests/msssim_ref.py, and through BasicVSR.evaluate and multi_gpu_test.

Inputs are msssim_ref.test_pair's: a smooth pattern plus noise, and the same blended with its 8 x 8 block means plus offsets, so that
every level's CS_s and S_s lies in [0.1, 0.999] in the restatement (asserted on the CPU side: no case passes by being trivial)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import msssim_ref as ref
import test_gpu_metrics_io as mio
import test_gpu_yuv16_frames as y16
import test_gpu_yuv_frames as yf
import test_gpu_yuv_metrics as m8
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
dev = yf.dev
T = 2
SIZES = [(176, 176, 0),      # level 4 is one window
         (178, 215, 0),      # an odd dimension at three levels: 215 -> 107 -> 53 -> 26 -> 13
         (200, 300, 4)]      # several ragged tiles at level 0, part tiles at every level
_CACHE = {}


def lut(u8):
    """uint8 CPU tensor -> fp32 device tensor byte / 255 (to_u8 of it is the byte)"""
    return (torch.arange(256, dtype=torch.float32) / 255.0)[u8.long()].to(dev())


def rgb_case(h, w, crop):
    """-> (a, b: (T,h,w,3) uint8 RGB CPU tensors; the restatement's scales (T,3,5,2) of the channels and (T,1,5,2) of the Y), computed once"""
    key = ('rgb', h, w, crop)
    if key not in _CACHE:
        pairs = [ref.test_pair(h, w, 100 * h + w + i, planes=3) for i in range(T)]
        a = np.stack([p[0].transpose(1, 2, 0) for p in pairs]).astype(np.uint8)
        b = np.stack([p[1].transpose(1, 2, 0) for p in pairs]).astype(np.uint8)
        cut = (lambda x: x[crop:-crop, crop:-crop]) if crop else (lambda x: x)
        none = np.array([[ref.plane_scales(cut(a[i, ..., c]), cut(b[i, ..., c])) for c in range(3)] for i in range(T)])
        y = np.array([[ref.plane_scales(cut(mio.ref_y(a[i, ..., ::-1])), cut(mio.ref_y(b[i, ..., ::-1])))] for i in range(T)])
        for s in (none, y):
            assert s.min() >= 0.1 and s.max() <= 0.999, (s.min(), s.max())
        _CACHE[key] = (torch.from_numpy(a), torch.from_numpy(b), none, y)
    return _CACHE[key]


def check(got, scales, want, tag):
    """device value and raw scales against the restatement's scales: 1e-10 per level; the value within 1e-9 (every factor >= 0.1: the
    product's error is at most sum w_s * 1e-10 / 0.1)"""
    err = float(np.abs(scales.numpy() - want).max())
    verr = float(np.abs(got.numpy() - ref.value(want).mean(axis=-1)).max())
    print(f'{tag}: scales in [{want.min():.4f}, {want.max():.4f}], max |device - restatement| = {err:.3e} per level, {verr:.3e} on the value')
    assert got.dtype == torch.float64 and scales.dtype == torch.float64 and not got.is_cuda
    assert err <= 1e-10, (tag, err)
    assert verr <= 1e-9, (tag, verr)


# ------------------------------------------------------------------------------------------------ 1. fp32 planes against the restatement
@pytest.mark.parametrize('convert_to', [None, 'y'])
@pytest.mark.parametrize('h,w,crop', SIZES)
def test_fp32_planes_against_the_restatement(h, w, crop, convert_to):
    a, b, none, y = rgb_case(h, w, crop)
    fa, fb = lut(a.permute(0, 3, 1, 2)), lut(b.permute(0, 3, 1, 2))
    got, scales = ops.msssim_frames(fa, fb, crop, convert_to, scales=True)
    want = y if convert_to else none
    assert got.shape == (T,) and scales.shape == (T,) + want.shape[1:]
    check(got, scales, want, f'{h}x{w} crop {crop} convert_to {convert_to}')
    assert torch.equal(ops.msssim_frames(fa, fb, crop, convert_to), got)
    if convert_to is None:      # one plane a frame: planes of any count go the same way
        g1, s1 = ops.msssim_frames(fa[:, 1:2], fb[:, 1:2], crop, scales=True)
        assert torch.equal(s1, scales[:, 1:2])


# ------------------------------------------------------------------------------------------------ 2. byte frames give the planes' result
@pytest.mark.parametrize('convert_to', [None, 'y'])
@pytest.mark.parametrize('h,w,crop', SIZES[1:])
def test_uint8_frames_give_exactly_the_fp32_planes_result(h, w, crop, convert_to):
    a, b, _, _ = rgb_case(h, w, crop)
    fa, fb = lut(a.permute(0, 3, 1, 2)), lut(b.permute(0, 3, 1, 2))
    want = ops.msssim_frames(fa, fb, crop, convert_to, scales=True)
    ua, ub = a.to(dev()), b.to(dev())
    for x, y in ((ua, ub), (ua, fb), (fa, ub), (mio.at_offset(ua, 1), mio.at_offset(ub, 3))):      # the last: odd base addresses
        got = ops.msssim_frames(x, y, crop, convert_to, scales=True)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), (x.dtype, y.dtype, x.data_ptr() % 4)


# ------------------------------------------------------------------------------------------------ 3. 8-bit 4:2:0 planes
def plane_case(h, w, peak=255):
    """-> two clips of planes [(T,h,w), (T,h/2,w/2), (T,h/2,w/2)] as int32 CPU tensors of sample values"""
    key = ('yuv', h, w, peak)
    if key not in _CACHE:
        out = ([], [])
        for k, (r, c) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
            pairs = [ref.test_pair(r, c, 7 * h + w + 10 * k + i, peak=peak) for i in range(T)]
            for side in (0, 1):
                out[side].append(torch.from_numpy(np.stack([p[side][0] for p in pairs]).astype(np.int32)))
        _CACHE[key] = out
    return _CACHE[key]


def test_8_bit_planes_are_msssim_frames_of_each_plane():
    h, w = 352, 356                                                 # chroma 176 x 178: its level 4 is 11 x 11
    a, b = [[p.to(torch.uint8) for p in clip] for clip in plane_case(h, w)]
    want = [ops.msssim_frames(m8.f32_plane(a[k]), m8.f32_plane(b[k]), 0, scales=True) for k in range(3)]
    want_v, want_s = torch.stack([x[0] for x in want], dim=1), torch.cat([x[1] for x in want], dim=1)      # (T,3), (T,3,5,2)
    s_ref = np.array([[ref.plane_scales(a[k][i].numpy(), b[k][i].numpy()) for k in range(3)] for i in range(T)])
    assert s_ref.min() >= 0.1 and s_ref.max() <= 0.999
    check(want_v.mean(dim=1), want_s, s_ref, '352x356 planes')      # (and the planes' result is the restatement's)
    ti = yf.Planes(T, h, w, 'i420').fill(*b)
    for layout, pitch, off, cpitch in (('nv12', w + 6, 3, None), ('nv21', w + 7, 1, None), ('i420', w + 7, 1, w // 2 + 3), ('i420', w, 0, None)):
        pa = yf.Planes(T, h, w, layout, pitch, off, cpitch).fill(*a)      # the two clips in different layouts
        got_v, got_s = ops.msssim_yuv420(pa.views, ti.views, 0, 'yuv', scales=True)
        assert got_v.shape == (T, 3) and got_v.dtype == torch.float64
        assert torch.equal(got_s, want_s) and torch.equal(got_v, want_v), (layout, pitch, off)
        assert torch.equal(pa.flat.cpu(), pa.expect(*a))              # read only
    pb = yf.Planes(T, h, w, 'nv21', w + 6, 2).fill(*b)
    assert torch.equal(ops.msssim_yuv420(yf.Planes(T, h, w, 'i420', w + 7, 3).fill(*a).views, pb.views, 0, 'vy'), want_v[:, [2, 0]])
    assert torch.equal(ops.msssim_yuv420(pa.views, ti.views, 0, 'u'), want_v[:, 1:2])


def test_a_crop_that_leaves_only_the_y_plane_large_enough():
    h, w, crop = 356, 360, 4
    a, b = [[p.to(torch.uint8) for p in clip] for clip in plane_case(h, w)]
    pa, pb = yf.Planes(T, h, w, 'nv12', w + 6, 1).fill(*a), yf.Planes(T, h, w, 'i420').fill(*b)
    got = ops.msssim_yuv420(pa.views, pb.views, crop, 'y', scales=True)
    want = ops.msssim_frames(m8.f32_plane(a[0]), m8.f32_plane(b[0]), crop, scales=True)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0][:, 0], want[0])
    for planes in ('u', 'v', 'yu'):                                 # chroma: 178 - 4 = 174 rows
        with pytest.raises(ValueError, match='176'):
            ops.msssim_yuv420(pa.views, pb.views, crop, planes)


# ------------------------------------------------------------------------------------------------ 4. 10 and 12 bit
@pytest.mark.parametrize('depth', [10, 12])
def test_16_bit_planes_against_the_restatement_whatever_the_container(depth):
    h = w = 352
    top = (1 << depth) - 1
    a, b = plane_case(h, w, top)
    s_ref = np.array([[ref.plane_scales(a[k][i].numpy(), b[k][i].numpy(), float(top)) for k in range(3)] for i in range(T)])
    assert s_ref.min() >= 0.1 and s_ref.max() <= 0.999
    base = None
    for msb, order, pitch, off in ((False, 'i420', None, 0), (True, 'nv12', 2 * w + 6, 6), (True, 'i420', 2 * w + 2, 2), (False, 'nv21', None, 0)):
        pa = y16.Planes16(T, h, w, order, depth, msb, pitch, off).fill(*a)
        pb = y16.Planes16(T, h, w, 'nv12' if order == 'i420' else 'i420', depth, not msb).fill(*b)      # described each on its own
        got = ops.msssim_yuv420(pa.views, pb.views, 0, 'yuv', scales=True)
        if base is None:
            base = got
            check(got[0].mean(dim=1), got[1], s_ref, f'{depth} bit 352x352')
            assert float(np.abs(got[0].numpy() - ref.value(s_ref)).max()) <= 1e-9
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (msb, order, pitch, off)
    # stray bits outside the value of a low-aligned word change nothing
    pa = y16.Planes16(T, h, w, 'i420', depth, False).fill(*a)
    pb = y16.Planes16(T, h, w, 'i420', depth, False).fill(*b)
    g = torch.Generator().manual_seed(depth)
    for v in pa.views[:3]:
        junk = torch.randint(1, 1 << (16 - depth), v.shape, generator=g, dtype=torch.int32) << depth
        v.copy_((v.cpu().int() & top | junk).to(torch.int16))
    assert int(pa.views.y.cpu().int().bitwise_and(0xffff).max()) > top
    got = ops.msssim_yuv420(pa.views, pb.views, 0, 'yuv', scales=True)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


# ------------------------------------------------------------------------------------------------ 5. fixed points
def test_fixed_points_and_determinism_on_the_device():
    a, b, _, _ = rgb_case(178, 215, 0)
    ua, ub = a.to(dev()), b.to(dev())
    fa = lut(a.permute(0, 3, 1, 2))
    for x, y, convert_to in ((fa, fa, None), (ua, ua, None), (fa, ua, None), (fa, fa, 'y'), (ua, fa, 'y')):      # identical clips: 1.0
        got = ops.msssim_frames(x, y, 0, convert_to)
        assert float((got - 1.0).abs().max()) <= 1e-12, (x.dtype, y.dtype, convert_to, got.tolist())
    p8 = [p.to(torch.uint8) for p in plane_case(352, 356)[0]]
    got = ops.msssim_yuv420(yf.Planes(T, 352, 356, 'nv12', 362, 1).fill(*p8).views, yf.Planes(T, 352, 356, 'i420').fill(*p8).views, 0, 'yuv')
    assert float((got - 1.0).abs().max()) <= 1e-12
    p16 = plane_case(352, 352, 1023)[0]
    got = ops.msssim_yuv420(y16.Planes16(T, 352, 352, 'nv12', 10, True).fill(*p16).views,
                            y16.Planes16(T, 352, 352, 'i420', 10, False).fill(*p16).views, 0, 'yuv')
    assert float((got - 1.0).abs().max()) <= 1e-12
    # the anticorrelated pair: exactly 0, not NaN; the raw means are finite and CS_0 is negative
    n = torch.randint(0, 256, (T, 176, 180, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(dev())
    got, scales = ops.msssim_frames(n, 255 - n, 0, scales=True)
    assert bool((got == 0.0).all()) and bool(torch.isfinite(scales).all()) and bool((scales[..., 0, 0] < 0).all())
    # two runs of one call: the same bits
    for call in (lambda: ops.msssim_frames(ua, ub, 0, scales=True), lambda: ops.msssim_frames(ua, ub, 0, 'y', scales=True)):
        r1, r2 = call(), call()
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_raise_before_any_gpu_work():
    z = torch.zeros((T, 3, 175, 400), device=dev())
    with pytest.raises(ValueError, match='176'):
        ops.msssim_frames(z, z)                                     # a 175-row frame
    z = torch.zeros((T, 184, 184, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError, match='176'):
        ops.msssim_frames(z, z, 6)                                  # a crop that takes the frame below 176
    with pytest.raises(ValueError, match='Wrong color model'):
        ops.msssim_frames(z, z, 0, 'ycbcr')
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.msssim_frames(z.cpu(), z.cpu())                         # no fallback
    p8 = [torch.zeros((T, 352, 352), dtype=torch.uint8), torch.zeros((T, 176, 176), dtype=torch.uint8), torch.zeros((T, 176, 176), dtype=torch.uint8)]
    pa, pb = yf.Planes(T, 352, 352, 'nv12').fill(*p8), yf.Planes(T, 352, 352, 'i420').fill(*p8)
    q10 = y16.Planes16(T, 352, 352, 'i420', 10, False).fill(*p8)
    q12 = y16.Planes16(T, 352, 352, 'i420', 12, False).fill(*p8)
    for crop in (1, 3, -2):
        with pytest.raises(ValueError, match='crop_border'):
            ops.msssim_yuv420(pa.views, pb.views, crop)             # an odd crop on 4:2:0
    with pytest.raises(ValueError, match='176'):
        ops.msssim_yuv420(pa.views, pb.views, 2, 'u')               # chroma 176 - 2
    with pytest.raises(ValueError, match='both'):
        ops.msssim_yuv420(pa.views, q10.views)                      # mixed 8 / 16-bit clips
    with pytest.raises(ValueError, match='bit depth'):
        ops.msssim_yuv420(q10.views, q12.views)                     # different depths
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.msssim_yuv420(pa.views, ops.Yuv420Frames(*[x.cpu() for x in pb.views]))
    with pytest.raises(ValueError, match='planes'):
        ops.msssim_yuv420(pa.views, pb.views, 0, 'yy')
    small = yf.Planes(T, 174, 352, 'i420').fill(*[torch.zeros((T, 174, 352), dtype=torch.uint8)] + [torch.zeros((T, 87, 176), dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match='176'):
        ops.msssim_yuv420(small.views, small.views)


# ------------------------------------------------------------------------------------------------ 7. through the model
def model_with(metrics, crop_border=0, **cfg):
    from pnp_vcve_amd import restorer, synthetic as syn      # noqa: F401
    from pnp_vcve_amd.registry import build_model
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **dict(syn.DEFAULT_GENERATOR_CFG))
    return build_model(dict(type='BasicVSR', generator=gen), train_cfg=None, test_cfg=dict(metrics=list(metrics), crop_border=crop_border, **cfg))


def test_evaluate_returns_the_means_of_the_ops_values():
    a, b, _, _ = rgb_case(176, 192, 0)
    fa, fb = lut(a.permute(0, 3, 1, 2)), lut(b.permute(0, 3, 1, 2))
    ua, ub = a.to(dev()), b.to(dev())
    for convert_to in (None, 'y'):
        m = model_with(['PSNR', 'SSIM', 'MS-SSIM'], convert_to=convert_to)
        want = {'PSNR': float(ops.psnr_frames(fa, fb, 0, convert_to).mean()), 'SSIM': float(ops.ssim_frames(fa, fb, 0, convert_to).mean()),
                'MS-SSIM': float(ops.msssim_frames(fa, fb, 0, convert_to).mean())}
        assert 0.1 < want['MS-SSIM'] < 0.999
        assert m.evaluate(fa[None], fb[None]) == want
        assert m.evaluate(ua[None], ub[None]) == want               # byte clips
        assert m.evaluate(ua[None], fb[None]) == want
    # the host path serves the name too: CPU tensors, a 4-D centre-frame pair
    m = model_with(['MS-SSIM'])
    host = m.evaluate(fa[:1].cpu(), fb[:1].cpu())['MS-SSIM']
    assert abs(host - float(ops.msssim_frames(fa[:1], fb[:1])[0])) <= 1e-9
    with pytest.raises(KeyError):
        model_with(['MS-SSIM_U']).evaluate(fa[None], fb[None])      # a plane metric on the RGB path, as PSNR_YUV
    # the plane path
    h = w = 352
    pa_, pb_ = [[p.to(torch.uint8) for p in clip] for clip in plane_case(h, w)]
    pa, pb = yf.Planes(T, h, w, 'nv12', w + 6, 1).fill(*pa_), yf.Planes(T, h, w, 'i420').fill(*pb_)
    m = model_with(['MS-SSIM', 'MS-SSIM_U', 'MS-SSIM_V', 'PSNR', 'SSIM_V'])
    got = m.evaluate(pa.views, pb.views)
    v = ops.msssim_yuv420(pa.views, pb.views, 0, 'yuv')
    assert [got[k] for k in ('MS-SSIM', 'MS-SSIM_U', 'MS-SSIM_V')] == [float(v[:, k].mean()) for k in range(3)]
    assert got['PSNR'] == float(ops.psnr_yuv420(pa.views, pb.views)[:, 0].mean()) and got['SSIM_V'] == float(ops.ssim_yuv420(pa.views, pb.views, 0, 'v').mean())
    assert list(got) == ['MS-SSIM', 'MS-SSIM_U', 'MS-SSIM_V', 'PSNR', 'SSIM_V']
    p10a, p10b = plane_case(h, w, 1023)
    qa, qb = y16.Planes16(T, h, w, 'nv12', 10, True).fill(*p10a), y16.Planes16(T, h, w, 'i420', 10, False).fill(*p10b)
    got = model_with(['MS-SSIM_V', 'MS-SSIM']).evaluate(qa.views, qb.views)
    v = ops.msssim_yuv420(qa.views, qb.views, 0, 'vy')
    assert got == {'MS-SSIM_V': float(v[:, 0].mean()), 'MS-SSIM': float(v[:, 1].mean())}


@pytest.fixture(scope='module')
def clip_tree(tmp_path_factory):
    """two synthetic 176 x 192 clips of 3 frames: the smallest the 176 rule and the generator both take"""
    from pnp_vcve_amd import synthetic as syn
    return syn.write_clip_tree(str(tmp_path_factory.mktemp('msssim') / 'data'), clips=['000', '011'], t=3, h=176, w=192, seed=6)


def test_multi_gpu_test_carries_the_metric_with_byte_metrics(clip_tree):
    from pnp_vcve_amd import synthetic as syn
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset
    lq, gt, qp = clip_tree
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    model = model_with(['PSNR', 'MS-SSIM'])
    model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=9).items()})
    model = model.to(dev()).eval()
    seen, orig_eval = [], model.evaluate

    def spy_eval(output, gt):
        seen.append((output.clone(), gt.clone()))
        return orig_eval(output, gt)

    model.evaluate = spy_eval
    try:
        got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, metrics=('PSNR', 'MS-SSIM'), byte_metrics=True)
    finally:
        model.evaluate = orig_eval
    assert len(got) == 2 and all(set(r['eval_result']) == {'PSNR', 'MS-SSIM'} for r in got)
    assert all(np.isfinite(v) and v > 0 for r in got for v in r['eval_result'].values())
    assert got[0]['eval_result'] != got[1]['eval_result']
    # clip by clip: evaluate on the two byte clips the loop scored, and the ops' per-frame values behind it
    assert [(o.dtype, g.dtype, tuple(g.shape)) for o, g in seen] == [(torch.uint8, torch.uint8, (1, 3, 176, 192, 3))] * 2
    for r, (out, gt_u8) in zip(got, seen):
        assert model.evaluate(out, gt_u8) == r['eval_result']
        assert r['eval_result']['MS-SSIM'] == float(ops.msssim_frames(out[0], gt_u8[0]).mean())
        assert r['eval_result']['PSNR'] == float(ops.psnr_frames(out[0], gt_u8[0]).mean())


def test_tools_test_prints_a_third_field_only_when_the_config_lists_the_metric(clip_tree, tmp_path):
    lq, gt, qp = clip_tree
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for name, metrics in (('with', ['PSNR', 'SSIM', 'MS-SSIM']), ('without', ['PSNR', 'SSIM'])):
        cfgp = tmp_path / f'cfg_{name}.py'
        cfgp.write_text(
            f"_base_ = [{os.path.join(root, 'configs', 'REDS_folder_example.py')!r}]\n"
            f"data = dict(test=dict(_delete_=True, type='SRREDSMultipleGTCompressDataset', lq_folder={lq!r}, gt_folder={gt!r},\n"
            f"                      num_input_frames=100, pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file={qp!r})], scale=1,\n"
            f"                      val_partition='REDS4', test_mode=True))\n"
            f"test_cfg = dict(metrics={metrics!r}, crop_border=0)\n")
        out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test.py'), str(cfgp), 'none', '--seed', '0', '--byte-metrics'],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        closing = [ln for ln in out.stdout.splitlines() if re.fullmatch(r'[0-9.naif]+(/[0-9.naif]+)+', ln.strip())]
        assert len(closing) == 1, out.stdout
        lines[name] = (closing[0].strip(), out.stdout)
    with_, without = lines['with'], lines['without']
    print(with_[0], without[0])
    assert re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}/\d\.\d{4}', with_[0]) and re.fullmatch(r'\d+\.\d{4}/\d\.\d{4}', without[0])
    assert with_[0].rsplit('/', 1)[0] == without[0]                # the two fields of today, byte for byte
    ms = float(re.search(r'Eval-MS-SSIM: (\S+)', with_[1]).group(1))
    assert 0 < ms <= 1 and f'{ms:.4f}' == with_[0].rsplit('/', 1)[1]
    assert 'MS-SSIM' not in without[1]


def test_multi_gpu_test_carries_the_plane_metrics_with_yuv_frames(tmp_path):
    """352 x 352: the smallest frame whose chroma planes hold level 4"""
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    names = ['PSNR', 'MS-SSIM', 'MS-SSIM_U', 'MS-SSIM_V']
    lq, gt, qp = m8.write_yuv_tree(tmp_path / 'data', 'i420', clips=('000',), t=3, h=352, w=352)
    ds = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=352, width=352, layout='i420', qp_slice_file=qp))
    model = m8.restorer_model(metrics=names)
    data = _to_device(collate([ds[0]]), dev())
    with torch.no_grad():
        buf = model.generator(data['lq'], *[data[k] for k in yf.SIDE], out_dtype='nv12')
    out = ops.yuv420_views(buf, 352, 352, 'nv12')
    want = model.evaluate(out, data['gt'])
    v = ops.msssim_yuv420(ops.Yuv420Frames(*[p[0] for p in out]), ops.Yuv420Frames(*[p[0] for p in data['gt']]), 0, 'yuv')
    assert [want[k] for k in names[1:]] == [float(v[:, k].mean()) for k in range(3)] and all(0 < want[k] <= 1 for k in names[1:])
    got = multi_gpu_test(model, ds, device=dev(), metrics=tuple(names), yuv_frames=True, yuv_out_layout='nv12')
    assert [r['eval_result'] for r in got] == [want]                # digit for digit
