"""GPU: the chroma modes of the 4:2:0 boundary (include/pnpvcve.h, "Chroma modes"): 'center', 'left' and 'topleft' beside the default.
The two conversions are held bit for bit to the numpy restatement (tests/yuv_chroma_ref.py) at 8, 10 and 12 bit; everything above them
is a composition of things that exist, as in tests/test_gpu_yuv_frames.py.  Every check is torch.equal or byte-equal: no tolerance."""
import os

import numpy as np
import pytest
import torch

import test_gpu_yuv16_frames as y16
import test_gpu_yuv_frames as yf
import yuv_chroma_ref as cref
import yuv_ref
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
dev, fwd = yf.dev, yf.fwd
MODES = ('center', 'left', 'topleft')
# name, 8-bit layout / 16-bit plane order, depth, msb_aligned
CONTAINERS = [('nv12', 'nv12', 8, False), ('nv21', 'nv21', 8, False), ('i420', 'i420', 8, False), ('p010', 'nv12', 10, True),
              ('yuv420p12le', 'i420', 12, False)]
STANDARDS = {'nv12': 'bt601-limited', 'nv21': 'bt709-full', 'i420': 'bt709-limited', 'p010': 'bt709-limited', 'yuv420p12le': 'bt601-full'}
# 2 x 2: every clamp hits at once; one chroma row / one chroma column; two blocks of threads at an odd pitch and address (8 bit) or an
# even one that is not 8-byte aligned (16 bit)
SIZES = [(2, 2, False), (2, 6, False), (6, 2, False), (64, 96, True)]
T = 2
_MODELS = {}


def planes_of(container, t, h, w, awkward=False):
    name, order, depth, msb = container
    if depth == 8:
        return yf.Planes(t, h, w, order, w + 7 if awkward else None, 1 if awkward else 0)
    return y16.Planes16(t, h, w, order, depth, msb, 2 * w + 6 if awkward else None, 2 if awkward else 0)


def values_of(seed, container, t, h, w):
    depth = container[2]
    return yf.random_planes(seed, t, h, w) if depth == 8 else y16.random_values(seed, t, h, w, depth)


def from_ref(vals, standard, depth, mode):
    return torch.from_numpy(cref.from_planes(*[v.numpy() for v in vals], standard, depth, mode))


def ops_of(container):
    """-> (frames_from, frames_to, pack) of the container's sample size"""
    if container[2] == 8:
        return ops.frames_from_yuv420, ops.frames_to_yuv420, ops.pack_lr_yuv420
    return ops.frames_from_yuv420p16, ops.frames_to_yuv420p16, ops.pack_lr_yuv420p16


@pytest.mark.parametrize('container', CONTAINERS, ids=[c[0] for c in CONTAINERS])
@pytest.mark.parametrize('mode', MODES)
def test_planes_to_rgb_is_the_restatement_and_reads_only(mode, container):
    standard, depth = STANDARDS[container[0]], container[2]
    frames_from, _, pack = ops_of(container)
    for h, w, awkward in SIZES:
        vals = values_of(100 + h + w, container, T, h, w)
        want = from_ref(vals, standard, depth, mode).to(dev())
        p = planes_of(container, T, h, w, awkward).fill(*vals)
        got = frames_from(p.views, standard, chroma=mode)
        assert got.shape == (T, 3, h, w) and torch.equal(got, want), (h, w, int((got != want).sum()))
        for general in (False, True):       # the forward's unpacking: the same values as RGB0
            lr4 = pack(p.views, standard, general=general, chroma=mode)
            assert torch.equal(lr4[..., :3].permute(0, 3, 1, 2), want) and not bool(lr4[..., 3].any()), (h, w, general)
        assert torch.equal(p.flat.cpu(), p.expect(*vals)), (h, w, 'the planes or their guard bytes were written')
    if depth == 8:      # the custom op keeps its schema: its `standard` integer carries the code
        code = ops._yuv_code(standard, mode)
        assert code == yuv_ref.STANDARDS.index(standard) | _native.YUV_CHROMA[mode] << 8
        assert torch.equal(torch.ops.pnpvcve.frames_from_yuv420(*p.views, code), got)
        assert torch.equal(torch.ops.pnpvcve.frames_from_yuv420(*p.views, code & 255), frames_from(p.views, standard))


@pytest.mark.parametrize('container', CONTAINERS, ids=[c[0] for c in CONTAINERS])
@pytest.mark.parametrize('mode', MODES)
def test_rgb_to_planes_is_the_restatement_and_writes_nothing_else(mode, container):
    standard, depth = STANDARDS[container[0]], container[2]
    _, frames_to, _ = ops_of(container)
    for h, w, awkward in SIZES:
        g = torch.Generator().manual_seed(7 * h + w)
        x = torch.rand((T, 3, h, w), generator=g) * 1.4 - 0.2
        want = [torch.from_numpy(v.astype(np.int32)) for v in cref.to_planes(x.numpy(), standard, depth, mode)]
        if depth == 8:
            want = [v.to(torch.uint8) for v in want]
        p = planes_of(container, T, h, w, awkward)
        frames_to(x.to(dev()), standard, out=p.views, chroma=mode)
        got, exp = p.flat.cpu(), p.expect(*want)
        assert torch.equal(got, exp), (h, w, int((got != exp).sum()))
        if mode == 'center':        # the box mean, as 'replicate'
            q = planes_of(container, T, h, w, awkward)
            frames_to(x.to(dev()), standard, out=q.views)
            assert torch.equal(q.flat, p.flat), (h, w)


@pytest.mark.parametrize('container', CONTAINERS, ids=[c[0] for c in CONTAINERS])
def test_the_aligned_and_the_general_pack_agree_with_each_other_and_with_the_conversion(container):
    standard = STANDARDS[container[0]]
    frames_from, _, pack = ops_of(container)
    for h, w, off in ((64, 96, 0), (64, 98, 0), (64, 96, 2)):       # 98: no multiple of 4, and an offset of 2: the general form only
        vals = values_of(31 + w + off, container, 3, h, w)
        name, order, depth, msb = container
        p = (yf.Planes(3, h, w, order, None, off) if depth == 8 else y16.Planes16(3, h, w, order, depth, msb, None, off)).fill(*vals)
        for mode in MODES:
            fast, slow = pack(p.views, standard, chroma=mode), pack(p.views, standard, general=True, chroma=mode)
            assert fast.shape == (3, h, w, 4) and torch.equal(fast, slow), (w, off, mode, int((fast != slow).sum()))
            assert torch.equal(fast[..., :3].permute(0, 3, 1, 2), frames_from(p.views, standard, chroma=mode)), (w, off, mode)
            assert torch.equal(fast[..., :3].permute(0, 3, 1, 2).cpu(), from_ref(vals, standard, depth, mode)), (w, off, mode)
        assert torch.equal(p.flat.cpu(), p.expect(*vals))


# ------------------------------------------------------------------------------------------------ the forward
def model(**cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _MODELS:
        _MODELS[key] = yf.build(dict(num_blocks=2, **cfg), seed=433)
    return _MODELS[key]


@pytest.mark.parametrize('mode', ['left', 'topleft'])
def test_forward_on_planes_is_the_forward_on_their_conversion_in_that_mode(mode):
    m, std = model(), 'bt709-limited'
    a = yf.yuv_clip(seed=61, t=3, h=64, w=96)
    frames = yf.batch_views(a)
    rgb = ops.frames_from_yuv420(frames, std, chroma=mode)
    ref = fwd(m, rgb, a)
    assert float(ref.min()) < 0.0 and float(ref.max()) > 1.0
    got = fwd(m, frames, a, yuv_standard=std, chroma=mode)
    assert torch.equal(got, ref)
    refy = ops.frames_to_yuv420(ref, std, 'nv12', chroma=mode)[0]
    goty = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype='nv12')
    assert goty.dtype == torch.uint8 and goty.shape == (1, 3, 96, 96) and torch.equal(goty, refy)
    both = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype=(torch.float32, 'i420'))
    assert torch.equal(both[0], ref) and torch.equal(both[1], ops.frames_to_yuv420(ref, std, 'i420', chroma=mode)[0])
    # the default is the call without the argument, and the mode matters on both sides
    plain = fwd(m, frames, a, yuv_standard=std)
    assert torch.equal(fwd(m, frames, a, yuv_standard=std, chroma='replicate'), plain)
    assert torch.equal(plain, fwd(m, ops.frames_from_yuv420(frames, std), a)) and not torch.equal(got, plain)
    assert not torch.equal(refy, ops.frames_to_yuv420(ref, std, 'nv12')[0])
    # forward_clips by pointer
    clips = [(a['planes'][0].views, a['QPs'][0], a['slices'][0], a['mvs'][0], a['base_QPs'][0], a['partitions'][0])]
    with torch.no_grad():
        out = m.forward_clips(clips, out_dtype=(torch.float32, 'nv12'), yuv_standard=std, chroma=mode)
    assert torch.equal(out[0][0], ref) and torch.equal(out[0][1], refy)
    assert torch.equal(a['planes'][0].flat.cpu(), a['planes'][0].expect(*a['bytes'][0]))
    with pytest.raises(ValueError, match='chroma'):
        fwd(m, frames, a, chroma='top-left')


def test_forward_on_10_bit_planes_in_a_sited_mode():
    m, std, mode = model(), 'bt601-limited', 'left'
    a = y16.clip16(seed=62, depth=10, msb=True, order='nv12', t=3, h=64, w=96)
    frames = y16.batch_views(a)
    ref = fwd(m, ops.frames_from_yuv420p16(frames, std, chroma=mode), a)
    assert torch.equal(fwd(m, frames, a, yuv_standard=std, chroma=mode), ref)
    assert not torch.equal(ref, fwd(m, frames, a, yuv_standard=std))
    got16 = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype='p010')
    assert torch.equal(got16, ops.frames_to_yuv420p16(ref, std, 'p010', chroma=mode)[0])
    got8 = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype='nv12')       # 8-bit planes of a 10-bit clip: made of the fp32 output
    assert torch.equal(got8, ops.frames_to_yuv420(ref, std, 'nv12', chroma=mode)[0])


def test_forward_x4_writes_sited_planes_of_the_large_frame():
    m, std, mode = model(vsr=True), 'bt601-limited', 'topleft'
    a = yf.yuv_clip(seed=63, t=3, h=64, w=96)
    frames = yf.batch_views(a)
    ref = fwd(m, ops.frames_from_yuv420(frames, std, chroma=mode), a)
    assert ref.shape == (1, 3, 3, 256, 384)
    f32, planes = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype=(torch.float32, 'nv12'))
    assert torch.equal(f32, ref) and planes.shape == (1, 3, 384, 384)
    assert torch.equal(planes, ops.frames_to_yuv420(ref, std, 'nv12', chroma=mode)[0])


def test_a_graph_is_keyed_by_the_mode():
    std = 'bt601-limited'
    a = yf.yuv_clip(seed=64, t=3, h=64, w=96)
    frames = yf.batch_views(a)
    want = {mode: fwd(model(), frames, a, yuv_standard=std, chroma=mode, out_dtype=(torch.float32, 'nv12')) for mode in ('left', 'topleft', 'replicate')}
    assert not torch.equal(want['left'][0], want['topleft'][0]) and not torch.equal(want['left'][1], want['replicate'][1])
    g = yf.build(dict(num_blocks=2), seed=433, use_graphs=True)
    for mode in ('left', 'topleft', 'left', 'replicate', 'topleft'):
        got = fwd(g, frames, a, yuv_standard=std, chroma=mode, out_dtype=(torch.float32, 'nv12'))
        assert torch.equal(got[0], want[mode][0]) and torch.equal(got[1], want[mode][1]), mode
    assert len(g._graphs) == 3


# ------------------------------------------------------------------------------------------------ the restorer and the loop
def test_restorer_and_multi_gpu_test_on_a_left_sited_tree(tmp_path):
    import test_gpu_yuv_metrics as ym
    from pnp_vcve_amd import restorer      # noqa: F401
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    from pnp_vcve_amd.registry import build_model
    metrics = ['PSNR', 'SSIM', 'PSNR_U', 'PSNR_V', 'PSNR_YUV']
    lq, gt, qp = ym.write_yuv_tree(tmp_path / 'data', 'i420')
    ds = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=64, layout='i420', qp_slice_file=qp,
                            chroma='left'))
    assert len(ds) == 2 and ds[0]['meta']['chroma'] == 'left'
    gen_cfg = dict(yf.gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=2)
    net = build_model(dict(type='BasicVSR', generator=dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **gen_cfg)),
                      train_cfg=None, test_cfg=dict(metrics=metrics, crop_border=0))
    net.generator.load_state_dict(model().state_dict())
    net = net.to(dev()).eval()
    want, want_bytes, sited = [], {}, False
    for i in range(2):
        data = _to_device(collate([ds[i]]), dev())
        side = [data[k] for k in ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions')]
        with torch.no_grad():
            f32 = net.generator(data['lq'], *side, chroma='left')
            assert torch.equal(f32, net.generator(ops.frames_from_yuv420(data['lq'], 'bt601-limited', chroma='left'), *side))
            r = net(data['lq'], data['gt'], *side, test_mode=True, out_dtype='i420', chroma='left')
        packed, views = ops.frames_to_yuv420(f32, 'bt601-limited', 'i420', chroma='left')
        sited = sited or not torch.equal(packed, ops.frames_to_yuv420(f32, 'bt601-limited', 'i420')[0])
        want_bytes[ds.keys[i]] = packed[0].cpu().numpy().tobytes()
        want.append(net.evaluate(views, data['gt']))
        assert r['eval_result'] == want[-1] and all(np.isfinite(v) for v in want[-1].values())
    assert sited
    asked = []
    orig = net.generator.forward_clips

    def spy(clips, out_dtype=None, **kw):
        asked.append((len(clips), out_dtype, kw))
        return orig(clips, out_dtype=out_dtype, **kw)

    net.generator.forward_clips = spy
    for cif in (1, 2):
        save = tmp_path / f'out{cif}'
        got = multi_gpu_test(net, ds, save_image=True, save_path=str(save), device=dev(), metrics=tuple(metrics), clips_in_flight=cif,
                             yuv_frames=True, yuv_out_layout='i420')
        assert [r['eval_result'] for r in got] == want, cif
        assert sorted(os.listdir(save)) == ['000.yuv', '011.yuv']
        for clip, b in want_bytes.items():
            with open(save / f'{clip}.yuv', 'rb') as fh:
                assert fh.read() == b, (cif, clip)
    assert asked == [(2, 'i420', dict(yuv_standard='bt601-limited', chroma='left'))]
