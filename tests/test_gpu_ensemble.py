"""GPU: the self-ensemble (include/pnpvcve.h, "Self-ensemble") -- the two kernels against tests/ensemble_ref.py by torch.equal,
generator.forward_ensemble against the composition it is defined as (ensemble_ref's views, generator.forward one variant at a time,
a sequential sum), the symmetrised network on the device, and the restorer / test-loop plumbing.

Sizes: 64x80 (2.5 tiles of 32 wide), 66x79 (odd: uint8 rows at odd addresses; any_size) and 64x64 (one orientation)."""
import ctypes

import pytest
import torch

import ensemble_ref as er
import golden_util as gu
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
KEYS = ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions')
T4, T3 = [73, 66, 80, 66], [73, 66, 66]
GUARD = 4096        # bytes


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def poison(shape, dtype=torch.float32):
    """leave a NaN-filled (0xA5-filled) block of the output's size on top of the caching allocator's free list: the wrapper's
    torch.empty of that size takes it, so an element the kernels skip shows"""
    x = torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda') if dtype == torch.uint8 else torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    del x


def raw_clip(h, w, t=4, seed=11):
    """random frames, vectors and planes (t,...) on the device: every element distinct enough that a misplaced one shows"""
    g = torch.Generator().manual_seed(seed)
    return dict(lq=torch.rand(t, 3, h, w, generator=g).to(dev()), u8=torch.randint(0, 256, (t, h, w, 3), generator=g, dtype=torch.uint8).to(dev()),
                mvs=(torch.rand(t, 4, h, w, generator=g) * 16 - 8).to(dev()), par=torch.rand(t, 3, h, w, generator=g).to(dev()))


def make_clip(h, w, t, n=1, seed=7):
    c = gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=T4 if t == 4 else T3, crf=[15, 35][:n] if n > 1 else 25)
    return {k: torch.from_numpy(c[k]).to(dev()) for k in KEYS}


def build(precision='fp32', sd=None, num_blocks=2, **over):
    from pnp_vcve_amd.registry import build_backbone
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=num_blocks, **over)
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    if sd is None:
        sd = {k: torch.from_numpy(v.copy()) for k, v in gu.syn.make_state_dict(cfg, seed=300, par_gain=10.0).items()}
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    if precision != 'fp32':
        m.precision = precision
    return m


# ------------------------------------------------------------------------------------------------ ops.ensemble_view
@pytest.mark.parametrize('hw', [(64, 80), (66, 79)], ids=lambda hw: f'{hw[0]}x{hw[1]}')
@pytest.mark.parametrize('byte', [False, True], ids=['fp32', 'uint8'])
def test_view_equals_the_reference_for_all_16_variants(hw, byte):
    h, w = hw
    c = raw_clip(h, w)
    lq = c['u8'] if byte else c['lq']
    for v in ops.ENSEMBLE_SPATIAL_TEMPORAL:
        ho, wo = (w, h) if v & 4 else (h, w)
        poison((4, ho, wo, 3), torch.uint8) if byte else poison((4, 3, ho, wo))
        poison((4, 4, ho, wo))
        poison((4, 3, ho, wo))
        lq_v, mv_v, par_v = ops.ensemble_view(lq, c['mvs'], c['par'], v)
        assert lq_v.dtype == lq.dtype and torch.equal(lq_v, er.view_frames(lq, v)), v
        assert torch.equal(mv_v, er.view_mvs(c['mvs'], v)), v
        assert torch.equal(par_v, er.view_planes(c['par'], v)), v
        if v:
            assert not torch.equal(mv_v, er.view_mvs(c['mvs'], v, wrong=True)), v
    assert ops.ENSEMBLE_SPATIAL == tuple(range(8)) and ops.ENSEMBLE_SPATIAL_TEMPORAL == tuple(range(16))


def test_view_null_pairs_ranks_and_refusals():
    c = raw_clip(66, 79, t=3)
    for v in (3, 6, 13):
        for present in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):
            for lq in (c['lq'], c['u8']):
                args = [x if on else None for x, on in zip((lq, c['mvs'], c['par']), present)]
                got = ops.ensemble_view(*args, v)
                want = (er.view_frames(lq, v), er.view_mvs(c['mvs'], v), er.view_planes(c['par'], v))
                for g, wnt, on in zip(got, want, present):
                    assert (g is None) if not on else torch.equal(g, wnt), (v, present)
    assert ops.ensemble_view(None, None, None, 5) == (None, None, None)
    # 5-D with n = 1 in, 5-D out
    lq5, mv5, par5 = ops.ensemble_view(c['u8'][None], c['mvs'][None], c['par'], 6)
    assert lq5.shape == (1, 3, 79, 66, 3) and mv5.shape == (1, 3, 4, 79, 66) and par5.shape == (3, 3, 79, 66)
    assert torch.equal(lq5[0], er.view_frames(c['u8'], 6)) and torch.equal(mv5[0], er.view_mvs(c['mvs'], 6))
    with pytest.raises(RuntimeError):
        ops.ensemble_view(c['lq'].cpu(), None, None, 1)
    with pytest.raises(ValueError):
        ops.ensemble_view(c['lq'], c['mvs'], c['par'], 16)
    with pytest.raises(ValueError):
        ops.ensemble_view(c['lq'], c['mvs'][:, :, :64], None, 1)
    with pytest.raises(ValueError):
        ops.ensemble_view(torch.cat([c['lq'][None]] * 2), None, None, 1)
    # ops.ensemble_side: plain torch
    qp = torch.arange(3.0).view(1, 3, 1, 1, 1)
    for v in (0, 7, 8, 15):
        a, b, none = ops.ensemble_side(qp, qp[0], None, v)
        assert none is None and torch.equal(a[0], er.view_side(qp[0], v)) and torch.equal(b, er.view_side(qp[0], v))


def guarded(nbytes, fill=0xA5):
    """a poisoned uint8 allocation with `nbytes` (rounded up to a dword) between two 4 KB guard bands -> (buffer, payload address)"""
    n = (nbytes + 3) // 4 * 4
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8, device=dev())
    return buf, buf.data_ptr() + GUARD


def bands_untouched(buf, nbytes, fill=0xA5):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + nbytes:] == fill).all())


@pytest.mark.parametrize('byte', [False, True], ids=['fp32', 'uint8'])
def test_c_abi_view_writes_its_outputs_and_nothing_else(byte):
    t, h, w = 3, 66, 79
    c = raw_clip(h, w, t=t, seed=12)
    lq = c['u8'] if byte else c['lq']
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sizes = (lq.numel() * lq.element_size(), c['mvs'].numel() * 4, c['par'].numel() * 4)
    for v in (0, 2, 5, 7, 9, 14):
        bufs = [guarded(s) for s in sizes]
        rc = L.pnp_ensemble_view(lq.data_ptr(), c['mvs'].data_ptr(), c['par'].data_ptr(), bufs[0][1], bufs[1][1], bufs[2][1],
                                 _native.FRAMES_U8_HWC if byte else _native.FRAMES_F32_NCHW, t, h, w, v, st)
        assert rc == 0, (v, rc)
        torch.cuda.synchronize()
        want = (er.view_frames(lq, v), er.view_mvs(c['mvs'], v), er.view_planes(c['par'], v))
        for (buf, _), s, wnt in zip(bufs, sizes, want):
            assert bands_untouched(buf, s), v
            assert torch.equal(buf[GUARD:GUARD + s], wnt.reshape(-1).view(torch.uint8)), v      # bytes: -0.0 must not appear where nothing is negated
        # one pair alone: the other outputs are not touched at all
        bufs = [guarded(s) for s in sizes]
        assert L.pnp_ensemble_view(None, c['mvs'].data_ptr(), None, None, bufs[1][1], None, 0, t, h, w, v, st) == 0
        torch.cuda.synchronize()
        assert bool((bufs[0][0] == 0xA5).all()) and bool((bufs[2][0] == 0xA5).all()) and bands_untouched(bufs[1][0], sizes[1])
        assert torch.equal(bufs[1][0][GUARD:GUARD + sizes[1]].view(torch.float32), want[1].reshape(-1))


def test_c_abi_accumulate_writes_acc_and_nothing_else():
    t, ch, H, W = 2, 3, 66, 79
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(13)
    n = t * ch * H * W * 4
    for v in (0, 3, 4, 6, 13):
        x = torch.rand((t, ch, W, H) if v & 4 else (t, ch, H, W), generator=g).to(dev())
        x_before = x.clone()
        buf, p = guarded(n)
        assert L.pnp_ensemble_accumulate_f32(x.data_ptr(), p, t, ch, H, W, v, 1, 1.0, st) == 0       # first: acc's poison is not read
        torch.cuda.synchronize()
        acc = buf[GUARD:GUARD + n].view(torch.float32).view(t, ch, H, W)
        assert bands_untouched(buf, n) and torch.equal(acc, er.inverse(x, v)), v
        prev = acc.clone()
        assert L.pnp_ensemble_accumulate_f32(x.data_ptr(), p, t, ch, H, W, v, 0, 0.125, st) == 0
        torch.cuda.synchronize()
        assert bands_untouched(buf, n) and torch.equal(acc, (prev + er.inverse(x, v)) * 0.125), v
        assert torch.equal(x, x_before)


# ------------------------------------------------------------------------------------------------ ops.ensemble_accumulate
@pytest.mark.parametrize('v', [2, 5, 11, 14])
def test_accumulate_first_middle_and_scaled_last_step(v):
    t, c, H, W = 4, 3, 64, 80
    g = torch.Generator().manual_seed(20 + v)
    xs = [torch.randn((t, c, W, H) if v & 4 else (t, c, H, W), generator=g).to(dev()) for _ in range(3)]
    acc = torch.full((t, c, H, W), float('nan'), device=dev())
    assert ops.ensemble_accumulate(acc, xs[0], v, first=True) is acc
    want = er.inverse(xs[0], v)
    assert torch.equal(acc, want)
    ops.ensemble_accumulate(acc, xs[1], v, first=False)
    want = want + er.inverse(xs[1], v)
    assert torch.equal(acc, want)
    ops.ensemble_accumulate(acc[None], xs[2][None], v, first=False, scale=1.0 / 8)          # 5-D with n = 1: the same storage
    want = (want + er.inverse(xs[2], v)) * (1.0 / 8)
    assert torch.equal(acc, want)
    ops.ensemble_accumulate(acc, xs[0], v, first=True, scale=0.5)
    assert torch.equal(acc, er.inverse(xs[0], v) * 0.5)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            ops.ensemble_accumulate(acc, xs[0], v, first=True, scale=bad)
    with pytest.raises(ValueError):
        ops.ensemble_accumulate(acc, xs[0][:, :, 1:], v, first=True)
    with pytest.raises(RuntimeError):
        ops.ensemble_accumulate(acc.cpu(), xs[0], v, first=True)


# ------------------------------------------------------------------------------------------------ forward_ensemble == the composition
def compose(m, a, temporal):
    """the Definition with generator.forward: ensemble_ref's views, one variant per call, a sequential sum, one scaling"""
    variants = er.SPATIAL_TEMPORAL if temporal else er.SPATIAL
    outs = []
    for b in range(a['lq'].shape[0]):
        clip = {k: a[k][b] for k in KEYS}

        def run(cl):
            with torch.no_grad():
                return m(*(cl[k][None] for k in KEYS))[0]

        outs.append(er.ensemble(run, clip, variants))
    return torch.stack(outs)


def spy_groups(m):
    """record how many clips each forward_clips call of m gets"""
    sizes, inner = [], m.forward_clips

    def wrapped(clips, *args, **kw):
        clips = list(clips)
        sizes.append(len(clips))
        return inner(clips, *args, **kw)

    m.forward_clips = wrapped
    return sizes


@pytest.mark.parametrize('temporal', [False, True], ids=['spatial', 'spatial-temporal'])
def test_forward_ensemble_is_the_composition_fp32(temporal):
    m = build()
    a = make_clip(64, 80, 4)
    want = compose(m, a, temporal)
    sizes = spy_groups(m)
    poison(tuple(want.shape))
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS), temporal=temporal)
    assert got.dtype == torch.float32 and got.shape == want.shape == (1, 4, 3, 64, 80)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert sizes == [4] * (4 if temporal else 2)                # 64x80: groups of one orientation
    with torch.no_grad():
        plain = m(*(a[k] for k in KEYS))
    assert not torch.equal(got, plain) and float((got - plain).abs().max()) < 0.5      # an average of 8 different runs, of the same clip


@pytest.mark.parametrize('out_dtype', [torch.uint8, 'both'], ids=['uint8', 'both'])
def test_forward_ensemble_byte_frames(out_dtype):
    m = build()
    a = make_clip(64, 80, 4)
    a['lq'] = ops.frames_to_rgb8(a['lq'][0])[None]              # (1,t,h,w,3) uint8
    want = compose(m, a, False)
    want8 = ops.frames_to_rgb8(want[0])[None]
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS), out_dtype=out_dtype)
    if out_dtype == 'both':
        assert isinstance(got, tuple) and torch.equal(got[0], want) and torch.equal(got[1], want8)
    else:
        assert got.dtype == torch.uint8 and got.shape == (1, 4, 64, 80, 3) and torch.equal(got, want8)
    # the same bytes and planes from the fp32 form of the same frames
    a32 = dict(a, lq=ops.frames_from_rgb8(a['lq']))
    with torch.no_grad():
        assert torch.equal(m.forward_ensemble(*(a32[k] for k in KEYS)), want)


def test_forward_ensemble_batch_of_two():
    m = build()
    a = make_clip(64, 80, 4, n=2)
    want = compose(m, a, False)
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS))
    assert got.shape == (2, 4, 3, 64, 80) and torch.equal(got, want)
    assert not torch.equal(got[0], got[1])


def test_forward_ensemble_fp16():
    m = build(precision='fp16')
    a = make_clip(64, 80, 4)
    want = compose(m, a, False)
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS))
    assert torch.equal(got, want), float((got - want).abs().max())


def test_forward_ensemble_vsr_square_frame_one_group():
    m = build(vsr=True)
    a = make_clip(64, 64, 3)
    want = compose(m, a, False)
    sizes = spy_groups(m)
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS))
    assert got.shape == (1, 3, 3, 256, 256) and torch.equal(got, want)
    assert sizes == [8]                                         # h == w: all 8 variants in one call


def test_forward_ensemble_square_frame_temporal_two_groups_of_eight():
    m = build()
    a = make_clip(64, 64, 3)
    want = compose(m, a, True)
    sizes = spy_groups(m)
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS), temporal=True)
    assert torch.equal(got, want) and sizes == [8, 8]


def test_forward_ensemble_any_size():
    m = build()
    a = make_clip(66, 79, 4)
    with pytest.raises(ValueError):                             # forward's own rule, at the first variant
        m.forward_ensemble(*(a[k] for k in KEYS))
    m.any_size = True
    want = compose(m, a, False)
    with torch.no_grad():
        got = m.forward_ensemble(*(a[k] for k in KEYS))
    assert got.shape == (1, 4, 3, 66, 79) and torch.equal(got, want)
    u8 = dict(a, lq=ops.frames_to_rgb8(a['lq'][0])[None])        # rows of 237 bytes: odd addresses
    with torch.no_grad():
        assert torch.equal(m.forward_ensemble(*(u8[k] for k in KEYS)), compose(m, u8, False))


def test_symmetrised_weights_ensemble_equals_the_plain_forward():
    """every 3x3 kernel symmetrised: the network is equivariant, all 8 variants compute the same function and their mean is the plain
    forward up to the kernels' rounding -- 5e-6, the project's fp32 gate (measured 2.4e-7; the clip's residual out - lq is 7.4e-2)"""
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG)
    sd = er.symmetrise_3x3({k: torch.from_numpy(v.copy()) for k, v in gu.syn.make_state_dict(cfg, seed=300, par_gain=10.0).items()})
    m = build(sd=sd, num_blocks=cfg['num_blocks'])
    a = make_clip(64, 80, 4)
    with torch.no_grad():
        plain = m(*(a[k] for k in KEYS))
        got = m.forward_ensemble(*(a[k] for k in KEYS), temporal=False)
    d = float((got - plain).abs().max())
    print(f'symmetrised weights: max|ensemble - forward| = {d:.3e}; residual {float((plain - a["lq"]).abs().max()):.3e}')
    assert d <= 5e-6, d


def test_forward_ensemble_refusals():
    m = build()
    a = make_clip(64, 64, 3)
    y = torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=dev())
    cbcr = torch.zeros(1, 3, 32, 32, dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError):
        m.forward_ensemble(ops.Yuv420Frames(y, cbcr, cbcr.clone()), *(a[k] for k in KEYS[1:]))
    with pytest.raises(ValueError):
        m.forward_ensemble(*(a[k] for k in KEYS), out_dtype='i420')
    with pytest.raises(RuntimeError):
        m.forward_ensemble(*(a[k].cpu() for k in KEYS))
    basic = build(deform='basic')
    with pytest.raises(ValueError):
        basic.forward_ensemble(*(a[k] for k in KEYS))


# ------------------------------------------------------------------------------------------------ restorer and test loop
def build_restorer(ensemble, metrics=('PSNR', 'SSIM')):
    from pnp_vcve_amd import restorer  # noqa: F401
    from pnp_vcve_amd.registry import build_model
    gcfg = dict(gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=2)
    torch.manual_seed(0)
    model = build_model(dict(type='BasicVSR', generator=dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **gcfg),
                             pixel_loss=dict(type='CharbonnierLoss'), ensemble=ensemble), train_cfg=None,
                        test_cfg=dict(metrics=list(metrics), crop_border=0) if metrics else None)
    return model.to(dev()).eval()


@pytest.mark.parametrize('temporal', [False, True], ids=['spatial', 'spatial-temporal'])
def test_restorer_forward_test_runs_the_ensemble(temporal):
    model = build_restorer(dict(type='SpatialTemporalEnsemble', is_temporal_ensemble=temporal))
    assert model.forward_ensemble is not None and model.is_temporal_ensemble is temporal
    c = gu.syn.make_clip(seed=7, n=1, t=4, h=64, w=80, slices=T4)
    a = {k: torch.from_numpy(c[k]).to(dev()) for k in KEYS}
    gt = torch.from_numpy(c['gt']).to(dev())
    with torch.no_grad():
        want = model.generator.forward_ensemble(*(a[k] for k in KEYS), temporal=temporal)
        res = model(test_mode=True, gt=gt, lq=a['lq'], QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'], partitions=a['partitions'])
    assert res['eval_result'] == model.evaluate(want, gt)
    assert model.last_forward_seconds is not None and model.last_forward_seconds > 0
    plain = build_restorer(None)
    plain.generator.load_state_dict(model.generator.state_dict())
    with torch.no_grad():
        res0 = plain(test_mode=True, gt=gt, lq=a['lq'], QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'], partitions=a['partitions'])
    assert res0['eval_result'] != res['eval_result']
    # out_dtype is passed through; a precomputed output is taken as it is
    a8 = dict(a, lq=ops.frames_to_rgb8(a['lq'][0])[None])
    gt8 = ops.frames_to_rgb8(gt[0])[None]
    with torch.no_grad():
        want8 = model.generator.forward_ensemble(*(a8[k] for k in KEYS), temporal=temporal, out_dtype=torch.uint8)
        res8 = model(test_mode=True, gt=gt8, lq=a8['lq'], QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'],
                     partitions=a['partitions'], out_dtype=torch.uint8)
        pre = model(test_mode=True, gt=gt8, lq=a8['lq'], QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'],
                    partitions=a['partitions'], out_dtype=torch.uint8, precomputed_output=want8)
    assert want8.dtype == torch.uint8 and res8['eval_result'] == model.evaluate(want8, gt8) == pre['eval_result']


def test_restorer_refusals():
    with pytest.raises(NotImplementedError, match=r'Currently support only "SpatialTemporalEnsemble", but got type \[Nope\]'):
        build_restorer(dict(type='Nope'))
    model = build_restorer(dict(type='SpatialTemporalEnsemble'))
    assert model.is_temporal_ensemble is False
    a = make_clip(64, 64, 3)
    y = torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=dev())
    cbcr = torch.zeros(1, 3, 32, 32, dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError):
        model(test_mode=True, lq=ops.Yuv420Frames(y, cbcr, cbcr.clone()), QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'],
              partitions=a['partitions'], out_dtype='i420')
    with pytest.raises(ValueError):
        model(test_mode=True, lq=ops.Yuv420Frames(y, cbcr, cbcr.clone()), QPs=a['QPs'], slices=a['slices'], mvs=a['mvs'], base_QPs=a['base_QPs'],
              partitions=a['partitions'])


def test_multi_gpu_test_runs_an_ensemble_model_clip_by_clip(tmp_path):
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    lq, gt, qp = gu.syn.write_clip_tree(str(tmp_path / 'data'), clips=['000', '011'], t=4, h=64, w=80, seed=3)
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    assert len(ds) == 2
    model = build_restorer(dict(type='SpatialTemporalEnsemble'), metrics=('PSNR',))
    sizes = spy_groups(model.generator)
    two = multi_gpu_test(model, ds, device='cuda', metrics=('PSNR',), clips_in_flight=2)
    assert sizes == [4, 4, 4, 4]                                # two clips, each its own 8 variants: never paired
    one = []
    for i in range(2):                                          # clip by clip, the model called directly
        data = _to_device(collate([ds[i]]), dev())
        with torch.no_grad():
            one.append(model(test_mode=True, **data)['eval_result']['PSNR'])
    assert [r['eval_result']['PSNR'] for r in two] == one and one[0] != one[1]
    assert all(r['frames_per_s'] > 0 for r in two)
    for kw in (dict(byte_frames=True), dict(byte_metrics=True)):
        got = multi_gpu_test(model, ds, device='cuda', metrics=('PSNR',), clips_in_flight=2, **kw)
        assert [r['eval_result']['PSNR'] for r in got] == one, kw
    with pytest.raises(ValueError):
        multi_gpu_test(model, ds, device='cuda', metrics=('PSNR',), yuv_frames=True)
