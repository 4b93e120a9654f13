"""GPU: the byte-frame boundary.  uint8 HWC frames in, uint8 HWC frames out, clips passed by pointer -- everything new is a
composition of things that exist (ops.frames_from_rgb8 in front of the fp32 forward, ops.frames_to_rgb8 behind it, torch.cat of the
clips), so every check is torch.equal: no tolerance anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions')


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def build(cfg_over=None, seed=300, precision='fp32', **attrs):
    from pnp_vcve_amd.registry import build_backbone
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG)
    cfg.update(cfg_over or {})
    sd = gu.syn.make_state_dict(cfg, seed=seed, par_gain=10.0)
    # a residual of both signs and some size whatever the seed (conv_last's output is added to the frame): outputs below 0 and above 1
    sd['conv_last.weight'] = sd['conv_last.weight'] * 6.0
    sd['conv_last.bias'] = np.zeros_like(sd['conv_last.bias'])
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    if precision != 'fp32':
        m.precision = precision
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def byte_clip(seed, n=1, t=7, h=128, w=128, slices='IBBBP'):
    """side info of a synthetic clip + decoder-like bytes: smooth content with a third of the pixels at 0 or 255, so that conv_last's
    residual pushes outputs below 0 and above 1 and the clamp of the byte output has work to do"""
    c = gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=slices, qp_mode='qp', crf=[15, 35, 25, 30, 20, 40, 22, 33][:n] if n > 1 else 25)
    a = {k: torch.from_numpy(c[k]).to(dev()) for k in SIDE}
    g = torch.Generator(device='cuda').manual_seed(seed)
    u8 = torch.randint(0, 256, (n, t, h, w, 3), device='cuda', generator=g, dtype=torch.uint8)
    r = torch.rand((n, t, h, w, 1), device='cuda', generator=g)
    u8 = torch.where(r < 1 / 6, torch.zeros_like(u8), torch.where(r > 5 / 6, torch.full_like(u8, 255), u8))
    a['lq_u8'] = u8.contiguous()
    return a


def fwd(m, lq, a, **kw):
    with torch.no_grad():
        return m(lq, a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'], **kw)


def poison(shape, dtype):
    """leave a block of the output's size, full of a poison byte, at the top of the caching allocator's free list: the forward's
    torch.empty of that size takes it"""
    x = torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda') if dtype == torch.uint8 else torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    del x


def to_rgb8(out):
    n, t = out.shape[:2]
    return ops.frames_to_rgb8(out.reshape((n * t,) + tuple(out.shape[2:]))).reshape(n, t, out.shape[3], out.shape[4], 3)


def check_boundary(m, a, label, replays=1):
    """input side: forward(u8) == forward(frames_from_rgb8(u8)); output side: uint8 == frames_to_rgb8(plain forward), from byte and
    from fp32 frames; 'both' == the pair"""
    u8 = a['lq_u8']
    planes = ops.frames_from_rgb8(u8)
    assert planes.shape == (u8.shape[0], u8.shape[1], 3, u8.shape[2], u8.shape[3])
    for _ in range(replays):
        ref = fwd(m, planes, a).clone()
    ref8 = to_rgb8(ref)
    lo, hi = float(ref.min()), float(ref.max())
    print(f'{label}: plain output in [{lo:.3f}, {hi:.3f}]')
    assert lo < 0.0 and hi > 1.0, (label, lo, hi)                   # the clamp is exercised
    assert int(ref8.min()) == 0 and int(ref8.max()) == 255
    s = 4 if m.vsr else 1
    n, t, h, w = u8.shape[:4]
    for _ in range(replays):
        poison((n, t, 3, h * s, w * s), torch.float32)
        got = fwd(m, u8, a)
    assert got.dtype == torch.float32 and torch.equal(got, ref), (label, 'byte in')
    for name, lq in (('byte in', u8), ('fp32 in', planes)):
        for _ in range(replays):
            poison((n, t, h * s, w * s, 3), torch.uint8)
            got8 = fwd(m, lq, a, out_dtype=torch.uint8)
        assert got8.dtype == torch.uint8 and got8.shape == (n, t, h * s, w * s, 3)
        assert torch.equal(got8, ref8), (label, name, 'uint8 out', int((got8 != ref8).sum()))
    for _ in range(replays):
        poison((n, t, 3, h * s, w * s), torch.float32)
        poison((n, t, h * s, w * s, 3), torch.uint8)
        both = fwd(m, u8, a, out_dtype='both')
    assert isinstance(both, tuple) and len(both) == 2
    assert torch.equal(both[0], ref) and torch.equal(both[1], ref8), (label, 'both')
    assert torch.equal(fwd(m, planes, a, out_dtype=torch.float32), ref)
    return ref, ref8


# ------------------------------------------------------------------------------------------------ the stand-alone op
def test_frames_from_rgb8_is_the_ieee_division_of_all_256_values():
    v = torch.arange(256, dtype=torch.uint8).repeat(3)[:, None].expand(768, 3).reshape(1, 16, 48, 3).contiguous().to(dev())
    got = ops.frames_from_rgb8(v)
    assert got.shape == (1, 3, 16, 48) and got.dtype == torch.float32
    want = (torch.arange(256, dtype=torch.float32) / 255.0)
    want_np = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255))
    assert torch.equal(want, want_np)
    flat = got.cpu().permute(0, 2, 3, 1).reshape(-1, 3)
    idx = v.cpu().reshape(-1, 3).long()
    assert torch.equal(flat, want[idx]) and torch.equal(flat, want_np[idx])
    assert set(idx[:, 0].tolist()) == set(range(256))
    assert torch.equal(torch.ops.pnpvcve.frames_from_rgb8(v), got)


def test_frames_from_rgb8_matches_the_loaders_device_branch_on_a_ragged_clip():
    from pnp_vcve_amd.apis import _to_device
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (1, 5, 100, 132, 3), generator=g, dtype=torch.uint8)
    ref = _to_device({'lq_u8': u8.clone()}, dev())['lq']              # the present branch: a table lookup per frame
    got = ops.frames_from_rgb8(u8.to(dev()))
    assert got.shape == ref.shape == (1, 5, 3, 100, 132) and torch.equal(got, ref)
    # and the byte branch of the same function: lq stays the bytes, gt becomes planes
    byte = _to_device({'lq_u8': u8.clone(), 'gt_u8': u8.clone()}, dev(), byte_frames=True)
    assert byte['lq'].dtype == torch.uint8 and torch.equal(byte['lq'].cpu(), u8) and torch.equal(byte['gt'], ref)
    # round trip: bytes -> planes -> bytes
    assert torch.equal(ops.frames_to_rgb8(got[0]).cpu(), u8[0])
    with pytest.raises(TypeError):
        ops.frames_from_rgb8(got)
    with pytest.raises(ValueError):
        ops.frames_from_rgb8(torch.zeros(4, 8, 8, 4, dtype=torch.uint8, device=dev()))


# ------------------------------------------------------------------------------------------------ shapes
SHAPES = [('s128_t7', dict(t=7, h=128, w=128)), ('s180x320_t5', dict(t=5, h=180, w=320)), ('s192x256_n2', dict(n=2, t=4, h=192, w=256))]


@pytest.mark.parametrize('name,kw', SHAPES, ids=[s[0] for s in SHAPES])
def test_byte_boundary_shapes(name, kw):
    m = build()
    check_boundary(m, byte_clip(seed=11 + len(name), **kw), name)


def test_byte_boundary_720p_bench_clip_with_band_chains():
    m = build()
    assert m.band_split == 1
    check_boundary(m, byte_clip(seed=21, t=7, h=720, w=1280), '720p_t7')


# ------------------------------------------------------------------------------------------------ modes
def _mode_cases():
    W = _native.OPT_WINOGRAD
    return [
        ('graphs', {}, dict(use_graphs=True), {}, dict(t=5, h=128, w=128), 2),
        ('graphs_n2', {}, dict(use_graphs=True), {}, dict(n=2, t=3, h=64, w=96), 2),
        ('bounded_min', {}, {}, {}, dict(t=11, h=64, w=96), 1),
        ('fp16', {}, dict(precision='fp16'), {}, dict(t=5, h=128, w=128), 1),
        ('fp16_n2', {}, dict(precision='fp16'), {}, dict(n=2, t=3, h=64, w=96), 1),
        ('f16x3', {}, dict(precision='f16x3'), {}, dict(t=5, h=128, w=128), 1),
        ('wino0', {}, {}, {W: 0}, dict(t=5, h=128, w=128), 1),
        ('wino2', {}, {}, {W: 2}, dict(t=5, h=128, w=128), 1),
        ('mfma_last', {}, {}, {_native.OPT_CONV_LAST_VALU: 0}, dict(t=5, h=128, w=128), 1),
        ('mfma_last_n2', {}, {}, {_native.OPT_CONV_LAST_VALU: 0}, dict(n=2, t=3, h=64, w=96), 1),
        ('vsr_180x320', dict(vsr=True, num_blocks=2), {}, {}, dict(t=3, h=180, w=320), 1),
        ('vsr_fp16', dict(vsr=True, num_blocks=2), dict(precision='fp16'), {}, dict(t=3, h=64, w=96), 1),
        ('vsr_mfma_last', dict(vsr=True, num_blocks=2), {}, {_native.OPT_CONV_LAST_VALU: 0}, dict(t=3, h=64, w=96), 1),
        ('basic', dict(deform='basic', num_blocks=2), {}, {}, dict(t=5, h=64, w=96), 1),
        ('sparse_val', dict(sparse_val=True), {}, {}, dict(t=5, h=64, w=96), 1),
        ('sparse_val_bounded', dict(sparse_val=True), {}, {}, dict(t=11, h=64, w=96), 1),
    ]


@pytest.mark.parametrize('case', _mode_cases(), ids=[c[0] for c in _mode_cases()])
def test_byte_boundary_modes(case):
    name, cfg_over, attrs, opts, kw, replays = case
    precision = attrs.pop('precision', 'fp32')
    m = build(cfg_over, seed=310 + len(name), precision=precision, **attrs)
    for o, v in opts.items():
        m.set_option(o, v)
    if 'bounded' in name:
        m.max_resident_features = m.min_resident_features(kw['t'])
        assert m.max_resident_features < kw['t']
    ref, _ = check_boundary(m, byte_clip(seed=31 + len(name), **kw), name, replays=replays)
    if name == 'vsr_180x320':
        assert ref.shape[-2:] == (720, 1280)


def test_layout_and_dtype_errors():
    m = build()
    a = byte_clip(seed=5, t=3, h=64, w=64)
    with pytest.raises(ValueError, match=r'\(n,t,h,w,3\)'):
        fwd(m, a['lq_u8'].permute(0, 1, 4, 2, 3).contiguous(), a)            # uint8 planes: not the decoder's layout
    with pytest.raises(ValueError, match=r'\(n,t,h,w,3\)'):
        fwd(m, a['lq_u8'][0], a)
    with pytest.raises(ValueError, match='out_dtype'):
        fwd(m, a['lq_u8'], a, out_dtype=torch.float16)
    small = byte_clip(seed=5, t=3, h=64, w=64)
    small['lq_u8'] = small['lq_u8'][:, :, :60].contiguous()
    with pytest.raises(AssertionError, match='at least 64'):
        fwd(m, small['lq_u8'], small)
    odd = byte_clip(seed=5, t=3, h=64, w=64)
    odd['lq_u8'] = torch.zeros(1, 3, 66, 64, 3, dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError):
        fwd(m, odd['lq_u8'], odd)                                             # maps of another size / a size that is not a multiple of 4
    with pytest.raises(TypeError):
        with torch.no_grad():
            m(a['lq_u8'], a['QPs'], None, a['mvs'], a['base_QPs'], a['partitions'])


# ------------------------------------------------------------------------------------------------ clips by pointer
def _split(a, i):
    return tuple(a[k][i:i + 1].clone() for k in ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions'))


@pytest.mark.parametrize('name,kw', [('two_128', dict(n=2, t=5, h=128, w=128)), ('three_64x96', dict(n=3, t=4, h=64, w=96)),
                                     ('eight_contexts_128', dict(n=8, t=3, h=128, w=128)), ('two_720p', dict(n=2, t=3, h=720, w=1280))],
                         ids=['two_128', 'three_64x96', 'eight_contexts_128', 'two_720p'])
def test_forward_clips_equals_forward_on_the_concatenation(name, kw):
    m = build()
    a = byte_clip(seed=41 + len(name), **kw)
    n = kw['n']
    for lq_key in ('planes', 'lq_u8'):
        a['lq'] = ops.frames_from_rgb8(a['lq_u8']) if lq_key == 'planes' else a['lq_u8']
        ref = fwd(m, a['lq'], a).clone()
        ref8 = to_rgb8(ref)
        clips = [_split(a, i) for i in range(n)]                  # separately allocated copies: nothing is contiguous across clips
        outs = m.forward_clips(clips)
        assert len(outs) == n and all(o.shape == ref[i:i + 1].shape for i, o in enumerate(outs))
        assert all(torch.equal(o, ref[i:i + 1]) for i, o in enumerate(outs)), (name, lq_key)
        outs8 = m.forward_clips(clips, out_dtype=torch.uint8)
        assert all(o.dtype == torch.uint8 and torch.equal(o, ref8[i:i + 1]) for i, o in enumerate(outs8)), (name, lq_key)
        both = m.forward_clips(clips, out_dtype='both')
        assert all(torch.equal(f, ref[i:i + 1]) and torch.equal(u, ref8[i:i + 1]) for i, (f, u) in enumerate(both)), (name, lq_key)
        # clips without the batch dimension
        bare = [tuple(x[0] for x in c) for c in clips]
        assert all(torch.equal(o, ref[i:i + 1]) for i, o in enumerate(m.forward_clips(bare)))
        if name == 'two_128':
            for _ in range(10):                                   # ten repeats identical
                again = m.forward_clips(clips, out_dtype='both')
                assert all(torch.equal(f, ref[i:i + 1]) and torch.equal(u, ref8[i:i + 1]) for i, (f, u) in enumerate(again))


def test_prefilled_outputs_are_completely_overwritten_on_the_abi_path():
    """buffers this test allocates and fills with a poison itself (0xA5 bytes, NaN planes), handed to ONE pnp_generator_forward_clips
    call as two separately allocated clips: each mask writes every element of what it asks for, and the values are the plain forward's"""
    m = build()
    a = byte_clip(seed=71, n=2, t=3, h=128, w=128)
    n, t, h, w = a['lq_u8'].shape[:4]
    ref = fwd(m, ops.frames_from_rgb8(a['lq_u8']), a).clone()
    ref8 = to_rgb8(ref)
    side = torch.stack([a['slices'].reshape(n, t).float(), a['QPs'].reshape(n, t).float(), a['base_QPs'].reshape(n, t).float()]).cpu().contiguous()
    lrs = [a['lq_u8'][i].clone() for i in range(n)]
    mvs = [a['mvs'][i].float().clone() for i in range(n)]
    par = [a['partitions'][i].float().clone() for i in range(n)]
    for mask in (1, 2, 3):
        f32 = [torch.full((t, 3, h, w), float('nan'), device=dev()) for _ in range(n)] if mask & 1 else None
        u8 = [torch.full((t, h, w, 3), 0xA5, dtype=torch.uint8, device=dev()) for _ in range(n)] if mask & 2 else None
        ws = torch.empty(2 * int(_native.lib().pnp_generator_workspace_bytes_io(m._handle, t, h, w, _native.FRAMES_U8_HWC, mask)),
                         dtype=torch.uint8, device=dev())
        m._launch_clips(lrs, mvs, par, side, f32, u8, ws, t, h, w)
        torch.cuda.synchronize()
        for i in range(n):
            if f32 is not None:
                assert not torch.isnan(f32[i]).any() and torch.equal(f32[i], ref[i]), (mask, i)
            if u8 is not None:
                assert torch.equal(u8[i], ref8[i]), (mask, i, int((u8[i] != ref8[i]).sum()))
    # a uint8 view at an odd storage offset is copied to an aligned buffer instead of surfacing as a bad-argument error
    flat = torch.empty(a['lq_u8'][0:1].numel() + 1, dtype=torch.uint8, device=dev())
    odd = flat[1:].view(a['lq_u8'][0:1].shape)
    odd.copy_(a['lq_u8'][0:1])
    assert odd.data_ptr() % 4 == 1
    one = {k: v[0:1] for k, v in a.items()}
    assert torch.equal(fwd(m, odd, one), ref[0:1])
    clip = (odd,) + tuple(one[k] for k in ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions'))
    assert torch.equal(m.forward_clips([clip])[0], ref[0:1])


def test_forward_clips_refuses_mixtures():
    m = build()
    a = byte_clip(seed=51, n=2, t=3, h=64, w=96)
    b = byte_clip(seed=52, n=1, t=3, h=64, w=64)
    a['lq'] = a['lq_u8']
    b['lq'] = b['lq_u8']
    c0, c1 = _split(a, 0), _split(a, 1)
    with pytest.raises(ValueError, match='agree'):
        m.forward_clips([c0, _split(b, 0)])                                  # shapes
    planes1 = (ops.frames_from_rgb8(c1[0]),) + c1[1:]
    with pytest.raises(ValueError, match='agree'):
        m.forward_clips([c0, planes1])                                       # uint8 with float frames
    with pytest.raises(ValueError):
        m.forward_clips([])
    with pytest.raises(ValueError):
        m.forward_clips([tuple(a[k] for k in ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions'))])      # a batch of two is not a clip
    with pytest.raises(ValueError, match='out_dtype'):
        m.forward_clips([c0], out_dtype='uint8')
    ms = build(dict(sparse_val=True))
    with pytest.raises(NotImplementedError):
        ms.forward_clips([c0, c1])


# ------------------------------------------------------------------------------------------------ memory
_MEM_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_byte_frames as T
from pnp_vcve_amd import _native
m = T.build()
t, h, w = 7, 720, 1280
a = T.byte_clip(seed=61, t=t, h=h, w=w)
m._ensure_packed(a['lq_u8'].device)
torch.cuda.synchronize()
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
out = T.fwd(m, a['lq_u8'], a, out_dtype=torch.uint8)
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated() - base
ws = int(_native.lib().pnp_generator_workspace_bytes_io(m._handle, t, h, w, _native.FRAMES_U8_HWC, _native.OUT_U8))
print('PEAK', peak, 'WS', ws, 'OUT', out.numel(), 'CLIP_F32', 12 * t * h * w)
'''


def test_no_clip_sized_fp32_frame_tensor_at_720p(tmp_path):
    """byte frames in, bytes out, 720p t = 7: what the forward allocates above its inputs is the workspace and the uint8 output; the
    rest (side info, the descriptor array's host memory is not device memory) stays below the size of ONE fp32 clip, 12*t*h*w bytes"""
    script = tmp_path / 'mem_child.py'
    script.write_text(_MEM_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    peak, ws, out, clip = (int(v) for v in re.search(r'PEAK (\d+) WS (\d+) OUT (\d+) CLIP_F32 (\d+)', r.stdout).groups())
    print(f'peak above the inputs {peak / 1e6:.1f} MB = workspace {ws / 1e6:.1f} MB + uint8 output {out / 1e6:.1f} MB + {(peak - ws - out) / 1e6:.1f} MB; '
          f'one fp32 clip is {clip / 1e6:.1f} MB')
    assert peak >= ws + out
    assert peak - ws - out < clip, (peak, ws, out, clip)


# ------------------------------------------------------------------------------------------------ the loop
def test_tools_test_byte_frames_prints_the_same_metrics_and_writes_the_same_pngs(tmp_path):
    """tools/test.py on an on-disk tree (PNG + MV-record decode, GPU rasteriser, PSNR / SSIM, PNG write-back): --byte-frames prints
    the default loop's PSNR and SSIM digit for digit and writes byte-identical PNGs, with one and with two clips in flight"""
    from pnp_vcve_amd import synthetic as syn
    lq, gt, qp = syn.write_clip_tree(str(tmp_path / 'data'), clips=['000', '011', '015'], t=5, h=72, w=104, seed=3)
    cfgp = tmp_path / 'folder_cfg.py'
    cfgp.write_text(
        f"_base_ = [{os.path.join(ROOT, 'configs', 'REDS_folder_example.py')!r}]\n"
        f"data = dict(test=dict(_delete_=True, type='SRREDSMultipleGTCompressDataset', lq_folder={lq!r}, gt_folder={gt!r},\n"
        f"                      num_input_frames=100, pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file={qp!r})], scale=1,\n"
        f"                      val_partition='REDS4', test_mode=True))\n")
    runs = {}
    for cif in ('1', '2'):
        for flag in ((), ('--byte-frames',)):
            save = tmp_path / f'out_{cif}_{len(flag)}'
            out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), str(cfgp), 'none', '--seed', '0', '--clips-in-flight', cif,
                                  '--save-path', str(save)] + list(flag), capture_output=True, text=True, timeout=900)
            assert out.returncode == 0, out.stdout + out.stderr
            pngs = {}
            for d, _, files in os.walk(save):
                for f in files:
                    with open(os.path.join(d, f), 'rb') as fh:
                        pngs[os.path.relpath(os.path.join(d, f), save)] = fh.read()
            runs[(cif, bool(flag))] = (re.search(r'Eval-PSNR: (\S+)', out.stdout).group(1), re.search(r'Eval-SSIM: (\S+)', out.stdout).group(1), pngs)
    base = runs[('1', False)]
    assert len(base[2]) == 15
    for key, (p, s, pngs) in runs.items():
        print(key, p, s, len(pngs))
        assert (p, s) == base[:2], (key, p, s, base[:2])
        assert pngs.keys() == base[2].keys() and all(pngs[k] == base[2][k] for k in pngs), key


def test_multi_gpu_test_byte_frames_asks_for_what_is_needed(tmp_path):
    """metrics only -> fp32 planes; images only -> uint8; both -> both; the pair goes through forward_clips (no concatenation)"""
    from pnp_vcve_amd import restorer, synthetic as syn  # noqa: F401
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset
    from pnp_vcve_amd.registry import build_model
    lq, gt, qp = syn.write_clip_tree(str(tmp_path / 'data'), clips=['000', '011'], t=3, h=64, w=96, seed=4)
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='REDS4', test_mode=True))
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg)
    model = build_model(dict(type='BasicVSR', generator=gen, pixel_loss=dict(type='CharbonnierLoss')), train_cfg=None,
                        test_cfg=dict(metrics=['PSNR', 'SSIM'], crop_border=0))
    model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=9).items()})
    model = model.to(dev()).eval()
    asked = []
    orig_clips = model.generator.forward_clips

    def spy(clips, out_dtype=None):
        asked.append((len(list(clips)), out_dtype, clips[0][0].dtype))
        return orig_clips(clips, out_dtype=out_dtype)

    model.generator.forward_clips = spy
    ref = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2)
    got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_frames=True)
    assert asked == [(2, torch.float32, torch.uint8)]
    assert [r['eval_result'] for r in got] == [r['eval_result'] for r in ref]
    got = multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_frames=True, save_image=True, save_path=str(tmp_path / 'a'))
    assert asked[-1] == (2, 'both', torch.uint8) and [r['eval_result'] for r in got] == [r['eval_result'] for r in ref]
    ref1 = multi_gpu_test(model, ds, device=dev(), clips_in_flight=1, save_image=True, save_path=str(tmp_path / 'b'))
    assert [r['eval_result'] for r in ref1] == [r['eval_result'] for r in ref]
    for clip in ('000', '011'):
        for i in range(3):
            with open(tmp_path / 'a' / clip / f'{i:08d}.png', 'rb') as fa, open(tmp_path / 'b' / clip / f'{i:08d}.png', 'rb') as fb:
                assert fa.read() == fb.read()
    model.test_cfg = dict(crop_border=0)                       # no metrics: only the images are wanted
    multi_gpu_test(model, ds, device=dev(), clips_in_flight=2, byte_frames=True, save_image=True, save_path=str(tmp_path / 'c'), metrics=())
    assert asked[-1] == (2, torch.uint8, torch.uint8)
    with open(tmp_path / 'c' / '011' / '00000002.png', 'rb') as fa, open(tmp_path / 'b' / '011' / '00000002.png', 'rb') as fb:
        assert fa.read() == fb.read()
