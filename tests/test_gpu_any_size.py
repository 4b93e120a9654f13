"""GPU: generator.any_size -- the forward on frames whose height and width are no multiple of 4.

The reference raises on these sizes (its spatial_padding pads lrs alone, flow_warp then refuses the unpadded flow), so there is no
reference output: expected values come from tests/any_size_ref.py, the loop of iconvsr_ipb_par.py:44-149 restated from the oracle's
pinned blocks and held to torch.equal with the oracle wherever the oracle runs (tests/test_any_size_ref.py).  Gates are the project's
existing ones: 5e-6 for fp32 and split fp16, 2e-2 for fp16; everything that is a reordering of the same arithmetic is torch.equal.

Sizes, each for the edge it cuts (16x16 Winograd tiles of 2x2 output tiles, 8x8 quadrants, 8x16 flag tiles):
    65x65    last tile row and column one pixel wide; a frame is 12675 bytes, odd
    66x79    a 2x2 Winograd tile and an 8x8 quadrant cut; w = 16 k + 15
    73x67    a quadrant row one pixel high
    67x129   a ninth tile column one pixel wide
    177x193  12 x 13 = 156 tiles: the tile kernels on default routing (128 tiles is the unit kernels' limit)
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import any_size_ref
import golden_util as gu
from oracle import cpu_ref
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_F16 = 5e-6, 2e-2          # tests/test_gpu_generator.py's and tests/test_gpu_fp16.py's gates
KEYS = ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions')
SMALL = [(65, 65), (66, 79), (73, 67), (67, 129)]
SIZES = SMALL + [(177, 193)]
T3, T5 = [73, 66, 80], [73, 66, 66, 80, 66]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def sid(hw):
    return f'{hw[0]}x{hw[1]}'


def make_cfg(**over):
    return dict(gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=2, **over)


def weights(cfg, seed=500):
    return gu.syn.make_state_dict(cfg, seed=seed, par_gain=10.0)


def make_clip(h, w, t=3, n=1, slices=None, seed=600, overlap_par=False):
    """partition maps on 8x8 blocks cropped by the frame, quarter-pel block MVs (synthetic.make_clip)"""
    if slices is None:
        slices = T3 if t == 3 else (T5 if t == 5 else 'IBBBP')
    c = gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=slices, qp_mode='qp', crf=[15, 35][:n] if n > 1 else 25)
    if overlap_par:         # sparse_val: planes that overlap and are not binary, on 4x4 blocks cropped by the frame
        bh, bw = (h + 3) // 4, (w + 3) // 4
        blk = (gu.syn.randint(seed, 'par_on', (n, t, 3, bh, bw), 0, 1).astype(np.float32) * gu.syn.uniform(seed, 'par_val', (n, t, 3, bh, bw), 0.05, 1.0))
        c['partitions'] = np.ascontiguousarray(np.repeat(np.repeat(blk, 4, axis=3), 4, axis=4)[..., :h, :w])
    return c


def build(cfg, sd_np, any_size=True, precision='fp32', wino=None, **attrs):
    from pnp_vcve_amd.registry import build_backbone
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    m = m.to(dev()).eval()
    m.any_size = any_size
    if precision != 'fp32':
        m.precision = precision
    if wino is not None:
        m.set_option(_native.OPT_WINOGRAD, wino)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def poison(shape, dtype=torch.float32):
    """leave a NaN-filled (0xA5-filled) block of the output's size on top of the caching allocator's free list: the forward's
    torch.empty of that size takes it, so a pixel the kernels skip shows"""
    x = torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda') if dtype == torch.uint8 else torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    del x


def run(m, clip, lq=None, **kw):
    a = {k: torch.from_numpy(v).to(dev()) if isinstance(v, np.ndarray) else v for k, v in clip.items()}
    n, t, _, h, w = a['partitions'].shape
    s = 4 if m.vsr else 1
    poison((n, t, 3, h * s, w * s))
    with torch.no_grad():
        return m(a['lq'] if lq is None else lq, a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'], **kw)


_REFS = {}


def expected(cfg, sd_np, clip, key):
    """any_size_ref on the CPU, once per case of this module"""
    if key not in _REFS:
        c = [torch.from_numpy(clip[k]) for k in KEYS]
        with torch.no_grad():
            _REFS[key] = any_size_ref.generator_forward(cpu_ref.to_torch_state(sd_np), cfg, *c)
    return _REFS[key]


def maxdiff(out, ref):
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), 'a pixel of the output was never written'
    return float((out.cpu() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ the switch
def test_off_by_default_and_the_refusal_is_the_references():
    cfg = make_cfg()
    m = build(cfg, weights(cfg), any_size=False)
    assert m.any_size is False
    with pytest.raises(ValueError, match='spatial sizes of input and flow'):
        run(m, make_clip(65, 65))
    m.any_size = True
    assert m.any_size is True and run(m, make_clip(65, 65)).shape == (1, 3, 3, 65, 65)
    with pytest.raises(AssertionError):          # h, w >= 64 in both modes
        run(m, make_clip(63, 65))
    from pnp_vcve_amd.registry import build_backbone
    assert build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', any_size=True, **cfg)).any_size is True


def test_a_dcn_aligner_is_refused_with_the_switch_on():
    cfg = make_cfg(deform='basic')
    m = build(cfg, weights(cfg))
    with pytest.raises(RuntimeError, match='unsupported'):
        run(m, make_clip(65, 65))


# ------------------------------------------------------------------------------------------------ against any_size_ref
@pytest.mark.parametrize('precision', ['fp32', 'f16x3', 'fp16'])
@pytest.mark.parametrize('hw', SIZES, ids=sid)
def test_ragged_frames_vs_the_restated_oracle(hw, precision):
    cfg = make_cfg()
    sd_np, clip = weights(cfg), make_clip(*hw)
    ref = expected(cfg, sd_np, clip, ('plain',) + hw)
    m = build(cfg, sd_np, precision=precision)
    d = maxdiff(run(m, clip), ref)
    print(f'{sid(hw)} {precision}: max|hip - any_size_ref| = {d:.3g}')
    assert d < (TOL_F16 if precision == 'fp16' else TOL)


#            name             cfg overrides                 size        clip kwargs
VARIANTS = [('channel_last', dict(channel_first=False), (66, 79), {}),
            ('vsr', dict(vsr=True), (65, 67), {}),
            ('n2_mixed_keys', {}, (73, 67), dict(n=2, t=5, slices=[[73, 66, 66, 80, 66], [73, 80, 66, 66, 66]])),
            ('sparse_val', dict(sparse_val=True), (66, 79), dict(overlap_par=True)),
            ('nocat_t5', dict(with_cat=False), (67, 129), dict(t=5)),
            ('noalignkey_t5', dict(align_key=False), (65, 65), dict(t=5, slices=[73, 80, 66, 80, 66]))]


@pytest.mark.parametrize('wino', [0, 1, 2])
@pytest.mark.parametrize('name,over,hw,ckw', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_configurations_and_kernel_routings_vs_the_restated_oracle(name, over, hw, ckw, wino):
    cfg = make_cfg(**over)
    sd_np, clip = weights(cfg, seed=510), make_clip(*hw, seed=610, **ckw)
    ref = expected(cfg, sd_np, clip, (name,) + hw)
    m = build(cfg, sd_np, wino=wino)
    out = run(m, clip)
    s = 4 if cfg['vsr'] else 1
    assert out.shape == (ckw.get('n', 1), ckw.get('t', 3), 3, hw[0] * s, hw[1] * s)
    d = maxdiff(out, ref)
    print(f'{name} {sid(hw)} PNP_OPT_WINOGRAD={wino}: max|hip - any_size_ref| = {d:.3g}')
    assert d < TOL


def test_davis_480p_vs_the_restated_oracle_and_band_chains():
    """2 x 3 x 480 x 854 (854 % 4 = 2) on the default path: 30 x 54 = 1620 tiles, the tile kernels; two clips run on two contexts, so the
    row-band chains are off.  Then one clip alone, where they are on: forced on == off, bit for bit."""
    cfg = make_cfg()
    sd_np, clip = weights(cfg, seed=520), make_clip(480, 854, n=2, seed=620)
    ref = expected(cfg, sd_np, clip, ('davis',))
    m = build(cfg, sd_np)
    out = run(m, clip)
    assert next(iter(m._workspace))[0] == 2
    d = maxdiff(out, ref)
    print(f'2x3x480x854: max|hip - any_size_ref| = {d:.3g}')
    assert d < TOL
    one = {k: v[:1] for k, v in clip.items()}
    m.band_split = 1
    on = run(m, one).clone()
    assert torch.equal(on, out[:1])
    m.band_split = 0
    assert torch.equal(run(m, one), on)


# ------------------------------------------------------------------------------------------------ bit-identical reorderings
@pytest.mark.parametrize('hw', SMALL, ids=sid)
def test_unit_kernels_equal_tile_kernels(hw):
    """PNP_OPT_WINOGRAD 1 (these sizes: the quadrant-unit kernels) == 2 (the tile kernels)"""
    cfg = make_cfg()
    sd_np, clip = weights(cfg), make_clip(*hw)
    assert _native.wino_kernel_form(hw[0], hw[1], 1) == 'units'
    outs = [run(build(cfg, sd_np, wino=wv), clip).clone() for wv in (1, 2)]
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('hw', [(66, 79), (177, 193)], ids=sid)
def test_partition_branch_skipping_changes_no_bit(hw):
    """fp32: a skipped branch drops exact zeros, PNP_OPT_PAR_SKIP 0 == 1 bit for bit"""
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clip = make_clip(*hw)
    m.set_option(_native.OPT_PAR_SKIP, 0)
    ref = run(m, clip).clone()
    m.set_option(_native.OPT_PAR_SKIP, 1)
    assert torch.equal(run(m, clip), ref)


@pytest.mark.parametrize('hw', [(66, 79), (177, 193)], ids=sid)
def test_split_fp16_with_and_without_tile_flags_vs_the_restated_oracle(hw):
    """split fp16: with the tile flags a tile whose partition values are all 0 or 1/255 contracts the branches with weights scaled at
    pack time and a masked operand -- another rounding point than par * x per fragment (tests/test_gpu_f16x3.py holds the two forms to
    0 < d < 2e-6 per conv), so the switch is not bit-neutral on this path at any frame size.  Both settings are held to the path's
    gate against the oracle instead."""
    cfg = make_cfg()
    sd_np, clip = weights(cfg), make_clip(*hw)
    ref = expected(cfg, sd_np, clip, ('plain',) + hw)
    m = build(cfg, sd_np, precision='f16x3')
    for skip in (0, 1):
        m.set_option(_native.OPT_PAR_SKIP, skip)
        d = maxdiff(run(m, clip), ref)
        print(f'{sid(hw)} f16x3 PNP_OPT_PAR_SKIP={skip}: max|hip - any_size_ref| = {d:.3g}')
        assert d < TOL


def test_band_chains_at_177x193_change_no_bit():
    """12 tile rows, chains of 5 and 6 convs: one clip in flight on the tile kernels runs as two row-band chains (the last tile row is
    one pixel high)"""
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clip = make_clip(177, 193)
    assert _native.wino_kernel_form(177, 193, 1) == 'tiles' and m.band_split == 1
    on = run(m, clip).clone()
    for split in (0, 5):          # one launch per conv; another first boundary
        m.band_split = split
        assert torch.equal(run(m, clip), on), split


def byte_frames(n, t, h, w, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randint(0, 256, (n, t, h, w, 3), device='cuda', generator=g, dtype=torch.uint8)


def to_rgb8(out):
    n, t = out.shape[:2]
    return ops.frames_to_rgb8(out.reshape((n * t,) + tuple(out.shape[2:]))).reshape(n, t, out.shape[3], out.shape[4], 3)


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
@pytest.mark.parametrize('hw', [(65, 65), (66, 79)], ids=sid)
def test_byte_frames_in_and_out(hw, precision):
    """n = 2: clip 1 of the (n,t,h,w,3) batch starts t*h*w*3 bytes in -- 38025 and 46926, no multiple of 4 -- on the way in and on the
    way out.  forward(u8) == forward(frames_from_rgb8(u8)), uint8 out == frames_to_rgb8(fp32 out).  fp16: the staged boundary."""
    h, w = hw
    cfg = make_cfg()
    m = build(cfg, weights(cfg), precision=precision)
    clip = make_clip(h, w, n=2)
    u8 = byte_frames(2, 3, h, w, seed=7)
    assert (3 * h * w * 3) % 4 != 0 and u8[1].data_ptr() % 4 != 0
    planes = ops.frames_from_rgb8(u8)
    ref = run(m, clip, lq=planes).clone()
    ref8 = to_rgb8(ref)
    assert torch.equal(run(m, clip, lq=u8), ref)
    for lq in (u8, planes):
        poison((2, 3, h, w, 3), torch.uint8)
        got8 = run(m, clip, lq=lq, out_dtype=torch.uint8)
        assert got8.shape == (2, 3, h, w, 3) and torch.equal(got8, ref8)
    poison((2, 3, h, w, 3), torch.uint8)
    both = run(m, clip, lq=u8, out_dtype='both')
    assert torch.equal(both[0], ref) and torch.equal(both[1], ref8)


@pytest.mark.parametrize('hw', [(65, 65), (66, 79)], ids=sid)
def test_forward_clips_on_two_views_of_one_byte_tensor(hw):
    """the second clip's pointer is misaligned and is read where it lies: no copy is made"""
    h, w = hw
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clip = make_clip(h, w, n=2)
    a = {k: torch.from_numpy(v).to(dev()) for k, v in clip.items()}
    u8 = byte_frames(2, 3, h, w, seed=8)
    ref = run(m, clip, lq=ops.frames_from_rgb8(u8)).clone()
    clips = [(u8[b], a['QPs'][b:b + 1], a['slices'][b:b + 1], a['mvs'][b], a['base_QPs'][b:b + 1], a['partitions'][b]) for b in range(2)]
    assert clips[1][0].data_ptr() % 4 != 0
    seen = []
    launch = m._launch_clips
    m._launch_clips = lambda lrs, *rest: (seen.extend(x.data_ptr() for x in lrs), launch(lrs, *rest))[1]
    with torch.no_grad():
        outs = m.forward_clips(clips, out_dtype='both')
    del m._launch_clips
    assert seen == [u8[0].data_ptr(), u8[1].data_ptr()]
    for b in range(2):
        assert torch.equal(outs[b][0], ref[b:b + 1]) and torch.equal(outs[b][1], to_rgb8(ref[b:b + 1]))
    # with the switch off the view is copied to an aligned address, as before (a multiple of 4 in h and w: 64x72, clip 1 at 41472 + 1)
    m.any_size = False
    flat = torch.zeros(1 + 3 * 64 * 72 * 3, dtype=torch.uint8, device='cuda')
    view = flat[1:].view(3, 64, 72, 3)
    c64 = make_clip(64, 72)
    a64 = {k: torch.from_numpy(v).to(dev()) for k, v in c64.items()}
    assert view.data_ptr() % 4 != 0
    with torch.no_grad():
        o = m.forward_clips([(view, a64['QPs'], a64['slices'], a64['mvs'][0], a64['base_QPs'], a64['partitions'][0])])
    assert o[0].shape == (1, 3, 3, 64, 72)


def test_two_contexts_equal_one_clip_at_a_time():
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clip = make_clip(73, 67, n=2, t=5, slices=[[73, 66, 66, 80, 66], [73, 80, 66, 66, 66]])
    out = run(m, clip)
    assert next(iter(m._workspace))[0] == 2
    singles = [run(m, {k: v[b:b + 1] for k, v in clip.items()}).clone() for b in range(2)]
    assert next(iter(m._workspace))[0] == 1
    assert torch.equal(out, torch.cat(singles)) and not torch.equal(out[0], out[1])


@pytest.mark.parametrize('byte_io', [False, True])
def test_graph_replay_equals_eager(byte_io):
    h, w = 66, 79
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clips = [make_clip(h, w, n=2, seed=630)]
    other = make_clip(h, w, n=2, seed=631)           # new pixel data behind the same side info: the same graph
    clips.append(dict(clips[0], lq=other['lq'], mvs=other['mvs'], partitions=other['partitions']))
    lqs = [byte_frames(2, 3, h, w, seed=9 + i) if byte_io else None for i in range(2)]
    kw = dict(out_dtype=torch.uint8) if byte_io else {}
    eager = [run(m, c, lq=q, **kw).clone() for c, q in zip(clips, lqs)]
    m.use_graphs = True
    for _ in range(2):
        for c, q, e in zip(clips, lqs, eager):
            assert torch.equal(run(m, c, lq=q, **kw), e)
    assert len(m._graphs) == 1


def test_bounded_schedule_at_the_minimum_equals_the_unbounded_one():
    cfg = make_cfg()
    m = build(cfg, weights(cfg))
    clip = make_clip(65, 65, t=9)
    ref = run(m, clip).clone()
    m.max_resident_features = m.min_resident_features(9)
    assert m.max_resident_features < 9
    assert torch.equal(run(m, clip), ref)


@pytest.mark.parametrize('byte_io', [False, True])
def test_on_equals_off_on_a_multiple_of_four(byte_io):
    cfg = make_cfg()
    sd_np = weights(cfg)
    clip = make_clip(64, 72, n=2)
    lq = byte_frames(2, 3, 64, 72, seed=11) if byte_io else None
    kw = dict(out_dtype='both') if byte_io else {}
    off, on = (run(build(cfg, sd_np, any_size=s), clip, lq=lq, **kw) for s in (False, True))
    if byte_io:
        assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    else:
        assert torch.equal(on, off)


# ------------------------------------------------------------------------------------------------ the unpacking kernel alone
def _pack(src, t, h, w, any_size, guard=64):
    """pnp_debug_pack_lr_u8 into a destination with `guard` sentinel floats in front of and behind it -> (rc, frames, guards intact)"""
    total = t * h * w
    buf = torch.full((total * 4 + 2 * guard,), -7.0, device='cuda')
    dst = buf[guard:guard + total * 4]
    rc = _native.lib().pnp_debug_pack_lr_u8(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), t, h, w, any_size,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    intact = bool((buf[:guard] == -7.0).all()) and bool((buf[guard + total * 4:] == -7.0).all())
    return rc, dst.view(total, 4), intact


@pytest.mark.parametrize('hw', [(65, 65), (66, 79)], ids=sid)
def test_pack_lr_u8_at_every_alignment_and_every_remainder(hw):
    """all four byte alignments of the clip x t*h*w % 4 in {0, 1, 2, 3}: equal to the table path (frames_from_rgb8), nothing written
    outside the destination; the aligned whole-group form keeps its refusals"""
    h, w = hw
    store = torch.randint(0, 256, (4 * h * w * 3 + 16,), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(h))
    assert store.data_ptr() % 4 == 0
    seen = set()
    # whole frames (t = 1 .. 4), and one row of `total` pixels for the remainders t * h * w does not reach
    shapes = [(t, h, w) for t in (1, 2, 3, 4)] + [(1, 1, h * w + r) for r in range(4)]
    for t, hh, ww in shapes:
        total = t * hh * ww
        for off in range(4):
            src = store[off:off + total * 3]
            assert src.data_ptr() % 4 == off
            want = ops.frames_from_rgb8(src.clone().view(1, 1, total, 3)).view(3, total).t()        # (total, 3) through the table
            rc, got, intact = _pack(src, t, hh, ww, 1)
            assert rc == 0 and intact, (t, hh, ww, off)
            assert torch.equal(got[:, :3], want) and bool((got[:, 3] == 0).all()), (t, hh, ww, off)
            rc0, got0, intact0 = _pack(src, t, hh, ww, 0)
            assert intact0
            if off or total % 4:
                assert rc0 == 1001 and bool((got0 == -7.0).all())          # PNP_ERR_BAD_ARG, nothing launched
            else:
                assert rc0 == 0 and torch.equal(got0, got)
            seen.add((off, total % 4))
    assert len(seen) == 16


# ------------------------------------------------------------------------------------------------ side info, metrics, the test loop
def test_rasteriser_at_66x79_is_its_80x80_result_cropped():
    """The reference paints a record with Python slices (loading_ipb.py:328-369): a block cut by the far edge is clipped and one that
    straddles the near edge (negative start, positive stop) selects nothing -- at every frame size alike, so the 66x79 maps are the
    80x80 maps cropped.  Only a block that lies WHOLLY beyond the top or left edge (start and stop both negative) wraps around to
    rows or columns counted from the far edge, which depends on the frame size: such records (warped P-frame blocks, x_w + w/2 < 0 or
    y_w + h/2 < 0) are left out of the crop comparison and kept in the comparison with the oracle's rasteriser at 66x79."""
    sl = 'IPBBP'
    rec, rf = gu.syn.make_mv_records(77, 5, 80, 80, sl)
    G = lambda a: torch.from_numpy(a).to(dev())      # noqa: E731
    mv, par = ops.rasterise_side_info(G(rec), G(rf), sl, 66, 79)
    assert mv.shape == (5, 4, 66, 79) and par.shape == (5, 3, 66, 79)
    mv_ref, par_ref = cpu_ref.rasterise_side_info(rec, rf, sl, 66, 79)
    assert np.array_equal(mv.cpu().numpy(), mv_ref) and np.array_equal(par.cpu().numpy(), par_ref)
    wraps = (rec[:, 3] + rec[:, 1] // 2 < 0) | (rec[:, 4] + rec[:, 2] // 2 < 0)
    assert 0 < int(wraps.sum()) < len(rec) // 4
    rec, rf = np.ascontiguousarray(rec[~wraps]), np.ascontiguousarray(rf[~wraps])
    mv80, par80 = ops.rasterise_side_info(G(rec), G(rf), sl, 80, 80)
    mv, par = ops.rasterise_side_info(G(rec), G(rf), sl, 66, 79)
    assert torch.equal(mv, mv80[..., :66, :79]) and torch.equal(par, par80[..., :66, :79])
    assert float(mv[:, :2].abs().max()) > 0 and float(mv[:, 2:].abs().max()) > 0 and float(par.max()) > 0
    assert not torch.equal(mv80[..., 66:, :], torch.zeros_like(mv80[..., 66:, :]))          # the crop cuts painted blocks


@pytest.mark.parametrize('crop', [0, 2])
def test_metrics_at_65x67(crop):
    from pnp_vcve_amd.metrics import psnr, ssim, tensor2img
    a = torch.from_numpy(gu.syn.uniform01(81, 'a', (3, 3, 65, 67)))
    b = (a + 0.05 * torch.from_numpy(gu.syn.normal(81, 'n', (3, 3, 65, 67)))).clamp(0, 1)
    gp = ops.psnr_frames(a.to(dev()), b.to(dev()), crop)
    gs = ops.ssim_frames(a.to(dev()), b.to(dev()), crop)
    for i in range(3):
        x, y = tensor2img(a[i]), tensor2img(b[i])
        assert abs(float(gp[i]) - psnr(x, y, crop)) < 1e-4            # (the host definition averages in float32)
        assert abs(float(gs[i]) - ssim(x, y, crop)) < 1e-10


def test_test_driver_any_size_flag_on_an_on_disk_tree(tmp_path):
    """a 3-frame 66x70 clip in the reference's directory layout: tools/test.py --any-size prints the PSNR the API gives and writes
    66x70 PNGs; without the flag it ends with the reference's message"""
    import pnp_vcve_amd  # noqa: F401
    from pnp_vcve_amd import restorer  # noqa: F401
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.config import Config
    from pnp_vcve_amd.datasets import build_dataset
    from pnp_vcve_amd.registry import build_model
    lq, gt, qp = gu.syn.write_clip_tree(str(tmp_path / 'data'), clips=('000',), t=3, h=66, w=70, seed=5)
    cfgp = str(tmp_path / 'ragged_folder.py')
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'REDS_folder_example.py'))
    pipeline = [dict(p) for p in base.data.test.pipeline]
    pipeline[1]['qp_slice_file'] = qp
    with open(cfgp, 'w') as fh:
        fh.write(f"_base_ = [{os.path.join(ROOT, 'configs', 'REDS_folder_example.py')!r}]\n"
                 f"data = dict(test=dict(lq_folder={lq!r}, gt_folder={gt!r}, pipeline={pipeline!r}))\n"
                 "model = dict(generator=dict(num_blocks=2))\n")
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfgp, 'none', '--seed', '0']
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and 'the spatial sizes of input and flow are not the same' in bad.stderr, bad.stdout + bad.stderr
    save = tmp_path / 'png'
    good = subprocess.run(cmd + ['--any-size', '--save-path', str(save)], capture_output=True, text=True, timeout=600)
    assert good.returncode == 0, good.stdout + good.stderr
    from PIL import Image
    assert Image.open(str(save / '000' / '00000000.png')).size == (70, 66)
    # the same through the API: tools/test.py's steps
    cfg = Config.fromfile(cfgp)
    torch.manual_seed(0)
    ds = build_dataset(cfg.data.test)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg).to(dev())
    model.generator.any_size = True
    stats = ds.evaluate(multi_gpu_test(model, ds, device=dev(), metrics=tuple(cfg.test_cfg['metrics'])))
    assert re.search(r'Eval-PSNR: (\S+)', good.stdout).group(1) == str(stats['PSNR'])
    assert re.search(r'Eval-SSIM: (\S+)', good.stdout).group(1) == str(stats['SSIM'])
    # ... and as a config option
    opt = subprocess.run(cmd + ['--cfg-options', 'model.generator.any_size=True'], capture_output=True, text=True, timeout=600)
    assert opt.returncode == 0 and re.search(r'Eval-PSNR: (\S+)', opt.stdout).group(1) == str(stats['PSNR']), opt.stdout + opt.stderr
