"""GPU: the Y'CbCr 4:2:0 boundary.  NV12 / NV21 / I420 planes in, packed 4:2:0 buffers out.  The two conversions are held bit for bit
to the numpy restatement of include/pnpvcve.h's arithmetic (tests/yuv_ref.py); everything above them is a composition of things that
exist (ops.frames_from_yuv420 in front of the fp32 forward, ops.frames_to_yuv420 behind it), so every check is torch.equal or
byte-equal: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import golden_util as gu
import yuv_ref
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
SIDE = ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions')
GUARD = 64          # bytes of 0xA5 in front of and behind every allocation the tests hand out


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ planes behind guard bands
class Planes:
    """t frames of h x w in one flat device allocation full of 0xA5: `off` bytes behind the guard band the Y plane of frame 0 starts,
    rows `pitch` apart; NV12 / NV21: the interleaved chroma rows follow at the same pitch; I420: the Cb and the Cr plane follow with
    rows `cpitch` apart.  expect(y, cb, cr) is the whole allocation as it must look after exactly those planes were written."""

    def __init__(self, t, h, w, layout, pitch=None, off=0, cpitch=None):
        self.t, self.h, self.w, self.layout = t, h, w, layout
        self.pitch = pitch = w if pitch is None else pitch
        self.step = 1 if layout == 'i420' else 2
        self.cpitch = cpitch = (pitch if self.step == 2 else (pitch + 1) // 2) if cpitch is None else cpitch
        self.y0 = GUARD + off
        self.c0 = self.y0 + h * pitch
        nchroma = (h // 2) * cpitch * (1 if self.step == 2 else 2)
        self.frame = h * pitch + nchroma
        self.nbytes = self.y0 + t * self.frame + GUARD
        self.flat = torch.full((self.nbytes,), 0xA5, dtype=torch.uint8, device=dev())
        self.views = self._views(self.flat)

    def _views(self, flat):
        t, h, w, st = self.t, self.h, self.w, self.step
        y = flat.as_strided((t, h, w), (self.frame, self.pitch, 1), self.y0)
        if st == 2:
            a = flat.as_strided((t, h // 2, w // 2), (self.frame, self.cpitch, 2), self.c0)
            b = flat.as_strided((t, h // 2, w // 2), (self.frame, self.cpitch, 2), self.c0 + 1)
            cb, cr = (a, b) if self.layout == 'nv12' else (b, a)
        else:
            cb = flat.as_strided((t, h // 2, w // 2), (self.frame, self.cpitch, 1), self.c0)
            cr = flat.as_strided((t, h // 2, w // 2), (self.frame, self.cpitch, 1), self.c0 + (h // 2) * self.cpitch)
        return ops.Yuv420Frames(y, cb, cr)

    def fill(self, y, cb, cr):
        for dst, src in zip(self.views, (y, cb, cr)):
            dst.copy_(src)
        return self

    def expect(self, y, cb, cr):
        flat = torch.full((self.nbytes,), 0xA5, dtype=torch.uint8)
        for dst, src in zip(self._views(flat), (y, cb, cr)):
            dst.copy_(src.cpu())
        return flat


def random_planes(seed, t, h, w):
    """decoder-like bytes, a third of the samples at the range's ends (out-of-gamut triples: the clamp has work to do)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        x = torch.randint(0, 256, (t, hh, ww), generator=g, dtype=torch.uint8)
        r = torch.rand((t, hh, ww), generator=g)
        out.append(torch.where(r < 1 / 6, torch.zeros_like(x), torch.where(r > 5 / 6, torch.full_like(x, 255), x)))
    return out


def ref_planes(y, cb, cr, standard):
    return torch.from_numpy(yuv_ref.frames_from_yuv420(y.numpy(), cb.numpy(), cr.numpy(), standard))


# layouts x pitches (w, w + 6, w + 7) x base address offsets 0..3; I420 also with an odd chroma pitch of its own
def layouts(w):
    for layout in ops.YUV_LAYOUTS:
        for pitch in (w, w + 6, w + 7):
            for off in range(4):
                yield layout, pitch, off, None
    yield 'i420', w + 7, 1, w // 2 + 3


# ------------------------------------------------------------------------------------------------ the ops against the restatement
_ALL = {}


def all_triples():
    """one 4096 x 4096 frame that enumerates all 2^24 (Y, Cb, Cr) triples: block b = by * 2048 + bx carries the chroma pair
    (b >> 8 & 255, b & 255) and the four luma values 4 (b >> 16) + 0..3"""
    if not _ALL:
        b = np.arange(1 << 22, dtype=np.int64).reshape(2048, 2048)
        cb, cr = ((b >> 8) & 255).astype(np.uint8), (b & 255).astype(np.uint8)
        y = np.empty((4096, 4096), np.uint8)
        for j in range(4):
            y[j >> 1::2, j & 1::2] = 4 * (b >> 16) + j
        up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1).astype(np.int64)      # noqa: E731
        code = (y.astype(np.int64) << 16) | (up(cb) << 8) | up(cr)
        assert np.unique(code).size == 1 << 24
        _ALL['planes'] = tuple(torch.from_numpy(x[None]) for x in (y, cb, cr))
    return _ALL['planes']


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_frames_from_yuv420_on_all_triples_is_the_restatement(standard):
    y, cb, cr = all_triples()
    want = ref_planes(y, cb, cr, standard)                                      # (1, 3, 4096, 4096)
    p = Planes(1, 4096, 4096, 'nv12').fill(y, cb, cr)
    got = ops.frames_from_yuv420(p.views, standard)
    assert got.shape == (1, 3, 4096, 4096) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    assert torch.equal(torch.ops.pnpvcve.frames_from_yuv420(*p.views, yuv_ref.STANDARDS.index(standard)), got)
    # the forward's unpacking, aligned form and byte-load form: the same values as (h,w,4) RGB0
    for general in (False, True):
        lr4 = ops.pack_lr_yuv420(p.views, standard, general=general)
        assert torch.equal(lr4[..., :3].permute(0, 3, 1, 2), got) and not bool(lr4[..., 3].any()), general
    assert torch.equal(p.flat.cpu(), p.expect(y, cb, cr))                       # read only


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_frames_from_yuv420_layouts_pitches_and_addresses(standard):
    t, h, w = 2, 64, 96
    y, cb, cr = random_planes(5, t, h, w)
    want = ref_planes(y, cb, cr, standard).to(dev())
    for layout, pitch, off, cpitch in layouts(w):
        p = Planes(t, h, w, layout, pitch, off, cpitch).fill(y, cb, cr)
        tag = (layout, pitch, off, cpitch)
        assert torch.equal(ops.frames_from_yuv420(p.views, standard), want), tag
        fast = ops.pack_lr_yuv420(p.views, standard)
        slow = ops.pack_lr_yuv420(p.views, standard, general=True)
        assert torch.equal(fast, slow) and torch.equal(fast[..., :3].permute(0, 3, 1, 2), want) and not bool(fast[..., 3].any()), tag
        assert torch.equal(p.flat.cpu(), p.expect(y, cb, cr)), tag
    # a batch: (n,t,...) views, clips one after the other
    p = Planes(4, h, w, 'nv12').fill(*random_planes(6, 4, h, w))
    v4 = ops.Yuv420Frames(*[x.unflatten(0, (2, 2)) for x in p.views])
    assert torch.equal(ops.frames_from_yuv420(v4, standard), ops.frames_from_yuv420(p.views, standard).unflatten(0, (2, 2)))


def crafted_planes(standard, h=64, w=96):
    """(3, 3, h, w): random values in [-0.2, 1.2]; the k / 255 grid; greys whose luma lands exactly on n + 0.5 (rint ties) mixed with
    saturated primaries (chroma at the range's ends)"""
    k = yuv_ref.constants(standard)
    g = torch.Generator().manual_seed(17)
    a = torch.rand((3, h, w), generator=g) * 1.4 - 0.2
    b = torch.randint(0, 256, (3, h, w), generator=g).float() / 255.0
    ties = []
    for n in range(k['yoff'], k['yoff'] + 219):
        v = np.float32((n + 0.5 - k['yoff']) / float(k['sy']))
        yl = (k['kr'] * v + k['kg'] * v) + k['kb'] * v
        if np.float32(k['yoff']) + k['sy'] * yl == np.float32(n + 0.5):
            ties.append(float(v))
    assert len(ties) > 20
    c = torch.tensor(ties, dtype=torch.float32).repeat(h * w // len(ties) + 1)[:h * w].reshape(1, h, w).repeat(3, 1, 1).clone()
    prim = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=torch.float32)
    for j in range(6):
        c[:, 8 * j:8 * j + 8, 48:] = prim[j][:, None, None]
    return torch.stack([a, b, c])


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_frames_to_yuv420_is_the_restatement_and_writes_nothing_else(standard):
    planes = crafted_planes(standard)
    t, _, h, w = planes.shape
    assert float(planes.min()) < 0 and float(planes.max()) > 1
    y, cb, cr = [torch.from_numpy(x) for x in yuv_ref.frames_to_yuv420(planes.numpy(), standard)]
    assert int(y.min()) == yuv_ref.constants(standard)['yoff'] and int(cb.min()) < 20 and int(cr.max()) > 235
    dplanes = planes.to(dev())
    for layout, pitch, off, cpitch in layouts(w):
        p = Planes(t, h, w, layout, pitch, off, cpitch)
        ops.frames_to_yuv420(dplanes, standard, out=p.views)
        got, want = p.flat.cpu(), p.expect(y, cb, cr)
        assert torch.equal(got, want), (layout, pitch, off, cpitch, int((got != want).sum()))
    for layout in ('nv12', 'nv21', 'i420'):
        buf, views = ops.frames_to_yuv420(dplanes, standard, layout)
        assert buf.shape == (t, h * 3 // 2, w) and buf.dtype == torch.uint8
        assert torch.equal(buf.cpu(), torch.from_numpy(yuv_ref.pack(y.numpy(), cb.numpy(), cr.numpy(), layout))), layout
        assert all(torch.equal(a.cpu(), b) for a, b in zip(views, (y, cb, cr)))
        assert all(torch.equal(a, b) for a, b in zip(ops.yuv420_views(buf, h, w, layout), views))


def test_bad_frames_raise_before_any_gpu_work():
    d = dev()
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=d)      # noqa: E731
    with pytest.raises(ValueError, match='even'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 65, 64), z(1, 32, 32), z(1, 32, 32)))
    with pytest.raises(ValueError, match='even'):
        ops.yuv420_views(z(1, 96, 66), 64, 65)
    with pytest.raises(ValueError, match='h/2'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 64), z(1, 32, 31), z(1, 32, 31)))
    with pytest.raises(ValueError, match='last stride'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 128)[..., ::2], z(1, 32, 32), z(1, 32, 32)))
    with pytest.raises(ValueError, match='last stride'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 64), z(1, 32, 96)[..., ::3], z(1, 32, 96)[..., ::3]))
    with pytest.raises(ValueError, match='interleaved'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 64), z(1, 32, 64)[..., ::2], z(1, 32, 64)[..., ::2]))
    with pytest.raises(TypeError):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 64).float(), z(1, 32, 32), z(1, 32, 32)))
    with pytest.raises(ValueError, match='yuv_standard'):
        ops.frames_from_yuv420(ops.Yuv420Frames(z(1, 64, 64), z(1, 32, 32), z(1, 32, 32)), 'bt2020')
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.frames_from_yuv420(ops.Yuv420Frames(*[x.cpu() for x in (z(1, 64, 64), z(1, 32, 32), z(1, 32, 32))]))


# ------------------------------------------------------------------------------------------------ the forward
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


def yuv_clip(seed, n=1, t=3, h=64, w=64, slices=(73, 66, 80), layout='nv12', pitch=None, off=0):
    """side info of a synthetic clip (slices: 'IBP' by default) + its frames as 4:2:0 planes: clip b in an allocation of its own behind
    guard bands"""
    c = gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=slices, qp_mode='qp', crf=[15, 35, 25, 30][:n] if n > 1 else 25)
    a = {k: torch.from_numpy(c[k]).to(dev()) for k in SIDE}
    a['bytes'] = [random_planes(seed + 7 * b, t, h, w) for b in range(n)]
    a['planes'] = [Planes(t, h, w, layout, pitch, off).fill(*a['bytes'][b]) for b in range(n)]
    return a


def batch_views(a):
    """the clips of `a` as ONE Yuv420Frames of (n,t,...) views: n = 1 the allocation itself, n > 1 a packed copy"""
    if len(a['planes']) == 1:
        return ops.Yuv420Frames(*[x[None] for x in a['planes'][0].views])
    return ops.Yuv420Frames(*[torch.stack([p.views[j] for p in a['planes']]) for j in range(3)])


def fwd(m, lq, a, **kw):
    with torch.no_grad():
        return m(lq, a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'], **kw)


def poison(shape, dtype):
    """leave a block of the output's size, full of a poison byte, at the top of the caching allocator's free list: the forward's
    torch.empty of that size takes it"""
    x = torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda') if dtype == torch.uint8 else torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    del x


def check_boundary(m, a, label, standard='bt601-limited', replays=1, out_layout='nv12'):
    """input side: forward(Yuv420Frames) == forward(frames_from_yuv420(...)); output side: the packed 4:2:0 buffer ==
    frames_to_yuv420(plain forward); (fp32, uint8, nv12) at once == the three separate calls; the input planes are left as they were"""
    frames = batch_views(a)
    planes = ops.frames_from_yuv420(frames, standard)
    n, t, h, w = frames.y.shape
    assert planes.shape == (n, t, 3, h, w)
    for _ in range(replays):
        ref = fwd(m, planes, a).clone()
    lo, hi = float(ref.min()), float(ref.max())
    print(f'{label}: plain output in [{lo:.3f}, {hi:.3f}]')
    assert lo < 0.0 and hi > 1.0, (label, lo, hi)                   # the clamps are exercised
    s = 4 if m.vsr else 1
    H, W = h * s, w * s
    assert ref.shape == (n, t, 3, H, W)
    refy = ops.frames_to_yuv420(ref, standard, out_layout)[0]
    ref8 = ops.frames_to_rgb8(ref.reshape(n * t, 3, H, W)).reshape(n, t, H, W, 3)
    for _ in range(replays):
        poison((n, t, 3, H, W), torch.float32)
        got = fwd(m, frames, a, yuv_standard=standard)
    assert got.dtype == torch.float32 and torch.equal(got, ref), (label, 'planes in')
    for _ in range(replays):
        poison((n, t, H * 3 // 2, W), torch.uint8)
        goty = fwd(m, frames, a, yuv_standard=standard, out_dtype=out_layout)
    assert goty.dtype == torch.uint8 and goty.shape == (n, t, H * 3 // 2, W)
    assert torch.equal(goty, refy), (label, out_layout, int((goty != refy).sum()))
    for _ in range(replays):
        poison((n, t, 3, H, W), torch.float32)
        poison((n, t, H, W, 3), torch.uint8)
        poison((n, t, H * 3 // 2, W), torch.uint8)
        three = fwd(m, frames, a, yuv_standard=standard, out_dtype=(torch.float32, torch.uint8, out_layout))
    assert isinstance(three, tuple) and len(three) == 3
    assert torch.equal(three[0], ref) and torch.equal(three[1], ref8) and torch.equal(three[2], refy), (label, 'three outputs')
    got8 = fwd(m, frames, a, yuv_standard=standard, out_dtype=torch.uint8)
    assert torch.equal(got8, ref8), (label, 'uint8 out')
    pair = fwd(m, frames, a, yuv_standard=standard, out_dtype=[out_layout, torch.uint8])
    assert torch.equal(pair[0], refy) and torch.equal(pair[1], ref8), (label, 'pair')
    for p, b in zip(a['planes'], a['bytes']):
        assert torch.equal(p.flat.cpu(), p.expect(*b)), (label, 'input planes touched')
    return ref, refy


def _cases():
    V = _native.OPT_CONV_LAST_VALU
    #        name, cfg, attrs, options, clip, check
    return [('s64_ibp', {}, {}, {}, dict(t=3, h=64, w=64), {}),
            ('s64x96_ibp_bt709', {}, {}, {}, dict(t=3, h=64, w=96, layout='nv21'), dict(standard='bt709-limited', out_layout='i420')),
            ('s128_t7_ibbbp', {}, {}, {}, dict(t=7, h=128, w=128, slices='IBBBP'), dict(standard='bt709-full')),
            ('odd_pitch_and_address', {}, {}, {}, dict(t=3, h=64, w=96, pitch=103, off=3), dict(standard='bt601-full')),
            ('i420_n2', {}, {}, {}, dict(n=2, t=3, h=64, w=96, layout='i420'), {}),
            ('any_size_66x70', {}, dict(any_size=True), {}, dict(t=3, h=66, w=70), {}),
            ('vsr', dict(vsr=True, num_blocks=2), {}, {}, dict(t=3, h=64, w=64), {}),
            ('vsr_fp16', dict(vsr=True, num_blocks=2), dict(precision='fp16'), {}, dict(t=3, h=64, w=64), {}),
            ('vsr_mfma_last', dict(vsr=True, num_blocks=2), {}, {V: 0}, dict(t=3, h=64, w=64), {}),
            ('fp16', {}, dict(precision='fp16'), {}, dict(t=3, h=64, w=96), {}),
            ('f16x3', {}, dict(precision='f16x3'), {}, dict(t=3, h=64, w=96), {}),
            ('mfma_last', {}, {}, {V: 0}, dict(t=3, h=64, w=96), {}),
            ('bounded_min', {}, {}, {}, dict(t=11, h=64, w=96, slices='IBBBP'), {}),
            ('graphs', {}, dict(use_graphs=True), {}, dict(t=3, h=64, w=96), dict(replays=2)),
            ('graphs_n2', {}, dict(use_graphs=True), {}, dict(n=2, t=3, h=64, w=64), dict(replays=2))]


@pytest.mark.parametrize('case', _cases(), ids=[c[0] for c in _cases()])
def test_yuv_boundary(case):
    name, cfg_over, attrs, opts, kw, ckw = case
    attrs = dict(attrs)
    precision = attrs.pop('precision', 'fp32')
    m = build(cfg_over, seed=410 + len(name), precision=precision, **attrs)
    for o, v in opts.items():
        m.set_option(o, v)
    if 'bounded' in name:
        m.max_resident_features = m.min_resident_features(kw['t'])
        assert m.max_resident_features < kw['t']
    ref, _ = check_boundary(m, yuv_clip(seed=41 + len(name), **kw), name, **ckw)
    if name.startswith('vsr'):
        assert ref.shape[-2:] == (256, 256)


def test_nv12_from_one_packed_allocation_and_i420_from_three():
    m = build()
    a = yuv_clip(seed=77, t=3, h=64, w=96)
    y, cb, cr = a['bytes'][0]
    want = fwd(m, ops.frames_from_yuv420(batch_views(a)), a)
    packed = torch.from_numpy(yuv_ref.pack(y.numpy(), cb.numpy(), cr.numpy(), 'nv12'))[None].to(dev())      # (1, t, 3h/2, w)
    assert torch.equal(fwd(m, ops.yuv420_views(packed, 64, 96, 'nv12'), a), want)
    three = ops.Yuv420Frames(*[x[None].to(dev()).clone() for x in (y, cb, cr)])                               # three allocations
    assert len({x.untyped_storage().data_ptr() for x in three}) == 3
    assert torch.equal(fwd(m, three, a), want)
    flat = torch.from_numpy(yuv_ref.pack(y.numpy(), cb.numpy(), cr.numpy(), 'i420')).reshape(1, 3, -1).to(dev())
    assert torch.equal(fwd(m, ops.yuv420_views(flat, 64, 96, 'i420'), a), want)


def test_forward_clips_with_planes_in_separate_allocations_and_the_custom_op():
    m = build()
    a = yuv_clip(seed=91, n=2, t=3, h=64, w=96, pitch=100, off=1)
    assert a['planes'][0].flat.data_ptr() != a['planes'][1].flat.data_ptr()
    std = 'bt709-limited'
    clips = [(a['planes'][b].views, a['QPs'][b], a['slices'][b], a['mvs'][b], a['base_QPs'][b], a['partitions'][b]) for b in range(2)]
    ref = fwd(m, ops.frames_from_yuv420(batch_views(a), std), a)
    refy = ops.frames_to_yuv420(ref, std, 'nv12')[0]
    with torch.no_grad():
        outs = m.forward_clips(clips, yuv_standard=std)
        both = m.forward_clips(clips, out_dtype=(torch.float32, 'nv12'), yuv_standard=std)
    for b in range(2):
        assert outs[b].shape == (1, 3, 3, 64, 96) and torch.equal(outs[b][0], ref[b]), b
        assert torch.equal(both[b][0][0], ref[b]) and torch.equal(both[b][1][0], refy[b]), b
        p = a['planes'][b]
        assert torch.equal(p.flat.cpu(), p.expect(*a['bytes'][b]))
    # the custom op is what forward_clips calls: the same tensors from its own entry
    side = torch.stack([a['slices'].reshape(2, 3).float(), a['QPs'].reshape(2, 3).float(), a['base_QPs'].reshape(2, 3).float()]).cpu().contiguous()
    v = [p.views for p in a['planes']]
    with torch.no_grad():
        got = torch.ops.pnpvcve.generator_forward_clips_yuv(m._op_handle, [x.y for x in v], [x.cb for x in v], [x.cr for x in v],
                                                            list(a['mvs'].float().contiguous()), list(a['partitions'].float().contiguous()), side,
                                                            yuv_ref.STANDARDS.index(std), 5, 0)
    assert len(got) == 4
    assert all(torch.equal(got[b], ref[b]) and torch.equal(got[2 + b], refy[b]) for b in range(2))


def test_forward_errors_before_any_gpu_work():
    m = build()
    a = yuv_clip(seed=3, t=3, h=64, w=64)
    frames = batch_views(a)
    with pytest.raises(ValueError, match='out_dtype'):
        fwd(m, frames, a, out_dtype='p010')
    with pytest.raises(ValueError, match='one 4:2:0'):
        fwd(m, frames, a, out_dtype=('nv12', 'i420'))
    with pytest.raises(ValueError, match='yuv_standard'):
        fwd(m, frames, a, yuv_standard='bt2020')
    with pytest.raises(ValueError, match='even'):
        fwd(m, ops.Yuv420Frames(frames.y[..., :63, :], frames.cb, frames.cr), a)
    with pytest.raises(ValueError):      # 4:2:0 output is offered on the 4:2:0 entry only
        fwd(m, ops.frames_from_yuv420(frames), a, out_dtype='nv12')
    # 66 x 70 without any_size: the reference's refusal of frames that are no multiple of 4
    b = yuv_clip(seed=4, t=3, h=66, w=70)
    with pytest.raises(ValueError, match='multiple of 4'):
        fwd(m, batch_views(b), b)
