"""GPU: the 10 / 12-bit Y'CbCr 4:2:0 boundary.  P010 / P012 / yuv420p10le / yuv420p12le planes in, packed buffers of 16-bit words out.
The two conversions are held bit for bit to the numpy restatement of include/pnpvcve.h's arithmetic (tests/yuv16_ref.py); everything
above them is a composition of things that exist (ops.frames_from_yuv420p16 in front of the fp32 forward, ops.frames_to_yuv420p16
behind it), and in limited range the path is tied to the pinned 8-bit one by the header's identity: every check is torch.equal or
byte-equal, no tolerance anywhere.  Every allocation handed to the library has guard bands."""
import numpy as np
import pytest
import torch

import test_gpu_yuv_frames as t8        # the 8-bit boundary's helpers: the small generator, the synthetic clip, planes behind guard bands
import yuv16_ref
import yuv_ref
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
GUARD = 64          # bytes of 0xA5 in front of and behind every allocation the tests hand out
dev, fwd = t8.dev, t8.fwd


class Planes16:
    """t frames of h x w 16-bit samples in one flat device allocation full of 0xA5: `off` bytes (even) behind the guard band the Y
    plane of frame 0 starts, rows `pitch` BYTES apart; interleaved ('nv12' | 'nv21' order): the chroma rows follow at `cpitch`; planar
    ('i420'): the Cb and the Cr plane follow with rows `cpitch` apart.  expect(y, cb, cr) is the whole allocation as it must look after
    exactly those planes were written."""

    def __init__(self, t, h, w, order, depth, msb, pitch=None, off=0, cpitch=None, dtype=torch.int16):
        self.t, self.h, self.w, self.order, self.depth, self.msb, self.dtype = t, h, w, order, depth, msb, dtype
        self.pitch = pitch = 2 * w if pitch is None else pitch
        self.step = 1 if order == 'i420' else 2
        self.cpitch = cpitch = (pitch if self.step == 2 else (pitch // 2 + 1) // 2 * 2) if cpitch is None else cpitch
        assert off % 2 == 0 and pitch % 2 == 0 and cpitch % 2 == 0 and cpitch >= self.step * w
        self.y0 = GUARD + off
        self.c0 = self.y0 + h * pitch
        self.frame = h * pitch + (h // 2) * cpitch * (1 if self.step == 2 else 2)
        self.nbytes = (self.y0 + t * self.frame + GUARD + 1) // 2 * 2
        self.flat = torch.full((self.nbytes,), 0xA5, dtype=torch.uint8, device=dev())
        self.views = self._views(self.flat)

    def _views(self, flat):
        t, h, w, st = self.t, self.h, self.w, self.step
        words = flat.view(self.dtype)
        fr, p, cp, y0, c0 = self.frame // 2, self.pitch // 2, self.cpitch // 2, self.y0 // 2, self.c0 // 2
        y = words.as_strided((t, h, w), (fr, p, 1), y0)
        if st == 2:
            a = words.as_strided((t, h // 2, w // 2), (fr, cp, 2), c0)
            b = words.as_strided((t, h // 2, w // 2), (fr, cp, 2), c0 + 1)
            cb, cr = (a, b) if self.order == 'nv12' else (b, a)
        else:
            cb = words.as_strided((t, h // 2, w // 2), (fr, cp, 1), c0)
            cr = words.as_strided((t, h // 2, w // 2), (fr, cp, 1), c0 + (h // 2) * cp)
        return ops.Yuv420Frames16(y, cb, cr, self.depth, self.msb)

    def fill(self, y, cb, cr):
        """y, cb, cr: CPU tensors of sample VALUES (any integer dtype)"""
        for dst, src in zip(self.views[:3], (y, cb, cr)):
            dst.copy_(to_words(src, self.depth, self.msb).view(self.dtype))
        return self

    def expect(self, y, cb, cr):
        flat = torch.full((self.nbytes,), 0xA5, dtype=torch.uint8)
        for dst, src in zip(self._views(flat)[:3], (y, cb, cr)):
            dst.copy_(to_words(src, self.depth, self.msb).view(self.dtype))
        return flat


def to_words(vals, depth, msb):
    """CPU tensor of sample values -> int16 tensor carrying the container's words"""
    return torch.from_numpy(yuv16_ref.words(vals.numpy(), depth, msb).view(np.int16))


def random_values(seed, t, h, w, depth):
    """decoder-like sample values (int32 CPU tensors), a third of them at the range's ends (out-of-gamut triples: the clamp works)"""
    g = torch.Generator().manual_seed(seed)
    top = (1 << depth) - 1
    out = []
    for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        x = torch.randint(0, top + 1, (t, hh, ww), generator=g, dtype=torch.int32)
        r = torch.rand((t, hh, ww), generator=g)
        out.append(torch.where(r < 1 / 6, torch.zeros_like(x), torch.where(r > 5 / 6, torch.full_like(x, top), x)))
    return out


def ref_planes(vals, standard, depth):
    y, cb, cr = [yuv16_ref.words(v.numpy(), depth, False) for v in vals]
    return torch.from_numpy(yuv16_ref.from_yuv16(y, cb, cr, standard, depth, False))


# orders x (pitch, chroma pitch) = row + 0 | + 2 | + 6 bytes x base address offsets 0, 2, 4, 6 bytes: 8-byte aligned planes and pitches
# (the aligned form of the pack launch, where w is a multiple of 4) and everything else (the general form)
def layouts(w):
    for order in ('nv12', 'nv21', 'i420'):
        crow = 2 * w if order != 'i420' else w
        for extra in (0, 2, 6):
            for off in (0, 2, 4, 6):
                yield order, 2 * w + extra, off, crow + extra


CONTAINERS = [(10, False), (10, True), (12, False), (12, True)]


# ------------------------------------------------------------------------------------------------ the ops against the restatement
def lattice(depth):
    """one frame of sample values: every Y code against the chroma codes {0, 1, mid-1, mid, mid+1, max-1, max} and every 16 s-th
    code, Cb x Cr.  Block row = one (Cb, Cr) pair, block column j carries the four luma codes 4 j + 0..3."""
    top, mid, s = (1 << depth) - 1, 1 << (depth - 1), 1 << (depth - 8)
    c = np.unique(np.array([0, 1, mid - 1, mid, mid + 1, top - 1, top] + list(range(0, top + 1, 16 * s)), np.int32))
    cbv, crv = [x.reshape(-1) for x in np.meshgrid(c, c, indexing='ij')]
    nb = (top + 1) // 4
    cb = np.broadcast_to(cbv[:, None], (cbv.size, nb)).copy()
    cr = np.broadcast_to(crv[:, None], (crv.size, nb)).copy()
    y = np.empty((2 * cbv.size, 2 * nb), np.int32)
    for j in range(4):
        y[j >> 1::2, j & 1::2] = 4 * np.arange(nb, dtype=np.int32)[None, :] + j
    assert np.unique(y).size == top + 1 and c.size == 21      # (0 and mid are on both lists)
    return tuple(torch.from_numpy(x[None]) for x in (y, cb, cr))


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', yuv16_ref.STANDARDS)
def test_frames_from_yuv420p16_on_the_lattice_is_the_restatement(standard, depth):
    vals = lattice(depth)
    _, h, w = vals[0].shape
    want = ref_planes(vals, standard, depth)                                    # (1, 3, h, w), shared by both containers
    for msb in (False, True):
        for order in ('nv12', 'i420'):
            p = Planes16(1, h, w, order, depth, msb).fill(*vals)
            got = ops.frames_from_yuv420p16(p.views, standard)
            assert got.shape == (1, 3, h, w) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (msb, order)
            for general in (False, True):      # the forward's unpacking, aligned form and 2-byte-load form, as (h,w,4) RGB0
                lr4 = ops.pack_lr_yuv420p16(p.views, standard, general=general)
                assert torch.equal(lr4[..., :3].permute(0, 3, 1, 2), got) and not bool(lr4[..., 3].any()), (msb, order, general)
            assert torch.equal(p.flat.cpu(), p.expect(*vals))                   # read only


@pytest.mark.parametrize('hw', [(66, 70), (64, 64)])
@pytest.mark.parametrize('standard', yuv16_ref.STANDARDS)
def test_frames_from_yuv420p16_layouts_pitches_and_addresses(standard, hw):
    t, (h, w) = 2, hw
    for depth, msb in CONTAINERS:
        vals = random_values(5 + depth, t, h, w, depth)
        want = ref_planes(vals, standard, depth).to(dev())
        for order, pitch, off, cpitch in layouts(w):
            p = Planes16(t, h, w, order, depth, msb, pitch, off, cpitch).fill(*vals)
            tag = (depth, msb, order, pitch, off, cpitch)
            assert torch.equal(ops.frames_from_yuv420p16(p.views, standard), want), tag
            fast = ops.pack_lr_yuv420p16(p.views, standard)
            slow = ops.pack_lr_yuv420p16(p.views, standard, general=True)
            assert torch.equal(fast, slow) and torch.equal(fast[..., :3].permute(0, 3, 1, 2), want) and not bool(fast[..., 3].any()), tag
            assert torch.equal(p.flat.cpu(), p.expect(*vals)), tag
    # reading is total: the bits outside the value are ignored in either container
    depth, msb = 10, True
    vals = random_values(9, t, h, w, depth)
    p = Planes16(t, h, w, 'nv12', depth, msb).fill(*vals)
    for v in p.views[:3]:
        v.bitwise_or_(0x3F)                                                     # dirt in the low six bits of a P010 word
    assert torch.equal(ops.frames_from_yuv420p16(p.views, standard).cpu(), ref_planes(vals, standard, depth))
    # a batch: (n,t,...) views, clips one after the other; uint16 views carry the same bits
    p = Planes16(4, h, w, 'i420', 12, False).fill(*random_values(6, 4, h, w, 12))
    v4 = ops.Yuv420Frames16(*[x.unflatten(0, (2, 2)) for x in p.views[:3]], 12, False)
    one = ops.frames_from_yuv420p16(p.views, standard)
    assert torch.equal(ops.frames_from_yuv420p16(v4, standard), one.unflatten(0, (2, 2)))
    if hasattr(torch, 'uint16'):
        pu = Planes16(4, h, w, 'i420', 12, False, dtype=torch.uint16)
        pu.flat.copy_(p.flat)
        assert pu.views.y.dtype == torch.uint16 and torch.equal(ops.frames_from_yuv420p16(pu.views, standard), one)


def crafted_planes(standard, depth, h=64, w=96):
    """(3, 3, h, w): random values in [-0.1, 1.1]; the k / top grid; greys whose luma lands exactly on n + 0.5 (rint ties) mixed with
    saturated primaries (chroma at the range's ends)"""
    k = yuv16_ref.constants(standard, depth)
    g = torch.Generator().manual_seed(17 + depth)
    a = torch.rand((3, h, w), generator=g) * 1.2 - 0.1
    a[:, 0, 0], a[:, 0, 1] = -0.1, 1.1                          # a pixel below black and one above white in every channel
    b = torch.randint(0, k['top'] + 1, (3, h, w), generator=g).float() / float(k['top'])
    n = np.arange(k['yoff'], k['yoff'] + int(k['sy']))
    v = ((n + 0.5 - k['yoff']) / float(k['sy'])).astype(np.float32)
    c = torch.from_numpy(np.resize(v, h * w)).reshape(1, h, w).repeat(3, 1, 1).clone()
    prim = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=torch.float32)
    for j in range(6):
        c[:, 8 * j:8 * j + 8, 48:] = prim[j][:, None, None]
    return torch.stack([a, b, c])


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', yuv16_ref.STANDARDS)
def test_frames_to_yuv420p16_is_the_restatement_and_writes_nothing_else(standard, depth):
    planes = crafted_planes(standard, depth)
    t, _, h, w = planes.shape
    assert float(planes.min()) < 0 and float(planes.max()) > 1
    # the set contains rounding ties (checked on the CPU, from the restatement's own pre-rounding values): halves with an even and
    # with an odd integer part, so that half-to-even differs from both half-up and half-down
    pre = yuv16_ref.pre_round(planes.numpy(), standard, depth)[0]
    tie = pre[(pre - np.floor(pre)) == np.float32(0.5)]
    print(f'{standard} {depth} bit: {tie.size} luma samples on a rounding tie')
    assert (np.floor(tie) % 2 == 0).sum() > 20 and (np.floor(tie) % 2 == 1).sum() > 20
    k = yuv16_ref.constants(standard, depth)
    vals = [torch.from_numpy(x.astype(np.int32)) for x in yuv16_ref.to_yuv16(planes.numpy(), standard, depth, False)]
    assert int(vals[0].min()) == k['yoff'] and int(vals[1].min()) < k['mid'] // 4 and int(vals[2].max()) > k['top'] - k['mid'] // 4
    dplanes = planes.to(dev())
    for msb in (False, True):
        for order, pitch, off, cpitch in layouts(w):
            p = Planes16(t, h, w, order, depth, msb, pitch, off, cpitch)
            ops.frames_to_yuv420p16(dplanes, standard, out=p.views)
            got, want = p.flat.cpu(), p.expect(*vals)       # the samples, zeros outside the value, and 0xA5 everywhere else
            assert torch.equal(got, want), (msb, order, pitch, off, cpitch, int((got != want).sum()))
    for name, (order, d, msb) in yuv16_ref.LAYOUTS.items():
        if d != depth:
            continue
        buf, views = ops.frames_to_yuv420p16(dplanes, standard, name)
        assert buf.shape == (t, h * 3 // 2, w) and buf.dtype == torch.int16 and (views.bit_depth, views.msb_aligned) == (d, msb)
        wy, wcb, wcr = [yuv16_ref.words(v.numpy(), d, msb) for v in vals]
        assert np.array_equal(buf.cpu().numpy().view(np.uint16), yuv16_ref.pack(wy, wcb, wcr, order)), name
        assert all(torch.equal(a, b) for a, b in zip(ops.yuv420p16_views(buf, h, w, name)[:3], views[:3]))
        assert all(torch.equal(a, b) for a, b in zip(ops.yuv420p16_views(buf, h, w, (order, d, msb))[:3], views[:3]))


def test_bad_frames_raise_before_any_gpu_work():
    d = dev()
    z = lambda *s: torch.zeros(s, dtype=torch.int16, device=d)      # noqa: E731
    F16 = ops.Yuv420Frames16
    ok = (z(1, 64, 64), z(1, 32, 32), z(1, 32, 32))
    with pytest.raises(ValueError, match='even'):
        ops.frames_from_yuv420p16(F16(z(1, 65, 64), z(1, 32, 32), z(1, 32, 32)))
    with pytest.raises(ValueError, match='even'):
        ops.yuv420p16_views(z(1, 96, 66), 64, 65, 'p010')
    with pytest.raises(ValueError, match='layout'):
        ops.yuv420p16_views(z(1, 96, 64), 64, 64, 'nv12')
    with pytest.raises(ValueError, match='bit_depth'):
        ops.yuv420p16_views(z(1, 96, 64), 64, 64, ('nv12', 8, False))
    with pytest.raises(TypeError, match='16-bit'):
        ops.yuv420p16_views(z(1, 96, 64).to(torch.uint8), 64, 64, 'p010')
    with pytest.raises(TypeError, match='uint8'):                    # ... and the 8-bit views keep refusing words
        ops.yuv420_views(z(1, 96, 64), 64, 64, 'nv12')
    with pytest.raises(TypeError, match='uint8'):
        ops.frames_from_yuv420(ops.Yuv420Frames(*ok))
    with pytest.raises(TypeError, match='Yuv420Frames16'):
        ops.frames_from_yuv420p16(ops.Yuv420Frames(*[x.to(torch.uint8) for x in ok]))
    with pytest.raises(ValueError, match='h/2'):
        ops.frames_from_yuv420p16(F16(z(1, 64, 64), z(1, 32, 31), z(1, 32, 31)))
    with pytest.raises(ValueError, match='last stride'):
        ops.frames_from_yuv420p16(F16(z(1, 64, 128)[..., ::2], z(1, 32, 32), z(1, 32, 32)))
    with pytest.raises(ValueError, match='interleaved'):
        ops.frames_from_yuv420p16(F16(z(1, 64, 64), z(1, 32, 64)[..., ::2], z(1, 32, 64)[..., ::2]))
    with pytest.raises(TypeError, match='int16'):
        ops.frames_from_yuv420p16(F16(z(1, 64, 64).float(), z(1, 32, 32), z(1, 32, 32)))
    for depth in (8, 11, 16, True):
        with pytest.raises(ValueError, match='bit_depth'):
            ops.frames_from_yuv420p16(F16(*ok, depth))
    with pytest.raises(ValueError, match='yuv_standard'):
        ops.frames_from_yuv420p16(F16(*ok), 'bt2020')
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.frames_from_yuv420p16(F16(*[x.cpu() for x in ok]))
    with pytest.raises(ValueError, match='out is'):
        ops.frames_to_yuv420p16(torch.zeros(1, 3, 64, 64, device=d), out=F16(z(1, 32, 32), z(1, 16, 16), z(1, 16, 16)))


# ------------------------------------------------------------------------------------------------ the forward
def clip16(seed, depth, msb, order, n=1, t=3, h=64, w=64, pitch=None, off=0, values=None):
    """side info of a synthetic clip ('IBP') + its frames as 16-bit planes: clip b in an allocation of its own behind guard bands"""
    c = t8.gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=(73, 66, 80), qp_mode='qp', crf=[15, 35][:n] if n > 1 else 25)
    a = {k: torch.from_numpy(c[k]).to(dev()) for k in t8.SIDE}
    a['values'] = values if values is not None else [random_values(seed + 7 * b, t, h, w, depth) for b in range(n)]
    a['planes'] = [Planes16(t, h, w, order, depth, msb, pitch, off).fill(*a['values'][b]) for b in range(n)]
    return a


def batch_views(a):
    p = a['planes'][0]
    if len(a['planes']) == 1:
        return ops.Yuv420Frames16(*[x[None] for x in p.views[:3]], p.depth, p.msb)
    return ops.Yuv420Frames16(*[torch.stack([q.views[j] for q in a['planes']]) for j in range(3)], p.depth, p.msb)


#         name, cfg, attrs, precision, clip, standard
CASES = [('s64_p010', {}, {}, 'fp32', dict(depth=10, msb=True, order='nv12'), 'bt601-limited'),
         ('any_size_66x70_yuv420p12le', {}, dict(any_size=True), 'fp32', dict(depth=12, msb=False, order='i420', h=66, w=70, pitch=146, off=2),
          'bt709-full'),
         ('fp16_p012', {}, {}, 'fp16', dict(depth=12, msb=True, order='nv21', pitch=134, off=6), 'bt709-limited'),      # the staged conversion
         ('f16x3_yuv420p10le', {}, {}, 'f16x3', dict(depth=10, msb=False, order='i420'), 'bt601-full')]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_yuv16_boundary(case):
    name, cfg_over, attrs, precision, kw, standard = case
    m = t8.build(dict(cfg_over, num_blocks=2), seed=500 + len(name), precision=precision, **attrs)
    a = clip16(seed=61 + len(name), **kw)
    frames = batch_views(a)
    planes = ops.frames_from_yuv420p16(frames, standard)
    n, t, h, w = frames.y.shape
    ref = fwd(m, planes, a).clone()
    lo, hi = float(ref.min()), float(ref.max())
    print(f'{name}: plain output in [{lo:.3f}, {hi:.3f}]')
    assert lo < 0.0 and hi > 1.0                                                 # the clamps are exercised
    got = fwd(m, frames, a, yuv_standard=standard)
    assert got.dtype == torch.float32 and torch.equal(got, ref), 'planes in'
    ref8 = ops.frames_to_rgb8(ref.reshape(n * t, 3, h, w)).reshape(n, t, h, w, 3)
    assert torch.equal(fwd(m, frames, a, yuv_standard=standard, out_dtype=torch.uint8), ref8), 'the uint8 output is what it is today'
    for layout in ops.YUV16_LAYOUTS:                                             # depth and container of the output are its own
        refy = ops.frames_to_yuv420p16(ref, standard, layout)[0]
        t8.poison((n, t, h * 3 // 2, w * 2), torch.uint8)
        goty = fwd(m, frames, a, yuv_standard=standard, out_dtype=layout)
        assert goty.dtype == torch.int16 and goty.shape == (n, t, h * 3 // 2, w)
        assert torch.equal(goty, refy), (layout, int((goty != refy).sum()))
    layout = 'p012' if kw['depth'] == 10 else 'yuv420p10le'
    refy = ops.frames_to_yuv420p16(ref, standard, layout)[0]
    three = fwd(m, frames, a, yuv_standard=standard, out_dtype=(torch.float32, torch.uint8, layout))
    assert isinstance(three, tuple) and len(three) == 3
    assert torch.equal(three[0], ref) and torch.equal(three[1], ref8) and torch.equal(three[2], refy), 'three outputs'
    # 8-bit planes out of 16-bit planes in: ops.frames_to_yuv420 of the same fp32 output
    pair = fwd(m, frames, a, yuv_standard=standard, out_dtype=('nv12', torch.uint8))
    assert pair[0].dtype == torch.uint8 and torch.equal(pair[0], ops.frames_to_yuv420(ref, standard, 'nv12')[0]) and torch.equal(pair[1], ref8)
    for p, v in zip(a['planes'], a['values']):
        assert torch.equal(p.flat.cpu(), p.expect(*v)), 'input planes touched'


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_limited_range_planes_scaled_by_s_give_the_8_bit_forwards_output(precision, depth):
    """the header's identity: samples = s x an 8-bit clip's samples, limited range -> the fp32 output of the existing 8-bit 4:2:0
    forward, bit for bit (the pack launch with fp32; with fp16 the staged conversion too)"""
    m = t8.build(dict(num_blocks=2), seed=777, precision=precision)
    s = 1 << (depth - 8)
    for standard, msb, order in (('bt601-limited', True, 'nv12'), ('bt709-limited', False, 'i420')):
        a8 = t8.yuv_clip(seed=23, t=3, h=64, w=64, layout=order)
        want = fwd(m, t8.batch_views(a8), a8, yuv_standard=standard)
        vals = [[x.to(torch.int32) * s for x in a8['bytes'][0]]]
        a = clip16(seed=23, depth=depth, msb=msb, order=order, values=vals)
        assert all(torch.equal(a[k], a8[k]) for k in t8.SIDE)
        got = fwd(m, batch_views(a), a, yuv_standard=standard)
        assert torch.equal(got, want), (standard, msb, order)


def test_forward_clips_by_pointer_vsr_and_the_custom_op():
    m = t8.build(dict(num_blocks=2))
    std = 'bt709-limited'
    a = clip16(seed=91, depth=10, msb=True, order='nv12', n=2, pitch=134, off=2)
    assert a['planes'][0].flat.data_ptr() != a['planes'][1].flat.data_ptr()
    clips = [(a['planes'][b].views, a['QPs'][b], a['slices'][b], a['mvs'][b], a['base_QPs'][b], a['partitions'][b]) for b in range(2)]
    with torch.no_grad():
        outs = m.forward_clips(clips, yuv_standard=std)
        both = m.forward_clips(clips, out_dtype=(torch.float32, 'yuv420p10le'), yuv_standard=std)
        ones = [m.forward_clips([c], out_dtype=(torch.float32, 'yuv420p10le'), yuv_standard=std)[0] for c in clips]
    ref = fwd(m, ops.frames_from_yuv420p16(batch_views(a), std), a)
    for b in range(2):
        assert outs[b].shape == (1, 3, 3, 64, 64) and torch.equal(outs[b][0], ref[b]), b
        assert torch.equal(both[b][0], ones[b][0]) and torch.equal(both[b][1], ones[b][1]), b      # two by pointer == one at a time
        assert torch.equal(both[b][0][0], ref[b]) and torch.equal(both[b][1][0], ops.frames_to_yuv420p16(ref[b], std, 'yuv420p10le')[0]), b
        assert both[b][1].dtype == torch.int16 and both[b][1].shape == (1, 3, 96, 64)
        p = a['planes'][b]
        assert torch.equal(p.flat.cpu(), p.expect(*a['values'][b]))
    # the custom op is what forward_clips calls: the same tensors from its own entry; its fake kernel knows the shapes
    side = torch.stack([a['slices'].reshape(2, 3).float(), a['QPs'].reshape(2, 3).float(), a['base_QPs'].reshape(2, 3).float()]).cpu().contiguous()
    v = [p.views for p in a['planes']]
    args = (m._op_handle, [x.y for x in v], [x.cb for x in v], [x.cr for x in v], 10, True, list(a['mvs'].float().contiguous()),
            list(a['partitions'].float().contiguous()), side, yuv_ref.STANDARDS.index(std), 5, sorted(ops.YUV16_LAYOUTS).index('yuv420p10le'))
    with torch.no_grad():
        got = torch.ops.pnpvcve.generator_forward_clips_yuv16(*args)
    assert len(got) == 4 and all(torch.equal(got[b], ref[b]) and torch.equal(got[2 + b], both[b][1][0]) for b in range(2))
    # x4 heads: the output planes are 4h x 4w
    mv = t8.build(dict(vsr=True, num_blocks=2), seed=431)
    b = clip16(seed=12, depth=12, msb=False, order='i420')
    f32, y16 = fwd(mv, batch_views(b), b, yuv_standard=std, out_dtype=(torch.float32, 'p012'))
    assert f32.shape == (1, 3, 3, 256, 256) and y16.shape == (1, 3, 384, 256) and y16.dtype == torch.int16
    assert torch.equal(f32, fwd(mv, ops.frames_from_yuv420p16(batch_views(b), std), b))
    assert torch.equal(y16, ops.frames_to_yuv420p16(f32, std, 'p012')[0])


def test_forward_errors_before_any_gpu_work():
    m = t8.build(dict(num_blocks=2))
    a = clip16(seed=3, depth=10, msb=True, order='nv12')
    frames = batch_views(a)
    a8 = t8.yuv_clip(seed=3, t=3, h=64, w=64)
    for layout in ops.YUV16_LAYOUTS:      # 16-bit planes out of 8-bit planes in
        with pytest.raises(ValueError, match='8-bit planes in'):
            fwd(m, t8.batch_views(a8), a8, out_dtype=layout)
        with pytest.raises(ValueError, match='8-bit planes in'):
            m.forward_clips([(a8['planes'][0].views, a8['QPs'][0], a8['slices'][0], a8['mvs'][0], a8['base_QPs'][0], a8['partitions'][0])],
                            out_dtype=(torch.float32, layout))
    with pytest.raises(ValueError, match='out_dtype'):
        fwd(m, frames, a, out_dtype='p016')
    with pytest.raises(ValueError, match='one 4:2:0'):
        fwd(m, frames, a, out_dtype=('p010', 'nv12'))
    with pytest.raises(ValueError, match='yuv_standard'):
        fwd(m, frames, a, yuv_standard='bt2020')
    with pytest.raises(ValueError, match='bit_depth'):
        fwd(m, ops.Yuv420Frames16(*frames[:3], 9, False), a)
    with pytest.raises(ValueError, match='even'):
        fwd(m, ops.Yuv420Frames16(frames.y[..., :63, :], frames.cb, frames.cr, 10, True), a)
    with pytest.raises(ValueError, match='agree'):      # the clips of one call share depth and container
        mk = lambda msb: (ops.Yuv420Frames16(*a['planes'][0].views[:3], 10, msb), a['QPs'][0], a['slices'][0], a['mvs'][0], a['base_QPs'][0],      # noqa: E731
                          a['partitions'][0])
        m.forward_clips([mk(True), mk(False)])
    b = clip16(seed=4, depth=10, msb=False, order='i420', h=66, w=70)
    with pytest.raises(ValueError, match='multiple of 4'):      # 66 x 70 without any_size: the reference's refusal
        fwd(m, batch_views(b), b)
