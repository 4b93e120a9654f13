"""GPU: the 4:2:2 and 4:4:4 chroma formats of the Y'CbCr boundary (include/pnpvcve.h, "Chroma formats"), 8 to 12 bit, every chroma
mode.  The two conversions and the forward's unpacking are held bit for bit to the numpy restatement (tests/yuv_formats_ref.py); the
identities between the formats are checked on the device against the 4:2:0 kernels; the forward on planes is a composition of things
that exist.  Every check is torch.equal or byte-equal: no tolerance.  Planes sit in guard-banded allocations (FPlanes)."""
import numpy as np
import pytest
import torch

import test_gpu_yuv_frames as yf
import yuv_formats_ref as fref
from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
dev, fwd = yf.dev, yf.fwd
GUARD = 64          # samples of 0xA5 bytes in front of and behind every allocation
T = 2
MODES = fref.MODES
# layout name (ffmpeg's), format, plane order ('nv21': Cr first), depth, msb_aligned, standard
CONTAINERS = [('yuv422p', '422', 'i420', 8, False, 'bt601-limited'), ('nv16', '422', 'nv12', 8, False, 'bt709-full'),
              ('nv16-crfirst', '422', 'nv21', 8, False, 'bt709-limited'), ('p210', '422', 'nv12', 10, True, 'bt709-limited'),
              ('yuv422p12le', '422', 'i420', 12, False, 'bt601-full'), ('yuv444p', '444', 'i420', 8, False, 'bt709-limited'),
              ('nv24', '444', 'nv12', 8, False, 'bt601-limited'), ('p410', '444', 'nv12', 10, True, 'bt601-full'),
              ('yuv444p10le', '444', 'i420', 10, False, 'bt709-full')]
IDS = [c[0] for c in CONTAINERS]
# the smallest frames (every clamp at once), one chroma column, one row, several rows of one chroma column; then two blocks of
# threads at an odd pitch and address (8 bit) or an even address that is not 8-byte aligned (16 bit: 3 samples of slack and offset)
SIZES = {'422': [(1, 2, False), (2, 2, False), (1, 6, False), (5, 2, False), (64, 96, True)],
         '444': [(1, 1, False), (1, 5, False), (5, 1, False), (64, 96, True)]}


class FPlanes:
    """t frames of h x w in a format, in one flat device allocation full of 0xA5 bytes; units are SAMPLES (bytes or 16-bit words).
    `off` samples behind the guard band the Y plane of frame 0 starts, rows `pitch` apart; then h chroma rows: interleaved pairs
    ('nv12' | 'nv21' order) or the Cb plane and the Cr plane ('i420'), rows `cpitch` apart, which keeps the Y rows' slack.
    fill / expect take sample VALUES; expect(y, cb, cr) is the whole allocation as it must look after exactly those were written."""

    def __init__(self, t, h, w, container, pitch=None, off=0):
        _, self.fmt, self.order, self.depth, self.msb, _ = container
        self.t, self.h, self.w = t, h, w
        self.sx = _native.YUV_FACTORS[self.fmt][0]
        self.step = 1 if self.order == 'i420' else 2
        self.pitch = pitch = w if pitch is None else pitch
        self.cpitch = self.step * (w // self.sx) + (pitch - w)
        self.y0 = GUARD + off
        self.c0 = self.y0 + h * pitch
        self.frame = h * pitch + h * self.cpitch * (1 if self.step == 2 else 2)
        self.n = self.y0 + t * self.frame + GUARD
        self.dtype = torch.uint8 if self.depth == 8 else torch.int16
        self.flat = self._blank(dev())
        self.views = self._views(self.flat)

    def _blank(self, device):
        return torch.full((self.n * (1 if self.depth == 8 else 2),), 0xA5, dtype=torch.uint8, device=device).view(self.dtype)

    def _views(self, flat):
        t, h, cw, st = self.t, self.h, self.w // self.sx, self.step
        y = flat.as_strided((t, h, self.w), (self.frame, self.pitch, 1), self.y0)
        if st == 2:
            a = flat.as_strided((t, h, cw), (self.frame, self.cpitch, 2), self.c0)
            b = flat.as_strided((t, h, cw), (self.frame, self.cpitch, 2), self.c0 + 1)
            cb, cr = (a, b) if self.order == 'nv12' else (b, a)
        else:
            cb = flat.as_strided((t, h, cw), (self.frame, self.cpitch, 1), self.c0)
            cr = flat.as_strided((t, h, cw), (self.frame, self.cpitch, 1), self.c0 + h * self.cpitch)
        cls8, cls16 = ops._YUV_CLASSES[self.fmt]
        return cls8(y, cb, cr) if self.depth == 8 else cls16(y, cb, cr, self.depth, self.msb)

    def words(self, v):
        """sample values -> what is stored (a CPU tensor of the allocation's dtype)"""
        v = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64)
        if self.depth == 8:
            return torch.from_numpy(v.astype(np.uint8))
        return torch.from_numpy((v << (16 - self.depth if self.msb else 0)).astype(np.uint16).view(np.int16))

    def fill(self, y, cb, cr):
        for dst, src in zip(self.views[:3], (y, cb, cr)):
            dst.copy_(self.words(src))
        return self

    def expect(self, y, cb, cr):
        flat = self._blank('cpu')
        for dst, src in zip(self._views(flat)[:3], (y, cb, cr)):
            dst.copy_(self.words(src))
        return flat


def awkward(container, w):
    """(pitch, offset) in samples: an odd pitch and address for bytes; for words an even address that is not 8-byte aligned"""
    return (w + 7, 1) if container[3] == 8 else (w + 3, 3)


def planes_of(container, t, h, w, awk=False, off=0):
    pitch, o = awkward(container, w) if awk else (None, off)
    return FPlanes(t, h, w, container, pitch, o)


def random_values(seed, container, t, h, w):
    """decoder-like sample values (int32 CPU tensors), a third of them at the range's ends (out-of-gamut triples: the clamp works)"""
    g = torch.Generator().manual_seed(seed)
    top = (1 << container[3]) - 1
    ch, cw = fref.chroma_shape(h, w, container[1])
    out = []
    for hh, ww in ((h, w), (ch, cw), (ch, cw)):
        x = torch.randint(0, top + 1, (t, hh, ww), generator=g, dtype=torch.int32)
        r = torch.rand((t, hh, ww), generator=g)
        out.append(torch.where(r < 1 / 6, torch.zeros_like(x), torch.where(r > 5 / 6, torch.full_like(x, top), x)))
    return out


def from_ref(vals, container, mode):
    return torch.from_numpy(fref.from_planes(*[v.numpy() for v in vals], container[5], container[3], mode, container[1]))


@pytest.mark.parametrize('container', CONTAINERS, ids=IDS)
@pytest.mark.parametrize('mode', MODES)
def test_planes_to_rgb_is_the_restatement_and_reads_only(mode, container):
    std = container[5]
    for h, w, awk in SIZES[container[1]]:
        vals = random_values(100 + h + w, container, T, h, w)
        want = from_ref(vals, container, mode).to(dev())
        p = planes_of(container, T, h, w, awk).fill(*vals)
        got = ops.frames_from_yuv(p.views, std, chroma=mode)
        assert got.shape == (T, 3, h, w) and torch.equal(got, want), (h, w, int((got != want).sum()))
        for general in (False, True):       # the forward's unpacking: the same values as RGB0, the fourth channel zero
            lr4 = ops.pack_lr_yuv(p.views, std, general=general, chroma=mode)
            assert lr4.shape == (T, h, w, 4) and torch.equal(lr4[..., :3].permute(0, 3, 1, 2), want) and not bool(lr4[..., 3].any()), (h, w, general)
        assert torch.equal(p.flat.cpu(), p.expect(*vals)), (h, w, 'the planes or their guard bytes were written')


@pytest.mark.parametrize('container', CONTAINERS, ids=IDS)
@pytest.mark.parametrize('mode', MODES)
def test_rgb_to_planes_is_the_restatement_and_writes_nothing_else(mode, container):
    std, depth, fmt = container[5], container[3], container[1]
    for h, w, awk in SIZES[fmt]:
        g = torch.Generator().manual_seed(7 * h + w)
        x = torch.rand((T, 3, h, w), generator=g) * 1.4 - 0.2
        want = fref.to_planes(x.numpy(), std, depth, mode, fmt)
        p = planes_of(container, T, h, w, awk)
        buf, out = ops.frames_to_yuv(x.to(dev()), std, out=p.views, chroma=mode)
        assert buf is None and out is p.views
        got, exp = p.flat.cpu(), p.expect(*want)      # (guard bytes and row tails included)
        assert torch.equal(got, exp), (h, w, int((got != exp).sum()))


@pytest.mark.parametrize('container', CONTAINERS, ids=IDS)
def test_the_aligned_and_the_general_pack_agree_with_each_other_and_with_the_conversion(container):
    std, fmt = container[5], container[1]
    # 98: no multiple of 4; 97 (4:4:4): an odd width; an offset of 2 samples: the general form only
    cases = [(64, 96, 0), (64, 98, 0), (64, 96, 2)] + ([(64, 97, 0)] if fmt == '444' else [])
    for h, w, off in cases:
        vals = random_values(31 + w + off, container, 3, h, w)
        p = planes_of(container, 3, h, w, off=off).fill(*vals)
        for mode in MODES:
            fast, slow = ops.pack_lr_yuv(p.views, std, chroma=mode), ops.pack_lr_yuv(p.views, std, general=True, chroma=mode)
            assert fast.shape == (3, h, w, 4) and torch.equal(fast, slow), (w, off, mode, int((fast != slow).sum()))
            assert torch.equal(fast[..., :3].permute(0, 3, 1, 2), ops.frames_from_yuv(p.views, std, chroma=mode)), (w, off, mode)
            assert torch.equal(fast[..., :3].permute(0, 3, 1, 2).cpu(), from_ref(vals, container, mode)), (w, off, mode)
        assert torch.equal(p.flat.cpu(), p.expect(*vals))


def test_the_packed_layouts_are_views_of_one_buffer_and_round_trip():
    """ops.yuv_views / empty_yuv / frames_to_yuv with a fresh buffer, every layout name: the buffer's shape, and reading it back gives
    the restatement of what was written"""
    h, w = 6, 8
    x = torch.rand((T, 3, h, w), generator=torch.Generator().manual_seed(5)) * 1.4 - 0.2
    for layout, (fmt, order, depth, msb) in ops.YUV_FORMAT_LAYOUTS.items():
        buf, views = ops.frames_to_yuv(x.to(dev()), 'bt709-limited', layout, chroma='left')
        assert buf.shape == (T, {'422': 2, '444': 3}[fmt] * h, w) and buf.dtype == (torch.uint8 if depth == 8 else torch.int16), layout
        assert ops.yuv_format(views) == fmt and ops.is_yuv(views)
        want = fref.to_planes(x.numpy(), 'bt709-limited', depth, 'left', fmt)
        shift = 16 - depth if msb else 0
        for got, exp in zip(views[:3], want):
            vals = got.cpu().numpy().astype(np.int64) & (0xffff if depth > 8 else 0xff)
            assert np.array_equal(vals >> shift, exp) and not (vals & ((1 << shift) - 1)).any(), layout
        again = ops.yuv_views(buf, h, w, layout)
        assert all(a.data_ptr() == b.data_ptr() and a.stride() == b.stride() for a, b in zip(again[:3], views[:3]))
        back = ops.frames_from_yuv(views, 'bt709-limited', chroma='left')
        assert torch.equal(back.cpu(), torch.from_numpy(fref.from_planes(*want, 'bt709-limited', depth, 'left', fmt)))


# ------------------------------------------------------------------------------------------------ against the 4:2:0 kernels, on the device
def rep(c, ry, rx):
    return c.repeat_interleave(ry, dim=-2).repeat_interleave(rx, dim=-1)


@pytest.mark.parametrize('depth', [8, 10])
def test_the_identities_between_the_formats_hold_against_the_420_kernels(depth):
    std, t, h, w = 'bt601-limited', 2, 64, 96
    c420 = ('i420', '420', 'i420', depth, False, std)
    c422, c444 = ('p', '422', 'i420', depth, False, std), ('p', '444', 'nv12', depth, False, std)
    y, cb, cr = random_values(9, c420, t, h, w)
    if depth == 8:
        p0 = yf.Planes(t, h, w, 'i420').fill(*[v.to(torch.uint8) for v in (y, cb, cr)])
        from420 = lambda mode='replicate': ops.frames_from_yuv420(p0.views, std, chroma=mode)      # noqa: E731
    else:
        import test_gpu_yuv16_frames as y16
        p0 = y16.Planes16(t, h, w, 'i420', depth, False).fill(y, cb, cr)
        from420 = lambda mode='replicate': ops.frames_from_yuv420p16(p0.views, std, chroma=mode)      # noqa: E731
    want = from420()
    # 4:4:4 of chroma repeated 2x2 and 4:2:2 of chroma rows repeated are 4:2:0; 4:4:4 of chroma columns repeated is 4:2:2
    p444 = planes_of(c444, t, h, w).fill(y, rep(cb, 2, 2), rep(cr, 2, 2))
    p422 = planes_of(c422, t, h, w).fill(y, rep(cb, 2, 1), rep(cr, 2, 1))
    assert torch.equal(ops.frames_from_yuv(p444.views, std), want) and torch.equal(ops.frames_from_yuv(p422.views, std), want)
    assert torch.equal(ops.pack_lr_yuv(p422.views, std)[..., :3].permute(0, 3, 1, 2), want)
    v422 = random_values(10, c422, t, h, w)
    q422 = planes_of(c422, t, h, w).fill(*v422)
    q444 = planes_of(c444, t, h, w).fill(v422[0], rep(v422[1], 1, 2), rep(v422[2], 1, 2))
    assert torch.equal(ops.frames_from_yuv(q444.views, std), ops.frames_from_yuv(q422.views, std))
    # on the way out: RGB with every row doubled gives 4:2:2 chroma rows 2j and 2j + 1 equal to the 4:2:0 row j, and one Y plane
    g = torch.Generator().manual_seed(11)
    x = (torch.rand((t, 3, h // 2, w), generator=g) * 1.4 - 0.2).repeat_interleave(2, dim=-2).to(dev())
    lay420, lay422, lay444 = ('i420', 'yuv422p', 'yuv444p') if depth == 8 else ('yuv420p10le', 'yuv422p10le', 'yuv444p10le')
    to420 = ops.frames_to_yuv420 if depth == 8 else ops.frames_to_yuv420p16
    for mode in ('replicate', 'center', 'left'):
        a = to420(x, std, lay420, chroma=mode)[1]
        b = ops.frames_to_yuv(x, std, lay422, chroma=mode)[1]
        c = ops.frames_to_yuv(x, std, lay444, chroma=mode)[1]
        assert torch.equal(b.y, a.y) and torch.equal(c.y, a.y), mode
        for k in (1, 2):
            assert torch.equal(b[k][..., 0::2, :], a[k]) and torch.equal(b[k][..., 1::2, :], a[k]), (mode, k)


# ------------------------------------------------------------------------------------------------ the forward
_MODELS = {}


def model(**cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _MODELS:
        attrs = {k: cfg.pop(k) for k in list(cfg) if k == 'any_size'}
        _MODELS[key] = yf.build(dict(num_blocks=2, **cfg), seed=433, **attrs)
    return _MODELS[key]


def clip_of(seed, container, n=1, t=T, h=64, w=64, awk=False):
    """side info of a synthetic clip + its frames as planes of the container: clip b in an allocation of its own behind guard bands"""
    c = yf.gu.syn.make_clip(seed=seed, n=n, t=t, h=h, w=w, slices=(73, 80), qp_mode='qp', crf=[15, 35][:n] if n > 1 else 25)
    a = {k: torch.from_numpy(c[k]).to(dev()) for k in yf.SIDE}
    a['values'] = [random_values(seed + 7 * b, container, t, h, w) for b in range(n)]
    a['planes'] = [planes_of(container, t, h, w, awk).fill(*a['values'][b]) for b in range(n)]
    return a


def batch_views(a):
    p = a['planes'][0]
    if len(a['planes']) == 1:
        return type(p.views)(*[x[None] for x in p.views[:3]], *p.views[3:])
    return type(p.views)(*[torch.stack([q.views[j] for q in a['planes']]) for j in range(3)], *p.views[3:])


BY_NAME = {c[0]: c for c in CONTAINERS}


@pytest.mark.parametrize('name', ['nv16', 'p210', 'yuv444p', 'yuv444p10le'])
@pytest.mark.parametrize('mode', ['replicate', 'left'])
def test_forward_on_planes_is_the_forward_on_their_conversion_and_writes_their_format(mode, name):
    container = BY_NAME[name]
    m, std = model(), container[5]
    a = clip_of(61, container)
    frames = batch_views(a)
    rgb = ops.frames_from_yuv(frames, std, chroma=mode)
    ref = fwd(m, rgb, a)
    assert ref.shape == (1, T, 3, 64, 64) and float(ref.min()) < 0.0 and float(ref.max()) > 1.0
    assert torch.equal(fwd(m, frames, a, yuv_standard=std, chroma=mode), ref)
    refy = ops.frames_to_yuv(ref, std, name, chroma=mode)[0]
    goty = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype=name)
    assert goty.dtype == refy.dtype and goty.shape == refy.shape == (1, T, {'422': 128, '444': 192}[container[1]], 64) and torch.equal(goty, refy)
    both = fwd(m, frames, a, yuv_standard=std, chroma=mode, out_dtype=(torch.float32, name))
    assert torch.equal(both[0], ref) and torch.equal(both[1], refy)
    assert torch.equal(a['planes'][0].flat.cpu(), a['planes'][0].expect(*a['values'][0]))
    with pytest.raises(ValueError, match='chroma format'):
        fwd(m, frames, a, yuv_standard=std, out_dtype='nv12')
    if container[3] == 8:
        with pytest.raises(ValueError, match='8-bit planes in'):
            fwd(m, frames, a, yuv_standard=std, out_dtype='p210' if container[1] == '422' else 'p410')
    with pytest.raises(ValueError):
        m.forward_ensemble(frames, a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])


def test_forward_x4_writes_planes_of_the_large_frame():
    container = BY_NAME['nv16']
    m, std = model(vsr=True), container[5]
    a = clip_of(63, container)
    frames = batch_views(a)
    ref = fwd(m, ops.frames_from_yuv(frames, std, chroma='left'), a)
    assert ref.shape == (1, T, 3, 256, 256)
    f32, planes = fwd(m, frames, a, yuv_standard=std, chroma='left', out_dtype=(torch.float32, 'nv16'))
    assert torch.equal(f32, ref) and planes.shape == (1, T, 512, 256)
    assert torch.equal(planes, ops.frames_to_yuv(ref, std, 'nv16', chroma='left')[0])


def test_forward_clips_with_two_clips_by_pointer():
    container = BY_NAME['yuv444p10le']
    m, std = model(), container[5]
    a = clip_of(64, container, n=2)
    clips = [(a['planes'][b].views, a['QPs'][b], a['slices'][b], a['mvs'][b], a['base_QPs'][b], a['partitions'][b]) for b in range(2)]
    with torch.no_grad():
        out = m.forward_clips(clips, out_dtype=(torch.float32, 'yuv444p10le'), yuv_standard=std, chroma='center')
    ref = fwd(m, ops.frames_from_yuv(batch_views(a), std, chroma='center'), a)
    refy = ops.frames_to_yuv(ref, std, 'yuv444p10le', chroma='center')[0]
    for b in range(2):
        assert torch.equal(out[b][0][0], ref[b]) and torch.equal(out[b][1][0], refy[b]), b
        assert torch.equal(a['planes'][b].flat.cpu(), a['planes'][b].expect(*a['values'][b]))


@pytest.mark.parametrize('name,h,w', [('yuv422p12le', 66, 70), ('nv24', 67, 69)])
def test_any_size_runs_the_sizes_the_format_admits(name, h, w):
    container = BY_NAME[name]
    m, std = model(any_size=True), container[5]
    a = clip_of(65, container, h=h, w=w, awk=True)
    frames = batch_views(a)
    ref = fwd(m, ops.frames_from_yuv(frames, std, chroma='left'), a)
    f32, planes = fwd(m, frames, a, yuv_standard=std, chroma='left', out_dtype=(torch.float32, name))
    assert f32.shape == (1, T, 3, h, w) and torch.equal(f32, ref)
    assert torch.equal(planes, ops.frames_to_yuv(ref, std, name, chroma='left')[0])
