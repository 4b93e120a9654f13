"""CPU: the numpy restatement of the 10 / 12-bit 4:2:0 boundary (tests/yuv16_ref.py): the limited-range identity that ties it to the
pinned 8-bit restatement, grey ramps through to -> from -> to, the anchors and the two containers."""
import numpy as np
import pytest

import yuv16_ref
import yuv_ref

F = np.float32
LIMITED = ('bt601-limited', 'bt709-limited')


def _planes8(seed, shape=(2, 16, 24)):
    rng = np.random.default_rng(seed)
    t, h, w = shape
    y = rng.integers(0, 256, (t, h, w), dtype=np.uint8)
    cb, cr = rng.integers(0, 256, (t, h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (t, h // 2, w // 2), dtype=np.uint8)
    # every byte value of each plane at least once
    y.reshape(-1)[:256] = np.arange(256)
    cb.reshape(-1)[:192] = np.arange(192)
    cr.reshape(-1)[:192] = np.arange(64, 256)
    return y, cb, cr


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', LIMITED)
def test_limited_range_planes_scaled_by_s_convert_to_the_8_bit_rgb_bit_for_bit(standard, depth):
    s = 1 << (depth - 8)
    y, cb, cr = _planes8(depth)
    want = yuv_ref.frames_from_yuv420(y, cb, cr, standard)
    got = yuv16_ref.from_yuv16(*(p.astype(np.uint16) * s for p in (y, cb, cr)), standard, depth)
    assert got.dtype == F and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and over every (Y, Cb, Cr) byte triple on a lattice of chroma, not only the random frame
    Y = np.arange(256, dtype=np.uint8)[:, None, None]
    C = np.arange(0, 256, 5, dtype=np.uint8)
    Y, Cb, Cr = np.broadcast_arrays(Y, C[None, :, None], C[None, None, :])
    a = yuv_ref.rgb_from_bytes(Y, Cb, Cr, standard)
    b = yuv16_ref.rgb_from_values(Y.astype(np.int32) * s, Cb.astype(np.int32) * s, Cr.astype(np.int32) * s, standard, depth)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
def test_every_limited_range_constant_is_the_8_bit_one_times_a_power_of_two(depth):
    s = F(1 << (depth - 8))
    for standard in LIMITED:
        k8, k = yuv_ref.constants(standard), yuv16_ref.constants(standard, depth)
        for name in ('cy', 'crv', 'cbu', 'cgu', 'cgv'):
            assert k[name] * s == k8[name]
        for name in ('sy', 'sc'):
            assert k[name] == k8[name] * s
        assert k['yoff'] == k8['yoff'] * int(s) and k['mid'] == 128 * int(s)
        for name in ('kr', 'kg', 'kb', 'ipb', 'ipr'):
            assert k[name] == k8[name]
    for standard in ('bt601-full', 'bt709-full'):      # no such identity in full range
        assert yuv16_ref.constants(standard, depth)['cy'] * s != yuv_ref.constants(standard)['cy']


@pytest.mark.parametrize('msb', (False, True))
@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', yuv16_ref.STANDARDS)
def test_grey_ramps_round_trip_exactly(standard, depth, msb):
    k = yuv16_ref.constants(standard, depth)
    full = standard.endswith('full')
    lo, hi = (0, k['top']) if full else (k['yoff'], k['yoff'] + 219 * (1 << (depth - 8)))
    codes = np.arange(lo, hi + 1, dtype=np.int32)
    n = -(-codes.size // 4) * 4
    ramp = np.resize(codes, n).reshape(1, 2, n // 2)            # one frame of two rows of an even width: every code of the range
    y = yuv16_ref.words(ramp, depth, msb)
    mid = yuv16_ref.words(np.full((1, 1, n // 4), k['mid']), depth, msb)
    planes = yuv16_ref.from_yuv16(y, mid, mid, standard, depth, msb)
    assert (planes[:, 0] == planes[:, 1]).all() and (planes[:, 0] == planes[:, 2]).all()      # grey
    y2, cb2, cr2 = yuv16_ref.to_yuv16(planes, standard, depth, msb)
    assert np.array_equal(y2, y) and (yuv16_ref.values(cb2, depth, msb) == k['mid']).all() and (yuv16_ref.values(cr2, depth, msb) == k['mid']).all()
    again = yuv16_ref.from_yuv16(y2, cb2, cr2, standard, depth, msb)
    assert np.array_equal(again.view(np.uint32), planes.view(np.uint32))


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', yuv16_ref.STANDARDS)
def test_anchors(standard, depth):
    k = yuv16_ref.constants(standard, depth)
    full = standard.endswith('full')
    s = 1 << (depth - 8)
    one = lambda *t: yuv16_ref.rgb_from_values(*[np.array([v], np.int32) for v in t], standard, depth)[0]
    black = one(0 if full else 16 * s, k['mid'], k['mid'])
    white = one(k['top'] if full else 235 * s, k['mid'], k['mid'])
    assert (black == 0).all()
    assert (white == (F(1.0) if full else F(0.99999994))).all()      # the 8-bit note's value, by the identity
    assert (one(0, k['mid'], k['mid']) == 0).all() and (one(k['top'], k['mid'], k['mid']) == 1).all()
    grey = lambda v: np.full((3, 2, 2), v, F)
    lo, hi = yuv16_ref.to_yuv16(grey(-0.2), standard, depth), yuv16_ref.to_yuv16(grey(1.2), standard, depth)
    assert [int(p.flat[0]) for p in lo] == [k['yoff'], k['mid'], k['mid']]
    assert [int(p.flat[0]) for p in hi] == [k['top'] if full else 235 * s, k['mid'], k['mid']]


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
def test_the_containers_agree_after_alignment(depth):
    rng = np.random.default_rng(depth)
    raw = rng.integers(0, 1 << 16, (2, 8, 12), dtype=np.uint16)       # words with every bit in use: reading is total
    rawc = rng.integers(0, 1 << 16, (2, 2, 4, 6), dtype=np.uint16)
    top = (1 << depth) - 1
    lo = [yuv16_ref.values(p, depth, False) for p in (raw, rawc[0], rawc[1])]
    hi = [yuv16_ref.values(p, depth, True) for p in (raw, rawc[0], rawc[1])]
    assert all((v >= 0).all() and (v <= top).all() for v in lo + hi)
    assert np.array_equal(lo[0], raw.astype(np.int32) & top) and np.array_equal(hi[0], raw.astype(np.int32) >> (16 - depth))
    # the same values in either container convert alike, and are written back with zeros outside the value
    vals = [rng.integers(0, top + 1, p.shape) for p in (raw, rawc[0], rawc[1])]
    a = yuv16_ref.from_yuv16(*[yuv16_ref.words(v, depth, False) for v in vals], 'bt709-full', depth, False)
    b = yuv16_ref.from_yuv16(*[yuv16_ref.words(v, depth, True) for v in vals], 'bt709-full', depth, True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    planes = rng.random((2, 3, 8, 12)).astype(F)
    wl, wh = yuv16_ref.to_yuv16(planes, 'bt601-limited', depth, False), yuv16_ref.to_yuv16(planes, 'bt601-limited', depth, True)
    for l, h in zip(wl, wh):
        assert l.dtype == np.uint16 and (l <= top).all() and (h & ((1 << (16 - depth)) - 1) == 0).all()
        assert np.array_equal(h >> (16 - depth), l)
    for name, (order, d, msb) in yuv16_ref.LAYOUTS.items():
        assert (name.startswith('p0')) == msb and str(d) in name
    buf = yuv16_ref.pack(*wl, 'nv12', 14)
    assert buf.shape == (2, 12, 14) and (buf[:, 8:, 0:12:2] == wl[1]).all() and (buf[:, 8:, 1:12:2] == wl[2]).all() and (buf[..., 12:] == 0).all()
