"""CPU: tests/yuv_formats_ref.py, the numpy restatement of the chroma formats of include/pnpvcve.h ("Chroma formats"), against the
restatement of the 4:2:0 chroma modes it generalises and against the identities the header claims for 4:2:2 and 4:4:4."""
import numpy as np
import pytest

import yuv_chroma_ref as cref
import yuv_formats_ref as fref

F = np.float32
H, W = 12, 20
STD = 'bt709-limited'


def planes_of(seed, depth, fmt, h=H, w=W, lead=(2,)):
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    ch, cw = fref.chroma_shape(h, w, fmt)
    return rng.integers(0, top + 1, lead + (h, w)), rng.integers(0, top + 1, lead + (ch, cw)), rng.integers(0, top + 1, lead + (ch, cw))


def rgb_of(seed, h=H, w=W, lead=(2,)):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, lead + (3, h, w)).astype(F)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def rep(c, ry, rx):
    return np.repeat(np.repeat(c, ry, axis=-2), rx, axis=-1)


@pytest.mark.parametrize('depth', fref.DEPTHS)
@pytest.mark.parametrize('mode', fref.MODES)
def test_at_2_2_it_is_the_420_restatement_exactly(mode, depth):
    y, cb, cr = planes_of(1, depth, '420')
    for std in range(4):
        assert np.array_equal(bits(fref.from_planes(y, cb, cr, std, depth, mode, '420')), bits(cref.from_planes(y, cb, cr, std, depth, mode)))
        x = rgb_of(2 + std)
        for got, want in zip(fref.to_planes(x, std, depth, mode, '420'), cref.to_planes(x, std, depth, mode)):
            assert np.array_equal(got, want)


@pytest.mark.parametrize('depth', fref.DEPTHS)
def test_replicate_identities_between_the_formats(depth):
    y, cb, cr = planes_of(3, depth, '420')
    want = bits(fref.from_planes(y, cb, cr, STD, depth, 0, '420'))
    assert np.array_equal(bits(fref.from_planes(y, rep(cb, 2, 2), rep(cr, 2, 2), STD, depth, 0, '444')), want)
    assert np.array_equal(bits(fref.from_planes(y, rep(cb, 2, 1), rep(cr, 2, 1), STD, depth, 0, '422')), want)
    y, cb, cr = planes_of(4, depth, '422')
    assert np.array_equal(bits(fref.from_planes(y, rep(cb, 1, 2), rep(cr, 1, 2), STD, depth, 0, '444')),
                          bits(fref.from_planes(y, cb, cr, STD, depth, 0, '422')))


@pytest.mark.parametrize('depth', fref.DEPTHS)
def test_444_all_four_modes_are_one_function_both_ways(depth):
    y, cb, cr = planes_of(5, depth, '444', h=5, w=7)
    x = rgb_of(6, 5, 7)
    ins = [bits(fref.from_planes(y, cb, cr, STD, depth, m, '444')) for m in fref.MODES]
    outs = [fref.to_planes(x, STD, depth, m, '444') for m in fref.MODES]
    for m in range(1, 4):
        assert np.array_equal(ins[m], ins[0])
        assert all(np.array_equal(a, b) for a, b in zip(outs[m], outs[0]))
    assert outs[0][1].shape == outs[0][0].shape == (2, 5, 7)


@pytest.mark.parametrize('depth', fref.DEPTHS)
def test_422_left_is_topleft_both_ways_and_differs_from_center(depth):
    y, cb, cr = planes_of(7, depth, '422', h=5)
    x = rgb_of(8, 5)
    assert np.array_equal(bits(fref.from_planes(y, cb, cr, STD, depth, 'left', '422')), bits(fref.from_planes(y, cb, cr, STD, depth, 'topleft', '422')))
    assert not np.array_equal(fref.from_planes(y, cb, cr, STD, depth, 'left', '422'), fref.from_planes(y, cb, cr, STD, depth, 'center', '422'))
    assert not np.array_equal(fref.from_planes(y, cb, cr, STD, depth, 'center', '422'), fref.from_planes(y, cb, cr, STD, depth, 'replicate', '422'))
    a, b, c = (fref.to_planes(x, STD, depth, m, '422') for m in ('left', 'topleft', 'center'))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert not np.array_equal(a[1], c[1]) and np.array_equal(a[0], c[0])
    assert all(np.array_equal(p, q) for p, q in zip(c, fref.to_planes(x, STD, depth, 'replicate', '422')))
    assert a[1].shape == (2, 5, W // 2)


@pytest.mark.parametrize('depth', fref.DEPTHS)
@pytest.mark.parametrize('mode', ('replicate', 'center', 'left'))
def test_row_doubled_rgb_gives_422_chroma_rows_equal_to_the_420_row(mode, depth):
    """exact: (s + s) * 0.25 = s * 0.5 for the box mean of two equal rows, and the co-sited row filter is the same expression"""
    x = np.repeat(rgb_of(9, H // 2), 2, axis=-2)
    y2, cb2, cr2 = fref.to_planes(x, STD, depth, mode, '422')
    y0, cb0, cr0 = fref.to_planes(x, STD, depth, mode, '420')
    for c2, c0 in ((cb2, cb0), (cr2, cr0)):
        assert np.array_equal(c2[..., 0::2, :], c0) and np.array_equal(c2[..., 1::2, :], c0)
    assert np.array_equal(y2, y0)


def test_the_y_plane_is_the_same_for_every_format():
    x = rgb_of(10)
    for depth in fref.DEPTHS:
        for mode in fref.MODES:
            ys = [fref.to_planes(x, 'bt601-full', depth, mode, f)[0] for f in fref.FORMAT_NAMES]
            assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])


@pytest.mark.parametrize('mode', fref.MODES[1:])
def test_a_chroma_ramp_across_upsamples_to_the_line_through_the_samples_positions_at_422(mode):
    """C[i] = a + b i on the factor-2 axis -> a + b (x - off) / 2 away from the clamped edges; times 16 it is an integer"""
    n, a, b = 16, 100, 6
    c = np.broadcast_to(a + b * np.arange(n), (3, n)) - 128
    up = fref.upsample16(c, mode, '422')
    assert up.shape == (3, 2 * n)
    off2 = 0 if cref.cosited(mode)[1] else 1          # twice the offset
    x = np.arange(2 * n)
    want = 16 * (a - 128) + 8 * b * x - 4 * b * off2
    assert np.array_equal(up[:, 2:-2], np.broadcast_to(want, (3, 2 * n))[:, 2:-2])
    # and down a 4:2:2 or 4:4:4 plane nothing is interpolated: rows are taken as they are, with weight 4 of the 16
    rows = np.arange(5)[:, None] * 7 + np.zeros((5, 4), int)
    assert np.array_equal(fref.upsample16(rows, mode, '444'), 16 * rows)
    assert np.array_equal(fref.upsample16(rows, mode, '422')[:, ::2][:, :1], 16 * rows[:, :1])
