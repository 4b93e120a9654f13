"""CPU: tests/yuv_chroma_ref.py, the numpy restatement of the chroma modes of include/pnpvcve.h, against the pinned restatements of the
default boundary and against the geometry the header claims for each mode."""
import numpy as np
import pytest

import yuv16_ref
import yuv_chroma_ref as cref
import yuv_ref

F = np.float32
H, W = 12, 20


def planes_of(seed, depth, h=H, w=W, lead=(2,)):
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    return (rng.integers(0, top + 1, lead + (h, w)), rng.integers(0, top + 1, lead + (h // 2, w // 2)),
            rng.integers(0, top + 1, lead + (h // 2, w // 2)))


def rgb_of(seed, h=H, w=W, lead=(2,)):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, lead + (3, h, w)).astype(F)


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_mode_0_is_the_pinned_8_bit_boundary_bit_for_bit(standard):
    y, cb, cr = (p.astype(np.uint8) for p in planes_of(1, 8))
    assert np.array_equal(cref.from_planes(y, cb, cr, standard, 8, 'replicate').view(np.uint32),
                          yuv_ref.frames_from_yuv420(y, cb, cr, standard).view(np.uint32))
    x = rgb_of(2)
    for got, want in zip(cref.to_planes(x, standard, 8, 0), yuv_ref.frames_to_yuv420(x, standard)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize('depth', yuv16_ref.DEPTHS)
@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_mode_0_is_the_pinned_16_bit_boundary_bit_for_bit(standard, depth):
    y, cb, cr = (p.astype(np.uint16) for p in planes_of(3, depth))
    assert np.array_equal(cref.from_planes(y, cb, cr, standard, depth, 0).view(np.uint32),
                          yuv16_ref.from_yuv16(y, cb, cr, standard, depth).view(np.uint32))
    x = rgb_of(4)
    for got, want in zip(cref.to_planes(x, standard, depth, 0), yuv16_ref.to_yuv16(x, standard, depth)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize('depth', cref.DEPTHS)
def test_center_writes_what_replicate_writes_and_reads_otherwise(depth):
    x = rgb_of(5)
    for a, b in zip(cref.to_planes(x, 'bt709-limited', depth, 'center'), cref.to_planes(x, 'bt709-limited', depth, 'replicate')):
        assert np.array_equal(a, b)
    y, cb, cr = planes_of(6, depth)
    assert not np.array_equal(cref.from_planes(y, cb, cr, 0, depth, 'center'), cref.from_planes(y, cb, cr, 0, depth, 'replicate'))
    # the written planes of the two co-sited modes differ from the box mean's and from each other, in chroma only
    out = {m: cref.to_planes(x, 0, depth, m) for m in cref.MODES}
    assert all(np.array_equal(out[m][0], out['replicate'][0]) for m in cref.MODES)
    assert not np.array_equal(out['left'][1], out['replicate'][1]) and not np.array_equal(out['left'][2], out['topleft'][2])


@pytest.mark.parametrize('mode', cref.MODES[1:])
def test_a_chroma_ramp_upsamples_to_the_line_through_the_samples_positions(mode):
    """C[i] = a + b i -> a + b (x - off) / 2 at luma index x, off = 0 on a co-sited axis and 1/2 on a midway one, away from the clamped
    edge; a mirrored or mis-sited filter misses this"""
    n, a, b = 9, 100, 8
    yco, xco = cref.cosited(mode)
    ramp = a + b * np.arange(n)
    for axis, co in ((-1, xco), (-2, yco)):
        c = np.broadcast_to(ramp, (n, n)) if axis == -1 else np.broadcast_to(ramp[:, None], (n, n))
        up = cref.upsample16(c, mode)
        x = np.arange(2 * n)
        want16 = 16 * a + (8 * b * x if co else 4 * b * (2 * x - 1))        # 16 (a + b (x - off) / 2), an integer
        inner = slice(0 if co else 1, 2 * n - 1)                               # the first midway index and the last index clamp
        line = np.moveaxis(up, axis, -1)
        assert np.array_equal(line[..., inner], np.broadcast_to(want16[inner], line[..., inner].shape)), (mode, axis)
        # at the clamped edges the nearest sample is repeated
        assert np.all(line[..., -1] == 16 * ramp[-1]) and np.all(line[..., 0] == 16 * ramp[0])
    # the other axis of a ramp is constant: nothing leaks across
    assert np.array_equal(cref.upsample16(np.broadcast_to(ramp, (n, n)), mode)[0], cref.upsample16(np.broadcast_to(ramp, (n, n)), mode)[-1])


@pytest.mark.parametrize('mode', cref.MODES)
def test_a_pixel_ramp_downsamples_to_its_value_at_the_samples_position(mode):
    """p[x] = a + b x -> sample i = a + b (2i + off): exact in fp32 for small integers"""
    n, a, b = 8, 3.0, 2.0
    yco, xco = cref.cosited(mode)
    ramp = (a + b * np.arange(2 * n)).astype(F)
    i = np.arange(n)
    for axis, co in ((-1, xco), (-2, yco)):
        p = np.broadcast_to(ramp, (2 * n, 2 * n)) if axis == -1 else np.broadcast_to(ramp[:, None], (2 * n, 2 * n))
        got = np.moveaxis(cref.downsample(p, mode), axis, -1)
        want = (a + b * (2 * i + (0.0 if co else 0.5))).astype(F)
        inner = slice(1 if co else 0, n)                                       # sample 0 of a co-sited axis clamps its left tap
        assert np.array_equal(got[..., inner], np.broadcast_to(want[inner], got[..., inner].shape)), (mode, axis)
        if co:
            assert np.all(got[..., 0] == F((3 * ramp[0] + ramp[1]) * 0.25))       # taps 0, 0, 1


@pytest.mark.parametrize('mode', cref.MODES)
def test_weights_sum_to_16_with_every_clamp_at_a_one_sample_chroma_plane(mode):
    assert np.array_equal(cref.upsample16(np.ones((1, 1), int), mode), np.full((2, 2), 16))
    assert np.array_equal(cref.upsample16(np.full((1, 1), -77), mode), np.full((2, 2), -77 * 16))
    assert np.array_equal(cref.upsample16(np.ones((3, 5), int), mode), np.full((6, 10), 16))
    for n in (1, 2, 5):
        for co in (False, True):
            i0, w0, i1, w1 = cref.taps(n, co)
            assert np.all(w0 + w1 == 4) and i0.min() >= 0 and i1.min() >= 0 and i0.max() < n and i1.max() < n
    # a 2x2 frame converts like one pixel's chroma on all four pixels, whatever the mode
    y, cb, cr = np.array([[16, 235], [100, 200]]), np.array([[90]]), np.array([[240]])
    assert np.array_equal(cref.from_planes(y, cb, cr, 0, 8, mode), cref.from_planes(y, cb, cr, 0, 8, 0))


@pytest.mark.parametrize('mode', cref.MODES)
def test_u16_is_exact_in_fp32_at_12_bit(mode):
    rng = np.random.default_rng(7)
    c = rng.choice(np.array([0, 1, 2047, 2048, 4094, 4095]), (40, 40)) - 2048
    u16 = cref.upsample16(c, mode)
    assert np.abs(u16).max() <= 16 * 2048 < 2 ** 16
    u = u16.astype(F) * F(0.0625)
    assert np.array_equal(u.astype(np.float64) * 16.0, u16.astype(np.float64))


@pytest.mark.parametrize('mode', cref.MODES)
@pytest.mark.parametrize('depth,s', [(10, 4), (12, 16)])
def test_the_limited_range_identity_holds_in_every_mode(mode, depth, s):
    y, cb, cr = planes_of(8, 8)
    for standard in ('bt601-limited', 'bt709-limited'):
        want = cref.from_planes(y, cb, cr, standard, 8, mode)
        got = cref.from_planes(s * y, s * cb, s * cr, standard, depth, mode)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (standard, mode)
