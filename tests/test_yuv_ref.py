"""CPU: the numpy restatement of the 4:2:0 boundary's arithmetic (tests/yuv_ref.py) against the float64 definition of
include/pnpvcve.h, over all 2^24 (Y, Cb, Cr) triples of each standard, and the RGB -> bytes direction on crafted values."""
import numpy as np
import pytest

import yuv_ref

F = np.float32
# in-gamut triples (unclamped float32 RGB inside [0, 1]) per standard: the round-trip identity is asserted on exactly these, and the
# count keeps the mask from silently emptying
IN_GAMUT = {'bt601-limited': 2596344, 'bt601-full': 3917576, 'bt709-limited': 2689428, 'bt709-full': 4058320}


def _sweep(standard):
    """-> (max |float32 - float64| of the clamped RGB, in-gamut count, round-trip failures) over all 2^24 triples"""
    cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    err, count, fails = 0.0, 0, 0
    step = 16
    for y0 in range(0, 256, step):
        Y = np.broadcast_to(np.arange(y0, y0 + step, dtype=np.uint8)[:, None, None], (step, 256, 256))
        Cb, Cr = np.broadcast_to(cb, Y.shape), np.broadcast_to(cr, Y.shape)
        raw = yuv_ref.rgb_from_bytes(Y, Cb, Cr, standard, clamp=False)
        rgb = np.clip(raw, F(0), F(1))
        ref = np.clip(yuv_ref.rgb_from_bytes_f64(Y, Cb, Cr, standard), 0.0, 1.0)
        err = max(err, float(np.abs(rgb.astype(np.float64) - ref).max()))
        inside = ((raw >= 0) & (raw <= 1)).all(axis=-1)
        count += int(inside.sum())
        # a 2x2 block of four equal pixels per triple: (3, 2, 2 N) planes
        px = rgb[inside]                                           # (N, 3)
        planes = np.repeat(np.repeat(px.T[:, None, :], 2, axis=1), 2, axis=2)
        y8, cb8, cr8 = yuv_ref.frames_to_yuv420(planes, standard)
        good = (y8 == Y[inside][None, :].repeat(2, 0).repeat(2, 1)).all(axis=0).reshape(-1, 2).all(axis=1)
        good &= (cb8[0] == Cb[inside]) & (cr8[0] == Cr[inside])
        fails += int((~good).sum())
    return err, count, fails


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_float32_restatement_against_the_float64_definition_over_all_triples(standard):
    err, count, fails = _sweep(standard)
    print(f'{standard}: max |f32 - f64| = {err:.3e}, in gamut {count}, round-trip failures {fails}')
    assert err <= 5e-7
    assert count == IN_GAMUT[standard]
    assert fails == 0


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_anchors(standard):
    full = standard.endswith('full')
    one = lambda *t: yuv_ref.rgb_from_bytes(*[np.array([v], np.uint8) for v in t], standard)[0]
    black = one(0 if full else 16, 128, 128)
    white = one(255 if full else 235, 128, 128)
    assert (black == 0).all()
    assert (white == (F(1.0) if full else F(0.99999994))).all()
    # below black / above white clamp
    assert (one(0, 128, 128) == 0).all() and (one(255, 128, 128) == 1).all()
    k = yuv_ref.constants(standard)
    if standard == 'bt601-limited':      # the luma the metrics use: 65.481 / 128.553 / 24.966
        for name, want in (('kr', 65.481), ('kg', 128.553), ('kb', 24.966)):
            assert abs(float(k[name]) * 219.0 - want) < 1e-4


def test_replication_and_layouts():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (2, 4, 6), dtype=np.uint8)
    cb, cr = rng.integers(0, 256, (2, 2, 3), dtype=np.uint8), rng.integers(0, 256, (2, 2, 3), dtype=np.uint8)
    out = yuv_ref.frames_from_yuv420(y, cb, cr, 0)
    assert out.shape == (2, 3, 4, 6) and out.dtype == F
    for yy in range(4):
        for xx in range(6):
            want = yuv_ref.rgb_from_bytes(y[:, yy, xx], cb[:, yy >> 1, xx >> 1], cr[:, yy >> 1, xx >> 1], 0)
            assert (out[:, :, yy, xx] == want).all()
    nv12 = yuv_ref.pack(y, cb, cr, 'nv12', 8)
    assert nv12.shape == (2, 6, 8) and (nv12[:, 4:, 0:6:2] == cb).all() and (nv12[:, 4:, 1:6:2] == cr).all() and (nv12[..., 6:] == 0).all()
    nv21 = yuv_ref.pack(y, cb, cr, 'nv21')
    assert (nv21[:, 4:, 0::2] == cr).all() and (nv21[:, 4:, 1::2] == cb).all()
    i420 = yuv_ref.pack(y, cb, cr, 'i420').reshape(2, -1)
    assert (i420[:, 24:30].reshape(2, 2, 3) == cb).all() and (i420[:, 30:36].reshape(2, 2, 3) == cr).all()


@pytest.mark.parametrize('standard', yuv_ref.STANDARDS)
def test_rgb_to_bytes_ties_clamps_and_summation_order(standard):
    k = yuv_ref.constants(standard)
    grey = lambda v: np.full((3, 2, 2), v, F)
    # values below 0 and above 1 are clamped BEFORE the luma: the bytes of 0 and of 1
    lo, hi = yuv_ref.frames_to_yuv420(grey(-0.2), standard), yuv_ref.frames_to_yuv420(grey(1.2), standard)
    assert [int(p.flat[0]) for p in lo] == [k['yoff'], 128, 128]
    white = int(np.rint(F(k['yoff']) + k['sy'] * ((k['kr'] + k['kg']) + k['kb'])))
    assert [int(p.flat[0]) for p in hi] == [white, 128, 128] and white in (235, 255)
    # rint ties go to the even byte: a grey g with yoff + sy * yl exactly n + 0.5
    hits = 0
    for n in range(k['yoff'], k['yoff'] + 200):
        g = F((n + 0.5 - k['yoff']) / float(k['sy']))
        yl = (k['kr'] * g + k['kg'] * g) + k['kb'] * g
        if F(k['yoff']) + k['sy'] * yl == F(n + 0.5):
            hits += 1
            assert int(yuv_ref.frames_to_yuv420(grey(g), standard)[0].flat[0]) == (n if n % 2 == 0 else n + 1)
    assert hits > 0
    # the box mean adds left + right of each row first, then the rows: an order that shows in float32
    rng = np.random.default_rng(3)
    for _ in range(2000):
        x = rng.random((3, 2, 2)).astype(F)
        x[1:] = 0                                              # red only: pr large, four different values
        r = x[0]
        yl = (k['kr'] * r + k['kg'] * F(0)) + k['kb'] * F(0)
        pr = (r - yl) * k['ipr']
        a = ((pr[0, 0] + pr[0, 1]) + (pr[1, 0] + pr[1, 1])) * F(0.25)
        want = int(np.clip(np.rint(F(128) + k['sc'] * a), 0, 255))
        assert int(yuv_ref.frames_to_yuv420(x, standard)[2].flat[0]) == want
