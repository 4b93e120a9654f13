"""CPU: keeps tests/dcn_ref.py honest -- the float64 reference against the oracle, the census of the main case (every sample
class and every wave class is populated, so the GPU tests do exercise the edges they claim to) and the sensitivity of the inputs
(a kernel wrong at one class, or wrong in one of four classic ways, would land far outside the tolerances)."""
import functools

import numpy as np
import pytest
import torch

import dcn_ref as R
from oracle import cpu_ref

H, W = 44, 52


@functools.lru_cache(maxsize=None)
def main(with_flow):
    c = R.dcn_case('main_44x52')
    if not with_flow:
        c['flow'] = None
    b = R.dcn_bounds(**c)
    classes, waves = R.dcn_census(c['offset'], c['flow'], H, W)
    return c, b, classes, waves


def oracle_f64(c):
    T = torch.from_numpy
    off = T(R._offsets_f32(c['offset'], c['flow'], *c['x'].shape[:2]).reshape(1, 288, *c['x'].shape[:2]).copy()).double()
    x = T(np.ascontiguousarray(c['x'].transpose(2, 0, 1))[None]).double()
    out = cpu_ref.modulated_deform_conv2d(x, off, torch.sigmoid(T(c['mask_logits'])[None].double()), T(c['weight']).double(),
                                          T(c['bias']).double(), 16)
    return out[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize('name', ['main_44x52', 'flow_folded', 'saturation'] + ['geo_%dx%d' % g for g in R.GEOMETRY])
def test_reference_equals_the_oracle_in_float64(name):
    """two independent restatements (numpy here, torch in oracle/cpu_ref.py, whose degenerate cases test_oracle_dcn.py pins to
    ATen) agree to 1e-12 (relative to the output scale where the saturation case's 1e6 activations raise it)."""
    c = R.dcn_case(name)
    ref = R.dcn_reference(**c)
    assert ref.shape == c['x'].shape and ref.dtype == np.float64
    assert np.abs(ref - oracle_f64(c)).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_flow_folded_and_strip_walk_are_the_main_case_rearranged():
    m, f = R.dcn_case('main_44x52'), R.dcn_case('flow_folded')
    assert f['flow'] is None
    assert np.array_equal(R.dcn_reference(**m), R.dcn_reference(**f))          # same sample positions, bit for bit
    grid = 16
    s = R.dcn_case('strip_walk', grid=grid)
    h, w = s['x'].shape[:2]
    tiles = 3 * ((w + 15) // 16)
    assert h == 20 and w % 16 == 12 and tiles >= 2 * grid + 8 > tiles - 3
    assert np.array_equal(s['offset'][:, :, 52:104], m['offset'][:, :20]) and np.array_equal(s['flow'][:, :, :52], m['flow'][:, :20])


def test_lattice_makes_every_sample_position_exact():
    c = R.dcn_case('main_44x52')
    off = R._offsets_f32(c['offset'], c['flow'], H, W)
    small = np.abs(off) < 1e6
    assert np.array_equal((off * 8)[small], np.round(off * 8)[small])
    exact = c['offset'].reshape(16, 9, 2, H, W).astype(np.float64) + c['flow'][::-1][None, None].astype(np.float64)
    assert np.array_equal(off[small].astype(np.float64), exact[small])          # the fp32 sum offset + flow lost nothing
    p32, p64 = R._positions(off, H, W, np.float32), R._positions(off, H, W, np.float64)
    assert np.array_equal(p32[0][small[:, :, 0]].astype(np.float64), p64[0][small[:, :, 0]])
    assert np.array_equal(p32[1][small[:, :, 1]].astype(np.float64), p64[1][small[:, :, 1]])


@pytest.mark.parametrize('with_flow', [False, True], ids=['noflow', 'flow'])
def test_census_of_the_main_case(with_flow):
    c, b, classes, waves = main(with_flow)
    counts = R.census_counts(classes, waves)
    print(counts)
    assert set(classes) == set(R.TAKEN_CLASSES) | set(R.UNTAKEN_CLASSES)
    for name in classes:
        assert counts[name] >= 32, (name, counts[name])
    for name in ('wave_none', 'wave_mixed', 'wave_all'):
        assert counts[name] >= 4, (name, counts[name])
    # the classes partition the samples the way the kernel's paths do
    win = classes['win_frac'] | classes['win_int']
    glob = classes['glob_near'] | classes['glob_other']
    assert not (win & glob).any() and not ((win | glob) & classes['far']).any() and (win | glob | classes['far']).all()
    assert not (classes['exact_-1'] & ~classes['far']).any() and not (classes['exact_H_or_W'] & ~classes['far']).any()
    # ragged last tile row (4 of 8) and column (4 of 16)
    assert H % 8 == 4 and W % 16 == 4


def test_census_of_the_small_frames_runs():
    for g in R.GEOMETRY:
        c = R.dcn_case('geo_%dx%d' % g)
        classes, waves = R.dcn_census(c['offset'], c['flow'], *g)
        live = -(-g[0] // 2) * -(-g[1] // 16) * 2 * 9
        assert sum(waves.values()) == live, (g, waves)


@pytest.mark.parametrize('with_flow', [False, True], ids=['noflow', 'flow'])
def test_every_sample_class_moves_the_output(with_flow):
    """A kernel that lost the samples of ONE class would miss the fp16 tolerance tenfold at 8 or more pixels.  For the classes
    of samples that are taken this is dcn_reference(drop=class).  A sample that is NOT taken (far, exactly -1, exactly H / W)
    contributes zero whether dropped or not, so there the wrong kernel is the one that reads it after all, with clamped
    addresses: dcn_reference(replicate=class)."""
    c, b, classes, waves = main(with_flow)
    for name in R.TAKEN_CLASSES + R.UNTAKEN_CLASSES:
        kw = dict(drop=classes[name]) if name in R.TAKEN_CLASSES else dict(replicate=classes[name])
        d = np.abs(R.dcn_reference(**c, **kw) - b['ref64']).max(axis=2)
        n = int((d > 10 * b['tol16']).sum())
        print(name, 'pixels off by > 10 tol16:', n, 'max', d.max())
        assert n >= 8, (name, n)


@pytest.mark.parametrize('with_flow', [False, True], ids=['noflow', 'flow'])
@pytest.mark.parametrize('variant', R.VARIANTS[1:])
def test_wrong_variants_are_far_outside_the_fp32_tolerance(variant, with_flow):
    """dy / dx swapped, `<= H-1` for `< H`, `>= 0` for `> -1`, border replicate for zeros."""
    c, b, classes, waves = main(with_flow)
    d = np.abs(R.dcn_reference(**c, variant=variant) - b['ref64']).max()
    print(variant, d, 'tol32', b['tol32'])
    assert d > 100 * b['tol32']


def test_fp16_operand_rule_saturates_and_rounds_to_nearest_even():
    v = np.array([1e6, -1e6, 65504.0, 65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25])
    assert np.array_equal(R._round_f16(v), [65504.0, -65504.0, 65504.0, 65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0])
    c = R.dcn_case('saturation')
    r = R.dcn_reference(**c, operands='fp16')
    assert np.isfinite(r).all() and np.abs(r).max() > 1e3


def test_tolerances_come_out_where_the_formats_put_them():
    """tol32 a few fp32 ulp of a 576-term sum of O(0.03) products, tol16 a few fp16 tie flips of one product -- both far below
    the bounds the suite had before (5e-5; 4e-3 * scale)."""
    for with_flow in (False, True):
        b = main(with_flow)[1]
        print({k: v for k, v in b.items() if not k.startswith('ref')})
        assert 1e-7 < b['e32'] < 2e-6 and b['tol32'] == 16 * b['e32']
        assert 0 < b['n16'] < 0.06 * 2.0 ** -10 * 2 and b['tol16'] == b['tol32'] + 4 * b['n16']
