"""CPU: keeps tests/warp_ref.py honest -- the float64 reference against the oracle, against ATen's grid_sample and against the
reference's committed goldens; the census of every case (the GPU tests do exercise the edges, ties and tails they claim to); the
deviation from ATen on non-finite vectors, pinned to exactly those pixels; and the sensitivity of the inputs (a kernel wrong in one
of six classic ways would land outside warp_tol, or move a pixel in nearest mode)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import warp_ref as R
from oracle import cpu_ref

MODES = ('bilinear', 'nearest')
ALL = R.nhwc_cases() + R.nchw_cases() + [R.BIG]
TAME = [n for n in ALL if R.parse(n)['kind'] != 'wild']
WILD = [n for n in ALL if R.parse(n)['kind'] == 'wild']
# ~12 % (~3.5 % at 258x256) is all that vectors of +-8 px can take out of a frame this large: a tap leaves it only from the 8-pixel
# band at an edge, with probability (8 - d) / 16 at distance d, i.e. 2.25 pixels' worth per edge -> 4.5 / h + 4.5 / w.  These cases are
# held to two thirds of that instead of the 30 % of every other case.
SPARSE_OUTSIDE = {n: (4.5 / R.parse(n)['h'] + 4.5 / R.parse(n)['w']) * 2 / 3 for n in TAME
                  if R.parse(n)['kind'] in ('frac', 'block') and R.parse(n)['h'] >= 64}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=8)
def case_nchw(name):
    """-> x (n, c, h, w), flow (n, h, w, 2) of any case"""
    c = R.warp_case(name)
    if R.parse(name)['n'] is None:
        return np.ascontiguousarray(c['x'].transpose(2, 0, 1))[None], c['flow'][None]
    return c['x'], c['flow']


def aten(x, flow, mode):
    """flow_warp as the reference builds it: pixel grid + flow, normalised to [-1, 1], F.grid_sample(zeros, align_corners=True)"""
    n, c, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    fl = T(flow)
    nx = 2.0 * (gx + fl[..., 0]) / max(w - 1, 1) - 1.0
    ny = 2.0 * (gy + fl[..., 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(T(x), torch.stack((nx, ny), 3), mode=mode, padding_mode='zeros', align_corners=True).numpy()


@pytest.mark.parametrize('name', TAME)
def test_reference_agrees_with_the_oracle_and_with_aten(name):
    x, flow = case_nchw(name)
    tol = R.warp_tol(x)
    for mode in MODES:
        ref = R.warp_ref_nchw(x, flow, mode)
        assert ref.dtype == np.float64 and ref.shape == x.shape
        for who, out in (('oracle', cpu_ref.flow_warp(T(x), T(flow), mode).numpy()), ('aten', aten(x, flow, mode))):
            if mode == 'nearest':
                assert np.array_equal(out, ref), (name, who)
            else:
                assert np.abs(out - ref).max() <= tol, (name, who, np.abs(out - ref).max(), tol)


@pytest.mark.parametrize('case', gu.WARP_CASES, ids=[c['name'] for c in gu.WARP_CASES])
def test_reference_agrees_with_the_goldens_of_the_real_reference(case):
    x, flow = gu.warp_case_inputs(case)
    mode = case.get('mode', 'bilinear')
    ref = R.warp_ref_nchw(x, flow, mode)
    gold = gu.load_golden(case['name'])['out']
    if mode == 'nearest':
        assert np.array_equal(gold, ref)
    else:
        assert np.abs(gold - ref).max() <= R.warp_tol(x)


@pytest.mark.parametrize('name', WILD)
def test_wild_vectors_deviate_from_aten_only_where_the_chain_is_not_finite(name):
    """ATen's bilinear returns NaN where the fp32 chain overflows or is NaN; the kernels, by their code, and warp_ref return 0 there.
    Everywhere else, and in nearest mode everywhere, the two agree."""
    x, flow = case_nchw(name)
    n, c, h, w = x.shape
    ix, iy = R.coords(h, w, flow)
    wild = ~(np.isfinite(ix) & np.isfinite(iy))                         # (n, h, w)
    assert wild.any() and (~wild).any() or h * w < 8
    near = aten(x, flow, 'nearest')
    assert np.array_equal(near, R.warp_ref_nchw(x, flow, 'nearest'))
    bil, ref = aten(x, flow, 'bilinear'), R.warp_ref_nchw(x, flow, 'bilinear')
    nan = np.isnan(bil)
    assert not np.isinf(bil).any()
    assert not (nan & ~wild[:, None]).any()                            # every NaN of ATen's sits on a non-finite chain
    assert np.abs(bil - ref)[~nan].max(initial=0.0) <= R.warp_tol(x)
    assert np.isfinite(ref).all() and not ref[np.broadcast_to(wild[:, None], ref.shape)].any()
    print(name, 'non-finite chains', int(wild.sum()), 'ATen NaN pixels', int(nan.any(axis=1).sum()))


def test_aten_bilinear_does_return_nan_on_a_non_finite_chain():
    x = np.ones((1, 1, 3, 17), np.float32)
    for v in (np.inf, -np.inf, np.nan, 3e38, -3e38):
        flow = np.zeros((1, 3, 17, 2), np.float32)
        flow[0, 1, 5, 0] = v
        out = aten(x, flow, 'bilinear')
        assert np.isnan(out[0, 0, 1, 5]) and np.isfinite(np.delete(out.ravel(), 17 + 5)).all(), v
        assert aten(x, flow, 'nearest')[0, 0, 1, 5] == 0
        for mode in MODES:
            ref = R.warp_ref_nchw(x, flow, mode)
            assert ref[0, 0, 1, 5] == 0 and np.isfinite(ref).all()


# --------------------------------------------------------------------------------------------------------------- census
def census(name):
    p = R.parse(name)
    flow = case_nchw(name)[1]
    return p, [R.warp_census(p['h'], p['w'], f) for f in flow]


@pytest.mark.parametrize('name', TAME)
def test_census(name):
    p, per_sample = census(name)
    for d in per_sample:
        print(name, R.census_line(d))
        assert d['nonfinite'] == 0
        if (p['h'], p['w']) in ((1, 1), (1, 5)):         # 1 and 5 samples: every size rule is still run, no share can be asked for
            continue
        if p['kind'] != 'oob':
            assert d['inside'] >= 0.30, (name, d)
            assert d['outside'] >= SPARSE_OUTSIDE.get(name, 0.30), (name, d)
        if p['kind'] == 'edge':                          # aimed exactly at -1, 0, size-1, size (see warp_ref.chain_image)
            for k in ('x_-1', 'x_0', 'x_last', 'x_size', 'y_-1', 'y_0', 'y_last', 'y_size'):
                assert d[k] >= 1, (name, k, d)
        if p['kind'] == 'half':
            assert d['ties'] >= 0.25, (name, d)
            assert d['edge_ties'] >= 1, (name, d)


def test_where_the_chain_returns_the_edges_exactly():
    for size in sorted({s for f in R.FRAMES for s in f} | {256, 258}):
        for v in (0.0, size - 1.0, float(size)):
            assert R.chain_image(size, v) == np.float32(v if size > 1 else 0.0), (size, v)
        got = float(R.chain_image(size, -1.0))
        if size in (16, 47, 64, 96, 256):
            assert -1.0 < got < -1.0 + 2e-6, (size, got)          # a weight of up to 2e-6 on the edge pixel: ATen's own result
        elif size > 1:
            assert got == -1.0, (size, got)


def test_wild_cases_hold_every_value_and_some_live_samples():
    for name in WILD:
        p = R.parse(name)
        if p['h'] * p['w'] < 500:
            continue
        flow = case_nchw(name)[1]
        for v in R.WILD:
            v = np.float32(v)
            assert (np.isnan(flow).any() if np.isnan(v) else (flow == v).any()), (name, v)
        d = R.warp_census(p['h'], p['w'], flow[0])
        assert d['nonfinite'] > 0.3 * p['h'] * p['w'] and d['inside'] > 0


# -------------------------------------------------------------------------------------------------------------- mutants
def mutant_shows(name, mutant, mode):
    c = R.warp_case(name)
    ref, bad = R.warp_ref(c['x'], c['flow'], mode), R.warp_ref(c['x'], c['flow'], mode, _mutant=mutant)
    d = np.abs(bad - ref)
    return float(d.max()), int((d.max(axis=2) > (R.warp_tol(c['x']) if mode == 'bilinear' else 0)).sum()), R.warp_tol(c['x'])


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """on at least one 64-channel case AND at least one general-kernel case, in every mode the mutant exists in.  The direct
    coordinate must show at 64x96 in bilinear (a smaller frame's chain is too exact) and on the `half` ties in nearest; the
    dropped row mask must show at odd H and only there."""
    for mode in R.MUTANT_MODES[mutant]:
        for chans in ((R.CHANNELS_64,), R.CHANNELS_GENERAL):
            names = [n for n in R.nhwc_cases(chans) if R.parse(n)['kind'] != 'wild']
            if mutant == 'direct':                       # bilinear: 64x96 is large enough; nearest: the ties of `half`
                names = [n for n in names if ('64x96' in n if mode == 'bilinear' else R.parse(n)['kind'] == 'half')]
            if mutant == 'no_row_mask':
                names = [n for n in names if R.parse(n)['h'] % 2 == 1 and R.parse(n)['h'] > 1]
            caught = {}
            for n in names:
                err, pixels, tol = mutant_shows(n, mutant, mode)
                if pixels:
                    caught[n] = (err, pixels)
            print(mutant, mode, 'c%s' % (chans,), 'caught by %d of %d cases' % (len(caught), len(names)),
                  'e.g.', sorted(caught.items(), key=lambda kv: -kv[1][1])[:2])
            assert caught, (mutant, mode, chans)
            if mutant == 'no_row_mask':                  # ... and never at an even H
                even = [n for n in R.nhwc_cases(chans) if R.parse(n)['h'] % 2 == 0 and R.parse(n)['kind'] != 'wild']
                assert not any(mutant_shows(n, mutant, mode)[1] for n in even)


def test_mutants_are_far_outside_the_tolerance_where_they_matter_most():
    """the edge rules and the weights on the 17x47 edge case, bilinear: hundreds of pixels, errors of the order of the data"""
    for mutant in ('le_edge', 'clamp', 'swap_w'):
        err, pixels, tol = mutant_shows('c64_17x47_edge', mutant, 'bilinear')
        assert pixels >= 100 and err > 1e4 * tol, (mutant, err, pixels, tol)
    err, pixels, tol = mutant_shows('c64_64x96_frac', 'direct', 'bilinear')
    print('direct at 64x96', err, pixels, tol)
    assert pixels >= 100 and err > 4 * tol


# ---------------------------------------------------------------------------------------------------------- tol and fp16
def test_tolerance_and_fp16_rule():
    assert R.warp_tol(np.array([0.5, -1.0])) == 6 * 2.0 ** -24
    v = np.array([1e6, -1e6, 65504.0, 65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25])
    assert R.h16(v).dtype == np.float16
    assert np.array_equal(R.h16(v).astype(np.float64), [65504.0, -65504.0, 65504.0, 65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0])


@pytest.mark.parametrize('name', ['c%d_%s_%s_sat' % (c, f, k) for c in (64, 8) for f in ('3x17', '17x47') for k in ('edge', 'wild')])
def test_saturation_cases_carry_a_sampled_spike(name):
    c = R.warp_case(name)
    assert (c['x'] == np.float32(R.SPIKE)).sum() == 1 and np.abs(c['x']).max() == R.SPIKE
    for mode in MODES:
        ref = R.warp_ref(c['x'], c['flow'], mode)
        assert ref.max() > R.F16_MAX and np.isfinite(R.h16(ref).astype(np.float64)).all()
        assert (R.h16(ref) == np.float16(R.F16_MAX)).any()
