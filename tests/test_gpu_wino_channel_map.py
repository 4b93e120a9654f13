"""The Winograd kernels' output-channel mapping, pinned with exact data (csrc/conv_wino.hip).

The weight images put output channel co into column co >> 2 of N tile co & 3, so that a lane's four N tiles are one 16-byte run of a
pixel's channels; the quadrant forms keep "wave w = channels 16 w + m" and only read the images at other offsets.  A mapping that is
wrong but self-consistent between image and epilogue passes any test with random weights against a tolerance, so here every value is
exact and the expected map is plain indexing:

  * x, the residual and the frame are multiples of 2^-8 in [0, 1); the bias is a multiple of 2^-8, distinct per channel;
  * every weight is one-hot at the centre tap: output channel c takes input channel sigma(c) = (5 c + 3) mod 64 (each further source
    and each 1x1 branch has a permutation of its own); gamma is in {1/2, 1, 2};
  * then the input transform (sums of four values), the transformed weights (+-1/4 gamma), every product and the output transform
    (sums of nine) are exact in fp32, and the result is compared with torch.equal.

The one body whose sums cannot be exact is the fold-only path on a one-hot / 255 map: fl(1/255) has a full 24-bit significand, so its
products with the transformed patch round.  That case is pinned twice: bit for bit with the live value 2^-8 in place of 1/255, and with
1/255 itself against a bound worked out from the arithmetic (see the test)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (100, 132)]          # 16 whole tiles | 7 x 9 tiles, ragged on both edges
C = np.arange(64)
SIGMA = (5 * C + 3) % 64


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _grid(seed, shape, lo=0, hi=256):
    """multiples of 2^-8 in [lo, hi) / 256"""
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi, shape).astype(np.float32) / 256.0).to(dev())


def _onehot3x3(sigma, cin=64, cbase=0):
    wt = np.zeros((64, cin, 3, 3), np.float32)
    wt[C, cbase + sigma, 1, 1] = 1.0
    return wt


def _act(v, act):
    return [v, torch.relu(v), torch.maximum(v, v * np.float32(0.1))][act]


@pytest.fixture(scope='module')
def data():
    from pnp_vcve_amd import ops
    d = {}
    d['bias'] = torch.from_numpy(((3 * C - 96) / 256.0).astype(np.float32)).to(dev())          # distinct, both signs
    d['gamma'] = torch.from_numpy(np.array([0.5, 1.0, 2.0], np.float32)[(C * 7 + C // 3) % 3]).to(dev())
    sig = torch.from_numpy(SIGMA).to(dev())
    d['sigma'] = sig
    packed = ops.pack_conv3x3(torch.from_numpy(_onehot3x3(SIGMA)).to(dev()))
    d['u'] = ops.wino_image(packed)
    d['ug'] = ops.wino_image(packed, d['gamma'])
    d['sig1'] = [torch.from_numpy(((2 * j + 7) * C + j + 1) % 64).to(dev()) for j in range(3)]
    w1 = []
    for j in range(3):
        w = np.zeros((64, 64, 1, 1), np.float32)
        w[C, d['sig1'][j].cpu().numpy(), 0, 0] = 1.0
        w1.append(torch.from_numpy(w).to(dev()))
    d['up'] = ops.wino_par_image(ops.pack_conv1x1(w1))
    for hw in SIZES:
        d[hw] = dict(x=_grid(hw[0], hw + (64,)), res=_grid(hw[0] + 1, hw + (64,)))
    return d


def test_image_sizes_are_unchanged():
    from pnp_vcve_amd import _native
    L = _native.lib()
    assert int(L.pnp_wino_image_floats()) == 65536
    assert int(L.pnp_wino_par_image_floats()) == 4 * 3 * 1024
    assert int(L.pnp_wino_rgb_image_floats()) == 4096


@pytest.mark.parametrize('units', [False, True], ids=['tiles', 'units'])
@pytest.mark.parametrize('hw', SIZES, ids=['64x64', '100x132'])
def test_plain_and_residual_bodies_put_every_channel_where_it_belongs(data, hw, units):
    from pnp_vcve_amd import ops
    x, res = data[hw]['x'], data[hw]['res']
    picked = x[:, :, data['sigma']]
    for act in (0, 1, 2):
        out = ops.conv3x3_wino(x, data['u'], bias=data['bias'], act=act, units=units)
        assert torch.equal(out, _act(picked + data['bias'], act)), act
    out = ops.conv3x3_wino(x, data['u'], bias=data['bias'], residual=res, units=units)
    assert torch.equal(out, picked + data['bias'] + res)
    # the gain lives in the image, the bias is scaled in the kernel
    out = ops.conv3x3_wino(x, data['ug'], bias=data['bias'], gamma=data['gamma'], act=2, units=units)
    assert torch.equal(out, _act(data['gamma'] * (picked + data['bias']), 2))


@pytest.mark.parametrize('units', [False, True], ids=['tiles', 'units'])
@pytest.mark.parametrize('hw', SIZES, ids=['64x64', '100x132'])
def test_branch_bodies_on_a_dense_float_partition_map(data, hw, units):
    """act(gamma (conv + b) + sum_j par_j conv1x1_j(x)) (+ residual): par_j are multiples of 2^-4 per pixel, so nothing folds and nothing
    is skipped; the products par_j x are multiples of 2^-12 and every sum stays exact"""
    from pnp_vcve_amd import ops
    x, res = data[hw]['x'], data[hw]['res']
    par = torch.from_numpy(np.random.RandomState(hw[1]).randint(1, 16, (3,) + hw).astype(np.float32) / 16.0).to(dev())
    main = data['gamma'] * (x[:, :, data['sigma']] + data['bias'])
    for j in range(3):
        main = main + par[j][:, :, None] * x[:, :, data['sig1'][j]]
    kw = dict(bias=data['bias'], gamma=data['gamma'], wino_w1x1=data['up'], par=par, units=units)
    for flags in (None, ops.par_tile_flags(par)):
        assert torch.equal(ops.conv3x3_wino(x, data['ug'], par_flags=flags, act=1, **kw), torch.relu(main))
        assert torch.equal(ops.conv3x3_wino(x, data['ug'], par_flags=flags, residual=res, **kw), main + res)


def _one_hot_blocks(hw, value, seed):
    h, w = hw
    cls = np.random.RandomState(seed).randint(0, 4, ((h + 7) // 8, (w + 7) // 8))        # class 3: a block without a record
    cls = np.repeat(np.repeat(cls, 8, 0), 8, 1)[:h, :w]
    return torch.from_numpy(np.stack([(cls == j).astype(np.float32) * np.float32(value) for j in range(3)])).to(dev())


@pytest.mark.parametrize('units', [False, True], ids=['tiles', 'units'])
@pytest.mark.parametrize('hw', SIZES, ids=['64x64', '100x132'])
def test_gated_fold_only_body(data, hw, units):
    """The fold-only body behind the frame's partition word (bit 3 set, as the generator computes it for such a frame): one-hot maps on
    8x8 blocks, the live plane folded into the B fragments.

    Live value 2^-8: every sum exact, torch.equal.  Live value fl(1/255), the loader's: its significand is 24 bits wide, so the folded
    fragment times a transformed patch value (|V| < 2, a multiple of 2^-8) does not fit fp32.  Per folded position (four of them, all
    of which reach every output pixel): the fragment gamma / 4 + p / 4 rounds when both land on the same input channel (relative 2^-24
    on a product < 1: 2^-24) and the product is added to an accumulator of magnitude < 2 (half an ulp: 2^-23).  The output transform
    adds nine such values in eight steps whose partial sums stay below 8 (2^-22 each); the residual is one more sum below 4 (2^-23).
    Bound: 4 (2^-23 + 2^-24) + 8 * 2^-22 + 2^-23 = 2.8e-6 < 3e-6.  A wrong channel moves a pixel by p |x - x'| ~ 1e-3."""
    from pnp_vcve_amd import _native, ops
    x, res = data[hw]['x'], data[hw]['res']
    L = _native.lib()
    word = torch.full((1,), 8 | 7, dtype=torch.int32, device=dev())
    for value, exact in ((1.0 / 256.0, True), (1.0 / 255.0, False)):
        par = _one_hot_blocks(hw, value, 5 + hw[0])
        main = (data['gamma'] * (x[:, :, data['sigma']] + data['bias'])).double()
        for j in range(3):
            main = main + par[j][:, :, None].double() * x[:, :, data['sig1'][j]].double()
        kw = dict(bias=data['bias'], gamma=data['gamma'], wino_w1x1=data['up'], par=par, par_flags=ops.par_tile_flags(par), units=units)
        assert L.pnp_debug_wino_gate_word(ctypes.c_void_p(word.data_ptr())) == 0
        try:
            out = ops.conv3x3_wino(x, data['ug'], act=1, **kw)
            out_res = ops.conv3x3_wino(x, data['ug'], residual=res, **kw)
        finally:
            L.pnp_debug_wino_gate_word(None)
        for got, want in ((out, torch.relu(main)), (out_res, main + res.double())):
            d = float((got.double() - want).abs().max())
            print(hw, units, value, 'max|got - expected| =', d)
            if exact:
                assert torch.equal(got.double(), want)
            else:
                assert d < 3e-6


@pytest.mark.parametrize('units', [False, True], ids=['tiles', 'units'])
@pytest.mark.parametrize('nwide', [1, 2, 3])
@pytest.mark.parametrize('hw', SIZES, ids=['64x64', '100x132'])
def test_multi_source_input_conv(data, hw, nwide, units):
    """[frame, 1..3 wide sources]: output channel c = frame channel c mod 3 + sum_s x_s[sigma_s(c)] + bias, each source with a
    permutation of its own"""
    from pnp_vcve_amd import ops
    h, w = hw
    lr4 = _grid(40 + nwide, hw + (4,))
    lr4[..., 3] = 0
    xs = [data[hw]['x'], data[hw]['res'], _grid(77, hw + (64,))][:nwide]
    sig = [((5 + 2 * s) * C + 3 + s) % 64 for s in range(nwide)]
    wt = np.zeros((64, 3 + 64 * nwide, 3, 3), np.float32)
    wt[C, C % 3, 1, 1] = 1.0
    for s in range(nwide):
        wt[C, 3 + 64 * s + sig[s], 1, 1] = 1.0
    wt = torch.from_numpy(wt).to(dev())
    urgb = ops.wino_rgb_image(ops.pack_conv3x3(wt, cbase=0, csrc=3))
    img = torch.empty(nwide, 65536, device=dev())
    for s in range(nwide):
        img[s] = ops.wino_image(ops.pack_conv3x3(wt, cbase=3 + 64 * s, csrc=64))
    want = lr4[:, :, torch.from_numpy(C % 3).to(dev())] + data['bias']
    for s in range(nwide):
        want = want + xs[s][:, :, torch.from_numpy(sig[s]).to(dev())]
    for act in (0, 2):
        out = ops.conv3x3_wino_ms([lr4] + xs, [urgb] + [img[s] for s in range(nwide)], bias=data['bias'], act=act, units=units)
        assert torch.equal(out, _act(want, act)), act
