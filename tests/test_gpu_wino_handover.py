"""The Winograd tile kernels' hand-over between tiles (csrc/conv_wino.hip: halo offsets of the next tile, interior / edge split of
their bounds test, the multi-source kernel's segment switch), bit for bit against the quadrant-unit kernels, which share none of it:
a unit fetches its own 10x10 halo with plain loads and has no tile loop.  Same arithmetic in the same order per accumulator, so
torch.equal throughout.

Frames.  48x48 is the smallest frame with an interior tile (3x3 tiles: the centre one's halo lies inside the frame, the other eight
take the masked form); 64x80 has interior tiles in a row; 53x71 is ragged right and bottom with an interior tile; 16x16 is one tile,
edge on every side.  On 9-20 tiles the launch is 8-16 blocks, so blocks walk more than one tile and prefetch a next tile's halo.

The tail frame.  The launcher starts min(tiles, CUs) blocks rounded down to a multiple of 8, an XCD band is tiles / 8 (+ 1 for the
first tiles % 8 bands), a block walks every (blocks / 8)-th tile of its band, and a band's last `left` tiles become quadrant units
when rounds >= 1, left > 0 and 4 left <= blocks / 8.  With 256 CUs that needs more than 256 tiles; 257 is prime (one tile row), 258 =
3 x 86 tiles is the smallest count that makes a frame of three tile rows, the fewest with an interior tile: bands 0 and 1 hold 33 tiles
= one round + 1.  33 x 1361 pixels is its smallest frame (ragged both ways).  tail_frame() derives it from the device's CU count."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES = [(48, 48), (64, 80), (53, 71), (16, 16)]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def par_planes(seed, h, w, block):
    """one-hot partition planes, constant on block x block squares (values 0 or 1/255); the first block row has no record"""
    rng = np.random.RandomState(seed)
    cls = rng.randint(0, 3, ((h + block - 1) // block, (w + block - 1) // block))
    cls = np.repeat(np.repeat(cls, block, 0), block, 1)[:h, :w]
    par = np.stack([(cls == j).astype(np.float32) / np.float32(255.0) for j in range(3)])
    par[:, :block] = 0
    return torch.from_numpy(par).to(dev())


def tail_frame(cus):
    """smallest frame (fewest tiles, then at least three tile rows, ragged) whose whole-frame launch leaves a quadrant-unit tail"""
    for tiles in range(cus + 1, 4 * cus):
        grid = min(tiles, cus)
        grid -= grid % 8
        tstep, bq, br = grid // 8, tiles // 8, tiles % 8
        tail = False
        for nband in ([bq + 1] if br else []) + [bq]:
            rounds, left = nband // tstep, nband % tstep
            tail = tail or (rounds >= 1 and left > 0 and 4 * left <= tstep)
        if not tail:
            continue
        for rows in range(3, int(tiles ** 0.5) + 1):
            if tiles % rows == 0:
                return 16 * (rows - 1) + 1, 16 * (tiles // rows - 1) + 1
    raise AssertionError('no frame with a tail')


@pytest.fixture(scope='module')
def weights():
    from pnp_vcve_amd import ops
    g = torch.Generator(device=dev()).manual_seed(11)
    wt = torch.randn(64, 64, 3, 3, device=dev(), generator=g) * 0.05
    b = torch.randn(64, device=dev(), generator=g) * 0.1
    gamma = torch.rand(64, device=dev(), generator=g)
    w1 = [torch.randn(64, 64, 1, 1, device=dev(), generator=g) * 0.1 for _ in range(3)]
    wms = torch.randn(64, 195, 3, 3, device=dev(), generator=g) * 0.04
    imgs = torch.stack([ops.wino_image(ops.pack_conv3x3(wms, cbase=3 + 64 * k, csrc=64)) for k in range(3)])
    return dict(u=ops.wino_image(ops.pack_conv3x3(wt)), ug=ops.wino_image(ops.pack_conv3x3(wt), gamma), up=ops.wino_par_image(ops.pack_conv1x1(w1)),
                b=b, gamma=gamma, imgs=imgs, urgb=ops.wino_rgb_image(ops.pack_conv3x3(wms, cbase=0, csrc=3)),
                fold_word=torch.tensor([8], dtype=torch.int32, device=dev()))


def maps(h, w, n, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return [torch.randn(h, w, 64, device=dev(), generator=g) for _ in range(n)]


def frame(h, w, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    lr4 = torch.rand(h, w, 4, device=dev(), generator=g)
    lr4[..., 3] = 0
    return lr4


@pytest.mark.parametrize('hw', FRAMES)
@pytest.mark.parametrize('body', ['plain', 'residual', 'fold_only', 'branches_residual'])
def test_tile_path_equals_the_quadrant_unit_path(hw, body, weights):
    """every body of the tile kernel against the unit kernel of the same body: plain + activation, residual, the fold-only body behind
    the gate (a map constant on 8x8 blocks + flags), the branch body + residual (a map constant on 4x4 blocks only: branch chunks run)"""
    from pnp_vcve_amd import _native, ops
    h, w = hw
    x, res = maps(h, w, 2, 100 + h)
    k = weights
    gate = None
    if body == 'plain':
        kw = dict(wino_w=k['u'], bias=k['b'], act=2)
    elif body == 'residual':
        kw = dict(wino_w=k['u'], bias=k['b'], residual=res)
    elif body == 'fold_only':
        par = par_planes(5, h, w, 8)
        kw = dict(wino_w=k['ug'], bias=k['b'], gamma=k['gamma'], wino_w1x1=k['up'], par=par, par_flags=ops.par_tile_flags(par), act=1)
        gate = k['fold_word']
    else:
        par = par_planes(6, h, w, 4)
        kw = dict(wino_w=k['ug'], bias=k['b'], gamma=k['gamma'], wino_w1x1=k['up'], par=par, par_flags=ops.par_tile_flags(par), residual=res)
    # (the units run ungated, i.e. the branch body, whose values a foldable map's fold-only body reproduces bit for bit)
    units = ops.conv3x3_wino(x, units=True, **kw)
    if gate is not None:
        _native.lib().pnp_debug_wino_gate_word(ctypes.c_void_p(gate.data_ptr()))
    try:
        tiles = ops.conv3x3_wino(x, **kw)
    finally:
        _native.lib().pnp_debug_wino_gate_word(None)
    assert torch.equal(tiles, units), (hw, body)


@pytest.mark.parametrize('hw', [(48, 48), (53, 71)])
@pytest.mark.parametrize('nwide', [1, 2, 3])
def test_multi_source_tile_kernel_equals_the_quadrant_unit_kernel(hw, nwide, weights):
    from pnp_vcve_amd import ops
    h, w = hw
    args = ([frame(h, w, 7)] + maps(h, w, nwide, 200 + h), [weights['urgb']] + [weights['imgs'][s] for s in range(nwide)])
    for act in (0, 2):
        assert torch.equal(ops.conv3x3_wino_ms(*args, bias=weights['b'], act=act), ops.conv3x3_wino_ms(*args, bias=weights['b'], act=act, units=True))


@pytest.fixture(scope='module')
def tail_case(weights):
    """the tail frame's sources and its quadrant-unit result per source count, computed once"""
    from pnp_vcve_amd import ops
    h, w = tail_frame(torch.cuda.get_device_properties(0).multi_processor_count)
    srcs = [frame(h, w, 9)] + maps(h, w, 3, 300)
    ws = [weights['urgb']] + [weights['imgs'][s] for s in range(3)]
    units = {n: ops.conv3x3_wino_ms(srcs[:n + 1], ws[:n + 1], bias=weights['b'], act=2, units=True) for n in (1, 2, 3)}
    return h, w, srcs, ws, units


def test_tail_frame_is_the_one_the_docstring_names():
    assert tail_frame(256) == (33, 1361)


@pytest.mark.parametrize('nwide', [1, 2, 3])
def test_multi_source_at_the_tail_frame(nwide, tail_case, weights):
    """a band's 33rd tile is a second round of one block here (the multi-source kernel has no quadrant-unit tail): that block
    prefetched it as its next tile through every source segment of its first tile"""
    from pnp_vcve_amd import ops
    h, w, srcs, ws, units = tail_case
    assert torch.equal(ops.conv3x3_wino_ms(srcs[:nwide + 1], ws[:nwide + 1], bias=weights['b'], act=2), units[nwide])


def test_multi_source_row_ranges_equal_one_launch_at_the_tail_frame(tail_case, weights):
    """two launches over complementary tile rows (tile0 / tcount: a row-band chain's two parts) write what one launch writes"""
    from pnp_vcve_amd import ops
    h, w, srcs, ws, units = tail_case
    rows = (h + 15) // 16
    for cut in sorted({1, rows - 1}):
        out = torch.full((h, w, 64), float('nan'), device=dev())
        with ops.wino_tile_rows(cut, rows - cut):
            ops.conv3x3_wino_ms(srcs, ws, bias=weights['b'], act=2, out=out)
        assert bool(torch.isnan(out[:16 * cut]).all()) and not bool(torch.isnan(out[16 * cut:]).any())
        with ops.wino_tile_rows(0, cut):
            ops.conv3x3_wino_ms(srcs, ws, bias=weights['b'], act=2, out=out)
        assert torch.equal(out, units[3]), cut


def test_single_source_tail_units_at_the_tail_frame(tail_case, weights):
    """the single-source kernels do cut the band's last tile into quadrant units there: plain and residual against the unit kernel"""
    from pnp_vcve_amd import ops
    h, w, srcs, ws, units = tail_case
    for kw in (dict(bias=weights['b'], act=2), dict(bias=weights['b'], residual=srcs[2])):
        assert torch.equal(ops.conv3x3_wino(srcs[1], weights['u'], **kw), ops.conv3x3_wino(srcs[1], weights['u'], units=True, **kw))
