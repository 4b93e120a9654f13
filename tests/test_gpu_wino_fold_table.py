"""The fold table of the Winograd front halves (csrc/fold_table.h, csrc/conv_persist.hip launch_par_fold_table; read by the fold-only
body of csrc/conv_wino.hip's gated kernels through one scalar load per tile).  Every result here is a torch.equal: the table holds the
numbers the body computed itself, so no output bit may move.

Frames (with 256 CUs).  272x256 = 17 x 16 = 272 tiles on 256 blocks: an XCD band is 34 tiles for 32 blocks.  A band's last `left`
tiles become quadrant units when rounds >= 1, left > 0 and 4 * left <= 32: here left = 2, so every band ends in 8 units whose blocks
read the unit's record -- every wave that quadrant's -- a tile ahead, behind their one whole tile; with fewer CUs (more than one round)
blocks also read a second whole tile's records ahead.  64x64 and 48x80 are 16 / 15 tiles, one per block: only the prologue's read.
100x132 is ragged both ways: quadrants cut by the right and the bottom edge, and a last tile row (7 tile rows over 100 pixel rows)
whose lower quadrants lie outside the frame."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES = [(272, 256), (64, 64), (48, 80), (100, 132)]
MAPS = ['one_hot', 'zero', 'constants', 'two_live']


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def planes(kind, h, w, seed=3):
    """(3,h,w) partition planes, constant on 8x8 blocks from the origin (the frame cuts the last row / column of blocks):
    one_hot: one plane per block at 1/255 (a fifth of the blocks none) | zero | constants: one plane per block, its value drawn per
    block | two_live: the one-hot map with a second live plane in a few blocks (not foldable: the gate must fail)"""
    rng = np.random.RandomState(seed + 7 * h + w)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    cls = rng.randint(0, 5, (bh, bw))                         # 3, 4: no record
    cls[0, 0] = 0
    val = np.full((bh, bw), np.float32(1.0) / np.float32(255.0), np.float32)
    if kind == 'constants':
        val = (rng.randint(1, 200, (bh, bw)).astype(np.float32) / np.float32(255.0)) * np.where(rng.rand(bh, bw) < 0.3, -1, 1).astype(np.float32)
    blk = np.stack([(cls == j) * val for j in range(3)]).astype(np.float32)
    if kind == 'zero':
        blk[:] = 0
    if kind == 'two_live':
        hit = rng.rand(bh, bw) < 0.2
        hit[0, 0] = hit[-1, -1] = True
        blk[1][hit & (cls != 1)] = np.float32(2.0) / np.float32(255.0)
        blk[0][hit & (cls == 1)] = np.float32(2.0) / np.float32(255.0)
    return np.ascontiguousarray(np.repeat(np.repeat(blk, 8, 1), 8, 2)[:, :h, :w])


def table_numpy(par):
    """csrc/fold_table.h restated: record (tile, quadrant) from the quadrant's first pixel"""
    _, h, w = par.shape
    ty, tx = (h + 15) // 16, (w + 15) // 16
    out = np.zeros((ty * tx * 4, 2), np.int32)
    out[:, 0] = -1
    for qy in range(2 * ty):
        for qx in range(2 * tx):
            if 8 * qy >= h or 8 * qx >= w:
                continue
            v = par[:, 8 * qy, 8 * qx]
            nz = np.flatnonzero(v != 0)
            if len(nz):
                i = ((qy >> 1) * tx + (qx >> 1)) * 4 + (qy & 1) * 2 + (qx & 1)
                out[i, 0] = nz[0]
                out[i, 1] = (np.float32(0.25) * v[nz[0]]).view(np.int32)
    return out


def gate_word(flags):
    """the frame's partition word as launch_par_frame_any makes it from the tile flags"""
    f = flags.cpu().numpy()
    return int(np.bitwise_or.reduce(f.ravel() & 7)) | (8 if bool(((f & 64) != 0).all()) else 0)


@pytest.fixture(scope='module')
def weights():
    from pnp_vcve_amd import ops
    g = torch.Generator(device=dev()).manual_seed(23)
    wt = torch.randn(64, 64, 3, 3, device=dev(), generator=g) * 0.05
    gamma = torch.rand(64, device=dev(), generator=g)
    w1 = [torch.randn(64, 64, 1, 1, device=dev(), generator=g) * 0.1 for _ in range(3)]
    return dict(ug=ops.wino_image(ops.pack_conv3x3(wt), gamma), up=ops.wino_par_image(ops.pack_conv1x1(w1)), gamma=gamma,
                b=torch.randn(64, device=dev(), generator=g) * 0.1)


@pytest.fixture(scope='module')
def inputs():
    """per frame size: the source map and a residual, made once"""
    out = {}
    for h, w in FRAMES:
        g = torch.Generator(device=dev()).manual_seed(1000 + h)
        out[(h, w)] = (torch.randn(h, w, 64, device=dev(), generator=g), torch.randn(h, w, 64, device=dev(), generator=g))
    return out


@pytest.mark.parametrize('kind', MAPS)
@pytest.mark.parametrize('hw', FRAMES)
def test_fold_table_kernel_equals_its_numpy_restatement(hw, kind):
    from pnp_vcve_amd import ops
    par = planes(kind, *hw)
    got = ops.par_fold_table(torch.from_numpy(par).to(dev())).cpu().numpy()
    assert np.array_equal(got, table_numpy(par)), (hw, kind)
    # the maps are what their names say: only two_live fails the gate (bit 3 of the frame's word)
    word = gate_word(ops.par_tile_flags(torch.from_numpy(par).to(dev())))
    assert bool(word & 8) == (kind != 'two_live'), (hw, kind, word)
    assert ((word & 7) == 0) == (kind == 'zero')


@pytest.mark.parametrize('res', [False, True], ids=['act', 'residual'])
@pytest.mark.parametrize('kind', MAPS)
@pytest.mark.parametrize('hw', FRAMES)
def test_gated_front_half_equals_the_branch_body_and_the_unskipped_launch(hw, kind, res, weights, inputs):
    """one front half (gated<false>: + activation; gated<true>, the channel-last blocks' form: + residual) behind the frame's own word
    -- the fold-only body with its table on every map but two_live, whose word sends the launch to the branch body -- against (a)
    the same gated launch with the word forced to 0: the branch body on the same map, and (b) the launch without tile flags
    (PNP_OPT_PAR_SKIP = 0 in the generator): the ungated branch kernel with every branch run"""
    from pnp_vcve_amd import _native, ops
    h, w = hw
    x, r = inputs[hw]
    k = weights
    par = torch.from_numpy(planes(kind, h, w)).to(dev())
    flags = ops.par_tile_flags(par)
    kw = dict(wino_w=k['ug'], bias=k['b'], gamma=k['gamma'], wino_w1x1=k['up'], par=par)
    kw.update(dict(residual=r) if res else dict(act=1))
    words = {v: torch.tensor([v], dtype=torch.int32, device=dev()) for v in (gate_word(flags), 0)}

    def gated(word):
        _native.lib().pnp_debug_wino_gate_word(ctypes.c_void_p(words[word].data_ptr()))
        try:
            return ops.conv3x3_wino(x, par_flags=flags, **kw)
        finally:
            _native.lib().pnp_debug_wino_gate_word(None)
    own = gated(gate_word(flags))
    assert torch.equal(own, gated(0)), (hw, kind, res, 'fold-only body vs branch body')
    assert torch.equal(own, ops.conv3x3_wino(x, **kw)), (hw, kind, res, 'gated vs no flags')
    assert torch.equal(own, ops.conv3x3_wino(x, par_flags=flags, **kw)), (hw, kind, res, 'gated vs ungated with flags')


# ------------------------------------------------------------------------------------------------- whole generator
def build(cfg, sd_np):
    from pnp_vcve_amd import _native
    from pnp_vcve_amd.registry import build_backbone
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    m = m.to(dev()).eval()
    m.set_option(_native.OPT_WINOGRAD, 2)          # the tile kernels at every frame size
    return m


def run(m, clip):
    a = {k: torch.from_numpy(v).to(dev()) for k, v in clip.items()}
    with torch.no_grad():
        return m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])


@pytest.fixture(scope='module')
def generator_case():
    """64x64, T = 3 ('IBP'), two clips; the model; and each clip's result with PNP_OPT_PAR_SKIP off (no flags, no gate, no table:
    the branch kernel on every frame), computed once"""
    from pnp_vcve_amd import _native, synthetic as syn
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    m = build(cfg, syn.make_state_dict(cfg, seed=2025, par_gain=10.0))
    clip = syn.make_clip(seed=515, n=2, t=3, h=64, w=64, slices=[73, 66, 80], qp_mode='qp', crf=[15, 35], block=8, par_classes=3)
    assert float(np.abs(clip['partitions'][:, 0]).max()) == 0.0 and float(np.abs(clip['partitions'][:, 1:]).max()) > 0.0
    m.set_option(_native.OPT_PAR_SKIP, 0)
    off = [run(m, {k: v[b:b + 1] for k, v in clip.items()}).clone() for b in range(2)]
    m.set_option(_native.OPT_PAR_SKIP, 1)
    return m, clip, off


def test_generator_forward_with_the_table_equals_the_ungated_forward(generator_case):
    m, clip, off = generator_case
    for b in range(2):
        assert torch.equal(run(m, {k: v[b:b + 1] for k, v in clip.items()}), off[b]), b


def test_generator_forward_under_graph_replay(generator_case):
    m, clip, off = generator_case
    one = {k: v[:1] for k, v in clip.items()}
    m.use_graphs = True
    try:
        for _ in range(2):                         # capture, then a replay
            assert torch.equal(run(m, one), off[0])
    finally:
        m.use_graphs = False


def test_generator_forward_with_two_clips_in_flight(generator_case):
    """n = 2: two workspace contexts on two streams, each with its own table buffers"""
    m, clip, off = generator_case
    assert torch.equal(run(m, clip), torch.cat(off))
