"""GPU: row-band chains (pnp_generator_set_band_split, include/pnpvcve.h).  A conv of a branch runs as two
launches of the same tile kernel over complementary tile-row bands on two streams.  Which block walks a tile is all that changes, so
every check here is torch.equal, never a tolerance:
  * op level: every body of the tile kernels (plain, residual -- also written over its own residual, as a block's back half runs --,
    gated fold-only, gated branch, ungated branch, multi-source) over two complementary row ranges against one whole-frame launch,
    at 720p and on a ragged frame whose last tile row and column are cut by the frame's edge;
  * generator: switch on against switch off on the benchmark's clip, under hipGraph replay, with the bounded-memory schedule, with
    two clips in one call (two contexts in flight: the split switches itself off), with channel-last blocks;
  * ten forwards with the split on are identical: a missing ordering edge between the two chains would show as nondeterminism."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(720, 1280), (708, 1276)]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _par(h, w, seed, foldable):
    """one-hot partition planes with one value per 8x8 codec block (every quadrant foldable: the gate picks the fold-only body), or
    the same map shifted by 4 pixels (quadrants straddle codec blocks: the gate picks the branch body)"""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, 3, ((h + 7) // 8 + 1, (w + 7) // 8 + 1), generator=g)
    cls = cls.repeat_interleave(8, 0).repeat_interleave(8, 1)
    off = 0 if foldable else 4
    cls = cls[off:off + h, off:off + w]
    return torch.stack([(cls == j).float() / 255.0 for j in range(3)]).contiguous().to(dev())


def _two_bands(fn, like, row, rows):
    """fn(out) launched over tile rows [0, row) and [row, rows) into one buffer that starts as NaN: every pixel written exactly once"""
    from pnp_vcve_amd import ops
    out = torch.full_like(like, float('nan'))
    with ops.wino_tile_rows(row, rows - row):            # (B first: the parts are independent of each other)
        fn(out)
    with ops.wino_tile_rows(0, row):
        fn(out)
    return out


@pytest.mark.parametrize('hw', SIZES, ids=['720x1280', '708x1276'])
def test_two_row_bands_equal_one_launch_for_every_body(hw):
    from pnp_vcve_amd import _native, ops
    h, w = hw
    rows = (h + 15) // 16
    g = torch.Generator(device=dev()).manual_seed(1234 + h)
    x = torch.randn(h, w, 64, device=dev(), generator=g)
    res = torch.randn(h, w, 64, device=dev(), generator=g)
    wt = torch.randn(64, 64, 3, 3, device=dev(), generator=g) * 0.05
    b = torch.randn(64, device=dev(), generator=g) * 0.1
    gamma = torch.rand(64, device=dev(), generator=g)
    w1 = [torch.randn(64, 64, 1, 1, device=dev(), generator=g) * 0.1 for _ in range(3)]
    u, ug, up = ops.wino_image(ops.pack_conv3x3(wt)), ops.wino_image(ops.pack_conv3x3(wt), gamma), ops.wino_par_image(ops.pack_conv1x1(w1))
    L = _native.lib()
    word = torch.zeros(1, dtype=torch.int32, device=dev())
    bodies = {'plain': (dict(wino_w=u, bias=b, act=2), None),
              'residual': (dict(wino_w=u, bias=b, residual=res), None),
              'branch, ungated': (dict(wino_w=ug, bias=b, gamma=gamma, wino_w1x1=up, par=_par(h, w, 5, False), act=1), None)}
    for foldable in (True, False):
        par = _par(h, w, 7, foldable)
        flags = ops.par_tile_flags(par)
        kw = dict(wino_w=ug, bias=b, gamma=gamma, wino_w1x1=up, par=par, par_flags=flags)
        name = 'gated fold-only' if foldable else 'gated branch'
        bodies[name] = (dict(kw, act=1), 8 if foldable else 0)
        bodies[name + ' + residual'] = (dict(kw, residual=res), 8 if foldable else 0)
    for row in (1, rows // 2, 31 if rows > 32 else rows - 2, rows - 1):
        for name, (kw, gate) in bodies.items():
            if gate is not None:                         # the frame's partition word as the generator computes it (bit 3 = foldable)
                word.fill_(gate | 7)
                assert L.pnp_debug_wino_gate_word(ctypes.c_void_p(word.data_ptr())) == 0
            try:
                whole = ops.conv3x3_wino(x, **kw)
                split = _two_bands(lambda out: ops.conv3x3_wino(x, out=out, **kw), whole, row, rows)
            finally:
                L.pnp_debug_wino_gate_word(None)
            assert torch.equal(split, whole), (name, hw, row)
        # a block's back half writes over its own residual (run_branch: x = tmp0 is residual and destination)
        whole = ops.conv3x3_wino(x, wino_w=u, bias=b, residual=res)
        buf = res.clone()
        with ops.wino_tile_rows(row, rows - row):
            ops.conv3x3_wino(x, wino_w=u, bias=b, residual=buf, out=buf)
        with ops.wino_tile_rows(0, row):
            ops.conv3x3_wino(x, wino_w=u, bias=b, residual=buf, out=buf)
        assert torch.equal(buf, whole), ('in-place residual', hw, row)
    # a range beyond the frame is refused, and the hook resets
    with pytest.raises(RuntimeError):
        with ops.wino_tile_rows(rows - 1, 2):
            ops.conv3x3_wino(x, wino_w=u)
    assert torch.equal(ops.conv3x3_wino(x, wino_w=u, bias=b, act=2), ops.conv3x3_wino(x, wino_w=u, bias=b, act=2))


@pytest.mark.parametrize('hw', SIZES, ids=['720x1280', '708x1276'])
@pytest.mark.parametrize('nwide', [1, 3])
def test_two_row_bands_equal_one_launch_for_the_input_conv(hw, nwide):
    from pnp_vcve_amd import ops
    h, w = hw
    rows = (h + 15) // 16
    g = torch.Generator(device=dev()).manual_seed(99 + nwide)
    lr4 = torch.rand(h, w, 4, device=dev(), generator=g)
    lr4[..., 3] = 0
    xs = [torch.randn(h, w, 64, device=dev(), generator=g) for _ in range(nwide)]
    wt = torch.randn(64, 3 + 64 * nwide, 3, 3, device=dev(), generator=g) * 0.03
    b = torch.randn(64, device=dev(), generator=g) * 0.1
    imgs = torch.stack([ops.wino_image(ops.pack_conv3x3(wt, cbase=3 + 64 * k, csrc=64)) for k in range(nwide)])
    urgb = ops.wino_rgb_image(ops.pack_conv3x3(wt, cbase=0, csrc=3))
    args = ([lr4] + xs, [urgb] + [imgs[k] for k in range(nwide)])
    whole = ops.conv3x3_wino_ms(*args, bias=b, act=2)
    for row in (1, 31 if rows > 32 else rows - 2, rows - 1):
        split = _two_bands(lambda out: ops.conv3x3_wino_ms(*args, bias=b, act=2, out=out), whole, row, rows)
        assert torch.equal(split, whole), (hw, nwide, row)


# ------------------------------------------------------------------------------------------------- whole generator
def _model(**extra):
    import bench
    from pnp_vcve_amd import synthetic as syn
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    cfg.update(extra)
    sd = syn.make_state_dict(cfg, seed=2025)
    return bench.build_model(cfg, sd, dev(), 'fp32')


def _clip(n=1, t=7):
    import bench
    return bench.make_inputs(1000, t, 720, 1280, dev(), n)[1]


def _run(m, a):
    with torch.no_grad():
        out = m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])
    torch.cuda.synchronize()
    return out


def test_generator_switch_on_equals_switch_off_on_the_bench_clip():
    m, a = _model(), _clip()
    assert m.band_split == 1                              # the default
    on = _run(m, a)
    m.band_split = 0
    off = _run(m, a)
    assert torch.equal(on, off)
    for a0 in (18, 38, 44):                               # other first boundaries, up to the thinnest chain B the chain allows
        m.band_split = a0
        assert torch.equal(_run(m, a), off), a0
    m.band_split = 45                                     # leaves chain B empty: one launch per conv
    assert torch.equal(_run(m, a), off)
    # profiling keeps the split on and counts a split conv once: the same launches either way
    counts = {}
    for sw in (0, 1):
        m.band_split = sw
        m.profile(True)
        assert torch.equal(_run(m, a), off)
        counts[sw] = {k: v['launches'] for k, v in m.profile_read().items()}
        m.profile(False)
    assert counts[0] == counts[1] and counts[1]['conv_block'] == 2 * 7 * 16 + 7


def test_generator_switch_under_graph_replay_bounded_memory_two_clips_and_channel_last():
    m, a = _model(), _clip()
    m.band_split = 0
    off = _run(m, a)
    m.band_split = 1
    m.use_graphs = True
    assert torch.equal(_run(m, a), off)                   # capture
    assert torch.equal(_run(m, a), off)                   # replay
    assert torch.equal(_run(m, a), off)
    m.use_graphs = False
    m.max_resident_features = m.min_resident_features(7)
    assert m.max_resident_features < 7
    assert torch.equal(_run(m, a), off)
    m.max_resident_features = None
    a2 = _clip(n=2)
    on2 = _run(m, a2)                                     # two contexts in flight: no split
    m.band_split = 0
    assert torch.equal(_run(m, a2), on2)
    del m
    m = _model(channel_first=False)
    a3 = _clip(t=3)
    on3 = _run(m, a3)
    m.band_split = 0
    assert torch.equal(_run(m, a3), on3)


def test_ten_forwards_with_the_split_on_are_identical():
    m, a = _model(), _clip()
    assert m.band_split == 1
    first = _run(m, a)
    for i in range(9):
        assert torch.equal(_run(m, a), first), i
