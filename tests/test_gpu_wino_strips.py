"""GPU: the strip walk of the Winograd tile kernels (csrc/conv_wino.hip, the top of wino_tile_body and launch_wino_rows) at every
schedule class, against fp64.

tests/wino_strip_walk.py restates the walk; tests/test_wino_strip_walk.py shows on the CPU that the restatement covers every tile once.
Here, on the device, with the device's own CU count:
  * five frames, ragged in both directions, chosen so that together they run every class of band -- whole rounds only (A, one round and
    two), quadrant units with every block taking one and with idle blocks (B, B-idle), a partial round (C, one round and six) -- in
    uneven launches (tile count no multiple of 8), where neighbouring bands differ in class.  A frame that no longer hits its classes
    (another CU count, another grid rule) FAILS: a skip would hide the missing class;
  * every body of the tile kernels on each: (a) into a buffer that starts as NaN -- no NaN left: every pixel written; (b) the whole
    frame against the fp64 host reference at the gates of tests/test_gpu_wino.py (TOL_OP * max(1, max|ref|); 2 * TOL_OP with a
    residual); (c) bit for bit against the quadrant-unit form of the same call;
  * the walk itself: the single-source kernels' trace words (include/pnpvcve_debug.h: [7] tiles walked, [4] start tick of the block's
    quadrant unit) equal walk() block by block, so an edit of the kernel's scheduler or of the restatement alone fails here;
  * row bands whose second part starts at tile0 > 0 with a tile count that is no multiple of 8: two launches into one NaN buffer equal
    the whole-frame launch, trace words checked per part."""
import contextlib
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import wino_strip_walk as sw
from test_gpu_wino import TOL_OP, G, dev, nchw, nhwc, par_maps, ref_conv

pytestmark = pytest.mark.gpu

# frame (h, w) -> what walk() must report for it on this device (256 CUs: tiles_y x tiles_x, bands of tcount >> 3 (+ 1) tiles)
FRAMES = {
    (100, 132): dict(tiles=63, classes={'A', 'B', 'B-idle'}, rounds=1, units=28),      # 7x9, grid 56, tstep 7: 7 bands of 8 (left 1), one of 7
    (277, 283): dict(tiles=324, classes={'B', 'C'}, rounds=1, units=128),              # 18x18: 4 bands of 41 (left 9: C), 4 of 40 (left 8: all 32 slots)
    (340, 361): dict(tiles=506, classes={'A', 'C'}, rounds=2, units=0),                # 22x23: 2 bands of 64 (two rounds), 6 of 63 (left 31)
    (297, 421): dict(tiles=513, classes={'A', 'B', 'B-idle'}, rounds=2, units=4),      # 19x27: one band of 65 (left 1, 28 idle slots), 7 of 64
    (480, 854): dict(tiles=1620, classes={'C'}, rounds=6, units=0),                    # 30x54: 4 bands of 203 (left 11), 4 of 202 (left 10)
}
FEW_BODIES = ('plain', 'residual', 'residual in place', 'branch, straddling', 'branch, foldable')       # 480x854
BODIES = FEW_BODIES + ('gated fold-only', 'gated branch', 'gated fold-only + residual', 'gated branch + residual', 'input conv, 1 source',
                       'input conv, 3 sources')
# row bands: frame -> first tile row of the second part
BAND_ROW = {(277, 283): 7, (297, 421): 10}                 # 126 + 198 tiles; 270 + 243 tiles (tile0 = 270)
BAND_BODIES = ('plain', 'residual in place', 'gated fold-only', 'input conv, 3 sources')


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def frame_walk(hw):
    """walk() of the whole-frame launch, after the check that the frame still hits the classes it is here for"""
    h, w = hw
    want = FRAMES[hw]
    tiles = ((h + 15) // 16) * ((w + 15) // 16)
    wk = sw.walk(tiles, 0, cus())
    got = dict(tiles=tiles, classes=wk.classes, rounds=wk.max_rounds, units=sum(q is not None for q in wk.units))
    assert got == want and tiles % 8 != 0, \
        '%dx%d on %d CUs no longer runs the schedule classes it was chosen for: %r, wanted %r -- choose another frame' % (h, w, cus(), got, want)
    return wk


@functools.lru_cache(maxsize=1)
def frame_data(hw):
    """inputs of every body on one frame (host arrays) and a cache for their device copies and the fp64 references"""
    h, w = hw
    u = lambda name, shape, lo, hi: gu.syn.uniform(41, f'{name}{h}x{w}', shape, lo, hi)      # noqa: E731
    d = types.SimpleNamespace(hw=hw, cache={})
    d.x, d.res = u('x', (1, 64, h, w), -1, 1), u('r', (1, 64, h, w), -2, 2)
    d.wt, d.b, d.gamma = u('w', (64, 64, 3, 3), -0.06, 0.06), u('b', (64,), -0.1, 0.1), u('g', (64,), 0.0, 1.0)
    d.gamma[5] = 0.0
    d.w1f = [u(f'w1f{j}', (64, 64, 1, 1), -0.3, 0.3) * 25.5 for j in range(3)]         # front halves (test_wino_front_half_folds_...)
    d.w1r = [u(f'w1r{j}', (64, 64, 1, 1), -3.0, 3.0) for j in range(3)]                # with a residual (test_wino_back_half_...)
    d.par_fold = par_maps(43, h, w, 1.0 / 255.0, block=8, empty_rows=1)                # every 8x8 quadrant: all zero or one constant plane
    d.par_str = np.ascontiguousarray(par_maps(44, h + 4, w + 4, 1.0 / 255.0, block=8)[:, 4:, 4:])      # quadrants straddle the codec blocks
    return d


def cached(d, key, make):
    if key not in d.cache:
        d.cache[key] = make()
    return d.cache[key]


def ms_inputs(d, nwide):
    """the input conv over [frame, nwide wide sources] (test_wino_input_conv_over_the_virtual_concat's data): host arrays"""
    h, w = d.hw
    u = lambda name, shape, lo, hi: gu.syn.uniform(45, f'{name}{h}x{w}', shape, lo, hi)      # noqa: E731
    lr = cached(d, 'lr', lambda: u('lr', (1, 3, h, w), 0, 1))
    wide = [cached(d, f'wide{k}', lambda k=k: u(f'wide{k}', (1, 64, h, w), -1, 1)) for k in range(nwide)]
    wt = cached(d, f'wtms{nwide}', lambda: u(f'wtms{nwide}', (64, 3 + 64 * nwide, 3, 3), -0.06, 0.06))
    return lr, wide, wt


def reference(d, name):
    """fp64 on the host, once per frame and operation (several bodies share one)"""
    key = {'residual in place': 'residual', 'gated fold-only': 'branch, foldable', 'gated branch': 'branch, straddling'}.get(name, name)

    def make():
        if key == 'plain':
            return ref_conv(d.x, d.wt, d.b, act=2)
        if key == 'residual':
            return ref_conv(d.x, d.wt, d.b, residual=d.res)
        par = d.par_fold if 'fold' in key else d.par_str
        if key.startswith('branch'):
            return ref_conv(d.x, d.wt, d.b, d.gamma, d.w1f, par, act=1)
        if key.startswith('gated'):
            return ref_conv(d.x, d.wt, d.b, d.gamma, d.w1r, par, residual=d.res)
        lr, wide, wt = ms_inputs(d, 1 if '1 source' in key else 3)
        return F.leaky_relu(F.conv2d(torch.from_numpy(np.concatenate([lr] + wide, 1)).double(), torch.from_numpy(wt).double(),
                                     torch.from_numpy(d.b).double(), padding=1), 0.1)
    return cached(d, 'ref ' + key, make)


def device_args(d, name):
    """(op, positional args, keyword args, gate word or None) of a body on the device"""
    from pnp_vcve_amd import ops
    c = lambda key, make: cached(d, 'dev ' + key, make)      # noqa: E731
    b = c('b', lambda: G(d.b))
    if name.startswith('input conv'):
        nwide = 1 if '1 source' in name else 3
        lr, wide, wt = ms_inputs(d, nwide)

        def frame4():
            lr4 = torch.zeros(d.hw + (4,), device=dev())
            lr4[..., :3] = G(lr)[0].permute(1, 2, 0)
            return lr4
        srcs = [c('lr4', frame4)] + [c(f'wide{k}', lambda k=k: nhwc(wide[k])) for k in range(nwide)]

        def images():
            imgs = torch.empty(nwide, 65536, device=dev())               # ONE tensor: the images within 4 GiB of each other
            for k in range(nwide):
                imgs[k] = ops.wino_image(ops.pack_conv3x3(G(wt), cbase=3 + 64 * k, csrc=64))
            return [ops.wino_rgb_image(ops.pack_conv3x3(G(wt), cbase=0, csrc=3))] + [imgs[k] for k in range(nwide)]
        return ops.conv3x3_wino_ms, (srcs, c(f'ms images {nwide}', images)), dict(bias=b, act=2), None
    x = c('x', lambda: nhwc(d.x))
    u = c('u', lambda: ops.wino_image(ops.pack_conv3x3(G(d.wt))))
    if name == 'plain':
        return ops.conv3x3_wino, (x,), dict(wino_w=u, bias=b, act=2), None
    res = c('res', lambda: nhwc(d.res))
    if name.startswith('residual'):
        return ops.conv3x3_wino, (x,), dict(wino_w=u, bias=b, residual=res), None
    gamma = c('gamma', lambda: G(d.gamma))
    ug = c('ug', lambda: ops.wino_image(ops.pack_conv3x3(G(d.wt)), gamma))
    fold = 'fold' in name
    par = c('par fold', lambda: G(d.par_fold)) if fold else c('par str', lambda: G(d.par_str))
    kw = dict(wino_w=ug, bias=b, gamma=gamma, par=par)
    if name.startswith('gated') or name == 'branch, foldable':
        kw['par_flags'] = c('flags fold' if fold else 'flags str', lambda: ops.par_tile_flags(par))
    if name.endswith('residual'):
        kw.update(wino_w1x1=c('upr', lambda: ops.wino_par_image(ops.pack_conv1x1([G(v) for v in d.w1r]))), residual=res)
    else:
        kw.update(wino_w1x1=c('upf', lambda: ops.wino_par_image(ops.pack_conv1x1([G(v) for v in d.w1f]))), act=1)
    # the frame's partition word as the generator computes it (bit 3 = every quadrant foldable), as test_gpu_band_split.py sets it
    return ops.conv3x3_wino, (x,), kw, ((8 if fold else 0) | 7) if name.startswith('gated') else None


@contextlib.contextmanager
def gate_word(value):
    """the next conv3x3_wino calls with branches and tile flags take the one gated launch (pnp_debug_wino_gate_word)"""
    from pnp_vcve_amd import _native
    if value is None:
        yield
        return
    word = torch.full((1,), value, dtype=torch.int32, device=dev())
    assert _native.lib().pnp_debug_wino_gate_word(ctypes.c_void_p(word.data_ptr())) == 0
    try:
        yield
        torch.cuda.synchronize()                                     # (the launches read the word)
    finally:
        _native.lib().pnp_debug_wino_gate_word(None)


def launch(d, name, units=False, trace=None):
    """one launch of the body into a buffer that starts as NaN (in place: into a copy of the residual); returns the buffer"""
    op, args, kw, gate = device_args(d, name)
    kw = dict(kw)
    if name == 'residual in place':
        kw['residual'] = out = kw['residual'].clone()
    else:
        out = torch.full(d.hw + (64,), float('nan'), device=dev())
    if trace is not None:
        kw['trace'] = trace
    with gate_word(gate):
        op(*args, out=out, units=units, **kw)
    return out


def new_trace(wk):
    """16 words per block; room for one block per CU whatever grid walk() expects, so that a disagreement about the grid shows as a
    failed check, not as a write past the buffer"""
    return torch.zeros(16 * max(wk.grid, cus()), dtype=torch.int64, device=dev())


def check_trace(trace, wk, hw, what):
    """the kernel's own account of its walk against walk(): per block the whole tiles it walked ([7]; a block that returns at once
    writes nothing) and whether it worked on a quadrant unit ([4] != 0; a unit whose origin lies outside the frame is skipped)"""
    t = trace.view(-1, 16).cpu()
    assert not bool(t[wk.grid:].any()), '%s %r: more than the %d blocks walk() expects ran' % (what, hw, wk.grid)
    got =[(int(t[b, 7]), bool(t[b, 4] != 0)) for b in range(wk.grid)]
    want = [(len(wk.tiles[b]), wk.units[b] is not None and sw.unit_inside(wk.units[b], *hw)) for b in range(wk.grid)]
    diff = [(b, got[b], want[b]) for b in range(wk.grid) if got[b] != want[b]]
    assert not diff, '%s %r: (block, kernel (tiles, unit), walk() (tiles, unit)) differ: %r' % (what, hw, diff[:8])


CASES = [(hw, name) for hw in FRAMES for name in (FEW_BODIES if hw == (480, 854) else BODIES)]


@pytest.mark.parametrize('hw', list(FRAMES), ids=lambda hw: '%dx%d' % hw)
def test_the_frames_run_the_schedule_classes_they_were_chosen_for(hw):
    frame_walk(hw)
    assert sw.walk(FRAMES[hw]['tiles'], 0, cus(), units=False).classes <= {'A', 'C'}       # the input conv never takes units
    if hw in BAND_ROW:
        tiles_x, rows = (hw[1] + 15) // 16, (hw[0] + 15) // 16
        parts = [tiles_x * BAND_ROW[hw], tiles_x * (rows - BAND_ROW[hw])]
        assert parts == {(277, 283): [126, 198], (297, 421): [270, 243]}[hw] and all(n % 8 for n in parts)


@pytest.mark.parametrize('hw,name', CASES, ids=['%dx%d %s' % (hw + (name,)) for hw, name in CASES])
def test_every_body_on_every_class_against_fp64_the_unit_form_and_the_walk(hw, name):
    wk = frame_walk(hw)
    d = frame_data(hw)
    out = launch(d, name)
    assert not bool(torch.isnan(out).any()), 'pixels no block wrote'    # (a)
    ref = reference(d, name)                                             # (b)
    mag = float(ref.abs().max())
    delta = float((nchw(out).double() - ref).abs().max())
    bound = 2 * TOL_OP if 'residual' in name else TOL_OP * max(1.0, mag)
    print('%dx%d %s: max|winograd - fp64| = %.3g (bound %.3g, max|ref| = %.3g)' % (hw + (name, delta, bound, mag)))
    assert delta < bound
    assert torch.equal(launch(d, name, units=True), out)                 # (c) also in place: a tile walked twice adds its conv twice
    if name == 'residual in place':
        assert torch.equal(out, launch(d, 'residual'))
    if name == 'branch, foldable':                                       # with / without branch skipping: skipped branches add exact zeros
        op, args, kw, _ = device_args(d, name)
        assert torch.equal(op(*args, **{k: v for k, v in kw.items() if k != 'par_flags'}), out)
    if not name.startswith('input conv'):
        trace = new_trace(wk)
        assert torch.equal(launch(d, name, trace=trace), out)
        check_trace(trace, wk, hw, name)


BAND_CASES = [(hw, name) for hw in BAND_ROW for name in BAND_BODIES]


@pytest.mark.parametrize('hw,name', BAND_CASES, ids=['%dx%d %s' % (hw + (name,)) for hw, name in BAND_CASES])
def test_uneven_row_bands_equal_the_whole_frame_launch(hw, name):
    """the second part starts at tile0 > 0 and neither part's tile count is a multiple of 8 (at 720p and 1080p tiles_x is 80 or 120:
    a band split there always is)"""
    from pnp_vcve_amd import ops
    frame_walk(hw)
    d = frame_data(hw)
    whole = launch(d, name)                                              # the launch the test above ties to fp64
    tiles_x, rows, row = (hw[1] + 15) // 16, (hw[0] + 15) // 16, BAND_ROW[hw]
    op, args, kw, gate = device_args(d, name)
    kw = dict(kw)
    if name == 'residual in place':
        kw['residual'] = out = kw['residual'].clone()
    else:
        out = torch.full(hw + (64,), float('nan'), device=dev())
    traced = not name.startswith('input conv')
    with gate_word(gate):
        for row0, nrows in ((row, rows - row), (0, row)):               # the lower band second
            wk = sw.walk(tiles_x * nrows, tiles_x * row0, cus(), units=traced)
            assert not sw.coverage_errors(wk, tiles_x * nrows, tiles_x * row0)
            if traced:
                kw['trace'] = new_trace(wk)
            with ops.wino_tile_rows(row0, nrows):
                op(*args, out=out, **kw)
            if traced:
                check_trace(kw['trace'], wk, hw, '%s, tile rows %d..%d' % (name, row0, row0 + nrows - 1))
    assert torch.equal(out, whole)
