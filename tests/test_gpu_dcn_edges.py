"""GPU: dcn_window_kernel (pnp_vcve_amd/csrc/dcn.hip), both instantiations, against the float64 reference of tests/dcn_ref.py at
window, tile and frame edges: ragged and sub-tile frames, samples exactly on -1 / 0 / H-1 / H and on the window's edges, waves
with no, some and only fallback samples, blocks that walk several tiles, XCD bands without tiles, saturating fp16 operands.

fp16=False is held to operands='fp64' within tol32, fp16=True to operands='fp16' (the project's operand rule, accumulated in
float64) within tol16.  Both tolerances come from the reference alone (dcn_ref.dcn_bounds); tests/test_dcn_ref.py shows that the
inputs tell a wrong kernel from a right one at these tolerances."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dcn_ref as R

pytestmark = pytest.mark.gpu

FLOW = pytest.mark.parametrize('with_flow', [False, True], ids=['noflow', 'flow'])
PREC = pytest.mark.parametrize('fp16', [False, True], ids=['fp32', 'fp16'])


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def G(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev())          # a copy: the shared inputs are read-only


def device_grid():
    from pnp_vcve_amd import _native
    n = int(_native.lib().pnp_dcn_trace_u64s())
    assert n > 0 and n % 64 == 0, n
    return n // 64


@functools.lru_cache(maxsize=None)
def prepared(name, with_flow):
    """inputs, references, tolerances and census of one case: computed once, shared by the tests, never written to"""
    c = R.dcn_case(name, grid=device_grid()) if name == 'strip_walk' else R.dcn_case(name)
    if not with_flow:
        c['flow'] = None
    h, w = c['x'].shape[:2]
    b = R.dcn_bounds(**c)
    counts = R.census_counts(*R.dcn_census(c['offset'], c['flow'], h, w))
    for v in list(c.values()) + [b['ref64'], b['ref16']]:
        if v is not None:
            v.setflags(write=False)
    return c, b, counts


def run(c, fp16):
    from pnp_vcve_amd import ops
    out = ops.modulated_deform_conv_nhwc(G(c['x']), G(c['offset']), G(c['mask_logits']), G(c['weight']), G(c['bias']),
                                         flow=G(c['flow']), fp16=fp16)
    return out.cpu().numpy().astype(np.float64)


def check(tag, out, b, counts, fp16, extra=''):
    ref, tol = (b['ref16'], b['tol16']) if fp16 else (b['ref64'], b['tol32'])
    assert out.shape == ref.shape
    finite = bool(np.isfinite(out).all())
    err = float(np.abs(out - ref).max()) if finite else float('nan')
    print('DCN_EDGES %s %s err %.3e tol %.3e | e32 %.3e tol32 %.3e n16 %.3e tol16 %.3e | %s%s'
          % (tag, 'fp16' if fp16 else 'fp32', err, tol, b['e32'], b['tol32'], b['n16'], b['tol16'],
             ' '.join('%s=%d' % kv for kv in counts.items()), extra))
    assert finite, tag
    assert err <= tol, (tag, err, tol)


@PREC
@FLOW
def test_main_44x52(with_flow, fp16):
    """ragged last tile row (4 of 8) and column (4 of 16); every sample class of the census populated (test_dcn_ref.py)"""
    c, b, counts = prepared('main_44x52', with_flow)
    check('main_44x52/%s' % ('flow' if with_flow else 'noflow'), run(c, fp16), b, counts, fp16)


@PREC
@FLOW
@pytest.mark.parametrize('hw', R.GEOMETRY, ids=['%dx%d' % g for g in R.GEOMETRY])
def test_small_and_ragged_frames(hw, with_flow, fp16):
    """frames smaller than a half, a tile and a window; fewer than 8 tiles, so some blockIdx.x % 8 bands are empty"""
    c, b, counts = prepared('geo_%dx%d' % hw, with_flow)
    check('geo_%dx%d/%s' % (hw + ('flow' if with_flow else 'noflow',)), run(c, fp16), b, counts, fp16)


@PREC
def test_flow_folded_into_the_offsets(fp16):
    """same sample positions as the main case, but the windows are placed without the flow: far more samples take the global
    path, and both forms meet the same reference"""
    c, b, counts = prepared('flow_folded', True)
    m, mb, mcounts = prepared('main_44x52', True)
    assert np.array_equal(b['ref64'], mb['ref64']) and np.array_equal(b['ref16'], mb['ref16'])
    glob, mglob = counts['glob_near'] + counts['glob_other'], mcounts['glob_near'] + mcounts['glob_other']
    assert glob > 1.5 * mglob, (glob, mglob)
    check('flow_folded', run(c, fp16), b, counts, fp16)


def run_f32_traced(c):
    """the fp32 kernel through pnp_dcn_nhwc_f32_ex -> (out, trace (blocks, 8 waves, 8 words))"""
    from pnp_vcve_amd import _native, ops
    L = _native.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    x = G(c['x'])
    h, w, _ = x.shape
    refc = torch.tensor([L.pnp_dcn_ref_channel(i) for i in range(448)], device=x.device)
    src = torch.cat([G(c['offset']), G(c['mask_logits'])], 0)
    om = torch.zeros((448, h, w), device=x.device, dtype=torch.float32)
    om[refc >= 0] = src[refc[refc >= 0]]
    om = om.permute(1, 2, 0).contiguous()
    wp, bias, flow = ops.pack_conv3x3(G(c['weight'])), G(c['bias']), G(c['flow'])
    nq = int(L.pnp_dcn_trace_u64s())
    trace = torch.zeros(nq, dtype=torch.int64, device=x.device)
    out = torch.empty_like(x)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(L.pnp_dcn_nhwc_f32_ex(P(x), P(om), P(flow[0]) if flow is not None else P(None),
                                        P(flow[1]) if flow is not None else P(None), P(wp), P(bias), P(out), h, w, P(trace), st),
                  'pnp_dcn_nhwc_f32_ex')
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), trace.cpu().numpy().reshape(nq // 64, 8, 8)


@PREC
@FLOW
def test_strip_walk(with_flow, fp16):
    """sized from the device so that every block walks 2 or more tiles and some walk 3 (20 rows: three tile rows, the last one
    ragged); consecutive tiles of a block differ in flow and in fallback pattern.  The fp32 run is traced: word 7 = tiles/wave."""
    grid = device_grid()
    c, b, counts = prepared('strip_walk', with_flow)
    h, w = c['x'].shape[:2]
    tiles = 3 * ((w + 15) // 16)
    tag = 'strip_walk_%dx%d_grid%d/%s' % (h, w, grid, 'flow' if with_flow else 'noflow')
    if fp16:
        check(tag, run(c, True), b, counts, True)
        return
    out, trace = run_f32_traced(c)
    per_wave = trace[:, :, 7]
    extra = ' | tiles %d tiles/wave min %d max %d' % (tiles, per_wave.min(), per_wave.max())
    check(tag, out, b, counts, False, extra)
    assert per_wave.min() >= 2 and per_wave.max() >= 3, extra
    assert int(per_wave.sum()) == 8 * tiles, (int(per_wave.sum()), tiles)


def test_fp16_operands_saturate():
    """One activation of 1e6 and one of -1e6 in the main case.  Every other fp16 operand path saturates to +-65504 (f16_util.h
    to_h4); the gathered A operand of the DCN kernel has to as well, or the activation becomes inf and, once it meets a weight of
    the other sign, NaN.  Pixels that sample neither activation keep the main case's tol16.  Pixels that sample one are held to
    the saturated-operand reference within 1e-3 of the pixel's largest output (the norm in which 'relative' is meaningful for a
    64-vector whose entries are one shared saturated term times 64 weights of any size): a saturated operand is the same number
    in the kernel and in the reference, an unsaturated one of ~1e4 differs by at most one fp16 ulp, 2^-10 relative."""
    c, b, counts = prepared('main_44x52', True)
    s = R.dcn_case('saturation')
    ref = R.dcn_reference(**s, operands='fp16')
    touched = np.abs(ref - b['ref16']).max(axis=2) > 0          # pixels whose samples reach one of the two activations
    assert 8 <= int(touched.sum()) < touched.size // 4
    assert np.abs(ref).max() > 1e3                               # saturated terms are there: 65504 * 0.06 * ...
    out = run(s, True)
    n_bad = int((~np.isfinite(out)).sum())
    rest = float(np.abs(out - ref)[~touched].max()) if n_bad == 0 else float('nan')
    rel = float((np.abs(out - ref).max(axis=2)[touched] / np.abs(ref).max(axis=2)[touched]).max()) if n_bad == 0 else float('nan')
    print('DCN_EDGES saturation fp16 non-finite %d | touched pixels %d rel err %.3e (bound 1e-3) | other pixels err %.3e tol16 %.3e'
          % (n_bad, int(touched.sum()), rel, rest, b['tol16']))
    assert n_bad == 0
    assert rest <= b['tol16']
    assert rel <= 1e-3
