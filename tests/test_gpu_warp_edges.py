"""GPU: the MV-alignment warp kernels (pnp_vcve_amd/csrc/warp.hip), every instantiation, against the float64 reference of
tests/warp_ref.py at edges, ties and tails: taps leaving the frame on all four sides, samples aimed exactly at -1, 0, size-1 and
size, the .5 ties of the nearest rounding, odd H (the masked second row of the 64-kernel's row pair), W % 16 of 1, 15 and 0, frames
of one pixel, one block and several, the general kernel's grid-stride loop, infinite / NaN / overflowing vectors, saturating fp16.

bilinear is held to |out - ref| <= warp_tol = 6 * 2^-24 * max|x|, nearest to array_equal; both come from the reference alone, and
tests/test_warp_ref.py shows that the inputs tell a wrong kernel from a right one at these gates.

Instantiations and the tests that hold them to the reference:
  mv_warp_nhwc64_kernel<false, false, 2> / <false, true, 2>   test_mv_warp_nhwc[c64_*]
  mv_warp_nhwc64_kernel<true, false, 2> / <true, true, 2>     test_fp16_output_is_the_rounded_fp32_output[c64_*]
  mv_warp_nhwc_kernel<false, false> / <false, true>           test_mv_warp_nhwc[c4_* c8_* c60_* c128_*], through the grid-stride
                                                              loop in test_mv_warp_nhwc[c128_258x256_frac]
  mv_warp_nhwc_kernel<true, false> / <true, true>             test_fp16_output_is_the_rounded_fp32_output[c8_*]
  flow_warp_nchw_kernel, both modes                           test_flow_warp_nchw[*]
Not tested: launch_mv_warp_nhwc sends a 64-channel map of 2^24 pixels or more (4 GB) to the general kernel; that dispatch stays
untested."""
import functools

import numpy as np
import pytest
import torch

import warp_ref as R

pytestmark = pytest.mark.gpu

MODES = ('bilinear', 'nearest')
F16_CASES = ['c%d_%s_%s_sat' % (c, f, k) for c in (64, 8) for f in ('3x17', '17x47') for k in ('edge', 'wild')]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())          # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=4)
def prepared(name):
    """inputs, both references, tolerance and census of one case: computed once, shared by the tests, never written to"""
    c = R.warp_case(name)
    p = R.parse(name)
    ref_fn = R.warp_ref if p['n'] is None else R.warp_ref_nchw
    refs = {m: ref_fn(c['x'], c['flow'], m) for m in MODES}
    flows = c['flow'][None] if p['n'] is None else c['flow']
    ix, iy = R.coords(p['h'], p['w'], flows)
    wild = ~(np.isfinite(ix) & np.isfinite(iy))              # (n, h, w)
    census = R.census_line(R.warp_census(p['h'], p['w'], flows[0]))
    for v in (c['x'], c['flow'], wild) + tuple(refs.values()):
        v.setflags(write=False)
    return c, p, refs, R.warp_tol(c['x']), wild, census


def kernel_name(p, f16=False):
    if p['n'] is not None:
        return 'flow_warp_nchw'
    return ('nhwc64' if p['c'] == 64 else 'nhwc') + ('<f16>' if f16 else '<f32>')


def check(name, kernel, mode, out, ref, tol, census, extra=''):
    assert out.shape == ref.shape and out.dtype == np.float64
    finite = bool(np.isfinite(out).all())
    err = float(np.abs(out - ref).max()) if finite else float('nan')
    gate = tol if mode == 'bilinear' else 0.0
    print('WARP_EDGES %s %s %s err %.3e tol %.3e | %s%s' % (name, kernel, mode, err, gate, census, extra))
    assert finite, (name, mode)
    if mode == 'nearest':
        assert np.array_equal(out, ref), (name, err, int((out != ref).sum()))
    else:
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize('name', R.nhwc_cases() + [R.BIG])
def test_mv_warp_nhwc(name):
    """C = 64: mv_warp_nhwc64_kernel; C = 4, 8, 60, 128: mv_warp_nhwc_kernel (R.BIG: more float4 than its grid has threads)"""
    from pnp_vcve_amd import ops
    c, p, refs, tol, wild, census = prepared(name)
    x, fx, fy = G(c['x']), G(c['flow'][..., 0]), G(c['flow'][..., 1])
    for mode in MODES:
        out = ops.mv_warp_nhwc(x, fx, fy, interpolation=mode).cpu().numpy().astype(np.float64)
        check(name, kernel_name(p), mode, out, refs[mode], tol, census)
        assert not out[wild[0]].any()                        # a non-finite chain has no tap: zeros, not ATen's NaN


@pytest.mark.parametrize('name', R.nchw_cases())
def test_flow_warp_nchw(name):
    from pnp_vcve_amd import ops
    c, p, refs, tol, wild, census = prepared(name)
    x, flow = G(c['x']), G(c['flow'])
    for mode in MODES:
        out = ops.flow_warp(x, flow, interpolation=mode).cpu().numpy().astype(np.float64)
        check(name, kernel_name(p), mode, out, refs[mode], tol, census)
        assert not out.transpose(0, 2, 3, 1)[wild].any()


@pytest.mark.parametrize('mode', MODES)
def test_general_kernel_and_64_kernel_are_bit_identical(mode):
    """"the same expression, in the same order" (warp.hip): a 128-channel map through the general kernel, its two 64-channel halves,
    made contiguous, through the 64-kernel"""
    from pnp_vcve_amd import ops
    c, p, refs, tol, wild, census = prepared('c128_17x47_edge')
    x, fx, fy = G(c['x']), G(c['flow'][..., 0]), G(c['flow'][..., 1])
    whole = ops.mv_warp_nhwc(x, fx, fy, interpolation=mode)
    halves = torch.cat([ops.mv_warp_nhwc(x[..., s:s + 64].contiguous(), fx, fy, interpolation=mode) for s in (0, 64)], dim=2)
    d = float((whole - halves).abs().max())
    print('WARP_EDGES c128_17x47_edge nhwc<f32> vs 2 x nhwc64<f32> %s max|d| %.3e differing %d | %s'
          % (mode, d, int((whole != halves).sum()), census))
    assert torch.equal(whole, halves), d


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', F16_CASES)
def test_fp16_output_is_the_rounded_fp32_output(name, mode):
    """features x 1000 with one activation of 1e6 that a sample reads: the fp16 map is the saturated, round-to-nearest-even fp32
    result of the same call, bit for bit, and finite.  Against the reference: nearest is a copy, so h16(ref) exactly; bilinear is
    within warp_tol before the rounding and half an fp16 ulp (2^-11 relative, 2^-25 below the normal range) after it."""
    from pnp_vcve_amd import ops
    c, p, refs, tol, wild, census = prepared(name)
    x, fx, fy = G(c['x']), G(c['flow'][..., 0]), G(c['flow'][..., 1])
    o32 = ops.mv_warp_nhwc(x, fx, fy, interpolation=mode)
    o16 = ops.mv_warp_nhwc_f16(x, fx, fy, interpolation=mode)
    assert o16.dtype == torch.float16 and o16.shape == o32.shape
    a16, a32 = o16.cpu().numpy(), o32.cpu().numpy()
    sat = np.clip(refs[mode], -R.F16_MAX, R.F16_MAX)
    err = np.abs(a16.astype(np.float64) - (R.h16(sat).astype(np.float64) if mode == 'nearest' else sat))
    bound = 0.0 if mode == 'nearest' else tol + 2.0 ** -11 * (np.abs(sat) + tol) + 2.0 ** -25
    print('WARP_EDGES %s %s %s fp16 == h16(fp32): %s | max %.1f saturated %d | err vs saturated ref %.3e (largest bound %.3e) | %s'
          % (name, kernel_name(p, True), mode, np.array_equal(a16, R.h16(a32)), float(a16.astype(np.float64).max()),
             int((np.abs(a16.astype(np.float64)) == R.F16_MAX).sum()), float(err.max()), float(np.max(bound)), census))
    assert np.isfinite(a16.astype(np.float64)).all() and a32.max() > R.F16_MAX
    assert torch.equal(o16, o32.clamp(-65504, 65504).half()) and np.array_equal(a16, R.h16(a32))
    assert (a16 == np.float16(R.F16_MAX)).any()
    if mode == 'nearest':
        assert np.array_equal(a16, R.h16(refs[mode]))
    else:
        assert (err <= bound).all(), float((err - bound).max())


def test_fp16_generator_with_nearest_alignment_tracks_the_fp32_path():
    """precision 'fp16' with flow_inter 'nearest' launches mv_warp_nhwc64_kernel<true, true, 2>, the pair no other generator test has"""
    import test_gpu_fp16 as F16
    syn = F16.gu.syn
    cfg = dict(syn.DEFAULT_GENERATOR_CFG, flow_inter='nearest', num_blocks=2)
    m = F16._gen_model(cfg, syn.make_state_dict(cfg, seed=5100, par_gain=10.0))
    clip = syn.make_clip(seed=5101, n=1, t=3, h=64, w=96, slices='IBBBP')
    a = {k: F16.G(v) for k, v in clip.items()}
    outs = []
    for f16 in (False, True):
        m.fp16_enabled = f16
        with torch.no_grad():
            outs.append(m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions']).cpu())
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    scale = max(1.0, float(outs[0].abs().max()))
    d = float((outs[0] - outs[1]).abs().max()) / scale
    print('WARP_EDGES generator fp16 + nearest 64x96 t=3: max|fp16 - fp32| / scale = %.3e (TOL_F16_PATH %.1e)' % (d, F16.TOL_F16_PATH))
    assert 0.0 < d < F16.TOL_F16_PATH, d
