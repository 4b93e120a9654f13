"""GPU: the kernels of the reconstruction head (generator.hip head(): the two pixel-shuffle convs and conv_last + the frame), each
addressed alone through pnp_debug_pixel_shuffle_conv / pnp_debug_conv_last with an explicit route, against the float64 reference of
tests/head_ref.py, at the shapes where their launch rules switch and their tiles are ragged:

  conv_last    vector-ALU kernel (KS = 4 below 768 tiles, KS = 1 from there; fp32 planes, byte and RGB0 frames; fp32 and byte output),
               fp32 matrix-core RGB configuration, fp16 RGB body (fp32 and fp16 source map); out_mode 2 and 3 (x4 bilinear)
  pixel shuffle   fp32 tile kernel (4x16 tiles below 1024 8x16 tiles, 8x16 from there), fp16 kernel in the four map combinations,
               split-fp16 kernel (four launches)

Every output is pre-filled (NaN, or two different byte patterns) and has to be written completely.  The project's gates: fp32
routes TOL_CONV (tests/test_gpu_ops.py) against the reference; fp16 routes TOL_F16_KERNEL (tests/test_gpu_fp16.py) against the
reference on fp16-rounded map and weights; the split-fp16 pixel shuffle TOL_CONV / 4 (tests/test_gpu_f16x3.py); an fp16 output map
adds half an fp16 ulp of the reference value.  tests/test_head_ref.py shows that these inputs tell the obvious wrong kernels from the
right one by 1e-3 at the frame edges.

Observed on the MI355X, max |kernel - reference| over all cases of a route (OBSERVED_ON_MI355X below; the last test prints a run's
own): conv_last vector-ALU 2.44e-6, matrix-core RGB 2.44e-6 (both at the same pixel of the 185x497 frame), fp16 RGB body 7.2e-7;
pixel shuffle fp32 3.15e-6, fp16 1.15e-6 (fp16 output: 2.8e-7 beyond the half ulp), split fp16 1.16e-6.  The fp32 and fp16 gates
used here are therefore tighter than the project's: four times the largest figure of the routes they cover, rounded up (1.3e-5 for
2e-5, 5e-6 for 3e-5); the split-fp16 gate already sits at that factor."""
import functools

import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

TOL_CONV = 2e-5              # tests/test_gpu_ops.py: the exact-fp32 conv on this data scale
TOL_F16_KERNEL = 3e-5        # tests/test_gpu_fp16.py: fp32 accumulation of fp16 x fp16 products, against fp16-rounded operands
TOL_X3 = TOL_CONV / 4        # tests/test_gpu_f16x3.py: the split-fp16 kernels
HALF_ULP_F16 = 2.0 ** -11    # an fp16 output map: round-to-nearest of the fp32 value

OBSERVED_ON_MI355X = {'last_valu': 2.442e-06, 'last_mfma': 2.442e-06, 'last_f16': 7.184e-07, 'last_valu_x2': 9.158e-07,
                      'ps_f32': 3.149e-06, 'ps_f16': 1.154e-06, 'ps_f16_out16': 2.752e-07, 'ps_f16x3': 1.155e-06}
GATE_F32 = 1.3e-5            # >= 4 x 3.149e-6, the largest fp32 route (ps_f32)
GATE_F16 = 5e-6              # >= 4 x 1.154e-6, the largest fp16 route (ps_f16)
GATE_X3 = TOL_X3             # 4.3 x 1.155e-6
assert GATE_F32 <= TOL_CONV and GATE_F16 <= TOL_F16_KERNEL
assert GATE_F32 >= 4 * max(OBSERVED_ON_MI355X[k] for k in ('last_valu', 'last_mfma', 'ps_f32'))
assert GATE_F16 >= 4 * max(OBSERVED_ON_MI355X[k] for k in ('last_f16', 'ps_f16', 'ps_f16_out16'))
assert GATE_X3 >= 4 * OBSERVED_ON_MI355X['ps_f16x3']

_seen = {}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())          # a copy: the shared inputs are read-only


def ident(hw):
    return '%dx%d' % hw


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(route, case, out, ref, gate, rel=0.0):
    """out within gate + rel * |ref| of ref everywhere, every element written; books the largest error under `route`"""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    unwritten = int(np.isnan(out).sum())
    assert unwritten == 0, '%s %s: %d elements not written' % (route, case, unwritten)
    o = out.astype(np.float64)
    assert np.isfinite(o).all(), (route, case)
    err = np.abs(o - ref)
    over = err - rel * np.abs(ref)
    worst = float(over.max())
    _seen[route] = max(_seen.get(route, 0.0), worst)
    at = np.unravel_index(int(over.argmax()), over.shape)
    print('HEAD_EDGES %-14s %-28s err %.3e (max |err| %.3e) gate %.1e at %s' % (route, case, worst, float(err.max()), gate, at))
    assert worst <= gate, (route, case, worst, gate, at)


# ---------------------------------------------------------------- conv_last
@functools.lru_cache(maxsize=None)
def packed_last(which='seeded'):
    from pnp_vcve_amd import ops
    if which == 'zero':
        w, b = np.zeros((3, 64, 3, 3), np.float32), np.zeros(3, np.float32)
    else:
        w, b = R.clamp_weights() if which == 'clamp' else R.last_weights()
    return ops.pack_conv_last(G(w), G(b))


def last_frame(H, W, mode, form, planes=None):
    if form == 'u8':
        return G(R.frame_bytes(H, W, mode))
    p = R.frame_planes(H, W, mode) if planes is None else planes
    return G(R.rgb0_from_planes(p)) if form == 'rgb0' else G(p)


def run_last(H, W, mode, route, form='planes', src16=False, planes=None, frame=None, want='f32', which='seeded', precision=0, act=0,
             sentinel=0x5A):
    """-> (out (3,H,W) float32 or None, out_u8 (H,W,3) or None); want 'f32' | 'u8' | 'both'"""
    from pnp_vcve_amd import ops
    x = G(R.feature_map('last', H, W))
    x = x.half() if src16 else x
    f = last_frame(H, W, mode, form, planes) if frame is None else frame
    out = torch.full((3, H, W), float('nan'), device=dev()) if want != 'u8' else False
    out8 = torch.full((H, W, 3), sentinel, device=dev(), dtype=torch.uint8) if want != 'f32' else False
    o, o8 = ops.head_conv_last(x, packed_last(which), f, out_mode=mode, act=act, route=route, precision=precision, frame_form=form,
                               out=out, out_u8=out8)
    torch.cuda.synchronize()
    return (o.cpu().numpy() if o is not None else None), (o8.cpu().numpy() if o8 is not None else None)


def run_last_bytes(*args, **kw):
    """run_last with a byte output, twice over two different pre-fills: a byte that is not written differs between the two"""
    o, o8 = run_last(*args, sentinel=0x5A, **kw)
    o_b, o8_b = run_last(*args, sentinel=0xA5, **kw)
    assert np.array_equal(o8, o8_b), 'bytes left unwritten: %d' % int((o8 != o8_b).sum())
    if o is not None:
        assert np.array_equal(bits(o), bits(o_b))
    return o, o8


def last_ref(H, W, mode, planes=None, operands='fp64'):
    p = R.frame_planes(H, W, mode) if planes is None else planes
    return R.last_term_case(H, W, operands) + R.conv_last_base(p, mode)


LAST_ALL = [(2, hw) for hw in R.LAST_MODE2] + [(3, hw) for hw in R.LAST_MODE3]
LAST_FORMS = [(2, (37, 53)), (2, (100, 932)), (2, (185, 497)), (3, (36, 52)), (3, (100, 932)), (3, (188, 500))]
LAST_MATRIX = [(2, (9, 17)), (3, (12, 20)), (2, (37, 53)), (3, (36, 52)), (2, (185, 497)), (3, (188, 500))]
mode_hw = lambda cases: pytest.mark.parametrize('mode,hw', cases, ids=['mode%d-%s' % (m, ident(hw)) for m, hw in cases])      # noqa: E731


@mode_hw(LAST_ALL)
def test_valu_conv_last(mode, hw):
    """the vector-ALU kernel, fp32 planes in and out, at every shape: sub-tile frames, ragged tiles, XCD remap remainders 7 and 0,
    767 tiles (the last KS = 4 frame) and 768 (the first KS = 1 frame)"""
    out, _ = run_last(*hw, mode, 'valu')
    check('last_valu', 'mode%d %s' % (mode, ident(hw)), out, last_ref(*hw, mode), GATE_F32)


@pytest.mark.parametrize('act', [1, 2])
def test_valu_conv_last_activations(act):
    w, b = R.last_weights()
    ref = R.conv_last_ref(R.feature_map('last', 37, 53), w, b, R.frame_planes(37, 53, 2), 2, act)
    assert np.abs(ref - last_ref(37, 53, 2)).max() > 0.1
    out, _ = run_last(37, 53, 2, 'valu', act=act)
    check('last_valu', 'mode2 37x53 act%d' % act, out, ref, GATE_F32)


@mode_hw(LAST_FORMS)
def test_valu_conv_last_frame_forms_equal_the_planes_form_bit_for_bit(mode, hw):
    """conv_last.hip's claim for IO = 1 / 2: the byte frame through the table and the RGB0 frame give the fp32 value of the planes
    form fed the same values, bit for bit -- on both sides of the 767 / 768 tile switch of both launchers"""
    case = 'mode%d %s' % (mode, ident(hw))
    table = R.planes_from_bytes(R.frame_bytes(*hw, mode))
    from_planes8, _ = run_last(*hw, mode, 'valu', planes=table)
    from_bytes, _ = run_last(*hw, mode, 'valu', form='u8')
    check('last_valu', case + ' u8', from_bytes, last_ref(*hw, mode, table), GATE_F32)
    assert np.array_equal(bits(from_bytes), bits(from_planes8)), int((bits(from_bytes) != bits(from_planes8)).sum())
    from_planes, _ = run_last(*hw, mode, 'valu')
    from_rgb0, _ = run_last(*hw, mode, 'valu', form='rgb0')
    check('last_valu', case + ' rgb0', from_rgb0, last_ref(*hw, mode), GATE_F32)
    assert np.array_equal(bits(from_rgb0), bits(from_planes)), int((bits(from_rgb0) != bits(from_planes)).sum())


@pytest.mark.parametrize('mode,hw,form', [(2, (37, 53), 'u8'), (3, (36, 52), 'u8'), (2, (185, 497), 'planes'), (3, (188, 500), 'rgb0')],
                         ids=['mode2-37x53-u8', 'mode3-36x52-u8', 'mode2-185x497-planes', 'mode3-188x500-rgb0'])
def test_byte_output_is_the_rounding_of_the_launch_own_fp32_planes(mode, hw, form):
    planes = R.planes_from_bytes(R.frame_bytes(*hw, mode)) if form == 'u8' else None
    out, out8 = run_last_bytes(*hw, mode, 'valu', form=form, want='both')
    check('last_valu', 'mode%d %s %s both' % (mode, ident(hw), form), out, last_ref(*hw, mode, planes), GATE_F32)
    assert np.array_equal(out8, R.to_bytes(out)), int((out8 != R.to_bytes(out)).sum())
    _, only8 = run_last_bytes(*hw, mode, 'valu', form=form, want='u8')
    assert np.array_equal(only8, out8), int((only8 != out8).sum())
    fp32_only, _ = run_last(*hw, mode, 'valu', form=form)
    assert np.array_equal(bits(fp32_only), bits(out))


def test_byte_frame_of_all_256_values_comes_back_unchanged():
    frame = (np.arange(16 * 16 * 3) % 256).astype(np.uint8).reshape(16, 16, 3)
    assert len(np.unique(frame)) == 256
    _, out8 = run_last_bytes(16, 16, 2, 'valu', form='u8', frame=G(frame), want='u8', which='zero')
    assert np.array_equal(out8, frame), int((out8 != frame).sum())


def test_byte_output_rounds_ties_to_even():
    k = np.arange(3 * 16 * 16) % 255
    planes = ((k + 0.5) / 255.0).astype(np.float32).reshape(3, 16, 16)
    prod = planes * np.float32(255.0)
    ties = prod - np.floor(prod) == 0.5
    assert ties.sum() >= 100, int(ties.sum())                  # exact ties in float32, of both parities
    assert (np.floor(prod[ties]) % 2 == 0).any() and (np.floor(prod[ties]) % 2 == 1).any()
    out, out8 = run_last_bytes(16, 16, 2, 'valu', planes=planes, want='both', which='zero')
    assert np.array_equal(bits(out), bits(planes))             # zero weights and bias: the sum is the frame
    assert np.array_equal(out8, R.to_bytes(planes)), int((out8 != R.to_bytes(planes)).sum())


def test_byte_output_clamps_on_both_sides():
    """conv_last weights at twice the scale (every product, sum and rounding error twice as large: twice the gate)"""
    H, W = R.CLAMP_HW
    out, out8 = run_last_bytes(H, W, 2, 'valu', want='both', which='clamp')
    check('last_valu_x2', 'mode2 %dx%d clamp' % (H, W), out, R.clamp_case_ref(), 2 * GATE_F32)
    assert (out < 0).mean() >= 0.1 and (out > 1).mean() >= 0.1, ((out < 0).mean(), (out > 1).mean())
    exp = R.to_bytes(out)
    assert (exp == 0).mean() >= 0.1 and (exp == 255).mean() >= 0.1
    assert np.array_equal(out8, exp), int((out8 != exp).sum())


@mode_hw(LAST_MATRIX)
def test_mfma_conv_last(mode, hw):
    """the fp32 matrix-core RGB configuration with its own copy of the bilinear in the epilogue"""
    out, _ = run_last(*hw, mode, 'f32')
    check('last_mfma', 'mode%d %s' % (mode, ident(hw)), out, last_ref(*hw, mode), GATE_F32)


@pytest.mark.parametrize('src16', [False, True], ids=['src32', 'src16'])
@mode_hw(LAST_MATRIX)
def test_f16_conv_last(mode, hw, src16):
    """the fp16 RGB body (prefetch_rgb_operands); at 768 tiles its persistent blocks walk more than one tile"""
    out, _ = run_last(*hw, mode, 'f16', src16=src16)
    check('last_f16', 'mode%d %s %s' % (mode, ident(hw), 'src16' if src16 else 'src32'), out, last_ref(*hw, mode, operands='fp16'),
          GATE_F16)


def test_conv_last_auto_route_is_the_kernel_the_precision_names():
    for mode, hw in ((2, (37, 53)), (3, (36, 52))):
        valu, _ = run_last(*hw, mode, 'valu')
        f16, _ = run_last(*hw, mode, 'f16')
        f16s, _ = run_last(*hw, mode, 'f16', src16=True)
        for prec, src16, named in ((0, False, valu), (2, False, valu), (1, False, f16), (1, True, f16s)):
            auto, _ = run_last(*hw, mode, 'auto', precision=prec, src16=src16)
            assert np.array_equal(bits(auto), bits(named)), (mode, hw, prec, src16)
        assert not np.array_equal(bits(valu), bits(f16))
        valu8, _ = run_last(*hw, mode, 'valu', form='u8')
        auto8, _ = run_last(*hw, mode, 'auto', form='u8')
        assert np.array_equal(bits(auto8), bits(valu8))


# ---------------------------------------------------------------- pixel-shuffle conv
@functools.lru_cache(maxsize=None)
def packed_shuffle(which='seeded'):
    """-> (packed, fp16 twin, split twin)"""
    from pnp_vcve_amd import ops
    w, b = R.identity_shuffle_weights() if which == 'identity' else R.shuffle_weights()
    packed = ops.pack_pixel_shuffle(G(w), G(b))
    images = packed[:4 * 36864]
    return packed, ops.f16_image(images), ops.f16x3_image(images)


def run_shuffle(h, w, route, act=2, src16=False, out16=False, queue=False, which='seeded', x=None, auto_kind=0):
    from pnp_vcve_amd import ops
    packed, twin16, twin_x3 = packed_shuffle(which)
    twin = {'f32': None, 'f16': twin16, 'f16x3': twin_x3, 'auto': (None, twin16, twin_x3)[auto_kind]}[route]
    xd = G(R.feature_map('ps', h, w) if x is None else x)
    xd = xd.half() if src16 else xd
    out = torch.full((2 * h, 2 * w, 64), float('nan'), device=dev(), dtype=torch.float16 if out16 else torch.float32)
    q = torch.zeros(16, dtype=torch.int32, device=dev()) if queue else None
    ops.head_pixel_shuffle_conv(xd, packed, act=act, route=route, twin=twin, out=out, tile_queue=q)
    torch.cuda.synchronize()
    if queue:
        assert not q.cpu().numpy().any(), 'the tile queue is not left zeroed'
    return out.cpu().numpy()


PS_SMALL = [(5, 17), (37, 53), (121, 1009)]
hw_param = lambda shapes: pytest.mark.parametrize('hw', shapes, ids=ident)      # noqa: E731


@hw_param(R.PIXEL_SHUFFLE)
def test_f32_pixel_shuffle(hw):
    """the fp32 tile kernel: sub-tile and ragged frames, 945 8x16 tiles (the last frame on 4x16 tiles), 1024 (the first on 8x16)"""
    check('ps_f32', ident(hw), run_shuffle(*hw, 'f32'), R.shuffle_case(*hw, 2), GATE_F32)


@pytest.mark.parametrize('out16', [False, True], ids=['out32', 'out16'])
@pytest.mark.parametrize('src16', [False, True], ids=['src32', 'src16'])
@hw_param(PS_SMALL)
def test_f16_pixel_shuffle(hw, src16, out16):
    out = run_shuffle(*hw, 'f16', src16=src16, out16=out16)
    case = '%s %s %s' % (ident(hw), 'src16' if src16 else 'src32', 'out16' if out16 else 'out32')
    check('ps_f16_out16' if out16 else 'ps_f16', case, out, R.shuffle_case(*hw, 2, 'fp16'), GATE_F16, rel=HALF_ULP_F16 if out16 else 0.0)


@pytest.mark.parametrize('queue', [False, True], ids=['static', 'queue'])
@hw_param(PS_SMALL)
def test_f16x3_pixel_shuffle(hw, queue):
    """four launches with hand-computed output strides; with and without the generator's tile queue"""
    check('ps_f16x3', '%s %s' % (ident(hw), 'queue' if queue else 'static'), run_shuffle(*hw, 'f16x3', queue=queue), R.shuffle_case(*hw, 2),
          GATE_X3)


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('route', ['f32', 'f16', 'f16x3'])
def test_pixel_shuffle_activations(route, act):
    ref = R.shuffle_case(37, 53, act, 'fp16' if route == 'f16' else 'fp64')
    assert np.abs(ref - R.shuffle_case(37, 53, 2, 'fp16' if route == 'f16' else 'fp64')).max() > 0.05
    gate = {'f32': GATE_F32, 'f16': GATE_F16, 'f16x3': GATE_X3}[route]
    check('ps_' + route, '37x53 act%d' % act, run_shuffle(37, 53, route, act=act), ref, gate)


@pytest.mark.parametrize('route,src16,out16', [('f32', False, False), ('f16', False, False), ('f16', True, True), ('f16x3', False, False)],
                         ids=['f32', 'f16', 'f16-maps16', 'f16x3'])
def test_pixel_shuffle_layout_with_identity_weights(route, src16, out16):
    """conv channel 4c + sub copies input channel identity_channel(c, sub): the output is a pure rearrangement of the input, exactly
    (values exact in fp16), so a layout slip shows at the sub-pixel and channel where it happens"""
    x = R.identity_map(5, 17)
    out = run_shuffle(5, 17, route, act=0, src16=src16, out16=out16, which='identity', x=x).astype(np.float32)
    exp = R.identity_shuffle_expected(x)
    bad = np.argwhere(out != exp)
    assert bad.size == 0, 'first mismatches (row, column, channel): %s' % bad[:8].tolist()


def test_pixel_shuffle_auto_route_is_the_kernel_the_twin_names():
    for kind, route in enumerate(('f32', 'f16', 'f16x3')):
        named = run_shuffle(37, 53, route)
        auto = run_shuffle(37, 53, 'auto', auto_kind=kind)
        assert np.array_equal(bits(auto), bits(named)), route
    assert not np.array_equal(bits(run_shuffle(37, 53, 'f32')), bits(run_shuffle(37, 53, 'f16')))


def test_zz_observed_maxima():
    """prints what this run observed per route (the figures of OBSERVED_ON_MI355X)"""
    print('HEAD_EDGES observed maxima: ' + ', '.join('%s %.3e' % kv for kv in sorted(_seen.items())))
