"""Tensor-level wrappers over the C ABI (device pointers + the current HIP stream).

PyTorch is plumbing here: it owns device memory and the stream; every computation
runs in libpnpvcve_hip.so.  All functions require CUDA(HIP) fp32 contiguous tensors (the frame converters and the metrics also take
uint8 frames) and raise otherwise -- there is deliberately no CPU path.
"""
import collections
import contextlib
import ctypes

import torch

from . import _native


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _on_device_of_first_tensor(fn):
    """Run the wrapper with the first tensor argument's device current: the launch goes to torch's current stream of
    THAT device (a process may hold tensors on several GPUs), like generator.forward does."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        first = next((a for a in args if isinstance(a, torch.Tensor)), None)
        if first is None:
            first = next((a[0] for a in args if isinstance(a, (list, tuple)) and a and isinstance(a[0], torch.Tensor)), None)
        if first is not None and first.is_cuda:
            with torch.cuda.device(first.device):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return wrapped


def _chk(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32, got {t.dtype}')
    return t.contiguous()


_WARP_MODES = {'bilinear': 0, 'nearest': 1}       # F.grid_sample modes flow_warp.py:47 can receive through flow_inter


@_on_device_of_first_tensor
def flow_warp(x, flow, interpolation='bilinear', padding_mode='zeros', align_corners=True):
    """Drop-in for mmedit.models.common.flow_warp (flow_warp.py:6-50).
    x (n,c,h,w), flow (n,h,w,2) in pixels."""
    if x.size()[-2:] != flow.size()[1:3]:
        raise ValueError(f'The spatial sizes of input ({x.size()[-2:]}) and '
                         f'flow ({flow.size()[1:3]}) are not the same.')
    if interpolation not in _WARP_MODES or padding_mode != 'zeros' or not align_corners:
        raise NotImplementedError("only 'bilinear' | 'nearest' / zeros / align_corners=True (what the generator can ask for)")
    x, flow = _chk(x, 'x'), _chk(flow, 'flow')
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    _native.check(_native.lib().pnp_flow_warp_nchw_mode_f32(_ptr(x), _ptr(flow), _ptr(out), n, c, h, w, _WARP_MODES[interpolation],
                                                            _stream()), 'pnp_flow_warp_nchw_mode_f32')
    return out


@_on_device_of_first_tensor
def mv_warp_nhwc(feat, flow_x, flow_y, interpolation='bilinear'):
    """feat (h,w,c) pixel-major; flow_x/flow_y (h,w)."""
    feat, flow_x, flow_y = _chk(feat, 'feat'), _chk(flow_x, 'flow_x'), _chk(flow_y, 'flow_y')
    h, w, c = feat.shape
    out = torch.empty_like(feat)
    _native.check(_native.lib().pnp_mv_warp_nhwc_mode_f32(_ptr(feat), _ptr(flow_x), _ptr(flow_y), _ptr(out), h, w, c,
                                                          _WARP_MODES[interpolation], _stream()), 'pnp_mv_warp_nhwc_mode_f32')
    return out


@_on_device_of_first_tensor
def nchw_to_nhwc(x):
    x = _chk(x, 'x')
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), device=x.device, dtype=x.dtype)
    _native.check(_native.lib().pnp_nchw_to_nhwc_f32(_ptr(x), _ptr(out), n, c, h, w, _stream()), 'nchw_to_nhwc')
    return out


@_on_device_of_first_tensor
def nhwc_to_nchw(x):
    x = _chk(x, 'x')
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), device=x.device, dtype=x.dtype)
    _native.check(_native.lib().pnp_nhwc_to_nchw_f32(_ptr(x), _ptr(out), n, c, h, w, _stream()), 'nhwc_to_nchw')
    return out


@_on_device_of_first_tensor
def caa_predict(q_ew, q_gamma, w1, b1, w2, b2, v1=None, v2=None, softmax=True):
    """Base_Predictor + SEModule (domain_aware.py:172-183, 210-222).
    q_ew/q_gamma: python sequences of floats (host).  Returns (ew (count,E), gamma (count,64))."""
    count = len(q_ew)
    E = w2.shape[0]
    dev = w1.device
    ew = torch.empty((count, E), device=dev, dtype=torch.float32)
    gamma = torch.empty((count, 64), device=dev, dtype=torch.float32)
    qa = (ctypes.c_float * count)(*[float(v) for v in q_ew])
    qg = (ctypes.c_float * count)(*[float(v) for v in q_gamma])
    ts = [_chk(t, 'param') for t in (w1, b1, w2, b2)]
    vs = [(_chk(v, 'param') if v is not None else None) for v in (v1, v2)]
    _native.check(_native.lib().pnp_caa_predict_f32(qa, qg, count, E, int(bool(softmax)), _ptr(ts[0]), _ptr(ts[1]),
                                                    _ptr(ts[2]), _ptr(ts[3]), _ptr(vs[0]), _ptr(vs[1]), _ptr(ew),
                                                    _ptr(gamma), _stream()), 'pnp_caa_predict_f32')
    return ew, gamma


@_on_device_of_first_tensor
def pack_conv3x3(weight, cbase=0, csrc=64, ew=None):
    """OIHW (cout,cin,3,3) [or (E,cout,cin,3,3) with ew (E,)] -> packed image for input
    channels [cbase, cbase+csrc)."""
    weight = _chk(weight, 'weight')
    E = 1
    if weight.dim() == 5:
        E = weight.shape[0]
        ew = _chk(ew, 'ew')
    cout, cin = weight.shape[-4], weight.shape[-3]
    L = _native.lib()
    dst = torch.empty(int(L.pnp_packed_conv_floats(64 if csrc == 64 else 4)), device=weight.device, dtype=torch.float32)
    _native.check(L.pnp_pack_conv3x3_f32(_ptr(weight), _ptr(ew), E, cout, cin, cbase, csrc, _ptr(dst), _stream()),
                  'pnp_pack_conv3x3_f32')
    return dst


@_on_device_of_first_tensor
def pack_conv1x1(weights):
    """three (64,64,1,1) weights -> one tensor of 3 chunks (conv16x16, conv16x8, conv8x8)."""
    L = _native.lib()
    n = int(L.pnp_packed_conv_floats(4))
    dst = torch.empty(3 * n, device=weights[0].device, dtype=torch.float32)
    for j, w in enumerate(weights):
        w = _chk(w, 'w1x1')
        _native.check(L.pnp_pack_conv1x1_f32(_ptr(w), ctypes.c_void_p(dst.data_ptr() + 4 * n * j), _stream()),
                      'pnp_pack_conv1x1_f32')
    return dst


@_on_device_of_first_tensor
def par_tile_flags(par):
    """(3,h,w) partition planes -> int32 (tiles_y, tiles_x) of 8x16 tiles: bit j set iff plane j is nonzero in the tile."""
    par = _chk(par, 'par')
    if par.dim() != 3 or par.shape[0] != 3:
        raise ValueError('par must be (3,h,w)')
    h, w = par.shape[1:]
    out = torch.empty(((h + 7) // 8, (w + 15) // 16), device=par.device, dtype=torch.int32)
    _native.check(_native.lib().pnp_par_tile_flags_f32(_ptr(par), ctypes.c_void_p(out.data_ptr()), h, w, _stream()),
                  'pnp_par_tile_flags_f32')
    return out


@_on_device_of_first_tensor
def par_fold_table(par):
    """(3,h,w) partition planes -> int32 (4 * tiles16, 2): the frame's fold table (csrc/fold_table.h), per 8x8 quadrant in 16x16-tile-major
    order the plane the fold-only Winograd body folds (-1: none) and the bits of its fp32 factor 0.25f * value."""
    par = _chk(par, 'par')
    if par.dim() != 3 or par.shape[0] != 3:
        raise ValueError('par must be (3,h,w)')
    h, w = par.shape[1:]
    out = torch.empty((4 * ((h + 15) // 16) * ((w + 15) // 16), 2), device=par.device, dtype=torch.int32)
    _native.check(_native.lib().pnp_debug_par_fold_table(_ptr(par), ctypes.c_void_p(out.data_ptr()), h, w, _stream()),
                  'pnp_debug_par_fold_table')
    return out


@_on_device_of_first_tensor
def f16_image(packed):
    """fp32 packed weight image (whole chunks) -> fp16 image for conv3x3(..., fp16=True)."""
    packed = _chk(packed, 'packed')
    nchunks, rem = divmod(packed.numel(), 4096)
    if rem:
        raise ValueError('packed image must be whole 4096-float chunks')
    dst = torch.empty(packed.numel(), device=packed.device, dtype=torch.float16)
    _native.check(_native.lib().pnp_f16_image_from_f32(_ptr(packed), ctypes.c_void_p(dst.data_ptr()), nchunks, _stream()),
                  'pnp_f16_image_from_f32')
    return dst


@_on_device_of_first_tensor
def f16x3_image(packed):
    """fp32 packed weight image -> its split image for conv3x3_f16x3: hi = fp16(w), lo = fp16((w - hi) * 2048), interleaved per
    k-step (twice the halfs of f16_image)."""
    packed = _chk(packed, 'packed')
    nchunks, rem = divmod(packed.numel(), 4096)
    if rem:
        raise ValueError('packed image must be whole 4096-float chunks')
    dst = torch.empty(2 * packed.numel(), device=packed.device, dtype=torch.float16)
    _native.check(_native.lib().pnp_f16x3_image_from_f32(_ptr(packed), ctypes.c_void_p(dst.data_ptr()), nchunks, _stream()),
                  'pnp_f16x3_image_from_f32')
    return dst


@_on_device_of_first_tensor
def conv3x3_f16x3(srcs, packed_w, bias=None, gamma=None, packed_w1x1=None, par=None, par_flags=None, residual=None, act=0,
                  trace=None, scaled_w1x1=False, tile_queue=None):
    """conv3x3 in split fp16 (pnp_conv3x3_f16x3, PNP_PREC_F16X3): packed_w / packed_w1x1 are the fp32 images of conv3x3 (their
    split images are made here) or, for 64-channel sources / the 1x1 branches, float16 tensors that already are f16x3_image()
    results.  fp32 sources, fp32 result at fp32-level accuracy.  tile_queue: 16 zeroed int32 (the generator's per-context queue:
    blocks draw their tiles from it instead of walking a static share; left zeroed by every launch)."""
    srcs = [_chk(s, 'src') for s in srcs]
    h, w = srcs[0].shape[:2]
    n = len(srcs)

    def split(p, wide=True):
        if p is None or not wide:
            return None
        if p.dtype == torch.float16:
            if not p.is_cuda or not p.is_contiguous():
                raise TypeError('split weight images must be contiguous CUDA float16 tensors (ops.f16x3_image)')
            return p
        return f16x3_image(p)

    # the RGB frame's image is split too (k = 4 tap + channel: two 32-deep chunks): with it the whole conv is ONE launch; the fp32
    # image still travels for the traced variant, where the RGB link stays on the exact fp32 kernel
    x3 = [split(p) for p in packed_w]
    # scaled_w1x1 (include/pnpvcve_debug.h): the branch images followed by the same images x 1/255, as pnp_generator_pack lays them
    # out -- tiles whose partition values are all 0 or exactly 1/255 (par_flags bits 3..5) then take the masked-operand fast path
    if scaled_w1x1:
        if packed_w1x1 is None or packed_w1x1.dtype != torch.float32:
            raise TypeError('scaled_w1x1: packed_w1x1 must be the fp32 images of pack_conv1x1')
        packed_w1x1 = torch.cat([packed_w1x1.reshape(-1), packed_w1x1.reshape(-1) * (torch.ones((), device=packed_w1x1.device) / 255.0)])
    p_x3 = split(packed_w1x1)
    packed_w = [(_chk(p, 'packed_w') if p.dtype == torch.float32 else None) for p in packed_w]
    vp = lambda ts: (ctypes.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in ts])
    out = torch.empty((h, w, 64), device=srcs[0].device, dtype=torch.float32)
    sc = (ctypes.c_int * n)(*[s.shape[2] for s in srcs])
    keep = [(_chk(t, 'arg') if t is not None else None) for t in (bias, gamma, par, residual)]
    one = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    if tile_queue is not None and (tile_queue.dtype != torch.int32 or tile_queue.numel() < 16 or not tile_queue.is_cuda):
        raise TypeError('tile_queue: 16 int32 on the device')
    if trace is None and not scaled_w1x1 and tile_queue is None:
        _native.check(_native.lib().pnp_conv3x3_f16x3(n, vp(srcs), sc, vp(packed_w), vp(x3), _ptr(keep[0]), _ptr(keep[1]),
                                                      one(p_x3), _ptr(keep[2]), one(par_flags), _ptr(keep[3]), act,
                                                      _ptr(out), h, w, _stream()), 'pnp_conv3x3_f16x3')
    else:       # include/pnpvcve_debug.h: in-kernel timeline, scaled branch images, tile queue
        _native.check(_native.lib().pnp_conv3x3_f16x3_ex(n, vp(srcs), sc, vp(packed_w), vp(x3), _ptr(keep[0]), _ptr(keep[1]),
                                                         one(p_x3), _ptr(keep[2]), one(par_flags), _ptr(keep[3]), act,
                                                         _ptr(out), h, w, int(bool(scaled_w1x1)), one(tile_queue), one(trace), _stream()),
                      'pnp_conv3x3_f16x3_ex')
    return out


@_on_device_of_first_tensor
def conv3x3(srcs, packed_w, bias=None, gamma=None, packed_w1x1=None, par=None, residual=None, act=0, fp16=False,
            variant=None, par_flags=None, trace=None):
    """Fused conv over pixel-major sources [(h,w,64) or (h,w,4)].  See include/pnpvcve.h.
    fp16=True: packed_w / packed_w1x1 are f16_image() tensors and the MFMA operands are fp16.
    variant / par_flags / trace: include/pnpvcve_debug.h (kernel selection, per-tile branch flags, timeline buffer)."""
    if fp16:
        if variant is not None or par_flags is not None:
            raise ValueError('conv3x3(fp16=True): `variant` and `par_flags` select among the fp32 kernels only '
                             '(pnp_conv3x3_f16_ex takes neither)')
        return _conv3x3_f16(srcs, packed_w, bias, gamma, packed_w1x1, par, residual, act, trace)
    srcs = [_chk(s, 'src') for s in srcs]
    h, w = srcs[0].shape[:2]
    n = len(srcs)
    out = torch.empty((h, w, 64), device=srcs[0].device, dtype=torch.float32)
    sp = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    sc = (ctypes.c_int * n)(*[s.shape[2] for s in srcs])
    wp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in packed_w])
    keep = [(_chk(t, 'arg') if t is not None else None) for t in (bias, gamma, packed_w1x1, par, residual)]
    if variant is None and par_flags is None and trace is None:
        _native.check(_native.lib().pnp_conv3x3_f32(n, sp, sc, wp, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                                    _ptr(keep[3]), _ptr(keep[4]), act, _ptr(out), h, w, _stream()),
                      'pnp_conv3x3_f32')
    else:
        _native.check(_native.lib().pnp_conv3x3_f32_ex(n, sp, sc, wp, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                                       _ptr(keep[3]), _ptr(keep[4]), act, _ptr(out), h, w,
                                                       int(variant or 0), _ptr(par_flags), _ptr(trace), _stream()),
                      'pnp_conv3x3_f32_ex')
    return out


def _conv3x3_f16(srcs, packed_w, bias, gamma, packed_w1x1, par, residual, act, trace=None):
    srcs = [_chk(s, 'src') for s in srcs]
    for p in list(packed_w) + ([packed_w1x1] if packed_w1x1 is not None else []):
        if not p.is_cuda or p.dtype != torch.float16 or not p.is_contiguous():
            raise TypeError('fp16 conv: weight images must be contiguous CUDA float16 tensors (ops.f16_image)')
    h, w = srcs[0].shape[:2]
    n = len(srcs)
    out = torch.empty((h, w, 64), device=srcs[0].device, dtype=torch.float32)
    sp = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    sc = (ctypes.c_int * n)(*[s.shape[2] for s in srcs])
    wp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in packed_w])
    keep = [(_chk(t, 'arg') if t is not None else None) for t in (bias, gamma, par, residual)]
    w1 = ctypes.c_void_p(packed_w1x1.data_ptr()) if packed_w1x1 is not None else None
    _native.check(_native.lib().pnp_conv3x3_f16_ex(n, sp, sc, wp, _ptr(keep[0]), _ptr(keep[1]), w1, _ptr(keep[2]),
                                                   _ptr(keep[3]), act, _ptr(out), h, w, _ptr(trace), _stream()),
                  'pnp_conv3x3_f16')
    return out


@_on_device_of_first_tensor
def conv3x3_f16_maps(srcs, packed_w, bias=None, gamma=None, packed_w1x1=None, par=None, par_flags=None, residual=None, act=0,
                     out_f16=False, mirror=False, chain=False, trace=None):
    """The fp16-operand conv with explicit fp16 maps (include/pnpvcve_debug.h, pnp_conv3x3_f16_maps): a source of dtype
    float16 (h,w,64) is read as an fp16 map (the mirror its producer wrote), float32 sources are rounded on the fly.
    out_f16: the output is an fp16 map; mirror: additionally return the fp16 copy of the fp32 output written in the same
    pass -> (out, out16).  chain=True forces the chain of single-source launches for several fp32 sources."""
    n = len(srcs)
    mask = 0
    for i, t in enumerate(srcs):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError('sources must be contiguous CUDA/HIP tensors')
        if t.dtype == torch.float16:
            mask |= 1 << i
        elif t.dtype != torch.float32:
            raise TypeError(f'source {i}: float32 or float16, got {t.dtype}')
    for p in list(packed_w) + ([packed_w1x1] if packed_w1x1 is not None else []):
        if not p.is_cuda or p.dtype != torch.float16 or not p.is_contiguous():
            raise TypeError('fp16 conv: weight images must be contiguous CUDA float16 tensors (ops.f16_image)')
    h, w = srcs[0].shape[:2]
    dev = srcs[0].device
    out = torch.empty((h, w, 64), device=dev, dtype=torch.float16 if out_f16 else torch.float32)
    out16 = torch.empty((h, w, 64), device=dev, dtype=torch.float16) if mirror else None
    sp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    sc = (ctypes.c_int * n)(*[t.shape[2] for t in srcs])
    wp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in packed_w])
    keep = [(_chk(t, 'arg') if t is not None else None) for t in (bias, gamma, par, residual)]
    if par_flags is not None and (par_flags.dtype != torch.int32 or not par_flags.is_cuda):
        raise TypeError('par_flags: int32 CUDA tensor (ops.par_tile_flags)')
    w1 = ctypes.c_void_p(packed_w1x1.data_ptr()) if packed_w1x1 is not None else None
    _native.check(_native.lib().pnp_conv3x3_f16_maps(n, sp, sc, mask, wp, _ptr(keep[0]), _ptr(keep[1]), w1, _ptr(keep[2]),
                                                     _ptr(par_flags), _ptr(keep[3]), act, _ptr(out), int(bool(out_f16)),
                                                     _ptr(out16), h, w, int(bool(chain)), _ptr(trace), _stream()),
                  'pnp_conv3x3_f16_maps')
    return (out, out16) if mirror else out


@_on_device_of_first_tensor
def mv_warp_nhwc_f16(feat, flow_x, flow_y, interpolation='bilinear'):
    """mv_warp_nhwc writing an fp16 (h,w,c) map: saturating round-to-nearest-even of the fp32 result."""
    feat, flow_x, flow_y = _chk(feat, 'feat'), _chk(flow_x, 'flow_x'), _chk(flow_y, 'flow_y')
    h, w, c = feat.shape
    out = torch.empty((h, w, c), device=feat.device, dtype=torch.float16)
    _native.check(_native.lib().pnp_mv_warp_nhwc_f16out_mode(_ptr(feat), _ptr(flow_x), _ptr(flow_y), _ptr(out), h, w, c,
                                                             _WARP_MODES[interpolation], _stream()), 'pnp_mv_warp_nhwc_f16out_mode')
    return out


@_on_device_of_first_tensor
def wino_image(packed, gamma=None):
    """Winograd F(2x2,3x3) image (65536 floats) of a packed 64 -> 64 direct-conv image (pack_conv3x3), times gamma[co] if given."""
    packed = _chk(packed, 'packed')
    if packed.numel() != 9 * 4096:
        raise ValueError('packed must be a 9-chunk 64-channel image')
    out = torch.empty(int(_native.lib().pnp_wino_image_floats()), device=packed.device, dtype=torch.float32)
    _native.check(_native.lib().pnp_wino_image_from_packed_f32(_ptr(packed), _ptr(_chk(gamma, 'gamma')) if gamma is not None else None,
                                                               _ptr(out), _stream()), 'pnp_wino_image_from_packed_f32')
    # which gain the image carries: conv3x3_wino scales only the BIAS by its `gamma` argument (the conv term's gain lives in the image), so
    # the two must be the same tensor -- checked there when the image still carries this tag
    out._pnp_gamma = None if gamma is None else gamma.detach().clone()
    return out


@_on_device_of_first_tensor
def wino_par_image(packed_w1x1):
    packed_w1x1 = _chk(packed_w1x1, 'packed_w1x1')
    out = torch.empty(int(_native.lib().pnp_wino_par_image_floats()), device=packed_w1x1.device, dtype=torch.float32)
    _native.check(_native.lib().pnp_wino_par_image_from_packed_f32(_ptr(packed_w1x1), _ptr(out), _stream()),
                  'pnp_wino_par_image_from_packed_f32')
    return out


@_on_device_of_first_tensor
def wino_rgb_image(packed_rgb):
    """Winograd image (4096 floats) of the frame's packed chunk (pack_conv3x3(w, cbase=0, csrc=3))."""
    packed_rgb = _chk(packed_rgb, 'packed_rgb')
    out = torch.empty(int(_native.lib().pnp_wino_rgb_image_floats()), device=packed_rgb.device, dtype=torch.float32)
    _native.check(_native.lib().pnp_wino_rgb_image_from_packed_f32(_ptr(packed_rgb), _ptr(out), _stream()),
                  'pnp_wino_rgb_image_from_packed_f32')
    return out


@_on_device_of_first_tensor
def conv3x3_wino_ms(srcs, wino_ws, bias=None, act=0, units=False, out=None):
    """The input conv on conv_wino.hip: srcs = [(h,w,4) frame, (h,w,64) maps ...], wino_ws = [wino_rgb_image(...), wino_image(...) ...];
    the 64-channel sources' images must sit within 4 GiB of each other (slices of ONE tensor do).  out: an (h,w,64) tensor to write
    into (inside wino_tile_rows() only the named tile rows of it are written)."""
    srcs = [_chk(x, 'src') for x in srcs]
    wino_ws = [_chk(x, 'wino_w') for x in wino_ws]
    h, w = srcs[0].shape[:2]
    n = len(srcs)
    if n != len(wino_ws) or srcs[0].shape[2] != 4 or any(x.shape != (h, w, 64) for x in srcs[1:]):
        raise ValueError('srcs must be [(h,w,4), (h,w,64) ...] with one Winograd image each')
    if out is None:
        out = torch.empty((h, w, 64), device=srcs[0].device, dtype=torch.float32)
    elif _chk(out, 'out').shape != (h, w, 64) or not out.is_contiguous():
        raise ValueError('out must be a contiguous (h, w, 64) tensor')
    sp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in srcs])
    wp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in wino_ws])
    fn = _native.lib().pnp_conv3x3_wino_ms_units_f32 if units else _native.lib().pnp_conv3x3_wino_ms_f32
    _native.check(fn(n, sp, wp, _ptr(_chk(bias, 'bias')) if bias is not None else None, int(act), _ptr(out), h, w, _stream()),
                  'pnp_conv3x3_wino_ms_f32')
    return out


@contextlib.contextmanager
def wino_tile_rows(row0, nrows):
    """Inside the block conv3x3_wino / conv3x3_wino_ms (tile kernels) compute the 16-pixel tile rows [row0, row0 + nrows) of the frame
    only (pnp_debug_wino_tile_rows, include/pnpvcve_debug.h): one part of a row-band chain.  Process-wide: a test hook."""
    _native.check(_native.lib().pnp_debug_wino_tile_rows(int(row0), int(nrows)), 'pnp_debug_wino_tile_rows')
    try:
        yield
    finally:
        _native.lib().pnp_debug_wino_tile_rows(0, 0)


@_on_device_of_first_tensor
def conv3x3_wino(x, wino_w, bias=None, gamma=None, wino_w1x1=None, par=None, par_flags=None, residual=None, act=0, trace=None, units=False,
                 out=None):
    """act(gamma * (conv3x3(x; W) + bias) + sum_j par_j * conv1x1_j(x)) + residual on conv_wino.hip; x (h,w,64) NHWC fp32,
    wino_w = wino_image(packed W, gamma) -- the SAME gamma -- and wino_w1x1 = wino_par_image(packed 1x1 images).  units=True: one block
    per 8x8 quadrant unit (the small-frame form, pnp_conv3x3_wino_units_f32; same values).  out: an (h,w,64) tensor to write into (it
    may be `residual` itself, as a block's back half runs; inside wino_tile_rows() only the named tile rows of it are written)."""
    x = _chk(x, 'x')
    h, w, c = x.shape
    if c != 64:
        raise ValueError('x must be (h, w, 64)')
    tag = getattr(wino_w, '_pnp_gamma', 'untagged')              # (set by wino_image; lost by views / copies: then nothing is checked)
    if not isinstance(tag, str) and ((tag is None) != (gamma is None) or (gamma is not None and not torch.equal(tag, gamma))):
        raise ValueError('conv3x3_wino: `gamma` scales only the bias -- the conv term carries the gain wino_image() folded into wino_w; '
                         'pass the SAME gamma tensor to both (or none to both)')
    if out is None:
        out = torch.empty_like(x)
    elif _chk(out, 'out').shape != x.shape or not out.is_contiguous():
        raise ValueError('out must be a contiguous tensor of the shape of x')
    opt = lambda t, n: _ptr(_chk(t, n)) if t is not None else None   # noqa: E731
    if par_flags is not None and (par_flags.dtype != torch.int32 or not par_flags.is_cuda):
        raise ValueError('par_flags must be a CUDA int32 tensor')
    args = (_ptr(x), _ptr(_chk(wino_w, 'wino_w')), opt(bias, 'bias'), opt(gamma, 'gamma'), opt(wino_w1x1, 'wino_w1x1'), opt(par, 'par'),
            ctypes.c_void_p(par_flags.data_ptr()) if par_flags is not None else None, opt(residual, 'residual'), int(act), _ptr(out), h, w)
    if units:
        _native.check(_native.lib().pnp_conv3x3_wino_units_f32(*args, _stream()), 'pnp_conv3x3_wino_units_f32')
    elif trace is None:
        _native.check(_native.lib().pnp_conv3x3_wino_f32(*args, _stream()), 'pnp_conv3x3_wino_f32')
    else:       # include/pnpvcve_debug.h: 16 uint64 per block
        _native.check(_native.lib().pnp_conv3x3_wino_f32_ex(*args, ctypes.c_void_p(trace.data_ptr()), _stream()), 'pnp_conv3x3_wino_f32_ex')
    return out


@_on_device_of_first_tensor
def frames_to_rgb8(frames):
    """(n,3,h,w) fp32 CUDA frames -> (n,h,w,3) uint8 RGB CUDA tensor with tensor2img's arithmetic."""
    frames = _chk(frames, 'frames')
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError('frames must be (n,3,h,w)')
    n, _, h, w = frames.shape
    out = torch.empty((n, h, w, 3), device=frames.device, dtype=torch.uint8)
    _native.check(_native.lib().pnp_frames_to_rgb8(_ptr(frames), ctypes.c_void_p(out.data_ptr()), n, h, w, _stream()),
                  'pnp_frames_to_rgb8')
    return out


@_on_device_of_first_tensor
def frames_from_rgb8(u8):
    """(...,h,w,3) uint8 RGB CUDA frames -> (...,3,h,w) fp32 planes, byte v -> float32(v) / float32(255) (IEEE division; one table in
    the library): what RescaleToZeroOne + HWC->CHW make of a decoded frame, bit for bit.  The inverse layout of frames_to_rgb8."""
    if not isinstance(u8, torch.Tensor) or not u8.is_cuda:
        raise RuntimeError('u8 must be a CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
    if u8.dtype != torch.uint8:
        raise TypeError(f'u8 must be uint8, got {u8.dtype}')
    if u8.dim() < 3 or u8.shape[-1] != 3:
        raise ValueError('u8 must be (...,h,w,3) uint8 RGB')
    u8 = u8.contiguous()
    lead, (h, w) = tuple(u8.shape[:-3]), u8.shape[-3:-1]
    n = 1
    for d in lead:
        n *= int(d)
    out = torch.empty(lead + (3, h, w), device=u8.device, dtype=torch.float32)
    if n:
        _native.check(_native.lib().pnp_frames_from_rgb8(ctypes.c_void_p(u8.data_ptr()), _ptr(out), n, h, w, _stream()),
                      'pnp_frames_from_rgb8')
    return out


def _metric_frames(t, name):
    """One input of a device metric: fp32 (...,c,h,w) planes or uint8 (...,h,w,3) RGB bytes -> (contiguous tensor, PNP_FRAMES_*
    format, leading shape, c, h, w)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
    if t.dtype == torch.uint8:
        if t.dim() < 3 or t.shape[-1] != 3:
            raise ValueError(f'{name}: uint8 frames must be (...,h,w,3) RGB')
        h, w = t.shape[-3:-1]
        return t.contiguous(), _native.FRAMES_U8_HWC, tuple(t.shape[:-3]), 3, int(h), int(w)
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32 planes or uint8 RGB frames, got {t.dtype}')
    if t.dim() < 3:
        raise ValueError(f'{name}: fp32 frames must be (...,c,h,w)')
    c, h, w = t.shape[-3:]
    return t.contiguous(), _native.FRAMES_F32_NCHW, tuple(t.shape[:-3]), int(c), int(h), int(w)


def _metric_color(convert_to):
    """convert_to None | 'y' / 'Y' -> PNP_COLOR_*"""
    if isinstance(convert_to, str) and convert_to.lower() == 'y':
        return _native.COLOR_Y
    if convert_to is None:
        return _native.COLOR_NONE
    raise ValueError('Wrong color model. Supported values are "Y" and None.')


def _metric_pair(a, b, convert_to):
    """-> (a, a_format, b, b_format, PNP_COLOR_*, leading shape, frames, c, h, w) of two clips that show the same frames"""
    color = _metric_color(convert_to)
    a, fa, lead_a, ca, ha, wa = _metric_frames(a, 'a')
    b, fb, lead_b, cb, hb, wb = _metric_frames(b, 'b')
    if (lead_a, ca, ha, wa) != (lead_b, cb, hb, wb):
        raise AssertionError(f'Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.')
    if a.device != b.device:
        raise RuntimeError('a and b must be on the same device')
    frames = 1
    for d in lead_a:
        frames *= d
    return a, fa, b, fb, color, lead_a, frames, ca, ha, wa


@_on_device_of_first_tensor
def luma_frames(x):
    """fp32 (...,3,h,w) planes (rounded to bytes as tensor2img does) or uint8 (...,h,w,3) RGB frames -> fp32 (...,h,w) CUDA tensor of
    the reference's Y, mmcv.bgr2ycbcr(img / 255., y_only=True) * 255. of the uint8 BGR image, bit for bit (pnp_luma_from_frames)."""
    x, fmt, lead, c, h, w = _metric_frames(x, 'x')
    if c != 3:
        raise ValueError('x must have 3 channels')
    frames = 1
    for d in lead:
        frames *= d
    out = torch.empty(lead + (h, w), device=x.device, dtype=torch.float32)
    if frames:
        _native.check(_native.lib().pnp_luma_from_frames(_ptr(x), fmt, _ptr(out), frames, h, w, _stream()), 'pnp_luma_from_frames')
    return out


@_on_device_of_first_tensor
def psnr_frames(a, b, crop_border=0, convert_to=None):
    """Per-frame PSNR with the reference's definition (uint8-rounded frames), computed on the GPU.
    a, b, each on its own: fp32 (..., c, h, w) planes or uint8 (..., h, w, 3) RGB frames, any leading dims; convert_to None | 'y' / 'Y'
    (the Y of the BGR image, metrics.py:201-203).  Returns a float64 CPU tensor of the leading shape."""
    a, fa, b, fb, color, lead, frames, c, h, w = _metric_pair(a, b, convert_to)
    crop_border = int(crop_border)
    L = _native.lib()
    if color == _native.COLOR_Y:
        nb = int(L.pnp_psnr_luma_blocks(h, w, crop_border))
        stat = torch.empty((frames, max(nb, 1)), dtype=torch.float64, device=a.device)
    else:
        stat = torch.empty(frames, dtype=torch.int64, device=a.device)
    _native.check(L.pnp_psnr_stat_io(_ptr(a), fa, _ptr(b), fb, color, _ptr(stat), frames, c, h, w, crop_border, _stream()),
                  'pnp_psnr_stat_io')
    if color == _native.COLOR_Y:
        n = (h - 2 * crop_border) * (w - 2 * crop_border)
        sse = torch.from_numpy(stat.cpu().numpy().cumsum(axis=1)[:, -1].copy())      # a frame's partials added in index order
    else:
        n = c * (h - 2 * crop_border) * (w - 2 * crop_border)
        sse = stat.cpu().double()
    mse = sse / n
    out = 20.0 * torch.log10(255.0 / mse.sqrt())
    out[mse == 0] = float('inf')
    return out.reshape(lead)


@_on_device_of_first_tensor
def rasterise_side_info(records, rec_frame, slices, h, w):
    """Decoder MV records -> (mvs (T,4,h,w), partitions (T,3,h,w)) on the GPU
    (LoadImageFromFileList_ipb.__call__, loading_ipb.py:328-369, + RescaleToZeroOne + FramesToTensor).
    records (R,10) fp32 CUDA, rec_frame (R,) int32 CUDA, slices: sequence of 'I'/'P'/'B' (or ord values)."""
    records = _chk(records, 'records')
    if not rec_frame.is_cuda or rec_frame.dtype != torch.int32:
        raise TypeError('rec_frame must be a CUDA int32 tensor')
    rec_frame = rec_frame.contiguous()
    t = len(slices)
    sl = (ctypes.c_float * t)(*[float(ord(s) if isinstance(s, str) else s) for s in slices])
    dev = records.device
    mvs = torch.empty((t, 4, h, w), device=dev, dtype=torch.float32)
    par = torch.empty((t, 3, h, w), device=dev, dtype=torch.float32)
    scratch = torch.empty((t, 2, h, w), device=dev, dtype=torch.int32)
    _native.check(_native.lib().pnp_rasterise_side_info_f32(_ptr(records), _ptr(rec_frame), records.shape[0], sl, t, h, w,
                                                            _ptr(mvs), _ptr(par), _ptr(scratch), _stream()),
                  'pnp_rasterise_side_info_f32')
    return mvs, par


@_on_device_of_first_tensor
def modulated_deform_conv_nhwc(x, offset, mask_logits, weight, bias, flow=None, fp16=False):
    """mmcv.ops.modulated_deform_conv2d(x, offset, sigmoid(mask_logits), weight, bias, 1, 1, 1, 1, 16) for the
    hot path's shapes.  x (h,w,64) pixel-major; offset (288,h,w) and mask_logits (144,h,w) in mmcv's channel
    order; weight (64,64,3,3); optional flow (2,h,w) = (dx,dy) added to every offset.  Returns (h,w,64).
    fp16=True: fp16 MFMA operands (what PNP_PREC_F16 runs), fp32 accumulation."""
    x = _chk(x, 'x')
    h, w, _ = x.shape
    L = _native.lib()
    ref = torch.tensor([L.pnp_dcn_ref_channel(c) for c in range(448)], device=x.device)
    src = torch.cat([_chk(offset, 'offset'), _chk(mask_logits, 'mask')], 0)             # (432,h,w)
    om = torch.zeros((448, h, w), device=x.device, dtype=torch.float32)
    om[ref >= 0] = src[ref[ref >= 0]]
    om = om.permute(1, 2, 0).contiguous()
    wp = pack_conv3x3(weight)
    out = torch.empty_like(x)
    fx = _chk(flow[0], 'flow') if flow is not None else None
    fy = _chk(flow[1], 'flow') if flow is not None else None
    if fp16:
        w16 = torch.empty(9 * 4096, device=x.device, dtype=torch.float16)
        _native.check(L.pnp_dcn_f16_image_from_f32(_ptr(wp), ctypes.c_void_p(w16.data_ptr()), _stream()),
                      'pnp_dcn_f16_image_from_f32')
        _native.check(L.pnp_dcn_nhwc_f16(_ptr(x), _ptr(om), _ptr(fx), _ptr(fy), ctypes.c_void_p(w16.data_ptr()),
                                         _ptr(_chk(bias, 'bias')), _ptr(out), h, w, _stream()), 'pnp_dcn_nhwc_f16')
        return out
    _native.check(L.pnp_dcn_nhwc_f32(_ptr(x), _ptr(om), _ptr(fx), _ptr(fy), _ptr(wp), _ptr(_chk(bias, 'bias')), _ptr(out),
                                     h, w, _stream()), 'pnp_dcn_nhwc_f32')
    return out


@_on_device_of_first_tensor
def ssim_frames(a, b, crop_border=0, convert_to=None):
    """Per-frame SSIM with the reference's definition (metrics.py:266-355), computed on the GPU in fp64.
    a, b, each on its own: fp32 (..., c, h, w) planes or uint8 (..., h, w, 3) RGB frames; convert_to None | 'y' / 'Y' (one channel, the
    fp32 Y of the BGR image, metrics.py:338-343).  Returns a float64 CPU tensor of the leading shape."""
    a, fa, b, fb, color, lead, frames, c, h, w = _metric_pair(a, b, convert_to)
    crop_border = int(crop_border)
    L = _native.lib()
    nb = int(L.pnp_ssim_blocks(h, w, crop_border))
    if nb < 1:
        raise ValueError('frames are smaller than the 11x11 SSIM window')
    planes = 1 if color == _native.COLOR_Y else c
    part = torch.empty((frames * planes, nb), dtype=torch.float64, device=a.device)
    _native.check(L.pnp_ssim_partials_io(_ptr(a), fa, _ptr(b), fb, color, _ptr(part), frames, c, h, w, crop_border, _stream()),
                  'pnp_ssim_partials_io')
    n = (h - 2 * crop_border - 10) * (w - 2 * crop_border - 10)
    per_plane = (part.sum(dim=1) / n).reshape(frames, planes)
    if crop_border != 0 and planes == 3:
        # reference quirk (metrics.py:343-350, see pnp_vcve_amd/metrics.py): with a crop only channel 0 of the BGR image,
        # i.e. the B plane of these RGB frames, enters the SSIM mean
        per_plane = per_plane[:, 2:3]
    return per_plane.mean(dim=1).cpu().reshape(lead)


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003, as published (sum 1.0001)


def _msssim_plan(h, w, crop):
    """one plane of h x w samples cropped by `crop` -> (blocks per level, valid-map sizes per level), or None when it cannot be
    scored (pnp_msssim_blocks / pnp_msssim_level_dims: a cropped plane below 176 x 176)"""
    L = _native.lib()
    blocks = [int(L.pnp_msssim_blocks(h, w, crop, s)) for s in range(5)]
    if min(blocks) < 1:
        return None
    sizes = []
    for s in range(5):
        r, c = ctypes.c_int(0), ctypes.c_int(0)
        _native.check(L.pnp_msssim_level_dims(h, w, crop, s, ctypes.byref(r), ctypes.byref(c)), 'pnp_msssim_level_dims')
        sizes.append((r.value - 10) * (c.value - 10))
    return blocks, sizes


def _msssim_scales(part, blocks, sizes):
    """partials (units, sum(blocks), 2) of planes of one plan -> (units, 5, 2) float64 CPU: a level's partials added in index order,
    divided by the level's valid-map size: the raw (CS_s, S_s)"""
    import numpy as np
    p = part.cpu().numpy()
    out = np.empty((p.shape[0], 5, 2), np.float64)
    off = 0
    for s in range(5):
        out[:, s] = p[:, off:off + blocks[s]].cumsum(axis=1)[:, -1] / sizes[s]
        off += blocks[s]
    return torch.from_numpy(out)


def _msssim_value(scales):
    """(..., 5, 2) raw (CS_s, S_s) -> (...): prod_{s<4} max(CS_s, 0)^w_s * max(S_4, 0)^w_4 in float64"""
    f = torch.cat([scales[..., :4, 0], scales[..., 4:, 1]], dim=-1).clamp(min=0.0)
    return (f ** torch.tensor(MSSSIM_WEIGHTS, dtype=torch.float64)).prod(dim=-1)


def _msssim_too_small(what):
    n = int(_native.lib().pnp_msssim_min_size())
    return ValueError(f'MS-SSIM needs {n} x {n} samples of {what} after the crop: level 4 of the pyramid must hold one 11 x 11 window')


@_on_device_of_first_tensor
def msssim_frames(a, b, crop_border=0, convert_to=None, scales=False):
    """Per-frame multi-scale SSIM (include/pnpvcve.h, pnp_msssim_partials_io: five scales, ssim_frames' window at each, 2 x 2 mean
    pyramid), computed on the GPU in fp64.  Inputs as ssim_frames: a, b, each on its own, fp32 (..., c, h, w) planes or uint8
    (..., h, w, 3) RGB frames; convert_to None (the mean over the channels' values, with or without a crop) | 'y' / 'Y' (one plane,
    the fp32 Y).  Returns a float64 CPU tensor of the leading shape; with scales=True also the raw, unclamped per-level means, a
    float64 CPU tensor lead + (planes, 5, 2) = (CS_s, S_s).  The cropped frames must be at least 176 x 176."""
    a, fa, b, fb, color, lead, frames, c, h, w = _metric_pair(a, b, convert_to)
    crop_border = int(crop_border)
    if crop_border < 0 or 2 * crop_border >= h or 2 * crop_border >= w:
        raise ValueError(f'a crop of {crop_border} leaves nothing of {h} x {w} frames')
    plan = _msssim_plan(h, w, crop_border)
    if plan is None:
        raise _msssim_too_small('every frame')
    blocks, sizes = plan
    L = _native.lib()
    planes = 1 if color == _native.COLOR_Y else c
    if not frames:
        res, sc = torch.empty(lead, dtype=torch.float64), torch.empty(lead + (planes, 5, 2), dtype=torch.float64)
        return (res, sc) if scales else res
    part = torch.empty((frames * planes, sum(blocks), 2), dtype=torch.float64, device=a.device)
    ws = torch.empty(int(L.pnp_msssim_workspace_bytes(frames, planes, h, w, crop_border)) // 4, dtype=torch.float32, device=a.device)
    _native.check(L.pnp_msssim_partials_io(_ptr(a), fa, _ptr(b), fb, color, _ptr(part), _ptr(ws), frames, c, h, w, crop_border, _stream()),
                  'pnp_msssim_partials_io')
    sc = _msssim_scales(part, blocks, sizes).reshape(frames, planes, 5, 2)
    res = _msssim_value(sc).mean(dim=1).reshape(lead)
    return (res, sc.reshape(lead + (planes, 5, 2))) if scales else res


@_on_device_of_first_tensor
def bae_block(x, w2_packed, b2, gamma, w1x1_packed, par, w1_packed, b1):
    """One BAE block (ResidualBlockNoBNDynamic_drt.forward, sr_backbone_utils.py:305-313,329), pnp_bae_block_f32.
    x (h,w,64) pixel-major; w2_packed = pack_conv3x3(experts, ew=attention); w1_packed = pack_conv3x3(conv1.weight);
    w1x1_packed = pack_conv1x1([...]) and par (3,h,w), or both None; gamma (64,) or None."""
    x = _chk(x, 'x')
    h, w, _ = x.shape
    keep = [(_chk(t, 'arg') if t is not None else None) for t in (w2_packed, b2, gamma, w1x1_packed, par, w1_packed, b1)]
    scratch = torch.empty_like(x)
    out = torch.empty_like(x)
    _native.check(_native.lib().pnp_bae_block_f32(_ptr(x), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]),
                                                  _ptr(keep[4]), _ptr(keep[5]), _ptr(keep[6]), _ptr(scratch), _ptr(out),
                                                  h, w, _stream()), 'pnp_bae_block_f32')
    return out


@_on_device_of_first_tensor
def pack_pixel_shuffle(weight, bias):
    """PixelShufflePack.upsample_conv (256,64,3,3) + bias (256) -> packed image for pixel_shuffle_conv."""
    weight, bias = _chk(weight, 'weight'), _chk(bias, 'bias')
    if tuple(weight.shape) != (256, 64, 3, 3) or tuple(bias.shape) != (256,):
        raise ValueError('pixel-shuffle conv: weight (256,64,3,3), bias (256,)')
    L = _native.lib()
    dst = torch.empty(int(L.pnp_packed_pixel_shuffle_floats()), device=weight.device, dtype=torch.float32)
    _native.check(L.pnp_pack_pixel_shuffle_f32(_ptr(weight), _ptr(bias), _ptr(dst), _stream()), 'pnp_pack_pixel_shuffle_f32')
    return dst


@_on_device_of_first_tensor
def pixel_shuffle_conv(x, packed, act=0):
    """PixelShufflePack.forward (upsample.py:40-51): x (h,w,64) -> (2h,2w,64); act 0 none / 1 relu / 2 leaky-relu(0.1)."""
    x, packed = _chk(x, 'x'), _chk(packed, 'packed')
    h, w, _ = x.shape
    out = torch.empty((2 * h, 2 * w, 64), device=x.device, dtype=torch.float32)
    _native.check(_native.lib().pnp_pixel_shuffle_conv_f32(_ptr(x), _ptr(packed), int(act), _ptr(out), h, w, _stream()),
                  'pnp_pixel_shuffle_conv_f32')
    return out


def _head_map(t, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
    if t.dtype not in (torch.float32, torch.float16):
        raise TypeError(f'{name}: float32 or float16, got {t.dtype}')
    if t.dim() != 3 or t.shape[2] != 64 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f'{name}: a pixel-major (h,w,64) map' + (f' of shape {tuple(shape)}' if shape is not None else ''))
    return int(t.dtype == torch.float16)


@_on_device_of_first_tensor
def head_pixel_shuffle_conv(x, packed, act=0, route='auto', twin=None, out=None, out_f16=False, tile_queue=None):
    """The head's pixel-shuffle conv with an explicit kernel route (include/pnpvcve_debug.h, pnp_debug_pixel_shuffle_conv).
    x (h,w,64) float32 or float16; packed = pack_pixel_shuffle(); twin = f16_image(packed[:4 * 36864]) or f16x3_image of the same
    (told apart by size), or None; route 'auto' | 'f32' | 'f16' | 'f16x3'.  out: a (2h,2w,64) float32 / float16 tensor to write
    into, or None: a new one (float16 when out_f16).  A route the arguments are not eligible for raises (pnp error 1002)."""
    x16 = _head_map(x, 'x')
    packed = _chk(packed, 'packed')
    h, w, _ = x.shape
    kind = 0
    if twin is not None:
        if not twin.is_cuda or twin.dtype != torch.float16 or not twin.is_contiguous() or twin.numel() not in (4 * 36864, 8 * 36864):
            raise TypeError('twin: ops.f16_image or ops.f16x3_image of the four sub-pixel images')
        kind = 1 if twin.numel() == 4 * 36864 else 2
    if out is None:
        out = torch.empty((2 * h, 2 * w, 64), device=x.device, dtype=torch.float16 if out_f16 else torch.float32)
    o16 = _head_map(out, 'out', (2 * h, 2 * w, 64))
    if tile_queue is not None and (tile_queue.dtype != torch.int32 or tile_queue.numel() < 16 or not tile_queue.is_cuda):
        raise TypeError('tile_queue: 16 int32 on the device')
    _native.check(_native.lib().pnp_debug_pixel_shuffle_conv(_ptr(x), x16, _ptr(packed), _ptr(twin), kind, int(act), _ptr(out), o16, h, w,
                                                             _native.HEAD_ROUTES[route], _ptr(tile_queue), _stream()),
                  'pnp_debug_pixel_shuffle_conv')
    return out


@_on_device_of_first_tensor
def pack_conv_last(weight, bias):
    """conv_last.weight (3,64,3,3) + bias (3,) -> the buffer head_conv_last reads: every layout pnp_generator_pack makes of them."""
    weight, bias = _chk(weight, 'weight'), _chk(bias, 'bias')
    if tuple(weight.shape) != (3, 64, 3, 3) or tuple(bias.shape) != (3,):
        raise ValueError('conv_last: weight (3,64,3,3), bias (3,)')
    L = _native.lib()
    dst = torch.empty(int(L.pnp_debug_conv_last_packed_floats()), device=weight.device, dtype=torch.float32)
    _native.check(L.pnp_debug_pack_conv_last(_ptr(weight), _ptr(bias), _ptr(dst), _stream()), 'pnp_debug_pack_conv_last')
    return dst


@_on_device_of_first_tensor
def head_conv_last(src, packed, frame, out_mode=2, act=0, route='auto', precision=0, frame_form=None, out=True, out_u8=False):
    """conv_last + the frame with an explicit kernel route (include/pnpvcve_debug.h, pnp_debug_conv_last) -> (out, out_u8).
    src (H,W,64) float32 or float16; packed = pack_conv_last(); out_mode 2: the frame is H x W, 3: H/4 x W/4 (bilinear x4).
    frame_form 'planes' (3,h,w) float32 | 'u8' (h,w,3) uint8 | 'rgb0' (h,w,4) float32; None: by dtype, planes or u8.
    route 'auto' (at `precision` 0 fp32 / 1 fp16 / 2 split fp16) | 'valu' | 'f32' | 'f16'.  out / out_u8: True (a new tensor), a
    tensor to write into ((3,H,W) float32 / (H,W,3) uint8), or False (not written; None is returned in its place)."""
    s16 = _head_map(src, 'src')
    packed = _chk(packed, 'packed')
    H, W, _ = src.shape
    if frame_form is None:
        frame_form = 'u8' if frame.dtype == torch.uint8 else 'planes'
    fh, fw = (H // 4, W // 4) if out_mode == 3 else (H, W)
    want = {'planes': ((3, fh, fw), torch.float32), 'u8': ((fh, fw, 3), torch.uint8), 'rgb0': ((fh, fw, 4), torch.float32)}[frame_form]
    if not frame.is_cuda or not frame.is_contiguous() or tuple(frame.shape) != want[0] or frame.dtype != want[1]:
        raise ValueError(f'frame ({frame_form}): a contiguous CUDA {want[1]} tensor of shape {want[0]}, got {tuple(frame.shape)} {frame.dtype}')
    form = {'planes': _native.HEAD_FRAME_PLANES, 'u8': _native.HEAD_FRAME_U8, 'rgb0': _native.HEAD_FRAME_RGB0}[frame_form]
    if out is True:
        out = torch.empty((3, H, W), device=src.device, dtype=torch.float32)
    if out_u8 is True:
        out_u8 = torch.empty((H, W, 3), device=src.device, dtype=torch.uint8)
    out = None if out is False else out
    out_u8 = None if out_u8 is False else out_u8
    for t, shp, dt, nm in ((out, (3, H, W), torch.float32, 'out'), (out_u8, (H, W, 3), torch.uint8, 'out_u8')):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shp or t.dtype != dt):
            raise ValueError(f'{nm}: a contiguous CUDA {dt} tensor of shape {shp}')
    _native.check(_native.lib().pnp_debug_conv_last(_ptr(src), s16, _ptr(packed), int(precision), int(act), int(out_mode), _ptr(frame), form,
                                                    _ptr(out), _ptr(out_u8), H, W, _native.HEAD_ROUTES[route], _stream()),
                  'pnp_debug_conv_last')
    return out, out_u8


# ---------------------------------------------------------------- Y'CbCr 4:2:0 frames (include/pnpvcve.h states the arithmetic)
# 8-bit planes (Yuv420Frames: bytes) and 10 / 12-bit planes (Yuv420Frames16: 16-bit words) share every helper below; the sample's size
# is the tensors' element_size(), and a function named for one sample size refuses frames of the other.
_Yuv420Base = collections.namedtuple('Yuv420Frames', ['y', 'cb', 'cr'])
_Yuv420Base16 = collections.namedtuple('Yuv420Frames16', ['y', 'cb', 'cr', 'bit_depth', 'msb_aligned'], defaults=(10, False))


class Yuv420Frames(_Yuv420Base):
    """8-bit 4:2:0 frames as three uint8 CUDA VIEWS of wherever the decoder wrote them: y (n,t,h,w), cb and cr (n,t,h/2,w/2) (or
    without the batch dimension: one clip).  Pitches, the chroma step and the frame strides are read from the tensors' strides: the
    last-dimension stride is 1 for y and 1 (I420) or 2 (NV12 / NV21: cb and cr one byte apart in one buffer) for chroma.  Nothing is
    copied; yuv420_views builds the views of a packed buffer."""
    __slots__ = ()


class Yuv420Frames16(_Yuv420Base16):
    """10 / 12-bit 4:2:0 frames as three CUDA VIEWS of 16-bit words (torch.int16, or torch.uint16 where torch has it: the same bits)
    of wherever the decoder wrote them: y (n,t,h,w), cb and cr (n,t,h/2,w/2), or without the batch dimension.  bit_depth 10 | 12;
    msb_aligned: the value sits in the high bits of the word (P010 / P012) instead of the low ones (yuv420p10le / yuv420p12le).
    Strides are in samples: the last-dimension stride is 1 for y and 1 (planar) or 2 (interleaved: cb and cr one sample apart in one
    buffer) for chroma.  Nothing is copied; yuv420p16_views builds the views of a packed buffer."""
    __slots__ = ()


# 4:2:2 and 4:4:4 frames (include/pnpvcve.h, "Chroma formats"): siblings of the 4:2:0 classes, not subclasses -- the *_yuv420*
# functions keep refusing them -- with chroma planes (n,t,h,w/2) and (n,t,h,w).  The format-generic functions (yuv_views, empty_yuv,
# frames_from_yuv, frames_to_yuv, pack_lr_yuv, psnr_yuv, ssim_yuv) and generator.forward take every class.
class Yuv422Frames(collections.namedtuple('Yuv422Frames', ['y', 'cb', 'cr'])):
    """8-bit 4:2:2 frames: Yuv420Frames' rules with cb and cr (n,t,h,w/2) (yuv422p: last stride 1; NV16: 2, one byte apart)"""
    __slots__ = ()


class Yuv444Frames(collections.namedtuple('Yuv444Frames', ['y', 'cb', 'cr'])):
    """8-bit 4:4:4 frames: Yuv420Frames' rules with cb and cr (n,t,h,w) (yuv444p: last stride 1; NV24: 2, one byte apart)"""
    __slots__ = ()


class Yuv422Frames16(collections.namedtuple('Yuv422Frames16', ['y', 'cb', 'cr', 'bit_depth', 'msb_aligned'], defaults=(10, False))):
    """10 / 12-bit 4:2:2 frames: Yuv420Frames16's rules with cb and cr (n,t,h,w/2) (yuv422p10le / yuv422p12le, P210 / P212)"""
    __slots__ = ()


class Yuv444Frames16(collections.namedtuple('Yuv444Frames16', ['y', 'cb', 'cr', 'bit_depth', 'msb_aligned'], defaults=(10, False))):
    """10 / 12-bit 4:4:4 frames: Yuv420Frames16's rules with cb and cr (n,t,h,w) (yuv444p10le / yuv444p12le, P410 / P412)"""
    __slots__ = ()


YUV_LAYOUTS = ('nv12', 'nv21', 'i420')
# name -> (the 8-bit layout with the same plane order, bit depth, msb_aligned)
YUV16_LAYOUTS = {'p010': ('nv12', 10, True), 'p012': ('nv12', 12, True), 'yuv420p10le': ('i420', 10, False), 'yuv420p12le': ('i420', 12, False)}
_WORD_DTYPES = tuple(d for d in (torch.int16, getattr(torch, 'uint16', None)) if d is not None)
YUV_FORMATS = tuple(sorted(_native.YUV_FORMAT, key=_native.YUV_FORMAT.get))      # '420', '422', '444': the chroma formats in the order of their codes
_YUV_CLASSES = {'420': (Yuv420Frames, Yuv420Frames16), '422': (Yuv422Frames, Yuv422Frames16), '444': (Yuv444Frames, Yuv444Frames16)}
_YUV8_CLASSES = tuple(c[0] for c in _YUV_CLASSES.values())
_YUV16_CLASSES = tuple(c[1] for c in _YUV_CLASSES.values())
# The layouts of the 4:2:2 and 4:4:4 formats by ffmpeg's names: name -> (format, the 4:2:0 layout with the same plane order, bit depth,
# msb_aligned).  Their order here is the index a custom op's `layout` integer carries, offset by _FORMAT_LAYOUT0.
YUV_FORMAT_LAYOUTS = {
    'yuv422p': ('422', 'i420', 8, False), 'nv16': ('422', 'nv12', 8, False), 'yuv444p': ('444', 'i420', 8, False), 'nv24': ('444', 'nv12', 8, False),
    'yuv422p10le': ('422', 'i420', 10, False), 'yuv422p12le': ('422', 'i420', 12, False), 'yuv444p10le': ('444', 'i420', 10, False),
    'yuv444p12le': ('444', 'i420', 12, False), 'p210': ('422', 'nv12', 10, True), 'p212': ('422', 'nv12', 12, True),
    'p410': ('444', 'nv12', 10, True), 'p412': ('444', 'nv12', 12, True)}
_FORMAT_LAYOUT0 = 16


def is_yuv(frames):
    """frames are Y'CbCr planes of any chroma format and either sample size"""
    return isinstance(frames, _YUV8_CLASSES + _YUV16_CLASSES)


def yuv_format(frames):
    """the chroma format of Y'CbCr frames: '420' | '422' | '444'"""
    for fmt, classes in _YUV_CLASSES.items():
        if isinstance(frames, classes):
            return fmt
    raise TypeError(f'not Y\'CbCr frames: {type(frames).__name__}')


def yuv_layout(layout):
    """a layout name of any format -> (format, the 4:2:0 layout with the same plane order, bit depth, msb_aligned)"""
    if isinstance(layout, str):
        if layout in YUV_FORMAT_LAYOUTS:
            return YUV_FORMAT_LAYOUTS[layout]
        if layout in YUV_LAYOUTS:
            return '420', layout, 8, False
        if layout in YUV16_LAYOUTS:
            return ('420',) + tuple(YUV16_LAYOUTS[layout])
    raise ValueError(f'layout must be one of {YUV_LAYOUTS + tuple(sorted(YUV16_LAYOUTS)) + tuple(YUV_FORMAT_LAYOUTS)}, got {layout!r}')


def _yuv_layout_index(layout):
    """the integer a custom op's `layout` argument carries (-1: none): the 4:2:0 layouts keep the index of their own list"""
    if layout is None:
        return -1
    if layout in YUV_FORMAT_LAYOUTS:
        return _FORMAT_LAYOUT0 + list(YUV_FORMAT_LAYOUTS).index(layout)
    return YUV_LAYOUTS.index(layout) if layout in YUV_LAYOUTS else sorted(YUV16_LAYOUTS).index(layout)


def _yuv_layout_of_index(i, sixteen):
    if i < 0:
        return None
    if i >= _FORMAT_LAYOUT0:
        return list(YUV_FORMAT_LAYOUTS)[i - _FORMAT_LAYOUT0]
    return sorted(YUV16_LAYOUTS)[i] if sixteen else YUV_LAYOUTS[i]


def _yuv_standard(standard):
    if isinstance(standard, str):
        if standard not in _native.YUV_STANDARDS:
            raise ValueError(f'yuv_standard must be one of {sorted(_native.YUV_STANDARDS)}, got {standard!r}')
        return _native.YUV_STANDARDS[standard]
    if int(standard) not in _native.YUV_STANDARDS.values():
        raise ValueError(f'yuv_standard must be one of {sorted(_native.YUV_STANDARDS)} or 0..3, got {standard!r}')
    return int(standard)


YUV_CHROMA = tuple(sorted(_native.YUV_CHROMA, key=_native.YUV_CHROMA.get))      # the chroma modes by name, in the order of their codes


def _yuv_code(standard, chroma='replicate', format='420'):
    """PNP_YUV_CODE3(standard, chroma, format), what every Y'CbCr entry of the library takes as yuv_standard: the standard (a name or
    0..3) in bits 0..7, the chroma mode (a name of YUV_CHROMA) in bits 8..11, the chroma format (a name of YUV_FORMATS) in bits
    12..13; 'replicate' and '420' leave the bare standard"""
    if not isinstance(chroma, str) or chroma not in _native.YUV_CHROMA:
        raise ValueError(f'chroma must be one of {YUV_CHROMA}, got {chroma!r}')
    if not isinstance(format, str) or format not in _native.YUV_FORMAT:
        raise ValueError(f'format must be one of {YUV_FORMATS}, got {format!r}')
    return _yuv_standard(standard) | _native.YUV_CHROMA[chroma] << 8 | _native.YUV_FORMAT[format] << 12


def _yuv_code_split(code):
    """a code of _yuv_code (as a custom op's `standard` integer carries it) -> (standard 0..3, chroma name)"""
    code = int(code)
    if code < 0 or code >> 8 >= len(YUV_CHROMA):
        raise ValueError(f'not a code of a yuv_standard and a chroma mode: {code!r}')
    return _yuv_standard(code & 255), YUV_CHROMA[code >> 8]


def _yuv_code_split3(code):
    """a code of _yuv_code with its format -> (standard 0..3, chroma name, format name)"""
    code = int(code)
    if code < 0 or code >> 12 >= len(YUV_FORMATS):
        raise ValueError(f'not a code of a yuv_standard, a chroma mode and a chroma format: {code!r}')
    return _yuv_code_split(code & 0xfff) + (YUV_FORMATS[code >> 12],)


def _yuv16_layout(layout):
    """a layout name of YUV16_LAYOUTS or ('nv12' | 'nv21' | 'i420', bit_depth, msb_aligned) -> (order, bit_depth, msb_aligned)"""
    if isinstance(layout, str):
        if layout not in YUV16_LAYOUTS:
            raise ValueError(f'layout must be one of {sorted(YUV16_LAYOUTS)} or (order, bit_depth, msb_aligned), got {layout!r}')
        return YUV16_LAYOUTS[layout]
    if not isinstance(layout, (tuple, list)) or len(layout) != 3 or layout[0] not in YUV_LAYOUTS:
        raise ValueError(f'layout must be one of {sorted(YUV16_LAYOUTS)} or ({YUV_LAYOUTS}, bit_depth, msb_aligned), got {layout!r}')
    return layout[0], _bit_depth(layout[1]), bool(layout[2])


def _bit_depth(d):
    if isinstance(d, bool) or d not in (10, 12):
        raise ValueError(f'bit_depth must be 10 or 12, got {d!r}')
    return int(d)


def _yuv_expect(frames, what, cls=None):
    """TypeError unless frames are `cls` (Yuv420Frames | Yuv420Frames16; None: either, anything else is told what 8-bit frames are)
    -> frames are 16-bit"""
    if cls is None and is_yuv(frames):          # (frames of any chroma format: the format-generic callers)
        return isinstance(frames, _YUV16_CLASSES)
    if cls is not None and cls not in (Yuv420Frames, Yuv420Frames16):      # a class of another format, asked for by name
        if not isinstance(frames, cls):
            raise TypeError(f'{what} must be ops.{cls.__name__}({", ".join(cls._fields)})')
        return cls in _YUV16_CLASSES
    if cls is Yuv420Frames16 or (cls is None and isinstance(frames, Yuv420Frames16)):
        if not isinstance(frames, Yuv420Frames16):
            raise TypeError(f'{what} must be ops.Yuv420Frames16(y, cb, cr, bit_depth, msb_aligned)')
        return True
    if not isinstance(frames, Yuv420Frames):
        raise TypeError(f'{what} must be ops.Yuv420Frames(y, cb, cr)')
    return False


def _yuv_entry(name, frames):
    """the C entry `name` for the frames' sample size"""
    return name + ('p16' if isinstance(frames, _YUV16_CLASSES) else '')


def _yuv_each_clip(name, frames, clips, t, call):
    """The plane metrics' call loop: the C entry `name` for the frames' sample size, called once per clip of `clips` (descriptor pairs
    or triples; nothing is called for clips of no frames) on the frames' device: call(entry, i, *descriptors by reference) -> status.
    A generator: it yields i after clip i's call was checked, for callers that read a per-clip buffer before the next call."""
    entry = getattr(_native.lib(), _yuv_entry(name, frames))
    with torch.cuda.device(frames.y.device):
        for i, descs in enumerate(clips):
            if t:
                _native.check(call(entry, i, *(ctypes.byref(d) for d in descs)), _yuv_entry(name, frames))
                yield i


def _yuv_all_clips(*args):
    """_yuv_each_clip for callers whose calls write into one tensor of all clips"""
    for _ in _yuv_each_clip(*args):
        pass


def _yuv_views_format(buf, h, w, fmt, order, tail=()):
    """yuv420_views / yuv420p16_views / yuv_views: a packed buffer (..., h + 2 (h / sy) / sx, pitch) -> views of the format's frame
    class; order 'nv12' | 'nv21' | 'i420' (the plane order); tail () -> the class of a uint8 buffer, (bit_depth, msb_aligned) -> the
    class of 16-bit words.  The format is its factors (sx, sy): the chroma planes are (h / sy) x (w / sx)"""
    cls = _YUV_CLASSES[fmt][1 if tail else 0]
    sx, sy = _native.YUV_FACTORS[fmt]
    _yuv_size_check(fmt, h, w)
    if tail and (not isinstance(buf, torch.Tensor) or buf.dtype not in _WORD_DTYPES):
        raise TypeError(f'buf must be a tensor of 16-bit words (torch.int16 / torch.uint16), got {getattr(buf, "dtype", type(buf))}')
    if not tail and buf.dtype != torch.uint8:
        raise TypeError(f'buf must be uint8, got {buf.dtype}')
    ch = h // sy
    rows = h + 2 * ch // sx         # Y, then two chroma planes of h / sy rows, w / sx samples each
    if buf.dim() >= 2 and buf.shape[-2] == rows and buf.shape[-1] >= w and buf.stride(-1) == 1:
        pitch = buf.shape[-1]
        y = buf[..., :h, :w]
        if order != 'i420':         # h / sy rows of chroma pairs: w samples of a row at sx = 2, 2w samples of two buffer rows at 4:4:4
            if sx == 2:
                c = buf[..., h:, :w]
            elif buf.stride(-2) != pitch:
                raise ValueError('an interleaved 4:4:4 buffer needs whole rows: a row of chroma pairs is two buffer rows long')
            else:
                c = buf[..., h:, :].flatten(-2).unflatten(-1, (h, 2 * pitch))[..., :2 * w]
            a, b = c[..., 0::2], c[..., 1::2]
            return cls(y, a, b, *tail) if order == 'nv12' else cls(y, b, a, *tail)
        if sx == 1:
            return cls(y, buf[..., h:2 * h, :w], buf[..., 2 * h:, :w], *tail)
        if pitch % 2 or buf.stride(-2) != pitch:
            planar = 'a planar 4:2:2' if fmt == '422' else 'a planar' if tail else 'an I420'
            raise ValueError(f'{planar} buffer needs an even pitch and whole rows: its chroma rows are half a luma row long')
        flat = buf.flatten(-2)          # (a view: the two last dimensions are contiguous)
        n = ch * (pitch // 2)
        cb = flat[..., h * pitch:h * pitch + n].unflatten(-1, (ch, pitch // 2))[..., :w // 2]
        cr = flat[..., h * pitch + n:h * pitch + 2 * n].unflatten(-1, (ch, pitch // 2))[..., :w // 2]
        return cls(y, cb, cr, *tail)
    if order == 'i420' and buf.dim() >= 1 and buf.shape[-1] == rows * w and buf.stride(-1) == 1:
        return _yuv_views_format(buf.unflatten(-1, (rows, w)), h, w, fmt, order, tail)
    words = '' if fmt != '420' else ' 16-bit words' if tail else ' uint8'
    raise ValueError(f'buf must be (..., {rows}, pitch >= {w}){words} with a unit last stride, got {tuple(buf.shape)}')


def yuv420_views(buf, h, w, layout='nv12'):
    """A packed uint8 buffer (..., 3h/2, pitch) -- or flat (..., nbytes) for I420 whose chroma rows are pitch/2 = w/2 apart -- ->
    Yuv420Frames of views into it (no copy).  NV12 / NV21: h rows of Y, then h/2 rows of interleaved chroma pairs, all `pitch`
    bytes apart.  I420: the Y plane, then the Cb plane and the Cr plane with rows pitch/2 apart (pitch even)."""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f'layout must be one of {YUV_LAYOUTS}, got {layout!r}')
    return _yuv_views_format(buf, h, w, '420', layout)


def yuv420p16_views(buf, h, w, layout='yuv420p10le'):
    """A packed buffer of 16-bit words (..., 3h/2, pitch) -- or flat (..., 3hw/2) for planar layouts -- -> Yuv420Frames16 of views
    into it (no copy): yuv420_views' rules with samples for bytes.  layout: 'p010' | 'p012' (Y, then interleaved Cb Cr, value in the
    high bits) | 'yuv420p10le' | 'yuv420p12le' (Y, Cb, Cr planes, value in the low bits), or ('nv12' | 'nv21' | 'i420', bit_depth,
    msb_aligned)."""
    order, depth, msb = _yuv16_layout(layout)
    return _yuv_views_format(buf, h, w, '420', order, (depth, msb))


def _yuv_size_check(fmt, h, w):
    """ValueError unless h x w frames exist in the format: sx divides w and sy divides h"""
    if fmt == '420':
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f'4:2:0 frames need an even height and width, got {h} x {w}')
    elif h < 1 or w < 1 or (fmt == '422' and w % 2):
        raise ValueError(f'4:2:2 frames need an even width, got {h} x {w}' if fmt == '422' else f'frames need a height and a width, got {h} x {w}')


def _yuv_shape_check(fmt, y_shape, cb_shape, cr_shape):
    """ValueError unless (t,h,w) frames exist in the format and the chroma planes have the format's shape, (t, h / sy, w / sx)"""
    t, h, w = y_shape
    sx, sy = _native.YUV_FACTORS[fmt]
    _yuv_size_check(fmt, h, w)
    if tuple(cb_shape) != (t, h // sy, w // sx) or tuple(cr_shape) != (t, h // sy, w // sx):
        named_c = {'420': '(t,h/2,w/2)', '422': '(t,h,w/2)', '444': '(t,h,w)'}[fmt]
        raise ValueError(f'cb and cr must be {named_c} = {(t, h // sy, w // sx)}, got {tuple(cb_shape)} and {tuple(cr_shape)}')


def _yuv_clip_desc(frames, what='frames', cls=None):
    """Yuv420Frames / Yuv420Frames16 of (t,h,w) / (t,h/2,w/2) views -> (_native.Yuv420Planes / Yuv420Planes16, t, h, w): pointers,
    pitches and frame strides in BYTES, the chroma step in samples; every refusal a ValueError / TypeError raised before any GPU
    work.  cls: as _yuv_expect"""
    sixteen = _yuv_expect(frames, what, cls)
    y, cb, cr = frames[:3]
    if sixteen:
        depth = _bit_depth(frames.bit_depth)
    dtypes, named, apart, unit = ((_WORD_DTYPES, 'int16 or uint16', 'sample apart (P010 / P012)', 'samples') if sixteen else
                                  ((torch.uint8,), 'uint8', 'byte apart (NV12 / NV21)', 'bytes'))
    for name, x in (('y', y), ('cb', cb), ('cr', cr)):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(f'{what}.{name} must be a CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
        if x.dtype not in dtypes:
            raise TypeError(f'{what}.{name} must be {named}, got {x.dtype}')
        if x.dim() != 3:
            raise ValueError(f'{what}.{name} must be (t,rows,cols) per clip, got {tuple(x.shape)}')
    t, h, w = y.shape
    fmt = yuv_format(frames)
    sx = _native.YUV_FACTORS[fmt][0]
    _yuv_shape_check(fmt, y.shape, cb.shape, cr.shape)
    if y.stride(2) != 1:
        raise ValueError(f'{what}.y must have a unit last stride, got {y.stride(2)}')
    if cb.stride() != cr.stride() or cb.stride(2) not in (1, 2):
        raise ValueError(f'{what}.cb and .cr must share their strides, with a last stride of 1 or 2: got {cb.stride()} and {cr.stride()}')
    step, size = cb.stride(2), y.element_size()
    if step == 2 and abs(cb.data_ptr() - cr.data_ptr()) != size:
        raise ValueError(f'chroma with a step of 2 must be interleaved: cb and cr one {apart}')
    if y.stride(1) < w or cb.stride(1) < step * (w // sx) or (t > 1 and (y.stride(0) < 0 or cb.stride(0) < 0)):
        raise ValueError(f'{what}: a pitch below the row\'s {unit} (strides {y.stride()}, {cb.stride()})')
    if size == 2 and (y.data_ptr() | cb.data_ptr() | cr.data_ptr()) & 1:
        raise ValueError(f'{what}: 16-bit planes must lie at even addresses')
    args = (y.data_ptr(), cb.data_ptr(), cr.data_ptr(), size * y.stride(1), size * cb.stride(1), size * y.stride(0) if t > 1 else 0,
            size * cb.stride(0) if t > 1 else 0, step)
    d = _native.Yuv420Planes16(*args, depth, int(bool(frames.msb_aligned))) if sixteen else _native.Yuv420Planes(*args)
    return d, t, h, w      # (the descriptors serve every format: the format rides in the code, yuv_format(frames))


def _yuv_clips(frames, what='frames', cls=None):
    """Yuv420Frames / Yuv420Frames16 with or without the batch dimension -> (list of per-clip frames of the same kind, lead shape).
    cls: as _yuv_expect"""
    _yuv_expect(frames, what, cls)
    if any(not isinstance(x, torch.Tensor) for x in frames[:3]):
        raise TypeError(f'{what}: y, cb and cr must be tensors')
    d = frames.y.dim()
    if d not in (3, 4) or frames.cb.dim() != d or frames.cr.dim() != d:
        raise ValueError(f'{what}: y, cb, cr must all be (n,t,rows,cols) or all (t,rows,cols), got {tuple(frames.y.shape)}, '
                         f'{tuple(frames.cb.shape)}, {tuple(frames.cr.shape)}')
    if d == 3:
        return [frames], ()
    n = frames.y.shape[0]
    if frames.cb.shape[0] != n or frames.cr.shape[0] != n:
        raise ValueError(f'{what}: y, cb and cr disagree in the batch size')
    kind = type(frames)
    return [kind(frames.y[b], frames.cb[b], frames.cr[b], *frames[3:]) for b in range(n)], (n,)


def _frames_from_yuv(frames, standard, cls=None, chroma='replicate'):
    """frames_from_yuv420 / frames_from_yuv420p16 (cls: as _yuv_expect; None: by the frames' type)"""
    std = _yuv_code(standard, chroma)
    clips, lead = _yuv_clips(frames, 'frames', cls)
    std |= _native.YUV_FORMAT[yuv_format(frames)] << 12
    descs = [_yuv_clip_desc(c) for c in clips]
    _, t, h, w = descs[0]
    if any(d[1:] != (t, h, w) for d in descs):
        raise ValueError('the clips of a batch must agree in shape')
    entry = _yuv_entry('pnp_frames_from_yuv420', frames)
    dev = frames.y.device
    with torch.cuda.device(dev):
        out = torch.empty((len(clips), t, 3, h, w), device=dev, dtype=torch.float32)
        for b, (d, _, _, _) in enumerate(descs):
            if t:
                _native.check(getattr(_native.lib(), entry)(ctypes.byref(d), std, _ptr(out[b]), t, h, w, _stream()), entry)
    return out if lead else out[0]


def _frames_to_yuv(planes, standard, out, cls, empty, chroma='replicate', fmt='420'):
    """frames_to_yuv420 / frames_to_yuv420p16 / frames_to_yuv; empty(lead, h, w, device) -> (a fresh packed buffer, its views) where out
    is None; fmt: the chroma format of the planes written"""
    std = _yuv_code(standard, chroma, fmt)
    planes = _chk(planes, 'planes')
    if planes.dim() not in (4, 5) or planes.shape[-3] != 3:
        raise ValueError(f'planes must be (n,t,3,h,w) or (t,3,h,w), got {tuple(planes.shape)}')
    h, w = planes.shape[-2:]
    _yuv_size_check(fmt, h, w)
    lead = tuple(planes.shape[:-3])
    with torch.cuda.device(planes.device):
        buf = None
        if out is None:
            buf, out = empty(lead, h, w, planes.device)
        clips, olead = _yuv_clips(out, 'out', cls)
        src = planes if planes.dim() == 5 else planes[None]
        if len(clips) != src.shape[0]:
            raise ValueError('out and planes disagree in the batch size')
        entry = _yuv_entry('pnp_frames_to_yuv420', out)
        for b, c in enumerate(clips):
            d, t, oh, ow = _yuv_clip_desc(c, 'out')
            if (t, oh, ow) != (src.shape[1], h, w):
                raise ValueError(f'out is {(t, oh, ow)}, planes are {(src.shape[1], h, w)}')
            if t:
                _native.check(getattr(_native.lib(), entry)(_ptr(src[b]), ctypes.byref(d), std, t, h, w, _stream()), entry)
    return buf, out


def _pack_lr_yuv(frames, standard, general, cls, chroma='replicate'):
    """pack_lr_yuv420 / pack_lr_yuv420p16"""
    std = _yuv_code(standard, chroma)
    d, t, h, w = _yuv_clip_desc(frames, 'frames', cls)
    std |= _native.YUV_FORMAT[yuv_format(frames)] << 12
    entry = _yuv_entry('pnp_debug_pack_lr_yuv420', frames)
    with torch.cuda.device(frames.y.device):
        out = torch.empty((t, h, w, 4), device=frames.y.device, dtype=torch.float32)
        _native.check(getattr(_native.lib(), entry)(ctypes.byref(d), std, _ptr(out), t, h, w, int(bool(general)), _stream()), entry)
    return out


def frames_from_yuv420(frames, standard='bt601-limited', chroma='replicate'):
    """Yuv420Frames (n,t,...) or (t,...) -> (n,t,3,h,w) / (t,3,h,w) fp32 RGB planes, clamped to [0,1], chroma replicated: the
    arithmetic of include/pnpvcve.h, bit-equal to tests/yuv_ref.py.  What generator.forward(Yuv420Frames) computes on, without this
    fp32 clip.  chroma: 'replicate' | 'center' | 'left' | 'topleft', the header's chroma modes (the siting of the chroma samples;
    every mode but the first interpolates them bilinearly; bit-equal to tests/yuv_chroma_ref.py)."""
    return _frames_from_yuv(frames, standard, Yuv420Frames, chroma)


def frames_from_yuv420p16(frames, standard='bt601-limited', chroma='replicate'):
    """Yuv420Frames16 (n,t,...) or (t,...) -> (n,t,3,h,w) / (t,3,h,w) fp32 RGB planes, clamped to [0,1], chroma replicated: the
    arithmetic of include/pnpvcve.h at the frames' depth, bit-equal to tests/yuv16_ref.py.  What generator.forward(Yuv420Frames16)
    computes on, without this fp32 clip.  chroma: as frames_from_yuv420."""
    return _frames_from_yuv(frames, standard, Yuv420Frames16, chroma)


def empty_yuv420(lead, h, w, layout, device):
    """-> (packed uint8 buffer lead + (3h/2, w), its Yuv420Frames views)"""
    buf = torch.empty(tuple(lead) + (h * 3 // 2, w), device=device, dtype=torch.uint8)
    return buf, yuv420_views(buf, h, w, layout)


def empty_yuv420p16(lead, h, w, layout, device, dtype=torch.int16):
    """-> (packed buffer of 16-bit words lead + (3h/2, w), its Yuv420Frames16 views)"""
    buf = torch.empty(tuple(lead) + (h * 3 // 2, w), device=device, dtype=dtype)
    return buf, yuv420p16_views(buf, h, w, layout)


def frames_to_yuv420(planes, standard='bt601-limited', layout='nv12', out=None, chroma='replicate'):
    """(n,t,3,h,w) or (t,3,h,w) fp32 CUDA planes -> (packed uint8 buffer (...,3h/2,w) in `layout`, its Yuv420Frames views): clamp,
    luma, box-mean chroma, round half to even (include/pnpvcve.h).  out: Yuv420Frames views to write instead of a fresh buffer
    (any pitch and address; returns (None, out)).  chroma: the header's chroma mode; 'left' and 'topleft' filter [1 2 1] / 4 on
    their co-sited axes where the other two take the box mean."""
    return _frames_to_yuv(planes, standard, out, Yuv420Frames, lambda lead, h, w, dev: empty_yuv420(lead, h, w, layout, dev), chroma)


def frames_to_yuv420p16(planes, standard='bt601-limited', layout='yuv420p10le', out=None, dtype=torch.int16, chroma='replicate'):
    """(n,t,3,h,w) or (t,3,h,w) fp32 CUDA planes -> (packed buffer of 16-bit words (...,3h/2,w) in `layout`, its Yuv420Frames16
    views): clamp, luma, box-mean chroma, round half to even to [0, 2^d - 1], the bits outside the value zero (include/pnpvcve.h).
    out: Yuv420Frames16 views to write instead of a fresh buffer (any pitch, any even address; returns (None, out)); the depth and
    container are then out's.  chroma: as frames_to_yuv420."""
    return _frames_to_yuv(planes, standard, out, Yuv420Frames16, lambda lead, h, w, dev: empty_yuv420p16(lead, h, w, layout, dev, dtype), chroma)


def pack_lr_yuv420(frames, standard='bt601-limited', general=False, chroma='replicate'):
    """(include/pnpvcve_debug.h) one clip's Yuv420Frames (t,...) -> the (t,h,w,4) fp32 RGB0 conv source the forward unpacks them into;
    general: the byte-load form whatever the alignment; chroma: the header's chroma mode"""
    return _pack_lr_yuv(frames, standard, general, Yuv420Frames, chroma)


def pack_lr_yuv420p16(frames, standard='bt601-limited', general=False, chroma='replicate'):
    """(include/pnpvcve_debug.h) one clip's Yuv420Frames16 (t,...) -> the (t,h,w,4) fp32 RGB0 conv source the forward unpacks them
    into; general: the 2-byte-load form whatever the alignment; chroma: the header's chroma mode"""
    return _pack_lr_yuv(frames, standard, general, Yuv420Frames16, chroma)


# ---------------------------------------------------------------- every chroma format (include/pnpvcve.h, "Chroma formats")
def yuv_views(buf, h, w, layout):
    """A packed buffer in any layout of any chroma format -> views of the format's frame class (no copy).  4:2:0 layouts: yuv420_views /
    yuv420p16_views.  4:2:2 ('yuv422p', 'nv16', 'yuv422p10le', 'yuv422p12le', 'p210', 'p212'): (..., 2h, pitch); 4:4:4 ('yuv444p',
    'nv24', 'yuv444p10le', 'yuv444p12le', 'p410', 'p412'): (..., 3h, pitch) -- h rows of Y, then the Cb and the Cr plane (planar) or h
    rows of Cb Cr pairs (interleaved), by yuv420_views' plane-order rules; planar layouts also as a flat (..., samples) buffer."""
    fmt, order, depth, msb = yuv_layout(layout)
    if fmt == '420':
        return yuv420_views(buf, h, w, layout) if depth == 8 else yuv420p16_views(buf, h, w, layout)
    return _yuv_views_format(buf, h, w, fmt, order, () if depth == 8 else (depth, msb))


def empty_yuv(lead, h, w, layout, device, dtype=torch.int16):
    """-> (a fresh packed buffer lead + (rows, w) in `layout`, its views); dtype: the dtype of 16-bit words"""
    fmt, order, depth, msb = yuv_layout(layout)
    if fmt == '420':
        return empty_yuv420(lead, h, w, layout, device) if depth == 8 else empty_yuv420p16(lead, h, w, layout, device, dtype)
    _yuv_size_check(fmt, h, w)
    buf = torch.empty(tuple(lead) + (h + 2 * h // _native.YUV_FACTORS[fmt][0], w), device=device, dtype=torch.uint8 if depth == 8 else dtype)
    return buf, yuv_views(buf, h, w, layout)


def frames_from_yuv(frames, standard='bt601-limited', chroma='replicate'):
    """Frames of any class (n,t,...) or (t,...) -> (n,t,3,h,w) / (t,3,h,w) fp32 RGB planes clamped to [0,1]: the arithmetic of
    include/pnpvcve.h for the frames' chroma format, bit-equal to tests/yuv_formats_ref.py.  In 4:2:2 'left' and 'topleft' are one
    function, in 4:4:4 all four chroma modes are."""
    if not is_yuv(frames):
        raise TypeError('frames must be ops.Yuv420Frames / Yuv422Frames / Yuv444Frames or their 16-bit siblings')
    return _frames_from_yuv(frames, standard, None, chroma)


def frames_to_yuv(planes, standard='bt601-limited', layout='nv16', out=None, chroma='replicate', dtype=torch.int16):
    """(n,t,3,h,w) or (t,3,h,w) fp32 CUDA planes -> (a packed buffer in `layout`, its views), any layout of any format
    (include/pnpvcve.h).  out: views of any frame class to write instead (returns (None, out)); the format, depth and container are
    then out's."""
    if out is not None:
        if not is_yuv(out):
            raise TypeError('out must be ops.Yuv420Frames / Yuv422Frames / Yuv444Frames or their 16-bit siblings')
        fmt = yuv_format(out)
    else:
        fmt = yuv_layout(layout)[0]
    return _frames_to_yuv(planes, standard, out, None, lambda lead, h, w, dev: empty_yuv(lead, h, w, layout, dev, dtype), chroma, fmt)


def pack_lr_yuv(frames, standard='bt601-limited', general=False, chroma='replicate'):
    """(include/pnpvcve_debug.h) one clip's frames of any class (t,...) -> the (t,h,w,4) fp32 RGB0 conv source the forward unpacks them
    into; general: the single-sample-load form whatever the alignment"""
    if not is_yuv(frames):
        raise TypeError('frames must be ops.Yuv420Frames / Yuv422Frames / Yuv444Frames or their 16-bit siblings')
    return _pack_lr_yuv(frames, standard, general, None, chroma)


# ---------------------------------------------------------------- plane metrics of 4:2:0 clips (include/pnpvcve.h states the arithmetic)
_PLANE_BITS = {'y': _native.PLANE_Y, 'u': _native.PLANE_CB, 'v': _native.PLANE_CR}


def _metric_planes(planes):
    """planes of a 4:2:0 metric: any of 'y', 'u', 'v' in any order, each at most once -> in lower case"""
    if not isinstance(planes, str) or not planes or len(set(planes.lower())) != len(planes) or any(p not in _PLANE_BITS for p in planes.lower()):
        raise ValueError(f"planes must name each of 'y', 'u', 'v' at most once, got {planes!r}")
    return planes.lower()


def _yuv_metric_pair(a, b, crop_border, any_format=False):
    """two Yuv420Frames that show the same frames, (n,t,...) or (t,...), each in a layout of its own -> (per-clip descriptor pairs,
    lead shape, t, h, w, crop); every refusal a ValueError / TypeError raised before any GPU work.  Two Yuv420Frames16 of one bit
    depth (each in a container of its own) are scored at that depth; an 8-bit clip against a 16-bit one is refused.  any_format: frames
    of the other chroma formats are taken too (both clips of one format; crop_border even unless the format is 4:4:4); otherwise they
    are a TypeError."""
    for name, x in (('a', a), ('b', b)):
        if is_yuv(x) and yuv_format(x) != '420' and not any_format:
            raise TypeError(f'{name} must be ops.Yuv420Frames or ops.Yuv420Frames16: the metric is defined on 4:2:0 clips, got a 4:{yuv_format(x)[1:2]}:'
                            f'{yuv_format(x)[2:]} clip ({type(x).__name__})')
    if is_yuv(a) and is_yuv(b) and yuv_format(a) != yuv_format(b):
        raise ValueError(f'the two clips differ in chroma format: {yuv_format(a)} and {yuv_format(b)}')
    if isinstance(a, _YUV16_CLASSES) != isinstance(b, _YUV16_CLASSES):
        raise ValueError('a and b must both be 8-bit (Yuv420Frames) or both 16-bit (Yuv420Frames16) clips')
    if isinstance(a, _YUV16_CLASSES) and _bit_depth(a.bit_depth) != _bit_depth(b.bit_depth):
        raise ValueError(f'the two clips differ in bit depth: {a.bit_depth} and {b.bit_depth}')
    clips_a, lead_a = _yuv_clips(a, 'a')
    clips_b, lead_b = _yuv_clips(b, 'b')
    da = [_yuv_clip_desc(c, 'a') for c in clips_a]
    db = [_yuv_clip_desc(c, 'b') for c in clips_b]
    t, h, w = da[0][1:]
    if lead_a != lead_b or any(d[1:] != (t, h, w) for d in da + db):
        raise ValueError(f'the two clips differ in shape: {tuple(a.y.shape)} and {tuple(b.y.shape)}')
    if a.y.device != b.y.device:
        raise RuntimeError('a and b must be on the same device')
    if isinstance(crop_border, bool) or int(crop_border) != crop_border:
        raise TypeError(f'crop_border must be an integer, got {crop_border!r}')
    crop = int(crop_border)
    if crop < 0 or (crop % 2 and yuv_format(a) != '444'):
        raise ValueError(f'crop_border must be even and >= 0 (the chroma planes are cropped by half of it), got {crop}')
    if 2 * crop >= h or 2 * crop >= w:
        raise ValueError(f'a crop of {crop} leaves nothing of {h} x {w} frames')
    return [(x[0], y[0]) for x, y in zip(da, db)], lead_a + (t,), t, h, w, crop


def _plane_geometry(fmt, h, w, crop):
    """-> {'y' | 'u' | 'v': (rows, cols, crop down, crop across)} of a format (include/pnpvcve.h, the crop rule)"""
    sx, sy = _native.YUV_FACTORS[fmt]
    c = (h // sy, w // sx, crop // sy, crop // sx)
    return {'y': (h, w, crop, crop), 'u': c, 'v': c}


def _psnr_sse_yuv(a, b, crop_border, any_format):
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, b, crop_border, any_format=any_format)
    fmt = _native.YUV_FORMAT[yuv_format(a)]
    sse = torch.empty((len(pairs), t, 3), dtype=torch.int64, device=a.y.device)
    _yuv_all_clips('pnp_psnr_sse_yuv', a, pairs, t, lambda entry, i, da, db: entry(da, db, _ptr(sse[i]), t, h, w, crop, fmt, _stream()))
    return sse.cpu().reshape(lead + (3,))


def _psnr_yuv(a, b, crop_border, any_format):
    import numpy as np
    sse = _psnr_sse_yuv(a, b, crop_border, any_format).numpy().astype(np.float64)
    h, w = a.y.shape[-2:]
    geo = _plane_geometry(yuv_format(a), h, w, int(crop_border))
    n = [(r - 2 * cy) * (c - 2 * cx) for r, c, cy, cx in (geo[p] for p in 'yuv')]
    with np.errstate(divide='ignore'):
        peak = float((1 << a.bit_depth) - 1) if isinstance(a, _YUV16_CLASSES) else 255.0
        out = 10.0 * np.log10(peak ** 2 * np.array(n, np.float64) / sse)
    out[sse == 0] = np.inf
    return torch.from_numpy(out)


def _ssim_yuv(a, b, crop_border, planes, any_format):
    planes = _metric_planes(planes)
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, b, crop_border, any_format=any_format)
    L = _native.lib()
    fmt = _native.YUV_FORMAT[yuv_format(a)]
    geo = _plane_geometry(yuv_format(a), h, w, crop)
    mask = sum(_PLANE_BITS[p] for p in planes)
    order = [p for p in 'yuv' if p in planes]                      # the order the library writes
    nb = {p: int(L.pnp_ssim_blocks_yuv(h, w, crop, _PLANE_BITS[p], fmt)) for p in order}
    if any(v < 1 for v in nb.values()):
        raise ValueError('a cropped plane is smaller than the 11x11 SSIM window')
    res = torch.empty((len(pairs), t, len(planes)), dtype=torch.float64)
    part = torch.empty(t * sum(nb.values()), dtype=torch.float64, device=a.y.device)
    for i in _yuv_each_clip('pnp_ssim_partials_yuv', a, pairs, t,
                            lambda entry, i, da, db: entry(da, db, mask, _ptr(part), t, h, w, crop, fmt, _stream())):
        off = 0
        for p in order:
            rows, cols, cy, cx = geo[p]
            n = (rows - 2 * cy - 10) * (cols - 2 * cx - 10)
            res[i, :, planes.index(p)] = (part[off:off + t * nb[p]].reshape(t, nb[p]).sum(dim=1) / n).cpu()
            off += t * nb[p]
    return res.reshape(lead + (len(planes),))


def psnr_sse_yuv420(a, b, crop_border=0):
    """The statistic behind psnr_yuv420: the exact sum of squared byte differences of the cropped Y, Cb and Cr planes of every frame, an
    int64 CPU tensor lead + (3,) (pnp_psnr_sse_yuv420: integer, the same bits every run).  Two Yuv420Frames16: the sample values'
    differences (pnp_psnr_sse_yuv420p16)."""
    return _psnr_sse_yuv(a, b, crop_border, False)


def psnr_yuv420(a, b, crop_border=0):
    """Per-frame plane PSNR of two 8-bit 4:2:0 clips, read from the planes where they lie (1.5 B per pixel and clip).
    a, b: Yuv420Frames (n,t,...) or (t,...) of one shape, each in its own layout (NV12 output against an I420 ground truth); the Y
    plane is cropped by crop_border (even), the chroma planes by crop_border / 2.  Returns a float64 CPU tensor lead + (3,) = Y, U, V:
    PSNR_p = 10 log10(255^2 N_p / SSE_p) with N_p the samples of the cropped plane, inf where the planes are equal.  Two
    Yuv420Frames16 of one bit depth d are scored on their sample values with the peak 2^d - 1 in place of 255."""
    return _psnr_yuv(a, b, crop_border, False)


def ssim_yuv420(a, b, crop_border=0, planes='y'):
    """Per-frame plane SSIM of two 8-bit 4:2:0 clips (pnp_ssim_partials_yuv420: ssim_frames' window and fp64 arithmetic on the bytes of a
    plane).  planes: any of 'y', 'u', 'v' in any order ('yuv', 'u', 'vy', ...); returns a float64 CPU tensor lead + (len(planes),) in
    that order.  Crop as psnr_yuv420.  Two Yuv420Frames16 of one bit depth d: the same on the sample values, L = 2^d - 1
    (pnp_ssim_partials_yuv420p16)."""
    return _ssim_yuv(a, b, crop_border, planes, False)


def psnr_sse_yuv(a, b, crop_border=0):
    """psnr_sse_yuv420 for clips of any chroma format (pnp_psnr_sse_yuv / pnp_psnr_sse_yuvp16): the exact SSE of the cropped Y, Cb and Cr
    planes of every frame, an int64 CPU tensor lead + (3,).  The chroma planes are cropped by crop_border / sx across and / sy down;
    crop_border is even for 4:2:0 and 4:2:2, any value >= 0 for 4:4:4."""
    return _psnr_sse_yuv(a, b, crop_border, True)


def psnr_yuv(a, b, crop_border=0):
    """psnr_yuv420 for clips of any chroma format: a float64 CPU tensor lead + (3,) = Y, U, V, PSNR_p = 10 log10(peak^2 N_p / SSE_p) with
    N_p the samples of the cropped plane (N_C = (h/sy - 2c/sy)(w/sx - 2c/sx)), inf where the planes are equal."""
    return _psnr_yuv(a, b, crop_border, True)


def ssim_yuv(a, b, crop_border=0, planes='y'):
    """ssim_yuv420 for clips of any chroma format (pnp_ssim_partials_yuv / pnp_ssim_partials_yuvp16): per-frame plane SSIM, a float64
    CPU tensor lead + (len(planes),) in the order of `planes`.  Crop as psnr_sse_yuv."""
    return _ssim_yuv(a, b, crop_border, planes, True)


def msssim_yuv420(a, b, crop_border=0, planes='y', scales=False):
    """Per-frame plane MS-SSIM of two 4:2:0 clips (pnp_msssim_partials_yuv420 / _yuv420p16: msssim_frames' definition on the samples of
    a plane, peak 255 or 2^d - 1).  a, b, planes and the crop as ssim_yuv420: two Yuv420Frames, or two Yuv420Frames16 of one depth,
    each in a layout of its own; returns a float64 CPU tensor lead + (len(planes),) in the order of `planes`, with scales=True also the
    raw per-level means lead + (len(planes), 5, 2) = (CS_s, S_s).  Every cropped plane asked for must be at least 176 x 176: chroma
    planes need 352-line frames."""
    planes = _metric_planes(planes)
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, b, crop_border)
    L = _native.lib()
    mask = sum(_PLANE_BITS[p] for p in planes)
    order = [p for p in 'yuv' if p in planes]                      # the order the library writes
    plans = {}
    for p in order:
        plans[p] = _msssim_plan(h, w, crop) if p == 'y' else _msssim_plan(h // 2, w // 2, crop // 2)
        if plans[p] is None:
            raise _msssim_too_small(f'plane {p!r}')
    dev = a.y.device
    res = torch.empty((len(pairs), t, len(planes)), dtype=torch.float64)
    sc = torch.empty((len(pairs), t, len(planes), 5, 2), dtype=torch.float64)
    part = torch.empty(t * sum(sum(plans[p][0]) for p in order) * 2, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.pnp_msssim_workspace_bytes(t, len(order), h, w, crop)) // 4, dtype=torch.float32, device=dev)
    for i in _yuv_each_clip('pnp_msssim_partials_yuv420', a, pairs, t,
                            lambda entry, i, da, db: entry(da, db, mask, _ptr(part), _ptr(ws), t, h, w, crop, _stream())):
        off = 0
        for p in order:
            blocks, sizes = plans[p]
            n = t * sum(blocks) * 2
            s = _msssim_scales(part[off:off + n].reshape(t, sum(blocks), 2), blocks, sizes)
            sc[i, :, planes.index(p)] = s
            res[i, :, planes.index(p)] = _msssim_value(s)
            off += n
    res = res.reshape(lead + (len(planes),))
    return (res, sc.reshape(lead + (len(planes), 5, 2))) if scales else res


def _xpsnr_args(planes, fps):
    planes = _metric_planes(planes)
    if isinstance(fps, bool) or not isinstance(fps, int) or fps < 1:
        raise ValueError(f'fps must be an integer >= 1 (it chooses the order of the temporal activity), got {fps!r}')
    return planes, int(fps)


def xpsnr_sums_yuv420(a, b, crop_border=0, planes='y', fps=30):
    """The statistic behind xpsnr_yuv420 (pnp_xpsnr_sums_yuv420 / _yuv420p16; include/pnpvcve.h states the metric): a is the test clip, b
    the ORIGINAL, two Yuv420Frames or two Yuv420Frames16 of one depth, (n,t,...) or (t,...), each in a layout of its own.  Returns an
    int64 CPU tensor lead + (rows * cols, 5): per frame and block of the XPSNR grid of the cropped frame the exact sse_y, sse_u, sse_v
    (0 for planes not named in `planes`) and the spatial and temporal activity sums sa, ta of b's luma.  Integer, the same bits every
    run; a clip's frames are one call, since frame t reads the original's frames t - 1 and t - 2."""
    planes, fps = _xpsnr_args(planes, fps)
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, b, crop_border)
    L = _native.lib()
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    _native.check(L.pnp_xpsnr_grid(h, w, crop, ctypes.byref(rows), ctypes.byref(cols)), 'pnp_xpsnr_grid')
    nblk = rows.value * cols.value
    mask = sum(_PLANE_BITS[p] for p in planes)
    sums = torch.empty((len(pairs), t, nblk, 5), dtype=torch.int64, device=a.y.device)
    _yuv_all_clips('pnp_xpsnr_sums_yuv420', a, pairs, t, lambda entry, i, da, db: entry(da, db, mask, _ptr(sums[i]), t, h, w, crop, fps, _stream()))
    return sums.cpu().reshape(lead + (nblk, 5))


def xpsnr_yuv420(a, b, crop_border=0, planes='y', fps=30, clip=False):
    """XPSNR of two 4:2:0 clips (include/pnpvcve.h: a PSNR whose squared error is weighted block by block with the inverse of the
    original's spatio-temporal activity).  a: the test clip, b: the ORIGINAL; two Yuv420Frames, or two Yuv420Frames16 of one depth,
    each in a layout of its own; crop as psnr_yuv420; planes as ssim_yuv420; fps >= 1 (from 32 on the temporal activity is of second
    order).  Returns (wsse, dB): float64 CPU tensors lead + (len(planes),), the weighted squared error and XPSNR of every frame, in the
    order of `planes`; with clip=True also the clip's value lead[:-1] + (len(planes),), 10 log10 of the MEAN weighted error over the
    frames (the metric's convention, not the mean of the frames' dB).  The integers are the device's (xpsnr_sums_yuv420); the fp64 part
    is metrics.xpsnr_values, the host path's own."""
    from . import metrics
    planes, fps = _xpsnr_args(planes, fps)
    sums = xpsnr_sums_yuv420(a, b, crop_border, planes, fps)
    t = sums.shape[-3]
    crop = int(crop_border)
    h, w = a.y.shape[-2] - 2 * crop, a.y.shape[-1] - 2 * crop
    d = a.bit_depth if isinstance(a, Yuv420Frames16) else 8
    flat = sums.reshape((-1,) + tuple(sums.shape[-3:])).numpy()
    if not t:
        raise ValueError('XPSNR needs at least one frame')
    vals = [metrics.xpsnr_values(s, d, fps, h, w, planes) for s in flat]
    lead = tuple(sums.shape[:-2])

    def gather(k, shape):
        import numpy as np
        return torch.from_numpy(np.ascontiguousarray(np.stack([v[k] for v in vals]), dtype=np.float64)).reshape(shape)

    wsse, db = gather(0, lead + (len(planes),)), gather(1, lead + (len(planes),))
    return (wsse, db, gather(2, lead[:-1] + (len(planes),))) if clip else (wsse, db)


# ---------------------------------------------------------------- PSNR-B (include/pnpvcve.h, pnp_psnrb_*)
def _psnrb_values(sums, plane_dims, block, peak, chroma):
    """sums (..., planes, 5) -> (PSNR-B, BEF) float64 tensors (..., planes): metrics.psnrb_values, the host path's own fp64 part, on each
    plane.  plane_dims[k] = (rows, cols, crop) of plane k, chroma[k] whether it is a chroma plane of 4:2:0 (half the block)."""
    import numpy as np
    from . import metrics
    s = sums.numpy()
    val, bef = np.empty(s.shape[:-1], np.float64), np.empty(s.shape[:-1], np.float64)
    for k, (rows, cols, crop) in enumerate(plane_dims):
        bp = metrics.psnrb_block(block, chroma[k])
        counts = metrics.psnrb_counts(rows, cols, crop, bp)
        val[..., k], bef[..., k] = metrics.psnrb_values(s[..., k, :], counts, bp, (rows - 2 * crop, cols - 2 * crop), peak)
    return torch.from_numpy(val), torch.from_numpy(bef)


@_on_device_of_first_tensor
def psnrb_sums_frames(a, b, crop_border=0, convert_to=None, block=8):
    """The statistic behind psnrb_frames (pnp_psnrb_sums_io; include/pnpvcve.h states the metric).  a: the TEST clip, whose block edges
    are measured; b: the reference, or None (the no-reference form: sse = 0, b is not read); each on its own fp32 (...,c,h,w) planes or
    uint8 (...,h,w,3) RGB frames.  convert_to None: an int64 CPU tensor lead + (c, 5) = sse, sbh, snh, sbv, snv of every frame and channel,
    exact, the same bits every run.  'y': a float64 CPU tensor lead + (1, 5), the sums over the fp32 Y (a frame's per-block partials
    added in index order)."""
    from . import metrics
    if b is None:
        color = _metric_color(convert_to)
        a, fa, lead, c, h, w = _metric_frames(a, 'a')
        if color == _native.COLOR_Y and c != 3:
            raise ValueError('a must have 3 channels')
        frames = 1
        for d in lead:
            frames *= d
        fb = fa
    else:
        a, fa, b, fb, color, lead, frames, c, h, w = _metric_pair(a, b, convert_to)
    crop = int(crop_border)
    metrics.psnrb_counts(h, w, crop, metrics.psnrb_block(block))         # every refusal a ValueError raised before any GPU work
    L = _native.lib()
    if color == _native.COLOR_Y:
        nb = int(L.pnp_psnrb_luma_blocks(h, w, crop))
        out = torch.empty((frames, nb, 5), dtype=torch.float64, device=a.device)
    else:
        out = torch.empty((frames, c, 5), dtype=torch.int64, device=a.device)
    if frames:
        _native.check(L.pnp_psnrb_sums_io(_ptr(a), fa, None if b is None else _ptr(b), fb, color, _ptr(out), frames, c, h, w, crop, int(block),
                                          _stream()), 'pnp_psnrb_sums_io')
    if color == _native.COLOR_Y:
        import numpy as np
        part = out.cpu().numpy()
        sums = part.cumsum(axis=1)[:, -1].copy() if frames else np.zeros((0, 5), np.float64)      # index order
        return torch.from_numpy(sums).reshape(lead + (1, 5))
    return out.cpu().reshape(lead + (c, 5))


def _psnrb_frames(a, b, crop_border, convert_to, block):
    sums = psnrb_sums_frames(a, b, crop_border, convert_to, block)
    h, w = (a.shape[-3:-1] if a.dtype == torch.uint8 else a.shape[-2:])
    planes = sums.shape[-2]
    return _psnrb_values(sums, [(int(h), int(w), int(crop_border))] * planes, block, 255.0, [False] * planes)


def psnrb_frames(a, b, crop_border=0, convert_to=None, block=8):
    """Per-frame PSNR-B (Yim and Bovik 2011; include/pnpvcve.h) of the test clip a against the reference b on the GPU: PSNR with the
    blocking effect factor of a's `block` x `block` grid (4, 8, 16, 32 or 64; anchored at the uncropped frame's origin) added to the mean
    squared error.  a, b, crop_border and convert_to as psnr_frames; several channels give the mean of the channels' values.  Returns a
    float64 CPU tensor of the leading shape.  The sums are the device's (psnrb_sums_frames); the fp64 part is metrics.psnrb_values."""
    import numpy as np
    return torch.from_numpy(np.asarray(_psnrb_frames(a, b, crop_border, convert_to, block)[0].numpy().mean(axis=-1)))


def bef_frames(a, crop_border=0, convert_to=None, block=8):
    """The blocking effect factor of a clip alone, per frame (the BEF of psnrb_frames, the mean over the channels): a no-reference
    blockiness figure in squared sample units.  Nothing but `a` is read."""
    import numpy as np
    return torch.from_numpy(np.asarray(_psnrb_frames(a, None, crop_border, convert_to, block)[1].numpy().mean(axis=-1)))


def psnrb_sums_yuv420(a, b, crop_border=0, planes='y', block=8):
    """The statistic behind psnrb_yuv420 (pnp_psnrb_sums_yuv420 / _yuv420p16): a is the TEST clip, b the reference or None (sse = 0, b is
    not read); two Yuv420Frames or two Yuv420Frames16 of one depth, (n,t,...) or (t,...), each in a layout of its own.  Returns an int64
    CPU tensor lead + (3, 5): per frame and plane Y, Cb, Cr the exact sse, sbh, snh, sbv, snv, 0 for the planes not named in `planes`
    (they are not read).  Blocks are `block` on Y and block / 2 on the chroma planes; the crop as psnr_yuv420."""
    from . import metrics
    planes = _metric_planes(planes)
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, a if b is None else b, crop_border)
    for p in planes:
        rows, cols, c = (h, w, crop) if p == 'y' else (h // 2, w // 2, crop // 2)
        metrics.psnrb_counts(rows, cols, c, metrics.psnrb_block(block, p != 'y'))
    mask = sum(_PLANE_BITS[p] for p in planes)
    sums = torch.empty((len(pairs), t, 3, 5), dtype=torch.int64, device=a.y.device)
    _yuv_all_clips('pnp_psnrb_sums_yuv420', a, pairs, t,
                   lambda entry, i, da, db: entry(da, None if b is None else db, mask, _ptr(sums[i]), t, h, w, crop, int(block), _stream()))
    return sums.cpu().reshape(lead + (3, 5))


def _psnrb_yuv420(a, b, crop_border, planes, block):
    planes = _metric_planes(planes)
    sums = psnrb_sums_yuv420(a, b, crop_border, planes, block)
    h, w = (int(x) for x in a.y.shape[-2:])
    crop = int(crop_border)
    idx = ['yuv'.index(p) for p in planes]
    dims = [(h, w, crop) if p == 'y' else (h // 2, w // 2, crop // 2) for p in planes]
    peak = float((1 << a.bit_depth) - 1) if isinstance(a, Yuv420Frames16) else 255.0
    return _psnrb_values(sums[..., idx, :], dims, block, peak, [p != 'y' for p in planes])


def psnrb_yuv420(a, b, crop_border=0, planes='y', block=8):
    """Per-frame plane PSNR-B of two 4:2:0 clips (include/pnpvcve.h): a is the test clip, b the reference; two Yuv420Frames, or two
    Yuv420Frames16 of one depth d (peak 2^d - 1), each in a layout of its own.  planes as ssim_yuv420; returns a float64 CPU tensor lead +
    (len(planes),) in that order.  The integers are the device's (psnrb_sums_yuv420); the fp64 part is metrics.psnrb_values."""
    return _psnrb_yuv420(a, b, crop_border, planes, block)[0]


def bef_yuv420(a, crop_border=0, planes='y', block=8):
    """The blocking effect factor of the planes of one 4:2:0 clip alone, per frame: float64 CPU tensor lead + (len(planes),)"""
    return _psnrb_yuv420(a, None, crop_border, planes, block)[1]


# ---------------------------------------------------------------- enhancement gain (include/pnpvcve.h, pnp_gain_*)
def _gain_par(par, lead, h, w, device):
    """the partition map of a gain call: None, or fp32 lead + (3, h, w) on the clips' device -> contiguous"""
    if par is None:
        return None
    if not isinstance(par, torch.Tensor) or not par.is_cuda or par.device != device:
        raise RuntimeError("par must be a CUDA/HIP tensor on the clips' device: the PnP-VCVE hot path has no CPU fallback")
    if par.dtype != torch.float32 or tuple(par.shape) != tuple(lead) + (3, h, w):
        raise ValueError(f'par must be float32 {tuple(lead) + (3, h, w)}, as the generator takes it: got {par.dtype} {tuple(par.shape)}')
    return par.contiguous()


def _gain_crop(crop_border, h, w):
    if isinstance(crop_border, bool) or int(crop_border) != crop_border or crop_border < 0 or 2 * crop_border >= h or 2 * crop_border >= w:
        raise ValueError(f'a crop of {crop_border!r} leaves nothing of {h} x {w} frames (or is no integer >= 0)')
    return int(crop_border)


@_on_device_of_first_tensor
def gain_sums_frames(a, l, g, crop_border=0, convert_to=None, block=64, par=None):
    """The sums behind gain_frames (pnp_gain_sums_io; include/pnpvcve.h states the definition): a the test clip, l the compressed input,
    g the original, each on its own fp32 (...,3,h,w) planes or uint8 (...,h,w,3) RGB frames of one leading shape.  ONE launch reads the
    three clips once.  -> (grid, classes): grid lead + (1, rows, cols, 2) = E_a, E_l of every block x block cell (16, 32, 64 or 128;
    anchored at the uncropped frame's origin), an int64 CPU tensor -- the three channels of a pixel added, exact, the same bits every
    run --, float64 with convert_to 'y'; classes lead + (8, 3) = N, E_a, E_l of every partition class of par (fp32 lead + (3, h, w)),
    or None without par.  Every refusal is raised before any GPU work."""
    from . import metrics
    a, fa, g, fg, color, lead, frames, c, h, w = _metric_pair(a, g, convert_to)
    l, fl, lead_l, cl, hl, wl = _metric_frames(l, 'l')
    if (lead_l, cl, hl, wl) != (lead, c, h, w):
        raise ValueError(f'the three clips differ in shape: a and g show {lead + (c, h, w)}, l {lead_l + (cl, hl, wl)}')
    if l.device != a.device:
        raise RuntimeError('a, l and g must be on the same device')
    if c != 3:
        raise ValueError(f'the gain is kept on RGB frames (3 channels), got {c}')
    block, crop = metrics.gain_block(block), _gain_crop(crop_border, h, w)
    par = _gain_par(par, lead, h, w, a.device)
    rows, cols = metrics.gain_grid(h, w, block)
    L = _native.lib()
    y = color == _native.COLOR_Y
    grid = torch.empty((frames, 1, rows, cols, 2), dtype=torch.float64 if y else torch.int64, device=a.device)
    cls = None
    if par is not None:
        tiles = int(L.pnp_gain_luma_tiles(h, w, crop, block))
        cls = torch.empty((frames, tiles, 8, 3) if y else (frames, 8, 3), dtype=grid.dtype, device=a.device)
    if frames:
        _native.check(L.pnp_gain_sums_io(_ptr(a), fa, _ptr(l), fl, _ptr(g), fg, color, None if par is None else _ptr(par), _ptr(grid),
                                         None if cls is None else _ptr(cls), frames, c, h, w, crop, block, _stream()), 'pnp_gain_sums_io')
    grid = grid.cpu().reshape(lead + (1, rows, cols, 2))
    if cls is None:
        return grid, None
    if y:
        import numpy as np
        part = cls.cpu().numpy()
        cls = torch.from_numpy(part.cumsum(axis=1)[:, -1].copy() if frames else np.zeros((0, 8, 3), np.float64))      # a frame's tiles in index order
    return grid, cls.cpu().reshape(lead + (8, 3))


def gain_sums_yuv(a, l, g, crop_border=0, planes='y', block=64, par=None):
    """The sums behind gain_yuv (pnp_gain_sums_yuv / _yuvp16): three clips of ONE frame class (any of the six: 4:2:0, 4:2:2, 4:4:4, 8-bit
    or 16-bit words of one depth), (n,t,...) or (t,...), each in a layout of its own.  -> (grid, classes): grid an int64 CPU tensor lead +
    (len(planes), rows, cols, 2) = E_a, E_l of every cell of the planes named, in that order (a chroma cell is block / sy x block / sx
    samples: cell (i, j) is the same picture area in every plane); classes lead + (8, 3) = N, E_a, E_l of every partition class on the Y
    plane (par: fp32 lead + (3, h, w); it needs 'y' among the planes), or None.  The crop as psnr_yuv."""
    from . import metrics
    planes = _metric_planes(planes)
    if type(a) is not type(l) or type(a) is not type(g):
        raise ValueError(f'the three clips must be of one frame class, got {type(a).__name__}, {type(l).__name__} and {type(g).__name__}')
    pairs, lead, t, h, w, crop = _yuv_metric_pair(a, g, crop_border, any_format=True)
    pairs_l = _yuv_metric_pair(l, g, crop_border, any_format=True)[0]
    block = metrics.gain_block(block)
    if par is not None and 'y' not in planes:
        raise ValueError(f"partition classes are kept on the Y plane: planes must name 'y' with par, got {planes!r}")
    dev = a.y.device
    par = _gain_par(par, lead, h, w, dev)
    rows, cols = metrics.gain_grid(h, w, block)
    mask = sum(_PLANE_BITS[p] for p in planes)
    fmt = _native.YUV_FORMAT[yuv_format(a)]
    grid = torch.empty((len(pairs), t, 3, rows, cols, 2), dtype=torch.int64, device=dev)
    cls = None if par is None else torch.empty((len(pairs), t, 8, 3), dtype=torch.int64, device=dev)
    par_clips = None if par is None else par.reshape((len(pairs), t, 3, h, w))
    _yuv_all_clips('pnp_gain_sums_yuv', a, [(da, dl, dg) for (da, dg), (dl, _) in zip(pairs, pairs_l)], t,
                   lambda entry, i, da, dl, dg: entry(da, dl, dg, mask, None if par is None else _ptr(par_clips[i]), _ptr(grid[i]),
                                                      None if cls is None else _ptr(cls[i]), t, h, w, crop, block, fmt, _stream()))
    idx = ['yuv'.index(p) for p in planes]
    grid = grid.cpu()[:, :, idx].reshape(lead + (len(planes), rows, cols, 2))
    return grid, (None if cls is None else cls.cpu().reshape(lead + (8, 3)))


def _gain_frame_values(grid, n, peak):
    """grid (..., planes, rows, cols, 2), n (planes,) samples of a frame's region -> three float64 tensors (..., planes)"""
    import numpy as np
    from . import metrics
    e = metrics.gain_frame_sums(grid.numpy())
    return tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in metrics.gain_values(e[..., 0], e[..., 1], np.asarray(n, np.float64), peak))


def gain_frames(a, l, g, crop_border=0, convert_to=None, block=64):
    """Per-frame gain of the test clip a over the compressed input l against the original g on the GPU (include/pnpvcve.h): -> (PSNR_t(a),
    PSNR_t(l), dPSNR_t), three float64 CPU tensors of the leading shape; a, l, g, crop_border and convert_to as psnr_frames.  The sums are
    the device's (gain_sums_frames, one launch for both halves); the fp64 part is metrics.gain_values."""
    grid = gain_sums_frames(a, l, g, crop_border, convert_to, block)[0]
    h, w = (a.shape[-3:-1] if a.dtype == torch.uint8 else a.shape[-2:])
    n = (int(h) - 2 * int(crop_border)) * (int(w) - 2 * int(crop_border)) * (1 if _metric_color(convert_to) == _native.COLOR_Y else 3)
    return tuple(v[..., 0] for v in _gain_frame_values(grid, [n], 255.0))


def gain_yuv(a, l, g, crop_border=0, planes='y', block=64):
    """Per-frame plane gain of three clips of one frame class (gain_sums_yuv): -> (PSNR_t(a), PSNR_t(l), dPSNR_t), three float64 CPU
    tensors lead + (len(planes),) in the order of `planes`; the peak is 255 or 2^d - 1."""
    planes = _metric_planes(planes)
    grid = gain_sums_yuv(a, l, g, crop_border, planes, block)[0]
    h, w = (int(x) for x in a.y.shape[-2:])
    geo = _plane_geometry(yuv_format(a), h, w, int(crop_border))
    n = [(r - 2 * cy) * (c - 2 * cx) for r, c, cy, cx in (geo[p] for p in planes)]
    peak = float((1 << a.bit_depth) - 1) if isinstance(a, _YUV16_CLASSES) else 255.0
    return _gain_frame_values(grid, n, peak)


# ---------------------------------------------------------------- self-ensemble (include/pnpvcve.h, "Self-ensemble")
#: variant ids: bit 0 flips the width axis, bit 1 the height axis, bit 2 transposes, bit 3 reverses time
ENSEMBLE_SPATIAL = tuple(range(8))
ENSEMBLE_SPATIAL_TEMPORAL = tuple(range(16))


def _ensemble_variant(variant):
    if isinstance(variant, bool) or not isinstance(variant, int) or not 0 <= variant < 16:
        raise ValueError(f'variant must be an int in 0..15, got {variant!r}')
    return variant


def _ensemble_clip(x, name, byte_ok=False):
    """one clip tensor of ensemble_view: (t,...) or (1,t,...) -> (the contiguous 4-D tensor, whether it had a batch dimension)"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA/HIP tensor: the PnP-VCVE hot path has no CPU fallback')
    if x.dim() not in (4, 5) or (x.dim() == 5 and x.shape[0] != 1):
        raise ValueError(f'{name} must be one clip: a 4-D tensor, or a 5-D one with n = 1, got {tuple(x.shape)}')
    if x.dtype != torch.float32 and not (byte_ok and x.dtype == torch.uint8):
        raise TypeError(f'{name} must be float32' + (' planes or uint8 (t,h,w,3) frames' if byte_ok else '') + f', got {x.dtype}')
    return x.reshape(x.shape[-4:]).contiguous(), x.dim() == 5


@_on_device_of_first_tensor
def ensemble_view(lq, mvs, par, variant):
    """Variant `variant`'s view of a clip's frames and maps, in one launch (pnp_ensemble_view): lq (t,3,h,w) fp32 or (t,h,w,3) uint8,
    mvs (t,4,h,w), par (t,3,h,w) -- 4-D, or 5-D with n = 1; any of them may be None -> (lq', mvs', par') in the input's rank, None
    where None was given.  The frames and partition planes are moved; the motion vectors are moved, negated and swapped with them."""
    v = _ensemble_variant(variant)
    ins, shape = [], None
    for x, name, c in ((lq, 'lq', 3), (mvs, 'mvs', 4), (par, 'par', 3)):
        if x is None:
            ins.append(None)
            continue
        x4, lead = _ensemble_clip(x, name, byte_ok=name == 'lq')
        if x4.dtype == torch.uint8:
            if x4.shape[-1] != 3:
                raise ValueError(f'uint8 frames must be (t,h,w,3), got {tuple(x4.shape)}')
            thw = (x4.shape[0], x4.shape[1], x4.shape[2])
        else:
            if x4.shape[1] != c:
                raise ValueError(f'{name} must have {c} channels, got {tuple(x4.shape)}')
            thw = (x4.shape[0], x4.shape[2], x4.shape[3])
        if shape is None:
            shape = thw
        elif thw != shape:
            raise ValueError(f'lq, mvs and par must agree in (t, h, w): {thw} against {shape}')
        ins.append((x4, lead))
    if shape is None:
        return None, None, None
    t, h, w = shape
    ho, wo = (w, h) if v & 4 else (h, w)
    outs = []
    for item in ins:
        if item is None:
            outs.append(None)
        elif item[0].dtype == torch.uint8:
            outs.append(torch.empty((t, ho, wo, 3), device=item[0].device, dtype=torch.uint8))
        else:
            outs.append(torch.empty((t, item[0].shape[1], ho, wo), device=item[0].device, dtype=torch.float32))
    fmt = _native.FRAMES_U8_HWC if (ins[0] is not None and ins[0][0].dtype == torch.uint8) else _native.FRAMES_F32_NCHW
    P = lambda x: _ptr(x[0] if isinstance(x, tuple) else x)      # noqa: E731
    _native.check(_native.lib().pnp_ensemble_view(P(ins[0]), P(ins[1]), P(ins[2]), P(outs[0]), P(outs[1]), P(outs[2]), fmt, t, h, w, v,
                                                  _stream()), 'pnp_ensemble_view')
    return tuple(None if o is None else (o[None] if item[1] else o) for o, item in zip(outs, ins))


def ensemble_side(QPs, slices, base_QPs, variant):
    """Variant `variant`'s (..., t, 1, 1, 1) side tensors: reversed in time under bit 3, untouched otherwise (plain torch; None stays None)."""
    v = _ensemble_variant(variant)
    return tuple(x if (x is None or not v & 8) else x.flip(-4) for x in (QPs, slices, base_QPs))


@_on_device_of_first_tensor
def ensemble_accumulate(acc, x, variant, first, scale=1.0):
    """In place (pnp_ensemble_accumulate_f32): acc (t,c,H,W), original orientation and frame order, takes variant `variant`'s output
    x (t,c,H',W') through the variant's inverse -- acc = x if first else acc + x, then times `scale` unless it is 1.  4-D tensors, or
    5-D with n = 1.  Returns acc."""
    v = _ensemble_variant(variant)
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or not acc.is_contiguous() or acc.dtype != torch.float32:
        raise RuntimeError('acc must be a contiguous float32 CUDA/HIP tensor (it is written in place)')
    x4, _ = _ensemble_clip(x, 'x')
    a4 = acc.reshape(acc.shape[-4:]) if acc.dim() in (4, 5) and (acc.dim() == 4 or acc.shape[0] == 1) else None
    if a4 is None:
        raise ValueError(f'acc must be one clip: a 4-D tensor, or a 5-D one with n = 1, got {tuple(acc.shape)}')
    t, c, H, W = a4.shape
    if tuple(x4.shape) != ((t, c, W, H) if v & 4 else (t, c, H, W)):
        raise ValueError(f'x is {tuple(x4.shape)}, acc {tuple(a4.shape)}: not variant {v}\'s output of this clip')
    scale = float(scale)
    if not (scale > 0.0) or scale == float('inf'):
        raise ValueError(f'scale must be finite and > 0, got {scale!r}')
    _native.check(_native.lib().pnp_ensemble_accumulate_f32(_ptr(x4), _ptr(a4), t, c, H, W, v, int(bool(first)), scale, _stream()),
                  'pnp_ensemble_accumulate_f32')
    return acc
