"""PyTorch custom-op registration of the hot path (`torch.ops.pnpvcve.*`).

north_star asks for the HIP kernels to be "invoked from Python via PyTorch-ROCm custom ops": these are thin
`torch.library` registrations over the C ABI (include/pnpvcve.h) -- torch carries the tensors, the device memory and
the current stream; the arithmetic is libpnpvcve_hip.so.  Each op has a fake (meta) implementation so that shape
propagation / tracing works without a GPU; there is no CPU implementation (a CPU tensor raises, like the rest of the
package).

    torch.ops.pnpvcve.flow_warp(x, flow)                        mmedit/models/common/flow_warp.py:6-50
    torch.ops.pnpvcve.mv_warp(feat_hwc, flow_x, flow_y)         iconvsr_mv.py:17-18 in the fused path's layout
    torch.ops.pnpvcve.psnr_sse(a, b, crop_border)               core/evaluation/metrics.py:200-215 statistic
    torch.ops.pnpvcve.generator_forward(handle, lrs, mvs, par, side)   iconvsr_ipb_par.py:44-149
    torch.ops.pnpvcve.generator_forward_clips(handle, lrs[], mvs[], par[], side, out_mask)
                                                                the same forward over clips given one by one (fp32 planes or uint8 HWC
                                                                frames in; fp32 planes and / or uint8 HWC frames out, out_mask 1 | 2 | 3)
    torch.ops.pnpvcve.frames_from_rgb8(u8)                      RescaleToZeroOne + HWC->CHW of decoded frames
    torch.ops.pnpvcve.generator_forward_clips_yuv(handle, y[], cb[], cr[], mvs[], par[], side, standard, out_mask, layout)
                                                                the same forward on 8-bit 4:2:0 plane views (NV12 / NV21 / I420); fp32
                                                                planes, uint8 HWC frames and / or packed 4:2:0 buffers out (out_mask 1..7)
    torch.ops.pnpvcve.generator_forward_clips_yuv16(handle, y[], cb[], cr[], bit_depth, msb_aligned, mvs[], par[], side, standard, out_mask, layout)
                                                                the same on 10 / 12-bit plane views (16-bit words); layout indexes
                                                                sorted(ops.YUV16_LAYOUTS)
    torch.ops.pnpvcve.frames_from_yuv420(y, cb, cr, standard)   4:2:0 planes -> fp32 RGB planes (include/pnpvcve.h states the arithmetic)
                                                                `standard` of the three 4:2:0 ops: PNP_YUV_* (0..3), or with a chroma mode
                                                                PNP_YUV_CODE(standard, chroma) = standard | mode << 8 (ops._yuv_code)

    torch.ops.pnpvcve.conv3x3(srcs, packed_w, bias, gamma, packed_w1x1, par, residual, act)
                                                                basicvsr_net.py:484, sr_backbone_utils.py:304-333 halves, iconvsr.py:365
    torch.ops.pnpvcve.expert_mix(experts, attention)            Dynamic_conv2d_se.forward's mm(attention, weight), sr_backbone_utils.py:198-199
    torch.ops.pnpvcve.bae_block(x, w2, b2, gamma, w1x1, par, w1, b1)   ResidualBlockNoBNDynamic_drt.forward, :304-333
    torch.ops.pnpvcve.pixel_shuffle_conv(x, packed, act)        PixelShufflePack.forward, common/upsample.py:40-51

`handle` is the integer id under which a generator module registered itself (register_generator); `side` is the CPU
float tensor (3, n, t) = (slices, QPs, base_QPs).  generator.forward() goes through this op.
"""
import weakref

import torch

from . import ops

_GENERATORS = weakref.WeakValueDictionary()
_NEXT_ID = [1]


def register_generator(module):
    hid = _NEXT_ID[0]
    _NEXT_ID[0] += 1
    _GENERATORS[hid] = module
    return hid


@torch.library.custom_op('pnpvcve::flow_warp', mutates_args=())
def flow_warp(x: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    return ops.flow_warp(x, flow)


@flow_warp.register_fake
def _(x, flow):
    return torch.empty_like(x)


@torch.library.custom_op('pnpvcve::mv_warp', mutates_args=())
def mv_warp(feat: torch.Tensor, flow_x: torch.Tensor, flow_y: torch.Tensor) -> torch.Tensor:
    return ops.mv_warp_nhwc(feat, flow_x, flow_y)


@mv_warp.register_fake
def _(feat, flow_x, flow_y):
    return torch.empty_like(feat)


@torch.library.custom_op('pnpvcve::psnr_sse', mutates_args=())
def psnr_sse(a: torch.Tensor, b: torch.Tensor, crop_border: int) -> torch.Tensor:
    """per-frame PSNR (float64, CPU) of the uint8-rounded frames; a, b (..., c, h, w)"""
    return ops.psnr_frames(a, b, crop_border)


@psnr_sse.register_fake
def _(a, b, crop_border):
    return torch.empty(a.shape[:-3], dtype=torch.float64)


@torch.library.custom_op('pnpvcve::generator_forward', mutates_args=())
def generator_forward(handle: int, lrs: torch.Tensor, mvs: torch.Tensor, par: torch.Tensor,
                      side: torch.Tensor) -> torch.Tensor:
    m = _GENERATORS.get(handle)
    if m is None:
        raise RuntimeError(f'pnpvcve::generator_forward: unknown generator handle {handle}')
    return m._forward_native(lrs, mvs, par, side)


@generator_forward.register_fake
def _(handle, lrs, mvs, par, side):
    m = _GENERATORS.get(handle)
    s = 4 if (m is not None and m.vsr) else 1
    n, t, _, h, w = lrs.shape
    return lrs.new_empty((n, t, 3, h * s, w * s))


@torch.library.custom_op('pnpvcve::frames_from_rgb8', mutates_args=())
def frames_from_rgb8(u8: torch.Tensor) -> torch.Tensor:
    return ops.frames_from_rgb8(u8)


@frames_from_rgb8.register_fake
def _(u8):
    return u8.new_empty(tuple(u8.shape[:-3]) + (3,) + tuple(u8.shape[-3:-1]), dtype=torch.float32)


@torch.library.custom_op('pnpvcve::generator_forward_clips', mutates_args=())
def generator_forward_clips(handle: int, lrs: list[torch.Tensor], mvs: list[torch.Tensor], par: list[torch.Tensor],
                            side: torch.Tensor, out_mask: int) -> list[torch.Tensor]:
    """one clip per list entry: lrs[i] (t,3,h,w) fp32 or (t,h,w,3) uint8; -> per clip the fp32 planes (out_mask & 1), then the uint8
    frames (out_mask & 2): len(lrs) tensors for out_mask 1 or 2, the fp32 ones followed by the uint8 ones for out_mask 3"""
    m = _GENERATORS.get(handle)
    if m is None:
        raise RuntimeError(f'pnpvcve::generator_forward_clips: unknown generator handle {handle}')
    return m._forward_clips_native(list(lrs), list(mvs), list(par), side, int(out_mask))


@generator_forward_clips.register_fake
def _(handle, lrs, mvs, par, side, out_mask):
    m = _GENERATORS.get(handle)
    s = 4 if (m is not None and m.vsr) else 1
    outs = []
    for bit, dt in ((1, torch.float32), (2, torch.uint8)):
        for x in lrs:
            if not out_mask & bit:
                continue
            t, (h, w) = x.shape[0], (x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:4])
            outs.append(x.new_empty((t, 3, h * s, w * s) if bit == 1 else (t, h * s, w * s, 3), dtype=dt))
    return outs


_YUV_ROWS2 = (3, 4, 6)      # twice the rows of a packed buffer per luma row, by the chroma format in bits 12..13 of `standard`


@torch.library.custom_op('pnpvcve::frames_from_yuv420', mutates_args=())
def frames_from_yuv420(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, standard: int) -> torch.Tensor:
    """uint8 views y (...,h,w), cb / cr (...,h/2,w/2) with 3 or 4 dimensions -> (...,3,h,w) fp32 RGB; standard = PNP_YUV_*, or
    PNP_YUV_CODE(standard, chroma) (ops._yuv_code)"""
    std, chroma = ops._yuv_code_split(standard)
    return ops.frames_from_yuv420(ops.Yuv420Frames(y, cb, cr), std, chroma)


@frames_from_yuv420.register_fake
def _(y, cb, cr, standard):
    return y.new_empty(tuple(y.shape[:-2]) + (3,) + tuple(y.shape[-2:]), dtype=torch.float32)


@torch.library.custom_op('pnpvcve::generator_forward_clips_yuv', mutates_args=())
def generator_forward_clips_yuv(handle: int, y: list[torch.Tensor], cb: list[torch.Tensor], cr: list[torch.Tensor], mvs: list[torch.Tensor],
                                par: list[torch.Tensor], side: torch.Tensor, standard: int, out_mask: int, layout: int) -> list[torch.Tensor]:
    """one clip per list entry: y[i] (t,h,w), cb[i] / cr[i] (t,h/2,w/2) uint8 views; -> per clip the fp32 planes (out_mask & 1), then
    the uint8 frames (& 2), then the packed (t,3H/2,W) 4:2:0 buffers (& 4) in layout 0 'nv12' | 2 'i420' (ops.YUV_LAYOUTS; -1 = none)"""
    m = _GENERATORS.get(handle)
    if m is None:
        raise RuntimeError(f'pnpvcve::generator_forward_clips_yuv: unknown generator handle {handle}')
    return m._forward_clips_yuv_native(list(y), list(cb), list(cr), list(mvs), list(par), side, int(standard), int(out_mask),
                                       ops._yuv_layout_of_index(layout, False))


@generator_forward_clips_yuv.register_fake
def _(handle, y, cb, cr, mvs, par, side, standard, out_mask, layout):
    m = _GENERATORS.get(handle)
    s = 4 if (m is not None and m.vsr) else 1
    outs = []
    for bit in (1, 2, 4):
        for x in y:
            if not out_mask & bit:
                continue
            t, h, w = x.shape
            shape = {1: (t, 3, h * s, w * s), 2: (t, h * s, w * s, 3), 4: (t, h * s * _YUV_ROWS2[(standard >> 12) & 3] // 2, w * s)}[bit]
            outs.append(x.new_empty(shape, dtype=torch.float32 if bit == 1 else torch.uint8))
    return outs


@torch.library.custom_op('pnpvcve::conv3x3', mutates_args=())
def conv3x3(srcs: list[torch.Tensor], packed_w: list[torch.Tensor], bias: torch.Tensor | None, gamma: torch.Tensor | None,
            packed_w1x1: torch.Tensor | None, par: torch.Tensor | None, residual: torch.Tensor | None,
            act: int) -> torch.Tensor:
    return ops.conv3x3(srcs, packed_w, bias=bias, gamma=gamma, packed_w1x1=packed_w1x1, par=par, residual=residual, act=act)


@conv3x3.register_fake
def _(srcs, packed_w, bias, gamma, packed_w1x1, par, residual, act):
    h, w = srcs[0].shape[:2]
    return srcs[0].new_empty((h, w, 64))


@torch.library.custom_op('pnpvcve::expert_mix', mutates_args=())
def expert_mix(experts: torch.Tensor, attention: torch.Tensor) -> torch.Tensor:
    """(E,64,64,3,3) expert bank + (E,) attention -> the packed image of sum_e attention[e] * experts[e]"""
    return ops.pack_conv3x3(experts, ew=attention)


@expert_mix.register_fake
def _(experts, attention):
    return experts.new_empty((9 * 4096,))


@torch.library.custom_op('pnpvcve::bae_block', mutates_args=())
def bae_block(x: torch.Tensor, w2_packed: torch.Tensor, b2: torch.Tensor | None, gamma: torch.Tensor | None,
              w1x1_packed: torch.Tensor | None, par: torch.Tensor | None, w1_packed: torch.Tensor,
              b1: torch.Tensor | None) -> torch.Tensor:
    return ops.bae_block(x, w2_packed, b2, gamma, w1x1_packed, par, w1_packed, b1)


@bae_block.register_fake
def _(x, w2_packed, b2, gamma, w1x1_packed, par, w1_packed, b1):
    return torch.empty_like(x)


@torch.library.custom_op('pnpvcve::pixel_shuffle_conv', mutates_args=())
def pixel_shuffle_conv(x: torch.Tensor, packed: torch.Tensor, act: int) -> torch.Tensor:
    return ops.pixel_shuffle_conv(x, packed, act)


@pixel_shuffle_conv.register_fake
def _(x, packed, act):
    h, w, c = x.shape
    return x.new_empty((2 * h, 2 * w, c))


@torch.library.custom_op('pnpvcve::generator_forward_clips_yuv16', mutates_args=())
def generator_forward_clips_yuv16(handle: int, y: list[torch.Tensor], cb: list[torch.Tensor], cr: list[torch.Tensor], bit_depth: int,
                                  msb_aligned: bool, mvs: list[torch.Tensor], par: list[torch.Tensor], side: torch.Tensor, standard: int,
                                  out_mask: int, layout: int) -> list[torch.Tensor]:
    """generator_forward_clips_yuv on views of 16-bit words (int16 / uint16) holding bit_depth-bit samples in the low (msb_aligned False)
    or high bits; the packed (t,3H/2,W) 4:2:0 buffers (& 4) are 16-bit words of y's dtype in layout sorted(ops.YUV16_LAYOUTS)[layout]"""
    m = _GENERATORS.get(handle)
    if m is None:
        raise RuntimeError(f'pnpvcve::generator_forward_clips_yuv16: unknown generator handle {handle}')
    return m._forward_clips_yuv_native(list(y), list(cb), list(cr), list(mvs), list(par), side, int(standard), int(out_mask),
                                       ops._yuv_layout_of_index(layout, True), int(bit_depth), bool(msb_aligned))


@generator_forward_clips_yuv16.register_fake
def _(handle, y, cb, cr, bit_depth, msb_aligned, mvs, par, side, standard, out_mask, layout):
    m = _GENERATORS.get(handle)
    s = 4 if (m is not None and m.vsr) else 1
    outs = []
    for bit in (1, 2, 4):
        for x in y:
            if not out_mask & bit:
                continue
            t, h, w = x.shape
            shape = {1: (t, 3, h * s, w * s), 2: (t, h * s, w * s, 3), 4: (t, h * s * _YUV_ROWS2[(standard >> 12) & 3] // 2, w * s)}[bit]
            outs.append(x.new_empty(shape, dtype={1: torch.float32, 2: torch.uint8, 4: x.dtype}[bit]))
    return outs
