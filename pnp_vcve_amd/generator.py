"""The generator behind the reference's registry name.

Same constructor kwargs, forward signature, state-dict keys and error behaviour as
/root/reference/mmedit/models/backbones/sr_backbones/iconvsr_ipb_par.py:16-149
(class IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par), but the forward is a
single call into libpnpvcve_hip.so (pnp_generator_forward), which schedules the whole clip
as hand-written HIP kernels.  The nn.Module only holds the parameters in the reference's
layout so that released checkpoints load unchanged.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _native, ops
from .registry import BACKBONES

_DEFORM = {'vos': 0, 'basic': 1, 'fvc': 2}
_FLOW_INTER = {'bilinear': 0, 'nearest': 1}        # flow_warp.py:18
_BLOCKTYPES = {'drt': 0, 'drt_woqp': 1}            # basicvsr_net.py:487-503


def _kaiming_normal_fan_in(t, scale):
    nn.init.kaiming_normal_(t, a=0, mode='fan_in', nonlinearity='relu')
    t.data.mul_(scale)


@BACKBONES.register_module()
class IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par(nn.Module):
    def __init__(self, mid_channels=64, num_blocks=30, num_experts=10, num_group=1, expert_softmax=False,
                 use_base_qp=False, with_bias=False, with_se=False, with_par=False, init_weight=False,
                 one_layer=False, small_sft=False, blocktype='default', channel_first=False, drconv=False,
                 sparse_val=False, vsr=False, align_key=False,
                 # parents: iconvsr_ipb.py:16, iconvsr.py:346-351
                 with_cat=False, deform='vos', max_residue_magnitude=10, flow_inter='bilinear',
                 keyframe_stride=5, padding=2,
                 # this build's own switch (no reference counterpart): see the any_size property
                 any_size=False):
        super().__init__()
        if deform == 'stdf':
            raise TypeError('Not implemented yet')          # iconvsr_ipb.py:25-26
        if deform not in _DEFORM:
            raise TypeError('Not such DCN type')            # iconvsr_ipb.py:27-28
        if blocktype not in _BLOCKTYPES:
            # basicvsr_net.py:487-503 builds self.main for 'drt' and 'drt_woqp' only (any other value: AttributeError at forward)
            raise NotImplementedError(f"blocktype={blocktype!r}: 'drt' | 'drt_woqp' (basicvsr_net.py:487-503)")
        if blocktype == 'drt_woqp' and not one_layer:
            # sr_backbone_utils.py:376-384 calls conv1 / conv2 on the bare map; a Dynamic_conv2d_se indexes it with 'x' and raises
            raise NotImplementedError("blocktype='drt_woqp' runs only with one_layer=True (the reference raises in its first forward)")
        if mid_channels != 64:
            raise NotImplementedError('only mid_channels=64 (every shipped config; the kernels are built for 64-channel maps)')
        if not isinstance(num_group, int) or num_group < 1 or 64 % num_group:
            raise ValueError('in_channels must be divisible by groups')        # nn.Conv2d's own check
        if sparse_val and num_group != 1:
            raise NotImplementedError('sparse_val with num_group > 1: the reference multiplies a (64, 64/groups) weight with 64-channel '
                                      'columns and raises (sr_backbone_utils.py:295)')
        if flow_inter not in _FLOW_INTER:
            raise NotImplementedError("flow_inter: 'bilinear' | 'nearest' (flow_warp.py:18)")
        if with_bias:
            assert use_base_qp is True or use_base_qp == 1     # iconvsr_ipb_par.py:27
        self.mid_channels = mid_channels
        self.padding = padding
        self.keyframe_stride = keyframe_stride
        self.flow_inter = flow_inter
        self.with_cat, self.use_base_qp, self.with_bias = with_cat, use_base_qp, with_bias
        self.with_par, self.vsr, self.align_key = with_par, vsr, align_key
        self.sparse_val = bool(sparse_val)
        self.is_mirror_extended = False
        self._cfg = _native.GeneratorCfg(
            mid_channels=mid_channels, num_blocks=num_blocks, num_experts=num_experts, with_cat=int(with_cat),
            use_base_qp=int(use_base_qp), expert_softmax=int(expert_softmax), with_bias=int(with_bias),
            with_se=int(with_se), one_layer=int(one_layer), channel_first=int(channel_first),
            align_key=int(align_key), vsr=int(vsr), deform=_DEFORM[deform], sparse_val=int(bool(sparse_val)),
            num_group=int(num_group), flow_inter=_FLOW_INTER[flow_inter], blocktype=_BLOCKTYPES[blocktype])
        self._handle = ctypes.c_void_p()
        L = _native.lib()
        _native.check(L.pnp_generator_create(ctypes.byref(self._cfg), ctypes.byref(self._handle)),
                      'pnp_generator_create')
        # parameters, named and shaped as the native library's schema says (== reference state-dict)
        self._schema = []
        for i in range(L.pnp_generator_num_params(self._handle)):
            name = L.pnp_generator_param_name(self._handle, i).decode()
            shape = tuple(int(L.pnp_generator_param_dim(self._handle, i, d))
                          for d in range(L.pnp_generator_param_ndim(self._handle, i)))
            off = int(L.pnp_generator_param_offset(self._handle, i))
            self._schema.append((name, shape, off))
            self._register(name, nn.Parameter(torch.zeros(shape)))
        self._flat_floats = int(L.pnp_generator_flat_floats(self._handle))
        self._packed_floats = int(L.pnp_generator_packed_floats(self._handle))
        self._init_like_reference(init_weight)
        self._flat = self._packed = None
        self._pack_key = None
        self._workspace = {}
        self._graphs = {}
        self._profiling = False
        from . import torch_ops
        self._op_handle = torch_ops.register_generator(self)       # id under which torch.ops.pnpvcve finds this module
        if any_size:
            self.any_size = True

    # ---------------------------------------------------------------- precision
    @property
    def fp16_enabled(self):
        """mmcv's fp16 switch (wrap_fp16_model sets it; basic_restorer.py:64 @auto_fp16 reads it).  True selects
        fp16 MFMA operands for the 64-channel convs (pnp_generator_set_precision); default False = exact fp32."""
        return int(_native.lib().pnp_generator_get_precision(self._handle)) == 1

    @fp16_enabled.setter
    def fp16_enabled(self, value):
        self.precision = 'fp16' if value else 'fp32'

    _PRECISIONS = ('fp32', 'fp16', 'f16x3')      # PNP_PREC_F32 / F16 / F16X3

    @property
    def precision(self):
        """'fp32' (default, exact fp32 MFMA) | 'fp16' (mmcv's fp16 switch: fp16 MFMA operands) | 'f16x3' (split fp16: every
        operand of the 64-channel convs carried as two fp16 numbers, three MFMAs per product; fp32-level results -- inside the
        1e-3 parity gate -- from the fp16 matrix pipe).  include/pnpvcve.h PNP_PREC_*."""
        return self._PRECISIONS[int(_native.lib().pnp_generator_get_precision(self._handle))]

    @precision.setter
    def precision(self, value):
        if value not in self._PRECISIONS:
            raise ValueError(f'precision must be one of {self._PRECISIONS}, got {value!r}')
        L = _native.lib()
        _native.check(L.pnp_generator_set_precision(self._handle, self._PRECISIONS.index(value)), 'pnp_generator_set_precision')
        self._packed_floats = int(L.pnp_generator_packed_floats(self._handle))
        self._flat = self._packed = None        # images and workspace are sized per precision
        self._pack_key = None
        self._workspace = {}
        self._graphs = {}

    def set_option(self, option, value):
        """pnp_generator_set_option: A/B switches of the native scheduler (_native.OPT_*); per-generator state."""
        # PNP_OPT_WINOGRAD takes 0 / 1 / 2 (off / large frames / every frame size); the others are booleans
        v = int(value) if int(option) == _native.OPT_WINOGRAD else int(bool(value))
        _native.check(_native.lib().pnp_generator_set_option(self._handle, int(option), v),
                      'pnp_generator_set_option')
        self._graphs = {}


    def get_option(self, option):
        return int(_native.lib().pnp_generator_get_option(self._handle, int(option)))

    # ---------------------------------------------------------------- bounded memory for long clips
    @property
    def max_resident_features(self):
        """None (default): one 64-channel feature map per frame, as in the reference.  An int k bounds the frame feature maps the two
        sweeps hold (pnp_generator_set_max_resident): the forward sweep then recomputes segments of the backward features from
        checkpoints -- bit-identical output, a workspace of k maps instead of t, at the cost of the recomputed frames.  k >= t (or
        None) runs the unbounded schedule; a k below min_resident_features(t) raises ValueError at forward time."""
        k = int(_native.lib().pnp_generator_get_max_resident(self._handle))
        return None if k == 0 else k

    @max_resident_features.setter
    def max_resident_features(self, value):
        if value is not None and (isinstance(value, bool) or not isinstance(value, int) or value < 1):
            raise ValueError(f'max_resident_features must be None or a positive int, got {value!r}')
        _native.check(_native.lib().pnp_generator_set_max_resident(self._handle, 0 if value is None else int(value)),
                      'pnp_generator_set_max_resident')
        self._workspace = {}
        self._graphs = {}

    # ---------------------------------------------------------------- row-band chains
    @property
    def band_split(self):
        """1 (default): on frames that qualify (fp32, Winograd tile kernels, one clip in flight, 720p and up) every conv of a branch
        runs as two launches over complementary tile-row bands on two streams, so that one band's launch tail is filled by the
        other's next conv (pnp_generator_set_band_split, include/pnpvcve.h; bit-identical output).  0: one launch per conv.
        k >= 2: as 1 with the chain's first boundary at tile row k (a tuning aid)."""
        return int(_native.lib().pnp_generator_get_band_split(self._handle))

    @band_split.setter
    def band_split(self, value):
        if isinstance(value, bool):
            value = int(value)
        if not isinstance(value, int) or value < 0:
            raise ValueError(f'band_split must be an int >= 0, got {value!r}')
        _native.check(_native.lib().pnp_generator_set_band_split(self._handle, value), 'pnp_generator_set_band_split')
        self._graphs = {}

    # ---------------------------------------------------------------- frames that are no multiple of 4
    @property
    def any_size(self):
        """False (default): a frame whose height or width is no multiple of 4 raises ValueError, as the reference does (its
        spatial_padding pads lrs alone and flow_warp then refuses the unpadded flow).  True: such frames run
        (pnp_generator_set_any_size, include/pnpvcve.h) -- the same formulas on the h x w grid as given, no padding and no crop; the
        output is (n,t,3,h,w), or (n,t,3,4h,4w) with vsr.  Multiples of 4 run exactly as with False.  h, w >= 64 holds either way;
        deform='basic' | 'fvc' is refused with the switch on.  Also a constructor kwarg (model.generator.any_size=True in a config)."""
        return bool(_native.lib().pnp_generator_get_any_size(self._handle))

    @any_size.setter
    def any_size(self, value):
        _native.check(_native.lib().pnp_generator_set_any_size(self._handle, int(bool(value))), 'pnp_generator_set_any_size')
        self._graphs = {}

    def min_resident_features(self, t):
        """The smallest max_resident_features the bounded schedule accepts for a clip of t frames (pnp_generator_min_resident)."""
        if int(t) < 1:
            raise ValueError(f't must be >= 1, got {t!r}')
        return int(_native.lib().pnp_generator_min_resident(self._handle, int(t)))

    def _check_resident(self, t):
        k = self.max_resident_features
        if k is not None and k < t and k < self.min_resident_features(t):
            raise ValueError(f'max_resident_features={k} is below the minimum {self.min_resident_features(t)} for a clip of {t} frames')

    # ---------------------------------------------------------------- parameters
    def _register(self, dotted, param):
        mod = self
        parts = dotted.split('.')
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        mod.register_parameter(parts[-1], param)

    def _init_like_reference(self, init_weight):
        """SURVEY.md Appendix B (sr_backbone_utils.py:41-57,152-164,291-292; torch defaults)."""
        for name, p in self.named_parameters():
            with torch.no_grad():
                in_block = '.main.' in name
                if p.dim() == 5:                                        # Dynamic_conv2d experts (E,64,64,3,3)
                    if init_weight:
                        for k in range(p.shape[0]):
                            nn.init.kaiming_uniform_(p[k])
                    else:
                        p.normal_()
                elif in_block and name.endswith('.bias'):               # expert biases (E,64) and conv1.bias
                    p.zero_()
                elif in_block:                                          # conv1 / 1x1: default_init_weights(m, 0.1)
                    _kaiming_normal_fan_in(p, 0.1)
                elif 'upsample' in name:                                # PixelShufflePack: default_init_weights(self, 1)
                    p.zero_() if name.endswith('.bias') else _kaiming_normal_fan_in(p, 1.0)
                elif name.endswith('.bias'):                            # torch default conv / linear bias
                    ref = dict(self.named_parameters())[name[:-4] + 'weight']
                    bound = 1.0 / math.sqrt(ref[0].numel())
                    p.uniform_(-bound, bound)
                else:                                                   # torch default conv / linear weight
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))

    def init_weights(self, pretrained=None, strict=True):
        """iconvsr.py:510-523."""
        if isinstance(pretrained, str):
            from .checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=strict)
        elif pretrained is not None:
            raise TypeError(f'"pretrained" must be a str or None. But received {type(pretrained)}.')

    def invalidate_packed(self):
        """Drop the native weight images (flat / packed / fp16 mirrors); the next forward() re-packs them.
        The cache is keyed on each parameter's (data_ptr, _version), which in-place writes through `param.data`
        (EMA helpers, weight surgery, some optimizers) do NOT change -- call this after such writes.
        load_state_dict(), .to()/.cuda()/.half() and friends call it themselves."""
        self._flat = self._packed = None
        self._pack_key = None
        self._graphs = {}

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_packed()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def _ensure_packed(self, device):
        params = dict(self.named_parameters())
        key = (str(device), self._packed_floats) + tuple((p.data_ptr(), p._version) for p in params.values())
        if self._pack_key == key:
            return
        flat = torch.zeros(self._flat_floats, device=device, dtype=torch.float32)
        for name, shape, off in self._schema:
            p = params[name]
            if not p.is_cuda:
                raise RuntimeError('generator parameters must be on the GPU: call .cuda() first '
                                   '(no CPU fallback exists for this path)')
            flat[off:off + p.numel()].copy_(p.detach().reshape(-1))
        packed = torch.zeros(self._packed_floats, device=device, dtype=torch.float32)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.check(_native.lib().pnp_generator_pack(self._handle, ctypes.c_void_p(flat.data_ptr()),
                                                       ctypes.c_void_p(packed.data_ptr()), st), 'pnp_generator_pack')
        self._flat, self._packed, self._pack_key = flat, packed, key
        self._graphs = {}               # captured launches point into the previous buffers

    #: frames below this many pixels cannot fill the chip alone: samples of a batch then run concurrently
    CONCURRENT_BELOW_PIXELS = 512 * 512
    MAX_CONTEXTS = 8                       # PNP_MAX_CONTEXTS (r02, 128x128 fp32, 8 clips: 2 ctx 2130, 4 ctx 2022, 8 ctx 2213 frames/s)
    #: a large frame fills the chip by itself, but every persistent conv launch ends with a partial round (720p: 7200 tiles on
    #: 512 strips = 14.06 rounds, the 15th on 32 blocks) and a dispatch gap: two samples interleaved on two streams fill each
    #: other's tails -- measured +4.9 % fp32 / +4.5 % split fp16 / +5.2 % fp16 at 720p, bit-identical (tools/tail_fill_probe.py);
    #: more than two gain nothing and cost a workspace each
    LARGE_FRAME_CONTEXTS = 2

    def _contexts(self, n, h, w):
        return min(n, self.LARGE_FRAME_CONTEXTS if h * w >= self.CONCURRENT_BELOW_PIXELS else self.MAX_CONTEXTS)

    def _workspace_bytes(self, t, h, w, fmt=_native.FRAMES_F32_NCHW, mask=_native.OUT_F32):
        """bytes of one workspace context for a boundary (pnp_generator_workspace_bytes / _io: equal at the fp32 boundary)"""
        L = _native.lib()
        if (fmt, mask) == (_native.FRAMES_F32_NCHW, _native.OUT_F32):
            return int(L.pnp_generator_workspace_bytes(self._handle, t, h, w))
        if fmt == 'yuv':        # the 4:2:0 boundary (pnp_generator_forward_clips_yuv)
            return int(L.pnp_generator_workspace_bytes_yuv(self._handle, t, h, w, mask))
        return int(L.pnp_generator_workspace_bytes_io(self._handle, t, h, w, fmt, mask))

    def _get_workspace(self, n, t, h, w, device, fmt=_native.FRAMES_F32_NCHW, mask=_native.OUT_F32):
        ctx = self._contexts(n, h, w)
        k = (ctx, t, h, w, str(device), self.max_resident_features, fmt, mask)
        ws = self._workspace.get(k)
        if ws is None:
            nbytes = self._workspace_bytes(t, h, w, fmt, mask) * ctx
            self._workspace.clear()        # keep one shape resident
            ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
            self._workspace[k] = ws
        return ws

    # ---------------------------------------------------------------- forward
    @staticmethod
    def _out_mask(out_dtype):
        if out_dtype is None or out_dtype == torch.float32:
            return _native.OUT_F32
        if out_dtype == torch.uint8:
            return _native.OUT_U8
        if isinstance(out_dtype, str) and out_dtype == 'both':
            return _native.OUT_F32 | _native.OUT_U8
        raise ValueError(f"out_dtype must be None, torch.float32, torch.uint8 or 'both', got {out_dtype!r}")

    def forward(self, lrs, QPs=None, slices=None, mvs=None, base_QPs=None, par_map=None, out_dtype=None, yuv_standard='bt601-limited',
                chroma='replicate'):
        """iconvsr_ipb_par.py:44-149.  lrs (n,t,3,h,w); QPs/slices/base_QPs (n,t,1,1,1);
        mvs (n,t,4,h,w); par_map (n,t,3,h,w).  Returns (n,t,3,h,w) (x4 spatial when vsr).

        Byte frames: a uint8 `lrs` is the decoder's layout (n,t,h,w,3), RGB, byte v standing for float32(v) / float32(255) -- the
        result is bit-identical to forward(ops.frames_from_rgb8(lrs), ...), without the fp32 clip.  out_dtype: None / torch.float32
        (the fp32 planes above) | torch.uint8 ((n,t,H,W,3) display bytes, ops.frames_to_rgb8's arithmetic on the same fp32 values) |
        'both' (the pair (fp32, uint8)).

        4:2:0 frames: an ops.Yuv420Frames `lrs` is the decoder's planes where they lie (NV12 / NV21 / I420 views, any pitch) in the
        colour standard `yuv_standard` ('bt601-limited' | 'bt601-full' | 'bt709-limited' | 'bt709-full') -- bit-identical to
        forward(ops.frames_from_yuv420(lrs, yuv_standard), ...), without the fp32 clip.  out_dtype then also takes 'nv12' / 'i420'
        (a packed uint8 (n,t,3H/2,W) buffer, ops.frames_to_yuv420's arithmetic on the same fp32 values) and a tuple or list of
        dtypes (several outputs, returned as a tuple in that order).  chroma: 'replicate' (the default: replicated on the way in, box
        mean on the way out) | 'center' | 'left' (H.264 / HEVC / VVC streams) | 'topleft' (BT.2020 / UHD), the chroma modes of
        include/pnpvcve.h -- where the chroma samples lie, bilinear on the way in and the matching filter on the way out; the two
        identities above hold with the same `chroma` passed to ops.frames_from_yuv420 / ops.frames_to_yuv420.

        10 / 12-bit 4:2:0 frames: an ops.Yuv420Frames16 `lrs` (P010 / P012 / yuv420p10le / yuv420p12le views) -- bit-identical to
        forward(ops.frames_from_yuv420p16(lrs, yuv_standard), ...).  out_dtype then also takes 'p010' | 'p012' | 'yuv420p10le' |
        'yuv420p12le' (a packed (n,t,3H/2,W) buffer of 16-bit words of lrs' dtype, ops.frames_to_yuv420p16's arithmetic; its depth and
        container need not be the input's) beside 'nv12' / 'i420'.  16-bit planes out of 8-bit planes in are refused."""
        if ops.is_yuv(lrs):
            return self._forward_yuv(lrs, QPs, slices, mvs, base_QPs, par_map, out_dtype, yuv_standard, chroma)
        if not lrs.is_cuda:
            raise RuntimeError('PnP-VCVE generator: inputs must be CUDA/HIP tensors; this build has no CPU path '
                               '(the CPU restatement under oracle/ is test infrastructure only)')
        mask = self._out_mask(out_dtype)
        byte_in = lrs.dtype == torch.uint8
        if byte_in:
            if lrs.dim() != 5 or lrs.shape[-1] != 3:
                raise ValueError(f'uint8 frames must be (n,t,h,w,3) -- the decoder\'s HWC RGB layout -- got {tuple(lrs.shape)}')
            n, t, h, w, c = lrs.size()
        else:
            n, t, c, h, w = lrs.size()
        assert h >= 64 and w >= 64, (
            f'The height and width of inputs should be at least 64, but got {h} and {w}.')
        dev = lrs.device
        self._check_resident(t)
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            lrs_c = lrs.detach().contiguous() if byte_in else lrs.detach().float().contiguous()
            # the library reads the bytes as dwords: a view at an odd storage offset is copied (any_size reads a clip at any address)
            if byte_in and lrs_c.data_ptr() % 4 and not self.any_size:
                lrs_c = lrs_c.clone()
            mvs_c = mvs.detach().float().contiguous()
            par_c = par_map.detach().float().contiguous()
            if mvs_c.shape != (n, t, 4, h, w) or par_c.shape != (n, t, 3, h, w):
                raise ValueError(f'The spatial sizes of input ({(h, w)}) and flow/partition maps '
                                 f'({tuple(mvs_c.shape)}, {tuple(par_c.shape)}) are not the same.')
            if self.sparse_val:
                # the reference's blocks take sparse_conv only when `self.sparse_val and not self.training`
                # (sr_backbone_utils.py:308,322, basicvsr_net.py:511); in train() mode they run the dense formula
                sparse_now = 0 if self.training else 1
                if self.get_option(_native.OPT_SPARSE_EVAL) != sparse_now:
                    self.set_option(_native.OPT_SPARSE_EVAL, sparse_now)
            if self.sparse_val and not self.training and n != 1:
                raise NotImplementedError('sparse_val=True evaluates one clip at a time: the reference reads feature[0] '
                                          'only (sr_backbone_utils.py:262-275)')
            # a side tensor the configuration does not read may be None, as in the reference (QPs is always read when
            # with_bias; base_QPs only when use_base_qp, iconvsr_ipb_par.py:45-48)
            zero = torch.zeros(n, t, device=slices.device) if slices is not None else None
            if slices is None:
                raise TypeError('slices (n,t,1,1,1) is required: it selects the key frames (iconvsr_ipb_par.py:60-62)')
            if QPs is None and (self.with_bias or not self.use_base_qp):
                raise TypeError('QPs is required by this configuration (iconvsr_ipb_par.py:45-48)')
            if base_QPs is None and self.use_base_qp:
                raise TypeError('base_QPs is required when use_base_qp=True (iconvsr_ipb_par.py:45)')
            # the three (n,t,1,1,1) side-info tensors drive host control flow (key frames, expert dedup): ONE D2H copy
            side = torch.stack([slices.reshape(n, t).float(),
                                QPs.reshape(n, t).float() if QPs is not None else zero,
                                base_QPs.reshape(n, t).float() if base_QPs is not None else zero]).cpu().contiguous()
            if byte_in or mask != _native.OUT_F32:
                return self._forward_io(lrs_c, mvs_c, par_c, side, mask)
            # the PyTorch custom op over pnp_generator_forward (pnp_vcve_amd/torch_ops.py)
            out = torch.ops.pnpvcve.generator_forward(self._op_handle, lrs_c, mvs_c, par_c, side)
        return out

    # ---------------------------------------------------------------- byte frames, clips by pointer
    def _alloc_outs(self, n, t, h, w, mask, dev):
        s = 4 if self.vsr else 1
        f32 = torch.empty((n, t, 3, h * s, w * s), device=dev, dtype=torch.float32) if mask & _native.OUT_F32 else None
        u8 = torch.empty((n, t, h * s, w * s, 3), device=dev, dtype=torch.uint8) if mask & _native.OUT_U8 else None
        return f32, u8

    @staticmethod
    def _ret(f32, u8, mask):
        return f32 if mask == _native.OUT_F32 else (u8 if mask == _native.OUT_U8 else (f32, u8))

    def _forward_io(self, lrs_c, mvs_c, par_c, side, mask):
        """forward() at a byte boundary: (n,...) batch tensors in, the outputs allocated as (n,...) tensors, every clip handed to
        pnp_generator_forward_clips as a descriptor of its slices."""
        byte_in = lrs_c.dtype == torch.uint8
        n, t = lrs_c.shape[:2]
        h, w = lrs_c.shape[2:4] if byte_in else lrs_c.shape[3:5]
        dev = lrs_c.device
        if self.use_graphs and not self._profiling:
            return self._forward_graphed(lrs_c, mvs_c, par_c, side, None, mask)
        f32, u8 = self._alloc_outs(n, t, h, w, mask, dev)
        ws = self._get_workspace(n, t, h, w, dev, int(byte_in), mask)
        self._launch_clips(list(lrs_c), list(mvs_c), list(par_c), side, list(f32) if f32 is not None else None,
                           list(u8) if u8 is not None else None, ws, t, h, w)
        return self._ret(f32, u8, mask)

    def _launch_clips(self, lrs, mvs, par, side, outs_f32, outs_u8, ws, t, h, w):
        """One pnp_generator_forward_clips call on torch's current stream: per-clip contiguous tensors, nothing concatenated."""
        n = len(lrs)
        byte_in = lrs[0].dtype == torch.uint8
        mask = (_native.OUT_F32 if outs_f32 is not None else 0) | (_native.OUT_U8 if outs_u8 is not None else 0)
        clips = (_native.ClipIO * n)()
        for b in range(n):
            clips[b] = _native.ClipIO(lrs[b].data_ptr(), mvs[b].data_ptr(), par[b].data_ptr(),
                                      outs_f32[b].data_ptr() if outs_f32 is not None else None,
                                      outs_u8[b].data_ptr() if outs_u8 is not None else None)
        fp = ctypes.POINTER(ctypes.c_float)
        base = side.data_ptr()
        P = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = _native.lib().pnp_generator_forward_clips(
            self._handle, P(self._flat), P(self._packed), ctypes.cast(clips, ctypes.c_void_p), n,
            _native.FRAMES_U8_HWC if byte_in else _native.FRAMES_F32_NCHW, mask, ctypes.cast(base, fp),
            ctypes.cast(base + 4 * n * t, fp), ctypes.cast(base + 8 * n * t, fp), P(ws), ws.numel(), t, h, w,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, 'pnp_generator_forward_clips')

    def forward_clips(self, clips, out_dtype=None, yuv_standard='bt601-limited', chroma='replicate'):
        """A batch as a sequence of clips, each where it lives: clips[i] = (lrs, QPs, slices, mvs, base_QPs, par_map) with the tensors
        of forward() for n = 1 (or without the batch dimension).  All clips go to the library in ONE call as pointers -- nothing is
        concatenated -- and run like a batch (large frames two at a time on two streams, small ones up to eight).  Returns a list of
        per-clip outputs, each what forward(..., out_dtype) returns for that clip (with the batch dimension, n = 1).  The clips must
        agree in shape and in the dtype class of lrs (uint8 or floating point): ValueError otherwise.  Not replayed from a graph
        (use_graphs concerns forward()): a graph's static buffers would be the copies this call exists to avoid.
        Clips whose lrs are ops.Yuv420Frames (each clip's planes in allocations of their own) take yuv_standard, chroma and the
        out_dtype values of forward()'s 4:2:0 boundary."""
        clips = list(clips)
        if clips and ops.is_yuv(clips[0][0]):
            return self._forward_clips_yuv(clips, out_dtype, yuv_standard, chroma)
        mask = self._out_mask(out_dtype)
        if not clips:
            raise ValueError('forward_clips needs at least one clip')
        if self.sparse_val and not self.training and len(clips) != 1:
            raise NotImplementedError('sparse_val=True evaluates one clip at a time: the reference reads feature[0] '
                                      'only (sr_backbone_utils.py:262-275)')
        lr_l, mv_l, par_l, sides = [], [], [], []
        first = None
        for lrs, QPs, slices, mvs, base_QPs, par_map in clips:
            if not lrs.is_cuda:
                raise RuntimeError('PnP-VCVE generator: inputs must be CUDA/HIP tensors; this build has no CPU path')
            byte_in = lrs.dtype == torch.uint8
            nd = 4 if lrs.dim() == 4 else 5
            if lrs.dim() not in (4, 5) or (nd == 5 and lrs.shape[0] != 1):
                raise ValueError(f'a clip of forward_clips is one sample: (t,...) or (1,t,...) tensors, got lrs {tuple(lrs.shape)}')
            lrs = lrs.reshape(lrs.shape[-4:])
            if byte_in and lrs.shape[-1] != 3:
                raise ValueError(f'uint8 frames must be (t,h,w,3) -- the decoder\'s HWC RGB layout -- got {tuple(lrs.shape)}')
            t, (h, w) = lrs.shape[0], (lrs.shape[1:3] if byte_in else lrs.shape[2:4])
            sig = (byte_in, t, h, w, lrs.device)
            if first is None:
                first = sig
            elif sig != first:
                raise ValueError(f'the clips of one forward_clips call must agree in shape, device and in uint8 / float frames: '
                                 f'{sig} against {first}')
            assert h >= 64 and w >= 64, f'The height and width of inputs should be at least 64, but got {h} and {w}.'
            if slices is None:
                raise TypeError('slices (n,t,1,1,1) is required: it selects the key frames (iconvsr_ipb_par.py:60-62)')
            if QPs is None and (self.with_bias or not self.use_base_qp):
                raise TypeError('QPs is required by this configuration (iconvsr_ipb_par.py:45-48)')
            if base_QPs is None and self.use_base_qp:
                raise TypeError('base_QPs is required when use_base_qp=True (iconvsr_ipb_par.py:45)')
            mvs_c = mvs.detach().float().reshape(mvs.shape[-4:]).contiguous()
            par_c = par_map.detach().float().reshape(par_map.shape[-4:]).contiguous()
            if mvs_c.shape != (t, 4, h, w) or par_c.shape != (t, 3, h, w):
                raise ValueError(f'The spatial sizes of input ({(h, w)}) and flow/partition maps '
                                 f'({tuple(mvs_c.shape)}, {tuple(par_c.shape)}) are not the same.')
            lrs = lrs.detach().contiguous() if byte_in else lrs.detach().float().contiguous()
            # the library reads the bytes as dwords: a view at an odd storage offset is copied (any_size reads a clip at any address)
            if byte_in and lrs.data_ptr() % 4 and not self.any_size:
                lrs = lrs.clone()
            lr_l.append(lrs)
            mv_l.append(mvs_c)
            par_l.append(par_c)
            zero = torch.zeros(t, device=slices.device)
            sides.append(torch.stack([slices.reshape(t).float(), QPs.reshape(t).float() if QPs is not None else zero,
                                      base_QPs.reshape(t).float() if base_QPs is not None else zero]))
        byte_in, t, h, w, dev = first
        self._check_resident(t)
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            if self.sparse_val:
                sparse_now = 0 if self.training else 1
                if self.get_option(_native.OPT_SPARSE_EVAL) != sparse_now:
                    self.set_option(_native.OPT_SPARSE_EVAL, sparse_now)
            side = torch.stack(sides, dim=1).cpu().contiguous()          # (3, n, t): ONE D2H copy
            outs = torch.ops.pnpvcve.generator_forward_clips(self._op_handle, lr_l, mv_l, par_l, side, mask)
        n = len(lr_l)
        f32 = [o[None] for o in outs[:n]] if mask & _native.OUT_F32 else None
        u8 = [o[None] for o in outs[-n:]] if mask & _native.OUT_U8 else None
        return [self._ret(f32[i] if f32 else None, u8[i] if u8 else None, mask) for i in range(n)]

    # ---------------------------------------------------------------- self-ensemble (include/pnpvcve.h, "Self-ensemble")
    def _ensemble_group_limit(self, h, w):
        """variants per forward_clips call: what the library runs concurrently (see _contexts); a sparse_val generator in eval mode
        takes one clip per call"""
        if self.sparse_val and not self.training:
            return 1
        return self.LARGE_FRAME_CONTEXTS if h * w >= self.CONCURRENT_BELOW_PIXELS else self.MAX_CONTEXTS

    def forward_ensemble(self, lrs, QPs=None, slices=None, mvs=None, base_QPs=None, par_map=None, temporal=False, out_dtype=None):
        """The self-ensemble of forward(): the mean of the outputs over the 8 flips / transposes of the clip (temporal: and their 8
        time reversals), every variant's side information -- motion vectors, partition planes, slices, QPs -- transformed together
        with the frames (ops.ensemble_view / ensemble_side; the rule: include/pnpvcve.h), every output taken back through the
        variant's inverse.  The sum is sequential in fp32 in ascending variant order, scaled once by 1/8 or 1/16
        (ops.ensemble_accumulate).  Inputs as forward()'s, fp32 or uint8 frames, (n,t,...); samples run one after another, a
        sample's variants go through forward_clips in groups of one orientation.  out_dtype: None / torch.float32 | torch.uint8 |
        'both', the bytes being ops.frames_to_rgb8 of the fp32 mean.  4:2:0 frames and deform != 'vos' raise ValueError; the
        frame-size rules are forward()'s own, for both orientations.  Not replayed from a graph."""
        if ops.is_yuv(lrs):
            raise ValueError('the self-ensemble takes fp32 or uint8 RGB frames: where the chroma samples of a flipped 4:2:0 frame lie is '
                             'not defined here')
        if self._cfg.deform != _DEFORM['vos']:
            raise ValueError("the self-ensemble runs deform='vos' generators only: the learned offsets of a DCN aligner are not "
                             'transformed with the frame')
        mask = self._out_mask(out_dtype)
        if not lrs.is_cuda:
            raise RuntimeError('PnP-VCVE generator: inputs must be CUDA/HIP tensors; this build has no CPU path')
        byte_in = lrs.dtype == torch.uint8
        if lrs.dim() != 5 or (byte_in and lrs.shape[-1] != 3):
            raise ValueError(f'frames must be (n,t,3,h,w) fp32 or (n,t,h,w,3) uint8, got {tuple(lrs.shape)}')
        n, t = lrs.shape[:2]
        h, w = lrs.shape[2:4] if byte_in else lrs.shape[3:5]
        if mvs is None or par_map is None:
            raise TypeError('mvs (n,t,4,h,w) and par_map (n,t,3,h,w) are required')
        variants = ops.ENSEMBLE_SPATIAL_TEMPORAL if temporal else ops.ENSEMBLE_SPATIAL
        limit = self._ensemble_group_limit(h, w)
        groups = []        # ascending v; a group holds one orientation (a square frame has one)
        for v in variants:
            if groups and len(groups[-1]) < limit and (h == w or (groups[-1][-1] ^ v) & 4 == 0):
                groups[-1].append(v)
            else:
                groups.append([v])
        s = 4 if self.vsr else 1
        dev = lrs.device
        with torch.cuda.device(dev):
            acc = torch.empty((n, t, 3, h * s, w * s), device=dev, dtype=torch.float32)
            lq_all = lrs.detach().contiguous() if byte_in else lrs.detach().float().contiguous()
            mv_all, par_all = mvs.detach().float().contiguous(), par_map.detach().float().contiguous()
            for b in range(n):
                side = tuple(x[b] if x is not None else None for x in (QPs, slices, base_QPs))
                for group in groups:
                    clips = []
                    for v in group:
                        lq_v, mv_v, par_v = (lq_all[b], mv_all[b], par_all[b]) if v == 0 else ops.ensemble_view(lq_all[b], mv_all[b], par_all[b], v)
                        qp_v, sl_v, bq_v = ops.ensemble_side(*side, v)
                        clips.append((lq_v, qp_v, sl_v, mv_v, bq_v, par_v))
                    outs = self.forward_clips(clips, out_dtype=torch.float32)
                    for v, out in zip(group, outs):
                        ops.ensemble_accumulate(acc[b], out, v, first=v == variants[0], scale=1.0 / len(variants) if v == variants[-1] else 1.0)
                    del clips, outs
            u8 = torch.stack([ops.frames_to_rgb8(acc[b]) for b in range(n)]) if mask & _native.OUT_U8 else None
        return self._ret(acc, u8, mask)

    def _forward_clips_native(self, lrs, mvs, par, side, mask):
        """Body of torch.ops.pnpvcve.generator_forward_clips: per-clip contiguous CUDA tensors + the (3, n, t) host side info ->
        the fp32 outputs (mask & 1), then the uint8 ones (mask & 2), one freshly allocated tensor per clip."""
        n = len(lrs)
        byte_in = lrs[0].dtype == torch.uint8
        t = lrs[0].shape[0]
        h, w = lrs[0].shape[1:3] if byte_in else lrs[0].shape[2:4]
        dev = lrs[0].device
        with torch.cuda.device(dev):
            f32 = [self._alloc_outs(1, t, h, w, _native.OUT_F32, dev)[0][0] for _ in range(n)] if mask & _native.OUT_F32 else None
            u8 = [self._alloc_outs(1, t, h, w, _native.OUT_U8, dev)[1][0] for _ in range(n)] if mask & _native.OUT_U8 else None
            ws = self._get_workspace(n, t, h, w, dev, int(byte_in), mask)
            self._launch_clips(lrs, mvs, par, side, f32, u8, ws, t, h, w)
        return (f32 or []) + (u8 or [])

    # ---------------------------------------------------------------- 4:2:0 frames (pnp_generator_forward_clips_yuv)
    @staticmethod
    def _yuv_outs(out_dtype):
        """out_dtype of the 4:2:0 boundary -> (the requested kinds in order, 'f32' | 'u8' | 'yuv'; the mask; the layout of 'yuv' or
        None; whether a tuple was asked for)"""
        many = isinstance(out_dtype, (tuple, list))
        kinds, layout = [], None
        for d in (out_dtype if many else [out_dtype]):
            if d is None or d == torch.float32:
                kinds.append('f32')
            elif d == torch.uint8:
                kinds.append('u8')
            elif isinstance(d, str) and (d in ('nv12', 'i420') or d in ops.YUV16_LAYOUTS or d in ops.YUV_FORMAT_LAYOUTS):
                if layout is not None:
                    raise ValueError('one 4:2:0 / 4:2:2 / 4:4:4 planes layout per call')
                layout = d
                kinds.append('yuv')
            else:
                raise ValueError(f"out_dtype must be None, torch.float32, torch.uint8, 'nv12', 'i420', one of {sorted(ops.YUV16_LAYOUTS)}, "
                                 f"one of {list(ops.YUV_FORMAT_LAYOUTS)} (4:2:2 / 4:4:4 planes in) or a tuple of them, got {d!r}")
        if not kinds or len(set(kinds)) != len(kinds):
            raise ValueError(f'out_dtype names no output or one twice: {out_dtype!r}')
        bits = {'f32': _native.OUT_F32, 'u8': _native.OUT_U8, 'yuv': _native.OUT_YUV420}
        return kinds, sum(bits[k] for k in kinds), layout, many

    @staticmethod
    def _yuv_out_route(lrs, kinds, layout):
        """What the planes output of a call needs beside the library's own: (None, out_dtype) where the library writes it, or -- 8-bit
        planes of a 10 / 12-bit clip, which the library's entry for such clips does not write -- (layout, the out_dtype tuple to run
        instead: the other outputs and the fp32 one the planes are then made of).  16-bit planes of an 8-bit clip are refused, and so is
        a layout of another chroma format than the input's (one code serves both directions: there is no format conversion)."""
        sixteen = isinstance(lrs, ops._YUV16_CLASSES)
        if layout is None:
            return None, None
        fmt, _, depth, _ = ops.yuv_layout(layout)
        if fmt != ops.yuv_format(lrs):
            raise ValueError(f'out_dtype {layout!r} is a 4:{fmt[1]}:{fmt[2]} layout and the input planes are {type(lrs).__name__}: the planes '
                             f'written have the input\'s chroma format')
        if depth != 8 and not sixteen:
            raise ValueError(f'out_dtype {layout!r}: 10 / 12-bit planes out of 8-bit planes in are not offered (the input holds no such '
                             f'precision); pass ops.Yuv420Frames16 frames or ask for \'nv12\' / \'i420\'')
        if not sixteen or depth != 8:
            return None, None
        run = [torch.float32 if k == 'f32' else torch.uint8 for k in kinds if k != 'yuv']
        return layout, tuple(run if 'f32' in kinds else run + [torch.float32])

    @staticmethod
    def _yuv8_of_16(res, kinds, layout, std):
        """the outputs `kinds` asks for, from a run of _yuv_out_route's out_dtype: the 8-bit planes are ops.frames_to_yuv420 of the fp32
        output; std: the code of ops._yuv_code"""
        ran = [k for k in kinds if k != 'yuv'] + ([] if 'f32' in kinds else ['f32'])
        got = dict(zip(ran, res))
        standard, chroma, _ = ops._yuv_code_split3(std)      # (the layout names the format)
        got['yuv'] = ops.frames_to_yuv(got['f32'], standard, layout, chroma=chroma)[0]
        return tuple(got[k] for k in kinds)

    def _yuv_side(self, t, QPs, slices, base_QPs):
        """one clip's (3, t) side info, with forward()'s refusals"""
        if slices is None:
            raise TypeError('slices (n,t,1,1,1) is required: it selects the key frames (iconvsr_ipb_par.py:60-62)')
        if QPs is None and (self.with_bias or not self.use_base_qp):
            raise TypeError('QPs is required by this configuration (iconvsr_ipb_par.py:45-48)')
        if base_QPs is None and self.use_base_qp:
            raise TypeError('base_QPs is required when use_base_qp=True (iconvsr_ipb_par.py:45)')
        zero = torch.zeros(t, device=slices.device)
        return torch.stack([slices.reshape(t).float(), QPs.reshape(t).float() if QPs is not None else zero,
                            base_QPs.reshape(t).float() if base_QPs is not None else zero])

    def _forward_yuv(self, frames, QPs, slices, mvs, base_QPs, par_map, out_dtype, yuv_standard, chroma='replicate'):
        std = ops._yuv_code(yuv_standard, chroma, ops.yuv_format(frames))      # (what the library takes as yuv_standard; part of a graph's key)
        kinds, mask, layout, many = self._yuv_outs(out_dtype)
        clips, lead = ops._yuv_clips(frames, 'lrs')
        if not lead:
            raise ValueError('forward() takes a batch: Yuv420Frames of (n,t,rows,cols) views')
        descs = [ops._yuv_clip_desc(c, 'lrs') for c in clips]      # (every refusal before any GPU work)
        via8, run_dtype = self._yuv_out_route(frames, kinds, layout)
        if via8:
            res = self._yuv8_of_16(self._forward_yuv(frames, QPs, slices, mvs, base_QPs, par_map, run_dtype, yuv_standard, chroma), kinds, via8, std)
            return res if many else res[0]
        n, (_, t, h, w) = len(clips), descs[0]
        assert h >= 64 and w >= 64, f'The height and width of inputs should be at least 64, but got {h} and {w}.'
        self._check_resident(t)
        dev = frames.y.device
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            mvs_c = mvs.detach().float().contiguous()
            par_c = par_map.detach().float().contiguous()
            if mvs_c.shape != (n, t, 4, h, w) or par_c.shape != (n, t, 3, h, w):
                raise ValueError(f'The spatial sizes of input ({(h, w)}) and flow/partition maps '
                                 f'({tuple(mvs_c.shape)}, {tuple(par_c.shape)}) are not the same.')
            if self.sparse_val:
                sparse_now = 0 if self.training else 1
                if self.get_option(_native.OPT_SPARSE_EVAL) != sparse_now:
                    self.set_option(_native.OPT_SPARSE_EVAL, sparse_now)
            if self.sparse_val and not self.training and n != 1:
                raise NotImplementedError('sparse_val=True evaluates one clip at a time: the reference reads feature[0] '
                                          'only (sr_backbone_utils.py:262-275)')
            side = torch.stack([self._yuv_side(t, QPs[b] if QPs is not None else None, slices[b] if slices is not None else None,
                                               base_QPs[b] if base_QPs is not None else None) for b in range(n)], dim=1).cpu().contiguous()
            if self.use_graphs and not self._profiling:
                outs = self._forward_yuv_graphed(clips, mvs_c, par_c, side, std, mask, layout, (n, t, h, w))
            else:
                outs = self._alloc_yuv_outs(n, t, h, w, mask, layout, dev, frames.y.dtype)
                ws = self._get_workspace(n, t, h, w, dev, 'yuv', mask)
                self._launch_clips_yuv(clips, list(mvs_c), list(par_c), side, outs, ws, t, h, w, std)
        res = tuple(outs[k][0] for k in kinds)
        return res if many else res[0]

    def _alloc_yuv_outs(self, n, t, h, w, mask, layout, dev, word_dtype=torch.int16):
        """-> {'f32' | 'u8' | 'yuv': (the (n,...) tensor returned, what the launch writes per clip)} for the bits of mask; word_dtype:
        the dtype of a 16-bit planes buffer"""
        s = 4 if self.vsr else 1
        outs = {}
        if mask & _native.OUT_F32:
            x = torch.empty((n, t, 3, h * s, w * s), device=dev, dtype=torch.float32)
            outs['f32'] = (x, list(x))
        if mask & _native.OUT_U8:
            x = torch.empty((n, t, h * s, w * s, 3), device=dev, dtype=torch.uint8)
            outs['u8'] = (x, list(x))
        if mask & _native.OUT_YUV420:
            buf, views = ops.empty_yuv((n, t), h * s, w * s, layout, dev, word_dtype)
            outs['yuv'] = (buf, ops._yuv_clips(views, 'out')[0])
        return outs

    def _launch_clips_yuv(self, clips, mvs, par, side, outs, ws, t, h, w, std):
        """One pnp_generator_forward_clips_yuv call (Yuv420Frames16 clips: pnp_generator_forward_clips_yuv16) on torch's current stream:
        per-clip plane views, nothing copied or concatenated."""
        n = len(clips)
        sixteen = isinstance(clips[0], ops._YUV16_CLASSES)
        Clip, Planes = (_native.ClipYuv16, _native.Yuv420Planes16) if sixteen else (_native.ClipYuv, _native.Yuv420Planes)
        entry = 'pnp_generator_forward_clips_yuv16' if sixteen else 'pnp_generator_forward_clips_yuv'
        arr = (Clip * n)()
        mask = 0
        for kind, bit in (('f32', _native.OUT_F32), ('u8', _native.OUT_U8), ('yuv', _native.OUT_YUV420)):
            mask |= bit if kind in outs else 0
        for b in range(n):
            lq = ops._yuv_clip_desc(clips[b], 'lrs')[0]
            oy = ops._yuv_clip_desc(outs['yuv'][1][b], 'out')[0] if 'yuv' in outs else Planes()
            if not isinstance(oy, Planes):
                raise ValueError('the planes output must have the sample size of the input planes')
            arr[b] = Clip(lq, mvs[b].data_ptr(), par[b].data_ptr(), outs['f32'][1][b].data_ptr() if 'f32' in outs else None,
                                     outs['u8'][1][b].data_ptr() if 'u8' in outs else None, oy)
        fp = ctypes.POINTER(ctypes.c_float)
        base = side.data_ptr()
        P = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = getattr(_native.lib(), entry)(
            self._handle, P(self._flat), P(self._packed), ctypes.cast(arr, ctypes.c_void_p), n, std, mask, ctypes.cast(base, fp),
            ctypes.cast(base + 4 * n * t, fp), ctypes.cast(base + 8 * n * t, fp), P(ws), ws.numel(), t, h, w,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, entry)

    def _forward_yuv_graphed(self, clips, mvs_c, par_c, side, std, mask, layout, shape):
        """use_graphs at the 4:2:0 boundary: the planes are copied into static planes of their own (1.5 B per pixel), the outputs out"""
        n, t, h, w = shape
        dev = mvs_c.device
        c0 = clips[0]
        key = ('yuv', n, t, h, w, str(dev), side.numpy().tobytes(), self._packed.data_ptr(), self._packed_floats, self.max_resident_features,
               std, mask, layout, c0.y.dtype, tuple(c0[3:]))
        ent = self._graphs.get(key)
        fill = lambda e: [dst.copy_(src) for b in range(n) for dst, src in zip(e['clips'][b][:3], clips[b][:3])]      # noqa: E731
        if ent is None:
            mk = lambda hh, ww: torch.empty((n, t, hh, ww), device=dev, dtype=c0.y.dtype)      # noqa: E731
            sx, sy = _native.YUV_FACTORS[ops.yuv_format(c0)]
            static = type(c0)(mk(h, w), mk(h // sy, w // sx), mk(h // sy, w // sx), *c0[3:])
            ent = dict(clips=ops._yuv_clips(static, 'lrs')[0], mvs=torch.empty_like(mvs_c), par=torch.empty_like(par_c), side=side.clone(),
                       ws=torch.empty(self._workspace_bytes(t, h, w, 'yuv', mask) * self._contexts(n, h, w), device=dev, dtype=torch.uint8),
                       outs=self._alloc_yuv_outs(n, t, h, w, mask, layout, dev, c0.y.dtype))
            run = lambda: self._launch_clips_yuv(ent['clips'], list(ent['mvs']), list(ent['par']), ent['side'], ent['outs'], ent['ws'],      # noqa: E731
                                                 t, h, w, std)
            fill(ent)
            ent['mvs'].copy_(mvs_c)
            ent['par'].copy_(par_c)
            cur = torch.cuda.current_stream()
            warm = torch.cuda.Stream()
            warm.wait_stream(cur)
            with torch.cuda.stream(warm):       # eager once: first-use attribute calls must not land in a capture
                run()
            cur.wait_stream(warm)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            ent['graph'] = graph
            while len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = ent
        else:
            fill(ent)
            ent['mvs'].copy_(mvs_c)
            ent['par'].copy_(par_c)
        ent['graph'].replay()
        return {k: (v[0].clone(), None) for k, v in ent['outs'].items()}

    def _forward_clips_yuv(self, clips, out_dtype, yuv_standard, chroma='replicate'):
        if not ops.is_yuv(clips[0][0]):
            raise TypeError('the clips of one forward_clips call must all be planes')
        std = ops._yuv_code(yuv_standard, chroma, ops.yuv_format(clips[0][0]))
        kinds, mask, layout, many = self._yuv_outs(out_dtype)
        if self.sparse_val and not self.training and len(clips) != 1:
            raise NotImplementedError('sparse_val=True evaluates one clip at a time: the reference reads feature[0] '
                                      'only (sr_backbone_utils.py:262-275)')
        lrs0 = clips[0][0]
        via8, run_dtype = self._yuv_out_route(lrs0, kinds, layout)
        if via8:
            res = [self._yuv8_of_16(r, kinds, via8, std) for r in self._forward_clips_yuv(clips, run_dtype, yuv_standard, chroma)]
            return res if many else [r[0] for r in res]
        ys, cbs, crs, mv_l, par_l, sides, first = [], [], [], [], [], [], None
        for lrs, QPs, slices, mvs, base_QPs, par_map in clips:
            one, lead = ops._yuv_clips(lrs, 'lrs')
            if len(one) != 1:
                raise ValueError('a clip of forward_clips is one sample: Yuv420Frames of (t,...) or (1,t,...) views')
            _, t, h, w = ops._yuv_clip_desc(one[0], 'lrs')
            sig = (t, h, w, lrs.y.device, type(lrs)) + ((lrs.y.dtype,) + tuple(lrs[3:]) if isinstance(lrs0, ops._YUV16_CLASSES) else ())
            if first is None:
                first = sig
            elif sig != first:
                raise ValueError(f'the clips of one forward_clips call must agree in shape and device: {sig} against {first}')
            assert h >= 64 and w >= 64, f'The height and width of inputs should be at least 64, but got {h} and {w}.'
            mvs_c = mvs.detach().float().reshape(mvs.shape[-4:]).contiguous()
            par_c = par_map.detach().float().reshape(par_map.shape[-4:]).contiguous()
            if mvs_c.shape != (t, 4, h, w) or par_c.shape != (t, 3, h, w):
                raise ValueError(f'The spatial sizes of input ({(h, w)}) and flow/partition maps '
                                 f'({tuple(mvs_c.shape)}, {tuple(par_c.shape)}) are not the same.')
            ys.append(one[0].y), cbs.append(one[0].cb), crs.append(one[0].cr)
            mv_l.append(mvs_c)
            par_l.append(par_c)
            sides.append(self._yuv_side(t, QPs, slices, base_QPs))
        t, h, w, dev = first[:4]
        self._check_resident(t)
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            if self.sparse_val:
                sparse_now = 0 if self.training else 1
                if self.get_option(_native.OPT_SPARSE_EVAL) != sparse_now:
                    self.set_option(_native.OPT_SPARSE_EVAL, sparse_now)
            side = torch.stack(sides, dim=1).cpu().contiguous()
            if isinstance(lrs0, ops._YUV16_CLASSES):
                flat = torch.ops.pnpvcve.generator_forward_clips_yuv16(self._op_handle, ys, cbs, crs, int(lrs0.bit_depth), bool(lrs0.msb_aligned),
                                                                       mv_l, par_l, side, std, mask, ops._yuv_layout_index(layout))
            else:
                flat = torch.ops.pnpvcve.generator_forward_clips_yuv(self._op_handle, ys, cbs, crs, mv_l, par_l, side, std, mask,
                                                                     ops._yuv_layout_index(layout))
        n = len(ys)
        order = [k for k in ('f32', 'u8', 'yuv') if k in kinds]
        per = {k: flat[j * n:(j + 1) * n] for j, k in enumerate(order)}
        res = [tuple(per[k][i][None] for k in kinds) for i in range(n)]
        return res if many else [r[0] for r in res]

    def _forward_clips_yuv_native(self, ys, cbs, crs, mvs, par, side, std, mask, layout, bit_depth=8, msb_aligned=False):
        """Body of torch.ops.pnpvcve.generator_forward_clips_yuv: per-clip plane views -> the fp32 outputs (mask & 1), then the uint8
        ones (mask & 2), then the packed 4:2:0 buffers (mask & 4), one freshly allocated tensor per clip."""
        n = len(ys)
        cls8, cls16 = ops._YUV_CLASSES[ops._yuv_code_split3(std)[2]]      # (the `standard` integer carries the chroma format)
        if bit_depth == 8:
            clips = [cls8(ys[b], cbs[b], crs[b]) for b in range(n)]
        else:      # (torch.ops.pnpvcve.generator_forward_clips_yuv16)
            clips = [cls16(ys[b], cbs[b], crs[b], bit_depth, msb_aligned) for b in range(n)]
        t, h, w = ys[0].shape
        dev = ys[0].device
        with torch.cuda.device(dev):
            per = [self._alloc_yuv_outs(1, t, h, w, mask, layout, dev, ys[0].dtype) for _ in range(n)]
            outs = {k: (None, [p[k][1][0] for p in per]) for k in per[0]}
            ws = self._get_workspace(n, t, h, w, dev, 'yuv', mask)
            self._launch_clips_yuv(clips, mvs, par, side, outs, ws, t, h, w, std)
        return [p[k][0][0] for k in ('f32', 'u8', 'yuv') if k in per[0] for p in per]

    def _forward_native(self, lrs_c, mvs_c, par_c, side):
        """Body of torch.ops.pnpvcve.generator_forward: contiguous fp32 CUDA tensors + the (3, n, t) host side info."""
        n, t, _, h, w = lrs_c.shape
        s = 4 if self.vsr else 1
        with torch.cuda.device(lrs_c.device):
            if self.use_graphs and not self._profiling:
                return self._forward_graphed(lrs_c, mvs_c, par_c, side, (n, t, 3, h * s, w * s))
            out = torch.empty((n, t, 3, h * s, w * s), device=lrs_c.device, dtype=torch.float32)
            ws = self._get_workspace(n, t, h, w, lrs_c.device)
            self._launch(lrs_c, mvs_c, par_c, side, out, ws)
        return out

    def _launch(self, lrs_c, mvs_c, par_c, side, out, ws):
        """One pnp_generator_forward call on torch's current stream."""
        n, t, _, h, w = lrs_c.shape
        fp = ctypes.POINTER(ctypes.c_float)
        base = side.data_ptr()
        P = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = _native.lib().pnp_generator_forward(
            self._handle, P(self._flat), P(self._packed), P(lrs_c), P(mvs_c), P(par_c), ctypes.cast(base, fp),
            ctypes.cast(base + 4 * n * t, fp), ctypes.cast(base + 8 * n * t, fp), P(out), P(ws), ws.numel(), n, t, h, w,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, 'pnp_generator_forward')

    # ---------------------------------------------------------------- HIP graphs (small frames are launch-bound)
    #: opt-in: replay the clip's ~700 launches as one hipGraph.  A graph is keyed by everything its launches bake in:
    #: shape, the side info (QP values are kernel arguments, slice types steer the schedule), precision and the
    #: packed weights; inputs are copied into the graph's static buffers, the output is copied out.
    use_graphs = False
    MAX_GRAPHS = 8

    def _forward_graphed(self, lrs_c, mvs_c, par_c, side, out_shape, mask=_native.OUT_F32):
        """(a byte boundary -- uint8 lrs_c (n,t,h,w,3) and / or mask != OUT_F32 -- gets static buffers of the input's dtype and of the
        outputs asked for, and a key with the format and the mask; out_shape is then unused)"""
        byte_in = lrs_c.dtype == torch.uint8
        io = byte_in or mask != _native.OUT_F32
        n, t = lrs_c.shape[:2]
        h, w = lrs_c.shape[2:4] if byte_in else lrs_c.shape[3:5]
        dev = lrs_c.device
        key = (n, t, h, w, str(dev), side.numpy().tobytes(), self._packed.data_ptr(), self._packed_floats, self.max_resident_features)
        if io:
            key = key + (int(byte_in), mask)
        ent = self._graphs.get(key)
        if ent is None:
            ctx = self._contexts(n, h, w)
            nbytes = self._workspace_bytes(t, h, w, int(byte_in), mask) * ctx
            ent = dict(lrs=torch.empty_like(lrs_c), mvs=torch.empty_like(mvs_c), par=torch.empty_like(par_c),
                       ws=torch.empty(nbytes, device=dev, dtype=torch.uint8), side=side.clone())
            if io:
                ent['out'], ent['out8'] = self._alloc_outs(n, t, h, w, mask, dev)
                run = lambda: self._launch_clips(list(ent['lrs']), list(ent['mvs']), list(ent['par']), ent['side'],      # noqa: E731
                                                 list(ent['out']) if ent['out'] is not None else None,
                                                 list(ent['out8']) if ent['out8'] is not None else None, ent['ws'], t, h, w)
            else:
                ent['out'] = torch.empty(out_shape, device=dev, dtype=torch.float32)
                run = lambda: self._launch(ent['lrs'], ent['mvs'], ent['par'], ent['side'], ent['out'], ent['ws'])      # noqa: E731
            for k, src in (('lrs', lrs_c), ('mvs', mvs_c), ('par', par_c)):
                ent[k].copy_(src)
            cur = torch.cuda.current_stream()
            warm = torch.cuda.Stream()
            warm.wait_stream(cur)
            with torch.cuda.stream(warm):       # eager once: first-use attribute calls must not land in a capture
                run()
            cur.wait_stream(warm)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            ent['graph'] = graph
            while len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = ent
        else:
            for k, src in (('lrs', lrs_c), ('mvs', mvs_c), ('par', par_c)):
                ent[k].copy_(src)
        ent['graph'].replay()
        if io:
            return self._ret(ent['out'].clone() if ent['out'] is not None else None,
                             ent['out8'].clone() if ent['out8'] is not None else None, mask)
        return ent['out'].clone()

    # ---------------------------------------------------------------- measurement aid
    PROF_KINDS = {'conv_block': 0, 'conv_input': 1, 'conv_head': 2, 'mv_warp': 3, 'dcn': 4}

    def profile(self, enable=True):
        """Bracket every kernel launch of forward() with HIP events (pnp_generator_profile)."""
        _native.check(_native.lib().pnp_generator_profile(self._handle, int(bool(enable))), 'pnp_generator_profile')
        self._profiling = bool(enable)

    def profile_read(self):
        """-> {kind: dict(ms=total device ms, launches=n, work=FLOPs or bytes)} since profile(True)."""
        res = {}
        for name, k in self.PROF_KINDS.items():
            ms, n, wk = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _native.check(_native.lib().pnp_generator_profile_read(self._handle, k, ctypes.byref(ms), ctypes.byref(n),
                                                                   ctypes.byref(wk)), 'pnp_generator_profile_read')
            res[name] = dict(ms=ms.value, launches=n.value, work=wk.value)
        return res

    def __del__(self):
        try:
            if self._handle:
                _native.lib().pnp_generator_destroy(self._handle)
                self._handle = ctypes.c_void_p()
        except Exception:
            pass
