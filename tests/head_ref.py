"""float64 reference of the reconstruction head's two conv forms (pnp_vcve_amd/csrc/generator.hip head(); iconvsr_ipb_par.py:135-146),
built from the calls the model itself makes, and the seeded inputs tests/test_gpu_head_edges.py runs the kernels on.

    pixel-shuffle conv:  act(F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2))
    conv_last:           act(F.conv2d(x, w, b, padding=1)) + base
                         base = the frame (out_mode 2) or F.interpolate(frame, scale_factor=4, 'bilinear', align_corners=False) (3)

A byte frame enters as float32(b) / float32(255) (the table of pnp_frames_from_rgb8), a byte output is
rint(clip(x, 0, 1) * 255) in float32 on the fp32 sum x.  tests/test_head_ref.py checks the reference against a second, hand-written
form of the bilinear and shows that the seeded inputs tell the obvious wrong kernels from the right one."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import syn

SEED = 7301

# sizes: output H x W for conv_last, input h x w for the pixel-shuffle conv; each the smallest shape that reaches its case
LAST_MODE2 = [(1, 1), (7, 15), (8, 16), (9, 17), (37, 53),
              (40, 48),       # 15 tiles: remainder 7 in the XCD remap
              (64, 64),       # 32 tiles: remainder 0
              (100, 932),     # 767 tiles: the last frame on KS = 4
              (185, 497)]     # 768 tiles, ragged: the first frame on KS = 1
LAST_MODE3 = [(4, 4),         # a 1 x 1 frame: both clamps apply at once
              (8, 16), (12, 20), (36, 52), (64, 64), (100, 932),
              (188, 500)]     # 768 tiles
PIXEL_SHUFFLE = [(3, 7), (4, 16), (5, 17), (37, 53), (64, 64),
                 (120, 1008),     # 945 8x16 tiles: the last frame on the 4x16 configuration
                 (121, 1009)]     # 1024 tiles: the first frame on the 8x16 configuration


def tiles_8x16(h, w):
    return ((h + 7) // 8) * ((w + 15) // 16)


def _ro(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- seeded inputs (read-only, computed once)
@functools.lru_cache(maxsize=None)
def last_weights():
    """conv_last.weight (3,64,3,3) in +-0.06, conv_last.bias (3,) in +-0.1"""
    return _ro(syn.uniform(SEED, 'last_w', (3, 64, 3, 3), -0.06, 0.06)), _ro(syn.uniform(SEED, 'last_b', (3,), -0.1, 0.1))


@functools.lru_cache(maxsize=None)
def shuffle_weights():
    """upsample_conv.weight (256,64,3,3) in +-0.06, .bias (256,) in +-0.1, different in every channel"""
    return _ro(syn.uniform(SEED, 'ps_w', (256, 64, 3, 3), -0.06, 0.06)), _ro(syn.uniform(SEED, 'ps_b', (256,), -0.1, 0.1))


@functools.lru_cache(maxsize=None)
def feature_map(kind, h, w):
    """(h,w,64) pixel-major map, uniform in (-1, 1); kind 'last' | 'ps'"""
    return _ro(syn.uniform(SEED, '%s_x_%dx%d' % (kind, h, w), (h, w, 64), -1.0, 1.0))


def frame_size(H, W, out_mode):
    return (H // 4, W // 4) if out_mode == 3 else (H, W)


@functools.lru_cache(maxsize=None)
def frame_planes(H, W, out_mode):
    """the frame conv_last adds at output size H x W: (3,h,w) float32 in [0, 1]"""
    h, w = frame_size(H, W, out_mode)
    return _ro(syn.uniform(SEED, 'frame_%dx%d_m%d' % (H, W, out_mode), (3, h, w), 0.0, 1.0))


@functools.lru_cache(maxsize=None)
def frame_bytes(H, W, out_mode):
    """... as (h,w,3) uint8"""
    h, w = frame_size(H, W, out_mode)
    return _ro(syn.randint(SEED, 'frame8_%dx%d_m%d' % (H, W, out_mode), (h, w, 3), 0, 255).astype(np.uint8))


def planes_from_bytes(u8):
    """(h,w,3) uint8 -> (3,h,w) float32: the table's definition, float32(b) / float32(255)"""
    return np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def rgb0_from_planes(p):
    """(3,h,w) float32 -> (h,w,4) float32 RGB0"""
    out = np.zeros(p.shape[1:] + (4,), np.float32)
    out[..., :3] = p.transpose(1, 2, 0)
    return out


def to_bytes(x):
    """(3,H,W) float32 sums -> (H,W,3) uint8: rint(clip(x, 0, 1) * 255) in float32 (round half to even)"""
    assert x.dtype == np.float32
    v = np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0))
    return np.ascontiguousarray(v.astype(np.uint8).transpose(1, 2, 0))


def round_f16(a):
    """the values an fp16 operand holds: float16 round-to-nearest-even of the fp32 value, as float64"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------- the reference
def _act(t, act):
    return t if act == 0 else (F.relu(t) if act == 1 else F.leaky_relu(t, 0.1))


def _nchw64(x_hwc):
    return torch.from_numpy(np.asarray(x_hwc, np.float64)).permute(2, 0, 1)[None]


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def pixel_shuffle_conv_ref(x_hwc, w, b, act):
    """(h,w,64) -> (2h,2w,64) float64"""
    y = _act(F.pixel_shuffle(F.conv2d(_nchw64(x_hwc), _t64(w), _t64(b), padding=1), 2), act)
    return np.ascontiguousarray(y[0].permute(1, 2, 0).numpy())


def conv_last_term(x_hwc, w, b, act=0):
    """act(conv_last(x)): (H,W,64) -> (3,H,W) float64"""
    return _act(F.conv2d(_nchw64(x_hwc), _t64(w), _t64(b), padding=1), act)[0].numpy()


def upsample_x4(planes):
    """(3,h,w) -> (3,4h,4w) float64: the model's F.interpolate call"""
    return F.interpolate(_t64(planes)[None], scale_factor=4, mode='bilinear', align_corners=False)[0].numpy()


def conv_last_base(planes, out_mode):
    return np.asarray(planes, np.float64) if out_mode == 2 else upsample_x4(planes)


def conv_last_ref(x_hwc, w, b, planes, out_mode, act=0):
    """(H,W,64) + the frame as (3,h,w) planes -> (3,H,W) float64"""
    return conv_last_term(x_hwc, w, b, act) + conv_last_base(planes, out_mode)


# ---------------------------------------------------------------- references of the seeded cases (computed once, shared, read-only)
@functools.lru_cache(maxsize=None)
def last_term_case(H, W, operands='fp64'):
    """act 0 conv term of the seeded conv_last case; operands 'fp16': map and weights rounded to fp16, bias not"""
    w, b = last_weights()
    x = feature_map('last', H, W)
    if operands == 'fp16':
        return _ro(conv_last_term(round_f16(x), round_f16(w), b))
    return _ro(conv_last_term(x, w, b))


@functools.lru_cache(maxsize=None)
def shuffle_case(h, w, act, operands='fp64'):
    wt, b = shuffle_weights()
    x = feature_map('ps', h, w)
    if operands == 'fp16':
        return _ro(pixel_shuffle_conv_ref(round_f16(x), round_f16(wt), b, act))
    return _ro(pixel_shuffle_conv_ref(x, wt, b, act))


CLAMP_HW = (37, 53)


@functools.lru_cache(maxsize=None)
def clamp_weights():
    """conv_last weights at twice the scale: the sum conv + frame then leaves [0, 1] on both sides for a good share of the pixels"""
    w, b = last_weights()
    return _ro(w * np.float32(2.0)), b


@functools.lru_cache(maxsize=None)
def clamp_case_ref():
    w, b = clamp_weights()
    return _ro(conv_last_ref(feature_map('last', *CLAMP_HW), w, b, frame_planes(*CLAMP_HW, 2), 2))


# ---------------------------------------------------------------- the layout case: a pixel-shuffle conv that only moves values
def identity_channel(c, sub):
    """the input channel that output channel c of sub-pixel sub = 2 dy + dx copies (a bijection in c for every sub)"""
    return (5 * c + 17 * sub + 3) % 64


@functools.lru_cache(maxsize=None)
def identity_shuffle_weights():
    """weight (256,64,3,3): conv channel 4c + sub has a single 1 at the centre tap of input channel identity_channel(c, sub); bias 0"""
    w = np.zeros((256, 64, 3, 3), np.float32)
    for c in range(64):
        for sub in range(4):
            w[4 * c + sub, identity_channel(c, sub), 1, 1] = 1.0
    return _ro(w), _ro(np.zeros(256, np.float32))


@functools.lru_cache(maxsize=None)
def identity_map(h, w):
    """(h,w,64) multiples of 1/512 in [-1, 1]: exact in fp16, so every route has to reproduce them bit for bit"""
    return _ro((syn.randint(SEED, 'id_x_%dx%d' % (h, w), (h, w, 64), -512, 512) / 512.0).astype(np.float32))


def identity_shuffle_expected(x):
    h, w, _ = x.shape
    out = np.empty((2 * h, 2 * w, 64), x.dtype)
    cs = np.arange(64)
    for sub in range(4):
        out[(sub >> 1)::2, (sub & 1)::2, :] = x[:, :, identity_channel(cs, sub)]
    return out


# ---------------------------------------------------------------- deliberately wrong variants (tests/test_head_ref.py)
def bilinear_x4_by_hand(planes, align_corners=False, clamp_low=True, edge='clamp'):
    """The x4 bilinear written out as the kernels write it, in float64, with the slips a kernel can make as switches:
    align_corners=True; clamp_low=False: the source coordinate is not clamped at 0 (truncation then extrapolates); edge='zero': the
    tap beyond the last row / column reads zero instead of the last row / column."""
    p = np.asarray(planes, np.float64)
    _, lh, lw = p.shape
    H, W = 4 * lh, 4 * lw

    def axis(n_out, n_in):
        d = np.arange(n_out, dtype=np.float64)
        s = d * (n_in - 1) / max(n_out - 1, 1) if align_corners else (d + 0.5) * 0.25 - 0.5
        if clamp_low:
            s = np.maximum(s, 0.0)
        i0 = np.trunc(s).astype(np.int64)
        i0 = np.minimum(i0, n_in - 1)
        lam = s - i0
        return i0, i0 + 1, lam

    y0, y1, ly = axis(H, lh)
    x0, x1, lx = axis(W, lw)
    if edge == 'clamp':
        pad = np.pad(p, ((0, 0), (0, 1), (0, 1)), mode='edge')
    else:
        pad = np.pad(p, ((0, 0), (0, 1), (0, 1)), mode='constant')
    ly, lx = ly[None, :, None], lx[None, None, :]
    g = lambda yy, xx: pad[:, yy[:, None], xx[None, :]]      # noqa: E731
    return (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))


def pixel_shuffle_swapped(conv_nchw):
    """F.pixel_shuffle(., 2) with (dy, dx) swapped: conv channel 4c + 2dy + dx lands on pixel (2y + dx, 2x + dy)"""
    n, c4, h, w = conv_nchw.shape
    t = conv_nchw.reshape(n, c4 // 4, 2, 2, h, w)              # (n, c, dy, dx, h, w)
    return t.permute(0, 1, 4, 3, 5, 2).reshape(n, c4 // 4, 2 * h, 2 * w)      # rows take dx, columns take dy


def unpermuted_bias(b):
    """The kernels read the pixel-shuffle bias as [sub][c], which the pack step makes from b[4c + sub].  Had it copied b as it is,
    conv channel 4c + sub would get b[64 sub + c]: that bias, per conv channel."""
    return np.ascontiguousarray(np.asarray(b).reshape(4, 64).T).reshape(256)
