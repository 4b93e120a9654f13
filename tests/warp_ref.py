"""CPU reference, sample census and seeded inputs for the tests of the MV-alignment warp kernels (pnp_vcve_amd/csrc/warp.hip).
numpy only: no torch, no import of the package.

coords        the reference's coordinate chain (flow_warp.py:41-42 + ATen's align_corners=True un-normalise), every operation
              rounded to float32 in the order the kernels' sample_coords documents -> meant to be the kernels' ix, iy bit for bit.
warp_ref      float64 4-tap sum (or the nearest pixel) over those fp32 coordinates; zeros outside the frame.  The private
              `_mutant` switch evaluates one of the WRONG rules the sensitivity tests need (MUTANTS).
warp_tol      6 * 2^-24 * max|x|, derived below from the reference alone.
warp_census   classifies the samples of one case (taps inside / outside the frame, exact hits on -1, 0, size-1, size, ties of the
              nearest rounding, non-finite chains); never computes an expected value.
warp_case     seeded builders of the inputs, by name (see nhwc_cases / nchw_cases).

Layouts: x (h, w, c) pixel-major and flow (h, w, 2) = (dx, dy), as ops.mv_warp_nhwc takes them (flow planes [..., 0], [..., 1]);
the NCHW drop-in's x (n, c, h, w), flow (n, h, w, 2) go through warp_ref_nchw.
"""
import zlib

import numpy as np

F32 = np.float32
F16_MAX = 65504.0
# the wrong kernels the sensitivity tests evaluate:
#   le_edge      `<=` for `<` at the right and bottom edge (the tap reads what pixel-major memory holds there)
#   clamp        taps outside the frame clamped to the border instead of zeroed
#   half_away    nearest: round half away from zero instead of ties to even
#   direct       ix = x + fx instead of the normalise / un-normalise chain
#   swap_w       wx0 and wx1 swapped
#   no_row_mask  the 64-kernel's second row of a row pair without its `y < H` mask: at an odd H the absent row H is computed from the
#                flow of the row above it and lands on that row
MUTANTS = ('le_edge', 'clamp', 'half_away', 'direct', 'swap_w', 'no_row_mask')
MUTANT_MODES = {'le_edge': ('bilinear', 'nearest'), 'clamp': ('bilinear', 'nearest'), 'half_away': ('nearest',),
                'direct': ('bilinear', 'nearest'), 'swap_w': ('bilinear',), 'no_row_mask': ('bilinear', 'nearest')}


# ------------------------------------------------------------------------------------------------------------ reference
def coords(h, w, flow, _direct=False, _last_row_as=None):
    """flow (..., h, w, 2) = (dx, dy) -> (ix, iy) float32 (..., h, w): px = x + fx; nx = 2 px / max(w-1, 1) - 1;
    ix = ((nx + 1) / 2) (w - 1), each operation rounded to float32 (numpy float32 arithmetic is correctly rounded, as HIP's is
    without fast-math; no product feeds a sum here, so nothing can contract into an FMA).  The same for y.
    _direct: the WRONG chain ix = px.  _last_row_as: the WRONG pixel row number of the last row (mutant 'no_row_mask')."""
    fl = np.asarray(flow, F32)
    assert fl.shape[-3:] == (h, w, 2), fl.shape
    gx = np.arange(w, dtype=F32)[None, :]
    gy = np.arange(h, dtype=F32)
    if _last_row_as is not None:
        gy[-1] = _last_row_as
    gy = gy[:, None]
    with np.errstate(all='ignore'):
        px, py = gx + fl[..., 0], gy + fl[..., 1]
        if _direct:
            return px, py
        nx = F32(2) * px / F32(max(w - 1, 1)) - F32(1)
        ny = F32(2) * py / F32(max(h - 1, 1)) - F32(1)
        ix = ((nx + F32(1)) / F32(2)) * F32(w - 1)
        iy = ((ny + F32(1)) / F32(2)) * F32(h - 1)
    assert ix.dtype == F32 and iy.dtype == F32
    return ix, iy


def _gather(xf, ty, tx, h, w, rule):
    """xf (h*w, c) float64; ty / tx integer-valued float64 (h, w), possibly huge or NaN -> (values (h, w, c), taken (h, w)).
    rule None: the pixel if 0 <= tx < w and 0 <= ty < h, else no tap.  'le_edge': `<=` at the right and bottom edge; the tap
    then reads what pixel-major memory holds there (the next row's first pixel; nothing past the map's end).  'clamp': border
    replicate."""
    with np.errstate(invalid='ignore'):
        fin = np.isfinite(ty) & np.isfinite(tx)
        ty, tx = np.where(fin, ty, -9.0), np.where(fin, tx, -9.0)
        if rule == 'le_edge':
            flat = ty * w + tx
            ok = (tx >= 0) & (tx <= w) & (ty >= 0) & (ty <= h) & (flat < h * w)
            idx = np.clip(flat, 0, h * w - 1)
        else:
            ok = fin if rule == 'clamp' else (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
            idx = np.clip(ty, 0, h - 1) * w + np.clip(tx, 0, w - 1)
    return xf[idx.astype(np.int64).reshape(-1)].reshape(h, w, -1), ok


def warp_ref(x, flow, mode='bilinear', _mutant=None):
    """flow_warp(x, flow, mode, 'zeros', align_corners=True) of one (h, w, c) map in float64, on the fp32 coordinates of coords().

    bilinear: x0 = floor(ix), wx1 = ix - x0 (exact in fp32 wherever a tap is inside the frame), wx0 = float32(1 - wx1) (the one
              rounding the kernels share with ATen), the same for y; the four products w * w and the 4-tap sum in float64; a tap
              outside [0, w) x [0, h) contributes 0.
    nearest:  the pixel at rint (ties to even) of ix, iy if it lies inside the frame, else 0 -- a copy, so the values are exact.
    A non-finite ix or iy (an infinite or NaN vector, or one whose chain overflows, such as 3e38) has no tap and gives 0 in both
    modes.  That is the kernels' documented choice (sample_coords clamps such a coordinate to where no tap is valid); ATen's
    bilinear grid_sample returns NaN at those pixels, its nearest mode 0."""
    assert mode in ('bilinear', 'nearest') and (_mutant is None or _mutant in MUTANTS)
    x = np.asarray(x, F32)
    h, w, c = x.shape
    last = F32(h) if (_mutant == 'no_row_mask' and h % 2) else None       # the absent second row of the last pair lands on h-1
    ix, iy = coords(h, w, flow, _direct=(_mutant == 'direct'), _last_row_as=last)
    assert ix.shape == (h, w)
    xf = x.reshape(h * w, c).astype(np.float64)
    rule = _mutant if _mutant in ('le_edge', 'clamp') else None
    with np.errstate(invalid='ignore'):
        if mode == 'nearest':
            if _mutant == 'half_away':
                rnd = lambda v: np.sign(v) * np.floor(np.abs(v.astype(np.float64)) + 0.5)          # noqa: E731
            else:
                rnd = lambda v: np.rint(v).astype(np.float64)                                      # noqa: E731
            v, ok = _gather(xf, rnd(iy), rnd(ix), h, w, rule)
            return np.where(ok[..., None], v, 0.0)
        x0, y0 = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - x0, iy - y0
        wx0, wy0 = F32(1) - wx1, F32(1) - wy1
        assert wx0.dtype == F32
        if _mutant == 'swap_w':
            wx0, wx1 = wx1, wx0
        x0, y0 = x0.astype(np.float64), y0.astype(np.float64)
        out = np.zeros((h, w, c), np.float64)
        for dy, dx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
            v, ok = _gather(xf, y0 + dy, x0 + dx, h, w, rule)
            wt = np.where(ok, wy.astype(np.float64) * wx.astype(np.float64), 0.0)
            out += np.where(ok[..., None], v * wt[..., None], 0.0)
    return out


def warp_ref_nchw(x, flow, mode='bilinear', _mutant=None):
    """x (n, c, h, w), flow (n, h, w, 2) -> (n, c, h, w) float64"""
    return np.stack([warp_ref(np.ascontiguousarray(x[i].transpose(1, 2, 0)), flow[i], mode, _mutant).transpose(2, 0, 1)
                     for i in range(x.shape[0])])


def warp_tol(x):
    """6 * 2^-24 * max|x|: what an fp32 kernel may differ from warp_ref by, from the reference alone.

    warp_ref already carries the kernels' fp32 ix, iy, wx1, wy1 and the rounded wx0, wy0, so its weights ARE the kernels' factors.
    What an fp32 evaluation adds per output, in units of u = 2^-24 (half an ulp, relative), with M = max|x|, weights in [0, 1] whose
    four products sum to 1 + O(u):
      * one rounding of each product w * w:            the four errors are <= u w w each, together <= u M (1 + O(u));
      * one rounding of each v * (w w):                 <= u |v| w w each, together <= u M   (none under FMA);
      * three additions of partial sums bounded by M (1 + O(u)):  <= u M each, 3 u M.
    That is 5 u M; the sixth unit covers the second-order terms and the O(u) excess of the weight sum.  Nearest is a copy: no
    tolerance, array_equal."""
    return 6.0 * 2.0 ** -24 * float(np.abs(np.asarray(x, np.float64)).max())


def h16(a):
    """the project's fp16 rule: saturate to +-65504, round to nearest even -> float16 (dcn_ref._round_f16's rule; restated
    because dcn_ref imports the package, and torch with it)"""
    return np.clip(np.asarray(a, np.float64), -F16_MAX, F16_MAX).astype(np.float16)


# --------------------------------------------------------------------------------------------------------------- census
def warp_census(h, w, flow):
    """Shares and counts over the h * w samples of one map.  A tap counts where its bilinear weight is not zero.
    inside / outside: at least one such tap inside / outside the frame.  x_-1 ... y_h: samples whose fp32 ix (iy) is exactly -1, 0,
    size-1, size, with the other coordinate close enough for the sample to matter (-1 <= . <= size).  ties: rint decides a .5 in x
    or y, with the other coordinate's pixel inside the frame.  edge_ties: ties between a pixel and zero (-0.5, size-0.5).
    nonfinite: ix or iy is not finite."""
    ix, iy = coords(h, w, flow)
    with np.errstate(invalid='ignore'):
        fin = np.isfinite(ix) & np.isfinite(iy)
        x0, y0 = np.floor(ix), np.floor(iy)
        fx, fy = ix - x0, iy - y0
        inx = ((x0 >= 0) & (x0 <= w - 1) & (fx < 1)) | ((x0 + 1 >= 0) & (x0 + 1 <= w - 1) & (fx > 0))
        iny = ((y0 >= 0) & (y0 <= h - 1) & (fy < 1)) | ((y0 + 1 >= 0) & (y0 + 1 <= h - 1) & (fy > 0))
        outx = ~(((x0 >= 0) & (x0 <= w - 1)) | (fx == 1)) | ~(((x0 + 1 >= 0) & (x0 + 1 <= w - 1)) | (fx == 0))
        outy = ~(((y0 >= 0) & (y0 <= h - 1)) | (fy == 1)) | ~(((y0 + 1 >= 0) & (y0 + 1 <= h - 1)) | (fy == 0))
        nearx, neary = (ix >= -1) & (ix <= w), (iy >= -1) & (iy <= h)
        tx, ty = np.abs(fx - F32(0.5)) == 0, np.abs(fy - F32(0.5)) == 0
        rx, ry = np.rint(ix), np.rint(iy)
        pinx, piny = (rx >= 0) & (rx <= w - 1), (ry >= 0) & (ry <= h - 1)
        n = float(h * w)
        d = {'inside': float((fin & inx & iny).sum()) / n, 'outside': float((~fin | outx | outy).sum()) / n,
             'ties': float(((tx & piny & nearx) | (ty & pinx & neary)).sum()) / n,
             'edge_ties': int((((ix == F32(-0.5)) | (ix == F32(w - 0.5))) & piny).sum()
                              + (((iy == F32(-0.5)) | (iy == F32(h - 0.5))) & pinx).sum()),
             'nonfinite': int((~fin).sum())}
        for name, v in (('-1', -1.0), ('0', 0.0), ('last', None), ('size', None)):
            vx = {'last': w - 1.0, 'size': float(w)}.get(name, v)
            vy = {'last': h - 1.0, 'size': float(h)}.get(name, v)
            d['x_' + name] = int(((ix == chain_image(w, vx)) & neary).sum())
            d['y_' + name] = int(((iy == chain_image(h, vy)) & nearx).sum())
    return d


def chain_image(size, v):
    """what the fp32 chain makes of a sample aimed at px = v on an axis of `size` pixels.  0, size-1 and size come back exactly at
    every size; -1 does wherever size-1 is a power of two and at some other sizes, but e.g. not at 16 (-0.99999994), 47
    (-0.99999976), 64 (-0.99999994) and 96 (-0.99999845): there the reference itself (and ATen) puts a weight of 1e-7 .. 1.5e-6 on
    the edge pixel, and so must the kernels."""
    f = np.zeros((1, size, 2), F32)
    f[0, :, 0] = F32(v) - np.arange(size, dtype=F32)
    return coords(1, size, f)[0][0, 0]


def census_line(d):
    return ' '.join(('%s=%.2f' if isinstance(v, float) else '%s=%d') % (k, v) for k, v in d.items())


# ---------------------------------------------------------------------------------------------------------------- cases
FRAMES = ((1, 1), (1, 5), (2, 16), (3, 17), (5, 33), (17, 47), (64, 96))
KINDS = ('edge', 'half', 'frac', 'oob', 'block', 'wild')
CHANNELS_64, CHANNELS_GENERAL = 64, (4, 8, 60, 128)
NCHW_FRAMES, NCHW_N, NCHW_C = ((3, 17), (17, 47), (64, 96)), (1, 2), (1, 3, 8)
BIG = 'c128_258x256_frac'         # 258 * 256 * 32 = 2 113 536 float4 > the general kernel's 256 * 32 blocks * 256 threads
WILD = (1e9, -1e9, 2.0 ** 31, -2.0 ** 31, 2.0 ** 24 + 1, 3e38, -3e38, np.inf, -np.inf, np.nan, 0.0, 1.0)
SPIKE, SAT_SCALE = 1e6, 1000.0
# seeds: crc32 of the case's name plus, where the first draw misses a census condition of tests/test_warp_ref.py, a bump
_SEED_BUMP = {
    'c128_2x16_block': 3, 'c128_2x16_edge': 1, 'c128_3x17_edge': 1, 'c128_3x17_half': 4, 'c128_5x33_block': 1,
    'c4_2x16_block': 8, 'c4_2x16_edge': 4, 'c4_2x16_half': 2, 'c4_3x17_block': 5, 'c4_3x17_half': 1, 'c60_2x16_block': 16,
    'c60_3x17_block': 5, 'c60_3x17_edge': 1, 'c60_3x17_half': 1, 'c60_5x33_block': 1, 'c64_17x47_block': 1, 'c64_2x16_block': 1,
    'c64_2x16_edge': 4, 'c64_2x16_half': 3, 'c64_3x17_block': 2, 'c64_3x17_half': 2, 'c8_2x16_half': 1, 'c8_3x17_block': 3,
    'c8_3x17_edge': 2, 'c8_3x17_half': 1, 'c8_5x33_block': 1, 'c8_5x33_half': 1, 'n1_c1_17x47_block': 3, 'n1_c1_3x17_block': 1,
    'n1_c8_17x47_block': 2, 'n1_c8_3x17_block': 1, 'n1_c8_3x17_edge': 1, 'n1_c8_3x17_half': 3, 'n2_c1_17x47_block': 2,
    'n2_c1_3x17_block': 1, 'n2_c1_3x17_half': 1, 'n2_c3_17x47_block': 5, 'n2_c3_3x17_block': 16, 'n2_c3_3x17_edge': 1,
    'n2_c3_3x17_half': 3, 'n2_c8_3x17_half': 5,
}


def nhwc_cases(channels=(CHANNELS_64,) + CHANNELS_GENERAL):
    return ['c%d_%dx%d_%s' % ((c,) + f + (k,)) for c in channels for f in FRAMES for k in KINDS]


def nchw_cases():
    return ['n%d_c%d_%dx%d_%s' % ((n, c) + f + (k,)) for n in NCHW_N for c in NCHW_C for f in NCHW_FRAMES for k in KINDS]


def parse(name):
    """-> dict(n (None for a pixel-major case), c, h, w, kind, sat)"""
    parts = name.split('_')
    n = int(parts.pop(0)[1:]) if parts[0][0] == 'n' else None
    c = int(parts[0][1:])
    h, w = (int(v) for v in parts[1].split('x'))
    assert parts[2] in KINDS and parts[3:] in ([], ['sat']), name
    return dict(n=n, c=c, h=h, w=w, kind=parts[2], sat=parts[3:] == ['sat'])


def _quarter_targets(rs, size, shape):
    lo = np.arange(-1.25, 0.5 + 0.01, 0.25)
    hi = np.arange(size - 1.5, size + 0.25 + 0.01, 0.25)
    return rs.choice(np.concatenate([lo, hi]), shape)


def _half_targets(rs, size, shape):
    """the half-integer grid over [-1.5, size + 0.5]: half of the draws from the six positions about the two edges, the others
    from the whole range, three of four of those on an odd half (a tie of the nearest rounding)"""
    edge = rs.choice(np.array([-1.5, -1.0, -0.5, size - 0.5, size, size + 0.5]), shape)
    odd = rs.randint(-2, size + 1, shape) + 0.5
    whole = rs.randint(-1, size + 1, shape).astype(np.float64)
    inner = np.where(rs.randint(0, 4, shape) > 0, odd, whole)
    return np.where(rs.randint(0, 2, shape) > 0, edge, inner)


def make_flow(rs, kind, h, w):
    """-> (h, w, 2) float32 = (dx, dy)"""
    gx, gy = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    if kind == 'edge':          # absolute targets on the quarter-pel grid about both edges of each axis; flow = target - position
        f = np.stack([_quarter_targets(rs, w, (h, w)) - gx, _quarter_targets(rs, h, (h, w)) - gy], -1)
    elif kind == 'half':
        f = np.stack([_half_targets(rs, w, (h, w)) - gx, _half_targets(rs, h, (h, w)) - gy], -1)
    elif kind == 'frac':
        f = np.stack([rs.uniform(-min(8.0, w / 2.0), min(8.0, w / 2.0), (h, w)),
                      rs.uniform(-min(8.0, h / 2.0), min(8.0, h / 2.0), (h, w))], -1)
    elif kind == 'oob':
        f = rs.uniform(-1.5 * w, 1.5 * w, (h, w, 2))
    elif kind == 'block':       # golden_util's quarter-pel vectors in +-8, constant over 8x8 blocks (the last ones cropped)
        blk = rs.randint(-32, 33, (-(-h // 8), -(-w // 8), 2)) / 4.0
        f = np.repeat(np.repeat(blk, 8, axis=0), 8, axis=1)[:h, :w]
    elif kind == 'wild':
        f = rs.choice(np.array(WILD), (h, w, 2))
    else:
        raise KeyError(kind)
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(f.astype(F32))


def _one(rs, p):
    h, w, c = p['h'], p['w'], p['c']
    x = rs.uniform(-1.0, 1.0, (h, w, c)).astype(F32)
    flow = make_flow(rs, p['kind'], h, w)
    if p['sat']:                # features x 1000 and one activation of 1e6, at a pixel that a sample reads with weight >= 1/4
        x *= F32(SAT_SCALE)
        ix, iy = coords(h, w, flow)
        with np.errstate(invalid='ignore'):
            rx, ry = np.rint(ix), np.rint(iy)
            hit = np.argwhere((rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1))
        assert len(hit), 'no sample lands in the frame'
        y, xx = hit[len(hit) // 2]
        x[int(ry[y, xx]), int(rx[y, xx]), 3 % c] = F32(SPIKE)
    return x, flow


def warp_case(name):
    """-> dict(x, flow), float32.  'c<C>_<h>x<w>_<kind>[_sat]': x (h, w, C), flow (h, w, 2).
    'n<N>_c<C>_<h>x<w>_<kind>': x (N, C, h, w), flow (N, h, w, 2) for the NCHW drop-in."""
    p = parse(name)
    rs = np.random.RandomState((zlib.crc32(name.encode()) + _SEED_BUMP.get(name, 0)) & 0x7FFFFFFF)
    if p['n'] is None:
        x, flow = _one(rs, p)
        return dict(x=x, flow=flow)
    xs, flows = zip(*[_one(rs, p) for _ in range(p['n'])])
    return dict(x=np.ascontiguousarray(np.stack(xs).transpose(0, 3, 1, 2)), flow=np.stack(flows))
