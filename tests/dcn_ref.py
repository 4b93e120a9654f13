"""CPU reference, sample census and seeded inputs for the tests of the DCN kernel (pnp_vcve_amd/csrc/dcn.hip).  No GPU import.

dcn_reference   a plain float64 restatement of mmcv's modulated_deformable_im2col + the matmul (deform_groups 16), written
                independently of oracle/cpu_ref.py (tests/test_dcn_ref.py holds the two together to 1e-12).
dcn_bounds      the references and the tolerances of one case, from the reference alone (never from a kernel's output).
dcn_census      restates the kernel's WINDOW RULE only to classify samples (which path a sample takes, which edge it sits on); it
                never computes an expected value.
dcn_case        seeded builders of the inputs.  Offsets lie on a 1/8-px lattice and flows on a 1/4-px lattice, so every sample
                position is exact in fp32 and in fp64 and the edge classes (-1, 0, H-1, H, window edges) are hit exactly.

Layouts are those of ops.modulated_deform_conv_nhwc: x (h, w, 64) pixel-major, offset (288, h, w) = (group, tap, (dy, dx)),
mask_logits (144, h, w) = (group, tap), weight (64, 64, 3, 3), bias (64,), flow (2, h, w) = (dx, dy).  Results are (h, w, 64).
"""
import numpy as np

from pnp_vcve_amd import synthetic as syn

DG, CPG = 16, 4
F16_MAX = 65504.0
TILE_H, TILE_W, HALF_W, WIN, WR = 8, 16, 8, 16, 4
VARIANTS = (None, 'swap_dy_dx', 'le_last', 'ge_zero', 'border')


# ------------------------------------------------------------------------------------------------------------ reference
def _offsets_f32(offset, flow, h, w):
    """offset + flow.flip in fp32, as the kernel forms it -> (16, 9, 2, h, w) fp32, [..., 0] = dy."""
    off = np.ascontiguousarray(offset, np.float32).reshape(DG, 9, 2, h, w)
    if flow is not None:
        off = off + np.ascontiguousarray(flow, np.float32)[::-1][None, None]
    return off


def _positions(off, h, w, dt):
    """sample positions (16, 9, h, w) in dtype dt: (pixel + tap) + offset."""
    k = np.arange(9)
    gy = (np.arange(h)[None, :, None] + (k // 3 - 1)[:, None, None]).astype(dt)
    gx = (np.arange(w)[None, None, :] + (k % 3 - 1)[:, None, None]).astype(dt)
    return gy[None] + off[:, :, 0].astype(dt), gx[None] + off[:, :, 1].astype(dt)


def _sigmoid(m, dt):
    one = dt(1)
    with np.errstate(over='ignore'):
        return (one / (one + np.exp(-m.astype(dt)))).astype(dt)


def _bilinear_group(xg, py, px, h, w, variant, replicate):
    """dmcn_im2col_bilinear for one deform group: xg (4, h*w), py / px (9, h, w) -> (4, 9, h, w) in their dtype.
    `variant` names one of the WRONG rules the sensitivity tests need; `replicate` (9, h, w) marks samples read with clamped
    addresses and no validity test at all (what a kernel that clamps instead of testing would read)."""
    dt = py.dtype.type
    y0, x0 = np.floor(py), np.floor(px)
    ly, lx = py - y0, px - x0
    if variant == 'le_last':
        inside = (py > -1) & (px > -1) & (py <= h - 1) & (px <= w - 1)
    elif variant == 'ge_zero':
        inside = (py >= 0) & (px >= 0) & (py < h) & (px < w)
    else:
        inside = (py > -1) & (px > -1) & (py < h) & (px < w)
    free = np.ones_like(inside) if variant == 'border' else replicate
    val = np.zeros((CPG,) + py.shape, dt)
    for yy, xx, wt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                       (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
        ok = (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1) & inside
        if free is not None:
            ok = ok | free
        idx = (np.clip(yy, 0, h - 1) * w + np.clip(xx, 0, w - 1)).astype(np.int64)
        val += xg[:, idx] * (wt * ok.astype(dt))[None]
    return val


def _round_f16(v):
    """the project's fp16 operand rule: saturate to +-65504, round to nearest even."""
    return np.clip(v, -F16_MAX, F16_MAX).astype(np.float16).astype(np.float64)


def _evaluate(x, offset, mask_logits, weight, bias, flow, evals, drop=None, variant=None, replicate=None):
    """Runs the im2col once per sample dtype and feeds every evaluation in `evals`:
    name -> (sample dtype, sigmoid nudge in ulp, round operands to fp16, accumulate dtype).  -> name -> (h, w, 64) float64."""
    assert variant in VARIANTS, variant
    h, w, _ = x.shape
    off = _offsets_f32(offset, flow, h, w)
    if variant == 'swap_dy_dx':
        off, variant = off[:, :, ::-1], None
    ml = np.ascontiguousarray(mask_logits, np.float32).reshape(DG, 9, h, w)
    wmat = np.ascontiguousarray(weight, np.float32).reshape(64, DG, CPG * 9)
    out, sig, pos, xs, whole = {}, {}, {}, {}, {}
    for name, (sdt, nudge, r16, adt) in evals.items():
        out[name] = np.zeros((64, h * w), adt)
        if sdt not in pos:
            pos[sdt] = _positions(off, h, w, sdt)
            xs[sdt] = np.ascontiguousarray(np.asarray(x, np.float32).reshape(h * w, DG, CPG).transpose(1, 2, 0)).astype(sdt)
        if (sdt, nudge) not in sig:
            s = _sigmoid(ml, sdt)
            for _ in range(abs(nudge)):
                s = np.nextafter(s, sdt(2 if nudge > 0 else -1))
            sig[(sdt, nudge)] = s
    for g in range(DG):
        bil = {sdt: _bilinear_group(xs[sdt][g], pos[sdt][0][g], pos[sdt][1][g], h, w, variant,
                                    None if replicate is None else replicate[g]) for sdt in pos}
        for name, (sdt, nudge, r16, adt) in evals.items():
            col = bil[sdt] * sig[(sdt, nudge)][g][None]
            if drop is not None:
                col = col * (~drop[g]).astype(sdt)[None]
            wg = wmat[:, g]
            if r16:
                col, wg = _round_f16(col), _round_f16(wg)
            if adt is np.float32:                    # the fp32 evaluation is ONE matmul over K = 576, as the formulas have it
                whole.setdefault(name, []).append(col.reshape(CPG * 9, h * w))
            else:
                out[name] += wg.astype(adt) @ col.reshape(CPG * 9, h * w).astype(adt)
    for name, cols in whole.items():
        out[name] = wmat.reshape(64, 576) @ np.concatenate(cols, 0)
    b = np.asarray(bias, np.float32)
    return {name: np.ascontiguousarray((o + b.astype(o.dtype)[:, None]).astype(np.float64).T.reshape(h, w, 64))
            for name, o in out.items()}


_EVALS = {
    'fp64': (np.float64, 0, False, np.float64),
    'fp16': (np.float64, 0, True, np.float64),           # operands rounded to fp16 (saturating, RNE), accumulated in fp64
    'fp32-eval': (np.float32, 0, False, np.float32),     # the same formulas evaluated in fp32 throughout
}


def dcn_reference(x, offset, mask_logits, weight, bias, flow=None, operands='fp64', drop=None, variant=None, replicate=None):
    """mmcv.ops.modulated_deform_conv2d(x, offset + flow.flip, sigmoid(mask_logits), weight, bias, 1, 1, 1, 1, 16) in float64:
    a sample is taken only for -1 < h_im < H and -1 < w_im < W, validity is then decided corner by corner.
    operands: 'fp64' | 'fp16' | 'fp32-eval' (see _EVALS).  drop: bool (16, 9, h, w), samples whose contribution is zeroed.
    variant / replicate: deliberately WRONG rules for the sensitivity tests (see _bilinear_group).  -> (h, w, 64) float64."""
    return _evaluate(x, offset, mask_logits, weight, bias, flow, {operands: _EVALS[operands]}, drop, variant, replicate)[operands]


def dcn_bounds(x, offset, mask_logits, weight, bias, flow=None):
    """References and tolerances of one case, from the reference alone:
    e32   = max|fp32-eval - fp64|;  tol32 = min(16 * e32, 5e-5)
            (16: the hardware exp / rcp sigmoid is 1-2 ulp on the mask, i.e. of the order of the fp32 rounding per term, plus the
            MFMA summation order and the two-partial-tile sum; 5e-5 is the bound the suite already held the fp32 kernel to)
    n16   = max|ref16(samples from fp64) - ref16(samples from fp32-eval, sigmoid nudged 2 ulp either way)|: the reference's own
            noise from fp16 rounding ties that flip when the pre-rounding sample moves by an fp32 ulp, as the kernel's does
    tol16 = tol32 + 4 * n16."""
    evals = dict(_EVALS)
    evals['n16+'] = (np.float32, 2, True, np.float64)
    evals['n16-'] = (np.float32, -2, True, np.float64)
    r = _evaluate(x, offset, mask_logits, weight, bias, flow, evals)
    e32 = float(np.abs(r['fp32-eval'] - r['fp64']).max())
    n16 = float(max(np.abs(r['n16+'] - r['fp16']).max(), np.abs(r['n16-'] - r['fp16']).max()))
    tol32 = min(16 * e32, 5e-5)
    return dict(ref64=r['fp64'], ref16=r['fp16'], e32=e32, n16=n16, tol32=tol32, tol16=tol32 + 4 * n16)


# --------------------------------------------------------------------------------------------------------------- census
def dcn_census(offset, flow, h, w):
    """Classifies every sample (16, 9, h, w) by the kernel's window rule: an 8x16 tile, half s = columns tx0 + 8 s .., window
    origin (ty0 + floor(fy[c] + 0.5) - 4, tx0 + 8 s + floor(fx[c] + 0.5) - 4) with c = (min(ty0, H-1), min(tx0 + 8 s, W-1)),
    in-window <=> 0 <= ry, rx <= 14.  -> (dict class -> bool mask, dict wave-tap counts).  Classification only."""
    off = _offsets_f32(offset, flow, h, w)
    py, px = _positions(off, h, w, np.float32)          # the kernel's own fp32 positions (exact on the lattice)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    ty0, hx0 = (yy // TILE_H) * TILE_H + 0 * xx, (xx // HALF_W) * HALF_W + 0 * yy
    by = bx = np.zeros((h, w), np.float32)
    if flow is not None:
        fl = np.ascontiguousarray(flow, np.float32)
        cy, cx = np.minimum(ty0, h - 1), np.minimum(hx0, w - 1)
        by, bx = np.floor(fl[1][cy, cx] + np.float32(0.5)), np.floor(fl[0][cy, cx] + np.float32(0.5))
    oy, ox = ty0 + by.astype(np.int64) - WR, hx0 + bx.astype(np.int64) - WR
    fy_, fx_ = np.floor(py), np.floor(px)
    ry, rx = fy_.astype(np.int64) - oy[None, None], fx_.astype(np.int64) - ox[None, None]
    inw = (ry >= 0) & (ry <= WIN - 2) & (rx >= 0) & (rx <= WIN - 2)
    taken = (py > -1) & (px > -1) & (py < h) & (px < w)
    win, glob = inw & taken, ~inw & taken
    frac_y, frac_x = py != fy_, px != fx_
    near = ((ry == -1) | (ry == WIN - 1) | (rx == -1) | (rx == WIN - 1)) & (ry >= -1) & (ry <= WIN - 1) & (rx >= -1) & (rx <= WIN - 1)
    c = {
        'win_frac': win & frac_y & frac_x,
        'win_int': win & ~(frac_y & frac_x),
        'win_edge_lo': win & ((ry == 0) | (rx == 0)),
        'win_edge_hi': win & ((ry == WIN - 2) | (rx == WIN - 2)),
        'glob_near': glob & near,
        'glob_other': glob & ~near,
        'far': ~taken,
        # rejected by an exact boundary alone: the other coordinate would have let the sample through
        'exact_-1': ((py == -1) & (px >= -1) & (px <= w)) | ((px == -1) & (py >= -1) & (py <= h)),
        'exact_H_or_W': ((py == h) & (px >= -1) & (px <= w)) | ((px == w) & (py >= -1) & (py <= h)),
    }
    per_path = {
        'neg_partial': ((py > -1) & (py < 0)) | ((px > -1) & (px < 0)),
        'pos_partial': ((py > h - 1) & (py < h)) | ((px > w - 1) & (px < w)),
        'exact_0': (py == 0) | (px == 0),
        'exact_last': (py == h - 1) | (px == w - 1),
    }
    for name, m in per_path.items():
        c[name + '_win'] = m & win
        c[name + '_glob'] = m & glob
    # wave-taps: one tile, one row pair, 16 columns, deform groups 8 grp .. 8 grp + 7
    hp, wp = -(-h // TILE_H) * TILE_H, -(-w // TILE_W) * TILE_W

    def per_wave(m):
        p = np.zeros((DG, 9, hp, wp), np.int64)
        p[:, :, :h, :w] = m
        return p.reshape(2, 8, 9, hp // 2, 2, wp // TILE_W, TILE_W).sum(axis=(1, 4, 6))       # (grp, tap, row pair, tile x)
    n_fall, n_all = per_wave(glob), per_wave(np.ones_like(glob))
    live = n_all > 0
    waves = {
        'wave_none': int((live & (n_fall == 0)).sum()),
        'wave_mixed': int((live & (n_fall > 0) & (n_fall < n_all)).sum()),
        'wave_all': int((live & (n_fall == n_all)).sum()),
    }
    return c, waves


TAKEN_CLASSES = ('win_frac', 'win_int', 'win_edge_lo', 'win_edge_hi', 'glob_near', 'glob_other', 'neg_partial_win',
                 'neg_partial_glob', 'pos_partial_win', 'pos_partial_glob', 'exact_0_win', 'exact_0_glob', 'exact_last_win',
                 'exact_last_glob')
UNTAKEN_CLASSES = ('far', 'exact_-1', 'exact_H_or_W')


def census_counts(classes, waves):
    d = {k: int(v.sum()) for k, v in classes.items()}
    d.update(waves)
    return d


# ---------------------------------------------------------------------------------------------------------------- cases
GEOMETRY = ((1, 1), (5, 7), (8, 8), (3, 20), (13, 37), (8, 16), (9, 17), (64, 64))
PLANT_GROUPS = (3, 12)            # one deform group of each wave group
SPIKES = ((20, 20, 5, 1e6), (30, 10, 40, -1e6))          # (y, x, channel, value) of the saturation case


def _lattice(seed, name, shape, lo8, hi8, den=8.0):
    return (syn.randint(seed, name, shape, lo8, hi8).astype(np.float32) / np.float32(den)).astype(np.float32)


def _recipe(seed, h, w):
    """The main recipe at any frame size (regions that do not fit are clipped away by the slices)."""
    x = syn.uniform(seed, 'x', (h, w, 64), -1.0, 1.0)
    wt = syn.uniform(seed, 'w', (64, 64, 3, 3), -0.06, 0.06)
    b = syn.uniform(seed, 'b', (64,), -0.1, 0.1)
    ml = syn.uniform(seed, 'm', (DG, 9, h, w), -2.0, 2.0)
    # ---- flow (dx, dy): block-constant quarter-pel per 8x8 (the .5 ties of floor(f + 0.5) included, negatives too)
    bh, bw = -(-h // 8), -(-w // 8)
    blk = _lattice(seed, 'fl', (2, bh, bw), -32, 32, 4.0)
    flow = np.ascontiguousarray(np.repeat(np.repeat(blk, 8, 1), 8, 2)[:, :h, :w])
    flow[:, 16:24, 8:16] = _lattice(seed, 'flpix', (2, h, w), -32, 32, 4.0)[:, 16:24, 8:16]      # one half with per-pixel flow
    flow[0, 24:32, 32:40] = 60.0                         # the whole window outside the frame
    flow[1, 24:32, 32:40] = -60.0
    for cx in (16, 24):                                  # the first pixel's flow, which places the window, is 20 px off the rest:
        flow[:, 8:9, cx:cx + 1] += 20.0                  # wave_all through the flow.  In BOTH halves of one tile of the quiet row: a
                                                         # wave spans the tile's 16 columns, so one half alone only gives wave_mixed
    # ---- offsets (dy, dx) on the 1/8 lattice, U(-3.25, 3.25): straddles the window edge
    off = _lattice(seed, 'off', (DG, 9, 2, h, w), -26, 26)
    off[::7] = np.round(off[::7])                        # every 7th deform group: integer offsets
    off[:, :, :, :min(2, h // 8)] *= 8.0                 # two top rows (one / none in a frame below 16 / 8 rows): far out of frame
    # ---- planted exact positions, on striped pixels, for two deform groups and all 9 taps: the sample's y (or x) is exactly one
    #      of -1, -0.5, 0, last, last + 0.5, last + 1.  Half of them are planted for the run WITH the flow, half for the run without.
    k = np.arange(9)
    yy, xx = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    stripe = np.broadcast_to((yy + 2 * xx) % 3 == 0, (9, h, w))
    for gi, g in enumerate(PLANT_GROUPS):
        sel = syn.randint(seed, 'plant%d' % gi, (9, h, w), 0, 23)        # target (6) x axis (2) x with / without flow (2)
        tgt, axis, wf = sel % 6, (sel // 6) % 2, sel // 12
        for a, n, tap, pix in ((0, h, (k // 3 - 1)[:, None, None] + 0 * xx, yy), (1, w, (k % 3 - 1)[:, None, None] + 0 * yy, xx)):
            want = np.choose(tgt, [-1.0, -0.5, 0.0, n - 1.0, n - 0.5, float(n)]).astype(np.float32)
            val = want - (pix + tap).astype(np.float32) - np.where(wf == 1, flow[1 - a][None], np.float32(0))
            m = stripe & (axis == a)
            off[g, :, a][m] = val[m].astype(np.float32)
    # ---- one tile 6.5 - 8 px off, towards the frame's centre: wave_all (planted positions excluded: some of them are not taken)
    ys, xs = slice(16, 24), slice(16, 32)
    mag = _lattice(seed, 'mag', (DG, 9, 2, h, w), 52, 64)
    sy = np.where(np.arange(h) // 8 * 8 < h / 2, 1.0, -1.0).astype(np.float32)[:, None]       # one direction per tile
    sx = np.where(np.arange(w) // 16 * 16 < w / 2, 1.0, -1.0).astype(np.float32)[None, :]
    off[:, :, 0, ys, xs] = (mag[:, :, 0] * sy)[:, :, ys, xs]
    off[:, :, 1, ys, xs] = (mag[:, :, 1] * sx)[:, :, ys, xs]
    # ---- a quiet tile row, |off| <= 1.5: waves without any fallback (planted positions excluded)
    off[:, :, :, 8:16] = _lattice(seed, 'quiet', (DG, 9, 2, h, w), -12, 12)[:, :, :, 8:16]
    # ---- a handful of offsets +-1e9 and of logits +-90
    n = 6
    pg, pk, pc = syn.randint(seed, 'hg', (n,), 0, DG - 1), syn.randint(seed, 'hk', (n,), 0, 8), syn.randint(seed, 'hc', (n,), 0, 1)
    py_, px_ = syn.randint(seed, 'hy', (n,), 0, h - 1), syn.randint(seed, 'hx', (n,), 0, w - 1)
    for i in range(n):
        off[pg[i], pk[i], pc[i], py_[i], px_[i]] = 1e9 if i % 2 else -1e9
        ml[pg[(i + 1) % n], pk[i], py_[(i + 2) % n], px_[(i + 3) % n]] = 90.0 if i % 2 else -90.0
    return dict(x=x, offset=np.ascontiguousarray(off.reshape(288, h, w)), mask_logits=np.ascontiguousarray(ml.reshape(144, h, w)),
                weight=wt, bias=b, flow=flow)


def strip_walk_width(grid):
    """W = 16 k - 4 with k the smallest value that makes 3 k >= 2 * grid + 8 (H = 20: three tile rows, the last one ragged):
    every block of a `grid`-block launch then walks 2 or more tiles and some walk 3."""
    k = -(-(2 * grid + 8) // 3)
    return 16 * k - 4


def dcn_case(name, grid=None):
    """-> dict(x, offset, mask_logits, weight, bias, flow).  Names: 'main_44x52', 'geo_<h>x<w>', 'flow_folded' (flow None,
    offset + flow pre-added in fp32), 'strip_walk' (needs the launch's grid), 'saturation' (main + two activations of +-1e6)."""
    if name == 'main_44x52':
        return _recipe(41, 44, 52)
    if name.startswith('geo_'):
        h, w = (int(v) for v in name[4:].split('x'))
        return _recipe(100 + h * 131 + w, h, w)
    if name == 'flow_folded':
        c = dcn_case('main_44x52')
        c['offset'] = np.ascontiguousarray(_offsets_f32(c['offset'], c['flow'], 44, 52).reshape(288, 44, 52))
        c['flow'] = None
        return c
    if name == 'saturation':
        c = dcn_case('main_44x52')
        for y, x, ch, v in SPIKES:
            c['x'][y, x, ch] = v
        return c
    if name == 'strip_walk':
        h, w = 20, strip_walk_width(grid)
        m = dcn_case('main_44x52')
        reps = -(-w // 52)
        c = dict(weight=m['weight'], bias=m['bias'], x=syn.uniform(43, 'x', (h, w, 64), -1.0, 1.0))
        for key in ('offset', 'mask_logits', 'flow'):   # the main case, tiled: 52 is no multiple of 16, so consecutive tiles differ
            c[key] = np.ascontiguousarray(np.tile(m[key][:, :h], (1, 1, reps))[:, :, :w])
        return c
    raise KeyError(name)
