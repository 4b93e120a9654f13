"""An independent restatement of the enhancement gain of include/pnpvcve.h (pnp_gain_*), for the tests: it loops over cells with
explicit slices and over pixels for the partition classes, in Python integers and math.fsum.  It shares no code with
pnp_vcve_amd/metrics.py."""
import math

import numpy as np

FORMATS = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}      # chroma format -> (sx, sy)
BLOCKS = (16, 32, 64, 128)


def grid_size(h, w, block):
    return (h + block - 1) // block, (w + block - 1) // block


def plane_rule(h, w, crop, block, plane, fmt):
    """plane 0 (Y, or a frame of pixels) | 1 | 2 -> (rows, cols, y0, y1, x0, x1, cell rows, cell columns)"""
    sx, sy = (1, 1) if plane == 0 else FORMATS[fmt]
    rows, cols, cy, cx = h // sy, w // sx, crop // sy, crop // sx
    return rows, cols, cy, rows - cy, cx, cols - cx, block // sy, block // sx


def cell_box(rule, i, j):
    """the samples of cell (i, j) inside the region: row and column slices (possibly empty)"""
    rows, cols, y0, y1, x0, x1, bh, bw = rule
    ya, yb = max(i * bh, y0), min((i + 1) * bh, y1)
    xa, xb = max(j * bw, x0), min((j + 1) * bw, x1)
    return slice(ya, max(ya, yb)), slice(xa, max(xa, xb))


def brute_counts(h, w, crop, block, plane=0, fmt='444'):
    """the samples of every cell inside the region by visiting every sample of the plane"""
    rule = plane_rule(h, w, crop, block, plane, fmt)
    rows, cols, y0, y1, x0, x1, bh, bw = rule
    gr, gc = grid_size(h, w, block)
    out = [[0] * gc for _ in range(gr)]
    for y in range(rows):
        for x in range(cols):
            if y0 <= y < y1 and x0 <= x < x1:
                out[y // bh][x // bw] += 1
    return np.array(out, np.int64)


def sq_errors(x, g):
    """(rows, cols[, C]) -> (rows, cols) squared errors, a pixel's channels added: Python-exact for integers (int64 here: far below
    2^63); for float32 luma one float32 subtraction, squared in float64"""
    x, g = np.asarray(x), np.asarray(g)
    if x.dtype == np.float32:
        assert g.dtype == np.float32
        d = np.subtract(x, g, dtype=np.float32).astype(np.float64)
    else:
        d = x.astype(np.int64) - g.astype(np.int64)
    e = np.multiply(d, d)
    return e if e.ndim == 2 else np.add.reduce(e, axis=2)


def cell_sums(e, rule, gr, gc):
    """(rows, cols) errors -> gr x gc nested list of the cells' sums: Python ints, or math.fsum of the float64 terms"""
    out = []
    for i in range(gr):
        row = []
        for j in range(gc):
            ys, xs = cell_box(rule, i, j)
            vals = e[ys, xs].reshape(-1).tolist()
            row.append(math.fsum(vals) if e.dtype == np.float64 else sum(int(v) for v in vals))
        out.append(row)
    return out


def gain_grid(a, l, g, crop, block, fmt=None):
    """a, l, g: (y, u, v) triples of (T, rows, cols) integer arrays of a clip of planes in format fmt; or (T, h, w, C) integer pixels; or
    (T, h, w) float32 luma -> (T, planes, gr, gc, 2) = E_a, E_l of every cell: int64, float64 for luma"""
    planes = [(a[k], l[k], g[k]) for k in range(3)] if isinstance(a, (tuple, list)) else [(a, l, g)]
    t, h, w = np.asarray(planes[0][0]).shape[:3]
    gr, gc = grid_size(h, w, block)
    is_f = np.asarray(planes[0][0]).dtype == np.float32
    out = np.zeros((t, len(planes), gr, gc, 2), np.float64 if is_f else np.int64)
    for k, (pa, pl, pg) in enumerate(planes):
        rule = plane_rule(h, w, crop, block, k, fmt)
        assert np.asarray(pa).shape[1:3] == rule[:2], (np.asarray(pa).shape, rule)
        for f in range(t):
            out[f, k, :, :, 0] = cell_sums(sq_errors(pa[f], pg[f]), rule, gr, gc)
            out[f, k, :, :, 1] = cell_sums(sq_errors(pl[f], pg[f]), rule, gr, gc)
    return out


def pixel_class(p0, p1, p2):
    return (1 if p0 != 0 else 0) | ((1 if p1 != 0 else 0) << 1) | ((1 if p2 != 0 else 0) << 2)


def gain_classes(a, l, g, par, crop):
    """the Y plane / the pixels of three clips (T, h, w[, C]) and par (T, 3, h, w) -> (T, 8, 3) = N, E_a, E_l of every class, pixel by
    pixel over the region"""
    t, h, w = np.asarray(a).shape[:3]
    is_f = np.asarray(a).dtype == np.float32
    out = np.zeros((t, 8, 3), np.float64 if is_f else np.int64)
    for f in range(t):
        ea, el = sq_errors(a[f], g[f]), sq_errors(l[f], g[f])
        terms = [[[], []] for _ in range(8)]
        count = [0] * 8
        for y in range(crop, h - crop):
            for x in range(crop, w - crop):
                k = pixel_class(par[f, 0, y, x], par[f, 1, y, x], par[f, 2, y, x])
                count[k] += 1
                terms[k][0].append(ea[y, x])
                terms[k][1].append(el[y, x])
        for k in range(8):
            out[f, k, 0] = count[k]
            for q in range(2):
                out[f, k, 1 + q] = math.fsum(float(v) for v in terms[k][q]) if is_f else sum(int(v) for v in terms[k][q])
    return out


def luma(rgb):
    """(..., 3) uint8 RGB -> float32 Y as include/pnpvcve.h states it for PNP_COLOR_Y: x_c = float32(byte) / 255 in float32;
    ((x_B 24.966 + x_G 128.553) + x_R 65.481 + 16) / 255 in float64; rounded to float32; times 255 in float32"""
    x = np.asarray(rgb).astype(np.float32) / np.float32(255.0)
    r, gr, b = (x[..., c].astype(np.float64) for c in range(3))
    y64 = (((b * 24.966 + gr * 128.553) + r * 65.481) + 16.0) / 255.0
    return y64.astype(np.float32) * np.float32(255.0)


def psnr(e, n, peak):
    return math.inf if e == 0 else 10.0 * math.log10(peak * peak * n / e)


def dpsnr(e_a, e_l):
    if e_a == 0 and e_l == 0:
        return 0.0
    if e_a == 0:
        return math.inf
    if e_l == 0:
        return -math.inf
    return 10.0 * math.log10(e_l / e_a)


def sd(values):
    m = math.fsum(values) / len(values)
    return math.sqrt(math.fsum((v - m) ** 2 for v in values) / len(values))
