"""An independent restatement of PSNR-B as include/pnpvcve.h states it (pnp_psnrb_*): every neighbour pair of the region is ENUMERATED,
sample by sample, and sorted by the boundary rule -- no slicing and no closed form for the counts, which are the lengths of the
enumerated lists.  Integer planes are summed in exact integers; the fp32 Y is subtracted in float32, squared in float64 and added with
math.fsum.  The value is formed with Python floats.  It shares no code with pnp_vcve_amd/metrics.py.

TEST INFRASTRUCTURE: used by tests/test_psnrb_ref.py (CPU) and tests/test_gpu_psnrb.py (GPU)."""
import functools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def pairs(rows, cols, crop, bp):
    """-> four (n, 2) arrays of flat sample indices: horizontal boundary, horizontal other, vertical boundary, vertical other pairs of
    the region rows [crop, rows - crop) x columns [crop, cols - crop) of a rows x cols plane; the grid starts at the plane's origin"""
    y0, y1, x0, x1 = crop, rows - crop, crop, cols - crop
    hb, hn, vb, vn = [], [], [], []
    for y in range(y0, y1):
        for x in range(x0, x1):
            if x + 1 < x1:
                (hb if (x + 1) % bp == 0 else hn).append((y * cols + x, y * cols + x + 1))
            if y + 1 < y1:
                (vb if (y + 1) % bp == 0 else vn).append((y * cols + x, (y + 1) * cols + x))
    return tuple(np.array(p, np.int64).reshape(-1, 2) for p in (hb, hn, vb, vn))


def counts(rows, cols, crop, bp):
    """(NBh, NNh, NBv, NNv) by enumeration"""
    return tuple(len(p) for p in pairs(rows, cols, crop, bp))


def _total(d):
    """the sum of the squares of the differences d: exact for integers, correctly rounded for float32 differences"""
    if np.issubdtype(d.dtype, np.integer):
        assert d.dtype == np.int64 and (not d.size or int(np.abs(d).max()) < 1 << 16) and d.size < 1 << 30       # no sum leaves 63 bits
        return int((d * d).sum())
    assert d.dtype == np.float32
    return math.fsum(float(v) * float(v) for v in d.tolist())


def plane_sums(a, b, crop, bp):
    """[sse, sbh, snh, sbv, snv] of one plane: Python ints for integer planes, floats for float32 planes.  b None: sse = 0."""
    rows, cols = a.shape
    exact = np.issubdtype(a.dtype, np.integer)
    fa = a.reshape(-1).astype(np.int64 if exact else np.float32)
    out = [0 if exact else 0.0]
    if b is not None:
        fb = b.reshape(-1).astype(fa.dtype)
        inside = np.array([y * cols + x for y in range(crop, rows - crop) for x in range(crop, cols - crop)], np.int64)
        out[0] = _total(fa[inside] - fb[inside])
    for p in pairs(rows, cols, crop, bp):
        out.append(_total(fa[p[:, 0]] - fa[p[:, 1]]) if len(p) else (0 if exact else 0.0))
    return out


def value(sums, cnt, bp, h, w, peak):
    """(PSNR-B, BEF, D_B, D_N) of one plane from its five sums and four counts; h x w: the region"""
    sse, sbh, snh, sbv, snv = (float(v) for v in sums)
    nbh, nnh, nbv, nnv = cnt
    d_b = (sbh + sbv) / (nbh + nbv) if nbh + nbv else 0.0
    d_n = (snh + snv) / (nnh + nnv) if nnh + nnv else 0.0
    eta = math.log2(bp) / math.log2(min(h, w))
    bef = eta * (d_b - d_n) if d_b > d_n else 0.0
    den = sse / (h * w) + bef
    return (math.inf if den == 0 else 10.0 * math.log10(peak * peak / den)), bef, d_b, d_n


def psnrb_plane(a, b, crop, bp, peak):
    """-> dict(sums, counts, value, bef) of one plane pair"""
    rows, cols = a.shape
    s = plane_sums(a, b, crop, bp)
    c = counts(rows, cols, crop, bp)
    v, bef, d_b, d_n = value(s, c, bp, rows - 2 * crop, cols - 2 * crop, peak)
    return dict(sums=s, counts=c, value=v, bef=bef, d_b=d_b, d_n=d_n)


def blocky_plane(rows, cols, d, bp, seed, noise=3, dx=0, dy=0):
    """a plane that is coded-looking: constant within the bp x bp blocks of a grid shifted by (dy, dx), plus a little noise -> the test
    plane; and a smooth reference (the block values without the noise, blurred once).  Values in [0, 2^d - 1]."""
    rng = np.random.RandomState(seed)
    top = (1 << d) - 1
    by, bx = (rows + dy + bp - 1) // bp + 1, (cols + dx + bp - 1) // bp + 1
    vals = rng.randint(top // 4, 3 * top // 4, size=(by, bx))
    base = np.kron(vals, np.ones((bp, bp), np.int64))[dy:dy + rows, dx:dx + cols]
    a = np.clip(base + rng.randint(-noise, noise + 1, size=(rows, cols)) * (1 << (d - 8)), 0, top)
    sm = base.astype(np.float64)
    sm[1:-1, 1:-1] = (sm[:-2, 1:-1] + sm[2:, 1:-1] + sm[1:-1, :-2] + sm[1:-1, 2:] + 4 * sm[1:-1, 1:-1]) / 8
    b = np.clip(np.rint(sm) + rng.randint(-1, 2, size=(rows, cols)), 0, top).astype(np.int64)
    return a.astype(np.int64), b


def block_constant(rows, cols, bp, seed, top=255):
    """exactly constant within each grid-aligned bp x bp block, random block values"""
    rng = np.random.RandomState(seed)
    vals = rng.randint(0, top + 1, size=((rows + bp - 1) // bp, (cols + bp - 1) // bp))
    return np.kron(vals, np.ones((bp, bp), np.int64))[:rows, :cols].astype(np.int64)
