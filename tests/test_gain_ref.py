"""CPU: the enhancement gain as include/pnpvcve.h states it (pnp_gain_*).

* pnp_vcve_amd.metrics.gain_sums / gain_cell_counts / gain_values / gain_sd / gain_yuv (the numpy host path, which reshapes and counts in
  closed form, and whose fp64 part ops.gain_* and BasicVSR.evaluate run on the device's sums) against the independent restatement
  tests/gain_ref.py, which loops over cells and pixels: integer sums equal, fp64 sums and values to 1e-12 relative -- the bound the
  project uses for two fp64 restatements of one formula (tests/test_psnrb_ref.py);
* the grid summed over its cells against the squared error the existing host psnr() path scores;
* pnp_gain_grid / pnp_gain_cell_count / pnp_gain_luma_tiles of the C ABI (host calls, no GPU) against enumeration, and the entries'
  refusals with null device pointers, decided before any HIP call;
* csrc/gain_plan.h on the host under AddressSanitizer + UBSan: a stand-alone program (tests/host/gain_stub.cpp) run as a subprocess;
  nothing is loaded into this interpreter."""
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import gain_ref as ref
from pnp_vcve_amd import _native, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 1001
A = 0x1000        # an aligned "device address": never dereferenced on these paths
T = 3
SIZES = [(64, 80), (66, 78), (130, 70)]
BLOCKS = (16, 64)
CROPS = (0, 2, 6)


def rel(got, want):
    if math.isinf(want) or math.isinf(got):
        return 0.0 if got == want else math.inf
    return abs(got - want) / abs(want) if want else abs(got)


def planes_clip(seed, h, w, fmt, depth):
    """(y, u, v) of T frames of seeded random sample values"""
    rng = np.random.RandomState(seed)
    sx, sy = ref.FORMATS[fmt]
    return tuple(rng.randint(0, 1 << depth, (T, hh, ww)).astype(np.int32) for hh, ww in ((h, w), (h // sy, w // sx), (h // sy, w // sx)))


def near(g, seed, spread, top):
    """a clip that differs from g by at most `spread` per sample: the errors of a codec, not of noise"""
    rng = np.random.RandomState(seed)
    return tuple(np.clip(p + rng.randint(-spread, spread + 1, p.shape), 0, top).astype(p.dtype) for p in g) if isinstance(g, tuple) else \
        np.clip(g.astype(np.int64) + rng.randint(-spread, spread + 1, g.shape), 0, top).astype(g.dtype)


@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('fmt', ['420', '422', '444'])
@pytest.mark.parametrize('h,w', SIZES)
def test_plane_sums_are_the_restatements(h, w, fmt, depth):
    top = (1 << depth) - 1
    g = planes_clip(h + depth, h, w, fmt, depth)
    a, l = near(g, 1, 9, top), near(g, 2, 14, top)
    for block in BLOCKS:
        for crop in CROPS:
            want = ref.gain_grid(a, l, g, crop, block, fmt)
            got, classes = metrics.gain_sums(a, l, g, crop, block, fmt)
            assert classes is None and got.dtype == np.int64 and got.shape == (T, 3) + ref.grid_size(h, w, block) + (2,)
            assert np.array_equal(got, want), (block, crop)
            assert (want.sum(axis=(2, 3))[:, 0] > 0).all()          # every frame has an E_a and an E_l
            # the grid summed over its cells is the squared error of the cropped planes
            for k in range(3):
                rows, cols, y0, y1, x0, x1, _, _ = ref.plane_rule(h, w, crop, block, k, fmt)
                for q, x in enumerate((a, l)):
                    d = x[k][:, y0:y1, x0:x1].astype(np.int64) - g[k][:, y0:y1, x0:x1].astype(np.int64)
                    assert np.array_equal(got[:, k, :, :, q].sum(axis=(1, 2)), (d * d).sum(axis=(1, 2)))


@pytest.mark.parametrize('h,w', SIZES)
def test_rgb_bytes_and_luma_sums_are_the_restatements_and_the_sse_of_the_host_psnr(h, w):
    rng = np.random.RandomState(h)
    g = rng.randint(0, 256, (T, h, w, 3)).astype(np.uint8)
    a, l = near(g, 3, 9, 255), near(g, 4, 14, 255)
    ya, yl, yg = (ref.luma(x) for x in (a, l, g))
    assert ya.dtype == np.float32
    # the restatement's luma is the host path's (two statements of one arithmetic): metrics.bgr2y takes BGR in [0, 1]
    assert np.array_equal(ya[0], metrics.bgr2y(a[0][..., ::-1].astype(np.float32) / 255.) * 255.)
    worst = 0.0
    for block in BLOCKS:
        for crop in CROPS:
            want = ref.gain_grid(a, l, g, crop, block)
            got, _ = metrics.gain_sums(a, l, g, crop, block)
            assert got.dtype == np.int64 and got.shape == (T, 1) + ref.grid_size(h, w, block) + (2,) and np.array_equal(got, want), (block, crop)
            wy = ref.gain_grid(ya, yl, yg, crop, block)
            gy, _ = metrics.gain_sums(ya, yl, yg, crop, block)
            assert gy.dtype == np.float64 and gy.shape == wy.shape
            worst = max(worst, max(rel(float(x), float(y)) for x, y in zip(gy.reshape(-1), wy.reshape(-1))))
            # Against the existing host psnr(): it takes BGR bytes, crops img[c:-c, c:-c] and averages the squared float32 differences
            # in float32, so its dB are compared at float32's accuracy (2^-24 per rounding, a few of them: 1e-6 relative is generous and far
            # below any mistake of a sample); the integers themselves are compared with the exact sum over that same slice.
            n = 3 * (h - 2 * crop) * (w - 2 * crop)
            for f in range(T):
                for q, x in enumerate((a, l)):
                    e = int(got[f, 0, :, :, q].sum())
                    s = (slice(crop, h - crop), slice(crop, w - crop))
                    d = x[f][s].astype(np.int64) - g[f][s].astype(np.int64)
                    assert e == int((d * d).sum())
                    assert rel(ref.psnr(e, n, 255.0), float(metrics.psnr(x[f][..., ::-1], g[f][..., ::-1], crop))) <= 1e-6
                    ey = float(gy[f, 0, :, :, q].sum())
                    assert rel(ref.psnr(ey, n // 3, 255.0), float(metrics.psnr(x[f][..., ::-1], g[f][..., ::-1], crop, convert_to='y'))) <= 1e-6
    print(f'{h}x{w}: luma sums, max relative difference {worst}')
    assert worst <= 1e-12


@pytest.mark.parametrize('h,w', SIZES)
def test_cell_counts_in_closed_form_are_the_brute_force_counts(h, w):
    L = _native.lib()
    for block in BLOCKS + (32, 128):
        for crop in CROPS:
            for fmt in ('420', '422', '444'):
                for plane in (0, 1):
                    sx, sy = (1, 1) if plane == 0 else ref.FORMATS[fmt]
                    want = ref.brute_counts(h, w, crop, block, plane, fmt)
                    got = metrics.gain_cell_counts(h, w, crop, block, sx, sy)
                    assert got.dtype == np.int64 and np.array_equal(got, want), (block, crop, fmt, plane)
                    assert int(got.sum()) == (h // sy - 2 * (crop // sy)) * (w // sx - 2 * (crop // sx))
                    rows, cols = ctypes.c_int(), ctypes.c_int()
                    assert L.pnp_gain_grid(h, w, block, ctypes.byref(rows), ctypes.byref(cols)) == 0
                    assert (rows.value, cols.value) == ref.grid_size(h, w, block) == metrics.gain_grid(h, w, block)
                    if block in BLOCKS:
                        n = ctypes.c_int64()
                        for i in range(rows.value):
                            for j in range(cols.value):
                                bit = _native.PLANE_Y if plane == 0 else _native.PLANE_CR
                                assert L.pnp_gain_cell_count(h, w, crop, block, bit, _native.YUV_FORMAT[fmt], i, j, ctypes.byref(n)) == 0
                                assert n.value == want[i, j], (block, crop, fmt, plane, i, j)
    # a cell wholly inside the crop holds nothing: 130 x 70 cropped by 16 with blocks of 16 loses its outer ring of cells
    ring = metrics.gain_cell_counts(130, 70, 16, 16)
    assert not ring[0].any() and not ring[:, 0].any() and not ring[:, -1].any() and ring[1, 1] == 256 and ring[7, 3] == 2 * 6 and not ring[8].any()


def test_values():
    # dPSNR is PSNR - PSNR_LQ to rounding when all are finite
    rng = np.random.RandomState(0)
    ea, el = rng.randint(1, 10 ** 9, 50), rng.randint(1, 10 ** 9, 50)
    n = 3 * 60 * 76
    pa, pl, dp = metrics.gain_values(ea, el, n, 255.0)
    assert pa.dtype == np.float64 and dp.shape == (50,)
    for i in range(50):
        assert rel(float(pa[i]), ref.psnr(int(ea[i]), n, 255.0)) <= 1e-12 and rel(float(pl[i]), ref.psnr(int(el[i]), n, 255.0)) <= 1e-12
        assert rel(float(dp[i]), ref.dpsnr(int(ea[i]), int(el[i]))) <= 1e-12
        assert abs(float(dp[i]) - (float(pa[i]) - float(pl[i]))) <= 1e-12 * max(abs(float(pa[i])), abs(float(pl[i])))
    # 10 and 12 bit peaks
    assert rel(float(metrics.gain_values(7, 9, 100, 1023.0)[0]), ref.psnr(7, 100, 1023.0)) <= 1e-12
    # the edge cases: 0 / 0, E_a = 0, E_l = 0
    pa, pl, dp = metrics.gain_values([0, 0, 5], [0, 3, 0], 10, 255.0)
    assert dp.tolist() == [0.0, math.inf, -math.inf]
    assert pa.tolist()[:2] == [math.inf, math.inf] and pl.tolist()[0] == math.inf and pl.tolist()[2] == math.inf and math.isfinite(pl[1])
    assert [ref.dpsnr(0, 0), ref.dpsnr(0, 3), ref.dpsnr(5, 0)] == [0.0, math.inf, -math.inf]
    # the fluctuation: population standard deviation, 0 for a one-frame clip
    assert metrics.gain_sd([31.25]) == 0.0
    x = [30.0, 32.5, 31.0, 35.25]
    assert rel(metrics.gain_sd(x), ref.sd(x)) <= 1e-12 and rel(metrics.gain_sd(x), float(np.std(x, ddof=0))) <= 1e-12
    assert metrics.gain_sd(x) < float(np.std(x, ddof=1))
    # the 6:1:1 weights
    assert metrics.gain_yuv(1.0, 0.0, 0.0) == 0.75 and metrics.gain_yuv(0.0, 1.0, 0.0) == 0.125 and metrics.gain_yuv(0.0, 0.0, 1.0) == 0.125
    assert np.array_equal(metrics.gain_yuv([8.0, 16.0], [8.0, 0.0], [8.0, 0.0]), [8.0, 12.0])
    for bad in (0, 8, 48, 256, True, 64.0, None):
        with pytest.raises(ValueError, match='block'):
            metrics.gain_block(bad)
    for bad in (-1, 33, 1.5):
        with pytest.raises(ValueError, match='crop'):
            metrics.gain_cell_counts(64, 80, bad, 64)
    assert metrics.gain_block(128) == 128 and metrics.GAIN_BLOCKS == ref.BLOCKS


def overlapping_map(h, w, seed=0):
    """a partition map whose three planes overlap (as the sparse_val goldens' do): rectangles painted plane by plane, values != 1 too"""
    rng = np.random.RandomState(seed)
    par = np.zeros((T, 3, h, w), np.float32)
    for f in range(T):
        for c in range(3):
            for _ in range(6):
                y, x = rng.randint(0, h - 8), rng.randint(0, w - 8)
                par[f, c, y:y + rng.randint(4, 40), x:x + rng.randint(4, 40)] = rng.choice([1.0, 0.5, -2.0])
    return par


@pytest.mark.parametrize('h,w', SIZES[1:])
def test_partition_classes(h, w):
    rng = np.random.RandomState(w)
    g = rng.randint(0, 256, (T, h, w, 3)).astype(np.uint8)
    a, l = near(g, 5, 9, 255), near(g, 6, 14, 255)
    par = overlapping_map(h, w)
    for crop in (0, 6):
        grid, got = metrics.gain_sums(a, l, g, crop, 16, par=par)
        want = ref.gain_classes(a, l, g, par, crop)
        assert got.dtype == np.int64 and got.shape == (T, 8, 3) and np.array_equal(got, want)
        assert (got[:, :, 0] > 0).sum() >= 6 * T // 2 and (got[:, [3, 5, 6, 7], 0].sum(axis=1) > 0).all()        # mixed classes exist
        assert (got[:, :, 0].sum(axis=1) == (h - 2 * crop) * (w - 2 * crop)).all()                               # counts sum to the region
        assert np.array_equal(got[:, :, 1:].sum(axis=1), grid[:, 0].sum(axis=(1, 2)))                            # class sums add up to the frame's
        # float32 luma: the same classes, fp64 sums
        ya, yl, yg = (ref.luma(x) for x in (a, l, g))
        gy, cy = metrics.gain_sums(ya, yl, yg, crop, 16, par=par)
        wy = ref.gain_classes(ya, yl, yg, par, crop)
        assert cy.dtype == np.float64 and np.array_equal(cy[:, :, 0], want[:, :, 0])
        assert max(rel(float(x), float(y)) for x, y in zip(cy.reshape(-1), wy.reshape(-1))) <= 1e-12
        # the Y plane of a clip of planes
        planes = tuple(x[..., 0].astype(np.int32) for x in (a, l, g))
        half = np.zeros((T, h // 2, w // 2), np.int32)
        _, cp = metrics.gain_sums((planes[0], half, half), (planes[1], half, half), (planes[2], half, half), crop, 16, '420', par=par)
        assert np.array_equal(cp, ref.gain_classes(planes[0], planes[1], planes[2], par, crop))
    _, zero = metrics.gain_sums(a, l, g, 2, 64, par=np.zeros_like(par))
    assert (zero[:, 0, 0] == (h - 4) * (w - 4)).all() and not zero[:, 1:].any()                                  # an all-zero map: class 0 holds everything
    assert [ref.pixel_class(*p) for p in ((0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, -1), (1, 1, 1))] == [0, 1, 2, 4, 7]
    assert metrics.gain_classes(np.array([[[[1.0]], [[0.0]], [[0.5]]]], np.float32)).tolist() == [[[5]]]


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_the_entries_refuse_before_any_hip_call():
    L = _native.lib()
    U8, F32 = _native.FRAMES_U8_HWC, _native.FRAMES_F32_NCHW

    def io(a=A, fa=F32, l=A, fl=U8, g=A, fg=F32, color=_native.COLOR_NONE, par=None, grid=A, cls=None, frames=2, c=3, h=64, w=80, crop=2, block=64):
        return L.pnp_gain_sums_io(a, fa, l, fl, g, fg, color, par, grid, cls, frames, c, h, w, crop, block, None)

    assert io(a=None) == BAD_ARG and io(l=None) == BAD_ARG and io(g=None) == BAD_ARG and io(grid=None) == BAD_ARG
    assert io(fa=7) == BAD_ARG and io(fl=7) == BAD_ARG and io(fg=-1) == BAD_ARG and io(color=5) == BAD_ARG
    assert io(frames=0) == BAD_ARG and io(c=1) == BAD_ARG and io(c=4) == BAD_ARG and io(h=0) == BAD_ARG and io(crop=-1) == BAD_ARG and io(crop=32) == BAD_ARG
    for block in (0, 8, 24, 48, 256, -64):
        assert io(block=block) == BAD_ARG and io(block=block, color=_native.COLOR_Y) == BAD_ARG, block
    assert io(cls=A) == BAD_ARG and io(par=A) == BAD_ARG                     # class sums without a map, a map without class sums

    P = _native.Yuv420Planes

    def desc(w, step=1):
        return P(A, A + 0x10000, A + 0x20000 if step == 1 else A + 0x10001, w, step * w, 0, 0, step)

    def yuv(a=desc(80), l=desc(80, 2), g=desc(80), mask=7, par=None, grid=A, cls=None, frames=2, h=64, w=80, crop=2, block=64, fmt=0):
        ref_ = lambda d: None if d is None else ctypes.byref(d)      # noqa: E731
        return L.pnp_gain_sums_yuv(ref_(a), ref_(l), ref_(g), mask, par, grid, cls, frames, h, w, crop, block, fmt, None)

    assert yuv(a=None) == BAD_ARG and yuv(l=None) == BAD_ARG and yuv(g=None) == BAD_ARG and yuv(grid=None) == BAD_ARG
    assert yuv(mask=0) == BAD_ARG and yuv(mask=8) == BAD_ARG and yuv(block=8) == BAD_ARG and yuv(fmt=3) == BAD_ARG and yuv(fmt=-1) == BAD_ARG
    assert yuv(crop=3) == BAD_ARG and yuv(crop=32) == BAD_ARG and yuv(h=63) == BAD_ARG and yuv(frames=0) == BAD_ARG
    assert yuv(l=desc(40)) == BAD_ARG                                        # a pitch below the row
    assert yuv(cls=A) == BAD_ARG and yuv(par=A) == BAD_ARG and yuv(par=A, cls=A, mask=6) == BAD_ARG      # a map with a chroma-only mask
    P16 = _native.Yuv420Planes16
    d10 = P16(A, A + 0x10000, A + 0x20000, 160, 80, 0, 0, 1, 10, 0)
    d12 = P16(A, A + 0x10000, A + 0x20000, 160, 80, 0, 0, 1, 12, 0)
    y16 = lambda a, l, g, **kw: L.pnp_gain_sums_yuvp16(ctypes.byref(a), ctypes.byref(l), ctypes.byref(g), kw.get('mask', 7), None, kw.get('grid', A),      # noqa: E731
                                                       None, 2, 64, 80, 2, kw.get('block', 64), 0, None)
    assert y16(d10, d12, d10) == BAD_ARG and y16(d12, d10, d10) == BAD_ARG and y16(d10, d10, d12) == BAD_ARG      # one bit depth
    assert y16(d10, d10, d10, grid=None) == BAD_ARG and y16(d10, d10, d10, block=20) == BAD_ARG and y16(d10, d10, d10, mask=9) == BAD_ARG
    # the host queries
    r, c, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert L.pnp_gain_grid(64, 80, 48, ctypes.byref(r), ctypes.byref(c)) == BAD_ARG and L.pnp_gain_grid(0, 80, 64, ctypes.byref(r), ctypes.byref(c)) == BAD_ARG
    assert L.pnp_gain_grid(64, 80, 64, None, ctypes.byref(c)) == BAD_ARG
    count = lambda *a: L.pnp_gain_cell_count(*a, ctypes.byref(n))      # noqa: E731
    assert count(64, 80, 2, 64, 1, 0, 0, 0) == 0 and n.value == 60 * 62
    assert count(64, 80, 2, 64, 1, 0, 1, 0) == BAD_ARG and count(64, 80, 2, 64, 1, 0, 0, 2) == BAD_ARG and count(64, 80, 2, 64, 3, 0, 0, 0) == BAD_ARG
    assert count(64, 80, 3, 64, 2, 0, 0, 0) == BAD_ARG and count(64, 80, 3, 64, 2, 2, 0, 0) == 0 and count(64, 80, 2, 20, 1, 0, 0, 0) == BAD_ARG
    assert L.pnp_gain_cell_count(64, 80, 2, 64, 1, 0, 0, 0, None) == BAD_ARG
    assert L.pnp_gain_luma_tiles(64, 80, 2, 64) == 1 and L.pnp_gain_luma_tiles(130, 530, 0, 16) == 9 * 3 and L.pnp_gain_luma_tiles(64, 80, 2, 8) == 0


# ------------------------------------------------------------------------------------------------ the plan under the sanitizers
def test_the_plan_on_the_host_under_asan(tmp_path):
    """tests/host/gain_stub.cpp: a stand-alone program; nothing is loaded into this interpreter"""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'gain_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'gain_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    docs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    cases = [d for d in docs if 'h' in d]
    assert docs[-1] == {'cases': len(cases)} and len(cases) >= 100
    fmt_of = {(1, 1): '444', (2, 2): '420', (2, 1): '422'}
    for d in cases:
        assert d['errors'] == [], d
        plane = 0 if (d['sx'], d['sy']) == (1, 1) else 1
        want = ref.brute_counts(d['h'], d['w'], d['crop'], d['block'], plane, fmt_of[(d['sx'], d['sy'])])
        assert d['counts'] == want.reshape(-1).tolist() and (d['grows'], d['gcols']) == want.shape, d
    for h, w in SIZES:                                                           # every size, block and crop of the tests above was walked
        for block in BLOCKS:
            for crop in CROPS:
                assert sum(1 for d in cases if (d['h'], d['w'], d['block'], d['crop']) == (h, w, block, crop)) == 3
    assert any(d['tiles_x'] >= 3 and d['grows'] >= 3 for d in cases) and any(d['crop'] == 3 for d in cases)
