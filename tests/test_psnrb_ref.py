"""CPU: PSNR-B as include/pnpvcve.h states it (pnp_psnrb_*).

* pnp_vcve_amd.metrics.psnrb_plane_sums / psnrb_counts / psnrb_values / psnrb (the numpy host path, which slices and counts in closed
  form, and whose fp64 part ops.psnrb_* run on the device's sums) against the independent restatement tests/psnrb_ref.py, which
  enumerates every pair: integer sums equal, values to 1e-12 relative -- the bound the project uses for two fp64 restatements of one
  formula (tests/test_xpsnr_ref.py);
* pnp_psnrb_counts of the C ABI (a host call, no GPU) against enumeration over a ladder of sizes and every crop that fits;
* closed forms on a 32 x 40 plane with blocks of 8;
* the entries' refusals with null device pointers, decided before any HIP call;
* csrc/psnrb_plan.h on the host under AddressSanitizer + UBSan: a stand-alone program (tests/host/psnrb_stub.cpp) run as a subprocess;
  nothing is loaded into this interpreter."""
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import psnrb_ref as ref
from pnp_vcve_amd import _native, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 1001
A = 0x1000        # an aligned "device address": never dereferenced on these paths


def rel(got, want):
    if math.isinf(want):
        return 0.0 if got == want else math.inf
    return abs(got - want) / abs(want) if want else abs(got)


@pytest.mark.parametrize('d', [8, 10, 12])
@pytest.mark.parametrize('rows,cols', [(54, 70), (33, 40)])
def test_host_path_against_the_independent_restatement(rows, cols, d):
    peak = float((1 << d) - 1)
    a, b = ref.blocky_plane(rows, cols, d, 8, seed=rows + d)
    worst = 0.0
    for block in (4, 8, 16):
        for crop in (0, 2, 3):
            want = ref.psnrb_plane(a, b, crop, block, peak)
            sums = metrics.psnrb_plane_sums(a, b, crop, block)
            assert sums.dtype == np.int64 and np.array_equal(sums, np.array(want['sums'], np.int64)), (block, crop)
            counts = metrics.psnrb_counts(rows, cols, crop, block)
            assert tuple(counts) == want['counts'], (block, crop)
            val, bef = metrics.psnrb_values(sums, counts, block, (rows - 2 * crop, cols - 2 * crop), peak)
            assert val.dtype == np.float64 and bef.dtype == np.float64
            worst = max(worst, rel(float(val), want['value']), rel(float(bef), want['bef']))
            assert rel(float(val), want['value']) <= 1e-12 and rel(float(bef), want['bef']) <= 1e-12, (block, crop)
            # the no-reference form: sse 0, the four pair sums unchanged
            alone = metrics.psnrb_plane_sums(a, None, crop, block)
            assert alone[0] == 0 and np.array_equal(alone[1:], sums[1:])
            if block == 8:          # the planted grid is seen: a blocky test plane has a BEF, its smooth reference next to none
                assert want['d_b'] > 4 * want['d_n'] and want['bef'] > 0 and 10 < want['value'] < 60
    print(f'{rows}x{cols} d {d}: max relative difference {worst}')


def test_the_image_path_is_the_mean_of_the_channels_and_the_y_of_psnr():
    rng = np.random.RandomState(5)
    planes = [ref.blocky_plane(33, 40, 8, 8, seed=s) for s in (1, 2, 3)]
    img1 = np.stack([p[0] for p in planes], axis=-1).astype(np.uint8)          # BGR, as psnr() takes it
    img2 = np.stack([p[1] for p in planes], axis=-1).astype(np.uint8)
    for block, crop in ((8, 0), (4, 3), (16, 2)):
        want = [ref.psnrb_plane(x, y, crop, block, 255.0) for x, y in planes]
        got = metrics.psnrb(img1, img2, crop, block=block)
        assert rel(got, sum(w['value'] for w in want) / 3) <= 1e-12
        assert rel(metrics.psnrb(img1.transpose(2, 0, 1), img2.transpose(2, 0, 1), crop, input_order='CHW', block=block), got) == 0
        assert rel(metrics.bef(img1, crop, block=block), sum(w['bef'] for w in want) / 3) <= 1e-12
        ya, yb = (metrics.bgr2y(i.astype(np.float32) / 255.) * 255. for i in (img1, img2))
        assert ya.dtype == np.float32
        wy = ref.psnrb_plane(ya, yb, crop, block, 255.0)
        sy = metrics.psnrb_plane_sums(ya, yb, crop, block)
        assert sy.dtype == np.float64 and max(rel(float(g), w) for g, w in zip(sy, wy['sums'])) <= 1e-12
        assert rel(metrics.psnrb(img1, img2, crop, convert_to='y', block=block), wy['value']) <= 1e-12
        assert rel(metrics.psnrb(img1, img2, crop, convert_to='Y', block=block), wy['value']) <= 1e-12
    assert metrics.ALLOWED_METRICS['PSNR-B'] is metrics.psnrb
    assert metrics.psnrb(img1, img2) == metrics.psnrb(img1, img2, block=8)
    assert metrics.psnrb(img1, img2) != metrics.psnrb(img2, img1)                # the BEF is the FIRST argument's, the test image's
    grey = rng.randint(0, 256, size=(33, 40)).astype(np.uint8)                   # a 2-D image is one channel
    assert rel(metrics.psnrb(grey, grey[::-1].copy()), ref.psnrb_plane(grey.astype(np.int64), grey[::-1].astype(np.int64), 0, 8, 255.0)['value']) <= 1e-12
    for bad in (dict(block=3), dict(block=128), dict(block=True), dict(block=8.0), dict(convert_to='ycbcr'), dict(crop_border=13, block=8),
                dict(crop_border=17)):
        with pytest.raises(ValueError):
            metrics.psnrb(img1, img2, **bad)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def test_the_count_query_is_the_enumeration(lib):
    checked = refused = 0
    for rows, cols in ((7, 9), (16, 16), (20, 27), (33, 40), (54, 70), (8, 64), (2, 2)):
        for bp in (2, 4, 8, 16, 32, 64):
            for crop in range(0, min(rows, cols) // 2 + 2):
                out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
                code = lib.pnp_psnrb_counts(rows, cols, crop, bp, out)
                fits = 2 * crop < min(rows, cols) and min(rows, cols) - 2 * crop >= bp
                if not fits:
                    assert code == BAD_ARG and list(out) == [-1] * 4, (rows, cols, bp, crop)
                    with pytest.raises(ValueError):
                        metrics.psnrb_counts(rows, cols, crop, bp)
                    refused += 1
                    continue
                want = ref.counts(rows, cols, crop, bp)
                assert code == 0 and tuple(out) == want == tuple(metrics.psnrb_counts(rows, cols, crop, bp)), (rows, cols, bp, crop)
                h, w = rows - 2 * crop, cols - 2 * crop
                assert want[0] + want[1] == h * (w - 1) and want[2] + want[3] == w * (h - 1)
                checked += 1
    assert checked >= 60 and refused >= 60
    out = (ctypes.c_int64 * 4)()
    for rows, cols, crop, bp in ((0, 8, 0, 8), (8, 0, 0, 8), (16, 16, -1, 8), (16, 16, 0, 3), (16, 16, 0, 1), (16, 16, 0, 128), (16, 16, 0, 0),
                                 (16, 16, 0, -8)):
        assert lib.pnp_psnrb_counts(rows, cols, crop, bp, out) == BAD_ARG, (rows, cols, crop, bp)
    assert lib.pnp_psnrb_counts(16, 16, 0, 8, None) == BAD_ARG
    # a 3840 x 2160 plane: the counts need 64 bits only in the product, and are the closed form
    assert lib.pnp_psnrb_counts(2160, 3840, 0, 8, out) == 0
    assert tuple(out) == (2160 * 479, 2160 * (3839 - 479), 3840 * 269, 3840 * (2159 - 269))
    assert lib.pnp_psnrb_luma_blocks(64, 80, 0) == 2 and lib.pnp_psnrb_luma_blocks(66, 530, 0) == 9 and lib.pnp_psnrb_luma_blocks(66, 530, 1) == 6
    assert lib.pnp_psnrb_luma_blocks(0, 8, 0) == 0 and lib.pnp_psnrb_luma_blocks(8, 8, 4) == 0 and lib.pnp_psnrb_luma_blocks(8, 8, -1) == 0
    assert lib.pnp_abi_version() == 5


# ------------------------------------------------------------------------------------------------ closed forms, 32 x 40, blocks of 8
def test_a_block_constant_plane_has_steps_on_the_grid_only():
    a = ref.block_constant(32, 40, 8, seed=11)
    sse, sbh, snh, sbv, snv = metrics.psnrb_plane_sums(a, a, 0, 8)
    assert sse == 0 and snh == 0 and snv == 0 and sbh > 0 and sbv > 0
    counts = metrics.psnrb_counts(32, 40, 0, 8)
    assert counts == (32 * 4, 32 * 35, 40 * 3, 40 * 28)
    val, bef = metrics.psnrb_values(np.array([sse, sbh, snh, sbv, snv]), counts, 8, (32, 40), 255.0)
    assert float(bef) == (math.log2(8) / math.log2(32)) * (float(sbh + sbv) / (counts[0] + counts[2]))          # exactly
    assert rel(float(val), 10.0 * math.log10(255.0 ** 2 / float(bef))) <= 1e-12
    assert ref.plane_sums(a, a, 0, 8) == [sse, sbh, snh, sbv, snv]
    # rolled by 3 columns no step lies on a vertical grid line any more; the horizontal grid lines keep theirs
    r = np.roll(a, 3, axis=1)
    s = metrics.psnrb_plane_sums(r, None, 0, 8)
    assert s[1] == 0 and s[2] > 0 and s[3] == sbv and s[4] == 0
    # a crop does not move the grid: cropped by 3 the steps are still all on it
    c = metrics.psnrb_plane_sums(a, None, 3, 8)
    assert c[2] == 0 and c[4] == 0 and c[1] > 0 and c[3] > 0
    assert metrics.psnrb_counts(32, 40, 3, 8) == ref.counts(32, 40, 3, 8) == (26 * 4, 26 * 29, 34 * 3, 34 * 22)


def test_ramps():
    y, x = np.mgrid[0:32, 0:40]
    same = (3 * x + 3 * y).astype(np.int64)                 # the same step both ways: every pair differs by 3
    s = metrics.psnrb_plane_sums(same, same, 0, 8)
    counts = metrics.psnrb_counts(32, 40, 0, 8)
    assert list(s) == [0, 9 * counts[0], 9 * counts[1], 9 * counts[2], 9 * counts[3]]
    val, bef = metrics.psnrb_values(s, counts, 8, (32, 40), 255.0)
    assert float(bef) == 0.0 and float(val) == math.inf      # D_B == D_N, and a == b
    assert metrics.psnrb(same.astype(np.uint8), same.astype(np.uint8)) == math.inf
    w = ref.psnrb_plane(same, same, 0, 8, 255.0)
    assert w['d_b'] == w['d_n'] == 9.0 and w['value'] == math.inf
    # unequal steps: the boundary set's mix of horizontal and vertical pairs differs from the rest's, so D_B != D_N
    skew = (5 * x + 1 * y).astype(np.int64)
    w = ref.psnrb_plane(skew, skew, 0, 8, 255.0)
    d_b = (25 * counts[0] + 1 * counts[2]) / (counts[0] + counts[2])
    d_n = (25 * counts[1] + 1 * counts[3]) / (counts[1] + counts[3])
    assert w['d_b'] == d_b and w['d_n'] == d_n and d_b != d_n
    val, bef = metrics.psnrb_values(metrics.psnrb_plane_sums(skew, skew, 0, 8), counts, 8, (32, 40), 255.0)
    assert rel(float(bef), w['bef']) <= 1e-12 and (float(bef) > 0) == (d_b > d_n)


def test_a_10_bit_clip_that_is_an_8_bit_clip_times_4():
    a, b = ref.blocky_plane(32, 40, 8, 8, seed=4)
    for crop in (0, 3):
        s8, s10 = metrics.psnrb_plane_sums(a, b, crop, 8), metrics.psnrb_plane_sums(4 * a, 4 * b, crop, 8)
        assert np.array_equal(s10, 16 * s8) and ref.plane_sums(4 * a, 4 * b, crop, 8) == [16 * int(v) for v in s8]
    top = np.full((32, 40), 4095, np.int64)                  # the largest squared difference, 12 bit
    top[:, 7::8] = 0
    s = metrics.psnrb_plane_sums(top, np.zeros_like(top), 0, 8)
    assert s[0] == 4095 ** 2 * 32 * 35 and s[1] == 4095 ** 2 * 32 * 4


# ------------------------------------------------------------------------------------------------ refusals, no GPU
def test_the_entries_refuse_on_the_host_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    def planes8(w, step=2, y=A):
        return _native.Yuv420Planes(y, A + 0x100000, A + (0x100001 if step == 2 else 0x200000), w, step * (w // 2), 1 << 22, 1 << 22, step)

    def planes16(w, depth=10, msb=0, y=A):
        return _native.Yuv420Planes16(y, A + 0x100000, A + 0x200000, 2 * w, w, 1 << 22, 1 << 22, 1, depth, msb)

    def call(a, b, entry, mask=1, sums=A, frames=2, h=54, w=70, crop=0, block=8):
        return getattr(lib, entry)(ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None, mask, sums, frames, h, w,
                                   crop, block, None)

    for entry, mk in (('pnp_psnrb_sums_yuv420', planes8), ('pnp_psnrb_sums_yuv420p16', planes16)):
        ok = mk(70)
        assert call(ok, ok, entry, mask=0) == BAD_ARG and call(ok, ok, entry, mask=8) == BAD_ARG and call(ok, ok, entry, mask=-1) == BAD_ARG
        for block in (0, 2, 3, 12, 128, -8):
            assert call(ok, ok, entry, block=block) == BAD_ARG, block
        assert call(ok, ok, entry, sums=None) == BAD_ARG and call(None, ok, entry) == BAD_ARG and call(None, None, entry) == BAD_ARG
        assert call(ok, ok, entry, frames=0) == BAD_ARG
        assert call(ok, ok, entry, crop=1) == BAD_ARG and call(ok, ok, entry, crop=-2) == BAD_ARG and call(ok, ok, entry, crop=28) == BAD_ARG
        assert call(ok, ok, entry, h=53) == BAD_ARG and call(ok, ok, entry, w=72) == BAD_ARG          # odd rows; a pitch below the row
        assert call(ok, mk(70, y=None), entry) == BAD_ARG and call(mk(70, y=None), None, entry) == BAD_ARG
        # a plane asked for that is smaller than its block: 54 x 70 holds a 32 block on Y and a 16 block on chroma, no 64 / 32 block
        assert call(ok, ok, entry, mask=1, block=64) == BAD_ARG and call(ok, ok, entry, mask=2, block=64) == BAD_ARG
        assert call(ok, ok, entry, mask=1, block=16, crop=20) == BAD_ARG and call(ok, None, entry, mask=4, block=16, crop=20) == BAD_ARG
    assert call(planes16(70, 10), planes16(70, 12), 'pnp_psnrb_sums_yuv420p16') == BAD_ARG            # differing depths
    assert call(planes16(70, 9), planes16(70, 9), 'pnp_psnrb_sums_yuv420p16') == BAD_ARG

    def io(a=A, fa=_native.FRAMES_F32_NCHW, b=A, fb=_native.FRAMES_F32_NCHW, color=_native.COLOR_NONE, out=A, frames=2, c=3, h=54, w=70, crop=0,
           block=8):
        return lib.pnp_psnrb_sums_io(a, fa, b, fb, color, out, frames, c, h, w, crop, block, None)

    U8 = _native.FRAMES_U8_HWC
    assert io(a=None) == BAD_ARG and io(out=None) == BAD_ARG and io(a=None, b=None) == BAD_ARG
    assert io(fa=7) == BAD_ARG and io(fb=7) == BAD_ARG and io(color=5) == BAD_ARG
    assert io(frames=0) == BAD_ARG and io(c=0) == BAD_ARG and io(h=0) == BAD_ARG and io(crop=-1) == BAD_ARG and io(crop=27) == BAD_ARG
    assert io(c=1, fa=U8) == BAD_ARG and io(c=1, color=_native.COLOR_Y) == BAD_ARG and io(c=4, fb=U8) == BAD_ARG        # pnp_psnr_stat_io's rule
    for block in (0, 2, 3, 12, 128, -8):
        assert io(block=block) == BAD_ARG and io(block=block, b=None, color=_native.COLOR_Y) == BAD_ARG, block
    assert io(block=64) == BAD_ARG and io(block=32, crop=12) == BAD_ARG and io(block=16, crop=20, fa=U8, b=None) == BAD_ARG


# ------------------------------------------------------------------------------------------------ the plan under the sanitizers
def test_the_plan_on_the_host_under_asan(tmp_path):
    """tests/host/psnrb_stub.cpp: a stand-alone program; nothing is loaded into this interpreter"""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'psnrb_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'psnrb_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    docs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    cases = [d for d in docs if 'rows' in d]
    assert docs[-1] == {'cases': len(cases)} and len(cases) >= 40
    for d in cases:
        assert d['errors'] == [], d
        assert tuple(d['counts']) == ref.counts(d['rows'], d['cols'], d['crop'], d['bp']), d
    assert any(d['tiles_x'] >= 3 and d['tiles_y'] >= 3 for d in cases) and any(d['crop'] == 3 for d in cases)
