"""CPU: MS-SSIM as include/pnpvcve.h states it (pnp_msssim_*).

* pnp_vcve_amd.metrics.msssim (the numpy restatement the host path of evaluate() serves) against the independent scipy restatement
  tests/msssim_ref.py, 1e-12 on every CS_s / S_s;
* fixed points: identical images, the anticorrelated pair, frames below 176 x 176;
* the claim the fp32 workspace rests on: the fp32 pyramid of 8-, 10- and 12-bit integer planes IS the fp64 pyramid;
* the sizing queries of the C ABI (host calls, no GPU) against the restatement's shapes, and the entries' refusals;
* csrc/msssim_plan.h on the host under AddressSanitizer + UBSan: a stand-alone program (tests/host/msssim_stub.cpp) run as a
  subprocess; nothing is loaded into this interpreter."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import msssim_ref as ref
from pnp_vcve_amd import _native, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 1001
A = 0x1000        # an aligned "device address": never dereferenced on these paths
SIZES = [(176, 176, 0), (178, 215, 0), (200, 300, 4)]


def bgr_pair(h, w, seed):
    a, b = ref.test_pair(h, w, seed, planes=3)
    return a.transpose(1, 2, 0).astype(np.uint8), b.transpose(1, 2, 0).astype(np.uint8)


@pytest.mark.parametrize('h,w,crop', SIZES)
def test_msssim_against_independent_scipy_restatement(h, w, crop):
    a, b = bgr_pair(h, w, 11 + h)
    cut = (lambda x: x[crop:-crop, crop:-crop]) if crop else (lambda x: x)
    vals = []
    for ch in range(3):
        got = metrics.msssim_plane_scales(cut(a[..., ch]), cut(b[..., ch]))
        want = ref.plane_scales(cut(a[..., ch]), cut(b[..., ch]))
        print(h, w, crop, ch, np.abs(got - want).max(), want.min(), want.max())
        assert want.min() > 0.1 and want.max() < 0.999            # not a trivial case
        assert np.abs(got - want).max() <= 1e-12
        vals.append(ref.value(want))
    assert abs(metrics.msssim(a, b, crop) - np.mean(vals)) <= 1e-12       # several planes: the mean of the planes' values, crop or not
    assert abs(metrics.msssim(a.transpose(2, 0, 1), b.transpose(2, 0, 1), crop, input_order='CHW') - np.mean(vals)) <= 1e-12
    # convert_to='y': one plane, the float32 Y that ssim() reads
    ya = metrics.bgr2y(a.astype(np.float32) / 255.) * 255.
    yb = metrics.bgr2y(b.astype(np.float32) / 255.) * 255.
    assert abs(metrics.msssim(a, b, crop, convert_to='y') - ref.value(ref.plane_scales(cut(ya), cut(yb)))) <= 1e-12
    assert metrics.ALLOWED_METRICS['MS-SSIM'] is metrics.msssim


def test_fixed_points():
    a, _ = bgr_pair(176, 180, 5)
    assert abs(metrics.msssim(a, a) - 1.0) <= 1e-12
    assert abs(metrics.msssim(a, a, convert_to='y') - 1.0) <= 1e-12
    rng = np.random.RandomState(3)
    n = rng.randint(0, 256, (176, 176, 3)).astype(np.uint8)
    raw = metrics.msssim_plane_scales(n[..., 0], 255 - n[..., 0])
    print('raw CS_0 of the anticorrelated pair:', raw[0, 0])
    assert raw[0, 0] < 0 and np.isfinite(raw).all()
    assert metrics.msssim(n, 255 - n) == 0.0                      # exactly 0, not NaN
    assert ref.value(ref.plane_scales(n[..., 0], 255 - n[..., 0])) == 0.0
    for h, w, crop in ((175, 400, 0), (184, 184, 6)):
        x = np.zeros((h, w, 3), np.uint8)
        with pytest.raises(ValueError, match='176'):
            metrics.msssim(x, x, crop)


@pytest.mark.parametrize('depth', [8, 10, 12])
def test_the_fp32_pyramid_of_integer_planes_is_the_fp64_pyramid(depth):
    rng = np.random.RandomState(depth)
    x = rng.randint(0, 1 << depth, (179, 215))
    x[:8, :8] = (1 << depth) - 1                                   # the peak, held down the levels
    p32, p64 = ref.pyramid(x, np.float32), ref.pyramid(x, np.float64)
    assert [p.shape for p in p32] == ref.level_shapes(179, 215)
    for s in range(1, 5):
        assert p32[s].dtype == np.float32 and np.array_equal(p32[s].astype(np.float64), p64[s]), s
        # and it is the exact mean: an integer over 4^s
        assert np.array_equal(p64[s] * 4.0 ** s, np.rint(p64[s] * 4.0 ** s))
    assert np.array_equal(metrics._msssim_down(x.astype(np.float32)), p32[1])


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def test_the_sizing_queries_are_the_restatements_shapes(lib):
    assert lib.pnp_msssim_min_size() == 176 == ref.MIN_SIZE == metrics.MSSSIM_MIN_SIZE
    for h, w, crop in SIZES + [(352, 356, 0), (720, 1280, 0), (176, 400, 0), (191, 177, 0), (188, 188, 6)]:
        shapes = ref.level_shapes(h, w, crop)
        floats = 0
        for s in range(5):
            r, c = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.pnp_msssim_level_dims(h, w, crop, s, ctypes.byref(r), ctypes.byref(c)) == 0
            assert (r.value, c.value) == shapes[s], (h, w, crop, s)
            assert lib.pnp_msssim_blocks(h, w, crop, s) == ref.blocks_of(*shapes[s]), (h, w, crop, s)
            if s:
                floats += (shapes[s][0] * shapes[s][1] + 3) // 4 * 4
        assert shapes[4][0] >= 11 and shapes[4][1] >= 11
        # levels 1..4 of both clips in fp32, each level rounded up to 16 bytes
        assert lib.pnp_msssim_workspace_bytes(3, 2, h, w, crop) == 2 * 3 * 2 * floats * 4, (h, w, crop)
        assert floats * 4 <= (h - 2 * crop) * (w - 2 * crop) * 4 / 3 + 64
    assert lib.pnp_msssim_blocks(176, 176, 0, 4) == 1 and lib.pnp_msssim_blocks(176, 176, 0, 0) == 11 * 6
    # 0 / an error when it cannot run
    r, c = ctypes.c_int(-1), ctypes.c_int(-1)
    for h, w, crop in ((175, 400, 0), (400, 175, 0), (184, 184, 6), (176, 176, -1), (0, 0, 0), (176, 176, 200)):
        assert ref.level_shapes(h, w, crop) is None
        assert lib.pnp_msssim_blocks(h, w, crop, 0) == 0 and lib.pnp_msssim_workspace_bytes(1, 1, h, w, crop) == 0, (h, w, crop)
        assert lib.pnp_msssim_level_dims(h, w, crop, 0, ctypes.byref(r), ctypes.byref(c)) == BAD_ARG
    assert lib.pnp_msssim_blocks(176, 176, 0, 5) == 0 and lib.pnp_msssim_blocks(176, 176, 0, -1) == 0
    assert lib.pnp_msssim_level_dims(176, 176, 0, 5, ctypes.byref(r), ctypes.byref(c)) == BAD_ARG
    assert lib.pnp_msssim_level_dims(176, 176, 0, 0, None, ctypes.byref(c)) == BAD_ARG
    assert lib.pnp_msssim_workspace_bytes(0, 1, 176, 176, 0) == 0 and lib.pnp_msssim_workspace_bytes(1, 0, 176, 176, 0) == 0
    assert lib.pnp_abi_version() == 5


def test_the_entries_refuse_on_the_host_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    F32, U8, NONE, Y = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC, _native.COLOR_NONE, _native.COLOR_Y

    def io(a=A, fa=F32, b=A, fb=U8, color=NONE, part=A, ws=A, frames=1, c=3, h=176, w=176, crop=0):
        return lib.pnp_msssim_partials_io(a, fa, b, fb, color, part, ws, frames, c, h, w, crop, None)

    assert io(h=175) == BAD_ARG and io(w=175) == BAD_ARG and io(h=184, w=184, crop=6) == BAD_ARG      # below 176 after the crop
    assert io(a=None) == BAD_ARG and io(b=None) == BAD_ARG and io(part=None) == BAD_ARG and io(ws=None) == BAD_ARG
    assert io(fa=2) == BAD_ARG and io(color=2) == BAD_ARG and io(frames=0) == BAD_ARG and io(crop=-1) == BAD_ARG
    assert io(c=1) == BAD_ARG and io(c=1, fb=F32, color=Y) == BAD_ARG                                 # bytes and Y need 3 channels

    def planes8(w, step=2):
        return _native.Yuv420Planes(A, A + 0x100000, A + (0x100001 if step == 2 else 0x200000), w, step * (w // 2), 1 << 22, 1 << 22, step)

    def planes16(w, depth=10, msb=0):
        return _native.Yuv420Planes16(A, A + 0x100000, A + 0x200000, 2 * w, w, 1 << 22, 1 << 22, 1, depth, msb)

    def yuv(a, b, entry, mask=1, part=A, ws=A, frames=1, h=352, w=352, crop=0):
        return getattr(lib, entry)(ctypes.byref(a), ctypes.byref(b), mask, part, ws, frames, h, w, crop, None)

    for entry, mk in (('pnp_msssim_partials_yuv420', planes8), ('pnp_msssim_partials_yuv420p16', planes16)):
        ok = mk(352)
        assert yuv(ok, ok, entry, mask=0) == BAD_ARG and yuv(ok, ok, entry, mask=8) == BAD_ARG
        assert yuv(ok, ok, entry, ws=None) == BAD_ARG and yuv(ok, ok, entry, part=None) == BAD_ARG
        assert yuv(ok, ok, entry, crop=1) == BAD_ARG and yuv(ok, ok, entry, crop=-2) == BAD_ARG       # an odd or negative crop
        assert yuv(ok, ok, entry, h=174) == BAD_ARG                                                    # Y below 176
        for mask in (2, 4, 6, 3, 7):                                                                   # chroma of 350 lines: 175 rows
            assert yuv(ok, ok, entry, mask=mask, h=350) == BAD_ARG, mask
            assert yuv(mk(360), mk(360), entry, mask=mask, h=356, w=360, crop=4) == BAD_ARG, mask      # 178 - 4 = 174 chroma rows
    assert yuv(planes16(352, 10), planes16(352, 12), 'pnp_msssim_partials_yuv420p16') == BAD_ARG      # differing depths


# ------------------------------------------------------------------------------------------------ the plan and the loader under the sanitizers
def test_the_plan_and_the_level_1_loader_on_the_host_under_asan(tmp_path):
    """tests/host/msssim_stub.cpp: a stand-alone program; nothing is loaded into this interpreter"""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'msssim_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'msssim_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    docs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert docs[0] == {'plan': True, 'errors': []}
    cases = [d for d in docs if 'off' in d]
    assert docs[-1] == {'cases': len(cases)}
    want = {(off, extra, step, rows, cols, crop) for off in range(4) for extra in (0, 5, 7) for step in (1, 2)
            for rows, cols, crop in ((176, 176, 0), (178, 216, 0), (178, 216, 1))}
    assert {(d['off'], d['pitch_extra'], d['step'], d['rows'], d['cols'], d['crop']) for d in cases} == want and len(cases) == len(want)
    for d in cases:
        assert d['errors'] == [], d
        assert 0 < d['dwords'], d
        # bytes at heads, tails and misaligned rows: a misaligned base or an odd pitch cannot be read with dwords alone
        if d['off'] or d['pitch_extra']:
            assert d['dwords'] < d['fetches'], d
