"""CPU: XPSNR as include/pnpvcve.h states it (pnp_xpsnr_*).

* pnp_vcve_amd.metrics.xpsnr (the vectorised numpy host path, whose fp64 part ops.xpsnr_yuv420 runs on the device's sums) against the
  independent block-by-block restatement tests/xpsnr_ref.py: integer sums equal, values to 1e-12 relative (fp64, the two differ in
  summation grouping at most);
* the clips exercise the rules -- asserted from the restatement's diagnostics: blocks at the floor, blocks raised by the smoothing,
  ragged edge blocks in both directions;
* closed forms: a constant-grey original, and a 10-bit clip that is an 8-bit clip times 4;
* the plan queries of the C ABI (host calls, no GPU) against the restatement, and the entries' refusals with null device pointers;
* csrc/xpsnr_plan.h on the host under AddressSanitizer + UBSan: a stand-alone program (tests/host/xpsnr_stub.cpp) run as a
  subprocess; nothing is loaded into this interpreter."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import xpsnr_ref as ref
from pnp_vcve_amd import _native, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 1001
A = 0x1000        # an aligned "device address": never dereferenced on these paths
T = 4
_CLIPS = {}


def clip(h, w, d=8, t=T):
    key = (h, w, d, t)
    if key not in _CLIPS:
        _CLIPS[key] = ref.test_clip(t, h, w, d, seed=1)
    return _CLIPS[key]


def agree(got, want, tag):
    assert got['sums'].dtype == np.int64 and np.array_equal(got['sums'], want['sums']), tag
    for k in ('wsse', 'frames', 'clip'):
        rel = float(np.max(np.abs(got[k] - want[k]) / np.abs(want[k])))
        print(tag, k, 'max relative difference', rel)
        assert got[k].dtype == np.float64 and rel <= 1e-12, (tag, k, rel)


@pytest.mark.parametrize('d', [8, 10, 12])
@pytest.mark.parametrize('h,w', [(54, 70), (122, 204)])
def test_host_path_against_the_independent_restatement(h, w, d):
    o, r = clip(h, w, d)
    for fps in (30, 60):
        for crop in (0, 2):
            want = ref.xpsnr(o, r, d, fps, crop)
            agree(metrics.xpsnr(o, r, d, fps, crop), want, f'{h}x{w} d {d} fps {fps} crop {crop}')
            assert np.isfinite(want['clip']).all() and (want['clip'] > 20).all() and (want['clip'] < 60).all()
            if crop == 0:       # the clip exercises the rules
                g = want['diag']
                print(g)
                assert g['n'] == (4 if h == 54 else 8) and g['b'] == 1
                assert g['floored'] >= 1 and g['smoothed'] >= 1 and g['ragged_rows'] == 1 and g['ragged_cols'] == 1 and g['empty'] == 0
    # t = 0 has no temporal term, t = 1 is first order whatever the rate, t >= 2 differs between 30 and 60 frames a second
    s30, s60 = ref.xpsnr(o, r, d, 30)['sums'], ref.xpsnr(o, r, d, 60)['sums']
    assert (s30[0, :, 4] == 0).all() and (s30[1:, :, 4] > 0).any()
    assert np.array_equal(s30[:2], s60[:2]) and not np.array_equal(s30[2:, :, 4], s60[2:, :, 4]) and np.array_equal(s30[..., :4], s60[..., :4])


def test_the_6x6_filter_path_against_the_independent_restatement():
    """b = 2 needs more than 2048 x 1152 samples: 2064 x 1146, N = 68, ragged 24 and 58"""
    h, w = 1146, 2064
    o, r = clip(h, w, 8, 3)
    want = ref.xpsnr(o, r, 8, 60, 0)
    assert want['diag']['b'] == 2 and want['diag']['n'] == 68 and want['diag']['smoothed'] >= 1
    agree(metrics.xpsnr(o, r, 8, 60, 0), want, '2064x1146 b 2')
    assert (want['sums'][:, :, 3] > 0).all() and (want['sums'][1:, :, 4] > 0).all()


@pytest.mark.parametrize('d', [8, 10, 12])
def test_a_constant_grey_original_puts_every_block_at_the_floor(d):
    h, w = 54, 70
    rng = np.random.RandomState(d)
    o = [np.full((T, h, w), 1 << (d - 1)), np.full((T, h // 2, w // 2), 1 << (d - 1)), np.full((T, h // 2, w // 2), 1 << (d - 1))]
    r = [p + rng.randint(-2, 3, p.shape) for p in o]
    got = metrics.xpsnr(o, r, d, 30)
    assert (got['sums'][..., 3:] == 0).all()
    big_a = np.sqrt(16.0 * 2.0 ** (2 * d - 9) * np.sqrt(3840.0 * 2160.0 / (w * h)))
    wk = metrics.xpsnr_weights(got['sums'][0, :, 3].reshape(14, 18), got['sums'][0, :, 4].reshape(14, 18), metrics.xpsnr_areas(h, w), 0, 30, d, h, w)
    assert wk.shape == (14, 18) and (wk == big_a / 2.0 ** (d - 6)).all()
    # every weight alike: the weighted error is the weight times the plain squared error
    sse = got['sums'][..., :3].sum(axis=1).astype(np.float64)
    assert np.max(np.abs(got['wsse'] - sse * (big_a / 2.0 ** (d - 6))) / got['wsse']) <= 1e-12
    agree(got, ref.xpsnr(o, r, d, 30), f'grey d {d}')


def test_a_10_bit_clip_that_is_an_8_bit_clip_times_4():
    h, w = 122, 204
    o, r = clip(h, w, 8)
    o4, r4 = [p * 4 for p in o], [p * 4 for p in r]
    for fps in (30, 60):
        a, b = metrics.xpsnr(o, r, 8, fps), metrics.xpsnr(o4, r4, 10, fps)
        assert np.array_equal(b['sums'][..., :3], 16 * a['sums'][..., :3]) and np.array_equal(b['sums'][..., 3:], 4 * a['sums'][..., 3:])
        area = metrics.xpsnr_areas(h, w)
        for t in range(T):
            wa = metrics.xpsnr_weights(a['sums'][t, :, 3].reshape(area.shape), a['sums'][t, :, 4].reshape(area.shape), area, t, fps, 8, h, w)
            wb = metrics.xpsnr_weights(b['sums'][t, :, 3].reshape(area.shape), b['sums'][t, :, 4].reshape(area.shape), area, t, fps, 10, h, w)
            assert np.array_equal(wa, wb), (fps, t)                 # activity x 4, floor x 4, A x 4: every step a power of two


def test_single_block_and_refusals_of_the_host_path():
    one = [np.full((2, 4, 4), 9), np.full((2, 2, 2), 9), np.full((2, 2, 2), 9)]
    got = metrics.xpsnr(one, one, 8)
    assert got['sums'].shape == (2, 1, 5) and np.isinf(got['clip']).all() and np.isinf(got['frames']).all()      # a block with no neighbour; identical clips
    assert np.isfinite(metrics.xpsnr_weights(np.zeros((1, 1)), np.zeros((1, 1)), np.full((1, 1), 4), 0, 30, 8, 4, 4)).all()
    for bad in (dict(crop_border=1), dict(crop_border=-2), dict(d=9), dict(fps=0), dict(fps=29.97)):
        kw = dict(dict(d=8, fps=30, crop_border=0), **bad)
        with pytest.raises(ValueError):
            metrics.xpsnr(one, one, **kw)
    assert 'XPSNR' not in metrics.ALLOWED_METRICS                 # a plane metric: RGB / Y clips refuse the name like any unknown one


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def test_the_plan_queries_are_the_restatements(lib):
    expected = {(720, 1280): 44, (1080, 1920): 64, (2160, 3840): 128, (54, 70): 4, (122, 204): 8, (1146, 2064): 68}
    for (h, w), n in expected.items():
        for crop in (0, 2):
            H, W = h - 2 * crop, w - 2 * crop
            assert lib.pnp_xpsnr_block_size(h, w, crop) == ref.block_size(H, W) == metrics.xpsnr_plan(H, W)[0], (h, w, crop)
            if crop == 0:
                assert lib.pnp_xpsnr_block_size(h, w, 0) == n, (h, w)
            rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.pnp_xpsnr_grid(h, w, crop, ctypes.byref(rows), ctypes.byref(cols)) == 0
            assert (rows.value, cols.value) == ref.grid(H, W) == metrics.xpsnr_plan(H, W)[1:3], (h, w, crop)
            assert metrics.xpsnr_plan(H, W)[3] == ref.border(H, W)
            assert np.array_equal(metrics.xpsnr_areas(H, W).reshape(-1),
                                  [max(r[1] - r[0], 0) * max(r[3] - r[2], 0) for r in (ref.region(b, H, W, ref.border(H, W)) for b in ref.blocks(H, W))])
    assert ref.border(1146, 2064) == 2 and ref.border(1152, 2048) == 1 and ref.border(1142, 2060) == 1
    # the integer rounding of N is the floating-point formula's over a sweep of sizes
    for h in range(2, 2300, 94):
        for w in range(2, 4100, 166):
            assert lib.pnp_xpsnr_block_size(h, w, 0) == ref.block_size(h, w), (h, w)
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    for h, w, crop in ((0, 0, 0), (53, 70, 0), (54, 69, 0), (54, 70, 1), (54, 70, -2), (54, 70, 28), (8, 8, 4)):
        assert lib.pnp_xpsnr_block_size(h, w, crop) == 0, (h, w, crop)
        assert lib.pnp_xpsnr_grid(h, w, crop, ctypes.byref(rows), ctypes.byref(cols)) == BAD_ARG, (h, w, crop)
    assert lib.pnp_xpsnr_grid(54, 70, 0, None, ctypes.byref(cols)) == BAD_ARG and lib.pnp_xpsnr_grid(54, 70, 0, ctypes.byref(rows), None) == BAD_ARG
    assert lib.pnp_abi_version() == 5


def test_the_entries_refuse_on_the_host_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    def planes8(w, step=2, y=A):
        return _native.Yuv420Planes(y, A + 0x100000, A + (0x100001 if step == 2 else 0x200000), w, step * (w // 2), 1 << 22, 1 << 22, step)

    def planes16(w, depth=10, msb=0, y=A):
        return _native.Yuv420Planes16(y, A + 0x100000, A + 0x200000, 2 * w, w, 1 << 22, 1 << 22, 1, depth, msb)

    def call(a, b, entry, mask=1, sums=A, frames=2, h=54, w=70, crop=0, fps=30):
        return getattr(lib, entry)(ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None, mask, sums, frames, h, w,
                                   crop, fps, None)

    for entry, mk in (('pnp_xpsnr_sums_yuv420', planes8), ('pnp_xpsnr_sums_yuv420p16', planes16)):
        ok = mk(70)
        assert call(ok, ok, entry, mask=0) == BAD_ARG and call(ok, ok, entry, mask=8) == BAD_ARG and call(ok, ok, entry, mask=-1) == BAD_ARG
        assert call(ok, ok, entry, fps=0) == BAD_ARG and call(ok, ok, entry, fps=-30) == BAD_ARG
        assert call(ok, ok, entry, sums=None) == BAD_ARG and call(None, ok, entry) == BAD_ARG and call(ok, None, entry) == BAD_ARG
        assert call(ok, ok, entry, frames=0) == BAD_ARG
        assert call(ok, ok, entry, crop=1) == BAD_ARG and call(ok, ok, entry, crop=-2) == BAD_ARG and call(ok, ok, entry, crop=28) == BAD_ARG
        assert call(ok, ok, entry, h=53) == BAD_ARG and call(ok, ok, entry, w=72) == BAD_ARG          # odd rows; a pitch below the row
        for mask in (1, 2, 4, 7):                                                                      # the original's Y is the activity's source
            assert call(ok, mk(70, y=None), entry, mask=mask) == BAD_ARG, mask
    assert call(planes16(70, 10), planes16(70, 12), 'pnp_xpsnr_sums_yuv420p16') == BAD_ARG            # differing depths
    assert call(planes16(70, 9), planes16(70, 9), 'pnp_xpsnr_sums_yuv420p16') == BAD_ARG


# ------------------------------------------------------------------------------------------------ the plan under the sanitizers
def test_the_plan_on_the_host_under_asan(tmp_path):
    """tests/host/xpsnr_stub.cpp: a stand-alone program; nothing is loaded into this interpreter"""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'xpsnr_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'xpsnr_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    docs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert docs[0] == {'refusals': True, 'errors': []}
    cases = [d for d in docs if 'h' in d]
    assert docs[-1] == {'cases': len(cases)} and len(cases) >= 40
    for d in cases:
        assert d['errors'] == [], d
        H, W = d['h'] - 2 * d['crop'], d['w'] - 2 * d['crop']
        assert d['N'] == ref.block_size(H, W) and (d['rows'], d['cols']) == ref.grid(H, W), d
    by_b = {b_: [d for d in cases if d['b'] == b_] for b_ in (1, 2)}
    assert all(any(d['positions'] > 0 for d in v) for v in by_b.values())                  # both filters walked
    assert all(any(d['empty'] > 0 and d['positions'] == 0 for d in v) for v in by_b.values())      # a forced empty region with either border
    assert any(d['b'] == 2 and d['N'] == 128 for d in cases) and any(d['crop'] == 6 for d in cases)
    big = [d for d in cases if d['h'] == 1146 and d['crop'] == 0][0]
    assert big['b'] == 2 and big['positions'] == ((1146 - 4) // 2) * ((2064 - 4) // 2) and big['empty'] == 0
