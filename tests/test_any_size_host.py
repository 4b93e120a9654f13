"""CPU: the any_size switch of the C ABI (pnp_generator_set_any_size; include/pnpvcve.h).

* through ctypes on the built library, with null device buffers and no GPU: with the switch off every refusal is what it was
  (PNP_ERR_SIZE_VALUE for a frame that is no multiple of 4, PNP_ERR_BAD_ARG for a byte clip that is not 4-byte aligned); with it on
  those frames pass the size checks, the workspace queries size them, and a DCN aligner is refused;
* the scheduler on the host under AddressSanitizer + UBSan (tests/host/any_size_stub.cpp over the unchanged tests/host/sched_stub.cpp
  recording launchers) at 65x65, 66x79, 73x67, 177x193, 480x854 and 1078x1918: plain, bounded at the minimum k, two byte clips by
  pointer at odd addresses, and the x4 heads -- no byte range outside its buffer, every output frame written exactly once."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8 = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC
BAD_ARG, UNSUPPORTED, WORKSPACE, SIZE_ASSERT, SIZE_VALUE = 1001, 1002, 1003, 1004, 1005
RAGGED = ((65, 65), (66, 79), (73, 67), (67, 129), (177, 193), (480, 854), (1078, 1918))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def _create(lib, **over):
    kw = dict(mid_channels=64, num_blocks=2, num_experts=6, with_cat=1, use_base_qp=1, expert_softmax=1, with_bias=1,
              with_se=1, one_layer=1, channel_first=1, align_key=1, vsr=0, deform=0)
    kw.update(over)
    h = ctypes.c_void_p()
    assert lib.pnp_generator_create(ctypes.byref(_native.GeneratorCfg(**kw)), ctypes.byref(h)) == 0
    return h


SIDE = (ctypes.c_float * 2)(73.0, 80.0)
A = 0x1000        # an aligned "device address": never dereferenced on these paths


def _forward(lib, g, hh, ww):
    return lib.pnp_generator_forward(g, None, None, None, None, None, SIDE, SIDE, SIDE, None, None, 0, 1, 1, hh, ww, None)


def _clips(lib, g, clip, fmt, mask, hh=128, ww=128):
    arr = (_native.ClipIO * 1)(_native.ClipIO(*clip))
    return lib.pnp_generator_forward_clips(g, None, None, ctypes.cast(arr, ctypes.c_void_p), 1, fmt, mask, SIDE, SIDE, SIDE, None, 0, 1, hh, ww, None)


def test_the_switch_is_off_by_default_and_the_refusals_are_what_they_were(lib):
    g = _create(lib)
    assert lib.pnp_generator_get_any_size(g) == 0
    assert lib.pnp_generator_get_any_size(None) == -1
    assert lib.pnp_generator_set_any_size(None, 1) == BAD_ARG and lib.pnp_generator_set_any_size(g, -1) == BAD_ARG
    for hh, ww in RAGGED + ((64, 66), (66, 64)):
        assert _forward(lib, g, hh, ww) == SIZE_VALUE, (hh, ww)
        assert _clips(lib, g, (A, A, A, A, A), U8, 3, hh, ww) == SIZE_VALUE, (hh, ww)
    assert _forward(lib, g, 63, 65) == SIZE_ASSERT
    assert _forward(lib, g, 64, 72) == WORKSPACE                       # a multiple of 4: on to the (null) workspace
    # the byte clip the aligned unpacking kernel cannot read, and the byte output: refused before any HIP call
    for off in (1, 2, 3):
        assert _clips(lib, g, (A + off, A, A, A, A), U8, 1) == BAD_ARG
        assert _clips(lib, g, (A, A, A, A, A + off), F32, 2) == BAD_ARG
    lib.pnp_generator_destroy(g)


def test_with_the_switch_on_such_frames_pass_the_size_checks(lib):
    g = _create(lib)
    assert lib.pnp_generator_set_any_size(g, 1) == 0 and lib.pnp_generator_get_any_size(g) == 1
    for hh, ww in RAGGED:
        assert _forward(lib, g, hh, ww) == WORKSPACE, (hh, ww)          # passed every size check, stopped at the (null) workspace
        assert _clips(lib, g, (A + 1, A, A, A, A + 3), U8, 3, hh, ww) == WORKSPACE, (hh, ww)      # ... a byte clip at any address too
    assert _forward(lib, g, 63, 65) == SIZE_ASSERT and _forward(lib, g, 65, 63) == SIZE_ASSERT      # h, w >= 64 in both modes
    assert _forward(lib, g, 4097, 4097) == UNSUPPORTED                 # the 32-bit addressing limit, host-side as ever
    assert _clips(lib, g, (None, A, A, A, A), U8, 1, 65, 65) == BAD_ARG
    assert lib.pnp_generator_set_any_size(g, 0) == 0 and _forward(lib, g, 65, 65) == SIZE_VALUE       # and off again
    assert lib.pnp_generator_set_any_size(g, 7) == 0 and lib.pnp_generator_get_any_size(g) == 1       # a boolean
    lib.pnp_generator_destroy(g)


@pytest.mark.parametrize('deform', [1, 2])
def test_the_dcn_aligners_are_refused_with_the_switch_on(lib, deform):
    g = _create(lib, deform=deform)
    assert _forward(lib, g, 65, 65) == SIZE_VALUE and _forward(lib, g, 64, 64) == WORKSPACE
    assert lib.pnp_generator_set_any_size(g, 1) == 0
    assert _forward(lib, g, 65, 65) == UNSUPPORTED and _forward(lib, g, 64, 64) == UNSUPPORTED
    assert _clips(lib, g, (A, A, A, A, A), U8, 2, 66, 79) == UNSUPPORTED
    lib.pnp_generator_destroy(g)


@pytest.mark.parametrize('over,prec,k', [({}, 0, 0), (dict(vsr=1), 0, 0), ({}, 1, 0), ({}, 2, 0), ({}, 0, -1), (dict(sparse_val=1), 0, 0)])
def test_the_workspace_queries_size_any_frame_and_grow_with_it(lib, over, prec, k):
    g = _create(lib, **over)
    t = 9
    assert lib.pnp_generator_set_precision(g, prec) == 0
    assert lib.pnp_generator_set_max_resident(g, lib.pnp_generator_min_resident(g, t) if k < 0 else k) == 0      # (-1: bounded, at the minimum)
    # each ragged size between its two neighbours on the grid of 4, and the sizes among each other: strictly monotone in h * w
    ladder = [(64, 64), (65, 65), (68, 68), (64, 80), (66, 79), (68, 80), (480, 852), (480, 854), (480, 856), (1076, 1916), (1078, 1918), (1080, 1920)]
    assert [a * b for a, b in ladder] == sorted(a * b for a, b in ladder)
    before = [lib.pnp_generator_workspace_bytes(g, t, hh, ww) for hh, ww in ladder]
    assert lib.pnp_generator_set_any_size(g, 1) == 0
    for fmt, mask in ((F32, 1), (U8, 2), (U8, 3)):
        sizes = [lib.pnp_generator_workspace_bytes_io(g, t, hh, ww, fmt, mask) for hh, ww in ladder]
        assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        if (fmt, mask) == (F32, 1):
            assert sizes == [lib.pnp_generator_workspace_bytes(g, t, hh, ww) for hh, ww in ladder]
            assert sizes == before            # the switch changes no size
    lib.pnp_generator_destroy(g)


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('anysize') / 'any_size_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'any_size_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith('{'):
            d = json.loads(ln)
            out[d['name']] = d
    return out


STUB_SIZES = ('65x65', '66x79', '73x67', '177x193', '480x854', '1078x1918')


def test_the_scheduler_stays_inside_every_buffer_and_writes_every_output_frame_once(docs):
    """the stub's own checks (ranges against ASan's shadow, reads of unwritten bytes, outputs written exactly once) are in `errors`"""
    want = {f'{kind}_{sz}' for sz in STUB_SIZES for kind in ('plain', 'bounded', 'clips', 'heads')} - {'heads_1078x1918'}
    assert set(docs) == want
    for name, d in docs.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
        assert d['rc_off'] == SIZE_VALUE, name


def test_the_routing_at_ragged_sizes(docs):
    """65x65 .. 73x67 are 25 tiles: the quadrant-unit kernels; 177x193 is 12 x 13 = 156 tiles, 480x854 1620: the tile kernels; row-band
    chains wherever one clip is in flight on the tile kernels, and none with two contexts"""
    for sz in STUB_SIZES:
        small = sz in ('65x65', '66x79', '73x67')
        for kind in ('plain', 'bounded'):
            d = docs[f'{kind}_{sz}']
            assert (d['wino_units'] > 0 and d['wino_tiles'] == 0 and d['banded'] == 0) if small else \
                (d['wino_units'] == 0 and d['wino_tiles'] > 0 and d['banded'] == d['wino_tiles']), (kind, sz, d)
        c = docs[f'clips_{sz}']
        assert c['n_pack'] == 2 and c['n_last_io'] == c['frames']          # one unpacking launch per clip, bytes out of every last conv
        assert c['banded'] == (c['wino_tiles'] if sz == '1078x1918' else 0), (sz, c)
