"""CPU: the byte-frame boundary of the C ABI (pnp_generator_forward_clips, pnp_generator_workspace_bytes_io; include/pnpvcve.h).

* sizes and argument errors through ctypes on the built library: they are decided on the host, before any HIP call, so they run
  without a GPU and with null device buffers;
* the scheduler on the host under AddressSanitizer + UBSan (tests/host/byte_frames_stub.cpp over the unchanged
  tests/host/sched_stub.cpp harness): an fp32 batch given as descriptors issues pnp_generator_forward's launch list record for record;
  clips in separately allocated buffers are read and written inside their own buffers only, with exactly the bytes the layout names;
  each output mask writes exactly the buffers it asks for; the staging buffers exist only where a kernel keeps its fp32 interface
  and hold one frame."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8 = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC
BAD_ARG = 1001


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


def _align256(v):
    return (v + 255) // 256 * 256


# (constructor overrides, precision, bounded k or 0): plain, x4 heads, fp16 operands, split fp16, a bounded schedule, a DCN aligner
CONFIGS = [({}, 0, 0), (dict(vsr=1), 0, 0), ({}, 1, 0), ({}, 2, 0), ({}, 0, 14), (dict(vsr=1), 1, 0), (dict(deform=1), 0, 0),
           (dict(sparse_val=1), 0, 0)]


@pytest.mark.parametrize('over,prec,k', CONFIGS)
def test_workspace_bytes_io_equals_the_plain_query_at_the_fp32_boundary_and_adds_one_frame_at_most(lib, over, prec, k):
    h = _create(lib, **over)
    assert lib.pnp_generator_set_precision(h, prec) == 0
    assert lib.pnp_generator_set_max_resident(h, k) == 0
    os_ = 4 if over.get('vsr') else 1
    for valu in (1, 0):
        assert lib.pnp_generator_set_option(h, _native.OPT_CONV_LAST_VALU, valu) == 0
        # the kernels that keep an fp32 interface: the fp16 path's RGB body, and the matrix-core conv_last
        staged = prec == 1 or not valu
        for t, hh, ww in ((7, 128, 128), (20, 180, 320), (7, 720, 1280)):
            plain = lib.pnp_generator_workspace_bytes(h, t, hh, ww)
            assert plain > 0
            assert lib.pnp_generator_workspace_bytes_io(h, t, hh, ww, F32, _native.OUT_F32) == plain
            lr1, out1 = _align256(hh * ww * 12), _align256(hh * ww * 12 * os_ * os_)
            for fmt in (F32, U8):
                for mask in (1, 2, 3):
                    want = plain + (lr1 if staged and fmt == U8 else 0) + (out1 if staged and mask == 2 else 0)
                    assert lib.pnp_generator_workspace_bytes_io(h, t, hh, ww, fmt, mask) == want, (fmt, mask, valu)
    for fmt, mask in ((2, 1), (-1, 1), (U8, 0), (U8, 4), (F32, 7), (F32, -1)):
        assert lib.pnp_generator_workspace_bytes_io(h, 7, 128, 128, fmt, mask) == -1
    if k:       # a bound below the minimum: -1 from both queries
        assert lib.pnp_generator_set_max_resident(h, 2) == 0
        assert lib.pnp_generator_workspace_bytes(h, 40, 128, 128) == -1
        assert lib.pnp_generator_workspace_bytes_io(h, 40, 128, 128, U8, 2) == -1
    lib.pnp_generator_destroy(h)


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    h = _create(lib)
    side = (ctypes.c_float * 2)(73.0, 80.0)
    a = 0x1000        # an aligned "device address": never dereferenced on these paths

    def call(clips, n, fmt, mask, hh=128, ww=128, ws=None, ws_bytes=0, t=1):
        arr = (_native.ClipIO * max(len(clips), 1))(*[_native.ClipIO(*c) for c in clips])
        return lib.pnp_generator_forward_clips(h, None, None, ctypes.cast(arr, ctypes.c_void_p) if clips else None, n, fmt, mask, side, side,
                                               side, ws, ws_bytes, t, hh, ww, None)

    ok = (a, a, a, a, a)
    assert call([ok], 1, 2, 1) == BAD_ARG and call([ok], 1, -1, 1) == BAD_ARG                  # unknown format
    assert call([ok], 1, U8, 0) == BAD_ARG and call([ok], 1, U8, 4) == BAD_ARG and call([ok], 1, F32, 8) == BAD_ARG      # mask
    assert call([], 1, U8, 2) == BAD_ARG and call([ok], 0, U8, 2) == BAD_ARG                   # no descriptors, no clips
    assert call([(None, a, a, a, a)], 1, U8, 2) == BAD_ARG                                     # required pointers
    assert call([(a, None, a, a, a)], 1, U8, 2) == BAD_ARG and call([(a, a, None, a, a)], 1, U8, 2) == BAD_ARG
    assert call([(a, a, a, None, a)], 1, U8, 1) == BAD_ARG and call([(a, a, a, None, a)], 1, U8, 3) == BAD_ARG
    assert call([(a, a, a, a, None)], 1, U8, 2) == BAD_ARG and call([(a, a, a, a, None)], 1, F32, 3) == BAD_ARG
    assert call([ok, (a, a, a, a, None)], 2, U8, 2) == BAD_ARG                                 # ... of every clip
    assert call([(a + 2, a, a, a, a)], 1, U8, 1) == BAD_ARG                                    # uint8 pointers: 4-byte aligned
    assert call([(a, a, a, a, a + 1)], 1, F32, 2) == BAD_ARG
    # what the mask does not ask for may be NULL, an fp32 frame pointer needs no more than it did: these pass the new checks and
    # stop where pnp_generator_forward stops -- size (1004, 1005), then the (null) workspace (1003)
    assert call([(a, a, a, None, a)], 1, U8, 2) == 1003 and call([(a, a, a, a, None)], 1, U8, 1) == 1003
    assert call([ok], 1, U8, 3, hh=60) == 1004 and call([ok], 1, U8, 3, ww=66) == 1005
    assert call([ok], 1, U8, 2, hh=4096, ww=4096) == 1002
    assert call([ok], 1, U8, 2, t=0) == BAD_ARG
    lib.pnp_generator_destroy(h)
    hs = _create(lib, sparse_val=1)            # sparse_val evaluates one clip at a time, as before
    arr = (_native.ClipIO * 2)(_native.ClipIO(*ok), _native.ClipIO(*ok))
    assert lib.pnp_generator_forward_clips(hs, None, None, ctypes.cast(arr, ctypes.c_void_p), 2, U8, 2, side, side, side, None, 0, 1, 128, 128,
                                           None) == 1002
    lib.pnp_generator_destroy(hs)
    # a bound below the minimum
    hb = _create(lib)
    assert lib.pnp_generator_set_max_resident(hb, 2) == 0
    sl = (ctypes.c_float * 40)(*([73.0] * 40))
    one = (_native.ClipIO * 1)(_native.ClipIO(*ok))
    assert lib.pnp_generator_forward_clips(hb, None, None, ctypes.cast(one, ctypes.c_void_p), 1, U8, 2, sl, sl, sl, None, 0, 40, 128, 128,
                                           None) == BAD_ARG
    lib.pnp_generator_destroy(hb)


def test_the_ctypes_struct_is_the_headers():
    with open(os.path.join(ROOT, 'include', 'pnpvcve.h')) as fh:
        hdr = fh.read()
    body = hdr[hdr.index('typedef struct pnp_clip_io {'):hdr.index('} pnp_clip_io;')]
    import re
    names = re.findall(r'(\w+);', body)
    assert names == [f[0] for f in _native.ClipIO._fields_]
    assert ctypes.sizeof(_native.ClipIO) == 5 * ctypes.sizeof(ctypes.c_void_p)
    for name, val in (('PNP_FRAMES_F32_NCHW', F32), ('PNP_FRAMES_U8_HWC', U8), ('PNP_OUT_F32', _native.OUT_F32), ('PNP_OUT_U8', _native.OUT_U8)):
        assert int(re.search(r'#define %s (\d+)' % name, hdr).group(1)) == val


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('bytes') / 'byte_frames_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'byte_frames_stub.cpp'), '-o', exe]
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
    assert len(out) == 20
    for name, d in out.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
    return out


def test_descriptors_of_an_fp32_batch_issue_the_same_launch_list(docs):
    """(a) pnp_generator_forward is the descriptor call with its strides: launches, convs with every argument, warps, expert mixes,
    event records and waits, in order"""
    for name in ('same_128_n3_ctx3', 'same_720_band', 'same_128_bounded', 'same_128_f16'):
        d = docs[name]
        assert d['same'] == 1 and d['records'] > 100, (name, d['first_diff'])
        assert d['n_pack'] == d['n_from'] == d['n_to'] == d['n_last_io'] == 0          # no byte launcher at the fp32 boundary
    assert docs['same_128_n3_ctx3']['streams_used'] == [1, 2, 3]                        # three contexts on three side streams
    assert docs['same_720_band']['banded'] > 0                                         # band chains were on


def test_byte_clips_are_read_and_written_inside_their_own_buffers(docs):
    """(b) separately allocated clips (the stub's own checks are in `errors`, asserted empty by the fixture): one pack launch per clip
    over exactly its bytes, the last conv reads and writes bytes itself, nothing takes the frame as fp32 planes"""
    for name in ('u8_128_n2_mask2', 'u8_720_band_n2_mask2', 'u8_128_bounded_mask2', 'u8_vsr_mask3', 'u8_sparse_mask2', 'u8_x3_mask2',
                 'u8_direct_convs_mask1', 'u8_128_n2_mask1', 'u8_128_n2_mask3'):
        d = docs[name]
        assert d['staged'] == 0 and d['ctx_bytes'] == d['plain_bytes'], name
        assert d['n_pack'] == d['frames'] // (9 if 'bounded' in name else 2 if ('720' in name or 'vsr' in name) else 3), name
        assert d['n_last_io'] == d['frames'] and d['rgb_heads_fp32_interface'] == 0 and d['n_from'] == d['n_to'] == 0, name
    assert len(docs['u8_128_n2_mask2']['streams_used']) == 3                            # two contexts: the caller's stream + two
    assert docs['u8_720_band_n2_mask2']['banded'] > 0 and docs['u8_720_band_n2_mask2']['streams_used'] == [0]
    # (a bounded schedule recomputes backward branches, never a last conv: nine frames, nine byte frames out)
    assert docs['u8_128_bounded_mask2']['n_last_io'] == 9


def test_each_mask_writes_exactly_what_it_asks_for(docs):
    """(c) the stub allocates both outputs of every clip whatever the mask and fails a scenario whose unrequested buffer was touched
    or whose requested one was not completely written; fp32 frames in with bytes out go through the same kernel"""
    for name in ('u8_128_n2_mask1', 'u8_128_n2_mask2', 'u8_128_n2_mask3', 'f32_128_n2_mask2', 'f32_128_n2_mask3'):
        d = docs[name]
        assert d['n_last_io'] == 6 and d['rgb_heads_fp32_interface'] == 0, name
        assert d['n_pack'] == (2 if name.startswith('u8') else 0), name


def test_kernels_with_an_fp32_interface_stage_one_frame(docs):
    for name, lr1, out1 in (('u8_f16_mask2', 1, 1), ('u8_f16_mask3', 1, 0), ('u8_f16_vsr_mask2', 1, 1), ('u8_mfma_last_mask2', 1, 1),
                            ('f32_mfma_last_mask2', 0, 1)):
        d = docs[name]
        assert d['staged'] == 1 and d['n_last_io'] == 0 and d['rgb_heads_fp32_interface'] == d['frames'], name
        assert d['n_from'] == lr1 * d['frames'] and d['n_to'] == d['frames'], name
        assert d['ctx_bytes'] - d['plain_bytes'] == lr1 * _align256(d['frame_bytes']) + out1 * _align256(d['out_frame_bytes']), name
