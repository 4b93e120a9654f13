"""CPU: the Y'CbCr 4:2:0 boundary of the C ABI (pnp_generator_forward_clips_yuv, pnp_generator_workspace_bytes_yuv, pnp_frames_from_yuv420,
pnp_frames_to_yuv420; include/pnpvcve.h).

* sizes and argument errors through ctypes on the built library: they are decided on the host, before any HIP call, so they run
  without a GPU and with null device buffers;
* the entry points that existed keep their refusals (format 2, masks beyond 3);
* the scheduler on the host under AddressSanitizer + UBSan (tests/host/yuv_stub.cpp over the unchanged tests/host/sched_stub.cpp
  harness): planes at odd addresses with odd pitches are read and written inside their rows only, every output sample exactly once,
  and apart from the pack launch, conv_last's arguments and the converters the launch list is the fp32 boundary's, record for record."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED, WORKSPACE, SIZE_ASSERT, SIZE_VALUE = 1001, 1002, 1003, 1004, 1005
A = 0x1000        # an aligned "device address": never dereferenced on these paths


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


def planes(w, y=A, cb=A + 0x100000, cr=A + 0x100001, y_pitch=None, c_pitch=None, c_step=2, frame=1 << 22):
    return _native.Yuv420Planes(y, cb, cr, w if y_pitch is None else y_pitch, c_step * (w // 2) if c_pitch is None else c_pitch, frame, frame,
                                c_step)


def clip(w, W=None, lq=None, mvs=A, par=A, f32=A, u8=A, out=None):
    W = w if W is None else W
    return _native.ClipYuv(lq if lq is not None else planes(w), mvs, par, f32, u8, out if out is not None else planes(W))


# (constructor overrides, precision, bounded k or 0): the grid of tests/test_byte_frames_host.py
CONFIGS = [({}, 0, 0), (dict(vsr=1), 0, 0), ({}, 1, 0), ({}, 2, 0), ({}, 0, 14), (dict(vsr=1), 1, 0), (dict(deform=1), 0, 0),
           (dict(sparse_val=1), 0, 0)]


@pytest.mark.parametrize('over,prec,k', CONFIGS)
def test_workspace_bytes_yuv_is_the_plain_query_plus_exactly_the_staged_frames(lib, over, prec, k):
    h = _create(lib, **over)
    assert lib.pnp_generator_set_precision(h, prec) == 0
    assert lib.pnp_generator_set_max_resident(h, k) == 0
    os_ = 4 if over.get('vsr') else 1
    for valu in (1, 0):
        assert lib.pnp_generator_set_option(h, _native.OPT_CONV_LAST_VALU, valu) == 0
        # the kernels that keep an fp32 interface: the fp16 path's RGB body, and the matrix-core conv_last
        staged = prec == 1 or not valu
        for t, hh, ww in ((7, 128, 128), (20, 180, 320), (7, 720, 1280), (3, 66, 70)):
            plain = lib.pnp_generator_workspace_bytes(h, t, hh, ww)
            assert plain > 0
            lr1, out1 = _align256(hh * ww * 12), _align256(hh * ww * 12 * os_ * os_)
            for mask in range(1, 8):
                # an output frame of fp32 planes exists only where bytes or planes are made of an fp32 frame the caller did not ask for
                need_out1 = not mask & 1 and (bool(mask & 4) or (staged and bool(mask & 2)))
                want = plain + (lr1 if staged else 0) + (out1 if need_out1 else 0)
                assert lib.pnp_generator_workspace_bytes_yuv(h, t, hh, ww, mask) == want, (mask, valu, t, hh, ww)
            # the queries that existed are what they were
            assert lib.pnp_generator_workspace_bytes_io(h, t, hh, ww, 0, 1) == plain
            assert lib.pnp_generator_workspace_bytes_io(h, t, hh, ww, 1, 2) == plain + (lr1 + out1 if staged else 0)
    for mask in (0, 8, -1, 15):
        assert lib.pnp_generator_workspace_bytes_yuv(h, 7, 128, 128, mask) == -1
    assert lib.pnp_generator_workspace_bytes_yuv(None, 7, 128, 128, 1) == -1
    if k:       # a bound below the minimum: -1
        assert lib.pnp_generator_set_max_resident(h, 2) == 0
        assert lib.pnp_generator_workspace_bytes_yuv(h, 40, 128, 128, 4) == -1
    lib.pnp_generator_destroy(h)


def test_the_entries_that_existed_still_refuse_format_2_and_mask_4(lib):
    h = _create(lib)
    side = (ctypes.c_float * 2)(73.0, 80.0)
    arr = (_native.ClipIO * 1)(_native.ClipIO(A, A, A, A, A))
    call = lambda fmt, mask: lib.pnp_generator_forward_clips(h, None, None, ctypes.cast(arr, ctypes.c_void_p), 1, fmt, mask, side, side, side,      # noqa: E731
                                                             None, 0, 1, 128, 128, None)
    assert call(2, 1) == BAD_ARG and call(1, 4) == BAD_ARG and call(0, 5) == BAD_ARG and call(0, 7) == BAD_ARG
    assert call(1, 3) == WORKSPACE
    for fmt, mask in ((2, 1), (0, 4), (1, 4), (0, 7)):
        assert lib.pnp_generator_workspace_bytes_io(h, 7, 128, 128, fmt, mask) == -1
    assert lib.pnp_abi_version() == 5
    lib.pnp_generator_destroy(h)


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    h = _create(lib)
    side = (ctypes.c_float * 2)(73.0, 80.0)

    def call(clips, n=None, std=0, mask=7, hh=128, ww=128, t=1, g=h, ws=None, ws_bytes=0):
        arr = (_native.ClipYuv * max(len(clips), 1))(*clips)
        return lib.pnp_generator_forward_clips_yuv(g, None, None, ctypes.cast(arr, ctypes.c_void_p) if clips else None, len(clips) if n is None else n,
                                                   std, mask, side, side, side, ws, ws_bytes, t, hh, ww, None)

    ok = clip(128)
    assert call([ok]) == WORKSPACE                                                  # everything in order up to the (null) workspace
    assert call([ok], std=4) == BAD_ARG and call([ok], std=-1) == BAD_ARG           # unknown standard
    assert call([ok], mask=0) == BAD_ARG and call([ok], mask=8) == BAD_ARG and call([ok], mask=-1) == BAD_ARG
    assert call([]) == BAD_ARG and call([ok], n=0) == BAD_ARG and call([ok], g=None) == BAD_ARG
    for field in ('y', 'cb', 'cr'):                                                 # a NULL plane of the frames ...
        assert call([clip(128, lq=planes(128, **{field: None}))]) == BAD_ARG, field
        bad_out = clip(128, out=planes(128, **{field: None}))                       # ... or of the output the mask needs
        for mask in (4, 5, 6, 7):
            assert call([bad_out], mask=mask) == BAD_ARG, (field, mask)
        for mask in (1, 2, 3):
            assert call([bad_out], mask=mask) == WORKSPACE, (field, mask)
    assert call([clip(128, mvs=None)]) == BAD_ARG and call([clip(128, par=None)]) == BAD_ARG
    assert call([clip(128, f32=None)], mask=1) == BAD_ARG and call([clip(128, f32=None)], mask=5) == BAD_ARG
    assert call([clip(128, f32=None)], mask=6) == WORKSPACE
    assert call([clip(128, u8=None)], mask=2) == BAD_ARG and call([clip(128, u8=None)], mask=5) == WORKSPACE
    assert call([ok, clip(128, mvs=None)]) == BAD_ARG                               # ... of every clip
    for step in (0, 3, -1):                                                         # c_step 1 | 2
        assert call([clip(128, lq=planes(128, c_step=step, c_pitch=256))]) == BAD_ARG, step
        assert call([clip(128, out=planes(128, c_step=step, c_pitch=256))], mask=4) == BAD_ARG, step
    assert call([clip(128, lq=planes(128, y_pitch=127))]) == BAD_ARG                # a pitch below the row's bytes
    assert call([clip(128, lq=planes(128, c_pitch=127))]) == BAD_ARG
    assert call([clip(128, lq=planes(128, c_step=1, c_pitch=63))]) == BAD_ARG
    assert call([clip(128, out=planes(128, y_pitch=127))], mask=4) == BAD_ARG and call([clip(128, out=planes(128, y_pitch=127))], mask=3) == WORKSPACE
    # any address, any pitch that holds a row, both chroma orders, I420
    assert call([clip(128, lq=planes(128, y=A + 1, cb=A + 0x100003, cr=A + 0x100002, y_pitch=131, c_pitch=129))]) == WORKSPACE
    assert call([clip(128, lq=planes(128, c_step=1, cb=A + 0x100001, cr=A + 0x200003, c_pitch=65))]) == WORKSPACE
    # odd h or w: BAD_ARG whatever else is wrong with the size; then the forward's own checks in their order
    assert call([ok], hh=127) == BAD_ARG and call([ok], ww=129) == BAD_ARG and call([ok], hh=63) == BAD_ARG
    assert call([clip(60)], hh=60, ww=60) == SIZE_ASSERT and call([clip(128)], hh=62) == SIZE_ASSERT
    assert call([clip(70)], hh=66, ww=70) == SIZE_VALUE and call([clip(128)], hh=66) == SIZE_VALUE
    assert call([clip(70)], hh=60, ww=70) == SIZE_ASSERT                            # (the assert comes first, as ever)
    assert call([clip(4096)], hh=4096, ww=4096) == UNSUPPORTED
    assert call([ok], t=0) == BAD_ARG
    assert lib.pnp_generator_set_any_size(h, 1) == 0                                # every even size >= 64 runs; odd ones stay refused
    assert call([clip(70)], hh=66, ww=70) == WORKSPACE and call([clip(70)], hh=65, ww=70) == BAD_ARG and call([clip(71)], hh=66, ww=71) == BAD_ARG
    assert call([clip(70)], hh=62, ww=70) == SIZE_ASSERT
    assert call([clip(128, u8=A + 1)], mask=2) == WORKSPACE                         # (a byte output at any address, as on the byte entry)
    assert lib.pnp_generator_set_any_size(h, 0) == 0
    assert call([clip(128, u8=A + 1)], mask=2) == BAD_ARG
    # the x4 heads: the output planes hold 4h x 4w
    hv = _create(lib, vsr=1)
    assert call([clip(128, W=512)], g=hv) == WORKSPACE and call([clip(128, W=128)], g=hv, mask=4) == BAD_ARG and call([clip(128, W=128)], g=hv, mask=3) == WORKSPACE
    lib.pnp_generator_destroy(hv)
    # a workspace that is too small or misaligned
    need = lib.pnp_generator_workspace_bytes_yuv(h, 1, 128, 128, 7)
    assert call([ok], ws=ctypes.c_void_p(A), ws_bytes=need - 1) == WORKSPACE and call([ok], ws=ctypes.c_void_p(A + 16), ws_bytes=need) == WORKSPACE
    lib.pnp_generator_destroy(h)
    hs = _create(lib, sparse_val=1)            # sparse_val evaluates one clip at a time, as before
    assert call([ok, ok], g=hs) == UNSUPPORTED
    lib.pnp_generator_destroy(hs)
    hb = _create(lib)                          # a bound below the minimum
    assert lib.pnp_generator_set_max_resident(hb, 2) == 0
    sl = (ctypes.c_float * 40)(*([73.0] * 40))
    one = (_native.ClipYuv * 1)(ok)
    assert lib.pnp_generator_forward_clips_yuv(hb, None, None, ctypes.cast(one, ctypes.c_void_p), 1, 0, 4, sl, sl, sl, None, 0, 40, 128, 128,
                                               None) == BAD_ARG
    lib.pnp_generator_destroy(hb)


def test_the_converters_refuse_bad_arguments_before_any_hip_call(lib):
    p = planes(64)
    frm = lambda d, std=0, out=A, n=1, hh=64, ww=64: lib.pnp_frames_from_yuv420(ctypes.byref(d) if d is not None else None, std, out, n, hh, ww, None)      # noqa: E731
    to = lambda d, std=0, src=A, n=1, hh=64, ww=64: lib.pnp_frames_to_yuv420(src, ctypes.byref(d) if d is not None else None, std, n, hh, ww, None)      # noqa: E731
    for f in (frm, to):
        assert f(None) == BAD_ARG and f(p, std=4) == BAD_ARG and f(p, n=0) == BAD_ARG and f(p, hh=63) == BAD_ARG and f(p, ww=65) == BAD_ARG
        assert f(planes(64, y=None)) == BAD_ARG and f(planes(64, cr=None)) == BAD_ARG and f(planes(64, c_step=4)) == BAD_ARG
        assert f(planes(64, y_pitch=63)) == BAD_ARG and f(planes(64, c_pitch=63)) == BAD_ARG
    assert frm(p, out=None) == BAD_ARG and to(p, src=None) == BAD_ARG


def test_the_ctypes_structs_are_the_headers():
    with open(os.path.join(ROOT, 'include', 'pnpvcve.h')) as fh:
        hdr = fh.read()
    strip = lambda s: re.sub(r'/\*.*?\*/', '', s, flags=re.S)      # noqa: E731
    body = strip(hdr[hdr.index('typedef struct pnp_yuv420_planes {'):hdr.index('} pnp_yuv420_planes;')])
    assert re.findall(r'(\w+)[,;]', body) == [f[0] for f in _native.Yuv420Planes._fields_]
    body = strip(hdr[hdr.index('typedef struct pnp_clip_yuv {'):hdr.index('} pnp_clip_yuv;')])
    assert re.findall(r'(\w+)[,;]', body) == [f[0] for f in _native.ClipYuv._fields_]
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_native.Yuv420Planes) == 3 * P + 4 * 8 + 8                 # three pointers, four int64, an int and its padding
    assert ctypes.sizeof(_native.ClipYuv) == 2 * ctypes.sizeof(_native.Yuv420Planes) + 4 * P
    assert ctypes.sizeof(_native.ClipIO) == 5 * P                                   # the struct that existed is five pointers
    for name, val in (('PNP_OUT_F32', 1), ('PNP_OUT_U8', 2), ('PNP_OUT_YUV420', _native.OUT_YUV420), ('PNP_YUV_BT601_LIMITED', 0),
                      ('PNP_YUV_BT601_FULL', 1), ('PNP_YUV_BT709_LIMITED', 2), ('PNP_YUV_BT709_FULL', 3)):
        assert int(re.search(r'#define %s (\d+)' % name, hdr).group(1)) == val
    assert _native.YUV_STANDARDS == {'bt601-limited': 0, 'bt601-full': 1, 'bt709-limited': 2, 'bt709-full': 3}
    import yuv_ref
    assert list(yuv_ref.STANDARDS) == sorted(_native.YUV_STANDARDS, key=_native.YUV_STANDARDS.get)


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('yuv') / 'yuv_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'yuv_stub.cpp'), '-o', exe]
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
    assert len(out) == 10
    for name, d in out.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
    return out


def test_the_launch_list_is_the_fp32_boundarys_apart_from_the_frames_way_in_and_out(docs):
    """the stub's own range checks (planes at odd addresses with odd pitches behind poisoned bytes; every output sample written exactly
    once) are in `errors`, asserted empty by the fixture; here: the trace and the launch counts"""
    for name, d in docs.items():
        assert d['same'] == 1 and d['records'] > 80, (name, d['first_diff'])
        clips = 2 if name.startswith('two_clips') else 1
        assert d['n_pack'] == clips, name                                      # ONE pack launch per clip, whatever the schedule recomputes
    assert docs['two_clips_nv12_mask7']['streams_used'] == [1, 2]              # two contexts on two side streams
    assert docs['bounded_i420_mask4']['frames'] == 9 and docs['bounded_i420_mask4']['n_to'] == 9


def test_conv_last_reads_the_rgb0_frame_and_output_planes_are_made_per_frame(docs):
    for name in ('plain_nv12_mask7', 'plain_nv21_mask4', 'vsr_i420_mask4', 'x3_nv12_mask5', 'bounded_i420_mask4', 'two_clips_nv12_mask7',
                 'any_size_66x70_nv12_mask7'):
        d = docs[name]
        mask = int(name.rsplit('mask', 1)[1])
        assert d['staged'] == 0 and d['n_from'] == 0 and d['n_to8'] == 0, name
        assert d['n_last_io'] == d['n_last_rgb0'] == d['frames'] and d['rgb_heads_fp32_interface'] == 0, name
        assert d['n_to'] == (d['frames'] if mask & 4 else 0), name
        # the workspace grows by one output frame of planes only where nobody asked for the fp32 output
        assert d['ctx_bytes'] - d['plain_bytes'] == (_align256(d['out_frame_bytes']) if mask & 4 and not mask & 1 else 0), name
        h, w = (66, 70) if 'any_size' in name else (128, 128) if ('mask7' in name or 'x3' in name) else (64, 96)
        s = 4 if 'vsr' in name else 1
        assert d['out_samples'] == (d['frames'] * h * s * w * s * 3 // 2 if mask & 4 else 0), name


def test_kernels_with_an_fp32_interface_stage_one_frame_each_way(docs):
    for name, out1 in (('f16_nv21_mask6', 1), ('f16_vsr_nv12_mask5', 0), ('mfma_last_i420_mask2', 1)):
        d = docs[name]
        mask = int(name.rsplit('mask', 1)[1])
        assert d['staged'] == 1 and d['n_last_io'] == 0 and d['rgb_heads_fp32_interface'] == d['frames'], name
        assert d['n_from'] == d['frames'] and d['n_to'] == (d['frames'] if mask & 4 else 0) and d['n_to8'] == (d['frames'] if mask & 2 else 0), name
        assert d['ctx_bytes'] - d['plain_bytes'] == _align256(d['frame_bytes']) + out1 * _align256(d['out_frame_bytes']), name
