"""CPU: the 10 / 12-bit 4:2:0 boundary of the C ABI (pnp_generator_forward_clips_yuv16, pnp_frames_from_yuv420p16, pnp_frames_to_yuv420p16,
pnp_psnr_sse_yuv420p16, pnp_ssim_partials_yuv420p16, pnp_debug_pack_lr_yuv420p16; include/pnpvcve.h).

* argument errors through ctypes on the built library: they are decided on the host, before any HIP call, so they run without a GPU
  and with null device buffers;
* the 8-bit entries and the workspace query return what they returned; pnp_abi_version() stays 5;
* the scheduler on the host under AddressSanitizer + UBSan (tests/host/yuv16_stub.cpp over the unchanged tests/host/sched_stub.cpp
  harness, a stand-alone program): planes at even addresses with ragged pitches are read and written inside their rows only, every
  output sample exactly once, and apart from the pack launch, the staged conversion and the output conversion the launch list is the
  8-bit 4:2:0 boundary's, record for record."""
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


def planes(w, y=A, cb=A + 0x100000, cr=A + 0x100002, y_pitch=None, c_pitch=None, c_step=2, frame=1 << 22, depth=10, msb=1):
    return _native.Yuv420Planes16(y, cb, cr, 2 * w if y_pitch is None else y_pitch, 2 * c_step * (w // 2) if c_pitch is None else c_pitch,
                                  frame, frame, c_step, depth, msb)


def clip(w, W=None, lq=None, mvs=A, par=A, f32=A, u8=A, out=None):
    W = w if W is None else W
    return _native.ClipYuv16(lq if lq is not None else planes(w), mvs, par, f32, u8, out if out is not None else planes(W))


def bad_planes(w):
    """every refusal the header lists for a descriptor of w-wide frames, as keyword overrides of planes(w)"""
    return [dict(depth=8), dict(depth=11), dict(depth=16), dict(depth=0), dict(msb=2), dict(msb=-1),            # unknown depth / container
            dict(y=A + 1), dict(cb=A + 0x100001, cr=A + 0x100003), dict(cr=A + 0x100001),                       # an odd pointer
            dict(y_pitch=2 * w + 1), dict(c_pitch=2 * w + 1), dict(frame=(1 << 22) + 1),                        # an odd pitch or stride
            dict(y=None), dict(cb=None), dict(cr=None),                                                         # a NULL plane
            dict(c_step=0), dict(c_step=3, c_pitch=8 * w), dict(c_step=-1),                                     # c_step 1 | 2
            dict(y_pitch=2 * w - 2), dict(c_pitch=2 * w - 2), dict(c_step=1, c_pitch=w - 2)]                    # a pitch below the row's bytes


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    h = _create(lib)
    side = (ctypes.c_float * 2)(73.0, 80.0)

    def call(clips, n=None, std=0, mask=7, hh=128, ww=128, t=1, g=h, ws=None, ws_bytes=0):
        arr = (_native.ClipYuv16 * max(len(clips), 1))(*clips)
        return lib.pnp_generator_forward_clips_yuv16(g, None, None, ctypes.cast(arr, ctypes.c_void_p) if clips else None,
                                                     len(clips) if n is None else n, std, mask, side, side, side, ws, ws_bytes, t, hh, ww, None)

    ok = clip(128)
    assert call([ok]) == WORKSPACE                                                  # everything in order up to the (null) workspace
    assert call([ok], std=4) == BAD_ARG and call([ok], std=-1) == BAD_ARG           # unknown standard
    assert call([ok], mask=0) == BAD_ARG and call([ok], mask=8) == BAD_ARG and call([ok], mask=-1) == BAD_ARG
    assert call([]) == BAD_ARG and call([ok], n=0) == BAD_ARG and call([ok], g=None) == BAD_ARG
    for bad in bad_planes(128):
        assert call([clip(128, lq=planes(128, **bad))]) == BAD_ARG, bad             # ... of the frames
        bad_out = clip(128, out=planes(128, **bad))                                 # ... or of the output, where the mask needs it
        for mask in (4, 5, 6, 7):
            assert call([bad_out], mask=mask) == BAD_ARG, (bad, mask)
        for mask in (1, 2, 3):
            assert call([bad_out], mask=mask) == WORKSPACE, (bad, mask)
    assert call([clip(128, mvs=None)]) == BAD_ARG and call([clip(128, par=None)]) == BAD_ARG
    assert call([clip(128, f32=None)], mask=1) == BAD_ARG and call([clip(128, f32=None)], mask=5) == BAD_ARG
    assert call([clip(128, f32=None)], mask=6) == WORKSPACE
    assert call([clip(128, u8=None)], mask=2) == BAD_ARG and call([clip(128, u8=None)], mask=5) == WORKSPACE
    assert call([ok, clip(128, mvs=None)]) == BAD_ARG                               # ... of every clip
    # any even address, any even pitch that holds a row, both chroma orders, planar; the output's depth and container are its own
    assert call([clip(128, lq=planes(128, y=A + 2, cb=A + 0x100006, cr=A + 0x100004, y_pitch=258, c_pitch=262))]) == WORKSPACE
    assert call([clip(128, lq=planes(128, c_step=1, cb=A + 0x100002, cr=A + 0x200006, c_pitch=130, depth=12, msb=0))]) == WORKSPACE
    assert call([clip(128, lq=planes(128, depth=10, msb=1), out=planes(128, depth=12, msb=0, c_step=1, cr=A + 0x300000))]) == WORKSPACE
    # odd h or w: BAD_ARG whatever else is wrong with the size; then the forward's own checks in their order
    assert call([ok], hh=127) == BAD_ARG and call([ok], ww=129) == BAD_ARG and call([ok], hh=63) == BAD_ARG
    assert call([clip(60)], hh=60, ww=60) == SIZE_ASSERT and call([clip(128)], hh=62) == SIZE_ASSERT
    assert call([clip(70)], hh=66, ww=70) == SIZE_VALUE and call([clip(128)], hh=66) == SIZE_VALUE
    assert call([clip(4096)], hh=4096, ww=4096) == UNSUPPORTED
    assert call([ok], t=0) == BAD_ARG
    assert lib.pnp_generator_set_any_size(h, 1) == 0
    assert call([clip(70)], hh=66, ww=70) == WORKSPACE and call([clip(70)], hh=65, ww=70) == BAD_ARG
    assert lib.pnp_generator_set_any_size(h, 0) == 0
    hv = _create(lib, vsr=1)                                                        # the x4 heads: the output planes hold 4h x 4w
    assert call([clip(128, W=512)], g=hv) == WORKSPACE and call([clip(128, W=128)], g=hv, mask=4) == BAD_ARG
    lib.pnp_generator_destroy(hv)
    # the workspace is sized by the 8-bit boundary's query: one byte less, or a misaligned address, is refused
    need = lib.pnp_generator_workspace_bytes_yuv(h, 1, 128, 128, 7)
    assert call([ok], ws=ctypes.c_void_p(A), ws_bytes=need - 1) == WORKSPACE and call([ok], ws=ctypes.c_void_p(A + 16), ws_bytes=need) == WORKSPACE
    lib.pnp_generator_destroy(h)


def test_the_converters_and_the_pack_launch_refuse_bad_arguments_before_any_hip_call(lib):
    p = planes(64)
    frm = lambda d, std=0, out=A, n=1, hh=64, ww=64: lib.pnp_frames_from_yuv420p16(ctypes.byref(d) if d is not None else None, std, out, n, hh, ww, None)      # noqa: E731
    to = lambda d, std=0, src=A, n=1, hh=64, ww=64: lib.pnp_frames_to_yuv420p16(src, ctypes.byref(d) if d is not None else None, std, n, hh, ww, None)      # noqa: E731
    pack = lambda d, std=0, out=A, n=1, hh=64, ww=64: lib.pnp_debug_pack_lr_yuv420p16(ctypes.byref(d) if d is not None else None, std, out, n, hh, ww, 0, None)      # noqa: E731
    for f in (frm, to, pack):
        assert f(None) == BAD_ARG and f(p, std=4) == BAD_ARG and f(p, n=0) == BAD_ARG and f(p, hh=63) == BAD_ARG and f(p, ww=66) == BAD_ARG
        assert f(p, ww=65) == BAD_ARG
        for bad in bad_planes(64):
            assert f(planes(64, **bad)) == BAD_ARG, bad
    assert frm(p, out=None) == BAD_ARG and to(p, src=None) == BAD_ARG and pack(p, out=None) == BAD_ARG


def test_the_plane_metrics_refuse_bad_arguments_before_any_hip_call(lib):
    p = planes(64)
    psnr = lambda a, b, out=A, n=1, hh=64, ww=64, crop=0: lib.pnp_psnr_sse_yuv420p16(      # noqa: E731
        ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None, out, n, hh, ww, crop, None)
    ssim = lambda a, b, out=A, n=1, hh=64, ww=64, crop=0, mask=7: lib.pnp_ssim_partials_yuv420p16(      # noqa: E731
        ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None, mask, out, n, hh, ww, crop, None)
    for f in (psnr, ssim):
        assert f(None, p) == BAD_ARG and f(p, None) == BAD_ARG and f(p, p, out=None) == BAD_ARG and f(p, p, n=0) == BAD_ARG
        assert f(p, p, hh=63) == BAD_ARG and f(p, p, ww=65) == BAD_ARG and f(p, p, crop=-2) == BAD_ARG and f(p, p, crop=3) == BAD_ARG
        assert f(p, p, crop=32) == BAD_ARG
        for bad in bad_planes(64):
            q = planes(64, **bad)
            assert f(q, p) == BAD_ARG and f(p, q) == BAD_ARG, bad
        # the two clips differ in depth: refused; in container, layout or pitch: each is described on its own (no refusal to test here
        # without a GPU -- the GPU suite runs those)
        assert f(planes(64, depth=10), planes(64, depth=12)) == BAD_ARG and f(planes(64, depth=12, msb=0), planes(64, depth=10, msb=0)) == BAD_ARG
    assert ssim(p, p, mask=0) == BAD_ARG and ssim(p, p, mask=8) == BAD_ARG
    assert ssim(p, p, hh=20, ww=64, mask=2) == BAD_ARG and ssim(planes(20), planes(20), hh=64, ww=20, mask=4) == BAD_ARG      # a chroma plane below 11x11


def test_the_entries_that_existed_return_what_they_returned(lib):
    h = _create(lib)
    side = (ctypes.c_float * 2)(73.0, 80.0)
    p8 = _native.Yuv420Planes(A + 1, A + 0x100003, A + 0x100002, 131, 129, 1 << 22, 1 << 22, 2)      # odd addresses and pitches: 8-bit planes may
    arr = (_native.ClipYuv * 1)(_native.ClipYuv(p8, A, A, A, A, p8))
    call = lambda mask, std=0: lib.pnp_generator_forward_clips_yuv(h, None, None, ctypes.cast(arr, ctypes.c_void_p), 1, std, mask, side, side, side,      # noqa: E731
                                                                   None, 0, 1, 128, 128, None)
    assert call(7) == WORKSPACE and call(8) == BAD_ARG and call(0) == BAD_ARG and call(7, std=4) == BAD_ARG
    assert lib.pnp_frames_from_yuv420(ctypes.byref(p8), 0, None, 1, 128, 128, None) == BAD_ARG
    io = (_native.ClipIO * 1)(_native.ClipIO(A, A, A, A, A))
    for fmt, mask in ((2, 1), (3, 1), (0, 4), (1, 4), (0, 7)):      # no new frame format and no new mask bit on the byte entry
        assert lib.pnp_generator_forward_clips(h, None, None, ctypes.cast(io, ctypes.c_void_p), 1, fmt, mask, side, side, side, None, 0, 1, 128, 128,
                                               None) == BAD_ARG
        assert lib.pnp_generator_workspace_bytes_io(h, 7, 128, 128, fmt, mask) == -1
    # the workspace query: the plain query plus exactly the staged fp32 frames, as tests/test_yuv_frames_host.py holds it
    al = lambda v: (v + 255) // 256 * 256      # noqa: E731
    plain = lib.pnp_generator_workspace_bytes(h, 7, 128, 128)
    for mask in range(1, 8):
        assert lib.pnp_generator_workspace_bytes_yuv(h, 7, 128, 128, mask) == plain + (al(128 * 128 * 12) if mask & 4 and not mask & 1 else 0)
    assert lib.pnp_generator_workspace_bytes_yuv(h, 7, 128, 128, 8) == -1
    assert lib.pnp_ssim_blocks_yuv420(64, 64, 0, 1) == lib.pnp_ssim_blocks(64, 64, 0) > 0
    assert lib.pnp_ssim_blocks_yuv420(64, 64, 4, 2) == lib.pnp_ssim_blocks_yuv420(64, 64, 4, 4) == lib.pnp_ssim_blocks(32, 32, 2) > 0
    assert lib.pnp_abi_version() == 5
    lib.pnp_generator_destroy(h)


def test_the_ctypes_structs_are_the_headers():
    with open(os.path.join(ROOT, 'include', 'pnpvcve.h')) as fh:
        hdr = fh.read()
    strip = lambda s: re.sub(r'/\*.*?\*/', '', s, flags=re.S)      # noqa: E731
    body = strip(hdr[hdr.index('typedef struct pnp_yuv420_planes16 {'):hdr.index('} pnp_yuv420_planes16;')])
    assert re.findall(r'(\w+)[,;]', body) == [f[0] for f in _native.Yuv420Planes16._fields_]
    body = strip(hdr[hdr.index('typedef struct pnp_clip_yuv16 {'):hdr.index('} pnp_clip_yuv16;')])
    assert re.findall(r'(\w+)[,;]', body) == [f[0] for f in _native.ClipYuv16._fields_]
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_native.Yuv420Planes16) == 3 * P + 4 * 8 + 16              # three pointers, four int64, three ints and their padding
    assert ctypes.sizeof(_native.ClipYuv16) == 2 * ctypes.sizeof(_native.Yuv420Planes16) + 4 * P
    assert ctypes.sizeof(_native.Yuv420Planes) == 3 * P + 4 * 8 + 8                 # the 8-bit struct is what it was
    assert 'not offered' in hdr and '10 bit, 4:2:2' not in hdr
    import yuv16_ref
    from pnp_vcve_amd import ops
    assert ops.YUV16_LAYOUTS == yuv16_ref.LAYOUTS


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('yuv16') / 'yuv16_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'yuv16_stub.cpp'), '-o', exe]
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
    assert len(out) == 7
    for name, d in out.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
    return out


def test_the_launch_list_is_the_8_bit_yuv_boundarys_apart_from_the_three_dispatch_sites(docs):
    """the stub's own range checks (planes at even addresses with ragged pitches behind poisoned bytes; every output sample written
    exactly once) are in `errors`, asserted empty by the fixture; here: the trace and the launch counts"""
    for name, d in docs.items():
        assert d['same'] == 1 and d['records'] > 80, (name, d['first_diff'])
        assert d['n8'] == 0, name                                              # no 8-bit launcher ran for a 16-bit clip
        assert d['n_pack'] == (2 if name.startswith('two_clips') else 1), name
        mask = int(name.rsplit('mask', 1)[1])
        assert d['n_to'] == (d['frames'] if mask & 4 else 0), name
        assert d['n_from'] == (d['frames'] if d['staged'] else 0), name
        assert d['ctx_bytes'] == d['ctx_bytes_8bit_run'], name
    assert docs['two_clips_p010_mask7']['streams_used'] == [1, 2]
    assert docs['f16_p010_mask6']['staged'] == 1 and docs['plain_p010_mask7']['staged'] == 0
    assert docs['aligned_p010_mask5']['n_pack_fast'] == 1 and docs['plain_p010_mask7']['n_pack_fast'] == 0
