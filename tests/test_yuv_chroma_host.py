"""CPU: PNP_YUV_CODE(standard, chroma) at the C ABI (include/pnpvcve.h, "Chroma modes"): the chroma mode travels in bits 8..11 of the
integer every 4:2:0 entry takes as yuv_standard.  Through ctypes on the built library with null device buffers, as
tests/test_yuv_frames_host.py: every code below is decided on the host, before any HIP call."""
import ctypes
import os
import re

import pytest

from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE = 1001, 1003
A = 0x1000        # an aligned "device address": never dereferenced on these paths
BAD_CODES = [m << 8 for m in range(4, 16)] + [s | m << 8 for s in (1, 2) for m in (4, 9, 15)] + [
    1 << 16, 1 << 16 | 2 << 8 | 1, 1 << 20, 1 << 30, 4, 5, 255, 4 | 2 << 8, 0x80 | 1 << 8, -1, -256, -(1 << 31)]


def code(standard, chroma):
    return standard | chroma << 8


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


@pytest.fixture(scope='module')
def gen(lib):
    h = ctypes.c_void_p()
    cfg = _native.GeneratorCfg(mid_channels=64, num_blocks=2, num_experts=6, with_cat=1, use_base_qp=1, expert_softmax=1, with_bias=1, with_se=1,
                               one_layer=1, channel_first=1, align_key=1, vsr=0, deform=0)
    assert lib.pnp_generator_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    yield h
    lib.pnp_generator_destroy(h)


def planes8(w):
    return _native.Yuv420Planes(A, A + 0x100000, A + 0x100001, w, w, 1 << 22, 1 << 22, 2)


def planes16(w, depth=10, msb=1):
    return _native.Yuv420Planes16(A, A + 0x100000, A + 0x100002, 2 * w, 2 * w, 1 << 22, 1 << 22, 2, depth, msb)


def forwards(lib, gen):
    """-> the two forwards as f(std, mask=7) on one 128 x 128 frame with a null workspace"""
    side = (ctypes.c_float * 2)(73.0, 80.0)
    out = []
    for entry, Clip, mk in ((lib.pnp_generator_forward_clips_yuv, _native.ClipYuv, planes8),
                            (lib.pnp_generator_forward_clips_yuv16, _native.ClipYuv16, planes16)):
        arr = (Clip * 1)(Clip(mk(128), A, A, A, A, mk(128)))
        out.append(lambda std, mask=7, entry=entry, arr=arr: entry(gen, None, None, ctypes.cast(arr, ctypes.c_void_p), 1, std, mask, side, side, side,
                                                                    None, 0, 1, 128, 128, None))
    return out


def test_every_standard_with_every_chroma_mode_gets_as_far_as_the_workspace(lib, gen):
    """(on the commit before the chroma modes 0x100 was an unknown standard: this is the test that fails there)"""
    for fwd in forwards(lib, gen):
        for s in range(4):
            for m in range(4):
                for mask in (1, 4, 7):
                    assert fwd(code(s, m), mask) == WORKSPACE, (s, m, mask)


def test_every_other_code_is_a_bad_argument_at_every_entry(lib, gen):
    for fwd in forwards(lib, gen):
        for c in BAD_CODES:
            assert fwd(c) == BAD_ARG, hex(c)
    p8, p16 = planes8(64), planes16(64)
    entries = [lambda c: lib.pnp_frames_from_yuv420(ctypes.byref(p8), c, A, 1, 64, 64, None),
               lambda c: lib.pnp_frames_to_yuv420(A, ctypes.byref(p8), c, 1, 64, 64, None),
               lambda c: lib.pnp_debug_pack_lr_yuv420(ctypes.byref(p8), c, A, 1, 64, 64, 0, None),
               lambda c: lib.pnp_frames_from_yuv420p16(ctypes.byref(p16), c, A, 1, 64, 64, None),
               lambda c: lib.pnp_frames_to_yuv420p16(A, ctypes.byref(p16), c, 1, 64, 64, None),
               lambda c: lib.pnp_debug_pack_lr_yuv420p16(ctypes.byref(p16), c, A, 1, 64, 64, 1, None)]
    for i, f in enumerate(entries):
        for c in BAD_CODES:
            assert f(c) == BAD_ARG, (i, hex(c))
    # a good code does not mend a bad frame or descriptor (refused before any launch)
    for c in (code(0, 2), code(3, 3)):
        assert lib.pnp_frames_from_yuv420(ctypes.byref(p8), c, A, 1, 63, 64, None) == BAD_ARG
        assert lib.pnp_frames_to_yuv420(None, ctypes.byref(p8), c, 1, 64, 64, None) == BAD_ARG
        assert lib.pnp_debug_pack_lr_yuv420p16(ctypes.byref(planes16(64, depth=9)), c, A, 1, 64, 64, 0, None) == BAD_ARG


def test_no_export_was_added_and_the_workspace_query_is_what_it_was(lib, gen):
    assert lib.pnp_abi_version() == 5
    plain = lib.pnp_generator_workspace_bytes(gen, 7, 128, 128)
    assert plain > 0
    out1 = (128 * 128 * 12 + 255) // 256 * 256
    for mask in range(1, 8):        # (the default precision and last conv: nothing staged on the way in; tests/test_yuv_frames_host.py)
        assert lib.pnp_generator_workspace_bytes_yuv(gen, 7, 128, 128, mask) == plain + (out1 if mask & 4 and not mask & 1 else 0), mask
    for mask in (0, 8, -1, 0x100, 0x207):       # the query takes a mask, never a code
        assert lib.pnp_generator_workspace_bytes_yuv(gen, 7, 128, 128, mask) == -1


def test_the_macros_are_the_headers_and_pythons_names():
    with open(os.path.join(ROOT, 'include', 'pnpvcve.h')) as fh:
        hdr = fh.read()
    for name, val in (('REPLICATE', 0), ('CENTER', 1), ('LEFT', 2), ('TOPLEFT', 3)):
        assert int(re.search(r'#define PNP_YUV_CHROMA_%s (\d+)' % name, hdr).group(1)) == val
        assert _native.YUV_CHROMA[name.lower()] == val
    assert re.search(r'#define PNP_YUV_CODE\(standard, chroma\) \(\(standard\) \| \(\(chroma\) << 8\)\)', hdr)
    import yuv_chroma_ref
    assert list(yuv_chroma_ref.MODES) == sorted(_native.YUV_CHROMA, key=_native.YUV_CHROMA.get)


def test_the_python_helper_builds_the_code_and_keeps_bare_integers_0_to_3():
    """ops._yuv_code; importing ops needs torch only, nothing here touches a device"""
    from pnp_vcve_amd import ops
    assert ops.YUV_CHROMA == ('replicate', 'center', 'left', 'topleft')
    for s, name in enumerate(('bt601-limited', 'bt601-full', 'bt709-limited', 'bt709-full')):
        assert ops._yuv_code(name) == ops._yuv_code(s) == ops._yuv_standard(name) == s
        for m, chroma in enumerate(ops.YUV_CHROMA):
            assert ops._yuv_code(name, chroma) == ops._yuv_code(s, chroma) == code(s, m)
            assert ops._yuv_code_split(code(s, m)) == (s, chroma)
    for bad in (4, -1, 0x100, 0x203, 'bt2020'):
        with pytest.raises(ValueError, match='yuv_standard'):
            ops._yuv_code(bad, 'left')
    for bad in ('Left', 'top-left', 2, None, ''):
        with pytest.raises(ValueError, match='chroma'):
            ops._yuv_code(0, bad)
    for bad in (0x400, -1, 0x104):
        with pytest.raises(ValueError):
            ops._yuv_code_split(bad)
