"""CPU: the C-ABI library builds/loads and exports every symbol include/pnpvcve.h declares;
host-side schema logic (no GPU compute)."""
import os
import re
import sys

import pytest
import torch

from pnp_vcve_amd import _native, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def _declared(header):
    hdr = open(os.path.join(ROOT, 'include', header)).read()
    return set(re.findall(r'\b(pnp_[a-z0-9_]+)\s*\(', hdr))


def test_every_declared_symbol_is_exported(lib):
    declared = _declared('pnpvcve.h')
    assert declared, 'no declarations found'
    assert declared == set(_native.SIGNATURES), declared ^ set(_native.SIGNATURES)
    debug = _declared('pnpvcve_debug.h')
    assert debug == set(_native.DEBUG_SIGNATURES), debug ^ set(_native.DEBUG_SIGNATURES)
    for name in declared | debug:
        assert hasattr(lib, name), name
    assert lib.pnp_abi_version() == 5


def test_no_undeclared_pnp_symbol_is_exported(lib):
    """Everything the .so exports under the pnp_ prefix is declared in include/*.h (no hidden global switches)."""
    import subprocess
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm'
    out = subprocess.check_output([nm if os.path.exists(nm) else 'nm', '-D', '--defined-only', _native.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('pnp_')}
    declared = _declared('pnpvcve.h') | _declared('pnpvcve_debug.h')
    assert exported, 'no pnp_* exports found'
    assert exported <= declared, sorted(exported - declared)


def test_schema_equals_reference_state_dict():
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as Gen
    for over in ({}, dict(vsr=True), dict(with_cat=False), dict(one_layer=False), dict(with_se=False),
                 dict(deform='basic'), dict(deform='fvc'),
                 dict(with_bias=False, with_se=False, num_experts=4, num_blocks=3)):
        cfg = dict(syn.DEFAULT_GENERATOR_CFG)
        cfg.update(over)
        m = Gen(**cfg)
        sd = m.state_dict()
        sch = syn.state_dict_schema(cfg)
        assert set(sd) == set(sch), (over, set(sd) ^ set(sch))
        for k, shp in sch.items():
            assert tuple(sd[k].shape) == tuple(shp), k
    m = Gen(**syn.DEFAULT_GENERATOR_CFG)
    assert sum(p.numel() for p in m.parameters()) == 4559885


def test_constructor_errors_like_reference():
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as Gen
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    with pytest.raises(TypeError):
        Gen(**dict(cfg, deform='nope'))
    with pytest.raises(TypeError):
        Gen(**dict(cfg, deform='stdf'))
    with pytest.raises(AssertionError):
        Gen(**dict(cfg, use_base_qp=False))      # with_bias requires use_base_qp (iconvsr_ipb_par.py:27)


def test_no_cpu_fallback():
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as Gen
    m = Gen(**syn.DEFAULT_GENERATOR_CFG)
    z = torch.zeros(1, 2, 3, 64, 64)
    s = torch.zeros(1, 2, 1, 1, 1)
    with pytest.raises(RuntimeError):
        m(z, s, s, torch.zeros(1, 2, 4, 64, 64), s, z)


def test_c_abi_error_codes_without_a_gpu(lib):
    """pnp_generator_create / set_precision validate on the host: PNP_ERR_UNSUPPORTED 1002, PNP_ERR_BAD_ARG 1001."""
    import ctypes

    def create(**over):
        kw = dict(mid_channels=64, num_blocks=2, num_experts=6, with_cat=1, use_base_qp=1, expert_softmax=1, with_bias=1,
                  with_se=1, one_layer=1, channel_first=1, align_key=1, vsr=0, deform=0)
        kw.update(over)
        h = ctypes.c_void_p()
        rc = lib.pnp_generator_create(ctypes.byref(_native.GeneratorCfg(**kw)), ctypes.byref(h))
        return rc, h

    assert create(mid_channels=32)[0] == 1002
    assert create(num_experts=0)[0] == 1001
    assert create(num_blocks=0)[0] == 1001
    assert create(with_bias=0, with_se=1)[0] == 1001
    assert create(with_bias=1, use_base_qp=0)[0] == 1001
    assert create(deform=3)[0] == 1001
    # r04 (ABI 4): num_group / flow_inter / blocktype
    assert create(num_group=3)[0] == 1001 and create(num_group=128)[0] == 1001      # nn.Conv2d: channels % groups
    assert create(flow_inter=2)[0] == 1001 and create(blocktype=2)[0] == 1001
    assert create(blocktype=1, one_layer=0)[0] == 1002        # 'drt_woqp' with Dynamic_conv2d_se convs: the reference raises too
    assert create(sparse_val=1, num_group=2)[0] == 1002       # ... and so does its sparse_conv on grouped 1x1 weights
    rc, hg = create(num_group=4, blocktype=1, flow_inter=1)
    assert rc == 0
    lib.pnp_generator_param_name.restype = ctypes.c_char_p
    shapes = {}
    for i in range(lib.pnp_generator_num_params(hg)):
        nm = lib.pnp_generator_param_name(hg, i).decode()
        shapes[nm] = tuple(int(lib.pnp_generator_param_dim(hg, i, d)) for d in range(lib.pnp_generator_param_ndim(hg, i)))
    assert shapes['forward_resblocks.main.1.conv2.weight'] == (64, 16, 3, 3)       # a plain conv, grouped
    assert shapes['forward_resblocks.main.1.conv2.bias'] == (64,)
    assert shapes['backward_resblocks.main.0.conv1.weight'] == (64, 16, 3, 3)
    assert shapes['backward_resblocks.main.0.conv16x8.weight'] == (64, 16, 1, 1)
    from pnp_vcve_amd import synthetic
    assert shapes == {k: tuple(v) for k, v in synthetic.state_dict_schema(dict(num_blocks=2, num_group=4, blocktype='drt_woqp')).items()}
    lib.pnp_generator_destroy(hg)
    rc, h = create()            # (num_group left 0 = the reference's default 1)
    assert rc == 0 and h.value
    n32 = lib.pnp_generator_packed_floats(h)
    ctx = lib.pnp_generator_workspace_bytes(h, 7, 128, 128)
    assert lib.pnp_generator_get_precision(h) == 0
    assert lib.pnp_generator_set_precision(h, 7) == 1001
    assert lib.pnp_generator_set_precision(h, 1) == 0 and lib.pnp_generator_get_precision(h) == 1
    assert lib.pnp_generator_packed_floats(h) == n32 + n32 // 2          # fp16 mirror of every image
    assert lib.pnp_generator_workspace_bytes(h, 7, 128, 128) > ctx       # + mirror of the mixed experts
    for opt in range(10):                                                # per-handle switches, default on (the chain mirrors off)
        assert lib.pnp_generator_get_option(h, opt) == (0 if opt == 7 else 1)
    assert lib.pnp_generator_set_option(h, 3, 0) == 0 and lib.pnp_generator_get_option(h, 3) == 0
    # r05 (ABI 5): PNP_OPT_WINOGRAD, default off, three-valued (off / large frames / every frame size)
    assert lib.pnp_generator_get_option(h, 9) == 1
    assert lib.pnp_generator_set_option(h, 9, 2) == 0 and lib.pnp_generator_get_option(h, 9) == 2
    assert lib.pnp_generator_set_option(h, 9, 7) == 0 and lib.pnp_generator_get_option(h, 9) == 2          # clamped
    assert lib.pnp_generator_set_option(h, 9, 1) == 0 and lib.pnp_generator_get_option(h, 9) == 1
    assert lib.pnp_generator_set_option(h, 10, 0) == 1001 and lib.pnp_generator_get_option(h, 10) == -1
    assert lib.pnp_wino_image_floats() == 65536 and lib.pnp_wino_par_image_floats() == 12288
    assert n32 % 4096 == 0 and ctx % 256 == 0
    lib.pnp_generator_destroy(h)


def test_forward_refuses_maps_beyond_32_bit_offsets_before_touching_memory(lib):
    """Feature maps are addressed with 32-bit byte offsets: a frame whose largest map reaches 4 GiB is PNP_ERR_UNSUPPORTED
    (1002), decided on the host before any launch (so this runs without a GPU, with null buffers)."""
    import ctypes
    kw = dict(mid_channels=64, num_blocks=1, num_experts=2, with_cat=1, use_base_qp=1, expert_softmax=1, with_bias=1,
              with_se=1, one_layer=1, channel_first=1, align_key=1, vsr=0, deform=0)
    # deform != 0: the 448-channel offset/mask map (1792 B/pixel) is the widest one -> 1440p is already too large
    for vsr, hw, rc_exp, deform in ((0, (4096, 4096), 1002, 0), (1, (1024, 1024), 1002, 0), (0, (60, 64), 1004, 0),
                                    (0, (66, 64), 1005, 0), (0, (1440, 2560), 1002, 1), (0, (1440, 2560), 1002, 2),
                                    (0, (1440, 2560), 1003, 0), (0, (1080, 1920), 1003, 1), (1, (720, 1280), 1003, 0)):
        kw['vsr'] = vsr
        kw['deform'] = deform
        h = ctypes.c_void_p()
        assert lib.pnp_generator_create(ctypes.byref(_native.GeneratorCfg(**kw)), ctypes.byref(h)) == 0
        side = (ctypes.c_float * 1)(73.0)
        rc = lib.pnp_generator_forward(h, None, None, None, None, None, side, side, side, None, None, 0, 1, 1, hw[0], hw[1],
                                       None)
        assert rc == rc_exp, (vsr, hw, deform, rc)      # 1003: passed the guard, stopped at the (null) workspace
        lib.pnp_generator_destroy(h)


def test_dcn_and_split_conv_are_built_without_slp_vectorisation():
    """DESIGN.md 3.5 / profiles/r03_dcn_hazard_report.txt: every build of dcn.hip whose gather arithmetic hipcc's SLP vectoriser had
    packed gave run-to-run varying samples in the fp16 instantiation under some timing; the flag is part of the kernel's
    correctness, so dropping it has to fail a test (the behaviour itself is held by the -m gpu determinism tests).  Same for
    conv_f16x3.hip since r04 (DESIGN.md 3.6 finding 5: the general partition re-split)."""
    from pnp_vcve_amd import build_native
    assert '-fno-slp-vectorize' in build_native.EXTRA_FLAGS.get('dcn.hip', [])
    assert '-fno-slp-vectorize' in build_native.EXTRA_FLAGS.get('conv_f16x3.hip', [])
    assert all(src in build_native.SOURCES for src in build_native.EXTRA_FLAGS)


def test_op_level_convs_refuse_maps_beyond_32_bit_offsets_before_touching_memory(lib):
    """pnp_conv3x3_f32 / _f16 / _f16x3: an NHWC64 fp32 map of 4096 x 4096 pixels is exactly 4 GiB -> PNP_ERR_UNSUPPORTED (1002) on the
    host, before any pointer is dereferenced on the device (runs without a GPU; the pointers are fakes)."""
    import ctypes
    fake = 0x1000
    srcs = (ctypes.c_void_p * 1)(fake)
    chans = (ctypes.c_int * 1)(64)
    w = (ctypes.c_void_p * 1)(fake)
    for hw, rc_exp in (((4096, 4096), 1002), ((0, 64), 1002)):
        assert lib.pnp_conv3x3_f32(1, srcs, chans, w, None, None, None, None, None, 0, fake, hw[0], hw[1], None) == rc_exp
        assert lib.pnp_conv3x3_f16(1, srcs, chans, w, None, None, None, None, None, 0, fake, hw[0], hw[1], None) == rc_exp
        assert lib.pnp_conv3x3_f16x3(1, srcs, chans, w, w, None, None, None, None, None, None, 0, fake, hw[0], hw[1], None) == rc_exp
    assert lib.pnp_conv3x3_f16x3(0, srcs, chans, w, w, None, None, None, None, None, None, 0, fake, 64, 64, None) == 1001


def test_warp_entries_refuse_bad_sizes_before_touching_memory(lib):
    """every pixel-major warp entry: h < 1, w < 1, c < 4, c % 4 != 0 and a mode other than 0 / 1 are PNP_ERR_BAD_ARG (1001), decided
    on the host before any launch (runs without a GPU; the pointers are fakes)"""
    fake = 0x1000
    entries = {'f32': lambda h, w, c, mode: lib.pnp_mv_warp_nhwc_f32(fake, fake, fake, fake, h, w, c, None),
               'mode_f32': lambda h, w, c, mode: lib.pnp_mv_warp_nhwc_mode_f32(fake, fake, fake, fake, h, w, c, mode, None),
               'f16out': lambda h, w, c, mode: lib.pnp_mv_warp_nhwc_f16out(fake, fake, fake, fake, h, w, c, None),
               'f16out_mode': lambda h, w, c, mode: lib.pnp_mv_warp_nhwc_f16out_mode(fake, fake, fake, fake, h, w, c, mode, None)}
    for name, call in entries.items():
        for h, w, c in ((0, 8, 64), (-1, 8, 64), (8, 0, 64), (8, -3, 8), (8, 8, 0), (8, 8, 3), (8, 8, -4), (8, 8, 6), (8, 8, 66),
                        (0, 0, 0)):
            assert call(h, w, c, 0) == 1001, (name, h, w, c)
        if 'mode' in name:
            assert call(8, 8, 64, 2) == 1001 and call(8, 8, 8, -1) == 1001, name


def test_head_debug_entries_refuse_bad_arguments_and_ineligible_routes_before_touching_memory(lib):
    """pnp_debug_pixel_shuffle_conv / pnp_debug_conv_last / pnp_debug_pack_conv_last (include/pnpvcve_debug.h): NULL pointers, an act
    outside 0..2, h or w below 1, an out_mode other than 2 / 3 and unknown routes are PNP_ERR_BAD_ARG (1001); a map beyond 32-bit
    byte offsets and a route the project's eligibility rules do not select for the arguments are PNP_ERR_UNSUPPORTED (1002): all
    decided on the host before any launch (runs without a GPU; the pointers are fakes)."""
    fake = 0x1000
    AUTO, F32, F16, F16X3, VALU = (_native.HEAD_ROUTES[k] for k in ('auto', 'f32', 'f16', 'f16x3', 'valu'))

    def shuffle(x=fake, x16=0, packed=fake, twin=None, kind=0, act=2, out=fake, o16=0, h=8, w=8, route=F32, queue=None):
        return lib.pnp_debug_pixel_shuffle_conv(x, x16, packed, twin, kind, act, out, o16, h, w, route, queue, None)

    for kw in (dict(x=None), dict(packed=None), dict(out=None), dict(act=-1), dict(act=3), dict(h=0), dict(w=0), dict(h=-4), dict(route=VALU),
               dict(route=7), dict(route=-1), dict(kind=3, twin=fake), dict(kind=1), dict(kind=0, twin=fake), dict(kind=2, twin=None)):
        assert shuffle(**kw) == 1001, kw
    # the (2h, 2w, 64) fp32 map of a 2048 x 2048 input is exactly 4 GiB
    assert shuffle(h=2048, w=2048) == 1002 and shuffle(h=2048, w=2048, route=AUTO) == 1002
    for kw in (dict(route=F16), dict(route=F16X3),                                   # no twin to read
               dict(route=F16, twin=fake, kind=2), dict(route=F16X3, twin=fake, kind=1),     # the other kernel's twin
               dict(route=F32, x16=1), dict(route=F32, o16=1),                       # fp16 maps exist on the fp16 kernel only
               dict(route=F16X3, twin=fake, kind=2, x16=1), dict(route=F16X3, twin=fake, kind=2, o16=1),
               dict(route=AUTO, x16=1), dict(route=AUTO, twin=fake, kind=2, o16=1)):
        assert shuffle(**kw) == 1002, kw

    def last(src=fake, s16=0, packed=fake, prec=0, act=0, mode=2, frame=fake, form=0, out=fake, out8=None, H=8, W=16, route=VALU):
        return lib.pnp_debug_conv_last(src, s16, packed, prec, act, mode, frame, form, out, out8, H, W, route, None)

    for kw in (dict(src=None), dict(packed=None), dict(frame=None), dict(out=None), dict(act=-1), dict(act=3), dict(H=0), dict(W=0), dict(W=-16),
               dict(mode=0), dict(mode=1), dict(mode=4), dict(form=3), dict(form=-1), dict(route=F16X3), dict(route=9), dict(prec=3),
               dict(mode=3, H=10), dict(mode=3, W=18)):
        assert last(**kw) == 1001, kw
    assert last(H=4096, W=4096) == 1002 and last(H=4096, W=4096, route=AUTO) == 1002      # the NHWC64 fp32 source map is exactly 4 GiB
    for kw in (dict(route=VALU, s16=1), dict(route=VALU, s16=1, form=1), dict(route=VALU, s16=1, out8=fake),      # conv_last_valu_shape
               dict(route=F32, form=1), dict(route=F32, form=2), dict(route=F32, out8=fake), dict(route=F32, s16=1),
               dict(route=F16, form=1), dict(route=F16, form=2), dict(route=F16, out8=fake),
               dict(route=AUTO, prec=1, form=1), dict(route=AUTO, prec=1, out8=fake),     # the fp16 path stages bytes around its fp32 interface
               dict(route=AUTO, prec=0, s16=1), dict(route=AUTO, prec=2, s16=1), dict(route=AUTO, prec=0, s16=1, form=2)):
        assert last(**kw) == 1002, kw
    assert lib.pnp_debug_pack_conv_last(None, fake, fake, None) == 1001
    assert lib.pnp_debug_pack_conv_last(fake, None, fake, None) == 1001
    assert lib.pnp_debug_pack_conv_last(fake, fake, None, None) == 1001
    # image (9 chunks of 2048) + bias (32) + vector-ALU layout (9 * 64 * 4) + the image's fp16 twin (half the floats)
    assert lib.pnp_debug_conv_last_packed_floats() == 9 * 2048 + 32 + 2304 + 9 * 1024


def test_graft_entry_build_runs_and_agrees_with_the_header_on_the_abi_version():
    """__graft_entry__.build() is the driver's "does it build" check: it must pass on a CPU box (hipcc cross-compiles) and its ABI
    assertion must follow include/pnpvcve.h (r04: the header went to 4 while build() still asserted 3)."""
    import importlib
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    ge = importlib.import_module('__graft_entry__')
    ge.build()
    with open(os.path.join(root, 'include', 'pnpvcve.h')) as fh:
        declared = int(re.search(r'pnp_abi_version\(void\); /\* (\d+):', fh.read()).group(1))
    assert _native.lib().pnp_abi_version() == declared
