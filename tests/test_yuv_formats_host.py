"""CPU: the chroma formats at the C ABI and in Python (include/pnpvcve.h, "Chroma formats"): PNP_YUV_CODE3(standard, chroma, format)
carries the format in bits 12..13 of the integer every Y'CbCr entry takes as yuv_standard.  Through ctypes on the built library with
fake device addresses, as tests/test_yuv_chroma_host.py: every code below is decided on the host, before any HIP call.  The descriptor
predicates and the chroma plane sources run in a stand-alone host program under AddressSanitizer (tests/host/yuv_formats_desc.cpp)."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import test_yuv_chroma_host as ch
from pnp_vcve_amd import _native, ops

ROOT = ch.ROOT
BAD_ARG, WORKSPACE, A = ch.BAD_ARG, ch.WORKSPACE, ch.A
lib, gen = ch.lib, ch.gen          # (module-scoped fixtures)


def code3(standard, chroma, fmt):
    return standard | chroma << 8 | fmt << 12


def planes8(w, step=2, c_pitch=None):
    return _native.Yuv420Planes(A, A + 0x100000, A + 0x100001 if step == 2 else A + 0x200000, w, 2 * w if c_pitch is None else c_pitch, 1 << 22, 1 << 22, step)


def planes16(w, step=2, c_pitch=None, depth=10, msb=1):
    return _native.Yuv420Planes16(A, A + 0x100000, A + 0x100002 if step == 2 else A + 0x200000, 2 * w, 4 * w if c_pitch is None else c_pitch, 1 << 22, 1 << 22,
                                  step, depth, msb)


def forwards(lib, gen, h=128, w=128, mk8=planes8, mk16=planes16):
    """-> the two forwards as f(std, mask=7) on one h x w frame with a null workspace; the chroma pitches hold a 4:4:4 row of pairs.
    A forward that finds nothing wrong with its arguments ends at the workspace check: no entry is ever called here with arguments it
    would accept AND a fake address it would hand to a kernel."""
    side = (ctypes.c_float * 2)(73.0, 80.0)
    out = []
    for entry, Clip, mk in ((lib.pnp_generator_forward_clips_yuv, _native.ClipYuv, mk8), (lib.pnp_generator_forward_clips_yuv16, _native.ClipYuv16, mk16)):
        arr = (Clip * 1)(Clip(mk(w), A, A, A, A, mk(w)))
        out.append(lambda std, mask=7, entry=entry, arr=arr: entry(gen, None, None, ctypes.cast(arr, ctypes.c_void_p), 1, std, mask, side, side, side,
                                                                    None, 0, 1, h, w, None))
    return out


def conversions(lib, p8, p16, h, w):
    return [lambda c: lib.pnp_frames_from_yuv420(ctypes.byref(p8), c, A, 1, h, w, None),
            lambda c: lib.pnp_frames_to_yuv420(A, ctypes.byref(p8), c, 1, h, w, None),
            lambda c: lib.pnp_frames_from_yuv420p16(ctypes.byref(p16), c, A, 1, h, w, None),
            lambda c: lib.pnp_frames_to_yuv420p16(A, ctypes.byref(p16), c, 1, h, w, None)]


def packs(lib, p8, p16, h, w):
    return [lambda c: lib.pnp_debug_pack_lr_yuv420(ctypes.byref(p8), c, A, 1, h, w, 0, None),
            lambda c: lib.pnp_debug_pack_lr_yuv420p16(ctypes.byref(p16), c, A, 1, h, w, 1, None)]


def test_every_standard_mode_and_new_format_gets_as_far_as_the_workspace(lib, gen):
    """(on the commit before the chroma formats bit 12 was refused with PNP_ERR_BAD_ARG: this is the test that fails there)"""
    for fwd in forwards(lib, gen):
        for f in (1, 2):
            for s in range(4):
                for m in range(4):
                    for mask in (1, 4, 7):
                        assert fwd(code3(s, m, f), mask) == WORKSPACE, (s, m, f, mask)


def test_format_3_and_bits_from_14_up_are_bad_arguments_at_every_entry(lib, gen):
    bad = [code3(0, 0, 3), code3(2, 1, 3), 1 << 14, 1 << 14 | code3(1, 2, 1), 1 << 15 | code3(0, 0, 2), 1 << 16 | code3(0, 0, 1), 1 << 30 | 1 << 12,
           -(1 << 31) | 1 << 12]
    p8, p16 = planes8(64), planes16(64)
    entries = forwards(lib, gen) + conversions(lib, p8, p16, 64, 64) + packs(lib, p8, p16, 64, 64)
    for i, f in enumerate(entries):
        for c in bad:
            assert f(c) == BAD_ARG, (i, hex(c))
    # every refusal of the 4:2:0 codes is still a refusal with a format beside it
    for i, f in enumerate(entries):
        for c in ch.BAD_CODES:
            for fmt in (1, 2):
                assert f(c | fmt << 12) == BAD_ARG, (i, hex(c), fmt)


def test_the_descriptor_checks_know_the_chroma_planes_size(lib, gen):
    w = 128
    for step in (1, 2):
        # 4:4:4: a chroma row holds c_step * w samples; 4:2:2 and 4:2:0: c_step * w / 2.  One sample short is refused by the
        # conversions, the pack and the forwards; the exact row is accepted (asked of the forwards, which then stop at the workspace)
        for fmt, need in ((0, step * w // 2), (1, step * w // 2), (2, step * w)):
            short8, short16 = planes8(w, step, need - 1), planes16(w, step, 2 * need - 2)
            for i, f in enumerate(conversions(lib, short8, short16, 128, w) + packs(lib, short8, short16, 128, w)):
                assert f(code3(0, 0, fmt)) == BAD_ARG, (step, fmt, i)
            for pitch, want in ((need - 1, BAD_ARG), (need, WORKSPACE)):
                for fwd in forwards(lib, gen, 128, w, lambda ww: planes8(ww, step, pitch), lambda ww: planes16(ww, step, 2 * pitch)):
                    assert fwd(code3(0, 0, fmt)) == want, (step, fmt, pitch)
    # the parity rules: 4:2:2 needs an even w only, 4:4:4 none; 4:2:0 keeps both.  (A conversion that accepts its arguments launches a
    # kernel on its addresses: only refusals are asked of the conversions here; what they accept -- 4:2:2 with an odd h, 4:4:4 with odd
    # h and w -- is asked of the forwards below and run on real planes by tests/test_gpu_yuv_formats.py at 1 x 2, 5 x 2, 1 x 1, 5 x 1.)
    p8, p16 = planes8(65), planes16(65)
    for i, f in enumerate(conversions(lib, p8, p16, 64, 65) + packs(lib, p8, p16, 64, 65)):
        assert f(code3(0, 0, 1)) == BAD_ARG and f(code3(0, 0, 0)) == BAD_ARG, i
    for i, f in enumerate(conversions(lib, p8, p16, 63, 64) + packs(lib, p8, p16, 63, 64)):
        assert f(code3(0, 0, 0)) == BAD_ARG, i
    for fwd in forwards(lib, gen, 128, 129):
        assert fwd(code3(0, 0, 1)) == BAD_ARG and fwd(code3(0, 0, 0)) == BAD_ARG
    for fwd in forwards(lib, gen, 129, 128):
        assert fwd(code3(0, 0, 0)) == BAD_ARG
    # a null plane, a null output: refused whatever the format
    for fmt in (1, 2):
        assert lib.pnp_frames_to_yuv420(None, ctypes.byref(planes8(64)), code3(0, 2, fmt), 1, 64, 64, None) == BAD_ARG
        assert lib.pnp_frames_from_yuv420(ctypes.byref(planes8(64)), code3(0, 2, fmt), None, 1, 64, 64, None) == BAD_ARG
        assert lib.pnp_debug_pack_lr_yuv420p16(ctypes.byref(planes16(64, depth=9)), code3(0, 0, fmt), A, 1, 64, 64, 0, None) == BAD_ARG


def test_odd_sizes_the_formats_admit_reach_the_forwards_size_rules(lib, gen):
    """4:2:2 with an odd h and 4:4:4 with odd h and w pass the boundary's own checks: the forward then answers with ITS size rule (a
    frame that is no multiple of 4 without any_size: PNP_ERR_SIZE_VALUE = 1005), not with PNP_ERR_BAD_ARG"""
    for fwd in forwards(lib, gen, 129, 128):
        assert fwd(code3(0, 0, 1)) == 1005 and fwd(code3(0, 0, 2)) == 1005
    for fwd in forwards(lib, gen, 129, 131):
        assert fwd(code3(0, 0, 2)) == 1005 and fwd(code3(0, 0, 1)) == BAD_ARG
    assert lib.pnp_generator_set_any_size(gen, 1) == 0
    try:
        for fwd in forwards(lib, gen, 129, 128):
            assert fwd(code3(0, 0, 1)) == WORKSPACE and fwd(code3(0, 0, 2)) == WORKSPACE and fwd(code3(0, 0, 0)) == BAD_ARG
        for fwd in forwards(lib, gen, 129, 131):
            assert fwd(code3(0, 0, 2)) == WORKSPACE and fwd(code3(0, 0, 1)) == BAD_ARG
    finally:
        assert lib.pnp_generator_set_any_size(gen, 0) == 0


def test_the_metric_entries_take_a_format_and_refuse_what_it_refuses(lib):
    assert lib.pnp_abi_version() == 5
    p8, q8, p16, q16 = planes8(64), planes8(64), planes16(64), planes16(64)
    calls = [lambda f, c=0, h=64, w=64: lib.pnp_psnr_sse_yuv(ctypes.byref(p8), ctypes.byref(q8), None, 1, h, w, c, f, None),
             lambda f, c=0, h=64, w=64: lib.pnp_ssim_partials_yuv(ctypes.byref(p8), ctypes.byref(q8), 7, None, 1, h, w, c, f, None),
             lambda f, c=0, h=64, w=64: lib.pnp_psnr_sse_yuvp16(ctypes.byref(p16), ctypes.byref(q16), None, 1, h, w, c, f, None),
             lambda f, c=0, h=64, w=64: lib.pnp_ssim_partials_yuvp16(ctypes.byref(p16), ctypes.byref(q16), 7, None, 1, h, w, c, f, None)]
    # (a null output is BAD_ARG for every format: what is asked for below is decided in front of it only where the answer is 0 blocks)
    for f in (-1, 3, 4, 1 << 12):
        assert all(c(f) == BAD_ARG for c in calls), f
        assert lib.pnp_ssim_blocks_yuv(64, 64, 0, _native.PLANE_Y, f) == 0
    # the crop rule through the block count: odd crops are 4:4:4's alone, and there chroma is cropped like luma
    for plane in (_native.PLANE_Y, _native.PLANE_CB, _native.PLANE_CR):
        assert lib.pnp_ssim_blocks_yuv(64, 64, 3, plane, 1) == 0 and lib.pnp_ssim_blocks_yuv(64, 64, 3, plane, 0) == 0
        assert lib.pnp_ssim_blocks_yuv(64, 64, 3, plane, 2) == lib.pnp_ssim_blocks(64, 64, 3) > 0
        for h, w, crop in ((64, 64, 0), (64, 96, 4), (178, 64, 2), (20, 20, 0), (63, 64, 0), (64, 63, 0)):
            assert lib.pnp_ssim_blocks_yuv(h, w, crop, plane, 0) == lib.pnp_ssim_blocks_yuv420(h, w, crop, plane), (plane, h, w, crop)
    assert lib.pnp_ssim_blocks_yuv(64, 96, 4, _native.PLANE_CB, 1) == lib.pnp_ssim_blocks(64 - 8, 48 - 4, 0) == 6
    assert lib.pnp_ssim_blocks_yuv(63, 96, 0, _native.PLANE_CR, 1) == lib.pnp_ssim_blocks(63, 48, 0)        # an odd h is 4:2:2's to take
    assert lib.pnp_ssim_blocks_yuv(64, 95, 0, _native.PLANE_Y, 1) == 0 and lib.pnp_ssim_blocks_yuv(63, 95, 1, _native.PLANE_CB, 2) > 0
    assert lib.pnp_ssim_blocks_yuv(64, 64, 0, 3, 2) == 0 and lib.pnp_ssim_blocks_yuv(64, 64, -2, 1, 2) == 0


def test_the_macros_are_the_headers_and_pythons_names():
    with open(os.path.join(ROOT, 'include', 'pnpvcve.h')) as fh:
        hdr = fh.read()
    for name, val in (('420', 0), ('422', 1), ('444', 2)):
        assert int(re.search(r'#define PNP_YUV_FORMAT_%s (\d+)' % name, hdr).group(1)) == val
        assert _native.YUV_FORMAT[name] == val and ops.YUV_FORMATS[val] == name
    assert re.search(r'#define PNP_YUV_CODE3\(standard, chroma, format\) \(\(standard\) \| \(\(chroma\) << 8\) \| \(\(format\) << 12\)\)', hdr)
    assert re.search(r'#define PNP_YUV_CODE\(standard, chroma\) \(\(standard\) \| \(\(chroma\) << 8\)\)', hdr)
    assert re.search(r'#define PNP_OUT_YUV420 4\b', hdr) and 'historical' in hdr
    import yuv_formats_ref
    assert yuv_formats_ref.FORMAT_NAMES == ops.YUV_FORMATS and yuv_formats_ref.FORMATS == _native.YUV_FACTORS
    for s, name in enumerate(('bt601-limited', 'bt601-full', 'bt709-limited', 'bt709-full')):
        for m, chroma in enumerate(ops.YUV_CHROMA):
            assert ops._yuv_code(name, chroma) == ops._yuv_code(name, chroma, format='420') == ch.code(s, m)
            for f, fmt in enumerate(ops.YUV_FORMATS):
                assert ops._yuv_code(s, chroma, format=fmt) == code3(s, m, f)
                assert ops._yuv_code_split3(code3(s, m, f)) == (s, chroma, fmt)
    for bad in ('4:2:2', 422, None, '440'):
        with pytest.raises(ValueError, match='format'):
            ops._yuv_code(0, 'left', format=bad)
    for bad in (code3(0, 0, 1), code3(3, 3, 2)):       # the two-part split keeps refusing what it refused
        with pytest.raises(ValueError):
            ops._yuv_code_split(bad)
    with pytest.raises(ValueError):
        ops._yuv_code_split3(code3(0, 0, 3))


# ------------------------------------------------------------------------------------------------ Python refusals, before any GPU call
def cpu_frames(cls, t, h, w, ch_, cw, dtype=torch.uint8, tail=()):
    return cls(torch.zeros((t, h, w), dtype=dtype), torch.zeros((t, ch_, cw), dtype=dtype), torch.zeros((t, ch_, cw), dtype=dtype), *tail)


def test_the_frame_classes_are_siblings_and_the_420_functions_keep_refusing_them():
    f422, f444 = cpu_frames(ops.Yuv422Frames, 2, 8, 8, 8, 4), cpu_frames(ops.Yuv444Frames16, 2, 8, 8, 8, 8, torch.int16, (10, False))
    for f, fmt in ((f422, '422'), (f444, '444'), (cpu_frames(ops.Yuv420Frames, 2, 8, 8, 4, 4), '420')):
        assert ops.is_yuv(f) and ops.yuv_format(f) == fmt
    assert not isinstance(f422, ops.Yuv420Frames) and not isinstance(f444, (ops.Yuv420Frames16, ops.Yuv444Frames))
    assert not ops.is_yuv((f422.y, f422.cb, f422.cr))
    with pytest.raises(TypeError):
        ops.yuv_format(f422.y)
    for fn in (ops.frames_from_yuv420, ops.pack_lr_yuv420):
        with pytest.raises(TypeError, match='Yuv420Frames'):
            fn(f422)
    with pytest.raises(TypeError, match='Yuv420Frames16'):
        ops.frames_from_yuv420p16(f444)
    for fn in (ops.psnr_yuv420, ops.ssim_yuv420, ops.msssim_yuv420, ops.xpsnr_yuv420, ops.psnrb_yuv420, ops.psnr_sse_yuv420):
        with pytest.raises(TypeError, match='4:2:0'):
            fn(f422, f422)
    with pytest.raises(TypeError):
        ops.frames_from_yuv((f422.y, f422.cb, f422.cr))


def test_wrong_shapes_layouts_and_crops_raise_before_any_gpu_call():
    # the chroma shape of the class
    for fmt, cshape in (('422', (2, 4, 4)), ('422', (2, 8, 8)), ('444', (2, 8, 4)), ('444', (2, 4, 4)), ('420', (2, 8, 4))):
        with pytest.raises(ValueError, match='cb and cr must be'):
            ops._yuv_shape_check(fmt, (2, 8, 8), cshape, cshape)
    ops._yuv_shape_check('422', (2, 7, 8), (2, 7, 4), (2, 7, 4))
    ops._yuv_shape_check('444', (2, 7, 7), (2, 7, 7), (2, 7, 7))
    with pytest.raises(ValueError, match='even width'):
        ops._yuv_shape_check('422', (2, 8, 7), (2, 8, 3), (2, 8, 3))
    with pytest.raises(ValueError, match='even width'):
        ops.yuv_views(torch.zeros((2, 14, 7), dtype=torch.uint8), 7, 7, 'nv16')
    v = ops.yuv_views(torch.zeros((2, 21, 7), dtype=torch.uint8), 7, 7, 'yuv444p')
    assert isinstance(v, ops.Yuv444Frames) and v.cb.shape == (2, 7, 7)
    v = ops.yuv_views(torch.zeros((2, 21, 7), dtype=torch.int16), 7, 7, 'p412')
    assert isinstance(v, ops.Yuv444Frames16) and v.cb.shape == (2, 7, 7) and v.cb.stride(-1) == 2 and (v.bit_depth, v.msb_aligned) == (12, True)
    v = ops.yuv_views(torch.zeros((3, 7 * 8 * 2), dtype=torch.uint8), 7, 8, 'yuv422p')
    assert isinstance(v, ops.Yuv422Frames) and v.cr.shape == (3, 7, 4)
    assert isinstance(ops.yuv_views(torch.zeros((2, 12, 8), dtype=torch.uint8), 8, 8, 'nv12'), ops.Yuv420Frames)
    assert isinstance(ops.yuv_views(torch.zeros((2, 12, 8), dtype=torch.int16), 8, 8, 'p010'), ops.Yuv420Frames16)
    for buf, layout in ((torch.zeros((2, 16, 8), dtype=torch.uint8), 'yuv444p'), (torch.zeros((2, 16, 8), dtype=torch.uint8), 'p210'),
                        (torch.zeros((2, 16, 8), dtype=torch.int16), 'nv16')):
        with pytest.raises((ValueError, TypeError)):
            ops.yuv_views(buf, 8, 8, layout)
    with pytest.raises(ValueError, match='layout'):
        ops.yuv_views(torch.zeros((2, 16, 8), dtype=torch.uint8), 8, 8, 'yuv440p')
    # the generator's routing of out_dtype: a layout of another format, 16-bit planes out of 8-bit planes in
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as G
    f422 = cpu_frames(ops.Yuv422Frames, 2, 64, 64, 64, 32)
    for layout in ('nv12', 'yuv444p', 'p010', 'nv24'):
        kinds, mask, lay, many = G._yuv_outs((torch.float32, layout))
        assert lay == layout and mask == 5
        with pytest.raises(ValueError, match='chroma format'):
            G._yuv_out_route(f422, kinds, lay)
    with pytest.raises(ValueError, match='8-bit planes in'):
        G._yuv_out_route(f422, ['yuv'], 'p210')
    assert G._yuv_out_route(f422, ['yuv'], 'nv16') == (None, None)
    f16 = cpu_frames(ops.Yuv422Frames16, 2, 64, 64, 64, 32, torch.int16, (10, True))
    assert G._yuv_out_route(f16, ['yuv'], 'p212') == (None, None)
    assert G._yuv_out_route(f16, ['u8', 'yuv'], 'nv16') == ('nv16', (torch.uint8, torch.float32))
    # metrics: an odd crop at 4:2:2, clips of two formats, metric names out of scope
    a = cpu_frames(ops.Yuv422Frames, 2, 32, 32, 32, 16)
    with pytest.raises((ValueError, RuntimeError)) as e:
        ops.psnr_yuv(a, cpu_frames(ops.Yuv444Frames, 2, 32, 32, 32, 32))
    assert 'chroma format' in str(e.value)
    from pnp_vcve_amd.restorer import BasicVSR
    assert set(ops.YUV_FORMAT_LAYOUTS) <= set(BasicVSR.YUV_OUT_LAYOUTS)
    net = BasicVSR.__new__(BasicVSR)
    for metric in ('MS-SSIM', 'XPSNR_U', 'PSNR-B'):
        net.test_cfg = dict(metrics=['PSNR', metric], crop_border=0)
        with pytest.raises(ValueError, match='4:2:2'):
            net._evaluate_yuv(a, a)
    net.test_cfg = dict(metrics=['PSNR'], crop_border=0)
    with pytest.raises(ValueError, match='plane metrics compare'):
        net.evaluate(a, cpu_frames(ops.Yuv444Frames, 2, 32, 32, 32, 32))


# ------------------------------------------------------------------------------------------------ the dataset
def write_tree(root, layout, depth, t=2, h=64, w=64, clips=('000', '011')):
    """a tree of tiny raw clips + MV records in `layout`; -> (lq folder, gt folder, {clip: the buffer as read back})"""
    rows = {'yuv422p': 2 * h, 'nv16': 2 * h, 'yuv444p': 3 * h, 'nv24': 3 * h}[layout]
    lq, gt, mv = root / 'crf25' / 'yuv', root / 'gt' / 'yuv', root / 'crf25' / 'mv'
    bufs = {}
    for d in (lq, gt):
        os.makedirs(d)
    rng = np.random.default_rng(3)
    for clip in clips:
        os.makedirs(mv / clip)
        for i in range(t):
            np.save(mv / clip / f'{i:08d}.npy', np.zeros((0, 10), np.float32))
        for d in (lq, gt):
            x = rng.integers(0, 1 << depth, (t, rows, w)).astype('<u2' if depth > 8 else np.uint8)
            x.tofile(d / f'{clip}.yuv')
            if d is lq:
                bufs[clip] = x
    return str(lq), str(gt), bufs


@pytest.mark.parametrize('layout,depth', [('yuv422p', 8), ('nv16', 8), ('yuv444p', 10)])
def test_the_dataset_reads_clips_of_the_new_formats(tmp_path, layout, depth):
    from pnp_vcve_amd.datasets import build_dataset, collate
    lq, gt, bufs = write_tree(tmp_path / 'data', layout, depth)
    ds = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=64, layout=layout, bit_depth=depth,
                            chroma='left'))
    fmt = '422' if '422' in layout or layout == 'nv16' else '444'
    assert len(ds) == 2 and ds.format == fmt
    s = ds[1]
    assert s['meta']['format'] == fmt and s['meta']['layout'] == layout and s['meta']['bit_depth'] == depth
    rows = 128 if fmt == '422' else 192
    assert s['lq_yuv'].shape == s['gt_yuv'].shape == (2, rows, 64) and s['lq_yuv'].dtype == (torch.uint8 if depth == 8 else torch.int16)
    assert np.array_equal(s['lq_yuv'].numpy().view(bufs['011'].dtype.newbyteorder('=')), bufs['011'])
    # the views the loop builds of the uploaded buffer (apis._to_device; here of the buffer where it is) are the format's class
    batch = collate([s])
    assert batch['meta'][0]['format'] == fmt and batch['lq_yuv'].shape == (1, 2, rows, 64)
    v = ops._yuv_views_format(batch['lq_yuv'], 64, 64, fmt, ops.YUV_FORMAT_LAYOUTS[layout][1], () if depth == 8 else (depth, False))
    cls = ops._YUV_CLASSES[fmt][0 if depth == 8 else 1]
    assert isinstance(v, cls) and v.y.shape == (1, 2, 64, 64) and v.cb.shape == (1, 2, 64, 32 if fmt == '422' else 64)
    assert v.cb.stride(-1) == (2 if layout == 'nv16' else 1) and v.y.data_ptr() == batch['lq_yuv'].data_ptr()
    # the file-size check carries the format: a 4:2:0 reading of the same file, and a file that is no whole number of frames
    with pytest.raises(ValueError, match='4:%s:%s' % (fmt[1], fmt[2])):
        build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=60, layout=layout, bit_depth=depth))[0]
    with pytest.raises(ValueError, match='layout'):
        build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=64, layout='yuv440p'))
    if fmt == '422':
        with pytest.raises(ValueError, match='even width'):
            build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=64, width=63, layout=layout))


# ------------------------------------------------------------------------------------------------ the stand-alone host program
def test_the_descriptor_predicates_and_the_chroma_sources_under_a_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'yuv_formats_desc')
    cmd = [cxx, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'yuv_formats_desc.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    sweep, walk, forms = out
    print(sweep, walk, forms)
    assert sweep['wrong8'] == 0, sweep['first8']
    assert sweep['wrong16'] == 0, sweep['first16']
    for name, total in (('ok8', sweep['tuples8']), ('fast8', sweep['tuples8']), ('ok16', sweep['tuples16']), ('fast16', sweep['tuples16'])):
        assert 0 < sweep[name] < total, name       # no predicate is constant on the sweep
    assert walk['errors'] == 0, walk['first']
    assert walk['cases'] == 4 * 4 * 3 * (2 + 2 + 3) and walk['loads'] > 0
    # the pack launch takes its aligned form for tight aligned planes of every new layout, and only for those
    assert forms['errors'] == 0, forms['first']
    assert forms['cases'] == 2 * (2 * 4 + 2 * 5) and r.returncode == 0
