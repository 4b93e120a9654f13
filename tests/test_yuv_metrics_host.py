"""CPU: the plane metrics of 4:2:0 clips (pnp_psnr_sse_yuv420, pnp_ssim_blocks_yuv420, pnp_ssim_partials_yuv420; include/pnpvcve.h), the
raw-clip dataset and the evaluate() refusals.

* every refusal of the C entries through ctypes on the built library: they are decided on the host, before any HIP call, so they run
  without a GPU and with null device buffers;
* the block counts against pnp_ssim_blocks;
* the plane loader both kernels fetch through (csrc/plane_load.h) on the host under AddressSanitizer + UBSan: a stand-alone program
  (tests/host/plane_metrics_stub.cpp) run as a subprocess;
* Yuv420ClipFolderDataset on files written to tmp_path;
* BasicVSR.evaluate refuses a pair of which only one side is planes."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import yuv_metrics_ref as ref
import yuv_ref
from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 1001
A = 0x1000        # an aligned "device address": never dereferenced on these paths


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def planes(w, y=A, cb=A + 0x100000, cr=A + 0x100001, y_pitch=None, c_pitch=None, c_step=2, frame=1 << 22):
    return _native.Yuv420Planes(y, cb, cr, w if y_pitch is None else y_pitch, c_step * (w // 2) if c_pitch is None else c_pitch, frame, frame,
                                c_step)


def i420(w, **kw):
    return planes(w, cb=A + 0x100000, cr=A + 0x200000, c_step=1, **kw)


# ------------------------------------------------------------------------------------------------ the C entries' refusals
def _entries(lib):
    ref_ = lambda d: ctypes.byref(d) if d is not None else None      # noqa: E731

    def psnr(a, b, out=A, frames=1, h=64, w=64, crop=0):
        return lib.pnp_psnr_sse_yuv420(ref_(a), ref_(b), out, frames, h, w, crop, None)

    def ssim(a, b, out=A, frames=1, h=64, w=64, crop=0, mask=7):
        return lib.pnp_ssim_partials_yuv420(ref_(a), ref_(b), mask, out, frames, h, w, crop, None)

    return psnr, ssim


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null device buffers and no GPU: every code below is decided on the host"""
    ok, ok_i = planes(64), i420(64)
    for f in _entries(lib):
        assert f(None, ok) == BAD_ARG and f(ok, None) == BAD_ARG                              # a NULL descriptor
        for field in ('y', 'cb', 'cr'):                                                       # a NULL plane of either clip
            assert f(planes(64, **{field: None}), ok) == BAD_ARG, field
            assert f(ok_i, planes(64, **{field: None})) == BAD_ARG, field
        assert f(ok, ok_i, out=None) == BAD_ARG                                               # a NULL output
        assert f(ok, ok_i, frames=0) == BAD_ARG and f(ok, ok_i, frames=-3) == BAD_ARG
        for h, w in ((63, 64), (64, 65), (0, 64), (64, 0), (1, 64), (64, 1), (-2, 64)):       # odd or < 2
            assert f(planes(max(w, 2)), planes(max(w, 2)), h=h, w=w) == BAD_ARG, (h, w)
        assert f(ok, ok_i, crop=-2) == BAD_ARG and f(ok, ok_i, crop=-1) == BAD_ARG            # a negative crop
        for crop in (1, 3, 5, 31):                                                            # an odd one
            assert f(ok, ok_i, crop=crop) == BAD_ARG, crop
        assert f(ok, ok_i, crop=32) == BAD_ARG and f(ok, ok_i, crop=34) == BAD_ARG            # 2 crop >= h, w
        assert f(planes(128), i420(128), h=64, w=128, crop=32) == BAD_ARG and f(planes(64), i420(64), h=128, w=64, crop=32) == BAD_ARG
        for step in (0, 3, 4, -1):                                                            # c_step 1 | 2
            assert f(planes(64, c_step=step, c_pitch=256), ok) == BAD_ARG and f(ok, planes(64, c_step=step, c_pitch=256)) == BAD_ARG, step
        assert f(planes(64, y_pitch=63), ok) == BAD_ARG and f(ok, planes(64, y_pitch=63)) == BAD_ARG      # a pitch below the row's bytes
        assert f(planes(64, c_pitch=63), ok) == BAD_ARG and f(ok, i420(64, c_pitch=31)) == BAD_ARG
    psnr, ssim = _entries(lib)
    for mask in (0, 8, -1, 15):                                                               # plane_mask 0 or beyond 7
        assert ssim(ok, ok_i, mask=mask) == BAD_ARG, mask
    # a cropped plane OF THE MASK below 11 x 11: 20 x 20 frames hold an 11 x 11 window in Y (up to a crop of 4) and none in chroma
    s20 = lambda mask, crop=0: ssim(planes(20), i420(20), h=20, w=20, crop=crop, mask=mask)      # noqa: E731
    for mask in (2, 4, 6, 3, 5, 7):
        assert s20(mask) == BAD_ARG, mask
    assert s20(1, crop=6) == BAD_ARG
    # 32 x 32 frames: chroma is 16 x 16, a crop of 6 leaves 10 x 10 of it (and 20 x 20 of Y)
    assert ssim(planes(32), i420(32), h=32, w=32, crop=6, mask=2) == BAD_ARG
    assert lib.pnp_abi_version() == 5


def test_block_counts_are_pnp_ssim_blocks_of_each_plane(lib):
    Y, CB, CR = _native.PLANE_Y, _native.PLANE_CB, _native.PLANE_CR
    assert (Y, CB, CR) == (1, 2, 4)
    for h, w in ((40, 56), (34, 70), (66, 38), (64, 64), (720, 1280), (20, 20), (22, 24), (180, 320)):
        for crop in (0, 2, 4, 8):
            if 2 * crop >= min(h, w):
                continue
            assert lib.pnp_ssim_blocks_yuv420(h, w, crop, Y) == lib.pnp_ssim_blocks(h, w, crop), (h, w, crop)
            for plane in (CB, CR):
                assert lib.pnp_ssim_blocks_yuv420(h, w, crop, plane) == lib.pnp_ssim_blocks(h // 2, w // 2, crop // 2), (h, w, crop)
    assert lib.pnp_ssim_blocks_yuv420(34, 70, 0, Y) == 2 * 2 and lib.pnp_ssim_blocks_yuv420(66, 38, 0, CB) == 2 * 1
    assert lib.pnp_ssim_blocks_yuv420(20, 20, 0, CB) == 0 and lib.pnp_ssim_blocks_yuv420(20, 20, 0, Y) == 1
    # 0 when it cannot run: an unknown plane (or a mask of several), odd sizes, an odd or negative crop
    for plane in (0, 3, 5, 7, 8, -1):
        assert lib.pnp_ssim_blocks_yuv420(64, 64, 0, plane) == 0, plane
    assert lib.pnp_ssim_blocks_yuv420(63, 64, 0, Y) == 0 and lib.pnp_ssim_blocks_yuv420(64, 65, 0, Y) == 0
    assert lib.pnp_ssim_blocks_yuv420(64, 64, 1, Y) == 0 and lib.pnp_ssim_blocks_yuv420(64, 64, -2, Y) == 0


# ------------------------------------------------------------------------------------------------ the loader under the sanitizers
def test_the_plane_loader_fetches_every_sample_once_inside_its_rows_under_asan(tmp_path):
    """tests/host/plane_metrics_stub.cpp: a stand-alone program; nothing is loaded into this interpreter"""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path / 'plane_metrics_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-Wno-attributes',
           '-Wno-unknown-pragmas', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'plane_metrics_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    docs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    cases = [d for d in docs if 'off' in d]
    assert docs[-1] == {'cases': len(cases)}
    # every base offset 0..3, pitches w, w + 6, w + 7, steps 1 and 2, widths 36, 38 and 70 (and three crops each)
    want = {(off, extra, step, cols, crop) for off in range(4) for extra in (0, 6, 7) for step in (1, 2) for cols in (36, 38, 70) for crop in (0, 1, 2)}
    assert {(d['off'], d['pitch_extra'], d['step'], d['cols'], d['crop']) for d in cases} == want and len(cases) == len(want)
    for d in cases:
        assert d['errors'] == [], d
        assert d['dwords'] > 0, d
    # byte loads at heads, tails and short groups: a misaligned plane read from its first sample has some (behind a crop the covering
    # dwords of the first and the last group lie inside the plane), and so has every cropped width that is no multiple of 4
    assert all(d['bytes'] > 0 for d in cases if (d['off'] and not d['crop']) or (d['cols'] - 2 * d['crop']) % 4), [d for d in cases if not d['bytes']][:3]
    # an aligned plane with an aligned pitch and width needs none
    assert all(d['bytes'] == 0 for d in cases if not d['off'] and d['pitch_extra'] == 0 and d['cols'] == 36 and d['crop'] == 0)


# ------------------------------------------------------------------------------------------------ the numpy restatement itself
def test_the_restatement_on_a_hand_made_case():
    y = np.zeros((1, 8, 8), np.uint8)
    y2 = y.copy()
    y2[0, 0, 0] = 255          # outside a crop of 2
    y2[0, 3, 3] = 2            # inside
    c = np.full((1, 4, 4), 10, np.uint8)
    c2 = c.copy()
    c2[0, 0, 0] = 13           # outside a chroma crop of 1
    c2[0, 1, 2] = 7            # inside
    a, b = (y, c, c), (y2, c2, c)
    assert ref.sse_yuv420(a, b, 0).tolist() == [[255 * 255 + 4, 9 + 9, 0]]
    assert ref.sse_yuv420(a, b, 2).tolist() == [[4, 9, 0]]
    assert ref.counts(8, 8, 2).tolist() == [16.0, 4.0, 4.0]
    p = ref.psnr_yuv420(a, b, 2)
    assert p[0, 0] == 10.0 * np.log10(255.0 ** 2 * 16 / 4) and p[0, 1] == 10.0 * np.log10(255.0 ** 2 * 4 / 9) and np.isinf(p[0, 2])
    q = np.array([[40.0, 44.0, 48.0]])
    assert ref.psnr_611(q).tolist() == [(6 * 40.0 + 44.0 + 48.0) / 8.0]


# ------------------------------------------------------------------------------------------------ the dataset
def _write_tree(root, layout, t=4, h=16, w=24, scale=1, clips=('000', '001')):
    """<root>/crf25/yuv/<clip>.yuv, <root>/crf25/mv/<clip>/%08d.npy, <root>/gt/<clip>.yuv, <root>/qp.json -> the planes written"""
    lq_dir, mv_dir, gt_dir = root / 'crf25' / 'yuv', root / 'crf25' / 'mv', root / 'gt'
    for d in (lq_dir, gt_dir):
        d.mkdir(parents=True)
    rng = np.random.default_rng(5)
    table, written = {'crf25': {}}, {}
    for key in clips:
        (mv_dir / key).mkdir(parents=True)
        table['crf25'][key] = {}
        for i in range(t):
            np.save(mv_dir / key / f'{i:08d}.npy', rng.random((3 + i, 10)).astype(np.float32))
            table['crf25'][key][str(i)] = dict(slice='IBP'[min(i, 2)], QP=20 + i)
        for folder, s in ((lq_dir, 1), (gt_dir, scale)):
            p = [rng.integers(0, 256, (t, h * s, w * s), dtype=np.uint8), rng.integers(0, 256, (t, h * s // 2, w * s // 2), dtype=np.uint8),
                 rng.integers(0, 256, (t, h * s // 2, w * s // 2), dtype=np.uint8)]
            yuv_ref.pack(*p, layout).tofile(folder / f'{key}.yuv')
            written[(folder.name, key)] = p
    (root / 'qp.json').write_text(json.dumps(table))
    return lq_dir, gt_dir, root / 'qp.json', written


def _unpack(buf, h, w, layout):
    """packed (t, 3h/2, w) uint8 -> y, cb, cr, by the layout's definition (tightly packed)"""
    t = buf.shape[0]
    flat = buf.reshape(t, -1)
    y = flat[:, :h * w].reshape(t, h, w)
    c = flat[:, h * w:]
    if layout == 'i420':
        n = (h // 2) * (w // 2)
        return y, c[:, :n].reshape(t, h // 2, w // 2), c[:, n:].reshape(t, h // 2, w // 2)
    pairs = c.reshape(t, h // 2, w // 2, 2)
    return (y, pairs[..., 0], pairs[..., 1]) if layout == 'nv12' else (y, pairs[..., 1], pairs[..., 0])


@pytest.mark.parametrize('layout', ['i420', 'nv12', 'nv21'])
def test_dataset_reads_back_the_planes_that_were_written(tmp_path, layout):
    from pnp_vcve_amd import datasets
    from pnp_vcve_amd.registry import DATASETS
    lq_dir, gt_dir, qp, written = _write_tree(tmp_path, layout, scale=2)
    ds = datasets.build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=str(lq_dir), gt_folder=str(gt_dir), height=16, width=24, layout=layout,
                                     yuv_standard='bt709-limited', scale=2, qp_slice_file=str(qp)))
    assert DATASETS.get('Yuv420ClipFolderDataset') is datasets.Yuv420ClipFolderDataset
    assert len(ds) == 2 and ds.mv_folder == str(tmp_path / 'crf25' / 'mv')
    for i, key in enumerate(('000', '001')):
        s = ds[i]
        assert s['lq_yuv'].dtype == torch.uint8 and tuple(s['lq_yuv'].shape) == (4, 24, 24)
        assert s['gt_yuv'].dtype == torch.uint8 and tuple(s['gt_yuv'].shape) == (4, 48, 48)
        for name, hh, ww, folder in (('lq_yuv', 16, 24, 'yuv'), ('gt_yuv', 32, 48, 'gt')):
            got = _unpack(s[name].numpy(), hh, ww, layout)
            assert all(np.array_equal(g, p) for g, p in zip(got, written[(folder, key)])), (name, key)
        assert s['meta']['layout'] == layout and s['meta']['yuv_standard'] == 'bt709-limited' and s['meta']['key'] == f'{key}/00000000'
        # the side info and the records of the PNG dataset
        assert s['slices'].reshape(-1).tolist() == [73.0, 66.0, 80.0, 80.0] and tuple(s['slices'].shape) == (4, 1, 1, 1)
        assert torch.equal(s['QPs'].reshape(-1), torch.tensor([20.0, 21.0, 22.0, 23.0]) / 255.0)
        assert torch.equal(s['base_QPs'], torch.full((4, 1, 1, 1), 25 / 255.0))
        assert tuple(s['mv_records'].shape) == (3 + 4 + 5 + 6, 10) and s['rec_frame'].tolist() == [0] * 3 + [1] * 4 + [2] * 5 + [3] * 6
        assert s['mv_records'].dtype == torch.float32 and s['rec_frame'].dtype == torch.int32
    batch = datasets.collate([ds[0]])
    assert tuple(batch['lq_yuv'].shape) == (1, 4, 24, 24) and batch['meta'][0]['layout'] == layout
    assert ds.evaluate([dict(eval_result=dict(PSNR=30.0, PSNR_YUV=31.0)), dict(eval_result=dict(PSNR=32.0, PSNR_YUV=35.0))]) == dict(PSNR=31.0, PSNR_YUV=33.0)


def test_dataset_truncates_repeats_and_finds_its_mv_folder(tmp_path):
    from pnp_vcve_amd.datasets import Yuv420ClipFolderDataset
    lq_dir, gt_dir, qp, written = _write_tree(tmp_path, 'i420')
    ds = Yuv420ClipFolderDataset(str(lq_dir), str(gt_dir), height=16, width=24, num_input_frames=3, repeat=2, qp_slice_file=str(qp))
    assert len(ds) == 4 and ds.layout == 'i420' and ds.yuv_standard == 'bt601-limited'
    s = ds[3]
    assert s['meta']['key'].startswith('001/') and tuple(s['lq_yuv'].shape) == (3, 24, 24) and tuple(s['gt_yuv'].shape) == (3, 24, 24)
    assert np.array_equal(_unpack(s['lq_yuv'].numpy(), 16, 24, 'i420')[0], written[('yuv', '001')][0][:3])
    assert tuple(s['slices'].shape) == (3, 1, 1, 1) and s['rec_frame'].tolist() == [0] * 3 + [1] * 4 + [2] * 5
    # without a QP table: I then P, QP 0, as the PNG dataset does
    s = Yuv420ClipFolderDataset(str(lq_dir), str(gt_dir), height=16, width=24, num_input_frames=2)[0]
    assert s['slices'].reshape(-1).tolist() == [73.0, 80.0] and s['QPs'].reshape(-1).tolist() == [0.0, 0.0]
    # an explicit mv_folder; a folder without a 'yuv' component needs one
    other = tmp_path / 'elsewhere'
    shutil.copytree(tmp_path / 'crf25' / 'mv', other)
    shutil.copytree(lq_dir, tmp_path / 'crf25' / 'raw')
    with pytest.raises(ValueError, match='mv_folder'):
        Yuv420ClipFolderDataset(str(tmp_path / 'crf25' / 'raw'), str(gt_dir), height=16, width=24)
    ds = Yuv420ClipFolderDataset(str(tmp_path / 'crf25' / 'raw'), str(gt_dir), height=16, width=24, mv_folder=str(other))
    assert torch.equal(ds[0]['mv_records'], Yuv420ClipFolderDataset(str(lq_dir), str(gt_dir), height=16, width=24)[0]['mv_records'])
    for bad in (dict(height=15), dict(width=0), dict(layout='p010'), dict(yuv_standard='bt2020')):
        with pytest.raises(ValueError):
            Yuv420ClipFolderDataset(str(lq_dir), str(gt_dir), **dict(dict(height=16, width=24), **bad))


def test_a_ragged_or_empty_file_raises_naming_the_file(tmp_path):
    from pnp_vcve_amd.datasets import Yuv420ClipFolderDataset
    lq_dir, gt_dir, qp, _ = _write_tree(tmp_path, 'i420')
    ds = Yuv420ClipFolderDataset(str(lq_dir), str(gt_dir), height=16, width=24)
    per = 16 * 24 * 3 // 2
    with open(lq_dir / '001.yuv', 'ab') as f:
        f.write(b'\x00' * 7)                                         # not a whole number of frames
    with pytest.raises(ValueError, match='001.yuv'):
        ds[1]
    assert tuple(ds[0]['lq_yuv'].shape) == (4, 24, 24)               # the other clip is what it was
    (lq_dir / '001.yuv').write_bytes(b'\x00' * (per - 1))            # fewer than one frame
    with pytest.raises(ValueError, match='001.yuv'):
        ds[1]
    (lq_dir / '001.yuv').write_bytes(b'')
    with pytest.raises(ValueError, match='001.yuv'):
        ds[1]
    (gt_dir / '000.yuv').write_bytes(b'\x00' * (2 * per + 1))        # the ground truth is held to the same rule
    with pytest.raises(ValueError, match='gt.000.yuv'):
        ds[0]
    (gt_dir / '000.yuv').write_bytes(b'\x00' * (2 * per))            # ... and must hold the frames of the clip
    with pytest.raises(ValueError, match='000.yuv'):
        ds[0]


# ------------------------------------------------------------------------------------------------ evaluate
def _model(metrics=('PSNR', 'SSIM'), **cfg):
    import golden_util as gu
    from pnp_vcve_amd import restorer      # noqa: F401
    from pnp_vcve_amd.registry import build_model
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **dict(gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=1))
    return build_model(dict(type='BasicVSR', generator=gen), train_cfg=None, test_cfg=dict(metrics=list(metrics), crop_border=0, **cfg))


def test_evaluate_refuses_a_pair_of_which_one_side_is_planes():
    from pnp_vcve_amd import ops
    m = _model()
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    frames = ops.Yuv420Frames(z(1, 3, 64, 64), z(1, 3, 32, 32), z(1, 3, 32, 32))
    for out, gt in ((frames, torch.zeros(1, 3, 3, 64, 64)), (torch.zeros(1, 3, 3, 64, 64), frames), (frames, z(1, 3, 64, 64, 3))):
        with pytest.raises(ValueError, match='Yuv420Frames'):
            m.evaluate(out, gt)
    # two clips of planes: refused for what they are before any GPU work -- a batch of two, an unknown metric, a colour model
    two = ops.Yuv420Frames(z(2, 3, 64, 64), z(2, 3, 32, 32), z(2, 3, 32, 32))
    with pytest.raises(ValueError, match='one clip'):
        m.evaluate(two, two)
    with pytest.raises(ValueError, match='PSNR_W'):
        _model(metrics=('PSNR', 'PSNR_W')).evaluate(frames, frames)
    with pytest.raises(ValueError, match='color model'):
        _model(convert_to='rgb').evaluate(frames, frames)
    # the plane-only metric names stay unknown to the RGB path
    with pytest.raises(KeyError):
        _model(metrics=('PSNR_YUV',)).evaluate(torch.zeros(1, 3, 3, 64, 64), torch.zeros(1, 3, 3, 64, 64))
    # the planes themselves are on the host here: no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        m.evaluate(frames, frames)


def test_the_ops_refuse_bad_pairs_before_any_gpu_work():
    from pnp_vcve_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    a = ops.Yuv420Frames(z(3, 64, 64), z(3, 32, 32), z(3, 32, 32))
    with pytest.raises(TypeError):
        ops.psnr_yuv420(a, torch.zeros(3, 3, 64, 64))
    with pytest.raises(TypeError):
        ops.ssim_yuv420(torch.zeros(3, 3, 64, 64), a)
    for planes_arg in ('', 'yy', 'rgb', 'yuvy', None, 3):
        with pytest.raises(ValueError, match='planes'):
            ops.ssim_yuv420(a, a, planes=planes_arg)
    assert hasattr(ops, 'psnr_sse_yuv420') and _native.SIGNATURES['pnp_psnr_sse_yuv420'][0] is ctypes.c_int
