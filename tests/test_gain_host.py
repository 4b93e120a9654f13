"""CPU: the enhancement gain above the sums -- BasicVSR.evaluate with the gain names on host tensors (the numpy path), every refusal
raised before any GPU work, metrics.gain_report, and the binding's declarations.  The sums themselves are tests/test_gain_ref.py's."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import gain_ref as ref
from pnp_vcve_amd import _native, metrics, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN = ['PSNR_LQ', 'SSIM_LQ', 'dPSNR', 'dSSIM', 'PSNR_SD', 'PSNR_SD_LQ']
PLANE_ONLY = ['dPSNR_U', 'dPSNR_V', 'PSNR_LQ_U', 'PSNR_LQ_V', 'dSSIM_U', 'dSSIM_V', 'SSIM_LQ_U', 'SSIM_LQ_V', 'dPSNR_YUV']
T, H, W = 3, 66, 78


def _model(metrics=('PSNR', 'SSIM'), crop_border=0, **cfg):
    import golden_util as gu
    from pnp_vcve_amd import restorer      # noqa: F401
    from pnp_vcve_amd.registry import build_model
    gen = dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **dict(gu.syn.DEFAULT_GENERATOR_CFG, num_blocks=1, **cfg.pop('gen', {})))
    return build_model(dict(type='BasicVSR', generator=gen), train_cfg=None, test_cfg=dict(metrics=list(metrics), crop_border=crop_border, **cfg))


def clips(seed=0):
    """gt, lq, output as (1,T,3,H,W) fp32 frames on the byte grid (so tensor2img's rounding is exact) and their bytes (T,H,W,3) RGB"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    l = np.clip(g.astype(np.int64) + rng.randint(-14, 15, g.shape), 0, 255).astype(np.uint8)
    a = np.clip(g.astype(np.int64) + rng.randint(-9, 10, g.shape), 0, 255).astype(np.uint8)
    f32 = lambda x: torch.from_numpy(x.astype(np.float32) / 255.0).permute(0, 3, 1, 2)[None].contiguous()      # noqa: E731
    return (f32(a), f32(l), f32(g)), (a, l, g)


def rel(got, want):
    if math.isinf(want) or math.isinf(got):
        return 0.0 if got == want else math.inf
    return abs(got - want) / abs(want) if want else abs(got)


def test_the_names_and_the_binding():
    assert list(metrics.GAIN_METRICS) == GAIN and list(metrics.GAIN_PLANE_METRICS) == PLANE_ONLY
    from pnp_vcve_amd.restorer import BasicVSR
    for name in GAIN + PLANE_ONLY:
        assert name in BasicVSR.YUV_METRICS and name in BasicVSR.YUV_FORMAT_METRICS and name not in metrics.ALLOWED_METRICS
    hdr = open(os.path.join(ROOT, 'include', 'pnpvcve.h')).read()
    declared = set(re.findall(r'\b(pnp_gain_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'pnp_gain_grid', 'pnp_gain_cell_count', 'pnp_gain_luma_tiles', 'pnp_gain_sums_io', 'pnp_gain_sums_yuv', 'pnp_gain_sums_yuvp16'}
    assert declared <= set(_native.SIGNATURES)
    L = _native.lib()
    for name in declared:
        assert hasattr(L, name) and len(_native.SIGNATURES[name][1]) == len(re.search(r'^int ' + name + r'\(([^;]*)\);', hdr, re.M).group(1).split(',')), name
    assert L.pnp_abi_version() == 5
    for fn in ('gain_sums_frames', 'gain_sums_yuv', 'gain_frames', 'gain_yuv'):
        assert callable(getattr(ops, fn))
    from pnp_vcve_amd import build_native
    assert 'gain.hip' in build_native.SOURCES


@pytest.mark.parametrize('convert_to', [None, 'y'])
@pytest.mark.parametrize('crop', [0, 6])
def test_evaluate_serves_the_names_with_lq_on_host_tensors(crop, convert_to):
    (a, l, g), (ba, bl, bg) = clips(1)
    m = _model(metrics=['PSNR', 'SSIM'] + GAIN, crop_border=crop, convert_to=convert_to, gain_block=16)
    got = m.evaluate(a, g, lq=l)
    assert list(got) == ['PSNR', 'SSIM'] + GAIN
    # every existing result is what it is without a gain name
    plain = _model(metrics=['PSNR', 'SSIM'], crop_border=crop, convert_to=convert_to).evaluate(a, g)
    assert plain == {k: got[k] for k in ('PSNR', 'SSIM')}
    assert _model(metrics=['PSNR', 'SSIM'], crop_border=crop, convert_to=convert_to).evaluate(a, g, lq=l) == plain
    # the values from the restatement's sums
    if convert_to == 'y':
        xa, xl, xg = (ref.luma(x) for x in (ba, bl, bg))
        n = (H - 2 * crop) * (W - 2 * crop)
    else:
        xa, xl, xg = ba, bl, bg
        n = 3 * (H - 2 * crop) * (W - 2 * crop)
    grid = ref.gain_grid(xa, xl, xg, crop, 16)[:, 0]
    ea, el = [float(v) for v in grid[..., 0].sum(axis=(1, 2))], [float(v) for v in grid[..., 1].sum(axis=(1, 2))]
    pa, pl = [ref.psnr(e, n, 255.0) for e in ea], [ref.psnr(e, n, 255.0) for e in el]
    want = dict(PSNR_LQ=sum(pl) / T, dPSNR=sum(ref.dpsnr(x, y) for x, y in zip(ea, el)) / T, PSNR_SD=ref.sd(pa), PSNR_SD_LQ=ref.sd(pl))
    for k, v in want.items():
        assert rel(got[k], v) <= 1e-12, (k, got[k], v)
    assert got['dPSNR'] > 0 and abs(got['dPSNR'] - (got['PSNR'] - got['PSNR_LQ'])) <= 1e-3     # (PSNR itself is the host path's float32 mean: ~1e-6 of 30 dB a frame)
    # the SSIM halves are the existing SSIM, called twice
    ssim_lq = _model(metrics=['SSIM'], crop_border=crop, convert_to=convert_to).evaluate(l, g)['SSIM']
    assert got['SSIM_LQ'] == ssim_lq and rel(got['dSSIM'], got['SSIM'] - ssim_lq) <= 1e-9
    # what evaluate leaves for the report
    assert m.last_gain['grid'].shape == grid.shape and m.last_gain['classes'] is None and m.last_gain['block'] == 16
    assert int(m.last_gain['counts'].sum()) == n
    # the identity "enhancement": the output is lq
    same = _model(metrics=GAIN, crop_border=crop, convert_to=convert_to).evaluate(l, g, lq=l)
    assert same['dPSNR'] == 0.0 and same['dSSIM'] == 0.0 and same['PSNR_SD'] == same['PSNR_SD_LQ']


def test_evaluate_refuses_before_any_gpu_work():
    (a, l, g), _ = clips(2)
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    z16 = lambda *s: torch.zeros(s, dtype=torch.int16)      # noqa: E731
    for name in GAIN:
        with pytest.raises(ValueError, match='lq'):
            _model(metrics=['PSNR', name]).evaluate(a, g)
    with pytest.raises(ValueError, match='lq'):
        _model(metrics=['PSNR'], gain_report='/nonexistent').evaluate(a, g)
    with pytest.raises(ValueError, match='vsr'):
        _model(metrics=['dPSNR'], gen=dict(vsr=True)).evaluate(a, g, lq=l[..., ::4, ::4])
    with pytest.raises(ValueError, match='block'):
        _model(metrics=['dPSNR'], gain_block=48).evaluate(a, g, lq=l)
    with pytest.raises(ValueError, match=r'\(3, 66, 74\)'):
        _model(metrics=['dPSNR']).evaluate(a, g, lq=l[..., :-4])
    with pytest.raises(ValueError, match='frames'):
        _model(metrics=['PSNR_SD']).evaluate(a, g, lq=l[:, :2])
    with pytest.raises(ValueError, match='centre-frame'):
        _model(metrics=['dPSNR']).evaluate(a[:, 1], g[:, 1], lq=l)
    # the plane-only names stay unknown to the RGB path, as 'PSNR_YUV'
    for name in PLANE_ONLY:
        with pytest.raises(KeyError):
            _model(metrics=['PSNR', name]).evaluate(a, g, lq=l)
    # clips of planes: lq of another frame class, bit depth, format or size (host tensors: nothing reaches the GPU)
    f8 = ops.Yuv420Frames(z8(1, T, 64, 64), z8(1, T, 32, 32), z8(1, T, 32, 32))
    f10 = ops.Yuv420Frames16(z16(1, T, 64, 64), z16(1, T, 32, 32), z16(1, T, 32, 32), 10, False)
    f12 = ops.Yuv420Frames16(z16(1, T, 64, 64), z16(1, T, 32, 32), z16(1, T, 32, 32), 12, False)
    f422 = ops.Yuv422Frames(z8(1, T, 64, 64), z8(1, T, 64, 32), z8(1, T, 64, 32))
    small = ops.Yuv420Frames(z8(1, T, 32, 64), z8(1, T, 16, 32), z8(1, T, 16, 32))
    m = _model(metrics=['PSNR', 'dPSNR', 'dPSNR_YUV'])
    with pytest.raises(ValueError, match='lq'):
        m.evaluate(f8, f8)
    with pytest.raises(ValueError, match='10-bit.*8-bit'):
        m.evaluate(f8, f8, lq=f10)
    with pytest.raises(ValueError, match='12-bit.*10-bit'):
        m.evaluate(f10, f10, lq=f12)
    with pytest.raises(ValueError, match='422'):
        m.evaluate(f8, f8, lq=f422)
    with pytest.raises(ValueError, match='frame class'):
        m.evaluate(f8, f8, lq=l)
    with pytest.raises(ValueError, match='frame class'):
        _model(metrics=['dPSNR']).evaluate(a, g, lq=f8)
    with pytest.raises(ValueError, match=r'\(3, 32, 64\)'):
        m.evaluate(f8, f8, lq=small)
    # accepted names on planes get as far as the device check: no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        m.evaluate(f8, f8, lq=f8)
    with pytest.raises(RuntimeError, match='CUDA'):
        _model(metrics=PLANE_ONLY + GAIN).evaluate(f422, f422, lq=f422)


def test_the_ops_refuse_before_any_gpu_work():
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    z16 = lambda *s: torch.zeros(s, dtype=torch.int16)      # noqa: E731
    f8 = ops.Yuv420Frames(z8(T, 64, 64), z8(T, 32, 32), z8(T, 32, 32))
    f10 = ops.Yuv420Frames16(z16(T, 64, 64), z16(T, 32, 32), z16(T, 32, 32), 10, False)
    f12 = ops.Yuv420Frames16(z16(T, 64, 64), z16(T, 32, 32), z16(T, 32, 32), 12, False)
    f444 = ops.Yuv444Frames(z8(T, 64, 64), z8(T, 64, 64), z8(T, 64, 64))
    with pytest.raises(ValueError, match='frame class'):
        ops.gain_sums_yuv(f8, f10, f8)
    with pytest.raises(ValueError, match='frame class'):
        ops.gain_sums_yuv(f8, f8, f444)
    with pytest.raises(ValueError, match='bit depth'):
        ops.gain_sums_yuv(f10, f10, f12)
    with pytest.raises(ValueError, match='bit depth'):
        ops.gain_yuv(f12, f10, f10)
    with pytest.raises(ValueError, match='planes'):
        ops.gain_sums_yuv(f8, f8, f8, planes='yy')
    with pytest.raises(RuntimeError, match='CUDA'):          # everything else about them is fine: the planes are on the host
        ops.gain_sums_yuv(f8, f8, f8)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.gain_sums_frames(torch.zeros(T, 3, 64, 64), torch.zeros(T, 3, 64, 64), torch.zeros(T, 3, 64, 64))


def test_gain_report_groups_by_slice_type_and_qp(tmp_path):
    rng = np.random.RandomState(7)
    t, h, w = 4, 66, 78
    g = rng.randint(0, 256, (t, h, w, 3)).astype(np.uint8)
    l = np.clip(g.astype(np.int64) + rng.randint(-14, 15, g.shape), 0, 255).astype(np.uint8)
    a = np.clip(g.astype(np.int64) + rng.randint(-9, 10, g.shape), 0, 255).astype(np.uint8)
    par = np.zeros((t, 3, h, w), np.float32)
    par[:, 0, :40, :40] = 1
    par[:, 1, 20:, 30:] = 1
    par[:, 2, 50:, :] = 1
    crop, block = 2, 32
    grid, classes = metrics.gain_sums(a, l, g, crop, block, par=par)
    counts = metrics.gain_cell_counts(h, w, crop, block) * 3
    ssim = np.array([0.9, 0.8, 0.85, 0.7])
    ssim_lq = np.array([0.8, 0.75, 0.8, 0.72])
    doc = metrics.gain_report(grid[:, 0], counts, 255.0, slices=[float(ord(c)) for c in 'IBPB'], qps=[22, 27, 22, 27], base_qps=[25] * 4,
                              classes=classes, class_samples=3, ssim=ssim, ssim_lq=ssim_lq, block=block)
    doc = json.loads(json.dumps(doc))                                  # it is JSON
    assert set(doc) == {'block', 'frames', 'by_slice', 'by_qp', 'classes', 'grid', 'dPSNR'} and doc['block'] == 32
    keys = {'index', 'slice', 'qp', 'base_qp', 'PSNR', 'PSNR_LQ', 'dPSNR', 'SSIM', 'SSIM_LQ', 'dSSIM'}
    assert [set(f) for f in doc['frames']] == [keys] * 4
    assert [f['slice'] for f in doc['frames']] == list('IBPB') and [f['qp'] for f in doc['frames']] == [22.0, 27.0, 22.0, 27.0]
    assert [f['index'] for f in doc['frames']] == [0, 1, 2, 3] and all(f['base_qp'] == 25.0 for f in doc['frames'])
    n = float(counts.sum())
    ea, el = grid[:, 0, :, :, 0].sum(axis=(1, 2)), grid[:, 0, :, :, 1].sum(axis=(1, 2))
    for i, f in enumerate(doc['frames']):
        assert rel(f['PSNR'], ref.psnr(int(ea[i]), n, 255.0)) <= 1e-12 and rel(f['PSNR_LQ'], ref.psnr(int(el[i]), n, 255.0)) <= 1e-12
        assert rel(f['dPSNR'], ref.dpsnr(int(ea[i]), int(el[i]))) <= 1e-12 and rel(f['dSSIM'], ssim[i] - ssim_lq[i]) <= 1e-12
    d = [f['dPSNR'] for f in doc['frames']]
    assert set(doc['by_slice']) == {'I', 'B', 'P'} and set(doc['by_qp']) == {'22.0', '27.0'}
    assert doc['by_slice']['B']['frames'] == 2 and doc['by_slice']['I']['frames'] == 1 and doc['by_qp']['22.0']['frames'] == 2
    assert rel(doc['by_slice']['B']['dPSNR'], (d[1] + d[3]) / 2) <= 1e-12 and rel(doc['by_slice']['P']['dPSNR'], d[2]) <= 1e-12
    assert rel(doc['by_qp']['22.0']['dPSNR'], (d[0] + d[2]) / 2) <= 1e-12 and rel(doc['by_qp']['27.0']['SSIM'], 0.75) <= 1e-12
    assert rel(doc['dPSNR'], sum(d) / 4) <= 1e-12
    # the class table: summed over the clip, the counts are the region's pixels and the errors the clip's
    table = doc['classes']
    assert [row['class'] for row in table] == list(range(8)) and all(set(row) == {'class', 'N', 'PSNR', 'PSNR_LQ', 'dPSNR'} for row in table)
    assert sum(row['N'] for row in table) == t * (h - 2 * crop) * (w - 2 * crop)
    want = ref.gain_classes(a, l, g, par, crop).sum(axis=0)
    assert sum(1 for k in range(8) if want[k, 0]) >= 5                  # the map's planes overlap: mixed classes
    for k, row in enumerate(table):
        assert row['N'] == int(want[k, 0])
        if want[k, 0]:
            assert rel(row['PSNR'], ref.psnr(int(want[k, 1]), 3.0 * int(want[k, 0]), 255.0)) <= 1e-12
            assert rel(row['dPSNR'], ref.dpsnr(int(want[k, 1]), int(want[k, 2]))) <= 1e-12
        else:
            assert row['dPSNR'] == 0.0 and row['PSNR'] == 'inf'
    # the grid: the cells' dPSNR with the frames summed
    cells = grid[:, 0].sum(axis=0)
    assert np.array(doc['grid']).shape == cells.shape[:2]
    for i in range(cells.shape[0]):
        for j in range(cells.shape[1]):
            assert rel(doc['grid'][i][j], ref.dpsnr(int(cells[i, j, 0]), int(cells[i, j, 1]))) <= 1e-12
    # without slices, QPs, classes or SSIM the report still stands
    bare = metrics.gain_report(grid[:, 0], counts, block=block)
    assert bare['classes'] is None and bare['by_slice'] == {} and bare['by_qp'] == {} and 'SSIM' not in bare['frames'][0]
    assert bare['frames'][0]['slice'] is None and bare['dPSNR'] == doc['dPSNR']


def test_forward_test_writes_the_report_of_a_clip(tmp_path):
    """psnr_only scores the input frames: the output IS lq, so the identity gain comes out of the whole host path, report included"""
    (a, l, g), _ = clips(3)
    from pnp_vcve_amd import restorer      # noqa: F401
    m = _model(metrics=['PSNR', 'dPSNR', 'PSNR_SD', 'PSNR_SD_LQ', 'dSSIM'], gain_report=str(tmp_path / 'gain'), gain_block=64)
    m.psnr_only = True
    par = torch.zeros(1, T, 3, H, W)
    par[:, :, 0, :32] = 1
    par[:, :, 1, 16:48] = 1
    sl = torch.tensor([73.0, 66.0, 80.0]).view(1, T, 1, 1, 1)
    qps = (torch.tensor([22.0, 27.0, 27.0]) / 255.0).view(1, T, 1, 1, 1)
    res = m.forward_test(l, g, QPs=qps, slices=sl, base_QPs=torch.full((1, T, 1, 1, 1), 25.0 / 255.0), par_map=par, meta=[dict(key='clipA/00000000')])
    ev = res['eval_result']
    assert ev['dPSNR'] == 0.0 and ev['dSSIM'] == 0.0 and ev['PSNR_SD'] == ev['PSNR_SD_LQ'] and ev['PSNR_SD'] > 0
    assert os.listdir(tmp_path / 'gain') == ['clipA.json']
    doc = json.load(open(tmp_path / 'gain' / 'clipA.json'))
    assert doc['clip'] == 'clipA' and doc['block'] == 64 and [f['slice'] for f in doc['frames']] == ['I', 'B', 'P']
    assert [f['qp'] for f in doc['frames']] == [22.0, 27.0, 27.0] and doc['frames'][0]['base_qp'] == 25.0
    assert all(f['dPSNR'] == 0.0 and f['dSSIM'] == 0.0 for f in doc['frames']) and doc['dPSNR'] == 0.0
    assert rel(sum(f['PSNR'] for f in doc['frames']) / T, ev['PSNR']) <= 1e-5
    assert [row['N'] for row in doc['classes']] == [T * (H - 48) * W, T * 16 * W, T * 16 * W, T * 16 * W, 0, 0, 0, 0]
    assert np.array(doc['grid']).shape == (2, 2) and not np.array(doc['grid']).any()
