"""GPU: the bounded-memory forward (generator.max_resident_features, pnp_generator_set_max_resident) recomputes backward features
from checkpoints and must give the unbounded forward's output bit for bit, in every configuration, precision and kernel form, with a
peak device memory that follows workspace_bytes(k)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from pnp_vcve_amd import _native

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-6          # tests/test_gpu_generator.py's golden gate

TWO_KEYS_24 = [73] + [66] * 11 + [80] + [66] * 11


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def build(cfg, sd_np):
    from pnp_vcve_amd.registry import build_backbone
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m.to(dev()).eval()


def run(m, clip):
    a = {k: torch.from_numpy(v).to(dev()) if isinstance(v, np.ndarray) else v for k, v in clip.items()}
    with torch.no_grad():
        return m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])


def _mirror(clip):
    t = clip['lq'].shape[1]
    for i in range(t // 2):
        clip['lq'][:, t - 1 - i] = clip['lq'][:, i]
    return clip


def _bounded_vs_unbounded(cfg_over, t, slices, h=64, w=96, n=1, precision='fp32', wino=None, ks=('min',), graphs=False,
                          mirror=False, seed=0):
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG)
    cfg.update(cfg_over)
    m = build(cfg, gu.syn.make_state_dict(cfg, seed=300 + seed, par_gain=10.0))
    if precision != 'fp32':
        m.precision = precision
    if wino is not None:
        m.set_option(_native.OPT_WINOGRAD, wino)
    clip = gu.syn.make_clip(seed=400 + seed, n=n, t=t, h=h, w=w, slices=slices, qp_mode='qp',
                            crf=[15, 35][:n] if n > 1 else 25)
    if mirror:
        clip = _mirror(clip)
    m.use_graphs = graphs
    ref = run(m, clip).clone()
    kmin = m.min_resident_features(t)
    assert 1 <= kmin <= t
    for k in ks:
        m.max_resident_features = kmin if k == 'min' else (kmin + k if isinstance(k, int) else None)
        out = run(m, clip)
        if graphs:
            out = run(m, clip)              # the replay, not the eager warm-up of the capture
        assert torch.equal(out, ref), (cfg_over, t, slices, precision, wino, k, float((out - ref).abs().max()))
    return m


# (config overrides, t, slices, extra kwargs)
CASES = [
    ('ibbbp_t11', {}, 11, 'IBBBP', dict(ks=('min', 2, 'none'))),
    ('allB_t9', {}, 9, 'allB', {}),
    ('allP_t9', {}, 9, 'allP', {}),
    ('two_keys_t24', {}, 24, TWO_KEYS_24, {}),
    ('mirror_t8', {}, 8, [73, 66, 80, 66, 66, 80, 66, 73], dict(mirror=True)),
    ('mirror_t24', {}, 24, 'IBBBP', dict(mirror=True)),
    ('nocat_t13', dict(with_cat=False), 13, 'IBBBP', {}),
    ('noalign_t13', dict(align_key=False), 13, 'allP', {}),
    ('vsr_t9', dict(vsr=True, num_blocks=2), 9, 'IBBBP', {}),
    ('basic_t9', dict(deform='basic', num_blocks=2), 9, 'IBBBP', {}),
    ('sparse_val_t9', dict(sparse_val=True), 9, 'IBBBP', {}),
    ('fp16_t11', {}, 11, 'IBBBP', dict(precision='fp16')),
    ('f16x3_t11', {}, 11, 'IBBBP', dict(precision='f16x3')),
    ('fp16_vsr_t9', dict(vsr=True, num_blocks=2), 9, 'allB', dict(precision='fp16')),
    ('wino0_t11', {}, 11, 'IBBBP', dict(wino=0)),
    ('wino1_t11', {}, 11, 'IBBBP', dict(wino=1)),
    ('wino2_t11', {}, 11, 'IBBBP', dict(wino=2)),
    ('wino2_sparse_t9', dict(sparse_val=True), 9, 'allB', dict(wino=2)),
    ('n2_two_contexts_t9', {}, 9, 'IBBBP', dict(n=2)),
    ('f16x3_n2_t9', {}, 9, 'allP', dict(n=2, precision='f16x3')),
    ('graphs_t9', {}, 9, 'IBBBP', dict(graphs=True)),
    ('graphs_fp16_n2_t9', {}, 9, 'IBBBP', dict(graphs=True, n=2, precision='fp16')),
    ('s128x128_t11', {}, 11, 'IBBBP', dict(h=128, w=128)),
    ('s180x320_t11', {}, 11, 'IBBBP', dict(h=180, w=320)),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_bounded_forward_is_bit_identical(case):
    name, cfg_over, t, slices, kw = case
    _bounded_vs_unbounded(cfg_over, t, slices, seed=CASES.index(case), **kw)


def test_720p_t24_at_the_minimum_is_bit_identical():
    _bounded_vs_unbounded({}, 24, 'IBBBP', h=720, w=1280, seed=99)


@pytest.mark.parametrize('name', ['gen_t7_128x128', 'gen_t9_two_keys_64x64', 'gen_t8_mirror_64x64'])
def test_goldens_at_the_minimum(name):
    case = next(c for c in gu.GEN_CASES if c['name'] == name)
    cfg, sd_np, clip = gu.gen_case_inputs(case)
    m = build(cfg, sd_np)
    t = clip['lq'].shape[1]
    m.max_resident_features = m.min_resident_features(t)
    assert m.max_resident_features < t
    out = run(m, clip).cpu().numpy()
    ref = gu.load_golden(name)['out']
    d = float(np.abs(out - ref).max())
    print(name, 'k =', m.max_resident_features, 'max|hip - reference| =', d)
    assert d < TOL


def test_a_bound_below_the_minimum_raises():
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG)
    m = build(cfg, gu.syn.make_state_dict(cfg, seed=1))
    clip = gu.syn.make_clip(seed=2, n=1, t=9, h=64, w=64, slices='IBBBP')
    m.max_resident_features = m.min_resident_features(9) - 1
    with pytest.raises(ValueError, match=f'minimum {m.min_resident_features(9)}'):
        run(m, clip)


def test_peak_memory_follows_the_bound():
    """360x640, t = 200, fp32: the bounded forward's peak is its inputs + output + workspace_bytes(k) + 256 MB at most, and less
    than half the unbounded one's."""
    cfg = dict(gu.syn.DEFAULT_GENERATOR_CFG)
    m = build(cfg, gu.syn.make_state_dict(cfg, seed=3, par_gain=10.0))
    t, h, w = 200, 360, 640
    g = torch.Generator(device='cuda').manual_seed(5)
    c = dict(lq=torch.rand(1, t, 3, h, w, device='cuda', generator=g),
             mvs=((torch.randint(-16, 17, (1, t, 4, h // 8, w // 8), device='cuda', generator=g).float() / 4)
                  .repeat_interleave(8, 3).repeat_interleave(8, 4).contiguous()),
             partitions=torch.zeros(1, t, 3, h, w, device='cuda'),
             slices=torch.tensor([73.0 if i == 0 else (80.0 if i % 4 == 0 else 66.0) for i in range(t)], device='cuda').view(1, t, 1, 1, 1),
             QPs=torch.full((1, t, 1, 1, 1), 28 / 255.0, device='cuda'), base_QPs=torch.full((1, t, 1, 1, 1), 25 / 255.0, device='cuda'))
    L = _native.lib()
    kmin = m.min_resident_features(t)
    peaks, outs, ws = {}, {}, {}
    for k in (kmin, None):
        m.max_resident_features = k             # (drops the cached workspace of the previous setting)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        outs[k] = run(m, c)
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated() - base
        ws[k] = int(L.pnp_generator_workspace_bytes(m._handle, t, h, w))
        print(f'k = {k}: peak above the inputs {peaks[k] / 1e9:.2f} GB, workspace {ws[k] / 1e9:.2f} GB')
    assert peaks[kmin] <= outs[kmin].numel() * 4 + ws[kmin] + (256 << 20), (peaks, ws)
    assert torch.equal(outs[kmin], outs[None])
    inputs = sum(v.numel() * 4 for v in c.values())
    assert peaks[kmin] + inputs < 0.5 * (peaks[None] + inputs), (peaks, inputs)


def test_test_driver_flag_gives_the_same_metrics_digit_for_digit():
    """tools/test.py --max-resident-features K: the same PSNR / SSIM lines, digit for digit, as the run without the flag (9-frame
    synthetic clips, K = 6 < 9: two recomputed segments per clip)."""
    common = ['--seed', '0', '--cfg-options', 'data.test.num_clips=2', 'data.test.num_input_frames=9', 'data.test.height=64',
              'data.test.width=64']
    res = []
    for extra in ([], ['--max-resident-features', '6']):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'),
                              os.path.join(ROOT, 'configs', 'HR_davis_LR_128x128_IPB.py'), 'none'] + common + extra,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        res.append((re.search(r'Eval-PSNR: (\S+)', out.stdout).group(1), re.search(r'Eval-SSIM: (\S+)', out.stdout).group(1)))
    assert res[0] == res[1], res
