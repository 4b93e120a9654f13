"""CPU tests of the host-side boundary: config loader, registry, metrics, checkpoint schema,
clip sharding and the world_size-2 metric all-gather (gloo)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configs_carry_the_reference_keys():
    from pnp_vcve_amd.config import Config
    from pnp_vcve_amd import synthetic as syn
    for name in ('HR_davis_LR_128x128.py', 'HR_davis_LR_128x128_IPB.py', 'HR_davis_LR_128x128_IPB_LR_test.py'):
        cfg = Config.fromfile(os.path.join(ROOT, 'configs', name))
        assert cfg.model.type == 'BasicVSR'
        g = dict(cfg.model.generator)
        assert g.pop('type') == 'IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par'
        assert g == syn.DEFAULT_GENERATOR_CFG                 # kwargs of configs/HR_davis_LR_128x128.py:8-24
        assert cfg.test_cfg.metrics == ['PSNR', 'SSIM'] and cfg.test_cfg.crop_border == 0
        assert cfg.dist_params.backend == 'nccl'
        assert cfg.data.test_dataloader.samples_per_gpu == 1
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'HR_davis_LR_128x128_IPB_LR_test.py'))
    assert (cfg.data.test.height, cfg.data.test.width, cfg.data.test.qp_mode) == (180, 320, 'ipb')   # _base_ chain
    cfg.merge_from_dict({'model.generator.vsr': True, 'data.test.num_clips': 2})
    assert cfg.model.generator.vsr is True and cfg.data.test.num_clips == 2 and cfg.model.generator.num_blocks == 8


def test_registry_builds_model_from_config():
    import pnp_vcve_amd  # noqa: F401
    from pnp_vcve_amd import restorer  # noqa: F401
    from pnp_vcve_amd.config import Config
    from pnp_vcve_amd.registry import MODELS, build_model
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'HR_davis_LR_128x128.py'))
    m = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(m).__name__ == 'BasicVSR'
    assert 'step_counter' in m.state_dict()                  # basicvsr.py:50
    assert any(k.startswith('generator.forward_resblocks.main.7.conv2.weight') for k in m.state_dict())
    with pytest.raises(KeyError):
        build_model(dict(type='NoSuchModel'))
    assert 'CharbonnierLoss' in MODELS


def test_checkpoint_round_trip_with_reference_prefixes(tmp_path):
    import pnp_vcve_amd  # noqa: F401
    from pnp_vcve_amd import restorer  # noqa: F401
    from pnp_vcve_amd import synthetic as syn
    from pnp_vcve_amd.checkpoint import load_checkpoint
    from pnp_vcve_amd.registry import build_backbone
    cfg = dict(syn.DEFAULT_GENERATOR_CFG, num_blocks=2)
    sd = {('generator.' + k): torch.from_numpy(v) for k, v in syn.make_state_dict(cfg, seed=3).items()}
    sd['step_counter'] = torch.zeros(1)
    f = str(tmp_path / 'ckpt.pth')
    torch.save({'meta': {}, 'state_dict': {('module.' + k): v for k, v in sd.items()}}, f)
    g = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    g.init_weights(pretrained=f, strict=True)
    assert torch.equal(g.state_dict()['conv_last.weight'], sd['generator.conv_last.weight'])
    with pytest.raises(TypeError):
        g.init_weights(pretrained=123)
    load_checkpoint(g, f, strict=False)


def test_psnr_ssim_definitions():
    from pnp_vcve_amd.metrics import psnr, ssim, tensor2img
    from oracle import cpu_ref
    a = torch.rand(1, 3, 40, 48)
    b = (a + 0.03 * torch.randn_like(a)).clamp(0, 1)
    ia, ib = tensor2img(a), tensor2img(b)
    assert ia.dtype == np.uint8 and ia.shape == (40, 48, 3)
    assert np.array_equal(ia, cpu_ref.tensor2img_uint8(a[0]))
    assert abs(psnr(ia, ib) - cpu_ref.psnr_uint8(ia, ib)) < 1e-9
    assert psnr(ia, ia) == float('inf')
    s = ssim(ia, ib)
    assert 0.5 < s < 1.0 and abs(ssim(ia, ia) - 1.0) < 1e-12
    # brute-force check of the 'valid' Gaussian window on one channel
    x, y = ia[..., 0].astype(np.float64), ib[..., 0].astype(np.float64)
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    win = np.outer(g, g)
    mu = sum(win[i, j] * x[i:i + 30, j:j + 38] for i in range(11) for j in range(11))
    from pnp_vcve_amd.metrics import _gauss_valid
    assert np.abs(_gauss_valid(x, g) - mu).max() < 1e-9


def test_sharding_rule_matches_reference_sampler():
    from pnp_vcve_amd.dist import shard_indices
    # reference: indices += indices[:total-n]; indices[rank::world]  (distributed_sampler.py:62-70)
    for n, world in ((8, 8), (10, 4), (4, 3), (100, 8)):
        per = -(-n // world)
        idx = list(range(n))
        idx += idx[:per * world - n]
        for r in range(world):
            assert shard_indices(n, r, world) == idx[r::world]
    with pytest.raises(ValueError):
        shard_indices(4, 0, 8)                               # distributed_sampler.py:45-49


WORKER = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, %r)
    import torch, torch.distributed as dist
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import SyntheticCompressedClipDataset
    dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))

    class Fake(torch.nn.Module):            # stands in for BasicVSR: the GPU path is covered by -m gpu tests
        last_forward_seconds = 0.5
        def forward(self, test_mode=False, lq=None, meta=None, **kw):
            clip = int(meta[0]['key'].split('/')[0])
            return dict(eval_result={'PSNR': 30.0 + clip, 'SSIM': 0.9 + clip / 1000.0})

    ds = SyntheticCompressedClipDataset(num_clips=5, num_input_frames=2, height=64, width=64)
    out = multi_gpu_test(Fake(), ds, device='cpu')
    assert len(out) == 5
    for i, o in enumerate(out):
        assert abs(o['eval_result']['PSNR'] - (30.0 + i)) < 1e-12, (i, o)
        assert abs(o['frames_per_s'] - 4.0) < 1e-12
    stats = ds.evaluate(out)
    assert abs(stats['PSNR'] - 32.0) < 1e-12
    dist.barrier()
    print('rank', dist.get_rank(), 'ok')
''')


def test_two_rank_clip_sharding_and_metric_all_gather_gloo(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % ROOT)
    port = 29600 + os.getpid() % 300
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert 'ok' in o


def _write_clip_tree(root, clips=('000', '011'), t=4, h=64, w=64, crf='crf25'):
    """a tiny dataset in the reference's on-disk layout (PNG frames, .npy MV records, JSON QP/slice table)."""
    import json
    from PIL import Image
    import golden_util as gu
    table = {crf: {}}
    slices = 'IBPB'[:t]
    for ci, clip in enumerate(clips):
        png = os.path.join(root, crf, 'png', clip)
        mv = os.path.join(root, crf, 'mv', clip)
        gt = os.path.join(root, 'X4', 'png', clip)
        for d in (png, mv, gt):
            os.makedirs(d)
        rec, rf, _, _, _ = gu.raster_case_inputs(dict(seed=900 + ci, h=h, w=w, slices=slices, per_frame=30))
        table[crf][clip] = {}
        rng = np.random.RandomState(ci)
        for f in range(t):
            img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(png, f'{f:08d}.png'))
            Image.fromarray(np.clip(img.astype(int) + rng.randint(-9, 10, img.shape), 0, 255).astype(np.uint8)).save(
                os.path.join(gt, f'{f:08d}.png'))
            np.save(os.path.join(mv, f'{f:08d}.npy'), rec[rf == f])
            table[crf][clip][str(f)] = {'slice': slices[f], 'QP': 22 + f}
    qp = os.path.join(root, 'qp.json')
    with open(qp, 'w') as fq:
        json.dump(table, fq)
    return os.path.join(root, crf, 'png'), os.path.join(root, 'X4', 'png'), qp, slices


def test_folder_dataset_reads_the_reference_layout(tmp_path):
    from pnp_vcve_amd.datasets import build_dataset
    import golden_util as gu
    lq, gt, qp, slices = _write_clip_tree(str(tmp_path))
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1,
                            val_partition='REDS4', test_mode=True))
    assert len(ds) == 2
    item = ds[1]
    assert item['lq'].shape == (4, 3, 64, 64) and item['gt'].shape == (4, 3, 64, 64)
    assert [chr(int(v)) for v in item['slices'].reshape(-1)] == list(slices)
    assert torch.allclose(item['QPs'].reshape(-1), torch.tensor([22., 23., 24., 25.]) / 255.0)
    assert torch.allclose(item['base_QPs'].reshape(-1), torch.full((4,), 25 / 255.0))
    rec, rf, _, _, _ = gu.raster_case_inputs(dict(seed=901, h=64, w=64, slices=slices, per_frame=30))
    assert np.array_equal(item['mv_records'].numpy(), rec) and np.array_equal(item['rec_frame'].numpy(), rf)
    assert item['meta']['key'].startswith('011/')


def test_clip_prefetcher_preserves_order_and_surfaces_errors():
    from pnp_vcve_amd.apis import ClipPrefetcher
    from pnp_vcve_amd.datasets import SyntheticCompressedClipDataset
    ds = SyntheticCompressedClipDataset(num_clips=4, num_input_frames=2, height=64, width=64)
    keys = [d['meta'][0]['key'] for d in ClipPrefetcher(ds, [2, 0, 3], 'cpu')]
    assert [k.split('/')[0] for k in keys] == ['002', '000', '003']

    class Bad(SyntheticCompressedClipDataset):
        def __getitem__(self, i):
            raise OSError('disk gone')
    with pytest.raises(OSError):
        list(ClipPrefetcher(Bad(num_clips=2), [0], 'cpu'))


def test_wrap_fp16_model_flips_only_modules_that_carry_the_switch():
    """mmcv.runner.wrap_fp16_model semantics (basic_restorer.py:45-46): set fp16_enabled where it exists."""
    import torch.nn as nn
    from pnp_vcve_amd.restorer import wrap_fp16_model

    class WithSwitch(nn.Module):
        def __init__(self):
            super().__init__()
            self.fp16_enabled = False

    class Plain(nn.Module):
        pass

    m = nn.Sequential(WithSwitch(), Plain(), nn.Sequential(WithSwitch()))
    wrap_fp16_model(m)
    assert m[0].fp16_enabled is True and m[2][0].fp16_enabled is True
    assert not hasattr(m[1], 'fp16_enabled')


def test_async_frame_writer_matches_tensor2img_and_surfaces_errors(tmp_path):
    """io_async: uint8 conversion == the reference's tensor2img (core/misc.py:51-71) incl. clamping and round-half-even
    ties; files written by the pool are pixel-identical to a synchronous save; a failed write is raised by close()."""
    import numpy as np
    from PIL import Image
    from pnp_vcve_amd.io_async import FrameWriter, frames_to_uint8_hwc
    from pnp_vcve_amd.metrics import tensor2img
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, 20, 24, generator=g) * 1.2 - 0.1            # some values outside [0, 1]
    x[0, 0, 0, :8] = torch.tensor([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 253.5, 254.5]) / 255.0      # exact ties
    q = frames_to_uint8_hwc(x)
    assert q.shape == (3, 20, 24, 3) and q.dtype == np.uint8
    for i in range(3):
        ref = tensor2img(x[i])[..., ::-1]                              # BGR (cv2 convention) -> RGB
        assert np.array_equal(q[i], ref)
    with FrameWriter(max_workers=3) as w:
        for i in range(3):
            w.submit(str(tmp_path / 'clip' / f'{i:08d}.png'), q[i])
    for i in range(3):
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'clip' / f'{i:08d}.png')), q[i])
    blocker = tmp_path / 'file'
    blocker.write_text('x')
    w = FrameWriter(max_workers=1)
    w.submit(str(blocker / 'sub' / 'a.png'), q[0])                     # parent is a file: makedirs fails in the worker
    with pytest.raises(OSError):
        w.close()


def test_torch_custom_ops_are_registered_with_fake_kernels():
    """torch.ops.pnpvcve.*: schemas exist and the fake (meta) kernels propagate shapes without a GPU."""
    import pnp_vcve_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ('flow_warp', 'mv_warp', 'psnr_sse', 'generator_forward', 'conv3x3', 'expert_mix', 'bae_block',
                 'pixel_shuffle_conv'):                       # SURVEY 8(b)'s op list
        assert hasattr(torch.ops.pnpvcve, name), name
    assert 'Tensor x, Tensor flow' in str(torch.ops.pnpvcve.flow_warp.default._schema)
    with FakeTensorMode():
        x = torch.empty(2, 8, 64, 96)
        assert torch.ops.pnpvcve.flow_warp(x, torch.empty(2, 64, 96, 2)).shape == x.shape
        f = torch.empty(64, 96, 64)
        assert torch.ops.pnpvcve.mv_warp(f, torch.empty(64, 96), torch.empty(64, 96)).shape == f.shape
        lrs = torch.empty(1, 3, 3, 64, 64)
        out = torch.ops.pnpvcve.generator_forward(0, lrs, torch.empty(1, 3, 4, 64, 64), torch.empty(1, 3, 3, 64, 64),
                                                  torch.empty(3, 1, 3))
        assert out.shape == (1, 3, 3, 64, 64)
        pw = torch.empty(9 * 4096)
        assert torch.ops.pnpvcve.conv3x3([f, f], [pw, pw], None, None, None, None, None, 2).shape == (64, 96, 64)
        assert torch.ops.pnpvcve.expert_mix(torch.empty(6, 64, 64, 3, 3), torch.empty(6)).shape == (9 * 4096,)
        assert torch.ops.pnpvcve.bae_block(f, pw, None, None, None, None, pw, None).shape == f.shape
        assert torch.ops.pnpvcve.pixel_shuffle_conv(f, torch.empty(4 * 9 * 4096 + 256), 2).shape == (128, 192, 64)


def test_bench_gpus_n_spawns_ranks_and_propagates_their_failure():
    """`python bench.py --gpus 2` with no torch.distributed environment launches the ranks as child processes before
    touching the GPU.  Without a GPU the ranks cannot run: the launcher must come back non-zero (the children's status)
    instead of silently measuring one rank."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip('CPU-only check (the GPU variant lives in tests/test_gpu_restorer.py)')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env['PNP_DIST_BACKEND'] = 'gloo'
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--workload', '128', '--steps', '1',
                          '--warmup', '0'], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert 'torch.distributed' in out.stderr or 'ChildFailedError' in out.stderr or 'rank' in out.stderr.lower()


def test_bench_cpu_baseline_for_the_128_workload_states_cores_as_numbers():
    """bench.py's CPU leg beside the 7x3x128x128 entries (north_star: "alongside the reference CPU path timed on the host
    cores (core count stated)"): the oracle, median of 5, thread and logical-CPU counts as numeric fields."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    c = bench.cpu_baseline_128(2)           # 2 frames keep the CPU suite short; bench.py passes T = 7
    assert c['kind'] == 'port' and c['unit'] == 'frames/s' and c['value'] > 0
    assert isinstance(c['threads'], int) and c['cores'] == c['threads'] and 1 <= c['threads'] <= c['host_logical_cpus']
    assert len(c['seconds_per_clip_runs']) == 5
    assert abs(c['value'] - 2 / c['seconds_per_clip_median']) < 1e-9


def _ssim_scipy(img1, img2, crop_border=0):
    """The reference formula (mmedit/core/evaluation/metrics.py:266-355) restated with scipy.ndimage, independently of
    pnp_vcve_amd.metrics: cv2.filter2D(img, -1, window) is a correlation with BORDER_REFLECT_101 (= scipy 'mirror'),
    cropped [5:-5, 5:-5]; cv2.getGaussianKernel(11, 1.5) = normalised exp(-(i-5)^2 / (2 * 1.5^2))."""
    from scipy import ndimage
    k = np.exp(-((np.arange(11) - 5) ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()
    window = np.outer(k, k)
    if crop_border != 0:                    # :343-345 -- (H', W', 1, 3): the loop below then sees channel 0 only
        img1 = img1[crop_border:-crop_border, crop_border:-crop_border, None]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, None]
    vals = []
    for i in range(img1.shape[2]):
        a = img1[..., i].astype(np.float64)
        b = img2[..., i].astype(np.float64)
        if a.ndim == 3:                     # (H', W', 1) after the crop: cv2 filters it as a 1-channel image
            a, b = a[..., 0], b[..., 0]
        f = lambda x: ndimage.correlate(x, window, mode='mirror')[5:-5, 5:-5]       # noqa: E731
        C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        mu1, mu2 = f(a), f(b)
        s1, s2, s12 = f(a ** 2) - mu1 ** 2, f(b ** 2) - mu2 ** 2, f(a * b) - mu1 * mu2
        m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
        vals.append(m.mean())
    return float(np.array(vals).mean())


@pytest.mark.parametrize('crop', [0, 3])
def test_ssim_against_independent_scipy_restatement(crop):
    """pnp_vcve_amd.metrics.ssim (the host definition the GPU kernel is tested against) vs a scipy.ndimage
    restatement of the reference's cv2 formula that shares no code with it."""
    from pnp_vcve_amd.metrics import ssim, tensor2img
    rng = np.random.RandomState(5)
    for hw in ((40, 48), (33, 61)):
        a = torch.from_numpy(rng.rand(1, 3, *hw).astype(np.float32))
        b = (a + 0.05 * torch.from_numpy(rng.randn(1, 3, *hw).astype(np.float32))).clamp(0, 1)
        ia, ib = tensor2img(a), tensor2img(b)
        ref = _ssim_scipy(ia, ib, crop)
        assert abs(ssim(ia, ib, crop) - ref) < 1e-12, (hw, crop)
    if crop:                                  # the quirk is visible: all-channel SSIM differs
        assert abs(_ssim_scipy(ia[crop:-crop, crop:-crop], ib[crop:-crop, crop:-crop], 0) - ref) > 1e-6


def _load_bench():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_line_is_bounded_and_strict_json():
    """bench.py's stdout contract (round 3's 21 KB line with nine inlined `secondary` entries was truncated by the driver and never
    parsed): whatever the result object holds -- prose definitions, NaN / inf, eight per-rank entries -- the line is one strict-JSON
    object of at most 4 KB with value / roofline / cpu_baseline intact."""
    import json
    from bench_util import MAX_LINE_BYTES
    bench = _load_bench()
    prose = 'x' * 1500
    roof = {'kernel': 'conv3x3_persist_kernel<PAR> (' + prose + ')', 'bound': 'mfma', 'achieved': 125.26916303185266, 'peak': 157.3,
            'unit': 'TFLOP/s', 'frac': 0.7963710300817078, 'traffic': 686521221.7258297, 'definition': prose, 'note': prose,
            'device_ms_per_step': {'conv_block': 135.9, 'dcn': float('nan')}, 'launches': 693, 'avg_launch_us': 588.42}
    res = {'metric': 'enhanced frames/sec (1280x720, 7-frame window)', 'value': 45.87263935306233, 'unit': 'frames/s', 'n_gpus': 8,
           'steps': 20, 'warmup': 5, 'ms_per_step': 152.59640820149798, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
           'dtype': 'f32', 'data': 'synthetic', 'config': {'workload': 'w' * 400}, 'roofline': roof,
           'roofline_mv_warp': dict(roof, bound='hbm', algorithmic_bytes_per_launch=479232000.0),
           'cpu_baseline': {'value': 0.057, 'unit': 'frames/s', 'cores': 16, 'kind': 'port', 'sample': 's' * 400},
           'parity': {'max_abs_diff_vs_cpu': 1.3e-7, 'psnr_delta_db': float('inf'), 'gate': 1e-3},
           'psnr_per_rank': [30.0 + i / 7 for i in range(8)], 'frames_per_s_per_rank': [float('nan')] + [45.5] * 7,
           'north_star_128': {'clips_1': 1710.123456789, 'cpu': 21.7}}
    line = bench.bounded_line(res)
    assert len(line.encode()) <= MAX_LINE_BYTES and '\n' not in line
    d = json.loads(line, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    assert d['value'] == 45.8726 and d['roofline']['frac'] == 0.796371 and d['roofline']['kernel'] == 'conv3x3_persist_kernel<PAR>'
    assert 'definition' not in d['roofline'] and 'note' not in d['roofline'] and 'device_ms_per_step' not in d['roofline']
    assert d['roofline_mv_warp']['algorithmic_bytes_per_launch'] == 479232000      # integral floats stay exact integers
    assert d['parity']['psnr_delta_db'] is None and d['frames_per_s_per_rank'][0] is None and len(d['psnr_per_rank']) == 8
    assert d['cpu_baseline']['cores'] == 16 and d['n_gpus'] == 8
    # too long even when compacted: optional blocks go first, the contract keys never; a line that cannot fit raises
    res['north_star_128'] = {f'k{i}': 'y' * 100 for i in range(30)}
    d2 = json.loads(bench.bounded_line(res))
    assert 'north_star_128' not in d2 and d2['roofline']['frac'] == 0.796371 and 'cpu_baseline' in d2
    res['config'] = {'workload': 'w' * 5000}
    with pytest.raises(RuntimeError):
        bench.bounded_line(res)


def test_bench_steps_and_full_options():
    """--steps is the number of timed steps (at least one), --full is off unless asked for, --dump-outputs takes a directory"""
    bench = _load_bench()
    a = bench.parse_args(['--steps', '7', '--warmup', '0'])
    assert a.steps == 7 and a.warmup == 0 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(['--full', '--dump-outputs', 'x'])
    assert a.full is True and a.dump_outputs == 'x'
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_bench_dump_outputs_writes_float32_whole_or_as_a_fixed_sample(tmp_path):
    """--dump-outputs: an output up to DUMP_MAX_BYTES is written whole; a larger one (a 720p clip is 77 MB) as DUMP_SAMPLE
    elements at seeded positions, the same on every run, and a file of an earlier run does not linger beside it"""
    bench = _load_bench()
    small = torch.arange(2 * 3 * 8 * 8, dtype=torch.float32).reshape(1, 2, 3, 8, 8)
    bench.dump_outputs(small, str(tmp_path))
    got = np.load(tmp_path / 'output.npy')
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())
    big = torch.from_numpy(np.random.RandomState(3).rand(bench.DUMP_MAX_BYTES // 4 + 1).astype(np.float32))
    bench.dump_outputs(big, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['output_sample.npy']
    s1 = np.load(tmp_path / 'output_sample.npy')
    assert s1.dtype == np.float32 and s1.shape == (bench.DUMP_SAMPLE,) and s1.nbytes <= 64 << 20
    assert np.isin(s1, big.numpy()).all()
    bench.dump_outputs(big.clone(), str(tmp_path))
    assert np.array_equal(np.load(tmp_path / 'output_sample.npy'), s1)


BENCH_RANK = textwrap.dedent('''
    import importlib.util, os, sys, time
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(%r, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def stub_measure(dev, sd_np, cfg, *, steps, T, clips, rank, world, dist, cdev, **kw):
        # the GPU forward is covered by -m gpu tests; here a step is a sleep that grows with the rank, and the REAL timed region
        # (barrier, steps, barrier, all_reduce(MAX)) runs around it
        assert dist is not None and cdev.type == 'cpu'
        _, elapsed, emax = bench.timed_steps(lambda: time.sleep(0.01 * (rank + 1)), steps, dist, cdev)
        frames = steps * T * clips
        return ({'value': world * frames / emax, 'ms_per_step': 1e3 * emax / steps, 'elapsed_rank': elapsed,
                 'psnr_rank': 30.0 + rank, 'frames_per_s_rank': frames / elapsed, 'kernel_events': 'none',
                 'launches_per_frame': None}, None, None)

    bench.main(sys.argv[1:], measure_fn=stub_measure)
''')


def test_bench_eight_rank_path_over_gloo_prints_one_bounded_line(tmp_path):
    """The driver's N = 8 form (`python -m torch.distributed.run --nproc-per-node 8 bench.py --gpus 8 ...`) on CPU: eight gloo ranks
    run bench.main() with the GPU forward stubbed out -- process group, barrier-bracketed timed region, MAX over ranks, all_gather
    of the per-rank metrics, rank 0's ONE line: under 4 KB, strict JSON, eight per-rank entries, whole-job arithmetic
    (tools/dist_test.sh:11-22, mmedit/apis/test.py:211-233).  The real forward at 8 ranks is a -m gpu test."""
    from bench_util import bench_line
    script = tmp_path / 'bench_rank.py'
    script.write_text(BENCH_RANK % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env.update(PNP_DIST_BACKEND='gloo', OMP_NUM_THREADS='1')
    port = 29900 + os.getpid() % 90
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=8', '--master-addr',
                          '127.0.0.1', '--master-port', str(port), str(script), '--gpus', '8', '--workload', '128', '--frames', '3',
                          '--steps', '2', '--warmup', '1', '--no-kernel-events', '--full'], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    d = bench_line(out.stdout)          # clean: bench.py points fd 1 at stderr, so even gloo's connection lines stay off stdout
    assert d['n_gpus'] == 8 and d['scaling'] == 'weak' and d['config']['parallelism'] == 'clip-sharded replicas x8'
    assert d['psnr_per_rank'] == [30.0 + r for r in range(8)] and len(d['frames_per_s_per_rank']) == 8
    assert d['dist'] == {'process_group': True, 'backend': 'gloo', 'rccl_version': None,
                         'collectives': ['barrier', 'all_reduce(MAX)', 'all_gather', 'barrier']}
    # whole-job rate = all ranks' frames over the SLOWEST rank's time (rank 7 sleeps 80 ms per step)
    assert abs(d['value'] - 8 * 2 * 3 / (d['ms_per_step'] * 2e-3)) < 1e-4 * d['value'] and d['ms_per_step'] >= 80.0
    # the N > 1 line is complete under SURVEY 8d: rank 0 timed the oracle (128x128 clip) after the timed region
    cb = d['cpu_baseline']
    assert cb['kind'] == 'port' and cb['unit'] == 'frames/s' and cb['value'] > 0 and isinstance(cb['cores'], int) and cb['cores'] >= 1
    assert '128x128' in cb['sample'] and 'north_star_128' not in d


def test_tools_test_rejects_contradictory_precision_switches():
    """tools/test.py: --fp16 IS --precision fp16; a contradiction is an error before anything is built, not "the last one wins"."""
    cfgp = os.path.join(ROOT, 'configs', 'HR_davis_LR_128x128_IPB.py')
    for flags in (['--fp16', '--precision', 'fp32'], ['--fp16', '--precision', 'f16x3'],
                  ['--cfg-options', 'fp16.loss_scale=1', 'precision=f16x3']):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfgp, 'none'] + flags,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and ('contradicts' in out.stderr or 'the config sets' in out.stderr), out.stderr[-500:]


def test_folder_dataset_decode_pool_survives_pickling_and_is_per_process(tmp_path):
    """CompressedClipFolderDataset: the cached thread pool must not make the dataset unpicklable (spawn DataLoader workers) and
    must not be reused in a forked child, where its threads do not exist."""
    import pickle
    from pnp_vcve_amd.datasets import build_dataset
    lq, gt, qp, _ = _write_clip_tree(str(tmp_path))
    ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                            pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1,
                            val_partition='REDS4', test_mode=True))
    a = ds[0]                                    # creates the pool
    assert ds._decode_pool[0] == os.getpid()
    ds2 = pickle.loads(pickle.dumps(ds))
    assert not hasattr(ds2, '_decode_pool') and torch.equal(ds2[0]['lq'], a['lq'])
    ds._decode_pool = (ds._decode_pool[0] + 1, ds._decode_pool[1])      # as seen from a forked child: another pid
    assert torch.equal(ds[0]['lq'], a['lq']) and ds._decode_pool[0] == os.getpid()


def test_roofline_traffic_counts_exactly_the_block_conv_launches_of_the_committed_profile():
    """bench.py's roofline.traffic: launch-weighted (2 x FETCH + WRITE) over conv3x3_wino_kernel<PAR,RES,MS,FO> with MS = false (plain =
    conv_hr, RES = back halves, FO = fold-only front halves) -- not the multi-source input conv, not the 336 gated returns of the
    branch kernel (21 KB each).  r05's committed PMC passes: (21 x 596.5 + 336 x 618.6 + 336 x 952.3) / 693 = 779.7 MB per launch against
    591.6 MB algorithmic (round 5's line said 539.7: the filter predated the fourth template flag)."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, 'profiles', 'r05_pmc.json')) as fh:
        pmc = json.load(fh)
    t = bench._launch_weighted_traffic(pmc, 'conv3x3_wino_kernel', min_bytes=0.01 * 512 * 720 * 1280)
    by_hand = (21 * 596475739.4 + 336 * 618621092.6 + 336 * 952330097.9) / 693
    assert abs(t - by_hand) < 1.0 and abs(t / 1e6 - 779.7) < 0.1
    alg = bench.block_conv_algorithmic_bytes(720, 1280, 8)
    assert abs(alg / 1e6 - 591.6) < 0.1 and abs(t / alg - 1.318) < 0.002
    assert bench._wino_flags('conv3x3_wino_kernel<false, true, false, true>') == (False, True, False, True)
    assert bench._wino_flags('conv3x3_wino_quad_kernel<false,true>') is None
    # round 6's committed passes (front halves are conv3x3_wino_gated_kernel launches there): 677 MB = 1.14x -- the spill traffic is gone
    with open(os.path.join(ROOT, 'profiles', 'r06_pmc.json')) as fh:
        p6 = json.load(fh)
    t6 = bench._launch_weighted_traffic(p6, 'conv3x3_wino_kernel', min_bytes=0.01 * 512 * 720 * 1280)
    assert sum(v['launches'] for k, v in p6.items() if bench._wino_flags(k) and not bench._wino_flags(k)[2]) == 693
    assert 1.10 < t6 / alg < 1.18 and bench.committed_pmc_traffic('')[1] >= 'profiles/r06_pmc.json'
    assert bench._wino_flags('conv3x3_wino_gated_kernel<true>') == (None, True, False, None)        # r06: one launch per gated front half
    assert abs(bench._launch_weighted_traffic({'conv3x3_wino_gated_kernel<false>': {'hbm_bytes_per_launch': 5e8, 'launches': 3},
                                               'conv3x3_wino_kernel<false,false,true,false>': {'hbm_bytes_per_launch': 9e8, 'launches': 1}},
                                              'conv3x3_wino_kernel') - 5e8) < 1
    # without the floor the gated returns dilute the mean; the input conv never enters
    assert bench._launch_weighted_traffic(pmc, 'conv3x3_wino_kernel') < t
    assert 'traffic_ratio' in bench.ROOFLINE_KEEP and 'algorithmic_bytes_per_launch' in bench.ROOFLINE_KEEP


def test_winograd_routing_rule_is_stated_once():
    """PNP_OPT_WINOGRAD = 1: quadrant units up to PNP_WINO_UNITS_MAX_TILES 16x16 tiles, tile kernels above (include/pnpvcve.h);
    _native.wino_kernel_form is that rule for bench.py, generator.hip uses the header's constant"""
    import re
    from pnp_vcve_amd import _native
    hdr = open(os.path.join(ROOT, 'include', 'pnpvcve.h')).read()
    assert int(re.search(r'#define PNP_WINO_UNITS_MAX_TILES (\d+)', hdr).group(1)) == _native.WINO_UNITS_MAX_TILES
    src = open(os.path.join(ROOT, 'pnp_vcve_amd', 'csrc', 'generator.hip')).read()
    assert 'ntiles16(hh, ww) <= PNP_WINO_UNITS_MAX_TILES' in src and '< 512' not in hdr
    assert _native.wino_kernel_form(128, 128, 1) == 'units' and _native.wino_kernel_form(128, 128, 2) == 'tiles'
    assert _native.wino_kernel_form(180, 320, 1) == 'tiles' and _native.wino_kernel_form(720, 1280, 0) is None
    assert _native.wino_kernel_form(128, 256, 1) == 'units' and _native.wino_kernel_form(128, 272, 1) == 'tiles'
