#!/usr/bin/env python
"""Evaluation driver with the reference's CLI (tools/test.py:18-61 of ZeldaM1/PnP-VCVE):
    python tools/test.py CONFIG CHECKPOINT [--launcher pytorch] [--save-path DIR] [--cfg-options k=v ...]
CHECKPOINT may be 'none' (seeded random weights: released checkpoints are not available offline)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pnp_vcve_amd  # noqa: E402,F401
from pnp_vcve_amd import restorer  # noqa: E402,F401
from pnp_vcve_amd.apis import multi_gpu_test  # noqa: E402
from pnp_vcve_amd.checkpoint import load_checkpoint  # noqa: E402
from pnp_vcve_amd.config import Config, parse_cfg_options  # noqa: E402
from pnp_vcve_amd.datasets import build_dataset  # noqa: E402
from pnp_vcve_amd.dist import get_dist_info, init_dist  # noqa: E402
from pnp_vcve_amd.registry import build_model  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description='PnP-VCVE hot-path tester (MI355X)')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--deterministic', action='store_true')
    p.add_argument('--out')
    p.add_argument('--gpu-collect', action='store_true', help='accepted for CLI parity; collection is always on-GPU')
    p.add_argument('--testdir_lr', default=None)
    p.add_argument('--testdir_gt', default=None)
    p.add_argument('--save-path', default=None, type=str)
    p.add_argument('--tmpdir')
    p.add_argument('--cfg-options', nargs='+', default=None)
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none')
    p.add_argument('--fp16', action='store_true',
                   help='fp16 MFMA operands for the 64-channel convs (same as `fp16 = dict()` in the config); default fp32')
    p.add_argument('--precision', choices=['fp32', 'fp16', 'f16x3'], default=None,
                   help="arithmetic of the 64-channel convs: fp32 (exact, default), fp16 (= --fp16), f16x3 (split fp16: fp32-level "
                        "results from three fp16 MFMAs per product, ~2.2x the fp32 rate); also `precision = '...'` in the config")
    p.add_argument('--clips-in-flight', type=int, default=2, choices=[1, 2],
                   help='2 (default): two clips of equal shape go through the generator as one batch, interleaved on two streams '
                        '(+5 % at 720p, bit-identical, a second workspace); 1: strictly one clip per forward like the reference')
    p.add_argument('--max-resident-features', type=int, default=None, metavar='K',
                   help='bound the frame feature maps the generator holds to K (long clips: the backward features are recomputed '
                        'from checkpoints, bit-identical output, a workspace of K maps instead of one per frame); default unbounded')
    p.add_argument('--byte-frames', action='store_true',
                   help='keep the frames uint8 from the decoder into the generator and take its output as display bytes for the PNGs '
                        '(fp32 planes only for the metrics); a pair of clips goes in by pointer instead of concatenated.  Same '
                        'metrics and PNG bytes; default off')
    p.add_argument('--byte-metrics', action='store_true',
                   help='implies --byte-frames; PSNR / SSIM / MS-SSIM / PSNR-B read bytes too: the ground truth stays uint8 on the device and the generator '
                        'writes display bytes only, with or without --save-path (6 B per pixel into the metrics instead of 24).  Same '
                        'metrics; default off')
    p.add_argument('--yuv-frames', action='store_true',
                   help='raw 4:2:0 evaluation (a Yuv420ClipFolderDataset of .yuv clips): the generator reads the planes and writes packed '
                        '4:2:0 only, the ground truth stays 8-bit planes on the device, PSNR / SSIM are the Y plane\'s (PSNR_U, PSNR_V, '
                        'SSIM_U, SSIM_V, the 6:1:1 PSNR_YUV, MS-SSIM, MS-SSIM_U, MS-SSIM_V -- five scales, planes of 176 x 176 or more -- and the '
                        'activity-weighted XPSNR, XPSNR_U, XPSNR_V -- the ground truth is the original, test_cfg.xpsnr_fps (30) its frame rate -- '
                        'and the blocking-aware PSNR-B, PSNR-B_U, PSNR-B_V -- test_cfg.psnrb_block (8) the coded block size -- '
                        'may be listed in test_cfg.metrics too) and --save-path gets one <clip>.yuv '
                        'per clip; a dataset with bit_depth=10 | 12 (16-bit little-endian .yuv files) goes the same way at its depth; '
                        'default off')
    p.add_argument('--yuv-out-layout', choices=['i420', 'nv12', 'p010', 'p012', 'yuv420p10le', 'yuv420p12le', 'yuv422p', 'nv16', 'yuv444p', 'nv24', 'yuv422p10le',
                                                'yuv422p12le', 'yuv444p10le', 'yuv444p12le', 'p210', 'p212', 'p410', 'p412'], default='i420',
                   help='with --yuv-frames: the layout of the packed planes output (and of the written .yuv files); default i420 (yuv420p); '
                        'the 10 / 12-bit layouts for a dataset of that bit depth, the 4:2:2 / 4:4:4 layouts (yuv422p, nv16, yuv444p, nv24, '
                        'p210, ...) for a dataset of that chroma format: the output has the input\'s format')
    p.add_argument('--yuv-chroma', choices=['replicate', 'center', 'left', 'topleft'], default=None,
                   help='with --yuv-frames: where the clips\' chroma samples lie (sets data.test.chroma; include/pnpvcve.h states the modes): '
                        'replicate -- replicated in, box mean out, the default; center -- the same position, bilinear in; left -- H.264 / '
                        'HEVC / VVC streams (chroma_sample_loc_type 0); topleft -- BT.2020 / UHD (type 2).  The written planes use the '
                        'same mode')
    p.add_argument('--any-size', action='store_true',
                   help='run frames whose height or width is no multiple of 4 (generator.any_size; the same as --cfg-options '
                        'model.generator.any_size=True): the same formulas on the frame as given, no padding.  Default off: such '
                        'frames raise ValueError, as in the reference')
    p.add_argument('--ensemble', choices=['spatial', 'spatial-temporal'], default=None,
                   help="self-ensemble (sets cfg.model.ensemble = dict(type='SpatialTemporalEnsemble', is_temporal_ensemble=...)): the mean "
                        'of the outputs over the 8 flips / transposes of every clip, with spatial-temporal also over their 8 time '
                        'reversals, the motion vectors and partition maps transformed with the frames; 8 or 16 generator runs per '
                        'clip, clips run one at a time; not with --yuv-frames.  Default off')
    p.add_argument('--gain-report', default=None, type=str, metavar='DIR',
                   help='sets test_cfg.gain_report: every rank writes DIR/<clip>.json for each clip it scored -- per frame the slice type, QP, '
                        'PSNR of the output and of the compressed input and their difference dPSNR (SSIM likewise when dSSIM or SSIM_LQ is '
                        'listed), the same grouped by slice type and by QP, the table of partition classes and the grid of '
                        'test_cfg.gain_block (64) cells (include/pnpvcve.h, "Enhancement gain").  The gain names PSNR_LQ, SSIM_LQ, dPSNR, '
                        'dSSIM, PSNR_SD, PSNR_SD_LQ (and on --yuv-frames their _U / _V forms and dPSNR_YUV) may be listed in '
                        'test_cfg.metrics with or without it')
    p.add_argument('--local_rank', type=int, default=0)
    a = p.parse_args()
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(a.local_rank)
    return a


def main():
    args = parse_args()
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    # One arithmetic per run.  `--fp16` / `fp16 = dict(...)` in the config (the mmcv idiom) IS precision 'fp16'; a command line
    # switch overrides the config; two switches that disagree are an error instead of the last one silently winning.
    cli = {p for p in (args.precision, 'fp16' if args.fp16 else None) if p is not None}
    if len(cli) > 1:
        raise SystemExit(f'tools/test.py: --fp16 contradicts --precision {args.precision}')
    conf = {p for p in (cfg.get('precision', None), 'fp16' if cfg.get('fp16', None) is not None else None) if p is not None}
    if not cli and len(conf) > 1:
        raise SystemExit(f"tools/test.py: the config sets fp16 = dict(...) and precision = {cfg.get('precision')!r}")
    precision = next(iter(cli or conf), None)
    if args.launcher != 'none':
        init_dist(args.launcher, **cfg.dist_params)
    rank, world = get_dist_info()
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.testdir_lr is not None:                     # tools/test.py:98-103 of the reference
        cfg.merge_from_dict({'data.test.lq_folder': args.testdir_lr})
        print('-------------------- test LR dir :', args.testdir_lr)
    if args.testdir_gt is not None:
        cfg.merge_from_dict({'data.test.gt_folder': args.testdir_gt})
        print('-------------------- test GT dir :', args.testdir_gt)
    if args.yuv_chroma is not None:
        if not args.yuv_frames:
            raise SystemExit('tools/test.py: --yuv-chroma describes the clips of --yuv-frames')
        cfg.merge_from_dict({'data.test.chroma': args.yuv_chroma})
    if args.ensemble is not None:
        cfg.merge_from_dict({'model.ensemble': dict(_delete_=True, type='SpatialTemporalEnsemble',
                                                    is_temporal_ensemble=args.ensemble == 'spatial-temporal')})
    if args.gain_report is not None:
        cfg.merge_from_dict({'test_cfg.gain_report': args.gain_report})
    dataset = build_dataset(cfg.data.test)
    model = build_model(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if args.checkpoint.lower() != 'none':
        load_checkpoint(model, args.checkpoint, map_location='cpu')
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)) % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    model = model.to(dev)          # no DDP wrap: inference replicas share nothing
    if precision == 'fp16':
        from pnp_vcve_amd.restorer import wrap_fp16_model
        wrap_fp16_model(model)
    elif precision is not None:
        model.precision = precision
    if args.max_resident_features is not None:
        model.generator.max_resident_features = args.max_resident_features
    if args.any_size:
        model.generator.any_size = True
    if args.save_path is not None:      # PNG encode off the critical path (pnp_vcve_amd/io_async.py)
        from pnp_vcve_amd.io_async import FrameWriter
        model.frame_writer = FrameWriter(max_workers=4)
    try:
        outputs = multi_gpu_test(model, dataset, save_image=args.save_path is not None, save_path=args.save_path,
                                 device=dev, metrics=tuple(cfg.test_cfg['metrics']), clips_in_flight=args.clips_in_flight,
                                 byte_frames=args.byte_frames or args.byte_metrics, byte_metrics=args.byte_metrics,
                                 yuv_frames=args.yuv_frames, yuv_out_layout=args.yuv_out_layout)
    finally:
        if getattr(model, 'frame_writer', None) is not None:
            model.frame_writer.close()
            model.frame_writer = None
    if rank == 0:
        stats = dataset.evaluate(outputs)
        for k, v in stats.items():
            print(f'Eval-{k}: {v}')
        line = '{:.4f}/{:.4f}'.format(float(stats.get('PSNR', float('nan'))), float(stats.get('SSIM', float('nan'))))
        if 'MS-SSIM' in (cfg.test_cfg.get('metrics', None) or ()):      # a third field only when the config lists it
            line += '/{:.4f}'.format(float(stats.get('MS-SSIM', float('nan'))))
        if 'XPSNR' in (cfg.test_cfg.get('metrics', None) or ()):        # and an XPSNR field only when the config lists it
            line += '/{:.4f}'.format(float(stats.get('XPSNR', float('nan'))))
        if 'PSNR-B' in (cfg.test_cfg.get('metrics', None) or ()):       # and a PSNR-B field only when the config lists it
            line += '/{:.4f}'.format(float(stats.get('PSNR-B', float('nan'))))
        if 'dPSNR' in (cfg.test_cfg.get('metrics', None) or ()):        # and a dPSNR field only when the config lists it
            line += '/{:.4f}'.format(float(stats.get('dPSNR', float('nan'))))
        print(line)
        fps = [o['frames_per_s'] for o in outputs]
        import torch.distributed as dist
        backend = dist.get_backend() if dist.is_available() and dist.is_initialized() else 'none'
        print(f'clips {len(outputs)}  world {world}  backend {backend}  mean frames/s per clip {sum(fps) / len(fps):.2f}')
        if args.out:
            torch.save(outputs, args.out)


if __name__ == '__main__':
    main()
