#!/usr/bin/env python
"""The end-to-end loop of bench.py (pipeline_e2e) by itself, a few repetitions: where does the forward inside the loop lose against the
same two-clip forward in the bench?   [GPU_MAX_HW_QUEUES=8] python tools/e2e_probe.py [--reps 3]
--byte-frames: the same tree, model and warm-up through apis.multi_gpu_test(byte_frames=True) -- what `tools/test.py --byte-frames`
runs: uint8 frames into the generator, display bytes out of it, a pair of clips by pointer; --loop: that loop with the switch off;
--byte-metrics: that loop with byte_metrics=True (`tools/test.py --byte-metrics`: uint8 output only, PSNR / SSIM from the two byte clips)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--workers', type=int, default=16)
ap.add_argument('--prewarm', action='store_true', help='fill the caching allocators (device + pinned host) before the first pass')
ap.add_argument('--byte-frames', action='store_true', help='the tools/test.py loop with --byte-frames (apis.multi_gpu_test)')
ap.add_argument('--byte-metrics', action='store_true', help='the tools/test.py loop with --byte-metrics (apis.multi_gpu_test)')
ap.add_argument('--loop', action='store_true', help='the tools/test.py loop (apis.multi_gpu_test) with byte frames off: the same harness as --byte-frames')
args = ap.parse_args()
dev = torch.device('cuda:0')
print('GPU_MAX_HW_QUEUES =', os.environ.get('GPU_MAX_HW_QUEUES'), ' prewarm =', args.prewarm, flush=True)
if args.prewarm:
    x = [torch.empty(512 << 20, dtype=torch.uint8, device=dev) for _ in range(8)]
    y = [torch.empty(64 << 20, dtype=torch.uint8).pin_memory() for _ in range(12)]
    torch.cuda.synchronize()
    del x, y


def loop_e2e(dev, T, byte_frames, clips=10, workers=16, byte_metrics=False):
    """bench.pipeline_e2e's tree, model, warm-up clip and timed window (loader start to the last PNG on disk) around apis.multi_gpu_test"""
    import shutil
    import tempfile
    import time
    from pnp_vcve_amd import restorer, synthetic as syn   # noqa: F401
    from pnp_vcve_amd.apis import multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset
    from pnp_vcve_amd.io_async import FrameWriter
    from pnp_vcve_amd.registry import build_model

    class Tail:          # the clips behind the warm-up clip
        def __init__(self, ds, first, count):
            self.ds, self.first, self.count = ds, first, count

        def __len__(self):
            return self.count

        def __getitem__(self, i):
            return self.ds[i + self.first]

        def get_uint8(self, i):
            return self.ds.get_uint8(i + self.first)

    h, w = bench.WORKLOADS['720p']
    root = tempfile.mkdtemp(prefix='pnp_e2e_')
    try:
        lq, gt, qp = syn.write_clip_tree(os.path.join(root, 'data'), clips=[f'{i:03d}' for i in range(clips + 1)], t=T, h=h, w=w)
        ds = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq, gt_folder=gt, num_input_frames=100,
                                pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1,
                                val_partition='REDS4', test_mode=True))
        cfg = dict(syn.DEFAULT_GENERATOR_CFG)
        model = build_model(dict(type='BasicVSR', generator=dict(type=bench.GEN_TYPE, **cfg), pixel_loss=dict(type='CharbonnierLoss')),
                            train_cfg=None, test_cfg=dict(metrics=['PSNR', 'SSIM'], crop_border=0))
        model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=2025).items()})
        model = model.to(dev).eval()
        out_dir = os.path.join(root, 'out')
        with FrameWriter(max_workers=workers) as writer:
            model.frame_writer = writer
            multi_gpu_test(model, Tail(ds, 0, 1), save_image=True, save_path=out_dir, device=dev, clips_in_flight=2, byte_frames=byte_frames,
                           byte_metrics=byte_metrics)
            torch.cuda.synchronize()
            writer.drain()
            t0 = time.perf_counter()
            res = multi_gpu_test(model, Tail(ds, 1, clips), save_image=True, save_path=out_dir, device=dev, clips_in_flight=2,
                                 byte_frames=byte_frames, byte_metrics=byte_metrics)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            writer.drain()
            t2 = time.perf_counter()
        frames = clips * T
        fwd = sum(T / r['frames_per_s'] for r in res)
        return dict(value=frames / (t2 - t0), seconds_total=t2 - t0, frames=frames, seconds_generator_forward=fwd,
                    seconds_png_drain_after_last_clip=t2 - t1, psnr=sum(r['eval_result']['PSNR'] for r in res) / len(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


for r in range(args.reps):
    if args.byte_frames or args.byte_metrics or args.loop:
        e = loop_e2e(dev, 7, args.byte_frames, workers=args.workers, byte_metrics=args.byte_metrics)
        print('rep %d [%s]: %.1f frames/s  total %.3f s  forward %.3f s (%.1f frames/s inside the forward)  drain %.3f  PSNR %.6f'
              % (r, 'byte metrics' if args.byte_metrics else ('byte frames' if args.byte_frames else 'loop'), e['value'], e['seconds_total'], e['seconds_generator_forward'],
                 e['frames'] / e['seconds_generator_forward'], e['seconds_png_drain_after_last_clip'], e['psnr']), flush=True)
        continue
    e = bench.pipeline_e2e(dev, 7, workers=args.workers)
    print('rep %d: %.1f frames/s  total %.3f s  forward %.3f s (%.1f frames/s inside the forward)  loader waits %.3f  metrics+submit %.3f  drain %.3f'
          % (r, e['value'], e['seconds_total'], e['seconds_generator_forward'], e['frames'] / e['seconds_generator_forward'],
             e['seconds_main_thread_waiting_for_loader_h2d'], e['seconds_metrics_and_uint8_d2h_and_submit'], e['seconds_png_drain_after_last_clip']), flush=True)
