"""Records for profiles/yuv_metrics.txt (a record, not a gate; bench.py measures the headline):

    python tools/yuv_metrics_probe.py [--reps 20] [--loop-clips 4]

1. device time (HIP events around `--reps` back-to-back calls of the C entries, after a warm-up) of the plane metrics on one
   7 x 720 x 1280 clip, NV12 against I420 -- pnp_psnr_sse_yuv420, pnp_ssim_partials_yuv420 for Y alone and for all three planes --
   beside pnp_psnr_stat_io / pnp_ssim_partials_io on the uint8 RGB clips of the same frames;
2. the test loop (apis.multi_gpu_test, what tools/test.py runs) on `--loop-clips` 7 x 720p clips written to a temporary tree as PNG
   folders and as .yuv files of the same content: byte_metrics=True beside yuv_frames=True, metrics only, the second pass of each."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import _native, ops, restorer, synthetic as syn       # noqa: E402,F401
from pnp_vcve_amd.apis import multi_gpu_test                            # noqa: E402
from pnp_vcve_amd.datasets import build_dataset                         # noqa: E402
from pnp_vcve_amd.registry import build_model                           # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps      # us per call


def kernels(t, h, w, reps, dev):
    L = _native.lib()
    g = torch.Generator(device='cuda').manual_seed(3)
    nv12 = torch.randint(0, 256, (t, h * 3 // 2, w), device=dev, generator=g, dtype=torch.uint8)
    a = ops.yuv420_views(nv12, h, w, 'nv12')
    rgb = ops.frames_from_yuv420(a, 'bt709-limited')
    noisy = (rgb + 0.02 * torch.randn(rgb.shape, device=dev, generator=g)).clamp(0, 1)
    i420, b = ops.frames_to_yuv420(noisy, 'bt709-limited', 'i420')
    a8, b8 = ops.frames_to_rgb8(rgb), ops.frames_to_rgb8(noisy)
    da, db = ops._yuv_clip_desc(a)[0], ops._yuv_clip_desc(b)[0]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    sse3 = torch.empty((t, 3), dtype=torch.int64, device=dev)
    sse1 = torch.empty((t,), dtype=torch.int64, device=dev)
    nby, nbc = L.pnp_ssim_blocks_yuv420(h, w, 0, 1), L.pnp_ssim_blocks_yuv420(h, w, 0, 2)
    part = torch.empty(t * (nby + 2 * nbc), dtype=torch.float64, device=dev)
    part8 = torch.empty(t * 3 * L.pnp_ssim_blocks(h, w, 0), dtype=torch.float64, device=dev)
    ok = lambda rc: _native.check(rc, 'probe')      # noqa: E731
    res = {
        'psnr_yuv420_us': timed(lambda: ok(L.pnp_psnr_sse_yuv420(ctypes.byref(da), ctypes.byref(db), P(sse3), t, h, w, 0, st)), reps),
        'psnr_u8_rgb_us': timed(lambda: ok(L.pnp_psnr_stat_io(P(a8), 1, P(b8), 1, 0, P(sse1), t, 3, h, w, 0, st)), reps),
        'ssim_yuv420_y_us': timed(lambda: ok(L.pnp_ssim_partials_yuv420(ctypes.byref(da), ctypes.byref(db), 1, P(part), t, h, w, 0, st)), reps),
        'ssim_yuv420_yuv_us': timed(lambda: ok(L.pnp_ssim_partials_yuv420(ctypes.byref(da), ctypes.byref(db), 7, P(part), t, h, w, 0, st)), reps),
        'ssim_u8_rgb_us': timed(lambda: ok(L.pnp_ssim_partials_io(P(a8), 1, P(b8), 1, 0, P(part8), t, 3, h, w, 0, st)), reps),
    }
    res['psnr_yuv_db'] = [round(float(v), 3) for v in ops.psnr_yuv420(a, b).mean(dim=0)]
    res['bytes_read_psnr_yuv420'] = 2 * t * h * w * 3 // 2
    res['bytes_read_psnr_u8_rgb'] = 2 * t * h * w * 3
    return {k: (round(v, 1) if isinstance(v, float) else v) for k, v in res.items()}


def loop(nclips, t, h, w, dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import yuv_ref
    from PIL import Image
    clips = [f'{i:03d}' for i in range(nclips)]
    with tempfile.TemporaryDirectory() as root:
        lq_png, gt_png, qp = syn.write_clip_tree(root, clips=clips, t=t, h=h, w=w, seed=1)
        folders = []
        for png in (lq_png, gt_png):
            folder = os.path.join(os.path.dirname(png), 'yuv')
            os.makedirs(folder)
            for clip in clips:
                rgb = np.stack([np.asarray(Image.open(os.path.join(png, clip, f'{i:08d}.png')).convert('RGB')) for i in range(t)])
                planes = (rgb.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)
                yuv_ref.pack(*yuv_ref.frames_to_yuv420(planes, 'bt601-limited'), 'i420').tofile(os.path.join(folder, clip + '.yuv'))
            folders.append(folder)
        ds_png = build_dataset(dict(type='SRREDSMultipleGTCompressDataset', lq_folder=lq_png, gt_folder=gt_png, num_input_frames=100,
                                    pipeline=[dict(type='LoadImageFromFileList_ipb', qp_slice_file=qp)], scale=1, val_partition='none', test_mode=True))
        ds_yuv = build_dataset(dict(type='Yuv420ClipFolderDataset', lq_folder=folders[0], gt_folder=folders[1], height=h, width=w, qp_slice_file=qp))
        cfg = dict(syn.DEFAULT_GENERATOR_CFG)
        model = build_model(dict(type='BasicVSR', generator=dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg)),
                            train_cfg=None, test_cfg=dict(metrics=['PSNR', 'SSIM'], crop_border=0))
        model.generator.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_state_dict(cfg, seed=1).items()})
        model = model.to(dev).eval()
        out = {}
        for name, ds, kw in (('byte_metrics', ds_png, dict(byte_metrics=True)), ('yuv_frames', ds_yuv, dict(yuv_frames=True)),
                             ('byte_metrics_again', ds_png, dict(byte_metrics=True)), ('yuv_frames_again', ds_yuv, dict(yuv_frames=True))):
            passes = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.time()
                r = multi_gpu_test(model, ds, device=dev, clips_in_flight=2, **kw)
                torch.cuda.synchronize()
                passes.append(round(nclips * t / (time.time() - t0), 2))
            out[name] = dict(loop_frames_per_s=passes, forward_frames_per_s=round(float(np.mean([x['frames_per_s'] for x in r])), 2),
                             psnr=round(float(np.mean([x['eval_result']['PSNR'] for x in r])), 4))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=7)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--loop-clips', type=int, default=4, help='0: skip the loop')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    doc = dict(probe='yuv_metrics_probe', frames=a.frames, h=a.height, w=a.width, reps=a.reps,
               kernels=kernels(a.frames, a.height, a.width, a.reps, dev))
    print(json.dumps(doc), flush=True)
    if a.loop_clips:
        print(json.dumps(dict(probe='yuv_metrics_probe_loop', clips=a.loop_clips, loop=loop(a.loop_clips, a.frames, a.height, a.width, dev))), flush=True)


if __name__ == '__main__':
    main()
