"""The three boundaries of the forward side by side on one synthetic clip, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/yuv_probe.py --reps 4

runs `--reps` forwards at the fp32 boundary, at the byte boundary (uint8 HWC in and out) and at the 4:2:0 boundary (NV12 in and out),
so that pack_lr_kernel / pack_lr_u8_kernel / pack_lr_yuv420_fast_kernel<unsigned char, 2, 0> (the aligned NV12 pack), the three forms
of conv_last and the per-frame converters appear in one trace.  Prints wall-clock frames/s per boundary (HIP events; a record, not a benchmark: bench.py measures the
headline)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import ops, synthetic as syn       # noqa: E402
from pnp_vcve_amd.registry import build_backbone      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--frames', type=int, default=7)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--standard', default='bt709-limited')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    sd = syn.make_state_dict(cfg, seed=1)
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    t, h, w = a.frames, a.height, a.width
    c = syn.make_clip(seed=2, n=1, t=t, h=h, w=w, slices='IBBBP', qp_mode='qp', crf=25)
    side = [torch.from_numpy(np.asarray(c[k])).to(dev) for k in ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions')]
    g = torch.Generator(device='cuda').manual_seed(3)
    nv12 = torch.randint(0, 256, (1, t, h * 3 // 2, w), device=dev, generator=g, dtype=torch.uint8)
    frames = ops.yuv420_views(nv12, h, w, 'nv12')
    planes = ops.frames_from_yuv420(frames, a.standard)
    u8 = ops.frames_to_rgb8(planes[0]).reshape(1, t, h, w, 3)
    runs = (('fp32', lambda: m(planes, *side)),
            ('u8', lambda: m(u8, *side, out_dtype=torch.uint8)),
            ('yuv420', lambda: m(frames, *side, out_dtype='nv12', yuv_standard=a.standard)))
    res = {}
    with torch.no_grad():
        for name, fn in runs:
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(a.reps * t / (e0.elapsed_time(e1) / 1e3), 2)
    print(json.dumps(dict(probe='yuv_probe', frames=t, h=h, w=w, reps=a.reps, frames_per_s=res)))


if __name__ == '__main__':
    main()
