"""Time the boundary's kernels of the three chroma formats beside each other: the aligned pack (planes -> the RGB0 conv source) and
frames_to (fp32 planes -> planes) of 4:2:0, 4:2:2 and 4:4:4 at 8 and 10 bit, on one clip of T frames in ONE process -- device events on
the caller's stream around runs of launches, the variants alternated round by round after a warm-up, the median round per variant
(tools/bench_pack_yuv16.py's scheme).  Information only: nothing here is a gate.

    python tools/bench_yuv_formats.py [--t 7 --h 720 --w 1280 --rounds 20 --launches 50] > profiles/yuv_formats_bench.txt

Bytes counted per pixel: the pack reads its samples (1.5, 2 or 3, times the sample size) and writes 16 B; frames_to reads 12 B and
writes its samples.  The pack's figure includes torch.empty of its output, as in tools/bench_pack_yuv16.py; frames_to writes planes
that exist."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import ops      # noqa: E402

SAMPLES = {'420': 1.5, '422': 2.0, '444': 3.0}
LAYOUTS = [('nv12', '420', 8), ('nv16', '422', 8), ('nv24', '444', 8), ('p010', '420', 10), ('p210', '422', 10), ('p410', '444', 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--t', type=int, default=7)
    ap.add_argument('--h', type=int, default=720)
    ap.add_argument('--w', type=int, default=1280)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--launches', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: no fallback')
    dev = torch.device('cuda:0')
    t, h, w = a.t, a.h, a.w
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand((t, 3, h, w), generator=g).to(dev)
    variants = {}
    for layout, fmt, depth in LAYOUTS:
        buf, views = ops.frames_to_yuv(rgb, 'bt709-limited', layout)       # decoder-like planes of the layout, tightly packed: the aligned form
        bytes_in = SAMPLES[fmt] * (1 if depth == 8 else 2)
        variants[f'pack_{layout}'] = (lambda v=views: ops.pack_lr_yuv(v, 'bt709-limited'), bytes_in + 16.0)
        variants[f'frames_to_{layout}'] = (lambda v=views: ops.frames_to_yuv(rgb, 'bt709-limited', out=v), 12.0 + bytes_in)
    for f, _ in variants.values():      # warm up every variant: code objects, the allocator's block for the output
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (f, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    px = t * h * w
    for k, v in ms.items():
        v.sort()
        med = v[len(v) // 2]
        bpp = variants[k][1]
        print(json.dumps(dict(variant=k, t=t, h=h, w=w, rounds=a.rounds, launches_per_round=a.launches, us_median=round(med * 1e3, 2),
                              us_min=round(v[0] * 1e3, 2), us_max=round(v[-1] * 1e3, 2), bytes_per_pixel=bpp,
                              gb_per_s_at_median=round(px * bpp / med / 1e6, 1),
                              note='per launch (frames_to: one launch per call on t frames); device events around a run of launches')))


if __name__ == '__main__':
    main()
