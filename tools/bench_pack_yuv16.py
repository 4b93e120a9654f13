"""Time the 4:2:0 unpacking in front of the forward's convs: the 8-bit pack kernel (NV12) against the 10-bit one (P010, and
yuv420p10le), aligned and general form, on one clip of T frames in ONE process -- device events around runs of launches, the
variants alternated round by round, the median round per variant.  Information only: both are expected to be
bound by the 16 B per pixel they write.

    python tools/bench_pack_yuv16.py [--t 7 --h 720 --w 1280 --rounds 20 --launches 50] > profiles/pack_yuv16.txt
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import ops      # noqa: E402


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
    buf8 = torch.randint(0, 256, (t, h * 3 // 2, w), generator=g, dtype=torch.uint8).to(dev)
    buf16 = torch.randint(0, 1024, (t, h * 3 // 2, w), generator=g, dtype=torch.int16)
    variants = {
        'nv12_8bit_aligned': (ops.pack_lr_yuv420, ops.yuv420_views(buf8, h, w, 'nv12'), False),
        'nv12_8bit_general': (ops.pack_lr_yuv420, ops.yuv420_views(buf8, h, w, 'nv12'), True),
        'p010_aligned': (ops.pack_lr_yuv420p16, ops.yuv420p16_views((buf16 << 6).to(dev), h, w, 'p010'), False),
        'p010_general': (ops.pack_lr_yuv420p16, ops.yuv420p16_views((buf16 << 6).to(dev), h, w, 'p010'), True),
        'yuv420p10le_aligned': (ops.pack_lr_yuv420p16, ops.yuv420p16_views(buf16.to(dev), h, w, 'yuv420p10le'), False),
    }
    for f, v, general in variants.values():      # warm up every variant: code objects, the allocator's block for the output
        for _ in range(3):
            f(v, 'bt709-limited', general=general)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (f, v, general) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f(v, 'bt709-limited', general=general)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    px = t * h * w
    for k, v in ms.items():
        v.sort()
        med = v[len(v) // 2]
        rd = 1.5 if '8bit' in k else 3.0
        print(json.dumps(dict(variant=k, t=t, h=h, w=w, rounds=a.rounds, launches_per_round=a.launches, ms_median=round(med, 5), ms_min=round(v[0], 5),
                              ms_max=round(v[-1], 5), bytes_per_pixel=rd + 16.0, gb_per_s_at_median=round(px * (rd + 16.0) / med / 1e6, 1),
                              note='per launch, torch.empty of the output included; device events around a run of launches')))


if __name__ == '__main__':
    main()
