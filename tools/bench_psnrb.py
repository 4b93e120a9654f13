"""Time the PSNR-B kernel (pnp_psnrb_sums_yuv420 / _yuv420p16: a zeroing launch and one kernel per call) against pnp_psnr_sse_yuv420 /
_yuv420p16 of the same build -- kernels that read the same bytes -- on the same clips in ONE process: device events around runs of calls
of the C entries (no allocation, no copy back), the variants alternated round by round, the median round per variant.  Information
only: no test or gate rests on it (profiles/psnrb_bench.txt holds a recorded run, DESIGN.md section 3.3 quotes it).

The algorithmic bytes of either metric are the two clips once each: 2 * 1.5 B per pixel at 8 bit, 2 * 3 B at 10 bit.  A 7-frame 720p
pair is 19 / 39 MB and would stay in the 256 MiB last-level cache from call to call, so every call takes the next of `--copies`
separate pairs (default 16: 310 / 620 MB in rotation) and the rate printed is one over memory, not over the cache.

    python tools/bench_psnrb.py [--t 7 --h 720 --w 1280 --block 8 --copies 16 --rounds 20 --launches 48] > profiles/psnrb_bench.txt
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import _native, ops      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--t', type=int, default=7)
    ap.add_argument('--h', type=int, default=720)
    ap.add_argument('--w', type=int, default=1280)
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--copies', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--launches', type=int, default=48)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: no fallback')
    dev = torch.device('cuda:0')
    t, h, w = a.t, a.h, a.w
    L = _native.lib()
    g = torch.Generator().manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, variants = [], {}
    for name, wide in (('i420_8bit', False), ('p010', True)):
        pairs = []
        for _ in range(a.copies):
            if wide:
                o = torch.randint(0, 1024, (t, h * 3 // 2, w), generator=g, dtype=torch.int16)
                r = (o + torch.randint(-3, 4, o.shape, generator=g, dtype=torch.int16)).clamp_(0, 1023)
                views = [ops.yuv420p16_views((x << 6).to(dev), h, w, 'p010') for x in (r, o)]
            else:
                o = torch.randint(0, 256, (t, h * 3 // 2, w), generator=g, dtype=torch.int16)
                r = (o + torch.randint(-3, 4, o.shape, generator=g, dtype=torch.int16)).clamp_(0, 255)
                views = [ops.yuv420_views(x.to(torch.uint8).to(dev), h, w, 'i420') for x in (r, o)]
            keep.append(views)
            pairs.append(ops._yuv_metric_pair(views[0], views[1], 0)[0][0])      # (descriptor of the test clip, of the reference)
        sums = torch.empty((t, 3, 5), dtype=torch.int64, device=dev)
        sse = torch.empty((t, 3), dtype=torch.int64, device=dev)
        pb = getattr(L, 'pnp_psnrb_sums_yuv420p16' if wide else 'pnp_psnrb_sums_yuv420')
        ps = getattr(L, 'pnp_psnr_sse_yuv420p16' if wide else 'pnp_psnr_sse_yuv420')
        sp, ep = ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(sse.data_ptr())
        variants['psnrb_' + name] = (lambda d, pb=pb, sp=sp: pb(ctypes.byref(d[0]), ctypes.byref(d[1]), 7, sp, t, h, w, 0, a.block, stream), pairs)
        variants['bef_' + name] = (lambda d, pb=pb, sp=sp: pb(ctypes.byref(d[0]), None, 7, sp, t, h, w, 0, a.block, stream), pairs)
        variants['psnr_' + name] = (lambda d, ps=ps, ep=ep: ps(ctypes.byref(d[0]), ctypes.byref(d[1]), ep, t, h, w, 0, stream), pairs)
        keep += [sums, sse]
    for f, pairs in variants.values():          # warm up every variant on every pair: code objects, page tables
        for d in pairs:
            _native.check(f(d), 'warm-up')
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (f, pairs) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                f(pairs[i % len(pairs)])
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    px = t * h * w
    med = {}
    for k, v in ms.items():
        v.sort()
        med[k] = v[len(v) // 2]
        bpp = (1 if k.startswith('bef') else 2) * (3.0 if 'p010' in k else 1.5)
        print(json.dumps(dict(variant=k, t=t, h=h, w=w, block=a.block, planes='yuv', copies=a.copies, rounds=a.rounds, launches_per_round=a.launches,
                              ms_median=round(med[k], 5), ms_min=round(v[0], 5), ms_max=round(v[-1], 5), algorithmic_bytes_per_pixel=bpp,
                              gb_per_s_at_median=round(px * bpp / med[k] / 1e6, 1),
                              note='per call of the C entry (its zeroing launch and its kernel); bef_*: the no-reference form, one clip read; '
                                   'device events around a run of calls, the pairs of clips taken in rotation')))
    for name in ('i420_8bit', 'p010'):
        print(json.dumps(dict(ratio=f'psnrb_{name} / psnr_{name}', value=round(med['psnrb_' + name] / med['psnr_' + name], 2))))


if __name__ == '__main__':
    main()
