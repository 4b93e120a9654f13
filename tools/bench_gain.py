"""Time the enhancement-gain kernel (pnp_gain_sums_yuv / _yuvp16: two zeroing launches at most and ONE kernel per call, which reads the
test clip, the compressed input and the original once each) against what it replaces -- TWO calls of pnp_psnr_sse_yuv / _yuvp16 of the
same build, output against original and input against original, which read the original twice -- on the same clips in ONE process:
device events around runs of calls of the C entries (no allocation, no copy back), the variants alternated round by round, the median
round per variant.  Information only: no test or gate rests on it (profiles/gain_bench.txt holds a recorded run, DESIGN.md section 3.3
quotes it).

The algorithmic bytes: three clips once each for the gain (3 * 1.5 B per pixel at 8 bit, 3 * 3 B at 10 bit), four clip reads for the two
PSNR calls.  A 7-frame 720p triple is 29 / 58 MB and would stay in the 256 MiB last-level cache from call to call, so every call takes
the next of `--copies` separate triples (default 16: 464 / 929 MB in rotation) and the rate printed is one over memory, not the cache.
gain_par_*: the same call with a partition map (12 B per pixel more) and the class sums.

    python tools/bench_gain.py [--t 7 --h 720 --w 1280 --block 64 --copies 16 --rounds 20 --launches 48] > profiles/gain_bench.txt
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
    ap.add_argument('--block', type=int, default=64)
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
    rows, cols = ctypes.c_int(), ctypes.c_int()
    _native.check(L.pnp_gain_grid(h, w, a.block, ctypes.byref(rows), ctypes.byref(cols)), 'pnp_gain_grid')
    par = (torch.rand((t, 3, h, w), generator=g) > 0.6).float().to(dev)
    keep, variants = [par], {}
    for name, wide in (('nv12_8bit', False), ('p010', True)):
        triples = []
        top = 1023 if wide else 255
        for _ in range(a.copies):
            o = torch.randint(0, top + 1, (t, h * 3 // 2, w), generator=g, dtype=torch.int16)
            lq = (o + torch.randint(-5, 6, o.shape, generator=g, dtype=torch.int16)).clamp_(0, top)
            out = (o + torch.randint(-3, 4, o.shape, generator=g, dtype=torch.int16)).clamp_(0, top)
            if wide:
                views = [ops.yuv420p16_views((x << 6).to(dev), h, w, 'p010') for x in (out, lq, o)]
            else:
                views = [ops.yuv420_views(x.to(torch.uint8).to(dev), h, w, 'nv12') for x in (out, lq, o)]
            keep.append(views)
            da, dg = ops._yuv_metric_pair(views[0], views[2], 0)[0][0]
            dl = ops._yuv_metric_pair(views[1], views[2], 0)[0][0][0]
            triples.append((da, dl, dg))
        grid = torch.empty((t, 3, rows.value, cols.value, 2), dtype=torch.int64, device=dev)
        cls = torch.empty((t, 8, 3), dtype=torch.int64, device=dev)
        sse = torch.empty((2, t, 3), dtype=torch.int64, device=dev)
        gn = getattr(L, 'pnp_gain_sums_yuvp16' if wide else 'pnp_gain_sums_yuv')
        ps = getattr(L, 'pnp_psnr_sse_yuvp16' if wide else 'pnp_psnr_sse_yuv')
        gp, cp, pp = (ctypes.c_void_p(x.data_ptr()) for x in (grid, cls, par))
        e0, e1 = ctypes.c_void_p(sse[0].data_ptr()), ctypes.c_void_p(sse[1].data_ptr())

        def gain(d, gn=gn, gp=gp):
            return gn(ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]), 7, None, gp, None, t, h, w, 0, a.block, 0, stream)

        def gain_par(d, gn=gn, gp=gp, cp=cp, pp=pp):
            return gn(ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]), 7, pp, gp, cp, t, h, w, 0, a.block, 0, stream)

        def two_psnr(d, ps=ps, e0=e0, e1=e1):
            rc = ps(ctypes.byref(d[0]), ctypes.byref(d[2]), e0, t, h, w, 0, 0, stream)
            return rc or ps(ctypes.byref(d[1]), ctypes.byref(d[2]), e1, t, h, w, 0, 0, stream)

        variants['gain_' + name] = (gain, triples)
        variants['two_psnr_' + name] = (two_psnr, triples)
        variants['gain_par_' + name] = (gain_par, triples)
        keep += [grid, cls, sse]
    for f, triples in variants.values():          # warm up every variant on every triple: code objects, page tables
        for d in triples:
            _native.check(f(d), 'warm-up')
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (f, triples) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                f(triples[i % len(triples)])
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    px = t * h * w
    med = {}
    for k, v in ms.items():
        v.sort()
        med[k] = v[len(v) // 2]
        reads = 4 if k.startswith('two_psnr') else 3
        bpp = reads * (3.0 if 'p010' in k else 1.5) + (12.0 if k.startswith('gain_par') else 0.0)
        print(json.dumps(dict(variant=k, t=t, h=h, w=w, block=a.block, planes='yuv', copies=a.copies, rounds=a.rounds, launches_per_round=a.launches,
                              ms_median=round(med[k], 5), ms_min=round(v[0], 5), ms_max=round(v[-1], 5), algorithmic_bytes_per_pixel=bpp,
                              gb_per_s_at_median=round(px * bpp / med[k] / 1e6, 1),
                              note='per call of the C entry (its zeroing launches and its kernel); two_psnr_*: two calls of the plane PSNR, output '
                                   'and input against the original; gain_par_*: with a partition map and the class sums; device events around a '
                                   'run of calls, the triples of clips taken in rotation')))
    for name in ('nv12_8bit', 'p010'):
        print(json.dumps(dict(ratio=f'gain_{name} / two_psnr_{name}', value=round(med['gain_' + name] / med['two_psnr_' + name], 2))))
        print(json.dumps(dict(ratio=f'gain_par_{name} / gain_{name}', value=round(med['gain_par_' + name] / med['gain_' + name], 2))))


if __name__ == '__main__':
    main()
