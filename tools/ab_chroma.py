#!/usr/bin/env python
"""The chroma modes of the 4:2:0 boundary (include/pnpvcve.h) measured against the default, in ONE process:

1. the pack kernel in front of the convs at T x h x w, every mode x (aligned | general form) x (NV12 | I420 | P010): device events
   around runs of launches, the variants alternated round by round, the median round per variant, and the bytes moved (the planes read
   once + 16 B per pixel written) over that time as a fraction of the HBM peak.  'replicate' is the kernel the default path always had:
   the yardstick of the same session;
2. the forward's frames/s on one NV12 clip per mode, the modes alternated `--fwd-rounds` times.

Information only: the sited forms write the same 16 B per pixel and read the same planes.

    python tools/ab_chroma.py [--t 7 --h 720 --w 1280 --rounds 20 --launches 50 --fwd-rounds 3 --steps 4] > profiles/chroma_siting_bench.txt
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pnp_vcve_amd import ops  # noqa: E402
from pnp_vcve_amd import synthetic as syn  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, the MI355X's specified peak


def pack_rates(a, dev):
    t, h, w = a.t, a.h, a.w
    g = torch.Generator().manual_seed(0)
    buf8 = torch.randint(0, 256, (t, h * 3 // 2, w), generator=g, dtype=torch.uint8).to(dev)
    buf16 = (torch.randint(0, 1024, (t, h * 3 // 2, w), generator=g, dtype=torch.int16) << 6).to(dev)
    clips = {'nv12': (ops.pack_lr_yuv420, ops.yuv420_views(buf8, h, w, 'nv12'), 1.5),
             'i420': (ops.pack_lr_yuv420, ops.yuv420_views(buf8, h, w, 'i420'), 1.5),
             'p010': (ops.pack_lr_yuv420p16, ops.yuv420p16_views(buf16, h, w, 'p010'), 3.0)}
    variants = {(c, mode, general): clips[c] for c in clips for mode in ops.YUV_CHROMA for general in (False, True)}
    run = lambda key: variants[key][0](variants[key][1], 'bt709-limited', general=key[2], chroma=key[1])      # noqa: E731
    ref = {}
    for key in variants:        # warm up every variant; the two forms of a mode must agree
        for _ in range(3):
            out = run(key)
        same = ref.setdefault(key[:2], out)
        assert torch.equal(same, out), key
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for key in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                run(key)
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / a.launches)
    px = t * h * w
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for (c, mode, general), v in ms.items():
        m, bpp = med[(c, mode, general)], variants[(c, mode, general)][2] + 16.0
        print(json.dumps(dict(section='pack', planes=c, chroma=mode, form='general' if general else 'aligned', t=t, h=h, w=w, rounds=a.rounds,
                              launches_per_round=a.launches, ms_median=round(m, 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5),
                              bytes_per_pixel=bpp, tb_per_s_at_median=round(px * bpp / m / 1e9, 3),
                              fraction_of_hbm_peak=round(px * bpp / (m * 1e-3) / HBM_PEAK, 3),
                              against_replicate=round(m / med[(c, 'replicate', general)], 3))), flush=True)


def forward_rates(a, dev):
    t, h, w = a.t, a.h, a.w
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    m = bench.build_model(cfg, syn.make_state_dict(cfg, seed=2025), dev, 'fp32')
    _, x = bench.make_inputs(1000, t, h, w, dev, 1)
    frames = ops.frames_to_yuv420(x['lq'].float(), 'bt709-limited', 'nv12')[1]
    f = lambda mode: m(frames, x['QPs'], x['slices'], x['mvs'], x['base_QPs'], x['partitions'], yuv_standard='bt709-limited', chroma=mode)      # noqa: E731
    rates = {mode: [] for mode in ops.YUV_CHROMA}
    with torch.no_grad():
        for mode in rates:
            f(mode)
        for _ in range(a.fwd_rounds):
            for mode in rates:
                f(mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    f(mode)
                torch.cuda.synchronize()
                rates[mode].append(a.steps * t / (time.perf_counter() - t0))
    base = sorted(rates['replicate'])[len(rates['replicate']) // 2]
    for mode, v in rates.items():
        med = sorted(v)[len(v) // 2]
        print(json.dumps(dict(section='forward', planes='nv12', chroma=mode, t=t, h=h, w=w, steps=a.steps, frames_per_s=[round(r, 2) for r in v],
                              frames_per_s_median=round(med, 2), against_replicate=round(med / base, 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--t', type=int, default=7)
    ap.add_argument('--h', type=int, default=720)
    ap.add_argument('--w', type=int, default=1280)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--fwd-rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: no fallback')
    dev = torch.device('cuda:0')
    pack_rates(a, dev)
    if a.fwd_rounds > 0:
        forward_rates(a, dev)


if __name__ == '__main__':
    main()
