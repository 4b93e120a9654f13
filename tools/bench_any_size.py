#!/usr/bin/env python
"""generator.any_size at DAVIS 480p: 7x3x480x854 with the switch on against 7x3x480x856 (the next multiple of 4) with it off, fp32,
default options, in ONE process.  Two models on the same weights; the two runs are alternated `--rounds` times, each after a warm-up
forward of its own shape, and timed with a host clock around `--steps` forwards that end in a device synchronise.  Prints frames/s
and Mpixel/s per run (the frames differ by 0.23 % in pixels).

    python tools/bench_any_size.py [--rounds 5] [--steps 8]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pnp_vcve_amd import synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=8)
ap.add_argument('--t', type=int, default=7)
args = ap.parse_args()

dev = torch.device('cuda:0')
cfg = dict(syn.DEFAULT_GENERATOR_CFG)
sd = syn.make_state_dict(cfg, seed=2025)
runs = {}
for name, (h, w, any_size) in {'480x854 any_size': (480, 854, True), '480x856': (480, 856, False)}.items():
    m = bench.build_model(cfg, sd, dev, 'fp32')
    m.any_size = any_size
    _, a = bench.make_inputs(1000, args.t, h, w, dev, 1)
    runs[name] = (m, a, h * w)


def rate(m, a):
    f = lambda: m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])      # noqa: E731
    with torch.no_grad():
        out = f()                   # warm-up of this shape (the workspace is per shape)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = f()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return args.steps * args.t / (time.perf_counter() - t0)


rates = {k: [] for k in runs}
for _ in range(args.rounds):
    for name, (m, a, _) in runs.items():
        rates[name].append(rate(m, a))
for name, v in rates.items():
    med = sorted(v)[len(v) // 2]
    print(f'{args.t}x3x{name} fp32: ' + ' '.join(f'{x:.1f}' for x in v) + f' frames/s; median {med:.1f} (min {min(v):.1f}, max {max(v):.1f}); '
          f'{med * runs[name][2] / 1e6:.1f} Mpixel/s')
