#!/usr/bin/env python
"""Row-band chains (generator.band_split, pnp_generator_set_band_split) off against on at 720p, in ONE process: the settings are
alternated `--rounds` times, frames/s each, and the outputs compared with torch.equal.

    python tools/ab_band_split.py [--rounds 3] [--steps 8] [--settings 0,1]     # a setting >= 2 is the chain's first boundary row
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
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--steps', type=int, default=8)
ap.add_argument('--settings', default='0,1')
ap.add_argument('--hw', default='720x1280')
args = ap.parse_args()
settings = [int(v) for v in args.settings.split(',')]
h, w = (int(v) for v in args.hw.split('x'))

dev = torch.device('cuda:0')
cfg = dict(syn.DEFAULT_GENERATOR_CFG)
m = bench.build_model(cfg, syn.make_state_dict(cfg, seed=2025), dev, 'fp32')
_, a = bench.make_inputs(1000, 7, h, w, dev, 1)
f = lambda: m(a['lq'], a['QPs'], a['slices'], a['mvs'], a['base_QPs'], a['partitions'])      # noqa: E731


def rate(setting):
    m.band_split = setting
    with torch.no_grad():
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = f()
        torch.cuda.synchronize()
    return args.steps * 7 / (time.perf_counter() - t0), out


with torch.no_grad():
    for _ in range(2):
        f()
rates = {s: [] for s in settings}
ref = None
same = True
for r in range(args.rounds):
    for s in settings:
        fps, out = rate(s)
        rates[s].append(fps)
        ref = out if ref is None else ref
        same = same and torch.equal(out, ref)
base = rates[settings[0]]
for s in settings:
    v = rates[s]
    print(f'{h}x{w} fp32 band_split={s}: ' + ' '.join(f'{x:.2f}' for x in v) + f' frames/s; min {min(v):.2f} max {max(v):.2f} '
          f'({100 * (sum(v) / len(v) / (sum(base) / len(base)) - 1):+.2f} % on band_split={settings[0]})')
print(f'outputs bit-identical across all runs and settings: {same}')
