#!/usr/bin/env python
"""The self-ensemble's cost beside the forwards it is made of (generator.forward_ensemble, spatial: 8 variants), fp32, default options,
at 7x3x720x1280 and 7x3x128x128, in ONE process:

    A  forward_ensemble on one clip: 7 views + 8 forwards in forward_clips groups + 8 oriented accumulations;
    B  the same forward_clips calls on views made beforehand -- the 8 forwards alone.

A and B are alternated `--rounds` times after a warm-up of each; every sample is `--steps` calls between two device events; the median
over the rounds is reported: ensemble frames/s (the clip's frames over A), the 8 forwards' frames/s and the share of A outside them.

    python tools/bench_ensemble.py [--rounds 5] [--steps 3]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o ens -- python tools/bench_ensemble.py --trace-run 720x1280 [--steps 3]
    python tools/bench_ensemble.py --summarize DIR --trace-run 720x1280 [--steps 3]

The last form reads the trace's *kernel_trace.csv and sets the two ensemble kernels' time against their algorithmic bytes: a view moves
40 B per pixel and frame in and 40 out (lq 12, mvs 16, par 12); an accumulation reads 12 (the first) or 24 and writes 12."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0      # the MI355X's HBM3E peak
KEYS = ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions')
SHAPES = ((720, 1280), (128, 128))


def setup(h, w, t):
    import torch
    import bench
    from pnp_vcve_amd import ops, synthetic as syn
    dev = torch.device('cuda:0')
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    m = bench.build_model(cfg, syn.make_state_dict(cfg, seed=2025), dev, 'fp32')
    _, a = bench.make_inputs(1000, t, h, w, dev, 1)
    ensemble = lambda: m.forward_ensemble(*(a[k] for k in KEYS))      # noqa: E731
    # B: forward_ensemble's own grouping, recorded from one run of it, on views that already exist
    sizes, inner = [], m.forward_clips
    m.forward_clips = lambda clips, **kw: (sizes.append(len(clips)), inner(clips, **kw))[1]
    with torch.no_grad():
        ensemble()
    m.forward_clips = inner
    views = []
    for v in ops.ENSEMBLE_SPATIAL:
        lq, mv, par = ops.ensemble_view(a['lq'][0], a['mvs'][0], a['partitions'][0], v)
        qp, sl, bq = ops.ensemble_side(a['QPs'][0], a['slices'][0], a['base_QPs'][0], v)
        views.append((lq, qp, sl, mv, bq, par))
    groups, i = [], 0
    for n in sizes:
        groups.append(views[i:i + n])
        i += n

    def forwards():
        out = None
        for g in groups:
            out = m.forward_clips(g, out_dtype=torch.float32)
        return out[-1]

    return ensemble, forwards, sizes


def sample_ms(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        e0.record()
        for _ in range(steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return e0.elapsed_time(e1) / steps


def timing(args):
    for h, w in SHAPES:
        ensemble, forwards, sizes = setup(h, w, args.t)
        for fn in (ensemble, forwards):
            sample_ms(fn, 1)                                          # warm-up: workspaces, code objects
        ms = {'ensemble': [], 'forwards': []}
        for _ in range(args.rounds):
            ms['ensemble'].append(sample_ms(ensemble, args.steps))
            ms['forwards'].append(sample_ms(forwards, args.steps))
        a, b = statistics.median(ms['ensemble']), statistics.median(ms['forwards'])
        print(f'{args.t}x3x{h}x{w} fp32 spatial ensemble, forward_clips groups {sizes}: ensemble {a:.2f} ms/clip = {args.t * 1e3 / a:.2f} frames/s '
              f'(samples ' + ' '.join(f'{x:.2f}' for x in ms['ensemble']) + f'); the 8 forwards alone {b:.2f} ms = {8 * args.t * 1e3 / b:.2f} '
              f'forward frames/s (samples ' + ' '.join(f'{x:.2f}' for x in ms['forwards']) + f'); outside the forwards {100 * (a - b) / a:.2f} % of the ensemble', flush=True)


def trace_run(args):
    h, w = (int(x) for x in args.trace_run.split('x'))
    ensemble, _, _ = setup(h, w, args.t)             # (setup itself runs the ensemble once and makes the 7 views once more)
    for _ in range(args.steps):
        sample_ms(ensemble, 1)


def summarize(args):
    h, w = (int(x) for x in args.trace_run.split('x'))
    px = args.t * h * w
    agg = {}
    for f in glob.glob(os.path.join(args.summarize, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ('ensemble_view_kernel', 'ensemble_accumulate_kernel'):
                if k in r['Kernel_Name']:
                    n, ns = agg.get(k, (0, 0))
                    agg[k] = (n + 1, ns + int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    if not agg:
        raise SystemExit(f'no ensemble kernel in the traces under {args.summarize}')
    # bytes per launch: a view 80 B per pixel and frame; an accumulation 36, the first of 8 24: 34.5 on average
    per = {'ensemble_view_kernel': 80.0 * px, 'ensemble_accumulate_kernel': (7 * 36.0 + 24.0) / 8 * px}
    for k, (n, ns) in sorted(agg.items()):
        tbs = per[k] * n / (ns * 1e-9) / 1e12
        print(f'{k}: {n} launches at {args.t}x3x{h}x{w}, {ns / n / 1e3:.1f} us each, {per[k] / 1e6:.1f} MB algorithmic per launch: {tbs:.2f} TB/s = '
              f'{100 * tbs / HBM_TBS:.1f} % of {HBM_TBS:.0f} TB/s')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--t', type=int, default=7)
    ap.add_argument('--trace-run', default=None, metavar='HxW', help='only run the ensemble --steps times at this size (under rocprofv3)')
    ap.add_argument('--summarize', default=None, metavar='DIR', help='read the kernel trace under DIR (made with --trace-run HxW)')
    args = ap.parse_args()
    if args.summarize:
        summarize(args)
    elif args.trace_run:
        trace_run(args)
    else:
        timing(args)
