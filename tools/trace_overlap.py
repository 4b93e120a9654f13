#!/usr/bin/env python
"""How much of a clip step's wall time is covered by kernels, and by how much they overlap: reads the kernel-trace csv of

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 2 --warmup 1

and prints, for the last traced step (from one pack_lr_kernel to the next): wall time, the sum of the kernel durations, the time
during which at least one kernel runs, the same per hardware queue, and the tile kernels' average duration per queue.  With row-band
chains (generator.band_split) the durations of a step add up to more than its wall time: the two chains overlap.

    python tools/trace_overlap.py DIR
"""
import csv
import glob
import os
import sys
from collections import defaultdict


def main(root):
    rows = []
    for f in glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'], r['Queue_Id']))
    rows.sort()
    marks = [s for s, _, n, _ in rows if 'pack_lr_kernel' in n]
    if len(marks) < 2:
        sys.exit('need at least two traced clip steps')
    lo, hi = marks[-2], marks[-1]
    sel = [r for r in rows if lo <= r[0] < hi]
    wall = (hi - lo) / 1e3
    total = sum(e - s for s, e, _, _ in sel) / 1e3
    busy, cs, ce = 0, None, None
    for s, e, _, _ in sel:
        if ce is None or s > ce:
            busy += (ce - cs) if ce is not None else 0
            cs, ce = s, e
        else:
            ce = max(ce, e)
    busy = (busy + ce - cs) / 1e3
    print(f'one step: {len(sel)} dispatches, wall {wall:.1f} us; kernel durations add up to {total:.1f} us ({100 * total / wall:.1f} % of wall); '
          f'some kernel running {busy:.1f} us ({100 * busy / wall:.1f} %)')
    per_q = defaultdict(lambda: [0, 0.0])
    tiles = defaultdict(lambda: [0, 0.0])
    for s, e, n, q in sel:
        per_q[q][0] += 1
        per_q[q][1] += (e - s) / 1e3
        if 'conv3x3_wino' in n and 'quad' not in n:
            tiles[q][0] += 1
            tiles[q][1] += (e - s) / 1e3
    for q in sorted(per_q):
        n, us = per_q[q]
        tn, tus = tiles[q]
        print(f'  queue {q}: {n} dispatches, {us:.1f} us' + (f'; Winograd tile kernels {tn} x {tus / tn:.1f} us' if tn else ''))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '.')
