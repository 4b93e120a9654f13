"""Cost of the bounded-memory forward (generator.max_resident_features) against the unbounded one, in one process.

For 7 x 3 x 720 x 1280 and 100 x 3 x 720 x 1280 fp32 clips: unbounded, k = the minimum, and one k in between.  Per setting: frames/s
(median of --reps timed forwards, HIP events, after a warm-up; the settings alternate run by run), peak device memory
(torch.cuda.max_memory_allocated over one forward, inputs excluded), the timed-launch count of one profiled forward (recomputed
branch runs included) and torch.equal against the unbounded output.  --long T adds one forward of a T-frame 720p clip at k = min
(no repeat) when torch.cuda.mem_get_info() shows room for it: a clip the unbounded schedule could not hold when T is large enough.

    python tools/bench_long_clip.py [--reps 5] [--long 1200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_clip(t, h, w, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    lq = torch.rand(1, t, 3, h, w, device='cuda', generator=g)
    mvs = (torch.randint(-16, 17, (1, t, 4, h // 8, w // 8), device='cuda', generator=g).float() / 4
           ).repeat_interleave(8, 3).repeat_interleave(8, 4).contiguous()
    cls = torch.randint(0, 3, (1, t, 1, h // 8, w // 8), device='cuda', generator=g)
    par = (torch.cat([(cls == j) for j in range(3)], dim=2).float() / 255.0).repeat_interleave(8, 3).repeat_interleave(8, 4).contiguous()
    sl = torch.tensor([73.0 if i == 0 else (80.0 if i % 4 == 0 else 66.0) for i in range(t)], device='cuda').view(1, t, 1, 1, 1)
    qp = torch.full((1, t, 1, 1, 1), 28 / 255.0, device='cuda')
    return dict(lq=lq, QPs=qp, slices=sl, mvs=mvs, base_QPs=torch.full_like(qp, 25 / 255.0), partitions=par)


def ws_bytes(m, t, h, w):
    from pnp_vcve_amd import _native
    return int(_native.lib().pnp_generator_workspace_bytes(m._handle, t, h, w))


def forward(m, c):
    with torch.no_grad():
        return m(c['lq'], c['QPs'], c['slices'], c['mvs'], c['base_QPs'], c['partitions'])


def timed(m, c, k):
    m.max_resident_features = k
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = forward(m, c)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def peak_and_launches(m, c, k):
    m.max_resident_features = k
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = forward(m, c)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    m.profile(True)
    forward(m, c)
    launches = sum(v['launches'] for v in m.profile_read().values())
    m.profile(False)
    return peak, launches


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--long', type=int, default=0)
    args = p.parse_args()
    from pnp_vcve_amd import synthetic as syn
    from pnp_vcve_amd.registry import build_backbone
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)         # configs/HR_davis_LR_128x128.py's generator
    sd = syn.make_state_dict(cfg, seed=5, par_gain=1.0)
    m = build_backbone(dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par', **cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.cuda().eval()
    h, w = 720, 1280
    results = []
    for t in (7, 100):
        c = make_clip(t, h, w, seed=t)
        kmin = m.min_resident_features(t)
        settings = [None, (kmin + t) // 2, kmin]
        ms = {k: [] for k in settings}
        ref = None
        for k in settings:                     # warm-up of every setting
            timed(m, c, k)
        for rep in range(args.reps):           # alternated
            for k in (settings if rep % 2 == 0 else settings[::-1]):
                dt, out = timed(m, c, k)
                ms[k].append(dt)
                if k is None and ref is None:
                    ref = out.clone()
        for k in settings:
            _, out = timed(m, c, k)
            equal = bool(torch.equal(out, ref))
            del out
            peak, launches = peak_and_launches(m, c, k)
            med = statistics.median(ms[k])
            r = dict(t=t, h=h, w=w, k=k if k is not None else 'unbounded', min_k=kmin, frames_per_s=round(t * 1000.0 / med, 2),
                     median_ms=round(med, 2), runs_ms=[round(x, 2) for x in ms[k]], peak_gb=round(peak / 1e9, 3),
                     workspace_gb=round(ws_bytes(m, t, h, w) / 1e9, 3), timed_launches=launches, equal_to_unbounded=equal)
            print(json.dumps(r), flush=True)
            results.append(r)
        del c, ref
        m.max_resident_features = None
        m._workspace = {}
        torch.cuda.empty_cache()
    if args.long:
        t = args.long
        kmin = m.min_resident_features(t)
        m.max_resident_features = kmin
        need = ws_bytes(m, t, h, w) + t * h * w * (3 + 4 + 3 + 3) * 4
        m.max_resident_features = None
        unbounded = ws_bytes(m, t, h, w) + t * h * w * (3 + 4 + 3 + 3) * 4
        free, total = torch.cuda.mem_get_info()
        r = dict(t=t, h=h, w=w, k=kmin, bounded_need_gb=round(need / 1e9, 1), unbounded_need_gb=round(unbounded / 1e9, 1),
                 free_gb=round(free / 1e9, 1))
        if need + (8 << 30) < free:
            c = make_clip(t, h, w, seed=t)
            m.max_resident_features = kmin
            torch.cuda.reset_peak_memory_stats()
            dt, out = timed(m, c, kmin)
            r.update(frames_per_s=round(t * 1000.0 / dt, 2), peak_gb_total=round(torch.cuda.max_memory_allocated() / 1e9, 1),
                     finite=bool(torch.isfinite(out).all()))
        else:
            r.update(skipped='not enough free device memory')
        print(json.dumps(r), flush=True)
        results.append(r)
    print(json.dumps(dict(bench_long_clip=results)))


if __name__ == '__main__':
    main()
