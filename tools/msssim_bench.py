"""Times ops.msssim_frames / msssim_yuv420 against ops.ssim_frames / ssim_yuv420 of the same build on the same inputs (information only:
no test or gate rests on it; profiles/msssim_bench.txt and DESIGN.md section 5 hold a recorded run).

    python tools/msssim_bench.py [--frames 7] [--height 720] [--width 1280] [--calls 10] [--rounds 9]

Method: device events around runs of `calls` calls, the two metrics alternated round by round after a warm-up of every shape, the median
over the rounds.  A call is the op as a user makes it: its launches, its workspace and partials allocation and the copy of the partials
to the host.  The algorithmic bytes are counted from the shapes (halo re-reads of the 26 x 42 tiles are not counted)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_vcve_amd import ops  # noqa: E402

PYRAMID = sum(0.25 ** s for s in range(1, 5))          # samples of levels 1..4 per sample of level 0
READ_AGAIN = sum(0.25 ** s for s in range(1, 4))       # levels 1..3 are read by the pyramid step as well


def bytes_per_sample(src_bytes):
    """(SSIM, MS-SSIM) algorithmic bytes per sample of one plane, both clips: SSIM reads the source once; MS-SSIM reads it twice (the
    pyramid step and the level-0 statistics), writes levels 1..4 in fp32, reads levels 1..3 for the next level and 1..4 for the statistics"""
    ssim = 2 * src_bytes
    return ssim, 2 * ssim + 2 * 4 * (PYRAMID + READ_AGAIN + PYRAMID)


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def compare(name, ssim, msssim, calls, rounds, src_bytes, samples_per_pixel, pixels):
    for fn in (ssim, msssim):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {'ssim': [], 'msssim': []}
    for _ in range(rounds):
        t['ssim'].append(timed(ssim, calls))
        t['msssim'].append(timed(msssim, calls))
    a, b = statistics.median(t['ssim']), statistics.median(t['msssim'])
    bs, bm = bytes_per_sample(src_bytes)
    print(f'{name}: SSIM {a:.3f} ms (min {min(t["ssim"]):.3f}, max {max(t["ssim"]):.3f}), MS-SSIM {b:.3f} ms '
          f'(min {min(t["msssim"]):.3f}, max {max(t["msssim"]):.3f}) per call, median of {rounds} runs of {calls} calls: ratio {b / a:.2f}')
    print(f'   algorithmic bytes per pixel of the frame: SSIM {bs * samples_per_pixel:.2f}, MS-SSIM {bm * samples_per_pixel:.2f}; '
          f'that is {bs * samples_per_pixel * pixels / a / 1e6:.1f} and {bm * samples_per_pixel * pixels / b / 1e6:.1f} GB/s of the call\'s time')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, default=7)
    p.add_argument('--height', type=int, default=720)
    p.add_argument('--width', type=int, default=1280)
    p.add_argument('--calls', type=int, default=10)
    p.add_argument('--rounds', type=int, default=9)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/msssim_bench.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    t, h, w = a.frames, a.height, a.width
    g = torch.Generator().manual_seed(0)
    x = torch.rand((t, 3, h, w), generator=g).to(dev)
    y = (x + 0.05 * torch.randn((t, 3, h, w), generator=g).to(dev)).clamp_(0, 1)
    print(f'{torch.cuda.get_device_name(0)}; {t} frames of {w}x{h}')
    compare(f'fp32 planes {t}x3x{h}x{w}', lambda: ops.ssim_frames(x, y), lambda: ops.msssim_frames(x, y), a.calls, a.rounds, 4, 3, t * h * w)
    buf_a = torch.randint(0, 256, (t, h * w * 3 // 2), generator=g, dtype=torch.uint8).to(dev)
    buf_b = (buf_a.int() + torch.randint(-6, 7, buf_a.shape, generator=g).to(dev)).clamp_(0, 255).to(torch.uint8)
    ya, yb = ops.yuv420_views(buf_a, h, w, 'i420'), ops.yuv420_views(buf_b, h, w, 'i420')
    compare(f'I420 planes {t}x{w}x{h}, planes yuv', lambda: ops.ssim_yuv420(ya, yb, 0, 'yuv'), lambda: ops.msssim_yuv420(ya, yb, 0, 'yuv'),
            a.calls, a.rounds, 1, 1.5, t * h * w)
    compare(f'I420 planes {t}x{w}x{h}, plane y', lambda: ops.ssim_yuv420(ya, yb, 0, 'y'), lambda: ops.msssim_yuv420(ya, yb, 0, 'y'),
            a.calls, a.rounds, 1, 1.0, t * h * w)


if __name__ == '__main__':
    main()
