"""Asynchronous PNG write-back (overlap the write-back with compute).

The reference saves every enhanced frame synchronously inside forward_test (basicvsr.py:205-231:
tensor2img -> mmcv.imwrite), i.e. a full-precision D2H copy and a PNG encode per frame on the critical
path -- 50-80 ms per 720p frame against 24 ms of GPU time here.  FrameWriter takes the frames as uint8
(converted on the device with tensor2img's arithmetic, 4x fewer bytes over PCIe) and encodes them on a
small thread pool while the next clip is being enhanced; close() waits and re-raises the first error.
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import torch


def frames_to_uint8_hwc(frames):
    """(T,3,H,W) or (3,H,W) float tensor in [0,1] (any device) -> uint8 (T,H,W,3) RGB on the host, with
    tensor2img's arithmetic (mmedit/core/misc.py:51-71: clamp, * 255, round half to even).  A uint8 (T,H,W,3) or (H,W,3) tensor --
    frames the generator already wrote as display bytes -- passes through."""
    if frames.dtype == torch.uint8:
        if frames.shape[-1] != 3 or frames.dim() not in (3, 4):
            raise ValueError(f'uint8 frames must be (T,H,W,3) or (H,W,3) RGB, got {tuple(frames.shape)}')
        return (frames.unsqueeze(0) if frames.dim() == 3 else frames).detach().cpu().contiguous().numpy()
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.is_cuda:                       # HIP kernel (pnp_frames_to_rgb8), then a uint8 D2H copy
        from .ops import frames_to_rgb8
        return frames_to_rgb8(frames.detach().float().contiguous()).cpu().numpy()
    q = (frames.detach().float().clamp(0, 1) * 255.0).round().to(torch.uint8)
    return q.permute(0, 2, 3, 1).contiguous().numpy()


class FrameWriter:
    def __init__(self, max_workers=4, max_pending=64):
        self._pool = ThreadPoolExecutor(max_workers=max_workers, thread_name_prefix='pnp-png')
        self._slots = threading.Semaphore(max_pending)       # bounds the host memory held by queued frames
        self._futures = []
        self._lock = threading.Lock()

    @staticmethod
    def _write(path, rgb):
        from PIL import Image
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        # lossless either way; zlib level 1 is the effort the reference's writer spends (mmcv.imwrite -> cv2.imwrite, whose PNG encoder
        # defaults to Z_BEST_SPEED + RLE), PIL's default 6 takes 1.8x as long per 720p frame for 12 % smaller files
        Image.fromarray(rgb).save(path, compress_level=1)

    @staticmethod
    def _write_bytes(path, array):
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'wb') as f:
            array.tofile(f)

    def _submit(self, write, path, data):
        self._slots.acquire()

        def job():
            try:
                write(path, data)
            finally:
                self._slots.release()

        fut = self._pool.submit(job)
        with self._lock:
            self._futures.append(fut)
        return fut

    def submit(self, path, rgb_uint8_hwc):
        return self._submit(self._write, path, rgb_uint8_hwc)

    def submit_bytes(self, path, array):
        """Raw write-back: the bytes of a C-contiguous numpy array as they are (a clip's packed 4:2:0 frames -> one .yuv file), one
        job per file."""
        return self._submit(self._write_bytes, path, array)

    def drain(self):
        """Wait for every frame queued so far (the pool stays usable); raise the first failure."""
        with self._lock:
            futs, self._futures = self._futures, []
        err = None
        for f in futs:
            try:
                f.result()
            except BaseException as e:      # noqa: BLE001 -- surfaced to the caller below
                err = err or e
        if err is not None:
            raise err

    def close(self):
        """Wait for every queued frame; raise the first failure."""
        try:
            self.drain()
        finally:
            self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
