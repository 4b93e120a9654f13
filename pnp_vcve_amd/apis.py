"""Test loops (mmedit/apis/test.py:13-126) for the hot path: one process per GPU, each runs its
shard of clips through model(test_mode=True, **data); metrics are gathered with one all-gather."""
import torch

from .datasets import collate
from .dist import gather_clip_metrics, get_dist_info, shard_indices


def _to_device(data, device, byte_frames=False, byte_metrics=False):
    """Host -> device; when the clip carries raw decoder MV records (CompressedClipFolderDataset) the dense
    motion / partition maps are painted on the GPU (pnp_rasterise_side_info_f32) instead of on the host.
    byte_frames: frames uploaded as uint8 stay what the decoder made -- `lq` is the (n,T,H,W,3) uint8 tensor itself, which the
    generator reads directly (generator.forward's byte frames), and `gt` becomes fp32 planes in one kernel (ops.frames_from_rgb8:
    the same 256 values as the loop below, bit for bit).
    byte_metrics (with byte_frames): `gt` stays the (n,T,H,W,3) uint8 tensor too -- the device metrics read the bytes.
    Raw 4:2:0 clips (Yuv420ClipFolderDataset: `lq_yuv` / `gt_yuv`, packed (n,T,3h/2,w) uint8) are uploaded as they are, 1.5 B per
    pixel, and become ops.Yuv420Frames views of those buffers (`lq`, `gt`) in the layout the sample's meta names: nothing is converted.
    Where the meta names a bit_depth of 10 or 12 the buffers are 16-bit words (3 B per pixel) and the views ops.Yuv420Frames16."""
    out = {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in data.items()}
    for k in ('lq', 'gt'):
        if k + '_yuv' in out:
            from .ops import YUV_FORMAT_LAYOUTS, _yuv_views_format, yuv420_views, yuv420p16_views
            buf = out.pop(k + '_yuv')                                      # (n, T, 3h/2, w); 4:2:2: 2h rows, 4:4:4: 3h
            meta = data['meta'][0]
            if meta.get('format', '420') != '420':                         # (the layout names the format and the plane order)
                fmt, order = YUV_FORMAT_LAYOUTS[meta['layout']][:2]
                tail = () if meta.get('bit_depth', 8) == 8 else (meta['bit_depth'], meta.get('msb_aligned', False))
                out[k] = _yuv_views_format(buf, buf.shape[-2] // (2 if fmt == '422' else 3), buf.shape[-1], fmt, order, tail)
            elif meta.get('bit_depth', 8) != 8:
                out[k] = yuv420p16_views(buf, buf.shape[-2] * 2 // 3, buf.shape[-1], (meta['layout'], meta['bit_depth'], meta.get('msb_aligned', False)))
            else:
                out[k] = yuv420_views(buf, buf.shape[-2] * 2 // 3, buf.shape[-1], meta['layout'])
    if byte_frames:
        from .ops import frames_from_rgb8
        if 'lq_u8' in out:
            out['lq'] = out.pop('lq_u8')
        if 'gt_u8' in out:
            out['gt'] = out.pop('gt_u8') if byte_metrics else frames_from_rgb8(out.pop('gt_u8'))
    for k in ('lq', 'gt'):
        if k + '_u8' in out:       # frames uploaded as uint8 (dataset.get_uint8): RescaleToZeroOne + FramesToTensor on the device.
            # The 256 possible values come from the host's own fp32 division (a device-side `x / 255.0` multiplies by a rounded
            # reciprocal and is not bit-equal): a table lookup reproduces numpy's bits by construction
            u8 = out.pop(k + '_u8')                                    # (n, T, H, W, 3)
            lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(u8.device)
            n, t, h, w, c = u8.shape
            f = torch.empty((n, t, c, h, w), dtype=torch.float32, device=u8.device)
            for i in range(n):
                for j in range(t):                                   # frame by frame: the int64 index of a 100-frame 720p clip is 2.2 GB
                    f[i, j] = lut[u8[i, j].permute(2, 0, 1).long()]
            out[k] = f
    if 'mv_records' in out:
        from .ops import rasterise_side_info
        rec, rf = out.pop('mv_records'), out.pop('rec_frame')
        if isinstance(out['lq'], tuple):           # ops.Yuv420Frames
            t, (h, w) = out['lq'].y.shape[1], out['lq'].y.shape[-2:]
        else:
            t = out['lq'].shape[1]
            h, w = out['lq'].shape[2:4] if out['lq'].dtype == torch.uint8 else out['lq'].shape[-2:]
        sl = [float(v) for v in data['slices'].reshape(-1)[:t]]
        mvs, par = rasterise_side_info(rec.float(), rf.int(), sl, h, w)
        out['mvs'], out['partitions'] = mvs.unsqueeze(0), par.unsqueeze(0)
    return out


class ClipPrefetcher:
    """Streams clips to the GPU one ahead of the compute: a worker thread reads /
    decodes clip i+1 on the host and its H2D copies run on a side HIP stream from pinned memory while clip i
    is being enhanced on the compute stream.  The reference's loop is strictly serial per rank (DataLoader ->
    scatter -> forward -> evaluate, mmedit/apis/test.py:100-119); with whole 100-frame 720p clips the input
    of one clip is 3.7 GB (lq + mvs + partitions), i.e. ~60 ms of PCIe time that this hides."""

    def __init__(self, dataset, indices, device, depth=1, byte_frames=False, byte_metrics=False):
        import queue
        import threading
        self.dataset, self.indices, self.device = dataset, list(indices), torch.device(device)
        self.byte_frames = bool(byte_frames)          # _to_device(byte_frames=...): lq stays the decoder's uint8 frames
        self.byte_metrics = bool(byte_metrics)        # ... and so does gt
        self.cuda = self.device.type == 'cuda'
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.q = queue.Queue(maxsize=max(1, int(depth)))      # clips staged ahead of the consumer
        self.th = threading.Thread(target=self._work, daemon=True)
        self.th.start()

    def _work(self):
        try:
            u8 = self.cuda and hasattr(self.dataset, 'get_uint8')      # frames travel as uint8, /255 + HWC->CHW on the device
            for i in self.indices:
                data = collate([self.dataset.get_uint8(i) if u8 else self.dataset[i]])
                if self.cuda:
                    data = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in data.items()}
                    with torch.cuda.stream(self.stream):
                        dev = _to_device(data, self.device, self.byte_frames, self.byte_metrics)
                        ev = torch.cuda.Event()
                        ev.record(self.stream)
                    self.q.put((dev, ev, data))           # keep the pinned host copies alive until consumed
                else:
                    self.q.put((_to_device(data, self.device, self.byte_frames, self.byte_metrics), None, None))
            self.q.put(None)
        except BaseException as e:                        # surface loader errors in the consumer
            self.q.put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            dev, ev, _host = item
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                for v in dev.values():
                    for x in (v if isinstance(v, tuple) else (v,)):        # (ops.Yuv420Frames: views of one uploaded buffer)
                        if torch.is_tensor(x):
                            x.record_stream(torch.cuda.current_stream(self.device))
            yield dev


def single_gpu_test(model, dataset, save_image=False, save_path=None, device='cuda'):
    model.eval()
    results = []
    for i in range(len(dataset)):
        data = _to_device(collate([dataset[i]]), device)
        with torch.no_grad():
            results.append(model(test_mode=True, save_image=save_image, save_path=save_path, **data))
    return results


GENERATOR_INPUTS = ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions')


def _frames(x):
    """the frame count of a clip's `lq`: a (n,t,...) tensor or ops.Yuv420Frames of such views"""
    return x.y.shape[1] if isinstance(x, tuple) else x.shape[1]


def _pairable(a, b):
    """two clips can go through the generator as one batch: same shapes of everything it reads"""
    if isinstance(a.get('lq'), tuple) or isinstance(b.get('lq'), tuple):       # ops.Yuv420Frames: the Y planes stand for the frames
        if not (isinstance(a.get('lq'), tuple) and isinstance(b.get('lq'), tuple)):
            return False
        a, b = dict(a, lq=a['lq'].y), dict(b, lq=b['lq'].y)
    return all(torch.is_tensor(a.get(k)) and torch.is_tensor(b.get(k)) and a[k].shape == b[k].shape and a[k].device == b[k].device
               for k in GENERATOR_INPUTS)


def multi_gpu_test(model, dataset, save_image=False, save_path=None, device='cuda', metrics=('PSNR', 'SSIM'), clips_in_flight=1,
                   byte_frames=False, byte_metrics=False, yuv_frames=False, yuv_out_layout='i420'):
    """Returns, on every rank, the ordered per-clip results [{'eval_result': {...}}, ...].

    clips_in_flight = 2: two clips of equal shape are enhanced by ONE generator call (a batch of two), which the generator runs
    interleaved on two streams -- each clip's conv launches fill the partial last round of tiles and the dispatch gaps of the
    other's (+5 % at 720p, bit-identical to one clip at a time); metrics and image saving stay clip by
    clip (the reference evaluates with samples_per_gpu=1, mmedit/apis/test.py:100-119).  Costs a second workspace.
    `frames_per_s` of a PAIRED clip is the pair's throughput (frames of both clips over the pair's wall time), not the clip's own
    forward time; an unpaired leftover clip (odd count, shape change, sparse_val model) reports its own.

    byte_frames (default off: the loop above, unchanged): the frames stay uint8 from the decoder to the generator, which also writes
    the display bytes the PNG writer takes -- fp32 planes only when metrics are computed, uint8 frames only when images are saved,
    both when both -- and a pair goes to the generator as two clips by pointer (generator.forward_clips) instead of a concatenated
    batch.  Same PSNR / SSIM and the same PNG bytes.

    byte_metrics (default off; implies byte_frames): the metrics read bytes as well -- `gt` stays the decoder's uint8 frames, the
    generator is asked for uint8 frames only, with or without save_image, and PSNR / SSIM are computed from the two byte clips
    (ops.psnr_frames / ssim_frames: 6 B per pixel and frame instead of 24, and no fp32 copy of either clip).  The same values: the
    metrics round the fp32 planes to exactly these bytes.

    yuv_frames (default off; a dataset of raw 4:2:0 clips, Yuv420ClipFolderDataset): the generator reads the decoder's planes and is
    asked for packed 4:2:0 in `yuv_out_layout` ('i420' | 'nv12') ONLY, the ground truth stays 8-bit planes on the device, the metrics
    are the plane metrics of BasicVSR.evaluate (ops.psnr_yuv420 / ssim_yuv420: 'PSNR' / 'SSIM' score the Y plane; 'PSNR_U', 'PSNR_V',
    'SSIM_U', 'SSIM_V', 'PSNR_YUV', the 'MS-SSIM', the 'XPSNR' and the 'PSNR-B' names are accepted too), and save_image writes <save_path>/<clip>.yuv -- exactly the bytes of
    ops.frames_to_yuv420(fp32 output, standard, layout).  A pair goes through generator.forward_clips by pointer, as under byte_frames.
    The dataset's `chroma` ('replicate' unless it says otherwise: where its clips' chroma samples lie, include/pnpvcve.h) is the
    chroma mode of every generator call and of the planes written; the generator is told only when it is not 'replicate'.
    A dataset of 10 / 12-bit clips (its samples' meta carry the depth) goes the same way as ops.Yuv420Frames16; yuv_out_layout then
    also takes 'p010' | 'p012' | 'yuv420p10le' | 'yuv420p12le', the ground truth and the output must agree in depth, and the file is
    ops.frames_to_yuv420p16's words, little-endian.

    The enhancement-gain names (metrics.GAIN_METRICS: 'dPSNR', 'dSSIM', 'PSNR_LQ', 'SSIM_LQ', 'PSNR_SD', 'PSNR_SD_LQ'; with yuv_frames
    also metrics.GAIN_PLANE_METRICS) travel as ordinary columns of the gathered table under every switch above: forward_test hands
    the clip's `lq` and partition map to BasicVSR.evaluate, and with test_cfg.gain_report = DIR each rank writes DIR/<clip>.json for
    the clips it scored.

    A model built with ensemble=dict(type='SpatialTemporalEnsemble', ...) runs clip by clip whatever clips_in_flight says (the same
    metrics); byte_frames / byte_metrics work as above, yuv_frames raises ValueError."""
    import time
    model.eval()
    rank, world = get_dist_info()
    mine = shard_indices(len(dataset), rank, world)
    local = []
    dev = torch.device(device)
    pairs = int(clips_in_flight) >= 2 and dev.type == 'cuda' and hasattr(model, 'generator') and not getattr(model, 'psnr_only', False)
    # a sparse_val generator evaluates one sample per call in eval mode (the reference indexes feature[0, ...],
    # sr_backbone_utils.py:262-275; generator.py refuses n != 1): such a model keeps the clip-by-clip loop
    pairs = pairs and not getattr(model.generator, 'sparse_val', False)
    # a model with a self-ensemble (BasicVSR(ensemble=...)) runs clip by clip: one clip is 8 or 16 generator runs already, which
    # generator.forward_ensemble sends through forward_clips in groups
    ensemble = getattr(model, 'forward_ensemble', None) is not None
    pairs = pairs and not ensemble
    if ensemble and yuv_frames:
        raise ValueError('yuv_frames with a self-ensemble model: the ensemble takes fp32 or uint8 RGB frames, not 4:2:0 planes')

    byte_frames = (bool(byte_frames) or bool(byte_metrics)) and dev.type == 'cuda' and hasattr(model, 'generator') and not getattr(model, 'psnr_only', False)
    byte_metrics = bool(byte_metrics) and byte_frames
    yuv_frames = bool(yuv_frames)
    if yuv_frames:
        if dev.type != 'cuda' or not hasattr(model, 'generator') or getattr(model, 'psnr_only', False):
            raise ValueError('yuv_frames runs the generator on the GPU: a CUDA/HIP device and a model with a generator (not psnr_only)')
        if byte_frames:
            raise ValueError('yuv_frames and byte_frames / byte_metrics are two boundaries: pick one')
        from .ops import YUV16_LAYOUTS, YUV_FORMAT_LAYOUTS, yuv_layout
        depth = getattr(dataset, 'bit_depth', 8)
        if yuv_out_layout not in ('i420', 'nv12') and yuv_out_layout not in YUV16_LAYOUTS and yuv_out_layout not in YUV_FORMAT_LAYOUTS:
            raise ValueError(f"yuv_out_layout must be 'i420' or 'nv12', or one of {sorted(YUV16_LAYOUTS)} for a 10 / 12-bit dataset, "
                             f'or one of {list(YUV_FORMAT_LAYOUTS)} for a 4:2:2 / 4:4:4 dataset, got {yuv_out_layout!r}')
        if yuv_layout(yuv_out_layout)[0] != getattr(dataset, 'format', '420'):
            raise ValueError(f'yuv_out_layout {yuv_out_layout!r} does not have the dataset\'s chroma format ({getattr(dataset, "format", "420")}): '
                             f'the planes written have the input\'s format')
        if yuv_layout(yuv_out_layout)[2] != depth:
            raise ValueError(f'yuv_out_layout {yuv_out_layout!r} does not have the dataset\'s bit depth ({depth}): the output is scored '
                             f'against the ground truth at one depth')
    yuv_standard = getattr(dataset, 'yuv_standard', 'bt601-limited')
    chroma = getattr(dataset, 'chroma', 'replicate')
    yuv_kw = {'yuv_standard': yuv_standard} if chroma == 'replicate' else {'yuv_standard': yuv_standard, 'chroma': chroma}
    out_dtype = None
    if yuv_frames:
        out_dtype = yuv_out_layout
    elif byte_metrics:
        out_dtype = torch.uint8
    elif byte_frames:
        test_cfg = getattr(model, 'test_cfg', None)
        want_f32 = bool(test_cfg is not None and test_cfg.get('metrics', None)) or not save_image
        out_dtype = 'both' if (want_f32 and save_image) else (torch.float32 if want_f32 else torch.uint8)

    def finish(data, out=None, fps=None):
        with torch.no_grad():
            kw = {} if out is None else {'precomputed_output': out}
            if byte_frames or yuv_frames:
                kw['out_dtype'] = out_dtype
            if yuv_frames:
                kw.update(yuv_kw)
            res = model(test_mode=True, save_image=save_image, save_path=save_path, **kw, **data)
        if fps is None:
            fps = _frames(data['lq']) / model.last_forward_seconds if getattr(model, 'last_forward_seconds', None) else 0.0
        local.append([float(res['eval_result'].get(m, float('nan'))) for m in metrics] + [fps])

    held = None
    for data in ClipPrefetcher(dataset, mine, device, depth=2 if pairs else 1, byte_frames=byte_frames, byte_metrics=byte_metrics):
        if not pairs:
            finish(data)
            continue
        if held is None:
            held = data
            continue
        if not _pairable(held, data):
            finish(held)
            held = data
            continue
        if byte_frames or yuv_frames:         # the two clips where they are: no concatenation
            with torch.no_grad():
                torch.cuda.synchronize()
                t0 = time.time()
                kw = dict(yuv_kw) if yuv_frames else {}
                outs = model.generator.forward_clips([tuple(c[k] for k in GENERATOR_INPUTS) for c in (held, data)], out_dtype=out_dtype, **kw)
                torch.cuda.synchronize()
                dt = time.time() - t0
        else:
            both = [torch.cat([held[k], data[k]]) for k in GENERATOR_INPUTS]
            with torch.no_grad():
                torch.cuda.synchronize()
                t0 = time.time()
                out = model.generator(*both)
                torch.cuda.synchronize()
                dt = time.time() - t0
            outs = (out[0:1], out[1:2])
        model.last_forward_seconds = dt
        fps = (_frames(held['lq']) + _frames(data['lq'])) / dt
        finish(held, outs[0], fps)
        finish(data, outs[1], fps)
        held = None
    if held is not None:
        finish(held)
    table = gather_clip_metrics(local, len(dataset), device=device)
    return [dict(eval_result={m: float(table[i, j]) for j, m in enumerate(metrics)}, frames_per_s=float(table[i, -1]))
            for i in range(len(dataset))]
