"""Datasets for the test path.

`SyntheticCompressedClipDataset` produces clips with the tensor contract of the reference's
test pipeline (configs/HR_davis_LR_128x128.py:109-131 ->
lq, gt, mvs, slices, QPs, base_QPs, partitions + meta) from seeds -- there are no datasets in
this environment.  The reference's on-disk loader (LoadImageFromFileList_ipb) is the "next" row
SURVEY.md section 8(f)-1.
"""
from collections import defaultdict

import torch

from . import synthetic as syn
from .registry import DATASETS


class _EvalMixin:
    def evaluate(self, results, logger=None):
        """mmedit/datasets/base_sr_dataset.py:61-93: mean over clips of each metric."""
        if not isinstance(results, list):
            raise TypeError(f'results must be a list, but got {type(results)}')
        assert len(results) == len(self), (
            f'The length of results is not equal to the dataset len: {len(results)} != {len(self)}')
        results = [res['eval_result'] for res in results]
        acc = defaultdict(list)
        for res in results:
            for metric, val in res.items():
                acc[metric].append(val)
        return {metric: sum(values) / len(self) for metric, values in acc.items()}


@DATASETS.register_module()
class SyntheticCompressedClipDataset(_EvalMixin, torch.utils.data.Dataset):
    def __init__(self, num_clips=8, num_input_frames=7, height=128, width=128, slices='IBBBP', qp_mode='qp',
                 crfs=(15, 25, 35), seed=0, repeat=1, test_mode=True, pipeline=None, **unused):
        self.n, self.t, self.h, self.w = num_clips * repeat, num_input_frames, height, width
        self.slices, self.qp_mode, self.crfs, self.seed = slices, qp_mode, tuple(crfs), seed
        self.base_clips = num_clips

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        i = idx % self.base_clips
        clip = syn.make_clip(seed=self.seed * 100003 + i, n=1, t=self.t, h=self.h, w=self.w, slices=self.slices,
                             qp_mode=self.qp_mode, crf=self.crfs[i % len(self.crfs)],
                             block=8 if (self.h % 8 == 0 and self.w % 8 == 0) else 4)
        out = {k: torch.from_numpy(v[0]) for k, v in clip.items()}
        out['meta'] = dict(key=f'{i:03d}/{0:08d}', lq_path=f'synthetic/{i:03d}', gt_path=f'synthetic/{i:03d}')
        return out


@DATASETS.register_module(name='SRREDSMultipleGTCompressDataset')
@DATASETS.register_module()
class CompressedClipFolderDataset(_EvalMixin, torch.utils.data.Dataset):
    """On-disk clips in the reference's layout (mmedit/datasets/sr_reds_multiple_gt_compress_dataset.py +
    pipelines GenerateSegmentIndices_LR / LoadImageFromFileList_ipb / LoadImageFromFileList /
    RescaleToZeroOne / FramesToTensor, configs/HR_davis_LR_128x128.py:109-131):

        <lq_folder>/<clip>/<%08d>.png        e.g. dataset/REDS_test_HR/crf25/png/000/00000000.png
        <lq_folder with 'png'->'mv'>/<clip>/<%08d>.npy   decoder MV records, rows
              (direction, w, h, x_w, y_w, x, y, motion_x, motion_y, scale)
        qp_slice_file: JSON  {crfXX: {clip: {frame: {'slice': 'I|P|B', 'QP': q}}}}
        <gt_folder>/<clip>/<%08d>.png

    Frames, QP / slice side info and the raw MV records are read on the host; the dense motion and
    partition maps are NOT built here -- the records travel to the GPU and pnp_rasterise_side_info_f32
    paints them there (apis.prepare_batch).  Clips are discovered on disk (REDS4 names if present)."""

    REDS4 = ['000', '011', '015', '020']

    def __init__(self, lq_folder, gt_folder, num_input_frames=100, pipeline=None, scale=1, val_partition='REDS4',
                 repeat=1, cprs_folder=None, test_mode=True, qp_slice_file=None, replace_qp_withIPB=False, **unused):
        import json
        import os
        if not isinstance(repeat, int):
            raise TypeError(f'"repeat" must be an integer, but got {type(repeat)}.')
        self.lq_folder, self.gt_folder = str(lq_folder), str(gt_folder)
        self.num_input_frames = num_input_frames
        # the loader options live inside the pipeline list in the reference configs
        for step in (pipeline or []):
            if isinstance(step, dict) and step.get('type', '').startswith('LoadImageFromFileList_ipb'):
                qp_slice_file = step.get('qp_slice_file', qp_slice_file)
                replace_qp_withIPB = step.get('replace_qp_withIPB', replace_qp_withIPB)
        self.replace_qp = bool(replace_qp_withIPB)
        self.table = None
        if qp_slice_file is not None:
            with open(qp_slice_file) as f:
                self.table = json.load(f)
        clips = sorted(d for d in os.listdir(self.lq_folder) if os.path.isdir(os.path.join(self.lq_folder, d)))
        if val_partition == 'REDS4' and all(c in clips for c in self.REDS4):
            clips = list(self.REDS4)
        self.keys = clips * repeat

    def __len__(self):
        return len(self.keys)

    @staticmethod
    def _png(path):
        import numpy as np
        from PIL import Image
        return np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8)

    #: PNG / record files of a clip are decoded on this many threads (PIL and numpy release the GIL while they inflate / read)
    decode_workers = 8

    def _pool(self):
        """the decode pool of THIS process: a forked DataLoader worker inherits the parent's executor object without its threads
        (futures submitted to it would never complete), so the pool is keyed on the pid and re-created after a fork"""
        import os
        pool = getattr(self, '_decode_pool', None)
        if pool is None or pool[0] != os.getpid():
            from concurrent.futures import ThreadPoolExecutor
            pool = self._decode_pool = (os.getpid(), ThreadPoolExecutor(max_workers=self.decode_workers,
                                                                        thread_name_prefix='pnp-decode'))
        return pool[1]

    def __getstate__(self):
        """picklable for spawn-started DataLoader workers: the executor stays behind"""
        state = dict(self.__dict__)
        state.pop('_decode_pool', None)
        return state

    def _read_clip(self, idx):
        """host side of one clip: uint8 HWC frames, side info and raw MV records (files decoded in parallel)"""
        import os
        import numpy as np
        key = self.keys[idx]
        d = os.path.join(self.lq_folder, key)
        names = sorted(f for f in os.listdir(d) if f.endswith('.png'))[:self.num_input_frames]
        crf_dir = self.lq_folder.rstrip('/').split('/')[-2] if '/' in self.lq_folder.rstrip('/') else ''
        base_qp = int(crf_dir.split('crf')[1]) if 'crf' in crf_dir else 0          # loading_ipb.py:239
        pool = self._pool()
        lq_f = [pool.submit(self._png, os.path.join(d, name)) for name in names]
        gt_f = [pool.submit(self._png, os.path.join(self.gt_folder, key, name)) for name in names]
        mv_f = [pool.submit(np.load, os.path.join(d, name).replace('.png', '.npy').replace('png', 'mv'))    # loading_ipb.py:326
                for name in names]
        slices, qps = [], []
        for name in names:
            frame = str(int(name.split('.')[0]))
            if crf_dir.startswith('crf') and self.table is not None:                # loading_ipb.py:298-312
                e = self.table[crf_dir][key][frame]
                sl = e['slice']
                qp = ord(sl) if self.replace_qp else e['QP']
            else:
                sl = 'I' if frame == '0' else 'P'
                qp = ord(sl) if self.replace_qp else 0.0
            slices.append(float(ord(sl)))
            qps.append(float(qp) / 255.0)
        recs = [f.result().astype(np.float32).reshape(-1, 10) for f in mv_f]
        rec_frame = [np.full((r.shape[0],), t, np.int32) for t, r in enumerate(recs)]
        T = len(names)
        side = dict(slices=torch.tensor(slices, dtype=torch.float32).view(T, 1, 1, 1),
                    QPs=torch.tensor(qps, dtype=torch.float32).view(T, 1, 1, 1),
                    base_QPs=torch.full((T, 1, 1, 1), base_qp / 255.0, dtype=torch.float32),
                    mv_records=torch.from_numpy(np.concatenate(recs) if recs else np.zeros((0, 10), np.float32)),
                    rec_frame=torch.from_numpy(np.concatenate(rec_frame) if rec_frame else np.zeros((0,), np.int32)),
                    meta=dict(key=f'{key}/{0:08d}', lq_path=d, gt_path=os.path.join(self.gt_folder, key)))
        return np.stack([f.result() for f in lq_f]), np.stack([f.result() for f in gt_f]), side

    def __getitem__(self, idx):
        """the reference pipeline's sample: RescaleToZeroOne + FramesToTensor give float32 (T,3,H,W) frames in [0,1]"""
        import numpy as np
        lq, gt, side = self._read_clip(idx)
        f32 = lambda a: torch.from_numpy(a.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
        return dict(lq=f32(lq), gt=f32(gt), **side)

    def get_uint8(self, idx):
        """the same sample with the frames still uint8 (T,H,W,3) under lq_u8 / gt_u8: a quarter of the host and PCIe bytes; the
        consumer (apis.ClipPrefetcher) divides by 255 and transposes on the device -- the same IEEE fp32 division, bit-identical"""
        lq, gt, side = self._read_clip(idx)
        return dict(lq_u8=torch.from_numpy(lq), gt_u8=torch.from_numpy(gt), **side)


@DATASETS.register_module()
class Yuv420ClipFolderDataset(_EvalMixin, torch.utils.data.Dataset):
    """Raw 8-bit 4:2:0 clips, what a decoder writes with `-pix_fmt yuv420p` (or nv12 / nv21) -- the frames never become RGB on the way
    to the generator or to the metrics (apis.multi_gpu_test(yuv_frames=True)):

        <lq_folder>/<clip>.yuv           raw frames back to back, layout 'i420' (yuv420p, default) | 'nv12' | 'nv21', tightly packed
        <gt_folder>/<clip>.yuv           the same, scale*height x scale*width
        <mv_folder>/<clip>/<%08d>.npy    the decoder MV records of CompressedClipFolderDataset, one file per frame
        qp_slice_file                    the same JSON {crfXX: {clip: {frame: {'slice': 'I|P|B', 'QP': q}}}}

    height, width: the frame size of the lq clips (a raw file does not carry it).  mv_folder defaults to lq_folder with its last
    'yuv' path component replaced by 'mv'; the base QP comes from the crfNN path component, as in CompressedClipFolderDataset.
    A sample carries lq_yuv / gt_yuv, packed uint8 (T, 3h/2, w) buffers as on disk, the side info and MV records of the PNG dataset,
    and meta with `layout`, `yuv_standard` and `chroma` -- where the clips' chroma samples lie: 'replicate' (default) | 'center' |
    'left' (H.264 / HEVC / VVC streams) | 'topleft' (BT.2020 / UHD), the chroma modes of include/pnpvcve.h.
    bit_depth 10 | 12: the files hold 16-bit little-endian samples (`-pix_fmt yuv420p10le` / `yuv420p12le`, VTM / HM output; with
    msb_aligned the value sits in the word's high bits, as in P010 / P012 with layout 'nv12'), a frame is 3 h w bytes, the buffers are
    int16 (T, 3h/2, w) -- the words as they are, uploaded as they are -- and meta carries `bit_depth` and `msb_aligned`.
    4:2:2 and 4:4:4 clips (HEVC RExt / VVC streams, what HM and VTM write for those profiles): layout 'yuv422p' | 'nv16' | 'yuv444p' |
    'nv24' names the plane order AND implies the chroma format (meta `format`: '420' | '422' | '444'); a frame is 2hw or 3hw samples,
    the buffers (T, 2h, w) or (T, 3h, w); with bit_depth 10 | 12 the same order applies in words ('yuv422p' reads yuv422p10le, 'nv16'
    with msb_aligned P210, ...).  4:2:2 needs an even width only, 4:4:4 no parity."""

    def __init__(self, lq_folder, gt_folder, height, width, layout='i420', yuv_standard='bt601-limited', mv_folder=None,
                 num_input_frames=100, scale=1, repeat=1, qp_slice_file=None, replace_qp_withIPB=False, pipeline=None, test_mode=True,
                 bit_depth=8, msb_aligned=False, chroma='replicate', **unused):
        import json
        import os
        if not isinstance(repeat, int):
            raise TypeError(f'"repeat" must be an integer, but got {type(repeat)}.')
        formats = {'yuv422p': '422', 'nv16': '422', 'yuv444p': '444', 'nv24': '444'}      # the layout implies the chroma format
        if layout not in ('i420', 'nv12', 'nv21') and layout not in formats:
            raise ValueError(f"layout must be 'i420', 'nv12' or 'nv21', or {tuple(formats)} for 4:2:2 / 4:4:4 clips, got {layout!r}")
        self.format = formats.get(layout, '420')
        if yuv_standard not in ('bt601-limited', 'bt601-full', 'bt709-limited', 'bt709-full'):
            raise ValueError(f'unknown yuv_standard {yuv_standard!r}')
        if chroma not in ('replicate', 'center', 'left', 'topleft'):
            raise ValueError(f"chroma must be 'replicate', 'center', 'left' or 'topleft', got {chroma!r}")
        self.chroma = chroma
        if isinstance(bit_depth, bool) or bit_depth not in (8, 10, 12):
            raise ValueError(f'bit_depth must be 8, 10 or 12, got {bit_depth!r}')
        if msb_aligned and bit_depth == 8:
            raise ValueError('msb_aligned describes 16-bit containers: bit_depth 10 or 12')
        self.bit_depth, self.msb_aligned = int(bit_depth), bool(msb_aligned)
        self.h, self.w, self.scale = int(height), int(width), int(scale)
        if self.format == '420' and (self.h < 2 or self.w < 2 or self.h % 2 or self.w % 2 or self.scale < 1):
            raise ValueError(f'4:2:0 frames need an even height and width (and scale >= 1), got {height} x {width}, scale {scale}')
        if self.h < 1 or self.w < 1:
            raise ValueError(f'4:{self.format[1]}:{self.format[2]} frames need a height and a width of at least 1, got {height} x {width}')
        if self.scale < 1:
            raise ValueError(f'scale must be at least 1, got {scale}')
        if self.format == '422' and self.w % 2:
            raise ValueError(f'4:2:2 frames need an even width, got {height} x {width}')
        self.lq_folder, self.gt_folder = str(lq_folder), str(gt_folder)
        self.layout, self.yuv_standard, self.num_input_frames = layout, yuv_standard, int(num_input_frames)
        if mv_folder is None:
            parts = self.lq_folder.rstrip('/').split('/')
            where = [i for i, p in enumerate(parts) if p == 'yuv']
            if not where:
                raise ValueError(f"mv_folder is not given and lq_folder {self.lq_folder!r} has no 'yuv' path component to replace by 'mv'")
            parts[where[-1]] = 'mv'
            mv_folder = '/'.join(parts)
        self.mv_folder = str(mv_folder)
        self.replace_qp = bool(replace_qp_withIPB)
        self.table = None
        if qp_slice_file is not None:
            with open(qp_slice_file) as f:
                self.table = json.load(f)
        clips = sorted(f[:-4] for f in os.listdir(self.lq_folder) if f.endswith('.yuv'))
        self.keys = clips * repeat

    def __len__(self):
        return len(self.keys)

    @staticmethod
    def _read_yuv(path, h, w, max_frames, bit_depth=8, fmt='420'):
        """-> the first min(frames in the file, max_frames) frames as (T, 3h/2, w) uint8 (4:2:2: 2h rows, a frame is 2hw samples; 4:4:4:
        3h rows, 3hw samples), or int16 words (little-endian in the file) for bit_depth 10 | 12"""
        import os
        import numpy as np
        wide = bit_depth != 8
        rows = {'420': h * 3 // 2, '422': 2 * h, '444': 3 * h}[fmt]
        per = rows * w * (2 if wide else 1)
        size = os.path.getsize(path)
        if size < per or size % per:
            raise ValueError(f'{path}: {size} bytes is not a whole number (>= 1) of {h} x {w} {bit_depth}-bit 4:{fmt[1]}:{fmt[2]} frames of {per} bytes')
        t = min(size // per, max_frames)
        if wide:
            return np.fromfile(path, dtype='<i2', count=t * per // 2).astype(np.int16, copy=False).reshape(t, rows, w)
        return np.fromfile(path, dtype=np.uint8, count=t * per).reshape(t, rows, w)

    def __getitem__(self, idx):
        import os
        import numpy as np
        key = self.keys[idx]
        lq_path, gt_path = os.path.join(self.lq_folder, key + '.yuv'), os.path.join(self.gt_folder, key + '.yuv')
        lq = self._read_yuv(lq_path, self.h, self.w, self.num_input_frames, self.bit_depth, self.format)
        T = lq.shape[0]
        gt = self._read_yuv(gt_path, self.h * self.scale, self.w * self.scale, T, self.bit_depth, self.format)
        if gt.shape[0] != T:
            raise ValueError(f'{gt_path}: {gt.shape[0]} frames for the {T} of {lq_path}')
        parts = self.lq_folder.rstrip('/').split('/')
        crf_dir = parts[-2] if len(parts) > 1 else ''
        base_qp = int(crf_dir.split('crf')[1]) if 'crf' in crf_dir else 0          # loading_ipb.py:239
        slices, qps, recs = [], [], []
        for i in range(T):
            frame = str(i)
            if crf_dir.startswith('crf') and self.table is not None:                # loading_ipb.py:298-312
                e = self.table[crf_dir][key][frame]
                sl = e['slice']
                qp = ord(sl) if self.replace_qp else e['QP']
            else:
                sl = 'I' if i == 0 else 'P'
                qp = ord(sl) if self.replace_qp else 0.0
            slices.append(float(ord(sl)))
            qps.append(float(qp) / 255.0)
            recs.append(np.load(os.path.join(self.mv_folder, key, f'{i:08d}.npy')).astype(np.float32).reshape(-1, 10))
        rec_frame = [np.full((r.shape[0],), t, np.int32) for t, r in enumerate(recs)]
        return dict(lq_yuv=torch.from_numpy(lq), gt_yuv=torch.from_numpy(gt),
                    slices=torch.tensor(slices, dtype=torch.float32).view(T, 1, 1, 1),
                    QPs=torch.tensor(qps, dtype=torch.float32).view(T, 1, 1, 1),
                    base_QPs=torch.full((T, 1, 1, 1), base_qp / 255.0, dtype=torch.float32),
                    mv_records=torch.from_numpy(np.concatenate(recs)), rec_frame=torch.from_numpy(np.concatenate(rec_frame)),
                    meta=dict(key=f'{key}/{0:08d}', lq_path=lq_path, gt_path=gt_path, layout=self.layout, yuv_standard=self.yuv_standard,
                              bit_depth=self.bit_depth, msb_aligned=self.msb_aligned, chroma=self.chroma, format=self.format))


def collate(batch):
    """samples_per_gpu=1 (forced by the reference, tools/test.py:110): add the batch dim."""
    out = {}
    for k in batch[0]:
        if k == 'meta':
            out[k] = [b[k] for b in batch]
        elif k in ('mv_records', 'rec_frame'):      # ragged per clip: samples_per_gpu is 1
            assert len(batch) == 1
            out[k] = batch[0][k]
        else:
            out[k] = torch.stack([b[k] for b in batch])
    return out


def build_dataset(cfg, default_args=None):
    from .registry import build_from_cfg
    return build_from_cfg(cfg, DATASETS, default_args)
