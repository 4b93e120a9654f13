"""`BasicVSR` -- the model wrapper the reference's configs name (model.type).

Reproduces the test-time surface of mmedit/models/restorers/basicvsr.py:33-233 and
basic_restorer.py:49-98: constructor keys, forward(test_mode=True, **data) plumbing of the
side-information tensors into generator(lq, QPs, slices, mvs, base_QPs, partitions), per-frame
PSNR/SSIM on uint8-rounded BGR frames averaged over the clip, optional PNG dump.
Training (forward_train / train_step) is out of scope for this build and raises.
"""
import os.path as osp
import time

import numpy as np
import torch
import torch.nn as nn

from .metrics import ALLOWED_METRICS, GAIN_METRICS, GAIN_PLANE_METRICS, tensor2img
from .registry import LOSSES, MODELS, build_backbone, build_loss


@LOSSES.register_module()
class CharbonnierLoss(nn.Module):
    """mmedit/models/losses/pixelwise_loss.py:139-184 -- accepted so that configs build; only
    used by training, which this build does not provide."""

    def __init__(self, loss_weight=1.0, reduction='mean', sample_wise=False, eps=1e-12):
        super().__init__()
        self.loss_weight, self.reduction, self.sample_wise, self.eps = loss_weight, reduction, sample_wise, eps

    def forward(self, pred, target, weight=None, **kwargs):
        loss = torch.sqrt((pred - target) ** 2 + self.eps)
        if weight is not None:
            loss = loss * weight
        loss = loss.mean() if self.reduction == 'mean' else (loss.sum() if self.reduction == 'sum' else loss)
        return self.loss_weight * loss


@MODELS.register_module()
class BasicVSR(nn.Module):
    allowed_metrics = ALLOWED_METRICS

    def __init__(self, generator, pixel_loss=None, ensemble=None, train_cfg=None, test_cfg=None, psnr_only=False,
                 pretrained=None):
        super().__init__()
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.psnr_only = psnr_only
        self.generator = build_backbone(generator)
        self.pixel_loss = build_loss(pixel_loss) if pixel_loss else None
        # basicvsr.py:52-64.  The reference's SpatialTemporalEnsemble calls the generator with the frames only and cannot run this one;
        # here the switch selects generator.forward_ensemble, which transforms the side information with the frames
        self.forward_ensemble = None
        self.is_temporal_ensemble = False
        if ensemble is not None:
            if ensemble['type'] == 'SpatialTemporalEnsemble':
                self.is_temporal_ensemble = bool(ensemble.get('is_temporal_ensemble', False))
                self.forward_ensemble = self._forward_ensemble
            else:
                raise NotImplementedError('Currently support only "SpatialTemporalEnsemble", but got type '
                                          f'[{ensemble["type"]}]')
        self.fix_iter = train_cfg.get('fix_iter', 0) if train_cfg else 0
        self.is_weight_fixed = False
        self.register_buffer('step_counter', torch.zeros(1))          # basicvsr.py:50
        self.last_forward_seconds = None
        if pretrained is not None:
            self.generator.init_weights(pretrained)

    # mmcv's mixed-precision switch (basic_restorer.py:45-46 `self.fp16_enabled = False`, set by wrap_fp16_model): here it
    # selects the generator's fp16-operand conv kernels (BASELINE configs[4]); the default stays exact fp32.
    @property
    def fp16_enabled(self):
        return self.generator.fp16_enabled

    @fp16_enabled.setter
    def fp16_enabled(self, value):
        self.generator.fp16_enabled = bool(value)

    # the native precision switch in full ('fp32' | 'fp16' | 'f16x3'; generator.precision)
    @property
    def precision(self):
        return self.generator.precision

    @precision.setter
    def precision(self, value):
        self.generator.precision = value

    def _forward_ensemble(self, lq, QPs, slices, mvs, base_QPs, par_map, **kw):
        return self.generator.forward_ensemble(lq, QPs, slices, mvs, base_QPs, par_map, temporal=self.is_temporal_ensemble, **kw)

    def check_if_mirror_extended(self, lrs):
        """basicvsr.py:52-68."""
        is_mirror_extended = False
        if lrs.size(1) % 2 == 0:
            lrs_1, lrs_2 = torch.chunk(lrs, 2, dim=1)
            if lrs.dtype == torch.uint8:        # byte frames (n,t,h,w,3): the same test, exact on integers
                return torch.equal(lrs_1, lrs_2.flip(1))
            if torch.norm(lrs_1 - lrs_2.flip(1)) == 0:
                is_mirror_extended = True
        return is_mirror_extended

    def forward(self, lq, gt=None, QPs=None, slices=None, mvs=None, base_QPs=None, partitions=None, test_mode=False,
                **kwargs):
        """basic_restorer.py:64-98."""
        if test_mode:
            return self.forward_test(lq, gt, QPs, slices, mvs, base_QPs, partitions, **kwargs)
        raise NotImplementedError('training is out of scope of the MI355X hot-path build')

    def evaluate(self, output, gt, lq=None, par_map=None):
        """basicvsr.py:119-153.
        Enhancement gain (not in the reference; include/pnpvcve.h, pnp_gain_*): with `lq`, the compressed input the generator was given,
        the names of metrics.GAIN_METRICS -- 'PSNR_LQ', 'SSIM_LQ' (lq against gt), 'dPSNR', 'dSSIM' (the mean over frames of the output's
        value minus lq's), 'PSNR_SD', 'PSNR_SD_LQ' (the population standard deviation of the frames' PSNR) -- are served on every kind
        of clip, and on clips of planes also their `_U` / `_V` forms and 'dPSNR_YUV' (6:1:1; KeyError on RGB clips, as 'PSNR_YUV').
        test_cfg.get('gain_block', 64) is the cell size; `par_map` (the generator's partition map) adds the per-class sums to
        self.last_gain, which test_cfg.gain_report writes out (forward_test).  A gain name without lq, with a vsr generator (lq is a
        quarter of the size) or with an lq of another frame class, size or bit depth raises ValueError before any GPU work.  Every
        other result is what it was.
        4:2:0 clips (not in the reference): when `output` and `gt` are both ops.Yuv420Frames -- one clip, (t,...) or (1,t,...) views,
        each in a layout of its own -- the metrics are PLANE metrics read from the 8-bit planes on the device (ops.psnr_yuv420 /
        ssim_yuv420 / msssim_yuv420): 'PSNR' / 'SSIM' / 'MS-SSIM' score the Y plane, and in this mode only 'PSNR_U', 'PSNR_V', 'SSIM_U',
        'SSIM_V', 'MS-SSIM_U', 'MS-SSIM_V' and 'PSNR_YUV' = (6 PSNR_Y + PSNR_U + PSNR_V) / 8 per frame are accepted too; every value is
        the mean over frames.  'XPSNR', 'XPSNR_U', 'XPSNR_V' (this mode only; include/pnpvcve.h) are the activity-weighted PSNR of the
        planes with `gt` as the original and test_cfg.get('xpsnr_fps', 30) frames per second; their value is the CLIP's, the log of the
        mean weighted error over the frames, not the mean of the frames' dB.  'PSNR-B', 'PSNR-B_U', 'PSNR-B_V' (include/pnpvcve.h) are the
        blocking-aware PSNR of the planes, the output being the test clip, with blocks of test_cfg.get('psnrb_block', 8) on Y and half of
        that on chroma, the mean over frames; 'PSNR-B' is served on RGB / Y clips too (the `_U` / `_V` names raise KeyError there).
        'MS-SSIM' (five scales; include/pnpvcve.h) is served on the device path of RGB / Y clips too and needs 176 x 176 samples of every plane it scores after the crop.  crop_border (even)
        crops the Y plane, half of it the chroma planes.  test_cfg.convert_to may be None or 'y' and both mean the same here: the decoder's
        Y' plane IS the luma -- it is NOT the BT.601 Y that convert_to='y' derives from RGB bytes, so the two modes' numbers differ.
        Two ops.Yuv420Frames16 of one bit depth d are scored the same way on their sample values, with the peak 2^d - 1."""
        from .ops import is_yuv
        if is_yuv(output) or is_yuv(gt):
            if not (is_yuv(output) and type(output) is type(gt)):      # (one chroma format and one sample size: one frame class)
                raise ValueError('plane metrics compare two clips of one chroma format and sample size: output and gt must both be '
                                 "ops.Yuv420Frames (ask the generator for out_dtype='i420' / 'nv12', or convert with ops.frames_to_yuv420), "
                                 'both ops.Yuv420Frames16 of one bit depth, or both the same 4:2:2 / 4:4:4 class (ops.Yuv422Frames, '
                                 f'Yuv444Frames, their 16 forms; ops.frames_to_yuv): got {type(output).__name__} and {type(gt).__name__}')
            self._gain_check(output, lq)
            return self._evaluate_yuv(output, gt, lq, par_map)
        self._gain_check(output, lq)
        crop_border = self.test_cfg['crop_border']
        convert_to = self.test_cfg.get('convert_to', None)
        eval_result = dict()
        if output.ndim == 5 and output.size(0) != 1:
            # the reference evaluates with samples_per_gpu=1 (configs/*: test_dataloader); with n > 1 its tensor2img
            # would compare make_grid mosaics of the batch.  Refuse loudly instead of scoring sample 0 only.
            raise ValueError(f'evaluate() expects one clip per call (samples_per_gpu=1), got a batch of {output.size(0)}')
        # byte clips (1,t,h,w,3) uint8 count as 5-D clips; the device path serves convert_to None and 'y' / 'Y' and reads either
        # layout as it is (ops.psnr_frames / ssim_frames): two byte clips cost 6 B per pixel, no fp32 copy of either
        on_device = output.is_cuda and output.ndim == 5 and (convert_to is None or (isinstance(convert_to, str) and convert_to.lower() == 'y'))
        if (output.dtype == torch.uint8 or gt.dtype == torch.uint8) and not on_device:
            raise ValueError('uint8 frames are evaluated on the device: a (1,t,h,w,3) clip on the GPU and convert_to None or "Y"')

        def frames_of(x):      # one clip without its batch dimension, on the output's device, in a dtype the kernels read
            x = x[0].to(output.device)
            return x if x.dtype == torch.uint8 else x.float()

        for metric in self.test_cfg['metrics']:
            if metric in GAIN_PLANE_METRICS:
                raise KeyError(metric)                  # a plane metric, as 'PSNR_YUV': clips of planes only
        gain = self._gain_frames(output, gt, lq, par_map, crop_border, convert_to, on_device, frames_of) if self._gain_wanted() else {}
        for metric in self.test_cfg['metrics']:
            if metric in GAIN_METRICS:
                eval_result[metric] = gain[metric]
                continue
            if metric == 'PSNR' and on_device:
                # on-device statistic (pnp_psnr_stat_io): 8 bytes per frame (or per block, for Y) cross PCIe instead of the frames
                from .ops import psnr_frames
                per_frame = psnr_frames(frames_of(output), frames_of(gt), crop_border, convert_to)
                eval_result[metric] = float(per_frame.mean())
                continue
            if metric == 'SSIM' and on_device:
                from .ops import ssim_frames           # pnp_ssim_partials_io (fp64 on the GPU)
                per_frame = ssim_frames(frames_of(output), frames_of(gt), crop_border, convert_to)
                eval_result[metric] = float(per_frame.mean())
                continue
            if metric == 'MS-SSIM' and on_device:
                from .ops import msssim_frames         # pnp_msssim_partials_io (five scales, fp64 on the GPU)
                per_frame = msssim_frames(frames_of(output), frames_of(gt), crop_border, convert_to)
                eval_result[metric] = float(per_frame.mean())
                continue
            if metric == 'PSNR-B' and on_device:
                from .ops import psnrb_frames          # pnp_psnrb_sums_io: the output is the test clip, whose block edges are measured
                per_frame = psnrb_frames(frames_of(output), frames_of(gt), crop_border, convert_to, self.test_cfg.get('psnrb_block', 8))
                eval_result[metric] = float(per_frame.mean())
                continue
            kw = dict(convert_to=convert_to)
            if metric == 'PSNR-B':
                kw['block'] = self.test_cfg.get('psnrb_block', 8)
            if output.ndim == 5:
                avg = []
                for i in range(output.size(1)):
                    avg.append(self.allowed_metrics[metric](tensor2img(output[:, i]), tensor2img(gt[:, i]), crop_border, **kw))
                eval_result[metric] = np.mean(avg)
            else:
                eval_result[metric] = self.allowed_metrics[metric](tensor2img(output), tensor2img(gt), crop_border, **kw)
        return eval_result

    # ---- enhancement gain (include/pnpvcve.h, pnp_gain_*): the output against the compressed input, both scored against gt
    def _gain_names(self):
        return [m for m in ((self.test_cfg or {}).get('metrics', None) or ()) if m in GAIN_METRICS or m in GAIN_PLANE_METRICS]

    def _gain_wanted(self):
        return bool(self._gain_names()) or bool((self.test_cfg or {}).get('gain_report', None))

    def _gain_check(self, output, lq):
        """what the gain refuses, before any GPU work: no lq, a vsr generator, an lq of another frame class, bit depth or size"""
        from .metrics import gain_block
        from .ops import _YUV16_CLASSES, is_yuv, yuv_format
        self.last_gain = None
        if not self._gain_wanted():
            return
        names = self._gain_names() or ['test_cfg.gain_report']
        if lq is None:
            raise ValueError(f'{names} compare the output with the compressed input: evaluate() needs lq, the frames the generator was given '
                             '(forward_test passes them on)')
        if getattr(self.generator, 'vsr', False):
            raise ValueError(f'{names} with a vsr generator: lq is a quarter of the output size, so the gain over it is not defined')
        gain_block(self.test_cfg.get('gain_block', 64))
        if is_yuv(output) != is_yuv(lq):
            raise ValueError(f'{names}: lq and the output must be of one frame class, got {type(lq).__name__} and {type(output).__name__}')
        if is_yuv(output):
            depth = lambda x: int(x.bit_depth) if isinstance(x, _YUV16_CLASSES) else 8
            if depth(lq) != depth(output):
                raise ValueError(f'{names}: lq has {depth(lq)}-bit samples and the output {depth(output)}-bit: the gain compares clips of one bit depth')
            if yuv_format(lq) != yuv_format(output):
                raise ValueError(f'{names}: lq is a {yuv_format(lq)} clip and the output a {yuv_format(output)} clip')
            if tuple(lq.y.shape[-3:]) != tuple(output.y.shape[-3:]):
                raise ValueError(f'{names}: lq shows {tuple(lq.y.shape[-3:])} and the output {tuple(output.y.shape[-3:])} (frames, rows, columns)')
            return
        if output.ndim != 5 or lq.ndim != 5:
            raise ValueError(f'{names} are a clip\'s: the centre-frame output has no frame of lq to be compared with')
        size = lambda x: (x.shape[1],) + (tuple(x.shape[2:4]) if x.dtype == torch.uint8 else tuple(x.shape[3:5]))
        if size(lq) != size(output) or lq.size(0) != output.size(0):
            raise ValueError(f'{names}: lq shows {size(lq)} and the output {size(output)} (frames, rows, columns)')

    @staticmethod
    def _gain_results(names, pa, pl, dp, ssim_a=None, ssim_l=None, suffix=''):
        """the clip's values of the names that end in `suffix` from the frames' values (float64 numpy arrays)"""
        from .metrics import gain_sd
        out = {}
        for m in names:
            base = m[:-len(suffix)] if suffix and m.endswith(suffix) else (m if not suffix else None)
            if base == 'PSNR_LQ':
                out[m] = float(np.mean(pl))
            elif base == 'dPSNR':
                out[m] = float(np.mean(dp))
            elif base == 'PSNR_SD' and not suffix:
                out[m] = gain_sd(pa)
            elif base == 'PSNR_SD_LQ' and not suffix:
                out[m] = gain_sd(pl)
            elif base == 'SSIM_LQ':
                out[m] = float(np.mean(ssim_l))
            elif base == 'dSSIM':
                out[m] = float(np.mean(ssim_a - ssim_l))
        return out

    def _gain_frames(self, output, gt, lq, par_map, crop_border, convert_to, on_device, frames_of):
        """the gain names of an RGB / Y clip (1,t,...): the device's sums (ops.gain_sums_frames, one launch for both halves) or, for host
        tensors, the numpy path's (metrics.gain_sums); the values are metrics.gain_values' either way.  Leaves self.last_gain."""
        from . import metrics
        names = self._gain_names()
        block = metrics.gain_block(self.test_cfg.get('gain_block', 64))
        is_y = isinstance(convert_to, str) and convert_to.lower() == 'y'
        want_ssim = any(m in ('SSIM_LQ', 'dSSIM') for m in names)
        ssim_a = ssim_l = None
        if on_device:
            from .ops import gain_sums_frames, ssim_frames
            a, l, g = frames_of(output), frames_of(lq), frames_of(gt)
            par = None if par_map is None else par_map.to(output.device).float().reshape((-1,) + tuple(par_map.shape[-3:]))
            grid, classes = gain_sums_frames(a, l, g, crop_border, convert_to, block, par)
            grid, classes = grid.numpy()[:, 0], (None if classes is None else classes.numpy())
            if want_ssim:       # the existing SSIM entry, called twice
                ssim_a, ssim_l = (ssim_frames(x, g, crop_border, convert_to).numpy() for x in (a, l))
            h, w = (a.shape[-3:-1] if a.dtype == torch.uint8 else a.shape[-2:])
        else:
            if convert_to is not None and not is_y:
                raise ValueError('Wrong color model. Supported values are "Y" and None.')
            t = output.size(1)
            imgs = [np.stack([tensor2img(x[:, i]) for i in range(t)]) for x in (output, lq, gt)]          # (t,h,w,3) BGR bytes
            if want_ssim:
                ssim_a, ssim_l = (np.array([self.allowed_metrics['SSIM'](x[i], imgs[2][i], crop_border, convert_to=convert_to) for i in range(t)])
                                  for x in imgs[:2])
            if is_y:
                imgs = [np.stack([metrics.bgr2y(f.astype(np.float32) / 255.) * 255. for f in x]) for x in imgs]
            par = None if par_map is None else par_map.detach().cpu().float().numpy().reshape((-1,) + tuple(par_map.shape[-3:]))
            grid, classes = metrics.gain_sums(imgs[0], imgs[1], imgs[2], crop_border, block, par=par)
            grid = grid[:, 0]
            h, w = imgs[0].shape[1:3]
        ch = 1 if is_y else 3
        counts = metrics.gain_cell_counts(int(h), int(w), crop_border, block) * ch
        e = metrics.gain_frame_sums(grid)
        pa, pl, dp = metrics.gain_values(e[:, 0], e[:, 1], float(counts.sum()), 255.0)
        self.last_gain = dict(grid=grid, counts=counts, peak=255.0, classes=classes, class_samples=ch, ssim=ssim_a, ssim_lq=ssim_l, block=block)
        return self._gain_results(names, pa, pl, dp, ssim_a, ssim_l)

    def _gain_yuv(self, output, gt, lq, par_map, crop_border):
        """the gain names of a clip of planes: ops.gain_sums_yuv on the planes the names ask for (Y always: the report is the Y plane's)"""
        from . import metrics
        from .ops import _YUV16_CLASSES, _plane_geometry, gain_sums_yuv, ssim_yuv, yuv_format
        names = self._gain_names()
        block = metrics.gain_block(self.test_cfg.get('gain_block', 64))
        need = lambda s: any(m.endswith(s) for m in names) or 'dPSNR_YUV' in names
        planes = 'y' + ('u' if need('_U') else '') + ('v' if need('_V') else '')
        par = None if par_map is None else par_map.to(output.y.device).float().reshape((-1,) + tuple(par_map.shape[-3:]))
        grid, classes = gain_sums_yuv(output, lq, gt, crop_border, planes, block, par)
        grid = grid.numpy()
        h, w = (int(x) for x in output.y.shape[-2:])
        fmt = yuv_format(output)
        sx, sy = metrics.GAIN_FACTORS[fmt]
        peak = float((1 << output.bit_depth) - 1) if isinstance(output, _YUV16_CLASSES) else 255.0
        scol = {'y': ('SSIM_LQ', 'dSSIM'), 'u': ('SSIM_LQ_U', 'dSSIM_U'), 'v': ('SSIM_LQ_V', 'dSSIM_V')}
        splanes = ''.join(p for p in planes if any(m in names for m in scol[p]))
        ssim_a = ssim_l = None
        if splanes:             # the existing SSIM entries, called twice
            ssim_a, ssim_l = (ssim_yuv(x, gt, crop_border, splanes).numpy() for x in (output, lq))
        out, d = {}, {}
        for k, p in enumerate(planes):
            counts = metrics.gain_cell_counts(h, w, crop_border, block, *((1, 1) if p == 'y' else (sx, sy)))
            e = metrics.gain_frame_sums(grid[:, k])
            pa, pl, d[p] = metrics.gain_values(e[:, 0], e[:, 1], float(counts.sum()), peak)
            sa, sl = (None, None) if p not in splanes else (ssim_a[:, splanes.index(p)], ssim_l[:, splanes.index(p)])
            out.update(self._gain_results([m for m in names if m != 'dPSNR_YUV'], pa, pl, d[p], sa, sl, suffix={'y': '', 'u': '_U', 'v': '_V'}[p]))
            if p == 'y':
                self.last_gain = dict(grid=grid[:, 0], counts=counts, peak=peak, classes=None if classes is None else classes.numpy(),
                                      class_samples=1, ssim=sa, ssim_lq=sl, block=block)
        if 'dPSNR_YUV' in names:
            out['dPSNR_YUV'] = float(np.mean(metrics.gain_yuv(d['y'], d['u'], d['v'])))
        return out

    def _gain_report(self, meta, slices, QPs, base_QPs):
        """test_cfg.gain_report = DIR: one <clip>.json per clip scored (metrics.gain_report of the sums evaluate() left), as save_path
        gets one file per clip; the QPs are written as the codec's numbers (the tensors carry qp / 255)"""
        import json
        import os
        from .metrics import gain_report
        folder = (self.test_cfg or {}).get('gain_report', None)
        if not folder or self.last_gain is None:
            return
        qp = lambda x: None if x is None else np.round(x.detach().cpu().double().reshape(-1).numpy() * 255.0, 3)
        sl = None if slices is None else slices.detach().cpu().reshape(-1).numpy()
        doc = gain_report(slices=sl, qps=qp(QPs), base_qps=qp(base_QPs), **self.last_gain)
        clip = meta[0]['key'].split('/')[0] if meta else 'clip'
        doc['clip'] = clip
        os.makedirs(folder, exist_ok=True)
        with open(osp.join(folder, f'{clip}.json'), 'w') as f:
            json.dump(doc, f, indent=1)

    # the packed layouts generator.forward writes: 4:2:0, then 4:2:2 and 4:4:4 (ops.YUV_FORMAT_LAYOUTS)
    YUV_OUT_LAYOUTS = ('nv12', 'i420', 'p010', 'p012', 'yuv420p10le', 'yuv420p12le', 'yuv422p', 'nv16', 'yuv444p', 'nv24', 'yuv422p10le',
                       'yuv422p12le', 'yuv444p10le', 'yuv444p12le', 'p210', 'p212', 'p410', 'p412')
    # what 4:2:2 and 4:4:4 clips are scored by (the gain names are served wherever PSNR and SSIM are)
    YUV_FORMAT_METRICS = ('PSNR', 'SSIM', 'PSNR_U', 'PSNR_V', 'SSIM_U', 'SSIM_V', 'PSNR_YUV') + GAIN_METRICS + GAIN_PLANE_METRICS
    YUV_METRICS = ('PSNR', 'SSIM', 'PSNR_U', 'PSNR_V', 'SSIM_U', 'SSIM_V', 'PSNR_YUV', 'MS-SSIM', 'MS-SSIM_U', 'MS-SSIM_V', 'XPSNR', 'XPSNR_U',
                   'XPSNR_V', 'PSNR-B', 'PSNR-B_U', 'PSNR-B_V') + GAIN_METRICS + GAIN_PLANE_METRICS

    def _evaluate_yuv(self, output, gt, lq=None, par_map=None):
        """evaluate() of two ops.Yuv420Frames (or two ops.Yuv420Frames16) clips: plane PSNR / SSIM on the device, means over the clip's frames.
        Two clips of one 4:2:2 or 4:4:4 class are scored by YUV_FORMAT_METRICS through ops.psnr_yuv / ops.ssim_yuv; MS-SSIM, XPSNR and
        PSNR-B are defined on 4:2:0 clips only and raise a ValueError that names the format."""
        from .ops import msssim_yuv420, psnr_yuv, psnrb_yuv420, ssim_yuv, xpsnr_yuv420, yuv_format
        # PSNR and SSIM go through the format-generic functions for every clip (at 4:2:0 they are the _yuv420 entries called with format
        # 0: the same numbers); the other three metrics are defined on 4:2:0 clips only and refused for the other formats below
        fmt = yuv_format(output)
        crop_border = self.test_cfg['crop_border']
        convert_to = self.test_cfg.get('convert_to', None)
        if not (convert_to is None or (isinstance(convert_to, str) and convert_to.lower() == 'y')):
            raise ValueError('Wrong color model. Supported values are "Y" and None.')
        metrics = list(self.test_cfg['metrics'])
        for metric in metrics:
            if metric not in self.YUV_METRICS:
                raise ValueError(f'clips of planes are scored by {self.YUV_METRICS} (4:2:0; 4:2:2 and 4:4:4: {self.YUV_FORMAT_METRICS}), got {metric!r}')
            if fmt != '420' and metric not in self.YUV_FORMAT_METRICS:
                raise ValueError(f'{metric!r} is defined on 4:2:0 clips only: 4:{fmt[1]}:{fmt[2]} clips are scored by {self.YUV_FORMAT_METRICS}')

        def one_clip(x, name):
            if x.y.dim() == 4:
                if x.y.size(0) != 1:
                    raise ValueError(f'evaluate() expects one clip per call (samples_per_gpu=1), got a batch of {x.y.size(0)}')
                return type(x)(x.y[0], x.cb[0], x.cr[0], *x[3:])
            return x

        output, gt = one_clip(output, 'output'), one_clip(gt, 'gt')
        gt = type(gt)(*[p.to(output.y.device) for p in gt[:3]], *gt[3:])
        eval_result = dict()
        gain = {}
        if self._gain_wanted():         # (refused before this point without lq or with an lq of another kind: _gain_check)
            lq = one_clip(lq, 'lq')
            gain = self._gain_yuv(output, gt, type(lq)(*[p.to(output.y.device) for p in lq[:3]], *lq[3:]), par_map, crop_border)
        psnr = psnr_yuv(output, gt, crop_border) if any(m in ('PSNR', 'PSNR_U', 'PSNR_V', 'PSNR_YUV') for m in metrics) else None      # (t, 3)
        col = {'SSIM': 'y', 'SSIM_U': 'u', 'SSIM_V': 'v'}
        planes = ''.join(dict.fromkeys(col[m] for m in metrics if m in col))
        ssim = ssim_yuv(output, gt, crop_border, planes) if planes else None                                       # (t, len(planes))
        ms_col = {'MS-SSIM': 'y', 'MS-SSIM_U': 'u', 'MS-SSIM_V': 'v'}
        ms_planes = ''.join(dict.fromkeys(ms_col[m] for m in metrics if m in ms_col))
        msssim = msssim_yuv420(output, gt, crop_border, ms_planes) if ms_planes else None                          # (t, len(ms_planes))
        xp_col = {'XPSNR': 'y', 'XPSNR_U': 'u', 'XPSNR_V': 'v'}
        xp_planes = ''.join(dict.fromkeys(xp_col[m] for m in metrics if m in xp_col))
        # gt is the original, whose activity sets the weights; the value is the CLIP's (the log of the mean weighted error): (len(xp_planes),)
        xpsnr = xpsnr_yuv420(output, gt, crop_border, xp_planes, self.test_cfg.get('xpsnr_fps', 30), clip=True)[2] if xp_planes else None
        pb_col = {'PSNR-B': 'y', 'PSNR-B_U': 'u', 'PSNR-B_V': 'v'}
        pb_planes = ''.join(dict.fromkeys(pb_col[m] for m in metrics if m in pb_col))
        # the output is the test clip, whose block edges are measured: (t, len(pb_planes))
        psnrb = psnrb_yuv420(output, gt, crop_border, pb_planes, self.test_cfg.get('psnrb_block', 8)) if pb_planes else None
        for metric in metrics:
            if metric in gain:
                eval_result[metric] = gain[metric]
            elif metric in col:
                eval_result[metric] = float(ssim[:, planes.index(col[metric])].mean())
            elif metric in pb_col:
                eval_result[metric] = float(psnrb[:, pb_planes.index(pb_col[metric])].mean())
            elif metric in xp_col:
                eval_result[metric] = float(xpsnr[xp_planes.index(xp_col[metric])])
            elif metric in ms_col:
                eval_result[metric] = float(msssim[:, ms_planes.index(ms_col[metric])].mean())
            elif metric == 'PSNR_YUV':
                eval_result[metric] = float(((6.0 * psnr[:, 0] + psnr[:, 1] + psnr[:, 2]) / 8.0).mean())
            else:
                eval_result[metric] = float(psnr[:, ('PSNR', 'PSNR_U', 'PSNR_V').index(metric)].mean())
        return eval_result

    def forward_test(self, lq, gt=None, QPs=None, slices=None, mvs=None, base_QPs=None, par_map=None, meta=None,
                     save_image=False, save_path=None, iteration=None, precomputed_output=None, out_dtype=None,
                     yuv_standard='bt601-limited', chroma='replicate'):
        """basicvsr.py:155-233.  `precomputed_output` (not in the reference): this clip's enhanced frames when the caller has
        already run the generator -- apis.multi_gpu_test does so for two clips at a time, which the generator interleaves on two
        streams; evaluation and saving then proceed clip by clip exactly as below.
        Byte frames (not in the reference): `lq` may be the decoder's uint8 (n,t,h,w,3) frames, and `out_dtype` (generator.forward's)
        asks the generator for the display bytes as well as / instead of the fp32 planes: the PNG writer takes the bytes as they
        are, and so do the metrics when the bytes are all there is (`gt` may then be a uint8 (n,t,h,w,3) clip too); only the
        centre-frame case (a 4-D `gt`) still needs the fp32 planes.
        4:2:0 frames (not in the reference): `lq` may be ops.Yuv420Frames in the colour standard `yuv_standard`, and with
        out_dtype = 'i420' | 'nv12' the generator writes packed 4:2:0 only (`precomputed_output`: that packed buffer): the
        metrics are then evaluate()'s plane metrics against a Yuv420Frames `gt`, and save_image writes <save_path>/<clip>.yuv -- the
        buffer's bytes, frames in order, one FrameWriter job per clip.  ops.Yuv420Frames16 `lq` (10 / 12 bit) likewise, with the four
        16-bit layout names beside them: the buffer is then 16-bit little-endian words, 3 B per pixel in the file.  `chroma`
        ('replicate' | 'center' | 'left' | 'topleft'): the chroma mode of generator.forward, for the planes in and the planes out.
        Self-ensemble (basicvsr.py:172-173): a model built with ensemble=dict(type='SpatialTemporalEnsemble', ...) runs
        generator.forward_ensemble where it would run the generator -- fp32 or uint8 frames and out_dtype as above,
        last_forward_seconds covers the whole ensemble, precomputed_output is taken as it is; 4:2:0 `lq` raises ValueError."""
        from . import ops
        yuv_in = ops.is_yuv(lq)
        if yuv_in and self.forward_ensemble is not None:
            raise ValueError('the self-ensemble takes fp32 or uint8 RGB frames, not 4:2:0 planes (generator.forward_ensemble)')
        yuv_layout = out_dtype if (yuv_in and isinstance(out_dtype, str) and out_dtype in self.YUV_OUT_LAYOUTS) else None
        if ops.is_yuv(gt) and yuv_layout is None:
            raise ValueError("a 4:2:0 ground truth is compared with 4:2:0 output: lq must be ops.Yuv420Frames and out_dtype one of "
                             f'{self.YUV_OUT_LAYOUTS}')
        if yuv_layout is not None:
            return self._forward_test_yuv(lq, gt, QPs, slices, mvs, base_QPs, par_map, meta, save_image, save_path, iteration,
                                          precomputed_output, yuv_layout, yuv_standard, chroma)
        if precomputed_output is not None:
            output = precomputed_output
        elif not self.psnr_only:
            with torch.no_grad():
                torch.cuda.synchronize()
                begin = time.time()
                kw = {} if out_dtype is None else {'out_dtype': out_dtype}
                if yuv_in:
                    kw['yuv_standard'] = yuv_standard
                    if chroma != 'replicate':
                        kw['chroma'] = chroma
                run = self.generator if self.forward_ensemble is None else self.forward_ensemble
                output = run(lq, QPs, slices, mvs, base_QPs, par_map, **kw)
                torch.cuda.synchronize()
                self.last_forward_seconds = time.time() - begin
        else:
            output = lq
        output_u8 = None            # (n,t,H,W,3) display bytes from the generator, when asked for
        if isinstance(output, tuple):
            output, output_u8 = output
        elif output.dtype == torch.uint8 and not self.psnr_only:
            output_u8 = output
            if gt is not None and gt.ndim == 4:
                raise ValueError("the centre-frame output reads the fp32 planes: ask for out_dtype='both' or torch.float32")
        if gt is not None and gt.ndim == 4:
            t = output.size(1)
            if self.check_if_mirror_extended(lq):
                output = 0.5 * (output[:, t // 4] + output[:, -1 - t // 4])
            else:
                output = output[:, t // 2]
        if self.test_cfg is not None and self.test_cfg.get('metrics', None):
            assert gt is not None, 'evaluation with metrics must have gt images.'
            gain_kw = dict(lq=lq, par_map=par_map) if self._gain_wanted() else {}
            results = dict(eval_result=self.evaluate(output, gt, **gain_kw))
            self._gain_report(meta, slices, QPs, base_QPs)
        else:
            lq_planes = lq
            if yuv_in:
                lq_planes = ops._frames_from_yuv(lq, yuv_standard, chroma=chroma)
            elif lq.dtype == torch.uint8 and lq.ndim == 5 and lq.is_cuda:       # byte frames: hand back the planes the caller knows
                from .ops import frames_from_rgb8
                lq_planes = frames_from_rgb8(lq)
            results = dict(lq=lq_planes.cpu(), output=output.cpu())
            if gt is not None:
                results['gt'] = gt.cpu()
        if save_image:
            # frames leave the device as uint8 (tensor2img's arithmetic); with a FrameWriter attached
            # (`model.frame_writer`, tools/test.py) the PNG encode overlaps the next clip's compute
            from .io_async import FrameWriter, frames_to_uint8_hwc
            writer = getattr(self, 'frame_writer', None)
            own = writer is None
            if own:
                writer = FrameWriter(max_workers=1)
            try:
                if output.ndim == 5:
                    folder_name = meta[0]['key'].split('/')[0]
                    rgb = frames_to_uint8_hwc(output_u8[0] if output_u8 is not None else output[0])
                    for i in range(rgb.shape[0]):
                        name = f'{i:08d}.png' if iteration is None else f'{i:08d}-{iteration + 1:06d}.png'
                        writer.submit(osp.join(save_path, folder_name, name), rgb[i])
                else:
                    img_name = meta[0]['key'].replace('/', '_')
                    name = f'{img_name}.png' if iteration is None else f'{img_name}-{iteration + 1:06d}.png'
                    writer.submit(osp.join(save_path, name), frames_to_uint8_hwc(output[0])[0])
            finally:
                if own:
                    writer.close()
        return results

    def _forward_test_yuv(self, lq, gt, QPs, slices, mvs, base_QPs, par_map, meta, save_image, save_path, iteration, precomputed_output,
                          layout, yuv_standard, chroma='replicate'):
        """forward_test with 4:2:0 planes in and packed 4:2:0 out: the generator's (n,t,3H/2,W) uint8 buffer is all that exists of the output"""
        from . import ops
        if gt is not None and not ops.is_yuv(gt):
            raise ValueError('4:2:0 output is scored against a 4:2:0 ground truth (ops.Yuv420Frames / Yuv420Frames16); the centre-frame case and RGB ground '
                             'truths read the fp32 planes')
        if precomputed_output is not None:
            buf = precomputed_output
        elif self.psnr_only:
            raise ValueError('psnr_only scores the input frames: evaluate(lq, gt) does that for 4:2:0 clips')
        else:
            with torch.no_grad():
                torch.cuda.synchronize()
                begin = time.time()
                kw = {} if chroma == 'replicate' else {'chroma': chroma}
                buf = self.generator(lq, QPs, slices, mvs, base_QPs, par_map, out_dtype=layout, yuv_standard=yuv_standard, **kw)
                torch.cuda.synchronize()
                self.last_forward_seconds = time.time() - begin
        fmt, _, depth, _ = ops.yuv_layout(layout)
        wide = depth != 8
        rows2 = {'420': 3, '422': 4, '444': 6}[fmt]        # twice the buffer's rows per luma row
        if not isinstance(buf, torch.Tensor) or (buf.dtype == torch.uint8) == wide or buf.dim() != 4 or 2 * buf.shape[-2] % rows2:
            raise ValueError('the 4:2:0 output is the packed (n,t,3H/2,W) buffer the generator returns (4:2:2: 2H rows, 4:4:4: 3H): uint8, or '
                             '16-bit words for a 10 / 12-bit layout')
        H, W = buf.shape[-2] * 2 // rows2, buf.shape[-1]
        output = ops.yuv_views(buf, H, W, layout)
        if self.test_cfg is not None and self.test_cfg.get('metrics', None):
            assert gt is not None, 'evaluation with metrics must have gt images.'
            gain_kw = dict(lq=lq, par_map=par_map) if self._gain_wanted() else {}
            results = dict(eval_result=self.evaluate(output, gt, **gain_kw))
            self._gain_report(meta, slices, QPs, base_QPs)
        else:
            from_planes = ops._frames_from_yuv
            results = dict(lq=from_planes(lq, yuv_standard, chroma=chroma).cpu(), output=buf.cpu())
            if gt is not None:
                results['gt'] = type(gt)(*[p.cpu() for p in gt[:3]], *gt[3:])
        if save_image:
            from .io_async import FrameWriter
            writer = getattr(self, 'frame_writer', None)
            own = writer is None
            if own:
                writer = FrameWriter(max_workers=1)
            try:
                clip = meta[0]['key'].split('/')[0]
                name = f'{clip}.yuv' if iteration is None else f'{clip}-{iteration + 1:06d}.yuv'
                # (16-bit words leave as their bytes, little-endian: the host's and the file's order)
                writer.submit_bytes(osp.join(save_path, name), buf[0].contiguous().cpu().view(torch.uint8).numpy())
            finally:
                if own:
                    writer.close()
        return results


def wrap_fp16_model(model):
    """mmcv.runner.wrap_fp16_model: switch on `fp16_enabled` of every sub-module that has it."""
    for m in model.modules():
        if hasattr(type(m), 'fp16_enabled') or 'fp16_enabled' in getattr(m, '__dict__', {}):
            m.fp16_enabled = True
    return model
