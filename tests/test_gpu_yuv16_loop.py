"""GPU: the raw 10-bit .yuv loop.  A folder of yuv420p10le clips goes through Yuv420ClipFolderDataset(bit_depth=10) and
multi_gpu_test(yuv_frames=True, yuv_out_layout='yuv420p10le'): the written files are ops.frames_to_yuv420p16 of the fp32 forward's
output, 3 B per pixel, and the reported metrics are evaluate()'s on those planes -- byte-equal and digit for digit."""
import os

import numpy as np
import pytest
import torch

import test_gpu_yuv_metrics as m8
import yuv16_ref
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
T, H, W = 5, 64, 64


def write_yuv10_tree(root, clips=('000', '011')):
    """write_clip_tree's PNG / MV-record / QP tree, plus its frames as raw yuv420p10le: <root>/crf25/yuv/<clip>.yuv, <root>/X4/yuv/<clip>.yuv"""
    from PIL import Image
    lq_png, gt_png, qp = m8.yf.gu.syn.write_clip_tree(str(root), clips=list(clips), t=T, h=H, w=W, seed=6, slices='IBBBP')
    out = []
    for png in (lq_png, gt_png):
        folder = os.path.join(os.path.dirname(png), 'yuv')
        os.makedirs(folder)
        for clip in clips:
            rgb = np.stack([np.asarray(Image.open(os.path.join(png, clip, f'{i:08d}.png')).convert('RGB')) for i in range(T)])
            planes = (rgb.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)
            words = yuv16_ref.pack(*yuv16_ref.to_yuv16(planes, 'bt601-limited', 10, False), 'i420')
            words.astype('<u2').tofile(os.path.join(folder, clip + '.yuv'))
        out.append(folder)
    return out[0], out[1], qp


def test_multi_gpu_test_on_raw_10_bit_clips_scores_and_writes_what_the_forward_gives(tmp_path):
    from pnp_vcve_amd.apis import _to_device, multi_gpu_test
    from pnp_vcve_amd.datasets import build_dataset, collate
    lq, gt, qp = write_yuv10_tree(tmp_path / 'data')
    cfg = dict(type='Yuv420ClipFolderDataset', lq_folder=lq, gt_folder=gt, height=H, width=W, layout='i420', qp_slice_file=qp)
    ds = build_dataset(dict(cfg, bit_depth=10))
    assert len(ds) == 2 and os.path.getsize(os.path.join(lq, '000.yuv')) == T * 3 * H * W
    model = m8.restorer_model()
    want, want_bytes = [], {}
    for i in range(2):
        sample = ds[i]
        assert sample['lq_yuv'].dtype == torch.int16 and sample['lq_yuv'].shape == (T, H * 3 // 2, W) and sample['meta']['bit_depth'] == 10
        data = _to_device(collate([sample]), m8.dev())
        assert isinstance(data['lq'], ops.Yuv420Frames16) and isinstance(data['gt'], ops.Yuv420Frames16) and data['lq'].y.shape == (1, T, H, W)
        assert (data['lq'].bit_depth, data['lq'].msb_aligned) == (10, False)
        side = [data[k] for k in ('QPs', 'slices', 'mvs', 'base_QPs', 'partitions')]
        with torch.no_grad():
            f32 = model.generator(data['lq'], *side)
        packed, views = ops.frames_to_yuv420p16(f32, 'bt601-limited', 'yuv420p10le')
        want_bytes[ds.keys[i]] = packed[0].cpu().numpy().astype('<i2').tobytes()
        assert len(want_bytes[ds.keys[i]]) == T * 3 * H * W
        want.append(model.evaluate(views, data['gt']))
        assert list(want[-1]) == m8.ALL_METRICS and all(np.isfinite(v) for v in want[-1].values())
    for cif in (1, 2):
        save = tmp_path / f'out{cif}'
        got = multi_gpu_test(model, ds, save_image=True, save_path=str(save), device=m8.dev(), metrics=tuple(m8.ALL_METRICS), clips_in_flight=cif,
                             yuv_frames=True, yuv_out_layout='yuv420p10le')
        assert [r['eval_result'] for r in got] == want, cif                 # digit for digit
        assert sorted(os.listdir(save)) == ['000.yuv', '011.yuv']
        for clip, b in want_bytes.items():
            with open(save / f'{clip}.yuv', 'rb') as fh:
                assert fh.read() == b, (cif, clip)
    # the output is scored at the ground truth's depth: an 8-bit layout, or 12 bits, for a 10-bit dataset is refused
    for layout in ('i420', 'nv12', 'yuv420p12le', 'p012', 'rgb'):
        with pytest.raises(ValueError, match='yuv_out_layout'):
            multi_gpu_test(model, ds, device=m8.dev(), yuv_frames=True, yuv_out_layout=layout)
    # a file whose size is no multiple of the 10-bit frame size: the 8-bit frame size divides it, the dataset's error all the same
    with open(os.path.join(lq, '000.yuv'), 'rb') as fh:
        blob = fh.read()
    with open(os.path.join(lq, '000.yuv'), 'wb') as fh:
        fh.write(blob[:T * 3 * H * W - 3 * H * W // 2])
    with pytest.raises(ValueError, match='not a whole number'):
        ds[0]
    for bad in (9, 16, True):
        with pytest.raises(ValueError, match='bit_depth'):
            build_dataset(dict(cfg, bit_depth=bad))
