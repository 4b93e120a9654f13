"""CPU: how the chroma mode travels above the library -- Yuv420ClipFolderDataset records it in every sample's meta, and
BasicVSR.forward_test hands it to the generator ONLY when it is not 'replicate', so the default call's keyword arguments are exactly
what they were (tests/test_gpu_yuv_metrics.py pins those of apis.multi_gpu_test on the GPU)."""
import pytest
import torch

import test_yuv_metrics_host as mh
from pnp_vcve_amd import ops


def test_the_dataset_records_chroma_in_meta_and_refuses_unknown_names(tmp_path):
    from pnp_vcve_amd import datasets
    lq_dir, gt_dir, qp, _ = mh._write_tree(tmp_path, 'i420')
    base = dict(type='Yuv420ClipFolderDataset', lq_folder=str(lq_dir), gt_folder=str(gt_dir), height=16, width=24, qp_slice_file=str(qp))
    ds = datasets.build_dataset(dict(base))
    assert ds.chroma == 'replicate' and ds[0]['meta']['chroma'] == 'replicate'
    for name in ('center', 'left', 'topleft'):
        ds = datasets.build_dataset(dict(base, chroma=name))
        assert ds.chroma == name and all(ds[i]['meta']['chroma'] == name for i in range(len(ds)))
        assert datasets.collate([ds[1]])['meta'][0]['chroma'] == name
        # nothing else of a sample depends on it: the planes are the file's
        assert torch.equal(ds[0]['lq_yuv'], datasets.build_dataset(dict(base))[0]['lq_yuv'])
    for bad in ('top-left', 'Left', 'bilinear', 2, None):
        with pytest.raises(ValueError, match='chroma'):
            datasets.build_dataset(dict(base, chroma=bad))


def test_forward_test_tells_the_generator_only_when_the_mode_is_not_the_default(monkeypatch):
    from pnp_vcve_amd import restorer      # noqa: F401
    from pnp_vcve_amd import synthetic as syn
    from pnp_vcve_amd.registry import build_model
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    model = build_model(dict(type='BasicVSR', generator=dict(type='IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par',
                                                             **dict(syn.DEFAULT_GENERATOR_CFG))),
                        train_cfg=None, test_cfg=dict(metrics=['PSNR'], crop_border=0)).eval()
    t, h, w = 2, 64, 64
    lq = ops.Yuv420Frames(torch.zeros(1, t, h, w, dtype=torch.uint8), torch.zeros(1, t, h // 2, w // 2, dtype=torch.uint8),
                          torch.zeros(1, t, h // 2, w // 2, dtype=torch.uint8))
    asked = []

    def generator(lrs, QPs=None, slices=None, mvs=None, base_QPs=None, par_map=None, **kw):
        asked.append(kw)
        if kw.get('out_dtype') == 'i420':
            return torch.zeros(1, t, h * 3 // 2, w, dtype=torch.uint8)
        return torch.zeros(1, t, 3, h, w)

    model.generator.forward = generator
    model.evaluate = lambda out, gt: dict(PSNR=1.0)
    gt_yuv, gt_rgb = lq, torch.zeros(1, t, 3, h, w)
    # planes out (what apis.multi_gpu_test(yuv_frames=True) asks for), then fp32 out
    model.forward_test(lq, gt_yuv, out_dtype='i420')
    model.forward_test(lq, gt_yuv, out_dtype='i420', chroma='replicate')
    model.forward_test(lq, gt_yuv, out_dtype='i420', yuv_standard='bt709-full', chroma='left')
    model.forward_test(lq, gt_rgb)
    model.forward_test(lq, gt_rgb, chroma='topleft')
    assert asked == [dict(out_dtype='i420', yuv_standard='bt601-limited'), dict(out_dtype='i420', yuv_standard='bt601-limited'),
                     dict(out_dtype='i420', yuv_standard='bt709-full', chroma='left'), dict(yuv_standard='bt601-limited'),
                     dict(yuv_standard='bt601-limited', chroma='topleft')]
