"""CPU: tests/any_size_ref.generator_forward IS the oracle.  On every input cpu_ref.generator_forward accepts the two are torch.equal,
so what any_size_ref gives on a frame that is no multiple of 4 -- where cpu_ref raises, as the reference does -- is the oracle's blocks
on that grid and needs no tolerance of its own."""
import numpy as np
import pytest
import torch

import any_size_ref
import golden_util as gu
from oracle import cpu_ref

KEYS = ('lq', 'QPs', 'slices', 'mvs', 'base_QPs', 'partitions')

#        name              cfg overrides                        clip
CASES = [
    ('cat_alignkey', dict(num_blocks=2), dict(seed=901, n=1, t=5, h=64, w=64, slices='IBBBP', qp_mode='qp', crf=25)),
    ('cat_alignkey_64x72', dict(num_blocks=2), dict(seed=902, n=1, t=5, h=64, w=72, slices='allP', qp_mode='qp', crf=35)),
    ('nocat', dict(num_blocks=2, with_cat=False), dict(seed=903, n=1, t=5, h=64, w=72, slices='IBBBP', qp_mode='qp', crf=25)),
    ('cat_noalignkey', dict(num_blocks=2, align_key=False), dict(seed=904, n=1, t=5, h=64, w=64, slices='allP', qp_mode='ipb', crf=15)),
    ('vsr', dict(num_blocks=2, vsr=True), dict(seed=905, n=1, t=5, h=64, w=64, slices=[73, 66, 80, 66, 66], qp_mode='qp', crf=25)),
    ('mirror_t8', dict(num_blocks=2), dict(seed=906, n=1, t=8, h=64, w=64, slices=[73, 66, 80, 66, 66, 80, 66, 73], qp_mode='qp', crf=25)),
    ('n2_mixed_keys', dict(num_blocks=2), dict(seed=907, n=2, t=5, h=64, w=72, slices=[[73, 66, 66, 80, 66], [73, 80, 66, 66, 66]],
                                              qp_mode='qp', crf=[15, 35])),
    ('sparse_val', dict(num_blocks=2, sparse_val=True), dict(seed=908, n=1, t=5, h=64, w=72, slices='IBBBP', qp_mode='qp', crf=25)),
]


def inputs(name, cfg_over, clip_kw):
    case = dict(name=name, cfg=cfg_over, wseed=40, par_gain=10.0, clip=clip_kw, mirror=name.startswith('mirror'),
                par_kind='overlap' if cfg_over.get('sparse_val') else None)
    cfg, sd, clip = gu.gen_case_inputs(case)
    return cfg, cpu_ref.to_torch_state(sd), [torch.from_numpy(np.ascontiguousarray(clip[k])) for k in KEYS]


@pytest.mark.parametrize('name,cfg_over,clip_kw', CASES, ids=[c[0] for c in CASES])
def test_the_restated_loop_equals_the_oracle_where_the_oracle_runs(name, cfg_over, clip_kw):
    cfg, sd, (lq, qps, sl, mvs, bq, par) = inputs(name, cfg_over, clip_kw)
    with torch.no_grad():
        want = cpu_ref.generator_forward(sd, cfg, lq, qps, sl, mvs, bq, par)
        got = any_size_ref.generator_forward(sd, cfg, lq, qps, sl, mvs, bq, par)
    s = 4 if cfg.get('vsr') else 1
    assert got.shape == (clip_kw['n'], clip_kw['t'], 3, clip_kw['h'] * s, clip_kw['w'] * s)
    assert torch.equal(got, want)


def test_it_runs_where_the_oracle_raises_and_keeps_the_minimum_size():
    cfg, sd, (lq, qps, sl, mvs, bq, par) = inputs('ragged', dict(num_blocks=2), dict(seed=909, n=1, t=3, h=65, w=66, slices=[73, 66, 80],
                                                                                      qp_mode='qp', crf=25))
    with torch.no_grad():
        with pytest.raises(ValueError):
            cpu_ref.generator_forward(sd, cfg, lq, qps, sl, mvs, bq, par)
        out = any_size_ref.generator_forward(sd, cfg, lq, qps, sl, mvs, bq, par)
        assert out.shape == (1, 3, 3, 65, 66) and bool(torch.isfinite(out).all())
        with pytest.raises(AssertionError):
            any_size_ref.generator_forward(sd, cfg, lq[..., :63, :], qps, sl, mvs[..., :63, :], bq, par[..., :63, :])
