"""CPU: pnp_ensemble_view / pnp_ensemble_accumulate_f32 refuse every bad argument on the host, before any HIP call -- the pointers
are fake device addresses and no valid call is made, so this runs without a GPU."""
import os

import pytest

from pnp_vcve_amd import _native

BAD = 1001      # PNP_ERR_BAD_ARG
A, B, C, D, E, F = (0x10000 * k for k in range(1, 7))      # six distinct fake device addresses
F32, U8 = _native.FRAMES_F32_NCHW, _native.FRAMES_U8_HWC


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def view(lib, lq=A, mvs=B, par=C, lq_out=D, mvs_out=E, par_out=F, fmt=F32, t=4, h=64, w=80, variant=5):
    return lib.pnp_ensemble_view(lq, mvs, par, lq_out, mvs_out, par_out, fmt, t, h, w, variant, None)


def accumulate(lib, x=A, acc=B, t=4, c=3, H=64, W=80, variant=5, first=0, scale=1.0):
    return lib.pnp_ensemble_accumulate_f32(x, acc, t, c, H, W, variant, first, scale, None)


@pytest.mark.parametrize('over', [dict(lq=None), dict(lq_out=None), dict(mvs=None), dict(mvs_out=None), dict(par=None), dict(par_out=None),
                                  dict(lq=None, mvs_out=None), dict(lq=None, lq_out=None, par=None)],
                         ids=lambda o: '+'.join(sorted(o)))
def test_view_refuses_one_side_of_a_pair(lib, over):
    assert view(lib, **over) == BAD
    assert view(lib, fmt=U8, **over) == BAD


@pytest.mark.parametrize('over', [dict(variant=-1), dict(variant=16), dict(variant=1 << 20), dict(t=0), dict(t=-3), dict(h=0), dict(h=-64),
                                  dict(w=0), dict(w=-1), dict(fmt=2), dict(fmt=-1), dict(lq_out=A), dict(mvs_out=B), dict(par_out=C)],
                         ids=lambda o: ','.join(f'{k}={v}' for k, v in o.items()))
def test_view_refuses_bad_values(lib, over):
    assert view(lib, **over) == BAD
    if 'fmt' not in over:
        assert view(lib, fmt=U8, **over) == BAD
    # ... also when the pairs the value does not concern are absent
    if not set(over) & {'lq_out', 'mvs_out', 'par_out'}:
        assert view(lib, **dict(dict(lq=None, lq_out=None), **over)) == BAD
        assert view(lib, **dict(dict(mvs=None, mvs_out=None, par=None, par_out=None), **over)) == BAD


@pytest.mark.parametrize('over', [dict(x=None), dict(acc=None), dict(x=None, acc=None), dict(acc=A), dict(variant=-1), dict(variant=16),
                                  dict(t=0), dict(t=-1), dict(c=0), dict(c=-3), dict(H=0), dict(H=-2), dict(W=0), dict(W=-80),
                                  dict(scale=0.0), dict(scale=-0.125), dict(scale=float('inf')), dict(scale=float('-inf')),
                                  dict(scale=float('nan'))],
                         ids=lambda o: ','.join(f'{k}={v}' for k, v in o.items()))
def test_accumulate_refuses_bad_arguments(lib, over):
    for first in (0, 1):
        assert accumulate(lib, first=first, **over) == BAD
