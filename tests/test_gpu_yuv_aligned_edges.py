"""GPU: the aligned forms of the pack (pack_lr_yuv420_fast_kernel, pack_lr_rows_fast_kernel) at the edges of the frame.  Elsewhere they
only run at 64 x 96, where no thread has both of its side columns clamped, and the small sizes of the other files have widths that are
no multiple of 4 and take the general form.  Here a row holds one group of four pixels with both clamps (w = 4), two groups with one
clamp each (w = 8), or those and an interior one (w = 12); the frame holds one chroma row or an interior one.  Tight planes at offset 0
of a guard-banded allocation, so that the aligned form applies -- which every case asserts first, by the conditions of yuv_planes_fast
(csrc/yuv.h) restated on the views' addresses and strides: a case that fails that is a bug of this file, never a skip.  Every check is
torch.equal or byte-equal: no tolerance."""
import pytest
import torch

import test_gpu_yuv16_frames as y16
import test_gpu_yuv_formats as yfm
import test_gpu_yuv_frames as yf
import yuv_chroma_ref as cref
import yuv_formats_ref as fref
from pnp_vcve_amd import ops

pytestmark = pytest.mark.gpu
T = 2
MODES = cref.MODES          # 'replicate', 'center', 'left', 'topleft'
SIZES = [(2, 4), (2, 8), (4, 8), (6, 12)]
SIZES_444 = SIZES + [(1, 4), (3, 8)]    # rows need not pair up
STANDARDS = {'nv12': 'bt601-limited', 'nv21': 'bt709-full', 'i420': 'bt709-limited'}      # by the plane order ('nv21': Cr first)
DEPTHS = [(8, False), (10, True)]


def fast_form_applies(views, fmt):
    """yuv_planes_fast(p, w, format) of csrc/yuv.h for the descriptor ops makes of (t,h,w) views: pointers, pitches and frame strides
    in bytes, c_step in samples"""
    y, cb, cr = views[:3]
    S, w = y.element_size(), y.shape[2]
    four = 4 * S - 1
    two = four if fmt == '444' else 2 * S - 1
    if w & 3 or (y.data_ptr() | S * y.stride(1) | S * y.stride(0)) & four:
        return False
    assert cb.stride() == cr.stride()
    c_pitch, c_frame, c_step = S * cb.stride(1), S * cb.stride(0), cb.stride(2)
    if c_step == 2:
        lo, hi = sorted((cb.data_ptr(), cr.data_ptr()))
        return hi - lo == S and not (lo | c_pitch | c_frame) & four
    return c_step == 1 and not (cb.data_ptr() | cr.data_ptr() | c_pitch | c_frame) & two


def planes_of(fmt, order, depth, msb, h, w):
    """(tight planes at offset 0 behind their guard band, sample values to fill them with)"""
    if fmt != '420':
        container = (None, fmt, order, depth, msb, None)
        return yfm.FPlanes(T, h, w, container), yfm.random_values(17 * h + w, container, T, h, w)
    if depth == 8:
        return yf.Planes(T, h, w, order), yf.random_planes(17 * h + w, T, h, w)
    return y16.Planes16(T, h, w, order, depth, msb), y16.random_values(17 * h + w, T, h, w, depth)


def restatement(vals, standard, depth, mode, fmt):
    vals = [v.numpy() for v in vals]
    if fmt == '420':
        return torch.from_numpy(cref.from_planes(*vals, standard, depth, mode))
    return torch.from_numpy(fref.from_planes(*vals, standard, depth, mode, fmt))


@pytest.mark.parametrize('depth,msb', DEPTHS, ids=['8bit', '10bit-high'])
@pytest.mark.parametrize('order', list(STANDARDS))
@pytest.mark.parametrize('fmt', fref.FORMAT_NAMES)
def test_the_aligned_pack_at_the_frame_edges_is_the_general_pack_and_the_restatement(fmt, order, depth, msb):
    standard = STANDARDS[order]
    for h, w in (SIZES_444 if fmt == '444' else SIZES):
        p, vals = planes_of(fmt, order, depth, msb, h, w)
        p.fill(*vals)
        assert fast_form_applies(p.views, fmt), (h, w, 'the planes of this test must take the aligned form')
        for mode in MODES:
            want = restatement(vals, standard, depth, mode, fmt).to(yf.dev())
            fast = ops.pack_lr_yuv(p.views, standard, chroma=mode)
            slow = ops.pack_lr_yuv(p.views, standard, general=True, chroma=mode)
            assert fast.shape == (T, h, w, 4) and torch.equal(fast, slow), (h, w, mode, int((fast != slow).sum()))
            assert torch.equal(fast[..., :3].permute(0, 3, 1, 2), want) and not bool(fast[..., 3].any()), (h, w, mode)
        assert torch.equal(p.flat.cpu(), p.expect(*vals)), (h, w, 'the planes or their guard bytes were written')
