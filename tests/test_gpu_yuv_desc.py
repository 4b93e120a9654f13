"""GPU (device tensors, no kernel launched): the ctypes descriptor ops._yuv_clip_desc builds from a clip's views, field by field
against hand-computed values, for bytes and for 16-bit words.  Pointers, pitches and frame strides are BYTES, the chroma step is
SAMPLES: the one place where the two sample sizes' shared code could confuse them."""
import pytest
import torch

from pnp_vcve_amd import _native, ops

pytestmark = pytest.mark.gpu
T, H, W, PITCH = 2, 4, 6, 8                  # pitch = w + 2 samples; a frame is 3h/2 = 6 rows
FIELDS8 = [f[0] for f in _native.Yuv420Planes._fields_]


def fields(d):
    return {name: getattr(d, name) for name, _ in d._fields_}


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int16], ids=['uint8', 'int16'])
def test_every_field_of_the_descriptor(dtype):
    S = 1 if dtype == torch.uint8 else 2     # bytes of a sample
    buf = torch.zeros((T, H * 3 // 2, PITCH), dtype=dtype, device='cuda')
    base = buf.data_ptr()
    row, frame, chroma = PITCH * S, (H * 3 // 2) * PITCH * S, H * PITCH * S      # bytes: a row, a frame, the Y plane in front of the chroma
    tail = {} if S == 1 else dict(bit_depth=12, msb_aligned=1)
    want = {
        # Y, then rows of interleaved pairs: the planes one SAMPLE apart, two samples from pair to pair
        'nv12': dict(y=base, cb=base + chroma, cr=base + chroma + S, y_pitch=row, c_pitch=row, y_frame=frame, c_frame=frame, c_step=2),
        'nv21': dict(y=base, cb=base + chroma + S, cr=base + chroma, y_pitch=row, c_pitch=row, y_frame=frame, c_frame=frame, c_step=2),
        # Y, the Cb plane, the Cr plane: chroma rows half a luma row apart, h/2 of them per plane
        'i420': dict(y=base, cb=base + chroma, cr=base + chroma + (H // 2) * (row // 2), y_pitch=row, c_pitch=row // 2, y_frame=frame,
                     c_frame=frame, c_step=1),
    }
    for order, exp in want.items():
        views = ops.yuv420_views(buf, H, W, order) if S == 1 else ops.yuv420p16_views(buf, H, W, (order, 12, True))
        d, t, h, w = ops._yuv_clip_desc(views)
        assert isinstance(d, _native.Yuv420Planes if S == 1 else _native.Yuv420Planes16), order
        assert (t, h, w) == (T, H, W) and fields(d) == {**exp, **tail}, order
        # one frame of the clip (the second): its own addresses, and no stride from frame to frame
        kind = type(views)
        one = kind(views.y[1:], views.cb[1:], views.cr[1:], *views[3:])
        d1, t1, _, _ = ops._yuv_clip_desc(one)
        exp1 = {**exp, **tail, 'y': exp['y'] + frame, 'cb': exp['cb'] + frame, 'cr': exp['cr'] + frame, 'y_frame': 0, 'c_frame': 0}
        assert t1 == 1 and fields(d1) == exp1, order
    assert FIELDS8 == list(want['nv12'])     # every field of the 8-bit struct was named above; the 16-bit one adds `tail`
