"""CPU: tests/head_ref.py -- the float64 reference of the reconstruction head agrees with a second, hand-written form, the shapes of
tests/test_gpu_head_edges.py reach the launch rules they are named for, and the seeded inputs tell the obvious wrong kernels from the
right one: every deliberately wrong variant differs from the reference by more than 1e-3 (about 50 times the loosest gate of the GPU
tests) somewhere in the last row or column of the output (the first, for a slip at coordinate 0)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ref as R

MARGIN = 1e-3


def edge_max(d, which='last'):
    """largest |d| over the last (or first) row and column of (..., H, W)"""
    d = np.abs(d)
    i = -1 if which == 'last' else 0
    return float(max(d[..., i, :].max(), d[..., :, i].max()))


def test_the_shapes_reach_the_launch_rules_they_are_named_for():
    t = R.tiles_8x16
    assert [t(40, 48) % 8, t(64, 64) % 8] == [7, 0]                     # XCD remap remainders
    assert t(100, 932) == 767 and t(185, 497) == 768 and t(188, 500) == 768      # conv_last: KS = 4 below 768 tiles, KS = 1 from there
    assert 185 % 8 and 497 % 16                                        # ... the first KS = 1 frame is ragged both ways
    assert t(120, 1008) == 945 and t(121, 1009) == 1024                 # pixel shuffle: 4x16 tiles below 1024 8x16 tiles, 8x16 from there
    assert all(h % 4 == 0 and w % 4 == 0 for h, w in R.LAST_MODE3)
    assert R.frame_size(4, 4, 3) == (1, 1)


def test_inputs_are_at_the_scale_of_the_op_tests():
    w, b = R.last_weights()
    pw, pb = R.shuffle_weights()
    x = R.feature_map('last', 37, 53)
    assert -1 < x.min() < -0.99 and 0.99 < x.max() < 1
    for wt in (w, pw):
        assert -0.06 <= wt.min() < -0.059 and 0.059 < wt.max() <= 0.06
    assert np.abs(pb).max() <= 0.1 and len(set(pb.tolist())) == 256 and len(set(b.tolist())) == 3
    f = R.frame_planes(36, 52, 3)
    assert f.shape == (3, 9, 13) and 0 <= f.min() and f.max() <= 1
    assert R.frame_bytes(37, 53, 2).shape == (37, 53, 3)


@pytest.mark.parametrize('hw', R.LAST_MODE3, ids=lambda s: '%dx%d' % s)
def test_bilinear_by_hand_is_the_interpolate_call(hw):
    p = R.frame_planes(*hw, 3)
    assert np.abs(R.bilinear_x4_by_hand(p) - R.upsample_x4(p)).max() < 1e-14


def test_pixel_shuffle_reference_by_index():
    """out[2y + dy, 2x + dx, c] = act(conv[4c + 2dy + dx, y, x])"""
    w, b = R.shuffle_weights()
    x = R.feature_map('ps', 3, 7)
    conv = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(2, 0, 1)[None], torch.from_numpy(w.astype(np.float64)),
                    torch.from_numpy(b.astype(np.float64)), padding=1)[0].numpy()
    for act in (0, 1, 2):
        ref = R.pixel_shuffle_conv_ref(x, w, b, act)
        assert ref.shape == (6, 14, 64)
        a = conv if act == 0 else np.where(conv > 0, conv, 0.0 if act == 1 else 0.1 * conv)
        for dy in (0, 1):
            for dx in (0, 1):
                assert np.array_equal(ref[dy::2, dx::2, :], a[2 * dy + dx::4].transpose(1, 2, 0))
    assert np.array_equal(R.shuffle_case(3, 7, 2), R.pixel_shuffle_conv_ref(x, w, b, 2))


def test_conv_last_reference_pieces():
    w, b = R.last_weights()
    x = R.feature_map('last', 9, 17)
    f2, f3 = R.frame_planes(9, 17, 2), R.frame_planes(12, 20, 3)
    ref = R.conv_last_ref(x, w, b, f2, 2)
    assert ref.shape == (3, 9, 17) and np.array_equal(ref, R.last_term_case(9, 17) + f2)
    # one pixel by hand: the corner, where 5 of the 9 taps are padding
    acc = b[0].astype(np.float64) + sum(float(np.dot(x[dy, dx].astype(np.float64), w[0, :, dy + 1, dx + 1].astype(np.float64)))
                                        for dy in (0, 1) for dx in (0, 1))
    assert abs(ref[0, 0, 0] - (acc + f2[0, 0, 0])) < 1e-13
    assert R.conv_last_base(f3, 3).shape == (3, 12, 20)
    neg = R.conv_last_term(x, w, b, 2)
    t = R.last_term_case(9, 17)
    assert np.allclose(neg, np.where(t > 0, t, 0.1 * t), rtol=0, atol=1e-15)
    # fp16 operands: the map and the weights are rounded, the bias is not
    t16 = R.last_term_case(9, 17, 'fp16')
    assert 1e-5 < np.abs(t16 - t).max() < 5e-3


def test_byte_boundary_definitions():
    u8 = np.arange(768, dtype=np.uint8).reshape(16, 16, 3)
    p = R.planes_from_bytes(u8)
    assert p.dtype == np.float32 and p.shape == (3, 16, 16)
    assert all(p[c, y, x] == np.float32(u8[y, x, c]) / np.float32(255) for c, y, x in ((0, 0, 0), (1, 3, 7), (2, 15, 15)))
    assert np.array_equal(R.to_bytes(p), u8)                       # every byte survives the round trip
    x = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, 0.25, 0.75], np.float32).reshape(1, 1, 7).repeat(3, 0)
    assert R.to_bytes(x)[0, :, 0].tolist() == [0, 0, 128, 255, 255, 64, 191]      # 127.5 -> 128, 63.75 -> 64, 191.25 -> 191
    r = R.rgb0_from_planes(p)
    assert r.shape == (16, 16, 4) and np.array_equal(r[..., :3], p.transpose(1, 2, 0)) and not r[..., 3].any()


@pytest.mark.parametrize('hw', R.LAST_MODE3, ids=lambda s: '%dx%d' % s)
def test_wrong_bilinear_variants_show_at_the_frame_edges(hw):
    """the conv term is common to both sides: the variants differ from the reference by what they do to the frame"""
    for planes in (R.frame_planes(*hw, 3), R.planes_from_bytes(R.frame_bytes(*hw, 3))):
        ref = R.upsample_x4(planes)
        zero_pad = R.bilinear_x4_by_hand(planes, edge='zero')
        assert edge_max(zero_pad - ref, 'last') > MARGIN
        if hw == (4, 4):
            continue        # a 1 x 1 frame is constant under every clamped or extrapolating form: only the zero tap shows
        assert edge_max(R.bilinear_x4_by_hand(planes, align_corners=True) - ref, 'last') > MARGIN
        assert edge_max(R.bilinear_x4_by_hand(planes, clamp_low=False) - ref, 'first') > MARGIN
        # (a clamp dropped on one axis only shows on that axis' first line)
        no_low = R.bilinear_x4_by_hand(planes, clamp_low=False)
        assert np.abs(no_low - ref)[:, 0, :].max() > MARGIN and np.abs(no_low - ref)[:, :, 0].max() > MARGIN
        assert np.abs(zero_pad - ref)[:, -1, :].max() > MARGIN and np.abs(zero_pad - ref)[:, :, -1].max() > MARGIN


@pytest.mark.parametrize('hw', R.PIXEL_SHUFFLE, ids=lambda s: '%dx%d' % s)
def test_wrong_pixel_shuffle_variants_show_in_the_last_row_and_column(hw):
    w, b = R.shuffle_weights()
    x = R.feature_map('ps', *hw)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    conv = F.conv2d(t(x).permute(2, 0, 1)[None], t(w), None, padding=1)
    bias = lambda v: conv + t(v)[None, :, None, None]      # noqa: E731
    ref = F.leaky_relu(F.pixel_shuffle(bias(b), 2), 0.1).numpy()
    swapped = F.leaky_relu(R.pixel_shuffle_swapped(bias(b)), 0.1).numpy()
    raw_bias = F.leaky_relu(F.pixel_shuffle(bias(R.unpermuted_bias(b)), 2), 0.1).numpy()
    assert edge_max(swapped - ref) > MARGIN and edge_max(raw_bias - ref) > MARGIN
    if hw == (3, 7):
        assert np.array_equal(ref[0].transpose(1, 2, 0), R.shuffle_case(3, 7, 2))
        # the swap is the transposition of every 2 x 2 block of sub-pixels
        assert np.array_equal(swapped[..., 0::2, 1::2], ref[..., 1::2, 0::2]) and np.array_equal(swapped[..., 0::2, 0::2], ref[..., 0::2, 0::2])


def test_identity_weights_make_the_pixel_shuffle_a_rearrangement():
    w, b = R.identity_shuffle_weights()
    x = R.identity_map(5, 17)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and len(np.unique(x)) > 900
    for sub in range(4):
        assert sorted(R.identity_channel(c, sub) for c in range(64)) == list(range(64))
    exp = R.identity_shuffle_expected(x)
    assert np.array_equal(R.pixel_shuffle_conv_ref(x, w, b, 0), exp.astype(np.float64))
    # a swapped sub-pixel or a shifted channel is a different rearrangement, at nearly every element
    assert (exp[0::2, 1::2] != exp[1::2, 0::2]).mean() > 0.99 and (exp != np.roll(exp, 1, axis=2)).mean() > 0.99


def test_the_clamp_input_leaves_the_unit_interval_on_both_sides():
    ref = R.clamp_case_ref()
    assert (ref < 0).mean() >= 0.1 and (ref > 1).mean() >= 0.1
