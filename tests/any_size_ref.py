"""Expected values of the any_size forward (test infrastructure only).

oracle/cpu_ref.generator_forward refuses a frame whose height or width is no multiple of 4, as the reference does: its
spatial_padding (iconvsr.py:371-394) pads `lrs` alone, so flow_warp.py:27-29 raises on the unpadded flow.  Nothing in the network needs
the multiple, and any_size runs the same formulas on the h x w grid as given.  The reference therefore has no output to pin this mode
to; it is pinned to the oracle's own blocks instead.  `generator_forward` below restates the loop of iconvsr_ipb_par.py:44-149 from
cpu_ref's pinned blocks -- base_predictor, bias_predictor, deform_align, resblocks, pixel_shuffle_pack -- and leaves the size check out.
tests/test_any_size_ref.py holds it to torch.equal with cpu_ref.generator_forward wherever that one runs, so the ragged expectations
need no tolerance of their own.
"""
import torch
import torch.nn.functional as F

from oracle import cpu_ref


def generator_forward(sd, cfg, lrs, QPs, slices, mvs, base_QPs, par_map):
    """iconvsr_ipb_par.py:44-149 on the (h, w) grid as given: (n,t,3,h,w), or (n,t,3,4h,4w) with cfg['vsr']."""
    with_cat = cfg.get('with_cat', False)
    align_key = cfg.get('align_key', False)
    with_bias = cfg.get('with_bias', False)
    ew_all = cpu_ref.base_predictor(sd, base_QPs if cfg.get('use_base_qp', False) else QPs, cfg.get('expert_softmax', False))     # :45-46
    gammas = cpu_ref.bias_predictor(sd, cfg, QPs)[0] if with_bias else None                                                          # :47-48
    n, t, _, h, w = lrs.shape
    assert h >= 64 and w >= 64, f'The height and width of inputs should be at least 64, but got {h} and {w}.'
    flows_forward = mvs[:, 1:, 0:2]                     # iconvsr_ipb.py:33-46 (mirror extension selects the same maps)
    flows_backward = mvs[:, :t - 1, 2:4]
    key = ((slices[:, :, 0, 0, 0] == 73) | (slices[:, :, 0, 0, 0] == 80)).clone()                                                    # :60-62
    key[:, 0] = True
    key[:, -1] = True
    zeros = lrs.new_zeros(n, cfg.get('mid_channels', 64), h, w)

    def aligned(feats, i, flows, nearest_key, step):
        """per sample: the nearest key frame's map warped by frame i's flow, and the neighbour's (the same tensor with align_key when
        the neighbour IS the key frame)"""
        kws, nbs = [], []
        for b in range(n):
            k = nearest_key(b)
            kf = cpu_ref.deform_align(sd, cfg, feats[k][b:b + 1], flows[b:b + 1])
            kws.append(kf)
            nbs.append(kf if (align_key and k == i + step) else feats[i + step][b:b + 1])
        return torch.cat(kws), torch.cat(nbs)

    feats = [None] * t
    for i in range(t - 1, -1, -1):                                                                                                   # :71-100
        key_warp, neighbor = zeros, zeros
        if i < t - 1:
            key_warp, neighbor = aligned(feats, i, flows_backward[:, i], lambda b: i + 1 + int(torch.where(key[b, i + 1:])[0][0]), 1)
        feat = torch.cat([lrs[:, i], key_warp, neighbor] if with_cat else [lrs[:, i], key_warp], 1)
        feats[i] = cpu_ref.resblocks(sd, cfg, 'backward_resblocks', feat, par_map[:, i], ew_all[:, i], gammas[:, i] if with_bias else None)

    outs = []
    for i in range(t):                                                                                                               # :103-147
        lr = lrs[:, i]
        key_warp, neighbor = zeros, zeros
        if i > 0:
            key_warp, neighbor = aligned(feats, i, flows_forward[:, i - 1], lambda b: int(torch.where(key[b, :i])[0][-1]), -1)
        feat = torch.cat([lr, key_warp, neighbor, feats[i]] if with_cat else [lr, key_warp, feats[i]], 1)
        fp = cpu_ref.resblocks(sd, cfg, 'forward_resblocks', feat, par_map[:, i], ew_all[:, i], gammas[:, i] if with_bias else None)
        feats[i] = fp
        if cfg.get('vsr', False):                                                                                                    # :135-142
            o = F.leaky_relu(cpu_ref.pixel_shuffle_pack(sd, 'upsample1.', fp), 0.1)
            o = F.leaky_relu(cpu_ref.pixel_shuffle_pack(sd, 'upsample2.', o), 0.1)
            o = F.leaky_relu(F.conv2d(o, sd['conv_hr.weight'], sd['conv_hr.bias'], padding=1), 0.1)
            o = F.conv2d(o, sd['conv_last.weight'], sd['conv_last.bias'], padding=1)
            o = o + F.interpolate(lr, scale_factor=4, mode='bilinear', align_corners=False)
        else:                                                                                                                        # :144-146
            o = F.leaky_relu(F.conv2d(fp, sd['conv_hr.weight'], sd['conv_hr.bias'], padding=1), 0.1)
            o = F.conv2d(o, sd['conv_last.weight'], sd['conv_last.bias'], padding=1) + lr
        outs.append(o)
    return torch.stack(outs, dim=1)                                                                                                  # :149
