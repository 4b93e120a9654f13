"""The self-ensemble's Definition (include/pnpvcve.h, "Self-ensemble") restated in plain torch: flip / transpose / index lists, no
kernels.  Test infrastructure only; works on CPU and GPU tensors alike.

A variant is 4 bits v: bit 0 flips the width axis ('vertical' in the reference's naming), bit 1 the height axis ('horizontal'),
bit 2 transposes, bit 3 reverses time.  Views apply bit 0, then bit 1, then bit 2; the inverse applies bit 2, then bit 1, then bit 0."""
import torch

SPATIAL = tuple(range(8))
SPATIAL_TEMPORAL = tuple(range(16))


def view_planes(x, v):
    """x (t,c,h,w) -> variant v's view (t,c,h',w'): moved, nothing else"""
    if v & 1:
        x = x.flip(-1)
    if v & 2:
        x = x.flip(-2)
    if v & 4:
        x = x.transpose(-1, -2)
    if v & 8:
        x = x.flip(0)
    return x.contiguous()


def view_frames(lq, v):
    """fp32 (t,3,h,w) planes or uint8 (t,h,w,3) frames"""
    if lq.dtype == torch.uint8:
        return view_planes(lq.permute(0, 3, 1, 2), v).permute(0, 2, 3, 1).contiguous()
    return view_planes(lq, v)


def view_mvs(mvs, v, wrong=False):
    """(t,4,h,w), channels (fwd x, fwd y, bwd x, bwd y): moved, then bit 0 negates 0 and 2, bit 1 negates 1 and 3, bit 2 swaps 0 <-> 1
    and 2 <-> 3, bit 3 swaps (0,1) <-> (2,3).  wrong: the frames-only rule -- the maps moved, the vectors left as they are."""
    m = view_planes(mvs, v)
    if wrong:
        return m
    if v & 1:
        m = m * m.new_tensor([-1.0, 1.0, -1.0, 1.0]).view(1, 4, 1, 1)
    if v & 2:
        m = m * m.new_tensor([1.0, -1.0, 1.0, -1.0]).view(1, 4, 1, 1)
    if v & 4:
        m = m[:, [1, 0, 3, 2]]
    if v & 8:
        m = m[:, [2, 3, 0, 1]]
    return m.contiguous()


def view_side(x, v):
    """(t,1,1,1) slices / QPs / base_QPs: reversed in time under bit 3"""
    return x.flip(0).contiguous() if v & 8 else x


def inverse(out, v):
    """variant v's output (t,c,H',W') -> the original orientation and frame order"""
    if v & 4:
        out = out.transpose(-1, -2)
    if v & 2:
        out = out.flip(-2)
    if v & 1:
        out = out.flip(-1)
    if v & 8:
        out = out.flip(0)
    return out.contiguous()


def view_clip(clip, v, wrong=False):
    """clip: dict of one sample's lq, mvs, partitions, slices, QPs, base_QPs (no batch dimension) -> variant v's"""
    return dict(lq=view_frames(clip['lq'], v), mvs=view_mvs(clip['mvs'], v, wrong), partitions=view_planes(clip['partitions'], v),
                slices=view_side(clip['slices'], v), QPs=view_side(clip['QPs'], v), base_QPs=view_side(clip['base_QPs'], v))


def ensemble(run, clip, variants):
    """The Definition's output: run(view) -> (t,c,H',W'); a sequential fp32 sum in ascending v, then one scaling by 1/|V|"""
    acc = None
    for v in variants:
        o = inverse(run(view_clip(clip, v)), v)
        acc = o if acc is None else acc + o
    return acc * (1.0 / len(variants))


def symmetrise_3x3(sd):
    """every 3x3 kernel of a state dict replaced by its mean over the 8 flips and transposes: the network is then equivariant"""
    out = {}
    for k, w in sd.items():
        if w.dim() >= 2 and tuple(w.shape[-2:]) == (3, 3):
            w64 = w.double()
            four = [w64, w64.flip(-1), w64.flip(-2), w64.flip(-1).flip(-2)]
            w = (sum(four + [x.transpose(-1, -2) for x in four]) / 8.0).to(w.dtype)
        out[k] = w
    return out
