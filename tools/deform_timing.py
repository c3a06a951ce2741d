"""Time epropnp.deform.sample_attend (epropnp_deform_sample_forward / _backward) on the device next to the reference's formulation.

    python tools/deform_timing.py [--out profiles/deform_timing.txt]

The detection shape: 600 objects on 6 images, 8 heads x 32 channels, 32 points (and 16, the second sampler of the configs), maps of
232 x 400 (the configs' 928 x 1600 padded input at stride 4), NCHW maps and channels-last maps.  Forward, and forward + backward with
cotangents on all five outputs and gradients to query, key, value and location.

The yardstick is `composite` below: the reference's own formulation (deformable_attention_sampler.py:84-137 -- four grid_sample
calls on permuted 5-D views with the image index as a third grid axis, softmax, two matmuls, autograd for the backward) in PyTorch
on the same device and the same tensors.  Both sides are timed with events around the Python calls (mean after warm-up); for the
fused op the library's stage recorder gives the device time of the forward launch and of the backward (zero fill of the two map
gradients + the scatter launch) as well.  The backward's float atomics are counted from the locations (one per corner of non-zero
weight, channel and map) and set against the chip-wide rate of about 1.3 TB/s of added bytes.  Engine / memory clocks as bench.py's
sampler reads them while the loops run.  There is no pass / fail ratio, the file is the record.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import event_ms      # noqa: E402


def composite(query, key, value, dense_x2d, dense_mask, loc, img, stride):
    B, H, _, D = query.shape
    NI, E, h, w = key.shape
    P = loc.shape[2]
    size = loc.new_tensor([w * stride, h * stride])
    grid = (loc * (2 / size) - 1).transpose(0, 1).reshape(H, B, P, 1, 2)
    z = (img.to(loc.dtype) + 0.5) * (2 / NI) - 1.0
    grid = torch.cat((grid, z[None, :, None, None, None].expand(H, -1, P, 1, 1)), -1)
    heads = lambda m: m.reshape(NI, H, D, h, w).permute(1, 2, 0, 3, 4)
    shared = lambda m: m.transpose(0, 1)[None].expand(H, -1, -1, -1, -1)
    gs = lambda m, pad: F.grid_sample(m, grid, mode='bilinear', padding_mode=pad, align_corners=False).squeeze(-1).permute(2, 0, 1, 3)
    k, v = gs(heads(key), 'border'), gs(heads(value), 'border')
    x2d, mask = gs(shared(dense_x2d), 'border'), gs(shared(dense_mask), 'zeros')
    a = query @ k / np.sqrt(D)
    attn = (v @ (a.softmax(-1) * mask).reshape(B, H, P, 1)).reshape(B, E)
    return attn, v, a, mask, x2d


def stage_pair_ms(fn, n):
    """device time of the forward stage and of the backward stage over n calls of fn (the library's stage recorder)"""
    from epropnp import _hip
    _hip.profile(True, reset=True)
    for _ in range(n):
        fn()
    fwd, nf = _hip.profile_read('deform_sample_forward')
    bwd, nb = _hip.profile_read('deform_sample_backward')
    _hip.profile(False, reset=True)
    return fwd, nf, bwd, nb


def atomic_bytes(loc, stride, h, w, D):
    """bytes the backward adds with float atomics: corners of non-zero weight x D channels x 2 maps x 4 bytes"""
    c = loc.double() / stride - 0.5
    cx, cy = c[..., 0].clamp(0, w - 1), c[..., 1].clamp(0, h - 1)
    fx, fy = cx - cx.floor(), cy - cy.floor()
    nx, ny = 1 + (fx != 0).long(), 1 + (fy != 0).long()      # fx == 0: the right-hand corners weigh nothing
    return int((nx * ny).sum()) * D * 2 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import deform
    dev = torch.device('cuda:0')
    n, warm = a.launches, 3
    B, NI, H, D, h, w, stride = 600, 6, 8, 32, 232, 400, 4
    E = H * D
    lines = [f'deform.sample_attend timing: mean of {n} calls after {warm} warm-up calls; {torch.cuda.get_device_name(0)}',
             f'{B} objects, {NI} images, {H} heads x {D} channels, maps {h} x {w} at stride {stride} ({NI * E * h * w * 4 / 1e6:.0f} MB each)']
    g = torch.Generator().manual_seed(11)
    key, value = torch.randn(NI, E, h, w, generator=g).to(dev), torch.randn(NI, E, h, w, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    x2d = ((torch.stack((xx, yy)) + 0.5)[None] * stride + torch.randn(NI, 2, h, w, generator=g)).contiguous().to(dev)
    mask = (torch.rand(NI, 1, h, w, generator=g) > 0.3).float().to(dev)
    img = torch.randint(0, NI, (B,), generator=g).to(dev)
    centre = torch.rand(B, 2, generator=g) * torch.tensor([w * stride, h * stride], dtype=torch.float32)
    obj_stride = torch.tensor([8.0, 16.0, 32.0])[torch.randint(0, 3, (B,), generator=g)]
    for P in (32, 16):
        query = torch.randn(B, H, 1, D, generator=g).to(dev)
        loc = (centre[:, None, None] + torch.randn(B, H, P, 2, generator=g) * obj_stride[:, None, None, None]).to(dev)
        c = loc / stride - 0.5
        inside = float(((c[..., 0] >= 0) & (c[..., 0] <= w - 1) & (c[..., 1] >= 0) & (c[..., 1] <= h - 1)).float().mean())
        added = atomic_bytes(loc.cpu(), stride, h, w, D)
        lines.append(f'P = {P}: {100 * inside:.1f} % of the samples inside the map; the backward adds {added / 1e6:.1f} MB with float atomics '
                     f'and zero-fills {2 * NI * E * h * w * 4 / 1e6:.0f} MB')
        for layout in ('channels_last', 'nchw'):
            fmt = torch.channels_last if layout == 'channels_last' else torch.contiguous_format
            k_, v_ = key.contiguous(memory_format=fmt), value.contiguous(memory_format=fmt)
            leaves = [t.clone().requires_grad_(True) for t in (query, k_, v_, loc)]
            fused = lambda q, k, v, l: deform.sample_attend(q, k, v, x2d, mask, l, img, stride)
            comp = lambda q, k, v, l: composite(q, k, v, x2d, mask, l, img, stride)
            with torch.no_grad():
                cot = [torch.randn_like(o) for o in fused(query, k_, v_, loc)]
                diff = [float((x - y).abs().max()) for x, y in zip(fused(query, k_, v_, loc), comp(query, k_, v_, loc))]
            lines.append(f'  {layout} maps; largest |fused - composite| per output {" ".join(f"{d:.1e}" for d in diff)}')

            def fwd(fn):
                with torch.no_grad():
                    fn(query, k_, v_, loc)

            def both(fn):
                outs = fn(*leaves)
                torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cot)), leaves)
            for name, fn in (('fused op', fused), ('torch composite', comp)):
                for _ in range(warm):
                    both(fn)
                torch.cuda.synchronize()
                with ClockSampler(0) as clk:
                    ms_f = event_ms(lambda: fwd(fn), n)
                    ms_b = event_ms(lambda: both(fn), n)
                lines.append(f'    {name + ", forward (events)":48s} {ms_f * 1e3:10.1f} us')
                lines.append(f'    {name + ", forward + backward (events)":48s} {ms_b * 1e3:10.1f} us   clocks {json.dumps(clk.summary())}')
                if fn is fused:
                    sf, nf, sb, nb = stage_pair_ms(lambda: both(fn), n)
                    lines.append(f'    {"  its forward launch (stage recorder)":48s} {sf * 1e3:10.1f} us')
                    bufs = [torch.empty_like(k_), torch.empty_like(v_)]
                    fill = event_ms(lambda: [b.zero_() for b in bufs], n)
                    del bufs
                    rest = max(sb - fill, 1e-6)
                    lines.append(f'    {"  its backward: zero fill + scatter launch":48s} {sb * 1e3:10.1f} us   of which about {fill * 1e3:.1f} us '
                                 f'zero fill (torch zero_ of two such buffers); the rest adds {added / (rest * 1e-3) / 1e12:.3f} TB/s = '
                                 f'{100 * added / (rest * 1e-3) / 1.3e12:.0f} % of the 1.3 TB/s atomic rate')
            del leaves, k_, v_
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
