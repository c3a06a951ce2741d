"""Time epropnp.roi.logsumexp_across_rois (epropnp_roi_logsumexp_forward / _backward) on the device next to two PyTorch formulations.

    python tools/roi_timing.py [--out profiles/roi_timing.txt]

The detection training shape: 6 images of 928 x 1600, 192 active GT RoIs (32 per image, width and height 20 .. 400 px, centres
uniform over the image), maps of 28 x 28 with c = 8 (the attention logits of deform_pnp_head.py:985) and c = 1 (the mixture
log-likelihood of the reprojection loss).  Forward, and forward + backward with a random cotangent.

Yardsticks, on the same device and tensors:
  loop     the reference's formulation (inter_roi_ops.py:19-81), restated in `loop` below: per RoI the overlap boxes, boolean indexing
           (which synchronises with the host), affine_grid, grid_sample, masked_fill, logsumexp, autograd for the backward
  batched  `batched` below: the list of neighbour pairs and their affine maps built ONCE outside the timed region (a training step
           would have to rebuild them per step: this flatters it), one grid_sample over all pairs, a segmented logsumexp with
           scatter_reduce / index_add
Events around the Python calls (mean after warm-up); for the fused op the library's stage recorder gives the device time of the two
launches as well.  Engine / memory clocks as bench.py's sampler reads them while the loops run.  There is no pass / fail ratio, the
file is the record.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import event_ms      # noqa: E402


def loop(x, rois):
    n, c, rh, rw = x.shape
    ids, box = rois[:, 0].round().int(), rois[:, 1:]
    rows = []
    for i in range(n):
        lo, hi = torch.max(box[i, :2], box[:, :2]), torch.min(box[i, 2:], box[:, 2:])
        pos = (ids == ids[i]) & (ids[i] >= 0) & ((hi - lo) > 0).all(1)
        pos[i] = False
        if not pos.any():
            rows.append(x[i])
            continue
        js = pos.nonzero().squeeze(1)
        wh_i, wh_j = box[i, 2:] - box[i, :2], box[js, 2:] - box[js, :2]
        scale = wh_i / wh_j
        corner_j = 2 * (lo[js] - box[js, :2]) / wh_j - 1
        corner_i = 2 * (lo[js] - box[i, :2]) / wh_i - 1
        theta = x.new_zeros((len(js), 2, 3))
        theta[:, 0, 0], theta[:, 1, 1] = scale[:, 0], scale[:, 1]
        theta[:, :, 2] = corner_j - scale * corner_i
        grid = F.affine_grid(theta, (len(js), 1, rh, rw), align_corners=False)
        s = F.grid_sample(x[js], grid, padding_mode='border', align_corners=False)
        ok = ((grid > -1) & (grid < 1)).all(3).unsqueeze(1)
        rows.append(torch.cat((s.masked_fill(~ok, float('-inf')), x[i][None])).logsumexp(0))
    return torch.stack(rows)


def pair_plan(rois, rh, rw):
    """what `batched` needs of the boxes, built once: the pair list (i, j), the sampling grid of every pair and its validity"""
    ids, box = rois[:, 0].round(), rois[:, 1:]
    lo, hi = torch.max(box[:, None, :2], box[None, :, :2]), torch.min(box[:, None, 2:], box[None, :, 2:])
    nb = (ids[:, None] == ids[None]) & (ids[:, None] >= 0) & ((hi - lo) > 0).all(2)
    nb.fill_diagonal_(False)
    i, j = nb.nonzero(as_tuple=True)
    wh_i, wh_j = box[i, 2:] - box[i, :2], box[j, 2:] - box[j, :2]
    theta = rois.new_zeros((len(i), 2, 3))
    theta[:, 0, 0], theta[:, 1, 1] = (wh_i / wh_j).unbind(1)
    theta[:, :, 2] = (2 * (box[i, :2] - box[j, :2]) + wh_i) / wh_j - 1
    grid = F.affine_grid(theta, (len(i), 1, rh, rw), align_corners=False)
    return i, j, grid, ((grid > -1) & (grid < 1)).all(3).unsqueeze(1)


def batched(x, plan):
    i, j, grid, ok = plan
    s = F.grid_sample(x[j], grid, padding_mode='border', align_corners=False).masked_fill(~ok, float('-inf'))
    idx = i[:, None, None, None].expand_as(s)
    top = x.detach().scatter_reduce(0, idx, s.detach(), 'amax', include_self=True)
    total = (x - top).exp().index_add(0, i, (s - top[i]).exp())
    return top + total.log()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import _hip, roi
    dev = torch.device('cuda:0')
    n, warm = a.launches, 3
    images, per, H, W, rh, rw = 6, 32, 928, 1600, 28, 28
    g = torch.Generator().manual_seed(21)
    centre = torch.rand(images * per, 2, generator=g) * torch.tensor([float(W), float(H)])
    half = (20 + 380 * torch.rand(images * per, 2, generator=g)) / 2
    ids = torch.arange(images).repeat_interleave(per).float()[:, None]
    rois = torch.cat((ids, centre - half, centre + half), 1).to(dev)
    plan = pair_plan(rois, rh, rw)
    pairs = len(plan[0])
    with_nb = int(torch.unique(plan[0]).numel())
    lines = [f'roi.logsumexp_across_rois timing: mean of {n} calls ({max(n // 10, 3)} for the loop) after {warm} warm-up calls; {torch.cuda.get_device_name(0)}',
             f'{images} images of {H} x {W}, {images * per} RoIs ({per} per image, 20 .. 400 px), maps {rh} x {rw}; {pairs} ordered neighbour pairs '
             f'({pairs // 2} overlapping pairs of boxes), {with_nb} RoIs have a neighbour, at most {int(torch.bincount(plan[0]).max())} per RoI']
    for c in (8, 1):
        x = (3 * torch.randn(images * per, c, rh, rw, generator=g)).to(dev)
        cot = torch.randn(x.shape, generator=g).to(dev)
        leaf = x.clone().requires_grad_(True)
        forms = (('fused op', lambda t: roi.logsumexp_across_rois(t, rois), n), ('torch, batched over the pairs', lambda t: batched(t, plan), n),
                 ('torch, the loop over RoIs', lambda t: loop(t, rois), max(n // 10, 3)))
        with torch.no_grad():
            ref = forms[0][1](x)
            diff = [float((fn(x) - ref).abs().max()) for _, fn, _ in forms[1:]]
        lines.append(f'c = {c}: largest |fused - batched| {diff[0]:.1e}, |fused - loop| {diff[1]:.1e}')
        for name, fn, reps in forms:
            def fwd():
                with torch.no_grad():
                    fn(x)

            def both():
                torch.autograd.grad((fn(leaf) * cot).sum(), leaf)
            for _ in range(warm if reps == n else 1):
                both()
            torch.cuda.synchronize()
            with ClockSampler(0) as clk:
                ms_f = event_ms(fwd, reps)
                ms_b = event_ms(both, reps)
            lines.append(f'    {name + ", forward (events)":52s} {ms_f * 1e3:10.1f} us')
            lines.append(f'    {name + ", forward + backward (events)":52s} {ms_b * 1e3:10.1f} us   clocks {json.dumps(clk.summary())}')
            if name == 'fused op':
                _hip.profile(True, reset=True)
                for _ in range(reps):
                    both()
                sf, nf = _hip.profile_read('roi_logsumexp_forward')
                sb, nb = _hip.profile_read('roi_logsumexp_backward')
                _hip.profile(False, reset=True)
                lines.append(f'    {"  its forward launch (stage recorder)":52s} {sf * 1e3:10.1f} us   ({nf} launches)')
                lines.append(f'    {"  its backward launch (stage recorder)":52s} {sb * 1e3:10.1f} us   ({nb} launches)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
