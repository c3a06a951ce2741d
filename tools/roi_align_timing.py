"""Time epropnp.roi.extract_rois (epropnp_roi_align_forward / _backward) on the device next to a floor and a PyTorch composite.

    python tools/roi_align_timing.py [--out profiles/roi_align_timing.txt]

The detection training shape: 6 images of 928 x 1600, 192 active GT RoIs (32 per image, width and height 20 .. 400 px, centres
uniform over the image), key / value (6, 256, 232, 400) at 1 / 4 of the image, img_dense_x2d (6, 2, 928, 1600), 28 x 28 cells.
Forward of extract_rois, and forward + backward w.r.t. key and value with random cotangents, with NCHW and with channels-last maps.

Yardsticks, taken in the same run on the same device:
  floor      forward: a device copy of the bytes of key_roi and value_roi (read + write); backward: a fill of the two gradient maps plus
             a read (sum) of the two cotangents.  What any implementation has to move at the very least.
  composite  PyTorch on the same device, `composite` below: per image ONE grid_sample (border padding, align_corners=False) over the
             stacked sample grids of the image's RoIs, times the out-of-range mask, then avg_pool2d over the sample grid.  The grids and
             masks are built once outside the timed region (a training step would rebuild them: this flatters it).  The adaptive grid
             needs a per-RoI loop in PyTorch, so BOTH sides run at sampling_ratio = 2 for this comparison; the adaptive grid
             (sampling_ratio = 0, what the head uses) is timed for the fused op alone.
Events around the Python calls, mean after warm-up, over windows of a few hundred milliseconds; bytes / s are the bytes the op has to
write (forward: the three outputs; backward: the two gradient maps) plus those it has to read at least once (forward: nothing counted
-- the RoIs cover the maps only in part; backward: the two cotangents), over the event time, next to the 8 TB/s HBM peak.  Engine /
memory clocks as bench.py's sampler reads them while the loops run.  There is no pass / fail ratio, the file is the record.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import event_ms      # noqa: E402

PEAK = 8.0e12


def plan(rois, images, shape, out_size, scale, sampling):
    """per image: the indices of its RoIs, the normalised sample grid (1, R ph s, pw s, 2) and the out-of-range mask, aligned=True"""
    h, w = shape
    ph, pw = out_size
    plans = []
    for n in range(images):
        idx = (rois[:, 0] == n).nonzero().squeeze(1)
        r = rois[idx].double()
        xs, ys = r[:, 1] * scale - 0.5, r[:, 2] * scale - 0.5
        bw, bh = (r[:, 3] - r[:, 1]) * scale / pw, (r[:, 4] - r[:, 2]) * scale / ph
        sy = (torch.arange(ph * sampling, device=rois.device, dtype=torch.float64) + 0.5) / sampling
        sx = (torch.arange(pw * sampling, device=rois.device, dtype=torch.float64) + 0.5) / sampling
        y = ys[:, None] + sy[None] * bh[:, None]                 # (R, ph s)
        x = xs[:, None] + sx[None] * bw[:, None]                 # (R, pw s)
        ok = ((y >= -1) & (y <= h))[:, :, None] & ((x >= -1) & (x <= w))[:, None, :]
        gy, gx = (y + 0.5) * 2 / h - 1, (x + 0.5) * 2 / w - 1
        grid = torch.stack((gx[:, None, :].expand(-1, ph * sampling, -1), gy[:, :, None].expand(-1, -1, pw * sampling)), -1)
        plans.append((idx, grid.reshape(1, -1, pw * sampling, 2).float(), ok.reshape(1, 1, -1, pw * sampling).float()))
    return plans


def composite(x, plans, bn, out_size, sampling):
    ph, pw = out_size
    out = x.new_empty((bn, x.shape[1], ph, pw))
    for n, (idx, grid, ok) in enumerate(plans):
        s = F.grid_sample(x[n:n + 1], grid, mode='bilinear', padding_mode='border', align_corners=False) * ok
        cells = F.avg_pool2d(s, sampling)                        # (1, C, R ph, pw)
        out[idx] = cells.reshape(x.shape[1], len(idx), ph, pw).transpose(0, 1)
    return out


def footprint_terms(rois, shape, out_size, scale):
    """sum over the RoIs of (map rows under its cell rows) x (map columns under its cell columns) on the adaptive, aligned grid: the
    multiply-adds per channel of the separable forward (every map element under a cell is read once per cell)"""
    h, w = shape
    total = 0
    for _, x1, y1, x2, y2 in rois.double().cpu().tolist():
        spans = []
        for c1, c2, cells, size in ((y1, y2, out_size[0], h), (x1, x2, out_size[1], w)):
            start, bin_ = c1 * scale - 0.5, (c2 - c1) * scale / cells
            g = math.ceil(bin_)
            n = 0
            for c in range(cells):
                first, last = start + c * bin_ + 0.5 * bin_ / g, start + c * bin_ + (g - 0.5) * bin_ / g
                if last >= -1 and first <= size:
                    n += min(int(min(max(last, 0), size - 1)) + 1, size - 1) - int(min(max(first, 0), size - 1)) + 1
            spans.append(n)
        total += spans[0] * spans[1]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ms', type=float, default=300.0, help='length of a timed window')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import _hip, roi
    dev = torch.device('cuda:0')
    images, per, H, W, C, stride, cells = 6, 32, 928, 1600, 256, 4, (28, 28)
    h, w, bn = H // stride, W // stride, images * per
    g = torch.Generator().manual_seed(21)
    centre = torch.rand(bn, 2, generator=g) * torch.tensor([float(W), float(H)])
    half = (20 + 380 * torch.rand(bn, 2, generator=g)) / 2
    ids = torch.arange(images).repeat_interleave(per).float()[:, None]
    rois = torch.cat((ids, centre - half, centre + half), 1).to(dev)
    x2d = torch.randn(images, 2, H, W, device=dev)
    out_bytes = 4 * bn * cells[0] * cells[1] * (2 * C + 2)
    map_bytes = 4 * images * C * h * w
    cot_bytes = 4 * bn * cells[0] * cells[1] * 2 * C
    lines = [f'roi.extract_rois timing: event means over windows of about {a.ms:.0f} ms after warm-up; {torch.cuda.get_device_name(0)}',
             f'{images} images of {H} x {W}, {bn} RoIs ({per} per image, 20 .. 400 px), key / value ({images}, {C}, {h}, {w}), x2d ({images}, 2, {H}, {W}), '
             f'{cells[0]} x {cells[1]} cells; outputs {out_bytes / 1e6:.0f} MB, the two gradient maps {2 * map_bytes / 1e6:.0f} MB, the two cotangents {cot_bytes / 1e6:.0f} MB']

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        once = max(event_ms(fn, 3), 1e-3)
        with ClockSampler(0) as clk:
            ms = event_ms(fn, max(int(a.ms / once), 5))
        return ms, clk.summary()

    def row(name, ms, nbytes, clk=None, floor=None):
        text = f'    {name:66s} {ms * 1e3:9.1f} us   {nbytes / ms / 1e9:7.2f} TB/s = {100 * nbytes / ms * 1e3 / PEAK:5.1f} % of 8 TB/s'
        if floor:
            text += f'   {ms / floor:5.2f} x floor'
        if clk is not None:
            text += f'   clocks {json.dumps(clk)}'
        lines.append(text)

    # the floors
    src = torch.randn(2, bn, C, *cells, device=dev)
    dst = torch.empty_like(src)
    gm = torch.empty(2, images, C, h, w, device=dev)
    floor_f, clk = timed(lambda: dst.copy_(src))
    lines.append('floors')
    row('forward: copy of the bytes of key_roi and value_roi', floor_f, 2 * src.numel() * 4, clk)

    def floor_backward():
        gm.zero_()
        src.sum()
    floor_b, clk = timed(floor_backward)
    row('backward: fill of the two gradient maps + read of the two cotangents', floor_b, 2 * map_bytes + cot_bytes, clk)
    del dst, gm

    for fmt, name in ((torch.contiguous_format, 'NCHW'), (torch.channels_last, 'channels-last')):
        key = torch.randn(images, C, h, w, device=dev).contiguous(memory_format=fmt).requires_grad_(True)
        value = torch.randn(images, C, h, w, device=dev).contiguous(memory_format=fmt).requires_grad_(True)
        cots = [c.contiguous(memory_format=fmt) for c in src.unbind(0)]
        lines.append(f'{name} maps')
        for sampling in (0, 2):
            def fused(k=key, v=value):
                x2d_roi = roi.roi_align(x2d, rois, cells, 1.0, sampling)
                kr, vr = roi._roi_align([k, v], rois, cells, 1.0 / stride, sampling, 'avg', True, 'timing')
                return x2d_roi, kr, vr

            def fwd():
                with torch.no_grad():
                    fused()

            def both():
                _, kr, vr = fused()
                torch.autograd.grad([kr, vr], [key, value], cots)
            tag = 'adaptive grid' if sampling == 0 else 'sampling_ratio 2'
            ms_f, clk_f = timed(fwd)
            ms_b, clk_b = timed(both)
            row(f'fused, {tag}: forward (x2d launch + key/value launch)', ms_f, out_bytes, clk_f, floor_f)
            with torch.no_grad():
                ms_x, _ = timed(lambda: roi.roi_align(x2d, rois, cells, 1.0, sampling))
            row('    of which the x2d launch', ms_x, 4 * bn * 2 * cells[0] * cells[1])
            row('    of which the key/value launch', ms_f - ms_x, out_bytes - 4 * bn * 2 * cells[0] * cells[1], None, floor_f)
            if sampling == 0 and (ms_f - ms_x) > 2 * floor_f:
                fma = 2 * C * footprint_terms(rois, (h, w), cells, 1.0 / stride)
                lines.append(f'        where the time goes: the launch is {(ms_f - ms_x) / floor_f:.1f} x the copy floor and moves its output at a few per cent of '
                             f'the HBM peak, so HBM bandwidth is not what it waits for.  It executes {fma / 1e9:.2f} G fp64 multiply-adds (counted from the '
                             f'boxes: every map element under a cell, once per cell and channel), {fma / (ms_f - ms_x) / 1e9:.1f} T/s against the 39.3 T/s '
                             f'fp64 vector peak ({100 * fma / (ms_f - ms_x) * 1e3 / 39.3e12:.0f} % of it), so arithmetic is not it either.  A thread walks '
                             f'its 28 (channel, cell) pairs one after the other; each pair is a few dependent trips of gathers from rows of the map that '
                             f'lie {w * (C if fmt == torch.channels_last else 1) * 4} bytes apart, and the thread waits for each trip: the launch is bound by load latency at the occupancy the '
                             f'17 KB table per workgroup and 94 VGPRs allow.  Evidence: issuing 16 independent loads per trip instead of 1 took this launch '
                             f'from 1110 to about 650 us with the arithmetic unchanged.  Not separated further: no counter run was taken.  Next steps, '
                             f'not measured: a workgroup per RoI and several cell rows (tables built once, map rows shared between neighbouring '
                             f'cell rows in LDS), fp32 tables.')
            row(f'fused, {tag}: forward + backward', ms_b, out_bytes + 2 * map_bytes + cot_bytes, clk_b, floor_f + floor_b)
            row('    backward alone (difference)', ms_b - ms_f, 2 * map_bytes + cot_bytes, None, floor_b)
            _hip.profile(True, reset=True)
            for _ in range(5):
                both()
            sf, nf = _hip.profile_read('roi_align_forward')
            sb, nb = _hip.profile_read('roi_align_backward')
            _hip.profile(False, reset=True)
            lines.append(f'        stage recorder: forward launches {sf * 1e3:.1f} us mean of {nf} (x2d and key/value alternate), backward launch {sb * 1e3:.1f} us mean of {nb}')
        pk, px = plan(rois, images, (h, w), cells, 1.0 / stride, 2), plan(rois, images, (H, W), cells, 1.0, 2)

        def comp(k=key, v=value):
            return composite(x2d, px, bn, cells, 2), composite(k, pk, bn, cells, 2), composite(v, pk, bn, cells, 2)
        with torch.no_grad():
            ref, got = fused(key.detach(), value.detach()), comp(key.detach(), value.detach())     # sampling == 2 here
            diff = max(float((r - c).abs().max()) for r, c in zip(ref, got))
        lines.append(f'    largest |fused - composite| at sampling_ratio 2: {diff:.1e}')

        def comp_fwd():
            with torch.no_grad():
                comp()

        def comp_both():
            _, kr, vr = comp()
            torch.autograd.grad([kr, vr], [key, value], cots)
        ms_f, clk_f = timed(comp_fwd)
        ms_b, clk_b = timed(comp_both)
        row('torch composite, sampling_ratio 2: forward', ms_f, out_bytes, clk_f, floor_f)
        row('torch composite, sampling_ratio 2: forward + backward', ms_b, out_bytes + 2 * map_bytes + cot_bytes, clk_b, floor_f + floor_b)
        del key, value, cots
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
