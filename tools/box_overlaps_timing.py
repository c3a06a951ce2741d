"""Time epropnp_box_overlap and epropnp_box_overlap_segmented on the device with the library's stage recorder.

    python tools/box_overlaps_timing.py [--out profiles/box_overlaps_timing.txt]

  * aligned box3d_overlaps at N = 600 under the reference's torch height rule: the detection head's score targets, once per step;
  * pairwise box3d_overlaps and rotated_overlaps at 4096 x 4096 in pairs per second, next to bev_iou on the same boxes in the same run
    (the yardstick: the 3D pair adds two loads and about ten flops to a routine of a few hundred);
  * the KITTI-val-like evaluation: 3769 images with 0..24 ground truths and 0..50 detections each, 3D boxes with KITTI's height --
    ONE segmented launch over the per-image blocks, against the reference's scheme on the same device: one pairwise call per part of
    50 images (every pair of the part) with the per-image blocks sliced out afterwards.  Kernel time from the stage recorder, and the
    time of the Python calls from events around them (the segmented call includes the host-side tile table and its copy).
Scenes are clustered near-duplicate boxes (the recipe of tests/test_boxes.py).  Means over the launches after warm-up, with the engine /
memory clocks bench.py's sampler reads while they run.  There is no pass / fail ratio, the file is the record."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from boxes_timing import scene             # noqa: E402


def scene7(N, seed):
    """the BEV scene with a centre height of 1 + N(0, 0.15) and a height of 1.6 U(0.85, 1.15): rows [x, y, z, l, h, w, ry]"""
    b = scene(N, 1, seed)[0].numpy()
    rng = np.random.default_rng(seed + 1000)
    y, h = 1.0 + rng.normal(0.0, 0.15, N), 1.6 * rng.uniform(0.85, 1.15, N)
    return torch.from_numpy(np.stack((b[:, 0], y, b[:, 1], b[:, 2], h, b[:, 3], b[:, 4]), 1).astype(np.float32))


def events_ms(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import _hip, boxes as bx
    dev = torch.device('cuda:0')
    n, warm = a.launches, 5
    lines = [f'box overlap timing: mean of {n} launches after {warm} warm-up launches; {torch.cuda.get_device_name(0)}; clustered scenes, '
             f'TILE {bx.TILE}']

    def timed(label, fn, stage, pairs=None, launches_per_call=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            _hip.profile(True, reset=True)
            for _ in range(n):
                fn()
            ms, count = _hip.profile_read(stage)
            _hip.profile(False, reset=True)
        assert count == n * launches_per_call, (stage, count)
        ms *= launches_per_call
        rate = f'{pairs / ms / 1e6:8.2f} G pairs/s   ' if pairs else ''
        lines.append(f'{label + " (stage recorder)":58s} {ms * 1e3:10.2f} us   {rate}clocks {json.dumps(clk.summary())}')
        return ms

    b7 = scene7(1200, 5).to(dev)
    timed('aligned box3d_overlaps N=600, reference_torch', lambda: bx.box3d_overlaps(b7[:600], b7[600:], aligned=True, height_rule='reference_torch'),
          'box_overlap')
    ms = events_ms(lambda: bx.bbox3d_overlaps_aligned_torch(b7[:600], b7[600:]), n)
    lines.append(f'{"  bbox3d_overlaps_aligned_torch, events around the call":58s} {ms * 1e3:10.2f} us')
    M = 4096
    b7 = scene7(M, 7).to(dev)
    b5 = b7[:, [0, 2, 3, 5, 6]].contiguous()
    iou = timed(f'bev_iou {M}x{M} (the yardstick)', lambda: bx.bev_iou(b5, b5), 'bev_overlap', M * M)
    rot = timed(f'rotated_overlaps {M}x{M} iou', lambda: bx.rotated_overlaps(b5, b5), 'box_overlap', M * M)
    d3 = timed(f'box3d_overlaps {M}x{M} iou', lambda: bx.box3d_overlaps(b7, b7), 'box_overlap', M * M)
    iou2 = timed(f'bev_iou {M}x{M} once more (the clocks ramp up on the way)', lambda: bx.bev_iou(b5, b5), 'bev_overlap', M * M)
    lines.append(f'  pair rate against bev_iou before / after: rotated_overlaps {iou / rot:.3f} / {iou2 / rot:.3f} x, box3d_overlaps {iou / d3:.3f} / '
                 f'{iou2 / d3:.3f} x (expected: no less than 0.8 x)')
    # the KITTI-val-like evaluation
    rng = np.random.default_rng(11)
    images, part = 3769, 50
    gts, dts = rng.integers(0, 25, images), rng.integers(0, 51, images)
    g7, d7 = scene7(int(gts.sum()), 8).to(dev), scene7(int(dts.sum()), 8).to(dev)
    d7 = d7 + 0.05
    counts = (gts.tolist(), dts.tolist())
    blocks = int((gts * dts).sum())
    go, do = np.concatenate(([0], np.cumsum(gts))), np.concatenate(([0], np.cumsum(dts)))
    parts = [(i, min(i + part, images)) for i in range(0, images, part)]
    all_pairs = sum(int(go[j] - go[i]) * int(do[j] - do[i]) for i, j in parts)

    def segmented():
        return bx.box3d_overlaps(g7, d7, z_axis=1, z_center=1.0, counts=counts)

    def per_part():
        out = []
        for i, j in parts:
            full = bx.box3d_overlaps(g7[go[i]:go[j]], d7[do[i]:do[j]], z_axis=1, z_center=1.0)
            r0, c0 = int(go[i]), int(do[i])
            out.extend(full[go[k] - r0:go[k + 1] - r0, do[k] - c0:do[k + 1] - c0] for k in range(i, j))
        return out
    flat, views = segmented()
    ref = per_part()
    same = all(torch.equal(x, y) for x, y in zip(views, ref))
    lines.append(f'KITTI-val-like: {images} images, {int(gts.sum())} gts, {int(dts.sum())} dts: {blocks} pairs in the per-image blocks, '
                 f'{all_pairs} pairs in the {len(parts)} parts of {part} images; the same bits either way: {same}')
    seg = timed('  ONE segmented launch', segmented, 'box_overlap_segmented')
    par = timed(f'  {len(parts)} pairwise launches, one per part', per_part, 'box_overlap', launches_per_call=len(parts))
    seg_e, par_e = events_ms(segmented, n), events_ms(per_part, n)
    lines.append(f'{"  events around the Python calls: segmented":58s} {seg_e * 1e3:10.2f} us   per part, blocks sliced out {par_e * 1e3:10.2f} us')
    lines.append(f'  per-part scheme / segmented launch: kernels {par / seg:.2f} x, Python calls {par_e / seg_e:.2f} x')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
