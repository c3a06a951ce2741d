"""Time epropnp_bev_nms and epropnp_bev_overlap on the device with the library's stage recorder, next to what the reference does
instead of the reduce launch: a blocking device-to-host copy of the (N, N / 64) suppression mask and a host loop over its rows.

    python tools/boxes_timing.py [--out profiles/boxes_timing.txt]

bev_nms at N = 600 / 60 groups (the detection head's step), N = 4096 / 1 group, N = 16384 / 60 groups, on scenes of clustered
near-duplicate detections (the recipe of tests/test_boxes.py), threshold 0.25, through the library call on buffers allocated once:
both launches together, and each alone (EPROPNP_TUNE="bev_nms_phase=mask" / "=reduce" on the same scratch).  The host route is timed
with a wall clock around the copy and around a numpy loop (one OR of N / 64 words per kept row) and checked to keep the same boxes;
the reference's loop is C++, the copy and its synchronisation are the same.  bev_iou at 4096 x 4096 in pairs per second.  Means
over the launches after warm-up, with the engine / memory clocks bench.py's sampler reads while they run.  There is no pass / fail
ratio, the file is the record."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import stage_ms      # noqa: E402

SIZES = np.array([(4.6, 1.9), (11.0, 2.9), (0.7, 0.7), (2.1, 0.8), (6.9, 2.5)])


def scene(N, G, seed):
    rng = np.random.default_rng(seed)
    n_obj = max(N // 4, 1)
    centre = rng.uniform([-40.0, 3.0], [40.0, 70.0], (n_obj, 2))
    size = SIZES[rng.integers(0, len(SIZES), n_obj)]
    yaw = rng.uniform(-math.pi, math.pi, n_obj)
    group = rng.integers(0, G, n_obj)
    which = rng.integers(0, n_obj, N)
    c = centre[which] + rng.normal(0.0, 1.0, (N, 2)) * (0.35 * size[which].min(1))[:, None]
    wh = size[which] * rng.uniform(0.85, 1.15, (N, 2))
    a = yaw[which] + rng.normal(0.0, 0.15, N) + math.pi * rng.integers(0, 2, N)
    boxes = np.concatenate((c, wh, a[:, None]), 1).astype(np.float32)
    return torch.from_numpy(boxes), torch.from_numpy(rng.uniform(0.05, 1.0, N).astype(np.float32)), torch.from_numpy(group[which].astype(np.int32))


def host_reduce(mask, N):
    """the reference's nms_gpu tail on a (N, T) uint64 mask of the sorted boxes: kept positions"""
    T = mask.shape[1]
    removed = np.zeros(T, dtype=np.uint64)
    keep = []
    for i in range(N):
        if not (int(removed[i >> 6]) >> (i & 63)) & 1:
            keep.append(i)
            removed |= mask[i]
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import _hip, boxes as bx
    dev = torch.device('cuda:0')
    n, warm = a.launches, 5
    lines = [f'bev_nms / bev_iou timing: mean of {n} launches after {warm} warm-up launches; {torch.cuda.get_device_name(0)}; '
             f'threshold 0.25, clustered scenes, TILE {bx.TILE}']
    for N, G in ((600, 60), (4096, 1), (16384, 60)):
        b, s, g = (t.to(dev) for t in scene(N, G, 6))
        order = torch.sort(s, descending=True, stable=True).indices.to(torch.int32)
        T = (N + bx.TILE - 1) // bx.TILE
        scratch = torch.zeros((N, T), dtype=torch.int64, device=dev)
        keep_index = torch.empty((N,), dtype=torch.int32, device=dev)
        keep_mask = torch.empty((N,), dtype=torch.uint8, device=dev)
        num_keep = torch.empty((1,), dtype=torch.int32, device=dev)
        grp = g if G > 1 else None
        call = lambda: _hip.call('epropnp_bev_nms', _hip.ptr(b), _hip.ptr(order), _hip.ptr(grp), N, 0.25, _hip.ptr(scratch),
                                 scratch.numel() * 8, _hip.ptr(keep_index), _hip.ptr(keep_mask), _hip.ptr(num_keep), _hip.stream_of(b))
        lines.append(f'N={N} groups={G}: {T * (T + 1) // 2} mask tiles, mask {N * T * 8 / 1e6:.2f} MB')
        saved = os.environ.get('EPROPNP_TUNE')
        for label, phase in (('bev_nms, both launches', None), ('  mask launch alone', 'mask'), ('  reduce launch alone', 'reduce')):
            if phase:
                os.environ['EPROPNP_TUNE'] = f'bev_nms_phase={phase}'
            for _ in range(warm):
                call()
            torch.cuda.synchronize()
            with ClockSampler(0) as clk:
                ms = stage_ms(call, 'bev_nms', n)
            lines.append(f'  {label + " (stage recorder)":44s} {ms * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
            if saved is None:
                os.environ.pop('EPROPNP_TUNE', None)
            else:
                os.environ['EPROPNP_TUNE'] = saved
        call()
        torch.cuda.synchronize()
        kept = keep_index[:int(num_keep)].cpu().tolist()
        # the reference's route from the same mask: blocking copy, host loop
        t0 = time.perf_counter()
        host = scratch.cpu()
        t1 = time.perf_counter()
        pos = host_reduce(host.numpy().view(np.uint64), N)
        t2 = time.perf_counter()
        same = order.cpu()[torch.tensor(pos, dtype=torch.int64)].tolist() == kept
        lines.append(f'  {"host route: blocking copy of the mask":44s} {(t1 - t0) * 1e6:10.2f} us   + numpy loop over the rows '
                     f'{(t2 - t1) * 1e6:.2f} us (wall clock, once); keeps {len(kept)} of {N}, the same boxes: {same}')
    M = 4096
    b, _, _ = scene(M, 1, 7)
    b = b.to(dev)
    iou = lambda: bx.bev_iou(b, b)
    for _ in range(warm):
        iou()
    torch.cuda.synchronize()
    with ClockSampler(0) as clk:
        ms = stage_ms(iou, 'bev_overlap', n)
    lines.append(f'bev_iou {M}x{M}: {ms * 1e3:10.2f} us (stage recorder)   {M * M / ms / 1e6:8.2f} G pairs/s   clocks {json.dumps(clk.summary())}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
