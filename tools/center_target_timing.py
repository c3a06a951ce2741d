"""Time epropnp.targets.volume_centers on the device, next to the same maths written in batched PyTorch on the same device.

    python tools/center_target_timing.py [--out profiles/center_target_timing.txt]

  * the fused op at the Det training shape (6 images, 192 objects, 900 x 1600 images: 232 x 400 output cells, 225 x 400 render pixels,
    strides 4 / 4, faces_per_pixel 16) and at a few objects (6 images, 12 objects): the three launches from the library's stage
    recorder, and device events around the Python call;
  * the same definition in batched PyTorch: the slab test of every object on the full render grid, the faces_per_pixel-th nearest
    fragment of each image pixel by kthvalue, grid_sample at the cells, the sums.  Device events around the call.  It never builds
    the reference's (num_obj, num_img, h_rend, w_rend, faces_per_pixel) comparison, so it is a kinder yardstick than the reference's
    post_proc would be; nothing of the reference is read or run here;
  * peak allocated memory above the inputs for both, and the largest centre difference between the two on the objects both keep.
Scenes are seeded random boxes in front of a nuScenes-like camera.  Means over the calls after warm-up, with the engine / memory
clocks bench.py's sampler reads while they run.  There is no pass / fail ratio, the file is the record."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

Z_CLIP = 1e-2


def scene(num_img, per_img, seed, dev):
    rng = np.random.default_rng(seed)
    n = num_img * per_img
    z = rng.uniform(5.0, 60.0, n)
    boxes = np.stack((rng.uniform(3.5, 5.0, n), rng.uniform(1.4, 2.0, n), rng.uniform(1.6, 2.1, n), rng.uniform(-0.55, 0.55, n) * z,
                      rng.uniform(0.5, 1.5, n), z, rng.uniform(-math.pi, math.pi, n)), 1).astype(np.float32)
    inds = np.repeat(np.arange(num_img), per_img)
    cam = np.tile(np.array([[1266.0, 0.0, 816.0], [0.0, 1266.0, 491.0], [0.0, 0.0, 1.0]], dtype=np.float32), (num_img, 1, 1))
    h, w = 232, 400
    x, y = np.meshgrid(np.arange(w) * 4 + 1.5, np.arange(h) * 4 + 1.5)
    x2d = np.stack((x, y))[None].repeat(num_img, 0).astype(np.float32)
    x2d[1::2, 0] = 1599.0 - x2d[1::2, 0]                                   # every second image flipped
    mask = np.ones((num_img, 1, h, w), dtype=np.float32)
    mask[:, :, 225:] = 0.0                                                # the rows that pad 900 to 928
    return [torch.from_numpy(a).to(dev) for a in (boxes, inds, cam, x2d, mask)]


def torch_centers(boxes, inds, cam, x2d, mask, max_shape, os_=4, rs=4, fpp=16, min_box=4.0):
    """the definition of epropnp_volume_centers in batched PyTorch (get_bbox_2d): every object on the full render grid"""
    dev = boxes.device
    B, G = boxes.shape[0], cam.shape[0]
    pad_h, pad_w = (int(math.ceil(s / os_)) * os_ for s in max_shape)
    Hr, Wr = pad_h // rs, pad_w // rs
    u = rs * (torch.arange(Wr, device=dev, dtype=torch.float32) + 0.5) - 0.5
    v = rs * (torch.arange(Hr, device=dev, dtype=torch.float32) + 0.5) - 0.5
    K = cam[inds]
    dx = ((u[None, None, :] - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None]).expand(B, Hr, Wr)
    dy = ((v[None, :, None] - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None]).expand(B, Hr, Wr)
    c, s = torch.cos(boxes[:, 6])[:, None, None], torch.sin(boxes[:, 6])[:, None, None]
    X, Y, Z = (boxes[:, k, None, None] for k in (3, 4, 5))
    o = (-(c * X - s * Z), -Y, -(s * X + c * Z))
    d = (c * dx - s, dy, s * dx + c)
    lo = torch.full((B, Hr, Wr), -math.inf, device=dev)
    hi = torch.full((B, Hr, Wr), math.inf, device=dev)
    for k in range(3):
        e = 0.5 * boxes[:, k, None, None]
        t1, t2 = (-e - o[k]) / d[k], (e - o[k]) / d[k]
        lo, hi = torch.maximum(lo, torch.minimum(t1, t2)), torch.minimum(hi, torch.maximum(t1, t2))
    hit = lo <= hi
    own = hit & (hi > lo) & (lo > Z_CLIP)
    # the fpp-th nearest fragment of each image pixel: the far face must lie in front of it or be it
    frag = torch.stack((torch.where(hit & (lo > Z_CLIP), lo, math.inf), torch.where(hit & (hi > Z_CLIP), hi, math.inf)), 1)      # (B, 2, Hr, Wr)
    per = B // G
    if 2 * per > fpp:
        kth = frag.reshape(G, per * 2, Hr, Wr).kthvalue(fpp, dim=1).values                                                     # (G, Hr, Wr)
        own = own & (hi <= kth[inds])
    thick = torch.where(own, hi - lo, 0.0)
    grid = torch.stack((((x2d[:, 0] + 0.5) / rs - 0.5 + 0.5) * 2 / Wr - 1, ((x2d[:, 1] + 0.5) / rs - 0.5 + 0.5) * 2 / Hr - 1), -1)[inds]
    both = F.grid_sample(torch.stack((thick, own.float()), 1), grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    both = both * mask[inds]
    t, vm = both[:, 0], both[:, 1]
    h, w = t.shape[1:]
    py = (torch.arange(h, device=dev, dtype=torch.float32) * os_ + os_ / 2)[None, :, None]
    px = (torch.arange(w, device=dev, dtype=torch.float32) * os_ + os_ / 2)[None, None, :]
    W = t.sum((1, 2))
    centers = torch.stack(((t * px).sum((1, 2)), (t * py).sum((1, 2))), 1) / W[:, None]
    on = vm >= 0.5
    cols, rows = on.any(1), on.any(2)
    xs, ys = torch.arange(w, device=dev, dtype=torch.float32) * os_, torch.arange(h, device=dev, dtype=torch.float32) * os_
    x1 = torch.where(cols, xs, float(w * os_)).amin(1)
    x2 = torch.where(cols, xs, 0.0).amax(1) + os_
    y1 = torch.where(rows, ys, float(h * os_)).amin(1)
    y2 = torch.where(rows, ys, 0.0).amax(1) + os_
    b2 = torch.stack((x1, y1, x2, y2), 1)
    valid = (W >= 1e-6) & ((b2[:, 2:] - b2[:, :2]) >= min_box).all(1)
    return centers, b2, valid


def events_ms(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool times the device: no GPU, no numbers'
    from bench import ClockSampler
    from epropnp import _hip, targets
    dev = torch.device('cuda:0')
    n, warm = a.calls, 10
    lines = [f'centre target timing: mean of {n} calls after {warm} warm-up calls; {torch.cuda.get_device_name(0)}; 900 x 1600 images, '
             f'232 x 400 cells, 225 x 400 render pixels, strides 4 / 4, faces_per_pixel 16, get_bbox_2d']
    for per_img in (32, 2):
        boxes, inds, cam, x2d, mask = scene(6, per_img, 21 + per_img, dev)

        def fused():
            return targets.volume_centers(boxes, inds, cam, x2d, mask, (900, 1600), get_bbox_2d=True)

        def batched():
            return torch_centers(boxes, inds, cam, x2d, mask, (900, 1600))
        got, want = fused(), batched()
        both = got[2] & want[2]
        diff = (got[0] - want[0])[both].abs().max().item() if bool(both.any()) else float('nan')
        lines.append(f'{6 * per_img} objects on 6 images: {int(got[2].sum())} valid (fused), {int(want[2].sum())} valid (PyTorch), '
                     f'{int((got[2] != want[2]).sum())} differ; boxes differ on {int((got[1] != want[1]).any(1).sum())}; '
                     f'largest centre difference on the objects both keep {diff:.2e} px')
        for _ in range(warm):
            fused()
            batched()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            _hip.profile(True, reset=True)
            for _ in range(n):
                fused()
            ms, count = _hip.profile_read('volume_centers')
            _hip.profile(False, reset=True)
        assert count == n, count
        lines.append(f'  {"fused, the three launches (stage recorder)":52s} {ms * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
        # alternate the two, so that both see the same clocks and neighbours
        fe, be = [], []
        for _ in range(4):
            fe.append(events_ms(fused, n // 4))
            be.append(events_ms(batched, max(n // 8, 5)))
        lines.append(f'  {"fused, events around the Python call":52s} {np.mean(fe) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in fe)})')
        lines.append(f'  {"batched PyTorch, events around the call":52s} {np.mean(be) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in be)})')
        lines.append(f'  peak allocated above the inputs: fused {peak_mb(fused):.2f} MiB, batched PyTorch {peak_mb(batched):.2f} MiB')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
