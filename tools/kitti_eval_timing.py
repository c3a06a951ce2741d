"""Time the KITTI AP evaluation (epropnp.evaluation) on the device with the library's stage recorder.

    python tools/kitti_eval_timing.py [--out profiles/kitti_eval_timing.txt]                      # on the device
    python tools/kitti_eval_timing.py --interpreted 60 [--out FILE --append]                      # on a CPU, next to the reference

KITTI-val-like shape: 3769 images with 0..24 ground truths and 0..50 detections each, classes Car / Pedestrian / Cyclist (and Van,
Person_sitting, DontCare among the ground truths); about half of the detections are jittered ground truths, so that every stage has
work.  Per metric (0 image boxes with AOS, 1 BEV, 2 3D) one `eval_class` call evaluates 18 cases (3 classes x 3 difficulties x the
strict and loose overlaps):
  * device time of the three stages (kitti_match, kitti_thresholds, kitti_statistics) and of the overlap launch from the stage
    recorder, and the number of launches of each per call;
  * the whole `eval_class` call: wall time, which includes the host preparation, the uploads and the final copy;
  * host time of the vectorised preparation (`prepare`: what `_prepare_data` does, for all nine class x difficulty pairs at once).
Means over the calls after warm-up, with the engine / memory clocks bench.py's sampler reads while they run.

--interpreted N: the only host baseline there is without numba -- the reference's eval_class cut out of the reference checkout
(tools/make_kitti_eval_golden.py) and run INTERPRETED on the first N images, overlaps excluded.  It is recorded as what it is; numba
would compile these loops, so the ratio to the device time is not a speed-up of anything a user runs.  There is no pass / fail
figure, the file is the record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
GT_NAMES = np.array(['Car', 'Car', 'Car', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare'])
SIZES = {'Car': (3.9, 1.5, 1.6), 'Pedestrian': (0.8, 1.75, 0.6), 'Cyclist': (1.8, 1.7, 0.6), 'Van': (5.0, 2.2, 1.9),
         'Person_sitting': (0.8, 1.3, 0.6), 'DontCare': (1.0, 1.0, 1.0)}
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5]] + [[0.5, 0.25, 0.25]] * 2])


def _anno(names, loc, dims, ry, rng, score=None):
    n = len(names)
    half = (dims[:, 0] * np.abs(np.cos(ry)) + dims[:, 2] * np.abs(np.sin(ry))) / 2
    z = loc[:, 2]
    bbox = np.stack([720 * (loc[:, 0] - half) / z + 620, 720 * (loc[:, 1] - dims[:, 1]) / z + 190, 720 * (loc[:, 0] + half) / z + 620,
                     720 * loc[:, 1] / z + 190], 1).reshape(n, 4)
    a = {'name': names, 'bbox': bbox, 'alpha': ry - np.arctan2(loc[:, 0], z), 'occluded': rng.choice(4, n, p=[0.55, 0.25, 0.12, 0.08]),
         'truncated': np.where(rng.uniform(size=n) < 0.8, 0.0, np.round(rng.uniform(0, 0.6, n), 2)), 'location': loc, 'dimensions': dims,
         'rotation_y': ry}
    if score is not None:
        a['score'] = score
    return a


def scene(images, seed):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(images):
        ng, nd = int(rng.integers(0, 25)), int(rng.integers(0, 51))
        names = GT_NAMES[rng.integers(0, len(GT_NAMES), ng)].astype('<U14')
        z = rng.uniform(6.0, 70.0, ng)
        loc = np.stack([rng.uniform(-0.45, 0.45, ng) * z, np.full(ng, 1.65), z], 1).reshape(ng, 3)
        dims = np.array([SIZES[n] for n in names]).reshape(ng, 3) * rng.uniform(0.9, 1.1, (ng, 3))
        ry = rng.uniform(-np.pi, np.pi, ng)
        gts.append(_anno(names, loc, dims, ry, rng))
        k = min(ng, nd // 2)      # detections of the first k ground truths, the rest anywhere
        z2 = rng.uniform(6.0, 70.0, nd - k)
        loc2 = np.concatenate([loc[:k] + rng.normal(0, 0.08, (k, 3)), np.stack([rng.uniform(-0.45, 0.45, nd - k) * z2, np.full(nd - k, 1.65), z2], 1)], 0)
        names2 = np.concatenate([np.where(np.isin(names[:k], ['Car', 'Pedestrian', 'Cyclist']), names[:k], 'Car'),      # found ones score higher
                                 np.array(['Car', 'Pedestrian', 'Cyclist'])[rng.integers(0, 3, nd - k)]]).astype('<U14')
        dims2 = np.concatenate([dims[:k] * rng.uniform(0.95, 1.05, (k, 3)), np.array([SIZES[n] for n in names2[k:]]).reshape(nd - k, 3)], 0)
        ry2 = np.concatenate([ry[:k] + rng.normal(0, 0.03, k), rng.uniform(-np.pi, np.pi, nd - k)])
        dts.append(_anno(names2, loc2.reshape(nd, 3), dims2.reshape(nd, 3), ry2, rng, score=np.round(np.concatenate([rng.uniform(0.4, 1.0, k), rng.uniform(0.05, 0.7, nd - k)]), 2)))
    return gts, dts


def interpreted(n_images, seed, out, append):
    import make_kitti_eval_golden as mk
    ref = mk.reference_functions()
    gts, dts = scene(3769, seed)
    gts, dts = gts[:n_images], dts[:n_images]
    lines = []
    for metric in (0, 1, 2):
        blocks = [mk.image_overlaps(ref, d, g, metric) for g, d in zip(gts, dts)]
        ref['__space__']['calculate_iou_partly'] = mk.make_calculate_iou_partly(ref, {metric: blocks})
        t0 = time.perf_counter()
        ref['eval_class'](gts, dts, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, compute_aos=(metric == 0))
        s = time.perf_counter() - t0
        lines.append(f'metric {metric}: the reference eval_class, INTERPRETED (no numba), first {n_images} of the 3769 images, 18 cases, overlaps '
                     f'given: {s:8.2f} s = {s / n_images * 1e3:8.2f} ms per image  (not a speed-up baseline: numba compiles these loops)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out:
        with open(out, 'a' if append else 'w') as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--interpreted', type=int, default=0, help='time the interpreted reference on the first N images instead (CPU)')
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.interpreted:
        return interpreted(a.interpreted, a.seed, a.out, a.append)
    import torch
    from bench import ClockSampler
    from epropnp import _hip, evaluation as ev
    images, n, warm = 3769, a.calls, 2
    gts, dts = scene(images, a.seed)
    G, D = sum(len(g['name']) for g in gts), sum(len(d['name']) for d in dts)
    lines = [f'KITTI evaluation timing: mean of {n} eval_class calls after {warm} warm-up calls; {torch.cuda.get_device_name(0)}; '
             f'{images} images, {G} ground truths, {D} detections, 18 cases per call']
    t0 = time.perf_counter()
    for _ in range(n):
        ev.prepare(gts, dts, [0, 1, 2], [0, 1, 2])
    lines.append(f'{"host: prepare (all 9 class x difficulty pairs, vectorised)":62s} {(time.perf_counter() - t0) / n * 1e3:10.2f} ms')
    stages = ('box_overlap_segmented', 'kitti_match', 'kitti_thresholds', 'kitti_statistics')
    for metric in (0, 1, 2):
        call = lambda: ev.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, compute_aos=(metric == 0))
        for _ in range(warm):
            ret = call()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            _hip.profile(True, reset=True)
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            wall = (time.perf_counter() - t0) / n
            read = {s: _hip.profile_read(s) for s in stages}
            _hip.profile(False, reset=True)
        assert all(c == n for _, c in read.values()), read
        ap11 = ev.get_mAP(ret['precision'], 'R11')[0, 1]
        lines.append(f'metric {metric}{" (with AOS)" if metric == 0 else ""}: Car moderate AP(R11) strict / loose {ap11[0]:.2f} / {ap11[1]:.2f}; '
                     f'clocks {json.dumps(clk.summary())}')
        for s in stages:
            lines.append(f'{"  " + s + " (stage recorder, 1 per call)":62s} {read[s][0] * 1e3:10.2f} us')
        dev_us = sum(read[s][0] for s in stages[1:]) * 1e3
        lines.append(f'{"  the three evaluation stages together":62s} {dev_us:10.2f} us   (+ torch.sort of the (18, G) scores between the first two)')
        lines.append(f'{"  eval_class, wall time of the call":62s} {wall * 1e3:10.2f} ms   (host preparation, uploads, launches, one copy back)')
    lines.append('launches per eval_class call, whatever the images and cases: 1 overlap launch; kitti_match = count fill + 1 kernel; '
                 'kitti_thresholds = 1 kernel; kitti_statistics = count fill + 2 kernels (per image, then the fixed-order reduce)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
