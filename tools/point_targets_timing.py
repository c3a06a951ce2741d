"""Time epropnp.targets.point_targets and obj_sampler on the device, next to the same maths written in batched PyTorch on the same
device and inputs.

    python tools/point_targets_timing.py [--out profiles/point_targets_timing.txt]

Det training shape: 6 images of 928 x 1600 at strides 8 .. 128 (116 x 200 ... 8 x 13 cells: 30 929 points per image), 32 objects per
image, regress ranges ((-1, 48), (48, 96), (96, 192), (192, 384), (384, 1e8)), 10 classes; the sampler at N = 288 on the targets that
come out.
  * point_targets: the launch from the library's stage recorder, device events around the Python call, and the same definition as ONE
    batched PyTorch expression over (image, point, object) with the objects padded per image -- padding, the level-major permutation
    and the per-point level constants are prepared outside the timed region, so it is a kinder yardstick than the reference's
    per-image Python loop over about twenty temporaries would be; nothing of the reference is read or run here;
  * obj_sampler behind injected draws: the launch from the stage recorder, events around the Python call (which reads the foreground
    count back), and the reference's arithmetic in PyTorch with a (N, N) comparison in place of its (num_gt, N) mask and the same one
    read-back; then both with their own torch.multinomial draws;
  * kernel launches per call of each side, counted by torch.profiler; peak allocated memory above the inputs; agreement of the two.
Means over the calls after warm-up, with the engine / memory clocks bench.py's sampler reads while they run.  There is no pass / fail
ratio, the file is the record."""
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

SHAPE, STRIDES = (928, 1600), (8, 16, 32, 64, 128)
RANGES = ((-1, 48), (48, 96), (96, 192), (192, 384), (384, 1e8))
NUM_CLASSES, RADIUS, ALPHA, INF = 10, 1.5, 2.5, 1e8


def scene(num_img, per_img, seed, dev):
    rng = np.random.default_rng(seed)
    n = num_img * per_img
    size = np.exp(rng.uniform(np.log(24.0), np.log(600.0), (n, 2)))
    ctr = np.stack((rng.uniform(0, SHAPE[1], n), rng.uniform(0.3 * SHAPE[0], 0.9 * SHAPE[0], n)), 1)
    boxes = np.concatenate((ctr - size / 2, ctr + size / 2), 1).astype(np.float32)
    centres = (ctr + rng.normal(0, 0.08, (n, 2)) * size).astype(np.float32)
    labels = rng.integers(0, NUM_CLASSES, n)
    inds = np.repeat(np.arange(num_img), per_img)
    return [torch.from_numpy(a).to(dev) for a in (boxes, centres, labels, inds)]


def prepare_batched(points, counts, boxes, centres, labels, num_img, per_img, dev):
    """what the batched formulation needs besides the inputs: per-point level constants, objects per image, the output permutation"""
    lvl = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(dev)
    radius = torch.tensor([s * RADIUS for s in STRIDES], dtype=torch.float32, device=dev)[lvl]
    lo = torch.tensor([r[0] for r in RANGES], dtype=torch.float32, device=dev)[lvl]
    hi = torch.tensor([r[1] for r in RANGES], dtype=torch.float32, device=dev)[lvl]
    P = points.shape[0]
    flat = torch.arange(num_img * P, device=dev).reshape(num_img, P)
    perm = torch.cat([part.reshape(-1) for part in flat.split(counts, dim=1)])
    base = torch.arange(num_img, device=dev) * per_img
    return dict(radius=radius, lo=lo, hi=hi, perm=perm, base=base, boxes=boxes.reshape(num_img, per_img, 4),
                centres=centres.reshape(num_img, per_img, 2), labels=labels.reshape(num_img, per_img))


def torch_point_targets(points, c):
    """the definition of epropnp_point_targets as one expression over (image, point, object)"""
    x, y = points[None, :, 0, None], points[None, :, 1, None]
    cx, cy = c['centres'][:, None, :, 0], c['centres'][:, None, :, 1]
    b = c['boxes'][:, None]
    s = c['radius'][None, :, None]
    inside = torch.minimum(torch.minimum(x - (cx - s), y - (cy - s)), torch.minimum((cx + s) - x, (cy + s) - y)) > 0
    reg = torch.maximum(torch.maximum(x - b[..., 0], y - b[..., 1]), torch.maximum(b[..., 2] - x, b[..., 3] - y))
    ok = inside & (reg >= c['lo'][None, :, None]) & (reg <= c['hi'][None, :, None])
    d = torch.where(ok, torch.sqrt((x - cx) ** 2 + (y - cy) ** 2), INF)
    dmin, j = d.min(-1)
    labels = torch.where(dmin == INF, NUM_CLASSES, c['labels'].gather(1, j))
    cen = torch.exp(-ALPHA * (dmin / (1.414 * c['radius'])[None]))
    gt = j + c['base'][:, None]
    perm = c['perm']
    labels = labels.reshape(-1)[perm]
    return labels, cen.reshape(-1)[perm], gt.reshape(-1)[perm], (labels < NUM_CLASSES).sum()


def torch_sampler(N, fg, cen, gt, ratio=0.5, eps=1e-5, draws=None):
    """the reference's arithmetic with a (N, N) comparison in place of the (num_gt, N) mask; one read-back, the foreground count"""
    count = int(fg.count_nonzero())
    if count == 0:
        return gt[[]], cen[[]], cen[[]]
    nu = min(int(round(N * ratio)), count)
    r = nu / N
    prob = cen * fg
    prob = prob / prob.sum().clamp(min=eps)
    uni = fg / count
    mix = uni * r + prob * (1 - r)
    if draws is None:
        draws = torch.cat((torch.multinomial(uni, nu, replacement=False), torch.multinomial(prob, N - nu, replacement=True)))
    sgt = gt[draws]
    w = prob[draws] / mix[draws]
    same = sgt[:, None] == sgt[None, :]
    sw = w / (same * w[None, :]).sum(1).clamp(min=eps)
    sw = sw / sw.mean().clamp(min=eps)
    uw = 1 / same.sum(1).clamp(min=1)
    uw = uw / uw.mean().clamp(min=eps)
    return sgt, sw, uw


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


def launches(fn):
    """kernel launches of one call, counted by torch.profiler (memory copies aside); 'n/a' where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'mem' not in e.name.lower())
        return str(n) if n else 'n/a'
    except Exception as e:      # the record says so rather than failing the timing
        return f'n/a ({type(e).__name__})'


def compare(fused, batched, n, stage, label_f, label_b):
    from bench import ClockSampler
    from epropnp import _hip
    lines = []
    for _ in range(10):
        fused()
        batched()
    torch.cuda.synchronize()
    with ClockSampler(0) as clk:
        _hip.profile(True, reset=True)
        for _ in range(n):
            fused()
        ms, count = _hip.profile_read(stage)
        _hip.profile(False, reset=True)
    assert count == n, count
    lines.append(f'  {"fused, the entry (stage recorder)":58s} {ms * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
    fe, be = [], []
    for _ in range(4):      # alternate the two, so that both see the same clocks and neighbours
        fe.append(events_ms(fused, n // 4))
        be.append(events_ms(batched, max(n // 8, 5)))
    lines.append(f'  {label_f:58s} {np.mean(fe) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in fe)})')
    lines.append(f'  {label_b:58s} {np.mean(be) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in be)})')
    lines.append(f'  kernel launches per call: fused {launches(fused)}, batched PyTorch {launches(batched)}')
    lines.append(f'  peak allocated above the inputs: fused {peak_mb(fused):.2f} MiB, batched PyTorch {peak_mb(batched):.2f} MiB')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool times the device: no GPU, no numbers'
    from epropnp import targets
    dev = torch.device('cuda:0')
    n, num_img, per_img, N = a.calls, 6, 32, 288
    sizes = [(-(-SHAPE[0] // s), -(-SHAPE[1] // s)) for s in STRIDES]
    pts = targets.fcos_points(sizes, STRIDES, torch.float32, dev)
    counts = [int(p.shape[0]) for p in pts]
    points = torch.cat(pts)
    boxes, centres, labels, inds = scene(num_img, per_img, 33, dev)
    consts = prepare_batched(points, counts, boxes, centres, labels, num_img, per_img, dev)
    lines = [f'point target timing: mean of {n} calls after 10 warm-up calls; {torch.cuda.get_device_name(0)}; {num_img} images of '
             f'{SHAPE[0]} x {SHAPE[1]}, strides {STRIDES}: {points.shape[0]} points per image, {per_img} objects per image']

    def fused():
        return targets.point_targets(points, counts, STRIDES, RANGES, boxes, labels, centres, inds, num_img, NUM_CLASSES,
                                     center_sample_radius=RADIUS, centerness_alpha=ALPHA)

    def batched():
        return torch_point_targets(points, consts)
    got, want = fused(), batched()
    differ = int((got[0] != want[0]).sum()) + int((got[2] != want[2]).sum())
    lines.append(f'point_targets: {int(got[4])} foreground points (fused), {int(want[3])} (PyTorch); labels / gt_inds differ on {differ} '
                 f'points; largest centerness difference {float((got[1] - want[1]).abs().max()):.2e}')
    lines += compare(fused, batched, n, 'point_targets', 'fused, events around the Python call', 'batched PyTorch, events around the call')
    fg, cen, gt = got[0] < NUM_CLASSES, got[1], got[2]
    torch.manual_seed(5)
    draws = torch_sampler(N, fg, cen, targets_index(fg))[0]

    def fused_s():
        return targets.obj_sampler(N, fg, cen, gt, sample_point_inds=draws)

    def batched_s():
        return torch_sampler(N, fg, cen, gt, draws=draws)
    got_s, want_s = fused_s(), batched_s()
    lines.append(f'obj_sampler, N = {N} on {fg.numel()} points, injected draws: gt indices differ on {int((got_s[0] != want_s[0]).sum())}; '
                 f'largest relative weight difference {float(((got_s[1] / want_s[1] - 1).abs().max())):.2e} / '
                 f'{float(((got_s[2] / want_s[2] - 1).abs().max())):.2e}')
    lines += compare(fused_s, batched_s, n, 'obj_sample_weights', 'fused, events around the Python call (one read-back)',
                     'PyTorch, events around the call (one read-back)')
    lines.append('obj_sampler with its own torch.multinomial draws on both sides:')
    fe, be = [], []
    for _ in range(4):
        fe.append(events_ms(lambda: targets.obj_sampler(N, fg, cen, gt), n // 4))
        be.append(events_ms(lambda: torch_sampler(N, fg, cen, gt), n // 4))
    lines.append(f'  {"fused":58s} {np.mean(fe) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in fe)})')
    lines.append(f'  {"PyTorch":58s} {np.mean(be) * 1e3:10.2f} us   (four windows: {", ".join(f"{x * 1e3:.1f}" for x in be)})')
    lines.append(f'  kernel launches per call: fused {launches(lambda: targets.obj_sampler(N, fg, cen, gt))}, '
                 f'PyTorch {launches(lambda: torch_sampler(N, fg, cen, gt))}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


def targets_index(fg):
    """point indices as the `gt` of a first torch_sampler call, so that its first output is the draws themselves"""
    return torch.arange(fg.numel(), device=fg.device)


if __name__ == '__main__':
    main()
