"""Time epropnp_posterior_summary on the device with the library's stage recorder, next to the plain-torch statement of the same
quantities (bracketed by events: the composite has no stage of its own) and to weight_stats at the same (S,B).

    python tools/posterior_timing.py [--launches 300] [--out profiles/posterior_summary.txt]
    python tools/posterior_timing.py --modes [--out profiles/posterior_modes_timing.txt]

--modes times epropnp_posterior_modes (stage recorder: its three launches together) at S = 512, B = 4096, 6-DoF; S = 512, B = 600,
4-DoF; S = 4096, B = 32, 6-DoF, next to the plain-torch composite of the same definition.  The composite needs (b,S,S) temporaries,
so it runs in chunks of objects that keep one such temporary at 256 MB, the chunks one after another on the same stream.

Shapes: the Det shape (S = 512, B = 600, 4-DoF) and S = 512, B = 4096, 6-DoF.  Means over `launches` launches after warm-up, with
the engine / memory clocks bench.py's sampler reads while the launches run."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_composite(ps, lw, ref):
    """The same quantities in plain torch, the way a caller of the raw outputs writes them (deform_pnp_head.py:524-536 for the
    score; epropnp.py:240-257 for the moments; eigh for the quaternion mean)."""
    w = lw.softmax(dim=0)
    t = ps[..., :3]
    mean = (w[..., None] * t).sum(0)
    dev = t - mean
    cov = (w[..., None, None] * dev.unsqueeze(-1) * dev.unsqueeze(-2)).sum(0)
    sample_dev = (ps[..., [0, 2]] - ref[:, [0, 2]]).norm(dim=-1)
    score = (((-sample_dev.log2() + 2.5) / 4).clamp(min=0, max=1) * w).sum(dim=0)
    if ps.shape[-1] == 4:
        s, c = (w * ps[..., 3].sin()).sum(0), (w * ps[..., 3].cos()).sum(0)
        return mean, cov, score, torch.atan2(s, c), (s * s + c * c).sqrt()
    q = ps[..., 3:]
    lam, vec = torch.linalg.eigh((w[..., None, None] * q.unsqueeze(-1) * q.unsqueeze(-2)).sum(0))
    return mean, cov, score, vec[..., 3], lam[:, 3]


def torch_modes(ps, lw, bw, link=3.0, max_modes=4, chunk_bytes=256e6):
    """epropnp.posterior.modes in plain torch (finite log-weights), in chunks of objects whose (b,S,S) fp32 temporaries hold
    chunk_bytes each."""
    S, B, P = ps.shape
    step = max(1, int(chunk_bytes // (4 * S * S)))
    idx = torch.arange(S, device=ps.device)
    outs = []
    for b0 in range(0, B, step):
        p, l, h = ps[:, b0:b0 + step].transpose(0, 1), lw[:, b0:b0 + step].t(), bw[b0:b0 + step]
        w = torch.exp(l - l.max(dim=1, keepdim=True).values)
        D = sum((p[:, :, None, k] - p[:, None, :, k]).square() for k in range(3)) / h[:, 0, None, None].square()
        if P == 4:
            rho = 4 * torch.sin((p[:, :, None, 3] - p[:, None, :, 3]) / 2).square()
        else:
            d2 = torch.minimum(sum((p[:, :, None, k] - p[:, None, :, k]).square() for k in range(3, 7)),
                               sum((p[:, :, None, k] + p[:, None, :, k]).square() for k in range(3, 7)))
            rho = d2 * (4 - d2)
        D = D + rho / h[:, 1, None, None].square()
        W = w.sum(1, keepdim=True)
        f = (w[:, None, :] * torch.exp(-D / 2)).sum(-1) / W
        cand = ((f[:, None, :] > f[:, :, None]) | ((f[:, None, :] == f[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))) & (D <= link * link)
        best, parent = torch.where(cand, D, torch.full_like(D, float('inf'))).min(-1)
        parent = torch.where(torch.isinf(best), idx[None, :].expand_as(parent), parent)
        labels = parent
        for _ in range(max(1, (S - 1).bit_length())):
            labels = labels.gather(1, labels)
        mass = torch.zeros_like(w).scatter_add_(1, labels, w) / W
        top = torch.topk(torch.where(labels == idx[None, :], mass, torch.full_like(mass, -1.0)), min(max_modes, S), dim=1)
        outs.append((f, parent, labels, top.values, top.indices, p.gather(1, top.indices[..., None].expand(-1, -1, P))))
    return outs


def modes_leg(a):
    from bench import ClockSampler
    from epropnp import posterior
    dev = torch.device('cuda:0')
    n, n_torch, warm = 50, 5, 5
    lines = [f'posterior_modes timing: mean of {n} launches after {warm} warm-up launches (torch composite: {n_torch} after 2); '
             f'{torch.cuda.get_device_name(0)}; bandwidth (0.25, 0.5), link 3, max_modes 4']
    for S, B, dof in ((512, 4096, 6), (512, 600, 4), (4096, 32, 6)):
        g = torch.Generator().manual_seed(S + B)
        P = 4 if dof == 4 else 7
        ps = torch.randn(S, B, P, generator=g)
        ps[..., :3] = ps[..., :3] * 0.5 + torch.tensor([2.0, 1.0, 50.0])
        if dof == 6:
            ps[..., 3:] = torch.nn.functional.normalize(ps[..., 3:], dim=-1)
        lw = torch.randn(S, B, generator=g) * 3.0
        ps, lw = ps.to(dev), lw.to(dev)
        bw = torch.tensor([0.25, 0.5], device=dev).expand(B, 2).contiguous()
        step = max(1, int(256e6 // (4 * S * S)))
        lines.append(f'S={S} B={B} dof={dof}: {S * S * B / 1e9:.2f} G pairs per pass, two passes; torch composite in chunks of {step} objects')
        kern = lambda: posterior.modes(ps, lw, bw)
        comp = lambda: torch_modes(ps, lw, bw)
        for _ in range(warm):
            kern()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            ms = stage_ms(kern, 'posterior_modes', n)
        lines.append(f'  {"posterior_modes (stage recorder)":42s} {ms * 1e3:9.2f} us   clocks {json.dumps(clk.summary())}')
        for _ in range(2):
            comp()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            ms_t = event_ms(comp, n_torch)
        lines.append(f'  {"torch composite, chunked (events)":42s} {ms_t * 1e3:9.2f} us   clocks {json.dumps(clk.summary())}')
        got, want = posterior.modes(ps, lw, bw), comp()
        same = torch.cat([w[2] for w in want], 0).t().eq(got.labels).float().mean().item()
        lines.append(f'  labels equal to the composite\'s: {same * 100:.2f} %   kernel / composite = {ms / ms_t:.3f}')
    return lines


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def stage_ms(fn, stage, n):
    from epropnp import _hip
    _hip.profile(True, reset=True)
    for _ in range(n):
        fn()
    ms, count = _hip.profile_read(stage)
    _hip.profile(False, reset=True)
    assert count == n, (stage, count)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--modes', action='store_true', help='time epropnp_posterior_modes against its torch composite instead')
    a = ap.parse_args()
    if a.modes:
        text = '\n'.join(modes_leg(a)) + '\n'
        print(text, end='')
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text)
        return
    assert a.launches >= 200
    from bench import ClockSampler
    from epropnp import functional as F
    from epropnp import posterior
    dev = torch.device('cuda:0')
    lines = [f'posterior_summary timing: mean of {a.launches} launches after {a.warmup} warm-up launches; {torch.cuda.get_device_name(0)}']
    for S, B, dof in ((512, 600, 4), (512, 4096, 6)):
        g = torch.Generator().manual_seed(S + B)
        P = 4 if dof == 4 else 7
        ps = torch.randn(S, B, P, generator=g)
        ps[..., :3] = ps[..., :3] * 0.5 + torch.tensor([2.0, 1.0, 50.0])
        if dof == 6:
            ps[..., 3:] = torch.nn.functional.normalize(ps[..., 3:], dim=-1)
        lw = torch.randn(S, B, generator=g) * 3.0
        ps, lw = ps.to(dev), lw.to(dev)
        ref = ps[0].clone()
        runs = {'posterior_summary (stage recorder)': lambda: posterior.summarize(ps, lw, ref),
                'weight_stats (stage recorder)': lambda: F.weight_stats(lw, 4),
                'posterior_resample R=64 (stage recorder)': lambda: posterior.resample(ps, lw, 64, seed=1),
                'torch composite (events)': lambda: torch_composite(ps, lw, ref)}
        stages = {'posterior_summary (stage recorder)': 'posterior_summary', 'weight_stats (stage recorder)': 'weight_stats',
                  'posterior_resample R=64 (stage recorder)': 'posterior_resample'}
        lines.append(f'S={S} B={B} dof={dof}: {S * B * (P + 1) * 4 / 1e6:.2f} MB of samples + log-weights, {S * B * 4 / 1e6:.2f} MB of log-weights')
        for name, fn in runs.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            with ClockSampler(0) as clk:
                ms = stage_ms(fn, stages[name], a.launches) if name in stages else event_ms(fn, a.launches)
            lines.append(f'  {name:42s} {ms * 1e3:9.2f} us   clocks {json.dumps(clk.summary())}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
