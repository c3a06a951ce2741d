"""Time epropnp_pose_errors on the device with the library's stage recorder (its two launches together), next to the plain-torch
composite of the same definitions (bracketed by events: the composite has no stage of its own).

    python tools/metrics_timing.py [--out profiles/metrics_timing.txt]

Shapes, 6-DoF, one model, every object symmetric (ADD-S, the M^2 part, for every row): B = 1024 poses x M = 8192 points;
B = 32 x M = 32768; S x B = 512 x 64 pose samples x M = 2048.  The composite transforms the model by both poses and takes
`torch.cdist(...).min` per row; its (rows, M, M) temporary is kept at 256 MB by running in chunks of rows, one after another on the
same stream.  Means over the launches after warm-up, with the engine / memory clocks bench.py's sampler reads while they run.
The composite is the yardstick; there is no pass / fail ratio, the file is the record."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import event_ms, stage_ms      # noqa: E402


def quat_rot(q):
    w, x, y, z = torch.nn.functional.normalize(q, dim=-1).unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).reshape(q.shape[:-1] + (3, 3))


def torch_composite(est, gt, pts, K, chunk_bytes=256e6):
    """rot_deg, trans, arp_2d, add, adi of (R,B,7) poses against (B,7) in plain torch, the reference's expressions batched"""
    R, B = est.shape[:2]
    M = pts.shape[0]
    Re, Rg = quat_rot(est[..., 3:]), quat_rot(gt[..., 3:]).expand(R, B, 3, 3)
    te, tg = est[..., :3], gt[..., :3].expand(R, B, 3)
    cos = ((Re.transpose(-1, -2) @ Rg).diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2
    rot = torch.rad2deg(torch.acos(cos.clamp(-1, 1)))
    trans = (te - tg).norm(dim=-1)
    pe = pts @ Re.transpose(-1, -2) + te[..., None, :]          # (R,B,M,3)
    pg = pts @ Rg.transpose(-1, -2) + tg[..., None, :]
    add = (pe - pg).norm(dim=-1).mean(-1)
    ue, ug = pe @ K.T, pg @ K.T
    arp = (ue[..., :2] / ue[..., 2:] - ug[..., :2] / ug[..., 2:]).norm(dim=-1).mean(-1)
    pe, pg = pe.reshape(R * B, M, 3), pg.reshape(R * B, M, 3)
    step = max(1, int(chunk_bytes // (4 * M * M)))
    adi = torch.cat([torch.cdist(pg[i:i + step], pe[i:i + step]).min(dim=-1).values.mean(-1) for i in range(0, R * B, step)])
    return rot, trans, arp, add, adi.reshape(R, B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import metrics
    dev = torch.device('cuda:0')
    n, n_torch, warm = a.launches, 3, 3
    lines = [f'pose_errors timing: mean of {n} launches after {warm} warm-up launches (torch composite: {n_torch} after 1); '
             f'{torch.cuda.get_device_name(0)}; 6-DoF, one model, every object symmetric; QUERY_TILE {metrics.QUERY_TILE}, '
             f'CAND_TILE {metrics.CAND_TILE}']
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], device=dev)
    for S, B, M in ((1, 1024, 8192), (1, 32, 32768), (512, 64, 2048)):
        g = torch.Generator().manual_seed(S + B + M)
        pts = (torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1) * torch.tensor([0.05, 0.08, 0.03])).to(dev)
        gt = torch.cat((torch.tensor([0.05, -0.03, 1.0]) + 0.1 * torch.randn(B, 3, generator=g),
                        torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)), -1)
        est = gt.expand(S, B, 7) + torch.cat((0.01 * torch.randn(S, B, 3, generator=g), 0.05 * torch.randn(S, B, 4, generator=g)), -1)
        est, gt = est.contiguous().to(dev), gt.to(dev)
        sym = torch.ones(B, dtype=torch.bool, device=dev)
        step = max(1, int(256e6 // (4 * M * M)))
        lines.append(f'rows={S}x{B} M={M}: {S * B * M * M / 1e9:.2f} G pairs; torch composite in chunks of {step} rows')
        kern = lambda: metrics.pose_errors(est, gt, pts, cam_mats=K, symmetric=sym)
        comp = lambda: torch_composite(est, gt, pts, K)
        for _ in range(warm):
            kern()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            ms = stage_ms(kern, 'pose_errors', n)
        lines.append(f'  {"pose_errors (stage recorder)":42s} {ms * 1e3:10.2f} us   {S * B * M * M / ms / 1e9:8.2f} T pairs/s   clocks {json.dumps(clk.summary())}')
        comp()
        torch.cuda.synchronize()
        with ClockSampler(0) as clk:
            ms_t = event_ms(comp, n_torch)
        lines.append(f'  {"torch composite, chunked (events)":42s} {ms_t * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
        got, want = kern(), comp()
        d_adi = ((got.adi - want[4]).abs() / (want[4] + 8e-5)).max().item()
        d_add = ((got.add - want[3]).abs() / (want[3] + 8e-5)).max().item()
        lines.append(f'  largest difference from the (fp32) composite: adi {d_adi:.2e}, add {d_add:.2e} of value + 1e-3 radius   '
                     f'kernel / composite = {ms / ms_t:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
