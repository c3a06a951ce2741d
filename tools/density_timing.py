"""Time epropnp_orient_density and epropnp_bev_density on the device next to the PyTorch composite of the same arithmetic.

    python tools/density_timing.py [--out profiles/density_timing.txt]

The sphere at (S,B,size) = (512,1,512) and (512,32,512), window (5,5), the reference's other defaults; the BEV grid at 6 images x 100
objects x 512 samples on 900 x 1600 at scale 10, window 3.  The library calls run on buffers allocated once and are read off the
library's stage recorder (both launches of an entry together).  The yardstick is `torch_orient` / `torch_bev` below: the
reference's arithmetic (draw_orient_density.py:15-51; image_bev_vis.py:79-95 with the host's np.bincount / cv2.blur replaced by
scatter_add_ / avg_pool2d ON THE DEVICE, i.e. a better route than the reference's own) in plain torch on the same device, timed
with events around the launches; its device-to-host copies (the reference makes two of full canvases for the sphere, and moves
every sample to the host for the grid) are timed separately with a wall clock, as is the one copy of the finished image the
drop-in makes.  Means after warm-up, with the engine / memory clocks bench.py's sampler reads while they run.  There is no
pass / fail ratio, the file is the record."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'epro-pnp_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from posterior_timing import event_ms, stage_ms      # noqa: E402


def torch_orient(pose_samples, logw, size=512, saturation=0.5, sphere_opacity=0.6, sample_kernel=(5, 5), intensity_scale=50):
    """draw_orient_density.py:15-51 in plain torch, up to (not including) the two device-to-host copies: -> (draw, front_layer)"""
    dev = pose_samples.device
    bs = pose_samples.shape[1]
    w = logw.softmax(dim=0)[..., None].expand(-1, -1, 3)
    q = pose_samples[..., 3:]
    qw, x, y, z = q.unbind(-1)
    dd = qw * qw - (x * x + y * y + z * z)
    ax = torch.stack((2 * x * x + dd, 2 * (x * y - qw * z), 2 * (x * z + qw * y)), -1)
    ay = torch.stack((2 * (x * y + qw * z), 2 * y * y + dd, 2 * (y * z - qw * x)), -1)
    az = torch.stack((2 * (x * z - qw * y), 2 * (y * z + qw * x), 2 * z * z + dd), -1)
    px, py = (ax * (0.4 * size) + (size / 2 - 0.5)).round().long(), (ay * (0.4 * size) + (size / 2 - 0.5)).round().long()
    inds = py * size + px
    vis = az <= 0
    canvas = torch.zeros((bs, size, size, 3), device=dev)
    front = canvas.reshape(bs, -1, 3).transpose(0, 1).clone().scatter_add_(0, inds, w * vis).transpose(0, 1).reshape(bs, size, size, 3)
    back = canvas.reshape(bs, -1, 3).transpose(0, 1).clone().scatter_add_(0, inds, w * (~vis)).transpose(0, 1).reshape(bs, size, size, 3)
    pad = (sample_kernel[0] // 2, sample_kernel[1] // 2)
    front = F.avg_pool2d(front.permute(0, 3, 1, 2), sample_kernel, 1, pad).permute(0, 2, 3, 1)
    back = F.avg_pool2d(back.permute(0, 3, 1, 2), sample_kernel, 1, pad).permute(0, 2, 3, 1)
    front = front * (intensity_scale * sample_kernel[0] * sample_kernel[1])
    back = back * (intensity_scale * sample_kernel[0] * sample_kernel[1])
    colors = torch.eye(3, device=dev) * saturation + (1 - saturation) / 2
    front_layer = torch.pow(colors, front[..., None]).prod(-2)
    back_layer = torch.pow(colors, back[..., None]).prod(-2)
    wh = torch.arange(size, device=dev, dtype=torch.float32).sub(size / 2 - 0.5).div(0.4 * size)
    s = wh.square()
    circle = 1 - ((s + s[:, None]) <= 1.0).float() * 0.5
    draw = back_layer * sphere_opacity + circle[..., None] * (1 - sphere_opacity)
    return draw, front_layer


def torch_bev(pose_samples, logw, score, groups, G, H, W, scale, origin, window=3):
    """show_bev's density block with the histogram and the blur kept on the device: -> (G,H,W) box-summed density"""
    w = logw.softmax(dim=0) * score
    px = (pose_samples[..., 2] * scale).round().long() + origin[0]
    py = (pose_samples[..., 0] * scale).round().long() + origin[1]
    ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    flat = (groups[None, :].long() * H + py) * W + px
    dens = torch.zeros(G * H * W, device=w.device).scatter_add_(0, flat[ok], w[ok]).reshape(G, 1, H, W)
    return F.avg_pool2d(dens, window, 1, window // 2).mul(window * window)[:, 0]


def wall_us(fn, n=3):
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import ClockSampler
    from epropnp import _hip
    dev = torch.device('cuda:0')
    n, warm = a.launches, 3
    lines = [f'orient_density / bev_density timing: mean of {n} launches after {warm} warm-up launches; {torch.cuda.get_device_name(0)}']
    for S, B, size in ((512, 1, 512), (512, 32, 512)):
        g = torch.Generator().manual_seed(S + B)
        q = torch.randn(1, B, 4, generator=g) + 0.3 * torch.randn(S, B, 4, generator=g)
        pose = torch.cat((torch.randn(S, B, 3, generator=g), q / q.norm(dim=-1, keepdim=True)), -1).contiguous().to(dev)
        logw = (2.0 * torch.randn(S, B, generator=g)).to(dev)
        nbytes = int(_hip.lib().epropnp_orient_density_scratch_bytes(S, B))
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        image = torch.empty((B, size, size, 3), device=dev)
        call = lambda: _hip.call('epropnp_orient_density', _hip.ptr(pose), _hip.ptr(logw), None, S, B, 6, size, 5, 5, 0.5, 0.6, 50.0,
                                 _hip.ptr(scratch), nbytes, _hip.ptr(image), None, None, None, _hip.stream_of(pose))
        comp = lambda: torch_orient(pose, logw, size)
        for _ in range(warm):
            call()
            comp()
        torch.cuda.synchronize()
        draw, front_layer = comp()
        diff = float((draw * front_layer - image).abs().max())
        lines.append(f'sphere S={S} B={B} size={size}: image {image.numel() * 4 / 1e6:.1f} MB; largest difference from the composite {diff:.2e} '
                     f'(a sample on a rounding fence moves a pixel)')
        with ClockSampler(0) as clk:
            ms = stage_ms(call, 'orient_density', n)
        lines.append(f'  {"epropnp_orient_density (stage recorder)":52s} {ms * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
        with ClockSampler(0) as clk:
            ms_c = event_ms(comp, n)
        lines.append(f'  {"torch composite, device work (events)":52s} {ms_c * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
        lines.append(f'  {"  its two device-to-host copies (wall clock)":52s} {wall_us(lambda: (draw.cpu(), front_layer.cpu())):10.2f} us')
        lines.append(f'  {"  the drop-in, one copy of the image (wall clock)":52s} {wall_us(lambda: image.cpu()):10.2f} us')
    G, per, S, H, W, scale = 6, 100, 512, 900, 1600, 10.0
    B = G * per
    g = torch.Generator().manual_seed(7)
    centre = torch.stack((20.0 * torch.randn(B, generator=g), torch.zeros(B), 5.0 + 70.0 * torch.rand(B, generator=g)), -1)
    pose = torch.zeros(S, B, 4)
    pose[..., :3] = centre[None] + torch.tensor([0.3, 0.1, 1.0]) * torch.randn(S, B, 3, generator=g)
    pose, logw = pose.contiguous().to(dev), (2.0 * torch.randn(S, B, generator=g)).to(dev)
    score = torch.rand(B, generator=g).to(dev)
    groups = torch.arange(B, device=dev) // per
    offsets = (torch.arange(G + 1, device=dev) * per).to(torch.int32)
    origin = (int(W / 16), int(H / 2))
    nbytes = int(_hip.lib().epropnp_bev_density_scratch_bytes(S, B))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    density = torch.empty((G, H, W), device=dev)
    call = lambda: _hip.call('epropnp_bev_density', _hip.ptr(pose), _hip.ptr(logw), _hip.ptr(score), _hip.ptr(offsets), S, B, G, 4, H, W,
                             scale, origin[0], origin[1], 3, _hip.ptr(scratch), nbytes, _hip.ptr(density), None, _hip.stream_of(pose))
    comp = lambda: torch_bev(pose, logw, score, groups, G, H, W, scale, origin)
    for _ in range(warm):
        call()
        comp()
    torch.cuda.synchronize()
    want = comp()
    lines.append(f'bev G={G} objects={B} S={S} grid {H}x{W} scale {scale}: density {density.numel() * 4 / 1e6:.1f} MB; mass on the grid '
                 f'{float(density.sum()) / 9:.2f} (composite {float(want.sum()) / 9:.2f}); largest difference {float((want - density).abs().max()):.2e}')
    with ClockSampler(0) as clk:
        ms = stage_ms(call, 'bev_density', n)
    lines.append(f'  {"epropnp_bev_density (stage recorder)":52s} {ms * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
    with ClockSampler(0) as clk:
        ms_c = event_ms(comp, n)
    lines.append(f'  {"torch composite on the device (events)":52s} {ms_c * 1e3:10.2f} us   clocks {json.dumps(clk.summary())}')
    lines.append(f'  {"  the reference instead copies every sample to the host first (wall clock)":52s} '
                 f'{wall_us(lambda: (pose.cpu(), logw.cpu())):10.2f} us')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
