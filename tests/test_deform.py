"""epropnp.deform.sample_attend / DeformableAttentionSampler (epropnp_deform_sample_forward / _backward) against an fp64 oracle written here.

The oracle states the definition with an explicit four-corner gather (no grid_sample): px = x / stride - 0.5; k, v, x2d bilinear with
the coordinate clamped to the map; the mask bilinear with zeros outside; a = q . k / sqrt(D); attn = sum_p v_p softmax(a)_p mask_p.
Next to it `composite32` restates the reference's own formulation (four 5-D grid_sample calls with the image index as a third grid
axis, softmax, two matmuls) in fp32 on the CPU; its deviation from the fp64 oracle ON THE SAME CASE is the cap: a kernel less accurate
than the reference is a defect, not a tolerance.  Every comparison of an output the kernels form without atomics -- the five forward
outputs, dquery, dlocation -- asserts   error <= BAR   and   error <= the case's cap.  The kernels compute in fp64 between their loads
and one rounding per output, and a correctly rounded value is at least as close to the exact one as any fp32 evaluation: the cap holds by
construction, on the smallest cases too, where both sides are down to their last bit.

Forward bars: 4 x the worst absolute error seen over every case of this file and of tests/test_deform_reference.py (which compares with
the reference's recorded fp32 outputs at the same bars and holds every worst case: the reference's own rounding), on the CPU emulation
and on the MI355X (each case prints its figures).  Against fp64 alone the worst is half an ulp of the largest value.
                  vs the recorded reference                 vs fp64 alone (emulation = MI355X)
    attn          emulation 2.831e-7,  MI355X 2.831e-7   -> bar 1.14e-6        3.172e-8    (the reference at 'config': 2.7e-6)
    v_samples     emulation 1.790e-6,  MI355X 1.790e-6   -> bar 7.16e-6        1.192e-7    (1.2e-5)
    a_samples     emulation 1.028e-6,  MI355X 1.028e-6   -> bar 4.12e-6        1.183e-7    (7.7e-6)
    mask_samples  emulation 9.835e-7,  MI355X 9.835e-7   -> bar 3.94e-6        2.980e-8    (3.8e-6)
    x2d_samples   emulation 7.629e-6,  MI355X 7.629e-6   -> bar 3.06e-5        7.629e-6    (2.7e-5; values up to 160 px)
Backward bars: errors relative to the largest |fp64 gradient| of the tensor, 4 x the worst seen over the cases, the single-cotangent and
the unwanted-gradient runs; cap = the same figure of composite32's autograd on the same case (at 'config': dquery 1.4e-6, dkey 1.2e-6,
dvalue 7.1e-7, dlocation 2.3e-6; at the small cases 6e-8 .. 3e-7):
    dquery        emulation 4.457e-8,  MI355X 4.457e-8   -> bar 1.79e-7
    dkey          emulation 3.371e-7,  MI355X 3.585e-7   -> bar 1.44e-6
    dvalue        emulation 2.553e-7,  MI355X 2.553e-7   -> bar 1.03e-6
    dlocation     emulation 5.263e-8,  MI355X 5.263e-8   -> bar 2.11e-7
dkey / dvalue are sums of fp32 atomic adds in arrival order, as the reference's grid_sample backward is an fp32 sum in its own order.
Which of two such orders lands closer to fp64 on a small case is chance (at 'limits' the kernel's dkey was 3.4e-7 .. 3.6e-7 against the
reference's 2.7e-7, at 'p16' its dvalue 1.2e-7 against 1.0e-7 on one run and below it on another; at 'config' it is 7 x closer), so for
these two the per-case cap is the rounding bound that holds for an fp32 sum in ANY order, checked per element:
|error| <= n 2^-24 sum |term|, n = the (sample, corner) pairs that name the pixel, sum |term| from the fp64 graph; the reference's figure
is printed next to it.  The bar still applies.
The backward inputs are fenced: no map coordinate within 1e-3 px of an integer (the clamp borders 0 and n - 1 and the mask's borders
-1 and n are integers), where the location gradient is discontinuous.  A whole draw never passes at the larger shapes (20480
coordinates, 0.2 % each), so the seeds are tried upwards from the case's first seed PER COORDINATE: every coordinate keeps its value
from the first seed that puts it outside the fence.
Determinism: two launches give the same bits for the five forward outputs, dquery and dlocation.  dkey / dvalue are exempt: they are
sums of float atomics, whose last bits depend on the arrival order.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

NAMES = ('attn', 'v_samples', 'a_samples', 'mask_samples', 'x2d_samples')
GRADS = ('dquery', 'dkey', 'dvalue', 'dlocation')
FWD_BAR = {'attn': 1.14e-6, 'v_samples': 7.16e-6, 'a_samples': 4.12e-6, 'mask_samples': 3.94e-6, 'x2d_samples': 3.06e-5}
BWD_BAR = {'dquery': 1.79e-7, 'dkey': 1.44e-6, 'dvalue': 1.03e-6, 'dlocation': 2.11e-7}
_worst = {}

# (B, NI, H, P, D, h, w), map stride, spread of the sampling offsets (in units of the object stride), first seed
CASES = {
    'odd': ((7, 3, 2, 5, 4, 6, 9), 4, 1.0, 100),
    'tiny_map': ((5, 1, 8, 32, 32, 5, 7), 4, 6.0, 200),
    'config': ((40, 6, 8, 32, 32, 23, 40), 4, 4.0, 300),
    'p16': ((3, 2, 8, 16, 32, 8, 8), 8, 1.0, 400),
    'limits': ((2, 1, 1, 64, 64, 4, 4), 4, 0.5, 500),
    'one_pixel': ((3, 2, 2, 7, 8, 1, 1), 4, 0.1, 600),
}


def _deform():
    from epropnp import deform
    return deform


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the fp64 oracle and the reference's fp32 formulation ---------------------------------------------------------------------------
def oracle(query, key, value, dense_x2d, dense_mask, loc, img, stride, taps=None):
    """the definition, differentiable, in the dtype of its inputs; NaN coordinates count as 0 for the clamped maps.  `taps`: a dict
    that receives the k and v samples (B,H,P,D) as nodes of the graph"""
    B, H, _, D = query.shape
    NI, E, h, w = key.shape
    img = img.clamp(0, NI - 1)
    px, py = loc[..., 0] / stride - 0.5, loc[..., 1] / stride - 0.5                 # (B,H,P)
    cx, cy = torch.nan_to_num(px, nan=0.0).clamp(0, w - 1), torch.nan_to_num(py, nan=0.0).clamp(0, h - 1)
    x0, y0 = cx.detach().floor().long().clamp(0, w - 1), cy.detach().floor().long().clamp(0, h - 1)
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    fx, fy = (cx - x0)[..., None], (cy - y0)[..., None]
    bi, hi = img[:, None, None], torch.arange(H)[None, :, None]

    def border(m):                                                                  # (NI,H,C,h,w) -> (B,H,P,C)
        g = lambda yy, xx: m[bi, hi, :, yy, xx]
        return (1 - fx) * (1 - fy) * g(y0, x0) + fx * (1 - fy) * g(y0, x1) + (1 - fx) * fy * g(y1, x0) + fx * fy * g(y1, x1)

    k = border(key.reshape(NI, H, D, h, w))
    v = border(value.reshape(NI, H, D, h, w))
    x2d = border(dense_x2d[:, None].expand(NI, H, 2, h, w))
    if taps is not None:
        taps['k'], taps['v'] = k, v
    inside = (px > -1) & (px < w) & (py > -1) & (py < h)
    mx, my = torch.where(inside, px, torch.zeros_like(px)), torch.where(inside, py, torch.zeros_like(py))
    mx0, my0 = mx.detach().floor().long(), my.detach().floor().long()
    gx, gy = mx - mx0, my - my0

    def zeros(yy, xx):
        ok = inside & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        val = dense_mask[bi, 0, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
        return torch.where(ok, val, torch.zeros_like(val))
    mask = ((1 - gx) * (1 - gy) * zeros(my0, mx0) + gx * (1 - gy) * zeros(my0, mx0 + 1)
            + (1 - gx) * gy * zeros(my0 + 1, mx0) + gx * gy * zeros(my0 + 1, mx0 + 1))
    a = (query * k).sum(-1) / math.sqrt(D)                                          # (B,H,1,D) * (B,H,P,D)
    wgt = a.softmax(-1) * mask
    attn = (v * wgt[..., None]).sum(2).reshape(B, E)
    return attn, v.transpose(2, 3), a[:, :, None], mask[:, :, None], x2d.transpose(2, 3)


def composite32(query, key, value, dense_x2d, dense_mask, loc, img, stride):
    """the reference's formulation (deformable_attention_sampler.py:84-137), restated: the yardstick of the caps"""
    B, H, _, D = query.shape
    NI, E, h, w = key.shape
    P = loc.shape[2]
    size = loc.new_tensor([w * stride, h * stride])
    grid = (loc * (2 / size) - 1).transpose(0, 1).reshape(H, B, P, 1, 2)
    z = (img.to(loc.dtype) + 0.5) * (2 / NI) - 1.0
    grid = torch.cat((grid, z[None, :, None, None, None].expand(H, -1, P, 1, 1)), -1)
    heads = lambda m: m.reshape(NI, H, D, h, w).permute(1, 2, 0, 3, 4)
    shared = lambda m: m.transpose(0, 1)[None].expand(H, -1, -1, -1, -1)
    gs = lambda m, pad: F.grid_sample(m, grid, mode='bilinear', padding_mode=pad, align_corners=False).squeeze(-1).permute(2, 0, 1, 3)
    k, v = gs(heads(key), 'border'), gs(heads(value), 'border')
    x2d, mask = gs(shared(dense_x2d), 'border'), gs(shared(dense_mask), 'zeros')
    a = query @ k / np.sqrt(D)
    attn = (v @ (a.softmax(-1) * mask).reshape(B, H, P, 1)).reshape(B, E)
    return attn, v, a, mask, x2d


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _draw(shape, stride, spread, seed):
    B, NI, H, P, D, h, w = shape
    g = torch.Generator().manual_seed(seed)
    t = {'query': torch.randn(B, H, 1, D, generator=g), 'key': torch.randn(NI, H * D, h, w, generator=g),
         'value': torch.randn(NI, H * D, h, w, generator=g)}
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    grid = (torch.stack((xx, yy)) + 0.5) * stride                                  # the pixel centres in image coordinates
    t['dense_x2d'] = (grid[None] + 0.3 * stride * torch.randn(NI, 2, h, w, generator=g)).contiguous()
    t['dense_mask'] = (torch.rand(NI, 1, h, w, generator=g) > 0.3).float()
    t['img'] = torch.randint(0, NI, (B,), generator=g)
    centre = torch.rand(B, 2, generator=g) * torch.tensor([w * stride, h * stride], dtype=torch.float32)
    obj_stride = torch.tensor([8.0, 16.0, 32.0])[torch.randint(0, 3, (B,), generator=g)]
    t['loc'] = centre[:, None, None] + spread * torch.randn(B, H, P, 2, generator=g) * obj_stride[:, None, None, None]
    return t


def _coords(loc, stride):
    return loc.double() / stride - 0.5


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """inputs with some locations exactly on pixel centres, on the clamp borders and on the mask's borders; fp64 outputs; caps"""
    shape, stride, spread, seed = CASES[name]
    B, NI, H, P, D, h, w = shape
    t = _draw(shape, stride, spread, seed)
    flat = t['loc'].view(-1, 2)
    special = [((0 + 0.5) * stride, (h - 1 + 0.5) * stride), ((w - 1 + 0.5) * stride, 0.5 * stride), (0.5 * stride, 0.5 * stride),
               (-0.5 * stride, (h + 0.5) * stride), ((w + 0.5) * stride, -0.5 * stride), ((w // 2 + 0.5) * stride, (h // 2 + 0.5) * stride)]
    for i, xy in enumerate(special):
        flat[(i * 7) % flat.shape[0]] = torch.tensor(xy)
    return _finish(t, stride)


def _finish(t, stride):
    args = ('query', 'key', 'value', 'dense_x2d', 'dense_mask', 'loc')
    with torch.no_grad():
        want = oracle(*(t[k].double() for k in args), t['img'], stride)
        ref = composite32(*(t[k] for k in args), t['img'], stride)
    cap = {n: float((r.double() - o).abs().max()) for n, r, o in zip(NAMES, ref, want)}
    return t, stride, want, cap


def _fence_ok(loc, stride):
    c = _coords(loc, stride)
    return (c - c.round()).abs() >= 1e-3


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """fenced inputs, random cotangents, fp64 gradients (all five cotangents), the composite's fp32 gradients' deviation"""
    shape, stride, spread, seed = CASES[name]
    t = _draw(shape, stride, spread, seed)
    ok = _fence_ok(t['loc'], stride)
    tries = 0
    while not ok.all():                                        # seeds upwards, per coordinate (docstring)
        tries += 1
        assert tries < 50
        again = _draw(shape, stride, spread, seed + tries)['loc']
        t['loc'] = torch.where(ok, t['loc'], again)
        ok = _fence_ok(t['loc'], stride)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        outs = oracle(*(t[k].double() for k in ('query', 'key', 'value', 'dense_x2d', 'dense_mask', 'loc')), t['img'], stride)
    cot = tuple(torch.randn(o.shape, generator=g) for o in outs)
    return t, stride, cot


def _autograd(fn, t, stride, cot, dtype, which=range(5)):
    leaves = [t[k].clone().to(dtype).requires_grad_(True) for k in ('query', 'key', 'value')]
    loc = t['loc'].clone().to(dtype).requires_grad_(True)
    outs = fn(*leaves, t['dense_x2d'].to(dtype), t['dense_mask'].to(dtype), loc, t['img'], stride)
    total = sum((outs[i] * cot[i].to(dtype)).sum() for i in which)
    return torch.autograd.grad(total, leaves + [loc], allow_unused=True)


def _hits(t, stride):
    """(NI,E,h,w): how many (sample, corner) pairs name the pixel, in the channels of the sample's head"""
    NI, E, h, w = t['key'].shape
    B, H, P, _ = t['loc'].shape
    c = _coords(t['loc'], stride)
    cx, cy = c[..., 0].clamp(0, w - 1), c[..., 1].clamp(0, h - 1)
    x0, y0 = cx.floor().long(), cy.floor().long()
    n = torch.zeros(NI, H, h, w, dtype=torch.float64)
    bi, hi = t['img'][:, None, None].expand(B, H, P), torch.arange(H)[None, :, None].expand(B, H, P)
    for yy in (y0, (y0 + 1).clamp(max=h - 1)):
        for xx in (x0, (x0 + 1).clamp(max=w - 1)):
            n.index_put_((bi, hi, yy, xx), torch.ones(B, H, P, dtype=torch.float64), accumulate=True)
    return n[:, :, None].expand(NI, H, E // H, h, w).reshape(NI, E, h, w)


@functools.lru_cache(maxsize=None)
def backward_truth(name):
    """fp64 gradients; their scales; the caps (composite32's autograd on the same case); for dkey / dvalue the rounding bound of an
    fp32 sum in ANY order: n 2^-24 sum |term| per element, n = the number of (sample, corner) pairs that name the pixel"""
    t, stride, cot = backward_case(name)
    leaves = [t[k].double().requires_grad_(True) for k in ('query', 'key', 'value', 'loc')]
    taps = {}
    outs = oracle(leaves[0], leaves[1], leaves[2], t['dense_x2d'].double(), t['dense_mask'].double(), leaves[3], t['img'], stride, taps)
    total = sum((o * c.double()).sum() for o, c in zip(outs, cot))
    want = torch.autograd.grad(total, leaves, retain_graph=True)
    dk, dv = torch.autograd.grad(total, [taps['k'], taps['v']], retain_graph=True)
    abs_k = torch.autograd.grad((taps['k'] * dk.abs()).sum(), leaves[1], retain_graph=True)[0]      # sum w_c |dk|: the weights are >= 0
    abs_v = torch.autograd.grad((taps['v'] * dv.abs()).sum(), leaves[2])[0]
    n = _hits(t, stride)
    bound = {'dkey': 1.01 * n * 2.0 ** -24 * abs_k, 'dvalue': 1.01 * n * 2.0 ** -24 * abs_v}
    ref = _autograd(composite32, t, stride, cot, torch.float32)
    scale = [float(w.abs().max()) or 1.0 for w in want]
    cap = {n_: float((r.double() - w).abs().max()) / s for n_, r, w, s in zip(GRADS, ref, want, scale)}
    return want, scale, cap, bound


def _layout(t, layout, dev):
    """a fresh tensor on `dev` (the cached cases are shared between the tests and stay as they are)"""
    t = t.clone().to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else t


def _run(t, stride, dev, layout, grad=False):
    leaves = [t['query'].clone().to(dev), _layout(t['key'], layout, dev), _layout(t['value'], layout, dev), t['loc'].clone().to(dev)]
    if grad is True:
        grad = (True,) * 4
    if grad:
        leaves = [x.requires_grad_(g) for x, g in zip(leaves, grad)]
    outs = _deform().sample_attend(leaves[0], leaves[1], leaves[2], t['dense_x2d'].to(dev), t['dense_mask'].to(dev), leaves[3],
                                   t['img'].to(dev), stride)
    return leaves, outs


def _check(kind, what, name, got, want, bar, cap, scale=1.0, bound=None):
    diff = (got.double().cpu() - want).abs()
    err = float(diff.max()) / scale
    _worst[(kind, name)] = max(_worst.get((kind, name), 0.0), err)
    print(f'{what}: {name} error {err:.3e}  the reference on this case {cap:.3e}  bar {bar:.3e}  worst so far {_worst[(kind, name)]:.3e}')
    assert err <= bar, f'{what}: {name} error {err:.3e} > bar {bar:.3e}'
    if bound is None:
        assert err <= cap, f'{what}: {name} error {err:.3e} > the reference\'s own {cap:.3e}'
    else:
        assert (diff <= bound).all(), f'{what}: {name} is beyond the rounding bound of an fp32 sum by {float((diff - bound).max()):.3e}'


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('name', list(CASES))
def test_forward_against_the_fp64_oracle(backend, name, layout):
    t, stride, want, cap = forward_case(name)
    B, NI, H, P, D, h, w = CASES[name][0]
    _, outs = _run(t, stride, backend, layout)
    shapes = ((B, H * D), (B, H, D, P), (B, H, 1, P), (B, H, 1, P), (B, H, 2, P))
    c = _coords(t['loc'], stride)
    inside = ((c[..., 0] >= 0) & (c[..., 0] <= w - 1) & (c[..., 1] >= 0) & (c[..., 1] <= h - 1)).float().mean()
    print(f'{name} {layout}: {100 * float(inside):.1f} % of the samples inside the map')
    if name == 'odd':
        assert (c[..., 0] < 0).any() and (c[..., 0] > w - 1).any() and (c[..., 1] < 0).any() and (c[..., 1] > h - 1).any()
    for n, got, o, shape in zip(NAMES, outs, want, shapes):
        assert tuple(got.shape) == shape, (n, tuple(got.shape))
        _check('fwd', f'{name} {layout}', n, got, o, FWD_BAR[n], cap[n])


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _touched(t, stride):
    """(NI,E,h,w) bool: the pixels some sample's four (clamped) corners name, in the channels of the sample's head"""
    NI, E, h, w = t['key'].shape
    B, H, P, _ = t['loc'].shape
    D = E // H
    c = _coords(t['loc'], stride)
    cx, cy = c[..., 0].clamp(0, w - 1), c[..., 1].clamp(0, h - 1)
    x0, y0 = cx.floor().long(), cy.floor().long()
    hit = torch.zeros(NI, H, h, w, dtype=torch.bool)
    bi, hi = t['img'][:, None, None].expand(B, H, P), torch.arange(H)[None, :, None].expand(B, H, P)
    for yy in (y0, (y0 + 1).clamp(max=h - 1)):
        for xx in (x0, (x0 + 1).clamp(max=w - 1)):
            hit[bi, hi, yy, xx] = True
    return hit[:, :, None].expand(NI, H, D, h, w).reshape(NI, E, h, w)


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('name', list(CASES))
def test_backward_against_fp64_autograd(backend, name, layout):
    t, stride, cot = backward_case(name)
    want, scale, cap, bound = backward_truth(name)
    leaves, outs = _run(t, stride, backend, layout, grad=True)
    total = sum((o * c.to(backend)).sum() for o, c in zip(outs, cot))
    got = torch.autograd.grad(total, leaves)
    for n, g_, w_, s in zip(GRADS, got, want, scale):
        _check('bwd', f'{name} {layout}', n, g_, w_, BWD_BAR[n], cap[n], s, bound.get(n))
    untouched = ~_touched(t, stride)
    assert (got[1].cpu()[untouched] == 0).all() and (got[2].cpu()[untouched] == 0).all(), 'a pixel no sample touches has a gradient'
    fmt = torch.channels_last if layout == 'channels_last' else torch.contiguous_format
    assert got[1].is_contiguous(memory_format=fmt) and got[2].is_contiguous(memory_format=fmt)


@pytest.mark.parametrize('only', range(5))
def test_backward_with_a_single_cotangent(backend, only):
    t, stride, cot = backward_case('odd')
    want = _autograd(oracle, t, stride, cot, torch.float64, which=[only])
    leaves, outs = _run(t, stride, backend, 'channels_last', grad=True)
    got = torch.autograd.grad((outs[only] * cot[only].to(backend)).sum(), leaves, allow_unused=True)
    for n, g_, w_ in zip(GRADS, got, want):
        if w_ is None or float(w_.abs().max()) == 0.0:        # e.g. x2d_samples reaches the location only
            assert g_ is None or (g_ == 0).all(), n
            continue
        err = float((g_.double().cpu() - w_).abs().max()) / float(w_.abs().max())
        print(f'cotangent of {NAMES[only]} alone: {n} error {err:.3e}')
        assert err <= BWD_BAR[n]


@pytest.mark.parametrize('unwanted', range(4))
def test_backward_with_a_gradient_unwanted(backend, unwanted):
    t, stride, cot = backward_case('odd')
    want, scale, _, _ = backward_truth('odd')
    leaves, outs = _run(t, stride, backend, 'nchw', grad=tuple(i != unwanted for i in range(4)))
    sum((o * c.to(backend)).sum() for o, c in zip(outs, cot)).backward()
    for i, (n, x) in enumerate(zip(GRADS, leaves)):
        if i == unwanted:
            assert x.grad is None
            continue
        err = float((x.grad.double().cpu() - want[i]).abs().max()) / scale[i]
        assert err <= BWD_BAR[n], (n, err)


# ---- determinism, every element, errors ---------------------------------------------------------------------------------------------
def test_two_launches_agree_to_the_bit(backend):
    t, stride, cot = backward_case('p16')
    runs = []
    for _ in range(2):
        leaves, outs = _run(t, stride, backend, 'channels_last', grad=True)
        grads = torch.autograd.grad(sum((o * c.to(backend)).sum() for o, c in zip(outs, cot)), leaves)
        runs.append(list(outs) + [grads[0], grads[3]])           # dkey / dvalue are float-atomic sums: exempt
    for x, y in zip(*runs):
        assert torch.equal(_bits(x.detach()), _bits(y.detach()))


def test_every_output_and_gradient_element_is_written(backend, poisoned_empty):
    t, stride, cot = backward_case('odd')
    for layout in ('nchw', 'channels_last'):
        leaves, outs = _run(t, stride, backend, layout, grad=True)
        grads = torch.autograd.grad(sum((o * c.to(backend)).sum() for o, c in zip(outs, cot)), leaves)
        for x in list(outs) + list(grads):
            assert torch.isfinite(x).all()


def test_no_objects(backend):
    t, stride, _ = backward_case('odd')
    q = t['query'][:0].clone().to(backend).requires_grad_(True)
    key, loc = t['key'].clone().to(backend).requires_grad_(True), t['loc'][:0].clone().to(backend).requires_grad_(True)
    outs = _deform().sample_attend(q, key, t['value'].to(backend), t['dense_x2d'].to(backend), t['dense_mask'].to(backend), loc,
                                   t['img'][:0].to(backend), stride)
    assert [tuple(o.shape) for o in outs] == [(0, 8), (0, 2, 4, 5), (0, 2, 1, 5), (0, 2, 1, 5), (0, 2, 2, 5)]
    sum(o.sum() for o in outs).backward()
    assert q.grad.shape == q.shape and loc.grad.shape == loc.shape and (key.grad == 0).all()


def test_limits_dtype_and_device_raise(backend):
    f = _deform().sample_attend
    mk = lambda B=2, NI=1, H=2, P=3, D=4, h=3, w=3, dt=torch.float32: [
        torch.zeros(B, H, 1, D, dtype=dt, device=backend), torch.zeros(NI, H * D, h, w, dtype=dt, device=backend),
        torch.zeros(NI, H * D, h, w, dtype=dt, device=backend), torch.zeros(NI, 2, h, w, dtype=dt, device=backend),
        torch.zeros(NI, 1, h, w, dtype=dt, device=backend), torch.zeros(B, H, P, 2, dtype=dt, device=backend),
        torch.zeros(B, dtype=torch.int64, device=backend), 4]
    f(*mk())
    f(*mk(P=64, D=64))
    for bad in (dict(P=65), dict(D=65)):
        with pytest.raises(ValueError):
            f(*mk(**bad))
    with pytest.raises(ValueError):
        f(*mk()[:7], 0)
    with pytest.raises(ValueError):
        a = mk()
        a[2] = a[2][:, :4]
        f(*a)
    with pytest.raises(RuntimeError):
        f(*mk(dt=torch.float64))
    other = 'cuda' if backend.type == 'cpu' else 'cpu'
    if other == 'cpu' or torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            a = mk()
            a[0] = a[0].to(other)
            f(*a)
    # the C entries refuse the same limits
    from epropnp import _hip
    z = torch.zeros(4096, device=backend)
    i = torch.zeros(8, dtype=torch.int64, device=backend)
    p = _hip.ptr(z)
    for P, D in ((65, 4), (0, 4), (3, 65), (3, 0)):
        rc = _hip.lib().epropnp_deform_sample_forward(p, p, p, p, p, p, _hip.ptr(i), 2, 1, 2, P, D, 3, 3, 4, 72, 9, 3, 1, p, p, p, p, p, p, None)
        assert rc == -1, (P, D, rc)
    rc = _hip.lib().epropnp_deform_sample_forward(p, p, p, p, p, p, _hip.ptr(i), 2, 1, 2, 3, 4, 3, 3, 4, 72, 10, 3, 1, p, p, p, p, p, p, None)
    assert rc == -1 and b'strides' in _hip.lib().epropnp_last_error()


def test_nonfinite_and_huge_locations_and_image_indices_out_of_range():
    """emulation only (a wrong kernel must show up on the CPU, not on a shared GPU): NaN, +-inf and 1e30 locations and image indices
    outside [0, NI): the border-mode maps are sampled at the clamped coordinate (NaN as 0), mask_samples = 0 there, the location
    gradient 0 along every such axis (the other axis of the point is an ordinary clamped or inside coordinate), everything finite, and
    the result equals the oracle's on the clamped image index"""
    import conftest
    import install as emu
    emu.install(conftest._emu_lib())
    try:
        shape, stride, spread, seed = CASES['odd']
        B, NI, H, P, D, h, w = shape
        t = _draw(shape, stride, spread, seed)
        loc = t['loc']
        nan, inf = float('nan'), float('inf')
        bad = [(nan, 5.0), (7.0, nan), (nan, nan), (inf, 3.0), (-inf, -inf), (1e30, -1e30), (3.4e38, 3.4e38), (-3.4e38, 9.0)]
        for i, xy in enumerate(bad):
            loc[i % B, i % H, i % P] = torch.tensor(xy)
        t['img'] = torch.tensor([-5, 0, 1, 2, 3, 2 ** 40, -2 ** 40])
        leaves, outs = _run(t, stride, torch.device('cpu'), 'channels_last', grad=True)
        cot = [torch.ones_like(o) for o in outs]
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cot)), leaves)
        for x in list(outs) + list(grads):
            assert torch.isfinite(x).all()
        with torch.no_grad():
            want = oracle(*(t[k].double() for k in ('query', 'key', 'value', 'dense_x2d', 'dense_mask', 'loc')), t['img'], stride)
        for n, got, o in zip(NAMES, outs, want):
            assert float((got.detach().double() - o).abs().max()) <= FWD_BAR[n], n
        for i, xy in enumerate(bad):
            b, j, p = i % B, i % H, i % P
            assert outs[3][b, j, 0, p] == 0
            for axis, c in enumerate(xy):
                if not math.isfinite(c) or abs(c) >= 1e29:
                    assert grads[3][b, j, p, axis] == 0, (xy, grads[3][b, j, p])
        im = int(t['img'].clamp(0, NI - 1)[2])
        assert torch.equal(outs[4][2, 0, :, 2], t['dense_x2d'][im, :, 0, 0])          # (NaN, NaN) of object 2: pixel (0, 0)
    finally:
        emu.uninstall()


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def _module_inputs(dev, seed=7, B=6, NI=2, H=4, D=8, h=7, w=9):
    g = torch.Generator().manual_seed(seed)
    E = H * D
    t = _draw((B, NI, H, 1, D, h, w), 4, 1.0, seed)
    return dict(query=t['query'].to(dev), obj_emb=torch.randn(B, E, generator=g).to(dev), key=t['key'].to(dev), value=t['value'].to(dev),
                img_dense_x2d=t['dense_x2d'].to(dev), img_dense_x2d_mask=t['dense_mask'].to(dev),
                obj_xy_point=(torch.rand(B, 2, generator=g) * torch.tensor([w * 4.0, h * 4.0])).to(dev),
                strides=torch.tensor([8.0, 16.0, 32.0])[torch.randint(0, 3, (B,), generator=g)].to(dev), obj_img_ind=t['img'].to(dev))


def test_module_against_its_own_layers_around_the_oracle(backend):
    torch.manual_seed(3)
    H, D, P = 4, 8, 5
    m = _deform().DeformableAttentionSampler(embed_dims=H * D, num_heads=H, num_points=P, stride=4,
                                             ffn_cfg=dict(type='FFN', embed_dims=H * D, feedforward_channels=64, num_fcs=2, ffn_drop=0.1,
                                                          act_cfg=dict(type='ReLU', inplace=True))).eval()
    assert sorted(m.state_dict()) == sorted(
        [f'{p}.{s}' for p in ('sampling_offsets', 'out_proj', 'layer_norms.0', 'layer_norms.1', 'ffn.layers.0.0', 'ffn.layers.1')
         for s in ('weight', 'bias')])
    bound = 2.5 * math.sqrt(6.0 / (H * D + H * P * 2))
    wgt = m.sampling_offsets.weight.detach()
    assert float(wgt.abs().max()) <= bound and float(wgt.abs().max()) > 0.9 * bound and (m.sampling_offsets.bias == 0).all()
    a = _module_inputs(torch.device('cpu'))
    m = m.to(backend)
    with torch.no_grad():
        got = m(**{k: v.to(backend) for k, v in a.items()})
        m64 = m.to('cpu').double()
        d = {k: (v.double() if v.is_floating_point() else v) for k, v in a.items()}
        offsets = m64.sampling_offsets(d['obj_emb']).reshape(6, H, P, 2)
        # the location in fp32 as the module forms it: the comparison is of the op and of the layers, not of this sum's rounding
        loc = (a['obj_xy_point'][:, None, None] + offsets.float() * a['strides'][:, None, None, None]).double()
        attn, v, s, mk, x = oracle(d['query'], d['key'], d['value'], d['img_dense_x2d'], d['img_dense_x2d_mask'], loc, d['obj_img_ind'], 4)
        out = m64.layer_norms[0](m64.out_proj(attn) + d['obj_emb'])
        out = m64.layer_norms[1](m64.ffn(out, out))
    assert [tuple(o.shape) for o in got] == [(6, H * D), (6, H, D, P), (6, H, 1, P), (6, H, 1, P), (6, H, 2, P)]
    # the offsets come out of an fp32 Linear of 32 terms (|error| ~ 1e-6 x 32 px of stride): compare at 1e-3 of each output's scale
    for n, g_, w_ in zip(NAMES, got, (out, v, s, mk, x)):
        err = float((g_.double().cpu() - w_).abs().max()) / max(1.0, float(w_.abs().max()))
        print(f'module: {n} error {err:.3e} of its scale')
        assert err <= 1e-3, (n, err)


def test_module_gradients_reach_every_input(backend):
    torch.manual_seed(4)
    H, D, P = 4, 8, 5
    m = _deform().DeformableAttentionSampler(embed_dims=H * D, num_heads=H, num_points=P, stride=4,
                                             ffn_cfg=dict(type='FFN', embed_dims=H * D, feedforward_channels=64, num_fcs=2, ffn_drop=0.0,
                                                          act_cfg=dict(type='ReLU', inplace=True))).to(backend).eval()
    a = _module_inputs(backend)
    for k in ('query', 'key', 'value', 'obj_xy_point'):
        a[k].requires_grad_(True)
    outs = m(**a)
    sum(o.square().sum() for o in outs).backward()
    for name, x in [('sampling_offsets', m.sampling_offsets.weight), ('out_proj', m.out_proj.weight)] + [(k, a[k]) for k in ('query', 'key', 'value', 'obj_xy_point')]:
        assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0, name


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_bits():
    import install as emu
    emu.uninstall()
    dev = torch.device('cuda:0')
    t, stride, cot = backward_case('p16')
    q, loc = t['query'].clone().to(dev).requires_grad_(True), t['loc'].clone().to(dev).requires_grad_(True)
    key, value = (_layout(t[k], 'channels_last', dev).requires_grad_(True) for k in ('key', 'value'))
    x2d, mask, img = t['dense_x2d'].to(dev), t['dense_mask'].to(dev), t['img'].to(dev)
    cot = [c.to(dev) for c in cot]

    def step():
        outs = _deform().sample_attend(q, key, value, x2d, mask, loc, img, stride)
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cot)), (q, key, value, loc))
        return list(outs), list(grads)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs, grads = step()
    with torch.no_grad():
        loc.copy_(backward_case('p16')[0]['loc'].to(dev) + 3.0)
    graph.replay()
    graph.replay()
    eager_outs, eager_grads = step()
    torch.cuda.synchronize()
    for x, y in zip(outs + [grads[0], grads[3]], eager_outs + [eager_grads[0], eager_grads[3]]):
        assert torch.equal(_bits(x.detach()), _bits(y.detach()))
    for x, y in zip(grads[1:3], eager_grads[1:3]):
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
