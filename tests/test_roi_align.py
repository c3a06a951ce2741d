"""epropnp.roi.roi_align / roi_align_wrapper / extract_rois (epropnp_roi_align_forward / _backward) against an fp64 oracle written here.

mmcv's roi_align is a native extension that is not installed where this package is built, so there is no recording of its results; the
oracle is the per-sample definition in numpy fp64.  For RoI r on image n, o = 0.5 if aligned else 0: xs = x1 scale - o, xe = x2 scale -
o, rw = xe - xs (clamped to >= 1 only when not aligned), bw = rw / pw, gw = sampling_ratio or ceil(bw); y alike; cell (i, j) is
1 / max(gh gw, 1) times the sum over iy < gh, ix < gw of the bilinear sample at y = ys + i bh + (iy + .5) bh / gh, x alike; a sample
with y < -1, y > h, x < -1 or x > w is 0, any other has its coordinates clamped to the map.  The oracle loops over the RoIs and over the
samples (iy, ix) of a cell, forms the four corner weights of every sample as a product and gathers / scatters the four corners: it does
not use the separable form the kernels use.  (The cells of one sample index are evaluated together as arrays; nothing is merged across
samples.)  With sampling_ratio > 0 a RoI of zero or negative size still has sampling_ratio^2 samples per cell, as in the reference;
on the adaptive grid it has none and gives zeros.

Fences, asserted from the oracle for every case before anything is compared: no sample coordinate within 1e-3 of -1, h or w (the rule
"y < -1 -> 0" is a discontinuity) and no rh / ph or rw / pw within 1e-4 of an integer without being that integer (the ceil is one).

Forward bar: |out - out64| in units of 2^-24 max|map| of the case.  The kernels accumulate in fp64 and round each output once, so the
error is the rounding of the output: at most half an ulp, which is at most 2^-24 |out| <= one unit.  Worst over every case of this file
(each case prints its figure):   emulation 0.6164,  MI355X 0.6164   -> FWD_BAR = 4 x that = 2.466.  The cap the bar may never exceed is
(gh gw + 3) 2^-24 max|map| -- a sequentially accumulated fp32 mean of gh gw bilinear samples -- which is 4 units on the smallest grid
(1 x 1); it is asserted per case with the smallest grid of the case.
Backward bar, per element of the gradient map and for a cotangent on multiples of 1/8: |dmap - dmap64| <= (k + 2) 2^-24 A, k the number
of (sample, corner) terms that reach the element and A their absolute sum; the oracle gets both from its own backward on |cot|.  An
element no RoI reaches has k = 0 and must be exactly 0.0.  Worst ratio to that tolerance:   emulation 0.3259,  MI355X 0.3259   (the one
rounding of the gradient, where k is 1: at most 1 / 3).
"""
import functools
import math

import numpy as np
import pytest
import torch

FWD_BAR = 2.466                                 # units of 2^-24 max|map|: 4 x the worst seen (docstring)
UNIT = 2.0 ** -24
FENCE, FENCE_CEIL = 1e-3, 1e-4
_worst = {}

# [image id, x1, y1, x2, y2], every coordinate a multiple of 1/8: inside, out past -1 at the top-left, out past h, w at the bottom-right,
# zero size, negative size, a size that is a multiple of the cell counts; then two more copies of the first (the backward sums over RoIs)
BOXES = [(0, 3.125, 2.5, 30.75, 22.375), (1, -30.5, -21.25, 20.125, 14.625), (1, 18.25, 9.5, 77.375, 51.125), (0, 10, 10, 10, 10),
         (0, 20.5, 12.25, 12.5, 6), (1, 1, 1, 49, 33)]
ROIS = BOXES + [BOXES[0], BOXES[0]]
MAPS = {'small': (9, 13, 0.25), 'large': (36, 52, 1.0)}          # h, w, spatial_scale
GEOMS = [('small', s) for s in ((1, 1), (3, 2), (7, 7), (28, 28))] + [('large', s) for s in ((1, 1), (3, 2), (7, 7))]
CMAX = 70


def _roi():
    from epropnp import roi
    return roi


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the fp64 oracle ----------------------------------------------------------------------------------------------------------------
def _corners(u, size):
    """clamped coordinate -> low index, high index, low weight, high weight (arrays over the cells)"""
    u = np.maximum(u, 0.0)
    lo = np.floor(u).astype(np.int64)
    edge = lo >= size - 1
    lo = np.where(edge, size - 1, lo)
    hi = np.where(edge, size - 1, lo + 1)
    u = np.where(edge, lo.astype(np.float64), u)
    frac = u - lo
    return lo, hi, 1.0 - frac, frac


def oracle(maps, rois, out_size, scale, sampling, aligned, cot=None):
    """maps (NI, C, h, w) fp64, rois (bn, 5) -> out (bn, C, ph, pw), and with `cot` (bn, C, ph, pw): the gradient, per element the
    absolute sum A of its terms (the backward on |cot|) and their number k.  Also what the fences and the cap need: the smallest
    distance of a sample coordinate from a cut, the smallest distance of a bin size from an integer it is not, the smallest grid, the
    share of samples that fall outside."""
    NI, C, h, w = maps.shape
    ph, pw = out_size
    out = np.zeros((len(rois), C, ph, pw))
    grad = None if cot is None else np.zeros((3,) + maps.shape)          # gradient, A, k
    info = dict(cut=math.inf, ceil=math.inf, grid=math.inf, samples=0, outside=0)
    o = 0.5 if aligned else 0.0
    I, J = np.arange(ph, dtype=np.float64), np.arange(pw, dtype=np.float64)
    for r, (n, x1, y1, x2, y2) in enumerate(np.asarray(rois, dtype=np.float64)):
        if not (np.isfinite([n, x1, y1, x2, y2]).all() and 0 <= n < NI):
            continue
        n = int(n)
        xs, ys, xe, ye = x1 * scale - o, y1 * scale - o, x2 * scale - o, y2 * scale - o
        rw, rh = xe - xs, ye - ys
        if not aligned:
            rw, rh = max(rw, 1.0), max(rh, 1.0)
        bh, bw = rh / ph, rw / pw
        for v in (bh, bw):
            if v != round(v):
                info['ceil'] = min(info['ceil'], abs(v - round(v)))
        gh = sampling if sampling > 0 else math.ceil(bh)
        gw = sampling if sampling > 0 else math.ceil(bw)
        count = max(gh * gw, 1)
        if gh > 0 and gw > 0:
            info['grid'] = min(info['grid'], gh * gw)
        if cot is not None:
            c3 = np.stack((cot[r], np.abs(cot[r]), np.ones_like(cot[r]))) / count           # (3, C, ph, pw)
            c3[2] *= count
        for iy in range(gh):
            y = ys + I * bh + (iy + .5) * bh / gh
            oky = ~((y < -1.0) | (y > h))
            info['cut'] = min(info['cut'], np.abs(y + 1.0).min(), np.abs(y - h).min())
            ylo, yhi, hy, ly = _corners(y, h)
            for ix in range(gw):
                x = xs + J * bw + (ix + .5) * bw / gw
                okx = ~((x < -1.0) | (x > w))
                if iy == 0:
                    info['cut'] = min(info['cut'], np.abs(x + 1.0).min(), np.abs(x - w).min())
                xlo, xhi, hx, lx = _corners(x, w)
                ok = oky[:, None] & okx[None, :]
                info['samples'] += ok.size
                info['outside'] += int((~ok).sum())
                for yy, wy in ((ylo, hy), (yhi, ly)):
                    for xx, wx in ((xlo, hx), (xhi, lx)):
                        wgt = np.where(ok, wy[:, None] * wx[None, :], 0.0)                    # (ph, pw): this sample's corner weight
                        out[r] += wgt * maps[n][:, yy[:, None], xx[None, :]]
                        if cot is not None:
                            YY, XX = np.broadcast_arrays(yy[:, None], xx[None, :])
                            term = c3 * wgt
                            term[2] = c3[2] * (wgt > 0)
                            np.add.at(grad[:, n], (slice(None), slice(None), YY, XX), term)
        out[r] /= count
    return out, grad, info


def _data(kind):
    h, w, _ = MAPS[kind]
    g = torch.Generator().manual_seed(20 + h)
    return torch.randn(2, CMAX, h, w, generator=g)


def _cot(shape, seed=5):
    return torch.randint(-16, 17, shape, generator=torch.Generator().manual_seed(seed)).float() / 8


@functools.lru_cache(maxsize=None)
def reference(kind, out_size, sampling, aligned):
    """the oracle on all CMAX channels (a case of fewer channels is the first ones: the op does not mix channels), with the fences"""
    h, w, scale = MAPS[kind]
    maps = _data(kind)
    cot = _cot((len(ROIS), CMAX) + out_size)
    out, grad, info = oracle(maps.double().numpy(), ROIS, out_size, scale, sampling, aligned, cot.double().numpy())
    assert info['cut'] >= FENCE, f'a sample coordinate lies {info["cut"]:.3e} from a cut: the inputs of this case are wrong'
    assert info['ceil'] >= FENCE_CEIL, f'a bin size lies {info["ceil"]:.3e} from an integer it is not: the inputs of this case are wrong'
    return dict(map=maps, cot=cot, out=torch.from_numpy(out), grad=torch.from_numpy(grad[0]), A=torch.from_numpy(grad[1]),
                k=torch.from_numpy(grad[2]), info=info, scale=scale)


def layout(x, how):
    """a copy of the values as a contiguous NCHW tensor, a channels-last one, or a channel slice of a wider tensor (not dense)"""
    if how == 'nchw':
        return x.clone(memory_format=torch.contiguous_format)
    if how == 'cl':
        return x.clone(memory_format=torch.channels_last)
    wide = torch.full((x.shape[0], x.shape[1] + 3) + tuple(x.shape[2:]), 9.0, dtype=x.dtype, device=x.device)
    wide[:, 1:1 + x.shape[1]] = x
    view = wide[:, 1:1 + x.shape[1]]
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    return view


def note(kind, what, value):
    _worst[kind] = max(_worst.get(kind, 0.0), value)
    print(f'{what}: {kind} {value:.4f}  worst so far {_worst[kind]:.4f}')


def check_forward(what, got, want, peak, grid):
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    err = float((got.double().cpu() - want).abs().max()) / (UNIT * peak)
    note('forward error / (2^-24 max|map|)', what, err)
    assert FWD_BAR <= grid + 3, f'{what}: the bar {FWD_BAR} exceeds the cap {grid + 3} of a {grid}-sample grid'
    assert err <= FWD_BAR, f'{what}: forward error {err:.4f} > bar {FWD_BAR} (units of 2^-24 max|map|)'


def check_backward(what, got, want, A, k):
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    got = got.double().cpu()
    assert torch.equal(got[k == 0], torch.zeros_like(got[k == 0])), f'{what}: an element no RoI reaches is not exactly 0.0'
    tol = (k + 2) * UNIT * A
    err = (got - want).abs()
    assert bool((err[tol == 0] == 0).all()), f'{what}: an element whose terms are all zero is not exact'
    ratio = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    note('backward error / ((k + 2) 2^-24 A)', what, ratio)
    assert ratio <= 1.0, f'{what}: backward error is {ratio:.4f} of its tolerance'


# ---- the op against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['nchw', 'cl', 'sliced'])
@pytest.mark.parametrize('C', [1, 5, 70])
@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('sampling', [0, 2])
@pytest.mark.parametrize('kind,out_size', GEOMS)
def test_forward_and_backward_against_the_fp64_oracle(backend, kind, out_size, sampling, aligned, C, how):
    d = reference(kind, out_size, sampling, aligned)
    what = f'{kind} {out_size} sampling {sampling} aligned {aligned} C {C} {how}'
    x = layout(d['map'][:, :C].to(backend), how).requires_grad_(True)
    rois = torch.tensor(ROIS, dtype=torch.float32, device=backend)
    out = _roi().roi_align(x, rois, out_size, d['scale'], sampling, 'avg', aligned)
    assert out.shape == (len(ROIS), C) + out_size
    if how == 'cl' and C > 1:
        assert out.is_contiguous(memory_format=torch.channels_last), 'the output follows the memory format of the input'
    else:
        assert out.is_contiguous()
    peak = float(d['map'][:, :C].abs().max())
    check_forward(what, out.detach(), d['out'][:, :C], peak, d['info']['grid'])
    cot = d['cot'][:, :C].to(backend)
    grad, = torch.autograd.grad(out, x, cot)
    assert grad.shape == x.shape
    check_backward(what, grad, d['grad'][:, :C], d['A'][:, :C], d['k'][:, :C])
    # the adjoint identity, both sides summed in fp64: the backward is the transpose of the forward
    lhs = float((out.detach().double().cpu() * cot.double().cpu()).sum())
    rhs = float((x.detach().double().cpu() * grad.double().cpu()).sum())
    scale = float((d['A'][:, :C] * d['map'][:, :C].abs().double()).sum()) or 1.0
    assert abs(lhs - rhs) <= 4 * UNIT * scale, f'{what}: <out, cot> = {lhs!r} but <map, dmap> = {rhs!r}'


def test_the_cases_reach_what_they_are_meant_to_reach():
    """the samples of the six boxes: a quarter to a third fall outside the map on the aligned, adaptive grid; no cut closer than 4.9e-3"""
    for kind, out_size in GEOMS:
        for sampling in (0, 2):
            for aligned in (True, False):
                info = reference(kind, out_size, sampling, aligned)['info']
                assert info['cut'] >= 4.9e-3 and info['ceil'] >= 1e-2, (kind, out_size, sampling, aligned, info)
                assert info['outside'] > 0 and info['samples'] > info['outside']


# ---- paths the small cases do not take ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['nchw', 'cl'])
def test_spans_longer_than_the_weight_table_and_more_cells_than_a_round(backend, how):
    """a bin of 75 x 70 map pixels (the forward walks its span in chunks of 64) and 34 x 33 cells (two blocks of cell columns in the
    forward, two rounds of cells per axis in the backward)"""
    g = torch.Generator().manual_seed(3)
    for shape, box, out_size in (((1, 3, 70, 150), [(0, 0.25, 0.125, 150.375, 70.25)], (1, 2)),
                                 ((2, 3, 9, 13), [(1, 0.625, -1.25, 11.875, 8.375), (1, 2.125, 3.0, 6.5, 5.25)], (34, 33))):
        maps = torch.randn(shape, generator=g)
        cot = _cot((len(box), shape[1]) + out_size, seed=9)
        want, grad, info = oracle(maps.double().numpy(), box, out_size, 1.0, 0, True, cot.double().numpy())
        assert info['cut'] >= FENCE and info['ceil'] >= FENCE_CEIL, info
        x = layout(maps.to(backend), how).requires_grad_(True)
        out = _roi().roi_align(x, torch.tensor(box, dtype=torch.float32, device=backend), out_size)
        what = f'{shape} {out_size} {how}'
        check_forward(what, out.detach(), torch.from_numpy(want), float(maps.abs().max()), info['grid'])
        got, = torch.autograd.grad(out, x, cot.to(backend))
        check_backward(what, got, *(torch.from_numpy(a) for a in grad))


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['nchw', 'cl'])
def test_many_workgroups_per_roi_and_per_tile(how):
    """2 images x 256 channels x 58 x 100, 16 RoIs of 28 x 28 cells: several passes of a workgroup over its channels, four channel
    blocks per gradient tile, 7 x 13 tiles per image"""
    import install as emu
    emu.uninstall()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(11)
    maps = torch.randn(2, 256, 58, 100, generator=g)
    rois = []
    for k in range(16):                         # multiples of 1/8 in image pixels (scale 0.25); some stick out of the 400 x 232 image
        cx, cy = 8 * torch.randint(2, 48, (2,), generator=g).tolist()[0], 8 * torch.randint(2, 28, (1,), generator=g).item()
        half_w, half_h = torch.randint(90, 700, (2,), generator=g).tolist()
        rois.append((k % 2, cx - half_w / 8 + 0.125, cy - half_h / 8, cx + half_w / 8, cy + half_h / 8 + 0.375))
    cot = _cot((16, 256, 28, 28), seed=12)
    want, grad, info = oracle(maps.double().numpy(), rois, (28, 28), 0.25, 0, True, cot.double().numpy())
    assert info['cut'] >= FENCE and info['ceil'] >= FENCE_CEIL, info
    x = layout(maps.to(dev), how).requires_grad_(True)
    out = _roi().roi_align(x, torch.tensor(rois, dtype=torch.float32, device=dev), (28, 28), 0.25)
    check_forward(f'256 channels {how}', out.detach(), torch.from_numpy(want), float(maps.abs().max()), info['grid'])
    got, = torch.autograd.grad(out, x, cot.to(dev))
    check_backward(f'256 channels {how}', got, *(torch.from_numpy(a) for a in grad))


# ---- properties -----------------------------------------------------------------------------------------------------------------------
def _small(backend, C=5, how='nchw', out_size=(7, 7)):
    d = reference('small', out_size, 0, True)
    x = layout(d['map'][:, :C].to(backend), how).requires_grad_(True)
    return d, x, torch.tensor(ROIS, dtype=torch.float32, device=backend), d['cot'][:, :C].to(backend)


def test_an_image_without_rois_has_an_all_zero_gradient(backend):
    d, x, rois, cot = _small(backend)
    rois[:, 0] = 1.0
    out = _roi().roi_align(x, rois, (7, 7), 0.25)
    grad, = torch.autograd.grad(out, x, cot)
    assert torch.equal(grad[0], torch.zeros_like(grad[0])) and bool((grad[1] != 0).any())
    want, g64, _ = oracle(d['map'][:, :5].double().numpy(), rois.cpu().numpy(), (7, 7), 0.25, 0, True, cot.double().cpu().numpy())
    check_forward('all on image 1', out.detach(), torch.from_numpy(want), float(d['map'][:, :5].abs().max()), 1)
    check_backward('all on image 1', grad, *(torch.from_numpy(a) for a in g64))


@pytest.mark.parametrize('how', ['nchw', 'cl'])
def test_two_launches_agree_to_the_bit(backend, how):
    _, x, rois, cot = _small(backend, C=70, how=how)
    runs = []
    for _ in range(2):
        out = _roi().roi_align(x, rois, (7, 7), 0.25)
        runs.append((out.detach(), torch.autograd.grad(out, x, cot)[0]))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize('how', ['nchw', 'cl'])
def test_extract_rois_is_two_one_map_calls_bit_for_bit(backend, how):
    """key and value share one forward and one backward launch; x2d goes through its own at scale 1"""
    d = reference('small', (7, 7), 0, True)
    key = layout(d['map'][:, :6].to(backend), how).requires_grad_(True)
    value = layout(d['map'][:, 6:12].to(backend), how).requires_grad_(True)
    x2d = torch.randn(2, 2, 36, 52, generator=torch.Generator().manual_seed(1)).to(backend)
    rois = torch.tensor(ROIS, dtype=torch.float32, device=backend)
    cot_k, cot_v = d['cot'][:, :6].to(backend), d['cot'][:, 6:12].to(backend)
    x2d_roi, key_roi, value_roi = _roi().extract_rois(rois, x2d, key, value, roi_shape=(7, 7), output_stride=4)
    gk, gv = torch.autograd.grad([key_roi, value_roi], [key, value], [cot_k, cot_v])
    one_k, one_v = (_roi().roi_align(m, rois, (7, 7), 0.25, 0, 'avg', True) for m in (key, value))
    assert torch.equal(_bits(key_roi), _bits(one_k)) and torch.equal(_bits(value_roi), _bits(one_v))
    assert torch.equal(_bits(gk), _bits(torch.autograd.grad(one_k, key, cot_k)[0]))
    assert torch.equal(_bits(gv), _bits(torch.autograd.grad(one_v, value, cot_v)[0]))
    assert torch.equal(_bits(x2d_roi), _bits(_roi().roi_align(x2d, rois, (7, 7), 1.0)))
    assert x2d_roi.shape == (8, 2, 7, 7) and key_roi.shape == value_roi.shape == (8, 6, 7, 7)
    # a gradient for one of the two only
    only_v, = torch.autograd.grad(_roi().extract_rois(rois, x2d, key.detach(), value)[2][..., :7, :7].sum(), value, allow_unused=True)
    assert only_v is not None and torch.isfinite(only_v).all()


def test_no_roi_keeps_the_graph_connected(backend):
    _, x, rois, _ = _small(backend)
    out = _roi().roi_align_wrapper(x, rois[:0], (3, 2), 0.25)
    assert out.shape == (0, 5, 3, 2) and out.requires_grad
    grad, = torch.autograd.grad(out.sum(), x)
    assert torch.equal(grad, torch.zeros_like(grad))
    assert not _roi().roi_align_wrapper(x.detach(), rois[:0], 4).requires_grad
    parts = _roi().extract_rois(rois[:0], x.detach(), x, x, roi_shape=(3, 2))
    assert [tuple(p.shape) for p in parts] == [(0, 5, 3, 2)] * 3 and parts[1].requires_grad
    full = _roi().roi_align_wrapper(x, rois, (3, 2), 0.25)
    assert torch.equal(_bits(full), _bits(_roi().roi_align(x, rois, (3, 2), 0.25)))


def test_what_is_not_built_raises(backend):
    _, x, rois, _ = _small(backend)
    with pytest.raises(ValueError, match='not differentiable'):
        _roi().roi_align(x, rois.clone().requires_grad_(True), (7, 7))
    with pytest.raises(NotImplementedError, match='max'):
        _roi().roi_align(x, rois, (7, 7), 1.0, 0, 'max')
    with pytest.raises(ValueError):
        _roi().roi_align(x, rois[:, :4], (7, 7))
    with pytest.raises(ValueError):
        _roi().roi_align(x[0], rois, (7, 7))
    with pytest.raises(ValueError):
        _roi().roi_align(x, rois, (0, 7))


def test_a_cpu_tensor_raises():
    import install as emu
    emu.uninstall()
    x, rois = torch.randn(1, 2, 5, 5), torch.tensor([[0, 0.0, 0.0, 4.0, 4.0]])
    with pytest.raises(RuntimeError, match='HIP'):
        _roi().roi_align(x, rois, (2, 2))


def test_boxes_that_name_no_image_or_are_not_finite_give_zeros(backend):
    d, x, rois, cot = _small(backend)
    nan, inf = float('nan'), float('inf')
    bad = torch.tensor([[2, 4, 4, 40, 30], [-1, 4, 4, 40, 30], [nan, 4, 4, 40, 30], [1e9, 4, 4, 40, 30], [0, nan, 4, 40, 30],
                        [0, 4, -inf, 40, 30], [1, 4, 4, inf, 30], [0, -3e38, -3e38, 3e38, 3e38]], dtype=torch.float32, device=backend)
    both = torch.cat((bad[:4], rois[:1], bad[4:]))
    out = _roi().roi_align(x, both, (7, 7), 0.25)
    grad, = torch.autograd.grad(out, x, torch.ones_like(out))
    alone = _roi().roi_align(x, rois[:1], (7, 7), 0.25)
    assert torch.equal(_bits(out[4]), _bits(alone[0])) and bool((out[4] != 0).any())
    rest = torch.cat((out[:4], out[5:]))
    assert torch.equal(rest, torch.zeros_like(rest))
    assert torch.equal(_bits(grad), _bits(torch.autograd.grad(alone, x, torch.ones_like(alone))[0]))


def test_other_floating_dtypes_pass_the_dtype_boundary(backend):
    d, x, rois, cot = _small(backend)
    x64 = x.detach().double().requires_grad_(True)
    out = _roi().roi_align(x64, rois.double(), (7, 7), 0.25)
    assert out.dtype == torch.float64
    grad, = torch.autograd.grad(out, x64, cot.double())
    assert grad.dtype == torch.float64
    ref = _roi().roi_align(x, rois, (7, 7), 0.25)
    assert torch.equal(out.float(), ref.detach())


def test_every_output_and_gradient_element_is_written(backend, poisoned_empty):
    _, x, rois, cot = _small(backend, C=70, how='cl')
    out = _roi().roi_align(x, rois, (7, 7), 0.25)
    grad, = torch.autograd.grad(out, x, cot)
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()


@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_bits():
    import install as emu
    emu.uninstall()
    dev = torch.device('cuda:0')
    _, key, rois, cot = _small(dev, C=70, how='cl')
    value = (key.detach() * 0.5).requires_grad_(True)
    x2d = torch.randn(2, 2, 36, 52, device=dev)

    def step():
        _, k, v = _roi().extract_rois(rois, x2d, key, value, roi_shape=(7, 7))
        return (k, v) + torch.autograd.grad([k, v], [key, value], [cot, cot])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        key.mul_(-1.5)
    graph.replay()
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(captured, eager))
