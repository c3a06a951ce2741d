"""epropnp.roi.logsumexp_across_rois / logsoftmax_across_rois / softmax_across_rois (epropnp_roi_logsumexp_forward / _backward) and
epropnp.losses.MVDGaussianMixtureNLLLoss against an fp64 oracle written here.

The oracle states the definition with explicit four-corner gathers (no grid_sample): the image position of a cell centre of RoI i,
X = x1_i + (px + 0.5) / rw (x2_i - x1_i); for a neighbour j (same non-negative image id, strictly overlapping box) gx = 2 (X - x1_j) /
(x2_j - x1_j) - 1, valid = -1 < gx, gy < 1, u = clamp(((gx + 1) rw - 1) / 2, 0, rw - 1); out = log(exp(x_i) + sum_valid exp(bilinear
sample of x_j at (v, u))).  Next to it `composite32` restates the reference's own formulation (affine_grid through the overlap box,
grid_sample, masked_fill(-inf), logsumexp) in fp32 on the CPU; its deviation from the fp64 oracle ON THE SAME CASE is the cap: a kernel
less accurate than the reference is a defect, not a tolerance.  Every comparison of the op alone asserts   error <= bar   and
error <= the case's cap.  The forward computes in fp64 between its loads and the one rounding of each output, and a correctly rounded
value is at least as close to the exact one as any fp32 evaluation: its cap holds by construction.  The backward computes in fp64 too,
but from the SAVED fp32 output, which sits in the exponent of every gradient weight: half an ulp of it is the gradient's relative
error (the figures below), and the reference's autograd starts from its own, less accurate, fp32 output.  At 'crowd' the two come
within 5 % of each other (3.59e-7 against 3.78e-7), everywhere else the kernel is 1.9 .. 20 x closer.

Errors: the forward's is the largest absolute one, the backward's is relative to the largest |gradient|; both in units of the case's
input scale (30 for 'large', whose logits reach +-350, else 1), so 'large' is held to the same bars relative to its values.
Bars: 4 x the worst error seen over every case of this file and of tests/test_roi_reference.py, on the CPU emulation and on the
MI355X (each case prints its figures; the two agree to the digits shown):
                vs the recorded reference                 vs fp64 alone
    forward     emulation 5.102e-5,  MI355X 5.102e-5      emulation 4.761e-7,  MI355X 4.761e-7     (composite32: 1.8e-6 .. 8.1e-5)
                -> FWD_BAR 2.04e-4                        -> FWD_BAR64 1.90e-6
    backward    emulation 4.921e-6,  MI355X 4.921e-6      emulation 5.041e-7,  MI355X 5.041e-7     (composite32: 1.4e-7 .. 5.4e-6)
                -> BWD_BAR 1.97e-5                        -> BWD_BAR64 2.02e-6
The recorded reference's figures are its own rounding (it rounds the sampling grid through the overlap box: 5.1e-5 on a 28 x 28 map);
the tests of this file compare with fp64 and use the tighter pair.  The backward's worst against fp64 is the softmax(extra_dim=1)
run, which adds PyTorch's fp32 logsumexp / subtraction / exp on top of the op (the op alone: 3.592e-7); the composed runs are held to
the bar, not to a cap (both sides are fp32 there and which lands closer is chance).

The fence: the output is discontinuous where a cell centre lies on the border of a neighbour's box (|gx| = 1 or |gy| = 1).  Every box
of a drawn case is redrawn, with seeds counted upwards per box, until no cell centre of it or of an earlier box lies within 1e-3 (in g
units) of such a border; an unfenced draw of 40 RoIs does come within 1e-5.  Elsewhere the output is continuous (bilinear sampling is
continuous in u), so there are no other ties.  The deliberate cases of `nested` are constructed, not drawn.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

FWD_BAR, BWD_BAR = 2.04e-4, 1.97e-5            # the bars of the issue: every comparison of the two files, the recorded reference included
FWD_BAR64, BWD_BAR64 = 1.90e-6, 2.02e-6        # against fp64 alone (they imply the ones above)
assert FWD_BAR64 <= FWD_BAR and BWD_BAR64 <= BWD_BAR
FENCE = 1e-3
_worst = {}

# (n, images, c, rh, rw), first seed, (centre range, size range) in px, input scale
CASES = {
    'odd': ((9, 2, 3, 5, 7), 100, ((20.0, 180.0), (40.0, 140.0)), 3.0),
    'heads': ((12, 1, 8, 28, 28), 200, ((30.0, 170.0), (40.0, 160.0)), 3.0),
    'mix': ((10, 2, 1, 28, 28), 300, ((30.0, 170.0), (40.0, 160.0)), 3.0),
    'crowd': ((70, 1, 2, 4, 4), 400, ((90.0, 110.0), (60.0, 120.0)), 3.0),
    'large': ((9, 2, 3, 5, 7), 100, ((20.0, 180.0), (40.0, 140.0)), 90.0),          # 'odd' with inputs x 30
}


def _roi():
    from epropnp import roi
    return roi


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the fp64 oracle and the reference's fp32 formulation ---------------------------------------------------------------------------
def _pairs(rois):
    """(n, n) bool: j is a neighbour of i.  The differences are formed in the dtype of `rois` (exact or fp32: the sign is the same)"""
    ids = rois[:, 0].round()
    x1, y1, x2, y2 = rois[:, 1:].unbind(1)
    ow = torch.minimum(x2[:, None], x2[None]) - torch.maximum(x1[:, None], x1[None])
    oh = torch.minimum(y2[:, None], y2[None]) - torch.maximum(y1[:, None], y1[None])
    return (ids[:, None] == ids[None]) & (ids[:, None] >= 0) & (ow > 0) & (oh > 0) & ~torch.eye(len(rois), dtype=torch.bool)


def _axis(a1, a2, b1, b2, r):
    """cells of [a1, a2] (scalars) seen from the boxes [b1, b2] (J,): g (J, r), valid, the two corner indices, the fraction"""
    X = a1 + (torch.arange(r, dtype=a1.dtype) + 0.5) / r * (a2 - a1)
    g = 2 * (X[None] - b1[:, None]) / (b2 - b1)[:, None] - 1
    u = (((g + 1) * r - 1) / 2).clamp(0, r - 1)
    u0 = u.floor().long().clamp(0, r - 1)
    return g, (g > -1) & (g < 1), u0, (u0 + 1).clamp(max=r - 1), u - u0


def oracle(x, rois):
    """the definition, differentiable w.r.t. x, in the dtype of x"""
    n, c, rh, rw = x.shape
    if n == 0:
        return x.clone()
    r = rois.to(x.dtype)
    nb = _pairs(rois)
    rows = []
    for i in range(n):
        js = nb[i].nonzero().squeeze(1)
        if len(js) == 0:
            rows.append(x[i])
            continue
        _, okx, u0, u1, fu = _axis(r[i, 1], r[i, 3], r[js, 1], r[js, 3], rw)
        _, oky, v0, v1, fv = _axis(r[i, 2], r[i, 4], r[js, 2], r[js, 4], rh)
        k = js[:, None, None]
        g = lambda vv, uu: x[k, :, vv[:, :, None], uu[:, None, :]]                  # (J, rh, rw, c)
        fu, fv = fu[:, None, :, None], fv[:, :, None, None]
        s = ((1 - fu) * (1 - fv) * g(v0, u0) + fu * (1 - fv) * g(v0, u1)) + ((1 - fu) * fv * g(v1, u0) + fu * fv * g(v1, u1))
        ok = (oky[:, :, None] & okx[:, None, :])[..., None]
        s = torch.where(ok, s, torch.full_like(s, float('-inf'))).permute(0, 3, 1, 2)
        rows.append(torch.cat((x[i][None], s)).logsumexp(0))
    return torch.stack(rows)


def composite32(x, rois):
    """the reference's formulation (inter_roi_ops.py:19-81), restated: the yardstick of the caps"""
    n, c, rh, rw = x.shape
    if n == 0:
        return x.clone()
    ids, box = rois[:, 0].round().int(), rois[:, 1:]
    rows = []
    for i in range(n):
        lo, hi = torch.max(box[i, :2], box[:, :2]), torch.min(box[i, 2:], box[:, 2:])
        pos = (ids == ids[i]) & (ids[i] >= 0) & ((hi - lo) > 0).all(1)
        pos[i] = False
        if not pos.any():
            rows.append(x[i])
            continue
        js = pos.nonzero().squeeze(1)
        wh_i, wh_j = box[i, 2:] - box[i, :2], box[js, 2:] - box[js, :2]
        scale = wh_i / wh_j
        corner_j = 2 * (lo[js] - box[js, :2]) / wh_j - 1
        corner_i = 2 * (lo[js] - box[i, :2]) / wh_i - 1
        theta = x.new_zeros((len(js), 2, 3))
        theta[:, 0, 0], theta[:, 1, 1] = scale[:, 0], scale[:, 1]
        theta[:, :, 2] = corner_j - scale * corner_i
        grid = F.affine_grid(theta, (len(js), 1, rh, rw), align_corners=False)
        s = F.grid_sample(x[js], grid, padding_mode='border', align_corners=False)
        ok = ((grid > -1) & (grid < 1)).all(3).unsqueeze(1)
        rows.append(torch.cat((s.masked_fill(~ok, float('-inf')), x[i][None])).logsumexp(0))
    return torch.stack(rows)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def fence_distance(rois, rh, rw):
    """the smallest distance, in g units, of a cell centre from a border of a neighbour's box (inf without neighbours)"""
    r, nb = rois.double(), _pairs(rois)
    worst = float('inf')
    for i in range(len(rois)):
        js = nb[i].nonzero().squeeze(1)
        if len(js):
            gx = _axis(r[i, 1], r[i, 3], r[js, 1], r[js, 3], rw)[0]
            gy = _axis(r[i, 2], r[i, 4], r[js, 2], r[js, 4], rh)[0]
            worst = min(worst, float((gx.abs() - 1).abs().min()), float((gy.abs() - 1).abs().min()))
    return worst


def draw_rois(n, images, rh, rw, seed, spec):
    """fenced boxes, one after the other: box k keeps the first of the seeds seed + 1000 k, + 1, ... that fences it against the boxes
    before it.  Image ids are interleaved and given as floats off by 1e-4."""
    (c_lo, c_hi), (s_lo, s_hi) = spec
    rois = torch.zeros(0, 5)
    for k in range(n):
        for attempt in range(400):
            g = torch.Generator().manual_seed(seed + 1000 * k + attempt)
            centre = c_lo + torch.rand(2, generator=g) * (c_hi - c_lo)
            half = (s_lo + torch.rand(2, generator=g) * (s_hi - s_lo)) / 2
            row = torch.cat((torch.tensor([k % images + (1e-4 if k % 2 else -1e-4)]), centre - half, centre + half))
            cand = torch.cat((rois, row[None]))
            if fence_distance(cand, rh, rw) >= FENCE:
                break
        else:
            raise AssertionError('no fenced box found')
        rois = cand
    return rois


def _nested():
    """constructed: a box strictly inside another (image 0), two identical boxes (image 1: every cell valid, u on integers), a pair
    touching along an edge (image 2), a zero-width box inside another (image 3)"""
    rois = torch.tensor([[0, 10.0, 10.0, 110.0, 90.0], [0, 30.3, 25.7, 71.9, 60.1],
                         [1, 5.0, 5.0, 61.0, 47.0], [1, 5.0, 5.0, 61.0, 47.0],
                         [2, 0.0, 0.0, 50.0, 50.0], [2, 50.0, 0.0, 90.0, 50.0],
                         [3, 20.0, 20.0, 20.0, 60.0], [3, 10.0, 10.0, 40.0, 70.0]])
    x = 3.0 * torch.randn(8, 2, 5, 6, generator=torch.Generator().manual_seed(500))
    return x, rois


def _alone():
    """one RoI per image (ids 0, 1, 2), two RoIs with id -1 on one box and a RoI of another image on that box too"""
    same = [40.0, 40.0, 90.0, 100.0]
    rois = torch.tensor([[0, 10.0, 10.0, 80.0, 90.0], [1, 10.0, 10.0, 80.0, 90.0], [2, 30.0, 5.0, 60.0, 70.0],
                         [-1] + same, [-1] + same, [3] + same])
    x = 3.0 * torch.randn(6, 2, 5, 7, generator=torch.Generator().manual_seed(600))
    return x, rois


@functools.lru_cache(maxsize=None)
def case(name):
    """x, rois, the fp64 output, a random cotangent, the fp64 gradient, composite32's forward and backward error (the caps)"""
    if name == 'nested':
        x, rois = _nested()
    elif name == 'alone':
        x, rois = _alone()
    else:
        (n, images, c, rh, rw), seed, spec, scale = CASES[name]
        rois = draw_rois(n, images, rh, rw, seed, spec)
        x = scale * torch.randn(n, c, rh, rw, generator=torch.Generator().manual_seed(seed + 7))
    assert fence_distance(rois, x.shape[2], x.shape[3]) >= FENCE
    x64 = x.double().requires_grad_(True)
    want = oracle(x64, rois)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(77))
    grad = torch.autograd.grad((want * cot.double()).sum(), x64)[0]
    want = want.detach()
    if name in CASES:                                 # a drawn case that pairs nothing would test nothing
        changed = (want != x.double()).flatten(1).any(1)
        assert int(changed.sum()) * 2 >= len(rois), f'{name}: only {int(changed.sum())} of {len(rois)} RoIs change'
    x32 = x.clone().requires_grad_(True)
    ref = composite32(x32, rois)
    ref_grad = torch.autograd.grad((ref * cot).sum(), x32)[0]
    unit = CASES[name][3] / 3.0 if name in CASES else 1.0
    return dict(x=x, rois=rois, want=want, cot=cot, grad=grad, unit=unit, cap_fwd=fwd_error(ref.detach(), want, unit),
                cap_bwd=bwd_error(ref_grad, grad, unit))


def fwd_error(got, want, unit=1.0):
    """the largest absolute error, in units of the case's input scale (30 for 'large', else 1)"""
    assert torch.isfinite(got).all()
    return float((got.double().cpu() - want).abs().max()) / unit


def bwd_error(got, want, unit=1.0):
    """the largest error relative to the largest |gradient|, in units of the case's input scale: the saved fp32 output sits in the
    exponent of every gradient weight, so its half ulp -- which grows with the values -- is the gradient's relative error"""
    assert torch.isfinite(got).all()
    return float((got.double().cpu() - want).abs().max()) / (float(want.abs().max()) or 1.0) / unit


def check(kind, what, err, bar, cap=None):
    _worst[kind] = max(_worst.get(kind, 0.0), err)
    print(f'{what}: {kind} error {err:.3e}  the reference on this case {cap if cap is None else format(cap, ".3e")}  bar {bar:.3e}  '
          f'worst so far {_worst[kind]:.3e}')
    assert err <= bar, f'{what}: {kind} error {err:.3e} > bar {bar:.3e}'
    if cap is not None:
        assert err <= cap, f'{what}: {kind} error {err:.3e} > the reference\'s own {cap:.3e}'


ALL = list(CASES) + ['nested', 'alone']


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_forward_against_the_fp64_oracle(backend, name):
    d = case(name)
    got = _roi().logsumexp_across_rois(d['x'].to(backend), d['rois'].to(backend))
    assert got.shape == d['x'].shape and got.dtype == torch.float32
    check('forward', name, fwd_error(got, d['want'], d['unit']), FWD_BAR64, d['cap_fwd'])
    untouched = ~_pairs(d['rois']).any(1)
    if name == 'nested':
        assert untouched.tolist() == [False] * 4 + [True] * 4          # the touching pair and the zero-width box pair with nobody
        assert (d['want'][1] != d['x'][1].double()).all() and (d['want'][2] != d['x'][2].double()).all()      # every cell valid
    if name == 'alone':
        assert untouched.all()
    assert torch.equal(_bits(got.cpu()[untouched]), _bits(d['x'][untouched])), 'a RoI without neighbours must return its input bits'


def test_one_roi_and_no_roi(backend):
    f = _roi().logsumexp_across_rois
    d = case('alone')
    x, rois = d['x'][:1].to(backend), d['rois'][:1].to(backend)
    assert torch.equal(_bits(f(x, rois)), _bits(x))
    x0 = d['x'][:0].clone().to(backend).requires_grad_(True)
    out = f(x0, d['rois'][:0].to(backend))
    assert out.shape == (0, 2, 5, 7)
    out.sum().backward()
    assert x0.grad.shape == x0.shape
    for fn in (_roi().logsoftmax_across_rois, _roi().softmax_across_rois):
        assert fn(x0, d['rois'][:0].to(backend), extra_dim=1).shape == (0, 2, 5, 7)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _grad(dev, d, cot, fn=None):
    x = d['x'].clone().to(dev).requires_grad_(True)
    out = (fn or _roi().logsumexp_across_rois)(x, d['rois'].to(dev))
    return torch.autograd.grad((out * cot.to(dev)).sum(), x)[0]


@pytest.mark.parametrize('name', ALL)
def test_backward_against_fp64_autograd(backend, name):
    d = case(name)
    check('backward', name, bwd_error(_grad(backend, d, d['cot']), d['grad'], d['unit']), BWD_BAR64, d['cap_bwd'])


@pytest.mark.parametrize('name', ['odd', 'nested'])
def test_backward_with_the_cotangent_on_a_single_roi(backend, name):
    d = case(name)
    k = int(_pairs(d['rois']).any(1).nonzero()[1])          # a RoI with neighbours: its cotangent reaches them through the samples
    cot = torch.zeros_like(d['cot'])
    cot[k] = d['cot'][k]
    x64 = d['x'].double().requires_grad_(True)
    want = torch.autograd.grad((oracle(x64, d['rois']) * cot.double()).sum(), x64)[0]
    assert (want[torch.arange(len(want)) != k] != 0).any()
    got = _grad(backend, d, cot)
    check('backward', f'{name}, cotangent of RoI {k} alone', bwd_error(got, want), BWD_BAR64)
    assert ((got.cpu() == 0) | (want != 0)).all(), 'a cell the cotangent does not reach has a gradient'


@pytest.mark.parametrize('which', ['logsoftmax', 'logsoftmax_extra_dim', 'softmax', 'softmax_extra_dim'])
def test_backward_through_the_softmax_forms(backend, which):
    d = case('odd')
    extra = 1 if which.endswith('extra_dim') else None
    fn = getattr(_roi(), which.split('_')[0] + '_across_rois')

    def restated(x, rois):
        lse = oracle(x, rois)
        y = x - (lse.logsumexp(dim=extra, keepdim=True) if extra else lse)
        return y.exp() if which.startswith('softmax') else y
    x64 = d['x'].double().requires_grad_(True)
    out64 = restated(x64, d['rois'])
    want = torch.autograd.grad((out64 * d['cot'].double()).sum(), x64)[0]
    x = d['x'].clone().to(backend).requires_grad_(True)
    out = fn(x, d['rois'].to(backend), extra_dim=extra)
    assert out.shape == x.shape
    # the value: the op's rounding, PyTorch's fp32 logsumexp over the channels and the subtraction: at most ~6 roundings at the
    # magnitude of the normaliser (below 32 here) -> 6 x 32 x 2^-24 absolute in the log-softmax, and exp() <= 1 passes that on
    assert float(oracle(d['x'].double(), d['rois']).abs().max()) < 32
    assert float((out.detach().double().cpu() - out64.detach()).abs().max()) <= 192 * 2.0 ** -24
    got = torch.autograd.grad((out * d['cot'].to(backend)).sum(), x)[0]
    check('backward', which, bwd_error(got, want), BWD_BAR64)


def test_rois_that_require_a_gradient_raise(backend):
    d = case('odd')
    rois = d['rois'].clone().to(backend).requires_grad_(True)
    for fn in (_roi().logsumexp_across_rois, _roi().logsoftmax_across_rois, _roi().softmax_across_rois):
        with pytest.raises(ValueError):
            fn(d['x'].to(backend), rois)


def test_shapes_limits_and_dtypes(backend):
    f = _roi().logsumexp_across_rois
    d = case('odd')
    x, rois = d['x'].to(backend), d['rois'].to(backend)
    with pytest.raises(ValueError):
        f(x[0], rois)
    with pytest.raises(ValueError):
        f(x, rois[:, :4])
    with pytest.raises(ValueError):
        f(torch.zeros(2, 1, 65, 64, device=backend), rois[:2])
    f(torch.zeros(2, 1, 64, 64, device=backend), rois[:2])
    # another floating dtype: through the package's dtype boundary (fp32 on the device) and back
    x64 = d['x'].double().to(backend).requires_grad_(True)
    out = f(x64, d['rois'].double().to(backend))
    assert out.dtype == torch.float64 and fwd_error(out.detach(), d['want']) <= FWD_BAR64
    g = torch.autograd.grad((out * d['cot'].double().to(backend)).sum(), x64)[0]
    assert g.dtype == torch.float64 and bwd_error(g, d['grad']) <= BWD_BAR64
    # the C entries refuse the same limits
    from epropnp import _hip
    z = torch.zeros(64, device=backend)
    p = _hip.ptr(z)
    for n, c, rh, rw in ((2, 1, 0, 4), (2, 1, 4, 0), (2, 1, 65, 64), (-1, 1, 4, 4)):
        assert _hip.lib().epropnp_roi_logsumexp_forward(p, p, n, c, rh, rw, p, None) == -1
        assert _hip.lib().epropnp_roi_logsumexp_backward(p, p, p, p, n, c, rh, rw, p, None) == -1
    assert _hip.lib().epropnp_roi_logsumexp_forward(None, None, 0, 3, 4, 4, None, None) == 0


# ---- determinism, every element -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['heads', 'crowd'])
def test_two_launches_agree_to_the_bit(backend, name):
    d = case(name)
    runs = []
    for _ in range(2):
        x = d['x'].clone().to(backend).requires_grad_(True)
        out = _roi().logsumexp_across_rois(x, d['rois'].to(backend))
        runs.append((out, torch.autograd.grad((out * d['cot'].to(backend)).sum(), x)[0]))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('name', ['odd', 'alone'])
def test_every_output_and_gradient_element_is_written(backend, poisoned_empty, name):
    d = case(name)
    x = d['x'].clone().to(backend).requires_grad_(True)
    out = _roi().logsumexp_across_rois(x, d['rois'].to(backend))
    grad = torch.autograd.grad((out * d['cot'].to(backend)).sum(), x)[0]
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert fwd_error(out.detach(), d['want']) <= FWD_BAR64 and bwd_error(grad, d['grad']) <= BWD_BAR64


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_bits():
    import install as emu
    emu.uninstall()
    dev = torch.device('cuda:0')
    d = case('heads')
    x, rois, cot = d['x'].clone().to(dev).requires_grad_(True), d['rois'].to(dev), d['cot'].to(dev)

    def step():
        out = _roi().logsumexp_across_rois(x, rois)
        return out, torch.autograd.grad((out * cot).sum(), x)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = step()
    with torch.no_grad():
        x.copy_(case('heads')['x'].to(dev).flip(0) * 1.5)
    graph.replay()
    graph.replay()
    eager_out, eager_grad = step()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager_out)) and torch.equal(_bits(grad), _bits(eager_grad))
    assert not torch.equal(_bits(eager_out), _bits(_roi().logsumexp_across_rois(d['x'].to(dev), rois)))


# ---- MVDGaussianMixtureNLLLoss ------------------------------------------------------------------------------------------------------
def mvd_restated(pred, target, logstd, logmix, rois, mean_inv_std, training, momentum=0.1, eps=1e-4):
    """mvd_gaussian_mixture_nll_loss.py:33-63, literally, in fp64 around the oracle -> the (n, h, w) loss and the buffer afterwards"""
    pred, logstd, logmix = pred.double(), logstd.double(), logmix.double()
    diff = pred.abs() if isinstance(target, int) and target == 0 else (pred if isinstance(target, int) else (pred - target.double()).abs())
    inv = torch.exp(-logstd).clamp(max=1 / eps)
    comp = -0.5 * (diff * inv).square().sum(-1) + logmix - logstd.sum(-1)
    lse = comp.logsumexp(1, keepdim=True)
    loss = -(lse if rois is None else oracle(lse, rois)).squeeze(1)
    if training:
        mw = logmix.exp().unsqueeze(-1)
        mean_inv_std = (1 - momentum) * mean_inv_std + momentum * float(((inv * mw).sum() / (mw.sum() * 2).clamp(min=eps)).detach())
    return loss / max(mean_inv_std, eps), mean_inv_std, float(comp.detach().abs().max())


@functools.lru_cache(maxsize=None)
def mvd_case():
    n, mix, rh, rw = 6, 3, 5, 7
    g = torch.Generator().manual_seed(900)
    rois = draw_rois(n, 2, rh, rw, 900, CASES['odd'][2])
    assert _pairs(rois).any(1).sum() * 2 >= n
    pred, target = 4 * torch.randn(n, mix, rh, rw, 2, generator=g), 4 * torch.randn(n, mix, rh, rw, 2, generator=g)
    logstd = 0.5 * torch.randn(n, mix, rh, rw, 2, generator=g)
    logstd[0, 0, 0, 0] = -12.0                         # exp(12) > 1 / eps: the clamp of the inverse standard deviation is hit
    pred[0, 0, 0, 0], target[0, 0, 0, 0] = torch.tensor([1e-4, -2e-4]), 0.0       # (a deviation that keeps the term of order 1)
    logmix = torch.randn(n, mix, rh, rw, generator=g).log_softmax(1)
    weight = torch.rand(n, rh, rw, generator=g)
    return pred, target, logstd, logmix, rois, weight


@pytest.mark.parametrize('with_rois', [False, True])
@pytest.mark.parametrize('target', ['tensor', 0, -1])
def test_mvd_loss_against_its_fp64_restatement(backend, target, with_rois):
    from epropnp.losses import MVDGaussianMixtureNLLLoss
    pred, tgt, logstd, logmix, rois, weight = mvd_case()
    tgt = tgt if target == 'tensor' else target
    dev = lambda t: t.to(backend) if torch.is_tensor(t) else t
    kw = dict(rois=rois.to(backend)) if with_rois else {}
    m = MVDGaussianMixtureNLLLoss(reduction='none', loss_weight=0.7).to(backend)
    assert m.mean_inv_std.dtype == torch.float32 and float(m.mean_inv_std) == 1.0 and list(m.state_dict()) == ['mean_inv_std']
    mean = 1.0
    for call in range(2):                              # training: the buffer moves with momentum 0.1, the loss is divided by the NEW value
        got = m(dev(pred), dev(tgt), logstd=dev(logstd), logmixweight=dev(logmix), **kw)
        want, mean, scale = mvd_restated(pred, tgt, logstd, logmix, rois if with_rois else None, mean, True)
        assert got.shape == (6, 5, 7)
        # fp32 against fp64: a chain of ~40 rounded operations on terms up to `scale` (2^-24 each -> 2.4e-6), with 4 x headroom
        tol = 1e-5 * max(1.0, scale, float(want.abs().max())) / min(1.0, mean)
        assert float((got.double().cpu() - 0.7 * want).abs().max()) <= tol
        assert abs(float(m.mean_inv_std) - mean) <= 1e-6 * mean
    m.eval()                                           # eval: the buffer stays
    got = m(dev(pred), dev(tgt), logstd=dev(logstd), logmixweight=dev(logmix), **kw)
    want, still, scale = mvd_restated(pred, tgt, logstd, logmix, rois if with_rois else None, mean, False)
    assert still == mean and abs(float(m.mean_inv_std) - mean) <= 1e-6 * mean
    tol = 1e-5 * max(1.0, scale, float(want.abs().max())) / min(1.0, mean)
    assert float((got.double().cpu() - 0.7 * want).abs().max()) <= tol
    # weight, avg_factor, reduction: mmdet's weighted_loss rule
    w64 = weight.double()
    args = (dev(pred), dev(tgt))
    kw.update(logstd=dev(logstd), logmixweight=dev(logmix))
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-5 * max(1.0, abs(float(b)), scale * want.numel() / min(1.0, mean))
    assert close(m(*args, weight=dev(weight), reduction_override='sum', **kw), 0.7 * (want * w64).sum())
    assert close(m(*args, weight=dev(weight), reduction_override='mean', **kw) * want.numel(), 0.7 * (want * w64).sum())
    assert close(m(*args, weight=dev(weight), avg_factor=13.0, reduction_override='mean', **kw) * 13.0, 0.7 * (want * w64).sum())
    none = m(*args, weight=dev(weight), avg_factor=13.0, reduction_override='none', **kw)
    assert none.shape == (6, 5, 7) and float((none.double().cpu() - 0.7 * want * w64).abs().max()) <= tol
    with pytest.raises(ValueError):
        m(*args, avg_factor=13.0, reduction_override='sum', **kw)
    with pytest.raises(ValueError):
        m(dev(pred), 1, **kw)


def test_mvd_loss_gradients_reach_the_predictions(backend):
    from epropnp.losses import MVDGaussianMixtureNLLLoss
    pred, tgt, logstd, logmix, rois, weight = mvd_case()
    leaves = [t.clone().to(backend).requires_grad_(True) for t in (pred, logstd, logmix)]
    m = MVDGaussianMixtureNLLLoss().to(backend)
    m(leaves[0], tgt.to(backend), logstd=leaves[1], logmixweight=leaves[2], rois=rois.to(backend)).backward()
    l64 = [t.double().requires_grad_(True) for t in (pred, logstd, logmix)]
    want, _, _ = mvd_restated(l64[0], tgt, l64[1], l64[2], rois, 1.0, True)
    want.mean().backward()
    for got, ref in zip(leaves, l64):
        assert bwd_error(got.grad, ref.grad) <= 1e-5      # fp32 autograd of the PyTorch part around the op: ~40 rounded operations
