"""The training step's glue kernels (csrc/eval_kernels.hip: adaptive_delta, mc_loss_*, shift_poses*, center_points, prepare_*,
exchange_pack, fill_u32) at the edges of their launch shapes, against plain PyTorch in fp64 on the CPU.

Every test runs on the `backend` fixture: the kernel sources on the CPU emulation, and the device under `-m gpu`.  B = 9 and 17 put
more than one object on an XCD (`object_of_block` permutes the blocks then) and 9 leaves a padded tail of blocks that return before
the block reductions; the objects carry distinct data, so a permuted or skipped object fails.

Tolerances: taken from the existing test of the same op where one exists (tests/test_api_dropin.py, test_preprocess.py,
test_sweep_kernels.py: named at the use).  Where a new input needs another, the bar is 4 x the error of the fp32 PyTorch
statement of the op against fp64 on the same input (the factor covers the order of the sums); the measured value stands next to the
bar.  None is derived from a kernel's output.

Inputs are cloned on their way to the backend: on the emulation `t.to('cpu', torch.float32)` is the tensor itself, and two runs
would accumulate into one `.grad`."""
import contextlib
import math
import os
import warnings

import pytest
import torch

import epropnp_oracle as orc
import preprocess_oracle as porc

U = 2.0 ** -24      # unit roundoff of fp32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t, backend, grad=False):
    t = t.clone().to(backend)
    return t.requires_grad_(True) if grad else t


def _f64(t):
    return t.detach().cpu().double()


def _binding_names(backend):
    """the ctypes nodes everywhere; the C++ nodes as well where they exist (the device; never under emulation)"""
    if backend.type != 'cuda':
        return ['ctypes']
    from epropnp import _hip
    held = os.environ.pop('EPROPNP_NO_TORCH_EXT', None)      # `poisoned_empty` sets it: ask _hip itself, with the variable lifted
    try:
        _hip._torch_ext = False                              # detect again
        found = _hip.torch_ext() is not None
    finally:
        _hip._torch_ext = False
        if held is not None:
            os.environ['EPROPNP_NO_TORCH_EXT'] = held
    return ['ctypes', 'ext'] if found else ['ctypes']


@contextlib.contextmanager
def _binding(name, monkeypatch):
    """`poisoned_empty` selects the ctypes binding through the environment; the 'ext' leg takes that back for its duration"""
    from epropnp import _hip
    if name == 'ext':
        monkeypatch.delenv('EPROPNP_NO_TORCH_EXT', raising=False)
        _hip._torch_ext = False                       # detect again
        assert _hip.torch_ext() is not None
    else:
        _hip._torch_ext = None
    try:
        yield
    finally:
        _hip._torch_ext = False
        monkeypatch.setenv('EPROPNP_NO_TORCH_EXT', '1')


def _rel_obj(a, b):
    """max |a - b| over an object's entries over the object's largest |b| -> (B,)"""
    a, b = _f64(a), _f64(b)
    d = (a - b).abs().reshape(a.shape[0], -1).amax(1)
    return d / b.abs().reshape(b.shape[0], -1).amax(1).clamp(min=1e-300)


# ======================================================================================================================
# 1. adaptive_delta
# ======================================================================================================================
DELTA_N = (2, 64, 257, 513, 1025, 4096)      # 64, 128 and 256 threads; one to sixteen trips of a thread's loop
REL = 0.3


def delta_inputs(family, B, N):
    g = _gen(100003 * B + 7 * N + len(family))
    u = torch.rand(B, N, 2, generator=g) * 2 - 1
    step = 3.0 * torch.arange(B, dtype=torch.float32)[:, None, None]          # every object somewhere else
    if family in ('wide', 'pivot_wide'):
        x = torch.tensor([620.0, 190.0]) + 40.0 * u + step
    elif family == 'tight':
        x = torch.tensor([1500.0, 900.0]) + 0.05 * u + step
    else:
        assert family == 'pivot'
        x = torch.tensor([1500.0, 900.0]) + 0.5 * u + step
    if family.startswith('pivot'):
        x[:, 0] = 0.0                                                          # the kernel's former pivot, far from the rest
    w = (torch.rand(B, N, 2, generator=g) * 0.01 + 1e-3) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float32)[:, None, None])
    return x, w


def _check_delta_values(delta, stats, x, w):
    ref = orc.adaptive_huber_delta(x.double(), w.double(), REL)
    sd = x.double().var(dim=-2).sum(dim=-1).sqrt()
    torch.testing.assert_close(_f64(delta), ref, rtol=1e-5, atol=1e-9)      # test_fused_delta_and_loss_match_torch's bar
    torch.testing.assert_close(_f64(stats[:, 1]), sd, rtol=1e-5, atol=0.0)
    # mean_w is a factor of delta: delta's bar
    torch.testing.assert_close(_f64(stats[:, 0]), w.double().mean(dim=(-2, -1)), rtol=1e-5, atol=0.0)
    # the mean: one fp32 rounding of the result (0.5 ulp) and of the pass-2 correction; 8 ulp = 2^-20 covers them
    torch.testing.assert_close(_f64(stats[:, 2:4]), x.double().mean(dim=-2), rtol=2.0 ** -20, atol=0.0)


@pytest.mark.parametrize('family', ['wide', 'tight'])
@pytest.mark.parametrize('B', [9, 17])
@pytest.mark.parametrize('N', DELTA_N)
def test_adaptive_delta_values_and_stats(backend, poisoned_empty, family, B, N):
    """delta and the four stats against fp64 at every thread count of the launcher and several trips of the loop"""
    from epropnp import functional as F
    x, w = delta_inputs(family, B, N)
    delta, stats = F.adaptive_delta(_dev(x, backend), _dev(w, backend), REL)
    _check_delta_values(delta, stats, x, w)


@pytest.mark.parametrize('family,N', [('pivot', 4096), ('pivot_wide', 512), ('pivot_wide', 4096)])
def test_adaptive_delta_outlier_first_point(backend, poisoned_empty, family, N):
    """x2d[b, 0] far from the object's other points.  Moments taken about the first point cancel by (distance / sd)^2 in
    sum d^2 - (sum d)^2 / n: 1.2e-4 of delta at ('pivot', 4096) where the fp32 PyTorch statement is at 1e-7, and 1.3e-5 at
    ('pivot_wide', 4096).  The bar is the one of every other input."""
    from epropnp import functional as F
    x, w = delta_inputs(family, 9, N)
    delta, stats = F.adaptive_delta(_dev(x, backend), _dev(w, backend), REL)
    _check_delta_values(delta, stats, x, w)


# gradient w.r.t. x2d, per object and relative to the object's largest entry: (x - mean) carries the rounding of the mean and of x
# itself in absolute terms.  Measured: the fp32 statement (autograd of orc.adaptive_huber_delta in fp32) against fp64 on these inputs,
# largest over the objects, per N.  ('tight': 0.05 px deviations from a mean near 1500, where an fp32 ulp is 1.2e-4 px; at N = 2 the
# two deviations are half a difference of a few ulp.)  The bar is 4 x the measured value.
DELTA_GX_FP32 = {'wide': {2: 7.3e-6, 64: 1.5e-6, 257: 1.6e-6, 513: 9.8e-7, 1025: 1.9e-6, 4096: 1.5e-6},
                 'tight': {2: 2.3e-2, 64: 2.5e-3, 257: 2.6e-3, 513: 4.4e-3, 1025: 2.7e-3, 4096: 2.0e-3}}


@pytest.mark.parametrize('family,B', [('wide', 9), ('tight', 17)])
@pytest.mark.parametrize('N', DELTA_N)
def test_adaptive_delta_gradients(backend, poisoned_empty, monkeypatch, family, B, N):
    """both gradients against fp64 autograd of the reference statement, through the ctypes node and the C++ node"""
    from epropnp import functional as F
    x, w = delta_inputs(family, B, N)
    up = torch.randn(B, generator=_gen(N))
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (orc.adaptive_huber_delta(xr, wr, REL) * up.double()).sum().backward()
    for name in _binding_names(backend):
        with _binding(name, monkeypatch):
            a, b = _dev(x, backend, True), _dev(w, backend, True)
            delta, _ = F.adaptive_delta(a, b, REL)
            (delta * up.to(backend)).sum().backward()
        torch.testing.assert_close(_f64(b.grad), wr.grad, rtol=1e-4, atol=1e-9)      # the existing test's bar
        err = _rel_obj(a.grad, xr.grad)
        assert float(err.max()) <= 4 * DELTA_GX_FP32[family][N], (name, err)


@pytest.mark.parametrize('N', [64, 1025])
def test_adaptive_delta_keeps_nonfinite_input(backend, poisoned_empty, N):
    """A NaN or an inf in x2d, or a NaN in w2d, gives a NaN delta exactly where the fp32 reference statement does (a clamp of the
    variance by fmaxf turned it into delta = 0), and the clean objects keep their values."""
    from epropnp import functional as F
    B = 9
    x, w = delta_inputs('wide', B, N)
    x[0, 3, 1] = float('nan')
    x[1, 0, 0] = float('inf')           # the first point
    w[2, N - 1, 0] = float('nan')
    x[4, 0, 1] = float('nan')           # the first point
    x[6, N // 2, 0] = float('-inf')
    ref32 = orc.adaptive_huber_delta(x, w, REL)
    bad = torch.isnan(ref32)
    assert bad.tolist() == [True, True, True, False, True, False, True, False, False]
    delta, _ = F.adaptive_delta(_dev(x, backend), _dev(w, backend), REL)
    delta = delta.cpu()
    assert torch.equal(torch.isnan(delta), bad), delta
    assert bool(torch.isfinite(delta[~bad]).all())
    ref = orc.adaptive_huber_delta(x.double(), w.double(), REL)
    torch.testing.assert_close(delta[~bad].double(), ref[~bad], rtol=1e-5, atol=1e-9)


def test_adaptive_delta_single_point(backend, poisoned_empty):
    """N = 1: the unbiased variance is 0 / 0, the reference statement returns NaN"""
    from epropnp import functional as F
    x, w = delta_inputs('wide', 9, 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')             # torch.var: degrees of freedom <= 0
        ref32 = orc.adaptive_huber_delta(x, w, REL)
    assert bool(torch.isnan(ref32).all())
    delta, stats = F.adaptive_delta(_dev(x, backend), _dev(w, backend), REL)
    assert bool(torch.isnan(delta).all()), delta
    torch.testing.assert_close(_f64(stats[:, 0]), w.double().mean(dim=(-2, -1)), rtol=1e-5, atol=0.0)
    assert torch.equal(stats[:, 2:4].cpu(), x[:, 0])


def test_adaptive_delta_identical_points(backend, poisoned_empty, monkeypatch):
    """All points of an object identical: sd = 0 and delta = 0 exactly, and the nodes' documented gradients -- d/dw = sd rel / 2N = 0,
    d/dx = mean_w rel (x - mean) / ((N - 1) max(sd, 1e-30)) = 0 -- are finite zeros.  (The reference statement's own gradient w.r.t.
    x2d is NaN there: sqrt'(0) = inf times 0.)"""
    from epropnp import functional as F
    B, N = 9, 257
    pt = torch.tensor([620.3, 190.7]) + 7.1 * torch.arange(B, dtype=torch.float32)[:, None]
    x = pt[:, None, :].expand(B, N, 2).contiguous()
    _, w = delta_inputs('wide', B, N)
    up = torch.randn(B, generator=_gen(1)) + 3.0
    for name in _binding_names(backend):
        with _binding(name, monkeypatch):
            a, b = _dev(x, backend, True), _dev(w, backend, True)
            delta, stats = F.adaptive_delta(a, b, REL)
            (delta * up.to(backend)).sum().backward()
        assert bool((delta == 0).all()) and bool((stats[:, 1] == 0).all()), (name, delta)
        assert torch.equal(stats[:, 2:4].detach().cpu(), pt)
        assert bool((a.grad == 0).all()) and bool((b.grad == 0).all()), name
        assert a.grad.shape == x.shape and b.grad.shape == w.shape


# ======================================================================================================================
# 2. mc_pose_loss, mc_pose_loss_reduced
# ======================================================================================================================
LOSS_SHAPES = [(1, 1), (5, 17), (31, 16), (33, 15), (257, 33),
               (2100, 1000)]     # 2.1 M elements: past the backward's 8192 x 256 threads, into its grid-stride loop
COL_EMPTY, COL_POSINF, COL_NAN, COL_LEAD = 2, 5, 7, 11


def loss_inputs(S, B):
    g = _gen(10007 * S + B)
    logw = 6.0 * torch.randn(S, B, generator=g) - 40.0
    ct = torch.rand(B, generator=g) * 5.0
    if B >= 15:
        logw[:, COL_EMPTY] = float('-inf')
        logw[S // 2, COL_POSINF] = float('inf')
        logw[S - 1, COL_NAN] = float('nan')
        logw[:max(1, S // 3), COL_LEAD] = float('-inf')      # a leading run: the online maximum starts at -inf
    return logw, ct


def _loss_statement(logw, ct):
    """the reference statement (monte_carlo_pose_loss.py): loss[isnan(loss)] = 0, in place -- a zero gradient enters a NaN column"""
    loss = torch.logsumexp(logw, dim=0)
    if ct is not None:
        loss = loss + ct
    loss = loss.clone()
    loss[torch.isnan(loss)] = 0
    return loss


@pytest.mark.parametrize('with_ct', [True, False])
@pytest.mark.parametrize('S,B', LOSS_SHAPES)
def test_mc_pose_loss_per_object(backend, poisoned_empty, monkeypatch, S, B, with_ct):
    """Values and both gradients against fp64 logsumexp; an empty column (loss -inf), a +inf (loss +inf), a NaN (loss 0, `lse` NaN:
    the mark the backward reads) and a leading run of -inf.  Bars: test_mc_loss_kernel_edge_values (values), test_fused_delta_and_loss_match_torch (gradients).
    The gradient's NaN pattern is the reference statement's, but for the NaN column: there the statement's autograd returns
    0 x NaN = NaN for the log-weights, and the kernels return the zero that enters (pinned by the existing test as well)."""
    from epropnp import functional as F
    logw, ct = loss_inputs(S, B)
    up = torch.randn(B, generator=_gen(S + B))
    lr = logw.double().requires_grad_(True)
    cr = ct.double().requires_grad_(True) if with_ct else None
    ref = _loss_statement(lr, cr)
    (ref * up.double()).sum().backward()
    ref = ref.detach()
    fin = torch.isfinite(ref)
    special = B >= 15
    if special:
        fin[COL_NAN] = False
        assert (~fin).nonzero().flatten().tolist() == [COL_EMPTY, COL_POSINF, COL_NAN]
        assert ref[COL_EMPTY] == float('-inf') and ref[COL_POSINF] == float('inf') and ref[COL_NAN] == 0
    for name in _binding_names(backend):
        with _binding(name, monkeypatch):
            a = _dev(logw, backend, True)
            b = _dev(ct, backend, True) if with_ct else None
            loss = F.mc_pose_loss(a, b)
            # the forward's second output is reachable as the ctypes node's saved tensor only (the C++ node keeps it to itself)
            lse = _f64(loss.grad_fn.saved_tensors[1]) if name == 'ctypes' else None
            (loss * up.to(backend)).sum().backward()
        loss = _f64(loss)
        if lse is not None:
            want = torch.logsumexp(logw.double(), dim=0)
            assert torch.equal(torch.isnan(lse), torch.isnan(want)) and bool(torch.isnan(lse).any()) == special
            keep = torch.isfinite(want)
            torch.testing.assert_close(lse[keep], want[keep], rtol=1e-5, atol=1e-5)
            assert torch.equal(lse[~keep & ~torch.isnan(want)], want[~keep & ~torch.isnan(want)])
        torch.testing.assert_close(loss[fin], ref[fin], rtol=1e-5, atol=1e-5)
        assert torch.equal(loss[~fin], ref[~fin]), (name, loss[~fin])
        ga, gr = _f64(a.grad), lr.grad.clone()
        if special:
            assert bool((ga[:, COL_NAN] == 0).all()), name
            assert bool(torch.isnan(gr[:, COL_NAN]).all())
            gr[:, COL_NAN] = 0
        nan = torch.isnan(gr)
        assert torch.equal(torch.isnan(ga), nan), name
        torch.testing.assert_close(ga[~nan], gr[~nan], rtol=1e-4, atol=1e-6)
        if with_ct:
            torch.testing.assert_close(_f64(b.grad), cr.grad, rtol=1e-6, atol=1e-7)
            if special:
                assert float(b.grad[COL_NAN]) == 0.0


def _ema32(nf, momentum, nf_in):
    """the reference's update of the running estimate: two separately rounded products, in fp32"""
    return nf.clone().mul_(1 - momentum).add_(momentum * nf_in)


REDUCED_LW, REDUCED_AVG = 0.5, 3.5


def _reduced_case(backend, monkeypatch, B, combos):
    """combos: (with_weight, scale, form of norm_factor_in) -- none, evaluation (norm_factor only), a scalar, one value per rank
    contiguous and as a strided view of a receive buffer.

    Loss bar, derived: the per-object losses carry the per-object bar (atol = rtol = 1e-5, above); the weighted sum adds
    gamma_d sum |w_b loss_b| with d the number of roundings on the longest path: ceil(B / T) additions of a thread's chain, 6 levels of
    the wave, up to 15 additions over the waves, and the products with the weight, with scale / norm_factor and that quotient.
    Gradients: the per-object bars (rtol 1e-4 / atol 1e-6 for the log-weights, 1e-6 / 1e-7 for cost_target) with the absolute parts
    scaled by the largest upstream factor |g scale / norm_factor w_b|, which is of order one in the per-object test."""
    from epropnp import functional as F
    S, mom = 3, 0.1
    g = _gen(B)
    logw = 6.0 * torch.randn(S, B, generator=g) - 40.0
    ct = torch.rand(B, generator=g) * 5.0
    weight = torch.rand(B, generator=g) + 0.5
    if B >= 255:
        logw[1, 3] = float('nan')
    ranks = torch.tensor([3.25, 4.5, 2.75, 5.0, 1.5])               # multiples of 1/4: their sum is exact in any order
    T = 256 if B <= 4096 else 1024
    depth = -(-B // T) + 6 + 15 + 3
    gup = 1.7
    for with_w, scale, mode in combos:
        nf0 = None if mode == 'none' else torch.tensor([2.5])
        nf_in = {'none': None, 'eval': None, 'scalar': torch.tensor(3.75), 'ranks': ranks}.get(mode)
        if mode == 'strided':
            buf = torch.full((3 * ranks.numel(),), float('nan'))
            buf[1::3] = ranks
        nf32 = nf0
        if mode == 'scalar':
            nf32 = _ema32(nf0, mom, nf_in)
        elif mode in ('ranks', 'strided'):
            nf32 = _ema32(nf0, mom, ranks.mean())
        nf64 = 1.0 if nf32 is None else float(nf32.double())
        lr, cr = logw.double().requires_grad_(True), ct.double().requires_grad_(True)
        per = _loss_statement(lr, cr)
        wper = per * weight.double() if with_w else per
        ref = wper.sum() * scale / nf64
        (ref * gup).backward()
        c = scale / nf64
        wabs = weight.double() if with_w else torch.ones(B, dtype=torch.float64)
        bar = c * float((wabs * (1e-5 + 1e-5 * per.detach().abs())).sum()) + depth * U * c * float(wper.detach().abs().sum())
        gscale = gup * c * float(wabs.max())
        for name in _binding_names(backend):
            runs = []
            for _ in range(2):
                with _binding(name, monkeypatch):
                    a, b = _dev(logw, backend, True), _dev(ct, backend, True)
                    nf = None if nf0 is None else _dev(nf0, backend)
                    if mode == 'strided':
                        vin = _dev(buf, backend)[1::3]
                        assert vin.stride(0) == 3
                    else:
                        vin = None if nf_in is None else _dev(nf_in, backend)
                    v = F.mc_pose_loss_reduced(a, b, weight=_dev(weight, backend) if with_w else None, scale=scale,
                                               momentum=mom, norm_factor_in=vin, norm_factor=nf)
                    (v * gup).backward()
                runs.append((v.detach().cpu(), None if nf is None else nf.cpu(), a.grad.cpu(), b.grad.cpu()))
            what = (name, with_w, scale, mode)
            v, nf, ga, gb = runs[0]
            assert v.dim() == 0
            assert abs(float(v) - float(ref.detach())) <= bar, (what, float(v), float(ref.detach()), bar)
            if nf is not None:
                assert torch.equal(nf, nf32), (what, nf, nf32)
            gr = lr.grad.clone()
            if B >= 255:
                assert bool((ga[:, 3] == 0).all()) and float(gb[3]) == 0.0, what
                gr[:, 3] = 0
            torch.testing.assert_close(ga.double(), gr, rtol=1e-4, atol=1e-6 * gscale)
            torch.testing.assert_close(gb.double(), cr.grad, rtol=1e-6, atol=1e-7 * gscale)
            for x, y in zip(runs[0], runs[1]):      # two calls on equal inputs: the same bits
                assert (x is None and y is None) or torch.equal(x, y), what


REDUCED_MODES = ('none', 'eval', 'scalar', 'ranks', 'strided')


def _reduced_scales(B):
    return (REDUCED_LW / B, REDUCED_LW, REDUCED_LW / REDUCED_AVG)      # mean, sum, avg_factor


@pytest.mark.parametrize('B', [1, 255, 256, 257])
def test_mc_pose_loss_reduced(backend, poisoned_empty, monkeypatch, B):
    """every reduction x with and without weight x every form of norm_factor_in, on the 256-thread launch"""
    _reduced_case(backend, monkeypatch, B, [(w, s, m) for w in (False, True) for s in _reduced_scales(B) for m in REDUCED_MODES])


@pytest.mark.parametrize('B', [4096, 4097])
def test_mc_pose_loss_reduced_thread_switch(backend, poisoned_empty, monkeypatch, B):
    """Both sides of the switch from 256 to 1024 threads.  Every reduction with and without weight, and every form of norm_factor_in,
    but not their full product (sixteen chain additions per thread make the emulation leg of one combination a quarter of a second)."""
    mean, total, avg = _reduced_scales(B)
    combos = [(w, s, 'scalar') for w in (False, True) for s in (mean, total, avg)]
    combos += [(True, avg, m) for m in REDUCED_MODES if m != 'scalar'] + [(False, mean, 'none')]
    _reduced_case(backend, monkeypatch, B, combos)


# ======================================================================================================================
# 3. shift_poses
# ======================================================================================================================
def shift_inputs(P, B, dof):
    g = _gen(1009 * P + 13 * B + dof)
    pose = torch.randn(P, B, 7 if dof == 6 else 4, generator=g)
    if dof == 6:      # R(q) is not normalised by the kernels: |q| in [0.8, 1.2]
        pose[..., 3:] = torch.nn.functional.normalize(pose[..., 3:], dim=-1) * (0.8 + 0.4 * torch.rand(P, B, 1, generator=g))
    offset = torch.randn(B, 3, generator=g)
    up = torch.randn(pose.shape, generator=g)
    return pose, offset, up


def _shift_statement(pose, offset, sign):
    from epropnp.common import rotate_offset
    return torch.cat((pose[..., :3] + sign * rotate_offset(pose, offset), pose[..., 3:]), dim=-1)


def _check_shift(backend, monkeypatch, P, B, dof, sign, atol_out=1e-6, atol_grad=1e-6):
    from epropnp import functional as F
    pose, offset, up = shift_inputs(P, B, dof)
    r = pose.double().requires_grad_(True)
    ref = _shift_statement(r, offset.double(), sign)
    (ref * up.double()).sum().backward()
    plain = F.shift_poses(_dev(pose, backend), _dev(offset, backend), sign)          # the launch without a node
    for name in _binding_names(backend):
        with _binding(name, monkeypatch):
            a = _dev(pose, backend, True)
            out = F.shift_poses(a, _dev(offset, backend), sign)
            (out * up.to(backend)).sum().backward()
        assert torch.equal(out.detach(), plain), name
        # defaults: the bars of test_shift_poses_is_differentiable_in_the_pose (the same input distribution)
        torch.testing.assert_close(_f64(out), ref.detach(), rtol=1e-5, atol=atol_out)
        torch.testing.assert_close(_f64(a.grad), r.grad, rtol=1e-5, atol=atol_grad)


@pytest.mark.parametrize('sign', [1.0, -1.0])
@pytest.mark.parametrize('dof', [4, 6])
def test_shift_poses_backward_many_poses_per_object(backend, poisoned_empty, monkeypatch, dof, sign):
    """P = 37 poses of each of B = 11 objects: the backward's `b = i % B` with P > 1, against fp64 autograd of rotate_offset"""
    _check_shift(backend, monkeypatch, 37, 11, dof, sign)


@pytest.mark.parametrize('dof', [4, 6])
def test_shift_poses_grid_stride(backend, poisoned_empty, monkeypatch, dof):
    """P B = 1,054,720 > 4096 blocks x 256 threads: forward and backward take a second trip of their grid-stride loops; every
    element compared.  A million normal draws reach further than the six poses of the existing test: the fp32 PyTorch statement (forward
    and autograd) against fp64 on these inputs needs, beside rtol = 1e-5, an absolute part of 1.9e-7 (values) / 4.6e-7 (gradients) at
    4-DoF and 5.2e-7 / 1.47e-6 at 6-DoF; the bars are 4 x those, or the existing 1e-6 where that is more."""
    atol_out, atol_grad = (1e-6, 4 * 4.6e-7) if dof == 4 else (4 * 5.2e-7, 4 * 1.47e-6)
    _check_shift(backend, monkeypatch, 1030, 1024, dof, -1.0, atol_out, atol_grad)


@pytest.mark.parametrize('dof', [4, 6])
def test_shift_poses_pair_equals_two_launches(backend, poisoned_empty, monkeypatch, dof):
    """shift_poses_pair_kernel -- pnp_denormalize of pose_opt and of the samples in one launch, which the one-call forward makes with
    EPROPNP_TUNE=no_denorm_fold (by default the AMIS launch writes both) -- against two launches of shift_poses on the solver-frame
    outputs of the same call: the same bits."""
    from epropnp import _hip
    from epropnp import functional as F
    from epropnp.epropnp import EProPnP4DoF, EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver
    from helpers import make_layer_objects, pack_noise, set_tune
    B, N, S, K = 9, 40, 32, 2
    prob = orc.make_problem(B, N, dof, seed=21)
    p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
    cf.set_param(p['x2d'], p['w2d'])
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=22), dof).to(backend)
    layer = (EProPnP6DoF if dof == 6 else EProPnP4DoF)(mc_samples=S, num_iter=K, normalize=True, solver=LMSolver(dof=dof, num_iter=3))
    seen = []
    real = F._FusedMonteCarlo.apply
    monkeypatch.setattr(F._FusedMonteCarlo, 'apply', staticmethod(lambda *a: (seen.append(real(*a)), seen[-1])[1]))
    set_tune(monkeypatch, no_denorm_fold=True)
    with _binding('ctypes', monkeypatch):
        _hip.profile(enable=True, reset=True)
        try:
            layer.monte_carlo_forward(p['x3d'], p['x2d'], p['w2d'], cam, cf, pose_init=p['pose_init'], force_init_solve=False, noise=noise)
            launches = _hip.profile_read('shift_poses')[1]
        finally:
            _hip.profile(enable=False, reset=True)
    assert launches == 1 and len(seen) == 1
    pose_opt_n, samples_n, _, _, _, pose_opt, samples, _, offset = seen[0]
    assert samples.shape == (S, B, 7 if dof == 6 else 4)
    assert torch.equal(pose_opt, F.shift_poses(pose_opt_n, offset, -1.0))
    assert torch.equal(samples, F.shift_poses(samples_n, offset, -1.0))


# ======================================================================================================================
# 4. center_points / pnp_normalize
# ======================================================================================================================
CENTER_SHAPES = [(1, 1), (9, 63), (17, 128), (3, 8193),      # 8193: past kMaxResidentPoints, the 256-thread path
                 (2, 4097)]


def center_inputs(B, N, shift):
    g = _gen(31 * B + N)
    spread = 0.5 + 0.5 * torch.arange(B, dtype=torch.float32)[:, None, None]
    centre = torch.randn(B, 1, 3, generator=g)
    return torch.randn(B, N, 3, generator=g) * spread + centre + shift


# |mean - fp64 mean| of the fp32 PyTorch statement `x3d.mean(dim=-2)` on these inputs, largest over CENTER_SHAPES and the entries:
# shift 0: 2.4e-7, shift 100: 1.24e-5
CENTER_BAR = {0.0: 4 * 2.4e-7, 100.0: 4 * 1.24e-5}


@pytest.mark.parametrize('shift', [0.0, 100.0])
@pytest.mark.parametrize('B,N', CENTER_SHAPES)
def test_center_points(backend, poisoned_empty, B, N, shift):
    """offset and centred points against fp64, at the error of the fp32 mean; the centred points add the rounding of one subtraction"""
    from epropnp import functional as F
    x = center_inputs(B, N, shift)
    offset, out = F.center_points(_dev(x, backend))
    mean = x.double().mean(dim=-2)
    bar = CENTER_BAR[shift]
    assert offset.shape == (B, 3) and out.shape == (B, N, 3)
    assert float((_f64(offset) - mean).abs().max()) <= bar
    refc = x.double() - mean[:, None, :]
    assert float((_f64(out) - refc).abs().max()) <= bar + U * float(refc.abs().max())
    assert torch.equal(out, _dev(x, backend) - offset[:, None, :])      # centred on the offset the kernel reports


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('B,N', [(9, 63), (17, 128)])
def test_pnp_normalize_is_the_kernel_pair(backend, poisoned_empty, B, N, dof):
    """pose_n of pnp_normalize equals center_points followed by shift_poses, bit for bit"""
    from epropnp import functional as F
    from epropnp.common import pnp_normalize
    x = _dev(center_inputs(B, N, 100.0), backend)
    pose = _dev(shift_inputs(1, B, dof)[0][0], backend)
    offset, x_n, pose_n = pnp_normalize(x, pose)
    off2, x2 = F.center_points(x)
    assert torch.equal(offset, off2) and torch.equal(x_n, x2)
    assert torch.equal(pose_n, F.shift_poses(pose, off2, 1.0))
    ref = _shift_statement(_f64(pose), _f64(off2), 1.0)
    torch.testing.assert_close(_f64(pose_n), ref, rtol=1e-5, atol=1e-6 * 100)      # the shift's bar; offsets near 100, not 1


# ======================================================================================================================
# 5. prepare_correspondences / prepare_dense_correspondences
# ======================================================================================================================
PREP_N = (1, 2, 64, 65, 129, 257, 1500)


def prep_inputs(B, N, sigma, with_x3d, with_scale):
    g = _gen(977 * N + B + int(sigma))
    noc = (torch.rand(B, N, 3, generator=g) - 0.5) if with_x3d else None
    dim = (torch.rand(B, 3, generator=g) + 0.5) if with_x3d else None
    logits = 50.0 + sigma * torch.randn(B, N, 2, generator=g)       # the common offset cancels in both modes
    scale = (torch.rand(B, 2, generator=g) * 3 + 0.1) if with_scale else None
    up_w, up_x = torch.randn(B, N, 2, generator=g), torch.randn(B, N, 3, generator=g)
    return noc, dim, logits, scale, up_w, up_x


def _prep_run(fn, ins, extra, mode, up_w, up_x, dev, dtype):
    ins = [None if t is None else t.clone().to(dev, dtype).requires_grad_(True) for t in ins]
    out = fn(*ins, *extra, mode)
    x3d, w2d = out[0], out[-1]
    loss = (w2d * up_w.to(dev, dtype)).sum()
    if x3d is not None:
        loss = loss + (x3d * up_x.to(dev, dtype)).sum()
    loss.backward()
    return out, [None if t is None else t.grad for t in ins]


# w2d of the fp32 statement (preprocess_oracle.prepare_ref in fp32) against fp64 with logits 50 + 30 randn, relative, over PREP_N, B = 9
# and 17 and both modes, where the fp64 weight is a normal fp32 number: 1.32e-5 (the exponent's argument, up to ~130, is rounded to 4e-6 absolute
# more than once).  With 50 + 2 randn (measured 7.7e-6) the bar of test_prepare_matches_torch holds.
PREP_W_RTOL = {2.0: 2e-5, 30.0: 4 * 1.32e-5}


@pytest.mark.parametrize('mode', ['softmax', 'mean_exp'])
@pytest.mark.parametrize('sigma', [2.0, 30.0])
@pytest.mark.parametrize('with_x3d,with_scale', [(True, True), (False, False)])
@pytest.mark.parametrize('N', PREP_N)
@pytest.mark.parametrize('B', [9, 17])
def test_prepare_correspondences_many_objects(backend, poisoned_empty, B, mode, sigma, with_x3d, with_scale, N):
    """B = 9 and 17 through prepare_forward / prepare_backward: values and gradients with the bars of test_prepare_matches_torch.

    mean_exp at sigma = 30 has weights beyond fp32 in fp64 already.  The gradient of the logits of an (object, channel) holds the sum
    over all its points, so there it is compared on the channels whose every weight is an fp32 number (603 of the 728 of these
    inputs), with the same bar taken per channel -- rtol 2e-4 and 2e-5 of the channel's largest entry, not of the whole tensor's,
    because the channels' scales are up to e^80 apart.  Measured: the fp32 statement against fp64 on those channels is within 1.1e-5
    of the channel's largest entry and meets rtol = 2e-4 entry by entry without an absolute part; grad_scale within 2.0e-5 relative."""
    from epropnp.preprocess import prepare_correspondences
    noc, dim, logits, scale, up_w, up_x = prep_inputs(B, N, sigma, with_x3d, with_scale)
    ins = (noc, dim, logits, scale)
    (x_ref, w_ref), g_ref = _prep_run(porc.prepare_ref, ins, (), mode, up_w, up_x, 'cpu', torch.float64)
    (x, w), gr = _prep_run(prepare_correspondences, ins, (), mode, up_w, up_x, backend, torch.float32)
    w, w_ref = _f64(w), w_ref.detach()
    # weights whose exponential, before or after the scale, is beyond fp32 in fp64 already (mean_exp, sigma = 30) are left out
    ok = (w_ref < 1e38) & ((w_ref if scale is None else w_ref / scale.double()[:, None, :]) < 1e38)
    assert bool(ok.any())
    torch.testing.assert_close(w[ok], w_ref[ok], rtol=PREP_W_RTOL[sigma], atol=1e-7)
    if with_x3d:
        torch.testing.assert_close(_f64(x), x_ref.detach(), rtol=1e-6, atol=1e-7)
    wide = mode == 'mean_exp' and sigma == 30.0
    okc = ok.all(dim=1) & (g_ref[2].abs().amax(dim=1) < 1e38)            # (B, 2) channels
    assert bool(okc.any())
    for k, (a, b) in enumerate(zip(gr, g_ref)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        a = _f64(a)
        if wide and k == 2:        # grad_logits (B,N,2), per channel
            lim = 2e-4 * b.abs() + 2e-5 * b.abs().amax(dim=1, keepdim=True)
            bad = ~((a - b).abs() <= lim) & okc[:, None, :]
            assert not bool(bad.any()), (int(bad.sum()), float(((a - b).abs() / b.abs().amax(dim=1, keepdim=True))[bad].max()))
        elif wide and k == 3:      # grad_scale (B,2) = sum_n g_n p_n
            torch.testing.assert_close(a[okc], b[okc], rtol=2e-4, atol=0.0)
        else:
            torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5 * float(b.abs().max()))


@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('N', [129, 1500])
@pytest.mark.parametrize('B', [9, 17])
def test_mean_exp_overflows_where_the_reference_does(backend, poisoned_empty, B, N, with_scale):
    """mean_exp with one logit per object and channel 90 + log(N) / 2 above the others: l - mean lies in (88.7, 88.7 + log N), where
    exp(l - mean) is inf in fp32 and the weight exp(l - mean - log N) is not.  The fp32 reference statement is finite everywhere
    (checked first), so the kernel is."""
    from epropnp.preprocess import prepare_correspondences
    _, _, logits, scale, _, _ = prep_inputs(B, N, 2.0, False, with_scale)
    logits = 50.0 + 0.1 * (logits - 50.0)
    for b in range(B):
        logits[b, (7 * b) % N, 0] += 90.0 + 0.5 * math.log(N)
        logits[b, (11 * b + 1) % N, 1] += 90.0 + 0.5 * math.log(N)
    _, w32 = porc.prepare_ref(None, None, logits, scale, 'mean_exp')
    assert bool(torch.isfinite(w32).all())
    gap = (logits - logits.mean(dim=1, keepdim=True)).amax(dim=1)
    assert bool((gap > 88.8).all()) and bool((gap < 88.6 + math.log(N)).all())       # inside the window, off its ends
    _, w = prepare_correspondences(None, None, _dev(logits, backend), None if scale is None else _dev(scale, backend), 'mean_exp')
    assert bool(torch.isfinite(w).all()), int((~torch.isfinite(w)).sum())
    _, w64 = porc.prepare_ref(None, None, logits.double(), None if scale is None else scale.double(), 'mean_exp')
    torch.testing.assert_close(_f64(w), w64, rtol=PREP_W_RTOL[30.0], atol=1e-7)
    # the backward recomputes the same weights: finite gradients against fp64
    up = torch.zeros(B, N, 2)
    up[:, ::3] = 1e-30
    lg = _dev(logits, backend, True)
    (prepare_correspondences(None, None, lg, None, 'mean_exp')[1] * up.to(backend)).sum().backward()
    lr = logits.double().requires_grad_(True)
    (porc.prepare_ref(None, None, lr, None, 'mean_exp')[1] * up.double()).sum().backward()
    assert bool(torch.isfinite(lg.grad).all())
    torch.testing.assert_close(_f64(lg.grad), lr.grad, rtol=2e-4, atol=2e-5 * float(lr.grad.abs().max()))


def _dense_case(backend, B, H, W, N, mode, with_x3d, with_scale):
    import numpy as np
    from epropnp.preprocess import box_grid_params, prepare_dense_correspondences
    g = _gen(H * W + N + B)
    noc = (torch.rand(B, 3, H, W, generator=g) - 0.5) if with_x3d else None
    dim = (torch.rand(B, 3, generator=g) + 0.5) if with_x3d else None
    logits = 50.0 + 2.0 * torch.randn(B, 2, H, W, generator=g)
    scale = (torch.rand(B, 2, generator=g) * 3 + 0.1) if with_scale else None
    c_box = torch.rand(B, 2, generator=g) * 400 + 50.3
    s_box = torch.rand(B, generator=g) * 250 + 40.7
    box = box_grid_params(c_box, s_box, W)
    rs = np.random.RandomState(N + B)
    inds = torch.tensor(np.stack([rs.choice(H * W, size=N, replace=False) for _ in range(B)]), dtype=torch.int64)
    assert int(inds.max()) > H * W - H * W // 8             # the far end of the map is sampled
    up_w, up_x = torch.randn(B, N, 2, generator=g), torch.randn(B, N, 3, generator=g)
    ins = (noc, dim, logits, scale)
    (x_ref, p_ref, w_ref), g_ref = _prep_run(porc.prepare_dense_ref, ins, (box, inds), mode, up_w, up_x, 'cpu', torch.float64)
    p_ref32 = porc.prepare_dense_ref(None, None, logits, None, box, inds, mode)[1]
    (x, p, w), gr = _prep_run(prepare_dense_correspondences, ins, (box.to(backend), inds.to(backend)), mode, up_w, up_x, backend,
                              torch.float32)
    # the bars of test_prepare_dense_matches_reference_composite
    assert torch.equal(p.cpu(), p_ref32)
    torch.testing.assert_close(_f64(w), w_ref.detach(), rtol=2e-5, atol=1e-7)
    if with_x3d:
        torch.testing.assert_close(_f64(x), x_ref.detach(), rtol=1e-6, atol=1e-7)
    for a, b in zip(gr, g_ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape
            torch.testing.assert_close(_f64(a), b, rtol=2e-4, atol=2e-5 * float(b.abs().max()))      # the whole map, zeros included
            if a.dim() == 4:
                hit = torch.zeros(B, H * W, dtype=torch.bool)
                hit.scatter_(1, inds, True)
                assert bool((a.cpu().flatten(2)[~hit[:, None, :].expand(-1, a.shape[1], -1)] == 0).all())


@pytest.mark.parametrize('mode', ['mean_exp', 'softmax'])
@pytest.mark.parametrize('with_x3d,with_scale,N', [(True, True, 129), (False, False, 65)])
def test_prepare_dense_b9_wide_map(backend, poisoned_empty, mode, with_x3d, with_scale, N):
    """B = 9 on a 300 x 301 map: H W > 65536, W no power of two (the pixel grid's 32-bit divide / modulo)"""
    _dense_case(backend, 9, 300, 301, N, mode, with_x3d, with_scale)


@pytest.mark.parametrize('mode', ['mean_exp', 'softmax'])
def test_prepare_dense_b17_wide_map(backend, poisoned_empty, mode):
    """B = 17 on the same map: three objects per block group, a grid of 24 with seven returning blocks"""
    _dense_case(backend, 17, 300, 301, 129, mode, True, True)


def test_prepare_dense_zero_fill_past_the_grid_clamp(backend, poisoned_empty):
    """B = 3, 512 x 512, N = 64 with noc gradients: the zero fill of grad_noc is 2,359,296 words, past fill_u32_kernel's 2048 blocks x 1024
    words, so its grid-stride loop takes a second trip; the full gradient maps are compared, and every pixel that was not sampled is an
    exact zero (the buffers come NaN-filled)"""
    _dense_case(backend, 3, 512, 512, 64, 'mean_exp', True, True)


# ======================================================================================================================
# 6. exchange_pack
# ======================================================================================================================
def _pack(backend, rows, scalars, n_extra=3, **kw):
    from epropnp import functional as F
    n_scal = (0 if scalars is None else scalars.numel())
    if kw.get('sum_of') is not None:
        n_scal = max(n_scal, 1)
    send = torch.full((n_scal + rows.numel() + n_extra,), float('nan'), device=backend)
    kw = {k: (None if v is None else (_dev(v, backend) if torch.is_tensor(v) else v)) for k, v in kw.items()}
    out = F.exchange_pack(send, _dev(rows, backend), None if scalars is None else _dev(scalars, backend), **kw)
    assert out is send
    return send.cpu(), n_scal


@pytest.mark.parametrize('n_scal', [0, 1, 4, 300])                      # 300: more scalars than block 0 has threads
@pytest.mark.parametrize('n_rows', [0, 10, 1030, 1100000])             # 1.1 M: past the 1024-block clamp, a second trip of the copy loop
def test_exchange_pack_copies(backend, n_rows, n_scal):
    """rows and scalars land where ObjectExchange reads them, exactly; the floats behind them stay as they were"""
    g = _gen(n_rows + n_scal)
    rows = torch.randn(n_rows // 5, 5, generator=g) if n_rows % 5 == 0 else torch.randn(n_rows, generator=g)
    scalars = torch.randn(n_scal, generator=g) if n_scal else None
    a, n = _pack(backend, rows, scalars)
    b, _ = _pack(backend, rows, scalars)
    assert n == n_scal
    if n_scal:
        assert torch.equal(a[:n_scal], scalars)
    assert torch.equal(a[n_scal:n_scal + n_rows], rows.flatten())
    assert bool(torch.isnan(a[n_scal + n_rows:]).all()) and a.numel() == n_scal + n_rows + 3
    assert torch.equal(a[:n_scal + n_rows], b[:n_scal + n_rows])


@pytest.mark.parametrize('n_scal', [1, 4])
@pytest.mark.parametrize('weighted,row_len', [(False, 1), (True, 1), (True, 5)])
@pytest.mark.parametrize('n_sum', [1, 1023, 1024, 1025, 4099, 5000])      # around one trip of the four-chain loop (4 x 256), and several
def test_exchange_pack_sum(backend, n_sum, weighted, row_len, n_scal):
    """The first scalar as sum_scale * sum(sum_of [* row weight]) against fp64.

    Bound: |error| <= gamma_d |sum_scale| sum |term|, gamma_d = d u / (1 - d u), u = 2^-24, with d the number of roundings on the longest
    path from a term to the result: one product with the row weight; at most floor(n / 1024) + 4 additions into one of a thread's four
    chains (the full trips, then up to three tail additions into chain 0, and one to spare); 2 for (c0 + c1) + (c2 + c3); 6 levels of the
    wave's butterfly; 3 additions over the four waves; one product with sum_scale."""
    if row_len == 5:
        n_sum = -(-n_sum // 5) * 5            # (rows, 5): 5, 1025, 1025, 1025, 4100, 5000 floats
    g = _gen(n_sum + 17 * row_len)
    sum_of = torch.randn(n_sum // row_len, row_len, generator=g)
    roww = (torch.rand(n_sum // row_len, generator=g) + 0.5) if weighted else None
    rows = torch.randn(2, 5, generator=g)
    scalars = torch.randn(n_scal, generator=g) if n_scal > 1 else None
    sum_scale = 1.0 / 7.0
    a, n = _pack(backend, rows, scalars, sum_of=sum_of, sum_scale=sum_scale, sum_row_weight=roww)
    b, _ = _pack(backend, rows, scalars, sum_of=sum_of, sum_scale=sum_scale, sum_row_weight=roww)
    assert n == n_scal
    terms = sum_of.double() * (roww.double()[:, None] if weighted else 1.0)
    d = 1 + (n_sum // 1024 + 4) + 2 + 6 + 3 + 1
    gamma = d * U / (1 - d * U)
    s32 = float(torch.tensor(sum_scale, dtype=torch.float32))
    assert abs(float(a[0]) - s32 * float(terms.sum())) <= gamma * s32 * float(terms.abs().sum())
    if n_scal > 1:
        assert torch.equal(a[1:n_scal], scalars[1:])          # the first slot belongs to the sum
    assert torch.equal(a[n_scal:n_scal + 10], rows.flatten()) and bool(torch.isnan(a[n_scal + 10:]).all())
    assert torch.equal(a[:n_scal + 10], b[:n_scal + 10])


def test_exchange_pack_refusals(backend):
    """the launcher's refusals -- row weights without sum_of or without a positive row_len, a sum without a scalar slot, NULL scalars
    with slots, negative counts (the row and sum counts are unsigned in the ABI) -- raise, and nothing is written"""
    from epropnp import _hip
    t = lambda *s: torch.ones(*s, device=backend)
    rows, scal, src, roww = t(10), t(4), t(20), t(4)
    send = torch.full((64,), float('nan'), device=backend)
    p, st = _hip.ptr, _hip.stream_of(send)
    cases = {'row weights without sum_of': (p(rows), 10, p(scal), 4, None, 0, 1.0, p(roww), 5, p(send), st),
             'a sum without a scalar slot': (p(rows), 10, None, 0, p(src), 20, 1.0, None, 1, p(send), st),
             'NULL scalars with slots': (p(rows), 10, None, 2, None, 0, 1.0, None, 1, p(send), st),
             'NULL scalars with slots beside the sum': (p(rows), 10, None, 2, p(src), 20, 1.0, None, 1, p(send), st),
             'negative scalar count': (p(rows), 10, p(scal), -1, None, 0, 1.0, None, 1, p(send), st),
             'row weights with row_len 0': (p(rows), 10, p(scal), 4, p(src), 20, 1.0, p(roww), 0, p(send), st),
             'row weights with a negative row_len': (p(rows), 10, p(scal), 4, p(src), 20, 1.0, p(roww), -5, p(send), st)}
    for what, args in cases.items():
        with pytest.raises(RuntimeError, match='exchange_pack'):
            _hip.call('epropnp_exchange_pack', *args)
        if backend.type == 'cuda':
            torch.cuda.synchronize()
        assert bool(torch.isnan(send).all()), what
