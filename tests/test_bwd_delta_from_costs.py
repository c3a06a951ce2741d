"""The backward's threshold gradient from the forward's sample costs (include/epropnp_hip.h: epropnp_amis_backward_costs).

    grad_delta / delta = 2 sum_j a_j cost_j / delta^2 - sum_pairs c1 a_j |r|^2        (residuals in units of delta)

replaces the per-pair term sum_pairs a_j min(|r|^2, 1) of the sweep.  What must hold: the exported costs are the samples' Huber
costs; the per-point gradients keep their bits; grad_delta stays inside the bar the per-pair form is held to (tests/test_amis.py,
test_sweeps_over_the_range_of_delta_and_z_min); without costs the new entries are the old ones, bit for bit.

Shapes: B = 3, N = 300 (not a multiple of 16), S = 48, K = 2 -- under EPROPNP_TUNE=bwd_mfma=4,4 two chunks of 256 points per object,
under 4,2 three chunks of 128; nsplit 2 and 4 deal those chunks to workgroups, some of which then sweep nothing."""
import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise, set_tune
from test_amis import GRAD_TOL

B, N, S, K = 3, 300, 48, 2


def _has(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == want, f'the case no longer launches what it is named after: plan {plan}, wanted {want}'


def _ocam64(prob):
    return orc.Cam(prob['cam_mats'].double(), 0.1, *(prob[k].double() if k in prob else None for k in ('lb', 'ub')))


def _rho(prob, poses):
    """weighted residual norms (poses, B, N) without the projection clamp: only used to place the mid threshold"""
    p = orc.evaluate_project(prob['x3d'].double(), poses.double(), orc.Cam(prob['cam_mats'].double(), 0.1))
    return ((p - prob['x2d'].double()) * prob['w2d'].double()).norm(dim=-1)


def _problem(dev, dof, bounds, delta):
    """-> prob (host, fp32, with the case's threshold), device tensors, PnPProblem"""
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    prob = orc.make_problem(B, N, dof, seed=31, bounds=bounds)
    if delta == 'mid':      # the median residual norm at pose_init, per object: inliers and outliers in every object
        prob['delta'] = _rho(prob, prob['pose_init'].unsqueeze(0))[0].median(dim=-1).values.float()
    else:
        prob['delta'] = torch.full((B,), float(delta))
    p, cam, _ = make_layer_objects(prob, dev)
    return prob, p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)


def _forward(dev, hp, p, dof, check_plain=False):
    """the kernel's own samples and their exported costs, the cost of pose_init"""
    from epropnp import functional as F
    cov = (torch.eye(dof) * torch.tensor([0.02, 0.02, 0.3] + [1e-3] * (dof - 3))).expand(B, dof, dof).contiguous()
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=32), dof).to(dev)
    samples, logw, costs = F.amis_forward(hp, p['pose_gt'], cov.to(dev), S, K, noise=noise, with_costs=True)
    if check_plain:      # the extra output changes no other
        plain = F.amis_forward(hp, p['pose_gt'], cov.to(dev), S, K, noise=noise)
        assert torch.equal(samples, plain[0]) and torch.equal(logw, plain[1])
    cost_init = F.evaluate_cost(hp, p['pose_init'])
    return samples, costs, cost_init


def _oracle(prob, samples, g_logw, g_init, delta):
    """fp64: costs of the samples, autograd of sum_j -g_logw cost_j (+ g_init cost(pose_init)) w.r.t. delta"""
    dl = prob['delta'].double().clone()
    if delta == 1e20 or delta == float('inf'):
        dl = torch.full((B,), 1e20, dtype=torch.float64)
    dl.requires_grad_(True)
    x3d, x2d, w2d = (prob[k].double() for k in ('x3d', 'x2d', 'w2d'))
    cost = orc.evaluate(x3d, x2d, w2d, samples.double(), _ocam64(prob), dl, want_cost=True)[1]
    total = ((-cost) * g_logw.double()).sum()
    if g_init is not None:
        total = total + (orc.evaluate(x3d, x2d, w2d, prob['pose_init'].double(), _ocam64(prob), dl, want_cost=True)[1] * g_init.double()).sum()
    total.backward()
    return cost.detach(), dl.grad


def _weights(kind, seed=33):
    g = torch.Generator().manual_seed(seed)
    g_logw = torch.randn(S, B, generator=g)          # mixed signs
    g_init = torch.randn(B, generator=g)
    if kind == 'zeros':                              # exact zeros: never compacted into the pose table
        g_logw[3] = 0.0
        g_logw[10:14, 1] = 0.0
    elif kind == 'tail':                             # a low-weight tail that the default drop threshold (2^-24 of the total) removes
        g_logw[5:20, B - 1] *= 1e-12
        g_logw[40:, 0] *= 1e-10
    return g_logw, g_init


# every (dof, bounds, delta) with the pose_init term under 4,4 (exact zeros among the weights) and without it under 4,2 (a dropped
# tail), each at nsplit 1, 2, 4; the opposite pairing for the mid threshold, where grad_delta is largest
CASES = [pytest.param(dof, bounds, delta, tune, kind, with_init, id=f'{dof}dof-{bounds}-delta{delta}-{tune}-{kind}-init{int(with_init)}')
         for dof, bounds in ((6, None), (6, 'tight'), (4, None), (4, 'tight'))
         for delta in (0.0, 'mid', 3e3, 1e20)
         for tune, kind, with_init in (('4,4', 'zeros', True), ('4,2', 'tail', False)) + ((('4,4', 'tail', False), ('4,2', 'zeros', True)) if delta == 'mid' else ())]


@pytest.mark.parametrize('dof,bounds,delta,tune,kind,with_init', CASES)
def test_grad_delta_from_the_forwards_costs(backend, monkeypatch, dof, bounds, delta, tune, kind, with_init):
    from epropnp import functional as F
    set_tune(monkeypatch, bwd_mfma=tune)
    prob, p, hp = _problem(backend, dof, bounds, delta)
    waves, tiles = (int(v) for v in tune.split(','))
    samples, costs, cost_init = _forward(backend, hp, p, dof)
    g_logw, g_init = _weights(kind)
    if delta == 'mid':
        inl = (_rho(prob, samples.cpu()) <= prob['delta'].double()[None, :, None]).double().mean().item()
        assert 0.05 < inl < 0.95, f'the mid threshold should leave inliers and outliers: inlier share {inl}'
    dmax = float(prob['delta'].max())
    ref_cost, ref_gd = _oracle(prob, samples.cpu(), g_logw, g_init if with_init else None, delta)
    # 1. exported costs against the fp64 oracle: the bar of the log-weights (test_amis.py: 2e-4 max(1, |.|max))
    err = (costs.cpu().double() - ref_cost).abs().max().item()
    print(f'costs: err {err:.3e} (bar {2e-4 * max(1.0, ref_cost.abs().max().item()):.3e})')
    assert err <= 2e-4 * max(1.0, ref_cost.abs().max().item())
    pin, gin, cin = (p['pose_init'], g_init.to(backend), cost_init) if with_init else (None, None, None)
    args = (samples, g_logw.to(backend), pin, gin)
    # all weighted poses: pose_init is pose S of the table, with weight g_init (= sum |g_logw| without the init term)
    asum = g_logw.abs().sum(0).double() + (g_init.abs().double() if with_init else 0.0)
    for nsplit in (1, 2, 4):
        _has(F.launch_plan('backward', hp, S, pose_init=with_init, nsplit=nsplit), waves=waves, tiles=tiles, bf16=True,
             valu=False, parked=False, nsplit=nsplit)
        pair = F.amis_backward(hp, *args, nsplit=nsplit)
        cost = F.amis_backward(hp, *args, nsplit=nsplit, sample_costs=costs, cost_init=cin)
        again = F.amis_backward(hp, *args, nsplit=nsplit, sample_costs=costs, cost_init=cin) if nsplit == 2 else cost
        # 2. per-point gradients: the same bits with and without costs;  5. a second launch: the same bits
        for name, a, b, c in zip(('x3d', 'x2d', 'w2d', 'delta'), pair, cost, again):
            assert bool(torch.isfinite(b).all()), name
            assert torch.equal(b, c), name
            if name != 'delta':
                assert torch.equal(a, b), name
        # 3. grad_delta against the fp64 oracle, both paths inside the bar of test_amis.py's delta sweep:
        #    GRAD_TOL |ref|max + 1e-7 max(delta, 1) N sum_j |a_j|
        bound = GRAD_TOL * ref_gd.abs().max() + 1e-7 * max(dmax, 1.0) * N * asum
        e_pair, e_cost = ((g[3].cpu().double() - ref_gd).abs() for g in (pair, cost))
        print(f'init {with_init} nsplit {nsplit}: grad_delta err per-pair {e_pair.max().item():.3e}, from costs {e_cost.max().item():.3e}, '
              f'bound {bound.min().item():.3e}, |ref| {ref_gd.abs().max().item():.3e}')
        assert bool((e_pair <= bound).all()), (e_pair, bound)
        assert bool((e_cost <= bound).all()), (e_cost, bound)


@pytest.mark.parametrize('dof,bounds', [(6, None), (4, 'tight')])
def test_without_costs_the_new_entries_are_the_old_ones(backend, monkeypatch, dof, bounds):
    """4. NULL costs -- or cost_init NULL while the pose_init term is there -- through epropnp_amis_backward[_split]_costs: the bits of
    epropnp_amis_backward[_split]; so does EPROPNP_TUNE=bwd_dcost=0 with costs."""
    import ctypes as C
    from epropnp import _hip
    from epropnp import functional as F
    set_tune(monkeypatch, bwd_mfma='4,4')
    prob, p, hp = _problem(backend, dof, bounds, 'mid')
    samples, costs, cost_init = _forward(backend, hp, p, dof, check_plain=True)
    g_logw, g_init = (t.to(backend) for t in _weights('zeros'))
    ptr = _hip.ptr

    def entry(nsplit, *costs):
        """the old entries (no costs arguments) / the new ones, through raw pointers"""
        gx3d, gx2d, gw2d = hp.new(B, N, 3), hp.new(B, N, 2), hp.new(B, N, 2)
        gd = hp.new(B) if nsplit == 1 else hp.new(B, nsplit)
        name = ('epropnp_amis_backward' if nsplit == 1 else 'epropnp_amis_backward_split') + ('_costs' if costs else '')
        _hip.call(name, C.byref(hp.c), ptr(samples), ptr(g_logw), S, ptr(p['pose_init']), ptr(g_init), *((nsplit,) if nsplit > 1 else ()),
                  *(ptr(c) for c in costs), ptr(gx3d), ptr(gx2d), ptr(gw2d), ptr(gd), hp.stream)
        return gx3d, gx2d, gw2d, gd if nsplit == 1 else gd.sum(dim=1)

    for nsplit in (1, 2):
        old = entry(nsplit)
        for a, b in zip(old, F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, nsplit=nsplit)):      # (the package: NULL costs)
            assert torch.equal(a, b), nsplit
        for c, ci in ((None, None), (None, cost_init), (costs, None)):
            for a, b in zip(old, entry(nsplit, c, ci)):
                assert torch.equal(a, b), (nsplit, c is None, ci is None)
        with_costs = entry(nsplit, costs, cost_init)
        assert not torch.equal(with_costs[3], old[3])          # (the cost path is taken when both are there: other roundings)
        set_tune(monkeypatch, bwd_mfma='4,4', bwd_dcost=0)
        for a, b in zip(old, entry(nsplit, costs, cost_init)):
            assert torch.equal(a, b), nsplit
        set_tune(monkeypatch, bwd_mfma='4,4')


def test_non_finite_cost_of_a_kept_sample_and_costs_of_dropped_samples(backend, monkeypatch):
    """A kept sample whose pose is NaN makes grad_delta of its object non-finite on both paths (and leaves the other objects alone);
    the costs of dropped and zero-weight samples are never read: inf / NaN there changes nothing (no 0 x inf)."""
    from epropnp import functional as F
    set_tune(monkeypatch, bwd_mfma='4,4')
    prob, p, hp = _problem(backend, 6, None, 'mid')
    samples, costs, cost_init = _forward(backend, hp, p, 6)
    g_logw, g_init = (t.to(backend) for t in _weights('tail'))
    g_logw[7, 1] = 0.0
    base = F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, nsplit=1, sample_costs=costs, cost_init=cost_init)
    poisoned = costs.clone()
    poisoned[7, 1] = float('inf')                    # zero weight
    poisoned[5:20, B - 1] = float('nan')             # below the drop threshold
    poisoned[40:, 0] = float('inf')
    got = F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, nsplit=1, sample_costs=poisoned, cost_init=cost_init)
    for a, b in zip(base, got):
        assert torch.equal(a, b)
    bad = samples.clone()
    bad[2, 1] = float('nan')                         # a kept sample: its cost is NaN in the forward, its residuals in the sweep
    bad_costs = costs.clone()
    bad_costs[2, 1] = float('nan')
    pair = F.amis_backward(hp, bad, g_logw, p['pose_init'], g_init, nsplit=1)
    cost = F.amis_backward(hp, bad, g_logw, p['pose_init'], g_init, nsplit=1, sample_costs=bad_costs, cost_init=cost_init)
    assert bool((torch.isfinite(pair[3]) == torch.isfinite(cost[3])).all()), (pair[3], cost[3])
    assert not bool(torch.isfinite(cost[3][1])) and bool(torch.isfinite(cost[3][[0, 2]]).all())
    bad_costs[2, 1] = float('inf')                   # (a cost that overflowed)
    cost = F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, nsplit=1, sample_costs=bad_costs, cost_init=cost_init)
    assert not bool(torch.isfinite(cost[3][1])) and bool(torch.isfinite(cost[3][[0, 2]]).all())


@pytest.mark.parametrize('route', ['ctypes', 'composite'])
def test_layer_takes_the_cost_path_and_the_switch_restores_the_per_pair_bits(backend, monkeypatch, route):
    """Through the layer (one-call forward and the composite route): the node hands the forward's costs to the backward.  With
    EPROPNP_TUNE=bwd_dcost=0 the gradients are the per-pair ones; the two agree per point to the bits for x3d / x2d and, for grad_w2d
    (which carries the threshold's gradient under the adaptive delta), to the bar of the delta fold (2e-6 of the object's largest)."""
    from test_amis import run_layer
    monkeypatch.setenv('EPROPNP_NO_TORCH_EXT', '1')
    if route == 'composite':
        monkeypatch.setenv('EPROPNP_FUSED_FORWARD', '0')
    prob = orc.make_problem(B, 100, 6, seed=41)
    noise = orc.make_noise(B, 32, 2, 6, seed=42)
    a = run_layer(backend, prob, noise, 6, 32, 2, 3)
    set_tune(monkeypatch, bwd_dcost=0)
    b = run_layer(backend, prob, noise, 6, 32, 2, 3)
    for k in ('pose_opt', 'pose_samples', 'logweights', 'cost_init', 'loss_obj', 'gx3d', 'gx2d'):
        assert torch.equal(a[k], b[k]), k
    scale = b['gw2d'].abs().amax(dim=(1, 2), keepdim=True).clamp(min=1e-20)
    rel = ((a['gw2d'] - b['gw2d']).abs() / scale).max().item()
    print(f'grad_w2d: largest difference between the cost path and the per-pair path {rel:.3e} of the object\'s largest entry')
    assert 0 < rel < 2e-6


BIG = [pytest.param(600, 128, 128, 4, 'tensor', dict(waves=4, tiles=2), id='B600-N128-S128-4dof'),
       pytest.param(512, 512, 512, 6, None, dict(waves=4, tiles=4), id='B512-N512-S512-6dof')]


@pytest.mark.gpu
@pytest.mark.parametrize('Bb,Nb,Sb,dof,bounds,want', BIG)
def test_big_batch_instantiations_against_the_per_pair_path(Bb, Nb, Sb, dof, bounds, want):
    """6. The instantiations that the big batches launch (C4: 600 x 128, 4-DoF with a projection clamp; C2: >= 512 objects x 512 points),
    with and without the delta fold: per-point gradients to the bits of the per-pair path.  grad_delta: each path is held to
    GRAD_TOL |ref|max + 1e-7 max(delta, 1) N sum_j |a_j| of the fp64 truth (tests/test_amis.py, the case above), so two correct paths
    are within twice that of each other -- with the per-pair result standing in for |ref|max."""
    import install as emu
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    emu.uninstall()
    dev = torch.device('cuda:0')
    prob = orc.make_problem(Bb, Nb, dof, seed=51, bounds=bounds)
    p, cam, _ = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    _has(F.launch_plan('backward', hp, Sb, pose_init=True), valu=False, bf16=True, nsplit=1, **want)
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)
    samples, logw, costs = F.amis_forward(hp, pose_opt, pose_cov, Sb, 4, seed=3, with_costs=True)
    cost_init = F.evaluate_cost(hp, p['pose_init'])
    g = torch.Generator().manual_seed(52)
    g_logw = torch.softmax(logw, 0) * torch.randn(Bb, generator=g).to(dev)         # the loss's gradient shape: weights of one sign per object
    g_init = torch.randn(Bb, generator=g).to(dev)
    args = (samples, g_logw, p['pose_init'], g_init)
    pair = F.amis_backward(hp, *args)
    cost = F.amis_backward(hp, *args, sample_costs=costs, cost_init=cost_init)
    again = F.amis_backward(hp, *args, sample_costs=costs, cost_init=cost_init)
    for i in range(3):
        assert torch.equal(pair[i], cost[i]) and torch.equal(cost[i], again[i]), i
    assert torch.equal(cost[3], again[3])
    asum = g_logw.abs().sum(0) + g_init.abs()
    bound = 2 * (GRAD_TOL * pair[3].abs().max() + 1e-7 * hp.delta.clamp(min=1.0) * Nb * asum)
    err = (cost[3] - pair[3]).abs()
    print(f'grad_delta: largest |cost path - per-pair| / bound {float((err / bound).max()):.3e}, relative to |grad_delta|max '
          f'{float(err.max() / pair[3].abs().max()):.3e}')
    assert bool((err <= bound).all())
    # with the fold: grad_w2d moves by the difference of grad_delta times d delta / d w2d and no more
    rel = 0.5
    _, stats = F.adaptive_delta(hp.x2d, hp.w2d, rel)
    hf = F.PnPProblem(hp.x3d, hp.x2d, hp.w2d, cam, HuberPnPCost(delta=hp.delta), dof).fold_delta(stats, rel)
    fpair = F.amis_backward(hf, *args)
    fcost = F.amis_backward(hf, *args, sample_costs=costs, cost_init=cost_init)
    assert torch.equal(fpair[0], fcost[0]) and torch.equal(fpair[1], fcost[1]) and torch.equal(fcost[3], cost[3])
    want_w = pair[2] + (cost[3] * stats[:, 1] * (rel / (2 * Nb)))[:, None, None]
    scale = want_w.abs().amax(dim=(1, 2), keepdim=True).clamp(min=1e-20)
    assert ((fcost[2] - want_w).abs() / scale).max().item() < 2e-6


def test_huber_eps_does_not_enter_the_identity(backend, monkeypatch):
    """HuberPnPCost.eps smooths the solver's Jacobian (max(rho, eps)), not the Huber value that the sampler and this backward
    differentiate: a problem with a large eps exports the same costs and takes the cost path to the same grad_delta, to the bits."""
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    set_tune(monkeypatch, bwd_mfma='4,4')
    prob, p, hp = _problem(backend, 6, None, 'mid')
    _, cam, _ = make_layer_objects(prob, backend)
    he = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta'], eps=0.5), 6)
    assert he.huber_eps == 0.5 and hp.huber_eps != 0.5
    g_logw, g_init = (t.to(backend) for t in _weights('zeros'))
    outs = []
    for h in (hp, he):
        samples, costs, cost_init = _forward(backend, h, p, 6)
        outs.append((samples, costs, cost_init) + F.amis_backward(h, samples, g_logw, p['pose_init'], g_init, nsplit=1,
                                                                  sample_costs=costs, cost_init=cost_init))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
