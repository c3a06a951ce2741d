"""Oracle tests of the kernel instantiations that LARGE batches launch, at small batches.

The launchers pick template instantiations from the number of objects and the CU count as well as from N, so the tight,
conditioning-independent checks of tests/test_amis.py and tests/test_shape_fuzz.py (B = 1...7) never reach what C2, C4, C5 and
dense LineMOD launch on a 256-CU device.  Objects are independent: B only selects the template, so a few objects at the threshold
N, with the existing knobs forcing the instantiation, are the smallest shapes at which these kernels can go wrong.

Every case first asserts through `functional.launch_plan` -- the launchers' own decision functions -- that it launches the
instantiation it is named after, so a later change of the heuristics cannot turn a case into a test of another kernel silently.
Bars: those of the existing tests of the same quantities (test_amis, test_shape_fuzz._check, test_sweep_kernels,
test_pose_cam_grad, test_fused_and_limits._delta_fold_case)."""
import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise, set_tune
from test_amis import GRAD_TOL, _check_logweights, _mixture_logq, _ocam64, _rel  # noqa: F401  (_rel: the yardstick the bars were written in)

SK = [(32, 2), (80, 2)]      # S = 80, K = 2: 40 samples per iteration, a pose tile padded from 40 to 48 rows


def _has(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == want, f'the case no longer launches what it is named after: plan {plan}, wanted {want}'


def _setup(dev, B, N, dof, bounds, seed):
    from epropnp import functional as F
    prob = orc.make_problem(B, N, dof, seed=seed, bounds=bounds)
    p, cam, cf = make_layer_objects(prob, dev)
    return prob, p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)


def _take(prob, idx):
    """the objects `idx` of a problem dict as a problem of their own"""
    return {k: (v[idx].contiguous() if isinstance(v, torch.Tensor) and v.dim() > 0 else v) for k, v in prob.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def _forward(dev, hp, prob, dof, S, K, noise=None, lm=None):
    from epropnp import functional as F
    if noise is None:
        noise = pack_noise(orc.make_noise(hp.B, S, K, dof, seed=8), dof).to(dev)
    pose_opt, pose_cov = lm if lm is not None else F.lm_solve(hp, hp_pose_init(prob, dev), 3, with_pose_cov=True)[:2]
    out = F.amis_forward(hp, pose_opt, pose_cov, S, K, noise=noise, with_proposals=True)
    again = F.amis_forward(hp, pose_opt, pose_cov, S, K, noise=noise, with_proposals=True)
    for a, b in zip(out, again):       # fixed reduction order, no atomics: a second launch returns the same bits
        assert torch.equal(a, b)
    return out, noise, (pose_opt, pose_cov)


def hp_pose_init(prob, dev):
    return prob['pose_init'].to(dev)


# instantiation -> (dof, EPROPNP_FWD_SPLIT, tune keys, plan it must show, [(N, bounds), ...])
FORWARD = {
    '4x8': (6, 1, dict(fwd_mfma='4,8'), dict(waves=4, tiles=8, G=1, chunks=1, bf16=True, chunked=False, spilled=False),
            [(257, None), (512, None), (257, 'tight'), (512, 'tight')]),
    '4x12': (6, 1, {}, dict(waves=4, tiles=12, G=1, chunks=1, bf16=True, chunked=False, spilled=False), [(513, None), (768, None)]),
    # 769: two chunks, the second one holds a single point tile of one point
    'chunked-2': (6, 1, {}, dict(waves=4, tiles=8, G=1, chunks=2, bf16=True, chunked=True, spilled=False), [(769, None), (769, 'tight')]),
    'chunked-3': (6, 1, {}, dict(waves=4, tiles=8, G=1, chunks=3, bf16=True, chunked=True, spilled=False), [(1025, None)]),
    'chunked-4': (6, 1, {}, dict(waves=4, tiles=8, G=1, chunks=4, bf16=True, chunked=True, spilled=False), [(2048, None)]),
    'lds': (6, 1, {}, dict(tiles=0, G=1, chunks=1, bf16=False, chunked=False, spilled=False), [(2049, None)]),
    # 4-DoF: 12 resident tiles are not taken (they spill next to the von Mises sampler): the points stream through LDS
    'lds-4dof': (4, 1, {}, dict(tiles=0, G=1, chunks=1, bf16=False, chunked=False, spilled=False), [(513, 'tensor')]),
    # what the remaining BASELINE shapes launch (coverage gate below): C4's 4-DoF kernel with a projection clamp, and the split
    # kernel with a clamp at the tiles per wave of the LineMOD training call (G = 4) and of the dense crops (G = 8)
    '4x2-4dof': (4, 1, {}, dict(waves=4, tiles=2, G=1, chunks=1, bf16=True, chunked=False, spilled=False), [(128, 'tensor')]),
    'split-4x2': (6, 4, {}, dict(waves=4, tiles=2, G=4, chunks=1, bf16=True, chunked=False, spilled=False), [(512, 'tensor')]),
    'split-4x8': (6, 8, {}, dict(waves=4, tiles=8, G=8, chunks=1, bf16=True, chunked=False, spilled=False), [(2100, 'tensor')]),
}
# (one object for the eight-part split: on the emulation every part recomputes its siblings' shares, 64 sweeps per object)
FORWARD_B = {'split-4x8': 1}
FORWARD_CASES = [pytest.param(name, N, bounds, S, K, id=f'{name}-N{N}-{bounds}-S{S}')
                 for name, (_, _, _, _, shapes) in FORWARD.items() for N, bounds in shapes for S, K in (SK[:1] if name == 'split-4x8' else SK)]


@pytest.mark.parametrize('name,N,bounds,S,K', FORWARD_CASES)
def test_forward_instantiation_against_the_oracle(backend, monkeypatch, poisoned_empty, name, N, bounds, S, K):
    """The unsplit register instantiations (4 x 8, 4 x 12, chunked with 2...4 chunks) and the LDS-streaming one, which few objects
    reach on a 256-CU device only with the split over workgroups switched off (EPROPNP_FWD_SPLIT=1)."""
    from epropnp import functional as F
    dof, split, tune, want, _ = FORWARD[name]
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', str(split))
    set_tune(monkeypatch, **tune)
    prob, p, hp = _setup(backend, FORWARD_B.get(name, 3), N, dof, bounds, seed=7)
    _has(F.launch_plan('forward', hp, S, K), **want)
    (samples, logw, props), _, _ = _forward(backend, hp, prob, dof, S, K)
    _check_logweights(prob, dof, K, samples, logw, props)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _backward_inputs(prob, dof, S, seed=5):
    """the pattern of test_backward_matches_autograd_of_oracle_at_fixed_samples: a pose behind the camera, a zero row of g_logw,
    a few weights of 1e-12 relative"""
    B = prob['x3d'].shape[0]
    g = torch.Generator().manual_seed(seed)
    poses = prob['pose_gt'].unsqueeze(0).repeat(S, 1, 1)
    poses[..., :3] += 0.2 * torch.randn(S, B, 3, generator=g)
    if dof == 6:
        q = poses[..., 3:] + 0.1 * torch.randn(S, B, 4, generator=g)
        poses[..., 3:] = q / q.norm(dim=-1, keepdim=True)
    else:
        poses[..., 3] += 0.3 * torch.randn(S, B, generator=g)
    poses[0, 0, 2] = -1.0
    g_logw = torch.randn(S, B, generator=g)
    g_logw[3] = 0.0
    g_logw[5:9, B - 1] *= 1e-12
    g_init = torch.randn(B, generator=g)
    return poses, g_logw, g_init


def _oracle_backward(prob, poses, g_logw, g_init):
    """fp64 autograd of orc.evaluate -> gradients w.r.t. x3d, x2d, w2d, delta"""
    leaves = [prob[k].double().clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d', 'delta')]
    ocam = _ocam64(prob)
    c_s = orc.evaluate(*leaves[:3], poses.double(), ocam, leaves[3], want_cost=True)[1]
    c_i = orc.evaluate(*leaves[:3], prob['pose_init'].double(), ocam, leaves[3], want_cost=True)[1]
    ((-c_s) * g_logw.double()).sum().add((c_i * g_init.double()).sum()).backward()
    return [t.grad for t in leaves]


def _check_backward(grads, want, N, bounded):
    """the bars of test_shape_fuzz._check"""
    for name, mine, ref in zip(('x3d', 'x2d', 'w2d', 'delta'), grads, want):
        assert bool(torch.isfinite(mine).all()), name
        if name == 'delta':      # sums of max(rho - delta, 0): a few point-poses near the threshold dominate; absolute floor
            err = (mine.cpu().double() - ref).abs().max().item()
            print(f'{name}: err {err:.3e} (bar {GRAD_TOL * ref.abs().max().item() + 1e-6 * N:.3e})')
            assert err <= GRAD_TOL * ref.abs().max().item() + 1e-6 * N, (name, err)
        else:
            # per point, relative to the tensor's largest entry; with a projection clamp a point-pose whose projection sits within
            # rounding of the bound passes its gradient in fp32 and not in fp64 (or the reverse): at most two such points
            err = (mine.cpu().double() - ref).abs().flatten(2).amax(-1) / ref.abs().max().clamp(min=1e-12)
            flips = 2 if bounded else 0
            bad = err > GRAD_TOL
            print(f'{name}: err {err.max().item():.3e}, {int(bad.sum())} points above {GRAD_TOL:g}')
            assert int(bad.sum()) <= flips and err.max().item() <= (5e-2 if flips else GRAD_TOL), (name, err.max().item(), int(bad.sum()))


def _check_fold(dev, prob, hp, args, plain, parked, S):
    """The same launch on a problem whose threshold came from AdaptiveHuberPnPCost on this w2d (epropnp_problem.delta_stats): the
    kernel's epilogue adds grad_delta * d delta / d w2d to grad_w2d -- from the rows parked in LDS, or reading back what it has
    just written.  Everything else the same bits; grad_w2d to 2e-6 of the object's largest entry (_delta_fold_case's bar)."""
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    rel = 0.5
    _, stats = F.adaptive_delta(hp.x2d, hp.w2d, rel)
    _, cam, _ = make_layer_objects(prob, dev)
    hf = F.PnPProblem(hp.x3d, hp.x2d, hp.w2d, cam, HuberPnPCost(delta=hp.delta), hp.dof).fold_delta(stats, rel)
    _has(F.launch_plan('backward', hf, S, pose_init=True, nsplit=1), parked=parked, valu=False)
    folded = F.amis_backward(hf, *args, nsplit=1)
    for a, b in zip((folded[0], folded[1], folded[3]), (plain[0], plain[1], plain[3])):
        assert torch.equal(a, b)
    want = plain[2] + (plain[3] * stats[:, 1] * (rel / (2 * hp.N)))[:, None, None]
    scale = want.abs().amax(dim=(1, 2), keepdim=True).clamp(min=1e-20)
    assert float((want - plain[2]).abs().max()) > 0
    assert ((folded[2] - want).abs() / scale).max().item() < 2e-6


# instantiation -> (tune keys, plan, [(N, dof, bounds, fold: None | 'parked' | 'readback' [with S = 800]) ...])
BACKWARD = {
    # 4 waves x 4 tiles, looping over chunks of 256 points: 256 + 44, two full chunks, a third chunk of one point
    '4x4': (dict(bwd_mfma='4,4'), dict(waves=4, tiles=4, bf16=True, valu=False, nsplit=1),
            [(N, dof, bounds, None) for N in (300, 512, 513) for dof, bounds in ((6, None), (6, 'tight'), (4, 'tight'))]
            + [(512, 6, None, 'parked'), (512, 6, None, 'readback')]),
    '4x2': (dict(bwd_mfma='4,2'), dict(waves=4, tiles=2, bf16=True, valu=False, nsplit=1),
            [(300, 6, 'tight', None), (300, 6, 'tight', 'parked'), (128, 4, 'tight', 'parked')]),
    # few objects, more than 16 tiles: 8 waves, chunks of 512 points
    '8x4': ({}, dict(waves=8, tiles=4, bf16=True, valu=False, nsplit=1),
            [(300, 6, None, None), (600, 6, None, None), (300, 6, 'tight', None), (600, 6, 'tight', None)]),
}
BACKWARD_CASES = [pytest.param(name, N, dof, bounds, fold, S, id=f'{name}-N{N}-{dof}dof-{bounds}-{fold}-S{S}')
                  for name, (_, _, shapes) in BACKWARD.items() for N, dof, bounds, fold in shapes
                  for S in ((800,) if fold == 'readback' else (32, 80))]


@pytest.mark.parametrize('name,N,dof,bounds,fold,S', BACKWARD_CASES)
def test_backward_instantiation_against_the_oracle(backend, monkeypatch, poisoned_empty, name, N, dof, bounds, fold, S):
    """The unsplit backward instantiations (few objects are dealt to several workgroups from N = 128 on, and take 8 waves beyond 16
    tiles): nsplit = 1 and the bwd_mfma knob, against fp64 autograd of the oracle at fixed samples."""
    from epropnp import functional as F
    tune, want, _ = BACKWARD[name]
    set_tune(monkeypatch, **tune)
    B = 2 if fold == 'readback' else 3
    prob, p, hp = _setup(backend, B, N, dof, bounds, seed=11)
    _has(F.launch_plan('backward', hp, S, pose_init=True, nsplit=1), parked=False, **want)
    poses, g_logw, g_init = _backward_inputs(prob, dof, S)
    args = (poses.to(backend), g_logw.to(backend), p['pose_init'], g_init.to(backend))
    grads = F.amis_backward(hp, *args, nsplit=1)
    again = F.amis_backward(hp, *args, nsplit=1)
    for a, b in zip(grads, again):
        assert torch.equal(a, b)
    _check_backward(grads, _oracle_backward(prob, poses, g_logw, g_init), N, bounds is not None)
    if fold is not None:
        _check_fold(backend, prob, hp, args, grads, fold == 'parked', S)


def test_backward_epilogue_reads_grad_w2d_back(backend, monkeypatch):
    """Three workgroups' pose tables of 800 samples plus the rows of 512 points exceed 160 KiB: the epilogue of the unsplit kernel
    reads grad_w2d back instead of parking its rows in LDS -- the arm that the C5 shard takes (1024 samples, 2048 points).  Through
    the layer, against autograd through the AdaptiveDelta node (EPROPNP_DELTA_FOLD=0)."""
    from epropnp import functional as F
    from test_fused_and_limits import _delta_fold_case
    monkeypatch.setenv('EPROPNP_BWD_SPLIT', '1')
    plan = F.launch_plan('backward', F.PlanProblem(2, 512, 6, delta_fold=True), 800, pose_init=True)
    _has(plan, nsplit=1, waves=8, tiles=4, parked=False, valu=False)
    _delta_fold_case(backend, monkeypatch, 6, 2, 512, 800, 2, None, False, nsplit_env='1')


# ---------------------------------------------------------------------------------------------------------------------------------
# cost sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def _cost_poses(prob, P, seed=5):
    g = torch.Generator().manual_seed(seed)
    B = prob['x3d'].shape[0]
    poses = prob['pose_init'].unsqueeze(0).repeat(P, 1, 1)
    poses[1:, :, :3] += 0.05 * torch.randn(P - 1, B, 3, generator=g)
    weights = torch.randn(P, B, generator=g)
    return poses, weights


def _check_cost(prob, poses, cost):
    """rtol 2e-5 / atol 1e-5 against the fp64 oracle: the bar of test_evaluate_cost_matches_reference"""
    ref = orc.evaluate(prob['x3d'].double(), prob['x2d'].double(), prob['w2d'].double(), poses.double(), _ocam64(prob),
                       prob['delta'].double(), want_cost=True)[1]
    torch.testing.assert_close(cost.cpu().double(), ref, rtol=2e-5, atol=1e-5)


def _check_pose_cam_grad(prob, dof, poses, weights, m, gp, gk):
    """per object relative to the object's largest entry, 2e-4: the bar of tests/test_pose_cam_grad.py"""
    from test_pose_cam_grad import _oracle_grads
    B = poses.shape[1]
    ref_p, ref_k, _ = _oracle_grads(prob, dof, poses, weights, 'bounded' if 'lb' in prob else None)
    for mine, ref in ((gp, ref_p[m]), (gk, ref_k)):
        err = (mine.cpu().double() - ref).abs().reshape(B, -1).amax(1) / ref.abs().reshape(B, -1).amax(1).clamp(min=1e-12)
        assert err.max().item() <= 2e-4, (m, err)


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('dof,bounds', [(6, None), (4, 'tight'), (6, 'tight')])
@pytest.mark.parametrize('shape,N', [('1,2', 65), ('1,2', 128), ('1,4', 200), ('1,8', 449), ('1,8', 512), ('2,4', 449), ('2,4', 512),
                                     ('4,8', 1800), ('4,8', 2048)])       # (4 x 8: what the C5 shard takes)
def test_cost_sweep_fat_lanes_against_the_oracle(backend, monkeypatch, poisoned_empty, shape, N, dof, bounds, P):
    """evaluate_cost with 2 / 4 / 8 points per lane, which it takes from 4096 waves' worth of objects on (ev_shape reaches them with
    three objects), and cost_pose_cam_grad at the same shapes (its block size follows N alone)."""
    from epropnp import functional as F
    set_tune(monkeypatch, ev_shape=shape)
    waves, ppl = (int(v) for v in shape.split(','))
    prob, p, hp = _setup(backend, 3, N, dof, bounds, seed=31)
    assert F.launch_plan('cost', hp) == dict(waves=waves, ppl=ppl)
    poses, weights = _cost_poses(prob, P)
    cost = F.evaluate_cost(hp, poses.to(backend))
    assert torch.equal(cost, F.evaluate_cost(hp, poses.to(backend)))
    _check_cost(prob, poses, cost)
    m = P - 1
    gp, gk = F.pose_cam_grad(hp, poses.to(backend), weights.to(backend), m_pose=m)
    _check_pose_cam_grad(prob, dof, poses, weights, m, gp, gk)


def test_ev_shape_is_ignored_when_invalid(backend, monkeypatch):
    """the rule of ne_shape / lm_shape: a shape that is not instantiated or does not cover the object changes nothing"""
    from epropnp import functional as F
    prob, p, hp = _setup(backend, 3, 200, 6, None, seed=31)
    set_tune(monkeypatch)
    default = F.launch_plan('cost', hp)
    for bad in ('1,2', '3,4', '1,16', '0,8'):            # 128 < 200 points; 3 waves; 16 points per lane; no wave
        set_tune(monkeypatch, ev_shape=bad)
        assert F.launch_plan('cost', hp) == default
    set_tune(monkeypatch, ev_shape='2,2')
    assert F.launch_plan('cost', hp) == dict(waves=2, ppl=2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the defaults at the batch sizes that choose these instantiations (GPU only, no knob), and the same objects as a batch of 16
# ---------------------------------------------------------------------------------------------------------------------------------
EDGE = list(range(8)) + list(range(-8, 0))       # the oracle runs on the first and the last eight objects


def _same_but_grid(big, small, keys):
    return all(big[k] == small[k] for k in keys)


@pytest.mark.gpu
@pytest.mark.parametrize('N,tune,want', [(500, dict(fwd_mfma='4,8'), dict(waves=4, tiles=8, G=1, chunks=1, chunked=False)),
                                          (300, dict(fwd_mfma='2,12'), dict(waves=2, tiles=12, G=1, chunks=1, chunked=False)),
                                          (769, {}, dict(waves=4, tiles=8, G=1, chunks=2, chunked=True))])
def test_forward_defaults_at_512_objects(monkeypatch, poisoned_empty, N, tune, want):
    """From 512 objects on the defaults take 4 waves x 8 tiles for 25...32 point tiles (N = 500; C2's kernel) -- for the 19 tiles
    of N = 300 the least padding is 2 waves x 12 tiles, which only this case launches -- and two chunks at N = 769."""
    import install as emu
    emu.uninstall()
    from epropnp import functional as F
    dev = torch.device('cuda:0')
    B, S, K, dof = 512, 32, 2, 6
    monkeypatch.delenv('EPROPNP_FWD_SPLIT', raising=False)
    set_tune(monkeypatch)
    prob, p, hp = _setup(dev, B, N, dof, None, seed=61)
    big_plan = F.launch_plan('forward', hp, S, K)
    _has(big_plan, bf16=True, spilled=False, **want)
    (samples, logw, props), noise, (pose_opt, pose_cov) = _forward(dev, hp, prob, dof, S, K)
    sub = _take(prob, EDGE)
    _check_logweights(sub, dof, K, samples[:, EDGE], logw[:, EDGE], props[EDGE])
    # the same sixteen objects as a batch of their own, under the knobs of the matrix above: the same kernel, another grid
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    set_tune(monkeypatch, **tune)
    _, _, hs = _setup_from(sub, dev, dof)
    small_plan = F.launch_plan('forward', hs, S, K)
    assert small_plan == big_plan, (small_plan, big_plan)
    (s2, w2, p2), _, _ = _forward(dev, hs, sub, dof, S, K, noise=noise[EDGE].contiguous(),
                                  lm=(pose_opt[EDGE].contiguous(), pose_cov[EDGE].contiguous()))
    assert torch.equal(s2, samples[:, EDGE]) and torch.equal(w2, logw[:, EDGE]) and torch.equal(p2, props[EDGE])


def _setup_from(prob, dev, dof):
    from epropnp import functional as F
    p, cam, cf = make_layer_objects(prob, dev)
    return prob, p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)


@pytest.mark.gpu
@pytest.mark.parametrize('bounds,tiles', [(None, 4), ('tight', 2)])
def test_backward_defaults_at_512_objects(monkeypatch, poisoned_empty, bounds, tiles):
    """4 x 4 without a projection clamp; with one, 4 x 2 from two objects per CU on.  "Which projection arithmetic an object gets
    must not depend on how many objects share the launch" (launcher comment): the same sixteen objects alone, same bits."""
    import install as emu
    emu.uninstall()
    from epropnp import functional as F
    dev = torch.device('cuda:0')
    B, N, S, dof = 512, 300, 32, 6
    monkeypatch.delenv('EPROPNP_BWD_SPLIT', raising=False)
    set_tune(monkeypatch)
    prob, p, hp = _setup(dev, B, N, dof, bounds, seed=63)
    big_plan = F.launch_plan('backward', hp, S, pose_init=True)
    _has(big_plan, waves=4, tiles=tiles, bf16=True, valu=False, nsplit=1, parked=False)
    poses, g_logw, g_init = _backward_inputs(prob, dof, S)
    grads = F.amis_backward(hp, poses.to(dev), g_logw.to(dev), p['pose_init'], g_init.to(dev))
    sub = _take(prob, EDGE)
    want = _oracle_backward(sub, poses[:, EDGE], g_logw[:, EDGE], g_init[EDGE])
    _check_backward([g[EDGE] for g in grads], want, N, bounds is not None)
    set_tune(monkeypatch, bwd_mfma=f'4,{tiles}')
    _, ps, hs = _setup_from(sub, dev, dof)
    small_plan = F.launch_plan('backward', hs, S, pose_init=True, nsplit=1)
    assert small_plan == big_plan, (small_plan, big_plan)
    small = F.amis_backward(hs, poses[:, EDGE].contiguous().to(dev), g_logw[:, EDGE].contiguous().to(dev), ps['pose_init'],
                            g_init[EDGE].to(dev), nsplit=1)
    for a, b in zip(small[:3], grads[:3]):
        assert torch.equal(a, b[EDGE])


@pytest.mark.gpu
def test_cost_sweep_defaults_at_4096_objects(monkeypatch, poisoned_empty):
    import install as emu
    emu.uninstall()
    from epropnp import functional as F
    dev = torch.device('cuda:0')
    B, N, P, dof = 4096, 512, 5, 6
    set_tune(monkeypatch)
    prob, p, hp = _setup(dev, B, N, dof, None, seed=65)
    assert F.launch_plan('cost', hp) == dict(waves=1, ppl=8)
    poses, _ = _cost_poses(prob, P)
    cost = F.evaluate_cost(hp, poses.to(dev))
    sub = _take(prob, EDGE)
    _check_cost(sub, poses[:, EDGE], cost[:, EDGE])
    set_tune(monkeypatch, ev_shape='1,8')
    _, _, hs = _setup_from(sub, dev, dof)
    assert F.launch_plan('cost', hs) == dict(waves=1, ppl=8)
    assert torch.equal(F.evaluate_cost(hs, poses[:, EDGE].contiguous().to(dev)), cost[:, EDGE])


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage gate: every instantiation that a BASELINE shape launches on a 256-CU device is one that a test above (or a named
# existing test) launches and holds against the oracle.  Host only: launch_plan(..., cus=256) runs on any build.
# ---------------------------------------------------------------------------------------------------------------------------------
CUS = 256
FWD_KEYS = ('waves', 'tiles', 'G', 'chunks', 'bf16', 'spilled', 'truncated', 'chunked')
BWD_KEYS = ('waves', 'tiles', 'bf16', 'parked', 'valu', 'nsplit')

# BASELINE shape -> (B, N, S, K, dof, bounded).  Every one of them takes its threshold from AdaptiveHuberPnPCost (bench.py), so
# the backward folds the threshold's gradient.  C4 at one GPU (600 objects) and as an eighth (75 objects per GPU).
SHAPES = {
    'C2': (4096, 512, 512, 4, 6, False),
    'C2-bounded': (4096, 512, 512, 4, 6, True),
    'C3-train': (32, 512, 512, 4, 6, True),
    'C3-dense': (32, 4096, 512, 4, 6, True),
    'C4': (600, 128, 128, 4, 4, True),
    'C4/8': (75, 128, 128, 4, 4, True),
    'C5-shard': (8192, 2048, 1024, 4, 6, False),
}
# (shape, kind) -> the test that holds this instantiation (template arguments: dof, projection clamp, tiles, variant) against the
# oracle, and how it launches: (B, N, S, K, dof, bounded, environment, tune keys)
_F = 'test_forward_instantiation_against_the_oracle'
_B = 'test_backward_instantiation_against_the_oracle'
_D = 'test_fused_and_limits::test_delta_gradient_folded_into_the_backward_kernel_gpu'
_S1 = {'EPROPNP_FWD_SPLIT': '1'}
COVERED_BY = {
    ('C2', 'forward'): (f'{_F}[4x8-N512-None]', (3, 512, 32, 2, 6, False, _S1, dict(fwd_mfma='4,8'))),
    ('C2-bounded', 'forward'): (f'{_F}[4x8-N512-tight]', (3, 512, 32, 2, 6, True, _S1, dict(fwd_mfma='4,8'))),
    ('C3-train', 'forward'): (f'{_F}[split-4x2-N512-tensor]', (3, 512, 32, 2, 6, True, {'EPROPNP_FWD_SPLIT': '4'}, {})),
    ('C3-dense', 'forward'): (f'{_F}[split-4x8-N2100-tensor]', (1, 2100, 32, 2, 6, True, {'EPROPNP_FWD_SPLIT': '8'}, {})),
    ('C4', 'forward'): (f'{_F}[4x2-4dof-N128-tensor]', (3, 128, 32, 2, 4, True, _S1, {})),
    ('C4/8', 'forward'): (f'{_F}[4x2-4dof-N128-tensor]', (3, 128, 32, 2, 4, True, _S1, {})),
    ('C5-shard', 'forward'): (f'{_F}[chunked-4-N2048-None]', (3, 2048, 32, 2, 6, False, _S1, {})),
    ('C2', 'backward'): (f'{_B}[4x4-N512-6dof-None-parked]', (3, 512, 32, 0, 6, False, {'nsplit': 1}, dict(bwd_mfma='4,4'))),
    ('C2-bounded', 'backward'): (f'{_B}[4x2-N300-6dof-tight-parked]', (3, 300, 32, 0, 6, True, {'nsplit': 1}, dict(bwd_mfma='4,2'))),
    ('C3-train', 'backward'): (f'{_D}[6-32-512-128-4-tensor]', (32, 512, 128, 0, 6, True, {}, {})),
    ('C4', 'backward'): (f'{_B}[4x2-N128-4dof-tight-parked]', (3, 128, 32, 0, 4, True, {'nsplit': 1}, dict(bwd_mfma='4,2'))),
    ('C4/8', 'backward'): (f'{_D}[4-40-128-64-2-tensor-True-2]', (40, 128, 64, 0, 4, True, {'nsplit': 2}, {})),
    ('C5-shard', 'backward'): (f'{_B}[4x4-N512-6dof-None-readback-S800]', (2, 512, 800, 0, 6, False, {'nsplit': 1}, dict(bwd_mfma='4,4'))),
    ('C2', 'cost'): ('test_cost_sweep_fat_lanes_against_the_oracle[1,8-512-6-None]', (3, 512, 0, 0, 6, False, {}, dict(ev_shape='1,8'))),
    ('C5-shard', 'cost'): ('test_cost_sweep_fat_lanes_against_the_oracle[4,8-2048-6-None]', (3, 2048, 0, 0, 6, False, {}, dict(ev_shape='4,8'))),
    ('C2-bounded', 'cost'): ('test_cost_sweep_fat_lanes_against_the_oracle[1,8-512-6-tight]', (3, 512, 0, 0, 6, True, {}, dict(ev_shape='1,8'))),
}
NOT_LAUNCHED = {('C3-dense', 'backward')}      # the dense LineMOD shape is an inference call


def _plan_of(monkeypatch, kind, B, N, S, K, dof, bounded, env, tune):
    from epropnp import functional as F
    for k in ('EPROPNP_FWD_SPLIT', 'EPROPNP_BWD_SPLIT', 'EPROPNP_FWD_PROJ', 'EPROPNP_BWD_PROJ'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if k.startswith('EPROPNP_'):
            monkeypatch.setenv(k, v)
    set_tune(monkeypatch, **tune)
    pp = F.PlanProblem(B, N, dof, bounds=bounded, delta_fold=True)
    if kind == 'forward':
        plan = F.launch_plan('forward', pp, S, K, cus=CUS)
        plan['G'] = min(plan['G'], 2)                    # (split or not: how many parts is the grid)
        return {k: plan[k] for k in FWD_KEYS}
    if kind == 'backward':
        plan = F.launch_plan('backward', pp, S, pose_init=True, nsplit=env.get('nsplit'), cus=CUS)
        plan['nsplit'] = min(plan['nsplit'], 2)
        return {k: plan[k] for k in BWD_KEYS}
    return F.launch_plan('cost', pp, cus=CUS)


@pytest.mark.parametrize('kind', ['forward', 'backward', 'cost'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_baseline_shapes_launch_covered_instantiations(backend, monkeypatch, shape, kind):
    """`backend`: the emulation build answers the query as the HIP build does (the same host functions)."""
    B, N, S, K, dof, bounded = SHAPES[shape]
    if (shape, kind) in NOT_LAUNCHED:
        return
    mine = _plan_of(monkeypatch, kind, B, N, S, K, dof, bounded, {}, {})
    if kind == 'cost' and mine == _plan_of(monkeypatch, kind, 3, N, S, K, dof, bounded, {}, {}):
        return            # the shape follows from N alone: what every test of evaluate_cost at this N launches at a few objects
    assert (shape, kind) in COVERED_BY, f'{shape} {kind} launches {mine}: name the test that holds this instantiation to the oracle'
    test_id, (cB, cN, cS, cK, cdof, cbnd, env, tune) = COVERED_BY[(shape, kind)]
    theirs = _plan_of(monkeypatch, kind, cB, cN, cS, cK or 1, cdof, cbnd, env, tune)
    assert (dof, bounded) == (cdof, cbnd), (shape, test_id)
    assert mine == theirs, f'{shape} {kind} launches {mine}, {test_id} launches {theirs}'


def test_launch_plan_reads_the_cu_count(backend, monkeypatch):
    """the explicit CU count is what decides: the bounded backward takes two tiles from two objects per CU on, the forward splits
    while a workgroup per part fits the device"""
    from epropnp import functional as F
    set_tune(monkeypatch)
    monkeypatch.delenv('EPROPNP_FWD_SPLIT', raising=False)
    pp = F.PlanProblem(512, 300, 6, bounds=True)
    assert F.launch_plan('backward', pp, 32, pose_init=True, cus=256)['tiles'] == 2
    assert F.launch_plan('backward', pp, 32, pose_init=True, cus=304)['tiles'] == 4
    few = F.PlanProblem(32, 512, 6)
    assert F.launch_plan('forward', few, 512, 4, cus=256)['G'] == 4
    assert F.launch_plan('forward', few, 512, 4, cus=64)['G'] == 1
    assert F.launch_plan('forward', few, 512, 4, cus=256, scratch=False)['G'] == 1
    with pytest.raises(ValueError):
        F.launch_plan('sweep', few)
