"""Fused LM / GN kernel vs the reference's LMSolver.solve (golden fixtures) and vs the oracle on seeded problems."""
import pytest
import torch

import epropnp_oracle as orc
from helpers import assert_within_spread, load_golden, make_layer_objects, rel_per_object

POSE_TOL = 1e-4      # north-star tolerance on the pose


def _solve(backend, g, prob_dict=None):
    from epropnp.levenberg_marquardt import LMSolver
    dof = int(g['dof'])
    p, cam, cf = make_layer_objects(prob_dict or g['prob'], backend)
    solver = LMSolver(dof=dof, num_iter=int(g['lm_iter']))
    return solver.solve(p['x3d'], p['x2d'], p['w2d'], cam, cf, pose_init=p['pose_init'], with_pose_cov=True,
                        with_cost=True, fast_mode=bool(g['fast_mode']))


@pytest.mark.parametrize('name', ['lm6_tr', 'lm6_gn', 'lm6_tr_clip', 'lm4_tr', 'lm4_gn'])
def test_lm_matches_reference(backend, name):
    """pose <= 1e-4, cost <= 1e-5 rel, covariance <= 1e-3 rel of the reference -- each bar widened only by the
    reference's OWN rounding sensitivity (fixture `spread.*`: max change of the reference's fp32 result under <= 3 ulp
    input perturbations, plus its fp32-vs-fp64 drift), matched by rank over the objects.  That yardstick is what a
    trust-region accept/reject flip at convergence (a 1-ulp effect on `cost - cost_new`, SURVEY.md section 7 hard part
    2) looks like from outside: no accept-history bookkeeping, no equal-cost escape."""
    from epropnp import functional as F
    g = load_golden(name)
    dof = int(g['dof'])
    p, cam, cf = make_layer_objects(g['prob'], backend)
    prob = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)
    pose, cov, cost = F.lm_solve(prob, p['pose_init'], int(g['lm_iter']), fast_mode=bool(g['fast_mode']),
                                 with_pose_cov=True, with_cost=True)
    pose, cov, cost, sp = pose.cpu(), cov.cpu(), cost.cpu(), g['spread']
    assert_within_spread((pose - g['pose_opt']).abs().max(-1).values, sp['pose_opt'], POSE_TOL, what='pose_opt')
    assert_within_spread((cost - g['cost']).abs() / g['cost'].abs().clamp(min=1e-30), sp['cost'], 1e-5, what='cost')
    assert_within_spread(rel_per_object(cov, g['pose_cov']), sp['pose_cov'], 1e-3, what='pose_cov')


def test_lm_accept_history_matches_reference(backend):
    from epropnp import functional as F
    g = load_golden('lm6_tr')
    p, cam, cf = make_layer_objects(g['prob'], backend)
    prob = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, 6)
    _, _, _, acc = F.lm_solve(prob, p['pose_init'], int(g['lm_iter']), with_accepts=True)
    ref_bits = (g['accepts'].long() << torch.arange(g['accepts'].shape[0])[:, None]).sum(0)
    # decisions on the first three (non-marginal) steps must agree; later steps run at convergence where
    # cost - cost_new is rounding noise and either decision is legitimate
    first = (acc.cpu().long() & 7) == (ref_bits & 7)
    assert bool(first.all()), (acc, ref_bits)


@pytest.mark.parametrize('dof,N,lm_iter,fast', [(6, 512, 3, False), (6, 200, 4, True), (4, 128, 5, False),
                                                 (6, 1100, 3, False), (4, 64, 10, True)])
def test_lm_vs_oracle_seeded(backend, dof, N, lm_iter, fast):
    """Sizes beyond the fixtures (multi-wave objects, ragged N) against the restatement run here, fp32 and fp64."""
    from epropnp import functional as F
    B = 3 if N > 600 else 5
    prob = orc.make_problem(B, N, dof, seed=100 + N)
    p, cam, cf = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)
    pose, _, cost = F.lm_solve(hp, p['pose_init'], lm_iter, fast_mode=fast, with_cost=True)
    pose, cost = pose.cpu(), cost.cpu()

    def run(q, dt=torch.float32):
        q = {k: v.to(dt) for k, v in q.items()}
        out = orc.lm_solve(q['x3d'], q['x2d'], q['w2d'], orc.Cam(q['cam_mats'], 0.1), q['delta'], q['pose_init'],
                           fast_mode=fast, with_pose_cov=True, with_cost=True, num_iter=lm_iter)
        return dict(pose_opt=out[0].float(), cost=out[2].float())
    base = run(prob)
    sp = orc.rounding_spread(run, prob, base, extra=[run(prob, torch.float64)])
    assert_within_spread((pose - base['pose_opt']).abs().max(-1).values, sp['pose_opt'], POSE_TOL, what='pose_opt')
    assert_within_spread((cost - base['cost']).abs() / base['cost'].abs().clamp(min=1e-30), sp['cost'], 1e-5, what='cost')


def test_lm_empty_batch(backend):
    from epropnp.camera import PerspectiveCamera
    from epropnp.cost_fun import HuberPnPCost
    from epropnp.levenberg_marquardt import LMSolver
    z = lambda *s: torch.zeros(*s, device=backend)
    pose, cov, cost = LMSolver(dof=6, num_iter=3).solve(z(0, 16, 3), z(0, 16, 2), z(0, 16, 2),
                                                        PerspectiveCamera(cam_mats=z(0, 3, 3)), HuberPnPCost(),
                                                        pose_init=z(0, 7), with_pose_cov=True, with_cost=True)
    assert pose.shape == (0, 7) and cov.shape == (0, 6, 6) and cost.shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize('dof,bounds,B,N,lm_iter,fast', [(6, None, 32, 4096, 5, False), (6, 'tensor', 32, 4096, 3, True),
                                                         (4, 'tensor', 16, 2500, 5, False), (6, 'tight', 5, 3000, 4, False),
                                                         (6, None, 8, 8192, 10, False), (4, None, 7, 6000, 1, True)])
def test_lm_split_over_workgroups(monkeypatch, dof, bounds, B, N, lm_iter, fast):
    """Few objects x many points: the points of an object are dealt to up to 8 workgroups that exchange their partial normal
    equations after every sweep (csrc/lm_kernel.hip, SPLIT).  Against the one-workgroup kernel (same decisions, sums in
    another order), against the oracle, bit-reproducible, and twice at once on two streams."""
    import install as emu
    emu.uninstall()
    from epropnp import functional as F
    dev = torch.device('cuda:0')
    prob = orc.make_problem(B, N, dof, seed=300 + N, bounds=bounds)
    p, cam, cf = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)
    kw = dict(fast_mode=fast, with_pose_cov=True, with_cost=True)
    par = F._hip.LmParams(lm_iter, int(fast), 1e-6, 1e32, 1e-3, 30.0, 1e16, 1e-5)
    assert F.lm_split_scratch(hp, par) is not None, 'this shape is meant to take the split'
    monkeypatch.setenv('EPROPNP_LM_SPLIT', '1')
    one = F.lm_solve(hp, p['pose_init'], lm_iter, **kw)
    monkeypatch.delenv('EPROPNP_LM_SPLIT')
    outs = [F.lm_solve(hp, p['pose_init'], lm_iter, **kw) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    pose, cov, cost = (t.cpu() for t in outs[0])

    def run(q, dt=torch.float32):
        q = {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in q.items()}
        out = orc.lm_solve(q['x3d'], q['x2d'], q['w2d'], orc.Cam(q['cam_mats'], 0.1, q.get('lb'), q.get('ub')), q['delta'],
                           q['pose_init'], fast_mode=fast, with_pose_cov=True, with_cost=True, num_iter=lm_iter)
        return dict(pose_opt=out[0].float(), cost=out[2].float())
    base = run(prob)
    sp = orc.rounding_spread(run, prob, base, extra=[run(prob, torch.float64), dict(pose_opt=one[0].cpu(), cost=one[2].cpu())])
    assert_within_spread((pose - base['pose_opt']).abs().max(-1).values, sp['pose_opt'], POSE_TOL, what='pose_opt')
    assert_within_spread((cost - base['cost']).abs() / base['cost'].abs().clamp(min=1e-30), sp['cost'], 1e-5, what='cost')
    assert bool(torch.isfinite(cov).all())
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    both = []
    for q in st:
        q.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(q):
            both.append(F.lm_solve(hp, p['pose_init'], lm_iter, **kw))
    torch.cuda.synchronize()
    F.flush_status()
    assert all(torch.equal(o[0], outs[0][0]) for o in both)


@pytest.mark.parametrize('dof,bounds,N,G,fast', [(6, None, 300, 4, False), (4, 'tight', 200, 2, False), (6, 'tensor', 520, 8, True)])
def test_lm_split_recomputes_missing_parts(backend, monkeypatch, dof, bounds, N, G, fast):
    """The split LM solve never depends on its sibling workgroups being resident: a part whose partial normal equations are
    not there within EPROPNP_SPLIT_TIMEOUT_CYCLES is recomputed from its points by the same lanes in the same order.
    On the CPU emulation workgroups run one after another, so EVERY later part is missing for the earlier ones: the whole
    solve then goes through the recomputation path and must match the one-workgroup kernel to summation order.  On the GPU
    a zero timeout forces the path wherever a sibling is not there at the first look: bit-identical to the patient run.
    Against the one-workgroup kernel the GPU run is held to the strict form -- the same accept / reject history for every object,
    pose and covariance compared for every object; only the emulation may let one object part ways at an equal cost."""
    from epropnp import functional as F
    B, L = 3, 4
    prob = orc.make_problem(B, N, dof, seed=77, bounds=bounds)
    p, cam, cf = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)
    kw = dict(fast_mode=fast, with_pose_cov=True, with_cost=True, with_accepts=True)
    monkeypatch.setenv('EPROPNP_LM_SPLIT', '1')
    one = F.lm_solve(hp, p['pose_init'], L, **kw)
    monkeypatch.setenv('EPROPNP_LM_SPLIT', str(G))
    par = F._hip.LmParams(L, int(fast), 1e-6, 1e32, 1e-3, 30.0, 1e16, 1e-5)
    assert F.lm_split_scratch(hp, par) is not None
    many = F.lm_solve(hp, p['pose_init'], L, **kw)
    # the same accept / reject history -- except that a step of an already converged object changes the cost by rounding only
    # and is taken or not by the summation order: such an object may part ways, at an equal cost
    same = many[3] == one[3]
    assert int(same.sum()) >= (B if backend.type == 'cuda' else B - 1) and _close(many[2], one[2], 2e-5)
    assert (many[0] - one[0])[same].abs().max().item() <= 2e-5
    assert _close(many[1][same], one[1][same], 2e-3)
    if backend.type == 'cuda':
        monkeypatch.setenv('EPROPNP_SPLIT_TIMEOUT_CYCLES', '0')
        hasty = F.lm_solve(hp, p['pose_init'], L, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(hasty, many))


def _close(a, b, rel):
    return bool(((a - b).abs() <= rel * b.abs().clamp(min=1e-30) + 1e-30).all()) if a.dim() == 1 else \
        bool((a - b).abs().max() <= rel * b.abs().max())
