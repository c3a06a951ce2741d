"""Per-object, general camera matrices through every PnP kernel.

Every other seeded test, fixture and the benchmark expand ONE pinhole matrix (or the identity) over the batch, so a camera or
bound read for the wrong object, the same mistake in the host code, or a kernel that assumes pinhole structure (K[0,1] = K[1,0] = 0,
third row (0,0,1), fx = fy > 0) would pass them all.  Here every object has its own matrix (helpers.vary_cameras): independent
focal lengths and principal points ('per_object'), skew and a horizontal flip on top ('skewed'), a general matrix with a
non-trivial third row and its own scale ('full').  The expected values come from the fp64 oracle, whose arithmetic is the
reference's for any (*,3,3) matrix (epropnp/camera.py:10-30,111-143); the bars are those of each entry point's existing test."""
import functools

import pytest
import torch

import epropnp_oracle as orc
from helpers import CAMERA_KINDS, assert_within_spread, make_layer_objects, pack_noise, rel_per_object, set_tune, vary_cameras
from test_amis import _mixture_logq
from test_pose_cam_grad import _oracle_grads

CASES = [(6, None), (4, 'tight'), (6, 'tight')]          # (dof, bounds); vary_cameras turns the box into per-object quantiles
kinds_and_cases = lambda f: pytest.mark.parametrize('kind', CAMERA_KINDS)(pytest.mark.parametrize('dof,bounds', CASES)(f))


@functools.lru_cache(maxsize=None)
def _problem(B, N, dof, bounds, kind, seed=0):
    """shared between the tests and never modified"""
    return vary_cameras(orc.make_problem(B, N, dof, seed=500 + seed + N, bounds=bounds), kind, seed=900 + seed + B)


def _f64(prob):
    return {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in prob.items()}


def _ocam(q, z_min=0.1):
    return orc.Cam(q['cam_mats'], z_min, q.get('lb'), q.get('ub'))


def _hip_problem(prob, backend, dof):
    from epropnp import functional as F
    p, cam, cf = make_layer_objects(prob, backend)
    return p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)


EDGE_PX = 1e-3        # ~16 ulp of a 500-pixel coordinate: no correct fp32 projection lands on the other side


def _edge_margin(prob, poses):
    """Smallest distance, per pose (*,B), of an unclipped projection to the bounds it is clamped at (pixels) and of a depth to
    z_min (relative, in units of 1e-6).  The gradients (not the cost) jump where a projection crosses a bound: a test that
    compares them must keep its inputs off those edges, where the side fp32 lands on is decided by rounding.  (Found with the
    'skewed' 4-DoF bounded problem: one of 30000 projections lay 1e-4 pixels -- 2 ulp -- inside its lower bound, the kernels
    clipped it, the fp32 and fp64 oracles did not, and the gradient to x3d was off by 2.8e-4 of its largest entry on every path.)"""
    q = _f64(prob)
    K, ps = q['cam_mats'], poses.double()
    h = q['x3d'] @ (K @ orc.pose_to_rotmat(ps)).transpose(-1, -2) + (K @ ps[..., :3, None]).squeeze(-1).unsqueeze(-2)
    m = (h[..., 2] - 0.1).abs().amin(-1) / 0.1 * 1e6 * EDGE_PX
    if 'lb' in q:
        p = h[..., :2] / h[..., 2:3].clamp(min=0.1)
        m = torch.minimum(m, torch.minimum((p - q['lb'].unsqueeze(-2)).abs(), (p - q['ub'].unsqueeze(-2)).abs()).amin(dim=(-1, -2)))
    return m


def _poses_around(prob, dof, P, seed, spread=1.0):
    """(P,B,pose_len) poses scattered about pose_gt, the first one behind the camera for object 0 (z clamp active); a pose with
    a projection within EDGE_PX of a bound is drawn again (_edge_margin)"""
    g = torch.Generator().manual_seed(seed)
    B = prob['x3d'].shape[0]

    def draw():
        poses = prob['pose_gt'].unsqueeze(0).repeat(P, 1, 1)
        poses[..., :3] += 0.2 * spread * torch.randn(P, B, 3, generator=g)
        if dof == 6:
            q = poses[..., 3:] + 0.1 * spread * torch.randn(P, B, 4, generator=g)
            poses[..., 3:] = q / q.norm(dim=-1, keepdim=True)
        else:
            poses[..., 3] += 0.3 * spread * torch.randn(P, B, generator=g)
        return poses
    poses = draw()
    poses[0, 0, 2] = -1.0
    for _ in range(8):
        near = _edge_margin(prob, poses) < EDGE_PX
        if not bool(near.any()):
            return poses
        poses[near] = draw()[near]
    raise AssertionError('no poses off the clipping edges')


def _pose_init_off_the_edges(prob):
    assert float(_edge_margin(prob, prob['pose_init']).min()) >= EDGE_PX, 'pose_init projects a point onto a bound: take another seed'


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-12)).item()


# ----------------------------------------------------------------------------------------------------------------------
# sweeps: B = 7, N = 150 (three waves' worth of points, ragged; 7 objects: the swizzle's remainder rows only)
# ----------------------------------------------------------------------------------------------------------------------


@kinds_and_cases
def test_evaluate_cost(backend, kind, dof, bounds):
    """bar: test_sweep_kernels.test_evaluate_cost_matches_reference (rtol 2e-5, atol 1e-5)"""
    from epropnp import functional as F
    prob = _problem(7, 150, dof, bounds, kind)
    p, hp = _hip_problem(prob, backend, dof)
    poses = _poses_around(prob, dof, 5, seed=1)
    q = _f64(prob)
    want = orc.evaluate(q['x3d'], q['x2d'], q['w2d'], poses.double(), _ocam(q), q['delta'], want_cost=True)[1]
    got = F.evaluate_cost(hp, poses.to(backend)).cpu().double()
    print(f'cost {kind} dof={dof} bounds={bounds}: rel err {((got - want).abs() / want.abs()).max().item():.3e}')
    torch.testing.assert_close(got, want, rtol=2e-5, atol=1e-5)


@kinds_and_cases
def test_normal_equations(backend, kind, dof, bounds):
    """bars: test_sweep_kernels.test_normal_equations_launch_shapes_agree (jtj 2e-5, jtr 1e-4 of the object's largest entry,
    cost 1e-5 rel)"""
    from epropnp import functional as F
    prob = _problem(7, 150, dof, bounds, kind)
    _pose_init_off_the_edges(prob)
    p, hp = _hip_problem(prob, backend, dof)
    q = _f64(prob)
    res, cost, jac = orc.evaluate(q['x3d'], q['x2d'], q['w2d'], q['pose_init'], _ocam(q), q['delta'], True, True, clip_jac=True)
    jtj = jac.transpose(-1, -2) @ jac
    jtr = (jac.transpose(-1, -2) @ res.unsqueeze(-1)).squeeze(-1)
    a, b, c = (t.cpu().double() for t in F.normal_equations(hp, p['pose_init'], clip_jac=True))
    e_jtj = ((a - jtj).abs() / jtj.abs().amax(dim=(-1, -2), keepdim=True)).max().item()
    e_jtr = ((b - jtr).abs() / jtr.abs().amax(-1, keepdim=True).clamp(min=1e-3)).max().item()
    print(f'normal equations {kind} dof={dof} bounds={bounds}: jtj {e_jtj:.3e} jtr {e_jtr:.3e} '
          f'cost {((c - cost).abs() / cost.abs()).max().item():.3e}')
    assert e_jtj < 2e-5 and e_jtr < 1e-4
    torch.testing.assert_close(c, cost, rtol=1e-5, atol=1e-6)


def _gn_oracle(prob, pose, gvec, plus):
    q = _f64(prob)
    leaves = {k: q[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d', 'delta')}
    out = orc.gn_step(leaves['x3d'], leaves['x2d'], leaves['w2d'], pose.double(), _ocam(q), leaves['delta'])
    if plus:
        out = orc.pose_add(pose.double(), out)
    (out * gvec.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize('plus', [False, True], ids=['gn_step', 'pose_opt_plus'])
@kinds_and_cases
def test_gn_step_and_pose_opt_plus(backend, kind, dof, bounds, plus):
    """bars: test_gn_step.test_gn_step_forward_backward (step 5e-4 of the object's largest entry, input gradients 2e-3);
    pose_opt_plus = pose_add(pose, step) is held to the same bars (on the pose increment)."""
    from epropnp import functional as F
    B = 7
    prob = _problem(B, 150, dof, bounds, kind)
    _pose_init_off_the_edges(prob)
    pose = prob['pose_init']
    gvec = torch.randn(B, pose.shape[-1] if plus else dof, generator=torch.Generator().manual_seed(3))
    want, grad64 = _gn_oracle(prob, pose, gvec, plus)
    d, cam, cf = make_layer_objects(prob, backend)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d', 'delta')}
    cf.delta = leaves['delta']
    hp = F.PnPProblem(leaves['x3d'], leaves['x2d'], leaves['w2d'], cam, cf, dof)
    fn = F.pose_opt_plus if plus else F.gn_step
    got = fn(leaves['x3d'], leaves['x2d'], leaves['w2d'], leaves['delta'], hp, pose.to(backend), 1e-5)
    (got * gvec.to(backend)).sum().backward()
    base = pose.double() if plus else torch.zeros_like(want)
    scale = (want - base).abs().amax(-1, keepdim=True)
    e_step = ((got.detach().cpu().double() - want).abs() / scale).max().item()
    errs = {}
    for k in ('x3d', 'x2d', 'w2d', 'delta'):
        ref, mine = grad64[k], leaves[k].grad.detach().cpu().double()
        den = ref.abs().max().clamp(min=1e-12) if k == 'delta' else ref.reshape(B, -1).abs().amax(-1).clamp(min=1e-12).reshape(B, 1, 1)
        errs[k] = ((mine - ref).abs() / den).max().item()
    print(f'gn {"plus" if plus else "step"} {kind} dof={dof} bounds={bounds}: step {e_step:.3e} grads '
          + ' '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert e_step < 5e-4
    assert all(v < 2e-3 for v in errs.values()), errs


# ----------------------------------------------------------------------------------------------------------------------
# solvers
# ----------------------------------------------------------------------------------------------------------------------


def _lm_oracle(prob, L, dt=torch.float32):
    q = {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in prob.items()}
    pose, cov, cost, hist = orc.lm_solve(q['x3d'], q['x2d'], q['w2d'], _ocam(q), q['delta'], q['pose_init'],
                                         with_pose_cov=True, with_cost=True, num_iter=L)
    return pose, cov, cost, sum(h.to(torch.int32) << i for i, h in enumerate(hist))


@kinds_and_cases
def test_lm_solve(backend, kind, dof, bounds):
    """Four iterations against orc.lm_solve on identical fp32 inputs.  Objects whose accept mask equals the oracle's history agree
    in pose to 1e-4 outright (test_diagnostics.test_pose_parity_of_objects_with_the_oracles_accept_history); over all objects pose
    (1e-4), cost (1e-5 rel) and covariance (1e-3 of its largest entry) hold with the oracle's spread; at most 25 % of the objects may differ
    in the history of the first three steps (the cap test_diagnostics states, for L = 3; the fourth step of a converged object
    changes the cost by rounding only and either decision is legitimate)."""
    from epropnp import functional as F
    B, L = 7, 4
    prob = _problem(B, 150, dof, bounds, kind)
    p, hp = _hip_problem(prob, backend, dof)
    pose, cov, cost, acc = (t.cpu() for t in F.lm_solve(hp, p['pose_init'], L, with_pose_cov=True, with_cost=True, with_accepts=True))
    pose_o, cov_o, cost_o, mask_o = _lm_oracle(prob, L)
    same = acc == mask_o
    d_pose = orc.per_object_diff(pose, pose_o, 'pose_opt')
    d_cost = orc.per_object_diff(cost, cost_o, 'cost')
    d_cov = rel_per_object(cov, cov_o).float()
    print(f'lm {kind} dof={dof} bounds={bounds}: {int((~same).sum())} of {B} objects differ in accept history; history-equal: pose '
          f'{d_pose[same].max().item():.3e} cost {d_cost[same].max().item():.3e} cov {d_cov[same].max().item():.3e}; all: pose '
          f'{d_pose.max().item():.3e} cost {d_cost.max().item():.3e} cov {d_cov.max().item():.3e}')
    assert int(((acc & 7) != (mask_o & 7)).sum()) <= B // 4
    assert d_pose[same].max().item() <= 1e-4

    def run(pr, dt=torch.float32):
        o = _lm_oracle(pr, L, dt)
        return dict(pose_opt=o[0].float(), pose_cov=o[1].float(), cost=o[2].float())
    # cost and covariance, over all objects: the bar plus the oracle's own rounding spread, matched by rank (the fp32 oracle's
    # cost alone is up to 8e-5 off its fp64 run on these problems) -- test_lm_solver.test_lm_vs_oracle_seeded
    sp = orc.rounding_spread(run, prob, dict(pose_opt=pose_o, pose_cov=cov_o, cost=cost_o), trials=4, extra=[run(prob, torch.float64)])
    assert_within_spread(d_pose, sp['pose_opt'], 1e-4, what='pose_opt')
    assert_within_spread(d_cost, sp['cost'], 1e-5, what='cost')
    assert_within_spread(d_cov, sp['pose_cov'], 1e-3, what='pose_cov')


@kinds_and_cases
def test_rslm_solve(backend, kind, dof, bounds):
    """The one-launch initialiser on injected draws against orc.rslm_solve (test_rslm.test_fused_rslm_matches_oracle_on_injected_draws:
    cost rtol 5e-4 / atol 1e-5, the winning pose for all objects but at most one tie).  The centre-based start inverts K in closed
    form (csrc/rslm_kernel.hip): skew, a negative fx and a general third row go through it here."""
    from epropnp import functional as F
    B, N, P, n, L = 10, 96, 16, 16, 3
    prob = _problem(B, N, dof, bounds, kind)
    rn = orc.make_rslm_noise(prob, dof, n, P, seed=71)
    p, hp = _hip_problem(prob, backend, dof)
    pose, cost = F.rslm_solve(hp, P, n, L, inds=rn['inds'].to(backend), rot=rn['rot'].float().to(backend))
    o_pose, o_cost = orc.rslm_solve(prob['x3d'], prob['x2d'], prob['w2d'], _ocam(prob), prob['delta'], rn['inds'], rn['rot'].float(),
                                    dof, num_iter=L)
    d = (pose.cpu() - o_pose).abs().max(-1).values
    print(f'rslm {kind} dof={dof} bounds={bounds}: cost rel err {((cost.cpu() - o_cost).abs() / o_cost.abs()).max().item():.3e}, '
          f'pose diff {d.tolist()}')
    torch.testing.assert_close(cost.cpu(), o_cost, rtol=5e-4, atol=1e-5)
    assert int((d < 1e-3).sum()) >= B - 1, d


# ----------------------------------------------------------------------------------------------------------------------
# AMIS
# ----------------------------------------------------------------------------------------------------------------------


def _logw_error(prob, dof, K, samples, logw, props, z_min=0.1):
    """log-weights against the fp64 oracle's cost plus the mixture density at the kernel's own samples and proposals
    -> (largest error, its bar: 2e-4 x max(1, |expect|), test_amis._check_logweights)"""
    samples, logw, props = samples.cpu(), logw.cpu(), props.cpu()
    assert bool(torch.isfinite(samples).all()) and bool(torch.isfinite(props).all())
    q = _f64(prob)
    cost = orc.evaluate(q['x3d'], q['x2d'], q['w2d'], samples.double(), _ocam(q, z_min), q['delta'], want_cost=True)[1]
    expect = -cost.float() - _mixture_logq(samples, props, dof, K)
    fin = torch.isfinite(expect)
    assert bool((torch.isfinite(logw) == fin).all())
    return (logw[fin] - expect[fin]).abs().max().item(), 2e-4 * max(1.0, expect[fin].abs().max().item())


@kinds_and_cases
def test_amis_forward_logweights(backend, kind, dof, bounds):
    from epropnp import functional as F
    B, N, S, K = 5, 96, 64, 4
    prob = _problem(B, N, dof, bounds, kind)
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=8), dof).to(backend)
    p, hp = _hip_problem(prob, backend, dof)
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)
    samples, logw, props = F.amis_forward(hp, pose_opt, pose_cov, S, K, noise=noise, with_proposals=True)
    err, bar = _logw_error(prob, dof, K, samples, logw, props)
    print(f'logw {kind} dof={dof} bounds={bounds}: err {err:.3e} (bar {bar:.3e})')
    assert err <= bar


def _backward_inputs(prob, dof, S, seed, far=False):
    g = torch.Generator().manual_seed(seed)
    B = prob['x3d'].shape[0]
    poses = _poses_around(prob, dof, S, seed + 100)
    if far:
        poses[1, :, :3] *= 300.0                  # far away: large (K t) entries against small rotation entries
    g_logw = torch.randn(S, B, generator=g)
    g_logw[3] = 0.0                               # exact zeros are skipped by the kernel
    g_logw[5:9, B - 1] *= 1e-12                   # below the 2^-30 relative drop threshold
    return poses, g_logw, torch.randn(B, generator=g)


def _backward_oracle(prob, poses, g_logw, g_init):
    q = _f64(prob)
    leaves = [q[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d', 'delta')]
    c_s = orc.evaluate(*leaves[:3], poses.double(), _ocam(q), leaves[3], want_cost=True)[1]
    c_i = orc.evaluate(*leaves[:3], q['pose_init'], _ocam(q), leaves[3], want_cost=True)[1]
    ((-c_s) * g_logw.double()).sum().add((c_i * g_init.double()).sum()).backward()
    return [t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def _backward_case(kind, dof, bounds, far):
    """problem, inputs and fp64 gradients, computed once for the launch paths that share them"""
    prob = _problem(5, 150, dof, bounds, kind)
    poses, g_logw, g_init = _backward_inputs(prob, dof, 40, seed=5, far=far)
    return prob, poses, g_logw, g_init, _backward_oracle(prob, poses, g_logw, g_init)


# (bwd_impl, EPROPNP_BWD_PROJ, bwd_presplit)
BWD_PATHS = [('valu', None, None), ('mfma', None, None), ('mfma', 'bf16', 0), ('mfma', 'f32', None)]


@pytest.mark.parametrize('impl,proj,presplit', BWD_PATHS, ids=['valu', 'mfma', 'mfma-bf16-per-tile', 'mfma-f32'])
@kinds_and_cases
def test_amis_backward(backend, monkeypatch, kind, dof, bounds, impl, proj, presplit):
    """The backward kernels at fixed samples against fp64 autograd of orc.evaluate: gradients to x3d, x2d, w2d and delta within
    2e-4 of the largest entry (test_amis.test_backward_matches_autograd_of_oracle_at_fixed_samples).  Both `bwd_impl` values, each
    as `backward_split` decides and unsplit.  The MFMA kernel's default is the bf16-split projection with the pose rows split
    once per object; `bwd_presplit=0` splits them per tile (test_presplit_pose_rows), EPROPNP_BWD_PROJ=f32 is the fp32 matrix
    path (test_amis.test_backward_bf16_split_projection_against_the_fp32_matrix_path, whose far-away pose is among the samples)."""
    from epropnp import functional as F
    set_tune(monkeypatch, bwd_impl=impl, bwd_presplit=presplit)
    if proj is not None:
        monkeypatch.setenv('EPROPNP_BWD_PROJ', proj)
    prob, poses, g_logw, g_init, want = _backward_case(kind, dof, bounds, impl == 'mfma')
    p, hp = _hip_problem(prob, backend, dof)
    if impl == 'mfma':
        plan = F.launch_plan('backward', hp, poses.shape[0], pose_init=True)
        assert not plan['valu'] and plan['bf16'] == (proj != 'f32'), plan
    for nsplit in (None, 1):
        got = F.amis_backward(hp, poses.to(backend), g_logw.to(backend), p['pose_init'], g_init.to(backend), nsplit=nsplit)
        errs = [_rel(a.cpu().double(), b) for a, b in zip(got, want)]
        print(f'backward {kind} dof={dof} bounds={bounds} {impl} {proj} presplit={presplit} nsplit={nsplit}: '
              + ' '.join(f'{e:.3e}' for e in errs))
        assert max(errs) <= 2e-4, (nsplit, errs)


# ----------------------------------------------------------------------------------------------------------------------
# gradients to the pose and to all nine entries of each object's own K
# ----------------------------------------------------------------------------------------------------------------------


def _pose_cam_inputs(prob, dof, P=3):
    g = torch.Generator().manual_seed(5)
    B = prob['x3d'].shape[0]
    poses = prob['pose_init'].unsqueeze(0).repeat(P, 1, 1)
    poses[1:, :, :3] += 0.05 * torch.randn(P - 1, B, 3, generator=g)
    weights = torch.randn(P, B, generator=g)
    weights[2, 1] = 0.0                                  # a skipped pose
    assert float(_edge_margin(prob, poses).min()) >= EDGE_PX, 'a pose projects a point onto a bound: take another seed'
    return poses, weights


def _oracle_grads_fp32(prob, dof, poses, weights, bounds):
    """the same autograd in fp32: what a correct fp32 implementation of the reference's arithmetic is off by, per entry"""
    x3d, x2d, w2d = (prob[k].float() for k in ('x3d', 'x2d', 'w2d'))
    K = prob['cam_mats'].float().clone().requires_grad_(True)
    cam = orc.Cam(K, 0.1, None if bounds is None else prob['lb'].float(), None if bounds is None else prob['ub'].float())
    cost = orc.evaluate(x3d, x2d, w2d, poses.float(), cam, prob['delta'].float(), want_cost=True)[1]
    (cost * weights.float()).sum().backward()
    return K.grad.double()


@kinds_and_cases
def test_pose_cam_grad(backend, kind, dof, bounds):
    """d/d pose and d/d K against fp64 autograd of the oracle, per object at 2e-4 of the object's largest entry
    (test_pose_cam_grad.test_pose_cam_grad_kernel_matches_autograd) -- and d/d K per ENTRY, since a per-object maximum lets the
    large entries hide an error in the small ones:

      * an entry is allowed the fp32 oracle's own error at that entry (fp32 autograd of orc.evaluate against fp64, same inputs)
        plus the per-object bar carried over to the entry, 2e-4 x max|grad_K_b| / |entry|, both relative to the entry.  In
        absolute terms that is the per-object bar plus the fp32 oracle's error, so it cannot bind where the per-object bar holds;
      * the check that does bind: the same 2e-4, with the scale taken per matrix POSITION over the batch instead of per object
        over the positions -- |error[b,i,j]| <= fp32 oracle's error[b,i,j] + 2e-4 x max_b' |grad_K[b',i,j]|.  The nine positions
        differ in size by the pixel scale (d/dK[2,:] carries a factor of the projection, hundreds of pixels, that d/dK[:2,:]
        does not), whereas the objects of a batch are alike: an entry is measured against entries that are sums of the same
        kind of terms, and a wrong or missing term at one position shows at that position.

    fp32 oracle against fp64, per entry relative to the entry, largest over the objects and the nine (kind, dof, bounds) cases at
    B = 7, N = 150: K[0,0] 6.3e-5, K[0,1] 2.1e-4, K[0,2] 1.1e-4, K[1,0] 8.5e-6, K[1,1] 2.7e-5, K[1,2] 8.2e-6, K[2,0] 2.9e-5,
    K[2,1] 3.4e-5, K[2,2] 3.2e-5 (the kernel on the CPU emulation: within 1.6x of these at every position, 2.5e-4 at K[0,1])."""
    from epropnp import functional as F
    B = 7
    prob = _problem(B, 150, dof, bounds, kind)
    poses, weights = _pose_cam_inputs(prob, dof)
    p, hp = _hip_problem(prob, backend, dof)
    ref_p, ref_k, _ = _oracle_grads(prob, dof, poses, weights, bounds)
    o32 = (_oracle_grads_fp32(prob, dof, poses, weights, bounds) - ref_k).abs()
    big = ref_k.abs().reshape(B, -1).amax(1).clamp(min=1e-12).reshape(B, 1, 1)
    pos = ref_k.abs().amax(0, keepdim=True)
    fmt = lambda t: ' '.join(f'{v:.1e}' for v in t.flatten().tolist())
    for m in (0, 2):
        gp, gk = F.pose_cam_grad(hp, poses.to(backend), weights.to(backend), m_pose=m)
        gp, err = gp.cpu().double(), (gk.cpu().double() - ref_k).abs()
        e_p = (gp - ref_p[m]).abs().amax(1) / ref_p[m].abs().amax(1).clamp(min=1e-12)
        print(f'pose_cam_grad {kind} dof={dof} bounds={bounds} m={m}: pose {e_p.max().item():.3e} K per object '
              f'{(err / big).max().item():.3e}, per position {(err / pos).max().item():.3e}; per entry, relative to the entry, largest '
              f'over the objects:\n  kernel      {fmt((err / ref_k.abs()).amax(0))}\n  fp32 oracle {fmt((o32 / ref_k.abs()).amax(0))}'
              f'\n  position scale / object scale {fmt((pos / big).amin(0))}')
        assert e_p.max().item() <= 2e-4, e_p
        assert (err / big).max().item() <= 2e-4, (err / big).reshape(B, -1).amax(1)
        assert bool((err <= o32 + 2e-4 * big).all()), (err / ref_k.abs()).amax(0)
        assert bool((err <= o32 + 2e-4 * pos).all()), ((err - o32) / pos).amax(0)


@kinds_and_cases
def test_layer_gradient_to_per_object_cam_mats(backend, kind, dof, bounds):
    """monte_carlo_forward with a (B,3,3) leaf `cam_mats`: the gradient has that shape and is, object by object, fp64 autograd's of
    the oracle at the kernel's own samples -- cost_init and every log-weight w.r.t. the object's own K (bar: 2e-4 per object,
    test_pose_cam_grad.test_layer_gradients_reach_pose_init_and_cam_mats, which shares ONE matrix and compares the sum)."""
    from epropnp.camera import PerspectiveCamera
    from epropnp.epropnp import EProPnP4DoF, EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver
    B, N, S, K = 5, 96, 64, 4
    prob = _problem(B, N, dof, bounds, kind)
    _pose_init_off_the_edges(prob)
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=38), dof)
    p, cam0, cf = make_layer_objects(prob, backend)
    layer = (EProPnP6DoF if dof == 6 else EProPnP4DoF)(mc_samples=S, num_iter=K, normalize=(dof == 4), solver=LMSolver(dof=dof, num_iter=4))
    g = torch.Generator().manual_seed(7)
    g_logw, g_init = torch.randn(S, B, generator=g) * 0.1, torch.randn(B, generator=g)
    x3d, x2d, w2d = (p[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d'))
    Kmat = p['cam_mats'].clone().requires_grad_(True)
    cam = PerspectiveCamera(cam_mats=Kmat, z_min=0.1, lb=p.get('lb'), ub=p.get('ub'))
    out = layer.monte_carlo_forward(x3d, x2d, w2d, cam, cf, pose_init=p['pose_init'], force_init_solve=False, noise=noise.to(backend))
    samples = out[3].detach().cpu()
    near = _edge_margin(prob, samples) < EDGE_PX         # the kernel's own samples cannot be redrawn: such a one gets no upstream gradient
    assert float(near.float().mean()) < 0.1
    g_logw[near] = 0.0
    ((out[4] * g_logw.to(backend)).sum() + (out[5] * g_init.to(backend)).sum()).backward()
    assert Kmat.grad.shape == (B, 3, 3)
    allp = torch.cat((samples, prob['pose_init'].unsqueeze(0)), 0)
    _, ref_k, _ = _oracle_grads(prob, dof, allp, torch.cat((-g_logw, g_init.unsqueeze(0)), 0), bounds)
    err = rel_per_object(Kmat.grad.cpu(), ref_k)
    print(f'layer cam_mats.grad {kind} dof={dof} bounds={bounds}: per object {err.tolist()}, {int(near.sum())} samples left out')
    assert err.max().item() <= 2e-4, err


# ----------------------------------------------------------------------------------------------------------------------
# the one-call forward
# ----------------------------------------------------------------------------------------------------------------------


def _one_call(backend, monkeypatch, prob, dof, fused):
    """monte_carlo_forward + backward() of EProPnP6DoF / EProPnP4DoF(normalize=True) with the RSLM initialiser (injected draws)
    and with_pose_opt_plus=True -> the six outputs and the three input gradients"""
    from epropnp.epropnp import EProPnP4DoF, EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver, RSLMSolver
    B, S, K = prob['x3d'].shape[0], 32, 2
    set_tune(monkeypatch, no_fused_forward=not fused)
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=4), dof).to(backend)
    rn = orc.make_rslm_noise(prob, dof, 8, 12, seed=5)
    p, cam, cf = make_layer_objects(prob, backend)
    x3d, x2d, w2d = (p[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d'))
    init = RSLMSolver(dof=dof, num_points=8, num_proposals=12, num_iter=3)
    init.draw = lambda w: (rn['inds'].to(backend), rn['rot'].float().to(backend))
    layer = (EProPnP6DoF if dof == 6 else EProPnP4DoF)(mc_samples=S, num_iter=K, normalize=(dof == 4),
                                                       solver=LMSolver(dof=dof, num_iter=3, init_solver=init))
    assert layer._fusable(x3d, x2d, w2d, p['pose_init'], True, dict(with_pose_opt_plus=True)) == fused
    out = layer.monte_carlo_forward(x3d, x2d, w2d, cam, cf, pose_init=p['pose_init'], force_init_solve=True,
                                    with_pose_opt_plus=True, with_cost=True, noise=noise)
    pose_opt, cost, plus, samples, logw, cost_init = out
    ((cost_init + torch.logsumexp(logw, 0)).mean() + 0.1 * plus.sum()).backward()
    res = [t.detach().cpu() for t in (pose_opt, cost, plus, samples, logw, cost_init, x3d.grad, x2d.grad, w2d.grad)]
    assert all(bool(torch.isfinite(t).all()) for t in res)
    return res


@kinds_and_cases
def test_one_call_forward_equals_composite(backend, monkeypatch, poisoned_empty, kind, dof, bounds):
    """The fused entry against EPROPNP_TUNE=no_fused_forward under poisoned allocations (ctypes binding): the same bits
    (test_fused_and_limits.test_fused_forward_equals_composite), with every object on its own camera and bounds."""
    prob = dict(_problem(5, 70, dof, bounds, kind))
    prob['pose_init'] = prob['pose_init'].clone()
    prob['pose_init'][0, :3] += 3.0                        # object 0: a bad pose_init, so the initialiser's start wins there
    a = _one_call(backend, monkeypatch, prob, dof, True)
    b = _one_call(backend, monkeypatch, prob, dof, False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.gpu
@kinds_and_cases
def test_one_call_forward_cpp_nodes_equal_ctypes_nodes(monkeypatch, kind, dof, bounds):
    """the same step through the C++ extension and through the ctypes binding (EPROPNP_NO_TORCH_EXT=1): equal again
    (test_torch_binding.test_cpp_nodes_equal_ctypes_nodes)"""
    import install as emu
    from epropnp import _hip
    emu.uninstall()
    dev = torch.device('cuda:0')
    prob = _problem(5, 70, dof, bounds, kind)
    outs = []
    try:
        for use_ext in (True, False):
            if use_ext:
                monkeypatch.delenv('EPROPNP_NO_TORCH_EXT', raising=False)
            else:
                monkeypatch.setenv('EPROPNP_NO_TORCH_EXT', '1')
            _hip._torch_ext = False                           # detect again
            assert (_hip.torch_ext() is not None) == use_ext
            outs.append(_one_call(dev, monkeypatch, prob, dof, True))
    finally:
        _hip._torch_ext = False
    for i, (x, y) in enumerate(zip(*outs)):
        assert torch.equal(x, y), i


# ----------------------------------------------------------------------------------------------------------------------
# split launches: every split run against its unsplit run, at the bars of the sibling tests
# ----------------------------------------------------------------------------------------------------------------------


def _close(a, b, rel):
    return bool(((a - b).abs() <= rel * b.abs().clamp(min=1e-30) + 1e-30).all()) if a.dim() == 1 else \
        bool((a - b).abs().max() <= rel * b.abs().max())


def _lm_split_check(F, hp, pose_init, monkeypatch, splits):
    """test_lm_solver.test_lm_split_recomputes_missing_parts: cost 2e-5; pose 2e-5 and covariance 2e-3 for the objects with the
    same accept history -- which at L = 2, where no object has converged and every decision is clear, must be all of them on the
    GPU and all but one on the emulation.  At L = 4 a step of a converged object changes the cost by rounding only and is taken or
    not by the summation order (measured on the emulation with these problems: up to all three objects part ways, at costs equal
    to 3e-6): there the cost bar holds for every object, the pose and covariance bars for those that kept their history."""
    B = hp.B
    kw = dict(with_pose_cov=True, with_cost=True, with_accepts=True)
    for L in (2, 4):
        monkeypatch.setenv('EPROPNP_LM_SPLIT', '1')
        one = F.lm_solve(hp, pose_init, L, **kw)
        for G in splits:
            if G is None:
                monkeypatch.delenv('EPROPNP_LM_SPLIT')
            else:
                monkeypatch.setenv('EPROPNP_LM_SPLIT', str(G))
            par = F._hip.LmParams(L, 0, 1e-6, 1e32, 1e-3, 30.0, 1e16, 1e-5)
            assert (F.lm_split_scratch(hp, par) is not None) == (G != 1), G
            many = F.lm_solve(hp, pose_init, L, **kw)
            same = many[3] == one[3]
            if L == 2:
                assert int(same.sum()) >= (B if hp.device.type == 'cuda' else B - 1), (G, many[3], one[3])
            assert _close(many[2], one[2], 2e-5), (L, G)
            if bool(same.any()):
                assert (many[0] - one[0])[same].abs().max().item() <= 2e-5, (L, G)
                assert _close(many[1][same], one[1][same], 2e-3), (L, G)


def _lm_split_as_picked_check(F, prob, hp, pose_init, monkeypatch, L=4):
    """test_lm_solver.test_lm_split_over_workgroups (few objects x thousands of points, where the library splits on its own): the
    split run against the oracle at pose 1e-4 and cost 1e-5, each widened only by the oracle's own rounding spread, to which
    the one-workgroup run is added; the covariance finite"""
    par = F._hip.LmParams(L, 0, 1e-6, 1e32, 1e-3, 30.0, 1e16, 1e-5)
    kw = dict(with_pose_cov=True, with_cost=True)
    monkeypatch.setenv('EPROPNP_LM_SPLIT', '1')
    assert F.lm_split_scratch(hp, par) is None
    one = F.lm_solve(hp, pose_init, L, **kw)
    monkeypatch.delenv('EPROPNP_LM_SPLIT')
    assert F.lm_split_scratch(hp, par) is not None, 'this shape is meant to take the split'
    pose, cov, cost = (t.cpu() for t in F.lm_solve(hp, pose_init, L, **kw))

    def run(pr, dt=torch.float32):
        o = _lm_oracle(pr, L, dt)
        return dict(pose_opt=o[0].float(), cost=o[2].float())
    base = run(prob)
    sp = orc.rounding_spread(run, prob, base, extra=[run(prob, torch.float64), dict(pose_opt=one[0].cpu(), cost=one[2].cpu())])
    d_pose, d_cost = orc.per_object_diff(pose, base['pose_opt'], 'pose_opt'), orc.per_object_diff(cost, base['cost'], 'cost')
    print(f'lm split as picked: against the oracle pose {d_pose.max().item():.3e} cost {d_cost.max().item():.3e}; against one workgroup '
          f'pose {(pose - one[0].cpu()).abs().max().item():.3e} cost {orc.per_object_diff(cost, one[2].cpu(), "cost").max().item():.3e}')
    assert_within_spread(d_pose, sp['pose_opt'], 1e-4, what='pose_opt')
    assert_within_spread(d_cost, sp['cost'], 1e-5, what='cost')
    assert bool(torch.isfinite(cov).all())


def _fwd_split_check(F, prob, hp, pose_init, monkeypatch, dof, split, S, K, bars):
    """test_amis.test_forward_split_recomputes_missing_parts (emulation: samples 5e-3, logsumexp 2e-2) /
    test_forward_split_over_workgroups (GPU: samples 5e-4, logsumexp 1e-3 + 2e-6 max|logw|): the first iteration's samples are the
    same bits, and the split run's log-weights are the oracle's at its own samples"""
    B = hp.B
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=30), dof).to(hp.device)
    monkeypatch.setenv('EPROPNP_LM_SPLIT', '1')
    pose_opt, pose_cov, _ = F.lm_solve(hp, pose_init, 3, with_pose_cov=True)
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    assert F.launch_plan('forward', hp, S, K)['G'] == 1
    s1, w1 = F.amis_forward(hp, pose_opt, pose_cov, S, K, noise=noise)
    if split is None:
        monkeypatch.delenv('EPROPNP_FWD_SPLIT')
    else:
        monkeypatch.setenv('EPROPNP_FWD_SPLIT', str(split))
    assert F.split_scratch(hp, S, K) is not None and F.launch_plan('forward', hp, S, K)['G'] > 1
    s2, w2, pr2 = F.amis_forward(hp, pose_opt, pose_cov, S, K, noise=noise, with_proposals=True)
    assert torch.equal(s1[:S // K], s2[:S // K])
    assert (s1 - s2).abs().max().item() <= bars[0] * max(1.0, s1.abs().max().item())
    assert (torch.logsumexp(w1, 0) - torch.logsumexp(w2, 0)).abs().max().item() < bars[1] + bars[2] * w1[torch.isfinite(w1)].abs().max().item()
    err, bar = _logw_error(prob, dof, K, s2, w2, pr2)
    assert err <= bar, (err, bar)


def _bwd_split_check(F, prob, hp, pose_init, dof, S, splits):
    """test_amis.test_backward_split_over_workgroups: per-point gradients bit-identical to the one-workgroup kernel, grad_delta 1e-5"""
    poses, g_logw, g_init = _backward_inputs(prob, dof, S, seed=6)
    args = (hp, poses.to(hp.device), g_logw.to(hp.device), pose_init, g_init.to(hp.device))
    one = F.amis_backward(*args, nsplit=1)
    for nsplit in splits:
        if nsplit is None:
            assert F.launch_plan('backward', hp, S, pose_init=True)['nsplit'] > 1
        many = F.amis_backward(*args, nsplit=nsplit)
        for a, b in zip(many[:3], one[:3]):
            assert torch.equal(a, b), nsplit
        assert _rel(many[3].cpu(), one[3].cpu()) <= 1e-5, nsplit


def _rslm_parts_check(F, prob, hp, monkeypatch, dof, parts):
    """test_fused_and_limits.test_rslm_split_winner_is_picked_inside_the_lm_launch: the same bits as one workgroup per object
    (64 proposals: four whole rounds of 16, which is what the parts deal out)"""
    P, n = 64, 8
    rn = orc.make_rslm_noise(prob, dof, n, P, seed=71)
    inds, rot = rn['inds'].to(hp.device), rn['rot'].float().to(hp.device)
    words = lambda k: k * hp.B * (hp.pose_len + 1)          # csrc/rslm_kernel.hip: rslm_scratch_bytes
    set_tune(monkeypatch, rslm_parts=1)
    assert F.rslm_scratch(hp, P).numel() == words(1)
    one = F.rslm_solve(hp, P, n, 1, inds=inds, rot=rot, with_winner=True)
    for k in parts:
        set_tune(monkeypatch, rslm_parts=k)
        assert F.rslm_scratch(hp, P).numel() == words(k or 4), k
        many = F.rslm_solve(hp, P, n, 1, inds=inds, rot=rot, with_winner=True)
        for a, b in zip(many, one):
            assert torch.equal(a, b), k
    set_tune(monkeypatch)


@kinds_and_cases
def test_split_launches(backend, monkeypatch, kind, dof, bounds):
    """B = 3 objects on their own cameras; LM solve split over {4} workgroups (and EPROPNP_LM_SPLIT=1, the base) at N = 300, the
    AMIS forward over 4, the RSLM proposals over {4} parts, the backward over {2, 4} (and 1, the base)."""
    from epropnp import functional as F
    prob = _problem(3, 300, dof, bounds, kind)
    p, hp = _hip_problem(prob, backend, dof)
    _lm_split_check(F, hp, p['pose_init'], monkeypatch, (4,))
    _fwd_split_check(F, prob, hp, p['pose_init'], monkeypatch, dof, 4, 32, 2, (5e-3, 2e-2, 0.0))
    _bwd_split_check(F, prob, hp, p['pose_init'], dof, 40, (2, 4))
    prob = _problem(3, 96, dof, bounds, kind)               # (64 proposals an object: the smallest N the other tests use)
    p, hp = _hip_problem(prob, backend, dof)
    _rslm_parts_check(F, prob, hp, monkeypatch, dof, (4,))


@pytest.mark.gpu
@kinds_and_cases
def test_split_launches_as_the_library_picks_them(monkeypatch, kind, dof, bounds):
    """the sizes at which lm_split_scratch / launch_plan / rslm_scratch split on their own on an MI355X (asserted), against the unsplit runs"""
    import install as emu
    emu.uninstall()
    from epropnp import functional as F
    dev = torch.device('cuda:0')
    prob = _problem(3, 2100, dof, bounds, kind)             # (beyond 2048 points an object's sweep outlasts the exchange)
    p, hp = _hip_problem(prob, dev, dof)
    _lm_split_as_picked_check(F, prob, hp, p['pose_init'], monkeypatch)
    prob = _problem(3, 1000, dof, bounds, kind)
    p, hp = _hip_problem(prob, dev, dof)
    _fwd_split_check(F, prob, hp, p['pose_init'], monkeypatch, dof, None, 64, 2, (5e-4, 1e-3, 2e-6))
    prob = _problem(3, 512, dof, bounds, kind)
    p, hp = _hip_problem(prob, dev, dof)
    _bwd_split_check(F, prob, hp, p['pose_init'], dof, 40, (None,))
    _rslm_parts_check(F, prob, hp, monkeypatch, dof, (None,))


# ----------------------------------------------------------------------------------------------------------------------
# permutation of the batch: the check that catches a camera or a bound read for the wrong object
# ----------------------------------------------------------------------------------------------------------------------


def _twelve_outputs(F, prob, backend, dof, perm, S, K=2):
    """lm_solve (pose, covariance, cost), normal_equations (jtj, jtr, cost), amis_forward on injected noise (samples, log-weights)
    and amis_backward (gradients to x3d, x2d, w2d, delta) with the objects in the order `perm`, returned in natural order"""
    B = perm.numel()
    inv = torch.argsort(perm)
    sub = {k: (v[perm].contiguous() if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == B else v) for k, v in prob.items()}
    p, hp = _hip_problem(sub, backend, dof)
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=8), dof)[perm].contiguous().to(backend)
    g = torch.Generator().manual_seed(9)
    g_logw, g_init = torch.randn(S, B, generator=g)[:, perm].contiguous().to(backend), torch.randn(B, generator=g)[perm].to(backend)
    pose, cov, cost = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True, with_cost=True)
    jtj, jtr, c0 = F.normal_equations(hp, p['pose_init'], clip_jac=True)
    samples, logw = F.amis_forward(hp, pose, cov, S, K, noise=noise)
    grads = F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init)
    out = dict(pose=pose, cov=cov, cost=cost, jtj=jtj, jtr=jtr, cost_init=c0, samples=samples, logw=logw,
               gx3d=grads[0], gx2d=grads[1], gw2d=grads[2], gdelta=grads[3])
    return {k: (v[:, inv] if k in ('samples', 'logw') else v[inv]).cpu() for k, v in out.items()}


@pytest.mark.parametrize('B', [11, 64])
@pytest.mark.parametrize('dof,bounds', CASES)
def test_permuted_batch_gives_the_same_bits_per_object(backend, dof, bounds, B):
    """The objects in natural order and in a seeded permutation (noise and upstream gradients permuted with them): every output of
    object b is bit-identical in both runs.  An object's result depends on its own inputs only -- the block that serves it
    (pnp_sweep.h: object_of_block, the (g & 7) * per + (g >> 3) swizzle; v / nsplit, v / parts, blockIdx.x / spans; the clamp of
    the idle rows to B - 1 in lm_kernel.hip) must read that object's camera and bounds, and with the 'full' kind no two objects
    share either.  B = 11 is odd and no multiple of 8 (the swizzle's remainder rows), B = 64 fills its rows."""
    from epropnp import functional as F
    N, S = (70, 32) if B == 11 else (33, 16)               # (64 objects: one ragged wave of points, 8 samples an iteration)
    prob = _problem(B, N, dof, bounds, 'full')
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    assert not bool((perm == torch.arange(B)).all())
    a = _twelve_outputs(F, prob, backend, dof, torch.arange(B), S)
    b = _twelve_outputs(F, prob, backend, dof, perm, S)
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max())


# ----------------------------------------------------------------------------------------------------------------------
# scale of K
# ----------------------------------------------------------------------------------------------------------------------


@kinds_and_cases
def test_scaled_camera_matrix_is_the_same_camera(backend, kind, dof, bounds):
    """K and c K with z_min scaled by the same c describe the same camera; with c = 2 every product and quotient of the
    projection is exact in the factor, so the cost, the samples and log-weights (from the same pose_opt and covariance), the
    gradients to the correspondences and to the pose are the same bits, and the gradient to cam_mats is exactly 1/c times the other.

    The LM pose is NOT among them: the reference's Jacobian takes d p / d z_cam = (K[:2,2] - p) / z (epropnp/camera.py:111-143),
    which is the derivative of the projection only for a third row (0, 0, 1) -- with c K the term becomes (c K[:2,2] - p) / (c z),
    the normal equations change (J^T J of the first problem by up to 1e3 absolute) and the reference's own solve takes another
    path.  The kernels follow the reference there: the solve on c K is held to the oracle's solve on c K, history-equal objects
    at 1e-4 as in test_lm_solve."""
    from epropnp import functional as F
    from epropnp.camera import PerspectiveCamera
    from epropnp.cost_fun import HuberPnPCost
    B, N, S, K, c, L = 5, 96, 32, 2, 2.0, 4
    prob = _problem(B, N, dof, bounds, kind)
    d = {k: (v.to(backend) if isinstance(v, torch.Tensor) else v) for k, v in prob.items()}
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=8), dof).to(backend)
    g = torch.Generator().manual_seed(9)
    g_logw, g_init = torch.randn(S, B, generator=g).to(backend), torch.randn(B, generator=g).to(backend)
    outs, start = [], None
    for f in (1.0, c):
        cam = PerspectiveCamera(cam_mats=(d['cam_mats'] * f).contiguous(), z_min=0.1 * f, lb=d.get('lb'), ub=d.get('ub'))
        hp = F.PnPProblem(d['x3d'], d['x2d'], d['w2d'], cam, HuberPnPCost(delta=d['delta']), dof)
        pose, cov, cost, acc = F.lm_solve(hp, d['pose_init'], L, with_pose_cov=True, with_cost=True, with_accepts=True)
        if f != 1.0:
            o = orc.lm_solve(prob['x3d'], prob['x2d'], prob['w2d'], orc.Cam(prob['cam_mats'] * f, 0.1 * f, prob.get('lb'), prob.get('ub')),
                             prob['delta'], prob['pose_init'], with_cost=True, num_iter=L)
            same = acc.cpu() == sum(h.to(torch.int32) << i for i, h in enumerate(o[3]))
            assert int(((acc.cpu() & 7) != (sum(h.to(torch.int32) << i for i, h in enumerate(o[3])) & 7)).sum()) <= B // 4
            assert (pose.cpu() - o[0])[same].abs().max().item() <= 1e-4
        start = start or (pose, cov)
        samples, logw = F.amis_forward(hp, *start, S, K, noise=noise)
        grads = F.amis_backward(hp, samples, g_logw, d['pose_init'], g_init)
        gp, gk = F.pose_cam_grad(hp, samples, g_logw, m_pose=0)
        outs.append([F.evaluate_cost(hp, d['pose_init']), F.evaluate_cost(hp, samples), samples, logw, *grads, gp, gk * f])
    for i, (x, y) in enumerate(zip(*outs)):
        assert bool(torch.isfinite(x).all()), i
        assert torch.equal(x, y), (i, (x - y).abs().max())
