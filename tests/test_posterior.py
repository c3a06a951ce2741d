"""epropnp.posterior: summarize (epropnp_posterior_summary) and resample (epropnp_posterior_resample) of the weighted pose samples
against fp64 torch on the same fp32 inputs, at the smallest shapes at which the 16-column x 32-row-group decomposition can go
wrong: (1,1); (64,3) one partly filled column block; (510,70) S no multiple of the row groups, five column blocks, a ragged last
one, and the edge columns; (4096,2) many rows per group."""
import math

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise

SHAPES = [(1, 1), (64, 3), (510, 70), (4096, 2)]
CENTER = (2.0, 1.0, 50.0)
EDGE = {5: 'empty', 9: 'nan', 40: 'inf'}      # the column positions of test_weight_stats_against_fp64; 66: half the samples -inf
# trans_cov against fp64, relative to its Frobenius norm, offset case (translations (2, 1, 50) + 0.05 randn): 4 x the larger of the
# largest errors seen on the CPU emulation and on the MI355X (see test_second_moments_offset_case); may not exceed 1e-4
COV_BAR = 4 * 1.66e-6


def _bits(t):
    return t.contiguous().view(torch.int32)


_cases = {}


def _case(S, B, dof, spread):
    """(pose_samples, logweights, pose_ref, good columns) on the CPU, built once per shape: log-weights spread over +-40, translations
    CENTER + spread * randn, yaws anywhere / quaternions around a per-object q0 with every second sign flipped; a NaN pose under a
    -inf log-weight in column 0; in the widest case the edge columns."""
    key = (S, B, dof, spread)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * dof + S + B)
        lw = torch.rand(S, B, generator=g) * 80.0 - 40.0
        t = torch.tensor(CENTER) + spread * torch.randn(S, B, 3, generator=g)
        ref_t = torch.tensor(CENTER) + spread * torch.randn(B, 3, generator=g)
        if dof == 4:
            rot = torch.rand(B, 1, generator=g) * 6.0 - 3.0 + 0.3 * torch.randn(S, B, 1, generator=g)
            ref_r = torch.zeros(B, 1)
        else:
            q0 = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
            rot = torch.nn.functional.normalize(q0 + 0.1 * torch.randn(S, B, 4, generator=g), dim=-1)
            rot[1::2] = -rot[1::2]
            ref_r = q0
        ps = torch.cat((t, rot), -1).contiguous()
        ref = torch.cat((ref_t, ref_r), -1).contiguous()
        ref[0, [0, 2]] = ps[lw[:, 0].argmax(), 0][[0, 2]]          # object 0: its heaviest sample deviates by exactly 0 (score 1)
        if S >= 2:
            lw[S // 2, 0] = float('-inf')
            ps[S // 2, 0] = float('nan')
        good = list(range(B))
        if B >= 70:
            lw[:, 5] = float('-inf')
            lw[S // 3, 9] = float('nan')
            lw[S - 1, 40] = float('inf')
            lw[::2, 66] = float('-inf')
            ps[::2, 66] = float('nan')
            good = [b for b in range(B) if b not in EDGE]
        _cases[key] = (ps, lw, ref, good)
    return _cases[key]


_refs = {}


def _fp64(ps, lw, ref, key=None):
    """The summary in fp64 torch from the same fp32 inputs; score_te is the reference caller's expression (EPro-PnP-Det
    deform_pnp_head.py:524, 534-536)."""
    if key is not None and key in _refs:
        return _refs[key]
    ps, lw, ref = ps.double(), lw.double(), ref.double()
    w = torch.softmax(lw, dim=0)                                        # pose_sample_logweights.softmax(dim=0)
    ps = torch.where((w > 0)[..., None], ps, torch.zeros_like(ps))      # zero-weight samples are skipped, not multiplied
    t = ps[..., :3]
    mean = (w[..., None] * t).sum(0)
    dev = t - mean
    cov = torch.einsum('mb,mbi,mbj->bij', w, dev, dev)
    sample_dev = (ps[..., [0, 2]] - ref[:, [0, 2]]).norm(dim=-1)
    score = (((-sample_dev.log2() + 2.5) / 4).clamp(min=0, max=1) * w).sum(dim=0)
    out = dict(mean=mean, cov=cov, score=score, spread=(w * dev.square().sum(-1)).sum(0).sqrt())
    if ps.shape[-1] == 4:
        c, s = (w * ps[..., 3].cos()).sum(0), (w * ps[..., 3].sin()).sum(0)
        out.update(resultant=(c * c + s * s).sqrt(), yaw=torch.atan2(s, c))
    else:
        q = ps[..., 3:]
        lam, vec = torch.linalg.eigh(torch.einsum('mb,mbi,mbj->bij', w, q, q))
        out.update(resultant=lam[:, 3], quat=vec[:, :, 3], gap=lam[:, 3] - lam[:, 2])
    if key is not None:
        _refs[key] = out
    return out


def _angle(a, b):
    """angle between the lines spanned by unit vectors (sign-free), accurate near 0"""
    a, b = a.double(), b.double()
    return 2 * torch.asin((torch.minimum((a - b).norm(dim=-1), (a + b).norm(dim=-1)) / 2).clamp(max=1))


def _check_first_moments(got, want, tag):
    err_m = (got.trans_mean.double().cpu() - want['mean']).abs().amax(-1) / (want['mean'].norm(dim=-1) + want['spread'])
    err_r = (got.rot_resultant.double().cpu() - want['resultant']).abs()
    err_s = (got.score_te.double().cpu() - want['score']).abs()
    print(f'{tag}: trans_mean rel err {err_m.max().item():.3e}, resultant abs err {err_r.max().item():.3e}, '
          f'score_te abs err {err_s.max().item():.3e}')
    assert err_m.max().item() <= 1e-5 and err_r.max().item() <= 1e-5 and err_s.max().item() <= 1e-5


def _check_quaternion(got, want, tag):
    assert bool((want['gap'] > 0.05).all()), want['gap'].min()         # the input stays within the condition of the angle bar
    ang = _angle(got.rot_mean.cpu(), want['quat'])
    err_l = (got.rot_resultant.double().cpu() - want['resultant']).abs()
    print(f'{tag}: quaternion mean angle err {ang.max().item():.3e} rad, eigenvalue abs err {err_l.max().item():.3e}, '
          f'smallest eigen-gap {want["gap"].min().item():.3f}')
    assert ang.max().item() <= 1e-4 and err_l.max().item() <= 1e-5
    torch.testing.assert_close(got.rot_mean.cpu().norm(dim=-1), torch.ones(ang.shape[0]), rtol=0, atol=1e-6)


def _cov_err(got, want):
    return ((got.trans_cov.double().cpu() - want['cov']).flatten(1).norm(dim=-1) / want['cov'].flatten(1).norm(dim=-1))


def _run(backend, S, B, dof, spread):
    from epropnp import posterior
    ps, lw, ref, good = _case(S, B, dof, spread)
    dev = [t.to(backend) for t in (ps, lw, ref)]
    got = posterior.summarize(*dev)
    return got, dev, good


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('S,B', SHAPES)
def test_first_moments_and_hygiene(backend, poisoned_empty, S, B, dof):
    """trans_mean to 1e-5 of |mean| + spread, the 4-DoF resultant / 6-DoF eigenvalue and score_te to 1e-5 absolute (the project's
    bar for per-object reductions), the quaternion mean to 1e-4 rad.  Under poisoned_empty every word of every row is written; two
    launches agree in every bit; the NaN poses under -inf log-weights (column 0, column 66) reach no sum; NaN, +inf and all--inf
    columns give NaN rows and leave their neighbours intact."""
    from epropnp import posterior
    got, dev, good = _run(backend, S, B, dof, 1.0)
    assert torch.equal(_bits(got.raw), _bits(posterior.summarize(*dev).raw)), 'two launches differ'
    raw = got.raw.cpu()
    assert raw.shape == (B, 16) and got.trans_mean.shape == (B, 3) and got.trans_cov.shape == (B, 3, 3)
    assert got.rot_mean.shape == ((B,) if dof == 4 else (B, 4)) and got.rot_resultant.shape == got.score_te.shape == (B,)
    assert bool(torch.isfinite(raw[good]).all()), 'a word was not written, or a zero-weight NaN pose reached a sum'
    assert torch.equal(_bits(got.trans_cov), _bits(got.trans_cov.transpose(1, 2))) and bool((raw[good, 15] == 0).all())
    if dof == 4:
        assert bool((raw[good, 12:15] == 0).all())
    for b in (EDGE if B >= 70 else ()):
        assert bool(torch.isnan(raw[b]).all()), (b, raw[b])
    ps, lw, ref, _ = _case(S, B, dof, 1.0)
    want = _fp64(ps[:, good], lw[:, good], ref[good], key=(S, B, dof, 1.0))
    sel = type(got)(*[None if f is None else f[good] for f in got])
    _check_first_moments(sel, want, f'posterior S={S} B={B} dof={dof}')
    if S > 1:
        assert bool((want['score'] > 0.05).any()) and bool((want['score'] < 0.95).any())       # the clamp is not all there is
    if dof == 6:
        _check_quaternion(sel, want, f'posterior S={S} B={B}')
        assert bool(((sel.rot_mean.cpu() * ref[good, 3:]).sum(-1) >= 0).all())
    else:
        d = (sel.rot_mean.double().cpu() - want['yaw'] + math.pi) % (2 * math.pi) - math.pi
        sharp = want['resultant'] > 0.1
        print(f'posterior S={S} B={B}: circular mean abs err {d[sharp].abs().max().item():.3e} rad')
        assert d[sharp].abs().max().item() <= 1e-5
    # without pose_ref: no score, everything else keeps its bits (the 6-DoF sign apart)
    bare = posterior.summarize(dev[0], dev[1])
    assert bare.score_te is None and bool(torch.isnan(bare.raw[:, 9]).all())
    keep = [i for i in range(16) if i != 9 and (dof == 4 or i < 11 or i == 15)]
    assert torch.equal(_bits(bare.raw[:, keep]), _bits(got.raw[:, keep]))


@pytest.mark.parametrize('shift', [0.0, 4 * math.pi])
@pytest.mark.parametrize('S,B', [(64, 3), (510, 70)])
def test_circular_mean_wraps(backend, poisoned_empty, S, B, shift):
    """Yaws pi +- d in pairs of equal weight, d ~ 0.05, stored wrapped into (-pi, pi] (so half of them sit at -pi + d) or shifted by
    4 pi: the circular mean is pi modulo 2 pi to 1e-5 rad (the pairs' fp32 roundings of pi +- d are 5e-7 at most), and the fp64 mean
    of the same fp32 yaws is met to 1e-5 too."""
    from epropnp import posterior
    g = torch.Generator().manual_seed(7 + S)
    d = 0.05 * torch.randn(S // 2, B, generator=g, dtype=torch.float64)
    yaw = torch.cat((math.pi + d, math.pi - d), 0)
    yaw = (torch.where(yaw > math.pi, yaw - 2 * math.pi, yaw) + shift).float()
    half = torch.rand(S // 2, B, generator=g) * 8.0 - 4.0
    lw = torch.cat((half, half), 0)
    ps = torch.cat((torch.randn(S, B, 3, generator=g), yaw[..., None]), -1).contiguous()
    got = posterior.summarize(ps.to(backend), lw.to(backend))
    want = _fp64(ps, lw, torch.zeros(B, 4))
    off_pi = (got.rot_mean.double().cpu() - math.pi + math.pi) % (2 * math.pi) - math.pi
    off_64 = (got.rot_mean.double().cpu() - want['yaw'] + math.pi) % (2 * math.pi) - math.pi
    print(f'circular mean S={S} B={B} shift={shift:.2f}: |mean - pi| {off_pi.abs().max().item():.3e}, against fp64 {off_64.abs().max().item():.3e}')
    assert off_pi.abs().max().item() <= 1e-5 and off_64.abs().max().item() <= 1e-5
    assert (got.rot_resultant.double().cpu() - want['resultant']).abs().max().item() <= 1e-5


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('S,B', SHAPES)
def test_second_moments_offset_case(backend, poisoned_empty, S, B, dof):
    """trans_cov of translations (2, 1, 50) + 0.05 randn against fp64, relative to its Frobenius norm.  A sum without a pivot
    (E[t^2] - mean^2 at depth 50, spread 0.05) errs by more than 1e-2 here; the bar is 4 x the largest error measured, and <= 1e-4.

    Largest error measured over the eight cases: 1.651e-6 on the CPU emulation (S=510 B=70, 6-DoF); on the MI355X: NOT measured."""
    assert COV_BAR <= 1e-4
    got, dev, good = _run(backend, S, B, dof, 0.05)
    ps, lw, ref, _ = _case(S, B, dof, 0.05)
    want = _fp64(ps[:, good], lw[:, good], ref[good], key=(S, B, dof, 0.05))
    sel = type(got)(*[None if f is None else f[good] for f in got])
    err = _cov_err(sel, want)
    multi = want['cov'].flatten(1).norm(dim=-1) > 0               # (one sample: the covariance is exactly zero on both sides)
    print(f'posterior S={S} B={B} dof={dof}: trans_cov rel Frobenius err {(err[multi].max().item() if bool(multi.any()) else 0.0):.3e}')
    assert bool((sel.trans_cov.cpu()[~multi] == 0).all())
    if bool(multi.any()):
        assert err[multi].max().item() <= COV_BAR
    _check_first_moments(sel, want, f'posterior (offset case) S={S} B={B} dof={dof}')


def test_quaternion_sign_invariance_and_sign_choice(backend, poisoned_empty):
    """Flipping the sign of any subset of the input quaternions changes no bit of the row; the mean points towards pose_ref's
    quaternion when there is one (so -pose_ref gives the negated mean), else its first non-zero component is positive."""
    from epropnp import posterior
    S, B = 510, 70
    ps, lw, ref, good = _case(S, B, 6, 1.0)
    g = torch.Generator().manual_seed(5)
    flip = torch.where(torch.rand(S, B, 1, generator=g) < 0.5, -1.0, 1.0)
    flipped = torch.cat((ps[..., :3], ps[..., 3:] * flip), -1).contiguous()
    dev = [t.to(backend) for t in (ps, lw, ref)]
    a = posterior.summarize(*dev)
    b = posterior.summarize(flipped.to(backend), dev[1], dev[2])
    assert torch.equal(_bits(a.raw), _bits(b.raw))
    neg = torch.cat((ref[:, :3], -ref[:, 3:]), -1).contiguous()
    c = posterior.summarize(dev[0], dev[1], neg.to(backend))
    assert torch.equal(_bits(c.rot_mean[good]), _bits(-a.rot_mean[good])) and torch.equal(_bits(c.raw[:, :11]), _bits(a.raw[:, :11]))
    assert bool(((a.rot_mean[good].cpu() * ref[good, 3:]).sum(-1) > 0).all())
    bare = posterior.summarize(flipped.to(backend), dev[1]).rot_mean[good].cpu()
    first = bare.gather(1, (bare != 0).float().argmax(1, keepdim=True))
    assert bool((first > 0).all())
    assert bool((_angle(bare, a.rot_mean[good].cpu()) == 0).all())


# ---- resampling ------------------------------------------------------------------------------------------------------
def _check_draws(index, poses, ps, lw, good, R):
    S, B = lw.shape
    index, poses = index.cpu(), poses.cpu()
    assert index.shape == (R, B) and index.dtype == torch.int32 and poses.shape == (R, B, ps.shape[-1])
    idx = index[:, good].long()
    assert bool(((idx >= 0) & (idx < S)).all()), 'an index was not written (or is out of range)'
    assert bool((idx[1:] >= idx[:-1]).all()), 'indices decrease in r'
    w = torch.softmax(lw[:, good].double(), dim=0)
    counts = torch.zeros(S, len(good), dtype=torch.float64).scatter_add_(0, idx, torch.ones(R, len(good), dtype=torch.float64))
    assert bool((counts[lw[:, good] == float('-inf')] == 0).all()), 'a zero-weight sample was drawn'
    off = (counts - R * w).abs().max().item()
    print(f'resample S={S} B={B} R={R}: max |count - R w| = {off:.6f}')
    assert off < 1 + 1e-3
    cols = torch.tensor(good)
    assert torch.equal(_bits(poses[:, good]), _bits(ps[idx, cols[None, :]])), 'poses are not pose_samples[index, b]'
    for b in range(B):
        if b not in good:
            assert bool((index[:, b] == -1).all()) and bool(torch.isnan(poses[:, b]).all())


@pytest.mark.parametrize('R', [1, 64, 1000])
@pytest.mark.parametrize('S,B,dof', [(1, 1, 4), (64, 3, 6), (510, 70, 4), (510, 70, 6), (4096, 2, 6)])
def test_systematic_resampling(backend, poisoned_empty, S, B, dof, R):
    """With injected u: every index is written, in [0, S), non-decreasing in r; zero-weight samples are never drawn; every sample's
    count is within 1 (+ 1e-3) of R times its fp64 weight; the gathered poses are the indexed samples bit for bit; bad and empty
    columns get -1 / NaN; two launches agree."""
    from epropnp import posterior
    ps, lw, _, good = _case(S, B, dof, 1.0)
    u = torch.rand(B, generator=torch.Generator().manual_seed(R + S))
    dev = [t.to(backend) for t in (ps, lw)]
    index, poses = posterior.resample(*dev, R, u=u.to(backend))
    _check_draws(index, poses, ps, lw, good, R)
    again, none = posterior.resample(*dev, R, u=u.to(backend), with_poses=False)
    assert none is None and torch.equal(again, index)


@pytest.mark.parametrize('S,B', [(64, 3), (510, 70)])
def test_resampling_at_the_last_threshold(backend, poisoned_empty, S, B):
    """u = 1 - 2^-24, R = 1000: (u + R - 1) / R rounds to 1, the last threshold to the total weight itself -- every draw is still
    written; and flat weights with u = 1/2: draw r is sample r of S = R."""
    from epropnp import posterior
    ps, lw, _, good = _case(S, B, 6, 1.0)
    u = torch.full((B,), 1.0 - 2.0 ** -24)
    assert float(u[0]) < 1.0 and float(((u + 999.0) / 1000.0)[0]) == 1.0
    index, poses = posterior.resample(ps.to(backend), lw.to(backend), 1000, u=u.to(backend))
    _check_draws(index, poses, ps, lw, good, 1000)
    flat = torch.zeros(S, B)
    index, _ = posterior.resample(ps.to(backend), flat.to(backend), S, u=torch.full((B,), 0.5).to(backend), with_poses=False)
    assert torch.equal(index.cpu().long(), torch.arange(S)[:, None].expand(S, B))


def test_resampling_with_the_philox_stream(backend, poisoned_empty):
    """u == NULL: the same (seed, offset) gives identical bits, another offset other indices for at least one of 70 objects, and
    seed=None takes its seed from torch's generator."""
    from epropnp import posterior
    S, B, R = 510, 70, 64
    ps, lw, _, good = _case(S, B, 4, 1.0)
    dev = [t.to(backend) for t in (ps, lw)]
    a = posterior.resample(*dev, R, seed=1234, offset=5)
    b = posterior.resample(*dev, R, seed=1234, offset=5)
    c = posterior.resample(*dev, R, seed=1234, offset=6)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert not torch.equal(a[0][:, good], c[0][:, good])
    _check_draws(a[0], a[1], ps, lw, good, R)
    _check_draws(c[0], c[1], ps, lw, good, R)
    torch.manual_seed(3)
    d = posterior.resample(*dev, R)
    torch.manual_seed(3)
    e = posterior.resample(*dev, R)
    assert torch.equal(d[0], e[0])
    _check_draws(d[0], d[1], ps, lw, good, R)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_refuses_other_dtypes_shapes_and_sizes(backend):
    from epropnp import posterior
    ps, lw = torch.zeros(8, 3, 7, device=backend), torch.zeros(8, 3, device=backend)
    with pytest.raises(TypeError):
        posterior.summarize(ps.double(), lw)
    with pytest.raises(TypeError):
        posterior.summarize(ps, lw.half())
    with pytest.raises(TypeError):
        posterior.resample(ps, lw.double(), 4)
    with pytest.raises(TypeError):
        posterior.resample(ps, lw, 4, u=torch.zeros(3, dtype=torch.float64, device=backend))
    with pytest.raises(ValueError):
        posterior.summarize(ps[..., :5].contiguous(), lw)
    with pytest.raises(ValueError):
        posterior.summarize(ps, lw[:4])
    with pytest.raises(ValueError):
        posterior.summarize(ps, lw, torch.zeros(3, 4, device=backend))
    with pytest.raises(ValueError):
        posterior.resample(ps, lw, 0)
    # inputs that require grad are detached: nothing is differentiable
    out = posterior.summarize(ps.clone().requires_grad_(True), lw.clone().requires_grad_(True))
    assert not out.raw.requires_grad and not out.trans_cov.requires_grad


def test_refuses_cpu_tensors_without_a_fallback():
    from epropnp import posterior
    import install as emu
    assert not emu.installed()
    with pytest.raises(RuntimeError, match='HIP device'):
        posterior.summarize(torch.zeros(8, 3, 4), torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match='HIP device'):
        posterior.resample(torch.zeros(8, 3, 4), torch.zeros(8, 3), 4)


def test_empty_batch_returns_empty_tensors_without_a_launch(backend, monkeypatch):
    from epropnp import _hip, posterior
    monkeypatch.setattr(_hip, 'call', lambda *a: (_ for _ in ()).throw(AssertionError('launched for an empty batch')))
    for P in (4, 7):
        ps, lw = torch.zeros(8, 0, P, device=backend), torch.zeros(8, 0, device=backend)
        s = posterior.summarize(ps, lw, torch.zeros(0, P, device=backend))
        assert s.raw.shape == (0, 16) and s.trans_mean.shape == (0, 3) and s.trans_cov.shape == (0, 3, 3) and s.score_te.shape == (0,)
        assert s.rot_mean.shape == ((0,) if P == 4 else (0, 4))
        index, poses = posterior.resample(ps, lw, 5)
        assert index.shape == (5, 0) and index.dtype == torch.int32 and poses.shape == (5, 0, P)


# ---- through the layer -------------------------------------------------------------------------------------------------
RSLM = dict(num_points=16, num_proposals=16, num_iter=3)
LAYER_CASES = {'4dof': dict(dof=4, B=6, N=128, S=64, K=4, L=5, normalize=True, rslm=True, bounds='tensor'),
               '6dof': dict(dof=6, B=5, N=96, S=64, K=4, L=3, normalize=False, rslm=False, bounds=None)}


def _forward(case, backend, summarize):
    from epropnp import functional as F
    from epropnp import posterior
    from epropnp.epropnp import EProPnP4DoF, EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver, RSLMSolver
    c = LAYER_CASES[case]
    dof, B, S, K = c['dof'], c['B'], c['S'], c['K']
    prob = orc.make_problem(B, c['N'], dof, seed=3, bounds=c['bounds'])
    prob['pose_init'][0, :3] += 3.0
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=4), dof).to(backend)
    p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
    cf.set_param(p['x2d'], p['w2d'])
    init = None
    if c['rslm']:
        rn = orc.make_rslm_noise(prob, dof, RSLM['num_points'], RSLM['num_proposals'], seed=5)
        init = RSLMSolver(dof=dof, **RSLM)
        init.draw = lambda w: (rn['inds'].to(backend), rn['rot'].float().to(backend))
    layer = (EProPnP6DoF if dof == 6 else EProPnP4DoF)(mc_samples=S, num_iter=K, normalize=c['normalize'],
                                                      solver=LMSolver(dof=dof, num_iter=c['L'], init_solver=init))
    summary = None
    with F.diagnostics() as d:
        out = layer.monte_carlo_forward(p['x3d'], p['x2d'], p['w2d'], cam, cf, pose_init=p['pose_init'],
                                        force_init_solve=c['rslm'], noise=noise, fast_mode=True)
        if summarize:
            summary = posterior.summarize(out[3], out[4], out[0])
    assert len(d.records) == 1
    return out, d.records[0], summary


@pytest.mark.parametrize('case', ['4dof', '6dof'])
def test_through_the_layer(backend, poisoned_empty, case):
    """monte_carlo_forward(fast_mode=True) of the two diagnostics cases: summarize(pose_samples, logweights, pose_opt) meets the
    bars above on the layer's own samples, and changes nothing -- outputs and the diagnostics record's ess are torch.equal with and
    without the call."""
    plain, rec0, _ = _forward(case, backend, False)
    out, rec, got = _forward(case, backend, True)
    for a, b in zip(plain, out):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert torch.equal(_bits(rec.ess), _bits(rec0.ess)) and torch.equal(_bits(rec.weight_stats), _bits(rec0.weight_stats))
    want = _fp64(out[3].detach().cpu(), out[4].detach().cpu(), out[0].detach().cpu())
    assert bool(torch.isfinite(got.raw).all())
    _check_first_moments(got, want, f'through the layer {case}')
    err = _cov_err(got, want)
    print(f'through the layer {case}: trans_cov rel Frobenius err {err.max().item():.3e}')
    assert err.max().item() <= COV_BAR
    if case == '6dof':
        _check_quaternion(got, want, f'through the layer {case}')
        assert bool(((got.rot_mean * out[0][:, 3:]).sum(-1) >= 0).all())
    else:
        d = (got.rot_mean.double().cpu() - want['yaw'] + math.pi) % (2 * math.pi) - math.pi
        assert d.abs().max().item() <= 1e-5


# ---- hipGraph ----------------------------------------------------------------------------------------------------------
def _graph_body():
    from epropnp import posterior
    dev = torch.device('cuda:0')
    S, B, R = 510, 70, 64
    outs = {}
    for dof in (4, 6):
        ps, lw, ref, _ = _case(S, B, dof, 1.0)
        ps, lw, ref = ps.to(dev), lw.to(dev), ref.to(dev)
        u = torch.rand(B, generator=torch.Generator().manual_seed(dof)).to(dev)

        def body():
            s = posterior.summarize(ps, lw, ref)
            index, poses = posterior.resample(ps, lw, R, u=u)
            return s.raw, s.trans_cov, index, poses

        eager = [t.clone() for t in body()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs[dof] = body()
        for t in outs[dof]:
            t.fill_(float('nan') if t.is_floating_point() else -7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs[dof]):
            assert torch.equal(_bits(a), _bits(b)), f'dof {dof}: replay differs from the eager call'
        del graph
        outs.clear()
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_summarize_and_resample_replay_from_a_hip_graph():
    """summarize and resample (injected u) captured on the capture stream into one torch.cuda.graph, replayed once: bit-equal to the
    eager calls.  Own interpreter, as tests/test_graph_rng.py: keeps graph / private-pool teardown away from the other GPU tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys; sys.path[:0] = [%r, %r, %r]; import test_posterior as t; t._graph_body(); '
            'print("POSTERIOR-GRAPH-OK", flush=True)') % (here, os.path.join(os.path.dirname(here), 'oracle'),
                                                           os.path.join(os.path.dirname(here), 'epro-pnp_amd'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'POSTERIOR-GRAPH-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
