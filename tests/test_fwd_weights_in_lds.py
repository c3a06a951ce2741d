"""AMIS forward: the per-tile weights (w_u, w_v, -u w_u, -v w_v) of the resident point tiles in LDS instead of registers
(amis_forward_mfma.hip: WLDS; the 6-DoF bf16 kernel with 4 waves x 8 tiles, compiled for four waves per SIMD), the refit's reduction
scratch at half size on the partial-cost rows (amis_common.h: amis_refit<DOF, true>).

The weights are the same floats read from another place, huber_cost_4 and its order are untouched, and a row of the refit's
transposed sums does not depend on which rows share its pass: the bar is equality of bits.  Every case compares
EPROPNP_TUNE=fwd_wlds=1 with fwd_wlds=0 through int32 views (NaNs included): pose_samples, logweights, the sample costs, the proposal
records and the status word.

Shapes: B = 3 under fwd_mfma=4,8 (small batches otherwise take 8 waves x 4 tiles) and EPROPNP_FWD_SPLIT=1 (a small batch on a whole
device is otherwise split over workgroups, which the new instantiation is not); N = 512 (all 32 tiles full) and N = 260 (17 tiles, the
rest zero-weight padding, the last tile partly filled); S = 64, K = 4 (one full pose tile per iteration) and S = 40, K = 2 (s = 20: a
padded second pose tile).  The plan record keeps its eight ints, so _wlds_bytes restates the launcher's LDS rule: a case fails if the
shape is not the instantiated one or would not fit, i.e. if fwd_wlds=1 could not have taken the new path."""
import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise, set_tune

B = 3
REFIT_HALF_FLOATS = 11 * 68 + 24      # amis_common.h: kRefitHalfFloats
SHAPES = [(64, 4), (40, 2)]


def _wlds_bytes(S, K, waves=4, tiles=8):
    """plan_amis_forward's lds_bytes(false, true) for 6-DoF in register mode: pose table | sampler state | partial-cost rows that
    also hold the half-size refit scratch | proposals | red | weights | the noise drawn ahead unless it shares the pose table"""
    s = S // K
    s16 = (s + 15) // 16 * 16
    floats = (12 * s16 + ((10 * S + 3) & ~3) + max(waves * s16, REFIT_HALF_FLOATS) + 40 * K + 256 + 64 * waves * tiles +
              (0 if s <= 64 * waves else 8 * s))
    return 4 * floats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _problem(dev, bounds, N, seed=71):
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    prob = orc.make_problem(B, N, 6, seed=seed, bounds=bounds)
    p, cam, _ = make_layer_objects(prob, dev)
    return p, cam, lambda: F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), 6)


def _assert_new_path_possible(hp, S, K):
    from epropnp import functional as F
    plan = F.launch_plan('forward', hp, S, K, scratch=False)
    want = dict(waves=4, tiles=8, G=1, chunks=1, bf16=True, spilled=False, truncated=False, chunked=False)
    assert plan == want, plan
    assert _wlds_bytes(S, K) <= 160 * 1024


def _forward(monkeypatch, make, p, S, K, knob, noise, seed=0):
    """amis_forward with every output, under a status word of its own -> five tensors"""
    from epropnp import functional as F
    set_tune(monkeypatch, fwd_mfma='4,8', fwd_wlds=knob)
    cov = (torch.eye(6) * torch.tensor([0.02, 0.02, 0.3, 1e-3, 1e-3, 1e-3])).expand(B, 6, 6).contiguous().to(p['x3d'].device)
    with F.numerics_check():
        hp = make()
        _assert_new_path_possible(hp, S, K)
        out = F.amis_forward(hp, p['pose_gt'], cov, S, K, noise=noise, seed=seed, with_proposals=True, with_costs=True)
        status = F.status_buffer(hp.device).clone()
    return out + (status,)


def _same_bits(a, b, what):
    for name, x, y in zip(('pose_samples', 'logweights', 'proposals', 'sample_costs', 'status'), a, b):
        assert torch.equal(_bits(x), _bits(y)), (what, name)


@pytest.mark.parametrize('bounds', [None, 'tight'])
@pytest.mark.parametrize('S,K', SHAPES)
@pytest.mark.parametrize('N', [512, 260])
def test_weights_in_lds_keep_every_bit_of_the_forward(backend, monkeypatch, N, S, K, bounds):
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    p, _, make = _problem(backend, bounds, N)
    noise = pack_noise(orc.make_noise(B, S, K, 6, seed=72), 6).to(backend)
    runs = {knob: _forward(monkeypatch, make, p, S, K, knob, noise) for knob in (1, 0)}
    assert bool(torch.isfinite(runs[1][0]).all()) and bool(torch.isfinite(runs[1][3]).all())
    assert float(runs[1][3].abs().max()) > 0
    _same_bits(runs[1], runs[0], (N, S, K, bounds))


@pytest.mark.parametrize('S,K', SHAPES)
def test_weights_in_lds_with_the_kernels_own_draw(backend, monkeypatch, S, K):
    """no injected noise: the other waves draw the next iteration's base noise ahead, into the pose table's LDS, while wave 0's refit
    runs its reductions on the partial-cost rows"""
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    p, _, make = _problem(backend, None, 260)
    runs = {knob: _forward(monkeypatch, make, p, S, K, knob, None, seed=5) for knob in (1, 0)}
    assert bool(torch.isfinite(runs[1][0]).all()) and bool(torch.isfinite(runs[1][1]).all())
    _same_bits(runs[1], runs[0], (S, K))
    again = _forward(monkeypatch, make, p, S, K, 1, None, seed=5)
    _same_bits(runs[1], again, ('again', S, K))


def test_weights_in_lds_with_a_nan_weight(backend, monkeypatch):
    """a NaN weight of one point of object 1: the NaNs that come out carry the same bits, the other objects stay finite"""
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    S, K = SHAPES[0]
    p, _, make = _problem(backend, None, 260)
    p['w2d'] = p['w2d'].clone()
    p['w2d'][1, 200, 0] = float('nan')
    noise = pack_noise(orc.make_noise(B, S, K, 6, seed=72), 6).to(backend)
    runs = {knob: _forward(monkeypatch, make, p, S, K, knob, noise) for knob in (1, 0)}
    _same_bits(runs[1], runs[0], 'nan weight')
    costs = runs[1][3]
    assert bool(torch.isnan(costs[:, 1]).all()) and bool(torch.isfinite(costs[:, 0]).all()) and bool(torch.isfinite(costs[:, 2]).all())


def test_weights_in_lds_through_the_one_call_forward(backend, monkeypatch):
    """monte_carlo_forward with normalize=True: the forward also stores the samples and pose_opt in the caller's frame"""
    from epropnp import functional as F
    from epropnp.epropnp import EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    S, K = SHAPES[1]
    prob = orc.make_problem(B, 260, 6, seed=73)
    noise = pack_noise(orc.make_noise(B, S, K, 6, seed=74), 6).to(backend)
    p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
    runs = {}
    for knob in (1, 0):
        set_tune(monkeypatch, fwd_mfma='4,8', fwd_wlds=knob)
        x3d, x2d, w2d = (p[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d'))
        cf.set_param(x2d.detach(), w2d)
        layer = EProPnP6DoF(mc_samples=S, num_iter=K, normalize=True, solver=LMSolver(dof=6, num_iter=3))
        assert layer._fusable(x3d, x2d, w2d, p['pose_init'], False, dict(with_cost=True))
        _assert_new_path_possible(F.PlanProblem(B, 260, 6), S, K)
        out = layer.monte_carlo_forward(x3d, x2d, w2d, cam, cf, pose_init=p['pose_init'], force_init_solve=False, with_cost=True, noise=noise)
        runs[knob] = [t.detach().clone() for t in out if t is not None]
    assert len(runs[1]) == len(runs[0]) >= 4
    for i, (a, b) in enumerate(zip(runs[1], runs[0])):
        assert bool(torch.isfinite(a).all()), i
        assert torch.equal(_bits(a), _bits(b)), f'output {i} of monte_carlo_forward'
