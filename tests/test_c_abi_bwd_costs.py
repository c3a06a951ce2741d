"""The sample-cost additions to the C ABI (epropnp_amis_forward_costs, epropnp_monte_carlo_forward_costs, epropnp_amis_backward_costs,
epropnp_amis_backward_split_costs, epropnp_request_sample_costs) are additive: same ABI version, the header is still plain C, the
entries validate their arguments as the entries they extend, and the Python layer refuses host tensors and wrong sizes for the
new arguments as it does for the old ones."""
import ctypes

import pytest
import torch

import epropnp_oracle as orc
from helpers import abi_lib, check_abi_additive, check_header_is_plain_c, make_layer_objects

NEW = ('epropnp_amis_forward_costs', 'epropnp_monte_carlo_forward_costs', 'epropnp_amis_backward_costs',
       'epropnp_amis_backward_split_costs', 'epropnp_request_sample_costs')


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_cost_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


def test_argument_validation_without_launch(lib):
    """The checks of the entries they extend, in the same order: problem, sizes, NULL outputs -- nothing is launched."""
    from epropnp import _hip
    bad_dof = _hip.Problem(None, None, None, None, None, None, None, 0.1, 4, 16, 5)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(bad_dof), *([None] * 2), 8, *([None] * 9)) == -1
    assert b'dof' in lib.epropnp_last_error()
    here = (ctypes.c_float * 4)()
    p = ctypes.addressof(here)
    prob = _hip.Problem(p, p, p, p, None, None, p, 0.1, 4, 128, 6)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(prob), None, None, 8, None, None, None, None, None, None, None, None, None) == -1
    assert b'NULL' in lib.epropnp_last_error()
    assert lib.epropnp_amis_backward_costs(ctypes.byref(prob), None, None, -1, *([None] * 9)) == -1
    assert b'negative' in lib.epropnp_last_error()
    assert lib.epropnp_amis_backward_split_costs(ctypes.byref(prob), p, p, 8, None, None, 3, None, None, p, p, p, p, None) == -1
    assert b'nsplit' in lib.epropnp_last_error()          # 3 x 64 > the 128 points
    par = _hip.AmisParams(10, 4, 1e-5, 3, 1e-3, 0, 0, None, None, 0)
    assert lib.epropnp_amis_forward_costs(ctypes.byref(prob), ctypes.byref(par), *([None] * 8)) == -1
    assert b'multiple' in lib.epropnp_last_error()
    empty = _hip.Problem(None, None, None, None, None, None, None, 0.1, 0, 128, 6)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(empty), *([None] * 2), 8, *([None] * 9)) == 0       # no objects: nothing to do
    assert lib.epropnp_request_sample_costs(None) == 0


def test_python_layer_refuses_wrong_sizes(backend):
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    B, N, S, dof = 2, 64, 16, 6
    prob = orc.make_problem(B, N, dof, seed=3)
    p, cam, _ = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    samples = p['pose_gt'].unsqueeze(0).repeat(S, 1, 1).contiguous()
    g_logw, g_init = torch.ones(S, B, device=backend), torch.ones(B, device=backend)
    costs, cinit = torch.ones(S, B, device=backend), torch.ones(B, device=backend)
    with pytest.raises(ValueError, match='sample_costs'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs[:-1], cost_init=cinit)
    with pytest.raises(ValueError, match='sample_costs'):
        F.amis_backward(hp, samples, g_logw, None, None, sample_costs=costs.t().contiguous())
    with pytest.raises(ValueError, match='cost_init'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=torch.ones(B + 1, device=backend))
    with pytest.raises(TypeError, match='fp32'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs.double(), cost_init=cinit)


@pytest.mark.gpu
def test_python_layer_refuses_host_tensors_for_the_costs():
    import install as emu
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    emu.uninstall()
    dev = torch.device('cuda:0')
    B, N, S, dof = 2, 64, 16, 6
    prob = orc.make_problem(B, N, dof, seed=3)
    p, cam, _ = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    samples = p['pose_gt'].unsqueeze(0).repeat(S, 1, 1).contiguous()
    g_logw, g_init = torch.ones(S, B, device=dev), torch.ones(B, device=dev)
    with pytest.raises(RuntimeError, match='HIP device'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=torch.ones(S, B), cost_init=torch.ones(B, device=dev))
    with pytest.raises(RuntimeError, match='HIP device'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=torch.ones(S, B, device=dev), cost_init=torch.ones(B))


def _same_bits(old, new, what):
    assert len(old) == len(new), what
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, i)


@pytest.mark.parametrize('with_init', [True, False], ids=['pose_init', 'no_pose_init'])
@pytest.mark.parametrize('dof', [6, 4])
def test_old_entries_are_their_supersets_with_null_extras(backend, dof, with_init):
    """The package calls only the superset entries (epropnp/functional.py); the entries they extend stay in the ABI for other callers.
    Each old entry against its superset with NULL extras, and the request side channel / the _diag entry against the _costs entry
    with the same extras, through raw pointers into NaN- / -7-filled buffers: every output to the bits.
    B = 3, N = 100 (no multiple of 64; two chunks for nsplit 2), S = 32, K = 4; with pose_init the one-call forward runs
    init_mode 2 (random-sample initialiser and pose_init), without it init_mode 1."""
    from epropnp import _hip
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    B, N, S, K, PL = 3, 100, 32, 4, 7 if dof == 6 else 4
    prob = orc.make_problem(B, N, dof, seed=61, bounds='tensor' if dof == 4 else None)
    p, cam, _ = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    ptr, ref = _hip.ptr, ctypes.byref
    nan = lambda *s: torch.full(s, float('nan'), device=backend)
    ints = lambda *s: torch.full(s, -7, dtype=torch.int32, device=backend)
    lm = _hip.LmParams(3, 0, 1e-6, 1e32, 1e-3, 30.0, 1e16, 1e-5)
    amis = _hip.AmisParams(S, K, 1e-5, 3, 0.001, 7, 2, None, None, 0)
    pin = p['pose_init'].contiguous() if with_init else None

    # ---- epropnp_rslm_solve | epropnp_rslm_solve_diag: same seed and offset, winner NULL, then with the winner
    def rslm(entry, *winner):
        pose, cost = nan(B, PL), nan(B)
        _hip.call(entry, ref(hp.c), ref(lm), 16, 8, 5, 3, None, None, None, ptr(pose), ptr(cost), None, 0, *winner, hp.stream)
        return [pose, cost]
    old = rslm('epropnp_rslm_solve')
    _same_bits(old, rslm('epropnp_rslm_solve_diag', None), 'rslm_solve')
    winner = ints(B)
    _same_bits(old, rslm('epropnp_rslm_solve_diag', ptr(winner)), 'rslm_solve with winner')
    assert bool(((winner >= 0) & (winner < 16)).all())

    # ---- epropnp_amis_forward | epropnp_amis_forward_costs
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)

    def forward(entry, *costs):
        samples, logw, props = nan(S, B, PL), nan(S, B), nan(B, K, 40)
        _hip.call(entry, ref(hp.c), ref(amis), ptr(pose_opt), ptr(pose_cov), None, ptr(samples), ptr(logw), ptr(props), *costs,
                  hp.stream)
        return [samples, logw, props]
    old = forward('epropnp_amis_forward')
    _same_bits(old, forward('epropnp_amis_forward_costs', None), 'amis_forward')
    costs = nan(S, B)
    _same_bits(old, forward('epropnp_amis_forward_costs', ptr(costs)), 'amis_forward with costs')
    assert bool(torch.isfinite(costs).all())
    samples = old[0]

    # ---- epropnp_amis_backward[_split] | epropnp_amis_backward[_split]_costs
    g = torch.Generator().manual_seed(62)
    g_logw = torch.randn(S, B, generator=g).to(backend)
    gin = torch.randn(B, generator=g).to(backend) if with_init else None

    def backward(entry, nsplit, *costs):
        grads = [nan(B, N, 3), nan(B, N, 2), nan(B, N, 2), nan(B, nsplit) if nsplit > 1 else nan(B)]
        _hip.call(entry, ref(hp.c), ptr(samples), ptr(g_logw), S, ptr(pin), ptr(gin), *((nsplit,) if nsplit > 1 else ()), *costs,
                  *(ptr(t) for t in grads), hp.stream)
        return grads
    _same_bits(backward('epropnp_amis_backward', 1), backward('epropnp_amis_backward_costs', 1, None, None), 'amis_backward')
    assert F.launch_plan('backward', hp, S, pose_init=with_init, nsplit=2)['nsplit'] == 2
    _same_bits(backward('epropnp_amis_backward_split', 2), backward('epropnp_amis_backward_split_costs', 2, None, None),
               'amis_backward_split')

    # ---- epropnp_monte_carlo_forward[_diag] (+ epropnp_request_sample_costs) | epropnp_monte_carlo_forward_costs
    par = _hip.McParams()
    par.lm, par.amis, par.rslm_lm = lm, amis, lm
    par.normalize, par.init_mode = 1, 2 if with_init else 1
    par.rslm_points, par.rslm_proposals, par.rslm_seed, par.rslm_offset = 8, 16, 5, 3

    def one_call(entry, *extras, request=None, also=()):
        out = [nan(B, N, 3), nan(B, 3), nan(B, PL) if with_init else None, nan(B, PL), nan(B), nan(B, PL), nan(B, dof, dof), nan(B),
               nan(S, B, PL), nan(S, B), nan(B) if with_init else None, nan(B, PL), nan(S, B, PL)]
        if request is not None:
            _hip.call('epropnp_request_sample_costs', ptr(request))
        _hip.call(entry, ref(hp.c), ref(par), ptr(pin), None, *(ptr(t) for t in out), *extras, hp.stream)
        return [t for t in out if t is not None] + list(also)
    old = one_call('epropnp_monte_carlo_forward')
    assert all(bool(torch.isfinite(t).all()) for t in old)
    _same_bits(old, one_call('epropnp_monte_carlo_forward_costs', None, None), 'monte_carlo_forward')
    c_old, c_new = nan(S, B), nan(S, B)
    _same_bits(one_call('epropnp_monte_carlo_forward', request=c_old, also=[c_old]),
               one_call('epropnp_monte_carlo_forward_costs', None, ptr(c_new), also=[c_new]), 'monte_carlo_forward after a request')
    assert bool(torch.isfinite(c_new).all())

    def diag():
        rec = [ints(B), ints(B), nan(B, K, 40), nan(B, K + 3)]
        return rec, ref(_hip.Diag(*(ptr(t) for t in rec)))
    rec_old, dg_old = diag()
    rec_new, dg_new = diag()
    _same_bits(one_call('epropnp_monte_carlo_forward_diag', dg_old, also=rec_old),
               one_call('epropnp_monte_carlo_forward_costs', dg_new, None, also=rec_new), 'monte_carlo_forward_diag')
    assert bool(torch.isfinite(rec_new[3]).all()) and bool((rec_new[1] >= -1).all())
