"""The diagnostics additions to the C ABI (epropnp_diag, epropnp_monte_carlo_forward_diag, epropnp_rslm_solve_diag,
epropnp_weight_stats) are additive: same ABI version, the header is still plain C, the struct matches its ctypes mirror, and the
forward entries with and without a diag are one."""
import ctypes

import pytest
import torch

import epropnp_oracle as orc
from helpers import abi_lib, check_abi_additive, check_header_is_plain_c, make_layer_objects, pack_noise

NEW = ('epropnp_monte_carlo_forward_diag', 'epropnp_rslm_solve_diag', 'epropnp_weight_stats')


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_diag_struct_is_plain_c_and_matches_ctypes(tmp_path):
    from epropnp import _hip
    fields = [f for f, _ in _hip.Diag._fields_]
    assert fields == ['lm_accept_mask', 'rslm_winner', 'proposals', 'weight_stats']
    body = ['epropnp_diag d = {0, 0, 0, 0};', 'printf("size %zu\\n", sizeof(d));']
    body += [f'printf("{f} %zu\\n", offsetof(epropnp_diag, {f}));' for f in fields]
    got = check_header_is_plain_c(tmp_path, NEW, run=True, body=body)      # (linked and run: the symbols must link)
    assert int(got['size']) == ctypes.sizeof(_hip.Diag)
    for f in fields:
        assert int(got[f]) == getattr(_hip.Diag, f).offset, f


def test_weight_stats_validates_without_launching(lib):
    assert lib.epropnp_weight_stats(None, 64, 0, 4, None, None) == 0            # no objects: nothing to do
    assert lib.epropnp_weight_stats(None, 64, 3, 4, None, None) == -1 and b'NULL' in lib.epropnp_last_error()


@pytest.mark.parametrize('how', ['null', 'empty'])
def test_forward_diag_without_a_diag_is_the_plain_entry(backend, monkeypatch, poisoned_empty, how):
    """The package's one-call forward is epropnp_monte_carlo_forward_costs with diag = NULL.  Routed from the outside through the
    entries it extends -- epropnp_request_sample_costs, then epropnp_monte_carlo_forward ('null') or epropnp_monte_carlo_forward_diag
    with a struct of NULLs ('empty') -- the layer returns the same bits, gradients included (the backward reads the samples' costs)."""
    from epropnp import _hip
    from epropnp.epropnp import EProPnP4DoF
    from epropnp.levenberg_marquardt import LMSolver, RSLMSolver
    B, N, S, K = 5, 70, 32, 2
    prob = orc.make_problem(B, N, 4, seed=3, bounds='tensor')
    prob['pose_init'][0, :3] += 3.0
    noise = pack_noise(orc.make_noise(B, S, K, 4, seed=4), 4).to(backend)
    rn = orc.make_rslm_noise(prob, 4, 8, 16, seed=5)
    # the ctypes node, whose host call can be re-routed from here (a C++ node loaded earlier in the process stays cached whatever
    # EPROPNP_NO_TORCH_EXT says now)
    monkeypatch.setattr(_hip, 'torch_ext', lambda: None)
    real_call, routed = _hip.call, []

    def via_old_entries(name, *args):
        if name != 'epropnp_monte_carlo_forward_costs':
            return real_call(name, *args)
        routed.append(name)
        *plain, diag, costs, stream = args
        assert diag is None and costs is not None
        real_call('epropnp_request_sample_costs', costs)
        if how == 'null':
            return real_call('epropnp_monte_carlo_forward', *plain, stream)
        return real_call('epropnp_monte_carlo_forward_diag', *plain, ctypes.byref(_hip.Diag(None, None, None, None)), stream)
    outs = []
    for patched in (False, True):
        if patched:
            monkeypatch.setattr(_hip, 'call', via_old_entries)
        p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
        x3d, x2d, w2d = (p[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d'))
        cf.set_param(x2d.detach(), w2d)
        init = RSLMSolver(dof=4, num_points=8, num_proposals=16, num_iter=3)
        init.draw = lambda w: (rn['inds'].to(backend), rn['rot'].float().to(backend))
        layer = EProPnP4DoF(mc_samples=S, num_iter=K, normalize=True, solver=LMSolver(dof=4, num_iter=3, init_solver=init))
        out = layer.monte_carlo_forward(x3d, x2d, w2d, cam, cf, pose_init=p['pose_init'], force_init_solve=True, with_cost=True,
                                        noise=noise)
        (out[5] + torch.logsumexp(out[4], 0)).mean().backward()
        outs.append([t.detach().clone() for t in out if t is not None] + [x3d.grad, x2d.grad, w2d.grad])
    assert routed == ['epropnp_monte_carlo_forward_costs']
    for a, b in zip(*outs):
        assert torch.equal(a, b)
