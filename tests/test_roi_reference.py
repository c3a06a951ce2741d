"""epropnp.roi and epropnp.losses.MVDGaussianMixtureNLLLoss against the REFERENCE's inter_roi_ops.py and
mvd_gaussian_mixture_nll_loss.py (EPro-PnP-Det), through tests/golden/roi_across.npz: inputs, the reference's logsumexp_across_rois,
logsoftmax_across_rois(extra_dim=1), its autograd gradient for a stored cotangent, the loss module's 'none' output and its buffer,
written by tools/make_roi_golden.py.  The generator fences the boxes (no cell centre within 1e-3 of a border of a neighbour's box), so
both sides pair and mask the same cells; what is left is fp32 rounding on the reference's side -- it rounds the sampling grid through
the overlap box -- and one rounding per output on the package's, compared at test_roi.FWD_BAR / BWD_BAR (whose measured worst cases
count the figures printed here too).

The last test re-runs the live reference where its checkout exists (build container only) and checks that the fixture is still what
it returns."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_roi as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'roi_across.npz')
SHAPES = {'a': (9, 2, 3, 5, 7), 'b': (6, 1, 8, 14, 14), 'c': (5, 2, 1, 28, 28)}
TARGET = {'a': 'tensor', 'b': -1, 'c': 0}
RESULTS = ('logsumexp', 'logsoftmax_dim1', 'grad', 'loss', 'mean_inv_std')


def _case(name):
    z = np.load(GOLDEN)
    n, _, c, rh, rw = SHAPES[name]
    x, cot = torch.from_numpy(z[f'{name}_x_q4']).float() / 4, torch.from_numpy(z[f'{name}_cot_q4']).float() / 4
    assert x.shape == (n, c, rh, rw)
    return z, x, cot, torch.from_numpy(z[f'{name}_rois'])


@pytest.mark.parametrize('name', list(SHAPES))
def test_against_the_recorded_reference(backend, name):
    from epropnp import roi
    z, x, cot, rois = _case(name)
    assert tr.fence_distance(rois, x.shape[2], x.shape[3]) >= tr.FENCE
    xd = x.clone().to(backend).requires_grad_(True)
    lse = roi.logsumexp_across_rois(xd, rois.to(backend))
    grad = torch.autograd.grad((lse * cot.to(backend)).sum(), xd)[0]
    lsm = roi.logsoftmax_across_rois(x.to(backend), rois.to(backend), extra_dim=1)
    want = torch.from_numpy(z[f'{name}_logsumexp']).double()
    assert (want != x.double()).flatten(1).any(1).sum() * 2 >= len(x)
    tr.check('forward', f'recorded {name}', tr.fwd_error(lse.detach(), want), tr.FWD_BAR)
    tr.check('forward', f'recorded {name}, logsoftmax(extra_dim=1)',
             tr.fwd_error(lsm, torch.from_numpy(z[f'{name}_logsoftmax_dim1']).double()), tr.FWD_BAR)
    tr.check('backward', f'recorded {name}', tr.bwd_error(grad, torch.from_numpy(z[f'{name}_grad']).double()), tr.BWD_BAR)


@pytest.mark.parametrize('name', list(SHAPES))
def test_loss_against_the_recorded_reference(backend, name):
    from epropnp.losses import MVDGaussianMixtureNLLLoss
    z, _, _, rois = _case(name)
    q8 = lambda k: torch.from_numpy(z[f'{name}_{k}_q8']).float() / 8
    pred, logstd, logmix = q8('pred'), q8('logstd'), q8('logmixweight')
    target = q8('target') if TARGET[name] == 'tensor' else TARGET[name]
    m = MVDGaussianMixtureNLLLoss(reduction='none').to(backend)
    dev = lambda t: t.to(backend) if torch.is_tensor(t) else t
    got = m(dev(pred), dev(target), logstd=dev(logstd), logmixweight=dev(logmix), rois=rois.to(backend))
    want = torch.from_numpy(z[f'{name}_loss']).double()
    assert got.shape == want.shape
    _, mean, scale = tr.mvd_restated(pred, target, logstd, logmix, rois, 1.0, True)
    # two fp32 evaluations of the same chain (~40 rounded operations on terms up to `scale`, 2^-24 each), with 4 x headroom
    err = float((got.double().cpu() - want).abs().max())
    print(f'recorded {name}: loss differs by {err:.3e} (terms up to {scale:.1f}); buffer {float(m.mean_inv_std):.7f}')
    assert err <= 1e-5 * max(1.0, scale, float(want.abs().max())) / min(1.0, mean)
    assert abs(float(m.mean_inv_std) - float(z[f'{name}_mean_inv_std'])) <= 1e-6 * mean


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 260 * 1024


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get('EPROPNP_REFERENCE', '/root/reference'), 'EPro-PnP-Det')),
                    reason='the reference checkout is only present in the build container')
def test_fixture_is_what_the_reference_returns_today():
    spec = importlib.util.spec_from_file_location('make_roi_golden', os.path.join(ROOT, 'tools', 'make_roi_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    live, z = tool.make(), np.load(GOLDEN)
    assert sorted(live) == sorted(z.files)
    for k in z.files:
        if k.split('_', 1)[1] in RESULTS:
            scale = max(1.0, float(np.abs(z[k]).max()))
            assert np.abs(live[k].astype(np.float64) - z[k]).max() <= 1e-6 * scale, k      # (another torch build may order its fp32 sums differently)
        else:
            assert np.array_equal(live[k], z[k]), k
