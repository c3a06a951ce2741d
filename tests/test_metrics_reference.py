"""epropnp.metrics.pose_errors against what the reference's own evaluation returns (EPro-PnP-6DoF lib/utils/eval.py: calc_all_errs,
add, adi -- scipy logm and cKDTree in fp64) on the fp32 poses of tests/golden/metrics_eval.npz (tools/make_metrics_golden.py).

Two parts.  On the CPU, where the reference checkout and scipy are present, the tool's exec of the reference functions is re-run and
the committed fixture must still be what they return, to 1e-12.  On the emulation and on the GPU -- no reference, no scipy --
pose_errors on the fixture's inputs must meet the fixture's numbers at the bars of test_metrics.py, with one extra term for
add / adi: 2e-7 x model radius, the residue of normalising an fp32 quaternion (evaluated in fp64 through the relative-frame form the
kernel uses, the reference itself stays within 1.6e-7 of the radius of its own cKDTree result on such inputs)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_metrics as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'metrics_eval.npz')
QUAT_RESIDUE = 2e-7      # x model radius


def _tool():
    spec = importlib.util.spec_from_file_location('make_metrics_golden', os.path.join(ROOT, 'tools', 'make_metrics_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _have_scipy():
    return importlib.util.find_spec('scipy') is not None


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, 'EPro-PnP-6DoF', 'lib', 'utils', 'eval.py')) or not _have_scipy(),
                    reason='needs the reference checkout and scipy (build container only)')
def test_fixture_is_what_the_reference_returns_today():
    data = _tool().compute(REF)
    old = np.load(FIXTURE)
    assert sorted(old.files) == sorted(data)
    for k, v in data.items():
        assert old[k].dtype == v.dtype and old[k].shape == v.shape, k
        if k.startswith('errs'):
            np.testing.assert_allclose(old[k], v, rtol=1e-12, atol=1e-12, err_msg=k)
        else:
            assert np.array_equal(old[k], v), k


def test_fixture_holds_the_cases_it_promises():
    z = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 200 * 1024
    assert z['range'].tolist() == [[0, 1], [1, 257], [258, 1500]]
    n = np.bincount(z['model_id6'], minlength=3) + np.bincount(z['model_id4'], minlength=3)
    assert n.tolist() == [40, 40, 40]
    assert z['est6'].dtype == np.float32 and z['errs6'].dtype == np.float64 and z['errs6'].shape == (96, 5)
    assert 45.0 < float(np.median(z['gt4'][:, 2])) < 55.0 and 0.7 < float(np.median(z['gt6'][:, 2])) < 1.3


@pytest.mark.parametrize('dof', [4, 6])
def test_pose_errors_meet_the_reference(backend, poisoned_empty, dof):
    from epropnp import metrics
    z = np.load(FIXTURE)
    tag = str(dof)
    pts, rng = torch.from_numpy(z['points']), torch.from_numpy(z['range'])
    est, gt = torch.from_numpy(z['est' + tag]), torch.from_numpy(z['gt' + tag])
    mid = torch.from_numpy(z['model_id' + tag])
    sym, half = torch.from_numpy(z['symmetric' + tag]).bool(), torch.from_numpy(z['half_turn' + tag]).bool()
    errs = torch.from_numpy(z['errs' + tag])
    e = metrics.pose_errors(est.to(backend), gt.to(backend), pts.to(backend), rng.to(backend), model_id=mid.to(backend),
                            cam_mats=torch.from_numpy(z['cam_mats' + tag]).to(backend), symmetric=sym.to(backend), half_turn=half.to(backend))
    want = torch.full((1, est.shape[0], 6), float('nan'), dtype=torch.float64)
    want[0, :, :4] = errs[:, :4]
    want[0, sym, 4] = errs[sym, 4]
    want[0, :, 5] = torch.where(sym, errs[:, 4], errs[:, 3])
    radius = torch.stack([pts[f:f + c].norm(dim=-1).max() for f, c in rng.tolist()])[mid.long()]
    tm.check(e.raw, want, radius, est, gt, f'reference fixture dof={dof}', extra_adi=QUAT_RESIDUE * radius)
    if dof == 6:
        assert int(half.sum()) >= 24
