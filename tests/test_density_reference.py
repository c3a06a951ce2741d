"""epropnp.visualize.draw_orient_density against the REFERENCE's function of that name (EPro-PnP-6DoF
lib/utils/draw_orient_density.py), through tests/golden/density_orient.npz: inputs and the image the reference returned for them,
written by tools/make_density_golden.py with a stub `cv2` whose `line` does nothing -- the picture without the axis lines, which is
what the package is asked for here (pose_opt=None).  The generator fences the inputs from fp64 (no axis point within 1e-4 px of a
pixel boundary, none with |a_z| < 1e-5), so both sides take the same binning decisions; what is left is fp32 rounding on both
sides, compared at test_density.IMG_BAR (whose measured worst case counts the figures printed here too).

For the BEV half no reference run is possible -- `show_bev` needs cv2, which is not installed: the fp64 oracle of
tests/test_density.py is its yardstick.

The last test re-runs the live reference where its checkout exists (build container only) and checks that the fixture is still
what it returns."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_density as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'density_orient.npz')
KWARGS = {'a': {}, 'b': dict(sample_kernel=(3, 3), saturation=0.7, sphere_opacity=0.4, intensity_scale=20)}
SHAPES = {'a': (32, 2, 64), 'b': (96, 3, 64)}


@pytest.mark.parametrize('case', ['a', 'b'])
def test_drop_in_against_the_recorded_reference_image(backend, case):
    from epropnp import visualize
    z = np.load(GOLDEN)
    S, B, size = SHAPES[case]
    pose_samples, logw = torch.from_numpy(z[f'{case}_pose_samples']), torch.from_numpy(z[f'{case}_logweights'])
    assert pose_samples.shape == (S, B, 7) and z[f'{case}_image'].shape == (B, size, size, 3)
    got = visualize.draw_orient_density(None, pose_samples.to(backend), logw.to(backend), size=size, **KWARGS[case])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (B, size, size, 3)
    err = float(np.abs(got.astype(np.float64) - z[f'{case}_image'].astype(np.float64)).max())
    print(f'case {case}: worst difference from the reference image {err:.3e}')
    assert err <= td.IMG_BAR, f'{err:.3e} > {td.IMG_BAR:.3e}'
    # with pose_opt the picture differs on the lines only: they cover a small part of it
    lined = visualize.draw_orient_density(torch.from_numpy(z[f'{case}_pose_opt']).to(backend), pose_samples.to(backend), logw.to(backend),
                                          size=size, **KWARGS[case])
    changed = (lined != got).any(-1).mean()
    assert 0.0 < changed < 0.12, changed


def test_bev_density_layer_is_the_reference_line():
    from epropnp import visualize
    d = torch.tensor([[0.0, 0.5], [2.0, 1.0]])
    layer = visualize.bev_density_layer(d)
    want = np.array((0.9, 0.5, 0.1), dtype=np.float32) ** d.numpy()[..., None]
    assert layer.shape == (2, 2, 3) and np.allclose(layer.numpy(), want, rtol=1e-6, atol=0)
    assert (layer[0, 0] == 1).all()


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get('EPROPNP_REFERENCE', '/root/reference'), 'EPro-PnP-6DoF')),
                    reason='the reference checkout is only present in the build container')
def test_fixture_is_what_the_reference_returns_today():
    spec = importlib.util.spec_from_file_location('make_density_golden', os.path.join(ROOT, 'tools', 'make_density_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    live, z = tool.make(), np.load(GOLDEN)
    assert sorted(live) == sorted(z.files)
    for k in z.files:
        if k.endswith('_image'):
            assert np.abs(live[k].astype(np.float64) - z[k]).max() <= 1e-6, k      # (another torch build may order its fp32 sums differently)
        else:
            assert np.array_equal(live[k], z[k]), k
