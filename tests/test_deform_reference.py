"""epropnp.deform.sample_attend against the REFERENCE's DeformableAttentionSampler (EPro-PnP-Det
epropnp_det/ops/deformable_attention_sampler.py), through tests/golden/deform_sampler.npz: inputs, the sampling locations the module
formed, `attn` (captured in front of its out_proj) and its four sample tensors, written by tools/make_deform_golden.py with stub mmcv
modules.  The generator fences the locations (no map coordinate within 1e-3 px of an integer), so both sides sample the same pixels;
what is left is fp32 rounding on the reference's side and one rounding per output on the package's, compared at test_deform.FWD_BAR
(whose measured worst case counts the figures printed here too).

The last test re-runs the live reference where its checkout exists (build container only) and checks that the fixture is still what
it returns."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_deform as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'deform_sampler.npz')
SHAPES = {'a': (7, 3, 2, 5, 4, 6, 9), 'b': (4, 1, 8, 16, 32, 4, 6)}


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('case', ['a', 'b'])
def test_against_the_recorded_reference(backend, case, layout):
    from epropnp import deform
    z = np.load(GOLDEN)
    B, NI, H, P, D, h, w = SHAPES[case]
    t = {k: torch.from_numpy(z[f'{case}_{k}']) for k in ('query', 'key', 'value', 'dense_x2d', 'dense_mask', 'sampling_location', 'obj_img_ind')}
    assert t['key'].shape == (NI, H * D, h, w) and t['sampling_location'].shape == (B, H, P, 2)
    got = deform.sample_attend(t['query'].to(backend), td._layout(t['key'], layout, backend), td._layout(t['value'], layout, backend),
                               t['dense_x2d'].to(backend), t['dense_mask'].to(backend), t['sampling_location'].to(backend),
                               t['obj_img_ind'].to(backend), int(z[f'{case}_stride']))
    for n, g in zip(td.NAMES, got):
        want = torch.from_numpy(z[f'{case}_{n}'])
        assert g.shape == want.shape, (n, tuple(g.shape), tuple(want.shape))
        err = float((g.double().cpu() - want.double()).abs().max())
        print(f'case {case} {layout}: {n} worst difference from the reference {err:.3e}')
        assert err <= td.FWD_BAR[n], f'{n}: {err:.3e} > {td.FWD_BAR[n]:.3e}'


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get('EPROPNP_REFERENCE', '/root/reference'), 'EPro-PnP-Det')),
                    reason='the reference checkout is only present in the build container')
def test_fixture_is_what_the_reference_returns_today():
    spec = importlib.util.spec_from_file_location('make_deform_golden', os.path.join(ROOT, 'tools', 'make_deform_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    live, z = tool.make(), np.load(GOLDEN)
    assert sorted(live) == sorted(z.files)
    for k in z.files:
        if k.split('_', 1)[1] in td.NAMES:
            scale = max(1.0, float(np.abs(z[k]).max()))
            assert np.abs(live[k].astype(np.float64) - z[k]).max() <= 1e-6 * scale, k      # (another torch build may order its fp32 sums differently)
        else:
            assert np.array_equal(live[k], z[k]), k
    assert os.path.getsize(GOLDEN) < 260 * 1024
