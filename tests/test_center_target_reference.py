"""epropnp.targets.volume_centers against what the REFERENCE's VolumeCenter.post_proc computes.  No reference file is read by the
comparison: tests/golden/center_target.npz holds scenes and the results of post_proc, run by tools/make_center_target_golden.py out of
the reference checkout on the fragments of the fp64 rasteriser of tests/test_center_target.py in place of the pytorch3d step (fp32
zbuf, the reference's own fp32 grid_sample and sums).  Centres within CENTER_BAR of tests/test_center_target.py on the objects the
reference keeps, boxes and valid mask exactly.  Where a reference checkout is at hand, the last test runs the tool again and holds
the fixture to what the reference still computes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_center_target import CENTER_BAR, dev

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'center_target.npz')
NUM_CASES = 4
_rec = {}


def rec():
    if not _rec:
        with np.load(GOLDEN) as z:
            _rec.update({k: z[k] for k in z.files})
    return _rec


@pytest.mark.parametrize('get_bbox', [False, True])
@pytest.mark.parametrize('case', range(NUM_CASES))
def test_volume_centers_against_the_fixture(backend, poisoned_empty, case, get_bbox):
    from epropnp import targets
    r, t = rec(), f'c{case}_'
    mh, mw, os_, rs, fpp, min_box = r[t + 'params']
    c, b, v = targets.volume_centers(dev(r[t + 'bboxes_3d'], backend), dev(r[t + 'obj_img_inds'], backend), dev(r[t + 'cam_intrinsic'], backend),
                                     dev(r[t + 'x2d'], backend), dev(r[t + 'mask'], backend), (int(mh), int(mw)),
                                     bboxes_2d=dev(r[t + 'bboxes_2d'], backend), output_stride=int(os_), render_stride=int(rs),
                                     faces_per_pixel=int(fpp), min_box_size=float(min_box), get_bbox_2d=get_bbox)
    want_c, want_b, want_v = (r[f'{t}{k}_{int(get_bbox)}'] for k in ('centers', 'boxes', 'valid'))
    c, b, v = c.cpu().numpy(), b.cpu().numpy(), v.cpu().numpy()
    assert np.array_equal(v, want_v) and np.array_equal(b, want_b)
    assert want_v.sum() >= 2 and (get_bbox or not want_v.all())      # min_box_size rejects the 3 px input box
    worst = np.abs(c[want_v].astype(np.float64) - want_c[want_v]).max()
    print(f'centre worst {worst:.3e} px against the reference')
    assert worst <= CENTER_BAR
    assert (c[np.isnan(want_c).any(1)] == 0).all()             # the reference's 0 / 0: (0, 0) here


def test_fixture_is_what_the_reference_computes():
    ref = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
    if not os.path.isdir(os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'core', 'bbox_3d')):
        pytest.skip('no reference checkout here: the fixture is compared as recorded')
    spec = importlib.util.spec_from_file_location('make_center_target_golden', os.path.join(os.path.dirname(HERE), 'tools', 'make_center_target_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    again, r = tool.record(ref), rec()
    assert sorted(again) == sorted(r) and len(tool.CASES) == NUM_CASES
    for k in r:
        assert np.array_equal(again[k], r[k], equal_nan=again[k].dtype.kind == 'f'), k
