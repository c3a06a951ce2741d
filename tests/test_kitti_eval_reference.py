"""The pinning check of tests/golden/kitti_eval.npz: tools/make_kitti_eval_golden.py, run against the reference checkout, writes every
array of the committed fixture again, bit for bit.  Skipped where the reference checkout is absent."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
EVAL_PY = os.path.join(REF, 'EPro-PnP-Det', 'epropnp_det', 'core', 'evaluation', 'kitti_utils', 'eval.py')


@pytest.mark.skipif(not os.path.exists(EVAL_PY), reason='the reference checkout is not present')
def test_the_fixture_regenerates_bit_for_bit(tmp_path):
    spec = importlib.util.spec_from_file_location('make_kitti_eval_golden', os.path.join(ROOT, 'tools', 'make_kitti_eval_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rec, facts = tool.build(REF, tool.SEED)
    assert tool.conditions(rec, facts) == []
    out = str(tmp_path / 'kitti_eval.npz')
    np.savez_compressed(out, **rec)
    new, old = np.load(out), np.load(os.path.join(ROOT, 'tests', 'golden', 'kitti_eval.npz'))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k
