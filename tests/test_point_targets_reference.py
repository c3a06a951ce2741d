"""epropnp.targets.get_targets / fcos_points against tests/golden/point_targets.npz: what the reference's own
FCOSEmbHead._get_points_single, get_targets and _get_target_single return for the scenes of tests/test_point_targets.py, cut out of
the checkout at recording time by tools/make_point_target_golden.py and run on the CPU.

The three per-level lists: labels and gt_inds exact, centerness within test_point_targets.CENTERNESS_BAR (there against fp64, here
against the reference's fp32: one more rounding of at most half an ulp of a value in [0, 1], 3e-8, which the bar's factor 4 holds).
This pins the level-major, image, point order and the per-image index base, the `base + 0` of background rows and of empty images
after the first included."""
import os

import numpy as np
import pytest
import torch

import test_point_targets as tp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_targets.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fcos_points_are_the_reference_grid(golden):
    from epropnp import targets
    pts = targets.fcos_points([tuple(s) for s in golden['featmap_sizes'].tolist()], golden['strides'].tolist(), torch.float32, 'cpu')
    assert len(pts) == len(tp.STRIDES)
    for k, p in enumerate(pts):
        assert p.dtype == torch.float32 and np.array_equal(p.numpy(), golden[f'points_lvl{k}'])
        assert np.array_equal(p.numpy(), tp.level_points()[k])


@pytest.mark.parametrize('name', sorted(tp.SCENES))
def test_get_targets_returns_the_reference_lists(backend, golden, name):
    from epropnp import targets
    num_img, img = int(golden[f'{name}_num_img']), golden[f'{name}_obj_img_inds']
    per_img = lambda a: [tp.dev(a[img == i], backend) for i in range(num_img)]      # noqa: E731
    points = targets.fcos_points([tuple(s) for s in golden['featmap_sizes'].tolist()], golden['strides'].tolist(), torch.float32, backend)
    ranges = [tuple(r) for r in golden['regress_ranges'].tolist()]
    num_classes, radius, alpha = int(golden['params'][0]), float(golden['params'][1]), float(golden['params'][2])
    labels, centerness, gt_inds = targets.get_targets(points, per_img(golden[f'{name}_gt_bboxes']), per_img(golden[f'{name}_gt_labels']),
                                                      per_img(golden[f'{name}_centers2d']), strides=golden['strides'].tolist(),
                                                      regress_ranges=ranges, num_classes=num_classes, center_sample_radius=radius,
                                                      centerness_alpha=alpha)
    assert len(labels) == len(centerness) == len(gt_inds) == len(points)
    worst, fg = 0.0, 0
    for k in range(len(points)):
        want_l, want_c, want_g = (golden[f'{name}_{what}_lvl{k}'] for what in ('labels', 'centerness', 'gt_inds'))
        assert labels[k].dtype == torch.int64 and gt_inds[k].dtype == torch.int64 and centerness[k].dtype == torch.float32
        assert np.array_equal(labels[k].cpu().numpy(), want_l), k
        assert np.array_equal(gt_inds[k].cpu().numpy(), want_g), k
        worst = max(worst, float(np.abs(centerness[k].cpu().numpy().astype(np.float64) - want_c).max()))
        fg += int((want_l < num_classes).sum())
    print(f'get_targets[{name}] on {backend}: worst centerness difference from the reference {worst:.3e}')
    assert worst <= tp.CENTERNESS_BAR and fg > 0
    if name == 'main':
        # the base of the empty middle image and of the background rows of the last one: 5 objects precede them
        n0 = len(golden['points_lvl0'])
        g0, l0 = golden['main_gt_inds_lvl0'], golden['main_labels_lvl0']
        assert (g0[n0:2 * n0] == 5).all() and (g0[2 * n0:][l0[2 * n0:] == num_classes] == 5).all()
