"""epropnp.targets.VolumeCenter as a drop-in for the reference's class (core/bbox_3d/center_target.py): the constructor, the 6-tuple of
get_centers_2d with its types, shapes and splits, the warning, the empty return, what is not provided, and the registry."""
import warnings

import numpy as np
import pytest
import torch

import test_center_target as tc


def _inputs(backend, n_keep=None):
    boxes, inds, cams = tc.scene_main()
    if n_keep is not None:
        boxes, inds = boxes[n_keep], inds[n_keep]
    x2d, mask = tc.x2d_maps('identity', 3, 24, 40, 4)
    b2 = np.tile(np.array([10.0, 12.0, 50.0, 40.0], dtype=np.float32), (len(boxes), 1))
    return [tc.dev(a, backend) for a in (b2, boxes, inds, x2d, mask, cams)] + [torch.tensor([96.0, 160.0])]


def test_six_tuple(backend, poisoned_empty):
    from epropnp.targets import VolumeCenter, volume_centers
    vc = VolumeCenter(faces_per_pixel=16, output_stride=4, render_stride=4, get_bbox_2d=True, min_box_size=9.0, max_gpu_obj=50)
    args = _inputs(backend)
    with pytest.warns(UserWarning, match='Some annotated objects are disgarded'):
        centers, boxes, centers_list, boxes_list, valid, counts = vc.get_centers_2d(*args)
    dense = volume_centers(args[1], args[2], args[5], args[3], args[4], (96, 160), get_bbox_2d=True, min_box_size=9.0)
    assert valid.dtype == torch.bool and valid.shape == (9,) and torch.equal(valid, dense[2])
    keep = valid.cpu().numpy()
    assert keep.tolist() == [True, True, True, True, False, False, False, False, True]      # (object 7 is one cell: under 9 px)
    assert torch.equal(centers, dense[0][valid]) and torch.equal(boxes, dense[1][valid])
    assert centers.shape == (5, 2) and boxes.shape == (5, 4) and centers.dtype == torch.float32
    assert counts == [4, 0, 1] and all(type(c) is int for c in counts)
    assert len(centers_list) == 3 and len(boxes_list) == 3
    assert [tuple(c.shape) for c in centers_list] == [(4, 2), (0, 2), (1, 2)] and [tuple(b.shape) for b in boxes_list] == [(4, 4), (0, 4), (1, 4)]
    assert torch.equal(torch.cat(list(centers_list)), centers) and torch.equal(torch.cat(list(boxes_list)), boxes)


def test_no_warning_when_every_object_survives(backend):
    from epropnp.targets import VolumeCenter
    vc = VolumeCenter()
    args = _inputs(backend, n_keep=[0, 1, 2, 8])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        centers, boxes, _, _, valid, counts = vc.get_centers_2d(*args)
    assert bool(valid.all()) and counts == [3, 0, 1] and torch.equal(boxes, args[0])      # get_bbox_2d=False: the input boxes pass through


def test_empty_input(backend):
    from epropnp.targets import VolumeCenter
    args = _inputs(backend, n_keep=[])
    centers, boxes, centers_list, boxes_list, valid, counts = VolumeCenter().get_centers_2d(*args)
    assert centers.shape == (0, 2) and boxes.shape == (0, 4) and valid.shape == (0,) and valid.dtype == torch.bool
    assert counts == [0, 0, 0] and len(centers_list) == 3 and len(boxes_list) == 3
    assert all(c.shape == (0, 2) for c in centers_list) and all(b.shape == (0, 4) for b in boxes_list)


def test_what_is_not_provided_says_why():
    from epropnp.targets import VolumeCenter
    with pytest.raises(NotImplementedError, match='icosphere'):
        VolumeCenter(base_mesh=dict(type='ellipsoid'))
    with pytest.raises(NotImplementedError, match='reshape_'):
        VolumeCenter(occlusion_factor=0.1)
    assert VolumeCenter(occlusion_factor=0.0, base_mesh=dict(type='box')).max_gpu_obj == -1


def test_registry():
    from epropnp.builder import CENTER_TARGETS, build_center_target
    from epropnp.targets import VolumeCenter
    vc = build_center_target(dict(type='VolumeCenter', output_stride=4, render_stride=4, min_box_size=4.0))
    assert type(vc) is VolumeCenter and CENTER_TARGETS['VolumeCenter'] is VolumeCenter
    assert (vc.output_stride, vc.render_stride, vc.min_box_size, vc.faces_per_pixel, vc.rend_bbox_2d) == (4, 4, 4.0, 16, False)
