"""The drop-ins of epropnp.boxes under the reference's names against what the REFERENCE computes, and the conventions they have to get
right.  No reference file is read here: tests/golden/box3d_overlaps.npz holds boxes and the results of the reference's numba-free
functions (bev_to_box3d_overlaps, bev_to_box3d_overlaps_aligned, bev_to_box3d_overlaps_aligned_torch, d3_box_overlap_kernel,
image_box_overlap, get_split_parts), run in fp64 by tools/make_box_overlaps_golden.py out of the reference checkout with the fp64
clip of tests/test_boxes.py in place of the numba-CUDA step.  The pairwise ROTATED functions are numba-CUDA from end to end, so the
fixture cannot cover them: their criterion 0 / 1 order (the kernels call devRotateIoUEval(query_box, box): rotate_iou_kernel.py:288-290,
kitti_utils/rotate_iou.py:333-335) is checked against the hand-transposed fp64 oracle of tests/test_box_overlaps.py.

Bars: those of tests/test_box_overlaps.py (ratios |r - r64|, raw intersections |v - v64| / max(size_a, size_b)); the recorded reference
values are fp64 results on the same fp32 boxes, so they are that file's oracle under the reference's conventions.  The reference's
ratios have no floor (pairwise) or a 1e-6 floor (aligned) where ours have 1e-8: no box of the fixture has zero size."""
import os

import numpy as np
import pytest
import torch

import test_box_overlaps as tbo
from test_box_overlaps import INTER_BAR, RATIO_BAR, dev, oracle, value64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'box3d_overlaps.npz')
_rec = {}


def rec():
    if not _rec:
        with np.load(GOLDEN) as z:
            _rec.update({k: z[k] for k in z.files})
    return _rec


def _mod():
    from epropnp import boxes
    return boxes


def close(got, want, criterion, scale, tag):
    """ratios within RATIO_BAR; a raw intersection (a criterion other than -1 / 0 / 1) within INTER_BAR of max(size_a, size_b)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = np.abs(got - want)
    bar = RATIO_BAR
    if criterion not in (-1, 0, 1):
        err, bar = err / scale, INTER_BAR
    print(f'{tag} criterion {criterion}: worst error {err.max(initial=0.0):.3e} (bar {bar:.2e})')
    assert np.isfinite(got).all() and err.max(initial=0.0) <= bar, (tag, criterion)


def vol_scale(a, b, aligned=False):
    va, vb = a[:, 3:6].astype(np.float64).prod(1), b[:, 3:6].astype(np.float64).prod(1)
    return np.maximum(va, vb) if aligned else np.maximum(va[:, None], vb[None, :])


@pytest.mark.parametrize('criterion', [-1, 0, 1, 2])
def test_pairwise_3d_and_image_drop_ins_against_the_fixture(backend, poisoned_empty, criterion):
    m, r = _mod(), rec()
    pa, pb = r['pair_a'], r['pair_b']
    got = m.bbox3d_overlaps(pa, pb, criterion, device=backend)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    close(got, r[f'bbox3d_overlaps_{criterion}'], criterion, vol_scale(pa, pb), 'bbox3d_overlaps')
    got64 = m.bbox3d_overlaps(pa.astype(np.float64), pb.astype(np.float64), criterion, z_axis=1, z_center=0.5, device=backend)
    assert got64.dtype == np.float64 and np.array_equal(got64, got.astype(np.float64))
    # KITTI's height: y is the bottom face; a criterion other than -1 / 0 / 1 gives 1 where the volume is positive
    got = m.d3_box_overlap(pa, pb, criterion, device=backend)
    want = r[f'd3_box_overlap_{criterion}']
    if criterion == 2:
        vol = value64(oracle('box3d', pa, pb, z_axis=1, z_center=1.0), 'inter') / vol_scale(pa, pb)
        assert set(np.unique(got)) <= {0.0, 1.0} and set(np.unique(want)) <= {0.0, 1.0} and (want == 1).mean() > 0.2
        # (positive: above 1e-5 of the larger volume, the cap of the intersection's bar -- the drop-in's rule; between 0 and 2e-5
        # the fp32 result may fall on either side)
        assert np.array_equal(got[vol > 2e-5], want[vol > 2e-5]) and np.array_equal(got[vol == 0], want[vol == 0])
        assert (vol == 0).mean() > 0.1 and (got[vol == 0] == 0).all()
    else:
        close(got, want, criterion, None, 'd3_box_overlap')
    assert np.abs(r['d3_box_overlap_-1'] - r['bbox3d_overlaps_-1']).max() > 0.01          # the two height conventions do differ
    ia, ib = r['image_a'], r['image_b']
    got = m.image_box_overlap(ia, ib, criterion, device=backend)
    assert got.dtype == np.float32
    area_a, area_b = (ia[:, 2] - ia[:, 0]) * (ia[:, 3] - ia[:, 1]), (ib[:, 2] - ib[:, 0]) * (ib[:, 3] - ib[:, 1])
    close(got, r[f'image_box_overlap_{criterion}'], criterion, np.maximum(area_a[:, None], area_b[None, :]).astype(np.float64), 'image_box_overlap')


@pytest.mark.parametrize('criterion', [-1, 0, 1])
def test_aligned_3d_drop_ins_against_the_fixture(backend, poisoned_empty, criterion):
    """`bbox3d_overlaps_aligned` (numpy) takes the common height interval, `bbox3d_overlaps_aligned_torch` the reference's torch.min"""
    m, r = _mod(), rec()
    qa, qb = r['aligned_a'], r['aligned_b']
    got = m.bbox3d_overlaps_aligned(qa, qb, criterion, device=backend)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (120,)
    close(got, r[f'bbox3d_overlaps_aligned_{criterion}'], criterion, None, 'bbox3d_overlaps_aligned')
    got = m.bbox3d_overlaps_aligned_torch(dev(qa, backend), dev(qb, backend), criterion)
    assert torch.is_tensor(got) and got.dtype == torch.float32 and got.device.type == backend.type and got.shape == (120,)
    close(got.cpu().numpy(), r[f'bbox3d_overlaps_aligned_torch_{criterion}'], criterion, None, 'bbox3d_overlaps_aligned_torch')
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def test_the_torch_min_finding_is_in_the_fixture():
    """bbox3d_iou_calculator.py:151 takes torch.min of the two bottoms where :90 takes np.maximum: the recorded results of the two
    reference functions differ, and the `_torch` one is never the smaller"""
    r = rec()
    a, t = r['bbox3d_overlaps_aligned_-1'], r['bbox3d_overlaps_aligned_torch_-1']
    assert (np.abs(t - a) > 0.01).sum() >= 1 and (t >= a).all()
    print(f'the recorded IoUs differ by up to {np.abs(t - a).max():.3f}, by more than 0.01 on {(np.abs(t - a) > 0.01).sum()} of {a.size} pairs')


def test_aligned_criterion_outside_the_three_is_the_clamped_volume(backend, poisoned_empty):
    """(the reference's aligned functions raise there -- `ua = 1.0` has no clip; what they would return is clip(volume, 0, 1))"""
    m, r = _mod(), rec()
    qa, qb = r['aligned_a'], r['aligned_b']
    vol = value64(oracle('box3d', qa, qb, aligned=True), 'inter')
    assert (vol > 1).any() and (vol < 1).any()
    got = m.bbox3d_overlaps_aligned(qa, qb, 2, device=backend)
    assert got.max() == 1.0 and np.abs(got - np.clip(vol, 0, 1)).max() <= INTER_BAR * vol_scale(qa, qb, True).max()
    got_t = m.bbox3d_overlaps_aligned_torch(dev(qa, backend), dev(qb, backend), 2)
    assert float(got_t.max()) == 1.0


@pytest.mark.parametrize('criterion', [-1, 0, 1, 2])
def test_pairwise_rotated_functions_swap_criterion_0_and_1(backend, poisoned_empty, criterion):
    """criterion 0 of bbox_rotate_overlaps / rotate_iou_gpu_eval / bev_box_overlap divides by the QUERY box's area, 1 by `boxes`';
    the aligned functions divide by `boxes`' for 0"""
    m, r = _mod(), rec()
    a, b = tbo.as_kind(r['pair_a'], 'bev'), tbo.as_kind(r['pair_b'], 'bev')
    orc = oracle('bev', a, b)
    scale = np.maximum(orc[1], orc[2])
    want = value64(orc, {-1: 'iou', 0: 'b', 1: 'a', 2: 'inter'}[criterion])
    unswapped = value64(orc, {-1: 'iou', 0: 'a', 1: 'b', 2: 'inter'}[criterion])
    assert criterion in (-1, 2) or np.abs(want - unswapped).max() > 0.05
    for fn in (m.bbox_rotate_overlaps, m.rotate_iou_gpu_eval, m.bev_box_overlap):
        got = fn(a, b, criterion, device=backend)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        close(got, want, criterion, scale, fn.__name__)
    assert m.bbox_rotate_overlaps(a.astype(np.float64), b.astype(np.float64), criterion, device=backend).dtype == np.float64
    qa, qb = tbo.as_kind(r['aligned_a'], 'bev'), tbo.as_kind(r['aligned_b'], 'bev')
    orc = oracle('bev', qa, qb, aligned=True)
    scale = np.maximum(orc[1], orc[2])
    got = m.bbox_rotate_overlaps_aligned(qa, qb, criterion, device=backend)
    assert got.dtype == np.float32 and got.shape == (120,)
    close(got, value64(orc, {-1: 'iou', 0: 'a', 1: 'b', 2: 'inter'}[criterion]), criterion, scale, 'bbox_rotate_overlaps_aligned')
    got_t = m.bbox_rotate_overlaps_aligned_torch(dev(qa, backend), dev(qb, backend), criterion)
    assert torch.is_tensor(got_t) and np.array_equal(got_t.cpu().numpy(), got)


def test_empty_inputs_have_the_references_shapes(backend):
    m = _mod()
    e5, e7, e4 = np.zeros((0, 5), np.float32), np.zeros((0, 7), np.float64), np.zeros((0, 4), np.float32)
    f5, f7, f4 = np.ones((3, 5), np.float32), np.ones((3, 7), np.float64), np.ones((3, 4), np.float32)
    assert m.bbox_rotate_overlaps(e5, f5, device=backend).shape == (0, 3) and m.rotate_iou_gpu_eval(f5, e5, device=backend).shape == (3, 0)
    assert m.bbox3d_overlaps(e7, f7, device=backend).shape == (0, 3) and m.bbox3d_overlaps(e7, f7, device=backend).dtype == np.float64
    assert m.d3_box_overlap(f7, e7, device=backend).shape == (3, 0) and m.image_box_overlap(e4, f4, device=backend).shape == (0, 3)
    assert m.bbox_rotate_overlaps_aligned(e5, e5, device=backend).shape == (0,) and m.bbox3d_overlaps_aligned(e7, e7, device=backend).shape == (0,)
    t = m.bbox3d_overlaps_aligned_torch(torch.zeros(0, 7, device=backend), torch.zeros(0, 7, device=backend))
    assert t.shape == (0,) and t.dtype == torch.float32


# ---- calculate_iou_partly ------------------------------------------------------------------------------------------------------------
GT_COUNTS, DT_COUNTS = [3, 0, 5, 2, 0, 4, 1], [4, 2, 0, 6, 0, 3, 1]


def annos(counts, boxes7):
    """KITTI annotations (camera frame: location [x, y, z] with y the bottom face, dimensions [l, h, w]) of consecutive scene boxes"""
    out, at = [], 0
    for n in counts:
        b = boxes7[at:at + n].astype(np.float64)
        img = tbo.as_kind(boxes7[at:at + n], 'image').astype(np.float64) * 8.0 + 300.0
        out.append(dict(name=np.array(['Car'] * n), bbox=img.reshape(n, 4), location=b[:, :3], dimensions=b[:, 3:6], rotation_y=b[:, 6]))
        at += n
    return out


@pytest.mark.parametrize('metric', [0, 1, 2])
def test_calculate_iou_partly(backend, poisoned_empty, metric):
    """7 images, among them one without gts, one without dts and one without either; num_parts = 3, so that a remainder part exists.
    The per-image blocks against the fp64 oracle under KITTI's conventions, the parted shapes, the counts, and ONE segmented launch"""
    from epropnp import _hip
    m, r = _mod(), rec()
    s = tbo.scene7(sum(GT_COUNTS) + sum(DT_COUNTS), 3)
    gts, dts = annos(GT_COUNTS, s[:sum(GT_COUNTS)]), annos(DT_COUNTS, s[sum(GT_COUNTS):])
    _hip.profile(True, reset=True)
    try:
        overlaps, parted, total_gt, total_dt = m.calculate_iou_partly(gts, dts, metric, num_parts=3, device=backend)
        assert _hip.profile_read('box_overlap_segmented')[1] == 1 and _hip.profile_read('box_overlap')[1] == 0
    finally:
        _hip.profile(False, reset=True)
    assert total_gt.tolist() == GT_COUNTS and total_dt.tolist() == DT_COUNTS and isinstance(total_gt, np.ndarray)
    assert len(overlaps) == 7
    some = 0
    for i, (g, d, ov) in enumerate(zip(gts, dts, overlaps)):
        assert ov.shape == (GT_COUNTS[i], DT_COUNTS[i]) and ov.dtype == np.float64
        if metric == 0:
            ga, da = g['bbox'].astype(np.float32), d['bbox'].astype(np.float32)
            want = value64(oracle('image', ga, da), 'iou')
        elif metric == 1:
            ga, da = (np.concatenate((x['location'][:, [0, 2]], x['dimensions'][:, [0, 2]], x['rotation_y'][:, None]), 1).astype(np.float32) for x in (g, d))
            want = value64(oracle('bev', ga, da), 'iou')
        else:
            ga, da = (np.concatenate((x['location'], x['dimensions'], x['rotation_y'][:, None]), 1).astype(np.float32) for x in (g, d))
            want = value64(oracle('box3d', ga, da, z_axis=1, z_center=1.0), 'iou')
        close(ov, want, -1, None, f'metric {metric} image {i}')
        some += int((want > 0.05).sum())
    assert some >= 5, 'the annotations do not overlap'
    parts = r['split_parts_7_3'].tolist()
    assert parts == [2, 2, 2, 1] and len(parted) == len(parts)
    at = 0
    for n, part in zip(parts, parted):
        assert part.shape == (sum(GT_COUNTS[at:at + n]), sum(DT_COUNTS[at:at + n])) and part.dtype == np.float64
        row = col = 0
        for i in range(at, at + n):
            assert np.array_equal(part[row:row + GT_COUNTS[i], col:col + DT_COUNTS[i]], overlaps[i])
            row, col = row + GT_COUNTS[i], col + DT_COUNTS[i]
        at += n
    # no remainder part when the images divide evenly
    assert r['split_parts_6_3'].tolist() == [2, 2, 2]
    assert len(m.calculate_iou_partly(gts[:6], dts[:6], metric, num_parts=3, device=backend)[1]) == 3
    with pytest.raises(ValueError, match='unknown metric'):
        m.calculate_iou_partly(gts, dts, 3, num_parts=3, device=backend)


# ---- the head's slice ----------------------------------------------------------------------------------------------------------------
def test_the_heads_iou_score_targets(backend, poisoned_empty):
    """deform_pnp_head.py:894-899 with score_type = 'iou', restated: the solved poses and the decoded dimensions against the targets"""
    m, r = _mod(), rec()
    pose_opt, dim_decoded, bbox_3d_targets, sample_weights = (dev(r[k], backend) for k in (
        'head_pose_opt', 'head_dim_decoded', 'head_bbox_3d_targets', 'head_sample_weights'))
    num_obj_actual = float(r['head_num_obj_actual'])
    ious = m.bbox3d_overlaps_aligned_torch(
        torch.cat((pose_opt[:, :3], dim_decoded, pose_opt[:, 3:]), dim=-1),
        bbox_3d_targets[:, [3, 4, 5, 0, 1, 2, 6]]).reshape(-1)
    metric = {'mean_iou': (ious * sample_weights).sum() / num_obj_actual}
    score_targets = (2 * ious - 0.5).clamp(min=0, max=1)
    close(ious.cpu().numpy(), r['head_ious'], -1, None, 'ious')
    assert abs(float(metric['mean_iou']) - float(r['head_mean_iou'])) <= RATIO_BAR + 1e-6      # (+ the fp32 sum of 120 terms)
    assert np.abs(score_targets.cpu().numpy() - r['head_score_targets']).max() <= 2 * RATIO_BAR
    assert 0.2 < float(r['head_mean_iou']) < 0.9 and (r['head_score_targets'] == 0).any() and (r['head_score_targets'] > 0.5).any()
