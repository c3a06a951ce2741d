"""Rotated bird's-eye-view boxes on the device: overlap area, IoU and the grouped greedy NMS the detection head ends with.

The reference turns poses and scores into detections through its one native extension, the CUDA `ops/iou3d`
(EPro-PnP-Det core/bbox_3d/misc.py:300-324 `batched_bev_nms` in `DeformPnPHead.get_bbox_3d_result`, nuscenes3d_dataset.py:395
`nms_gpu` for the cross-camera merge): the suppression mask goes to the host and is reduced there, and images / classes are kept
apart by shifting coordinates.  Here (include/epropnp_hip.h: epropnp_bev_overlap, epropnp_bev_nms) the mask is reduced on the
device and groups are compared as integers, so no coordinate is shifted.

A box is (cx, cy, dx, dy, angle): corners (cx + u cos a + v sin a, cy - u sin a + v cos a), u = +-dx/2, v = +-dy/2 -- the yaw
convention of `yaw_to_rot_mat` with (x, z) as the plane.  A box is valid iff its five numbers are finite and dx, dy >= 0.

`bev_overlap`, `bev_iou` and `bev_nms` run on the current HIP stream of the inputs' device, allocate with torch.empty, never
synchronise; `bev_nms(..., order=...)` can be captured into a hipGraph.  `batched_bev_nms` and `nms_gpu` are drop-ins for the
reference's functions of those names and read `num_keep` once (their output shape depends on it).  Nothing is differentiable.

`rotated_overlaps`, `box3d_overlaps` and `image_overlaps` (epropnp_box_overlap, epropnp_box_overlap_segmented) put the reference's
criteria, the height interval of 3D boxes and axis-aligned image boxes around the same overlap routine -- pairwise, aligned, or per
segment (`counts=`: many independent (gts, dts) blocks in one launch).  They stand in for the reference's two numba-CUDA files
(core/bbox_3d/iou_calculators/rotate_iou_kernel.py, core/evaluation/kitti_utils/rotate_iou.py), which have no ROCm path; the drop-ins
below them carry the reference's names: `bbox3d_overlaps_aligned_torch` for the head's score targets, `calculate_iou_partly` for the
KITTI evaluation, and the functions those are made of.  The ratios floor their denominator at 1e-8 (the reference's aligned functions
at 1e-6, its pairwise ones not at all): the results differ only for boxes of zero size.
"""
from collections import namedtuple

import torch

from . import _hip
from .functional import _f32c

TILE = 64             # include/epropnp_hip.h: EPROPNP_BEV_TILE

BevNms = namedtuple('BevNms', ['keep_index', 'keep_mask', 'num_keep'])
BevNms.__doc__ = """keep_index (N,) int32: the kept box indices in visiting order, then -1;  keep_mask (N,) bool by box index;
num_keep (1,) int32.  All on the device: reading num_keep is the caller's synchronisation."""


def _boxes(t, name):
    if not torch.is_tensor(t):
        raise ValueError(f'{name}: a (N,5) tensor is expected, got {type(t)}')
    t = _f32c(t, name)
    if t.dim() != 2 or t.shape[1] != 5:
        raise ValueError(f'{name}: (N,5) rows (cx, cy, dx, dy, angle) expected, got {tuple(t.shape)}')
    return t


def _ints(t, name, N, device):
    if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.shape != (N,):
        raise ValueError(f'{name}: a ({N},) int32 tensor is expected')
    _hip.check_device(t, name)
    if t.device != device:
        raise RuntimeError(f'{name} lives on {t.device}, the boxes on {device}')
    return t.detach().to(torch.int32).contiguous()


def _overlap(boxes_a, boxes_b, aligned, want_iou):
    a, b = _boxes(boxes_a, 'boxes_a'), _boxes(boxes_b, 'boxes_b')
    if a.device != b.device:
        raise RuntimeError(f'boxes_a lives on {a.device}, boxes_b on {b.device}')
    M, N = int(a.shape[0]), int(b.shape[0])
    if aligned and M != N:
        raise ValueError(f'aligned needs as many boxes_a as boxes_b, got {M} and {N}')
    out = torch.empty((N,) if aligned else (M, N), dtype=torch.float32, device=a.device)
    if M > 0 and N > 0:
        _hip.call('epropnp_bev_overlap', _hip.ptr(a), M, _hip.ptr(b), N, int(want_iou), int(bool(aligned)), _hip.ptr(out),
                  _hip.stream_of(a))
    return out


def bev_overlap(boxes_a, boxes_b, aligned=False):
    """Overlap area of boxes_a (M,5) and boxes_b (N,5) -> (M,N); aligned: of boxes_a[i] and boxes_b[i] -> (N,), the bits of the
    pairwise result's diagonal.  NaN exactly where either box is invalid."""
    return _overlap(boxes_a, boxes_b, aligned, 0)


def bev_iou(boxes_a, boxes_b, aligned=False):
    """overlap / max(area_a + area_b - overlap, 1e-8), shapes as `bev_overlap`: exactly 1 for identical boxes, exactly 0 for
    boxes that only touch."""
    return _overlap(boxes_a, boxes_b, aligned, 1)


def bev_nms(boxes, scores, iou_thr, groups=None, order=None):
    """Greedy NMS of boxes (N,5) -> BevNms.  Visiting order: `order` (N,) int32 if given (entries outside [0, N) are skipped;
    `scores` is then not looked at and may be None), else by descending `scores` (N,), equal scores lower index first; a box with a
    NaN score is treated as invalid.  A valid box that is not yet suppressed is kept and suppresses every later box of its group
    (`groups` (N,) int32, one group without) whose IoU with it is > iou_thr.  Invalid boxes are never kept and suppress nothing."""
    b = _boxes(boxes, 'boxes')
    N, dev = int(b.shape[0]), b.device
    if order is None:
        if not torch.is_tensor(scores) or scores.shape != (N,):
            raise ValueError(f'scores: a ({N},) fp32 tensor is expected')
        s = _f32c(scores, 'scores')
        if s.device != dev:
            raise RuntimeError(f'scores lives on {s.device}, the boxes on {dev}')
        idx = torch.sort(s, descending=True, stable=True).indices
        order = torch.where(s[idx].isnan(), torch.full_like(idx, -1), idx).to(torch.int32)
    else:
        order = _ints(order, 'order', N, dev)
    grp = None if groups is None else _ints(groups, 'groups', N, dev)
    tiles = (N + TILE - 1) // TILE
    scratch = torch.empty((N * tiles,), dtype=torch.int64, device=dev)
    keep_index = torch.empty((N,), dtype=torch.int32, device=dev)
    keep_mask = torch.empty((N,), dtype=torch.uint8, device=dev)
    num_keep = torch.empty((1,), dtype=torch.int32, device=dev)
    _hip.call('epropnp_bev_nms', _hip.ptr(b), _hip.ptr(order), _hip.ptr(grp), N, float(iou_thr), _hip.ptr(scratch),
              scratch.numel() * 8, _hip.ptr(keep_index), _hip.ptr(keep_mask), _hip.ptr(num_keep), _hip.stream_of(b))
    return BevNms(keep_index=keep_index, keep_mask=keep_mask.view(torch.bool), num_keep=num_keep)


def _kept(res):
    """the kept indices as int64 (n,): the one read of num_keep the dynamic shape needs"""
    return res.keep_index[:int(res.num_keep.item())].to(torch.int64)


def batched_bev_nms(bbox_3d, batch_inds, nms_thr=0.25):
    """Drop-in for the reference's `batched_bev_nms`: bbox_3d (N,8+) rows [l, h, w, x, y, z, ry, score, ...], batch_inds (N,)
    -> (bbox_3d[keep_inds], keep_inds int64 by descending score).  `batch_inds` is the group: no coordinate is shifted.  As in the
    reference, n <= 1 returns an empty keep_inds (a lone box is dropped; `bev_nms` keeps it)."""
    if not torch.is_tensor(bbox_3d) or bbox_3d.dim() != 2 or bbox_3d.shape[1] < 8:
        raise ValueError('bbox_3d: (N,8+) rows [l, h, w, x, y, z, ry, score, ...] expected')
    n = int(bbox_3d.shape[0])
    if n > 1:
        box = _f32c(bbox_3d, 'bbox_3d')
        if not torch.is_tensor(batch_inds) or batch_inds.shape != (n,):
            raise ValueError(f'batch_inds: a ({n},) tensor is expected')
        groups = batch_inds if batch_inds.dtype in (torch.int32, torch.int64) else batch_inds.to(torch.int64)
        keep_inds = _kept(bev_nms(box[:, [3, 5, 0, 2, 6]], box[:, 7], nms_thr, groups=groups))
    else:
        keep_inds = bbox_3d.new_zeros(0, dtype=torch.int64)
    return bbox_3d[keep_inds], keep_inds


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """Drop-in for the reference's `ops.iou3d.nms_gpu`: boxes (N,5) [x1, y1, x2, y2, ry], scores (N,) -> kept indices, int64, by
    descending score; only the pre_maxsize best-scored boxes take part, at most post_max_size are returned."""
    x = _f32c(boxes, 'boxes')
    if x.dim() != 2 or x.shape[1] != 5:
        raise ValueError(f'boxes: (N,5) rows [x1, y1, x2, y2, ry] expected, got {tuple(x.shape)}')
    N = int(x.shape[0])
    if not torch.is_tensor(scores) or scores.shape != (N,):
        raise ValueError(f'scores: a ({N},) fp32 tensor is expected')
    s = _f32c(scores, 'scores')
    b = torch.stack(((x[:, 0] + x[:, 2]) * 0.5, (x[:, 1] + x[:, 3]) * 0.5, x[:, 2] - x[:, 0], x[:, 3] - x[:, 1], x[:, 4]), -1)
    order = None
    if pre_maxsize is not None:
        idx = torch.sort(s, descending=True, stable=True).indices
        skip = s[idx].isnan() | (torch.arange(N, device=x.device) >= int(pre_maxsize))
        order = torch.where(skip, torch.full_like(idx, -1), idx).to(torch.int32)
    keep = _kept(bev_nms(b, s, thresh, order=order))
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


# ---- overlaps of rotated, 3D and image boxes under the reference's criteria ----------------------------------------------------------
# include/epropnp_hip.h: epropnp_box_overlap, epropnp_box_overlap_plan, epropnp_box_overlap_segmented
_KINDS = {'bev': (0, 5, '(cx, cy, dx, dy, angle)'), 'box3d': (1, 7, '[x0, x1, x2, d0, d1, d2, ry]'), 'image': (2, 4, '(x1, y1, x2, y2)')}
_CRITERIA = {'iou': -1, 'a': 0, 'b': 1, 'inter': 2}
_HEIGHT_RULES = {'interval': 0, 'reference_torch': 1}


def _rows(t, name, kind):
    _, width, what = _KINDS[kind]
    if not torch.is_tensor(t):
        raise ValueError(f'{name}: a (N,{width}) tensor is expected, got {type(t)}')
    t = _f32c(t, name)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f'{name}: (N,{width}) rows {what} expected, got {tuple(t.shape)}')
    return t


def _counts(counts, M, N):
    import ctypes as C
    try:
        ca, cb = counts
        ca, cb = [int(v) for v in ca], [int(v) for v in cb]
    except (TypeError, ValueError):
        raise ValueError('counts: a pair (counts_a, counts_b) of host integer sequences is expected') from None
    if len(ca) != len(cb):
        raise ValueError(f'counts: {len(ca)} segments of boxes_a, {len(cb)} of boxes_b')
    if min(ca + cb, default=0) < 0:
        raise ValueError('counts: a negative count')
    if sum(ca) != M or sum(cb) != N:
        raise ValueError(f'counts: the sums are {sum(ca)} and {sum(cb)}, the boxes {M} and {N}')
    G = len(ca)
    arr_a, arr_b = (C.c_int32 * max(G, 1))(*ca), (C.c_int32 * max(G, 1))(*cb)
    nt, no = C.c_int64(0), C.c_int64(0)
    _hip.call('epropnp_box_overlap_plan', arr_a, arr_b, G, None, 0, C.byref(nt), C.byref(no))
    table = torch.zeros((max(nt.value, 1), 6), dtype=torch.int32)
    _hip.call('epropnp_box_overlap_plan', arr_a, arr_b, G, C.c_void_p(table.data_ptr()), nt.value, None, None)
    return ca, cb, table, nt.value, no.value


def _box_overlaps(kind, boxes_a, boxes_b, criterion, aligned, z_axis, z_center, height_rule, counts):
    a, b = _rows(boxes_a, 'boxes_a', kind), _rows(boxes_b, 'boxes_b', kind)
    if a.device != b.device:
        raise RuntimeError(f'boxes_a lives on {a.device}, boxes_b on {b.device}')
    if criterion not in _CRITERIA:
        raise ValueError(f'criterion: one of {sorted(_CRITERIA)} is expected, got {criterion!r}')
    if height_rule not in _HEIGHT_RULES:
        raise ValueError(f'height_rule: one of {sorted(_HEIGHT_RULES)} is expected, got {height_rule!r}')
    if z_axis not in (0, 1, 2):
        raise ValueError(f'z_axis: 0, 1 or 2 is expected, got {z_axis!r}')
    M, N = int(a.shape[0]), int(b.shape[0])
    mode = (_KINDS[kind][0], _CRITERIA[criterion], int(z_axis), float(z_center), _HEIGHT_RULES[height_rule])
    if counts is not None:
        if aligned:
            raise ValueError('counts and aligned exclude each other')
        ca, cb, table, num_tiles, num_out = _counts(counts, M, N)
        out = torch.empty((num_out,), dtype=torch.float32, device=a.device)
        if num_tiles > 0:
            tiles = table.to(a.device)
            _hip.call('epropnp_box_overlap_segmented', _hip.ptr(a), M, _hip.ptr(b), N, *mode, _hip.ptr(tiles), num_tiles,
                      _hip.ptr(out), num_out, _hip.stream_of(a))
        views = [v.view(na, nb) for v, na, nb in zip(out.split([na * nb for na, nb in zip(ca, cb)]), ca, cb)] if ca else []
        return out, views
    if aligned and M != N:
        raise ValueError(f'aligned needs as many boxes_a as boxes_b, got {M} and {N}')
    out = torch.empty((N,) if aligned else (M, N), dtype=torch.float32, device=a.device)
    if M > 0 and N > 0:
        _hip.call('epropnp_box_overlap', _hip.ptr(a), M, _hip.ptr(b), N, *mode, int(bool(aligned)), _hip.ptr(out), _hip.stream_of(a))
    return out


def rotated_overlaps(boxes_a, boxes_b, criterion='iou', aligned=False, counts=None):
    """Rotated boxes (M,5), (N,5) rows (cx, cy, dx, dy, angle) -> (M,N), or (N,) aligned.  criterion: 'iou' inter / max(area_a +
    area_b - inter, 1e-8), 'a' inter / max(area_a, 1e-8), 'b' inter / max(area_b, 1e-8), each through min(., 1), or 'inter', the
    bits of `bev_overlap`.  NaN exactly where either box is invalid.
    counts=(counts_a, counts_b), host integer sequences of equal length with sums M and N: segment g pairs the next counts_a[g]
    boxes_a with the next counts_b[g] boxes_b, all segments in ONE launch -> (flat, views): the flat fp32 tensor and the list of its
    (counts_a[g], counts_b[g]) views, each the bits of the pairwise call on that segment's boxes."""
    return _box_overlaps('bev', boxes_a, boxes_b, criterion, aligned, 1, 0.5, 'interval', counts)


def box3d_overlaps(boxes_a, boxes_b, criterion='iou', aligned=False, z_axis=1, z_center=0.5, height_rule='interval', counts=None):
    """3D boxes (M,7), (N,7) rows [x0, x1, x2, d0, d1, d2, ry], shapes, criteria and counts as `rotated_overlaps` on volumes.  The
    BEV box is the two centres and sizes that are not z_axis's, and ry; the height interval is [z - h z_center, z + h (1 -
    z_center)] (z_center 0.5: centred, 1.0: z is the interval's upper end -- KITTI's bottom face with y downwards).  height_rule
    'interval' multiplies the BEV intersection by the common part of the two intervals; 'reference_torch' by max(min(hi_a, hi_b) -
    min(lo_a, lo_b), 0), what the reference's `bev_to_box3d_overlaps_aligned_torch` computes (`bbox3d_overlaps_aligned_torch`)."""
    return _box_overlaps('box3d', boxes_a, boxes_b, criterion, aligned, z_axis, z_center, height_rule, counts)


def image_overlaps(boxes_a, boxes_b, criterion='iou', counts=None):
    """Axis-aligned image boxes (M,4), (N,4) rows (x1, y1, x2, y2) -> (M,N); criteria and counts as `rotated_overlaps`.  A box with
    x2 < x1 or y2 < y1 is invalid."""
    return _box_overlaps('image', boxes_a, boxes_b, criterion, False, 1, 0.5, 'interval', counts)


# The reference's functions, by name.  Numbers: criterion -1 IoU, 0 / 1 a ratio, anything else the raw intersection.  Every 3D and
# aligned function divides by `boxes`' size for 0 and by `qboxes`' for 1; the PAIRWISE rotated functions the other way round, since
# their numba kernels call devRotateIoUEval(query_box, box) (rotate_iou_kernel.py:288-290, kitti_utils/rotate_iou.py:333-335).
def _criterion(c, swapped=False):
    if c == -1:
        return 'iou'
    if c in (0, 1):
        return 'ab'[int(c) ^ int(swapped)]
    return 'inter'


def _device(device_id, device):
    return torch.device(device) if device is not None else torch.device('cuda', int(device_id))


def _to_device(x, dev):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def bbox_rotate_overlaps(boxes, query_boxes, criterion=-1, device_id=0, device=None):
    """Drop-in for the reference's numba-CUDA `bbox_rotate_overlaps`: numpy (n,5), (k,5) -> numpy (n,k) of boxes' dtype, computed in
    fp32 on cuda:device_id (or `device`); the read-back is the synchronisation.  Criterion 0 divides by the QUERY box's area, 1 by
    `boxes`' -- the reference's pairwise kernel hands the query box over first."""
    import numpy as np
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32).astype(boxes.dtype)
    dev = _device(device_id, device)
    out = rotated_overlaps(_to_device(boxes, dev), _to_device(query_boxes, dev), _criterion(criterion, swapped=True))
    return out.cpu().numpy().astype(boxes.dtype)


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0, device=None):
    """Drop-in for kitti_utils/rotate_iou.py `rotate_iou_gpu_eval`: `bbox_rotate_overlaps` under its other name."""
    return bbox_rotate_overlaps(boxes, query_boxes, criterion, device_id, device)


def bbox_rotate_overlaps_aligned(boxes, qboxes, criterion=-1, device_id=0, device=None):
    """Drop-in for `bbox_rotate_overlaps_aligned`: numpy (n,5), (n,5) -> numpy (n,) of boxes' dtype; criterion 0 divides by
    `boxes`' area."""
    import numpy as np
    n = boxes.shape[0]
    if n == 0:
        return np.empty(0, dtype=boxes.dtype)
    dev = _device(device_id, device)
    out = rotated_overlaps(_to_device(boxes, dev), _to_device(qboxes, dev), _criterion(criterion), aligned=True)
    return out.cpu().numpy().astype(boxes.dtype)


def bbox_rotate_overlaps_aligned_torch(boxes, qboxes, criterion=-1):
    """Drop-in for `bbox_rotate_overlaps_aligned_torch`: device tensors (n,5) -> (n,) on the current stream.  Unlike the reference
    (cuda.synchronize() after its launch) it does not synchronise."""
    return rotated_overlaps(boxes, qboxes, _criterion(criterion), aligned=True)


def _clamped(x, criterion):
    """the reference's aligned 3D functions end in clip(0, 1): the ratios are there already, the raw volume is not (there the
    reference itself raises -- `ua = 1.0` has no clip -- so this is what it would return)"""
    return x if criterion in (-1, 0, 1) else x.clamp(min=0.0, max=1.0)


def bbox3d_overlaps(boxes, qboxes, criterion=-1, z_axis=1, z_center=0.5, device_id=0, device=None):
    """Drop-in for `bbox3d_overlaps`: numpy (N,7), (K,7) rows [x, y, z, l, h, w, ry] -> numpy (N,K) of boxes' dtype; criterion 0
    divides by `boxes`' volume, another number than -1 / 0 / 1 gives the intersection volume."""
    import numpy as np
    n, k = boxes.shape[0], qboxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32).astype(boxes.dtype)
    dev = _device(device_id, device)
    out = box3d_overlaps(_to_device(boxes, dev), _to_device(qboxes, dev), _criterion(criterion), z_axis=z_axis, z_center=z_center)
    return out.cpu().numpy().astype(boxes.dtype)


def bbox3d_overlaps_aligned(boxes, qboxes, criterion=-1, z_axis=1, z_center=0.5, device_id=0, device=None):
    """Drop-in for `bbox3d_overlaps_aligned`: numpy (N,7), (N,7) -> numpy (N,), clamped to [0, 1]; height rule 'interval' (the
    numpy function takes np.maximum of the two bottoms)."""
    import numpy as np
    if boxes.shape[0] == 0:
        return np.zeros(0, dtype=boxes.dtype)
    dev = _device(device_id, device)
    out = box3d_overlaps(_to_device(boxes, dev), _to_device(qboxes, dev), _criterion(criterion), aligned=True, z_axis=z_axis,
                         z_center=z_center)
    return _clamped(out, criterion).cpu().numpy().astype(boxes.dtype)


def bbox3d_overlaps_aligned_torch(boxes, qboxes, criterion=-1, z_axis=1, z_center=0.5):
    """Drop-in for `bbox3d_overlaps_aligned_torch`, the call behind the head's score targets (deform_pnp_head.py:894-899): device
    tensors (N,7) -> (N,), clamped to [0, 1], no synchronisation.  Height rule 'reference_torch': the unmodified reference takes
    torch.min of the two bottoms (bbox3d_iou_calculator.py:151), and its training targets are built with that."""
    if boxes.shape[0] == 0:
        return boxes.new_zeros(size=(0,))
    out = box3d_overlaps(boxes, qboxes, _criterion(criterion), aligned=True, z_axis=z_axis, z_center=z_center,
                         height_rule='reference_torch')
    return _clamped(out, criterion)


def image_box_overlap(boxes, query_boxes, criterion=-1, device_id=0, device=None):
    """Drop-in for kitti_utils/eval.py `image_box_overlap`: numpy (N,4), (K,4) rows (x1, y1, x2, y2) -> numpy (N,K) of boxes'
    dtype; criterion 0 divides by `boxes`' area."""
    import numpy as np
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=boxes.dtype)
    dev = _device(device_id, device)
    out = image_overlaps(_to_device(boxes, dev), _to_device(query_boxes, dev), _criterion(criterion))
    return out.cpu().numpy().astype(boxes.dtype)


def bev_box_overlap(boxes, qboxes, criterion=-1, device_id=0, device=None):
    """Drop-in for kitti_utils/eval.py `bev_box_overlap` (= `rotate_iou_gpu_eval`, with its criterion 0 / 1 order)."""
    return rotate_iou_gpu_eval(boxes, qboxes, criterion, device_id, device)


def d3_box_overlap(boxes, qboxes, criterion=-1, device_id=0, device=None):
    """Drop-in for kitti_utils/eval.py `d3_box_overlap`: numpy (N,7), (K,7) rows [x, y, z, l, h, w, ry] in KITTI's camera frame --
    y is the bottom face and points down, so z_axis = 1 and z_center = 1.0.  criterion 0 divides by `boxes`' volume; a number other
    than -1 / 0 / 1 gives 1 where the intersection volume is positive (the reference divides the volume by itself).  Positive means
    above 1e-5 of the larger box's volume: the fp32 edge integrals of two boxes that are apart cancel up to rounding, not always to 0."""
    import numpy as np
    n, k = boxes.shape[0], qboxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32).astype(boxes.dtype)
    dev = _device(device_id, device)
    a, b = _to_device(boxes, dev), _to_device(qboxes, dev)
    out = box3d_overlaps(a, b, _criterion(criterion), z_axis=1, z_center=1.0)
    if criterion not in (-1, 0, 1):
        out = (out > 1e-5 * torch.maximum(a[:, 3:6].prod(1)[:, None], b[:, 3:6].prod(1)[None, :])).to(torch.float32)
    return out.cpu().numpy().astype(boxes.dtype)


def _anno_boxes(annos, metric):
    import numpy as np
    if metric == 0:
        return np.concatenate([a['bbox'] for a in annos], 0)
    cols = [0, 2] if metric == 1 else [0, 1, 2]
    loc = np.concatenate([a['location'][:, cols] for a in annos], 0)
    dims = np.concatenate([a['dimensions'][:, cols] for a in annos], 0)
    rots = np.concatenate([a['rotation_y'] for a in annos], 0)
    return np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1)


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50, device_id=0, device=None):
    """Drop-in for kitti_utils/eval.py `calculate_iou_partly` (metric 0: image boxes, 1: BEV, 2: 3D; camera frame) -> (overlaps,
    parted_overlaps, total_gt_num, total_dt_num).  `overlaps[i]` is image i's (gts, dts) matrix; all of them come from ONE segmented
    launch over all images (the reference computes every pair of each part of ~num_examples / num_parts images and keeps the
    block diagonal).  `parted_overlaps` is reassembled from the per-image blocks because the signature returns it: the shapes are
    the reference's, pairs of different images -- which the evaluation never reads -- are 0."""
    import numpy as np
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError('unknown metric')
    total_dt_num = np.stack([len(a['name']) for a in dt_annos], 0)
    total_gt_num = np.stack([len(a['name']) for a in gt_annos], 0)
    num_examples = len(gt_annos)
    same, rest = num_examples // num_parts, num_examples % num_parts      # the reference's get_split_parts
    split_parts = [same] * num_parts + ([rest] if rest else [])
    gt_boxes, dt_boxes = _anno_boxes(gt_annos, metric), _anno_boxes(dt_annos, metric)
    dev = _device(device_id, device)
    counts = (total_gt_num.tolist(), total_dt_num.tolist())
    g, d = _to_device(gt_boxes, dev), _to_device(dt_boxes, dev)
    if metric == 0:
        flat, _ = image_overlaps(g, d, 'iou', counts=counts)
    elif metric == 1:
        flat, _ = rotated_overlaps(g, d, 'iou', counts=counts)
    else:
        flat, _ = box3d_overlaps(g, d, 'iou', z_axis=1, z_center=1.0, counts=counts)
    flat = flat.cpu().numpy().astype(gt_boxes.dtype if metric == 0 else np.float64)
    overlaps, at = [], 0
    for na, nb in zip(*counts):
        overlaps.append(flat[at:at + na * nb].reshape(na, nb))
        at += na * nb
    parted_overlaps, example_idx = [], 0
    for num_part in split_parts:
        gts, dts = total_gt_num[example_idx:example_idx + num_part], total_dt_num[example_idx:example_idx + num_part]
        part = np.zeros((int(gts.sum()), int(dts.sum())), dtype=flat.dtype)
        r = c = 0
        for i in range(num_part):
            part[r:r + gts[i], c:c + dts[i]] = overlaps[example_idx + i]
            r, c = r + int(gts[i]), c + int(dts[i])
        parted_overlaps.append(part)
        example_idx += num_part
    return overlaps, parted_overlaps, total_gt_num, total_dt_num
