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
