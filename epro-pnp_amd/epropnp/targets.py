"""Centre targets of the detection head's training step on the device: the reference's `VolumeCenter`
(EPro-PnP-Det core/bbox_3d/center_target.py) without pytorch3d.

`DeformPnPHead.forward_train` calls `center_target.get_centers_2d(...)` before anything else: every ground-truth box is rendered with
a mesh rasteriser, the depth thickness of each box along each pixel's ray is resampled at the output cells, and the
thickness-weighted 2D centre of each object comes back with the mask of the objects that survive.  For the box mesh the
rasteriser's near / far depth pair is the ray-box slab intersection, so `volume_centers` computes the target in one fused pass that
never stores a render (include/epropnp_hip.h: epropnp_volume_centers has the definition); `box_thickness` renders what that pass
never stores, through the same device function; `VolumeCenter` is the drop-in under the reference's name and signature.

The two steps that follow it in `forward_train` live here as well.  `point_targets` is `self.detector.get_targets(...)`
(models/dense_heads/fcos_emb_head.py:299-438): which object, if any, each point of each level of each image is assigned to, its label
and its centerness target, in one pass that reads 6 floats per object and 2 per point and writes the flattened level-major outputs
directly (epropnp_point_targets has the definition); `get_targets` is the drop-in with the reference's lists and `fcos_points` the
point grid it is called on.  `obj_sampler` (deform_pnp_head.py:1112-1184) draws the objects the Monte-Carlo PnP runs on with
`torch.multinomial`, as the reference does, and computes their balancing weights in one launch (epropnp_obj_sample_weights).
"""
import ctypes
import math
import warnings

import torch

from . import _hip

__all__ = ['volume_centers', 'box_thickness', 'VolumeCenter', 'point_targets', 'get_targets', 'fcos_points', 'obj_sampler']

Z_CLIP = 1e-2


def _f32c(t, name, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f'{name}: a float32 tensor is expected')
    if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f'{name}: expected shape {tuple("*" if s is None else s for s in shape)}, got {tuple(t.shape)}')
    _hip.check_device(t, name)
    return t.detach().contiguous()


def _shape2(max_shape):
    """[h, w] as Python ints; a device tensor is read off the device (one synchronisation, as the reference's int(pad_shape[0]))"""
    if torch.is_tensor(max_shape):
        max_shape = max_shape.tolist()
    h, w = max_shape
    return int(math.ceil(h)), int(math.ceil(w))


def _pad_shape(max_shape, output_stride):
    h, w = _shape2(max_shape)
    return -(-h // output_stride) * output_stride, -(-w // output_stride) * output_stride


def _offsets(obj_img_inds, num_obj, num_img, dev):
    """(num_img + 1,) int32 starts of the images' objects from the ascending image indices, on the device"""
    if not torch.is_tensor(obj_img_inds) or obj_img_inds.dtype not in (torch.int32, torch.int64) or obj_img_inds.shape != (num_obj,):
        raise ValueError(f'obj_img_inds: a ({num_obj},) integer tensor is expected')
    _hip.check_device(obj_img_inds, 'obj_img_inds')
    if obj_img_inds.device != dev:
        raise RuntimeError(f'obj_img_inds lives on {obj_img_inds.device}, the boxes on {dev}')
    return torch.searchsorted(obj_img_inds.detach().to(torch.int64).contiguous(),
                              torch.arange(num_img + 1, dtype=torch.int64, device=dev)).to(torch.int32)


def _common(bboxes_3d, obj_img_inds, cam_intrinsic, render_stride, faces_per_pixel):
    b3 = _f32c(bboxes_3d, 'bboxes_3d', (None, 7))
    cam = _f32c(cam_intrinsic, 'cam_intrinsic', (None, 3, 3))
    B, G = b3.shape[0], cam.shape[0]
    if cam.device != b3.device:
        raise RuntimeError(f'cam_intrinsic lives on {cam.device}, the boxes on {b3.device}')
    rs = int(render_stride)
    if rs < 1:
        raise ValueError(f'render_stride must be >= 1, got {render_stride}')
    K = 0 if faces_per_pixel is None else int(faces_per_pixel)
    if faces_per_pixel is not None and K < 2:
        raise ValueError(f'faces_per_pixel must be >= 2 or None (no limit), got {faces_per_pixel}')
    if B > 0 and G == 0:
        raise ValueError(f'{B} objects but no image')
    return b3, cam, B, G, rs, K, _offsets(obj_img_inds, B, G, b3.device)


def _check_size(name, h, w):
    if h < 1 or h > 4096 or w < 1 or w > 4096:
        raise ValueError(f'{name} must be 1 .. 4096 in both directions, got ({h}, {w})')


def volume_centers(bboxes_3d, obj_img_inds, cam_intrinsic, img_dense_x2d_small, img_dense_x2d_mask_small, max_shape, bboxes_2d=None,
                   output_stride=4, render_stride=4, faces_per_pixel=16, z_clip=Z_CLIP, min_box_size=4.0, get_bbox_2d=False):
    """Thickness-weighted 2D centres of 3D boxes -> (centers_2d (num_obj, 2), bboxes_2d (num_obj, 4), valid (num_obj,) bool), dense:
    one row per input object, nothing read back from the device.

    bboxes_3d (num_obj, 7) = [l, h, w, x, y, z, yaw]; obj_img_inds (num_obj,) ascending; cam_intrinsic (num_img, 3, 3);
    img_dense_x2d_small (num_img, 2, h_out, w_out) the original-image pixel coordinates of each output cell and
    img_dense_x2d_mask_small (num_img, 1, h_out, w_out); max_shape [h, w] (a sequence, or a tensor: a device tensor costs one
    synchronisation).  The render grid is pad_shape // render_stride with pad_shape = ceil(max_shape / output_stride) *
    output_stride; faces_per_pixel=None means no limit.  With get_bbox_2d the boxes are those of the cells whose resampled valid
    value is >= 0.5, otherwise `bboxes_2d` passes through.  valid = (sum of thickness >= 1e-6) and both box sides >= min_box_size.
    The definition is the header comment of epropnp_volume_centers; two calls agree to the last bit."""
    b3, cam, B, G, rs, K, offsets = _common(bboxes_3d, obj_img_inds, cam_intrinsic, render_stride, faces_per_pixel)
    dev = b3.device
    os_ = int(output_stride)
    if os_ < 1:
        raise ValueError(f'output_stride must be >= 1, got {output_stride}')
    x2d = _f32c(img_dense_x2d_small, 'img_dense_x2d_small', (G, 2, None, None))
    h, w = x2d.shape[2:]
    mask = _f32c(img_dense_x2d_mask_small, 'img_dense_x2d_mask_small', (G, 1, h, w))
    pad_h, pad_w = _pad_shape(max_shape, os_)
    Hr, Wr = pad_h // rs, pad_w // rs
    _check_size('the output size', h, w)
    _check_size('the render size', Hr, Wr)
    b2 = None
    if not get_bbox_2d:
        if bboxes_2d is None:
            raise ValueError('bboxes_2d is needed unless get_bbox_2d is set')
        b2 = _f32c(bboxes_2d, 'bboxes_2d', (B, 4))
    for t, name in ((x2d, 'img_dense_x2d_small'), (mask, 'img_dense_x2d_mask_small'), (b2, 'bboxes_2d')):
        if t is not None and t.device != dev:
            raise RuntimeError(f'{name} lives on {t.device}, the boxes on {dev}')
    centers = torch.empty((B, 2), dtype=torch.float32, device=dev)
    boxes = torch.empty((B, 4), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.uint8, device=dev)
    if B > 0:
        nbytes = int(_hip.lib().epropnp_volume_centers_scratch_bytes(B, h, w))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _hip.call('epropnp_volume_centers', _hip.ptr(b3), _hip.ptr(b2), _hip.ptr(offsets), _hip.ptr(cam), _hip.ptr(x2d), _hip.ptr(mask),
                  B, G, h, w, Hr, Wr, os_, rs, K, float(z_clip), float(min_box_size), int(bool(get_bbox_2d)), _hip.ptr(scratch), nbytes,
                  _hip.ptr(centers), _hip.ptr(boxes), _hip.ptr(valid), _hip.stream_of(b3))
    return centers, boxes, valid.view(torch.bool)


def box_thickness(bboxes_3d, obj_img_inds, cam_intrinsic, max_shape, output_stride=4, render_stride=4, faces_per_pixel=16,
                  z_clip=Z_CLIP):
    """The render `volume_centers` never stores -> (thickness (num_obj, h_rend, w_rend), valid (num_obj, h_rend, w_rend) bool): per
    render pixel of the object's image the depth thickness of the box along the pixel's ray and whether both of its faces are among
    the `faces_per_pixel` nearest fragments of the image there.  Same device function as the fused pass; for tests and for looking
    at the targets."""
    b3, cam, B, G, rs, K, offsets = _common(bboxes_3d, obj_img_inds, cam_intrinsic, render_stride, faces_per_pixel)
    dev = b3.device
    pad_h, pad_w = _pad_shape(max_shape, int(output_stride))
    Hr, Wr = pad_h // rs, pad_w // rs
    _check_size('the render size', Hr, Wr)
    thick = torch.empty((B, Hr, Wr), dtype=torch.float32, device=dev)
    valid = torch.empty((B, Hr, Wr), dtype=torch.uint8, device=dev)
    if B > 0:
        nbytes = int(_hip.lib().epropnp_volume_centers_scratch_bytes(B, 0, 0))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _hip.call('epropnp_box_thickness', _hip.ptr(b3), _hip.ptr(offsets), _hip.ptr(cam), B, G, Hr, Wr, rs, K, float(z_clip),
                  _hip.ptr(scratch), nbytes, _hip.ptr(thick), _hip.ptr(valid), _hip.stream_of(b3))
    return thick, valid.view(torch.bool)


class VolumeCenter(object):
    """Drop-in for the reference's `VolumeCenter` (core/bbox_3d/center_target.py:17-259): same constructor, same
    `get_centers_2d(...)` and the same 6-tuple, computed by `volume_centers`.

    `max_gpu_obj` is accepted and ignored: there is no large temporary left to move to the host.  Not provided, with the reason in
    the error: the ellipsoid mesh and `occlusion_factor > 0`."""

    def __init__(self, base_mesh=dict(type='box'), faces_per_pixel=16, output_stride=4, render_stride=4, occlusion_factor=0.0,
                 get_bbox_2d=False, min_box_size=4.0, max_gpu_obj=-1):
        kind = base_mesh['type']
        if kind == 'ellipsoid':
            raise NotImplementedError("base_mesh=dict(type='ellipsoid'): the reference's ellipsoid is a 5120-face icosphere, not an "
                                      'analytic ellipsoid, and only the box mesh has a closed-form near / far depth pair here')
        if kind != 'box':
            raise ValueError(f"base_mesh type must be 'box', got {kind!r}")
        if occlusion_factor > 0:
            raise NotImplementedError("occlusion_factor > 0: the reference's branch calls Tensor.reshape_, which no torch has, so it "
                                      'raises AttributeError there and there is no behaviour to match')
        assert faces_per_pixel is None or faces_per_pixel <= torch.iinfo(torch.int8).max
        self.faces_per_pixel = faces_per_pixel
        self.output_stride = output_stride
        self.render_stride = render_stride
        self.occlusion_factor = occlusion_factor
        self.rend_bbox_2d = get_bbox_2d
        self.min_box_size = min_box_size
        self.max_gpu_obj = max_gpu_obj

    def get_centers_2d(self, bboxes_2d, bboxes_3d, obj_img_inds, img_dense_x2d_small, img_dense_x2d_mask_small, cam_intrinsic,
                       max_shape):
        """-> centers_2d, bboxes_2d (both filtered by valid_mask), their per-image lists, valid_mask (num_obj,) bool and
        num_obj_per_img_list (Python ints: the one read-back of the call, as in the reference)"""
        num_obj = bboxes_3d.size(0)
        num_img = cam_intrinsic.size(0)
        if num_obj == 0:
            centers_2d = bboxes_3d.new_empty((0, 2))
            bboxes_2d = bboxes_3d.new_empty((0, 4))
            valid_mask = bboxes_3d.new_empty((0, ), dtype=torch.bool)
            return centers_2d, bboxes_2d, [centers_2d] * num_img, [bboxes_2d] * num_img, valid_mask, [0] * num_img
        centers_2d, bboxes_2d, valid_mask = volume_centers(
            bboxes_3d, obj_img_inds, cam_intrinsic, img_dense_x2d_small, img_dense_x2d_mask_small, max_shape, bboxes_2d=bboxes_2d,
            output_stride=self.output_stride, render_stride=self.render_stride, faces_per_pixel=self.faces_per_pixel,
            min_box_size=self.min_box_size, get_bbox_2d=self.rend_bbox_2d)
        centers_2d = centers_2d[valid_mask]
        bboxes_2d = bboxes_2d[valid_mask]
        kept_inds = obj_img_inds[valid_mask]
        num_obj_per_img_list = torch.count_nonzero(
            kept_inds == torch.arange(num_img, device=kept_inds.device)[:, None], dim=1).tolist()
        if sum(num_obj_per_img_list) < num_obj:
            warnings.warn('Some annotated objects are disgarded. This can be triggered by small objects'
                          ' or small value of faces_per_pixel or objects outside the canvas')
        centers_2d_list = centers_2d.split(num_obj_per_img_list, dim=0)
        bboxes_2d_list = bboxes_2d.split(num_obj_per_img_list, dim=0)
        return centers_2d, bboxes_2d, centers_2d_list, bboxes_2d_list, valid_mask, num_obj_per_img_list


POINT_TARGET_CHUNK = 64      # csrc/tuning.h: PNP_PT_CHUNK, the objects of an image the kernel stages at a time (tests cross the size)
MAX_OBJ_SAMPLES = 2048       # csrc/point_target_kernels.hip: kOsMaxN


def _on(t, name, dev):
    if t.device != dev:
        raise RuntimeError(f'{name} lives on {t.device}, the points on {dev}')
    return t


def _i64c(t, name, shape):
    if not torch.is_tensor(t) or t.dtype != torch.int64:
        raise ValueError(f'{name}: an int64 tensor is expected')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    _hip.check_device(t, name)
    return t.detach().contiguous()


def point_targets(points, num_points_per_lvl, strides, regress_ranges, gt_bboxes, gt_labels, centers2d, obj_img_inds, num_img,
                  num_classes, center_sample_radius=1.5, centerness_alpha=2.5, with_strides=False):
    """Label, centerness target and assigned object of every point of every image -> (labels int64, centerness_targets float32,
    gt_inds int64, strides int64 | None, num_fg (1,) int32), the first four of length num_img * num_points in the reference's
    flattened order (level-major, then image, then the point within the level: `torch.cat` of `get_targets`' lists).  Nothing is read
    back from the device.

    points (num_points, 2), the levels' points concatenated, level 0 first; num_points_per_lvl, strides and regress_ranges one entry
    per level (at most 8; Python numbers); gt_bboxes (num_gt, 4), gt_labels (num_gt,) int64 and centers2d (num_gt, 2) of all images
    concatenated, obj_img_inds (num_gt,) ascending.  num_fg counts the points with label < num_classes.  The definition is the
    header comment of epropnp_point_targets; two calls agree to the last bit."""
    pts = _f32c(points, 'points', (None, 2))
    dev = pts.device
    P, num_img, L = pts.shape[0], int(num_img), len(num_points_per_lvl)
    boxes = _on(_f32c(gt_bboxes, 'gt_bboxes', (None, 4)), 'gt_bboxes', dev)
    G = boxes.shape[0]
    cen = _on(_f32c(centers2d, 'centers2d', (G, 2)), 'centers2d', dev)
    lab = _on(_i64c(gt_labels, 'gt_labels', (G,)), 'gt_labels', dev)
    if num_img < 0:
        raise ValueError(f'num_img must be >= 0, got {num_img}')
    if L < 1 or L > 8:
        raise ValueError(f'num_points_per_lvl: 1 .. 8 levels are expected, got {L}')
    if len(strides) != L or len(regress_ranges) != L:
        raise ValueError(f'strides and regress_ranges: one entry per level ({L}) is expected, got {len(strides)} and {len(regress_ranges)}')
    counts = [int(n) for n in num_points_per_lvl]
    if any(n < 0 for n in counts) or sum(counts) != P:
        raise ValueError(f'num_points_per_lvl: {counts} do not add up to the {P} points')
    if G > 0 and num_img == 0:
        raise ValueError(f'{G} objects but no image')
    offsets = _offsets(obj_img_inds, G, num_img, dev)
    total = num_img * P
    labels = torch.empty((total,), dtype=torch.int64, device=dev)
    centerness = torch.empty((total,), dtype=torch.float32, device=dev)
    gt_inds = torch.empty((total,), dtype=torch.int64, device=dev)
    out_strides = torch.empty((total,), dtype=torch.int64, device=dev) if with_strides else None
    if total == 0:
        return labels, centerness, gt_inds, out_strides, torch.zeros((1,), dtype=torch.int32, device=dev)
    num_fg = torch.empty((1,), dtype=torch.int32, device=dev)
    starts = [0]
    for n in counts:
        starts.append(starts[-1] + n)
    lvl = (ctypes.c_int32 * (L + 1))(*starts)
    radius = (ctypes.c_float * L)(*[float(s) * float(center_sample_radius) for s in strides])
    lo = (ctypes.c_float * L)(*[float(r[0]) for r in regress_ranges])
    hi = (ctypes.c_float * L)(*[float(r[1]) for r in regress_ranges])
    sv = (ctypes.c_int64 * L)(*[int(s) for s in strides])
    as_vp = lambda arr: ctypes.cast(arr, ctypes.c_void_p)      # noqa: E731
    _hip.call('epropnp_point_targets', _hip.ptr(pts), as_vp(lvl), as_vp(radius), as_vp(lo), as_vp(hi),
              as_vp(sv) if with_strides else None, L, _hip.ptr(boxes), _hip.ptr(cen), _hip.ptr(lab), _hip.ptr(offsets), P, G, num_img,
              int(num_classes), float(centerness_alpha), _hip.ptr(labels), _hip.ptr(centerness), _hip.ptr(gt_inds),
              _hip.ptr(out_strides), _hip.ptr(num_fg), _hip.stream_of(pts))
    return labels, centerness, gt_inds, out_strides, num_fg


def fcos_points(featmap_sizes, strides, dtype=torch.float32, device=None):
    """The point grid `FCOSEmbHead.get_points` hands to `get_targets`: per level a (h * w, 2) tensor of (x, y) =
    index * stride + stride // 2, row-major (`_get_points_single`, fcos_emb_head.py:288-297)."""
    points = []
    for (h, w), stride in zip(featmap_sizes, strides):
        stride = int(stride)
        x = torch.arange(int(w), dtype=dtype, device=device) * stride + stride // 2
        y = torch.arange(int(h), dtype=dtype, device=device) * stride + stride // 2
        points.append(torch.stack((x[None, :].expand(int(h), int(w)).reshape(-1), y[:, None].expand(int(h), int(w)).reshape(-1)), dim=-1))
    return points


def get_targets(points, gt_bboxes_list, gt_labels_list, centers2d_list, *, strides, regress_ranges, num_classes,
                center_sample_radius=1.5, centerness_alpha=2.5):
    """Drop-in for `FCOSEmbHead.get_targets` (fcos_emb_head.py:299-361) -> (labels, centerness_targets, gt_inds), each a list with
    one (num_img * num_points_of_level,) tensor per level: views of `point_targets`' flat outputs, so `torch.cat` of a list is
    free of the reference's splitting and re-concatenating.  `strides`, `regress_ranges`, `num_classes`, `center_sample_radius` and
    `centerness_alpha` are the head's attributes of the same names.  Nothing is read back from the device."""
    if len(points) != len(regress_ranges):
        raise ValueError(f'points: one tensor per regress range ({len(regress_ranges)}) is expected, got {len(points)}')
    num_img = len(gt_bboxes_list)
    if len(gt_labels_list) != num_img or len(centers2d_list) != num_img:
        raise ValueError(f'gt_labels_list and centers2d_list: one entry per image ({num_img}) is expected')
    counts = [int(p.shape[0]) for p in points]
    dev = points[0].device
    num_gt = [int(b.shape[0]) for b in gt_bboxes_list]

    def cat(ts, tail, dtype):
        return torch.cat([t.reshape((-1,) + tail) for t in ts]) if ts else torch.zeros((0,) + tail, dtype=dtype, device=dev)
    img_inds = torch.repeat_interleave(torch.arange(num_img, dtype=torch.int64), torch.tensor(num_gt, dtype=torch.int64)).to(dev)
    flat = point_targets(torch.cat(list(points)), counts, strides, regress_ranges, cat(gt_bboxes_list, (4,), torch.float32),
                         cat(gt_labels_list, (), torch.int64), cat(centers2d_list, (2,), torch.float32), img_inds, num_img,
                         num_classes, center_sample_radius=center_sample_radius, centerness_alpha=centerness_alpha)
    sizes = [num_img * n for n in counts]
    return tuple(list(t.split(sizes)) for t in flat[:3])


def obj_sampler(num_obj_samples, fg_mask, flatten_centerness_targets, flatten_gt_inds, *args, uniform_mix_ratio=0.5, eps=1e-5,
                sample_point_inds=None, generator=None):
    """Drop-in for the reference's `obj_sampler` (deform_pnp_head.py:1112-1184): draws `num_obj_samples` foreground points and
    returns (sample_gt_inds int64, sample_weights, sample_uniform_weights, *[arg[sample_point_inds] for arg in args]).

    The draws stay `torch.multinomial` on the device, exactly as in the reference: num_uniform = min(round(num_obj_samples *
    uniform_mix_ratio), foreground count) without replacement from the uniform distribution over the foreground, the others with
    replacement from prob = centerness * fg / max(sum, eps) (`generator` seeds them; a part with zero draws is skipped).
    `sample_point_inds` (num_obj_samples,) int64 injects the draws instead -- for tests and for reproducing a step -- in the
    reference's order, the uniform part first.  The weights behind the draws are one launch (epropnp_obj_sample_weights: every sum
    in a fixed order, no (num_gt, num_obj_samples) mask, no largest index).  Around it stay the foreground count's own launch
    (it has to be known before the draws, so the kernel's count cannot serve), the gathers of `args` and, without injected draws,
    the few launches that form `prob` for `torch.multinomial` and the draws themselves.

    One read-back: the foreground count.  The result has `num_obj_samples` rows or none, so the reference's contract implies it
    (there it is `if fg_mask_count > 0`, next to two more).  Without foreground the reference's empty tensors come back, with the
    same dtypes."""
    N = int(num_obj_samples)
    if N < 1 or N > MAX_OBJ_SAMPLES:
        raise ValueError(f'num_obj_samples must be 1 .. {MAX_OBJ_SAMPLES}, got {num_obj_samples}')
    if not torch.is_tensor(fg_mask) or fg_mask.dtype != torch.bool or fg_mask.dim() != 1:
        raise ValueError('fg_mask: a 1-D bool tensor is expected')
    T = fg_mask.shape[0]
    _hip.check_device(fg_mask, 'fg_mask')
    dev = fg_mask.device
    cen = _on(_f32c(flatten_centerness_targets, 'flatten_centerness_targets', (T,)), 'flatten_centerness_targets', dev)
    gts = _on(_i64c(flatten_gt_inds, 'flatten_gt_inds', (T,)), 'flatten_gt_inds', dev)
    fg = fg_mask.detach().contiguous()
    count = int(fg.count_nonzero())                                       # the one read-back
    if count == 0:
        none = torch.zeros((0,), dtype=torch.int64, device=dev)
        weights = cen[none]
        return (gts[none], weights, weights) + tuple(arg[none] for arg in args)
    wanted = int(round(N * uniform_mix_ratio))
    if wanted < 0 or wanted > N:
        raise ValueError(f'uniform_mix_ratio must lie in [0, 1], got {uniform_mix_ratio}')
    num_uniform = min(wanted, count)
    if sample_point_inds is None:
        prob = cen * fg
        prob = prob / prob.sum().clamp(min=eps)
        parts = []
        if num_uniform > 0:
            parts.append(torch.multinomial(fg / count, num_uniform, replacement=False, generator=generator))
        if N - num_uniform > 0:
            parts.append(torch.multinomial(prob, N - num_uniform, replacement=True, generator=generator))
        draws = torch.cat(parts, dim=0)
    else:
        draws = _on(_i64c(sample_point_inds, 'sample_point_inds', (N,)), 'sample_point_inds', dev)
    sample_gt_inds = torch.empty((N,), dtype=torch.int64, device=dev)
    sample_weights = torch.empty((N,), dtype=torch.float32, device=dev)
    sample_uniform_weights = torch.empty((N,), dtype=torch.float32, device=dev)
    _hip.call('epropnp_obj_sample_weights', _hip.ptr(fg.view(torch.uint8)), _hip.ptr(cen), _hip.ptr(gts), T, _hip.ptr(draws), N, wanted,
              float(eps), _hip.ptr(sample_gt_inds), _hip.ptr(sample_weights), _hip.ptr(sample_uniform_weights), None,
              _hip.stream_of(fg))
    return (sample_gt_inds, sample_weights, sample_uniform_weights) + tuple(arg[draws] for arg in args)
