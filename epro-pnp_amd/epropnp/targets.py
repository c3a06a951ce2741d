"""Centre targets of the detection head's training step on the device: the reference's `VolumeCenter`
(EPro-PnP-Det core/bbox_3d/center_target.py) without pytorch3d.

`DeformPnPHead.forward_train` calls `center_target.get_centers_2d(...)` before anything else: every ground-truth box is rendered with
a mesh rasteriser, the depth thickness of each box along each pixel's ray is resampled at the output cells, and the
thickness-weighted 2D centre of each object comes back with the mask of the objects that survive.  For the box mesh the
rasteriser's near / far depth pair is the ray-box slab intersection, so `volume_centers` computes the target in one fused pass that
never stores a render (include/epropnp_hip.h: epropnp_volume_centers has the definition); `box_thickness` renders what that pass
never stores, through the same device function; `VolumeCenter` is the drop-in under the reference's name and signature.
"""
import math
import warnings

import torch

from . import _hip

__all__ = ['volume_centers', 'box_thickness', 'VolumeCenter']

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
