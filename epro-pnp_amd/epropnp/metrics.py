"""Pose-error metrics of the 6-DoF evaluation on the device: rotation / translation error, ARP-2D, ADD and ADD-S.

The reference scores a pose on the host, one object at a time (EPro-PnP-6DoF lib/test.py:227-238 converts `pose_opt` to numpy
rotation matrices, lib/utils/eval.py runs re / te / arp_2d / add / adi in a Python loop, with one scipy cKDTree per symmetric
object).  `pose_errors` does it for all B poses -- or for S x B pose samples against B ground truths -- in two launches
(include/epropnp_hip.h: epropnp_pose_errors), so that the metric can also be asked of the layer's pose distribution:

    p_correct = (logw.softmax(0) * (pose_errors(pose_samples, pose_gt, ...).add_or_adi < 0.1 * diameter)).sum(0)

Runs on the current HIP stream of the inputs' device, allocates its outputs and scratch with torch.empty, never synchronises and
can be captured into a hipGraph.  Not differentiable: inputs are detached.
"""
from collections import namedtuple

import torch

from . import _hip
from .functional import _f32c

WORDS = 8             # include/epropnp_hip.h: EPROPNP_POSE_ERROR_WORDS
QUERY_TILE = 1024     # EPROPNP_POSE_ERROR_QUERY_TILE: model points per ADD-S query tile (one scratch float per row and tile)
CAND_TILE = 1024      # EPROPNP_POSE_ERROR_CAND_TILE: model points per LDS tile of ADD-S candidates

PoseErrors = namedtuple('PoseErrors', ['rot_deg', 'trans', 'arp_2d', 'add', 'adi', 'add_or_adi', 'raw'])
PoseErrors.__doc__ = """Per-pose errors (views of `raw`); (B,) each for pose_est (B,P), (S,B) for (S,B,P).

rot_deg     rotation angle between estimate and ground truth in degrees
trans       |t_est - t_gt|
arp_2d      mean re-projection distance of the model points in pixels; NaN without cam_mats
add         mean distance of the model points under the two poses
adi         ADD-S, mean distance to the nearest model point under the other pose; NaN where `symmetric` is not set
add_or_adi  adi where `symmetric`, else add (the reference's calc_all_errs)
raw         (B,8) | (S,B,8): the row layout of include/epropnp_hip.h: epropnp_pose_errors"""


def pack_models(models):
    """[(M_c,3) tensors] -> (points (Mtot,3) fp32, range (C,2) int32 of (first, count)) on the models' device: the packed form
    `pose_errors` takes.  Done once per dataset (it copies); an empty model is allowed and gives NaN rows."""
    models = list(models)
    if not models:
        raise ValueError('pack_models: at least one model is needed')
    for m in models:
        if not torch.is_tensor(m) or m.dim() != 2 or m.shape[1] != 3:
            raise ValueError(f'pack_models: (M,3) tensors expected, got {tuple(m.shape) if torch.is_tensor(m) else type(m)}')
    counts = [int(m.shape[0]) for m in models]
    firsts = [sum(counts[:i]) for i in range(len(counts))]
    pts = torch.cat([m.detach().to(torch.float32) for m in models], 0).contiguous()
    if pts.shape[0] == 0:
        pts = torch.zeros((1, 3), dtype=torch.float32, device=pts.device)
    rng = torch.tensor(list(zip(firsts, counts)), dtype=torch.int32).to(pts.device)
    return pts, rng


def _mask(m, name, B, device):
    if m is None:
        return None
    if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8) or m.shape != (B,):
        raise ValueError(f'{name}: a ({B},) bool tensor is expected')
    if m.device != device:
        raise RuntimeError(f'{name} lives on {m.device}, the poses on {device}')
    return m.detach().to(torch.uint8).contiguous()


def pose_errors(pose_est, pose_gt, model_points, model_range=None, model_id=None, cam_mats=None, symmetric=None, half_turn=None):
    """Errors of pose_est (B,P) | (S,B,P) against pose_gt (B,P), P = 7 (x, y, z, quaternion w i j k) or 4 (x, y, z, yaw)
    -> PoseErrors.  Not differentiable (inputs are detached).

    model_points, model_range: what `pack_models` returns; or one model as an (M,3) tensor with model_range None.
    model_id   (B,) int32 | None   the model of each object (None: model 0)
    cam_mats   (3,3) | (B,3,3) | None   intrinsics for arp_2d
    symmetric  (B,) bool | None    objects scored by ADD-S (the reference's eggbox and glue): fills adi, switches add_or_adi
    half_turn  (B,) bool | None    objects with the reference's eggbox rule: beyond 90 degrees of raw rotation error rot_deg, trans
                                   and arp_2d are taken with the estimate turned by pi about its z axis (4-DoF: yaw + pi)
    Quaternions are normalised first.  A pose that is not finite, a model_id outside the packed models and an empty model give NaNs
    in their own rows only."""
    est = _f32c(pose_est, 'pose_est')
    gt = _f32c(pose_gt, 'pose_gt')
    pts = _f32c(model_points, 'model_points')
    if gt.dim() != 2 or gt.shape[-1] not in (4, 7) or est.dim() not in (2, 3) or est.shape[-2:] != gt.shape:
        raise ValueError(f'pose_est (B,4|7) or (S,B,4|7) and pose_gt (B,4|7) expected, got {tuple(est.shape)} and {tuple(gt.shape)}')
    if est.dim() == 3 and est.shape[0] < 1:
        raise ValueError('at least one pose row per object is needed')
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f'model_points: (Mtot,3) with Mtot >= 1 expected, got {tuple(pts.shape)}')
    B, P = gt.shape
    R = 1 if est.dim() == 2 else est.shape[0]
    dev, dof = gt.device, 4 if P == 4 else 6
    if model_range is None:
        if model_id is not None:
            raise ValueError('model_id needs the model_range of pack_models')
        rng = torch.empty((1, 2), dtype=torch.int32, device=dev)      # written with fill launches (no host-to-device copy: capturable)
        rng[:, 0].fill_(0)
        rng[:, 1].fill_(int(pts.shape[0]))
    else:
        rng = model_range
        if not torch.is_tensor(rng) or rng.dtype != torch.int32 or rng.dim() != 2 or rng.shape[1] != 2 or rng.shape[0] < 1:
            raise ValueError('model_range: a (C,2) int32 tensor of (first, count) is expected (pack_models)')
        _hip.check_device(rng, 'model_range')
        rng = rng.detach().contiguous()
    mid = None
    if model_id is not None:
        if not torch.is_tensor(model_id) or model_id.dtype != torch.int32 or model_id.shape != (B,):
            raise ValueError(f'model_id: a ({B},) int32 tensor is expected')
        _hip.check_device(model_id, 'model_id')
        mid = model_id.detach().contiguous()
    cam = None
    if cam_mats is not None:
        cam = _f32c(cam_mats, 'cam_mats')
        if cam.shape == (3, 3):
            cam = cam.expand(B, 3, 3).contiguous()
        elif cam.shape != (B, 3, 3):
            raise ValueError(f'cam_mats: (3,3) or {(B, 3, 3)} expected, got {tuple(cam.shape)}')
    sym = _mask(symmetric, 'symmetric', B, dev)
    half = _mask(half_turn, 'half_turn', B, dev)
    raw = torch.empty(tuple(est.shape[:-1]) + (WORDS,), dtype=torch.float32, device=dev)
    if B > 0:
        scratch, nbytes = None, 0
        if sym is not None:
            # sized for the largest model the packed points can hold: no look at model_range, which lives on the device
            tiles = (int(pts.shape[0]) + QUERY_TILE - 1) // QUERY_TILE
            scratch = torch.empty((R * B * tiles,), dtype=torch.float32, device=dev)
            nbytes = scratch.numel() * 4
        _hip.call('epropnp_pose_errors', _hip.ptr(est), _hip.ptr(gt), R, B, dof, _hip.ptr(pts), _hip.ptr(rng), int(rng.shape[0]),
                  _hip.ptr(mid), _hip.ptr(cam), _hip.ptr(sym), _hip.ptr(half), _hip.ptr(scratch), nbytes, _hip.ptr(raw),
                  _hip.stream_of(gt))
    return PoseErrors(rot_deg=raw[..., 0], trans=raw[..., 1], arp_2d=raw[..., 2], add=raw[..., 3], adi=raw[..., 4],
                      add_or_adi=raw[..., 5], raw=raw)
