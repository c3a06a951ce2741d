"""The cross-RoI logsumexp / log-softmax / softmax of the detection head's auxiliary losses as one fused op.

The reference (EPro-PnP-Det epropnp_det/ops/inter_roi_ops.py) normalises a per-RoI map -- the attention logits of the active GT RoIs
(deform_pnp_head.py:985) and the per-RoI mixture log-likelihood of the reprojection loss (mvd_gaussian_mixture_nll_loss.py:50) --
across every other RoI of the same image that covers the same image position: a Python loop over images and RoIs around boolean
indexing, `affine_grid`, `grid_sample`, `masked_fill` and `logsumexp`, which synchronises with the host per RoI and cannot be captured
into a hipGraph.  `logsumexp_across_rois` is that loop in one forward and one backward launch (csrc/roi_kernels.hip); the log-softmax
and softmax are composed in PyTorch on top of it (the channel logsumexp of `extra_dim` does not commute with the bilinear sampling, so
it cannot be folded in front of it).  HIP kernels only: there is no CPU path.

`rois` is not differentiable here (the callers' RoIs are GT boxes): `rois.requires_grad` raises instead of returning a silent zero.
"""
import torch

from ._dtype import F32, foreign_dtype

MAX_CELLS = 64 * 64


class _RoiLogSumExp(torch.autograd.Function):

    @staticmethod
    def forward(ctx, roi_inputs, rois):
        from . import _hip
        from .functional import _f32c
        x, r = _f32c(roi_inputs, 'roi_inputs'), _f32c(rois, 'rois')
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ctx.dims = tuple(x.shape)
        _hip.call('epropnp_roi_logsumexp_forward', _hip.ptr(x), _hip.ptr(r), *ctx.dims, _hip.ptr(out), _hip.stream_of(x))
        ctx.save_for_backward(x, r, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _hip
        x, r, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        g = grad_out.contiguous()
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _hip.call('epropnp_roi_logsumexp_backward', _hip.ptr(x), _hip.ptr(r), _hip.ptr(out.detach()), _hip.ptr(g), *ctx.dims, _hip.ptr(gx),
                  _hip.stream_of(x))
        return gx, None


def logsumexp_across_rois(roi_inputs, rois):
    """roi_inputs (bn, chn, rh, rw), rois (bn, 5) = [image id, x1, y1, x2, y2] -> (bn, chn, rh, rw): per RoI, channel and cell the log
    of exp(own value) + the sum of exp(bilinear sample) over the other RoIs of the same image whose box strictly contains the cell
    centre (inter_roi_ops.py:19-81).  A RoI without such a neighbour returns its input bit for bit.  Differentiable w.r.t. roi_inputs."""
    from . import _hip
    if roi_inputs.dim() != 4:
        raise ValueError(f'roi_inputs must be (bn, chn, rh, rw), got {tuple(roi_inputs.shape)}')
    bn, chn, rh, rw = roi_inputs.shape
    if tuple(rois.shape) != (bn, 5):
        raise ValueError(f'rois must be ({bn}, 5), got {tuple(rois.shape)}')
    if rois.requires_grad:
        raise ValueError('logsumexp_across_rois: rois is not differentiable here (the boxes are treated as constants); detach it')
    if roi_inputs.numel() == 0:                      # nothing to launch; as the reference: a copy that stays connected to autograd
        return roi_inputs.clone()
    if rh * rw > MAX_CELLS:
        raise ValueError(f'rh * rw = {rh * rw} exceeds the kernel limit {MAX_CELLS}')
    dt = foreign_dtype(roi_inputs)
    if dt is not None:                               # the package's dtype boundary: fp32 on the device, the caller's dtype outside
        return logsumexp_across_rois(roi_inputs.to(F32), rois.to(F32)).to(dt)
    if not rois.is_floating_point():
        raise TypeError(f'rois must be a floating tensor, got {rois.dtype}')
    rois = rois.to(F32)
    if not _hip.on_hip_path(roi_inputs, rois) or rois.device != roi_inputs.device:
        raise RuntimeError('logsumexp_across_rois: tensors on one HIP device required (no CPU fallback)')
    return _RoiLogSumExp.apply(roi_inputs, rois)


def logsoftmax_across_rois(roi_inputs, rois, extra_dim=None):
    """roi_inputs - logsumexp_across_rois(roi_inputs, rois); with `extra_dim` the normaliser is also summed over that dimension
    (inter_roi_ops.py:84-96)."""
    if extra_dim:
        return roi_inputs - logsumexp_across_rois(roi_inputs, rois).logsumexp(dim=extra_dim, keepdim=True)
    return roi_inputs - logsumexp_across_rois(roi_inputs, rois)


def softmax_across_rois(roi_inputs, rois, extra_dim=None):
    """exp of logsoftmax_across_rois (inter_roi_ops.py:99-107)."""
    return logsoftmax_across_rois(roi_inputs, rois, extra_dim).exp()
