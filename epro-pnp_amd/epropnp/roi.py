"""The RoI ops of the detection head's auxiliary branch: the cross-RoI logsumexp / log-softmax / softmax of its losses as one fused
op, and the RoIAlign that makes the per-RoI maps they work on.

The reference (EPro-PnP-Det epropnp_det/ops/inter_roi_ops.py) normalises a per-RoI map -- the attention logits of the active GT RoIs
(deform_pnp_head.py:985) and the per-RoI mixture log-likelihood of the reprojection loss (mvd_gaussian_mixture_nll_loss.py:50) --
across every other RoI of the same image that covers the same image position: a Python loop over images and RoIs around boolean
indexing, `affine_grid`, `grid_sample`, `masked_fill` and `logsumexp`, which synchronises with the host per RoI and cannot be captured
into a hipGraph.  `logsumexp_across_rois` is that loop in one forward and one backward launch (csrc/roi_kernels.hip); the log-softmax
and softmax are composed in PyTorch on top of it (the channel logsumexp of `extra_dim` does not commute with the bilinear sampling, so
it cannot be folded in front of it).  HIP kernels only: there is no CPU path.

`roi_align`, `roi_align_wrapper` and `extract_rois` stand in for `mmcv.ops.roi_align` (a CUDA extension this package does not depend
on), the head's wrapper of it and `DeformPnPHead.extract_rois` (deform_pnp_head.py:719-741, :1187-1196): average pooling over the
regular sample grid in its separable form, one forward and one backward launch (csrc/roi_align_kernels.hip), the backward gathered by
destination -- no zero-fill pass, no float atomics, forward and backward reproducible to the bit.  `extract_rois` sends `key` and
`value` through ONE launch each way; they share the per-RoI sampling tables.

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


def _dense_map(t, like=None):
    """a map as the kernels read it -> (tensor, channels_last).  A contiguous NCHW map and a `torch.channels_last` map are read in
    place; any other striding is copied to NCHW (`like`: the layout to follow, the key's for the value)."""
    from . import _hip
    if t.dtype != torch.float32:
        raise TypeError(f'input: the HIP path computes in fp32, got {t.dtype}')
    _hip.check_device(t, 'input')
    t = t.detach()
    cl = (not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)) if like is None else like
    return (t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()), cl


def _strides(shape, cl):
    n, c, h, w = shape
    return (h * w * c, 1, w * c, c) if cl else (c * h * w, h * w, w, 1)


def _like(shape, cl, ref):
    return torch.empty(shape, dtype=torch.float32, device=ref.device, memory_format=torch.channels_last if cl else torch.contiguous_format)


class _RoiAlign(torch.autograd.Function):
    """rois, the geometry, then one map or two maps of one shape and layout -> one output per map"""

    @staticmethod
    def forward(ctx, rois, geom, *maps):
        from . import _hip
        from .functional import _f32c
        ph, pw, scale, sampling, aligned = geom
        r = _f32c(rois, 'rois')
        first, cl = _dense_map(maps[0])
        dense = [first] + [_dense_map(m, like=cl)[0] for m in maps[1:]]
        NI, C, h, w = first.shape
        bn = r.shape[0]
        outs = [_like((bn, C, ph, pw), cl, first) for _ in dense]
        ctx.args = (bn, NI, C, h, w, ph, pw, scale, sampling, int(aligned)) + _strides(first.shape, cl) + _strides((bn, C, ph, pw), cl)
        ctx.cl, ctx.map_shape = cl, tuple(first.shape)
        pad = [None] * (2 - len(dense))
        _hip.call('epropnp_roi_align_forward', *[_hip.ptr(m) for m in dense + pad], _hip.ptr(r), *ctx.args,
                  *[_hip.ptr(o) for o in outs + pad], _hip.stream_of(first))
        ctx.save_for_backward(r)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from . import _hip
        r, = ctx.saved_tensors
        fmt = torch.channels_last if ctx.cl else torch.contiguous_format
        want = [k for k, g in enumerate(grads) if ctx.needs_input_grad[2 + k] and g is not None]
        res = [None] * len(grads)
        if want:
            cots = [grads[k].contiguous(memory_format=fmt) for k in want]
            gmaps = [_like(ctx.map_shape, ctx.cl, r) for _ in want]
            pad = [None] * (2 - len(want))
            _hip.call('epropnp_roi_align_backward', *[_hip.ptr(g) for g in cots + pad], _hip.ptr(r), *ctx.args,
                      *[_hip.ptr(g) for g in gmaps + pad], _hip.stream_of(r))
            for k, g in zip(want, gmaps):
                res[k] = g
        return (None, None) + tuple(res)


def _size(output_size):
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    if int(ph) != ph or int(pw) != pw or ph < 1 or pw < 1:
        raise ValueError(f'output_size must be a positive int or (ph, pw), got {output_size!r}')
    return int(ph), int(pw)


def _roi_align(maps, rois, output_size, spatial_scale, sampling_ratio, pool_mode, aligned, who):
    from . import _hip
    if pool_mode != 'avg':
        raise NotImplementedError(f'pool_mode {pool_mode!r}: only avg is built here')
    x = maps[0]
    if x.dim() != 4:
        raise ValueError(f'{who}: input must be (num_img, C, h, w), got {tuple(x.shape)}')
    if any(m.shape != x.shape or m.dtype != x.dtype or m.device != x.device for m in maps[1:]):
        raise ValueError(f'{who}: maps that share a launch must have one shape, dtype and device')
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError(f'{who}: rois must be (bn, 5) = [image id, x1, y1, x2, y2], got {tuple(rois.shape)}')
    if rois.requires_grad:
        raise ValueError(f'{who}: rois is not differentiable here (the boxes are treated as constants); detach it')
    ph, pw = _size(output_size)
    if int(sampling_ratio) != sampling_ratio or sampling_ratio < 0:
        raise ValueError(f'{who}: sampling_ratio must be a non-negative integer, got {sampling_ratio!r}')
    if x.numel() == 0:
        raise ValueError(f'{who}: empty input map {tuple(x.shape)}')
    dt = foreign_dtype(x)
    if dt is not None:                               # the package's dtype boundary: fp32 on the device, the caller's dtype outside
        outs = _roi_align([m.to(F32) for m in maps], rois.to(F32), (ph, pw), spatial_scale, sampling_ratio, pool_mode, aligned, who)
        return tuple(o.to(dt) for o in outs)
    if not rois.is_floating_point():
        raise TypeError(f'{who}: rois must be a floating tensor, got {rois.dtype}')
    rois = rois.to(F32)
    if not _hip.on_hip_path(*maps, rois) or rois.device != x.device:
        raise RuntimeError(f'{who}: tensors on one HIP device required (no CPU fallback)')
    geom = (ph, pw, float(spatial_scale), int(sampling_ratio), bool(aligned))
    return _RoiAlign.apply(rois, geom, *maps)


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    """mmcv.ops.roi_align with average pooling: input (NI, C, h, w), rois (bn, 5) = [image id, x1, y1, x2, y2], output_size an int or
    (ph, pw) -> (bn, C, ph, pw).  Cell (i, j) of RoI r is the mean over a gh x gw grid (sampling_ratio, or ceil(bin size) when it is
    0) of bilinear samples of the map at y = ys + i bh + (iy + .5) bh / gh, x alike, with xs = x1 spatial_scale - (0.5 if aligned else
    0) and the RoI's size clamped to >= 1 only when not aligned; a sample further than one pixel outside the map is 0, any other is
    clamped to it.  A RoI whose image id is outside [0, NI) or whose corners are not finite gives zeros and no gradient.  A contiguous
    or `torch.channels_last` input is read in place and the output follows its memory format.  Differentiable w.r.t. input."""
    return _roi_align([input], rois, output_size, spatial_scale, sampling_ratio, pool_mode, aligned, 'roi_align')[0]


def roi_align_wrapper(x, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    """The head's wrapper (deform_pnp_head.py:1187-1196): roi_align, and with no RoI at all an empty (0, C, ph, pw) that stays
    connected to autograd when x requires grad."""
    if rois.size(0) > 0:
        return roi_align(x, rois, output_size, spatial_scale, sampling_ratio, pool_mode, aligned)
    output = x.new_zeros((0, x.size(1)) + _size(output_size))
    if x.requires_grad:
        output = output + x[:0].sum()                # the reference adds x.sum(); an empty slice connects as well and reads nothing
    return output


def extract_rois(rois, img_dense_x2d, key, value, roi_shape=(28, 28), output_stride=4):
    """DeformPnPHead.extract_rois (deform_pnp_head.py:719-741) as a function: rois (bn, 5), img_dense_x2d (num_img, 2, h_img, w_img),
    key / value (num_img, embed_dim, h, w) at 1 / output_stride of the image -> x2d_roi (bn, 2, rh, rw), key_roi and value_roi
    (bn, embed_dim, rh, rw), adaptive grid, aligned.  key and value go through one forward and one backward launch and share the
    per-RoI sampling tables; the results are the bits of two separate roi_align calls."""
    rh, rw = roi_shape
    if rois.size(0) == 0:
        return tuple(roi_align_wrapper(m, rois, (rh, rw)) for m in (img_dense_x2d, key, value))
    x2d_roi = roi_align(img_dense_x2d, rois, (rh, rw), 1.0, 0, 'avg', True)
    key_roi, value_roi = _roi_align([key, value], rois, (rh, rw), 1.0 / output_stride, 0, 'avg', True, 'extract_rois')
    return x2d_roi, key_roi, value_roi
