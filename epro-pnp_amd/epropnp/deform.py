"""The deformable attention sampler of the detection head as one fused op (forward + backward kernels) and a drop-in module.

The reference (EPro-PnP-Det epropnp_det/ops/deformable_attention_sampler.py:77-137, called from deform_pnp_head.py:447-451) makes
the correspondences of the PnP layer here: for every object, head and point it samples the key map, the value map, the dense 2-D
coordinate map and its validity mask at a learned location -- four `F.grid_sample` calls on permuted 5-D views with the image index
as a third grid axis --, attends over the points of a head (softmax, two batched matmuls) and returns the attended feature next to
the raw samples that `forward_correspondence` turns into x3d / x2d / w2d.  `sample_attend` is that composite in one launch
(csrc/deform_kernels.hip); the arithmetic in front of it (centre + offset x stride) and behind it (out_proj, LayerNorm, FFN) stays
PyTorch.  HIP kernels only: tensors that are not fp32 on a HIP device raise.
"""
import torch
import torch.nn as nn

MAX_POINTS, MAX_HEAD_DIM = 64, 64


def _map(t, name, like=None):
    """a key / value map as the kernel reads it -> (tensor, (sN, sC, sH, sW), channels_last).  A `torch.channels_last` map and a
    contiguous NCHW map are read in place; anything else is copied to NCHW (`like`: the layout to follow, the key's for the value)."""
    from . import _hip
    if t.dtype != torch.float32:
        raise TypeError(f'{name}: the HIP path computes in fp32, got {t.dtype}')
    _hip.check_device(t, name)
    t = t.detach()
    _, E, h, w = t.shape
    cl = (not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)) if like is None else like
    t = t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()
    return t, ((h * w * E, 1, w * E, E) if cl else (E * h * w, h * w, w, 1)), cl


class _SampleAttend(torch.autograd.Function):
    """outputs in the kernel's point-major layouts: attn (B,E), v (B,H,P,D), a (B,H,P), mask (B,H,P), x2d (B,H,P,2)"""

    @staticmethod
    def forward(ctx, query, key, value, dense_x2d, dense_mask, location, obj_img_ind, stride):
        from . import _hip
        from .functional import _f32c
        B, H, _, D = query.shape
        NI, E, h, w = key.shape
        P = location.shape[2]
        q, lc = _f32c(query, 'query'), _f32c(location, 'sampling_location')
        x2, mk = _f32c(dense_x2d, 'dense_x2d'), _f32c(dense_mask, 'dense_mask')
        k, strides, cl = _map(key, 'key')
        v, _, _ = _map(value, 'value', like=cl)
        im = obj_img_ind.to(torch.int64).contiguous()
        dev = q.device
        attn = torch.empty((B, E), dtype=torch.float32, device=dev)
        vs = torch.empty((B, H, P, D), dtype=torch.float32, device=dev)
        a = torch.empty((B, H, P), dtype=torch.float32, device=dev)
        ms = torch.empty((B, H, P), dtype=torch.float32, device=dev)
        xs = torch.empty((B, H, P, 2), dtype=torch.float32, device=dev)
        stats = torch.empty((B, H, 2), dtype=torch.float32, device=dev)
        ctx.dims = (B, NI, H, P, D, h, w, int(stride)) + strides
        _hip.call('epropnp_deform_sample_forward', _hip.ptr(q), _hip.ptr(k), _hip.ptr(v), _hip.ptr(x2), _hip.ptr(mk), _hip.ptr(lc),
                  _hip.ptr(im), *ctx.dims, _hip.ptr(attn), _hip.ptr(vs), _hip.ptr(a), _hip.ptr(ms), _hip.ptr(xs), _hip.ptr(stats),
                  _hip.stream_of(q))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, x2, mk, lc, im, stats)
        return attn, vs, a, ms, xs

    @staticmethod
    def backward(ctx, *grads):
        from . import _hip
        q, k, v, x2, mk, lc, im, stats = ctx.saved_tensors
        want_q, want_k, want_v, _, _, want_l, _, _ = ctx.needs_input_grad
        if all(g is None for g in grads) or not (want_q or want_k or want_v or want_l):
            return (None,) * 8
        g = [None if t is None else t.contiguous() for t in grads]
        shape, strides = tuple(k.shape), ctx.dims[8:]
        # zero-filled by the library, then scattered into; the memory format of the maps
        like_map = lambda: torch.empty((k.numel(),), dtype=torch.float32, device=k.device).as_strided(shape, strides)
        gq = torch.empty_like(q) if want_q else None
        gl = torch.empty_like(lc) if want_l else None
        gk = like_map() if want_k else None
        gv = like_map() if want_v else None
        _hip.call('epropnp_deform_sample_backward', _hip.ptr(q), _hip.ptr(k), _hip.ptr(v), _hip.ptr(x2), _hip.ptr(mk), _hip.ptr(lc),
                  _hip.ptr(im), _hip.ptr(stats), *(_hip.ptr(t) for t in g), *ctx.dims, _hip.ptr(gq), _hip.ptr(gk), _hip.ptr(gv),
                  _hip.ptr(gl), _hip.stream_of(q))
        return gq, gk, gv, None, None, gl, None, None


def sample_attend(query, key, value, dense_x2d, dense_mask, sampling_location, obj_img_ind, stride):
    """query (B,H,1,D), key / value (NI,E,h,w) with E = H*D (contiguous or `torch.channels_last`: the fast layout, one corner of one
    head is D contiguous floats), dense_x2d (NI,2,h,w), dense_mask (NI,1,h,w), sampling_location (B,H,P,2) in input-image pixels
    [x, y], obj_img_ind (B,) integer, stride (int, the map's stride)
      -> attn (B,E), v_samples (B,H,D,P), a_samples (B,H,1,P), mask_samples (B,H,1,P), x2d_samples (B,H,2,P)
    as deformable_attention_sampler.py:84-137 computes them (`attn` is what it feeds to out_proj).  v_samples and x2d_samples are
    transposed views of point-major buffers, as the reference's are permuted views.  Map coordinates are x / stride - 0.5; k, v and
    x2d clamp them to the map (border padding), the mask pads with zeros.  A non-finite location samples the border-mode maps at
    coordinate 0 with mask_samples = 0 and no location gradient along that axis; obj_img_ind is clamped to [0, NI - 1] on the device.
    Differentiable w.r.t. query, key, value and sampling_location."""
    from . import _hip
    if query.dim() != 4 or query.size(2) != 1:
        raise ValueError(f'query must be (num_obj, num_heads, 1, head_dim), got {tuple(query.shape)}')
    B, H, _, D = query.shape
    if key.dim() != 4 or key.shape != value.shape or key.size(1) != H * D:
        raise ValueError(f'key and value must both be (num_img, {H * D}, h, w), got {tuple(key.shape)} and {tuple(value.shape)}')
    NI, E, h, w = key.shape
    if sampling_location.dim() != 4 or sampling_location.shape[:2] != (B, H) or sampling_location.size(3) != 2:
        raise ValueError(f'sampling_location must be ({B}, {H}, num_points, 2), got {tuple(sampling_location.shape)}')
    P = sampling_location.size(2)
    if tuple(dense_x2d.shape) != (NI, 2, h, w) or tuple(dense_mask.shape) != (NI, 1, h, w):
        raise ValueError(f'dense_x2d / dense_mask must be ({NI}, 2 / 1, {h}, {w}), got {tuple(dense_x2d.shape)} and {tuple(dense_mask.shape)}')
    if tuple(obj_img_ind.shape) != (B,) or obj_img_ind.dtype.is_floating_point:
        raise ValueError(f'obj_img_ind must be ({B},) integer')
    if not 1 <= P <= MAX_POINTS or not 1 <= D <= MAX_HEAD_DIM:
        raise ValueError(f'num_points {P} / head_dim {D} outside the kernel limits 1 .. {MAX_POINTS} / 1 .. {MAX_HEAD_DIM}')
    if H < 1 or NI < 1 or h < 1 or w < 1 or int(stride) != stride or stride < 1:
        raise ValueError('num_heads, num_img, h, w must be >= 1 and stride a positive integer')
    ts = (query, key, value, dense_x2d, dense_mask, sampling_location)
    if not _hip.on_hip_path(*ts) or obj_img_ind.device != query.device:
        raise RuntimeError('sample_attend: fp32 tensors on one HIP device required (no CPU fallback)')
    if B == 0:       # empty detection batch: nothing to launch; correctly shaped empty tensors that stay connected to autograd
        z = query.sum() + sampling_location.sum() + key.flatten()[:0].sum() + value.flatten()[:0].sum()
        return tuple(query.new_zeros(s) + z for s in ((0, E), (0, H, D, P), (0, H, 1, P), (0, H, 1, P), (0, H, 2, P)))
    attn, vs, a, ms, xs = _SampleAttend.apply(query, key, value, dense_x2d, dense_mask, sampling_location, obj_img_ind, int(stride))
    return attn, vs.transpose(2, 3), a.unsqueeze(2), ms.unsqueeze(2), xs.transpose(2, 3)


class _FFN(nn.Module):
    """Linear-ReLU-Dropout (num_fcs - 1 times), Linear, Dropout, plus the identity; parameters named as mmcv 1.x's FFN names them
    (`layers.0.0.*`, `layers.1.*` for two layers)."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type='ReLU', inplace=True),
                 add_identity=True, **unused):
        super().__init__()
        assert num_fcs >= 2, f'num_fcs must be at least 2, got {num_fcs}'
        if act_cfg.get('type') != 'ReLU':
            raise NotImplementedError(f"FFN activation {act_cfg.get('type')!r}: only ReLU is built here")
        layers, width = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(width, feedforward_channels), nn.ReLU(inplace=bool(act_cfg.get('inplace', False))),
                                        nn.Dropout(ffn_drop)))
            width = feedforward_channels
        layers += [nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop)]
        self.layers = nn.Sequential(*layers)
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        out = self.layers(x)
        if not self.add_identity:
            return out
        return (x if identity is None else identity) + out


class DeformableAttentionSampler(nn.Module):
    """The reference's module (deformable_attention_sampler.py:16-142) over `sample_attend`: same constructor arguments and defaults,
    same `forward` signature and return tuple.  The layers around the sampling are plain torch (no mmcv)."""

    def __init__(self, embed_dims=256, num_heads=8, num_points=32, stride=4,
                 ffn_cfg=dict(type='FFN', embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.1,
                              act_cfg=dict(type='ReLU', inplace=True)),
                 norm_cfg=dict(type='LN'), init_cfg=None):
        super().__init__()
        assert embed_dims % num_heads == 0, 'embed_dims must be a multiple of num_heads'
        self.embed_dims, self.num_heads, self.num_points, self.stride = embed_dims, num_heads, num_points, stride
        self.ffn_cfg, self.norm_cfg = ffn_cfg, norm_cfg
        if norm_cfg.get('type') != 'LN':
            raise NotImplementedError(f"norm layer {norm_cfg.get('type')!r}: only LN is built here")
        norm_args = {k: v for k, v in norm_cfg.items() if k not in ('type', 'requires_grad')}
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_points * 2)
        self.out_proj = nn.Linear(embed_dims, embed_dims)
        self.layer_norms = nn.ModuleList([nn.LayerNorm(embed_dims, **norm_args) for _ in range(2)])
        if ffn_cfg.get('type', 'FFN') != 'FFN':
            raise NotImplementedError(f"feed-forward network {ffn_cfg.get('type')!r}: only FFN is built here")
        self.ffn = _FFN(**{k: v for k, v in ffn_cfg.items() if k != 'type'})
        self.init_weights()

    def init_weights(self):
        nn.init.xavier_uniform_(self.sampling_offsets.weight, gain=2.5)       # mmcv's xavier_init(gain=2.5, distribution='uniform')
        nn.init.constant_(self.sampling_offsets.bias, 0)
        self._is_init = True

    def forward(self, query, obj_emb, key, value, img_dense_x2d, img_dense_x2d_mask, obj_xy_point, strides, obj_img_ind):
        """query (num_obj, num_head, 1, head_emb_dim), obj_emb (num_obj, embed_dim), key / value (num_img, embed_dim, h, w),
        img_dense_x2d (num_img, 2, h, w), img_dense_x2d_mask (num_img, 1, h, w), obj_xy_point (num_obj, 2), strides (num_obj,),
        obj_img_ind (num_obj,) -> output (num_obj, embed_dim), v_samples (num_obj, num_head, head_emb_dim, num_point),
        a_samples (num_obj, num_head, 1, num_point), mask_samples (num_obj, num_head, 1, num_point),
        x2d_samples (num_obj, num_head, 2, num_point)"""
        num_obj = query.size(0)
        offsets = self.sampling_offsets(obj_emb).reshape(num_obj, self.num_heads, self.num_points, 2)
        sampling_location = obj_xy_point[:, None, None] + offsets * strides[:, None, None, None]
        attn, v_samples, a_samples, mask_samples, x2d_samples = sample_attend(
            query, key, value, img_dense_x2d, img_dense_x2d_mask, sampling_location, obj_img_ind, self.stride)
        output = self.out_proj(attn) + obj_emb
        output = self.layer_norms[0](output)
        output = self.ffn(output, output)
        output = self.layer_norms[1](output)
        return output, v_samples, a_samples, mask_samples, x2d_samples
