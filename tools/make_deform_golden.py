"""Writes tests/golden/deform_sampler.npz: inputs and what the REFERENCE's DeformableAttentionSampler computes for them.

    python tools/make_deform_golden.py [--reference DIR] [--out FILE]

The reference's module (EPro-PnP-Det epropnp_det/ops/deformable_attention_sampler.py) is imported from the reference checkout at run
time -- nothing of it is stored here -- with stub `mmcv.cnn`, `mmcv.cnn.bricks.transformer` and `mmcv.cnn.bricks.registry` modules in
sys.modules (mmcv is not installed): a registry whose decorator returns the class, torch's Xavier initialisation, nn.LayerNorm and the
package's own plain-torch FFN.  None of those layers reaches the fixture: a forward pre-hook on `out_proj` captures `attn`, the tensor
the sampling produces, and the four sample tensors are the module's own return values.  Runs on the CPU.  Two cases, (B,NI,H,P,D,h,w):
    a  (7,3,2,5,4,6,9), map stride 4
    b  (4,1,8,16,32,4,6), map stride 8
The sampling locations are chosen, not learned: obj_emb is one-hot per object and column b of the `sampling_offsets` weight holds
object b's offsets (bias 0), so the module's Linear returns them exactly; the fixture stores the location the module then forms,
obj_xy_point + offsets * strides in fp32.  Object strides are drawn from {8, 16, 32}.  A case is fenced: no map coordinate within
1e-3 px of an integer (pixel centres, the clamp borders, the mask's borders); the seeds are tried upwards from the case's first seed
per coordinate, each coordinate keeping the value of the first seed that passes (a whole draw of hundreds of coordinates at 0.2 %
each rarely does), the same ones on every run: the file regenerates bit for bit.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'deform_sampler.npz')
CASES = {'a': dict(shape=(7, 3, 2, 5, 4, 6, 9), stride=4, seed=1100), 'b': dict(shape=(4, 1, 8, 16, 32, 4, 6), stride=8, seed=1200)}
FENCE = 1e-3


def reference_class(ref=REF):
    path = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'ops', 'deformable_attention_sampler.py')
    sys.path.insert(0, os.path.join(ROOT, 'epro-pnp_amd'))
    from epropnp.deform import _FFN

    def xavier_init(module, gain=1, bias=0, distribution='normal'):
        (torch.nn.init.xavier_uniform_ if distribution == 'uniform' else torch.nn.init.xavier_normal_)(module.weight, gain=gain)
        torch.nn.init.constant_(module.bias, bias)

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls
    stubs = {name: types.ModuleType(name) for name in ('mmcv', 'mmcv.cnn', 'mmcv.cnn.bricks', 'mmcv.cnn.bricks.transformer',
                                                       'mmcv.cnn.bricks.registry')}
    stubs['mmcv.cnn'].xavier_init = xavier_init
    stubs['mmcv.cnn'].build_norm_layer = lambda cfg, dims: ('ln', torch.nn.LayerNorm(dims))
    stubs['mmcv.cnn.bricks.transformer'].build_feedforward_network = lambda cfg, default=None: _FFN(**{k: v for k, v in cfg.items() if k != 'type'})
    stubs['mmcv.cnn.bricks.registry'].ATTENTION = Registry()
    saved = {name: sys.modules.get(name) for name in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location('reference_deformable_attention_sampler', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in saved.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return mod.DeformableAttentionSampler


def draw(shape, stride, seed):
    B, NI, H, P, D, h, w = shape
    g = torch.Generator().manual_seed(seed)
    t = {'query': torch.randn(B, H, 1, D, generator=g), 'key': torch.randn(NI, H * D, h, w, generator=g),
         'value': torch.randn(NI, H * D, h, w, generator=g)}
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    t['dense_x2d'] = ((torch.stack((xx, yy)) + 0.5)[None] * stride + 0.3 * stride * torch.randn(NI, 2, h, w, generator=g)).contiguous()
    t['dense_mask'] = (torch.rand(NI, 1, h, w, generator=g) > 0.3).float()
    t['obj_img_ind'] = torch.randint(0, NI, (B,), generator=g)
    t['obj_xy_point'] = torch.rand(B, 2, generator=g) * torch.tensor([w * stride, h * stride], dtype=torch.float32)
    t['strides'] = torch.tensor([8.0, 16.0, 32.0])[torch.randint(0, 3, (B,), generator=g)]
    t['offsets'] = 0.7 * torch.randn(B, H, P, 2, generator=g)
    return t


def location(t):
    return t['obj_xy_point'][:, None, None] + t['offsets'] * t['strides'][:, None, None, None]


def fence(t, stride):
    c = location(t).double() / stride - 0.5
    return (c - c.round()).abs() >= FENCE


def make(ref=REF):
    cls = reference_class(ref)
    out = {}
    for name, c in CASES.items():
        shape, stride = c['shape'], c['stride']
        B, NI, H, P, D, h, w = shape
        t = draw(shape, stride, c['seed'])
        ok, tries = fence(t, stride), 0
        while not ok.all():
            tries += 1
            assert tries < 50, f'case {name}: the fence does not close'
            t['offsets'] = torch.where(ok, t['offsets'], draw(shape, stride, c['seed'] + tries)['offsets'])
            ok = fence(t, stride)
        E = H * D
        assert E >= B
        torch.manual_seed(0)
        m = cls(embed_dims=E, num_heads=H, num_points=P, stride=stride,
                ffn_cfg=dict(type='FFN', embed_dims=E, feedforward_channels=2 * E, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type='ReLU', inplace=True))).eval()
        with torch.no_grad():
            m.sampling_offsets.weight.zero_()
            m.sampling_offsets.bias.zero_()
            m.sampling_offsets.weight[:, :B] = t['offsets'].reshape(B, H * P * 2).t()
        obj_emb = torch.zeros(B, E)
        obj_emb[torch.arange(B), torch.arange(B)] = 1.0
        seen = {}
        m.out_proj.register_forward_pre_hook(lambda mod, args: seen.__setitem__('attn', args[0].detach().clone()))
        with torch.no_grad():
            assert torch.equal(m.sampling_offsets(obj_emb).reshape(B, H, P, 2), t['offsets'])
            _, v, a, mask, x2d = m(t['query'], obj_emb, t['key'], t['value'], t['dense_x2d'], t['dense_mask'], t['obj_xy_point'], t['strides'],
                                   t['obj_img_ind'])
        out[f'{name}_stride'] = np.int64(stride)
        for k in ('query', 'key', 'value', 'dense_x2d', 'dense_mask', 'obj_img_ind'):
            out[f'{name}_{k}'] = t[k].numpy()
        out[f'{name}_sampling_location'] = location(t).numpy()
        for k, x in (('attn', seen['attn']), ('v_samples', v), ('a_samples', a), ('mask_samples', mask), ('x2d_samples', x2d)):
            out[f'{name}_{k}'] = np.ascontiguousarray(x.numpy(), dtype=np.float32)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    data = make(a.reference)
    np.savez(a.out, **data)
    print(a.out, {k: v.shape for k, v in data.items()})
