"""Writes tests/golden/roi_across.npz: inputs and what the REFERENCE's cross-RoI ops and its reprojection loss compute for them.

    python tools/make_roi_golden.py [--reference DIR] [--out FILE]

The reference's `ops/inter_roi_ops.py` (EPro-PnP-Det; it needs nothing but torch) and `models/losses/mvd_gaussian_mixture_nll_loss.py`
are imported from the reference checkout at run time -- nothing of them is stored here.  The loss file imports mmdet, which is not
installed, and the ops through a relative import, so it is loaded as a module of a stub package tree in sys.modules: `mmdet.core` with
`reduce_mean` as the identity (one process), `mmdet.models` with `LOSSES` as a registry whose decorator returns the class and
`weighted_loss` restated from mmdet's rule (the weight multiplies element-wise; 'mean' with an avg_factor is sum / avg_factor; 'sum'
with an avg_factor raises), and `<pkg>.ops` with the reference's own `logsumexp_across_rois`.  Runs on the CPU.

Three cases (n, images, c, rh, rw): a (9,2,3,5,7), b (6,1,8,14,14), c (5,2,1,28,28), each with fenced boxes (tests/test_roi.py:
draw_rois -- no cell centre within 1e-3, in grid units, of a border of a neighbour's box, seeds counted upwards per box, the same on
every run).  Per case: the map x and a cotangent, both on a grid of 1/4 and stored as int8 (x = q / 4, exactly; the file has to stay
small), rois, the reference's logsumexp_across_rois(x, rois), logsoftmax_across_rois(x, rois, extra_dim=1), its autograd gradient of
sum(logsumexp * cotangent), and for the loss: pred / target / logstd / logmixweight on a grid of 1/8 as int8 (the target of case a
is a tensor, of b the integer -1, of c the integer 0), the module's reduction='none' output in training mode and its buffer afterwards.
"""
import argparse
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'roi_across.npz')
# (n, images, c, rh, rw), first seed, number of mixture components, the loss target
CASES = {'a': ((9, 2, 3, 5, 7), 2100, 3, 'tensor'), 'b': ((6, 1, 8, 14, 14), 2200, 2, -1), 'c': ((5, 2, 1, 28, 28), 2300, 2, 0)}
SPEC = ((30.0, 170.0), (40.0, 160.0))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_modules(ref=REF):
    """(inter_roi_ops, mvd_gaussian_mixture_nll_loss) of the reference checkout"""
    det = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det')
    ops = _load('reference_inter_roi_ops', os.path.join(det, 'ops', 'inter_roi_ops.py'))

    def weighted_loss(fn):
        @functools.wraps(fn)
        def wrapper(pred, target, weight=None, reduction='mean', avg_factor=None, **kwargs):
            loss = fn(pred, target, **kwargs)
            if weight is not None:
                loss = loss * weight
            if avg_factor is None:
                return loss.mean() if reduction == 'mean' else (loss.sum() if reduction == 'sum' else loss)
            if reduction == 'mean':
                return loss.sum() / avg_factor
            if reduction != 'none':
                raise ValueError('avg_factor can not be used with reduction="sum"')
            return loss
        return wrapper

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls
    pkg = 'reference_det'
    stubs = {name: types.ModuleType(name) for name in ('mmdet', 'mmdet.core', 'mmdet.models', pkg, pkg + '.ops', pkg + '.models',
                                                       pkg + '.models.losses')}
    for m in stubs.values():
        m.__path__ = []
    stubs['mmdet.core'].reduce_mean = lambda t: t
    stubs['mmdet.models'].LOSSES = Registry()
    stubs['mmdet.models'].weighted_loss = weighted_loss
    stubs[pkg + '.ops'].logsumexp_across_rois = ops.logsumexp_across_rois
    saved = {name: sys.modules.get(name) for name in stubs}
    sys.modules.update(stubs)
    try:
        loss = _load(pkg + '.models.losses.mvd_gaussian_mixture_nll_loss', os.path.join(det, 'models', 'losses', 'mvd_gaussian_mixture_nll_loss.py'))
    finally:
        for name, old in saved.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return ops, loss


def _grid(shape, sigma, step, g):
    """N(0, sigma^2) on a grid of 1 / step -> the int8 numerators"""
    return (sigma * step * torch.randn(shape, generator=g)).round().clamp(-127, 127).to(torch.int8)


def make(ref=REF):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_roi
    ops, loss_mod = reference_modules(ref)
    out = {}
    for name, ((n, images, c, rh, rw), seed, mix, target) in CASES.items():
        rois = test_roi.draw_rois(n, images, rh, rw, seed, SPEC)
        assert int(test_roi._pairs(rois).any(1).sum()) * 2 >= n, f'case {name}: too few RoIs overlap'
        g = torch.Generator().manual_seed(seed + 7)
        xq, cq = _grid((n, c, rh, rw), 3.0, 4, g), _grid((n, c, rh, rw), 1.0, 4, g)
        x = (xq.float() / 4).requires_grad_(True)
        lse = ops.logsumexp_across_rois(x, rois)
        grad = torch.autograd.grad((lse * (cq.float() / 4)).sum(), x)[0]
        with torch.no_grad():
            lsm = ops.logsoftmax_across_rois(x.detach(), rois, extra_dim=1)
        out.update({f'{name}_x_q4': xq.numpy(), f'{name}_cot_q4': cq.numpy(), f'{name}_rois': rois.numpy(),
                    f'{name}_logsumexp': lse.detach().numpy(), f'{name}_logsoftmax_dim1': lsm.numpy(), f'{name}_grad': grad.numpy()})
        pq, tq = _grid((n, mix, rh, rw, 2), 2.0, 8, g), _grid((n, mix, rh, rw, 2), 2.0, 8, g)
        sq, mq = _grid((n, mix, rh, rw, 2), 0.5, 8, g), _grid((n, mix, rh, rw), 1.0, 8, g)
        m = loss_mod.MVDGaussianMixtureNLLLoss(reduction='none')
        with torch.no_grad():
            tgt = tq.float() / 8 if target == 'tensor' else target
            val = m(pq.float() / 8, tgt, logstd=sq.float() / 8, logmixweight=mq.float() / 8, rois=rois)
        out.update({f'{name}_pred_q8': pq.numpy(), f'{name}_logstd_q8': sq.numpy(), f'{name}_logmixweight_q8': mq.numpy(),
                    f'{name}_loss': val.numpy(), f'{name}_mean_inv_std': m.mean_inv_std.numpy().copy()})
        if target == 'tensor':
            out[f'{name}_target_q8'] = tq.numpy()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    data = make(a.reference)
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), {k: v.shape for k, v in data.items()})
