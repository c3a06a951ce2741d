"""Writes tests/golden/point_targets.npz: the scenes of tests/test_point_targets.py and what the REFERENCE's FCOSEmbHead.get_targets
and obj_sampler compute for them.

    python tools/make_point_target_golden.py --reference DIR [--out FILE]          (or EPROPNP_REFERENCE=DIR)

EPro-PnP-Det's models/dense_heads/fcos_emb_head.py and deform_pnp_head.py import mmcv and mmdet, which are not installed and have no
ROCm build to count on; the functions recorded here need neither.  At run time this tool cuts the text of

    FCOSEmbHead._get_points_single, .get_targets, ._get_target_single      (models/dense_heads/fcos_emb_head.py)
    obj_sampler                                                            (models/dense_heads/deform_pnp_head.py)

out of the reference checkout (by name, with ast) and execs it.  Nothing of the reference is stored here.  Supplied in their place:
a one-line `multi_apply`, `INF = 1e8`, a base class whose `_get_points_single` is the (y, x) index meshgrid mmdet's AnchorFreeHead
returns, and a `self` that holds the six attributes the methods read (strides, regress_ranges, num_classes, center_sampling,
center_sample_radius, centerness_alpha).  `obj_sampler` is handed a `torch` stand-in whose `multinomial` records what it returned, so
that the fixture holds the draws.  Runs on the CPU.

Recorded per scene ('main', 'chunk'): the points per level, the objects, and get_targets' three lists per level.  Recorded per sampler
case (on the main scene's flattened targets, num_obj_samples 24): fg_mask, uniform_mix_ratio, two extra per-point arrays, the draws
and the outputs."""
import argparse
import ast
import os
import sys
import textwrap
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'point_targets.npz')
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'epro-pnp_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
NUM_OBJ_SAMPLES = 24
SAMPLER_CASES = [('half', 0.5, None), ('few', 0.5, 5), ('most', 0.75, None)]      # name, uniform_mix_ratio, keep only the first n foreground points


def multi_apply(func, *args, **kwargs):
    return tuple(map(list, zip(*map(partial(func, **kwargs), *args))))


class _Base:
    def _get_points_single(self, featmap_size, stride, dtype, device, flatten=False):
        h, w = featmap_size
        return torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device), indexing='ij')


class _RecordingTorch:
    """`torch` with a multinomial that remembers its results"""

    def __init__(self):
        self.draws = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def multinomial(self, *args, **kwargs):
        out = torch.multinomial(*args, **kwargs)
        self.draws.append(out)
        return out


def _source(path, names, inside=None):
    """the text of the functions `names` of `path` (methods of class `inside` when given), as it stands in the file"""
    text = open(path).read()
    body = ast.parse(text).body
    if inside is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == inside).body
    found = {n.name: '\n'.join(text.splitlines()[n.lineno - 1:n.end_lineno]) + '\n' for n in body
             if isinstance(n, ast.FunctionDef) and n.name in names}
    missing = [n for n in names if n not in found]
    if missing:
        raise RuntimeError(f'{path}: {missing} not found')
    return [found[n] for n in names]


def reference_functions(ref):
    heads = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'models', 'dense_heads')
    path = os.path.join(heads, 'fcos_emb_head.py')
    methods = _source(path, ('_get_points_single', 'get_targets', '_get_target_single'), inside='FCOSEmbHead')
    space = {'torch': torch, 'multi_apply': multi_apply, 'INF': 1e8, '_Base': _Base}
    # the methods go back into a class statement, so that the zero-argument super() of _get_points_single finds its cell
    exec(compile('class Head(_Base):\n' + ''.join(textwrap.indent(textwrap.dedent(m), '    ') for m in methods), path, 'exec'), space)
    recorder = _RecordingTorch()
    path = os.path.join(heads, 'deform_pnp_head.py')
    sampler = {'torch': recorder}
    exec(compile(_source(path, ('obj_sampler',))[0], path, 'exec'), sampler)
    return space['Head'], sampler['obj_sampler'], recorder


def record(ref):
    import test_point_targets as tp
    Head, obj_sampler, recorder = reference_functions(ref)
    head = Head()
    head.strides, head.regress_ranges, head.num_classes = tp.STRIDES, tp.RANGES, tp.NUM_CLASSES
    head.center_sampling, head.center_sample_radius, head.centerness_alpha = True, tp.RADIUS, tp.ALPHA
    sizes = [(tp.SHAPE[0] // s, tp.SHAPE[1] // s) for s in tp.STRIDES]
    points = [head._get_points_single(size, s, torch.float32, 'cpu') for size, s in zip(sizes, tp.STRIDES)]
    rec = {'featmap_sizes': np.array(sizes, dtype=np.int64), 'strides': np.array(tp.STRIDES, dtype=np.int64),
           'regress_ranges': np.array(tp.RANGES, dtype=np.float64),
           'params': np.array([tp.NUM_CLASSES, tp.RADIUS, tp.ALPHA, NUM_OBJ_SAMPLES], dtype=np.float64)}
    for k, p in enumerate(points):
        rec[f'points_lvl{k}'] = p.numpy()
    flat = {}
    for name, (make, num_img) in tp.SCENES.items():
        boxes, centres, labels, img = make()
        per_img = lambda a: [torch.from_numpy(a[img == i]) for i in range(num_img)]      # noqa: E731
        got = head.get_targets(points, per_img(boxes), per_img(labels), per_img(centres))
        rec.update({f'{name}_gt_bboxes': boxes, f'{name}_centers2d': centres, f'{name}_gt_labels': labels,
                    f'{name}_obj_img_inds': img.astype(np.int64), f'{name}_num_img': np.array(num_img)})
        for what, lists in zip(('labels', 'centerness', 'gt_inds'), got):
            for k, t in enumerate(lists):
                rec[f'{name}_{what}_lvl{k}'] = t.numpy()
        flat[name] = tuple(torch.cat(lists) for lists in got)
    labels, centerness, gt_inds = flat['main']
    T = labels.numel()
    rng = np.random.RandomState(11)
    extra_f = torch.from_numpy(rng.randn(T, 3).astype(np.float32))
    extra_i = torch.cat([torch.full((3 * len(p),), s, dtype=torch.int64) for p, s in zip(points, tp.STRIDES)])
    rec.update({'sampler_centerness': centerness.numpy(), 'sampler_gt_inds': gt_inds.numpy(), 'sampler_extra_f': extra_f.numpy(),
                'sampler_extra_i': extra_i.numpy()})
    torch.manual_seed(3)
    for name, ratio, keep in SAMPLER_CASES:
        fg = labels < tp.NUM_CLASSES
        if keep is not None:
            fg = fg & (torch.cumsum(fg.long(), 0) <= keep)
        recorder.draws.clear()
        out = obj_sampler(NUM_OBJ_SAMPLES, fg, centerness.clone(), gt_inds.clone(), extra_f, extra_i, uniform_mix_ratio=ratio)
        draws = torch.cat(recorder.draws)
        assert len(recorder.draws) == 2 and draws.numel() == NUM_OBJ_SAMPLES and torch.equal(gt_inds[draws], out[0])
        rec.update({f'sampler_{name}_fg_mask': fg.numpy(), f'sampler_{name}_ratio': np.array(ratio),
                    f'sampler_{name}_num_uniform': np.array(recorder.draws[0].numel()), f'sampler_{name}_draws': draws.numpy()})
        for what, t in zip(('gt_inds', 'weights', 'uniform_weights', 'extra_f', 'extra_i'), out):
            rec[f'sampler_{name}_out_{what}'] = t.numpy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('EPROPNP_REFERENCE'), help='the reference checkout (or EPROPNP_REFERENCE)')
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    if not a.reference:
        ap.error('--reference DIR (or EPROPNP_REFERENCE) is needed')
    rec = record(a.reference)
    np.savez_compressed(a.out, **rec)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, {len(rec)} arrays')
    for name, _, _ in SAMPLER_CASES:
        print(name, 'num_uniform', int(rec[f'sampler_{name}_num_uniform']), 'objects drawn', sorted(set(rec[f'sampler_{name}_out_gt_inds'].tolist())))


if __name__ == '__main__':
    main()
