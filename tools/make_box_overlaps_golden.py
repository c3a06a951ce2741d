"""Writes tests/golden/box3d_overlaps.npz: boxes and what the REFERENCE's numba-free overlap functions compute for them.

    python tools/make_box_overlaps_golden.py [--reference DIR] [--out FILE]

EPro-PnP-Det's core/bbox_3d/iou_calculators/bbox3d_iou_calculator.py and core/evaluation/kitti_utils/eval.py import numba (and,
through rotate_iou_calculator.py / rotate_iou.py, numba.cuda), which is not installed and has no ROCm path.  The functions around the
numba-CUDA step need neither: at run time this tool cuts the text of

    bev_to_box3d_overlaps, bev_to_box3d_overlaps_aligned, bev_to_box3d_overlaps_aligned_torch      (bbox3d_iou_calculator.py)
    d3_box_overlap_kernel, image_box_overlap, get_split_parts                                      (kitti_utils/eval.py)

out of the reference checkout (by name, with ast) and execs it with `numba.jit` stubbed to the identity and `numba.prange` to `range`.
Nothing of the reference is stored here.  In place of the numba-CUDA step (the rotated intersection area `rinc`) they are fed the fp64
Sutherland-Hodgman clip of tests/test_boxes.py.  Runs on the CPU.

Recorded (boxes are fp32 in the file; the reference functions get them as fp64, so that what is recorded is their arithmetic and not
a second fp32 rounding): 130 + 70 boxes [x, y, z, l, h, w, ry] of a clustered scene (tests/test_box_overlaps.py::scene7) for the
pairwise functions, 120 + 120 for the aligned ones, every function under criterion -1, 0, 1 and 2 (the aligned ones, which raise
under 2, under -1, 0 and 1); image boxes (x1, y1, x2, y2) of the same scene for image_box_overlap; get_split_parts(7, 3) and (6, 3);
and the detection head's slice deform_pnp_head.py:894-899 -- pose_opt (x, y, z, yaw), dim_decoded, bbox_3d_targets [l, h, w, x, y,
z, ry] and sample_weights in, ious (bbox3d_overlaps_aligned_torch's arithmetic), mean_iou and score_targets out."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'box3d_overlaps.npz')
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'epro-pnp_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
CRITERIA = (-1, 0, 1, 2)


class _Numba:
    """numba.jit / numba.jit(nopython=True, ...) as the identity, numba.prange as range"""
    prange = range

    @staticmethod
    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn


def reference_functions(ref=REF):
    """{name: function} of the six numba-free functions, exec'd from the text of the reference checkout"""
    det = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'core')
    wanted = {os.path.join(det, 'bbox_3d', 'iou_calculators', 'bbox3d_iou_calculator.py'):
              ('bev_to_box3d_overlaps', 'bev_to_box3d_overlaps_aligned', 'bev_to_box3d_overlaps_aligned_torch'),
              os.path.join(det, 'evaluation', 'kitti_utils', 'eval.py'): ('d3_box_overlap_kernel', 'image_box_overlap', 'get_split_parts')}
    out = {}
    for path, names in wanted.items():
        text = open(path).read()
        tree = ast.parse(text)
        space = {'np': np, 'torch': torch, 'numba': _Numba}
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                first = min([node.lineno] + [d.lineno for d in node.decorator_list])
                exec(compile('\n' * (first - 1) + '\n'.join(text.splitlines()[first - 1:node.end_lineno]) + '\n', path, 'exec'), space)
                out[node.name] = space[node.name]
        missing = [n for n in names if n not in out]
        if missing:
            raise RuntimeError(f'{path}: {missing} not found')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    import test_boxes as tb
    import test_box_overlaps as tbo
    ref = reference_functions(a.reference)
    rec = {}
    s = tbo.scene7(200, 1)
    pa, pb = s[:130].copy(), s[130:].copy()
    ax = [0, 2, 3, 5, 6]
    rinc = tb.oracle(pa[:, ax], pb[:, ax])[0]                  # the numba-CUDA step's result, in fp64
    rec['pair_a'], rec['pair_b'] = pa, pb
    for c in CRITERIA:
        out = rinc.copy()
        ref['bev_to_box3d_overlaps'](pa.astype(np.float64), pb.astype(np.float64), out, c, 1, 0.5)
        rec[f'bbox3d_overlaps_{c}'] = out
        out = rinc.copy()
        ref['d3_box_overlap_kernel'](pa.astype(np.float64), pb.astype(np.float64), out, c)
        rec[f'd3_box_overlap_{c}'] = out
    ia, ib = tbo.as_kind(pa, 'image'), tbo.as_kind(pb, 'image')
    rec['image_a'], rec['image_b'] = ia, ib
    for c in CRITERIA:
        rec[f'image_box_overlap_{c}'] = ref['image_box_overlap'](ia.astype(np.float64), ib.astype(np.float64), c)
    s = tbo.scene7(240, 2)
    qa, qb = s[:120].copy(), s[120:].copy()
    qb[::2] = qa[::2] + np.random.default_rng(3).normal(0.0, 0.12, (60, 7)).astype(np.float32)      # every second pair does overlap
    rinc = tb.oracle(qa[:, ax], qb[:, ax], aligned=True)[0]
    rec['aligned_a'], rec['aligned_b'] = qa, qb
    for c in CRITERIA[:3]:          # (criterion 2 raises in the reference's aligned functions: `ua = 1.0` has no clip / clamp)
        rec[f'bbox3d_overlaps_aligned_{c}'] = ref['bev_to_box3d_overlaps_aligned'](qa.astype(np.float64), qb.astype(np.float64), rinc.copy(), c, 1, 0.5)
        rec[f'bbox3d_overlaps_aligned_torch_{c}'] = ref['bev_to_box3d_overlaps_aligned_torch'](
            torch.from_numpy(qa).double(), torch.from_numpy(qb).double(), torch.from_numpy(rinc.copy()), c, 1, 0.5).numpy()
    rec['split_parts_7_3'] = np.array(ref['get_split_parts'](7, 3), dtype=np.int64)
    rec['split_parts_6_3'] = np.array(ref['get_split_parts'](6, 3), dtype=np.int64)
    # the head's slice (deform_pnp_head.py:894-899) on the aligned boxes: boxes = cat(pose_opt[:, :3], dim_decoded, pose_opt[:, 3:]),
    # qboxes = bbox_3d_targets[:, [3, 4, 5, 0, 1, 2, 6]]
    rng = np.random.default_rng(4)
    pose_opt, dim_decoded = qa[:, [0, 1, 2, 6]].copy(), qa[:, 3:6].copy()
    targets = qb[:, [3, 4, 5, 0, 1, 2, 6]].copy()
    weights = (rng.uniform(0.0, 1.0, 120) > 0.2).astype(np.float32)
    num_obj_actual = float(max(weights.sum(), 1.0))
    t_pose, t_dim, t_tgt = (torch.from_numpy(x).double() for x in (pose_opt, dim_decoded, targets))
    boxes, qboxes = torch.cat((t_pose[:, :3], t_dim, t_pose[:, 3:]), dim=-1), t_tgt[:, [3, 4, 5, 0, 1, 2, 6]]
    ious = ref['bev_to_box3d_overlaps_aligned_torch'](boxes, qboxes, torch.from_numpy(rinc.copy()), -1, 1, 0.5).reshape(-1)
    rec.update(head_pose_opt=pose_opt, head_dim_decoded=dim_decoded, head_bbox_3d_targets=targets, head_sample_weights=weights,
               head_num_obj_actual=np.float64(num_obj_actual), head_ious=ious.numpy(),
               head_mean_iou=((ious * torch.from_numpy(weights).double()).sum() / num_obj_actual).numpy(),
               head_score_targets=(2 * ious - 0.5).clamp(min=0, max=1).numpy())
    np.savez_compressed(a.out, **rec)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, {len(rec)} arrays')
    d = np.abs(rec['bbox3d_overlaps_aligned_torch_-1'] - rec['bbox3d_overlaps_aligned_-1'])
    print(f'torch.min against np.maximum: the recorded IoUs differ by up to {d.max():.3f}, by more than 0.01 on {(d > 0.01).sum()} of {d.size} pairs')


if __name__ == '__main__':
    main()
