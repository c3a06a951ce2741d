"""Writes tests/golden/center_target.npz: scenes and what the REFERENCE's VolumeCenter.post_proc computes for them.

    python tools/make_center_target_golden.py [--reference DIR] [--out FILE]

EPro-PnP-Det's core/bbox_3d/center_target.py imports pytorch3d, which is not installed and has no ROCm build to count on.  Only the
rasterisation step needs it.  At run time this tool cuts the text of

    VolumeCenter.post_proc                (core/bbox_3d/center_target.py)
    yaw_to_rot_mat, box_mesh              (core/bbox_3d/misc.py; `Meshes` stubbed to hold its two lists)

out of the reference checkout (by name, with ast) and execs it.  Nothing of the reference is stored here.  In place of the
pytorch3d step `post_proc` is fed the `pix_to_face` / `zbuf` of the fp64 rasteriser of tests/test_center_target.py -- the
faces_per_pixel nearest fragments per pixel, nearest first, -1 beyond them -- rounded to fp32, for the images that have objects, as
get_centers_2d selects them.  box_mesh's vertices and faces and yaw_to_rot_mat's matrices are checked against that rasteriser's.
Runs on the CPU.

Recorded per case: bboxes_3d, obj_img_inds, cam_intrinsic, the x2d map and its mask, bboxes_2d, max_shape, strides, faces_per_pixel,
min_box_size, and centers_2d / bboxes_2d / valid_mask of post_proc for get_bbox_2d False and True (centres of objects without
thickness are the reference's 0 / 0 = nan)."""
import argparse
import ast
import os
import sys
import textwrap
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'center_target.npz')
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'epro-pnp_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
CASES = [('main', (96, 160), 4, 4, 16, 'identity'), ('main', (94, 158), 4, 4, 16, 'crop'), ('main', (96, 160), 4, 2, 16, 'shift'),
         ('row', (96, 160), 4, 4, 4, 'identity')]


class _Meshes:
    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces


def _cut(path, names, space, inside=None):
    """exec the functions `names` of `path` (methods of class `inside`, dedented, when given) in `space`"""
    text = open(path).read()
    body = ast.parse(text).body
    if inside is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == inside).body
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            src = textwrap.dedent('\n'.join(text.splitlines()[node.lineno - 1:node.end_lineno]) + '\n')
            exec(compile('\n' * (node.lineno - 1) + src, path, 'exec'), space)
    missing = [n for n in names if n not in space]
    if missing:
        raise RuntimeError(f'{path}: {missing} not found')
    return space


def reference_functions(ref=REF):
    core = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'core', 'bbox_3d')
    space = _cut(os.path.join(core, 'misc.py'), ('yaw_to_rot_mat', 'box_mesh'), {'np': np, 'torch': torch, 'Meshes': _Meshes})
    space.update(_cut(os.path.join(core, 'center_target.py'), ('post_proc',), {'torch': torch, 'F': F, 'warnings': warnings},
                      inside='VolumeCenter'))
    return space


class _Self:
    occlusion_factor = 0.0

    def __init__(self, fpp, os_, get_bbox, min_box):
        self.faces_per_pixel, self.output_stride, self.rend_bbox_2d, self.min_box_size = fpp, os_, get_bbox, min_box


def fragments(tc, boxes, K, Hr, Wr, rs, fpp, first_obj):
    """(zbuf, pix_to_face) (Hr, Wr, fpp) of one image: the fpp nearest fragments beyond z_clip, nearest first, -1 beyond them"""
    t = tc.face_depths(tc.box_vertices(boxes), K, Hr, Wr, rs, 0.0, 0.0)          # (n, 6, P)
    n, P = len(boxes), Hr * Wr
    with np.errstate(invalid='ignore'):
        flat = np.where(t > tc.Z_CLIP, t, np.inf).reshape(n * 6, P)
    order = np.argsort(flat, axis=0, kind='stable')[:fpp]
    z = np.take_along_axis(flat, order, 0)
    face = (first_obj + order // 6) * 12 + 2 * (order % 6)                       # the first triangle of the face
    none = ~np.isfinite(z)
    z, face = np.where(none, -1.0, z), np.where(none, -1, face)
    pad = fpp - z.shape[0]
    if pad > 0:
        z, face = np.concatenate((z, -np.ones((pad, P)))), np.concatenate((face, -np.ones((pad, P), dtype=face.dtype)))
    return z.T.reshape(Hr, Wr, fpp), face.T.reshape(Hr, Wr, fpp)


def record(ref=REF):
    import math
    import test_center_target as tc
    fn = reference_functions(ref)
    mesh = fn['box_mesh']()
    assert np.array_equal(mesh.verts[0].numpy().astype(np.float64), tc.VERTS) and np.array_equal(mesh.faces[0].numpy(), tc.FACES)
    rec = {}
    for ci, (name, max_shape, os_, rs, fpp, kind) in enumerate(CASES):
        boxes, inds, cams = tc.SCENES[name]()
        R = fn['yaw_to_rot_mat'](torch.from_numpy(boxes[:, 6])).numpy().astype(np.float64)
        verts = np.einsum('nij,nvj->nvi', R, tc.VERTS[None] * 0.5 * boxes[:, None, :3].astype(np.float64)) + boxes[:, None, 3:6]
        assert np.abs(verts - tc.box_vertices(boxes)).max() < 1e-5
        pad = [int(math.ceil(s / os_)) * os_ for s in max_shape]
        Hr, Wr = pad[0] // rs, pad[1] // rs
        h, w = pad[0] // os_, pad[1] // os_
        x2d, mask = tc.x2d_maps(kind, len(cams), h, w, os_)
        has = np.array([(inds == g).any() for g in range(len(cams))])
        zbuf, p2f = [], []
        for g in np.nonzero(has)[0]:
            z, f = fragments(tc, boxes[inds == g], cams[g], Hr, Wr, rs, fpp, int((inds < g).sum()))
            zbuf.append(z)
            p2f.append(f)
        zbuf, p2f = torch.from_numpy(np.stack(zbuf)).float(), torch.from_numpy(np.stack(p2f)).long()
        inds_new = torch.from_numpy((np.cumsum(has) - 1)[inds]).long()
        b2 = np.tile(np.array([10.0, 12.0, 50.0, 40.0], dtype=np.float32), (len(boxes), 1))
        b2[0] = [10.0, 12.0, 13.0, 40.0]
        tag = f'c{ci}_'
        rec.update({tag + 'bboxes_3d': boxes, tag + 'obj_img_inds': inds.astype(np.int64), tag + 'cam_intrinsic': cams, tag + 'x2d': x2d,
                    tag + 'mask': mask, tag + 'bboxes_2d': b2,
                    tag + 'params': np.array([max_shape[0], max_shape[1], os_, rs, fpp, 4.0], dtype=np.float64)})
        for get_bbox in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                c, b, v = fn['post_proc'](_Self(fpp, os_, get_bbox, 4.0), zbuf.clone(), p2f.clone(), torch.from_numpy(x2d[has]),
                                          torch.from_numpy(mask[has]), torch.tensor([float(pad[0]), float(pad[1])]), len(boxes),
                                          inds_new, torch.from_numpy(b2.copy()), 12)
            rec.update({f'{tag}centers_{int(get_bbox)}': c.numpy(), f'{tag}boxes_{int(get_bbox)}': b.numpy(),
                        f'{tag}valid_{int(get_bbox)}': v.numpy()})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    rec = record(a.reference)
    np.savez_compressed(a.out, **rec)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, {len(rec)} arrays')
    for k in sorted(rec):
        if '_valid_' in k:
            print(k, rec[k].astype(int))


if __name__ == '__main__':
    main()
