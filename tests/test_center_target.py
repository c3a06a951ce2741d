"""epropnp.targets.box_thickness / volume_centers (epropnp_box_thickness, epropnp_volume_centers) against fp64 oracles written here.

Geometry: `box_thickness` against a brute-force fp64 rasteriser -- the 12 triangles of the reference's box mesh per object, the ray of
each render pixel's centre against each triangle (so the depth is perspective-correct), the two triangles of a face merged (a
pixel on a face's diagonal counts once), fragments <= z_clip dropped, the K nearest kept per image pixel, count == 2.  Thickness
changes fast under grazing faces, so a pixel is accepted if the kernel's value lies within [min, max] of the fp64 thickness over the
pixel centre shifted by 0 and by +-DELTA px in u and in v (DELTA = 2^-10 px: a few fp32 ulps of a 1600 px coordinate), widened by
THICK_BAR x t_far.  Excluded: a pixel where in fp64 a fragment lies within 1e-4 relative of z_clip, or where K binds and fragments of
two objects lie within 1e-4 relative of each other.  Asserted from the oracle alone, before anything is compared: at most 2 % of a
scene's hit pixels are excluded, and on the others the five shifted rasterisations agree on validity.  There validity must agree
exactly.

End to end: `volume_centers` against the fp64 restatement of the resampling and the sums (post_proc, center_target.py:213-259) fed by
that rasteriser.  Box and valid must agree exactly; the scenes keep the resampled valid value 1e-3 away from 0.5 in fp64 (asserted).

Shapes: 3 images (the middle one without objects), 9 objects, max_shape (96, 160) and (94, 158), strides 4 / 4: a 24 x 40 render and
24 x 40 cells, six 16 x 16 tiles per image, partly filled; plus output_stride 4 with render_stride 2.

Bars: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over every case of this file (each case prints
its worst error); test_bars_under_caps holds them under the caps.
    centre     |centre - centre64| px                         emulation 9.778e-6, MI355X 9.077e-6   -> bar 3.911e-5, cap 1e-2
               (1e-2 px is 1 % of the smooth-L1 beta and about 80 fp32 ulps at 1600)
    thickness  distance from [min, max] / t_far               emulation 0, MI355X 0                 -> bar 0, cap 1e-4
               (every fp32 thickness of every case lies inside the fp64 range over the shifts: the range of 2^-10 px is wider than
               the fp32 error of the slab test at these depths, so the bar adds nothing to it)
"""
import math

import numpy as np
import pytest
import torch

CENTER_BAR = 3.911e-5    # px; cap 1e-2
THICK_BAR = 0.0          # relative to t_far, beyond the fp64 range over the shifts; cap 1e-4
CENTER_CAP, THICK_CAP = 1e-2, 1e-4
DELTA = 2.0 ** -10
Z_CLIP = 1e-2

VERTS = np.array([[-1, -1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, 1], [-1, -1, -1], [1, -1, -1], [-1, 1, -1], [1, 1, -1]], dtype=np.float64)
FACES = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 7], [2, 7, 6], [1, 7, 3], [1, 5, 7], [6, 7, 4], [7, 5, 4], [0, 4, 1], [1, 4, 5],
                  [2, 6, 4], [0, 2, 4]])      # box_mesh(): consecutive pairs are the two triangles of one face


def _mod():
    from epropnp import targets
    return targets


def dev(x, backend):
    return torch.from_numpy(np.ascontiguousarray(x)).to(backend)


# ---- scenes (built once, never modified) -----------------------------------------------------------------------------------------------
def cam(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def scene_main():
    """3 images, the middle one empty.  Image 0: boxes at varied yaw and one that straddles the near plane.  Image 2: the camera inside
    a box, a box behind the camera, one off the canvas, a far small one, an ordinary one."""
    boxes = np.array([
        [4.2, 1.6, 1.8, -3.0, 0.9, 12.0, 0.3],
        [3.9, 1.5, 1.7, 2.5, 1.0, 9.0, -1.1],
        [4.5, 1.9, 2.0, 5.5, 0.7, 22.0, 2.4],
        [2.2, 2.1, 2.3, 1.7, 0.2, 0.6, 0.45],       # straddles z = 0: the faces at z < z_clip are cut away
        [3.1, 2.9, 3.3, 0.2, 0.1, 0.4, 0.2],        # the camera is inside
        [4.0, 1.6, 1.8, 0.5, 1.0, -10.0, 0.7],      # behind the camera
        [4.0, 1.6, 1.8, 60.0, 1.0, 10.0, 0.1],      # off the canvas
        [3.8, 1.5, 1.7, -9.0, 1.2, 58.0, 1.3],      # far: about two cells
        [4.1, 1.7, 1.9, 1.0, 1.1, 15.0, 1.9],
    ], dtype=np.float32)
    inds = np.array([0, 0, 0, 0, 2, 2, 2, 2, 2])
    cams = np.stack([cam(118.0, 121.0, 79.5, 47.5), cam(100.0, 100.0, 80.0, 48.0), cam(131.0, 127.0, 75.25, 50.75)])
    return boxes, inds, cams


def scene_row():
    """three boxes in a row along the optical axis: with faces_per_pixel = 4 the last one loses the pixels the first two cover"""
    boxes = np.array([[2.4, 1.9, 1.7, 0.3, 0.2, 8.0, 0.2], [4.2, 3.3, 1.6, 0.1, 0.3, 14.0, -0.3], [7.1, 5.5, 1.8, -0.2, 0.1, 21.0, 0.15]],
                     dtype=np.float32)
    return boxes, np.array([0, 0, 0]), np.stack([cam(125.0, 125.0, 79.5, 47.5)])


SCENES = {'main': scene_main, 'row': scene_row}


# ---- the fp64 rasteriser ---------------------------------------------------------------------------------------------------------------
def box_vertices(boxes):
    b = boxes.astype(np.float64)
    v = VERTS[None] * 0.5 * b[:, None, :3]
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    R = np.zeros((len(b), 3, 3))
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1.0, -s, c
    return np.einsum('nij,nvj->nvi', R, v) + b[:, None, 3:6]


def face_depths(verts, K, Hr, Wr, rs, du, dv):
    """(n, 6, Hr * Wr) depth at which the ray of each render pixel's centre (+ (du, dv) px) meets each face; nan for a miss"""
    K = K.astype(np.float64)
    c, r = np.meshgrid(np.arange(Wr, dtype=np.float64), np.arange(Hr, dtype=np.float64))
    u, v = rs * (c + 0.5) - 0.5 + du, rs * (r + 0.5) - 0.5 + dv
    d = np.stack(((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)), -1).reshape(-1, 3)      # (P, 3), origin 0
    tri = verts[:, FACES]                                                                                       # (n, 12, 3, 3)
    v0, e1, e2 = tri[:, :, 0], tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        p = np.cross(d[None, None], e2[:, :, None])                  # (n, 12, P, 3)
        det = np.einsum('ntk,ntpk->ntp', e1, p)
        tv = -v0
        bu = np.einsum('ntk,ntpk->ntp', tv, p) / det
        q = np.cross(tv, e1)                                         # (n, 12, 3)
        bv = np.einsum('pk,ntk->ntp', d, q) / det
        t = np.einsum('ntk,ntk->nt', e2, q)[:, :, None] / det
        hit = (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1)
    t = np.where(hit, t, np.nan).reshape(len(verts), 6, 2, -1)
    return np.fmin(t[:, :, 0], t[:, :, 1])       # (fmin / fmax skip a nan operand)


def render_image(boxes, K, Hr, Wr, rs, fpp, du=0.0, dv=0.0):
    """objects of ONE image -> thickness (n, P), valid (n, P), hit (n, P), excluded (n, P), t_far (n, P)"""
    n = len(boxes)
    P = Hr * Wr
    if n == 0:
        z = np.zeros((0, P))
        return z, z.astype(bool), z.astype(bool), z.astype(bool), z
    t = face_depths(box_vertices(boxes), K, Hr, Wr, rs, du, dv)       # (n, 6, P)
    hit = np.isfinite(t).any(1)
    with np.errstate(invalid='ignore'):
        near_clip = (np.abs(t - Z_CLIP) <= 1e-4 * Z_CLIP).any(1)
        frag = np.where(t > Z_CLIP, t, np.inf)
    flat = frag.reshape(n * 6, P)
    order = np.argsort(flat, axis=0, kind='stable')
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(n * 6)[:, None].repeat(P, 1), axis=0)
    kept = np.isfinite(flat) & ((rank < fpp) if fpp else True)
    kept = kept.reshape(n, 6, P)
    valid = kept.sum(1) == 2
    tk = np.where(kept, frag, np.nan)
    far, near = np.fmax.reduce(tk, axis=1), np.fmin.reduce(tk, axis=1)
    thick = np.where(valid, far - near, 0.0)
    far = np.where(valid, far, 0.0)
    excl = near_clip.copy()
    if fpp:
        binding = np.isfinite(flat).sum(0) > fpp
        owner = np.arange(n).repeat(6)
        srt = np.take_along_axis(flat, order, 0)
        own = owner[order]
        with np.errstate(invalid='ignore'):
            close = (np.abs(srt[1:] - srt[:-1]) <= 1e-4 * np.abs(srt[1:])) & np.isfinite(srt[1:]) & (own[1:] != own[:-1])
        excl |= (binding & close.any(0))[None] & hit
    return thick, valid, hit, excl, far


_oracle_cache = {}


def oracle(name, max_shape, os_, rs, fpp):
    """per object over its image's render grid: thick, valid, hit, excl, far, lo, hi (thickness range over the shifts), agree"""
    key = (name, max_shape, os_, rs, fpp)
    if key not in _oracle_cache:
        boxes, inds, cams = SCENES[name]()
        pad = [int(math.ceil(s / os_)) * os_ for s in max_shape]
        Hr, Wr = pad[0] // rs, pad[1] // rs
        out = {k: np.zeros((len(boxes), Hr * Wr), dtype=(np.float64 if k in ('thick', 'far', 'lo', 'hi') else bool))
               for k in ('thick', 'valid', 'hit', 'excl', 'far', 'lo', 'hi', 'agree')}
        for g in range(len(cams)):
            sel = inds == g
            base = render_image(boxes[sel], cams[g], Hr, Wr, rs, fpp)
            for k, v in zip(('thick', 'valid', 'hit', 'excl', 'far'), base):
                out[k][sel] = v
            lo, hi, agree = base[0].copy(), base[0].copy(), np.ones_like(base[1])
            for du, dv in ((DELTA, 0), (-DELTA, 0), (0, DELTA), (0, -DELTA)):
                th, va = render_image(boxes[sel], cams[g], Hr, Wr, rs, fpp, du, dv)[:2]
                lo, hi, agree = np.minimum(lo, th), np.maximum(hi, th), agree & (va == base[1])
            out['lo'][sel], out['hi'][sel], out['agree'][sel] = lo, hi, agree
        out = {k: v.reshape(len(boxes), Hr, Wr) for k, v in out.items()}
        out.update(boxes=boxes, inds=inds, cams=cams, Hr=Hr, Wr=Wr)
        _oracle_cache[key] = out
    return _oracle_cache[key]


# ---- the fp64 restatement of the resampling and the sums ---------------------------------------------------------------------------------
def bilinear64(img, gx, gy):
    """grid_sample(bilinear, zeros, align_corners=False) of img (Hr, Wr) at unnormalised coordinates; a non-finite coordinate gives 0"""
    Hr, Wr = img.shape
    ok = np.isfinite(gx) & np.isfinite(gy)
    gx, gy = np.where(ok, gx, -10.0), np.where(ok, gy, -10.0)
    x0, y0 = np.floor(gx), np.floor(gy)
    out = np.zeros_like(gx)
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            wgt = (1 - np.abs(gx - (x0 + dx))) * (1 - np.abs(gy - (y0 + dy)))
            inb = (xi >= 0) & (xi < Wr) & (yi >= 0) & (yi < Hr)
            out += np.where(inb, wgt * img[np.clip(yi, 0, Hr - 1), np.clip(xi, 0, Wr - 1)], 0.0)
    return out


def centers64(o, x2d, mask, os_, rs, get_bbox, boxes_in, min_box):
    """-> centres (B, 2), boxes (B, 4), valid (B,), margin: the smallest |resampled valid value - 0.5| (what the boxes hang on)"""
    B = len(o['boxes'])
    h, w = x2d.shape[2:]
    centres, boxes, valid, margin = np.zeros((B, 2)), np.zeros((B, 4)), np.zeros(B, dtype=bool), np.inf
    px, py = np.meshgrid(np.arange(w) * os_ + os_ / 2.0, np.arange(h) * os_ + os_ / 2.0)
    for b in range(B):
        g = o['inds'][b]
        gx, gy = (x2d[g, 0].astype(np.float64) + 0.5) / rs - 0.5, (x2d[g, 1].astype(np.float64) + 0.5) / rs - 0.5
        m = mask[g, 0].astype(np.float64)
        t = bilinear64(o['thick'][b], gx, gy) * m
        vm = bilinear64(o['valid'][b].astype(np.float64), gx, gy) * m
        W = t.sum()
        if W != 0:
            centres[b] = (t * px).sum() / W, (t * py).sum() / W
        if get_bbox:
            margin = min(margin, np.abs(vm - 0.5).min())
            on = vm >= 0.5
            if on.any():
                ys, xs = np.nonzero(on)
                boxes[b] = xs.min() * os_, ys.min() * os_, xs.max() * os_ + os_, ys.max() * os_ + os_
            else:
                boxes[b] = w * os_, h * os_, os_, os_
        else:
            boxes[b] = boxes_in[b]
        valid[b] = W >= 1e-6 and (boxes[b, 2] - boxes[b, 0]) >= min_box and (boxes[b, 3] - boxes[b, 1]) >= min_box
    return centres, boxes, valid, margin


def x2d_maps(kind, G, h, w, os_):
    """(x2d (G, 2, h, w), mask (G, 1, h, w)) fp32: the average-pooled pixel grid of the augmented image, in original-image pixels"""
    j, i = np.meshgrid(np.arange(w) * os_ + (os_ - 1) / 2.0, np.arange(h) * os_ + (os_ - 1) / 2.0)
    x, y, m = j.copy(), i.copy(), np.ones((h, w))
    if kind == 'flip':
        x = (w * os_ - 1) - x
    elif kind == 'shift':                        # a fraction of a pixel: bilinear weights that are neither 0, 1 nor 0.5
        x, y = x + 0.3, y + 0.6
    elif kind in ('crop', 'fraction', 'nan'):    # scaled and cropped, with a padded border
        x, y = 0.8 * x + 11.27, 0.8 * y + 6.41
        m[:, -5:] = 0.0
        m[-3:, :] = 0.0
        x[:, -5:], y[:, -5:], x[-3:, :], y[-3:, :] = 0.0, 0.0, 0.0, 0.0
        if kind == 'fraction':
            m[:, -7:-5] = 0.6
            m[-5:-3, :] *= 0.25
        if kind == 'nan':
            x[3, 4:9], y[10, 20:23], x[11, 17] = np.nan, np.nan, np.inf
    x2d = np.stack((x, y))[None].repeat(G, 0).astype(np.float32)
    return x2d, m[None, None].repeat(G, 0).astype(np.float32)


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
GEOMETRY = [('main', (96, 160), 4, 4, 16), ('main', (94, 158), 4, 4, 16), ('main', (96, 160), 4, 2, 16), ('main', (96, 160), 4, 4, None),
            ('row', (96, 160), 4, 4, 4), ('row', (96, 160), 4, 4, 16), ('row', (96, 160), 4, 4, 5)]


def check_scene(o):
    """conditions on the scene, from the oracle alone"""
    hits = o['hit'].sum()
    assert hits > 200
    assert o['excl'].sum() <= 0.02 * hits, (o['excl'].sum(), hits)
    assert (o['agree'] | o['excl']).all(), 'a pixel centre lies within DELTA of a silhouette: choose another scene'


@pytest.mark.parametrize('name,max_shape,os_,rs,fpp', GEOMETRY)
def test_thickness_against_rasteriser(backend, poisoned_empty, name, max_shape, os_, rs, fpp):
    o = oracle(name, max_shape, os_, rs, fpp)
    check_scene(o)
    thick, valid = _mod().box_thickness(dev(o['boxes'], backend), dev(o['inds'], backend), dev(o['cams'], backend), max_shape,
                                        output_stride=os_, render_stride=rs, faces_per_pixel=fpp)
    assert thick.shape == (len(o['boxes']), o['Hr'], o['Wr']) and valid.dtype == torch.bool
    thick, valid = thick.cpu().numpy().astype(np.float64), valid.cpu().numpy()
    keep = ~o['excl']
    assert np.isfinite(thick).all()
    assert (valid == o['valid'])[keep].all(), np.argwhere((valid != o['valid']) & keep)[:5]
    assert (thick[~valid] == 0).all()
    sel = keep & o['valid']
    out = np.maximum(np.maximum(o['lo'] - thick, thick - o['hi']), 0.0)[sel] / o['far'][sel]
    worst = out.max() if out.size else 0.0
    print(f'thickness worst {worst:.3e} over {sel.sum()} valid pixels ({o["excl"].sum()} excluded)')
    assert worst <= THICK_BAR
    if name == 'row':        # the scene does what it is for: the last box loses pixels under 4 and 5, keeps them under 16
        lost = o['hit'][2] & ~o['valid'][2]
        assert (lost.sum() > 20) == (fpp in (4, 5)) and o['valid'][2].sum() > 20
    else:
        assert o['valid'][[0, 1, 2, 3, 8]].sum(axis=(1, 2)).min() > 10      # also the box that straddles the near plane
        assert not o['valid'][[4, 5, 6]].any()                               # camera inside, behind the camera, off the canvas


E2E = [('main', (96, 160), 4, 4, 16, 'identity'), ('main', (96, 160), 4, 4, 16, 'flip'), ('main', (94, 158), 4, 4, 16, 'crop'),
       ('main', (96, 160), 4, 4, 16, 'fraction'), ('main', (96, 160), 4, 4, 16, 'nan'), ('main', (96, 160), 4, 2, 16, 'shift'),
       ('row', (96, 160), 4, 4, 4, 'identity'), ('row', (96, 160), 4, 4, 4, 'crop')]


def run_e2e(backend, o, max_shape, os_, rs, fpp, kind, get_bbox, min_box, boxes_in=None):
    h, w = int(math.ceil(max_shape[0] / os_)), int(math.ceil(max_shape[1] / os_))
    x2d, mask = x2d_maps(kind, len(o['cams']), h, w, os_)
    c, b, v = _mod().volume_centers(dev(o['boxes'], backend), dev(o['inds'], backend), dev(o['cams'], backend), dev(x2d, backend),
                                    dev(mask, backend), max_shape, bboxes_2d=None if boxes_in is None else dev(boxes_in, backend),
                                    output_stride=os_, render_stride=rs, faces_per_pixel=fpp, min_box_size=min_box, get_bbox_2d=get_bbox)
    return (x2d, mask), (c, b, v)


@pytest.mark.parametrize('get_bbox', [False, True])
@pytest.mark.parametrize('name,max_shape,os_,rs,fpp,kind', E2E)
def test_centers_against_restatement(backend, poisoned_empty, name, max_shape, os_, rs, fpp, kind, get_bbox):
    o = oracle(name, max_shape, os_, rs, fpp)
    check_scene(o)
    B = len(o['boxes'])
    boxes_in = None
    if not get_bbox:
        boxes_in = np.tile(np.array([10.0, 12.0, 50.0, 40.0], dtype=np.float32), (B, 1))
        boxes_in[0] = [10.0, 12.0, 13.0, 40.0]                 # 3 px wide: min_box_size = 4 rejects it
    min_box = 9.0 if get_bbox else 4.0                       # rendered boxes are whole cells: 9 px rejects one and two cells
    (x2d, mask), (c, b, v) = run_e2e(backend, o, max_shape, os_, rs, fpp, kind, get_bbox, min_box, boxes_in)
    c64, b64, v64, margin = centers64(o, x2d, mask, os_, rs, get_bbox, boxes_in, min_box)
    assert margin >= 1e-3, margin
    assert c.shape == (B, 2) and b.shape == (B, 4) and v.shape == (B,) and v.dtype == torch.bool
    c, b, v = c.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64), v.cpu().numpy()
    assert (v == v64).all(), (v, v64)
    assert (b == b64).all(), (b, b64)
    worst = np.abs(c - c64).max()
    print(f'centre worst {worst:.3e} px')
    assert np.isfinite(c).all() and worst <= CENTER_BAR
    if name == 'main':
        assert v64.sum() >= 3 and not v64[[4, 5, 6]].any() and (c64[[4, 5, 6]] == 0).all()
        assert not v64[0] if not get_bbox else not v64[7]      # min_box_size rejects one object either way
        if get_bbox and kind == 'identity':
            assert not v64[7] and (b64[7, 2:] - b64[7, :2]).min() < 9 and v64[0]


def test_convention_symmetric_box(backend):
    """a box on the optical axis under the identity map: the centre is (cx + 0.5, cy + 0.5) -- pins the pixel-centre convention"""
    boxes = np.array([[3.4, 1.6, 2.0, 0.0, 0.0, 10.0, 0.0]], dtype=np.float32)
    cams = cam(100.0, 100.0, 79.5, 47.5)[None]
    x2d, mask = x2d_maps('identity', 1, 24, 40, 4)
    inds = np.zeros(1, dtype=np.int64)
    c, b, v = _mod().volume_centers(dev(boxes, backend), dev(inds, backend), dev(cams, backend), dev(x2d, backend), dev(mask, backend),
                                    (96, 160), get_bbox_2d=True)
    o = dict(boxes=boxes, inds=inds, cams=cams)
    o['thick'], o['valid'] = [a.reshape(1, 24, 40) for a in render_image(boxes, cams[0], 24, 40, 4, 16)[:2]]
    c64 = centers64(o, x2d, mask, 4, 4, True, None, 4.0)[0]
    assert np.abs(c64[0] - [80.0, 48.0]).max() < 1e-9
    worst = np.abs(c.cpu().numpy().astype(np.float64)[0] - [80.0, 48.0]).max()
    print(f'centre worst {worst:.3e} px')
    assert worst <= CENTER_BAR and bool(v[0])
    assert b.cpu().numpy()[0].tolist() == [60.0, 40.0, 100.0, 56.0]      # the front face: +-18.9 px by +-8.9 px about the centre


def test_bars_under_caps():
    assert 0 < CENTER_BAR <= CENTER_CAP and 0 <= THICK_BAR <= THICK_CAP


def test_two_launches_same_bits(backend):
    o = oracle('main', (96, 160), 4, 4, 16)
    first = run_e2e(backend, o, (96, 160), 4, 4, 16, 'crop', True, 4.0)[1]
    second = run_e2e(backend, o, (96, 160), 4, 4, 16, 'crop', True, 4.0)[1]
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))


def test_no_objects(backend, poisoned_empty):
    x2d, mask = x2d_maps('identity', 2, 24, 40, 4)
    cams = np.stack([cam(100.0, 100.0, 80.0, 48.0)] * 2)
    c, b, v = _mod().volume_centers(torch.zeros((0, 7), device=backend), torch.zeros((0,), dtype=torch.int64, device=backend),
                                    dev(cams, backend), dev(x2d, backend), dev(mask, backend), (96, 160), get_bbox_2d=True)
    assert c.shape == (0, 2) and b.shape == (0, 4) and v.shape == (0,) and v.dtype == torch.bool
    t, tv = _mod().box_thickness(torch.zeros((0, 7), device=backend), torch.zeros((0,), dtype=torch.int64, device=backend),
                                 dev(cams, backend), (96, 160))
    assert t.shape == (0, 24, 40) and tv.shape == (0, 24, 40)


@pytest.mark.parametrize('what', ['box', 'intrinsics'])
def test_non_finite_gives_invalid(backend, poisoned_empty, what):
    o = oracle('main', (96, 160), 4, 4, 16)
    boxes, cams = o['boxes'].copy(), o['cams'].copy()
    if what == 'box':
        boxes[1, 5], boxes[8, 0] = np.nan, np.inf
        bad = [1, 8]
    else:
        cams[2, 0, 0] = np.nan
        bad = [4, 5, 6, 7, 8]
    x2d, mask = x2d_maps('identity', 3, 24, 40, 4)
    c, b, v = _mod().volume_centers(dev(boxes, backend), dev(o['inds'], backend), dev(cams, backend), dev(x2d, backend),
                                    dev(mask, backend), (96, 160), get_bbox_2d=True)
    c, v = c.cpu().numpy(), v.cpu().numpy()
    assert not v[bad].any() and (c[bad] == 0).all() and np.isfinite(c).all() and np.isfinite(b.cpu().numpy()).all()
    good = [k for k in (0, 2) if k not in bad]
    c0 = run_e2e(backend, o, (96, 160), 4, 4, 16, 'identity', True, 4.0)[1][0].cpu().numpy()
    assert v[good].all() and (c[good] == c0[good]).all()      # the others are what they are without the bad rows


@pytest.mark.gpu
def test_graph_capture_replays_bit_for_bit():
    backend = torch.device('cuda:0')
    import install as emu
    emu.uninstall()
    o = oracle('main', (96, 160), 4, 4, 16)
    x2d, mask = x2d_maps('crop', 3, 24, 40, 4)
    args = [dev(o['boxes'], backend), dev(o['inds'], backend), dev(o['cams'], backend), dev(x2d, backend), dev(mask, backend)]
    eager = _mod().volume_centers(*args, (96, 160), get_bbox_2d=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _mod().volume_centers(*args, (96, 160), get_bbox_2d=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _mod().volume_centers(*args, (96, 160), get_bbox_2d=True)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert bool(eager[2].any())
