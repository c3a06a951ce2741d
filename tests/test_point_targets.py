"""epropnp.targets.point_targets (epropnp_point_targets) against an fp64 oracle written here: a plain double loop over points and
objects of the definition in include/epropnp_hip.h.

Scene: image 96 x 160, three levels with strides 8 / 16 / 32 -- 12 x 20, 6 x 10 and 3 x 5 points, 315 in all, so 256-lane tiles
straddle both level boundaries --, regress ranges ((-1, 24), (24, 48), (48, 1e8)), 3 images, the middle one without objects, 9 objects
with boxes and centres on multiples of 0.25 px: every difference and every threshold comparison is exact in fp32, so the inside /
in-range masks must agree exactly.  Planted (asserted from the oracle alone in test_scenes_hold_their_cases): a point exactly on a
centre box's edge (not inside); a max regress distance exactly on lo and one exactly on hi (both in range); two objects mirrored about
a point column (an exact tie: the lower index wins); an object with a NaN centre; an object no point is assigned to.  Second case
'chunk': one image with POINT_TARGET_CHUNK + 2 objects (and a second image with 3) on the same points, a mirrored pair split over the two
staged chunks.

labels, gt_inds and num_fg must agree exactly on every decided point.  A point is undecided only if, in fp64, its two smallest finite
distances belong to different objects and differ by less than 1e-6 relative, but by more than 0; at most 1 % of a case's points may be
(asserted from the oracle alone; with quarter-pixel inputs there are none).

Bar: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over the cases of this file (each case prints its
worst error); test_bars_under_caps holds it under the cap.
    centerness  |centerness - centerness64|, values in [0, 1]   emulation 5.478e-8, MI355X 5.478e-8   -> bar 2.191e-7, cap 1e-5
                (both read off the printed output of their runs, which agree to the printed digits in every case)
"""
import numpy as np
import pytest
import torch

CENTERNESS_BAR = 2.191e-7      # absolute; cap 1e-5
CENTERNESS_CAP = 1e-5
INF = 1e8
STRIDES = (8, 16, 32)
RANGES = ((-1, 24), (24, 48), (48, 1e8))
SHAPE = (96, 160)
NUM_CLASSES = 3
RADIUS, ALPHA = 1.5, 2.5


def _mod():
    from epropnp import targets
    return targets


def dev(x, backend):
    return torch.from_numpy(np.ascontiguousarray(x)).to(backend)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- scenes (built once, never modified) -----------------------------------------------------------------------------------------------
def level_points():
    """per level (h * w, 2) float32 (x, y) = index * stride + stride // 2, row-major"""
    out = []
    for s in STRIDES:
        h, w = SHAPE[0] // s, SHAPE[1] // s
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        out.append(np.stack((xs.reshape(-1) * s + s // 2, ys.reshape(-1) * s + s // 2), axis=-1).astype(np.float32))
    return out


def scene_main():
    """(boxes (9, 4), centres (9, 2), labels (9,), image of each object); image 1 has no objects"""
    nan = np.nan
    rows = [
        # image 0
        (20, 16, 44, 40, 32, 28, 0),                # centre box of level 0 is 20 .. 44: the points of column x = 20 lie on its edge
        (16, 30, 50, 52, 33, 41, 1),                # level-1 point (40, 40): max regress distance 24 = lo of level 1
        (12, 20, 48, 50, 30.25, 35.5, 2),           # level-0 point (36, 36): max regress distance 24 = hi of level 0
        (8, 30, 70, 60, 44.75, 45.25, 1),           # level-1 point (56, 40): max regress distance 48 = hi of level 1
        (100, 10, 150, 60, nan, 40, 0),             # NaN centre: never wins
        # image 2
        (86, 50, 108, 72, 96.5, 60.25, 2),          # mirrored about the level-0 column x = 100 ...
        (92, 50, 114, 72, 103.5, 60.25, 0),         # ... with this one: equal distances on that column, the lower index wins
        (290, 290, 330, 330, 310, 310, 1),          # off the canvas: no point is assigned to it
        (10, 5, 150, 90, 80.25, 47.75, 2),          # large: the level-2 points
    ]
    a = np.array(rows, dtype=np.float64)
    return a[:, :4].astype(np.float32), a[:, 4:6].astype(np.float32), a[:, 6].astype(np.int64), np.array([0, 0, 0, 0, 0, 2, 2, 2, 2])


def scene_chunk():
    """image 0: chunk + 2 objects, the mirrored pair of scene_main at indices 10 and chunk + 1; image 1: 3 objects"""
    n0 = _mod().POINT_TARGET_CHUNK + 2
    rng = np.random.RandomState(5)
    n = n0 + 3
    c = np.stack((rng.randint(0, 4 * SHAPE[1], n), rng.randint(0, 4 * SHAPE[0], n)), axis=-1) / 4.0
    half = rng.randint(16, 200, (n, 4)) / 4.0
    boxes = np.concatenate((c - half[:, :2], c + half[:, 2:]), axis=1)
    main = scene_main()
    for at, src in ((10, 5), (n0 - 1, 6)):
        boxes[at], c[at] = main[0][src], main[1][src]
    labels = rng.randint(0, NUM_CLASSES, n).astype(np.int64)
    return boxes.astype(np.float32), c.astype(np.float32), labels, np.array([0] * n0 + [1] * 3)


SCENES = {'main': (scene_main, 3), 'chunk': (scene_chunk, 2)}
_CACHE = {}


def oracle(name):
    """The definition in fp64, a double loop: per (image, flat point) label, centerness, local winner and whether the point is
    decided; plus how often each planted comparison is met with equality.  Computed once per scene."""
    if name in _CACHE:
        return _CACHE[name]
    make, num_img = SCENES[name]
    boxes, centres, labels, img = make()
    pts = level_points()
    counts = [len(p) for p in pts]
    flat = np.concatenate(pts).astype(np.float64)
    lvl = np.repeat(np.arange(len(pts)), counts)
    P = len(flat)
    lab = np.zeros((num_img, P), dtype=np.int64)
    cen = np.zeros((num_img, P))
    win = np.zeros((num_img, P), dtype=np.int64)
    decided = np.ones((num_img, P), dtype=bool)
    met = {'edge': 0, 'lo': 0, 'hi': 0, 'tie': 0}
    b64, c64 = boxes.astype(np.float64), centres.astype(np.float64)
    for i in range(num_img):
        objs = np.nonzero(img == i)[0]
        for p in range(P):
            x, y = flat[p]
            s = STRIDES[lvl[p]] * RADIUS
            lo, hi = RANGES[lvl[p]]
            best, best_j, dists = INF, 0, []
            for k, j in enumerate(objs):
                cx, cy = c64[j]
                x1, y1, x2, y2 = b64[j]
                with np.errstate(invalid='ignore'):
                    in_min = min(x - (cx - s), y - (cy - s), (cx + s) - x, (cy + s) - y) if not np.isnan(c64[j]).any() else np.nan
                    reg_max = max(x - x1, y - y1, x2 - x, y2 - y)
                    inside, in_range = bool(in_min > 0), bool(lo <= reg_max <= hi)
                met['edge'] += int(in_min == 0 and in_range)
                met['lo'] += int(inside and reg_max == lo)
                met['hi'] += int(inside and reg_max == hi)
                d = float(np.sqrt((x - cx) ** 2 + (y - cy) ** 2)) if inside and in_range else INF
                if d < INF:
                    dists.append((d, k))
                if d < best:
                    best, best_j = d, k
            dists.sort()
            if len(dists) > 1 and dists[0][1] != dists[1][1]:
                gap = dists[1][0] - dists[0][0]
                met['tie'] += int(gap == 0)
                if 0 < gap < 1e-6 * dists[1][0]:
                    decided[i, p] = False
            win[i, p] = best_j
            if len(objs):
                lab[i, p] = labels[objs[best_j]] if best < INF else NUM_CLASSES
                cen[i, p] = np.exp(-ALPHA * (best / (float(np.float32(1.414)) * s)))
            else:
                lab[i, p] = NUM_CLASSES
    base = np.array([(img < i).sum() for i in range(num_img)], dtype=np.int64)
    # the flattened order: level-major, then image, then the point within the level
    order = [(i, p) for k in range(len(pts)) for i in range(num_img) for p in np.nonzero(lvl == k)[0]]
    ii, pp = np.array([o[0] for o in order]), np.array([o[1] for o in order])
    out = dict(labels=lab[ii, pp], centerness=cen[ii, pp], gt_inds=(win + base[:, None])[ii, pp], decided=decided[ii, pp],
               strides=np.array(STRIDES, dtype=np.int64)[lvl[pp]], met=met, local=win, raw_labels=lab,
               inputs=(np.concatenate(pts), counts, boxes, labels, centres, img, num_img))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[name] = out
    return out


def run(name, backend, with_strides=False):
    pts, counts, boxes, labels, centres, img, num_img = oracle(name)['inputs']
    return _mod().point_targets(dev(pts, backend), counts, STRIDES, RANGES, dev(boxes, backend), dev(labels, backend),
                                dev(centres, backend), dev(img, backend), num_img, NUM_CLASSES, center_sample_radius=RADIUS,
                                centerness_alpha=ALPHA, with_strides=with_strides)


# ---- the oracle alone --------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_their_cases():
    for name in SCENES:
        o = oracle(name)
        undecided = int((~o['decided']).sum())
        assert undecided <= 0.01 * o['decided'].size, (name, undecided)
        assert undecided == 0, 'quarter-pixel inputs: every distance gap is either 0 or far above 1e-6 relative'
    o = oracle('main')
    assert o['met']['edge'] >= 1 and o['met']['lo'] >= 1 and o['met']['hi'] >= 1 and o['met']['tie'] >= 1, o['met']
    assert sum(len(p) for p in level_points()) == 315
    fg = o['raw_labels'] < NUM_CLASSES
    assert not fg[1].any() and fg[0].any() and fg[2].any()
    won = {int(j) for i in (0, 2) for j in (o['local'][i][fg[i]] + (0 if i == 0 else 5))}
    assert 4 not in won and 7 not in won, 'the NaN-centre object and the one off the canvas own no point'
    assert {0, 1, 2, 3, 5, 6, 8} <= won, won
    # the column the pair is mirrored about goes to the lower index where both qualify
    pts = np.concatenate(level_points())
    col = np.nonzero((pts[:, 0] == 100) & (pts[:, 1] == 60))[0]
    assert len(col) == 1 and o['local'][2][col[0]] == 0 and fg[2][col[0]]
    o = oracle('chunk')
    n0 = _mod().POINT_TARGET_CHUNK + 2
    assert o['met']['tie'] >= 1 and o['local'][0][col[0]] == 10
    assert (o['local'][0][o['raw_labels'][0] < NUM_CLASSES] >= _mod().POINT_TARGET_CHUNK).any(), 'a winner from the second chunk'
    assert (np.asarray(o['inputs'][5]) == 0).sum() == n0


def test_bars_under_caps():
    assert 0 < CENTERNESS_BAR <= CENTERNESS_CAP


# ---- against the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SCENES))
def test_point_targets_match_fp64(backend, poisoned_empty, name):
    o = oracle(name)
    labels, cen, gt_inds, strides, num_fg = run(name, backend, with_strides=True)
    assert labels.dtype == torch.int64 and gt_inds.dtype == torch.int64 and strides.dtype == torch.int64
    assert cen.dtype == torch.float32 and num_fg.dtype == torch.int32 and tuple(num_fg.shape) == (1,)
    ok = o['decided']
    labels, cen, gt_inds, strides = (t.cpu().numpy() for t in (labels, cen, gt_inds, strides))
    assert labels.shape == o['labels'].shape
    assert np.array_equal(labels[ok], o['labels'][ok])
    assert np.array_equal(gt_inds[ok], o['gt_inds'][ok])
    assert int(num_fg.item()) == int((o['labels'] < NUM_CLASSES).sum()) > 0
    assert np.array_equal(strides, o['strides'])
    assert np.isfinite(cen).all()                     # the poison is gone
    worst = float(np.abs(cen.astype(np.float64) - o['centerness'])[ok].max())
    print(f'point_targets[{name}] on {backend}: worst centerness error {worst:.3e} (bar {CENTERNESS_BAR:.3e})')
    assert worst <= CENTERNESS_BAR
    assert (cen[o['labels'] == NUM_CLASSES] == 0).all()


def test_without_strides_and_bit_reproducible(backend):
    first = run('main', backend)
    assert first[3] is None
    again = run('main', backend, with_strides=True)
    for a, b in zip(first[:3] + first[4:], again[:3] + again[4:]):
        assert torch.equal(bits(a), bits(b))


def test_empty_sides(backend):
    m = _mod()
    pts, counts, boxes, labels, centres, img, num_img = oracle('main')['inputs']
    args = lambda p, c, b, l, ce, im, n: m.point_targets(dev(p, backend), c, STRIDES, RANGES, dev(b, backend), dev(l, backend),       # noqa: E731,E741
                                                         dev(ce, backend), dev(im, backend), n, NUM_CLASSES, with_strides=True)
    # no points
    out = args(pts[:0], [0, 0, 0], boxes, labels, centres, img, num_img)
    assert all(t.numel() == 0 for t in out[:4]) and int(out[4].item()) == 0
    # no images (and then no objects)
    out = args(pts, counts, boxes[:0], labels[:0], centres[:0], img[:0], 0)
    assert all(t.numel() == 0 for t in out[:4]) and int(out[4].item()) == 0
    # no objects: all background, winner 0, centerness 0
    lab, cen, gt, st, nfg = args(pts, counts, boxes[:0], labels[:0], centres[:0], img[:0], 2)
    assert lab.numel() == 2 * len(pts) and bool((lab == NUM_CLASSES).all()) and bool((cen == 0).all()) and bool((gt == 0).all())
    assert int(nfg.item()) == 0 and np.array_equal(st.cpu().numpy()[:2 * counts[0]], np.full(2 * counts[0], STRIDES[0]))


def test_bad_arguments_are_named(backend):
    m = _mod()
    pts, counts, boxes, labels, centres, img, num_img = oracle('main')['inputs']
    good = dict(points=dev(pts, backend), num_points_per_lvl=counts, strides=STRIDES, regress_ranges=RANGES, gt_bboxes=dev(boxes, backend),
                gt_labels=dev(labels, backend), centers2d=dev(centres, backend), obj_img_inds=dev(img, backend), num_img=num_img,
                num_classes=NUM_CLASSES)
    bad = [('points', good['points'].double()), ('points', good['points'][:, :1]), ('gt_bboxes', good['gt_bboxes'].double()),
           ('gt_bboxes', good['gt_bboxes'][:, :3]), ('centers2d', good['centers2d'][:-1]), ('centers2d', good['centers2d'].half()),
           ('gt_labels', good['gt_labels'].int()), ('gt_labels', good['gt_labels'][:-1]), ('obj_img_inds', good['obj_img_inds'][:-1]),
           ('obj_img_inds', good['obj_img_inds'].float()), ('num_points_per_lvl', [counts[0], counts[1], counts[2] + 1]),
           ('num_points_per_lvl', [1] * 9), ('strides', STRIDES[:2]), ('regress_ranges', RANGES[:2])]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            m.point_targets(**dict(good, **{name: value}))
    with pytest.raises(RuntimeError, match='radius_px'):
        m.point_targets(**dict(good, strides=(8, 0, 32)))
    other = torch.device('cuda:0') if backend.type == 'cpu' else torch.device('cpu')
    if other.type == 'cpu' or torch.cuda.is_available():
        for name in ('points', 'gt_bboxes', 'gt_labels', 'centers2d', 'obj_img_inds'):
            with pytest.raises(RuntimeError, match=name):
                m.point_targets(**dict(good, **{name: good[name].to(other)}))


@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_bits():
    """a call captured with torch.cuda.graph after a side-stream warm-up, replayed on changed objects: each replay equals the eager call"""
    import install as emu
    emu.uninstall()
    m = _mod()
    d = torch.device('cuda:0')
    pts, counts, boxes, labels, centres, img, num_img = oracle('main')['inputs']
    p, b, l, c, im = (dev(a, d) for a in (pts, boxes, labels, centres, img))      # noqa: E741

    def step():
        return m.point_targets(p, counts, STRIDES, RANGES, b, l, c, im, num_img, NUM_CLASSES, with_strides=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for shift in (0.0, 8.0):
        c.copy_(dev(centres + np.float32(shift), d))
        b.copy_(dev(boxes + np.float32(shift), d))
        graph.replay()
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        for a, e in zip(out, eager):
            assert torch.equal(bits(a), bits(e))
        assert int(out[4].item()) > 0
