"""epropnp.boxes.rotated_overlaps / box3d_overlaps / image_overlaps (epropnp_box_overlap, epropnp_box_overlap_segmented) against an fp64
oracle: the Sutherland-Hodgman clip of tests/test_boxes.py for the BEV intersection, with the height interval, the sizes and the four
criteria added here in fp64, all on the fp32 inputs.

Scenes are clusters of near-duplicate boxes (the recipe of tests/test_boxes.py::scene with TWO objects, so that a large share of the
pairs overlaps), with centre height and height jittered.  Shapes: pairwise (M,N) in {(1,1), (3,65), (65,3), (64,64), (130,70)}, aligned
N in {1, 65, 257}, segmented counts_a = [0, 3, 70, 1, 0, 64] / counts_b = [5, 0, 65, 1, 0, 130] (an empty side either way, ragged
multi-tile, a lone pair, both sides empty, a full tile); all three kinds and all four criteria at every shape, and for 3D boxes
z_axis in {1, 2} x z_center in {0.5, 1.0, 0.0} x both height rules at pairwise (130,70) and aligned 65.

Condition, asserted from the oracle before anything is compared: at least 20 % of a case's pairs have fp64 IoU > 0.05 and at least
10 % have IoU exactly 0 -- a kernel that writes zeros, or never writes zero, cannot pass.  It holds for every pairwise and segmented
case of ten pairs or more; the (1,1) case has ONE pair, which cannot be both, and is required to overlap (IoU > 0.05).

Bars: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over every case of this file; neither bar may
exceed 1e-5, the cap of tests/test_boxes.py (the height pass adds a handful of fp32 roundings to a routine measured at 2.5e-7 / 1.7e-7).
    ratio   |ratio - ratio64| (iou, a, b)                     emulation 3.974e-7, MI355X 3.974e-7   -> bar 1.590e-6
    inter   |inter - inter64| / max(size_a, size_b)           emulation 2.691e-7, MI355X 2.691e-7   -> bar 1.076e-6
"""
import math

import numpy as np
import pytest
import torch

import test_boxes as tb

RATIO_BAR = 1.590e-6     # |ratio - ratio64|; cap 1e-5
INTER_BAR = 1.076e-6     # |inter - inter64| / max(size_a, size_b); cap 1e-5
CAP = 1e-5
KINDS = ('bev', 'box3d', 'image')
CRITERIA = ('iou', 'a', 'b', 'inter')
PAIR_SHAPES = [(1, 1), (3, 65), (65, 3), (64, 64), (130, 70)]
COUNTS_A, COUNTS_B = [0, 3, 70, 1, 0, 64], [5, 0, 65, 1, 0, 130]
_worst = {'ratio': 0.0, 'inter': 0.0}


def _mod():
    from epropnp import boxes
    return boxes


def _bits(t):
    return t.contiguous().view(torch.int32)


def dev(x, backend):
    return torch.from_numpy(np.ascontiguousarray(x)).to(backend)


# ---- scenes (CPU, built once per key, never modified) --------------------------------------------------------------------------------
_scenes = {}


def scene7(N, seed, n_obj=2):
    """N fp32 3D boxes [x, y, z, l, h, w, ry] (z_axis = 1): n_obj objects, each box an object's box with the jitter of
    tests/test_boxes.py::scene in the (x, z) plane, centre height 1 + N(0, 0.15), height 1.6 U(0.85, 1.15)"""
    key = (N, seed, n_obj)
    if key not in _scenes:
        rng = np.random.default_rng(seed)
        centre = rng.uniform([-40.0, 3.0], [40.0, 70.0], (n_obj, 2))
        size = tb.SIZES[rng.integers(0, len(tb.SIZES), n_obj)]
        yaw = rng.uniform(-math.pi, math.pi, n_obj)
        which = rng.integers(0, n_obj, N)
        c = centre[which] + rng.normal(0.0, 1.0, (N, 2)) * (0.35 * size[which].min(1))[:, None]
        wh = size[which] * rng.uniform(0.85, 1.15, (N, 2))
        a = yaw[which] + rng.normal(0.0, 0.15, N) + math.pi * rng.integers(0, 2, N)
        y = 1.0 + rng.normal(0.0, 0.15, N)
        h = 1.6 * rng.uniform(0.85, 1.15, N)
        _scenes[key] = np.stack((c[:, 0], y, c[:, 1], wh[:, 0], h, wh[:, 1], a), 1).astype(np.float32)
    return _scenes[key]


def as_kind(b7, kind, z_axis=1):
    """the scene's boxes as rows of `kind`: bev (cx, cy, dx, dy, angle); box3d with the height on z_axis; image (x1, y1, x2, y2) of the
    unrotated BEV rectangle"""
    if kind == 'bev':
        return np.ascontiguousarray(b7[:, [0, 2, 3, 5, 6]])
    if kind == 'image':
        return np.stack((b7[:, 0] - b7[:, 3] / 2, b7[:, 2] - b7[:, 5] / 2, b7[:, 0] + b7[:, 3] / 2, b7[:, 2] + b7[:, 5] / 2), 1).astype(np.float32)
    order = {0: [1, 0, 2, 4, 3, 5, 6], 1: [0, 1, 2, 3, 4, 5, 6], 2: [0, 2, 1, 3, 5, 4, 6]}[z_axis]
    return np.ascontiguousarray(b7[:, order])


# ---- the fp64 oracle -----------------------------------------------------------------------------------------------------------------
def bev_axes(z_axis):
    axes = list(range(7))
    axes.pop(z_axis + 3)
    axes.pop(z_axis)
    return axes


def valid64(kind, x):
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x).all(1)
    with np.errstate(invalid='ignore'):
        if kind == 'image':
            return fin & (x[:, 2] >= x[:, 0]) & (x[:, 3] >= x[:, 1])
        if kind == 'bev':
            return fin & (x[:, 2] >= 0) & (x[:, 3] >= 0)
        return fin & (x[:, 3:6] >= 0).all(1)


def oracle(kind, a, b, aligned=False, z_axis=1, z_center=0.5, rule='interval'):
    """fp64 (inter, size_a, size_b, ok) of fp32 boxes a (M,w), b (N,w): (M,N), or (N,) aligned"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    va, vb = valid64(kind, a), valid64(kind, b)
    a, b = np.where(va[:, None], a, 0.0), np.where(vb[:, None], b, 0.0)

    def pair(x, y):
        return (x, y) if aligned else (x[:, None], y[None, :])
    if kind == 'image':
        (ax1, bx1), (ay1, by1), (ax2, bx2), (ay2, by2) = (pair(a[:, k], b[:, k]) for k in range(4))
        iw, ih = np.minimum(ax2, bx2) - np.maximum(ax1, bx1), np.minimum(ay2, by2) - np.maximum(ay1, by1)
        inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
        sa, sb = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    elif kind == 'bev':
        inter = np.nan_to_num(tb.oracle(a, b, aligned)[0])
        sa, sb = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    else:
        ax = bev_axes(z_axis)
        inter = np.nan_to_num(tb.oracle(a[:, ax], b[:, ax], aligned)[0])
        lo_a, lo_b = pair(a[:, z_axis] - a[:, z_axis + 3] * z_center, b[:, z_axis] - b[:, z_axis + 3] * z_center)
        hi_a, hi_b = pair(a[:, z_axis] + a[:, z_axis + 3] * (1 - z_center), b[:, z_axis] + b[:, z_axis + 3] * (1 - z_center))
        bottom = np.maximum(lo_a, lo_b) if rule == 'interval' else np.minimum(lo_a, lo_b)
        inter = inter * np.maximum(np.minimum(hi_a, hi_b) - bottom, 0.0)
        sa, sb = a[:, 3:6].prod(1), b[:, 3:6].prod(1)
    sa, sb = pair(sa, sb)
    va, vb = pair(va, vb)
    shape = inter.shape
    return inter, np.broadcast_to(sa, shape), np.broadcast_to(sb, shape), np.broadcast_to(va & vb, shape)


def value64(orc, criterion):
    inter, sa, sb, ok = orc
    if criterion == 'inter':
        v = inter
    else:
        den = {'iou': sa + sb - inter, 'a': sa, 'b': sb}[criterion]
        v = np.minimum(inter / np.maximum(den, 1e-8), 1.0)
    return np.where(ok, v, np.nan)


def check(got, orc, criterion, tag):
    """got fp32 tensor against the oracle: NaN exactly where a box is invalid, the rest within the bar; prints the figure"""
    want = value64(orc, criterion)
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{tag}: NaN not exactly where a box is invalid'
    assert np.isfinite(got[~nan]).all(), tag
    which = 'inter' if criterion == 'inter' else 'ratio'
    err = np.abs(got - want)
    if which == 'inter':
        s = np.maximum(orc[1], orc[2])
        err = err / np.where(np.isfinite(s) & (s > 0), s, 1.0)
    else:
        assert (got[~nan] <= 1.0).all() and (got[~nan] >= 0.0).all(), f'{tag}: a ratio outside [0, 1]'
    err = float(err[~nan].max(initial=0.0))
    _worst[which] = max(_worst[which], err)
    bar = INTER_BAR if which == 'inter' else RATIO_BAR
    print(f'{tag} {criterion}: worst {which} error {err:.3e} (bar {bar:.2e}); over the file so far {_worst[which]:.3e}')
    assert bar <= CAP and err <= bar, (tag, criterion, err)


def condition(orc, tag):
    """the case exercises the kernel: enough pairs that overlap, enough that do not"""
    iou = value64(orc, 'iou')
    n = iou.size
    over, zero = float((iou > 0.05).sum()) / n, float((iou == 0).sum()) / n
    print(f'{tag}: {n} pairs, {100 * over:.1f} % with IoU > 0.05, {100 * zero:.1f} % with IoU exactly 0')
    if n >= 10:
        assert over >= 0.2 and zero >= 0.1, f'{tag}: the scene does not exercise the kernel: choose another seed'
    else:
        assert over == 1.0, f'{tag}: the lone pair does not overlap: choose another seed'


def call(kind, a, b, criterion, **kw):
    m = _mod()
    if kind == 'bev':
        return m.rotated_overlaps(a, b, criterion, **kw)
    if kind == 'image':
        kw.pop('aligned', None)
        return m.image_overlaps(a, b, criterion, **kw)
    return m.box3d_overlaps(a, b, criterion, **kw)


# ---- cases, with their oracle (built once, never modified) ---------------------------------------------------------------------------
_cases = {}
PAIR_SEEDS = {(1, 1): 1, (3, 65): 1, (65, 3): 1, (64, 64): 1, (130, 70): 1}


def pair_case(M, N, kind, z_axis=1, z_center=0.5, rule='interval'):
    key = (M, N, kind, z_axis, z_center, rule)
    if key not in _cases:
        s = scene7(M + N, PAIR_SEEDS[(M, N)])
        a, b = as_kind(s[:M], kind, z_axis), as_kind(s[M:], kind, z_axis)
        _cases[key] = (a, b, oracle(kind, a, b, False, z_axis, z_center, rule))
    return _cases[key]


def aligned_case(N, kind, z_axis=1, z_center=0.5, rule='interval'):
    key = ('aligned', N, kind, z_axis, z_center, rule)
    if key not in _cases:
        s = scene7(2 * N, 40 + N)
        s7a, s7b = s[:N].copy(), s[N:].copy()
        s7b[::2] = s7a[::2] + np.float32(0.1)          # every second pair does overlap
        a, b = as_kind(s7a, kind, z_axis), as_kind(s7b, kind, z_axis)
        _cases[key] = (a, b, oracle(kind, a, b, True, z_axis, z_center, rule))
    return _cases[key]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,N', PAIR_SHAPES)
def test_pairwise_against_fp64(backend, poisoned_empty, M, N, kind):
    a, b, orc = pair_case(M, N, kind)
    condition(orc, f'pairwise {kind} {M}x{N}')
    da, db = dev(a, backend), dev(b, backend)
    for criterion in CRITERIA:
        got = call(kind, da, db, criterion)
        assert got.shape == (M, N) and got.dtype == torch.float32
        check(got, orc, criterion, f'pairwise {kind} {M}x{N}')
        assert torch.equal(_bits(call(kind, da, db, criterion)), _bits(got)), 'two launches differ'
    # the other way round: the same pairs, the other box's frame; 'a' and 'b' change places
    back = tuple(np.ascontiguousarray(x.T) for x in (orc[0], orc[2], orc[1], orc[3]))
    check(call(kind, db, da, 'a'), back, 'a', f'pairwise {kind} {N}x{M} (swapped)')


@pytest.mark.parametrize('rule', ['interval', 'reference_torch'])
@pytest.mark.parametrize('z_center', [0.5, 1.0, 0.0])
@pytest.mark.parametrize('z_axis', [1, 2])
def test_box3d_height_options_against_fp64(backend, poisoned_empty, z_axis, z_center, rule):
    """z_axis, z_center and both height rules at pairwise (130, 70) and aligned 65"""
    kw = dict(z_axis=z_axis, z_center=z_center, height_rule=rule)
    a, b, orc = pair_case(130, 70, 'box3d', z_axis, z_center, rule)
    condition(orc, f'pairwise box3d 130x70 z_axis={z_axis} z_center={z_center} {rule}')
    da, db = dev(a, backend), dev(b, backend)
    for criterion in CRITERIA:
        check(call('box3d', da, db, criterion, **kw), orc, criterion, f'pairwise box3d 130x70 z_axis={z_axis} z_center={z_center} {rule}')
    a, b, orc = aligned_case(65, 'box3d', z_axis, z_center, rule)
    da, db = dev(a, backend), dev(b, backend)
    for criterion in CRITERIA:
        got = call('box3d', da, db, criterion, aligned=True, **kw)
        check(got, orc, criterion, f'aligned box3d 65 z_axis={z_axis} z_center={z_center} {rule}')
        assert torch.equal(_bits(got), _bits(call('box3d', da, db, criterion, **kw).diagonal()))


def test_the_two_height_rules_differ(backend, poisoned_empty):
    """'reference_torch' is not 'interval': boxes at different heights get a taller intersection under it"""
    a, b, _ = pair_case(130, 70, 'box3d')
    da, db = dev(a, backend), dev(b, backend)
    x, y = call('box3d', da, db, 'inter'), call('box3d', da, db, 'inter', height_rule='reference_torch')
    assert bool((y >= x).all()) and bool((y > x * 1.01).any())


@pytest.mark.parametrize('kind', ['bev', 'box3d'])
@pytest.mark.parametrize('N', [1, 65, 257])
def test_aligned_is_the_diagonal(backend, poisoned_empty, N, kind):
    a, b, orc = aligned_case(N, kind)
    da, db = dev(a, backend), dev(b, backend)
    for criterion in CRITERIA:
        got = call(kind, da, db, criterion, aligned=True)
        assert got.shape == (N,)
        check(got, orc, criterion, f'aligned {kind} N={N}')
        assert torch.equal(_bits(got), _bits(call(kind, da, db, criterion).diagonal())), 'aligned differs from the diagonal of the pairwise call'
        assert torch.equal(_bits(got), _bits(call(kind, da, db, criterion, aligned=True))), 'two launches differ'


@pytest.mark.parametrize('kind', KINDS)
def test_segmented_blocks_are_the_pairwise_calls(backend, poisoned_empty, kind):
    M, N = sum(COUNTS_A), sum(COUNTS_B)
    s = scene7(M + N, 1)
    a, b = as_kind(s[:M], kind), as_kind(s[M:], kind)
    da, db = dev(a, backend), dev(b, backend)
    blocks, ra, rb = [], 0, 0
    for na, nb in zip(COUNTS_A, COUNTS_B):
        blocks.append((slice(ra, ra + na), slice(rb, rb + nb)))
        ra, rb = ra + na, rb + nb
    orcs = [oracle(kind, a[p], b[q]) for p, q in blocks]
    condition(tuple(np.concatenate([o[k].reshape(-1) for o in orcs]) for k in range(4)), f'segmented {kind}')
    for criterion in CRITERIA:
        flat, views = call(kind, da, db, criterion, counts=(COUNTS_A, COUNTS_B))
        assert flat.shape == (sum(x * y for x, y in zip(COUNTS_A, COUNTS_B)),) and flat.dtype == torch.float32 and len(views) == len(COUNTS_A)
        assert not bool(flat.isnan().any()), 'an output element was not written'
        for g, ((p, q), view, orc) in enumerate(zip(blocks, views, orcs)):
            assert view.shape == (COUNTS_A[g], COUNTS_B[g])
            if view.numel():
                assert view.data_ptr() == flat[sum(x * y for x, y in zip(COUNTS_A[:g], COUNTS_B[:g])):].data_ptr()
                check(view, orc, criterion, f'segmented {kind} block {g}')
                assert torch.equal(_bits(view), _bits(call(kind, da[p], db[q], criterion))), f'block {g} differs from the pairwise call'
        again, _ = call(kind, da, db, criterion, counts=(COUNTS_A, COUNTS_B))
        assert torch.equal(_bits(again), _bits(flat)), 'two launches differ'
    # numpy integers and no segment at all
    flat, views = call(kind, da[:3], db[:5], 'iou', counts=(np.array([3]), np.array([5])))
    assert torch.equal(_bits(views[0]), _bits(call(kind, da[:3], db[:5], 'iou')))
    flat, views = call(kind, da[:0], db[:0], 'iou', counts=([], []))
    assert flat.shape == (0,) and views == []
    flat, views = call(kind, da[:4], db[:0], 'iou', counts=([4, 0], [0, 0]))
    assert flat.shape == (0,) and [tuple(v.shape) for v in views] == [(4, 0), (0, 0)]


def test_rotated_overlaps_are_the_bits_of_bev_overlap_and_bev_iou(backend, poisoned_empty):
    m = _mod()
    a, b, _ = pair_case(130, 70, 'bev')
    da, db = dev(a, backend), dev(b, backend)
    assert torch.equal(_bits(m.rotated_overlaps(da, db, 'inter')), _bits(m.bev_overlap(da, db)))
    one = torch.ones((), device=backend)
    assert torch.equal(_bits(m.rotated_overlaps(da, db, 'iou')), _bits(torch.minimum(m.bev_iou(da, db), one)))
    assert torch.equal(_bits(m.rotated_overlaps(da[:70], db, 'inter', aligned=True)), _bits(m.bev_overlap(da[:70], db, aligned=True)))
    # a 3D box with the unit height interval [0, 1] against itself: the BEV numbers
    s = scene7(200, 1)
    b7 = s.copy()
    b7[:, 1], b7[:, 4] = 0.5, 1.0
    d7a, d7b = dev(b7[:130], backend), dev(b7[130:], backend)
    assert torch.equal(_bits(m.box3d_overlaps(d7a, d7b, 'inter')), _bits(m.bev_overlap(da, db)))


def test_exact_values(backend, poisoned_empty):
    m = _mod()
    box = (1.5, 1.0, 20.0, 4.0, 2.0, 1.8, 0.7)

    def moved(**kw):
        v = list(box)
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v
    a = np.array([box, box, box, box, moved(_4=0.0)], dtype=np.float32)
    b = np.array([moved(_1=3.0),            # the height intervals [0, 2] and [2, 4] only touch
                  moved(_0=101.5),          # 100 m apart in BEV
                  box,                      # itself
                  moved(_1=2.5),            # a quarter of the height in common
                  box], dtype=np.float32)   # a zero-height box against a real one
    da, db = dev(a, backend), dev(b, backend)
    orc = oracle('box3d', a, b, aligned=True)
    for aligned in (True, False):
        iou = m.box3d_overlaps(da, db, 'iou', aligned=aligned)
        vol = m.box3d_overlaps(da, db, 'inter', aligned=aligned)
        iou, vol = (iou, vol) if aligned else (iou.diagonal(), vol.diagonal())
        check(iou, orc, 'iou', 'exact values')
        check(vol, orc, 'inter', 'exact values')
        iou, vol = iou.cpu().tolist(), vol.cpu().tolist()
        print('  iou', iou, 'volume', vol)
        assert iou[0] == 0.0 and vol[0] == 0.0, 'touching height intervals'
        assert iou[1] == 0.0 and vol[1] == 0.0, 'apart in BEV'
        assert 1.0 - RATIO_BAR <= iou[2] <= 1.0, 'a box against itself'
        assert abs(iou[3] - (0.5 / 3.5)) <= RATIO_BAR
        assert iou[4] == 0.0 and vol[4] == 0.0, 'a zero-height box'
    # image boxes that share an edge, and one inside another
    ia = np.array([(0, 0, 4, 2), (0, 0, 4, 2), (1, 1, 2, 2)], dtype=np.float32)
    ib = np.array([(4, 0, 8, 2), (0, 0, 4, 2), (0, 0, 4, 4)], dtype=np.float32)
    got = m.image_overlaps(dev(ia, backend), dev(ib, backend), 'iou').diagonal().cpu().tolist()
    assert got == [0.0, 1.0, 0.0625]
    assert m.image_overlaps(dev(ia, backend), dev(ib, backend), 'a').diagonal().cpu().tolist() == [0.0, 1.0, 1.0]
    assert m.image_overlaps(dev(ia, backend), dev(ib, backend), 'b').diagonal().cpu().tolist() == [0.0, 1.0, 0.0625]


@pytest.mark.parametrize('kind', KINDS)
def test_nan_exactly_in_the_rows_and_columns_of_invalid_boxes(backend, poisoned_empty, kind):
    a, b, _ = pair_case(130, 70, kind)
    a, b = a.copy(), b.copy()
    size = {'bev': 2, 'box3d': 4, 'image': 2}[kind]         # a size column (image: x2, set below x1)
    a[3, 0] = np.nan                                        # a NaN coordinate
    a[64, size] = np.inf                                    # an inf size / corner
    a[129, size] = -1.0 if kind != 'image' else a[129, 0] - 1.0          # a negative size; x2 < x1
    b[0, -1] = np.nan
    b[65, 1] = -np.inf
    b[69, size + 1] = -0.5 if kind != 'image' else b[69, 1] - 0.5        # y2 < y1
    orc = oracle(kind, a, b)
    want = value64(orc, 'iou')
    assert np.isnan(want[[3, 64, 129]]).all() and np.isnan(want[:, [0, 65, 69]]).all() and np.isnan(want).sum() == 3 * 70 + 3 * 127
    da, db = dev(a, backend), dev(b, backend)
    for criterion in CRITERIA:
        check(call(kind, da, db, criterion), orc, criterion, f'invalid boxes {kind}')
    if kind != 'image':
        al = call(kind, da[:70], db, 'iou', aligned=True)
        assert torch.equal(al.isnan().cpu(), torch.from_numpy(np.isnan(np.diagonal(want[:70]))))
    flat, views = call(kind, da, db, 'iou', counts=([4, 126], [66, 4]))
    assert torch.equal(views[0].isnan().cpu(), torch.from_numpy(np.isnan(want[:4, :66])))
    assert torch.equal(views[1].isnan().cpu(), torch.from_numpy(np.isnan(want[4:, 66:])))


def test_python_errors(backend):
    m = _mod()
    s = scene7(65, 1)
    b7, b5, b4 = (dev(as_kind(s, k), backend) for k in ('box3d', 'bev', 'image'))
    for bad in (lambda: m.box3d_overlaps(b7.double(), b7), lambda: m.rotated_overlaps(b5, b5.half()), lambda: m.image_overlaps(b4.double(), b4)):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: m.box3d_overlaps(b5, b7), lambda: m.box3d_overlaps(b7, b7.reshape(-1)), lambda: m.rotated_overlaps(b7, b5),
                lambda: m.image_overlaps(b4, b5), lambda: m.rotated_overlaps(b5[:3], b5, aligned=True),
                lambda: m.box3d_overlaps(b7, b7[:64], aligned=True), lambda: m.box3d_overlaps(b7, b7, 'union'),
                lambda: m.rotated_overlaps(b5, b5, -1), lambda: m.box3d_overlaps(b7, b7, height_rule='torch'),
                lambda: m.box3d_overlaps(b7, b7, z_axis=3), lambda: m.box3d_overlaps(b7.cpu().numpy(), b7),
                lambda: m.box3d_overlaps(b7, b7, counts=([65], [64])), lambda: m.box3d_overlaps(b7, b7, counts=([64], [65])),
                lambda: m.rotated_overlaps(b5, b5, counts=([60, 5], [65])), lambda: m.image_overlaps(b4, b4, counts=([66, -1], [60, 5])),
                lambda: m.rotated_overlaps(b5, b5, counts=[65]), lambda: m.rotated_overlaps(b5, b5, aligned=True, counts=([65], [65]))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):          # mismatched devices
        m.box3d_overlaps(b7, torch.empty((65, 7), device='meta'))
    with pytest.raises(RuntimeError, match='z_center'):
        m.box3d_overlaps(b7, b7, z_center=float('nan'))
    assert m.box3d_overlaps(b7[:0], b7).shape == (0, 65) and m.rotated_overlaps(b5, b5[:0]).shape == (65, 0)
    assert m.box3d_overlaps(b7[:0], b7[:0], aligned=True).shape == (0,)


def test_cpu_tensors_are_refused():
    """the product binding, no emulation installed: a CPU tensor is an error, not a fallback"""
    import install as emu
    emu.uninstall()
    m = _mod()
    s = scene7(65, 1)
    b7, b5, b4 = (torch.from_numpy(as_kind(s, k)) for k in ('box3d', 'bev', 'image'))
    for bad in (lambda: m.box3d_overlaps(b7, b7), lambda: m.rotated_overlaps(b5, b5, aligned=True), lambda: m.image_overlaps(b4, b4),
                lambda: m.box3d_overlaps(b7, b7, counts=([65], [65])), lambda: m.bbox3d_overlaps_aligned_torch(b7, b7),
                lambda: m.bbox_rotate_overlaps_aligned_torch(b5, b5)):
        with pytest.raises(RuntimeError, match='HIP device'):
            bad()


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_boxes():
    """an aligned box3d_overlaps at N = 65 captured with torch.cuda.graph after a side-stream warm-up, replayed on changed box contents:
    each replay equals the eager call"""
    import install as emu
    emu.uninstall()
    m = _mod()
    d = torch.device('cuda:0')
    a, b, _ = aligned_case(65, 'box3d')
    sa, sb = dev(a, d), dev(b, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.box3d_overlaps(sa, sb, aligned=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.box3d_overlaps(sa, sb, aligned=True)
    for seed in (7, 8):
        s = scene7(130, seed)
        s2 = s[65:].copy()
        s2[::2] = s[:65][::2] + np.float32(0.05)
        sa.copy_(dev(s[:65], d))
        sb.copy_(dev(s2, d))
        graph.replay()
        eager = m.box3d_overlaps(sa.clone(), sb.clone(), aligned=True)
        torch.cuda.synchronize()
        assert float(eager.max()) > 0.3
        assert torch.equal(_bits(out), _bits(eager)), f'replay on scene {seed} differs from the eager call'
