"""epropnp.boxes (epropnp_bev_overlap, epropnp_bev_nms) against an fp64 oracle written here: a Sutherland-Hodgman clip of the two
corner quadrilaterals (a different algorithm from the kernel's edge integral) for overlap and IoU, and a greedy Python loop over that
fp64 IoU matrix for the suppression.  The reference's implementation is a CUDA extension: there is no fixture of its results.

Shapes: pairwise (M,N) in {(1,1), (3,65), (65,3), (64,64), (130,70)} -- one box, a ragged second tile either way, one full tile,
several ragged tiles -- and aligned at N in {1, 65}; NMS at N in {0, 1, 2, 63, 64, 65, 130, 600} -- nothing, a lone box, one tile
short / full / one over, several tiles, the ten tiles of the detection head's step -- each with one group at 0.25, with 3 (60 at
N = 600) groups at 0.25 and with the same groups at 0.5.  Scenes are clusters of near-duplicate detections (`scene`).

The keep lists are compared exactly.  That is fair only while no decision sits on the fence: every NMS case first asserts, from the
fp64 matrix, that no same-group pair has |IoU - thr| < 2e-5 (twice the cap of the IoU bar); the seeds are chosen so that it holds.

Bars: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over every case of this file; neither bar may
exceed 1e-5 (the smallest decision margin of the scenes is 6e-5).
    iou       |iou - iou64|                                   emulation 2.505e-7, MI355X 2.505e-7   -> bar 1.002e-6
    overlap   |overlap - overlap64| / max(area_a, area_b)     emulation 1.676e-7, MI355X 1.676e-7   -> bar 6.70e-7
"""
import math

import numpy as np
import pytest
import torch

IOU_BAR = 1.002e-6       # |iou - iou64|; cap 1e-5
OV_BAR = 6.70e-7         # |overlap - overlap64| / max(area_a, area_b); cap 1e-5
CAP = 1e-5
FENCE = 2e-5
SIZES = np.array([(4.6, 1.9), (11.0, 2.9), (0.7, 0.7), (2.1, 0.8), (6.9, 2.5)])
NMS_SIZES = (0, 1, 2, 63, 64, 65, 130, 600)
SEEDS = {0: 2, 1: 2, 2: 2, 63: 2, 64: 3, 65: 4, 130: 5, 600: 6}
_worst = {'iou': 0.0, 'overlap': 0.0}


def _boxes():
    from epropnp import boxes
    return boxes


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the fp64 oracle -----------------------------------------------------------------------------------------------------------
def corners64(b):
    """(n,5) -> (n,4,2) fp64 corners, counter-clockwise: (cx + u cos a + v sin a, cy - u sin a + v cos a)"""
    b = np.asarray(b, dtype=np.float64)
    u = b[:, 2:3] / 2 * np.array([1.0, -1.0, -1.0, 1.0])
    v = b[:, 3:4] / 2 * np.array([1.0, 1.0, -1.0, -1.0])
    c, s = np.cos(b[:, 4:5]), np.sin(b[:, 4:5])
    return np.stack((b[:, 0:1] + u * c + v * s, b[:, 1:2] - u * s + v * c), -1)


def _clip_area(pa, pb):
    """areas of the intersections of P pairs of convex counter-clockwise quadrilaterals pa, pb (P,4,2): Sutherland-Hodgman, all pairs
    at once (polygons in 8 slots + a vertex count)"""
    P, K = pa.shape[0], 8
    poly = np.zeros((P, K, 2))
    poly[:, :4] = pa
    cnt = np.full(P, 4)
    slot = np.arange(K)[None, :]
    for e in range(4):
        a, d = pb[:, e], pb[:, (e + 1) % 4] - pb[:, e]
        nxt_i = np.where(slot + 1 < cnt[:, None], slot + 1, 0)
        nxt = np.take_along_axis(poly, nxt_i[:, :, None], 1)
        side = d[:, None, 0] * (poly[:, :, 1] - a[:, None, 1]) - d[:, None, 1] * (poly[:, :, 0] - a[:, None, 0])
        side_n = np.take_along_axis(side, nxt_i, 1)
        live = slot < cnt[:, None]
        keep_cur = live & (side >= 0)
        cross = live & ((side >= 0) != (side_n >= 0))
        den = np.where(cross, side - side_n, 1.0)
        inter = poly + (side / den)[:, :, None] * (nxt - poly)
        cand = np.stack((poly, inter), 2).reshape(P, 2 * K, 2)
        ok = np.stack((keep_cur, cross), 2).reshape(P, 2 * K)
        first = np.argsort(~ok, axis=1, kind='stable')[:, :K]
        assert int(ok.sum(1).max(initial=0)) <= K
        poly = np.take_along_axis(cand, first[:, :, None], 1)
        cnt = ok.sum(1)
    nxt_i = np.where(slot + 1 < cnt[:, None], slot + 1, 0)
    nxt = np.take_along_axis(poly, nxt_i[:, :, None], 1)
    # shoelace about the first vertex (no cancellation against the scene's offset)
    p, q = poly - poly[:, :1], nxt - poly[:, :1]
    twice = np.where(slot < cnt[:, None], p[:, :, 0] * q[:, :, 1] - q[:, :, 0] * p[:, :, 1], 0.0).sum(1)
    return np.abs(twice) / 2


def valid64(b):
    b = np.asarray(b, dtype=np.float64)
    return np.isfinite(b).all(1) & (b[:, 2] >= 0) & (b[:, 3] >= 0)


def oracle(a, b, aligned=False):
    """(overlap64, iou64) of fp32 boxes a (M,5), b (N,5): (M,N), or (N,) aligned; NaN where either box is invalid"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    va, vb = valid64(a), valid64(b)
    a0, b0 = np.where(va[:, None], a, 0.0), np.where(vb[:, None], b, 0.0)
    if aligned:
        i = j = np.arange(a.shape[0])
        shape, ok = (a.shape[0],), va & vb
    else:
        shape, ok = (a.shape[0], b.shape[0]), va[:, None] & vb[None, :]
        # only the pairs that can touch are clipped
        ra, rb = np.hypot(a0[:, 2], a0[:, 3]) / 2, np.hypot(b0[:, 2], b0[:, 3]) / 2
        near = np.hypot(a0[:, None, 0] - b0[None, :, 0], a0[:, None, 1] - b0[None, :, 1]) <= (ra[:, None] + rb[None, :]) * 1.001 + 1e-9
        i, j = np.nonzero(near & ok)
    ov = np.zeros(shape)
    if len(i):
        flat = _clip_area(corners64(a0[i]), corners64(b0[j]))
        if aligned:
            ov[:] = flat
        else:
            ov[i, j] = flat
    area_a, area_b = a0[:, 2] * a0[:, 3], b0[:, 2] * b0[:, 3]
    union = (area_a + area_b - ov) if aligned else (area_a[:, None] + area_b[None, :] - ov)
    iou = ov / np.maximum(union, 1e-8)
    return np.where(ok, ov, np.nan), np.where(ok, iou, np.nan)


def greedy64(iou, scores, thr, groups=None, valid=None):
    """the kept indices in visiting order: descending score, equal scores lower index first"""
    n = len(scores)
    order = sorted(range(n), key=lambda k: (-scores[k], k))
    dead = np.zeros(n, dtype=bool)
    keep = []
    for pos, i in enumerate(order):
        if dead[i] or (valid is not None and not valid[i]):
            continue
        keep.append(i)
        for j in order[pos + 1:]:
            if (groups is None or groups[i] == groups[j]) and iou[i, j] > thr:
                dead[j] = True
    return keep


# ---- scenes (CPU, built once per key, never modified) --------------------------------------------------------------------------------
_scenes = {}


def scene(N, seed, G):
    """Det-like clusters of near-duplicate detections: N // 4 objects with centres uniform in [-40,40] x [3,70], a size of SIZES, any
    yaw and a group; each box an object's box with centre jitter N(0, 0.35 min size), size factor U(0.85, 1.15), yaw jitter
    N(0, 0.15) plus a random half turn, score U(0.05, 1).  -> dict of fp32 boxes (N,5), scores (N,), int32 groups (N,), fp64 IoU"""
    key = (N, seed, G)
    if key not in _scenes:
        rng = np.random.default_rng(seed)
        n_obj = max(N // 4, 1)
        centre = rng.uniform([-40.0, 3.0], [40.0, 70.0], (n_obj, 2))
        size = SIZES[rng.integers(0, len(SIZES), n_obj)]
        yaw = rng.uniform(-math.pi, math.pi, n_obj)
        group = rng.integers(0, G, n_obj)
        which = rng.integers(0, n_obj, N)
        c = centre[which] + rng.normal(0.0, 1.0, (N, 2)) * (0.35 * size[which].min(1))[:, None]
        wh = size[which] * rng.uniform(0.85, 1.15, (N, 2))
        a = yaw[which] + rng.normal(0.0, 0.15, N) + math.pi * rng.integers(0, 2, N)
        boxes = np.concatenate((c, wh, a[:, None]), 1).astype(np.float32).reshape(N, 5)
        scores = rng.uniform(0.05, 1.0, N).astype(np.float32)
        _scenes[key] = dict(boxes=boxes, scores=scores, groups=group[which].astype(np.int32), iou=oracle(boxes, boxes)[1])
    return _scenes[key]


def fence_margin(iou, groups, thr):
    """the smallest |IoU - thr| over the pairs that may interact"""
    n = iou.shape[0]
    if n < 2:
        return float('inf')
    same = np.ones((n, n), dtype=bool) if groups is None else groups[:, None] == groups[None, :]
    pick = same & ~np.eye(n, dtype=bool) & np.isfinite(iou)
    return float(np.abs(iou[pick] - thr).min()) if pick.any() else float('inf')


def check_values(got, want, scale, which, tag):
    """got fp32 tensor against the fp64 oracle: NaN exactly where the oracle has it, the rest within the bar; prints the figure"""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{tag}: NaN not exactly where a box is invalid'
    assert np.isfinite(got[~nan]).all(), tag
    err = float((np.abs(got - want)[~nan] / (scale[~nan] if scale is not None else 1.0)).max(initial=0.0))
    _worst[which] = max(_worst[which], err)
    bar = IOU_BAR if which == 'iou' else OV_BAR
    print(f'{tag}: worst {which} error {err:.3e} (bar {bar:.1e}); over the file so far {_worst[which]:.3e}')
    assert bar <= CAP and err <= bar, tag


def area_scale(a, b, aligned=False):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    aa, ab = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    with np.errstate(invalid='ignore'):
        s = np.maximum(aa, ab) if aligned else np.maximum(aa[:, None], ab[None, :])
    return np.where(np.isfinite(s) & (s > 0), s, 1.0)


def dev(x, backend):
    return torch.from_numpy(np.ascontiguousarray(x)).to(backend)


# ---- degenerate pairs ----------------------------------------------------------------------------------------------------------------
PI32 = float(np.float32(math.pi))
DEGENERATE = [
    # name, box a, box b, exact IoU or None
    ('identical', (1.5, 20.0, 4.0, 2.0, 0.7), (1.5, 20.0, 4.0, 2.0, 0.7), 1.0),
    ('turned by pi', (1.5, 20.0, 4.0, 2.0, 0.5), (1.5, 20.0, 4.0, 2.0, 0.5 + PI32), 1.0),
    ('turned by pi/2', (1.5, 20.0, 4.0, 2.0, 0.5), (1.5, 20.0, 4.0, 2.0, 0.5 + PI32 / 2), None),
    ('sharing an edge', (0.0, 0.0, 4.0, 2.0, 0.0), (4.0, 0.0, 4.0, 2.0, 0.0), 0.0),
    ('sharing a corner', (0.0, 0.0, 4.0, 2.0, 0.0), (4.0, 2.0, 4.0, 2.0, 0.0), 0.0),
    ('one inside another', (10.0, 30.0, 2.1, 0.8, 1.1), (10.2, 30.1, 11.0, 2.9, 0.9), None),
    ('the octagon', (-3.0, 12.0, 2.0, 2.0, 0.2), (-3.0, 12.0, 2.0, 2.0, 0.2 + PI32 / 4), None),
    ('zero width', (5.0, 8.0, 0.0, 2.9, 0.6), (5.1, 8.2, 4.6, 1.9, -0.4), 0.0),
    ('100 m apart', (0.0, 5.0, 4.6, 1.9, 0.3), (100.0, 5.0, 4.6, 1.9, 1.3), 0.0),
    ('identical at (30, 40)', (30.0, 40.0, 4.6, 1.9, -2.2), (30.0, 40.0, 4.6, 1.9, -2.2), 1.0),
]


def test_degenerate_pairs(backend, poisoned_empty):
    """exactly 1.0 for identical boxes (also away from the origin) and a box against itself turned by pi, exactly 0.0 for touching,
    zero-width and distant boxes, both ways round; everything finite and within the bars of the fp64 clip"""
    boxes = _boxes()
    a = np.array([d[1] for d in DEGENERATE], dtype=np.float32)
    b = np.array([d[2] for d in DEGENERATE], dtype=np.float32)
    for x, y, tag in ((a, b, 'a,b'), (b, a, 'b,a')):
        ov64, iou64 = oracle(x, y, aligned=True)
        iou = boxes.bev_iou(dev(x, backend), dev(y, backend), aligned=True)
        ov = boxes.bev_overlap(dev(x, backend), dev(y, backend), aligned=True)
        check_values(iou, iou64, None, 'iou', f'degenerate {tag} iou')
        check_values(ov, ov64, area_scale(x, y, True), 'overlap', f'degenerate {tag} overlap')
        for k, (name, _, _, exact) in enumerate(DEGENERATE):
            print(f'  {name:24s} iou {iou[k].item():.9g}  fp64 {iou64[k]:.12g}')
            if exact is not None:
                assert iou[k].item() == exact, f'{name} ({tag}): IoU {iou[k].item()!r} is not exactly {exact}'
        full = boxes.bev_iou(dev(x, backend), dev(y, backend))
        assert torch.equal(_bits(full.diagonal()), _bits(iou))
    octagon = 8 * (math.sqrt(2) - 1)           # of a square of side 2 against itself turned by pi/4
    assert abs(iou64[6] - octagon / (8 - octagon)) < 1e-6      # the oracle knows its octagon
    assert abs(iou64[5] - 2.1 * 0.8 / (11.0 * 2.9)) < 1e-6


# ---- pairwise shapes -------------------------------------------------------------------------------------------------------------
_pairs = {}


def pair_case(M, N):
    """M + N boxes of one clustered scene (so that pairs do overlap), fp32, with their fp64 results"""
    if (M, N) not in _pairs:
        s = scene(M + N, 11 + M + 3 * N, 1)
        a, b = s['boxes'][:M].copy(), s['boxes'][M:].copy()
        ov, iou = oracle(a, b)
        assert M * N < 50 or (iou > 0.05).sum() >= 3
        _pairs[(M, N)] = (a, b, ov, iou)
    return _pairs[(M, N)]


@pytest.mark.parametrize('M,N', [(1, 1), (3, 65), (65, 3), (64, 64), (130, 70)])
def test_pairwise_against_fp64(backend, poisoned_empty, M, N):
    boxes = _boxes()
    a, b, ov64, iou64 = pair_case(M, N)
    da, db = dev(a, backend), dev(b, backend)
    ov, iou = boxes.bev_overlap(da, db), boxes.bev_iou(da, db)
    assert ov.shape == (M, N) and iou.dtype == torch.float32
    check_values(iou, iou64, None, 'iou', f'pairwise {M}x{N} iou')
    check_values(ov, ov64, area_scale(a, b), 'overlap', f'pairwise {M}x{N} overlap')
    assert torch.equal(_bits(boxes.bev_iou(da, db)), _bits(iou)) and torch.equal(_bits(boxes.bev_overlap(da, db)), _bits(ov))
    # the other way round: the same pairs, the other box's frame
    check_values(boxes.bev_iou(db, da), iou64.T, None, 'iou', f'pairwise {N}x{M} (swapped) iou')


@pytest.mark.parametrize('N', [1, 65])
def test_aligned_is_the_diagonal(backend, poisoned_empty, N):
    boxes = _boxes()
    s = scene(2 * N, 40 + N, 1)
    a, b = s['boxes'][:N].copy(), s['boxes'][N:].copy()
    b[::2] = a[::2] + np.float32(0.1)          # every second pair does overlap
    da, db = dev(a, backend), dev(b, backend)
    ov64, iou64 = oracle(a, b, aligned=True)
    for fn, want, which, scale in ((boxes.bev_iou, iou64, 'iou', None), (boxes.bev_overlap, ov64, 'overlap', area_scale(a, b, True))):
        got = fn(da, db, aligned=True)
        assert got.shape == (N,)
        check_values(got, want, scale, which, f'aligned N={N} {which}')
        assert torch.equal(_bits(got), _bits(fn(da, db).diagonal())), 'aligned differs from the diagonal of the pairwise call'
        assert torch.equal(_bits(got), _bits(fn(da, db, aligned=True))), 'two launches differ'


def test_nan_exactly_in_the_rows_and_columns_of_invalid_boxes(backend, poisoned_empty):
    boxes = _boxes()
    a, b, _, _ = pair_case(130, 70)
    a, b = a.copy(), b.copy()
    a[3, 0] = np.nan          # a NaN coordinate
    a[64, 2] = np.inf         # an inf size
    a[129, 3] = -1.0          # a negative size
    b[0, 4] = np.nan
    b[65, 1] = -np.inf
    b[69, 2] = -0.5
    ov64, iou64 = oracle(a, b)
    assert np.isnan(iou64[[3, 64, 129]]).all() and np.isnan(iou64[:, [0, 65, 69]]).all() and np.isnan(iou64).sum() == 3 * 70 + 3 * 127
    da, db = dev(a, backend), dev(b, backend)
    check_values(boxes.bev_iou(da, db), iou64, None, 'iou', 'invalid boxes iou')
    check_values(boxes.bev_overlap(da, db), ov64, area_scale(a, b), 'overlap', 'invalid boxes overlap')
    al = boxes.bev_iou(da[:70], db, aligned=True)
    assert torch.equal(al.isnan().cpu(), torch.from_numpy(np.isnan(np.diagonal(iou64[:70]))))


# ---- NMS -----------------------------------------------------------------------------------------------------------------------------
def check_nms(res, want, N, tag):
    idx, mask, num = res.keep_index.cpu(), res.keep_mask.cpu(), res.num_keep.cpu()
    assert idx.dtype == torch.int32 and idx.shape == (N,) and mask.dtype == torch.bool and mask.shape == (N,)
    assert num.dtype == torch.int32 and num.shape == (1,)
    assert int(num) == len(want), f'{tag}: num_keep {int(num)}, the oracle keeps {len(want)}'
    assert idx[:len(want)].tolist() == want, f'{tag}: keep_index differs from the oracle'
    assert bool((idx[len(want):] == -1).all()), f'{tag}: the tail of keep_index is not -1'
    expect = torch.zeros(N, dtype=torch.bool)
    expect[torch.tensor(want, dtype=torch.int64)] = True
    assert torch.equal(mask, expect), f'{tag}: keep_mask is not the set of keep_index'


@pytest.mark.parametrize('mode', ['one group, 0.25', 'groups, 0.25', 'groups, 0.5'])
@pytest.mark.parametrize('N', NMS_SIZES)
def test_nms_against_the_greedy_oracle(backend, poisoned_empty, N, mode):
    boxes = _boxes()
    G = 60 if N >= 600 else 3
    s = scene(N, SEEDS[N], G)
    thr = 0.5 if mode.endswith('0.5') else 0.25
    groups = None if mode.startswith('one') else s['groups']
    margin = fence_margin(s['iou'], groups, thr)
    want = greedy64(s['iou'], s['scores'], thr, groups)
    above = 0 if N < 2 else int(((s['iou'] > thr) & (np.ones((N, N), bool) if groups is None else groups[:, None] == groups[None, :])).sum() - N) // 2
    print(f'N={N} {mode}: keeps {len(want)} of {N}, {above} interacting pairs above the threshold, smallest |IoU - thr| {margin:.2e}')
    assert margin >= FENCE, f'a decision of this scene sits on the fence ({margin:.2e}): choose another seed'
    assert N < 63 or (0.3 * N <= len(want) <= 0.8 * N and above >= 20), 'the scene does not exercise the suppression'
    db, ds = dev(s['boxes'], backend), dev(s['scores'], backend)
    dg = None if groups is None else dev(groups, backend)
    res = boxes.bev_nms(db, ds, thr, groups=dg)
    check_nms(res, want, N, f'N={N} {mode}')
    again = boxes.bev_nms(db, ds, thr, groups=dg)
    for x, y in zip(res, again):
        assert torch.equal(x, y), 'two launches differ'
    if groups is None:
        zero = boxes.bev_nms(db, ds, thr, groups=torch.zeros(N, dtype=torch.int32, device=backend))
        for x, y in zip(res, zero):
            assert torch.equal(x, y), 'groups=None differs from all groups 0'
    elif N == 600:
        one = boxes.bev_nms(db, ds, thr)
        saved = res.keep_mask & ~one.keep_mask
        print(f'  {int(saved.sum())} boxes are kept that the one-group call suppresses')
        assert int(saved.sum()) >= 1


def test_equal_scores_are_visited_lower_index_first(backend, poisoned_empty):
    boxes = _boxes()
    b = np.array([(0, 10, 4.6, 1.9, 0.3), (0.1, 10, 4.6, 1.9, 0.3), (30, 10, 4.6, 1.9, 0.3), (0, 10.1, 4.6, 1.9, 0.3),
                  (30, 10.1, 4.6, 1.9, 0.3)], dtype=np.float32)
    sc = np.array([0.5, 0.5, 0.5, 0.7, 0.5], dtype=np.float32)
    res = boxes.bev_nms(dev(b, backend), dev(sc, backend), 0.25)
    check_nms(res, [3, 2], 5, 'equal scores')
    res = boxes.bev_nms(dev(b[:3], backend), dev(sc[:3], backend), 0.25)
    check_nms(res, [0, 2], 3, 'equal scores')


def test_invalid_boxes_and_nan_scores_are_never_kept_and_suppress_nothing(backend, poisoned_empty):
    """box 0 has duplicates that come before it in the visiting order and would suppress it if they counted: one with a NaN score, one
    with a NaN coordinate, one with an inf size, one with a negative size.  It survives, and suppresses its one real duplicate."""
    boxes = _boxes()
    v = (2.0, 30.0, 4.6, 1.9, 0.4)
    b = np.array([v, v, v, v, v, v, (20.0, 30.0, 4.6, 1.9, 0.4)], dtype=np.float32)
    b[2, 1] = np.nan
    b[3, 2] = np.inf
    b[4, 3] = -1.9
    sc = np.array([0.5, np.nan, 0.9, 0.8, 0.7, 0.4, np.nan], dtype=np.float32)
    res = boxes.bev_nms(dev(b, backend), dev(sc, backend), 0.25)
    check_nms(res, [0], 7, 'invalid boxes')
    # the same through `order`: an entry outside [0, N) is skipped
    order = torch.tensor([7, 2, 3, 4, 0, -1, 5], dtype=torch.int32, device=backend)
    res = boxes.bev_nms(dev(b, backend), None, 0.25, order=order)
    check_nms(res, [0], 7, 'invalid boxes through order')


def test_far_from_the_origin_gives_the_same_keep_list(backend, poisoned_empty):
    """the scene at (3000, 3000) -- centres on a 2^-10 grid, so that the shift is exact in fp32 and the geometry identical -- with
    groups: the same keep list, since only centre differences enter the overlap"""
    boxes = _boxes()
    s = scene(130, SEEDS[130], 3)
    b = s['boxes'].copy()
    b[:, :2] = np.round(b[:, :2] * 1024) / 1024
    far = b.copy()
    far[:, :2] += np.float32(3000.0)
    assert np.array_equal(far[:, :2] - np.float32(3000.0), b[:, :2])
    iou = oracle(b, b)[1]
    assert fence_margin(iou, s['groups'], 0.25) >= FENCE
    want = greedy64(iou, s['scores'], 0.25, s['groups'])
    dg, ds = dev(s['groups'], backend), dev(s['scores'], backend)
    near_res = boxes.bev_nms(dev(b, backend), ds, 0.25, groups=dg)
    far_res = boxes.bev_nms(dev(far, backend), ds, 0.25, groups=dg)
    check_nms(near_res, want, 130, 'at the origin')
    check_nms(far_res, want, 130, 'at (3000, 3000)')
    assert torch.equal(_bits(boxes.bev_iou(dev(far, backend), dev(far, backend))), _bits(boxes.bev_iou(dev(b, backend), dev(b, backend))))


# ---- drop-ins ------------------------------------------------------------------------------------------------------------------------
def test_batched_bev_nms_is_the_references_call(backend, poisoned_empty):
    boxes = _boxes()
    s = scene(130, SEEDS[130], 3)
    N = 130
    g = torch.Generator().manual_seed(3)
    bbox = torch.rand(N, 10, generator=g)
    bev = torch.from_numpy(s['boxes'])
    bbox[:, 3], bbox[:, 5], bbox[:, 0], bbox[:, 2], bbox[:, 6], bbox[:, 7] = bev[:, 0], bev[:, 1], bev[:, 2], bev[:, 3], bev[:, 4], torch.from_numpy(s['scores'])
    want = greedy64(s['iou'], s['scores'], 0.25, s['groups'])
    batch_inds = torch.from_numpy(s['groups']).long()
    out, keep = boxes.batched_bev_nms(bbox.to(backend), batch_inds.to(backend))
    assert keep.dtype == torch.int64 and keep.cpu().tolist() == want
    assert torch.equal(out.cpu(), bbox[torch.tensor(want)])
    assert bool((out[:-1, 7] >= out[1:, 7]).all()), 'keep_inds are not in score order'
    for n in (0, 1):          # the reference's n <= 1: nothing is kept, a lone box included
        out, keep = boxes.batched_bev_nms(bbox[:n].to(backend), batch_inds[:n].to(backend))
        assert keep.dtype == torch.int64 and keep.shape == (0,) and out.shape == (0, 10)
    lone = boxes.bev_nms(dev(s['boxes'][:1], backend), dev(s['scores'][:1], backend), 0.25)
    assert lone.keep_index.cpu().tolist() == [0] and int(lone.num_keep) == 1


def test_nms_gpu_takes_xyxyr_boxes(backend, poisoned_empty):
    boxes = _boxes()
    s = scene(130, SEEDS[130], 3)
    b = s['boxes'].copy()
    b[:, :4] = np.round(b[:, :4] * 64) / 64          # corners and centres exact in fp32 either way
    xyxyr = np.stack((b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2, b[:, 4]), 1)
    db, dx, ds = dev(b, backend), dev(xyxyr, backend), dev(s['scores'], backend)
    ref = boxes.bev_nms(db, ds, 0.25)
    n = int(ref.num_keep)
    keep = boxes.nms_gpu(dx, ds, 0.25)
    assert keep.dtype == torch.int64 and torch.equal(keep, ref.keep_index[:n].long())
    assert torch.equal(boxes.nms_gpu(dx, ds, 0.25, post_max_size=5), keep[:5])
    # pre_maxsize: only the 40 best-scored boxes take part
    top = torch.sort(ds, descending=True, stable=True).indices[:40]
    sub = boxes.bev_nms(db[top], ds[top], 0.25)
    want = top[sub.keep_index[:int(sub.num_keep)].long()]
    got = boxes.nms_gpu(dx, ds, 0.25, pre_maxsize=40)
    assert torch.equal(got, want) and 1 <= got.numel() < n
    assert torch.equal(boxes.nms_gpu(dx, ds, 0.25, pre_maxsize=40, post_max_size=3), want[:3])


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def test_python_errors(backend):
    boxes = _boxes()
    s = scene(65, SEEDS[65], 3)
    b, sc, g = dev(s['boxes'], backend), dev(s['scores'], backend), dev(s['groups'], backend)
    for bad in (lambda: boxes.bev_iou(b.double(), b), lambda: boxes.bev_overlap(b, b.half()), lambda: boxes.bev_nms(b.double(), sc, 0.25),
                lambda: boxes.bev_nms(b, sc.double(), 0.25)):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: boxes.bev_iou(b[:, :4], b), lambda: boxes.bev_iou(b, b.reshape(-1)), lambda: boxes.bev_iou(b[:3], b, aligned=True),
                lambda: boxes.bev_overlap(b, b[:64], aligned=True), lambda: boxes.bev_nms(b, sc[:3], 0.25),
                lambda: boxes.bev_nms(b[:, :4], sc, 0.25), lambda: boxes.bev_nms(b, sc, 0.25, groups=g[:5]),
                lambda: boxes.bev_nms(b, sc, 0.25, groups=g.float()), lambda: boxes.bev_nms(b, None, 0.25),
                lambda: boxes.bev_nms(b, sc, 0.25, order=g.float()), lambda: boxes.bev_nms(b, sc, 0.25, order=g[:7]),
                lambda: boxes.batched_bev_nms(b, g), lambda: boxes.nms_gpu(b[:, :4], sc, 0.25), lambda: boxes.nms_gpu(b, sc[:4], 0.25)):
        with pytest.raises(ValueError):
            bad()
    assert boxes.bev_iou(b[:0], b).shape == (0, 65) and boxes.bev_iou(b, b[:0]).shape == (65, 0)
    assert boxes.bev_overlap(b[:0], b[:0], aligned=True).shape == (0,)


def test_cpu_tensors_are_refused():
    """the product binding, no emulation installed: a CPU tensor is an error, not a fallback"""
    import install as emu
    emu.uninstall()
    boxes = _boxes()
    s = scene(65, SEEDS[65], 3)
    b, sc = torch.from_numpy(s['boxes']), torch.from_numpy(s['scores'])
    for call in (lambda: boxes.bev_iou(b, b), lambda: boxes.bev_overlap(b, b, aligned=True), lambda: boxes.bev_nms(b, sc, 0.25),
                 lambda: boxes.nms_gpu(b, sc, 0.25), lambda: boxes.batched_bev_nms(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match='HIP device'):
            call()


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_boxes():
    """bev_nms(..., order=...) captured with torch.cuda.graph after a side-stream warm-up, replayed twice on changed box contents:
    each replay equals the eager call"""
    import install as emu
    emu.uninstall()
    boxes = _boxes()
    d = torch.device('cuda:0')
    s = scene(130, SEEDS[130], 3)
    sb = dev(s['boxes'], d)
    sg = dev(s['groups'], d)
    so = torch.sort(dev(s['scores'], d), descending=True, stable=True).indices.to(torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        boxes.bev_nms(sb, None, 0.25, groups=sg, order=so)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = boxes.bev_nms(sb, None, 0.25, groups=sg, order=so)
    for N2, seed in ((130, 6), (130, 7)):
        s2 = scene(N2, seed, 3)
        sb.copy_(dev(s2['boxes'], d))
        sg.copy_(dev(s2['groups'], d))
        so.copy_(torch.sort(dev(s2['scores'], d), descending=True, stable=True).indices.to(torch.int32))
        graph.replay()
        eager = boxes.bev_nms(sb.clone(), None, 0.25, groups=sg.clone(), order=so.clone())
        torch.cuda.synchronize()
        assert 30 <= int(eager.num_keep) <= 110
        for x, y in zip(out, eager):
            assert torch.equal(x, y), f'replay on scene {seed} differs from the eager call'
