"""Writes tests/golden/kitti_eval.npz: synthetic KITTI annotations and what the REFERENCE's evaluation computes for them.

    python tools/make_kitti_eval_golden.py [--reference DIR] [--out FILE]

EPro-PnP-Det's core/evaluation/kitti_utils/eval.py imports numba, which is not installed and has no ROCm path.  At run time this tool
cuts the text of

    get_thresholds, clean_data, image_box_overlap, compute_statistics_jit, get_split_parts, fused_compute_statistics, _prepare_data,
    eval_class, get_mAP, do_eval, kitti_eval, d3_box_overlap_kernel

out of the reference checkout (by name, with ast) and execs it with `numba.jit` stubbed to the identity and `numba.prange` to `range`,
and with a `calculate_iou_partly` of this file in their namespace in place of the numba-CUDA one.  Nothing of the reference is stored
here.  Runs on the CPU (about a minute: the reference's loops run interpreted).

Overlaps: metric 0 from the reference's image_box_overlap, metric 1 the rotated IoU of the fp64 Sutherland-Hodgman clip of
tests/test_boxes.py, metric 2 the same clip through the reference's d3_box_overlap_kernel.  At the MATCHING level the per-image blocks
(detections x ground truths) are stored as fp32 values and the reference functions get them widened to fp64, so that both sides
compare the same numbers.  END TO END the reference gets the fp64 blocks and the package computes its own in fp32; the scene keeps
every fp64 overlap 1e-4 away from the minimum overlaps in use and distinct overlaps of one ground truth 2e-6 apart (the package's
fp32 overlaps are within 4e-7 of the fp64 ones, tests/test_box_overlaps.py, so neither a comparison nor an argmax can turn), and this tool asserts that both levels then give the reference the SAME
results, which are stored once.

Recorded: the annotations of 40 images (names as codes into `name_table`; boxes as fp32 values, which the reference gets as fp64);
per metric the stored blocks; for the 18 cases (Car, Pedestrian, Cyclist x 3 difficulties x the strict and loose minimum overlaps) the
reference's per-image pass-1 tuples, threshold lists, `pr` of fused_compute_statistics, precision / recall / orientation of
eval_class, get_mAP under R11 and R40; kitti_eval's result string and ret_dict; the signatures of the functions the package re-creates; the
figures the conditions are judged on (`facts_*`).
The conditions under CONDITIONS below are asserted before anything is written."""
import argparse
import ast
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'kitti_eval.npz')
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'epro-pnp_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
NAMES = ('get_thresholds', 'clean_data', 'image_box_overlap', 'compute_statistics_jit', 'get_split_parts', 'fused_compute_statistics',
         '_prepare_data', 'eval_class', 'get_mAP', 'do_eval', 'kitti_eval', 'd3_box_overlap_kernel')
NAME_TABLE = ('Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare')
CLASSES, DIFFICULTIES = (0, 1, 2), (0, 1, 2)
# [num_minoverlap, metric, class]: KITTI's strict and loose rows for Car, Pedestrian, Cyclist
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5]] + [[0.5, 0.25, 0.25]] * 2])
SIZES = {0: (3.9, 1.5, 1.6), 1: (0.8, 1.75, 0.6), 2: (1.8, 1.7, 0.6), 3: (5.0, 2.2, 1.9), 4: (0.8, 1.3, 0.6)}      # l, h, w
FOCAL, CU, CV = 720.0, 620.0, 190.0
GT_KEYS = ('name', 'bbox', 'alpha', 'occluded', 'truncated', 'location', 'dimensions', 'rotation_y')
DT_KEYS = GT_KEYS + ('score',)


class _Numba:
    """numba.jit / numba.jit(nopython=True, ...) as the identity, numba.prange as range"""
    prange = range

    @staticmethod
    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn


def reference_functions(ref=REF):
    """{name: function} exec'd from the text of the reference checkout into ONE namespace, which is returned under '__space__'"""
    import gc
    import io
    path = os.path.join(ref, 'EPro-PnP-Det', 'epropnp_det', 'core', 'evaluation', 'kitti_utils', 'eval.py')
    text = open(path).read()
    space = {'np': np, 'numba': _Numba, 'gc': gc, 'sysio': io}
    out = {}
    for node in ast.parse(text).body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            first = min([node.lineno] + [d.lineno for d in node.decorator_list])
            exec(compile('\n' * (first - 1) + '\n'.join(text.splitlines()[first - 1:node.end_lineno]) + '\n', path, 'exec'), space)
            out[node.name] = space[node.name]
    missing = [n for n in NAMES if n not in out]
    if missing:
        raise RuntimeError(f'{path}: {missing} not found')
    out['__space__'] = space
    return out


# ---- the scene ------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _bbox(loc, dims, ry):
    """a pinhole box: the object's extent along x (l |cos ry| + w |sin ry|) and its height h at depth z"""
    x, y, z = loc
    ln, h, w = dims
    half = (ln * abs(np.cos(ry)) + w * abs(np.sin(ry))) / 2
    return [FOCAL * (x - half) / z + CU, FOCAL * (y - h) / z + CV, FOCAL * (x + half) / z + CU, FOCAL * y / z + CV]


class _Rows:
    def __init__(self, with_score):
        self.rows, self.with_score = [], with_score

    def add(self, code, loc, dims, ry, occluded=0, truncated=0.0, score=0.0, bbox=None, alpha=None):
        bbox = _bbox(loc, dims, ry) if bbox is None else bbox
        alpha = ry - np.arctan2(loc[0], loc[2]) if alpha is None else alpha
        self.rows.append((code, bbox, alpha, occluded, truncated, list(loc), list(dims), ry, score))

    def anno(self):
        r = self.rows
        a = {'name': np.array([NAME_TABLE[x[0]] for x in r], dtype='<U14'), 'bbox': _f32([x[1] for x in r]).reshape(-1, 4),
             'alpha': _f32([x[2] for x in r]), 'occluded': np.array([x[3] for x in r], dtype=np.int64),
             'truncated': _f32([x[4] for x in r]), 'location': _f32([x[5] for x in r]).reshape(-1, 3),
             'dimensions': _f32([x[6] for x in r]).reshape(-1, 3), 'rotation_y': _f32([x[7] for x in r])}
        if self.with_score:
            a['score'] = np.array([x[8] for x in r], dtype=np.float64)
        return a


def _detect(rng, dt, code, loc, dims, ry, sigma, score=None):
    """a detection of an object: centre, size and yaw jittered by `sigma` (metres / relative / radians), score in hundredths"""
    loc2 = [loc[0] + rng.normal(0, sigma), loc[1] + rng.normal(0, sigma / 2), loc[2] + rng.normal(0, sigma)]
    dims2 = [d * (1 + rng.normal(0, sigma / 4)) for d in dims]
    ry2 = ry + rng.normal(0, sigma / 3)
    score = round(float(rng.uniform(0.05, 1.0)), 2) if score is None else score
    dt.add(code, loc2, dims2, ry2, score=score, alpha=ry2 - np.arctan2(loc2[0], loc2[2]) + rng.normal(0, 0.2))
    return loc2, dims2, ry2, score


def _objects(rng, gt, dt, n, codes, depth=(7.0, 60.0), rate=0.8, x0=None):
    for k in range(n):
        code = int(rng.choice(codes))
        z = rng.uniform(*depth)
        x = rng.uniform(-0.45, 0.45) * z if x0 is None else x0 + 6.0 * k
        loc, dims, ry = [x, 1.65, z], [s * rng.uniform(0.9, 1.1) for s in SIZES[code]], rng.uniform(-np.pi, np.pi)
        easy = rng.uniform() < 0.55
        occluded = 0 if easy else int(rng.integers(0, 4))
        truncated = round(float(rng.uniform(0, 0.1) if easy else rng.uniform(0, 0.6)), 2)
        if code == 2:      # cyclists: near, unoccluded, always found, tightly -> a case that reaches every recall position
            z = rng.uniform(7.0, 22.0)
            loc, occluded, truncated = [rng.uniform(-0.45, 0.45) * z, 1.65, z], 0, 0.0
        gt.add(code, loc, dims, ry, occluded, truncated)
        if code == 2 or rng.uniform() < (0.3 if code == 1 else rate):      # pedestrians: seldom and loosely -> cases with few thresholds
            sigma = {0: 0.12, 1: 0.3, 2: 0.01, 3: 0.15, 4: 0.1}[code]
            code_dt = {3: 0, 4: 1}.get(code, code)      # vans are found as cars, sitting persons as pedestrians
            found = _detect(rng, dt, code_dt, loc, dims, ry, sigma)
            if rng.uniform() < 0.25:      # a duplicate with the identical box: tied overlaps, another orientation, sometimes a tied score
                score = found[3] if rng.uniform() < 0.5 else round(float(rng.uniform(0.05, 1.0)), 2)
                dt.add(code_dt, found[0], found[1], found[2], score=score, alpha=rng.uniform(-3, 3))


def _tie_cluster(gt, dt, z, score):
    """two pedestrians half a length apart and two detections with ONE score: the first fits only the first pedestrian (IoU 0.67 /
    0.18), the second fits both (0.6 / 0.6) -- in the image, in BEV and in 3D.  In order the pedestrians take one each; with the
    detections reversed the first pedestrian takes the one the second needs."""
    dims = [1.0, 1.75, 0.6]
    for dx in (0.0, 0.5):
        gt.add(1, [2.0 + dx, 1.65, z], dims, 0.0)
    for dx in (-0.2, 0.25):
        dt.add(1, [2.0 + dx, 1.65, z], dims, 0.0, score=score, alpha=0.3 + dx)


def scene(seed):
    """-> (gt_annos, dt_annos) of 40 images"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for i in range(40):
        gt, dt = _Rows(False), _Rows(True)
        if i == 0:        # no ground truth
            for _ in range(4):
                _detect(rng, dt, int(rng.integers(0, 3)), [rng.uniform(-5, 5), 1.65, rng.uniform(8, 30)], SIZES[0], 0.3, 0.1)
        elif i == 1:      # no detection
            _objects(rng, gt, _Rows(True), 6, [0, 1, 3])
        elif i == 2:      # neither
            pass
        elif i == 3:      # 70 detections on 3 ground truths
            _objects(rng, gt, dt, 3, [0], depth=(10.0, 20.0), rate=1.0)
            while len(dt.rows) < 70:
                k = int(rng.integers(0, 3))
                _detect(rng, dt, 0, gt.rows[k][5], gt.rows[k][6], gt.rows[k][7], 0.25)
        elif i == 4:      # 70 ground truths
            _objects(rng, gt, dt, 70, [0, 0, 0, 1, 3], depth=(9.0, 55.0), rate=0.2, x0=-200.0)
        else:
            _objects(rng, gt, dt, int(rng.integers(4, 13)), [0, 0, 0, 0, 1, 1, 2, 2, 3, 4])
            if i % 7 == 5:
                _tie_cluster(gt, dt, 9.0 + i / 10, round(0.5 + i / 100, 2))
            for _ in range(int(rng.integers(0, 4))):      # false alarms, near and far
                z = rng.uniform(7.0, 70.0)
                _detect(rng, dt, int(rng.integers(0, 3)), [rng.uniform(-0.45, 0.45) * z, 1.65, z], SIZES[int(rng.integers(0, 3))], 0.3, 0.1)
            if i % 3 == 0:      # a DontCare region with detections inside it
                box = [40.0, 120.0, 300.0, 260.0]
                gt.add(5, [-1000.0, -1000.0, -1000.0], [1.0, 1.0, 1.0], 0.0, -1, -1.0, bbox=box, alpha=-10.0)
                for _ in range(2):
                    z = rng.uniform(12.0, 16.0)
                    code = int(rng.integers(0, 2))
                    x = (rng.uniform(80.0, 260.0) - CU) * z / FOCAL
                    _detect(rng, dt, code, [x, 1.65, z], SIZES[code], 0.2, 0.1)
        gts.append(gt.anno())
        dts.append(dt.anno())
    return gts, dts


# ---- overlaps ---------------------------------------------------------------------------------------------------------------------
def _boxes7(a):
    return np.concatenate([a['location'], a['dimensions'], a['rotation_y'][:, None]], 1)


def image_overlaps(ref, rows, cols, metric):
    """fp64 (rows, cols) IoU matrix of one image's annotations"""
    import test_boxes as tb
    if metric == 0:
        return ref['image_box_overlap'](rows['bbox'], cols['bbox'])
    a, b = _boxes7(rows), _boxes7(cols)
    inter, iou = tb.oracle(a[:, [0, 2, 3, 5, 6]], b[:, [0, 2, 3, 5, 6]])
    if metric == 1:
        return iou
    rinc = inter.copy()
    ref['d3_box_overlap_kernel'](a, b, rinc, -1)
    return rinc


def make_calculate_iou_partly(ref, stored=None):
    """a `calculate_iou_partly` for the reference's eval_class: per-image fp64 blocks (or the `stored` fp32 values, widened) and the
    block-diagonal part matrices"""
    def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50):
        total_dt_num = np.stack([len(a['name']) for a in dt_annos], 0)
        total_gt_num = np.stack([len(a['name']) for a in gt_annos], 0)
        if stored is None:
            overlaps = [image_overlaps(ref, g, d, metric) for g, d in zip(gt_annos, dt_annos)]
        else:
            overlaps = [b.astype(np.float64) for b in stored[metric]]
        parted, at = [], 0
        for n in ref['get_split_parts'](len(gt_annos), num_parts):
            part = np.zeros((int(total_gt_num[at:at + n].sum()), int(total_dt_num[at:at + n].sum())))
            r = c = 0
            for i in range(at, at + n):
                part[r:r + total_gt_num[i], c:c + total_dt_num[i]] = overlaps[i]
                r, c = r + int(total_gt_num[i]), c + int(total_dt_num[i])
            parted.append(part)
            at += n
        return overlaps, parted, total_gt_num, total_dt_num
    return calculate_iou_partly


def reversed_dets(anno):
    return {k: v[::-1].copy() for k, v in anno.items()}


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def cases():
    """(class, difficulty, k) in the order of the package's case axis"""
    return [(m, l, k) for m in CLASSES for l in DIFFICULTIES for k in range(MIN_OVERLAPS.shape[0])]


def build(ref_dir, seed):
    ref = reference_functions(ref_dir)
    space = ref['__space__']
    gts, dts = scene(seed)
    I = len(gts)
    rec, facts = {}, {}
    rec['name_table'] = np.array(NAME_TABLE, dtype='<U14')
    for tag, annos, keys in (('gt', gts, GT_KEYS), ('dt', dts, DT_KEYS)):
        rec[f'{tag}_counts'] = np.array([len(a['name']) for a in annos], dtype=np.int32)
        for k in keys:
            cat = np.concatenate([a[k] for a in annos], 0)
            if k == 'name':
                cat = np.array([NAME_TABLE.index(n) for n in cat], dtype=np.int8)
            elif k == 'occluded':
                cat = cat.astype(np.int8)
            elif k != 'score':
                cat = cat.astype(np.float32)
            rec[f'{tag}_{k}'] = cat
    used = sorted(set(MIN_OVERLAPS.reshape(-1).tolist()))
    blocks64 = {m: [image_overlaps(ref, d, g, m) for g, d in zip(gts, dts)] for m in (0, 1, 2)}
    stored = {m: [b.astype(np.float32) for b in blocks64[m]] for m in (0, 1, 2)}
    for m in (0, 1, 2):
        flat64 = np.concatenate([b.reshape(-1) for b in blocks64[m]])
        flat32 = np.concatenate([b.reshape(-1) for b in stored[m]])
        rec[f'overlaps_{m}'] = flat32
        facts[f'margin64_{m}'] = min(np.abs(flat64 - t).min() for t in used)
        facts[f'margin32_{m}'] = min(np.abs(flat32.astype(np.float64) - t).min() for t in used)
        gap = np.inf
        for b in blocks64[m]:      # distinct overlaps of one ground truth
            for col in b.T:
                v = np.unique(col[col > 0])
                if v.size > 1:
                    gap = min(gap, np.diff(v).min())
        facts[f'gap_{m}'] = gap
    # DontCare overlaps (intersection over the detection's area), fp64
    dc_margin, nstuff = np.inf, 0
    for g, d in zip(gts, dts):
        dc = g['bbox'][g['name'] == 'DontCare']
        if len(dc) and len(d['name']):
            o = ref['image_box_overlap'](d['bbox'], dc, 0)
            dc_margin = min(dc_margin, min(np.abs(o - t).min() for t in used))
    facts['dc_margin'] = dc_margin
    scores = np.concatenate([d['score'] for d in dts])
    facts['scores_are_hundredths'] = bool((np.round(scores, 2) == scores).all())
    facts['score_ties'] = int(scores.size - np.unique(scores).size)

    C = len(cases())
    results = {}
    for level, table in (('stored', stored), ('fp64', None)):
        space['calculate_iou_partly'] = make_calculate_iou_partly(ref, table)
        out = {'precision': [], 'recall': [], 'orientation': []}
        for metric in (0, 1, 2):
            r = ref['eval_class'](gts, dts, list(CLASSES), list(DIFFICULTIES), metric, MIN_OVERLAPS, compute_aos=(metric == 0))
            for k in out:
                out[k].append(r[k])
        results[level] = {k: np.stack(v, 0) for k, v in out.items()}
    for k in ('precision', 'recall', 'orientation'):
        assert np.array_equal(results['stored'][k], results['fp64'][k], equal_nan=True), \
            f'{k}: the reference gives other results on the fp64 overlaps than on their fp32 values'
        rec[k] = results['stored'][k]
    rec['mAP_R11'] = np.stack([ref['get_mAP'](rec['precision'][m], 'R11') for m in (0, 1, 2)], 0)
    rec['mAP_R40'] = np.stack([ref['get_mAP'](rec['precision'][m], 'R40') for m in (0, 1, 2)], 0)
    memo = {m: {k: results['stored'][k][m] for k in results['stored']} for m in (0, 1, 2)}      # kitti_eval asks for the same six runs
    space['eval_class'] = lambda g, d, classes, diffs, metric, mo, compute_aos=False, num_parts=200: memo[metric]
    for crit in ('R11', 'R40'):
        result, ret = ref['kitti_eval'](gts, dts, ['Car', 'Pedestrian', 'Cyclist'], eval_types=['bbox', 'bev', '3d'], criteria=crit)
        rec[f'result_{crit}'] = np.array(result)
        rec[f'ret_keys_{crit}'] = np.array(sorted(ret), dtype='<U40')
        rec[f'ret_values_{crit}'] = np.array([ret[k] for k in sorted(ret)], dtype=np.float64)

    # the stages, from the stored fp32 blocks
    p1_counts = np.zeros((3, C, I, 3), dtype=np.int32)
    p1_scores = {m: [] for m in (0, 1, 2)}
    p1_offsets = np.zeros((3, C, I + 1), dtype=np.int32)
    thresholds, thr_count, pr = np.zeros((3, C, 41)), np.zeros((3, C), dtype=np.int32), np.zeros((3, C, 41, 4))
    tie1, tie2, minus_one = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32), 0
    gt_num, dt_num = rec['gt_counts'].astype(np.int64), rec['dt_counts'].astype(np.int64)
    for metric in (0, 1, 2):
        ov = [b.astype(np.float64) for b in stored[metric]]
        part = make_calculate_iou_partly(ref, stored)(dts, gts, metric, 1)[1][0]
        for c, (m, l, k) in enumerate(cases()):
            min_overlap = MIN_OVERLAPS[k, metric, m]
            gd, dd, igs, ids, dcs, dc_num, num_valid = ref['_prepare_data'](gts, dts, CLASSES[m], DIFFICULTIES[l])
            every = []
            for i in range(I):
                tp, fp, fn, sim, thr = ref['compute_statistics_jit'](ov[i], gd[i], dd[i], igs[i], ids[i], dcs[i], metric,
                                                                     min_overlap=min_overlap, thresh=0.0, compute_fp=False)
                p1_counts[metric, c, i] = (tp, fp, fn)
                every += thr.tolist()
                p1_offsets[metric, c, i + 1] = len(every)
                if dt_num[i] > 1 and gt_num[i] > 0:      # the tie rule of pass 1: another result with the detections reversed
                    rv = ref['compute_statistics_jit'](ov[i][::-1], gd[i], dd[i][::-1], igs[i], ids[i][::-1], dcs[i], metric,
                                                       min_overlap=min_overlap, thresh=0.0, compute_fp=False)
                    tie1[metric] += int((tp, fp, fn) != rv[:3] or sorted(thr.tolist()) != sorted(rv[4].tolist()))
            p1_scores[metric].append(np.array(every, dtype=np.float64))
            thr = np.array(ref['get_thresholds'](np.array(every), num_valid))
            thr_count[metric, c] = len(thr)
            thresholds[metric, c, :len(thr)] = thr
            acc = np.zeros([len(thr), 4])
            ref['fused_compute_statistics'](part, acc, gt_num, dt_num, dc_num, np.concatenate(gd, 0), np.concatenate(dd, 0),
                                            np.concatenate(dcs, 0), np.concatenate(igs, 0), np.concatenate(ids, 0), metric,
                                            min_overlap=min_overlap, thresholds=thr, compute_aos=(metric == 0))
            pr[metric, c, :len(thr)] = acc
            if len(thr) and c % 2 == 1:      # the tie rule of pass 2 (largest overlap), probed at the lowest threshold, and similarity -1
                for i in range(I):
                    if dt_num[i] == 0:
                        continue
                    fw = ref['compute_statistics_jit'](ov[i], gd[i], dd[i], igs[i], ids[i], dcs[i], metric, min_overlap=min_overlap,
                                                       thresh=thr[-1], compute_fp=True, compute_aos=True)
                    minus_one += int(fw[3] == -1)
                    if metric == 0 and len(dcs[i]):
                        unassigned = ref['compute_statistics_jit'](ov[i], gd[i], dd[i], igs[i], ids[i], dcs[i][:0], metric,
                                                                   min_overlap=min_overlap, thresh=thr[-1], compute_fp=True)
                        nstuff += unassigned[1] - fw[1]
                    if dt_num[i] > 1 and gt_num[i] > 0:
                        rv = ref['compute_statistics_jit'](ov[i][::-1], gd[i], dd[i][::-1], igs[i], ids[i][::-1], dcs[i], metric,
                                                           min_overlap=min_overlap, thresh=thr[-1], compute_fp=True, compute_aos=True)
                        tie2[metric] += int(fw[:3] == rv[:3] and abs(fw[3] - rv[3]) > 1e-9)
    rec['pass1_counts'], rec['pass1_offsets'] = p1_counts, p1_offsets
    for metric in (0, 1, 2):
        rec[f'pass1_scores_{metric}'] = np.concatenate(p1_scores[metric]) if p1_scores[metric] else np.zeros(0)
        rec[f'pass1_case_offsets_{metric}'] = np.cumsum([0] + [len(s) for s in p1_scores[metric]]).astype(np.int32)
    rec['thresholds'], rec['threshold_counts'], rec['pr'] = thresholds, thr_count, pr
    facts.update(tie1=tie1, tie2=tie2, minus_one=minus_one, nstuff=nstuff)

    import epropnp.evaluation as ours      # only the NAMES are read here: the package's functions are not run
    sig = [f'{n}{inspect.signature(ref[n])}' for n in NAMES if n in ours.__dict__ or n in ('kitti_eval', 'do_eval')]
    rec['signatures'] = np.array(sig, dtype=f'<U{max(len(s) for s in sig)}')
    for k, v in facts.items():      # what only a run of the reference can tell, for the test that re-asserts the conditions
        rec[f'facts_{k}'] = np.asarray(v)
    return rec, facts


def conditions(rec, facts):
    """CONDITIONS: properties of the inputs and of the reference alone -> list of failures"""
    bad = []
    cs = cases()
    car_moderate = [c for c, (m, l, k) in enumerate(cs) if m == 0 and l == 1]
    n = rec['threshold_counts']
    for metric in (0, 1, 2):
        if min(n[metric, c] for c in car_moderate) < 20:
            bad.append(f'metric {metric}: Car moderate has {[int(n[metric, c]) for c in car_moderate]} thresholds, 20 are wanted')
        ap = rec['mAP_R11'][metric, 0]
        if not ((ap > 5).all() and (ap < 95).all()):
            bad.append(f'metric {metric}: Car AP(R11) {np.round(ap, 1).tolist()} is not inside (5, 95)')
        if facts['tie1'][metric] < 1 or facts['tie2'][metric] < 1:
            bad.append(f"metric {metric}: ties decide {facts['tie1'][metric]} pass-1 and {facts['tie2'][metric]} pass-2 results, 1 each is wanted")
        if facts[f'margin32_{metric}'] <= 1e-6 or facts[f'margin64_{metric}'] <= 1e-4:
            bad.append(f"metric {metric}: an overlap lies {facts[f'margin64_{metric}']:.2e} from a minimum overlap")
        if facts[f'gap_{metric}'] <= 2e-6:
            bad.append(f"metric {metric}: two distinct overlaps of one ground truth are {facts[f'gap_{metric}']:.2e} apart")
    if n.max() != 41:
        bad.append(f'no case reaches 41 thresholds (most: {n.max()})')
    if n.min() >= 10:
        bad.append(f'no case has fewer than 10 thresholds (fewest: {n.min()})')
    if facts['dc_margin'] <= 1e-9:
        bad.append('a DontCare overlap lies on a minimum overlap')
    if not facts['scores_are_hundredths'] or facts['score_ties'] < 1:
        bad.append('scores: hundredths with at least one tie are wanted')
    if facts['nstuff'] < 1:
        bad.append('no detection is taken off fp by a DontCare box')
    if facts['minus_one'] < 1:
        bad.append('similarity == -1 does not occur')
    return bad


def annotations(rec):
    """the fixture's annotations as the lists of dicts the evaluation takes (fp32 values as fp64)"""
    out = []
    for tag, keys in (('gt', GT_KEYS), ('dt', DT_KEYS)):
        cuts = np.cumsum(rec[f'{tag}_counts'])[:-1]
        cols = {}
        for k in keys:
            a = rec[f'{tag}_{k}']
            a = rec['name_table'][a.astype(np.int64)] if k == 'name' else (a.astype(np.int64) if k == 'occluded' else a.astype(np.float64))
            cols[k] = np.split(a, cuts)
        out.append([{k: cols[k][i] for k in keys} for i in range(len(cuts) + 1)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--seed', type=int, default=SEED)
    a = ap.parse_args()
    rec, facts = build(a.reference, a.seed)
    for k, v in facts.items():
        print(f'{k}: {v}')
    print('threshold counts:', rec['threshold_counts'].tolist())
    print('Car AP(R11) [metric, difficulty, strict/loose]:', np.round(rec['mAP_R11'][:, 0], 1).tolist())
    bad = conditions(rec, facts)
    if bad:
        raise SystemExit('the scene misses its conditions:\n  ' + '\n  '.join(bad))
    np.savez_compressed(a.out, **rec)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, {len(rec)} arrays')


SEED = 4

if __name__ == '__main__':
    main()
