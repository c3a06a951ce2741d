"""KITTI AP evaluation on the device: the reference's core/evaluation/kitti_utils/eval.py (numba-jit host code) under its own names.

    from epropnp.evaluation import kitti_eval
    result, ret_dict = kitti_eval(gt_annos, dt_annos, ['Car', 'Pedestrian', 'Cyclist'])

One `eval_class` call runs overlaps (`epropnp.boxes`, one segmented launch, detections as rows), greedy matching, recall thresholds
and PR sums on the device for ALL its class x difficulty x min-overlap cases at once, with a fixed number of launches, no
synchronisation between the stages, and one small copy of thresholds and sums to the host at the end; precision, recall, AOS and
their running maxima are formed there in fp64 as eval.py:547-560 does.  `kitti_pr` is the device layer underneath.  What needs
class-name strings (`clean_data`, `_prepare_data`) is host code, vectorised over the concatenated annotations.

The drop-ins keep the reference's signatures, so the device is chosen outside them: the current HIP device, or `with on_device(d):`.
`kitti_eval_coco_style` is not provided: the reference's `do_coco_style_eval` hands a bool to `do_eval` where the list of evaluation
types is expected and raises."""
import contextlib

import numpy as np
import torch

from . import _hip, boxes

N_SAMPLE_PTS = 41
GT_SKIPPED, GT_UNMATCHED, GT_TRUE_POSITIVE, GT_MISSED, GT_IGNORED_MATCH = -1, 0, 1, 2, 3      # include/epropnp_hip.h
_CLASS_NAMES = ('car', 'pedestrian', 'cyclist')
_MIN_HEIGHT = (40, 25, 25)
_MAX_OCCLUSION = (0, 1, 2)
_MAX_TRUNCATION = (0.15, 0.3, 0.5)
_NEIGHBOUR = {'pedestrian': 'person_sitting', 'car': 'van'}      # ground truths of these classes are neither hits nor misses
_device = None


@contextlib.contextmanager
def on_device(device):
    """Run the drop-ins of this module on `device` inside the block (default: the current HIP device)."""
    global _device
    saved, _device = _device, torch.device(device)
    try:
        yield
    finally:
        _device = saved


def _dev():
    return _device if _device is not None else torch.device('cuda', torch.cuda.current_device())


# ---- device layer ---------------------------------------------------------------------------------------------------------------
def _as(t, dtype, name, dev):
    if not torch.is_tensor(t):
        raise ValueError(f'{name}: a tensor is expected, got {type(t)}')
    if t.device != dev:
        raise RuntimeError(f'{name} lives on {t.device}, the overlaps on {dev}')
    return t.to(dtype).contiguous()


def kitti_pr(overlaps, block_offsets, gt_offsets, dt_offsets, dc_offsets, gt_data, dt_data, dc_boxes, ignored_gt, ignored_det,
             min_overlap, num_valid_gt, metric, compute_aos=False, recall_step=1.0 / (N_SAMPLE_PTS - 1.0), details=False):
    """Matching, thresholds and PR sums of C cases over I concatenated images, all on the device, no synchronisation.

    overlaps: flat fp32 or fp64, block i the row-major (detections of i, ground truths of i) matrix from block_offsets (I+1,);
    gt_offsets / dt_offsets / dc_offsets (I+1,); gt_data (G,5) bbox + alpha, dt_data (D,6) bbox + alpha + score, dc_boxes (Q,4);
    ignored_gt (C,G), ignored_det (C,D) in {-1, 0, 1}; min_overlap (C,), num_valid_gt (C,).
    -> thresholds (C,41) fp64 (zeros beyond the count), their counts (C,) int32, pr (C,41,4) fp64 [tp, fp, fn, similarity].
    details=True adds a dict: the pass-1 `tp_scores` (C,G), `tp_count` (C,), `gt_state` (C,G) and the pass-2 `tp_scores_at` (C,41,G)."""
    if not torch.is_tensor(overlaps) or overlaps.dtype not in (torch.float32, torch.float64):
        raise ValueError('overlaps: a flat fp32 or fp64 tensor is expected')
    dev = overlaps.device
    _hip.check_device(overlaps, 'overlaps')
    ov = overlaps.contiguous().view(-1)
    blk = _as(block_offsets, torch.int64, 'block_offsets', dev)
    go, do, qo = (_as(t, torch.int32, n, dev) for t, n in ((gt_offsets, 'gt_offsets'), (dt_offsets, 'dt_offsets'), (dc_offsets, 'dc_offsets')))
    gt, dt, dc = (_as(t, torch.float64, n, dev) for t, n in ((gt_data, 'gt_data'), (dt_data, 'dt_data'), (dc_boxes, 'dc_boxes')))
    ig, idt = _as(ignored_gt, torch.int8, 'ignored_gt', dev), _as(ignored_det, torch.int8, 'ignored_det', dev)
    mo, nv = _as(min_overlap, torch.float64, 'min_overlap', dev), _as(num_valid_gt, torch.int32, 'num_valid_gt', dev)
    I = int(go.shape[0]) - 1
    G, D, Q, Cn = int(gt.shape[0]), int(dt.shape[0]), int(dc.shape[0]), int(mo.shape[0])
    if I < 0 or do.shape[0] != I + 1 or qo.shape[0] != I + 1 or blk.shape[0] != I + 1:
        raise ValueError('the four offset arrays need the same length I + 1 >= 1')
    if gt.shape[1:] != (5,) or dt.shape[1:] != (6,) or dc.shape[1:] != (4,):
        raise ValueError(f'gt_data (G,5), dt_data (D,6), dc_boxes (Q,4) expected, got {tuple(gt.shape)}, {tuple(dt.shape)}, {tuple(dc.shape)}')
    if tuple(ig.shape) != (Cn, G) or tuple(idt.shape) != (Cn, D) or nv.shape[0] != Cn:
        raise ValueError(f'ignored_gt ({Cn},{G}), ignored_det ({Cn},{D}), num_valid_gt ({Cn},) expected')
    if metric not in (0, 1, 2):
        raise ValueError('unknown metric')
    f64 = 1 if ov.dtype == torch.float64 else 0
    st, p = _hip.stream_of(ov), _hip.ptr
    lib = _hip.lib()
    tp_scores = torch.empty((Cn, G), dtype=torch.float64, device=dev)
    tp_count = torch.empty((Cn,), dtype=torch.int32, device=dev)
    gt_state = torch.empty((Cn, G), dtype=torch.int8, device=dev) if details else None
    thresholds = torch.empty((Cn, N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    thr_count = torch.empty((Cn,), dtype=torch.int32, device=dev)
    pr = torch.empty((Cn, N_SAMPLE_PTS, 4), dtype=torch.float64, device=dev)
    tp_at = torch.empty((Cn, N_SAMPLE_PTS, G), dtype=torch.float64, device=dev) if details else None
    if Cn > 0:
        nb = int(lib.epropnp_kitti_match_scratch_bytes(D, Cn))
        scratch = torch.empty((max(nb, 8) // 8,), dtype=torch.int64, device=dev)
        _hip.call('epropnp_kitti_match', p(ov), f64, ov.numel(), p(go), p(do), p(blk), I, p(dt), G, D, p(ig), p(idt), p(mo), Cn,
                  p(scratch), nb, p(tp_scores), p(tp_count), p(gt_state), st)
        ordered = torch.sort(tp_scores, dim=1, descending=True).values if G > 0 else tp_scores
        _hip.call('epropnp_kitti_thresholds', p(ordered), p(tp_count), p(nv), G, Cn, float(recall_step), p(thresholds), p(thr_count), st)
        nb = int(lib.epropnp_kitti_statistics_scratch_bytes(I, D, Cn, int(bool(compute_aos))))
        scratch = torch.empty((max(nb, 8) // 8,), dtype=torch.int64, device=dev)
        _hip.call('epropnp_kitti_statistics', p(ov), f64, ov.numel(), p(go), p(do), p(qo), p(blk), I, p(gt), p(dt), p(dc), G, D, Q,
                  p(ig), p(idt), p(mo), Cn, p(thresholds), p(thr_count), int(metric), int(bool(compute_aos)), p(scratch), nb, p(pr),
                  p(tp_at), st)
    if details:
        return thresholds, thr_count, pr, dict(tp_scores=tp_scores, tp_count=tp_count, gt_state=gt_state, tp_scores_at=tp_at)
    return thresholds, thr_count, pr


# ---- host preparation: everything that compares class names -------------------------------------------------------------------------
def _cat(annos, key, width=None, dtype=None):
    tail = () if width is None else (width,)
    parts = [np.asarray(a[key], dtype=dtype).reshape((-1,) + tail) for a in annos]
    return np.concatenate(parts, 0) if parts else np.zeros((0,) + tail, dtype=dtype or np.float64)


def _offsets(counts, dtype=np.int32):
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out.astype(dtype)


def _gt_flags(names_lower, bbox, occluded, truncated, current_class, difficulty, same=None, neighbour=None):
    """clean_data's ignored_gt for concatenated ground truths: 0 counts, 1 neither hit nor miss, -1 another class"""
    cls = _CLASS_NAMES[current_class]
    if same is None:
        same, neighbour = _gt_classes(names_lower, cls)
    height = bbox[:, 3] - bbox[:, 1]
    hard = (occluded > _MAX_OCCLUSION[difficulty]) | (truncated > _MAX_TRUNCATION[difficulty]) | (height <= _MIN_HEIGHT[difficulty])
    return np.where(same & ~hard, 0, np.where(neighbour | (same & hard), 1, -1)).astype(np.int8)


def _gt_classes(names_lower, cls):
    same = names_lower == cls
    return same, (names_lower == _NEIGHBOUR[cls] if cls in _NEIGHBOUR else np.zeros(same.shape, dtype=bool))


def _dt_flags(names_lower, bbox, current_class, difficulty, same=None):
    """clean_data's ignored_dt: 1 below the minimum height (whatever the class), else 0 for this class and -1 for another"""
    if same is None:
        same = names_lower == _CLASS_NAMES[current_class]
    height = np.abs(bbox[:, 3] - bbox[:, 1])
    return np.where(height < _MIN_HEIGHT[difficulty], 1, np.where(same, 0, -1)).astype(np.int8)


def _lower(names):
    """np.char.lower, which calls str.lower per element; ASCII names (KITTI's are) are lowered on their code points instead"""
    if names.size == 0 or names.dtype.kind != 'U':
        return np.char.lower(names) if names.size else names
    codes = np.ascontiguousarray(names).view(np.uint32)
    if codes.max() > 127:
        return np.char.lower(names)
    return np.where((codes >= 65) & (codes <= 90), codes + 32, codes).astype(np.uint32).view(names.dtype).reshape(names.shape)


def _names(annos):
    return _cat(annos, 'name', dtype=str)


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """Drop-in for eval.py:33-85 -> (num_valid_gt, ignored_gt, ignored_dt, dc_bboxes), lists as the reference's."""
    gt_names, gt_bbox = _names([gt_anno]), _cat([gt_anno], 'bbox', 4)
    ignored_gt = _gt_flags(_lower(gt_names), gt_bbox, _cat([gt_anno], 'occluded'), _cat([gt_anno], 'truncated'), current_class, difficulty)
    ignored_dt = _dt_flags(_lower(_names([dt_anno])), _cat([dt_anno], 'bbox', 4), current_class, difficulty)
    dc_bboxes = [gt_anno['bbox'][i] for i in np.flatnonzero(gt_names == 'DontCare')]
    return int((ignored_gt == 0).sum()), ignored_gt.astype(int).tolist(), ignored_dt.astype(int).tolist(), dc_bboxes


class Prepared:
    """The concatenated annotations of an evaluation and the per-case flags, as host arrays (see `prepare`)."""


def prepare(gt_annos, dt_annos, current_classes, difficultys):
    """Concatenate the annotations and form clean_data's flags for every (class, difficulty) pair in one vectorised pass ->
    a `Prepared` with gt_counts / dt_counts / dc_counts (I,), gt_data (G,5), dt_data (D,6), dc_boxes (Q,4) in fp64, ignored_gt
    (M,L,G) and ignored_det (M,L,D) int8, num_valid_gt (M,L)."""
    assert len(gt_annos) == len(dt_annos)
    P = Prepared()
    P.num_images = len(gt_annos)
    P.gt_counts = np.array([len(a['name']) for a in gt_annos], dtype=np.int64)
    P.dt_counts = np.array([len(a['name']) for a in dt_annos], dtype=np.int64)
    gt_names, dt_names = _names(gt_annos), _names(dt_annos)
    gt_bbox, dt_bbox = _cat(gt_annos, 'bbox', 4), _cat(dt_annos, 'bbox', 4)
    occluded, truncated = _cat(gt_annos, 'occluded'), _cat(gt_annos, 'truncated')
    gl, dl = _lower(gt_names), _lower(dt_names)
    M, L = len(current_classes), len(difficultys)
    P.ignored_gt = np.zeros((M, L, gt_names.shape[0]), dtype=np.int8)
    P.ignored_det = np.zeros((M, L, dt_names.shape[0]), dtype=np.int8)
    for m, cls in enumerate(current_classes):
        same_gt, neighbour = _gt_classes(gl, _CLASS_NAMES[cls])      # the string comparisons, once per class
        same_dt = dl == _CLASS_NAMES[cls]
        for l, diff in enumerate(difficultys):
            P.ignored_gt[m, l] = _gt_flags(gl, gt_bbox, occluded, truncated, cls, diff, same_gt, neighbour)
            P.ignored_det[m, l] = _dt_flags(dl, dt_bbox, cls, diff, same_dt)
    P.num_valid_gt = (P.ignored_gt == 0).sum(-1)
    is_dc = gt_names == 'DontCare'
    image_of_gt = np.repeat(np.arange(P.num_images), P.gt_counts)
    P.dc_counts = np.bincount(image_of_gt[is_dc], minlength=P.num_images).astype(np.int64)
    P.dc_boxes = gt_bbox[is_dc].astype(np.float64).reshape(-1, 4)
    P.gt_data = np.concatenate([gt_bbox, _cat(gt_annos, 'alpha')[:, None]], 1).astype(np.float64)
    P.dt_data = np.concatenate([dt_bbox, _cat(dt_annos, 'alpha')[:, None], _cat(dt_annos, 'score')[:, None]], 1).astype(np.float64)
    return P


def _prepare_data(gt_annos, dt_annos, current_class, difficulty):
    """Drop-in for eval.py:424-452 -> (gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares, total_dc_num,
    total_num_valid_gt), per-image lists cut out of one concatenated pass."""
    P = prepare(gt_annos, dt_annos, [current_class], [difficulty])
    g, d, q = np.cumsum(P.gt_counts)[:-1], np.cumsum(P.dt_counts)[:-1], np.cumsum(P.dc_counts)[:-1]
    gt_datas = [np.concatenate([a['bbox'], a['alpha'][..., np.newaxis]], 1) for a in gt_annos]      # the annotations' own dtype
    dt_datas = [np.concatenate([a['bbox'], a['alpha'][..., np.newaxis], a['score'][..., np.newaxis]], 1) for a in dt_annos]
    return (gt_datas, dt_datas, np.split(P.ignored_gt[0, 0].astype(np.int64), g), np.split(P.ignored_det[0, 0].astype(np.int64), d),
            np.split(P.dc_boxes, q), P.dc_counts.copy(), int(P.num_valid_gt[0, 0]))


# ---- thin wrappers over the kernels, in the reference's types -----------------------------------------------------------------------
def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(_dev())


def _pr_of_blocks(blocks, gt_counts, dt_counts, dc_counts, gt_data, dt_data, dc_boxes, ignored_gt, ignored_det, min_overlap,
                  num_valid_gt, metric, compute_aos=False, thresholds=None, details=False, recall_step=1.0 / (N_SAMPLE_PTS - 1.0)):
    """host arrays in, `kitti_pr` (or, with thresholds given, its statistics stage alone) on the current device"""
    flat = np.concatenate([np.ascontiguousarray(b).reshape(-1) for b in blocks]) if len(blocks) else np.zeros(0)
    if flat.dtype not in (np.float32, np.float64):
        flat = flat.astype(np.float64)
    sizes = np.asarray(gt_counts, dtype=np.int64) * np.asarray(dt_counts, dtype=np.int64)
    args = (torch.from_numpy(flat).to(_dev()), _t(_offsets(sizes, np.int64), np.int64), _t(_offsets(gt_counts), np.int32),
            _t(_offsets(dt_counts), np.int32), _t(_offsets(dc_counts), np.int32), _t(np.reshape(gt_data, (-1, 5)), np.float64),
            _t(np.reshape(dt_data, (-1, 6)), np.float64), _t(np.reshape(dc_boxes, (-1, 4)), np.float64), _t(ignored_gt, np.int8),
            _t(ignored_det, np.int8), _t(min_overlap, np.float64), _t(num_valid_gt, np.int32), metric)
    if thresholds is None:
        return kitti_pr(*args, compute_aos=compute_aos, details=details, recall_step=recall_step)
    return _statistics(*args, _t(thresholds, np.float64), compute_aos=compute_aos)


def _statistics(ov, blk, go, do, qo, gt, dt, dc, ig, idt, mo, nv, metric, thresholds, compute_aos=False):
    """the statistics stage alone under GIVEN thresholds (Cn, n <= 41) -> pr (Cn,41,4), tp_scores_at (Cn,41,G)"""
    dev = ov.device
    Cn, n = int(thresholds.shape[0]), int(thresholds.shape[1])
    I, G, D, Q = int(go.shape[0]) - 1, int(gt.shape[0]), int(dt.shape[0]), int(dc.shape[0])
    thr = torch.zeros((Cn, N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    thr[:, :n] = thresholds
    cnt = torch.full((Cn,), n, dtype=torch.int32, device=dev)
    pr = torch.empty((Cn, N_SAMPLE_PTS, 4), dtype=torch.float64, device=dev)
    tp_at = torch.empty((Cn, N_SAMPLE_PTS, G), dtype=torch.float64, device=dev)
    nb = int(_hip.lib().epropnp_kitti_statistics_scratch_bytes(I, D, Cn, int(bool(compute_aos))))
    scratch = torch.empty((max(nb, 8) // 8,), dtype=torch.int64, device=dev)
    p = _hip.ptr
    _hip.call('epropnp_kitti_statistics', p(ov), 1 if ov.dtype == torch.float64 else 0, ov.numel(), p(go), p(do), p(qo), p(blk), I,
              p(gt), p(dt), p(dc), G, D, Q, p(ig), p(idt), p(mo), Cn, p(thr), p(cnt), int(metric), int(bool(compute_aos)), p(scratch),
              nb, p(pr), p(tp_at), _hip.stream_of(ov))
    return pr, tp_at


def get_thresholds(scores: np.ndarray, num_gt, num_sample_pts=41):
    """Drop-in for eval.py:12-30 -> list of thresholds.  Sorts `scores` in place, as the reference does; at most 41 sample points."""
    if num_sample_pts > N_SAMPLE_PTS:
        raise ValueError(f'num_sample_pts: at most {N_SAMPLE_PTS}, got {num_sample_pts}')
    scores.sort()
    dev, n = _dev(), int(scores.shape[0])
    ordered = torch.from_numpy(np.ascontiguousarray(scores[::-1], dtype=np.float64)).to(dev).view(1, n)
    tp_count, nv = torch.tensor([n], dtype=torch.int32, device=dev), torch.tensor([int(num_gt)], dtype=torch.int32, device=dev)
    thr = torch.empty((1, N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    _hip.call('epropnp_kitti_thresholds', _hip.ptr(ordered), _hip.ptr(tp_count), _hip.ptr(nv), n, 1, 1 / (num_sample_pts - 1.0),
              _hip.ptr(thr), _hip.ptr(cnt), _hip.stream_of(thr))
    return thr[0, :int(cnt.item())].cpu().tolist()


def compute_statistics_jit(overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap, thresh=0,
                           compute_fp=False, compute_aos=False):
    """Drop-in for eval.py:166-284 on one image -> (tp, fp, fn, similarity, thresholds): the scores of the true positives in
    ground-truth order last."""
    ng, nd = gt_datas.shape[0], dt_datas.shape[0]
    dc = np.reshape(np.asarray(dc_bboxes, dtype=np.float64), (-1, 4))
    common = ([np.reshape(overlaps, (nd, ng))], [ng], [nd], [dc.shape[0]], gt_datas, dt_datas, dc, np.reshape(ignored_gt, (1, ng)),
              np.reshape(ignored_det, (1, nd)), [min_overlap], [int((np.asarray(ignored_gt) == 0).sum())], metric)
    if not compute_fp:
        _, _, _, more = _pr_of_blocks(*common, details=True)
        state, scores = more['gt_state'][0].cpu().numpy(), more['tp_scores'][0].cpu().numpy()
        hit = state == GT_TRUE_POSITIVE
        return int(hit.sum()), 0, int((state == GT_MISSED).sum()), 0, scores[hit]
    pr, tp_at = _pr_of_blocks(*common, thresholds=[[thresh]], compute_aos=compute_aos)
    pr, scores = pr[0, 0].cpu().numpy(), tp_at[0, 0].cpu().numpy()
    tp, fp, fn = int(pr[0]), int(pr[1]), int(pr[2])
    similarity = 0 if not compute_aos else (pr[3] if tp > 0 or fp > 0 else -1)
    return tp, fp, fn, similarity, scores[scores > -np.inf]


def fused_compute_statistics(overlaps, pr, gt_nums, dt_nums, dc_nums, gt_datas, dt_datas, dontcares, ignored_gts, ignored_dets, metric,
                             min_overlap, thresholds, compute_aos=False):
    """Drop-in for eval.py:296-343: `overlaps` is a part's (detections, ground truths) matrix, of which image i's block on the
    diagonal is read; pr (len(thresholds), 4) += the sums over the part's images."""
    gt_nums, dt_nums = np.asarray(gt_nums, dtype=np.int64), np.asarray(dt_nums, dtype=np.int64)
    g, d = _offsets(gt_nums, np.int64), _offsets(dt_nums, np.int64)
    blocks = [overlaps[d[i]:d[i + 1], g[i]:g[i + 1]] for i in range(gt_nums.shape[0])]
    thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    G, D = int(g[-1]), int(d[-1])
    for t0 in range(0, thresholds.shape[0], N_SAMPLE_PTS):
        part = thresholds[t0:t0 + N_SAMPLE_PTS]
        out, _ = _pr_of_blocks(blocks, gt_nums, dt_nums, dc_nums, gt_datas[:G], dt_datas[:D], dontcares, np.reshape(ignored_gts[:G], (1, G)),
                               np.reshape(ignored_dets[:D], (1, D)), [min_overlap], [0], metric, compute_aos=compute_aos,
                               thresholds=part[None])
        pr[t0:t0 + part.shape[0]] += out[0, :part.shape[0]].cpu().numpy()


# ---- the evaluation -----------------------------------------------------------------------------------------------------------------
def _overlap_boxes(annos, metric):
    if metric == 0:
        return _cat(annos, 'bbox', 4)
    cols = [0, 2] if metric == 1 else [0, 1, 2]
    return np.concatenate([_cat(annos, 'location', 3)[:, cols], _cat(annos, 'dimensions', 3)[:, cols], _cat(annos, 'rotation_y')[:, None]], 1)


def device_overlaps(gt_annos, dt_annos, metric, counts):
    """flat fp32 overlaps on the device, block i the (detections, ground truths) IoU matrix of image i: ONE segmented launch"""
    dev = _dev()
    d = torch.from_numpy(np.ascontiguousarray(_overlap_boxes(dt_annos, metric), dtype=np.float32)).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(_overlap_boxes(gt_annos, metric), dtype=np.float32)).to(dev)
    if metric == 0:
        return boxes.image_overlaps(d, g, 'iou', counts=counts)[0]
    if metric == 1:
        return boxes.rotated_overlaps(d, g, 'iou', counts=counts)[0]
    return boxes.box3d_overlaps(d, g, 'iou', z_axis=1, z_center=1.0, counts=counts)[0]


def curves(thresholds_count, pr, compute_aos):
    """eval.py:547-560 for every case: pr (C,41,4) and the counts (C,) on the host -> precision, recall, aos (C,41) fp64, zero
    beyond each count, every entry the maximum of itself and the entries to its right"""
    Cn = pr.shape[0]
    precision, recall, aos = (np.zeros((Cn, N_SAMPLE_PTS)) for _ in range(3))
    with np.errstate(divide='ignore', invalid='ignore'):
        for c in range(Cn):
            n = int(thresholds_count[c])
            tp, fp, fn, sim = (pr[c, :n, k] for k in range(4))
            recall[c, :n] = tp / (tp + fn)
            precision[c, :n] = tp / (tp + fp)
            if compute_aos:
                aos[c, :n] = sim / (tp + fp)
            for a in (precision, recall) + ((aos,) if compute_aos else ()):
                a[c, :n] = np.maximum.accumulate(a[c, ::-1])[::-1][:n]
    return precision, recall, aos


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=200):
    """Drop-in for eval.py:455-572 -> {'recall', 'precision', 'orientation'}, each (num_class, num_difficulty, num_minoverlap, 41).
    All cases go through one launch per stage; `num_parts` is accepted and ignored."""
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError('unknown metric')
    M, L = len(current_classes), len(difficultys)
    min_overlaps = np.asarray(min_overlaps)
    K = len(min_overlaps)
    shape = [M, L, K, N_SAMPLE_PTS]
    ret = {'recall': np.zeros(shape), 'precision': np.zeros(shape), 'orientation': np.zeros(shape)}
    if len(gt_annos) == 0 or M * L * K == 0:
        return ret
    P = prepare(gt_annos, dt_annos, current_classes, difficultys)
    counts = (P.dt_counts.tolist(), P.gt_counts.tolist())
    flat = device_overlaps(gt_annos, dt_annos, metric, counts)
    rep = lambda a: np.repeat(a.reshape(M * L, -1), K, axis=0)      # case = ((m, l), k)
    min_ov = np.stack([np.asarray(min_overlaps[:, metric, m], dtype=np.float64) for m in range(M)], 0)      # (M, K)
    min_ov = np.broadcast_to(min_ov[:, None, :], (M, L, K)).reshape(-1)
    thr, cnt, pr = kitti_pr(flat, _t(_offsets(P.dt_counts * P.gt_counts, np.int64), np.int64), _t(_offsets(P.gt_counts), np.int32),
                            _t(_offsets(P.dt_counts), np.int32), _t(_offsets(P.dc_counts), np.int32), _t(P.gt_data, np.float64),
                            _t(P.dt_data, np.float64), _t(P.dc_boxes, np.float64), _t(rep(P.ignored_gt), np.int8),
                            _t(rep(P.ignored_det), np.int8), _t(min_ov, np.float64), _t(rep(P.num_valid_gt), np.int32), metric,
                            compute_aos=compute_aos)
    # the one copy: counts and sums travel together (the counts are exact in fp64)
    host = torch.cat([cnt.to(torch.float64)[:, None], pr.reshape(pr.shape[0], -1)], 1).cpu().numpy()
    precision, recall, aos = curves(host[:, 0], host[:, 1:].reshape(-1, N_SAMPLE_PTS, 4), compute_aos)
    ret['precision'], ret['recall'], ret['orientation'] = precision.reshape(shape), recall.reshape(shape), aos.reshape(shape)
    return ret


def get_mAP(prec, criteria='R11'):
    """Drop-in for eval.py:575-585: the mean of 11 (every fourth of the 41) or 40 (all but the first) sample points, in percent."""
    assert criteria in ['R11', 'R40']
    sums = 0
    picks = range(0, prec.shape[-1], 4) if criteria == 'R11' else range(1, prec.shape[-1])
    for i in picks:
        sums = sums + prec[..., i]
    return sums / (11 if criteria == 'R11' else 40) * 100


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, eval_types=['bbox', 'bev', '3d'], criteria='R11'):
    """Drop-in for eval.py:597-630 -> (mAP_bbox, mAP_bev, mAP_3d, mAP_aos), each (num_class, 3 difficulties, num_minoverlap) or None."""
    difficultys = [0, 1, 2]
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 0, min_overlaps, compute_aos=('aos' in eval_types))
    mAP_bbox = get_mAP(ret['precision'], criteria=criteria)
    mAP_aos = get_mAP(ret['orientation'], criteria=criteria) if 'aos' in eval_types else None
    mAP_bev = mAP_3d = None
    if 'bev' in eval_types:
        mAP_bev = get_mAP(eval_class(gt_annos, dt_annos, current_classes, difficultys, 1, min_overlaps)['precision'], criteria=criteria)
    if '3d' in eval_types:
        mAP_3d = get_mAP(eval_class(gt_annos, dt_annos, current_classes, difficultys, 2, min_overlaps)['precision'], criteria=criteria)
    return mAP_bbox, mAP_bev, mAP_3d, mAP_aos


_CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting'}
# [num_minoverlap, metric, class]: the strict and the loose row of KITTI's overlap requirements
_MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5]] * 3, [[0.7, 0.5, 0.5, 0.7, 0.5]] + [[0.5, 0.25, 0.25, 0.5, 0.25]] * 2])


def kitti_eval(gt_annos, dt_annos, current_classes, eval_types=['bbox', 'bev', '3d'], criteria='R11'):
    """Drop-in for eval.py:652-774 -> (result string, ret_dict).  `eval_types` is copied, not appended to."""
    assert 'bbox' in eval_types, 'must evaluate bbox at least'
    eval_types = list(eval_types)
    name_to_class = {v: n for n, v in _CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = _MIN_OVERLAPS[:, :, current_classes]
    compute_aos = False      # alpha == -10 marks detections without an orientation
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            if anno['alpha'][0] != -10:
                compute_aos = True
                eval_types.append('aos')
            break
    mAPbbox, mAPbev, mAP3d, mAPaos = do_eval(gt_annos, dt_annos, current_classes, min_overlaps, eval_types, criteria=criteria)
    rows = (('bbox AP:', mAPbbox, '{:.4f}', '2D'), ('bev  AP:', mAPbev, '{:.4f}', 'BEV'), ('3d   AP:', mAP3d, '{:.4f}', '3D'),
            ('aos  AP:', mAPaos if compute_aos else None, '{:.2f}', None))

    def line(head, values, fmt):
        return head + ', '.join(fmt.format(v) for v in values) + '\n'
    result, ret_dict = '', {}
    difficulty = ['easy', 'moderate', 'hard']
    for j, curcls in enumerate(current_classes):
        name = _CLASS_TO_NAME[curcls]
        for i in range(min_overlaps.shape[0]):
            result += '{} AP@{:.2f}, {:.2f}, {:.2f}:\n'.format(name, *min_overlaps[i, :, j])
            for head, mAP, fmt, _ in rows:
                if mAP is not None:
                    result += line(head, mAP[j, :, i], fmt)
            for idx in range(3):
                postfix = f"{difficulty[idx]}_{'strict' if i == 0 else 'loose'}"
                for _, mAP, _, key in (rows[2], rows[1], rows[0]):
                    if mAP is not None:
                        ret_dict[f'KITTI/{name}_{key}_{postfix}'] = mAP[j, idx, i]
    if len(current_classes) > 1:
        result += '\nOverall AP@{}, {}, {}:\n'.format(*difficulty)
        means = [(head, None if mAP is None else mAP.mean(axis=0), fmt, key) for head, mAP, fmt, key in rows]
        for head, mAP, fmt, _ in means:
            if mAP is not None:
                result += line(head, mAP[:, 0], fmt)
        for idx in range(3):
            for _, mAP, _, key in (means[2], means[1], means[0]):
                if mAP is not None:
                    ret_dict[f'KITTI/Overall_{key}_{difficulty[idx]}'] = mAP[idx, 0]
    return result, ret_dict
