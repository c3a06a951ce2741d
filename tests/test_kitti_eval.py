"""epropnp.evaluation against the reference's KITTI evaluation recorded in tests/golden/kitti_eval.npz (tools/make_kitti_eval_golden.py):
40 synthetic images, 18 cases (Car, Pedestrian, Cyclist x 3 difficulties x strict / loose), three metrics.

Matching level: the fixture's fp32 overlap blocks through `kitti_pr` -- pass-1 tuples per image, threshold lists and counts, tp / fp /
fn, precision and recall EXACTLY; the similarity within n_tp * 2^-52 * (similarity + 1) (two fixed-order fp64 sums of n_tp terms in
[0, 1] plus one ulp of cos per term) and the orientation curve within what follows from that.  End to end: the annotations through
`eval_class` / `kitti_eval` with the package's own fp32 overlaps, same assertions, and the result string.  Runs on the CPU emulation
and, marked gpu, on the device."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kitti_eval.npz')
EPS = 2.0 ** -52
_cache = {}


def tool():
    if 'tool' not in _cache:
        spec = importlib.util.spec_from_file_location('make_kitti_eval_golden', os.path.join(ROOT, 'tools', 'make_kitti_eval_golden.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache['tool'] = mod
    return _cache['tool']


def golden():
    """the fixture, its annotations and the host side of every case, computed once and shared (read-only)"""
    if 'rec' not in _cache:
        from epropnp import evaluation as ev
        rec = dict(np.load(GOLDEN))
        gts, dts = tool().annotations(rec)
        P = ev.prepare(gts, dts, list(tool().CLASSES), list(tool().DIFFICULTIES))
        _cache.update(rec=rec, gts=gts, dts=dts, P=P)
    return _cache['rec'], _cache['gts'], _cache['dts'], _cache['P']


def case_arrays(P, metric):
    """(ignored_gt (C,G), ignored_det (C,D), min_overlap (C,), num_valid_gt (C,)) in the fixture's case order"""
    cs = tool().cases()
    ig = np.stack([P.ignored_gt[m, l] for m, l, k in cs], 0)
    idt = np.stack([P.ignored_det[m, l] for m, l, k in cs], 0)
    mo = np.array([tool().MIN_OVERLAPS[k, metric, m] for m, l, k in cs])
    nv = np.array([P.num_valid_gt[m, l] for m, l, k in cs])
    return ig, idt, mo, nv


def device_args(backend, rec, P, metric, rows=None, dtype=torch.float32):
    from epropnp.evaluation import _offsets
    ig, idt, mo, nv = case_arrays(P, metric)
    if rows is not None:
        ig, idt, mo, nv = ig[rows], idt[rows], mo[rows], nv[rows]
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(d).to(backend)
    return (t(rec[f'overlaps_{metric}'], dtype), t(_offsets(P.dt_counts * P.gt_counts, np.int64), torch.int64),
            t(_offsets(P.gt_counts), torch.int32), t(_offsets(P.dt_counts), torch.int32), t(_offsets(P.dc_counts), torch.int32),
            t(P.gt_data, torch.float64), t(P.dt_data, torch.float64), t(P.dc_boxes, torch.float64), t(ig, torch.int8),
            t(idt, torch.int8), t(mo, torch.float64), t(nv, torch.int32), metric)


def similarity_bar(pr):
    """n_tp * 2^-52 * (similarity + 1), per (case, threshold)"""
    return pr[..., 0] * EPS * (pr[..., 3] + 1.0)


def orientation_bar(pr, n):
    """what the similarity bar leaves of aos = similarity / (tp + fp) and one rounding of the quotient; the running maximum from the
    right can only hand an entry's error on, so the largest bar of the row holds for every entry"""
    with np.errstate(divide='ignore', invalid='ignore'):
        bar = similarity_bar(pr) / (pr[..., 0] + pr[..., 1]) + EPS * np.abs(pr[..., 3] / (pr[..., 0] + pr[..., 1]))
    bar = np.where(np.arange(41)[None, :] < n[:, None], bar, 0.0)
    return np.nanmax(bar, axis=1, keepdims=True)


def check_pr(got_thr, got_cnt, got_pr, rec, metric, aos):
    want_thr, want_cnt, want_pr = rec['thresholds'][metric], rec['threshold_counts'][metric], rec['pr'][metric]
    assert np.array_equal(got_cnt, want_cnt)
    assert got_thr.tobytes() == want_thr.tobytes(), 'thresholds differ in a bit'
    assert np.array_equal(got_pr[..., :3], want_pr[..., :3]), 'tp / fp / fn'
    if aos:
        err, bar = np.abs(got_pr[..., 3] - want_pr[..., 3]), similarity_bar(want_pr)
        print(f'metric {metric}: similarity error up to {err.max():.3e}, the bar there {bar.flat[err.argmax()]:.3e}')
        assert (err <= bar).all()
    else:
        assert (got_pr[..., 3] == 0).all()


def check_curves(got, rec, metric, aos):
    shape = rec['precision'][metric].shape
    assert got['precision'].tobytes() == rec['precision'][metric].tobytes() and got['precision'].shape == shape
    assert got['recall'].tobytes() == rec['recall'][metric].tobytes()
    if aos:
        bar = orientation_bar(rec['pr'][metric], rec['threshold_counts'][metric]).reshape(shape[:3] + (1,))
        err = np.abs(got['orientation'] - rec['orientation'][metric])
        print(f'metric {metric}: orientation error up to {err.max():.3e}, the bar {bar.max():.3e}')
        assert (err <= bar).all()
    else:
        assert (got['orientation'] == 0).all()


def test_the_fixture_meets_its_conditions():
    rec = golden()[0]
    facts = {k[6:]: rec[k] for k in rec if k.startswith('facts_')}
    used = sorted(set(tool().MIN_OVERLAPS.reshape(-1).tolist()))
    for m in (0, 1, 2):      # what the arrays themselves show is taken from them, not from the record
        facts[f'margin32_{m}'] = min(np.abs(rec[f'overlaps_{m}'].astype(np.float64) - t).min() for t in used)
        assert rec[f'overlaps_{m}'].dtype == np.float32
    scores = rec['dt_score']
    facts['scores_are_hundredths'] = bool((np.round(scores, 2) == scores).all())
    facts['score_ties'] = int(scores.size - np.unique(scores).size)
    assert tool().conditions(rec, facts) == []
    gt, dt = rec['gt_counts'], rec['dt_counts']
    assert ((gt == 0) & (dt > 0)).any() and ((gt > 0) & (dt == 0)).any() and ((gt == 0) & (dt == 0)).any()
    assert ((dt >= 70) & (gt == 3)).any() and (gt >= 70).any()
    names = rec['name_table'][rec['gt_name']]
    assert {'Van', 'Person_sitting', 'DontCare'} <= set(names.tolist())
    assert (np.abs(rec['dt_bbox'][:, 3] - rec['dt_bbox'][:, 1]) < 25).any()
    assert os.path.getsize(GOLDEN) <= 300 * 1000 and all(rec[k].dtype != object for k in rec)


@pytest.mark.parametrize('metric', [0, 1, 2])
def test_matching_level(backend, metric):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    aos = metric == 0
    thr, cnt, pr, more = ev.kitti_pr(*device_args(backend, rec, P, metric), compute_aos=aos, details=True)
    thr, cnt, pr = thr.cpu().numpy(), cnt.cpu().numpy(), pr.cpu().numpy()
    check_pr(thr, cnt, pr, rec, metric, aos)
    # pass 1, per case and image: (tp, fp, fn) and the true positives' scores in ground-truth order
    state, scores = more['gt_state'].cpu().numpy(), more['tp_scores'].cpu().numpy()
    cuts = np.cumsum(P.gt_counts)[:-1]
    flat, case_off, off = rec[f'pass1_scores_{metric}'], rec[f'pass1_case_offsets_{metric}'], rec['pass1_offsets'][metric]
    for c in range(state.shape[0]):
        want = flat[case_off[c]:case_off[c + 1]]
        for i, (s, v) in enumerate(zip(np.split(state[c], cuts), np.split(scores[c], cuts))):
            hit = s == ev.GT_TRUE_POSITIVE
            assert (int(hit.sum()), 0, int((s == ev.GT_MISSED).sum())) == tuple(rec['pass1_counts'][metric, c, i]), (c, i)
            assert v[hit].tobytes() == want[off[c, i]:off[c, i + 1]].tobytes(), (c, i)
            assert np.isneginf(v[~hit]).all()
    assert np.array_equal(more['tp_count'].cpu().numpy(), rec['pass1_counts'][metric, :, :, 0].sum(1))
    got = ev.curves(cnt, pr, aos)
    shape = rec['precision'][metric].shape
    check_curves({k: v.reshape(shape) for k, v in zip(('precision', 'recall', 'orientation'), got)}, rec, metric, aos)
    for crit in ('R11', 'R40'):
        assert np.array_equal(ev.get_mAP(got[0].reshape(shape), crit), rec[f'mAP_{crit}'][metric])


@pytest.mark.parametrize('metric', [0, 1, 2])
def test_eval_class_end_to_end(backend, metric):
    """overlaps computed by the package in fp32 on the device; the recorded results come from fp64 overlaps"""
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    with ev.on_device(backend):
        got = ev.eval_class(gts, dts, list(tool().CLASSES), list(tool().DIFFICULTIES), metric, tool().MIN_OVERLAPS,
                            compute_aos=(metric == 0), num_parts=7)
    check_curves(got, rec, metric, metric == 0)


@pytest.mark.parametrize('criteria', ['R11', 'R40'])
def test_kitti_eval_end_to_end(backend, criteria):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    types = ['bbox', 'bev', '3d']
    with ev.on_device(backend):
        result, ret = ev.kitti_eval(gts, dts, ['Car', 'Pedestrian', 'Cyclist'], eval_types=types, criteria=criteria)
    assert types == ['bbox', 'bev', '3d'], 'the list of evaluation types was appended to'
    assert result == str(rec[f'result_{criteria}'])
    assert sorted(ret) == rec[f'ret_keys_{criteria}'].tolist()
    assert np.array_equal(np.array([ret[k] for k in sorted(ret)]), rec[f'ret_values_{criteria}'])


def test_fp64_overlaps_the_case_axis_and_a_second_call(backend):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    bits = lambda out: [t.cpu().numpy().tobytes() for t in out]
    first = bits(ev.kitti_pr(*device_args(backend, rec, P, 0), compute_aos=True))
    assert bits(ev.kitti_pr(*device_args(backend, rec, P, 0), compute_aos=True)) == first, 'a second call gives other bits'
    assert bits(ev.kitti_pr(*device_args(backend, rec, P, 0, dtype=torch.float64), compute_aos=True)) == first, 'fp64 overlaps'
    single = [ev.kitti_pr(*device_args(backend, rec, P, 0, rows=[c]), compute_aos=True) for c in range(18)]
    joined = bits([torch.cat([s[k] for s in single], 0) for k in range(3)])
    assert joined == first, 'C cases in one call are not C calls of one case'


def test_more_cases_than_the_lanes_of_a_wave(backend):
    """72 cases: the matching pass deals them to two waves per image, and the image beyond 64 detections keeps one flag row per wave"""
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    args = list(device_args(backend, rec, P, 0))
    for k in (8, 9, 10, 11):
        args[k] = torch.cat([args[k]] * 4, 0)
    thr, cnt, pr = (t.cpu().numpy() for t in ev.kitti_pr(*args, compute_aos=True))
    for r in range(4):
        check_pr(thr[18 * r:18 * r + 18], cnt[18 * r:18 * r + 18], pr[18 * r:18 * r + 18], rec, 0, True)
    assert all(pr[18 * r:18 * r + 18].tobytes() == pr[:18].tobytes() for r in range(4))


def test_every_output_element_is_written(backend, poisoned_empty):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    args = list(device_args(backend, rec, P, 0))
    # one more case without any ground truth of its class: no true positive, no threshold
    args[8] = torch.cat([args[8], torch.full_like(args[8][:1], -1)], 0)
    args[9] = torch.cat([args[9], args[9][:1]], 0)
    args[10], args[11] = torch.cat([args[10], args[10][:1]]), torch.cat([args[11], torch.zeros_like(args[11][:1])])
    thr, cnt, pr, more = ev.kitti_pr(*args, compute_aos=True, details=True)
    thr, cnt, pr = thr.cpu().numpy(), cnt.cpu().numpy(), pr.cpu().numpy()
    check_pr(thr[:18], cnt[:18], pr[:18], rec, 0, True)
    assert cnt[18] == 0 and (thr[18] == 0).all() and (pr[18] == 0).all()
    for c in range(19):
        assert (thr[c, cnt[c]:] == 0).all() and (pr[c, cnt[c]:] == 0).all()
    assert np.isfinite(pr).all() and np.isfinite(thr).all() and (cnt >= 0).all()
    assert not torch.isnan(more['tp_scores']).any() and (more['gt_state'] != -7).all() and (more['tp_count'].cpu()[18] == 0)
    assert not torch.isnan(more['tp_scores_at'][0, :int(cnt[0])]).any()


def test_degenerate_inputs_give_zeros(backend):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    mo = tool().MIN_OVERLAPS
    zeros = np.zeros((3, 3, 2, 41))
    with ev.on_device(backend):
        out = ev.eval_class([], [], [0, 1, 2], [0, 1, 2], 0, mo, compute_aos=True)      # zero images
        assert all(np.array_equal(out[k], zeros) for k in ('precision', 'recall', 'orientation'))
        empty = lambda a: {k: v[:0] for k, v in a.items()}
        out = ev.eval_class([empty(g) for g in gts[:3]], [empty(d) for d in dts[:3]], [0, 1, 2], [0, 1, 2], 2, mo)      # no boxes at all
        assert np.array_equal(out['precision'], zeros)
        no_cyclist = [{k: v[d['name'] != 'Cyclist'] for k, v in d.items()} for d in dts]      # a class without any detection
        out = ev.eval_class(gts, no_cyclist, [0, 1, 2], [0, 1, 2], 1, mo)
        assert np.array_equal(out['precision'][2], zeros[2]) and np.array_equal(out['recall'][2], zeros[2])
        assert out['precision'][0].tobytes() == rec['precision'][1][0].tobytes()
        no_car = [{k: v[g['name'] != 'Car'] for k, v in g.items()} for g in gts]      # num_valid_gt == 0 for Car
        out = ev.eval_class(no_car, dts, [0], [0, 1, 2], 0, mo[:, :, :1], compute_aos=True)
        assert all(np.array_equal(out[k], zeros[:1]) for k in ('precision', 'recall', 'orientation'))
    # all ground truths ignored (flag 1): matches are assigned, nothing is counted
    args = list(device_args(backend, rec, P, 0, rows=[2]))
    args[8] = torch.ones_like(args[8])
    args[11] = torch.zeros_like(args[11])
    thr, cnt, pr = ev.kitti_pr(*args, compute_aos=True)
    assert int(cnt[0]) == 0 and not thr.any() and not pr.any()
    # zero images at the device layer
    z = lambda *s, d=torch.float64: torch.zeros(s, dtype=d, device=backend)
    thr, cnt, pr = ev.kitti_pr(z(0, d=torch.float32), z(1, d=torch.int64), z(1, d=torch.int32), z(1, d=torch.int32), z(1, d=torch.int32),
                               z(0, 5), z(0, 6), z(0, 4), z(2, 0, d=torch.int8), z(2, 0, d=torch.int8), z(2) + 0.5, z(2, d=torch.int32), 0)
    assert not cnt.any() and not thr.any() and not pr.any()


def test_the_launch_count_does_not_depend_on_images_or_cases(backend):
    from epropnp import _hip, evaluation as ev
    rec, gts, dts, P = golden()
    seen = []
    for n_img, classes in ((40, [0, 1, 2]), (6, [1])):
        _hip.profile(True, reset=True)
        try:
            with ev.on_device(backend):
                ev.eval_class(gts[:n_img], dts[:n_img], classes, [0, 1, 2], 0, tool().MIN_OVERLAPS[:, :, classes], compute_aos=True)
            seen.append([_hip.profile_read(s)[1] for s in ('box_overlap_segmented', 'kitti_match', 'kitti_thresholds', 'kitti_statistics')])
        finally:
            _hip.profile(False, reset=True)
    assert seen == [[1, 1, 1, 1], [1, 1, 1, 1]]


def test_drop_ins_keep_the_reference_signatures_and_types(backend):
    from epropnp import evaluation as ev
    rec, gts, dts, P = golden()
    for line in rec['signatures'].tolist():
        name = line[:line.index('(')]
        assert f'{name}{inspect.signature(getattr(ev, name))}' == line
    assert not hasattr(ev, 'kitti_eval_coco_style')
    # clean_data / _prepare_data agree with the vectorised pass, in the reference's types
    i, cls, diff = 9, 0, 1
    nv, ig, idt, dc = ev.clean_data(gts[i], dts[i], cls, diff)
    g0, d0 = int(P.gt_counts[:i].sum()), int(P.dt_counts[:i].sum())
    assert isinstance(ig, list) and ig == P.ignored_gt[cls, diff, g0:g0 + len(ig)].tolist()
    assert idt == P.ignored_det[cls, diff, d0:d0 + len(idt)].tolist() and nv == ig.count(0) and isinstance(nv, int)
    gd, dd, igs, ids, dcs, dc_num, total = ev._prepare_data(gts, dts, cls, diff)
    assert len(gd) == len(gts) and igs[i].dtype == np.int64 and igs[i].tolist() == ig and ids[i].tolist() == idt
    assert total == int(P.num_valid_gt[cls, diff]) and dc_num.tolist() == P.dc_counts.tolist() and dcs[i].shape == (len(dc), 4)
    assert gd[i].shape == (len(ig), 5) and dd[i].shape == (len(idt), 6)
    # the per-image and per-part functions against the record, case (Car, moderate, loose) of metric 0
    c = tool().cases().index((cls, diff, 1))
    mo = tool().MIN_OVERLAPS[1, 0, cls]
    blocks = np.split(rec['overlaps_0'].astype(np.float64), np.cumsum(P.dt_counts * P.gt_counts)[:-1])
    ov = blocks[i].reshape(len(idt), len(ig))
    with ev.on_device(backend):
        tp, fp, fn, sim, thr = ev.compute_statistics_jit(ov, gd[i], dd[i], igs[i], ids[i], dcs[i], 0, min_overlap=mo, thresh=0.0)
        off, at = rec['pass1_offsets'][0, c], rec['pass1_case_offsets_0'][c]
        assert (tp, fp, fn) == tuple(rec['pass1_counts'][0, c, i]) and sim == 0
        assert thr.tobytes() == rec['pass1_scores_0'][at + off[i]:at + off[i + 1]].tobytes()
        every = rec['pass1_scores_0'][at:rec['pass1_case_offsets_0'][c + 1]].copy()
        n = rec['threshold_counts'][0, c]
        got = ev.get_thresholds(every, total)
        assert isinstance(got, list) and np.array(got).tobytes() == rec['thresholds'][0, c, :n].tobytes()
        part = np.zeros((int(P.dt_counts.sum()), int(P.gt_counts.sum())))
        r = q = 0
        for b, nd, ng in zip(blocks, P.dt_counts, P.gt_counts):
            part[r:r + nd, q:q + ng] = b.reshape(nd, ng)
            r, q = r + nd, q + ng
        pr = np.zeros((n, 4))
        ev.fused_compute_statistics(part, pr, P.gt_counts, P.dt_counts, dc_num, np.concatenate(gd, 0), np.concatenate(dd, 0),
                                    np.concatenate(dcs, 0), np.concatenate(igs, 0), np.concatenate(ids, 0), 0, min_overlap=mo,
                                    thresholds=np.array(got), compute_aos=True)
        assert np.array_equal(pr[:, :3], rec['pr'][0, c, :n, :3])
        assert (np.abs(pr[:, 3] - rec['pr'][0, c, :n, 3]) <= similarity_bar(rec['pr'][0, c, :n])).all()
        tp, fp, fn, sim, _ = ev.compute_statistics_jit(ov, gd[i], dd[i], igs[i], ids[i], dcs[i], 0, min_overlap=mo, thresh=got[-1],
                                                       compute_fp=True, compute_aos=True)
        assert tp + fn <= len(ig) and (sim == -1) == (tp == 0 and fp == 0)
