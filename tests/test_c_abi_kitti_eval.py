"""epropnp_kitti_match / epropnp_kitti_thresholds / epropnp_kitti_statistics (and their scratch size queries) are additive entries of
the C ABI: same ABI version, the header is still plain C, the entries validate their arguments on the host, naming themselves, before
anything is launched, zero cases follow no pointer, a direct call gives what the header says, and offsets that point outside the arrays
-- device memory, which the host cannot check -- make the kernels skip that image."""

import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_kitti_match', 'epropnp_kitti_thresholds', 'epropnp_kitti_statistics', 'epropnp_kitti_match_scratch_bytes',
       'epropnp_kitti_statistics_scratch_bytes')
EINVAL = -1
MATCH = ['ov', 'f64', 'nov', 'go', 'do', 'blk', 'I', 'dt', 'G', 'D', 'ig', 'id', 'mo', 'C', 'scratch', 'bytes', 'tps', 'tpc', 'state']
THRESH = ['sorted', 'tpc', 'nv', 'G', 'C', 'step', 'thr', 'cnt']
STATS = ['ov', 'f64', 'nov', 'go', 'do', 'qo', 'blk', 'I', 'gt', 'dt', 'dc', 'G', 'D', 'Q', 'ig', 'id', 'mo', 'C', 'thr', 'cnt', 'metric',
         'aos', 'scratch', 'bytes', 'pr', 'tps']


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_kitti_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW, facts=[
        'EPROPNP_KITTI_SAMPLE_PTS == 41', 'EPROPNP_KITTI_GT_SKIPPED == -1', 'EPROPNP_KITTI_GT_UNMATCHED == 0',
        'EPROPNP_KITTI_GT_TRUE_POSITIVE == 1', 'EPROPNP_KITTI_GT_MISSED == 2', 'EPROPNP_KITTI_GT_IGNORED_MATCH == 3'])


def test_scratch_size_queries(lib):
    assert lib.epropnp_kitti_match_scratch_bytes(0, 5) == 0 and lib.epropnp_kitti_match_scratch_bytes(100, 0) == 0
    assert lib.epropnp_kitti_match_scratch_bytes(100, 64) == 100 * 8 and lib.epropnp_kitti_match_scratch_bytes(100, 65) == 2 * 100 * 8
    counts = ((3 * 41 * 3 * 4 + 7) // 8) * 8
    assert lib.epropnp_kitti_statistics_scratch_bytes(7, 100, 3, 0) == counts + 3 * 100 * 8
    assert lib.epropnp_kitti_statistics_scratch_bytes(7, 100, 3, 1) == 3 * 7 * 41 * 8 + counts + 3 * 100 * 8
    assert lib.epropnp_kitti_statistics_scratch_bytes(7, 100, 0, 1) == 0


def test_no_cases_is_not_an_error_and_touches_no_pointer(lib):
    p = 1      # pointers that must not be followed
    assert lib.epropnp_kitti_match(p, 0, 9, p, p, p, 3, p, 4, 5, p, p, p, 0, p, 0, p, p, p, None) == 0
    assert lib.epropnp_kitti_match(None, 0, 0, None, None, None, 0, None, 0, 0, None, None, None, 0, None, 0, None, None, None, None) == 0
    assert lib.epropnp_kitti_thresholds(p, p, p, 4, 0, 0.025, p, p, None) == 0
    assert lib.epropnp_kitti_statistics(p, 0, 9, p, p, p, p, 3, p, p, p, 4, 5, 6, p, p, p, 0, p, p, 0, 1, p, 0, p, p, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    big = 1 << 30

    def bad(entry, names, ok, cases):
        for kw in cases:
            args = [kw.get(n, v) for n, v in zip(names, ok)]
            assert getattr(lib, entry)(*args, None) == EINVAL, (entry, kw)
            assert entry.encode() + b':' in lib.epropnp_last_error(), lib.epropnp_last_error()
    ok = dict(ov=p, f64=0, nov=9, go=p, do=p, blk=p, I=3, dt=p, G=4, D=5, ig=p, id=p, mo=p, C=2, scratch=p, bytes=big, tps=p, tpc=p, state=None)
    bad(NEW[0], MATCH, [ok[n] for n in MATCH],
        [dict(I=-1), dict(G=-1), dict(D=-1), dict(C=-1), dict(nov=-1), dict(C=65536), dict(ov=None), dict(go=None), dict(do=None),
         dict(blk=None), dict(dt=None), dict(ig=None), dict(id=None), dict(mo=None), dict(tps=None), dict(tpc=None),
         dict(D=65, scratch=None), dict(D=65, bytes=65 * 8 - 1)])
    ok = dict(sorted=p, tpc=p, nv=p, G=4, C=2, step=0.025, thr=p, cnt=p)
    bad(NEW[1], THRESH, [ok[n] for n in THRESH],
        [dict(G=-1), dict(C=-1), dict(step=0.0), dict(step=-1.0), dict(step=float('nan')), dict(sorted=None), dict(tpc=None), dict(nv=None),
         dict(thr=None), dict(cnt=None)])
    ok = dict(ov=p, f64=0, nov=9, go=p, do=p, qo=p, blk=p, I=3, gt=p, dt=p, dc=p, G=4, D=5, Q=6, ig=p, id=p, mo=p, C=2, thr=p, cnt=p,
              metric=0, aos=1, scratch=p, bytes=big, pr=p, tps=None)
    need = lib.epropnp_kitti_statistics_scratch_bytes(3, 5, 2, 1)
    bad(NEW[2], STATS, [ok[n] for n in STATS],
        [dict(I=-1), dict(G=-1), dict(D=-1), dict(Q=-1), dict(C=-1), dict(nov=-1), dict(C=65536), dict(metric=3), dict(metric=-1),
         dict(ov=None), dict(go=None), dict(do=None), dict(qo=None), dict(blk=None), dict(gt=None), dict(dt=None), dict(dc=None),
         dict(ig=None), dict(id=None), dict(mo=None), dict(thr=None), dict(cnt=None), dict(pr=None), dict(scratch=None),
         dict(bytes=need - 1)])


# two images by hand: image 0 has ground truths 0, 1 and detections 0 .. 2, image 1 ground truth 2 and detection 3
OVERLAPS = [0.8, 0.6, 0.7, 0.9, 0.1, 0.2, 0.4]      # (3, 2) then (1, 1), detections as rows
SCORES = [0.9, 0.9, 0.3, 0.8]                       # a tied score: ground truth 0 takes detection 0, the lower index


def _problem(backend, gt_off, dt_off, dc_off, blk_off):
    t = lambda v, d: torch.tensor(v, dtype=d).to(backend)
    dt_data = torch.zeros(4, 6, dtype=torch.float64)
    dt_data[:, 5] = torch.tensor(SCORES, dtype=torch.float64)
    return dict(ov=t(OVERLAPS, torch.float32), go=t(gt_off, torch.int32), do=t(dt_off, torch.int32), qo=t(dc_off, torch.int32),
                blk=t(blk_off, torch.int64), gt=torch.zeros(3, 5, dtype=torch.float64).to(backend), dt=dt_data.to(backend),
                dc=torch.zeros(0, 4, dtype=torch.float64).to(backend), ig=torch.zeros(1, 3, dtype=torch.int8).to(backend),
                id=torch.zeros(1, 4, dtype=torch.int8).to(backend), mo=t([0.5], torch.float64), nv=t([3], torch.int32))


def _round_trip(backend, q):
    from epropnp import _hip
    p, lib = _hip.ptr, _hip.lib()
    I = q['go'].shape[0] - 1
    new = lambda shape, d, fill: torch.full(shape, fill, dtype=d).to(backend)
    tps, tpc, state = new((1, 3), torch.float64, 7.0), new((1,), torch.int32, -7), new((1, 3), torch.int8, -7)
    thr, cnt, pr = new((1, 41), torch.float64, 7.0), new((1,), torch.int32, -7), new((1, 41, 4), torch.float64, 7.0)
    st = _hip.stream_of(tps)
    nb = lib.epropnp_kitti_match_scratch_bytes(4, 1)
    scratch = new((max(nb, 8) // 8,), torch.int64, -1)
    _hip.call('epropnp_kitti_match', p(q['ov']), 0, 7, p(q['go']), p(q['do']), p(q['blk']), I, p(q['dt']), 3, 4, p(q['ig']), p(q['id']),
              p(q['mo']), 1, p(scratch), nb, p(tps), p(tpc), p(state), st)
    ordered = torch.sort(tps, dim=1, descending=True).values
    _hip.call('epropnp_kitti_thresholds', p(ordered), p(tpc), p(q['nv']), 3, 1, 1 / 40.0, p(thr), p(cnt), st)
    nb = lib.epropnp_kitti_statistics_scratch_bytes(I, 4, 1, 1)
    scratch = new((nb // 8,), torch.int64, -1)
    _hip.call('epropnp_kitti_statistics', p(q['ov']), 0, 7, p(q['go']), p(q['do']), p(q['qo']), p(q['blk']), I, p(q['gt']), p(q['dt']),
              p(q['dc']), 3, 4, 0, p(q['ig']), p(q['id']), p(q['mo']), 1, p(thr), p(cnt), 0, 1, p(scratch), nb, p(pr), None, st)
    return [x.cpu() for x in (tps, tpc, state, thr, cnt, pr)]


def _check(tps, tpc, state, thr, cnt, pr):
    assert tps[0].tolist() == [0.9, 0.9, float('-inf')] and tpc.tolist() == [2] and state[0].tolist() == [1, 1, 2]
    assert cnt.tolist() == [2] and thr[0, :2].tolist() == [0.9, 0.9] and not thr[0, 2:].any()
    # under the threshold 0.9 detections 2 and 3 are out: two true positives of similarity (1 + cos 0) / 2 each, one miss
    assert pr[0, 0].tolist() == [2.0, 0.0, 1.0, 2.0] and pr[0, 1].tolist() == [2.0, 0.0, 1.0, 2.0] and not pr[0, 2:].any()


def test_direct_calls_round_trip(backend):
    _check(*_round_trip(backend, _problem(backend, [0, 2, 3], [0, 3, 4], [0, 0, 0], [0, 6, 7])))


def test_an_image_whose_offsets_leave_the_arrays_is_skipped(backend):
    """the offsets are device memory: four more images with ranges beyond the arrays, reversed ranges, a block beyond the overlaps and
    negative offsets add nothing and touch nothing"""
    big = 2 ** 31 - 1
    q = _problem(backend, [0, 2, 3, 100, 3, 3, -5, 3], [0, 3, 4, 4, 4, big, 4, 4], [0, 0, 0, 0, 0, 7, 0, 0], [0, 6, 7, 7, 2 ** 40, 7, -1, 7])
    # images: 0, 1 good | 2: ground truths 3 .. 100 | 3: reversed range, block at 2^40 | 4: detections up to 2^31 - 1, DontCare 0 .. 7 of 0 |
    # 5: negative offsets | 6: empty
    _check(*_round_trip(backend, q))
