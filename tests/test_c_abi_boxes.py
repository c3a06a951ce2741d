"""epropnp_bev_overlap / epropnp_bev_nms / epropnp_bev_nms_scratch_bytes are additive entries of the C ABI: same ABI version, the
header is still plain C, the entries validate their arguments on the host, naming themselves, before anything is launched, an
`order` entry outside [0, N) is skipped on the device, and both calls show up in the stage recorder."""

import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_bev_overlap', 'epropnp_bev_nms', 'epropnp_bev_nms_scratch_bytes')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_box_entries_is_plain_c(tmp_path):
    from epropnp import boxes
    check_header_is_plain_c(tmp_path, NEW, facts=[f'EPROPNP_BEV_TILE == {boxes.TILE}'])


def test_no_boxes_is_not_an_error_and_touches_no_pointer(lib):
    assert lib.epropnp_bev_overlap(None, 0, None, 5, 1, 0, None, None) == 0
    assert lib.epropnp_bev_overlap(1, 3, 1, 0, 0, 0, 1, None) == 0          # (pointers that must not be followed)
    assert lib.epropnp_bev_overlap(1, 0, 1, 0, 1, 1, 1, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    cases = [(p, -1, p, 3, 1, 0, p), (p, 3, p, -2, 0, 0, p), (p, 3, p, 4, 1, 1, p), (None, 3, p, 3, 1, 0, p), (p, 3, None, 3, 1, 0, p),
             (p, 3, p, 3, 1, 0, None), (p, 3, p, 3, 1, 1, None)]
    for args in cases:
        assert lib.epropnp_bev_overlap(*args, None) == EINVAL, args
        assert NEW[0].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
    need = lib.epropnp_bev_nms_scratch_bytes(130)
    assert need == 130 * 3 * 8
    #     boxes order group N thr scratch bytes keep_index keep_mask num_keep
    ok = [p, p, p, 130, 0.25, p, need, p, p, p]
    cases = [ok[:3] + [-1] + ok[4:], ok[:3] + [-130] + ok[4:], ok[:3] + [(1 << 18) + 1] + ok[4:5] + [p, 1 << 40] + ok[7:]]
    for nbytes in (0, need - 1):                       # a scratch smaller than the size query, down to one byte short
        cases.append(ok[:6] + [nbytes] + ok[7:])
    for k in (0, 1, 5, 7, 8, 9):                       # each required pointer in turn (group may be NULL)
        cases.append(ok[:k] + [None] + ok[k + 1:])
    cases.append([None, None, None, 0, 0.25, None, 0, None, None, None])      # no boxes, but num_keep is still written
    for args in cases:
        assert lib.epropnp_bev_nms(*args, None) == EINVAL, args
        assert NEW[1].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_scratch_query_is_monotone_and_at_least_the_mask(lib):
    q = lib.epropnp_bev_nms_scratch_bytes
    assert q(0) == 0 and q(-5) == 0 and q(1) == 8 and q(64) == 64 * 8 and q(65) == 65 * 2 * 8
    last = 0
    for n in list(range(0, 200)) + [600, 4095, 4096, 4097, 16384, 1 << 18]:
        assert q(n) >= n * ((n + 63) // 64) * 8 and q(n) >= last, n
        last = q(n)
    assert q(1 << 18) == (1 << 18) * (1 << 12) * 8      # no 32-bit overflow


def _nms(backend, boxes, order, thr=0.25):
    """the library call itself, on raw pointers"""
    from epropnp import _hip
    N = boxes.shape[0]
    scratch = torch.zeros((N * ((N + 63) // 64),), dtype=torch.int64, device=backend)
    keep_index = torch.full((N,), -7, dtype=torch.int32, device=backend)
    keep_mask = torch.full((N,), 9, dtype=torch.uint8, device=backend)
    num_keep = torch.full((1,), -7, dtype=torch.int32, device=backend)
    _hip.call('epropnp_bev_nms', _hip.ptr(boxes), _hip.ptr(order), None, N, thr, _hip.ptr(scratch), scratch.numel() * 8,
              _hip.ptr(keep_index), _hip.ptr(keep_mask), _hip.ptr(num_keep), _hip.stream_of(boxes))
    return keep_index.cpu().tolist(), keep_mask.cpu().tolist(), int(num_keep)


def test_an_order_entry_out_of_range_is_skipped(backend):
    """70 well separated boxes (two tiles), visited backwards, with entries below 0, at N and far beyond in both tiles: the rest is
    kept in visiting order, the boxes those entries replaced are not"""
    N = 70
    boxes = torch.zeros(N, 5)
    boxes[:, 0] = torch.arange(N) * 10.0
    boxes[:, 2:4] = torch.tensor([4.6, 1.9])
    order = torch.arange(N - 1, -1, -1, dtype=torch.int32)
    bad = {0: -1, 5: N, 63: 2 ** 31 - 1, 64: -2 ** 31, 69: N + 1000}
    for pos, v in bad.items():
        order[pos] = v
    want = [int(v) for pos, v in enumerate(order.tolist()) if pos not in bad]
    idx, mask, num = _nms(backend, boxes.to(backend), order.to(backend))
    assert num == N - len(bad) and idx[:num] == want and idx[num:] == [-1] * len(bad)
    assert mask == [1 if i in want else 0 for i in range(N)]


def test_both_calls_show_up_in_the_stage_recorder(backend):
    from epropnp import _hip, boxes
    b = torch.zeros(3, 5)
    b[:, 0] = torch.arange(3) * 10.0
    b[:, 2:4] = 2.0
    b = b.to(backend)
    _hip.profile(True, reset=True)
    try:
        boxes.bev_iou(b, b)
        boxes.bev_overlap(b, b, aligned=True)
        boxes.bev_nms(b, b[:, 0].contiguous(), 0.25)
        assert _hip.profile_read('bev_overlap')[1] == 2
        assert _hip.profile_read('bev_nms')[1] == 1          # one stage over both launches
    finally:
        _hip.profile(False, reset=True)
