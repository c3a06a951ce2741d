"""epropnp_box_overlap / epropnp_box_overlap_plan / epropnp_box_overlap_segmented are additive entries of the C ABI: same ABI version,
the header is still plain C, the entries validate their arguments on the host, naming themselves, before anything is launched, zero
counts follow no pointer, the plan's tile table is what the header says, a table entry that points outside the boxes or the output is
skipped on the device, and both launches show up in the stage recorder."""
import ctypes

import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_box_overlap', 'epropnp_box_overlap_plan', 'epropnp_box_overlap_segmented')
EINVAL = -1
BEV, BOX3D, IMAGE = 0, 1, 2
IOU, CRIT_A, CRIT_B, INTER = -1, 0, 1, 2
INTERVAL, REFERENCE_TORCH = 0, 1
COUNTS_A, COUNTS_B = [0, 3, 70, 1, 0, 64], [5, 0, 65, 1, 0, 130]


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_box_overlap_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW, run=True, facts=[
        f'EPROPNP_BOX_BEV == {BEV}', f'EPROPNP_BOX_3D == {BOX3D}', f'EPROPNP_BOX_IMAGE == {IMAGE}', f'EPROPNP_BOX_CRIT_IOU == {IOU}',
        f'EPROPNP_BOX_CRIT_A == {CRIT_A}', f'EPROPNP_BOX_CRIT_B == {CRIT_B}', f'EPROPNP_BOX_CRIT_INTER == {INTER}',
        f'EPROPNP_BOX_HEIGHT_INTERVAL == {INTERVAL}', f'EPROPNP_BOX_HEIGHT_REFERENCE_TORCH == {REFERENCE_TORCH}',
        'EPROPNP_BOX_TILE_INTS == 6'])


def test_no_boxes_is_not_an_error_and_touches_no_pointer(lib):
    assert lib.epropnp_box_overlap(None, 0, None, 5, BOX3D, IOU, 1, 0.5, INTERVAL, 0, None, None) == 0
    assert lib.epropnp_box_overlap(1, 3, 1, 0, BEV, INTER, 1, 0.5, INTERVAL, 0, 1, None) == 0          # (pointers that must not be followed)
    assert lib.epropnp_box_overlap(1, 0, 1, 0, IMAGE, CRIT_A, 1, 0.5, INTERVAL, 1, 1, None) == 0
    assert lib.epropnp_box_overlap_segmented(1, 3, 1, 4, BOX3D, IOU, 1, 0.5, INTERVAL, 1, 0, 1, 12, None) == 0      # no tiles
    assert lib.epropnp_box_overlap_segmented(1, 0, 1, 4, BOX3D, IOU, 1, 0.5, INTERVAL, 1, 3, 1, 0, None) == 0       # no boxes, no output
    assert lib.epropnp_box_overlap_plan(None, None, 0, None, 0, None, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    nan, inf = float('nan'), float('inf')
    #     boxes_a num_a boxes_b num_b kind criterion z_axis z_center rule aligned out
    ok = [p, 3, p, 3, BOX3D, IOU, 1, 0.5, INTERVAL, 0, p]

    def but(**kw):
        names = ['a', 'na', 'b', 'nb', 'kind', 'crit', 'z_axis', 'z_center', 'rule', 'aligned', 'out']
        return [kw.get(n, v) for n, v in zip(names, ok)]
    cases = [but(na=-1), but(nb=-2), but(nb=4, aligned=1), but(a=None), but(b=None), but(out=None), but(out=None, aligned=1),
             but(kind=3), but(kind=-1), but(crit=3), but(crit=-2), but(rule=2), but(rule=-1), but(z_axis=3), but(z_axis=-1),
             but(z_center=nan), but(z_center=inf), but(kind=BEV, z_center=-inf), but(na=65535 * 64 + 1)]
    for args in cases:
        assert lib.epropnp_box_overlap(*args, None) == EINVAL, args
        assert NEW[0].encode() + b':' in lib.epropnp_last_error(), lib.epropnp_last_error()
    # z_axis is read for 3D boxes only
    assert lib.epropnp_box_overlap(*but(kind=BEV, z_axis=7, na=0), None) == 0
    #     boxes_a num_a boxes_b num_b kind criterion z_axis z_center rule tiles num_tiles out num_out
    ok = [p, 3, p, 3, BOX3D, IOU, 1, 0.5, INTERVAL, p, 1, p, 9]
    names = ['a', 'na', 'b', 'nb', 'kind', 'crit', 'z_axis', 'z_center', 'rule', 'tiles', 'nt', 'out', 'no']
    cases = [dict(na=-1), dict(nb=-1), dict(nt=-1), dict(no=-1), dict(no=1 << 31), dict(a=None), dict(b=None), dict(tiles=None),
             dict(out=None), dict(kind=5), dict(crit=7), dict(rule=9), dict(z_axis=4), dict(z_center=nan)]
    for kw in cases:
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        assert lib.epropnp_box_overlap_segmented(*args, None) == EINVAL, args
        assert NEW[2].encode() + b':' in lib.epropnp_last_error(), lib.epropnp_last_error()


def _plan(lib, ca, cb, capacity=None):
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    G = len(ca)
    a, b = (i32 * max(G, 1))(*ca), (i32 * max(G, 1))(*cb)
    nt, no = i64(-1), i64(-1)
    rc = lib.epropnp_box_overlap_plan(a, b, G, None, 0, ctypes.byref(nt), ctypes.byref(no))
    if rc != 0:
        return rc, None, None, None
    cap = nt.value if capacity is None else capacity
    table = (i32 * (6 * max(cap, 1)))(*([-7] * (6 * max(cap, 1))))
    nt2, no2 = i64(-1), i64(-1)
    rc = lib.epropnp_box_overlap_plan(a, b, G, table, cap, ctypes.byref(nt2), ctypes.byref(no2))
    if rc == 0:
        assert (nt2.value, no2.value) == (nt.value, no.value), 'the size query and the fill disagree'
    return rc, nt.value, no.value, [tuple(table[6 * t:6 * t + 6]) for t in range(cap)]


def test_plan_of_the_ragged_counts(lib):
    rc, nt, no, tiles = _plan(lib, COUNTS_A, COUNTS_B)
    assert rc == 0
    want_out = sum(x * y for x, y in zip(COUNTS_A, COUNTS_B))
    want_tiles = sum(((x + 63) // 64) * ((y + 63) // 64) for x, y in zip(COUNTS_A, COUNTS_B) if x and y)
    assert no == want_out == 70 * 65 + 1 + 64 * 130 and nt == want_tiles == 4 + 1 + 3 and len(tiles) == nt
    # every output element is covered exactly once, by a tile inside its segment
    cover = [0] * no
    row0 = col0 = out0 = 0
    seen = 0
    for na, nb in zip(COUNTS_A, COUNTS_B):
        for r, nr, c, nc, o, stride in tiles:
            if row0 <= r < row0 + na and col0 <= c < col0 + nb:
                seen += 1
                assert 1 <= nr <= 64 and 1 <= nc <= 64 and r + nr <= row0 + na and c + nc <= col0 + nb and stride == nb
                assert o == out0 + (r - row0) * nb + (c - col0)
                for i in range(nr):
                    for j in range(nc):
                        cover[o + i * stride + j] += 1
        row0, col0, out0 = row0 + na, col0 + nb, out0 + na * nb
    assert seen == nt and cover == [1] * no
    assert tiles[0] == (3, 64, 0 + 5, 64, 0, 65) and tiles[4] == (73, 1, 70, 1, 70 * 65, 1)
    # the size query alone, with either result pointer missing
    i64 = ctypes.c_int64
    a, b = (ctypes.c_int32 * 6)(*COUNTS_A), (ctypes.c_int32 * 6)(*COUNTS_B)
    only = i64(-1)
    assert lib.epropnp_box_overlap_plan(a, b, 6, None, 0, ctypes.byref(only), None) == 0 and only.value == nt
    assert lib.epropnp_box_overlap_plan(a, b, 6, None, 0, None, ctypes.byref(only)) == 0 and only.value == no
    assert _plan(lib, [], [])[:3] == (0, 0, 0)


def test_plan_validates(lib):
    i32 = ctypes.c_int32
    one = (i32 * 1)(1)
    cases = [lambda: lib.epropnp_box_overlap_plan(one, one, -1, None, 0, None, None),
             lambda: lib.epropnp_box_overlap_plan(None, one, 1, None, 0, None, None),
             lambda: lib.epropnp_box_overlap_plan(one, None, 1, None, 0, None, None),
             lambda: _plan(lib, [3, -1], [2, 2])[0], lambda: _plan(lib, [3, 1], [2, -2])[0],
             lambda: _plan(lib, [1 << 16], [1 << 15])[0],               # exactly 2^31 output elements
             lambda: _plan(lib, [40000, 40000], [40000, 40000])[0],     # ... and summed over the segments
             lambda: _plan(lib, [(1 << 31) - 1, 1], [0, 0])[0],         # 2^31 boxes on a side
             lambda: _plan(lib, COUNTS_A, COUNTS_B, capacity=7)[0]]     # a table one tile short
    for k, bad in enumerate(cases):
        assert bad() == EINVAL, k
        assert NEW[1].encode() + b':' in lib.epropnp_last_error(), lib.epropnp_last_error()
    nt, no = ctypes.c_int64(-1), ctypes.c_int64(-1)                     # just below 2^31: the size query alone
    assert lib.epropnp_box_overlap_plan((i32 * 1)(46341), (i32 * 1)(46340), 1, None, 0, ctypes.byref(nt), ctypes.byref(no)) == 0
    assert no.value == 46341 * 46340 and nt.value == 725 * 725


def test_a_table_entry_out_of_range_is_skipped(backend):
    """the table is memory: entries that point outside the boxes or the output write nothing, the good entry next to them does"""
    from epropnp import _hip, boxes
    a = torch.zeros(70, 5)
    a[:, 0] = torch.arange(70) * 0.25
    a[:, 2:4] = torch.tensor([4.6, 1.9])
    b = a[:66].clone()
    a, b = a.to(backend), b.to(backend)
    num_out = 70 * 66
    good = (64, 6, 64, 2, 64 * 66 + 64, 66)
    bad = [(-1, 6, 0, 2, 0, 66), (65, 6, 0, 2, 0, 66), (0, 65, 0, 2, 0, 66), (0, 0, 0, 2, 0, 66), (0, 6, 65, 2, 0, 66), (0, 6, -2, 2, 0, 66),
           (0, 6, 0, 65, 0, 66), (0, 6, 0, 0, 0, 66), (0, 6, 0, 2, -1, 66), (0, 6, 0, 2, num_out - 5 * 66 - 1, 66), (0, 6, 0, 2, 0, 1),
           (2 ** 31 - 1, 64, 2 ** 31 - 1, 64, 2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 64, -2 ** 31, 64, -2 ** 31, -2 ** 31)]
    tiles = torch.tensor(bad[:6] + [good] + bad[6:], dtype=torch.int32).to(backend)
    out = torch.full((num_out,), -7.0).to(backend)
    _hip.call('epropnp_box_overlap_segmented', _hip.ptr(a), 70, _hip.ptr(b), 66, BEV, IOU, 1, 0.5, INTERVAL, _hip.ptr(tiles),
              tiles.shape[0], _hip.ptr(out), num_out, _hip.stream_of(a))
    out = out.view(70, 66)
    want = boxes.rotated_overlaps(a, b)
    assert torch.equal(out[64:, 64:], want[64:, 64:]) and float(want[64:, 64:].min()) > 0.5
    out[64:, 64:] = -7.0
    assert bool((out == -7.0).all()), 'an entry out of range wrote something'


def test_both_launches_show_up_in_the_stage_recorder(backend):
    from epropnp import _hip, boxes
    b = torch.zeros(3, 7)
    b[:, 0] = torch.arange(3) * 10.0
    b[:, 3:6] = 2.0
    b = b.to(backend)
    _hip.profile(True, reset=True)
    try:
        boxes.box3d_overlaps(b, b)
        boxes.box3d_overlaps(b, b, aligned=True)
        boxes.rotated_overlaps(b[:, [0, 2, 3, 5, 6]].contiguous(), b[:, [0, 2, 3, 5, 6]].contiguous(), 'a')
        boxes.box3d_overlaps(b, b, counts=([1, 2], [2, 1]))
        assert _hip.profile_read('box_overlap')[1] == 3
        assert _hip.profile_read('box_overlap_segmented')[1] == 1
    finally:
        _hip.profile(False, reset=True)
