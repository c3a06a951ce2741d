"""epropnp_pose_errors / epropnp_pose_errors_scratch_bytes are additive entries of the C ABI: same ABI version, the header is still
plain C, and the entry validates its arguments on the host, naming itself, before anything is launched."""

import pytest

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_pose_errors', 'epropnp_pose_errors_scratch_bytes')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_metrics_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW, facts=['EPROPNP_POSE_ERROR_WORDS == 8', 'EPROPNP_POSE_ERROR_QUERY_TILE > 0',
                                                  'EPROPNP_POSE_ERROR_CAND_TILE > 0'])


def test_no_objects_is_not_an_error_and_touches_no_pointer(lib):
    assert lib.epropnp_pose_errors(None, None, 1, 0, 6, None, None, 1, None, None, None, None, None, 0, None, None) == 0
    assert lib.epropnp_pose_errors(1, 1, 3, 0, 4, 1, 1, 2, 1, 1, 1, 1, 1, 64, 1, None) == 0      # (pointers that must not be followed)


def test_pose_errors_validates_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    #     est gt R  B  dof pts rng C  mid cam sym half scratch bytes errors
    ok = [p, p, 2, 3, 6, p, p, 2, p, p, p, p, p, 1 << 20, p]
    cases = []
    for k in (0, 1, 5, 6, 14):                         # each required pointer in turn (model_id, cam_mats and the masks may be NULL)
        cases.append(ok[:k] + [None] + ok[k + 1:])
    cases.append(ok[:12] + [None] + ok[13:])           # no scratch although a symmetric mask is given
    for dof in (5, 0, 7, 3):
        cases.append(ok[:4] + [dof] + ok[5:])
    for R in (0, -2):
        cases.append(ok[:2] + [R] + ok[3:])
    for C in (0, -1):
        cases.append(ok[:7] + [C] + ok[8:])
    cases.append(ok[:3] + [-3] + ok[4:])               # num_obj < 0
    need = lib.epropnp_pose_errors_scratch_bytes(2, 3, 1)
    assert need == 2 * 3 * 4
    for nbytes in (0, need - 1):                       # a scratch smaller than the size query
        cases.append(ok[:13] + [nbytes] + ok[14:])
    for args in cases:
        assert lib.epropnp_pose_errors(*args, None) == EINVAL, args
        assert NEW[0].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_scratch_query_is_monotone(lib):
    from epropnp import metrics
    q = lib.epropnp_pose_errors_scratch_bytes
    assert q(1, 1, 1) == 4 and q(1, 1, metrics.QUERY_TILE) == 4 and q(1, 1, metrics.QUERY_TILE + 1) == 8
    assert q(3, 5, 40000) == 3 * 5 * 4 * ((40000 + metrics.QUERY_TILE - 1) // metrics.QUERY_TILE)
    assert q(1, 0, 100) == 0
    grid = [(r, b, m) for r in (1, 2, 7) for b in (1, 3, 64) for m in (1, 1000, 1024, 1025, 40000)]
    for r, b, m in grid:
        for r2, b2, m2 in grid:
            if r2 >= r and b2 >= b and m2 >= m:
                assert q(r2, b2, m2) >= q(r, b, m)
    assert q(1 << 15, 1 << 15, 1 << 30) == (1 << 30) * 4 * ((1 << 30) // metrics.QUERY_TILE)      # no 32-bit overflow
