"""epropnp_posterior_modes is an additive entry of the C ABI: same ABI version, the header is still plain C, and the entry validates
its arguments on the host, naming itself, before anything is launched."""

import pytest

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = 'epropnp_posterior_modes'
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbol_is_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, [NEW])


def test_header_with_the_modes_entry_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, [NEW])


def test_no_objects_is_not_an_error_and_touches_no_pointer(lib):
    assert lib.epropnp_posterior_modes(None, None, None, 64, 0, 4, 3.0, 4, None, None, None, None, None, None, None, None) == 0
    assert lib.epropnp_posterior_modes(1, 1, 1, 64, 0, 6, 3.0, 4, 1, 1, 1, 1, 1, 1, 1, None) == 0      # (pointers that must not be followed)


def test_modes_validates_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    ok = [p, p, p, 64, 3, 6, 3.0, 4, p, p, p, p, p, p, None]
    cases = []
    for k in (0, 1, 2, 8, 9, 10, 11, 12, 13):                                   # each required pointer in turn (mode_poses may be NULL)
        cases.append(ok[:k] + [None] + ok[k + 1:])
    for dof in (5, 0, 7, 3):
        cases.append(ok[:5] + [dof] + ok[6:])
    for S in (0, -2):
        cases.append(ok[:3] + [S] + ok[4:])
    for M in (0, -1):
        cases.append(ok[:7] + [M] + ok[8:])
    for link in (0.0, -1.0, float('inf'), float('nan')):
        cases.append(ok[:6] + [link] + ok[7:])
    cases.append(ok[:4] + [-3] + ok[5:])                                        # num_obj < 0
    for args in cases:
        assert lib.epropnp_posterior_modes(*args, None) == EINVAL, args
        assert NEW.encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
