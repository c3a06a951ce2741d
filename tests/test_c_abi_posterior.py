"""The posterior additions to the C ABI (epropnp_posterior_summary, epropnp_posterior_resample) are additive: same ABI version, the
header is still plain C, and both entries validate their arguments on the host, naming themselves, before anything is launched."""

import pytest

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_posterior_summary', 'epropnp_posterior_resample')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_posterior_entries_is_plain_c(tmp_path):
    got = check_header_is_plain_c(tmp_path, NEW, run=True, body=['printf("words %d\\n", EPROPNP_POSTERIOR_WORDS);'])
    assert got['words'] == '16'


def test_no_objects_is_not_an_error_and_touches_no_pointer(lib):
    assert lib.epropnp_posterior_summary(None, None, None, 64, 0, 4, None, None) == 0
    assert lib.epropnp_posterior_summary(1, 1, 1, 64, 0, 6, 1, None) == 0            # (pointers that must not be followed)
    assert lib.epropnp_posterior_resample(None, None, 64, 0, 4, 8, None, 0, 0, None, None, None) == 0
    assert lib.epropnp_posterior_resample(1, 1, 64, 0, 6, 8, 1, 0, 0, 1, 1, None) == 0


def test_summary_validates_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    for args in ((None, p, None, 64, 3, 4, p), (p, None, None, 64, 3, 4, p), (p, p, None, 64, 3, 4, None),      # NULL buffers
                 (p, p, None, 64, 3, 5, p), (p, p, None, 64, 3, 0, p), (p, p, None, 64, 3, 7, p),              # dof
                 (p, p, None, 0, 3, 4, p), (p, p, None, -2, 3, 6, p)):                                         # mc_samples
        assert lib.epropnp_posterior_summary(*args, None) == EINVAL, args
        assert b'epropnp_posterior_summary' in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_resample_validates_without_launching(lib):
    p = 4096
    for args in ((None, p, 64, 3, 4, 8, None, 0, 0, p, None), (p, None, 64, 3, 4, 8, None, 0, 0, p, None),
                 (p, p, 64, 3, 4, 8, None, 0, 0, None, p),                                                     # NULL buffers
                 (p, p, 64, 3, 5, 8, None, 0, 0, p, None), (p, p, 64, 3, 3, 8, None, 0, 0, p, None),           # dof
                 (p, p, 0, 3, 4, 8, None, 0, 0, p, None),                                                      # mc_samples
                 (p, p, 64, 3, 4, 0, None, 0, 0, p, None), (p, p, 64, 3, 6, -1, None, 0, 0, p, None)):         # num_draws
        assert lib.epropnp_posterior_resample(*args, None) == EINVAL, args
        assert b'epropnp_posterior_resample' in lib.epropnp_last_error(), lib.epropnp_last_error()
