"""The posterior additions to the C ABI (epropnp_posterior_summary, epropnp_posterior_resample) are additive: same ABI version, the
header is still plain C, and both entries validate their arguments on the host, naming themselves, before anything is launched."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'epro-pnp_amd', 'lib', 'libepropnp_hip.so')
NEW = ('epropnp_posterior_summary', 'epropnp_posterior_resample')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        import importlib.util
        spec = importlib.util.spec_from_file_location('epropnp_build', os.path.join(ROOT, 'epro-pnp_amd', 'build.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    handle = ctypes.CDLL(LIB)
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    handle.epropnp_last_error.restype = ctypes.c_char_p
    handle.epropnp_posterior_summary.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    handle.epropnp_posterior_resample.argtypes = [vp, vp, i32, i32, i32, i32, vp, u64, u64, vp, vp, vp]
    return handle


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    from epropnp import _hip
    assert lib.epropnp_abi_version() == 7 and _hip.ABI_VERSION == 7
    for s in NEW:
        assert hasattr(lib, s), f'{s} not exported'
        assert s in _hip.EXPORTS


def test_header_with_the_posterior_entries_is_plain_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    lines = ['#include <stdio.h>', '#include "epropnp_hip.h"', 'int main(void) {',
             '  printf("words %d\\n", EPROPNP_POSTERIOR_WORDS);']
    lines += [f'  printf("{s} %d\\n", (int)(sizeof(&{s}) > 0));' for s in NEW] + ['  return 0;', '}']      # (the symbols must link)
    src = tmp_path / 'posterior.c'
    src.write_text('\n'.join(lines) + '\n')
    inc = os.path.join(ROOT, 'include')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', inc, '-fsyntax-only', str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / 'posterior'
    libdir = os.path.dirname(LIB)
    r = subprocess.run(['gcc', '-std=c99', '-I', inc, str(src), '-o', str(exe), '-L', libdir, '-lepropnp_hip',
                        '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-L', '/opt/rocm/lib'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = dict(line.split() for line in out.stdout.splitlines())
    assert got['words'] == '16' and all(got[s] == '1' for s in NEW)


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
