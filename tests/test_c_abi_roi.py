"""epropnp_roi_logsumexp_forward / epropnp_roi_logsumexp_backward are additive entries of the C ABI: same ABI version, the header is
still plain C, and one forward / backward through raw pointers gives the bits of the Python path."""
import ctypes
import os
import subprocess

import pytest
import torch

import test_roi as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'epro-pnp_amd', 'lib', 'libepropnp_hip.so')
NEW = ('epropnp_roi_logsumexp_forward', 'epropnp_roi_logsumexp_backward')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        import importlib.util
        spec = importlib.util.spec_from_file_location('epropnp_build', os.path.join(ROOT, 'epro-pnp_amd', 'build.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    return ctypes.CDLL(LIB)


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    from epropnp import _hip
    assert lib.epropnp_abi_version() == 7 and _hip.ABI_VERSION == 7
    for name in NEW:
        assert hasattr(lib, name), f'{name} not exported'
        assert name in _hip.EXPORTS


def test_header_with_the_roi_entries_is_plain_c(tmp_path):
    src = tmp_path / 'roi.c'
    src.write_text('#include <stdio.h>\n#include "epropnp_hip.h"\nint main(void) {\n'
                   + ''.join(f'  printf("%d\\n", (int)(sizeof(&{n}) > 0));\n' for n in NEW)
                   + '  return EPROPNP_ABI_VERSION == 7 ? 0 : 1;\n}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                        '-fsyntax-only', str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_raw_pointer_calls_match_the_python_path(backend):
    from epropnp import _hip, roi
    d = tr.case('odd')
    n, c, rh, rw = d['x'].shape
    x = d['x'].clone().to(backend).requires_grad_(True)
    rois, cot = d['rois'].to(backend), d['cot'].to(backend)
    out = roi.logsumexp_across_rois(x, rois)
    want = torch.autograd.grad((out * cot).sum(), x)[0]
    fill = lambda: torch.full((n, c, rh, rw), -7.0, device=backend)
    raw_out, raw_grad = fill(), fill()
    xd = x.detach()
    _hip.call('epropnp_roi_logsumexp_forward', _hip.ptr(xd), _hip.ptr(rois), n, c, rh, rw, _hip.ptr(raw_out), _hip.stream_of(xd))
    assert torch.equal(raw_out.view(torch.int32), out.detach().view(torch.int32))
    _hip.call('epropnp_roi_logsumexp_backward', _hip.ptr(xd), _hip.ptr(rois), _hip.ptr(raw_out), _hip.ptr(cot), n, c, rh, rw,
              _hip.ptr(raw_grad), _hip.stream_of(xd))
    assert torch.equal(raw_grad.view(torch.int32), want.view(torch.int32))
