"""epropnp_roi_logsumexp_forward / epropnp_roi_logsumexp_backward are additive entries of the C ABI: same ABI version, the header is
still plain C, and one forward / backward through raw pointers gives the bits of the Python path."""

import pytest
import torch

import test_roi as tr
from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_roi_logsumexp_forward', 'epropnp_roi_logsumexp_backward')


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_roi_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


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
