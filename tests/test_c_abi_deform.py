"""epropnp_deform_sample_forward / epropnp_deform_sample_backward are additive entries of the C ABI: same ABI version, the header is
still plain C, and one forward / backward through raw pointers with a strided (channels-last) key gives the bits of the Python path
(dkey / dvalue, float-atomic sums, to rounding)."""

import pytest
import torch

import test_deform as td
from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_deform_sample_forward', 'epropnp_deform_sample_backward')


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_deform_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


def test_raw_pointer_calls_match_the_python_path(backend):
    from epropnp import _hip, deform
    t, stride, cot = td.backward_case('odd')
    B, NI, H, P, D, h, w = td.CASES['odd'][0]
    E = H * D
    q, loc = t['query'].clone().to(backend).requires_grad_(True), t['loc'].clone().to(backend).requires_grad_(True)
    key, value = (td._layout(t[k], 'channels_last', backend).requires_grad_(True) for k in ('key', 'value'))
    x2d, mask, img = t['dense_x2d'].to(backend), t['dense_mask'].to(backend), t['img'].to(backend)
    outs = deform.sample_attend(q, key, value, x2d, mask, loc, img, stride)
    cot = [c.to(backend) for c in cot]
    want = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cot)), (q, key, value, loc), retain_graph=True)
    # the same through the raw entries: the maps as NHWC buffers, described by their element strides
    k_nhwc, v_nhwc = (x.detach().permute(0, 2, 3, 1).contiguous() for x in (key, value))
    strides = (h * w * E, 1, w * E, E)
    fill = lambda *shape: torch.full(shape, -7.0, device=backend)
    attn, vs, a, ms, xs, stats = fill(B, E), fill(B, H, P, D), fill(B, H, P), fill(B, H, P), fill(B, H, P, 2), fill(B, H, 2)
    dims = (B, NI, H, P, D, h, w, stride) + strides
    qd, ld = q.detach(), loc.detach()
    _hip.call('epropnp_deform_sample_forward', _hip.ptr(qd), _hip.ptr(k_nhwc), _hip.ptr(v_nhwc), _hip.ptr(x2d), _hip.ptr(mask), _hip.ptr(ld),
              _hip.ptr(img), *dims, _hip.ptr(attn), _hip.ptr(vs), _hip.ptr(a), _hip.ptr(ms), _hip.ptr(xs), _hip.ptr(stats), _hip.stream_of(qd))
    raw = (attn, vs.transpose(2, 3), a.unsqueeze(2), ms.unsqueeze(2), xs.transpose(2, 3))
    for x, y in zip(raw, outs):
        assert torch.equal(x.contiguous().view(torch.int32), y.detach().contiguous().view(torch.int32))
    g = [cot[0].contiguous(), cot[1].transpose(2, 3).contiguous(), cot[2].squeeze(2).contiguous(), cot[3].squeeze(2).contiguous(),
         cot[4].transpose(2, 3).contiguous()]
    gq, gl, gk, gv = fill(B, H, 1, D), fill(B, H, P, 2), fill(NI, h, w, E), fill(NI, h, w, E)
    _hip.call('epropnp_deform_sample_backward', _hip.ptr(qd), _hip.ptr(k_nhwc), _hip.ptr(v_nhwc), _hip.ptr(x2d), _hip.ptr(mask), _hip.ptr(ld),
              _hip.ptr(img), _hip.ptr(stats), *(_hip.ptr(x) for x in g), *dims, _hip.ptr(gq), _hip.ptr(gk), _hip.ptr(gv), _hip.ptr(gl),
              _hip.stream_of(qd))
    assert torch.equal(gq.view(torch.int32), want[0].contiguous().view(torch.int32))
    assert torch.equal(gl.view(torch.int32), want[3].contiguous().view(torch.int32))
    for x, y in ((gk, want[1]), (gv, want[2])):          # float-atomic sums: equal up to the order of the additions
        assert float((x.permute(0, 3, 1, 2) - y).abs().max()) <= 1e-5 * float(y.abs().max())
    # absent cotangents and unwanted gradients are NULL pointers: only dquery from the cotangent of attn
    gq2 = fill(B, H, 1, D)
    _hip.call('epropnp_deform_sample_backward', _hip.ptr(qd), _hip.ptr(k_nhwc), _hip.ptr(v_nhwc), _hip.ptr(x2d), _hip.ptr(mask), _hip.ptr(ld),
              _hip.ptr(img), _hip.ptr(stats), _hip.ptr(g[0]), None, None, None, None, *dims, _hip.ptr(gq2), None, None, None, _hip.stream_of(qd))
    only = torch.autograd.grad((outs[0] * cot[0]).sum(), q)[0]
    assert torch.equal(gq2.view(torch.int32), only.contiguous().view(torch.int32))
