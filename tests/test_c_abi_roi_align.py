"""epropnp_roi_align_forward / epropnp_roi_align_backward are additive entries of the C ABI: same ABI version, the header is still plain
C, a forward / backward through raw pointers gives the bits of the Python path into buffers that start out as NaN (every element of the
outputs AND of the gradient maps is overwritten: the backward needs no zero fill), and bad arguments come back as EPROPNP_EINVAL."""

import pytest
import torch

import test_roi_align as ta
from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_roi_align_forward', 'epropnp_roi_align_backward')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_roi_align_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW, facts=['EPROPNP_EINVAL == -1'])


def _setup(backend, cl):
    d = ta.reference('small', (3, 2), 0, True)
    fmt = torch.channels_last if cl else torch.contiguous_format
    key = d['map'][:, :5].to(backend).contiguous(memory_format=fmt)
    value = d['map'][:, 5:10].to(backend).contiguous(memory_format=fmt)
    rois = torch.tensor(ta.ROIS, dtype=torch.float32, device=backend)
    cots = [d['cot'][:, s].to(backend).contiguous(memory_format=fmt) for s in (slice(0, 5), slice(5, 10))]
    dims = (len(ta.ROIS), 2, 5, 9, 13, 3, 2)
    strides = ((9 * 13 * 5, 1, 13 * 5, 5) if cl else (5 * 9 * 13, 9 * 13, 13, 1)) + ((3 * 2 * 5, 1, 2 * 5, 5) if cl else (5 * 3 * 2, 3 * 2, 2, 1))
    return key, value, rois, cots, dims, strides, fmt


@pytest.mark.parametrize('cl', [False, True])
def test_raw_pointer_calls_overwrite_nan_buffers_with_the_bits_of_the_python_path(backend, cl):
    from epropnp import _hip, roi
    key, value, rois, cots, dims, strides, fmt = _setup(backend, cl)
    nan = lambda shape: torch.full(shape, float('nan'), device=backend).contiguous(memory_format=fmt)
    k, v = key.clone().requires_grad_(True), value.clone().requires_grad_(True)
    _, want_k, want_v = roi.extract_rois(rois, torch.zeros(2, 2, 4, 4, device=backend), k, v, roi_shape=(3, 2))
    want_gk, want_gv = torch.autograd.grad([want_k, want_v], [k, v], cots)
    tail = (0.25, 0, 1) + strides
    # two maps, then one map with the second pair NULL
    for maps, wants, grads in (((key, value), (want_k, want_v), (want_gk, want_gv)), ((value,), (want_v,), (want_gv,))):
        pad = [None] * (2 - len(maps))
        outs = [nan((8, 5, 3, 2)) for _ in maps]
        _hip.call('epropnp_roi_align_forward', *[_hip.ptr(m) for m in maps], *pad, _hip.ptr(rois), *dims, *tail,
                  *[_hip.ptr(o) for o in outs], *pad, _hip.stream_of(key))
        gmaps = [nan(tuple(key.shape)) for _ in maps]
        use = cots[-len(maps):]
        _hip.call('epropnp_roi_align_backward', *[_hip.ptr(c) for c in use], *pad, _hip.ptr(rois), *dims, *tail,
                  *[_hip.ptr(g) for g in gmaps], *pad, _hip.stream_of(key))
        for got, want in zip(outs + gmaps, wants + grads):
            assert torch.isfinite(got).all(), 'an element was not written'
            assert got.stride() == want.stride() and torch.equal(ta._bits(got), ta._bits(want))
    # no RoI at all: the forward launches nothing, the backward still writes every element (zeros)
    g = nan(tuple(key.shape))
    _hip.call('epropnp_roi_align_backward', None, None, None, 0, *dims[1:], *tail, _hip.ptr(g), None, _hip.stream_of(key))
    assert torch.equal(g, torch.zeros_like(g))


def test_bad_arguments_return_einval(backend):
    from epropnp import _hip
    key, value, rois, cots, dims, strides, _ = _setup(backend, False)
    out, gmap = torch.empty(8, 5, 3, 2, device=backend), torch.empty_like(key)
    L = _hip.lib()
    st = _hip.stream_of(key)

    def fwd(map0=key, map1=None, r=rois, dims=dims, scale=0.25, sampling=0, strides=strides, out0=out, out1=None):
        return L.epropnp_roi_align_forward(_hip.ptr(map0), _hip.ptr(map1), _hip.ptr(r), *dims, scale, sampling, 1, *strides,
                                           _hip.ptr(out0), _hip.ptr(out1), st)

    def bwd(g0=cots[0], g1=None, r=rois, dims=dims, scale=0.25, sampling=0, strides=strides, d0=gmap, d1=None):
        return L.epropnp_roi_align_backward(_hip.ptr(g0), _hip.ptr(g1), _hip.ptr(r), *dims, scale, sampling, 1, *strides,
                                            _hip.ptr(d0), _hip.ptr(d1), st)
    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        assert call(r=None) == EINVAL
        for k in range(7):                                        # a non-positive size (a negative one for num_rois)
            bad = list(dims)
            bad[k] = 0 if k else -1
            assert call(dims=tuple(bad)) == EINVAL, k
        for k in range(8):                                        # a stride of 0, and one whose largest offset leaves the buffer
            for v in (0, strides[k] + 1):
                bad = list(strides)
                bad[k] = v
                assert call(strides=tuple(bad)) == EINVAL, (k, v)
        assert call(sampling=-1) == EINVAL and call(scale=float('inf')) == EINVAL
        assert b'roi_align' in L.epropnp_last_error()
    assert fwd(map0=None) == EINVAL and fwd(out0=None) == EINVAL and fwd(map1=value) == EINVAL and fwd(out1=out) == EINVAL
    assert bwd(g0=None) == EINVAL and bwd(d0=None) == EINVAL and bwd(g1=cots[1]) == EINVAL and bwd(d1=gmap) == EINVAL
