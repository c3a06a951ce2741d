"""epropnp_orient_density / epropnp_bev_density and their scratch size queries are additive entries of the C ABI: same ABI version,
the header is still plain C, the entries validate their arguments on the host, naming themselves, before anything is launched, zero
counts follow no pointer, and a call through raw pointers gives the bits of the Python path."""

import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_orient_density', 'epropnp_bev_density', 'epropnp_orient_density_scratch_bytes', 'epropnp_bev_density_scratch_bytes')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_density_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


def test_scratch_queries(lib):
    qo, qb = lib.epropnp_orient_density_scratch_bytes, lib.epropnp_bev_density_scratch_bytes
    assert qo(0, 3) == 0 and qo(4, 0) == 0 and qo(-1, 3) == 0 and qb(4, -2) == 0
    assert qo(512, 32) == 32 * 32 + 512 * 32 * 4 * 4 and qb(512, 600) == 600 * 32 + 512 * 600 * 4 * 2
    assert qo(1 << 20, 1 << 12) == (1 << 12) * 32 + (1 << 32) * 16      # no 32-bit overflow


def test_zero_counts_follow_no_pointer(lib):
    p = 4096      # never followed
    assert lib.epropnp_orient_density(p, p, p, 8, 0, 6, 64, 5, 5, 0.5, 0.6, 50.0, p, 0, p, p, p, p, None) == 0
    assert lib.epropnp_orient_density(None, None, None, 8, 0, 6, 64, 5, 5, 0.5, 0.6, 50.0, None, 0, None, None, None, None, None) == 0
    assert lib.epropnp_bev_density(p, p, p, p, 8, 0, 0, 4, 48, 80, 10.0, 5, 24, 3, p, 0, p, p, None) == 0
    assert lib.epropnp_bev_density(None, None, None, None, 8, 0, 0, 6, 48, 80, 10.0, 5, 24, 3, None, 0, None, None, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    need = lib.epropnp_orient_density_scratch_bytes(8, 2)
    #     pose logw opt S B dof size kh kw sat opac int scratch bytes image front back bins
    ok = [p, p, p, 8, 2, 6, 64, 5, 5, 0.5, 0.6, 50.0, p, need, p, p, p, p]

    def but(**kw):
        names = ['pose', 'logw', 'opt', 'S', 'B', 'dof', 'size', 'kh', 'kw', 'sat', 'opac', 'int', 'scratch', 'bytes', 'image', 'front',
                 'back', 'bins']
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args
    cases = [but(B=-1), but(S=0), but(S=-3), but(dof=4), but(dof=5), but(size=0), but(size=4097), but(kh=4), but(kw=0), but(kw=11),
             but(kh=-1), but(pose=None), but(logw=None), but(scratch=None), but(bytes=need - 1), but(bytes=0),
             but(image=None, front=None, back=None, bins=None)]
    for args in cases:
        assert lib.epropnp_orient_density(*args, None) == EINVAL, args
        assert NEW[0].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
    need = lib.epropnp_bev_density_scratch_bytes(8, 3)
    #     pose logw objw offsets S B G dof H W scale ox oy window scratch bytes density bins
    ok = [p, p, p, p, 8, 3, 2, 4, 48, 80, 10.0, 5, 24, 3, p, need, p, p]
    names = ['pose', 'logw', 'objw', 'offsets', 'S', 'B', 'G', 'dof', 'H', 'W', 'scale', 'ox', 'oy', 'window', 'scratch', 'bytes',
             'density', 'bins']

    def but2(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args
    cases = [but2(B=-1), but2(G=-1), but2(S=0), but2(dof=5), but2(H=0), but2(W=4097), but2(window=2), but2(window=11), but2(window=0),
             but2(pose=None), but2(logw=None), but2(scratch=None), but2(offsets=None), but2(density=None), but2(bytes=need - 1)]
    for args in cases:
        assert lib.epropnp_bev_density(*args, None) == EINVAL, args
        assert NEW[1].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_raw_pointer_calls_match_the_python_path(backend):
    from epropnp import _hip, posterior
    g = torch.Generator().manual_seed(8)
    S, B, size = 70, 3, 40
    q = torch.randn(1, B, 4, generator=g) + 0.4 * torch.randn(S, B, 4, generator=g)
    pose = torch.cat((0.5 * torch.randn(S, B, 3, generator=g), q / q.norm(dim=-1, keepdim=True)), -1).contiguous().to(backend)
    logw = torch.randn(S, B, generator=g).to(backend)
    opt = pose[0].clone()
    want = posterior.orient_density(pose, logw, pose_opt=opt, size=size, window=(3, 5), with_density=True, with_bins=True)
    nbytes = int(_hip.lib().epropnp_orient_density_scratch_bytes(S, B))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=backend)
    image, front, back = (torch.full((B, size, size, 3), -7.0, device=backend) for _ in range(3))
    bins = torch.full((S, B, 3), -7, dtype=torch.int32, device=backend)
    _hip.call('epropnp_orient_density', _hip.ptr(pose), _hip.ptr(logw), _hip.ptr(opt), S, B, 6, size, 3, 5, 0.5, 0.6, 50.0,
              _hip.ptr(scratch), nbytes, _hip.ptr(image), _hip.ptr(front), _hip.ptr(back), _hip.ptr(bins), _hip.stream_of(pose))
    for x, y in zip((image, front, back, bins), want):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the grid: two groups in order, through obj_offsets
    H, W = 20, 33
    score = torch.rand(B, generator=g).to(backend)
    groups = torch.tensor([0, 0, 1], dtype=torch.int32, device=backend)
    want = posterior.bev_density(pose, logw, H, W, scale=6.0, origin=(16, 10), obj_weight=score, groups=groups, num_groups=2, with_bins=True)
    offsets = torch.tensor([0, 2, 3], dtype=torch.int32).to(backend)
    nbytes = int(_hip.lib().epropnp_bev_density_scratch_bytes(S, B))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=backend)
    density = torch.full((2, H, W), -7.0, device=backend)
    bins = torch.full((S, B), -7, dtype=torch.int32, device=backend)
    _hip.call('epropnp_bev_density', _hip.ptr(pose), _hip.ptr(logw), _hip.ptr(score), _hip.ptr(offsets), S, B, 2, 6, H, W, 6.0, 16, 10, 3,
              _hip.ptr(scratch), nbytes, _hip.ptr(density), _hip.ptr(bins), _hip.stream_of(pose))
    assert torch.equal(density.view(torch.int32), want.density.view(torch.int32)) and torch.equal(bins, want.bins)
    assert (want.bins >= 0).any() and float(want.density.sum()) > 0
