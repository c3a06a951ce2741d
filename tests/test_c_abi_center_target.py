"""epropnp_volume_centers / epropnp_box_thickness and the scratch size query are additive entries of the C ABI: same ABI version, the
header is still plain C, the entries validate their arguments on the host, naming themselves, before anything is launched, zero
objects follow no pointer, and a call through raw pointers gives the bits of the Python path."""

import numpy as np
import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

NEW = ('epropnp_volume_centers', 'epropnp_box_thickness', 'epropnp_volume_centers_scratch_bytes')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_centre_target_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


def test_scratch_query(lib):
    q = lib.epropnp_volume_centers_scratch_bytes
    assert q(0, 24, 40) == 0 and q(-1, 24, 40) == 0 and q(5, -1, 40) == 0 and q(5, 24, 4097) == 0
    assert q(9, 0, 0) == 9 * 64                              # the table alone: what epropnp_box_thickness asks for
    assert q(9, 24, 40) == 9 * 64 + 2 * 3 * 9 * 40           # 16 x 16 tiles: 2 x 3
    assert q(192, 232, 400) == 192 * 64 + 15 * 25 * 192 * 40
    assert q(1 << 20, 4096, 4096) == (1 << 20) * 64 + 256 * 256 * (1 << 20) * 40      # no 32-bit overflow


def test_zero_objects_follow_no_pointer(lib):
    p = 4096      # never followed
    for a in (p, None):
        assert lib.epropnp_volume_centers(a, a, a, a, a, a, 0, 3, 24, 40, 24, 40, 4, 4, 16, 1e-2, 4.0, 1, a, 0, a, a, a, None) == 0
        assert lib.epropnp_volume_centers(a, a, a, a, a, a, 0, 0, 24, 40, 24, 40, 4, 4, 0, 1e-2, 4.0, 0, a, 0, a, a, a, None) == 0
        assert lib.epropnp_box_thickness(a, a, a, 0, 3, 24, 40, 4, 16, 1e-2, a, 0, a, a, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    need = lib.epropnp_volume_centers_scratch_bytes(5, 24, 40)
    names = ['b3', 'b2', 'off', 'cam', 'x2d', 'mask', 'B', 'G', 'h', 'w', 'Hr', 'Wr', 'os', 'rs', 'K', 'zc', 'minbox', 'getbox',
             'scratch', 'bytes', 'centers', 'boxes', 'valid']
    ok = [p, p, p, p, p, p, 5, 2, 24, 40, 24, 40, 4, 4, 16, 1e-2, 4.0, 0, p, need, p, p, p]

    def but(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args
    cases = [but(B=-1), but(G=-1), but(G=0), but(G=65536), but(h=0), but(w=4097), but(Hr=0), but(Wr=4097), but(Hr=-4), but(os=0),
             but(rs=0), but(rs=-2), but(K=1), but(K=-1), but(zc=-1.0), but(b3=None), but(b2=None), but(off=None), but(cam=None),
             but(x2d=None), but(mask=None), but(scratch=None), but(bytes=need - 1), but(bytes=0), but(centers=None), but(boxes=None),
             but(valid=None)]
    for args in cases:
        assert lib.epropnp_volume_centers(*args, None) == EINVAL, args
        assert NEW[0].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
    need = lib.epropnp_volume_centers_scratch_bytes(5, 0, 0)
    names = ['b3', 'off', 'cam', 'B', 'G', 'Hr', 'Wr', 'rs', 'K', 'zc', 'scratch', 'bytes', 'thick', 'valid']
    ok = [p, p, p, 5, 2, 24, 40, 4, 16, 1e-2, p, need, p, p]
    cases = [but(B=-1), but(B=65536), but(G=-1), but(G=0), but(Hr=0), but(Wr=4097), but(rs=0), but(K=1), but(K=-3), but(zc=-0.5),
             but(b3=None), but(off=None), but(cam=None), but(scratch=None), but(bytes=need - 1), but(thick=None), but(valid=None)]
    for args in cases:
        assert lib.epropnp_box_thickness(*args, None) == EINVAL, args
        assert NEW[1].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_raw_pointer_calls_match_the_python_path(backend):
    from epropnp import _hip, targets
    import test_center_target as tc
    boxes, inds, cams = tc.scene_main()
    x2d, mask = tc.x2d_maps('crop', 3, 24, 40, 4)
    b3, cam, xs, ms = (tc.dev(a, backend) for a in (boxes, cams, x2d, mask))
    want = targets.volume_centers(b3, tc.dev(inds, backend), cam, xs, ms, (96, 160), get_bbox_2d=True, faces_per_pixel=None)
    offsets = torch.tensor([0, 4, 4, 9], dtype=torch.int32).to(backend)
    B = len(boxes)
    nbytes = int(_hip.lib().epropnp_volume_centers_scratch_bytes(B, 24, 40))
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=backend)
    centers, box2d = torch.full((B, 2), -7.0, device=backend), torch.full((B, 4), -7.0, device=backend)
    valid = torch.full((B,), 9, dtype=torch.uint8, device=backend)
    _hip.call('epropnp_volume_centers', _hip.ptr(b3), None, _hip.ptr(offsets), _hip.ptr(cam), _hip.ptr(xs), _hip.ptr(ms), B, 3, 24, 40,
              24, 40, 4, 4, 0, 1e-2, 4.0, 1, _hip.ptr(scratch), nbytes, _hip.ptr(centers), _hip.ptr(box2d), _hip.ptr(valid),
              _hip.stream_of(b3))
    assert torch.equal(centers.view(torch.int32), want[0].view(torch.int32)) and torch.equal(box2d, want[1])
    assert torch.equal(valid, want[2].to(torch.uint8)) and bool(want[2].any()) and not bool(want[2].all())
    # offsets that leave an object out: it is invalid, the others are what they were
    offsets = torch.tensor([0, 4, 4, 8], dtype=torch.int32).to(backend)
    _hip.call('epropnp_volume_centers', _hip.ptr(b3), None, _hip.ptr(offsets), _hip.ptr(cam), _hip.ptr(xs), _hip.ptr(ms), B, 3, 24, 40,
              24, 40, 4, 4, 0, 1e-2, 4.0, 1, _hip.ptr(scratch), nbytes, _hip.ptr(centers), _hip.ptr(box2d), _hip.ptr(valid),
              _hip.stream_of(b3))
    assert int(valid[8]) == 0 and centers[8].tolist() == [0.0, 0.0] and torch.equal(centers[:8], want[0][:8])
    thick, tv = targets.box_thickness(b3, tc.dev(inds, backend), cam, (96, 160))
    nbytes = int(_hip.lib().epropnp_volume_centers_scratch_bytes(B, 0, 0))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=backend)
    t2, v2 = torch.full((B, 24, 40), -7.0, device=backend), torch.full((B, 24, 40), 9, dtype=torch.uint8, device=backend)
    offsets = torch.tensor([0, 4, 4, 9], dtype=torch.int32).to(backend)
    _hip.call('epropnp_box_thickness', _hip.ptr(b3), _hip.ptr(offsets), _hip.ptr(cam), B, 3, 24, 40, 4, 16, 1e-2, _hip.ptr(scratch),
              nbytes, _hip.ptr(t2), _hip.ptr(v2), _hip.stream_of(b3))
    assert torch.equal(t2.view(torch.int32), thick.view(torch.int32)) and torch.equal(v2, tv.to(torch.uint8)) and float(thick.sum()) > 0
    assert np.isfinite(thick.cpu().numpy()).all()
