"""epropnp_point_targets / epropnp_obj_sample_weights are additive entries of the C ABI: same ABI version, the header is still plain C,
the entries validate their arguments on the host, naming themselves, before anything is launched, empty calls follow no pointer, and
a call through raw pointers gives the bits of the Python path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import abi_lib, check_abi_additive, check_header_is_plain_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('epropnp_point_targets', 'epropnp_obj_sample_weights')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


def host(ctype, values):
    arr = (ctype * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    check_abi_additive(lib, NEW)


def test_header_with_the_point_target_entries_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, NEW)


def test_python_constants_follow_the_sources():
    from epropnp import targets
    tuning = open(os.path.join(ROOT, 'epro-pnp_amd', 'csrc', 'tuning.h')).read()
    assert int(re.search(r'#define PNP_PT_CHUNK (\d+)', tuning).group(1)) == targets.POINT_TARGET_CHUNK
    unit = open(os.path.join(ROOT, 'epro-pnp_amd', 'csrc', 'point_target_kernels.hip')).read()
    assert int(re.search(r'kOsMaxN = (\d+)', unit).group(1)) == targets.MAX_OBJ_SAMPLES


def test_empty_calls_follow_no_pointer(lib):
    p = 4096      # never followed
    for a in (p, None):
        assert lib.epropnp_point_targets(a, a, a, a, a, a, 3, a, a, a, a, 0, 5, 2, 3, 2.5, a, a, a, a, a, None) == 0
        assert lib.epropnp_point_targets(a, a, a, a, a, a, 3, a, a, a, a, 315, 0, 0, 3, 2.5, a, a, a, a, a, None) == 0
        assert lib.epropnp_obj_sample_weights(a, a, a, 100, a, 0, 0, 1e-5, a, a, a, a, None) == 0


def test_entries_validate_without_launching(lib):
    p = 4096      # never followed: every call below fails its host-side checks
    keep = []

    def h(ctype, values):
        arr, ptr = host(ctype, values)
        keep.append(arr)
        return ptr
    names = ['points', 'lvl', 'radius', 'lo', 'hi', 'sv', 'L', 'boxes', 'centers', 'gt_labels', 'img_off', 'P', 'G', 'num_img',
             'classes', 'alpha', 'labels', 'cen', 'gt_inds', 'strides', 'num_fg']
    i32, f32, i64 = ctypes.c_int32, ctypes.c_float, ctypes.c_int64
    ok = [p, h(i32, [0, 240, 300, 315]), h(f32, [12, 24, 48]), h(f32, [-1, 24, 48]), h(f32, [24, 48, 1e8]), h(i64, [8, 16, 32]), 3,
          p, p, p, p, 315, 9, 3, 3, 2.5, p, p, p, p, p]

    def but(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args
    nan = float('nan')
    cases = [but(P=-1), but(G=-1), but(num_img=-1), but(num_img=65536), but(L=0), but(L=9), but(classes=-1), but(alpha=nan),
             but(lvl=None), but(radius=None), but(lo=None), but(hi=None), but(lvl=h(i32, [1, 240, 300, 315])),
             but(lvl=h(i32, [0, 240, 300, 314])), but(lvl=h(i32, [0, 301, 300, 315])), but(radius=h(f32, [12, 0, 48])),
             but(radius=h(f32, [12, nan, 48])), but(lo=h(f32, [-1, nan, 48])), but(hi=h(f32, [24, 48, nan])), but(sv=None),
             but(points=None), but(img_off=None), but(labels=None), but(cen=None), but(gt_inds=None), but(num_fg=None),
             but(boxes=None), but(centers=None), but(gt_labels=None)]
    for args in cases:
        assert lib.epropnp_point_targets(*args, None) == EINVAL, args
        assert NEW[0].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
    for bad, word in ((but(lvl=None), b'lvl_offsets'), (but(radius=h(f32, [12, 0, 48])), b'radius_px'), (but(L=9), b'num_levels'),
                      (but(num_img=65536), b'num_img'), (but(sv=None), b'level_strides')):
        assert lib.epropnp_point_targets(*bad, None) == EINVAL and word in lib.epropnp_last_error(), lib.epropnp_last_error()
    names = ['fg', 'cen', 'gt', 'T', 'draws', 'N', 'nu', 'eps', 'sgt', 'sw', 'suw', 'num_fg']
    ok = [p, p, p, 945, p, 24, 12, 1e-5, p, p, p, p]
    cases = [but(T=-1), but(N=-1), but(N=2049), but(nu=-1), but(nu=25), but(eps=0.0), but(eps=nan), but(T=0), but(fg=None),
             but(cen=None), but(gt=None), but(draws=None), but(sgt=None), but(sw=None), but(suw=None)]
    for args in cases:
        assert lib.epropnp_obj_sample_weights(*args, None) == EINVAL, args
        assert NEW[1].encode() in lib.epropnp_last_error(), lib.epropnp_last_error()
    for bad, word in ((but(N=2049), b'num_obj_samples'), (but(nu=25), b'num_uniform'), (but(eps=0.0), b'eps')):
        assert lib.epropnp_obj_sample_weights(*bad, None) == EINVAL and word in lib.epropnp_last_error(), lib.epropnp_last_error()


def test_raw_pointer_calls_match_the_python_path(backend):
    from epropnp import _hip, targets
    import test_point_targets as tp
    pts, counts, boxes, labels, centres, img, num_img = tp.oracle('main')['inputs']
    want = tp.run('main', backend, with_strides=True)
    P, G, total = len(pts), len(boxes), num_img * len(pts)
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    p_, b_, l_, c_ = d(pts), d(boxes), d(labels), d(centres)
    offsets = torch.tensor([0, 5, 5, 9], dtype=torch.int32).to(backend)
    out_l, out_g, out_s = (torch.full((total,), -1, dtype=torch.int64, device=backend) for _ in range(3))
    out_c = torch.full((total,), float('nan'), device=backend)
    num_fg = torch.full((1,), -1, dtype=torch.int32, device=backend)
    keep = [host(ctypes.c_int32, [0, counts[0], counts[0] + counts[1], P]), host(ctypes.c_float, [12, 24, 48]),
            host(ctypes.c_float, [-1, 24, 48]), host(ctypes.c_float, [24, 48, 1e8]), host(ctypes.c_int64, [8, 16, 32])]
    _hip.call('epropnp_point_targets', _hip.ptr(p_), *[k[1] for k in keep], 3, _hip.ptr(b_), _hip.ptr(c_), _hip.ptr(l_),
              _hip.ptr(offsets), P, G, num_img, tp.NUM_CLASSES, tp.ALPHA, _hip.ptr(out_l), _hip.ptr(out_c), _hip.ptr(out_g),
              _hip.ptr(out_s), _hip.ptr(num_fg), _hip.stream_of(p_))
    for got, exp in zip((out_l, out_c, out_g, out_s, num_fg), want):
        assert torch.equal(tp.bits(got), tp.bits(exp))
    assert int(num_fg.item()) > 0 and np.isfinite(out_c.cpu().numpy()).all()
    # offsets that leave the last object out: the points it owned go elsewhere, nothing is read beyond the objects
    offsets = torch.tensor([0, 5, 5, 8], dtype=torch.int32).to(backend)
    _hip.call('epropnp_point_targets', _hip.ptr(p_), *[k[1] for k in keep], 3, _hip.ptr(b_), _hip.ptr(c_), _hip.ptr(l_),
              _hip.ptr(offsets), P, G, num_img, tp.NUM_CLASSES, tp.ALPHA, _hip.ptr(out_l), _hip.ptr(out_c), _hip.ptr(out_g),
              None, _hip.ptr(num_fg), _hip.stream_of(p_))
    assert int(out_g.max()) == 6 and int(num_fg.item()) < int(want[4].item())
    # the sampler: the draws of the Python path through raw pointers, the foreground count as an extra output
    fg = want[0] < tp.NUM_CLASSES
    T, N = total, 24
    draws = torch.nonzero(fg)[:, 0][torch.arange(N, device=backend) * 2 % int(fg.sum())].contiguous()
    exp = targets.obj_sampler(N, fg, want[1], want[2], sample_point_inds=draws)
    sgt = torch.full((N,), -1, dtype=torch.int64, device=backend)
    sw, suw = torch.full((N,), float('nan'), device=backend), torch.full((N,), float('nan'), device=backend)
    count = torch.full((1,), -1, dtype=torch.int32, device=backend)
    _hip.call('epropnp_obj_sample_weights', _hip.ptr(fg.view(torch.uint8)), _hip.ptr(want[1]), _hip.ptr(want[2]), T, _hip.ptr(draws), N, 12,
              1e-5, _hip.ptr(sgt), _hip.ptr(sw), _hip.ptr(suw), _hip.ptr(count), _hip.stream_of(fg))
    for got, e in zip((sgt, sw, suw), exp):
        assert torch.equal(tp.bits(got), tp.bits(e))
    assert int(count.item()) == int(fg.sum()) == int(want[4].item())
