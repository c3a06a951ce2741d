"""Shared test helpers: golden fixtures, oracle <-> kernel noise layout, problem construction."""
import os

import numpy as np
import torch

import epropnp_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    out = {}
    for k in z.files:
        v = torch.from_numpy(z[k]) if z[k].ndim > 0 else z[k].item()
        if '.' in k:
            a, b = k.split('.', 1)
            out.setdefault(a, {})[b] = v
        else:
            out[k] = v
    return out


def pack_noise(noise, dof):
    """oracle noise dict ((K,s,B,.) tensors) -> kernel layout (B,K,s,stride)."""
    z, chi2 = noise['z'], noise['chi2']
    K, s, B, _ = z.shape
    if dof == 6:
        flat = torch.cat((z, chi2.unsqueeze(-1), noise['g']), -1)                    # (K,s,B,8)
    else:
        T = orc.VM_MAX_TRIES
        tail = torch.zeros(K, s, B, 3 * T, dtype=z.dtype)
        n_u = noise['u'].shape[1]
        tail[:, :n_u, :, 0] = noise['u'][..., 0]
        tail[:, n_u:] = noise['vm'].reshape(K, s - n_u, B, 3 * T)
        flat = torch.cat((z, chi2.unsqueeze(-1), tail), -1)
    return flat.permute(2, 0, 1, 3).contiguous().float()


def to_dev(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def make_layer_objects(prob, device, relative_delta=None):
    """reference-API camera / cost_fun objects for a problem dict (from a fixture or orc.make_problem)."""
    from epropnp.camera import PerspectiveCamera
    from epropnp.cost_fun import AdaptiveHuberPnPCost, HuberPnPCost
    p = to_dev(prob, device)
    cam = PerspectiveCamera(cam_mats=p['cam_mats'], z_min=float(p.get('z_min', 0.1)), lb=p.get('lb'), ub=p.get('ub'))
    if relative_delta is None:
        cf = HuberPnPCost(delta=p['delta'])
    else:
        cf = AdaptiveHuberPnPCost(relative_delta=relative_delta)
    return p, cam, cf


CAMERA_KINDS = ('per_object', 'skewed', 'full')


def vary_cameras(prob, kind, seed):
    """A copy of an `orc.make_problem` dict in which every object has its own camera matrix (make_problem expands ONE
    matrix over the batch; its random stream is not touched: the draws here come from a generator of their own).

      'per_object'  fx, fy independent in [500, 1400], cx in [200, 900], cy in [150, 500], third row (0, 0, 1)
      'skewed'      + K[0,1] in +-30, K[1,0] in +-20, fx negated (horizontal flip) for every second object
      'full'        + K[2,0], K[2,1] in +-0.05 (a rectifying homography), the whole matrix times its own factor in [0.5, 2.5]

    x2d is re-projected in fp64 from x3d and pose_gt through the new matrices and keeps the pixel noise make_problem drew (what
    x2d was off its own noise-free projection by); delta is recomputed; bounds, where the input has them, become the 5 % / 95 %
    quantiles of each object's own x2d (about 10 % of the points clipped per axis: a fixed box under wandering principal
    points clips most points, whose zero Jacobians leave the normal equations near-singular)."""
    assert kind in CAMERA_KINDS, kind
    g = torch.Generator().manual_seed(seed)
    dtype = prob['x2d'].dtype
    B = prob['x2d'].shape[0]
    uni = lambda lo, hi: lo + (hi - lo) * torch.rand(B, generator=g, dtype=torch.float64)
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 0], K[:, 1, 1] = uni(500, 1400), uni(500, 1400)
    K[:, 0, 2], K[:, 1, 2] = uni(200, 900), uni(150, 500)
    K[:, 2, 2] = 1.0
    if kind in ('skewed', 'full'):
        K[:, 0, 1], K[:, 1, 0] = uni(-30, 30), uni(-20, 20)
        K[1::2, 0, 0] *= -1.0
    if kind == 'full':
        K[:, 2, 0], K[:, 2, 1] = uni(-0.05, 0.05), uni(-0.05, 0.05)
        K *= uni(0.5, 2.5).reshape(B, 1, 1)
    x3d, pose_gt = prob['x3d'].double(), prob['pose_gt'].double()
    px_noise = prob['x2d'].double() - orc.evaluate_project(x3d, pose_gt, orc.Cam(prob['cam_mats'].double(), 0.1))
    out = dict(prob)
    out['cam_mats'] = K.to(dtype).contiguous()
    out['x2d'] = (orc.evaluate_project(x3d, pose_gt, orc.Cam(K, 0.1)) + px_noise).to(dtype)
    out['delta'] = orc.adaptive_huber_delta(out['x2d'], out['w2d'], 0.5)
    if 'lb' in prob:
        q = torch.quantile(out['x2d'].double(), torch.tensor([0.05, 0.95], dtype=torch.float64), dim=1)      # (2,B,2)
        out['lb'], out['ub'] = q[0].to(dtype).contiguous(), q[1].to(dtype).contiguous()
    for k in ('cam_mats', 'lb', 'ub'):
        if k in out:
            flat = out[k].reshape(B, -1)
            same = (flat.unsqueeze(0) == flat.unsqueeze(1)).all(-1) & ~torch.eye(B, dtype=torch.bool)
            assert not bool(same.any()), f'{k}: two objects share a value'
    return out


def assert_within_spread(err, spread, bar, k=2.0, what=''):
    """Parity bar with the reference's own rounding sensitivity as the yardstick, compared as ORDER STATISTICS over the
    objects of the batch: the i-th largest error must not exceed `bar + k x` the i-th largest spread.

    `spread` (orc.rounding_spread / the fixtures' `spread.*`) is how far the reference's own fp32 result moves per object
    when its inputs move by <= 3 ulp (plus its fp32-vs-fp64 drift).  It is ~0 for well-conditioned objects and large
    where a trust-region decision sits on a knife edge or the LM valley is flat -- but WHICH object of a batch trips
    depends on the individual roundings, so errors and spreads are matched by rank, not by object index.  HOW MANY trip
    is a count of rare independent events: if `n_trip` objects have a spread above the bar, two correct implementations
    differ in that count by ~sqrt(2 n_trip), so the error of rank i is held against the spread of rank
    i - (1 + ceil(sqrt(2 n_trip))); with no such object (n_trip = 0) the match is strict."""
    import math
    e = torch.sort(err.detach().flatten().double().cpu(), descending=True).values
    s = torch.sort(spread.detach().flatten().double().cpu(), descending=True).values
    assert e.numel() == s.numel(), (e.shape, s.shape)
    n_trip = int((s > bar).sum())
    slack = 0 if n_trip == 0 else 1 + math.ceil(math.sqrt(2 * n_trip))
    idx = (torch.arange(e.numel()) - slack).clamp(min=0)
    lim = bar + k * s[idx]
    bad = e > lim
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {e.numel()} order statistics above bar {bar:g} + {k:g} x spread '
                                 f'(rank slack {slack}); worst: err {e[bad][0].item():.3e} vs limit {lim[bad][0].item():.3e} '
                                 f'(rank {int(bad.nonzero()[0])})')

def rel_per_object(a, b):
    """max |a - b| over an object's entries relative to the object's largest |b| -> (B,)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs().reshape(a.shape[0], -1).amax(1)
    return d / b.abs().reshape(b.shape[0], -1).amax(1).clamp(min=1e-30)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'epro-pnp_amd', 'lib', 'libepropnp_hip.so')


def abi_lib():
    """A private handle of the in-tree library, built first if it is missing, with every function's argtypes and restype from the
    binding's one signature table (epropnp/_hip.py: SIGNATURES, held against the header by tests/test_c_abi.py)."""
    import ctypes
    if not os.path.exists(LIB):
        import importlib.util
        spec = importlib.util.spec_from_file_location('epropnp_build', os.path.join(ROOT, 'epro-pnp_amd', 'build.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    from epropnp import _hip
    return _hip._declare(ctypes.CDLL(LIB))


def check_abi_additive(lib, names):
    """`names` are exported by the library and listed by the binding, and the ABI version stays 7 in both."""
    from epropnp import _hip
    assert lib.epropnp_abi_version() == 7 and _hip.ABI_VERSION == 7
    for name in names:
        assert hasattr(lib, name), f'{name} not exported'
        assert name in _hip.EXPORTS


def check_header_is_plain_c(tmp_path, names, facts=(), body=(), run=False):
    """include/epropnp_hip.h with a program that takes the address of every function of `names` passes gcc -std=c99 -Wall -Wextra
    -pedantic -Werror and g++ -std=c++11 -Wall -Werror; EPROPNP_ABI_VERSION == 7 and every C constant expression of `facts` hold
    at compile time (an array of size -1 otherwise).  `body`: further statements of main.  run: also link the program against the
    library, run it and return its output as a dict of the first word of each line to the second (`name 1` per function)."""
    import shutil
    import subprocess
    import pytest
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "epropnp_hip.h"']
    lines += [f'typedef char fact_{i}[({fact}) ? 1 : -1];' for i, fact in enumerate(['EPROPNP_ABI_VERSION == 7', *facts])]
    lines += ['int main(void) {'] + [f'  printf("{n} %d\\n", (int)(sizeof(&{n}) > 0));' for n in names]
    lines += [f'  {stmt}' for stmt in body] + ['  return 0;', '}']
    src = tmp_path / 'abi_entries.c'
    src.write_text('\n'.join(lines) + '\n')
    inc = os.path.join(ROOT, 'include')
    for cmd in (['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror'], ['g++', '-std=c++11', '-Wall', '-Werror', '-x', 'c++']):
        r = subprocess.run(cmd + ['-I', inc, '-fsyntax-only', str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if not run:
        return None
    abi_lib()
    exe, libdir = tmp_path / 'abi_entries', os.path.dirname(LIB)
    r = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Werror', '-I', inc, str(src), '-o', str(exe), '-L', libdir, '-lepropnp_hip',
                        '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-L', '/opt/rocm/lib'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = dict(line.split() for line in out.stdout.splitlines())
    assert all(got[n] == '1' for n in names)
    return got


def set_tune(monkeypatch, **keys):
    """EPROPNP_TUNE (csrc/pnp_host.h: tune_value, epropnp/_hip.py: tune) from keyword arguments: `bwd_impl='valu'`, `bwd_mfma='4,2'`,
    a bare flag as `rslm_composite=True`; no keys (or only None / False values) removes the variable."""
    items = [k if v is True else f'{k}={v}' for k, v in keys.items() if v is not None and v is not False]
    if items:
        monkeypatch.setenv('EPROPNP_TUNE', ';'.join(items))
    else:
        monkeypatch.delenv('EPROPNP_TUNE', raising=False)
