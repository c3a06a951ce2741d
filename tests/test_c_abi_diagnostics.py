"""The diagnostics additions to the C ABI (epropnp_diag, epropnp_monte_carlo_forward_diag, epropnp_rslm_solve_diag,
epropnp_weight_stats) are additive: same ABI version, the header is still plain C, the struct matches its ctypes mirror, and the
new forward entry without a diag is the old one."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'epro-pnp_amd', 'lib', 'libepropnp_hip.so')
NEW = ('epropnp_monte_carlo_forward_diag', 'epropnp_rslm_solve_diag', 'epropnp_weight_stats')


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
    for s in NEW:
        assert hasattr(lib, s), f'{s} not exported'
        assert s in _hip.EXPORTS


def test_header_with_the_diag_struct_is_plain_c_and_matches_ctypes(tmp_path):
    from epropnp import _hip
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    fields = [f for f, _ in _hip.Diag._fields_]
    assert fields == ['lm_accept_mask', 'rslm_winner', 'proposals', 'weight_stats']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "epropnp_hip.h"', 'int main(void) {',
             '  epropnp_diag d = {0, 0, 0, 0};',
             '  printf("size %zu\\n", sizeof(d));']
    lines += [f'  printf("{f} %zu\\n", offsetof(epropnp_diag, {f}));' for f in fields]
    lines += [f'  printf("{s} %d\\n", (int)(sizeof(&{s}) > 0));' for s in NEW] + ['  return 0;', '}']      # (the symbols must link)
    src = tmp_path / 'diag.c'
    src.write_text('\n'.join(lines) + '\n')
    inc = os.path.join(ROOT, 'include')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', inc, '-fsyntax-only', str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / 'diag'
    libdir = os.path.dirname(LIB)
    r = subprocess.run(['gcc', '-std=c99', '-I', inc, str(src), '-o', str(exe), '-L', libdir, '-lepropnp_hip',
                        '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-L', '/opt/rocm/lib'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = dict(line.split() for line in out.stdout.splitlines())
    assert all(got[s] == '1' for s in NEW)
    assert int(got['size']) == ctypes.sizeof(_hip.Diag)
    for f in fields:
        assert int(got[f]) == getattr(_hip.Diag, f).offset, f


def test_weight_stats_validates_without_launching(lib):
    lib.epropnp_last_error.restype = ctypes.c_char_p
    lib.epropnp_weight_stats.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.epropnp_weight_stats(None, 64, 0, 4, None, None) == 0            # no objects: nothing to do
    assert lib.epropnp_weight_stats(None, 64, 3, 4, None, None) == -1 and b'NULL' in lib.epropnp_last_error()


@pytest.mark.parametrize('how', ['null', 'empty'])
def test_forward_diag_without_a_diag_is_the_plain_entry(backend, monkeypatch, poisoned_empty, how):
    """epropnp_monte_carlo_forward_diag with diag = NULL (and with a struct of NULLs) returns the bits of epropnp_monte_carlo_forward:
    the package's plain call is routed through it from the outside."""
    from epropnp import _hip
    from epropnp.epropnp import EProPnP4DoF
    from epropnp.levenberg_marquardt import LMSolver, RSLMSolver
    B, N, S, K = 5, 70, 32, 2
    prob = orc.make_problem(B, N, 4, seed=3, bounds='tensor')
    prob['pose_init'][0, :3] += 3.0
    noise = pack_noise(orc.make_noise(B, S, K, 4, seed=4), 4).to(backend)
    rn = orc.make_rslm_noise(prob, 4, 8, 16, seed=5)
    # the ctypes node, whose host call can be re-routed from here (a C++ node loaded earlier in the process stays cached whatever
    # EPROPNP_NO_TORCH_EXT says now)
    monkeypatch.setattr(_hip, 'torch_ext', lambda: None)
    real_call, routed = _hip.call, []

    def via_diag(name, *args):
        if name != 'epropnp_monte_carlo_forward':
            return real_call(name, *args)
        routed.append(name)
        empty = _hip.Diag(None, None, None, None)
        return real_call('epropnp_monte_carlo_forward_diag', *args[:-1], None if how == 'null' else ctypes.byref(empty), args[-1])
    outs = []
    for patched in (False, True):
        if patched:
            monkeypatch.setattr(_hip, 'call', via_diag)
        p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
        x3d, x2d, w2d = (p[k].clone().requires_grad_(True) for k in ('x3d', 'x2d', 'w2d'))
        cf.set_param(x2d.detach(), w2d)
        init = RSLMSolver(dof=4, num_points=8, num_proposals=16, num_iter=3)
        init.draw = lambda w: (rn['inds'].to(backend), rn['rot'].float().to(backend))
        layer = EProPnP4DoF(mc_samples=S, num_iter=K, normalize=True, solver=LMSolver(dof=4, num_iter=3, init_solver=init))
        out = layer.monte_carlo_forward(x3d, x2d, w2d, cam, cf, pose_init=p['pose_init'], force_init_solve=True, with_cost=True,
                                        noise=noise)
        (out[5] + torch.logsumexp(out[4], 0)).mean().backward()
        outs.append([t.detach().clone() for t in out if t is not None] + [x3d.grad, x2d.grad, w2d.grad])
    assert routed == ['epropnp_monte_carlo_forward']
    for a, b in zip(*outs):
        assert torch.equal(a, b)
