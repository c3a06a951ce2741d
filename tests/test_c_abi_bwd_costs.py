"""The sample-cost additions to the C ABI (epropnp_amis_forward_costs, epropnp_monte_carlo_forward_costs, epropnp_amis_backward_costs,
epropnp_amis_backward_split_costs, epropnp_request_sample_costs) are additive: same ABI version, the header is still plain C, the
entries validate their arguments as the entries they extend, and the Python layer refuses host tensors and wrong sizes for the
new arguments as it does for the old ones."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'epro-pnp_amd', 'lib', 'libepropnp_hip.so')
NEW = ('epropnp_amis_forward_costs', 'epropnp_monte_carlo_forward_costs', 'epropnp_amis_backward_costs',
       'epropnp_amis_backward_split_costs', 'epropnp_request_sample_costs')


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


def test_header_with_the_cost_entries_is_plain_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    lines = ['#include "epropnp_hip.h"', 'int main(void) {', '  int n = 0;']
    lines += [f'  n += (int)(sizeof(&{s}) > 0);' for s in NEW] + [f'  return n == {len(NEW)} ? 0 : 1;', '}']
    src = tmp_path / 'costs.c'
    src.write_text('\n'.join(lines) + '\n')
    for cmd in (['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror'], ['g++', '-std=c++11', '-Wall', '-Werror', '-x', 'c++']):
        r = subprocess.run(cmd + ['-I', os.path.join(ROOT, 'include'), '-fsyntax-only', str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_argument_validation_without_launch(lib):
    """The checks of the entries they extend, in the same order: problem, sizes, NULL outputs -- nothing is launched."""
    from epropnp import _hip
    lib.epropnp_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.epropnp_amis_backward_costs.argtypes = [ctypes.POINTER(_hip.Problem), vp, vp, i32] + [vp] * 9
    lib.epropnp_amis_backward_split_costs.argtypes = [ctypes.POINTER(_hip.Problem), vp, vp, i32, vp, vp, i32] + [vp] * 7
    lib.epropnp_amis_forward_costs.argtypes = [ctypes.POINTER(_hip.Problem), ctypes.POINTER(_hip.AmisParams)] + [vp] * 8
    lib.epropnp_request_sample_costs.argtypes = [vp]
    bad_dof = _hip.Problem(None, None, None, None, None, None, None, 0.1, 4, 16, 5)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(bad_dof), *([None] * 2), 8, *([None] * 9)) == -1
    assert b'dof' in lib.epropnp_last_error()
    here = (ctypes.c_float * 4)()
    p = ctypes.addressof(here)
    prob = _hip.Problem(p, p, p, p, None, None, p, 0.1, 4, 128, 6)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(prob), None, None, 8, None, None, None, None, None, None, None, None, None) == -1
    assert b'NULL' in lib.epropnp_last_error()
    assert lib.epropnp_amis_backward_costs(ctypes.byref(prob), None, None, -1, *([None] * 9)) == -1
    assert b'negative' in lib.epropnp_last_error()
    assert lib.epropnp_amis_backward_split_costs(ctypes.byref(prob), p, p, 8, None, None, 3, None, None, p, p, p, p, None) == -1
    assert b'nsplit' in lib.epropnp_last_error()          # 3 x 64 > the 128 points
    par = _hip.AmisParams(10, 4, 1e-5, 3, 1e-3, 0, 0, None, None, 0)
    assert lib.epropnp_amis_forward_costs(ctypes.byref(prob), ctypes.byref(par), *([None] * 8)) == -1
    assert b'multiple' in lib.epropnp_last_error()
    empty = _hip.Problem(None, None, None, None, None, None, None, 0.1, 0, 128, 6)
    assert lib.epropnp_amis_backward_costs(ctypes.byref(empty), *([None] * 2), 8, *([None] * 9)) == 0       # no objects: nothing to do
    assert lib.epropnp_request_sample_costs(None) == 0


def test_python_layer_refuses_wrong_sizes(backend):
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    B, N, S, dof = 2, 64, 16, 6
    prob = orc.make_problem(B, N, dof, seed=3)
    p, cam, _ = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    samples = p['pose_gt'].unsqueeze(0).repeat(S, 1, 1).contiguous()
    g_logw, g_init = torch.ones(S, B, device=backend), torch.ones(B, device=backend)
    costs, cinit = torch.ones(S, B, device=backend), torch.ones(B, device=backend)
    with pytest.raises(ValueError, match='sample_costs'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs[:-1], cost_init=cinit)
    with pytest.raises(ValueError, match='sample_costs'):
        F.amis_backward(hp, samples, g_logw, None, None, sample_costs=costs.t().contiguous())
    with pytest.raises(ValueError, match='cost_init'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=torch.ones(B + 1, device=backend))
    with pytest.raises(TypeError, match='fp32'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs.double(), cost_init=cinit)


@pytest.mark.gpu
def test_python_layer_refuses_host_tensors_for_the_costs():
    import install as emu
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    emu.uninstall()
    dev = torch.device('cuda:0')
    B, N, S, dof = 2, 64, 16, 6
    prob = orc.make_problem(B, N, dof, seed=3)
    p, cam, _ = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    samples = p['pose_gt'].unsqueeze(0).repeat(S, 1, 1).contiguous()
    g_logw, g_init = torch.ones(S, B, device=dev), torch.ones(B, device=dev)
    with pytest.raises(RuntimeError, match='HIP device'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=torch.ones(S, B), cost_init=torch.ones(B, device=dev))
    with pytest.raises(RuntimeError, match='HIP device'):
        F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=torch.ones(S, B, device=dev), cost_init=torch.ones(B))
