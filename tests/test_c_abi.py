"""The C-ABI shared library exists after build(), exports every symbol include/*.h declares, and refuses to compute on
the host (no CPU fallback).  No GPU needed: nothing is launched."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT, abi_lib


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'epropnp_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(epropnp_[a-z_]+)\s*\(', txt)))


@pytest.fixture(scope='module')
def lib():
    return abi_lib()


_STRUCT_TOKEN = {'epropnp_problem': 'problem*', 'epropnp_lm_params': 'lm*', 'epropnp_amis_params': 'amis*',
                 'epropnp_mc_params': 'mc*', 'epropnp_diag': 'diag*'}
_SCALAR_TOKEN = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'size_t': 'z', 'float': 'f', 'double': 'd'}
_POINTEES = ('void', 'float', 'double', 'int8_t', 'uint8_t', 'int32_t', 'int64_t', 'uint64_t')


def _c_type_token(decl, is_parameter):
    """One C declaration of the header ('const float* pose_init', 'uint64_t') -> its token in _hip.SIGNATURES; `int32_t*` -> 'i*',
    which a plain 'p' of the table also covers.  ValueError for anything else."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if is_parameter and len(words) > 1 and words[-1] != '*':
        words = words[:-1]      # the parameter's name
    if len(words) == 1 and words[0] in _SCALAR_TOKEN:
        return _SCALAR_TOKEN[words[0]]
    if len(words) == 2 and words[1] == '*':
        if words[0] in _STRUCT_TOKEN:
            return _STRUCT_TOKEN[words[0]]
        if words[0] == 'char':
            return 's'
        if words[0] in _POINTEES:
            return 'i*' if words[0] == 'int32_t' else 'p'
    raise ValueError(f'cannot classify {decl!r}')


def header_signatures():
    """{function: (return token, [parameter tokens])} of every prototype in include/epropnp_hip.h.  Whatever is left of the header
    after comments, preprocessor lines, struct typedefs and the extern "C" braces must read as a prototype: ValueError otherwise."""
    txt = open(os.path.join(ROOT, 'include', 'epropnp_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    txt = re.sub(r'typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;', '', txt, flags=re.S)
    txt = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', '', txt, flags=re.M)
    out = {}
    for stmt in filter(None, (s.strip() for s in txt.split(';'))):
        m = re.fullmatch(r'([\w\s\*]+?)\s*\b(epropnp_\w+)\s*\(([^()]*)\)', stmt)
        if m is None:
            raise ValueError(f'cannot read {stmt!r} as a prototype')
        ret, name, params = m.groups()
        params = [] if params.strip() in ('', 'void') else params.split(',')
        assert name not in out, f'{name} declared twice'
        out[name] = (_c_type_token(ret, False), [_c_type_token(p, True) for p in params])
    return out


def signature_mismatches(table, header):
    """What differs between a signature table in the form of _hip.SIGNATURES and header_signatures(), one line per difference."""
    from epropnp import _hip
    same = lambda mine, theirs: mine == theirs or (mine == 'p' and theirs == 'i*')
    bad = [f'{name}: in the table, not in the header' for name in table if name not in header]
    for name, (ret, params) in header.items():
        if name not in table:
            bad.append(f'{name}: in the header, not in the table')
            continue
        my_ret, my_params = _hip.signature(name, table)
        unknown = [t for t in [my_ret] + my_params if t not in _hip.CTYPES]
        if unknown:
            bad.append(f'{name}: unknown token(s) {unknown}')
        if not same(my_ret, ret):
            bad.append(f'{name}: returns {ret}, the table says {my_ret}')
        if len(my_params) != len(params):
            bad.append(f'{name}: {len(params)} parameters, the table has {len(my_params)}')
        bad += [f'{name}: parameter {i} is {theirs}, the table says {mine}'
                for i, (mine, theirs) in enumerate(zip(my_params, params)) if not same(mine, theirs)]
    return bad


def test_signature_table_matches_the_header():
    """Every prototype of the header against the binding's table: return type and each parameter's type class, the struct pointers
    by the struct's name.  The parser reads every prototype (it raises on one it cannot) and finds as many as declared_symbols()."""
    from epropnp import _hip
    header = header_signatures()
    assert sorted(header) == declared_symbols() and len(header) == len(declared_symbols())
    assert signature_mismatches(_hip.SIGNATURES, header) == []
    used = {t for name in _hip.SIGNATURES for t in _hip.signature(name)[1]}
    assert set(_STRUCT_TOKEN.values()) <= used and {'i', 'l', 'u', 'z', 'f', 'd', 's', 'p'} <= used      # every class is exercised


def test_signature_check_reports_a_wrong_table():
    """The comparison can fail: a dropped parameter, an int32_t taken for an int64_t, a struct pointer taken for a plain pointer or
    for another struct, a wrong return type and a missing or extra function are each reported, naming the function."""
    from epropnp import _hip
    header = header_signatures()

    def mutated(name, edit):
        ret, params = _hip.signature(name)
        ret, params = edit(ret, list(params))
        return dict(_hip.SIGNATURES, **{name: f'{ret}: {" ".join(params)}'})
    cases = {
        'epropnp_lm_solve': lambda r, p: (r, p[:-1]),                                          # one parameter dropped
        'epropnp_weight_stats': lambda r, p: (r, [p[0], 'l'] + p[2:]),                         # int32_t -> int64_t
        'epropnp_evaluate_cost': lambda r, p: (r, ['p'] + p[1:]),                              # struct pointer -> plain pointer
        'epropnp_rslm_solve': lambda r, p: (r, [p[0], 'amis*'] + p[2:]),                       # the wrong struct
        'epropnp_exchange_pack': lambda r, p: (r, [p[0], 'z'] + p[2:]),                        # uint64_t -> size_t
        'epropnp_bev_nms_scratch_bytes': lambda r, p: ('u', p),                                # size_t -> uint64_t return
        'epropnp_async_status_word': lambda r, p: ('i', p),                                    # pointer return -> int
    }
    for name, edit in cases.items():
        assert _hip.signature(name, mutated(name, edit)) != _hip.signature(name), name        # (the edit changed something)
        bad = signature_mismatches(mutated(name, edit), header)
        assert len(bad) == 1 and bad[0].startswith(name + ':'), (name, bad)
    less = {k: v for k, v in _hip.SIGNATURES.items() if k != 'epropnp_noise_stride'}
    assert signature_mismatches(less, header) == ['epropnp_noise_stride: in the header, not in the table']
    more = dict(_hip.SIGNATURES, epropnp_no_such_entry='i: p')
    assert signature_mismatches(more, header) == ['epropnp_no_such_entry: in the table, not in the header']
    with pytest.raises(ValueError, match='cannot classify'):
        _c_type_token('long double x', True)


def test_every_function_of_the_loaded_library_is_typed(lib):
    """The loader gives every exported function argtypes and restype from the table, the four without parameters included."""
    from epropnp import _hip
    for name in _hip.EXPORTS:
        ret, params = _hip.signature(name)
        fn = getattr(lib, name)
        assert fn.restype is _hip.CTYPES[ret] and list(fn.argtypes) == [_hip.CTYPES[t] for t in params], name
    assert lib.epropnp_async_status_word.restype is ctypes.POINTER(ctypes.c_int32)


def test_exports_match_header(lib):
    syms = declared_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/epropnp_hip.h but not exported'
    from epropnp import _hip
    assert sorted(_hip.EXPORTS) == syms


def test_abi_version_and_noise_stride(lib):
    assert lib.epropnp_abi_version() == 7
    assert lib.epropnp_noise_stride(6) == 8 and lib.epropnp_noise_stride(4) == 52 and lib.epropnp_noise_stride(5) == -1


def test_argument_validation_without_launch(lib):
    from epropnp import _hip
    prob = _hip.Problem(None, None, None, None, None, None, None, 0.1, 4, 16, 5)
    rc = lib.epropnp_evaluate_cost(ctypes.byref(prob), None, 1, None, None)
    assert rc == -1 and b'dof' in lib.epropnp_last_error()
    prob = _hip.Problem(None, None, None, None, None, None, None, 0.1, 4, 16, 6)
    rc = lib.epropnp_evaluate_cost(ctypes.byref(prob), None, 1, None, None)
    assert rc == -1 and b'NULL' in lib.epropnp_last_error()
    # z_min is a depth clamp: the forward sweep's one-instruction max(z, z_min) relies on z_min >= 0
    prob = _hip.Problem(None, None, None, None, None, None, None, -0.1, 0, 16, 6)
    rc = lib.epropnp_evaluate_cost(ctypes.byref(prob), None, 1, None, None)
    assert rc == -1 and b'z_min' in lib.epropnp_last_error()


def test_negative_z_min_is_refused_by_the_python_layer(backend):
    from epropnp import functional as F
    from epropnp.camera import PerspectiveCamera
    from epropnp.cost_fun import HuberPnPCost
    z = lambda *s: torch.zeros(*s, device=backend)
    cam = PerspectiveCamera(cam_mats=torch.eye(3, device=backend).expand(2, 3, 3), z_min=-0.1)
    with pytest.raises(ValueError, match='z_min'):
        F.PnPProblem(z(2, 8, 3), z(2, 8, 2), z(2, 8, 2), cam, HuberPnPCost(delta=1.0), 6)


def test_product_path_refuses_cpu_tensors():
    from epropnp import _hip
    from epropnp.camera import PerspectiveCamera
    from epropnp.cost_fun import HuberPnPCost
    from epropnp.levenberg_marquardt import LMSolver
    import install as emu
    emu.uninstall()
    z = torch.zeros
    with pytest.raises(RuntimeError, match='HIP device'):
        LMSolver(dof=6, num_iter=1).solve(z(2, 8, 3), z(2, 8, 2), z(2, 8, 2), PerspectiveCamera(cam_mats=torch.eye(3).expand(2, 3, 3)),
                                          HuberPnPCost(), pose_init=z(2, 7))


def test_header_is_plain_c(tmp_path):
    """include/epropnp_hip.h is the drop-in boundary: it must compile as C99 (and C++) with nothing but <stdint.h>."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / 'abi.c'
    src.write_text('#include "epropnp_hip.h"\nint main(void) { return epropnp_abi_version() == EPROPNP_ABI_VERSION ? 0 : 1; }\n')
    for cmd in (['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror'], ['g++', '-std=c++11', '-Wall', '-Werror', '-x', 'c++']):
        r = subprocess.run(cmd + ['-I', os.path.join(root, 'include'), '-fsyntax-only', str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_c_program_links_and_runs(tmp_path, lib):
    """A C caller: include the header, link -lepropnp_hip, call the two entry points that need no device."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, 'epro-pnp_amd', 'lib')
    src = tmp_path / 'caller.c'
    src.write_text('#include <stdio.h>\n#include "epropnp_hip.h"\n'
                   'int main(void) { printf("%d %d %d\\n", epropnp_abi_version(), epropnp_noise_stride(6), epropnp_noise_stride(4));'
                   ' return 0; }\n')
    exe = tmp_path / 'caller'
    r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe), '-L', libdir,
                        '-lepropnp_hip', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-L', '/opt/rocm/lib'],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ['7', '8', '52']


def _build_standalone(tmp_path):
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/include/hip/hip_runtime_api.h'):
        pytest.skip('g++ / HIP headers not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, 'epro-pnp_amd', 'lib')
    exe = tmp_path / 'standalone'
    r = subprocess.run(['g++', '-O2', '-std=c++17', '-I', os.path.join(root, 'include'), '-I', '/opt/rocm/include',
                        os.path.join(root, 'examples', 'standalone_c_abi.cpp'), '-o', str(exe), '-L', libdir,
                        '-lepropnp_hip', '-L', '/opt/rocm/lib', '-lamdhip64', '-Wl,-rpath,' + libdir,
                        '-Wl,-rpath,/opt/rocm/lib'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_standalone_program_builds(tmp_path, lib):
    """examples/standalone_c_abi.cpp (no torch, only hipMalloc + the C ABI) compiles with g++ and links the library."""
    _build_standalone(tmp_path)


@pytest.mark.gpu
def test_standalone_program_on_gpu(tmp_path, lib):
    """The torch-free host program runs the whole path (delta -> LM -> AMIS -> loss -> backward) on the device and
    checks its own result: LM never worse than the start, pose near the generating pose, all outputs finite."""
    import subprocess
    exe = _build_standalone(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'STANDALONE objects=64' in out.stdout and 'finite=1' in out.stdout


def _integration_stub():
    """The ctypes stub INTEGRATION.md shows a reference maintainer (section B), executed as written against the in-tree library."""
    import re
    from epropnp import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    block = [b for b in re.findall(r'```python\n(.*?)```', text, flags=re.S) if 'def lm_solve_hip' in b]
    assert len(block) == 1
    ns = {}
    exec(block[0].replace("C.CDLL('libepropnp_hip.so')", f'C.CDLL({_hip.LIB_PATH!r})'), ns)
    return ns


def test_integration_stub_matches_the_abi(lib):
    from epropnp import _hip
    ns = _integration_stub()
    for mine, doc in ((_hip.Problem, ns['_Problem']), (_hip.LmParams, ns['_LmParams'])):
        assert ctypes.sizeof(mine) == ctypes.sizeof(doc)
        assert [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(doc, n).offset) for n, _ in doc._fields_]


@pytest.mark.gpu
def test_integration_stub_runs_lm_on_the_gpu():
    import install as emu
    import epropnp_oracle as orc
    from helpers import make_layer_objects
    from epropnp import functional as F
    from epropnp.levenberg_marquardt import LMSolver
    emu.uninstall()
    dev = torch.device('cuda:0')
    ns = _integration_stub()
    prob = orc.make_problem(6, 200, 6, seed=8)
    p, cam, cf = make_layer_objects(prob, dev)
    solver = LMSolver(dof=6, num_iter=4)
    pose, cov, cost = ns['lm_solve_hip'](solver, p['x3d'], p['x2d'], p['w2d'], cam, cf, p['pose_init'], True, True, False)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, 6)
    ref = F.lm_solve(hp, p['pose_init'], 4, with_pose_cov=True, with_cost=True)
    for a, b in zip((pose, cov, cost), ref):
        assert torch.equal(a, b)


def test_struct_layouts_of_the_header_match_the_ctypes_binding(tmp_path):
    """sizeof / offsetof of every struct in include/epropnp_hip.h, printed by a C program, against the ctypes Structures of
    epropnp/_hip.py (the C++ binding includes the header itself)."""
    import shutil
    import subprocess
    from epropnp import _hip
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    pairs = (('epropnp_problem', _hip.Problem), ('epropnp_lm_params', _hip.LmParams),
             ('epropnp_amis_params', _hip.AmisParams), ('epropnp_mc_params', _hip.McParams))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "epropnp_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'layout'
    r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f'{cname}.{f}']) == getattr(cls, f).offset, (cname, f)
    assert _hip.torch_ext() is None or _hip.torch_ext().mc_params_size() == ctypes.sizeof(_hip.McParams)
