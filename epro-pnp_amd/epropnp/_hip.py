"""ctypes binding of libepropnp_hip.so (C ABI declared in include/epropnp_hip.h).

There is no CPU implementation behind this module: if the shared library has not been built
(`python epro-pnp_amd/build.py`) or a tensor does not live on a HIP device, calls raise.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# EPROPNP_LIB: alternative build of the SAME HIP library (kernel-tuning variants, tools/tune.py); otherwise the in-tree
# build (epro-pnp_amd/lib, `python epro-pnp_amd/build.py`) or the copy a `pip install .` places inside the package
_IN_TREE = os.path.join(os.path.dirname(_HERE), 'lib', 'libepropnp_hip.so')
_INSTALLED = os.path.join(_HERE, '_lib', 'libepropnp_hip.so')
LIB_PATH = os.environ.get('EPROPNP_LIB') or (_INSTALLED if (os.path.exists(_INSTALLED) and not os.path.exists(_IN_TREE)) else _IN_TREE)

_i32p = C.POINTER(C.c_int32)


def tune(key):
    """EPROPNP_TUNE="key=value;key2;...": the ONE string behind which launch-shape overrides, implementation selectors and
    phase ablation live (csrc/pnp_host.h: tune_value; tools/tune.py and the shape tests set it, users do not).  Returns the text
    behind `key=` ('' for a bare key) or None.  Read on every call: tests change the variable at run time."""
    text = os.environ.get('EPROPNP_TUNE')
    if not text:
        return None
    for item in text.split(';'):
        k, _, v = item.partition('=')
        if k == key:
            return v
    return None


class Problem(C.Structure):
    _fields_ = [('x3d', C.c_void_p), ('x2d', C.c_void_p), ('w2d', C.c_void_p), ('cam_mats', C.c_void_p),
                ('lb', C.c_void_p), ('ub', C.c_void_p), ('delta', C.c_void_p), ('z_min', C.c_float),
                ('num_obj', C.c_int32), ('num_pts', C.c_int32), ('dof', C.c_int32),
                ('huber_eps', C.c_float), ('status', C.c_void_p), ('delta_stats', C.c_void_p),
                ('delta_relative', C.c_float)]


class LmParams(C.Structure):
    _fields_ = [('num_iter', C.c_int32), ('fast_mode', C.c_int32), ('min_lm_diagonal', C.c_float),
                ('max_lm_diagonal', C.c_float), ('min_relative_decrease', C.c_float),
                ('initial_trust_region_radius', C.c_float), ('max_trust_region_radius', C.c_float),
                ('eps', C.c_float)]


class AmisParams(C.Structure):
    _fields_ = [('mc_samples', C.c_int32), ('num_iter', C.c_int32), ('eps', C.c_float),
                ('acg_mle_iter', C.c_int32), ('acg_dispersion', C.c_float), ('seed', C.c_uint64),
                ('offset', C.c_uint64), ('offset_dev', C.c_void_p), ('split_scratch', C.c_void_p),
                ('split_scratch_bytes', C.c_uint64), ('advance', C.c_void_p), ('advance_ticket', C.c_void_p),
                ('advance_count', C.c_int32)]


class McParams(C.Structure):
    _fields_ = [('lm', LmParams), ('amis', AmisParams), ('normalize', C.c_int32), ('init_mode', C.c_int32),
                ('rslm_lm', LmParams), ('rslm_points', C.c_int32), ('rslm_proposals', C.c_int32),
                ('rslm_seed', C.c_uint64), ('rslm_offset', C.c_uint64), ('rslm_offset_dev', C.c_void_p),
                ('rslm_inds', C.c_void_p), ('rslm_rot', C.c_void_p), ('rslm_scratch', C.c_void_p),
                ('rslm_scratch_bytes', C.c_uint64), ('lm_scratch', C.c_void_p), ('lm_scratch_bytes', C.c_uint64)]


class Diag(C.Structure):
    """epropnp_diag: optional per-object diagnostics of epropnp_monte_carlo_forward_diag (device pointers, None = not wanted)"""
    _fields_ = [('lm_accept_mask', C.c_void_p), ('rslm_winner', C.c_void_p), ('proposals', C.c_void_p),
                ('weight_stats', C.c_void_p)]


ABI_VERSION = 7
_lib = None


# Every function of include/epropnp_hip.h, in header order: 'return type: one token per parameter'.  The one place the binding
# states a signature; tests/test_c_abi.py parses the header and compares it with this table, token by token.
#   p  pointer (void*, float*, int32_t*, ... : device or host memory)      s  const char*
#   i  int / int32_t     l  int64_t     u  uint64_t     z  size_t     f  float     d  double
#   problem* lm* amis* mc* diag*  pointer to that ABI struct                i* (return) int32_t* that Python indexes
SIGNATURES = {
    'epropnp_amis_forward_split_bytes': 'u: problem* i i',
    'epropnp_plan_amis_forward': 'i: problem* i i i i p',
    'epropnp_plan_amis_backward': 'i: problem* i i i i p',
    'epropnp_plan_evaluate_cost': 'i: problem* i p',
    'epropnp_monte_carlo_forward': 'i: problem* mc* p p p p p p p p p p p p p p p p',
    'epropnp_monte_carlo_forward_diag': 'i: problem* mc* p p p p p p p p p p p p p p p diag* p',
    'epropnp_weight_stats': 'i: p i i i p p',
    'epropnp_posterior_summary': 'i: p p p i i i p p',
    'epropnp_posterior_resample': 'i: p p i i i i p u u p p p',
    'epropnp_posterior_modes': 'i: p p p i i i f i p p p p p p p p',
    'epropnp_pose_errors': 'i: p p i i i p p i p p p p p z p p',
    'epropnp_pose_errors_scratch_bytes': 'z: i i i',
    'epropnp_bev_overlap': 'i: p i p i i i p p',
    'epropnp_bev_nms_scratch_bytes': 'z: i',
    'epropnp_bev_nms': 'i: p p p i f p z p p p p',
    'epropnp_box_overlap': 'i: p i p i i i i f i i p p',
    'epropnp_box_overlap_plan': 'i: p p i p l p p',
    'epropnp_box_overlap_segmented': 'i: p i p i i i i f i p i p l p',
    'epropnp_kitti_match_scratch_bytes': 'z: i i',
    'epropnp_kitti_match': 'i: p i l p p p i p i i p p p i p z p p p p',
    'epropnp_kitti_thresholds': 'i: p p p i i d p p p',
    'epropnp_kitti_statistics_scratch_bytes': 'z: i i i i',
    'epropnp_kitti_statistics': 'i: p i l p p p p i p p p i i i p p p i p p i i p z p p p',
    'epropnp_orient_density_scratch_bytes': 'z: i i',
    'epropnp_orient_density': 'i: p p p i i i i i i f f f p z p p p p p',
    'epropnp_bev_density_scratch_bytes': 'z: i i',
    'epropnp_bev_density': 'i: p p p p i i i i i i f i i i p z p p p',
    'epropnp_volume_centers_scratch_bytes': 'z: i i i',
    'epropnp_volume_centers': 'i: p p p p p p i i i i i i i i i f f i p z p p p p',
    'epropnp_box_thickness': 'i: p p p i i i i i i f p z p p p',
    'epropnp_point_targets': 'i: p p p p p p i p p p p i i i i f p p p p p p',
    'epropnp_obj_sample_weights': 'i: p p p l p i i f p p p p p',
    'epropnp_abi_version': 'i:',
    'epropnp_last_error': 's:',
    'epropnp_profile_enable': 'i: i',
    'epropnp_profile_reset': 'i:',
    'epropnp_profile_read': 'i: s p p',
    'epropnp_async_status': 'i: p i',
    'epropnp_async_status_word': 'i*:',
    'epropnp_noise_stride': 'i: i',
    'epropnp_evaluate_cost': 'i: problem* p i p p',
    'epropnp_cost_pose_cam_grad': 'i: problem* p p i i p p p',
    'epropnp_normal_equations': 'i: problem* p i p p p p',
    'epropnp_lm_solve': 'i: problem* lm* p p p p p p u p',
    'epropnp_lm_solve_split_bytes': 'u: problem* lm*',
    'epropnp_amis_forward': 'i: problem* amis* p p p p p p p',
    'epropnp_amis_backward': 'i: problem* p p i p p p p p p p',
    'epropnp_amis_backward_split': 'i: problem* p p i p p i p p p p p',
    'epropnp_amis_forward_costs': 'i: problem* amis* p p p p p p p p',
    'epropnp_monte_carlo_forward_costs': 'i: problem* mc* p p p p p p p p p p p p p p p diag* p p',
    'epropnp_request_sample_costs': 'i: p',
    'epropnp_amis_backward_costs': 'i: problem* p p i p p p p p p p p p',
    'epropnp_amis_backward_split_costs': 'i: problem* p p i p p i p p p p p p p',
    'epropnp_adaptive_delta': 'i: p p i i f p p p',
    'epropnp_mc_loss_forward': 'i: p p i i p p p',
    'epropnp_mc_loss_backward': 'i: p p p p i i p p p',
    'epropnp_mc_loss_reduce': 'i: p p i f f p i l p p p',
    'epropnp_exchange_pack': 'i: p u p i p u f p i p p',
    'epropnp_mc_loss_reduce_backward': 'i: p p p p p i i p p p',
    'epropnp_gn_step_forward': 'i: problem* f p p p',
    'epropnp_gn_step_backward': 'i: problem* f p p p p p p p',
    'epropnp_pose_opt_plus_forward': 'i: problem* f p p p',
    'epropnp_pose_opt_plus_backward': 'i: problem* f p p p p p p p',
    'epropnp_rslm_draw': 'i: p i i i i u u p p',
    'epropnp_center_points': 'i: p i i p p p',
    'epropnp_shift_poses': 'i: p p i i i f p p',
    'epropnp_prepare_forward': 'i: p p p p i i i p p p p',
    'epropnp_prepare_backward': 'i: p p p p p p p i i i p p p p p',
    'epropnp_prepare_dense_forward': 'i: p p p p p p i i i i i p p p p p',
    'epropnp_prepare_dense_backward': 'i: p p p p p p p p i i i i i p p p p p',
    'epropnp_deform_sample_forward': 'i: p p p p p p p i i i i i i i i l l l l p p p p p p p',
    'epropnp_deform_sample_backward': 'i: p p p p p p p p p p p p p i i i i i i i i l l l l p p p p p',
    'epropnp_roi_logsumexp_forward': 'i: p p i i i i p p',
    'epropnp_roi_logsumexp_backward': 'i: p p p p i i i i p p',
    'epropnp_roi_align_forward': 'i: p p p i i i i i i i f i i l l l l l l l l p p p',
    'epropnp_roi_align_backward': 'i: p p p i i i i i i i f i i l l l l l l l l p p p',
    'epropnp_shift_poses_backward': 'i: p p p i i i f p p',
    'epropnp_rslm_solve': 'i: problem* lm* i i u u p p p p p p u p',
    'epropnp_rslm_solve_scratch_bytes': 'u: problem* i',
    'epropnp_rslm_solve_diag': 'i: problem* lm* i i u u p p p p p p u p p',
}
EXPORTS = tuple(SIGNATURES)
CTYPES = {'p': C.c_void_p, 's': C.c_char_p, 'i': C.c_int32, 'l': C.c_int64, 'u': C.c_uint64, 'z': C.c_size_t, 'f': C.c_float,
          'd': C.c_double, 'i*': _i32p, 'problem*': C.POINTER(Problem), 'lm*': C.POINTER(LmParams), 'amis*': C.POINTER(AmisParams),
          'mc*': C.POINTER(McParams), 'diag*': C.POINTER(Diag)}


def signature(name, table=SIGNATURES):
    """-> (return token, [parameter tokens]) of one table entry"""
    ret, _, params = table[name].partition(':')
    return ret, params.split()


def _declare(lib):
    """Give every exported function of a loaded library its argtypes and restype from SIGNATURES."""
    for name in SIGNATURES:
        ret, params = signature(name)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = CTYPES[ret], [CTYPES[t] for t in params]
    return lib


def lib():
    """The loaded library; raises if it was never built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: the HIP extension has not been built '
                '(run `python epro-pnp_amd/build.py`); there is no CPU fallback')
        loaded = _declare(C.CDLL(LIB_PATH))
        if loaded.epropnp_abi_version() != ABI_VERSION:
            raise RuntimeError('libepropnp_hip.so ABI version mismatch')
        _lib = loaded
    return _lib


_torch_ext = False      # not tried yet


def torch_ext():
    """The C++ autograd nodes (lib/_epropnp_torch.so, csrc/torch_binding.cpp: same C ABI, no interpreter in the backward)
    or None when the module was not built / EPROPNP_NO_TORCH_EXT is set / another library build is selected with
    EPROPNP_LIB (the module is linked to the default one).  Either way the kernels are the library's."""
    global _torch_ext
    if _torch_ext is False:
        _torch_ext = None
        path = os.path.join(os.path.dirname(LIB_PATH), '_epropnp_torch.so')
        if os.path.exists(path) and not os.environ.get('EPROPNP_NO_TORCH_EXT') and not os.environ.get('EPROPNP_LIB'):
            import importlib.util
            lib()                        # the HIP library first: a missing / mismatching build fails with a clear message
            try:
                spec = importlib.util.spec_from_file_location('_epropnp_torch', path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                if mod.abi_version() == ABI_VERSION and mod.mc_params_size() == C.sizeof(McParams):
                    _torch_ext = mod
            except (ImportError, OSError) as e:      # built against another torch: same kernels through the ctypes nodes
                import warnings
                warnings.warn(f'{path} could not be loaded ({e}); using the ctypes binding of the same library')
    return _torch_ext


def check_device(t, name):
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on a HIP device (got {t.device}); the EPro-PnP HIP path has no CPU fallback')


def on_hip_path(*tensors):
    """True when the fused kernels can serve these tensors: fp32 on a HIP device."""
    return all(t.dtype == torch.float32 and t.is_cuda for t in tensors)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)     # hipStream_t as an int, without a Stream object


def stream_of(t):
    idx, cur = t.device.index, torch.cuda.current_device()
    if idx is not None and idx != cur:
        # kernels are launched on the calling thread's current device: a foreign stream would fail inside HIP
        raise RuntimeError(f'epropnp: tensors live on {t.device} but the current device is cuda:{cur}; call '
                           f'torch.cuda.set_device({idx}) (one process per GPU, as under torch.distributed)')
    if _raw_stream is not None:
        return _raw_stream(cur)
    return torch.cuda.current_stream(t.device).cuda_stream


def profile(enable=None, reset=False):
    """Per-stage HIP-event timing inside the library (epropnp_profile_*): switch it on / off, optionally dropping what was
    recorded so far."""
    if reset:
        lib().epropnp_profile_reset()
    if enable is not None:
        lib().epropnp_profile_enable(int(bool(enable)))


def profile_read(stage):
    """(mean ms per launch, number of launches) of `stage` since the last reset; synchronises on the recorded events."""
    ms, n = C.c_float(0), C.c_int32(0)
    lib().epropnp_profile_read(stage.encode(), C.byref(ms), C.byref(n))
    return (ms.value if n.value else float('nan')), n.value


ST_LM_NOT_SPD, ST_NONFINITE_POSE = 1, 2          # include/epropnp_hip.h: the two events the reference raises on
ST_SPLIT_TIMEOUT = 16                            # a split kernel recomputed a sibling workgroup's share: slower, results unaffected
_status_words = {}


STATUS_MODE = os.environ.get('EPROPNP_ASYNC_STATUS', 'warn')     # 'warn' (default) | 'raise' | '0' (no status word at all)


_has_gpu = None


def _gpu_present():
    """torch.cuda.is_available(), asked once: it is a driver query (hipGetDeviceCount, ~50 us on an MI355X box) and every entry
    into the package passes through poll_status()."""
    global _has_gpu
    if _has_gpu is None:
        _has_gpu = bool(torch.cuda.is_available())
    return _has_gpu


def poll_status():
    """The asynchronous half of the error convention.  Kernels report a damped normal-equation system without a Cholesky
    factor / a non-finite pose into the library's host-mapped status word of the current device; reading it is a plain
    host load, so every entry into the package polls it -- at the first call after the failing kernel has run, without
    ever synchronising (`flush_status()` synchronises and polls).
    What happens then follows the reference's behaviour rather than its letter: `torch.linalg.solve` / `torch.inverse`
    (levenberg_marquardt.py:15-19,178-181) raise only on an exactly zero LU pivot, which the LM damping rules out, and
    otherwise hand NaN poses on silently -- the callers' losses zero NaN objects (monte_carlo_pose_loss.py:31).  So the
    default is a RuntimeWarning naming the object; EPROPNP_ASYNC_STATUS=raise (or `_hip.STATUS_MODE = 'raise'`) turns it
    into the RuntimeError, `with numerics_check():` does so for a block, synchronously.  Events the reference takes in its
    stride (Cholesky fallback of a proposal, non-finite log-weight) are dropped here."""
    dev = torch.cuda.current_device() if _gpu_present() else 0
    w = _status_words.get((id(_lib), dev))
    if w is None:
        w = lib().epropnp_async_status_word()
        _status_words[(id(_lib), dev)] = w if w else False
    if not w:
        return
    flags = w[0]
    if flags:
        first = w[1]
        w[0], w[1] = 0, 2 ** 31 - 1
        if flags & ST_SPLIT_TIMEOUT:
            _warn_split_degraded(first, dev)
        msg = None
        if flags & ST_LM_NOT_SPD:
            msg = (f'linalg.solve: the damped normal equations of object {first} are singular or not finite '
                   f'(reported asynchronously by an earlier EPro-PnP launch on device {dev})')
        elif flags & ST_NONFINITE_POSE:
            msg = (f'the solver produced a non-finite pose for object {first} (reported asynchronously by an earlier '
                   f'EPro-PnP launch on device {dev})')
        if msg is not None:
            if STATUS_MODE == 'raise':
                raise RuntimeError(msg)
            import warnings
            warnings.warn(msg, RuntimeWarning, stacklevel=3)


_split_warned = False


def _warn_split_degraded(first, dev):
    """EPROPNP_ST_SPLIT_TIMEOUT is a PERFORMANCE event: in a launch that splits an object over several workgroups (AMIS
    forward at <= 64 objects, LM solve beyond 2048 points per object) a workgroup did not see a sibling's partial sums in
    time -- the siblings were not all resident (CU mask, partitioned GPU, another kernel holding CUs) -- and recomputed them
    itself: same bits, more time.  Said once per process."""
    global _split_warned
    if not _split_warned:
        _split_warned = True
        import warnings
        warnings.warn(f'EPro-PnP: a workgroup-split launch on device {dev} (object {first}) found a sibling workgroup missing '
                      f'and recomputed its share -- results are unaffected, the launch was slower.  If this GPU is shared or '
                      f'partitioned, EPROPNP_FWD_SPLIT=1 / EPROPNP_LM_SPLIT=1 switch the AMIS forward / LM solve splits off.',
                      RuntimeWarning, stacklevel=4)


def flush_status():
    """Synchronise the current device and raise any pending numerical event now."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    poll_status()


def call(fn_name, *args):
    rc = getattr(lib(), fn_name)(*args)
    if rc != 0:
        raise RuntimeError(f'{fn_name} failed ({rc}): {lib().epropnp_last_error().decode()}')
