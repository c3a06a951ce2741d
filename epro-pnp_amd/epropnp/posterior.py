"""Posterior summaries and resampling of the weighted pose samples `monte_carlo_forward` returns.

The layer's product is a pose distribution in its raw form: `pose_samples (S,B,4|7)` with `pose_sample_logweights (S,B)`.
`summarize` reduces it, per object and in one launch, to what its consumers otherwise re-derive with chains of elementwise and
reduce launches over (S,B,.) temporaries -- the Det head's test-time orientation score and the moments of the distribution;
`resample` turns it into equally weighted draws (systematic resampling) for a tracker or planner; `modes` finds the hypotheses of
an ambiguous posterior -- the peaks, their probability mass and the samples that belong to each (quick-shift clustering).

All run on the current HIP stream of the inputs' device, allocate their outputs with torch.empty, never synchronise and can be
captured into a hipGraph.  None is differentiable: inputs are detached.
"""
from collections import namedtuple

import torch

from . import _hip
from .functional import _f32c

WORDS = 16      # include/epropnp_hip.h: EPROPNP_POSTERIOR_WORDS

PosteriorSummary = namedtuple('PosteriorSummary', ['trans_mean', 'trans_cov', 'rot_mean', 'rot_resultant', 'score_te', 'raw'])
PosteriorSummary.__doc__ = """Per-object summary of the weighted pose samples (views of `raw`, except trans_cov).

trans_mean    (B,3)     weighted mean of the sample translations
trans_cov     (B,3,3)   their weighted covariance (symmetric)
rot_mean      (B,) | (B,4)  4-DoF: circular mean of the yaw; 6-DoF: the quaternion mean that counts q and -q alike (principal
                        eigenvector of sum w q q^T / W), signed towards pose_ref's quaternion, else first non-zero component positive
rot_resultant (B,)      4-DoF: mean resultant length in [0, 1]; 6-DoF: the principal eigenvalue in [1/4, 1]
score_te      (B,) | None   the Det head's sample score about pose_ref (None without pose_ref)
raw           (B,16)    the row layout of include/epropnp_hip.h: epropnp_posterior_summary"""

_COV = (3, 4, 5, 4, 6, 7, 5, 7, 8)      # words of (xx xy xz / xy yy yz / xz yz zz)


def _inputs(pose_samples, logweights):
    ps = _f32c(pose_samples, 'pose_samples')
    lw = _f32c(logweights, 'pose_sample_logweights')
    if ps.dim() != 3 or ps.shape[-1] not in (4, 7) or lw.shape != ps.shape[:2]:
        raise ValueError(f'pose_samples (S,B,4|7) and pose_sample_logweights (S,B) expected, got {tuple(ps.shape)} and {tuple(lw.shape)}')
    if ps.shape[0] < 1:
        raise ValueError('at least one sample per object is needed')
    return ps, lw, 4 if ps.shape[-1] == 4 else 6


def summarize(pose_samples, pose_sample_logweights, pose_ref=None):
    """Weighted moments of the pose samples per object -> PosteriorSummary.  Not differentiable (inputs are detached).

    pose_ref (B,4|7), e.g. pose_opt: the pose `score_te` measures the samples' xz deviation from -- the reference's
    `((-sample_dev.log2() + 2.5) / 4).clamp(0, 1)` summed under softmax(logweights) -- and the sign of the 6-DoF mean.
    Samples of weight exp(logw - max) == 0 are skipped; a column holding a NaN / +inf log-weight or nothing but -inf gives NaNs."""
    ps, lw, dof = _inputs(pose_samples, pose_sample_logweights)
    S, B, P = ps.shape
    ref = None
    if pose_ref is not None:
        ref = _f32c(pose_ref, 'pose_ref')
        if ref.shape != (B, P):
            raise ValueError(f'pose_ref: expected {(B, P)}, got {tuple(ref.shape)}')
    raw = torch.empty((B, WORDS), dtype=torch.float32, device=ps.device)
    if B > 0:
        _hip.call('epropnp_posterior_summary', _hip.ptr(ps), _hip.ptr(lw), _hip.ptr(ref), S, B, dof, _hip.ptr(raw), _hip.stream_of(ps))
    return PosteriorSummary(trans_mean=raw[:, 0:3], trans_cov=torch.stack([raw[:, i] for i in _COV], 1).reshape(B, 3, 3),
                            rot_mean=raw[:, 11] if dof == 4 else raw[:, 11:15], rot_resultant=raw[:, 10],
                            score_te=None if ref is None else raw[:, 9], raw=raw)


def resample(pose_samples, pose_sample_logweights, num_draws, seed=None, offset=0, u=None, with_poses=True):
    """Systematic resampling into `num_draws` equally weighted draws per object -> (index (R,B) int32, poses (R,B,P) | None).
    Not differentiable (inputs are detached).

    One uniform u_b per object: `u` (B,) in [0, 1) when given, else the library's Philox stream of (seed, offset, b); seed=None
    draws one seed from torch's generator (torch.manual_seed governs it).  Draw r is the first sample whose running weight sum
    exceeds (u_b + r) / R of the total: index is non-decreasing in r, zero-weight samples are never drawn, and
    poses == pose_samples[index, b] bit for bit.  Bad and empty columns (see summarize): index -1, NaN poses."""
    ps, lw, dof = _inputs(pose_samples, pose_sample_logweights)
    S, B, P = ps.shape
    R = int(num_draws)
    if R < 1:
        raise ValueError(f'num_draws must be >= 1, got {num_draws}')
    if u is not None:
        u = _f32c(u, 'u')
        if u.shape != (B,):
            raise ValueError(f'u: expected {(B,)}, got {tuple(u.shape)}')
        seed = 0
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    index = torch.empty((R, B), dtype=torch.int32, device=ps.device)
    poses = torch.empty((R, B, P), dtype=torch.float32, device=ps.device) if with_poses else None
    if B > 0:
        _hip.call('epropnp_posterior_resample', _hip.ptr(ps), _hip.ptr(lw), S, B, dof, R, _hip.ptr(u), int(seed), int(offset),
                  _hip.ptr(index), _hip.ptr(poses), _hip.stream_of(ps))
    return index, poses


PosteriorModes = namedtuple('PosteriorModes', ['index', 'poses', 'mass', 'num_modes', 'labels', 'parent', 'density'])
PosteriorModes.__doc__ = """Per-object modes of the weighted pose samples (include/epropnp_hip.h: epropnp_posterior_modes), M = max_modes.

index     (M,B) int32   sample index of the m-th heaviest mode's root; -1 beyond min(M, num_modes)
poses     (M,B,P)       pose_samples[index, b] bit for bit; NaN beyond
mass      (M,B)         share of the total weight in the mode's tree, descending in m; 0 beyond
num_modes (B,) int32    number of modes found (may exceed M)
labels    (S,B) int32   the root sample of each sample's mode; -1 for samples of weight 0
parent    (S,B) int32   quick-shift parent (a root is its own parent); -1 for samples of weight 0
density   (S,B)         kernel density estimate at the samples; NaN for samples of weight 0"""


def _bandwidth(bandwidth, B, device):
    """(B,2) fp32 device tensor of (h_t, h_r) from a pair of floats / (B,) tensors or a (B,2) tensor; floats are written with fill
    launches (no host-to-device copy: capturable)."""
    if torch.is_tensor(bandwidth):
        bw = _f32c(bandwidth, 'bandwidth')
        if bw.shape != (B, 2):
            raise ValueError(f'bandwidth: expected {(B, 2)}, got {tuple(bw.shape)}')
        return bw
    if not isinstance(bandwidth, (tuple, list)) or len(bandwidth) != 2:
        raise ValueError('bandwidth: a pair (h_t, h_r) of floats or (B,) tensors, or a (B,2) tensor, is expected')
    bw = torch.empty((B, 2), dtype=torch.float32, device=device)
    for k, h in enumerate(bandwidth):
        if torch.is_tensor(h):
            h = _f32c(h, 'bandwidth')
            if h.shape != (B,):
                raise ValueError(f'bandwidth: expected {(B,)} tensors, got {tuple(h.shape)}')
            bw[:, k].copy_(h)
        else:
            bw[:, k].fill_(float(h))
    return bw


def modes(pose_samples, pose_sample_logweights, bandwidth, max_modes=4, link=3.0):
    """Modes of the weighted pose samples per object by quick-shift clustering -> PosteriorModes.  Not differentiable.

    bandwidth: the scale below which two poses are the same hypothesis -- a pair (h_t, h_r) of floats or (B,) tensors, or a (B,2)
    tensor; h_t in the translation's unit, h_r in radians.  There is deliberately no data-driven default: a rule on the global
    moments (Silverman) sees the spread BETWEEN the peaks of an ambiguous posterior and merges them.
    With w_j = exp(logw_j - max), D_ij = |t_i - t_j|^2 / h_t^2 + rho_ij / h_r^2 (rho ~ the squared rotation angle, q and -q alike)
    the density at sample i is f_i = sum_j w_j exp(-D_ij / 2) / sum w; every sample links to the nearest sample of higher density
    within D <= link^2, samples without one are the modes, and a mode's mass is the weight share of its tree.  The `max_modes`
    heaviest are returned, heaviest first.  Samples of weight 0 take no part (label -1); a column holding a NaN / +inf log-weight,
    nothing but -inf, or a bandwidth that is not finite and > 0 gives num_modes 0, indices -1 and NaNs."""
    ps, lw, dof = _inputs(pose_samples, pose_sample_logweights)
    S, B, P = ps.shape
    M, link = int(max_modes), float(link)
    if M < 1:
        raise ValueError(f'max_modes must be >= 1, got {max_modes}')
    if not (0.0 < link < float('inf')):
        raise ValueError(f'link must be finite and > 0, got {link}')
    bw = _bandwidth(bandwidth, B, ps.device)
    dev = ps.device
    out = PosteriorModes(index=torch.empty((M, B), dtype=torch.int32, device=dev), poses=torch.empty((M, B, P), dtype=torch.float32, device=dev),
                         mass=torch.empty((M, B), dtype=torch.float32, device=dev), num_modes=torch.empty((B,), dtype=torch.int32, device=dev),
                         labels=torch.empty((S, B), dtype=torch.int32, device=dev), parent=torch.empty((S, B), dtype=torch.int32, device=dev),
                         density=torch.empty((S, B), dtype=torch.float32, device=dev))
    if B > 0:
        _hip.call('epropnp_posterior_modes', _hip.ptr(ps), _hip.ptr(lw), _hip.ptr(bw), S, B, dof, link, M, _hip.ptr(out.density),
                  _hip.ptr(out.parent), _hip.ptr(out.labels), _hip.ptr(out.num_modes), _hip.ptr(out.index), _hip.ptr(out.mass),
                  _hip.ptr(out.poses), _hip.stream_of(ps))
    return out
