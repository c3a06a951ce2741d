"""Posterior summaries and resampling of the weighted pose samples `monte_carlo_forward` returns.

The layer's product is a pose distribution in its raw form: `pose_samples (S,B,4|7)` with `pose_sample_logweights (S,B)`.
`summarize` reduces it, per object and in one launch, to what its consumers otherwise re-derive with chains of elementwise and
reduce launches over (S,B,.) temporaries -- the Det head's test-time orientation score and the moments of the distribution;
`resample` turns it into equally weighted draws (systematic resampling) for a tracker or planner.

Both run on the current HIP stream of the inputs' device, allocate their outputs with torch.empty, never synchronise and can be
captured into a hipGraph.  Neither is differentiable: inputs are detached.
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
