"""Posterior summaries and resampling of the weighted pose samples `monte_carlo_forward` returns.

The layer's product is a pose distribution in its raw form: `pose_samples (S,B,4|7)` with `pose_sample_logweights (S,B)`.
`summarize` reduces it, per object and in one launch, to what its consumers otherwise re-derive with chains of elementwise and
reduce launches over (S,B,.) temporaries -- the Det head's test-time orientation score and the moments of the distribution;
`resample` turns it into equally weighted draws (systematic resampling) for a tracker or planner; `modes` finds the hypotheses of
an ambiguous posterior -- the peaks, their probability mass and the samples that belong to each (quick-shift clustering).
`orient_density` and `bev_density` draw it: the orientation sphere of the 6-DoF test loop and the bird's-eye-view sample density of
the Det detector, splat + box filter (+ colour composite) without a full-canvas temporary or a float atomic.

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


OrientDensity = namedtuple('OrientDensity', ['image', 'front', 'back', 'bins'])
OrientDensity.__doc__ = """Orientation-sphere picture of the weighted 6-DoF pose samples (include/epropnp_hip.h: epropnp_orient_density).

image (B,size,size,3)   the colour composite of the reference's `draw_orient_density`, in [0, 1]
front (B,size,size,3)   box-summed weight of rotated axis k on the front hemisphere (a_z <= 0); None unless with_density
back  (B,size,size,3)   the same on the back hemisphere; None unless with_density
bins  (S,B,3) int32     the bin each axis point fell into: py * size + px, + size^2 on the back hemisphere, -1 when dropped;
                        None unless with_bins"""

BevDensity = namedtuple('BevDensity', ['density', 'bins'])
BevDensity.__doc__ = """Bird's-eye-view density of the weighted pose samples (include/epropnp_hip.h: epropnp_bev_density).

density (G,H,W)       box-summed weight per grid cell and group
bins    (S,B) int32   the cell each sample fell into: py * W + px, -1 when off the grid; None unless with_bins"""


def _window(window, name):
    kh, kw = (window, window) if isinstance(window, int) else tuple(window)
    kh, kw = int(kh), int(kw)
    for k in (kh, kw):
        if k < 1 or k > 9 or k % 2 == 0:
            raise ValueError(f'{name}: odd sizes from 1 to 9 are expected, got {window}')
    return kh, kw


def orient_density(pose_samples, pose_sample_logweights, pose_opt=None, size=512, window=(5, 5), saturation=0.5,
                   sphere_opacity=0.6, intensity_scale=50, with_density=False, with_bins=False):
    """Orientation-sphere density of 6-DoF pose samples -> OrientDensity: the arithmetic of the reference's
    `draw_orient_density` (EPro-PnP-6DoF lib/utils/draw_orient_density.py) in two launches, without a full-canvas temporary.

    Per object the weights are softmax(logweights) over the samples; sample j puts weight w_j for axis k at the pixel
    rint(a * 0.4 size + size / 2 - 0.5) of a = column k of its quaternion's rotation (not normalised), on the front canvas iff
    a_z <= 0; points off the canvas or not finite are dropped.  front / back are the zero-padded (kh, kw) box sums; the image is
    (back_layer * opacity + circle * (1 - opacity)) * front_layer with layer_c = prod_k col[k, c] ** (intensity_scale * density_k).
    pose_opt (B,7): its three axes are drawn as lines from the centre -- a pixel whose centre lies within 1.5 px of the segment
    takes the axis' pure colour, a later axis over an earlier one (the reference's cv2.line(thickness=3) is not reproduced pixel
    for pixel).  A column holding a NaN / +inf log-weight or nothing but -inf gives a NaN canvas.  Every sum runs in sample order:
    two calls agree to the last bit."""
    ps, lw, dof = _inputs(pose_samples, pose_sample_logweights)
    if dof != 6:
        raise ValueError('orient_density shows orientations: pose_samples (S,B,7) expected')
    S, B, P = ps.shape
    size = int(size)
    if size < 1 or size > 4096:
        raise ValueError(f'size must be 1 .. 4096, got {size}')
    kh, kw = _window(window, 'window')
    opt = None
    if pose_opt is not None:
        opt = _f32c(pose_opt, 'pose_opt')
        if opt.shape != (B, P):
            raise ValueError(f'pose_opt: expected {(B, P)}, got {tuple(opt.shape)}')
    dev = ps.device
    image = torch.empty((B, size, size, 3), dtype=torch.float32, device=dev)
    front = torch.empty((B, size, size, 3), dtype=torch.float32, device=dev) if with_density else None
    back = torch.empty((B, size, size, 3), dtype=torch.float32, device=dev) if with_density else None
    bins = torch.empty((S, B, 3), dtype=torch.int32, device=dev) if with_bins else None
    if B > 0:
        nbytes = int(_hip.lib().epropnp_orient_density_scratch_bytes(S, B))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _hip.call('epropnp_orient_density', _hip.ptr(ps), _hip.ptr(lw), _hip.ptr(opt), S, B, dof, size, kh, kw, float(saturation),
                  float(sphere_opacity), float(intensity_scale), _hip.ptr(scratch), nbytes, _hip.ptr(image), _hip.ptr(front),
                  _hip.ptr(back), _hip.ptr(bins), _hip.stream_of(ps))
    return OrientDensity(image=image, front=front, back=back, bins=bins)


def bev_density(pose_samples, pose_sample_logweights, height, width, scale=10., origin=None, obj_weight=None, groups=None,
                num_groups=None, window=3, with_bins=False):
    """Bird's-eye-view density of the pose samples of many objects -> BevDensity: the density block of the reference's `show_bev`
    (EPro-PnP-Det core/visualizer/image_bev_vis.py:79-95) on the device.

    Sample j of object b adds softmax(logweights[:, b])_j * obj_weight[b] (the 2-D score; 1 without) at px = rint(z * scale) +
    origin[0], py = rint(x * scale) + origin[1] of the grid of its group (`groups` (B,) integers in [0, num_groups), e.g. the image
    index; one group without; objects of a group outside that range are left out); origin=None is (int(width / 16),
    int(height / 2)) as in `show_bev`.  Samples off the grid are dropped, an object with a bad column adds nothing.  density is the
    zero-padded window x window box sum -- cv2.blur times window^2, except in the outermost window // 2 rows and columns, where
    cv2.blur reflects.  Objects need not be sorted by group; with `groups` given pass `num_groups` too, or it is read off the
    device (groups.max() + 1: one synchronisation)."""
    ps, lw, dof = _inputs(pose_samples, pose_sample_logweights)
    S, B, P = ps.shape
    H, W = int(height), int(width)
    if H < 1 or H > 4096 or W < 1 or W > 4096:
        raise ValueError(f'height and width must be 1 .. 4096, got {height} and {width}')
    if not isinstance(window, int):
        raise ValueError(f'window: one odd size from 1 to 9 is expected, got {window}')
    k, _ = _window(window, 'window')
    ox, oy = (int(W / 16), int(H / 2)) if origin is None else (int(origin[0]), int(origin[1]))
    dev = ps.device
    ow = None
    if obj_weight is not None:
        ow = _f32c(obj_weight, 'obj_weight')
        if ow.shape != (B,):
            raise ValueError(f'obj_weight: expected {(B,)}, got {tuple(ow.shape)}')
    perm = None
    if groups is None:
        G = 1 if num_groups is None else int(num_groups)
        offsets = torch.zeros((G + 1,), dtype=torch.int32, device=dev)
        if G > 0:
            offsets[1:] = B
    else:
        if not torch.is_tensor(groups) or groups.dtype not in (torch.int32, torch.int64) or groups.shape != (B,):
            raise ValueError(f'groups: a ({B},) integer tensor is expected')
        _hip.check_device(groups, 'groups')
        if groups.device != dev:
            raise RuntimeError(f'groups lives on {groups.device}, the samples on {dev}')
        G = int(num_groups) if num_groups is not None else (int(groups.max().item()) + 1 if B > 0 else 0)
        sorted_groups, perm = torch.sort(groups.detach().to(torch.int64), stable=True)
        offsets = torch.searchsorted(sorted_groups, torch.arange(G + 1, dtype=torch.int64, device=dev)).to(torch.int32)
        ps, lw = ps[:, perm].contiguous(), lw[:, perm].contiguous()
        ow = None if ow is None else ow[perm].contiguous()
    if G < 0:
        raise ValueError(f'num_groups must be >= 0, got {num_groups}')
    density = torch.empty((G, H, W), dtype=torch.float32, device=dev)
    bins = torch.empty((S, B), dtype=torch.int32, device=dev) if with_bins else None
    if G > 0 or (B > 0 and with_bins):
        nbytes = int(_hip.lib().epropnp_bev_density_scratch_bytes(S, B))
        scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _hip.call('epropnp_bev_density', _hip.ptr(ps), _hip.ptr(lw), _hip.ptr(ow), _hip.ptr(offsets), S, B, G, dof, H, W, float(scale),
                  ox, oy, k, _hip.ptr(scratch), nbytes, _hip.ptr(density), _hip.ptr(bins), _hip.stream_of(ps))
    if bins is not None and perm is not None:
        unsorted = torch.empty_like(bins)
        unsorted[:, perm] = bins
        bins = unsorted
    return BevDensity(density=density, bins=bins)
