"""epropnp.posterior.modes (epropnp_posterior_modes): quick-shift modes of the weighted pose samples against the same definition in
fp64 torch on the same fp32 inputs.  Shapes: (1,1); (64,3) one chunk of samples, a partly filled lane set; (510,70) S no multiple of
the workgroup, a padded object grid and the edge columns; (4096,2) the largest column that stays in LDS, split over workgroups; and,
on the GPU only, (6000,2) which streams through LDS in tiles.  The split and the tiles are also forced at (510,70) on both backends."""
import math

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise

SMALL = [(1, 1), (64, 3), (510, 70)]
CENTER = (2.0, 1.0, 50.0)
EDGE = {5: 'empty', 9: 'nan', 40: 'inf'}      # as tests/test_posterior.py; column 66: half the samples -inf with NaN poses
EPS = 64 * 2.0 ** -24                          # D is about 20 fp32 roundings
LINK = 3.0
# Density against fp64, largest relative error over the participating samples.  The bar is 4 x the error of the SAME definition
# evaluated by torch in fp32 on the CPU, computed in the test at the same inputs (the factor covers the folded exp2 argument and another
# summation order).  Measured, kernel / fp32 torch, the case with the largest ratio and the one with the largest error:
#   CPU emulation: 1.65e-6 / 0.90e-6 (S=64 B=3 4-DoF +-40), 2.35e-6 / 2.36e-6 (S=510 B=70 4-DoF +-40)
#   MI355X:        1.71e-6 / 0.77e-6 (S=6000 B=2 6-DoF +-40), 2.35e-6 / 2.36e-6 (S=510 B=70 4-DoF +-40); (4096,2): 1.10e-6 / 0.97e-6
#   (4-DoF) and 0.91e-6 / 1.22e-6 (6-DoF).  The largest ratio seen is 2.2.
DENSITY_FACTOR = 4.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mass_bar(S):
    return (2 * 88 + S + 8) * 2.0 ** -24      # the rounding of exp's argument (|logw - max| < 88, twice) plus S additions


_cases = {}


def _case(S, B, dof, lw_half, spread=1.0):
    """(pose_samples, logweights, bandwidth (B,2), good columns) on the CPU, once per key: log-weights over +-lw_half, translations
    CENTER + spread * randn, yaws around a per-object centre anywhere in +-3 (so that some objects straddle +-pi) / quaternions
    around a per-object q0 with every second sign flipped, per-object bandwidths around (0.5, 0.2) * spread; a NaN pose under a -inf
    log-weight in column 0; at B >= 70 the edge columns."""
    key = (S, B, dof, lw_half, spread)
    if key not in _cases:
        g = torch.Generator().manual_seed(2000 * dof + S + B + int(lw_half))
        lw = (torch.rand(S, B, generator=g) * 2.0 - 1.0) * lw_half
        t = torch.tensor(CENTER) + spread * torch.randn(S, B, 3, generator=g)
        if dof == 4:
            rot = torch.rand(B, 1, generator=g) * 6.0 - 3.0 + 0.3 * torch.randn(S, B, 1, generator=g)
        else:
            q0 = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
            rot = torch.nn.functional.normalize(q0 + 0.1 * torch.randn(S, B, 4, generator=g), dim=-1)
            rot[1::2] = -rot[1::2]
        ps = torch.cat((t, rot), -1).contiguous()
        bw = (torch.tensor([0.5 * spread, 0.2]) * (0.75 + 0.5 * torch.rand(B, 2, generator=g))).contiguous()
        if S >= 2:
            lw[S // 2, 0] = float('-inf')
            ps[S // 2, 0] = float('nan')
        good = list(range(B))
        if B >= 70:
            lw[:, 5] = float('-inf')
            lw[S // 3, 9] = float('nan')
            lw[S - 1, 40] = float('inf')
            lw[::2, 66] = float('-inf')
            ps[::2, 66] = float('nan')
            good = [b for b in range(B) if b not in EDGE]
        _cases[key] = (ps, lw, bw, good)
    return _cases[key]


# ---- the definition, in torch, one object at a time ---------------------------------------------------------------------
def _weights(lw, dtype):
    lw = lw.to(dtype)
    w = torch.exp(lw - lw.max())
    return w, w.sum()


def _pair_d(ps, bw, rows, dtype):
    """D_ij for i in rows, all j; ps (S,P) with the poses of weight-0 samples zeroed"""
    ps, ht, hr = ps.to(dtype), bw[0].to(dtype), bw[1].to(dtype)
    t = ps[:, :3]
    dt2 = (t[rows, None, :] - t[None, :, :]).square().sum(-1)
    if ps.shape[-1] == 4:
        s = torch.sin((ps[rows, None, 3] - ps[None, :, 3]) / 2)
        rho = 4 * s * s
    else:
        q = ps[:, 3:]
        d2 = torch.minimum((q[rows, None, :] - q[None, :, :]).square().sum(-1), (q[rows, None, :] + q[None, :, :]).square().sum(-1))
        rho = d2 * (4 - d2)
    return dt2 / (ht * ht) + rho / (hr * hr)


def _blocks(S, step=1024):
    return [torch.arange(lo, min(lo + step, S)) for lo in range(0, S, step)]


def _density(ps, lw, bw, dtype):
    """f_i of one object in `dtype`; NaN where w == 0"""
    w, W = _weights(lw, dtype)
    live = w > 0
    ps = torch.where(live[:, None], ps, torch.zeros_like(ps))
    f = torch.cat([(w[None, :] * torch.exp(-_pair_d(ps, bw, rows, dtype) / 2)).sum(1) for rows in _blocks(ps.shape[0])]) / W
    return torch.where(live, f, torch.full_like(f, float('nan')))


def _pairs64(ps, lw, bw):
    """(D_ij, f_i) of one object in fp64, the poses of weight-0 samples zeroed, f NaN there"""
    w, W = _weights(lw, torch.float64)
    live = w > 0
    D = _pair_d(torch.where(live[:, None], ps, torch.zeros_like(ps)), bw, torch.arange(ps.shape[0], device=ps.device), torch.float64)
    f = (w[None, :] * torch.exp(-D / 2)).sum(1) / W
    return D, torch.where(live, f, torch.full_like(f, float('nan')))


def _quick_shift64(ps, lw, bw, link=LINK, pairs=None):
    """the whole definition in fp64 for one object -> (density, parent, parent D, labels)"""
    S = ps.shape[0]
    D, f = pairs if pairs is not None else _pairs64(ps, lw, bw)
    live = ~torch.isnan(f)
    idx = torch.arange(S, device=f.device)
    cand = live[None, :] & ((f[None, :] > f[:, None]) | ((f[None, :] == f[:, None]) & (idx[None, :] < idx[:, None]))) & (D <= link * link)
    Dc = torch.where(cand, D, torch.full_like(D, float('inf')))
    best, arg = Dc.min(1)
    parent = torch.where(torch.isinf(best), idx, arg)
    parent = torch.where(live, parent, torch.full_like(parent, -1))
    return f, parent, torch.where(torch.isinf(best), torch.zeros_like(best), best), _follow(parent[:, None])[:, 0]


def _follow(parent):
    """roots of the chains of parent (S,B), -1 kept"""
    lab = parent.long().clone()
    for _ in range(max(1, math.ceil(math.log2(max(parent.shape[0], 2))))):
        lab = torch.where(lab >= 0, lab.gather(0, lab.clamp(min=0)), lab)
    assert torch.equal(lab, torch.where(lab >= 0, lab.gather(0, lab.clamp(min=0)), lab))
    return lab


# ---- checks ---------------------------------------------------------------------------------------------------------------
def _check_object(got, ps, lw, bw, b, M, link, errs, odev=torch.device('cpu')):
    """items 1 - 3 of one good column b; the fp64 side runs on `odev` (the fp32 torch yardstick always on the CPU)"""
    S = ps.shape[0]
    f32 = _density(ps, lw, bw, torch.float32).double().to(odev)
    ps, lw, bw = ps.to(odev), lw.to(odev), bw.to(odev)
    got = type(got)(*[f[:, b:b + 1].to(odev) if f.dim() > 1 else f[b:b + 1].to(odev) for f in got])
    b = 0
    dens, parent, labels = got.density[:, b], got.parent[:, b].long(), got.labels[:, b].long()
    lwd = lw.double()
    off = lwd - lwd.max()
    must = off > -87.0                                    # takes part for certain; -inf certainly does not; between: either
    part = parent >= 0
    assert bool(part[must].all()) and not bool(part[torch.isinf(off)].any())
    assert torch.equal(part, labels >= 0) and torch.equal(part, ~torch.isnan(dens)), 'density / parent / labels disagree on who takes part'
    # 1. density
    D, f64 = pairs = _pairs64(ps, lw, bw)
    sel = must
    errs['kernel'] = max(errs['kernel'], ((dens.double() - f64).abs() / f64)[sel].max().item())
    errs['torch32'] = max(errs['torch32'], ((f32 - f64).abs() / f64)[sel].max().item())
    # 2. links, under the exact order of the returned fp32 densities
    idx = torch.arange(S, device=odev)
    cand = part[None, :] & ((dens[None, :] > dens[:, None]) | ((dens[None, :] == dens[:, None]) & (idx[None, :] < idx[:, None])))
    Dc = torch.where(cand, D, torch.full_like(D, float('inf')))
    dmin = Dc.min(1).values
    i = idx[part]
    p = parent[part]
    root = p == i
    assert bool(((p >= 0) & (p < S)).all())
    assert bool(cand[i[~root], p[~root]].all()), 'a parent is not of higher density'
    dp = D[i[~root], p[~root]]
    assert bool((dp <= link * link * (1 + EPS)).all()), 'a parent lies beyond the link radius'
    assert bool((dp <= (1 + EPS) * dmin[i[~root]]).all()), 'a parent is not the nearest candidate'
    assert bool((dmin[i[root]] > link * link * (1 - EPS)).all()), 'a root has a candidate within the link radius'
    # 3. exact consistency
    assert torch.equal(_follow(parent[:, None])[:, 0], labels), 'labels are not the roots of the parent chains'
    lab_live = labels[part]
    assert torch.equal(labels[lab_live], lab_live)
    roots = torch.unique(lab_live)
    nm = int(got.num_modes[b])
    assert nm == roots.numel()
    shown = min(M, nm)
    index, mass, poses = got.index[:, b].long(), got.mass[:, b], got.poses[:, b]
    assert bool((index[shown:] == -1).all()) and bool((mass[shown:] == 0).all()) and bool(torch.isnan(poses[shown:]).all())
    assert torch.equal(torch.sort(index[:shown]).values, torch.unique(index[:shown])) and bool(torch.isin(index[:shown], roots).all())
    assert torch.equal(_bits(poses[:shown]), _bits(ps[index[:shown]])), 'poses are not pose_samples[index, b]'
    w64, W64 = _weights(lw, torch.float64)
    m64 = torch.zeros(S, dtype=torch.float64, device=odev).scatter_add_(0, lab_live, w64[part]) / W64
    bar = _mass_bar(S)
    assert bool(((mass[:shown].double() - m64[index[:shown]]).abs() <= bar).all()), (mass[:shown], m64[index[:shown]])
    assert bool((mass[:shown][1:] <= mass[:shown][:-1]).all()), 'modes are not ordered by mass'
    if nm > shown:
        omitted = m64.clone()
        omitted[index[:shown]] = 0
        assert omitted.max().item() <= mass[shown - 1].item() + bar, 'an omitted mode is heavier than a reported one'
    return labels, must & part, _quick_shift64(ps, lw, bw, link, pairs)[3]


def _check_bad(got, b, tag):
    assert int(got.num_modes[b]) == 0, tag
    assert bool((got.index[:, b] == -1).all()) and bool((got.parent[:, b] == -1).all()) and bool((got.labels[:, b] == -1).all()), tag
    assert bool(torch.isnan(got.mass[:, b]).all()) and bool(torch.isnan(got.density[:, b]).all()) and bool(torch.isnan(got.poses[:, b]).all()), tag


def _to_cpu(got):
    return type(got)(*[f.cpu() for f in got])


def _run_case(device, S, B, dof, lw_half, M=4, link=LINK):
    from epropnp import posterior
    ps, lw, bw, good = _case(S, B, dof, lw_half)
    got = _to_cpu(posterior.modes(ps.to(device), lw.to(device), bw.to(device), max_modes=M, link=link))
    assert got.index.shape == (M, B) and got.index.dtype == torch.int32 and got.poses.shape == (M, B, ps.shape[-1])
    assert got.mass.shape == (M, B) and got.num_modes.shape == (B,) and got.num_modes.dtype == torch.int32
    assert got.labels.shape == got.parent.shape == got.density.shape == (S, B) and got.labels.dtype == got.parent.dtype == torch.int32
    errs = dict(kernel=0.0, torch32=0.0)
    agree = total = 0
    odev = device if (device.type == 'cuda' and S > 2048) else torch.device('cpu')      # (S,S) fp64 matrices: on the GPU where there is one
    for b in range(B):
        if b not in good:
            _check_bad(got, b, f'column {b} ({EDGE[b]})')
            continue
        labels, must, want = _check_object(got, ps[:, b], lw[:, b], bw[b], b, M, link, errs, odev)
        agree += int((labels[must] == want[must]).sum())
        total += int(must.sum())
    print(f'modes S={S} B={B} dof={dof} logw +-{lw_half:g}: density rel err kernel {errs["kernel"]:.3e}, fp32 torch {errs["torch32"]:.3e}; '
          f'labels equal to the fp64 restatement: {agree} of {total}; modes per object {got.num_modes[good].float().mean().item():.1f}')
    assert errs['kernel'] <= DENSITY_FACTOR * errs['torch32'], errs
    return got


@pytest.mark.parametrize('lw_half', [40.0, 4.0])
@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('S,B', SMALL)
def test_density_links_and_consistency(backend, poisoned_empty, S, B, dof, lw_half):
    """Items 1 - 3 of the contract on every good column, the specified fill on the bad ones, every element written (poisoned_empty).
    Density against fp64 within 4 x the error of the fp32 torch statement at the same inputs; every link allowed under the exact
    order of the returned densities and nearest / within the radius to 64 * 2^-24 in fp64; labels, counts, gathers exact; masses
    within (2 * 88 + S + 8) * 2^-24 of the fp64 sums over the kernel's labels.

    Largest density errors measured (kernel / fp32 torch), on the CPU emulation and on the MI355X: beside DENSITY_FACTOR above."""
    _run_case(backend, S, B, dof, lw_half)


@pytest.mark.gpu
@pytest.mark.parametrize('S,B,dof', [(4096, 2, 4), (4096, 2, 6), (6000, 2, 6)])
def test_large_columns(poisoned_empty, S, B, dof):
    """The same checks at the largest LDS-resident column, split over several workgroups per object, and at a column that streams
    through LDS in tiles."""
    import install as emu
    emu.uninstall()
    _run_case(torch.device('cuda:0'), S, B, dof, 40.0)


@pytest.mark.parametrize('dof', [4, 6])
def test_split_and_streamed_tiles_give_the_same_bits(backend, poisoned_empty, monkeypatch, dof):
    """(510,6) with one sample per lane, three workgroups per object and tiles of 100 samples, and with two samples per lane, two
    workgroups, tiles of 257 and the labels in global memory instead of LDS (EPROPNP_TUNE: modes_plan, modes_tile, modes_label_global)
    against the default plan: every output bit for bit."""
    from epropnp import posterior
    ps, lw, bw, _ = _case(510, 6, dof, 40.0)
    dev = [t.to(backend) for t in (ps, lw, bw)]
    base = posterior.modes(*dev)
    monkeypatch.setenv('EPROPNP_TUNE', 'modes_plan=1,3;modes_tile=100')
    other = posterior.modes(*dev)
    monkeypatch.setenv('EPROPNP_TUNE', 'modes_plan=2,2;modes_tile=257;modes_label_global')
    third = posterior.modes(*dev)
    for a, b, c in zip(base, other, third):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


def test_bad_bandwidths_and_more_modes_than_rows(backend, poisoned_empty):
    """A bandwidth that is 0, negative, NaN or inf makes its column bad and leaves the neighbours alone; with a bandwidth far below
    the sample spacing every sample is its own mode: num_modes = S exceeds max_modes and the heaviest samples are reported."""
    from epropnp import posterior
    S, B = 64, 6
    ps, lw, _, _ = _case(S, B, 6, 4.0)
    bw = torch.tensor([[0.5, 0.2], [0.0, 0.2], [0.5, -1.0], [float('nan'), 0.2], [0.5, float('inf')], [1e-4, 1e-4]])
    got = _to_cpu(posterior.modes(ps.to(backend), lw.to(backend), bw.to(backend), max_modes=3))
    for b in (1, 2, 3, 4):
        _check_bad(got, b, f'bandwidth {bw[b].tolist()}')
    errs = dict(kernel=0.0, torch32=0.0)
    for b in (0, 5):
        _check_object(got, ps[:, b], lw[:, b], bw[b], b, 3, LINK, errs)
    assert int(got.num_modes[5]) == S
    assert torch.equal(got.index[:, 5].long(), torch.sort(lw[:, 5], descending=True, stable=True).indices[:3])


# ---- planted clusters -------------------------------------------------------------------------------------------------
def _planted(S, B, dof, seed):
    """4-DoF: two clusters pi apart in yaw; 6-DoF: three -- a base pose, the base turned by pi about the object's x axis, the base
    shifted 2.0 in x.  sigma_t 0.05, yaw noise 0.03 rad / quaternion component noise 0.015, every second quaternion negated,
    log-weights uniform in +-3."""
    g = torch.Generator().manual_seed(seed)
    n = 2 if dof == 4 else 3
    which = torch.randint(0, n, (S, B), generator=g)
    which[:n] = torch.arange(n)[:, None]                               # no cluster is empty
    t = torch.tensor(CENTER) + torch.randn(B, 3, generator=g) + 0.05 * torch.randn(S, B, 3, generator=g)
    if dof == 4:
        yaw = torch.rand(B, generator=g) * 6.0 - 3.0 + math.pi * which + 0.03 * torch.randn(S, B, generator=g)
        rot = yaw[..., None]
    else:
        q0 = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
        w, x, y, z = q0.unbind(-1)
        turned = torch.stack((-x, w, z, -y), -1)                       # q0 * (0, 1, 0, 0): a half turn about the object's x axis
        base = torch.where((which == 1)[..., None], turned, q0)
        rot = torch.nn.functional.normalize(base + 0.015 * torch.randn(S, B, 4, generator=g), dim=-1)
        rot[1::2] = -rot[1::2]
        t[..., 0] += 2.0 * (which == 2)
    lw = torch.rand(S, B, generator=g) * 6.0 - 3.0
    return torch.cat((t, rot), -1).contiguous(), lw, which


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('S,B', [(64, 3), (510, 5)])
def test_planted_clusters(backend, poisoned_empty, S, B, dof):
    """Bandwidth (0.1, 0.06), link 3.  Precondition on the fp64 restatement: the largest parent D is <= link^2 / 2 and the smallest
    D between clusters is >= 2 link^2.  Then the number of modes, the partition of the samples and the masses (the planted softmax
    masses, within the mass bar) are those planted -- unconditionally."""
    from epropnp import posterior
    ps, lw, which = _planted(S, B, dof, seed=11 + S + dof)
    bw = torch.tensor([0.1, 0.06])
    n = 2 if dof == 4 else 3
    for b in range(B):
        _, parent, pd, labels = _quick_shift64(ps[:, b], lw[:, b], bw)
        D = _pair_d(ps[:, b], bw, torch.arange(S), torch.float64)
        between = D[which[:, b, None] != which[None, :, b]].min().item()
        print(f'planted S={S} dof={dof} object {b}: largest parent D {pd.max().item():.2f}, smallest D between clusters {between:.1f}')
        assert pd.max().item() <= LINK * LINK / 2 and between >= 2 * LINK * LINK
        assert torch.unique(labels).numel() == n
    got = _to_cpu(posterior.modes(ps.to(backend), lw.to(backend), (0.1, 0.06), max_modes=4, link=LINK))
    assert bool((got.num_modes == n).all()), got.num_modes
    soft = torch.softmax(lw.double(), dim=0)
    for b in range(B):
        labels = got.labels[:, b].long()
        same = labels[:, None] == labels[None, :]
        assert torch.equal(same, which[:, b, None] == which[None, :, b]), 'the labels do not partition the samples as planted'
        for m in range(n):
            k = which[got.index[m, b], b]
            assert abs(got.mass[m, b].item() - soft[which[:, b] == k, b].sum().item()) <= _mass_bar(S)
        assert int(got.index[n, b]) == -1


# ---- through the layer ------------------------------------------------------------------------------------------------
def _layer(backend, dof, with_modes):
    from epropnp import posterior
    from epropnp.epropnp import EProPnP4DoF, EProPnP6DoF
    from epropnp.levenberg_marquardt import LMSolver
    S, K = 512, 4
    if dof == 4:
        # objects whose correspondence set is closed under a half turn about the vertical axis: two posterior peaks pi apart
        B = 6
        prob = orc.make_problem(B, 64, 4, seed=3)
        half = prob['x3d'].shape[1] // 2
        flip = torch.tensor([-1.0, 1.0, -1.0], dtype=prob['x3d'].dtype)
        prob['x3d'][:, half:] = prob['x3d'][:, :half] * flip
        prob['x2d'][:, half:] = prob['x2d'][:, :half]
        prob['w2d'][:, half:] = prob['w2d'][:, :half]
        prob['w2d'] = prob['w2d'] * 3
        L, bw = 5, (1.0, 0.5)
    else:
        B = 5
        prob = orc.make_problem(B, 96, 6, seed=3)
        L, bw = 3, (0.1, 0.05)
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=4), dof).to(backend)
    p, cam, cf = make_layer_objects(prob, backend, relative_delta=0.5)
    cf.set_param(p['x2d'], p['w2d'])
    layer = (EProPnP6DoF if dof == 6 else EProPnP4DoF)(mc_samples=S, num_iter=K, solver=LMSolver(dof=dof, num_iter=L))
    out = layer.monte_carlo_forward(p['x3d'], p['x2d'], p['w2d'], cam, cf, pose_init=p['pose_init'], force_init_solve=False, noise=noise, fast_mode=True)
    got = posterior.modes(out[3], out[4], bw) if with_modes else None
    return out, got, bw


@pytest.mark.parametrize('dof', [4, 6])
def test_through_the_layer(backend, poisoned_empty, dof):
    """monte_carlo_forward on the symmetric 4-DoF objects, then modes(..., (1.0, 0.5)): for every object the two heaviest modes are
    within h_r of pi apart in yaw, hold >= 0.95 of the mass together and the second >= 0.05 (the fp64 oracle: <= 0.13 rad, > 0.99,
    >= 0.15).  A plain 6-DoF problem at (0.1, 0.05): the heaviest mode holds >= 0.9 (oracle 0.94 .. 1.0).  The layer's outputs are
    torch.equal with and without the call."""
    plain, _, _ = _layer(backend, dof, False)
    out, got, bw = _layer(backend, dof, True)
    for a, b in zip(plain, out):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    got = _to_cpu(got)
    if dof == 4:
        yaw = got.poses[:2, :, 3].double()
        apart = ((yaw[0] - yaw[1] + math.pi) % (2 * math.pi) - math.pi).abs()
        print(f'through the layer 4-DoF: modes {got.num_modes.tolist()}, |dyaw| - pi {(apart - math.pi).abs().max().item():.3f}, '
              f'masses {got.mass[0].tolist()} / {got.mass[1].tolist()}')
        assert bool((got.num_modes >= 2).all())
        assert bool(((apart - math.pi).abs() <= bw[1]).all())
        assert bool(((got.mass[0] + got.mass[1]) >= 0.95).all()) and bool((got.mass[1] >= 0.05).all())
    else:
        print(f'through the layer 6-DoF: modes {got.num_modes.tolist()}, heaviest masses {got.mass[0].tolist()}')
        assert bool((got.mass[0] >= 0.9).all())


# ---- determinism, hipGraph, refusals ------------------------------------------------------------------------------------
def _twice(device, S, B, dof):
    from epropnp import posterior
    ps, lw, bw, _ = _case(S, B, dof, 40.0)
    dev = [t.to(device) for t in (ps, lw, bw)]
    a, b = posterior.modes(*dev), posterior.modes(*dev)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), 'two launches differ'


@pytest.mark.parametrize('dof', [4, 6])
def test_two_launches_agree_in_every_bit(backend, poisoned_empty, dof):
    _twice(backend, 128, 300, dof)


@pytest.mark.gpu
@pytest.mark.parametrize('dof', [4, 6])
def test_two_launches_agree_in_every_bit_large_column(poisoned_empty, dof):
    import install as emu
    emu.uninstall()
    _twice(torch.device('cuda:0'), 4096, 2, dof)


def _graph_body():
    from epropnp import posterior
    dev = torch.device('cuda:0')
    for dof, (S, B) in ((4, (510, 70)), (6, (510, 70)), (6, (4096, 2))):
        ps, lw, bw, _ = _case(S, B, dof, 40.0)
        ps, lw, bw = ps.to(dev), lw.to(dev), bw.to(dev)

        def body():
            return tuple(posterior.modes(ps, lw, bw)) + tuple(posterior.modes(ps, lw, (0.5, 0.2), max_modes=2))

        eager = [t.clone() for t in body()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = body()
        for t in outs:
            t.fill_(float('nan') if t.is_floating_point() else -7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(_bits(a), _bits(b)), f'dof {dof} S {S}: replay differs from the eager call'
        del graph, outs
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_modes_replay_from_a_hip_graph():
    """modes (tensor and float bandwidths) captured into one torch.cuda.graph, replayed once: bit-equal to the eager calls.  Own
    interpreter, as tests/test_posterior.py: keeps graph / private-pool teardown away from the other GPU tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys; sys.path[:0] = [%r, %r, %r]; import test_posterior_modes as t; t._graph_body(); '
            'print("MODES-GRAPH-OK", flush=True)') % (here, os.path.join(os.path.dirname(here), 'oracle'),
                                                       os.path.join(os.path.dirname(here), 'epro-pnp_amd'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'MODES-GRAPH-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_refuses_other_dtypes_shapes_and_sizes(backend):
    from epropnp import posterior
    ps, lw = torch.zeros(8, 3, 7, device=backend), torch.zeros(8, 3, device=backend)
    bw = torch.ones(3, 2, device=backend)
    for args in ((ps.double(), lw, bw), (ps, lw.half(), bw), (ps, lw, bw.double()), (ps, lw, (bw[:, 0].double(), 0.5))):
        with pytest.raises(TypeError):
            posterior.modes(*args)
    for args in ((ps[..., :5].contiguous(), lw, bw), (ps, lw[:4], bw), (ps, lw, bw[:2]), (ps, lw, torch.ones(3, 3, device=backend)),
                 (ps, lw, (bw[:2, 0], 0.5)), (ps, lw, 0.5), (ps, lw, (0.5, 0.2, 0.1))):
        with pytest.raises(ValueError):
            posterior.modes(*args)
    for kw in (dict(max_modes=0), dict(link=0.0), dict(link=float('inf')), dict(link=float('nan')), dict(link=-1.0)):
        with pytest.raises(ValueError):
            posterior.modes(ps, lw, bw, **kw)
    out = posterior.modes(ps.clone().requires_grad_(True), lw.clone().requires_grad_(True), bw.clone().requires_grad_(True))
    assert not any(t.requires_grad for t in out)
    mixed = posterior.modes(ps, lw, (bw[:, 0], 1.0))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(mixed, posterior.modes(ps, lw, (1.0, 1.0))))


def test_refuses_cpu_tensors_without_a_fallback():
    from epropnp import posterior
    import install as emu
    assert not emu.installed()
    with pytest.raises(RuntimeError, match='HIP device'):
        posterior.modes(torch.zeros(8, 3, 4), torch.zeros(8, 3), (1.0, 0.5))


def test_empty_batch_returns_empty_tensors_without_a_launch(backend, monkeypatch):
    from epropnp import _hip, posterior
    monkeypatch.setattr(_hip, 'call', lambda *a: (_ for _ in ()).throw(AssertionError('launched for an empty batch')))
    for P in (4, 7):
        got = posterior.modes(torch.zeros(8, 0, P, device=backend), torch.zeros(8, 0, device=backend), (1.0, 0.5), max_modes=3)
        assert got.index.shape == (3, 0) and got.poses.shape == (3, 0, P) and got.mass.shape == (3, 0) and got.num_modes.shape == (0,)
        assert got.labels.shape == got.parent.shape == got.density.shape == (8, 0)
