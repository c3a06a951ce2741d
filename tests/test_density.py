"""epropnp.posterior.orient_density / bev_density (epropnp_orient_density, epropnp_bev_density) against fp64 oracles written here.

The oracle is decision-conditioned: every call asks for `bins`, the bin each point fell into.  (a) The decisions are checked
against fp64 geometry: the fp64 coordinate lies within 0.5 + 16 size 2^-24 px of the bin's centre (about six roundings in the
rotation column times 0.4 size, plus the rounding of the result; for the BEV grid one rounding of the product: 0.5 + 2 |v| 2^-24),
a dropped point lies outside the canvas by the same measure, and the hemisphere agrees wherever |a_z| > 16 2^-24.  (b) The
densities (and the sphere's image) are rebuilt in fp64 from the kernel's OWN bins and an fp64 softmax -- scatter, zero-padded box
sum, colour composite -- and compared: a pixel that is 0 in the oracle must be exactly 0, elsewhere |d - d64| <= DENS_BAR d64,
and |image - image64| <= IMG_BAR.  So the comparison is tight at any size without fenced seeds.

For the BEV half no run of the reference is possible (its `show_bev` needs cv2, which is not installed): the fp64 bincount + box sum
below is its yardstick.  cv2.blur reflects at the border where the kernel pads with zeros; the oracle pads with zeros too.

Bars: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over every case of this file (they are
printed by each case), under the caps 1e-4 (density, relative) and 1e-3 (image, absolute: a quarter of an 8-bit step).
    density  |d - d64| / d64        emulation 6.632e-7, MI355X 6.632e-7   -> bar 2.66e-6
    image    |image - image64|      emulation 1.788e-7, MI355X 1.788e-7   -> bar 7.16e-7
The image figure counts tests/test_density_reference.py, which compares with the reference's fp32 picture at the same bar and holds
the worst case (against fp64 alone: emulation 1.295e-7, MI355X 1.252e-7).
"""
import numpy as np
import pytest
import torch

DENS_BAR = 2.66e-6       # relative; cap 1e-4
IMG_BAR = 7.16e-7        # absolute; cap 1e-3
DENS_CAP, IMG_CAP = 1e-4, 1e-3
EPS = 2.0 ** -24
_worst = {'density': 0.0, 'image': 0.0}


def _post():
    from epropnp import posterior
    return posterior


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_bars_are_under_their_caps():
    assert 0 < DENS_BAR <= DENS_CAP and 0 < IMG_BAR <= IMG_CAP


# ---- fp64 oracles ----------------------------------------------------------------------------------------------------------------
def rot64(q):
    """(...,4) [w,x,y,z], not normalised -> (...,3,3): 2 (w [v]x + v v^T) + (w^2 - v.v) I"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    dd = w * w - (x * x + y * y + z * z)
    R = np.stack((2 * x * x + dd, 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 2 * y * y + dd, 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 2 * z * z + dd), -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def softmax64(logw):
    """(S,B) -> fp64 softmax over S; NaN columns where the kernel calls the column bad"""
    lw = np.asarray(logw, dtype=np.float64)
    with np.errstate(all='ignore'):
        m = lw.max(0, keepdims=True)
        e = np.exp(lw - m)
        w = e / e.sum(0, keepdims=True)
    bad = np.isnan(lw).any(0) | (lw == np.inf).any(0) | (lw == -np.inf).all(0)
    w[:, bad] = np.nan
    return w, bad


def box_sum64(raw, kh, kw):
    """(..., H, W) -> zero-padded (kh, kw) box sum"""
    H, W = raw.shape[-2:]
    pad = np.zeros(raw.shape[:-2] + (H + kh - 1, W + kw - 1))
    pad[..., kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = raw
    out = np.zeros_like(raw)
    for dy in range(kh):
        for dx in range(kw):
            out += pad[..., dy:dy + H, dx:dx + W]
    return out


def circle32(size):
    """the reference's circle mask, in its fp32 arithmetic"""
    c, r = np.float32(size / 2 - 0.5), np.float32(size) * np.float32(0.4)
    wh = (np.arange(size, dtype=np.float32) - c) / r
    s = wh * wh
    return (s[None, :] + s[:, None]) <= np.float32(1.0)


def layer64(dens, saturation, intensity):
    """(...,3) densities -> prod_k col[k,c] ** (intensity dens_k)"""
    col = np.eye(3) * float(np.float32(saturation)) + (1 - float(np.float32(saturation))) / 2
    with np.errstate(all='ignore'):
        return np.prod(col ** (float(np.float32(intensity)) * dens[..., :, None]), -2)


def check_sphere_bins(quat, bins, size):
    """(a): the kernel's decisions against fp64 geometry"""
    S, B = bins.shape[:2]
    R = rot64(quat)                                            # (S,B,3,3); axis k = column k
    r, c = 0.4 * size, size / 2 - 0.5
    fx, fy, az = R[..., 0, :] * r + c, R[..., 1, :] * r + c, R[..., 2, :]
    slack = 0.5 + 16 * size * EPS
    kept = bins >= 0
    hemi = bins >= size * size
    pix = np.where(kept, bins - hemi * size * size, 0)
    py, px = pix // size, pix % size
    assert (bins[kept] < 2 * size * size).all()
    assert (np.abs(fx - px)[kept] <= slack).all() and (np.abs(fy - py)[kept] <= slack).all()
    sure = kept & (np.abs(az) > 16 * EPS)
    assert (hemi[sure] == (az[sure] > 0)).all()
    lo, hi = -0.5 + (slack - 0.5), size - 0.5 - (slack - 0.5)
    with np.errstate(invalid='ignore'):
        outside = ~np.isfinite(fx) | ~np.isfinite(fy) | ~np.isfinite(az) | (fx <= lo) | (fx >= hi) | (fy <= lo) | (fy >= hi)
    assert outside[~kept].all()


def sphere64(logw, bins, size, window, saturation, opacity, intensity):
    """(b): front, back, image in fp64 from the kernel's bins"""
    S, B = bins.shape[:2]
    w, bad = softmax64(logw)
    raw = np.zeros((B, 2 * size * size, 3))
    for k in range(3):
        for b in range(B):
            kept = bins[:, b, k] >= 0
            np.add.at(raw[b, :, k], bins[kept, b, k], np.where(bad[b], 0.0, w[kept, b]))
    raw = raw.reshape(B, 2, size, size, 3).transpose(0, 1, 4, 2, 3)      # (B, hemi, k, y, x)
    dens = box_sum64(raw, *window).transpose(0, 1, 3, 4, 2)              # (B, hemi, y, x, k)
    dens[bad] = np.nan
    front, back = dens[:, 0], dens[:, 1]
    circle = 1.0 - 0.5 * circle32(size)
    o = float(np.float32(opacity))
    base = layer64(back, saturation, intensity) * o + circle[None, :, :, None] * (1 - o)
    return front, back, base, layer64(front, saturation, intensity)


def compare_density(d, d64, what):
    d = d.double().cpu().numpy()
    nan = np.isnan(d64)
    assert (np.isnan(d) == nan).all(), f'{what}: NaN pattern'
    zero = (d64 == 0) & ~nan
    assert (d[zero] == 0).all(), f'{what}: a pixel without a hit is not exactly 0'
    live = ~zero & ~nan
    err = float((np.abs(d - d64)[live] / d64[live]).max(initial=0.0))
    _worst['density'] = max(_worst['density'], err)
    print(f'{what}: worst relative density error {err:.3e} (so far {_worst["density"]:.3e})')
    assert err <= DENS_BAR, f'{what}: relative error {err:.3e} > {DENS_BAR:.3e}'


def compare_image(img, img64, what, where=None):
    img = img.double().cpu().numpy()
    nan = np.isnan(img64)
    assert (np.isnan(img) == nan).all(), f'{what}: NaN pattern'
    live = ~nan if where is None else (~nan & where)
    err = float(np.abs(img - img64)[live].max(initial=0.0))
    _worst['image'] = max(_worst['image'], err)
    print(f'{what}: worst image error {err:.3e} (so far {_worst["image"]:.3e})')
    assert err <= IMG_BAR, f'{what}: image error {err:.3e} > {IMG_BAR:.3e}'


# ---- sphere cases ----------------------------------------------------------------------------------------------------------------
def quats(S, B, seed, spread=0.3):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, B, 4, generator=g)
    q = base + spread * torch.randn(S, B, 4, generator=g)
    return q / q.norm(dim=-1, keepdim=True)


def samples(S, B, seed, spread=0.3):
    g = torch.Generator().manual_seed(seed + 1000)
    pose = torch.cat((torch.randn(S, B, 3, generator=g), quats(S, B, seed, spread)), -1)
    return pose.contiguous(), (2.0 * torch.randn(S, B, generator=g)).contiguous()


def _case_identical():
    pose, logw = samples(70, 2, 11)
    return pose[:1].expand(70, 2, 7).contiguous(), logw, 48, (5, 5)


def _case_scaled():
    """points on pixel 0, on pixel size - 1 and just outside, from scaled quaternions (the rotation scales with |q|^2)"""
    size = 64
    r, c = 0.4 * size, size / 2 - 0.5
    scales = [c / r, (c + 0.4) / r, (c + 0.6) / r, 2.0, 0.5]
    rows = []
    for s2 in scales:
        s = s2 ** 0.5
        rows += [[0, 0, 0, s, 0, 0, 0], [0, 0, 0, 0, 0, 0, s], [0, 0, 0, 0, s, 0, 0], [0, 0, 0, 0, 0, s, 0]]
    pose = torch.tensor(rows, dtype=torch.float32)[:, None, :].repeat(1, 2, 1)
    pose[:, 1, 3:] = pose[:, 1, 3:] * 0.97 + 0.02
    g = torch.Generator().manual_seed(5)
    return pose.contiguous(), torch.randn(pose.shape[0], 2, generator=g), size, (3, 3)


def _case_bad_columns():
    pose, logw = samples(40, 3, 12)
    logw[7, 0] = float('nan')
    logw[:, 1] = float('-inf')
    logw[3, 2] = float('-inf')
    return pose, logw, 40, (5, 5)


SPHERE_CASES = {
    's1': lambda: samples(1, 1, 1) + (16, (1, 1)),
    's33': lambda: samples(33, 2, 2) + (64, (5, 5)),
    's255': lambda: samples(255, 2, 3, 0.6) + (65, (5, 5)),
    's256': lambda: samples(256, 2, 4, 0.6) + (65, (5, 5)),
    's257': lambda: samples(257, 2, 5, 0.6) + (65, (5, 5)),
    's512': lambda: samples(512, 5, 6, 0.5) + (97, (7, 3)),
    's1100': lambda: samples(1100, 1, 7, 0.6) + (33, (3, 9)),      # beyond the samples a thread keeps in registers
    'identical': _case_identical,
    'scaled': _case_scaled,
    'bad_columns': _case_bad_columns,
}
PARAMS = dict(saturation=0.5, sphere_opacity=0.6, intensity_scale=50)


@pytest.mark.parametrize('name', list(SPHERE_CASES))
def test_sphere_against_the_fp64_oracle(backend, name):
    pose, logw, size, window = SPHERE_CASES[name]()
    res = _post().orient_density(pose.to(backend), logw.to(backend), size=size, window=window, with_density=True, with_bins=True, **PARAMS)
    bins = res.bins.cpu().numpy().astype(np.int64)
    check_sphere_bins(pose[..., 3:].numpy(), bins, size)
    front, back, base, front_layer = sphere64(logw.numpy(), bins, size, window, PARAMS['saturation'], PARAMS['sphere_opacity'],
                                              PARAMS['intensity_scale'])
    if name == 'identical':
        assert (bins == bins[:1]).all() and (bins >= 0).all()
    if name == 'scaled':
        kept = bins[:, 0, :] >= 0
        pix = bins[:, 0, :] % (size * size)
        assert (~kept).any() and ((pix % size == 0) & kept).any() and ((pix % size == size - 1) & kept).any()
        assert ((pix // size == 0) & kept).any() and ((pix // size == size - 1) & kept).any()
    if name == 'bad_columns':
        assert torch.isnan(res.image[:2]).all() and torch.isnan(res.front[:2]).all() and torch.isnan(res.back[:2]).all()
        assert torch.isfinite(res.image[2]).all()
    compare_density(res.front, front, f'{name} front')
    compare_density(res.back, back, f'{name} back')
    compare_image(res.image, base * front_layer, f'{name} image')


def test_sphere_without_objects(backend):
    res = _post().orient_density(torch.zeros(4, 0, 7, device=backend), torch.zeros(4, 0, device=backend), size=16, with_density=True,
                                 with_bins=True)
    assert res.image.shape == (0, 16, 16, 3) and res.front.shape == (0, 16, 16, 3) and res.bins.shape == (4, 0, 3)


def test_sphere_mass_and_determinism(backend):
    """unit quaternions, size >= 5 max(window): no point within a window of the border, so every plane holds kh kw in all; two
    launches agree bit for bit"""
    pose, logw = samples(33, 2, 2)
    one = _post().orient_density(pose.to(backend), logw.to(backend), size=64, window=(5, 3), with_density=True, with_bins=True)
    two = _post().orient_density(pose.to(backend), logw.to(backend), size=64, window=(5, 3), with_density=True, with_bins=True)
    total = (one.front.double() + one.back.double()).sum((1, 2)).cpu().numpy()
    assert np.abs(total / 15.0 - 1.0).max() <= 1e-5, total
    for x, y in zip(one, two):
        assert torch.equal(_bits(x), _bits(y))


def _segment_dist64(size, quat):
    """(3, size, size): distance of every pixel centre from the three axis segments of one pose"""
    R = rot64(quat)
    r, c = 0.4 * size, size / 2 - 0.5
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing='ij')
    out = []
    for k in range(3):
        dx, dy = R[0, k] * r, R[1, k] * r
        t = np.clip(((xx - c) * dx + (yy - c) * dy) / max(dx * dx + dy * dy, 1e-300), 0.0, 1.0)
        out.append(np.hypot(xx - c - t * dx, yy - c - t * dy))
    return np.stack(out)


def test_sphere_axis_lines(backend):
    """pose_opt draws its three axes: away from them (> 1.51 px) the bits of the picture without lines; where exactly one segment is
    within 1.49 px and no later one within 1.51 px the axis' colour times front_layer"""
    pose, logw = samples(64, 2, 21)
    size, window = 48, (5, 5)
    opt = torch.cat((torch.zeros(2, 3), quats(1, 2, 77)[0]), -1).contiguous()
    plain = _post().orient_density(pose.to(backend), logw.to(backend), size=size, window=window, with_density=True, **PARAMS)
    lined = _post().orient_density(pose.to(backend), logw.to(backend), pose_opt=opt.to(backend), size=size, window=window, **PARAMS)
    front_layer = layer64(plain.front.double().cpu().numpy(), PARAMS['saturation'], PARAMS['intensity_scale'])
    a, b = _bits(plain.image).cpu().numpy(), _bits(lined.image).cpu().numpy()
    img = lined.image.double().cpu().numpy()
    for i in range(2):
        dist = _segment_dist64(size, opt[i, 3:].numpy())
        away = (dist > 1.51).all(0)
        assert away.any() and (a[i][away] == b[i][away]).all()
        seen = 0
        for j in range(3):
            sure = (dist[j] < 1.49) & ((dist < 1.49).sum(0) == 1) & (dist[j + 1:] > 1.51).all(0)
            seen += int(sure.sum())
            want = np.zeros((size, size, 3))
            want[..., j] = front_layer[i, ..., j]
            others = [ch for ch in range(3) if ch != j]
            assert (img[i][sure][:, others] == 0).all()
            err = float(np.abs(img[i] - want)[sure].max(initial=0.0))
            _worst['image'] = max(_worst['image'], err)
            print(f'axis {j} of object {i}: worst image error on the line {err:.3e}')
            assert err <= IMG_BAR
        assert seen > 30


def test_sphere_writes_every_element(backend, poisoned_empty):
    pose, logw = samples(20, 2, 31)
    res = _post().orient_density(pose.to(backend), logw.to(backend), size=37, window=(3, 5), with_density=True, with_bins=True)
    for t in (res.image, res.front, res.back):
        assert torch.isfinite(t).all()
    assert (res.bins >= -1).all()


@pytest.mark.gpu
def test_sphere_graph_capture_replays_to_the_same_bits():
    import install as emu
    emu.uninstall()
    d = torch.device('cuda:0')
    pose, logw = samples(257, 2, 41, 0.6)
    pose, logw = pose.to(d), logw.to(d)
    opt = pose[0].clone()
    call = lambda: _post().orient_density(pose, logw, pose_opt=opt, size=65, with_density=True, with_bins=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    pose2, logw2 = samples(257, 2, 42, 0.6)
    pose.copy_(pose2.to(d))
    logw.copy_(logw2.to(d))
    graph.replay()
    eager = call()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(_bits(x), _bits(y))


# ---- BEV -------------------------------------------------------------------------------------------------------------------------
def bev_scene(S, dof, H, W, scale, origin, G, seed):
    """objects of G groups (one of them empty when G > 1), out of group order, their samples spilling over every side of the grid"""
    g = torch.Generator().manual_seed(seed)
    ox, oy = origin
    spots = [(W / 2, H / 2), (0.0, H / 2), (W - 1.0, H / 2), (W / 2, 0.0), (W / 2, H - 1.0), (-3.0, -3.0), (W + 2.0, H + 2.0),
             (W / 3, H / 3), (2 * W / 3, H / 4)]
    B = len(spots)
    centre = torch.tensor(spots, dtype=torch.float64)
    z0, x0 = (centre[:, 0] - ox) / scale, (centre[:, 1] - oy) / scale
    P = 4 if dof == 4 else 7
    pose = torch.randn(S, B, P, generator=g)
    pose[..., 0] = x0.float()[None] + (1.5 / scale) * torch.randn(S, B, generator=g)
    pose[..., 2] = z0.float()[None] + (1.5 / scale) * torch.randn(S, B, generator=g)
    logw = 2.0 * torch.randn(S, B, generator=g)
    groups = torch.tensor([(5 * i + 2) % G for i in range(B)], dtype=torch.int64)
    if G > 1:
        groups[groups == 1] = 0                                # group 1 stays empty
    score = torch.rand(B, generator=g) + 0.1
    return pose.contiguous(), logw.contiguous(), groups, score


def check_bev_bins(pose, bins, H, W, scale, origin):
    z, x = pose[..., 2].double().numpy(), pose[..., 0].double().numpy()
    s = float(np.float32(scale))
    fx, fy = z * s + origin[0], x * s + origin[1]
    kept = bins >= 0
    py, px = np.where(kept, bins, 0) // W, np.where(kept, bins, 0) % W
    sx, sy = 0.5 + 2 * np.abs(z * s) * EPS, 0.5 + 2 * np.abs(x * s) * EPS
    assert (bins[kept] < H * W).all()
    assert (np.abs(fx - px) <= sx)[kept].all() and (np.abs(fy - py) <= sy)[kept].all()
    outside = (fx <= -1 + sx) | (fx >= W - sx) | (fy <= -1 + sy) | (fy >= H - sy)
    assert outside[~kept].all()


def bev64(logw, bins, groups, score, G, H, W, window):
    S, B = bins.shape
    w, bad = softmax64(logw)
    raw = np.zeros((G, H * W))
    for b in range(B):
        g = int(groups[b])
        if bad[b] or not 0 <= g < G:
            continue
        kept = bins[:, b] >= 0
        raw[g] += np.bincount(bins[kept, b], weights=w[kept, b] * score[b], minlength=H * W)
    return box_sum64(raw.reshape(G, H, W), window, window)


@pytest.mark.parametrize('grid', [(1, 1), (48, 80), (70, 130)])
@pytest.mark.parametrize('G,dof,window,weighted', [(1, 4, 3, True), (3, 6, 1, False), (3, 4, 3, True), (1, 6, 3, False)])
def test_bev_against_the_fp64_oracle(backend, grid, G, dof, window, weighted):
    H, W = grid
    scale, origin = 4.0, (int(W / 16), int(H / 2))
    pose, logw, groups, score = bev_scene(300 if grid == (70, 130) else 40, dof, H, W, scale, origin, G, seed=H + G)
    logw[5, 7] = float('nan')                                  # one bad column: the object adds nothing
    res = _post().bev_density(pose.to(backend), logw.to(backend), H, W, scale=scale, obj_weight=score.to(backend) if weighted else None,
                              groups=groups.to(backend) if G > 1 else None, num_groups=G, window=window, with_bins=True)
    assert res.density.shape == (G, H, W)
    bins = res.bins.cpu().numpy().astype(np.int64)
    check_bev_bins(pose, bins, H, W, scale, origin)
    if grid != (1, 1):
        assert (bins >= 0).any() and (bins < 0).any()
    sc = score.double().numpy() if weighted else np.ones(len(score))
    want = bev64(logw.numpy(), bins, groups.numpy() if G > 1 else np.zeros(len(score), dtype=np.int64), sc, G, H, W, window)
    compare_density(res.density, want, f'bev {grid} G={G}')
    if G > 1:
        assert (res.density[1] == 0).all()


def test_bev_more_objects_than_one_round(backend):
    """300 objects in one group: the tile kernel sorts objects out 256 at a time"""
    H, W, S, B = 40, 70, 5, 300
    g = torch.Generator().manual_seed(17)
    pose = torch.zeros(S, B, 4)
    pose[..., 0] = (torch.rand(1, B, generator=g) - 0.5) * 12.0 + 0.2 * torch.randn(S, B, generator=g)
    pose[..., 2] = torch.rand(1, B, generator=g) * 18.0 + 0.2 * torch.randn(S, B, generator=g)
    logw = torch.randn(S, B, generator=g)
    score = torch.rand(B, generator=g) + 0.1
    groups = torch.zeros(B, dtype=torch.int64)
    groups[::7] = 1
    res = _post().bev_density(pose.to(backend), logw.to(backend), H, W, scale=4.0, obj_weight=score.to(backend),
                              groups=groups.to(backend), num_groups=2, window=5, with_bins=True)
    bins = res.bins.cpu().numpy().astype(np.int64)
    check_bev_bins(pose, bins, H, W, 4.0, (int(W / 16), int(H / 2)))
    assert int((groups == 0).sum()) > 256 and (bins >= 0).mean() > 0.5
    compare_density(res.density, bev64(logw.numpy(), bins, groups.numpy(), score.double().numpy(), 2, H, W, 5), 'bev 300 objects')


def test_bev_mass(backend):
    """sum density[g] = window^2 sum_{b in g} obj_weight[b] (weight share on the grid), no hit within window // 2 of the border"""
    H, W, S = 48, 80, 64
    g = torch.Generator().manual_seed(3)
    pose = torch.zeros(S, 4, 4)
    pose[..., 0] = 0.4 * torch.randn(S, 4, generator=g)
    pose[..., 2] = 4.0 + 0.4 * torch.randn(S, 4, generator=g)
    pose[:5, 1, 2] = 400.0                                     # five samples of object 1 leave the grid
    logw = torch.randn(S, 4, generator=g)
    score = torch.tensor([0.9, 0.5, 0.3, 0.7])
    groups = torch.tensor([1, 0, 1, 0], dtype=torch.int32)
    res = _post().bev_density(pose.to(backend), logw.to(backend), H, W, scale=4.0, obj_weight=score.to(backend),
                              groups=groups.to(backend), num_groups=2, window=3, with_bins=True)
    bins = res.bins.cpu().numpy()
    py, px = bins // W, bins % W
    kept = bins >= 0
    assert (~kept[:, 1]).sum() == 5 and kept[:, [0, 2, 3]].all()
    assert ((py >= 1) & (py < H - 1) & (px >= 1) & (px < W - 1))[kept].all()
    w, _ = softmax64(logw.numpy())
    share = (w * kept).sum(0) * score.double().numpy()
    want = np.array([share[1] + share[3], share[0] + share[2]]) * 9.0
    got = res.density.double().sum((1, 2)).cpu().numpy()
    assert np.abs(got / want - 1.0).max() <= 1e-5, (got, want)


def test_bev_determinism_and_every_element(backend, poisoned_empty):
    pose, logw, groups, score = bev_scene(40, 4, 33, 45, 4.0, (2, 16), 3, seed=9)
    call = lambda: _post().bev_density(pose.to(backend), logw.to(backend), 33, 45, scale=4.0, obj_weight=score.to(backend),
                                       groups=groups.to(backend), num_groups=3, with_bins=True)
    one, two = call(), call()
    assert torch.isfinite(one.density).all() and (one.bins >= -1).all()
    assert torch.equal(_bits(one.density), _bits(two.density)) and torch.equal(one.bins, two.bins)
    none = _post().bev_density(torch.zeros(3, 0, 4, device=backend), torch.zeros(3, 0, device=backend), 5, 7, num_groups=2)
    assert none.density.shape == (2, 5, 7) and (none.density == 0).all()
    empty = _post().bev_density(pose.to(backend), logw.to(backend), 5, 7, num_groups=0)
    assert empty.density.shape == (0, 5, 7)
