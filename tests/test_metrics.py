"""epropnp.metrics.pose_errors (epropnp_pose_errors) against fp64 torch on the same fp32 inputs: the reference's expressions
(EPro-PnP-6DoF lib/utils/eval.py:585-736) for rot_deg / trans / arp_2d / add and a brute-force cdist for adi.

Shapes: M in {1, 63, 65, QUERY_TILE - 1, QUERY_TILE + 1, 2 max(QUERY_TILE, CAND_TILE) + 7} -- one point, one wave short and one
point over, one short and one over a query tile, several query and candidate tiles with ragged last ones -- at 3 x 5 rows, and
(R,B) in {(1,1), (3,5), (1,70)} at M = 65; one call mixing three models, both masks set on some objects only; both dof.

Bars: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over every case of this file and of
test_metrics_reference.py.  The caps a bar may not exceed: 2e-4 for add / adi on their scale, 1e-3 px for arp_2d, 1e-4 degrees plus
1e-6 relative for rot_deg, 1e-6 relative plus one ulp of the larger translation for trans; the last two are measured as a
fraction of their cap.
    add, adi   |got - fp64| / (fp64 + 1e-3 model radius)          emulation 2.874e-6, MI355X 2.869e-6   -> bar 1.15e-5
               (three models, 4-DoF; M = 1: 1.80e-6; M >= 63 with one model: 5.0e-7)
    arp_2d     |got - fp64| in pixels                             emulation 1.189e-5, MI355X 1.189e-5   -> bar 4.76e-5
               (the reference fixture's half-turn rows, whose se3_mul rounds the turned pose to fp32; against fp64 torch 6.7e-6)
    rot_deg    |got - fp64| / (1e-4 deg + 1e-6 fp64)              emulation 3.03e-2,  MI355X 3.03e-2    -> bar 0.122
    trans      |got - fp64| / (1e-6 fp64 + ulp(max |t|))          emulation 1.16e-2,  MI355X 1.16e-2    -> bar 0.0464
"""
import math
import os
import re

import pytest
import torch

from helpers import set_tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADD_BAR = 1.15e-5        # on the scale |got - fp64| / (fp64 + 1e-3 radius); cap 2e-4
ARP_BAR = 4.76e-5        # pixels; cap 1e-3
ROT_ABS, ROT_REL = 1e-4, 1e-6      # the cap of rot_deg: 1e-4 degrees plus 1e-6 relative
ROT_BAR = 0.122          # as a fraction of that cap
TRANS_REL = 1e-6         # the cap of trans: 1e-6 relative plus one ulp of the larger translation
TRANS_BAR = 0.0464       # as a fraction of that cap
ANGLES = (1e-3, 0.02, 0.3, 3.0)
K6 = ((600.0, 0.0, 320.0), (0.0, 600.0, 240.0), (0.0, 0.0, 1.0))
K4 = ((1260.0, 0.0, 800.0), (0.0, 1260.0, 450.0), (0.0, 0.0, 1.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _metrics():
    from epropnp import metrics
    return metrics


def _big():
    m = _metrics()
    return 2 * max(m.QUERY_TILE, m.CAND_TILE) + 7


# ---- inputs (CPU, built once per key) ----------------------------------------------------------------------------------------
_models, _cases, _refs = {}, {}, {}


def ellipsoid(M, scale=1.0, seed=0):
    """M points on an ellipsoid of semi-axes 0.05 x 0.08 x 0.03 (times scale), fp32"""
    key = (M, scale, seed)
    if key not in _models:
        g = torch.Generator().manual_seed(77 + 13 * M + seed)
        d = torch.nn.functional.normalize(torch.randn(M, 3, generator=g, dtype=torch.float64), dim=-1)
        _models[key] = (d * torch.tensor([0.05, 0.08, 0.03], dtype=torch.float64) * scale).float()
    return _models[key]


def _qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def make_poses(R, B, dof, seed, depth=None, angles=ANGLES):
    """(pose_est (R,B,P), pose_gt (B,P)) fp32: gt anywhere, est = gt turned by ANGLES[(r + b) % 4] about a random axis (4-DoF: yaw)
    and shifted by 1e-3 .. 3e-2; every second quaternion of est with the opposite sign, none of them of unit length exactly."""
    g = torch.Generator().manual_seed(seed)
    depth = depth if depth is not None else (1.0 if dof == 6 else 50.0)
    centre = torch.tensor([0.1, -0.05, 1.0], dtype=torch.float64) * depth if dof == 6 else torch.tensor([2.0, 1.0, depth], dtype=torch.float64)
    tg = centre + 0.05 * depth * torch.randn(B, 3, generator=g, dtype=torch.float64)
    ang = torch.tensor([[angles[(r + b) % len(angles)] for b in range(B)] for r in range(R)], dtype=torch.float64)
    shift = torch.tensor([[(1e-3, 1e-2, 3e-2)[(r + 2 * b) % 3] for b in range(B)] for r in range(R)], dtype=torch.float64)
    te = tg + shift[..., None] * torch.nn.functional.normalize(torch.randn(R, B, 3, generator=g, dtype=torch.float64), dim=-1)
    if dof == 6:
        qg = torch.nn.functional.normalize(torch.randn(B, 4, generator=g, dtype=torch.float64), dim=-1)
        axis = torch.nn.functional.normalize(torch.randn(R, B, 3, generator=g, dtype=torch.float64), dim=-1)
        dq = torch.cat((torch.cos(ang / 2)[..., None], torch.sin(ang / 2)[..., None] * axis), -1)
        qe = _qmul(qg.expand(R, B, 4), dq) * (1.0 + 0.01 * torch.rand(R, B, 1, generator=g, dtype=torch.float64))
        qe[:, 1::2] = -qe[:, 1::2]
        return torch.cat((te, qe), -1).float().contiguous(), torch.cat((tg, qg), -1).float().contiguous()
    yg = torch.rand(B, 1, generator=g, dtype=torch.float64) * 6.0 - 3.0
    sign = torch.where(torch.rand(R, B, generator=g) < 0.5, -1.0, 1.0).double()
    ye = yg + (ang * sign)[..., None]
    return torch.cat((te, ye), -1).float().contiguous(), torch.cat((tg, yg), -1).float().contiguous()


def rot64(pose):
    """(..., P) fp64 -> (..., 3, 3): normalised quaternion [w, i, j, k] / yaw about y"""
    if pose.shape[-1] == 7:
        w, x, y, z = torch.nn.functional.normalize(pose[..., 3:], dim=-1).unbind(-1)
        rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    else:
        c, s, o, l = pose[..., 3].cos(), pose[..., 3].sin(), torch.zeros_like(pose[..., 3]), torch.ones_like(pose[..., 3])
        rows = (c, o, s, o, l, o, -s, o, c)
    return torch.stack(rows, -1).reshape(pose.shape[:-1] + (3, 3))


def angle_deg64(Re, Rg):
    """the angle |logm(Re^T Rg)|_F / sqrt 2 measures, in degrees: atan2 of the skew part's norm and (trace - 1) / 2"""
    D = Re.transpose(-1, -2) @ Rg
    v = torch.stack((D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]), -1).norm(dim=-1) / 2
    return torch.rad2deg(torch.atan2(v, (D.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2))


def fp64_errors(est, gt, models, model_id=None, K=None, sym=None, half=None):
    """(R,B,6) fp64: rot_deg, trans, arp_2d, add, adi, add_or_adi by the reference's expressions; models: list of (M,3) fp32"""
    est, gt = est.double(), gt.double()
    if est.dim() == 2:
        est = est[None]
    R, B = est.shape[:2]
    out = torch.full((R, B, 6), float('nan'), dtype=torch.float64)
    Re_all, Rg_all = rot64(est), rot64(gt)
    # the half turn: about the model's z axis (the reference's eggbox rule); a 4-DoF pose turns about its yaw axis, y
    flip = torch.diag(torch.tensor([-1.0, -1.0, 1.0] if est.shape[-1] == 7 else [-1.0, 1.0, -1.0], dtype=torch.float64))
    for b in range(B):
        pts = models[0 if model_id is None else int(model_id[b])].double()
        Rg, tg = Rg_all[b], gt[b, :3]
        pg = pts @ Rg.T + tg
        for r in range(R):
            Re, te = Re_all[r, b], est[r, b, :3]
            deg, Ra = angle_deg64(Re, Rg), Re
            if half is not None and bool(half[b]) and deg > 90:
                Ra = Re @ flip
                deg = angle_deg64(Ra, Rg)
            pe = pts @ Re.T + te
            out[r, b, 0], out[r, b, 1] = deg, (tg - te).norm()
            if K is not None:
                Kb = (K if K.dim() == 2 else K[b]).double()
                ue, ug = (pts @ Ra.T + te) @ Kb.T, pg @ Kb.T
                out[r, b, 2] = (ue[:, :2] / ue[:, 2:] - ug[:, :2] / ug[:, 2:]).norm(dim=-1).mean()
            out[r, b, 3] = (pe - pg).norm(dim=-1).mean()
            if sym is not None and bool(sym[b]):
                out[r, b, 4] = torch.cdist(pg, pe).min(dim=1).values.mean()
                out[r, b, 5] = out[r, b, 4]
            else:
                out[r, b, 5] = out[r, b, 3]
    return out


def check(raw, want, radius, est, gt, tag, extra_adi=0.0):
    """raw (R,B,8) against fp64_errors (R,B,6); radius (B,) model radius per object; prints every figure before it asserts.
    extra_adi: an absolute term of the ADD / ADD-S bar, a float or (B,), that the caller states (test_metrics_reference.py)"""
    got = raw.double().cpu().reshape(want.shape[:2] + (8,))
    nan_w = want.isnan()
    assert torch.equal(got[..., :6].isnan(), nan_w), f'{tag}: NaNs not exactly where specified'
    assert bool((got[..., 6:] == 0).all()), f'{tag}: words 6-7 must be 0'
    d = torch.where(nan_w, torch.zeros_like(want), (got[..., :6] - want).abs())
    w = torch.where(nan_w, torch.zeros_like(want), want)
    rad = radius.double().reshape(1, -1)
    extra = torch.as_tensor(extra_adi, dtype=torch.float64).reshape(1, -1, 1)
    e_add = ((d[..., 3:6] - extra).clamp(min=0) / (w[..., 3:6] + 1e-3 * rad[..., None])).max().item()
    e_arp = d[..., 2].max().item()
    e_rot = (d[..., 0] / (ROT_ABS + ROT_REL * w[..., 0])).max().item()
    tmax = torch.maximum(est.reshape(want.shape[:2] + (-1,))[..., :3].abs().amax(-1), gt[:, :3].abs().amax(-1)[None]).float()
    ulp = (torch.nextafter(tmax, torch.tensor(float('inf'))) - tmax).double()
    e_tr = (d[..., 1] / (TRANS_REL * w[..., 1] + ulp)).max().item()
    print(f'{tag}: add/adi scaled err {e_add:.3e} (bar {ADD_BAR:.1e}), arp_2d err {e_arp:.3e} px (bar {ARP_BAR:.1e}), '
          f'rot_deg err / (1e-4 deg + 1e-6 rel) {e_rot:.3e} (bar {ROT_BAR:.1e}), trans err / (1e-6 rel + 1 ulp) {e_tr:.3e} '
          f'(bar {TRANS_BAR:.1e})')
    assert e_add <= ADD_BAR and e_arp <= ARP_BAR and e_rot <= ROT_BAR and e_tr <= TRANS_BAR, tag


def _case(M, R, B, dof):
    """one model of M points, masks on some objects: symmetric b % 2 == 0, half_turn b % 3 == 0"""
    key = (M, R, B, dof)
    if key not in _cases:
        scale = 1.0 if dof == 6 else 20.0
        pts = ellipsoid(M, scale)
        est, gt = make_poses(R, B, dof, seed=1000 * dof + 7 * M + R + B)
        K = torch.tensor(K6 if dof == 6 else K4)
        sym = torch.tensor([b % 2 == 0 for b in range(B)])
        half = torch.tensor([b % 3 == 0 for b in range(B)])
        want = fp64_errors(est, gt, [pts], None, K, sym, half)
        _cases[key] = (pts, est, gt, K, sym, half, want, pts.norm(dim=-1).max().expand(B))
    return _cases[key]


def _run_case(backend, M, R, B, dof):
    metrics = _metrics()
    pts, est, gt, K, sym, half, want, radius = _case(M, R, B, dof)
    dev = [t.to(backend) for t in (est, gt, pts, K, sym, half)]
    e = metrics.pose_errors(dev[0], dev[1], dev[2], cam_mats=dev[3], symmetric=dev[4], half_turn=dev[5])
    return e, dev, (est, gt, want, radius)


def _sizes():
    m = _metrics()
    return [1, 63, 65, m.QUERY_TILE - 1, m.QUERY_TILE + 1, _big()]


def test_constants_are_the_headers():
    metrics = _metrics()
    text = open(os.path.join(ROOT, 'include', 'epropnp_hip.h')).read()
    for name, value in (('WORDS', metrics.WORDS), ('QUERY_TILE', metrics.QUERY_TILE), ('CAND_TILE', metrics.CAND_TILE)):
        assert int(re.search(rf'#define EPROPNP_POSE_ERROR_{name} (\d+)', text).group(1)) == value


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('which', range(6))
def test_model_sizes_against_fp64(backend, poisoned_empty, which, dof):
    """every model size at 3 x 5 rows, under poisoned_empty: accuracy, NaN exactly where specified (adi of the non-symmetric
    objects), words 6-7 zero, two launches bit-equal, (S,B,P) equal to S separate (B,P) calls bit for bit"""
    metrics = _metrics()
    M = _sizes()[which]
    e, dev, (est, gt, want, radius) = _run_case(backend, M, 3, 5, dof)
    assert e.raw.shape == (3, 5, 8) and e.add.shape == (3, 5)
    check(e.raw, want, radius, est, gt, f'M={M} dof={dof}')
    again = metrics.pose_errors(dev[0], dev[1], dev[2], cam_mats=dev[3], symmetric=dev[4], half_turn=dev[5])
    assert torch.equal(_bits(e.raw), _bits(again.raw)), 'two launches differ'
    for s in range(3):
        one = metrics.pose_errors(dev[0][s], dev[1], dev[2], cam_mats=dev[3], symmetric=dev[4], half_turn=dev[5])
        assert one.raw.shape == (5, 8)
        assert torch.equal(_bits(one.raw), _bits(e.raw[s])), f'row block {s} differs from its own (B,P) call'


@pytest.mark.parametrize('dof', [4, 6])
@pytest.mark.parametrize('R,B', [(1, 1), (3, 5), (1, 70)])
def test_row_shapes_against_fp64(backend, poisoned_empty, R, B, dof):
    e, dev, (est, gt, want, radius) = _run_case(backend, 65, R, B, dof)
    check(e.raw, want, radius, est, gt, f'M=65 R={R} B={B} dof={dof}')


def _mixed(dof):
    key = ('mixed', dof)
    if key not in _cases:
        metrics = _metrics()
        scale = 1.0 if dof == 6 else 20.0
        models = [ellipsoid(65, scale, 1), ellipsoid(metrics.QUERY_TILE + 1, scale, 2), ellipsoid(1, scale, 3)]
        B = 7
        est, gt = make_poses(2, B, dof, seed=4242 + dof)
        mid = torch.tensor([0, 1, 2, 1, 0, 2, 1], dtype=torch.int32)
        K = torch.tensor(K6 if dof == 6 else K4).expand(B, 3, 3) + torch.arange(B).float()[:, None, None] * torch.tensor(
            [[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 0.0]])
        sym = torch.tensor([True, True, True, False, False, False, True])
        half = torch.tensor([False, True, True, True, False, False, True])
        want = fp64_errors(est, gt, models, mid, K, sym, half)
        radius = torch.stack([models[int(i)].norm(dim=-1).max() for i in mid])
        _cases[key] = (models, est, gt, mid, K.contiguous(), sym, half, want, radius)
    return _cases[key]


@pytest.mark.parametrize('dof', [4, 6])
def test_three_models_in_one_call(backend, poisoned_empty, dof):
    """three models of different size in one call, per-object intrinsics, `symmetric` and `half_turn` on some objects only"""
    metrics = _metrics()
    models, est, gt, mid, K, sym, half, want, radius = _mixed(dof)
    pts, rng = metrics.pack_models([m.to(backend) for m in models])
    assert rng.dtype == torch.int32 and rng.cpu().tolist() == [[0, 65], [65, metrics.QUERY_TILE + 1], [66 + metrics.QUERY_TILE, 1]]
    e = metrics.pose_errors(est.to(backend), gt.to(backend), pts, rng, model_id=mid.to(backend), cam_mats=K.to(backend),
                            symmetric=sym.to(backend), half_turn=half.to(backend))
    check(e.raw, want, radius, est, gt, f'three models dof={dof}')
    assert torch.equal(_bits(e.add_or_adi), _bits(torch.where(sym.to(backend), e.adi, e.add)))


def test_half_turn_rows_bite(backend):
    """the case holds rows beyond 90 degrees on half_turn objects (the 3 rad offsets): there rot_deg differs from the raw angle, and
    add / adi keep the bits of a call without the mask"""
    metrics = _metrics()
    e, dev, (est, gt, want, radius) = _run_case(backend, 65, 3, 5, 6)
    raw = metrics.pose_errors(dev[0], dev[1], dev[2], cam_mats=dev[3], symmetric=dev[4])
    turned = (raw.rot_deg > 90) & dev[5]
    assert int(turned.sum()) >= 1
    assert bool((e.rot_deg[turned] < raw.rot_deg[turned] - 1.0).all()) and bool((e.arp_2d[turned] != raw.arp_2d[turned]).all())
    assert torch.equal(_bits(e.rot_deg[~turned]), _bits(raw.rot_deg[~turned]))
    assert torch.equal(_bits(e.raw[..., 3:6]), _bits(raw.raw[..., 3:6])), 'half_turn must leave add / adi alone'


def test_depth_50_add_keeps_its_digits(backend, poisoned_empty):
    """translations about (2, 1, 50), a rotation offset of 1e-3 rad, a translation offset of 1e-3: add (and adi) meet the bar of
    every other case, while the naive fp32 form -- transform the points by both poses, subtract -- misses it on this very input"""
    metrics = _metrics()
    key = 'depth50'
    if key not in _cases:
        pts = ellipsoid(257)
        g = torch.Generator().manual_seed(50)
        B = 6
        tg = torch.tensor([2.0, 1.0, 50.0], dtype=torch.float64) + 0.3 * torch.randn(B, 3, generator=g, dtype=torch.float64)
        qg = torch.nn.functional.normalize(torch.randn(B, 4, generator=g, dtype=torch.float64), dim=-1)
        axis = torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=torch.float64), dim=-1)
        dq = torch.cat((torch.full((B, 1), math.cos(5e-4), dtype=torch.float64), math.sin(5e-4) * axis), -1)
        te = tg + 1e-3 * torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=torch.float64), dim=-1)
        est, gt = torch.cat((te, _qmul(qg, dq)), -1).float(), torch.cat((tg, qg), -1).float()
        sym = torch.ones(B, dtype=torch.bool)
        K = torch.tensor(K6)
        _cases[key] = (pts, est, gt, K, sym, fp64_errors(est, gt, [pts], None, K, sym, None))
    pts, est, gt, K, sym, want = _cases[key]
    e = metrics.pose_errors(est.to(backend), gt.to(backend), pts.to(backend), cam_mats=K.to(backend), symmetric=sym.to(backend))
    radius = pts.norm(dim=-1).max().expand(est.shape[0])
    check(e.raw, want, radius, est, gt, 'depth 50')
    # the naive form in fp32, on the same inputs
    Re, Rg = rot64(est.double()).float(), rot64(gt.double()).float()
    naive = ((pts @ Re.transpose(-1, -2) + est[:, None, :3]) - (pts @ Rg.transpose(-1, -2) + gt[:, None, :3])).norm(dim=-1).mean(-1)
    err = ((naive.double() - want[0, :, 3]).abs() / (want[0, :, 3] + 1e-3 * radius.double())).max().item()
    print(f'depth 50: the naive fp32 add is off by {err:.3e} on the scale of the bar {ADD_BAR:.1e}')
    assert err > ADD_BAR, 'the depth-50 case does not bite'


def test_identical_poses_give_exact_zeros(backend, poisoned_empty):
    metrics = _metrics()
    for dof in (4, 6):
        _, gt = make_poses(1, 5, dof, seed=99 + dof)
        gt = gt.to(backend)
        pts = ellipsoid(65, 1.0 if dof == 6 else 20.0).to(backend)
        sym = torch.ones(5, dtype=torch.bool, device=backend)
        e = metrics.pose_errors(gt.clone(), gt, pts, cam_mats=torch.tensor(K6, device=backend), symmetric=sym, half_turn=sym)
        assert bool((e.raw == 0).all()), e.raw


@pytest.mark.parametrize('parts', [1, 4])
def test_nn_parts_does_not_change_a_bit(backend, monkeypatch, parts):
    """EPROPNP_TUNE="nn_parts=<n>": the query tiles of a row dealt to n workgroups; the tile sums are added in tile order"""
    metrics = _metrics()
    M = _big()
    set_tune(monkeypatch)
    base, dev, _ = _run_case(backend, M, 3, 5, 6)
    set_tune(monkeypatch, nn_parts=parts)
    got = metrics.pose_errors(dev[0], dev[1], dev[2], cam_mats=dev[3], symmetric=dev[4], half_turn=dev[5])
    assert torch.equal(_bits(got.raw), _bits(base.raw))


def test_bad_rows_poison_themselves_only(backend, poisoned_empty):
    """a NaN pose (estimate or ground truth), a model_id of -1 or C, and a model without points: NaN in words 0..5 of their own rows,
    every other row bit-equal to the clean call"""
    metrics = _metrics()
    models = [ellipsoid(65, 1.0, 1), torch.zeros(0, 3), ellipsoid(63, 1.0, 2)]
    pts, rng = metrics.pack_models([m.to(backend) for m in models])
    assert rng.cpu().tolist() == [[0, 65], [65, 0], [65, 63]]
    R, B = 2, 8
    est, gt = make_poses(R, B, 6, seed=31)
    mid = torch.tensor([0, 2, 0, 2, 0, 2, 0, 2], dtype=torch.int32)
    sym = torch.tensor([b % 2 == 0 for b in range(B)])
    K = torch.tensor(K6)
    args = dict(cam_mats=K.to(backend), symmetric=sym.to(backend))
    clean = metrics.pose_errors(est.to(backend), gt.to(backend), pts, rng, model_id=mid.to(backend), **args)
    assert bool(clean.raw[..., [0, 1, 2, 3, 5]].isfinite().all())
    est2, gt2, mid2 = est.clone(), gt.clone(), mid.clone()
    est2[1, 0, 4] = float('nan')       # row (1, 0)
    est2[0, 3, 1] = float('inf')       # row (0, 3)
    gt2[5, 3] = float('nan')           # rows (:, 5)
    mid2[1], mid2[2], mid2[6] = -1, 3, 1      # rows (:, 1), (:, 2), (:, 6): below, beyond, the empty model
    got = metrics.pose_errors(est2.to(backend), gt2.to(backend), pts, rng, model_id=mid2.to(backend), **args)
    bad = torch.zeros(R, B, dtype=torch.bool)
    bad[1, 0] = bad[0, 3] = True
    bad[:, [5, 1, 2, 6]] = True
    raw, ref = got.raw.cpu(), clean.raw.cpu()
    assert bool(raw[bad][:, :6].isnan().all()) and bool((raw[bad][:, 6:] == 0).all())
    assert torch.equal(_bits(raw[~bad]), _bits(ref[~bad]))


def test_nan_exactly_where_specified_without_camera_and_masks(backend, poisoned_empty):
    metrics = _metrics()
    pts, est, gt, K, sym, half, want, radius = _case(65, 3, 5, 6)
    e = metrics.pose_errors(est.to(backend), gt.to(backend), pts.to(backend))
    assert bool(e.arp_2d.isnan().all()) and bool(e.adi.isnan().all())
    assert bool(e.raw[..., [0, 1, 3, 5]].isfinite().all()) and bool((e.raw[..., 6:] == 0).all())
    assert torch.equal(_bits(e.add), _bits(e.add_or_adi))
    full = metrics.pose_errors(est.to(backend), gt.to(backend), pts.to(backend), cam_mats=K.to(backend), symmetric=sym.to(backend))
    assert torch.equal(_bits(e.add), _bits(full.add)) and torch.equal(_bits(e.rot_deg), _bits(full.rot_deg))


def test_python_errors(backend):
    metrics = _metrics()
    pts, est, gt, K, sym, half, want, radius = _case(65, 3, 5, 6)
    est, gt, pts, K, sym = (t.to(backend) for t in (est, gt, pts, K, sym))
    with pytest.raises(TypeError):
        metrics.pose_errors(est.double(), gt, pts)
    with pytest.raises(TypeError):
        metrics.pose_errors(est, gt, pts.double())
    for bad in (lambda: metrics.pose_errors(est[:, :4], gt, pts), lambda: metrics.pose_errors(est[..., :5], gt[..., :5], pts),
                lambda: metrics.pose_errors(est, gt, pts[:, :2]), lambda: metrics.pose_errors(est, gt, pts, cam_mats=K[:2]),
                lambda: metrics.pose_errors(est, gt, pts, symmetric=sym[:3]), lambda: metrics.pose_errors(est, gt, pts, symmetric=sym.float()),
                lambda: metrics.pose_errors(est, gt, pts, model_id=torch.zeros(5, dtype=torch.int32, device=backend)),
                lambda: metrics.pose_errors(est, gt, pts, torch.zeros(2, 2, dtype=torch.int64, device=backend)),
                lambda: metrics.pose_errors(est[:0], gt, pts), lambda: metrics.pack_models([]), lambda: metrics.pack_models([pts[:, :2]])):
        with pytest.raises(ValueError):
            bad()
    empty = metrics.pose_errors(est[:, :0], gt[:0], pts, cam_mats=K, symmetric=sym[:0])
    assert empty.raw.shape == (3, 0, 8) and empty.add_or_adi.shape == (3, 0)


def test_cpu_tensors_are_refused():
    """the product binding, no emulation installed: a CPU tensor is an error, not a fallback"""
    import install as emu
    emu.uninstall()
    metrics = _metrics()
    pts, est, gt = ellipsoid(65), *make_poses(1, 2, 6, seed=5)
    with pytest.raises(RuntimeError, match='HIP device'):
        metrics.pose_errors(est, gt, pts)


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_inputs():
    """captured with torch.cuda.graph after a side-stream warm-up, replayed twice on changed inputs: the bits of the eager call"""
    import install as emu
    emu.uninstall()
    metrics = _metrics()
    dev = torch.device('cuda:0')
    models, est, gt, mid, K, sym, half, want, radius = _mixed(6)
    pts, rng = metrics.pack_models([m.to(dev) for m in models])
    s_est, s_gt = est.to(dev), gt.to(dev)
    fixed = dict(model_id=mid.to(dev), cam_mats=K.to(dev), symmetric=sym.to(dev), half_turn=half.to(dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.pose_errors(s_est, s_gt, pts, rng, **fixed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.pose_errors(s_est, s_gt, pts, rng, **fixed)
    for seed in (1, 2):
        e2, g2 = make_poses(2, 7, 6, seed=900 + seed)
        s_est.copy_(e2.to(dev))
        s_gt.copy_(g2.to(dev))
        graph.replay()
        eager = metrics.pose_errors(e2.to(dev), g2.to(dev), pts, rng, **fixed)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.raw), _bits(eager.raw)), f'replay {seed} differs from the eager call'
