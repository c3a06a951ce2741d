"""AMIS backward: a second body of the sweep without the camera's depth clamp, taken per object where every pose of the table keeps
every point in front of z_min (amis_backward_mfma.hip: ZFREE; pnp_math.h: depth_clamp_clear).

Where the bound holds, max(h_z, z_min) returns h_z and the 0/1 front factor is exactly 1, so the bar is equality of bits, not a
tolerance: every case compares EPROPNP_TUNE=zfree=1 (the two-body instantiation wherever it exists, whatever the grid) with zfree=0
(never) through int32 views, NaNs included.

Shapes: B = 3, S = 40 (P = 41 with pose_init: a padded third pose tile), N = 40 (4 waves x 1 tile, a padded point tile) and N = 300
under bwd_mfma=4,4 (two chunks of 256 points).  The launch-plan record does not say which body an object took (its five ints keep
their meaning); `_margin` restates the bound in fp64 with the kernel's slack, and every case asserts which objects are on which side
of it, so that a case cannot silently compare the clamped body with itself."""
import os
import subprocess

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise, set_tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, K = 3, 40, 2
SEED = 61
SHAPES = [(40, None), (300, '4,4')]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    for name, x, y in zip(('grad_x3d', 'grad_x2d', 'grad_w2d', 'grad_delta'), a, b):
        assert torch.equal(_bits(x), _bits(y)), (what, name)


def _margin(prob, poses, z_min):
    """depth_clamp_clear restated in fp64 with the same slack: (P, B) lower bound of h_z over the ball |x| <= Rmax, minus
    max(z_min, 2^-30).  An object is clear when the margin of every pose of its table is >= 0; a NaN margin is not clear."""
    Kz = prob['cam_mats'].double()[:, 2, :]                                   # (B, 3)
    poses = poses.double().cpu()
    R = orc.pose_to_rotmat(poses)                                             # (P, B, 3, 3)
    kz = torch.einsum('bi,pbij->pbj', Kz, R)
    ktz = torch.einsum('bi,pbi->pb', Kz, poses[..., :3])
    rmax = prob['x3d'].double().norm(dim=-1).amax(1) * (1 + 2.0 ** -12)
    reach = (kz.norm(dim=-1) + 2.0 ** -60) * rmax
    lb = ktz - reach * (1 + 2.0 ** -8) - 2.0 ** -16 * (ktz.abs() + reach)
    return lb - max(z_min, 2.0 ** -30)


def _clear(prob, poses, z_min):
    """per object: True / False, with no finite margin so close to 0 that fp32 and fp64 could decide differently"""
    m = _margin(prob, poses, z_min)
    assert not bool((m.abs() < 1e-3).any()), 'a margin within 1e-3 of the bound: the restatement cannot vouch for the fp32 decision'
    return [bool(v) for v in (m >= 0).all(0)]      # (NaN >= 0 is False)


def _make(dev, dof, bounds, N, z_min=0.1, depths=None, seed=SEED):
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    prob = orc.make_problem(B, N, dof, seed=seed, bounds=bounds)
    if depths is not None:      # the objects at chosen depths: x2d re-projected (with the pixel noise make_problem drew), delta recomputed
        cam = orc.Cam(prob['cam_mats'].double(), 0.1)
        noise = prob['x2d'].double() - orc.evaluate_project(prob['x3d'].double(), prob['pose_gt'].double(), cam)
        for k in ('pose_gt', 'pose_init'):
            prob[k] = prob[k].clone()
            prob[k][:, 2] = torch.tensor(depths, dtype=prob[k].dtype)
        prob['x2d'] = (orc.evaluate_project(prob['x3d'].double(), prob['pose_gt'].double(), cam) + noise).float()
        prob['delta'] = orc.adaptive_huber_delta(prob['x2d'], prob['w2d'], 0.5)
    prob['z_min'] = z_min
    p, cam, _ = make_layer_objects(prob, dev)
    return prob, p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)


def _forward(dev, hp, p, dof):
    from epropnp import functional as F
    cov = (torch.eye(dof) * torch.tensor([0.02, 0.02, 0.3] + [1e-3] * (dof - 3))).expand(B, dof, dof).contiguous()
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=62), dof).to(dev)
    samples, _, costs = F.amis_forward(hp, p['pose_gt'], cov.to(dev), S, K, noise=noise, with_costs=True)
    return samples, costs, F.evaluate_cost(hp, p['pose_init'])


def _weights(dev, spread):
    """gradients of the log-weights.  spread: object 1 drops most of its samples and object 2 keeps exactly one (the compaction's
    paths, as in test_presplit_pose_rows); otherwise every object keeps every sample, so that the table holds all of them"""
    g = torch.Generator().manual_seed(63)
    lw = torch.rand(S, B, generator=g)
    if spread:
        lw[:, 1] = torch.linspace(0.0, -40.0, S)[torch.randperm(S, generator=g)]
        lw[:, 2] = -40.0
        lw[17, 2] = 0.0
    g_logw = torch.exp(lw) * torch.where(torch.rand(S, B, generator=g) < 0.5, -1.0, 1.0)
    g_init = torch.tensor([0.7, -0.3, 0.0 if spread else 0.4])
    return g_logw.to(dev), g_init.to(dev)


def _entries(hp, samples, g_logw, pin, gin, costs, cin):
    from epropnp import functional as F
    return [F.amis_backward(hp, samples, g_logw, pin, gin),                                      # per-pair entry
            F.amis_backward(hp, samples, g_logw, pin, gin, sample_costs=costs, cost_init=cin)]   # DCOST entry


def _both(monkeypatch, tune, *args):
    runs = {}
    for knob in (1, 0):
        set_tune(monkeypatch, bwd_mfma=tune, zfree=knob)
        runs[knob] = _entries(*args)
    set_tune(monkeypatch, bwd_mfma=tune)
    return runs


def _table(samples, pose_init):
    return torch.cat((samples.cpu(), pose_init.cpu()[None]), 0)


def test_the_bound_alone(tmp_path):
    """depth_clamp_clear on fixed cases and, over seeded random (pose, point cloud) draws, against the fp32 h_z of every point"""
    src = tmp_path / 'depth_bound.cpp'
    src.write_text(r'''
#include "pnp_math.h"
#include <cstdio>
#include <cmath>
#include <cstdint>
#include <limits>
using namespace pnp;
static int bad = 0;
static void expect(bool got, bool want, const char* what) {
  if (got != want) { std::printf("FAIL %s: got %d want %d\n", what, (int)got, (int)want); ++bad; }
}
static uint64_t lcg = 0x9e3779b97f4a7c15ull;
static double uni() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) / 9007199254740992.0;
}
static double gauss() { return std::sqrt(-2.0 * std::log(1.0 - uni())) * std::cos(6.283185307179586 * uni()); }
int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 5.f, 2.f, 0.1f), true, "depth 5, Rmax 2, z_min 0.1");
  // t_z - Rmax within the slack of z_min, on either side: slack = 2^-8 * 2 + 2^-16 * (t_z + 2) ~ 0.0079
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 2.1f + 0.004f, 2.f, 0.1f), false, "inside the slack, above");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 2.1f + 1e-6f, 2.f, 0.1f), false, "just above");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 2.1f - 0.004f, 2.f, 0.1f), false, "inside the slack, below");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 2.1f + 0.012f, 2.f, 0.1f), true, "beyond the slack");
  expect(depth_clamp_clear(nan, 0.f, 1.f, 5.f, 2.f, 0.1f), false, "NaN row");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, nan, 2.f, 0.1f), false, "NaN depth");
  expect(depth_clamp_clear(0.f, inf, 1.f, 5.f, 2.f, 0.1f), false, "inf row");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, inf, 2.f, 0.1f), false, "inf depth (inf - inf in the slack)");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, inf, inf, 0.1f), false, "inf depth, inf Rmax");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, -inf, 2.f, 0.1f), false, "-inf depth");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 5.f, nan, 0.1f), false, "NaN Rmax");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 5.f, inf, 0.1f), false, "inf Rmax");
  expect(depth_clamp_clear(0.f, 0.f, 0.f, 5.f, inf, 0.1f), false, "zero row, inf Rmax");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 5.f, 2.f, nan), false, "NaN z_min");
  expect(depth_clamp_clear(0.f, 0.f, 0.f, 0.f, 0.f, 0.f), false, "h_z = 0 (or -0) at z_min = 0");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 5.f, 2.f, -1.f), true, "negative z_min");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 1e-12f, 0.f, 0.f), false, "below the floor of 2^-30");
  expect(depth_clamp_clear(0.f, 0.f, 1.f, 0x1p40f, 2.f, 0x1p31f), false, "z_min beyond 2^30");
  expect(depth_r2(nan, 0.f, 0.f) == inf && depth_r2(0.f, 0.f, 3e30f) == inf && depth_r2(1.f, 2.f, 2.f) == 9.f, true, "depth_r2");
  expect(depth_rmax_up(9.f) > 3.f && depth_rmax_up(9.f) < 3.001f, true, "depth_rmax_up");
  for (float z_min : {0.01f, 0.1f, 3.f}) {      // the padding pose of the tables: a zero row at depth max(1, 2 z_min)
    expect(depth_clamp_clear(0.f, 0.f, 0.f, std::fmax(1.f, 2.f * z_min), 2.f, z_min), true, "padding pose");
    expect(depth_clamp_clear(0.f, 0.f, 0.f, std::fmax(1.f, 2.f * z_min), 1e6f, z_min), true, "padding pose, large object");
  }
  // random draws: a rotation-like row times a scale, a depth that puts the object near the clamp, a cloud of 24 points
  long draws = 0, clear = 0, behind = 0;
  for (int it = 0; it < 6000; ++it) {
    const float z_min = (it % 3 == 0) ? 0.01f : (it % 3 == 1) ? 0.1f : 3.f;
    double k[3] = {gauss(), gauss(), gauss()};
    const double kn = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]), sc = std::exp(2.0 * gauss());
    float kz[3];
    for (int i = 0; i < 3; ++i) kz[i] = (float)(k[i] / kn * sc);
    float X[24][3], r2 = 0.f;
    const double size = std::exp(gauss());
    for (auto& x : X) {
      for (int i = 0; i < 3; ++i) x[i] = (float)(size * gauss());
      r2 = std::fmax(r2, depth_r2(x[0], x[1], x[2]));
    }
    const float Rmax = depth_rmax_up(r2);
    // depth = z_min + reach * U(0.8, 1.3): on both sides of the bound
    const float ktz = (float)(z_min + sc * (double)Rmax * (0.8 + 0.5 * uni()));
    const bool c = depth_clamp_clear(kz[0], kz[1], kz[2], ktz, Rmax, z_min);
    float lo = inf;
    for (auto& x : X) lo = std::fmin(lo, std::fmaf(kz[0], x[0], std::fmaf(kz[1], x[1], std::fmaf(kz[2], x[2], ktz))));
    ++draws; clear += c; behind += (lo < z_min);
    if (c && !(lo >= z_min)) { std::printf("FAIL draw %d: clear, but h_z = %g < z_min = %g\n", it, lo, z_min); ++bad; }
  }
  std::printf("draws %ld, clear %ld, with a point behind z_min %ld, failures %d\n", draws, clear, behind, bad);
  return (bad != 0 || clear < draws / 10 || clear > draws - draws / 10) ? 1 : 0;
}
''')
    exe = tmp_path / 'depth_bound'
    emu = os.path.join(ROOT, 'tests', 'emu')
    r = subprocess.run(['g++', '-O1', '-std=c++17', '-x', 'c++', '-include', os.path.join(emu, 'hip_emu.h'), '-I', os.path.join(emu, 'include'),
                        '-I', os.path.join(ROOT, 'epro-pnp_amd', 'csrc'), '-ffp-contract=off', '-Wno-unknown-pragmas', '-Wno-attributes',
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'failures 0' in out.stdout


@pytest.mark.parametrize('dof,bounds', [(6, None), (6, 'tight'), (4, None), (4, 'tight')])
@pytest.mark.parametrize('N,tune', SHAPES)
def test_case_a_every_object_clear(backend, monkeypatch, dof, bounds, N, tune):
    prob, p, hp = _make(backend, dof, bounds, N)
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, dof)
    assert _clear(prob, _table(samples, p['pose_init']), 0.1) == [True, True, True]
    g_logw, g_init = _weights(backend, spread=True)
    for with_init in (True, False):
        pin, gin, cin = (p['pose_init'], g_init, cost_init) if with_init else (None, None, None)
        runs = _both(monkeypatch, tune, hp, samples, g_logw, pin, gin, costs, cin)
        for i, entry in enumerate(('per-pair', 'costs')):
            assert all(bool(torch.isfinite(t).all()) for t in runs[1][i]), entry
            assert float(runs[1][i][0].abs().max()) > 0, entry
            _same_bits(runs[1][i], runs[0][i], (entry, with_init))


@pytest.mark.parametrize('dof,bounds', [(6, None), (6, 'tight'), (4, None), (4, 'tight')])
@pytest.mark.parametrize('N,tune', SHAPES)
def test_case_b_one_sample_puts_a_point_behind_z_min(backend, monkeypatch, dof, bounds, N, tune):
    """Object 1's heaviest sample is moved along z until its nearest point has h_z = 0.05 < z_min = 0.1 (still in front of the camera),
    and sideways until that point lies on the optical axis, so that it stays inside the projection bounds of the 'tight' cases.
    The object must take the clamped body: the bits of zfree=0.  That this matters is shown twice: the same launch with z_min = 1e-6,
    where no depth is clamped -- what a body without the clamp computes -- gives object 1 other gradients, and so does zeroing the moved
    sample's weight (it contributes).  Objects 0 and 2 stay clear and are the same under both values of z_min."""
    prob, p, hp = _make(backend, dof, bounds, N)
    _, _, hp_low = _make(backend, dof, bounds, N, z_min=1e-6)
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, dof)
    g_logw, g_init = _weights(backend, spread=False)
    j = int(g_logw[:, 1].abs().argmax())
    moved = samples.clone()
    R = orc.pose_to_rotmat(moved[j, 1].double().cpu())
    hz = prob['x3d'][1].double() @ R[2] + float(moved[j, 1, 2])
    moved[j, 1, 2] -= float(hz.min()) - 0.05
    hz = prob['x3d'][1].double() @ R[2] + float(moved[j, 1, 2])
    assert 0.04 < float(hz.min()) < 0.06 and 1 <= int((hz < 0.1).sum()) < N
    # ... and sideways until that point sits on the optical axis: it projects to the principal point without the clamp and halfway
    # to the image corner with it, both inside the 'tight' projection bounds (beyond them neither body passes a gradient)
    near = prob['x3d'][1, int(hz.argmin())].double()
    moved[j, 1, 0] -= float(near @ R[0]) + float(moved[j, 1, 0])
    moved[j, 1, 1] -= float(near @ R[1]) + float(moved[j, 1, 1])
    assert _clear(prob, _table(moved, p['pose_init']), 0.1) == [True, False, True]
    args = (moved, g_logw, p['pose_init'], g_init, costs, cost_init)
    runs = _both(monkeypatch, tune, hp, *args)
    set_tune(monkeypatch, bwd_mfma=tune, zfree=0)
    low = _entries(hp_low, *args)
    zeroed = g_logw.clone()
    zeroed[j, 1] = 0.0
    without = _entries(hp, moved, zeroed, p['pose_init'], g_init, costs, cost_init)
    for i in range(2):
        _same_bits(runs[1][i], runs[0][i], i)
        gx, gx_low, gx_without = runs[1][i][0], low[i][0], without[i][0]
        assert bool(torch.isfinite(gx).all())
        assert not torch.equal(_bits(gx[1]), _bits(gx_low[1])), 'the clamp changes nothing: the case does not tell the bodies apart'
        assert torch.equal(_bits(gx[0]), _bits(gx_low[0])) and torch.equal(_bits(gx[2]), _bits(gx_low[2]))
        assert not torch.equal(_bits(gx[1]), _bits(gx_without[1])), 'the moved sample does not contribute'


@pytest.mark.parametrize('N,tune', SHAPES)
def test_case_c_a_nan_pose_component(backend, monkeypatch, N, tune):
    """a kept sample with a NaN component: its object fails the bound, the NaNs that come out carry the clamped body's bits, the other
    objects are clear and stay finite"""
    prob, p, hp = _make(backend, 6, None, N)
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, 6)
    g_logw, g_init = _weights(backend, spread=False)
    bad = samples.clone()
    bad[3, 0, 1] = float('nan')
    assert _clear(prob, _table(bad, p['pose_init']), 0.1) == [False, True, True]
    runs = _both(monkeypatch, tune, hp, bad, g_logw, p['pose_init'], g_init, costs, cost_init)
    for i in range(2):
        _same_bits(runs[1][i], runs[0][i], i)
        assert not bool(torch.isfinite(runs[1][i][0][0]).all())
        assert bool(torch.isfinite(runs[1][i][0][1:]).all())


@pytest.mark.parametrize('dof,bounds', [(6, None), (4, 'tight')])
@pytest.mark.parametrize('N,tune', SHAPES)
def test_case_d_a_large_z_min_splits_the_batch(backend, monkeypatch, dof, bounds, N, tune):
    """z_min = 3 with the objects at depth 5, 8 and 11 and Rmax about 2: the near object has samples whose points the clamp holds,
    the far one is clear"""
    prob, p, hp = _make(backend, dof, bounds, N, z_min=3.0, depths=(5.0, 8.0, 11.0))
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, dof)
    clear = _clear(prob, _table(samples, p['pose_init']), 3.0)
    assert clear[0] is False and clear[2] is True, clear
    g_logw, g_init = _weights(backend, spread=False)
    runs = _both(monkeypatch, tune, hp, samples, g_logw, p['pose_init'], g_init, costs, cost_init)
    for i in range(2):
        assert all(bool(torch.isfinite(t).all()) for t in runs[1][i])
        _same_bits(runs[1][i], runs[0][i], i)


@pytest.mark.gpu
@pytest.mark.parametrize('fold', [False, True], ids=['plain', 'delta-fold'])
def test_big_batch_takes_the_two_body_kernel_by_the_plans_rule_and_keeps_its_bits(monkeypatch, fold):
    """B = 512, N = 512, S = 512, 6-DoF: two workgroups per CU on every CU, the grid at which the plan takes the two-body instantiation
    unasked.  Forward, then backward: default against zfree=0 against default again -- equal bits, the second default launch included."""
    import install as emu
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    emu.uninstall()
    dev = torch.device('cuda:0')
    Bb, Nb, Sb = 512, 512, 512
    prob = orc.make_problem(Bb, Nb, 6, seed=81)
    p, cam, _ = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), 6)
    if fold:
        _, stats = F.adaptive_delta(hp.x2d, hp.w2d, 0.5)
        hp = F.PnPProblem(hp.x3d, hp.x2d, hp.w2d, cam, HuberPnPCost(delta=hp.delta), 6).fold_delta(stats, 0.5)
    plan = F.launch_plan('backward', hp, Sb, pose_init=True)
    assert {k: plan[k] for k in ('waves', 'tiles', 'bf16', 'valu', 'parked', 'nsplit')} == dict(waves=4, tiles=4, bf16=True, valu=False, parked=fold, nsplit=1), plan
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)
    g = torch.Generator().manual_seed(82)
    g_obj, g_init = torch.randn(Bb, generator=g).to(dev), torch.randn(Bb, generator=g).to(dev)
    runs = {}
    for knob in (None, 0, None):
        set_tune(monkeypatch, zfree=knob)
        samples, logw, costs = F.amis_forward(hp, pose_opt, pose_cov, Sb, 4, seed=3, with_costs=True)
        cost_init = F.evaluate_cost(hp, p['pose_init'])
        g_logw = torch.softmax(logw, 0) * g_obj
        out = [(samples, logw, costs), F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init),
               F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=cost_init)]
        if knob in runs:      # the second default launch
            for i in range(3):
                for x, y in zip(runs[knob][i], out[i]):
                    assert torch.equal(_bits(x), _bits(y)), ('again', i)
        runs[knob] = out
    # Most objects of this batch are clear (depth 5 +- 1, Rmax about 2): the comparison is of the two bodies, not of one with itself.
    # The table holds pose_init and the samples that the drop threshold keeps; a sample whose weight is below 2^-24 / S of the
    # object's total is dropped for certain (all such samples together stay below the 2^-24 of the total that the tail may hold), so
    # the others are a superset of the table -- the heavy-tailed proposal's far-out samples are not in it.
    samples, logw, _ = runs[None][0]
    m = _margin(prob, torch.cat((samples.cpu(), p['pose_init'].cpu()[None]), 0), 0.1) >= 0
    maybe_kept = torch.softmax(logw.double().cpu(), 0) >= 2.0 ** -24 / Sb
    clear = (m[:-1] | ~maybe_kept).all(0) & m[-1]
    print('objects clear by the restated bound:', int(clear.sum()), 'of', Bb)
    assert int(clear.sum()) > Bb // 2, int(clear.sum())
    for i in range(3):
        assert all(bool(torch.isfinite(t).all()) for t in runs[None][i])
        for x, y in zip(runs[None][i], runs[0][i]):
            assert torch.equal(_bits(x), _bits(y)), i
