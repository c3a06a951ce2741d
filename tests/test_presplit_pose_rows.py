"""AMIS backward: the projection's pose rows split to bf16 once, by the pose-table build, instead of per wave, pose tile and chunk
(amis_backward_mfma.hip: PRESPLIT; wave_ops.h: bf16_split_a_words / bf16_a_from_words).

The stored words are the dwords that bf16_split_a forms on the fly, so the bar is equality of bits, not a tolerance: every case
compares the default launch with EPROPNP_TUNE=bwd_presplit=0 through int32 views (NaNs included).

Shapes: B = 3, S = 40 (P = 41 with pose_init: a padded third pose tile), N = 40 (4 waves x 1 tile, a padded point tile) and N = 300
under bwd_mfma=4,4 (two chunks of 256 points).  The launch-plan record does not say whether the table is pre-split (its five ints keep
their meaning); _presplit_fits restates the launcher's LDS rule so that a case cannot silently compare the on-the-fly path with itself."""
import os
import subprocess

import pytest
import torch

import epropnp_oracle as orc
from helpers import make_layer_objects, pack_noise, set_tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, K = 3, 40, 2
DROP_HIST_FLOATS = 2 * 66      # amis_common.h: kDropHistFloats


def _presplit_fits(S_, with_init, tiles, N, parked):
    """plan_amis_backward's rule: 15 (+ 18 pre-split) dwords per table row, two workgroups per CU for four tiles, three otherwise"""
    P16 = ((S_ + int(with_init) + 15) // 16) * 16 + 16
    smem = 4 * (15 * P16 + 80 + DROP_HIST_FLOATS) + (8 * N if parked else 0)
    return smem <= 160 * 1024, (2 if tiles == 4 else 3) * (smem + 4 * 18 * P16) <= 160 * 1024


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    for name, x, y in zip(('grad_x3d', 'grad_x2d', 'grad_w2d', 'grad_delta'), a, b):
        assert torch.equal(_bits(x), _bits(y)), (what, name)


def _problem(dev, dof, bounds, N, seed=61):
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    prob = orc.make_problem(B, N, dof, seed=seed, bounds=bounds)
    p, cam, _ = make_layer_objects(prob, dev)
    return p, F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)


def _forward(dev, hp, p, dof):
    from epropnp import functional as F
    cov = (torch.eye(dof) * torch.tensor([0.02, 0.02, 0.3] + [1e-3] * (dof - 3))).expand(B, dof, dof).contiguous()
    noise = pack_noise(orc.make_noise(B, S, K, dof, seed=62), dof).to(dev)
    samples, _, costs = F.amis_forward(hp, p['pose_gt'], cov.to(dev), S, K, noise=noise, with_costs=True)
    return samples, costs, F.evaluate_cost(hp, p['pose_init'])


def _weights(dev):
    """gradients of the log-weights whose magnitudes spread by 40 units of the logarithm: object 0 keeps every sample, object 1 drops
    most of them (default threshold 2^-24 = e^-16.6 of the object's total), object 2 keeps exactly one (its pose_init weight is 0)"""
    g = torch.Generator().manual_seed(63)
    lw = torch.empty(S, B)
    lw[:, 0] = torch.rand(S, generator=g)
    lw[:, 1] = torch.linspace(0.0, -40.0, S)[torch.randperm(S, generator=g)]
    lw[:, 2] = -40.0
    lw[17, 2] = 0.0
    g_logw = torch.exp(lw) * torch.where(torch.rand(S, B, generator=g) < 0.5, -1.0, 1.0)
    g_init = torch.tensor([0.7, -0.3, 0.0])
    return g_logw.to(dev), g_init.to(dev)


def test_store_and_rebuild_give_the_dwords_of_the_on_the_fly_split(tmp_path):
    """bf16_split_a(x) == bf16_a_from_words(bf16_split_a_words(x)), also through the 16-bit form of the third piece, for every exponent
    with random mantissas and mantissas whose low 16 / low 8 bits are zero, +-0, denormals, +-inf and NaNs of several payloads --
    against the split written out independently in the program below."""
    src = tmp_path / 'split_words.cpp'
    src.write_text(r'''
#include "wave_ops.h"
#include <cstdio>
#include <cstring>
#include <cstdint>
using namespace pnp;
static void reference(uint32_t u, uint32_t (&w)[4]) {      // the split by truncation, written out: pieces in the high halves
  float x, f, r1, r2;
  std::memcpy(&x, &u, 4);
  const uint32_t p1 = u & 0xffff0000u;
  std::memcpy(&f, &p1, 4);
  r1 = x - f;
  uint32_t v;
  std::memcpy(&v, &r1, 4);
  const uint32_t p2 = v & 0xffff0000u;
  std::memcpy(&f, &p2, 4);
  r2 = r1 - f;
  uint32_t p3;
  std::memcpy(&p3, &r2, 4);
  w[0] = w[1] = w[2] = (p1 >> 16) | (p2 & 0xffff0000u);
  w[3] = (p3 >> 16) | (p3 & 0xffff0000u);
}
int main() {
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  long n = 0, bad = 0;
  auto check = [&](uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    uint32_t ref[4];
    reference(u, ref);
    const u32x4 fly = bf16_split_a(x);
    unsigned w0, w3;
    bf16_split_a_words(x, w0, w3);
    const u32x4 re = bf16_a_from_words(w0, w3);
    const unsigned h = bf16_a3_half(w3);
    const u32x4 lo = bf16_a_from_words(w0, bf16_dup_lo(h | 0xabcd0000u)), hi = bf16_a_from_words(w0, bf16_dup_hi(0x1234u | (h << 16)));
    for (int i = 0; i < 4; ++i)
      if (fly[i] != ref[i] || re[i] != ref[i] || lo[i] != ref[i] || hi[i] != ref[i]) {
        if (bad++ < 5) std::printf("mismatch at %08x dword %d: ref %08x fly %08x rebuilt %08x lo %08x hi %08x\n", u, i, ref[i], fly[i], re[i], lo[i], hi[i]);
        break;
      }
    ++n;
  };
  for (uint32_t sign = 0; sign < 2; ++sign)
    for (uint32_t e = 0; e < 256; ++e)
      for (int k = 0; k < 96; ++k) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        uint32_t m = (uint32_t)(lcg >> 40) & 0x7fffffu;
        if (k >= 64 && k < 80) m &= 0x7f0000u;          // low 16 mantissa bits zero
        if (k >= 80) m &= 0x7fff00u;                    // low 8 mantissa bits zero
        check((sign << 31) | (e << 23) | m);
      }
  const uint32_t fixed[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00008000u, 0x00010000u, 0x7f800000u,
                            0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fffffffu, 0xffffffffu, 0x7fa55a5au, 0x3f800000u};
  for (uint32_t u : fixed) check(u);
  std::printf("checked %ld patterns, %ld mismatches\n", n, bad);
  return bad != 0;
}
''')
    exe = tmp_path / 'split_words'
    emu = os.path.join(ROOT, 'tests', 'emu')
    r = subprocess.run(['g++', '-O1', '-std=c++17', '-x', 'c++', '-include', os.path.join(emu, 'hip_emu.h'), '-I', os.path.join(emu, 'include'),
                        '-I', os.path.join(ROOT, 'epro-pnp_amd', 'csrc'), '-ffp-contract=off', '-Wno-unknown-pragmas', '-Wno-attributes',
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'checked 49168 patterns, 0 mismatches' in out.stdout


@pytest.mark.parametrize('dof,bounds', [(6, None), (6, 'tight'), (4, None), (4, 'tight')])
@pytest.mark.parametrize('N,tune,tiles', [(40, None, 1), (300, '4,4', 4)])
def test_backward_presplit_equals_the_on_the_fly_split_bit_for_bit(backend, monkeypatch, dof, bounds, N, tune, tiles):
    from epropnp import functional as F
    p, hp = _problem(backend, dof, bounds, N)
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, dof)
    g_logw, g_init = _weights(backend)
    for with_init in (True, False):
        plan = F.launch_plan('backward', hp, S, pose_init=with_init)
        assert (plan['waves'], plan['tiles'], plan['bf16'], plan['valu']) == (4, tiles, True, False), plan
        assert _presplit_fits(S, with_init, tiles, N, plan['parked']) == (True, True)
        pin, gin, cin = (p['pose_init'], g_init, cost_init) if with_init else (None, None, None)
        runs = {}
        for knob in (None, 0):
            set_tune(monkeypatch, bwd_mfma=tune, bwd_presplit=knob)
            runs[knob] = [F.amis_backward(hp, samples, g_logw, pin, gin),                                      # per-pair entry
                          F.amis_backward(hp, samples, g_logw, pin, gin, sample_costs=costs, cost_init=cin)]   # DCOST entry
            if N > 64:      # the split entry takes at most ceil(N / 64) parts
                runs[knob] += [F.amis_backward(hp, samples, g_logw, pin, gin, nsplit=2),
                               F.amis_backward(hp, samples, g_logw, pin, gin, nsplit=2, sample_costs=costs, cost_init=cin)]
        for i, entry in enumerate(('per-pair', 'costs', 'split', 'split with costs')[:len(runs[0])]):
            assert all(bool(torch.isfinite(t).all()) for t in runs[None][i]), entry
            assert float(runs[None][i][0].abs().max()) > 0, entry
            _same_bits(runs[None][i], runs[0][i], (entry, with_init))


@pytest.mark.parametrize('N,tune', [(40, None), (300, '4,4')])
def test_backward_presplit_with_a_nan_pose_component(backend, monkeypatch, N, tune):
    """a kept sample with a NaN component: the NaNs that come out carry the same bits on both paths, the other objects stay finite"""
    from epropnp import functional as F
    p, hp = _problem(backend, 6, None, N)
    set_tune(monkeypatch, bwd_mfma=tune)
    samples, costs, cost_init = _forward(backend, hp, p, 6)
    g_logw, g_init = _weights(backend)
    bad = samples.clone()
    bad[3, 0, 1] = float('nan')              # object 0 keeps every sample
    runs = {}
    for knob in (None, 0):
        set_tune(monkeypatch, bwd_mfma=tune, bwd_presplit=knob)
        runs[knob] = (F.amis_backward(hp, bad, g_logw, p['pose_init'], g_init),
                      F.amis_backward(hp, bad, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=cost_init))
    for i in range(2):
        _same_bits(runs[None][i], runs[0][i], i)
        assert not bool(torch.isfinite(runs[None][i][0][0]).all())
        assert bool(torch.isfinite(runs[None][i][0][1:]).all())


def test_a_table_that_fits_only_unsplit_runs_the_on_the_fly_instantiation(backend, monkeypatch):
    """B = 1, N = 16, S = 1400: 15 x P16 x 4 B = 85 KB fit the 160 KB of a CU, 33 x P16 x 4 B = 188 KB do not -- the plan keeps today's
    instantiation (no VALU fallback) and the knob changes nothing."""
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    Sb = 1400
    prob = orc.make_problem(1, 16, 6, seed=64)
    p, cam, _ = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), 6)
    plan = F.launch_plan('backward', hp, Sb, pose_init=True)
    assert (plan['waves'], plan['tiles'], plan['bf16'], plan['valu']) == (4, 1, True, False), plan
    assert _presplit_fits(Sb, True, 1, 16, plan['parked']) == (True, False)
    g = torch.Generator().manual_seed(65)
    samples = p['pose_gt'].cpu()[None] + 0.05 * torch.randn(Sb, 1, 7, generator=g)
    samples[..., 3:] /= samples[..., 3:].norm(dim=-1, keepdim=True)
    samples = samples.to(backend)
    g_logw = torch.randn(Sb, 1, generator=g).to(backend)
    g_init = torch.tensor([0.5]).to(backend)
    costs = torch.rand(Sb, 1, generator=g).to(backend)
    cost_init = F.evaluate_cost(hp, p['pose_init'])
    runs = {}
    for knob in (None, 0):
        set_tune(monkeypatch, bwd_presplit=knob)
        runs[knob] = (F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init),
                      F.amis_backward(hp, samples, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=cost_init))
    for i in range(2):
        assert all(bool(torch.isfinite(t).all()) for t in runs[None][i])
        _same_bits(runs[None][i], runs[0][i], i)


BIG = [pytest.param(600, 128, 128, 4, 'tensor', dict(waves=4, tiles=2), id='B600-N128-S128-4dof'),
       pytest.param(512, 512, 512, 6, None, dict(waves=4, tiles=4), id='B512-N512-S512-6dof')]


@pytest.mark.gpu
@pytest.mark.parametrize('Bb,Nb,Sb,dof,bounds,want', BIG)
def test_big_batch_instantiations_keep_their_bits(monkeypatch, Bb, Nb, Sb, dof, bounds, want):
    """The instantiations that the big batches launch, with every CU busy (two workgroups of 76.8 KB per CU at S = 512, three at
    S = 128), with and without the delta fold (grad_w2d rows parked in LDS behind the larger table): the bits of the on-the-fly path,
    and the same bits from a second launch."""
    import install as emu
    from epropnp import functional as F
    from epropnp.cost_fun import HuberPnPCost
    emu.uninstall()
    dev = torch.device('cuda:0')
    prob = orc.make_problem(Bb, Nb, dof, seed=81, bounds=bounds)
    p, cam, _ = make_layer_objects(prob, dev)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, HuberPnPCost(delta=p['delta']), dof)
    _, stats = F.adaptive_delta(hp.x2d, hp.w2d, 0.5)
    hf = F.PnPProblem(hp.x3d, hp.x2d, hp.w2d, cam, HuberPnPCost(delta=hp.delta), dof).fold_delta(stats, 0.5)
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)
    samples, logw, costs = F.amis_forward(hp, pose_opt, pose_cov, Sb, 4, seed=3, with_costs=True)
    cost_init = F.evaluate_cost(hp, p['pose_init'])
    g = torch.Generator().manual_seed(82)
    g_logw = torch.softmax(logw, 0) * torch.randn(Bb, generator=g).to(dev)
    g_init = torch.randn(Bb, generator=g).to(dev)
    for h, parked in ((hp, False), (hf, True)):
        plan = F.launch_plan('backward', h, Sb, pose_init=True)
        assert {k: plan[k] for k in ('waves', 'tiles', 'bf16', 'valu', 'parked', 'nsplit')} == dict(bf16=True, valu=False, parked=parked, nsplit=1, **want), plan
        assert _presplit_fits(Sb, True, want['tiles'], Nb, parked) == (True, True)
        runs = {}
        for knob in (None, 0, None):
            set_tune(monkeypatch, bwd_presplit=knob)
            out = (F.amis_backward(h, samples, g_logw, p['pose_init'], g_init),
                   F.amis_backward(h, samples, g_logw, p['pose_init'], g_init, sample_costs=costs, cost_init=cost_init))
            if knob in runs:      # the second default launch
                for i in range(2):
                    _same_bits(runs[knob][i], out[i], ('again', i, parked))
            runs[knob] = out
        for i in range(2):
            assert all(bool(torch.isfinite(t).all()) for t in runs[None][i])
            _same_bits(runs[None][i], runs[0][i], (i, parked))
