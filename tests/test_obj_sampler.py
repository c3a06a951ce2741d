"""epropnp.targets.obj_sampler (epropnp_obj_sample_weights) on the assigned targets of the main scene of tests/test_point_targets.py,
num_obj_samples = 24, with the draws the reference made injected (tests/golden/point_targets.npz, tools/make_point_target_golden.py:
the reference's obj_sampler run on the CPU with a recording torch.multinomial).

sample_gt_inds and the gathered extra arrays must equal the fixture's.  Both weight vectors are compared with an fp64 restatement of
deform_pnp_head.py:1148-1174 written here (and that restatement with the reference's fp32 outputs, loosely, so that it restates the
right thing).

Bar: 4 x the larger of the worst errors seen on the CPU emulation and on the MI355X over the cases of this file (each case prints its
worst error); test_bars_under_caps holds it under the cap.
    weights  |w - w64| / w64, both vectors       emulation 5.946e-8, MI355X 5.946e-8   -> bar 2.378e-7, cap 1e-5
             (the two agree to the printed digits: the kernel works in fp64 and rounds once, on both)
"""
import os

import numpy as np
import pytest
import torch

import test_point_targets as tp

WEIGHT_BAR = 2.378e-7     # relative; cap 1e-5
WEIGHT_CAP = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_targets.npz')
CASES = ('half', 'few', 'most')
EPS = 1e-5


def _mod():
    from epropnp import targets
    return targets


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def restated(fg, cen, gt, draws, N, ratio, eps=EPS, num_uniform=None):
    """the reference's arithmetic behind its draws, in fp64"""
    fg, cen = fg.astype(np.float64), cen.astype(np.float64)
    count = fg.sum()
    num_uniform = min(int(round(N * ratio)), int(count)) if num_uniform is None else num_uniform
    r = num_uniform / N
    prob = cen * fg
    prob = prob / max(prob.sum(), eps)
    mix = fg / max(count, 1) * r + prob * (1 - r)
    sgt = gt[draws]
    w = prob[draws] / mix[draws]
    same = sgt[:, None] == sgt[None, :]
    sums = (same * w[None, :]).sum(1)
    sw = w / np.maximum(sums, eps)
    sw = sw / max(sw.mean(), eps)
    uw = 1.0 / np.maximum(same.sum(1), 1)
    uw = uw / max(uw.mean(), eps)
    return sgt, sw, uw, num_uniform


def call(g, name, backend, **kw):
    N = int(g['params'][3])
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    kw.setdefault('uniform_mix_ratio', float(g[f'sampler_{name}_ratio']))
    kw.setdefault('sample_point_inds', d(g[f'sampler_{name}_draws']))
    return _mod().obj_sampler(N, d(g[f'sampler_{name}_fg_mask']), d(g['sampler_centerness']), d(g['sampler_gt_inds']),
                              d(g['sampler_extra_f']), d(g['sampler_extra_i']), **kw)


def test_bars_under_caps():
    assert 0 < WEIGHT_BAR <= WEIGHT_CAP


def test_restatement_restates_the_reference(golden):
    for name in CASES:
        N = int(golden['params'][3])
        sgt, sw, uw, nu = restated(golden[f'sampler_{name}_fg_mask'], golden['sampler_centerness'], golden['sampler_gt_inds'],
                                   golden[f'sampler_{name}_draws'], N, float(golden[f'sampler_{name}_ratio']))
        assert nu == int(golden[f'sampler_{name}_num_uniform']) and np.array_equal(sgt, golden[f'sampler_{name}_out_gt_inds'])
        assert np.allclose(sw, golden[f'sampler_{name}_out_weights'], rtol=1e-5, atol=0)
        assert np.allclose(uw, golden[f'sampler_{name}_out_uniform_weights'], rtol=1e-5, atol=0)
    assert int(golden['sampler_few_num_uniform']) == 5 < int(golden['sampler_half_num_uniform']) == 12


@pytest.mark.parametrize('name', CASES)
def test_sampler_matches_fixture_and_fp64(backend, poisoned_empty, golden, name):
    N = int(golden['params'][3])
    out = call(golden, name, backend)
    assert len(out) == 5 and out[0].dtype == torch.int64 and out[1].dtype == torch.float32 and out[2].dtype == torch.float32
    sgt, sw, uw, ef, ei = (t.cpu().numpy() for t in out)
    assert np.array_equal(sgt, golden[f'sampler_{name}_out_gt_inds'])
    assert np.array_equal(ef, golden[f'sampler_{name}_out_extra_f']) and np.array_equal(ei, golden[f'sampler_{name}_out_extra_i'])
    _, sw64, uw64, _ = restated(golden[f'sampler_{name}_fg_mask'], golden['sampler_centerness'], golden['sampler_gt_inds'],
                                golden[f'sampler_{name}_draws'], N, float(golden[f'sampler_{name}_ratio']))
    worst = max(float(np.abs(sw / sw64 - 1).max()), float(np.abs(uw / uw64 - 1).max()))
    print(f'obj_sampler[{name}] on {backend}: worst relative weight error {worst:.3e} (bar {WEIGHT_BAR:.3e})')
    assert worst <= WEIGHT_BAR
    # what holds without a fixture
    assert abs(float(sw.astype(np.float64).mean()) - 1) < 1e-6 and abs(float(uw.astype(np.float64).mean()) - 1) < 1e-6
    objs = np.unique(sgt)
    sums = np.array([sw[sgt == o].astype(np.float64).sum() for o in objs])
    assert len(objs) > 1 and np.abs(sums / sums[0] - 1).max() < 1e-6
    for o in objs:
        assert len(set(uw[sgt == o].tolist())) == 1


def test_zero_mix_ratio_makes_the_vectors_coincide(backend, golden):
    out = call(golden, 'half', backend, uniform_mix_ratio=0.0)
    assert np.abs(out[1].cpu().numpy().astype(np.float64) / out[2].cpu().numpy() - 1).max() <= 2 * WEIGHT_BAR
    assert np.array_equal(out[0].cpu().numpy(), golden['sampler_half_out_gt_inds'])


def test_few_foreground_points_shrink_the_uniform_part(backend, golden):
    """5 foreground points against round(24 * 0.5) = 12: the mix ratio becomes 5 / 24, and the weights differ from those of 12 / 24"""
    N = int(golden['params'][3])
    fg, draws = golden['sampler_few_fg_mask'], golden['sampler_few_draws']
    assert int(fg.sum()) == 5
    got = call(golden, 'few', backend)[1].cpu().numpy()
    shrunk = restated(fg, golden['sampler_centerness'], golden['sampler_gt_inds'], draws, N, 0.5)[1]
    fixed = restated(fg, golden['sampler_centerness'], golden['sampler_gt_inds'], draws, N, 5 / 24 + 1e-9)[1]
    assert np.abs(got / shrunk - 1).max() <= WEIGHT_BAR and np.abs(got / fixed - 1).max() <= 2 * WEIGHT_BAR
    unshrunk = restated(fg, golden['sampler_centerness'], golden['sampler_gt_inds'], draws, N, 0.5, num_uniform=12)[1]
    assert np.abs(got / unshrunk - 1).max() > 1e-3


def test_no_foreground_gives_the_reference_empties(backend, golden):
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    fg = np.zeros_like(golden['sampler_half_fg_mask'])
    out = _mod().obj_sampler(24, d(fg), d(golden['sampler_centerness']), d(golden['sampler_gt_inds']), d(golden['sampler_extra_f']),
                             d(golden['sampler_extra_i']))
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0,), (0, 3), (0,)]
    assert [t.dtype for t in out] == [torch.int64, torch.float32, torch.float32, torch.float32, torch.int64]


def test_seeded_draws_are_foreground_points(backend, golden):
    N = int(golden['params'][3])
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    fg, T = golden['sampler_half_fg_mask'], len(golden['sampler_gt_inds'])
    index = torch.arange(T, dtype=torch.int64, device=backend)
    outs = []
    for _ in range(2):
        gen = torch.Generator(device=backend)
        gen.manual_seed(17)
        outs.append(_mod().obj_sampler(N, d(fg), d(golden['sampler_centerness']), d(golden['sampler_gt_inds']), index, generator=gen))
    drawn = outs[0][3].cpu().numpy()
    assert drawn.shape == (N,) and fg[drawn].all()
    assert len(set(drawn[:N // 2].tolist())) == N // 2, 'the uniform part is drawn without replacement'
    assert np.array_equal(outs[0][0].cpu().numpy(), golden['sampler_gt_inds'][drawn])
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(tp.bits(a), tp.bits(b))


def test_many_points_and_samples_match_fp64(backend, poisoned_empty):
    """T = 20 000 points, beyond the 16 x 1024 a thread reads ahead in one round (so both the read-ahead loop and its tail run), and
    N = 1500 samples, beyond one per thread; synthetic targets, 37 objects, draws with repeats from the foreground"""
    T, N, ratio = 20000, 1500, 0.5
    rng = np.random.RandomState(23)
    fg = rng.rand(T) < 0.3
    cen = rng.rand(T).astype(np.float32)
    gt = rng.randint(0, 37, T).astype(np.int64)
    draws = rng.choice(np.nonzero(fg)[0], N).astype(np.int64)
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    extra = np.arange(T, dtype=np.int64)
    out = _mod().obj_sampler(N, d(fg), d(cen), d(gt), d(extra), uniform_mix_ratio=ratio, sample_point_inds=d(draws))
    sgt, sw, uw, ex = (t.cpu().numpy() for t in out)
    sgt64, sw64, uw64, nu = restated(fg, cen, gt, draws, N, ratio)
    assert nu == 750 and np.array_equal(sgt, sgt64) and np.array_equal(ex, draws) and len(np.unique(sgt)) == 37
    worst = max(float(np.abs(sw / sw64 - 1).max()), float(np.abs(uw / uw64 - 1).max()))
    print(f'obj_sampler[many] on {backend}: worst relative weight error {worst:.3e} (bar {WEIGHT_BAR:.3e})')
    assert worst <= WEIGHT_BAR
    again = _mod().obj_sampler(N, d(fg), d(cen), d(gt), uniform_mix_ratio=ratio, sample_point_inds=d(draws))
    for a, b in zip(out[:3], again):
        assert torch.equal(tp.bits(a), tp.bits(b))


def test_two_calls_agree_bit_for_bit(backend, golden):
    a, b = call(golden, 'most', backend), call(golden, 'most', backend)
    for x, y in zip(a, b):
        assert torch.equal(tp.bits(x), tp.bits(y))


def test_bad_arguments_are_named(backend, golden):
    d = lambda a: tp.dev(a, backend)      # noqa: E731
    good = [d(golden['sampler_half_fg_mask']), d(golden['sampler_centerness']), d(golden['sampler_gt_inds'])]
    m = _mod()
    with pytest.raises(ValueError, match='fg_mask'):
        m.obj_sampler(24, good[0].float(), good[1], good[2])
    with pytest.raises(ValueError, match='flatten_centerness_targets'):
        m.obj_sampler(24, good[0], good[1].double(), good[2])
    with pytest.raises(ValueError, match='flatten_gt_inds'):
        m.obj_sampler(24, good[0], good[1], good[2][:-1])
    with pytest.raises(ValueError, match='sample_point_inds'):
        m.obj_sampler(24, *good, sample_point_inds=d(golden['sampler_half_draws'][:-1]))
    with pytest.raises(ValueError, match='num_obj_samples'):
        m.obj_sampler(0, *good)
    with pytest.raises(ValueError, match='uniform_mix_ratio'):
        m.obj_sampler(24, *good, uniform_mix_ratio=1.5)
