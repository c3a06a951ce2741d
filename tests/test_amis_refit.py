"""The AMIS proposal refit (csrc/amis_common.h: amis_refit) and the draws that follow it, one step at a time against fp64.

The other AMIS tests recompute the mixture density from the kernel's own records: any self-consistent fit passes them, a wrong one
included.  Here every record i+1 is compared with orc.estimate_6dof / estimate_4dof run in fp64 on exactly what the kernel's refit
had -- its own samples 0 .. (i+1)s and the log-weights that follow from its own records 0 .. i (orc.refit_steps) -- and every later
block of samples with the draw from the kernel's own record and the injected noise.

Yardstick (orc.refit_steps), from the reference alone, per field / refit / object: the larger of |fp32 run - fp64 run| of the same
estimate and the movement of the fp64 run over 8 trials with the samples moved by <= 3 ulp and the log-weights by uniform noise of
amplitude 2e-5 |cost| + 1e-5 (the bar of a fp32 cost against the fp64 one).  Bar = 1e-6 (the atol of the record checks in
test_amis.py) + 4 x yardstick through helpers.assert_within_spread: the device weights come from hardware exp / reciprocal
approximations where the restatement rounds correctly, and the 4x4 factor has cond ~1e5.  Draws: rtol 1e-4, atol 2e-5, yaw 2e-5 rad
modulo 2 pi -- the bars of the iteration-0 checks.  test_yardstick_notices_wrong_fits holds two wrong fits against the same bar.

Every case prints its largest error-to-bar ratio per field (`pytest -s`)."""
import math

import pytest
import torch

import epropnp_oracle as orc
from helpers import assert_within_spread, make_layer_objects, pack_noise, set_tune

FLOOR, K_SPREAD = 1e-6, 4.0
ESS_WELL = 2.5            # the well-conditioned group: effective sample size 1 / sum w^2 of every refit's weights
BLIND = 1e-2              # an L_t yardstick from here on: the reference itself sits on the Cholesky's knife edge
DEGENERATE_FACTOR = 30    # pose_cov scaled by this: proposal 0 far wider than the posterior, one sample takes all the weight


def _kernel_run(backend, dof, S, K, N, B=3, cov_factor=1.0, **kw):
    """lm_solve (3 iterations) + amis_forward on make_problem(seed=7) / make_noise(seed=8) -> prob, noise, samples, records"""
    from epropnp import functional as F
    prob = orc.make_problem(B, N, dof, seed=7)
    noise = orc.make_noise(B, S, K, dof, seed=8)
    p, cam, cf = make_layer_objects(prob, backend)
    hp = F.PnPProblem(p['x3d'], p['x2d'], p['w2d'], cam, cf, dof)
    pose_opt, pose_cov, _ = F.lm_solve(hp, p['pose_init'], 3, with_pose_cov=True)
    samples, _, props = F.amis_forward(hp, pose_opt, pose_cov * cov_factor, S, K, noise=pack_noise(noise, dof).to(backend),
                                       with_proposals=True, **kw)
    return prob, noise, samples.cpu(), props.cpu(), hp


def _ratio(err, spread):
    """largest error-to-bar ratio, errors and yardsticks matched by rank as assert_within_spread does (no rank slack)"""
    e = torch.sort(err.flatten().double(), descending=True).values
    s = torch.sort(spread.flatten().double(), descending=True).values
    return float((e / (FLOOR + K_SPREAD * s)).max())


def _check(tag, dof, K, prob, noise, samples, props, st=None, **kw):
    """every fitted field of records 1 .. K-1 within the bar, every sample of blocks 1 .. K-1 -> orc.refit_steps' dict + 'got'"""
    assert bool(torch.isfinite(samples).all()) and bool(torch.isfinite(props).all())
    S, B = samples.shape[:2]
    s = S // K
    st = orc.refit_steps(prob, dof, samples, props, noise, K, **kw) if st is None else st
    got = orc.record_fields(props[:, 1:].transpose(0, 1), dof)                  # (K-1,B,..)
    st['got'] = got
    for k in orc.REFIT_FIELDS[dof]:
        err = orc.refit_field_diff(got[k].flatten(0, 1), st['expect'][k].flatten(0, 1), k)
        print(f'REFIT {tag} dof{dof} {k}: ratio {_ratio(err, st["spread"][k]):.3f} max err {float(err.max()):.3e} '
              f'max yardstick {float(st["spread"][k].max()):.3e} min ESS {float(st["ess"].min()):.2f}')
    draws = st['draws']
    d_t = (samples[s:, :, :3].double() - draws[..., :3]).abs()
    print(f'REFIT {tag} dof{dof} draws: t {float((d_t / (2e-5 + 1e-4 * draws[..., :3].abs())).max()):.3f}', end=' ')
    if dof == 6:
        d_r = (samples[s:, :, 3:].double() - draws[..., 3:]).abs()
        print(f'q {float((d_r / (2e-5 + 1e-4 * draws[..., 3:].abs())).max()):.3f}')
    else:
        d_r = (samples[s:, :, 3].double() - draws[..., 3]).abs()
        d_r = torch.minimum(d_r, 2 * math.pi - d_r)
        print(f'yaw {float(d_r.max() / 2e-5):.3f}')
    for k in orc.REFIT_FIELDS[dof]:
        err = orc.refit_field_diff(got[k].flatten(0, 1), st['expect'][k].flatten(0, 1), k)
        assert_within_spread(err, st['spread'][k], FLOOR, k=K_SPREAD, what=f'{tag} {k}')
    torch.testing.assert_close(samples[s:, :, :3].double(), draws[..., :3], rtol=1e-4, atol=2e-5)
    if dof == 6:
        torch.testing.assert_close(samples[s:, :, 3:].double(), draws[..., 3:], rtol=1e-4, atol=2e-5)
    else:
        assert float(d_r.max()) < 2e-5, d_r.amax(0)
    return st


def _check_well_conditioned(tag, dof, K, prob, noise, samples, props, **kw):
    st = _check(tag, dof, K, prob, noise, samples, props, **kw)
    assert float(st['ess'].min()) >= ESS_WELL, st['ess']
    assert not bool(st['fallback'].any()) and not bool(st['got']['fallback'].any())


@pytest.mark.parametrize('dof,S,K,N', [(6, 64, 4, 96), (4, 64, 4, 96), (6, 200, 2, 130), (6, 27, 3, 200), (6, 510, 2, 64),
                                       (4, 510, 2, 64), (6, 2048, 2, 48), (4, 2048, 2, 48)])
def test_refit_matches_fp64_estimate(backend, dof, S, K, N):
    """Default parameters: the base shapes, s = 9, sample counts that leave the LDS layout off a multiple of 4 floats, several
    samples per lane of the refit's wave."""
    prob, noise, samples, props, _ = _kernel_run(backend, dof, S, K, N)
    _check_well_conditioned(f'S{S}K{K}N{N}', dof, K, prob, noise, samples, props)


def test_refit_with_the_sampler_state_in_global_scratch(backend):
    from epropnp import functional as F
    dof, S, K, N = 6, 4096, 4, 33
    prob, noise, samples, props, hp = _kernel_run(backend, dof, S, K, N)
    assert F.launch_plan('forward', hp, S, K)['spilled']
    _check_well_conditioned('spilled', dof, K, prob, noise, samples, props)


def test_refit_on_the_half_size_scratch(backend, monkeypatch):
    """amis_refit<6, true>: the reductions as 11 + 10 rows on the partial-cost block (tests/test_fwd_weights_in_lds.py)"""
    from epropnp import functional as F
    dof, S, K, N = 6, 64, 4, 512
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', '1')
    set_tune(monkeypatch, fwd_mfma='4,8', fwd_wlds=1)
    prob, noise, samples, props, hp = _kernel_run(backend, dof, S, K, N)
    plan = F.launch_plan('forward', hp, S, K, scratch=False)
    assert plan == dict(waves=4, tiles=8, G=1, chunks=1, bf16=True, spilled=False, truncated=False, chunked=False), plan
    _check_well_conditioned('half scratch', dof, K, prob, noise, samples, props)


def test_refit_in_the_split_forward(backend, monkeypatch):
    """four workgroups per object: every part runs the refit redundantly on gathered partial costs"""
    from epropnp import functional as F
    dof, S, K, N, G = 6, 48, 3, 300, 4
    monkeypatch.setenv('EPROPNP_FWD_SPLIT', str(G))
    prob, noise, samples, props, hp = _kernel_run(backend, dof, S, K, N)
    assert F.split_scratch(hp, S, K) is not None and F.launch_plan('forward', hp, S, K)['G'] == G
    _check_well_conditioned('split', dof, K, prob, noise, samples, props)


@pytest.mark.parametrize('dof,kw', [(6, dict(acg_mle_iter=0)), (6, dict(acg_mle_iter=1)), (6, dict(acg_mle_iter=2)),
                                    (6, dict(acg_mle_iter=5)), (6, dict(acg_dispersion=0.0)), (6, dict(acg_dispersion=0.05)),
                                    (6, dict(eps=1e-3)), (4, dict(eps=1e-3))])
def test_refit_parameters_off_their_defaults(backend, dof, kw):
    """eps, acg_mle_iter (the kernel branches on 0, 1 and more) and acg_dispersion as the layer's constructor can set them"""
    S, K, N = 96, 3, 64
    prob, noise, samples, props, _ = _kernel_run(backend, dof, S, K, N, **kw)
    tag = ','.join(f'{k}={v}' for k, v in kw.items())
    _check_well_conditioned(tag, dof, K, prob, noise, samples, props, **kw)


@pytest.mark.parametrize('dof', [6, 4])
def test_yardstick_notices_wrong_fits(dof):
    """Power of the bar, no kernel: on the oracle's own fp32 AMIS run of the base shape, a fit with one ACG iteration fewer and a
    covariance divided by 1 - sum w^2 (the `unbiased' weighted estimator) land outside bar in every refit of every object."""
    B, S, K, N = 3, 64, 4, 96
    prob = orc.make_problem(B, N, dof, seed=7)
    noise = orc.make_noise(B, S, K, dof, seed=8)
    cam = orc.Cam(prob['cam_mats'], 0.1)
    pose_opt, pose_cov, _, _ = orc.lm_solve(prob['x3d'], prob['x2d'], prob['w2d'], cam, prob['delta'], prob['pose_init'],
                                            with_pose_cov=True, num_iter=3)
    samples, _, pr = orc.amis(prob['x3d'], prob['x2d'], prob['w2d'], cam, prob['delta'], pose_opt, pose_cov, noise, S, K,
                              return_proposals=True)
    st = _check('oracle fp32', dof, K, prob, noise, samples, orc.pack_records(pr, dof))
    s = S // K
    for i in range(K - 1):
        M, lw = (i + 1) * s, st['logw'][i]
        w = torch.softmax(lw, dim=0)
        wrong = {'L_t': st['expect']['L_t'][i] / (1 - (w * w).sum(0)).sqrt()[:, None, None]}       # chol(C / c) = chol(C) / sqrt(c)
        if dof == 6:
            wrong['L_r'] = orc.estimate_6dof(samples[:M].double(), lw, acg_mle_iter=2)[2]
        for k, v in wrong.items():
            err = orc.refit_field_diff(v, st['expect'][k][i], k)
            bar = FLOOR + K_SPREAD * st['spread'][k][i]
            print(f'REFIT mutant dof{dof} refit {i} {k}: err / bar {(err / bar).tolist()}')
            assert bool((err > bar).all()), (k, i, err, bar)


@pytest.mark.parametrize('dof', [6, 4])
def test_refit_with_degenerate_weights(backend, dof):
    """An overconfident start: pose_cov x DEGENERATE_FACTOR makes proposal 0 far wider than the posterior and one sample takes nearly
    all the weight (ESS -> 1), the regime in which a covariance formed as E[dd^T] - dd^T about the previous mode cancels.  On top of
    the checks above the kernel reports the Cholesky fallback (record slot 37) exactly where the fp64 estimate takes it, wherever
    the reference is not itself on the knife edge (L_t yardstick below BLIND); the case must stay degenerate and mostly not blind.

    Factor, of {10, 30, 100}: 10 leaves 4 seen refits below ESS 1.1 for 4-DoF (8 are asked for).  30, on the CPU emulation: the
    single-pass fp32 covariance fell back to the default factor in 17 (6-DoF) and 1 (4-DoF) of 48 refits where fp64 never does, L_t
    up to 3e3 x its own size off.  Centred on the new mean but still summed in fp32, two 6-DoF refits kept falling back: one sample
    at 1 - 1e-5, the next at 1e-5, the rest below 1e-13 -- a covariance of condition > 1e7 that fp32 entries cannot hold (the
    yardstick's single fp32 run fails on it or not by chance: it failed on the emulation's inputs and passed on the device's).  Summed
    in fp64 no fallback is left; largest error-to-bar ratios on the MI355X: L_t 0.04 / 0.21, kappa 0.79, L_r 0.16, mode 0.03.
    100 is 23 of 48 blind for 6-DoF and adds exactly singular covariances (one sample at 1 - 1e-16), a coin toss in fp64 as well."""
    S, K, N, B = 128, 4, 64, 16
    prob, noise, samples, props, _ = _kernel_run(backend, dof, S, K, N, B=B, cov_factor=float(DEGENERATE_FACTOR))
    st = orc.refit_steps(prob, dof, samples, props, noise, K)
    sees = st['spread']['L_t'] < BLIND
    got_fb = orc.record_fields(props[:, 1:].transpose(0, 1), dof)['fallback']
    print(f'REFIT degenerate dof{dof}: blind {int((~sees).sum())} of {sees.numel()}, ESS < 1.1 and seen {int(((st["ess"] < 1.1) & sees).sum())}, '
          f'fallback kernel {got_fb.nonzero().tolist()} oracle {st["fallback"].nonzero().tolist()} (refit, object)')
    assert int((~sees).sum()) <= sees.numel() // 2
    assert int(((st['ess'] < 1.1) & sees).sum()) >= 8
    _check('degenerate', dof, K, prob, noise, samples, props, st=st)
    assert torch.equal(got_fb[sees], st['fallback'][sees]), (got_fb.nonzero().tolist(), st['fallback'].nonzero().tolist())
