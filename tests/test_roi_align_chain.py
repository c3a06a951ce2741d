"""The auxiliary slice of the detection head on the package (EPro-PnP-Det deform_pnp_head.py:940-946, :977-986): extract_rois ->
query . key_roi / sqrt(d) -> logsoftmax_across_rois(extra_dim=1), differentiated to key and query, against the same chain in fp64 on
the key_roi of test_roi_align's oracle and test_roi's oracle of the cross-RoI logsumexp, at the bars test_roi.py holds the logsumexp
part to (FWD_BAR64 / BWD_BAR64: absolute forward error, backward error relative to the largest |gradient|).  RoIAlign adds half an ulp
of key_roi to that (test_roi_align.py), far inside those bars."""
import math

import pytest
import torch

import test_roi as tr
import test_roi_align as ta

HEADS, DIM, CELLS = 2, 4, (7, 7)
ROIS = [(0, 10.125, 6.5, 90.75, 70.375), (0, 40.5, 30.5, 130.125, 100.625), (1, 20.25, 10.5, 100.375, 90.125),
        (1, 60.625, 50.125, 150.25, 120.25), (0, 5.75, 40.25, 70.625, 115.375)]


def _chain(key_roi, query, rois, logsoftmax):
    n = len(ROIS)
    attn = query @ key_roi.reshape(n, HEADS, DIM, CELLS[0] * CELLS[1]) / math.sqrt(DIM)
    return logsoftmax(attn.reshape(n, HEADS, *CELLS), rois, 1)


@pytest.mark.parametrize('how', ['nchw', 'cl'])
def test_extract_rois_feeds_the_cross_roi_logsoftmax(backend, how):
    from epropnp import roi
    g = torch.Generator().manual_seed(41)
    key = torch.randn(2, HEADS * DIM, 32, 40, generator=g)
    value = torch.randn(2, HEADS * DIM, 32, 40, generator=g)
    x2d = torch.randn(2, 2, 128, 160, generator=g)
    query = torch.randn(len(ROIS), HEADS, 1, DIM, generator=g)
    cot = torch.randn(len(ROIS), HEADS, *CELLS, generator=g)
    rois = torch.tensor(ROIS, dtype=torch.float32)
    assert tr.fence_distance(rois, *CELLS) >= tr.FENCE

    # fp64: the per-sample RoIAlign oracle (forward and, through its own backward, the gradient w.r.t. key), autograd in between
    key_roi64, _, info = ta.oracle(key.double().numpy(), ROIS, CELLS, 0.25, 0, True)
    assert info['cut'] >= ta.FENCE and info['ceil'] >= ta.FENCE_CEIL, info
    kr = torch.from_numpy(key_roi64).requires_grad_(True)
    q64 = query.double().requires_grad_(True)
    want = _chain(kr, q64, rois, lambda x, r, extra: x - tr.oracle(x, r).logsumexp(dim=extra, keepdim=True))
    g_kr, want_gq = torch.autograd.grad((want * cot.double()).sum(), [kr, q64])
    want_gk = torch.from_numpy(ta.oracle(key.double().numpy(), ROIS, CELLS, 0.25, 0, True, g_kr.numpy())[1][0])

    k = ta.layout(key.to(backend), how).requires_grad_(True)
    v = ta.layout(value.to(backend), how)
    q = query.to(backend).requires_grad_(True)
    x2d_roi, key_roi, value_roi = roi.extract_rois(rois.to(backend), x2d.to(backend), k, v, roi_shape=CELLS, output_stride=4)
    assert x2d_roi.shape == (len(ROIS), 2, *CELLS) and value_roi.shape == key_roi.shape == (len(ROIS), HEADS * DIM, *CELLS)
    got = _chain(key_roi, q, rois.to(backend), roi.logsoftmax_across_rois)
    got_gk, got_gq = torch.autograd.grad((got * cot.to(backend)).sum(), [k, q])
    tr.check('forward', f'chain {how}', tr.fwd_error(got.detach(), want.detach()), tr.FWD_BAR64)
    tr.check('backward', f'chain {how} dkey', tr.bwd_error(got_gk, want_gk), tr.BWD_BAR64)
    tr.check('backward', f'chain {how} dquery', tr.bwd_error(got_gq, want_gq.detach()), tr.BWD_BAR64)
