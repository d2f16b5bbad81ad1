"""The float64 mirror of the 16-bit-weight decode step (tests/oracle_runners.W16Mirror), on the CPU: that it is right — with
nothing rounded it IS the oracle — and that a comparison with it at the GPU tolerance (tests/test_decode_w16_gpu.py: atol 2e-4,
rtol 1e-4) can see what it must: it stands five tolerances from the unrounded oracle at every decode step, and each planted fault
(a swapped fragment half, a dropped residual, a shifted W2 block, a dead head row, a c1 off by one row, a late K row) moves it by
more than one.  The row-offset case measures what the epilogue's c1 term leaves on a row far from centred."""
import functools

import pytest
import torch

from tests import oracle_runners as R
from tests.golden import cases as C
from valle2_amd._lib import h16_dtype

H16 = h16_dtype()
MODEL_TOL = R.w16_model_tol(H16)
MODELS = ('d128', 'd256', 'd512', 'd1024')
ROWS = 3
KEEP = list(range(R.W16_STEPS))
STEPS = KEEP[1:]                        # the decode steps (the logits of step 0 are the prompt pass's: full precision)


@functools.lru_cache(maxsize=None)
def case(model):
    kw, sd, texts, firsts, forced = R.w16_inputs(model)
    cfg = C.cfg_of(kw)
    tx, fs = texts[:ROWS], firsts[:ROWS]
    oracle = R.w16_oracle_logits(sd, cfg, tx, fs, forced)
    R.w16_check_std(oracle[:, 0], model)
    mirror = R.w16_mirror_logits(sd, cfg, tx, fs, forced, KEEP, H16)
    return dict(sd=sd, cfg=cfg, tx=tx, fs=fs, forced=forced, oracle=oracle, mirror=mirror)


def test_model_tolerance_is_the_perf_mode_one():
    from tests import test_bf16_gpu
    assert MODEL_TOL == test_bf16_gpu.MODEL_TOL


@pytest.mark.parametrize('model', MODELS + ('d128s32',))
def test_no_rounding_reproduces_the_oracle(model):
    c = case(model)
    exact = R.w16_mirror_logits(c['sd'], c['cfg'], c['tx'], c['fs'], c['forced'], KEEP, torch.float64)
    err = R.worst(exact, c['oracle'])
    print(f'{model}: mirror with nothing rounded against _forced_logits64: max |diff| = {err:.2e}')
    assert exact.shape == c['oracle'].shape == (ROWS, R.W16_STEPS, c['cfg'].num_audio_tokens + 1)
    assert err <= 1e-9


@pytest.mark.parametrize('model', MODELS + ('d128s32',))
def test_mirror_stands_five_tolerances_from_the_unrounded_oracle(model):
    c = case(model)
    assert R.worst(c['mirror'][:, 0], c['oracle'][:, 0]) <= 1e-9            # step 0: the prompt pass and its head, nothing rounded
    dist = [R.w16_distance(c['mirror'][:, t], c['oracle'][:, t]) for t in STEPS]
    kv_only = R.w16_mirror_logits(c['sd'], c['cfg'], c['tx'], c['fs'], c['forced'], KEEP, H16, weights16=False)
    print(f'{model}: |mirror - oracle| in tolerances per decode step: {[round(x, 1) for x in dist]} '
          f'(max |diff| {R.worst(c["mirror"], c["oracle"]):.2e}; K/V rounded alone: {R.worst(kv_only, c["oracle"]):.2e})')
    assert min(dist) >= R.W16_POWER, dist


@pytest.mark.parametrize('fault', R.W16_FAULTS)
def test_planted_fault_moves_the_mirror_by_more_than_the_tolerance(fault):
    seen = {}
    for model in ('d128', 'd512'):
        c = case(model)
        args = (c['sd'], c['cfg'], c['tx'], c['fs'], c['forced'], KEEP, H16)
        assert torch.equal(R.w16_mirror_logits(*args, fault=None), c['mirror'])
        seen[model] = R.w16_distance(R.w16_mirror_logits(*args, fault=fault)[:, 1:], c['mirror'][:, 1:])
    print(f'fault {fault}: the mirror moves by {({k: round(v, 1) for k, v in seen.items()})} tolerances')
    assert max(seen.values()) > 1.0, seen


def test_unknown_fault_is_refused():
    c = case('d128')
    with pytest.raises(AssertionError):
        R.w16_mirror_logits(c['sd'], c['cfg'], c['tx'], c['fs'], c['forced'], KEEP, H16, fault='no_such_fault')


def test_row_far_from_centred():
    """One row's step inputs carry a constant of 30 standard deviations (its LayerNorm inputs then have |mean| / std >= 20;
    LayerNorm removes the constant, the residual stream keeps it).  Against the same rows with nothing rounded, on that row
    (fp16, the default build; the figures are DESIGN.md 8.2's):

      model   c1 of the fold   c1 of the h16 matrix   the c1 term alone   the head's own share
      d128    3.8e-2           3.7e-2                 5.2e-3              3.6e-2
      d256    5.1e-2           4.6e-2                 1.0e-2              4.4e-2
      d512    4.8e-2           3.2e-2                 2.3e-2              3.2e-2
      d1024   3.6e-2           3.3e-2                 2.2e-2              3.1e-2

    "The c1 term alone" is the distance between the two mirrors — rstd * mean * (rowsum(Wf16) - c1) carried to the logits — and
    exceeds the perf-mode model tolerance (1.5e-2) at d512 and d1024: the finding that made engine.decode_weights16 sum c1 over
    the rounded matrix.  "The head's own share" is offset * (rowsum(proj16) - rowsum(proj)): the head has no norm in front of
    it, so a constant in the residual stream meets the rounding of the head's rows directly, whatever c1 is; with it taken
    out, the row stays within the model tolerance."""
    worst_term = 0.0
    for model in MODELS:
        c = case(model)
        sd, cfg = c['sd'], c['cfg']
        x0 = sd['audio_emb.word_embeddings.weight'][c['forced'][0]] + sd['audio_position_emb.pe'][c['fs'].shape[1] + 1, 0]
        off = 30 * float(x0.std())
        args = (sd, cfg, c['tx'], c['fs'], c['forced'], KEEP)
        trace = {}
        exact = R.w16_mirror_logits(*args, torch.float64, x_offset=(1, off))
        fold = R.w16_mirror_logits(*args, H16, x_offset=(1, off), c1='fold', trace=trace)
        rounded = R.w16_mirror_logits(*args, H16, x_offset=(1, off), c1='rounded')
        proj = sd['proj.weight']
        head = off * (proj.to(H16).double().sum(1) - proj.double().sum(1))
        term = R.worst(fold[1], rounded[1])
        rest = R.worst(rounded[1, 1:] - head, exact[1, 1:])
        print(f'{model}: row with |mean| / std >= {trace["offset_ratio"]:.1f}: |mirror - oracle| {R.worst(fold[1], exact[1]):.2e} with '
              f'c1 of the fold, {R.worst(rounded[1], exact[1]):.2e} with c1 of the h16 matrix; the c1 term alone {term:.2e}; the '
              f"head's own share {float(head.abs().max()):.2e}, without it {rest:.2e}; other rows {R.worst(rounded[[0, 2]], exact[[0, 2]]):.2e}")
        assert trace['offset_ratio'] >= 20
        assert torch.equal(rounded[[0, 2]], c['mirror'][[0, 2]])              # rows are independent
        assert rest <= MODEL_TOL, (model, rest)
        worst_term = max(worst_term, term)
    assert worst_term > MODEL_TOL, worst_term                                  # what c1 of the unrounded fold left
