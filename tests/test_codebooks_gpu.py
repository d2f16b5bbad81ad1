"""More than 8 codebooks on the device: `vh_embed_sum_pe` at 9 to 32 tables (embed_sum_pe_many_kernel) and ValleNAR with 16
and 32 codebooks (EnCodec at 12 / 24 kbps) against the real reference's fixture (tests/golden/codebooks.npz,
gen_golden_codebooks.py) and the oracle."""
import pytest
import torch

from tests.golden import cases as C
from tests.golden.gen_golden_codebooks import NAR_Q, NAR_Q_STAGES, PREP_STRIDE, nar_q_inputs
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _tables(n, vocab, d, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(vocab + j, d, generator=g) for j in range(n)]


@pytest.mark.parametrize('n', [1, 8, 9, 16, 32])
def test_embed_sum_pe_is_the_sequential_fp32_sum(n):
    """sum_j tables[j][ids[..., j]] in table order, then + pe: bit-equal to torch's left-to-right fp32 sum, with and
    without per-row offsets (lens / row_pos0 / row_t0)."""
    from valle2_amd import _lib, kernels
    d, B, T = 96, 3, 11
    tabs = _tables(n, 40, d, 100 + n)
    g = torch.Generator().manual_seed(n)
    ids = torch.stack([torch.randint(0, t.shape[0], (B, T), generator=g) for t in tabs], dim=-1)
    pe = torch.randn(64, d, generator=g)

    def ref_rows(b, t, pos):
        e = tabs[0][ids[b, t, 0]].clone()
        for j in range(1, n):
            e = e + tabs[j][ids[b, t, j]]
        return e + pe[pos]

    dt = [t.to(DEV) for t in tabs]
    out = torch.zeros(B, T + 2, d, device=DEV)
    kernels.embed_sum_pe(ids.to(DEV), dt, pe.to(DEV), 5, out, out_t0=2)
    want = torch.zeros(B, T + 2, d)
    for b in range(B):
        for t in range(T):
            want[b, 2 + t] = ref_rows(b, t, 5 + t)
    assert torch.equal(out.cpu(), want)
    # ragged: per-row valid length, position and output offsets in one launch
    lens, pos0, t0 = [11, 4, 7], [0, 9, 3], [0, 6, 2]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)   # noqa: E731
    out = torch.zeros(B, 20, d, device=DEV)
    kernels.embed_sum_pe(ids.to(DEV), dt, pe.to(DEV), 0, out, lens=i32(lens), row_pos0=i32(pos0), row_t0=i32(t0),
                         max_pos=20)
    want = torch.zeros(B, 20, d)
    for b in range(B):
        for t in range(lens[b]):
            want[b, t0[b] + t] = ref_rows(b, t, pos0[b] + t)
    assert torch.equal(out.cpu(), want)
    _lib.raise_device_errors(DEV)


def test_embed_sum_pe_dropout_at_16_tables_is_the_field_applied_to_the_sum():
    from valle2_amd import dropout, kernels
    d, B, T, n = 64, 2, 9, 16
    tabs = [t.to(DEV) for t in _tables(n, 30, d, 7)]
    ids = torch.stack([torch.randint(0, 30, (B, T), generator=torch.Generator().manual_seed(j)) for j in range(n)],
                      dim=-1).to(DEV)
    pe = torch.randn(32, d, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain = torch.zeros(B, T, d, device=DEV)
    kernels.embed_sum_pe(ids, tabs, pe, 0, plain)
    spec = dropout.spec(1234, 5, 0.25)
    dropped = torch.zeros(B, T, d, device=DEV)
    kernels.embed_sum_pe(ids, tabs, pe, 0, dropped, drop=spec)
    keep = dropout.mask(spec, B * T, d, DEV).view(B, T, d).bool()
    assert 0.6 < float(keep.float().mean()) < 0.9
    want = torch.where(keep, plain / (1 - 0.25), torch.zeros_like(plain))
    torch.testing.assert_close(dropped, want, rtol=1e-6, atol=0)


def test_embed_sum_pe_bad_id_in_table_20_raises_the_device_error():
    from valle2_amd import _lib, kernels
    d, n = 64, 24
    tabs = [t.to(DEV) for t in _tables(n, 10, d, 9)]
    ids = torch.zeros(2, 3, n, dtype=torch.int64)
    ids[1, 2, 20] = 10 + 20                                   # table 20 has 30 rows: id 30 is outside it
    out = torch.zeros(2, 3, d, device=DEV)
    _lib.raise_device_errors(DEV)
    kernels.embed_sum_pe(ids.to(DEV), tabs, None, 0, out)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(IndexError):
        _lib.raise_device_errors(DEV)
    _lib.raise_device_errors(DEV)


def test_more_than_32_tables_is_refused():
    from valle2_amd import _lib, kernels
    tabs = [torch.zeros(4, 16, device=DEV)] * 33
    with pytest.raises(_lib.VhError, match='32'):
        kernels.embed_sum_pe(torch.zeros(1, 2, 33, dtype=torch.int64, device=DEV), tabs, None, 0,
                             torch.zeros(1, 2, 16, device=DEV))


def _nar(which):
    from tests.test_models_gpu import build
    kw, sd, batch = nar_q_inputs(which)
    return kw, sd, batch, build('ValleNAR', kw, sd)


@pytest.mark.parametrize('which', sorted(NAR_Q))
def test_nar_many_codebooks_prepare_and_stage_logits_match_the_reference(which):
    gold = load_golden('codebooks')
    kw, sd, batch, m = _nar(which)
    assert m.config.num_quantizers == {'q16': 16, 'q32': 32}[which]
    for stage in NAR_Q_STAGES[which]:
        y, p = m._prepare_audio_codes(batch['codes'], stage)
        assert p == int(gold[f'{which}_prefix_{stage}'])
        torch.testing.assert_close(y.cpu()[:, :, ::PREP_STRIDE], gold[f'{which}_prep_{stage}'], rtol=1e-6, atol=1e-6)
        logits, p = m.stage_logits(batch, stage)
        torch.testing.assert_close(logits.cpu(), gold[f'{which}_logits_{stage}'], rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize('which,stage', [('q16', 12), ('q32', 20)])
def test_nar_many_codebooks_training_step_matches_the_oracle(which, stage):
    """Loss and every parameter's gradient (relative norm 1e-3) against the oracle's autograd; the tables of
    codebooks 8 and up receive gradients (prompt frames and, below the stage, target frames)."""
    from oracle import valle_oracle as O
    from tests.test_train_gpu import _grad_check
    kw, sd, batch, m = _nar(which)
    cfg = C.cfg_of(kw)
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    ref_loss = O.nar_training_loss(params, cfg, batch, stage)
    ref_loss.backward()
    loss = m.training_step(batch, stage=stage)
    torch.testing.assert_close(loss.detach().cpu(), ref_loss.detach(), rtol=1e-5, atol=1e-6)
    loss.backward()
    used = sorted(k for k, v in params.items() if v.grad is not None and v.grad.abs().sum() > 0)
    for j in (8, stage - 1, cfg.num_quantizers - 1):
        assert f'codes_embs.{j}.word_embeddings.weight' in used
    _grad_check(m, params, used)


@pytest.mark.parametrize('which', sorted(NAR_Q))
def test_nar_many_codebooks_generate_batch_matches_the_oracle_per_utterance(which):
    from oracle import valle_oracle as O
    kw, sd, _, m = _nar(which)
    cfg = C.cfg_of(kw)
    q = cfg.num_quantizers
    g = torch.Generator().manual_seed(q)
    us = [(torch.randint(0, cfg.vocab_size, (tx,), generator=g),
           torch.randint(0, cfg.num_audio_tokens, (tc, q), generator=g),
           torch.randint(0, cfg.num_audio_tokens, (ty,), generator=g)) for tx, tc, ty in [(9, 12, 14), (6, 20, 9), (11, 5, 17)]]
    outs = m.generate_batch([u[0].to(DEV) for u in us], [u[1].to(DEV) for u in us], [u[2].to(DEV) for u in us],
                            greedy=True)
    for (text, pc, first), got in zip(us, outs):
        ref = O.nar_generate(sd, cfg, text[:4], pc, text[4:], first, greedy=True)
        assert got.shape == ref.shape == (first.shape[0], q)
        assert torch.equal(got.cpu(), ref), f'{(got.cpu() != ref).sum().item()} of {ref.numel()} tokens differ'
    one = m.generate(us[0][0][:4].to(DEV), us[0][1].to(DEV), us[0][0][4:].to(DEV), us[0][2].to(DEV), greedy=True)
    assert tuple(one.shape) == (us[0][2].shape[0], q) and torch.equal(one, outs[0])


def test_nar_16_codebooks_perf_mode_within_its_tolerance():
    gold = load_golden('codebooks')
    _, _, batch, m = _nar('q16')
    for stage in NAR_Q_STAGES['q16']:
        logits, _ = m.stage_logits(batch, stage, perf_mode=True)
        err = float((logits.cpu() - gold[f'q16_logits_{stage}']).abs().max())
        assert err < 5e-2, f'stage {stage}: perf-mode logits off by {err:.2e}'
    outs = m.generate_batch([batch['tokens'][0].to(DEV)], [batch['codes'][0, :5].to(DEV)], [batch['codes'][0, 5:, 0].to(DEV)],
                            greedy=True, perf_mode=True)
    assert tuple(outs[0].shape) == (10, 16)
