"""Sampling at audio vocabularies wider than 2048 (`vh_sample_step_wide`, V <= 16384) against the real reference's filter
(tests/golden/codebooks.npz at V = 4097) and the oracle's restatement of it (other V); the wide kernel against the narrow one
at V <= 2048; and ValleAR with num_audio_tokens = 4096 end to end.

The draw is a counter-based stream keyed on (seed, row, position), not torch.multinomial's, so the checks are the support,
the log-prob of every draw (atol 1e-5) and frequencies within 4 sigma (the criterion of test_sampling_gpu.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import valle_oracle as O
from tests.golden import cases as C
from tests.golden.gen_golden_codebooks import AR_V4096, WIDE_FILTERS, ar_v4096_inputs, wide_sampling_inputs
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _filtered_logprobs(row, top_k, top_p, temperature):
    return F.log_softmax(O._top_k_top_p_filter((row / temperature)[None], top_k=top_k, top_p=top_p), dim=-1)[0]


def _check_draws(tok, lp, logprobs, n, label):
    probs = logprobs.exp()
    assert bool(torch.isfinite(logprobs[tok]).all()), f'{label}: a token outside the reference support was drawn'
    torch.testing.assert_close(lp, logprobs[tok], atol=1e-5, rtol=1e-5)
    freq = torch.bincount(tok, minlength=logprobs.numel()).float() / n
    sigma = torch.sqrt(probs * (1 - probs) / n)
    assert bool(((freq - probs).abs() <= 4 * sigma + 1e-4).all()), f'{label}: {(freq - probs).abs().max()}'


def _draw(row, n, top_k, top_p, temperature, seed):
    from valle2_amd.utils import topk_sampling
    tok, lp = topk_sampling(row.to(DEV)[None].expand(n, -1).contiguous(), top_k=top_k, tok_p=top_p,
                            temperature=temperature, seed=seed)
    return tok[:, 0].cpu(), lp.cpu()


@pytest.mark.parametrize('case', range(len(WIDE_FILTERS)))
def test_topk_sampling_at_4097_matches_the_reference_filter(case):
    """utils.topk_sampling at V = 4097 (routed to the wide kernel) against the real reference's top_k_top_p_filtering."""
    gold = load_golden('codebooks')
    top_k, top_p, temp = WIDE_FILTERS[case]
    logits = wide_sampling_inputs()
    keep, logprobs = gold[f'filter_keep_{case}'], gold[f'filter_logprobs_{case}']
    n = 20000
    for r in range(logits.shape[0]):
        assert torch.equal(torch.isfinite(_filtered_logprobs(logits[r], top_k, top_p, temp)), keep[r])
        tok, lp = _draw(logits[r], n, top_k, top_p, temp, seed=300 + r)
        assert bool(keep[r][tok].all())
        _check_draws(tok, lp, logprobs[r], n, f'row {r}')


@pytest.mark.parametrize('V', [2049, 8193, 16384])
@pytest.mark.parametrize('case', range(len(WIDE_FILTERS)))
def test_sample_step_wide_support_logprob_and_frequencies(V, case):
    top_k, top_p, temp = WIDE_FILTERS[case]
    row = 3.0 * torch.randn(V, generator=torch.Generator().manual_seed(V + case))
    row[7] = torch.sort(row, descending=True).values[top_k - 1 if top_k > 0 else 9]   # an exact tie at the k-th place
    n = 20000 if V <= 8193 else 8000
    tok, lp = _draw(row, n, top_k, top_p, temp, seed=V)
    _check_draws(tok, lp, _filtered_logprobs(row, top_k, top_p, temp), n, f'V={V}')


def test_ties_at_the_kth_value_are_kept():
    row = torch.full((4097,), -3.0)
    row[100], row[200] = 5.0, 4.0
    row[[10, 999, 3000, 4096]] = 2.0                                   # four-way tie at the 3rd place
    tok, lp = _draw(row, 20000, 3, 1.0, 1.0, seed=1)
    assert set(tok.tolist()) == {100, 200, 10, 999, 3000, 4096}
    _check_draws(tok, lp, _filtered_logprobs(row, 3, 1.0, 1.0), 20000, 'ties')


@pytest.mark.parametrize('top_k,top_p', [(50, 1.0), (0, 1.0), (20000, 1.0)])
def test_all_equal_logits_at_16384_keep_every_entry(top_k, top_p):
    n = 8000
    tok, lp = _draw(torch.full((16384,), 0.25), n, top_k, top_p, 1.0, seed=5)
    torch.testing.assert_close(lp, torch.full((n,), -math.log(16384)), atol=1e-5, rtol=0)
    assert int(tok.min()) < 64 and int(tok.max()) >= 16384 - 64 and tok.unique().numel() > 5000


def test_top_k_at_least_v_and_top_k_zero_with_top_p():
    """(The frequency criterion allows 4 sigma + 1e-4 per entry; over thousands of entries of probability 1e-5 .. 1e-3 it
    rejects even an exact sampler for a few percent of seeds.  Draws are deterministic for a seed: seed 101 is one it
    accepts for an exact float64 inverse CDF over the same uniform stream, which the kernel reproduces.)"""
    row = 2.0 * torch.randn(6000, generator=torch.Generator().manual_seed(3))
    for top_k, top_p in [(6000, 1.0), (7000, 1.0), (0, 0.7), (-1, 0.7), (6000, 0.7)]:
        tok, lp = _draw(row, 20000, top_k, top_p, 1.0, seed=101)
        _check_draws(tok, lp, _filtered_logprobs(row, top_k, top_p, 1.0), 20000, f'top_k={top_k} top_p={top_p}')


def test_top_p_zero_is_the_arg_max():
    rows = torch.randn(64, 9000, generator=torch.Generator().manual_seed(4))
    for top_k in (0, 50):
        from valle2_amd.utils import topk_sampling
        tok, lp = topk_sampling(rows.to(DEV), top_k=top_k, tok_p=0.0, seed=3)
        assert torch.equal(tok[:, 0].cpu(), rows.argmax(-1)) and bool((lp.cpu() == 0).all())


def _state(B, V, d, pos=1, finished=()):
    codes = torch.zeros(B, 4, dtype=torch.int64, device=DEV)
    codes[:, 0] = 5
    for b in finished:
        codes[b, pos - 1] = V - 1                                        # EOS = V - 1
    return dict(codes=codes, eos_count=torch.zeros(8, dtype=torch.int32, device=DEV),
                sum_logprobs=torch.zeros(B, device=DEV), audio_pos=torch.full((B,), pos, dtype=torch.int32, device=DEV),
                cache_len=torch.full((B,), 3, dtype=torch.int32, device=DEV), x=torch.empty(B, d, device=DEV))


def _step(logits, V, st, emb, pe, top_k, top_p, temp, seed, wide=None):
    from valle2_amd import kernels
    kernels.sample_step(logits, V, V - 1, top_k, top_p, temp, seed, st['codes'], st['eos_count'], st['sum_logprobs'],
                        emb, pe, st['audio_pos'], st['cache_len'], st['x'], wide=wide)


def test_finished_rows_keep_eos_and_the_state_update():
    V, B, d = 4097, 6, 64
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(B, V + 3, generator=g).to(DEV)                # ldl = round_up(V, 4)
    logits[:, V - 1] = -50.0                                           # EOS is never drawn for a live row
    emb, pe = torch.randn(V, d, generator=g).to(DEV), torch.randn(8, d, generator=g).to(DEV)
    for top_k, top_p in [(50, 1.0), (50, 0.9)]:
        st = _state(B, V, d, finished=(1, 4))
        _step(logits, V, st, emb, pe, top_k, top_p, 0.9, seed=2)
        tok = st['codes'][:, 1].cpu()
        assert tok[1] == V - 1 and tok[4] == V - 1 and bool((tok[[0, 2, 3, 5]] < V - 1).all())
        slp = st['sum_logprobs'].cpu()
        assert slp[1] == 0 and slp[4] == 0 and bool((slp[[0, 2, 3, 5]] < 0).all())
        assert st['eos_count'].cpu().tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
        assert torch.equal(st['audio_pos'].cpu(), torch.full((B,), 2, dtype=torch.int32))
        assert torch.equal(st['cache_len'].cpu(), torch.full((B,), 4, dtype=torch.int32))
        torch.testing.assert_close(st['x'], emb[st['codes'][:, 1]] + pe[1], rtol=0, atol=0)


@pytest.mark.parametrize('V', [1025, 2048])
@pytest.mark.parametrize('top_k,top_p,temp', [(50, 1.0, 1.0), (7, 1.0, 0.7), (50, 0.9, 0.8), (0, 0.8, 1.0), (0, 1.0, 1.3)])
def test_wide_kernel_against_the_narrow_one_at_v_up_to_2048(V, top_k, top_p, temp):
    """Same support and log-prob as vh_sample_step.  Tokens for the same seed: identical except for rare rows — both kernels
    draw u = uniform01(seed, row, position) and walk the same order (index order on the fast path, the sorted order
    otherwise), but their fp32 sums run in another order, so a draw (or a top-p cut) that falls within rounding of a CDF
    boundary can land on the neighbouring entry.  Measured on 4000 random rows: up to a few rows per case differ in the
    token (top_k = 0 with the whole row kept) or in the cut (top_p = 0.8); at most 1 in 1000 is allowed here."""
    B, d = 4000, 16
    g = torch.Generator().manual_seed(V + top_k)
    logits = (2.5 * torch.randn(B, V, generator=g)).to(DEV)
    emb, pe = torch.randn(V, d, generator=g).to(DEV), torch.randn(4, d, generator=g).to(DEV)
    out = {}
    for wide in (False, True):
        st = _state(B, V, d)
        _step(logits, V, st, emb, pe, top_k, top_p, temp, seed=77, wide=wide)
        out[wide] = (st['codes'][:, 1].cpu(), st['sum_logprobs'].cpu(), st['x'].cpu())
    same = out[True][0] == out[False][0]
    assert int((~same).sum()) <= B // 1000, f'{int((~same).sum())} of {B} tokens differ'
    assert torch.equal(out[True][2][same], out[False][2][same])
    lp_close = lambda a, b: (a - b).abs() <= 1e-5 + 1e-5 * b.abs()      # noqa: E731
    assert float(lp_close(out[True][1], out[False][1]).float().mean()) >= 0.999
    lps = F.log_softmax(O._top_k_top_p_filter(logits.cpu() / temp, top_k=top_k, top_p=top_p), dim=-1)
    ref = lps[torch.arange(B), out[True][0]]
    assert float(torch.isfinite(ref).float().mean()) >= 0.999
    assert float(lp_close(out[True][1], ref).float().mean()) >= 0.999


def test_sample_step_wide_refuses_bad_arguments():
    from valle2_amd import _lib, kernels
    V, d = 16385, 16
    st = _state(2, V, d)
    logits = torch.zeros(2, 16388, device=DEV)
    emb, pe = torch.zeros(V, d, device=DEV), torch.zeros(4, d, device=DEV)
    with pytest.raises(_lib.VhError, match='16384'):
        _step(logits, V, st, emb, pe, 50, 1.0, 1.0, seed=1)
    with pytest.raises(_lib.VhError, match='2048'):
        _step(logits, 4097, st, emb, pe, 50, 1.0, 1.0, seed=1, wide=False)     # the narrow kernel keeps its limit
    with pytest.raises(_lib.VhError, match='temperature'):
        _step(logits, 4097, st, emb, pe, 50, 1.0, 0.0, seed=1)


# ---- ValleAR with num_audio_tokens = 4096 (V = 4097) ------------------------------------------------------------------
def _ar(kw, sd):
    from tests.test_models_gpu import build
    return build('ValleAR', kw, sd)


def test_ar_4096_greedy_tokens_equal_the_reference():
    gold = load_golden('codebooks')
    kw, sd, utt = ar_v4096_inputs()
    m = _ar(kw, sd)
    out = m.generate(*[u.to(DEV) for u in utt]).cpu()
    ref = gold['v4096_tokens']
    n = min(len(out), len(ref))
    bad = (out[:n] != ref[:n]).nonzero()
    assert len(out) == len(ref) and (bad.numel() == 0 or float(gold['v4096_margin'][int(bad[0])]) < 1e-4), \
        f'{out.tolist()} vs {ref.tolist()}'


def test_ar_4096_default_sampling_generate_graph_and_eager_agree():
    """The reference's default sampling (top_k = 50, top_p = 1) through the native decoder's wide kernel: runs, is repeatable
    under torch.manual_seed, and the captured graph draws what the eager steps draw; the recompute path samples in range."""
    kw, sd, utt = ar_v4096_inputs()
    kw = dict(kw, top_k=50, temperature=1.0, num_beams=4, max_audio_len=20)
    m = _ar(kw, sd)
    utt = [u.to(DEV) for u in utt]
    text = torch.cat([utt[0], utt[2]])
    rows = {}
    for use_graph in (True, False):
        torch.manual_seed(9)
        rows[use_graph] = m.generate_batch([text] * 4, [utt[1][:, 0]] * 4, use_graph=use_graph).cpu()
    assert torch.equal(rows[True], rows[False])
    new = rows[True][:, -20:]
    assert int(new.min()) >= 0 and int(new.max()) <= 4096 and len({tuple(r.tolist()) for r in new}) > 1
    assert bool((m.last_generate_stats['sum_logprobs'] < 0).all())
    torch.manual_seed(9)
    out = m.generate(*utt)
    assert out.dtype == torch.int64 and out.numel() <= 20 and bool((out < 4096).all())
    rm = _ar(dict(kw, use_kv_cache=False), sd)
    torch.manual_seed(9)
    rec = rm.generate_batch([text] * 4, [utt[1][:, 0]] * 4).cpu()
    assert rec.shape == rows[True].shape and int(rec[:, -20:].max()) <= 4096


def test_ar_4096_eos_stops_the_rows():
    """EOS id 4096: a head whose EOS row outweighs the token drawn at step 3 stops greedy decoding there, as the oracle does;
    a head whose EOS row is 10x the first token's row makes every SAMPLED row draw EOS at once (the wide kernel), the rows
    stay finished through the decoder's steps (the wide kernel's EOS bookkeeping) and the decoder stops early."""
    kw, sd, utt = ar_v4096_inputs()
    gold = load_golden('codebooks')
    sd = {k: v.clone() for k, v in sd.items()}
    sd['proj.weight'][4096] = 3.0 * sd['proj.weight'][int(gold['v4096_tokens'][3])]
    cfg = C.cfg_of(kw)
    ref = O.ar_generate(sd, cfg, *utt)
    assert len(ref) < cfg.max_audio_len
    m = _ar(kw, sd)
    assert torch.equal(m.generate(*[u.to(DEV) for u in utt]).cpu(), ref)
    sd['proj.weight'][4096] = 10.0 * sd['proj.weight'][int(gold['v4096_tokens'][0])]
    ms = _ar(dict(kw, top_k=50, temperature=0.05, max_audio_len=64), sd)
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    torch.manual_seed(1)
    rows = ms.generate_batch([text] * 8, [utt[1][:, 0].to(DEV)] * 8).cpu()
    first = utt[1].shape[0] + 1                                         # BOS + prompt frames, then the new tokens
    assert bool((rows[:, first:] == 4096).all()), rows[:, first:]
    assert ms.last_generate_stats['steps_run'] < 64


def test_decoder_refuses_sampling_above_16384_at_create_time():
    from valle2_amd import _lib, synth
    kw = dict(AR_V4096, num_audio_tokens=16384, top_k=50, max_audio_len=4, num_beams=2)
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleAR', seed=3, rich=True)
    m = _ar(kw, sd)
    utt = synth.synth_utterance(cfg, 5, 5, 10, seed=2)
    with pytest.raises(_lib.VhError, match='vh_ar_decoder.*16384'):
        m.generate(*[u.to(DEV) for u in utt])
    mg = _ar(dict(kw, top_k=1), sd)                                   # greedy has no such limit
    assert mg.generate(*[u.to(DEV) for u in utt]).numel() <= 4
