"""KV-cached AR decoding at d_model above 1024 (head width 64): the folded-LayerNorm skinny GEMMs at 1024 < K <= 4096
(vh_linear_folded / vh_linear_qkv_folded: 16 waves, statistics from the operand fragments) against float64 torch, and
ValleAR.generate_batch / generate on the cached decoder at d_model 1152 (LayerNorm + plain GEMMs as separate launches),
1536 and 2048 (wide folded GEMMs) against the recompute path, the CPU oracle and the real reference's tokens
(tests/golden/wide_d_model.npz).

Tolerance of the kernel test: none is fixed in advance.  On the same inputs the test measures the largest error against
float64 of the UNFUSED route (kernels.layernorm + kernels.linear) and allows the folded kernel twice that: its summation
order differs and its epilogue cancels (mean - shift)·c1.  Figures measured on an MI355X are in profiles/r7_wide_d_model.log."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.golden import cases as C
from tests.golden.gen_golden_wide_d_model import WIDE, wide_d_model_inputs
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def g(seed):
    return torch.Generator().manual_seed(seed)


def _folded_case(K_, M, N, seed):
    a = 2.0 * torch.randn(M, K_, generator=g(seed)) + 0.5
    a[0] += 3.0                                            # a row whose mean exceeds its deviation
    a[M - 1] = 50.0 + torch.randn(K_, generator=g(seed + 1))   # mean 50, deviation 1
    w = 0.1 * torch.randn(N, K_, generator=g(seed + 2))
    gm, bt = 1 + 0.1 * torch.randn(K_, generator=g(seed + 3)), 0.1 * torch.randn(K_, generator=g(seed + 4))
    bias, res = torch.randn(N, generator=g(seed + 5)), torch.randn(M, N, generator=g(seed + 6))
    return a, w, gm, bt, bias, res


@pytest.mark.parametrize('act', [0, 1], ids=['none', 'gelu'])
@pytest.mark.parametrize('M', [1, 3, 16, 17, 32, 64])
@pytest.mark.parametrize('K_', [1280, 1536, 1792, 2048, 2560, 3072, 3584, 4096])
def test_linear_folded_wide_k_within_twice_the_unfused_error(K_, M, act):
    from valle2_amd import kernels as K
    N = 544                                                # 34 column blocks: not a multiple of the 256 CUs or of 128
    a, w, gm, bt, bias, res = _folded_case(K_, M, N, seed=K_ + M)
    ref = F.linear(F.layer_norm(a.double(), (K_,), gm.double(), bt.double(), 1e-5), w.double(), bias.double())
    ref = (F.gelu(ref) if act else ref) + res.double()
    ad, wd, gd, bd, biasd, resd = (t.to(DEV) for t in (a, w, gm, bt, bias, res))
    unfused = K.linear(K.layernorm(ad, gd, bd), wd, biasd, resd, act=act)
    err_unfused = float((unfused.cpu().double() - ref).abs().max())
    folded = K.ln_fold(wd, gd, bd, biasd)
    out = K.linear_folded(ad, folded, residual=resd, act=act)
    err_folded = float((out.cpu().double() - ref).abs().max())
    print(f'linear_folded K={K_} M={M} act={act}: max|err| folded {err_folded:.3e} unfused {err_unfused:.3e} '
          f'ratio {err_folded / err_unfused:.2f}')
    assert err_unfused < 1e-4                              # the yardstick itself is sane
    assert err_folded <= 2 * err_unfused, (K_, M, act, err_folded, err_unfused)


@pytest.mark.parametrize('K_', [1280, 2048, 3072, 4096])
def test_linear_folded_wide_k_integer_exact_in_any_order(K_):
    """Small-integer weights on rows of +-1 (mean 0, variance 1 exactly): every sum of the kernel — the products on
    x - shift, the fragment statistics, the wave and pass partials — is exact, so the result cannot depend on which wave or
    pass meets which k: a permutation of the k axis and every row grouping give the same bits."""
    from valle2_amd import kernels as K
    M, N = 40, 96
    gen = g(K_)
    x = torch.ones(M, K_)
    x[:, ::2] = -1
    x = x[:, torch.randperm(K_, generator=gen)]
    w = torch.randint(-2, 3, (N, K_), generator=gen).float()
    b = torch.randint(-2, 3, (N,), generator=gen).float()
    ones, zeros = torch.ones(K_, device=DEV), torch.zeros(K_, device=DEV)
    out = K.linear_folded(x.to(DEV), K.ln_fold(w.to(DEV), ones, zeros, b.to(DEV)))
    rs = 1.0 / (1.0 + 1e-5) ** 0.5                         # rstd of a unit-variance row
    torch.testing.assert_close(out.cpu(), (x @ w.T) * rs + b, atol=0, rtol=1e-6)
    perm = torch.randperm(K_, generator=gen)
    out_p = K.linear_folded(x[:, perm].contiguous().to(DEV), K.ln_fold(w[:, perm].contiguous().to(DEV), ones, zeros, b.to(DEV)))
    assert torch.equal(out_p, out)
    for rows in (1, 16, 17):                               # one row tile / 8-row groups / 16-row groups: the same bits per row
        part = K.linear_folded(x[:rows].to(DEV), K.ln_fold(w.to(DEV), ones, zeros, b.to(DEV)))
        assert torch.equal(part, out[:rows])


@pytest.mark.parametrize('d', [1536, 2048])
@pytest.mark.parametrize('B', [5, 19, 40])
def test_linear_qkv_folded_wide_appends_k_v_at_cache_len_only(d, B):
    from valle2_amd import kernels as K
    h, S = d // 64, 24
    gen = g(d + B)
    x = (torch.randn(B, d, generator=gen) + 0.3).to(DEV)
    w = (0.05 * torch.randn(3 * d, d, generator=gen)).to(DEV)
    gamma = (1 + 0.1 * torch.randn(d, generator=gen)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=gen)).to(DEV)
    cache_len = torch.randint(0, S, (B,), generator=gen, dtype=torch.int32)
    kc = torch.full((B, h, S, 64), 7.25, device=DEV)
    vc = torch.full((B, h, S, 64), -3.5, device=DEV)
    q = torch.empty(B, d, device=DEV)
    K.linear_qkv_folded(x, K.ln_fold(w, gamma, beta), q, kc, vc, B, 1, h, cache_len=cache_len.to(DEV))
    y = F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5) @ w.double().T
    torch.testing.assert_close(q.double(), y[:, :d], atol=2e-5, rtol=1e-5)
    ek, ev = torch.full_like(kc, 7.25), torch.full_like(vc, -3.5)
    for b in range(B):
        ek[b, :, int(cache_len[b])] = y[b, d:2 * d].view(h, 64).float()
        ev[b, :, int(cache_len[b])] = y[b, 2 * d:].view(h, 64).float()
    torch.testing.assert_close(kc, ek, atol=2e-5, rtol=1e-5)      # the sentinel everywhere else: exact
    torch.testing.assert_close(vc, ev, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize('K_', [1280, 2560, 4096])
def test_linear_folded_wide_k_row_with_an_outlier_head(K_):
    """The shift of the one-pass statistics is the mean of the row's first 32 elements.  Rows whose head is unrepresentative
    (30 +- 1, a constant 1000, -30 in front of a unit-normal rest) make dm = mean - shift large against the deviation of the
    rest — but the head is part of the row, so dm^2 <= K/32 var.  Bound, from that and fp32's 2^-24 (not from measurement):
      * var = sb/K - dm^2 with both operands <= (1 + K/32) var and about four roundings each way: the relative error of
        rstd is at most (1 + K/32) 2^-23, on outputs up to max |LN(x) W^T|;
      * acc - dm c1 with |dm| rstd <= sqrt(K/32): both sides up to sqrt(K/32) max|c1| in output units, a few roundings:
        sqrt(K/32) max|c1| 2^-22;
      * everything else is the unfused route's kind of error, measured on the same inputs and added.
    A constant row (variance 0 exactly) must come out finite and equal to c2."""
    from valle2_amd import kernels as K
    M, N = 6, 96
    gen = g(77 + K_)
    a = torch.randn(M, K_, generator=gen)
    a[0, :32] = 30.0 + torch.randn(32, generator=gen)
    a[1, :32] = 1000.0
    a[2, :32] = -30.0
    a[3] = 5.0                                             # a constant row: variance 0 exactly, output = c2
    w = 0.1 * torch.randn(N, K_, generator=gen)
    gm, bt = 1 + 0.1 * torch.randn(K_, generator=gen), 0.1 * torch.randn(K_, generator=gen)
    bias = torch.randn(N, generator=gen)
    y = F.linear(F.layer_norm(a.double(), (K_,), gm.double(), bt.double(), 1e-5), w.double())
    ref = y + bias.double()
    ad, wd, gd, bd, biasd = (t.to(DEV) for t in (a, w, gm, bt, bias))
    err_unfused = float((K.linear(K.layernorm(ad, gd, bd), wd, biasd).cpu().double() - ref).abs().max())
    out = K.linear_folded(ad, K.ln_fold(wd, gd, bd, biasd))
    err = (out.cpu().double() - ref).abs().max(1)[0]
    c1 = (w * gm).double().sum(1).abs().max()
    bound = (1 + K_ / 32) * 2.0 ** -23 * float(y.abs().max()) + (K_ / 32) ** 0.5 * float(c1) * 2.0 ** -22 + err_unfused
    print(f'outlier head K={K_}: per-row max|err| {[f"{float(e):.2e}" for e in err]} unfused {err_unfused:.2e} bound {bound:.2e}')
    assert bool(torch.isfinite(out).all())
    assert float(err.max()) <= bound, (K_, err, bound)


@pytest.mark.parametrize('K_', [1088, 2304, 3840, 4352])
def test_linear_folded_refuses_k_outside_the_wide_set(K_):
    from valle2_amd import kernels as K
    from valle2_amd._lib import VhError
    w = torch.randn(32, K_, device=DEV)
    folded = K.ln_fold(w, torch.ones(K_, device=DEV), torch.zeros(K_, device=DEV))
    with pytest.raises(VhError, match='folded LayerNorm'):
        K.linear_folded(torch.randn(4, K_, device=DEV), folded)


def _model(kw, seed):
    from valle2_amd import get_model_class, synth
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=seed, rich=True), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, cfg


def _build(kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(kw))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _kw(d, **over):
    return dict(dict(d_model=d, n_heads=d // 64, dim_feedforward=2 * d, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                     top_k=1, max_audio_len=24), **over)


MAX_NEW = 24


@pytest.mark.parametrize('d', [1152, 1536, 2048])
def test_generate_batch_cached_equals_recompute_graph_and_eager(d):
    """1, 5 and 40 rows, equal and ragged: the cached decoder's greedy tokens (graph and eager) are the recompute path's —
    except, for equal rows only, at a step whose top-2 margin in the oracle is below 1e-4 — and graph == eager bit for bit."""
    from oracle import valle_oracle as O
    from valle2_amd import synth
    kw = _kw(d)
    m, sd, cfg = _model(kw, seed=300 + d)
    rc = _build(dict(kw, use_kv_cache=False), sd)
    utts = [synth.synth_utterance(cfg, 6 + 2 * i, 4 + i, 14 + 5 * i, seed=800 + d + i) for i in range(5)]
    texts = [torch.cat([u[0], u[2]]).to(DEV) for u in utts]
    firsts = [u[1][:, 0].to(DEV) for u in utts]
    trace = {}
    O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *utts[0], trace=trace)
    near_tie = [t for t, mg in enumerate(trace['margin']) if mg < 1e-4]
    cases = [([texts[0]], [firsts[0]], True), ([texts[0]] * 5, [firsts[0]] * 5, True), (texts, firsts, False),
             ([texts[0]] * 40, [firsts[0]] * 40, True), ([texts[i % 5] for i in range(40)], [firsts[i % 5] for i in range(40)], False)]
    for rows, fr, equal in cases:
        want = rc.generate_batch(rows, fr, max_new=MAX_NEW)
        assert rc.last_generate_stats['kv_cache'] is False
        got = {}
        for use_graph in (True, False):
            got[use_graph] = out = m.generate_batch(rows, fr, max_new=MAX_NEW, use_graph=use_graph)
            st = m.last_generate_stats
            assert st['kv_cache'] is True and not st['shared_prompt'] and not st['kv_bf16']
            assert st['ln_folded'] is (d % 256 == 0 and len(rows) <= 16)   # (more rows: LayerNorm + plain GEMMs, measured faster)
            if out.shape != want.shape or not torch.equal(out, want):
                n = min(out.shape[1], want.shape[1])
                diff = (out[:, :n] != want[:, :n]).any(0).nonzero()
                first = int(diff[0]) - min(st['prompt_lens']) if diff.numel() else n
                assert equal and first in near_tie, (d, len(rows), use_graph, out.cpu(), want.cpu())
        assert torch.equal(got[True], got[False]), (d, len(rows))


@pytest.mark.parametrize('d', [1152, 1536, 2048])
def test_sampling_graph_equals_eager_under_one_seed(d):
    from valle2_amd import synth
    m, _, cfg = _model(_kw(d, top_k=50, num_beams=5), seed=400 + d)
    utt = synth.synth_utterance(cfg, 8, 6, 20, seed=3 + d)
    rows = [torch.cat([utt[0], utt[2]]).to(DEV)] * 5
    firsts = [utt[1][:, 0].to(DEV)] * 5
    outs = []
    for use_graph in (True, False):
        torch.manual_seed(1234)
        outs.append(m.generate_batch(rows, firsts, max_new=MAX_NEW, use_graph=use_graph).cpu())
        assert m.last_generate_stats['kv_cache'] is True
    assert torch.equal(outs[0], outs[1])
    assert len({tuple(r.tolist()) for r in outs[0]}) > 1, 'sampled rows must not be copies of each other'


@pytest.mark.parametrize('which', sorted(WIDE))
def test_teacher_forced_logits_match_the_oracle(which):
    from oracle import valle_oracle as O
    kw, sd, utt = wide_d_model_inputs(which)
    kw = dict(kw, num_beams=1)
    m = _build(kw, sd)
    trace = {}
    O.ar_generate(sd, C.cfg_of(kw), *utt, trace=trace)
    n = len(trace['logits'])
    assert n == kw['max_audio_len']
    forced = torch.stack([t.reshape(-1)[0] for t in trace['tokens']])
    steps = [0, 1, 31, n - 1]
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    m.generate_batch([text] * 2, [utt[1][:, 0].to(DEV)] * 2, max_new=n, forced=forced, keep_logits=steps)
    st = m.last_generate_stats
    assert st['kv_cache'] is True and st['ln_folded'] is (which == 'd1536')
    for t in steps:
        torch.testing.assert_close(st['logits'][t].cpu(), trace['logits'][t][:1].expand(2, -1), atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize('which', sorted(WIDE))
def test_generate_matches_the_real_reference_on_every_step(which):
    """The reference's tokens, all steps (every margin of the fixture is >= 10 x the logit tolerance), through generate()
    (shared prompt), through independent rows of generate_batch, and shared == independent."""
    gold = load_golden('wide_d_model')
    kw, sd, utt = wide_d_model_inputs(which)
    m = _build(kw, sd)
    out = m.generate(*[u.to(DEV) for u in utt]).cpu()
    st = m.last_generate_stats
    assert st['kv_cache'] is True and st['shared_prompt'] and st['ln_folded'] is (which == 'd1536')
    assert torch.equal(out, gold[f'tokens_{which}']), (out, gold[f'tokens_{which}'])
    text, first = torch.cat([utt[0], utt[2]]).to(DEV), utt[1][:, 0].to(DEV)
    n = kw['max_audio_len']
    shared = m.generate_batch([text] * 4, [first] * 4, max_new=n, shared_prompt=True)
    assert m.last_generate_stats['shared_prompt'] is True
    indep = m.generate_batch([text] * 4, [first] * 4, max_new=n)
    assert m.last_generate_stats['shared_prompt'] is False
    assert torch.equal(shared, indep)
    gen = indep[0, first.numel() + 1:].cpu()
    gen = gen[gen != m.eos_token]
    assert torch.equal(gen, gold[f'tokens_{which}'][: gen.numel()]) and gen.numel() == len(gold[f'tokens_{which}'])


def test_d_model_2304_decodes_on_the_unfolded_route():
    """An odd multiple of 256 above 2048: not a K of the folded kernels — LayerNorm + plain GEMMs, same tokens as recompute."""
    from valle2_amd import synth
    kw = _kw(2304, max_audio_len=16)
    m, sd, cfg = _model(kw, seed=2304)
    rc = _build(dict(kw, use_kv_cache=False), sd)
    utt = synth.synth_utterance(cfg, 7, 5, 18, seed=23)
    rows, fr = [torch.cat([utt[0], utt[2]]).to(DEV)] * 3, [utt[1][:, 0].to(DEV)] * 3
    want = rc.generate_batch(rows, fr, max_new=16)
    got = m.generate_batch(rows, fr, max_new=16)
    assert m.last_generate_stats['kv_cache'] is True and m.last_generate_stats['ln_folded'] is False
    assert torch.equal(got, want), (got.cpu(), want.cpu())


def test_generate_above_4096_raises_naming_the_limit():
    from valle2_amd import synth
    kw = dict(d_model=4160, n_heads=65, dim_feedforward=64, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=2, top_k=1,
              max_audio_len=4)
    m, _, cfg = _model(kw, seed=4160)
    utt = synth.synth_utterance(cfg, 4, 4, 6, seed=1)
    rows, fr = [torch.cat([utt[0], utt[2]]).to(DEV)] * 2, [utt[1][:, 0].to(DEV)] * 2
    with pytest.raises(ValueError, match='d_model 4160.*4096'):
        m.generate_batch(rows, fr)


def test_perf_mode_is_refused_above_1024_before_any_gpu_work():
    """perf_mode's decode append (bf16 K/V rows) has no wide folded form: generate_batch says so, naming d_model."""
    kw, sd, utt = wide_d_model_inputs('d1536')
    m = _build(kw, sd)
    text, first = torch.cat([utt[0], utt[2]]).to(DEV), utt[1][:, 0].to(DEV)
    for mode in (True, 'kv'):
        with pytest.raises(ValueError, match='d_model 1536'):
            m.generate_batch([text] * 2, [first] * 2, perf_mode=mode)
    assert not getattr(m, '_decode_slots', None)          # nothing was built


def test_decoder_refuses_d_model_above_4096_naming_the_limit():
    """The C check behind cached_decode_supported: a served descriptor with d_model = 4160 / 65 heads is refused."""
    from valle2_amd import _lib, engine, synth
    kw = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=2, top_k=1,
              max_audio_len=8)
    m, _, cfg = _model(kw, seed=5)
    B, S = 2, 32
    cache = engine.KVCache(cfg.num_layers, B, cfg.n_heads, S, DEV)
    codes = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    dec = engine.ArDecoder(m, B, S, codes, cache, torch.zeros(B, **i32), torch.ones(B, **i32), torch.ones(B, **i32),
                           use_graph=False)
    L = _lib.lib()
    try:
        desc = type(dec._desc).from_buffer_copy(dec._desc)
        desc.d_model, desc.n_heads = 4160, 65
        assert not L.vh_ar_decoder_create(ctypes.byref(desc))
        msg = L.vh_last_error().decode()
        assert '4096' in msg and '4160' in msg, msg
        desc.d_model, desc.n_heads = 4096, 64               # the widest served: the check passes (nothing is launched)
        desc.ffn_ws, desc.ffn_ws_bytes = None, 0            # (sized for d_model 128)
        h = L.vh_ar_decoder_create(ctypes.byref(desc))
        assert h, L.vh_last_error().decode()
        L.vh_ar_decoder_destroy(h)
    finally:
        dec.close()
