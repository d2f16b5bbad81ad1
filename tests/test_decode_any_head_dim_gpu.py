"""KV-cached generation at head widths other than 64 (valle/models/modules.py:112 lets head_dim = d_model / n_heads be any
divisor; the reference decodes every width with use_kv_cache=True, modules.py:151-167): the kernels of the decode step at a
runtime width (vh_attn_decode_hd, vh_linear_qkv[_folded]_hd, vh_kv_store) against torch, and ValleAR.generate_batch /
generate on the cached decoder against the recompute path, the CPU oracle and the real reference's tokens
(tests/golden/head_dim_decode.npz)."""
import ctypes

import pytest
import torch

from tests.golden import cases as C
from tests.golden.gen_golden_head_dim_decode import HD_DECODE, head_dim_decode_inputs
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _attn_ref(q, k, v, lens, scale):
    """float64 softmax attention of one query per (row, head) over keys 0 .. lens[b] - 1."""
    B, h, _, hd = k.shape
    out = torch.empty(B, h * hd, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        qb = q[b, : h * hd].double().view(h, 1, hd)
        s = (qb @ k[b, :, :n].double().transpose(1, 2)) * scale
        out[b] = (torch.softmax(s, -1) @ v[b, :, :n].double()).reshape(h * hd)
    return out


@pytest.mark.parametrize('hd', [16, 32, 48, 96, 128, 192, 256])
@pytest.mark.parametrize('n_split', [1, 2, 16])
def test_attn_decode_hd_matches_float64_softmax(hd, n_split):
    from valle2_amd import kernels
    g = torch.Generator().manual_seed(hd * 7 + n_split)
    B, h, S = 5, 3, 720
    lens = torch.tensor([1, 31, 257, 700, 97], dtype=torch.int32)
    k0 = torch.randn(B, h, S, hd, generator=g)
    v0 = torch.randn(B, h, S, hd, generator=g)
    for len_bias in (0, 1):
        k, v = k0.clone(), v0.clone()
        for b in range(B):                             # beyond each row's length: NaN (selected away, never multiplied)
            k[b, :, int(lens[b]) + len_bias:] = float('nan')
            v[b, :, int(lens[b]) + len_bias:] = float('nan')
        q = torch.randn(B, h * hd + 8, generator=g)     # ldq > h * hd
        out = torch.full((B, h * hd), float('nan'), device=DEV)
        kernels.attn_decode_hd(q.to(DEV), k.to(DEV), v.to(DEV), out, lens.to(DEV), len_bias, n_split=n_split)
        ref = _attn_ref(q, k, v, lens + len_bias, hd ** -0.5)
        torch.testing.assert_close(out.cpu().double(), ref, atol=2e-5, rtol=0, msg=lambda m: f'len_bias={len_bias}: {m}')


def test_attn_decode_hd_at_width_64_equals_attn_decode():
    from valle2_amd import _lib, kernels
    from valle2_amd._lib import check, ptr, stream
    g = torch.Generator().manual_seed(64)
    B, h, S = 6, 4, 512
    lens = torch.tensor([1, 33, 100, 480, 511, 64], dtype=torch.int32, device=DEV)
    k = torch.randn(B, h, S, 64, generator=g).to(DEV)
    v = torch.randn(B, h, S, 64, generator=g).to(DEV)
    q = torch.randn(B, h * 64, generator=g).to(DEV)
    for n_split in (1, 4):
        a = torch.empty(B, h * 64, device=DEV)
        kernels.attn_decode(q, k, v, a, lens, 1, n_split=n_split, partial=kernels.attn_decode_ws(B, h, n_split, DEV))
        b = torch.empty(B, h * 64, device=DEV)
        ws = kernels.attn_decode_hd_ws(B, h, 64, n_split, DEV)
        check(_lib.lib().vh_attn_decode_hd(ptr(q), q.stride(0), ptr(k), ptr(v), ptr(b), b.stride(0), ptr(lens), 1, B, h, 64,
                                           S, 0.125, n_split, ptr(ws), ws.numel() * 4 if ws is not None else 0, stream()),
              'vh_attn_decode_hd')
        torch.testing.assert_close(b, a, atol=1e-6, rtol=0)


@pytest.mark.parametrize('hd', [8, 260, 50])
def test_attn_decode_hd_refuses_unserved_widths(hd):
    from valle2_amd import _lib, kernels
    k = torch.zeros(1, 1, 4, hd, device=DEV)
    with pytest.raises(_lib.VhError, match=f'head_dim={hd}'):
        kernels.attn_decode_hd(torch.zeros(1, hd, device=DEV), k, k.clone(), torch.zeros(1, hd, device=DEV),
                               torch.ones(1, dtype=torch.int32, device=DEV), 0)


@pytest.mark.parametrize('d,h,folded', [(256, 2, True), (128, 4, True), (192, 4, False), (512, 2, True), (96, 6, False)])
def test_linear_qkv_hd_appends_k_v_at_cache_len_only(d, h, folded):
    from valle2_amd import kernels
    hd = d // h
    g = torch.Generator().manual_seed(d + h)
    B, S = 19, 40
    x = torch.randn(B, d, generator=g).to(DEV)
    w = (0.05 * torch.randn(3 * d, d, generator=g)).to(DEV)
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
    cache_len = torch.randint(0, S, (B,), generator=g, dtype=torch.int32)
    kc = torch.full((B, h, S, hd), 7.25, device=DEV)
    vc = torch.full((B, h, S, hd), -3.5, device=DEV)
    q = torch.empty(B, d, device=DEV)
    if folded:
        kernels.linear_qkv_hd(x, None, q, kc, vc, h, cache_len.to(DEV), folded=kernels.ln_fold(w, gamma, beta))
    else:
        kernels.linear_qkv_hd(x, w, q, kc, vc, h, cache_len.to(DEV), ln=(gamma, beta, None, None, 1e-5))
    y = torch.nn.functional.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5) @ w.double().T
    torch.testing.assert_close(q.double(), y[:, :d], atol=2e-5, rtol=1e-5)
    ek, ev = torch.full_like(kc, 7.25), torch.full_like(vc, -3.5)
    for b in range(B):
        ek[b, :, int(cache_len[b])] = y[b, d:2 * d].view(h, hd).float()
        ev[b, :, int(cache_len[b])] = y[b, 2 * d:].view(h, hd).float()
    torch.testing.assert_close(kc, ek, atol=2e-5, rtol=1e-5)      # the sentinel everywhere else: exact
    torch.testing.assert_close(vc, ev, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize('hd', [16, 48, 128, 256])
def test_kv_store_equals_torch_view_copy(hd):
    from valle2_amd import kernels
    g = torch.Generator().manual_seed(hd)
    B, T, h, S = 3, 37, 2, 64
    d = h * hd
    qkv = torch.randn(B * T, 3 * d, generator=g).to(DEV)
    kc = torch.full((B, h, S, hd), 1.5, device=DEV)
    vc = torch.full((B, h, S, hd), 1.5, device=DEV)
    kernels.kv_store(qkv, kc, vc, B, T)
    ek, ev = torch.full_like(kc, 1.5), torch.full_like(vc, 1.5)
    ek[:, :, :T] = qkv.view(B, T, 3, h, hd)[:, :, 1].permute(0, 2, 1, 3)
    ev[:, :, :T] = qkv.view(B, T, 3, h, hd)[:, :, 2].permute(0, 2, 1, 3)
    assert torch.equal(kc, ek) and torch.equal(vc, ev)


def _model(kw, seed):
    from valle2_amd import get_model_class, synth
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=seed, rich=True), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, cfg


def _recompute_twin(kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(dict(kw, use_kv_cache=False)))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


WIDTH_MODELS = {32: dict(d_model=128, n_heads=4), 48: dict(d_model=192, n_heads=4), 128: dict(d_model=256, n_heads=2),
                256: dict(d_model=512, n_heads=2)}


@pytest.mark.parametrize('hd', sorted(WIDTH_MODELS))
def test_generate_batch_cached_equals_recompute(hd):
    """Greedy tokens of the cached decoder (graph and eager; equal and ragged rows) = the recompute path's, except at a step
    whose top-2 margin (oracle, row 0 of the equal-row case) is below 1e-4; a second call of the same shape reuses its slot."""
    from oracle import valle_oracle as O
    from valle2_amd import synth
    kw = dict(WIDTH_MODELS[hd], dim_feedforward=2 * WIDTH_MODELS[hd]['d_model'], num_layers=2, dropout=0.0, norm='LayerNorm',
              num_beams=3, top_k=1, max_audio_len=40)
    m, sd, cfg = _model(kw, seed=90 + hd)
    assert cfg.d_model // cfg.n_heads == hd
    rc = _recompute_twin(kw, sd)
    utts = [synth.synth_utterance(cfg, 6 + 3 * i, 5 + i, 20 + 17 * i, seed=500 + i) for i in range(3)]
    texts = [torch.cat([u[0], u[2]]).to(DEV) for u in utts]
    firsts = [u[1][:, 0].to(DEV) for u in utts]
    trace = {}
    O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *utts[0], trace=trace)
    near_tie = [t for t, mg in enumerate(trace['margin']) if mg < 1e-4]
    for rows in ([texts[0]] * 3, texts):                      # independent equal rows, then ragged rows
        fr = [firsts[0]] * 3 if rows[1] is rows[0] else firsts
        want = rc.generate_batch(rows, fr, max_new=40)
        assert rc.last_generate_stats['kv_cache'] is False
        for use_graph in (True, False):
            got = m.generate_batch(rows, fr, max_new=40, use_graph=use_graph)
            st = m.last_generate_stats
            assert st['kv_cache'] is True and not st['shared_prompt'] and not st['kv_bf16']
            if got.shape != want.shape or not torch.equal(got, want):
                n = min(got.shape[1], want.shape[1])
                diff = (got[:, :n] != want[:, :n]).any(0).nonzero()
                first = int(diff[0]) - min(st['prompt_lens']) if diff.numel() else n
                assert rows[1] is rows[0] and first in near_tie, (hd, use_graph, got.cpu(), want.cpu())
        m.generate_batch(rows, fr, max_new=40)
        assert m.last_generate_stats['decoder_reused'] is True


@pytest.mark.parametrize('hd', [48, 128])
def test_teacher_forced_logits_match_the_oracle(hd):
    from oracle import valle_oracle as O
    from valle2_amd import synth
    kw = dict(WIDTH_MODELS[hd], dim_feedforward=2 * WIDTH_MODELS[hd]['d_model'], num_layers=2, dropout=0.0, norm='LayerNorm',
              num_beams=1, top_k=1, max_audio_len=48)
    m, sd, cfg = _model(kw, seed=7 + hd)
    utt = synth.synth_utterance(cfg, 10, 8, 45, seed=41)
    trace = {}
    O.ar_generate(sd, cfg, *utt, trace=trace)
    n = len(trace['logits'])
    assert n == 48
    forced = torch.stack([t.reshape(-1)[0] for t in trace['tokens']])
    steps = [0, 1, 31, n - 1]
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    m.generate_batch([text] * 2, [utt[1][:, 0].to(DEV)] * 2, max_new=n, forced=forced, keep_logits=steps)
    st = m.last_generate_stats
    assert st['kv_cache'] is True
    for t in steps:
        torch.testing.assert_close(st['logits'][t].cpu(), trace['logits'][t][:1].expand(2, -1), atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize('which', sorted(HD_DECODE))
def test_generate_matches_the_real_reference(which):
    gold = load_golden('head_dim_decode')
    kw, sd, utt = head_dim_decode_inputs(which)
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(kw))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    out = m.generate(*[u.to(DEV) for u in utt]).cpu()
    st = m.last_generate_stats
    assert st['kv_cache'] is True and not st['shared_prompt']
    if which == 'w128':
        assert st['n_split'] > 1                              # 4 beams x 2 heads: key splits + the combine launch
    ref = gold[f'tokens_{which}']
    n = min(len(out), len(ref))
    bad = (out[:n] != ref[:n]).nonzero()
    assert len(out) == len(ref) and (bad.numel() == 0 or float(gold[f'margin_{which}'][int(bad[0])]) < 1e-4), (out, ref)


def test_sampling_graph_equals_eager_at_width_128():
    from valle2_amd import synth
    kw = dict(d_model=256, n_heads=2, dim_feedforward=512, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=4,
              top_k=50, max_audio_len=32)
    m, _, cfg = _model(kw, seed=12)
    utt = synth.synth_utterance(cfg, 8, 8, 30, seed=3)
    rows = [torch.cat([utt[0], utt[2]]).to(DEV)] * 4
    firsts = [utt[1][:, 0].to(DEV)] * 4
    outs = []
    for use_graph in (True, False):
        torch.manual_seed(1234)
        outs.append(m.generate_batch(rows, firsts, max_new=32, use_graph=use_graph).cpu())
        assert m.last_generate_stats['kv_cache'] is True
    assert torch.equal(outs[0], outs[1])


def test_width_128_refusals():
    from valle2_amd import _lib, engine, synth
    kw = dict(d_model=256, n_heads=2, dim_feedforward=512, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
              top_k=1, max_audio_len=8)
    m, _, cfg = _model(kw, seed=5)
    utt = synth.synth_utterance(cfg, 4, 4, 9, seed=2)
    rows, firsts = [torch.cat([utt[0], utt[2]]).to(DEV)] * 2, [utt[1][:, 0].to(DEV)] * 2
    with pytest.raises(ValueError, match='head width 128'):
        m.generate_batch(rows, firsts, shared_prompt=True)
    with pytest.raises(ValueError, match='head width 128'):
        m.generate_batch(rows, firsts, perf_mode=True)
    # the C check behind them: a descriptor ArDecoder built, with kv_bf16 / prefix_len set
    B, S = 2, 32
    cache = engine.KVCache(cfg.num_layers, B, cfg.n_heads, S, DEV, head_dim=128)
    codes = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    dec = engine.ArDecoder(m, B, S, codes, cache, torch.zeros(B, **i32), torch.ones(B, **i32), torch.ones(B, **i32),
                           use_graph=False)
    L = _lib.lib()
    try:
        for field, value, what in (('kv_bf16', 1, 'bf16'), ('prefix_len', 8, 'shared prompt')):
            desc = type(dec._desc).from_buffer_copy(dec._desc)
            setattr(desc, field, value)
            if field == 'prefix_len':
                desc.prefix_S = 8
            assert not L.vh_ar_decoder_create(ctypes.byref(desc))
            msg = L.vh_last_error().decode()
            assert what in msg and '128' in msg, msg
    finally:
        dec.close()
