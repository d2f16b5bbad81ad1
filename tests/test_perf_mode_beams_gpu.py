"""Perf mode (the 16-bit K/V cache of the decode step) below 256 (row, head) pairs and over a shared prompt:
vh_attn_decode_kv16_split, vh_attn_decode_shared_kv16, the decoder forms built on them and generate(perf_mode=...).
The kernels' arithmetic is fp32 on the rounded cache, so against fp32 / double attention over the SAME rounded K/V they may
differ by summation order only (atol 3e-5, the bound of test_attn_decode_kv16_matches_fp32_math_on_the_rounded_cache); the
decoder forms hold the same rounded cache under perf_mode='kv', so their logits agree to the project's summation-order
bound (atol 2e-4, rtol 1e-4) and their greedy tokens are equal."""
import pytest
import torch
import torch.nn.functional as F

from tests.golden import cases as C
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ATOL, RTOL = 2e-4, 1e-4


@pytest.fixture(scope='module')
def K():
    from valle2_amd import kernels
    return kernels


def g(seed):
    return torch.Generator().manual_seed(seed)


def build(name, kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class(name)(C.cfg_of(kw))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


EDGES = [1, 2, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1087, 2048, 2943]


def _length_sets(B, S_max, n_split):
    """Lengths at the chunk edges of the kv16 test (rotated by the split count so that small batches see different edges),
    the last row full, plus one row with a SINGLE key — most of its splits are empty."""
    lens = [min(S_max, EDGES[(i + n_split) % len(EDGES)] + i // len(EDGES)) for i in range(B)]
    lens[-1] = S_max
    if B > 1:
        lens[0] = 1
    sets = [lens] if B > 1 else [lens, [1]]
    # small batches: every split count also sees EVERY edge that fits (31 / 32 / 33, 63 / 64 / 65, ...), B rows at a time
    if B < len(EDGES):
        fit = [e for e in EDGES if e <= S_max]
        sets += [(fit[i:i + B] + fit[:B])[:B] for i in range(0, len(fit), B)]
    return sets


@pytest.mark.parametrize('S_max', [64, 320, 2944])
@pytest.mark.parametrize('n_split', [2, 5, 8, 16])
@pytest.mark.parametrize('B,h', [(4, 8), (1, 8), (8, 16), (3, 2)])
def test_attn_decode_kv16_split_matches_fp32_math_on_the_rounded_cache(K, B, h, n_split, S_max):
    H16 = K.H16
    d = 64 * h
    gen = g(1000 + 7 * S_max + 13 * n_split + B)
    q = torch.randn(B, d, generator=gen)
    k0 = torch.randn(B, h, S_max, 64, generator=gen).to(H16)
    v0 = torch.randn(B, h, S_max, 64, generator=gen).to(H16)
    for lens_l in _length_sets(B, S_max, n_split):
        lens = torch.tensor(lens_l, dtype=torch.int32)
        k, v = k0.clone(), v0.clone()
        ref = torch.empty(B, d)
        for b in range(B):
            n = int(lens[b])
            ref[b] = F.scaled_dot_product_attention(q[b].view(1, h, 1, 64), k[b:b + 1, :, :n].float(),
                                                    v[b:b + 1, :, :n].float()).reshape(d)
            k[b, :, n:] = float('nan')
            v[b, :, n:] = float('inf')
        qd, kd, vd, cl = q.to(DEV), k.to(DEV), v.to(DEV), (lens - 1).to(DEV)
        ws = K.attn_decode_ws(B, h, n_split, DEV)
        out = torch.full((B, d), float('nan'), device=DEV)
        K.attn_decode_kv16(qd, kd, vd, out, cl, 1, n_split=n_split, partial=ws)
        assert bool(torch.isfinite(out).all()), 'garbage beyond a row\'s length leaked into the attention output'
        err = float((out.cpu() - ref).abs().max())
        print(f'kv16 split B={B} h={h} n_split={n_split} S_max={S_max} lens={lens_l[:4]}..: max |err| = {err:.2e}')
        torch.testing.assert_close(out.cpu(), ref, atol=3e-5, rtol=0)
        out2 = torch.full((B, d), float('nan'), device=DEV)
        K.attn_decode_kv16(qd, kd, vd, out2, cl, 1, n_split=n_split, partial=torch.full_like(ws, float('nan')))
        assert torch.equal(out, out2), 'two runs of the key-split form differ'


@pytest.mark.parametrize('B,h,S_max', [(32, 8, 1120), (4, 8, 320), (3, 2, 64)])
def test_attn_decode_kv16_split_of_one_is_vh_attn_decode_kv16_bit_for_bit(K, B, h, S_max):
    H16 = K.H16
    d = 64 * h
    gen = g(2000 + S_max)
    q = torch.randn(B, d, generator=gen).to(DEV)
    k = torch.randn(B, h, S_max, 64, generator=gen).to(H16).to(DEV)
    v = torch.randn(B, h, S_max, 64, generator=gen).to(H16).to(DEV)
    lens = torch.tensor([min(S_max, EDGES[i % len(EDGES)]) for i in range(B)], dtype=torch.int32)
    a = torch.empty(B, d, device=DEV)
    b = torch.empty(B, d, device=DEV)
    K.attn_decode_kv16(q, k, v, a, (lens - 1).to(DEV), 1)                                         # vh_attn_decode_kv16
    K.attn_decode_kv16(q, k, v, b, (lens - 1).to(DEV), 1, n_split=1, partial=torch.empty(16, device=DEV))   # ..._split(n_split=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize('B,h,prefix_len,n_split', [(32, 8, 1024, 1), (4, 8, 1024, 8), (8, 16, 626, 2), (40, 2, 31, 1),
                                                    (64, 4, 1, 1), (3, 2, 2651, 3), (33, 8, 100, 1), (8, 16, 2907, 2)])
def test_attn_decode_shared_kv16(K, B, h, prefix_len, n_split):
    """The cases of test_attn_decode_shared_prompt over caches rounded to the 16-bit format, against double-precision attention
    over the concatenated ROUNDED keys: ragged suffixes (one beam with a single own row), NaN / Inf in the prefix cache beyond
    prefix_len and in the suffix caches beyond every beam's length, beams beyond 32, key splits of the suffix."""
    H16 = K.H16
    d = 64 * h
    S_suf = 96
    prefix_S = (prefix_len + 31) // 32 * 32 + 32
    gen = g(500 + prefix_len + B)
    q = torch.randn(B, d, generator=gen)
    kp = torch.randn(1, h, prefix_S, 64, generator=gen).to(H16)
    vp = torch.randn(1, h, prefix_S, 64, generator=gen).to(H16)
    ks = torch.randn(B, h, S_suf, 64, generator=gen).to(H16)
    vs = torch.randn(B, h, S_suf, 64, generator=gen).to(H16)
    slen = torch.tensor([(7 * i) % 90 for i in range(B)], dtype=torch.int32)          # rows in the suffix BEFORE the new one
    ref = torch.empty(B, d)
    for b in range(B):
        n = int(slen[b]) + 1
        kk = torch.cat([kp[0, :, :prefix_len], ks[b, :, :n]], dim=1).double()
        vv = torch.cat([vp[0, :, :prefix_len], vs[b, :, :n]], dim=1).double()
        s = (q[b].double().view(h, 1, 64) @ kk.transpose(-1, -2)) / 8.0
        ref[b] = (torch.softmax(s, dim=-1) @ vv).reshape(d).float()
        ks[b, :, n:] = float('nan')
        vs[b, :, n:] = float('inf')
    kp[:, :, prefix_len:] = float('nan')
    vp[:, :, prefix_len:] = float('inf')
    args = (q.to(DEV), kp.to(DEV), vp.to(DEV), prefix_len, ks.to(DEV), vs.to(DEV))
    out = torch.full((B, d), float('nan'), device=DEV)
    K.attn_decode_shared_kv16(*args, out, slen.to(DEV), 1, n_split=n_split)
    assert bool(torch.isfinite(out).all()), 'garbage beyond a length leaked into the attention output'
    err = float((out.cpu() - ref).abs().max())
    print(f'shared kv16 B={B} h={h} prefix={prefix_len} n_split={n_split}: max |err| = {err:.2e}')
    torch.testing.assert_close(out.cpu(), ref, atol=3e-5, rtol=0)
    out2 = torch.empty_like(out)
    K.attn_decode_shared_kv16(*args, out2, slen.to(DEV), 1, n_split=n_split)
    assert torch.equal(out, out2)


# ---- the decoder: three forms over the SAME rounded cache ----------------------------------------------------------
KEEP = [0, 16, 32, 47]


@pytest.fixture(scope='module')
def mid():
    kw, sd, utt = C.ar_generate_inputs('mid')
    m = build('ValleAR', kw, sd)
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    first = utt[1][:, 0].to(DEV)
    new = C.cfg_of(kw).max_audio_len
    assert new == 48
    # (1) the yardstick: 32 replicated rows, one (row, head) per workgroup, the cache narrowed from the fp32 prompt pass
    free = m.generate_batch([text] * 32, [first] * 32, perf_mode='kv')
    st = m.last_generate_stats
    assert st['kv_bf16'] and st['n_split'] == 1 and not st['shared_prompt'] and not st['prefill_bf16']
    pl = st['prompt_lens'][0]
    tokens = free[0, pl:pl + new].clone()
    assert tokens.numel() == new and bool((free[:, pl:pl + new] == tokens).all())
    m.generate_batch([text] * 32, [first] * 32, perf_mode='kv', forced=tokens, keep_logits=KEEP)
    logits = {t: m.last_generate_stats['logits'][t][0].clone() for t in KEEP}
    return dict(m=m, text=text, first=first, new=new, pl=pl, tokens=tokens, logits=logits, kw=kw, sd=sd, utt=utt)


def test_yardstick_margins_are_ten_times_the_logit_tolerance(mid):
    for t in KEEP:
        top2 = torch.topk(mid['logits'][t], 2).values
        margin = float(top2[0] - top2[1])
        print(f'yardstick step {t}: top-2 margin {margin:.3e}')
        assert margin >= 10 * ATOL, (t, margin)


@pytest.mark.parametrize('form', ['split', 'shared'])
def test_decoder_forms_agree_with_the_one_workgroup_form(mid, form):
    m, text, first, new, pl = mid['m'], mid['text'], mid['first'], mid['new'], mid['pl']
    kw = dict(perf_mode='kv', shared_prompt=form == 'shared')

    def check_stats(st):
        assert st['kv_bf16'] and not st['prefill_bf16']
        if form == 'split':
            assert st['n_split'] > 1 and not st['shared_prompt'], st['n_split']
        else:
            assert st['shared_prompt'] and 1 <= st['n_split'] <= 16
    # teacher-forced logits against run (1)
    m.generate_batch([text] * 4, [first] * 4, forced=mid['tokens'], keep_logits=KEEP, **kw)
    st = m.last_generate_stats
    check_stats(st)
    for t in KEEP:
        got = st['logits'][t]
        err = float((got - mid['logits'][t][None]).abs().max())
        print(f'{form} form, step {t}: max |logit - yardstick| = {err:.2e}')
        torch.testing.assert_close(got, mid['logits'][t][None].expand_as(got), atol=ATOL, rtol=RTOL)
    # free-running greedy tokens: all 48, graph and eager
    for use_graph in (True, False):
        out = m.generate_batch([text] * 4, [first] * 4, use_graph=use_graph, **kw)
        check_stats(m.last_generate_stats)
        assert out.shape[1] == pl + new
        assert bool((out[:, pl:] == mid['tokens'][None]).all()), (form, use_graph, out[:, pl:].tolist(), mid['tokens'].tolist())


@pytest.mark.parametrize('form', ['split', 'shared', 'shared_kv'])
def test_second_call_reuses_the_16_bit_slot(mid, form):
    m, text, first = mid['m'], mid['text'], mid['first']
    m.release_decoders()
    kw = dict(perf_mode='kv' if form == 'shared_kv' else True, shared_prompt=form != 'split')
    a = m.generate_batch([text] * 4, [first] * 4, **kw)
    st = m.last_generate_stats
    assert not st['decoder_reused'] and st['kv_bf16'] and st['shared_prompt'] == (form != 'split')
    assert st['prefill_bf16'] == (form != 'shared_kv')
    assert form != 'split' or st['n_split'] > 1
    b = m.generate_batch([text] * 4, [first] * 4, **kw)
    st = m.last_generate_stats
    assert st['decoder_reused'] and st['slot_uses'] == 2 and st['kv_bf16']
    assert torch.equal(a, b)
    if form == 'shared_kv':
        assert bool((a[:, mid['pl']:] == mid['tokens'][None]).all())
    # an fp32 shared-prompt call of the same shape must not land on the 16-bit slot
    if form != 'split':
        m.generate_batch([text] * 4, [first] * 4, shared_prompt=True)
        st = m.last_generate_stats
        assert not st['kv_bf16'] and not st['decoder_reused']


def test_generate_takes_perf_mode(mid):
    gold = load_golden('ar_generate_mid')
    kw = dict(mid['kw'], num_beams=4)
    m = build('ValleAR', kw, mid['sd'])
    utt = [u.to(DEV) for u in mid['utt']]
    eos = m.eos_token
    want = mid['tokens'][mid['tokens'] != eos]
    out = m.generate(*utt, perf_mode='kv')
    st = m.last_generate_stats
    assert st['kv_bf16'] and st['shared_prompt'] and not st['prefill_bf16'] and 1 <= st['n_split'] <= 16
    assert torch.equal(out, want), (out.tolist(), want.tolist())
    out = m.generate(*utt, perf_mode=True)
    st = m.last_generate_stats
    assert st['kv_bf16'] and st['shared_prompt'] and st['prefill_bf16']
    assert out.dim() == 1 and out.dtype == torch.int64 and 0 < out.numel() <= 48
    agree = float((out[:min(len(out), len(want))] == want[:min(len(out), len(want))]).float().mean())
    print(f'generate(perf_mode=True): {agree:.3f} of the greedy tokens equal the perf_mode="kv" run')
    # off: exactly today's generate()
    out = m.generate(*utt)
    st = m.last_generate_stats
    assert not st['kv_bf16'] and not st['prefill_bf16'] and st['shared_prompt']
    assert torch.equal(out.cpu(), gold['tokens'])
    out2 = m.generate(*utt, perf_mode=False)
    assert torch.equal(out, out2) and not m.last_generate_stats['kv_bf16']


def test_full_size_eight_rows_within_the_perf_mode_tolerance():
    """24L/1024d/16 heads against the REAL reference's teacher-forced pass (ar_forced_big.npz): 8 rows are 128 (row, head)
    pairs, so the independent form reads the 16-bit cache with two key splits; the shared form reads the prompt once.  Bound:
    the one of test_perf_mode_teacher_forced_logits_within_tolerance (5e-2; 1.5e-2 in the default fp16 build)."""
    from valle2_amd._lib import h16_dtype
    tol = 1.5e-2 if h16_dtype() == torch.float16 else 5e-2
    gold = load_golden('ar_forced_big')
    kw, sd, utt, forced = C.ar_forced_big_inputs()
    m = build('ValleAR', kw, sd)
    steps = [p - 225 for p in C.FORCED_BIG_POS]
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    first = utt[1][:, 0].to(DEV)
    for shared in (False, True):
        m.generate_batch([text] * 8, [first] * 8, max_new=C.FORCED_BIG_NEW, forced=forced, keep_logits=steps, perf_mode=True,
                         shared_prompt=shared)
        st = m.last_generate_stats
        assert st['kv_bf16'] and st['prefill_bf16'] and st['shared_prompt'] == shared and st['s0'] == 626
        assert shared or st['n_split'] == 2
        got = torch.stack([st['logits'][t] for t in steps]).cpu()
        err = float((got - gold['logits'][:, None]).abs().max())
        print(f'config4 long context, perf mode, 8 rows, shared_prompt={shared} (n_split={st["n_split"]}): '
              f'max |logit error| = {err:.2e}')
        assert err < tol, (shared, err)


def test_sampling_beams_under_perf_mode_and_shared_prompt(mid):
    kw = dict(mid['kw'], num_beams=4, top_k=50)
    m = build('ValleAR', kw, mid['sd'])
    text, first = mid['text'], mid['first']
    outs, lps = [], []
    for use_graph in (True, False):
        torch.manual_seed(1234)
        outs.append(m.generate_batch([text] * 4, [first] * 4, perf_mode=True, shared_prompt=True, use_graph=use_graph))
        st = m.last_generate_stats
        assert st['kv_bf16'] and st['shared_prompt'] and st['prefill_bf16']
        lps.append(st['sum_logprobs'].cpu())
    assert torch.equal(outs[0], outs[1]), 'graph and eager runs drew different tokens under the same seed'
    torch.testing.assert_close(lps[0], lps[1], atol=1e-4, rtol=1e-5)
    gen = outs[0][:, mid['pl']:]
    assert len({tuple(r.tolist()) for r in gen}) == 4, 'the beams did not diverge'
    assert tuple(lps[0].shape) == (4,) and bool((lps[0] < 0).all()) and len(set(lps[0].tolist())) == 4


def test_refusals_that_remain(mid):
    from valle2_amd import engine, kernels
    from valle2_amd._lib import VhError
    m, text, first = mid['m'], mid['text'], mid['first']
    for perf in (True, 'kv'):
        with pytest.raises(ValueError, match='shared_prompt'):
            m.generate_batch([text, text[:-1]], [first, first], perf_mode=perf, shared_prompt=True)
    cfg = m.config
    i32 = dict(device=DEV, dtype=torch.int32)
    codes = torch.zeros(4, 40, device=DEV, dtype=torch.int64)
    for pdt, cdt in ((torch.float32, kernels.H16), (kernels.H16, torch.float32)):
        cache = engine.KVCache(cfg.num_layers, 4, cfg.n_heads, 32, DEV, dtype=cdt)
        prefix = engine.KVCache(cfg.num_layers, 1, cfg.n_heads, 64, DEV, dtype=pdt)
        with pytest.raises(VhError, match='same dtype'):
            engine.ArDecoder(m, 4, 32, codes, cache, torch.zeros(4, **i32), torch.ones(4, **i32), torch.ones(4, **i32),
                             prefix=prefix, prefix_len=50)
