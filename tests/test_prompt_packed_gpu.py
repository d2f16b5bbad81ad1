"""The packed AR prompt pass on the device: `vh_kv_unpack` (bit-exact rows, nothing else written, the cuts), the packed
prefix-LM attention and `transformer_forward_packed_lm` against the padded forward of each segment alone and a float64 oracle,
and the generate entry points under `ValleAR.packed_prompt` against the oracle on each utterance alone.

Tolerances (none of them chosen from what the code gives):
  attention kernel vs `vh_attn_rows` on the segment alone   torch.equal (the same body over the same keys in the same order)
  attention kernel vs float64 softmax attention             atol 3e-5, rtol 2e-5  (tests/test_packed_rows_gpu.py, the fp32 kernel)
  composite (hidden rows, K/V rows) vs the padded forward   atol 2e-4, rtol 1e-4  (the project's summation-order bound: only the
  of the segment alone, and vs the float64 oracle           GEMM row count differs; tests/test_packed_rows_gpu.py's forward test)
  tokens                                                    `tokens_match` with the oracle's margins (tests/test_models_gpu.py)
"""
import functools

import pytest
import torch

from tests.golden import cases as C
from tests.test_models_gpu import build, tokens_match

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H, D, DFF, LAYERS = 2, 128, 512, 2
SENTINEL = -777.25
ATOL, RTOL = 2e-4, 1e-4
# (length, text length inside it, seed): lengths 1, 31, 32, 33, 64, 65, 129, 300 in shuffled order; the text lengths cover 0, 1,
# len - 1 and both sides of 32 and 64
SEGS_A = [(33, 32, 11), (300, 64, 12), (1, 0, 13), (65, 64, 14), (31, 1, 15), (129, 33, 16), (64, 63, 17), (32, 31, 18)]
SEGS_B = [SEGS_A[i] for i in (5, 0, 7, 2, 1, 6, 3, 4)]                # the same segments, other neighbours and offsets
SEGS_C = [(300, 65, 21), (129, 31, 22), (65, 63, 23), (33, 0, 24), (64, 32, 25), (32, 1, 26), (31, 30, 27), (1, 0, 28)]


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. vh_kv_unpack ----------------------------------------------------------------------------------------------------
def _unpack(starts, lens, dst_rows, S_src, B_dst, S_dst, seed=3):
    """kernels.kv_unpack of a random (2, 2, 1, H, S_src, 64) stream into a sentinel-filled (2, 2, B_dst, H, S_dst, 64) cache."""
    from valle2_amd import kernels as K
    src = torch.randn(LAYERS, 2, 1, H, S_src, 64, generator=g(seed)).to(DEV)
    dst = torch.full((LAYERS, 2, B_dst, H, S_dst, 64), SENTINEL, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)   # noqa: E731
    K.kv_unpack(src, dst, i32(starts), i32(lens), i32(dst_rows))
    torch.cuda.synchronize()
    return src, dst


def _check_unpack(src, dst, written):
    """written: {dst row: (first source row, rows)}; every other element of dst keeps the sentinel."""
    untouched = torch.ones(dst.shape, dtype=torch.bool, device=DEV)
    for row, (a, n) in written.items():
        assert torch.equal(dst[:, :, row, :, :n], src[:, :, 0, :, a:a + n]), f'row {row}: {n} rows from {a}'
        untouched[:, :, row, :, :n] = False
    assert bool((dst[untouched] == SENTINEL).all()), 'an element outside the segments\' rows was written'


def test_kv_unpack_copies_every_segment_bit_for_bit_and_nothing_else():
    from valle2_amd.engine import pack_plan
    lens = [n for n, _, _ in SEGS_A]
    starts, M, _ = pack_plan(lens)
    dst_rows = [7, 2, 9, 0, 5, 3, 8, 1]                               # a permutation into 10 rows: rows 4 and 6 stay untouched
    src, dst = _unpack(starts, lens, dst_rows, M + 5, 10, 304)
    _check_unpack(src, dst, {r: (a, n) for r, a, n in zip(dst_rows, starts, lens)})


def test_kv_unpack_cuts_at_the_end_of_the_source_and_of_the_destination():
    # S_src = 120: the segment at row 110 says 20 rows and has 10; S_dst = 40: the 70-row segment is cut at 40
    src, dst = _unpack([0, 110, 30], [5, 20, 70], [2, 0, 1], 120, 3, 40)
    _check_unpack(src, dst, {2: (0, 5), 0: (110, 10), 1: (30, 40)})


def test_kv_unpack_writes_nothing_for_a_row_or_a_start_out_of_range():
    src, dst = _unpack([0, 10, 20, 30, -4, 64, 40], [10, 10, 10, 10, 10, 10, -3], [-1, 4, 1, 1 << 20, 2, 3, 0], 64, 4, 16)
    _check_unpack(src, dst, {1: (20, 10)})


def test_kv_unpack_python_wrappers_check_shapes():
    from valle2_amd import _lib, kernels as K
    from valle2_amd.engine import KVCache
    i32 = torch.zeros(2, dtype=torch.int32, device=DEV)
    src, dst = KVCache(2, 1, H, 16, DEV), KVCache(2, 3, H, 8, DEV)
    with pytest.raises(_lib.VhError, match='one-row'):
        KVCache(2, 2, H, 16, DEV).unpack_into(dst, i32, i32, i32)
    with pytest.raises(_lib.VhError, match='same layers and heads'):
        src.unpack_into(KVCache(3, 3, H, 8, DEV), i32, i32, i32)
    with pytest.raises(_lib.VhError, match='same layers and heads'):
        src.unpack_into(KVCache(2, 3, H + 1, 8, DEV), i32, i32, i32)
    with pytest.raises(_lib.VhError, match='device int32'):
        K.kv_unpack(src.buf, dst.buf, i32, i32[:1], i32)
    with pytest.raises(_lib.VhError, match='device int32'):
        K.kv_unpack(src.buf, dst.buf, i32.long(), i32.long(), i32.long())
    with pytest.raises(_lib.VhError, match='float32'):
        K.kv_unpack(src.buf.half(), dst.buf, i32, i32, i32)


# ---- 2a. the packed prefix-LM attention ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment(length, xl, seed):
    """(q (len, H*64), k, v (H, len, 64)) of one segment and its float64 prefix-LM softmax attention (len, H*64) as float32."""
    from oracle import valle_oracle as O
    q = torch.randn(length, H * 64, generator=g(seed))
    k = torch.randn(H, length, 64, generator=g(seed + 100))
    v = torch.randn(H, length, 64, generator=g(seed + 200))
    qh = q.view(length, H, 64).permute(1, 0, 2).double()
    s = qh @ k.double().transpose(1, 2) / 8.0
    s = s.masked_fill(O.build_attn_mask(xl, length - xl), float('-inf'))
    ref = (torch.softmax(s, dim=-1) @ v.double()).permute(1, 0, 2).reshape(length, H * 64).float()
    return q, k, v, ref


@functools.lru_cache(maxsize=None)
def _attn_packed(segs):
    """vh_attn_rows_packed_lse under the prefix mask over `segs` back to back: (out (M, H*64), starts)."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows([n for n, _, _ in segs], DEV, x_lens=[xl for _, xl, _ in segs])
    M = rows.rows
    q, kc, vc = torch.empty(M, H * 64), torch.empty(1, H, M, 64), torch.empty(1, H, M, 64)
    for a, seg in zip(rows.starts, segs):
        n = seg[0]
        q[a:a + n], kc[0, :, a:a + n], vc[0, :, a:a + n] = _segment(*seg)[:3]
    out = torch.full((M, H * 64), SENTINEL, device=DEV)
    K.attn_rows_packed_lse(q.to(DEV), kc.to(DEV), vc.to(DEV), out, torch.empty(H, M, device=DEV), H, rows, K.MASK_PREFIX)
    torch.cuda.synchronize()
    return out, rows.starts


@pytest.mark.parametrize('segs', [SEGS_A, SEGS_C], ids=['A', 'C'])
def test_packed_prefix_attention_is_vh_attn_rows_on_each_segment_alone(segs):
    from valle2_amd import kernels as K
    out, starts = _attn_packed(tuple(segs))
    for a, (n, xl, seed) in zip(starts, segs):
        q, k, v, ref = _segment(n, xl, seed)
        alone = torch.empty(n, H * 64, device=DEV)
        K.attn_rows(q.to(DEV), k[None].contiguous().to(DEV), v[None].contiguous().to(DEV), alone, 1, H, n, n, K.MASK_PREFIX, x_len=xl)
        got = out[a:a + n]
        print(f'len {n} x_len {xl} at row {a}: max|err| vs float64 {(got.cpu() - ref).abs().max().item():.2e}')
        assert torch.equal(got, alone), f'len {n} x_len {xl} at row {a}: not vh_attn_rows\' bits'
        torch.testing.assert_close(got.cpu(), ref, atol=3e-5, rtol=2e-5)


def test_packed_prefix_attention_does_not_depend_on_neighbours_or_offset():
    out_a, starts_a = _attn_packed(tuple(SEGS_A))
    out_b, starts_b = _attn_packed(tuple(SEGS_B))
    for seg in SEGS_A:
        a, b, n = starts_a[SEGS_A.index(seg)], starts_b[SEGS_B.index(seg)], seg[0]
        assert torch.equal(out_a[a:a + n], out_b[b:b + n]), f'segment {seg} at row {a} and at row {b} differs'
    assert [starts_a[SEGS_A.index(s)] for s in SEGS_A] != [starts_b[SEGS_B.index(s)] for s in SEGS_A]


# ---- 2b. the composite ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack():
    """(cfg, float32 state dict, Transformer on the device): 2 layers, d_model 128, 2 heads, dff 512, LayerNorm."""
    from valle2_amd.modules import Transformer
    cfg = C.cfg_of(dict(d_model=D, n_heads=H, dim_feedforward=DFF, num_layers=LAYERS, dropout=0.0, norm='LayerNorm'))
    gen = g(7)
    tr = Transformer(cfg)
    sd = {k: (0.1 * torch.randn(v.shape, generator=gen) + (1.0 if k.endswith(('norm1.weight', 'norm2.weight')) else 0.0))
          for k, v in tr.state_dict().items()}
    tr.load_state_dict(sd)
    return cfg, sd, tr.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _alone(length, xl, seed):
    """One segment's input rows and, computed once: the padded forward of it alone (B = 1, MASK_PREFIX, its x_len) — hidden rows
    and every layer's K/V — and the float64 oracle's."""
    from oracle import valle_oracle as O
    from valle2_amd import kernels as K
    from valle2_amd.engine import KVCache, transformer_forward
    cfg, sd, tr = _stack()
    x = torch.randn(length, D, generator=g(seed))
    cache = KVCache(LAYERS, 1, H, length, DEV)
    with torch.inference_mode():
        hidden = transformer_forward(tr, x[None].to(DEV).clone(), cache, mode=K.MASK_PREFIX, x_len=xl)[0]
    sd64 = {k: v.double() for k, v in sd.items()}
    h64, kv64 = O.transformer(sd64, '', x[None].double(), cfg, attn_mask=O.build_attn_mask(xl, length - xl), use_cache=True)
    kv64 = torch.stack([torch.stack([k[0], v[0]]) for k, v in kv64]).float()      # (L, 2, H, len, 64)
    return x, hidden.clone(), cache.buf[:, :, 0].clone(), h64[0].float(), kv64


@pytest.mark.parametrize('segs', [SEGS_A, SEGS_C], ids=['A', 'C'])
def test_composite_and_unpack_match_the_padded_forward_of_each_segment_and_float64(segs):
    """x_len = 0 is in both sets: `transformer_forward` accepts it (the mask is then causal)."""
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_packed_lm
    cfg, sd, tr = _stack()
    rows = PackedRows([n for n, _, _ in segs], DEV, x_lens=[xl for _, xl, _ in segs])
    x = torch.cat([_alone(*seg)[0] for seg in segs]).to(DEV)
    stream = KVCache(LAYERS, 1, H, rows.rows + 3, DEV)
    dst = KVCache(LAYERS, len(segs) + 1, H, 304, DEV)
    dst.buf.fill_(SENTINEL)
    dst_rows = [(3 * i + 1) % len(segs) for i in range(len(segs))]          # a permutation (3 and 8 are coprime)
    with torch.inference_mode():
        out = transformer_forward_packed_lm(tr, x, stream, rows)
        stream.unpack_into(dst, rows.seg_start, rows.seg_len, torch.tensor(dst_rows, dtype=torch.int32, device=DEV))
    assert out is x
    worst = {'the padded forward alone': 0.0, 'float64': 0.0}
    for a, r, seg in zip(rows.starts, dst_rows, segs):
        n = seg[0]
        _, hidden, kv, h64, kv64 = _alone(*seg)
        got_kv = dst.buf[:, :, r, :, :n]
        assert torch.equal(got_kv, stream.buf[:, :, 0, :, a:a + n]), 'the unpacked rows are the packed stream\'s bits'
        assert bool((dst.buf[:, :, r, :, n:] == SENTINEL).all())
        for name, want_h, want_kv in (('the padded forward alone', hidden, kv), ('float64', h64.to(DEV), kv64.to(DEV))):
            worst[name] = max(worst[name], (x[a:a + n] - want_h).abs().max().item(), (got_kv - want_kv).abs().max().item())
            torch.testing.assert_close(x[a:a + n], want_h, atol=ATOL, rtol=RTOL, msg=lambda m: f'hidden rows of {seg} vs {name}: {m}')
            torch.testing.assert_close(got_kv, want_kv, atol=ATOL, rtol=RTOL, msg=lambda m: f'K/V rows of {seg} vs {name}: {m}')
    assert bool((dst.buf[:, :, len(segs)] == SENTINEL).all()), 'a cache row no segment names was written'
    print(', '.join(f'worst |packed - {k}| {v:.2e}' for k, v in worst.items()), 'over hidden and K/V rows')


def test_composite_python_wrapper_checks_shapes():
    from valle2_amd import _lib
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_packed_lm
    cfg, sd, tr = _stack()
    rows = PackedRows([4, 6], DEV, x_lens=[2, 0])
    x = torch.zeros(10, D, device=DEV)
    with pytest.raises(_lib.VhError, match='KV cache does not fit'):
        transformer_forward_packed_lm(tr, x, KVCache(LAYERS, 2, H, 10, DEV), rows)
    with pytest.raises(_lib.VhError, match='KV cache does not fit'):
        transformer_forward_packed_lm(tr, x, KVCache(LAYERS, 1, H, 9, DEV), rows)
    with pytest.raises(_lib.VhError, match='rows'):
        transformer_forward_packed_lm(tr, x[:9], KVCache(LAYERS, 1, H, 10, DEV), rows)
    with pytest.raises(_lib.VhError, match=r'\(M, d\)'):
        transformer_forward_packed_lm(tr, x[None], KVCache(LAYERS, 1, H, 10, DEV), rows)
    with pytest.raises(_lib.VhError, match='x_lens'):
        transformer_forward_packed_lm(tr, x, KVCache(LAYERS, 1, H, 10, DEV), PackedRows([4, 6], DEV))
    with pytest.raises(_lib.VhError, match='lse2'):
        transformer_forward_packed_lm(tr, x, KVCache(LAYERS, 1, H, 10, DEV), rows, lse2=torch.zeros(H, 9, device=DEV))


# ---- 3. end to end: the four utterances of test_generate_batch_ragged_rows_vs_oracle ------------------------------------------
KW = dict(d_model=256, n_heads=4, dim_feedforward=1024, num_layers=3, dropout=0.0, norm='LayerNorm', num_beams=1, top_k=1,
          max_audio_len=20)
SHAPES = [(5, 6, 40), (9, 3, 17), (2, 2, 140), (30, 20, 33)]          # (prompt text, target text, frames)
CTX = [a + b + f + 1 for a, b, f in SHAPES]                           # text + BOS + prompt


@functools.lru_cache(maxsize=None)
def _four():
    """(cfg, sd, utterances, per utterance the oracle's tokens and margins on it alone): computed once."""
    from oracle import valle_oracle as O
    from valle2_amd import synth
    cfg = C.cfg_of(KW)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=23, rich=True, std=0.15), cfg)
    utts = [synth.synth_utterance(cfg, a, b, f, seed=700 + i) for i, (a, b, f) in enumerate(SHAPES)]
    refs = []
    for u in utts:
        trace = {}
        ref = O.ar_generate(sd, cfg, *u, trace=trace)
        refs.append((ref, torch.tensor(trace['margin'])))
    return cfg, sd, utts, refs


def _model(packed):
    cfg, sd, utts, refs = _four()
    m = build('ValleAR', KW, sd)
    m.packed_prompt = packed
    return m


def _batch_args(utts):
    return [torch.cat([u[0], u[2]]).to(DEV) for u in utts], [u[1][:, 0].to(DEV) for u in utts]


def _check_packed_stats(st, ctx):
    assert st['packed_prompt'] is True
    assert st['prompt_rows'] == sum(ctx) < st['padded_prompt_rows'] == len(ctx) * max(ctx)


def test_generate_batch_packed_prompt_vs_oracle():
    cfg, sd, utts, refs = _four()
    m = _model(True)
    rows = m.generate_batch(*_batch_args(utts))
    st = m.last_generate_stats
    starts = st['prompt_lens']
    assert starts == [f + 1 for _, _, f in SHAPES] and rows.shape == (4, 141 + 20)
    _check_packed_stats(st, CTX)
    for r, (u, (ref, margin)) in enumerate(zip(utts, refs)):
        tokens_match(rows[r, starts[r]: starts[r] + 20], ref, margin)
        assert torch.equal(rows[r, 1:starts[r]].cpu(), u[1][:, 0]) and int(rows[r, 0]) == cfg.bos_token


def test_generate_many_beams_2_packed_prompt_vs_oracle():
    cfg, sd, utts, refs = _four()
    m = _model(True)
    outs = m.generate_many([(u[0].to(DEV), u[1].to(DEV), u[2].to(DEV)) for u in utts], beams=2)
    st = m.last_generate_stats
    _check_packed_stats(st, CTX)
    assert st['grouped_shared'] is True and st['beams'] == 2 and st['prompt_lens'] == [f + 1 for _, _, f in SHAPES for _ in range(2)]
    for out, (ref, margin) in zip(outs, refs):
        tokens_match(out, ref, margin)


def test_generate_queued_packed_start_and_packed_refill_vs_oracle():
    """max_audio_len 20 under silence_eos: both groups run to the cap inside the first poll of 32 steps, both retire there and
    both take a waiting utterance — the two refills are one packed pass."""
    cfg, sd, utts, refs = _four()
    m = _model(True)
    outs = m.generate_queued([(u[0].to(DEV), u[1].to(DEV), u[2].to(DEV)) for u in utts], beams=2, slots=2)
    st = m.last_generate_stats
    assert st['queued'] is True and st['refills'] == 2 and st['packed_refills'] == 2
    _check_packed_stats(st, CTX[:2])                                  # the starting pass: the first `slots` utterances
    for u, out, saved, (ref, margin) in zip(utts, outs, st['rows'], refs):
        tokens_match(out, ref, margin)
        pl = u[1].shape[0] + 1
        assert bool((saved[:, 0] == cfg.bos_token).all()) and all(torch.equal(row[1:pl].cpu(), u[1][:, 0]) for row in saved)


# ---- 4. the switch off ------------------------------------------------------------------------------------------------------
def _three_calls(m, utts):
    """(tokens, stats) of generate_batch, generate_many(beams=2) and generate_queued(slots=2, beams=2)."""
    tuples = [(u[0].to(DEV), u[1].to(DEV), u[2].to(DEV)) for u in utts]
    out = []
    out.append(([m.generate_batch(*_batch_args(utts))], m.last_generate_stats))
    out.append((m.generate_many(tuples, beams=2), m.last_generate_stats))
    out.append((m.generate_queued(tuples, beams=2, slots=2), m.last_generate_stats))
    return out


def test_switch_off_and_unset_run_the_padded_pass(monkeypatch):
    cfg, sd, utts, refs = _four()
    monkeypatch.delenv('VALLE2_PACKED_PROMPT', raising=False)
    off, unset = _three_calls(_model(False), utts), _three_calls(_model(None), utts)
    for (a, sa), (b, sb) in zip(off, unset):
        for st in (sa, sb):
            assert st['packed_prompt'] is False and st['prompt_rows'] == st['padded_prompt_rows']
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert off[2][1]['packed_refills'] == 0 and unset[2][1]['packed_refills'] == 0 and off[2][1]['refills'] == 2


def test_environment_variable_turns_the_unset_switch_on(monkeypatch):
    cfg, sd, utts, refs = _four()
    monkeypatch.setenv('VALLE2_PACKED_PROMPT', '1')
    m = _model(None)
    rows = m.generate_batch(*_batch_args(utts))
    _check_packed_stats(m.last_generate_stats, CTX)
    for r, (ref, margin) in enumerate(refs):
        tokens_match(rows[r, SHAPES[r][2] + 1: SHAPES[r][2] + 21], ref, margin)
    m.packed_prompt = False                                           # False overrides the variable
    m.generate_batch(*_batch_args(utts))
    assert m.last_generate_stats['packed_prompt'] is False


# ---- 5. calls that do not qualify run the padded pass -------------------------------------------------------------------------
def _tiny(n_heads, packed, max_audio_len=12):
    from valle2_amd import synth
    kw = dict(d_model=D, n_heads=n_heads, dim_feedforward=DFF, num_layers=LAYERS, dropout=0.0, norm='LayerNorm', num_beams=1,
              top_k=1, max_audio_len=max_audio_len)
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=29, rich=True), cfg)
    m = build('ValleAR', kw, sd)
    m.packed_prompt = packed
    return cfg, m


def _ids(cfg, txs, pls, seed=5):
    gen = g(seed)
    return ([torch.randint(0, cfg.vocab_size, (t,), generator=gen).to(DEV) for t in txs],
            [torch.randint(0, cfg.num_audio_tokens, (p,), generator=gen).to(DEV) for p in pls])


@pytest.mark.parametrize('case', ['equal lengths', 'perf_mode', 'head width 32'])
def test_a_call_that_does_not_qualify_runs_the_padded_pass_with_the_same_tokens(case):
    n_heads = 4 if case == 'head width 32' else 2
    txs, pls = ([9, 9, 9], [14, 14, 14]) if case == 'equal lengths' else ([9, 4, 17], [14, 33, 6])
    kwargs = dict(perf_mode=True) if case == 'perf_mode' else {}
    outs = []
    for packed in (True, False):
        cfg, m = _tiny(n_heads, packed)
        outs.append(m.generate_batch(*_ids(cfg, txs, pls), **kwargs))
        st = m.last_generate_stats
        assert st['packed_prompt'] is False and st['prompt_rows'] == st['padded_prompt_rows'] == 3 * max(t + p + 1 for t, p in zip(txs, pls))
    assert torch.equal(*outs), 'the switch changed the tokens of a call the packed pass does not take'


def test_the_same_model_qualifies_on_a_ragged_fp32_call():
    """The control of the fallback cases: the tiny width-64 model on the ragged inputs DOES take the packed pass (its tokens
    are judged against the oracle in the end-to-end tests above; here the stats and the prompt positions)."""
    cfg, m = _tiny(2, True)
    texts, firsts = _ids(cfg, [9, 4, 17], [14, 33, 6])
    rows = m.generate_batch(texts, firsts)
    _check_packed_stats(m.last_generate_stats, [9 + 15, 4 + 34, 17 + 7])
    for r, c in enumerate(firsts):
        assert int(rows[r, 0]) == cfg.bos_token and torch.equal(rows[r, 1:1 + c.shape[0]], c)


# ---- 6. the decoder slot ------------------------------------------------------------------------------------------------------
def test_second_packed_call_reuses_the_decoder_slot():
    cfg, m = _tiny(2, True)
    args = _ids(cfg, [9, 4, 17], [14, 33, 6])
    first = m.generate_batch(*args)
    assert m.last_generate_stats['decoder_reused'] is False and m.last_generate_stats['packed_prompt'] is True
    dec = [s.dec for s in m._decode_slots.values()]
    assert len(dec) == 1 and dec[0]._captured
    again = m.generate_batch(*_ids(cfg, [9, 4, 17], [14, 33, 6], seed=6))     # other ids, the same shape
    st = m.last_generate_stats
    assert st['decoder_reused'] is True and st['slot_uses'] == 2 and st['packed_prompt'] is True
    assert len(m._decode_slots) == 1 and next(iter(m._decode_slots.values())).dec is dec[0], 'nothing was built or captured'
    assert torch.equal(m.generate_batch(*args), first), 'the reused slot gives the first call\'s tokens for the first call\'s ids'
    assert again.shape == first.shape
    m.packed_prompt = False                                                   # the padded pass of the same shape: the same slot
    m.generate_batch(*args)
    assert m.last_generate_stats['decoder_reused'] is True and len(m._decode_slots) == 1


# ---- codec_io: the attribute is the only switch, and it reaches synthesize_* ----------------------------------------------------
def test_the_switch_reaches_codec_io_synthesize():
    from valle2_amd import ConfigValle, codec_io as CIO, get_model_class, synth
    base = dict(d_model=D, n_heads=H, dim_feedforward=256, num_layers=LAYERS, dropout=0.0)
    ar_cfg = ConfigValle(**base, norm='LayerNorm', num_beams=2, top_k=1, max_audio_len=12)
    nar_cfg = ConfigValle(**base, norm='AdaptiveLayerNorm')
    ar = get_model_class('ValleAR')(ar_cfg)
    ar.load_state_dict(synth.silence_eos(synth.make_state_dict(ar_cfg, 'ValleAR', seed=1), ar_cfg))
    nar = get_model_class('ValleNAR')(nar_cfg)
    nar.load_state_dict(synth.make_state_dict(nar_cfg, 'ValleNAR', seed=2))
    ar, nar = ar.to(DEV).eval(), nar.to(DEV).eval()
    items = []
    for i in range(3):
        pt, pc, tt = synth.synth_utterance(ar_cfg, 5 + 2 * i, 7 - i, 9 + 6 * i, seed=60 + i)
        items.append((pt.to(DEV), pc.T.contiguous().to(DEV), tt.to(DEV)))          # codec layout (Q, T)
    ctx = [12 + i + 9 + 6 * i + 1 for i in range(3)]                                # text + BOS + prompt
    for packed in (False, True):
        ar.packed_prompt = packed
        outs = CIO.synthesize_many(ar, nar, items, greedy_nar=True)
        st = ar.last_generate_stats
        assert len(outs) == 3 and st['packed_prompt'] is packed and st['padded_prompt_rows'] == 3 * max(ctx)
        assert st['prompt_rows'] == (sum(ctx) if packed else 3 * max(ctx))
        CIO.synthesize_queued(ar, nar, items, greedy_nar=True, slots=2)
        st = ar.last_generate_stats
        assert st['queued'] is True and st['packed_prompt'] is packed and st['prompt_rows'] == (sum(ctx[:2]) if packed else 2 * max(ctx[:2]))
