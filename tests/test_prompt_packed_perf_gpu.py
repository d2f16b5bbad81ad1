"""The packed AR prompt pass in perf mode on the device: `vh_attn_rows_packed_lm_bf16` against `vh_attn_rows_bf16` on each segment
alone (bit for bit) and float64 prefix-LM softmax attention, `vh_kv_unpack_bf16` (bit-exact rows, nothing else written, the
cuts), `transformer_forward_packed_lm_bf16` against the padded `transformer_forward_bf16(mode=PREFIX)` and the float64 oracle
stack, and `generate_batch(perf_mode=...)` under `ValleAR.packed_prompt_perf` against the float64 oracle with the padded
perf-mode call as the yardstick.

Tolerances (none of them chosen from what the code gives):
  attention kernel vs `vh_attn_rows_bf16` on the segment alone   the same bits (the same body over the same keys in the same order)
  attention kernel vs float64 softmax over the rounded operands  ATOL, RTOL of tests/test_packed_rows16_gpu.py (test_bf16_gpu's bound)
  composite, equal lengths, vs the padded 16-bit forward         the same bits (same GEMM row count, bit-equal attention)
  composite, ragged, vs the float64 oracle stack                 worst error at most 1.5 x the padded 16-bit forward's
                                                                 (tests/test_packed_rows16_gpu.py's factor)
  tokens                                                         every chosen token's float64 logit within 2 MODEL_TOL
                                                                 (tests/test_bf16_gpu.py) of the oracle's maximum, the oracle
                                                                 teacher-forced on the run's own tokens
"""
import functools

import pytest
import torch

from tests.golden import cases as C
from tests.test_bf16_gpu import MODEL_TOL
from tests.test_models_gpu import build
from tests.test_packed_rows16_gpu import ATOL, RTOL, bits
from tests.test_prompt_packed_gpu import KW, SEGS_A, SEGS_B, SEGS_C, SHAPES, CTX, _batch_args, _four, _ids, _tiny
from valle2_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H16 = _lib.h16_dtype()
H = 2                                     # heads of the kernel tests
SENTINEL = -776.0                         # (exact in fp16 and in bf16)
# SEGS_A / SEGS_B / SEGS_C: x_len of 0, 1 and len - 1, across a wave boundary and on a 64-key tile boundary, one row, 300 rows
# (five key tiles: the ring of three images wraps; three query blocks).  Added: x_len = len (full visibility) and x_len > len
# (the clamp)
EXTRA = [(70, 70, 31), (40, 99, 32)]
SETS = {'A': tuple(SEGS_A + EXTRA), 'B': tuple(EXTRA[::-1] + SEGS_B), 'C': tuple(SEGS_C[:4] + EXTRA + SEGS_C[4:])}


def g(seed):
    return torch.Generator().manual_seed(seed)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- 1. the packed prefix-LM attention in the 16-bit format -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment(length, xl, seed):
    """(q' (len, H*64), k, v (H, len, 64)) of one segment in the 16-bit format, q' pre-scaled as vh_linear_qkv_bf16 leaves it and
    rounded once, and float64 prefix-LM softmax attention (len, H*64) over those rounded operands (x_len clamped to len)."""
    from oracle import valle_oracle as O
    from valle2_amd import kernels as K
    q = (torch.randn(length, H * 64, generator=g(seed)) * K.Q16_PRESCALE).to(H16)
    k = torch.randn(H, length, 64, generator=g(seed + 100)).to(H16)
    v = torch.randn(H, length, 64, generator=g(seed + 200)).to(H16)
    qh = q.view(length, H, 64).permute(1, 0, 2).double() / K.Q16_PRESCALE
    s = qh @ k.double().transpose(1, 2) / 8.0
    x = min(xl, length)
    s = s.masked_fill(O.build_attn_mask(x, length - x), float('-inf'))
    ref = (torch.softmax(s, dim=-1) @ v.double()).permute(1, 0, 2).reshape(length, H * 64)
    return q, k, v, ref


def _packed_rows(segs):
    """PackedRows of the segments with their text lengths AS GIVEN on the device (PackedRows itself refuses x_len > len: the
    kernel's clamp is reached by writing the table directly)."""
    from valle2_amd.engine import PackedRows
    rows = PackedRows([n for n, _, _ in segs], DEV, x_lens=[min(xl, n) for n, xl, _ in segs])
    rows.seg_x_len = i32([xl for _, xl, _ in segs])
    return rows


@functools.lru_cache(maxsize=None)
def _run_packed(segs, scale_but=None, tail=8):
    """vh_attn_rows_packed_lm_bf16 over `segs` back to back.  K rows at or beyond M are NaN, V rows Inf, `out` is prefilled with
    a sentinel and has `tail` rows more than M.  scale_but: multiply q, K and V of every segment but this one by -1000.
    Returns (out with its tail, M, starts)."""
    from valle2_amd import kernels as K
    rows = _packed_rows(segs)
    M, S_max = rows.rows, rows.rows + 64
    q = torch.empty(M, H * 64, dtype=H16)
    kc = torch.full((1, H, S_max, 64), float('nan'), dtype=H16)
    vc = torch.full((1, H, S_max, 64), float('inf'), dtype=H16)
    for s, (a, seg) in enumerate(zip(rows.starts, segs)):
        n = seg[0]
        qs, ks, vs, _ = _segment(*seg)
        f = 1.0 if scale_but is None or s == scale_but else -1000.0
        q[a:a + n], kc[0, :, a:a + n], vc[0, :, a:a + n] = f * qs, f * ks, f * vs
    out = torch.full((M + tail, H * 64), SENTINEL, device=DEV, dtype=H16)
    K.attn_rows_packed_lm_bf16(q.to(DEV), kc.to(DEV), vc.to(DEV), out[:M], H, rows)
    torch.cuda.synchronize()
    return out, M, rows.starts


@pytest.mark.parametrize('which', ['A', 'C'])
def test_packed_prefix_attention16_is_vh_attn_rows_bf16_on_each_segment_alone(which):
    from valle2_amd import kernels as K
    segs = SETS[which]
    out, M, starts = _run_packed(segs)
    assert M == sum(n for n, _, _ in segs)
    assert bool(torch.isfinite(out[:M].float()).all()), 'a NaN / Inf row at or beyond M was read as a visible key'
    assert bool((out[M:] == SENTINEL).all()), 'rows of out at or beyond M must keep the sentinel'
    for a, (n, xl, seed) in zip(starts, segs):
        q, k, v, ref = _segment(n, xl, seed)
        alone = torch.empty(n, H * 64, device=DEV, dtype=H16)
        K.attn_rows_bf16(q.to(DEV), k[None].contiguous().to(DEV), v[None].contiguous().to(DEV), alone, 1, H, n, n, K.MASK_PREFIX, x_len=xl)
        got = out[a:a + n]
        same = torch.equal(bits(got), bits(alone))
        print(f'len {n} x_len {xl} at row {a}: bit-equal to vh_attn_rows_bf16 alone: {same}, '
              f'max|err| vs float64 {(got.cpu().double() - ref).abs().max().item():.2e}')
        torch.testing.assert_close(got.cpu().double(), ref, atol=ATOL, rtol=RTOL)
        assert same, f'len {n} x_len {xl} at row {a}: not vh_attn_rows_bf16\'s bits'
    again, _, _ = _run_packed.__wrapped__(segs)                   # (not the cached result: a second launch)
    assert torch.equal(bits(out), bits(again)), 'two runs of the same call must agree bit for bit'


def test_packed_prefix_attention16_does_not_depend_on_neighbours_or_offset():
    (out_a, _, starts_a), (out_b, _, starts_b) = _run_packed(SETS['A']), _run_packed(SETS['B'])
    for seg in SETS['A']:
        a, b, n = starts_a[SETS['A'].index(seg)], starts_b[SETS['B'].index(seg)], seg[0]
        assert torch.equal(bits(out_a[a:a + n]), bits(out_b[b:b + n])), f'segment {seg} at row {a} and at row {b} differs'
    assert [starts_a[SETS['A'].index(s)] for s in SETS['A']] != [starts_b[SETS['B'].index(s)] for s in SETS['A']]


def test_packed_prefix_attention16_segment_does_not_read_its_neighbours():
    segs = SETS['A']
    s = segs.index((129, 33, 16))                                  # neighbours on both sides, one row past a query block
    out, _, starts = _run_packed(segs)
    other, _, _ = _run_packed(segs, scale_but=s)
    a = starts[s]
    assert torch.equal(bits(out[a:a + 129]), bits(other[a:a + 129])), 'q, K, V of the other segments x -1000 changed this segment'
    assert not torch.equal(bits(out[:a]), bits(other[:a]))         # (the others did change)


def test_attn_rows_packed_lm_bf16_python_wrapper_checks_shapes():
    from valle2_amd import kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows([5, 9], DEV, x_lens=[2, 0])
    q = torch.zeros(14, 128, device=DEV, dtype=H16)
    cache = torch.zeros(1, 2, 14, 64, device=DEV, dtype=H16)
    with pytest.raises(_lib.VhError, match='q/out rows'):
        K.attn_rows_packed_lm_bf16(q[:13], cache, cache, q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='cache'):
        K.attn_rows_packed_lm_bf16(q, cache[:, :, :13].contiguous(), cache[:, :, :13].contiguous(), q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='x_lens'):
        K.attn_rows_packed_lm_bf16(q, cache, cache, q.clone(), 2, PackedRows([5, 9], DEV))
    with pytest.raises(_lib.VhError, match='row-major'):           # fp32 operands are not this entry point's
        K.attn_rows_packed_lm_bf16(q.float(), cache, cache, q.clone(), 2, rows)


# ---- 2. vh_kv_unpack_bf16 ---------------------------------------------------------------------------------------------------
LAYERS = 2


def _unpack(starts, lens, dst_rows, S_src, B_dst, S_dst, seed=3):
    """kernels.kv_unpack_bf16 of a random (2, 2, 1, H, S_src, 64) 16-bit stream into a sentinel-filled (2, 2, B_dst, H, S_dst, 64)
    16-bit cache."""
    from valle2_amd import kernels as K
    src = torch.randn(LAYERS, 2, 1, H, S_src, 64, generator=g(seed)).to(H16).to(DEV)
    dst = torch.full((LAYERS, 2, B_dst, H, S_dst, 64), SENTINEL, device=DEV, dtype=H16)
    K.kv_unpack_bf16(src, dst, i32(starts), i32(lens), i32(dst_rows))
    torch.cuda.synchronize()
    return src, dst


def _check_unpack(src, dst, written):
    """written: {dst row: (first source row, rows)}; every other element of dst keeps the sentinel."""
    untouched = torch.ones(dst.shape, dtype=torch.bool, device=DEV)
    for row, (a, n) in written.items():
        assert torch.equal(bits(dst[:, :, row, :, :n]), bits(src[:, :, 0, :, a:a + n])), f'row {row}: {n} rows from {a}'
        untouched[:, :, row, :, :n] = False
    assert bool((dst[untouched] == SENTINEL).all()), 'an element outside the segments\' rows was written'


def test_kv_unpack_bf16_copies_every_segment_bit_for_bit_and_nothing_else():
    from valle2_amd.engine import pack_plan
    lens = [n for n, _, _ in SEGS_A]
    starts, M, _ = pack_plan(lens)
    dst_rows = [7, 2, 9, 0, 5, 3, 8, 1]                               # a permutation into 10 rows: rows 4 and 6 stay untouched
    src, dst = _unpack(starts, lens, dst_rows, M + 5, 10, 304)
    _check_unpack(src, dst, {r: (a, n) for r, a, n in zip(dst_rows, starts, lens)})


def test_kv_unpack_bf16_cuts_at_the_end_of_the_source_and_of_the_destination():
    # S_src = 120: the segment at row 110 says 20 rows and has 10; S_dst = 40: the 70-row segment is cut at 40
    src, dst = _unpack([0, 110, 30], [5, 20, 70], [2, 0, 1], 120, 3, 40)
    _check_unpack(src, dst, {2: (0, 5), 0: (110, 10), 1: (30, 40)})


def test_kv_unpack_bf16_writes_nothing_for_a_row_or_a_start_out_of_range():
    src, dst = _unpack([0, 10, 20, 30, -4, 64, 40], [10, 10, 10, 10, 10, 10, -3], [-1, 4, 1, 1 << 20, 2, 3, 0], 64, 4, 16)
    _check_unpack(src, dst, {1: (20, 10)})


def test_kv_unpack_bf16_one_segment_to_two_destination_rows():
    # 200 rows: more than one 128-row trip of a workgroup
    src, dst = _unpack([3, 3, 210], [200, 200, 7], [1, 3, 0], 230, 5, 208)
    _check_unpack(src, dst, {1: (3, 200), 3: (3, 200), 0: (210, 7)})


def test_kv_unpack_bf16_python_wrappers_check_shapes():
    from valle2_amd import kernels as K
    from valle2_amd.engine import KVCache
    t = torch.zeros(2, dtype=torch.int32, device=DEV)
    src, dst = KVCache(2, 1, H, 16, DEV, dtype=H16), KVCache(2, 3, H, 8, DEV, dtype=H16)
    src.unpack_into(dst, t, i32([1, 1]), t)                           # (the two fit)
    with pytest.raises(_lib.VhError, match='one-row'):
        KVCache(2, 2, H, 16, DEV, dtype=H16).unpack_into(dst, t, t, t)
    with pytest.raises(_lib.VhError, match='same layers and heads'):
        src.unpack_into(KVCache(3, 3, H, 8, DEV, dtype=H16), t, t, t)
    with pytest.raises(_lib.VhError, match='same layers and heads'):
        src.unpack_into(KVCache(2, 3, H + 1, 8, DEV, dtype=H16), t, t, t)
    with pytest.raises(_lib.VhError, match='mixed dtypes'):
        src.unpack_into(KVCache(2, 3, H, 8, DEV), t, t, t)
    with pytest.raises(_lib.VhError, match='mixed dtypes'):
        KVCache(2, 1, H, 16, DEV).unpack_into(dst, t, t, t)
    with pytest.raises(_lib.VhError, match='device int32'):
        K.kv_unpack_bf16(src.buf, dst.buf, t, t[:1], t)
    with pytest.raises(_lib.VhError, match='device int32'):
        K.kv_unpack_bf16(src.buf, dst.buf, t.long(), t.long(), t.long())
    with pytest.raises(_lib.VhError, match='contiguous'):
        K.kv_unpack_bf16(src.buf.float(), dst.buf, t, t, t)
    with pytest.raises(_lib.VhError, match='float32'):                # the fp32 wrapper does not take 16-bit streams
        K.kv_unpack(src.buf, dst.buf, t, t, t)


# ---- 3. the composite -----------------------------------------------------------------------------------------------------
D, NH = 128, 2


@functools.lru_cache(maxsize=None)
def _stack():
    """(cfg, state dict, the stack on the device): 2 layers, d_model 128, 2 heads, dff 256, LayerNorm — test_packed_rows16_gpu's."""
    from tests.test_packed_rows16_gpu import _stack as stack16
    cfg, sd, tr, _ = stack16('LayerNorm')
    return cfg, sd, tr


def _both_forwards(lengths, x_lens, seed):
    """The padded and the packed perf-mode prefix-LM forward of the same utterances: (xs on the host, padded x (B, lmax, d), its
    cache, packed x (M, d), its cache, the PackedRows)."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_bf16, transformer_forward_packed_lm_bf16
    cfg, sd, tr = _stack()
    gen = g(seed)
    B, lmax = len(lengths), max(lengths)
    rows = PackedRows(lengths, DEV, x_lens=x_lens)
    xs = [torch.randn(n, D, generator=gen) for n in lengths]
    padded = torch.zeros(B, lmax, D)
    for b, x in enumerate(xs):
        padded[b, :x.shape[0]] = x
    padded = padded.to(DEV)
    packed = torch.cat(xs).to(DEV)
    cache_pad = KVCache(LAYERS, B, NH, lmax, DEV, dtype=H16)
    cache_pack = KVCache(LAYERS, 1, NH, rows.rows + 3, DEV, dtype=H16)
    if len(set(lengths)) == 1 and len(set(x_lens)) == 1:
        fwd = dict(x_len=x_lens[0])
    else:
        fwd = dict(x_len_dev=i32(x_lens), kv_len=i32(lengths))
    with torch.inference_mode():
        transformer_forward_bf16(tr, padded, cache_pad, mode=K.MASK_PREFIX, **fwd)
        out = transformer_forward_packed_lm_bf16(tr, packed, cache_pack, rows)
    assert out is packed
    torch.cuda.synchronize()
    return xs, padded, cache_pad, packed, cache_pack, rows


def test_forward_packed_lm_bf16_equal_lengths_is_the_padded_forward_bit_for_bit():
    """Three utterances of 96 rows, text length 40: the GEMMs of both forms see the same M = 288 rows and the attention is
    bit-equal per segment, so x and every layer's K and V rows are the same bits."""
    lengths = [96, 96, 96]
    _, padded, cache_pad, packed, cache_pack, rows = _both_forwards(lengths, [40, 40, 40], 11)
    assert packed.shape[0] == padded.shape[0] * padded.shape[1] == 288          # both forms: the same GEMM row count
    assert torch.equal(packed, padded.view(-1, D)), \
        f'x differs in {(packed != padded.view(-1, D)).sum().item()} elements, worst {(packed - padded.view(-1, D)).abs().max().item():.2e}'
    for layer in range(LAYERS):
        for kv in (0, 1):
            for b, n in enumerate(lengths):
                a = rows.starts[b]
                assert torch.equal(bits(cache_pack.buf[layer, kv, 0, :, a:a + n]), bits(cache_pad.buf[layer, kv, b, :, :n])), \
                    f'layer {layer} {"KV"[kv]} rows of utterance {b} differ'


def test_forward_packed_lm_bf16_ragged_is_as_close_to_the_oracle_as_the_padded_forward():
    """Against the float64 oracle stack under the prefix mask, per utterance: the packed and the padded 16-bit forward are the
    same arithmetic at other GEMM row counts, so their worst errors are rounding noise of one size; a wrong row, a wrong mask or
    a leaked neighbour is O(1)."""
    from oracle import valle_oracle as O
    lengths, x_lens = [5, 70, 129, 33], [2, 64, 33, 0]
    cfg, sd, _ = _stack()
    xs, padded, _, packed, _, rows = _both_forwards(lengths, x_lens, 13)
    sd64 = {k: v.double() for k, v in sd.items()}
    e_packed = e_padded = 0.0
    for b, (x, xl) in enumerate(zip(xs, x_lens)):
        n, a = x.shape[0], rows.starts[b]
        ref, _ = O.transformer(sd64, '', x.double()[None], cfg, attn_mask=O.build_attn_mask(xl, n - xl))
        e_packed = max(e_packed, (packed[a:a + n].cpu().double() - ref[0]).abs().max().item())
        e_padded = max(e_padded, (padded[b, :n].cpu().double() - ref[0]).abs().max().item())
    print(f'{lengths} / {x_lens}: worst |x - oracle| packed {e_packed:.2e}, padded {e_padded:.2e}')
    assert e_packed <= 1.5 * e_padded, f'packed {e_packed:.2e} against padded {e_padded:.2e}'


def test_forward_packed_lm_bf16_python_wrapper_checks_shapes():
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_packed_lm_bf16
    from valle2_amd.modules import Transformer
    _, _, tr = _stack()
    rows = PackedRows([4, 6], DEV, x_lens=[2, 0])
    x = torch.zeros(10, D, device=DEV)
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_lm_bf16(tr, x, KVCache(LAYERS, 1, NH, 10, DEV), rows)                      # an fp32 cache
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_lm_bf16(tr, x, KVCache(LAYERS, 2, NH, 10, DEV, dtype=H16), rows)          # two cache rows
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_lm_bf16(tr, x, KVCache(LAYERS, 1, NH, 9, DEV, dtype=H16), rows)           # s_max < M
    with pytest.raises(_lib.VhError, match='rows'):
        transformer_forward_packed_lm_bf16(tr, x[:9], KVCache(LAYERS, 1, NH, 10, DEV, dtype=H16), rows)
    with pytest.raises(_lib.VhError, match=r'\(M, d\)'):
        transformer_forward_packed_lm_bf16(tr, x[None], KVCache(LAYERS, 1, NH, 10, DEV, dtype=H16), rows)
    with pytest.raises(_lib.VhError, match='x_lens'):
        transformer_forward_packed_lm_bf16(tr, x, KVCache(LAYERS, 1, NH, 10, DEV, dtype=H16), PackedRows([4, 6], DEV))
    cfg = C.cfg_of(dict(d_model=D, n_heads=NH, dim_feedforward=192, num_layers=1, dropout=0.0, norm='LayerNorm'))
    with pytest.raises(_lib.VhError, match='multiples of 128'):                                               # a dff of 192
        transformer_forward_packed_lm_bf16(Transformer(cfg).to(DEV).eval(), x, KVCache(1, 1, NH, 10, DEV, dtype=H16), rows)


# ---- 4. end to end: the four ragged utterances of tests/test_prompt_packed_gpu.py ---------------------------------------------
N_NEW = KW['max_audio_len']


@functools.lru_cache(maxsize=None)
def _inputs(dff):
    """(kw, cfg, state dict, utterances): the model of test_prompt_packed_gpu (dff 1024), or the same at another dff."""
    from valle2_amd import synth
    if dff == KW['dim_feedforward']:
        cfg, sd, utts, _ = _four()
        return KW, cfg, sd, utts
    kw = dict(KW, dim_feedforward=dff)
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=23, rich=True, std=0.15), cfg)
    return kw, cfg, sd, _four()[2]


def _worst_gap_below_the_oracles_maximum(cfg, sd, utts, rows, starts):
    """The largest (oracle's max logit - oracle's logit of the chosen token) over every generated token of every utterance, the
    float64 oracle teacher-forced on the run's own tokens; also: the prompt columns hold BOS + the prompt."""
    from oracle import valle_oracle as O
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    rows, worst = rows.cpu(), 0.0
    assert rows.shape == (len(utts), max(starts) + N_NEW)
    for r, u in enumerate(utts):
        pl = starts[r]
        assert int(rows[r, 0]) == cfg.bos_token and torch.equal(rows[r, 1:pl], u[1][:, 0]), 'the prompt columns hold BOS + the prompt'
        text, codes = torch.cat([u[0], u[2]]), rows[r, :pl + N_NEW]
        assert int(codes[pl:].min()) >= 0 and int(codes[pl:].max()) < cfg.num_audio_tokens     # (EOS is silenced: 20 tokens each)
        batch = dict(tokens=text[None], codes=codes[None, :-1], tokens_lens=torch.tensor([text.shape[0]]),
                     codes_lens=torch.tensor([codes.shape[0] - 1]))
        logits = O.ar_logits(sd64, cfg, batch)[0].T[pl - 1:]                                   # (N_NEW, V + 1): position i predicts token i + 1
        gap = logits.max(dim=-1).values - logits.gather(1, codes[pl:, None]).squeeze(1)
        worst = max(worst, gap.max().item())
    return worst


@pytest.mark.parametrize('perf_mode,dff', [(True, 1024), ('kv', 1024), (True, 192)], ids=['perf', 'kv', 'perf-dff192'])
def test_generate_batch_packed_perf_chooses_a_leading_token_of_the_oracle(perf_mode, dff):
    """The padded perf-mode call goes first, as the yardstick: inputs on which IT leaves the bound would be the wrong inputs.
    perf_mode=True at dff 192 is a shape the 16-bit stack does not take: the fp32 packed pass, narrowed once."""
    kw, cfg, sd, utts = _inputs(dff)
    m = build('ValleAR', kw, sd)
    starts = [f + 1 for _, _, f in SHAPES]
    prefill16 = perf_mode is True and dff % 128 == 0
    m.packed_prompt_perf = False
    padded_rows = m.generate_batch(*_batch_args(utts), perf_mode=perf_mode)
    st = m.last_generate_stats
    assert st['packed_prompt'] is False and st['prompt_rows'] == st['padded_prompt_rows'] == len(CTX) * max(CTX)
    assert st['prefill_bf16'] is prefill16 and st['kv_bf16'] is True
    padded = _worst_gap_below_the_oracles_maximum(cfg, sd, utts, padded_rows, starts)
    m.packed_prompt_perf = True
    packed_rows = m.generate_batch(*_batch_args(utts), perf_mode=perf_mode)
    st = m.last_generate_stats
    assert st['packed_prompt'] is True
    assert st['prompt_rows'] == sum(CTX) < st['padded_prompt_rows'] == len(CTX) * max(CTX)
    assert st['prefill_bf16'] is prefill16 and st['kv_bf16'] is True and st['prompt_lens'] == starts
    packed = _worst_gap_below_the_oracles_maximum(cfg, sd, utts, packed_rows, starts)
    print(f'perf_mode={perf_mode!r} dff {dff}: largest (max logit - logit of the chosen token): padded {padded:.2e}, packed {packed:.2e} '
          f'(bound {2 * MODEL_TOL:.1e}); tokens equal: {torch.equal(padded_rows, packed_rows)}')
    assert padded <= 2 * MODEL_TOL, f'the padded perf-mode call itself is {padded:.2e} below the maximum: wrong inputs for this test'
    assert packed <= 2 * MODEL_TOL, f'the packed perf-mode call chose a token {packed:.2e} below the oracle\'s maximum'


def test_environment_variable_turns_the_unset_switch_on(monkeypatch):
    kw, cfg, sd, utts = _inputs(1024)
    m = build('ValleAR', kw, sd)
    monkeypatch.delenv('VALLE2_PACKED_PROMPT_PERF', raising=False)
    m.generate_batch(*_batch_args(utts), perf_mode=True)
    assert m.last_generate_stats['packed_prompt'] is False
    monkeypatch.setenv('VALLE2_PACKED_PROMPT_PERF', '1')
    m.generate_batch(*_batch_args(utts), perf_mode=True)
    assert m.last_generate_stats['packed_prompt'] is True and m.last_generate_stats['prompt_rows'] == sum(CTX)
    m.packed_prompt_perf = False                                      # False overrides the variable
    m.generate_batch(*_batch_args(utts), perf_mode=True)
    assert m.last_generate_stats['packed_prompt'] is False


# ---- 5. calls that do not qualify run the padded pass ---------------------------------------------------------------------------
RAGGED = ([9, 4, 17], [14, 33, 6])


@pytest.mark.parametrize('case', ['equal lengths', 'head width 32', 'shared_prompt', 'fp32'])
def test_a_call_that_does_not_qualify_runs_the_padded_pass_with_the_same_tokens(case):
    n_heads = 4 if case == 'head width 32' else 2
    txs, pls = ([9, 9, 9], [14, 14, 14]) if case in ('equal lengths', 'shared_prompt') else RAGGED
    kwargs = dict(perf_mode=True) if case in ('equal lengths', 'shared_prompt') else {}      # (head width 32 refuses perf_mode)
    outs = []
    for switch in (True, False):
        cfg, m = _tiny(n_heads, None)
        m.packed_prompt_perf = switch
        texts, firsts = _ids(cfg, txs, pls)
        if case == 'shared_prompt':
            texts, firsts, kwargs = [texts[0]] * 3, [firsts[0]] * 3, dict(perf_mode=True, shared_prompt=True)
        outs.append(m.generate_batch(texts, firsts, **kwargs))
        st = m.last_generate_stats
        rows = 1 if case == 'shared_prompt' else 3
        assert st['packed_prompt'] is False and st['prompt_rows'] == st['padded_prompt_rows'] == rows * max(t + p + 1 for t, p in zip(txs, pls))
        if case == 'head width 32':
            with pytest.raises(ValueError, match='head width 32'):
                m.generate_batch(texts, firsts, perf_mode=True)
    assert torch.equal(*outs), 'the switch changed the tokens of a call the packed pass does not take'


def test_the_fp32_switch_alone_leaves_a_perf_call_on_the_padded_pass_and_this_one_takes_it():
    cfg, m = _tiny(2, True)                                           # packed_prompt = True, packed_prompt_perf unset
    args = _ids(cfg, *RAGGED)
    padded = m.generate_batch(*args, perf_mode=True)
    assert m.last_generate_stats['packed_prompt'] is False
    m.packed_prompt, m.packed_prompt_perf = None, True                # the control: the same model and inputs DO take the packed pass
    rows = m.generate_batch(*args, perf_mode=True)
    st = m.last_generate_stats
    ctx = [t + p + 1 for t, p in zip(*RAGGED)]
    assert st['packed_prompt'] is True and st['prompt_rows'] == sum(ctx) < st['padded_prompt_rows'] == 3 * max(ctx)
    assert rows.shape == padded.shape
    for r, c in enumerate(args[1]):
        assert int(rows[r, 0]) == cfg.bos_token and torch.equal(rows[r, 1:1 + c.shape[0]], c)
    m.generate_batch(*args)                                           # and an fp32 call of it runs padded
    assert m.last_generate_stats['packed_prompt'] is False


# ---- 6. the decoder slot ------------------------------------------------------------------------------------------------------
def test_second_packed_perf_call_reuses_the_decoder_slot():
    cfg, m = _tiny(2, None)
    m.packed_prompt_perf = True
    args = _ids(cfg, *RAGGED)
    first = m.generate_batch(*args, perf_mode=True)
    st = m.last_generate_stats
    assert st['decoder_reused'] is False and st['packed_prompt'] is True and st['prefill_bf16'] is True
    dec = [s.dec for s in m._decode_slots.values()]
    assert len(dec) == 1
    again = m.generate_batch(*args, perf_mode=True)
    st = m.last_generate_stats
    assert st['decoder_reused'] is True and st['slot_uses'] == 2 and st['packed_prompt'] is True
    assert len(m._decode_slots) == 1 and next(iter(m._decode_slots.values())).dec is dec[0], 'nothing was built or captured'
    assert torch.equal(again, first), 'the reused slot gives the first call\'s tokens'
