"""Packed NAR decoding in perf mode on the device: `vh_attn_rows_packed_bf16` against float64 softmax attention per segment and,
bit for bit, against `vh_attn_rows_bf16` on the segment alone (and for what it may never do: read a neighbour, read or write
past the rows), `transformer_forward_packed_bf16` against the padded `transformer_forward_bf16` and the float64 oracle stack,
and `ValleNAR.generate_packed_perf` against the oracle with `generate_batch(perf_mode=True)` as the yardstick."""
import functools

import pytest
import torch

from tests.golden import cases as C
from tests.test_bf16_gpu import EPS, FP16, MODEL_TOL
from tests.test_nar_generate_gpu import _utterances
from tests.test_packed_rows_gpu import EDGES, EXISTING, _args, _oracle_stage_logits, _setup
from valle2_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H16 = _lib.h16_dtype()
H = 2                                     # heads of the kernel tests
SENTINEL = -776.0                         # (exact in fp16 and in bf16)
ATOL, RTOL = (1e-3 if FP16 else 6e-3), 2 * EPS            # test_bf16_gpu.test_attn_rows_bf16's
# M = 1028: starts off every 8-, 64- and 128-row boundary; 257 and 193 rows are five and four 64-key tiles (the ring of three
# images wraps), 129 and 257 are one row past a query block
MIXED = [1, 63, 64, 65, 127, 128, 129, 257, 5, 193]


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- kernel -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment(length, seed):
    """(q' (len, H*64), k, v (H, len, 64)) of one segment in the 16-bit format, q' pre-scaled as vh_linear_qkv_bf16 leaves it
    and rounded once, and the float64 softmax attention (len, H*64) over those rounded operands."""
    from valle2_amd import kernels as K
    q = (torch.randn(length, H * 64, generator=g(seed)) * K.Q16_PRESCALE).to(H16)
    k = torch.randn(H, length, 64, generator=g(seed + 1)).to(H16)
    v = torch.randn(H, length, 64, generator=g(seed + 2)).to(H16)
    qh = q.view(length, H, 64).permute(1, 0, 2).double() / K.Q16_PRESCALE
    p = torch.softmax(qh @ k.double().transpose(1, 2) / 8.0, dim=-1)
    ref = (p @ v.double()).permute(1, 0, 2).reshape(length, H * 64)
    return q, k, v, ref


def _run_packed(lengths, seeds, scale=None, tail=8):
    """vh_attn_rows_packed_bf16 over the segments (length, seed) laid out back to back; K rows at or beyond M are NaN, V rows
    Inf, `out` is prefilled with a sentinel and has `tail` rows more than M.  scale[s]: multiply segment s's q, K and V.
    Returns (out with its tail, M, starts)."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows(lengths, DEV)
    M, S_max = rows.rows, rows.rows + 64
    q = torch.empty(M, H * 64, dtype=H16)
    kc = torch.full((1, H, S_max, 64), float('nan'), dtype=H16)
    vc = torch.full((1, H, S_max, 64), float('inf'), dtype=H16)
    for s, (n, seed) in enumerate(zip(lengths, seeds)):
        qs, ks, vs, _ = _segment(n, seed)
        f = 1.0 if scale is None else scale[s]
        a = rows.starts[s]
        q[a:a + n], kc[0, :, a:a + n], vc[0, :, a:a + n] = f * qs, f * ks, f * vs
    out = torch.full((M + tail, H * 64), SENTINEL, device=DEV, dtype=H16)
    K.attn_rows_packed_bf16(q.to(DEV), kc.to(DEV), vc.to(DEV), out[:M], H, rows)
    torch.cuda.synchronize()
    return out, M, rows.starts


@pytest.mark.parametrize('lengths', [[1], [63], [64], [65], [128], [129], [193], MIXED], ids=lambda v: '-'.join(map(str, v)))
def test_attn_rows_packed_bf16_matches_float64_and_the_padded_kernel_per_segment(lengths):
    from valle2_amd import kernels as K
    seeds = [100 + 3 * i for i in range(len(lengths))]
    out, M, starts = _run_packed(lengths, seeds)
    assert M == sum(lengths)
    assert bool(torch.isfinite(out[:M].float()).all()), 'a NaN / Inf row at or beyond M was read as a visible key'
    assert bool((out[M:] == SENTINEL).all()), 'rows of out at or beyond M must keep the sentinel'
    for s, (n, seed) in enumerate(zip(lengths, seeds)):
        q, k, v, ref = _segment(n, seed)
        got = out[starts[s]:starts[s] + n]
        # the same segment through vh_attn_rows_bf16 alone (B = 1, Tq = Tk = len, full mask) on its own cache
        alone = torch.empty(n, H * 64, device=DEV, dtype=H16)
        K.attn_rows_bf16(q.to(DEV), k[None].contiguous().to(DEV), v[None].contiguous().to(DEV), alone, 1, H, n, n, K.MASK_FULL)
        same = torch.equal(bits(got), bits(alone))
        print(f'segment {s} (len {n} at row {starts[s]}): bit-equal to vh_attn_rows_bf16 alone: {same}, '
              f'max|err| vs float64 {(got.cpu().double() - ref).abs().max().item():.2e}')
        torch.testing.assert_close(got.cpu().double(), ref, atol=ATOL, rtol=RTOL)
        assert same, f'segment {s} (len {n} at row {starts[s]}) differs from vh_attn_rows_bf16 on the segment alone'
    again, _, _ = _run_packed(lengths, seeds)
    assert torch.equal(bits(out), bits(again)), 'two runs of the same call must agree bit for bit'


def test_attn_rows_packed_bf16_segment_does_not_depend_on_its_neighbours():
    seeds = [100 + 3 * i for i in range(len(MIXED))]
    s = MIXED.index(129)
    out, _, starts = _run_packed(MIXED, seeds)
    scale = [1.0 if i == s else -1000.0 for i in range(len(MIXED))]
    other, _, _ = _run_packed(MIXED, seeds, scale=scale)
    a = starts[s]
    assert torch.equal(bits(out[a:a + 129]), bits(other[a:a + 129])), 'q, K, V of the other segments x -1000 changed this segment'
    assert not torch.equal(bits(out[:a]), bits(other[:a]))        # (the others did change)


def test_attn_rows_packed_bf16_segment_does_not_depend_on_its_offset():
    first, _, _ = _run_packed([129], [300])
    after, _, starts = _run_packed([77, 129], [400, 300])
    assert starts == [0, 77]
    assert torch.equal(bits(first[:129]), bits(after[77:77 + 129])), 'the same segment at row 77 differs from itself at row 0'


def test_attn_rows_packed_bf16_python_wrapper_checks_shapes():
    from valle2_amd import kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows([5, 9], DEV)
    q = torch.zeros(14, 128, device=DEV, dtype=H16)
    cache = torch.zeros(1, 2, 14, 64, device=DEV, dtype=H16)
    with pytest.raises(_lib.VhError, match='q/out rows'):
        K.attn_rows_packed_bf16(q[:13], cache, cache, q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='cache'):
        K.attn_rows_packed_bf16(q, cache[:, :, :13].contiguous(), cache[:, :, :13].contiguous(), q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='cache'):
        K.attn_rows_packed_bf16(q, cache.expand(2, -1, -1, -1).contiguous(), cache.expand(2, -1, -1, -1).contiguous(), q.clone(),
                                2, rows)
    with pytest.raises(_lib.VhError, match='row-major'):           # fp32 operands are not this entry point's
        K.attn_rows_packed_bf16(q.float(), cache, cache, q.clone(), 2, rows)


# ---- forward ------------------------------------------------------------------------------------------------------------
D, NH, LAYERS = 128, 2, 2


@functools.lru_cache(maxsize=None)
def _stack(norm):
    """(cfg, state dict, the stack on the device, its AdaLN embedding on the host or None)."""
    from valle2_amd.modules import Transformer
    cfg = C.cfg_of(dict(d_model=D, n_heads=NH, dim_feedforward=256, num_layers=LAYERS, dropout=0.0, norm=norm))
    gen = g(7)
    tr = Transformer(cfg)
    sd = {k: (0.1 * torch.randn(v.shape, generator=gen) + (1.0 if k.endswith(('norm.weight', 'norm1.weight', 'norm2.weight'))
                                                            else 0.0)) for k, v in tr.state_dict().items()}
    tr.load_state_dict(sd)
    emb = torch.randn(1, D, generator=gen) if norm != 'LayerNorm' else None
    return cfg, sd, tr.to(DEV).eval(), emb


def _both_forwards(norm, lengths, seed):
    """The padded and the packed perf-mode forward of the same utterances: (xs on the host, padded x (B, lmax, d), its cache,
    packed x (M, d), its cache, the PackedRows)."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_bf16, transformer_forward_packed_bf16
    cfg, sd, tr, emb = _stack(norm)
    gen = g(seed)
    B, lmax = len(lengths), max(lengths)
    rows = PackedRows(lengths, DEV)
    xs = [torch.randn(n, D, generator=gen) for n in lengths]
    padded = torch.zeros(B, lmax, D)
    for b, x in enumerate(xs):
        padded[b, :x.shape[0]] = x
    padded = padded.to(DEV)
    packed = torch.cat(xs).to(DEV)
    cache_pad = KVCache(LAYERS, B, NH, lmax, DEV, dtype=H16)
    cache_pack = KVCache(LAYERS, 1, NH, rows.rows + 3, DEV, dtype=H16)
    e = None if emb is None else emb.to(DEV)
    kv_len = None if len(set(lengths)) == 1 else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    with torch.inference_mode():
        transformer_forward_bf16(tr, padded, cache_pad, mode=K.MASK_FULL, kv_len=kv_len, embedding=e)
        out = transformer_forward_packed_bf16(tr, packed, cache_pack, rows, embedding=e)
    assert out is packed
    torch.cuda.synchronize()
    return xs, padded, cache_pad, packed, cache_pack, rows


@pytest.mark.parametrize('norm', ['LayerNorm', 'AdaptiveLayerNorm'])
def test_forward_packed_bf16_equal_lengths_is_the_padded_forward_bit_for_bit(norm):
    """Three utterances of 96 rows: the GEMMs of both forms see the same M = 288 rows and the attention is bit-equal per
    segment, so x and every layer's K and V rows are the same bits."""
    lengths = [96, 96, 96]
    _, padded, cache_pad, packed, cache_pack, rows = _both_forwards(norm, lengths, 11)
    assert torch.equal(packed, padded.view(-1, D)), \
        f'x differs in {(packed != padded.view(-1, D)).sum().item()} elements, worst {(packed - padded.view(-1, D)).abs().max().item():.2e}'
    for layer in range(LAYERS):
        for kv in (0, 1):
            for b, n in enumerate(lengths):
                a = rows.starts[b]
                assert torch.equal(bits(cache_pack.buf[layer, kv, 0, :, a:a + n]), bits(cache_pad.buf[layer, kv, b, :, :n])), \
                    f'layer {layer} {"KV"[kv]} rows of utterance {b} differ'


@pytest.mark.parametrize('norm', ['LayerNorm', 'AdaptiveLayerNorm'])
@pytest.mark.parametrize('lengths', [[5, 70, 129, 33], [3, 40]], ids=lambda v: '-'.join(map(str, v)))
def test_forward_packed_bf16_ragged_is_as_close_to_the_oracle_as_the_padded_forward(lengths, norm):
    """Against the float64 oracle stack per utterance: the packed and the padded 16-bit forward are the same arithmetic at
    other GEMM row counts, so their worst errors are rounding noise of one size; a wrong row or a leaked neighbour is O(1)."""
    from oracle import valle_oracle as O
    cfg, sd, _, emb = _stack(norm)
    xs, padded, _, packed, _, rows = _both_forwards(norm, lengths, 13)
    sd64 = {k: v.double() for k, v in sd.items()}
    e_packed = e_padded = 0.0
    for b, x in enumerate(xs):
        n, a = x.shape[0], rows.starts[b]
        ref, _ = O.transformer(sd64, '', x.double()[None], cfg, embedding=None if emb is None else emb.double())
        e_packed = max(e_packed, (packed[a:a + n].cpu().double() - ref[0]).abs().max().item())
        e_padded = max(e_padded, (padded[b, :n].cpu().double() - ref[0]).abs().max().item())
    print(f'{norm} {lengths}: worst |x - oracle| packed {e_packed:.2e}, padded {e_padded:.2e}')
    assert e_packed <= 1.5 * e_padded, f'packed {e_packed:.2e} against padded {e_padded:.2e}'


def test_forward_packed_bf16_python_wrapper_checks_shapes():
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_packed_bf16
    from valle2_amd.modules import Transformer
    _, _, tr, _ = _stack('LayerNorm')
    rows = PackedRows([4, 6], DEV)
    x = torch.zeros(10, D, device=DEV)
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_bf16(tr, x, KVCache(LAYERS, 2, NH, 10, DEV, dtype=H16), rows)          # two cache rows
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_bf16(tr, x, KVCache(LAYERS, 1, NH, 9, DEV, dtype=H16), rows)           # s_max < M
    with pytest.raises(_lib.VhError, match='bf16 KV cache'):
        transformer_forward_packed_bf16(tr, x, KVCache(LAYERS, 1, NH, 10, DEV), rows)                      # an fp32 cache
    with pytest.raises(_lib.VhError, match='rows'):
        transformer_forward_packed_bf16(tr, x[:9], KVCache(LAYERS, 1, NH, 10, DEV, dtype=H16), rows)
    with pytest.raises(_lib.VhError, match=r'\(M, d\)'):
        transformer_forward_packed_bf16(tr, x[None], KVCache(LAYERS, 1, NH, 10, DEV, dtype=H16), rows)
    cfg = C.cfg_of(dict(d_model=D, n_heads=NH, dim_feedforward=192, num_layers=1, dropout=0.0, norm='LayerNorm'))
    with pytest.raises(_lib.VhError, match='multiples of 128'):
        transformer_forward_packed_bf16(Transformer(cfg).to(DEV).eval(), x, KVCache(1, 1, NH, 10, DEV, dtype=H16), rows)


# ---- model --------------------------------------------------------------------------------------------------------------
def _worst_gap_below_the_oracles_maximum(cfg, sd, us, outs):
    """Shapes, dtype, column 0 and token range of `outs`; returns the largest (oracle's max logit - oracle's logit of the chosen
    token) over every frame of every stage, the oracle teacher-forced on the run's own earlier codebooks."""
    worst = 0.0
    assert len(outs) == len(us)
    for (text, pc, first), got in zip(us, outs):
        assert got.dtype == torch.int64 and got.is_cuda
        got = got.cpu()
        assert got.shape == (first.shape[0], cfg.num_quantizers)
        assert torch.equal(got[:, 0], first), 'column 0 is the given first layer'
        assert int(got.min()) >= 0 and int(got.max()) < cfg.num_audio_tokens
        for n in range(1, cfg.num_quantizers):
            logits = _oracle_stage_logits(sd, cfg, text, pc, got, n)
            gap = logits.max(dim=-1).values - logits.gather(1, got[:, n:n + 1]).squeeze(1)
            worst = max(worst, gap.max().item())
    return worst


@pytest.mark.parametrize('which', ['existing', 'edges'])
def test_generate_packed_perf_chooses_a_leading_token_of_the_oracle(which):
    """At every frame of every stage the token the run chose is within 2 MODEL_TOL of the oracle's maximum.  The padded
    perf-mode form goes first, as the yardstick: inputs on which IT leaves the bound would be the wrong inputs."""
    cfg, sd, m = _setup()
    us = _utterances(cfg, *(EXISTING if which == 'existing' else EDGES))
    padded = _worst_gap_below_the_oracles_maximum(cfg, sd, us, m.generate_batch(*_args(us), greedy=True, perf_mode=True))
    packed = _worst_gap_below_the_oracles_maximum(cfg, sd, us, m.generate_packed_perf(*_args(us), greedy=True))
    print(f'{which}: largest (max logit - logit of the chosen token): padded perf mode {padded:.2e}, packed perf mode {packed:.2e} '
          f'(bound {2 * MODEL_TOL:.1e})')
    assert padded <= 2 * MODEL_TOL, f'generate_batch(perf_mode=True) itself is {padded:.2e} below the maximum: wrong inputs for this test'
    assert packed <= 2 * MODEL_TOL, f'generate_packed_perf chose a token {packed:.2e} below the oracle\'s maximum'


def test_generate_packed_perf_per_request_sampling():
    from valle2_amd import Sampling
    cfg, sd, m = _setup()
    us = _utterances(cfg, *EXISTING)
    greedy = m.generate_packed_perf(*_args(us), greedy=True)
    top1 = m.generate_packed_perf(*_args(us), sampling=[Sampling(seed=50 + i, top_k=1) for i in range(len(us))])
    assert all(torch.equal(a, b) for a, b in zip(greedy, top1)), 'top_k=1 per request is the greedy result'
    us = us[:3] + [us[0]]                                          # utterances 0 and 3: identical inputs
    reqs = [Sampling(seed=7, temperature=0.9), Sampling(seed=8, temperature=1.1), Sampling(seed=9, temperature=0.9),
            Sampling(seed=10, temperature=0.9)]
    a = m.generate_packed_perf(*_args(us), sampling=reqs)
    b = m.generate_packed_perf(*_args(us), sampling=reqs)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the same seeds must give the same codes'
    assert not torch.equal(a[0], a[3]), 'identical inputs, different seeds'
    for (_, _, first), x in zip(us, a):
        assert torch.equal(x[:, 0].cpu(), first) and int(x.min()) >= 0 and int(x.max()) < cfg.num_audio_tokens
    with pytest.raises(ValueError, match='seed='):
        m.generate_packed_perf(*_args(us), seed=3, sampling=reqs)
