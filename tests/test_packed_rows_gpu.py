"""NAR decoding over packed rows on the device: `vh_attn_rows_packed` against float64 softmax attention per segment (and for
what it may never do: read a neighbour, read or write past the rows), `transformer_forward_packed` against the padded
`transformer_forward`, and `ValleNAR.generate_packed` against `generate_batch` and the oracle."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.golden import cases as C
from tests.test_nar_generate_gpu import _model, _utterances

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = 2                                     # heads of the kernel tests
SENTINEL = -777.25
MIXED = [1, 31, 32, 33, 127, 128, 129, 257, 5]            # M = 743: starts off every 4-, 32- and 128-row boundary
ATOL, RTOL = 2e-4, 1e-4                   # the project's summation-order bound (test_perf_mode_beams_gpu.py)


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---- kernel -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment(length, seed):
    """(q (len, H*64), k, v (H, len, 64)) of one segment, and its float64 softmax attention (len, H*64) float32."""
    q = torch.randn(length, H * 64, generator=g(seed))
    k = torch.randn(H, length, 64, generator=g(seed + 1))
    v = torch.randn(H, length, 64, generator=g(seed + 2))
    qh = q.view(length, H, 64).permute(1, 0, 2).double()
    p = torch.softmax(qh @ k.double().transpose(1, 2) / 8.0, dim=-1)
    ref = (p @ v.double()).permute(1, 0, 2).reshape(length, H * 64).float()
    return q, k, v, ref


def _run_packed(lengths, seeds, scale=None, tail=8):
    """vh_attn_rows_packed over the segments (length, seed) laid out back to back; K rows at or beyond M are NaN, V rows Inf,
    `out` is prefilled with a sentinel and has `tail` rows more than M.  scale[s]: multiply segment s's q, K and V.
    Returns (out with its tail, M, starts)."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows(lengths, DEV)
    M, S_max = rows.rows, rows.rows + 64
    q = torch.empty(M, H * 64)
    kc = torch.full((1, H, S_max, 64), float('nan'))
    vc = torch.full((1, H, S_max, 64), float('inf'))
    for s, (n, seed) in enumerate(zip(lengths, seeds)):
        qs, ks, vs, _ = _segment(n, seed)
        f = 1.0 if scale is None else scale[s]
        a = rows.starts[s]
        q[a:a + n], kc[0, :, a:a + n], vc[0, :, a:a + n] = f * qs, f * ks, f * vs
    out = torch.full((M + tail, H * 64), SENTINEL, device=DEV)
    K.attn_rows_packed(q.to(DEV), kc.to(DEV), vc.to(DEV), out[:M], H, rows)
    torch.cuda.synchronize()
    return out, M, rows.starts


@pytest.mark.parametrize('lengths', [[1], [32], [33], [128], [129], MIXED], ids=lambda v: '-'.join(map(str, v)))
def test_attn_rows_packed_matches_float64_attention_per_segment(lengths):
    from valle2_amd import kernels as K
    seeds = [100 + 3 * i for i in range(len(lengths))]
    out, M, starts = _run_packed(lengths, seeds)
    assert M == sum(lengths)
    assert bool(torch.isfinite(out[:M]).all()), 'a NaN / Inf row at or beyond M was read as a visible key'
    assert bool((out[M:] == SENTINEL).all()), 'rows of out at or beyond M must keep the sentinel'
    for s, (n, seed) in enumerate(zip(lengths, seeds)):
        q, k, v, ref = _segment(n, seed)
        got = out[starts[s]:starts[s] + n]
        torch.testing.assert_close(got.cpu(), ref, atol=3e-5, rtol=2e-5)
        # the same segment through vh_attn_rows alone (B = 1, Tq = Tk = len, full mask) on its own cache
        alone = torch.empty(n, H * 64, device=DEV)
        K.attn_rows(q.to(DEV), k[None].contiguous().to(DEV), v[None].contiguous().to(DEV), alone, 1, H, n, n, K.MASK_FULL)
        torch.testing.assert_close(got, alone, atol=3e-5, rtol=0)
        print(f'segment {s} (len {n} at row {starts[s]}): bit-equal to vh_attn_rows alone: {torch.equal(got, alone)}, '
              f'max|err| vs float64 {(got.cpu() - ref).abs().max().item():.2e}')
    again, _, _ = _run_packed(lengths, seeds)
    assert torch.equal(out, again), 'two runs of the same call must agree bit for bit'


def test_attn_rows_packed_segment_does_not_depend_on_its_neighbours():
    seeds = [100 + 3 * i for i in range(len(MIXED))]
    s = MIXED.index(129)
    out, _, starts = _run_packed(MIXED, seeds)
    scale = [1.0 if i == s else -1000.0 for i in range(len(MIXED))]
    other, _, _ = _run_packed(MIXED, seeds, scale=scale)
    a = starts[s]
    assert torch.equal(out[a:a + 129], other[a:a + 129]), 'q, K, V of the other segments x -1000 changed this segment'
    assert not torch.equal(out[:a], other[:a])                    # (the others did change)


def test_attn_rows_packed_segment_does_not_depend_on_its_offset():
    first, _, _ = _run_packed([129], [300])
    after, _, starts = _run_packed([77, 129], [400, 300])
    assert starts == [0, 77]
    assert torch.equal(first[:129], after[77:77 + 129]), 'the same segment at row 77 differs from itself at row 0'


def test_attn_rows_packed_python_wrapper_checks_shapes():
    from valle2_amd import _lib, kernels as K
    from valle2_amd.engine import PackedRows
    rows = PackedRows([5, 9], DEV)
    q = torch.zeros(14, 128, device=DEV)
    cache = torch.zeros(1, 2, 14, 64, device=DEV)
    with pytest.raises(_lib.VhError, match='q/out rows'):
        K.attn_rows_packed(q[:13], cache, cache, q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='cache'):
        K.attn_rows_packed(q, cache[:, :, :13].contiguous(), cache[:, :, :13].contiguous(), q.clone(), 2, rows)
    with pytest.raises(_lib.VhError, match='cache'):
        K.attn_rows_packed(q, cache.expand(2, -1, -1, -1).contiguous(), cache.expand(2, -1, -1, -1).contiguous(), q.clone(), 2, rows)


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', ['LayerNorm', 'AdaptiveLayerNorm'])
@pytest.mark.parametrize('lengths', [[5, 70, 129, 33], [3, 40]], ids=lambda v: '-'.join(map(str, v)))
def test_forward_packed_matches_the_padded_forward(lengths, norm):
    """[3, 40]: the padded form has 80 rows, the packed one 43 — other GEMM kernel families, where the two forms diverge."""
    from valle2_amd import kernels as K
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward, transformer_forward_packed
    from valle2_amd.modules import Transformer
    d, h = 128, 2
    cfg = C.cfg_of(dict(d_model=d, n_heads=h, dim_feedforward=256, num_layers=2, dropout=0.0, norm=norm))
    gen = g(7)
    tr = Transformer(cfg)
    sd = {k: (0.1 * torch.randn(v.shape, generator=gen) + (1.0 if k.endswith(('norm.weight', 'norm1.weight', 'norm2.weight'))
                                                            else 0.0)) for k, v in tr.state_dict().items()}
    tr.load_state_dict(sd)
    tr = tr.to(DEV).eval()
    emb = torch.randn(1, d, generator=gen).to(DEV) if norm != 'LayerNorm' else None
    B, lmax = len(lengths), max(lengths)
    rows = PackedRows(lengths, DEV)
    xs = [torch.randn(n, d, generator=gen) for n in lengths]
    padded = torch.zeros(B, lmax, d)
    for b, x in enumerate(xs):
        padded[b, :x.shape[0]] = x
    padded = padded.to(DEV)
    packed = torch.cat(xs).to(DEV)
    cache_pad = KVCache(2, B, h, lmax, DEV)
    cache_pack = KVCache(2, 1, h, rows.rows + 3, DEV)
    with torch.inference_mode():
        transformer_forward(tr, padded, cache_pad, mode=K.MASK_FULL, kv_len=torch.tensor(lengths, dtype=torch.int32, device=DEV),
                            embedding=emb)
        out = transformer_forward_packed(tr, packed, cache_pack, rows, embedding=emb)
    assert out is packed
    worst = 0.0
    for b, n in enumerate(lengths):
        a = rows.starts[b]
        pairs = [(packed[a:a + n], padded[b, :n])]
        for kv in (0, 1):                                            # the last layer's K and V rows of this utterance
            pairs.append((cache_pack.buf[1, kv, 0, :, a:a + n], cache_pad.buf[1, kv, b, :, :n]))
        for got, want in pairs:
            worst = max(worst, (got - want).abs().max().item())
            torch.testing.assert_close(got, want, atol=ATOL, rtol=RTOL)
    print(f'{norm} {lengths}: worst |packed - padded| over x and the last layer\'s K/V = {worst:.2e}')


def test_forward_packed_python_wrapper_checks_shapes():
    from valle2_amd import _lib
    from valle2_amd.engine import KVCache, PackedRows, transformer_forward_packed
    from valle2_amd.modules import Transformer
    cfg = C.cfg_of(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='LayerNorm'))
    tr = Transformer(cfg).to(DEV).eval()
    rows = PackedRows([4, 6], DEV)
    x = torch.zeros(10, 128, device=DEV)
    with pytest.raises(_lib.VhError, match='KV cache does not fit'):
        transformer_forward_packed(tr, x, KVCache(2, 2, 2, 10, DEV), rows)            # two cache rows
    with pytest.raises(_lib.VhError, match='KV cache does not fit'):
        transformer_forward_packed(tr, x, KVCache(2, 1, 2, 9, DEV), rows)             # s_max < M
    with pytest.raises(_lib.VhError, match='rows'):
        transformer_forward_packed(tr, x[:9], KVCache(2, 1, 2, 10, DEV), rows)
    with pytest.raises(_lib.VhError, match=r'\(M, d\)'):
        transformer_forward_packed(tr, x[None], KVCache(2, 1, 2, 10, DEV), rows)


# ---- model --------------------------------------------------------------------------------------------------------------
KW = dict(d_model=256, n_heads=4, dim_feedforward=1024, num_layers=3, dropout=0.0, norm='AdaptiveLayerNorm')
EXISTING = ([(15, 12, 20), (9, 30, 41), (22, 5, 7), (15, 12, 20)], 5)          # test_nar_generate_gpu's utterances
EDGES = ([(10, 40, 100), (4, 2, 1), (7, 25, 96), (3, 60, 65), (12, 20, 32)], 6)  # rows of 150, 7, 128, 128 and 64


@functools.lru_cache(maxsize=None)
def _setup(temperature=None):
    from valle2_amd import synth
    kw = dict(KW) if temperature is None else dict(KW, temperature=temperature)
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleNAR', seed=41, rich=True)
    return cfg, sd, _model(kw, sd)


def _args(us, dev=DEV):
    return [u[0].to(dev) for u in us], [u[1].to(dev) for u in us], [u[2].to(dev) for u in us]


def test_generate_packed_tokens_equal_generate_batch_and_the_oracle():
    """On these inputs the oracle's smallest top-2 margins are 1.3e-4, 2.9e-4, 5.9e-4 and 1.0e-3 (computed on the CPU): the
    padded and the alone forms already agree with it token for token, so must the packed one."""
    from oracle import valle_oracle as O
    cfg, sd, m = _setup()
    us = _utterances(cfg, *EXISTING)
    packed = m.generate_packed(*_args(us), greedy=True)
    padded = m.generate_batch(*_args(us), greedy=True)
    assert len(packed) == len(us)
    for (text, pc, first), got, pad in zip(us, packed, padded):
        ref = O.nar_generate(sd, cfg, text[:4], pc, text[4:], first, greedy=True)
        assert got.shape == ref.shape == (first.shape[0], cfg.num_quantizers) and got.dtype == torch.int64 and got.is_cuda
        assert torch.equal(got, pad), f'{(got != pad).sum().item()} tokens differ from generate_batch'
        assert torch.equal(got.cpu(), ref), f'{(got.cpu() != ref).sum().item()} of {ref.numel()} tokens differ from the oracle'
    # CPU-resident inputs are accepted and give the same result
    host = m.generate_packed(*_args(us, 'cpu'), greedy=True)
    assert all(not x.is_cuda and torch.equal(x, y.cpu()) for x, y in zip(host, packed))


def _oracle_stage_logits(sd, cfg, text, pc, codes, n):
    """The oracle's logits of stage n for one utterance alone, teacher-forced on `codes`[:, :n] (oracle.nar_generate's body)."""
    from oracle import valle_oracle as O
    q = cfg.num_quantizers
    tab = [sd[f'codes_embs.{j}.word_embeddings.weight'] for j in range(q)]
    emb_prompt = sum(O.embed(tab[j], pc[:, j]) for j in range(q))
    tokens = O.add_position(O.embed(sd['tokens_emb.word_embeddings.weight'], text.unsqueeze(0)), sd['tokens_position_emb.pe'])
    emb_out = torch.zeros(codes.shape[0], cfg.d_model)
    for j in range(n):
        emb_out = emb_out + O.embed(tab[j], codes[:, j])
    y = O.add_position(torch.cat([emb_prompt, emb_out], dim=0).unsqueeze(0), sd['audio_position_emb.pe'])
    z, _ = O.transformer(sd, 'transformer.', torch.cat([tokens, y], dim=1), cfg,
                         embedding=sd[f'stage_embs.{n - 1}.word_embeddings.weight'])
    return F.linear(z[0, text.shape[0] + pc.shape[0]:], sd[f'proj_layers.{n - 1}.weight'])


def test_generate_packed_edge_lengths_choose_a_leading_token_of_the_oracle():
    """Row lengths 150, 7, 128, 128, 64: one past a 128-query block, two exactly one block, a one-frame target.  The oracle's
    smallest top-2 margin on these inputs is 7.7e-7 and a flipped token changes every later stage, so exact equality is the
    wrong test: at EVERY frame of every stage the token the packed run chose must be within twice the summation-order bound
    of the oracle's maximum, the oracle teacher-forced on the packed run's own earlier codebooks."""
    cfg, sd, m = _setup()
    us = _utterances(cfg, *EDGES)
    assert [sum(s) for s in EDGES[0]] == [150, 7, 128, 128, 64]
    outs = m.generate_packed(*_args(us), greedy=True)
    worst = 0.0
    for (text, pc, first), got in zip(us, outs):
        got = got.cpu()
        assert got.shape == (first.shape[0], cfg.num_quantizers)
        assert torch.equal(got[:, 0], first), 'column 0 is the given first layer'
        assert int(got.min()) >= 0 and int(got.max()) < cfg.num_audio_tokens
        for n in range(1, cfg.num_quantizers):
            logits = _oracle_stage_logits(sd, cfg, text, pc, got, n)
            top = logits.max(dim=-1).values
            gap = top - logits.gather(1, got[:, n:n + 1]).squeeze(1)
            worst = max(worst, gap.max().item())
            bound = 2 * (ATOL + RTOL * top.abs())
            assert bool((gap <= bound).all()), \
                f'stage {n}: frame {int((gap - bound).argmax())} chose a token {gap.max().item():.2e} below the oracle\'s maximum'
    print(f'largest (max logit - logit of the chosen token) over all frames and stages: {worst:.2e}')


def test_generate_packed_per_request_sampling():
    from valle2_amd import Sampling
    cfg, sd, m = _setup()
    us = _utterances(cfg, *EXISTING)
    greedy = m.generate_packed(*_args(us), greedy=True)
    top1 = m.generate_packed(*_args(us), sampling=[Sampling(seed=50 + i, top_k=1) for i in range(len(us))])
    assert all(torch.equal(a, b) for a, b in zip(greedy, top1)), 'top_k=1 per request is the greedy result'
    us = us[:3] + [us[0]]                                          # utterances 0 and 3: identical inputs
    reqs = [Sampling(seed=7, temperature=0.9), Sampling(seed=8, temperature=1.1), Sampling(seed=9, temperature=0.9),
            Sampling(seed=10, temperature=0.9)]
    a = m.generate_packed(*_args(us), sampling=reqs)
    b = m.generate_packed(*_args(us), sampling=reqs)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the same seeds must give the same codes'
    assert not torch.equal(a[0], a[3]), 'identical inputs, different seeds'
    for (_, _, first), x in zip(us, a):
        assert torch.equal(x[:, 0].cpu(), first) and int(x.min()) >= 0 and int(x.max()) < cfg.num_audio_tokens
    with pytest.raises(ValueError, match='seed='):
        m.generate_packed(*_args(us), seed=3, sampling=reqs)


def test_generate_packed_unkeyed_sampling_follows_torch_manual_seed():
    cfg, sd, m = _setup(0.9)
    us = _utterances(cfg, *EXISTING)
    us = us[:3] + [us[0]]                                          # utterances 0 and 3: identical inputs
    torch.manual_seed(11)
    a = m.generate_packed(*_args(us))
    torch.manual_seed(11)
    b = m.generate_packed(*_args(us))
    torch.manual_seed(12)
    c = m.generate_packed(*_args(us))
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'torch.manual_seed must make sampling repeatable'
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    assert not torch.equal(a[0], a[3]), 'identical utterances draw independently (the RNG is keyed on the packed row)'
