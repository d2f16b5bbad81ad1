"""Grouped shared-prompt decoding: G utterances with different texts and prompts, each replicated over `beams` rows whose
prompt K/V are read once per decode step for the group (vh_attn_decode_shared_groups).  The kernel against float64 softmax
attention, ValleAR.generate_batch(beams=n) / generate_many against the CPU oracle, this model's own generate() and the real
reference's tokens, EOS, decoder slots keyed on the prefix capacity, sampling, chunking and codec_io.synthesize_many."""
import pytest
import torch

from tests.golden import cases as C
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 1e-4


# ---- kernel -------------------------------------------------------------------------------------------------------------
KERNEL_CASES = {                                   # (G, beams, h, prefix lengths, n_split)
    'three_groups': (3, 4, 2, [1, 33, 100], 1),
    'second_lane_pass': (2, 33, 2, [31, 70], 2),
    '64_rows': (16, 4, 1, [7 * (i + 1) for i in range(16)], 3),
    'one_group': (1, 5, 2, [64], 1),
    'no_sharing': (4, 1, 2, [5, 32, 96, 97], 2),
    'long_merge_loop': (2, 4, 2, [2651, 40], 3),
}


def _kernel_case(name):
    """Inputs with NaN (K) / Inf (V) beyond every length, and the float64 reference over each row's own keys."""
    G, beams, h, plens, n_split = KERNEL_CASES[name]
    B, d, S_suf = G * beams, 64 * h, 96
    cap = max(plens)
    prefix_S = (cap + 31) // 32 * 32 + 32
    gen = torch.Generator().manual_seed(900 + sum(plens) + B)
    q = torch.randn(B, d, generator=gen)
    kp = torch.randn(G, h, prefix_S, 64, generator=gen)
    vp = torch.randn(G, h, prefix_S, 64, generator=gen)
    ks = torch.randn(B, h, S_suf, 64, generator=gen)
    vs = torch.randn(B, h, S_suf, 64, generator=gen)
    slen = torch.tensor([(7 * i) % 90 for i in range(B)], dtype=torch.int32)          # rows in the suffix BEFORE the new one
    ref = torch.empty(B, d, dtype=torch.float64)
    for b in range(B):
        n, grp = int(slen[b]) + 1, b // beams
        kk = torch.cat([kp[grp, :, :plens[grp]], ks[b, :, :n]], dim=1).double()
        vv = torch.cat([vp[grp, :, :plens[grp]], vs[b, :, :n]], dim=1).double()
        s = (q[b].double().view(h, 1, 64) @ kk.transpose(-1, -2)) / 8.0
        ref[b] = (torch.softmax(s, dim=-1) @ vv).reshape(d)
        ks[b, :, n:] = float('nan')
        vs[b, :, n:] = float('inf')
    for grp in range(G):
        kp[grp, :, plens[grp]:] = float('nan')
        vp[grp, :, plens[grp]:] = float('inf')
    dev = [t.to(DEV) for t in (q, kp, vp, ks, vs, slen)]
    return (G, beams, h, plens, n_split, cap), dev, ref


@pytest.mark.parametrize('name', sorted(KERNEL_CASES))
def test_attn_decode_shared_groups_matches_float64_softmax(name):
    from valle2_amd import kernels as K
    (G, beams, h, plens, n_split, cap), (q, kp, vp, ks, vs, slen), ref = _kernel_case(name)
    B = G * beams
    plen_dev = torch.tensor(plens, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        ws = K.attn_decode_shared_groups_ws(B, h, cap, n_split, DEV)
        ws.fill_(float('nan'))                                 # the workspace needs no initialisation: whatever it holds
        out = torch.full((B, 64 * h), float('nan'), device=DEV)
        K.attn_decode_shared_groups(q, kp, vp, plen_dev, cap, ks, vs, out, slen, 1, beams, n_split=n_split, partial=ws)
        outs.append(out)
    assert bool(torch.isfinite(outs[0]).all()), 'garbage beyond a length or in the workspace leaked into the attention output'
    err = (outs[0].cpu().double() - ref).abs().max().item()
    print(f'{name}: max |err| vs float64 = {err:.3e}')
    torch.testing.assert_close(outs[0].cpu().double(), ref, atol=2e-5, rtol=0)
    assert torch.equal(outs[0], outs[1]), 'the merge must be deterministic'
    if G == 1:
        one = torch.empty_like(outs[0])
        K.attn_decode_shared(q, kp, vp, plens[0], ks, vs, one, slen, 1, n_split=n_split)
        torch.testing.assert_close(outs[0], one, atol=1e-6, rtol=0)


def test_capacity_beyond_the_lengths_and_len_bias_0():
    """A capacity far beyond every length (the slot's rounded-up capacity: whole workgroups without a record) and
    len_bias = 0 (a row whose own cache holds nothing attends its prompt alone)."""
    from valle2_amd import kernels as K
    (G, beams, h, plens, n_split, _), (q, kp, vp, ks, vs, slen), _ = _kernel_case('three_groups')
    B = G * beams
    plen_dev = torch.tensor(plens, dtype=torch.int32, device=DEV)
    tight = torch.empty(B, 64 * h, device=DEV)
    K.attn_decode_shared_groups(q, kp, vp, plen_dev, max(plens), ks, vs, tight, slen, 1, beams, n_split=n_split)
    wide_k = torch.full((G, h, 640, 64), float('nan'), device=DEV)
    wide_v = torch.full((G, h, 640, 64), float('inf'), device=DEV)
    wide_k[:, :, :kp.shape[2]], wide_v[:, :, :vp.shape[2]] = kp, vp
    ws = K.attn_decode_shared_groups_ws(B, h, 640, n_split, DEV).fill_(float('nan'))
    wide = torch.full_like(tight, float('nan'))
    K.attn_decode_shared_groups(q, wide_k, wide_v, plen_dev, 640, ks, vs, wide, slen, 1, beams, n_split=n_split, partial=ws)
    assert torch.equal(wide, tight)                            # the same records merged in the same order
    out0 = torch.full_like(tight, float('nan'))
    K.attn_decode_shared_groups(q, kp, vp, plen_dev, max(plens), ks, vs, out0, slen, 0, beams, n_split=2)
    assert bool(torch.isfinite(out0).all())
    b = 0                                                      # slen[0] == 0: the prompt's keys only
    s = (q[b].double().view(h, 1, 64).cpu() @ kp[0, :, :plens[0]].double().cpu().transpose(-1, -2)) / 8.0
    want = (torch.softmax(s, -1) @ vp[0, :, :plens[0]].double().cpu()).reshape(-1)
    torch.testing.assert_close(out0[b].cpu().double(), want, atol=2e-5, rtol=0)


# ---- model --------------------------------------------------------------------------------------------------------------
def _build(kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(kw))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _same_up_to_a_near_tie(got, want, margins):
    """Token for token, except from a step whose oracle top-2 margin is below 1e-4 (a near-tie may fall either way and
    everything after it follows)."""
    got, want = got.cpu(), want.cpu()
    n = min(len(got), len(want))
    bad = (got[:n] != want[:n]).nonzero()
    if bad.numel() == 0:
        assert len(got) == len(want), (got, want)
        return
    assert float(margins[int(bad[0])]) < MARGIN, (int(bad[0]), float(margins[int(bad[0])]), got, want)


@pytest.fixture(scope='module')
def tiny():
    """An AR_TINY-sized greedy model, three utterances of different text and prompt lengths, the oracle's tokens + margins."""
    from oracle import valle_oracle as O
    from valle2_amd import synth
    kw = dict(C.AR_TINY, num_beams=3, max_audio_len=40)
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=31, rich=True), cfg)
    utts = [synth.synth_utterance(cfg, 6 + 3 * i, 5 + 2 * i, 20 + 23 * i, seed=700 + i) for i in range(3)]
    more = [synth.synth_utterance(cfg, 4 + 5 * i, 9 - 2 * i, 70 - 21 * i, seed=750 + i) for i in range(3)]   # same capacity
    refs = []
    for u in utts + more:
        trace = {}
        refs.append((O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *u, trace=trace), trace['margin']))
    return kw, sd, utts, more, refs


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_generate_batch_beams_matches_the_oracle_and_generate(tiny, use_graph):
    kw, sd, utts, _, refs = tiny
    m = _build(kw, sd)
    texts = [torch.cat([u[0], u[2]]).to(DEV) for u in utts]
    firsts = [u[1][:, 0].to(DEV) for u in utts]
    rows = m.generate_batch(texts, firsts, use_graph=use_graph, beams=3)
    st = m.last_generate_stats
    assert st['groups'] == 3 and st['beams'] == 3 and st['grouped_shared'] is True and not st['shared_prompt']
    assert rows.shape[0] == 9 and st['prompt_lens'] == [u[1].shape[0] + 1 for u in utts for _ in range(3)]
    assert st['sum_logprobs'].shape == (9,)
    own = _build(kw, sd)
    for g, u in enumerate(utts):
        assert torch.equal(rows[3 * g], rows[3 * g + 1]) and torch.equal(rows[3 * g], rows[3 * g + 2])
        got = rows[3 * g, st['prompt_lens'][3 * g]:]
        got = got[got != m.eos_token]
        _same_up_to_a_near_tie(got, *refs[g])
        _same_up_to_a_near_tie(got, own.generate(*[t.to(DEV) for t in u]), refs[g][1])


def test_generate_many_matches_the_oracle_and_reuses_the_slot_under_one_capacity(tiny):
    from valle2_amd import engine
    kw, sd, utts, more, refs = tiny
    m = _build(kw, sd)
    outs = m.generate_many([tuple(t.to(DEV) for t in u) for u in utts])           # beams: config.num_beams = 3
    st = m.last_generate_stats
    assert st['beams'] == 3 and st['groups'] == 3 and st['grouped_shared'] is True and st['decoder_reused'] is False
    for g in range(3):
        assert outs[g].dim() == 1 and outs[g].dtype == torch.int64
        _same_up_to_a_near_tie(outs[g], *refs[g])
    # other texts and prompts, other lengths, the same capacity: the captured graphs serve them
    ctx = lambda us: max(len(u[0]) + len(u[2]) + u[1].shape[0] + 1 for u in us)
    assert ctx(more) != ctx(utts) and engine.group_prefix_cap(ctx(more)) == engine.group_prefix_cap(ctx(utts))
    outs = m.generate_many([tuple(t.to(DEV) for t in u) for u in more])
    assert m.last_generate_stats['decoder_reused'] is True
    for g in range(3):
        _same_up_to_a_near_tie(outs[g], *refs[3 + g])
    # one utterance: what generate() gives
    one = m.generate_many([tuple(t.to(DEV) for t in utts[1])])
    assert len(one) == 1
    _same_up_to_a_near_tie(one[0], m.generate(*[t.to(DEV) for t in utts[1]]), refs[1][1])


def test_the_reference_golden_utterance_beside_two_others():
    from tests.test_models_gpu import tokens_match
    from valle2_amd import synth
    gold = load_golden('ar_generate_tiny')
    kw, sd, utt = C.ar_generate_inputs('tiny')
    cfg = C.cfg_of(kw)
    others = [synth.synth_utterance(cfg, 9, 4, 30, seed=811), synth.synth_utterance(cfg, 20, 31, 140, seed=812)]
    m = _build(kw, sd)
    outs = m.generate_many([tuple(t.to(DEV) for t in u) for u in (others[0], utt, others[1])])
    assert m.last_generate_stats['grouped_shared'] is True and m.last_generate_stats['beams'] == cfg.num_beams
    tokens_match(outs[1], gold['tokens'], gold['margin'])
    assert not torch.equal(outs[0], outs[1][:len(outs[0])]) and len(outs[2]) == cfg.max_audio_len


def test_eos_one_utterance_stops_early_beside_one_that_does_not():
    from oracle import valle_oracle as O
    from valle2_amd import synth
    gold = load_golden('ar_generate_eos')
    kw, sd, utt = C.ar_eos_inputs(gold['eos_row'])
    cfg = C.cfg_of(kw)
    other = synth.synth_utterance(cfg, 20, 20, 60, seed=6)           # the planted EOS row never wins on this one
    refs = []
    for u in (utt, other):
        trace = {}
        refs.append((O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *u, trace=trace), trace['margin']))
    assert torch.equal(refs[0][0], gold['tokens']) and len(refs[0][0]) < len(refs[1][0]) == cfg.max_audio_len, 'inputs: one early stop, one none'
    m = _build(kw, sd)
    outs = m.generate_many([tuple(t.to(DEV) for t in u) for u in (utt, other)])
    for g in range(2):
        _same_up_to_a_near_tie(outs[g], *refs[g])
    assert len(outs[0]) != len(outs[1])


def test_sampling_beams_scores_seed_and_best_beam(tiny):
    from valle2_amd.utils import get_best_beam
    kw, sd, utts, _, _ = tiny
    kw = dict(kw, top_k=50, num_beams=4, max_audio_len=24)
    m = _build(kw, sd)
    two = [tuple(t.to(DEV) for t in u) for u in utts[:2]]
    texts = [torch.cat([u[0], u[2]]) for u in two]
    firsts = [u[1][:, 0] for u in two]
    runs = []
    for use_graph in (True, False, True):
        torch.manual_seed(4321)
        rows = m.generate_batch(texts, firsts, use_graph=use_graph, beams=4)
        runs.append((rows.cpu(), m.last_generate_stats['sum_logprobs'].cpu()))
    st = m.last_generate_stats
    rows, scores = runs[0]
    assert rows.shape[0] == 8 and scores.shape == (8,) and bool((scores < 0).all())
    for g in range(2):
        assert len({tuple(r.tolist()) for r in rows[4 * g:4 * g + 4]}) > 1, 'sampled beams of a group must differ'
    for other_rows, other_scores in runs[1:]:                  # eager = graph; the same seed again = the same draw
        assert torch.equal(other_rows, rows) and torch.equal(other_scores, scores)
    torch.manual_seed(4321)
    outs = m.generate_many(two)
    for g in range(2):
        sl = slice(4 * g, 4 * g + 4)
        best = get_best_beam(rows[sl], scores[sl], m.eos_token, m.config.length_penalty)[st['prompt_lens'][4 * g]:]
        assert torch.equal(outs[g].cpu(), best[best != m.eos_token])


def test_more_than_64_rows_decode_in_chunks_of_whole_utterances(tiny):
    from valle2_amd import synth
    kw, sd, utts, more, _ = tiny
    kw = dict(kw, max_audio_len=12)
    cfg = C.cfg_of(kw)
    five = [tuple(t.to(DEV) for t in u) for u in (utts + more)[:5]]
    m = _build(kw, sd)
    outs = m.generate_many(five, beams=16)                     # 80 rows: 4 utterances, then 1
    st = m.last_generate_stats
    assert st['groups'] == 5 and st['beams'] == 16 and len(st['prompt_lens']) == 80 and st['sum_logprobs'].shape == (80,)
    parts = m.generate_many(five[:3], beams=16) + m.generate_many(five[3:], beams=16)     # calls of at most 64 rows
    for a, b in zip(outs, parts):
        assert torch.equal(a, b)


def test_synthesize_many_equals_synthesize_per_utterance():
    from valle2_amd import ConfigValle, codec_io as CIO, get_model_class, synth
    base = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0)
    ar_cfg = ConfigValle(**base, norm='LayerNorm', num_beams=2, top_k=1, max_audio_len=12)
    nar_cfg = ConfigValle(**base, norm='AdaptiveLayerNorm')
    ar = get_model_class('ValleAR')(ar_cfg)
    ar.load_state_dict(synth.silence_eos(synth.make_state_dict(ar_cfg, 'ValleAR', seed=1), ar_cfg))
    nar = get_model_class('ValleNAR')(nar_cfg)
    nar.load_state_dict(synth.make_state_dict(nar_cfg, 'ValleNAR', seed=2))
    ar, nar = ar.to(DEV).eval(), nar.to(DEV).eval()
    items = []
    for i in range(2):
        pt, pc, tt = synth.synth_utterance(ar_cfg, 5 + 2 * i, 7 - i, 9 + 6 * i, seed=60 + i)
        items.append((pt.to(DEV), pc.T.contiguous().to(DEV), tt.to(DEV)))          # codec layout (Q, T)
    many = CIO.synthesize_many(ar, nar, items, greedy_nar=True)
    assert len(many) == 2
    for item, got in zip(items, many):
        assert torch.equal(got, CIO.synthesize(ar, nar, *item, greedy_nar=True))
