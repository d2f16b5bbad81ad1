"""Repetition-aware sampling on the device (valle2_amd.RepetitionAware: the two reserved words of vh_row_sampling, read by
sample_step_kernel and sample_step_wide_kernel on their per-row forms).

Kernel level: single launches of kernels.sample_step(..., rs=...) over hand-made rows, for both kernels at V in {33, 1025,
2048} and the wide one at 2049 and 4096.  Every launch runs three times: with the two words zero (what the parent library
computes), with the words set through the narrow kernel and through the wide one.  A row whose rule cannot trigger must be
bit-equal to its words-zero self in everything the kernel writes; a row whose rule must trigger (its filter leaves survivors
that all stand in its history too often) must hold the float64 mirror's redraw over the same fp32 logits, its unfiltered
log-probability, and the state update of that token.

Draw margin: the redraw is asserted exactly, so the seeds are chosen on the CPU (`_seed_clear_of_boundaries`) such that u2 is
farther than MARGIN(V) from every boundary of the float64 CDF.  V * 2^-24 is the worst-case error of an fp32 running sum of V
terms; 2^-16 on top covers what else differs between the device and the mirror: expf (a few ulp per weight), the fp32
rounding of logit - max (up to 15 * 2^-24 in the exponent) and of 1 / temperature.

Model level (tests/ras_replay.py's V = 33 model, 2 layers, d_model 128): rows of every entry point against the mirror under
sampling_replay.AMBIGUOUS_CAP, graph and eager; the same request bit-equal wherever it decodes; a plain Sampling beside it
untouched; head width 128 and use_kv_cache=False through independent rows."""
import pytest
import torch

from tests import ras_replay as RR
from tests import sampling_replay as SR
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
D = 128
WIDTH = 24                      # codes row: BOS + 23 positions
INIT_SCORE = -1.5               # sum_logprobs before the launch: the kernel adds to it
LOGPROB_TOL = 1e-5              # atol = rtol: the suite's tolerance for sampler log-probabilities


def MARGIN(V):
    return V * 2.0 ** -24 + 2.0 ** -16


# ---- kernel level: the rows -------------------------------------------------------------------------------------------------
def _seed_clear_of_boundaries(logits64, temperature, key, pos, start, want=None):
    """The first seed >= start whose redraw at (key, pos) is farther than MARGIN from every CDF boundary (and draws `want`)."""
    V = len(logits64)
    for seed in range(start, start + 20000):
        tok, near, _ = RR.redraw(logits64, temperature, RR.uniform01(seed, key, pos | RR.RAS_STREAM), MARGIN(V) / 2)
        if not near and (want is None or tok == want):
            return seed
    raise AssertionError('no seed found')


def _rows(V, seed):
    """The scenarios at vocabulary V: a list of dicts (name, logits (V,) fp32, codes (WIDTH,), pos, record 7-tuple, trigger)."""
    eos = V - 1
    g = torch.Generator().manual_seed(seed)
    rows = []

    def add(name, pos, hist, window, max_repeats, trigger, top_k=0, top_p=0.02, temperature=1.0, lift=(), bos=None, want=None):
        """hist: codes[1 .. pos - 1]; lift: ((token, how far above the row's maximum), ...)."""
        assert len(hist) == pos - 1 and pos < WIDTH
        x = (2.0 * torch.randn(V, generator=g)).float()
        top = float(x.max())
        for tok, up in lift:
            x[tok] = top + up
        codes = torch.full((WIDTH,), eos, dtype=torch.int64)
        codes[0] = eos + 1 if bos is None else bos
        codes[1:pos] = torch.tensor(hist, dtype=torch.int64)
        key = len(rows) % 3
        s = 1000 * len(rows) + 17
        if trigger:
            s = _seed_clear_of_boundaries(x.double().numpy(), temperature, key, pos, s, want)
        rows.append(dict(name=name, logits=x, codes=codes, pos=pos, trigger=trigger,
                         record=(s, key, top_k, top_p, temperature, window, max_repeats)))

    c, a, b, far = 3 % eos, 5 % eos, 11 % eos, 7 % eos
    one = ((c, 1.0),)                                             # tok_p = 0.02 then keeps c alone: the first draw is c
    low = dict(lift=((far, -40.0),))                              # `far` is 40 below the maximum: no filter keeps it
    # window set, no trigger: the history lacks every token the filter can draw — fast path and sorted path
    add('no_trigger_fast', 12, [far] * 11, 10, 0, False, top_k=5, top_p=1.0, **low)
    add('no_trigger_sorted', 12, [far] * 11, 10, 0, False, top_k=0, top_p=0.9, **low)
    # certain trigger: one survivor (sorted path), or two survivors that both fill the history (fast path)
    add('full_one_survivor', 12, [c] * 11, 10, 1, True, lift=one)
    add('full_two_survivors', 12, [a, b] * 5 + [a], 10, 1, True, top_k=2, top_p=1.0, lift=((a, 1.0), (b, 0.7)))
    add('full_temperature', 12, [c] * 11, 10, 1, True, temperature=0.8, lift=one)
    # n_c == R beside n_c == R + 1; the tokens before the window do not count
    add('count_equals_max', 12, [c] * 5 + [far, c, far, c, far, far], 6, 2, False, lift=one)
    add('count_above_max', 12, [c] * 5 + [far, c, far, c, c, far], 6, 2, True, lift=one)
    # p - 1 < K
    add('history_shorter_than_window', 3, [c, c], 10, 1, True, lift=one)
    add('history_shorter_no_trigger', 3, [c, far], 10, 1, False, lift=one)
    # the window ends exactly at position 1 / one short of it
    add('window_reaches_position_1', 5, [c, far, far, far], 4, 0, True, lift=one)
    add('window_stops_at_position_2', 5, [c, far, far, far], 3, 0, False, lift=one)
    # K = 1
    add('window_1_repeat', 6, [far, far, far, far, c], 1, 0, True, lift=one)
    add('window_1_no_repeat', 6, [c, c, c, c, far], 1, 0, False, lift=one)
    # K larger than the codes row; BOS (here holding c's id) is never counted
    add('window_beyond_the_row', 9, [far] * 7 + [c], 2 ** 31 - 1, 0, True, lift=one)
    add('bos_is_never_counted', 9, [far] * 8, 1000, 0, False, lift=one, bos=c)
    # a finished row beside live ones: EOS written, the score untouched
    add('finished', 7, [c] * 5 + [eos], 10, 0, False, lift=one)
    # a redraw that returns EOS: the filter keeps c alone, the unfiltered distribution holds EOS at about the same weight
    add('redraw_returns_eos', 8, [c] * 7, 10, 1, True, lift=((c, 1.0), (eos, 0.8)), want=eos)
    # top_k == 1 with the words set: greedy whatever else the record says
    add('greedy_ignores_the_words', 8, [c] * 7, 5, 0, False, top_k=1, top_p=0.5, temperature=3.0, lift=one)
    return rows


GROUPS = [slice(0, 8), slice(8, 15), slice(15, 18), slice(2, 3)]          # launches of 8, 7, 3 rows and 1 row
CASES = [(33, False), (1025, False), (2048, False), (33, True), (1025, True), (2048, True), (2049, True), (4096, True)]


def _launch(rows, V, wide, words):
    """One launch over `rows`; returns what the kernel wrote, on the host."""
    from valle2_amd import kernels
    B = len(rows)
    g = torch.Generator().manual_seed(V)
    emb = torch.randn(V + 1, D, generator=g).to(DEV)
    pe = torch.randn(WIDTH, D, generator=g).to(DEV)
    logits = torch.stack([r['logits'] for r in rows]).to(DEV)
    codes = torch.stack([r['codes'] for r in rows]).to(DEV)
    pos = torch.tensor([r['pos'] for r in rows], dtype=torch.int32)
    st = dict(codes=codes, eos_count=torch.zeros(WIDTH, dtype=torch.int32, device=DEV), audio_pos=pos.to(DEV),
              sum_logprobs=torch.full((B,), INIT_SCORE, device=DEV), cache_len=(pos + 2).to(DEV), x=torch.zeros(B, D, device=DEV))
    rs = kernels.pack_row_sampling([r['record'] if words else r['record'][:5] for r in rows]).to(DEV)
    kernels.sample_step(logits, V, V - 1, 0, 1.0, 1.0, 0, st['codes'], st['eos_count'], st['sum_logprobs'], emb, pe,
                        st['audio_pos'], st['cache_len'], st['x'], wide=wide, rs=rs)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in st.items()}
    out['token'] = torch.stack([out['codes'][i, r['pos']] for i, r in enumerate(rows)])
    out['x_of_token'] = (emb[out['token'].to(DEV)] + pe[pos.long().to(DEV)]).cpu()
    return out


@pytest.fixture(scope='module')
def scenes():
    made = {}

    def get(V):
        if V not in made:
            made[V] = _rows(V, 900 + V)
        return made[V]
    return get


@pytest.fixture(scope='module')
def launched(scenes):
    """(V, wide, group) -> (rows, words-zero run, words-set run), each launch made once."""
    made = {}

    def get(V, wide, group):
        if (V, wide, group) not in made:
            rows = scenes(V)[GROUPS[group]]
            made[(V, wide, group)] = (rows, _launch(rows, V, wide, False), _launch(rows, V, wide, True))
        return made[(V, wide, group)]
    return get


@pytest.mark.parametrize('group', range(len(GROUPS)))
@pytest.mark.parametrize('V,wide', CASES)
def test_rows_keep_their_draw_or_hold_the_mirrors_redraw(launched, V, wide, group):
    rows, zero, got = launched(V, wide, group)
    eos = V - 1
    want_eos_count = torch.zeros(WIDTH, dtype=torch.int32)
    for i, r in enumerate(rows):
        seed, key, top_k, top_p, temperature, window, max_repeats = r['record']
        what = f'V={V} wide={wide} row {i} ({r["name"]})'
        pos, tok = r['pos'], int(got['token'][i])
        x64 = r['logits'].double().numpy()
        first = int(zero['token'][i])
        if top_p == 0.02 and r['name'] != 'finished':
            assert first == int(x64.argmax()), f'{what}: the filter was to leave the largest logit alone'
        if r['trigger']:
            assert RR.repeats(r['codes'].tolist(), pos, window, first) > max_repeats, f'{what}: the row was to trigger'
            want, near, lp = RR.redraw(x64, temperature, RR.uniform01(seed, key, pos | RR.RAS_STREAM), MARGIN(V) / 2)
            assert not near, f'{what}: the seed was to keep u2 clear of every boundary'
            assert tok == want, f'{what}: the device drew {tok}, the mirror\'s redraw is {want} (first draw {first})'
            score = float(got['sum_logprobs'][i])
            print(f'{what}: token {tok} (first draw {first}), log-probability {score - INIT_SCORE:.6f}, float64 {lp:.6f}')
            assert abs(score - (INIT_SCORE + lp)) <= LOGPROB_TOL + LOGPROB_TOL * abs(INIT_SCORE + lp), what
            assert abs(float(zero['sum_logprobs'][i]) - score) > 0.05, f'{what}: the score was to move to the unfiltered distribution\'s'
            if r['name'] == 'redraw_returns_eos':
                assert tok == eos != first
        else:
            assert RR.repeats(r['codes'].tolist(), pos, window, first) <= max_repeats or top_k == 1 or r['name'] == 'finished', what
            assert tok == first, f'{what}: the token moved without a trigger'
            assert got['sum_logprobs'].view(torch.int32)[i] == zero['sum_logprobs'].view(torch.int32)[i], f'{what}: the score is not bit-equal'
            assert torch.equal(got['x'][i], zero['x'][i]), what
            if r['name'] == 'finished':
                assert tok == eos and float(got['sum_logprobs'][i]) == INIT_SCORE, f'{what}: EOS written, the score untouched'
            if top_k == 1:
                assert tok == int(x64.argmax()) and float(got['sum_logprobs'][i]) == INIT_SCORE, f'{what}: greedy token, score 0'
        # the state update of whatever token was written
        assert torch.equal(got['x'][i], got['x_of_token'][i]), f'{what}: x_next is not emb[token] + pe[pos]'
        assert torch.equal(got['codes'][i, :pos], r['codes'][:pos]) and torch.equal(got['codes'][i, pos + 1:], r['codes'][pos + 1:]), what
        assert int(got['audio_pos'][i]) == pos + 1 and int(got['cache_len'][i]) == pos + 3, what
        want_eos_count[pos] += tok == eos
    assert torch.equal(got['eos_count'], want_eos_count), f'V={V} wide={wide}: eos_count {got["eos_count"].tolist()}'
    if not any(r['trigger'] for r in rows):
        for k in ('codes', 'eos_count', 'sum_logprobs', 'audio_pos', 'cache_len', 'x'):
            assert torch.equal(got[k], zero[k]), k


@pytest.mark.parametrize('group', range(len(GROUPS)))
@pytest.mark.parametrize('V', [33, 1025, 2048])
def test_narrow_and_wide_kernels_agree_token_for_token(launched, V, group):
    _, _, narrow = launched(V, False, group)
    _, _, wide = launched(V, True, group)
    assert torch.equal(narrow['codes'], wide['codes']) and torch.equal(narrow['eos_count'], wide['eos_count'])
    assert torch.equal(narrow['x'], wide['x']) and torch.equal(narrow['audio_pos'], wide['audio_pos'])
    assert torch.allclose(narrow['sum_logprobs'], wide['sum_logprobs'], atol=LOGPROB_TOL, rtol=LOGPROB_TOL)


# ---- model level ------------------------------------------------------------------------------------------------------------
MAX_NEW = RR.RAS_MAX_NEW
CFG_FILTER = dict(top_k=3, temperature=1.5)      # a filter no request uses: a row that fell back to the config fails the replay


@pytest.fixture(scope='module')
def inputs():
    made = {}

    def get(width='d128', **cfg_kw):
        if width not in made:
            made[width] = RR.ras_inputs(width)
        kw, sd, utts = made[width]
        return C.cfg_of(dict(kw, **dict(CFG_FILTER, **cfg_kw))), sd, utts
    return get


def _build(cfg, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _pad(rows, width, eos):
    rows = rows.cpu()
    out = torch.full((rows.shape[0], width), eos, dtype=torch.int64)
    out[:, :min(width, rows.shape[1])] = rows[:, :width]
    return out


def _text_first(utt):
    pt, pc, tt = utt
    return torch.cat([pt, tt]), pc[:, 0]


def _batch(m, utts, requests, beams, **kw):
    """generate_batch over utterances: per utterance (rows (beams, prompt + MAX_NEW) EOS-padded, scores (beams,))."""
    texts, firsts = zip(*[_text_first(u) for u in utts])
    out = m.generate_batch([t.to(DEV) for t in texts], [f.to(DEV) for f in firsts], beams=beams, sampling=requests, **kw)
    stats = dict(m.last_generate_stats)
    assert stats['sampling'] == 'rows'
    eos = m.config.num_audio_tokens
    return [(_pad(out[g * beams:(g + 1) * beams], len(firsts[g]) + 1 + MAX_NEW, eos), stats['sum_logprobs'][g * beams:(g + 1) * beams].cpu())
            for g in range(len(utts))], stats


def _generate_rows(m, utt, req, **kw):
    """generate(): the rows its best beam was chosen from."""
    kept, inner = [], m.generate_batch
    m.generate_batch = lambda *a, **k: kept.append(inner(*a, **k)) or kept[-1]
    try:
        m.generate(*[t.to(DEV) for t in utt], sampling=req, **kw)
    finally:
        del m.generate_batch
    stats = dict(m.last_generate_stats)
    return (_pad(kept[0], utt[1].shape[0] + 1 + MAX_NEW, m.config.num_audio_tokens), stats['sum_logprobs'].cpu()), stats


def _queued(m, utts, requests, beams, slots, use_graph=True):
    on_dev = [tuple(t.to(DEV) for t in u) + (r,) for u, r in zip(utts, requests)]
    m._generate_queued(on_dev, beams, slots, use_graph=use_graph)
    stats = dict(m.last_generate_stats)
    assert stats['queued'] is True and stats['refills'] == len(utts) - slots
    eos = m.config.num_audio_tokens
    return [(_pad(stats['rows'][i], utts[i][1].shape[0] + 1 + MAX_NEW, eos), stats['sum_logprobs'][i * beams:(i + 1) * beams].cpu())
            for i in range(len(utts))], stats


def _hold(name, cfg, sd, utts, which, per_utt, keys=None):
    counted = ambiguous = redrawn = 0
    for u, (rows, _) in zip(which, per_utt):
        text, first = _text_first(utts[u])
        c, a, r = RR.replay_rows(sd, cfg, text, rows, len(first) + 1, MAX_NEW, RR.ras_request(u), keys=keys)
        counted, ambiguous, redrawn = counted + c, ambiguous + a, redrawn + r
    print(f'{name}: {counted} counted steps, {ambiguous} ambiguous ({ambiguous / counted:.3f}), {redrawn} redrawn ({redrawn / counted:.2f})')
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted, f'{name}: {ambiguous} of {counted} counted steps are ambiguous'
    assert redrawn > 0, f'{name}: no step redrew'


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _same_rows(a, b):
    """Rows bit-equal; the scores, summed over logits that another entry point's attention kernel (one shared prompt, grouped
    prompts, a queue's slot) rounds in another order, to 1e-3 over at most 40 terms."""
    return torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], atol=1e-3, rtol=0)


@pytest.fixture(scope='module')
def runs(inputs):
    """The V = 33 model through its four entry points, graph mode, each decoded once: name -> (utterances, per_utt, stats)."""
    cfg, sd, utts = inputs(num_beams=3)
    m = _build(cfg, sd)
    req = [RR.ras_request(u) for u in range(3)]
    out = {}
    torch.manual_seed(0)
    one, stats = _generate_rows(m, utts[0], req[0])
    assert stats['shared_prompt'] is True and stats['repetition_aware'] is True
    out['generate'] = ([0], [one], stats)
    per, stats = _batch(m, utts, req, 3)
    assert stats['grouped_shared'] is True and stats['repetition_aware'] is True
    out['generate_batch'] = ([0, 1, 2], per, stats)
    from valle2_amd.utils import get_best_beam
    returned = m.generate_many([tuple(t.to(DEV) for t in utts[u]) + (req[u],) for u in (2, 0)], beams=3)
    many_stats = dict(m.last_generate_stats)
    per, stats = _batch(m, [utts[2], utts[0]], [req[2], req[0]], 3)                # the rows generate_many chose from
    assert torch.equal(many_stats['sum_logprobs'].cpu(), stats['sum_logprobs'].cpu()) and many_stats['repetition_aware'] is True
    for got, (rows, sc), u in zip(returned, per, (2, 0)):
        pl = utts[u][1].shape[0] + 1
        best = get_best_beam(rows, sc, cfg.num_audio_tokens, cfg.length_penalty)[pl:]
        assert torch.equal(got.cpu(), best[best != cfg.num_audio_tokens]), 'generate_many did not return the best of its rows'
    out['generate_many'] = ([2, 0], per, many_stats)
    order = [1, 2, 0]                                              # two slots: utterance 0 decodes in a refilled slot
    per, stats = _queued(m, [utts[u] for u in order], [req[u] for u in order], 3, 2)
    assert stats['repetition_aware'] is True
    out['generate_queued'] = (order, per, stats)
    return m, cfg, sd, utts, req, out


@pytest.mark.parametrize('name', ['generate', 'generate_batch', 'generate_many', 'generate_queued'])
def test_rows_of_every_entry_point_are_the_mirrors(runs, name):
    m, cfg, sd, utts, req, out = runs
    which, per_utt, _ = out[name]
    _hold(name, cfg, sd, utts, which, per_utt)


def test_eager_steps_decode_the_graphs_rows(runs):
    m, cfg, sd, utts, req, out = runs
    eager, _ = _batch(m, utts, req, 3, use_graph=False)
    _hold('generate_batch eager', cfg, sd, utts, [0, 1, 2], eager)
    for u in range(3):
        assert _same(eager[u], out['generate_batch'][1][u]), f'utterance {u}: eager steps differ from the graph'
    order = [1, 2, 0]
    queued, _ = _queued(m, [utts[u] for u in order], [req[u] for u in order], 3, 2, use_graph=False)
    for at, u in enumerate(order):
        assert _same(queued[at], out['generate_queued'][1][at]), f'utterance {u}: the eager queue differs from the graph'


def test_a_request_decodes_the_same_rows_wherever_it_stands(runs):
    m, cfg, sd, utts, req, out = runs
    base = out['generate_batch'][1]                                # utterance u at group u
    assert _same_rows(out['generate'][1][0], base[0]), 'generate() against generate_batch(beams=3)'
    many = dict(zip(*out['generate_many'][:2]))
    assert _same_rows(many[0], base[0]) and _same_rows(many[2], base[2]), 'generate_many at another group index'
    queued = dict(zip(*out['generate_queued'][:2]))
    for u in range(3):
        assert _same_rows(queued[u], base[u]), f'utterance {u} in the queue (utterance 0 in a refilled slot)'
    torch.manual_seed(4321)
    again, _ = _batch(m, utts, req, 3)
    for u in range(3):
        assert _same(again[u], base[u]), 'another torch.manual_seed'
    assert len({tuple(r.tolist()) for r in base[0][0]}) == 3, 'the beams of a request differ'


def test_perf_mode_repeats_itself(inputs):
    cfg, sd, utts = inputs(num_beams=3)
    m = _build(cfg, sd)
    got = []
    for seed in (0, 99):
        torch.manual_seed(seed)
        one, stats = _generate_rows(m, utts[1], RR.ras_request(1), perf_mode=True)
        assert stats['kv_bf16'] is True and stats['repetition_aware'] is True
        got.append(one)
    assert _same(got[0], got[1])


def test_a_plain_request_beside_a_repetition_aware_one_keeps_its_rows(runs):
    from valle2_amd import Sampling
    m, cfg, sd, utts, req, out = runs
    plain = Sampling(req[1].seed, top_k=req[1].top_k, tok_p=1.0, temperature=req[1].temperature)
    other = Sampling(99, top_k=8, tok_p=1.0, temperature=1.0)
    alone, stats = _batch(m, [utts[0], utts[1]], [other, plain], 3)
    assert stats['repetition_aware'] is False
    mixed, stats = _batch(m, [utts[0], utts[1]], [req[0], plain], 3)
    assert stats['repetition_aware'] is True
    assert _same(mixed[1], alone[1]), 'the plain request\'s rows moved with its neighbour'
    assert _same(mixed[0], out['generate_batch'][1][0])
    assert not torch.equal(mixed[1][0], out['generate_batch'][1][1][0]), 'the rule changed nothing for the same seed and filter'


def test_head_width_128_through_independent_rows(inputs):
    cfg, sd, utts = inputs('w128')
    m = _build(cfg, sd)
    from valle2_amd import sampling as S
    text, first = _text_first(utts[0])
    rows = m.generate_batch([text.to(DEV)] * 3, [first.to(DEV)] * 3, sampling=S.beam_rows(RR.ras_request(0), 3))
    stats = m.last_generate_stats
    assert stats['grouped_shared'] is False and stats['repetition_aware'] is True and stats['kv_cache'] is True
    _hold('head width 128', cfg, sd, utts, [0], [(_pad(rows, len(first) + 1 + MAX_NEW, cfg.num_audio_tokens), None)])


def test_use_kv_cache_false_through_independent_rows(inputs, runs):
    cfg, sd, utts = inputs(use_kv_cache=False)
    m = _build(cfg, sd)
    from valle2_amd import sampling as S
    text, first = _text_first(utts[2])
    rows = m.generate_batch([text.to(DEV)] * 3, [first.to(DEV)] * 3, sampling=S.beam_rows(RR.ras_request(2), 3))
    stats = m.last_generate_stats
    assert stats['kv_cache'] is False and stats['repetition_aware'] is True
    _hold('use_kv_cache=False', cfg, sd, utts, [2], [(_pad(rows, len(first) + 1 + MAX_NEW, cfg.num_audio_tokens), None)])
