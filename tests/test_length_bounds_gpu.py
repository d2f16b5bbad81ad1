"""Per-request length bounds on the device (valle2_amd.Bounded: vh_row_limits records read by sample_step_kernel and
sample_step_wide_kernel, vh_ar_decoder_set_row_limits).

Kernel level: 12 chained launches of kernels.sample_step(..., rs=, limits=) over six rows (off, min only, max only, both,
min == max, already finished), d = 128, at V = 17 (narrow), 1025 (both kernels) and 4097 (wide), under two logit sets (EOS the
arg-max by a wide margin: without min_new a row ends at once; EOS far below everything: without max_new a row never ends) and
four filters (top_k 50 / tok_p 1; top_k 0 / tok_p 0.9; top_k 1; a RepetitionAware record whose redraw fires while EOS is
suppressed).  Every step is held against tests/bounds_replay.py over the same fp32 logits and the device's own history.

The mirror's ambiguity width: the logits are the device's own, so what differs is fp32 arithmetic — V * 2^-24 for a running sum
of V terms plus 2^-16 for expf, the rounding of logit - max and of 1 / temperature (the margin of
tests/test_repetition_sampling_gpu.py); 2 w of the mirror is that margin.  Scores: atol = rtol = 1e-5, that file's tolerance.

Identity: an all-zero array against the _rows launch, and the two _bounded symbols called with limits NULL against the _rows
symbols, bit for bit in everything the kernels write, both kernels.  Model level: the d128 audit
model, four utterances x two beams through all four entry points, graph and eager.  Queue: six greedy utterances capped at 40."""
import numpy as np
import pytest
import torch

from tests import bounds_replay as BR
from tests import oracle_runners as R
from tests import sampling_replay as SR
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
D, B, STEPS, PL = 128, 6, 12, 4          # rows start at audio position PL (BOS + 3 prompt codes)
WIDTH = PL + STEPS + 1
LOGPROB_TOL = 1e-5
LIMITS = [(0, 0), (5, 0), (0, 7), (3, 9), (6, 6), (4, 8)]      # the last row is already finished: it reads neither word
FINISHED_ROW = 5
CASES = [(17, False), (1025, False), (1025, True), (4097, True)]
FILTERS = {'top_k50': (50, 1.0, 1.0, 0, 0), 'top_p09': (0, 0.9, 1.0, 0, 0), 'greedy': (1, 1.0, 1.0, 0, 0),
           'ras': (4, 1.0, 0.8, 10, 0)}                          # top_k, tok_p, temperature, window, max_repeats


def MARGIN(V):
    return V * 2.0 ** -24 + 2.0 ** -16


class _Req:
    """What bounds_replay reads of a request."""

    def __init__(self, seed, top_k, tok_p, temperature, window, max_repeats):
        self.seed, self.top_k, self.tok_p, self.temperature = seed, top_k, tok_p, temperature
        if window:
            self.window, self.max_repeats = window, max_repeats


def _logits(V, eos_high, step, g, heads=12):
    """(B, V) fp32: a floor of values 0.01 apart in shuffled order (a hundred times the mirror's ambiguity width: the top_k
    threshold never falls between two scores it cannot tell apart) and `heads` head tokens (the same ones at every step of a
    row: tokens repeat) about 14 above it, so the floor's whole mass is below 1e-3 and few CDF boundaries matter; EOS 15 above
    the largest entry, or 20 below the smallest."""
    x = torch.stack([-0.01 * torch.randperm(V, generator=g).float() for _ in range(B)])
    heads = min(heads, V - 2)
    for b in range(B):
        idx = torch.randperm(V - 1, generator=torch.Generator().manual_seed(V + b))[:heads]
        x[b, idx] = 14.0 + torch.randn(heads, generator=g)
    x[:, V - 1] = x[:, :V - 1].max(1).values + 15.0 if eos_high else x[:, :V - 1].min(1).values - 20.0
    return x.float()


def _chain(V, wide, eos_high, filt, limits='set'):
    """12 chained launches; returns per step what the kernel left (host tensors) and the inputs."""
    from valle2_amd import kernels
    top_k, tok_p, temperature, window, max_repeats = FILTERS[filt]
    eos = V - 1
    g = torch.Generator().manual_seed(1000 * V + 7 * eos_high + len(filt))
    emb = torch.randn(V + 1, D, generator=g).to(DEV)
    pe = torch.randn(WIDTH + 1, D, generator=g).to(DEV)
    codes = torch.full((B, WIDTH), eos, dtype=torch.int64)
    codes[:, 0] = eos + 1
    codes[:, 1:PL] = torch.randint(0, eos, (B, PL - 1), generator=g)
    codes[FINISHED_ROW, PL - 1] = eos
    recs = [(31 + 1000 * b, b % 3, top_k, tok_p, temperature) + ((window, max_repeats) if window else ()) for b in range(B)]
    st = dict(codes=codes.to(DEV), eos_count=torch.zeros(WIDTH + 1, dtype=torch.int32, device=DEV),
              audio_pos=torch.full((B,), PL, dtype=torch.int32, device=DEV), sum_logprobs=torch.zeros(B, device=DEV),
              cache_len=torch.full((B,), PL + 2, dtype=torch.int32, device=DEV), x=torch.zeros(B, D, device=DEV))
    pos_base = torch.full((B,), PL, dtype=torch.int32, device=DEV)
    rs = kernels.pack_row_sampling(recs).to(DEV)
    lim = {'set': LIMITS, 'zero': [(0, 0)] * B, 'none': None}[limits]
    lim_dev = None if lim is None else kernels.pack_row_limits(lim).to(DEV)
    steps, all_logits = [], []
    for s in range(STEPS):
        logits = _logits(V, eos_high, s, g, heads=3 if window else 12)     # (three heads: a repeat within a few steps)
        all_logits.append(logits)
        kernels.sample_step(logits.to(DEV), V, eos, 0, 1.0, 1.0, 0, st['codes'], st['eos_count'], st['sum_logprobs'], emb, pe,
                            st['audio_pos'], st['cache_len'], st['x'], pos_base=pos_base, wide=wide, rs=rs, limits=lim_dev)
        torch.cuda.synchronize()
        steps.append({k: v.cpu().clone() for k, v in st.items()})
    return dict(steps=steps, logits=all_logits, recs=recs, codes0=codes, emb=emb.cpu(), pe=pe.cpu())


@pytest.fixture(scope='module')
def chains():
    made = {}

    def get(*key):
        if key not in made:
            made[key] = _chain(*key)
        return made[key]
    return get


@pytest.mark.parametrize('filt', list(FILTERS))
@pytest.mark.parametrize('eos_high', [True, False])
@pytest.mark.parametrize('V,wide', CASES)
def test_chained_steps_hold_the_mirror_and_the_bounds(chains, V, wide, eos_high, filt):
    run = chains(V, wide, eos_high, filt)
    eos, what = V - 1, f'V={V} wide={wide} eos_high={eos_high} {filt}'
    final = run['steps'][-1]['codes']
    counted = ambiguous = suppressed = forced = redrawn_suppressed = 0
    for b in range(B):
        seed, key, top_k, tok_p, temperature, *ras = run['recs'][b]
        req = _Req(seed, top_k, tok_p, temperature, *(ras or (0, 0)))
        delta = temperature * MARGIN(V) / 2
        min_new, max_new = LIMITS[b]
        score, score_ok = 0.0, True
        for s in range(STEPS):
            pos, hist = PL + s, final[b].tolist()
            got = hist[pos]
            before = float(run['steps'][s - 1]['sum_logprobs'][b]) if s else 0.0
            after = float(run['steps'][s]['sum_logprobs'][b])
            want, case, re, amb, cands, lp = BR.mirror_step_bounded(run['logits'][s][b].double().numpy(), hist, req, key, pos, PL, delta,
                                                                    eos, limits=LIMITS[b])
            where = f'{what} row {b} {LIMITS[b]} step {s} ({case})'
            if case == BR.FINISHED:
                assert got == eos and after == before, f'{where}: a finished row writes EOS and keeps its score'
                continue
            counted, ambiguous = counted + 1, ambiguous + amb
            assert got == want or (amb and got in cands), f'{where}: the device drew {got}, the mirror {want} (candidates {sorted(cands)})'
            if case == BR.SUPPRESSED:
                suppressed += 1
                redrawn_suppressed += re
                assert got != eos, f'{where}: EOS while n < min_new'
            if case == BR.FORCED:
                forced += 1
                assert got == eos and s == max_new, f'{where}: EOS exactly at n == max_new'
                assert np.float32(after).view(np.int32) == np.float32(before).view(np.int32), f'{where}: the score moved on a forced step'
            elif got == want and score_ok:
                score += lp
                print(f'{where}: token {got}, score {after:.6f}, float64 {score:.6f}')
                assert abs(after - score) <= LOGPROB_TOL + LOGPROB_TOL * abs(score), f'{where}: score {after} against {score}'
            else:
                score_ok = False                                   # an excused token: the mirror's sum no longer follows the row
            assert torch.equal(run['steps'][s]['x'][b], run['emb'][got] + run['pe'][pos]), f'{where}: x_next is not emb[token] + pe[pos]'
        n_tokens = next((i for i, t in enumerate(final[b, PL:PL + STEPS].tolist()) if t == eos), STEPS)
        if b != FINISHED_ROW:
            assert n_tokens >= min(min_new, STEPS) and (max_new == 0 or n_tokens <= max_new), f'{what} row {b}: {n_tokens} tokens, bounds {LIMITS[b]}'
            if eos_high and top_k != 0:
                assert n_tokens == min_new, f'{what} row {b}: EOS dominates, the row ends where min_new lets it'
            if not eos_high:
                assert n_tokens == (max_new or STEPS), f'{what} row {b}: EOS is out of reach, only max_new ends the row'
        assert int(run['steps'][-1]['audio_pos'][b]) == PL + STEPS and int(run['steps'][-1]['cache_len'][b]) == PL + 2 + STEPS
    want_count = torch.zeros(WIDTH + 1, dtype=torch.int32)
    for s in range(STEPS):
        want_count[s] = int((final[:, PL + s] == eos).sum())
    assert torch.equal(run['steps'][-1]['eos_count'], want_count), f'{what}: eos_count'
    print(f'{what}: {counted} counted, {ambiguous} ambiguous, {suppressed} suppressed, {forced} forced, {redrawn_suppressed} redrawn under suppression')
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted, f'{what}: {ambiguous} of {counted} steps ambiguous'
    assert suppressed > 0 and (eos_high or forced > 0)
    if filt == 'ras' and eos_high:
        assert redrawn_suppressed > 0, f'{what}: no redraw fired under suppression'


@pytest.mark.parametrize('filt', ['top_k50', 'top_p09', 'ras'])
@pytest.mark.parametrize('V,wide', [(1025, False), (1025, True), (4097, True)])
def test_null_and_all_zero_limits_are_the_rows_launch_bit_for_bit(chains, V, wide, filt):
    """The all-zero array against the `_rows` launch (kernels.sample_step without limits takes the `_rows` symbols; the
    `_bounded` symbols with NULL are held against them in the next test)."""
    base = chains(V, wide, False, filt, 'none')
    zero = chains(V, wide, False, filt, 'zero')
    for s in range(STEPS):
        for k in ('codes', 'eos_count', 'audio_pos', 'cache_len', 'x'):
            assert torch.equal(base['steps'][s][k], zero['steps'][s][k]), f'step {s}: {k}'
        assert torch.equal(base['steps'][s]['sum_logprobs'].view(torch.int32), zero['steps'][s]['sum_logprobs'].view(torch.int32))


@pytest.mark.parametrize('filt', ['top_k50', 'top_p09', 'greedy', 'ras'])
@pytest.mark.parametrize('V,wide', [(17, False), (1025, False), (1025, True), (4097, True)])
def test_the_bounded_symbols_with_null_limits_are_the_rows_launch_bit_for_bit(V, wide, filt):
    """vh_sample_step_rows_bounded / vh_sample_step_wide_rows_bounded called themselves (through ctypes: kernels.sample_step
    reaches them only with an array) with limits == NULL, against vh_sample_step_rows / vh_sample_step_wide_rows: six chained
    launches, everything the kernel writes compared after each."""
    from valle2_amd import _lib, kernels
    from valle2_amd._lib import ptr, stream
    top_k, tok_p, temperature, window, max_repeats = FILTERS[filt]
    eos, steps = V - 1, 6
    g = torch.Generator().manual_seed(77 + V)
    emb, pe = torch.randn(V + 1, D, generator=g).to(DEV), torch.randn(WIDTH, D, generator=g).to(DEV)
    logits = [_logits(V, s == 3, s, g, heads=3 if window else 12).to(DEV) for s in range(steps)]     # (step 3: EOS dominates, rows finish)
    codes0 = torch.full((B, WIDTH), eos, dtype=torch.int64)
    codes0[:, 0] = eos + 1
    codes0[:, 1:PL] = torch.randint(0, eos, (B, PL - 1), generator=g)
    rs = kernels.pack_row_sampling([(5 + 100 * b, b % 3, top_k, tok_p, temperature) + ((window, max_repeats) if window else ())
                                    for b in range(B)]).to(DEV)
    pos_base = torch.full((B,), PL, dtype=torch.int32, device=DEV)
    name = 'vh_sample_step_wide_rows' if wide else 'vh_sample_step_rows'

    def run(bounded):
        st = dict(codes=codes0.to(DEV), eos_count=torch.zeros(WIDTH + 1, dtype=torch.int32, device=DEV),
                  sum_logprobs=torch.zeros(B, device=DEV), audio_pos=torch.full((B,), PL, dtype=torch.int32, device=DEV),
                  cache_len=torch.full((B,), PL + 2, dtype=torch.int32, device=DEV), x=torch.zeros(B, D, device=DEV))
        left = []
        for s in range(steps):
            head = (logits[s].data_ptr(), logits[s].stride(0), V, eos, ptr(rs))
            tail = (ptr(st['codes']), st['codes'].stride(0), ptr(st['eos_count']), ptr(pos_base), ptr(st['sum_logprobs']), ptr(emb),
                    ptr(pe), ptr(st['audio_pos']), ptr(st['cache_len']), ptr(st['x']), B, D, stream())
            rc = getattr(_lib.lib(), name + '_bounded')(*head, None, *tail) if bounded else getattr(_lib.lib(), name)(*head, *tail)
            assert rc == 0, _lib.lib().vh_last_error()
            torch.cuda.synchronize()
            left.append({k: v.cpu().clone() for k, v in st.items()})
        return left

    rows, null = run(False), run(True)
    for s in range(steps):
        for k in ('codes', 'eos_count', 'audio_pos', 'cache_len', 'x'):
            assert torch.equal(rows[s][k], null[s][k]), f'step {s}: {k}'
        assert torch.equal(rows[s]['sum_logprobs'].view(torch.int32), null[s]['sum_logprobs'].view(torch.int32)), f'step {s}: sum_logprobs'
    assert (rows[-1]['codes'][:, PL + 3] == eos).any() and (rows[-1]['codes'][:, PL:PL + 3] != eos).all(), 'rows were to run and then finish'
    # limits == NULL does not ask for pos_base either
    keep = [codes0.to(DEV), torch.zeros(WIDTH + 1, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV),
            torch.full((B,), PL, dtype=torch.int32, device=DEV), torch.full((B,), PL, dtype=torch.int32, device=DEV),
            torch.zeros(B, D, device=DEV)]                          # (held until the launch has finished)
    tail = (ptr(keep[0]), WIDTH, ptr(keep[1]), None, ptr(keep[2]), ptr(emb), ptr(pe), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]), B, D, stream())
    assert getattr(_lib.lib(), name + '_bounded')(logits[0].data_ptr(), logits[0].stride(0), V, eos, ptr(rs), None, *tail) == 0
    torch.cuda.synchronize()
    assert (keep[3].cpu() == PL + 1).all()


def test_the_entry_points_refuse_limits_without_pos_base_or_a_second_token():
    from valle2_amd import _lib, kernels
    V = 17
    emb, pe = torch.zeros(V + 1, D, device=DEV), torch.zeros(WIDTH, D, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    args = lambda V: (torch.zeros(1, 20, device=DEV), V, V - 1, 0, 1.0, 1.0, 0, torch.zeros(1, WIDTH, dtype=torch.int64, device=DEV),   # noqa: E731
                      torch.zeros(WIDTH, **i32), torch.zeros(1, device=DEV), emb, pe, torch.ones(1, **i32), torch.ones(1, **i32),
                      torch.zeros(1, D, device=DEV))
    rs = kernels.pack_row_sampling([(1, 0, 0, 1.0, 1.0)]).to(DEV)
    lim = kernels.pack_row_limits([(1, 2)]).to(DEV)
    with pytest.raises(_lib.VhError, match='pos_base'):
        kernels.sample_step(*args(V), rs=rs, limits=lim)
    with pytest.raises(_lib.VhError, match='V >= 2'):
        kernels.sample_step(*args(1), pos_base=torch.ones(1, **i32), rs=rs, limits=lim)
    torch.cuda.synchronize()


# ---- model level ------------------------------------------------------------------------------------------------------------
MAX_NEW = R.AUDIT_MAX_NEW
CFG_FILTER = dict(top_k=3, temperature=1.5)      # a filter no request uses: a row that fell back to the config fails the replay
N_UTTS = 4


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
    texts, firsts = zip(*[_text_first(u) for u in utts])
    out = m.generate_batch([t.to(DEV) for t in texts], [f.to(DEV) for f in firsts], beams=beams, sampling=requests, **kw)
    stats = dict(m.last_generate_stats)
    eos = m.config.num_audio_tokens
    return [(_pad(out[g * beams:(g + 1) * beams], len(firsts[g]) + 1 + MAX_NEW, eos), stats['sum_logprobs'][g * beams:(g + 1) * beams].cpu())
            for g in range(len(utts))], stats


def _generate_rows(m, utt, req, **kw):
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
    assert stats['queued'] is True
    eos = m.config.num_audio_tokens
    return [(_pad(stats['rows'][i], utts[i][1].shape[0] + 1 + MAX_NEW, eos), stats['sum_logprobs'][i * beams:(i + 1) * beams].cpu())
            for i in range(len(utts))], stats


def _same_rows(a, b):
    """Rows bit-equal; scores to 1e-3 (another entry point's attention kernel rounds the logits in another order)."""
    return torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], atol=1e-3, rtol=0)


def _within(rows, pl, req, eos):
    lo, hi = BR.limits_of(req)
    for r in rows:
        gen = r[pl:pl + MAX_NEW].tolist()
        n = next((i for i, t in enumerate(gen) if t == eos), MAX_NEW)
        assert n >= lo and (hi == 0 or n <= hi), f'a row of {n} tokens under bounds {(lo, hi)}'


@pytest.fixture(scope='module')
def runs():
    kw, sd, utts = R.audit_inputs('d128')
    cfg = C.cfg_of(dict(kw, num_beams=BR.BOUNDS_BEAMS, **CFG_FILTER))
    utts = utts[:N_UTTS]
    m = _build(cfg, sd)
    req = [BR.bounds_request(u) for u in range(N_UTTS)]
    nb = BR.BOUNDS_BEAMS
    out = {}
    per, stats = _batch(m, utts, req, nb)
    assert stats['grouped_shared'] is True and stats['bounded'] is True and stats['sampling'] == 'rows'
    out['generate_batch'] = (list(range(N_UTTS)), per)
    out['generate'] = (list(range(N_UTTS)), [_generate_rows(m, utts[u], req[u])[0] for u in range(N_UTTS)])
    m.generate_many([tuple(t.to(DEV) for t in utts[u]) + (req[u],) for u in (2, 0, 3, 1)], beams=nb)
    assert m.last_generate_stats['bounded'] is True
    per, _ = _batch(m, [utts[u] for u in (2, 0, 3, 1)], [req[u] for u in (2, 0, 3, 1)], nb)       # the rows generate_many chose from
    out['generate_many'] = ([2, 0, 3, 1], per)
    order = [1, 3, 2, 0]                                           # two slots: utterances 2 and 0 decode in refilled slots
    per, stats = _queued(m, [utts[u] for u in order], [req[u] for u in order], nb, 2)
    assert stats['bounded'] is True and stats['refills'] == 2
    out['generate_queued'] = (order, per)
    return m, cfg, sd, utts, req, out


@pytest.mark.parametrize('name', ['generate', 'generate_batch', 'generate_many', 'generate_queued'])
def test_rows_of_every_entry_point_hold_the_mirror_and_their_bounds(runs, name):
    m, cfg, sd, utts, req, out = runs
    which, per_utt = out[name]
    counted = ambiguous = forced = 0
    for u, (rows, _) in zip(which, per_utt):
        text, first = _text_first(utts[u])
        _within(rows, len(first) + 1, req[u], cfg.num_audio_tokens)
        c, a, _, f = BR.replay_rows(sd, cfg, text, rows, len(first) + 1, MAX_NEW, req[u])
        counted, ambiguous, forced = counted + c, ambiguous + a, forced + f
    print(f'{name}: {counted} counted steps, {ambiguous} ambiguous, {forced} forced')
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted and forced > 0


def test_a_request_decodes_the_same_rows_from_every_entry_point(runs):
    m, cfg, sd, utts, req, out = runs
    base = out['generate_batch'][1]
    for name in ('generate', 'generate_many', 'generate_queued'):
        got = dict(zip(*out[name]))
        for u in range(N_UTTS):
            assert _same_rows(got[u], base[u]), f'utterance {u}: {name} against generate_batch(beams=2)'


def test_eager_steps_decode_the_graphs_rows(runs):
    m, cfg, sd, utts, req, out = runs
    eager, _ = _batch(m, utts, req, BR.BOUNDS_BEAMS, use_graph=False)
    for u in range(N_UTTS):
        assert torch.equal(eager[u][0], out['generate_batch'][1][u][0]) and torch.equal(eager[u][1], out['generate_batch'][1][u][1])
    order = out['generate_queued'][0]
    queued, _ = _queued(m, [utts[u] for u in order], [req[u] for u in order], BR.BOUNDS_BEAMS, 2, use_graph=False)
    for at in range(N_UTTS):
        assert torch.equal(queued[at][0], out['generate_queued'][1][at][0]), f'utterance {order[at]}: the eager queue differs'


def test_plain_and_repetition_aware_requests_keep_their_rows_beside_bounded_ones(runs):
    from valle2_amd import Bounded
    m, cfg, sd, utts, req, out = runs
    assert not isinstance(req[3], Bounded) and isinstance(req[2], Bounded)
    plain = [r.request if isinstance(r, Bounded) else r for r in req]
    alone, stats = _batch(m, utts, plain, BR.BOUNDS_BEAMS)
    assert stats['bounded'] is False
    base = out['generate_batch'][1]
    assert torch.equal(alone[3][0], base[3][0]) and torch.equal(alone[3][1], base[3][1]), 'the plain request moved with its neighbours'
    assert not torch.equal(alone[0][0], base[0][0]) or not torch.equal(alone[1][0], base[1][0]), 'the bounds changed no row'


def test_perf_mode_generate_stays_within_its_bounds(runs):
    from valle2_amd import Bounded, Sampling
    m, cfg, sd, utts, req, out = runs
    r = Bounded(Sampling(5, top_k=8, tok_p=1.0, temperature=1.0), min_new=15, max_new=18)
    (rows, _), stats = _generate_rows(m, utts[1], r, perf_mode=True)
    assert stats['kv_bf16'] is True and stats['bounded'] is True
    _within(rows, utts[1][1].shape[0] + 1, r, cfg.num_audio_tokens)


def test_limits_cannot_be_set_after_capture(runs):
    from valle2_amd import _lib, kernels
    m, cfg, sd, utts, req, out = runs
    _batch(m, utts[:1], req[:1], BR.BOUNDS_BEAMS)                   # a bounded call: its decoder stays in a slot, captured
    slot = next(s for s in m._decode_slots.values()
                if s.dec is not None and s.row_limits is not None and getattr(s.dec, '_captured', False))
    for limits in (kernels.ptr(slot.row_limits), None):             # neither another array nor clearing it: the graphs hold the pointer
        rc = _lib.lib().vh_ar_decoder_set_row_limits(slot.dec._h, limits)
        assert rc == -5 and b'capture' in _lib.lib().vh_last_error()      # VH_ESTATE


# ---- the queue --------------------------------------------------------------------------------------------------------------
def test_capped_greedy_utterances_free_their_slots():
    from valle2_amd import Bounded, Sampling, engine
    from valle2_amd.generation import EOS_POLL
    kw, sd, utts = R.audit_inputs('d128')
    cfg = C.cfg_of(dict(kw, num_beams=1, max_audio_len=96, **CFG_FILTER))
    m = _build(cfg, sd)
    six = [utts[i % len(utts)] for i in range(6)]
    steps, lengths = {}, {}
    for name, wrap in (('plain', lambda s: s), ('capped', lambda s: Bounded(s, max_new=40))):
        reqs = [wrap(Sampling(100 + i, top_k=1)) for i in range(6)]
        m._generate_queued([tuple(t.to(DEV) for t in u) + (r,) for u, r in zip(six, reqs)], 1, 2)
        st = dict(m.last_generate_stats)
        assert st['queued'] is True and st['bounded'] is (name == 'capped')
        eos = cfg.num_audio_tokens
        lengths[name] = []
        for u, rows in zip(six, st['rows']):
            gen = rows[0, u[1].shape[0] + 1:].tolist()
            lengths[name].append(next((i for i, t in enumerate(gen) if t == eos), len(gen)) + 1)     # tokens written up to and including EOS
        steps[name] = st['steps']
        assert st['steps'] == engine.plan_queue(lengths[name], 2, EOS_POLL, cfg.max_audio_len)[1], f'{name}: {st["steps"]} steps, lengths {lengths[name]}'
    print(f'decode steps: plain {steps["plain"]} (lengths {lengths["plain"]}), capped {steps["capped"]} (lengths {lengths["capped"]})')
    assert all(n <= 41 for n in lengths['capped'])
    assert steps['capped'] < steps['plain']
