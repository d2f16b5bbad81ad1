"""Per-utterance sampling on the device (valle2_amd.Sampling: vh_sample_step_rows / vh_sample_step_wide_rows behind every
entry point).  An utterance that carries a Sampling draws from (its seed, the beam within it, the audio position) through its
own filter, so:

  replay      the float64 mirror (tests/sampling_replay.py) says which token every step of every row must hold, given the
              row's own history — generate(), generate_batch(beams=3), generate_many, the queue with 2 and 4 slots (refills,
              parked groups), independent rows at head width 128 and the wide sampler; graph mode everywhere and one eager
              arm per entry point.  Every utterance's scores pass audit_sampled_rows under ITS top_k and temperature.  At most
              AMBIGUOUS_CAP of a case's counted steps may be ambiguous (within AUDIT_DELTA of a boundary: one of the
              neighbouring candidates is accepted there);
  invariance  the same utterances in another order, under another torch.manual_seed, eager instead of graph: torch.equal;
  independence, a greedy request inside a sampled batch, top-p determinism, perf mode determinism.

The models' own config holds a filter no request uses (top_k 3, temperature 1.5): a row that fell back to it fails the replay.
Utterances, seeds and filters: sampling_replay.replay_request over oracle_runners.audit_inputs."""
import pytest
import torch

from tests import oracle_runners as R
from tests import sampling_replay as SR
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MAX_NEW = R.AUDIT_MAX_NEW
CFG_FILTER = dict(top_k=3, temperature=1.5)
QUEUE_ORDER = [1, 0, 2, 3, 4]          # two slots: three refills, each after a poll
DRAIN_ORDER = [4, 3, 2, 1, 0]          # four slots: one refill, the other groups park while it runs on

# case -> (entry point, model, utterances, beams, slots)
CASES = {
    'generate': ('generate', 'd128', [0], 4, None),
    'generate_batch_beams3': ('grouped', 'd128', [0, 2, 4], 3, None),
    'generate_many': ('many', 'd128', [1, 3, 4], 3, None),
    'queued_2': ('queued', 'd128', QUEUE_ORDER, 3, 2),
    'queued_2_drain': ('queued', 'd128', DRAIN_ORDER, 3, 2),
    'queued_4': ('queued', 'd128', DRAIN_ORDER, 3, 4),
    'queued_4_order': ('queued', 'd128', QUEUE_ORDER, 3, 4),
    'head_width_128': ('rows', 'w128', [0, 1, 2, 3], 1, None),
    'wide_sampler': ('grouped', 'v4096', [0, 1], 2, None),
}
EAGER = ['generate', 'generate_batch_beams3', 'generate_many', 'queued_2', 'head_width_128']


@pytest.fixture(scope='module')
def inputs():
    """(cfg, state dict, utterances) per audit model, built (and asserted peaked) once."""
    made = {}

    def get(model, **cfg_kw):
        if model not in made:
            made[model] = R.audit_inputs(model)
        kw, sd, utts = made[model]
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
    """generate_batch over utterances; returns per utterance (rows (beams, width), scores (beams,)) and the stats."""
    texts, firsts = zip(*[_text_first(u) for u in utts])
    out = m.generate_batch([t.to(DEV) for t in texts], [f.to(DEV) for f in firsts], beams=beams, sampling=requests, **kw)
    stats = dict(m.last_generate_stats)
    assert stats['sampling'] == 'rows'
    return [(out[g * beams:(g + 1) * beams].cpu(), stats['sum_logprobs'][g * beams:(g + 1) * beams].cpu()) for g in range(len(utts))], stats


def decode(name, inputs, use_graph=True):
    """Run case `name`; returns (cfg, sd, [(utterance index, rows (beams, width), scores)], stats)."""
    from valle2_amd import sampling as S
    from valle2_amd.utils import get_best_beam
    entry, model, which, beams, slots = CASES[name]
    cfg, sd, utts = inputs(model, num_beams=beams)
    eos = cfg.num_audio_tokens
    m = _build(cfg, sd)
    requests = [SR.replay_request(u) for u in which]
    on_dev = [tuple(t.to(DEV) for t in utts[u]) + (r,) for u, r in zip(which, requests)]
    torch.manual_seed(0)
    if entry == 'generate':
        (u,), (req,) = which, requests
        text, first = _text_first(utts[u])
        if use_graph:
            kept, inner = [], m.generate_batch
            m.generate_batch = lambda *a, **k: kept.append(inner(*a, **k)) or kept[-1]       # generate() returns the best beam only
            best = m.generate(*on_dev[0][:3], sampling=req)
            del m.generate_batch
            rows, stats = kept[0].cpu(), dict(m.last_generate_stats)
            scores = stats['sum_logprobs'].cpu()
            want = get_best_beam(rows, scores, eos, cfg.length_penalty)[len(first) + 1:]
            assert torch.equal(best.cpu(), want[want != eos]), 'generate() did not return the best of its rows'
        else:                                                                                   # what generate() runs, stepped eagerly
            rows = m.generate_batch([text.to(DEV)] * beams, [first.to(DEV)] * beams, shared_prompt=True, use_graph=False,
                                    sampling=S.beam_rows(req, beams)).cpu()
            stats = dict(m.last_generate_stats)
            scores = stats['sum_logprobs'].cpu()
        assert stats['shared_prompt'] is True and stats['sampling'] == 'rows'
        per_utt = [(rows, scores)]
    elif entry == 'queued':
        returned = m._generate_queued(on_dev, beams, slots, use_graph=use_graph)
        stats = dict(m.last_generate_stats)
        assert stats['queued'] is True and stats['sampling'] == 'rows'
        assert stats['refills'] == len(which) - slots >= 1, 'the case claims refills'
        if slots == 4:                                   # the one refill runs on while the groups beside it have nothing to take
            assert stats['parked_group_steps'] > 0, 'the case claims parked groups'
        per_utt = [(stats['rows'][i].cpu(), stats['sum_logprobs'][i * beams:(i + 1) * beams].cpu()) for i in range(len(which))]
        for got, (rows, sc), u in zip(returned, per_utt, which):
            pl = utts[u][1].shape[0] + 1
            best = get_best_beam(_pad(rows, pl + MAX_NEW, eos), sc, eos, cfg.length_penalty)[pl:]
            assert torch.equal(got.cpu(), best[best != eos]), 'the queue did not return the best of its rows'
    else:
        per_utt, stats = _batch(m, [utts[u] for u in which], requests, beams, use_graph=use_graph)
        assert stats['grouped_shared'] is (entry != 'rows')
        if entry == 'many' and use_graph:
            returned = m.generate_many(on_dev, beams=beams)
            assert torch.equal(m.last_generate_stats['sum_logprobs'].cpu(), torch.cat([sc for _, sc in per_utt]))
            for got, (rows, sc), u in zip(returned, per_utt, which):
                pl = utts[u][1].shape[0] + 1
                best = get_best_beam(_pad(rows, pl + MAX_NEW, eos), sc, eos, cfg.length_penalty)[pl:]
                assert torch.equal(got.cpu(), best[best != eos])
    groups = []
    for u, (rows, sc) in zip(which, per_utt):
        text, first = _text_first(utts[u])
        pl = len(first) + 1
        rows = _pad(rows, pl + MAX_NEW, eos)
        assert rows[:, 0].tolist() == [eos + 1] * len(rows) and bool((rows[:, 1:pl] == first).all()), 'a row lost its prompt'
        groups.append((u, rows, sc))
    return cfg, sd, utts, groups, stats


def check(name, cfg, sd, utts, groups):
    """The mirror's rule and the score audit over every utterance of a case; the cap over the case's counted steps."""
    counted = ambiguous = 0
    for u, rows, scores in groups:
        text, first = _text_first(utts[u])
        req = SR.replay_request(u)
        c, a = SR.replay_rows(sd, cfg, text, rows, len(first) + 1, MAX_NEW, req.seed, req.top_k, req.temperature)
        R.audit_sampled_rows(sd, cfg, text, rows, scores, len(first) + 1, MAX_NEW, req.top_k, 1.0, req.temperature, R.AUDIT_DELTA)
        counted, ambiguous = counted + c, ambiguous + a
        if len(rows) > 1:
            assert len({tuple(r.tolist()) for r in rows}) == len(rows), f'{name}: the beams of utterance {u} must differ'
    print(f'{name}: {counted} counted steps, {ambiguous} ambiguous ({ambiguous / counted:.3f})')
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted, f'{name}: {ambiguous} of {counted} counted steps are ambiguous'


@pytest.mark.parametrize('name', sorted(CASES))
def test_rows_are_the_mirrors(name, inputs):
    cfg, sd, utts, groups, stats = decode(name, inputs)
    check(name, cfg, sd, utts, groups)


@pytest.mark.parametrize('name', EAGER)
def test_eager_arm_rows_are_the_mirrors(name, inputs):
    cfg, sd, utts, groups, stats = decode(name, inputs, use_graph=False)
    check(name, cfg, sd, utts, groups)


# ---- exact statements ----------------------------------------------------------------------------------------------------
WHICH = [0, 2, 4]


@pytest.fixture(scope='module')
def base(inputs):
    """generate_batch(beams=3) over three utterances, graph mode: the run the exact tests compare against."""
    cfg, sd, utts = inputs('d128')
    m = _build(cfg, sd)
    requests = [SR.replay_request(u) for u in WHICH]
    torch.manual_seed(0)
    per_utt, _ = _batch(m, [utts[u] for u in WHICH], requests, 3)
    return m, utts, requests, per_utt


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rows_do_not_depend_on_the_order_the_torch_seed_or_the_graph(base):
    m, utts, requests, per_utt = base
    perm = [2, 0, 1]
    torch.manual_seed(1234)
    moved, _ = _batch(m, [utts[WHICH[i]] for i in perm], [requests[i] for i in perm], 3)
    for at, i in enumerate(perm):
        assert _same(moved[at], per_utt[i]), f'utterance {WHICH[i]} at group {at} differs from itself at group {i}'
    eager, _ = _batch(m, [utts[u] for u in WHICH], requests, 3, use_graph=False)
    for i in range(3):
        assert _same(eager[i], per_utt[i]), f'utterance {WHICH[i]}: eager steps differ from the graph'


def test_another_requests_seed_moves_only_that_request(base):
    from valle2_amd import Sampling
    m, utts, requests, per_utt = base
    r = requests[1]
    other = [requests[0], Sampling(r.seed + 1, top_k=r.top_k, tok_p=r.tok_p, temperature=r.temperature), requests[2]]
    got, _ = _batch(m, [utts[u] for u in WHICH], other, 3)
    assert _same(got[0], per_utt[0]) and _same(got[2], per_utt[2])
    assert not torch.equal(got[1][0], per_utt[1][0])


def test_a_greedy_request_inside_a_sampled_batch(base, inputs):
    from valle2_amd import Sampling
    m, utts, requests, per_utt = base
    got, _ = _batch(m, [utts[u] for u in WHICH], [requests[0], Sampling(5, top_k=1), requests[2]], 3)
    assert _same(got[0], per_utt[0]) and _same(got[2], per_utt[2])
    cfg, sd, _ = inputs('d128', top_k=1)
    g = _build(cfg, sd)
    texts, firsts = zip(*[_text_first(utts[u]) for u in WHICH])
    ref = g.generate_batch([t.to(DEV) for t in texts], [f.to(DEV) for f in firsts], beams=3).cpu()
    assert g.last_generate_stats['sampling'] == 'call'
    assert torch.equal(got[1][0], ref[3:6]) and bool((ref[3] == ref[4]).all()), 'the greedy request is not the greedy model\'s row'
    assert got[1][1].tolist() == [0.0, 0.0, 0.0], 'greedy scores are exactly 0'


def test_a_greedy_request_through_the_wide_sampler(inputs):
    """The same statement at V = 4097: the greedy branch of sample_step_wide_kernel against vh_greedy_step."""
    from valle2_amd import Sampling
    cfg, sd, utts = inputs('v4096')
    m = _build(cfg, sd)
    which = [1, 2]
    got, _ = _batch(m, [utts[u] for u in which], [SR.replay_request(1), Sampling(9, top_k=1, tok_p=0.5, temperature=3.0)], 2)
    gcfg, _, _ = inputs('v4096', top_k=1)
    g = _build(gcfg, sd)
    texts, firsts = zip(*[_text_first(utts[u]) for u in which])
    ref = g.generate_batch([t.to(DEV) for t in texts], [f.to(DEV) for f in firsts], beams=2).cpu()
    assert torch.equal(got[1][0], ref[2:4]) and bool((ref[2] == ref[3]).all()), 'the greedy request is not the greedy model\'s row'
    assert got[1][1].tolist() == [0.0, 0.0], 'greedy scores are exactly 0'
    assert not torch.equal(got[0][0][0], got[0][0][1]), 'the sampled request beside it must still sample'


def test_top_p_requests_repeat_and_move_with_their_utterance(inputs):
    from valle2_amd import Sampling
    cfg, sd, utts = inputs('d128')
    m = _build(cfg, sd)
    requests = [Sampling(SR.REPLAY_SEEDS[u], top_k=8, tok_p=0.9, temperature=1.0) for u in WHICH]
    first, _ = _batch(m, [utts[u] for u in WHICH], requests, 3)
    again, _ = _batch(m, [utts[u] for u in WHICH], requests, 3)
    perm = [1, 2, 0]
    moved, _ = _batch(m, [utts[WHICH[i]] for i in perm], [requests[i] for i in perm], 3)
    for i in range(3):
        assert _same(first[i], again[i])
        assert _same(moved[perm.index(i)], first[i])
        text, f = _text_first(utts[WHICH[i]])
        rows = _pad(first[i][0], len(f) + 1 + MAX_NEW, cfg.num_audio_tokens)
        assert SR.assert_in_topk_support(sd, cfg, text, rows, len(f) + 1, MAX_NEW, 8, 1.0) >= 3
    plain, _ = _batch(m, [utts[u] for u in WHICH], [Sampling(r.seed, top_k=8, tok_p=1.0, temperature=1.0) for r in requests], 3)
    assert any(not torch.equal(plain[i][0], first[i][0]) for i in range(3)), 'tok_p = 0.9 cut nothing in any row'


def test_perf_mode_generate_repeats(inputs):
    cfg, sd, utts = inputs('d128', num_beams=4)
    m = _build(cfg, sd)
    utt = tuple(t.to(DEV) for t in utts[2])
    req = SR.replay_request(2)
    runs = []
    for seed in (0, 99):
        torch.manual_seed(seed)
        out = m.generate(*utt, perf_mode='kv', sampling=req)
        st = m.last_generate_stats
        assert st['sampling'] == 'rows' and st['kv_bf16'] is True and st['shared_prompt'] is True
        runs.append((out.cpu(), st['sum_logprobs'].cpu()))
    assert _same(runs[0], runs[1])
