"""Repetition-aware sampling per request (valle2_amd.RepetitionAware; vh_row_sampling's two reserved words), the parts that
need no GPU: what RepetitionAware refuses, alone and where it meets a config, on a CPU model with no device; its records and
their packed bytes; the header and the ABI number; the float64 mirror (tests/ras_replay.py) on hand-made cases; and the
mirror decoding every model case of tests/test_repetition_sampling_gpu.py on the oracle's float64 logits — inside the cap
on ambiguous steps, redrawing at 10 to 60 % of the counted steps so that both branches carry weight, counts pinned."""
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ras_replay as RR
from tests import sampling_replay as SR
from tests.golden import cases as GC
from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()


# ---- 1. RepetitionAware and the entry points, on a CPU model --------------------------------------------------------------
def test_repetition_aware_is_a_sampling_with_two_more_fields():
    import valle2_amd
    from valle2_amd import ConfigValle, RepetitionAware, Sampling
    from valle2_amd import sampling as S
    assert 'RepetitionAware' in valle2_amd.__all__ and 'Sampling' in valle2_amd.__all__
    assert [f.name for f in dataclasses.fields(Sampling)] == ['seed', 'top_k', 'tok_p', 'temperature']
    assert [f.name for f in dataclasses.fields(RepetitionAware)] == ['seed', 'top_k', 'tok_p', 'temperature', 'window', 'max_repeats']
    r = RepetitionAware(7)
    assert isinstance(r, Sampling) and (r.window, r.max_repeats) == (10, 1), 'the paper\'s K = 10, t_r = 0.1'
    assert r == RepetitionAware(7, None, None, None, 10, 1) and hash(r) == hash(RepetitionAware(7, window=10, max_repeats=1))
    assert r != RepetitionAware(7, window=9) and r != Sampling(7)
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.window = 3
    cfg = ConfigValle(top_k=50, tok_p=1.0, temperature=0.7)
    q = RepetitionAware(9, top_k=8, tok_p=0.9, temperature=0.8, window=4, max_repeats=0)
    base = Sampling(9, top_k=8, tok_p=0.9, temperature=0.8)
    assert q.resolved(cfg) == base.resolved(cfg) == (8, 0.9, 0.8) and r.resolved(cfg) == (50, 1.0, 0.7)
    assert q.records(cfg, 2) == [(9, 0, 8, 0.9, 0.8, 4, 0), (9, 1, 8, 0.9, 0.8, 4, 0)]
    assert q.records(cfg, 1, first_key=3) == [(9, 3, 8, 0.9, 0.8, 4, 0)]
    assert base.records(cfg, 2) == [(9, 0, 8, 0.9, 0.8), (9, 1, 8, 0.9, 0.8)], 'Sampling.records keeps its 5-tuples'
    assert q.nar_record(cfg) == base.nar_record(cfg) and r.nar_record(cfg) == Sampling(7).nar_record(cfg), 'the NAR stage ignores the rule'
    # the lists and the internal row keys carry it like any Sampling
    assert S.check_list('e', [q, base], 2) == [q, base] and S.check_list('e', [q, base], 2, cfg=cfg) == [q, base]
    utt = (torch.arange(3), torch.zeros(4, 8, dtype=torch.int64), torch.arange(2))
    assert S.of_utterances('e', [utt + (q,), utt + (r,)]) == [q, r]
    rows = S.beam_rows(q, 2)
    assert [k.records(cfg, 1) for k in rows] == [[rec] for rec in q.records(cfg, 2)]
    assert S.repetition_aware([base, q]) and S.repetition_aware(rows) and not S.repetition_aware([base]) and not S.repetition_aware(None)


@pytest.mark.parametrize('kw,text', [
    (dict(window=0), 'window=0'), (dict(window=-3), 'window=-3'), (dict(window=2 ** 31), 'window='), (dict(window=2.0), 'window=2.0'),
    (dict(window=True), 'window=True'), (dict(window=None), 'window=None'),
    (dict(max_repeats=-1), 'max_repeats=-1'), (dict(max_repeats=10), 'max_repeats=10'), (dict(window=3, max_repeats=3), 'max_repeats=3'),
    (dict(max_repeats=1.0), 'max_repeats=1.0'), (dict(max_repeats=False), 'max_repeats=False'), (dict(window=1, max_repeats=1), 'max_repeats=1'),
    (dict(top_k=1), 'top_k=1'),
    (dict(seed=-1), 'seed=-1'), (dict(temperature=0.0), 'temperature=0.0'), (dict(tok_p=1.5), 'tok_p=1.5'),      # Sampling's own
])
def test_repetition_aware_validates(kw, text):
    from valle2_amd import RepetitionAware
    with pytest.raises(ValueError, match=re.escape(text)):
        RepetitionAware(**dict(dict(seed=1), **kw))
    RepetitionAware(1, window=2 ** 31 - 1, max_repeats=2 ** 31 - 2)
    RepetitionAware(1, window=1, max_repeats=0)
    RepetitionAware(1, top_k=0)


def _cpu_model(**kw):
    from valle2_amd import ConfigValle, get_model_class
    cfg = ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm',
                                  num_beams=4, top_k=50, max_audio_len=8), **kw))
    return get_model_class('ValleAR')(cfg)


def _utt(sampling):
    return torch.arange(5), torch.arange(7 * 8).reshape(7, 8) % 1024, torch.arange(10, 13), sampling


def test_a_greedy_config_is_refused_where_the_request_meets_it_before_any_device_work():
    """A CPU model: anything that went on to the device would raise VhError (no device) or copy the model there."""
    from valle2_amd import RepetitionAware, Sampling
    m = _cpu_model(top_k=1)
    r, own, plain = RepetitionAware(1), RepetitionAware(1, top_k=8), Sampling(2)
    names_both = r'RepetitionAware: top_k=None takes the config\'s top_k=1'
    texts, firsts = [torch.arange(5)] * 2, [torch.arange(7)] * 2
    with pytest.raises(ValueError, match=names_both):
        r.resolved(m.config)
    with pytest.raises(ValueError, match=names_both):
        m.generate(*_utt(r)[:3], sampling=r)
    with pytest.raises(ValueError, match=names_both):
        m.generate_batch(texts, firsts, sampling=[plain, r])
    with pytest.raises(ValueError, match=names_both):
        m.generate_batch(texts, firsts, beams=2, sampling=[own, r])
    with pytest.raises(ValueError, match=names_both):
        m.generate_many([_utt(own), _utt(r)])
    with pytest.raises(ValueError, match=names_both):
        m.generate_queued([_utt(plain), _utt(own), _utt(r)], beams=2)
    assert own.resolved(m.config) == (8, 1.0, 1.0), 'a top_k of its own is fine under a greedy config'
    # the config's temperature is checked at the same place
    cold = _cpu_model(temperature=0.0)
    with pytest.raises(ValueError, match='the config\'s temperature=0.0'):
        cold.generate_many([_utt(own), _utt(own)])


# ---- 2. records, packed bytes, header, ABI ---------------------------------------------------------------------------------
def test_packed_records_carry_the_two_words_at_bytes_24_and_28():
    from valle2_amd import ConfigValle, RepetitionAware, Sampling, kernels
    cfg = ConfigValle(top_k=50, tok_p=1.0, temperature=1.0)
    q = RepetitionAware(2 ** 64 - 1, top_k=8, temperature=0.8, window=2 ** 31 - 1, max_repeats=258)
    packed = kernels.pack_row_sampling(q.records(cfg, 2) + Sampling(5).records(cfg, 1))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, kernels.ROW_SAMPLING_BYTES) and kernels.ROW_SAMPLING_BYTES == 32
    words = packed.numpy().view('<u4').reshape(3, 8)
    assert words[:2, 6].tolist() == [2 ** 31 - 1] * 2 and words[:2, 7].tolist() == [258] * 2, 'reserved == [window, max_repeats]'
    assert words[2, 6:].tolist() == [0, 0], 'a plain Sampling still packs zeros'
    recs = (_lib.VhRowSampling * 3).from_buffer_copy(packed.numpy().tobytes())
    assert _lib.VhRowSampling.reserved.offset == 24 and list(recs[1].reserved) == [2 ** 31 - 1, 258] and list(recs[2].reserved) == [0, 0]
    assert (recs[1].seed, recs[1].key, recs[1].top_k) == (2 ** 64 - 1, 1, 8) and recs[1].temperature == np.float32(0.8)
    # the first 24 bytes are what the base request packs
    base = kernels.pack_row_sampling(Sampling(2 ** 64 - 1, top_k=8, temperature=0.8).records(cfg, 2))
    assert torch.equal(packed[:2, :24], base[:, :24]) and not base[:, 24:].any()
    with pytest.raises(ValueError, match='record 0 holds 6 values'):
        kernels.pack_row_sampling([(1, 0, 8, 1.0, 1.0, 10)])


def test_header_names_both_words_and_the_abi_number_moved():
    L = _lib.load_library()
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared >= 140
    comment = HEADER[HEADER.index('with PER-ROW sampling'):HEADER.index('} vh_row_sampling;')]
    for text in ('reserved[0]', 'reserved[1]', 'window', 'max_repeats', '0x40000000', 'top_k == 1', 'BOS'):
        assert text in comment, f'the comment above vh_row_sampling does not say {text!r}'
    text = (REPO / 'INTEGRATION.md').read_text()
    assert f'ABI {declared}' in text and 'max_repeats' in text
    for old in ('ABI 134', 'ABI 135', 'ABI 139'):
        assert old in text


# ---- 3. the mirror on hand-made cases --------------------------------------------------------------------------------------
V, EOS, BOS = 9, 8, 9


def _req(window, max_repeats, seed=3, top_k=2, temperature=1.0):
    from valle2_amd import RepetitionAware
    return RepetitionAware(seed, top_k=top_k, tok_p=1.0, temperature=temperature, window=window, max_repeats=max_repeats)


def _peaked(tok, others=0.0):
    """Logits under which top_k = 2 keeps `tok` and entry 0 (or 1), and the first draw is `tok` with probability ~ 1."""
    x = np.full(V, others)
    x[tok] = 40.0
    return x


def _second(logits, req, key, pos, temperature=1.0):
    return RR.redraw(logits, temperature, RR.uniform01(req.seed, key, pos | RR.RAS_STREAM), 0.0)[0]


def test_the_second_uniform_is_the_first_generators_at_bit_30():
    assert RR.RAS_STREAM == 0x40000000 == __import__('valle2_amd').sampling.RAS_STREAM
    u = [RR.uniform01(5, k, p | RR.RAS_STREAM) for k in range(3) for p in range(1, 40)]
    firsts = {RR.uniform01(5, k, p) for k in range(3) for p in range(5000)}
    assert all(0.0 <= x < 1.0 for x in u) and len(set(u)) > 100 and not set(u) <= firsts
    assert RR.uniform01(5, 1, 7 | RR.RAS_STREAM) == SR.uniform01(5, 1, 0x40000007)


def test_mirror_counts_the_window_and_triggers_above_max_repeats():
    flat = np.linspace(0.0, 1.0, V)                               # the unfiltered distribution is anything but peaked
    logits = flat.copy()
    logits[4] = 6.0                                               # first draw: 4 (top_k 2 keeps 4 and 7; 4 has p = 0.993)
    hist = [BOS, 4, 4, 1, 2, 4, 3]                                # pos 7: the last 4 tokens hold one 4, the last 6 three
    pos = len(hist)
    req = _req(4, 1)
    u1 = RR.uniform01(req.seed, 0, pos)
    assert SR.mirror_step(logits, 2, 1.0, u1, 0.0)[0] == 4
    assert RR.repeats(hist, pos, 4, 4) == 1 and RR.repeats(hist, pos, 6, 4) == 3 and RR.repeats(hist, pos, 100, 4) == 3
    # n_c == R: no redraw; n_c == R + 1: redraw
    assert RR.mirror_step_ras(logits, hist, _req(4, 1), 0, pos, 0.0, EOS)[:2] == (4, False)
    assert RR.mirror_step_ras(logits, hist, _req(4, 0), 0, pos, 0.0, EOS)[:2] == (_second(logits, req, 0, pos), True)
    assert RR.mirror_step_ras(logits, hist, _req(6, 3), 0, pos, 0.0, EOS)[:2] == (4, False)
    assert RR.mirror_step_ras(logits, hist, _req(6, 2), 0, pos, 0.0, EOS)[:2] == (_second(logits, req, 0, pos), True)
    # K = 1: only the previous token
    assert RR.mirror_step_ras(logits, hist, _req(1, 0), 0, pos, 0.0, EOS)[:2] == (4, False)
    assert RR.mirror_step_ras(logits, hist + [4], _req(1, 0), 0, pos + 1, 0.0, EOS)[1] is True
    # a history shorter than K, and a plain Sampling never redraws
    assert RR.mirror_step_ras(logits, [BOS, 4, 4], _req(10, 1), 2, 3, 0.0, EOS)[1] is True
    assert RR.mirror_step_ras(logits, [BOS, 4], _req(10, 1), 2, 2, 0.0, EOS)[:2] == (4, False)
    from valle2_amd import Sampling
    assert RR.mirror_step_ras(logits, hist, Sampling(3, top_k=2, tok_p=1.0, temperature=1.0), 0, pos, 0.0, EOS)[:2] == (4, False)


def test_mirror_never_counts_bos():
    logits = _peaked(BOS % V)                                     # a token whose id equals the BOS entry cannot be drawn (V = 9):
    assert RR.repeats([BOS, BOS, 1], 3, 10, BOS) == 1             # but position 0 is skipped whatever it holds
    assert RR.repeats([4, 1, 2], 3, 10, 4) == 0 and RR.repeats([4, 4], 2, 1, 4) == 1 and RR.repeats([4], 1, 5, 4) == 0
    logits = _peaked(4)
    assert RR.mirror_step_ras(logits, [4], _req(5, 0), 0, 1, 0.0, EOS)[:2] == (4, False), 'position 1: the window is empty'


def test_mirror_finished_rows_and_redraws_that_return_eos():
    logits = _peaked(4)
    assert RR.mirror_step_ras(logits, [BOS, 4, 4, EOS], _req(5, 0), 0, 4, 0.0, EOS) == (EOS, False, False, {EOS})
    # the unfiltered distribution is EOS almost surely, the filter (top_k 2 of a request with temperature 1) never keeps it
    logits = np.full(V, -30.0)
    logits[EOS] = 0.0
    logits[2], logits[5] = 1.0, 0.5                                # top_k 2: {2, 5}; unfiltered: p(EOS) = 0.19 ...
    req = _req(3, 0, seed=next(s for s in range(200) if RR.redraw(logits, 1.0, RR.uniform01(s, 1, 6 | RR.RAS_STREAM), 0.0)[0] == EOS
                               and SR.mirror_step(logits, 2, 1.0, RR.uniform01(s, 1, 6), 0.0)[0] == 2))
    tok, redrawn, amb, cands = RR.mirror_step_ras(logits, [BOS, 1, 1, 2, 5, 2], req, 1, 6, 0.0, EOS)
    assert (tok, redrawn, amb, cands) == (EOS, True, False, {EOS})
    assert RR.step_logprob(logits, req, EOS, True) == pytest.approx(float(logits[EOS] - np.log(np.exp(logits).sum())))
    assert RR.step_logprob(logits, req, 2, False) == pytest.approx(float(1.0 - np.log(np.exp(1.0) + np.exp(0.5))))


def test_mirror_greedy_requests_ignore_the_words():
    class Greedy:                       # what a record with top_k == 1 and the words set asks for (RepetitionAware refuses it)
        seed, top_k, tok_p, temperature, window, max_repeats = 3, 1, 1.0, 1.0, 5, 0
    logits = np.linspace(0.0, 1.0, V)
    logits[4] = 1.5
    assert RR.mirror_step_ras(logits, [BOS, 4, 4, 4], Greedy, 0, 4, 0.0, EOS)[:2] == (4, False)


def test_mirror_ambiguity_composes():
    # a redraw whose u2 sits on a boundary: both neighbours are candidates and the step is ambiguous
    logits = np.linspace(0.0, 2.0, V)
    logits[4] = 3.0                                               # top_k 2 keeps {4, EOS}; every entry holds 3 % or more
    hist = [BOS, 4, 4, 4]
    cdf = np.cumsum(np.exp(logits)) / np.exp(logits).sum()

    def gaps(s):
        return np.sort(np.abs(cdf[:-1] - RR.uniform01(s, 0, 4 | RR.RAS_STREAM)))
    seed = next(s for s in range(200) if SR.mirror_step(logits, 2, 1.0, RR.uniform01(s, 0, 4), gaps(s)[0])[:2] == (4, False)
                and gaps(s)[1] > 2 * gaps(s)[0])
    req = _req(3, 0, seed=seed)
    gap = float(gaps(seed)[0])
    tok, redrawn, amb, cands = RR.mirror_step_ras(logits, hist, req, 0, 4, gap * 0.51, EOS)       # 2 w just covers the gap
    assert redrawn and amb and len(cands) == 2 and tok in cands
    assert RR.mirror_step_ras(logits, hist, req, 0, 4, gap * 0.49, EOS)[2] is False
    # an ambiguous first draw: every candidate is followed through its own count
    logits = np.zeros(V)
    logits[2] = logits[6] = 5.0                                   # top_k 2 keeps {2, 6} at one half each
    seed = next(s for s in range(4000) if abs(RR.uniform01(s, 0, 4) - 0.5) < 1e-3)
    req = _req(3, 0, seed=seed)
    tok, redrawn, amb, cands = RR.mirror_step_ras(logits, [BOS, 1, 2, 2], req, 0, 4, 1e-3, EOS)    # 2 repeats, 6 does not
    second = _second(logits, req, 0, 4)
    assert amb and 6 in cands and second in cands and (2 in cands) == (second == 2)
    assert (tok, redrawn) == ((second, True) if RR.uniform01(seed, 0, 4) < 0.5 else (6, False))


# ---- 4. the model cases, on the CPU alone ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models():
    made = {}

    def get(width):
        if width not in made:
            kw, sd, utts = RR.ras_inputs(width)
            made[width] = (GC.cfg_of(kw), sd, utts)
        return made[width]
    return get


def test_the_model_cases_use_a_small_vocabulary_and_peaked_logits(models):
    from tests import oracle_runners as R
    cfg, sd, utts = models('d128')
    assert cfg.num_audio_tokens == 32 and cfg.num_layers == 2 and cfg.d_model == 128 and tuple(sd['proj.weight'].shape) == (33, 128)
    assert len(RR.RAS_REQUESTS) == len(utts) and {r[3] for r in RR.RAS_REQUESTS} >= {1, 10}, 'window 1 and the paper\'s 10'
    for pt, pc, tt in utts:
        assert 1.5 <= R.head_logit_std(sd, cfg, torch.cat([pt, tt]), pc[:, 0]) <= 3.0
    # 32 inner boundaries of width 4 delta / temperature: what a redraw step may be excused by
    assert 32 * 4 * R.AUDIT_DELTA / 0.8 < 0.02 < SR.AMBIGUOUS_CAP


@pytest.mark.parametrize('width,u', sorted(RR.RAS_MIRROR_COUNTS))
def test_mirror_decodes_every_model_case_within_the_cap_and_the_redraw_share(models, width, u):
    cfg, sd, utts = models(width)
    pt, pc, tt = utts[u]
    text, first = torch.cat([pt, tt]), pc[:, 0]
    req = RR.ras_request(u)
    rows, scores, counted, ambiguous, redrawn = RR.mirror_decode(sd, cfg, text, first, RR.RAS_BEAMS, RR.RAS_MAX_NEW, req)
    print(f'{width} utterance {u}: {counted} counted, {ambiguous} ambiguous, {redrawn} redrawn ({redrawn / counted:.2f})')
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted
    assert 0.10 * counted <= redrawn <= 0.60 * counted
    assert (counted, ambiguous, redrawn) == RR.RAS_MIRROR_COUNTS[(width, u)]
    assert len({tuple(r.tolist()) for r in rows}) == RR.RAS_BEAMS and bool(torch.isfinite(scores).all()) and bool((scores < 0).all())
    # the mirror's own rows replay, and a row with one token moved does not
    pl = len(first) + 1
    assert RR.replay_rows(sd, cfg, text, rows, pl, RR.RAS_MAX_NEW, req) == (counted, ambiguous, redrawn)
    if u == 0:
        # without the rule the same request decodes other rows: the rule is what these rows test
        from valle2_amd import Sampling
        plain = Sampling(req.seed, top_k=req.top_k, tok_p=1.0, temperature=req.temperature)
        with pytest.raises(SR.ReplayError):
            RR.replay_rows(sd, cfg, text, rows, pl, RR.RAS_MAX_NEW, plain)
