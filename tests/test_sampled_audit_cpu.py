"""oracle_runners.audit_sampled_rows can fail: it accepts the oracle's own sampled rows and scores and rejects each way a
decoder could get them wrong — by the check that is meant to catch it (asserted on the message).  No GPU."""
import re

import pytest
import torch

from oracle import valle_oracle as O
from tests import oracle_runners as R
from tests.golden import cases as C

MAX_NEW = R.AUDIT_MAX_NEW
RUN_ON = 8                 # the oracle runs this many steps past max_new: what a decoder that does not stop there would hold
BEAMS, TOP_K, TEMP = 4, 50, 1.0
SEED = 0                   # torch.manual_seed for the oracle's draws: beams that end by EOS and beams that reach max_new


@pytest.fixture(scope='module')
def sampled():
    """O.ar_generate on audit model 'd128' with sampling, MAX_NEW + RUN_ON steps; the rows rebuilt from trace['tokens'] and the
    scores from trace['logits'] by the reference's rule (sum_logprobs += lp * (previous token != EOS)), per step."""
    kw, sd, utts = R.audit_inputs('d128')
    cfg = C.cfg_of(dict(kw, top_k=TOP_K, temperature=TEMP, num_beams=BEAMS, max_audio_len=MAX_NEW + RUN_ON))
    pt, pc, tt = utts[2]
    eos, bos = cfg.num_audio_tokens, cfg.num_audio_tokens + 1
    trace = {}
    torch.manual_seed(SEED)
    O.ar_generate(sd, cfg, pt, pc, tt, trace=trace)
    toks = torch.stack(trace['tokens'], dim=1)                                # (beams, steps)
    steps = toks.shape[1]
    assert steps == MAX_NEW + RUN_ON, 'inputs drifted: every beam drew EOS early'
    prompt = torch.cat([torch.tensor([bos]), pc[:, 0]])
    rows = torch.cat([prompt[None].repeat(BEAMS, 1), toks], dim=1)
    lp = torch.zeros(BEAMS, steps, dtype=torch.float64)                       # log-prob of each step's token
    live = torch.zeros(BEAMS, steps, dtype=torch.bool)                        # previous token != EOS
    for s in range(steps):
        filt = O._top_k_top_p_filter(trace['logits'][s].double() / TEMP, top_k=TOP_K, top_p=1.0)
        logp = torch.log_softmax(filt, dim=-1)
        prev = rows[:, len(prompt) + s - 1]
        live[:, s] = prev != eos
        tok = toks[:, s].clone()
        # a finished beam's token is forced to EOS after the draw and the draw itself is not traced: its (uncounted) log-prob
        # is taken for the second likeliest token, a draw a decoder that counts the step could have made
        tok[~live[:, s]] = logp[~live[:, s]].topk(2, dim=-1)[1][:, 1]
        lp[:, s] = logp[torch.arange(BEAMS), tok]
    counted = live.clone()
    counted[:, MAX_NEW:] = False
    scores = (lp * counted).sum(dim=1)
    ended = [(toks[b, :MAX_NEW] == eos).any().item() for b in range(BEAMS)]
    first_eos = [int((toks[b] == eos).nonzero()[0]) if (toks[b] == eos).any() else None for b in range(BEAMS)]
    assert any(e is not None and e < MAX_NEW - 1 for e in first_eos) and not all(ended), f'inputs drifted: EOS at {first_eos}'
    text = torch.cat([pt, tt])
    return dict(cfg=cfg, sd=sd, text=text, rows=rows, scores=scores, lp=lp, live=live, pl=len(prompt), first_eos=first_eos)


def _audit(s, rows=None, scores=None):
    return R.audit_sampled_rows(s['sd'], s['cfg'], s['text'], s['rows'] if rows is None else rows,
                                s['scores'] if scores is None else scores, s['pl'], MAX_NEW, TOP_K, 1.0, TEMP, R.AUDIT_DELTA)


def test_accepts_the_oracles_own_rows_and_scores(sampled):
    rep = _audit(sampled)
    assert len(rep) == BEAMS
    for b, r in enumerate(rep):
        e = sampled['first_eos'][b]
        want = (e + 1, 'eos') if e is not None and e < MAX_NEW else (MAX_NEW, 'cap')
        assert (r['steps'], r['end']) == want
        assert r['hi'] - r['lo'] < 0.02 and abs(r['off']) < 0.01 + r['tol'], r     # a tight interval: no step's k-th token in doubt
    assert {r['end'] for r in rep} == {'eos', 'cap'}
    # EOS-padded to any width, and a float32 score as a decoder gives it
    padded = torch.cat([sampled['rows'][:, :sampled['pl'] + MAX_NEW], torch.full((BEAMS, 5), sampled['cfg'].num_audio_tokens)], dim=1)
    assert [r['steps'] for r in _audit(sampled, rows=padded, scores=sampled['scores'].float())] == [r['steps'] for r in rep]


def _eos_and_cap_beams(s):
    eos_b = next(b for b, e in enumerate(s['first_eos']) if e is not None and e < MAX_NEW - 1)
    cap_b = next(b for b, e in enumerate(s['first_eos']) if e is None or e >= MAX_NEW)
    return eos_b, cap_b


def test_rejects_two_beams_scores_swapped(sampled):
    a, b = _eos_and_cap_beams(sampled)
    scores = sampled['scores'].clone()
    scores[[a, b]] = scores[[b, a]]
    with pytest.raises(R.AuditError, match=rf'^score: row {min(a, b)}: device score'):
        _audit(sampled, scores=scores)


def test_rejects_a_beams_tokens_beside_another_beams_score(sampled):
    a, b = _eos_and_cap_beams(sampled)
    rows = sampled['rows'].clone()
    rows[a] = sampled['rows'][b]                                              # beam b's tokens, beam a's score
    with pytest.raises(R.AuditError, match=rf'^score: row {a}: device score'):
        _audit(sampled, rows=rows)


def test_rejects_a_token_outside_the_support(sampled):
    _, b = _eos_and_cap_beams(sampled)
    step = 17
    logits = R._forced_logits64(sampled['sd'], sampled['cfg'], sampled['text'], [sampled['rows'][b, :sampled['pl'] + step]])
    worst = int(logits[0, -1].argmin())                                       # the oracle's least likely token at that step
    rows = sampled['rows'].clone()
    rows[b, sampled['pl'] + step] = worst
    with pytest.raises(R.AuditError, match=rf'^support: row {b} step {step} token {worst}: .*{TOP_K}-th largest') as err:
        _audit(sampled, rows=rows)
    got = [float(x) for x in re.findall(r'-?\d+\.\d{6}', str(err.value))]
    assert got[0] == pytest.approx(float(logits[0, -1, worst]), abs=1e-6) and got[0] < got[1], 'the token\'s logit, then the k-th'


def test_rejects_a_score_with_one_step_after_eos(sampled):
    a, _ = _eos_and_cap_beams(sampled)
    e = sampled['first_eos'][a]
    scores = sampled['scores'].clone()
    scores[a] += sampled['lp'][a, e + 1]
    assert not sampled['live'][a, e + 1] and sampled['lp'][a, e + 1] < -10 * 2 * R.AUDIT_DELTA * MAX_NEW
    with pytest.raises(R.AuditError, match=rf'^score: row {a}: device score .*{e + 1} counted steps, ended by eos'):
        _audit(sampled, scores=scores)


def test_rejects_a_score_without_the_eos_draw(sampled):
    a, _ = _eos_and_cap_beams(sampled)
    e = sampled['first_eos'][a]
    scores = sampled['scores'].clone()
    scores[a] -= sampled['lp'][a, e]
    with pytest.raises(R.AuditError, match=rf'^score: row {a}: device score .*{e + 1} counted steps, ended by eos'):
        _audit(sampled, scores=scores)


def test_rejects_a_score_accumulated_past_max_new(sampled):
    _, b = _eos_and_cap_beams(sampled)
    past = (sampled['lp'] * sampled['live'])[:, MAX_NEW:].sum(dim=1)
    assert past[b] < -10 * 2 * R.AUDIT_DELTA * MAX_NEW
    scores = sampled['scores'] + past
    with pytest.raises(R.AuditError, match=rf'^score: row {b}: device score .*{MAX_NEW} counted steps, ended by cap'):
        _audit(sampled, scores=scores)


def test_top_k_0_and_a_temperature(sampled):
    """top_k = 0: every token is in the support and lo == hi; the score is the plain log-softmax of logits / T."""
    s = sampled
    logits = R._forced_logits64(s['sd'], s['cfg'], s['text'], [s['rows'][0, :s['pl'] + MAX_NEW - 1]])[0]
    n = (s['first_eos'][0] + 1) if s['first_eos'][0] is not None and s['first_eos'][0] < MAX_NEW else MAX_NEW
    lp = torch.log_softmax(logits[s['pl'] - 1:s['pl'] - 1 + n] / 1.2, dim=-1)
    score = lp[torch.arange(n), s['rows'][0, s['pl']:s['pl'] + n]].sum()
    rep = R.audit_sampled_rows(s['sd'], s['cfg'], s['text'], s['rows'][:1], score[None], s['pl'], MAX_NEW, 0, 1.0, 1.2, R.AUDIT_DELTA)
    assert rep[0]['lo'] == rep[0]['hi'] and abs(rep[0]['off']) < 1e-9 and rep[0]['steps'] == n
    with pytest.raises(R.AuditError, match=r'^score: row 0'):
        R.audit_sampled_rows(s['sd'], s['cfg'], s['text'], s['rows'][:1], score[None], s['pl'], MAX_NEW, 0, 1.0, 1.0, R.AUDIT_DELTA)
