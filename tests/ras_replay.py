"""The float64 mirror of repetition-aware sampling (valle2_amd.RepetitionAware; include/valle_hip.h, vh_row_sampling's two
reserved words): tests/sampling_replay.py's mirror of the filtered draw with the rule on top.  CPU only
(tests/test_repetition_sampling_cpu.py runs it as the sampler, tests/test_repetition_sampling_gpu.py holds device rows and
single launches against it).

The rule, restated from valle2_amd/csrc/elementwise.hip: at audio position p (BOS at 0) of a row that has not finished,
  1. c is the filtered draw with u1 = uniform01(seed, key, p): sampling_replay.mirror_step;
  2. n_c counts c in the row's own codes[max(1, p - window) .. p - 1] (the prompt counts, BOS never does);
  3. n_c > max_repeats: the token is drawn again over ALL V entries of softmax(logits / temperature), walked in index order,
     with u2 = uniform01(seed, key, p | RAS_STREAM); it may be c again, or EOS;
  4. a finished row (codes[p - 1] == eos) writes EOS; 5. top_k == 1 is the arg-max whatever window and max_repeats say.
A request without `window` (a plain Sampling) never redraws.

Ambiguity composes.  Where the first draw is ambiguous (sampling_replay's rule: u1 within 2 w of a CDF boundary, or scores
within 2 w of the top_k threshold, w = delta / temperature), EVERY candidate c of it is followed through its own count and,
where that triggers, its own redraw.  A redraw is ambiguous when u2 lies within 2 w of an inner boundary of the V-entry CDF;
its candidates are the two tokens that share the boundary.  At an ambiguous step the device's token must be one of the
candidates, at every other counted step the mirror's.  The redraw walks V - 1 boundaries of width 4 w: at delta = 1e-4 and
temperature 0.8 a 1025-entry vocabulary would excuse half of the redraw steps, so the model cases use V = 33 (1.6 %)."""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_runners as R
from tests.sampling_replay import AMBIGUOUS_CAP, ReplayError, _walk, counted_steps, mirror_step, uniform01  # noqa: F401

RAS_STREAM = 0x40000000


def rule_of(request):
    """(window, max_repeats) of a request; (0, 0) for one without the rule."""
    return int(getattr(request, 'window', 0)), int(getattr(request, 'max_repeats', 0))


def repeats(history, pos, window, tok):
    """n_c: how many of history[max(1, pos - window) .. pos - 1] equal tok (history[0] is BOS and never counted)."""
    return sum(int(t) == int(tok) for t in history[max(1, pos - window):pos])


def redraw(logits, temperature, u2, w):
    """The second draw over float64 `logits` (V,): (token, near — the tokens sharing a boundary within 2 w of u2, empty when
    there is none —, log-probability of the token under softmax(logits / temperature))."""
    x = np.asarray(logits, dtype=np.float64) / temperature
    tok, near = _walk(x, range(len(x)), u2, w, False)
    return tok, near, float(x[tok] - (x.max() + np.log(np.exp(x - x.max()).sum())))


def mirror_step_ras(logits, history, request, key, pos, delta, eos=None):
    """One step of one row: (token, redrawn, ambiguous, candidates).  logits (V,) float64 at this step; history the row's
    codes[0 .. pos - 1] (BOS first); request carries seed, top_k, temperature (its own, not None) and optionally window /
    max_repeats; eos defaults to V - 1 (the head's last entry)."""
    V = len(logits)
    eos = V - 1 if eos is None else eos
    if int(history[pos - 1]) == eos:
        return eos, False, False, {eos}
    tok_p = 1.0 if request.tok_p is None else request.tok_p
    c, amb, cands = mirror_step(logits, request.top_k, request.temperature, uniform01(request.seed, key, pos), delta, tok_p)
    window, max_repeats = rule_of(request)
    if window == 0 or request.top_k == 1:
        return c, False, amb, cands
    w = delta / request.temperature
    u2 = uniform01(request.seed, key, pos | RAS_STREAM)
    token, redrawn, out = c, False, set()
    for first in sorted(cands if amb else {c}):
        if repeats(history, pos, window, first) > max_repeats:
            t, near, _ = redraw(logits, request.temperature, u2, w)
            out |= near | {t}
            if first == c:
                token, redrawn, amb = t, True, amb or bool(near)
        else:
            out.add(first)
    return token, redrawn, amb, out


def step_logprob(logits, request, token, redrawn):
    """float64 log-probability of `token` at a step: unfiltered when the step redrew, else under the top_k filter."""
    x = np.asarray(logits, dtype=np.float64) / request.temperature
    V = len(x)
    if request.top_k == 1:
        return 0.0
    keep = np.ones(V, bool) if redrawn or not 1 < request.top_k < V else x >= np.sort(x)[V - request.top_k]
    return float(x[token] - (x[keep].max() + np.log(np.exp(x[keep] - x[keep].max()).sum())))


def replay_rows(sd, cfg, text, rows, prompt_len, max_new, request, delta=R.AUDIT_DELTA, keys=None):
    """sampling_replay.replay_rows under the rule: hold the rows of ONE utterance (n, width) int64 against the mirror, each
    step over the row's own history.  Returns (counted steps, ambiguous steps, redrawn steps); raises ReplayError naming the
    row and step of a token that is not allowed."""
    eos = cfg.num_audio_tokens
    rows = torch.as_tensor(rows).cpu().long()
    keys = list(range(len(rows))) if keys is None else list(keys)
    counts = [counted_steps(r, prompt_len, max_new, eos) for r in rows]
    logits = R._forced_logits64(sd, cfg, text, [rows[r, :prompt_len + counts[r] - 1] for r in range(len(rows))]).numpy()
    counted = ambiguous = redrawn = 0
    for r in range(len(rows)):
        hist = rows[r].tolist()
        for s in range(counts[r]):
            pos = prompt_len + s
            want, re, amb, cands = mirror_step_ras(logits[r, pos - 1], hist, request, keys[r], pos, delta, eos)
            got = hist[pos]
            if got != want and not (amb and got in cands):
                raise ReplayError(f'row {r} (key {keys[r]}) step {s}: the device drew {got}, the mirror {want} (redrawn: {re}, '
                                  f'ambiguous: {amb}, candidates {sorted(cands)}; {request})')
            counted, ambiguous, redrawn = counted + 1, ambiguous + amb, redrawn + re
    return counted, ambiguous, redrawn


def mirror_decode(sd, cfg, text, prompt_first, beams, max_new, request, delta=R.AUDIT_DELTA):
    """The mirror as the sampler: `beams` rows of one utterance decoded on the oracle's float64 logits under the rule.
    Returns (rows (beams, prompt_len + max_new) EOS-padded, scores (beams,) float64 — filtered log-probabilities of the first
    draws that stood, unfiltered ones of the redraws —, counted steps, ambiguous steps, redrawn steps)."""
    eos = cfg.num_audio_tokens
    prompt = torch.cat([torch.tensor([eos + 1]), prompt_first.cpu().long()])
    pl = len(prompt)
    rows = torch.full((beams, pl + max_new), eos, dtype=torch.int64)
    rows[:, :pl] = prompt
    scores = np.zeros(beams)
    live = list(range(beams))
    counted = ambiguous = redrawn = 0
    for s in range(max_new):
        if not live:
            break
        logits = R._forced_logits64(sd, cfg, text, [rows[r, :pl + s] for r in live])[:, -1].numpy()
        for i, r in enumerate(list(live)):
            tok, re, amb, _ = mirror_step_ras(logits[i], rows[r].tolist(), request, r, pl + s, delta, eos)
            scores[r] += step_logprob(logits[i], request, tok, re)
            rows[r, pl + s] = tok
            counted, ambiguous, redrawn = counted + 1, ambiguous + amb, redrawn + re
            if tok == eos:
                live.remove(r)
    return rows, torch.from_numpy(scores), counted, ambiguous, redrawn


# ---- the model cases (tests/test_repetition_sampling_cpu.py pins their counts; tests/test_repetition_sampling_gpu.py) ------
# The d128 audit model's recipe (oracle_runners.audit_inputs: 2 layers, d_model 128, rich weights, a scaled head, an EOS gain)
# with num_audio_tokens = 32: V = 33, so a redraw walks 32 inner boundaries (module docstring).
RAS_MAX_NEW = R.AUDIT_MAX_NEW
RAS_MODEL_SEED = R.AUDIT_MODEL_SEED
RAS_HEAD_SCALE, RAS_EOS_GAIN = 14.0, 1.0
RAS_UTTS = [(6, 5, 8), (9, 7, 25), (12, 9, 42)]            # (text a, text b, prompt frames), as oracle_runners.AUDIT_UTTS
RAS_WIDTHS = {'d128': dict(d_model=128, n_heads=2), 'w128': dict(d_model=256, n_heads=2)}
# utterance u carries RAS_REQUESTS[u]: (seed, top_k, temperature, window, max_repeats), tok_p 1.0.  Chosen on the CPU: over 33
# peaked entries a token repeats often, and the paper's window 10 / max_repeats 1 redraws at two steps in three — these redraw
# at 40 to 53 % of the mirror's own steps (test_repetition_sampling_cpu.py pins the counts), one of them with window 1.
RAS_REQUESTS = [(11, 16, 1.0, 3, 0), (2 ** 63 + 77, 8, 0.8, 10, 2), (7007, 4, 1.0, 1, 0)]
RAS_BEAMS = 4
# (width, utterance) -> (counted, ambiguous, redrawn) of mirror_decode over RAS_BEAMS rows: every model case of the GPU file
RAS_MIRROR_COUNTS = {('d128', 0): (117, 2, 62), ('d128', 1): (160, 1, 80), ('d128', 2): (138, 3, 55), ('w128', 0): (122, 1, 53)}


def ras_request(u):
    from valle2_amd import RepetitionAware
    seed, top_k, temperature, window, max_repeats = RAS_REQUESTS[u]
    return RepetitionAware(seed, top_k=top_k, tok_p=1.0, temperature=temperature, window=window, max_repeats=max_repeats)


def ras_inputs(width='d128', **cfg_kw):
    """(config kwargs, state dict, utterances) of the V = 33 model at `width`."""
    from tests.golden import cases as C
    from valle2_amd import synth
    kw = dict(C.AR_TINY, **RAS_WIDTHS[width])
    kw = dict(kw, num_audio_tokens=32, num_layers=2, max_audio_len=RAS_MAX_NEW, tok_p=1.0, **cfg_kw)
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleAR', seed=RAS_MODEL_SEED, rich=True)
    sd['proj.weight'] = sd['proj.weight'] * RAS_HEAD_SCALE
    sd['proj.weight'][cfg.num_audio_tokens] *= RAS_EOS_GAIN
    utts = [synth.synth_utterance(cfg, a, b, f, seed=2600 + i) for i, (a, b, f) in enumerate(RAS_UTTS)]
    return kw, sd, utts
