"""The float64 mirror of per-request length bounds (valle2_amd.Bounded; include/valle_hip.h, vh_row_limits): the rule on top
of tests/sampling_replay.py and tests/ras_replay.py, which are imported and not edited.  CPU only
(tests/test_length_bounds_cpu.py runs it on hand-worked rows and as the sampler, tests/test_length_bounds_gpu.py holds single
launches and device rows against it).

The rule, restated from valle2_amd/csrc/elementwise.hip (ROW_LIMITS_LOAD): for a row at audio position p (BOS at 0) that has
produced n = p - pos_base tokens,
  1. a finished row (codes[p - 1] == eos) writes EOS and reads neither bound;
  2. max_new > 0 and n >= max_new: EOS, forced — no draw, no count, no redraw, the score does not move;
  3. otherwise n < min_new: the EOS logit is -inf for everything that follows (top-k with its ties, top-p, the arg-max, the
     draw, the redraw over all V entries) and the log-probability is the one without EOS;
  4. the uniforms are ras_replay's: uniform01(seed, key, p) and uniform01(seed, key, p | RAS_STREAM).
Ambiguity is sampling_replay's (same rule, same AMBIGUOUS_CAP); a suppressed EOS is never a candidate.

top-p (tok_p < 1), which sampling_replay does not mirror, is mirrored here for the single launches: descending order (ties to
the lower index), top-k with ties, then entries dropped from the smallest up while the dropped mass is <= 1 - tok_p, the
largest always kept; the cut is ambiguous when a suffix sum lies within 2 w of 1 - tok_p, and then the kept sets one entry
shorter and longer are walked too."""
from __future__ import annotations

import numpy as np
import torch

from tests import oracle_runners as R
from tests import ras_replay as RR
from tests.sampling_replay import AMBIGUOUS_CAP, ReplayError, _walk, counted_steps, uniform01  # noqa: F401

FREE, SUPPRESSED, FORCED, FINISHED = 'free', 'suppressed', 'forced', 'finished'


def limits_of(request):
    """(min_new, max_new) of a request, 0 for a bound that is off; (0, 0) for one that is not a Bounded."""
    return int(getattr(request, 'min_new', 0) or 0), int(getattr(request, 'max_new', 0) or 0)


def inner(request):
    """The Sampling / RepetitionAware a Bounded wraps (the request itself otherwise)."""
    return request.request if hasattr(request, 'limits') else request


def state(history, pos, pos_base, min_new, max_new, eos):
    """Which of the four cases the row is in at this step."""
    if int(history[pos - 1]) == eos:
        return FINISHED
    n = pos - pos_base
    if max_new > 0 and n >= max_new:
        return FORCED
    return SUPPRESSED if n < min_new else FREE


def _kept_top_p(x, top_k, tok_p, w):
    """(kept indices in descending order, [alternative kept lists when the cut is ambiguous])."""
    V = len(x)
    order = [int(i) for i in np.lexsort((np.arange(V), -x))]
    n = V
    if top_k > 0:
        n = min(top_k, V)
        while n < V and x[order[n]] >= x[order[min(top_k, V) - 1]]:
            n += 1
    order = order[:n]
    e = np.exp(x[order] - x[order[0]])
    suffix = np.cumsum(e[::-1])[::-1] / e.sum()                       # suffix[j] = mass of entries j ..
    keep = 1 + int((suffix[1:] > 1.0 - tok_p).sum())
    alts = []
    if len(order) > 1 and np.any(np.abs(suffix[1:] - (1.0 - tok_p)) <= 2 * w):
        alts = [order[:k] for k in (keep - 1, keep + 1) if 1 <= k <= len(order)]
    return order[:keep], alts


def _first_draw(x, request, u, w):
    """(token, ambiguous, candidates, kept set or None for sampling_replay's own filter) over scaled-free float64 logits x."""
    tok_p = 1.0 if request.tok_p is None else float(request.tok_p)
    if tok_p == 1.0 or request.top_k == 1:
        from tests.sampling_replay import mirror_step
        tok, amb, cands = mirror_step(x, request.top_k, request.temperature, u, w * request.temperature)
        return tok, amb, cands, None
    xs = x / request.temperature
    kept, alts = _kept_top_p(xs, request.top_k, tok_p, w)
    tok, near = _walk(xs, kept, u, w, True)
    cands = near | {tok}
    for alt in alts:
        t, n = _walk(xs, alt, u, w, True)
        cands |= n | {t}
    return tok, bool(near) or bool(alts), cands, kept


def step_logprob(x, request, token, redrawn, kept=None):
    """float64 log-probability of `token` over logits x (a suppressed EOS already -inf): ras_replay's, or under the top-p
    kept set."""
    if kept is None or redrawn or request.top_k == 1:
        return RR.step_logprob(x, request, token, redrawn)
    xs = x / request.temperature
    sel = xs[np.asarray(kept)]
    return float(xs[token] - (sel.max() + np.log(np.exp(sel - sel.max()).sum())))


def mirror_step_bounded(logits, history, request, key, pos, pos_base, delta, eos=None, limits=None):
    """One step of one row: (token, case, redrawn, ambiguous, candidates, log-probability or None where the score does not
    move).  request: a Bounded, or anything ras_replay.mirror_step_ras takes (with limits=(min_new, max_new) given here)."""
    V = len(logits)
    eos = V - 1 if eos is None else eos
    min_new, max_new = limits_of(request) if limits is None else limits
    req = inner(request)
    case = state(history, pos, pos_base, min_new, max_new, eos)
    if case in (FINISHED, FORCED):
        return eos, case, False, False, {eos}, None
    x = np.asarray(logits, dtype=np.float64).copy()
    if case == SUPPRESSED:
        x[eos] = -np.inf
    w = delta / req.temperature
    c, amb, cands, kept = _first_draw(x, req, uniform01(req.seed, key, pos), w)
    window, max_repeats = RR.rule_of(req)
    token, redrawn, out = c, False, set()
    if window == 0 or req.top_k == 1:
        out = set(cands)
    else:
        u2 = uniform01(req.seed, key, pos | RR.RAS_STREAM)
        for first in sorted(cands if amb else {c}):
            if RR.repeats(history, pos, window, first) > max_repeats:
                t, near, _ = RR.redraw(x, req.temperature, u2, w)
                out |= near | {t}
                if first == c:
                    token, redrawn, amb = t, True, amb or bool(near)
            else:
                out.add(first)
    if case == SUPPRESSED:
        out.discard(eos)
        assert token != eos, 'the mirror itself drew a suppressed EOS'
    return token, case, redrawn, amb, out, step_logprob(x, req, token, redrawn, kept)


def replay_rows(sd, cfg, text, rows, prompt_len, max_new, request, delta=R.AUDIT_DELTA, keys=None):
    """ras_replay.replay_rows under the bounds: the rows of ONE utterance (n, width) int64 against the mirror over the oracle's
    logits, each step over the row's own history.  Returns (counted, ambiguous, redrawn, forced steps)."""
    eos = cfg.num_audio_tokens
    rows = torch.as_tensor(rows).cpu().long()
    keys = list(range(len(rows))) if keys is None else list(keys)
    counts = [counted_steps(r, prompt_len, max_new, eos) for r in rows]
    logits = R._forced_logits64(sd, cfg, text, [rows[r, :prompt_len + counts[r] - 1] for r in range(len(rows))]).numpy()
    counted = ambiguous = redrawn = forced = 0
    for r in range(len(rows)):
        hist = rows[r].tolist()
        for s in range(counts[r]):
            pos = prompt_len + s
            want, case, re, amb, cands, _ = mirror_step_bounded(logits[r, pos - 1], hist, request, keys[r], pos, prompt_len, delta, eos)
            got = hist[pos]
            if got != want and not (amb and got in cands):
                raise ReplayError(f'row {r} (key {keys[r]}) step {s} ({case}): the device drew {got}, the mirror {want} (redrawn: '
                                  f'{re}, ambiguous: {amb}, candidates {sorted(cands)}; {request})')
            counted, ambiguous, redrawn, forced = counted + 1, ambiguous + amb, redrawn + re, forced + (case == FORCED)
    return counted, ambiguous, redrawn, forced


def mirror_decode(sd, cfg, text, prompt_first, beams, max_new, request, delta=R.AUDIT_DELTA):
    """The mirror as the sampler under the bounds.  Returns (rows (beams, prompt_len + max_new) EOS-padded, scores (beams,)
    float64 — a forced step adds nothing —, counted, ambiguous, redrawn, forced steps)."""
    eos = cfg.num_audio_tokens
    prompt = torch.cat([torch.tensor([eos + 1]), prompt_first.cpu().long()])
    pl = len(prompt)
    rows = torch.full((beams, pl + max_new), eos, dtype=torch.int64)
    rows[:, :pl] = prompt
    scores = np.zeros(beams)
    live = list(range(beams))
    counted = ambiguous = redrawn = forced = 0
    for s in range(max_new):
        if not live:
            break
        logits = R._forced_logits64(sd, cfg, text, [rows[r, :pl + s] for r in live])[:, -1].numpy()
        for i, r in enumerate(list(live)):
            tok, case, re, amb, _, lp = mirror_step_bounded(logits[i], rows[r].tolist(), request, r, pl + s, pl, delta, eos)
            scores[r] += 0.0 if lp is None else lp
            rows[r, pl + s] = tok
            counted, ambiguous, redrawn, forced = counted + 1, ambiguous + amb, redrawn + re, forced + (case == FORCED)
            if tok == eos:
                live.remove(r)
    return rows, torch.from_numpy(scores), counted, ambiguous, redrawn, forced


# ---- the model cases (tests/test_length_bounds_cpu.py checks the mirror's own decode of them; tests/test_length_bounds_gpu.py)
# Four utterances of oracle_runners.audit_inputs('d128'), two beams each.  BOUNDS_REQUESTS[u]: (seed, top_k, temperature,
# window or 0, max_repeats, min_new, max_new); tok_p 1.0.  A plain request, min only, max only, and both around a
# RepetitionAware.  The seeds are sampling_replay's replay seeds, under which the mirror's decode stays within AMBIGUOUS_CAP.
BOUNDS_BEAMS = 2
BOUNDS_REQUESTS = [(1, 50, 1.0, 0, 0, 12, None), (2 ** 63 + 12345, 8, 0.8, 0, 0, None, 9), (7003, 8, 1.0, 10, 1, 5, 20),
                   (2 ** 64 - 2001, 50, 1.0, 0, 0, None, None)]


def bounds_request(u):
    from valle2_amd import Bounded, RepetitionAware, Sampling
    seed, top_k, temperature, window, max_repeats, min_new, max_new = BOUNDS_REQUESTS[u]
    base = (RepetitionAware(seed, top_k=top_k, tok_p=1.0, temperature=temperature, window=window, max_repeats=max_repeats)
            if window else Sampling(seed, top_k=top_k, tok_p=1.0, temperature=temperature))
    return base if min_new is None and max_new is None else Bounded(base, min_new=min_new, max_new=max_new)
