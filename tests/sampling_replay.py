"""A float64 mirror of the device sampler for utterances that carry a `valle2_amd.Sampling`: which token the device must
draw at every step of a row, given the row's own history.  CPU only (tests/test_row_sampling_cpu.py runs it as the sampler,
tests/test_row_sampling_gpu.py holds device rows against it).

What is restated here, from valle2_amd/csrc/elementwise.hip:
  * uniform01(seed, key, pos) in Python integers: the splitmix64 finaliser over seed + GOLDEN * ((key << 32) | (pos + 1)), its
    top 24 bits.  key is the beam index within the utterance, pos the audio position of the token being drawn (BOS at 0);
  * the kept set: every scaled logit (logit / temperature) >= the top_k-th largest, ties kept;
  * the walk over u * total: cumulative exp(x - max) over the kept set, the first entry whose inclusive sum exceeds it.  The
    order of the walk is the KERNEL's: with 0 < top_k < V and tok_p == 1 (the replay cases) both samplers walk the kept set in
    INDEX order (their fast path: radix select, no sort); otherwise in descending order, ties to the lower index first — the
    mirror takes the same branch (`descending`).  top-p itself is not mirrored (tok_p == 1.0 only, as in the existing audit);
  * top_k == 1: the arg-max, the lowest index on ties.
The logits are the oracle's (tests/oracle_runners._forced_logits64) over the row's own history.

A step is AMBIGUOUS when a device logit error of `delta` could change the token: every scaled logit may be off by w = delta /
temperature, so (a) two scores closer than 2 w around the top_k threshold may swap sides of it, and (b) a boundary of the
cumulative distribution may move by up to 2 w (one w on the entry's weight, one on the normaliser; the exact bound is 2 w c (1
- c) <= w / 2, the looser figure also covers the fp32 sums), so u within 2 w of a boundary may fall on either side.  At an
ambiguous step the device's token must be one of the neighbouring candidates (the two tokens that share the boundary; under a
threshold swap, the walk's token under each alternative kept set); at every other counted step it must be the mirror's.
Counted steps are audit_sampled_rows's: up to and including the draw of EOS, nothing at or beyond max_new.

AMBIGUOUS_CAP: at most 5 % of a case's counted steps may be ambiguous.  The worst replay case is top_k = 50: 49 inner
boundaries of width 4 w, about 2.5 % at temperature 0.8 and delta 1e-4; twice that keeps a case from passing while most of it
is excused.  top_k = 0 (a thousand boundaries) exceeds the cap by construction: the replay cases keep top_k in {8, 50}."""
from __future__ import annotations

import itertools

import numpy as np
import torch

from tests import oracle_runners as R

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
AMBIGUOUS_CAP = 0.05
MAX_ALTERNATIVES = 64        # kept sets tried at a step whose threshold is ambiguous (beyond: every near token is a candidate)


class ReplayError(AssertionError):
    """A device token that is neither the mirror's nor a neighbouring candidate of an ambiguous step."""


def uniform01(seed, key, pos):
    z = (seed + GOLDEN * (((key & 0xFFFFFFFF) << 32) | ((pos + 1) & 0xFFFFFFFF))) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def _walk(x, kept, u, w, descending):
    """The draw over the kept indices: (token, candidates when u lies within 2 w of a boundary — empty when it does not)."""
    kept = np.asarray(sorted(kept, key=(lambda i: (-x[i], i)) if descending else None), dtype=np.int64)
    e = np.exp(x[kept] - x[kept].max())
    cum = np.cumsum(e)
    total = cum[-1]
    hit = np.nonzero(cum > u * total)[0]
    j = int(hit[0]) if len(hit) else len(kept) - 1
    near = set()
    for b in np.nonzero(np.abs(cum[:-1] / total - u) <= 2 * w)[0]:        # inner boundaries only: 0 and 1 bound u itself
        near.update((int(kept[b]), int(kept[b + 1])))
    return int(kept[j]), near


def mirror_step(logits, top_k, temperature, u, delta, tok_p=1.0):
    """(token, ambiguous, candidates) of one draw over float64 `logits` (V,)."""
    if tok_p != 1.0:
        raise ValueError('sampling_replay: top-p is not mirrored (tok_p must be 1.0)')
    x = np.asarray(logits, dtype=np.float64) / temperature
    V, w = len(x), delta / temperature
    order = np.lexsort((np.arange(V), -x))                                 # descending, ties to the lower index first
    if top_k <= 0 or top_k >= V:
        tok, near = _walk(x, range(V), u, w, True)
        return tok, bool(near), near | {tok}
    kth = x[order[top_k - 1]]
    kept = [int(order[0])] if top_k == 1 else [int(i) for i in np.nonzero(x >= kth)[0]]
    tok, near = _walk(x, kept, u, w, False)
    cands, ambiguous = near | {tok}, bool(near)
    if kth - x[order[top_k]] <= 2 * w:                                     # the threshold may fall elsewhere on the device
        ambiguous = True
        sure = [int(i) for i in np.nonzero(x > kth + 2 * w)[0]]
        close = [int(i) for i in np.nonzero(np.abs(x - kth) <= 2 * w)[0]]
        need = top_k - len(sure)
        alts = list(itertools.islice(itertools.combinations(close, need), MAX_ALTERNATIVES + 1))
        if len(alts) > MAX_ALTERNATIVES:
            cands.update(close)
            alts = alts[:MAX_ALTERNATIVES]
        for alt in alts:
            t, n = _walk(x, sure + list(alt), u, w, False)
            cands |= n | {t}
    return tok, ambiguous, cands


def counted_steps(row, prompt_len, max_new, eos):
    gen = row[prompt_len:prompt_len + max_new]
    hit = (gen == eos).nonzero()
    if hit.numel():
        return int(hit[0]) + 1
    if gen.numel() < max_new:
        raise ValueError(f'sampling_replay: a row holds {gen.numel()} generated tokens without an EOS, max_new={max_new}')
    return max_new


def replay_rows(sd, cfg, text, rows, prompt_len, max_new, seed, top_k, temperature, delta=R.AUDIT_DELTA, keys=None):
    """Hold the rows of ONE utterance (n, width) int64 — BOS, prompt, generated, EOS padding; row j is beam keys[j] (default
    j) — against the mirror.  Returns (counted steps, ambiguous steps); raises ReplayError naming the row and step of a
    token that is not allowed."""
    eos = cfg.num_audio_tokens
    rows = torch.as_tensor(rows).cpu().long()
    keys = list(range(len(rows))) if keys is None else list(keys)
    counts = [counted_steps(r, prompt_len, max_new, eos) for r in rows]
    logits = R._forced_logits64(sd, cfg, text, [rows[r, :prompt_len + counts[r] - 1] for r in range(len(rows))]).numpy()
    counted = ambiguous = 0
    for r in range(len(rows)):
        for s in range(counts[r]):
            u = uniform01(seed, keys[r], prompt_len + s)
            want, amb, cands = mirror_step(logits[r, prompt_len - 1 + s], top_k, temperature, u, delta)
            got = int(rows[r, prompt_len + s])
            if got != want and not (amb and got in cands):
                raise ReplayError(f'row {r} (key {keys[r]}) step {s}: the device drew {got}, the mirror {want} (u = {u:.8f}, '
                                  f'top_k {top_k}, temperature {temperature}; ambiguous: {amb}, candidates {sorted(cands)})')
            counted += 1
            ambiguous += amb
    return counted, ambiguous


def mirror_decode(sd, cfg, text, prompt_first, beams, max_new, seed, top_k, temperature, delta=R.AUDIT_DELTA):
    """The mirror as the sampler: `beams` rows of one utterance decoded on the oracle's float64 logits.  Returns (rows (beams,
    prompt_len + max_new) EOS-padded, scores (beams,) float64 — the filtered log-probabilities of the counted draws —,
    counted steps, ambiguous steps)."""
    eos = cfg.num_audio_tokens
    prompt = torch.cat([torch.tensor([eos + 1]), prompt_first.cpu().long()])
    pl = len(prompt)
    rows = torch.full((beams, pl + max_new), eos, dtype=torch.int64)
    rows[:, :pl] = prompt
    scores = np.zeros(beams)
    live = list(range(beams))
    counted = ambiguous = 0
    for s in range(max_new):
        if not live:
            break
        logits = R._forced_logits64(sd, cfg, text, [rows[r, :pl + s] for r in live])[:, -1].numpy()
        for i, r in enumerate(list(live)):
            tok, amb, _ = mirror_step(logits[i], top_k, temperature, uniform01(seed, r, pl + s), delta)
            x = logits[i] / temperature
            V = len(x)
            keep = x >= np.sort(x)[V - top_k] if 1 < top_k < V else np.ones(V, bool)
            scores[r] += 0.0 if top_k == 1 else x[tok] - (x[keep].max() + np.log(np.exp(x[keep] - x[keep].max()).sum()))
            rows[r, pl + s] = tok
            counted += 1
            ambiguous += amb
            if tok == eos:
                live.remove(r)
    return rows, torch.from_numpy(scores), counted, ambiguous


def assert_in_topk_support(sd, cfg, text, rows, prompt_len, max_new, top_k, temperature, delta=R.AUDIT_DELTA):
    """Every counted token's scaled logit is at least the oracle's top_k-th largest minus delta / temperature (the support
    check of audit_sampled_rows, for cases whose scores are not audited: tok_p < 1)."""
    eos = cfg.num_audio_tokens
    rows = torch.as_tensor(rows).cpu().long()
    counts = [counted_steps(r, prompt_len, max_new, eos) for r in rows]
    logits = R._forced_logits64(sd, cfg, text, [rows[r, :prompt_len + counts[r] - 1] for r in range(len(rows))])
    for r in range(len(rows)):
        for s in range(counts[r]):
            x = logits[r, prompt_len - 1 + s] / temperature
            tok = int(rows[r, prompt_len + s])
            kth = torch.topk(x, top_k)[0][-1]
            assert x[tok] >= kth - delta / temperature, \
                f'row {r} step {s} token {tok}: scaled logit {float(x[tok]):.6f} below the oracle\'s {top_k}-th largest {float(kth):.6f}'
    return sum(counts)


# ---- the requests of the replay cases (tests/test_row_sampling_cpu.py, tests/test_row_sampling_gpu.py) ----------------------
# utterance u of oracle_runners.audit_inputs carries seed REPLAY_SEEDS[u] and filter REPLAY_FILTERS[u % 3] (top_k, temperature;
# tok_p 1.0).  The seeds were taken on the CPU: the mirror's own decode of the d128 audit model under them stays within
# AMBIGUOUS_CAP for every utterance (test_row_sampling_cpu.py asserts it).
REPLAY_FILTERS = [(50, 1.0), (8, 0.8), (8, 1.0)]
REPLAY_SEEDS = [1, 2 ** 63 + 12345, 7003, 2 ** 64 - 2001, 7005]
REPLAY_BEAMS = 4            # the most beams any case decodes: fewer beams are its first rows (beam j keeps key j)


def replay_request(u):
    """The valle2_amd.Sampling of utterance u."""
    from valle2_amd import Sampling
    top_k, temperature = REPLAY_FILTERS[u % len(REPLAY_FILTERS)]
    return Sampling(REPLAY_SEEDS[u], top_k=top_k, tok_p=1.0, temperature=temperature)
