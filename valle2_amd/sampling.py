"""Per-request sampling: what one utterance of a generate call asks of the sampler (seed, top-k, top-p, temperature, and with
RepetitionAware the redraw of a token that repeats), and the records the sample kernels read it from (include/valle_hip.h,
vh_row_sampling).  Pure Python, no device."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


# The NAR stage n draws on stream NAR_STREAM | n.  The generator's third argument is an audio position (< 5000) in the AR
# stage and the stream here, its second the beam index there and the frame index here: with the high bit set a request's AR
# draw (seed, beam j, position p) and its NAR draw (seed, frame t, stage n) never share a uniform (without it (j, p) == (t, n)
# would).
NAR_STREAM = 0x80000000


@dataclass(frozen=True)
class Sampling:
    """The sampling of ONE utterance: Sampling(seed, top_k=None, tok_p=None, temperature=None); None is the config's value.

    With it the utterance's draws are a function of (seed, beam index within the utterance, audio position) and its filter
    is its own: the same in generate(), generate_batch(beams=n) at any group index, generate_many and generate_queued at any
    slot, started or refilled, whatever else the call decodes.  top_k == 1 is greedy decoding for this utterance (the largest
    logit, the lowest index on ties, scores exactly 0); top_k == 0 keeps the whole vocabulary.  The NAR stage
    (ValleNAR.generate_batch(sampling=...)) takes the seed, the temperature and top_k == 1 from it: frame t of codebook n
    draws uniform01(seed, t, NAR_STREAM | n), whatever else the call refines.  Ranges (ValueError): seed an
    int in [0, 2**64), top_k an int >= 0, 0 < tok_p <= 1, temperature > 0."""
    seed: int
    top_k: int | None = None
    tok_p: float | None = None
    temperature: float | None = None

    def __post_init__(self):
        if not _is_int(self.seed) or not 0 <= self.seed < 2 ** 64:
            raise ValueError(f'Sampling: seed={self.seed!r} (an int in [0, 2**64))')
        if self.top_k is not None and (not _is_int(self.top_k) or not 0 <= self.top_k < 2 ** 31):
            raise ValueError(f'Sampling: top_k={self.top_k!r} (an int >= 0; 0 keeps the whole vocabulary, 1 is greedy)')
        if self.tok_p is not None and (not _is_real(self.tok_p) or not 0.0 < self.tok_p <= 1.0):
            raise ValueError(f'Sampling: tok_p={self.tok_p!r} (0 < tok_p <= 1)')
        if self.temperature is not None and (not _is_real(self.temperature) or not self.temperature > 0.0):
            raise ValueError(f'Sampling: temperature={self.temperature!r} (a finite number > 0)')

    def resolved(self, cfg):
        """(top_k, tok_p, temperature) with the config's values where this holds None."""
        top_k = int(cfg.top_k) if self.top_k is None else self.top_k
        tok_p = float(cfg.tok_p) if self.tok_p is None else float(self.tok_p)
        temperature = float(cfg.temperature) if self.temperature is None else float(self.temperature)
        if not temperature > 0.0:
            raise ValueError(f'Sampling: the config\'s temperature={temperature!r} must be > 0')
        return max(top_k, 0), tok_p, temperature

    def records(self, cfg, beams, first_key=0):
        """The (seed, key, top_k, top_p, temperature) of this utterance's `beams` rows (kernels.pack_row_sampling): beam j
        carries key first_key + j."""
        return [(self.seed, first_key + j) + self.resolved(cfg) for j in range(beams)]

    def nar_record(self, cfg):
        """The (seed, key, top_k, top_p, temperature) record the NAR stage sampler reads for this request
        (vh_categorical_rows_keyed): its seed, its temperature (the config's where this holds None), and top_k 1 only where its
        OWN top_k is 1 — the reference's NAR stage draws from the whole vocabulary (valle_nar.py:160), so the config's top_k,
        a request's other top_k values and tok_p do not filter it; the key is the frame's and travels with the row."""
        temperature = float(cfg.temperature) if self.temperature is None else float(self.temperature)
        if not temperature > 0.0:
            raise ValueError(f'Sampling: the config\'s temperature={temperature!r} must be > 0')
        return (self.seed, 0, 1 if self.top_k == 1 else 0, 1.0, temperature)


# A redraw at audio position p takes its uniform from position p | RAS_STREAM: bit 30 keeps it apart from every first draw
# (positions < 5000) and from the NAR stage's streams (bit 31).
RAS_STREAM = 0x40000000


@dataclass(frozen=True)
class RepetitionAware(Sampling):
    """Sampling with VALL-E 2's repetition-aware rule for the AR stage: RepetitionAware(seed, top_k=None, tok_p=None,
    temperature=None, window=10, max_repeats=1).

    The token c of audio position p is drawn as Sampling draws it.  If c stands MORE than `max_repeats` times among the row's
    own last `window` tokens (codes[max(1, p - window) .. p - 1]: the prompt counts, BOS does not, fewer than `window` early
    on), the token is drawn again from softmax(logits / temperature) over the whole vocabulary — no top-k, no top-p, index
    order, uniform01(seed, beam, p | RAS_STREAM) — and the beam's score takes that draw's unfiltered log-probability.  The
    redrawn token may be c again, or EOS.  A finished row keeps writing EOS.  The paper's ratio threshold t_r over a window K
    is max_repeats = floor(t_r * K): its K = 10, t_r = 0.1 are the defaults.  The draws stay a function of the request alone.

    An extension (the reference has no such rule) of the AR stage only: the NAR stage reads nar_record(), which is
    Sampling's, and ignores window and max_repeats.  Greedy decoding has nothing to redraw: an explicit top_k == 1 is a
    ValueError here, and so is top_k=None under a config whose top_k is 1 (raised where the request meets the config, before
    any device work).  Ranges (ValueError): window an int in [1, 2**31), max_repeats an int in [0, window) — a count of
    `window` tokens never exceeds `window`."""
    window: int = 10
    max_repeats: int = 1

    def __post_init__(self):
        super().__post_init__()
        if not _is_int(self.window) or not 1 <= self.window < 2 ** 31:
            raise ValueError(f'RepetitionAware: window={self.window!r} (an int in [1, 2**31))')
        if not _is_int(self.max_repeats) or not 0 <= self.max_repeats < self.window:
            raise ValueError(f'RepetitionAware: max_repeats={self.max_repeats!r} (an int in [0, window={self.window}): more '
                             'repeats than the window holds could never be counted)')
        if self.top_k == 1:
            raise ValueError('RepetitionAware: top_k=1 is greedy decoding, which draws nothing again (use Sampling)')

    def resolved(self, cfg):
        top_k, tok_p, temperature = super().resolved(cfg)
        if top_k == 1:
            raise ValueError(f'RepetitionAware: top_k={self.top_k!r} takes the config\'s top_k={cfg.top_k!r}, which is greedy '
                             'decoding and draws nothing again (give the request a top_k of its own, or use Sampling)')
        return top_k, tok_p, temperature

    def records(self, cfg, beams, first_key=0):
        """Sampling.records with the rule's two words: (seed, key, top_k, top_p, temperature, window, max_repeats)."""
        return [r + (self.window, self.max_repeats) for r in super().records(cfg, beams, first_key)]


@dataclass(frozen=True)
class Bounded:
    """Length bounds of ONE utterance in the AR stage, around its Sampling or RepetitionAware: Bounded(request, min_new=None,
    max_new=None).  It goes wherever a Sampling goes and mixes with plain requests in one call.

    With n the audio tokens a row has produced so far: while n < min_new EOS is outside the support — its score is -inf
    before top-k (ties included), top-p, the top_k == 1 arg-max, the draw and the repetition-aware redraw, and the beam's
    score takes the log-probability under the distribution without EOS — so every beam produces at least min_new tokens;
    once n >= max_new the token is EOS, forced: nothing is drawn or redrawn and the beam's score does not move (a forced
    token is not the model's choice), so every beam produces at most max_new tokens.  None (or 0 for min_new) switches a
    bound off.  The draws stay uniform01(seed, beam, position): the rows remain a function of the request alone, from
    every entry point, in any slot.  The NAR stage ignores the bounds: its length is the first layer's.

    Ranges (ValueError, before any device work): each bound an int in [0, 2**31) or None, max_new >= 1 when set, min_new <=
    max_new when both are set, and min_new within the call's own cap (generate_batch's max_new, else config.max_audio_len);
    a max_new above that cap is allowed and has no effect."""
    request: Sampling
    min_new: int | None = None
    max_new: int | None = None

    def __post_init__(self):
        if not isinstance(self.request, Sampling):
            raise ValueError(f'Bounded: request is {type(self.request).__name__}, not a valle2_amd.Sampling or RepetitionAware')
        for name in ('min_new', 'max_new'):
            v = getattr(self, name)
            if v is not None and (not _is_int(v) or not 0 <= v < 2 ** 31):
                raise ValueError(f'Bounded: {name}={v!r} (an int in [0, 2**31), or None)')
        if self.max_new is not None and self.max_new < 1:
            raise ValueError(f'Bounded: max_new={self.max_new!r} (at least 1 when set: a row always writes one token; None '
                             'switches the bound off)')
        if self.min_new is not None and self.max_new is not None and self.min_new > self.max_new:
            raise ValueError(f'Bounded: min_new={self.min_new} exceeds max_new={self.max_new}')

    # what a Sampling answers, from the request it wraps
    seed = property(lambda self: self.request.seed)
    top_k = property(lambda self: self.request.top_k)
    tok_p = property(lambda self: self.request.tok_p)
    temperature = property(lambda self: self.request.temperature)

    def resolved(self, cfg):
        return self.request.resolved(cfg)

    def records(self, cfg, beams, first_key=0):
        return self.request.records(cfg, beams, first_key)

    def nar_record(self, cfg):
        return self.request.nar_record(cfg)

    def limits(self, beams):
        """The (min_new, max_new) of this utterance's `beams` rows (kernels.pack_row_limits); 0 is a bound switched off."""
        return [(self.min_new or 0, self.max_new or 0)] * beams

    def check_cap(self, entry, cap):
        """min_new against the steps the call itself allows (ValueError)."""
        if (self.min_new or 0) > cap:
            raise ValueError(f'{entry}: Bounded min_new={self.min_new} exceeds the call\'s cap of {cap} new tokens (max_new of '
                             'generate_batch, else config.max_audio_len): no row could reach it')


def _request(s):
    return s.request if isinstance(s, KeyedRows) else s


def _unbounded(s):
    s = _request(s)
    return s.request if isinstance(s, Bounded) else s


def repetition_aware(sampling):
    """Whether any request of a call's sampling list (or None) carries the repetition-aware rule."""
    return any(isinstance(_unbounded(s), RepetitionAware) for s in sampling or ())


def bounded(sampling):
    """Whether any request of a call's sampling list (or None) carries a length bound that is switched on."""
    return any(isinstance(_request(s), Bounded) and any(v for v in _request(s).limits(1)[0]) for s in sampling or ())


def row_limits(sampling, beams):
    """[(min_new, max_new)] per decode row of a call's sampling list: a request's bounds for each of its beams, (0, 0) for a
    request without any (kernels.pack_row_limits)."""
    return [lim for s in sampling for lim in (s.limits(beams) if isinstance(s, (Bounded, KeyedRows)) else [(0, 0)] * beams)]


class KeyedRows(NamedTuple):
    """Internal: rows of a request handed over as utterances of their own, keyed from `first_key` on (generate() and the
    independent-rows fallback pass one utterance's beams as single rows: row j carries beam j).  Not part of the public
    interface: callers pass Sampling."""
    request: Sampling
    first_key: int

    def records(self, cfg, beams):
        return self.request.records(cfg, beams, self.first_key)

    def limits(self, beams):
        return self.request.limits(beams) if isinstance(self.request, Bounded) else [(0, 0)] * beams


def beam_rows(request, beams, first_key=0):
    """[KeyedRows] for the `beams` rows of `request` (a Sampling, a Bounded or a KeyedRows), one entry per row."""
    if isinstance(request, KeyedRows):
        request, first_key = request.request, request.first_key + first_key
    return [KeyedRows(request, first_key + j) for j in range(beams)]


def check_list(entry, sampling, n, what='utterance', cfg=None, cap=None):
    """None when no entry of `sampling` (None, or a list of n) is a Sampling (or a Bounded around one), the list when every
    one is; a mix is a ValueError naming the first without one.  With cfg every request is also resolved against the config,
    so what the two cannot do together (Sampling.resolved, RepetitionAware.resolved) is said here, and a Bounded's min_new is
    held against the call's cap (`cap`, else cfg.max_audio_len)."""
    if sampling is None:
        return None
    sampling = list(sampling)
    if len(sampling) != n:
        raise ValueError(f'{entry}: sampling holds {len(sampling)} entries for {n} {what}s (one Sampling each)')
    for i, s in enumerate(sampling):
        if s is not None and not isinstance(s, (Sampling, Bounded, KeyedRows)):
            raise ValueError(f'{entry}: sampling of {what} {i} is {type(s).__name__}, not a valle2_amd.Sampling')
    if all(s is None for s in sampling):
        return None
    for i, s in enumerate(sampling):
        if s is None:
            raise ValueError(f'{entry}: {what} {i} carries no Sampling and others do: either every {what} of a call '
                             'carries one or none does')
    if cfg is not None:
        for s in sampling:
            _request(s).resolved(cfg)
            if isinstance(_request(s), Bounded):
                _request(s).check_cap(entry, int(cfg.max_audio_len) if cap is None else int(cap))
    return sampling


def of_utterances(entry, utterances, cfg=None):
    """check_list over the optional fourth element of [(prompt_tokens, prompt_codes, target_tokens[, sampling]), ...]."""
    utterances = list(utterances)
    for i, u in enumerate(utterances):
        if len(u) not in (3, 4):
            raise ValueError(f'{entry}: utterance {i} has {len(u)} elements: (prompt_tokens, prompt_codes, target_tokens) '
                             'with an optional Sampling as the fourth')
    return check_list(entry, [u[3] if len(u) == 4 else None for u in utterances], len(utterances), cfg=cfg)
