"""Host side of AR generation, between ValleAR's public methods (valle_ar.py) and engine.ArDecoder: what a call decodes
on (`plan_decode`, pure Python), the buffers its captured graphs point at (`DecodeState`, kept per shape on the model), the
prompt pass, and the decode loops of generate_batch and generate_queued."""
from __future__ import annotations

import os
import threading
import time
from dataclasses import dataclass

import torch

from . import _lib, kernels
from . import sampling as _sampling
from .engine import (MAX_DECODE_D_MODEL, ArDecoder, ForwardScratch, ForwardScratch16, KVCache, PromptRows, QueueSchedule, StepSampler,
                     cached_decode_supported, ffn_fused_width, group_prefix_cap, grouped_prompts_fit, perf_forward_supported,
                     packed_forward_for, queue_steps_cap, transformer_forward, transformer_forward_bf16)
from .utils import get_best_beam

EOS_POLL = 32
MAX_DECODE_ROWS = 64      # rows per decode launch (vh_ar_decoder: 1..64)
# generate(): the beams of one utterance share its prompt K/V (read once per step for all beams).  VALLE2_SHARED_PROMPT=0
# decodes the beams as independent rows (round 4's form: the A/B arm, and what generate_batch does for distinct rows).
SHARED_PROMPT = os.environ.get('VALLE2_SHARED_PROMPT', '1') != '0'
_DECODER_ENV = ('VALLE2_HEAD_FUSED', 'VALLE2_SHARED_SPLIT', 'VALLE2_FOLD_LN', 'VALLE2_DECODE_W16')   # environment knobs read when a decoder is built
DECODER_SLOTS = int(os.environ.get('VALLE2_DECODER_SLOTS', '2'))    # decoders kept per model (0: build one per call, as before)
_SLOT_LOCK = threading.Lock()

# what a call decodes on (DecodePlan.kind); the caches of each are written down once, in _caches
RECOMPUTE_GENERAL = 'RECOMPUTE_GENERAL'    # a head width the cached decoder does not serve: every step recomputes on the general kernels
ROWS_HD = 'ROWS_HD'                        # another head width on the cached decoder (_hd kernels): fp32 rows of that width
SHARED = 'SHARED'                          # shared_prompt=True: ONE row through the prompt pass, its K/V read once per step for all rows
GROUPED = 'GROUPED'                        # beams > 1 and the queue: one prefix row per utterance, read once per step for its beams
ROWS_PERF_PREFILL = 'ROWS_PERF_PREFILL'    # perf mode: the prompt pass on the 16-bit matrix cores straight into 16-bit rows
ROWS = 'ROWS'                              # independent fp32 rows (use_kv_cache=False recomputes over them; perf_mode='kv' narrows them once)


def roundup32(n):
    """Whole 32-key chunks per (row, head) block (the ring kernel reads ahead in chunks of 32 keys)."""
    return (n + 31) // 32 * 32


# ---- refusals: pure Python, no device ------------------------------------------------------------------------------------
def _check_int(entry, name, value):
    if not isinstance(value, int) or isinstance(value, bool) or value < 1:
        raise ValueError(f'{entry}: {name}={value!r} (an integer >= 1)')


def _check_grouped_decoder(entry, cfg, beams, needs):
    if not cfg.use_kv_cache or cfg.d_model != cfg.n_heads * kernels.HEAD_DIM or cfg.d_model > MAX_DECODE_D_MODEL:
        raise ValueError(f'{entry}: beams={beams} with use_kv_cache={cfg.use_kv_cache}, d_model={cfg.d_model}, '
                         f'n_heads={cfg.n_heads}: {needs} the cached decoder at head width '
                         f'{kernels.HEAD_DIM} (d_model <= {MAX_DECODE_D_MODEL})')


def check_sampling(sampling, n, forced=None, cfg=None, max_new=None):
    """The refusals of generate_batch(sampling=...): one Sampling per utterance or none at all, each one the config can
    resolve (cfg), a Bounded's min_new within the call's cap (max_new, else the config's max_audio_len), and no teacher
    forcing.  Returns the list, or None for a call without row sampling."""
    sampling = _sampling.check_list('generate_batch', sampling, n, cfg=cfg, cap=max_new)
    if sampling is not None and forced is not None:
        raise ValueError('generate_batch: sampling with forced: teacher forcing appends the given tokens, nothing is drawn')
    return sampling


def check_beams(cfg, beams, shared_prompt=False, perf_mode=False, forced=None):
    """The refusals of generate_batch(beams=n)."""
    _check_int('generate_batch', 'beams', beams)
    if beams == 1:
        return
    if beams > MAX_DECODE_ROWS:
        raise ValueError(f'generate_batch: beams={beams}: the beams of an utterance decode in one launch of at most '
                         f'{MAX_DECODE_ROWS} rows')
    if shared_prompt:
        raise ValueError(f'generate_batch: beams={beams} with shared_prompt=True: shared_prompt takes the replicated rows of '
                         'ONE utterance, beams takes the utterances themselves and replicates them')
    if perf_mode:
        raise ValueError(f'generate_batch: beams={beams} with perf_mode={perf_mode!r}: grouped shared prompts decode on fp32 '
                         'caches only (perf_mode serves generate() and independent rows)')
    if forced is not None:
        raise ValueError(f'generate_batch: beams={beams} with forced: teacher forcing drives independent rows')
    _check_grouped_decoder('generate_batch', cfg, beams, 'grouped shared prompts need')


def check_queued(cfg, beams, slots):
    """The refusals of generate_queued."""
    _check_int('generate_queued', 'beams', beams)
    if slots is not None:
        _check_int('generate_queued', 'slots', slots)
    if (1 if slots is None else slots) * beams > MAX_DECODE_ROWS:
        raise ValueError(f'generate_queued: slots={slots} with beams={beams}: the slots decode in one launch of at most '
                         f'{MAX_DECODE_ROWS} rows (1 <= slots * beams <= {MAX_DECODE_ROWS})')
    _check_grouped_decoder('generate_queued', cfg, beams, 'queued decoding needs')


def check_forms(cfg, perf_mode=False, by_hand=False, shared_prompt=False):
    """The refusals of generate_batch that need only the config and which form of the decoder the call asks for
    (by_hand: profile_attn or forced)."""
    # a head width other than 64 (modules.py:109-111 allows it): a multiple of 4 from 16 to 256 at d_model <= 1024 decodes on
    # the cached decoder with the _hd kernels (ROWS_HD; the prompt pass runs on the general kernels and fills the cache);
    # any other width recomputes every step on the general kernels (RECOMPUTE_GENERAL)
    other_width = cfg.d_model != cfg.n_heads * kernels.HEAD_DIM
    hd_cached = other_width and cached_decode_supported(cfg)
    if not other_width and cfg.d_model > MAX_DECODE_D_MODEL:
        # (cached_decode_supported is False there, but the recompute path's vh_layernorm ends at 4096 as well)
        raise ValueError(f'd_model {cfg.d_model}: generation serves d_model <= {MAX_DECODE_D_MODEL} (the LayerNorm kernel of '
                         'the prompt pass and the decode GEMMs end there)')
    no_cache = not cfg.use_kv_cache or (other_width and not hd_cached)
    if no_cache and (perf_mode or by_hand or shared_prompt):
        raise ValueError('use_kv_cache=False (or a head width the cached decoder does not serve) recomputes every step '
                         'from scratch: perf_mode / profile_attn / forced / shared_prompt belong to the cached decoder')
    if hd_cached and (perf_mode or shared_prompt):
        raise ValueError(f'head width {cfg.d_model // cfg.n_heads}: perf_mode and shared_prompt are width-64 forms of the cached decoder '
                         '(this width decodes fp32 rows, each with its own prompt K/V)')
    if perf_mode and cfg.d_model > 1024:
        raise ValueError(f'd_model {cfg.d_model}: perf_mode (the bf16 K/V cache of the decode step) serves d_model <= 1024; '
                         'wider models decode fp32')


# ---- the plan of one call --------------------------------------------------------------------------------------------------
@dataclass
class DecodePlan:
    """Shapes and modes of one decode call (generate_batch, or the rows generate_queued starts with): everything its
    helpers, its caches and its slot key follow from."""
    kind: str             # one of the six above
    G: int                # utterances
    beams: int            # rows of each (1 unless GROUPED)
    B: int                # decode rows, G * beams
    max_new: int          # steps a row may run
    txs: list             # per utterance: text length
    pls: list             # per utterance: BOS + prompt
    ctx: list             # per utterance: text + BOS + prompt, the keys of its prompt pass
    row_pls: list         # pls per decode row: where its generated tokens start
    ragged: bool          # utterances differ in text or prompt length
    s0: int               # longest context
    s_max: int            # keys of a row cache that holds prompt and generated rows
    pl_max: int
    cap: int              # GROUPED: the prefix capacity per utterance (0 otherwise)
    fits: bool            # GROUPED: the capacity is within the records one merge serves (True otherwise)
    codes_width: int
    cache_len0: list      # per decode row: rows in the cache its steps append to before the first sample (+1 by the sample step)
    prefix_spec: tuple | None   # (rows, keys, dtype, head width) of the shared-prompt prefix cache, None without one
    rows_spec: tuple | None     # the same of the cache the decode rows append to
    perf_mode: object     # False, True or 'kv', as given
    prefill_bf16: bool    # the prompt pass runs on the 16-bit matrix cores (perf_mode True where they serve the shape)
    no_cache: bool        # every step recomputes the whole sequence
    use_graph: bool
    queued: bool          # the plan of generate_queued
    slot_eligible: bool   # the decoder may survive the call in a slot of the model
    row_sampling: bool = False   # every utterance carries its own Sampling: the sampler reads per-row records, not the config
    row_limits: bool = False     # a request of the call carries a length bound (sampling.Bounded): vh_row_limits beside the records


def _caches(kind, cfg, G, B, s0, s_max, cap, max_new, perf_mode):
    """(prefix_spec, rows_spec) of a kind: the one place that says which caches a call gets."""
    f32, hd = torch.float32, kernels.HEAD_DIM
    suffix = roundup32(max_new + 1)                       # generated rows only
    if kind == RECOMPUTE_GENERAL:
        return None, None
    if kind == ROWS_HD:                                   # (no shared / perf form)
        return None, (B, s_max, f32, cfg.d_model // cfg.n_heads)
    if kind == SHARED:
        # ONE row through the prompt pass: its K/V are the prefix every beam reads; the beams' cache holds generated rows only
        # (perf mode: both 16-bit)
        dtype = kernels.H16 if perf_mode else f32
        return (1, roundup32(s0), dtype, hd), (B, suffix, dtype, hd)
    if kind == GROUPED:
        # one row per UTTERANCE through the prompt pass, into a prefix cache of `cap` keys per utterance
        return (G, cap, f32, hd), (B, suffix, f32, hd)
    if kind == ROWS_PERF_PREFILL:
        return None, (B, s_max, kernels.H16, hd)
    # (perf_mode='kv': the fp32 prompt K/V, narrowed once to the 16-bit cache of s_max keys after the pass)
    return None, (B, s0 if perf_mode else s_max, f32, hd)


def plan_decode(cfg, txs, pls, *, max_new, beams=1, shared_prompt=False, perf_mode=False, use_graph=True, by_hand=False,
                queued=False, cap=None, pos_limits=None, row_sampling=False, row_limits=False):
    """The DecodePlan of a call over utterances of text lengths `txs` and prompt lengths `pls` (BOS included).  by_hand:
    profile_attn or forced, the forms that drive the decoder themselves.  queued: generate_queued's rows (GROUPED whatever
    `beams`, `cap` given: of the longest prompt of the whole list, max_new: its steps cap).  pos_limits: (audio, text) rows
    of the positional tables.  row_sampling: the utterances carry a Sampling each."""
    G, B = len(txs), len(txs) * beams
    other_width = cfg.d_model != cfg.n_heads * kernels.HEAD_DIM
    hd_cached = other_width and cached_decode_supported(cfg)
    no_cache = not cfg.use_kv_cache or (other_width and not hd_cached)
    ctx = [t + p for t, p in zip(txs, pls)]
    ragged = len(set(txs)) > 1 or len(set(pls)) > 1
    pl_max, s0 = max(pls), max(ctx)
    if pos_limits is not None and (pl_max + max_new > pos_limits[0] or max(txs) > pos_limits[1]):
        raise _lib.VhError('sequence exceeds the positional table (max_len 5000)')
    if shared_prompt and ragged:
        raise ValueError('shared_prompt: identical rows (equal text and prompt lengths)')
    prefill_bf16 = bool(perf_mode) and perf_mode != 'kv' and perf_forward_supported(cfg)
    kind = (ROWS_HD if hd_cached else RECOMPUTE_GENERAL if other_width else SHARED if shared_prompt
            else GROUPED if beams > 1 or queued else ROWS_PERF_PREFILL if prefill_bf16 else ROWS)
    grouped = kind == GROUPED
    # the prefix capacity (what the decoder is built and keyed for): the longest context rounded up to 128 keys
    cap = (group_prefix_cap(s0) if cap is None else cap) if grouped else 0
    s_max = roundup32(s0 + max_new)
    prefix_spec, rows_spec = _caches(kind, cfg, G, B, s0, s_max, cap, max_new, perf_mode)
    return DecodePlan(
        kind=kind, G=G, beams=beams, B=B, max_new=max_new, txs=list(txs), pls=list(pls), ctx=ctx,
        row_pls=[p for p in pls for _ in range(beams)], ragged=ragged, s0=s0, s_max=s_max, pl_max=pl_max, cap=cap,
        fits=not grouped or grouped_prompts_fit(B, cfg.n_heads, cap),
        # (the queue's rows stand one past their last whole poll)
        codes_width=(cap if grouped else pl_max) + max_new + (1 if queued else 0),
        # shared prompts: generated rows only
        cache_len0=[-1] * B if kind in (SHARED, GROUPED) else [c - 1 for c in ctx],
        prefix_spec=prefix_spec, rows_spec=rows_spec, perf_mode=perf_mode, prefill_bf16=prefill_bf16, no_cache=no_cache,
        use_graph=bool(use_graph), queued=queued,
        # (perf_mode='kv' with rows of their own narrows into a fresh cache per call: no slot; over a shared prompt it narrows
        # into the slot's 16-bit prefix)
        slot_eligible=not (no_cache or by_hand or (bool(perf_mode) and not prefill_bf16 and kind != SHARED)),
        row_sampling=bool(row_sampling), row_limits=bool(row_sampling and row_limits))


def slot_key(plan, cfg, device, weights):
    """What a kept decoder was built for, or None for a call that keeps none.  GROUPED: the prefix CAPACITY stands for every
    length — prompts of other lengths under the same capacity reuse the slot and its captured graphs.  weights: a value that
    changes with the model's parameters (weights_key)."""
    if not plan.slot_eligible:
        return None
    grouped = plan.kind == GROUPED
    return (plan.kind, plan.queued, plan.B, plan.s0 if plan.kind == SHARED else None, None if grouped else plan.s_max,
            plan.codes_width, plan.max_new, (plan.G, plan.beams, plan.cap) if grouped else None,
            int(cfg.max_audio_len) if plan.queued else None, plan.prefill_bf16, bool(plan.perf_mode), plan.use_graph,
            int(cfg.top_k), float(cfg.tok_p), float(cfg.temperature), str(device), _lib.TUNING_EPOCH,
            tuple(os.environ.get(k) for k in _DECODER_ENV), weights) + (('row_sampling',) if plan.row_sampling else ()) + \
        (('row_limits',) if plan.row_limits else ())    # (a decoder with the limits array attached: measured dearer per launch)


def weights_key(model):
    """Changes whenever a pointer or a value the decoder's tables were built from may have changed."""
    from . import engine
    return (engine._WEIGHTS_EPOCH,) + tuple((p.data_ptr(), p._version) for p in model.parameters())


# ---- the state of one call, kept per shape ---------------------------------------------------------------------------------
class DecodeState:
    """Everything of a decode call that a captured decode graph points at, kept per SHAPE on the model (`_decode_slots`) so
    that the next call of the same shape neither allocates, nor builds a decoder, nor captures (~1.7 ms of
    capture + the construction per call, which a 2 ms prompt pass no longer hides): the token buffer, the K/V caches, the
    per-row counters, the queue's poll buffers and the ArDecoder with its graphs and workspaces.  A slot is used by one call
    at a time (`busy`); a call that keeps nothing works on a state of its own."""

    def __init__(self):
        self.codes = self.cache_len = self.audio_pos = self.pos_base = self.group_len = None
        self.poll_dev = self.poll_host = self.first_len = None            # generate_queued only
        self.row_sampling = None                                          # (B, 32) uint8: vh_row_sampling records of a call with Sampling
        self.row_limits = None                                            # (B, 8) uint8 beside them when a request carries a bound: vh_row_limits (zeros: none)
        self.cache = self.prefix = self.dec = None
        self.prompt_rows = (False, 0)                                     # the last prompt pass: (packed, rows it computed)
        self.reused = self.busy = False
        self.uses = 0

    def arm(self, model, plan, sampling=None):
        """Ready for a call of `plan`: allocates on first use, refills in place where an earlier call left its buffers and
        decoder.  The small host-to-device copies and the decoder's reset go up BEFORE the prompt pass is enqueued (a copy
        behind it would hold the host until the pass has finished).  sampling: one Sampling per utterance (plan.row_sampling)
        — row g * beams + j gets (seed_g, j, top_k_g, tok_p_g, temperature_g) and nothing is drawn from torch's generator.
        Returns the call's sampling seed (0 with row sampling)."""
        cfg, dev = model.config, model.device
        i32 = dict(dtype=torch.int32)
        host = {'cache_len': torch.tensor(plan.cache_len0, **i32), 'audio_pos': torch.tensor(plan.row_pls, **i32)}
        if plan.kind == GROUPED:
            host['group_len'] = torch.tensor(plan.ctx, **i32)     # the prompts' lengths, where the (captured) decode steps read them
        # sampling seed drawn from torch's generator, so torch.manual_seed() makes a run repeatable
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if cfg.top_k != 1 and not plan.row_sampling else 0
        if plan.row_sampling:
            host['row_sampling'] = kernels.pack_row_sampling([r for s in sampling for r in s.records(cfg, plan.beams)])
        if plan.row_limits:
            # beside the records whenever ANY request of the call carries a bound (zeros for those without): the decoder of
            # such a call has the array attached before capture and serves every mix of bounds
            host['row_limits'] = kernels.pack_row_limits(_sampling.row_limits(sampling, plan.beams))
        self.reused = self.dec is not None
        if self.reused:
            self.codes.fill_(model.eos_token)
            for name, t in host.items():
                getattr(self, name).copy_(t, non_blocking=True)
            self.pos_base.copy_(self.audio_pos)
            self.dec.reset(seed)
        else:
            self.codes = torch.full((plan.B, plan.codes_width), model.eos_token, device=dev, dtype=torch.int64)
            for name, t in host.items():
                setattr(self, name, _lib.to_device_async(t, dev).clone())    # (its own storage: it outlives the call in the slot)
            self.pos_base = self.audio_pos.clone()
            self.prefix, self.cache = (spec and KVCache(cfg.num_layers, spec[0], cfg.n_heads, spec[1], dev, dtype=spec[2], head_dim=spec[3])
                                       for spec in (plan.prefix_spec, plan.rows_spec))
            if plan.queued:
                self.poll_dev = torch.zeros(4 + 2 * plan.G, device=dev, **i32)
                self.poll_host = torch.zeros(4 + 2 * plan.G, **i32).pin_memory()
                self.first_len = torch.zeros(plan.beams, device=dev, **i32)   # stands in for cache_len at a refill's first sample
        self.codes[:, 0] = model.bos_token                                 # valle_ar.py:115-117
        self.uses += 1
        return seed

    def decoder(self, model, plan, seed):
        """The call's decoder, built over the armed buffers AFTER the prompt pass is enqueued (host work the pass hides)."""
        if self.dec is None and plan.kind == RECOMPUTE_GENERAL:
            self.dec = StepSampler(model, plan.B, self.codes, self.cache_len, self.audio_pos, self.pos_base, seed=seed,
                                   row_sampling=self.row_sampling, row_limits=self.row_limits)
        elif self.dec is None:
            self.dec = ArDecoder(model, plan.B, self.cache.s_max, self.codes, self.cache, self.cache_len, self.audio_pos,
                                 self.pos_base, use_graph=plan.use_graph and not plan.no_cache, seed=seed, prefix=self.prefix,
                                 prefix_len=plan.s0, row_sampling=self.row_sampling, row_limits=self.row_limits,
                                 **(dict(prefix_lens=self.group_len, prefix_cap=plan.cap, beams=plan.beams) if plan.kind == GROUPED else {}))
        return self.dec

    def close(self):
        if self.dec is not None:
            self.dec.close()
            self.dec = None


def acquire_state(model, key):
    """The free slot of this key (LRU order), or a new one (the oldest free slot beyond DECODER_SLOTS is dropped); a state
    that belongs to the call alone when it keeps none (key None, slots off, or another host thread is decoding this shape
    right now)."""
    if key is None or DECODER_SLOTS <= 0:
        return DecodeState()
    with _SLOT_LOCK:
        slots = model.__dict__.setdefault('_decode_slots', {})
        slot = slots.pop(key, None)
        if slot is not None and slot.busy:
            slots[key] = slot
            return DecodeState()
        if slot is None:
            slot = DecodeState()
            free = [k for k, v in slots.items() if not v.busy]
            while len(slots) >= DECODER_SLOTS and free:
                slots.pop(free.pop(0)).close()
        slot.busy = True
        slots[key] = slot                                # most recently used last
        return slot


def release_state(model, key, state, ok):
    """The end of a call: a state of its own is closed; a slot is freed, and dropped when the call failed (a failed call
    leaves nothing behind)."""
    if not state.busy:
        state.close()
        return
    with _SLOT_LOCK:
        state.busy = False
        if not ok:
            model.__dict__.get('_decode_slots', {}).pop(key, None)
            state.close()


def release_decoders(model):
    with _SLOT_LOCK:
        for slot in model.__dict__.pop('_decode_slots', {}).values():
            if not slot.busy:
                slot.close()


# ---- utterances in, best beams out ----------------------------------------------------------------------------------------
def unpack_utterances(utterances):
    """[(prompt_tokens, prompt_codes, target_tokens | None[, sampling]), ...] -> (texts, firsts): per utterance the text ids
    the model reads (prompt text, then the target's) and the first codebook of its prompt (valle_ar.py:107-121).  The optional
    fourth element is the utterance's Sampling (sampling.of_utterances reads it)."""
    texts, firsts = [], []
    for prompt_tokens, prompt_codes, target_tokens, *_ in utterances:
        assert prompt_tokens.dim() == 1, 'Prompt tokens should be 1D tensor.'
        assert prompt_codes.dim() == 2, 'Prompt codes should be 2D tensor.'
        if target_tokens is not None:
            assert target_tokens.dim() == 1, 'Target tokens should be 1D tensor.'
        texts.append(prompt_tokens if target_tokens is None else torch.cat((prompt_tokens, target_tokens), dim=0))
        firsts.append(prompt_codes[..., 0])
    return texts, firsts


def best_beam_tokens(model, rows, sum_logprobs, prompt_len):
    """beams -> one sequence (valle_ar.py:174-180): the best beam with the prompt cut and EOS stripped; with top_k=1 every
    log-prob is exactly 0."""
    best = get_best_beam(rows, sum_logprobs, model.eos_token, model.config.length_penalty)[prompt_len:]
    return best[best != model.eos_token]


# ---- the prompt pass and the decode loops -----------------------------------------------------------------------------------
def _switch(model, attribute, variable):
    """A switch of the model: its attribute (True / False), or, while that is None, `variable`=1 in the environment of the call."""
    switch = getattr(model, attribute, None)
    return os.environ.get(variable, '0') == '1' if switch is None else bool(switch)


def packed_prompt_on(model):
    """The switch of the packed prompt pass: `model.packed_prompt` (ValleAR's class attribute; True / False), or, while that
    is None, VALLE2_PACKED_PROMPT=1 in the environment of the call."""
    return _switch(model, 'packed_prompt', 'VALLE2_PACKED_PROMPT')


def packed_prompt_qualifies(kind, perf_mode, head_dim, forced, ragged, no_cache=False):
    """Whether a call's prompt pass may run over packed rows (pure: no model, no device): utterances of different lengths
    (equal ones have no padding to drop), the fp32 parity path, head width 64, cached decoding on rows or grouped prefixes of
    their own (SHARED has a single row) and no teacher forcing.  Every other call runs the padded pass."""
    return bool(ragged) and not perf_mode and head_dim == kernels.HEAD_DIM and not no_cache and not forced and kind in (ROWS, GROUPED)


def packed_prompt_perf_on(model):
    """The switch of the packed prompt pass in PERF MODE, a switch of its own beside `packed_prompt_on`:
    `model.packed_prompt_perf` (ValleAR's class attribute; True / False), or, while that is None, VALLE2_PACKED_PROMPT_PERF=1 in
    the environment of the call."""
    return _switch(model, 'packed_prompt_perf', 'VALLE2_PACKED_PROMPT_PERF')


def packed_prompt_perf_qualifies(kind, perf_mode, head_dim, forced, ragged, no_cache=False):
    """`packed_prompt_qualifies` for perf mode (pure: no model, no device): utterances of different lengths, perf_mode True or
    'kv', head width 64, cached decoding on independent rows — ROWS_PERF_PREFILL (the 16-bit packed pass into the 16-bit row
    cache) or ROWS ('kv', or a shape the 16-bit stack does not take: the fp32 packed pass, narrowed once) — and no teacher
    forcing.  SHARED has a single row, grouped and queued calls refuse perf_mode; every other call runs the padded pass."""
    return (bool(ragged) and bool(perf_mode) and head_dim == kernels.HEAD_DIM and not no_cache and not forced
            and kind in (ROWS_PERF_PREFILL, ROWS))


def _write_prompts(codes, first_codes, n):
    """codes[g * n:(g + 1) * n, 1:1 + len(first_codes[g])] = first_codes[g] for every utterance in one scatter (the padded pass
    writes them utterance by utterance)."""
    lens = torch.tensor([int(c.shape[0]) for c in first_codes], dtype=torch.int64)
    total = int(lens.sum())
    if total == 0:
        return
    g = torch.repeat_interleave(torch.arange(len(first_codes)), lens)
    t = torch.arange(total) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    dest = (g * n * codes.shape[1] + 1 + t).unsqueeze(0) + (torch.arange(n) * codes.shape[1]).unsqueeze(1)
    codes.view(-1).index_copy_(0, _lib.to_device_async(dest.reshape(-1), codes.device), torch.cat(first_codes).repeat(n))


def packed_pass(model, texts, txs, pls, codes, into, dst_rows):
    """The prompt pass of several utterances over PACKED rows: one embed launch (`vh_embed_nar_packed` with one codebook: text
    rows, then BOS + prompt rows, positions restarting per stream), one packed prefix-LM forward into a transient one-row
    cache of sum(ctx) rows and one `vh_kv_unpack` into rows `dst_rows` of `into` (a row cache or a grouped prefix cache).
    A 16-bit `into` (perf mode's row cache) takes the 16-bit forms of the last two: `transformer_forward_packed_lm_bf16` into a
    transient 16-bit stream and `vh_kv_unpack_bf16`.
    codes (G, >= max(pls)): row g holds BOS + prompt g.  Returns the (G, d) hidden rows of the utterances' last positions."""
    cfg, dev, d = model.config, model.device, model.config.d_model
    rows = PromptRows(txs, pls, dst_rows, dev)
    G, width = rows.n_seg, max(rows.max_x_len, 1)
    flat = torch.cat(texts)
    if flat.numel():
        # the text ids as the (G, longest text) rows the embed kernel indexes: one gather of the concatenated ids
        lens = torch.tensor(rows.x_lens, dtype=torch.int64)
        idx = (torch.cumsum(lens, 0) - lens).unsqueeze(1) + torch.minimum(torch.arange(width).unsqueeze(0), (lens - 1).clamp(min=0).unsqueeze(1))
        tokens = flat.index_select(0, _lib.to_device_async(idx.clamp(max=flat.numel() - 1).reshape(-1), dev)).view(G, width)
    else:
        tokens = torch.zeros(G, width, device=dev, dtype=torch.int64)
    x = torch.empty(rows.rows, d, device=dev, dtype=torch.float32)
    kernels.embed_nar_packed(tokens, codes.unsqueeze(-1), model.tokens_emb.weight.detach(), [model.audio_emb.weight.detach()], 1,
                             model.tokens_position_emb.pe, model.audio_position_emb.pe, rows, x)
    stream_cache = KVCache(cfg.num_layers, 1, cfg.n_heads, rows.rows, dev, dtype=kernels.H16 if into.bf16 else torch.float32)
    packed_forward_for(stream_cache, lm=True)(model.transformer, x, stream_cache, rows,
                                              scratch=(ForwardScratch16 if into.bf16 else ForwardScratch)(rows.rows, d, cfg.dim_feedforward, dev))
    stream_cache.unpack_into(into, rows.seg_start, rows.seg_len, rows.dst_row)
    return x.index_select(0, rows.last_rows)


def prompt_pass(model, plan, state, texts, first_codes, forced=False):
    """Step 0 (valle_ar.py:143-155 at kv_cache=None): embed and run the whole prompt into the armed state's caches.  Row b is
    laid out [text_b | BOS + prompt_b | padding]; the prefix-LM mask takes per-row lengths.  Returns the last hidden row of
    every decode row, the length arguments of the pass and the stacked text ids of equal-length rows (the recompute steps
    run the same pass again).  With the packed switch on (`packed_prompt_on`) a call that qualifies
    (`packed_prompt_qualifies`) runs `packed_pass` instead: no padding row is computed; `state.prompt_rows` says which.  Perf
    mode has a switch of its own (`packed_prompt_perf_on`, `packed_prompt_perf_qualifies`): ROWS_PERF_PREFILL runs the 16-bit
    packed pass straight into the 16-bit row cache, ROWS the fp32 packed pass into the fp32 cache of s0 keys, narrowed once as
    after the padded pass."""
    cfg, dev, d = model.config, model.device, model.config.d_model
    B, s0, n, codes = plan.B, plan.s0, plan.beams, state.codes
    i32 = dict(device=dev, dtype=torch.int32)
    rows = 1 if plan.kind == SHARED else plan.G
    text_ids = None
    state.prompt_rows = (False, rows * s0)
    rule = (plan.kind, plan.perf_mode, d // cfg.n_heads, forced, plan.ragged, plan.no_cache)
    fp32_rule = packed_prompt_on(model) and packed_prompt_qualifies(*rule)
    perf_rule = not fp32_rule and packed_prompt_perf_on(model) and packed_prompt_perf_qualifies(*rule)
    if fp32_rule or perf_rule:
        _write_prompts(codes, first_codes, n)
        # the fp32 rule: rows or grouped prefixes, an utterance's beams n code rows apart; the perf rule: independent rows
        into = state.prefix if fp32_rule and state.prefix is not None else state.cache
        last = packed_pass(model, texts, plan.txs, plan.pls, codes[:plan.G * n:n] if fp32_rule else codes[:plan.G], into, range(plan.G))
        state.prompt_rows = (True, sum(plan.ctx))
        if plan.kind == GROUPED:
            last = last.repeat_interleave(n, 0)       # every beam starts from its utterance's last hidden row
        if perf_rule and plan.kind == ROWS:
            state.cache = state.cache.narrowed(plan.s_max)    # fp32 prompt K/V -> the bf16 cache of the decode steps
        return last.contiguous(), {}, None
    if not plan.ragged:
        text_ids = torch.stack(texts[:rows])
        codes[:, 1:plan.pl_max] = torch.stack(first_codes).repeat_interleave(n, 0) if plan.kind == GROUPED else torch.stack(first_codes)
        x = torch.empty(rows, s0, d, device=dev, dtype=torch.float32)
        model._embed_rows(text_ids, codes[:rows * n:n, :plan.pl_max], x)
        fwd = dict(x_len=plan.txs[0])
    else:
        x = torch.zeros(plan.G, s0, d, device=dev, dtype=torch.float32)
        for b in range(plan.G):
            codes[b * n:(b + 1) * n, 1:plan.pls[b]] = first_codes[b]
            model._embed_rows(texts[b].unsqueeze(0), codes[b * n:b * n + 1, :plan.pls[b]], x[b:b + 1])
        fwd = dict(x_len_dev=torch.tensor(plan.txs, **i32), kv_len=torch.tensor(plan.ctx, **i32))
    into = state.cache if state.prefix is None else state.prefix
    if plan.prefill_bf16:
        # (shared prompt: the ONE row's pass on the 16-bit matrix cores writes straight into the 16-bit prefix cache)
        transformer_forward_bf16(model.transformer, x, into, mode=kernels.MASK_PREFIX,
                                 scratch=ForwardScratch16(rows * s0, d, cfg.dim_feedforward, dev), **fwd)
    elif plan.kind == SHARED and plan.perf_mode:
        # perf_mode='kv' over a shared prompt: the fp32 pass of the one row, its K/V narrowed once into the 16-bit prefix
        wide = KVCache(cfg.num_layers, 1, cfg.n_heads, state.prefix.s_max, dev)
        transformer_forward(model.transformer, x, wide, mode=kernels.MASK_PREFIX,
                            scratch=ForwardScratch(s0, d, cfg.dim_feedforward, dev), **fwd)
        wide.narrow_into(state.prefix)
    else:
        scratch = None if plan.kind in (RECOMPUTE_GENERAL, ROWS_HD) else ForwardScratch(rows * s0, d, cfg.dim_feedforward, dev)
        transformer_forward(model.transformer, x, into, mode=kernels.MASK_PREFIX, scratch=scratch, **fwd)
    if plan.ragged:
        last = x[torch.arange(plan.G, device=dev), fwd['kv_len'].long() - 1]
    elif plan.kind == SHARED:
        last = x[:, -1].expand(B, d)                  # every beam starts from the one prompt row's last hidden state
    else:
        last = x[:, -1]
    if plan.kind == GROUPED:
        last = last.repeat_interleave(n, 0)           # every beam starts from its utterance's last hidden row
    if plan.kind == ROWS and plan.perf_mode:
        state.cache = state.cache.narrowed(plan.s_max)    # fp32 prompt K/V -> the bf16 cache of the decode steps
    return last.contiguous(), fwd, text_ids


def _decode_forced(model, plan, dec, forced, keep_logits):
    """TEACHER FORCING (tolerance tests): after every step replace the sampled token and its embedding by the given one;
    returns the logits the head produced at the steps listed in keep_logits."""
    dev, d = model.device, model.config.d_model
    forced = forced.to(dev)
    if plan.ragged or forced.numel() < plan.max_new:
        raise ValueError('forced: one token per step, equal-length rows')
    pe, kept = model.audio_position_emb.pe, {}
    for t in range(plan.max_new):
        if t:
            dec.run(1)
        if t in keep_logits:
            kept[t] = dec.logits[:, : dec.V].clone()
        dec.codes[:, plan.pl_max + t] = forced[t]
        kernels.embed_sum_pe(dec.codes[:, plan.pl_max + t:plan.pl_max + t + 1], [model.audio_emb.weight.detach()], pe,
                             plan.pl_max + t, dec.x.view(plan.B, 1, d))
    return kept


def _decode_recompute(model, plan, dec, texts, cache, fwd, text_ids):
    """config.use_kv_cache = False (valle_ar.py:132,150-155 — the reference's branch raises, D2; build-defined here as
    what the flag says): every step embeds the WHOLE sequence again and runs the full stack over it under the prefix
    mask — no state is carried from step to step except the tokens — and samples from its last row with the same head /
    sample kernels.  O(S^2) per token; it exists so that the flag works and as an independent check of the cached
    decoder (same tokens, tests/test_models_gpu.py).  Returns the number of steps run."""
    cfg, dev, d = model.config, model.device, model.config.d_model
    B, s0, codes = plan.B, plan.s0, dec.codes
    scratch = None if plan.kind == RECOMPUTE_GENERAL else ForwardScratch(B * (s0 + plan.max_new), d, cfg.dim_feedforward, dev)
    rows_idx = torch.arange(B, device=dev)
    done = 1
    while done < plan.max_new:
        t = done
        xs = (torch.zeros if plan.ragged else torch.empty)(B, s0 + t, d, device=dev, dtype=torch.float32)
        if scratch is not None:
            scratch.fit(B * (s0 + t))
        if not plan.ragged:
            model._embed_rows(text_ids, codes[:, :plan.pl_max + t], xs)
            transformer_forward(model.transformer, xs, cache, mode=kernels.MASK_PREFIX, scratch=scratch, **fwd)
            last = xs[:, -1]
        else:
            for b in range(B):
                model._embed_rows(texts[b].unsqueeze(0), codes[b:b + 1, :plan.pls[b] + t], xs[b:b + 1])
            transformer_forward(model.transformer, xs, cache, mode=kernels.MASK_PREFIX, scratch=scratch,
                                x_len_dev=fwd['x_len_dev'], kv_len=fwd['kv_len'] + t)
            last = xs[rows_idx, fwd['kv_len'].long() + t - 1]
        dec.sample_from(last.contiguous())
        done += 1
        if done % EOS_POLL == 0 and bool((dec.eos_count[:done] == B).any()):
            break
    return done


def _decode_cached(plan, dec, done):
    """Steps done .. max_new-1 on the cached decoder, EOS polled every EOS_POLL steps (valle_ar.py:169-170 breaks when
    every beam has emitted EOS).  Returns (steps run, step at which every row had finished or None)."""
    while done < plan.max_new:
        n = min(EOS_POLL, plan.max_new - done)
        dec.run(n)
        done += n
        full = (dec.eos_count[:done] == plan.B).nonzero()
        if full.numel():
            return done, int(full[0])
    return done, None


def _generate_in_groups(model, texts, first_codes, max_new, use_graph, perf_mode, beams=1, sampling=None):
    """More rows than one decode launch serves (64: 4 MFMA row tiles): consecutive groups of 64 rows; rows are
    independent, so the result is what one pass would give.  beams > 1: consecutive chunks of whole utterances, 64 // beams
    of them per launch."""
    B, dev = len(texts) * beams, model.device
    parts, stats = [], []
    per = MAX_DECODE_ROWS // beams
    for r0 in range(0, len(texts), per):
        parts.append(model.generate_batch(texts[r0:r0 + per], first_codes[r0:r0 + per],
                                          max_new=max_new, use_graph=use_graph, perf_mode=perf_mode, beams=beams,
                                          sampling=None if sampling is None else sampling[r0:r0 + per]))
        stats.append(model.last_generate_stats)
    width = max(p.shape[1] for p in parts)
    out = torch.full((B, width), model.eos_token, device=dev, dtype=torch.int64)
    r = 0
    for p in parts:
        out[r:r + p.shape[0], :p.shape[1]] = p
        r += p.shape[0]
    merged = dict(stats[-1])
    merged['prompt_lens'] = [x for st in stats for x in st['prompt_lens']]
    merged['sum_logprobs'] = torch.cat([st['sum_logprobs'] for st in stats])
    merged['tokens_appended'] = max(st['tokens_appended'] for st in stats)
    merged['groups'] = sum(st['groups'] for st in stats)
    merged['repetition_aware'] = any(st['repetition_aware'] for st in stats)
    merged['bounded'] = any(st['bounded'] for st in stats)
    merged['packed_prompt'] = any(st['packed_prompt'] for st in stats)
    merged['prompt_rows'] = sum(st['prompt_rows'] for st in stats)
    merged['padded_prompt_rows'] = sum(st['padded_prompt_rows'] for st in stats)
    model.last_generate_stats = merged
    return out


def generate_batch(model, texts, first_codes, max_new, use_graph, profile_attn, perf_mode, forced, keep_logits, shared_prompt,
                   beams, sampling=None):
    """ValleAR.generate_batch on the device (its docstring says what the arguments mean)."""
    model._require_layernorm()
    cfg, dev = model.config, model.device
    G = len(texts)
    if G == 0 or len(first_codes) != G:
        raise ValueError('generate_batch: texts and first_codes must be non-empty lists of equal length')
    check_beams(cfg, beams, shared_prompt, perf_mode, forced)
    sampling = check_sampling(sampling, G, forced, cfg, max_new)
    by_hand = forced is not None or bool(profile_attn)
    check_forms(cfg, perf_mode, by_hand, shared_prompt)
    max_new = cfg.max_audio_len if max_new is None else max_new
    if beams > 1 and G * beams > MAX_DECODE_ROWS:
        return _generate_in_groups(model, texts, first_codes, max_new, use_graph, perf_mode, beams=beams, sampling=sampling)
    if G > MAX_DECODE_ROWS:
        if shared_prompt or forced is not None:
            raise ValueError(f'shared_prompt / forced serve at most {MAX_DECODE_ROWS} rows')
        return _generate_in_groups(model, texts, first_codes, max_new, use_graph, perf_mode, sampling=sampling)
    plan = plan_decode(cfg, [int(t.shape[0]) for t in texts], [int(c.shape[0]) + 1 for c in first_codes],   # BOS + prompt
                       max_new=max_new, beams=beams, shared_prompt=bool(shared_prompt), perf_mode=perf_mode, use_graph=use_graph,
                       by_hand=by_hand, pos_limits=(model.audio_position_emb.pe.shape[0], model.tokens_position_emb.pe.shape[0]),
                       row_sampling=sampling is not None, row_limits=_sampling.bounded(sampling))
    if not plan.fits:
        # beyond the 256 records one merge serves: the same rows, each with its own prompt pass and K/V
        out = model.generate_batch([t for t in texts for _ in range(beams)], [c for c in first_codes for _ in range(beams)],
                                   max_new=max_new, use_graph=use_graph, profile_attn=profile_attn,
                                   # (the replicated records: beam j of an utterance keeps key j)
                                   sampling=None if sampling is None else [r for s in sampling for r in _sampling.beam_rows(s, beams)])
        model.last_generate_stats.update(groups=G, beams=beams, grouped_shared=False)
        return out
    B = plan.B
    t_host0 = time.perf_counter()
    # a decoder per shape survives the call (graphs, caches, counters: DecodeState) unless the call is one of the
    # measurement / test forms that drive the decoder by hand
    key = slot_key(plan, cfg, dev, weights_key(model))
    state = acquire_state(model, key)
    ok = False
    try:
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]   # prefill | decode phase times
        marks[0].record()
        texts = [kernels.ids_to_device(t, dev, cfg.vocab_size, 'text ids') for t in texts]
        first_codes = [kernels.ids_to_device(c, dev, cfg.num_audio_tokens, 'prompt codes') for c in first_codes]
        if plan.kind == SHARED and (any(t is not texts[0] and not torch.equal(t, texts[0]) for t in texts[1:])
                                    or any(c is not first_codes[0] and not torch.equal(c, first_codes[0]) for c in first_codes[1:])):
            raise ValueError('shared_prompt: every row must carry the same text and prompt ids')
        seed = state.arm(model, plan, sampling)
        t_host1 = time.perf_counter()
        last, fwd, text_ids = prompt_pass(model, plan, state, texts, first_codes, forced=forced is not None)
        t_host2 = time.perf_counter()
        dec = state.decoder(model, plan, seed)
        dec.capture()                                 # (a no-op without a graph: the no-cache path only borrows the sampler)
        t_host3 = time.perf_counter()
        dec.sample_from(last)
        marks[1].record()
        del last
        kept, done, stop = {}, 1, None
        attn_ms = attn_floor_ms = attn_kernel_ms = None
        if forced is not None:
            kept, done = _decode_forced(model, plan, dec, forced, keep_logits), max_new
        elif plan.no_cache:
            done = _decode_recompute(model, plan, dec, texts, state.cache, fwd, text_ids)
        elif profile_attn and max_new > 1:
            attn_ms, attn_floor_ms, attn_kernel_ms = dec.profile_attn(max_new - 1)
            done = max_new
        else:
            done, stop = _decode_cached(plan, dec, done)
        marks[2].record()
        if stop is None:
            full = (dec.eos_count[:done] == B).nonzero()
            stop = int(full[0]) if full.numel() else None
        n_new = max_new if stop is None else stop     # the all-EOS step is not appended (:169-171)
        marks[2].synchronize()
        t_host4 = time.perf_counter()
        _lib.raise_device_errors(dev)                 # ids that were already on the device: checked in-kernel
        stats = model.last_generate_stats = {
            'steps_run': done, 'tokens_appended': n_new, 'n_split': dec.n_split,
            'ffn_fused': dec.ffn_ws is not None and ffn_fused_width(cfg.d_model), 'kv_bf16': dec.kv_bf16,
            'decode_w16': bool(getattr(dec, 'w16', False)), 'ln_folded': bool(getattr(dec, 'ln_folded', False)),
            'head_fused': dec.head_ws is not None, 'prefill_bf16': plan.prefill_bf16, 'shared_prompt': plan.kind == SHARED,
            'logits': kept, 'prefill_ms': marks[0].elapsed_time(marks[1]), 'decode_ms': marks[1].elapsed_time(marks[2]),
            'attn_mean_ms': attn_ms, 'attn_floor_ms': attn_floor_ms, 'attn_kernel_ms': attn_kernel_ms, 's0': plan.s0,
            'prompt_lens': plan.row_pls, 'groups': G, 'beams': beams, 'grouped_shared': plan.kind == GROUPED,
            'sum_logprobs': dec.sum_logprobs.clone(), 'sampling': 'rows' if plan.row_sampling else 'call',
            'repetition_aware': _sampling.repetition_aware(sampling), 'bounded': _sampling.bounded(sampling),
            # host time this call spent OUTSIDE enqueueing the prompt pass and the replays and waiting for them: set-up of
            # the call's state + building / capturing the decoder (nothing on a reused slot) + the tail after the last step
            # has finished
            'decoder_reused': state.reused, 'slot_uses': state.uses if state.busy else 0,
            'host_setup_ms': (t_host1 - t_host0) * 1e3, 'host_decoder_ms': (t_host3 - t_host2) * 1e3,
            'kv_cache': not plan.no_cache,
            # the prompt pass: over packed rows or padded ones, the rows it computed and the rows the padded pass computes
            'packed_prompt': state.prompt_rows[0], 'prompt_rows': state.prompt_rows[1],
            'padded_prompt_rows': (1 if plan.kind == SHARED else G) * plan.s0}
        out_codes = state.codes[:, : plan.pl_max + n_new].clone()
        stats['host_tail_ms'] = (time.perf_counter() - t_host4) * 1e3
        stats['host_outside_ms'] = stats['host_setup_ms'] + stats['host_decoder_ms'] + stats['host_tail_ms']
        ok = True
        return out_codes
    finally:
        release_state(model, key, state, ok)


def generate_queued(model, utterances, beams, slots, use_graph=True):
    """ValleAR.generate_queued on the device, behind its refusals."""
    model._require_layernorm()
    check_queued(model.config, beams, slots)
    cfg, dev, d = model.config, model.device, model.config.d_model
    texts, firsts = unpack_utterances(utterances)
    sampling = _sampling.of_utterances('generate_queued', utterances, cfg)
    n = len(texts)
    if n == 0:
        raise ValueError('generate_queued: utterances must be a non-empty list')
    slots = min(n, MAX_DECODE_ROWS // beams if slots is None else slots)
    max_new, poll = cfg.max_audio_len, EOS_POLL
    txs = [int(t.shape[0]) for t in texts]
    pls = [int(c.shape[0]) + 1 for c in firsts]                        # BOS + prompt
    ctx = [t + p for t, p in zip(txs, pls)]
    # the rows the call starts with; the capacity of the longest prompt of the CALL: any refill fits.  Every row may run
    # whole polls up to the one that covers max_new before the host rewinds or re-arms it
    plan = plan_decode(cfg, txs[:slots], pls[:slots], max_new=queue_steps_cap(max_new, poll), beams=beams, use_graph=use_graph,
                       queued=True, cap=group_prefix_cap(max(ctx)), row_sampling=sampling is not None,
                       row_limits=_sampling.bounded(sampling))     # (of the whole list: a refill may bring the first bound)
    if not plan.fits:
        out = model.generate_many(utterances, beams=beams)
        model.last_generate_stats.update(queued=False)
        return out
    cap, s_suf, width = plan.cap, plan.rows_spec[1], plan.codes_width
    if max(pls) + plan.max_new + 1 > model.audio_position_emb.pe.shape[0] or max(txs) > model.tokens_position_emb.pe.shape[0]:
        raise _lib.VhError('sequence exceeds the positional table (max_len 5000)')
    key = slot_key(plan, cfg, dev, weights_key(model))
    state = acquire_state(model, key)
    ok = False
    try:
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        marks[0].record()
        texts = [kernels.ids_to_device(t, dev, cfg.vocab_size, 'text ids') for t in texts]
        firsts = [kernels.ids_to_device(c, dev, cfg.num_audio_tokens, 'prompt codes').contiguous() for c in firsts]
        seed = state.arm(model, plan, sampling and sampling[:slots])
        # the records of the utterances that wait: a refill copies its own over the group's, device to device
        waiting = waiting_limits = None
        if sampling is not None and n > slots:
            waiting = _lib.to_device_async(kernels.pack_row_sampling([r for s in sampling[slots:] for r in s.records(cfg, beams)]), dev)
            if plan.row_limits:
                waiting_limits = _lib.to_device_async(kernels.pack_row_limits(_sampling.row_limits(sampling[slots:], beams)), dev)
        last, _, _ = prompt_pass(model, plan, state, texts[:slots], firsts[:slots])
        dec = state.decoder(model, plan, seed)
        codes, cache_len, audio_pos, pos_base, group_len = state.codes, state.cache_len, state.audio_pos, state.pos_base, state.group_len
        poll_dev, poll_host, prefix = state.poll_dev, state.poll_host, state.prefix
        dec.capture()
        dec.sample_from(last)
        del last
        marks[1].record()
        sampled = cfg.top_k != 1 or plan.row_sampling
        sched = QueueSchedule(n, slots)
        saved, at_cap = {}, {}
        scratch = None
        polls = steps = parked_steps = 0
        max_cl = max_ap = kernels.POLL_NONE
        live_cl, live_ap = 0, plan.pl_max + 1                              # the fresh rows the first sample leaves
        gap_s, t_gap = 0.0, None
        p = 0
        # the packed switch: a poll's refills wait until all its groups are re-armed and, two or more, run as one packed pass
        pack_refills = packed_prompt_on(model)
        refills, packed_refills = [], 0

        def refill_pass(g, nxt):
            """The one-row prompt pass of utterance nxt into group g's region of the prefix cache; its last hidden row (1, d)."""
            nonlocal scratch
            x = torch.empty(1, ctx[nxt], d, device=dev, dtype=torch.float32)
            model._embed_rows(texts[nxt].unsqueeze(0), codes[g * beams:g * beams + 1, :pls[nxt]], x)
            if scratch is None:
                scratch = ForwardScratch(max(ctx), d, cfg.dim_feedforward, dev)
            transformer_forward(model.transformer, x, prefix.group_view(g), mode=kernels.MASK_PREFIX,
                                scratch=scratch.fit(ctx[nxt]), x_len=txs[nxt])
            return x[:, -1]

        def first_sample(g, nxt, last):
            """Group g's rows take utterance nxt's records and draw its first token from its last prompt row (1, d)."""
            nonlocal live_cl, live_ap
            rows = slice(g * beams, (g + 1) * beams)
            if waiting is not None:
                # the group's rows take the new utterance's seed, keys 0 .. beams - 1 and filter: a stream-ordered write
                # between replays (the captured steps hold the pointer), before the first sample reads them; its length
                # bounds travel with them
                state.row_sampling[rows].copy_(waiting[(nxt - slots) * beams:(nxt - slots + 1) * beams])
                if waiting_limits is not None:
                    state.row_limits[rows].copy_(waiting_limits[(nxt - slots) * beams:(nxt - slots + 1) * beams])
            # (first_len stands in for cache_len: the first sample appends no K/V row, and vh_decode_group_reset left
            # cache_len where the first step appends)
            dec.sample_from(last.expand(beams, d).contiguous(), rows, state.first_len)
            live_cl, live_ap = max(live_cl, 0), max(live_ap, pls[nxt] + 1)

        while not sched.finished:
            # the rows that step on stand at most here; every other row was re-armed or rewound to a fresh row below
            if live_cl + poll > s_suf or live_ap + poll > width:
                raise _lib.VhError(f'generate_queued: a row at cache_len {live_cl} / audio_pos {live_ap} cannot run {poll} more '
                                   f'steps within a suffix cache of {s_suf} rows and codes of {width} (a scheduling bug: '
                                   'nothing was replayed)')
            held = [g for g in range(slots) if sched.holder[g] is not None]
            # sampled rows that reach max_new inside this block: their scores are taken AT max_new (the steps between it
            # and the poll would add log-probabilities of tokens that are cut)
            capping = [g for g in held if 1 + (p - sched.start[sched.holder[g]] + 1) * poll > max_new] if sampled else []
            to_cap = max_new - 1 - (p - sched.start[sched.holder[capping[0]]]) * poll if capping else 0
            if t_gap is not None:
                gap_s += time.perf_counter() - t_gap
            if 0 < to_cap < poll:
                dec.run(to_cap)
                for g in capping:
                    at_cap[sched.holder[g]] = dec.sum_logprobs[g * beams:(g + 1) * beams].clone()
                dec.run(poll - to_cap)
            else:
                dec.run(poll)
            steps += poll
            parked_steps += (slots - len(held)) * poll
            p += 1
            kernels.decode_groups_poll(codes, cache_len, audio_pos, pos_base, model.eos_token, beams, max_new, poll_dev)
            poll_host.copy_(poll_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            t_gap = time.perf_counter()
            polls += 1
            got = poll_host.tolist()
            max_cl, max_ap = max(max_cl, got[0]), max(max_ap, got[1])
            live_cl, live_ap = got[2], got[3]
            for g in range(slots):
                u = sched.holder[g]
                rows = slice(g * beams, (g + 1) * beams)
                if u is None:                                          # parked: rewound, so that it never leaves its rows
                    kernels.decode_group_reset(codes, g, beams, None, 0, model.bos_token, model.eos_token, cache_len, audio_pos,
                                               pos_base, dec.sum_logprobs, group_len)
                    continue
                if not got[4 + g]:
                    continue
                saved[u] = (codes[rows, :pls[u] + min(got[4 + slots + g], max_new)].clone(),
                            at_cap.pop(u) if u in at_cap else dec.sum_logprobs[rows].clone())
                nxt = sched.retire(g, p)
                if nxt is None:
                    kernels.decode_group_reset(codes, g, beams, None, 0, model.bos_token, model.eos_token, cache_len, audio_pos,
                                               pos_base, dec.sum_logprobs, group_len)
                    continue
                # refill: re-arm the rows, one-row prompt pass into the group's region of the prefix cache, first sample
                kernels.decode_group_reset(codes, g, beams, firsts[nxt], ctx[nxt], model.bos_token, model.eos_token, cache_len,
                                           audio_pos, pos_base, dec.sum_logprobs, group_len)
                if pack_refills:
                    refills.append((g, nxt))              # (their passes run together once every group of the poll is re-armed)
                else:
                    first_sample(g, nxt, refill_pass(g, nxt))
            if len(refills) >= 2:
                # the refills of this poll as ONE packed pass: the groups' prompt rows back to back, their K/V unpacked into
                # the groups' regions of the prefix cache
                gs = [g for g, _ in refills]
                head_rows = _lib.to_device_async(torch.tensor([g * beams for g in gs], dtype=torch.int64), dev)
                lasts = packed_pass(model, [texts[u] for _, u in refills], [txs[u] for _, u in refills], [pls[u] for _, u in refills],
                                    codes.index_select(0, head_rows)[:, :max(pls[u] for _, u in refills)], prefix, gs)
                packed_refills += len(refills)
                for i, (g, nxt) in enumerate(refills):
                    first_sample(g, nxt, lasts[i:i + 1])
            elif refills:
                first_sample(*refills[0], refill_pass(*refills[0]))
            refills.clear()
        done_mark = torch.cuda.Event(enable_timing=True)
        done_mark.record()
        done_mark.synchronize()
        _lib.raise_device_errors(dev)
        model.last_generate_stats = {
            'queued': True, 'slots': slots, 'beams': beams, 'groups': n, 'refills': sched.refills, 'polls': polls,
            # the starting prompt pass (packed or padded, and the rows it computed) and the refills that ran in packed passes
            'packed_prompt': state.prompt_rows[0], 'prompt_rows': state.prompt_rows[1], 'padded_prompt_rows': slots * plan.s0,
            'packed_refills': packed_refills,
            'steps': steps, 'parked_group_steps': parked_steps, 'max_cache_len': max_cl, 'max_audio_pos': max_ap,
            's_suf': s_suf, 'codes_width': width, 'prefix_cap': cap, 'intervals': sched.intervals(),
            'sum_logprobs': torch.cat([saved[u][1] for u in range(n)]), 'prompt_lens': [pl for pl in pls for _ in range(beams)],
            'rows': [saved[u][0] for u in range(n)], 'grouped_shared': True,
            'decoder_reused': state.reused, 'slot_uses': state.uses if state.busy else 0,
            'n_split': dec.n_split, 'prefill_ms': marks[0].elapsed_time(marks[1]),
            'decode_ms': marks[1].elapsed_time(done_mark), 'poll_gap_ms': gap_s * 1e3, 'kv_cache': True,
            'sampling': 'rows' if plan.row_sampling else 'call', 'repetition_aware': _sampling.repetition_aware(sampling),
            'bounded': _sampling.bounded(sampling)}
        ok = True
        return [best_beam_tokens(model, *saved[u], pls[u]) for u in range(n)]
    finally:
        release_state(model, key, state, ok)
