"""ValleAR with the reference's constructor / training_step / generate / configure_optimizers
signatures and state_dict keys (valle/models/valle_ar.py:14-194), running on MI355X.

`generate()` does not walk the module tree per step as the reference does: the prompt is embedded
and prefilled once by the native forward composite (analytic prefix-LM mask, K/V written straight
into a preallocated cache) and every further token is one replay of a hipGraph holding the whole
decode step (engine.ArDecoder).  EOS is polled every `EOS_POLL` steps instead of a host sync per
step (valle_ar.py:169-170).  This file holds the model and the public entry points; what lies between
them and the decoder (the plan of a call, its state, the prompt pass, the decode loops) is generation.py.
"""
from __future__ import annotations

import functools
import inspect

import torch
import torch.nn as nn
from torch import optim

from . import _lib, dropout, generation, kernels
from . import sampling as _sampling
from .engine import KVCache, shared_prompt_fits, transformer_forward, transformer_forward_bf16
from .generation import DECODER_SLOTS, EOS_POLL, MAX_DECODE_ROWS, SHARED_PROMPT  # noqa: F401  (tools import them from here)
from .modules import PositionalEncoding, TokenEmbedding, Transformer, _on_device


try:  # the reference subclasses lightning.LightningModule; lightning is optional here
    import lightning as L
    _Base = L.LightningModule
except Exception:  # pragma: no cover - lightning is absent in this image
    class _Base(nn.Module):
        def log(self, *args, **kwargs):
            return None


def _beams_refused_early(fn):
    """generate_batch(beams=n > 1): the refusals that need only the arguments and the config come before anything touches
    a device (the wrappers below move the call to the HIP device first)."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if kwargs.get('beams', 1) != 1 or kwargs.get('sampling') is not None:
            a = sig.bind(self, *args, **kwargs).arguments
            generation.check_beams(self.config, a.get('beams', 1), a.get('shared_prompt', False), a.get('perf_mode', False), a.get('forced'))
            generation.check_sampling(a.get('sampling'), len(a['texts']), a.get('forced'), self.config, a.get('max_new'))
        return fn(self, *args, **kwargs)
    return wrapper


def _sampling_refused_early(fn):
    """generate(sampling=...) and the utterance lists of generate_many: what is wrong with the Sampling entries is said
    before anything touches a device."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        a = sig.bind(self, *args, **kwargs).arguments
        if 'utterances' in a:
            _sampling.of_utterances(fn.__name__, a['utterances'], self.config)
        elif a.get('sampling') is not None:
            if not isinstance(a['sampling'], (_sampling.Sampling, _sampling.Bounded)):
                raise ValueError(f'{fn.__name__}: sampling is {type(a["sampling"]).__name__}, not a valle2_amd.Sampling')
            a['sampling'].resolved(self.config)
            if isinstance(a['sampling'], _sampling.Bounded):
                a['sampling'].check_cap(fn.__name__, int(self.config.max_audio_len))
        return fn(self, *args, **kwargs)
    return wrapper


class ValleAR(_Base):
    # The prompt pass of ragged generate calls over PACKED rows (generation.packed_pass: no padding row is computed; one embed
    # launch, one packed prefix-LM forward, one vh_kv_unpack into the decoder's caches).  None: on when VALLE2_PACKED_PROMPT=1
    # is in the environment of the call, else off; True / False (on the class or on a model) override.  The only switch — the
    # signatures of generate, generate_many, generate_queued, generate_batch and codec_io.* do not change — and it reaches all
    # of them.  It takes effect where the call qualifies (generation.packed_prompt_qualifies: utterances of different lengths,
    # fp32, head width 64, cached decoding, no `forced`, not shared_prompt); every other call runs the padded pass as ever.
    # (A model that lives on the CPU computes through a cached device copy: set the switch on the class, or before the first
    # call.)
    packed_prompt = None
    # The same for PERF MODE, a switch of its own (`packed_prompt` leaves perf-mode calls on the padded pass): None: on when
    # VALLE2_PACKED_PROMPT_PERF=1 is in the environment of the call, else off; True / False override.  It takes effect where the
    # call qualifies (generation.packed_prompt_perf_qualifies: utterances of different lengths, perf_mode True or 'kv', head
    # width 64, independent cached rows, no `forced`): perf_mode=True runs the 16-bit packed pass into the 16-bit row cache,
    # 'kv' (or a shape the 16-bit stack does not take) the fp32 packed pass, narrowed once; every other call runs the padded pass.
    packed_prompt_perf = None

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.tokens_emb = TokenEmbedding(config.vocab_size, config.d_model)
        self.audio_emb = TokenEmbedding(config.num_audio_tokens + 2, config.d_model)
        self.tokens_position_emb = PositionalEncoding(config.d_model)
        self.audio_position_emb = PositionalEncoding(config.d_model)
        self.transformer = Transformer(config)
        self.proj = nn.Linear(config.d_model, config.num_audio_tokens + 1, bias=False)
        self.last_generate_stats: dict = {}

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def eos_token(self):
        return self.config.num_audio_tokens

    @property
    def bos_token(self):
        return self.config.num_audio_tokens + 1

    # ------------------------------------------------------------------------------------
    def _require_layernorm(self):
        if self.config.norm != 'LayerNorm':
            # reference defect D3: with AdaptiveLayerNorm the AR model passes embedding=None and
            # dies in Linear(None) with a TypeError; keep the failure, say why.
            raise TypeError("ValleAR needs norm='LayerNorm' (AdaptiveLayerNorm has no stage "
                            'embedding in the AR model; the reference raises TypeError too)')

    def _embed_rows(self, text_ids, codes_ids, x, x_t0=0):
        """x[:, x_t0:x_t0+Tx] = tokens_emb + PE; x[:, x_t0+Tx:] = audio_emb + PE (positions restart
        at 0 for the audio stream, valle_ar.py:61-66)."""
        tx = text_ids.shape[1]
        kernels.embed_sum_pe(text_ids, [self.tokens_emb.weight.detach()], self.tokens_position_emb.pe,
                             0, x, out_t0=x_t0)
        kernels.embed_sum_pe(codes_ids, [self.audio_emb.weight.detach()], self.audio_position_emb.pe,
                             0, x, out_t0=x_t0 + tx)

    @_on_device
    def forward_logits(self, batch, perf_mode: bool = False):
        """Teacher-forced logits (B, Ty, V_a+1) of valle_ar.py:54-83 (row-major, before the
        reference's rearrange to (B, V, Ty)).  A model that lives on the CPU computes through its
        device mirror (modules.device_mirror); the logits stay on the HIP device.
        perf_mode=True (opt-in, SECONDARY): the stack on the bf16 matrix cores (engine.transformer_forward_bf16); logits
        agree with the reference to 5e-2 instead of 2e-4."""
        self._require_layernorm()
        dev = self.device
        tokens = kernels.ids_to_device(batch['tokens'], dev, self.config.vocab_size, 'tokens')
        codes = kernels.ids_to_device(batch['codes'], dev, self.config.num_audio_tokens + 2, 'codes')
        codes_lens = batch['codes_lens']
        tx, ty = int(max(batch['tokens_lens'])), int(max(codes_lens))
        b = tokens.shape[0]
        d = self.config.d_model
        x = torch.empty(b, tx + ty, d, device=dev, dtype=torch.float32)
        self._embed_rows(tokens[:, :tx], codes[:, :ty], x)
        # key padding covers audio only; text padding is NOT masked (valle_ar.py:69-73)
        kv_len = _lib.to_device_async(codes_lens.to(torch.int64) + tx, dev, torch.int32)
        if perf_mode:
            cache = KVCache(self.config.num_layers, b, self.config.n_heads, tx + ty, dev, dtype=kernels.H16)
            transformer_forward_bf16(self.transformer, x, cache, mode=kernels.MASK_PREFIX, x_len=tx, kv_len=kv_len)
        else:
            cache = KVCache(self.config.num_layers, b, self.config.n_heads, tx + ty, dev)
            transformer_forward(self.transformer, x, cache, mode=kernels.MASK_PREFIX, x_len=tx, kv_len=kv_len)
        out = x[:, tx:].reshape(b * ty, d)
        logits = kernels.linear(out, self.proj.weight.detach())
        return logits.reshape(b, ty, -1)

    def _logits_with_graph(self, batch):
        """The same forward as `forward_logits`, composed from autograd Functions so that
        `loss.backward()` reaches every parameter (valle_ar.py:61-83)."""
        from . import autograd as A
        self._require_layernorm()
        dev = self.device
        if dev.type != 'cuda':
            raise _lib.VhError('ValleAR.training_step with gradients needs the model on its HIP device '
                               '(model.to("cuda")): gradients cannot flow into a CPU copy of the parameters')
        tokens = kernels.ids_to_device(batch['tokens'], dev, self.config.vocab_size, 'tokens')
        codes = kernels.ids_to_device(batch['codes'], dev, self.config.num_audio_tokens + 2, 'codes')
        codes_lens = batch['codes_lens']
        tx, ty = int(max(batch['tokens_lens'])), int(max(codes_lens))
        b, d = tokens.shape[0], self.config.d_model
        # PE dropout p = 0.1 is live in train mode whatever config.dropout says (D9).  Both streams' embeddings are written
        # into ONE buffer (no torch.cat, no strided copies of its gradient) and each part's dropout is a field applied by
        # the gather kernel itself before it stores the row (dropout.py) — the backward regenerates it in the scatter
        seed = dropout.seed_if(dropout.live(self.tokens_position_emb.dropout), dropout.live(self.audio_position_emb.dropout))
        dr_t = dropout.spec(seed, dropout.site(dropout.PE_TEXT), dropout.live(self.tokens_position_emb.dropout))
        dr_a = dropout.spec(seed, dropout.site(dropout.PE_AUDIO), dropout.live(self.audio_position_emb.dropout))
        dropout.record('tokens_position_emb.dropout', dr_t, b * (tx + ty), d)
        dropout.record('audio_position_emb.dropout', dr_a, b * (tx + ty), d)
        x = A.EmbedConcatFn.apply([(tokens[:, :tx], self.tokens_position_emb.pe, 0, [0], dr_t),
                                   (codes[:, :ty], self.audio_position_emb.pe, 0, [1], dr_a)],
                                  self.tokens_emb.weight, self.audio_emb.weight)
        x = x.reshape(b * (tx + ty), d)
        kv_len = _lib.to_device_async(codes_lens.to(torch.int64) + tx, dev, torch.int32)
        spec = dict(mode=kernels.MASK_PREFIX, x_len=tx, kv_len=kv_len)
        x = A.transformer_train(self.transformer, x, b, tx + ty, spec)
        out = x.view(b, tx + ty, d)[:, tx:].reshape(b * ty, d)
        return A.linear(out, self.proj.weight).reshape(b, ty, -1)

    def training_step(self, batch, **kwargs):
        """valle_ar.py:43-90: mean cross entropy over ALL (B, Ty) positions, pads included.  With
        grad mode on the loss carries a full autograd graph (hand-written HIP kernels forward and
        backward: tile GEMMs, TN weight-gradient GEMM, flash attention backward, row kernels —
        valle2_amd/autograd.py); under no_grad it takes the fused inference kernels."""
        from . import autograd as A
        if torch.is_grad_enabled():
            logits = self._logits_with_graph(batch)
        else:
            logits = self.forward_logits(batch)
        target = kernels.ids_to_device(batch['target'], logits.device, self.config.num_audio_tokens + 1, 'target')
        rows = logits.shape[0] * logits.shape[1]
        loss = A.CrossEntropyFn.apply(logits.reshape(rows, -1), target[:, : logits.shape[1]].reshape(rows))
        self.log('train/loss', loss)
        return loss

    def training_step_packed(self, batch, **kwargs):
        """`training_step` of a ragged batch WITHOUT its padding (extension, opt-in; `training_step` is untouched).  The same
        collated batch; utterance b contributes the rows [tokens[b, :tokens_lens[b]] | codes[b, :codes_lens[b]]], the
        utterances lie back to back in one (M, d) buffer, positions restart at 0 for each stream of each utterance, and every
        utterance attends its own rows only under its own prefix-LM mask (`vh_attn_rows_packed_lse` /
        `vh_attn_rows_bwd_packed`; every other kernel is the row-wise one over M rows).  The loss is the mean cross entropy
        over the sum(codes_lens) REAL target positions: the reference's training_step on each utterance alone (B = 1, nothing
        padded), the per-utterance losses combined token-weighted.  It differs from `training_step` on a ragged batch —
        that one averages over padded positions and lets every row see text padding (valle_ar.py:69-73,86) — and equals it
        when all lengths are equal.  Dropout as in training_step, the fields keyed on the packed row.  Head width 64,
        LayerNorm; under no_grad the same value without a graph."""
        self._require_layernorm()
        cfg = self.config
        if cfg.d_model != kernels.HEAD_DIM * cfg.n_heads:
            raise ValueError(f'training_step_packed: head width {cfg.d_model // cfg.n_heads} (d_model={cfg.d_model}, '
                             f'n_heads={cfg.n_heads}): the packed attention serves width {kernels.HEAD_DIM} only — '
                             'training_step serves the others')
        txs, tys = [int(n) for n in batch['tokens_lens']], [int(n) for n in batch['codes_lens']]
        n = batch['tokens'].shape[0]
        if len(txs) != n or len(tys) != n or batch['codes'].shape[0] != n or batch['target'].shape[0] != n:
            raise ValueError(f'training_step_packed: {n} rows of tokens, {len(txs)} tokens_lens, {len(tys)} codes_lens')
        for what, lens, width in (('tokens_lens', txs, batch['tokens'].shape[1]),
                                  ('codes_lens', tys, min(batch['codes'].shape[1], batch['target'].shape[1]))):
            bad = [v for v in lens if not 1 <= v <= width]
            if bad:
                raise ValueError(f'training_step_packed: {what} entry {bad[0]} is outside 1 .. {width} (the batch\'s padded width)')
        if not torch.is_grad_enabled():
            with torch.no_grad():
                loss = self._packed_loss_on_device(batch)
        elif self.device.type != 'cuda':
            raise _lib.VhError('ValleAR.training_step_packed with gradients needs the model on its HIP device '
                               '(model.to("cuda")): gradients cannot flow into a CPU copy of the parameters')
        else:
            loss = self._packed_loss(batch)
        self.log('train/loss', loss)
        return loss

    @_on_device
    def _packed_loss_on_device(self, batch):
        return self._packed_loss(batch)

    def _packed_loss(self, batch):
        from . import autograd as A
        from .engine import PackedRows
        dev, cfg = self.device, self.config
        d = cfg.d_model
        tokens = kernels.ids_to_device(batch['tokens'], dev, cfg.vocab_size, 'tokens')
        codes = kernels.ids_to_device(batch['codes'], dev, cfg.num_audio_tokens + 2, 'codes')
        target = kernels.ids_to_device(batch['target'], dev, cfg.num_audio_tokens + 1, 'target')
        txs, tys = torch.as_tensor(batch['tokens_lens']).cpu().long(), torch.as_tensor(batch['codes_lens']).cpu().long()
        tx, ty = int(txs.max()), int(tys.max())
        rows = PackedRows((txs + tys).tolist(), dev, x_lens=txs.tolist())
        M = rows.rows
        starts = torch.tensor(rows.starts, dtype=torch.int64)
        put = lambda t, dt=None: _lib.to_device_async(t, dev, dt)   # noqa: E731

        def ragged(lens, base, width):
            """(packed row, b * width + t) of every (b, t < lens[b]), row-major."""
            b = torch.repeat_interleave(torch.arange(len(lens)), lens)
            t = torch.arange(int(lens.sum())) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
            return base[b] + t, b * width + t

        dest_t, src_t = ragged(txs, starts, tx)
        dest_a, src_a = ragged(tys, starts + txs, ty)
        _, src_target = ragged(tys, starts, target.shape[1])
        dest_a_dev = put(dest_a)
        # PE dropout as in training_step (live in train mode whatever config.dropout says, D9): the fields of both streams
        # are keyed on the row of the packed buffer
        seed = dropout.seed_if(dropout.live(self.tokens_position_emb.dropout), dropout.live(self.audio_position_emb.dropout))
        dr_t = dropout.spec(seed, dropout.site(dropout.PE_TEXT), dropout.live(self.tokens_position_emb.dropout))
        dr_a = dropout.spec(seed, dropout.site(dropout.PE_AUDIO), dropout.live(self.audio_position_emb.dropout))
        dropout.record('tokens_position_emb.dropout', dr_t, M, d)
        dropout.record('audio_position_emb.dropout', dr_a, M, d)
        x = A.EmbedPackedFn.apply(
            [(tokens[:, :tx], self.tokens_position_emb.pe, put(txs, torch.int32), rows.seg_start, tx, 0, dr_t, put(dest_t), put(src_t)),
             (codes[:, :ty], self.audio_position_emb.pe, put(tys, torch.int32), put(starts + txs, torch.int32), ty, 1, dr_a,
              dest_a_dev, put(src_a))],
            M, self.tokens_emb.weight, self.audio_emb.weight)
        x = A.transformer_train(self.transformer, x, 1, M, dict(mode=kernels.MASK_PREFIX, rows=rows))
        logits = A.linear(x.index_select(0, dest_a_dev), self.proj.weight)
        return A.CrossEntropyFn.apply(logits, target.reshape(-1).index_select(0, put(src_target)))

    # ------------------------------------------------------------------------------------
    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate(self, prompt_tokens, prompt_codes, target_tokens=None, *, perf_mode=False, sampling=None):
        """valle_ar.py:92-180 — one utterance replicated over `num_beams` rows; returns the 1-D
        int64 first-codebook tokens of the best beam with EOS stripped.

        perf_mode (keyword-only, default off; True or 'kv' as in `generate_batch`): the decode steps stream a 16-bit K/V
        cache — with the shared prompt below, the prompt's K/V are read once per step AND at half the bytes.  Off, this runs
        exactly what it always ran.

        sampling (keyword-only, a valle2_amd.Sampling): the request's own seed and filter — beam j draws from (seed, j, audio
        position), whatever torch's generator holds, and the same draws come out of generate_batch(beams=n), generate_many
        and generate_queued for an utterance that carries the same Sampling.  None: the config's filter and a seed from
        torch's generator, as always.

        The beams share one prompt, so (SHARED_PROMPT, default on) the prompt pass runs for ONE row and its K/V are read
        once per decode step for all beams (`generate_batch(..., shared_prompt=True)`); the beams themselves — their
        sampled tokens, their own K/V rows, the per-beam log-probabilities — are never deduplicated."""
        (text,), (first,) = generation.unpack_utterances([(prompt_tokens, prompt_codes, target_tokens)])
        beams = self.config.num_beams
        shared = SHARED_PROMPT and self.config.use_kv_cache and self.config.d_model == self.config.n_heads * kernels.HEAD_DIM
        # (a prompt beyond the shared kernel's record bound — 7680 keys at 4 beams x 8 heads — decodes as independent rows)
        shared = shared and shared_prompt_fits(beams, self.config.n_heads, int(text.shape[0]) + int(prompt_codes.shape[0]) + 1)   # + BOS
        rows = self.generate_batch([text] * beams, [first] * beams, shared_prompt=shared and beams <= MAX_DECODE_ROWS,
                                   perf_mode=perf_mode,
                                   sampling=None if sampling is None else _sampling.beam_rows(sampling, beams))
        return generation.best_beam_tokens(self, rows, self.last_generate_stats['sum_logprobs'], prompt_codes.shape[0] + 1)

    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate_many(self, utterances, *, beams=None):
        """`generate()` for several utterances in one decode: utterances = [(prompt_tokens, prompt_codes, target_tokens |
        None), ...], each replicated over `beams` rows (default config.num_beams) that share its prompt's K/V
        (`generate_batch(..., beams=n)`).  Returns a list of 1-D int64 tensors, per utterance what generate() returns: the
        best beam by get_best_beam over that utterance's rows and scores, prompt cut, EOS stripped.  An utterance may carry
        its Sampling as a fourth element (every utterance of the call, or none): its draws and filter are then its own, the
        same at any place in the list."""
        beams = self.config.num_beams if beams is None else int(beams)
        texts, firsts = generation.unpack_utterances(utterances)
        rows = self.generate_batch(texts, firsts, beams=beams, sampling=_sampling.of_utterances('generate_many', utterances))
        stats = self.last_generate_stats
        return [generation.best_beam_tokens(self, rows[g * beams:(g + 1) * beams],
                                            stats['sum_logprobs'][g * beams:(g + 1) * beams].to(rows.device), stats['prompt_lens'][g * beams])
                for g in range(len(texts))]

    def generate_queued(self, utterances, *, beams=None, slots=None):
        """`generate_many` with the rows kept busy: `slots` utterances (default min(len(utterances), 64 // beams); 1 <= slots *
        beams <= 64) decode at once, and whenever the host polls (every EOS_POLL steps) an utterance whose beams have all
        emitted EOS — or that has run max_audio_len steps — is saved and its rows handed to the next waiting utterance: a
        one-row prompt pass into that group's region of the prefix cache, the head and the first sample on its rows, the rows'
        counters re-armed (vh_decode_group_reset).  With nothing waiting the group is PARKED (prefix length 0: the decode
        attention reads nothing for it) and rewound at every poll.  One decoder, one set of captured graphs, replayed between
        polls and never re-captured.  Same arguments and result as generate_many; what it serves is the grouped form: fp32,
        head width 64, use_kv_cache=True, d_model <= 4096, greedy and sampled.  A longest prompt whose capacity is beyond the
        256 records of the grouped merge falls back to generate_many (`last_generate_stats['queued']` is False).

        Greedy tokens do not depend on the schedule.  Neither do the SAMPLED tokens of utterances that carry a Sampling as
        their fourth element (every utterance of the call, or none): their draws are keyed on (the utterance's seed, the beam
        within it, the audio position) and their filter is their own — a refill rewrites its group's records before its
        first sample — so an utterance decodes the same in any slot, started or refilled, and as generate_many and
        generate() decode it.  WITHOUT a Sampling the sampler keys its draws on (the call's seed, the row index it is given,
        position): the decode steps hand it the decoder's rows and a refill's first sample the group's rows 0 .. beams - 1, so
        an utterance's draws then depend on the slot it lands in and on whether it started the call or refilled a slot (the
        same list, slots and seed give the same output).

        `last_generate_stats`: sampling ('rows' with Sampling, else 'call'), queued, slots, refills, polls, steps (decode steps replayed), parked_group_steps, max_cache_len
        / max_audio_pos (largest values any row reached) beside s_suf / codes_width (what they must stay within), intervals
        ((slot, start poll, end poll) per utterance), sum_logprobs and prompt_lens per row in utterance order, rows (per
        utterance in input order, the saved (beams, length) int64 tokens its best beam was chosen from: BOS + prompt + what was
        generated, cut at max_audio_len; a call that fell back to generate_many records none), packed_prompt / prompt_rows /
        padded_prompt_rows (the starting prompt pass, as generate_batch reports them) and packed_refills (the refills that ran in
        packed passes: with `packed_prompt` on, a poll that retires two or more groups refills them in one)."""
        beams = self.config.num_beams if beams is None else beams
        generation.check_queued(self.config, beams, slots)
        _sampling.of_utterances('generate_queued', utterances, self.config)
        return self._generate_queued(utterances, beams, slots)

    @_on_device
    @torch.inference_mode()
    def _generate_queued(self, utterances, beams, slots, use_graph=True):
        """generate_queued behind its refusals (use_graph=False steps eagerly: the tests' second arm)."""
        return generation.generate_queued(self, utterances, beams, slots, use_graph)

    def release_decoders(self):
        """Free the decoders (graphs, K/V caches, workspaces) kept from earlier generate() calls."""
        generation.release_decoders(self)

    @_beams_refused_early
    @_on_device
    @torch.inference_mode()
    def generate_batch(self, texts, first_codes, max_new=None, use_graph=True, profile_attn=False, perf_mode=False,
                       forced=None, keep_logits=(), shared_prompt=False, *, beams=1, sampling=None):
        """Batched greedy decoding of B independent rows (extension; `generate` is built on it).
        texts[b]: 1-D int64 text ids; first_codes[b]: 1-D int64 first-codebook prompt (no BOS).
        Rows may differ in text and prompt length.  Returns codes (B, max_prompt_len + n_new) int64
        on the device: row b holds BOS + prompt_b + its n_new generated tokens from index 0 (finished
        rows and the tail of shorter rows are EOS-filled; `last_generate_stats['prompt_lens'][b]` is
        where row b's generated tokens start).
        profile_attn=True runs the steps eagerly with HIP events around every decode-attention
        launch and leaves their mean duration in `last_generate_stats` (measurement only).
        perf_mode=True (opt-in): the prompt pass runs on the bf16 matrix cores (bf16 operands, fp32
        accumulators and residual stream; engine.transformer_forward_bf16) and writes its K/V straight into the bf16 cache
        the decode steps stream; the decode steps' weights and arithmetic stay fp32.  perf_mode='kv': only the cache is bf16
        (the fp32 prompt pass, its K/V narrowed once — round 3's form).  Greedy tokens are then NOT guaranteed to be the
        reference's (teacher-forced logits agree to 5e-2).  Any row count 1..64: below 256 (row, head) pairs the 16-bit cache
        is read with key splits (`last_generate_stats['n_split']`).
        forced (max_new,) int64 + keep_logits (step indices): TEACHER FORCING for the tolerance tests — step t appends
        forced[t] whatever the head says (steps run eagerly, one at a time) and the logits (B, V) the head produced at
        the steps listed in keep_logits are left in `last_generate_stats['logits']`.
        shared_prompt=True: the caller vouches that every row has the SAME text and prompt (the beams of one utterance,
        valle_ar.py:135-138; checked: equal lengths and equal ids) — the prompt pass then runs for one row and every decode
        step reads the prompt's K/V once for all rows (vh_attn_decode_shared); rows still sample, append and score
        independently.  Cached decoder only; combines with perf_mode (True and 'kv'): the one-row prompt pass then fills a
        16-bit prefix cache (on the 16-bit matrix cores, or fp32 and narrowed once for 'kv') and the beams' own rows are 16-bit
        too (vh_attn_decode_shared_kv16).  Rows of different lengths are refused.
        beams=n > 1 (keyword-only): texts / first_codes hold G UTTERANCES (texts and prompts of any lengths) and the call
        decodes G * n rows, row g * n + j being beam j of utterance g — `generate()`'s replication for several utterances at
        once.  The prompt pass runs for the G rows and every decode step reads each utterance's prompt K/V once for its n
        beams (vh_attn_decode_shared_groups); the result and `last_generate_stats` are laid out as for G * n independent rows
        (`prompt_lens`, `sum_logprobs` per row) plus `groups`, `beams` and `grouped_shared` (False when a prompt beyond the
        kernel's record bound sent the call down the independent-rows path).  More than 64 rows decode in consecutive chunks
        of whole utterances.  fp32 cached decoder at head width 64 only: shared_prompt, perf_mode and forced are refused.
        sampling (keyword-only): a list with one valle2_amd.Sampling per entry of texts (every entry or None).  Row g * beams +
        j then draws from (sampling[g].seed, j, audio position) through sampling[g]'s own top_k / tok_p / temperature (None:
        the config's) — on every kind of decode, graph or eager — and no seed is drawn from torch's generator;
        `last_generate_stats['sampling']` is 'rows' ('call' without).  Refused with forced.
        The prompt pass (`packed_prompt`, above the constructor): `last_generate_stats['packed_prompt']` says whether it ran over
        packed rows, `prompt_rows` how many rows it computed (the sum of the contexts when packed) and `padded_prompt_rows` how
        many the padded pass computes (pass rows x the longest context; one row under shared_prompt)."""
        return generation.generate_batch(self, texts, first_codes, max_new, use_graph, profile_attn, perf_mode, forced, keep_logits,
                                         shared_prompt, beams, sampling)

    def configure_optimizers(self):
        """valle_ar.py:182-194"""
        from .optim import FlatAdamW           # AdamW(fused=True) as one flat HIP pass (+ clip, + 1/world)
        optimizer = FlatAdamW(self.parameters(), lr=self.config.lr, betas=self.config.betas,
                              weight_decay=self.config.weight_decay)
        scheduler = optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, self.config.lr_warmup)
        return {'optimizer': optimizer, 'lr_scheduler': scheduler}
