"""ValleNAR with the reference's constructor / method signatures and state_dict keys
(valle/models/valle_nar.py:17-188), running on MI355X.

`_prepare_audio_codes` follows the reference exactly.  `training_step` and `generate` RAISE in the
reference (defects D4/D5); they implement the intended algorithm of SURVEY.md §3.4
here: stage n predicts codebook n from the sum of codebooks < n (all Q for the acoustic prompt),
AdaLN conditioned on stage_embs[n-1], full attention, head proj_layers[n-1].
"""
from __future__ import annotations

import functools
import inspect
import random

import torch
import torch.nn as nn

from . import _lib, dropout, kernels
from . import sampling as _sampling
from .engine import KVCache, NarLayout, head16, perf_forward_supported, transformer_forward, transformer_forward_bf16
from .modules import PositionalEncoding, TokenEmbedding, Transformer, _on_device
from .valle_ar import _Base


def _sampling_refused_early(fn):
    """generate(sampling=...) / generate_batch(sampling=[...]): what is wrong with the Sampling entries is said before
    anything touches a device (the wrappers below move the call to the HIP device first)."""
    sig = inspect.signature(fn)
    name = fn.__name__

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if kwargs.get('sampling') is not None:
            a = sig.bind(self, *args, **kwargs).arguments
            given = a['sampling']
            if 'texts' not in a:                                       # generate: one Sampling
                given = [given]
            elif not isinstance(given, (list, tuple)):
                raise ValueError(f'{name}: sampling is {type(given).__name__}, not a list with one valle2_amd.Sampling per utterance')
            for i, s in enumerate(given):
                if s is not None and not isinstance(s, (_sampling.Sampling, _sampling.Bounded)):   # (a Bounded's bounds are the AR stage's)
                    raise ValueError(f'{name}: sampling{f" of utterance {i}" if "texts" in a else ""} is {type(s).__name__}, '
                                     'not a valle2_amd.Sampling')
            if a.get('seed') is not None:
                raise ValueError(f'{name}: sampling together with seed= (every Sampling carries its own seed)')
            for s in _sampling.check_list(name, given, len(a['texts']) if 'texts' in a else 1) or ():
                s.nar_record(self.config)                              # the config's temperature, where the request has none
        return fn(self, *args, **kwargs)
    return wrapper


def _packed_width_refused_early(fn):
    """generate_packed: a head width the packed attention is not built for is said before anything touches a device."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        cfg = self.config
        if cfg.d_model != cfg.n_heads * kernels.HEAD_DIM:
            raise ValueError(f'{fn.__name__}: head width {cfg.d_model // cfg.n_heads} (d_model={cfg.d_model} / n_heads={cfg.n_heads}): '
                             'the packed attention serves width 64 only — generate_batch serves the others')
        return fn(self, *args, **kwargs)
    return wrapper


def _packed_perf_shape_refused_early(fn):
    """generate_packed_perf: a shape the 16-bit tile kernels are not built for is said before anything touches a device."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        cfg = self.config
        if not perf_forward_supported(cfg):
            raise ValueError(f'{fn.__name__}: d_model={cfg.d_model}, dim_feedforward={cfg.dim_feedforward}: perf mode serves '
                             'multiples of 128 only — generate_packed serves the others in fp32')
        return fn(self, *args, **kwargs)
    return wrapper


class ValleNAR(_Base):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.eos_token = config.num_audio_tokens
        self.bos_token = config.num_audio_tokens + 1
        self.tokens_emb = TokenEmbedding(config.vocab_size, config.d_model)
        self.codes_embs = nn.ModuleList(
            [TokenEmbedding(config.num_audio_tokens, config.d_model) for _ in range(config.num_quantizers)])
        self.tokens_position_emb = PositionalEncoding(config.d_model)
        self.audio_position_emb = PositionalEncoding(config.d_model)
        self.stage_embs = nn.ModuleList(
            [TokenEmbedding(1, config.d_model) for _ in range(config.num_quantizers - 1)])
        self.transformer = Transformer(config)
        self.proj_layers = nn.ModuleList(
            [nn.Linear(config.d_model, config.num_audio_tokens, bias=False)
             for _ in range(config.num_quantizers - 1)])

    @property
    def device(self):
        return next(self.parameters()).device

    def _dev(self):
        dev = self.device
        if dev.type != 'cuda':     # inference entry points never get here (they run on the device mirror)
            raise _lib.VhError('ValleNAR.training_step with gradients needs the model on its HIP device '
                               '(model.to("cuda")): gradients cannot flow into a CPU copy of the parameters')
        return dev

    def _tables(self, n):
        return [self.codes_embs[j].weight.detach() for j in range(n)]

    def prefix_len_of(self, codes_len: int) -> int:
        """3 s of audio or a third of it, whichever is shorter (valle_nar.py:179)."""
        return min(codes_len // 3, 3 * self.config.quantization_factor)

    def _embed_audio(self, codes, nar_stage, out, out_t0, pe):
        """out[:, out_t0 + t] = sum_j codes_embs[j](codes[:, t, j]) (+ pe[t]); all Q codebooks for
        t < prefix, codebooks < nar_stage after (valle_nar.py:180-185).  One gather kernel each."""
        _, t, q = codes.shape
        p = self.prefix_len_of(t)
        if p:
            kernels.embed_sum_pe(codes[:, :p], self._tables(q), pe, 0, out, out_t0=out_t0)
        if t > p:
            kernels.embed_sum_pe(codes[:, p:], self._tables(max(1, min(nar_stage, q))), pe, p, out,
                                 out_t0=out_t0 + p)
        return p

    @_on_device
    def _prepare_audio_codes(self, codes: torch.Tensor, nar_stage: int):
        """valle_nar.py:167-188 → ((B, T, d) embedding sum without position, prefix_len)."""
        dev = self._dev()
        codes = kernels.ids_to_device(codes, dev, self.config.num_audio_tokens, 'codes')
        b, t, _ = codes.shape
        y = torch.empty(b, t, self.config.d_model, device=dev, dtype=torch.float32)
        p = self._embed_audio(codes, nar_stage, y, 0, None)
        return y, p

    @_on_device
    def stage_logits(self, batch, stage: int, perf_mode: bool = False):
        """Intended forward of valle_nar.py:71-100 for `stage` in 1..Q-1: logits (B, T-prefix, V_a)
        of codebook `stage` for the non-prefix frames.  Full attention; key padding is dropped
        exactly as the reference's Transformer does when attn_mask is None (defect D6).
        perf_mode=True (opt-in, SECONDARY — SURVEY section 7): the stack's products run on the bf16 matrix cores
        (engine.transformer_forward_bf16); logits agree with the reference to 5e-2, not to the parity path's 2e-4."""
        dev = self._dev()
        cfg = self.config
        tokens = kernels.ids_to_device(batch['tokens'], dev, cfg.vocab_size, 'tokens')
        codes = kernels.ids_to_device(batch['codes'], dev, cfg.num_audio_tokens, 'codes (EOS/BOS have no codebook row)')
        tx = int(batch['tokens_lens'].max())
        b, t, _ = codes.shape
        d = cfg.d_model
        x = torch.empty(b, tx + t, d, device=dev, dtype=torch.float32)
        kernels.embed_sum_pe(tokens[:, :tx], [self.tokens_emb.weight.detach()],
                             self.tokens_position_emb.pe, 0, x)
        p = self._embed_audio(codes, stage, x, tx, self.audio_position_emb.pe)
        if perf_mode:
            cache = KVCache(cfg.num_layers, b, cfg.n_heads, tx + t, dev, dtype=kernels.H16)
            transformer_forward_bf16(self.transformer, x, cache, mode=kernels.MASK_FULL,
                                     embedding=self.stage_embs[stage - 1].weight)
        else:
            cache = KVCache(cfg.num_layers, b, cfg.n_heads, tx + t, dev)
            transformer_forward(self.transformer, x, cache, mode=kernels.MASK_FULL,
                                embedding=self.stage_embs[stage - 1].weight)  # (the parameter itself: adaln_table keys on it)
        z = x[:, tx + p:].reshape(b * (t - p), d)
        logits = self._head(z, stage, perf_mode)
        return logits.reshape(b, t - p, -1), p

    def _head(self, z, stage: int, perf_mode):
        """The stage's projection (valle_nar.py:97-98) over the packed target frames z (rows, d); in perf mode on the 16-bit
        matrix cores like the stack's products (fp32 accumulate, fp32 logits) when the tile GEMM takes the shape."""
        w = self.proj_layers[stage - 1].weight
        w16 = head16(self, w) if perf_mode else None
        if w16 is None:
            return kernels.linear(z, w.detach())
        return kernels.linear_bf16(kernels.to_bf16(z), w16)

    def _stage_logits_with_graph(self, batch, stage: int):
        """`stage_logits` composed from autograd Functions (training path)."""
        from . import autograd as A
        dev = self._dev()
        cfg = self.config
        tokens = kernels.ids_to_device(batch['tokens'], dev, cfg.vocab_size, 'tokens')
        codes = kernels.ids_to_device(batch['codes'], dev, cfg.num_audio_tokens, 'codes (EOS/BOS have no codebook row)')
        tx = int(batch['tokens_lens'].max())
        b, t, q = codes.shape
        d = cfg.d_model
        p = self.prefix_len_of(t)
        tabs = [e.weight for e in self.codes_embs]
        n_stage = max(1, min(stage, q))
        # text | prefix frames (all codebooks) | target frames (codebooks < stage) written into ONE buffer; a codebook
        # table that two parts read receives one gradient (no torch.cat, no strided copies, no gradient adds); the PE
        # dropouts (p = 0.1 in train mode, D9) are fields applied by the gather kernel before it stores a row
        seed = dropout.seed_if(dropout.live(self.tokens_position_emb.dropout), dropout.live(self.audio_position_emb.dropout))
        dr_t = dropout.spec(seed, dropout.site(dropout.PE_TEXT), dropout.live(self.tokens_position_emb.dropout))
        dr_a = dropout.spec(seed, dropout.site(dropout.PE_AUDIO), dropout.live(self.audio_position_emb.dropout))
        dropout.record('tokens_position_emb.dropout', dr_t, b * (tx + t), d)
        dropout.record('audio_position_emb.dropout', dr_a, b * (tx + t), d)
        spec = [(tokens[:, :tx], self.tokens_position_emb.pe, 0, [0], dr_t)]
        if p:
            spec.append((codes[:, :p], self.audio_position_emb.pe, 0, list(range(1, 1 + q)), dr_a))
        if t > p:
            spec.append((codes[:, p:], self.audio_position_emb.pe, p, list(range(1, 1 + n_stage)), dr_a))
        x = A.EmbedConcatFn.apply(spec, self.tokens_emb.weight, *tabs).reshape(b * (tx + t), d)
        x = A.transformer_train(self.transformer, x, b, tx + t, dict(mode=kernels.MASK_FULL),
                                embedding=self.stage_embs[stage - 1].weight)
        z = x.view(b, tx + t, d)[:, tx + p:].reshape(b * (t - p), d)
        return A.linear(z, self.proj_layers[stage - 1].weight).reshape(b, t - p, -1), p

    def training_step(self, batch, **kwargs):
        """Intended loss: CE of the stage's logits against the raw ids codes[:, prefix:, stage]
        (the reference slices the embedded tensor, valle_nar.py:81, and raises); mean over all
        positions.  `stage=` pins the stage (the reference draws it with random.randint, :76)."""
        from . import autograd as A
        stage = kwargs.get('stage') or random.randint(1, self.config.num_quantizers - 1)
        if torch.is_grad_enabled():
            logits, p = self._stage_logits_with_graph(batch, stage)
        else:
            logits, p = self.stage_logits(batch, stage)
        target = kernels.ids_to_device(batch['codes'][:, p:, stage], logits.device, self.config.num_audio_tokens, 'codes')
        rows = logits.shape[0] * logits.shape[1]
        return A.CrossEntropyFn.apply(logits.reshape(rows, -1), target.reshape(rows))

    def training_step_packed(self, batch, **kwargs):
        """`training_step` of a ragged batch WITHOUT its padding (extension, opt-in; `training_step` is untouched).  The same
        collated batch; utterance b contributes the rows [tokens[b, :tokens_lens[b]] | codes[b, :codes_lens[b]]], the
        utterances lie back to back in one (M, d) buffer, positions restart at 0 for each stream of each utterance, and every
        utterance attends its own rows only, under the full mask (`vh_attn_rows_packed_lse` / `vh_attn_rows_bwd_packed`;
        AdaptiveLayerNorm's scale and shift are one vector per stage, so it and every other kernel is the row-wise one over M
        rows).  The acoustic prefix of utterance b is p_b = prefix_len_of(codes_lens[b]) — a third of ITS OWN frames, capped
        at 3 s — where `training_step` takes it from the padded width: frames below p_b carry all Q codebooks, the rest the
        codebooks below the stage (`vh_embed_nar_packed`, one launch; one backward launch), and the head runs over the
        sum(codes_lens[b] - p_b) target frames only.  The loss is the mean cross entropy over those frames against
        codes[b, p_b:codes_lens[b], stage]: the intended `training_step` on each utterance alone (B = 1, nothing padded), the
        per-utterance losses combined token-weighted.  It differs from `training_step` on a ragged batch — that one trains
        short utterances with the long ones' prefix length, attends padding keys (D6) and averages over padded frames — and
        equals it when all lengths are equal and nothing is padded.  `stage=` pins the stage, drawn as in `training_step`
        otherwise.  Dropout as in training_step, the fields keyed on the packed row.  Head width 64; under no_grad the same
        value without a graph."""
        cfg = self.config
        q = cfg.num_quantizers
        stage = kwargs.get('stage')
        if stage is None:
            stage = random.randint(1, q - 1)
        if cfg.d_model != kernels.HEAD_DIM * cfg.n_heads:
            raise ValueError(f'training_step_packed: head width {cfg.d_model // cfg.n_heads} (d_model={cfg.d_model}, '
                             f'n_heads={cfg.n_heads}): the packed attention serves width {kernels.HEAD_DIM} only — '
                             'training_step serves the others')
        if isinstance(stage, bool) or not isinstance(stage, int) or not 1 <= stage <= q - 1:
            raise ValueError(f'training_step_packed: stage={stage!r} is outside 1 .. {q - 1} (num_quantizers - 1)')
        tokens, codes = batch['tokens'], batch['codes']
        txs, tys = [int(v) for v in batch['tokens_lens']], [int(v) for v in batch['codes_lens']]
        n = tokens.shape[0]
        if len(txs) != n or len(tys) != n or codes.shape[0] != n:
            raise ValueError(f'training_step_packed: {n} rows of tokens, {codes.shape[0]} of codes, {len(txs)} tokens_lens, '
                             f'{len(tys)} codes_lens')
        if tokens.dim() != 2 or codes.dim() != 3 or codes.shape[2] != q:
            raise ValueError(f'training_step_packed: expected tokens (B, Tx) and codes (B, T, {q}), got {tuple(tokens.shape)} and '
                             f'{tuple(codes.shape)}')
        for what, lens, width in (('tokens_lens', txs, tokens.shape[1]), ('codes_lens', tys, codes.shape[1])):
            bad = [v for v in lens if not 1 <= v <= width]
            if bad:
                raise ValueError(f'training_step_packed: {what} entry {bad[0]} is outside 1 .. {width} (the batch\'s padded width)')
        if max(txs) > self.tokens_position_emb.pe.shape[0] or max(tys) > self.audio_position_emb.pe.shape[0]:
            raise ValueError(f'training_step_packed: a stream of {max(txs)} text ids / {max(tys)} frames exceeds the positional table')
        ids = {'tokens': tokens, 'codes': codes}
        if not torch.is_grad_enabled():
            with torch.no_grad():
                return self._packed_loss_on_device(ids, txs, tys, stage)
        if self.device.type != 'cuda':
            raise _lib.VhError('ValleNAR.training_step_packed with gradients needs the model on its HIP device '
                               '(model.to("cuda")): gradients cannot flow into a CPU copy of the parameters')
        return self._packed_loss(ids, txs, tys, stage)

    @_on_device
    def _packed_loss_on_device(self, ids, txs, tys, stage):
        return self._packed_loss(ids, txs, tys, stage)

    def _packed_loss(self, ids, txs, tys, stage):
        from . import autograd as A
        from .engine import NarTrainLayout
        dev, cfg = self.device, self.config
        d, q = cfg.d_model, cfg.num_quantizers
        tokens = kernels.ids_to_device(ids['tokens'], dev, cfg.vocab_size, 'tokens')
        codes = kernels.ids_to_device(ids['codes'], dev, cfg.num_audio_tokens, 'codes (EOS/BOS have no codebook row)')
        layout = NarTrainLayout(txs, tys, [self.prefix_len_of(t) for t in tys], codes.shape[1], dev)
        M = layout.rows
        # PE dropout as in training_step (live in train mode whatever config.dropout says, D9): the fields of both streams are
        # keyed on the row of the packed buffer
        seed = dropout.seed_if(dropout.live(self.tokens_position_emb.dropout), dropout.live(self.audio_position_emb.dropout))
        dr_t = dropout.spec(seed, dropout.site(dropout.PE_TEXT), dropout.live(self.tokens_position_emb.dropout))
        dr_a = dropout.spec(seed, dropout.site(dropout.PE_AUDIO), dropout.live(self.audio_position_emb.dropout))
        dropout.record('tokens_position_emb.dropout', dr_t, M, d)
        dropout.record('audio_position_emb.dropout', dr_a, M, d)
        x = A.EmbedNarPackedFn.apply(tokens, codes, layout, max(1, min(stage, q)), self.tokens_position_emb.pe,
                                     self.audio_position_emb.pe, dr_t, dr_a, self.tokens_emb.weight,
                                     *[e.weight for e in self.codes_embs])
        x = A.transformer_train(self.transformer, x, 1, M, dict(mode=kernels.MASK_FULL, rows=layout.packed),
                                embedding=self.stage_embs[stage - 1].weight)
        logits = A.linear(x.index_select(0, layout.target_rows), self.proj_layers[stage - 1].weight)
        target = codes[:, :, stage].reshape(-1).index_select(0, layout.target_index)
        return A.CrossEntropyFn.apply(logits, target)

    def configure_optimizers(self):
        """The reference's ValleNAR has no configure_optimizers; same recipe as AR."""
        from torch import optim
        from .optim import FlatAdamW
        optimizer = FlatAdamW(self.parameters(), lr=self.config.lr, betas=self.config.betas,
                              weight_decay=self.config.weight_decay)
        scheduler = optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, self.config.lr_warmup)
        return {'optimizer': optimizer, 'lr_scheduler': scheduler}

    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate(self, prompt_tokens, prompt_codes, target_tokens, target_codes_first_layer,
                 greedy: bool = False, *, sampling=None):
        """valle_nar.py:107-165 (intended algorithm) → codes (Ty, Q) int64.  The reference samples
        from Categorical(logits / temperature) (:160); greedy=True takes the arg-max instead,
        which is what the parity tests pin.  One utterance of `generate_batch`.
        sampling (keyword-only, a valle2_amd.Sampling): the request's own seed and temperature, see `generate_batch`."""
        text = torch.cat([prompt_tokens, target_tokens], dim=0)
        return self.generate_batch([text], [prompt_codes], [target_codes_first_layer], greedy=greedy,
                                   sampling=None if sampling is None else [sampling])[0]

    def _ragged_inputs(self, name, dev, texts, prompt_codes, first_layers):
        """The input checks of `generate_batch` / `generate_packed`: the three id lists on the device, and their lengths
        (txs, tcs, tys)."""
        cfg = self.config
        B = len(texts)
        if B == 0 or len(prompt_codes) != B or len(first_layers) != B:
            raise ValueError(f'{name}: texts, prompt_codes and first_layers must be non-empty lists of equal length')
        texts = [kernels.ids_to_device(t, dev, cfg.vocab_size, 'text ids') for t in texts]
        pcs = [kernels.ids_to_device(c, dev, cfg.num_audio_tokens, 'prompt codes') for c in prompt_codes]
        firsts = [kernels.ids_to_device(f, dev, cfg.num_audio_tokens, 'first-layer codes') for f in first_layers]
        for t, c, f in zip(texts, pcs, firsts):
            if t.dim() != 1 or c.dim() != 2 or c.shape[1] != cfg.num_quantizers or f.dim() != 1:
                raise ValueError(f'{name}: expected text (Tx,), prompt codes (Tc, Q), first layer (Ty,)')
        txs, tcs, tys = [t.shape[0] for t in texts], [c.shape[0] for c in pcs], [f.shape[0] for f in firsts]
        if max(tc + ty for tc, ty in zip(tcs, tys)) > self.audio_position_emb.pe.shape[0] or \
                max(txs) > self.tokens_position_emb.pe.shape[0]:
            raise _lib.VhError('sequence exceeds the positional table (max_len 5000)')
        return (texts, pcs, firsts), (txs, tcs, tys)

    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate_batch(self, texts, prompt_codes, first_layers, greedy: bool = False, seed=None, perf_mode: bool = False, *,
                       sampling=None):
        """Batched NAR decoding of B independent utterances (extension; `generate` is built on it).
        texts[b]: 1-D int64 text ids (prompt + target text); prompt_codes[b]: (Tc_b, Q) int64 acoustic
        prompt; first_layers[b]: (Ty_b,) int64 first-codebook codes of the target (the AR model's
        output).  Rows may differ in every length.  Returns a list of (Ty_b, Q) int64 device tensors.

        Utterance b's rows [text_b | prompt_b | target_b] lie in one (rows, d) buffer, here PADDED to the longest
        (`engine.nar_rows`); attention is full over the utterance's own length (per-row key length in the kernel, nothing
        materialised).  Per stage n = 1..Q-1 (valle_nar.py:142-160): the target frames carry sum_{j<n} codes_embs[j](out[j]) +
        PE, one stack forward with AdaLN on stage_embs[n-1], head proj_layers[n-1] on the target frames of all utterances at
        once, and codebook n is drawn on the device by `vh_categorical_rows` (Categorical(logits / temperature), or the
        arg-max when greedy).
        perf_mode=True: the seven stack forwards on the bf16 matrix cores (see `stage_logits`); the drawn codes are then not
        guaranteed to be the parity path's.
        sampling (keyword-only): a list with one valle2_amd.Sampling per utterance (every entry or None).  Frame t of codebook
        n of utterance b is then drawn from uniform01(sampling[b].seed, t, NAR_STREAM | n) at sampling[b]'s temperature (None:
        the config's), or is the arg-max where sampling[b].top_k == 1 (its other top_k values and tok_p are not read: this
        stage has no filter) — by `vh_categorical_rows_keyed`, straight into the codes tensor.  Nothing is drawn from torch's
        generator and nothing of the draw depends on the other utterances, their order or their lengths; a token can differ
        between two calls only where the utterance's own logits do.  greedy=True makes every request greedy; refused with
        seed= (ValueError)."""
        dev = self._dev()
        ids, lens = self._ragged_inputs('generate_batch', dev, texts, prompt_codes, first_layers)
        return self._generate_stages('generate_batch', NarLayout(*lens, False, dev), ids, lens, greedy, seed, sampling, perf_mode)

    @_packed_width_refused_early
    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate_packed(self, texts, prompt_codes, first_layers, greedy: bool = False, seed=None, *, sampling=None):
        """`generate_batch` computed over PACKED rows: same inputs, checks, return value and sampling semantics (see there),
        fp32 only (no perf_mode), head width 64 only (ValueError otherwise, before any device work).

        The utterances lie back to back, no padding row (`engine.nar_rows`, packed).  LayerNorm, the GEMMs and the K/V append
        run over the M = sum(len_b) rows as one sequence; the attention runs each utterance over its own rows
        (`vh_attn_rows_packed`), so a ragged batch computes sum(len_b) rows and sum(len_b^2) scores where generate_batch
        computes B max(len) and max(len) sum(len_b).  The GEMMs see another row count than the padded form's, so logits agree
        with it to summation order, not to the bit; a greedy token can differ where the two leading logits are closer than
        that."""
        dev = self._dev()
        ids, lens = self._ragged_inputs('generate_packed', dev, texts, prompt_codes, first_layers)
        return self._generate_stages('generate_packed', NarLayout(*lens, True, dev), ids, lens, greedy, seed, sampling)

    @_packed_width_refused_early
    @_packed_perf_shape_refused_early
    @_sampling_refused_early
    @_on_device
    @torch.inference_mode()
    def generate_packed_perf(self, texts, prompt_codes, first_layers, greedy: bool = False, seed=None, *, sampling=None):
        """`generate_packed` in PERF MODE: the same inputs, checks, return value and sampling keys, the packed rows of
        `generate_packed` and the arithmetic of `generate_batch(perf_mode=True)` — the stack forwards on the 16-bit matrix
        cores over the M = sum(len_b) rows, each utterance attending its own rows of a one-row 16-bit K/V cache
        (`vh_attn_rows_packed_bf16`), and the stage heads on 16-bit weights.  Head width 64 only, and d_model and
        dim_feedforward multiples of 128 (ValueError otherwise, before any device work).  As with perf_mode=True the drawn
        codes are not guaranteed to be the parity path's; against the padded perf-mode form the attention of an utterance is
        the same bits and the GEMMs see another row count, so logits agree with it to 16-bit rounding, not to the bit."""
        dev = self._dev()
        ids, lens = self._ragged_inputs('generate_packed_perf', dev, texts, prompt_codes, first_layers)
        return self._generate_stages('generate_packed_perf', NarLayout(*lens, True, dev), ids, lens, greedy, seed, sampling, True)

    def _generate_stages(self, name, layout, ids, lens, greedy, seed, sampling, perf_mode=False):
        """The stage loop of `generate_batch`, `generate_packed` and `generate_packed_perf` over `layout` (an engine.NarLayout of
        `lens`): they differ only in where a row lies and which forward runs over the buffer (padded or packed, fp32 or
        `perf_mode`), and the layout knows both.  The gathered target rows, hence the logits rows and the draws' keys, are utterance by utterance and frame by frame
        under either layout."""
        cfg = self.config
        q, d = cfg.num_quantizers, cfg.d_model
        (texts, pcs, firsts), (txs, tcs, tys) = ids, lens
        B, dev = len(texts), layout.device
        pe_a, pe_t = self.audio_position_emb.pe, self.tokens_position_emb.pe
        ty_max = max(tys)
        pad = torch.nn.utils.rnn.pad_sequence                      # index plumbing: ragged id lists -> padded id tensors
        i32 = lambda v: _lib.to_device_async(torch.tensor(v, dtype=torch.int32), dev)   # noqa: E731
        out = torch.zeros(B, ty_max, q, device=dev, dtype=torch.int64)
        out[:, :, 0] = pad(firsts, batch_first=True)
        tx_d, tc_d, ty_d = i32(txs), i32(tcs), i32(tys)
        valid = torch.arange(ty_max, device=dev)[None, :] < ty_d[:, None]          # (B, ty_max) target frames that exist
        # text and acoustic-prompt embeddings do not change from stage to stage: build them once, ONE launch each for
        # the whole ragged batch (per-utterance lengths and first rows travel to the kernel)
        base = (torch.zeros if layout.zeroed else torch.empty)(layout.rows, d, device=dev, dtype=torch.float32)
        kernels.embed_sum_pe(pad(texts, batch_first=True), [self.tokens_emb.weight.detach()], pe_t, 0, base, lens=tx_d,
                             row_t0=layout.t0_text, max_pos=max(txs))
        if max(tcs):
            kernels.embed_sum_pe(pad(pcs, batch_first=True), self._tables(q), pe_a, 0, base, lens=tc_d, row_t0=layout.t0_prompt,
                                 max_pos=max(tcs))
        cache, scratch = layout.cache_and_scratch(cfg, perf_mode)
        x = torch.empty_like(base)
        sampling = _sampling.check_list(name, sampling, B)
        if sampling is not None:
            # one record per utterance and the (utterance, frame) of every logits row, once per call
            records = [s.nar_record(cfg) for s in sampling]
            if greedy:
                records = [(sd, key, 1, top_p, temperature) for sd, key, _, top_p, temperature in records]
            requests = _lib.to_device_async(kernels.pack_row_sampling(records), dev)
            row_request = i32([b for b in range(B) for _ in range(tys[b])])
            row_key = i32([t for b in range(B) for t in range(tys[b])])
        else:
            if seed is None:       # drawn from torch's generator, so torch.manual_seed() makes a run repeatable
                seed = 0 if greedy else int(torch.randint(0, 2 ** 62, (1,)).item())
            toks = torch.empty(layout.plan.logit_starts[-1], device=dev, dtype=torch.int64)
        for n in range(1, q):
            x.copy_(base)
            kernels.embed_sum_pe(out, self._tables(n), pe_a, 0, x, lens=ty_d, row_pos0=tc_d, row_t0=layout.t0_target,
                                 max_pos=max(tc + ty for tc, ty in zip(tcs, tys)))
            layout.forward(self.transformer, x, cache, scratch, self.stage_embs[n - 1].weight)   # (cached AdaLN table per stage)
            z = x.index_select(0, layout.target_rows)                           # target frames of every utterance
            logits = self._head(z, n, perf_mode)
            if sampling is not None:
                kernels.categorical_rows_keyed(logits, out[:, :, n], requests, row_request, row_key, _sampling.NAR_STREAM | n)
                continue
            kernels.categorical_rows(logits, toks, temperature=cfg.temperature, greedy=greedy, seed=seed,
                                     stream_id=n)
            out[:, :, n][valid] = toks                                          # logits rows -> (B, ty_max)
        _lib.raise_device_errors(dev)
        return [out[b, :tys[b]].clone() for b in range(B)]
