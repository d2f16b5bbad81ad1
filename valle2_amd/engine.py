"""Device-side runtime of the path: KV cache, scratch buffers, the native forward composite and the
hipGraph-replayed AR decoder.  Python here only wires pointers; all arithmetic runs in
libvalle_hip.so (`_lib.lib()` raises without a HIP device — there is no CPU fallback).

Data layout in HBM (all fp32):
  residual stream x        (B*T, d) row-major, updated in place by the GEMM epilogues
  KV cache per layer       K (B, h, S_max, hd), V (B, h, S_max, hd), hd = d_model / n_heads: one (b,head) stream is
                           contiguous, so decode attention reads it as pure 16-B-per-lane bursts
                           and a new token's K/V row is appended in place (no torch.cat regrow,
                           valle/models/modules.py:151-157)
  weights                  the nn.Linear / nn.LayerNorm parameters exactly as stored ((N,K)
                           row-major): both GEMM operands are K-contiguous, no repacking
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import typing
import weakref

import numpy as np
import torch

from . import _lib, kernels
from ._lib import VhArDecoderDesc, VhForwardDesc, VhLayer, check, ptr, stream

HEAD_DIM = kernels.HEAD_DIM


class KVCache:
    """(L, 2, B, h, S_max, head_dim) in one allocation; `length` rows are valid for every batch row
    unless a per-row `cache_len` tensor says otherwise."""

    def __init__(self, n_layers, batch, n_heads, s_max, device, dtype=torch.float32, head_dim=HEAD_DIM):
        self.buf = torch.empty(n_layers, 2, batch, n_heads, s_max, head_dim, device=device, dtype=dtype)
        self.n_layers, self.batch, self.n_heads, self.s_max = n_layers, batch, n_heads, s_max
        self.head_dim = head_dim

    @property
    def bf16(self):
        return self.buf.dtype == kernels.H16

    def narrowed(self, s_max):
        """A bf16 cache of `s_max` rows per (layer, K|V, row, head) stream holding this fp32 cache's rows (round to
        nearest even, vh_kv_to_bf16): the decode steps of perf mode read half the bytes."""
        if self.bf16 or s_max < self.s_max:
            raise _lib.VhError('KVCache.narrowed: an fp32 cache and s_max >= its length')
        if self.head_dim != HEAD_DIM:
            raise _lib.VhError(f'KVCache.narrowed: the bf16 cache is width 64 only (head width {self.head_dim})')
        out = KVCache(self.n_layers, self.batch, self.n_heads, s_max, self.buf.device, dtype=kernels.H16)
        check(_lib.lib().vh_kv_to_bf16(ptr(self.buf), ptr(out.buf), self.n_layers * 2 * self.batch * self.n_heads,
                                       self.s_max, self.s_max, s_max, stream()), 'vh_kv_to_bf16')
        return out

    def narrow_into(self, dst: 'KVCache'):
        """`narrowed` into an existing 16-bit cache of the same streams and at least this cache's rows (a decoder slot keeps
        its 16-bit prefix cache across calls: the captured graphs point at it)."""
        if self.bf16 or not dst.bf16 or dst.s_max < self.s_max or self.head_dim != HEAD_DIM or \
                (dst.n_layers, dst.batch, dst.n_heads, dst.head_dim) != (self.n_layers, self.batch, self.n_heads, self.head_dim):
            raise _lib.VhError('KVCache.narrow_into: an fp32 width-64 cache into a 16-bit cache of the same streams')
        check(_lib.lib().vh_kv_to_bf16(ptr(self.buf), ptr(dst.buf), self.n_layers * 2 * self.batch * self.n_heads,
                                       self.s_max, self.s_max, dst.s_max, stream()), 'vh_kv_to_bf16')
        return dst

    def group_view(self, g):
        """A one-row KVCache over row g's streams of this cache (no copy): a prompt pass writes ONE group's region of a grouped
        prefix cache through it — the refill of generate_queued — while the decoder's layer table keeps pointing at the whole."""
        if not 0 <= g < self.batch:
            raise _lib.VhError(f'KVCache.group_view: row {g} of {self.batch}')
        view = object.__new__(KVCache)
        view.buf = self.buf[:, :, g:g + 1]
        view.n_layers, view.batch, view.n_heads, view.s_max, view.head_dim = self.n_layers, 1, self.n_heads, self.s_max, self.head_dim
        return view

    def unpack_into(self, dst: 'KVCache', seg_start, seg_len, dst_row):
        """The rows a packed forward left in this ONE-ROW cache, to rows of `dst` (a row cache or a grouped prefix cache of the
        same layers and heads): rows seg_start[s] .. + seg_len[s] - 1 of every (layer, K|V, head) go to positions 0 ..
        seg_len[s] - 1 of dst's row dst_row[s], in one launch and bit for bit (`kernels.kv_unpack`; a 16-bit cache into a
        16-bit cache: `kernels.kv_unpack_bf16`); the tables are device int32 tensors of one entry per segment.  Nothing else
        of dst is written."""
        if self.bf16 != dst.bf16:
            raise _lib.VhError('KVCache.unpack_into: mixed dtypes (an fp32 cache into an fp32 cache, a 16-bit cache into a 16-bit cache)')
        if self.batch != 1 or self.head_dim != HEAD_DIM or \
                (dst.n_layers, dst.n_heads, dst.head_dim) != (self.n_layers, self.n_heads, self.head_dim):
            raise _lib.VhError('KVCache.unpack_into: a one-row fp32 width-64 cache into an fp32 cache of the same layers and heads '
                               '(or both 16-bit)')
        (kernels.kv_unpack_bf16 if self.bf16 else kernels.kv_unpack)(self.buf, dst.buf, seg_start, seg_len, dst_row)
        return dst

    def k(self, i):
        return self.buf[i, 0]

    def v(self, i):
        return self.buf[i, 1]


def _layer_params(layer):
    """The 11 parameter tensors of one EncoderLayer in VhLayer order."""
    at, ff = layer.self_attn, layer.ffn
    n1 = layer.norm1.norm if hasattr(layer.norm1, 'project_layer') else layer.norm1
    n2 = layer.norm2.norm if hasattr(layer.norm2, 'project_layer') else layer.norm2
    return (n1.weight, n1.bias, at.qkv.weight, at.out.weight, at.out.bias, n2.weight, n2.bias,
            ff.linear_1.weight, ff.linear_1.bias, ff.linear_2.weight, ff.linear_2.bias)


FOLD_LAYERNORM = os.environ.get('VALLE2_FOLD_LN', '1') != '0'   # LayerNorm folded into the QKV / linear_1
                                                                 # weights (vh_ln_fold); without it the decode step
                                                                 # normalises in the operand load and the FeedForward
                                                                 # runs as linear_1 + split-K linear_2 + reduce


_WEIGHTS_EPOCH = 0
# Derived weights (folded LayerNorm forms, AdaLN tables, bf16 copies) per Transformer module.  Kept HERE, not in the
# module's __dict__: the entries hold weak references and device tensors that torch.save(model) must not try to pickle, and
# an entry dies with its module.
_DERIVED = weakref.WeakKeyDictionary()


def _derived(module) -> dict:
    d = _DERIVED.get(module)
    if d is None:
        d = _DERIVED[module] = {}
    return d


def bump_weights_epoch():
    """Invalidate every derived weight form (folded LayerNorm weights, AdaLN tables, bf16 copies).  Called by code that
    rewrites parameters behind torch's back (the flat optimizer kernel) — and the hook for USER code that does: the caches
    are keyed on (tensor identity, `_version`, `data_ptr`), and a write through `p.data` (an EMA swap by
    `p.data.copy_(...)`) moves none of them.  After such a write call this (or `invalidate_derived`)."""
    global _WEIGHTS_EPOCH
    _WEIGHTS_EPOCH += 1


def invalidate_derived(module=None):
    """Drop the derived weights of `module` (a Transformer), or of every module when None."""
    if module is None:
        _DERIVED.clear()
        bump_weights_epoch()
    else:
        _DERIVED.pop(module, None)


MAX_DECODE_D_MODEL = 4096       # vh_layernorm (the prompt pass) and the wide folded decode GEMMs end here (plan.hip decoder_check)


WIDE_FOLD_MAX_ROWS = 16         # decode rows up to which a d_model > 1024 step takes the folded GEMMs (ArDecoder)


BASE_FOLD_WIDTHS = (640, 768, 896)      # 10 / 12 / 14 heads of width 64: the folded chain of 512 at PW 5..7 (fp32 weights only)


def ffn_fused_width(d: int) -> bool:
    """d_model at which the decoder plan takes vh_ffn_decode by default (plan.hip decoder_enqueue)."""
    return d <= 512 or d in BASE_FOLD_WIDTHS


def folded_width(d: int) -> bool:
    """K of the folded-LayerNorm decode GEMMs, as the library's dispatch plan has them (gemm.hip gemm_plan): the four narrow shapes, 640 / 768 / 896, or 256 PW
    passes with PW in 5..8 and one or two passes — a multiple of 256 from 1280 to 2048, of 512 from 2560 to 4096."""
    return _lib.linear_form(_lib.ENTRY_LINEAR, 1, 16, d, ln_kind=_lib.LN_FOLDED) is not None


def head_fused_shape(batch: int, V: int, d: int) -> bool:
    """Rows and d_model vh_head_greedy (head + greedy step in one launch) has a kernel for."""
    return _lib.linear_form(_lib.ENTRY_HEAD_GREEDY, batch, V, d) is not None


def w16_width(d: int) -> bool:
    """d_model at which the decode step's QKV product has a 16-bit-weight form (vh_linear_qkv_folded_kv16 with h16 weights)."""
    return _lib.linear_form(_lib.ENTRY_QKV_KV16, 1, 3 * d, d, ln_kind=_lib.LN_FOLDED, w16=True) is not None


def folded_layer_norms(transformer):
    """Per layer ((Wqkv∘γ1, c1, c2), (W1∘γ2, c1, c2)) for the decode step, or None when the shape is
    outside the folded kernels (d_model not in {128,256,512,640,768,896,1024} and not one of 1280 .. 2048 in steps of 256 / 2560 .. 4096 in steps of 512) or the
    norms are adaptive.  Cached on the module and rebuilt when any of the source parameters changed (optimizer step, load)."""
    layers = list(transformer.layers)
    d = transformer.hparams.d_model
    if (not FOLD_LAYERNORM or not folded_width(d) or transformer.hparams.dim_feedforward % 16
            or any(hasattr(l.norm1, 'project_layer') for l in layers)):
        return None
    srcs = [(l.norm1.weight, l.norm1.bias, l.self_attn.qkv.weight, l.norm2.weight, l.norm2.bias,
             l.ffn.linear_1.weight, l.ffn.linear_1.bias) for l in layers]
    key = (_WEIGHTS_EPOCH,) + tuple((t.data_ptr(), t._version) for ps in srcs for t in ps)
    cached = _derived(transformer).get('folded')
    if cached is not None and cached[0] == key:
        return cached[1]
    with torch.no_grad():
        folded = [(kernels.ln_fold(wq.detach(), g1.detach(), b1.detach()),
                   kernels.ln_fold(w1.detach(), g2.detach(), b2.detach(), bias1.detach()))
                  for g1, b1, wq, g2, b2, w1, bias1 in srcs]
    _derived(transformer)['folded'] = (key, folded)
    return folded


def layer_table(transformer, cache: KVCache, folded=None):
    """ctypes array of VhLayer for `transformer.layers` bound to `cache`."""
    layers = list(transformer.layers)
    arr = (VhLayer * len(layers))()
    for i, layer in enumerate(layers):
        ps = _layer_params(layer)
        for (name, _), t in zip(VhLayer._fields_[:11], ps):
            if t.dtype != torch.float32:
                raise _lib.VhError(f'parameter {name} of layer {i} is {t.dtype}; the path is fp32')
            setattr(arr[i], name, ptr(t.detach()))
        if cache is not None:
            arr[i].kcache = ptr(cache.k(i))
            arr[i].vcache = ptr(cache.v(i))
        if folded is not None:
            (arr[i].wqkv_f, arr[i].qkv_c1, arr[i].qkv_c2), (arr[i].w1_f, arr[i].w1_c1, arr[i].w1_c2) = (
                tuple(ptr(t) for t in folded[i][0]), tuple(ptr(t) for t in folded[i][1]))
    return arr


def adaln_table(transformer, embedding):
    """(L, 2, 2, d) [layer][norm1|norm2][scale|shift] = project_layer(embedding) for every AdaptiveLayerNorm of the
    stack (valle/models/modules.py:94-98) in ONE launch (`vh_adaproj_fwd`, the training path's kernel: a wave per 8
    output rows of one of the 2 L Linears), instead of 2 L single-row GEMV launches from Python.

    The table of a stage depends on the stage embedding and the projection weights only, so it is kept per embedding
    TENSOR OBJECT (a weak reference: a parameter such as stage_embs[n].weight lives as long as the model; an ad-hoc
    tensor's entry dies with it, and a recycled address can never alias a live entry) and reused while neither that
    tensor's version, nor any projection parameter's, nor the weights epoch (flat optimizer steps) has moved — the 7
    stages of ValleNAR.generate_batch build 7 tables once, not 7 per call."""
    layers = list(transformer.layers)
    d = embedding.shape[-1]
    projs = [(n.project_layer.weight, n.project_layer.bias) for l in layers for n in (l.norm1, l.norm2)]
    n = len(projs)
    state = _derived(transformer).setdefault('ada', {'items': None, 'tables': []})
    pkey = (_WEIGHTS_EPOCH,) + tuple(x for w, b in projs for x in (w.data_ptr(), w._version, b.data_ptr(), b._version))
    for ref, ver, key, table in state['tables']:
        if ref() is embedding and ver == embedding._version and key == pkey and table.device == embedding.device:
            return table
    # (room for one table per stage of a 32-codebook NAR: 31 stage embeddings)
    state['tables'] = [e for e in state['tables'] if e[0]() is not None and e[0]() is not embedding][-31:]
    if any(tuple(w.shape) != (2 * d, d) or not w.is_contiguous() or w.dtype != torch.float32 for w, _ in projs):
        raise _lib.VhError('adaln_table: project_layer weights must be contiguous fp32 (2 d, d)')
    ptrs = tuple(x for w, b in projs for x in (w.data_ptr(), b.data_ptr()))
    if state['items'] is None or state['items'][0] != ptrs or state['items'][1].device != embedding.device:
        rec = np.zeros(n, dtype=[('w', 'u8'), ('b', 'u8'), ('dw', 'u8'), ('db', 'u8')])
        for i, (w, b) in enumerate(projs):
            rec[i] = (w.data_ptr(), b.data_ptr(), 0, 0)
        state['items'] = (ptrs, _lib.to_device_async(torch.from_numpy(rec.view(np.uint8).copy()), embedding.device))
    emb = embedding.detach().reshape(-1).contiguous()
    with torch.inference_mode(False):            # a normal tensor: the cached table outlives an inference_mode() caller
        out = torch.empty(n, 2 * d, device=emb.device, dtype=torch.float32)
    check(_lib.lib().vh_adaproj_fwd(ptr(state['items'][1]), n, ptr(emb), ptr(out), 2 * d, d, stream()), 'vh_adaproj_fwd')
    table = out.view(len(layers), 2, 2, d)
    try:
        state['tables'].append((weakref.ref(embedding), embedding._version, pkey, table))
    except TypeError:
        pass
    return table


def bf16_weights(transformer):
    """Per layer (Wqkv, Wo, W1, W2) as bf16 (vh_to_bf16, round to nearest even) for the perf-mode forward; built once per
    weight set (same cache rule as `folded_layer_norms`)."""
    layers = list(transformer.layers)
    srcs = [(l.self_attn.qkv.weight, l.self_attn.out.weight, l.ffn.linear_1.weight, l.ffn.linear_2.weight) for l in layers]
    key = (_WEIGHTS_EPOCH,) + tuple((t.data_ptr(), t._version) for ps in srcs for t in ps)
    cached = _derived(transformer).get('bf16')
    if cached is not None and cached[0] == key:
        return cached[1]
    with torch.no_grad(), torch.inference_mode(False):
        out = [tuple(kernels.to_bf16(t.detach()) for t in ps) for ps in srcs]
    _derived(transformer)['bf16'] = (key, out)
    return out


def head16(module, weight):
    """The h16 copy of a head matrix (V, d) for the perf-mode NAR stage (valle_nar.py: the stage's projection over every target
    frame is a large-M product like the stack's; fp32 it was 0.5 of a 10 ms stage) — None when the 16-bit tile GEMM does not
    take the shape.  Built once per weight version, cached on the owning module like the other derived forms."""
    V, d = weight.shape
    if V % 128 or d % 64:
        return None
    cache = _derived(module).setdefault('head16', {})
    key = (_WEIGHTS_EPOCH, weight.data_ptr(), weight._version)
    hit = cache.get(id(weight))
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad(), torch.inference_mode(False):
        w16 = kernels.to_bf16(weight.detach())
    cache[id(weight)] = (key, w16)
    return w16


# perf mode's decode step over h16 copies of its four matrices (+ the head): built in round 6, measured SLOWER (471.1 vs 463.9 us per
# step at 32 rows x 12L/512d, profiles/r6_ab_decode_w16.log — the chain's launches are round trips, not byte streams, and an 8-byte
# fragment per lane halves the useful part of every line it touches) — so it is opt-in: VALLE2_DECODE_W16=1
DECODE_W16 = os.environ.get('VALLE2_DECODE_W16', '0') == '1'


def decode_weights16(transformer, folded):
    """Per layer (Wqkv∘γ1, Wo, W1∘γ2, W2, c1 of Wqkv∘γ1, c1 of W1∘γ2) for the PERF-MODE decode step (the second half of SURVEY
    section 7's perf mode: 16-bit storage of what a step streams, fp32 accumulate): the four matrices as h16 — the folded ones
    narrowed AFTER the fold — and the epilogue's c1 of the two folded ones summed over the ROUNDED matrix, so that
    rstd * (x Wf16^T - mean * c1) is LayerNorm(x) Wf16^T exactly.  With the c1 of the unrounded fold the epilogue leaves
    rstd * mean * (rowsum(Wf16) - c1): nothing for a centred row, 2e-2 on the logits of a row whose mean is 20 standard
    deviations (tests/test_decode_w16_cpu.py).  c2 stays the fp32 sum of the fold.  Built once per weight set, beside the
    folded weights."""
    layers = list(transformer.layers)
    key = (_WEIGHTS_EPOCH, id(folded)) + tuple((t.data_ptr(), t._version) for l in layers
                                               for t in (l.self_attn.out.weight, l.ffn.linear_2.weight))
    cached = _derived(transformer).get('decode16')
    if cached is not None and cached[0] == key:
        return cached[1]
    with torch.no_grad(), torch.inference_mode(False):
        out = []
        for i, l in enumerate(layers):                # (the row sums: once per weight set, in float64 — nothing a step runs)
            wq, w1 = kernels.to_bf16(folded[i][0][0]), kernels.to_bf16(folded[i][1][0])
            out.append((wq, kernels.to_bf16(l.self_attn.out.weight.detach()), w1, kernels.to_bf16(l.ffn.linear_2.weight.detach()),
                        wq.double().sum(1).float().contiguous(), w1.double().sum(1).float().contiguous()))
    _derived(transformer)['decode16'] = (key, out, folded)       # (the folded list is kept alive: its id is part of the key)
    return out


class ForwardScratch16:
    """bf16 activations of the perf-mode forward: xn, q, attn (rows, d) and hidden (rows, dff)."""

    def __init__(self, rows, d, dff, device):
        bf = dict(device=device, dtype=kernels.H16)
        self.xn = torch.empty(rows, d, **bf)
        self.q = torch.empty(rows, d, **bf)
        self.attn = torch.empty(rows, d, **bf)
        self.hidden = torch.empty(rows, dff, **bf)


def perf_forward_supported(cfg):
    """Shapes the bf16 tile kernels serve: d_model = n_heads x 64, d_model and dim_feedforward multiples of 128."""
    return cfg.d_model == cfg.n_heads * HEAD_DIM and cfg.d_model % 128 == 0 and cfg.dim_feedforward % 128 == 0


def _adaln(transformer, embedding):
    """The stack's `adaln_table` for `embedding`; None for a stack of plain LayerNorms."""
    if transformer.hparams.norm == 'LayerNorm':
        return None
    if embedding is None:
        raise TypeError('AdaptiveLayerNorm needs `embedding` (reference: Linear(None) TypeError)')
    return adaln_table(transformer, embedding)


def _check_x(x):
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise _lib.VhError('x must be contiguous fp32')


def _check_cache(cache, cfg, batch, rows, *, bf16=None, head=None, text=None):
    """A forward over `batch` x `rows` writes its K/V to `cache`: refuse one it does not fit.  bf16: the storage the forward
    writes (None: not looked at); head: the (n_heads, head_dim) it writes (None: not looked at)."""
    if cache is None or cache.batch != batch or cache.s_max < rows or cache.n_layers != cfg.num_layers or \
            (bf16 is not None and cache.bf16 != bf16) or (head is not None and (cache.n_heads, cache.head_dim) != head):
        raise _lib.VhError(text or 'KV cache does not fit this forward')


def _forward_front(transformer, x, batch, rows, cache, embedding, scratch, bf16=None):
    """What the native front-ends do alike once their own refusals have passed: x and the cache checked, the default scratch,
    and the fields the fp32 and the 16-bit descriptor share.  bf16=True: the perf-mode forward (16-bit cache and scratch, the
    layer table not bound to the cache).  Returns (scratch, fields)."""
    cfg = transformer.hparams
    _check_x(x)
    _check_cache(cache, cfg, batch, rows, bf16=bf16,
                 text='perf mode needs a bf16 KV cache that fits this forward' if bf16 else None)
    d = x.shape[-1]
    scratch = scratch or (ForwardScratch16 if bf16 else ForwardScratch)(batch * rows, d, cfg.dim_feedforward, x.device)
    return scratch, dict(B=batch, T=rows, d_model=d, n_heads=cfg.n_heads, dff=cfg.dim_feedforward, n_layers=cfg.num_layers,
                         S_max=cache.s_max, ln_eps=1e-5, layers=layer_table(transformer, None if bf16 else cache),
                         ada=ptr(_adaln(transformer, embedding)), x=ptr(x))


def _fp32_scratch_fields(scratch):
    return dict(xn=ptr(scratch.xn), q=ptr(scratch.q), attn=ptr(scratch.attn), hidden=ptr(scratch.hidden),
                gemm_ws=ptr(scratch.ws), gemm_ws_bytes=scratch.ws_bytes)


def _refuse_unless_perf_forward(cfg):
    if not perf_forward_supported(cfg):
        raise _lib.VhError(f'perf mode needs d_model = n_heads x 64 and d_model, dim_feedforward multiples of 128 '
                           f'(got {cfg.d_model}, {cfg.n_heads}, {cfg.dim_feedforward})')


def _forward16_desc(transformer, cache, scratch, common, **fields):
    """The 16-bit descriptor of both perf-mode forwards: the narrowed weights and the cache of every layer, the 16-bit scratch
    and `common` (`_forward_front`)."""
    t16 = (_lib.VhLayer16 * transformer.hparams.num_layers)()
    for i, (wq, wo, w1, w2) in enumerate(bf16_weights(transformer)):
        t16[i].wqkv, t16[i].wo, t16[i].w1, t16[i].w2 = wq.data_ptr(), wo.data_ptr(), w1.data_ptr(), w2.data_ptr()
        t16[i].kcache16, t16[i].vcache16 = cache.k(i).data_ptr(), cache.v(i).data_ptr()
    return _lib.VhForward16Desc(
        layers16=t16, xn16=scratch.xn.data_ptr(), q16=scratch.q.data_ptr(), attn16=scratch.attn.data_ptr(),
        hidden16=scratch.hidden.data_ptr(), **fields, **common)


def transformer_forward_bf16(transformer, x, cache: 'KVCache', *, mode, x_len=0, x_len_dev=None, kv_len=None, embedding=None,
                             scratch=None, x_in=None):
    """`transformer_forward` in PERF MODE (SECONDARY): every product of the stack on the bf16 matrix
    cores (bf16 operands, fp32 accumulators), residual stream x fp32 in place, K/V written to a bf16 cache.  Analytic
    masks only.  Teacher-forced logits agree with the reference to 5e-2, not to the parity path's 2e-4."""
    cfg = transformer.hparams
    B, T, d = x.shape
    _refuse_unless_perf_forward(cfg)
    scratch, common = _forward_front(transformer, x, B, T, cache, embedding, scratch, bf16=True)
    desc = _forward16_desc(transformer, cache, scratch, common, mode=mode, x_len=int(x_len), x_len_dev=ptr(x_len_dev),
                           kv_len=ptr(kv_len), x_in=ptr(x_in))
    check(_lib.lib().vh_transformer_forward_bf16(C.byref(desc), stream()), 'vh_transformer_forward_bf16')
    return x


class ForwardScratch:
    def __init__(self, rows, d, dff, device):
        self.xn = torch.empty(rows, d, device=device, dtype=torch.float32)
        self.q = torch.empty(rows, d, device=device, dtype=torch.float32)
        self.attn = torch.empty(rows, d, device=device, dtype=torch.float32)
        self.hidden = torch.empty(rows, dff, device=device, dtype=torch.float32)
        L = _lib.lib()
        self.ws_bytes = max(L.vh_linear_ws_bytes(rows, d, d), L.vh_linear_ws_bytes(rows, d, dff),
                            L.vh_linear_ws_bytes(rows, dff, d))
        self.ws = torch.zeros(self.ws_bytes // 4, device=device, dtype=torch.float32) if self.ws_bytes else None
        self.d, self.dff = d, dff

    def fit(self, rows):
        """Make the GEMM workspace fit a forward over `rows` <= the constructor's rows: the split-K plan of vh_linear_ws cuts
        K >= 1024 deeper the FEWER output tiles there are, so a shorter forward can need more than the longest one."""
        L = _lib.lib()
        need = max(L.vh_linear_ws_bytes(rows, self.d, self.d), L.vh_linear_ws_bytes(rows, self.d, self.dff),
                   L.vh_linear_ws_bytes(rows, self.dff, self.d))
        if need > self.ws_bytes:
            self.ws_bytes = need
            self.ws = torch.zeros(need // 4, device=self.xn.device, dtype=torch.float32)
        return self


def transformer_forward(transformer, x, cache: KVCache, *, mode, x_len=0, x_len_dev=None,
                        kv_len=None, mask=None, pad=None, embedding=None, scratch=None, x_in=None):
    """Run all layers over x (B, T, d) IN PLACE (valle/models/modules.py:341-349), writing each
    layer's K/V to `cache` rows 0..T-1.  Returns x.  With `x_in` (same shape, contiguous) the input rows are
    read from there and left untouched, x is output only."""
    cfg = transformer.hparams
    B, T, d = x.shape
    if x_in is not None and (tuple(x_in.shape) != tuple(x.shape) or x_in.dtype != torch.float32):
        raise _lib.VhError('x_in must match x')
    if d != cfg.n_heads * HEAD_DIM:                          # a head width the native composite is not built for
        # (a cache of this width is filled from the projections; any other cache argument is not this path's)
        kv = cache if cache is not None and getattr(cache, 'head_dim', HEAD_DIM) == d // cfg.n_heads else None
        return _transformer_forward_generic(transformer, x, mode=mode, x_len=x_len, x_len_dev=x_len_dev, kv_len=kv_len,
                                            mask=mask, pad=pad, embedding=embedding, x_in=x_in, cache=kv)
    scratch, common = _forward_front(transformer, x, B, T, cache, embedding, scratch)
    desc = VhForwardDesc(mode=mode, x_len=int(x_len), x_len_dev=ptr(x_len_dev), kv_len=ptr(kv_len), mask=ptr(mask), pad=ptr(pad),
                         x_in=ptr(x_in), **_fp32_scratch_fields(scratch), **common)
    check(_lib.lib().vh_transformer_forward(C.byref(desc), stream()), 'vh_transformer_forward')
    return x


PACK_QUERY_BLOCK = 128            # queries one workgroup of vh_attn_rows_packed takes (attention.hip QB)


def pack_plan(lengths):
    """The packed layout of a ragged batch (pure Python, no device): utterance b's `lengths[b]` rows sit at rows
    starts[b] .. starts[b] + lengths[b] - 1 of one (M, d) buffer, no gaps.  Returns (starts, M, blocks): starts the exclusive
    prefix sum, M the sum, blocks the (segment, first query) of every 128-query block of every segment — each query once —
    with the blocks of the LONGEST segment first (they visit the most key tiles; ties keep the batch order)."""
    lengths = [int(n) for n in lengths]
    if not lengths:
        raise ValueError('pack_plan: no lengths')
    if min(lengths) < 1:
        raise ValueError(f'pack_plan: every length must be >= 1, got {min(lengths)}')
    starts, m = [], 0
    for n in lengths:
        starts.append(m)
        m += n
    order = sorted(range(len(lengths)), key=lambda s: -lengths[s])
    blocks = [(s, q0) for s in order for q0 in range(0, lengths[s], PACK_QUERY_BLOCK)]
    return starts, m, blocks


PACK_BWD_CHUNK_KEYS = 256         # keys one workgroup of vh_attn_rows_bwd_packed takes (attention.hip FKMAX: the eight-wave kernel)


def _text_lengths(what, x_lens, lengths):
    """The text length inside each segment as ints (None stays None: the full mask), refused under the caller's name `what`
    unless there is one per segment and it lies inside its segment."""
    if x_lens is None:
        return None
    x_lens = [int(x) for x in x_lens]
    if len(x_lens) != len(lengths) or any(not 0 <= x <= n for x, n in zip(x_lens, lengths)):
        raise ValueError(f'{what}: one text length per segment, 0 <= x_len <= length')
    return x_lens


def pack_bwd_plan(lengths, chunk_keys=PACK_BWD_CHUNK_KEYS, x_lens=None):
    """The work items of the packed attention backward (pure Python, no device): every segment's keys in chunks of
    `chunk_keys` (a multiple of 32, at most 256; the last chunk of a segment may be short).  Returns (items, max_chunks):
    items the (segment, chunk) pairs, each once, HEAVIEST first — weight = the chunk's keys x the 32-query tiles it visits:
    all of the segment's, or under the prefix mask (x_lens given: the text length inside each segment) only those from the
    chunk's first key on when that key lies past the text; ties keep (segment, chunk) order — and max_chunks the largest
    chunk count of a segment (the dQ slabs the launch needs; 1: none)."""
    lengths = [int(n) for n in lengths]
    chunk_keys = int(chunk_keys)
    if not lengths:
        raise ValueError('pack_bwd_plan: no lengths')
    if min(lengths) < 1:
        raise ValueError(f'pack_bwd_plan: every length must be >= 1, got {min(lengths)}')
    if chunk_keys < 32 or chunk_keys > 256 or chunk_keys % 32:
        raise ValueError(f'pack_bwd_plan: chunk_keys={chunk_keys} must be a multiple of 32 in 32..256')
    x_lens = _text_lengths('pack_bwd_plan', x_lens, lengths)
    weighted = []
    for s, n in enumerate(lengths):
        tiles = (n + 31) // 32
        for c in range((n + chunk_keys - 1) // chunk_keys):
            k0 = c * chunk_keys
            first = k0 // 32 if x_lens is not None and k0 >= x_lens[s] else 0
            weighted.append((-(min(chunk_keys, n - k0) * (tiles - first)), s, c))
    weighted.sort()
    return [(s, c) for _, s, c in weighted], (max(lengths) + chunk_keys - 1) // chunk_keys


class PackedRows:
    """`pack_plan(lengths)` as device int32 tensors, built once per call: what `kernels.attn_rows_packed` and
    `transformer_forward_packed` take.  x_lens (packed training under the prefix mask): the text length inside each segment;
    `bwd_table` is the backward's work table (`pack_bwd_plan`), built on first use."""

    def __init__(self, lengths, device, x_lens=None):
        self.lengths = [int(n) for n in lengths]
        self.starts, self.rows, blocks = pack_plan(self.lengths)
        self.n_seg, self.n_blocks = len(self.lengths), len(blocks)
        i32 = self._i32 = lambda v: _lib.to_device_async(torch.tensor(v, dtype=torch.int32), device)   # noqa: E731
        self.seg_start, self.seg_len, self.blocks = i32(self.starts), i32(self.lengths), i32(blocks)
        self.x_lens = _text_lengths('PackedRows', x_lens, self.lengths)
        self.seg_x_len = None if x_lens is None else i32(self.x_lens)
        self._bwd = {}

    def bwd_table(self, chunk_keys=None):
        """(chunk_keys, max_chunks, items as a device int32 tensor, n_items) of `pack_bwd_plan`, cached per chunk_keys."""
        chunk_keys = PACK_BWD_CHUNK_KEYS if chunk_keys is None else int(chunk_keys)
        if chunk_keys not in self._bwd:
            items, max_chunks = pack_bwd_plan(self.lengths, chunk_keys, self.x_lens)
            self._bwd[chunk_keys] = (chunk_keys, max_chunks, self._i32(items), len(items))
        return self._bwd[chunk_keys]


def nar_train_plan(x_lens, a_lens, prefixes):
    """The packed layout of a NAR training batch (pure Python, no device): utterance b's rows [x_lens[b] text | a_lens[b]
    frames] lie back to back, its first prefixes[b] frames are the acoustic prefix (all codebooks, no target) and the rest
    are targets.  Returns (starts, M, target_rows, target_frames, weights): starts the first row of every utterance, M the
    row count, target_rows the packed row of every target frame and target_frames its (b, t), both utterance by utterance
    and frame by frame, weights the share (a_len_b - prefix_b) / sum of each utterance in the mean over target frames."""
    x_lens, a_lens, prefixes = ([int(v) for v in seq] for seq in (x_lens, a_lens, prefixes))
    if not x_lens or len(a_lens) != len(x_lens) or len(prefixes) != len(x_lens):
        raise ValueError('nar_train_plan: one text length, frame count and prefix per utterance')
    if min(x_lens) < 1 or min(a_lens) < 1:
        raise ValueError('nar_train_plan: every length must be >= 1')
    if any(not 0 <= p < a for p, a in zip(prefixes, a_lens)):
        raise ValueError('nar_train_plan: 0 <= prefix < frames for every utterance (at least one target frame)')
    starts, _, _ = pack_plan([x + a for x, a in zip(x_lens, a_lens)])
    m = starts[-1] + x_lens[-1] + a_lens[-1]
    target_rows = [starts[b] + x_lens[b] + t for b in range(len(x_lens)) for t in range(prefixes[b], a_lens[b])]
    target_frames = [(b, t) for b in range(len(x_lens)) for t in range(prefixes[b], a_lens[b])]
    total = len(target_rows)
    return starts, m, target_rows, target_frames, [(a - p) / total for a, p in zip(a_lens, prefixes)]


class NarTrainLayout:
    """`nar_train_plan` as device tensors, built once per step: what `kernels.embed_nar_packed` and its backward take
    (seg_start, x_len, a_len, prefix: int32 (B); max_x_len, max_a_len, n_seg, rows) and the step's gathers (target_rows:
    int64 packed rows of the target frames; target_index: int64 b * width + t of each, into a (B, width) view of the
    codes).  `packed` is the `PackedRows` of the same segments for the attention."""

    def __init__(self, x_lens, a_lens, prefixes, width, device):
        self.x_lens, self.a_lens, self.prefixes = ([int(v) for v in seq] for seq in (x_lens, a_lens, prefixes))
        self.packed = PackedRows([x + a for x, a in zip(self.x_lens, self.a_lens)], device)
        self.starts, self.rows, self.n_seg = self.packed.starts, self.packed.rows, self.packed.n_seg
        if any(not 0 <= p < a for p, a in zip(self.prefixes, self.a_lens)) or min(self.x_lens) < 1:
            raise ValueError('NarTrainLayout: every text length >= 1 and 0 <= prefix < frames for every utterance')
        i32 = lambda v: _lib.to_device_async(torch.tensor(v, dtype=torch.int32), device)   # noqa: E731
        self.seg_start, self.x_len, self.a_len, self.prefix = self.packed.seg_start, i32(self.x_lens), i32(self.a_lens), i32(self.prefixes)
        self.max_x_len, self.max_a_len = max(self.x_lens), max(self.a_lens)
        # nar_train_plan's target lists as tensor arithmetic (the plan itself is the readable form, and what the tests hold
        # this against): a step of 16 k rows should not walk them in Python
        x, a, p, s0 = (torch.tensor(v, dtype=torch.int64) for v in (self.x_lens, self.a_lens, self.prefixes, self.starts))
        n = a - p
        b = torch.repeat_interleave(torch.arange(self.n_seg), n)
        t = torch.arange(int(n.sum())) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n) + p[b]
        self.n_targets = int(n.sum())
        self.weights = (n.double() / self.n_targets).tolist()
        self.target_rows = _lib.to_device_async(s0[b] + x[b] + t, device)
        self.target_index = _lib.to_device_async(b * int(width) + t, device)


class NarRows(typing.NamedTuple):
    """`nar_rows`: where the rows of a NAR batch lie in its one (rows, d) buffer.  Python ints and lists only."""
    packed: bool
    lengths: list             # len_b = tx_b + tc_b + ty_b (the packed kind: what `PackedRows` takes)
    starts: list              # first row of utterance b
    rows: int
    t0_prompt: list           # first row of utterance b's acoustic prompt
    t0_target: list           # ... of its target frames
    target_rows: list         # the row of every target frame, utterance by utterance and frame by frame
    logit_starts: list        # where utterance b's run starts in the gathered target rows (B + 1 entries)
    kv_len: list | None       # the padded kind: every utterance's keys, None where all lengths are equal


def nar_rows(txs, tcs, tys, packed: bool) -> NarRows:
    """The row layout of ValleNAR's stage loop for B utterances [text_b | prompt_b | target_b] of txs[b] + tcs[b] + tys[b]
    rows (pure Python, no device).  Padded: utterance b at row b * max(len), the rows after its own are padding, each
    utterance attends its kv_len keys.  Packed: back to back as `pack_plan` lays them out, no padding row.  The padded
    layout is the packed one with other starts; everything that places a row reads `starts`."""
    lengths = [int(a) + int(b) + int(c) for a, b, c in zip(txs, tcs, tys)]
    if packed:
        starts, rows, _ = pack_plan(lengths)
    else:
        starts, rows = [b * max(lengths) for b in range(len(lengths))], len(lengths) * max(lengths)
    t0_prompt = [s + a for s, a in zip(starts, txs)]
    t0_target = [s + c for s, c in zip(t0_prompt, tcs)]
    target_rows, logit_starts = [], [0]
    for t0, ty in zip(t0_target, tys):
        target_rows.extend(range(t0, t0 + ty))
        logit_starts.append(logit_starts[-1] + ty)
    return NarRows(packed, lengths, starts, rows, t0_prompt, t0_target, target_rows, logit_starts,
                   lengths if not packed and len(set(lengths)) > 1 else None)


class NarLayout:
    """`nar_rows` on the device, its int32 tensors uploaded once per call, and what depends on the kind of layout: the K/V
    cache and scratch a stack forward over the buffer needs, whether the buffer's rows must start as zeros (the padded
    kind's padding rows are read by the row-wise kernels; the packed kind writes every row) and the forward itself."""

    def __init__(self, txs, tcs, tys, packed, device):
        p = self.plan = nar_rows(txs, tcs, tys, packed)
        i32 = lambda v: _lib.to_device_async(torch.tensor(v, dtype=torch.int32), device)   # noqa: E731
        self.device, self.rows, self.zeroed = device, p.rows, not packed
        self.segments = PackedRows(p.lengths, device) if packed else None
        self.t0_text = self.segments.seg_start if packed else i32(p.starts)
        self.t0_prompt, self.t0_target = i32(p.t0_prompt), i32(p.t0_target)
        # (through numpy: torch.tensor() of a 40 k-entry list costs twice as long on the host)
        self.target_rows = _lib.to_device_async(torch.from_numpy(np.array(p.target_rows, dtype=np.int64)), device)
        self.kv_len = None if p.kv_len is None else i32(p.kv_len)

    def cache_and_scratch(self, cfg, perf_mode=False):
        """(KVCache, scratch) of one stack forward over the buffer: (1, rows) packed, (B, max(len)) padded — fp32, or 16-bit in
        perf mode (either kind)."""
        B = 1 if self.segments else len(self.plan.lengths)
        cache = KVCache(cfg.num_layers, B, cfg.n_heads, self.rows // B, self.device, dtype=kernels.H16 if perf_mode else torch.float32)
        return cache, (ForwardScratch16 if perf_mode else ForwardScratch)(self.rows, cfg.d_model, cfg.dim_feedforward, self.device)

    def forward(self, transformer, x, cache, scratch, embedding):
        """The stack under the full mask over x (rows, d) in place, every utterance attending its own rows."""
        if self.segments:
            return packed_forward_for(cache, lm=False)(transformer, x, cache, self.segments, embedding=embedding, scratch=scratch)
        forward = transformer_forward_bf16 if cache.bf16 else transformer_forward
        return forward(transformer, x.view(cache.batch, -1, x.shape[-1]), cache, mode=kernels.MASK_FULL, kv_len=self.kv_len,
                       embedding=embedding, scratch=scratch)


def transformer_forward_packed(transformer, x, cache: KVCache, rows: PackedRows, embedding=None, scratch=None):
    """`transformer_forward(mode=MASK_FULL)` of a ragged batch over PACKED rows: x (M, d) holds utterance b at rows
    rows.starts[b] .. + rows.lengths[b] - 1 and is updated in place; each utterance attends its own rows only
    (`vh_attn_rows_packed`), every other launch is the row-wise one over M rows.  `cache`: a one-row KVCache of s_max >= M;
    each layer's K/V land at the packed rows.  Returns x."""
    return _packed_forward('transformer_forward_packed', transformer, x, cache, rows, lm=False, bf16=False, embedding=embedding,
                           scratch=scratch)


def _packed_forward(what, transformer, x, cache, rows, *, lm, bf16, embedding=None, scratch=None, lse2=None):
    """The four packed forwards (`what`: the one that was called, `vh_` + what its native entry): full mask or, lm, every
    segment's prefix-LM mask; fp32 or, bf16, perf mode.  Their refusals in one order, the descriptor, the call."""
    cfg = transformer.hparams
    if x.dim() != 2:
        raise _lib.VhError(f'{what}: x must be (M, d), got {tuple(x.shape)}')
    M, d = x.shape
    if d != cfg.n_heads * HEAD_DIM:
        raise _lib.VhError(f'{what}: head width {d // cfg.n_heads} (the packed attention is width 64 only)')
    if lm and cfg.norm != 'LayerNorm':
        raise _lib.VhError(f'{what}: norm={cfg.norm!r} (LayerNorm stacks only)')
    if M != rows.rows:
        raise _lib.VhError(f'{what}: x has {M} rows, the packed rows {rows.rows}')
    if lm:
        kernels.needs_x_lens(what, rows)
    if lm and not bf16:                     # the fp32 prefix-LM attention is the training forward's: it writes an lse2 nobody reads here
        if lse2 is None:
            lse2 = torch.empty(cfg.n_heads, M, device=x.device, dtype=torch.float32)
        elif tuple(lse2.shape) != (cfg.n_heads, M) or lse2.dtype != torch.float32 or not lse2.is_contiguous():
            raise _lib.VhError(f'{what}: lse2 must be contiguous float32 (n_heads, M)')
    if bf16:
        _refuse_unless_perf_forward(cfg)
    scratch, common = _forward_front(transformer, x, 1, M, cache, embedding, scratch, bf16=bf16)
    mode = dict(mode=kernels.MASK_PREFIX if lm else kernels.MASK_FULL, x_len=0)
    desc = _forward16_desc(transformer, cache, scratch, common, **mode) if bf16 else \
        VhForwardDesc(**mode, **_fp32_scratch_fields(scratch), **common)
    segments = [ptr(rows.seg_start), ptr(rows.seg_len)] + [ptr(rows.seg_x_len)] * lm + [rows.n_seg, ptr(rows.blocks), rows.n_blocks]
    check(getattr(_lib.lib(), 'vh_' + what)(C.byref(desc), *segments, *[ptr(lse2)] * (lm and not bf16), stream()), 'vh_' + what)
    return x


class PromptRows:
    """The packed layout of a ragged AR prompt pass (generation.prompt_pass), uploaded in ONE copy: utterance g's rows
    [txs[g] text | pls[g] BOS + prompt] lie back to back as `pack_plan` lays them out.  It stands for a `PackedRows` with text
    lengths (what `transformer_forward_packed_lm` takes) and for the segment tables of `kernels.embed_nar_packed` (x_len, a_len,
    prefix = 0: one codebook everywhere), and carries dst_row (the cache row each segment's K/V go to, `KVCache.unpack_into`)
    and last_rows (the packed row of each utterance's last position: where decoding starts from)."""

    def __init__(self, txs, pls, dst_rows, device):
        self.x_lens, a_lens, dst_rows = [int(t) for t in txs], [int(p) for p in pls], [int(r) for r in dst_rows]
        if not self.x_lens or len(a_lens) != len(self.x_lens) or len(dst_rows) != len(self.x_lens) or min(self.x_lens) < 0 or min(a_lens) < 1:
            raise ValueError('PromptRows: one text length >= 0, one BOS + prompt length >= 1 and one cache row per utterance')
        self.lengths = [t + p for t, p in zip(self.x_lens, a_lens)]
        self.starts, self.rows, blocks = pack_plan(self.lengths)
        n = self.n_seg = len(self.lengths)
        self.n_blocks = len(blocks)
        self.max_x_len, self.max_a_len = max(self.x_lens), max(a_lens)
        table = [self.starts, self.lengths, self.x_lens, a_lens, [0] * n, dst_rows,
                 [s + c - 1 for s, c in zip(self.starts, self.lengths)]]
        dev = _lib.to_device_async(torch.tensor([v for row in table for v in row] + [v for b in blocks for v in b],
                                                dtype=torch.int32), device)
        (self.seg_start, self.seg_len, self.seg_x_len, self.a_len, self.prefix, self.dst_row,
         self.last_rows) = (dev[i * n:(i + 1) * n] for i in range(7))
        self.x_len = self.seg_x_len
        self.blocks = dev[7 * n:].view(-1, 2)


def transformer_forward_packed_lm(transformer, x, cache: KVCache, rows, scratch=None, lse2=None):
    """`transformer_forward(mode=MASK_PREFIX)` of a ragged batch over PACKED rows, forward only: x (M, d) holds utterance b at
    rows rows.starts[b] .. + rows.lengths[b] - 1 and is updated in place; each utterance attends its own rows only, under the
    prefix-LM mask of its own text length rows.x_lens[b] (the packed training forward's kernel, `vh_attn_rows_packed_lse`: it
    writes the (n_heads, M) `lse2`, scratch nobody reads here); every other launch is the row-wise one over M rows.  `rows`: a
    `PackedRows` built with x_lens, or a `PromptRows`.  `cache`: a one-row fp32 KVCache of s_max >= M; each layer's K/V land at
    the packed rows (`KVCache.unpack_into` moves them to per-row caches).  fp32, head width 64, LayerNorm.  Returns x."""
    return _packed_forward('transformer_forward_packed_lm', transformer, x, cache, rows, lm=True, bf16=False, scratch=scratch, lse2=lse2)


def transformer_forward_packed_bf16(transformer, x, cache: KVCache, rows: PackedRows, embedding=None, scratch=None):
    """`transformer_forward_packed` in PERF MODE: `transformer_forward_bf16(mode=MASK_FULL)` of a ragged batch over packed rows.
    x (M, d) fp32 holds utterance b at rows rows.starts[b] .. + rows.lengths[b] - 1 and is updated in place; each utterance
    attends its own rows only (`vh_attn_rows_packed_bf16`), every other launch is the row-wise 16-bit one over M rows.
    `cache`: a one-row 16-bit KVCache of s_max >= M; `scratch`: a ForwardScratch16.  Returns x."""
    return _packed_forward('transformer_forward_packed_bf16', transformer, x, cache, rows, lm=False, bf16=True, embedding=embedding,
                           scratch=scratch)


def transformer_forward_packed_lm_bf16(transformer, x, cache: KVCache, rows, scratch=None):
    """`transformer_forward_packed_lm` in PERF MODE: `transformer_forward_bf16(mode=MASK_PREFIX)` of a ragged batch over packed
    rows, forward only.  x (M, d) fp32 holds utterance b at rows rows.starts[b] .. + rows.lengths[b] - 1 and is updated in place;
    each utterance attends its own rows only, under the prefix-LM mask of its own text length (`vh_attn_rows_packed_lm_bf16`),
    every other launch is the row-wise 16-bit one over M rows.  `rows`: a `PackedRows` built with x_lens, or a `PromptRows`.
    `cache`: a one-row 16-bit KVCache of s_max >= M (`KVCache.unpack_into` moves its rows to a 16-bit row cache); `scratch`: a
    ForwardScratch16.  Head width 64, LayerNorm, the shapes of `perf_forward_supported`.  Returns x."""
    return _packed_forward('transformer_forward_packed_lm_bf16', transformer, x, cache, rows, lm=True, bf16=True, scratch=scratch)


def packed_forward_for(cache, lm):
    """The packed forward that writes `cache`: 16-bit or fp32 by its storage; lm: under the prefix-LM masks, else the full mask."""
    return {(False, False): transformer_forward_packed, (False, True): transformer_forward_packed_lm,
            (True, False): transformer_forward_packed_bf16, (True, True): transformer_forward_packed_lm_bf16}[bool(cache.bf16), lm]


def _transformer_forward_generic(transformer, x, *, mode, x_len, x_len_dev, kv_len, mask, pad, embedding, x_in, cache=None):
    """`transformer_forward` for a head width other than 64 (valle/models/modules.py:109-111 allows any divisor of d_model;
    every configuration of the path and of the reference's tests has 64, which is what the flash kernels and the native
    composite are built for).  The same pre-norm stack layer by layer on the general kernels — LayerNorm, the tile / skinny
    GEMMs, materialised attention (`kernels.attn_generic`) — correct, not tuned.  With `cache` (a KVCache of this head
    width) every layer's K / V columns of the projection the attention used are copied into cache rows 0..T-1
    (`vh_kv_store`): the prompt pass of the cached decoder at these widths.  Without it nothing is cached."""
    cfg = transformer.hparams
    B, T, d = x.shape
    h = cfg.n_heads
    hd = d // h
    if hd % 4:
        raise _lib.VhError(f'head_dim {hd}: the general attention path needs a multiple of 4')
    _check_x(x)
    if cache is not None:
        _check_cache(cache, cfg, B, T, bf16=False, head=(h, hd))
    ada = _adaln(transformer, embedding)
    cur = (x_in if x_in is not None else x).reshape(B * T, d)
    spec = dict(mode=mode, x_len=int(x_len), x_len_dev=x_len_dev, kv_len=kv_len, mask=mask, pad=pad)
    f32 = dict(device=x.device, dtype=torch.float32)
    for i, layer in enumerate(transformer.layers):
        g1, b1, wqkv, wo, bo, g2, b2, w1, bb1, w2, bb2 = (t.detach() for t in _layer_params(layer))
        sc1, sh1, sc2, sh2 = (ada[i, 0, 0], ada[i, 0, 1], ada[i, 1, 0], ada[i, 1, 1]) if ada is not None else (None,) * 4
        xn = kernels.layernorm(cur, g1, b1, ada_scale=sc1, ada_shift=sh1, eps=layer.norm1.eps)
        qkv = kernels.linear(xn, wqkv, out=torch.empty(B * T, 3 * d, **f32))
        if cache is not None:
            kernels.kv_store(qkv, cache.k(i), cache.v(i), B, T)
        q, k, v = (qkv.view(B, T, 3, h, hd)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        attn = torch.empty(B * T, d, **f32)
        kernels.attn_generic(q, k, v, attn.view(B, T, h, hd).permute(0, 2, 1, 3), hd ** -0.5, **spec)
        nxt = kernels.linear(attn, wo, bo, residual=cur, out=torch.empty(B * T, d, **f32))
        xn = kernels.layernorm(nxt, g2, b2, ada_scale=sc2, ada_shift=sh2, eps=layer.norm2.eps)
        hid = kernels.linear(xn, w1, bb1, act=kernels.ACT_GELU, out=torch.empty(B * T, w1.shape[0], **f32))
        cur = kernels.linear(hid, w2, bb2, residual=nxt, out=torch.empty(B * T, d, **f32))
    x.reshape(B * T, d).copy_(cur)
    return x


def shared_n_split(batch: int, n_heads: int) -> int:
    """Key splits of the beams' own rows under a shared prompt (two workgroups per CU keep twice the loads in flight:
    profiles/r5_ab_shared_prompt.log).  VALLE2_SHARED_SPLIT: the A/B knob."""
    return int(os.environ.get('VALLE2_SHARED_SPLIT') or min(16, -(-512 // (batch * n_heads))))


def shared_prompt_fits(batch: int, n_heads: int, prefix_len: int) -> bool:
    """Whether vh_attn_decode_shared takes a prompt of prefix_len keys for `batch` beams (its merge serves at most 256
    records per (row, head): ceil(prefix_len / 32) prefix blocks + the suffix splits) — 4 beams x 8 heads: up to 7680 keys."""
    return _lib.attn_decode_form(_lib.ATTN_ENTRY_SHARED, batch, n_heads, shared_n_split(batch, n_heads), prefix=prefix_len) is not None


GROUP_PREFIX_STEP = 128           # grouped shared prompts: the prefix capacity is the longest prompt rounded up to this many keys


def group_prefix_cap(longest: int) -> int:
    """Prefix capacity (keys per group in the prefix cache, and what sizes the decode grid and the record stride) for prompts of
    at most `longest` keys: the next multiple of GROUP_PREFIX_STEP.  The decoder slot is keyed on it, not on the lengths, so
    calls whose prompts differ under one capacity replay the same captured graphs."""
    return -(-int(longest) // GROUP_PREFIX_STEP) * GROUP_PREFIX_STEP


def grouped_prompts_fit(batch: int, n_heads: int, prefix_cap: int) -> bool:
    """`shared_prompt_fits` for vh_attn_decode_shared_groups: the record slots of the prefix CAPACITY + the suffix splits."""
    return _lib.attn_decode_form(_lib.ATTN_ENTRY_SHARED_GROUPS, batch, n_heads, shared_n_split(batch, n_heads), prefix=prefix_cap) is not None


# ---- queued decoding (ValleAR.generate_queued): which utterance holds which slot between which polls -------------------------
def queue_polls(length: int, poll: int, max_new: int) -> int:
    """Polls (blocks of `poll` replayed steps) a slot is held by an utterance that finishes after `length` tokens — the step
    at which its last beam emits EOS, counted from 1 — cut at max_new.  The first token comes from the prompt pass, so a
    slot that has run k blocks has produced 1 + k * poll tokens, and the host sees the utterance done at the first poll
    k >= 1 with 1 + k * poll >= min(length, max_new) (the host looks after every block, so a slot is held for one at least)."""
    n = max(1, min(int(length), int(max_new)))
    return max(1, -(-(n - 1) // int(poll)))


def queue_steps_cap(max_new: int, poll: int) -> int:
    """Steps a row of the queued form may run before the host rewinds or re-arms it: whole polls covering max_new.  The suffix
    cache, the codes rows and the positions are sized for this many plus one."""
    return -(-int(max_new) // int(poll)) * int(poll)


class QueueSchedule:
    """The bookkeeping of queued decoding, pure Python: `slots` slots, utterances handed out in input order.  The first
    min(n, slots) start at poll 0; `retire(slot, poll)` ends the slot's utterance at that poll and starts the next waiting one
    there (returned), or leaves the slot parked (None).  generate_queued drives it from the device's done flags, plan_queue
    from given lengths: the same rules either way."""

    def __init__(self, n_utterances: int, slots: int):
        if slots < 1 or n_utterances < 1:
            raise ValueError(f'QueueSchedule: {n_utterances} utterances on {slots} slots')
        self.n, self.slots = int(n_utterances), int(slots)
        self.holder = [i if i < self.n else None for i in range(self.slots)]      # utterance in each slot (None: parked)
        self.start = {i: 0 for i in range(min(self.n, self.slots))}
        self.slot_of = {i: i for i in range(min(self.n, self.slots))}
        self.end = {}
        self.next = min(self.n, self.slots)
        self.refills = 0

    def retire(self, slot: int, poll: int):
        u = self.holder[slot]
        if u is None:
            raise ValueError(f'QueueSchedule: slot {slot} holds nothing at poll {poll}')
        self.end[u] = int(poll)
        nxt = None
        if self.next < self.n:
            nxt, self.next = self.next, self.next + 1
            self.start[nxt], self.slot_of[nxt] = int(poll), slot
            self.refills += 1
        self.holder[slot] = nxt
        return nxt

    @property
    def finished(self) -> bool:
        return all(h is None for h in self.holder)

    def intervals(self):
        return [(self.slot_of[u], self.start[u], self.end[u]) for u in range(self.n)]


def plan_queue(lengths, slots: int, poll: int, max_new: int):
    """The schedule generate_queued follows for utterances that finish after `lengths` tokens (see queue_polls): returns
    ([(slot, start poll, end poll) per utterance], total decode steps replayed = poll * the latest end).  Done slots are
    served in slot order at every poll, as the decode loop serves them."""
    sched = QueueSchedule(len(lengths), min(int(slots), len(lengths)))
    p = 0
    while not sched.finished:
        for slot in range(sched.slots):
            u = sched.holder[slot]
            if u is not None and p - sched.start[u] >= queue_polls(lengths[u], poll, max_new):
                sched.retire(slot, p)
        if not sched.finished:
            p += 1
    iv = sched.intervals()
    return iv, int(poll) * max(e for _, _, e in iv)


def chunk_schedule_steps(lengths, per: int, poll: int, max_new: int) -> int:
    """Decode steps of the static schedule in the same units (whole polls): consecutive chunks of `per` utterances, each run
    until its longest utterance is done — generate_many's schedule (which cuts its last block at max_new)."""
    return sum(int(poll) * max(queue_polls(n, poll, max_new) for n in lengths[i:i + per]) for i in range(0, len(lengths), per))


def cached_decode_supported(cfg) -> bool:
    """Whether ValleAR.generate_batch decodes `cfg` on the native K/V cache and the hipGraph decoder (pure Python: the
    rule of plan.hip's decoder_check).  Width 64: config.use_kv_cache up to d_model 4096 (above 1024 the step runs the wide
    folded GEMMs where `folded_width(d_model)`, else LayerNorm and the plain GEMMs as separate launches).  Other head widths d_model / n_heads:
    a multiple of 4 from 16 to 256 with d_model % 16 == 0 and d_model <= 1024 (the LayerNorm-fused decode GEMMs);
    anything else recomputes every step."""
    if not cfg.use_kv_cache:
        return False
    d, h = int(cfg.d_model), int(cfg.n_heads)
    if h > 0 and d == h * HEAD_DIM:
        return d <= MAX_DECODE_D_MODEL
    if h <= 0 or d % h:
        return False
    hd = d // h
    return hd % 4 == 0 and 16 <= hd <= 256 and d % 16 == 0 and d <= 1024


def pick_n_split(rows_x_heads: int) -> int:
    """Key-range splits of decode attention so that the grid covers the 256 CUs."""
    if rows_x_heads >= 256:
        return 1
    return max(1, min(16, -(-256 // rows_x_heads)))


_CAPTURE_STREAMS = {}
_CAPTURE_LOCK = threading.Lock()      # one capture at a time on the shared capture stream (host threads with their own streams)


def _capture_stream(device_index):
    """ONE side stream per device for every graph capture of the process (capture enqueues nothing, so decoders can
    share it): a fresh torch.cuda.Stream() per decoder walks through torch's stream pool, and every new stream that
    is used becomes another hardware queue — which also decides where a later stream of another priority lands
    (pipelined attention: the placement of its queue)."""
    st = _CAPTURE_STREAMS.get(device_index)
    if st is None:
        st = _CAPTURE_STREAMS[device_index] = torch.cuda.Stream(device=device_index)
    return st


def _check_row_sampling(rs, batch):
    if rs is not None and (rs.dtype != torch.uint8 or tuple(rs.shape) != (batch, kernels.ROW_SAMPLING_BYTES) or not rs.is_cuda
                           or not rs.is_contiguous()):
        raise _lib.VhError(f'row_sampling must be a contiguous uint8 device tensor ({batch}, {kernels.ROW_SAMPLING_BYTES})')
    return rs


def _check_row_limits(limits, batch, rs):
    if limits is not None and (rs is None or limits.dtype != torch.uint8 or tuple(limits.shape) != (batch, kernels.ROW_LIMITS_BYTES)
                               or not limits.is_cuda or not limits.is_contiguous()):
        raise _lib.VhError(f'row_limits must be a contiguous uint8 device tensor ({batch}, {kernels.ROW_LIMITS_BYTES}) beside '
                           'row_sampling (kernels.pack_row_limits)')
    return limits


class StepSampler:
    """Head + sampling step on the last hidden row of a full forward (valle_ar.py:158-171: logits, top-k / top-p / greedy
    draw, EOS bookkeeping, token append) with the decode state on the device — what ArDecoder.sample_from does, without
    the native decoder behind it: the recompute path of ValleAR.generate_batch (use_kv_cache=False, or a head width the
    decoder is not built for) samples through this."""

    def __init__(self, model, batch, codes, cache_len, audio_pos, pos_base, seed=0, row_sampling=None, row_limits=None):
        """row_sampling: a uint8 device tensor (batch, kernels.ROW_SAMPLING_BYTES) of vh_row_sampling records, or None.  With
        it every row samples from its own record (seed, draw key, filter) and the config's top_k, tok_p, temperature and
        `seed` are not read; the caller owns the tensor and may rewrite it between steps.  row_limits: beside it, a uint8
        device tensor (batch, kernels.ROW_LIMITS_BYTES) of vh_row_limits records (min_new, max_new per row; zeros: no
        bound), read by every sample — the first after a prompt pass included — and rewritten the same way."""
        cfg = model.config
        dev = codes.device
        self.B, self.V, self.d = batch, cfg.num_audio_tokens + 1, cfg.d_model
        self.eos = cfg.num_audio_tokens
        self.logits = torch.zeros(batch, (self.V + 3) // 4 * 4, device=dev, dtype=torch.float32)
        self.x = torch.empty(batch, cfg.d_model, device=dev, dtype=torch.float32)       # the appended token's embedding (unused here)
        self.eos_count = torch.zeros(codes.shape[1] + 1, device=dev, dtype=torch.int32)
        self.sum_logprobs = torch.zeros(batch, device=dev, dtype=torch.float32)
        self.sampling = (int(cfg.top_k), float(cfg.tok_p), float(cfg.temperature), int(seed))
        self.row_sampling = _check_row_sampling(row_sampling, batch)
        self.row_limits = _check_row_limits(row_limits, batch, self.row_sampling)
        self.codes, self.cache_len, self.audio_pos, self.pos_base = codes, cache_len, audio_pos, pos_base
        self._keep = (model.proj.weight.detach(), model.audio_emb.weight.detach(), model.audio_position_emb.pe)
        self.n_split, self.ffn_ws, self.kv_bf16, self.head_ws = 0, None, False, None

    def sample_from(self, hidden_last, rows=slice(None), cache_len=None):
        """Head + first sample on the last hidden rows of a prompt pass (the tail of step 0), for the decode rows `rows`:
        the one Python call site of the sample kernels.  cache_len stands in for the rows' own counter (generate_queued's
        refill: the first sample appends no K/V row, and vh_decode_group_reset left cache_len where the first step appends).
        Without row sampling the sampler keys its draws on the row index within what it is handed; with it, on the rows'
        own records."""
        m = self._keep
        cache_len = self.cache_len[rows] if cache_len is None else cache_len
        kernels.linear(hidden_last, m[0], out=self.logits[rows, : self.V])
        if self.row_sampling is not None:
            kernels.sample_step(self.logits[rows], self.V, self.eos, 0, 1.0, 1.0, 0, self.codes[rows], self.eos_count,
                                self.sum_logprobs[rows], m[1], m[2], self.audio_pos[rows], cache_len, self.x[rows],
                                pos_base=self.pos_base[rows], rs=self.row_sampling[rows],
                                limits=None if self.row_limits is None else self.row_limits[rows])
        elif self.sampling[0] == 1:
            kernels.greedy_step(self.logits[rows], self.V, self.eos, self.codes[rows], self.eos_count, m[1], m[2],
                                self.audio_pos[rows], cache_len, self.x[rows], pos_base=self.pos_base[rows])
        else:
            top_k, top_p, temp, seed = self.sampling
            kernels.sample_step(self.logits[rows], self.V, self.eos, top_k, top_p, temp, seed, self.codes[rows],
                                self.eos_count, self.sum_logprobs[rows], m[1], m[2], self.audio_pos[rows],
                                cache_len, self.x[rows], pos_base=self.pos_base[rows])

    def capture(self):
        pass

    def close(self):
        pass


class ArDecoder(StepSampler):
    """The AR decode loop of valle/models/valle_ar.py:141-171 for B independent rows, one token
    per row per step, the whole step enqueued natively and replayed as a hipGraph.  The head + first sample after a prompt
    pass is StepSampler's (`sample_from`, over the same buffer names)."""

    def __init__(self, model, batch, s_max, codes, cache: KVCache, cache_len, audio_pos, pos_base,
                 n_split=None, use_graph=True, seed=0, prefix: KVCache | None = None, prefix_len=0,
                 prefix_lens=None, prefix_cap=0, beams=1, row_sampling=None, row_limits=None):
        """prefix / prefix_len: SHARED-PROMPT decoding (the beams of ONE utterance, valle_ar.py:135-138): `prefix` is a
        one-row cache holding the prompt's K/V (its first prefix_len rows), `cache` then holds only the generated rows of
        every beam (s_max = its capacity) and cache_len counts those.  A 16-bit `cache` is perf mode; it takes key splits
        (rows x heads below 256) and a 16-bit `prefix` — the two caches must have the same dtype.

        prefix_lens / prefix_cap / beams: GROUPED shared prompts (several utterances, each replicated over `beams` rows):
        `prefix` is then a G-row cache, G = batch // beams, prefix_lens the int32 device tensor (G) of the prompts' lengths
        — read by every step, so the caller rewrites it between calls — and prefix_cap (<= prefix.s_max) bounds them.  fp32
        caches only; prefix_len is not used.

        row_sampling: as StepSampler's; the captured steps read the records through the pointer, so rewriting the tensor
        between replays re-keys the rows.  row_limits: as StepSampler's, attached to the native decoder before any capture
        (vh_ar_decoder_set_row_limits) and read through the pointer the same way."""
        cfg = model.config
        dev = cache.buf.device
        d, dff, V = cfg.d_model, cfg.dim_feedforward, cfg.num_audio_tokens + 1
        self.B, self.V, self.d, self.eos = batch, V, d, cfg.num_audio_tokens
        self.ldl = (V + 3) // 4 * 4
        self.n_split = n_split or pick_n_split(batch * cfg.n_heads)
        if prefix is not None and n_split is None:
            # shared prompt: the beams' own rows are short streams — two workgroups per CU keep twice the loads in flight
            # (32 beams x 8 heads: 436.8 us per step with one split, 420.9 with two, 426.9 with four — fp32 caches; a 16-bit
            # cache takes the same split counts here and in pick_n_split, which nobody has tuned for the half-width streams)
            self.n_split = shared_n_split(batch, cfg.n_heads)
        f32 = dict(device=dev, dtype=torch.float32)
        self.x = torch.empty(batch, d, **f32)
        self.q = torch.empty(batch, d, **f32)
        self.attn = torch.empty(batch, d, **f32)
        self.hidden = torch.empty(batch, dff, **f32)
        self.logits = torch.zeros(batch, self.ldl, **f32)
        self.prefix, self.prefix_len = prefix, int(prefix_len)
        self.prefix_lens, self.prefix_cap, self.beams = prefix_lens, int(prefix_cap), int(beams)
        self.grouped = prefix_lens is not None
        self.head_dim = hd = d // cfg.n_heads
        if hd != HEAD_DIM:
            # a head width other than 64: vh_attn_decode_hd over an fp32 cache of that width; no shared prompt, no bf16 cache
            if prefix is not None or cache.bf16 or cache.head_dim != hd:
                raise _lib.VhError(f'head width {hd}: the cached decoder takes an fp32 cache of that width, no shared prompt '
                                   'and no bf16 (perf-mode) cache')
            n = _lib.lib().vh_attn_decode_hd_ws_bytes(batch, cfg.n_heads, hd, self.n_split)
            self.partial = torch.empty(max(n, 16) // 4, **f32) if n else None
        elif self.grouped:
            if prefix is None or prefix.bf16 or cache.bf16:
                raise _lib.VhError('grouped shared prompts: fp32 prefix and row caches (no perf mode)')
            if self.beams < 1 or batch % self.beams or prefix.batch * self.beams != batch or prefix.n_layers != cfg.num_layers or \
                    not 0 < self.prefix_cap <= prefix.s_max:
                raise _lib.VhError(f'grouped shared prompts: {batch} rows = {prefix.batch} prefix rows x beams={self.beams}, '
                                   f'capacity {self.prefix_cap} of {prefix.s_max}')
            if prefix_lens.dtype != torch.int32 or prefix_lens.numel() != prefix.batch or not prefix_lens.is_cuda:
                raise _lib.VhError('grouped shared prompts: prefix_lens must be an int32 device tensor, one entry per group')
            self.prefix_len = 0
            self.partial = kernels.attn_decode_shared_groups_ws(batch, cfg.n_heads, self.prefix_cap, self.n_split, dev)
        elif prefix is not None:
            if prefix.bf16 != cache.bf16:
                raise _lib.VhError(f'shared-prompt decoding: the prefix cache ({prefix.buf.dtype}) and the beams\' cache '
                                   f'({cache.buf.dtype}) must have the same dtype')
            if prefix.batch != 1 or prefix.n_layers != cfg.num_layers or not 0 < prefix_len <= prefix.s_max:
                raise _lib.VhError('shared-prompt decoding: a one-row prefix cache holding prefix_len rows')
            self.partial = kernels.attn_decode_shared_ws(batch, cfg.n_heads, self.prefix_len, self.n_split, dev)
        else:
            self.partial = kernels.attn_decode_ws(batch, cfg.n_heads, self.n_split, dev)
        ws_bytes = _lib.lib().vh_linear_ws_bytes(batch, d, dff)
        self.gemm_ws = torch.empty(max(ws_bytes, 16) // 4, **f32) if ws_bytes else None
        self.eos_count = torch.zeros(codes.shape[1] + 1, device=dev, dtype=torch.int32)
        self.sum_logprobs = torch.zeros(batch, **f32)
        self.sampling = (int(cfg.top_k), float(cfg.tok_p), float(cfg.temperature), int(seed))
        # the sampling seed lives in device memory (desc.seed = 0 + *seed_dev): a captured graph would freeze a by-value
        # seed, and this decoder may serve many generate() calls (`reset`)
        self.row_sampling = _check_row_sampling(row_sampling, batch)
        self.row_limits = _check_row_limits(row_limits, batch, self.row_sampling)
        self.seed_dev = torch.tensor([int(seed)], dtype=torch.int64).to(dev) if self.sampling[0] != 1 and row_sampling is None else None
        self.codes, self.cache, self.cache_len, self.audio_pos = codes, cache, cache_len, audio_pos
        self.pos_base = pos_base
        # (above 1024 the folded GEMMs are one-row-tile kernels: more than 16 rows run as row groups that each stream the
        # weights, and measured slower than LayerNorm + the plain GEMMs there — profiles/r7_wide_d_model.log)
        wide_unfolded = d > 1024 and batch > WIDE_FOLD_MAX_ROWS
        # (640 / 768 / 896 are folded at head width 64 only: vh_linear_qkv_folded_hd has no form there, other widths keep the fused-LayerNorm GEMMs)
        wide_unfolded = wide_unfolded or (hd != HEAD_DIM and d in BASE_FOLD_WIDTHS)
        self._folded = None if wide_unfolded else folded_layer_norms(model.transformer)   # kept alive: the table holds raw pointers
        self.ln_folded = self._folded is not None          # False above 1024: LayerNorm + plain GEMMs as separate launches
        self.kv_bf16 = cache.bf16
        if self.kv_bf16 and self._folded is None:
            raise _lib.VhError('perf mode (16-bit K/V cache) needs the folded LayerNorm weights')
        if self.kv_bf16 and not 1 <= self.n_split <= 16:
            raise _lib.VhError(f'perf mode (16-bit K/V cache) serves n_split 1..16 (got {self.n_split})')
        # FeedForward of a layer as one launch split over dim_feedforward + the slab reduce (vh_ffn_decode)
        # (d_model <= 1024: vh_ffn_decode's shape set; the plan takes it at d_model <= 512)
        ffn_bytes = _lib.lib().vh_ffn_decode_ws_bytes(batch, d, dff) if self._folded is not None and d <= 1024 else 0
        self.ffn_ws = torch.empty(ffn_bytes // 4, **f32) if ffn_bytes else None
        # opt-in (VALLE2_HEAD_FUSED=1): head + greedy step as one launch (vh_head_greedy; DESIGN.md 3.20 has the A/B)
        self.head_ws = None
        if os.environ.get('VALLE2_HEAD_FUSED') == '1' and self.sampling[0] == 1 and row_sampling is None and head_fused_shape(batch, V, d):
            self.head_ws = kernels.head_greedy_ws(batch, V, dev)
        self._table = layer_table(model.transformer, cache, self._folded)
        # perf mode, second half: the step's four matrices (and the head) as h16 — half the weight bytes per launch
        self._w16 = self._proj16 = None
        if self.kv_bf16 and DECODE_W16 and self.ffn_ws is not None and w16_width(d) and cfg.dim_feedforward % 16 == 0:
            self._w16 = decode_weights16(model.transformer, self._folded)
            for i, (wq, wo, w1, w2, c1q, c1w) in enumerate(self._w16):
                self._table[i].wqkv_f16, self._table[i].wo16 = ptr(wq), ptr(wo)
                self._table[i].w1_f16, self._table[i].w2_16 = ptr(w1), ptr(w2)
                self._table[i].qkv_c1, self._table[i].w1_c1 = ptr(c1q), ptr(c1w)     # (this decoder's table: the sums of the h16 matrices)
            with torch.inference_mode(False):
                self._proj16 = kernels.to_bf16(model.proj.weight.detach()) if d % 8 == 0 else None
        self.w16 = self._w16 is not None
        if prefix is not None:
            for i in range(cfg.num_layers):
                self._table[i].kprefix, self._table[i].vprefix = ptr(prefix.k(i)), ptr(prefix.v(i))
        self._keep = (model.proj.weight.detach(), model.audio_emb.weight.detach(),
                      model.audio_position_emb.pe)
        desc = VhArDecoderDesc(
            B=batch, d_model=d, n_heads=cfg.n_heads, dff=dff, n_layers=cfg.num_layers, S_max=s_max,
            V=V, eos=cfg.num_audio_tokens, n_split=self.n_split, ln_eps=1e-5, layers=self._table,
            proj_w=ptr(self._keep[0]), audio_emb=ptr(self._keep[1]), audio_pe=ptr(self._keep[2]),
            x=ptr(self.x), q=ptr(self.q), attn=ptr(self.attn), hidden=ptr(self.hidden),
            logits=ptr(self.logits), attn_partial=ptr(self.partial), gemm_ws=ptr(self.gemm_ws),
            gemm_ws_bytes=ws_bytes, cache_len=ptr(cache_len),
            audio_pos=ptr(audio_pos), eos_count=ptr(self.eos_count), pos_base=ptr(pos_base),
            codes=ptr(codes), codes_stride=codes.stride(0), top_k=self.sampling[0], top_p=self.sampling[1],
            temperature=self.sampling[2], seed=0 if self.seed_dev is not None else self.sampling[3] & (2 ** 64 - 1),
            seed_dev=ptr(self.seed_dev), proj_w16=ptr(self._proj16),
            sum_logprobs=ptr(self.sum_logprobs), ffn_ws=ptr(self.ffn_ws), ffn_ws_bytes=ffn_bytes,
            kv_bf16=int(self.kv_bf16), prefix_len=self.prefix_len if prefix is not None else 0,
            prefix_S=prefix.s_max if prefix is not None else 0,
            n_groups=prefix.batch if self.grouped else 0, beams_per_group=self.beams if self.grouped else 0,
            prefix_cap=self.prefix_cap if self.grouped else 0, prefix_lens=ptr(prefix_lens) if self.grouped else None,
            attn_partial_bytes=self.partial.numel() * 4 if self.partial is not None else 0,
            head_ws=ptr(self.head_ws), head_ws_bytes=self.head_ws.numel() * 4 if self.head_ws is not None else 0,
            row_sampling=ptr(self.row_sampling))
        self._desc = desc
        self._h = _lib.lib().vh_ar_decoder_create(C.byref(desc))
        if not self._h:
            msg = _lib.lib().vh_last_error()
            raise _lib.VhError(f'vh_ar_decoder_create: {msg.decode() if msg else "failed"}')
        if self.row_limits is not None:
            check(_lib.lib().vh_ar_decoder_set_row_limits(self._h, ptr(self.row_limits)), 'vh_ar_decoder_set_row_limits')
        self._captured = False
        self.use_graph = use_graph

    def close(self):
        if getattr(self, '_h', None) and _lib is not None:     # (a decoder kept in a slot may outlive the module at interpreter exit)
            _lib.lib().vh_ar_decoder_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self, seed=0):
        """Ready for another generate() over the SAME buffers (codes, caches, cache_len, audio_pos, pos_base are the
        caller's to refill): counters and scores cleared, the new call's seed written where the captured steps read it."""
        self.eos_count.zero_()
        self.sum_logprobs.zero_()
        self.sampling = self.sampling[:3] + (int(seed),)
        if self.seed_dev is not None:
            self.seed_dev.copy_(torch.tensor([int(seed)], dtype=torch.int64), non_blocking=True)

    def capture(self):
        """Record the step graphs now (host work only: capture enqueues nothing).  generate_batch calls it right after
        the prompt pass is enqueued, so the ~1.7 ms of capture + instantiate run on the host while the GPU is busy."""
        if self.use_graph and not self._captured:
            with _CAPTURE_LOCK:
                cap = _capture_stream(torch.cuda.current_device())
                check(_lib.lib().vh_ar_decoder_capture(self._h, cap.cuda_stream), 'vh_ar_decoder_capture')
            self._captured = True

    def run(self, n_steps):
        """Enqueue n_steps decode steps on the current stream (graph replay when enabled)."""
        if n_steps <= 0:
            return
        s = stream()
        L = _lib.lib()
        if self.use_graph:
            self.capture()
            check(L.vh_ar_decoder_replay(self._h, n_steps, s), 'vh_ar_decoder_replay')
        else:
            for _ in range(n_steps):
                check(L.vh_ar_decoder_step(self._h, s), 'vh_ar_decoder_step')

    def profile_attn(self, n_steps):
        """(bracket_ms, floor_ms, kernel_ms) over n_steps eager steps: mean event-to-event time of marker events
        around the decode-attention launches, the same bracket with nothing inside, and the mean time between the
        start/stop events attached to the kernel dispatch itself (advances the decode state by n_steps)."""
        ms, floor, kern = C.c_float(0), C.c_float(0), C.c_float(0)
        check(_lib.lib().vh_ar_decoder_profile_attn(self._h, n_steps, stream(), C.byref(ms), C.byref(floor),
                                                    C.byref(kern)), 'vh_ar_decoder_profile_attn')
        return ms.value, floor.value, kern.value
