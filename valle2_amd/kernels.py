"""Tensor-level wrappers of the C-ABI primitives (include/valle_hip.h).

Each function checks shapes on the host (a kernel that faults can reset every GPU of the box),
passes raw device pointers + the current torch HIP stream, and raises on a non-zero status.
Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import check, ptr, stream

MASK_FULL, MASK_PREFIX, MASK_EXPLICIT = 0, 1, 2
H16 = _lib.h16_dtype()      # the 16-bit operand format of perf mode (float16 by default; the *_bf16 names are round 5's)
ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_GELU_D, ACT_MUL = 0, 1, 2, 3, 4
HEAD_DIM = 64
MAX_TABLES = 32           # VH_MAX_TABLES: codebooks one vh_embed_sum_pe sums (EnCodec at 24 kbps)
SAMPLE_NARROW_V = 2048    # widest row vh_sample_step takes; wider rows go to vh_sample_step_wide
SAMPLE_MAX_V = 16384      # VH_SAMPLE_MAX_V: widest row vh_sample_step_wide takes (num_audio_tokens <= 16383)


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise _lib.VhError(f'{name} must be float32, got {t.dtype}')
    return t


def _drop_ref(drop):
    return None if drop is None else C.byref(drop)


def embed_sum_pe(ids, tables, pe, pos0, out, out_t0=0, lens=None, row_pos0=None, row_t0=None, max_pos=None, drop=None):
    """out[b, out_t0+t] = sum_j tables[j][ids[b,t,j]] + pe[pos0+t].  ids (B,T) or (B,T,J) int64
    (any strides); tables: list of (vocab,d); pe (P,1,d)|(P,d)|None; out (B,T_out,d).
    lens / row_pos0 / row_t0: device int32 (B) — valid ids per row and per-row overrides of pos0 / out_t0 (a ragged
    batch in one launch); with them the caller vouches, through `max_pos` (largest position + 1 any row reaches) and
    its own layout, that positions stay inside the table and rows inside `out`.
    out (rows, d) with row_t0: the PACKED form — row t of batch row b goes to out[row_t0[b] + t], no batch stride (the
    rows of a ragged batch back to back in one buffer).
    drop: a dropout.spec — the dropout after the position add (modules.py:80), field row = the row's index in `out`."""
    if ids.dtype != torch.int64:
        raise _lib.VhError('ids must be int64')
    if ids.dim() == 2:
        ids = ids.unsqueeze(-1)
    B, T, J = ids.shape
    n = len(tables)
    if n > MAX_TABLES:
        raise _lib.VhError(f'embed_sum_pe: {n} codebook tables; at most {MAX_TABLES} are summed (VH_MAX_TABLES)')
    if n > J and J != 1:
        raise _lib.VhError(f'{n} tables but ids has {J} codebooks')
    d = tables[0].shape[1]
    packed = out.dim() == 2 and row_t0 is not None
    if packed:
        if out.shape[1] != d or not out.is_contiguous():
            raise _lib.VhError(f'packed out {tuple(out.shape)} must be contiguous (rows, {d})')
    elif out.dim() != 3 or out.shape[0] != B or out.shape[2] != d or (row_t0 is None and out_t0 + T > out.shape[1]):
        raise _lib.VhError(f'out shape {tuple(out.shape)} does not fit B={B} T={T} d={d} t0={out_t0}')
    if row_pos0 is not None or row_t0 is not None:
        for t_ in (row_pos0, row_t0, lens):
            if t_ is not None and (t_.dtype != torch.int32 or t_.numel() != B or not t_.is_cuda):
                raise _lib.VhError('embed_sum_pe: lens / row_pos0 / row_t0 must be device int32 tensors of B entries')
        if lens is None or max_pos is None:
            raise _lib.VhError('embed_sum_pe: per-row offsets need `lens` and `max_pos`')
        if pe is not None and max_pos > pe.shape[0]:
            raise _lib.VhError(f'position {max_pos} exceeds the table ({pe.shape[0]})')
    elif pe is not None and pos0 + T > pe.shape[0]:
        raise _lib.VhError(f'position {pos0 + T} exceeds the table ({pe.shape[0]})')
    if not ids.is_cuda:
        raise _lib.VhError('embed_sum_pe: ids must be on the HIP device')
    if any(t.dim() != 2 or t.shape[1] != d for t in tables):
        raise _lib.VhError('embed_sum_pe: every table must be (vocab, d)')
    arr = (C.c_void_p * n)(*[ptr(_f32(t, 'table')) for t in tables])
    vocab = (C.c_int32 * n)(*[int(t.shape[0]) for t in tables])    # ids are range-checked in the kernel
    check(_lib.lib().vh_embed_sum_pe(
        ids.data_ptr(), ids.stride(0), ids.stride(1), ids.stride(2), arr, vocab, n,
        ptr(_f32(pe, 'pe')), pos0, ptr(lens), ptr(_f32(out, 'out')), 0 if packed else out.stride(0), out_t0,
        B, T, d, ptr(_lib.err_flag(out.device)), ptr(row_pos0), ptr(row_t0), _drop_ref(drop), stream()),
        'vh_embed_sum_pe')
    return out


def _nar_packed_args(what, tokens, codes, text_table, code_tables, n_rest, layout, rows):
    """The host checks the two packed NAR input launches share; returns the argument run both entry points start with up to
    the segment tables (the tables / gradient tables go in between)."""
    n_full = len(code_tables)
    if not 1 <= n_rest <= n_full <= MAX_TABLES:
        raise _lib.VhError(f'{what}: n_rest={n_rest}, n_full={n_full}: need 1 <= n_rest <= n_full <= {MAX_TABLES} (VH_MAX_TABLES)')
    if tokens.dtype != torch.int64 or codes.dtype != torch.int64 or not tokens.is_cuda or not codes.is_cuda:
        raise _lib.VhError(f'{what}: tokens / codes must be int64 tensors on the HIP device')
    B = layout.n_seg
    if tokens.dim() != 2 or codes.dim() != 3 or tokens.shape[0] != B or codes.shape[0] != B or tokens.stride(1) != 1:
        raise _lib.VhError(f'{what}: tokens {tuple(tokens.shape)} / codes {tuple(codes.shape)} for {B} segments')
    if layout.max_x_len > tokens.shape[1] or layout.max_a_len > codes.shape[1] or n_full > codes.shape[2]:
        raise _lib.VhError(f'{what}: streams of up to {layout.max_x_len} text ids and {layout.max_a_len} frames of {n_full} '
                           f'codebooks do not fit tokens {tuple(tokens.shape)} / codes {tuple(codes.shape)}')
    d = text_table.shape[1]
    if tuple(rows.shape) != (layout.rows, d) or not rows.is_contiguous():
        raise _lib.VhError(f'{what}: packed rows {tuple(rows.shape)} must be contiguous ({layout.rows}, {d})')
    if any(t is not None and (t.dim() != 2 or t.shape[1] != d) for t in code_tables):
        raise _lib.VhError(f'{what}: every table must be (vocab, {d})')
    for t_ in (layout.seg_start, layout.x_len, layout.a_len, layout.prefix):
        if t_.dtype != torch.int32 or t_.numel() != B or not t_.is_cuda:
            raise _lib.VhError(f'{what}: seg_start / x_len / a_len / prefix must be device int32 tensors of {B} entries')
    return d, (tokens.data_ptr(), tokens.stride(0), codes.data_ptr(), codes.stride(0), codes.stride(1), codes.stride(2))


def embed_nar_packed(tokens, codes, text_table, code_tables, n_rest, pe_text, pe_audio, layout, out, drop_text=None,
                     drop_audio=None):
    """The model input of packed NAR training in ONE launch (vh_embed_nar_packed).  `layout` (an engine.NarTrainLayout):
    segment s of out (M, d) starts at layout.seg_start[s] and holds x_len[s] text rows — text_table[tokens[s, i]] +
    pe_text[i] — then a_len[s] audio rows — sum_{j < n(t)} code_tables[j][codes[s, t, j]] + pe_audio[t] with n(t) =
    len(code_tables) for t < prefix[s] and n_rest after.  Every row is bit for bit `embed_sum_pe`'s for that utterance alone
    at the same rows of out; drop_text / drop_audio: the two PositionalEncoding dropout specs, fields keyed on the packed row."""
    d, ids = _nar_packed_args('embed_nar_packed', tokens, codes, text_table, code_tables, n_rest, layout, out)
    n = len(code_tables)
    arr = (C.c_void_p * n)(*[ptr(_f32(t, 'table')) for t in code_tables])
    vocab = (C.c_int32 * n)(*[int(t.shape[0]) for t in code_tables])
    check(_lib.lib().vh_embed_nar_packed(
        *ids, ptr(_f32(text_table, 'text table')), int(text_table.shape[0]), arr, vocab, n, n_rest,
        ptr(_f32(pe_text, 'pe')), int(pe_text.shape[0]), ptr(_f32(pe_audio, 'pe')), int(pe_audio.shape[0]),
        ptr(layout.seg_start), ptr(layout.x_len), ptr(layout.a_len), ptr(layout.prefix), layout.n_seg, layout.max_x_len,
        layout.max_a_len, ptr(_f32(out, 'out')), layout.rows, d, ptr(_lib.err_flag(out.device)), _drop_ref(drop_text),
        _drop_ref(drop_audio), stream()), 'vh_embed_nar_packed')
    return out


def embed_nar_packed_bwd(tokens, codes, dout, dtext_table, dcode_tables, text_vocab, code_vocab, n_rest, pe_text_rows,
                         pe_audio_rows, layout, drop_text=None, drop_audio=None):
    """The backward of `embed_nar_packed` in ONE launch (vh_embed_nar_packed_bwd): dout (M, d), multiplied by the regenerated
    fields, is ADDED into dtext_table (text_vocab, d) and dcode_tables[j] (code_vocab[j], d) — fp32, zeroed or holding what
    the sums should start from; None: skipped — at the rows the ids name, each gradient row read once for all its tables.
    fp32 atomics, no promise of order."""
    n = len(dcode_tables)
    if len(code_vocab) != n:
        raise _lib.VhError(f'embed_nar_packed_bwd: {n} gradient tables, {len(code_vocab)} row counts')
    for t, v in zip([dtext_table, *dcode_tables], [text_vocab, *code_vocab]):
        if t is not None and (t.dim() != 2 or t.shape[0] != v or not t.is_contiguous()):
            raise _lib.VhError(f'embed_nar_packed_bwd: a gradient table {tuple(t.shape)} for {v} rows')
    d, ids = _nar_packed_args('embed_nar_packed_bwd', tokens, codes, dout, dcode_tables, n_rest, layout, dout)
    arr = (C.c_void_p * n)(*[None if t is None else ptr(_f32(t, 'table gradient')) for t in dcode_tables])
    vocab = (C.c_int32 * n)(*[int(v) for v in code_vocab])
    check(_lib.lib().vh_embed_nar_packed_bwd(
        *ids, ptr(_f32(dout, 'dout')), None if dtext_table is None else ptr(_f32(dtext_table, 'table gradient')),
        int(text_vocab), arr, vocab, n, n_rest, int(pe_text_rows), int(pe_audio_rows), ptr(layout.seg_start),
        ptr(layout.x_len), ptr(layout.a_len), ptr(layout.prefix), layout.n_seg, layout.max_x_len, layout.max_a_len, layout.rows,
        d, ptr(_lib.err_flag(dout.device)), _drop_ref(drop_text), _drop_ref(drop_audio), stream()), 'vh_embed_nar_packed_bwd')


def ids_to_device(ids, device, vocab, what):
    """Token ids → `device`.  Ids still on the host are range-checked here, before they travel (the
    reference's nn.Embedding raises IndexError); device-resident ids are checked by the kernels
    (`_lib.raise_device_errors`)."""
    if not ids.is_cuda and ids.numel():
        # numpy on the tensor's own memory, not torch's CPU reductions: those fan a 70 k-element min / max out over
        # every core `os.cpu_count()` reports (256 on a GPU box whose cgroup grants 16) and then cost 2-70 ms per
        # call, erratically — the NAR training step with host-resident batches ran at 40-60 ms instead of 28
        # (gpurun_out/nar_host.log, round 4); numpy's single-threaded pass over the same bytes takes ~30 us
        a = ids.detach().numpy()
        lo, hi = int(a.min()), int(a.max())
        if lo < 0 or hi >= vocab:
            raise IndexError(f'{what}: id {lo if lo < 0 else hi} is outside [0, {vocab}) (index out of range)')
    return _lib.to_device_async(ids, device)


def _dev_f32(t, name):
    """data_ptr of a row-major fp32 DEVICE tensor (a host pointer handed to a kernel is a fault)."""
    if not t.is_cuda:
        raise _lib.VhError(f'{name} is on {t.device}: kernels take HIP device tensors only')
    return _f32(t, name).data_ptr()


def add_pe(x, pe, pos0=0):
    """x (B, T, d) + pe[pos0 : pos0 + T] (pe (P, 1, d) or (P, d)) -> new tensor: PositionalEncoding.forward as a module call."""
    B, T, d = x.shape
    if pos0 + T > pe.shape[0] or pe.shape[-1] != d:
        raise _lib.VhError(f'add_pe: positions {pos0}..{pos0 + T} / width {d} outside the table {tuple(pe.shape)}')
    x = x.contiguous()
    out = torch.empty_like(x)
    check(_lib.lib().vh_add_pe(_dev_f32(x, 'x'), ptr(_f32(pe, 'pe')), ptr(out), B, T, d, pos0, stream()), 'vh_add_pe')
    return out


def layernorm(x, gamma, beta, out=None, ada_scale=None, ada_shift=None, eps=1e-5):
    d = x.shape[-1]
    rows = x.numel() // d
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().vh_layernorm(ptr(_f32(x, 'x')), ptr(gamma), ptr(beta), ptr(ada_scale),
                                  ptr(ada_shift), ptr(out), rows, d, eps, stream()), 'vh_layernorm')
    return out


def _ln_args(ln):
    if ln is None:
        return None, None, None, None, 0.0
    g, b, sc, sh, eps = ln
    return ptr(g), ptr(b), ptr(sc), ptr(sh), float(eps)


def linear(a, w, bias=None, residual=None, out=None, act=ACT_NONE, ln=None):
    """out = act(LN?(a) @ w.T + bias) + residual.  a (M,K) (row stride lda), w (N,K)."""
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VhError(f'linear: K mismatch {K} vs {K2}')
    if a.stride(1) != 1 or not w.is_contiguous():
        raise _lib.VhError('linear: operands must be row-major')
    if out is None:
        ldo = (N + 3) // 4 * 4
        out = torch.empty(M, ldo, device=a.device, dtype=torch.float32)[:, :N]
    if out.stride(1) != 1 or (residual is not None and residual.stride(1) != 1):
        raise _lib.VhError('linear: out/residual must be row-major')
    if bias is not None and bias.numel() != N:
        raise _lib.VhError('linear: bias size')
    if residual is not None and tuple(residual.shape) != (M, N):
        raise _lib.VhError('linear: residual shape')
    g, b, sc, sh, eps = _ln_args(ln)
    check(_lib.lib().vh_linear(
        _dev_f32(a, 'a'), a.stride(0), ptr(_f32(w, 'w')), ptr(bias),
        _dev_f32(residual, 'residual') if residual is not None else None,
        residual.stride(0) if residual is not None else 0,
        _dev_f32(out, 'out'), out.stride(0), M, N, K, act, g, b, sc, sh, eps, stream()),
        'vh_linear')
    return out


def linear_ws(a, w, bias=None, residual=None, out=None, act=ACT_NONE, workspace=None):
    """vh_linear_ws: split-K path for wide K (see include/valle_hip.h)."""
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VhError(f'linear_ws: K mismatch {K} vs {K2}')
    if a.stride(1) != 1 or not w.is_contiguous():
        raise _lib.VhError('linear_ws: operands must be row-major')
    if out is None:
        out = torch.empty(M, (N + 3) // 4 * 4, device=a.device, dtype=torch.float32)[:, :N]
    if tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise _lib.VhError(f'linear_ws: out must be a row-major ({M},{N}) tensor')
    if bias is not None and bias.numel() != N:
        raise _lib.VhError('linear_ws: bias size')
    if residual is not None and (tuple(residual.shape) != (M, N) or residual.stride(1) != 1):
        raise _lib.VhError('linear_ws: residual shape')
    need = _lib.lib().vh_linear_ws_bytes(M, N, K)
    if workspace is None and need:
        workspace = torch.empty(need // 4, device=a.device, dtype=torch.float32)
    if need and workspace.numel() * 4 < need:
        raise _lib.VhError(f'linear_ws: workspace of {workspace.numel() * 4} B < {need} B')
    check(_lib.lib().vh_linear_ws(
        _dev_f32(a, 'a'), a.stride(0), ptr(_f32(w, 'w')), ptr(bias),
        _dev_f32(residual, 'residual') if residual is not None else None,
        residual.stride(0) if residual is not None else 0,
        _dev_f32(out, 'out'), out.stride(0), M, N, K, act, ptr(workspace),
        workspace.numel() * 4 if workspace is not None else 0, stream()), 'vh_linear_ws')
    return out


def linear_qkv(a, wqkv, q_out, kcache, vcache, B, T, n_heads, cache_len=None, ln=None):
    """QKV projection; Q → q_out (B*T, d); K,V rows appended to the caches (B,h,S_max,64)."""
    M, d = a.shape
    if M != B * T or tuple(wqkv.shape) != (3 * d, d) or d != n_heads * HEAD_DIM:
        raise _lib.VhError(f'linear_qkv: shapes a={tuple(a.shape)} w={tuple(wqkv.shape)} B={B} T={T}')
    S_max = kcache.shape[2]
    if tuple(kcache.shape) != (B, n_heads, S_max, HEAD_DIM) or kcache.shape != vcache.shape:
        raise _lib.VhError(f'linear_qkv: cache shape {tuple(kcache.shape)}')
    if cache_len is None and T > S_max:
        raise _lib.VhError('linear_qkv: T > S_max')
    g, b, sc, sh, eps = _ln_args(ln)
    check(_lib.lib().vh_linear_qkv(
        _f32(a, 'a').data_ptr(), a.stride(0), ptr(wqkv), q_out.data_ptr(), q_out.stride(0),
        ptr(kcache), ptr(vcache), ptr(cache_len), B, T, d, n_heads, S_max, g, b, sc, sh, eps,
        stream()), 'vh_linear_qkv')
    return q_out


def ln_fold(w, gamma, beta, bias=None):
    """(Wf, c1, c2) of vh_ln_fold: LN(x) @ w.T + bias == rstd * (x @ Wf.T - mean * c1) + c2."""
    N, K = w.shape
    if not w.is_contiguous() or gamma.numel() != K or beta.numel() != K:
        raise _lib.VhError(f'ln_fold: w={tuple(w.shape)} gamma={tuple(gamma.shape)}')
    wf = torch.empty_like(w)
    c = torch.empty(2, (N + 3) // 4 * 4, device=w.device, dtype=torch.float32)
    check(_lib.lib().vh_ln_fold(_f32(w, 'w').data_ptr(), ptr(gamma), ptr(beta), ptr(bias), ptr(wf),
                                c[0].data_ptr(), c[1].data_ptr(), N, K, stream()), 'vh_ln_fold')
    return wf, c[0, :N], c[1, :N]


def linear_folded(a, folded, residual=None, out=None, act=ACT_NONE, eps=1e-5):
    """act(LN(a) @ w.T + bias) + residual from the folded triple of ln_fold (decode rows, M <= 64)."""
    wf, c1, c2 = folded
    M, K = a.shape
    N = wf.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    check(_lib.lib().vh_linear_folded(
        _f32(a, 'a').data_ptr(), a.stride(0), ptr(wf), ptr(c1), ptr(c2), ptr(residual),
        residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), M, N, K, act,
        eps, stream()), 'vh_linear_folded')
    return out


def linear_qkv_folded(a, folded, q_out, kcache, vcache, B, T, n_heads, cache_len=None, eps=1e-5):
    wf, c1, c2 = folded
    M, d = a.shape
    S_max = kcache.shape[2]
    if M != B * T or tuple(wf.shape) != (3 * d, d) or tuple(kcache.shape) != (B, n_heads, S_max, HEAD_DIM):
        raise _lib.VhError(f'linear_qkv_folded: shapes a={tuple(a.shape)} w={tuple(wf.shape)}')
    check(_lib.lib().vh_linear_qkv_folded(
        _dev_f32(a, 'a'), a.stride(0), ptr(wf), ptr(c1), ptr(c2),
        q_out.data_ptr(), q_out.stride(0), ptr(kcache), ptr(vcache), ptr(cache_len), B, T, d, n_heads, S_max,
        eps, stream()), 'vh_linear_qkv_folded')
    return q_out


def ffn_decode_ws(M, d, dff, device):
    n = _lib.lib().vh_ffn_decode_ws_bytes(M, d, dff)
    return torch.empty(max(n, 16) // 4, device=device, dtype=torch.float32) if n else None


def ffn_decode(x, folded, w2, b2=None, out=None, workspace=None, eps=1e-5):
    """out = x + b2 + GELU(LN2(x) @ W1.T + b1) @ w2.T for M <= 64 decode rows (vh_ffn_decode); `folded` =
    ln_fold(W1, ln2_gamma, ln2_beta, b1).  out may be x itself."""
    wf, c1, c2 = folded
    M, d = x.shape
    dff = wf.shape[0]
    if tuple(wf.shape) != (dff, d) or tuple(w2.shape) != (d, dff) or not w2.is_contiguous() or not wf.is_contiguous():
        raise _lib.VhError(f'ffn_decode: x {tuple(x.shape)} w1f {tuple(wf.shape)} w2 {tuple(w2.shape)}')
    if c1.numel() != dff or c2.numel() != dff or (b2 is not None and b2.numel() != d):
        raise _lib.VhError('ffn_decode: c1 / c2 / b2 sizes')
    if out is None:
        out = torch.empty(M, d, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (M, d) or out.stride(1) != 1 or x.stride(1) != 1:
        raise _lib.VhError('ffn_decode: x / out must be row-major (M, d)')
    if workspace is None:
        workspace = ffn_decode_ws(M, d, dff, x.device)
    if workspace is None:
        raise _lib.VhError(f'ffn_decode: unsupported shape M={M} d={d} dff={dff}')
    check(_lib.lib().vh_ffn_decode(
        _dev_f32(x, 'x'), x.stride(0), ptr(_f32(wf, 'w1f')), ptr(c1), ptr(c2), ptr(_f32(w2, 'w2')), ptr(b2),
        _dev_f32(out, 'out'), out.stride(0), M, d, dff, eps, ptr(workspace), workspace.numel() * 4, stream()),
        'vh_ffn_decode')
    return out


def attn_rows(q, kcache, vcache, out, B, n_heads, Tq, Tk, mode, x_len=0, x_len_dev=None,
              kv_len=None, mask=None, pad=None, lse2=None):
    S_max = kcache.shape[2]
    if tuple(kcache.shape) != (B, n_heads, S_max, HEAD_DIM) or Tk > S_max or Tq > Tk:
        raise _lib.VhError(f'attn_rows: cache {tuple(kcache.shape)} Tq={Tq} Tk={Tk}')
    if q.shape[0] != B * Tq or out.shape[0] != B * Tq:
        raise _lib.VhError('attn_rows: q/out rows')
    if mask is not None and mask.dim() == 3:       # one mask per batch row (inference only: no lse2)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, Tq, Tk) or not mask.is_contiguous() or lse2 is not None:
            raise _lib.VhError('attn_rows: a per-row mask must be contiguous uint8 (B,Tq,Tk); the training forward takes 2-D masks')
        if pad is not None and (pad.dtype != torch.uint8 or tuple(pad.shape) != (B, Tk)):
            raise _lib.VhError('attn_rows: pad must be uint8 (B,Tk)')
        check(_lib.lib().vh_attn_rows_bmask(
            _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), B, n_heads, Tq, Tk,
            S_max, ptr(mask), Tq * Tk, ptr(pad), stream()), 'vh_attn_rows_bmask')
        return out
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (Tq, Tk)):
        raise _lib.VhError('attn_rows: mask must be uint8 (Tq,Tk)')
    if pad is not None and (pad.dtype != torch.uint8 or tuple(pad.shape) != (B, Tk)):
        raise _lib.VhError('attn_rows: pad must be uint8 (B,Tk)')
    if lse2 is not None:        # training forward: keep the row log-sum-exp for attn_rows_bwd
        if tuple(lse2.shape) != (B, n_heads, Tq) or lse2.dtype != torch.float32:
            raise _lib.VhError('attn_rows: lse2 must be float32 (B, n_heads, Tq)')
        check(_lib.lib().vh_attn_rows_lse(
            _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), B,
            n_heads, Tq, Tk, S_max, mode, x_len, ptr(x_len_dev), ptr(kv_len), ptr(mask), ptr(pad),
            ptr(lse2), stream()), 'vh_attn_rows_lse')
        return out
    check(_lib.lib().vh_attn_rows(
        _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), B,
        n_heads, Tq, Tk, S_max, mode, x_len, ptr(x_len_dev), ptr(kv_len), ptr(mask), ptr(pad),
        stream()), 'vh_attn_rows')
    return out


def attn_rows_packed(q, kcache, vcache, out, n_heads, rows):
    """Full-mask attention of every segment of `rows` (an engine.PackedRows) over its own rows of ONE K/V stream: q / out
    (M, ·) with heads at columns head*64, kcache / vcache (1, n_heads, S_max >= M, 64) — `attn_rows` of each utterance alone,
    in one launch and with no padding rows (vh_attn_rows_packed)."""
    _, S_max = _packed_attn_args('attn_rows_packed', q, kcache, vcache, out, n_heads, rows)
    check(_lib.lib().vh_attn_rows_packed(
        _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), n_heads, S_max,
        ptr(rows.seg_start), ptr(rows.seg_len), rows.n_seg, ptr(rows.blocks), rows.n_blocks, stream()), 'vh_attn_rows_packed')
    return out


def needs_x_lens(what, rows):
    """Refuse, under the caller's name `what`, segments without text lengths where the prefix-LM mask is asked for."""
    if rows.seg_x_len is None:
        raise _lib.VhError(f'{what}: the prefix mask needs PackedRows(lengths, device, x_lens)')


def _packed_attn_args(what, q, kcache, vcache, out, n_heads, rows, prefix=False):
    """What every packed attention refuses alike, under the caller's name `what`: a K/V stream that is not (1, n_heads,
    S_max >= M, 64), q / out of other than M rows and, under the prefix mask, segments without text lengths.  Returns (M, S_max)."""
    S_max = kcache.shape[2]
    M = rows.rows
    if tuple(kcache.shape) != (1, n_heads, S_max, HEAD_DIM) or kcache.shape != vcache.shape or M > S_max:
        raise _lib.VhError(f'{what}: cache {tuple(kcache.shape)} M={M}')
    if q.shape[0] != M or out.shape[0] != M:
        raise _lib.VhError(f'{what}: q/out rows')
    if prefix:
        needs_x_lens(what, rows)
    return M, S_max


def _packed_train_args(what, q, kcache, vcache, out, lse2, n_heads, rows, mode):
    M, S_max = _packed_attn_args(what, q, kcache, vcache, out, n_heads, rows)
    if tuple(lse2.shape) != (n_heads, M) or lse2.dtype != torch.float32 or not lse2.is_contiguous():
        raise _lib.VhError(f'{what}: lse2 must be contiguous float32 (n_heads, M)')
    if mode == MASK_PREFIX:
        needs_x_lens(what, rows)
    return M, S_max


def attn_rows_packed_lse(q, kcache, vcache, out, lse2, n_heads, rows, mode):
    """The training forward over packed rows: `attn_rows(..., lse2=)` of every segment of `rows` (an engine.PackedRows) alone —
    B = 1, Tq = Tk = its length, mask `mode` (MASK_FULL, or MASK_PREFIX with the segment's text length rows.x_lens[s]) — in
    one launch, the same bits.  q / out (M, ·), kcache / vcache (1, n_heads, S_max >= M, 64), lse2 (n_heads, M)
    (vh_attn_rows_packed_lse)."""
    M, S_max = _packed_train_args('attn_rows_packed_lse', q, kcache, vcache, out, lse2, n_heads, rows, mode)
    check(_lib.lib().vh_attn_rows_packed_lse(
        _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), n_heads, M, S_max, mode,
        ptr(rows.seg_start), ptr(rows.seg_len), ptr(rows.seg_x_len), rows.n_seg, ptr(rows.blocks), rows.n_blocks, ptr(lse2),
        stream()), 'vh_attn_rows_packed_lse')
    return out


def attn_rows_bwd_packed(q, kcache, vcache, out, dout, lse2, dq, dk, dv, n_heads, rows, mode, chunk_keys=None):
    """dq, dk, dv ((M, d) views with a common row stride) of `attn_rows_packed_lse` given dout: the five-product kernel over
    the (segment, key chunk) items of `rows.bwd_table(chunk_keys)` and, when a segment has more than one chunk, the reduce
    over the dQ slabs in chunk order (vh_attn_rows_bwd_packed).  No atomics: two runs give the same bits."""
    M, S_max = _packed_train_args('attn_rows_bwd_packed', q, kcache, vcache, out, lse2, n_heads, rows, mode)
    if not (dq.stride(0) == dk.stride(0) == dv.stride(0)) or dq.stride(1) != 1:
        raise _lib.VhError('attn_rows_bwd_packed: dq/dk/dv must share one row stride')
    if dq.shape[0] != M or dout.shape[0] != M:
        raise _lib.VhError('attn_rows_bwd_packed: dq/dout rows')
    chunk_keys, max_chunks, items, n_items = rows.bwd_table(chunk_keys)
    need = _lib.lib().vh_attn_rows_bwd_packed_ws_bytes(n_heads, M, max_chunks)
    ws = _stream_ws(_BWD_WS, q.device, need)
    check(_lib.lib().vh_attn_rows_bwd_packed(
        q.data_ptr(), q.stride(0), ptr(kcache), ptr(vcache), out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0),
        ptr(lse2), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0), n_heads, M, S_max, mode, ptr(rows.seg_start),
        ptr(rows.seg_len), ptr(rows.seg_x_len), rows.n_seg, ptr(items), n_items, chunk_keys, max_chunks, ptr(rows.blocks),
        rows.n_blocks, ptr(ws), ws.numel() * 4, stream()), 'vh_attn_rows_bwd_packed')
    return dq, dk, dv


def attn_rows_bwd(q, kcache, vcache, out, dout, lse2, dq, dk, dv, B, n_heads, T, mode, x_len=0,
                  x_len_dev=None, kv_len=None, mask=None, pad=None):
    """dq, dk, dv (each (B*T, d) views with a common row stride, heads at columns h*64) of
    attn_rows(q, kcache, vcache) given dout; P is recomputed tile by tile, never materialised.  Five products in one
    kernel + the slab reduce (vh_attn_rows_bwd_ws); `_lib.lib().vh_set_tuning(VH_TUNE_ATTN_BWD = 13, 1)` selects the
    older two-kernel, seven-product form."""
    S_max = kcache.shape[2]
    if tuple(kcache.shape) != (B, n_heads, S_max, HEAD_DIM) or kcache.shape != vcache.shape or T > S_max:
        raise _lib.VhError(f'attn_rows_bwd: cache {tuple(kcache.shape)} T={T}')
    if not (dq.stride(0) == dk.stride(0) == dv.stride(0)) or dq.stride(1) != 1:
        raise _lib.VhError('attn_rows_bwd: dq/dk/dv must share one row stride')
    # scratch: the dQ partial slabs of the five-product kernel (chunks x (B*h, T, 64) floats: 134 MB at the configs[3] AR
    # step) or, under VH_TUNE_ATTN_BWD = 1, the two-kernel form's D vector.  One growing buffer per (device, stream) —
    # launches of a stream run in order, so its 12 layers share it — instead of 12 allocations of that size per step
    # whose sizes change with every ragged batch.
    need = _lib.lib().vh_attn_rows_bwd_ws_bytes(B, n_heads, T)
    ws = _stream_ws(_BWD_WS, q.device, need)
    check(_lib.lib().vh_attn_rows_bwd_ws(
        q.data_ptr(), q.stride(0), ptr(kcache), ptr(vcache), out.data_ptr(), out.stride(0),
        dout.data_ptr(), dout.stride(0), ptr(lse2), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
        dq.stride(0), B, n_heads, T, S_max, mode, x_len, ptr(x_len_dev), ptr(kv_len), ptr(mask), ptr(pad),
        ptr(ws), ws.numel() * 4, stream()), 'vh_attn_rows_bwd_ws')
    return dq, dk, dv


def softmax_rows(S, ld, B, n_heads, Tq, Tk, scale, mode=MASK_FULL, x_len=0, x_len_dev=None, kv_len=None, mask=None,
                 pad=None):
    """P = softmax(S * scale + mask) in place over the rows of the (B, h, Tq, Tk) maps inside S (row stride ld); the mask
    arguments are those of attn_rows."""
    check(_lib.lib().vh_softmax_rows(S.data_ptr(), ld, B, n_heads, Tq, Tk, float(scale), mode, x_len, ptr(x_len_dev),
                                     ptr(kv_len), ptr(mask), ptr(pad), stream()), 'vh_softmax_rows')
    return S


def attn_generic(q, k, v, out, scale, **spec):
    """Attention for a head width the flash kernels are not built for (they serve 64 = every configuration of the path;
    valle/models/modules.py:109-111 allows any divisor of d_model): the probabilities are MATERIALISED — S = Q K^T on the
    batched MFMA GEMM, the masked row softmax, O = P V on the same GEMM.  Correct for any head width that is a multiple
    of 4, not tuned: O(T^2) memory per (batch row, head).  q (B, h, Tq, hd), k / v (B, h, Tk, hd), out (B, h, Tq, hd):
    views with unit stride in the last dimension (the per-head column blocks of a (rows, 3 d) projection are read in
    place).  Returns P (B, h, Tq, Tk) for a backward that wants it."""
    B, h, Tq, hd = q.shape
    Tk = k.shape[2]
    ATTN_HD_CALLS['materialized'] += 1
    tp = (Tk + 3) // 4 * 4
    P = torch.empty(B, h, Tq, tp, device=q.device, dtype=torch.float32)[..., :Tk]
    gemm(q, k, P)                                               # raw scores
    mask = spec.get('mask')
    if mask is not None and mask.dim() == 3:                    # one mask per batch row: the row softmax row by row
        pad = spec.get('pad')
        for b in range(B):
            softmax_rows(P[b:b + 1], tp, 1, h, Tq, Tk, scale, mode=spec['mode'], mask=mask[b],
                         pad=None if pad is None else pad[b:b + 1])
    else:
        softmax_rows(P, tp, B, h, Tq, Tk, scale, **spec)
    gemm(P, v, out, b_kmajor=True)
    return P


# The flash route of the many-row attention at head widths other than 64 (vh_attn_rows_hd, vh_attn_rows_hd_lse,
# vh_attn_rows_hd_bwd).  None: the environment variable VALLE2_ATTN_HD_FLASH=1 decides; True / False: this value does.  Default
# OFF.  attn_hd_route answers for callers that pick a route per call: TRAINING asks it (autograd.QkvAttentionAnyHeadDimFn:
# flash forward with lse + flash backward, no score map kept) and so does tools/ab_attn_hd.py; the inference stack
# (engine._transformer_forward_generic) still does not and always takes attn_generic: the same kernels, launches and bits as
# before (DESIGN.md section 3.17 says why).
ATTN_HD_FLASH = None
ATTN_HD_CALLS = {'flash': 0, 'materialized': 0}     # calls of attn_rows_hd / attn_generic since reset_attn_hd_calls()
ATTN_HD_BWD_CALLS = {'flash': 0, 'materialized': 0}  # backward calls: attn_rows_hd_bwd / the node's five products


def reset_attn_hd_calls():
    for counts in (ATTN_HD_CALLS, ATTN_HD_BWD_CALLS):
        for key in counts:
            counts[key] = 0


def attn_hd_route(hd, spec):
    """Which many-row attention a head width and a mask spec take: 'flash' (attn_rows_hd) when the switch is on, hd is a
    multiple of 4 from 16 to 128 other than 64 (which has attention.hip's kernels) and `spec` carries no caller-supplied
    `mask` / `pad`; 'materialized' (attn_generic) otherwise.  Pure: no device, no library call."""
    on = ATTN_HD_FLASH if ATTN_HD_FLASH is not None else os.environ.get('VALLE2_ATTN_HD_FLASH') == '1'
    if not on or hd == HEAD_DIM or hd % 4 or not 16 <= hd <= 128:
        return 'materialized'
    if spec.get('mask') is not None or spec.get('pad') is not None or spec.get('mode', MASK_FULL) == MASK_EXPLICIT:
        return 'materialized'
    return 'flash'


def _attn_hd_views(name, views, spec):
    """The checks `attn_rows_hd` and `attn_rows_hd_bwd` share: (B, h, T, hd) float32 device views with unit stride in the last
    dimension, int32 device length vectors."""
    for t, nm in views:
        _f32(t, nm)
        if not t.is_cuda or t.stride(3) != 1:
            raise _lib.VhError(f'{name}: {nm} must be a device view with unit stride in the last dimension')
    B = views[0][0].shape[0]
    for t_, nm in ((spec.get('x_len_dev'), 'x_len_dev'), (spec.get('kv_len'), 'kv_len')):
        if t_ is not None and (t_.dtype != torch.int32 or t_.numel() < B or not t_.is_cuda or not t_.is_contiguous()):
            raise _lib.VhError(f'{name}: {nm} must be a contiguous device int32 tensor of B entries')


def _view_args(t):
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)


def attn_rows_hd(q, k, v, out, scale, lse2=None, **spec):
    """`attn_generic` without the score map: one flash kernel (vh_attn_rows_hd) over the same views — q (B, h, Tq, hd),
    k / v (B, h, Tk, hd), out (B, h, Tq, hd) with unit stride in the last dimension, the per-head column blocks of a
    (rows, 3 d) projection read in place — for hd a multiple of 4 from 16 to 128 and the analytic masks of `spec` (mode,
    x_len, x_len_dev, kv_len; a `mask` or `pad` is refused: those keep attn_generic).  Nothing is returned: no P exists.
    lse2: a contiguous (B, h, Tq) float32 tensor that receives every row's base-2 log-sum-exp (vh_attn_rows_hd_lse): what
    `attn_rows_hd_bwd` recomputes P from."""
    if spec.get('mask') is not None or spec.get('pad') is not None:
        raise _lib.VhError('attn_rows_hd: caller-supplied masks take attn_generic')
    if q.dim() != 4 or out.shape != q.shape or k.shape != v.shape or k.dim() != 4 or k.shape[:2] != q.shape[:2] \
            or k.shape[3] != q.shape[3]:
        raise _lib.VhError(f'attn_rows_hd: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} out {tuple(out.shape)}')
    _attn_hd_views('attn_rows_hd', ((q, 'q'), (k, 'k'), (v, 'v'), (out, 'out')), spec)
    B, h, Tq, hd = q.shape
    Tk = k.shape[2]
    args = (*_view_args(q), *_view_args(k), *_view_args(v), *_view_args(out), B, h, hd, Tq, Tk, float(scale),
            spec.get('mode', MASK_FULL), int(spec.get('x_len', 0)), ptr(spec.get('x_len_dev')), ptr(spec.get('kv_len')))
    if lse2 is not None and (lse2.dtype != torch.float32 or tuple(lse2.shape) != (B, h, Tq) or not lse2.is_cuda
                             or not lse2.is_contiguous()):
        raise _lib.VhError(f'attn_rows_hd: lse2 must be a contiguous device float32 tensor of shape {(B, h, Tq)}')
    ATTN_HD_CALLS['flash'] += 1
    if lse2 is None:
        check(_lib.lib().vh_attn_rows_hd(*args, stream()), 'vh_attn_rows_hd')
    else:
        check(_lib.lib().vh_attn_rows_hd_lse(*args, lse2.data_ptr(), stream()), 'vh_attn_rows_hd_lse')
    return out


def attn_rows_hd_bwd(q, k, v, out, dout, lse2, dq, dk, dv, scale, **spec):
    """dq, dk, dv of `attn_rows_hd(q, k, v, out, scale, lse2=lse2, **spec)` given dout (vh_attn_rows_hd_bwd): two flash
    launches, P recomputed tile by tile from lse2, no score map, no atomics (two runs give the same bits).  All nine are
    (B, h, T, hd) views with unit stride in the last dimension (Tq == Tk == T); dq / dk / dv share one stride set — the column
    blocks of one (rows, 3 d) gradient buffer — and every element of them is written once, so `torch.empty` memory will do."""
    if spec.get('mask') is not None or spec.get('pad') is not None:
        raise _lib.VhError('attn_rows_hd_bwd: caller-supplied masks take the materialised backward')
    views = ((q, 'q'), (k, 'k'), (v, 'v'), (out, 'out'), (dout, 'dout'), (dq, 'dq'), (dk, 'dk'), (dv, 'dv'))
    if q.dim() != 4 or any(t.shape != q.shape for t, _ in views):
        raise _lib.VhError('attn_rows_hd_bwd: ' + ' '.join(f'{nm} {tuple(t.shape)}' for t, nm in views) + ' (one shape, Tq == Tk)')
    _attn_hd_views('attn_rows_hd_bwd', views, spec)
    if not (dq.stride() == dk.stride() == dv.stride()):
        raise _lib.VhError('attn_rows_hd_bwd: dq/dk/dv must share one stride set')
    B, h, T, hd = q.shape
    if lse2.dtype != torch.float32 or tuple(lse2.shape) != (B, h, T) or not lse2.is_cuda or not lse2.is_contiguous():
        raise _lib.VhError(f'attn_rows_hd_bwd: lse2 must be a contiguous device float32 tensor of shape {(B, h, T)}')
    need = _lib.lib().vh_attn_rows_hd_bwd_ws_bytes(B, h, T)
    ws = _stream_ws(_BWD_WS, q.device, need)
    ATTN_HD_BWD_CALLS['flash'] += 1
    check(_lib.lib().vh_attn_rows_hd_bwd(
        *_view_args(q), *_view_args(k), *_view_args(v), *_view_args(out), *_view_args(dout), lse2.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0), dq.stride(1), dq.stride(2), B, h, hd, T, float(scale),
        spec.get('mode', MASK_FULL), int(spec.get('x_len', 0)), ptr(spec.get('x_len_dev')), ptr(spec.get('kv_len')),
        ptr(ws), ws.numel() * 4, stream()), 'vh_attn_rows_hd_bwd')
    return dq, dk, dv


def attn_decode_ws(B, n_heads, n_split, device):
    """Workspace of a key-split decode attention: split records + the per-(b, head) ticket words, which must start at
    zero (the kernel re-arms them itself) — hence zeros, not empty."""
    n = _lib.lib().vh_attn_decode_ws_bytes(B, n_heads, n_split)
    return torch.zeros(max(n, 16) // 4, device=device, dtype=torch.float32) if n else None


def attn_decode(q, kcache, vcache, out, cache_len, len_bias, n_split=1, partial=None):
    B, n_heads, S_max, hd = kcache.shape
    if hd != HEAD_DIM:                                   # another head width: the _hd kernel (width 64 is unchanged below)
        return attn_decode_hd(q, kcache, vcache, out, cache_len, len_bias, n_split, partial)
    if q.shape[0] != B or out.shape[0] != B:
        raise _lib.VhError('attn_decode: shapes')
    if cache_len.dtype != torch.int32 or cache_len.numel() != B:
        raise _lib.VhError('attn_decode: cache_len must be int32 (B)')
    check(_lib.lib().vh_attn_decode(
        q.data_ptr(), q.stride(0), ptr(kcache), ptr(vcache), out.data_ptr(), out.stride(0),
        ptr(cache_len), len_bias, B, n_heads, S_max, n_split, ptr(partial), stream()),
        'vh_attn_decode')
    return out


def attn_decode_hd_ws(B, n_heads, head_dim, n_split, device):
    """Record workspace of `attn_decode_hd` (vh_attn_decode_hd_ws_bytes), as a float32 tensor; None without key splits."""
    n = _lib.lib().vh_attn_decode_hd_ws_bytes(B, n_heads, head_dim, n_split)
    return torch.empty(max(n, 16) // 4, device=device, dtype=torch.float32) if n else None


def attn_decode_hd(q, kcache, vcache, out, cache_len, len_bias, n_split=1, partial=None, scale=None):
    """One-query attention of B rows over fp32 caches (B, h, S_max, head_dim) at any served head width (multiples of 4
    from 16 to 256; vh_attn_decode_hd): keys 0 .. cache_len[b] + len_bias - 1; scale defaults to head_dim ** -0.5."""
    B, n_heads, S_max, hd = kcache.shape
    if tuple(vcache.shape) != tuple(kcache.shape) or q.shape[0] != B or out.shape[0] != B or \
            q.shape[1] < n_heads * hd or out.shape[1] < n_heads * hd:
        raise _lib.VhError(f'attn_decode_hd: q {tuple(q.shape)} cache {tuple(kcache.shape)} out {tuple(out.shape)}')
    if not (kcache.is_contiguous() and vcache.is_contiguous()) or kcache.dtype != torch.float32 or vcache.dtype != torch.float32:
        raise _lib.VhError('attn_decode_hd: contiguous fp32 caches')
    if cache_len.dtype != torch.int32 or cache_len.numel() != B:
        raise _lib.VhError('attn_decode_hd: cache_len must be int32 (B)')
    if partial is None and n_split > 1:
        partial = attn_decode_hd_ws(B, n_heads, hd, n_split, q.device)
    scale = float(hd ** -0.5) if scale is None else float(scale)
    check(_lib.lib().vh_attn_decode_hd(
        _dev_f32(q, 'q'), q.stride(0), ptr(kcache), ptr(vcache), _dev_f32(out, 'out'), out.stride(0), ptr(cache_len),
        len_bias, B, n_heads, hd, S_max, scale, n_split, ptr(partial), partial.numel() * 4 if partial is not None else 0,
        stream()), 'vh_attn_decode_hd')
    return out


def linear_qkv_hd(a, wqkv, q_out, kcache, vcache, n_heads, cache_len, ln=None, folded=None, eps=1e-5):
    """The decode step's QKV projection at any head width (vh_linear_qkv_hd / vh_linear_qkv_folded_hd): one new row per
    sequence (T = 1, B <= 64); Q -> q_out (B, d), the K / V rows appended at cache_len[b] of the caches
    (B, h, S_max, d / h).  LayerNorm fused from ln = (gamma, beta, ada_scale, ada_shift, eps) as in `linear`, or from the
    folded triple of ln_fold."""
    B, d = a.shape
    S_max = kcache.shape[2]
    hd = d // n_heads if n_heads else 0
    w = folded[0] if folded is not None else wqkv
    if tuple(w.shape) != (3 * d, d) or d != n_heads * hd or tuple(kcache.shape) != (B, n_heads, S_max, hd) or \
            kcache.shape != vcache.shape or tuple(q_out.shape[:1]) != (B,):
        raise _lib.VhError(f'linear_qkv_hd: shapes a={tuple(a.shape)} w={tuple(w.shape)} cache={tuple(kcache.shape)}')
    if cache_len is None or cache_len.dtype != torch.int32 or cache_len.numel() != B:
        raise _lib.VhError('linear_qkv_hd: cache_len must be int32 (B)')
    if folded is not None:
        wf, c1, c2 = folded
        check(_lib.lib().vh_linear_qkv_folded_hd(
            _dev_f32(a, 'a'), a.stride(0), ptr(wf), ptr(c1), ptr(c2), _dev_f32(q_out, 'q_out'), q_out.stride(0), ptr(kcache),
            ptr(vcache), ptr(cache_len), B, 1, d, n_heads, S_max, eps, hd, stream()), 'vh_linear_qkv_folded_hd')
        return q_out
    g, b, sc, sh, ln_eps = _ln_args(ln)
    check(_lib.lib().vh_linear_qkv_hd(
        _dev_f32(a, 'a'), a.stride(0), ptr(wqkv), _dev_f32(q_out, 'q_out'), q_out.stride(0), ptr(kcache), ptr(vcache),
        ptr(cache_len), B, 1, d, n_heads, S_max, g, b, sc, sh, ln_eps, hd, stream()), 'vh_linear_qkv_hd')
    return q_out


def kv_store(qkv, kcache, vcache, B, T):
    """K / V column blocks of a (B*T, 3 d) QKV projection into cache rows 0..T-1 of (B, h, S_max, d / h) caches
    (vh_kv_store; a bit-exact copy)."""
    _, n_heads, S_max, hd = kcache.shape
    d = n_heads * hd
    if qkv.dim() != 2 or qkv.shape[0] != B * T or qkv.shape[1] < 3 * d or qkv.stride(1) != 1 or \
            tuple(kcache.shape[:2]) != (B, n_heads) or kcache.shape != vcache.shape or T > S_max:
        raise _lib.VhError(f'kv_store: qkv {tuple(qkv.shape)} cache {tuple(kcache.shape)} B={B} T={T}')
    if not (kcache.is_contiguous() and vcache.is_contiguous()) or kcache.dtype != torch.float32:
        raise _lib.VhError('kv_store: contiguous fp32 caches')
    check(_lib.lib().vh_kv_store(_dev_f32(qkv, 'qkv'), qkv.stride(0), ptr(kcache), ptr(vcache), B, T, n_heads, hd, S_max,
                                 stream()), 'vh_kv_store')
    return kcache, vcache


def kv_unpack(src, dst, seg_start, seg_len, dst_row):
    """The K/V rows a packed forward wrote, to the rows of a cache, all layers and both of K and V in ONE launch (vh_kv_unpack;
    a bit-exact copy).  src (..., h, S_src, 64) and dst (..., B_dst, h, S_dst, 64): contiguous fp32 with the same leading
    streams (a one-row `KVCache.buf` (L, 2, 1, h, S_src, 64) and a cache's (L, 2, B_dst, h, S_dst, 64)).  seg_start / seg_len /
    dst_row: device int32 (n_seg) — rows seg_start[s] .. + seg_len[s] - 1 of every (stream, head) go to positions 0 ..
    seg_len[s] - 1 of row dst_row[s]; nothing else of dst is written.  A segment past S_src or longer than S_dst is cut there, a
    row outside [0, B_dst) writes nothing."""
    if src.dtype != torch.float32 or dst.dtype != torch.float32 or not src.is_contiguous() or not dst.is_contiguous():
        raise _lib.VhError('kv_unpack: src and dst must be contiguous float32')
    return _kv_unpack('kv_unpack', _lib.lib().vh_kv_unpack, src, dst, seg_start, seg_len, dst_row)


def _kv_unpack(what, entry, src, dst, seg_start, seg_len, dst_row):
    """The shape checks and the call of `kv_unpack` and `kv_unpack_bf16` (the dtype is the caller's check)."""
    if not src.is_cuda or not dst.is_cuda:
        raise _lib.VhError(f'{what}: src and dst must be on the HIP device')
    if src.dim() < 4 or dst.dim() < 5 or src.shape[-1] != HEAD_DIM or dst.shape[-1] != HEAD_DIM:
        raise _lib.VhError(f'{what}: src {tuple(src.shape)} / dst {tuple(dst.shape)}: (streams, h, S_src, 64) and (streams, B_dst, h, S_dst, 64)')
    n_heads, S_src = src.shape[-3], src.shape[-2]
    B_dst, S_dst = dst.shape[-4], dst.shape[-2]
    if min(n_heads, S_src, B_dst, S_dst) < 1 or dst.shape[-3] != n_heads:
        raise _lib.VhError(f'{what}: src {tuple(src.shape)} / dst {tuple(dst.shape)}: the same heads, every dimension >= 1')
    n_streams = src.numel() // (n_heads * S_src * HEAD_DIM)
    if (src.dim() == 6 and src.shape[2] != 1) or dst.numel() != n_streams * B_dst * n_heads * S_dst * HEAD_DIM:
        raise _lib.VhError(f'{what}: src {tuple(src.shape)} holds {n_streams} one-row streams, dst {tuple(dst.shape)} does not match')
    n_seg = seg_start.numel()
    for t_ in (seg_start, seg_len, dst_row):
        if t_.dtype != torch.int32 or t_.numel() != n_seg or not t_.is_cuda or not t_.is_contiguous() or n_seg < 1:
            raise _lib.VhError(f'{what}: seg_start / seg_len / dst_row must be device int32 tensors of the same n_seg >= 1 entries')
    check(entry(ptr(src), ptr(dst), n_streams, n_heads, S_src, B_dst, S_dst, ptr(seg_start), ptr(seg_len), ptr(dst_row), n_seg,
                stream()), 'vh_' + what)
    return dst


def attn_decode_shared_ws(B, n_heads, prefix_len, n_split, device):
    """Record workspace of `attn_decode_shared` (vh_attn_decode_shared_ws_bytes), as a float32 tensor."""
    n = _lib.lib().vh_attn_decode_shared_ws_bytes(B, n_heads, prefix_len, n_split)
    return torch.empty(max(n, 16) // 4, device=device, dtype=torch.float32)


def attn_decode_shared(q, kprefix, vprefix, prefix_len, ksuffix, vsuffix, out, suffix_len, len_bias, n_split=1, partial=None):
    """One-query attention of B beams over a SHARED prompt (kprefix / vprefix (1, h, prefix_S, 64), first `prefix_len` rows)
    followed by each beam's own rows (ksuffix / vsuffix (B, h, S_suf, 64), suffix_len[b] + len_bias of them)."""
    B, n_heads, S_suf, hd = ksuffix.shape
    if hd != HEAD_DIM or tuple(kprefix.shape[:2]) != (1, n_heads) or kprefix.shape[3] != HEAD_DIM or q.shape[0] != B:
        raise _lib.VhError(f'attn_decode_shared: prefix {tuple(kprefix.shape)} suffix {tuple(ksuffix.shape)} q {tuple(q.shape)}')
    if suffix_len.dtype != torch.int32 or suffix_len.numel() != B:
        raise _lib.VhError('attn_decode_shared: suffix_len must be int32 (B)')
    if partial is None:
        partial = attn_decode_shared_ws(B, n_heads, prefix_len, n_split, q.device)
    check(_lib.lib().vh_attn_decode_shared(
        _dev_f32(q, 'q'), q.stride(0), ptr(kprefix), ptr(vprefix), prefix_len, kprefix.shape[2], ptr(ksuffix), ptr(vsuffix),
        _dev_f32(out, 'out'), out.stride(0), ptr(suffix_len), len_bias, B, n_heads, S_suf, n_split, ptr(partial),
        partial.numel() * 4, stream()), 'vh_attn_decode_shared')
    return out


def attn_decode_kv16(q, kcache16, vcache16, out, cache_len, len_bias, n_split=1, partial=None):
    """attn_decode over a 16-bit K/V cache (perf mode).  n_split == 1: one (row, head) per workgroup (vh_attn_decode_kv16);
    n_split 2..16: the key range of a (row, head) split over n_split workgroups whose records a second launch adds in split
    order (vh_attn_decode_kv16_split; `partial`: attn_decode_ws(), allocated here when None)."""
    B, n_heads, S_max, hd = kcache16.shape
    if hd != HEAD_DIM or kcache16.dtype != H16 or vcache16.dtype != H16 or q.shape[0] != B:
        raise _lib.VhError('attn_decode_kv16: bf16 caches (B, h, S_max, 64)')
    if cache_len.dtype != torch.int32 or cache_len.numel() != B:
        raise _lib.VhError('attn_decode_kv16: cache_len must be int32 (B)')
    if n_split == 1 and partial is None:
        check(_lib.lib().vh_attn_decode_kv16(_dev_f32(q, 'q'), q.stride(0), ptr(kcache16), ptr(vcache16), _dev_f32(out, 'out'),
                                             out.stride(0), ptr(cache_len), len_bias, B, n_heads, S_max, stream()),
              'vh_attn_decode_kv16')
        return out
    if partial is None and 1 < n_split <= 16:
        partial = attn_decode_ws(B, n_heads, n_split, q.device)
    check(_lib.lib().vh_attn_decode_kv16_split(
        _dev_f32(q, 'q'), q.stride(0), ptr(kcache16), ptr(vcache16), _dev_f32(out, 'out'), out.stride(0), ptr(cache_len),
        len_bias, B, n_heads, S_max, n_split, ptr(partial), partial.numel() * 4 if partial is not None else 0, stream()),
        'vh_attn_decode_kv16_split')
    return out


def attn_decode_shared_groups_ws(B, n_heads, prefix_cap, n_split, device):
    """Record workspace of `attn_decode_shared_groups` (vh_attn_decode_shared_groups_ws_bytes), as a float32 tensor."""
    n = _lib.lib().vh_attn_decode_shared_groups_ws_bytes(B, n_heads, prefix_cap, n_split)
    return torch.empty(max(n, 16) // 4, device=device, dtype=torch.float32)


def attn_decode_shared_groups(q, kprefix, vprefix, prefix_len, prefix_cap, ksuffix, vsuffix, out, suffix_len, len_bias, beams,
                              n_split=1, partial=None):
    """One-query attention of B = G * beams rows, rows g * beams .. g * beams + beams - 1 over THEIR prompt (kprefix /
    vprefix (G, h, prefix_S, 64), first prefix_len[g] rows; prefix_len an int32 DEVICE tensor (G), every entry in
    1..prefix_cap, or 0 for a PARKED group: nothing of it is read and its rows of `out` are exactly 0.0) followed by each row's own rows (ksuffix / vsuffix (B, h, S_suf, 64), suffix_len[b] + len_bias of them).

    vh_attn_decode_shared_groups serves at most 64 rows per call (the decoder never holds more).  More rows than that go
    through it here in consecutive calls of whole groups, at most 64 rows each, every call on its rows' own part of
    `partial` (the workspace of all B rows) — the same chunking as generate_batch(beams=n) applies to a whole decode."""
    B, n_heads, S_suf, hd = ksuffix.shape
    if beams < 1 or B % beams:
        raise _lib.VhError(f'attn_decode_shared_groups: {B} rows are not a multiple of beams={beams}')
    if B > 64:
        if beams > 64:
            raise _lib.VhError(f'attn_decode_shared_groups: beams={beams}: a group holds at most 64 rows')
        if partial is None:
            partial = attn_decode_shared_groups_ws(B, n_heads, prefix_cap, n_split, q.device)
        per_row = _lib.lib().vh_attn_decode_shared_groups_ws_bytes(1, n_heads, prefix_cap, n_split) // 4    # floats
        if per_row == 0 or q.shape[0] != B or out.shape[0] != B or kprefix.shape[0] != B // beams or vprefix.shape[0] != B // beams or \
                prefix_len.numel() != B // beams or suffix_len.numel() != B or partial.numel() < B * per_row:
            raise _lib.VhError(f'attn_decode_shared_groups: prefix {tuple(kprefix.shape)} suffix {tuple(ksuffix.shape)} '
                               f'q {tuple(q.shape)} beams {beams} workspace {partial.numel() * 4} bytes')
        step = 64 // beams                                       # whole groups per call
        for g0 in range(0, B // beams, step):
            g1 = min(g0 + step, B // beams)
            r = slice(g0 * beams, g1 * beams)
            attn_decode_shared_groups(q[r], kprefix[g0:g1], vprefix[g0:g1], prefix_len[g0:g1], prefix_cap, ksuffix[r], vsuffix[r],
                                      out[r], suffix_len[r], len_bias, beams, n_split,
                                      partial[r.start * per_row:r.stop * per_row])
        return out
    G = B // beams
    if hd != HEAD_DIM or tuple(kprefix.shape[:2]) != (G, n_heads) or kprefix.shape[3] != HEAD_DIM or q.shape[0] != B or \
            kprefix.shape != vprefix.shape or ksuffix.shape != vsuffix.shape:
        raise _lib.VhError(f'attn_decode_shared_groups: prefix {tuple(kprefix.shape)} suffix {tuple(ksuffix.shape)} '
                           f'q {tuple(q.shape)} beams {beams}')
    if prefix_len.dtype != torch.int32 or prefix_len.numel() != G or not prefix_len.is_cuda:
        raise _lib.VhError('attn_decode_shared_groups: prefix_len must be an int32 device tensor (G)')
    if suffix_len.dtype != torch.int32 or suffix_len.numel() != B:
        raise _lib.VhError('attn_decode_shared_groups: suffix_len must be int32 (B)')
    if partial is None:
        partial = attn_decode_shared_groups_ws(B, n_heads, prefix_cap, n_split, q.device)
    check(_lib.lib().vh_attn_decode_shared_groups(
        _dev_f32(q, 'q'), q.stride(0), ptr(kprefix), ptr(vprefix), ptr(prefix_len), prefix_cap, kprefix.shape[2], ptr(ksuffix),
        ptr(vsuffix), _dev_f32(out, 'out'), out.stride(0), ptr(suffix_len), len_bias, B, beams, n_heads, S_suf, n_split,
        ptr(partial), partial.numel() * 4, stream()), 'vh_attn_decode_shared_groups')
    return out


def attn_decode_shared_kv16(q, kprefix16, vprefix16, prefix_len, ksuffix16, vsuffix16, out, suffix_len, len_bias, n_split=1,
                            partial=None):
    """`attn_decode_shared` over 16-bit caches (perf mode with a shared prompt): kprefix16 / vprefix16 (1, h, prefix_S, 64) and
    ksuffix16 / vsuffix16 (B, h, S_suf, 64) in the library's 16-bit format; q, the softmax and the accumulators fp32."""
    B, n_heads, S_suf, hd = ksuffix16.shape
    if hd != HEAD_DIM or tuple(kprefix16.shape[:2]) != (1, n_heads) or kprefix16.shape[3] != HEAD_DIM or q.shape[0] != B or \
            kprefix16.shape != vprefix16.shape or ksuffix16.shape != vsuffix16.shape:
        raise _lib.VhError(f'attn_decode_shared_kv16: prefix {tuple(kprefix16.shape)} suffix {tuple(ksuffix16.shape)} '
                           f'q {tuple(q.shape)}')
    if any(t.dtype != H16 for t in (kprefix16, vprefix16, ksuffix16, vsuffix16)):
        raise _lib.VhError(f'attn_decode_shared_kv16: prefix and suffix caches must be {H16}')
    if suffix_len.dtype != torch.int32 or suffix_len.numel() != B:
        raise _lib.VhError('attn_decode_shared_kv16: suffix_len must be int32 (B)')
    if partial is None:
        partial = attn_decode_shared_ws(B, n_heads, prefix_len, n_split, q.device)
    check(_lib.lib().vh_attn_decode_shared_kv16(
        _dev_f32(q, 'q'), q.stride(0), ptr(kprefix16), ptr(vprefix16), prefix_len, kprefix16.shape[2], ptr(ksuffix16),
        ptr(vsuffix16), _dev_f32(out, 'out'), out.stride(0), ptr(suffix_len), len_bias, B, n_heads, S_suf, n_split, ptr(partial),
        partial.numel() * 4, stream()), 'vh_attn_decode_shared_kv16')
    return out


def linear_qkv_folded_kv16(a, folded, q_out, kcache16, vcache16, n_heads, cache_len, eps=1e-5):
    wf, c1, c2 = folded
    B, d = a.shape
    S_max = kcache16.shape[2]
    if tuple(wf.shape) != (3 * d, d) or tuple(kcache16.shape) != (B, n_heads, S_max, HEAD_DIM) or \
            kcache16.dtype != H16 or vcache16.dtype != H16:
        raise _lib.VhError('linear_qkv_folded_kv16: shapes / dtypes')
    check(_lib.lib().vh_linear_qkv_folded_kv16(_dev_f32(a, 'a'), a.stride(0), ptr(wf), ptr(c1), ptr(c2), q_out.data_ptr(),
                                               q_out.stride(0), ptr(kcache16), ptr(vcache16), ptr(cache_len), B, d,
                                               n_heads, S_max, eps, stream()), 'vh_linear_qkv_folded_kv16')
    return q_out


# ---- perf mode of the MFMA-bound legs: bf16 operands, fp32 accumulate (include/valle_hip.h; SECONDARY, never the parity path)
def _bf16(t, name):
    if t.dtype != H16 or not t.is_cuda or t.stride(-1) != 1:
        raise _lib.VhError(f'{name} must be a row-major {H16} HIP tensor, got {t.dtype} on {t.device}')
    return t.data_ptr()


def to_bf16(x, out=None):
    """Round-to-nearest-even narrowing of a (rows, cols) fp32 matrix (vh_to_bf16): weights once per weight set."""
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=H16)
    check(_lib.lib().vh_to_bf16(_dev_f32(x, 'x'), x.stride(0), _bf16(out, 'out'), out.stride(0), rows, cols, stream()),
          'vh_to_bf16')
    return out


def layernorm_bf16(x, gamma, beta, out=None, ada_scale=None, ada_shift=None, eps=1e-5):
    d = x.shape[-1]
    rows = x.numel() // d
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=H16)
    check(_lib.lib().vh_layernorm_bf16(ptr(_f32(x, 'x')), ptr(gamma), ptr(beta), ptr(ada_scale), ptr(ada_shift),
                                       _bf16(out, 'out'), rows, d, eps, stream()), 'vh_layernorm_bf16')
    return out


def linear_bf16(a, w, bias=None, residual=None, out=None, act=ACT_NONE, out_bf16=False):
    """out = act(a @ w.T + bias) + residual with a (M,K), w (N,K) bf16; fp32 accumulate; out fp32 or bf16."""
    M, K = a.shape
    N, K2 = w.shape
    if K != K2 or not w.is_contiguous():
        raise _lib.VhError(f'linear_bf16: K mismatch {K} vs {K2} / w must be contiguous')
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=H16 if out_bf16 else torch.float32)
    if out.dtype != (H16 if out_bf16 else torch.float32) or out.stride(1) != 1:
        raise _lib.VhError('linear_bf16: out dtype / layout')
    check(_lib.lib().vh_linear_bf16(_bf16(a, 'a'), a.stride(0), _bf16(w, 'w'), ptr(bias),
                                    _dev_f32(residual, 'residual') if residual is not None else None,
                                    residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0),
                                    int(out_bf16), M, N, K, act, stream()), 'vh_linear_bf16')
    return out


Q16_PRESCALE = 0.125 * 1.4426950408889634     # perf mode: q leaves linear_qkv_bf16 scaled by 1/sqrt(64) * log2(e); attn_rows_bf16 expects it


def linear_qkv_bf16(a, wqkv, q_out, kcache16, vcache16, B, T, n_heads, cache_len=None):
    d = a.shape[1]
    S_max = kcache16.shape[2]
    if tuple(wqkv.shape) != (3 * d, d) or tuple(kcache16.shape) != (B, n_heads, S_max, HEAD_DIM) or a.shape[0] != B * T:
        raise _lib.VhError('linear_qkv_bf16: shapes')
    check(_lib.lib().vh_linear_qkv_bf16(_bf16(a, 'a'), a.stride(0), _bf16(wqkv, 'wqkv'), _bf16(q_out, 'q_out'),
                                        q_out.stride(0), _bf16(kcache16, 'kcache'), _bf16(vcache16, 'vcache'), ptr(cache_len),
                                        B, T, d, n_heads, S_max, stream()), 'vh_linear_qkv_bf16')
    return q_out


def attn_rows_bf16(q, kcache16, vcache16, out, B, n_heads, Tq, Tk, mode, x_len=0, x_len_dev=None, kv_len=None):
    S_max = kcache16.shape[2]
    if tuple(kcache16.shape) != (B, n_heads, S_max, HEAD_DIM) or Tk > S_max or Tq > Tk or q.shape[0] != B * Tq:
        raise _lib.VhError(f'attn_rows_bf16: cache {tuple(kcache16.shape)} Tq={Tq} Tk={Tk}')
    check(_lib.lib().vh_attn_rows_bf16(_bf16(q, 'q'), q.stride(0), _bf16(kcache16, 'kcache'), _bf16(vcache16, 'vcache'),
                                       _bf16(out, 'out'), out.stride(0), B, n_heads, Tq, Tk, S_max, mode, x_len,
                                       ptr(x_len_dev), ptr(kv_len), stream()), 'vh_attn_rows_bf16')
    return out


def attn_rows_packed_bf16(q, kcache, vcache, out, n_heads, rows):
    """`attn_rows_packed` in the 16-bit format of perf mode: full-mask attention of every segment of `rows` (an
    engine.PackedRows) over its own rows of ONE 16-bit K/V stream.  q (pre-scaled by Q16_PRESCALE, as `linear_qkv_bf16` leaves
    it) / out (M, ·) H16 with heads at columns head*64, kcache / vcache (1, n_heads, S_max >= M, 64) H16 — `attn_rows_bf16` of
    each utterance alone, in one launch and with no padding rows (vh_attn_rows_packed_bf16)."""
    _, S_max = _packed_attn_args('attn_rows_packed_bf16', q, kcache, vcache, out, n_heads, rows)
    check(_lib.lib().vh_attn_rows_packed_bf16(
        _bf16(q, 'q'), q.stride(0), _bf16(kcache, 'kcache'), _bf16(vcache, 'vcache'), _bf16(out, 'out'), out.stride(0), n_heads,
        S_max, ptr(rows.seg_start), ptr(rows.seg_len), rows.n_seg, ptr(rows.blocks), rows.n_blocks, stream()),
        'vh_attn_rows_packed_bf16')
    return out


def attn_rows_packed_lm_bf16(q, kcache, vcache, out, n_heads, rows):
    """`attn_rows_packed_bf16` under the PREFIX-LM mask: every segment of `rows` (an engine.PackedRows built with x_lens, or an
    engine.PromptRows) attends its own rows of ONE 16-bit K/V stream under the prefix mask of its own text length — per segment
    the bits of `attn_rows_bf16(B=1, Tq=Tk=len, MASK_PREFIX, x_len)` on it alone (vh_attn_rows_packed_lm_bf16).  Operands as for
    `attn_rows_packed_bf16`."""
    _, S_max = _packed_attn_args('attn_rows_packed_lm_bf16', q, kcache, vcache, out, n_heads, rows, prefix=True)
    check(_lib.lib().vh_attn_rows_packed_lm_bf16(
        _bf16(q, 'q'), q.stride(0), _bf16(kcache, 'kcache'), _bf16(vcache, 'vcache'), _bf16(out, 'out'), out.stride(0), n_heads,
        S_max, ptr(rows.seg_start), ptr(rows.seg_len), ptr(rows.seg_x_len), rows.n_seg, ptr(rows.blocks), rows.n_blocks, stream()),
        'vh_attn_rows_packed_lm_bf16')
    return out


def kv_unpack_bf16(src, dst, seg_start, seg_len, dst_row):
    """`kv_unpack` for 16-bit streams (vh_kv_unpack_bf16): src (..., h, S_src, 64) and dst (..., B_dst, h, S_dst, 64) contiguous
    H16 with the same leading streams; the same tables, the same cuts, a bit-exact copy and nothing else of dst written."""
    if src.dtype != H16 or dst.dtype != H16 or not src.is_contiguous() or not dst.is_contiguous():
        raise _lib.VhError(f'kv_unpack_bf16: src and dst must be contiguous {H16}')
    return _kv_unpack('kv_unpack_bf16', _lib.lib().vh_kv_unpack_bf16, src, dst, seg_start, seg_len, dst_row)


def greedy_step(logits, V, eos, codes, eos_count, audio_emb, pe, audio_pos, cache_len, x_next,
                pos_base=None):
    B = logits.shape[0]
    d = x_next.shape[1]
    check(_lib.lib().vh_greedy_step(
        logits.data_ptr(), logits.stride(0), V, eos, ptr(codes), codes.stride(0), ptr(eos_count),
        ptr(pos_base), ptr(audio_emb), ptr(pe), ptr(audio_pos), ptr(cache_len), ptr(_f32(x_next, 'x_next')), B, d,
        stream()), 'vh_greedy_step')


def head_greedy_ws(B, V, device):
    """Zeroed workspace of vh_head_greedy (arrival counters + one candidate per row and 16-column block)."""
    return torch.zeros(_lib.lib().vh_head_greedy_ws_bytes(B, V) // 4, device=device, dtype=torch.int32)


def head_greedy(x, proj_w, logits, V, eos, codes, eos_count, audio_emb, pe, audio_pos, cache_len, x_next, ws, pos_base=None):
    """The AR head and the greedy step in ONE launch: logits = x @ proj_w.T, then what greedy_step does with them."""
    B, d = x.shape
    check(_lib.lib().vh_head_greedy(
        ptr(_f32(x, 'x')), x.stride(0), ptr(_f32(proj_w, 'proj_w')), ptr(_f32(logits, 'logits')), logits.stride(0), V, eos,
        ptr(codes), codes.stride(0), ptr(eos_count), ptr(pos_base), ptr(audio_emb), ptr(pe), ptr(audio_pos), ptr(cache_len),
        ptr(_f32(x_next, 'x_next')), B, d, ptr(ws), ws.numel() * 4, stream()), 'vh_head_greedy')


def sample_step(logits, V, eos, top_k, top_p, temperature, seed, codes, eos_count, sum_logprobs, audio_emb,
                pe, audio_pos, cache_len, x_next, pos_base=None, wide=None, rs=None, limits=None):
    """The stochastic decode step: `vh_sample_step` up to V = SAMPLE_NARROW_V, `vh_sample_step_wide` above it (up to
    SAMPLE_MAX_V).  wide=True / False forces one kernel (tests compare the two at V <= 2048).  rs: a uint8 device tensor
    (B, ROW_SAMPLING_BYTES) of vh_row_sampling records (`pack_row_sampling`) — every row's seed, draw key and filter come
    from its record (`vh_sample_step_rows` / `vh_sample_step_wide_rows`) and top_k, top_p, temperature and seed are not read.
    limits (with rs and pos_base): a uint8 device tensor (B, ROW_LIMITS_BYTES) of vh_row_limits records (`pack_row_limits`)
    — every row's (min_new, max_new), through `vh_sample_step_rows_bounded` / `vh_sample_step_wide_rows_bounded`."""
    B = logits.shape[0]
    d = x_next.shape[1]
    if wide is None:
        wide = V > SAMPLE_NARROW_V
    name = 'vh_sample_step_wide' if wide else 'vh_sample_step'
    if limits is not None:
        if rs is None:
            raise _lib.VhError('sample_step: limits without rs (the length bounds sit beside per-row sampling records)')
        if limits.dtype != torch.uint8 or tuple(limits.shape) != (B, ROW_LIMITS_BYTES) or not limits.is_cuda or not limits.is_contiguous():
            raise _lib.VhError(f'sample_step: limits must be a contiguous uint8 device tensor ({B}, {ROW_LIMITS_BYTES}), got '
                               f'{tuple(limits.shape)} {limits.dtype}')
    if rs is not None:
        if rs.dtype != torch.uint8 or tuple(rs.shape) != (B, ROW_SAMPLING_BYTES) or not rs.is_cuda:
            raise _lib.VhError(f'sample_step: rs must be a uint8 device tensor ({B}, {ROW_SAMPLING_BYTES}), got {tuple(rs.shape)} {rs.dtype}')
        name += '_rows'
        if limits is not None:
            name += '_bounded'
            check(getattr(_lib.lib(), name)(
                logits.data_ptr(), logits.stride(0), V, eos, ptr(rs), ptr(limits), ptr(codes), codes.stride(0), ptr(eos_count),
                ptr(pos_base), ptr(sum_logprobs), ptr(audio_emb), ptr(pe), ptr(audio_pos), ptr(cache_len),
                ptr(_f32(x_next, 'x_next')), B, d, stream()), name)
            return
        check(getattr(_lib.lib(), name)(
            logits.data_ptr(), logits.stride(0), V, eos, ptr(rs), ptr(codes), codes.stride(0), ptr(eos_count), ptr(pos_base),
            ptr(sum_logprobs), ptr(audio_emb), ptr(pe), ptr(audio_pos), ptr(cache_len), ptr(_f32(x_next, 'x_next')),
            B, d, stream()), name)
        return
    check(getattr(_lib.lib(), name)(
        logits.data_ptr(), logits.stride(0), V, eos, int(top_k), float(top_p), float(temperature),
        int(seed) & (2 ** 64 - 1), ptr(codes), codes.stride(0), ptr(eos_count), ptr(pos_base),
        ptr(sum_logprobs), ptr(audio_emb), ptr(pe), ptr(audio_pos), ptr(cache_len), ptr(_f32(x_next, 'x_next')),
        B, d, stream()), name)


ROW_SAMPLING_BYTES = 32   # sizeof(vh_row_sampling)
_ROW_SAMPLING_DTYPE = [('seed', '<u8'), ('key', '<u4'), ('top_k', '<i4'), ('top_p', '<f4'), ('temperature', '<f4'),
                       ('reserved', '<u4', (2,))]


def pack_row_sampling(records):
    """[(seed, key, top_k, top_p, temperature[, window, max_repeats]), ...] -> a HOST uint8 tensor (n, ROW_SAMPLING_BYTES)
    in the layout of vh_row_sampling (include/valle_hip.h), one record per decode row.  The two reserved words are the
    repetition-aware rule's (sampling.RepetitionAware.records); a 5-tuple leaves them (0, 0): the rule off."""
    import numpy as np
    arr = np.zeros(len(records), dtype=np.dtype(_ROW_SAMPLING_DTYPE))
    assert arr.dtype.itemsize == ROW_SAMPLING_BYTES
    for i, (seed, key, top_k, top_p, temperature, *ras) in enumerate(records):
        if len(ras) not in (0, 2):
            raise ValueError(f'pack_row_sampling: record {i} holds {5 + len(ras)} values (5, or 7 with window and max_repeats)')
        arr[i] = (int(seed), int(key), int(top_k), float(top_p), float(temperature), tuple(int(v) for v in ras) or (0, 0))
    return torch.from_numpy(arr.view(np.uint8).reshape(len(records), ROW_SAMPLING_BYTES).copy())


ROW_LIMITS_BYTES = 8      # sizeof(vh_row_limits)


def pack_row_limits(pairs):
    """[(min_new, max_new), ...] -> a HOST uint8 tensor (n, ROW_LIMITS_BYTES) in the layout of vh_row_limits
    (include/valle_hip.h): two little-endian int32 per decode row, min_new at byte 0, max_new at 4; 0 switches a bound off."""
    import numpy as np
    arr = np.zeros((len(pairs), 2), dtype='<i4')
    for i, pair in enumerate(pairs):
        if len(pair) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 2 ** 31 for v in pair):
            raise ValueError(f'pack_row_limits: record {i} is {pair!r} ((min_new, max_new), ints in [0, 2**31))')
        arr[i] = pair
    return torch.from_numpy(arr.view(np.uint8).reshape(len(pairs), ROW_LIMITS_BYTES).copy())


POLL_NONE = -(1 << 30)           # vh_decode_groups_poll: a maximum over no rows


def _i32_dev(t, n, what):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_cuda:
        raise _lib.VhError(f'{what} must be an int32 device tensor of {n} entries')
    return ptr(t)


def decode_groups_poll(codes, cache_len, audio_pos, pos_base, eos, beams, max_new, out):
    """vh_decode_groups_poll into ONE int32 device tensor `out` of 4 + 2 G entries (one small read per poll): the four maxima
    (cache_len and audio_pos over all rows, then over the rows of groups that are not done; POLL_NONE over no rows),
    group_done (G), group_steps (G).  codes (B, width) int64, G = B // beams."""
    B, width = codes.shape
    if beams < 1 or B % beams:
        raise _lib.VhError(f'decode_groups_poll: {B} rows are not a multiple of beams={beams}')
    G = B // beams
    if codes.dtype != torch.int64 or codes.stride(1) != 1:
        raise _lib.VhError('decode_groups_poll: codes must be int64 rows')
    _i32_dev(out, 4 + 2 * G, 'decode_groups_poll: out')
    check(_lib.lib().vh_decode_groups_poll(
        codes.data_ptr(), codes.stride(0), width, _i32_dev(cache_len, B, 'decode_groups_poll: cache_len'),
        _i32_dev(audio_pos, B, 'decode_groups_poll: audio_pos'), _i32_dev(pos_base, B, 'decode_groups_poll: pos_base'),
        int(eos), B, int(beams), int(max_new), out[4:4 + G].data_ptr(), out[4 + G:].data_ptr(), out.data_ptr(), stream()),
        'vh_decode_groups_poll')
    return out


def decode_group_reset(codes, group, beams, prompt, prefix_len, bos, eos, cache_len, audio_pos, pos_base, sum_logprobs,
                       prefix_lens):
    """vh_decode_group_reset on rows group * beams .. of codes (B, width) int64.  prompt: int64 device tensor of the new
    utterance's first-codebook ids (the row becomes BOS + prompt, EOS beyond; prefix_len = text + BOS + prompt keys), or None to
    PARK the group (prefix_lens[group] = 0, the rows rewound to a fresh row that holds EOS)."""
    B, width = codes.shape
    if beams < 1 or B % beams:
        raise _lib.VhError(f'decode_group_reset: {B} rows are not a multiple of beams={beams}')
    if codes.dtype != torch.int64 or codes.stride(1) != 1:
        raise _lib.VhError('decode_group_reset: codes must be int64 rows')
    if prompt is not None and (prompt.dtype != torch.int64 or prompt.dim() != 1 or not prompt.is_cuda or not prompt.is_contiguous()):
        raise _lib.VhError('decode_group_reset: prompt must be a 1-D int64 device tensor')
    if sum_logprobs.dtype != torch.float32 or sum_logprobs.numel() != B:
        raise _lib.VhError('decode_group_reset: sum_logprobs must be float32 (B)')
    prompt_len = 0 if prompt is None else prompt.numel() + 1
    check(_lib.lib().vh_decode_group_reset(
        codes.data_ptr(), codes.stride(0), width, ptr(prompt) if prompt is not None and prompt.numel() else None, prompt_len,
        int(prefix_len) if prompt is not None else 0, int(bos), int(eos), int(group), B, int(beams),
        _i32_dev(cache_len, B, 'decode_group_reset: cache_len'), _i32_dev(audio_pos, B, 'decode_group_reset: audio_pos'),
        _i32_dev(pos_base, B, 'decode_group_reset: pos_base'), ptr(sum_logprobs),
        _i32_dev(prefix_lens, B // beams, 'decode_group_reset: prefix_lens'), stream()), 'vh_decode_group_reset')


def pad32(n):
    return (n + 31) // 32 * 32


_TAIL_WS = {}
_BWD_WS = {}


def _stream_ws(pool, device, need, floor=1 << 20):
    """A float32 workspace of >= need bytes owned by (device, current stream): grown when too small, kept otherwise."""
    key = (device.index, stream())
    ws = pool.get(key)
    if ws is None or ws.numel() * 4 < need:
        if len(pool) >= 8 and key not in pool:       # streams come and go: keep the most recent few
            torch.cuda.synchronize(device)           # (rare: nothing in flight may still be using the one let go)
            pool.pop(next(iter(pool)))
        # (the buffer let go was allocated on this stream and only ever used by launches of this stream: torch's caching
        # allocator hands its block to later work of the same stream only, so no wait is needed before it is replaced)
        ws = pool[key] = torch.empty(max(need, floor) // 4, device=device, dtype=torch.float32)
    return ws


def _tail_ws(device, stream_handle, M, N, K):
    """Workspace of vh_linear_ex's tail split (K slices of the tiles beyond the last multiple of 256; <= 16 MiB), one per
    (device, stream): launches of one stream run in order, so they can share it."""
    need = _lib.lib().vh_linear_ex_ws_bytes(M, N, K)
    if not need:
        return None
    key = (device.index, stream_handle)
    ws = _TAIL_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        if len(_TAIL_WS) >= 8:                       # streams come and go: keep the most recent few (16 MiB each)
            torch.cuda.synchronize(device)           # (rare: nothing in flight may still be writing the one let go)
            _TAIL_WS.pop(next(iter(_TAIL_WS)))
        ws = _TAIL_WS[key] = torch.empty(max(need, 1 << 24) // 4, device=device, dtype=torch.float32)
    return ws


def linear_ex(a, w, bias=None, residual=None, out=None, pre_out=None, act=ACT_NONE, K=None, colsum=None, drop=None):
    """vh_linear_ex: out = act(a @ w.T + bias) + residual on the tile kernels whatever M is, with the training
    epilogues (pre_out: also store the pre-activation; ACT_GELU_BWD: out = (a @ w.T) * gelu'(residual)).
    `K` overrides the contraction width (operands whose rows are zero-padded to a multiple of 32).
    colsum (N,) fp32, N % 128 == 0: += the column sums of `out` (a bias gradient) in the same launch.
    drop: a dropout.spec — out = dropout(act(a @ w.T + bias)) + residual, field indexed by (row, column) of `out`."""
    M = a.shape[0]
    N = w.shape[0]
    K = K or a.shape[1]
    if a.stride(1) != 1 or w.stride(1) != 1 or a.stride(0) < K:
        raise _lib.VhError('linear_ex: operands must be row-major and cover K')
    if w.stride(0) != K:
        raise _lib.VhError(f'linear_ex: the weight rows must be exactly K={K} wide (stride {w.stride(0)})')
    if out is None:
        out = torch.empty(M, (N + 3) // 4 * 4, device=a.device, dtype=torch.float32)[:, :N]
    for t, name in ((residual, 'residual'), (pre_out, 'pre_out'), (out, 'out')):
        if t is not None and (tuple(t.shape) != (M, N) or t.stride(1) != 1):
            raise _lib.VhError(f'linear_ex: {name} must be a row-major ({M},{N}) tensor')
    st = stream()
    ws = _tail_ws(a.device, st, M, N, K)
    check(_lib.lib().vh_linear_ex(
        _dev_f32(a, 'a'), a.stride(0), _dev_f32(w, 'w'), ptr(bias),
        _dev_f32(residual, 'residual') if residual is not None else None,
        residual.stride(0) if residual is not None else 0, _dev_f32(out, 'out'), out.stride(0),
        _dev_f32(pre_out, 'pre_out') if pre_out is not None else None,
        pre_out.stride(0) if pre_out is not None else 0, ptr(colsum), M, N, K, act, _drop_ref(drop), ptr(ws),
        ws.numel() * 4 if ws is not None else 0, st), 'vh_linear_ex')
    return out


def transpose(w, ldo=None, out=None):
    """out (cols, ldo) = w (rows, cols)^T, rows zero-padded up to ldo (default: rows rounded up to 32)."""
    rows, cols = w.shape
    ldo = ldo or pad32(rows)
    if out is None:
        out = torch.empty(cols, ldo, device=w.device, dtype=torch.float32)
    if w.stride(1) != 1 or tuple(out.shape) != (cols, ldo) or not out.is_contiguous():
        raise _lib.VhError('transpose: w must be row-major and out a contiguous (cols, ldo) tensor')
    check(_lib.lib().vh_transpose(_dev_f32(w, 'w'), w.stride(0), rows, cols, _dev_f32(out, 'out'), ldo, stream()),
          'vh_transpose')
    return out


class TransposePlan:
    """Transposed copies (cols, ldo) of a fixed set of weight matrices, refreshed by ONE launch (vh_transpose_many).
    The weights must stay where they are (parameters re-homed into FlatAdamW's flat buffer do; the plan is rebuilt by
    its owner when a data_ptr changes)."""

    def __init__(self, weights, ldos):
        import numpy as np
        dev = weights[0].device
        self.outs = [torch.empty(w.shape[1], ldo, device=dev, dtype=torch.float32) for w, ldo in zip(weights, ldos)]
        rec = np.zeros(len(weights), dtype=[('in', 'u8'), ('out', 'u8'), ('ldi', 'i4'), ('rows', 'i4'), ('cols', 'i4'),
                                            ('ldo', 'i4'), ('tile0', 'i4'), ('pad', 'i4')])
        tile = 0
        for i, (w, ldo, o) in enumerate(zip(weights, ldos, self.outs)):
            if w.dim() != 2 or w.stride(1) != 1 or w.dtype != torch.float32 or not w.is_cuda or ldo < w.shape[0]:
                raise _lib.VhError('TransposePlan: row-major fp32 device matrices, ldo >= rows')
            rec[i] = (w.data_ptr(), o.data_ptr(), w.stride(0), w.shape[0], w.shape[1], ldo, tile, 0)
            tile += -(-w.shape[1] // 32) * -(-ldo // 32)
        self.n, self.tiles = len(weights), tile
        self.key = tuple(w.data_ptr() for w in weights)
        self.items = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)

    def run(self):
        check(_lib.lib().vh_transpose_many(self.items.data_ptr(), self.n, self.tiles, stream()), 'vh_transpose_many')
        return self.outs


_tn_ws = {}


def gemm_tn(a, b, out=None):
    """out (NI, NJ) = a.T @ b for a (M, NI), b (M, NJ) stored token-major (dW = dY^T X), read in place."""
    M, NI = a.shape
    M2, NJ = b.shape
    if M != M2 or a.stride(1) != 1 or b.stride(1) != 1:
        raise _lib.VhError(f'gemm_tn: a {tuple(a.shape)} b {tuple(b.shape)}')
    if out is None:
        out = torch.empty(NI, (NJ + 3) // 4 * 4, device=a.device, dtype=torch.float32)[:, :NJ]
    if tuple(out.shape) != (NI, NJ) or out.stride(1) != 1:
        raise _lib.VhError('gemm_tn: out shape')
    need = _lib.lib().vh_gemm_tn_ws_bytes(M, NI, NJ)
    ws = _stream_ws(_tn_ws, a.device, need) if need else None     # one growing workspace per (device, stream)
    check(_lib.lib().vh_gemm_tn(_dev_f32(a, 'a'), a.stride(0), _dev_f32(b, 'b'), b.stride(0), _dev_f32(out, 'out'),
                                out.stride(0), M, NI, NJ, ptr(ws), ws.numel() * 4 if ws is not None else 0, stream()),
          'vh_gemm_tn')
    return out


def categorical_rows(logits, tokens, temperature=1.0, greedy=False, seed=0, stream_id=0, logprob=None):
    """tokens[r] ~ Categorical(logits[r] / temperature) (valle_nar.py:160) or arg-max when greedy.
    logits (R, V) row-major (any row stride); tokens: int64 (R,) view with any element stride."""
    R, V = logits.shape
    if logits.stride(1) != 1 or tokens.dtype != torch.int64 or tokens.dim() != 1 or tokens.shape[0] != R:
        raise _lib.VhError(f'categorical_rows: logits {tuple(logits.shape)} / tokens {tuple(tokens.shape)} {tokens.dtype}')
    if not tokens.is_cuda or (logprob is not None and (logprob.numel() != R or not logprob.is_contiguous())):
        raise _lib.VhError('categorical_rows: tokens / logprob must be device tensors of R entries')
    check(_lib.lib().vh_categorical_rows(_dev_f32(logits, 'logits'), logits.stride(0), V, R, float(temperature),
                                         int(bool(greedy)), int(seed) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF,
                                         tokens.data_ptr(), tokens.stride(0) if R > 1 else 1, ptr(logprob),
                                         stream()), 'vh_categorical_rows')
    return tokens


def categorical_rows_keyed(logits, tokens, requests, row_request, row_key, stream_id, logprob=None):
    """`vh_categorical_rows_keyed`: packed row r of logits (R, V) is frame row_key[r] of request row_request[r]; its draw is
    uniform01(seed of the request, frame, stream_id) under the request's temperature (its top_k == 1: the arg-max) and its
    token goes to tokens[request, frame].  tokens: an int64 device view (n_requests, n_keys) with any strides (a codebook
    column of the codes tensor); requests: the uint8 (n_requests, ROW_SAMPLING_BYTES) device tensor of `pack_row_sampling`;
    row_request / row_key: int32 device tensors of R entries."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < 1:
        raise _lib.VhError(f'categorical_rows_keyed: logits {tuple(logits.shape)} must be (R, V) rows with unit stride')
    R, V = logits.shape
    if tokens.dtype != torch.int64 or tokens.dim() != 2 or not tokens.is_cuda or 0 in tokens.shape:
        raise _lib.VhError(f'categorical_rows_keyed: tokens must be an int64 device view (n_requests, n_keys), got '
                           f'{tuple(tokens.shape)} {tokens.dtype}')
    n_requests, n_keys = tokens.shape
    if requests.dtype != torch.uint8 or tuple(requests.shape) != (n_requests, ROW_SAMPLING_BYTES) or not requests.is_cuda:
        raise _lib.VhError(f'categorical_rows_keyed: requests must be a uint8 device tensor ({n_requests}, '
                           f'{ROW_SAMPLING_BYTES}), got {tuple(requests.shape)} {requests.dtype}')
    if logprob is not None and (logprob.dtype != torch.float32 or logprob.numel() != R or not logprob.is_contiguous()):
        raise _lib.VhError('categorical_rows_keyed: logprob must be a contiguous fp32 device tensor of R entries')
    if R == 0:
        return tokens
    check(_lib.lib().vh_categorical_rows_keyed(
        _dev_f32(logits, 'logits'), logits.stride(0) if R > 1 else V, V, R, ptr(requests), n_requests,
        _i32_dev(row_request, R, 'categorical_rows_keyed: row_request'), _i32_dev(row_key, R, 'categorical_rows_keyed: row_key'),
        n_keys, int(stream_id) & 0xFFFFFFFF, tokens.data_ptr(), tokens.stride(0) if n_requests > 1 else 1,
        tokens.stride(1) if n_keys > 1 else 1, ptr(logprob), stream()), 'vh_categorical_rows_keyed')
    return tokens


def gemm(a, b, out, a_kmajor=False, b_kmajor=False):
    """out = op(a) @ op(b) through vh_gemm_batched.  a, b, out are 2-D (rows, cols) or 4-D
    (batch, heads, rows, cols) tensors / views with unit stride in the last dimension:
      a_kmajor=False: a is (M, K);  True: a is stored (K, M)   (the left operand transposed)
      b_kmajor=False: b is (N, K) as an nn.Linear weight;  True: b is stored (K, N)
    out is (M, N).  Strides are taken from the tensors, so permuted views are read in place."""
    def spec(t):
        if t.dim() == 2:
            return t.shape[0], t.shape[1], t.stride(0), 0, 0, 1, 1
        if t.dim() == 4:
            return t.shape[2], t.shape[3], t.stride(2), t.stride(0), t.stride(1), t.shape[0], t.shape[1]
        raise _lib.VhError('gemm: operands must be 2-D or 4-D')
    for t in (a, b, out):
        if t.stride(-1) != 1 or t.dtype != torch.float32:
            raise _lib.VhError('gemm: fp32 operands with unit stride in the last dimension required')
    ar, ac, lda, sab, sah, nb, nh = spec(a)
    br, bc, ldb, sbb, sbh, nb2, nh2 = spec(b)
    cr, cc, ldc, scb, sch, nb3, nh3 = spec(out)
    M, K = (ac, ar) if a_kmajor else (ar, ac)
    N, K2 = (bc, br) if b_kmajor else (br, bc)
    if K != K2 or (cr, cc) != (M, N) or (nb, nh) != (nb2, nh2) or (nb, nh) != (nb3, nh3):
        raise _lib.VhError(f'gemm: shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} out{tuple(out.shape)}')
    # few output tiles but a long K (weight gradients: K = every token of the batch): split K over
    # more workgroups; their partial tiles are summed into a zeroed `out` with fp32 atomics
    tiles = -(-M // 128) * -(-N // 128) * nb * nh
    splits = 1
    if tiles < 256 and K >= 2048:
        splits = max(1, min(32, 512 // tiles, K // 512))
    if splits > 1:
        out.zero_()
    check(_lib.lib().vh_gemm_batched(a.data_ptr(), lda, sab, sah, int(a_kmajor), b.data_ptr(), ldb, sbb, sbh,
                                     int(b_kmajor), out.data_ptr(), ldc, scb, sch, M, N, K, nb, nh, splits,
                                     stream()), 'vh_gemm_batched')
    return out


# ---- the EnCodec decoder's kernels (csrc/codec.hip): channels-last (B, T, C) fp32 activations ------------------------------
PAD_ZERO, PAD_REFLECT = 0, 1


def _codec_dense(t, name, shape=None):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.VhError(f'{name}: a contiguous fp32 HIP device tensor is required, got {t.dtype} on {t.device}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.VhError(f'{name}: shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t.data_ptr()


def rvq_decode(codes, codebooks, out=None):
    """vh_rvq_decode: codes (B, Q, T) int64, codebooks (n_books, K, D) -> (B, T, D) = the sum of the Q embeddings in codebook
    order.  An id outside [0, K) raises the device error flag (`_lib.raise_device_errors`) and is never read."""
    if codes.dim() != 3 or codes.dtype != torch.int64 or not codes.is_cuda:
        raise _lib.VhError(f'rvq_decode: codes must be a (B, Q, T) int64 HIP device tensor, got {tuple(codes.shape)} {codes.dtype}')
    codes = codes.contiguous()
    B, Q, T = codes.shape
    n_books, K, D = codebooks.shape
    if out is None:
        out = torch.empty(B, T, D, device=codes.device, dtype=torch.float32)
    check(_lib.lib().vh_rvq_decode(codes.data_ptr(), _codec_dense(codebooks, 'codebooks'), _codec_dense(out, 'out', (B, T, D)),
                                   B, Q, T, n_books, K, D, ptr(_lib.err_flag(codes.device)), stream()), 'vh_rvq_decode')
    return out


def conv1d_causal(x, w, bias=None, residual=None, dilation=1, pad_mode=PAD_REFLECT, elu=False, out=None, lens=None, len_scale=1):
    """vh_conv1d_causal: x (B, T, C_in), w (C_out, taps, C_in) -> (B, T, C_out) =
    bias + sum_k sum_ci act(xpad[b, t + k dilation, ci]) w[co, k, ci] (+ residual), left-padded per batch row.
    lens (B) device int32: batch row b holds lens[b] * len_scale valid rows, beyond which the reflect padding reads zero (a
    right-padded ragged batch then gives every utterance the bits it has alone)."""
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_cuda or lens.numel() != x.shape[0] or not lens.is_contiguous()):
        raise _lib.VhError('conv1d_causal: lens must be a contiguous device int32 tensor of B entries')
    if x.dim() != 3 or w.dim() != 3 or w.shape[2] != x.shape[2]:
        raise _lib.VhError(f'conv1d_causal: x {tuple(x.shape)} (B, T, C_in) against w {tuple(w.shape)} (C_out, taps, C_in)')
    B, T, C_in = x.shape
    C_out, taps, _ = w.shape
    if out is None:
        out = torch.empty(B, T, C_out, device=x.device, dtype=torch.float32)
    check(_lib.lib().vh_conv1d_causal(
        _codec_dense(x, 'x'), _codec_dense(w, 'w'), None if bias is None else _codec_dense(bias, 'bias', (C_out,)),
        None if residual is None else _codec_dense(residual, 'residual', (B, T, C_out)), _codec_dense(out, 'out', (B, T, C_out)),
        B, T, C_in, C_out, taps, int(dilation), int(pad_mode), int(bool(elu)), None if lens is None else lens.data_ptr(),
        int(len_scale), stream()), 'vh_conv1d_causal')
    return out


def lstm_layer(xproj, w_hh, skip=None):
    """vh_lstm_layer: xproj (B, T, 4 H) = W_ih x + b_ih + b_hh of every frame, w_hh (4 H, H) -> h (B, T, H), or h + skip when
    `skip` (B, T, H) is given.  Zero initial state, gate order i, f, g, o; one launch per time step."""
    if xproj.dim() != 3 or w_hh.dim() != 2 or xproj.shape[2] != w_hh.shape[0] or w_hh.shape[0] != 4 * w_hh.shape[1]:
        raise _lib.VhError(f'lstm_layer: xproj {tuple(xproj.shape)} (B, T, 4 H) against w_hh {tuple(w_hh.shape)} (4 H, H)')
    B, T, _ = xproj.shape
    H = w_hh.shape[1]
    h = torch.empty(B, T, H, device=xproj.device, dtype=torch.float32)
    c = torch.empty(B, H, device=xproj.device, dtype=torch.float32)
    y = None if skip is None else torch.empty_like(h)
    check(_lib.lib().vh_lstm_layer(_codec_dense(xproj, 'xproj'), _codec_dense(w_hh, 'w_hh'), h.data_ptr(), c.data_ptr(),
                                   None if skip is None else _codec_dense(skip, 'skip', (B, T, H)),
                                   None if y is None else y.data_ptr(), B, T, H, stream()), 'vh_lstm_layer')
    return h if skip is None else y


# ---- the EnCodec encoder's kernels (csrc/codec.hip) --------------------------------------------------------------------------
def _codec_lens(lens, B, name):
    if lens is None:
        return None
    if lens.dtype != torch.int32 or not lens.is_cuda or lens.numel() != B or not lens.is_contiguous():
        raise _lib.VhError(f'{name}: lens must be a contiguous device int32 tensor of B entries')
    return lens.data_ptr()


def conv1d_wave(x, w, bias=None, lens=None, out=None):
    """vh_conv1d_wave: x (B, L) samples, w (C_out, taps) -> (B, L, C_out) = bias + sum_k xpad[b, t + k] w[co, k], taps - 1 samples
    of left reflection per batch row; lens (B) device int32: a forward read beyond lens[b] samples reads zero."""
    if x.dim() != 2 or w.dim() != 2:
        raise _lib.VhError(f'conv1d_wave: x {tuple(x.shape)} (B, L) against w {tuple(w.shape)} (C_out, taps)')
    B, L = x.shape
    C_out, taps = w.shape
    if out is None:
        out = torch.empty(B, L, C_out, device=x.device, dtype=torch.float32)
    check(_lib.lib().vh_conv1d_wave(_codec_dense(x, 'x'), _codec_dense(w, 'w'),
                                    None if bias is None else _codec_dense(bias, 'bias', (C_out,)),
                                    _codec_dense(out, 'out', (B, L, C_out)), B, L, C_out, taps, _codec_lens(lens, B, 'conv1d_wave'),
                                    stream()), 'vh_conv1d_wave')
    return out


def conv1d_down(x, w, bias=None, stride=1, elu=False, lens=None, out=None):
    """vh_conv1d_down: x (B, T, C_in), w (C_out, taps, C_in) -> (B, ceil(T / stride), C_out), the strided causal convolution
    with the reference's left and right ("extra") reflect padding over every batch row's own lens[b] valid rows."""
    if x.dim() != 3 or w.dim() != 3 or w.shape[2] != x.shape[2]:
        raise _lib.VhError(f'conv1d_down: x {tuple(x.shape)} (B, T, C_in) against w {tuple(w.shape)} (C_out, taps, C_in)')
    B, T, C_in = x.shape
    C_out, taps, _ = w.shape
    stride = int(stride)
    T_out = -(-T // stride) if stride >= 1 else T
    if out is None:
        out = torch.empty(B, T_out, C_out, device=x.device, dtype=torch.float32)
    check(_lib.lib().vh_conv1d_down(_codec_dense(x, 'x'), _codec_dense(w, 'w'),
                                    None if bias is None else _codec_dense(bias, 'bias', (C_out,)),
                                    _codec_dense(out, 'out', (B, T_out, C_out)), B, T, C_in, C_out, taps, stride, int(bool(elu)),
                                    _codec_lens(lens, B, 'conv1d_down'), stream()), 'vh_conv1d_down')
    return out


def rvq_encode(x, codebooks, e_sq, num_codebooks=None):
    """vh_rvq_encode: x (B, T, D), codebooks (n_books, K, D), e_sq (n_books, K) = |entry|^2 -> codes (B, Q, T) int64, every
    stage in one launch (nearest entry, the lowest index of a tie; then the entry is subtracted in fp32)."""
    if x.dim() != 3 or codebooks.dim() != 3 or codebooks.shape[2] != x.shape[2]:
        raise _lib.VhError(f'rvq_encode: x {tuple(x.shape)} (B, T, D) against codebooks {tuple(codebooks.shape)} (n_books, K, D)')
    B, T, D = x.shape
    n_books, K, _ = codebooks.shape
    Q = n_books if num_codebooks is None else int(num_codebooks)
    codes = torch.empty(B, max(Q, 0), T, device=x.device, dtype=torch.int64)
    check(_lib.lib().vh_rvq_encode(_codec_dense(x, 'x'), _codec_dense(codebooks, 'codebooks'), _codec_dense(e_sq, 'e_sq', (n_books, K)),
                                   codes.data_ptr(), B, T, D, Q, n_books, K, stream()), 'vh_rvq_encode')
    return codes
