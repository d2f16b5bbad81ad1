"""Run oracle/ on the golden cases' inputs (same keys as tests/golden/cases.REFERENCE_RUNNERS)."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import valle_oracle as O
from tests.golden import cases as C

GOLDEN_DIR = C.__file__.rsplit('/', 1)[0]


def load_golden(name):
    with np.load(f'{GOLDEN_DIR}/{name}.npz') as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def masks():
    out = {'attn_5_5': O.build_attn_mask(5, 5), 'attn_3_7': O.build_attn_mask(3, 7),
           'pad_a': O.build_pad_mask(torch.tensor([5, 5, 5, 5])),
           'pad_b': O.build_pad_mask(torch.tensor([5, 4, 3, 2]))}
    for d, h, b, t in C.MHA_SHAPES[:2]:
        _, _, causal, pad = C.mha_inputs(d, h, b, t)
        out[f'merge_{d}'] = O.merge_masks(b, h, causal, pad)
    return out


def mha():
    out = {}
    for d, h, b, t in C.MHA_SHAPES:
        sd, x, causal, pad = C.mha_inputs(d, h, b, t)
        o, (k, v) = O.multi_head_attention(sd, '', x, h, attn_mask=causal, use_cache=True)
        o2, _ = O.multi_head_attention(sd, '', x, h, attn_mask=causal, padding_mask=pad)
        o3, _ = O.multi_head_attention(sd, '', x, h)
        xn = C._randn((b, 1, d), 300 + d)
        o4, (k4, _) = O.multi_head_attention(sd, '', xn, h, kv_cache=(k, v), use_cache=True)
        out.update({f'out_{d}': o, f'k_{d}': k, f'v_{d}': v, f'out_pad_{d}': o2,
                    f'out_nomask_{d}': o3, f'out_step_{d}': o4, f'k_step_{d}': k4})
    return out


def transformer():
    out = {}
    for norm in ('LayerNorm', 'AdaptiveLayerNorm'):
        kw, sd, x, xl, yl, pad, emb = C.transformer_inputs(norm)
        cfg = C.cfg_of(kw)
        mask = O.build_attn_mask(xl, yl)
        e = emb if norm != 'LayerNorm' else None
        y, kv = O.transformer(sd, '', x, cfg, padding_mask=pad, attn_mask=mask, embedding=e,
                              use_cache=True)
        yfull, _ = O.transformer(sd, '', x, cfg, embedding=e)
        xn = torch.cat([x, C._randn((x.shape[0], 1, x.shape[2]), 19)], dim=1)
        ystep, kv2 = O.transformer(sd, '', xn, cfg, attn_mask=mask, embedding=e, kv_cache=kv,
                                   use_cache=True)
        out.update({f'{norm}_y': y, f'{norm}_yfull': yfull, f'{norm}_ystep': ystep,
                    f'{norm}_k0': kv[0][0], f'{norm}_vlast': kv2[-1][1]})
    return out


def head_dim():
    out = {}
    for d, h, b, t in C.HD_MHA_SHAPES:
        sd, x, causal, pad = C.mha_inputs(d, h, b, t)
        o, (k, v) = O.multi_head_attention(sd, '', x, h, attn_mask=causal, use_cache=True)
        o2, _ = O.multi_head_attention(sd, '', x, h, attn_mask=causal, padding_mask=pad)
        xn = C._randn((b, 1, d), 300 + d)
        o4, (k4, _) = O.multi_head_attention(sd, '', xn, h, kv_cache=(k, v), use_cache=True)
        out.update({f'out_{d}': o, f'k_{d}': k, f'out_pad_{d}': o2, f'out_step_{d}': o4, f'k_step_{d}': k4})
    kw, sd, utt, batch = C.head_dim_inputs()
    cfg = C.cfg_of(kw)
    trace = {}
    out['tokens'] = O.ar_generate(sd, cfg, *utt, trace=trace)
    out['margin'] = torch.tensor(trace['margin'])
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    with torch.enable_grad():
        loss = O.ar_training_loss(params, cfg, batch)
        loss.backward()
    names = sorted(k for k in params if not k.endswith('.pe'))
    out.update({'loss': loss.detach(), 'grad_norms': torch.stack([params[n].grad.norm() for n in names])})
    return out


def ar_train():
    kw, sd, batch = C.ar_train_inputs()
    cfg = C.cfg_of(kw)
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    with torch.enable_grad():
        loss = O.ar_training_loss(params, cfg, batch)
        loss.backward()
    names = sorted(k for k in params if not k.endswith('.pe'))
    return {'loss': loss.detach(),
            'grad_norms': torch.stack([params[n].grad.norm() for n in names])}


def ar_train_dropout():
    _, sd, batch = C.ar_train_inputs()
    cfg = C.cfg_of(C.AR_TINY_DROPOUT)
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    with torch.enable_grad():
        torch.manual_seed(C.DROPOUT_SEED)
        logits = O.ar_logits(params, cfg, batch, O.Dropout(cfg.dropout))
        loss = torch.nn.functional.cross_entropy(logits, batch['target'])
        loss.backward()
    names = sorted(k for k in params if not k.endswith('.pe'))
    return {'loss': loss.detach(), 'grad_norms': torch.stack([params[n].grad.norm() for n in names]),
            'logits': logits.detach().permute(0, 2, 1).contiguous()}


def transformer_dropout():
    out = {}
    for norm in ('LayerNorm', 'AdaptiveLayerNorm'):
        kw, sd, x, xl, yl, pad, emb = C.transformer_inputs(norm)
        cfg = C.cfg_of(dict(kw, dropout=0.1))
        torch.manual_seed(C.DROPOUT_SEED)
        y, _ = O.transformer(sd, '', x, cfg, padding_mask=pad, attn_mask=O.build_attn_mask(xl, yl),
                             embedding=emb if norm != 'LayerNorm' else None, drop=O.Dropout(cfg.dropout))
        out[f'{norm}_y'] = y
    return out


def _generate(kw, sd, utt):
    cfg = C.cfg_of(kw)
    trace = {}
    torch.manual_seed(0)
    tokens = O.ar_generate(sd, cfg, *utt, trace=trace)
    logits = torch.stack(trace['logits'])
    n = logits.shape[0]
    return {'tokens': tokens, 'margin': torch.tensor(trace['margin']),
            'logits_row0': logits[:, 0][:: max(1, n // 8)], 'steps': torch.tensor(n)}


def ar_generate_tiny():
    return _generate(*C.ar_generate_inputs('tiny'))


def ar_generate_mid():
    return _generate(*C.ar_generate_inputs('mid'))


def ar_generate_eos():
    gold = load_golden('ar_generate_eos')
    kw, sd, utt = C.ar_eos_inputs()
    torch.manual_seed(0)
    free = O.ar_generate(sd, C.cfg_of(kw), *utt)
    kw, sd, utt = C.ar_eos_inputs(gold['eos_row'])
    res = _generate(kw, sd, utt)
    return {'eos_row': gold['eos_row'], 'free_tokens': free, 'tokens': res['tokens'],
            'steps': res['steps']}


def nar():
    kw, sd, batch = C.nar_inputs()
    cfg = C.cfg_of(kw)
    out = {}
    for stage in (1, 4, 7):
        y, p = O.nar_prepare_audio_codes(sd, cfg, batch['codes'], stage)
        out[f'prep_{stage}'] = y
        out[f'prefix_{stage}'] = torch.tensor(p)
        out[f'logits_{stage}'] = O.nar_stage_logits(sd, cfg, batch, stage)[0]
    return out


def sampling():
    logits, x, lp = C.sampling_inputs()
    torch.manual_seed(0)
    tok, cur = O.topk_sampling(logits, top_k=1, tok_p=1.0, temperature=1.0)
    return {'greedy_tok': tok, 'greedy_lp': cur,
            'best_beam_1': O.get_best_beam(x, lp, 1024, 1.0),
            'best_beam_2': O.get_best_beam(x, lp, 1024, 0.0)}


def sampling_filter():
    logits, _, _ = C.sampling_inputs()
    out = {}
    for i, (k, p, temp) in enumerate(C.SAMPLING_FILTERS):
        filt = O._top_k_top_p_filter(logits / temp, top_k=k, top_p=p)
        out[f'keep_{i}'] = torch.isfinite(filt)
        out[f'logprobs_{i}'] = torch.log_softmax(filt, dim=-1)
        torch.manual_seed(i)
        out[f'tok_{i}'], out[f'lp_{i}'] = O.topk_sampling(logits.clone(), top_k=k, tok_p=p, temperature=temp)
    return out


ORACLE_FULL_STEPS = 20      # the oracle re-runs the first steps of the 512-step full-size golden (CPU time)


def ar_generate_full():
    kw, sd, utt = C.ar_generate_inputs('full')
    res = _generate(dict(kw, max_audio_len=ORACLE_FULL_STEPS), sd, utt)
    return {'tokens': res['tokens'], 'margin': res['margin']}


def ar_generate_big():
    """configs[4]'s AR leg (24L/1024d, 8 beams, 626-token prompt): the oracle re-runs the first steps of the 48."""
    kw, sd, utt = C.ar_generate_inputs('big')
    res = _generate(dict(kw, max_audio_len=4), sd, utt)
    return {'tokens': res['tokens'], 'margin': res['margin']}


def ar_prefill_full():
    kw, sd, text, codes, pos = C.ar_prefill_full_inputs()
    cfg = C.cfg_of(kw)
    tok = O.add_position(O.embed(sd['tokens_emb.word_embeddings.weight'], text), sd['tokens_position_emb.pe'])
    aud = O.add_position(O.embed(sd['audio_emb.word_embeddings.weight'], codes), sd['audio_position_emb.pe'])
    mask = O.build_attn_mask(text.shape[1], codes.shape[1])
    y, _ = O.transformer(sd, 'transformer.', torch.cat([tok, aud], dim=1), cfg, attn_mask=mask, use_cache=True)
    return {'logits': torch.nn.functional.linear(y[:, text.shape[1]:][:, pos], sd['proj.weight']),
            'hidden_last': y[:, -1]}


def ar_forced_big():
    """configs[4]'s AR leg, one teacher-forced pass over 400 text + 2475 audio positions (24L/1024d/h16)."""
    kw, sd, utt, forced = C.ar_forced_big_inputs()
    cfg = C.cfg_of(kw)
    text = torch.cat([utt[0], utt[2]])[None]
    codes = torch.cat([torch.tensor([cfg.bos_token]), utt[1][:, 0], forced[:-1]])[None]
    tok = O.add_position(O.embed(sd['tokens_emb.word_embeddings.weight'], text), sd['tokens_position_emb.pe'])
    aud = O.add_position(O.embed(sd['audio_emb.word_embeddings.weight'], codes), sd['audio_position_emb.pe'])
    mask = O.build_attn_mask(text.shape[1], codes.shape[1])
    y, _ = O.transformer(sd, 'transformer.', torch.cat([tok, aud], dim=1), cfg, attn_mask=mask)
    return {'logits': torch.nn.functional.linear(y[0, text.shape[1]:][list(C.FORCED_BIG_POS)], sd['proj.weight'])}


def ar_train_full():
    kw, sd, batch = C.ar_train_full_inputs()
    cfg = C.cfg_of(kw)
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    with torch.enable_grad():
        logits = O.ar_logits(params, cfg, batch)                       # (B, V, Ty)
        loss = torch.nn.functional.cross_entropy(logits, batch['target'])
        loss.backward()
    names = sorted(k for k in params if not k.endswith('.pe'))
    return {'loss': loss.detach(), 'grad_norms': torch.stack([params[n].grad.norm() for n in names]),
            'logits_sub': logits.detach().permute(0, 2, 1)[:, ::C.TRAIN_LOGIT_STRIDE].contiguous()}


def nar_big():
    kw, sd, batch = C.nar_big_inputs()
    cfg = C.cfg_of(kw)
    out = {}
    for stage in (2, 7):
        logits, p = O.nar_stage_logits(sd, cfg, batch, stage)
        out[f'logits_{stage}'] = logits[:, ::C.NAR_BIG_STRIDE].contiguous()
        out[f'prefix_{stage}'] = torch.tensor(p)
    return out


def nar_full():
    """configs[2] at full size: the oracle re-runs utterances 0 and 1 of the 64 (rows are independent in the NAR forward)."""
    kw, sd, batch = C.nar_full_inputs(rows=C.NAR_FULL_ROWS[:2])
    cfg = C.cfg_of(kw)
    logits, p = O.nar_stage_logits(sd, cfg, batch, C.NAR_FULL_STAGE)
    assert p == min(C.NAR_FULL_FRAMES // 3, 3 * cfg.quantization_factor)
    return {'logits': logits[:, ::C.NAR_FULL_STRIDE].contiguous()}


# golden keys that a runner reproduces only as a prefix (full-size cases trimmed for CPU time)
PREFIX_KEYS = {'ar_generate_full': ('tokens', 'margin'), 'ar_generate_big': ('tokens', 'margin'), 'nar_full': ('logits',)}

ORACLE_RUNNERS = {
    'sampling_filter': sampling_filter, 'ar_generate_full': ar_generate_full, 'ar_generate_big': ar_generate_big,
    'nar_full': nar_full, 'ar_forced_big': ar_forced_big,
    'ar_prefill_full': ar_prefill_full, 'ar_train_full': ar_train_full, 'nar_big': nar_big,
    'masks': masks, 'mha': mha, 'head_dim': head_dim, 'transformer': transformer, 'ar_train': ar_train,
    'ar_train_dropout': ar_train_dropout, 'transformer_dropout': transformer_dropout,
    'ar_generate_tiny': ar_generate_tiny, 'ar_generate_mid': ar_generate_mid,
    'ar_generate_eos': ar_generate_eos, 'nar': nar, 'sampling': sampling,
}


# ---- sampled decoding audited against the oracle ---------------------------------------------------------------------------
AUDIT_DELTA = 1e-4          # the suite's bound between device and oracle logits at these sizes (MARGIN in the grouped / queued tests)


class AuditError(AssertionError):
    """audit_sampled_rows found a token outside the oracle's support ('support: ...') or a score outside its interval
    ('score: ...')."""


AUDIT_MAX_NEW = 40         # rows reach max_new inside the second 32-step block
AUDIT_MODEL_SEED = 41
# (text a, text b, prompt frames) for synth.synth_utterance: contexts (text + BOS + prompt) of 20, 42, 64, 86 and 100 positions
AUDIT_UTTS = [(6, 5, 8), (9, 7, 25), (12, 9, 42), (15, 11, 59), (18, 13, 68)]


def _audit_model_table():
    from tests.golden.gen_golden_base_d_model import BASE
    from tests.golden.gen_golden_codebooks import AR_V4096
    from tests.golden.gen_golden_head_dim_decode import HD_DECODE
    from tests.golden.gen_golden_wide_d_model import WIDE
    # model -> (config, head scale, EOS row gain).  The scale brings the oracle's logit standard deviation at the prompts' last
    # positions to about 2.2 (as drawn it is 0.155, 0.37, 0.235, 0.515, 0.68, 0.97 and 0.16: measured on the CPU, float64).
    # The gain multiplies the EOS row once more: as drawn, the oracle's own sampling (top_k 50, 40 steps) ends one row in
    # seventy by EOS at d_model 128 and none at 768; with the gain, rows of one prompt end either way
    return {
        'd128': (C.AR_TINY, 14.0, 2.0),
        'd512': (dict(C.AR_MID, num_layers=2), 6.0, 2.0),
        'w128': (dict(HD_DECODE['w128'], num_layers=2), 9.4, 2.0),            # 256 / 2 heads: head width 128
        'd768': (BASE['d768'], 4.3, -2.0),                                    # the fast decode chain
        'd1152': (WIDE['d1152'], 3.2, 1.0),                                   # LayerNorm apart
        'd1536': (WIDE['d1536'], 2.25, 2.0),                                  # wide, LayerNorm folded
        'v4096': (AR_V4096, 13.7, 4.0),                                       # vh_sample_step_wide
    }


def audit_inputs(model):
    """(config kwargs, state dict, five utterances) of audit model `model`: 2 layers, synth.make_state_dict(rich=True), the
    head multiplied so that the next-token distributions are peaked — asserted here, on the CPU: the float64 oracle's logits at
    every prompt's last position have a standard deviation of 1.5 .. 3 (with the flat logits of std=0.02 every token scores
    about -log(50) under any history and an audit would see nothing).  The EOS row is not silenced; it carries a gain of its
    own on top (the table above), so that rows draw EOS within the 40 steps often enough for a case to audit rows that end
    either way."""
    from valle2_amd import synth
    kw, scale, eos_gain = _audit_model_table()[model]
    kw = dict(kw, max_audio_len=AUDIT_MAX_NEW, tok_p=1.0)
    assert kw['num_layers'] == 2
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleAR', seed=AUDIT_MODEL_SEED, rich=True)
    sd['proj.weight'] = sd['proj.weight'] * scale
    sd['proj.weight'][cfg.num_audio_tokens] *= eos_gain
    utts = [synth.synth_utterance(cfg, a, b, f, seed=2600 + i) for i, (a, b, f) in enumerate(AUDIT_UTTS)]
    for pt, pc, tt in utts:
        ctx = len(pt) + len(tt) + pc.shape[0] + 1
        std = head_logit_std(sd, cfg, torch.cat([pt, tt]), pc[:, 0])
        assert 20 <= ctx <= 100 and 1.5 <= std <= 3.0, f'inputs drifted: {model} context {ctx}, logit std {std:.3f}'
    return kw, sd, utts


def _forced_logits64(sd, cfg, text, codes_rows):
    """float64 oracle logits (n, T, V + 1) of rows teacher-forced through O.ar_logits: codes_rows is a list of 1-D id tensors
    (BOS first) over one text; shorter rows are padded (the mask is causal: a row's own positions do not see the pad)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    lens = torch.tensor([len(c) for c in codes_rows])
    codes = torch.zeros(len(codes_rows), int(lens.max()), dtype=torch.int64)
    for r, c in enumerate(codes_rows):
        codes[r, :len(c)] = c
    text = text.cpu().long()
    if text.dim() == 1:                                        # (2-D: a text of its own per row, equal lengths)
        text = text[None].repeat(len(codes_rows), 1)
    batch = {'tokens': text, 'tokens_lens': torch.full((len(codes_rows),), text.shape[1]), 'codes': codes, 'codes_lens': lens}
    with torch.no_grad():
        return O.ar_logits(sd64, cfg, batch).permute(0, 2, 1)


def head_logit_std(sd, cfg, text, prompt_first):
    """Standard deviation over the vocabulary of the float64 oracle's logits at the prompt's last position."""
    row = torch.cat([torch.tensor([cfg.num_audio_tokens + 1]), prompt_first.cpu().long()])
    return float(_forced_logits64(sd, cfg, text, [row])[0, -1].std())


def audit_sampled_rows(sd, cfg, text, rows, scores, prompt_len, max_new, top_k, tok_p, temperature, delta):
    """Audit sampled rows of ONE utterance against the float64 oracle, on the CPU.

    rows (n, width) int64: BOS, the prompt's first-codebook codes (prompt_len ids in all), what was generated, EOS padding;
    scores (n,): the decoder's sum_logprobs.  Each row is cut after its first generated EOS, or at prompt_len + max_new, and
    teacher-forced through O.ar_logits with the state dict in float64; the logits at audio position j are the distribution
    of token j + 1, so step s (token prompt_len + s) is read at position prompt_len - 1 + s.  Counted steps: up to and
    including the draw that produces EOS, nothing after it, nothing at or beyond max_new.

    support: at every counted step the token's scaled logit (logit / temperature) is at least the oracle's top_k-th largest
    scaled logit minus delta / temperature (top_k = 0: every token is in the support).  Top-p is not audited: tok_p = 1.0.
    score: the row's score lies in [sum(lo) - tol, sum(hi) + tol], lo / hi being the token's log-probability under the largest
    support consistent with delta (every logit >= kth - delta / T) and the smallest (every logit >= kth + delta / T, plus the
    token itself — and, top-k keeping at least k tokens, as many more at kth - delta / T as bring it to k members: without
    them the k-th token itself would be left out at every step and the interval would be its probability wide, per step);
    tol = 2 * delta / temperature * (counted steps): one delta on the token's logit and one on the log-sum-exp, per step.

    Returns one report per row: dict(steps, end ('eos' | 'cap'), lo, hi, tol, score, off (score minus the interval's
    midpoint)).  Raises AuditError naming the row, the step, the token, the oracle's k-th logit and the token's logit."""
    if tok_p != 1.0:
        raise ValueError('audit_sampled_rows: top-p support is not audited (tok_p must be 1.0)')
    eos, V = cfg.num_audio_tokens, cfg.num_audio_tokens + 1
    rows = torch.as_tensor(rows).cpu().long()
    scores = torch.as_tensor(scores).detach().cpu().double()
    n = rows.shape[0]
    if scores.shape != (n,):
        raise ValueError(f'audit_sampled_rows: {n} rows, scores of shape {tuple(scores.shape)}')
    counts, ends = [], []
    for r in range(n):
        gen = rows[r, prompt_len:prompt_len + max_new]
        hit = (gen == eos).nonzero()
        if hit.numel():
            counts.append(int(hit[0]) + 1)
            ends.append('eos')
        else:
            if gen.numel() < max_new:
                raise ValueError(f'audit_sampled_rows: row {r} holds {gen.numel()} generated tokens without an EOS, max_new={max_new}')
            counts.append(max_new)
            ends.append('cap')
    logits = _forced_logits64(sd, cfg, text, [rows[r, :prompt_len + counts[r] - 1] for r in range(n)])
    w = delta / temperature
    report = []
    for r in range(n):
        lo = hi = 0.0
        for s in range(counts[r]):
            x = logits[r, prompt_len - 1 + s] / temperature
            tok = int(rows[r, prompt_len + s])
            if not 0 <= tok < V:
                raise AuditError(f'support: row {r} step {s} token {tok}: not a token of the head (0..{V - 1})')
            if top_k > 0:
                k = min(top_k, V)
                kth = torch.topk(x, k)[0][-1]
                if x[tok] < kth - w:
                    raise AuditError(f'support: row {r} step {s} token {tok}: its scaled logit {float(x[tok]):.6f} is below the '
                                     f"oracle's {k}-th largest {float(kth):.6f} minus delta/T {w:.1e} (rank "
                                     f'{int((x > x[tok]).sum()) + 1} of {V})')
                big, small = x >= kth - w, x >= kth + w
                small[tok] = True
                lse_small = torch.logsumexp(x[small], 0)
                if int(small.sum()) < k:                                     # top-k keeps at least k tokens, each >= kth - w
                    lse_small = torch.logaddexp(lse_small, math.log(k - int(small.sum())) + kth - w)
                lo += float(x[tok] - torch.logsumexp(x[big], 0))
                hi += float(x[tok] - lse_small)
            else:
                lp = float(x[tok] - torch.logsumexp(x, 0))
                lo, hi = lo + lp, hi + lp
        tol = 2 * w * counts[r]
        got = float(scores[r])
        rep = dict(steps=counts[r], end=ends[r], lo=lo, hi=hi, tol=tol, score=got, off=got - 0.5 * (lo + hi))
        if not lo - tol <= got <= hi + tol:
            raise AuditError(f'score: row {r}: device score {got:.6f} outside [{lo - tol:.6f}, {hi + tol:.6f}] (the oracle over '
                             f'{counts[r]} counted steps, ended by {ends[r]}: lo {lo:.6f} hi {hi:.6f} tol {tol:.1e}; off the '
                             f'midpoint by {rep["off"]:+.6f})')
        report.append(rep)
    return report


# ---- the decode step over h16 weights (VALLE2_DECODE_W16) against a float64 mirror -----------------------------------------
# (tests/test_decode_w16_cpu.py, tests/test_decode_w16_gpu.py)
W16_ATOL, W16_RTOL = 2e-4, 1e-4     # the project's summation-order bound (tests/test_perf_mode_beams_gpu.py)
W16_POWER = 5                       # the mirror stands at least this many tolerances from the unrounded oracle
W16_STEPS = 7                       # forced tokens: the logits of step 0 are the prompt pass's, steps 1..6 are six decode steps
W16_FREE_STEPS = 24
W16_MAX_ROWS = 64
W16_MODEL_SEED = 77
# model -> (d_model, n_heads, dim_feedforward, text ids, prompt frames, head scale): contexts (text + BOS + prompt) of 20, 27, 33
# and 40 positions.  The scale brings the oracle's logit standard deviation at the prompts' ends to about 2.2 (as drawn:
# 0.160, 0.229, 0.362 and 0.631; float64, on the CPU).  'd128s32' is d128 with a dim_feedforward that takes 32-column slices.
W16_MODELS = {
    'd128': (128, 2, 528, 9, 10, 13.8),        # dim_feedforward % 32 != 0: slices of 16
    'd256': (256, 4, 1024, 14, 12, 9.7),
    'd512': (512, 8, 2048, 16, 16, 6.1),
    'd1024': (1024, 16, 2048, 20, 19, 3.5),
    'd128s32': (128, 2, 544, 9, 10, 13.5),     # ffn_decode_kernel<128, 32>: no model of the four reaches it
}


def w16_model_tol(h16):
    """What perf-mode logits may differ from the unrounded reference's: MODEL_TOL of tests/test_bf16_gpu.py."""
    return 1.5e-2 if h16 == torch.float16 else 5e-2


W16_FAULTS = ('swap_halves', 'no_residual', 'w2_shift8', 'eos_row_zero', 'c1_shift', 'k_late')


def w16_inputs(model):
    """(config kwargs, state dict, texts (64, T), firsts (64, F), forced (W16_STEPS,)) of w16 model `model`: two layers,
    LayerNorm, synth.make_state_dict(rich=True), the head scaled (asserted by the callers on the oracle's logits at the prompts'
    ends: standard deviation 1.5 .. 3).  Every row draws a text and a prompt of its own; a case of B rows takes the first B."""
    from valle2_amd import synth
    d, h, dff, T, F, scale = W16_MODELS[model]
    kw = dict(d_model=d, n_heads=h, dim_feedforward=dff, num_layers=2, dropout=0.0, norm='LayerNorm', top_k=1, tok_p=1.0,
              max_audio_len=W16_FREE_STEPS)
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleAR', seed=W16_MODEL_SEED, rich=True)
    sd['proj.weight'] = sd['proj.weight'] * scale
    gen = _g(7000 + d)
    texts = torch.randint(0, cfg.vocab_size, (W16_MAX_ROWS, T), generator=gen)
    firsts = torch.randint(0, cfg.num_audio_tokens, (W16_MAX_ROWS, F), generator=gen)
    forced = torch.randint(0, cfg.num_audio_tokens, (W16_STEPS,), generator=gen)
    assert len({tuple(r.tolist()) for r in texts}) == W16_MAX_ROWS and len({tuple(r.tolist()) for r in firsts}) == W16_MAX_ROWS
    assert 20 <= T + F + 1 <= 40
    return kw, sd, texts, firsts, forced


def w16_check_std(logits0, what=''):
    """The head's scale, as audit_inputs asserts it: the logits at every prompt's end have a standard deviation of 1.5 .. 3."""
    std = logits0.double().std(-1)
    assert 1.5 <= float(std.min()) and float(std.max()) <= 3.0, f'inputs drifted: {what} logit std {float(std.min()):.3f} .. {float(std.max()):.3f}'
    return std


def w16_oracle_logits(sd, cfg, texts, firsts, forced):
    """The unrounded float64 oracle's logits (B, len(forced), V + 1) at the steps of a forced decode: step t is read at audio
    position prompt_len - 1 + t of rows [BOS, prompt, forced[:-1]]."""
    bos = torch.tensor([cfg.num_audio_tokens + 1])
    pl = firsts.shape[1] + 1
    rows = [torch.cat([bos, f.long(), forced[:-1].long()]) for f in firsts]
    return _forced_logits64(sd, cfg, texts, rows)[:, pl - 1:pl - 1 + len(forced)]


def w16_distance(a, ref):
    """max |a - ref| / (atol + rtol |ref|): above 1, torch.testing.assert_close(a, ref, atol=W16_ATOL, rtol=W16_RTOL) fails."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float(((a - ref).abs() / (W16_ATOL + W16_RTOL * ref.abs())).max())


class W16Mirror:
    """What a perf_mode='kv' decode with h16 weights computes, restated in float64 from the state dict alone.

    Prompt pass: the float64 oracle with full-precision weights (O.transformer, use_cache=True); its K/V rounded once to h16.
    A step (include/valle_hip.h, "LayerNorm folded into the weights"): Wf = W * gamma as ONE fp32 multiply, rounded to h16;
    c1 = sum_k Wf16[n,k] from the ROUNDED matrix (engine.decode_weights16; c1='fold': from the unrounded fold, as the route was
    first built — what the row-offset case of tests/test_decode_w16_cpu.py measures) and c2 = sum_k beta[k] W[n,k] + b[n] from
    the unrounded fold (float64 sums rounded to fp32);
    the products rstd * (x Wf16^T - mean * c1) + c2 in float64; the new K/V rows rounded to h16 before they are attended; Wo,
    W2 and the head rounded to h16; exact-erf GELU; q and the residual stream never rounded.

    h16: torch.float16 | torch.bfloat16, or torch.float64 for "nothing rounded" (the fold in float64 too: the oracle itself).
    weights16=False: the matrices stay fp32 and only K/V are rounded — the fp32-weight perf_mode='kv' decoder.
    fault: one of W16_FAULTS planted (what the GPU comparison must be able to see).
    x_offset=(row, c): c added to every element of that row's step input (the residual stream keeps it; LayerNorm's mean is c
    off): `self.offset_ratio` is then the smallest |mean| / std over that row's LayerNorm inputs."""

    def __init__(self, sd, cfg, texts, firsts, h16, weights16=True, fault=None, x_offset=None, c1='rounded'):
        assert (fault is None or fault in W16_FAULTS) and c1 in ('rounded', 'fold'), (fault, c1)
        self.c1_rounded = c1 == 'rounded'
        self.cfg, self.h16, self.exact, self.fault, self.x_offset = cfg, h16, h16 == torch.float64, fault, x_offset
        self.w16 = weights16 and not self.exact
        self.sd = {k: v.double() for k, v in sd.items()}
        self.sd32 = sd
        self.offset_ratio = float('inf')
        texts, firsts = torch.as_tensor(texts).cpu().long(), torch.as_tensor(firsts).cpu().long()
        B, self.T = texts.shape
        self.pl = firsts.shape[1] + 1
        s = self.sd
        codes0 = torch.cat([torch.full((B, 1), cfg.num_audio_tokens + 1), firsts], dim=1)
        tok = O.add_position(O.embed(s['tokens_emb.word_embeddings.weight'], texts), s['tokens_position_emb.pe'])
        aud = O.add_position(O.embed(s['audio_emb.word_embeddings.weight'], codes0), s['audio_position_emb.pe'])
        with torch.no_grad():
            y, kv = O.transformer(s, 'transformer.', torch.cat([tok, aud], dim=1), cfg, attn_mask=O.build_attn_mask(self.T, self.pl),
                                  use_cache=True)
        self.logits0 = y[:, -1] @ s['proj.weight'].T                     # the prompt pass's head: full precision
        self.kv = [[self._round(k), self._round(v)] for k, v in kv]
        self.k_prev = [None] * cfg.num_layers                            # fault 'k_late'
        self.n_steps = 0
        self.layers = [self._layer_tables(i) for i in range(cfg.num_layers)]
        self.proj = self._matrix(s['proj.weight'], sd['proj.weight'])
        if fault == 'eos_row_zero':
            self.proj = self.proj.clone()
            self.proj[cfg.num_audio_tokens] = 0

    def _round(self, t):
        return t if self.exact else t.to(self.h16).double()

    def _matrix(self, w64, w32):
        return w32.float().to(self.h16).double() if self.w16 else w64

    def _fold(self, W, gamma, beta, bias):
        """(Wf as the step reads it, c1, c2) of `vh_ln_fold` + `decode_weights16`."""
        s64 = lambda k: self.sd[k]                                                                    # noqa: E731
        if self.exact:
            Wf = s64(W) * s64(gamma)
            Wq = Wf
        else:
            Wf32 = self.sd32[W].float() * self.sd32[gamma].float()
            Wf = Wf32.double()
            Wq = Wf32.to(self.h16).double() if self.w16 else Wf
        c1 = (Wq if self.c1_rounded else Wf).sum(1)
        c2 = (s64(W) * s64(beta)).sum(1) + (s64(bias) if bias is not None else 0)
        if not self.exact:
            c1, c2 = c1.float().double(), c2.float().double()
        if self.fault == 'c1_shift':
            c1 = torch.cat([c1[:1], c1[:-1]])
        return Wq, c1, c2

    def _layer_tables(self, i):
        p = f'transformer.layers.{i}.'
        qkv = self._fold(p + 'self_attn.qkv.weight', p + 'norm1.weight', p + 'norm1.bias', None)
        w1 = self._fold(p + 'ffn.linear_1.weight', p + 'norm2.weight', p + 'norm2.bias', p + 'ffn.linear_1.bias')
        if self.fault == 'swap_halves':
            Wq = qkv[0]
            qkv = (Wq.view(Wq.shape[0], -1, 2).flip(-1).reshape(Wq.shape),) + qkv[1:]
        wo = self._matrix(self.sd[p + 'self_attn.out.weight'], self.sd32[p + 'self_attn.out.weight'])
        w2 = self._matrix(self.sd[p + 'ffn.linear_2.weight'], self.sd32[p + 'ffn.linear_2.weight'])
        if self.fault == 'w2_shift8':
            w2 = w2.clone()
            w2[:, 8:16] = w2[:, 16:24]
        return dict(qkv=qkv, w1=w1, wo=wo, bo=self.sd[p + 'self_attn.out.bias'], w2=w2, b2=self.sd[p + 'ffn.linear_2.bias'])

    def _folded_linear(self, x, tab, row_stats):
        Wq, c1, c2 = tab
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        if row_stats is not None:
            self.offset_ratio = min(self.offset_ratio, float(mean[row_stats].abs() / var[row_stats].sqrt()))
        return (var + 1e-5).rsqrt() * (x @ Wq.T - mean * c1) + c2

    def step(self, tokens):
        """One decode step: `tokens` (B,) int64 (or one id for every row) are appended at the next audio position; returns the
        logits (B, V + 1) that follow them."""
        cfg, s = self.cfg, self.sd
        B, h = self.logits0.shape[0], cfg.n_heads
        tokens = torch.as_tensor(tokens).long().reshape(-1).expand(B)
        pos = self.pl + self.n_steps
        x = s['audio_emb.word_embeddings.weight'][tokens] + s['audio_position_emb.pe'][pos, 0]
        row = None
        if self.x_offset is not None:
            row = self.x_offset[0]
            x = x.clone()
            x[row] += self.x_offset[1]
        d = x.shape[1]
        hd = d // h
        for i, L in enumerate(self.layers):
            q, k, v = self._folded_linear(x, L['qkv'], row).chunk(3, dim=-1)
            k, v = (self._round(t).view(B, h, 1, hd) for t in (k, v))
            K, V = self.kv[i]
            k_seen = k
            if self.fault == 'k_late':                                   # this step's row lands one position on: the keys end
                k_seen = self.k_prev[i] if self.k_prev[i] is not None else torch.zeros_like(k)   # with what was there before
                self.k_prev[i] = k
            K_att = torch.cat([K, k_seen], dim=2)
            self.kv[i] = [torch.cat([K, k_seen], dim=2), torch.cat([V, v], dim=2)]
            V = self.kv[i][1]
            sc = (q.view(B, h, 1, hd) @ K_att.transpose(-1, -2)) / math.sqrt(hd)
            attn = (torch.softmax(sc, dim=-1) @ V).reshape(B, d)
            o = attn @ L['wo'].T + L['bo']
            x = o if self.fault == 'no_residual' else x + o
            hid = torch.nn.functional.gelu(self._folded_linear(x, L['w1'], row))
            x = x + hid @ L['w2'].T + L['b2']
        self.n_steps += 1
        return x @ self.proj.T


def w16_mirror_logits(sd, cfg, texts, firsts, forced, keep, h16, fault=None, weights16=True, x_offset=None, trace=None,
                      c1='rounded'):
    """Logits (B, len(keep), V + 1) of the W16Mirror teacher-forced as generation._decode_forced does it: forced[t] is appended
    after step t for every row, whatever the head said; the logits of step 0 are the prompt pass's.  trace (a dict) receives
    'offset_ratio'."""
    forced = torch.as_tensor(forced).cpu().long()
    with torch.no_grad():
        m = W16Mirror(sd, cfg, texts, firsts, h16, weights16=weights16, fault=fault, x_offset=x_offset, c1=c1)
        out = {0: m.logits0}
        for t in range(1, max(keep) + 1):
            out[t] = m.step(forced[t - 1])
    if trace is not None:
        trace['offset_ratio'] = m.offset_ratio
    return torch.stack([out[t] for t in keep], dim=1)


def w16_mirror_greedy(sd, cfg, texts, firsts, steps, h16):
    """(tokens, top-2 margins, top logits), each (B, steps), of the W16Mirror decoding greedily: a row that has drawn EOS keeps
    drawing it (valle_ar.py:166), so its tokens count up to and including the first EOS."""
    eos = cfg.num_audio_tokens
    with torch.no_grad():
        m = W16Mirror(sd, cfg, texts, firsts, h16)
        logits, toks, margins, tops = m.logits0, [], [], []
        for t in range(steps):
            top2 = torch.topk(logits, 2, dim=-1)
            tok = top2.indices[:, 0]
            if toks:
                tok = torch.where(toks[-1] == eos, torch.full_like(tok, eos), tok)
            toks.append(tok)
            margins.append(top2.values[:, 0] - top2.values[:, 1])
            tops.append(top2.values[:, 0])
            if t + 1 < steps:
                logits = m.step(tok)
    return torch.stack(toks, dim=1), torch.stack(margins, dim=1), torch.stack(tops, dim=1)


# ---- training at every width and row count (tests/test_train_widths_cpu.py, tests/test_train_widths_gpu.py) ----------------
# Whole models: (d_model, n_heads, dim_feedforward) of a two-layer model, and which models / NAR stages train at it.
TRAIN_WIDTHS = {
    'base': (768, 12, 3072),           # layernorm_bwd_kernel<4> with a masked last slot; the common size
    'd640': (640, 10, 1296),           # dff % 32 != 0: the node-by-node stack (LinearFn, GeluFn, vh_colsum) at head width 64
    'd896': (896, 14, 1792),           # <4> masked
    'odd_heads': (576, 9, 1152),       # 64 * n_heads is no multiple of 128
    'd1152': (1152, 18, 2304),         # <8> masked
    'd1536': (1536, 24, 3072),         # <8> under AdaptiveLayerNorm; adaproj K = 1536
    'd2048': (2048, 32, 2048),         # the upper bound of vh_layernorm_bwd / vh_adaproj_*
    'beyond': (2112, 33, 256),         # refused
}
TRAIN_WIDTH_RUNS = [('base', 'ValleAR', None), ('base', 'ValleNAR', 3), ('d640', 'ValleAR', None), ('d896', 'ValleAR', None),
                    ('odd_heads', 'ValleAR', None), ('odd_heads', 'ValleNAR', 2), ('d1152', 'ValleAR', None),
                    ('d1536', 'ValleNAR', 5), ('d2048', 'ValleAR', None), ('d2048', 'ValleNAR', 1)]


def train_width_inputs(case, model):
    """(config kwargs, state dict, batch) of whole-model case `case`: two layers, dropout 0, synth.make_state_dict(rich=True);
    AR: three rows of 5..12 text and 13..30 audio tokens (the size of cases.ar_train_inputs), NAR: three rows of 10 text
    tokens and 36 frames (cases.nar_inputs' lengths)."""
    from valle2_amd import synth
    d, h, dff = TRAIN_WIDTHS[case]
    kw = dict(d_model=d, n_heads=h, dim_feedforward=dff, num_layers=2, dropout=0.0,
              norm='LayerNorm' if model == 'ValleAR' else 'AdaptiveLayerNorm')
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, model, seed=300 + d, rich=True)
    if model == 'ValleAR':
        batch = synth.synth_ar_batch(cfg, 3, tok_range=(5, 12), code_range=(13, 30), seed=400 + d)
    else:
        batch = synth.synth_nar_batch(cfg, 3, n_tokens=10, n_frames=36, seed=400 + d)
    return kw, sd, batch


def oracle_training_loss(sd, cfg, batch, model, stage=None, dtype=torch.float64, grads=True):
    """(loss, params) of the oracle's training loss with the state dict cast to `dtype`; grads=True differentiates it by torch
    autograd (params[name].grad).  The oracle builds no floating-point constant of its own on this path (masks are bool, the
    position tables come from the state dict), so the cast of the state dict is the whole of the float64 form."""
    params = {k: v.to(dtype).clone().requires_grad_(grads and not k.endswith('.pe')) for k, v in sd.items()}
    with torch.set_grad_enabled(grads):
        loss = O.ar_training_loss(params, cfg, batch) if model == 'ValleAR' else O.nar_training_loss(params, cfg, batch, stage)
        if grads:
            loss.backward()
    assert loss.dtype == dtype
    return loss.detach(), params


# Row kernels.  Every reference below is plain torch in `dtype`: float64 is what the GPU tests compare against, float32 is the
# CPU companion's emulation of a kernel (the same arithmetic in the kernels' number format) — the measured error of the
# emulation against float64 is what the tolerances of the sums over rows rest on, and with one `fault` planted it is what
# the comparison helpers must reject.
SUM_MARGIN = 4              # a sum over rows on the GPU may be off by this many times the fp32 emulation's own error


def sum_rows(t):
    """Sum over dim 0.  float32: one row added after the other in fp32 (the plain order, fixed whatever the thread count:
    the error of a sum that promises no order, which is what the kernels' atomics give); float64: torch's sum."""
    if t.dtype == torch.float64:
        return t.sum(0)
    acc = torch.zeros_like(t[0])
    for r in range(t.shape[0]):
        acc += t[r]
    return acc


def _g(seed):
    return torch.Generator().manual_seed(seed)


def ln_inputs(rows, d, mean=0.3, dres=False):
    """Inputs of test_train_gpu.test_layernorm_backward (2 * randn + mean), fp32."""
    inp = dict(x=2 * torch.randn(rows, d, generator=_g(1)) + mean, gamma=1 + 0.1 * torch.randn(d, generator=_g(2)),
               beta=0.1 * torch.randn(d, generator=_g(3)), scale=1 + 0.2 * torch.randn(d, generator=_g(4)),
               shift=0.2 * torch.randn(d, generator=_g(5)), dy=torch.randn(rows, d, generator=_g(6)))
    if dres:
        inp['dres'] = torch.randn(rows, d, generator=_g(7))
    return inp


LN_WAVES = 2048             # waves of a vh_layernorm_bwd launch at >= 2048 rows (256 workgroups of 8): wave w owns rows w, w + 2048, ...


def ln_reference(inp, ada, dtype=torch.float64, fault=None, eps=1e-5):
    """y = s * (gamma * xhat + beta) + t and its backward under dy (+ dres added to dx, dcol = column sums of that dx), written
    out from the definition.  fault (fp32 emulations of a wrong kernel):
      'tail_unmasked'   the slot after the row's last 16-byte column group is read as data: the four floats that follow the
                        row in memory enter the sum its mean is made of
      'last_row'        rows >= LN_WAVES (a wave's second row) are never reached: dx stays as allocated (zero here), no sums
      'stale_ahead'     a wave's second row is computed from the operands of its first (the look-ahead never refilled)."""
    x, gamma, beta, dy = (inp[k].to(dtype) for k in ('x', 'gamma', 'beta', 'dy'))
    s, t = (inp['scale'].to(dtype), inp['shift'].to(dtype)) if ada else (None, None)
    dres = inp['dres'].to(dtype) if 'dres' in inp else None
    rows, d = x.shape
    if fault == 'stale_ahead':
        x, dy = x.clone(), dy.clone()
        x[LN_WAVES:], dy[LN_WAVES:] = x[:rows - LN_WAVES], dy[:rows - LN_WAVES]
        if dres is not None:
            dres = dres.clone()
            dres[LN_WAVES:] = dres[:rows - LN_WAVES]
    rsum = lambda m: m.sum(1, keepdim=True)                                                      # noqa: E731
    mu = rsum(x) / d
    if fault == 'tail_unmasked':
        after = torch.cat([x.reshape(-1), x.new_zeros(4)]).unfold(0, d + 4, d)[:, d:]           # (rows, 4): what follows each row
        mu = (rsum(x) + rsum(after)) / d
    v = x - mu
    rstd = (rsum(v * v) / d + eps).rsqrt()
    xhat = v * rstd
    u = gamma * xhat + beta
    du = dy * s if ada else dy
    g = du * gamma
    m1, m2 = rsum(g) / d, rsum(g * xhat) / d
    dx = (g - m1 - xhat * m2) * rstd
    if dres is not None:
        dx = dx + dres
    keep = slice(0, LN_WAVES) if fault == 'last_row' else slice(None)
    out = dict(y=s * u + t if ada else u, dgamma=sum_rows((du * xhat)[keep]), dbeta=sum_rows(du[keep]))
    if ada:
        out.update(dscale=sum_rows((dy * u)[keep]), dshift=sum_rows(dy[keep]))
    if fault == 'last_row':
        dx = dx.clone()
        dx[LN_WAVES:] = 0
    if dres is not None:
        out['dcol'] = sum_rows(dx[keep])
    out['dx'] = dx
    return out


LN_SUMS = ('dgamma', 'dbeta', 'dscale', 'dshift', 'dcol')


def ce_inputs(rows, V, ld=None, amp=None):
    """Logits (rows, V) of scale 2 as test_train_gpu.test_cross_entropy_forward_backward draws them — a column slice of a
    (rows, ld) buffer when ld is given; amp: uniform in [-amp, amp] instead, every row holding both ends — and targets."""
    buf = 2 * torch.randn(rows, ld or V, generator=_g(9))
    if amp is not None:
        buf = amp * (2 * torch.rand(rows, ld or V, generator=_g(9)) - 1)
        buf[:, 0], buf[:, V - 1] = amp, -amp
    return buf[:, :V], torch.randint(0, V, (rows,), generator=_g(10))


def ce_reference(logits, target, upstream, dtype=torch.float64, fault=None):
    """Mean cross entropy over the rows and d(upstream * loss) / d logits.  fault 'ld_for_V' (fp32 emulation): the row's
    maximum and log-sum-exp run over the buffer's ld columns."""
    rows, V = logits.shape
    lg = logits.to(dtype)
    wide = lg
    if fault == 'ld_for_V':
        wide = torch.as_strided(logits, (rows, logits.stride(0)), (logits.stride(0), 1)).to(dtype)
    lse = torch.logsumexp(wide, dim=1)
    per_row = lse - lg[torch.arange(rows), target]
    dl = torch.exp(lg - lse[:, None])
    dl[torch.arange(rows), target] -= 1
    return dict(loss=sum_rows(per_row / rows), dlogits=dl * (upstream / rows))


SOFTMAX_CASES = {       # (B, h, Tq, Tk, mode): the cases of vh_softmax_rows / vh_softmax_bwd
    'full': (2, 2, 5, 5, 'full'), 'prefix_rows': (2, 3, 70, 70, 'prefix'), 'prefix_tq_lt_tk': (1, 2, 33, 97, 'prefix'),
    'explicit_pad': (2, 2, 64, 129, 'explicit'), 'one_query': (3, 1, 1, 200, 'full'),
}
SOFTMAX_SCALE = 48 ** -0.5


def softmax_inputs(name):
    """Raw scores S and upstream dP (B, h, Tq, Tk) and the mask arguments of the case (CPU tensors: x_len / x_len_dev / kv_len
    int32, mask / pad uint8).  Every row keeps a visible key: kv_len >= 1, x_len >= 1, the diagonal unmasked and unpadded."""
    B, h, Tq, Tk, mode = SOFTMAX_CASES[name]
    S = 7 * torch.randn(B, h, Tq, Tk, generator=_g(50))                    # q . k at head width 48: standard deviation 7
    dP = torch.randn(B, h, Tq, Tk, generator=_g(51))
    spec = {}
    if name == 'prefix_rows':
        spec = dict(x_len_dev=torch.tensor([20, 35], dtype=torch.int32), kv_len=torch.tensor([70, 61], dtype=torch.int32))
    elif name == 'prefix_tq_lt_tk':
        spec = dict(x_len=70, kv_len=torch.tensor([90], dtype=torch.int32))          # queries on both sides of the prefix's end
    elif name == 'explicit_pad':
        mask = torch.rand(Tq, Tk, generator=_g(52)) < 0.3
        mask[torch.arange(Tq), Tk - Tq + torch.arange(Tq)] = False
        pad = torch.zeros(B, Tk, dtype=torch.bool)
        pad[1, 10:40] = True                                               # (the diagonal lies in columns 65 .. 128)
        spec = dict(mask=mask.to(torch.uint8), pad=pad.to(torch.uint8))
    elif name == 'one_query':
        spec = dict(kv_len=torch.tensor([200, 1, 77], dtype=torch.int32))
    return S, dP, mode, spec


def softmax_visible(name, spec, fault=None):
    """(B, 1, Tq, Tk) bool: the keys query i of batch row b sees — vh_attn_rows' rule (include/valle_hip.h), the query's
    position being Tk - Tq + i.  fault 'no_qpos' (emulation): the position taken for i."""
    B, h, Tq, Tk, mode = SOFTMAX_CASES[name]
    j = torch.arange(Tk)[None, None, :]
    i = torch.arange(Tq)[None, :, None]
    if mode == 'explicit':
        vis = ~spec['mask'].bool()[None] & ~spec['pad'].bool()[:, None, :]
    else:
        kvl = spec['kv_len'].long().clamp(max=Tk)[:, None, None] if 'kv_len' in spec else torch.full((B, 1, 1), Tk)
        vis = (j < kvl).expand(B, Tq, Tk)
        if mode == 'prefix':
            xl = spec['x_len_dev'].long()[:, None, None] if 'x_len_dev' in spec else torch.full((B, 1, 1), spec['x_len'])
            qpos = i if fault == 'no_qpos' else Tk - Tq + i
            vis = vis & ((j < xl) | ((qpos >= xl) & (j <= qpos)))
    return vis[:, None]


def softmax_reference(name, dtype=torch.float64, fault=None):
    """P = softmax(S * scale + mask) and dS = scale * P * (dP - sum(dP * P)) of the case."""
    S, dP, mode, spec = softmax_inputs(name)
    vis = softmax_visible(name, spec, fault)
    assert bool(softmax_visible(name, spec).any(-1).all()), 'a row without a visible key'
    P = torch.softmax((S.to(dtype) * SOFTMAX_SCALE).masked_fill(~vis, O.NEG_INF), dim=-1)
    dPd = dP.to(dtype)
    return dict(P=P, dS=SOFTMAX_SCALE * P * (dPd - (dPd * P).sum(-1, keepdim=True)))



def embed_inputs(d, T, B=3, vocab=40, J=3):
    """Ragged rows ending in a run of ONE id (test_train_gpu.test_embedding_backward_and_colsum): ids (B, T, J) int64 whose
    column slices are what the kernels read, J tables, upstream gradient for t0 + T positions."""
    tabs = [torch.randn(vocab, d, generator=_g(20 + j)) for j in range(J)]
    ids = torch.randint(0, vocab, (B, T, J), generator=_g(34))
    for b, n_real in enumerate((T, (T * 9) // 16, 1)[:B]):
        ids[b, n_real:] = vocab - 1
    return tabs, ids


def embed_table_grads(ids, dy, vocab, dtype=torch.float64):
    """d tables[j] = scatter-add of dy (B, T, d) over ids[..., j]: position after position in `dtype` (index_add_ walks the
    index in order)."""
    B, T, J = ids.shape
    flat = dy.to(dtype).reshape(B * T, -1)
    return [torch.zeros(vocab, flat.shape[1], dtype=dtype).index_add_(0, ids[..., j].reshape(-1), flat) for j in range(J)]


COLSUM_CASES = [(1, 4, 4), (63, 260, 260), (65, 768, 1000), (2053, 2048, 2048)]      # (rows, cols, ld)


def colsum_inputs(rows, cols, ld):
    buf = torch.randn(rows, ld, generator=_g(60))
    return buf[:, :cols], torch.randn(cols, generator=_g(61))          # x (a column slice), what `out` holds before the call


def colsum_reference(x, out0, dtype=torch.float64):
    return out0.to(dtype) + sum_rows(x.to(dtype).contiguous())


def worst(got, ref):
    """Largest absolute difference of `got` from the float64 reference."""
    return float((got.detach().cpu().double() - ref.detach().double()).abs().max())


def check_close(name, got, ref, atol=2e-5, rtol=1e-4):
    """A per-element quantity against float64 with the tolerances of tests/test_train_gpu.py; the failure names it."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    bad = ~((got - ref).abs() <= atol + rtol * ref.abs())              # (not <=: a NaN fails)
    assert not bool(bad.any()), f'{name}: {int(bad.sum())} of {bad.numel()} elements off, worst {worst(got, ref):.3e} (atol {atol:g} rtol {rtol:g})'


def check_sum(name, got, ref, measured):
    """A sum over rows against float64: at most SUM_MARGIN times the fp32 emulation's own measured error."""
    err = worst(got, ref)
    assert err <= SUM_MARGIN * measured, f'{name}: worst error {err:.3e} > {SUM_MARGIN} x {measured:.3e}'      # (a NaN fails)
    return err


def embed_reference(ids, dy, t0, vocab, dtype=torch.float64):
    """Table gradients of the embedding cases: t0 = 0, the J tables under dy (EmbedSumPeFn); t0 > 0, EmbedConcatFn's two parts —
    table 0 over the first t0 positions of ids[..., 0], then the J tables over all T positions at row offset t0."""
    grads = embed_table_grads(ids, dy[:, t0:], vocab, dtype)
    if t0:
        first = embed_table_grads(ids[:, :t0, :1], dy[:, :t0], vocab, dtype)[0]
        grads[0] = grads[0] + first if dtype == torch.float64 else grads[0].add_(first)
    return grads


def _collect(checks):
    """Run every check, then fail once, naming each quantity that failed (the CPU companion asserts on the names)."""
    failed = []
    for name, fn in checks:
        try:
            fn()
        except AssertionError as e:
            failed.append((name, str(e)))
    assert not failed, 'failed: ' + ', '.join(n for n, _ in failed) + ' | ' + ' | '.join(m for _, m in failed)


def check_ln(got, ref, measured):
    """LayerNorm backward results {dx, dgamma, dbeta[, dscale, dshift][, dcol]} against the float64 reference."""
    checks = [('dx', lambda: check_close('dx', got['dx'], ref['dx']))]
    checks += [(q, lambda q=q: check_sum(q, got[q], ref[q], measured[q])) for q in measured]
    if 'dcol' in measured:
        checks.append(('dcol_of_dx', lambda: check_sum('dcol against the columns of the dx written', got['dcol'],
                                                       got['dx'].detach().cpu().double().sum(0), measured['dcol'])))
    _collect(checks)


def check_ce(loss, dlogits, ref, rows):
    """Cross entropy.  The loss is a mean over rows: each row's term to test_train_gpu's rtol 1e-6 + atol 1e-6, plus the sum
    of `rows` non-negative fp32 terms in an order nobody fixes (a wave's rows, its workgroup, then one atomic per workgroup):
    the rounding errors of n additions, each at most 2^-24 of the running sum, add up like a random walk — sqrt(n) * 2^-24 *
    the sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2's rule of thumb: the worst-case n * u holds
    for no more than sqrt(n) * u in practice).  One scalar's measured fp32 error says nothing (at 8229 rows the plain fp32 sum
    happens to land 2e-8 from the float64 one), so this bound is worked out, not measured.  A row skipped moves the loss by
    1 / rows of itself: 20 times the allowance at 8229 rows.  dlogits per element at 1e-7 + 1e-4."""
    def loss_ok():
        err, tol = worst(loss, ref['loss']), 1e-6 + (1e-6 + rows ** 0.5 * 2.0 ** -24) * float(ref['loss'].abs())
        assert err <= tol, f'loss: error {err:.3e} > {tol:.3e}'
    _collect([('loss', loss_ok), ('dlogits', lambda: check_close('dlogits', dlogits, ref['dlogits'], atol=1e-7, rtol=1e-4))])


def check_softmax(P, dS, ref):
    _collect([('P', lambda: check_close('P', P, ref['P'])), ('dS', lambda: check_close('dS', dS, ref['dS']))])


# ---- many-row attention on every mask geometry (tests/test_attn_geometry_cpu.py, tests/test_attn_geometry_gpu.py) -----------
# name -> (B, h, Tq, Tk, mode).  What a case is for stands beside it; the per-row lengths are in ATTN_GEOMETRY_LENGTHS.  Block
# sizes of the kernels under test: 32-key tiles and 32-query waves, 64-key tiles (attn16), 128-query blocks, key chunks of
# attn_chunk_keys(T, n) <= 256 keys (the fused backward).  Tq < Tk cases are forward only (the backward is Tq == Tk).
ATTN_GEOMETRY_CASES = {
    'prefix_small': (4, 2, 100, 100, 'prefix'),      # T <= 128: one query block, one chunk; x_len 0, 1, T and above T
    'prefix_mid': (4, 2, 200, 200, 'prefix'),        # 129 .. 256: one chunk of 224 keys; kv_len ==, just above and below x_len
    'prefix_long': (4, 2, 600, 600, 'prefix'),       # > 512: three chunks of 224 (the last holds 152), five query blocks (88), a
                                                     # last tile of 24; the prefix ends on a chunk edge (224), inside chunks
    'prefix_512': (4, 2, 512, 512, 'prefix'),        # a multiple of 256: two full chunks, the prefix end on their edge; kv_len > Tk
    'prefix_scalar': (2, 1, 300, 300, 'prefix'),     # the host-side x_len (no x_len_dev) on a 32-key wave edge
    'full_small': (4, 2, 100, 100, 'full'),          # attn_bwd_fused_kernel<4> (one chunk of 128 keys); kv_len = 1
    'full_mid': (4, 2, 200, 200, 'full'),            # one chunk of 224 (<8>) or two of 128 (<4>)
    'full_long': (4, 2, 600, 600, 'full'),           # three to five chunks; kv_len > Tk, chunks that are all padding
    'full_512': (3, 1, 512, 512, 'full'),
    'explicit_shared': (2, 2, 300, 300, 'explicit'),         # one (Tq, Tk) mask + pad, forward and backward
    'explicit_bmask': (3, 2, 70, 150, 'explicit'),           # a (B, Tq, Tk) mask + pad: vh_attn_rows_bmask, forward only
    'prefix_tq_lt_tk': (4, 2, 150, 400, 'prefix'),           # q_off = 250 (no multiple of 32): queries on both sides of the prefix end
    'full_tq_lt_tk': (2, 2, 70, 333, 'full'),
    'empty_row_full': (3, 2, 300, 300, 'full'),              # a batch row with kv_len = 0 beside ordinary rows, slab path
    'empty_row_prefix': (4, 2, 300, 300, 'prefix'),
    'empty_row_small': (3, 2, 100, 100, 'prefix'),           # ... and where one chunk writes dQ itself (no slab, no reduce)
}
ATTN_GEOMETRY_LENGTHS = {       # per batch row: x_len_dev (prefix cases; an int = the host-side x_len) and kv_len
    'prefix_small': dict(x_len_dev=[0, 1, 100, 133], kv_len=[100, 1, 64, 33]),
    'prefix_mid': dict(x_len_dev=[31, 32, 33, 129], kv_len=[200, 32, 34, 128]),
    'prefix_long': dict(x_len_dev=[224, 257, 255, 127], kv_len=[600, 511, 256, 129]),
    'prefix_512': dict(x_len_dev=[256, 512, 64, 65], kv_len=[512, 257, 63, 700]),
    'prefix_scalar': dict(x_len=128, kv_len=[300, 127]),
    'full_small': dict(kv_len=[100, 1, 31, 65]),
    'full_mid': dict(kv_len=[200, 127, 128, 129]),
    'full_long': dict(kv_len=[900, 255, 449, 32]),
    'full_512': dict(kv_len=[512, 511, 385]),
    'explicit_shared': {}, 'explicit_bmask': {},
    'prefix_tq_lt_tk': dict(x_len_dev=[300, 285, 100, 401], kv_len=[400, 399, 320, 383]),
    'full_tq_lt_tk': dict(kv_len=[333, 193]),
    'empty_row_full': dict(kv_len=[300, 0, 191]),
    'empty_row_prefix': dict(x_len_dev=[63, 50, 128, 290], kv_len=[300, 0, 257, 192]),
    'empty_row_small': dict(x_len_dev=[40, 40, 96], kv_len=[100, 0, 97]),
}
ATTN_EMPTY_ROWS = {'empty_row_full': [1], 'empty_row_prefix': [1], 'empty_row_small': [1]}          # batch rows without a key (kv_len = 0)
ATTN_QUANTITIES = ('out', 'lse2', 'dq', 'dk', 'dv')
# (atol, rtol) per quantity: out from tests/test_kernels_gpu.py::test_attn_rows, the gradients from tests/test_train_gpu.py::
# test_attn_rows_bwd_vs_torch_autograd; lse2 has SUM_MARGIN times the fp32 emulation's measured error instead (the GPU file)
ATTN_TOL = {'out': (3e-5, 0.0), 'dq': (6e-5, 1e-4), 'dk': (6e-5, 1e-4), 'dv': (6e-5, 1e-4)}
ATTN_Q16_PRESCALE = 0.125 * 1.4426950408889634          # kernels.Q16_PRESCALE: what attn_rows_bf16 expects q multiplied by
ATTN_FAULTS = {       # fault -> (the case that must reject it, the quantities it must show on)
    'x_len_of_row0': ('prefix_mid', ('out', 'lse2', 'dq', 'dk', 'dv')),
    'causal_lt': ('prefix_long', ('out', 'lse2', 'dq', 'dk', 'dv')),
    'qpos_gt': ('prefix_long', ('out', 'lse2', 'dq', 'dk', 'dv')),
    'no_q_off': ('prefix_tq_lt_tk', ('out', 'lse2')),
    'kv_unclamped_pad_ignored': ('explicit_shared', ('out', 'lse2', 'dq', 'dk', 'dv')),
    'mask_of_row0': ('explicit_bmask', ('out', 'lse2')),
    'diag_tile_unmasked': ('prefix_long', ('out', 'lse2', 'dq', 'dk', 'dv')),
    'tile_skipped_by_first_query': ('prefix_tq_lt_tk', ('out', 'lse2')),
    'dq_chunk_lost': ('prefix_long', ('dq',)),
    'dq_chunk_extra': ('prefix_long', ('dq',)),
}


def attn_chunk_keys(T, n_chunks=None):
    """Keys per chunk of the fused backward when T keys are cut into n_chunks (default: the fewest, ceil(T / 256)): equal
    chunks of whole 32-key wave blocks (vh_attn_rows_bwd_ws)."""
    n = n_chunks or -(-T // 256)
    return (-(-T // n) + 31) // 32 * 32


def attn_geometry_inputs(name):
    """(q (B, h, Tq, 64), k, v (B, h, Tk, 64), dout (B, h, Tq, 64), mode, spec) of the case: seeded randn, so q . k / 8 has
    unit variance; spec holds the mask arguments as CPU tensors (x_len int / x_len_dev, kv_len int32; mask, pad uint8).  Every
    query keeps a visible key (kv_len >= 1; explicit: key 0 is never masked or padded) except the rows of ATTN_EMPTY_ROWS."""
    B, h, Tq, Tk, mode = ATTN_GEOMETRY_CASES[name]
    seed = 700 + 10 * list(ATTN_GEOMETRY_CASES).index(name)
    q, dout = (torch.randn(B, h, Tq, 64, generator=_g(seed + i)) for i in (0, 3))
    k, v = (torch.randn(B, h, Tk, 64, generator=_g(seed + i)) for i in (1, 2))
    spec = {key: (val if isinstance(val, int) else torch.tensor(val, dtype=torch.int32))
            for key, val in ATTN_GEOMETRY_LENGTHS[name].items()}
    if mode == 'explicit':
        per_row = name == 'explicit_bmask'
        mask = torch.rand((B, Tq, Tk) if per_row else (Tq, Tk), generator=_g(seed + 4)) < 0.3
        mask[..., 0] = False
        pad = torch.zeros(B, Tk, dtype=torch.bool)
        pad[1, 10:40] = True
        pad[1, Tk - 37:] = True
        pad[B - 1, 1:Tk:3] = True
        spec = dict(mask=mask.to(torch.uint8), pad=pad.to(torch.uint8))
    return q, k, v, dout, mode, spec


def attn_visible(name, spec, fault=None):
    """(B, Tq, Tk) bool: the keys query i of batch row b sees, written from the three lines of include/valle_hip.h
    (vh_attn_rows), the query's position being Tk - Tq + i.  fault: the visibility a wrong kernel would apply —
      'x_len_of_row0'   x_len_dev[0] for every batch row          'causal_lt'  key < qpos for key <= qpos
      'qpos_gt'         qpos > xl for qpos >= xl                   'no_q_off'   the query's position taken as i
      'kv_unclamped_pad_ignored'  explicit mode without pad        'mask_of_row0'  the mask's batch stride taken as 0
      'diag_tile_unmasked'  a wave (32 queries) takes a 32-key tile without the element mask when the tile's FIRST key, not
                        its last, is at or before the wave's first query (and the tile lies below kv_len, the wave past xl)
      'tile_skipped_by_first_query'  a wave skips the tiles that lie beyond its FIRST query, not its last."""
    B, h, Tq, Tk, mode = ATTN_GEOMETRY_CASES[name]
    q_off = Tk - Tq
    j = torch.arange(Tk)[None, None, :]
    i = torch.arange(Tq)[None, :, None]
    if mode == 'explicit':
        mask = spec['mask'].bool()
        mask = mask[None].expand(B, Tq, Tk) if mask.dim() == 2 else mask
        if fault == 'mask_of_row0':
            mask = mask[:1].expand(B, Tq, Tk)
        pad = torch.zeros_like(spec['pad']) if fault == 'kv_unclamped_pad_ignored' else spec['pad']
        return ~mask & ~pad.bool()[:, None, :]
    kvl = spec['kv_len'].long().clamp(max=Tk)
    vis = (j < kvl[:, None, None]).expand(B, Tq, Tk)
    if mode == 'full':
        return vis.clone()
    xl = spec['x_len_dev'].long() if 'x_len_dev' in spec else torch.full((B,), spec['x_len'])
    if fault == 'x_len_of_row0':
        xl = xl[:1].expand(B)
    x = xl[:, None, None]
    qpos = i if fault == 'no_q_off' else q_off + i
    past = qpos > x if fault == 'qpos_gt' else qpos >= x
    causal = j < qpos if fault == 'causal_lt' else j <= qpos
    vis = (vis & ((j < x) | (past & causal))).clone()
    if fault in ('diag_tile_unmasked', 'tile_skipped_by_first_query'):
        for b in range(B):
            for w0 in range(0, Tq, 32):                      # a wave's queries w0 .. w0 + 31, positions from wpos_min on
                wpos_min = q_off + w0
                for k0 in range(0, Tk, 32):
                    if fault == 'diag_tile_unmasked':
                        if k0 + 32 <= int(kvl[b]) and wpos_min >= int(xl[b]) and k0 <= wpos_min:
                            vis[b, w0:w0 + 32, k0:k0 + 32] = True
                    elif not (k0 < int(xl[b]) or (wpos_min >= int(xl[b]) and k0 <= wpos_min)):
                        vis[b, w0:w0 + 32, k0:k0 + 32] = False
    return vis


def attn_geometry_reference(name, dtype=torch.float64, fault=None, h16=None, operands=None):
    """out, lse2 (B, h, Tq) and — where Tq == Tk — dq, dk, dv of the case, written out from the definition in `dtype`
    (float64: what the GPU tests compare against; float32: the emulation of a kernel):
      P = softmax(q k^T / 8 + mask), lse2 = logsumexp / ln 2, out = P v, dV = P^T dO, dS = P o (dP - rowsum(dO o out)),
      dQ = dS k / 8, dK = dS^T q / 8.
    A batch row without a key (ATTN_EMPTY_ROWS) has P = 0: zero gradients; its out / lse2 are not compared.  h16: q (scaled
    by ATTN_Q16_PRESCALE first, as vh_linear_qkv_bf16 leaves it), k and v rounded to that 16-bit format before anything else.
    fault: one of attn_visible's, or in the chunk bookkeeping of the fused backward at the fewest chunks —
      'dq_chunk_lost'   dQ leaves out every key chunk that starts at or after x_len, whatever the query
      'dq_chunk_extra'  dQ adds a slab of ones for every chunk the fused kernel never wrote for the query (a chunk of
                        padding; under the prefix mask a chunk starting at or after x_len and after the query).
    operands: (q, k, v, dout) to take in place of the case's own, its masks kept (tests/attn_scores.py moves the scores)."""
    q, k, v, dout, mode, spec = attn_geometry_inputs(name)
    if operands is not None:
        q, k, v, dout = operands
    B, h, Tq, Tk, _ = ATTN_GEOMETRY_CASES[name]
    if h16 is not None:
        q = (q * ATTN_Q16_PRESCALE).to(h16).double() / ATTN_Q16_PRESCALE
        k, v = k.to(h16), v.to(h16)
    q, k, v, dout = (t.to(dtype) for t in (q, k, v, dout))
    chunk_fault = fault in ('dq_chunk_lost', 'dq_chunk_extra')
    vis = attn_visible(name, spec, None if chunk_fault else fault)[:, None]
    s = (q @ k.transpose(-1, -2) / 8).masked_fill(~vis, O.NEG_INF)
    lse = torch.logsumexp(s, dim=-1)
    P = torch.where(vis.any(-1, keepdim=True), torch.exp(s - lse[..., None]), torch.zeros((), dtype=dtype))
    out = P @ v
    res = dict(out=out, lse2=lse / math.log(2.0))
    if Tq != Tk:
        return res
    dP = dout @ v.transpose(-1, -2)
    dS = P * (dP - (dout * out).sum(-1, keepdim=True))
    res.update(dv=P.transpose(-1, -2) @ dout, dk=dS.transpose(-1, -2) @ q / 8)
    dS_q = dS
    if chunk_fault:
        ck = attn_chunk_keys(Tk)
        kb0 = (torch.arange(Tk) // ck * ck)[None, :]                          # first key of the chunk a key lies in
        xl = spec['x_len_dev'].long() if 'x_len_dev' in spec else torch.full((B,), spec.get('x_len', Tk))
        if fault == 'dq_chunk_lost':
            dS_q = dS * (kb0 < xl[:, None])[:, None, None, :].to(dtype)
    res['dq'] = dS_q @ k / 8
    if fault == 'dq_chunk_extra':
        kvl = spec['kv_len'].long().clamp(max=Tk)
        qi = torch.arange(Tq)[None, :]
        for c0 in range(0, Tk, ck):
            unwritten = (c0 >= kvl)[:, None] | ((c0 >= xl)[:, None] & (qi < c0) if mode == 'prefix' else False)
            res['dq'] = res['dq'] + 0.125 * unwritten[:, None, :, None].to(dtype)
    return res


def attn_kept_rows(name):
    """Batch rows whose out / lse2 are compared (all but ATTN_EMPTY_ROWS)."""
    return [b for b in range(ATTN_GEOMETRY_CASES[name][0]) if b not in ATTN_EMPTY_ROWS.get(name, [])]


def attn_miss(quantity, got, ref, lse2_measured=None):
    """How far `got` is from the float64 reference, in units of the tolerance the GPU file applies to the quantity: the largest
    |got - ref| / (atol + rtol |ref|) (lse2: / (SUM_MARGIN x the fp32 emulation's measured error)).  <= 1 passes; NaN -> inf."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, f'{quantity}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    if quantity == 'lse2':
        tol = torch.full_like(ref, SUM_MARGIN * lse2_measured)
    else:
        tol = ATTN_TOL[quantity][0] + ATTN_TOL[quantity][1] * ref.abs()
    ratio = ((got - ref).abs() / tol)
    return float(torch.nan_to_num(ratio, nan=float('inf')).max()) if ratio.numel() else 0.0


def check_attn(name, got, ref, lse2_measured, quantities=None):
    """The quantities of `got` (same layout as the reference's) against float64; out / lse2 on attn_kept_rows only, and the
    gradients of a row without a key exactly zero.  Fails once, naming every quantity that failed."""
    kept = attn_kept_rows(name)

    def one(qn):
        g_, r_ = got[qn], ref[qn]
        if qn in ('out', 'lse2'):
            g_, r_ = g_[kept], r_[kept]
        else:
            for b in ATTN_EMPTY_ROWS.get(name, []):
                assert float(g_[b].abs().max()) == 0.0, f'{qn}: row {b} has no key, its gradient must be exactly zero'
        m = attn_miss(qn, g_, r_, lse2_measured)
        assert m <= 1.0, f'{qn}: {m:.3g} x the tolerance (worst error {worst(g_, r_):.3e})'
    _collect([(qn, lambda qn=qn: one(qn)) for qn in (quantities or ATTN_QUANTITIES) if qn in ref and qn in got])
