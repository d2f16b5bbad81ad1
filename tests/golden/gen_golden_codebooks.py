"""Golden outputs for more than 8 codebooks and for audio vocabularies wider than 2048, written by the REAL reference on CPU.

    python tests/golden/gen_golden_codebooks.py      (writes tests/golden/codebooks.npz)

Runs only where the reference tree exists (see gen_golden.py); a no-op anywhere else.  Inputs are the seeded builders below
(valle2_amd.synth, regenerated on both sides); the file stores outputs only:
  q16 / q32: a 2-layer, d_model 128 / 2-head AdaLN ValleNAR with 16 / 32 codebooks (EnCodec at 12 / 24 kbps) and 128 audio
             tokens: `_prepare_audio_codes` (every PREP_STRIDE-th column) and the stage logits built from the reference's
             modules, at stages 1, 9, 15 (Q = 16) and 8, 31 (Q = 32).  From stage 9 on, the target frames sum more than 8
             tables; the prompt frames always sum all Q;
  v4096:     a 2-layer ValleAR with num_audio_tokens = 4096 (V = 4097 with EOS): greedy generate() tokens and per-step
             top-1 / top-2 margins of beam 0;
  filter:    the reference's top_k_top_p_filtering at V = 4097 for (top_k, top_p, temperature) in WIDE_FILTERS: the support
             (its finite entries) and the log_softmax row the returned log-prob is gathered from.
"""
from __future__ import annotations

import os
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from tests.golden.cases import cfg_of  # noqa: E402
from tests.golden.gen_golden import REF, import_reference  # noqa: E402

NAR_Q = {
    'q16': dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='AdaptiveLayerNorm',
                num_quantizers=16, num_audio_tokens=128),
    'q32': dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='AdaptiveLayerNorm',
                num_quantizers=32, num_audio_tokens=128),
}
NAR_Q_STAGES = {'q16': (1, 9, 15), 'q32': (8, 31)}
NAR_Q_SEEDS = {'q16': (71, 72), 'q32': (73, 74)}          # state dict, batch
NAR_Q_BATCH = dict(batch=2, n_tokens=8, n_frames=15)      # prefix 5 frames, 10 target frames
PREP_STRIDE = 4

AR_V4096 = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                top_k=1, max_audio_len=24, num_audio_tokens=4096)
AR_V4096_UTT = (10, 8, 30, 4096)                          # text a, text b, prompt frames, seed

WIDE_V = 4097
WIDE_FILTERS = [(50, 1.0, 1.0), (50, 0.9, 0.8), (0, 0.8, 1.0)]   # (top_k, tok_p, temperature)


def nar_q_inputs(which):
    """(config kwargs, state dict, batch) of the NAR fixture model `which` ('q16' | 'q32')."""
    from valle2_amd import synth
    kw = NAR_Q[which]
    cfg = cfg_of(kw)
    s_sd, s_b = NAR_Q_SEEDS[which]
    sd = synth.make_state_dict(cfg, 'ValleNAR', seed=s_sd, rich=True)
    batch = synth.synth_nar_batch(cfg, NAR_Q_BATCH['batch'], n_tokens=NAR_Q_BATCH['n_tokens'],
                                  n_frames=NAR_Q_BATCH['n_frames'], seed=s_b)
    return kw, sd, batch


def ar_v4096_inputs():
    """(config kwargs, state dict, utterance) of the AR fixture model with 4096 audio tokens (EOS silenced)."""
    from valle2_amd import synth
    cfg = cfg_of(AR_V4096)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=79, rich=True), cfg)
    ta, tb, frames, seed = AR_V4096_UTT
    return AR_V4096, sd, synth.synth_utterance(cfg, ta, tb, frames, seed=seed)


def wide_sampling_inputs():
    """(3, 4097) head rows: spread scores, one exact tie at the 50th place of row 0."""
    import torch
    logits = 3.0 * torch.randn((3, WIDE_V), generator=torch.Generator().manual_seed(83))
    srt = torch.sort(logits[0], descending=True).values
    logits[0, 11] = srt[49]
    return logits


def _ref_nar_q(ref, which):
    import torch
    kw, sd, batch = nar_q_inputs(which)
    cfg = cfg_of(kw, ref['config'].ConfigValle)
    m = ref['nar'].ValleNAR(cfg).eval()
    m.load_state_dict(sd)
    out = {}
    tx = int(batch['tokens_lens'].max())
    tok = m.tokens_position_emb(m.tokens_emb(batch['tokens']))
    for stage in NAR_Q_STAGES[which]:
        y, p = m._prepare_audio_codes(batch['codes'], stage)
        out[f'{which}_prep_{stage}'] = y[:, :, ::PREP_STRIDE]
        out[f'{which}_prefix_{stage}'] = torch.tensor(p)
        z, _ = m.transformer(torch.cat([tok, m.audio_position_emb(y)], dim=1), embedding=m.stage_embs[stage - 1].weight)
        out[f'{which}_logits_{stage}'] = m.proj_layers[stage - 1](z[:, tx + p:])
    return out


def _ref_ar_v4096(ref):
    import torch
    kw, sd, utt = ar_v4096_inputs()
    cfg = cfg_of(kw, ref['config'].ConfigValle)
    m = ref['ar'].ValleAR(cfg).eval()
    m.load_state_dict(sd)
    rows = []
    hook = m.proj.register_forward_hook(lambda mod, i, o: rows.append(o[:, -1].clone()))
    torch.manual_seed(0)
    tokens = m.generate(*utt)
    hook.remove()
    top2 = torch.topk(torch.stack(rows)[:, 0], 2, dim=-1)[0]
    return {'v4096_tokens': tokens, 'v4096_margin': top2[:, 0] - top2[:, 1], 'v4096_steps': torch.tensor(len(rows))}


def _ref_wide_filter(ref):
    import torch
    import torch.nn.functional as F
    u = ref['utils']
    logits = wide_sampling_inputs()
    real = u.top_k_top_p_filtering
    out = {}
    for i, (k, p, temp) in enumerate(WIDE_FILTERS):
        seen = []

        def spy(lg, **kw):
            res = real(lg, **kw)
            seen.append(res.clone())
            return res
        u.top_k_top_p_filtering = spy
        try:
            torch.manual_seed(i)
            u.topk_sampling(logits.clone(), top_k=k, tok_p=p, temperature=temp)
        finally:
            u.top_k_top_p_filtering = real
        out[f'filter_keep_{i}'] = torch.isfinite(seen[0])
        out[f'filter_logprobs_{i}'] = F.log_softmax(seen[0], dim=-1)
    return out


def main():
    if not REF.exists():
        print('no reference tree here: nothing to do')
        return 0
    os.chdir(tempfile.mkdtemp(prefix='golden_cwd_'))
    import numpy as np
    import torch
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ref = import_reference()
    out = {}
    for which in NAR_Q:
        out.update(_ref_nar_q(ref, which))
    out.update(_ref_ar_v4096(ref))
    out.update(_ref_wide_filter(ref))
    path = HERE / 'codebooks.npz'
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f'wrote {path.name} ({path.stat().st_size} B) keys={sorted(out)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
