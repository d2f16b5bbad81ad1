"""Golden outputs of KV-cached generation at d_model 768 and 640 (12 and 10 heads of width 64), written by the REAL
reference on CPU.

    python tests/golden/gen_golden_base_d_model.py      (writes tests/golden/base_d_model.npz)

Runs only where the reference tree exists (see gen_golden.py); a no-op anywhere else.  Inputs are the seeded builders of
`base_d_model_inputs` below (valle2_amd.synth, regenerated on both sides); the file stores outputs only: greedy tokens,
the per-step top-1 / top-2 margin of beam 0 and the step count for two models:
  d768: 2 layers, d_model 768 / 12 heads / dff 3072 (the "base" size: the folded-LayerNorm GEMMs at PW = 6, the fused
        FeedForward at 32 hidden columns per workgroup), 2 beams, 48 new tokens;
  d640: 2 layers, d_model 640 / 10 heads / dff 1296 (a multiple of 16 and not of 32: the fused FeedForward at 16 hidden
        columns per workgroup), 2 beams, 40 new tokens.
The seeds are chosen so that every step's margin is at least MIN_MARGIN = 2e-3, ten times the logit tolerance of the GPU
test (2e-4): the token comparison then excludes no step.  For d768 at least three quarters of the steps are also decided by
more than PERF_MARGIN = 0.15, ten times the perf-mode logit bound of the fp16 build (1.5e-2): the perf-mode test compares
its tokens on those steps (d768's weights are drawn at std 0.03 for that: at 0.02 a third of the steps are that clear).  main() asserts both on the reference's own logits.
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

MIN_MARGIN = 2e-3
PERF_MARGIN = 0.15
BASE = {
    'd768': dict(d_model=768, n_heads=12, dim_feedforward=3072, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                 top_k=1, max_audio_len=48),
    'd640': dict(d_model=640, n_heads=10, dim_feedforward=1296, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                 top_k=1, max_audio_len=40),
}
BASE_SEED = {'d768': 82, 'd640': 93}                                           # state dict
BASE_STD = {'d768': 0.03, 'd640': 0.02}                                      # its weight scale (synth.make_state_dict)
BASE_UTT = {'d768': (10, 8, 30, 82000), 'd640': (9, 7, 26, 93000)}                # text a, text b, prompt frames, seed


def base_d_model_inputs(which):
    """(config kwargs, state dict, utterance) of fixture model `which` ('d768' | 'd640')."""
    from valle2_amd import synth
    kw = BASE[which]
    cfg = cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=BASE_SEED[which], rich=True, std=BASE_STD[which]), cfg)
    ta, tb, frames, seed = BASE_UTT[which]
    utt = synth.synth_utterance(cfg, ta, tb, frames, seed=seed)
    return kw, sd, utt


def _ref_generate(ref, which):
    import torch
    kw, sd, utt = base_d_model_inputs(which)
    cfg = cfg_of(kw, ref['config'].ConfigValle)
    m = ref['ar'].ValleAR(cfg).eval()
    m.load_state_dict(sd)
    assert cfg.d_model == 64 * cfg.n_heads and cfg.d_model in (640, 768)
    rows = []
    hook = m.proj.register_forward_hook(lambda mod, i, o: rows.append(o[:, -1].clone()))
    torch.manual_seed(0)
    tokens = m.generate(*utt)
    hook.remove()
    top2 = torch.topk(torch.stack(rows)[:, 0], 2, dim=-1)[0]
    margin = top2[:, 0] - top2[:, 1]
    assert float(margin.min()) >= MIN_MARGIN, f'{which}: a step of margin {float(margin.min()):.2e} < {MIN_MARGIN}: pick other seeds'
    assert len(rows) == kw['max_audio_len'], f'{which}: {len(rows)} steps: pick seeds without an early EOS'
    sure = float((margin > PERF_MARGIN).float().mean())
    assert which != 'd768' or sure >= 0.75, f'{which}: only {sure:.2f} of the steps exceed {PERF_MARGIN}: pick other seeds'
    return {f'tokens_{which}': tokens, f'margin_{which}': margin, f'steps_{which}': torch.tensor(len(rows))}


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
    for which in BASE:
        out.update(_ref_generate(ref, which))
    path = HERE / 'base_d_model.npz'
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f'wrote {path.name} ({path.stat().st_size} B) keys={sorted(out)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
