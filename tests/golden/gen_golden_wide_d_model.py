"""Golden outputs of KV-cached generation at d_model above 1024 (head width 64), written by the REAL reference on CPU.

    python tests/golden/gen_golden_wide_d_model.py      (writes tests/golden/wide_d_model.npz)

Runs only where the reference tree exists (see gen_golden.py); a no-op anywhere else.  Inputs are the seeded builders of
`wide_d_model_inputs` below (valle2_amd.synth, regenerated on both sides); the file stores outputs only: greedy tokens,
the per-step top-1 / top-2 margin of beam 0 and the step count for two models:
  d1536: 2 layers, d_model 1536 / 24 heads / dff 3072 (a multiple of 256: the wide folded-LayerNorm GEMMs of the decode
         step), 2 beams, 56 new tokens;
  d1152: 2 layers, d_model 1152 / 18 heads / dff 2304 (a multiple of 64 only: LayerNorm and the plain GEMMs as separate
         launches), 2 beams, 48 new tokens.
The seeds are chosen so that every step's margin is at least MIN_MARGIN = 2e-3, ten times the logit tolerance of the GPU
test (2e-4): the token comparison then excludes no step.  main() asserts it on the reference's own logits.
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
WIDE = {
    'd1536': dict(d_model=1536, n_heads=24, dim_feedforward=3072, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                  top_k=1, max_audio_len=56),
    'd1152': dict(d_model=1152, n_heads=18, dim_feedforward=2304, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                  top_k=1, max_audio_len=48),
}
WIDE_SEED = {'d1536': 71, 'd1152': 73}                                       # state dict
WIDE_UTT = {'d1536': (10, 8, 30, 5540), 'd1152': (9, 7, 26, 5153)}           # text a, text b, prompt frames, seed


def wide_d_model_inputs(which):
    """(config kwargs, state dict, utterance) of fixture model `which` ('d1536' | 'd1152')."""
    from valle2_amd import synth
    kw = WIDE[which]
    cfg = cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=WIDE_SEED[which], rich=True), cfg)
    ta, tb, frames, seed = WIDE_UTT[which]
    utt = synth.synth_utterance(cfg, ta, tb, frames, seed=seed)
    return kw, sd, utt


def _ref_generate(ref, which):
    import torch
    kw, sd, utt = wide_d_model_inputs(which)
    cfg = cfg_of(kw, ref['config'].ConfigValle)
    m = ref['ar'].ValleAR(cfg).eval()
    m.load_state_dict(sd)
    assert cfg.d_model == 64 * cfg.n_heads and cfg.d_model > 1024
    rows = []
    hook = m.proj.register_forward_hook(lambda mod, i, o: rows.append(o[:, -1].clone()))
    torch.manual_seed(0)
    tokens = m.generate(*utt)
    hook.remove()
    top2 = torch.topk(torch.stack(rows)[:, 0], 2, dim=-1)[0]
    margin = top2[:, 0] - top2[:, 1]
    assert float(margin.min()) >= MIN_MARGIN, f'{which}: a step of margin {float(margin.min()):.2e} < {MIN_MARGIN}: pick other seeds'
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
    for which in WIDE:
        out.update(_ref_generate(ref, which))
    path = HERE / 'wide_d_model.npz'
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f'wrote {path.name} ({path.stat().st_size} B) keys={sorted(out)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
