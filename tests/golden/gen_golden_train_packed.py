"""Golden outputs of PACKED AR training (ValleAR.training_step_packed), written by the REAL reference on CPU.

    python tests/golden/gen_golden_train_packed.py      (writes tests/golden/ar_train_packed.npz)

Runs only where the reference tree exists (see gen_golden.py); a no-op anywhere else.  Packed training of a batch is the
reference's own training_step on each utterance ALONE (B = 1, nothing padded), the per-utterance losses combined
token-weighted — so the fixture is that: for each of the four utterances of `train_packed_inputs` as a B = 1 batch, the
loss and every parameter's gradient.  Inputs are seeded builders (valle2_amd.synth, regenerated on both sides); the file
stores outputs only.

Model: 2 layers, 128-d, 2 heads, dff 256, LayerNorm, dropout 0 and PositionalEncoding dropout 0 (the reference's p = 0.1
there is set to 0 on the module: a fixture of the dropout-free arithmetic).  Utterances: 5 / 8 / 4 text tokens with 12 /
20 / 10 audio positions (BOS included), and one of 40 text tokens with 230 audio positions — 270 rows, a segment that
crosses a 256-key chunk of the attention backward.

Size: the model has 0.56 M parameters, four full gradients would be 9 MB.  Per utterance and parameter the file keeps the
gradient's norm (float64 accumulation of the float32 gradient) and the gradient itself at the flat indices
`sample_index(numel)`: all of it up to SAMPLE elements, else SAMPLE elements at a fixed odd stride (rows and columns both
walk).  Whoever compares a full gradient does so against the float64 oracle, which the CPU test pins to these samples.
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

KW = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='LayerNorm')
MODEL_SEED, DATA_SEED = 61, 6100
TEXT_LENS = [5, 8, 4, 40]
AUDIO_LENS = [12, 20, 10, 230]          # codes_lens: BOS + first-codebook tokens (= target tokens + EOS)
SAMPLE = 2048


def sample_index(numel):
    """The flat indices of a gradient the fixture keeps (a torch int64 tensor)."""
    import torch
    if numel <= SAMPLE:
        return torch.arange(numel)
    stride = numel // SAMPLE
    stride -= 1 - stride % 2 if stride > 1 else 0          # odd, and (SAMPLE - 1) * stride < numel
    return torch.arange(SAMPLE) * stride


def train_packed_inputs():
    """(config kwargs, state dict, collated batch of the four utterances) — the batch in the collate wire format
    (valle/collate.py:23-44): codes = BOS + first codebook, target = first codebook + EOS, zero padded, plus *_lens."""
    import torch
    from valle2_amd import synth
    cfg = cfg_of(KW)
    sd = synth.make_state_dict(cfg, 'ValleAR', seed=MODEL_SEED, rich=True)
    g = torch.Generator(device='cpu').manual_seed(DATA_SEED)
    n = len(TEXT_LENS)
    tokens = torch.zeros(n, max(TEXT_LENS), dtype=torch.int64)
    codes = torch.zeros(n, max(AUDIO_LENS), dtype=torch.int64)
    target = torch.zeros(n, max(AUDIO_LENS), dtype=torch.int64)
    for b, (tl, cl) in enumerate(zip(TEXT_LENS, AUDIO_LENS)):
        tokens[b, :tl] = torch.randint(0, cfg.vocab_size, (tl,), generator=g)
        first = torch.randint(0, cfg.num_audio_tokens, (cl - 1,), generator=g)
        codes[b, 0] = cfg.bos_token
        codes[b, 1:cl] = first
        target[b, :cl - 1] = first
        target[b, cl - 1] = cfg.eos_token
    batch = {'codes': codes, 'codes_lens': torch.tensor(AUDIO_LENS), 'target': target, 'tokens': tokens,
             'tokens_lens': torch.tensor(TEXT_LENS)}
    return KW, sd, batch


def utterance_batch(batch, b):
    """Utterance b of a collated batch alone, as a B = 1 batch with nothing padded."""
    tl, cl = int(batch['tokens_lens'][b]), int(batch['codes_lens'][b])
    return {'tokens': batch['tokens'][b:b + 1, :tl].clone(), 'tokens_lens': batch['tokens_lens'][b:b + 1].clone(),
            'codes': batch['codes'][b:b + 1, :cl].clone(), 'codes_lens': batch['codes_lens'][b:b + 1].clone(),
            'target': batch['target'][b:b + 1, :cl].clone()}


def param_names(sd):
    return sorted(k for k in sd if not k.endswith('.pe'))


def _ref_train_packed(ref):
    import torch
    kw, sd, batch = train_packed_inputs()
    cfg = cfg_of(kw, ref['config'].ConfigValle)
    out = {}
    for b in range(len(TEXT_LENS)):
        with torch.enable_grad():
            m = ref['ar'].ValleAR(cfg).train()
            m.load_state_dict(sd)
            m.tokens_position_emb.dropout.p = 0.0
            m.audio_position_emb.dropout.p = 0.0
            loss = m.training_step(utterance_batch(batch, b))
            loss.backward()
            grads = {n: p.grad.detach() for n, p in m.named_parameters()}
        names = param_names(sd)
        assert sorted(grads) == names, sorted(set(grads) ^ set(names))
        out[f'loss_{b}'] = loss.detach()
        out[f'grad_norms_{b}'] = torch.stack([grads[n].double().norm() for n in names])
        out[f'grad_samples_{b}'] = torch.cat([grads[n].reshape(-1)[sample_index(grads[n].numel())] for n in names])
    return out


def main():
    if not REF.exists():
        print('no reference tree here: nothing to do')
        return 0
    os.chdir(tempfile.mkdtemp(prefix='golden_cwd_'))
    import numpy as np
    import torch
    torch.manual_seed(0)
    ref = import_reference()
    out = _ref_train_packed(ref)
    path = HERE / 'ar_train_packed.npz'
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f'wrote {path.name} ({path.stat().st_size} B) keys={sorted(out)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
