"""ValleAR.training_step (rows padded to the longest) against ValleAR.training_step_packed (rows back to back, no padding),
forward + backward, in ONE process, same model, same batches: configs[3]'s AR model (12L / d_model 512 / 8 heads / dff 2048,
LayerNorm), B = 16, dropout as configured (0.1, PositionalEncoding 0.1: training mode).  Three sets of row lengths (text +
audio positions per utterance; a quarter of each is text):

  equal    every utterance 1024                  (nothing to save: the packed form may only cost here)
  spread   evenly spread over 256 .. 1024
  mix      4 utterances of 256 to every one of 1024

Both forms are warm (two untimed steps each per set), the timed steps alternate padded / packed, and every figure is the median
over --reps repetitions of the wall time between two device synchronisations around loss + backward, with the spread
(max - min) beside it.  The two steps compute DIFFERENT losses on a ragged batch (training_step averages over padded positions
and lets every row see text padding; the packed step is the per-utterance loss, token-weighted), so the report gives ms per step
beside the rows each form computes; on `equal` the two losses coincide and are printed.

    python tools/ab_train_packed.py [--batch 16] [--reps 7] [--max-len 1024]   (one JSON line per set)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def length_sets(n, lmax):
    lo = lmax // 4
    return {'equal': [lmax] * n,
            'spread': [lo + (i * (lmax - lo)) // max(1, n - 1) for i in range(n)],
            'mix': [lmax if i % 5 == 4 else lo for i in range(n)]}


def make_batch(cfg, lengths, seed):
    """A collated AR batch (valle2_amd.synth.synth_ar_batch's format) whose utterance b has lengths[b] rows: a quarter text."""
    import torch
    g = torch.Generator().manual_seed(seed)
    tl = [n // 4 for n in lengths]
    cl = [n - t for n, t in zip(lengths, tl)]                 # BOS + first-codebook tokens
    B = len(lengths)
    tokens = torch.zeros(B, max(tl), dtype=torch.int64)
    codes = torch.zeros(B, max(cl), dtype=torch.int64)
    target = torch.zeros(B, max(cl), dtype=torch.int64)
    for b in range(B):
        tokens[b, :tl[b]] = torch.randint(0, cfg.vocab_size, (tl[b],), generator=g)
        first = torch.randint(0, cfg.num_audio_tokens, (cl[b] - 1,), generator=g)
        codes[b, 0] = cfg.bos_token
        codes[b, 1:cl[b]] = first
        target[b, :cl[b] - 1] = first
        target[b, cl[b] - 1] = cfg.eos_token
    return {'codes': codes, 'codes_lens': torch.tensor(cl), 'target': target, 'tokens': tokens, 'tokens_lens': torch.tensor(tl)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=1024)
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_train_packed_'))    # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, get_model_class, synth
    assert torch.cuda.is_available(), 'ab_train_packed.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'
    cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, norm='LayerNorm')
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 'ValleAR', seed=5, rich=True))
    m = m.to(dev).train()

    def step(fn, batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.zero_grad(set_to_none=True)
        loss = fn(batch)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.detach())

    for name, lengths in length_sets(args.batch, args.max_len).items():
        batch = make_batch(cfg, lengths, 9100)
        batch = {k: (v if k.endswith('_lens') else v.to(dev)) for k, v in batch.items()}
        forms = {'padded': m.training_step, 'packed': m.training_step_packed}
        losses = {}
        for k, fn in forms.items():                          # warm-up of every shape the timed steps use
            for _ in range(2):
                losses[k] = step(fn, batch)[1]
        ms = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():                      # alternate the two forms
                ms[k].append(step(fn, batch)[0])
        tx, ty = max(n // 4 for n in lengths), max(n - n // 4 for n in lengths)
        padded_rows, total = (tx + ty) * len(lengths), sum(lengths)
        report = dict(set=name, batch=len(lengths), reps=args.reps, rows_padded=padded_rows, rows_packed=total,
                      row_share=round(total / padded_rows, 3),
                      score_share=round(sum(n * n for n in lengths) / ((tx + ty) ** 2 * len(lengths)), 3),
                      loss_padded=round(losses['padded'], 5), loss_packed=round(losses['packed'], 5))
        for k, v in ms.items():
            med = statistics.median(v)
            report[k] = dict(wall_ms_median=round(med, 2), wall_ms_spread=round(max(v) - min(v), 2), wall_ms=[round(x, 2) for x in v],
                             us_per_row=round(med * 1e3 / (padded_rows if k == 'padded' else total), 3))
        report['packed_over_padded'] = round(report['packed']['wall_ms_median'] / report['padded']['wall_ms_median'], 3)
        print(json.dumps(report), flush=True)


if __name__ == '__main__':
    main()
