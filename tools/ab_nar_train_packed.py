"""ValleNAR.training_step (rows padded to the longest) against ValleNAR.training_step_packed (rows back to back, no padding),
forward + backward, in ONE process, same model, same batches, one pinned stage: configs[3]'s NAR model (12L / d_model 512 / 8
heads / dff 2048, AdaptiveLayerNorm), B = 16, dropout as configured (0.1, PositionalEncoding 0.1: training mode).  The three
sets of row lengths of tools/ab_train_packed.py (text + frames per utterance; a quarter of each is text):

  equal    every utterance 1024                  (nothing to save: the packed form may only cost here)
  spread   evenly spread over 256 .. 1024
  mix      4 utterances of 256 to every one of 1024

Both forms are warm (two untimed steps each per set), the timed steps alternate padded / packed, and every figure is the median
over --reps repetitions of the wall time between two device synchronisations around loss + backward, with the spread
(max - min) beside it.  The two steps compute DIFFERENT losses on a ragged batch (training_step takes every utterance's
acoustic prefix from the padded width, attends padding keys and averages over padded frames; the packed step is the
per-utterance loss, each utterance with the prefix of its own length, token-weighted), so the report gives ms per step beside
the rows each form computes; on `equal` the two losses are the same quantity and are printed.

    python tools/ab_nar_train_packed.py [--batch 16] [--reps 7] [--max-len 1024] [--stage 4]   (one JSON line per set)

Under `rocprofv3 --kernel-trace --stats -- python tools/ab_nar_train_packed.py` the kernel table gives the input path of both
forms: embed_nar_packed_kernel + embed_nar_packed_bwd_kernel (one launch each per packed step) against embed_sum_pe_kernel +
embed_bwd_kernel (3 and 1 + Q + stage launches per padded step); `steps_per_form` in the last line is the divisor.
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

from tools.ab_train_packed import length_sets  # noqa: E402


def make_batch(cfg, lengths, seed):
    """A collated NAR batch (valle2_amd.synth.synth_nar_batch's format, zero padded) whose utterance b has lengths[b] rows: a
    quarter text, the rest frames of all Q codebooks."""
    import torch
    g = torch.Generator().manual_seed(seed)
    tl = [n // 4 for n in lengths]
    fl = [n - t for n, t in zip(lengths, tl)]
    B = len(lengths)
    tokens = torch.zeros(B, max(tl), dtype=torch.int64)
    codes = torch.zeros(B, max(fl), cfg.num_quantizers, dtype=torch.int64)
    for b in range(B):
        tokens[b, :tl[b]] = torch.randint(0, cfg.vocab_size, (tl[b],), generator=g)
        codes[b, :fl[b]] = torch.randint(0, cfg.num_audio_tokens, (fl[b], cfg.num_quantizers), generator=g)
    return {'codes': codes, 'codes_lens': torch.tensor(fl), 'tokens': tokens, 'tokens_lens': torch.tensor(tl)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=1024)
    ap.add_argument('--stage', type=int, default=4)
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_nar_train_packed_'))    # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, get_model_class, synth
    assert torch.cuda.is_available(), 'ab_nar_train_packed.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'
    cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, norm='AdaptiveLayerNorm')
    m = get_model_class('ValleNAR')(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 'ValleNAR', seed=5, rich=True))
    m = m.to(dev).train()

    def step(fn, batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.zero_grad(set_to_none=True)
        loss = fn(batch, stage=args.stage)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.detach())

    steps = 0
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
        steps += 2 + args.reps
        tx, ty = max(n // 4 for n in lengths), max(n - n // 4 for n in lengths)
        padded_rows, total = (tx + ty) * len(lengths), sum(lengths)
        report = dict(set=name, batch=len(lengths), reps=args.reps, stage=args.stage, rows_padded=padded_rows, rows_packed=total,
                      row_share=round(total / padded_rows, 3),
                      score_share=round(sum(n * n for n in lengths) / ((tx + ty) ** 2 * len(lengths)), 3),
                      loss_padded=round(losses['padded'], 5), loss_packed=round(losses['packed'], 5))
        for k, v in ms.items():
            med = statistics.median(v)
            report[k] = dict(wall_ms_median=round(med, 2), wall_ms_spread=round(max(v) - min(v), 2), wall_ms=[round(x, 2) for x in v],
                             us_per_row=round(med * 1e3 / (padded_rows if k == 'padded' else total), 3))
        report['packed_over_padded'] = round(report['packed']['wall_ms_median'] / report['padded']['wall_ms_median'], 3)
        print(json.dumps(report), flush=True)
    print(json.dumps(dict(steps_per_form=steps, sets=3)), flush=True)


if __name__ == '__main__':
    main()
