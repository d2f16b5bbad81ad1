"""ValleNAR.generate_batch (rows padded to the longest) against ValleNAR.generate_packed (rows back to back, no padding) in ONE
process, same model, same utterances: configs[2]'s model (12L / d_model 512 / 8 heads / 8 codebooks), 64 utterances, greedy.
generate_batch in the same build is the yardstick.  Three sets of row lengths (text + prompt + target frames):

  equal    every row 1024                       (nothing to save: the packed form may only cost here)
  spread   evenly spread over 256 .. 1024       (0.62 of the padded GEMM / LayerNorm rows, 0.70 of its attention key tiles)
  mix      4 rows of 256 to every row of 1024   (0.40 of the rows)

Both forms are warm (one untimed call each per set), the timed calls alternate padded / packed, and every figure is the median
over --reps repetitions of the wall time between two device synchronisations with the spread (max - min) beside it.  The share
of greedy tokens on which the two forms agree is printed too: they run other GEMM row counts, so they agree to summation order
and a token may flip where the two leading logits are closer than that.

--perf-mode: the same comparison between the two 16-bit forms, generate_batch(perf_mode=True) and generate_packed_perf.

    python tools/ab_nar_packed.py [--utterances 64] [--reps 7] [--max-len 1024] [--perf-mode]   (one JSON line per set)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utterances', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=1024)
    ap.add_argument('--perf-mode', action='store_true', help='compare generate_batch(perf_mode=True) with generate_packed_perf')
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_nar_packed_'))      # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, get_model_class, synth
    assert torch.cuda.is_available(), 'ab_nar_packed.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'
    cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='AdaptiveLayerNorm')
    m = get_model_class('ValleNAR')(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 'ValleNAR', seed=5, rich=True))
    m = m.to(dev).eval()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, outs

    for name, lengths in length_sets(args.utterances, args.max_len).items():
        g = torch.Generator().manual_seed(9000)
        texts, pcs, firsts = [], [], []
        for n in lengths:                                    # an eighth text, a quarter acoustic prompt, the rest target frames
            tx, tc = n // 8, n // 4
            texts.append(torch.randint(0, cfg.vocab_size, (tx,), generator=g).to(dev))
            pcs.append(torch.randint(0, cfg.num_audio_tokens, (tc, cfg.num_quantizers), generator=g).to(dev))
            firsts.append(torch.randint(0, cfg.num_audio_tokens, (n - tx - tc,), generator=g).to(dev))
        packed = m.generate_packed_perf if args.perf_mode else m.generate_packed
        forms = {'padded': lambda: m.generate_batch(texts, pcs, firsts, greedy=True, perf_mode=args.perf_mode),
                 'packed': lambda: packed(texts, pcs, firsts, greedy=True)}
        outs = {k: timed(fn)[1] for k, fn in forms.items()}                      # warm-up of every shape the timed calls use
        ms = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():                                             # alternate the two forms
                ms[k].append(timed(fn)[0])
        tokens = sum(o.numel() for o in outs['padded'])
        same = sum(int((a == b).sum()) for a, b in zip(outs['padded'], outs['packed']))
        lmax, total = max(lengths), sum(lengths)
        report = dict(set=name, perf_mode=args.perf_mode, utterances=len(lengths), reps=args.reps, rows_padded=lmax * len(lengths), rows_packed=total,
                      row_share=round(total / (lmax * len(lengths)), 3),
                      key_tile_share=round(sum(n * n for n in lengths) / (lmax * total), 3),
                      tokens=tokens, tokens_equal_share=round(same / tokens, 6))
        for k, v in ms.items():
            med = statistics.median(v)
            report[k] = dict(wall_ms_median=round(med, 2), wall_ms_spread=round(max(v) - min(v), 2), wall_ms=[round(x, 2) for x in v])
        report['packed_over_padded'] = round(report['packed']['wall_ms_median'] / report['padded']['wall_ms_median'], 3)
        print(json.dumps(report), flush=True)


if __name__ == '__main__':
    main()
