"""A/B of grouped shared-prompt decoding: 8 utterances at the reference's sampling defaults (4 beams, top_k = 50) on the
configs[1] model (12L/512d/h8), each with a context of about 1024 tokens and a FIXED number of decode steps (the EOS row is
silenced), three ways in ONE process, alternating:

    many         generate_many(utterances)                       one grouped decode: 8 prompt rows, 32 decode rows
    serial       generate(utterance) x 8                          4 decode rows at a time, one prompt pass each
    independent  generate_batch of the same 32 rows, beams=1      32 prompt rows, every row streams its own prompt K/V

Wall time per arm is a host clock around work that ends in a device synchronise; the first round warms every shape
(decoder slots, captured graphs) and is dropped; the median of the others is reported with min and max.  Sampled tokens
differ between the arms by construction (other row indices draw other noise), so the arms are compared on time only; greedy
equality of the three forms is what tests/test_shared_groups_gpu.py checks.

    python tools/ab_generate_many.py [--reps 5] [--steps 256] [--utterances 8]
"""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--utterances', type=int, default=8)
    ap.add_argument('--beams', type=int, default=4)
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='vh_ab_'))
    from valle2_amd import ConfigValle, get_model_class, synth
    if not torch.cuda.is_available():
        raise SystemExit('ab_generate_many: needs a HIP device (a timing on anything else says nothing)')
    dev = 'cuda'
    cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='LayerNorm',
                      num_beams=args.beams, top_k=50, max_audio_len=args.steps)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=0, rich=False), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    # contexts of 1024 - 17 i tokens (text + BOS + prompt frames): different texts and prompt lengths, one prefix capacity
    utts = []
    for i in range(args.utterances):
        u = synth.synth_utterance(cfg, 128 - i, 128, 767 - 16 * i, seed=1234 + i)
        utts.append(tuple(t.to(dev) for t in u))
    texts = [torch.cat([u[0], u[2]]) for u in utts]
    firsts = [u[1][:, 0] for u in utts]
    n = args.beams

    def many():
        return m.generate_many(utts)

    def serial():
        return [m.generate(*u) for u in utts]

    def independent():
        return m.generate_batch([t for t in texts for _ in range(n)], [c for c in firsts for _ in range(n)])

    arms = [('many', many), ('serial', serial), ('independent', independent)]
    res = {name: [] for name, _ in arms}
    notes = {}
    for rep in range(args.reps + 1):
        for name, fn in arms:
            torch.manual_seed(100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            st = m.last_generate_stats
            notes[name] = (f"prompt pass {st['prefill_ms']:.2f} ms, decode {st['decode_ms'] / max(st['steps_run'] - 1, 1) * 1e3:.1f} us "
                           f"per step, grouped_shared={st.get('grouped_shared')}, decoder_reused={st['decoder_reused']} (last call of the arm)")
            if rep:
                res[name].append(dt)
    print(f'{args.utterances} utterances x {n} beams, {args.steps} steps, top_k=50, context ~1024; {args.reps} timed rounds')
    base = sorted(res['many'])[len(res['many']) // 2]
    for name, v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f'{name:12s} {med:9.2f} ms per {args.utterances} utterances (min {v[0]:.2f}, max {v[-1]:.2f}; {med / base:.2f}x many)  {notes[name]}')


if __name__ == '__main__':
    main()
