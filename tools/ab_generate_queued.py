"""generate_many against generate_queued on ONE utterance list in ONE process (configs[1]'s model: 12L / d_model 512 / 8 heads,
sampled or greedy beams): decode steps, wall time between two device barriers, tokens/s, and for the queued form the host gap
per poll (from the end of the synchronisation after one block of 32 steps to the first replay of the next: poll read, saves,
refills' launches).  generate_many's code is the yardstick; both decoders are warm (one untimed call each: build, capture,
slot) and every figure is the median over --reps repetitions with the spread (max - min) beside it.

Two length spreads:
  --spread planted   the EOS row of the head is planted from a free greedy run of utterance 0 (1.05 x the head row of the token
                     it emits at step --eos-step, the construction of tests/golden's EOS fixture), and the utterances differ in
                     text and prompt: they stop wherever that row overtakes.  The lengths that come out are printed (min /
                     median / max and the step counts both schedules need for them, engine.plan_queue) — they are measured,
                     not chosen.
  --spread equal     EOS silenced: every utterance runs max_audio_len steps.  Queuing can only cost here; the acceptance is
                     queued - many <= spread of generate_many's repetitions + host gap per poll x polls, both printed.

    python tools/ab_generate_queued.py [--utterances 64] [--beams 4] [--slots 16] [--new 1024] [--reps 5] [--spread planted|equal]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utterances', type=int, default=64)
    ap.add_argument('--beams', type=int, default=4)
    ap.add_argument('--slots', type=int, default=16)
    ap.add_argument('--new', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--spread', choices=('planted', 'equal'), default='planted')
    ap.add_argument('--eos-step', type=int, default=160)
    ap.add_argument('--top-k', type=int, default=1)
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_queued_'))      # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, engine, get_model_class, synth
    from valle2_amd.valle_ar import EOS_POLL
    dev = 'cuda'
    kw = dict(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='LayerNorm', num_beams=args.beams,
              top_k=args.top_k, max_audio_len=args.new)
    cfg = ConfigValle(**kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=5, rich=True), cfg)
    utts = [tuple(t.to(dev) for t in synth.synth_utterance(cfg, 40 + (7 * i) % 60, 40 + (11 * i) % 60, 150 + (37 * i) % 600, seed=4000 + i))
            for i in range(args.utterances)]
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    if args.spread == 'planted':
        free = m.generate_many(utts[:1], beams=1)[0]
        tok = int(free[min(args.eos_step, len(free) - 1)])
        with torch.no_grad():
            m.proj.weight[cfg.num_audio_tokens] = 1.05 * m.proj.weight[tok]
        m.release_decoders()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, outs, dict(m.last_generate_stats)

    forms = {'many': lambda: m.generate_many(utts, beams=args.beams),
             'queued': lambda: m.generate_queued(utts, beams=args.beams, slots=args.slots)}
    res = {}
    for name, fn in forms.items():
        _, outs, st = timed(fn)                              # warm-up: decoder built, graphs captured, slot kept
        ms, gaps = [], []
        for _ in range(args.reps):
            t, outs, st = timed(fn)
            ms.append(t)
            gaps.append(st.get('poll_gap_ms', 0.0) / max(1, st.get('polls', 1)))
        tokens = sum(len(o) for o in outs)
        res[name] = dict(ms=ms, outs=outs, st=st, tokens=tokens, gaps=gaps)
    lengths = [min(len(o) + 1, args.new) for o in res['many']['outs']]
    per = 64 // args.beams
    same = all(torch.equal(a, b) for a, b in zip(res['many']['outs'], res['queued']['outs']))
    report = dict(spread=args.spread, utterances=args.utterances, beams=args.beams, slots=args.slots, max_new=args.new, reps=args.reps,
                  top_k=args.top_k, lengths=dict(min=min(lengths), median=statistics.median(lengths), max=max(lengths)),
                  steps_many_schedule=engine.chunk_schedule_steps(lengths, per, EOS_POLL, args.new),
                  steps_queued_plan=engine.plan_queue(lengths, args.slots, EOS_POLL, args.new)[1],
                  steps_queued=res['queued']['st'].get('steps'), refills=res['queued']['st'].get('refills'),
                  polls=res['queued']['st'].get('polls'), parked_group_steps=res['queued']['st'].get('parked_group_steps'),
                  same_tokens=same)
    for name, r in res.items():
        med = statistics.median(r['ms'])
        report[name] = dict(wall_ms_median=round(med, 3), wall_ms_spread=round(max(r['ms']) - min(r['ms']), 3),
                            wall_ms=[round(x, 3) for x in r['ms']], tokens=r['tokens'], tokens_per_s=round(r['tokens'] / med * 1e3, 1))
    report['queued']['poll_gap_ms_median'] = round(statistics.median(res['queued']['gaps']), 4)
    allowed = report['many']['wall_ms_spread'] + report['queued']['poll_gap_ms_median'] * (report['polls'] or 0)
    report['queued_minus_many_ms'] = round(report['queued']['wall_ms_median'] - report['many']['wall_ms_median'], 3)
    report['equal_length_allowance_ms'] = round(allowed, 3)
    print(json.dumps(report))


if __name__ == '__main__':
    main()
