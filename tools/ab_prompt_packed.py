"""The AR prompt pass over padded rows against the same pass over packed rows (`ValleAR.packed_prompt`) in ONE process, same
model, same utterances: configs[1]'s AR model (12L / d_model 512 / 8 heads), greedy.  The padded pass of the same build is the
yardstick: with the switch off a call launches what it always launched.  Three sets of context lengths (text + BOS + prompt):

  equal    every utterance 1024                       (not ragged: the call takes the padded pass either way — the CONTROL)
  spread   evenly spread over 256 .. 1024             (0.62 of the padded rows, 0.70 of its attention key tiles)
  mix      4 utterances of 256 to every one of 1024   (0.40 of the rows)

Section 1, `generate_batch` of 32 utterances: `prefill_ms` (device events around the prompt pass and the first sample,
`last_generate_stats`) and the wall time of the whole call between two device synchronisations.
Section 2, `generate_queued` of 64 utterances over 16 slots, beams 2: the same two figures; here the switch also packs the refills of
a poll that retires two or more groups.  Every utterance carries a `Bounded` greedy request whose max_new is a multiple of the
poll (32 .. --queue-max-new), so groups retire at different polls, several at most of them.  (On the equal set the starting
pass is padded either way, but the refills still pack — several one-row passes become one — so there the set is no control.)

Both arms are warm (one untimed call each per set), the timed calls alternate off / on, and every figure is the median over
--reps repetitions with the spread (max - min) beside it.  The share of greedy tokens on which the two arms agree is printed
too: they run other GEMM row counts, so they agree to summation order and a token may flip where the two leading logits are
closer than that (and every later token of that row with it).

--perf-mode True | kv measures the PERF-MODE prompt pass instead (`ValleAR.packed_prompt_perf`; section 1 only: queued and
grouped calls refuse perf_mode): `generate_batch(..., perf_mode=True)` runs the 16-bit packed pass against the 16-bit padded
one, `perf_mode='kv'` the fp32 packed pass against the fp32 padded one, both narrowed once.

--padded-only times the padded arm alone and never touches a switch, and --package-root DIR imports `valle2_amd` from another
checkout (built there): together they measure the PARENT commit's padded pass with this tool, the control that shows the padded
route has not moved.

    python tools/ab_prompt_packed.py [--utterances 32] [--reps 7] [--max-len 1024] [--max-new 512] [--skip-queued]
                                     [--perf-mode {True,kv}] [--padded-only] [--package-root DIR]
    (one JSON line per set and section)
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


def length_sets(n, lmax):
    lo = lmax // 4
    return {'equal': [lmax] * n,
            'spread': [lo + (i * (lmax - lo)) // max(1, n - 1) for i in range(n)],
            'mix': [lmax if i % 5 == 4 else lo for i in range(n)]}


def summary(values):
    return dict(median=round(statistics.median(values), 3), spread=round(max(values) - min(values), 3), all=[round(v, 3) for v in values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utterances', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=1024)
    ap.add_argument('--max-new', type=int, default=512, help='steps of generate_batch (configs[1]: 512)')
    ap.add_argument('--queue-utterances', type=int, default=64)
    ap.add_argument('--queue-slots', type=int, default=16)
    ap.add_argument('--queue-max-new', type=int, default=256, help='max_audio_len of the queued section')
    ap.add_argument('--skip-queued', action='store_true')
    ap.add_argument('--perf-mode', choices=['True', 'kv'], default=None,
                    help='measure generate_batch(perf_mode=...) under ValleAR.packed_prompt_perf (section 1 only)')
    ap.add_argument('--padded-only', action='store_true', help='time the padded arm alone; no switch is set')
    ap.add_argument('--package-root', default=None, help='import valle2_amd from this checkout instead of the tool\'s own')
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.package_root).resolve() if args.package_root else Path(__file__).resolve().parents[1]))
    os.chdir(tempfile.mkdtemp(prefix='ab_prompt_packed_'))      # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import Bounded, ConfigValle, Sampling, get_model_class, synth
    assert torch.cuda.is_available(), 'ab_prompt_packed.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'

    def model(max_audio_len):
        cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='LayerNorm', num_beams=1,
                          top_k=1, max_audio_len=max_audio_len)
        m = get_model_class('ValleAR')(cfg)
        m.load_state_dict(synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=5, rich=True), cfg))
        return cfg, m.to(dev).eval()

    def ids(cfg, lengths):
        g = torch.Generator().manual_seed(9000)
        texts, firsts = [], []
        for n in lengths:                                        # a quarter text, then BOS + the acoustic prompt
            tx = n // 4
            texts.append(torch.randint(0, cfg.vocab_size, (tx,), generator=g).to(dev))
            firsts.append(torch.randint(0, cfg.num_audio_tokens, (n - tx - 1,), generator=g).to(dev))
        return texts, firsts

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    perf_mode = {None: False, 'True': True, 'kv': 'kv'}[args.perf_mode]
    switch = 'packed_prompt_perf' if perf_mode else 'packed_prompt'

    def compare(m, section, name, lengths, call, flat, extra):
        """Alternate the switch off / on around `call`; one JSON line."""
        def arm(on):
            if not args.padded_only:
                setattr(m, switch, on)
            ms, out = timed(call)
            return ms, out, dict(m.last_generate_stats)
        arms = {'padded': False} if args.padded_only else {'padded': False, 'packed': True}
        outs = {k: arm(on)[1:] for k, on in arms.items()}        # warm-up of every shape the timed calls use
        wall, prefill = {k: [] for k in arms}, {k: [] for k in arms}
        for _ in range(args.reps):
            for k, on in arms.items():                           # alternate the two arms
                ms, _, st = arm(on)
                wall[k].append(ms)
                prefill[k].append(st['prefill_ms'])
        a, b = flat(outs['padded'][0]), flat(outs[list(arms)[-1]][0])
        lmax, total = max(lengths), sum(lengths)
        report = dict(section=section, perf_mode=perf_mode, package=str(Path(sys.modules['valle2_amd'].__file__).parent.parent.name)
                      if args.package_root else 'this checkout', set=name, utterances=len(lengths), reps=args.reps, rows_padded=lmax * len(lengths),
                      rows_packed=total, row_share=round(total / (lmax * len(lengths)), 3),
                      key_tile_share=round(sum(n * n for n in lengths) / (lmax * total), 3),
                      tokens=int(a.numel()), tokens_equal_share=round(float((a == b).float().mean()), 6))
        for k in arms:
            st = outs[k][1]
            report[k] = dict(packed_prompt=st.get('packed_prompt'), prompt_rows=st.get('prompt_rows'), prefill_ms=summary(prefill[k]),
                             wall_ms=summary(wall[k]), **{key: st.get(key) for key in extra})
        for fig, src in (('prefill', prefill), ('wall', wall)) if not args.padded_only else ():
            report[f'{fig}_packed_over_padded'] = round(statistics.median(src['packed']) / statistics.median(src['padded']), 3)
        print(json.dumps(report), flush=True)

    cfg, m = model(args.max_new)
    for name, lengths in length_sets(args.utterances, args.max_len).items():
        texts, firsts = ids(cfg, lengths)
        compare(m, 'generate_batch', name, lengths, lambda: m.generate_batch(texts, firsts, perf_mode=perf_mode), lambda rows: rows,
                ('prefill_bf16', 'kv_bf16') if perf_mode else ())
    if args.skip_queued or perf_mode:
        return
    m.release_decoders()
    del m
    cfg, m = model(args.queue_max_new)
    polls = max(1, args.queue_max_new // 32)
    for name, lengths in length_sets(args.queue_utterances, args.max_len).items():
        texts, firsts = ids(cfg, lengths)
        utts = [(t, c.unsqueeze(1), None, Bounded(Sampling(seed=i, top_k=1), max_new=32 * (1 + (5 * i) % polls)))
                for i, (t, c) in enumerate(zip(texts, firsts))]
        compare(m, 'generate_queued', name, lengths, lambda: m.generate_queued(utts, beams=2, slots=args.queue_slots),
                lambda outs: torch.cat([torch.nn.functional.pad(o, (0, args.queue_max_new - o.shape[0]), value=-1) for o in outs]),
                ('refills', 'packed_refills', 'polls'))


if __name__ == '__main__':
    main()
