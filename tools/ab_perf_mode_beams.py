"""A/B of perf mode (the 16-bit K/V cache) below 256 (row, head) pairs and over a shared prompt: alternating generates in ONE
process, one warm-up round, equal tokens asserted within an arm.  Two workloads on the 12L/512d model with the bench's
utterance (256 text + BOS + 767 prompt frames):

  defaults   the reference's generation defaults (4 beams, top-k 50, 1024 steps; the same torch seed before every generate):
             fp32 shared prompt | perf_mode shared prompt
  beams32    configs[1] with 32 beams (greedy, 512 steps): fp32 shared | perf_mode independent rows | perf_mode shared

An arm the library refuses (the new arms on a commit that lacks them) is reported as refused and skipped, so the same tool
measures the yardstick arms on the parent commit.  After the timed rounds every arm runs once with profile_attn: the attention
launch's own time (start / stop events on its dispatch) and the K/V bytes it reads per second at the run's mean context.

    python tools/ab_perf_mode_beams.py [--reps 5] [--workload defaults|beams32|both]
"""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def kv_bytes_per_step(st, B, h, new):
    """K + V bytes the step's attention reads per layer at the run's mean context."""
    elem = 2 if st['kv_bf16'] else 4
    own = new / 2
    keys = st['s0'] + B * own if st['shared_prompt'] else B * (st['s0'] + own)
    return 2 * keys * 64 * h * elem


def run_workload(name, m, text, first, B, new, arms, reps, seed):
    from valle2_amd._lib import VhError
    h, layers = m.config.n_heads, m.config.num_layers
    res, ref, live = {}, {}, []
    for rep in range(reps + 1):
        for arm, kw in arms:
            if rep and arm not in live:
                continue
            if seed is not None:
                torch.manual_seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                out = m.generate_batch([text] * B, [first] * B, max_new=new, **kw)
            except (ValueError, VhError) as e:
                print(f'{name:9s} {arm:22s} refused: {str(e)[:110]}')
                continue
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = m.last_generate_stats
            if arm not in ref:
                ref[arm] = out.clone()
                live.append(arm)
            assert torch.equal(out, ref[arm]), f'{arm}: tokens changed between repeats'
            if rep:
                res.setdefault(arm, []).append((st['decode_ms'] / max(1, st['steps_run'] - 1) * 1e3, dt * 1e3, st['prefill_ms']))
    for arm, kw in arms:
        if arm not in live:
            continue
        us = sorted(x[0] for x in res[arm])
        ms = sorted(x[1] for x in res[arm])
        if seed is not None:
            torch.manual_seed(seed)
        m.generate_batch([text] * B, [first] * B, max_new=new, profile_attn=True, **kw)
        st = m.last_generate_stats
        kern_us = (st['attn_kernel_ms'] or 0.0) * 1e3
        byts = kv_bytes_per_step(st, B, h, new)
        rate = byts / (kern_us * 1e-6) / 1e12 if kern_us else float('nan')
        print(f'{name:9s} {arm:22s} n_split={st["n_split"]:2d}  {us[len(us) // 2]:7.1f} us per step (min {us[0]:.1f}, max {us[-1]:.1f}, '
              f'{len(us)} repeats)  {ms[len(ms) // 2]:8.2f} ms per generate  prompt pass {res[arm][-1][2]:.2f} ms  '
              f'attention launch {kern_us:6.2f} us x {layers} layers = {byts / 1e6:.2f} MB of K/V -> {rate:.2f} TB/s')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workload', default='both', choices=['defaults', 'beams32', 'both'])
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='vh_ab_'))
    from valle2_amd import ConfigValle, get_model_class, synth
    dev = 'cuda'
    base = dict(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='LayerNorm')
    greedy = ConfigValle(**base, num_beams=32, top_k=1, max_audio_len=512)
    sd = synth.silence_eos(synth.make_state_dict(greedy, 'ValleAR', seed=0, rich=False), greedy)
    u = synth.synth_utterance(greedy, 128, 128, 767, seed=1234)
    text, first = torch.cat([u[0], u[2]]).to(dev), u[1][:, 0].to(dev)

    def model(cfg):
        m = get_model_class('ValleAR')(cfg)
        m.load_state_dict(sd)
        return m.to(dev).eval()
    if args.workload in ('defaults', 'both'):
        cfg = ConfigValle(**base)
        assert (cfg.num_beams, cfg.top_k, cfg.max_audio_len) == (4, 50, 1024)
        run_workload('defaults', model(cfg), text, first, 4, 1024,
                     [('fp32 shared', dict(shared_prompt=True)), ('perf_mode shared', dict(shared_prompt=True, perf_mode=True))],
                     args.reps, seed=0)
    if args.workload in ('beams32', 'both'):
        run_workload('beams32', model(greedy), text, first, 32, 512,
                     [('fp32 shared', dict(shared_prompt=True)), ('perf_mode independent', dict(perf_mode=True)),
                      ('perf_mode shared', dict(shared_prompt=True, perf_mode=True))], args.reps, seed=None)


if __name__ == '__main__':
    main()
