"""A/B of the decode step at the "base" size, 12L / 768d / 12 heads / dff 3072: the generic LayerNorm-fused GEMMs with linear_1 +
split-K linear_2 + reduce (arm A, VALLE2_FOLD_LN=0: the route this width took before the folded forms served it) against the
folded-LayerNorm GEMMs + vh_ffn_decode (arm B, the default), at 4 beams of one utterance (shared prompt) and at 32 distinct rows.

Every (arm, round) is a fresh process (the knob is read when the package is imported), arms interleaved A B A B ..., each process
warms up with one generate (which also builds and captures the decoder) and times `--calls` further ones; the figure per
process is the median over its calls of decode_ms / steps, the figure per arm the median over the rounds.  Launches per step are
counted from the route: per layer QKV, attention (+ its merge when the keys are split), out-projection, and then either
linear_1, split-K linear_2, reduce (A) or vh_ffn_decode's two (B); head and greedy step once.

    python tools/ab_base_d_model.py [--rounds 5] [--calls 5] [--out profiles/ab_base_d_model.log]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CASES = {'beams4': dict(rows=4, shared=True), 'rows32': dict(rows=32, shared=False)}
TEXT, FRAMES, NEW = 128, 300, 256


def child(case, calls):
    import torch
    sys.path.insert(0, str(REPO))
    from valle2_amd import ConfigValle, get_model_class, synth
    c = CASES[case]
    rows = c['rows']
    cfg = ConfigValle(d_model=768, n_heads=12, dim_feedforward=3072, num_layers=12, dropout=0.0, norm='LayerNorm', num_beams=rows,
                      top_k=1, max_audio_len=NEW)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=0, rich=False), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    m = m.to('cuda').eval()
    utts = [synth.synth_utterance(cfg, TEXT // 2, TEXT - TEXT // 2, FRAMES, seed=1234 + (0 if c['shared'] else u)) for u in range(rows)]
    texts = [torch.cat([u[0], u[2]]).to('cuda') for u in utts]
    firsts = [u[1][:, 0].to('cuda') for u in utts]
    m.generate_batch(texts, firsts, shared_prompt=c['shared'])
    us = []
    for _ in range(calls):
        out = m.generate_batch(texts, firsts, shared_prompt=c['shared'])
        st = m.last_generate_stats
        us.append(st['decode_ms'] / (NEW - 1) * 1e3)
    split = st['n_split'] > 1 or st['shared_prompt']
    per_layer = 3 + int(split) + (2 if st['ffn_fused'] else 3)
    print(json.dumps(dict(case=case, us=statistics.median(us), ln_folded=st['ln_folded'], ffn_fused=st['ffn_fused'],
                          n_split=st['n_split'], launches=cfg.num_layers * per_layer + 2,
                          tokens=out[0, -8:].tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'ab_base_d_model.log'))
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    lines = []
    for case in CASES:
        res = {'A': [], 'B': []}
        for rnd in range(args.rounds):
            for arm in ('A', 'B'):
                env = dict(os.environ, VALLE2_FOLD_LN='0' if arm == 'A' else '1')
                p = subprocess.run([sys.executable, __file__, '--child', case, '--calls', str(args.calls)], env=env, check=True,
                                   capture_output=True, text=True, timeout=600)
                r = json.loads(p.stdout.strip().splitlines()[-1])
                assert r['ln_folded'] == (arm == 'B') and r['ffn_fused'] == (arm == 'B'), r
                res[arm].append(r)
                lines.append(f'{case} round {rnd} arm {arm}: {r["us"]:8.1f} us per step, {r["launches"]} launches per step, '
                             f'n_split {r["n_split"]}, last tokens {r["tokens"]}')
                print(lines[-1], flush=True)
        a, b = (statistics.median(r['us'] for r in res[k]) for k in 'AB')
        lines.append(f'{case}: median of {args.rounds} rounds: A (VALLE2_FOLD_LN=0) {a:.1f} us, B (default) {b:.1f} us per step '
                     f'(A / B = {a / b:.3f}); launches per step {res["A"][0]["launches"]} -> {res["B"][0]["launches"]}; '
                     f'tokens equal: {res["A"][0]["tokens"] == res["B"][0]["tokens"]}')
        print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
