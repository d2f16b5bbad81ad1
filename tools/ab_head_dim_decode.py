"""Decode step of the cached decoder at head widths 32 / 64 / 128 / 256 (12L / d_model 512 at n_heads 16 / 8 / 4 / 2), 32
rows, a 1024-token prompt (256 text + BOS + 767 codec tokens), 256 new tokens, greedy.  The K/V bytes a step streams are the
same at every width (2 x 12 x 32 x 512 x 4 B per context position), beyond the 256 MiB Infinity Cache at this context.

Reports per width: ms per decode step (graph replay, last_generate_stats['decode_ms'] / steps), the decode-attention
kernel's mean us per launch (profile_attn=True: events on the kernel's own dispatch) and its bytes/s over the mean context
of the run, and the recompute path's (use_kv_cache=False) ms per step at 32 new tokens for the ratio.  A kernel-trace run of
its own (rocprofv3 --kernel-trace --stats -- python tools/ab_head_dim_decode.py --widths 32,128 --no-recompute) gives the
trace view of the same kernels.

    python tools/ab_head_dim_decode.py [--widths 32,64,128,256] [--reps 3] [--no-recompute]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', default='32,64,128,256')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=32)
    ap.add_argument('--new', type=int, default=256)
    ap.add_argument('--no-recompute', action='store_true')
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_hd_'))          # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, get_model_class, synth
    dev = 'cuda'
    d, L, B = 512, 12, args.rows
    for hd in (int(w) for w in args.widths.split(',')):
        h = d // hd
        kw = dict(d_model=d, n_heads=h, dim_feedforward=4 * d, num_layers=L, dropout=0.0, norm='LayerNorm', num_beams=B,
                  top_k=1, max_audio_len=args.new)
        cfg = ConfigValle(**kw)
        sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=5, rich=True), cfg)
        m = get_model_class('ValleAR')(cfg)
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        utt = synth.synth_utterance(cfg, 128, 128, 767, seed=1234)
        texts = [torch.cat([utt[0], utt[2]]).to(dev)] * B
        firsts = [utt[1][:, 0].to(dev)] * B
        m.generate_batch(texts, firsts, max_new=args.new)                     # warm-up: build, capture, slot
        step_ms = []
        for _ in range(args.reps):
            m.generate_batch(texts, firsts, max_new=args.new)
            st = m.last_generate_stats
            step_ms.append(st['decode_ms'] / max(1, st['steps_run'] - 1))
        assert st['kv_cache'], 'the cached decoder did not run'
        m.generate_batch(texts, firsts, max_new=args.new, profile_attn=True)
        st = m.last_generate_stats
        s0 = st['s0']
        ctx = s0 + (args.new - 1) / 2                                          # mean keys attended per step
        kbytes = 2 * B * d * 4 * ctx                                           # K + V of one layer's launch
        kern_us = st['attn_kernel_ms'] * 1e3
        res = dict(head_dim=hd, n_heads=h, rows=B, s0=s0, new=args.new, n_split=st['n_split'],
                   decode_ms_per_step=round(min(step_ms), 4), decode_ms_reps=[round(x, 4) for x in step_ms],
                   attn_kernel_us=round(kern_us, 2), attn_bracket_us=round(st['attn_mean_ms'] * 1e3, 2),
                   attn_TBps=round(kbytes / (kern_us * 1e-6) / 1e12, 3))
        if not args.no_recompute:
            rc = get_model_class('ValleAR')(ConfigValle(**dict(kw, use_kv_cache=False)))
            rc.load_state_dict(sd)
            rc = rc.to(dev).eval()
            rc.generate_batch(texts, firsts, max_new=4)
            rc.generate_batch(texts, firsts, max_new=32)
            rst = rc.last_generate_stats
            assert not rst['kv_cache']
            res['recompute_ms_per_step_32new'] = round(rst['decode_ms'] / max(1, rst['steps_run'] - 1), 3)
            res['recompute_over_cached'] = round(res['recompute_ms_per_step_32new'] / res['decode_ms_per_step'], 1)
            del rc
        print(json.dumps(res), flush=True)
        m.release_decoders()
        del m
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
