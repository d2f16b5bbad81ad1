"""Costs of the wide-vocabulary sampler and the many-codebook embedding sum.

    python tools/bench_wide_vocab.py            (under `rocprofv3 --kernel-trace --stats -- python ...` for kernel totals)

Prints, from hip events around repeated launches:
  * vh_sample_step_wide per launch at V in {2049, 4097, 8193, 16384} x B in {4, 32}, fast path (top_k = 50, top_p = 1) and
    general path (top_k = 50, top_p = 0.9; and top_k = 0, top_p = 0.8: the whole row sorted); vh_sample_step at V = 1025 and
    2048 for reference;
  * vh_embed_sum_pe on a NAR prompt (8 rows x 225 frames, d_model 1024) at Q = 8, 16, 32 tables;
  * generate() per decode step (12 layers, d_model 512, 8 rows, top_k = 50) at num_audio_tokens 1024 and 4096.
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = 'cuda'


def timed(fn, reps=200, warm=10):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per launch


def sampler():
    from valle2_amd import kernels
    print('sampler: us per launch (hip events, 200 launches)')
    print(f'{"kernel":>8} {"V":>6} {"B":>3} {"mode":>22} {"us":>8}')
    for V in (1025, 2048, 2049, 4097, 8193, 16384):
        for B in (4, 32):
            g = torch.Generator().manual_seed(V)
            logits = (3.0 * torch.randn(B, (V + 3) // 4 * 4, generator=g)).to(DEV)
            emb, pe = torch.randn(V, 512, generator=g).to(DEV), torch.randn(8, 512, generator=g).to(DEV)
            codes = torch.zeros(B, 8, dtype=torch.int64, device=DEV)
            st = [torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV),
                  torch.ones(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV),
                  torch.empty(B, 512, device=DEV)]
            for name, k, p in (('fast (k=50)', 50, 1.0), ('general (k=50 p=0.9)', 50, 0.9), ('general (k=0 p=0.8)', 0, 0.8)):
                for wide in ((False,) if V <= 2048 else ()) + ((True,) if V > 1025 else ()):
                    def run():
                        st[2].fill_(1)                     # every launch samples position 1 again
                        kernels.sample_step(logits, V, V - 1, k, p, 1.0, 5, codes, st[0], st[1], emb, pe, st[2], st[3], st[4],
                                            wide=wide)
                    fill = timed(lambda: st[2].fill_(1))
                    us = timed(run) - fill
                    print(f'{"wide" if wide else "narrow":>8} {V:6d} {B:3d} {name:>22} {us:8.1f}')


def embedding():
    from valle2_amd import kernels
    print('embed_sum_pe on a NAR prompt (8 x 225 frames, d 1024): us per launch')
    B, T, d = 8, 225, 1024
    pe = torch.randn(512, d, device=DEV)
    out = torch.empty(B, T, d, device=DEV)
    for q in (8, 16, 32):
        tabs = [torch.randn(1024, d, device=DEV) for _ in range(q)]
        ids = torch.randint(0, 1024, (B, T, q), device=DEV)
        us = timed(lambda: kernels.embed_sum_pe(ids, tabs, pe, 0, out))
        gbs = (B * T * d * 4 * (q + 2)) / (us * 1e-6) / 1e9
        print(f'  Q={q:2d}: {us:7.1f} us  ({gbs:.0f} GB/s of row traffic)')


def generate():
    from valle2_amd import ConfigValle, get_model_class, synth
    print('generate(): ms per decode step (12L / 512d, 8 rows, top_k 50, 256 new tokens)')
    for va in (1024, 4096):
        cfg = ConfigValle(d_model=512, n_heads=8, dim_feedforward=2048, num_layers=12, dropout=0.0, norm='LayerNorm',
                          num_beams=8, top_k=50, max_audio_len=256, num_audio_tokens=va)
        sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=1), cfg)
        m = get_model_class('ValleAR')(cfg)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        utt = synth.synth_utterance(cfg, 40, 40, 150, seed=2)
        text = torch.cat([utt[0], utt[2]]).to(DEV)
        first = utt[1][:, 0].to(DEV)
        m.generate_batch([text] * 8, [first] * 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate_batch([text] * 8, [first] * 8)
        torch.cuda.synchronize()
        steps = m.last_generate_stats['steps_run']
        print(f'  num_audio_tokens={va}: {(time.perf_counter() - t0) * 1e3 / steps:.3f} ms per step over {steps} steps')


if __name__ == '__main__':
    torch.cuda.set_device(0)
    sampler()
    embedding()
    generate()
