"""Costs of the decode step at d_model above 1024 (the wide folded form).

    python tools/bench_wide_d_model.py            (every section runs as a child process under its own time limit)
    python tools/bench_wide_d_model.py gemm|step  (one section, in this process)

Prints:
  * gemm: per launch at M in {8, 32} and d in {1536, 2048, 4096}, the folded QKV (N = 3d) and linear_1 (N = 4d, GELU)
    GEMMs of the decode step against the unfused pair (vh_layernorm + the plain GEMM): HIP-event time over 200 launches
    after warm-up, the weight bytes per second the launch reaches and that as a fraction of a 6.4 TB/s HBM read ceiling.
    Every launch reads another copy of the weights (the copies add up to more than the 256 MB last-level cache), so the
    stream comes from HBM as it does in a model of many layers;
  * step: one decode step of a 24-layer 2048d / 32 heads / dff 8192 model at 8 rows and a context of about 1 k: us per
    step (graph replay) and the step's algorithmic bytes (fp32 weights + the K/V rows read) over that time.
"""
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

DEV = 'cuda'
HBM_CEILING = 6.4e12
LIMITS = {'gemm': 420, 'step': 540}        # seconds per section


def timed(fn, n_variants, reps=200, warm=20):
    import torch
    for i in range(warm):
        fn(i % n_variants)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i % n_variants)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per launch


def gemm():
    import torch
    from valle2_amd import kernels as K
    torch.cuda.set_device(0)
    print('decode GEMMs with LayerNorm, us per launch (hip events, 200 launches, weights rotated through > 512 MB)')
    print(f'{"gemm":>9} {"d":>5} {"M":>3} {"folded us":>10} {"LN + plain us":>14} {"folded TB/s":>12} {"of 6.4 TB/s":>12} {"folded / pair":>14}')
    for d in (1536, 2048, 4096):
        for name, N, act in (('qkv', 3 * d, K.ACT_NONE), ('linear_1', 4 * d, K.ACT_GELU)):
            wbytes = N * d * 4
            n = max(2, -(-(512 << 20) // wbytes))
            g = torch.Generator().manual_seed(d)
            gm = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
            bt = (0.1 * torch.randn(d, generator=g)).to(DEV)
            bias = torch.randn(N, generator=g).to(DEV)
            ws = [(0.05 * torch.randn(N, d, generator=g)).to(DEV) for _ in range(n)]
            folded = [K.ln_fold(w, gm, bt, bias) for w in ws]
            for M in (8, 32):
                x = torch.randn(M, d, generator=g).to(DEV)
                xn = torch.empty_like(x)
                out = torch.empty(M, N, device=DEV)
                if name == 'qkv':
                    h, S = d // 64, 8
                    kc, vc = torch.zeros(M, h, S, 64, device=DEV), torch.zeros(M, h, S, 64, device=DEV)
                    cl = torch.zeros(M, dtype=torch.int32, device=DEV)
                    q = torch.empty(M, d, device=DEV)
                    f_us = timed(lambda i: K.linear_qkv_folded(x, folded[i], q, kc, vc, M, 1, h, cache_len=cl), n)

                    def pair(i):
                        K.layernorm(x, gm, bt, out=xn)
                        K.linear_qkv(xn, ws[i], q, kc, vc, M, 1, h, cache_len=cl)
                else:
                    f_us = timed(lambda i: K.linear_folded(x, folded[i], out=out, act=act), n)

                    def pair(i):
                        K.layernorm(x, gm, bt, out=xn)
                        K.linear(xn, ws[i], bias, out=out, act=act)
                p_us = timed(pair, n)
                tbs = wbytes / (f_us * 1e-6)
                print(f'{name:>9} {d:5d} {M:3d} {f_us:10.1f} {p_us:14.1f} {tbs / 1e12:12.2f} {tbs / HBM_CEILING:12.0%} {f_us / p_us:14.2f}')
            del ws, folded


def step():
    import torch
    from valle2_amd import ConfigValle, get_model_class, synth
    torch.cuda.set_device(0)
    d, L, dff, B, new = 2048, 24, 8192, 8, 65
    cfg = ConfigValle(d_model=d, n_heads=d // 64, dim_feedforward=dff, num_layers=L, dropout=0.0, norm='LayerNorm',
                      num_beams=B, top_k=1, max_audio_len=new)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=1), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    del sd
    m = m.to(DEV).eval()
    utt = synth.synth_utterance(cfg, 120, 120, 750, seed=2)
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    first = utt[1][:, 0].to(DEV)
    m.generate_batch([text] * B, [first] * B)               # builds and captures the decoder
    m.generate_batch([text] * B, [first] * B)
    st = m.last_generate_stats
    steps = st['steps_run'] - 1
    us = st['decode_ms'] * 1e3 / steps
    ctx = st['s0'] + new // 2
    V = cfg.num_audio_tokens + 1
    wbytes = (L * (4 * d * d + 2 * d * dff) + V * d) * 4
    kvbytes = L * 2 * B * ctx * d * 4
    print(f'decode step, {L} layers {d}d / {d // 64} heads / dff {dff}, {B} rows, context {st["s0"]}..{st["s0"] + new}, '
          f'ln_folded={st["ln_folded"]}, decoder_reused={st["decoder_reused"]}:')
    print(f'  {us:.1f} us per step over {steps} steps; weights {wbytes / 1e6:.0f} MB + K/V {kvbytes / 1e6:.0f} MB per step '
          f'= {(wbytes + kvbytes) / (us * 1e-6) / 1e12:.2f} TB/s ({(wbytes + kvbytes) / (us * 1e-6) / HBM_CEILING:.0%} of 6.4 TB/s)')


SECTIONS = {'gemm': gemm, 'step': step}

if __name__ == '__main__':
    if len(sys.argv) > 1:
        SECTIONS[sys.argv[1]]()
        sys.exit(0)
    for name in SECTIONS:                                    # a fresh child per section, each under its own time limit;
        rc = subprocess.run(['timeout', '-k', '10', str(LIMITS[name]), sys.executable, __file__, name]).returncode
        if rc != 0:                                          # nothing more is started on the GPU after a failure
            print(f'section {name} ended with status {rc}: stopping')
            sys.exit(rc)
