"""A/B: EncodecEncoder.batch_encode (csrc/codec.hip) against the fp32 mirror (tests/codec_enc_mirror.py) run on the same GPU
through torch, default 24 kHz config with seeded random weights, 10 s of audio (240 000 samples, 750 frames), B in {1, 32}.
The two arms alternate in one process; the median, minimum and spread of 7 rounds are reported per arm, after one warm-up round
each.  Two parts of the native arm are then timed on their own, on the same inputs, to show where its time goes: the quantiser
(`vh_rvq_encode`, one launch) and the LSTM's recurrence (`vh_lstm_layer`, one launch per time step and layer).  Timing is not
pass/fail.

    python tools/ab_codec_encode.py [--rounds 7] [--seconds 10] [--batches 1 32] [--codebooks 8] > profiles/ab_codec_encode.log
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import codec_enc_mirror as E  # noqa: E402
from valle2_amd import EncodecEncoder, kernels as K  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def line(B, name, ts):
    print(f'B={B:3d} {name:18s} median {statistics.median(ts):9.2f} ms  min {min(ts):9.2f} ms  spread {max(ts) - min(ts):8.2f} ms  '
          f'all {" ".join(f"{t:.1f}" for t in ts)}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--codebooks', type=int, default=8)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sd = E.random_encoder_state_dict(seed=12, n_codebooks=args.codebooks)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    enc = EncodecEncoder.from_state_dict(sd)
    L = int(round(args.seconds * enc.sampling_rate))
    print(f'device: {torch.cuda.get_device_name(0)}; default config, {args.codebooks} codebooks, L={L} samples ({enc.frames(L)} frames), '
          f'{args.rounds} rounds, arms alternate')
    for B in args.batches:
        wave = (0.3 * torch.randn(B, L, generator=torch.Generator().manual_seed(B))).to(dev)
        arms = {'native': lambda: enc.batch_encode(wave),
                'torch_fp32_mirror': lambda: E.encode(sd_dev, wave, torch.float32)[0]}
        times = {k: [] for k in arms}
        outs = {}
        with torch.inference_mode():
            for rnd in range(args.rounds + 1):
                for name, fn in arms.items():
                    ms, outs[name] = timed(fn)
                    if rnd:                                   # round 0 warms up
                        times[name].append(ms)
            # the native arm's parts, on its own intermediate tensors
            w = enc._weights(dev)
            emb = enc._embed(wave)
            h0 = torch.randn(B, emb.shape[1], w['lstm'][0][2].shape[1], device=dev)
            xproj = [K.conv1d_causal(h0, w_ih, bias) for w_ih, bias, _ in w['lstm']]
            parts = {'vh_rvq_encode': lambda: enc._quantise(emb, args.codebooks),
                     'vh_lstm_layer x%d' % len(w['lstm']): lambda: [K.lstm_layer(xp, w_hh) for xp, (_, _, w_hh) in zip(xproj, w['lstm'])]}
            ptimes = {k: [] for k in parts}
            for rnd in range(args.rounds + 1):
                for name, fn in parts.items():
                    ms, _ = timed(fn)
                    if rnd:
                        ptimes[name].append(ms)
        same = (outs['native'] == outs['torch_fp32_mirror']).double().mean().item()
        for name, ts in times.items():
            line(B, name, ts)
        native = statistics.median(times['native'])
        for name, ts in ptimes.items():
            line(B, name, ts)
            print(f'B={B:3d} {name:18s} share of the native encode (medians) {100 * statistics.median(ts) / native:5.1f} %')
        print(f'B={B:3d} audio seconds per call {B * L / enc.sampling_rate:.0f}; codes equal to the mirror\'s: {100 * same:.2f} % '
              f'(the fp32 mirror is not the yardstick: tests/test_codec_enc_gpu.py holds the codes to the float64 one); '
              f'speed-up (medians) {statistics.median(times["torch_fp32_mirror"]) / native:.2f}x')


if __name__ == '__main__':
    main()
