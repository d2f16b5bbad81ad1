"""A/B: EncodecDecoder.batch_decode (csrc/codec.hip) against the fp32 mirror (tests/codec_mirror.py) run on the same GPU through
torch, default 24 kHz config with seeded random weights, T = 750 frames (10 s), B in {1, 32}.  The two arms alternate in one
process; the median and minimum of 7 rounds are reported per arm, after one warm-up round each.  Timing is not pass/fail.

    python tools/ab_codec_decode.py [--rounds 7] [--frames 750] [--batches 1 32] > profiles/ab_codec_decode.log
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import codec_mirror as M  # noqa: E402
from valle2_amd import EncodecDecoder  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sd = M.random_state_dict(seed=11)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    dec = EncodecDecoder.from_state_dict(sd)
    print(f'device: {torch.cuda.get_device_name(0)}; default config, T={args.frames} frames, {args.rounds} rounds, arms alternate')
    for B in args.batches:
        codes = torch.randint(0, 1024, (B, 8, args.frames), generator=torch.Generator().manual_seed(B)).to(dev)
        arms = {'native': lambda: dec.batch_decode(codes),
                'torch_fp32_mirror': lambda: M.decode(sd_dev, codes, torch.float32)}
        times = {k: [] for k in arms}
        outs = {}
        with torch.inference_mode():
            for rnd in range(args.rounds + 1):
                for name, fn in arms.items():
                    ms, outs[name] = timed(fn)
                    if rnd:                                   # round 0 warms up
                        times[name].append(ms)
        diff = (outs['native'] - outs['torch_fp32_mirror']).abs().max().item()
        scale = outs['torch_fp32_mirror'].abs().max().item()
        for name, ts in times.items():
            print(f'B={B:3d} {name:18s} median {statistics.median(ts):9.2f} ms  min {min(ts):9.2f} ms  all {" ".join(f"{t:.1f}" for t in ts)}')
        print(f'B={B:3d} audio seconds per call {B * args.frames / 75:.0f}; max |native - mirror| = {diff:.3e} at max |y| = {scale:.2f}; '
              f'speed-up (medians) {statistics.median(times["torch_fp32_mirror"]) / statistics.median(times["native"]):.2f}x')


if __name__ == '__main__':
    main()
