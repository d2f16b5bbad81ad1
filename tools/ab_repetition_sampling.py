"""What the repetition-aware tail of the per-row samplers costs: tools/ab_repetition_sampling.py OLD.so NEW.so [--reps 100]
[--rounds 9].  vh_sample_step_rows (V = 1025) and vh_sample_step_wide_rows (V = 1025 and 4096) over 32 rows, top_k = 50,
tok_p = 1, d = 1024, four arms alternating in ONE process on ONE device (both builds loaded with ctypes next to each other, as
tools/ab_lib.py does):

  1 parent      OLD.so, the two reserved words zero
  2 words zero  NEW.so, the two reserved words zero: one block-uniform compare more than the parent
  3 no trigger  NEW.so, window 10, max_repeats 9: every step counts its window, none redraws (ten equal tokens in a row of
                draws over 50 near-flat survivors do not happen)
  4 all trigger NEW.so, window 2^31 - 1, max_repeats 0, every row's prompt holding each of its 50 survivors: every step of every
                row counts its whole history and redraws over all V entries

A sample is `reps` launches between two HIP events after the state (codes, positions, scores) is put back to the prompt, so
every arm appends at the same positions; the figure is the window over reps, the median over `rounds` samples with their
minimum and maximum.  The arms' first tokens are compared: 1 == 2 == 3 bit for bit, 4 differs where the redraw does."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, D, TOP_K, PROMPT = 32, 1024, 50, 64


def main():
    from valle2_amd import kernels
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=9)
    args = ap.parse_args()
    torch.cuda.init()
    argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p]
    libs = {}
    for name, path in (('old', args.old), ('new', args.new)):
        lib = C.CDLL(str(Path(path).resolve()), mode=C.RTLD_LOCAL)
        for fn in ('vh_sample_step_rows', 'vh_sample_step_wide_rows'):
            getattr(lib, fn).restype = C.c_int
            getattr(lib, fn).argtypes = argtypes
        lib.vh_version.restype = C.c_int
        libs[name] = lib
    print(f'old: vh_version {libs["old"].vh_version()}  new: vh_version {libs["new"].vh_version()}  '
          f'{torch.cuda.get_device_name(0)}  rows {B}  top_k {TOP_K}  d {D}  reps {args.reps}  rounds {args.rounds}', flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    width = PROMPT + 3 + args.reps + 8
    for fn, V in (('vh_sample_step_rows', 1025), ('vh_sample_step_wide_rows', 1025), ('vh_sample_step_wide_rows', 4096)):
        g = torch.Generator().manual_seed(V)
        logits = (2.0 * torch.randn(B, V, generator=g)).cuda()
        logits[:, V - 1] = -30.0                                         # no row draws EOS and finishes inside a window
        emb = torch.randn(V + 1, D, generator=g).cuda()
        pe = torch.randn(width, D, generator=g).cuda()
        codes0 = torch.full((B, width), V - 1, dtype=torch.int64)
        codes0[:, 0] = V
        top = logits.cpu().topk(TOP_K, dim=1).indices
        codes0[:, 1:PROMPT] = top[:, torch.arange(PROMPT - 1) % TOP_K]      # every survivor of the row stands in its prompt
        codes0 = codes0.cuda()
        codes, x = codes0.clone(), torch.empty(B, D, device='cuda')
        pos = torch.empty(B, dtype=torch.int32, device='cuda')
        clen = torch.empty(B, dtype=torch.int32, device='cuda')
        score = torch.empty(B, device='cuda')
        eos_count = torch.zeros(width, dtype=torch.int32, device='cuda')
        base = [(1000 + b, b % 4, TOP_K, 1.0, 1.0) for b in range(B)]
        arms = {'1 parent': ('old', [r + (0, 0) for r in base]), '2 words zero': ('new', [r + (0, 0) for r in base]),
                '3 no trigger': ('new', [r + (10, 9) for r in base]), '4 all trigger': ('new', [r + (2 ** 31 - 1, 0) for r in base])}
        records = {k: kernels.pack_row_sampling(v[1]).cuda() for k, v in arms.items()}

        def reset():
            codes.copy_(codes0)
            pos.fill_(PROMPT)
            clen.fill_(PROMPT + 40)
            score.zero_()
            eos_count.zero_()

        def launch(arm):
            rc = getattr(libs[arms[arm][0]], fn)(logits.data_ptr(), V, V, V - 1, records[arm].data_ptr(), codes.data_ptr(), width,
                                               eos_count.data_ptr(), None, score.data_ptr(), emb.data_ptr(), pe.data_ptr(),
                                               pos.data_ptr(), clen.data_ptr(), x.data_ptr(), B, D, stream)
            assert rc == 0, rc

        def sample(arm):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch(arm)
            e1.record()
            e1.synchronize()
            assert int(pos.max()) == PROMPT + args.reps < width
            return e0.elapsed_time(e1) / args.reps * 1e3

        first, rows = {}, {}
        for arm in arms:                                                 # warm-up: every arm's code path, and the first tokens
            sample(arm)
            first[arm], rows[arm] = codes[:, PROMPT].clone(), codes.clone()
        ts = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                ts[arm].append(sample(arm))
        same = all(torch.equal(rows['1 parent'], rows[a]) for a in ('2 words zero', '3 no trigger'))
        moved = int((first['4 all trigger'] != first['2 words zero']).sum())
        med = {a: sorted(v)[len(v) // 2] for a, v in ts.items()}
        print(f'{fn} V={V}: rows of arms 1, 2 and 3 bit-equal over {args.reps} steps: {same}; first tokens arm 4 moved in {moved} of {B} rows')
        for a, v in ts.items():
            print(f'  {a:14s} median {med[a]:7.2f} us per launch (min {min(v):7.2f}, max {max(v):7.2f})  / parent {med[a] / med["1 parent"]:.3f}',
                  flush=True)


if __name__ == '__main__':
    main()
