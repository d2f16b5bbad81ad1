"""What the per-row length bounds cost in the per-row samplers: tools/ab_length_bounds.py OLD.so NEW.so [--reps 100]
[--rounds 7].  OLD.so is the PARENT commit's library, NEW.so this commit's; both are loaded with ctypes next to each other
in ONE process on ONE device (as tools/ab_lib.py does).  vh_sample_step_rows[_bounded] at V = 1025 and
vh_sample_step_wide_rows[_bounded] at V = 4096, 32 rows, top_k = 50, tok_p = 1, d = 1024, arms alternating:

  0 parent       OLD.so, vh_sample_step[_wide]_rows
  1 no limits    NEW.so, the _bounded entry with limits == NULL: the kernel instantiation without the bounds, the parent's code
  2 all zero     NEW.so, an array of zero records: the instantiation with them, one 8-byte block-uniform load per row and no
                 bound set
  3 min active   NEW.so, min_new beyond the window on every row: every step also loads pos_base and the row's last token and
                 writes -inf over the EOS score (EOS is out of reach in these logits anyway: the same tokens come out)
  4 all forced   NEW.so, max_new = 1 with the row one token in: every row is forced at every launch (no draw at all)
  0r parent, rewound   arm 0 measured the way arm 4 has to be, see below

A sample is `reps` launches between two HIP events after the state (codes, positions, scores) is put back to the prompt, so
every arm appends at the same positions; the figure is the window over reps, the median over `rounds` samples with their
minimum and maximum (the spread).  A forced row writes EOS and is a finished row from the next launch on, so arm 4 rewinds the
positions (one fill kernel) before every launch; arm 0r does the same on the parent, and arm 4 is read against 0r, not 0.
Arms 0 to 3 must append bit-equal rows.  The last line of each block puts the all-zero arm's difference from the parent
beside the parent's own spread: an attached array of zeros is kept for every call with per-row sampling only while that
difference stays within the spread."""
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
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    torch.cuda.init()
    head = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    tail = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p]
    libs = {}
    for name, path in (('old', args.old), ('new', args.new)):
        lib = C.CDLL(str(Path(path).resolve()), mode=C.RTLD_LOCAL)
        for fn in ('vh_sample_step_rows', 'vh_sample_step_wide_rows'):
            getattr(lib, fn).restype = C.c_int
            getattr(lib, fn).argtypes = head + tail
            if name == 'new':
                getattr(lib, fn + '_bounded').restype = C.c_int
                getattr(lib, fn + '_bounded').argtypes = head + [C.c_void_p] + tail
        lib.vh_version.restype = C.c_int
        libs[name] = lib
    print(f'old: vh_version {libs["old"].vh_version()}  new: vh_version {libs["new"].vh_version()}  '
          f'{torch.cuda.get_device_name(0)}  rows {B}  top_k {TOP_K}  d {D}  reps {args.reps}  rounds {args.rounds}', flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    width = PROMPT + 3 + args.reps + 8
    for fn, V in (('vh_sample_step_rows', 1025), ('vh_sample_step_wide_rows', 4096)):
        g = torch.Generator().manual_seed(V)
        logits = (2.0 * torch.randn(B, V, generator=g)).cuda()
        logits[:, V - 1] = -30.0                                         # no row draws EOS and finishes inside a window
        emb = torch.randn(V + 1, D, generator=g).cuda()
        pe = torch.randn(width, D, generator=g).cuda()
        codes0 = torch.full((B, width), V - 1, dtype=torch.int64)
        codes0[:, 0] = V
        codes0[:, 1:PROMPT] = torch.randint(0, V - 1, (B, PROMPT - 1), generator=g)
        codes0 = codes0.cuda()
        codes, x = codes0.clone(), torch.empty(B, D, device='cuda')
        pos = torch.empty(B, dtype=torch.int32, device='cuda')
        pos_base = torch.full((B,), PROMPT - 1, dtype=torch.int32, device='cuda')      # every row is one token in
        clen = torch.empty(B, dtype=torch.int32, device='cuda')
        score = torch.empty(B, device='cuda')
        eos_count = torch.zeros(width + 8, dtype=torch.int32, device='cuda')
        records = kernels.pack_row_sampling([(1000 + b, b % 4, TOP_K, 1.0, 1.0) for b in range(B)]).cuda()
        lim = {k: kernels.pack_row_limits([v] * B).cuda() for k, v in (('zero', (0, 0)), ('min', (10 ** 6, 0)), ('forced', (0, 1)))}
        # arm -> (library, limits: False = the _rows entry, None = _bounded with NULL, rewind the positions before every launch)
        arms = {'0 parent': ('old', False, False), '1 no limits': ('new', None, False), '2 all zero': ('new', lim['zero'], False),
                '3 min active': ('new', lim['min'], False), '4 all forced': ('new', lim['forced'], True),
                '0r parent, rewound': ('old', False, True)}

        def reset():
            codes.copy_(codes0)
            pos.fill_(PROMPT)
            clen.fill_(PROMPT + 40)
            score.zero_()
            eos_count.zero_()

        def launch(arm):
            lib, limits, rewind = arms[arm]
            if rewind:
                pos.fill_(PROMPT)
            a = [logits.data_ptr(), V, V, V - 1, records.data_ptr()]
            b = [codes.data_ptr(), width, eos_count.data_ptr(), pos_base.data_ptr(), score.data_ptr(), emb.data_ptr(), pe.data_ptr(),
                 pos.data_ptr(), clen.data_ptr(), x.data_ptr(), B, D, stream]
            if limits is False:
                rc = getattr(libs[lib], fn)(*a, *b)
            else:
                rc = getattr(libs[lib], fn + '_bounded')(*a, None if limits is None else limits.data_ptr(), *b)
            assert rc == 0, rc

        def sample(arm):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch(arm)
            e1.record()
            e1.synchronize()
            assert int(pos.max()) == PROMPT + (1 if arms[arm][2] else args.reps) < width
            return e0.elapsed_time(e1) / args.reps * 1e3

        rows = {}
        for arm in arms:                                                 # warm-up: every arm's code path, and the rows it appends
            sample(arm)
            rows[arm] = codes.clone()
        ts = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                ts[arm].append(sample(arm))
        same = all(torch.equal(rows['0 parent'], rows[a]) for a in ('1 no limits', '2 all zero', '3 min active'))
        forced = bool((rows['4 all forced'][:, PROMPT] == V - 1).all())
        med = {a: sorted(v)[len(v) // 2] for a, v in ts.items()}
        print(f'{fn} V={V}: rows of arms 0, 1, 2 and 3 bit-equal over {args.reps} steps: {same}; every row of arm 4 forced: {forced}')
        for a, v in ts.items():
            against = '0r parent, rewound' if arms[a][2] else '0 parent'
            print(f'  {a:20s} median {med[a]:7.2f} us per launch (min {min(v):7.2f}, max {max(v):7.2f})  / {against[:2].strip()} {med[a] / med[against]:.3f}',
                  flush=True)
        spread = max(ts['0 parent']) - min(ts['0 parent'])
        diff = med['2 all zero'] - med['0 parent']
        print(f'  all zero - parent: {diff:+.2f} us; spread of the parent\'s {args.rounds} runs: {spread:.2f} us; within the spread: {diff <= spread}',
              flush=True)


if __name__ == '__main__':
    main()
