"""Many-row attention at head widths other than 64: the flash kernel (kernels.attn_rows_hd, vh_attn_rows_hd) against the
materialised route (kernels.attn_generic: S = Q K^T, row softmax, O = P V with the (B, h, T, T) map in memory) in ONE
process, same inputs, alternating; kernels.attn_hd_route under the switch kernels.ATTN_HD_FLASH picks the route per call.

The attention launches of one layer alone, on the views the stack hands them (the per-head column blocks of a (rows, 3 d)
projection at d_model 512), timed by events on their own dispatch, at 16 heads (width 32) and 4 heads (width 128); 8 heads
(width 64: vh_attn_rows over the cache layout, which the switch does not reach) runs beside them as context:

  prompt   the bench's prompt-pass shape: 32 rows x 1024 keys, prefix-LM mask (256 text keys)
  nar      configs[2]'s stage shape: 64 rows x 1024 keys, full mask

Every figure is the median over --reps timed repetitions after one warm call per route, with the spread (max - min) beside
it.  Peak allocated bytes over one call of each route are printed too.  With --errors the worst error of both routes
against float64 on the kernel test's inputs is appended.  The stack does not call the flash kernel yet, so
there is no whole-stack case.

    python tools/ab_attn_hd.py [--reps 7] [--heads 16,4] [--errors]   (one JSON line per case; profiles/ab_attn_hd.log)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

D = 512
ROWS, TEXT = 32, 256                          # bench.py's prompt: 256 text + BOS + 767 codec tokens = 1024 keys
NAR_B = 64


def med(v):
    return dict(median=round(statistics.median(v), 3), spread=round(max(v) - min(v), 3), all=[round(x, 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--heads', default='16,4')
    ap.add_argument('--errors', action='store_true')
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_attn_hd_'))          # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import kernels as K
    assert torch.cuda.is_available(), 'ab_attn_hd.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def ab(name, head, fn, timer, routes):
        """fn() under every route of `routes` ({label: switch value}), alternating; one JSON line."""
        rep = dict(case=name, n_heads=head, head_dim=D // head, reps=args.reps)
        ms = {r: [] for r in routes}
        for r, sw in routes.items():                           # warm-up + peak memory of every route
            K.ATTN_HD_FLASH = sw
            fn()
            rep[f'{r}_peak_bytes'] = peak(fn)
        for _ in range(args.reps):
            for r, sw in routes.items():
                K.ATTN_HD_FLASH = sw
                ms[r].append(timer(fn))
        for r in routes:
            rep[f'{r}_ms'] = med(ms[r])
        if 'flash' in routes:
            rep['flash_over_materialized'] = round(rep['flash_ms']['median'] / rep['materialized_ms']['median'], 3)
        K.ATTN_HD_FLASH = None
        print(json.dumps(rep), flush=True)

    both = {'materialized': False, 'flash': True}
    for head in [int(h) for h in args.heads.split(',')] + [8]:
        hd = D // head
        routes = both if hd != 64 else {'width64': None}
        # ---- the attention launches of one layer alone -------------------------------------------------------------------
        for name, Bq, mode, xl in (('attn of one prompt layer (32 x 1024, prefix)', ROWS, K.MASK_PREFIX, TEXT),
                                   ('attn of one nar layer (64 x 1024, full)', NAR_B, K.MASK_FULL, 0)):
            Tn = 1024
            qkv = torch.randn(Bq * Tn, 3 * D, generator=torch.Generator().manual_seed(2)).to(dev)
            out = torch.empty(Bq * Tn, D, device=dev)
            q, k, v = (qkv.view(Bq, Tn, 3, head, hd)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
            o = out.view(Bq, Tn, head, hd).permute(0, 2, 1, 3)
            if hd == 64:
                kc, vc = k.contiguous(), v.contiguous()
                qc = qkv[:, :D].contiguous()
                fn = lambda: K.attn_rows(qc, kc, vc, out, Bq, head, Tn, Tn, mode, x_len=xl)
            else:
                def fn():
                    route = K.attn_rows_hd if K.attn_hd_route(hd, dict(mode=mode)) == 'flash' else K.attn_generic
                    route(q, k, v, o, hd ** -0.5, mode=mode, x_len=xl, x_len_dev=None, kv_len=None)
            ab(name, head, fn, events, routes)
            del qkv, out
        torch.cuda.empty_cache()

    if args.errors:
        # worst |error| of both routes against float64 on the kernel test's inputs (B 2, h 3, T 200, the prefix mask at 33)
        Bq, h, Tn, xl = 2, 3, 200, 33
        for hd in (16, 20, 32, 48, 96, 100, 128):
            qkv = torch.randn(Bq * Tn, 3 * h * hd, generator=torch.Generator().manual_seed(1000 * hd))
            q, k, v = (qkv.view(Bq, Tn, 3, h, hd)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
            s = (q.double() @ k.double().transpose(-1, -2)) * hd ** -0.5
            i, j = torch.arange(Tn)[:, None], torch.arange(Tn)[None, :]
            s = s.masked_fill(~((j < xl) | ((i >= xl) & (j <= i))), float('-inf'))
            ref = torch.softmax(s, -1) @ v.double()
            qd = qkv.to(dev)
            qv, kv_, vv = (qd.view(Bq, Tn, 3, h, hd)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
            err = {}
            for r, fn in (('flash', K.attn_rows_hd), ('materialized', K.attn_generic)):
                out = torch.zeros(Bq * Tn, h * hd, device=dev)
                fn(qv, kv_, vv, out.view(Bq, Tn, h, hd).permute(0, 2, 1, 3), hd ** -0.5, mode=K.MASK_PREFIX, x_len=xl,
                   x_len_dev=None, kv_len=None)
                err[r] = (out.cpu().view(Bq, Tn, h, hd).permute(0, 2, 1, 3).double() - ref).abs().max().item()
            print(json.dumps(dict(case='max |error| against float64 (B 2, h 3, T 200, prefix 33)', head_dim=hd,
                                  flash=float(f'{err["flash"]:.3e}'), materialized=float(f'{err["materialized"]:.3e}'))), flush=True)


if __name__ == '__main__':
    main()
