"""Training at head widths other than 64: the flash route (kernels.attn_rows_hd with lse + kernels.attn_rows_hd_bwd:
vh_attn_rows_hd_lse / vh_attn_rows_hd_bwd) against the materialised route (kernels.attn_generic + the five products of
autograd.QkvAttentionAnyHeadDimFn), in ONE process, same model, same batch, alternating; the switch kernels.ATTN_HD_FLASH picks
the route per step.  configs[3]'s AR model (12L / d_model 512 / dff 2048, LayerNorm, dropout as configured: training mode)
with n_heads changed so that the head width is 32 (16 heads) and 128 (4 heads), B = 16, configs[3]'s own lengths (tokens
40..120, codes 225..900).  If the materialised route does not fit in memory at B = 16 the batch is halved until it does, and
the B used is printed.

  step       ValleAR.training_step + backward: wall time between two device synchronisations, median over --reps repetitions with
             the spread (max - min) beside it, the two routes alternating; torch.cuda.max_memory_allocated of each route (peak
             above nothing: absolute, weights and gradients included).  Dropout is live, so the two losses printed are different
             draws (tests/test_attn_rows_hd_bwd_gpu.py compares the routes with dropout off).
  attention  one layer's shapes (B, h, T, hd; the step's prefix mask and lengths): flash forward + backward (3 launches)
             against the seven materialised launches (S, softmax, O; dV, dP, dS, dQ, dK), --inner calls per timed window.

    python tools/ab_train_attn_hd.py [--batch 16] [--reps 7] [--inner 10]      (one JSON line per head width)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def summary(v):
    return dict(ms_median=round(statistics.median(v), 3), ms_spread=round(max(v) - min(v), 3), ms=[round(x, 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--layers', type=int, default=12)
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp(prefix='ab_train_attn_hd_'))    # ConfigValle() mkdirs under the CWD
    import torch

    from valle2_amd import ConfigValle, _lib, autograd as A, get_model_class, kernels as K, synth
    assert torch.cuda.is_available(), 'ab_train_attn_hd.py measures on the HIP device; there is nothing to report without one'
    dev = 'cuda'

    for n_heads in (16, 4):
        cfg = ConfigValle(d_model=512, n_heads=n_heads, dim_feedforward=2048, num_layers=args.layers, norm='LayerNorm')
        hd = cfg.d_model // n_heads
        m = get_model_class('ValleAR')(cfg)
        m.load_state_dict(synth.make_state_dict(cfg, 'ValleAR', seed=5, rich=True))
        m = m.to(dev).train()

        def step(batch, switch):
            K.ATTN_HD_FLASH = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.zero_grad(set_to_none=True)
            loss = m.training_step(batch)
            loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, float(loss.detach())

        B = args.batch
        while True:                                            # the largest B <= --batch at which both routes fit
            batch = synth.synth_ar_batch(cfg, B, seed=9100)
            batch = {k: (v if k.endswith('_lens') else v.to(dev)) for k, v in batch.items()}
            try:
                losses = {}
                for name, sw in (('materialized', False), ('flash', True)):     # warm-up of every shape the timed steps use
                    for _ in range(2):
                        losses[name] = step(batch, sw)[1]
                break
            except torch.cuda.OutOfMemoryError:
                m.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                assert B > 1, 'the materialised route does not fit at B = 1'
                B //= 2
        tx, ty = int(max(batch['tokens_lens'])), int(max(batch['codes_lens']))
        T = tx + ty
        ms = {'materialized': [], 'flash': []}
        for _ in range(args.reps):
            for name, sw in (('materialized', False), ('flash', True)):         # alternate the two routes
                ms[name].append(step(batch, sw)[0])
        peak = {}
        for name, sw in (('materialized', False), ('flash', True)):
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            step(batch, sw)
            peak[name] = torch.cuda.max_memory_allocated()
        m.zero_grad(set_to_none=True)

        # ---- the attention launches alone, on one layer's shapes
        d = cfg.d_model
        g = torch.Generator().manual_seed(hd)
        qkv = torch.randn(B * T, 3 * d, generator=g).to(dev)
        dout = torch.randn(B * T, d, generator=g).to(dev)
        out = torch.empty(B * T, d, device=dev)
        grad = torch.empty(B * T, 3 * d, device=dev)
        view3 = lambda t: tuple(t.view(B, T, 3, n_heads, hd)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        view1 = lambda t: t.view(B, T, n_heads, hd).permute(0, 2, 1, 3)
        (q, k, v), (dq, dk, dv), o, do = view3(qkv), view3(grad), view1(out), view1(dout)
        kv_len = (batch['codes_lens'].to(torch.int64) + tx).to(device=dev, dtype=torch.int32)
        spec = dict(mode=K.MASK_PREFIX, x_len=tx, kv_len=kv_len)
        scale = hd ** -0.5
        lse2 = torch.empty(B, n_heads, T, device=dev)

        def flash():
            K.attn_rows_hd(q, k, v, o, scale, lse2=lse2, **spec)
            K.attn_rows_hd_bwd(q, k, v, o, do, lse2, dq, dk, dv, scale, **spec)

        def materialized():
            P = K.attn_generic(q, k, v, o, scale, **spec)
            tp = P.stride(2)
            dP = torch.empty(B, n_heads, T, tp, device=dev)[..., :T]
            A._mm(P, do, dv, a_kmajor=True, b_kmajor=True)
            A._mm(do, v, dP)
            _lib.check(_lib.lib().vh_softmax_bwd(P.data_ptr(), dP.data_ptr(), tp, B * n_heads * T, T, scale, _lib.stream()),
                       'vh_softmax_bwd')
            A._mm(dP, k, dq, b_kmajor=True)
            A._mm(dP, q, dk, a_kmajor=True, b_kmajor=True)

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.inner

        routes = {'materialized': materialized, 'flash': flash}
        grads = {}
        for name, fn in routes.items():
            window(fn)
            grads[name] = grad.clone()
        at = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                at[name].append(window(fn))
        K.ATTN_HD_FLASH = None
        report = dict(head_dim=hd, n_heads=n_heads, layers=cfg.num_layers, batch=B, batch_asked=args.batch, T=T, x_len=tx,
                      reps=args.reps, loss={k_: round(v_, 6) for k_, v_ in losses.items()},
                      step={k_: summary(v_) for k_, v_ in ms.items()},
                      step_flash_over_materialized=round(statistics.median(ms['flash']) / statistics.median(ms['materialized']), 3),
                      peak_bytes=peak, peak_gib={k_: round(v_ / 2 ** 30, 3) for k_, v_ in peak.items()},
                      kept_score_maps_gib=round(cfg.num_layers * B * n_heads * T * T * 4 / 2 ** 30, 3),
                      attention={k_: summary(v_) for k_, v_ in at.items()}, attention_inner=args.inner,
                      attention_flash_over_materialized=round(statistics.median(at['flash']) /
                                                              statistics.median(at['materialized']), 3),
                      attention_grad_max_abs_diff=float((grads['flash'] - grads['materialized']).abs().max()))
        print(json.dumps(report), flush=True)
        del m, qkv, dout, out, grad, grads
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
