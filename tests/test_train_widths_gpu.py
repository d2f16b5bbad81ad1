"""Training at every model width and row count it serves, against float64.

A. Whole models: one training step (loss, every parameter's gradient) at d_model 576 .. 2048 against the float64 oracle
   differentiated by torch autograd on the CPU; d_model 2112 is refused before a gradient exists.
B. The training-side row kernels directly — LayerNorm / AdaLN backward, cross entropy, the row softmax pair, the embedding
   scatter, column sums, the AdaLN projections — at the widths that pick each instantiation with a partly filled last
   slot, and at the row counts from which a wave walks more than one row.

Tolerances.  Per-element quantities keep those of tests/test_train_gpu.py (atol 2e-5 + rtol 1e-4; dlogits 1e-7 + 1e-4;
the adaproj weight / bias gradients 1e-6 + 1e-4; whole-model loss rtol 1e-5, gradients 1e-3 of the parameter's gradient
norm).  Sums over rows (dgamma, dbeta, dscale, dshift, dcol, embedding tables, colsum) grow with the row count, so each
is allowed SUM_MARGIN = 4 times the error that the SAME sum has when plain fp32 torch computes it on the CPU, one row
added after the other — measured against float64 on the same inputs by tests/test_train_widths_cpu.py, which asserts
that what it measures stays at or below the figure written next to the case here (the measurement plus 10 % for a CPU
whose vector units round a row's mean differently, rounded up to two digits).  The figures come from the reference's
arithmetic, never from a kernel; the margin covers another order of additions and the atomics.  The cross-entropy loss, one
scalar, has a worked-out bound instead (oracle_runners.check_ce)."""
import pytest
import torch
import torch.nn.functional as F

from tests import oracle_runners as R
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- A. whole models ---------------------------------------------------------------------------------------------------------


def _step(cls_name, kw, sd, batch, stage):
    from tests.test_models_gpu import build
    model = build(cls_name, kw, sd)            # eval mode: dropout off
    b = {k: v.clone() for k, v in batch.items()}
    loss = model.training_step(b) if stage is None else model.training_step(b, stage=stage)
    assert loss.requires_grad
    loss.backward()
    return model, loss.detach().cpu()


@pytest.mark.parametrize('case,cls_name,stage', R.TRAIN_WIDTH_RUNS, ids=[f'{c}-{m[5:]}' for c, m, _ in R.TRAIN_WIDTH_RUNS])
def test_training_step_vs_float64_oracle(case, cls_name, stage):
    """What each case reaches (R.TRAIN_WIDTHS): base / d896 layernorm_bwd_kernel<4> with a masked last slot, d1152 / d1536 /
    d2048 <8> (never launched before), d640 the node-by-node stack at head width 64 (dim_feedforward 1296), odd_heads the
    fused stack at d_model = 64 * 9: EncoderLayerFn.backward folds linear_1's bias gradient into the GEMM by
    dim_feedforward % 128 (1152 here: folded) and takes the d_model-wide bias gradients from the LayerNorm backward's
    column sums, which have no such limit — nothing of it keys on d_model % 128."""
    from tests.test_train_gpu import _grad_check
    kw, sd, batch = R.train_width_inputs(case, cls_name)
    cfg = C.cfg_of(kw)
    ref_loss, params = R.oracle_training_loss(sd, cfg, batch, cls_name, stage)
    model, loss = _step(cls_name, kw, sd, batch, stage)
    print(f'{case} {cls_name}: loss {float(loss):.7f} oracle {float(ref_loss):.7f}')
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-6)
    if cls_name == 'ValleAR':
        used = sorted(k for k in params if not k.endswith('.pe'))
    else:
        used = sorted(k for k, v in params.items() if v.grad is not None and v.grad.abs().sum() > 0)
        assert f'stage_embs.{stage - 1}.word_embeddings.weight' in used
        for n, p in model.named_parameters():      # parameters the stage does not touch get no/zero grad
            if n not in used:
                assert p.grad is None or float(p.grad.abs().sum()) == 0.0, n
    print(f'worst relative gradient error {_grad_check(model, params, used):.2e} over {len(used)} parameters')
    del model
    _, again = _step(cls_name, kw, sd, batch, stage)           # a fresh model from the same state dict
    torch.testing.assert_close(again.double(), ref_loss, rtol=1e-5, atol=1e-6)


def test_d_model_beyond_2048_is_refused_before_any_gradient():
    """d_model 2112 / 33 heads passes every forward kernel (they end at 4096): the loss used to come out, and backward() stopped
    at the top layer's vh_layernorm_bwd (d <= 2048) AFTER the head's and that layer's FeedForward gradients were written.
    transformer_train now refuses the width itself, naming the limit, before a graph exists."""
    from tests.test_models_gpu import build
    from valle2_amd import _lib
    kw, sd, batch = R.train_width_inputs('beyond', 'ValleAR')
    model = build('ValleAR', kw, sd)
    with pytest.raises(_lib.VhError, match=r'd_model <= 2048.*2112'):
        model.training_step({k: v.clone() for k, v in batch.items()}).backward()
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():                                      # (the forward-only path still serves the width)
        assert bool(torch.isfinite(model.training_step({k: v.clone() for k, v in batch.items()})))


# ---- B. row kernels ----------------------------------------------------------------------------------------------------------
# LayerNorm backward: (rows, d, adaptive, row mean, with dres + dcol), then the fp32 emulation's measured error per summed
# quantity.  9 rows: every instantiation (d <= 256: <1>, <= 512: <2>, <= 1024: <4>, else <8>) with a partly filled last slot
# (132 = 33 column groups, 260 = 65, 516 = 129, 640 = 160, 768 = 192, 1028 = 257, 1536 = 384) and the full one (2048).
# >= 2048 rows: 2048 waves walk the rows, so (2048, 128) gives every wave one row through the strided loop, 2053 gives five
# waves a second row (look-ahead at 512, none at 768), 4100 two or three rows per wave (look-ahead), 2600 one or two at <8>.
LN_CASES = {
    (9, 132, False, 0.3, False): {'dgamma': 1.4e-06, 'dbeta': 7.8e-07},
    (9, 132, True, 0.3, False): {'dgamma': 1.1e-06, 'dbeta': 1.2e-06, 'dscale': 1.2e-06, 'dshift': 7.8e-07},
    (9, 260, False, 0.3, False): {'dgamma': 1.2e-06, 'dbeta': 7.8e-07},
    (9, 260, True, 0.3, False): {'dgamma': 1.3e-06, 'dbeta': 7.8e-07, 'dscale': 1.3e-06, 'dshift': 7.8e-07},
    (9, 516, False, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 8.1e-07},
    (9, 516, True, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 1.2e-06, 'dscale': 1.8e-06, 'dshift': 8.1e-07},
    (9, 640, False, 0.3, False): {'dgamma': 1.7e-06, 'dbeta': 1.2e-06},
    (9, 640, True, 0.3, False): {'dgamma': 1.7e-06, 'dbeta': 9.8e-07, 'dscale': 1.7e-06, 'dshift': 1.2e-06},
    (9, 768, False, 0.3, False): {'dgamma': 1.3e-06, 'dbeta': 9.6e-07},
    (9, 768, True, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 1.4e-06, 'dscale': 1.4e-06, 'dshift': 9.6e-07},
    (9, 1028, False, 0.3, False): {'dgamma': 1.9e-06, 'dbeta': 8.3e-07},
    (9, 1028, True, 0.3, False): {'dgamma': 1.9e-06, 'dbeta': 9.6e-07, 'dscale': 1.7e-06, 'dshift': 8.3e-07},
    (9, 1536, False, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 9.7e-07},
    (9, 1536, True, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 1.2e-06, 'dscale': 1.6e-06, 'dshift': 9.7e-07},
    (9, 2048, False, 0.3, False): {'dgamma': 1.4e-06, 'dbeta': 1.4e-06},
    (9, 2048, True, 0.3, False): {'dgamma': 1.8e-06, 'dbeta': 1.5e-06, 'dscale': 2.1e-06, 'dshift': 1.4e-06},
    (2048, 128, False, 0.3, False): {'dgamma': 0.00017, 'dbeta': 0.00016},
    (2048, 128, True, 0.3, False): {'dgamma': 0.0002, 'dbeta': 0.00021, 'dscale': 0.00014, 'dshift': 0.00016},
    (2053, 512, False, 0.3, False): {'dgamma': 0.00025, 'dbeta': 0.00021},
    (2053, 512, True, 0.3, False): {'dgamma': 0.00017, 'dbeta': 0.00023, 'dscale': 0.00027, 'dshift': 0.00021},
    (4100, 256, False, 0.3, False): {'dgamma': 0.0003, 'dbeta': 0.00034},
    (4100, 256, True, 0.3, False): {'dgamma': 0.0005, 'dbeta': 0.00035, 'dscale': 0.00027, 'dshift': 0.00034},
    (2053, 768, False, 0.3, False): {'dgamma': 0.00022, 'dbeta': 0.00018},
    (2053, 768, True, 0.3, False): {'dgamma': 0.00022, 'dbeta': 0.00023, 'dscale': 0.00022, 'dshift': 0.00018},
    (2600, 1028, False, 0.3, False): {'dgamma': 0.00024, 'dbeta': 0.00028},
    (2600, 1028, True, 0.3, False): {'dgamma': 0.00029, 'dbeta': 0.00026, 'dscale': 0.00035, 'dshift': 0.00028},
    (2053, 512, True, 0.3, True): {'dgamma': 0.00017, 'dbeta': 0.00023, 'dscale': 0.00027, 'dshift': 0.00021, 'dcol': 0.00021},
    (9, 1028, True, 50.0, False): {'dgamma': 2.2e-05, 'dbeta': 9.6e-07, 'dscale': 2e-05, 'dshift': 8.3e-07},
    (2053, 768, True, 50.0, False): {'dgamma': 0.00029, 'dbeta': 0.00023, 'dscale': 0.00029, 'dshift': 0.00018},
}


@pytest.mark.parametrize('key', list(LN_CASES), ids=lambda k: '-'.join(str(v) for v in k))
def test_layernorm_backward_vs_float64(key):
    from valle2_amd import autograd as A
    rows, d, ada, mean, dres = key
    inp = R.ln_inputs(rows, d, mean=mean, dres=dres)
    ref = R.ln_reference(inp, ada)
    dev = {k: v.to(DEV).requires_grad_(k != 'dy' and k != 'dres') for k, v in inp.items()}
    s, t = (dev['scale'], dev['shift']) if ada else (None, None)
    y = A.layer_norm(dev['x'], dev['gamma'], dev['beta'], s, t)
    R.check_close('y', y, ref['y'])
    if dres:        # the call EncoderLayerFn.backward makes: residual gradient added, column sums of the result, AdaLN sums into dst
        dcol = torch.zeros(d, device=DEV)
        dst = torch.zeros(2, d, device=DEV)
        dx, dg, db, _ = A._ln_bwd(dev['x'].detach(), dev['gamma'].detach(), dev['beta'].detach(), s.detach() if ada else None,
                                  dev['dy'], dev['dres'], dcol, 1e-5, dst if ada else None)
        got = dict(dx=dx, dgamma=dg, dbeta=db, dscale=dst[0], dshift=dst[1], dcol=dcol)      # (dcol also against the columns of THIS dx)
    else:
        y.backward(dev['dy'])
        got = dict(dx=dev['x'].grad, dgamma=dev['gamma'].grad, dbeta=dev['beta'].grad)
        if ada:
            got.update(dscale=dev['scale'].grad, dshift=dev['shift'].grad)
    for name, measured in LN_CASES[key].items():
        print(f'{name}: worst error {R.worst(got[name], ref[name]):.3e} (fp32 emulation {measured:.3e})')
    R.check_ln(got, ref, LN_CASES[key])


# Cross entropy: (rows, V, ld, amplitude).  8229 rows: the grid is capped at 2048 workgroups of 4 waves = 8192 rows in flight, so 37
# waves walk a second row; V = 4097 / 16384: the wide vocabularies; ld = V + 7: a column slice of a wider buffer (ldd stays V);
# amplitude 80: exp(80) overflows fp32 unless the row maximum is taken off first.
CE_CASES = [(8192 + 37, 1025, None, None), (45, 4097, None, None), (9, 16384, None, None), (45, 1025, 1025 + 7, None),
            (45, 1025, None, 80.0)]


@pytest.mark.parametrize('key', CE_CASES, ids=lambda k: '-'.join(str(v) for v in k))
def test_cross_entropy_vs_float64(key):
    from valle2_amd import autograd as A
    rows, V, ld, amp = key
    logits, target = R.ce_inputs(rows, V, ld, amp)
    ref = R.ce_reference(logits, target, 3.0)
    buf = torch.as_strided(logits, (rows, ld or V), (ld or V, 1)).to(DEV)          # the whole buffer; the kernel sees a column slice
    lg = buf[:, :V].requires_grad_()
    assert lg.stride(0) == (ld or V)
    loss = A.CrossEntropyFn.apply(lg, target.to(DEV))
    print(f'loss {float(loss.detach()):.7f} reference {float(ref["loss"]):.7f} error {R.worst(loss, ref["loss"]):.3e}')
    (3.0 * loss).backward()                                     # a non-unit upstream gradient
    R.check_ce(loss, lg.grad, ref, rows)


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('name', list(R.SOFTMAX_CASES))
def test_softmax_rows_and_backward_vs_float64(name, pad):
    """vh_softmax_rows / vh_softmax_bwd (the recomputed-probability path of every head width other than 64) in place on
    (B, h, Tq, ld) buffers: Tk no multiple of 64, Tq < Tk, per-row prefix lengths, mask + pad, one query; the columns
    beyond Tk of a padded row stay as they were."""
    from valle2_amd import _lib, kernels as K
    B, h, Tq, Tk, mode = R.SOFTMAX_CASES[name]
    S, dP, _, spec = R.softmax_inputs(name)
    ref = R.softmax_reference(name)
    ld = Tk + pad
    bufs = []
    for src in (S, dP):
        b = torch.full((B, h, Tq, ld), 123.0)
        b[..., :Tk] = src
        bufs.append(b.to(DEV))
    P, dS = bufs
    spec = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in spec.items()}
    K.softmax_rows(P, ld, B, h, Tq, Tk, R.SOFTMAX_SCALE, mode=dict(full=K.MASK_FULL, prefix=K.MASK_PREFIX, explicit=K.MASK_EXPLICIT)[mode], **spec)
    R.check_close('P', P[..., :Tk], ref['P'])
    kept = P.clone()
    _lib.check(_lib.lib().vh_softmax_bwd(P.data_ptr(), dS.data_ptr(), ld, B * h * Tq, Tk, R.SOFTMAX_SCALE, _lib.stream()), 'vh_softmax_bwd')
    R.check_softmax(P[..., :Tk], dS[..., :Tk], ref)
    assert torch.equal(P, kept), 'the backward wrote to P'
    assert bool((P[..., Tk:] == 123.0).all()) and bool((dS[..., Tk:] == 123.0).all()), 'columns beyond Tk were written'


# Embedding scatter: (d, T, t0) -> measured error of the fp32 scatter-add.  d = 132 / 768 / 2048: one, three and eight turns
# of the 256-column loop, the first two ending inside a turn; T = 37 / 107 / 17: the last run of 16 positions partly filled;
# t0 = 5: the part starts inside the gradient buffer's rows (EmbedConcatFn's second part).
EMBED_CASES = {
    (132, 37, 0): 4.2e-06,
    (768, 107, 5): 2e-05,
    (2048, 17, 0): 3.4e-06,
}


@pytest.mark.parametrize('key', list(EMBED_CASES), ids=lambda k: '-'.join(str(v) for v in k))
def test_embedding_backward_vs_float64(key):
    from valle2_amd import autograd as A
    from valle2_amd.synth import sinusoid_table
    d, T, t0 = key
    tabs, ids = R.embed_inputs(d, T)
    vocab = tabs[0].shape[0]
    pe = sinusoid_table(d, 128)
    dy = torch.randn(3, t0 + T, d, generator=R._g(35))
    dt = [t.to(DEV).requires_grad_() for t in tabs]
    ids_dev = ids.to(DEV)
    assert not ids_dev[..., 1].is_contiguous()                # the kernel reads each codebook's ids as a strided column
    ref_out = sum(F.embedding(ids[..., j], tabs[j].double()) for j in range(3)) + pe[:T, 0].double()
    if t0 == 0:
        out = A.EmbedSumPeFn.apply(ids_dev, pe.to(DEV), 0, None, *dt)
        ref_tabs = R.embed_table_grads(ids, dy, vocab)
    else:           # a first part of t0 positions reading table 0 only, then the three-codebook part at row offset t0
        first = ids[:, :t0, 0].contiguous()
        out = A.EmbedConcatFn.apply([(first.to(DEV), pe.to(DEV), 0, [0], None), (ids_dev, pe.to(DEV), 0, [0, 1, 2], None)], *dt)
        ref_out = torch.cat([F.embedding(first, tabs[0].double()) + pe[:t0, 0].double(), ref_out], dim=1)
        ref_tabs = R.embed_table_grads(ids, dy[:, t0:], vocab)
        ref_tabs[0] = ref_tabs[0] + R.embed_table_grads(first[..., None], dy[:, :t0], vocab)[0]
    R.check_close('out', out, ref_out)
    out.backward(dy.to(DEV))
    for j in range(3):
        print(f'table {j}: worst error {R.check_sum(f"table {j}", dt[j].grad, ref_tabs[j], EMBED_CASES[key]):.3e}')


# Column sums: (rows, cols, ld) -> measured error of the fp32 sum.  One row and four columns; 63 / 65 rows either side of
# the 64-row slab; 260 columns: a second column block of four; ld > cols; 2053 x 2048: 33 slabs onto every column.
COLSUM_CASES = {
    (1, 4, 4): 5e-08,
    (63, 260, 260): 4.7e-06,
    (65, 768, 1000): 6.5e-06,
    (2053, 2048, 2048): 0.00037,
}


@pytest.mark.parametrize('key', list(COLSUM_CASES), ids=lambda k: '-'.join(str(v) for v in k))
def test_colsum_adds_onto_out_vs_float64(key):
    from valle2_amd import _lib
    rows, cols, ld = key
    x, out0 = R.colsum_inputs(rows, cols, ld)
    buf = torch.as_strided(x, (rows, ld), (ld, 1)).to(DEV)
    out = out0.to(DEV)
    _lib.check(_lib.lib().vh_colsum(buf.data_ptr(), ld, _lib.ptr(out), rows, cols, _lib.stream()), 'vh_colsum')
    print(f'worst error {R.check_sum("colsum", out, R.colsum_reference(x, out0), COLSUM_CASES[key]):.3e}')


@pytest.mark.parametrize('n,N,K_', [(4, 1536, 768), (4, 4096, 2048), (3, 264, 132)])
def test_adaproj_forward_backward_vs_float64(n, N, K_):
    """AdaProjFn at the widths of the wide NAR models: K = 768 (adaproj_*_kernel<4>, last slot masked), 2048 (<8>, full),
    132 (<1>, masked; N = 264 is no multiple of the 8 / 16 rows a wave owns)."""
    from valle2_amd import autograd as A
    emb = torch.randn(1, K_, generator=R._g(70))
    ws = [0.1 * torch.randn(N, K_, generator=R._g(71 + i)) for i in range(n)]
    bs = [torch.randn(N, generator=R._g(171 + i)) for i in range(n)]
    dout = torch.randn(n, N, generator=R._g(72))
    e64 = emb.double().requires_grad_()
    p64 = [t.double().requires_grad_() for t in ws + bs]
    ref = torch.cat([F.linear(e64, w, b) for w, b in zip(p64[:n], p64[n:])])
    ref.backward(dout.double())
    ed = emb.to(DEV).requires_grad_()
    pd = [t.to(DEV).requires_grad_() for pair in zip(ws, bs) for t in pair]
    out = A.AdaProjFn.apply(ed, *pd)
    R.check_close('out', out, ref)
    out.backward(dout.to(DEV))
    R.check_close('demb', ed.grad, e64.grad, atol=1e-4, rtol=1e-4)
    for i in range(n):
        R.check_close(f'dW[{i}]', pd[2 * i].grad, p64[i].grad, atol=1e-6)
        R.check_close(f'db[{i}]', pd[2 * i + 1].grad, p64[n + i].grad, atol=1e-6)
