"""Training on flash attention at head widths other than 64: `vh_attn_rows_hd_lse` + `vh_attn_rows_hd_bwd`
(kernels.attn_rows_hd(lse2=), kernels.attn_rows_hd_bwd) and the training node `autograd.QkvAttentionAnyHeadDimFn` behind the
switch `kernels.ATTN_HD_FLASH`.

The kernels are checked against float64 torch autograd on the CPU computed from the SAME strided views — q / k / v the per-head
column blocks of one (B T, 3 h hd + 4) buffer whose gap columns are NaN, out / dout those of (B T, h hd + 4) buffers, dq / dk /
dv the blocks of a gradient buffer shaped like qkv and NaN all over before the call — at every NB = ceil(hd / 32) instantiation
with a full and a partial last block, at row counts on both sides of the 32-row tile and the 128-row block, under every analytic
mask form.  Tolerances: `out` and `lse2` at test_kernels_gpu.py::test_attn_rows' own (atol 3e-5, rtol 2e-5; lse2 comes out of the
same fp32 score / exp2 pipeline as out and is O(10) here); dq, dk, dv at the project's tolerance for vh_attn_rows_bwd (atol 6e-5,
rtol 1e-4).  The materialised backward (the node's five products) runs on the same inputs as the yardstick and is held to the
same tolerance; its worst error is printed beside the flash kernels'.  Measured worst |error| per width over all cases: the
yardstick 2.2e-6 (hd 16) .. 4.2e-6 (hd 64) — it does not miss 6e-5 / 1e-4 at any width, so that tolerance stands for every width —
and the flash kernels out 0.8e-6 .. 1.7e-6, lse2 1.1e-6 .. 2.0e-6, dq 1.0e-6 .. 3.9e-6, dk 1.7e-6 .. 6.5e-6, dv 2.1e-6 .. 4.1e-6."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ATOL, RTOL = 3e-5, 2e-5             # out, lse2
G_ATOL, G_RTOL = 6e-5, 1e-4         # dq, dk, dv
H = 3
GAP = 4                             # NaN columns after the last head of every buffer row
# 1: a single row; 31 / 33: the 32-row tiles; 128 / 129: the 128-row block; 200: two blocks, the second partial
TS = [1, 31, 33, 128, 129, 200]


def g(seed):
    return torch.Generator().manual_seed(seed)


def _buffers(B, hd, T, seed):
    """CPU buffers: qkv (B T, 3 H hd + GAP) and dout (B T, H hd + GAP) random with NaN gap columns; out (like dout) and grad
    (like qkv) NaN all over."""
    ld, ldo = 3 * H * hd + GAP, H * hd + GAP
    qkv = torch.full((B * T, ld), float('nan'))
    qkv[:, :3 * H * hd] = torch.randn(B * T, 3 * H * hd, generator=g(seed))
    dout = torch.full((B * T, ldo), float('nan'))
    dout[:, :H * hd] = torch.randn(B * T, H * hd, generator=g(seed + 1))
    return qkv, dout, torch.full((B * T, ldo), float('nan')), torch.full((B * T, ld), float('nan'))


def _views3(buf, B, hd, T):
    """The three (B, H, T, hd) column-block views of a qkv-shaped buffer."""
    ld = buf.stride(0)
    x = buf.as_strided((B, T, 3, H, hd), (T * ld, ld, H * hd, hd, 1))
    return tuple(x[:, :, j].permute(0, 2, 1, 3) for j in range(3))


def _view1(buf, B, hd, T):
    ldo = buf.stride(0)
    return buf.as_strided((B, T, H, hd), (T * ldo, ldo, hd, 1)).permute(0, 2, 1, 3)


def _visible(B, T, mode, xl, kvl):
    """(B, T, T) bool, the header's semantics (Tq == Tk: query i sits at key position i)."""
    j = torch.arange(T)[None, None, :]
    p = torch.arange(T)[None, :, None]
    kv = torch.as_tensor(kvl).view(-1, 1, 1).expand(B, 1, 1)
    vis = (j < kv).expand(B, T, T)
    if mode == 'prefix':
        x = torch.as_tensor(xl).view(-1, 1, 1)
        vis = vis & ((j < x) | ((p >= x) & (j <= p)))
    return vis


def _ref64(q, k, v, do, vis):
    """float64 autograd on the CPU: out, lse2 (base 2, over the scaled scores), dq, dk, dv."""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    s = s.masked_fill(~vis[:, None], float('-inf'))
    out = torch.softmax(s, dim=-1) @ v
    out.backward(do.double())
    return out.detach(), torch.logsumexp(s.detach(), dim=-1) / math.log(2.0), q.grad, k.grad, v.grad


def _mask_cases(T):
    kvl = (T, max(1, T - 37))
    return [('full', 'full', 0, None, None), ('full+kv_len', 'full', 0, None, kvl), ('causal', 'prefix', 0, None, None),
            ('prefix33', 'prefix', 33, None, None), ('prefix_dev+kv_len', 'prefix', 0, (min(5, T), min(40, T)), kvl)]


def _spec(K, mode, xl, xl_dev, kvl):
    dev = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32, device=DEV)
    return dict(mode=K.MASK_PREFIX if mode == 'prefix' else K.MASK_FULL, x_len=xl, x_len_dev=dev(xl_dev), kv_len=dev(kvl))


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _flash(K, bufs_d, B, hd, T, spec):
    """Forward with lse + backward over the device buffers (qkv, dout, out, grad); returns lse2."""
    qkv_d, dout_d, out_d, grad_d = bufs_d
    q, k, v = _views3(qkv_d, B, hd, T)
    out = _view1(out_d, B, hd, T)
    lse2 = torch.full((B, H, T), float('nan'), device=DEV)
    K.attn_rows_hd(q, k, v, out, hd ** -0.5, lse2=lse2, **spec)
    K.attn_rows_hd_bwd(q, k, v, out, _view1(dout_d, B, hd, T), lse2, *_views3(grad_d, B, hd, T), hd ** -0.5, **spec)
    return lse2


def _materialized(K, qkv_d, dout_d, B, hd, T, spec):
    """The node's materialised route on the same views: attn_generic forward, five products backward."""
    from valle2_amd import _lib, autograd as A
    q, k, v = _views3(qkv_d, B, hd, T)
    do = _view1(dout_d, B, hd, T)
    out = torch.empty(B, H, T, hd, device=DEV)
    grad = torch.empty(B * T, 3 * H * hd, device=DEV)
    dq, dk, dv = _views3(grad, B, hd, T)
    P = K.attn_generic(q, k, v, out, hd ** -0.5, **spec)
    tp = P.stride(2)
    dP = torch.empty(B, H, T, tp, device=DEV)[..., :T]
    A._mm(P, do, dv, a_kmajor=True, b_kmajor=True)
    A._mm(do, v, dP)
    _lib.check(_lib.lib().vh_softmax_bwd(P.data_ptr(), dP.data_ptr(), tp, B * H * T, T, hd ** -0.5, _lib.stream()), 'vh_softmax_bwd')
    A._mm(dP, k, dq, b_kmajor=True)
    A._mm(dP, q, dk, a_kmajor=True, b_kmajor=True)
    return dq.cpu(), dk.cpu(), dv.cpu()


def _err(got, ref):
    return (got.double() - ref).abs().max().item()


def _check_case(K, B, hd, T, name, mode, xl, xl_dev, kvl, seed, worst):
    bufs = _buffers(B, hd, T, seed)
    qkv, dout, outb, gradb = bufs
    q, k, v = _views3(qkv, B, hd, T)
    vis = _visible(B, T, mode, xl if xl_dev is None else xl_dev, kvl if kvl is not None else (T,) * B)
    assert vis.any(-1).all(), 'every query of these cases sees a key'
    r_out, r_lse, r_dq, r_dk, r_dv = _ref64(q, k, v, _view1(dout, B, hd, T), vis)
    spec = _spec(K, mode, xl, xl_dev, kvl)
    bufs_d = [t.to(DEV) for t in bufs]
    lse2 = _flash(K, bufs_d, B, hd, T, spec).cpu()
    qkv_g, dout_g, out_g, grad_g = (t.cpu() for t in bufs_d)
    where = f'hd={hd} T={T} {name}'
    # nothing but the views was written
    assert _same_bits(qkv_g, qkv) and _same_bits(dout_g, dout), f'{where}: the q / k / v or dout buffer was written'
    assert out_g[:, H * hd:].isnan().all() and grad_g[:, 3 * H * hd:].isnan().all(), f'{where}: gap columns were written'
    got_out = _view1(out_g, B, hd, T)
    got = _views3(grad_g, B, hd, T)
    assert not got_out.isnan().any() and not lse2.isnan().any(), f'{where}: NaN in out or lse2'
    assert not grad_g[:, :3 * H * hd].isnan().any(), f'{where}: a gradient element was not written, or is NaN'
    # a second identical call: equal bits, and the backward leaves out alone
    again_d = [bufs_d[0], bufs_d[1], torch.full_like(bufs_d[2], float('nan')), torch.full_like(bufs_d[3], float('nan'))]
    lse2_again = _flash(K, again_d, B, hd, T, spec).cpu()
    assert _same_bits(again_d[2].cpu(), out_g) and _same_bits(lse2_again, lse2), f'{where}: the forward is not reproducible'
    assert _same_bits(again_d[3].cpu(), grad_g), f'{where}: the backward is not reproducible'
    # the yardstick on the same inputs
    mat = _materialized(K, bufs_d[0], bufs_d[1], B, hd, T, spec)
    errs = dict(out=_err(got_out, r_out), lse2=_err(lse2, r_lse), dq=_err(got[0], r_dq), dk=_err(got[1], r_dk),
                dv=_err(got[2], r_dv), mat=max(_err(m, r) for m, r in zip(mat, (r_dq, r_dk, r_dv))))
    for key, e in errs.items():
        worst[key] = max(worst.get(key, 0.0), e)
    print(f'attn_rows_hd_bwd {where}: max|err| vs float64 ' + ' '.join(f'{k_}={e:.2e}' for k_, e in errs.items()))
    msg = lambda what: (lambda m: f'{where} {what}: {m}')
    torch.testing.assert_close(got_out, r_out.float(), atol=ATOL, rtol=RTOL, msg=msg('out'))
    torch.testing.assert_close(lse2, r_lse.float(), atol=ATOL, rtol=RTOL, msg=msg('lse2'))
    for what, m, r in zip(('dq', 'dk', 'dv'), mat, (r_dq, r_dk, r_dv)):
        torch.testing.assert_close(m, r.float(), atol=G_ATOL, rtol=G_RTOL, msg=msg(f'materialised {what} (the yardstick)'))
    for what, t, r in zip(('dq', 'dk', 'dv'), got, (r_dq, r_dk, r_dv)):
        torch.testing.assert_close(t, r.float(), atol=G_ATOL, rtol=G_RTOL, msg=msg(what))


@pytest.mark.parametrize('hd', [16, 20, 32, 48, 64, 96, 100, 128])
def test_kernels_match_float64_on_strided_views(hd):
    from valle2_amd import kernels as K
    worst = {}
    for T in TS:
        for i, (name, mode, xl, xl_dev, kvl) in enumerate(_mask_cases(T)):
            _check_case(K, 2, hd, T, name, mode, xl, xl_dev, kvl, 1000 * hd + 10 * T + i, worst)
    print(f'attn_rows_hd_bwd hd={hd}: worst max|err| ' + ' '.join(f'{k_}={e:.2e}' for k_, e in worst.items()))


def test_a_row_without_keys_gets_zero_gradients():
    """kv_len = (T, 0, 17): batch row 1 has no visible key — its forward output is NaN (0 / 0), its lse2 -inf — and its dq,
    dk and dv are exactly zero; rows 0 and 2 are finite and match float64 (vh_attn_rows_bwd's precedent at width 64)."""
    from valle2_amd import kernels as K
    B, hd, T = 3, 32, 40
    kvl = (T, 0, 17)
    bufs = _buffers(B, hd, T, 4040)
    qkv, dout = bufs[0], bufs[1]
    bufs_d = [t.to(DEV) for t in bufs]
    _flash(K, bufs_d, B, hd, T, _spec(K, 'full', 0, None, kvl))
    grad = bufs_d[3].cpu()
    assert grad[:, 3 * H * hd:].isnan().all()
    got = _views3(grad, B, hd, T)
    for t, what in zip(got, ('dq', 'dk', 'dv')):
        assert torch.equal(t[1], torch.zeros_like(t[1])), f'{what} of the row without keys is not exactly zero'
        assert t.isfinite().all(), f'{what} is not finite'
    rows = [0, 2]
    q, k, v = (t[rows] for t in _views3(qkv, B, hd, T))
    vis = _visible(B, T, 'full', 0, kvl)[rows]
    _, _, r_dq, r_dk, r_dv = _ref64(q, k, v, _view1(dout, B, hd, T)[rows], vis)
    for t, r, what in zip(got, (r_dq, r_dk, r_dv), ('dq', 'dk', 'dv')):
        torch.testing.assert_close(t[rows], r.float(), atol=G_ATOL, rtol=G_RTOL, msg=lambda m: f'{what}: {m}')


@pytest.mark.parametrize('mode', ['full', 'prefix'])
def test_width_64_agrees_with_vh_attn_rows_lse_and_vh_attn_rows_bwd(mode):
    from valle2_amd import kernels as K
    B, hd, T, xl = 2, 64, 150, 41
    kvl = (T, T - 3)
    bufs_d = [t.to(DEV) for t in _buffers(B, hd, T, 64)]
    spec = _spec(K, mode, xl, None, kvl)
    lse2 = _flash(K, bufs_d, B, hd, T, spec)
    qkv_d, dout_d, out_d, grad_d = bufs_d
    q, k, v = _views3(qkv_d, B, hd, T)
    d = H * hd
    q2 = q.permute(0, 2, 1, 3).reshape(B * T, d).contiguous()
    kc, vc = k.contiguous(), v.contiguous()
    ref_out = torch.empty(B * T, d, device=DEV)
    ref_lse = torch.empty(B, H, T, device=DEV)
    K.attn_rows(q2, kc, vc, ref_out, B, H, T, T, spec['mode'], x_len=xl, kv_len=spec['kv_len'], lse2=ref_lse)
    ref_grad = torch.empty(B * T, 3 * d, device=DEV)
    K.attn_rows_bwd(q2, kc, vc, ref_out, dout_d[:, :d].contiguous(), ref_lse, ref_grad[:, :d], ref_grad[:, d:2 * d],
                    ref_grad[:, 2 * d:], B, H, T, spec['mode'], x_len=xl, kv_len=spec['kv_len'])
    torch.testing.assert_close(out_d[:, :d].cpu(), ref_out.cpu(), atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(lse2.cpu(), ref_lse.cpu(), atol=ATOL, rtol=RTOL)
    for j, what in enumerate(('dq', 'dk', 'dv')):
        torch.testing.assert_close(grad_d[:, j * d:(j + 1) * d].cpu(), ref_grad[:, j * d:(j + 1) * d].cpu(), atol=G_ATOL,
                                   rtol=G_RTOL, msg=lambda m: f'{what}: {m}')
    assert grad_d[:, 3 * d:].isnan().all() and out_d[:, d:].isnan().all()


# ---- the training node ---------------------------------------------------------------------------------------------------
def close(a, b, atol=2e-4, rtol=1e-4):
    torch.testing.assert_close(a.cpu(), b.cpu(), atol=atol, rtol=rtol)


def _node(K, monkeypatch, switch, x0, w0, B, T, h, spec, dy):
    """One forward + backward of the node under the switch; returns out, dx, dw, the call counts and the saved shapes."""
    from valle2_amd.autograd import QkvAttentionAnyHeadDimFn
    monkeypatch.setattr(K, 'ATTN_HD_FLASH', switch)
    K.reset_attn_hd_calls()
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        out = QkvAttentionAnyHeadDimFn.apply(x, w, B, T, h, spec)
    out.backward(dy)
    return out.detach(), x.grad, w.grad, dict(K.ATTN_HD_CALLS), dict(K.ATTN_HD_BWD_CALLS), saved


def _score_maps(saved, T):
    return [s for s in saved if len(s) >= 2 and s[-2] == T and s[-1] >= T]


@pytest.mark.parametrize('d,h', [(128, 4), (192, 4), (256, 2)])           # head widths 32, 48, 128
@pytest.mark.parametrize('mode', ['prefix', 'full'])
def test_node_takes_the_flash_pair_under_the_switch_and_agrees_with_the_materialised_route(monkeypatch, d, h, mode):
    from valle2_amd import kernels as K
    B, T = 2, 200
    x0 = torch.randn(B * T, d, generator=g(d + h)).to(DEV)
    w0 = (torch.randn(3 * d, d, generator=g(d)) * d ** -0.5).to(DEV)
    dy = torch.randn(B * T, d, generator=g(7)).to(DEV)
    spec = dict(mode=K.MASK_PREFIX if mode == 'prefix' else K.MASK_FULL, x_len=41,
                kv_len=torch.tensor([T, T - 29], dtype=torch.int32, device=DEV))
    out0, dx0, dw0, fwd0, bwd0, saved0 = _node(K, monkeypatch, False, x0, w0, B, T, h, spec, dy)
    out1, dx1, dw1, fwd1, bwd1, saved1 = _node(K, monkeypatch, True, x0, w0, B, T, h, spec, dy)
    assert fwd0 == {'flash': 0, 'materialized': 1} and bwd0 == {'flash': 0, 'materialized': 1}
    assert fwd1 == {'flash': 1, 'materialized': 0} and bwd1 == {'flash': 1, 'materialized': 0}
    assert _score_maps(saved0, T), 'the materialised route keeps P: the detector below must see it'
    assert not _score_maps(saved1, T), f'the flash route saved a (T, T) map: {saved1}'
    close(out1, out0)
    close(dx1, dx0)
    assert (dw1 - dw0).norm().item() < 1e-3 * dw0.norm().item()
    # an explicit mask keeps the materialised route whatever the switch says
    mask = torch.triu(torch.ones(T, T, dtype=torch.uint8, device=DEV), diagonal=1)
    _, _, _, fwd2, bwd2, saved2 = _node(K, monkeypatch, True, x0, w0, B, T, h, dict(mode=K.MASK_EXPLICIT, mask=mask, pad=None), dy)
    assert fwd2 == {'flash': 0, 'materialized': 1} and bwd2 == {'flash': 0, 'materialized': 1} and _score_maps(saved2, T)


# ---- models against the oracle, switch on ---------------------------------------------------------------------------------
@pytest.mark.parametrize('d,h', [(128, 4), (256, 2)])
def test_ar_model_trains_like_the_oracle_on_the_flash_route(monkeypatch, d, h):
    """The training half of test_head_dim_gpu.py's AR case (no generate) with the switch on."""
    from oracle import valle_oracle as O
    from tests.golden import cases as C
    from tests.test_train_gpu import _grad_check
    from valle2_amd import get_model_class, kernels as K, synth
    kw = dict(d_model=d, n_heads=h, dim_feedforward=2 * d, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=3,
              top_k=1, max_audio_len=24)
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=21, rich=True), cfg)
    model = get_model_class('ValleAR')(cfg)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = synth.synth_ar_batch(cfg, 3, tok_range=(5, 11), code_range=(20, 45), seed=8)
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    rl = O.ar_training_loss(params, cfg, batch)
    rl.backward()
    monkeypatch.setattr(K, 'ATTN_HD_FLASH', True)
    K.reset_attn_hd_calls()
    loss = model.training_step({k: v.clone() for k, v in batch.items()})
    torch.testing.assert_close(loss.detach().cpu(), rl.detach(), rtol=1e-5, atol=1e-6)
    loss.backward()
    _grad_check(model, params, sorted(k for k in params if not k.endswith('.pe')))
    assert K.ATTN_HD_CALLS == {'flash': cfg.num_layers, 'materialized': 0}
    assert K.ATTN_HD_BWD_CALLS == {'flash': cfg.num_layers, 'materialized': 0}


def test_nar_model_trains_like_the_oracle_on_the_flash_route(monkeypatch):
    """The training half of test_head_dim_gpu.py's NAR case (d 128 / 4 heads, AdaptiveLayerNorm, stage 4), switch on."""
    from oracle import valle_oracle as O
    from tests.golden import cases as C
    from tests.test_train_gpu import _grad_check
    from valle2_amd import get_model_class, kernels as K, synth
    kw = dict(d_model=128, n_heads=4, dim_feedforward=256, num_layers=2, dropout=0.0, norm='AdaptiveLayerNorm')
    cfg = C.cfg_of(kw)
    sd = synth.make_state_dict(cfg, 'ValleNAR', seed=5, rich=True)
    model = get_model_class('ValleNAR')(cfg)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = synth.synth_nar_batch(cfg, 3, n_tokens=9, n_frames=48, seed=3)
    stage = 4
    used = [k for k in sd if not k.endswith('.pe')]
    params = {k: v.clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    rl = O.nar_training_loss(params, cfg, batch, stage)
    rl.backward()
    monkeypatch.setattr(K, 'ATTN_HD_FLASH', True)
    K.reset_attn_hd_calls()
    loss = model.training_step(batch, stage=stage)
    torch.testing.assert_close(loss.detach().cpu(), rl.detach(), rtol=1e-5, atol=1e-6)
    loss.backward()
    _grad_check(model, params, sorted(k for k in used if params[k].grad is not None and params[k].grad.abs().sum() > 0))
    assert K.ATTN_HD_BWD_CALLS == {'flash': cfg.num_layers, 'materialized': 0}


def test_flash_route_keeps_no_score_map_in_memory(monkeypatch):
    """d 256 / 8 heads (width 32), 2 layers, B 2, T = 100 + 924 = 1024: the peak of an AR training step above its starting level
    is lower on the flash route by at least the kept P maps, num_layers x B x h x T x T x 4 bytes = 128 MiB."""
    from tests.golden import cases as C
    from valle2_amd import get_model_class, kernels as K, synth
    kw = dict(d_model=256, n_heads=8, dim_feedforward=512, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=1, top_k=1,
              max_audio_len=24)
    cfg = C.cfg_of(kw)
    model = get_model_class('ValleAR')(cfg)
    model.load_state_dict(synth.make_state_dict(cfg, 'ValleAR', seed=3, rich=False))
    model = model.to(DEV).eval()
    batch = synth.synth_ar_batch(cfg, 2, tok_range=(100, 100), code_range=(923, 923), seed=5)
    B, T = 2, 100 + 924

    def peak(switch):
        monkeypatch.setattr(K, 'ATTN_HD_FLASH', switch)
        K.reset_attn_hd_calls()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = model.training_step({k: v.clone() for k, v in batch.items()})
        loss.backward()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        assert K.ATTN_HD_BWD_CALLS == ({'flash': 2, 'materialized': 0} if switch else {'flash': 0, 'materialized': 2})
        del loss
        return top

    peak(False), peak(True)                    # gradients, workspaces and pools exist before anything is measured
    off, on = peak(False), peak(True)
    kept = cfg.num_layers * B * cfg.n_heads * T * T * 4
    print(f'peak above the starting level: materialised {off / 2 ** 20:.1f} MiB, flash {on / 2 ** 20:.1f} MiB, '
          f'kept P maps {kept / 2 ** 20:.0f} MiB')
    assert kept == 128 * 2 ** 20
    assert off - on >= kept
