"""The fast decode chain at d_model 640 / 768 / 896 (10, 12 and 14 heads of width 64): the folded-LayerNorm skinny GEMMs
(vh_linear_folded, vh_linear_qkv_folded and its fp16 append form), the fused FeedForward (vh_ffn_decode) and
ValleAR.generate_batch / generate on the cached decoder, fp32 and perf mode, against float64 torch, the recompute path, the
CPU oracle and the real reference's tokens (tests/golden/base_d_model.npz).

Kernel tolerance: as in test_wide_d_model_gpu.py — on the same inputs the largest error against float64 of the UNFUSED route
(kernels.layernorm + kernels.linear) is measured and the folded kernel is allowed twice that."""
import pytest
import torch
import torch.nn.functional as F

from tests.golden import cases as C
from tests.golden.gen_golden_base_d_model import BASE, PERF_MARGIN, base_d_model_inputs
from tests.oracle_runners import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WIDTHS = [640, 768, 896]
TUNE_ROW_GROUPS, TUNE_FFN_SLICE, TUNE_LN_STATS = 2, 7, 9


def g(seed):
    return torch.Generator().manual_seed(seed)


def _folded_case(K_, M, N, seed):
    a = 2.0 * torch.randn(M, K_, generator=g(seed)) + 0.5
    a[0] += 3.0                                            # a row whose mean exceeds its deviation
    a[M - 1] = 50.0 + torch.randn(K_, generator=g(seed + 1))   # mean 50, deviation 1
    w = 0.1 * torch.randn(N, K_, generator=g(seed + 2))
    gm, bt = 1 + 0.1 * torch.randn(K_, generator=g(seed + 3)), 0.1 * torch.randn(K_, generator=g(seed + 4))
    bias, res = torch.randn(N, generator=g(seed + 5)), torch.randn(M, N, generator=g(seed + 6))
    return a, w, gm, bt, bias, res


def _folded_against_unfused(K_, M, act):
    from valle2_amd import kernels as K
    N = 48
    a, w, gm, bt, bias, res = _folded_case(K_, M, N, seed=K_ + M)
    ref = F.linear(F.layer_norm(a.double(), (K_,), gm.double(), bt.double(), 1e-5), w.double(), bias.double())
    ref = (F.gelu(ref) if act else ref) + res.double()
    ad, wd, gd, bd, biasd, resd = (t.to(DEV) for t in (a, w, gm, bt, bias, res))
    unfused = K.linear(K.layernorm(ad, gd, bd), wd, biasd, resd, act=act)
    err_unfused = float((unfused.cpu().double() - ref).abs().max())
    out = K.linear_folded(ad, K.ln_fold(wd, gd, bd, biasd), residual=resd, act=act)
    err_folded = float((out.cpu().double() - ref).abs().max())
    print(f'linear_folded K={K_} M={M} act={act}: max|err| folded {err_folded:.3e} unfused {err_unfused:.3e} '
          f'ratio {err_folded / err_unfused:.2f}')
    assert err_unfused < 1e-4                              # the yardstick itself is sane
    assert err_folded <= 2 * err_unfused, (K_, M, act, err_folded, err_unfused)


@pytest.mark.parametrize('act', [0, 1], ids=['none', 'gelu'])
@pytest.mark.parametrize('M', [1, 4, 16, 17, 33, 64])
@pytest.mark.parametrize('K_', WIDTHS)
def test_linear_folded_within_twice_the_unfused_error(K_, M, act):
    _folded_against_unfused(K_, M, act)


@pytest.mark.parametrize('knob,value', [(TUNE_ROW_GROUPS, 2), (TUNE_LN_STATS, 1)], ids=['no_row_groups', 'row_statistics'])
@pytest.mark.parametrize('K_', WIDTHS)
def test_linear_folded_row_resident_forms(K_, knob, value):
    """Row groups switched off: 17 / 33 / 64 rows run the MT = 2 / 4 row-resident kernels (LN = 2) — except above 32 rows at 896,
    whose MT = 4 form is not built and which keep their row groups; VH_TUNE_LN_STATS = 1 sends every row count to LN = 2."""
    from valle2_amd import _lib
    lib = _lib.lib()
    try:
        lib.vh_set_tuning(knob, value)
        for M in (1, 17, 33, 64):
            _folded_against_unfused(K_, M, 1)
    finally:
        lib.vh_set_tuning(knob, 0)


@pytest.mark.parametrize('K_', WIDTHS)
def test_linear_folded_integer_exact_in_any_order(K_):
    """Rows of +-1 (mean 0, variance 1 exactly) against small-integer weights: every sum of the kernel is exact, so a
    permutation of k and every row grouping give the same bits."""
    from valle2_amd import kernels as K
    M, N = 40, 96
    gen = g(K_)
    x = torch.ones(M, K_)
    x[:, ::2] = -1
    x = x[:, torch.randperm(K_, generator=gen)]
    w = torch.randint(-2, 3, (N, K_), generator=gen).float()
    b = torch.randint(-2, 3, (N,), generator=gen).float()
    ones, zeros = torch.ones(K_, device=DEV), torch.zeros(K_, device=DEV)
    out = K.linear_folded(x.to(DEV), K.ln_fold(w.to(DEV), ones, zeros, b.to(DEV)))
    rs = 1.0 / (1.0 + 1e-5) ** 0.5                         # rstd of a unit-variance row
    torch.testing.assert_close(out.cpu(), (x @ w.T) * rs + b, atol=0, rtol=1e-6)
    perm = torch.randperm(K_, generator=gen)
    out_p = K.linear_folded(x[:, perm].contiguous().to(DEV), K.ln_fold(w[:, perm].contiguous().to(DEV), ones, zeros, b.to(DEV)))
    assert torch.equal(out_p, out)
    for rows in (1, 16, 17):                               # one row tile / 8-row groups / 16-row groups: the same bits per row
        part = K.linear_folded(x[:rows].to(DEV), K.ln_fold(w.to(DEV), ones, zeros, b.to(DEV)))
        assert torch.equal(part, out[:rows])


@pytest.mark.parametrize('K_', WIDTHS)
def test_linear_folded_row_with_an_outlier_head(K_):
    """The construction and the bound of test_linear_folded_wide_k_row_with_an_outlier_head: at these K the LN = 3 statistics
    are one-pass sums about the mean of the row's first 32 elements, and the products run on x - that shift, as in the 16-wave
    form.  Rows whose head is unrepresentative (30 +- 1, a constant 1000, -30 in front of a unit-normal rest) make dm = mean -
    shift large against the deviation of the rest — but the head is part of the row, so dm^2 <= K/32 var.  Bound, from that
    and fp32's 2^-24 (not from measurement):
      * var = sb/K - dm^2 with both operands <= (1 + K/32) var and about four roundings each way: the relative error of
        rstd is at most (1 + K/32) 2^-23, on outputs up to max |LN(x) W^T|;
      * acc - dm c1 with |dm| rstd <= sqrt(K/32): both sides up to sqrt(K/32) max|c1| in output units, a few roundings:
        sqrt(K/32) max|c1| 2^-22;
      * everything else is the unfused route's kind of error, measured on the same inputs and added.
    A constant row (variance 0 exactly) must come out finite and equal to c2."""
    from valle2_amd import kernels as K
    M, N = 6, 96
    gen = g(77 + K_)
    a = torch.randn(M, K_, generator=gen)
    a[0, :32] = 30.0 + torch.randn(32, generator=gen)
    a[1, :32] = 1000.0
    a[2, :32] = -30.0
    a[3] = 5.0                                             # a constant row: variance 0 exactly, output = c2
    w = 0.1 * torch.randn(N, K_, generator=gen)
    gm, bt = 1 + 0.1 * torch.randn(K_, generator=gen), 0.1 * torch.randn(K_, generator=gen)
    bias = torch.randn(N, generator=gen)
    y = F.linear(F.layer_norm(a.double(), (K_,), gm.double(), bt.double(), 1e-5), w.double())
    ref = y + bias.double()
    ad, wd, gd, bd, biasd = (t.to(DEV) for t in (a, w, gm, bt, bias))
    err_unfused = float((K.linear(K.layernorm(ad, gd, bd), wd, biasd).cpu().double() - ref).abs().max())
    out = K.linear_folded(ad, K.ln_fold(wd, gd, bd, biasd))
    err = (out.cpu().double() - ref).abs().max(1)[0]
    c1 = (w * gm).double().sum(1).abs().max()
    bound = (1 + K_ / 32) * 2.0 ** -23 * float(y.abs().max()) + (K_ / 32) ** 0.5 * float(c1) * 2.0 ** -22 + err_unfused
    print(f'outlier head K={K_}: per-row max|err| {[f"{float(e):.2e}" for e in err]} unfused {err_unfused:.2e} bound {bound:.2e}')
    assert bool(torch.isfinite(out).all())
    assert float(err.max()) <= bound, (K_, err, bound)
    torch.testing.assert_close(out[3].cpu(), F.linear(bt, w) + bias, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize('B', [1, 5, 40])
@pytest.mark.parametrize('d', WIDTHS)
def test_linear_qkv_folded_appends_k_v_at_cache_len_only_fp32_and_fp16(d, B):
    from valle2_amd import kernels as K
    H16 = K.H16
    h, S = d // 64, 24
    gen = g(d + B)
    x = (torch.randn(B, d, generator=gen) + 0.3).to(DEV)
    w = (0.05 * torch.randn(3 * d, d, generator=gen)).to(DEV)
    gamma = (1 + 0.1 * torch.randn(d, generator=gen)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=gen)).to(DEV)
    cache_len = torch.randint(0, S, (B,), generator=gen, dtype=torch.int32)
    folded = K.ln_fold(w, gamma, beta)
    kc = torch.full((B, h, S, 64), 7.25, device=DEV)
    vc = torch.full((B, h, S, 64), -3.5, device=DEV)
    q = torch.empty(B, d, device=DEV)
    K.linear_qkv_folded(x, folded, q, kc, vc, B, 1, h, cache_len=cache_len.to(DEV))
    y = F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5) @ w.double().T
    torch.testing.assert_close(q.double(), y[:, :d], atol=2e-5, rtol=1e-5)
    ek, ev = torch.full_like(kc, 7.25), torch.full_like(vc, -3.5)
    here = torch.zeros(B, h, S, 64, dtype=torch.bool, device=DEV)
    for b in range(B):
        ek[b, :, int(cache_len[b])] = y[b, d:2 * d].view(h, 64).float()
        ev[b, :, int(cache_len[b])] = y[b, 2 * d:].view(h, 64).float()
        here[b, :, int(cache_len[b])] = True
    torch.testing.assert_close(kc, ek, atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(vc, ev, atol=2e-5, rtol=1e-5)
    assert bool((kc[~here] == 7.25).all()) and bool((vc[~here] == -3.5).all())      # the sentinel everywhere else: exact
    # the 16-bit append: the fp32 form's values rounded to the build's format, within one unit in its last place
    k16 = torch.full((B, h, S, 64), 7.25, device=DEV, dtype=H16)
    v16 = torch.full((B, h, S, 64), -3.5, device=DEV, dtype=H16)
    q16 = torch.empty(B, d, device=DEV)
    K.linear_qkv_folded_kv16(x, folded, q16, k16, v16, h, cache_len.to(DEV))
    torch.testing.assert_close(q16.double(), y[:, :d], atol=2e-5, rtol=1e-5)
    for c16, c32, sentinel in ((k16, kc, 7.25), (v16, vc, -3.5)):
        assert bool((c16[~here].float() == sentinel).all())
        want = c32[here].to(H16)
        ulp = (want.view(torch.int16).int() - c16[here].view(torch.int16).int()).abs()      # same sign: adjacent bit patterns
        same_sign = (want.float() * c16[here].float()) >= 0
        assert bool(same_sign.all()) and int(ulp.max()) <= 1, (d, B, int(ulp.max()))


@pytest.mark.parametrize('d', WIDTHS)
def test_linear_qkv_folded_prompt_rows_take_the_row_resident_forms(d):
    """T > 1 has no row groups: 2 x 12 rows run MT = 2, 2 x 20 rows MT = 4 — which at 896 is not built (it would spill) and
    is refused naming the folded LayerNorm."""
    from valle2_amd import kernels as K
    from valle2_amd._lib import VhError
    h, S, T = d // 64, 24, 2
    gen = g(d)
    w = (0.05 * torch.randn(3 * d, d, generator=gen)).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=gen)).to(DEV), (0.1 * torch.randn(d, generator=gen)).to(DEV)
    folded = K.ln_fold(w, gamma, beta)
    for B in (12, 20):
        x = (torch.randn(B * T, d, generator=gen) + 0.3).to(DEV)
        kc, vc = torch.zeros(B, h, S, 64, device=DEV), torch.zeros(B, h, S, 64, device=DEV)
        q = torch.empty(B * T, d, device=DEV)
        if d == 896 and B == 20:
            with pytest.raises(VhError, match='folded LayerNorm'):
                K.linear_qkv_folded(x, folded, q, kc, vc, B, T, h)
            continue
        K.linear_qkv_folded(x, folded, q, kc, vc, B, T, h)
        y = (F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5) @ w.double().T).float()
        torch.testing.assert_close(q, y[:, :d], atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(kc[:, :, :T], y[:, d:2 * d].view(B, T, h, 64).transpose(1, 2), atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(vc[:, :, :T], y[:, 2 * d:].view(B, T, h, 64).transpose(1, 2), atol=2e-5, rtol=1e-5)
        assert bool((kc[:, :, T:] == 0).all()) and bool((vc[:, :, T:] == 0).all())


def _ffn_ref64(x, gm, bt, w1, b1, w2, b2):
    x, gm, bt, w1, b1, w2, b2 = (t.double() for t in (x, gm, bt, w1, b1, w2, b2))
    return x + F.linear(F.gelu(F.linear(F.layer_norm(x, (x.shape[1],), gm, bt, 1e-5), w1, b1)), w2, b2)


@pytest.mark.parametrize('dff_of', ['4d', '1296'])
@pytest.mark.parametrize('M', [1, 8, 19, 64])
@pytest.mark.parametrize('d', WIDTHS)
def test_ffn_decode_matches_float64(d, M, dff_of):
    """atol 1e-4 on O(1) rows (test_ffn_decode_matches_torch's), in place, reproducible, both slice widths where dff allows."""
    from valle2_amd import _lib
    from valle2_amd import kernels as K
    lib = _lib.lib()
    dff = 4 * d if dff_of == '4d' else 1296
    gen = g(300 + M + d + dff)
    x = torch.randn(M, d, generator=gen) + 0.2
    gm, bt = 1 + 0.1 * torch.randn(d, generator=gen), 0.1 * torch.randn(d, generator=gen)
    w1, b1 = 0.05 * torch.randn(dff, d, generator=gen), 0.1 * torch.randn(dff, generator=gen)
    w2, b2 = 0.05 * torch.randn(d, dff, generator=gen), 0.1 * torch.randn(d, generator=gen)
    ref = _ffn_ref64(x, gm, bt, w1, b1, w2, b2).float()
    folded = K.ln_fold(w1.to(DEV), gm.to(DEV), bt.to(DEV), b1.to(DEV))
    w2d, b2d = w2.to(DEV), b2.to(DEV)
    out = K.ffn_decode(x.to(DEV), folded, w2d, b2d)
    torch.testing.assert_close(out.cpu(), ref, atol=1e-4, rtol=2e-5)
    assert torch.equal(out, K.ffn_decode(x.to(DEV), folded, w2d, b2d)), 'not reproducible'
    xi = x.to(DEV)
    K.ffn_decode(xi, folded, w2d, b2d, out=xi)             # in place on the residual stream
    assert torch.equal(xi, out)
    try:
        for sw in (16, 32):
            if dff % sw == 0:
                lib.vh_set_tuning(TUNE_FFN_SLICE, sw)
                torch.testing.assert_close(K.ffn_decode(x.to(DEV), folded, w2d, b2d).cpu(), ref, atol=1e-4, rtol=2e-5)
    finally:
        lib.vh_set_tuning(TUNE_FFN_SLICE, 0)


@pytest.mark.parametrize('dff_of', ['4d', '1296'])
@pytest.mark.parametrize('d', WIDTHS)
def test_ffn_decode_integer_exact_and_strided(d, dff_of):
    """The construction of test_ffn_decode_integer_exact_and_strided (tests/test_kernels_gpu.py) at 19 rows: x and out as
    column blocks of wider buffers whose margins must stay untouched; a hidden tile of small integers survives phase 2
    bit for bit whatever the slice / wave / part order."""
    from valle2_amd import kernels as K
    M = 19
    dff = 4 * d if dff_of == '4d' else 1296
    gen = g(411 + d + dff)
    x = torch.ones(M, d)
    x[:, ::2] = -1
    x = x[:, torch.randperm(d, generator=gen)]
    w1 = torch.randint(-2, 3, (dff, d), generator=gen).float()
    b1 = torch.randint(-2, 3, (dff,), generator=gen).float()
    w2 = torch.randint(-2, 3, (d, dff), generator=gen).float()
    b2 = torch.randint(-2, 3, (d,), generator=gen).float()
    folded = K.ln_fold(w1.to(DEV), torch.ones(d, device=DEV), torch.zeros(d, device=DEV), b1.to(DEV))
    big_in = torch.full((M, d + 64), 7.0, device=DEV)
    big_in[:, 32:32 + d] = x.to(DEV)
    big_out = torch.full((M, d + 128), -3.0, device=DEV)
    K.ffn_decode(big_in[:, 32:32 + d], folded, w2.to(DEV), b2.to(DEV), out=big_out[:, 64:64 + d])
    rs = 1.0 / (1.0 + 1e-5) ** 0.5                         # rstd of a unit-variance row
    hid = F.gelu((x.double() @ w1.double().T) * rs + b1.double())
    ref = (x.double() + hid @ w2.double().T + b2.double()).float()
    torch.testing.assert_close(big_out[:, 64:64 + d].cpu(), ref, atol=2e-3, rtol=1e-5)
    assert bool((big_out[:, :64] == -3.0).all()) and bool((big_out[:, 64 + d:] == -3.0).all())
    assert bool((big_in[:, :32] == 7.0).all()) and bool((big_in[:, 32 + d:] == 7.0).all())
    w1z = torch.zeros(dff, d)
    b1i = torch.randint(0, 4, (dff,), generator=gen).float() * 8.0   # gelu(8k) == 8k in fp32 for k >= 1, gelu(0) = 0
    fz = K.ln_fold(w1z.to(DEV), torch.ones(d, device=DEV), torch.zeros(d, device=DEV), b1i.to(DEV))
    out = K.ffn_decode(x.to(DEV), fz, w2.to(DEV), b2.to(DEV))
    assert torch.equal(out.cpu(), x + (F.gelu(b1i)[None, :] @ w2.T) + b2)


@pytest.mark.parametrize('d', WIDTHS)
def test_ffn_decode_argument_checks(d):
    from valle2_amd import _lib
    from valle2_amd import kernels as K
    dff, M = 1296, 4
    folded = K.ln_fold(torch.randn(dff, d, device=DEV), torch.ones(d, device=DEV), torch.zeros(d, device=DEV))
    w2 = torch.randn(d, dff, device=DEV)
    x = torch.randn(M, d, device=DEV)
    with pytest.raises(_lib.VhError, match='w2'):
        K.ffn_decode(x, folded, w2[:, :1280].contiguous())
    need = _lib.lib().vh_ffn_decode_ws_bytes(M, d, dff)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    wf, c1, c2 = folded
    call = lambda nbytes: _lib.lib().vh_ffn_decode(x.data_ptr(), d, wf.data_ptr(), c1.data_ptr(), c2.data_ptr(), w2.data_ptr(),  # noqa: E731
                                                   None, out.data_ptr(), d, M, d, dff, 1e-5, ws.data_ptr(), nbytes, None)
    assert call(need - 1) < 0 and 'workspace' in _lib.lib().vh_last_error().decode()
    assert call(need) == 0
    torch.cuda.synchronize()


# ---- the decoder ----------------------------------------------------------------------------------------------------
def _model(kw, seed):
    from valle2_amd import get_model_class, synth
    cfg = C.cfg_of(kw)
    sd = synth.silence_eos(synth.make_state_dict(cfg, 'ValleAR', seed=seed, rich=True), cfg)
    m = get_model_class('ValleAR')(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, cfg


def _build(kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(kw))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _kw(d, **over):
    return dict(dict(d_model=d, n_heads=d // 64, dim_feedforward=2 * d, num_layers=2, dropout=0.0, norm='LayerNorm', num_beams=2,
                     top_k=1, max_audio_len=24), **over)


MAX_NEW = 24
# (state dict seed, utterance seed) per width, chosen on the CPU oracle so that every one of the 24 steps of utterance 0 is
# decided by at least 1e-4 (all five utterances: by 1e-3): the list of excused steps is asserted empty
DECODER_SEEDS = {640: (940, 1440), 768: (1069, 1569), 896: (1196, 1696)}


@pytest.mark.parametrize('d', WIDTHS)
def test_generate_batch_cached_equals_recompute_graph_and_eager(d):
    """2 and 40 rows, equal and ragged: the cached decoder's greedy tokens (graph and eager) are the recompute path's, graph
    == eager bit for bit, the folded chain and the fused FeedForward were taken."""
    from oracle import valle_oracle as O
    from valle2_amd import synth
    kw = _kw(d)
    sd_seed, utt_seed = DECODER_SEEDS[d]
    m, sd, cfg = _model(kw, seed=sd_seed)
    rc = _build(dict(kw, use_kv_cache=False), sd)
    utts = [synth.synth_utterance(cfg, 6 + 2 * i, 4 + i, 14 + 5 * i, seed=utt_seed + i) for i in range(5)]
    texts = [torch.cat([u[0], u[2]]).to(DEV) for u in utts]
    firsts = [u[1][:, 0].to(DEV) for u in utts]
    trace = {}
    O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *utts[0], trace=trace)
    near_tie = [t for t, mg in enumerate(trace['margin']) if mg < 1e-4]
    assert near_tie == [] and len(trace['margin']) == MAX_NEW, (d, trace['margin'])
    cases = [([texts[0]] * 2, [firsts[0]] * 2), (texts[:2], firsts[:2]), ([texts[0]] * 40, [firsts[0]] * 40),
             ([texts[i % 5] for i in range(40)], [firsts[i % 5] for i in range(40)])]
    for rows, fr in cases:
        want = rc.generate_batch(rows, fr, max_new=MAX_NEW)
        assert rc.last_generate_stats['kv_cache'] is False
        got = {}
        for use_graph in (True, False):
            got[use_graph] = out = m.generate_batch(rows, fr, max_new=MAX_NEW, use_graph=use_graph)
            st = m.last_generate_stats
            assert st['kv_cache'] is True and not st['shared_prompt'] and not st['kv_bf16']
            assert st['ln_folded'] is True and st['ffn_fused'] is True
            assert out.shape == want.shape and torch.equal(out, want), (d, len(rows), use_graph, out.cpu(), want.cpu())
        assert torch.equal(got[True], got[False]), (d, len(rows))


@pytest.mark.parametrize('d', WIDTHS)
def test_sampling_graph_equals_eager_under_one_seed(d):
    from valle2_amd import synth
    m, _, cfg = _model(_kw(d, top_k=50, num_beams=5), seed=400 + d)
    utt = synth.synth_utterance(cfg, 8, 6, 20, seed=3 + d)
    rows = [torch.cat([utt[0], utt[2]]).to(DEV)] * 5
    firsts = [utt[1][:, 0].to(DEV)] * 5
    outs = []
    for use_graph in (True, False):
        torch.manual_seed(1234)
        outs.append(m.generate_batch(rows, firsts, max_new=MAX_NEW, use_graph=use_graph).cpu())
        assert m.last_generate_stats['kv_cache'] is True and m.last_generate_stats['ln_folded'] is True
    assert torch.equal(outs[0], outs[1])
    assert len({tuple(r.tolist()) for r in outs[0]}) > 1, 'sampled rows must not be copies of each other'


@pytest.fixture(scope='module')
def oracle_traces():
    """The CPU oracle's single-beam run of the two fixture models, computed once for the tests below."""
    from oracle import valle_oracle as O
    out = {}
    for which in BASE:
        kw, sd, utt = base_d_model_inputs(which)
        trace = {}
        O.ar_generate(sd, C.cfg_of(dict(kw, num_beams=1)), *utt, trace=trace)
        out[which] = trace
    return out


@pytest.mark.parametrize('which', sorted(BASE))
def test_teacher_forced_logits_match_the_oracle(which, oracle_traces):
    kw, sd, utt = base_d_model_inputs(which)
    m = _build(dict(kw, num_beams=1), sd)
    trace = oracle_traces[which]
    n = len(trace['logits'])
    assert n == kw['max_audio_len']
    forced = torch.stack([t.reshape(-1)[0] for t in trace['tokens']])
    steps = [0, 1, 31, n - 1]
    text = torch.cat([utt[0], utt[2]]).to(DEV)
    m.generate_batch([text] * 2, [utt[1][:, 0].to(DEV)] * 2, max_new=n, forced=forced, keep_logits=steps)
    st = m.last_generate_stats
    assert st['kv_cache'] is True and st['ln_folded'] is True and st['ffn_fused'] is True
    for t in steps:
        err = float((st['logits'][t].cpu() - trace['logits'][t][:1]).abs().max())
        print(f'{which} step {t}: max |logit - oracle| = {err:.2e}')
        torch.testing.assert_close(st['logits'][t].cpu(), trace['logits'][t][:1].expand(2, -1), atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize('which', sorted(BASE))
def test_generate_matches_the_real_reference_on_every_step(which):
    gold = load_golden('base_d_model')
    kw, sd, utt = base_d_model_inputs(which)
    m = _build(kw, sd)
    out = m.generate(*[u.to(DEV) for u in utt]).cpu()
    st = m.last_generate_stats
    assert st['kv_cache'] is True and st['shared_prompt'] and st['ln_folded'] is True
    assert torch.equal(out, gold[f'tokens_{which}']), (out, gold[f'tokens_{which}'])
    text, first = torch.cat([utt[0], utt[2]]).to(DEV), utt[1][:, 0].to(DEV)
    n = kw['max_audio_len']
    shared = m.generate_batch([text] * 4, [first] * 4, max_new=n, shared_prompt=True)
    assert m.last_generate_stats['shared_prompt'] is True
    indep = m.generate_batch([text] * 4, [first] * 4, max_new=n)
    assert m.last_generate_stats['shared_prompt'] is False
    assert torch.equal(shared, indep)
    gen = indep[0, first.numel() + 1:].cpu()
    gen = gen[gen != m.eos_token]
    assert torch.equal(gen, gold[f'tokens_{which}'][: gen.numel()]) and gen.numel() == len(gold[f'tokens_{which}'])


# ---- perf mode at 768 -----------------------------------------------------------------------------------------------
KEEP = [0, 16, 32, 47]


@pytest.fixture(scope='module')
def d768():
    """The fp32 run of the d768 fixture model: free-running tokens and every step's teacher-forced logits."""
    kw, sd, utt = base_d_model_inputs('d768')
    m = _build(kw, sd)
    text, first = torch.cat([utt[0], utt[2]]).to(DEV), utt[1][:, 0].to(DEV)
    new = kw['max_audio_len']
    free = m.generate_batch([text] * 2, [first] * 2, max_new=new)
    pl = m.last_generate_stats['prompt_lens'][0]
    tokens = free[0, pl:pl + new].clone()
    m.generate_batch([text] * 2, [first] * 2, max_new=new, forced=tokens, keep_logits=list(range(new)))
    logits = torch.stack([m.last_generate_stats['logits'][t][0] for t in range(new)])
    top2 = torch.topk(logits, 2, dim=-1).values
    return dict(m=m, kw=kw, sd=sd, utt=utt, text=text, first=first, new=new, pl=pl, tokens=tokens, logits=logits,
                margin=(top2[:, 0] - top2[:, 1]).cpu())


def _perf_tol():
    from valle2_amd._lib import h16_dtype
    return 1.5e-2 if h16_dtype() == torch.float16 else 5e-2


@pytest.mark.parametrize('mode', ['kv', True], ids=['kv', 'full'])
@pytest.mark.parametrize('form', ['split', 'shared'])
def test_perf_mode_at_768_logits_and_tokens(d768, mode, form):
    """5 independent rows (60 (row, head) pairs: key splits) and 4 beams over a shared prompt.  Teacher-forced logits within
    the project's perf-mode bound of the fp32 run; greedy tokens equal the fp32 run's at every step whose fp32 margin exceeds
    ten times that bound — at least three quarters of the steps, asserted."""
    m, text, first, new, pl = d768['m'], d768['text'], d768['first'], d768['new'], d768['pl']
    tol = _perf_tol()
    assert tol * 10 <= PERF_MARGIN or tol == 5e-2
    rows = 5 if form == 'split' else 4
    kw = dict(perf_mode=mode, shared_prompt=form == 'shared')
    m.generate_batch([text] * rows, [first] * rows, max_new=new, forced=d768['tokens'], keep_logits=KEEP, **kw)
    st = m.last_generate_stats
    assert st['kv_bf16'] and st['ln_folded'] and st['shared_prompt'] == (form == 'shared')
    assert form != 'split' or st['n_split'] > 1
    assert st['prefill_bf16'] == (mode is True)            # 768 and dff 3072 are multiples of 128: the 16-bit prompt pass runs
    for t in KEEP:
        err = float((st['logits'][t] - d768['logits'][t][None]).abs().max())
        print(f'perf_mode={mode!r} {form} step {t}: max |logit - fp32| = {err:.2e} (bound {tol})')
        assert err <= tol, (mode, form, t, err)
    sure = d768['margin'] > 10 * tol
    assert float(sure.float().mean()) >= 0.75, f'only {int(sure.sum())} of {new} steps exceed ten times the bound'
    out = m.generate_batch([text] * rows, [first] * rows, max_new=new, **kw)
    assert out.shape[1] == pl + new
    # free-running: compare up to and including the first step that is not sure (a different token there changes the rest)
    first_unsure = int((~sure).nonzero()[0]) if bool((~sure).any()) else new
    same = (out[:, pl:] == d768['tokens'][None]).cpu()
    assert bool(same[:, :first_unsure].all()), (mode, form, out[:, pl:].tolist(), d768['tokens'].tolist())
    if bool(same.all()):
        return
    # beyond it the context may differ: teacher-force the fp32 tokens and compare the argmax on every sure step
    m.generate_batch([text] * rows, [first] * rows, max_new=new, forced=d768['tokens'], keep_logits=list(range(new)), **kw)
    arg = torch.stack([m.last_generate_stats['logits'][t].argmax(-1) for t in range(new)]).cpu()      # (new, rows)
    want = d768['logits'].argmax(-1).cpu()
    assert bool((arg[sure] == want[sure][:, None]).all())


@pytest.mark.parametrize('mode', ['kv', True], ids=['kv', 'full'])
def test_generate_takes_perf_mode_at_768_and_reuses_the_slot(d768, mode):
    m = _build(dict(d768['kw'], num_beams=4), d768['sd'])
    utt = [u.to(DEV) for u in d768['utt']]
    a = m.generate(*utt, perf_mode=mode)
    st = m.last_generate_stats
    assert st['kv_bf16'] and st['shared_prompt'] and st['ln_folded'] and not st['decoder_reused']
    assert st['prefill_bf16'] == (mode is True)
    b = m.generate(*utt, perf_mode=mode)
    st = m.last_generate_stats
    assert st['decoder_reused'] and st['slot_uses'] == 2 and st['kv_bf16']
    assert torch.equal(a, b) and a.dim() == 1 and 0 < a.numel() <= d768['new']


def test_perf_mode_fp32_prompt_pass_where_the_tile_kernels_do_not_serve_the_shape():
    """d640 has dim_feedforward 1296, not a multiple of 128: perf_mode=True takes the fp32 prompt pass and narrows it."""
    kw, sd, utt = base_d_model_inputs('d640')
    m = _build(kw, sd)
    gold = load_golden('base_d_model')
    out = m.generate(*[u.to(DEV) for u in utt], perf_mode=True)
    st = m.last_generate_stats
    assert st['kv_bf16'] and not st['prefill_bf16'] and st['ln_folded']
    assert out.dim() == 1 and 0 < out.numel() <= kw['max_audio_len']
    agree = float((out.cpu()[:8] == gold['tokens_d640'][:8]).float().mean())
    print(f'd640 perf_mode=True: {agree:.2f} of the first 8 tokens equal the reference')


def test_perf_mode_at_896_decodes_one_to_sixty_four_rows():
    from valle2_amd import synth
    m, _, cfg = _model(_kw(896, max_audio_len=8), seed=896)
    utt = synth.synth_utterance(cfg, 6, 4, 12, seed=896)
    text, first = torch.cat([utt[0], utt[2]]).to(DEV), utt[1][:, 0].to(DEV)
    for rows in (1, 17, 64):
        out = m.generate_batch([text] * rows, [first] * rows, max_new=8, perf_mode='kv')
        st = m.last_generate_stats
        assert st['kv_bf16'] and st['ln_folded'] and out.shape[0] == rows
        assert bool((out == out[:1]).all())                # replicated rows stay equal


def test_grouped_decoding_at_768_equals_two_generate_calls():
    from valle2_amd import synth
    kw = _kw(768, max_audio_len=16)
    m, sd, cfg = _model(kw, seed=1069)
    utts = [synth.synth_utterance(cfg, 6 + 3 * i, 4 + i, 14 + 6 * i, seed=1569 + i) for i in range(2)]
    want = [m.generate(*[u.to(DEV) for u in utt]).cpu() for utt in utts]
    got = m.generate_many([tuple(u.to(DEV) for u in utt) for utt in utts])
    assert m.last_generate_stats['ln_folded'] is True
    assert len(got) == 2
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b), (a, b)
