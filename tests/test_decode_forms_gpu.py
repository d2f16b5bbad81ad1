"""Every compiled form of the decode step's skinny GEMMs and of its attention, run on the GPU against float64.

The cases, inputs, references and bounds are tests/decode_forms.py's; tests/test_decode_forms_cpu.py shows (without a GPU) that
the cases cover every (FORM_TABLE row, epilogue) and every launch form, that each takes the form it is named for, that the
references are torch's, that plain fp32 arithmetic stays inside the bounds and that planted faults do not.  Before every
launch the form query is asked again under the knobs in force: a test id cannot claim a form it does not run.

GEMM (one test per form outside test_every_dispatched_form_without_layernorm_is_integer_exact): three launches on exact rows
(the three kinds of row rotated over the rows) against the per-element bound of decode_forms.gemm_exact_bound, one on ordinary
rows at atol 2e-5 / rtol 1e-5 (above K = 1024: within twice the unfused route's error on the same inputs, the yardstick of
test_wide_d_model_gpu).  The appending epilogues write q into a NaN buffer of row stride d + 8 and K / V at a random cache_len
of sentinel-filled caches; everything else must keep its bits; a 16-bit append lies between the float64 value minus and plus the
fp32 bound, each rounded to the build's format (decode_forms.stored16_outside: one unit in the last place wherever the value is
no cancellation).

Attention (one test per launch form): caches of 104 and of 8 rows (smaller than one 32-key burst), len_bias 0 and 1, q and out
with NaN pad columns, NaN in K and Inf in V beyond every length, NaN workspaces where the header asks for no initialisation,
six score sets.  Bound: the project's atol 2e-5 on the plain set; on the others 4 x the larger error against float64 of two
fp32 emulations on the same inputs (plain torch, and the chunked online softmax in base 2 with records merged in order), the
margin of test_attn_geometry_gpu: it covers another summation order and the hardware exp2.  ATTN_EMU_ERR records those errors,
the largest over every case, as measured on the CPU; the CPU file re-asserts them.  vh_attn_decode's records start as NaN too
(every split writes its record, an empty one included) with the ticket words behind them zero, as its in-launch combine asks.

Every test prints `FORM <family> <case>: <worst error over bound>`.  As first run on an MI355X (fp16 build; all 205 pass, the
whole file in 13 s, no test above 0.8 s), the largest figure per family:
  GEMM, forms                                  exact rows   ordinary rows
  no LayerNorm, 16-bit weights / d_model 192 (15)   0 (exact)    0.031
  LayerNorm in the operand load (45)                0.099        0.082
  folded, row-resident statistics (84)              0.192        0.094
  folded, fragment statistics, K <= 1024 (24)       0.162        0.061
  folded, fragment statistics, K > 1024 (8)         0.201        0.711 of twice the unfused route's error
  attention, forms     plain   peak    rising  falling  +200    -200
  decode (10)          0.021   0.160   0.113   0.174    0.204   0.198
  hd (12)              0.014   0.121   0.059   0.147    0.151   0.094
  kv16, kv16_split (4) 0.020   0.142   0.067   0.137    0.130   0.141
  shared (1)           0.027   0.345   0.160   0.215    0.174   0.155
  shared_groups (1)    0.047   0.292   0.205   0.198    0.208   0.173
  shared_kv16 (1)      0.035   0.212   0.170   0.213    0.199   0.151
No form needed a bound re-derived and no kernel bug was found."""
import ctypes as C

import pytest
import torch

from tests import decode_forms as D

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ATOL, RTOL = 2e-5, 1e-5                  # test_linear_qkv_folded_appends_k_v_at_cache_len_only_fp32_and_fp16's
S_CACHE, SENTINEL = 8, (7.25, -3.5)      # rows of the GEMM tests' K / V caches; what they are filled with (exact in fp16 and bf16)
# the larger of the two fp32 emulations' errors against float64, over every case and run of the set (measured on the CPU)
ATTN_EMU_ERR = {'plain': 6.0e-7, 'peak': 1.6e-6, 'rising': 4.3e-5, 'falling': 1.1e-6, 'plus200': 5.1e-5, 'minus200': 5.7e-5}


def attn_bound(score_set):
    return 2e-5 if score_set == 'plain' else 4 * ATTN_EMU_ERR[score_set]    # plain: test_attn_decode_long_context's atol


def excess(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 (or both are NaN pads) the bits must agree."""
    got, ref = got.double(), ref.double()
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    err = torch.where(same, torch.zeros_like(ref), (got - ref).abs() / bound.double().expand_as(ref))
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    return float(err.max())


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------
GEMM_CASES = D.gemm_cases()
# the decode step's two 16-bit-weight launches have no C entry point of their own (plan.hip calls them): their C++ symbols
W16_LINEAR = '_Z22vh_internal_linear_w16PKfiPKtS0_S0_iPfiiiiPv'
W16_QKV = '_Z38vh_internal_linear_qkv_folded_kv16_w16PKfiPKtS0_S0_PfiPtS4_PKiiiiifPv'


def _w16_functions(lib):
    P, I = C.c_void_p, C.c_int
    lin, qkv = getattr(lib, W16_LINEAR), getattr(lib, W16_QKV)     # AttributeError: the library no longer has the launch
    lin.restype, lin.argtypes = I, [P, I, P, P, P, I, P, I, I, I, I, P]
    qkv.restype, qkv.argtypes = I, [P, I, P, P, P, P, I, P, P, P, I, I, I, I, C.c_float, P]
    return lin, qkv


def _launch_gemm(c, x, w, bias, gamma, beta, act=False, res=None):
    """Run case c's entry point.  Returns (got, wf, kind): got = (out,) or (q, kcache, vcache) on the CPU, wf the matrix a
    16-bit-weight form multiplied by (else None)."""
    from valle2_amd import _lib
    from valle2_amd import kernels as K
    lib = _lib.lib()
    dev = lambda t: None if t is None else t.to(DEV)
    xd, wd, bd, gd, btd = dev(x), dev(w), dev(bias), dev(gamma), dev(beta)
    ln = D.gemm_ln(c)
    lnarg = (gd, btd, None, None, D.EPS) if ln == 1 else None
    wf_used = None
    if c.label.startswith('linear'):
        resd = dev(res)
        if c.label == 'linear+ln':
            out = K.linear(xd, wd, bd, resd, out=resd, act=int(act), ln=lnarg)
        elif c.label == 'linear_folded':
            out = K.linear_folded(xd, K.ln_fold(wd, gd, btd, bd), residual=resd, out=resd, act=int(act))
        else:
            assert c.label == 'linear_w16' and not act
            w16 = wd.to(K.H16).contiguous()
            wf_used = w16.float().cpu()
            out = resd if resd is not None else torch.empty(c.M, c.N, device=DEV)
            K.check(_w16_functions(lib)[0](xd.data_ptr(), xd.stride(0), w16.data_ptr(), K.ptr(bd), K.ptr(resd), c.N if resd is not None else 0,
                                           out.data_ptr(), out.stride(0), c.M, c.N, c.K, K.stream()), 'vh_internal_linear_w16')
        return (out.cpu(),), wf_used
    d, hd, B = c.K, D.gemm_head_dim(c), c.M // c.T
    h = d // hd
    kv16 = 'kv16' in c.label
    cl = D.gemm_cache_len(c, S_CACHE).to(DEV)
    q = torch.full((c.M, d + 8), float('nan'), device=DEV)
    kc = torch.full((B, h, S_CACHE, hd), SENTINEL[0], device=DEV, dtype=K.H16 if kv16 else torch.float32)
    vc = torch.full((B, h, S_CACHE, hd), SENTINEL[1], device=DEV, dtype=K.H16 if kv16 else torch.float32)
    qv = q[:, :d]
    folded = K.ln_fold(wd, gd, btd, bd) if ln >= 2 else None
    if c.label in ('qkv', 'qkv+ln'):
        K.linear_qkv(xd, wd, qv, kc, vc, B, c.T, h, cache_len=cl, ln=lnarg)
    elif c.label == 'qkv_folded':
        K.linear_qkv_folded(xd, folded, qv, kc, vc, B, c.T, h, cache_len=cl)
    elif c.label in ('qkv_hd', 'qkv_hd+ln'):
        K.linear_qkv_hd(xd, wd, qv, kc, vc, h, cl, ln=lnarg)
    elif c.label == 'qkv_folded_hd':
        K.linear_qkv_hd(xd, None, qv, kc, vc, h, cl, folded=folded)
    elif c.label == 'qkv_folded_kv16':
        K.linear_qkv_folded_kv16(xd, folded, qv, kc, vc, h, cl)
    else:
        assert c.label == 'qkv_folded_kv16_w16'
        wf16 = folded[0].to(K.H16).contiguous()
        c1 = wf16.double().sum(1).float().contiguous()           # of the ROUNDED matrix (engine.decode_weights16)
        wf_used = wf16.float().cpu()
        K.check(_w16_functions(lib)[1](xd.data_ptr(), xd.stride(0), wf16.data_ptr(), c1.data_ptr(), folded[2].data_ptr(), q.data_ptr(),
                                       q.stride(0), kc.data_ptr(), vc.data_ptr(), cl.data_ptr(), B, d, h, S_CACHE, D.EPS, K.stream()),
                'vh_internal_linear_qkv_folded_kv16_w16')
    return (q.cpu(), kc.cpu(), vc.cpu()), wf_used


def _compare(c, got, ref, bound, what):
    """Worst error over bound of a launch's outputs against the (M, N) reference; a QKV entry's through what its epilogue is to
    leave: NaN pads, sentinels and all.  A 16-bit append: decode_forms.stored16_outside, sentinels exact."""
    if len(got) == 1:
        return excess(got[0], ref, bound)
    hd = D.gemm_head_dim(c)
    args = (D.gemm_cache_len(c, S_CACHE), c.T, c.K // hd, hd, S_CACHE)
    want = D.scatter_qkv(ref, *args, SENTINEL, c.K + 8)
    tol = D.scatter_qkv(bound, *args, (0, 0), c.K + 8)
    worst = excess(got[0], want[0], tol[0])
    for g, w_, t in zip(got[1:], want[1:], tol[1:]):
        if g.dtype == torch.float32:
            worst = max(worst, excess(g, w_, t))
            continue
        bad = D.stored16_outside(g, w_, t)
        units = (w_.to(g.dtype).view(torch.int16).int() - g.view(torch.int16).int()).abs()[t > 0]
        assert bad == 0, f'{what}: {bad} elements of a 16-bit cache outside round16(reference -+ bound) (up to {int(units.max())} units from the rounded reference)'
    return worst


@pytest.mark.parametrize('i', range(len(GEMM_CASES)), ids=[D.gemm_case_id(c) for c in GEMM_CASES])
def test_gemm_form_against_float64(i):
    from valle2_amd import _lib
    from valle2_amd import kernels as K
    c = GEMM_CASES[i]
    lib = _lib.lib()
    ln = D.gemm_ln(c)
    try:
        D.set_knobs(lib, D.GEMM_KNOBS, c.knobs)
        assert D.gemm_query_form(lib, c) == c.form
        # ---- exact rows
        worst_exact = 0.0
        for rot in range(3):
            x, w, bias, gamma, beta = D.gemm_exact_inputs(c, rot)
            ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
            got, _ = _launch_gemm(c, x, w, bias, gamma, beta)
            worst_exact = max(worst_exact, _compare(c, got, ref, bound, f'exact rows {rot}'))
        # ---- ordinary rows
        act = bool(i % 2) and D.gemm_takes_act(c)
        x, w, bias, gamma, beta, res = D.gemm_ordinary_inputs(c)
        got, wf = _launch_gemm(c, x, w, bias, gamma, beta, act, res)
        if wf is None:
            ref = D.gemm_reference(x, w, bias, gamma, beta, act, res)
        elif ln == 0:
            ref = D.gemm_reference(x, wf, bias, None, None, act, res)
        else:
            ref = D.gemm_reference_folded(x, wf, beta.double() @ w.double().T + bias.double(), act, res)
        if c.K <= 1024:
            worst_ordinary = _compare(c, got, ref, ATOL + RTOL * ref.abs(), 'ordinary rows')
            note = 'of atol 2e-5 + rtol 1e-5'
        else:                                                    # the unfused route on the same inputs, allowed twice its error
            dev = lambda t: None if t is None else t.to(DEV)
            unfused = K.linear(K.layernorm(dev(x), dev(gamma), dev(beta)), dev(w), dev(bias), dev(res), act=int(act)).cpu()
            err_unfused = D.worst(unfused, ref)
            assert err_unfused < 1e-4
            worst_ordinary = _compare(c, got, ref, torch.full_like(ref, 2 * err_unfused), 'ordinary rows')
            note = f'of twice the unfused route\'s error {err_unfused:.2e}'
        print(f'FORM gemm {D.gemm_case_id(c)}: exact rows {worst_exact:.3f} of the bound, ordinary rows {worst_ordinary:.3f} {note}')
        assert worst_exact <= 1.0, f'exact rows: {worst_exact:.3g} x the bound'
        assert worst_ordinary <= 1.0, f'ordinary rows: {worst_ordinary:.3g} x the bound'
    finally:
        D.set_knobs(lib, D.GEMM_KNOBS, (0, 0, 0))


# ---- attention --------------------------------------------------------------------------------------------------------------------
ATTN_CASES = D.attn_cases()


def _launch_attn(c, inp, rows, info, bias):
    """One launch of case c over rows [rows.start, rows.stop) of a run's operands; returns out (B, h head_dim) on the CPU after
    checking that the pad columns kept their NaN."""
    from valle2_amd import kernels as K
    B, h, hd = c.B, c.h, c.head_dim
    d = h * hd
    h16 = K.H16 if c.entry in D.KV16 else torch.float32
    n = inp['length'][rows].long()

    def dirty(k, v, upto):                                       # NaN in K, Inf in V beyond every length
        k, v = k.clone(), v.clone()
        beyond = torch.arange(k.shape[2])[None] >= upto[:, None]
        k[beyond[:, None, :].expand(k.shape[:3])] = float('nan')
        v[beyond[:, None, :].expand(v.shape[:3])] = float('inf')
        return k.to(h16).to(DEV), v.to(h16).to(DEV)
    k, v = dirty(inp['k'][rows], inp['v'][rows], n)
    q = torch.full((B, d + 8), float('nan'), device=DEV)
    q[:, :d] = inp['q'][rows].reshape(B, d).to(DEV)
    out = torch.full((B, d + 8), float('nan'), device=DEV)
    cache_len = (n - bias).to(torch.int32).to(DEV)
    ws = None
    if info.ws_bytes:
        ws = torch.full(((info.ws_bytes + 15) // 16 * 4,), float('nan'), device=DEV)
        if c.entry == 'decode':                                  # vh_attn_decode: the ticket words behind the records start at zero
            ws[info.records * info.record_floats * B * h:].zero_()
    qv, ov = q[:, :d], out[:, :d]
    if c.entry == 'decode':
        K.attn_decode(qv, k, v, ov, cache_len, bias, n_split=c.n_split, partial=ws)
    elif c.entry == 'hd':
        K.attn_decode_hd(qv, k, v, ov, cache_len, bias, n_split=c.n_split, partial=ws, scale=inp['scale'])
    elif c.entry == 'kv16':
        K.attn_decode_kv16(qv, k, v, ov, cache_len, bias)
    elif c.entry == 'kv16_split':
        K.attn_decode_kv16(qv, k, v, ov, cache_len, bias, n_split=c.n_split, partial=ws if ws is not None else torch.zeros(4, device=DEV))
    else:
        g0, g1 = (int(inp['grp'][rows.start]), int(inp['grp'][rows.stop - 1]) + 1)
        plen = inp['plen'][g0:g1].long()
        kp, vp = dirty(inp['kp'][g0:g1], inp['vp'][g0:g1], plen)
        if c.entry == 'shared_groups':
            K.attn_decode_shared_groups(qv, kp, vp, plen.to(torch.int32).to(DEV), D.PREFIX_CAP, k, v, ov, cache_len, bias, inp['beams'],
                                        n_split=c.n_split, partial=ws)
        else:
            fn = K.attn_decode_shared if c.entry == 'shared' else K.attn_decode_shared_kv16
            fn(qv, kp, vp, int(plen[0]), k, v, ov, cache_len, bias, n_split=c.n_split, partial=ws)
    out = out.cpu()
    assert bool(torch.isnan(out[:, d:]).all()), 'a pad column of out was written'
    return out[:, :d].reshape(B, h, hd)


@pytest.mark.parametrize('i', range(len(ATTN_CASES)), ids=[D.attn_case_id(c) for c in ATTN_CASES])
def test_attention_form_against_float64(i):
    from valle2_amd import _lib
    from valle2_amd import kernels as K
    c = ATTN_CASES[i]
    lib = _lib.lib()
    h16 = K.H16 if c.entry in D.KV16 else None
    worst = {ss: 0.0 for ss in D.SCORE_SETS}
    try:
        D.set_knobs(lib, D.ATTN_KNOBS, c.knobs)
        for S, bias, sel, beams in D.attn_runs(c):
            for ss in D.SCORE_SETS:
                inp = D.attn_inputs(c, S, bias, sel, beams, ss, h16)
                ref = D.attn_reference(inp)
                for r0 in range(0, inp['R'], c.B):
                    prefix = D.PREFIXES[sel] if c.entry in ('shared', 'shared_kv16') else None
                    form, info = D.attn_query(lib, c, S, beams, prefix)
                    assert form == c.form, (form, S, bias, sel, beams)
                    got = _launch_attn(c, inp, slice(r0, r0 + c.B), info, bias)
                    assert bool(torch.isfinite(got).all()), f'{ss} S={S} len_bias={bias}: NaN / Inf beyond a length or in the workspace reached the output'
                    if 'plen' in inp:                            # a parked group's rows: exactly 0.0
                        parked = (inp['plen'] == 0)[inp['grp'][r0:r0 + c.B]]
                        assert bool((got[parked] == 0).all())
                    err = D.worst(got, ref[r0:r0 + c.B]) / attn_bound(ss)
                    worst[ss] = max(worst[ss], err)
    finally:
        D.set_knobs(lib, D.ATTN_KNOBS, (0, 0, 0))
    print(f'FORM attn {D.attn_case_id(c)}: worst error over bound ' + ' '.join(f'{ss} {worst[ss]:.3f}' for ss in D.SCORE_SETS))
    assert max(worst.values()) <= 1.0, worst
