"""CPU companion of tests/test_decode_forms_gpu.py (no GPU: the form queries launch nothing).

A. the ledger: every (FORM_TABLE row, epilogue) of the skinny GEMMs and every launch form of the decode attention belongs to a
   GPU test — the existing integer walk, test_head_greedy_one_launch_equals_head_then_greedy_step, or a case of
   tests/decode_forms.py — and every case takes exactly the form it is named for;
B. the float64 references are torch's own;
C. plain fp32 emulations of each arithmetic stay inside the bounds the GPU file uses (margins printed), and the emulation
   errors behind the attention bounds are what the GPU file records;
D. every planted fault misses a bound by more than 10 x on at least one case (the pattern of tests/test_attn_geometry_cpu.py)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import decode_forms as D
from tests import test_attn_forms_cpu as AF
from tests import test_decode_forms_gpu as G
from valle2_amd import _lib

GEMM_CASES, ATTN_CASES = D.gemm_cases(), D.attn_cases()


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


@pytest.fixture(scope='module')
def H16():
    return _lib.h16_dtype()


# ---- A. the ledger --------------------------------------------------------------------------------------------------------------
# (row, epilogue) instantiations / launch forms that no GPU test runs, each on purpose: {key: reason}
GEMM_NOT_RUN = {}
ATTN_NOT_RUN = {}


def test_gemm_ledger_every_row_and_epilogue_is_run(L):
    rows = set()
    info = _lib.VhLinearFormInfo()
    i = 0
    while L.vh_linear_form_row(i, C.byref(info)) == 0:
        rows |= {(info.family, info.mt, info.nw, info.pw, info.ln, info.nj, info.w16, epi) for epi in range(8) if info.epis >> epi & 1}
        i += 1
    walked = {D.gemm_form_tuple(f) for f in D.gemm_walked_forms()}
    new = [D.gemm_form_tuple(c.form) for c in GEMM_CASES]
    assert len(new) == len(set(new)) and not set(new) & walked, 'a form is run twice'
    assert len(D.gemm_head_forms()) == 3 and all(f.startswith('head<') for f in D.gemm_head_forms())
    accounted = walked | set(new)
    print(f'{i} table rows, {len(rows)} (row, epilogue) instantiations: {len(walked)} in the existing walk + {len(new)} new cases = '
          f'{len(accounted & rows)} of {len(rows)}; 3 head<> forms with the head_greedy test')
    assert accounted <= rows, f'cases name forms that are not compiled: {sorted(accounted - rows)}'
    assert rows - accounted == set(GEMM_NOT_RUN), f'instantiations no GPU test runs: {sorted(rows - accounted - set(GEMM_NOT_RUN))}'
    assert len(rows) == 233 and len(accounted) == 233


def test_gemm_cases_take_the_form_they_are_named_for(L):
    try:
        for c in GEMM_CASES:
            D.set_knobs(L, D.GEMM_KNOBS, c.knobs)
            assert D.gemm_query_form(L, c) == c.form, D.gemm_case_id(c)
            D.set_knobs(L, D.GEMM_KNOBS, (0, 0, 0))
            if c.knobs != (0, 0, 0):                              # a knob only where no shape reaches the form without one
                assert D.gemm_query_form(L, c) != c.form, D.gemm_case_id(c)
    finally:
        D.set_knobs(L, D.GEMM_KNOBS, (0, 0, 0))
    # the existing walk's cases too (a GPU test id cannot claim a form it does not run)
    from tests.test_kernels_gpu import _first_shape_of_each_form
    try:
        for p in _first_shape_of_each_form():
            knobs, label, M, N, K, T = p.values
            D.set_knobs(L, D.GEMM_KNOBS, knobs)
            got = D.gemm_query_form(L, D.GemmCase('', label, M, N, K, T, knobs))
            assert not D.is_skinny(p.id) or p.id.startswith(got.split(' ')[0] + '-'), (p.id, got)
    finally:
        D.set_knobs(L, D.GEMM_KNOBS, (0, 0, 0))


def test_attention_ledger_every_launch_form_is_run(L):
    forms, kernels = set(), set()
    info = _lib.VhAttnDecodeFormInfo()
    try:
        for knobs in AF.KNOB_SETS:
            D.set_knobs(L, D.ATTN_KNOBS, knobs)
            for s in AF.domain():
                for n in AF.SPLITS if s['label'] != 'kv16' else (1,):
                    if L.vh_attn_decode_form(AF.ENTRIES[s['label']], s['B'], s['h'], s['hd'], s['S_max'], n, s['prefix'], s['prefix_S'],
                                             s['beams'], AF.AMPLE, C.byref(info)) == 0:
                        forms.add(D.attn_info_form(s['label'], info))
                        kernels.add((info.kernel, info.nw, info.d, info.lk, info.nv))
    finally:
        D.set_knobs(L, D.ATTN_KNOBS, (0, 0, 0))
    run = [c.form for c in ATTN_CASES]
    print(f'{len(forms)} launch forms over {len(kernels)} compiled first kernels; {len(run)} cases')
    assert len(run) == len(set(run)) and set(run) <= forms
    assert forms - set(run) == set(ATTN_NOT_RUN), sorted(forms - set(run) - set(ATTN_NOT_RUN))
    assert len(forms) == 29 and len(kernels) == 16


def test_attention_cases_take_the_form_they_are_named_for(L):
    try:
        for c in ATTN_CASES:
            for S, bias, sel, beams in D.attn_runs(c):
                D.set_knobs(L, D.ATTN_KNOBS, c.knobs)
                assert D.attn_query(L, c, S, beams)[0] == c.form, (D.attn_case_id(c), S, beams)
            D.set_knobs(L, D.ATTN_KNOBS, (0, 0, 0))
            if c.knobs != (0, 0, 0):
                assert D.attn_query(L, c, 104)[0] != c.form, D.attn_case_id(c)
    finally:
        D.set_knobs(L, D.ATTN_KNOBS, (0, 0, 0))
    # smallest first, and the four-wave burst kernel at the default knobs
    assert any('attn_decode_kernel<4>' in c.form and c.knobs == (0, 0, 0) and c.B * c.h * c.n_split >= 1024 for c in ATTN_CASES)


# ---- B. the references are right -----------------------------------------------------------------------------------------------
# two float64 evaluations of a 5 +- 2^-8 row differ by 2^-52 |mean| / std |out| ~ 3e-10 (the centring cancels 11 bits); the GPU
# bounds start at 2^-21 |out|
F64 = dict(rtol=1e-10, atol=1e-9)


def _shapes(cases):
    """One case per (LayerNorm kind, entry family, M, N, K, T): cases that differ in the epilogue's store only share operands."""
    seen = {}
    for c in cases:
        seen.setdefault((D.gemm_ln(c), c.label.split('_')[0] + str('w16' in c.label), c.M, c.N, c.K, c.T), c)
    return list(seen.values())


@pytest.mark.parametrize('c', _shapes(GEMM_CASES), ids=D.gemm_case_id)
def test_gemm_reference_is_torch_in_float64(c, H16):
    sets = [D.gemm_exact_inputs(c, rot) + (None,) for rot in range(3)] + [D.gemm_ordinary_inputs(c)]
    for n, (x, w, bias, gamma, beta, res) in enumerate(sets):
        for act in (False, True):
            y = x.double()
            if gamma is not None:
                y = F.layer_norm(y, (c.K,), gamma.double(), beta.double(), D.EPS)
            y = F.linear(y, w.double(), None if bias is None else bias.double())
            y = (F.gelu(y) if act else y) + (0 if res is None else res.double())
            torch.testing.assert_close(D.gemm_reference(x, w, bias, gamma, beta, act, res), y, **F64)
        if gamma is None:
            if 'w16' in c.label and n == 3:                      # the 16-bit form: the matrix rounded first
                w16 = w.to(H16)
                assert float((w16.double() - w.double()).abs().max()) > 0
                torch.testing.assert_close(D.gemm_reference(x, w16, bias), F.linear(x.double(), w16.double(), bias.double()), **F64)
            continue
        # the folded form of the same thing, through the matrix as stored (fp32 or rounded to 16 bits) and c2 in float64
        for wf in ((w * gamma), (w * gamma).to(H16).float()):
            c2 = beta.double() @ w.double().T + (0 if bias is None else bias.double())
            y = F.linear(F.layer_norm(x.double(), (c.K,), None, None, D.EPS), wf.double()) + c2
            torch.testing.assert_close(D.gemm_reference_folded(x, wf, c2), y, **F64)
        if n < 3:                                                # exact rows: the bound functions' references are the same numbers
            ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
            torch.testing.assert_close(ref, D.gemm_reference(x, w, bias, gamma, beta), **F64)
            assert float(bound.min()) >= 0


def _naive_attention(inp, r):
    """Row r by the book: softmax(q K^T scale) V in float64 over the keys the row attends, prompt first."""
    q, n = inp['q'][r].double(), int(inp['length'][r])
    k, v = inp['k'][r, :, :n].double(), inp['v'][r, :, :n].double()
    if 'plen' in inp:
        g, p = int(inp['grp'][r]), int(inp['plen'][inp['grp'][r]])
        if p == 0:
            return torch.zeros_like(q)
        k, v = torch.cat([inp['kp'][g, :, :p].double(), k], 1), torch.cat([inp['vp'][g, :, :p].double(), v], 1)
    return (F.softmax((q[:, None, :] @ k.transpose(-1, -2)) * inp['scale'], dim=-1) @ v)[:, 0]


@pytest.mark.parametrize('c', ATTN_CASES, ids=D.attn_case_id)
def test_attention_reference_is_torch_softmax_in_float64(c, H16):
    h16 = H16 if c.entry in D.KV16 else None
    for S, bias, sel, beams in D.attn_runs(c):
        for ss in D.SCORE_SETS:
            inp = D.attn_inputs(c, S, bias, sel, beams, ss, h16)
            ref = D.attn_reference(inp)
            rows = range(inp['R']) if inp['R'] <= 36 else range(0, inp['R'], 5)
            for r in rows:
                torch.testing.assert_close(ref[r], _naive_attention(inp, r), rtol=1e-10, atol=1e-12)
            assert bool(torch.isfinite(ref).all())
            if h16 is not None:                                  # rounded first: the 16-bit caches are exactly representable
                assert torch.equal(inp['k'].to(h16).float(), inp['k']) and torch.equal(inp['v'].to(h16).float(), inp['v'])
            # the scores are what the set asks for
            if ss in ('plus200', 'minus200') and 'plen' not in inp:
                s = torch.einsum('rhd,rhsd->rhs', inp['q'].double(), inp['k'].double()) * inp['scale']
                assert float((s.abs() - 200).abs().max()) < 40, (ss, float(s.min()), float(s.max()))


def test_attention_geometry_is_what_the_issue_asks_for():
    for c in ATTN_CASES:
        runs = D.attn_runs(c)
        assert {(S, b) for S, b, _, _ in runs} == {(104, 0), (104, 1), (8, 0), (8, 1)}
        for S, bias, sel, beams in runs:
            inp = D.attn_inputs(c, S, bias, sel, beams, 'plain')
            assert set(inp['length'].tolist()) - {0} == set(D.LENGTHS[S]) and inp['R'] % c.B == 0
            assert int(inp['length'].min()) >= (0 if c.entry == 'shared_groups' and bias == 0 else 1)
        if c.entry in D.SHARED and c.entry != 'shared_groups':
            assert sorted(D.PREFIXES[sel] for _, _, sel, _ in runs) == sorted(D.PREFIXES) and c.B == 33
        if c.entry == 'shared_groups':
            seen = set()
            for S, bias, sel, beams in runs:
                inp = D.attn_inputs(c, S, bias, sel, beams, 'plain')
                seen |= set(inp['plen'].tolist())
                assert beams == c.B or (0 in inp['plen'].tolist() and len(set(inp['plen'].tolist())) > 2)
            assert seen >= set(D.PREFIXES) and {b for _, _, _, b in runs} == {1, 4, 36}
        if c.n_split > 1:                                        # split counts that leave some splits without a chunk
            assert (min(D.LENGTHS[104]) + 31) // 32 < c.n_split


# ---- C. the bounds hold for correct arithmetic ------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', _shapes([c for c in GEMM_CASES if D.gemm_ln(c)]), ids=D.gemm_case_id)
def test_gemm_emulation_stays_inside_the_bound(c):
    ln = D.gemm_ln(c)
    worst = 0.0
    for rot in range(3):
        x, w, bias, gamma, beta = D.gemm_exact_inputs(c, rot)
        ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
        got = D.emulate_gemm(ln, x, w, bias, gamma, beta)
        worst = max(worst, G.excess(got, ref, bound))
    x, w, bias, gamma, beta, res = D.gemm_ordinary_inputs(c)
    ref = D.gemm_reference(x, w, bias, gamma, beta)
    ordinary = G.excess(D.emulate_gemm(ln, x, w, bias, gamma, beta), ref, G.ATOL + G.RTOL * ref.abs())
    print(f'{D.gemm_case_id(c)}: fp32 emulation (LN {ln}) at {worst:.3f} of the exact rows\' bound, {ordinary:.3f} of atol 2e-5 + rtol 1e-5')
    assert worst <= 1.0 and (ordinary <= 1.0 or c.K > 1024)


def test_gemm_exact_rows_are_exact_without_a_layernorm():
    for c in [c for c in GEMM_CASES if D.gemm_ln(c) == 0]:
        for rot in range(3):
            x, w, bias, gamma, beta = D.gemm_exact_inputs(c, rot)
            ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
            got = x @ w.T + (0 if bias is None else bias)            # fp32, torch's order: any order gives these bits
            assert float(bound.max()) == 0 and torch.equal(got.double(), ref)
            assert torch.equal(w.half().float(), w) and torch.equal(w.bfloat16().float(), w)


@pytest.mark.parametrize('c', _shapes([c for c in GEMM_CASES if 'kv16' in c.label]), ids=D.gemm_case_id)
def test_16bit_append_check_holds_for_correct_arithmetic(c, H16):
    """fp32 torch rounded once to the 16-bit format lies inside round16(reference -+ bound) on every input set, and outside it
    as soon as it is rounded from a value two bounds away; within ONE unit of the rounded reference it is not, where the value
    is a cancellation (decode_forms.stored16_outside)."""
    ln, far = D.gemm_ln(c), 0
    sets = [D.gemm_exact_inputs(c, rot) for rot in range(3)] + [D.gemm_ordinary_inputs(c)[:5]]
    for n, (x, w, bias, gamma, beta) in enumerate(sets):
        ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
        if n == 3:
            bound = G.ATOL + G.RTOL * ref.abs()
        emu = D.emulate_gemm(ln, x, w, bias, gamma, beta)
        assert D.stored16_outside(emu.to(H16), ref, bound) == 0
        assert D.stored16_outside((emu.double() + 2 * bound).to(H16), ref, bound) > 0
        far = max(far, int((ref.to(H16).view(torch.int16).int() - emu.to(H16).view(torch.int16).int()).abs().max()))
    print(f'{D.gemm_case_id(c)}: correct fp32 arithmetic up to {far} units from the rounded float64 value')


@functools.lru_cache(maxsize=None)
def _attn_errors(i):
    """{(run, set): (plain fp32 error, chunked fp32 error)} of case i against float64, and the inputs' references."""
    c = ATTN_CASES[i]
    h16 = _lib.h16_dtype() if c.entry in D.KV16 else None
    out = {}
    for run in D.attn_runs(c):
        for ss in D.SCORE_SETS:
            inp = D.attn_inputs(c, *run, ss, h16)
            ref = D.attn_reference(inp)
            out[run, ss] = (D.worst(D.attn_reference(inp, torch.float32), ref), D.worst(D.attn_emulate_chunked(inp, c.n_split), ref))
    return out


def test_attention_emulation_errors_are_what_the_gpu_file_records():
    worst = {ss: 0.0 for ss in D.SCORE_SETS}
    for i, c in enumerate(ATTN_CASES):
        for (run, ss), errs in _attn_errors(i).items():
            worst[ss] = max(worst[ss], *errs)
    for ss in D.SCORE_SETS:
        print(f'{ss}: larger fp32 emulation error over every case {worst[ss]:.3e}, recorded {G.ATTN_EMU_ERR[ss]:.3e}, bound {G.attn_bound(ss):.3e}')
    for ss in D.SCORE_SETS:
        assert 0.25 * G.ATTN_EMU_ERR[ss] <= worst[ss] <= G.ATTN_EMU_ERR[ss], (ss, worst[ss])
        assert worst[ss] <= G.attn_bound(ss)                     # plain: inside the project's atol
    assert G.attn_bound('plain') == 2e-5 and all(G.attn_bound(ss) == 4 * G.ATTN_EMU_ERR[ss] for ss in D.SCORE_SETS[1:])


# ---- D. planted faults ---------------------------------------------------------------------------------------------------------
FAULT_SHAPES = [c for c in GEMM_CASES if (c.label, c.M, c.K) in {('linear_folded', 17, 256), ('linear_folded', 1, 1280), ('linear+ln', 17, 256),
                                                                    ('linear_folded', 1, 256), ('qkv_folded_hd', 17, 256)}]


@pytest.mark.parametrize('fault', D.GEMM_FAULTS)
def test_gemm_planted_fault_is_rejected_with_margin(fault):
    miss = {}
    assert len({(c.label, D.gemm_ln(c)) for c in FAULT_SHAPES}) >= 4
    for c in FAULT_SHAPES:
        ln = D.gemm_ln(c)
        for rot in range(3):
            x, w, bias, gamma, beta = D.gemm_exact_inputs(c, rot)
            ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
            if fault in ('kv_swapped', 'row_plus_one', 'head_shifted'):
                if not c.label.startswith('qkv'):
                    continue
                hd = D.gemm_head_dim(c)
                cl = D.gemm_cache_len(c, G.S_CACHE)
                got = D.emulate_gemm(ln, x, w, bias, gamma, beta).double()
                args = (cl, c.T, c.K // hd, hd, G.S_CACHE)
                want = D.scatter_qkv(ref, *args, G.SENTINEL, c.K + 8)
                tol = D.scatter_qkv(bound, *args, (0, 0), c.K + 8)
                bad = D.scatter_qkv(got, *args, G.SENTINEL, c.K + 8, fault=fault)
                good = D.scatter_qkv(got, *args, G.SENTINEL, c.K + 8)
                assert max(G.excess(a, b, t) for a, b, t in zip(good, want, tol)) <= 1.0
                m = max(G.excess(a, b, t) for a, b, t in zip(bad, want, tol))
            else:
                m = G.excess(D.emulate_gemm(ln, x, w, bias, gamma, beta, fault=fault, nw=16 if c.K > 1024 else 8), ref, bound)
            miss[D.gemm_case_id(c), rot] = m
    print(fault, {f'{k[0]} rot{k[1]}': f'{m:.3g}' for k, m in miss.items()})
    assert max(miss.values()) > 10, miss


def test_eps_shows_on_the_low_variance_rows_only():
    """Why the third kind of row exists: without eps the +-1 and {-1, +3} rows stay within ~10 x the bound, the 5 +- 2^-8 rows
    miss it by five orders of magnitude."""
    c = next(c for c in GEMM_CASES if (c.label, c.M, c.K) == ('linear_folded', 17, 256))
    x, w, bias, gamma, beta = D.gemm_exact_inputs(c, 0)
    ref, bound = D.gemm_exact_bound(c, x, w, bias, gamma, beta)
    e = (D.emulate_gemm(2, x, w, bias, gamma, beta, fault='no_eps').double() - ref).abs() / bound
    by_kind = [float(e[k::3].max()) for k in range(3)]
    print('eps omitted, error over bound by kind of row:', by_kind)
    assert by_kind[0] < 100 and by_kind[1] < 100 and by_kind[2] > 1e4


ATTN_FAULT_CASES = [i for i, c in enumerate(ATTN_CASES) if c.B * c.h <= 72]      # (the 512- and 1024-pair cases add nothing here)


@pytest.mark.parametrize('fault', D.ATTN_FAULTS)
def test_attention_planted_fault_is_rejected_with_margin(fault):
    worst, where = 0.0, None
    for i in ATTN_FAULT_CASES:
        c = ATTN_CASES[i]
        if fault in ('prefix_block_whole', 'group0_prefix', 'second_pass_columns') and c.entry not in D.SHARED:
            continue
        if fault == 'group0_prefix' and c.entry != 'shared_groups':
            continue
        if fault == 'empty_split_max_0' and c.n_split == 1 and c.entry not in D.SHARED:
            continue
        h16 = _lib.h16_dtype() if c.entry in D.KV16 else None
        for run in D.attn_runs(c):
            for ss in D.SCORE_SETS:
                inp = D.attn_inputs(c, *run, ss, h16)
                ref = D.attn_reference(inp)
                if fault in ('empty_split_max_0', 'no_rescale', 'exp_before_max'):
                    bad = D.attn_emulate_chunked(inp, c.n_split, fault=fault)
                else:
                    bad = D.attn_reference(inp, torch.float32, fault=fault)
                m = D.worst(bad, ref) / G.attn_bound(ss)
                if m > worst:
                    worst, where = m, (D.attn_case_id(c), run, ss)
    print(f'{fault}: misses the bound by {worst:.3g} x at {where}')
    assert worst > 10
