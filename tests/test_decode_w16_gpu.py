"""The perf-mode decode step over h16 weights (VALLE2_DECODE_W16=1: gemm_skinny_fast<..., W16> with the fp16 K/V append and
with the plain epilogue, ffn_decode_kernel<D, SW, W16>) against a float64 mirror of the same rounded operands
(tests/oracle_runners.W16Mirror; tests/test_decode_w16_cpu.py shows that the mirror is right and what it can see).

(a) teacher-forced logits against the mirror at the project's summation-order bound, atol 2e-4 / rtol 1e-4.  The bound is not
    taken from the w16 run: at every case the fp32-weight perf_mode='kv' decoder (the route that exists without the variable)
    is compared with the same mirror over unrounded matrices, under the same bound — what that bound cannot account for, an h16
    rounding of a new K/V element that falls the other way in fp32 than in float64, is common to both routes.  Measured on the
    MI355X (fp16 build), worst case over the decode steps of each route: fp32 weights 2.4e-5, h16 weights 2.4e-5 (both d1024,
    64 rows; 3.9e-6 / 1.0e-5 / 1.4e-5 at d128 / d256 / d512) — a tenth of the bound, which stands.
(b) the same logits against the unrounded float64 oracle within the perf-mode model tolerance (1.5e-2 fp16, 5e-2 bf16).
(c) free-running greedy and sampled decodes, graph and eager; the fp16 prompt pass in front of it.
(d) the fallbacks: a width without h16 kernels, no perf mode, a decoder slot built without the variable.

Template instantiations reached (gemm.hip gemm_plan — tests/golden/gemm_decode_forms.txt lists them per shape — and ffn.hip ffn_plan; M rows, mt = ceil(M / 16)):
  gemm_skinny_fast<MT, 8, EPI_QKV16, PW, LN, NJ, true>, (PW, NJ at LN 2) = (1, 2) d128, (2, 4) d256, (4, 8) d512, (4, 16) d1024:
    LN 3, MT 1, NJ 1   every case without a knob: one tile (M <= 16) and row groups of 8 (d128; d256 to 40 rows) or 16
                       (VH_TUNE_ROW_GROUPS 3: 16 everywhere); d512 and d1024 share <1, 8, EPI_QKV16, 4, 3, 1, true>
    LN 2, MT 1         VH_TUNE_LN_STATS 1 at 7 rows (one tile) and at 24 rows (d512: row groups)
    LN 2, MT 2 / MT 4  VH_TUNE_ROW_GROUPS 2 at 24 / 48 rows
  gemm_skinny_fast<MT, 8, EPI_PLAIN, PW, 0, 1, true>, PW = 1 d128, 2 d256, 4 d512 and d1024 — the out-projection (bias,
  in-place residual) and the head (N = 1025: 65 column groups, the last one a single column):
    MT 1               every case without VH_TUNE_ROW_GROUPS 2 (row groups of 8 or 16 from 17 rows on)
    MT 2 / MT 4        VH_TUNE_ROW_GROUPS 2 at 24 / 48 rows
  ffn_decode_kernel<D, SW, true>:
    <128, 16>          every d128 case (dim_feedforward 528 has no slices of 32)
    <128, 32>          model d128s32 (dim_feedforward 544) under VH_TUNE_FFN_SLICE 32
    <256, 16> / <256, 32>   d256 up to 24 rows / at 64 rows
    <512, 16> / <512, 32>   d512 up to 16 rows / from 17 rows; both with 8 and 16 rows per workgroup under the knobs at 24 rows
    <1024, 16>         every d1024 case;  <1024, 32> is never dispatched (ffn_plan: slices of 16 at d_model 1024)
  Not dispatched for h16 weights at all: LN 1 (the unfolded LayerNorm), NW 16 (K > 1024), PW 5..7 (640 / 768 / 896), EPI_QKV,
  EPI_QKV_HD, EPI_PARTIAL, EPI_HEAD — gemm_plan refuses them, and engine.ArDecoder's gate keeps those shapes on fp32 weights."""
import contextlib
import functools

import pytest
import torch

from tests import oracle_runners as R
from tests.golden import cases as C
from valle2_amd._lib import h16_dtype

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H16 = h16_dtype()
MODEL_TOL = R.w16_model_tol(H16)
KEEP = list(range(R.W16_STEPS))
ROW_GROUPS, FFN_SLICE, FFN_ROWS, LN_STATS = 2, 7, 8, 9            # VH_TUNE_* (include/valle_hip.h)


def build(kw, sd):
    from valle2_amd import get_model_class
    m = get_model_class('ValleAR')(C.cfg_of(kw))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def ref(model):
    """The references of `model` over all 64 rows, computed once (rows are independent: a case of B rows reads the first B):
    the unrounded oracle, the mirror, and the mirror over unrounded matrices (K/V rounded alone)."""
    kw, sd, texts, firsts, forced = R.w16_inputs(model)
    cfg = C.cfg_of(kw)
    oracle = R.w16_oracle_logits(sd, cfg, texts, firsts, forced)
    R.w16_check_std(oracle[:, 0], model)
    mirror = R.w16_mirror_logits(sd, cfg, texts, firsts, forced, KEEP, H16)
    kv_only = R.w16_mirror_logits(sd, cfg, texts, firsts, forced, KEEP, H16, weights16=False)
    power = min(R.w16_distance(mirror[:, t], oracle[:, t]) for t in KEEP[1:])
    assert power >= R.W16_POWER, (model, power)
    return dict(kw=kw, sd=sd, cfg=cfg, texts=texts, firsts=firsts, forced=forced, oracle=oracle, mirror=mirror, kv_only=kv_only,
                m=build(kw, sd))


@functools.lru_cache(maxsize=None)
def greedy_ref(model):
    r = ref(model)
    return R.w16_mirror_greedy(r['sd'], r['cfg'], r['texts'], r['firsts'], R.W16_FREE_STEPS, H16)


@contextlib.contextmanager
def route(monkeypatch, m, w16, knobs=None):
    """The decoders built inside see VALLE2_DECODE_W16 set (or unset) and the tuning knobs given; everything is put back."""
    from valle2_amd import _lib, engine
    lib = _lib.lib()
    knobs = knobs or {}
    m.release_decoders()
    with monkeypatch.context() as mp:
        if w16:
            mp.setenv('VALLE2_DECODE_W16', '1')
        else:
            mp.delenv('VALLE2_DECODE_W16', raising=False)
        mp.setattr(engine, 'DECODE_W16', bool(w16))
        try:
            for knob, value in knobs.items():
                lib.vh_set_tuning(knob, value)
            yield
        finally:
            for knob in knobs:
                lib.vh_set_tuning(knob, 0)
            m.release_decoders()


def rows_of(r, B):
    return [t.to(DEV) for t in r['texts'][:B]], [f.to(DEV) for f in r['firsts'][:B]]


def forced_logits(m, r, B, perf_mode='kv'):
    tx, fs = rows_of(r, B)
    m.generate_batch(tx, fs, max_new=R.W16_STEPS, perf_mode=perf_mode, forced=r['forced'], keep_logits=KEEP)
    st = m.last_generate_stats
    return torch.stack([st['logits'][t] for t in KEEP], dim=1).cpu(), st


def w16_stats(st, prefill=False):
    assert st['decode_w16'] and st['kv_bf16'] and bool(st['prefill_bf16']) == prefill, \
        {k: st[k] for k in ('decode_w16', 'kv_bf16', 'prefill_bf16')}


CASES = []
for _model, _rows in (('d128', (1, 7, 16, 17, 32, 33, 64)), ('d512', (1, 7, 16, 17, 32, 33, 64)), ('d256', (1, 16, 24, 64)),
                      ('d1024', (1, 16, 24, 64))):
    CASES += [(_model, B, {}) for B in _rows]
    # the row-resident forms: LN 2 at MT 2 / MT 4 (and the plain epilogue at MT 2 / MT 4), LN 2 at MT 1
    CASES += [(_model, 24, {ROW_GROUPS: 2}), (_model, 48, {ROW_GROUPS: 2}), (_model, 7, {LN_STATS: 1})]
CASES += [(_model, 24, {ROW_GROUPS: 3}) for _model in ('d512', 'd1024')]
CASES += [('d512', 24, {LN_STATS: 1})]                                     # LN 2, MT 1 as row groups
CASES += [('d512', 24, {FFN_SLICE: sw, FFN_ROWS: rows}) for sw in (16, 32) for rows in (8, 16)]
CASES += [('d128s32', 24, {FFN_SLICE: 32}), ('d128s32', 7, {})]            # ffn_decode_kernel<128, 32>, and its <128, 16>
KNOB_NAMES = {ROW_GROUPS: 'rowgroups', FFN_SLICE: 'slice', FFN_ROWS: 'ffnrows', LN_STATS: 'lnstats'}


def _case_id(case):
    model, B, knobs = case
    return '-'.join([model, f'{B}rows'] + [f'{KNOB_NAMES[k]}{v}' for k, v in knobs.items()])


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_forced_logits_against_the_mirror_and_the_oracle(monkeypatch, case):
    model, B, knobs = case
    r = ref(model)
    m = r['m']
    with route(monkeypatch, m, True, knobs):
        got, st = forced_logits(m, r, B)
        w16_stats(st)
        again, st = forced_logits(m, r, B)
        w16_stats(st)
    with route(monkeypatch, m, False, knobs):
        f32w, st = forced_logits(m, r, B)
        assert not st['decode_w16'] and st['kv_bf16'] and not st['prefill_bf16']
    mirror, oracle, kv_only = r['mirror'][:B], r['oracle'][:B], r['kv_only'][:B]
    e_mirror, e_oracle, e_f32w = R.worst(got[:, 1:], mirror[:, 1:]), R.worst(got, oracle), R.worst(f32w[:, 1:], kv_only[:, 1:])
    print(f'{_case_id(case)}: decode steps: max |logit - mirror| = {e_mirror:.2e} ({R.w16_distance(got[:, 1:], mirror[:, 1:]):.2f} '
          f'tolerances), fp32 weights against the mirror over unrounded matrices {e_f32w:.2e} '
          f'({R.w16_distance(f32w[:, 1:], kv_only[:, 1:]):.2f} tolerances); step 0 (the prompt pass): {R.worst(got[:, 0], mirror[:, 0]):.2e}; '
          f'max |logit - oracle| = {e_oracle:.2e}')
    assert torch.equal(got, again), 'two runs of the same case differ'
    # the basis of the bound: the route without the variable, against the same mirror over unrounded matrices
    torch.testing.assert_close(f32w.double(), kv_only, atol=R.W16_ATOL, rtol=R.W16_RTOL)
    torch.testing.assert_close(got.double(), mirror, atol=R.W16_ATOL, rtol=R.W16_RTOL)                   # (a)
    assert e_oracle < MODEL_TOL, e_oracle                                                                # (b)


@pytest.mark.parametrize('model', ['d128', 'd256', 'd512', 'd1024'])
def test_worst_error_against_the_oracle_per_model(monkeypatch, model):
    """(b) per model, all 64 rows: what the 16-bit weights cost against the unrounded oracle."""
    r = ref(model)
    with route(monkeypatch, r['m'], True):
        got, st = forced_logits(r['m'], r, R.W16_MAX_ROWS)
        w16_stats(st)
    err = R.worst(got, r['oracle'])
    print(f'{model}: 64 rows x {R.W16_STEPS} steps: max |logit - oracle| = {err:.2e}, max |logit - mirror| = '
          f'{R.worst(got, r["mirror"]):.2e}, max |mirror - oracle| = {R.worst(r["mirror"], r["oracle"]):.2e}')
    assert err < MODEL_TOL


def test_c1_is_summed_over_the_rounded_matrix(monkeypatch):
    """The epilogue's c1 of the h16 tables is the row sum of the ROUNDED folded matrix (engine.decode_weights16): with the c1 of
    the unrounded fold the mirror stands 2.2 tolerances away at d1024 on these ordinary rows (measured on the CPU, fp16) — and
    2e-2 away on a row far from centred (tests/test_decode_w16_cpu.py)."""
    r = ref('d1024')
    fold = R.w16_mirror_logits(r['sd'], r['cfg'], r['texts'][:16], r['firsts'][:16], r['forced'], KEEP, H16, c1='fold')
    assert R.w16_distance(fold, r['mirror'][:16]) > 2.0
    with route(monkeypatch, r['m'], True):
        got, st = forced_logits(r['m'], r, 16)
        w16_stats(st)
    near, far = R.w16_distance(got, r['mirror'][:16]), R.w16_distance(got, fold)
    print(f'd1024 x 16 rows: {near:.2f} tolerances from the mirror with c1 of the h16 matrix, {far:.2f} from the one with c1 of the fold')
    assert near <= 1.0 < far


def _free_rows(model, B):
    """The first B of the 64 rows whose mirror keeps a top-2 margin of ten tolerances through step 11, and per row the step up
    to which tokens are compared (the first step whose margin falls short; all of them otherwise)."""
    toks, margins, tops = greedy_ref(model)
    short = margins < 10 * (R.W16_ATOL + R.W16_RTOL * tops.abs())
    upto = torch.where(short.any(1), short.float().argmax(1), torch.full((short.shape[0],), short.shape[1]))
    rows = [i for i in range(short.shape[0]) if int(upto[i]) >= 12][:B]
    assert len(rows) == B, f'{model}: only {len(rows)} rows keep the margin through step 11'
    return rows, toks, upto


@pytest.mark.parametrize('model,B', [('d128', 4), ('d128', 32), ('d512', 4), ('d512', 32)])
def test_free_running_greedy_tokens_are_the_mirrors(monkeypatch, model, B):
    """(With random weights the positional table decides the greedy token: the rows' logits differ, their argmax seldom does —
    a mix-up of rows is the forced cases' to see, this test holds the 23 chained steps and the graph.)"""
    r = ref(model)
    m = r['m']
    rows, toks, upto = _free_rows(model, B)
    tx = [r['texts'][i].to(DEV) for i in rows]
    fs = [r['firsts'][i].to(DEV) for i in rows]
    outs = []
    with route(monkeypatch, m, True):
        for use_graph in (True, False):
            out = m.generate_batch(tx, fs, max_new=R.W16_FREE_STEPS, perf_mode='kv', use_graph=use_graph)
            w16_stats(m.last_generate_stats)
            pl = m.last_generate_stats['prompt_lens'][0]
            outs.append(out[:, pl:].cpu())
    assert torch.equal(outs[0], outs[1]), 'graph and eager runs decode different tokens'
    assert outs[0].shape[1] == R.W16_FREE_STEPS
    for j, i in enumerate(rows):
        n = int(upto[i])
        assert torch.equal(outs[0][j, :n], toks[i, :n]), (model, i, n, outs[0][j].tolist(), toks[i].tolist())
    print(f'{model} x {B} rows: {R.W16_FREE_STEPS} greedy steps equal the mirror\'s (compared up to step '
          f'{min(int(upto[i]) for i in rows)} .. {max(int(upto[i]) for i in rows)})')


def test_sampled_decode_graph_and_eager_agree(monkeypatch):
    r = ref('d512')
    m = build(dict(r['kw'], top_k=50), r['sd'])
    tx, fs = rows_of(r, 8)
    outs, lps = [], []
    with route(monkeypatch, m, True):
        for use_graph in (True, False):
            torch.manual_seed(4321)
            outs.append(m.generate_batch(tx, fs, max_new=R.W16_FREE_STEPS, perf_mode='kv', use_graph=use_graph))
            w16_stats(m.last_generate_stats)
            lps.append(m.last_generate_stats['sum_logprobs'].cpu())
    assert torch.equal(outs[0], outs[1]), 'graph and eager runs drew different tokens under the same seed'
    torch.testing.assert_close(lps[0], lps[1], atol=1e-4, rtol=0)
    pl = m.last_generate_stats['prompt_lens'][0]
    assert len({tuple(row.tolist()) for row in outs[0][:, pl:]}) > 1 and bool((lps[0] < 0).all())


def test_fp16_prompt_pass_in_front_of_the_w16_steps(monkeypatch):
    r = ref('d512')
    with route(monkeypatch, r['m'], True):
        got, st = forced_logits(r['m'], r, 16, perf_mode=True)
        w16_stats(st, prefill=True)
    err = R.worst(got, r['oracle'][:16])
    print(f'd512 x 16 rows, perf_mode=True (16-bit prompt pass, h16 decode weights): max |logit - oracle| = {err:.2e}')
    assert err < MODEL_TOL


# ---- (d) the fallbacks -------------------------------------------------------------------------------------------------------
def test_a_width_without_h16_kernels_keeps_fp32_weights(monkeypatch):
    from valle2_amd import synth
    kw = dict(d_model=768, n_heads=12, dim_feedforward=1536, num_layers=2, dropout=0.0, norm='LayerNorm', top_k=1)
    sd = synth.make_state_dict(C.cfg_of(kw), 'ValleAR', seed=5, rich=True)
    m = build(kw, sd)
    gen = torch.Generator().manual_seed(6)
    tx = [torch.randint(0, 256, (11,), generator=gen).to(DEV) for _ in range(4)]
    fs = [torch.randint(0, 1024, (9,), generator=gen).to(DEV) for _ in range(4)]
    outs = []
    for w16 in (True, False):
        with route(monkeypatch, m, w16):
            outs.append(m.generate_batch(tx, fs, max_new=12, perf_mode='kv'))
            st = m.last_generate_stats
            assert not st['decode_w16'] and st['kv_bf16'] and st['ln_folded']
    assert torch.equal(outs[0], outs[1])


def test_without_perf_mode_the_variable_changes_nothing(monkeypatch):
    r = ref('d128')
    m = r['m']
    got = []
    for w16 in (True, False):
        with route(monkeypatch, m, w16):
            logits, st = forced_logits(m, r, 7, perf_mode=False)
            got.append((logits, {k: st[k] for k in ('decode_w16', 'kv_bf16', 'prefill_bf16', 'ln_folded', 'ffn_fused', 'n_split')}))
    assert got[0][1] == got[1][1] and not got[0][1]['decode_w16'] and not got[0][1]['kv_bf16']
    assert torch.equal(got[0][0], got[1][0])
    torch.testing.assert_close(got[0][0].double(), r['oracle'][:7], atol=R.W16_ATOL, rtol=R.W16_RTOL)


def test_a_call_without_the_variable_does_not_land_on_the_w16_slot(monkeypatch):
    from valle2_amd import engine
    r = ref('d512')
    m = r['m']
    tx, fs = rows_of(r, 8)
    m.release_decoders()
    try:
        with monkeypatch.context() as mp:
            mp.setenv('VALLE2_DECODE_W16', '1')
            mp.setattr(engine, 'DECODE_W16', True)
            a = m.generate_batch(tx, fs, max_new=12, perf_mode=True)
            w16_stats(m.last_generate_stats, prefill=True)
            assert not m.last_generate_stats['decoder_reused']
            b = m.generate_batch(tx, fs, max_new=12, perf_mode=True)
            w16_stats(m.last_generate_stats, prefill=True)
            assert m.last_generate_stats['decoder_reused'] and torch.equal(a, b)
        with monkeypatch.context() as mp:
            mp.delenv('VALLE2_DECODE_W16', raising=False)
            mp.setattr(engine, 'DECODE_W16', False)
            c = m.generate_batch(tx, fs, max_new=12, perf_mode=True)
            st = m.last_generate_stats
            assert not st['decoder_reused'] and not st['decode_w16'] and st['kv_bf16'] and st['prefill_bf16']
            logits, st = forced_logits(m, r, 8, perf_mode=True)
            assert not st['decode_w16']
            fresh = build(r['kw'], r['sd'])                                # a model that never built an h16 table
            c_fresh = fresh.generate_batch(tx, fs, max_new=12, perf_mode=True)
            assert not fresh.last_generate_stats['decode_w16']
            logits_fresh, _ = forced_logits(fresh, r, 8, perf_mode=True)
            fresh.release_decoders()
        assert torch.equal(c, c_fresh)
        assert torch.equal(logits, logits_fresh)
    finally:
        m.release_decoders()
