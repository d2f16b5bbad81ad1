"""CPU companion of tests/test_train_steps_gpu.py: the float32 CPU oracle trainer stands in for the device and writes records of
the same form (tests/train_replay.py).  The fault-free records pass every check of the audit on every run and the free-running comparison
on every run through train(); every planted fault is rejected, by the check named for it; the float32-versus-float64 figures the GPU file's bounds
rest on are measured here, on the oracle, and re-asserted; and the runs are what they are meant to be (the clip acts on some
steps and is idle on others, the stage draws repeat, skip and start late).  No GPU."""
import ast
import functools
import random

import pytest
import torch

from tests import oracle_runners as R
from tests import test_train_steps_gpu as G
from tests import train_replay as T
from tests.attn_scores import written_figure


@functools.lru_cache(maxsize=None)
def cpu_record(run, fault=None):
    return T.oracle_train(run, torch.float32, fault=fault)


@functools.lru_cache(maxsize=None)
def free_reference(run):
    return T.oracle_train(run, torch.float64, replay=cpu_record(run))


def failed_checks(err):
    return set(str(err.value).split(' | ')[0][len('failed: '):].split(', '))


# ---- the helper itself --------------------------------------------------------------------------------------------------------
def test_train_replay_loads_no_library_at_import():
    tree = ast.parse(open(T.__file__).read())
    top = {a.name for n in tree.body if isinstance(n, ast.Import) for a in n.names} | \
          {n.module for n in tree.body if isinstance(n, ast.ImportFrom)}
    assert top == {'contextlib', 'math', 'random'}, top
    assert G.pytestmark.name == 'gpu' and set(G.ADAMW_DRIFT) == set(T.RUNS) and set(G.FREE_FIGURES) == set(T.FREE_RUNS)


def test_plan_restates_the_loop_of_train():
    """5 batches, accum 2, 7 steps: windows of 2, 2 and 1 per epoch; the cases of test_train_accumulation_windows_end_with_the_epoch
    follow from the same rule (an epoch's last window may be short, a window never spans two epochs)."""
    w = T.plan(5, 2, 7)
    assert [len(x['micro']) for x in w] == [2, 2, 1, 2, 2, 1, 2] and [x['epoch'] for x in w] == [0, 0, 0, 1, 1, 1, 2]
    assert [x['batches'] for x in w[:4]] == [[0, 1], [2, 3], [4], [0, 1]] and w[-1]['micro'] == [10, 11]
    assert [len(x['micro']) for x in T.plan(3, 1, 8)] == [1] * 8 and [x['epoch'] for x in T.plan(3, 1, 8)] == [0, 0, 0, 1, 1, 1, 2, 2]
    lrs = T.lr_schedule('ar_train', 3)
    assert lrs[0] == lrs[2] == 3e-3 and 0 < lrs[1] < lrs[0]             # lr changes per epoch; a warm restart inside the run


def test_the_runs_have_the_sizes_they_are_meant_to_have():
    for run, spec in T.RUNS.items():
        cfg, data = T.config_of(run), T.dataset_of(run)
        assert (cfg.num_layers, cfg.d_model, cfg.dim_feedforward, cfg.lr, cfg.weight_decay) == (2, 128, 256, 3e-3, 0.1)
        assert all(b['tokens'].shape[0] == 3 for b in data) and len(data) == spec['batches']
        if spec['model'] == 'ValleAR':
            assert all(4 <= int(b['tokens_lens'].min()) and int(b['tokens_lens'].max()) <= 8 for b in data)
            assert all(11 <= int(b['codes_lens'].min()) and int(b['codes_lens'].max()) <= 21 for b in data)   # BOS + 10..20
        else:
            assert all(b['tokens'].shape == (3, 8) and b['codes'].shape == (3, 20, cfg.num_quantizers) for b in data)
    assert T.config_of('ar_nodes').d_model // T.config_of('ar_nodes').n_heads == 32
    assert T.RUNS['resume']['resume_at'] == 4 and {k: v for k, v in T.RUNS['resume'].items() if k != 'resume_at'} == T.RUNS['nar_train']


def test_the_clip_acts_on_two_steps_and_is_idle_on_two():
    """On the float64 oracle's own free run of ar_train (5 % off the threshold either way, so float32 norms fall the same side)."""
    ref = free_reference('ar_train')
    norms = [s['norm'] for s in ref.steps]
    print('ar_train float64 norms', [round(n, 3) for n in norms])
    assert sum(n > 1.05 * T.AR_CLIP for n in norms) >= 2 and sum(n < 0.95 * T.AR_CLIP for n in norms) >= 2, norms


def test_the_stage_draws_repeat_skip_and_start_late():
    random.seed(T.NAR_SEED)
    cfg = T.config_of('nar_train')
    draws = [random.randint(1, cfg.num_quantizers - 1) for _ in range(cfg.max_steps)]
    assert draws == [m['stage'] for m in cpu_record('nar_train').micro] == [m['stage'] for m in cpu_record('resume').micro]
    first = {s: draws.index(s) for s in set(draws)}
    assert len(set(draws)) < len(draws), 'no stage repeats'
    assert len(set(draws)) < cfg.num_quantizers - 1, 'every stage is trained'
    assert any(i > 3 for i in first.values()), 'no stage starts after step 3'
    assert any(i >= T.RUNS['resume']['resume_at'] for i in first.values())          # ... nor after the resume
    counts = cpu_record('nar_train').final['slot_steps']
    assert {0, 1, 2, 3, cfg.max_steps} <= set(counts), sorted(set(counts))          # per-slot counts and corrections differ


# ---- the fault-free record passes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', list(T.RUNS))
def test_fault_free_float32_record_passes_the_audit(run):
    rec = cpu_record(run)
    rep = T.audit(rec, G.ADAMW_DRIFT[run])
    if run in T.FREE_RUNS:
        T.free_run(rec, G.FREE_FIGURES[run], rep)
        rep.raise_if_failed()
    print(rep.line(run))
    assert set(rep.worst) >= set('abcdefgh')
    # the dropout fields are the ones a forward of the device records: two PositionalEncoding fields, three per layer
    cfg = T.config_of(run)
    assert all(len(m['fields']) == 2 + (3 * cfg.num_layers if cfg.dropout else 0) for m in rec.micro)
    assert [sorted({f['seed'] for f in m['fields']}) for m in rec.micro] == [sorted(x) for x in T.drawn_seeds(run)]


# ---- the written figures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', list(T.RUNS))
def test_adamw_float32_drift_is_what_the_gpu_file_says(run):
    """torch's float32 AdamW against the float64 one on the float32 oracle's gradients of this run (same shapes, same steps),
    in units of check e's bound: it stays inside (< 1 / SUM_MARGIN), so the bound is test_flat_adamw_matches_torch_adamw_and_clip's."""
    drift = T.adamw_drift(cpu_record(run))
    written = G.ADAMW_DRIFT[run]
    print(f'{run}: drift {drift:.3e} of the bound, written {written_figure(drift):.1e}')
    assert 0.25 * written <= drift <= written, f'measured {drift:.3e}, the GPU file says {written:.3e}'
    assert R.SUM_MARGIN * written <= 1.0


@pytest.mark.parametrize('run', T.FREE_RUNS)
def test_free_running_float32_deviation_is_what_the_gpu_file_says(run):
    loss, disp, where = T.free_deviation(cpu_record(run), free_reference(run))
    print(f'{run}: loss {loss:.3e} displacement {disp:.3e} ({where}); written ({written_figure(loss):.1e}, {written_figure(disp):.1e})')
    for got, written in zip((loss, disp), G.FREE_FIGURES[run]):
        assert 0.25 * written <= got <= written, f'measured {got:.3e}, the GPU file says {written:.3e}'


def smallest_update_denominator(run, numel=1024):
    """Over the parameters of at most `numel` elements that the run trains by one or two steps (their whole displacement is first
    updates): the smallest non-zero |clipped gradient
    element| of the float32 oracle's record at the parameter's FIRST step, and where: AdamW's first update of an element is
    g / (|g| + eps), eps = 1e-8 (later ones divide by a root of the squares' average, which one small element does not make)."""
    rec, out, seen = cpu_record(run), (float('inf'), None), set()
    for st in rec.steps:
        coef = min(1.0, st['max_norm'] / st['norm']) if st['max_norm'] > 0 else 1.0
        for i, (n, g) in enumerate(rec.unflat(st['pre_grad']).items()):
            if st['touched'][i] and n not in seen and rec.final['slot_steps'][i] <= 2 and g.numel() <= numel and bool((g != 0).any()):
                out = min(out, (float(g[g != 0].abs().min()) * coef, n))
            seen |= {n} if st['touched'][i] else set()
    return out


@pytest.mark.parametrize('run', list(T.RUNS))
def test_runs_keep_small_tensors_off_adamws_eps(run):
    """What makes a run fit for the free-running comparison (train_replay.FREE_RUNS): a vector of 128 elements whose gradient
    holds an element at AdamW's eps moves by that element's round-off; every run's small tensors stay 10 eps clear of it.  (In
    the AR runs every parameter takes every step: nothing there is made of first updates alone.)"""
    g, where = smallest_update_denominator(run)
    print(f'{run}: smallest clipped gradient element of a small tensor {g:.2e} ({where})')
    assert g >= 1e-7, (run, g, where)
    assert (where is None) == (T.RUNS[run]['model'] == 'ValleAR')


# ---- every planted fault is rejected, by the check named for it ---------------------------------------------------------------
FAULT_CASES = [           # (fault, run, the checks that must reject it, and no other does)
    ('stale_weights', 'ar_train', {'b', 'c'}, True),
    ('stale_one_matrix', 'ar_nodes', {'c'}, True),
    ('no_zero_grad', 'ar_nodes', {'c', 'g'}, True),
    ('accum_unscaled', 'ar_nodes', {'c'}, True),
    ('no_clip', 'ar_nodes', {'e'}, True),
    ('decay_untouched', 'nar_dropout', {'e'}, True),
    ('global_step_count', 'nar_train', {'e'}, True),
    ('lr_frozen', 'ar_train', {'f'}, True),
    ('same_field_every_step', 'ar_dropout', {'h'}, True),
    ('moments_reset_on_resume', 'resume', {'e'}, True),
    ('weights_written_between_steps', 'ar_train', {'a'}, True),
    ('window_leaks_into_next_epoch', 'ar_train', {'c'}, False),      # (the steps fall into other epochs as well: b and f see it too)
]


def test_every_fault_has_a_case():
    assert [f for f, *_ in FAULT_CASES] == list(T.FAULTS)


@pytest.mark.parametrize('fault,run,named,only', FAULT_CASES, ids=[f for f, *_ in FAULT_CASES])
def test_planted_fault_is_rejected_by_its_check(fault, run, named, only):
    rec = cpu_record(run, fault)
    with pytest.raises(T.AuditError, match='failed: ') as err:
        T.audit(rec, G.ADAMW_DRIFT[run])
    failed = failed_checks(err)
    assert failed == named if only else failed >= named, str(err.value)[:2000]
    rep = T.audit(rec, G.ADAMW_DRIFT[run], raise_on_failure=False)
    first = {c: next(m for k, m in rep.failed if k == c) for c in named}
    if fault == 'no_zero_grad':                                       # c at the NEXT step: step 0 is still right
        assert first['c'].startswith('c: step 1 ') and first['g'].startswith('g: step 0:'), first
    if fault in ('stale_weights', 'stale_one_matrix'):                # step 0 is right: only a later step shows it
        assert first['c'].startswith('c: step 1 '), first
        if fault == 'stale_one_matrix':
            assert all(T.STALE_MATRIX in m for k, m in rep.failed), rep.failed
    if fault == 'moments_reset_on_resume':                            # on the first resumed step
        assert first['e'].startswith(f'e: step {rec.resume_at} '), first
    if fault == 'global_step_count':                                  # where the late stage takes its first step
        late = next(i for i, m in enumerate(rec.micro) if m['stage'] not in [x['stage'] for x in rec.micro[:i]] and i > 0)
        assert first['e'].startswith(f'e: step {late} '), first
    if fault == 'weights_written_between_steps':
        assert first['a'].startswith('a: step 3:') and T.STALE_MATRIX in first['a'], first
