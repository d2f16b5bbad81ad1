"""Training over several optimizer steps on the device, audited in lockstep against the float64 oracle (tests/train_replay.py).

Each run below is done once (a module fixture per run), through `train()` — `resume` through the same loop written by hand, with the
model, the optimizer and the scheduler saved after step 3 and loaded into fresh ones — and recorded: every micro-batch, every
optimizer step's parameters and gradient on entry and on exit.  The checks a .. h of the audit (train_replay's docstring) are
separate tests over the record; for the five runs through train() the float64 oracle is also trained freely over the same batches,
stages and dropout fields, and the losses and every parameter's displacement compared (free_loss, free_disp).  After ar_train
and nar_train a model whose decoder / derived weights / AdaLN table were cached BEFORE training is compared, bit for bit,
with a fresh model built from the trained state dict.

Every bound is one the suite already uses for the same quantity on one step (train_replay.LOSS_TOL, GRAD_TOL, NORM_RTOL,
ADAMW_TOL).  The float32-versus-float64 figures below were measured on the CPU oracle by tests/test_train_steps_cpu.py, which
re-asserts them — none is taken from a kernel.

Measured on an MI355X (profiles/train_steps_gpu.log), the largest figure per check as a fraction of its bound, over all runs:
  a 0 (exact)    b 0.016 (ar_train)    c 7.4e-4 (ar_train: a gradient 7.4e-7 of its norm off)    d 5.6e-3 (ar_train)
  e 0.020 (ar_train, exp_avg_sq of proj.weight at the end)    f 0 (exact)    g 0 (exact)    h 0 (exact)
  free_loss 0.016 (ar_train: 1.6e-7 relative)    free_disp 0.34 (nar_train, layers.0.ffn.linear_2.weight: 1.0e-4 of its norm;
  ar_train 0.19, ar_dropout 0.11, nar_dropout 0.13, ar_nodes 0.08)
"""
import contextlib
import os
import random

import pytest

from tests import train_replay as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# torch's float32 AdamW against the float64 one on the float32 oracle's gradients of the run, in units of check e's bound
# (written_figure of the measurement): all inside it, so check e keeps test_flat_adamw_matches_torch_adamw_and_clip's bound
ADAMW_DRIFT = {'ar_train': 8.1e-2, 'nar_train': 4.0e-2, 'ar_dropout': 6.8e-2, 'nar_dropout': 2.4e-2, 'ar_nodes': 9.8e-2,
               'resume': 4.0e-2}
# (worst relative loss difference, worst relative displacement difference) of the float32 CPU oracle trainer against the float64
# one on the run; the device may be SUM_MARGIN times as far (the losses: at least rtol 1e-5)
FREE_FIGURES = {'ar_train': (2.1e-7, 3.0e-5), 'nar_train': (9.9e-8, 7.3e-5), 'ar_dropout': (1.1e-7, 7.7e-5),
                'nar_dropout': (1.4e-7, 7.0e-5), 'ar_nodes': (1.3e-7, 1.5e-4)}

PROBE_NEW = 6                      # forced decode steps of the inference probe


@contextlib.contextmanager
def _cwd(path):
    old = os.getcwd()
    os.chdir(path)                 # ConfigValle() creates its directories under the CWD
    try:
        yield
    finally:
        os.chdir(old)


def _to_cpu(obj):
    import torch
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


# ---- section 5: what a model computes at inference ---------------------------------------------------------------------------
def ar_probe(model):
    """Kept logits of a teacher-forced decode, {(use_graph, perf_mode): (2, PROBE_NEW, V + 1)}: the fp32 decoder and perf_mode=True
    (head width 64 at d_model 128: the shape allows it), each with the graph and without; and one free sampled decode (top_k 50, the seed given), so
    that a decoder of the call's shape survives in the model's slots."""
    import torch
    from valle2_amd import synth
    cfg = model.config
    pt, pc, tt = synth.synth_utterance(cfg, 5, 4, 9, seed=77)
    text, first = torch.cat([pt, tt]).to(DEV), pc[:, 0].to(DEV)
    forced = torch.randint(0, cfg.num_audio_tokens, (PROBE_NEW,), generator=torch.Generator().manual_seed(78))
    was = model.training
    model.eval()
    out = {}
    for perf in (False, True):
        for graph in (True, False):
            model.generate_batch([text] * 2, [first] * 2, max_new=PROBE_NEW, use_graph=graph, perf_mode=perf, forced=forced,
                                 keep_logits=list(range(PROBE_NEW)))
            kept = model.last_generate_stats['logits']
            out[(graph, perf)] = torch.stack([kept[t] for t in range(PROBE_NEW)], dim=1).cpu()
        torch.manual_seed(82)                                    # the call draws its sampling seed from torch's generator
        out[('tokens', perf)] = model.generate_batch([text] * 2, [first] * 2, max_new=PROBE_NEW, perf_mode=perf).cpu()
    model.train(was)
    return out


def nar_probe(model):
    """One stage's logits through the cached AdaLN table (stage_logits is what a stage of generate() runs), and generate()'s
    greedy codes."""
    import torch
    from valle2_amd import synth
    cfg = model.config
    batch = synth.synth_nar_batch(cfg, 2, n_tokens=8, n_frames=20, seed=79)
    pt, pc, tt = synth.synth_utterance(cfg, 5, 4, 9, seed=80)
    first = torch.randint(0, cfg.num_audio_tokens, (11,), generator=torch.Generator().manual_seed(81))
    was = model.training
    model.eval()
    with torch.no_grad():
        out = {('stage', s): model.stage_logits(batch, s)[0].cpu() for s in (2, 7)}
    out['codes'] = model.generate(pt.to(DEV), pc.to(DEV), tt.to(DEV), first.to(DEV), greedy=True).cpu()
    model.train(was)
    return out


PROBES = {'ar_train': ar_probe, 'nar_train': nar_probe}


# ---- the runs -----------------------------------------------------------------------------------------------------------------
def _by_hand_with_resume(run):
    """train()'s loop for a re-iterable dataset at world 1, written out; after `resume_at` steps the three state dicts go into a
    freshly built model, optimizer and scheduler (as a checkpoint on the host would hand them back), which take the rest."""
    import torch
    from valle2_amd import dropout, get_model_class
    spec, cfg, data = T.RUNS[run], T.config_of(run), T.dataset_of(run)
    accum = max(1, cfg.grad_accum)
    torch.manual_seed(cfg.seed)
    random.seed(cfg.seed)
    dropout.set_rank(0)

    def fresh():
        model = get_model_class(spec['model'])(cfg).to(DEV).train()
        conf = model.configure_optimizers()
        return model, conf['optimizer'], conf['lr_scheduler']

    model, optimizer, scheduler = fresh()
    optimizer.zero_grad()
    losses, epoch = [], 0
    for s, w in enumerate(T.plan_of(run)):
        if s == spec['resume_at']:
            saved = _to_cpu((model.state_dict(), optimizer.state_dict(), scheduler.state_dict()))
            states = torch.get_rng_state(), random.getstate()
            model, optimizer, scheduler = fresh()                      # other initial weights: everything comes from the load
            torch.set_rng_state(states[0])
            random.setstate(states[1])
            model.load_state_dict(saved[0])
            optimizer.load_state_dict(saved[1])
            scheduler.load_state_dict(saved[2])
            optimizer.zero_grad()
        while epoch < w['epoch']:
            scheduler.step()
            epoch += 1
        for b in w['batches']:
            loss = model.training_step(data[b])
            (loss / accum).backward()
            losses.append(loss.detach())
        optimizer.step(grad_scale=1.0, max_norm=cfg.gradient_clip_val, zero_grad=True)
    optimizer.check_errors()
    return model, [float(x) for x in losses]


def _do(run, tmp_path_factory):
    import torch
    from valle2_amd import dropout
    from valle2_amd.train_model import train
    probe, before = PROBES.get(run), {}
    hook = (lambda m: before.update(probe(m))) if probe else None
    # the run is defined by its config seed: the dropout seeds come from torch's generator, which train() seeds — not from a
    # private generator that an earlier test installed with dropout.manual_seed and left behind (put back afterwards)
    private, dropout._state['generator'] = dropout._state['generator'], None
    try:
        with _cwd(tmp_path_factory.mktemp(run)), T.record(run, before_first_forward=hook) as rec:
            if run == 'resume':
                model, losses = _by_hand_with_resume(run)
            else:
                model, losses = train(T.config_of(run), T.RUNS[run]['model'], batches=T.dataset_of(run), log=lambda *_: None)
    finally:
        dropout._state['generator'] = private
    with _cwd(tmp_path_factory.mktemp(run + '_audit')):
        rec.losses = losses
        torch.cuda.synchronize()
        rep = T.audit(rec, ADAMW_DRIFT[run], raise_on_failure=False)
        if run in T.FREE_RUNS:
            T.free_run(rec, FREE_FIGURES[run], rep)
    print('\n' + rep.line(run))
    return dict(rec=rec, model=model, rep=rep, before=before)


def _run_fixture(run):
    @pytest.fixture(scope='module', name=run)
    def fixture(tmp_path_factory):
        done = _do(run, tmp_path_factory)
        yield done
        getattr(done['model'], 'release_decoders', lambda: None)()         # the trained model's decoders and graphs
    return fixture


# one fixture per run, named after it: the run is done once, the tests below read its record
for _run in T.RUNS:
    globals()['_fixture_' + _run] = _run_fixture(_run)


CHECKS = list(T.CHECKS) + ['free_loss', 'free_disp']


# (the free-running comparison: on train_replay.FREE_RUNS, the runs through train())
CASES = [(run, check) for run in T.RUNS for check in CHECKS if run in T.FREE_RUNS or not check.startswith('free')]


@pytest.mark.parametrize('run,check', CASES, ids=[f'{r}-{c}' for r, c in CASES])
def test_train_steps(run, check, request):
    """Check `check` of the audit (a .. h), or of the free-running comparison, over the record of run `run`."""
    done = request.getfixturevalue(run)
    rep, rec = done['rep'], done['rec']
    assert len(rec.steps) == T.RUNS[run]['max_steps'] and len(rec.losses) == len(rec.micro) == T.plan_of(run)[-1]['micro'][-1] + 1
    assert [m['loss'] for m in rec.micro] == rec.losses          # what train() returns is what the steps computed
    assert check in rep.worst, f'check {check} did not run'
    if check == 'a':           # step 0 starts from the initial state dict: the model train() seeds and builds, built again on the CPU
        import torch
        init = T.initial_state(run)
        assert set(init) == set(rec.init) and all(torch.equal(rec.init[k], v) for k, v in init.items())
    print(f'TRAIN {run}: {check} {rep.worst[check][0]:.3g} of its bound ({rep.worst[check][1]})')
    mine = [m for c, m in rep.failed if c == check]
    assert not mine, f'{len(mine)} failed: ' + ' | '.join(mine[:12])


@pytest.mark.parametrize('run', list(T.RUNS))
def test_train_steps_run_is_what_it_is_meant_to_be(run, request):
    done = request.getfixturevalue(run)
    cfg, rec = T.config_of(run), done['rec']
    # the fields of every forward were recorded: two PositionalEncoding fields (live in train mode), three per layer with dropout
    assert all(len(m['fields']) == 2 + (3 * cfg.num_layers if cfg.dropout else 0) for m in rec.micro)
    # ... and their seeds are the draws that follow the model's construction under the config seed: the run is the one the CPU
    # oracle trainer makes (whose float32 figures the free-running bounds are)
    assert [sorted({f['seed'] for f in m['fields']}) for m in rec.micro] == [sorted(x) for x in T.drawn_seeds(run)]
    if T.RUNS[run]['model'] == 'ValleNAR':
        random.seed(cfg.seed)
        assert [m['stage'] for m in rec.micro] == [random.randint(1, cfg.num_quantizers - 1) for _ in rec.micro]
    if run in ('ar_train', 'ar_dropout', 'ar_nodes'):
        acted = [s['norm'] > s['max_norm'] for s in rec.steps]
        assert any(acted) and (run != 'ar_train' or (sum(acted) >= 2 and len(acted) - sum(acted) >= 2)), [s['norm'] for s in rec.steps]


# ---- section 5: training, then inference -------------------------------------------------------------------------------------
def _fresh_from(model):
    from valle2_amd import get_model_class
    fresh = get_model_class(type(model).__name__)(model.config)
    fresh.load_state_dict(_to_cpu(model.state_dict()))
    return fresh.to(DEV).eval()


@pytest.mark.parametrize('run', ['ar_train', 'nar_train'])
def test_inference_after_training_is_a_fresh_models(run, request, tmp_path_factory):
    """The trained model ran the probe BEFORE its first training forward (inside train()), so its decoders, folded / 16-bit
    weights and AdaLN tables were cached from the initial weights; after training the same calls must give, bit for bit, what a
    fresh model built from the trained state dict gives — with the graph and without, fp32 and perf_mode=True."""
    import torch
    done = request.getfixturevalue(run)
    model, before = done['model'], done['before']
    assert before, 'the probe did not run before training'
    with _cwd(tmp_path_factory.mktemp(run + '_probe')):
        after = PROBES[run](model)
        fresh = PROBES[run](_fresh_from(model))
    assert set(after) == set(fresh) == set(before)
    moved = [k for k in after if not torch.equal(after[k], before[k])]
    assert {k for k in after if k[0] in (True, False, 'stage')} <= set(moved), 'training did not change what inference computes'
    stale = [k for k in after if not torch.equal(after[k], fresh[k])]
    assert not stale, f'after training, {stale} differ from a fresh model built from the trained state dict'
