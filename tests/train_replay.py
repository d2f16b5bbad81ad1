"""Training over several optimizer steps, recorded and audited against a float64 trainer
(tests/test_train_steps_cpu.py, tests/test_train_steps_gpu.py).

A run is RECORDED (`record`, around `train()` or a loop written by hand): every micro-batch with its NAR stage, its dropout
fields and its loss; every optimizer step with the flat parameters, the flat gradient and `_touched` on entry (after
gather_grads()), and the returned norm, the flat parameters, the flat gradient and `slot_steps` on exit.  `oracle_train` is the
CPU oracle doing the same loop in float32 or float64; it writes a record of the same form (the float32 one stands in for the
device where there is none, with one `fault` planted where the audit must be shown to see it).

`audit` checks a record step by step, every step from the record's OWN pre-step parameters (lockstep):
  a  the parameters on entry of step s are bit for bit the ones step s - 1 left (s = 0: the initial state dict)
  b  every micro-batch loss against the float64 oracle at those parameters                         rtol 1e-5, atol 1e-6
  c  the flat gradient against the oracle's gradients summed over the window, each / accum         per parameter < 1e-3 of its
     norm; a parameter the window does not reach: an all-zero slice and `_touched` False
  d  the returned norm against the float64 norm of the recorded gradient x grad_scale              rtol 1e-5
  e  the update against float64 torch.optim.AdamW + clip_grad_norm_ fed the RECORDED gradient      rtol 2e-5, atol 2e-7
     (state carried over the whole run, through a resume too; a parameter without a gradient is skipped); at the end exp_avg,
     exp_avg_sq and slot_steps against the reference's state
  f  lr at step s equals, as a float, CosineAnnealingWarmRestarts stepped once per epoch
  g  after the step the flat gradient is exactly zero and every p.grad is None
  h  the (seed, site) pairs of all the forwards of the run are distinct
`free_run` trains the float64 oracle freely over the same batches, stages and fields and compares the losses and every
parameter's displacement.  Nothing is imported before a function needs it.
"""
import contextlib
import math
import random

ALIGN = 64                       # optim.ALIGN: every slot of the flat buffers starts on a multiple of 64 floats
CHECKS = 'abcdefgh'
LOSS_TOL = (1e-5, 1e-6)          # b: rtol, atol (test_train_gpu, test_dropout_gpu)
GRAD_TOL = 1e-3                  # c: _grad_check's bound
NORM_RTOL = 1e-5                 # d: test_flat_adamw_matches_torch_adamw_and_clip
ADAMW_TOL = (2e-5, 2e-7)         # e: the same test's rtol, atol
PE_P = 0.1                       # PositionalEncoding's dropout, live in train mode whatever config.dropout says
# dropout.py's site kinds
PE_TEXT, PE_AUDIO, ATTN_RES, FFN_HID, FFN_RES = 1, 2, 4, 5, 6

BASE = dict(d_model=128, dim_feedforward=256, num_layers=2, lr=3e-3, weight_decay=0.1, batch_size=3, log_every_n_steps=1000)
AR = dict(model='ValleAR', norm='LayerNorm', n_heads=2)
NAR = dict(model='ValleNAR', norm='AdaptiveLayerNorm', n_heads=2, gradient_clip_val=1.0, grad_accum=1, lr_warmup=2, batches=3)
AR_CLIP = 2.5                    # between the float64 oracle's norms of ar_train: acts on some steps, idle on others (asserted)
NAR_SEED = 1                     # the stage draws of nar_train (asserted in the CPU file)
# `batches`: the re-iterable dataset's length (an epoch); `data_seed`: of its first batch
RUNS = {
    'ar_train': dict(AR, dropout=0.0, grad_accum=2, max_steps=7, lr_warmup=2, gradient_clip_val=AR_CLIP, seed=5, batches=5, data_seed=100),
    'nar_train': dict(NAR, dropout=0.0, max_steps=8, seed=NAR_SEED, data_seed=200),
    'ar_dropout': dict(AR, dropout=0.1, grad_accum=2, max_steps=4, lr_warmup=2, gradient_clip_val=AR_CLIP, seed=6, batches=5, data_seed=300),
    'nar_dropout': dict(NAR, dropout=0.1, max_steps=4, seed=7, data_seed=420),
    'ar_nodes': dict(AR, n_heads=4, dropout=0.0, grad_accum=2, max_steps=3, lr_warmup=2, gradient_clip_val=AR_CLIP, seed=8, batches=5, data_seed=500),
    'resume': dict(NAR, dropout=0.0, max_steps=8, seed=NAR_SEED, data_seed=200, resume_at=4),
}
# The runs through train(): audited in lockstep AND compared free-running.  A free-running comparison needs runs whose small
# tensors stay clear of AdamW's eps where their whole displacement is first updates: the first update of an element is
# g / (|g| + eps), so an element of the clipped gradient near eps = 1e-8 moves by its own round-off (a cancellation residue), and
# in a vector of 128 elements that a run trains once or twice, one such element makes the vector's displacement error.  The
# data seeds are chosen so that no run has one below 1e-7 (asserted on the float32 CPU oracle, tests/test_train_steps_cpu.py:
# nar_dropout's data_seed 400 gave 1.9e-8 in stage_embs.3, 420 gives 5.9e-6).
FREE_RUNS = [r for r in RUNS if r != 'resume']


class AuditError(AssertionError):
    """'failed: <checks> | <every failed comparison, naming step, micro-batch and parameter>'."""


class Record:
    def __init__(self, run):
        self.run, self.model = run, RUNS[run]['model']
        self.layout = None           # [(name, offset, numel, shape)] of the flat buffers
        self.numel = 0
        self.init = None             # the state dict before the first forward (buffers included)
        self.micro = []              # dict(batch, stage, fields, loss)
        self.steps = []              # dict(micro, pre_param, pre_grad, touched, lr, grad_scale, max_norm, norm, post_param, post_grad, slot_steps, grads_left)
        self.losses = None           # what train() returned
        self.final = None            # dict(exp_avg, exp_avg_sq, slot_steps)
        self.resume_at = RUNS[run].get('resume_at')

    def unflat(self, flat):
        return {n: flat[o:o + k].view(shape) for n, o, k, shape in self.layout}


# ---- the runs ---------------------------------------------------------------------------------------------------------------
def config_of(run):
    from valle2_amd.config import ConfigValle
    kw = {k: v for k, v in RUNS[run].items() if k not in ('model', 'batches', 'data_seed', 'resume_at')}
    return ConfigValle(**BASE, **kw)


def dataset_of(run):
    """The run's re-iterable dataset: a list of collated batches of 3 rows (AR: 4..8 text and 10..20 audio tokens; NAR: 8 text
    tokens and 20 frames)."""
    from valle2_amd import synth
    spec, cfg = RUNS[run], config_of(run)
    if spec['model'] == 'ValleAR':
        return [synth.synth_ar_batch(cfg, 3, tok_range=(4, 8), code_range=(10, 20), seed=spec['data_seed'] + i) for i in range(spec['batches'])]
    return [synth.synth_nar_batch(cfg, 3, n_tokens=8, n_frames=20, seed=spec['data_seed'] + i) for i in range(spec['batches'])]


def plan(n_batches, accum, max_steps):
    """train()'s loop restated: per optimizer step dict(epoch, micro (indices into the run's micro-batches), batches (indices
    into the dataset)).  A window ends with the epoch (the step on an incomplete window), the scheduler steps per epoch."""
    out, micro, epoch = [], 0, 0
    while len(out) < max_steps:
        pending = []
        for b in range(n_batches):
            pending.append((micro, b))
            micro += 1
            if len(pending) == accum:
                out.append(dict(epoch=epoch, micro=[m for m, _ in pending], batches=[i for _, i in pending]))
                pending = []
                if len(out) >= max_steps:
                    break
        if pending and len(out) < max_steps:
            out.append(dict(epoch=epoch, micro=[m for m, _ in pending], batches=[i for _, i in pending]))
        epoch += 1
    return out


def plan_of(run):
    spec = RUNS[run]
    return plan(spec['batches'], max(1, spec['grad_accum']), spec['max_steps'])


def lr_schedule(run, epochs):
    """lr of epoch 0 .. epochs - 1: CosineAnnealingWarmRestarts over a torch optimizer stepped once per epoch."""
    import torch
    cfg = config_of(run)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cfg.lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, cfg.lr_warmup)
    out = []
    for _ in range(epochs):
        out.append(float(opt.param_groups[0]['lr']))
        opt.step()
        sched.step()
    return out


def initial_model(run):
    """The model as train() creates it: torch.manual_seed(config.seed), random.seed(config.seed), then the constructor (on the
    CPU).  Leaves both generators where train() has them before its first forward."""
    import torch
    from valle2_amd import get_model_class
    cfg = config_of(run)
    torch.manual_seed(cfg.seed)
    random.seed(cfg.seed)
    return get_model_class(RUNS[run]['model'])(cfg)


def drawn_seeds(run):
    """Per micro-batch of the run, the dropout seeds its forward draws from torch's generator after train() has seeded it and
    built the model: one for the PositionalEncoding fields, one more for the stack's with config.dropout > 0."""
    import torch
    initial_model(run)
    cfg, n = config_of(run), plan_of(run)[-1]['micro'][-1] + 1
    return [[int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2 if cfg.dropout > 0 else 1)] for _ in range(n)]


def initial_state(run):
    return {k: v.detach().clone() for k, v in initial_model(run).state_dict().items()}


def flat_layout(names, shapes):
    """optim.flat_layout restated over names: reverse registration order, slots aligned to 64 floats."""
    out, off = [], 0
    for n in reversed(list(names)):
        k = math.prod(shapes[n])
        out.append((n, off, k, tuple(shapes[n])))
        off += (k + ALIGN - 1) // ALIGN * ALIGN
    return out, off


# ---- recording a run on the device ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def record(run, before_first_forward=None):
    """Wraps optim.FlatAdamW.step and the model class's training_step while the body runs; yields the Record, complete when the
    body has ended.  before_first_forward(model): called once, inside the first training_step, before anything ran (the run's
    model is created inside train(): this is where a test reaches it); both CPU generators are put back afterwards.
    The recorded run is not the asynchronous one train() makes on its own: the step wrapper calls gather_grads() before the
    copies (step() calls it again: it changes nothing the second time) and copies the flat buffers and the norm to the host at
    every step, which waits for the device.  What the kernels compute is recorded; an ordering hazard between the update launch
    and the next forward's enqueue is outside what a record can show."""
    import torch
    from valle2_amd import dropout, get_model_class, optim
    rec = Record(run)
    cls = get_model_class(rec.model)
    orig_step, orig_ts = optim.FlatAdamW.step, cls.training_step
    seen = {'opt': None, 'models': [], 'since': []}

    def training_step(self, batch, **kw):
        if not any(m is self for m in seen['models']):
            seen['models'].append(self)
        if rec.init is None:
            rec.init = {k: v.detach().cpu().clone() for k, v in self.state_dict().items()}
            if before_first_forward is not None:
                states = torch.get_rng_state(), random.getstate()
                before_first_forward(self)
                torch.set_rng_state(states[0])
                random.setstate(states[1])
        outer, dropout.RECORD = dropout.RECORD, []
        before = random.getstate()
        try:
            loss = orig_ts(self, batch, **kw)
            fields = dropout.RECORD
        finally:
            dropout.RECORD = outer
        stage = kw.get('stage')
        if rec.model == 'ValleNAR' and not stage:             # the draw training_step made (valle_nar.py), read back
            after = random.getstate()
            random.setstate(before)
            stage = random.randint(1, self.config.num_quantizers - 1)
            assert random.getstate() == after
        seen['since'].append(len(rec.micro))
        rec.micro.append(dict(batch={k: v.detach().cpu().clone() for k, v in batch.items()}, stage=stage, fields=fields,
                              loss=loss.detach().clone()))
        return loss

    def step(self, closure=None, **kw):
        self.gather_grads()
        model = seen['models'][-1]
        names = {id(p): n for n, p in model.named_parameters()}
        layout = [(names[id(p)], off, n, tuple(p.shape)) for p, off, n in self.slots]
        assert rec.layout in (None, layout), 'the flat layout changed during the run'
        rec.layout, rec.numel, seen['opt'] = layout, self.numel, self
        ent = dict(micro=seen['since'], pre_param=self.flat_param.cpu(), pre_grad=self.flat_grad.cpu(), touched=list(self._touched),
                   lr=float(self.param_groups[0]['lr']), grad_scale=float(kw.get('grad_scale', 1.0)),
                   max_norm=float(kw.get('max_norm', 0.0)))
        seen['since'] = []
        norm = orig_step(self, closure, **kw)
        ent.update(norm=float(norm), post_param=self.flat_param.cpu(), post_grad=self.flat_grad.cpu(),
                   slot_steps=list(self.slot_steps), grads_left=[names[id(p)] for p, _, _ in self.slots if p.grad is not None])
        rec.steps.append(ent)
        return norm

    optim.FlatAdamW.step, cls.training_step = step, training_step
    try:
        yield rec
    finally:
        optim.FlatAdamW.step, cls.training_step = orig_step, orig_ts
    opt = seen['opt']
    if opt is not None:
        opt.check_errors()
        rec.final = dict(exp_avg=opt.exp_avg.cpu(), exp_avg_sq=opt.exp_avg_sq.cpu(), slot_steps=list(opt.slot_steps))
    for m in rec.micro:
        m['loss'] = float(m['loss'])


# ---- dropout fields ---------------------------------------------------------------------------------------------------------
def draw_fields(cfg, rows):
    """The fields one training forward draws, as dropout.RECORD lists them: one seed for the two PositionalEncoding dropouts,
    then (config.dropout > 0) one for the stack — each one draw from torch's CPU generator, as dropout.draw_seed makes it."""
    import numpy as np
    import torch
    d, dff = cfg.d_model, cfg.dim_feedforward
    p_pe, p = float(np.float32(PE_P)), float(np.float32(cfg.dropout))
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    out = [dict(name='tokens_position_emb.dropout', seed=seed, site=PE_TEXT, p=p_pe, rows=rows, cols=d),
           dict(name='audio_position_emb.dropout', seed=seed, site=PE_AUDIO, p=p_pe, rows=rows, cols=d)]
    if cfg.dropout > 0:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        for i in range(cfg.num_layers):
            out += [dict(name=f'layer{i}.dropout1', seed=seed, site=(i << 8) | ATTN_RES, p=p, rows=rows, cols=d),
                    dict(name=f'layer{i}.ffn.dropout', seed=seed, site=(i << 8) | FFN_HID, p=p, rows=rows, cols=dff),
                    dict(name=f'layer{i}.dropout2', seed=seed, site=(i << 8) | FFN_RES, p=p, rows=rows, cols=d)]
    return out


def oracle_dropout(cfg, fields, b, tx):
    """O.Dropout over recorded fields (oracle/philox.py restates the device's field; tests/test_dropout_gpu.py pins the two to
    each other bit for bit), each in the layout of the tensor it multiplies."""
    import torch
    from oracle import philox as P
    from oracle import valle_oracle as O
    masks = {}
    for r in fields:
        f = torch.from_numpy(P.keep_field(r['seed'], r['site'], r['p'], r['rows'], r['cols'])) != 0
        if r['name'] == 'tokens_position_emb.dropout':
            f = f.view(b, -1, r['cols'])[:, :tx]
        elif r['name'] == 'audio_position_emb.dropout':
            f = f.view(b, -1, r['cols'])[:, tx:]
        masks[r['name']] = f
    p_pe = PE_P if 'tokens_position_emb.dropout' in masks else 0.0
    p = cfg.dropout if any(n.startswith('layer') for n in masks) else 0.0
    return O.Dropout(p, p_pe, masks)


def batch_shape(model, batch):
    """(rows of the batch, text width, positions per row) of a training forward."""
    b, tx = batch['tokens'].shape[0], int(batch['tokens_lens'].max())
    t = int(batch['codes_lens'].max()) if model == 'ValleAR' else batch['codes'].shape[1]
    return b, tx, tx + t


def oracle_loss(model, cfg, params, batch, stage, fields):
    """The oracle's training loss of one micro-batch over `params` (in their dtype), with the fields given."""
    from oracle import valle_oracle as O
    b, tx, _ = batch_shape(model, batch)
    drop = oracle_dropout(cfg, fields, b, tx) if fields else None
    if model == 'ValleAR':
        return O.ar_training_loss(params, cfg, batch, drop)
    return O.nar_training_loss(params, cfg, batch, stage, drop)


def window_grads(model, cfg, state, micro, accum, dtype):
    """(losses, {name: gradient | None}) of the oracle over one accumulation window at `state` (a state dict, cast to dtype):
    every micro-batch's loss divided by accum before it is differentiated, the gradients added up as autograd adds them."""
    import torch
    params = {k: v.to(dtype).clone().requires_grad_(not k.endswith('.pe')) for k, v in state.items()}
    losses = []
    with torch.enable_grad():
        for m in micro:
            loss = oracle_loss(model, cfg, params, m['batch'], m['stage'], m['fields'])
            (loss / accum).backward()
            losses.append(float(loss.detach()))
    return losses, {k: v.grad for k, v in params.items() if not k.endswith('.pe')}


# ---- the oracle as a trainer ------------------------------------------------------------------------------------------------
FAULTS = ('stale_weights', 'stale_one_matrix', 'no_zero_grad', 'accum_unscaled', 'no_clip', 'decay_untouched', 'global_step_count',
          'lr_frozen', 'same_field_every_step', 'moments_reset_on_resume', 'weights_written_between_steps',
          'window_leaks_into_next_epoch')
STALE_MATRIX = 'transformer.layers.1.ffn.linear_1.weight'


def oracle_train(run, dtype, fault=None, replay=None):
    """train()'s loop (and, for 'resume', the loop by hand with the state carried over the resume) on the CPU oracle in `dtype`,
    AdamW and the clip written out in that dtype; returns a Record.  replay (a Record): its initial state, stages and fields
    are used instead of drawn.  fault: one of FAULTS planted — what a device could do wrong after the first step."""
    import torch
    assert fault is None or fault in FAULTS, fault
    spec, cfg, data = RUNS[run], config_of(run), dataset_of(run)
    model, accum = spec['model'], max(1, spec['grad_accum'])
    rec = Record(run)
    if replay is None:
        rec.init = {k: v.detach().clone() for k, v in initial_model(run).state_dict().items()}
    else:
        rec.init = replay.init
    names = [k for k in rec.init if not k.endswith('.pe')]
    rec.layout, rec.numel = flat_layout(names, {k: rec.init[k].shape for k in names})
    state = {k: v.to(dtype).clone() for k, v in rec.init.items()}
    exp_avg, exp_avg_sq = torch.zeros(rec.numel, dtype=dtype), torch.zeros(rec.numel, dtype=dtype)
    m1, m2 = rec.unflat(exp_avg), rec.unflat(exp_avg_sq)
    counts = {n: 0 for n in names}
    flat_grad = torch.zeros(rec.numel, dtype=dtype)
    gview = rec.unflat(flat_grad)
    touched = {n: False for n in names}
    b1, b2 = cfg.betas
    lrs = lr_schedule(run, 4 * spec['max_steps'])
    epoch, losses, since, stale, first_fields = 0, [], [], None, None

    def flat_of(d):
        flat = torch.zeros(rec.numel, dtype=dtype)
        for n, t in rec.unflat(flat).items():
            t.copy_(d[n])
        return flat

    def forward_backward(batch):
        nonlocal first_fields
        i = len(rec.micro)
        if replay is not None:
            stage, fields = replay.micro[i]['stage'], replay.micro[i]['fields']
        else:
            stage = random.randint(1, cfg.num_quantizers - 1) if model == 'ValleNAR' else None
            b, _, T = batch_shape(model, batch)
            fields = draw_fields(cfg, b * T)
            if fault == 'same_field_every_step':
                first_fields = first_fields or {f['name']: f['seed'] for f in fields}
                fields = [dict(f, seed=first_fields[f['name']]) for f in fields]
        m = dict(batch=batch, stage=stage, fields=fields)
        at = stale if (fault == 'stale_weights' and stale is not None) else state
        scale = 1 if fault == 'accum_unscaled' else accum
        loss, grads = window_grads(model, cfg, at, [m], scale, dtype)
        if fault == 'stale_one_matrix' and stale is not None:
            grads[STALE_MATRIX] = window_grads(model, cfg, stale, [m], scale, dtype)[1][STALE_MATRIX]
        for n, g in grads.items():
            if g is not None:
                gview[n].add_(g)
                touched[n] = True
        m['loss'] = loss[0]
        since.append(i)
        rec.micro.append(m)
        losses.append(loss[0])

    def optimizer_step():
        nonlocal since, stale
        s = len(rec.steps)
        if fault == 'moments_reset_on_resume' and s == rec.resume_at:
            exp_avg.zero_()
            exp_avg_sq.zero_()
        lr = lrs[0] if fault == 'lr_frozen' else lrs[epoch]
        ent = dict(micro=since, pre_param=flat_of(state).float(), pre_grad=flat_grad.float().clone(), touched=[touched[n] for n, *_ in rec.layout],
                   lr=lr, grad_scale=1.0, max_norm=float(cfg.gradient_clip_val))
        since = []
        stale = {k: v.clone() for k, v in state.items()}
        norm = flat_grad.double().norm().to(dtype)           # (vh_adamw_flat adds its partial sums up in float64 too)
        coef = 1.0
        if cfg.gradient_clip_val > 0 and fault != 'no_clip':
            coef = min(1.0, float(cfg.gradient_clip_val / (norm + 1e-6)))
        for n in names:
            p = state[n]
            if not touched[n]:
                if fault == 'decay_untouched':
                    p.mul_(1 - lr * cfg.weight_decay)
                continue
            counts[n] += 1
            t = s + 1 if fault == 'global_step_count' else counts[n]
            g = gview[n] * coef
            p.mul_(1 - lr * cfg.weight_decay)
            m1[n].mul_(b1).add_(g, alpha=1 - b1)
            m2[n].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (m2[n].sqrt() / math.sqrt(1 - b2 ** t)).add_(1e-8)
            p.addcdiv_(m1[n], denom, value=-lr / (1 - b1 ** t))
        if fault != 'no_zero_grad':
            flat_grad.zero_()
        for n in names:
            touched[n] = False
        ent.update(norm=float(norm), post_param=flat_of(state).float(), post_grad=flat_grad.float().clone(),
                   slot_steps=[counts[n] for n, *_ in rec.layout], grads_left=[n for n in names if fault == 'no_zero_grad'])
        rec.steps.append(ent)
        if fault == 'weights_written_between_steps' and s == 2:
            state[STALE_MATRIX].mul_(1 + 2.0 ** -20)

    def steps():
        return len(rec.steps)

    while steps() < cfg.max_steps:
        pending = 0
        for batch in data:
            pending = len(since) + 1
            forward_backward(batch)
            if pending == accum:
                optimizer_step()
                if steps() >= cfg.max_steps:
                    break
        if since and steps() < cfg.max_steps and fault != 'window_leaks_into_next_epoch':
            optimizer_step()
        epoch += 1
    rec.losses = losses
    rec.final = dict(exp_avg=exp_avg.float(), exp_avg_sq=exp_avg_sq.float(), slot_steps=[counts[n] for n, *_ in rec.layout])
    rec.end_state = state
    return rec


# ---- the audit --------------------------------------------------------------------------------------------------------------
class _Report:
    def __init__(self):
        self.worst, self.failed = {}, []

    def note(self, check, ratio, what):
        """ratio: the figure over its bound (<= 1 passes; a NaN fails)."""
        if check not in self.worst or not ratio <= self.worst[check][0]:
            self.worst[check] = (ratio, what)
        if not ratio <= 1.0:
            self.failed.append((check, f'{check}: {what}: {ratio:.3g} x the bound'))

    def exact(self, check, ok, what):
        self.worst.setdefault(check, (0.0, 'exact'))
        if not ok:
            self.worst[check] = (float('inf'), what)
            self.failed.append((check, f'{check}: {what}'))

    def line(self, run):
        return f'TRAIN {run}: worst ' + ' '.join(f'{c} {self.worst[c][0]:.3g}' for c in sorted(self.worst))

    def raise_if_failed(self):
        if self.failed:
            names = sorted({c for c, _ in self.failed})
            raise AuditError('failed: ' + ', '.join(names) + ' | ' + ' | '.join(m for _, m in self.failed[:40]))


def _miss(got, ref, rtol, atol):
    d = (got.double() - ref.double()).abs() / (atol + rtol * ref.double().abs())
    return float(d.max()) if d.numel() else 0.0


def adamw_reference(rec, dtype, report=None, adamw_factor=1.0):
    """torch.optim.AdamW + clip_grad_norm_ in `dtype`, fed the record's gradients, each step from the record's pre-step
    parameters, its moments and step counts carried over the whole run.  Returns the post-step parameters per step (dicts) and
    the optimizer; with a report, checks e against them."""
    import torch
    cfg = config_of(rec.run)
    names = [n for n, *_ in rec.layout]
    params = {n: torch.nn.Parameter(torch.zeros(shape, dtype=dtype)) for n, _, _, shape in rec.layout}
    opt = torch.optim.AdamW(list(params.values()), lr=cfg.lr, betas=tuple(cfg.betas), eps=1e-8, weight_decay=cfg.weight_decay)
    out = []
    for s, st in enumerate(rec.steps):
        pre, grad, post = rec.unflat(st['pre_param']), rec.unflat(st['pre_grad']), rec.unflat(st['post_param'])
        with torch.no_grad():
            for n in names:
                params[n].copy_(pre[n])
        for i, n in enumerate(names):
            params[n].grad = (grad[n].to(dtype) * st['grad_scale']) if st['touched'][i] else None
        if st['max_norm'] > 0:
            torch.nn.utils.clip_grad_norm_(list(params.values()), st['max_norm'])
        opt.param_groups[0]['lr'] = st['lr']
        opt.step()
        out.append({n: params[n].detach().clone() for n in names})
        if report is not None:
            for n in names:
                report.note('e', _miss(post[n], out[-1][n], *ADAMW_TOL) / adamw_factor, f'step {s} {n} after the update')
    return out, opt, params


def adamw_drift(rec):
    """How far torch's float32 AdamW is from the float64 one on this record's gradients, in units of ADAMW_TOL (check e's bound)."""
    import torch
    p32, _, _ = adamw_reference(rec, torch.float32)
    p64, _, _ = adamw_reference(rec, torch.float64)
    return max(_miss(a[n], b[n], *ADAMW_TOL) for a, b in zip(p32, p64) for n in a)


def audit(rec, adamw_written=0.0, raise_on_failure=True):
    """Checks a .. h over a Record; adamw_written: the written float32-versus-float64 drift of check e (in units of its bound).
    Returns the report (`.worst[check] = (figure over bound, where)`, `.line(run)`); raises AuditError naming every failed
    check."""
    import torch
    from tests import oracle_runners as R
    run, spec, cfg = rec.run, RUNS[rec.run], config_of(rec.run)
    model, accum = spec['model'], max(1, spec['grad_accum'])
    rep = _Report()
    windows, data = plan_of(run), dataset_of(run)
    names = [n for n, *_ in rec.layout]
    buffers = {k: v for k, v in rec.init.items() if k.endswith('.pe')}
    lrs = lr_schedule(run, windows[-1]['epoch'] + 1)
    adamw_factor = max(1.0, R.SUM_MARGIN * adamw_written)
    rep.exact('c', len(rec.steps) == len(windows), f'{len(rec.steps)} optimizer steps, the loop takes {len(windows)}')
    for s, (st, w) in enumerate(zip(rec.steps, windows)):
        pre = rec.unflat(st['pre_param'])
        # a: nothing writes weights between the steps
        if s == 0:
            bad = [n for n in names if not torch.equal(pre[n], rec.init[n])]
        else:
            bad = [] if torch.equal(st['pre_param'], rec.steps[s - 1]['post_param']) else \
                [n for n, t in rec.unflat(rec.steps[s - 1]['post_param']).items() if not torch.equal(pre[n], t)]
        rep.exact('a', not bad, f'step {s}: parameters on entry differ from what step {s - 1} left ({", ".join(bad[:3])})')
        # the window: the micro-batches the loop hands to this step, and their batches
        rep.exact('c', st['micro'] == w['micro'], f'step {s}: gradient of micro-batches {st["micro"]}, the window is {w["micro"]}')
        micro = [rec.micro[i] for i in w['micro'] if i < len(rec.micro)]
        for m, bi in zip(micro, w['batches']):
            same = all(torch.equal(m['batch'][k], data[bi][k]) for k in data[bi])
            rep.exact('c', same, f'step {s}: a micro-batch is not batch {bi} of the dataset')
        # b, c: losses and the summed gradient against the float64 oracle at the pre-step parameters
        ref_losses, ref = window_grads(model, cfg, dict(pre, **buffers), micro, accum, torch.float64)
        for i, m, rl in zip(w['micro'], micro, ref_losses):
            err = abs(m['loss'] - rl) / (LOSS_TOL[1] + LOSS_TOL[0] * abs(rl))
            rep.note('b', err, f'step {s} micro-batch {i} loss {m["loss"]:.7f} against {rl:.7f}')
        got = rec.unflat(st['pre_grad'])
        for i, n in enumerate(names):
            if ref[n] is None:
                ok = not st['touched'][i] and float(got[n].abs().max()) == 0.0
                rep.exact('c', ok, f'step {s} {n}: the window does not reach it, touched {st["touched"][i]}, max |gradient| {float(got[n].abs().max()):.3e}')
            else:
                rep.exact('c', st['touched'][i], f'step {s} {n}: reached by the window but not marked touched')
                err = float((got[n].double() - ref[n]).norm()) / max(float(ref[n].norm()), 1e-300)
                rep.note('c', err / GRAD_TOL, f'step {s} {n} relative gradient error {err:.2e}')
        # d: the returned norm, of the recorded gradient
        want = float(st['pre_grad'].double().norm()) * st['grad_scale']
        rep.note('d', abs(st['norm'] - want) / (NORM_RTOL * want), f'step {s} norm {st["norm"]:.7g} against {want:.7g}')
        # f: the scheduler steps once per epoch
        rep.exact('f', st['lr'] == lrs[w['epoch']], f'step {s} (epoch {w["epoch"]}): lr {st["lr"]!r}, the scheduler gives {lrs[w["epoch"]]!r}')
        # g: the step leaves no gradient behind
        left = int(st['post_grad'].count_nonzero())
        rep.exact('g', left == 0 and not st['grads_left'], f'step {s}: {left} non-zero elements left in the flat gradient, p.grad kept by {st["grads_left"][:3]}')
    # e: the update, the state carried over the run
    _, opt, params = adamw_reference(rec, torch.float64, rep, adamw_factor)
    if rec.final is not None:
        for i, n in enumerate(names):
            state = opt.state.get(params[n], {})
            steps = int(state['step']) if state else 0
            rep.exact('e', rec.final['slot_steps'][i] == steps, f'{n}: slot_steps {rec.final["slot_steps"][i]} at the end, torch counts {steps}')
            for key in ('exp_avg', 'exp_avg_sq'):
                want = state[key] if state else torch.zeros_like(params[n])
                rep.note('e', _miss(rec.unflat(rec.final[key])[n], want, *ADAMW_TOL) / adamw_factor, f'{n} {key} at the end')
    # h: every forward drew its own fields
    pairs = [(f['seed'], f['site']) for m in rec.micro for f in m['fields']]
    if pairs:
        rep.exact('h', len(set(pairs)) == len(pairs), f'{len(pairs) - len(set(pairs))} (seed, site) pairs repeat among {len(pairs)} fields')
    if raise_on_failure:
        rep.raise_if_failed()
    return rep


# ---- free-running -----------------------------------------------------------------------------------------------------------
def displacement(rec, end):
    """{name: p_N - p_0} in float64; end: a flat post-step buffer or a state dict."""
    end = rec.unflat(end) if not isinstance(end, dict) else end
    return {n: end[n].double() - rec.init[n].double() for n, *_ in rec.layout}


def free_deviation(rec, ref):
    """(worst relative loss difference, worst relative displacement difference over the parameters) of a record against the
    float64 oracle trained freely (`ref = oracle_train(run, float64, replay=rec)`).  A parameter that no step reached has not
    moved in either."""
    loss = max(abs(a - b) / abs(b) for a, b in zip(rec.losses, ref.losses)) if len(rec.losses) == len(ref.losses) else float('inf')
    got, want = displacement(rec, rec.steps[-1]['post_param']), displacement(ref, ref.end_state)
    disp = {}
    for n in got:
        den = float(want[n].norm())
        num = float((got[n] - want[n]).norm())
        disp[n] = num / den if den > 0 else (0.0 if num == 0 else float('inf'))
    worst = max(disp, key=disp.get)
    return loss, disp[worst], worst


def free_run(rec, written, report):
    """Section 3: the record against the float64 oracle trained freely from the same initial state dict over the same batches,
    stages and fields; written = (loss, displacement): the float32 CPU oracle trainer's deviations on this run."""
    import torch
    from tests import oracle_runners as R
    ref = oracle_train(rec.run, torch.float64, replay=rec)
    loss, disp, where = free_deviation(rec, ref)
    report.note('free_loss', loss / max(LOSS_TOL[0], R.SUM_MARGIN * written[0]), f'free-running losses differ by {loss:.2e} relative')
    report.note('free_disp', disp / (R.SUM_MARGIN * written[1]), f'{where}: displacement differs by {disp:.2e} of its norm')
    return ref
