"""Packed AR training on the GPU: the two training forms of the packed attention against the padded kernels (bit for bit,
segment by segment) and float64, and `ValleAR.training_step_packed` against the real reference's per-utterance results
(tests/golden/ar_train_packed.npz), the float64 oracle, `training_step` and `train()`.

Bounds are the suite's own: the forward's atol 3e-5 and the backward's atol 6e-5 + rtol 1e-4 (tests/oracle_runners.py
ATTN_TOL, what tests/test_attn_geometry_gpu.py holds the padded kernels to), train_replay.LOSS_TOL and GRAD_TOL."""
import functools
import math

import pytest
import torch

from tests import attn_scores as S
from tests import oracle_runners as R
from tests import train_replay as T
from tests.golden import cases as C
from tests.golden import gen_golden_train_packed as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = 2
LENS = [1, 31, 32, 33, 127, 128, 129, 257, 300]
XLENS = [0, 7, 32, 33, 1, 128, 129, 200, 300]
ORDERS = {'given': list(range(9)), 'shuffled': [5, 0, 8, 2, 7, 1, 4, 6, 3]}     # starts are no multiples of 32 or 128
MODES = {'full': 0, 'prefix': 1}                                              # VH_MASK_FULL, VH_MASK_PREFIX
POISON = 12345.0
PAD_ROWS = 64                                                                 # rows behind M that must stay poisoned


def layout(order):
    lens, xlens = [LENS[i] for i in ORDERS[order]], [XLENS[i] for i in ORDERS[order]]
    starts = [sum(lens[:i]) for i in range(len(lens))]
    return lens, xlens, starts, sum(lens)


@functools.lru_cache(maxsize=None)
def operands(order, score_set):
    """q, dout (M, 128), k, v (1, 2, M, 64) fp32 on the CPU: per segment seeded operands with the scores moved as
    tests/attn_scores.py moves them (every key of a segment is seen by its last query under either mask).  Shared."""
    lens, _, _, M = layout(order)
    qs, ks, vs = [], [], []
    for i, n in enumerate(lens):
        gen = torch.Generator().manual_seed(7000 + 10 * ORDERS[order][i])
        q, k, v = (torch.randn(1, H, n, 64, generator=gen) for _ in range(3))
        add, sign = S.row_amounts(torch.ones(n, dtype=torch.bool), n, score_set)
        q, k = S.move_scores(q, k, add[None], sign, 7001 + 10 * ORDERS[order][i])
        qs.append(q[0].permute(1, 0, 2).reshape(n, H * 64))
        ks.append(k[0])
        vs.append(v[0])
    dout = torch.randn(M, H * 64, generator=torch.Generator().manual_seed(7999))
    return torch.cat(qs).contiguous(), torch.cat(ks, 1)[None].contiguous(), torch.cat(vs, 1)[None].contiguous(), dout


def visible(n, xl, mode):
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    return torch.ones(n, n, dtype=torch.bool) if mode == 'full' else (j < xl) | ((i >= xl) & (j <= i))


@functools.lru_cache(maxsize=None)
def reference(order, score_set, mode):
    """float64 over the same operands, segment by segment: out, dq, dk, dv (M, 128) and lse2 (2, M) in base 2."""
    lens, xlens, starts, M = layout(order)
    q, k, v, dout = operands(order, score_set)
    out, lse2 = torch.zeros(M, H * 64, dtype=torch.float64), torch.zeros(H, M, dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(out), torch.zeros_like(out), torch.zeros_like(out)
    flat = lambda t, n: t.permute(1, 0, 2).reshape(n, H * 64)                 # noqa: E731
    for n, xl, s0 in zip(lens, xlens, starts):
        qs = q[s0:s0 + n].double().view(n, H, 64).permute(1, 0, 2).clone().requires_grad_()
        ks, vs = k[0, :, s0:s0 + n].double().clone().requires_grad_(), v[0, :, s0:s0 + n].double().clone().requires_grad_()
        sc = (qs @ ks.transpose(-1, -2) / 8).masked_fill(~visible(n, xl, mode), -math.inf)
        o = flat(torch.softmax(sc, -1) @ vs, n)
        o.backward(dout[s0:s0 + n].double())
        out[s0:s0 + n], lse2[:, s0:s0 + n] = o.detach(), torch.logsumexp(sc.detach(), -1) * S.LOG2E
        dq[s0:s0 + n], dk[s0:s0 + n], dv[s0:s0 + n] = flat(qs.grad, n), flat(ks.grad, n), flat(vs.grad, n)
    return out, lse2, dq, dk, dv


def packed_forward(order, score_set, mode):
    """(rows, device operands, out with its poisoned tail, lse2) of one vh_attn_rows_packed_lse launch."""
    from valle2_amd import engine, kernels
    lens, xlens, _, M = layout(order)
    rows = engine.PackedRows(lens, DEV, x_lens=xlens)
    q, k, v, dout = (t.to(DEV) for t in operands(order, score_set))
    out = torch.full((M + PAD_ROWS, H * 64), POISON, device=DEV)
    lse2 = torch.full((H, M), POISON, device=DEV)
    kernels.attn_rows_packed_lse(q, k, v, out[:M], lse2, H, rows, MODES[mode])
    return rows, (q, k, v, dout), out, lse2


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('order', list(ORDERS))
def test_packed_forward_is_the_padded_forward_of_each_segment_alone(order, mode):
    from valle2_amd import kernels
    lens, xlens, starts, M = layout(order)
    _, (q, k, v, _), out, lse2 = packed_forward(order, 'plain', mode)
    assert bool((out[M:] == POISON).all()), 'rows beyond M were written'
    assert not bool((out[:M] == POISON).any()) and not bool((lse2 == POISON).any())
    for n, xl, s0 in zip(lens, xlens, starts):
        o1 = torch.empty(n, H * 64, device=DEV)
        l1 = torch.empty(1, H, n, device=DEV)
        kernels.attn_rows(q[s0:s0 + n], k[:, :, s0:s0 + n].contiguous(), v[:, :, s0:s0 + n].contiguous(), o1, 1, H, n, n,
                          MODES[mode], x_len=xl, lse2=l1)
        assert torch.equal(out[s0:s0 + n], o1), f'out of the segment of {n} rows at {s0} ({mode})'
        assert torch.equal(lse2[:, s0:s0 + n], l1[0]), f'lse2 of the segment of {n} rows at {s0} ({mode})'
    ref_out, ref_lse2, *_ = reference(order, 'plain', mode)
    torch.testing.assert_close(out[:M].cpu(), ref_out.float(), atol=R.ATTN_TOL['out'][0], rtol=R.ATTN_TOL['out'][1])
    torch.testing.assert_close(lse2.cpu(), ref_lse2.float(), atol=1e-4, rtol=1e-6)       # (bit-pinned above; a sanity bound)


@pytest.mark.parametrize('chunk_keys', [256, 128])                     # the 300-row segment in two chunks, and in three
@pytest.mark.parametrize('score_set', ['plain', 'peak'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('order', list(ORDERS))
def test_packed_backward_against_float64(order, mode, score_set, chunk_keys):
    from valle2_amd import kernels
    _, _, _, M = layout(order)
    rows, (q, k, v, dout), out, lse2 = packed_forward(order, score_set, mode)
    assert rows.bwd_table(chunk_keys)[1] == -(-300 // chunk_keys)
    ref = reference(order, score_set, mode)
    runs = []
    for _ in range(2):
        g = torch.full((M + PAD_ROWS, 3 * H * 64), POISON, device=DEV)
        d = H * 64
        kernels.attn_rows_bwd_packed(q, k, v, out[:M], dout, lse2, g[:M, :d], g[:M, d:2 * d], g[:M, 2 * d:], H, rows, MODES[mode],
                                     chunk_keys=chunk_keys)
        runs.append(g)
    g = runs[0]
    assert torch.equal(runs[0], runs[1]), 'two launches differ'
    assert bool((g[M:] == POISON).all()), 'rows beyond M were written'
    assert not bool((g[:M] == POISON).any()), 'a row of dq / dk / dv in [0, M) was not written'
    d = H * 64
    for name, got, want in (('dq', g[:M, :d], ref[2]), ('dk', g[:M, d:2 * d], ref[3]), ('dv', g[:M, 2 * d:], ref[4])):
        atol, rtol = R.ATTN_TOL[name]
        err = (got.cpu().double() - want).abs()
        worst = float((err - rtol * want.abs()).max())
        print(f'{order} {mode} {score_set} chunk_keys={chunk_keys} {name}: max|err|={float(err.max()):.3e} worst over rtol={worst:.3e}')
        torch.testing.assert_close(got.cpu(), want.float(), atol=atol, rtol=rtol, msg=lambda m: f'{name}: {m}')


# ---- the model -------------------------------------------------------------------------------------------------------
def _device_model(kw, sd, pe_p=None):
    from valle2_amd import get_model_class
    model = get_model_class('ValleAR')(C.cfg_of(kw))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    if pe_p is not None:
        model.tokens_position_emb.dropout.p = pe_p
        model.audio_position_emb.dropout.p = pe_p
    return model


def _weights():
    w = torch.tensor(G.AUDIO_LENS, dtype=torch.float64)
    return w / w.sum()


def _check_grads(model, want, what):
    """Every parameter's gradient within GRAD_TOL of the norm of `want[name]` (float64, full gradients)."""
    for n, p in model.named_parameters():
        assert p.grad is not None, f'no gradient reached {n}'
        err = float((p.grad.detach().cpu().double() - want[n]).norm()) / max(float(want[n].norm()), 1e-12)
        assert err < T.GRAD_TOL, f'{what}: {n}: relative gradient error {err:.2e}'


@pytest.fixture(scope='module')
def oracle64():
    kw, sd, batch = G.train_packed_inputs()
    per = [R.oracle_training_loss(sd, C.cfg_of(kw), G.utterance_batch(batch, b), 'ValleAR') for b in range(len(G.TEXT_LENS))]
    w = _weights()
    names = G.param_names(sd)
    return (sum(wi * l for wi, (l, _) in zip(w, per)), {n: sum(wi * p[n].grad for wi, (_, p) in zip(w, per)) for n in names})


def test_training_step_packed_against_the_reference_per_utterance(oracle64):
    gold = R.load_golden('ar_train_packed')
    kw, sd, batch = G.train_packed_inputs()
    model = _device_model(kw, sd, pe_p=0.0)
    loss = model.training_step_packed({k: v.clone() for k, v in batch.items()})
    loss.backward()
    w = _weights()
    want = sum(float(wi) * float(gold[f'loss_{b}']) for b, wi in enumerate(w))
    print(f'packed loss {float(loss.detach()):.8f}, the reference per utterance token-weighted {want:.8f}, float64 oracle {float(oracle64[0]):.8f}')
    assert abs(float(loss) - want) <= T.LOSS_TOL[0] * abs(want) + T.LOSS_TOL[1]
    names, grads = G.param_names(sd), dict(model.named_parameters())
    samples = sum(wi * gold[f'grad_samples_{b}'].double() for b, wi in enumerate(w))
    off = 0
    for n in names:                                      # the reference's own gradients where the fixture keeps them
        idx = G.sample_index(grads[n].numel())
        ref = samples[off:off + idx.numel()]
        off += idx.numel()
        got = grads[n].grad.detach().cpu().double().reshape(-1)[idx]
        err = float((got - ref).norm()) / max(float(ref.norm()), 1e-12)
        assert err < T.GRAD_TOL, f'{n}: relative gradient error {err:.2e} against the reference'
    _check_grads(model, oracle64[1], 'float64 oracle')   # and every element against the oracle the CPU test pins to them
    with torch.no_grad():                                # the same value without a graph
        again = model.training_step_packed({k: v.clone() for k, v in batch.items()})
    assert again.grad_fn is None and abs(float(again) - float(loss)) <= T.LOSS_TOL[0] * abs(want) + T.LOSS_TOL[1]


def test_training_step_packed_dropout_fields_replayed_by_the_oracle():
    from oracle import valle_oracle as O
    from valle2_amd import dropout
    kw, sd, batch = G.train_packed_inputs()
    kw = dict(kw, dropout=0.1)
    cfg = C.cfg_of(kw)
    model = _device_model(kw, sd)
    dropout.RECORD = []
    try:
        torch.manual_seed(11)
        loss = model.training_step_packed({k: v.clone() for k, v in batch.items()})
        loss.backward()
        recs = dropout.RECORD
    finally:
        dropout.RECORD = None
    M = sum(G.TEXT_LENS) + sum(G.AUDIO_LENS)
    assert sorted(r['name'] for r in recs) == sorted(['tokens_position_emb.dropout', 'audio_position_emb.dropout'] +
                                                     [f'layer{i}.{s}' for i in range(2) for s in ('dropout1', 'ffn.dropout', 'dropout2')])
    assert all(r['rows'] == M for r in recs)
    fields = {r['name']: dropout.mask(dropout.spec(r['seed'], r['site'], r['p']), r['rows'], r['cols'], DEV).cpu() != 0 for r in recs}
    w, names = _weights(), G.param_names(sd)
    want_loss, want = 0.0, {n: 0.0 for n in names}
    s0 = 0
    for b, (tl, cl) in enumerate(zip(G.TEXT_LENS, G.AUDIO_LENS)):       # the fields sliced per utterance: keyed on the packed row
        masks = {}
        for name, f in fields.items():
            rows = slice(s0, s0 + tl) if name.startswith('tokens_') else slice(s0 + tl, s0 + tl + cl) if name.startswith('audio_') \
                else slice(s0, s0 + tl + cl)
            masks[name] = f[rows][None]
        params = {k: v.double().clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
        ub = G.utterance_batch(batch, b)
        with torch.enable_grad():
            lb = torch.nn.functional.cross_entropy(O.ar_logits(params, cfg, ub, O.Dropout(cfg.dropout, masks=masks)), ub['target'])
            lb.backward()
        want_loss += float(w[b]) * float(lb)
        for n in names:
            want[n] = want[n] + w[b] * params[n].grad
        s0 += tl + cl
    print(f'packed loss under dropout {float(loss.detach()):.8f}, float64 oracle with the exported fields {want_loss:.8f}')
    assert abs(float(loss) - want_loss) <= T.LOSS_TOL[0] * abs(want_loss) + T.LOSS_TOL[1]
    _check_grads(model, want, 'oracle with the exported fields')


def test_equal_lengths_give_the_loss_of_training_step():
    from valle2_amd import synth
    kw, sd, _ = G.train_packed_inputs()
    batch = synth.synth_ar_batch(C.cfg_of(kw), 3, tok_range=(6, 6), code_range=(15, 15), seed=77)
    model = _device_model(kw, sd, pe_p=0.0)
    padded = model.training_step({k: v.clone() for k, v in batch.items()})
    packed = model.training_step_packed({k: v.clone() for k, v in batch.items()})
    assert abs(float(packed) - float(padded)) <= T.LOSS_TOL[0] * abs(float(padded)) + T.LOSS_TOL[1], (float(packed), float(padded))


# training_step on the fixture's batch (train mode, PositionalEncoding dropout set to 0), recorded on the commit before the
# packed path existed.  The gradient is reproducible there and is pinned bit for bit: the sum of layer 0's QKV weight gradient
# (float64 sum of the float32 elements) as hex.  The loss is not — vh_cross_entropy adds the rows' terms up in an order that is
# not fixed, and two runs of that commit returned 0x1.c4a624p+2 and 0x1.c4a620p+2 — so it is held to 4 ulp of the first.
PARENT_TRAINING_STEP = {'loss': '0x1.c4a6240000000p+2', 'qkv_grad_sum': '-0x1.8d7fb663c2180p-5'}


def test_training_step_keeps_its_bits():
    kw, sd, batch = G.train_packed_inputs()
    model = _device_model(kw, sd, pe_p=0.0)
    loss = model.training_step({k: v.clone() for k, v in batch.items()})
    loss.backward()
    qkv = dict(model.named_parameters())['transformer.layers.0.self_attn.qkv.weight'].grad
    got = {'loss': float(loss.detach()).hex(), 'qkv_grad_sum': float(qkv.double().sum()).hex()}
    print(got)
    assert got['qkv_grad_sum'] == PARENT_TRAINING_STEP['qkv_grad_sum']
    parent_loss = float.fromhex(PARENT_TRAINING_STEP['loss'])
    assert abs(float(loss.detach()) - parent_loss) <= 4 * 2.0 ** -23 * parent_loss


def _train_three_steps(monkeypatch, packed):
    from valle2_amd import get_model_class, synth, train_model
    from valle2_amd.config import ConfigValle
    if packed:
        monkeypatch.setenv('VALLE2_TRAIN_PACKED', '1')
    else:
        monkeypatch.delenv('VALLE2_TRAIN_PACKED', raising=False)
    cfg = ConfigValle(**G.KW, max_steps=3, batch_size=3, grad_accum=1, log_every_n_steps=1000, seed=3)
    batches = [synth.synth_ar_batch(cfg, 3, tok_range=(4, 8), code_range=(10, 20), seed=900 + i) for i in range(3)]
    cls = get_model_class('ValleAR')
    calls, orig = [], cls.training_step_packed

    def spy(self, batch, **kw):
        calls.append(1)
        return orig(self, batch, **kw)
    monkeypatch.setattr(cls, 'training_step_packed', spy)
    _, losses = train_model.train(cfg, 'ValleAR', batches=batches, device=torch.device('cuda', 0), log=lambda *a: None)
    return calls, losses


def test_train_takes_the_packed_step_only_when_asked(monkeypatch):
    calls, losses = _train_three_steps(monkeypatch, packed=True)
    assert len(calls) == 3 and len(losses) == 3 and all(math.isfinite(x) for x in losses), (calls, losses)
    calls, losses = _train_three_steps(monkeypatch, packed=False)
    assert calls == [] and len(losses) == 3 and all(math.isfinite(x) for x in losses)
