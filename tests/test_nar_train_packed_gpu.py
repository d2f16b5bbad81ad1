"""Packed NAR training on the GPU: the packed model input against `kernels.embed_sum_pe` on each utterance alone (bit for
bit) and its backward against a float64 scatter-add; `ValleNAR.training_step_packed` against the float64 oracle on each
utterance alone, combined with the weights (frames_b - prefix_b) / sum; against `training_step` on equal lengths; and `train()`.

The real reference's NAR training_step raises (D4 / D5), so there is no golden file: the yardstick is the float64 oracle.
Bounds are the suite's own: train_replay.LOSS_TOL and GRAD_TOL for the model, and for the backward's sums — which promise no
order — oracle_runners.check_sum with the error of the fp32 emulation of the same sums, computed here on the CPU."""
import functools
import math

import pytest
import torch

from tests import nar_train_packed_inputs as N
from tests import oracle_runners as R
from tests import train_replay as T
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POISON = 12345.0
PAD_ROWS = 64                          # rows behind M, and before and after every gradient table, that must stay poisoned
Q, VOCAB_T, VOCAB_A = 8, 50, 40
ORDERS = {'longest_first': [4, 3, 2, 0, 1], 'shuffled': [2, 4, 0, 3, 1]}
P_DROP = 0.1


def sinusoid(d, rows):
    from oracle import valle_oracle as O
    return O.positional_table(d, rows).reshape(rows, d).contiguous()


@functools.lru_cache(maxsize=None)
def kernel_inputs(order, d):
    """Seeded tables, ids and an upstream gradient for the five utterances of the fixture in `order` (CPU tensors, shared):
    code table 0 is read with 7 ids only, and the 100-frame utterance holds a run of 40 equal ids in every codebook — frames
    20..59, across its prefix boundary at 33 and across three 16-row boundaries of the packed stream."""
    g = torch.Generator().manual_seed(8100 + d)
    idx = ORDERS[order]
    txs, tys = [N.TEXT_LENS[i] for i in idx], [N.FRAME_LENS[i] for i in idx]
    ps = [N.PREFIXES[i] for i in idx]
    text_table = torch.randn(VOCAB_T, d, generator=g)
    code_tables = [torch.randn(VOCAB_A, d, generator=g) for _ in range(Q)]
    tokens = torch.full((5, max(txs)), VOCAB_T - 1, dtype=torch.int64)
    codes = torch.full((5, max(tys), Q), VOCAB_A - 1, dtype=torch.int64)          # padding: a valid id the kernels must not read
    for b, (tx, ty) in enumerate(zip(txs, tys)):
        tokens[b, :tx] = torch.randint(0, VOCAB_T, (tx,), generator=g)
        codes[b, :ty] = torch.randint(0, VOCAB_A, (ty, Q), generator=g)
        codes[b, :ty, 0] = torch.randint(0, 7, (ty,), generator=g)
        if ty == 100:
            codes[b, 20:60] = 5
    M = sum(txs) + sum(tys)
    dout = torch.randn(M, d, generator=g)
    starts = [sum(txs[:i]) + sum(tys[:i]) for i in range(5)]
    assert M == N.ROWS and all(s % 32 for s in starts[1:])
    run = starts[tys.index(100)] + txs[tys.index(100)] + 20
    assert len({r // 16 for r in range(run, run + 40)}) >= 3
    return dict(txs=txs, tys=tys, ps=ps, starts=starts, M=M, text_table=text_table, code_tables=code_tables, tokens=tokens,
                codes=codes, dout=dout)


def device_layout(k):
    from valle2_amd.engine import NarTrainLayout
    return NarTrainLayout(k['txs'], k['tys'], k['ps'], k['codes'].shape[1], DEV)


def specs(drop):
    from valle2_amd import dropout
    if not drop:
        return None, None
    return dropout.spec(0x1234567, dropout.site(dropout.PE_TEXT), P_DROP), dropout.spec(0x1234567, dropout.site(dropout.PE_AUDIO), 0.25)


# ---- forward ---------------------------------------------------------------------------------------------------------
def _forward_case(order, drop, n_rest, d):
    from valle2_amd import kernels
    k = kernel_inputs(order, d)
    lay = device_layout(k)
    M = k['M']
    tt, cts = k['text_table'].to(DEV), [t.to(DEV) for t in k['code_tables']]
    tokens, codes = k['tokens'].to(DEV), k['codes'].to(DEV)
    pe_t, pe_a = sinusoid(d, 64).to(DEV), sinusoid(d, 512).to(DEV)
    dr_t, dr_a = specs(drop)
    buf = torch.full((M + PAD_ROWS, d), POISON, device=DEV)
    kernels.embed_nar_packed(tokens, codes, tt, cts, n_rest, pe_t, pe_a, lay, buf[:M], dr_t, dr_a)
    assert bool((buf[M:] == POISON).all()), 'rows beyond M were written'
    assert not bool((buf[:M] == POISON).any()), 'a row in [0, M) was not written'
    # each utterance alone through vh_embed_sum_pe, at the same rows of a buffer of its own (the field's row is the row of out)
    want = torch.full((M + PAD_ROWS, d), POISON, device=DEV)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)                # noqa: E731
    for b, (s0, tx, ty, p) in enumerate(zip(k['starts'], k['txs'], k['tys'], k['ps'])):
        kernels.embed_sum_pe(tokens[b:b + 1, :tx], [tt], pe_t, 0, want[:M], lens=i32(tx), row_t0=i32(s0), max_pos=tx, drop=dr_t)
        if p:
            kernels.embed_sum_pe(codes[b:b + 1, :p], cts, pe_a, 0, want[:M], lens=i32(p), row_t0=i32(s0 + tx), max_pos=p, drop=dr_a)
        kernels.embed_sum_pe(codes[b:b + 1, p:ty], cts[:n_rest], pe_a, 0, want[:M], lens=i32(ty - p), row_pos0=i32(p),
                             row_t0=i32(s0 + tx + p), max_pos=ty, drop=dr_a)
        assert torch.equal(buf[s0:s0 + tx + ty], want[s0:s0 + tx + ty]), f'utterance {b} ({tx} text rows, {ty} frames, prefix {p})'
    assert torch.equal(buf, want)
    # and float64, so that the two kernels cannot be wrong together
    ref = torch.zeros(M, d, dtype=torch.float64)
    for b, (s0, tx, ty, p) in enumerate(zip(k['starts'], k['txs'], k['tys'], k['ps'])):
        ref[s0:s0 + tx] = k['text_table'].double()[k['tokens'][b, :tx]] + pe_t.cpu().double()[:tx]
        for t in range(ty):
            n = Q if t < p else n_rest
            ref[s0 + tx + t] = sum(k['code_tables'][j].double()[k['codes'][b, t, j]] for j in range(n)) + pe_a.cpu().double()[t]
    got = buf[:M].cpu().double()
    if drop:
        kept = got != 0
        text_row = torch.zeros(M, dtype=torch.bool)
        for s0, tx in zip(k['starts'], k['txs']):
            text_row[s0:s0 + tx] = True
        scale = torch.where(text_row, 1 / (1 - P_DROP), 1 / (1 - 0.25))[:, None]
        assert 0.05 < 1 - kept[text_row].double().mean() < 0.16 and 0.2 < 1 - kept[~text_row].double().mean() < 0.3
        ref = torch.where(kept, ref * scale, torch.zeros_like(ref))
    R.check_close('packed NAR input', got, ref, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize('n_rest', [1, 4, 7])
@pytest.mark.parametrize('drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('order', list(ORDERS))
def test_packed_input_is_embed_sum_pe_of_each_utterance_alone(order, drop, n_rest):
    _forward_case(order, drop, n_rest, 128)


def test_packed_input_wider_than_one_column_pass():
    """d = 1280: a lane takes two float4 of a row, the second pass only partly filled."""
    _forward_case('shuffled', True, 4, 1280)


# ---- backward --------------------------------------------------------------------------------------------------------
def _contributions(k, n_rest, skip=()):
    """Per table (text table first): the (table row, packed row) of every addition, in packed-row order.  skip: (b, t, j)
    of code ids, (b, i, 'text') of text ids, that are out of range and add nothing."""
    out = [([], []) for _ in range(1 + Q)]
    for b, (s0, tx, ty, p) in enumerate(zip(k['starts'], k['txs'], k['tys'], k['ps'])):
        for i in range(tx):
            if (b, i, 'text') not in skip:
                out[0][0].append(int(k['tokens'][b, i]))
                out[0][1].append(s0 + i)
        for t in range(ty):
            for j in range(Q if t < p else n_rest):
                if (b, t, j) not in skip:
                    out[1 + j][0].append(int(k['codes'][b, t, j]))
                    out[1 + j][1].append(s0 + tx + t)
    return out


def _scatter(contrib, vocab, dd, dtype):
    ids, rows = torch.tensor(contrib[0], dtype=torch.int64), torch.tensor(contrib[1], dtype=torch.int64)
    return torch.zeros(vocab, dd.shape[1], dtype=dtype).index_add_(0, ids, dd.to(dtype)[rows])     # (walks the index in order)


def _backward_case(order, drop, n_rest, d, bad=None):
    from valle2_amd import _lib, dropout, kernels
    k = kernel_inputs(order, d)
    lay = device_layout(k)
    M = k['M']
    tokens, codes = k['tokens'].clone(), k['codes'].clone()
    skip = set()
    if bad:
        b = k['tys'].index(10)
        codes[b, 5, 1], codes[b, 1, 0], tokens[b, 2] = VOCAB_A, -1, VOCAB_T + 3          # frame 1 is prefix, frame 5 is not
        skip = {(b, 5, 1), (b, 1, 0), (b, 2, 'text')}
    dr_t, dr_a = specs(drop)
    vocabs = [VOCAB_T] + [VOCAB_A] * Q
    bufs = [torch.full((v + 2 * PAD_ROWS, d), POISON, device=DEV) for v in vocabs]
    grads = [buf[PAD_ROWS:PAD_ROWS + v] for buf, v in zip(bufs, vocabs)]
    for g in grads:
        g.zero_()
    dout = k['dout'].to(DEV)
    _lib.raise_device_errors(DEV)                                                         # nothing pending
    kernels.embed_nar_packed_bwd(tokens.to(DEV), codes.to(DEV), dout, grads[0], grads[1:], VOCAB_T, [VOCAB_A] * Q, n_rest, 64, 512,
                                 lay, dr_t, dr_a)
    if bad:
        with pytest.raises(IndexError):
            _lib.raise_device_errors(DEV)
    _lib.raise_device_errors(DEV)                                                         # no flag, or cleared by the raise
    # the gradient the tables see: dout under the regenerated fields (exported by vh_dropout_mask), in float64
    dd64, dd32 = k['dout'].double(), k['dout'].clone()
    if drop:
        text_row = torch.zeros(M, dtype=torch.bool)
        for s0, tx in zip(k['starts'], k['txs']):
            text_row[s0:s0 + tx] = True
        keep_t = dropout.mask(dr_t, M, d, DEV).cpu() != 0
        keep_a = dropout.mask(dr_a, M, d, DEV).cpu() != 0
        keep = torch.where(text_row[:, None], keep_t, keep_a)
        s64 = torch.where(text_row, 1 / (1 - P_DROP), 1 / (1 - 0.25))[:, None]
        dd64 = torch.where(keep, dd64 * s64, torch.zeros_like(dd64))
        dd32 = torch.where(keep, dd32 * s64.float(), torch.zeros_like(dd32))
    contrib = _contributions(dict(k, tokens=tokens, codes=codes), n_rest, skip)
    prefix_only = _contributions(dict(k, tys=k['ps'], tokens=tokens, codes=codes), Q, skip)       # the prefix frames alone
    for j, (buf, g, v) in enumerate(zip(bufs, grads, vocabs)):
        name = 'text table' if j == 0 else f'code table {j - 1}'
        assert bool((buf[:PAD_ROWS] == POISON).all()) and bool((buf[PAD_ROWS + v:] == POISON).all()), f'{name}: guard rows written'
        ref = _scatter(contrib[j], v, dd64, torch.float64)
        measured = R.worst(_scatter(contrib[j], v, dd32, torch.float32), ref)
        err = R.check_sum(name, g, ref, measured)
        print(f'{order} drop={drop} n_rest={n_rest} d={d} {name}: {len(contrib[j][0])} additions, worst {err:.3e}, fp32 emulation {measured:.3e}')
        unnamed = torch.ones(v, dtype=torch.bool)
        unnamed[torch.tensor(contrib[j][0], dtype=torch.int64)] = False
        assert bool((g.cpu()[unnamed] == 0).all()), f'{name}: a row no id names is not exactly 0'
        if j == 1:
            assert int((~unnamed).sum()) <= 8                                            # heavily shared sums
        if j - 1 >= n_rest:                                                              # prefix frames only
            assert contrib[j] == prefix_only[j]
            assert len(contrib[j][0]) == sum(k['ps']) - sum(1 for s in skip if s[2] == j - 1)


@pytest.mark.parametrize('n_rest', [1, 4, 7])
@pytest.mark.parametrize('drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('order', list(ORDERS))
def test_packed_input_backward_against_float64(order, drop, n_rest):
    _backward_case(order, drop, n_rest, 128)


def test_packed_input_backward_wider_than_one_column_pass():
    _backward_case('longest_first', True, 4, 1280)


def test_packed_input_backward_skips_and_flags_an_id_out_of_range():
    _backward_case('shuffled', False, 4, 128, bad=True)


def test_packed_input_forward_reads_row_0_for_an_id_out_of_range():
    from valle2_amd import _lib, kernels
    k = kernel_inputs('shuffled', 128)
    lay = device_layout(k)
    tt, cts = k['text_table'].to(DEV), [t.to(DEV) for t in k['code_tables']]
    pe_t, pe_a = sinusoid(128, 64).to(DEV), sinusoid(128, 512).to(DEV)
    good = torch.empty(k['M'], 128, device=DEV)
    kernels.embed_nar_packed(k['tokens'].to(DEV), k['codes'].to(DEV), tt, cts, 4, pe_t, pe_a, lay, good)
    _lib.raise_device_errors(DEV)
    b = k['tys'].index(10)
    codes, zeroed = k['codes'].clone(), k['codes'].clone()
    codes[b, 5, 1], zeroed[b, 5, 1] = VOCAB_A, 0
    got, want = torch.empty_like(good), torch.empty_like(good)
    kernels.embed_nar_packed(k['tokens'].to(DEV), codes.to(DEV), tt, cts, 4, pe_t, pe_a, lay, got)
    with pytest.raises(IndexError):
        _lib.raise_device_errors(DEV)
    kernels.embed_nar_packed(k['tokens'].to(DEV), zeroed.to(DEV), tt, cts, 4, pe_t, pe_a, lay, want)
    _lib.raise_device_errors(DEV)
    row = k['starts'][b] + k['txs'][b] + 5
    assert torch.equal(got, want) and not torch.equal(got[row], good[row])
    assert torch.equal(torch.cat([got[:row], got[row + 1:]]), torch.cat([good[:row], good[row + 1:]]))


# ---- the model -------------------------------------------------------------------------------------------------------
def _device_model(kw, sd, pe_p=None):
    from valle2_amd import get_model_class
    model = get_model_class('ValleNAR')(C.cfg_of(kw))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    if pe_p is not None:
        model.tokens_position_emb.dropout.p = pe_p
        model.audio_position_emb.dropout.p = pe_p
    return model


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


def _combine(per, names):
    """Token-weighted loss and gradients of per-utterance (loss, {name: grad | None}); a parameter no utterance reaches: None."""
    w = N.weights()
    loss = sum(float(wi) * float(l) for wi, (l, _) in zip(w, per))
    grads = {}
    for n in names:
        parts = [wi * g[n] for wi, (_, g) in zip(w, per) if g[n] is not None]
        grads[n] = sum(parts) if parts else None
    return loss, grads


def _check_grads(model, want, what):
    """Every parameter's gradient within GRAD_TOL of the norm of `want[name]` (float64, full gradients); a parameter the
    stage does not reach (the other stages' embeddings and heads) has no gradient or an all-zero one."""
    checked = 0
    for n, p in model.named_parameters():
        if want[n] is None:
            assert p.grad is None or not bool(p.grad.any()), f'{what}: {n} is not part of this stage but has a gradient'
            continue
        assert p.grad is not None, f'no gradient reached {n}'
        err = float((p.grad.detach().cpu().double() - want[n]).norm()) / max(float(want[n].norm()), 1e-12)
        assert err < T.GRAD_TOL, f'{what}: {n}: relative gradient error {err:.2e}'
        checked += 1
    assert checked >= 2 + 8 + 2 + 14 * 2                  # text table, code tables, stage embedding + head, the stack


@functools.lru_cache(maxsize=None)
def oracle64(stage):
    kw, sd, batch = N.inputs()
    per = []
    for b in range(len(N.TEXT_LENS)):
        loss, params = R.oracle_training_loss(sd, C.cfg_of(kw), N.utterance_batch(batch, b), 'ValleNAR', stage=stage)
        per.append((loss, {n: params[n].grad for n in N.param_names(sd)}))
    return _combine(per, N.param_names(sd))


@pytest.mark.parametrize('stage', N.STAGES)
def test_training_step_packed_against_the_oracle_per_utterance(stage):
    kw, sd, batch = N.inputs()
    want, want_grads = oracle64(stage)
    model = _device_model(kw, sd, pe_p=0.0)
    loss = model.training_step_packed(_clone(batch), stage=stage)
    loss.backward()
    print(f'stage {stage}: packed loss {float(loss.detach()):.8f}, float64 oracle per utterance token-weighted {want:.8f}')
    assert abs(float(loss) - want) <= T.LOSS_TOL[0] * abs(want) + T.LOSS_TOL[1]
    _check_grads(model, want_grads, f'float64 oracle, stage {stage}')
    with torch.no_grad():                                # the same value without a graph
        again = model.training_step_packed(_clone(batch), stage=stage)
    assert again.grad_fn is None and abs(float(again) - float(loss)) <= T.LOSS_TOL[0] * abs(want) + T.LOSS_TOL[1]


def test_training_step_packed_dropout_fields_replayed_by_the_oracle():
    from oracle import valle_oracle as O
    from valle2_amd import dropout
    kw, sd, batch = N.inputs()
    kw = dict(kw, dropout=0.1)
    cfg = C.cfg_of(kw)
    stage = 3
    model = _device_model(kw, sd)
    dropout.RECORD = []
    try:
        torch.manual_seed(11)
        loss = model.training_step_packed(_clone(batch), stage=stage)
        loss.backward()
        recs = dropout.RECORD
    finally:
        dropout.RECORD = None
    M = N.ROWS
    assert sorted(r['name'] for r in recs) == sorted(['tokens_position_emb.dropout', 'audio_position_emb.dropout'] +
                                                     [f'layer{i}.{s}' for i in range(2) for s in ('dropout1', 'ffn.dropout', 'dropout2')])
    assert all(r['rows'] == M for r in recs)
    fields = {r['name']: dropout.mask(dropout.spec(r['seed'], r['site'], r['p']), r['rows'], r['cols'], DEV).cpu() != 0 for r in recs}
    names = N.param_names(sd)
    per, s0 = [], 0
    for b, (tl, fl) in enumerate(zip(N.TEXT_LENS, N.FRAME_LENS)):       # the fields sliced per utterance: keyed on the packed row
        masks = {}
        for name, f in fields.items():
            rows = slice(s0, s0 + tl) if name.startswith('tokens_') else slice(s0 + tl, s0 + tl + fl) if name.startswith('audio_') \
                else slice(s0, s0 + tl + fl)
            masks[name] = f[rows][None]
        params = {k: v.double().clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
        with torch.enable_grad():
            lb = O.nar_training_loss(params, cfg, N.utterance_batch(batch, b), stage, O.Dropout(cfg.dropout, masks=masks))
            lb.backward()
        per.append((lb.detach(), {n: params[n].grad for n in names}))
        s0 += tl + fl
    want_loss, want = _combine(per, names)
    print(f'packed loss under dropout {float(loss.detach()):.8f}, float64 oracle with the exported fields {want_loss:.8f}')
    assert abs(float(loss) - want_loss) <= T.LOSS_TOL[0] * abs(want_loss) + T.LOSS_TOL[1]
    _check_grads(model, want, 'oracle with the exported fields')


def test_equal_lengths_give_the_loss_of_training_step():
    from valle2_amd import synth
    kw, sd, _ = N.inputs()
    batch = synth.synth_nar_batch(C.cfg_of(kw), 3, n_tokens=6, n_frames=15, seed=77)
    model = _device_model(kw, sd, pe_p=0.0)
    padded = model.training_step(_clone(batch), stage=2)
    packed = model.training_step_packed(_clone(batch), stage=2)
    assert abs(float(packed) - float(padded)) <= T.LOSS_TOL[0] * abs(float(padded)) + T.LOSS_TOL[1], (float(packed), float(padded))


# training_step on the fixture's batch (train mode, PositionalEncoding dropout set to 0, stage 3), recorded on the commit before
# the packed NAR path existed.  The gradient is pinned bit for bit: the sum of layer 0's QKV weight gradient (float64 sum of the
# float32 elements) as hex.  The loss is held to 4 ulp, as tests/test_train_packed_gpu.py holds the AR step's and for its
# reason: vh_cross_entropy adds the rows' terms up in an order that is not fixed — two runs of that commit returned
# 0x1.c16e8ap+2 and 0x1.c16e82p+2, and the same gradient sum.
PARENT_TRAINING_STEP = {'loss': '0x1.c16e8a0000000p+2', 'qkv_grad_sum': '0x1.64291ceda51c0p-6'}


def test_training_step_keeps_its_bits():
    kw, sd, batch = N.inputs()
    model = _device_model(kw, sd, pe_p=0.0)
    loss = model.training_step(_clone(batch), stage=3)
    loss.backward()
    qkv = dict(model.named_parameters())['transformer.layers.0.self_attn.qkv.weight'].grad
    got = {'loss': float(loss.detach()).hex(), 'qkv_grad_sum': float(qkv.double().sum()).hex()}
    print(got)
    assert got['qkv_grad_sum'] == PARENT_TRAINING_STEP['qkv_grad_sum']
    parent_loss = float.fromhex(PARENT_TRAINING_STEP['loss'])
    assert abs(float(loss.detach()) - parent_loss) <= 4 * 2.0 ** -23 * parent_loss


def _train_three_steps(monkeypatch, packed):
    from valle2_amd import get_model_class, train_model
    from valle2_amd.config import ConfigValle
    if packed:
        monkeypatch.setenv('VALLE2_TRAIN_PACKED', '1')
    else:
        monkeypatch.delenv('VALLE2_TRAIN_PACKED', raising=False)
    cfg = ConfigValle(**N.KW, max_steps=3, batch_size=3, grad_accum=1, log_every_n_steps=1000, seed=3)
    batches = []
    for i in range(3):                                   # ragged: three utterances of the fixture's batch, rotated
        _, _, batch = N.inputs()
        pick = [(i + j) % 4 for j in range(3)]           # (the 500-frame utterance stays out: three quick steps)
        batches.append({k: v[pick].clone() for k, v in batch.items()})
    cls = get_model_class('ValleNAR')
    calls, orig = [], cls.training_step_packed

    def spy(self, batch, **kw):
        calls.append(1)
        return orig(self, batch, **kw)
    monkeypatch.setattr(cls, 'training_step_packed', spy)
    _, losses = train_model.train(cfg, 'ValleNAR', batches=batches, device=torch.device('cuda', 0), log=lambda *a: None)
    return calls, losses


def test_train_takes_the_packed_step_only_when_asked(monkeypatch):
    calls, losses = _train_three_steps(monkeypatch, packed=True)
    assert len(calls) == 3 and len(losses) == 3 and all(math.isfinite(x) for x in losses), (calls, losses)
    calls, losses = _train_three_steps(monkeypatch, packed=False)
    assert calls == [] and len(losses) == 3 and all(math.isfinite(x) for x in losses)
