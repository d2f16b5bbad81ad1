"""Packed AR training, the part that needs no GPU: the backward's work plan, the ABI, the refusals of the two new entry
points and of `ValleAR.training_step_packed`, and the fixture tests/golden/ar_train_packed.npz (the real reference's
training_step on each utterance alone) against the float64 oracle.

Refusals go through the entry points themselves with made-up aligned pointers, as tests/test_attn_forms_cpu.py does: a
refused call dereferences nothing."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import oracle_runners as R
from tests import train_replay as T
from tests.golden import cases as C
from tests.golden import gen_golden_train_packed as G

REPO = Path(__file__).resolve().parent.parent
PARENT_VERSION = 142
P, MIS = 0x10000, 0x10004            # "device pointers": never dereferenced (every call below is refused)


@pytest.fixture(scope='module')
def L():
    from valle2_amd import _lib
    return _lib.load_library()          # dlopen + every symbol bound: needs no device


# ---- the plan --------------------------------------------------------------------------------------------------------
LENGTHS = [1, 31, 33, 128, 129, 257, 300]


@pytest.mark.parametrize('chunk_keys', [256, 128])
@pytest.mark.parametrize('prefix', [False, True])
def test_bwd_plan_lists_every_chunk_once_heaviest_first(chunk_keys, prefix):
    from valle2_amd.engine import pack_bwd_plan
    x_lens = [0, 7, 33, 1, 128, 200, 130] if prefix else None
    items, max_chunks = pack_bwd_plan(LENGTHS, chunk_keys, x_lens)
    want = {(s, c) for s, n in enumerate(LENGTHS) for c in range(-(-n // chunk_keys))}
    assert len(items) == len(want) and set(items) == want                      # every (segment, chunk) exactly once
    assert max_chunks == -(-300 // chunk_keys)
    for s, n in enumerate(LENGTHS):                                            # chunks tile [0, len) without overlap
        spans = sorted((c * chunk_keys, min((c + 1) * chunk_keys, n)) for ss, c in items if ss == s)
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(a < b for a, b in spans)

    def weight(s, c):
        n, k0 = LENGTHS[s], c * chunk_keys
        first = k0 // 32 if prefix and k0 >= x_lens[s] else 0
        return min(chunk_keys, n - k0) * (-(-n // 32) - first)
    ws = [weight(s, c) for s, c in items]
    assert ws == sorted(ws, reverse=True)                                      # heaviest first
    assert items[0][0] == 6                                                    # (a chunk of the 300-row segment)


def test_bwd_plan_refuses_what_it_cannot_lay_out():
    from valle2_amd.engine import pack_bwd_plan
    for bad in ([], [4, 0, 3], [-1]):
        with pytest.raises(ValueError):
            pack_bwd_plan(bad)
    for ck in (0, 16, 48, 288):
        with pytest.raises(ValueError, match='chunk_keys'):
            pack_bwd_plan([40], ck)
    with pytest.raises(ValueError, match='text length'):
        pack_bwd_plan([40, 50], 256, [41, 0])
    with pytest.raises(ValueError, match='text length'):
        pack_bwd_plan([40, 50], 256, [4])


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_version_and_integration_line(L):
    from valle2_amd import _lib, kernels
    for name in ('vh_attn_rows_packed_lse', 'vh_attn_rows_bwd_packed', 'vh_attn_rows_bwd_packed_ws_bytes'):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None, name
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    declared = int(re.search(r'#define VH_VERSION (\d+)', header).group(1))
    assert L.vh_version() == declared > PARENT_VERSION
    for name in ('vh_attn_rows_packed_lse', 'vh_attn_rows_bwd_packed', 'vh_attn_rows_bwd_packed_ws_bytes'):
        assert re.search(rf'\b{name}\(', header), name
    text = (REPO / 'INTEGRATION.md').read_text()
    assert f'ABI {PARENT_VERSION + 1}' in text and 'vh_attn_rows_packed_lse' in text and 'vh_attn_rows_bwd_packed' in text
    assert callable(kernels.attn_rows_packed_lse) and callable(kernels.attn_rows_bwd_packed)
    assert L.vh_attn_rows_bwd_packed_ws_bytes(2, 1000, 1) == 0
    assert L.vh_attn_rows_bwd_packed_ws_bytes(2, 1000, 3) == 3 * 2 * 1000 * 64 * 4


# ---- refusals of the entry points ------------------------------------------------------------------------------------
def _fwd(L, **kw):
    a = dict(q=P, ldq=128, kc=P, vc=P, out=P, ldo=128, h=2, M=300, S_max=300, mode=1, seg_start=P, seg_len=P, seg_x_len=P,
             n_seg=2, blocks=P, n_blocks=3, lse2=P)
    a.update(kw)
    return L.vh_attn_rows_packed_lse(a['q'], a['ldq'], a['kc'], a['vc'], a['out'], a['ldo'], a['h'], a['M'], a['S_max'], a['mode'],
                                     a['seg_start'], a['seg_len'], a['seg_x_len'], a['n_seg'], a['blocks'], a['n_blocks'],
                                     a['lse2'], None)


def _bwd(L, **kw):
    a = dict(q=P, ldq=128, kc=P, vc=P, out=P, ldo=128, dout=P, lddo=128, lse2=P, dq=P, dk=P, dv=P, ldg=384, h=2, M=300,
             S_max=300, mode=1, seg_start=P, seg_len=P, seg_x_len=P, n_seg=2, items=P, n_items=3, chunk_keys=256, max_chunks=2,
             blocks=P, n_blocks=3, ws=P, ws_bytes=2 * 2 * 300 * 64 * 4)
    a.update(kw)
    return L.vh_attn_rows_bwd_packed(a['q'], a['ldq'], a['kc'], a['vc'], a['out'], a['ldo'], a['dout'], a['lddo'], a['lse2'],
                                     a['dq'], a['dk'], a['dv'], a['ldg'], a['h'], a['M'], a['S_max'], a['mode'], a['seg_start'],
                                     a['seg_len'], a['seg_x_len'], a['n_seg'], a['items'], a['n_items'], a['chunk_keys'],
                                     a['max_chunks'], a['blocks'], a['n_blocks'], a['ws'], a['ws_bytes'], None)


CODES = {'EINVAL': -1, 'EALIGN': -2}      # include/valle_hip.h


def _refused(L, rc, code, needle):
    msg = (L.vh_last_error() or b'').decode()
    assert rc == CODES[code], (rc, code, msg)
    assert needle in msg, msg


FWD_REFUSALS = [
    (dict(q=None), 'EINVAL', 'null pointer'), (dict(out=None), 'EINVAL', 'null pointer'), (dict(lse2=None), 'EINVAL', 'null pointer'),
    (dict(kc=None), 'EINVAL', 'null pointer'), (dict(seg_start=None), 'EINVAL', 'null pointer'),
    (dict(seg_len=None), 'EINVAL', 'null pointer'), (dict(blocks=None), 'EINVAL', 'null pointer'),
    (dict(seg_x_len=None), 'EINVAL', 'seg_x_len'),
    (dict(q=MIS), 'EALIGN', '16-byte'), (dict(out=MIS), 'EALIGN', '16-byte'), (dict(vc=MIS), 'EALIGN', '16-byte'),
    (dict(lse2=P + 2), 'EALIGN', 'lse2'),
    (dict(ldq=126), 'EINVAL', 'ldq'), (dict(ldq=64), 'EINVAL', 'ldq'), (dict(ldo=130), 'EINVAL', 'ldo'), (dict(ldo=124), 'EINVAL', 'ldo'),
    (dict(n_seg=0), 'EINVAL', 'n_seg'), (dict(n_blocks=0), 'EINVAL', 'n_blocks'),
    (dict(mode=2), 'EINVAL', 'mode=2'), (dict(mode=7), 'EINVAL', 'mode=7'), (dict(mode=-1), 'EINVAL', 'mode=-1'),
    (dict(M=0), 'EINVAL', 'bad dims'), (dict(S_max=299), 'EINVAL', 'bad dims'), (dict(h=0), 'EINVAL', 'bad dims'),
]
BWD_REFUSALS = [
    (dict(q=None), 'EINVAL', 'null pointer'), (dict(dout=None), 'EINVAL', 'null pointer'), (dict(lse2=None), 'EINVAL', 'null pointer'),
    (dict(dq=None), 'EINVAL', 'null pointer'), (dict(dk=None), 'EINVAL', 'null pointer'), (dict(dv=None), 'EINVAL', 'null pointer'),
    (dict(items=None), 'EINVAL', 'null pointer'), (dict(blocks=None), 'EINVAL', 'null pointer'),
    (dict(seg_start=None), 'EINVAL', 'null pointer'), (dict(seg_x_len=None), 'EINVAL', 'seg_x_len'),
    (dict(q=MIS), 'EALIGN', '16-byte'), (dict(dout=MIS), 'EALIGN', '16-byte'), (dict(dk=MIS), 'EALIGN', '16-byte'),
    (dict(ws=MIS), 'EALIGN', 'workspace'), (dict(ws=None), 'EALIGN', 'workspace'),
    (dict(ldq=126), 'EINVAL', 'leading'), (dict(lddo=64), 'EINVAL', 'leading'), (dict(ldg=382), 'EINVAL', 'leading'),
    (dict(ldo=120), 'EINVAL', 'leading'),
    (dict(n_seg=0), 'EINVAL', 'n_seg'), (dict(n_items=0), 'EINVAL', 'n_items'), (dict(n_blocks=0), 'EINVAL', 'n_blocks'),
    (dict(ws_bytes=2 * 2 * 300 * 64 * 4 - 1), 'EINVAL', 'workspace of'),
    (dict(max_chunks=3), 'EINVAL', 'workspace of'), (dict(max_chunks=0), 'EINVAL', 'max_chunks'),
    (dict(chunk_keys=0), 'EINVAL', 'chunk_keys'), (dict(chunk_keys=100), 'EINVAL', 'chunk_keys'), (dict(chunk_keys=288), 'EINVAL', 'chunk_keys'),
    (dict(mode=2), 'EINVAL', 'mode=2'), (dict(mode=5), 'EINVAL', 'mode=5'),
    (dict(M=0), 'EINVAL', 'bad dims'), (dict(S_max=10), 'EINVAL', 'bad dims'),
]


@pytest.mark.parametrize('kw,code,needle', FWD_REFUSALS, ids=[f'{i}-{"-".join(k)}' for i, (k, _, _) in enumerate(FWD_REFUSALS)])
def test_forward_entry_refuses_before_any_launch(L, kw, code, needle):
    _refused(L, _fwd(L, **kw), code, needle)


@pytest.mark.parametrize('kw,code,needle', BWD_REFUSALS, ids=[f'{i}-{"-".join(k)}' for i, (k, _, _) in enumerate(BWD_REFUSALS)])
def test_backward_entry_refuses_before_any_launch(L, kw, code, needle):
    _refused(L, _bwd(L, **kw), code, needle)


def test_full_mask_needs_no_text_lengths_but_everything_else(L):
    """mode = full with seg_x_len NULL passes the x_len check: the next fault in line is the one named."""
    _refused(L, _fwd(L, mode=0, seg_x_len=None, n_seg=0), 'EINVAL', 'n_seg')
    _refused(L, _bwd(L, mode=0, seg_x_len=None, n_seg=0), 'EINVAL', 'n_seg')


# ---- training_step_packed: refusals before any device work -----------------------------------------------------------
def _model(**kw):
    from valle2_amd import get_model_class
    cfg = C.cfg_of(dict(G.KW, **kw))
    return get_model_class('ValleAR')(cfg)


def _batch():
    return {k: v.clone() for k, v in G.train_packed_inputs()[2].items()}


def test_training_step_packed_refusals_need_no_device(monkeypatch):
    from valle2_amd import _lib, kernels
    monkeypatch.setattr(kernels, 'ids_to_device', lambda *a, **k: pytest.fail('device work before the refusal'))
    monkeypatch.setattr(_lib, 'to_device_async', lambda *a, **k: pytest.fail('device work before the refusal'))
    with pytest.raises(TypeError, match='LayerNorm'):
        _model(norm='AdaptiveLayerNorm').training_step_packed(_batch())
    with pytest.raises(ValueError, match='head width 32'):
        _model(n_heads=4).training_step_packed(_batch())
    with pytest.raises(_lib.VhError, match='HIP device'):
        with torch.enable_grad():
            _model().training_step_packed(_batch())
    b = _batch()
    b['codes_lens'][1] = 0
    with pytest.raises(ValueError, match='codes_lens entry 0 is outside 1 .. 230'):
        _model().training_step_packed(b)
    b = _batch()
    b['tokens_lens'][3] = 41
    with pytest.raises(ValueError, match='tokens_lens entry 41 is outside 1 .. 40'):
        _model().training_step_packed(b)
    b = _batch()
    b['codes_lens'][0] = 231
    with pytest.raises(ValueError, match='codes_lens entry 231'):
        with torch.no_grad():
            _model().training_step_packed(b)


def test_signatures_are_unchanged():
    from valle2_amd import get_model_class, train_model
    ar = get_model_class('ValleAR')
    assert str(inspect.signature(ar.training_step)) == '(self, batch, **kwargs)'
    assert str(inspect.signature(ar.training_step_packed)) == '(self, batch, **kwargs)'
    assert str(inspect.signature(train_model.train)) == "(hparams_fp: 'Path', model_name: 'str', batches=None, device=None, log=<built-in function print>)"


# ---- the fixture against the float64 oracle --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle64():
    """Per utterance alone (B = 1, nothing padded): (loss, {name: gradient}) of the float64 oracle."""
    kw, sd, batch = G.train_packed_inputs()
    cfg = C.cfg_of(kw)
    out = []
    for b in range(len(G.TEXT_LENS)):
        loss, params = R.oracle_training_loss(sd, cfg, G.utterance_batch(batch, b), 'ValleAR')
        out.append((loss, {n: params[n].grad for n in G.param_names(sd)}))
    return out


def test_oracle_reproduces_the_reference_per_utterance(oracle64):
    gold = R.load_golden('ar_train_packed')
    _, sd, _ = G.train_packed_inputs()
    names = G.param_names(sd)
    for b, (loss, grads) in enumerate(oracle64):
        torch.testing.assert_close(loss.float(), torch.as_tensor(gold[f'loss_{b}']), rtol=T.LOSS_TOL[0], atol=T.LOSS_TOL[1])
        samples, off = torch.as_tensor(gold[f'grad_samples_{b}']).double(), 0
        for i, n in enumerate(names):
            idx = G.sample_index(grads[n].numel())
            ref = samples[off:off + idx.numel()]
            off += idx.numel()
            got = grads[n].reshape(-1)[idx]
            # the reference computed in float32: its own error against float64 is what GRAD_TOL allows the device
            assert (got - ref).norm() <= T.GRAD_TOL * max(float(ref.norm()), 1e-12), (b, n)
            norm = float(gold[f'grad_norms_{b}'][i])
            assert abs(float(grads[n].norm()) - norm) <= T.GRAD_TOL * max(norm, 1e-12), (b, n)
        assert off == samples.numel()


def test_token_weighted_losses_are_the_packed_loss(oracle64):
    """The packed loss = mean CE over the sum(codes_lens) real positions = the per-utterance means weighted by their
    position counts: restated here with the oracle's logits of each utterance alone, all positions in one mean."""
    from oracle import valle_oracle as O
    gold = R.load_golden('ar_train_packed')
    kw, sd, batch = G.train_packed_inputs()
    cfg = C.cfg_of(kw)
    sd64 = {k: v.double() for k, v in sd.items()}
    logits, targets = [], []
    for b in range(len(G.TEXT_LENS)):
        ub = G.utterance_batch(batch, b)
        logits.append(O.ar_logits(sd64, cfg, ub)[0].T)               # (ty, V)
        targets.append(ub['target'][0])
    packed = torch.nn.functional.cross_entropy(torch.cat(logits), torch.cat(targets))
    w = torch.tensor(G.AUDIO_LENS, dtype=torch.float64)
    weighted64 = sum(wi * l for wi, (l, _) in zip(w, oracle64)) / w.sum()
    torch.testing.assert_close(weighted64, packed, rtol=1e-12, atol=0)
    weighted_ref = sum(float(wi) * float(gold[f'loss_{b}']) for b, wi in enumerate(w)) / float(w.sum())
    assert abs(weighted_ref - float(packed)) <= T.LOSS_TOL[0] * abs(float(packed)) + T.LOSS_TOL[1]
    assert np.isfinite(weighted_ref)
