"""Packed NAR training, the part that needs no GPU: the layout's prefix and weight arithmetic, the ABI, the refusals of the
two new entry points and of `ValleNAR.training_step_packed`, and the `VALLE2_TRAIN_PACKED` dispatch of `train()`.

Refusals go through the entry points themselves with made-up aligned pointers, as tests/test_train_packed_cpu.py does: a
refused call dereferences nothing."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from tests import nar_train_packed_inputs as N
from tests.golden import cases as C

REPO = Path(__file__).resolve().parent.parent
PARENT_VERSION = 143
P, MIS = 0x10000, 0x10004            # "device pointers": never dereferenced (every call below is refused)
NAMES = ('vh_embed_nar_packed', 'vh_embed_nar_packed_bwd')


@pytest.fixture(scope='module')
def L():
    from valle2_amd import _lib
    return _lib.load_library()          # dlopen + every symbol bound: needs no device


# ---- the layout ------------------------------------------------------------------------------------------------------
def test_plan_prefixes_targets_and_weights_follow_the_formulas():
    from valle2_amd import get_model_class
    from valle2_amd.engine import nar_train_plan
    model = get_model_class('ValleNAR')(C.cfg_of(N.KW))
    qf = model.config.quantization_factor
    assert 3 * qf == 150
    prefixes = [model.prefix_len_of(f) for f in N.FRAME_LENS]
    assert prefixes == [min(f // 3, 3 * qf) for f in N.FRAME_LENS] == N.PREFIXES
    assert model.prefix_len_of(449) == 149 and model.prefix_len_of(450) == 150 and model.prefix_len_of(453) == 150
    starts, M, target_rows, target_frames, weights = nar_train_plan(N.TEXT_LENS, N.FRAME_LENS, prefixes)
    assert starts == N.STARTS and M == N.ROWS == sum(N.TEXT_LENS) + sum(N.FRAME_LENS)
    assert all(s % 32 for s in starts[1:])
    want_rows, want_frames = [], []
    for b, (s0, tx, ty, p) in enumerate(zip(starts, N.TEXT_LENS, N.FRAME_LENS, prefixes)):
        for t in range(p, ty):
            want_rows.append(s0 + tx + t)
            want_frames.append((b, t))
    assert target_rows == want_rows and target_frames == want_frames
    total = sum(f - p for f, p in zip(N.FRAME_LENS, prefixes))
    assert len(target_rows) == total == 2 + 2 + 7 + 67 + 350
    assert weights == [(f - p) / total for f, p in zip(N.FRAME_LENS, prefixes)]
    assert weights == pytest.approx(N.weights().tolist(), abs=0, rel=1e-15) and abs(sum(weights) - 1) < 1e-15


def test_plan_refuses_what_it_cannot_lay_out():
    from valle2_amd.engine import nar_train_plan
    for bad in (([], [], []), ([3], [4, 5], [1, 1]), ([3, 0], [4, 5], [1, 1]), ([3, 2], [4, 0], [1, 0])):
        with pytest.raises(ValueError):
            nar_train_plan(*bad)
    for prefixes in ([4, 1], [-1, 1], [1, 5]):
        with pytest.raises(ValueError, match='prefix'):
            nar_train_plan([3, 2], [4, 5], prefixes)


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_version_and_documents(L):
    from valle2_amd import _lib, autograd, kernels
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    declared = int(re.search(r'#define VH_VERSION (\d+)', header).group(1))
    assert L.vh_version() == declared > PARENT_VERSION
    text = (REPO / 'INTEGRATION.md').read_text()
    assert f'ABI {PARENT_VERSION + 1}' in text
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None, name
        assert re.search(rf'\b{name}\(', header), name
        assert name in text, name
    assert callable(kernels.embed_nar_packed) and callable(kernels.embed_nar_packed_bwd)
    assert issubclass(autograd.EmbedNarPackedFn, torch.autograd.Function)
    design = (REPO / 'DESIGN.md').read_text()
    assert 'NAR training stays padded' not in design and 'training_step_packed' in design


# ---- refusals of the entry points ------------------------------------------------------------------------------------
def _tables(n=8, null=None, rows=1024):
    arr = (ctypes.c_void_p * n)(*[None if j == null else P for j in range(n)])
    return arr, (ctypes.c_int32 * n)(*[rows] * n)


def _drop(p):
    from valle2_amd import _lib
    s = _lib.VhDropoutSpec()
    s.seed, s.site, s.p = 1, 2, p
    return ctypes.byref(s)


BASE = dict(tokens=P, tokens_bs=40, codes=P, codes_bs=4000, codes_ts=8, codes_js=1, text_table=P, text_vocab=512, tables=None,
            n_full=8, n_rest=3, pe_text=P, pe_text_rows=5000, pe_audio=P, pe_audio_rows=5000, seg_start=P, x_len=P, a_len=P,
            prefix=P, n_seg=5, max_x_len=40, max_a_len=500, rows=P, M=682, d=128, drop_text=None, drop_audio=None)


def _fwd(L, **kw):
    a = dict(BASE, **kw)
    arr, vocab = a['tables'] or _tables(max(1, min(a['n_full'], 32)))
    return L.vh_embed_nar_packed(a['tokens'], a['tokens_bs'], a['codes'], a['codes_bs'], a['codes_ts'], a['codes_js'], a['text_table'],
                                 a['text_vocab'], arr, vocab, a['n_full'], a['n_rest'], a['pe_text'], a['pe_text_rows'], a['pe_audio'],
                                 a['pe_audio_rows'], a['seg_start'], a['x_len'], a['a_len'], a['prefix'], a['n_seg'], a['max_x_len'],
                                 a['max_a_len'], a['rows'], a['M'], a['d'], None, a['drop_text'], a['drop_audio'], None)


def _bwd(L, **kw):
    a = dict(BASE, **kw)
    arr, vocab = a['tables'] or _tables(max(1, min(a['n_full'], 32)))
    return L.vh_embed_nar_packed_bwd(a['tokens'], a['tokens_bs'], a['codes'], a['codes_bs'], a['codes_ts'], a['codes_js'], a['rows'],
                                     a['text_table'], a['text_vocab'], arr, vocab, a['n_full'], a['n_rest'], a['pe_text_rows'],
                                     a['pe_audio_rows'], a['seg_start'], a['x_len'], a['a_len'], a['prefix'], a['n_seg'],
                                     a['max_x_len'], a['max_a_len'], a['M'], a['d'], None, a['drop_text'], a['drop_audio'], None)


CODES = {'EINVAL': -1, 'EALIGN': -2}      # include/valle_hip.h

SHARED_REFUSALS = [          # one argument wrong at a time; the message names it
    (dict(tokens=None), 'EINVAL', 'null pointer: tokens'), (dict(codes=None), 'EINVAL', 'null pointer: codes'),
    (dict(seg_start=None), 'EINVAL', 'null pointer: seg_start'), (dict(x_len=None), 'EINVAL', 'null pointer: x_len'),
    (dict(a_len=None), 'EINVAL', 'null pointer: a_len'), (dict(prefix=None), 'EINVAL', 'null pointer: prefix'),
    (dict(n_rest=0), 'EINVAL', 'n_rest=0'), (dict(n_rest=9), 'EINVAL', 'n_rest=9'), (dict(n_full=0), 'EINVAL', 'n_full=0'),
    (dict(n_full=33, n_rest=1), 'EINVAL', 'n_full=33'),
    (dict(M=0), 'EINVAL', 'M=0'), (dict(M=-4), 'EINVAL', 'M=-4'), (dict(n_seg=0), 'EINVAL', 'n_seg=0'),
    (dict(pe_text_rows=39), 'EINVAL', 'pe_text_rows=39'), (dict(pe_audio_rows=499), 'EINVAL', 'pe_audio_rows=499'),
    (dict(d=0), 'EINVAL', 'd=0'),
    (dict(rows=MIS), 'EALIGN', '16-byte'), (dict(tables=_tables(8, rows=0)), 'EINVAL', 'code table 0 has 0 rows'),
]
FWD_REFUSALS = SHARED_REFUSALS + [
    (dict(rows=None), 'EINVAL', 'null pointer: out'), (dict(text_table=None), 'EINVAL', 'null pointer: text_table'),
    (dict(pe_text=None), 'EINVAL', 'null pointer: pe_text'), (dict(pe_audio=None), 'EINVAL', 'null pointer: pe_audio'),
    (dict(tables=_tables(8, null=5)), 'EINVAL', 'null pointer: code_tables[5]'),
    (dict(pe_audio=MIS), 'EALIGN', '16-byte'),
]
BWD_REFUSALS = SHARED_REFUSALS + [(dict(rows=None), 'EINVAL', 'null pointer: dout')]


def _refused(L, rc, code, needle, name):
    msg = (L.vh_last_error() or b'').decode()
    assert rc == CODES[code], (rc, code, msg)
    assert needle in msg and msg.startswith(name + ':'), msg


@pytest.mark.parametrize('kw,code,needle', FWD_REFUSALS, ids=[f'{i}-{"-".join(k)}' for i, (k, _, _) in enumerate(FWD_REFUSALS)])
def test_forward_entry_refuses_before_any_launch(L, kw, code, needle):
    _refused(L, _fwd(L, **kw), code, needle, NAMES[0])


@pytest.mark.parametrize('kw,code,needle', BWD_REFUSALS, ids=[f'{i}-{"-".join(k)}' for i, (k, _, _) in enumerate(BWD_REFUSALS)])
def test_backward_entry_refuses_before_any_launch(L, kw, code, needle):
    _refused(L, _bwd(L, **kw), code, needle, NAMES[1])


@pytest.mark.parametrize('call,name', [(_fwd, NAMES[0]), (_bwd, NAMES[1])])
def test_a_width_that_is_no_multiple_of_four_is_refused_with_dropout(L, call, name):
    _refused(L, call(L, d=130, drop_audio=_drop(0.1)), 'EINVAL', 'd=130', name)
    _refused(L, call(L, d=126, drop_text=_drop(0.1)), 'EINVAL', 'd=126', name)
    _refused(L, call(L, drop_text=_drop(1.0)), 'EINVAL', 'dropout p', name)


def test_backward_takes_null_gradient_tables_but_everything_else(L):
    """A NULL gradient table is a table without a gradient, not an error: the next fault in line is the one named."""
    _refused(L, _bwd(L, text_table=None, tables=_tables(8, null=2), M=0), 'EINVAL', 'M=0', NAMES[1])


# ---- training_step_packed: refusals before any device work -----------------------------------------------------------
def _model(**kw):
    from valle2_amd import get_model_class
    return get_model_class('ValleNAR')(C.cfg_of(dict(N.KW, **kw)))


def _batch():
    return {k: v.clone() for k, v in N.inputs()[2].items()}


def test_training_step_packed_refusals_need_no_device(monkeypatch):
    from valle2_amd import _lib, kernels
    monkeypatch.setattr(kernels, 'ids_to_device', lambda *a, **k: pytest.fail('device work before the refusal'))
    monkeypatch.setattr(_lib, 'to_device_async', lambda *a, **k: pytest.fail('device work before the refusal'))
    with pytest.raises(ValueError, match='head width 32'):
        _model(n_heads=4).training_step_packed(_batch(), stage=1)
    with pytest.raises(_lib.VhError, match='HIP device'):
        with torch.enable_grad():
            _model().training_step_packed(_batch(), stage=1)
    for stage in (0, 8, -1, 1.5, True):
        with pytest.raises(ValueError, match='stage=.* is outside 1 .. 7'):
            _model().training_step_packed(_batch(), stage=stage)
    b = _batch()
    b['codes_lens'][1] = 0
    with pytest.raises(ValueError, match='codes_lens entry 0 is outside 1 .. 500'):
        _model().training_step_packed(b, stage=1)
    b = _batch()
    b['tokens_lens'][3] = 41
    with pytest.raises(ValueError, match='tokens_lens entry 41 is outside 1 .. 40'):
        _model().training_step_packed(b, stage=1)
    b = _batch()
    b['codes_lens'][0] = 501
    with pytest.raises(ValueError, match='codes_lens entry 501'):
        with torch.no_grad():
            _model().training_step_packed(b, stage=1)
    b = _batch()
    b['codes_lens'] = b['codes_lens'][:4]
    with pytest.raises(ValueError, match='5 rows of tokens.* 4 codes_lens'):
        _model().training_step_packed(b, stage=1)
    b = _batch()
    b['tokens_lens'] = torch.cat([b['tokens_lens'], torch.tensor([3])])
    with pytest.raises(ValueError, match='6 tokens_lens'):
        _model().training_step_packed(b, stage=1)


def test_the_stage_is_drawn_where_training_step_draws_it(monkeypatch):
    """Without stage=, one random.randint(1, Q - 1) before anything else — the refusal that follows shows the draw came first."""
    import random
    drawn = []
    monkeypatch.setattr(random, 'randint', lambda a, b: drawn.append((a, b)) or 3)
    with pytest.raises(ValueError, match='head width 32'):
        _model(n_heads=4).training_step_packed(_batch())
    assert drawn == [(1, 7)]
    with pytest.raises(ValueError, match='head width 32'):
        _model(n_heads=4).training_step_packed(_batch(), stage=2)
    assert drawn == [(1, 7)]


def test_signatures_are_pinned():
    from valle2_amd import get_model_class, train_model
    nar = get_model_class('ValleNAR')
    assert str(inspect.signature(nar.training_step)) == '(self, batch, **kwargs)'
    assert str(inspect.signature(nar.training_step_packed)) == '(self, batch, **kwargs)'
    assert str(inspect.signature(get_model_class('ValleAR').training_step_packed)) == '(self, batch, **kwargs)'
    assert str(inspect.signature(train_model.train)) == "(hparams_fp: 'Path', model_name: 'str', batches=None, device=None, log=<built-in function print>)"


# ---- train(): which step VALLE2_TRAIN_PACKED selects, with a spy and no device ------------------------------------------
class _Stop(Exception):
    pass


@pytest.mark.parametrize('model_name', ['ValleAR', 'ValleNAR'])
@pytest.mark.parametrize('value,packed', [('1', True), (None, False), ('0', False)])
def test_train_dispatch(monkeypatch, model_name, value, packed):
    from valle2_amd import get_model_class, train_model
    from valle2_amd.config import ConfigValle
    if value is None:
        monkeypatch.delenv('VALLE2_TRAIN_PACKED', raising=False)
    else:
        monkeypatch.setenv('VALLE2_TRAIN_PACKED', value)
    cls = get_model_class(model_name)
    calls = []

    def spy(which):
        def step(self, batch, **kw):
            calls.append(which)
            raise _Stop()
        return step
    monkeypatch.setattr(cls, 'training_step', spy('padded'))
    monkeypatch.setattr(cls, 'training_step_packed', spy('packed'))
    # the optimizer and the gradient exchange live on the device: stand-ins with the attributes train() touches before
    # the first step
    from types import SimpleNamespace
    from valle2_amd import dp
    fake = SimpleNamespace(flat_grad=None, slots=None, zero_grad=lambda: None)
    monkeypatch.setattr(cls, 'configure_optimizers', lambda self: {'optimizer': fake, 'lr_scheduler': None})
    monkeypatch.setattr(dp, 'GradReducer', lambda *a: SimpleNamespace(enabled=False))
    norm = 'LayerNorm' if model_name == 'ValleAR' else 'AdaptiveLayerNorm'
    cfg = ConfigValle(**dict(N.KW, norm=norm), max_steps=1, batch_size=2, grad_accum=1, log_every_n_steps=1000, seed=3)
    with pytest.raises(_Stop):
        train_model.train(cfg, model_name, batches=[{}], device=torch.device('cpu'), log=lambda *a: None)
    assert calls == ['packed' if packed else 'padded']
