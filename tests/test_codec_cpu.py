"""The EnCodec decoder without a GPU: the float64 mirror (tests/codec_mirror.py) against the recorded fixture and, where
`transformers` is installed, against a live default-config model; the mirror's causality; every refusal of
`EncodecDecoder.from_state_dict`; the ABI of the three entries (header, binding, export, version 146); and
every refusal of each entry with made-up aligned pointers that are never dereferenced (all checks run before any launch)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import codec_mirror as M
from tests.golden.gen_codec_golden import SMALL

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
VH_OK, VH_EINVAL, VH_EALIGN, VH_EUNSUPPORTED = 0, -1, -2, -3
ENTRIES = ('vh_rvq_decode', 'vh_conv1d_causal', 'vh_lstm_layer')
CTYPE = {'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p,
         'const int64_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int': ctypes.c_int}


@pytest.fixture(scope='module')
def small():
    z = np.load(REPO / 'tests' / 'golden' / 'codec_small.npz')
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, torch.from_numpy(z['codes']), torch.from_numpy(z['wave64']), torch.from_numpy(z['wave32'])


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def test_mirror_reproduces_the_recorded_float64_waveform(small):
    sd, codes, wave64, wave32 = small
    assert tuple(codes.shape) == (2, 4, 9) and tuple(wave64.shape) == (2, 72) and wave64.dtype == torch.float64
    got = M.decode(sd, codes, **SMALL)
    assert (got - wave64).abs().max().item() <= 1e-10
    # the fp32 mode is the same arithmetic in fp32: as close to float64 as the recorded fp32 model is, to the order of magnitude
    e32 = (M.decode(sd, codes, torch.float32, **SMALL).double() - wave64).abs().max().item()
    assert 0 < e32 < 10 * (wave32.double() - wave64).abs().max().item()


@pytest.mark.parametrize('T', [1, 40])
def test_mirror_equals_a_live_default_config_model(T):
    pytest.importorskip('transformers')
    from tests.golden.gen_codec_golden import build_model, decoder_state_dict, model_decode
    model = build_model(3).double()                     # ratios 8, 5, 4, 2; channels 512 .. 16
    codes = torch.randint(0, 1024, (2, 8, T), generator=torch.Generator().manual_seed(T))
    want = model_decode(model, codes)
    got = M.decode(decoder_state_dict(model), codes)
    assert tuple(got.shape) == (2, 320 * T)
    assert (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item())


def test_mirror_is_causal_from_the_first_reflection_on(small):
    """A prefix of the codes decodes to the prefix of the waveform — once the prefix is longer than the first convolution's
    left padding (6 frames): the reflect padding at the start of an utterance reads x[1 .. 6], the FUTURE of frame 0, so a
    shorter utterance is not a prefix of a longer one (the reference's own behaviour; decode_many hands the kernels every
    utterance's length for that reason)."""
    sd = M.random_state_dict(seed=5, n_codebooks=2)
    codes = torch.randint(0, 1024, (1, 2, 20), generator=torch.Generator().manual_seed(6))
    full = M.decode(sd, codes)
    for T in (7, 13):
        assert (M.decode(sd, codes[:, :, :T]) - full[:, :320 * T]).abs().max().item() <= 1e-9 * full.abs().max().item()
    assert (M.decode(sd, codes[:, :, :3]) - full[:, :320 * 3]).abs().max().item() > 1e-3 * full.abs().max().item()


# ---- from_state_dict -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('field,value', [('use_causal_conv', False), ('norm_type', 'time_group_norm'), ('pad_mode', 'constant'),
                                         ('trim_right_ratio', 0.5), ('audio_channels', 2), ('normalize', True),
                                         ('chunk_length_s', 1.0), ('use_conv_shortcut', False), ('num_filters', 6),
                                         ('hidden_size', 30), ('compress', 16), ('num_lstm_layers', 0),
                                         ('upsampling_ratios', ())])
def test_from_state_dict_refuses_what_is_outside_the_family_by_field_name(small, monkeypatch, field, value):
    from valle2_amd import EncodecDecoder, _lib
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('device work before the refusal'))
    with pytest.raises(ValueError, match=field):
        EncodecDecoder.from_state_dict(small[0], **dict(SMALL, **{field: value}))


def test_from_state_dict_names_unknown_fields_missing_keys_and_wrong_shapes(small):
    from valle2_amd import EncodecDecoder
    sd = small[0]
    with pytest.raises(ValueError, match='bandwidth'):
        EncodecDecoder.from_state_dict(sd, bandwidth=6.0, **SMALL)
    for key in ('decoder.layers.0.conv.bias', 'decoder.layers.1.lstm.weight_hh_l1', 'decoder.layers.4.shortcut.conv.parametrizations.weight.original0',
                'decoder.layers.11.conv.parametrizations.weight.original1', 'quantizer.layers.0.codebook.embed'):
        with pytest.raises(KeyError, match=re.escape(key)):
            EncodecDecoder.from_state_dict({k: v for k, v in sd.items() if k != key}, **SMALL)
    with pytest.raises(ValueError, match='decoder.layers.0.conv weight has shape'):
        EncodecDecoder.from_state_dict(sd, **dict(SMALL, kernel_size=5))
    with pytest.raises(ValueError, match='codebook.embed has shape'):
        EncodecDecoder.from_state_dict(sd, **dict(SMALL, codebook_size=128))


def test_from_state_dict_folds_weight_norm_and_repacks_without_a_device(small):
    from valle2_amd import EncodecDecoder
    import valle2_amd
    sd = small[0]
    dec = EncodecDecoder.from_state_dict(sd, **SMALL)
    assert valle2_amd.EncodecDecoder is EncodecDecoder and 'EncodecDecoder' in valle2_amd.__all__
    assert dec.hop == 8 and dec.sampling_rate == 24000 and dec.num_codebooks == 8 and not hasattr(dec, 'encode')
    w, b = M.folded(sd, 'decoder.layers.0.conv', torch.float64)
    assert torch.equal(dec._host['first'][0], w.permute(0, 2, 1).float()) and dec._host['first'][0].dtype == torch.float32
    wt, bt = M.folded(sd, 'decoder.layers.3.conv', torch.float64)                    # (C_in 32, C_out 16, 8), stride 4
    up, up_b = dec._host['stages'][0]['up']
    assert tuple(up.shape) == (4 * 16, 2, 32) and torch.equal(up_b, bt.float().repeat(4))
    for p in range(4):
        assert torch.equal(up[p * 16:(p + 1) * 16, 0], wt[:, :, p + 4].t().float())   # the frame before
        assert torch.equal(up[p * 16:(p + 1) * 16, 1], wt[:, :, p].t().float())
    assert [blk['dilation'] for blk in dec._host['stages'][1]['blocks']] == [1, 2]


def test_codes_are_checked_with_validate_codes_messages(small):
    from valle2_amd import EncodecDecoder, _lib
    dec = EncodecDecoder.from_state_dict(small[0], **SMALL)
    codes = small[1]
    with pytest.raises(ValueError, match=r'expected a 2-D tensor in the codec layout \(Q, T\)'):
        dec.decode(codes)
    with pytest.raises(ValueError, match=r'expected a 3-D tensor in the codec layout \(B, Q, T\)'):
        dec.batch_decode(codes[0])
    with pytest.raises(ValueError, match='codec ids are int64'):
        dec.decode(codes[0].int())
    with pytest.raises(ValueError, match='9 codebooks, the decoder holds 8'):
        dec.decode(torch.zeros(9, 4, dtype=torch.int64))
    with pytest.raises(IndexError, match=r'ids span \[0, 64\], the codebooks hold 64 entries'):
        dec.decode(torch.tensor([[0, 64]]))
    with pytest.raises(IndexError, match=r'codes\[1\]: ids span \[-1, 3\]'):
        dec.decode_many([codes[0], torch.tensor([[3, -1]])])
    with pytest.raises(_lib.VhError, match='no CPU fallback'):
        dec.decode(codes[0])                                                         # host codes: nothing computes on the CPU


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def _declaration(name):
    m = re.search(r'^int %s\((.*?)\);' % name, HEADER, re.S | re.M)
    assert m, f'include/valle_hip.h does not declare {name}'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    return [(p.rsplit(' ', 1)[0], p.rsplit(' ', 1)[1]) for p in params]


@pytest.mark.parametrize('name', ENTRIES)
def test_header_binding_and_library_agree(name):
    from valle2_amd import _lib
    decl = _declaration(name)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args == [CTYPE[t] for t, _ in decl], 'argtypes of the binding differ from the declaration'
    lib = _lib.load_library()
    assert getattr(lib, name).argtypes == args
    assert decl[-1] == ('void*', 'stream')


def test_abi_version_stays_and_the_integration_guide_lists_the_entries_as_additions():
    from valle2_amd import _lib
    assert int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1)) == 146
    assert _lib.load_library().vh_version() == 146
    text = (REPO / 'INTEGRATION.md').read_text()
    for name in ENTRIES:
        row = next(line for line in text.splitlines() if f'`{name}`' in line)
        assert 'addition' in row, name


# ---- refusals: "device pointers" that are never dereferenced ---------------------------------------------------------------
P = [0x100000 * (i + 1) for i in range(8)]


def _call(name, defaults, over):
    from valle2_amd import _lib
    lib = _lib.load_library()
    assert set(over) <= set(defaults), over
    a = dict(defaults, **over)
    rc = getattr(lib, name)(*a.values())
    return rc, (lib.vh_last_error() or b'').decode()


def _refused(name, defaults, code, needle, **over):
    rc, msg = _call(name, defaults, over)
    assert rc == code and name in msg and needle in msg, (over, rc, msg)


RVQ = dict(codes=P[0], codebooks=P[1], out=P[2], B=2, Q=4, T=9, n_books=8, K=64, D=32, err_flag=P[3], stream=None)
CONV = dict(x=P[0], w=P[1], bias=P[2], residual=P[3], out=P[4], B=2, T=9, C_in=32, C_out=16, taps=3, dilation=2, pad_mode=1, elu=1,
            lens=P[5], len_scale=4, stream=None)
LSTM = dict(xproj=P[0], w_hh=P[1], h_seq=P[2], c=P[3], skip=P[4], y=P[5], B=2, T=9, H=32, stream=None)


def test_rvq_decode_refusals():
    for name in ('codes', 'codebooks', 'out'):
        _refused('vh_rvq_decode', RVQ, VH_EINVAL, 'null pointer', **{name: None})
    for name in ('codebooks', 'out'):
        _refused('vh_rvq_decode', RVQ, VH_EALIGN, '16-byte aligned', **{name: RVQ[name] + 4})
    _refused('vh_rvq_decode', RVQ, VH_EALIGN, '8-byte', codes=RVQ['codes'] + 4)
    for name in ('B', 'Q', 'T', 'n_books', 'K'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_rvq_decode', RVQ, VH_EINVAL, f'{name}={v}', **{name: v})
    _refused('vh_rvq_decode', RVQ, VH_EINVAL, 'Q=9 codebooks asked of n_books=8', Q=9)
    for d in (0, -4, 2, 30, 33):
        _refused('vh_rvq_decode', RVQ, VH_EUNSUPPORTED, f'D={d}', D=d)
    _refused('vh_rvq_decode', RVQ, VH_EINVAL, 'exceed one grid', B=2 ** 31 - 1, T=2 ** 31 - 1, D=2 ** 31 - 4)


def test_conv1d_causal_refusals():
    for name in ('x', 'w', 'out'):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, 'null pointer', **{name: None})
    for name in ('x', 'w', 'residual', 'out'):
        for off in (4, 8, 12):
            _refused('vh_conv1d_causal', CONV, VH_EALIGN, '16-byte aligned', **{name: CONV[name] + off})
    _refused('vh_conv1d_causal', CONV, VH_EALIGN, 'bias=', bias=CONV['bias'] + 2)
    _refused('vh_conv1d_causal', CONV, VH_EALIGN, 'lens=', lens=CONV['lens'] + 2)
    for name in ('B', 'T'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'{name}={v}', **{name: v})
    for c in (0, -4, 1, 2, 6, 30, 2 ** 31 - 1):
        _refused('vh_conv1d_causal', CONV, VH_EUNSUPPORTED, f'C_in={c}', C_in=c)
    for c in (0, -1, -4, 2, 3, 6, 30, 2 ** 31 - 1):
        _refused('vh_conv1d_causal', CONV, VH_EUNSUPPORTED, f'C_out={c}', C_out=c)
    for t in (0, -1, 65):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'taps={t}', taps=t)
    for d in (0, -1, 4097):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'dilation={d}', dilation=d)
    for m in (-1, 2, 7):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'pad_mode={m}', pad_mode=m)
    for e in (-1, 2):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'elu={e}', elu=e)
    for s in (0, -1, 2 ** 20 + 1):
        _refused('vh_conv1d_causal', CONV, VH_EINVAL, f'len_scale={s}', len_scale=s)
    _refused('vh_conv1d_causal', CONV, VH_EINVAL, 'exceed one grid', B=2 ** 31 - 1, T=2 ** 31 - 1)
    _refused('vh_conv1d_causal', CONV, VH_EINVAL, '2^40', B=2 ** 15, T=2 ** 20, C_in=64)
    # optional operands may be null; without lens the scale is not read
    from valle2_amd import _lib
    assert 'C_out=5' in _call('vh_conv1d_causal', CONV, dict(bias=None, residual=None, lens=None, len_scale=0, C_out=5))[1]
    assert _lib.load_library().vh_last_error().decode().startswith('vh_conv1d_causal: C_out=5 (a multiple of 4, or 1')


def test_lstm_layer_refusals():
    for name in ('xproj', 'w_hh', 'h_seq', 'c'):
        _refused('vh_lstm_layer', LSTM, VH_EINVAL, 'null pointer', **{name: None})
    _refused('vh_lstm_layer', LSTM, VH_EINVAL, 'go together', skip=None)
    _refused('vh_lstm_layer', LSTM, VH_EINVAL, 'go together', y=None)
    for name in ('xproj', 'w_hh', 'h_seq', 'c', 'skip', 'y'):
        _refused('vh_lstm_layer', LSTM, VH_EALIGN, '16-byte aligned', **{name: LSTM[name] + 8})
    for name in ('B', 'T'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_lstm_layer', LSTM, VH_EINVAL, f'{name}={v}', **{name: v})
    _refused('vh_lstm_layer', LSTM, VH_EINVAL, 'T=1048577', T=2 ** 20 + 1)
    for h in (0, -4, 2, 30, 1028, 2048, 2 ** 31 - 1):
        _refused('vh_lstm_layer', LSTM, VH_EUNSUPPORTED, f'H={h}', H=h)
    _refused('vh_lstm_layer', LSTM, VH_EINVAL, '2^40', B=2 ** 31 - 1, T=2 ** 20, H=1024)
