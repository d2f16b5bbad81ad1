"""The EnCodec encoder without a GPU: the float64 mirror (tests/codec_enc_mirror.py) against the recorded fixture and, where
`transformers` is installed, against a live default-config model; the frame count; every refusal of
`EncodecEncoder.from_state_dict` and of the encode methods; the ABI of the three entries (header, binding, export, version 146,
INTEGRATION.md); and every refusal of each entry with made-up aligned pointers that are never dereferenced (all checks run
before any launch)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import codec_enc_mirror as E
from tests import codec_mirror as M
from tests.golden.gen_codec_golden import SMALL

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
VH_OK, VH_EINVAL, VH_EALIGN, VH_EUNSUPPORTED = 0, -1, -2, -3
ENTRIES = ('vh_conv1d_wave', 'vh_conv1d_down', 'vh_rvq_encode')
CTYPE = {'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p,
         'const int64_t*': ctypes.c_void_p, 'int64_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int': ctypes.c_int}
LENGTHS = (1, 5, 8, 9, 67, 72)


@pytest.fixture(scope='module')
def small():
    z = np.load(REPO / 'tests' / 'golden' / 'codec_enc_small.npz')
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith('sd/')}


# ---- the mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_mirror_reproduces_the_recorded_embeddings_codes_and_margins(small, L):
    sd, rec = small
    wave, emb64, codes64 = rec[f'wave/{L}'], rec[f'emb64/{L}'], rec[f'codes64/{L}']
    T = -(-L // 8)
    assert tuple(wave.shape) == (2, L) and tuple(emb64.shape) == (2, T, 32) and tuple(codes64.shape) == (2, 8, T)
    assert emb64.dtype == torch.float64 and codes64.dtype == torch.int64
    codes, emb = E.encode(sd, wave, **SMALL)
    assert (emb - emb64).abs().max().item() <= 1e-10
    assert torch.equal(codes, codes64)
    # the fp32 mode is the same arithmetic in fp32: as close to float64 as the recorded fp32 model is, and the same codes
    codes32, emb32 = E.encode(sd, wave, torch.float32, **SMALL)
    e32 = (emb32.double() - emb64).abs().max().item()
    assert 0 < e32 < 10 * (rec[f'emb32/{L}'].double() - emb64).abs().max().item()
    assert torch.equal(codes32, rec[f'codes32/{L}']) and torch.equal(rec[f'codes32/{L}'], codes64)
    walked, margin, e_score = E.rvq_scores(E.codebooks_of(sd), emb64.reshape(2 * T, 32), emb32.reshape(2 * T, 32))
    assert torch.equal(walked.view(8, 2, T).transpose(0, 1), codes64)
    assert (margin.view(2, T) - rec[f'margin/{L}']).abs().max().item() <= 1e-9
    assert margin.min().item() > 16 * e_score > 0                       # every recorded frame is decided
    assert E.chosen_gaps(E.codebooks_of(sd), emb64.reshape(2 * T, 32), walked).abs().max().item() == 0.0


@pytest.mark.parametrize('L', [960, 967])
def test_mirror_equals_a_live_default_config_model(L):
    pytest.importorskip('transformers')
    from tests.golden.gen_codec_enc_golden import encoder_state_dict, model_encode
    from tests.golden.gen_codec_golden import build_model
    model = build_model(3).double()                     # ratios 8, 5, 4, 2 reversed; channels 32 .. 512
    wave = 0.3 * torch.randn(2, L, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    want_codes, want_emb = model_encode(model, wave)
    sd = encoder_state_dict(model)
    codes, emb = E.encode(sd, wave)
    T = -(-L // 320)
    assert tuple(emb.shape) == (2, T, 128) and tuple(codes.shape) == tuple(want_codes.shape) and codes.shape[2] == T
    assert (emb - want_emb).abs().max().item() <= 1e-10 * max(1.0, want_emb.abs().max().item())
    assert torch.equal(codes, want_codes)


@pytest.mark.parametrize('L', [1, 7, 8, 9, 15, 16, 17, 63, 64, 65])
def test_frame_count_is_the_ceiling(small, L):
    sd, _ = small
    from valle2_amd import EncodecEncoder
    wave = torch.randn(1, L, generator=torch.Generator().manual_seed(L))
    assert E.encoder(sd, wave, **SMALL).shape[-1] == -(-L // 8) == E.frames_of(L, M.arch_of(**SMALL))
    assert EncodecEncoder.from_state_dict(sd, **SMALL).frames(L) == -(-L // 8)
    assert E.frames_of(L, M.arch_of()) == -(-L // 320)


def test_padding_restates_the_small_input_rule():
    x = torch.arange(1.0, 4.0)[None, None]                                           # 1 2 3
    assert E.pad_causal(x, 2, 1)[0, 0].tolist() == [3, 2, 1, 2, 3, 2]
    assert E.pad_causal(x[..., :2], 2, 2)[0, 0].tolist() == [0, 2, 1, 2, 0, 2]      # zero-extended to 3, reflected, trimmed
    assert E.pad_causal(x[..., :1], 4, 3)[0, 0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert E.pad_causal(x[..., :1], 1, 1)[0, 0].tolist() == [0, 1, 0]


# ---- from_state_dict -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('field,value', [('use_causal_conv', False), ('norm_type', 'time_group_norm'), ('pad_mode', 'constant'),
                                         ('trim_right_ratio', 0.5), ('audio_channels', 2), ('normalize', True),
                                         ('chunk_length_s', 1.0), ('use_conv_shortcut', False), ('num_filters', 6),
                                         ('hidden_size', 30), ('hidden_size', 256), ('compress', 16), ('num_lstm_layers', 0),
                                         ('upsampling_ratios', ()), ('upsampling_ratios', (40, 2)), ('codebook_size', 32768)])
def test_from_state_dict_refuses_what_is_outside_the_family_by_field_name(small, monkeypatch, field, value):
    from valle2_amd import EncodecEncoder, _lib
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('device work before the refusal'))
    with pytest.raises(ValueError, match=field):
        EncodecEncoder.from_state_dict(small[0], **dict(SMALL, **{field: value}))


def test_from_state_dict_names_unknown_fields_missing_keys_and_wrong_shapes(small):
    from valle2_amd import EncodecEncoder
    sd = small[0]
    with pytest.raises(ValueError, match='bandwidth'):
        EncodecEncoder.from_state_dict(sd, bandwidth=6.0, **SMALL)
    for key in ('encoder.layers.0.conv.bias', 'encoder.layers.9.lstm.weight_hh_l1', 'encoder.layers.2.shortcut.conv.parametrizations.weight.original0',
                'encoder.layers.4.conv.parametrizations.weight.original1', 'encoder.layers.11.conv.bias', 'quantizer.layers.0.codebook.embed'):
        assert key in sd, key
        with pytest.raises(KeyError, match=re.escape(key)):
            EncodecEncoder.from_state_dict({k: v for k, v in sd.items() if k != key}, **SMALL)
    with pytest.raises(ValueError, match='encoder.layers.0.conv weight has shape'):
        EncodecEncoder.from_state_dict(sd, **dict(SMALL, kernel_size=5))
    with pytest.raises(ValueError, match='encoder.layers.4.conv weight has shape'):
        EncodecEncoder.from_state_dict(sd, **dict(SMALL, upsampling_ratios=(4, 4)))
    with pytest.raises(ValueError, match='codebook.embed has shape'):
        EncodecEncoder.from_state_dict(sd, **dict(SMALL, codebook_size=128))


def test_from_state_dict_folds_weight_norm_and_repacks_without_a_device(small):
    import valle2_amd
    from valle2_amd import EncodecCodec, EncodecEncoder
    sd = small[0]
    enc = EncodecEncoder.from_state_dict(sd, **SMALL)
    assert valle2_amd.EncodecEncoder is EncodecEncoder and {'EncodecEncoder', 'EncodecCodec'} <= set(valle2_amd.__all__)
    assert enc.hop == 8 and enc.ratios == (2, 4) and enc.sampling_rate == 24000 and enc.num_codebooks == 8
    w, b = M.folded(sd, 'encoder.layers.0.conv', torch.float64)                      # (8, 1, 7)
    assert torch.equal(enc._host['first'][0], w[:, 0].float()) and torch.equal(enc._host['first'][1], b.float())
    wd, bd = M.folded(sd, 'encoder.layers.4.conv', torch.float64)                    # (16, 8, 4), stride 2
    down, down_b = enc._host['stages'][0]['down']
    assert tuple(down.shape) == (16, 4, 8) and torch.equal(down, wd.permute(0, 2, 1).float()) and torch.equal(down_b, bd.float())
    assert tuple(enc._host['stages'][1]['down'][0].shape) == (32, 8, 16)
    assert [blk['dilation'] for blk in enc._host['stages'][1]['blocks']] == [1, 2]
    books = E.codebooks_of(sd)
    assert torch.equal(enc._host['e_sq'], books.pow(2).sum(-1).float()) and enc._host['e_sq'].dtype == torch.float32
    assert tuple(enc._host['lstm'][1][2].shape) == (128, 32) and tuple(enc._host['last'][0].shape) == (32, 7, 32)
    # both halves from one state dict
    both = dict(M.random_state_dict(seed=0, n_codebooks=8, **SMALL))
    both.update(sd)
    codec = EncodecCodec.from_state_dict(both, **SMALL)
    assert codec.hop == 8 and codec.num_codebooks == 8 and codec.sampling_rate == 24000
    for name in ('encode', 'batch_encode', 'encode_many', 'decode', 'batch_decode', 'decode_many', 'encode_decode', 'get_embedding'):
        assert callable(getattr(codec, name)), name
    other = dict(both)
    other.pop('quantizer.layers.7.codebook.embed')
    with pytest.raises(ValueError, match='two halves'):
        EncodecCodec(enc, valle2_amd.EncodecDecoder.from_state_dict(other, **SMALL))


def test_encode_refusals_come_before_any_device_work(small, monkeypatch):
    from valle2_amd import EncodecEncoder, _lib
    enc = EncodecEncoder.from_state_dict(small[0], **SMALL)
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('device work before the refusal'))
    wave = torch.zeros(40)
    with pytest.raises(ValueError, match='floating-point waveform'):
        enc.encode(torch.zeros(40, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'expected a 1-D waveform \(L,\)'):
        enc.encode(wave[None])
    with pytest.raises(ValueError, match=r'expected a 2-D waveform \(B, L\)'):
        enc.batch_encode(wave)
    with pytest.raises(ValueError, match='empty waveform'):
        enc.encode(wave[:0])
    with pytest.raises(ValueError, match='empty waveform'):
        enc.embed(wave[:0])
    with pytest.raises(ValueError, match=r'waves\[1\]: an empty waveform'):
        enc.encode_many([wave, wave[:0]])
    with pytest.raises(ValueError, match=r'waves\[1\] is on meta'):
        enc.encode_many([wave, torch.zeros(3, device='meta')])
    for q in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match='num_codebooks='):
            enc.encode(wave, num_codebooks=q)
        with pytest.raises(ValueError, match='num_codebooks='):
            enc.encode_many([wave, wave], num_codebooks=q)
    for call in (lambda: enc.encode(wave), lambda: enc.embed(wave), lambda: enc.batch_encode(wave[None]),
                 lambda: enc.encode_many([wave, wave[:3]])):
        with pytest.raises(_lib.VhError, match='no CPU fallback'):
            call()                                                                   # host samples: nothing computes on the CPU
    assert enc.encode_many([]) == []


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


WAVE = dict(x=P[0], w=P[1], bias=P[2], out=P[3], B=2, L=9, C_out=8, taps=7, lens=P[4], stream=None)
DOWN = dict(x=P[0], w=P[1], bias=P[2], out=P[3], B=2, T=9, C_in=32, C_out=64, taps=4, stride=2, elu=1, lens=P[4], stream=None)
RVQ = dict(x=P[0], codebooks=P[1], e_sq=P[2], codes=P[3], B=2, T=9, D=32, Q=4, n_books=8, K=64, stream=None)


def test_conv1d_wave_refusals():
    for name in ('x', 'w', 'out'):
        _refused('vh_conv1d_wave', WAVE, VH_EINVAL, 'null pointer', **{name: None})
    for off in (4, 8, 12):
        _refused('vh_conv1d_wave', WAVE, VH_EALIGN, '16-byte aligned', out=WAVE['out'] + off)
    for name in ('x', 'w', 'bias', 'lens'):
        _refused('vh_conv1d_wave', WAVE, VH_EALIGN, '4-byte aligned', **{name: WAVE[name] + 2})
    for name in ('B', 'L'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_conv1d_wave', WAVE, VH_EINVAL, f'{name}={v}', **{name: v})
    for t in (0, -1, 65, 2 ** 31 - 1):
        _refused('vh_conv1d_wave', WAVE, VH_EINVAL, f'taps={t}', taps=t)
    for c in (0, -4, 1, 2, 6, 30, 2 ** 31 - 1):
        _refused('vh_conv1d_wave', WAVE, VH_EUNSUPPORTED, f'C_out={c}', C_out=c)
    _refused('vh_conv1d_wave', WAVE, VH_EINVAL, '2^40', B=2 ** 15, L=2 ** 20, C_out=64)
    _refused('vh_conv1d_wave', WAVE, VH_EINVAL, '2^40', B=2 ** 31 - 1, L=2 ** 31 - 1, C_out=2 ** 31 - 4)
    # optional operands may be null: the next check in line refuses
    assert 'C_out=5' in _call('vh_conv1d_wave', WAVE, dict(bias=None, lens=None, C_out=5))[1]


def test_conv1d_down_refusals():
    for name in ('x', 'w', 'out'):
        _refused('vh_conv1d_down', DOWN, VH_EINVAL, 'null pointer', **{name: None})
    for name in ('x', 'w', 'out'):
        for off in (4, 8, 12):
            _refused('vh_conv1d_down', DOWN, VH_EALIGN, '16-byte aligned', **{name: DOWN[name] + off})
    for name in ('bias', 'lens'):
        _refused('vh_conv1d_down', DOWN, VH_EALIGN, '4-byte aligned', **{name: DOWN[name] + 2})
    for name in ('B', 'T'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_conv1d_down', DOWN, VH_EINVAL, f'{name}={v}', **{name: v})
    for s in (0, -1, 5, 65, 2 ** 31 - 1):                                           # stride beyond taps = 4
        _refused('vh_conv1d_down', DOWN, VH_EINVAL, f'stride={s}', stride=s)
    for t in (0, -1, 1, 65, 2 ** 31 - 1):                                           # taps below stride = 2, or beyond 64
        _refused('vh_conv1d_down', DOWN, VH_EINVAL, f'taps={t}', taps=t)
    for e in (-1, 2):
        _refused('vh_conv1d_down', DOWN, VH_EINVAL, f'elu={e}', elu=e)
    for c in (0, -4, 1, 2, 6, 30, 2 ** 31 - 1):
        _refused('vh_conv1d_down', DOWN, VH_EUNSUPPORTED, f'C_in={c}', C_in=c)
        _refused('vh_conv1d_down', DOWN, VH_EUNSUPPORTED, f'C_out={c}', C_out=c)
    _refused('vh_conv1d_down', DOWN, VH_EINVAL, 'exceed one grid', B=2 ** 31 - 1, T=2 ** 31 - 1, taps=1, stride=1)
    _refused('vh_conv1d_down', DOWN, VH_EINVAL, '2^40', B=2 ** 15, T=2 ** 20, C_in=64)
    _refused('vh_conv1d_down', DOWN, VH_EINVAL, 'exceeds one grid', C_out=2 ** 31 - 4, B=1, T=1)
    assert 'C_out=5' in _call('vh_conv1d_down', DOWN, dict(bias=None, lens=None, C_out=5))[1]


def test_rvq_encode_refusals():
    for name in ('x', 'codebooks', 'e_sq', 'codes'):
        _refused('vh_rvq_encode', RVQ, VH_EINVAL, 'null pointer', **{name: None})
    for name in ('x', 'codebooks'):
        for off in (4, 8, 12):
            _refused('vh_rvq_encode', RVQ, VH_EALIGN, '16-byte aligned', **{name: RVQ[name] + off})
    _refused('vh_rvq_encode', RVQ, VH_EALIGN, '4-byte aligned', e_sq=RVQ['e_sq'] + 2)
    _refused('vh_rvq_encode', RVQ, VH_EALIGN, '8-byte', codes=RVQ['codes'] + 4)
    for name in ('B', 'T', 'Q', 'n_books', 'K'):
        for v in (0, -1, -2 ** 31):
            _refused('vh_rvq_encode', RVQ, VH_EINVAL, f'{name}={v}', **{name: v})
    _refused('vh_rvq_encode', RVQ, VH_EINVAL, 'Q=9 codebooks asked of n_books=8', Q=9)
    for d in (0, -4, 2, 30, 33, 132, 256, 2 ** 31 - 1):
        _refused('vh_rvq_encode', RVQ, VH_EUNSUPPORTED, f'D={d}', D=d)
    for k in (16385, 2 ** 31 - 1):
        _refused('vh_rvq_encode', RVQ, VH_EUNSUPPORTED, f'K={k}', K=k)
    _refused('vh_rvq_encode', RVQ, VH_EINVAL, 'exceed one grid', B=2 ** 31 - 1, T=2 ** 31 - 1)
    _refused('vh_rvq_encode', RVQ, VH_EINVAL, '2^40', B=2 ** 15, T=2 ** 20, D=128)
