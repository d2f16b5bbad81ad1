"""The EnCodec decoder's kernels (`vh_rvq_decode`, `vh_conv1d_causal`, `vh_lstm_layer`) and `valle2_amd.EncodecDecoder` on the
device, every comparison against the float64 mirror (tests/codec_mirror.py).

Tolerance, the same rule everywhere: e_ref = max |mirror_fp32 - mirror_fp64| on the comparison's own inputs — the error of the
reference's own fp32 arithmetic on the CPU — and the kernels must stay within 8 e_ref of the float64 mirror (the factor covers
the MFMA's k-ordered sums and a recurrence of T steps on other roundings).  Every test prints its figures before it asserts.
`vh_rvq_decode` is held to bit equality with fp32 torch adding in codebook order.
Measured on an MI355X: worst error / e_ref 2.62 over the convolution cases, 1.15 over the LSTM cases, 0.68
on the small fixture and 0.83 / 1.01 / 0.96 at the default config for T = 1 / 3 / 40."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import codec_mirror as M
from tests.codec_rules import DEV, g, within
from tests.golden.gen_codec_golden import SMALL

pytestmark = pytest.mark.gpu
GOLDEN = M.__file__.rsplit('/', 1)[0] + '/golden/codec_small.npz'


# ---- vh_rvq_decode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Q', [1, 8])
def test_rvq_decode_is_bit_equal_to_fp32_torch_adding_in_codebook_order(Q):
    from valle2_amd import kernels as K
    B, T, n_books, Kc, D = 3, 37, 8, 64, 36
    books = torch.randn(n_books, Kc, D, generator=g(1))
    codes = torch.randint(0, Kc, (B, Q, T), generator=g(2))
    want = torch.full((), 0.0)
    for q in range(Q):
        want = want + F.embedding(codes[:, q], books[q])
    got = K.rvq_decode(codes.to(DEV), books.to(DEV)).cpu()
    assert torch.equal(got, want)


def test_rvq_decode_raises_the_device_error_flag_and_never_reads_a_bad_id():
    from valle2_amd import _lib, kernels as K
    books = torch.randn(2, 16, 8, generator=g(3))
    codes = torch.randint(0, 16, (1, 2, 5), generator=g(4))
    bad = codes.clone()
    bad[0, 1, 2] = 16
    bad[0, 0, 4] = -1
    _lib.raise_device_errors(DEV)
    got = K.rvq_decode(bad.to(DEV), books.to(DEV)).cpu()
    with pytest.raises(IndexError, match='codec id'):
        _lib.raise_device_errors(DEV)
    assert torch.equal(got[0, 2], books[0][codes[0, 0, 2]]) and torch.equal(got[0, 4], books[1][codes[0, 1, 4]])
    assert torch.equal(got[0, 0], books[0][codes[0, 0, 0]] + books[1][codes[0, 1, 0]])


# ---- vh_conv1d_causal ------------------------------------------------------------------------------------------------------
TAPS = [(7, 1), (3, 1), (3, 2), (1, 1)]
CHANNELS = [(128, 512), (32, 16), (16, 32), (32, 1), (4, 8)]


def lengths(taps, dil):
    pad = (taps - 1) * dil
    return sorted({1, 2, max(pad, 1), pad + 1, 33, 129})


def conv_case(B, T, c_in, c_out, taps, dil, seed):
    x = torch.randn(B, c_in, T, generator=g(seed))
    w = torch.randn(c_out, c_in, taps, generator=g(seed + 1)) / (c_in * taps) ** 0.5
    b = torch.randn(c_out, generator=g(seed + 2))
    r = torch.randn(B, c_out, T, generator=g(seed + 3))
    return x, w, b, r


def run_conv(x, w, b, r, dil, mode, elu):
    """The kernel on torch-layout operands: x (B, C, T), w (C_out, C_in, K), r (B, C_out, T) or None -> (B, C_out, T) on the CPU."""
    from valle2_amd import kernels as K
    out = K.conv1d_causal(x.transpose(1, 2).contiguous().to(DEV), w.permute(0, 2, 1).contiguous().to(DEV), b.to(DEV),
                          None if r is None else r.transpose(1, 2).contiguous().to(DEV), dilation=dil,
                          pad_mode=K.PAD_REFLECT if mode == 'reflect' else K.PAD_ZERO, elu=elu)
    return out.cpu().transpose(1, 2)


@pytest.mark.parametrize('c_in,c_out', CHANNELS)
@pytest.mark.parametrize('taps,dil', TAPS)
def test_conv1d_causal_against_the_float64_mirror(taps, dil, c_in, c_out):
    worst = 0.0
    for T in lengths(taps, dil):
        x, w, b, r = conv_case(2, T, c_in, c_out, taps, dil, 10 * T + taps)
        for mode, elu, res in itertools.product(('reflect', 'zeros'), (False, True), (False, True)):
            ref = [M.conv1d_causal(x.to(dt), w.to(dt), b.to(dt), dil, mode, elu, r.to(dt) if res else None)
                   for dt in (torch.float64, torch.float32)]
            got = run_conv(x, w, b, r if res else None, dil, mode, elu)
            e_ref, err = within(f'conv K{taps} d{dil} {c_in}->{c_out} T{T} {mode} elu{int(elu)} res{int(res)}', got, *ref)
            worst = max(worst, err / e_ref)
    print(f'worst ratio {worst:.2f}')


@pytest.mark.parametrize('taps,dil', TAPS)
def test_conv1d_causal_window_never_crosses_a_batch_row(taps, dil):
    """B = 3, the neighbouring batch rows NaN: batch row 1 is finite and what it is alone."""
    c_in, c_out = 32, 16
    for T in lengths(taps, dil):
        x, w, b, r = conv_case(3, T, c_in, c_out, taps, dil, 7 * T + dil)
        x[0] = float('nan')
        x[2] = float('nan')
        for mode in ('reflect', 'zeros'):
            ref = [M.conv1d_causal(x[1:2].to(dt), w.to(dt), b.to(dt), dil, mode, True, r[1:2].to(dt)) for dt in (torch.float64, torch.float32)]
            got = run_conv(x, w, b, r, dil, mode, True)
            assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all()
            within(f'NaN neighbours K{taps} d{dil} T{T} {mode}', got[1:2], *ref)
            assert torch.equal(got[1:2], run_conv(x[1:2], w, b, r[1:2], dil, mode, True))          # the bits it has alone


@pytest.mark.parametrize('r', [8, 5, 2])
def test_transposed_convolution_as_a_two_tap_window(r):
    """ConvTranspose1d(C_in, C_out, 2 r, stride r) trimmed by r on the right, against F.conv_transpose1d plus the trim."""
    from valle2_amd import kernels as K
    from valle2_amd.codec import _conv_transpose
    c_in, c_out = 64, 32
    for T in (1, 2, 33, 129):
        x = torch.randn(2, c_in, T, generator=g(r + T))
        v = torch.randn(c_in, c_out, 2 * r, generator=g(r + T + 1))
        gain = v.pow(2).sum((1, 2), keepdim=True).sqrt() / (2 * c_in) ** 0.5
        b = torch.randn(c_out, generator=g(r + T + 2))
        sd = {'up.parametrizations.weight.original0': gain, 'up.parametrizations.weight.original1': v, 'up.bias': b}
        ref = [M.conv_transpose1d_causal(x.to(dt), *M.folded(sd, 'up', dt), stride=r, elu=True) for dt in (torch.float64, torch.float32)]
        w2, b2 = _conv_transpose(sd, 'up', c_in, c_out, r)
        got = K.conv1d_causal(x.transpose(1, 2).contiguous().to(DEV), w2.to(DEV), b2.to(DEV), pad_mode=K.PAD_ZERO, elu=True)
        got = got.view(2, T * r, c_out).cpu().transpose(1, 2)
        within(f'transposed r{r} T{T}', got, *ref)


# ---- the LSTM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [1, 2, 40])
@pytest.mark.parametrize('H', [32, 512])
def test_lstm_block_against_the_float64_mirror(H, T, B):
    """Two layers and the skip, as the decoder runs them: out = lstm(x) + x."""
    from valle2_amd import kernels as K
    x = torch.randn(B, T, H, generator=g(H + T + B))
    params = [[(2 * torch.rand(s, generator=g(100 * layer + i)) - 1) / H ** 0.5 for i, s in enumerate([(4 * H, H), (4 * H, H), (4 * H,), (4 * H,)])]
              for layer in range(2)]
    ref = []
    for dt in (torch.float64, torch.float32):
        h = x.to(dt).transpose(0, 1)
        for p in params:
            h = M.lstm_layer(h, *[t.to(dt) for t in p])
        ref.append((h + x.to(dt).transpose(0, 1)).transpose(0, 1))
    xd = x.to(DEV)
    h = xd
    for layer, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        xproj = K.conv1d_causal(h, w_ih[:, None, :].contiguous().to(DEV), (b_ih.double() + b_hh.double()).float().to(DEV))
        h = K.lstm_layer(xproj, w_hh.to(DEV), skip=xd if layer == 1 else None)
    within(f'lstm H{H} T{T} B{B}', h.cpu(), *ref)


# ---- the whole decoder -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, torch.from_numpy(z['codes']), torch.from_numpy(z['wave64']), torch.from_numpy(z['wave32'])


@pytest.fixture(scope='module')
def default():
    """A seeded default-config state dict, its decoder, and the mirror's two waveforms of codes (2, 8, 40), computed once."""
    from valle2_amd import EncodecDecoder
    sd = M.random_state_dict(seed=11)
    codes = torch.randint(0, 1024, (2, 8, 40), generator=g(12))
    return sd, EncodecDecoder.from_state_dict(sd), codes, M.decode(sd, codes), M.decode(sd, codes, torch.float32)


def test_decoder_on_the_small_fixture(small):
    from valle2_amd import EncodecDecoder
    sd, codes, wave64, wave32 = small
    dec = EncodecDecoder.from_state_dict(sd, **SMALL)
    assert dec.hop == 8 and dec.num_codebooks == 8 and codes.shape[1] == 4          # Q smaller than the stored codebooks
    got = dec.batch_decode(codes.to(DEV))
    assert got.is_cuda and tuple(got.shape) == (2, 72) and got.dtype == torch.float32
    within('small fixture', got, wave64, M.decode(sd, codes, torch.float32, **SMALL))
    assert torch.equal(dec.decode(codes[1].to(DEV)), got[1])


@pytest.mark.parametrize('T', [1, 3, 40])
def test_decoder_at_the_default_config(default, T):
    sd, dec, codes, wave64, wave32 = default
    if T == 40:
        ref = (wave64, wave32)
    else:
        ref = (M.decode(sd, codes[:, :, :T]), M.decode(sd, codes[:, :, :T], torch.float32))
    got = dec.batch_decode(codes[:, :, :T].to(DEV))
    assert tuple(got.shape) == (2, 320 * T) and dec.sampling_rate == 24000
    within(f'default config T{T}', got, *ref)


def test_ragged_decode_many_equals_each_utterance_alone_bit_for_bit(default):
    sd, dec, codes, _, _ = default
    items = [codes[0, :, :1].to(DEV), codes[1, :, :7].to(DEV), codes[0].to(DEV)]
    many = dec.decode_many(items)
    assert [tuple(w.shape) for w in many] == [(320,), (320 * 7,), (320 * 40,)]
    for w, c in zip(many, items):
        assert w.is_cuda and torch.equal(w, dec.decode(c))
    assert dec.decode_many([]) == []


def test_codec_io_synthesize_returns_a_device_waveform(default):
    from valle2_amd import codec_io as CIO, get_model_class, synth
    from valle2_amd.config import ConfigValle
    _, dec, _, _, _ = default
    cfg = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0)
    ar_cfg = ConfigValle(**cfg, norm='LayerNorm', num_beams=2, top_k=1, max_audio_len=12)
    nar_cfg = ConfigValle(**cfg, norm='AdaptiveLayerNorm')
    ar = get_model_class('ValleAR')(ar_cfg)
    ar.load_state_dict(synth.silence_eos(synth.make_state_dict(ar_cfg, 'ValleAR', seed=1), ar_cfg))
    nar = get_model_class('ValleNAR')(nar_cfg)
    nar.load_state_dict(synth.make_state_dict(nar_cfg, 'ValleNAR', seed=2))
    ar, nar = ar.to(DEV).eval(), nar.to(DEV).eval()
    gen = g(5)
    prompt = torch.randint(0, 1024, (8, 9), generator=gen).to(DEV)
    pt, tt = torch.randint(0, 256, (5,), generator=gen).to(DEV), torch.randint(0, 256, (7,), generator=gen).to(DEV)
    codes, wave = CIO.synthesize(ar, nar, pt, prompt, tt, codec=dec, greedy_nar=True)
    assert codes.is_cuda and wave.is_cuda and wave.dtype == torch.float32
    assert tuple(wave.shape) == (320 * codes.shape[1],) and torch.isfinite(wave).all()
    assert torch.equal(wave, dec.decode(codes))
    assert not hasattr(dec, 'encode')                                             # prompts come as codes: no encode, no stub
