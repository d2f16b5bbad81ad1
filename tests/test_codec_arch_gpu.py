"""The whole codec (`valle2_amd.EncodecCodec`) on the device at three architectures beside the default config and the SMALL
fixture — `deep`, `taps` and `flat` of tests/codec_rules.py: every architecture field takes a value other than its default
somewhere (three residual layers of dilation 1, 2, 4 and compress 4; a ratio of 1, 5-tap kernels, dilation growth 3, one LSTM
layer; no residual layers and three LSTM layers; hidden sizes 64, 36, 12).  Seeded state dicts (decoder seed 21, encoder seed
22), every comparison against the float64 mirror under the rules of tests/codec_rules.py, every "equals the utterance alone"
with torch.equal.  tests/test_codec_arch_cpu.py pins the mirror to a live `transformers` model at these configs.

On `deep` the ragged decode runs the small-input reflection (lens * len_scale <= padding) inside both stages: padding up to 8
rows at len_scale 2 and 4, utterances of 1, 2 and 3 frames.

Measured on an MI355X, 33 tests in 3.1 s.  Worst error / e_ref, deep / taps / flat: `batch_decode` over
T = 1, 2, 3, 11: 0.96 / 1.74 / 2.52 (e_ref 1.1e-7 .. 7.9e-5); `decode_many` over T = 11, 1, 2, 3, 5: 2.52 / 1.79 / 0.94; `embed`
over the four lengths: 0.64 / 1.34 / 1.01 (e_ref 1.6e-8 .. 3.5e-6).  Codes: in all 12 `codes_rule` calls (3 .. 30 rows each) 0
undecided rows, 0 rows that differ from the float64 mirror and a worst gap / e_score of 0 (e_score 4.0e-6 .. 5.8e-5 against
smallest margins of 3.7e-3 .. 1.4)."""
import pytest
import torch

from tests import codec_enc_mirror as E
from tests import codec_mirror as M
from tests.codec_rules import CONFIGS, DEV, HOPS, codec_state_dict, codes_rule, g, within

pytestmark = pytest.mark.gpu
Q = 8


@pytest.fixture(scope='module', params=sorted(CONFIGS))
def arch(request):
    from valle2_amd import EncodecCodec
    name = request.param
    cfg = CONFIGS[name]
    sd = codec_state_dict(21, **cfg)
    codec = EncodecCodec.from_state_dict(sd, **cfg)
    assert codec.hop == HOPS[name] and codec.num_codebooks == Q
    return name, cfg, sd, codec


def random_codes(cfg, shape, seed):
    return torch.randint(0, cfg['codebook_size'], shape, generator=g(seed))


# ---- the decoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 3, 11])
def test_batch_decode_against_the_float64_mirror(arch, T):
    name, cfg, sd, codec = arch
    codes = random_codes(cfg, (2, Q, T), 30 + T)
    got = codec.batch_decode(codes.to(DEV))
    assert got.is_cuda and tuple(got.shape) == (2, codec.hop * T) and got.dtype == torch.float32
    within(f'{name} decode T{T}', got, M.decode(sd, codes, **cfg), M.decode(sd, codes, torch.float32, **cfg))
    assert torch.equal(codec.decode(codes[1].to(DEV)), got[1])


def test_ragged_decode_many_equals_each_utterance_alone(arch):
    name, cfg, sd, codec = arch
    items = [random_codes(cfg, (Q, T), 40 + T) for T in (11, 1, 2, 3, 5)]
    many = codec.decode_many([c.to(DEV) for c in items])
    assert [tuple(w.shape) for w in many] == [(codec.hop * c.shape[1],) for c in items]
    for w, c in zip(many, items):
        assert w.is_cuda and torch.equal(w, codec.decode(c.to(DEV)))
        within(f'{name} ragged decode T{c.shape[1]}', w[None], M.decode(sd, c[None], **cfg), M.decode(sd, c[None], torch.float32, **cfg))


# ---- the encoder -----------------------------------------------------------------------------------------------------------
def lengths(hop):
    return {'1': 1, 'hop-1': hop - 1, 'hop+1': hop + 1, '9hop+1': 9 * hop + 1}


@pytest.mark.parametrize('which', ['1', 'hop-1', 'hop+1', '9hop+1'])
def test_embed_and_batch_encode_against_the_float64_mirror(arch, which):
    name, cfg, sd, codec = arch
    L = lengths(codec.hop)[which]
    D = cfg['hidden_size']
    wave = 0.3 * torch.randn(3, L, generator=g(L))
    T = -(-L // codec.hop)
    (_, emb64), (_, emb32) = E.encode(sd, wave, **cfg), E.encode(sd, wave, torch.float32, **cfg)
    got = torch.stack([codec.encoder.embed(wave[b].to(DEV)) for b in range(3)])
    assert got.is_cuda and tuple(got.shape) == (3, T, D) and got.dtype == torch.float32
    within(f'{name} L{L} embed', got, emb64, emb32)
    codes = codec.batch_encode(wave.to(DEV))
    assert codes.is_cuda and tuple(codes.shape) == (3, Q, T) and codes.dtype == torch.int64
    codes_rule(f'{name} L{L} codes', codes.cpu().transpose(0, 1).reshape(Q, 3 * T), E.codebooks_of(sd), emb64.reshape(3 * T, D),
               emb32.reshape(3 * T, D))
    assert torch.equal(codec.encode(wave[1].to(DEV)), codes[1])
    assert torch.equal(codec.encode(wave[1].to(DEV), num_codebooks=2), codes[1, :2])
    assert torch.equal(codec.get_embedding(wave[0].to(DEV)), got[0].t())


def test_ragged_encode_many_equals_each_utterance_alone(arch):
    name, cfg, sd, codec = arch
    hop = codec.hop
    waves = [(0.3 * torch.randn(n, generator=g(50 + n))).to(DEV) for n in (9 * hop + 1, 1, hop + 1, hop - 1)]
    many, embs = codec.encoder.encode_many(waves, return_embeddings=True)
    assert [tuple(c.shape) for c in many] == [(Q, 10), (Q, 1), (Q, 2), (Q, 1)]
    for c, e, w in zip(many, embs, waves):
        assert c.is_cuda and torch.equal(c, codec.encode(w)) and torch.equal(e, codec.encoder.embed(w))
    assert all(torch.equal(a, b) for a, b in zip(codec.encode_many(waves), many))


# ---- both ------------------------------------------------------------------------------------------------------------------
def test_encode_decode_returns_hop_frames_of_finite_samples(arch):
    name, cfg, sd, codec = arch
    hop = codec.hop
    for L in (1, hop - 1, hop, 9 * hop + 1):
        wave = (0.3 * torch.randn(L, generator=g(60 + L))).to(DEV)
        out = codec.encode_decode(wave)
        T = -(-L // hop)
        assert out.is_cuda and tuple(out.shape) == (hop * T,) and out.dtype == torch.float32 and torch.isfinite(out).all()
        assert torch.equal(out, codec.decode(codec.encode(wave)))
