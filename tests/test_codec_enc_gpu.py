"""The EnCodec encoder's kernels (`vh_conv1d_wave`, `vh_conv1d_down`, `vh_rvq_encode`), `valle2_amd.EncodecEncoder` and
`valle2_amd.EncodecCodec` on the device, every comparison against the float64 mirror (tests/codec_enc_mirror.py).

Activations, the project's rule: e_ref = max |mirror_fp32 - mirror_fp64| on the comparison's own inputs, and the kernels stay
within 8 e_ref of the float64 mirror.  Every test prints its figures before it asserts.

Codes are integers and have their own rule.  e_score is the largest |score_fp32 - score_fp64| of the mirror on the test's
inputs (score = 2 r.e - |e|^2, both sides walking the float64 codes); a row is DECIDED when its smallest float64 margin between
the best and the second-best score, over all stages, exceeds 16 e_score (8 e_score on each of the two competing scores).
  * on every decided row the kernel's codes equal the float64 mirror's;
  * on EVERY row and stage the chosen entry's float64 score is within 16 e_score of the float64 maximum, the float64 residual
    rebuilt from the kernel's own earlier codes;
  * at most 5 % of a test's rows are undecided — a condition on the inputs (seeds are fixed so that the mirror alone meets it).

Measured on an MI355X.  Worst error / e_ref: 1.41 over the `vh_conv1d_wave` cases, 2.61 over the
`vh_conv1d_down` cases (1.70 on the ragged ones), 0.85 / 0.61 / 0.69 / 0.54 / 0.85 / 0.45 for `embed` on the small fixture at
L = 1 / 5 / 8 / 9 / 67 / 72 and 2.08 / 1.69 at the default config for L = 960 / 967.  Codes: in every test 0 undecided rows, 0 rows
that differ from the float64 mirror and a worst gap of 0 (e_score 4.4e-6 .. 1.2e-4 against smallest margins of 1.4e-3 .. 0.21)."""
import numpy as np
import pytest
import torch

from tests import codec_enc_mirror as E
from tests import codec_mirror as M
from tests.codec_rules import DEV, codec_state_dict, codes_rule, g, within
from tests.golden.gen_codec_golden import SMALL

pytestmark = pytest.mark.gpu
GOLDEN = M.__file__.rsplit('/', 1)[0] + '/golden/codec_enc_small.npz'


# ---- vh_conv1d_wave --------------------------------------------------------------------------------------------------------
def wave_case(L, c_out, taps, seed):
    x = torch.randn(2, L, generator=g(seed))
    w = torch.randn(c_out, 1, taps, generator=g(seed + 1)) / taps ** 0.5
    b = torch.randn(c_out, generator=g(seed + 2))
    return x, w, b


def run_wave(x, w, b, lens=None):
    from valle2_amd import kernels as K
    lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    return K.conv1d_wave(x.to(DEV), w[:, 0].contiguous().to(DEV), b.to(DEV), lens=lens).cpu()          # (B, L, C_out)


@pytest.mark.parametrize('taps', [3, 7])
@pytest.mark.parametrize('c_out', [4, 8, 32])
def test_conv1d_wave_against_the_float64_mirror(c_out, taps):
    worst = 0.0
    for L in sorted({1, 2, taps - 1, taps, 33, 130}):
        x, w, b = wave_case(L, c_out, taps, 10 * L + taps)
        ref = [M.conv1d_causal(x.to(dt)[:, None], w.to(dt), b.to(dt)).transpose(1, 2) for dt in (torch.float64, torch.float32)]
        got = run_wave(x, w, b)
        assert tuple(got.shape) == (2, L, c_out)
        e_ref, err = within(f'wave K{taps} ->{c_out} L{L}', got, *ref)
        worst = max(worst, err / e_ref)
        assert torch.equal(got[1:], run_wave(x[1:], w, b))                           # the bits it has alone
        # lens: batch row 1 holds n < L samples, NaN behind them — its first n rows are the utterance alone
        for n in sorted({1, max(1, L // 2), max(1, L - 1)}):
            if n == L:
                continue
            xr = x.clone()
            xr[1, n:] = float('nan')
            got = run_wave(xr, w, b, lens=[L, n])
            alone = [M.conv1d_causal(x[1:, None, :n].to(dt), w.to(dt), b.to(dt)).transpose(1, 2) for dt in (torch.float64, torch.float32)]
            e_ref, err = within(f'wave K{taps} ->{c_out} L{L} lens {n}', got[1:, :n], *alone)
            worst = max(worst, err / e_ref)
            assert torch.equal(got[1:, :n], run_wave(x[1:, :n].contiguous(), w, b)) and torch.equal(got[0], run_wave(x, w, b)[0])
    print(f'worst ratio {worst:.2f}')


# ---- vh_conv1d_down --------------------------------------------------------------------------------------------------------
DOWN = [(32, 64, 2), (8, 16, 4), (64, 128, 5), (16, 32, 8)]


def down_lengths(r):
    return sorted({1, 2, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, 33, 130} - {0})


def down_case(B, L, c_in, c_out, r, seed):
    x = torch.randn(B, c_in, L, generator=g(seed))
    w = torch.randn(c_out, c_in, 2 * r, generator=g(seed + 1)) / (c_in * 2 * r) ** 0.5
    b = torch.randn(c_out, generator=g(seed + 2))
    return x, w, b


def run_down(x, w, b, r, elu, lens=None):
    """The kernel on torch-layout operands: x (B, C, L), w (C_out, C_in, K) -> (B, C_out, ceil(L / r)) on the CPU."""
    from valle2_amd import kernels as K
    lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = K.conv1d_down(x.transpose(1, 2).contiguous().to(DEV), w.permute(0, 2, 1).contiguous().to(DEV), b.to(DEV), stride=r,
                        elu=elu, lens=lens)
    return out.cpu().transpose(1, 2)


@pytest.mark.parametrize('c_in,c_out,r', DOWN)
def test_conv1d_down_against_the_float64_mirror(c_in, c_out, r):
    worst = 0.0
    for L in down_lengths(r):
        x, w, b = down_case(2, L, c_in, c_out, r, 10 * L + r)
        for elu in (False, True):
            ref = [E.conv1d_down(x.to(dt), w.to(dt), b.to(dt), r, elu) for dt in (torch.float64, torch.float32)]
            got = run_down(x, w, b, r, elu)
            assert tuple(got.shape) == (2, c_out, -(-L // r))
            e_ref, err = within(f'down {c_in}->{c_out} r{r} L{L} elu{int(elu)}', got, *ref)
            worst = max(worst, err / e_ref)
    print(f'worst ratio {worst:.2f}')


@pytest.mark.parametrize('c_in,c_out,r', DOWN)
def test_conv1d_down_ragged_batch_equals_each_utterance_alone(c_in, c_out, r):
    """B = 3 with lens (L, 1, r + 1), NaN behind every utterance's own rows: torch.equal to the utterance alone, zeros after
    its own frames."""
    for L in (2 * r + 1, 33, 130):
        x, w, b = down_case(3, L, c_in, c_out, r, 7 * L + r)
        lens = (L, 1, r + 1)
        for i, n in enumerate(lens):
            x[i, :, n:] = float('nan')
        for elu in (False, True):
            got = run_down(x, w, b, r, elu, lens=lens)
            for i, n in enumerate(lens):
                frames = -(-n // r)
                alone = run_down(x[i:i + 1, :, :n].contiguous(), w, b, r, elu)
                assert torch.isfinite(alone).all() and torch.equal(got[i:i + 1, :, :frames], alone), (L, elu, i)
                assert (got[i, :, frames:] == 0).all()
                ref = [E.conv1d_down(x[i:i + 1, :, :n].to(dt), w.to(dt), b.to(dt), r, elu) for dt in (torch.float64, torch.float32)]
                within(f'ragged down r{r} L{L} row {i} ({n} rows) elu{int(elu)}', got[i:i + 1, :, :frames], *ref)


# ---- vh_rvq_encode ---------------------------------------------------------------------------------------------------------
RVQ = [(2, 35, 64, 32, 8, 8), (1, 130, 16, 8, 4, 4), (3, 67, 1024, 128, 8, 8), (2, 35, 64, 32, 3, 8)]      # the last: Q < n_books


def rvq_case(B, T, Kc, D, n_books, seed):
    return torch.randn(B, T, D, generator=g(seed)), torch.randn(n_books, Kc, D, generator=g(seed + 1))


def run_rvq(x, books, Q=None):
    """(B, T, D), (n_books, K, D) on the CPU -> codes (B, Q, T) on the CPU; |e|^2 as the encoder stores it."""
    from valle2_amd import kernels as K
    e_sq = books.double().pow(2).sum(-1).float()
    return K.rvq_encode(x.to(DEV), books.to(DEV), e_sq.to(DEV), Q).cpu()


@pytest.mark.parametrize('B,T,Kc,D,Q,n_books', RVQ)
def test_rvq_encode_against_the_float64_mirror(B, T, Kc, D, Q, n_books):
    x, books = rvq_case(B, T, Kc, D, n_books, 3)
    got = run_rvq(x, books, Q)
    assert tuple(got.shape) == (B, Q, T)
    x64 = x.double().reshape(B * T, D)
    codes_rule(f'rvq {B}x{T} K{Kc} D{D} Q{Q}/{n_books}', got.transpose(0, 1).reshape(Q, B * T), books.double(), x64, x.reshape(B * T, D))
    # a row's codes depend on that row alone: another batch shape, single rows, a short prefix of the stages
    assert torch.equal(run_rvq(x.reshape(1, B * T, D), books, Q)[0], got.transpose(0, 1).reshape(Q, B * T))
    for b, t in ((0, 0), (B - 1, T - 1), (0, T // 2)):
        assert torch.equal(run_rvq(x[b:b + 1, t:t + 1], books, Q)[0, :, 0], got[b, :, t])
    assert torch.equal(run_rvq(x, books, 1)[:, 0], got[:, 0])


def test_rvq_encode_picks_the_lower_index_of_duplicated_entries():
    B, T, Kc, D, n_books = 2, 35, 64, 32, 2
    x, books = rvq_case(B, T, Kc, D, n_books, 5)
    pairs = [(3, 35), (5, 9), (10, 63), (0, 32), (31, 33)]          # the same column in another chunk, another column, both
    for q in range(n_books):
        for lo, hi in pairs:
            books[q, hi] = books[q, lo]
    for i, (lo, hi) in enumerate(pairs):                            # rows whose nearest entry at both stages is a duplicate
        x[0, i] = books[0, lo] + books[1, pairs[(i + 1) % len(pairs)][0]] + 0.01 * x[0, i]
    got = run_rvq(x, books)
    for i, (lo, hi) in enumerate(pairs):
        assert got[0, 0, i].item() == lo and got[0, 1, i].item() == pairs[(i + 1) % len(pairs)][0], (i, got[0, :, i])
    his = torch.tensor([hi for _, hi in pairs])
    assert not torch.isin(got, his).any()                           # a duplicate's higher index is never chosen
    x64 = x.double().reshape(B * T, D)
    assert E.chosen_gaps(books.double(), x64, got.transpose(0, 1).reshape(n_books, B * T)).max().item() < 1e-3


def test_rvq_encode_gives_a_nan_row_ids_inside_the_codebook_and_leaves_the_others():
    B, T, Kc, D, n_books = 2, 35, 64, 32, 8
    x, books = rvq_case(B, T, Kc, D, n_books, 3)
    clean = run_rvq(x, books)
    x[0, 3] = float('nan')
    x[1, 34, 5] = float('inf')
    got = run_rvq(x, books)
    assert int(got.min()) >= 0 and int(got.max()) < Kc
    keep = torch.ones(B, T, dtype=torch.bool)
    keep[0, 3] = keep[1, 34] = False
    assert torch.equal(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])
    assert (got[0, :, 3] == 0).all()                                # no score of a NaN row beats the start: index 0


@pytest.mark.parametrize('B,T,Kc,D,Q', [(2, 35, 64, 32, 8), (3, 67, 1024, 128, 8)])
def test_rvq_decode_of_the_codes_leaves_a_residual_no_larger_than_the_input(B, T, Kc, D, Q):
    """x = a sum of one entry per stage of codebooks that shrink by half per stage, plus noise of 1 %: the encoder finds those
    entries, and x - vh_rvq_decode(codes) is no longer than x, row by row."""
    from valle2_amd import kernels as K
    books = torch.randn(Q, Kc, D, generator=g(8)) * 0.5 ** torch.arange(Q, dtype=torch.float32)[:, None, None]
    truth = torch.randint(0, Kc, (B, Q, T), generator=g(9))
    x = sum(books[q][truth[:, q]] for q in range(Q))
    x = x + 0.01 * 0.5 ** Q * torch.randn(x.shape, generator=g(10))
    got = run_rvq(x, books)
    assert torch.equal(got, truth)
    left = x - K.rvq_decode(got.to(DEV), books.to(DEV)).cpu()
    ratio = (left.norm(dim=-1) / x.norm(dim=-1)).max().item()
    print(f'residual / input norm, worst row: {ratio:.3e}')
    assert (left.norm(dim=-1) <= x.norm(dim=-1)).all()
    codes_rule(f'shrinking books K{Kc} D{D}', got.transpose(0, 1).reshape(Q, B * T), books.double(), x.double().reshape(B * T, D),
               x.reshape(B * T, D))


# ---- the whole encoder -----------------------------------------------------------------------------------------------------
LENGTHS = (1, 5, 8, 9, 67, 72)


@pytest.fixture(scope='module')
def small():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith('sd/')}


@pytest.fixture(scope='module')
def default():
    from valle2_amd import EncodecCodec
    sd = codec_state_dict(11)
    return sd, EncodecCodec.from_state_dict(sd)


@pytest.mark.parametrize('L', LENGTHS)
def test_encoder_on_the_small_fixture(small, L):
    from valle2_amd import EncodecEncoder
    sd, rec = small
    enc = EncodecEncoder.from_state_dict(sd, **SMALL)
    wave, emb64 = rec[f'wave/{L}'], rec[f'emb64/{L}']
    T = -(-L // 8)
    _, emb32 = E.encode(sd, wave, torch.float32, **SMALL)
    got = torch.stack([enc.embed(wave[b].to(DEV)) for b in range(2)])
    assert got.is_cuda and tuple(got.shape) == (2, T, 32) and got.dtype == torch.float32
    within(f'small fixture L{L} embed', got, emb64, emb32)
    codes = enc.batch_encode(wave.to(DEV))
    assert codes.is_cuda and tuple(codes.shape) == (2, 8, T) and codes.dtype == torch.int64
    codes_rule(f'small fixture L{L} codes', codes.cpu().transpose(0, 1).reshape(8, 2 * T), E.codebooks_of(sd),
               emb64.reshape(2 * T, 32), emb32.reshape(2 * T, 32))
    assert torch.equal(enc.encode(wave[1].to(DEV)), codes[1])
    assert torch.equal(enc.encode(wave[1].to(DEV), num_codebooks=3), codes[1, :3])
    assert torch.equal(enc.encode(wave[1].double().to(DEV)), codes[1])               # any floating dtype: converted to fp32


@pytest.mark.parametrize('L', [960, 967])
def test_encoder_at_the_default_config(default, L):
    sd, codec = default
    wave = 0.3 * torch.randn(2, L, generator=g(L))
    T = -(-L // 320)
    (codes64, emb64), (_, emb32) = E.encode(sd, wave), E.encode(sd, wave, torch.float32)
    got = torch.stack([codec.encoder.embed(wave[b].to(DEV)) for b in range(2)])
    assert tuple(got.shape) == (2, T, 128) and codec.sampling_rate == 24000 and codec.hop == 320
    within(f'default config L{L} embed', got, emb64, emb32)
    codes = codec.batch_encode(wave.to(DEV))
    assert tuple(codes.shape) == (2, 8, T)
    codes_rule(f'default config L{L} codes', codes.cpu().transpose(0, 1).reshape(8, 2 * T), E.codebooks_of(sd),
               emb64.reshape(2 * T, 128), emb32.reshape(2 * T, 128))
    assert torch.equal(codec.get_embedding(wave[0].to(DEV)), got[0].t())


def test_ragged_encode_many_equals_each_utterance_alone_bit_for_bit(small):
    from valle2_amd import EncodecEncoder
    sd, rec = small
    enc = EncodecEncoder.from_state_dict(sd, **SMALL)
    waves = [rec['wave/72'][0], rec['wave/1'][1], rec['wave/9'][0], rec['wave/67'][1]]
    waves = [w.to(DEV) for w in waves]
    many, embs = enc.encode_many(waves, return_embeddings=True)
    assert [tuple(c.shape) for c in many] == [(8, 9), (8, 1), (8, 2), (8, 9)]
    for c, e, w in zip(many, embs, waves):
        assert c.is_cuda and torch.equal(c, enc.encode(w)) and torch.equal(e, enc.embed(w))
    assert all(torch.equal(a, b) for a, b in zip(enc.encode_many(waves), many))
    assert all(torch.equal(a[:2], b) for a, b in zip(many, enc.encode_many(waves, num_codebooks=2)))
    assert enc.encode_many([]) == []


def test_codec_encode_decode_returns_hop_frames_of_finite_samples(default):
    _, codec = default
    for L in (1, 320, 967):
        wave = 0.3 * torch.randn(L, generator=g(L)).to(DEV)
        out = codec.encode_decode(wave)
        T = -(-L // 320)
        assert out.is_cuda and tuple(out.shape) == (320 * T,) and out.dtype == torch.float32 and torch.isfinite(out).all()
        assert torch.equal(out, codec.decode(codec.encode(wave)))


@pytest.fixture(scope='module')
def models():
    from valle2_amd import get_model_class, synth
    from valle2_amd.config import ConfigValle
    cfg = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0)
    ar_cfg = ConfigValle(**cfg, norm='LayerNorm', num_beams=2, top_k=1, max_audio_len=12)
    nar_cfg = ConfigValle(**cfg, norm='AdaptiveLayerNorm')
    ar = get_model_class('ValleAR')(ar_cfg)
    ar.load_state_dict(synth.silence_eos(synth.make_state_dict(ar_cfg, 'ValleAR', seed=1), ar_cfg))
    nar = get_model_class('ValleNAR')(nar_cfg)
    nar.load_state_dict(synth.make_state_dict(nar_cfg, 'ValleNAR', seed=2))
    return ar.to(DEV).eval(), nar.to(DEV).eval()


def test_codec_io_synthesize_takes_a_waveform_prompt(default, models):
    from valle2_amd import codec_io as CIO
    _, codec = default
    ar, nar = models
    gen = g(5)
    wave = (0.3 * torch.randn(9 * 320 - 7, generator=gen)).to(DEV)
    pt, tt = torch.randint(0, 256, (5,), generator=gen).to(DEV), torch.randint(0, 256, (7,), generator=gen).to(DEV)
    prompt = codec.encode(wave)
    assert tuple(prompt.shape) == (8, 9)
    codes, out = CIO.synthesize(ar, nar, pt, wave, tt, codec=codec, greedy_nar=True)
    codes2, out2 = CIO.synthesize(ar, nar, pt, prompt, tt, codec=codec, greedy_nar=True)
    assert codes.is_cuda and out.is_cuda and tuple(out.shape) == (320 * codes.shape[1],) and torch.isfinite(out).all()
    assert torch.equal(codes, codes2) and torch.equal(out, out2)


def test_codec_io_synthesize_many_encodes_waveform_prompts_in_one_call(default, models, monkeypatch):
    from valle2_amd import codec_io as CIO
    _, codec = default
    ar, nar = models
    gen = g(6)
    waves = [(0.3 * torch.randn(n, generator=gen)).to(DEV) for n in (9 * 320, 5 * 320 + 11)]
    texts = [(torch.randint(0, 256, (5,), generator=gen).to(DEV), torch.randint(0, 256, (7,), generator=gen).to(DEV)) for _ in waves]
    calls = {'many': 0, 'one': 0}
    encode_many, encode = codec.encode_many, codec.encode
    monkeypatch.setattr(codec, 'encode_many', lambda ws, *a: calls.__setitem__('many', calls['many'] + 1) or encode_many(ws, *a))
    monkeypatch.setattr(codec, 'encode', lambda w, *a: calls.__setitem__('one', calls['one'] + 1) or encode(w, *a))
    outs = CIO.synthesize_many(ar, nar, [(pt, w, tt) for (pt, tt), w in zip(texts, waves)], codec=codec, greedy_nar=True)
    assert calls == {'many': 1, 'one': 0}
    monkeypatch.undo()
    want = CIO.synthesize_many(ar, nar, [(pt, codec.encode(w), tt) for (pt, tt), w in zip(texts, waves)], codec=codec, greedy_nar=True)
    for (c, o), (c2, o2) in zip(outs, want):
        assert torch.equal(c, c2) and torch.equal(o, o2)
    # one waveform among codes: the single-utterance route
    mixed = CIO.synthesize_many(ar, nar, [(texts[0][0], waves[0], texts[0][1]), (texts[1][0], codec.encode(waves[1]), texts[1][1])],
                                codec=codec, greedy_nar=True)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(mixed, want))
