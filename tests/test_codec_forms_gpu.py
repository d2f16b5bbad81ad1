"""Every compiled form and every tile edge of the codec's kernels (csrc/codec.hip), at the kernels: the shapes that the two
architectures of tests/test_codec_gpu.py and tests/test_codec_enc_gpu.py never launch.  Operands in torch layout, every
comparison against the float64 mirror functions under the rules of tests/codec_rules.py (8 e_ref for activations, the decided-row
rule for codes, torch.equal for every bit claim); every test prints its figures before it asserts.

  * `vh_conv1d_causal`: C_in with a partial 32-channel chunk after a full one (36, 40, 68, 132), C_out with a partial last
    column tile at NT = 1 / 2 / 4 (4, 36, 68, 100) and a second, partial tile (132), batch-row boundaries inside and just after a
    128-row tile, bias = None; `lens` with `len_scale` 1, 2, 5 on utterances at or under the padding.
  * `vh_conv1d_down`: the same edges for the strided form, ratio 1 (taps 2, stride 1), 129 output frames, ragged batches.
  * `vh_conv1d_wave`: C_out / 4 that does not divide 256 (a row's lanes straddle workgroups), taps 1, 2 and 64.
  * `vh_lstm_layer`: lstm_step_kernel<1 .. 4> with full and nearly empty last slices, a recurrence of 256 steps, bits
    independent of B.
  * `vh_rvq_encode`: rvq_encode_kernel<4 / 8 / 16>, K = 1, 2, 33, 100, 1000 (a partial chunk after full ones), D with a
    zero-filled h = 1 half (4, 12, 36, 60, 100); ties at D = 64 and 100; NaN / inf rows at D = 64.
  * `vh_rvq_decode`: K = 33, D = 100 and K = 1, D = 4, bit-equal to fp32 torch adding in codebook order; and the decode of every
    encode case's codes.

One check differs from its first wording.  "x - decode(encode(x)) is no longer than x, row by row" is not a property of the
quantiser on N(0, 1) rows against N(0, 1) codebooks: the FLOAT64 mirror's own residual is longer than x on 70 / 70, 201 / 201
and 129 / 129 rows at (K, D) = (100, 64), (1000, 100), (96, 60), since no entry of |e|^2 ~ D reaches 2 r.e >= |e|^2.  It is held
where it is true — the shrinking codebooks of tests/test_codec_enc_gpu.py at those three shapes, where the codes also equal the
planted ones — and on the N(0, 1) cases the decode of the kernel's codes is held to bit equality with fp32 torch instead.

Measured on an MI355X, 81 tests in 3.7 s.  Worst error / e_ref: 2.28 over the 375 stride-1 convolution
comparisons (132 -> 4, taps 3, dilation 2, T = 129, no bias; e_ref 1.1e-7 .. 2.5e-6), 2.07 over the 72 `lens` comparisons
(32 -> 16, taps 3, dilation 4, len_scale 1, the utterance of one row), 2.20 over the 70 `vh_conv1d_down` comparisons (36 -> 68,
r = 3, L = 7) and 1.21 over the 48 ragged ones, 3.00 over the 132 `vh_conv1d_wave` comparisons (taps 1, C_out 36, L = 33) and
1.11 / 0.92 / 0.95 / 1.00 / 1.00 / 1.00 for the LSTM at (H, T) = (36, 3) / (260, 3) / (768, 3) / (772, 2) / (1024, 3) / (512, 256).
Codes: in all 10 `codes_rule` calls 0 undecided rows, 0 rows that differ from the float64 mirror and a worst gap / e_score
of 0 (e_score 1.4e-6 .. 7.4e-5 against smallest margins of 1.1e-3 .. 0.35); the shrinking codebooks leave 4.4e-5 .. 4.9e-5 of
the worst row's norm."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import codec_enc_mirror as E
from tests import codec_mirror as M
from tests.codec_rules import DEV, codes_rule, g, within
from tests.test_codec_enc_gpu import down_case, down_lengths, run_down, run_rvq, rvq_case, wave_case
from tests.test_codec_gpu import conv_case

pytestmark = pytest.mark.gpu
DTYPES = (torch.float64, torch.float32)


def dev(t):
    return None if t is None else t.to(DEV)


def dev_lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


# ---- vh_conv1d_causal, stride 1 ------------------------------------------------------------------------------------------------
CONV_CHANNELS = [(36, 36), (68, 100), (40, 132), (8, 68), (132, 4)]
CONV_TAPS = [(7, 1), (3, 2), (1, 1)]
CONV_T = (1, 127, 129)                    # B = 2: a batch-row boundary inside a 128-row tile and just after one
LENS_CHANNELS = [(32, 16), (36, 68)]
LENS_TAPS = [(3, 1), (3, 4), (5, 3), (7, 1)]
LEN_SCALES = [1, 2, 5]


def run_conv(x, w, b, r, dil, mode, elu, lens=None, len_scale=1):
    """The kernel on torch-layout operands: x (B, C, T), w (C_out, C_in, K), b (C_out) or None, r (B, C_out, T) or None
    -> (B, C_out, T) on the CPU."""
    from valle2_amd import kernels as K
    out = K.conv1d_causal(x.transpose(1, 2).contiguous().to(DEV), w.permute(0, 2, 1).contiguous().to(DEV), dev(b),
                          None if r is None else r.transpose(1, 2).contiguous().to(DEV), dilation=dil,
                          pad_mode=K.PAD_REFLECT if mode == 'reflect' else K.PAD_ZERO, elu=elu, lens=dev_lens(lens),
                          len_scale=len_scale)
    return out.cpu().transpose(1, 2)


@pytest.mark.parametrize('c_in,c_out', CONV_CHANNELS)
@pytest.mark.parametrize('taps,dil', CONV_TAPS)
def test_conv1d_causal_partial_chunks_and_column_tiles(taps, dil, c_in, c_out):
    worst = 0.0
    for T in CONV_T:
        x, w, b, r = conv_case(2, T, c_in, c_out, taps, dil, 10 * T + taps)
        for mode, elu, res in itertools.product(('reflect', 'zeros'), (False, True), (False, True)):
            ref = [M.conv1d_causal(x.to(dt), w.to(dt), b.to(dt), dil, mode, elu, r.to(dt) if res else None) for dt in DTYPES]
            got = run_conv(x, w, b, r if res else None, dil, mode, elu)
            e_ref, err = within(f'conv K{taps} d{dil} {c_in}->{c_out} T{T} {mode} elu{int(elu)} res{int(res)}', got, *ref)
            worst = max(worst, err / e_ref)
    # bias = nullptr: the mirror with a zero bias (x, w, r of the last T)
    ref = [M.conv1d_causal(x.to(dt), w.to(dt), torch.zeros(c_out, dtype=dt), dil, 'reflect', True, r.to(dt)) for dt in DTYPES]
    e_ref, err = within(f'conv K{taps} d{dil} {c_in}->{c_out} T{T} no bias', run_conv(x, w, None, r, dil, 'reflect', True), *ref)
    print(f'worst ratio {max(worst, err / e_ref):.2f}')


@pytest.mark.parametrize('len_scale', LEN_SCALES)
@pytest.mark.parametrize('taps,dil', LENS_TAPS)
@pytest.mark.parametrize('c_in,c_out', LENS_CHANNELS)
def test_conv1d_causal_lens_times_len_scale_rows_equal_the_utterance_alone(c_in, c_out, taps, dil, len_scale):
    """B = 3 holding (7, 1, 2) x len_scale valid rows, NaN behind them: rows 1 and 2 are at or under the padding for most
    (taps, dilation), so their reflection is the small-input branch, reading zero beyond lens[b] * len_scale."""
    lens = (7, 1, 2)
    T = lens[0] * len_scale
    x, w, b, r = conv_case(3, T, c_in, c_out, taps, dil, 7 * T + dil)
    for i, n in enumerate(lens):
        x[i, :, n * len_scale:] = float('nan')
    got = run_conv(x, w, b, r, dil, 'reflect', True, lens=lens, len_scale=len_scale)
    worst = 0.0
    for i, n in enumerate(lens):
        rows = n * len_scale
        xi, ri = x[i:i + 1, :, :rows].contiguous(), r[i:i + 1, :, :rows].contiguous()
        alone = run_conv(xi, w, b, ri, dil, 'reflect', True)
        assert torch.isfinite(alone).all() and torch.equal(got[i:i + 1, :, :rows], alone), (i, rows)
        ref = [M.conv1d_causal(xi.to(dt), w.to(dt), b.to(dt), dil, 'reflect', True, ri.to(dt)) for dt in DTYPES]
        e_ref, err = within(f'lens K{taps} d{dil} {c_in}->{c_out} scale {len_scale} row {i} ({rows} rows)', got[i:i + 1, :, :rows], *ref)
        worst = max(worst, err / e_ref)
    assert torch.equal(got[0], run_conv(x, w, b, r, dil, 'reflect', True)[0])          # the full row: lens changes nothing
    print(f'worst ratio {worst:.2f}')


# ---- vh_conv1d_down ------------------------------------------------------------------------------------------------------------
DOWN = [(36, 68, 3), (68, 36, 2), (12, 132, 5), (40, 100, 1)]          # r = 1: taps 2, stride 1


@pytest.mark.parametrize('c_in,c_out,r', DOWN)
def test_conv1d_down_partial_chunks_column_tiles_and_ratio_one(c_in, c_out, r):
    worst = 0.0
    for L in sorted(set(down_lengths(r)) | {128 * r + 1}):              # 128 r + 1: 129 output frames, across a row tile
        x, w, b = down_case(2, L, c_in, c_out, r, 10 * L + r)
        for elu in (False, True):
            ref = [E.conv1d_down(x.to(dt), w.to(dt), b.to(dt), r, elu) for dt in DTYPES]
            got = run_down(x, w, b, r, elu)
            assert tuple(got.shape) == (2, c_out, -(-L // r))
            e_ref, err = within(f'down {c_in}->{c_out} r{r} L{L} elu{int(elu)}', got, *ref)
            worst = max(worst, err / e_ref)
    print(f'worst ratio {worst:.2f}')


@pytest.mark.parametrize('c_in,c_out,r', DOWN)
def test_conv1d_down_ragged_batch_equals_each_utterance_alone(c_in, c_out, r):
    """B = 3 with lens (L, 1, r + 1), NaN behind every utterance's own rows: torch.equal to the utterance alone, zeros after
    its own frames."""
    worst = 0.0
    for L in (2 * r + 1, 130):
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
                ref = [E.conv1d_down(x[i:i + 1, :, :n].to(dt), w.to(dt), b.to(dt), r, elu) for dt in DTYPES]
                e_ref, err = within(f'ragged down {c_in}->{c_out} r{r} L{L} row {i} ({n} rows) elu{int(elu)}', got[i:i + 1, :, :frames], *ref)
                worst = max(worst, err / e_ref)
    print(f'worst ratio {worst:.2f}')


# ---- vh_conv1d_wave ------------------------------------------------------------------------------------------------------------
WAVE_C_OUT = [12, 36, 100]                # C_out / 4 = 3, 9, 25 lanes per row: none divides 256
WAVE_TAPS = [1, 2, 64]


def run_wave(x, w, b, lens=None):
    from valle2_amd import kernels as K
    return K.conv1d_wave(x.to(DEV), w[:, 0].contiguous().to(DEV), dev(b), lens=dev_lens(lens)).cpu()          # (B, L, C_out)


def wave_ref(x, w, b):
    return [M.conv1d_causal(x.to(dt)[:, None], w.to(dt), b.to(dt)).transpose(1, 2) for dt in DTYPES]


@pytest.mark.parametrize('taps', WAVE_TAPS)
@pytest.mark.parametrize('c_out', WAVE_C_OUT)
def test_conv1d_wave_rows_that_straddle_workgroups_and_the_tap_range(c_out, taps):
    worst = 0.0
    for L in sorted({1, 2, taps - 1, taps, 33, 130} - {0}):
        x, w, b = wave_case(L, c_out, taps, 10 * L + taps)
        got = run_wave(x, w, b)
        assert tuple(got.shape) == (2, L, c_out)
        e_ref, err = within(f'wave K{taps} ->{c_out} L{L}', got, *wave_ref(x, w, b))
        worst = max(worst, err / e_ref)
        assert torch.equal(got[1:], run_wave(x[1:], w, b))                           # the bits it has alone
        # lens: batch row 1 holds n < L samples, NaN behind them — its first n rows are the utterance alone
        for n in sorted({1, max(1, L // 2), max(1, L - 1)}):
            if n == L:
                continue
            xr = x.clone()
            xr[1, n:] = float('nan')
            got = run_wave(xr, w, b, lens=[L, n])
            e_ref, err = within(f'wave K{taps} ->{c_out} L{L} lens {n}', got[1:, :n], *wave_ref(x[1:, :n], w, b))
            worst = max(worst, err / e_ref)
            assert torch.equal(got[1:, :n], run_wave(x[1:, :n].contiguous(), w, b)) and torch.equal(got[0], run_wave(x, w, b)[0])
    # bias = nullptr: the mirror with a zero bias (x, w of the last L)
    e_ref, err = within(f'wave K{taps} ->{c_out} L{L} no bias', run_wave(x, w, None), *wave_ref(x, w, torch.zeros(c_out)))
    print(f'worst ratio {max(worst, err / e_ref):.2f}')


# ---- vh_lstm_layer -------------------------------------------------------------------------------------------------------------
# (H, T, B): NI = 1; NI = 2 with a nearly empty second slice; NI = 3 full; NI = 4 with a nearly empty last slice; NI = 4 full;
# and a recurrence of 256 steps at the default width
LSTM = [(36, 3, 2), (260, 3, 2), (768, 3, 1), (772, 2, 2), (1024, 3, 2), (512, 256, 1)]


def lstm_case(H, T, B):
    x = torch.randn(B, T, H, generator=g(H + T + B))
    params = [[(2 * torch.rand(s, generator=g(100 * layer + i)) - 1) / H ** 0.5 for i, s in enumerate([(4 * H, H), (4 * H, H), (4 * H,), (4 * H,)])]
              for layer in range(2)]
    return x, params


def lstm_ref(x, params):
    ref = []
    for dt in DTYPES:
        h = x.to(dt).transpose(0, 1)
        for p in params:
            h = M.lstm_layer(h, *[t.to(dt) for t in p])
        ref.append((h + x.to(dt).transpose(0, 1)).transpose(0, 1))
    return ref


def run_lstm(x, params):
    """Two layers and the skip, as the decoder runs them: out = lstm(x) + x, (B, T, H) on the CPU."""
    from valle2_amd import kernels as K
    xd = x.contiguous().to(DEV)
    h = xd
    for layer, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        xproj = K.conv1d_causal(h, w_ih[:, None, :].contiguous().to(DEV), (b_ih.double() + b_hh.double()).float().to(DEV))
        h = K.lstm_layer(xproj, w_hh.to(DEV), skip=xd if layer == 1 else None)
    return h.cpu()


@pytest.mark.parametrize('H,T,B', LSTM)
def test_lstm_block_at_every_slice_count(H, T, B):
    x, params = lstm_case(H, T, B)
    within(f'lstm H{H} T{T} B{B}', run_lstm(x, params), *lstm_ref(x, params))


@pytest.mark.parametrize('H', [260, 1024])
def test_lstm_bits_do_not_depend_on_the_batch(H):
    x, params = lstm_case(H, 3, 3)
    assert torch.equal(run_lstm(x, params)[1:2], run_lstm(x[1:2], params))


# ---- vh_rvq_encode -------------------------------------------------------------------------------------------------------------
# (B, T, K, D, Q, n_books): K = 33 and 100 end in a partial 32-entry chunk, K = 1 and 2 are below one; D = 36 .. 64 selects
# rvq_encode_kernel<8>; D = 4, 12, 36, 60, 100 leave the h = 1 half of the last k-step zero-filled
RVQ = [(2, 35, 33, 36, 4, 4), (2, 35, 100, 64, 8, 8), (1, 130, 1, 4, 2, 2), (3, 67, 1000, 100, 8, 8), (2, 35, 64, 12, 4, 4),
       (2, 35, 2, 48, 4, 4), (1, 129, 96, 60, 8, 8)]
# lo, hi: the same column in another chunk, another column of the same chunk, both; the last of each list ends at K - 1, which
# at K = 100 lies in the partial last chunk (96 .. 99) — (66, 98) the same column there, (10, 99) another
TIES = {(100, 64): [(3, 35), (5, 9), (0, 64), (31, 33), (66, 98), (10, 99)],
        (96, 100): [(3, 35), (5, 9), (0, 64), (31, 33), (2, 66), (10, 95)]}


def fp32_decode(codes, books):
    """fp32 torch adding in codebook order from a scalar 0.0: (B, Q, T) -> (B, T, D)."""
    want = torch.full((), 0.0)
    for q in range(codes.shape[1]):
        want = want + F.embedding(codes[:, q], books[q])
    return want


def run_rvq_decode(codes, books):
    from valle2_amd import kernels as K
    return K.rvq_decode(codes.to(DEV), books.to(DEV)).cpu()


@pytest.mark.parametrize('B,T,Kc,D,Q,n_books', RVQ)
def test_rvq_encode_partial_chunks_and_zero_filled_halves(B, T, Kc, D, Q, n_books):
    x, books = rvq_case(B, T, Kc, D, n_books, 3)
    got = run_rvq(x, books, Q)
    assert tuple(got.shape) == (B, Q, T)
    x64 = x.double().reshape(B * T, D)
    codes_rule(f'rvq {B}x{T} K{Kc} D{D} Q{Q}/{n_books}', got.transpose(0, 1).reshape(Q, B * T), books.double(), x64, x.reshape(B * T, D))
    if Kc == 1:
        assert (got == 0).all()
    # a row's codes depend on that row alone: another batch shape, single rows, a short prefix of the stages
    assert torch.equal(run_rvq(x.reshape(1, B * T, D), books, Q)[0], got.transpose(0, 1).reshape(Q, B * T))
    for b, t in ((0, 0), (B - 1, T - 1), (0, T // 2)):
        assert torch.equal(run_rvq(x[b:b + 1, t:t + 1], books, Q)[0, :, 0], got[b, :, t])
    assert torch.equal(run_rvq(x, books, 1)[:, 0], got[:, 0])
    # and vh_rvq_decode of these codes, at this K and D: the bits of fp32 torch adding in codebook order
    assert torch.equal(run_rvq_decode(got, books), fp32_decode(got, books))


@pytest.mark.parametrize('Kc,D', sorted(TIES))
def test_rvq_encode_picks_the_lower_index_of_duplicated_entries(Kc, D):
    B, T, n_books = 2, 35, 2
    pairs = TIES[Kc, D]
    x, books = rvq_case(B, T, Kc, D, n_books, 5)
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


def test_rvq_encode_gives_a_nan_row_ids_inside_the_codebook_and_leaves_the_others_at_d64():
    B, T, Kc, D, n_books = 2, 35, 100, 64, 8
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


# ---- vh_rvq_decode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('short', [0, 1])
@pytest.mark.parametrize('B,T,n_books,Kc,D', [(2, 130, 4, 33, 100), (1, 1, 2, 1, 4)])
def test_rvq_decode_is_bit_equal_to_fp32_torch_adding_in_codebook_order(B, T, n_books, Kc, D, short):
    Q = n_books - short
    books = torch.randn(n_books, Kc, D, generator=g(1))
    codes = torch.randint(0, Kc, (B, Q, T), generator=g(2))
    got = run_rvq_decode(codes, books)
    assert tuple(got.shape) == (B, T, D) and torch.equal(got, fp32_decode(codes, books))


@pytest.mark.parametrize('B,T,Kc,D,Q', [(2, 35, 100, 64, 8), (3, 67, 1000, 100, 8), (1, 129, 96, 60, 8)])
def test_rvq_decode_of_the_codes_leaves_a_residual_no_larger_than_the_input(B, T, Kc, D, Q):
    """The K >= 96 shapes of RVQ on codebooks that shrink by half per stage, x = one entry per stage plus noise of 1 %: the
    encoder finds those entries, and x - vh_rvq_decode(codes) is no longer than x, row by row (module docstring: on N(0, 1)
    rows the float64 quantiser itself does not shrink a row)."""
    books = torch.randn(Q, Kc, D, generator=g(8)) * 0.5 ** torch.arange(Q, dtype=torch.float32)[:, None, None]
    truth = torch.randint(0, Kc, (B, Q, T), generator=g(9))
    x = sum(books[q][truth[:, q]] for q in range(Q))
    x = x + 0.01 * 0.5 ** Q * torch.randn(x.shape, generator=g(10))
    got = run_rvq(x, books)
    assert torch.equal(got, truth)
    left = x - run_rvq_decode(got, books)
    ratio = (left.norm(dim=-1) / x.norm(dim=-1)).max().item()
    print(f'residual / input norm, worst row: {ratio:.3e}')
    assert (left.norm(dim=-1) <= x.norm(dim=-1)).all()
    codes_rule(f'shrinking books K{Kc} D{D}', got.transpose(0, 1).reshape(Q, B * T), books.double(), x.double().reshape(B * T, D),
               x.reshape(B * T, D))
