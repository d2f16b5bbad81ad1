"""What the codec's device tests share: the two rules every comparison is held to, the seeded state dict of both halves, the
three architectures beside the default config and the SMALL fixture, and a restatement of the dispatch rules of csrc/codec.hip.

Activations: e_ref = max |mirror_fp32 - mirror_fp64| on the comparison's own inputs, and the kernels stay within FACTOR e_ref of
the float64 mirror (`within`).  Codes: e_score is the largest |score_fp32 - score_fp64| of the mirror on the test's inputs; a
row is DECIDED when its smallest float64 margin exceeds CODE_FACTOR e_score; on decided rows the codes equal the float64
mirror's, on every row the chosen entry is within CODE_FACTOR e_score of the float64 maximum, and at most 5 % of a test's rows
are undecided — a condition on the inputs (`codes_rule`).  Both print their figures before they assert."""
import torch

from tests import codec_enc_mirror as E
from tests import codec_mirror as M

DEV = 'cuda'
FACTOR = 8
CODE_FACTOR = 16

# hop 4, LSTM width 64, dilations 1, 2, 4 (up to 8 rows of padding at len_scale 2 and 4), D = 64: rvq_encode_kernel<8>
DEEP = dict(num_filters=16, upsampling_ratios=(2, 2), hidden_size=64, codebook_size=128, num_residual_layers=3, compress=4)
# hop 6 with a ratio of 1, 5-tap residual convolutions of dilation growth 3, one LSTM layer, D = 36
TAPS = dict(num_filters=8, upsampling_ratios=(3, 1, 2), hidden_size=36, codebook_size=32, num_residual_layers=1, kernel_size=5,
            last_kernel_size=3, residual_kernel_size=5, dilation_growth_rate=3, num_lstm_layers=1)
# no residual blocks, three LSTM layers, D = 12
FLAT = dict(num_filters=16, upsampling_ratios=(4,), hidden_size=12, codebook_size=64, num_residual_layers=0, num_lstm_layers=3)
CONFIGS = {'deep': DEEP, 'taps': TAPS, 'flat': FLAT}
HOPS = {'deep': 4, 'taps': 6, 'flat': 4}


def g(seed):
    return torch.Generator().manual_seed(seed)


def within(name, got, ref64, ref32):
    """max |got - ref64| <= FACTOR * e_ref, e_ref = max |ref32 - ref64|; prints the figures first."""
    e_ref = (ref32.double() - ref64).abs().max().item()
    err = (got.double().cpu() - ref64).abs().max().item()
    print(f'{name}: e_ref={e_ref:.3e} gpu_err={err:.3e} ratio={err / e_ref if e_ref else float("inf"):.2f} max|ref|={ref64.abs().max().item():.3f}')
    assert torch.isfinite(got).all(), name
    assert err <= FACTOR * e_ref, f'{name}: |gpu - mirror64| = {err:.3e} > {FACTOR} x e_ref = {FACTOR * e_ref:.3e}'
    return e_ref, err


def codes_rule(name, got, books64, x64, x32):
    """got (Q, rows) int64 on the CPU against the float64 mirror of x64 (rows, D); x32 is the fp32 reference's input."""
    Q = got.shape[0]
    K = books64.shape[1]
    codes64, margin, e_score = E.rvq_scores(books64, x64, x32, Q)
    decided = margin > CODE_FACTOR * e_score
    assert got.dtype == torch.int64 and tuple(got.shape) == tuple(codes64.shape)
    assert int(got.min()) >= 0 and int(got.max()) < K
    gaps = E.chosen_gaps(books64, x64, got)
    differ = (got != codes64).any(0)
    print(f'{name}: rows={x64.shape[0]} e_score={e_score:.3e} undecided={int((~decided).sum())} differing rows={int(differ.sum())} '
          f'(decided among them {int((differ & decided).sum())}) min margin={margin.min().item():.3e} '
          f'worst gap / e_score={gaps.max().item() / e_score:.2f}')
    assert (~decided).double().mean().item() <= 0.05, f'{name}: {int((~decided).sum())} of {len(decided)} rows undecided'
    assert torch.equal(got[:, decided], codes64[:, decided]), f'{name}: codes differ on decided rows'
    assert gaps.max().item() <= CODE_FACTOR * e_score, f'{name}: a chosen entry is {gaps.max().item():.3e} below the best score'
    return e_score, gaps.max().item()


def codec_state_dict(seed, **over):
    """Both halves with the mirror's gains: the decoder's seeded state dict (and its codebooks) plus the encoder's."""
    sd = dict(M.random_state_dict(seed=seed, **over))
    sd.update({k: v for k, v in E.random_encoder_state_dict(seed=seed + 1, **over).items() if k.startswith('encoder.')})
    return sd


# ---- the dispatch rules of csrc/codec.hip, restated: which compiled form a shape selects -------------------------------------
def conv_form(c_out):
    """conv1d_causal_kernel<NT, DOWN>: 32 NT output columns per workgroup."""
    return 4 if c_out > 64 else 2 if c_out > 32 else 1


def lstm_form(H):
    """lstm_step_kernel<NI>: 256-wide slices of h per wave."""
    return -(-H // 256)


def rvq_form(D):
    """rvq_encode_kernel<NS>: 8-channel k-steps."""
    return 4 if D <= 32 else 8 if D <= 64 else 16
