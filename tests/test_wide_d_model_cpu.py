"""KV-cached generation at d_model above 1024 (head width 64), the parts that need no GPU: the CPU oracle against the real
reference's greedy tokens and margins at d_model 1536 and 1152 (tests/golden/wide_d_model.npz, gen_golden_wide_d_model.py)
and where the cached decoder ends (`engine.cached_decode_supported`: d_model <= 4096, the rule of plan.hip's decoder_check)."""
import pytest
import torch

from tests.golden import cases as C
from tests.golden.gen_golden_wide_d_model import MIN_MARGIN, WIDE, wide_d_model_inputs
from tests.oracle_runners import load_golden


@pytest.mark.parametrize('which', sorted(WIDE))
def test_oracle_generate_matches_the_real_reference_at_wide_d_model(which):
    from oracle import valle_oracle as O
    gold = load_golden('wide_d_model')
    kw, sd, utt = wide_d_model_inputs(which)
    cfg = C.cfg_of(kw)
    assert cfg.d_model == 64 * cfg.n_heads and cfg.d_model > 1024
    trace = {}
    tokens = O.ar_generate(sd, cfg, *utt, trace=trace)
    assert torch.equal(tokens, gold[f'tokens_{which}'])
    assert len(trace['margin']) == int(gold[f'steps_{which}']) == kw['max_audio_len']
    torch.testing.assert_close(torch.tensor(trace['margin']), gold[f'margin_{which}'], atol=2e-5, rtol=2e-5)


@pytest.mark.parametrize('which', sorted(WIDE))
def test_fixture_margins_are_ten_times_the_logit_tolerance(which):
    """Every step of the reference is decided by at least 10 x 2e-4 (the GPU test's logit tolerance): no step is excused."""
    gold = load_golden('wide_d_model')
    assert float(gold[f'margin_{which}'].min()) >= MIN_MARGIN == 10 * 2e-4


@pytest.mark.parametrize('d,h,expected', [(4096, 64, True), (1152, 18, True), (1536, 24, True), (4160, 65, False),
                                          (8192, 128, False)])
def test_cached_decode_supported_ends_at_4096(d, h, expected):
    from valle2_amd.engine import cached_decode_supported
    cfg = C.cfg_of(dict(d_model=d, n_heads=h, dim_feedforward=2 * d, num_layers=1, dropout=0.0, use_kv_cache=True))
    assert cached_decode_supported(cfg) is expected


@pytest.mark.parametrize('d,expected', [(128, True), (1024, True), (1280, True), (1536, True), (1792, True), (2048, True),
                                        (2560, True), (3072, True), (3584, True), (4096, True), (384, False), (1088, False),
                                        (1152, False), (2304, False), (2816, False), (3328, False), (3840, False),
                                        (4352, False), (4608, False)])
def test_folded_width_set(d, expected):
    """256 x PW x passes with PW in 5..8 and one or two passes: above 2048 the odd multiples of 256 are not tiled."""
    from valle2_amd.engine import folded_width
    assert folded_width(d) is expected
    wide = {256 * pw * passes for pw in (5, 6, 7, 8) for passes in (1, 2)}
    assert folded_width(d) is (d in wide or d in (128, 256, 512, 1024))


def test_wide_folded_kernels_compile_without_scratch_within_128_registers():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))
    import check_isa
    problems = check_isa.check_wide_folded(check_isa.compile_asm())
    assert not problems, problems
