"""KV-cached generation at head widths other than 64, the parts that need no GPU: which configurations the cached decoder
takes (`engine.cached_decode_supported`, the rule of plan.hip's decoder_check) and the CPU oracle against the real
reference's greedy tokens at head widths 128 and 48 (tests/golden/head_dim_decode.npz, gen_golden_head_dim_decode.py)."""
import pytest
import torch

from tests.golden import cases as C
from tests.golden.gen_golden_head_dim_decode import HD_DECODE, head_dim_decode_inputs
from tests.oracle_runners import load_golden


@pytest.mark.parametrize('d,h,use_kv_cache,expected', [
    (128, 4, True, True),        # width 32
    (192, 4, True, True),        # width 48
    (256, 2, True, True),        # width 128
    (512, 2, True, True),        # width 256
    (256, 8, True, True),        # width 32, more heads
    (64, 4, True, True),         # width 16, the narrowest served
    (64, 8, True, False),        # width 8
    (520, 2, True, False),       # width 260
    (64, 32, True, False),       # width 2
    (192, 4, False, False),      # use_kv_cache=False recomputes at every width
    (1536, 16, True, False),     # width 96 at d_model 1536 > 1024
    (96, 2, True, True),         # width 48 at d_model 96
    (100, 2, True, False),       # width 50: not a multiple of 4
    (200, 5, True, False),       # width 40 but d_model % 16 != 0
])
def test_cached_decode_supported_table(d, h, use_kv_cache, expected):
    from valle2_amd.engine import cached_decode_supported
    cfg = C.cfg_of(dict(d_model=d, n_heads=h, dim_feedforward=2 * d, num_layers=1, dropout=0.0, use_kv_cache=use_kv_cache))
    assert cached_decode_supported(cfg) is expected


@pytest.mark.parametrize('d,h', [(512, 8), (1024, 16), (64, 1), (1536, 24), (4096, 64)])
@pytest.mark.parametrize('use_kv_cache', [True, False])
def test_cached_decode_supported_width_64_is_use_kv_cache(d, h, use_kv_cache):
    """Width 64 routes as it always did: the cached decoder exactly when config.use_kv_cache (d_model is not consulted)."""
    from valle2_amd.engine import cached_decode_supported
    cfg = C.cfg_of(dict(d_model=d, n_heads=h, dim_feedforward=2 * d, num_layers=1, dropout=0.0, use_kv_cache=use_kv_cache))
    assert cached_decode_supported(cfg) is use_kv_cache


@pytest.mark.parametrize('which', sorted(HD_DECODE))
def test_oracle_generate_matches_the_real_reference_at_head_width(which):
    from oracle import valle_oracle as O
    gold = load_golden('head_dim_decode')
    kw, sd, utt = head_dim_decode_inputs(which)
    cfg = C.cfg_of(kw)
    assert cfg.d_model // cfg.n_heads in (48, 128)
    trace = {}
    tokens = O.ar_generate(sd, cfg, *utt, trace=trace)
    assert torch.equal(tokens, gold[f'tokens_{which}'])
    assert len(trace['margin']) == int(gold[f'steps_{which}'])
    torch.testing.assert_close(torch.tensor(trace['margin']), gold[f'margin_{which}'], atol=2e-5, rtol=2e-5)
