"""The fast decode chain at d_model 640 / 768 / 896 (10, 12 and 14 heads of width 64), the parts that need no GPU: the CPU
oracle against the real reference's tokens and margins (tests/golden/base_d_model.npz, gen_golden_base_d_model.py), the
Python gates, the library's argument checks through ctypes (made-up aligned pointers: nothing is dereferenced) and the
register / scratch figures of the new instantiations."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

from tests.golden import cases
from tests.golden.gen_golden_base_d_model import BASE, MIN_MARGIN, PERF_MARGIN, base_d_model_inputs
from tests.oracle_runners import load_golden
from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


@pytest.mark.parametrize('d', [640, 768, 896])
def test_folded_width_gains_the_three_widths(d):
    from valle2_amd.engine import cached_decode_supported, ffn_fused_width, folded_width
    assert folded_width(d) is True and ffn_fused_width(d) is True
    cfg = cases.cfg_of(dict(d_model=d, n_heads=d // 64, dim_feedforward=4 * d, num_layers=1, dropout=0.0, use_kv_cache=True))
    assert cached_decode_supported(cfg) is True


@pytest.mark.parametrize('d,expected', [(128, True), (1024, True), (1280, True), (1536, True), (1792, True), (2048, True),
                                        (2560, True), (3072, True), (3584, True), (4096, True), (384, False), (1088, False),
                                        (1152, False), (2304, False), (2816, False), (3328, False), (3840, False),
                                        (4352, False), (4608, False), (192, False), (320, False), (704, False), (832, False),
                                        (960, False)])
def test_folded_width_is_unchanged_elsewhere(d, expected):
    from valle2_amd.engine import folded_width
    assert folded_width(d) is expected


@pytest.mark.parametrize('which', sorted(BASE))
def test_oracle_generate_matches_the_real_reference(which):
    from oracle import valle_oracle as O
    gold = load_golden('base_d_model')
    kw, sd, utt = base_d_model_inputs(which)
    cfg = cases.cfg_of(kw)
    assert cfg.d_model == 64 * cfg.n_heads and cfg.d_model in (640, 768)
    trace = {}
    tokens = O.ar_generate(sd, cfg, *utt, trace=trace)
    assert torch.equal(tokens, gold[f'tokens_{which}'])
    assert len(trace['margin']) == int(gold[f'steps_{which}']) == kw['max_audio_len']
    torch.testing.assert_close(torch.tensor(trace['margin']), gold[f'margin_{which}'], atol=2e-5, rtol=2e-5)


@pytest.mark.parametrize('which', sorted(BASE))
def test_fixture_margins_are_ten_times_the_logit_tolerance(which):
    gold = load_golden('base_d_model')
    assert float(gold[f'margin_{which}'].min()) >= MIN_MARGIN == 10 * 2e-4
    assert int(gold[f'steps_{which}']) == BASE[which]['max_audio_len'] == gold[f'margin_{which}'].numel()
    assert BASE['d640']['dim_feedforward'] % 16 == 0 and BASE['d640']['dim_feedforward'] % 32 != 0


def test_d768_margins_leave_three_quarters_of_the_steps_to_the_perf_mode_test():
    gold = load_golden('base_d_model')
    assert PERF_MARGIN == 10 * 1.5e-2
    assert float((gold['margin_d768'] > PERF_MARGIN).float().mean()) >= 0.75


def test_version_is_133(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    declared = int(re.search(r'#define VH_VERSION (\d+)', header).group(1))
    assert declared >= 133 and L.vh_version() == declared
    assert 'ABI 133' in (REPO / 'INTEGRATION.md').read_text()


@pytest.mark.parametrize('d', [640, 768, 896])
def test_ffn_decode_workspace_and_argument_checks(L, d):
    for M, dff in ((1, 4 * d), (19, 1296), (64, 4 * d)):
        assert L.vh_ffn_decode_ws_bytes(M, d, dff) == (dff // 16) * M * d * 4
    M, dff = 8, 1296
    need = L.vh_ffn_decode_ws_bytes(M, d, dff)

    def call(M=M, dff=dff, ws=P2, nbytes=need, ldx=d, w2=P):
        return L.vh_ffn_decode(P, ldx, P, P, P, w2, P, P, d, M, d, dff, 1e-5, ws, nbytes, None)
    assert call(nbytes=need - 1) < 0 and 'workspace' in _err(L)
    assert call(M=65) < 0 and 'd_model' in _err(L)
    assert call(dff=1304) < 0 and 'd_model' in _err(L)          # dff % 16 != 0
    assert call(ldx=d - 4) < 0 and 'ldx' in _err(L)
    assert call(w2=None) < 0 and 'null pointer' in _err(L)
    assert call(w2=P + 4) < 0 and '16-byte aligned' in _err(L)
    # the widths that stay out, with the new set in the message
    assert L.vh_ffn_decode(P, 192, P, P, P, P, P, P, 192, M, 192, 768, 1e-5, P2, 1 << 24, None) < 0
    assert 'd_model' in _err(L) and '640,768,896' in _err(L)


def test_folded_refusals_name_the_new_set(L):
    assert L.vh_linear_folded(P, 384, P, P, P, None, 0, P, 64, 4, 64, 384, 0, 1e-5, None) < 0
    assert 'folded LayerNorm' in _err(L) and '640,768,896' in _err(L)
    assert L.vh_linear_folded(P, 768, P, P, P, None, 0, P, 64, 65, 64, 768, 0, 1e-5, None) < 0      # M = 65
    assert 'folded LayerNorm' in _err(L)
    assert L.vh_linear_folded(P, 768, P, P, P, None, 0, P, 72, 4, 72, 768, 0, 1e-5, None) < 0       # N % 16 != 0
    assert 'folded LayerNorm' in _err(L)


# ---- decoder_check through vh_ar_decoder_create on host-only descriptors: 768 / 12 heads reaches the verdicts of 512 / 8 ----
def _desc(d_model, folded=True, prefix=False, w1=True, **kw):
    h = d_model // 64
    layers = (_lib.VhLayer * 2)()
    for lay in layers:
        if folded:
            lay.wqkv_f = lay.qkv_c1 = lay.qkv_c2 = P
            if w1:
                lay.w1_f = lay.w1_c1 = lay.w1_c2 = P
        if prefix:
            lay.kprefix = lay.vprefix = P
    d = _lib.VhArDecoderDesc(B=4, d_model=d_model, n_heads=h, dff=4 * d_model, n_layers=2, S_max=64, V=1025, eos=1024, n_split=1,
                             ln_eps=1e-5, layers=layers, proj_w=P, audio_emb=P, audio_pe=P, x=P, q=P, attn=P, hidden=P,
                             logits=P, cache_len=I32, audio_pos=I32, eos_count=I32, codes=P, codes_stride=80, top_k=1,
                             temperature=1.0, kv_bf16=1)
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = layers
    return d


def _create(L, d):
    L.vh_ar_decoder_create.restype = C.c_void_p
    h = L.vh_ar_decoder_create(C.byref(d))
    if h:
        L.vh_ar_decoder_destroy.argtypes = [C.c_void_p]
        L.vh_ar_decoder_destroy(h)
    return bool(h), _err(L)


def _strip(msg):
    return re.sub(r'\d+', '#', msg)


def test_decoder_check_reaches_the_same_verdicts_at_768_as_at_512(L):
    def verdicts(d):
        h = d // 64
        out = []
        out.append(_create(L, _desc(d)))                                                   # kv_bf16, one split
        out.append(_create(L, _desc(d, folded=False)))                                     # ... needs folded weights
        need = L.vh_attn_decode_ws_bytes(4, h, 4)
        out.append(_create(L, _desc(d, n_split=4, attn_partial=P2, attn_partial_bytes=need)))
        out.append(_create(L, _desc(d, n_split=4, attn_partial=P2, attn_partial_bytes=need - 1)))
        out.append(_create(L, _desc(d, folded=False, n_split=4, attn_partial=P2, attn_partial_bytes=need)))
        need = L.vh_attn_decode_shared_ws_bytes(4, h, 100, 2)
        kw = dict(prefix=True, n_split=2, prefix_len=100, prefix_S=128, attn_partial=P2)
        out.append(_create(L, _desc(d, attn_partial_bytes=need, **kw)))
        out.append(_create(L, _desc(d, attn_partial_bytes=need - 1, **kw)))
        out.append(_create(L, _desc(d, attn_partial_bytes=need, **dict(kw, prefix=False))))
        out.append(_create(L, _desc(d, folded=False, attn_partial_bytes=need, **kw)))
        ffn = L.vh_ffn_decode_ws_bytes(4, d, 4 * d)
        assert ffn > 0
        out.append(_create(L, _desc(d, ffn_ws=P2, ffn_ws_bytes=ffn)))
        out.append(_create(L, _desc(d, ffn_ws=P2, ffn_ws_bytes=ffn - 1)))
        out.append(_create(L, _desc(d, w1=False, ffn_ws=P2, ffn_ws_bytes=ffn)))
        out.append(_create(L, _desc(d, kv_bf16=0, ffn_ws=P2, ffn_ws_bytes=ffn)))
        return out
    at512, at768 = verdicts(512), verdicts(768)
    assert [ok for ok, _ in at512] == [True, False, True, False, False, True, False, False, False, True, False, False, True]
    for (ok_a, msg_a), (ok_b, msg_b) in zip(at512, at768):
        assert ok_a == ok_b and (ok_a or _strip(msg_a) == _strip(msg_b)), (msg_a, msg_b)


def test_python_gates_keep_the_old_widths():
    """VALLE2_HEAD_FUSED and VALLE2_DECODE_W16 have no kernels at the new widths: their gates (queries of the library's dispatch
    plan) are false there and true at the old four."""
    from valle2_amd import engine
    for d in (640, 768, 896):
        assert engine.head_fused_shape(8, 1025, d) is False and engine.w16_width(d) is False
    for d in (128, 256, 512, 1024):
        assert engine.head_fused_shape(8, 1025, d) is True and engine.head_fused_shape(64, 1025, d) is True and engine.w16_width(d) is True
        assert engine.head_fused_shape(65, 1025, d) is False
    assert engine.BASE_FOLD_WIDTHS == (640, 768, 896)


def test_base_folded_kernels_compile_without_scratch_within_their_registers():
    sys.path.insert(0, str(REPO / 'tools'))
    import check_isa
    problems = check_isa.check_base_folded(check_isa.compile_asm() + check_isa.compile_ffn_asm())
    assert not problems, problems
