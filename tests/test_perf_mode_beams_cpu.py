"""Perf mode (the 16-bit K/V cache of the decode step) with key splits and with a shared prompt, the parts that need no GPU:
the two entry points are declared and exported, they and the decoder's descriptor check refuse what they must BEFORE any GPU
work (called through ctypes with made-up, aligned pointers: nothing is dereferenced on a refusal) and accept the descriptors
that used to be refused, and the new kernels' gfx950 code has no scratch and at most 256 vector registers."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced (every call is refused)
NEW = ('vh_attn_decode_kv16_split', 'vh_attn_decode_shared_kv16')


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


def test_header_declares_and_library_exports_the_two_entry_points(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, header), f'{name} is not declared in include/valle_hip.h'
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 131
    assert 'ABI 131' in (REPO / 'INTEGRATION.md').read_text()


def _split(L, q=P, k=P, v=P, out=P, cl=I32, len_bias=1, B=4, h=8, S_max=64, n_split=4, partial=P2, nbytes=None):
    if nbytes is None:
        nbytes = L.vh_attn_decode_ws_bytes(B, h, n_split)
    return L.vh_attn_decode_kv16_split(q, 64 * h, k, v, out, 64 * h, cl, len_bias, B, h, S_max, n_split, partial, nbytes, None)


@pytest.mark.parametrize('kw,text', [
    (dict(q=None), 'null pointer'), (dict(k=None), 'null pointer'), (dict(v=None), 'null pointer'),
    (dict(out=None), 'null pointer'), (dict(cl=None), 'null pointer'),
    (dict(n_split=0), 'n_split=0'), (dict(n_split=17), 'n_split=17'),
    (dict(partial=None), 'workspace'), (dict(nbytes=64), 'workspace'),
    (dict(len_bias=2), 'len_bias=2'), (dict(k=P + 2), '16-byte aligned'),
])
def test_kv16_split_refuses_before_any_gpu_work(L, kw, text):
    assert _split(L, **kw) < 0
    assert 'vh_attn_decode_kv16_split' in _err(L) and text in _err(L), _err(L)


def test_kv16_split_workspace_is_the_fp32_forms(L):
    """One byte short of vh_attn_decode_ws_bytes is refused for every split count served."""
    for B, h in ((4, 8), (1, 8), (8, 16), (3, 2)):
        for n_split in (2, 5, 8, 16):
            need = L.vh_attn_decode_ws_bytes(B, h, n_split)
            assert need >= B * h * n_split * 72 * 4
            assert _split(L, B=B, h=h, n_split=n_split, nbytes=need - 1) < 0
            assert 'workspace' in _err(L)


def _shared(L, q=P, kp=P, vp=P, prefix_len=100, prefix_S=128, ks=P, vs=P, out=P, sl=I32, len_bias=1, B=4, h=8, S_suf=32,
            n_split=2, partial=P2, nbytes=None):
    if nbytes is None:
        nbytes = L.vh_attn_decode_shared_ws_bytes(B, h, prefix_len, n_split)
    return L.vh_attn_decode_shared_kv16(q, 64 * h, kp, vp, prefix_len, prefix_S, ks, vs, out, 64 * h, sl, len_bias, B, h, S_suf,
                                        n_split, partial, nbytes, None)


@pytest.mark.parametrize('kw,text', [
    (dict(q=None), 'null pointer'), (dict(kp=None), 'null pointer'), (dict(vp=None), 'null pointer'),
    (dict(ks=None), 'null pointer'), (dict(vs=None), 'null pointer'), (dict(out=None), 'null pointer'),
    (dict(sl=None), 'null pointer'), (dict(partial=None), 'null pointer'),
    (dict(n_split=0), 'n_split=0'), (dict(n_split=17), 'n_split=17'),
    (dict(nbytes=64), 'workspace'),
    (dict(prefix_len=8192, prefix_S=8192, n_split=1, nbytes=1 << 30), '256 records'),
    (dict(prefix_len=7712, prefix_S=8192, n_split=16, nbytes=1 << 30), '256 records'),
    (dict(prefix_len=129, prefix_S=128), 'prefix=129/128'),
    (dict(B=65, nbytes=1 << 30), 'B=65'), (dict(vp=P + 4), '16-byte aligned'),
])
def test_shared_kv16_refuses_before_any_gpu_work(L, kw, text):
    assert _shared(L, **kw) < 0
    assert 'vh_attn_decode_shared_kv16' in _err(L) and text in _err(L), _err(L)


def test_shared_kv16_workspace_one_byte_short(L):
    need = L.vh_attn_decode_shared_ws_bytes(4, 8, 1024, 16)
    assert need == 4 * 8 * (32 + 16) * 72 * 4
    assert _shared(L, prefix_len=1024, prefix_S=1024, n_split=16, nbytes=need - 1) < 0 and 'workspace' in _err(L)


# ---- decoder_check through vh_ar_decoder_create on host-only descriptors -------------------------------------------
def _desc(L, folded=True, prefix=False, **kw):
    layers = (_lib.VhLayer * 2)()
    for lay in layers:
        if folded:
            lay.wqkv_f = lay.qkv_c1 = lay.qkv_c2 = P
        if prefix:
            lay.kprefix = lay.vprefix = P
    d = _lib.VhArDecoderDesc(B=4, d_model=128, n_heads=2, dff=256, n_layers=2, S_max=64, V=1025, eos=1024, n_split=1,
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
    return bool(h)


def test_decoder_accepts_the_16_bit_cache_with_key_splits(L):
    need = L.vh_attn_decode_ws_bytes(4, 2, 4)
    assert _create(L, _desc(L, n_split=4, attn_partial=P2, attn_partial_bytes=need)), _err(L)
    assert not _create(L, _desc(L, n_split=4, attn_partial=P2, attn_partial_bytes=need - 1))
    assert 'attn_partial' in _err(L) and 'n_split=4' in _err(L), _err(L)
    assert not _create(L, _desc(L, n_split=4, attn_partial=None, attn_partial_bytes=need))
    assert not _create(L, _desc(L, n_split=17, attn_partial=P2, attn_partial_bytes=1 << 24)) and '1..16' in _err(L)
    # the folded-weights requirement stays, and stays ahead of the new forms
    assert not _create(L, _desc(L, folded=False, n_split=4, attn_partial=P2, attn_partial_bytes=need)) and 'folded' in _err(L)


def test_decoder_accepts_the_16_bit_cache_with_a_shared_prompt(L):
    need = L.vh_attn_decode_shared_ws_bytes(4, 2, 100, 2)
    kw = dict(prefix=True, n_split=2, prefix_len=100, prefix_S=128, attn_partial=P2)
    assert _create(L, _desc(L, attn_partial_bytes=need, **kw)), _err(L)
    assert not _create(L, _desc(L, attn_partial_bytes=need - 1, **kw)) and 'attn_partial' in _err(L)
    assert not _create(L, _desc(L, attn_partial_bytes=need, **dict(kw, prefix=False))) and 'kprefix' in _err(L)
    assert not _create(L, _desc(L, attn_partial_bytes=1 << 30, **dict(kw, prefix_len=8000, prefix_S=8192, n_split=8)))
    assert '256 records' in _err(L)
    assert not _create(L, _desc(L, folded=False, attn_partial_bytes=need, **kw)) and 'folded' in _err(L)


def test_decoder_keeps_the_refusals_of_the_16_bit_cache(L):
    """d_model <= 1024 and head width 64 only, as before."""
    assert not _create(L, _desc(L, d_model=2048, n_heads=32, dff=4096)) and '1024' in _err(L)
    assert not _create(L, _desc(L, d_model=128, n_heads=4)) and 'width 64 only' in _err(L)


def test_python_gates_follow(monkeypatch):
    from valle2_amd import engine
    assert engine.pick_n_split(4 * 8) == 8 and engine.pick_n_split(8 * 16) == 2 and engine.pick_n_split(32 * 8) == 1
    assert 1 <= engine.shared_n_split(4, 8) <= 16
    import inspect
    from valle2_amd.valle_ar import ValleAR
    sig = inspect.signature(ValleAR.generate)
    assert list(sig.parameters)[:4] == ['self', 'prompt_tokens', 'prompt_codes', 'target_tokens']
    assert sig.parameters['perf_mode'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['perf_mode'].default is False


def test_new_kernels_compile_without_scratch_at_two_waves_per_simd():
    sys.path.insert(0, str(REPO / 'tools'))
    import check_isa
    problems = check_isa.check_perf_mode_beams(check_isa.compile_attention_asm())
    assert not problems, problems
