"""Grouped shared-prompt decoding (several utterances' beams, each group over its own prompt), the parts that need no GPU:
vh_attn_decode_shared_groups is declared and exported, it and the decoder's descriptor check refuse what they must BEFORE any
GPU work (called through ctypes with made-up, aligned pointers: nothing is dereferenced on a refusal), the workspace query is
the record count of the prefix CAPACITY, and generate_batch(beams=...) refuses its argument pairs without a device."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced (every call is refused)
PART_LD = 72                                      # floats per record: o[64], m, l, pad (csrc/attention.hip)
NAME = 'vh_attn_decode_shared_groups'


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


def test_header_declares_and_library_exports_the_entry_points(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    assert re.search(r'\bint %s\(' % NAME, header) and re.search(r'\bsize_t %s_ws_bytes\(' % NAME, header)
    for name in (NAME, NAME + '_ws_bytes'):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 132
    for field in ('n_groups', 'beams_per_group', 'prefix_cap', 'prefix_lens'):
        assert re.search(r'\b%s\b' % field, header) and field in dict(_lib.VhArDecoderDesc._fields_)


@pytest.mark.parametrize('B,h,cap,n_split', [(12, 2, 100, 1), (64, 1, 112, 3), (8, 8, 1024, 16), (5, 2, 1, 1), (8, 2, 2651, 3)])
def test_workspace_is_the_record_count_of_the_capacity(L, B, h, cap, n_split):
    assert L.vh_attn_decode_shared_groups_ws_bytes(B, h, cap, n_split) == B * h * ((cap + 31) // 32 + n_split) * PART_LD * 4


def _call(L, q=P, kp=P, vp=P, plen=I32, cap=100, prefix_S=128, ks=P, vs=P, out=P, sl=I32, len_bias=1, B=12, beams=4, h=2,
          S_suf=32, n_split=2, partial=P2, nbytes=None):
    if nbytes is None:
        nbytes = L.vh_attn_decode_shared_groups_ws_bytes(B, h, cap, n_split)
    return L.vh_attn_decode_shared_groups(q, 64 * h, kp, vp, plen, cap, prefix_S, ks, vs, out, 64 * h, sl, len_bias, B, beams, h,
                                          S_suf, n_split, partial, nbytes, None)


@pytest.mark.parametrize('kw,text', [
    (dict(q=None), 'null pointer'), (dict(kp=None), 'null pointer'), (dict(vp=None), 'null pointer'),
    (dict(plen=None), 'null pointer'), (dict(ks=None), 'null pointer'), (dict(vs=None), 'null pointer'),
    (dict(out=None), 'null pointer'), (dict(sl=None), 'null pointer'), (dict(partial=None), 'null pointer'),
    (dict(B=13), 'B=13 is not a multiple of beams=4'), (dict(beams=0), 'beams=0'),
    (dict(B=65, beams=5, nbytes=1 << 30), 'B=65'),
    (dict(cap=129), 'prefix_cap=129/128'), (dict(cap=0), 'prefix_cap=0/128'),
    (dict(cap=8192, prefix_S=8192, n_split=1, nbytes=1 << 30), '256 records'),
    (dict(cap=8129, prefix_S=8192, n_split=2, nbytes=1 << 30), '256 records'),
    (dict(vp=P + 4), '16-byte aligned'), (dict(partial=P2 + 8), '16-byte aligned'),
    (dict(len_bias=2), 'len_bias=2'), (dict(n_split=0), 'n_split=0'),
])
def test_entry_point_refuses_before_any_gpu_work(L, kw, text):
    assert _call(L, **kw) < 0
    assert NAME + ':' in _err(L) and text in _err(L), _err(L)


def test_workspace_one_byte_short(L):
    need = L.vh_attn_decode_shared_groups_ws_bytes(12, 2, 100, 2)
    assert _call(L, nbytes=need - 1) < 0
    assert NAME + ':' in _err(L) and 'workspace' in _err(L) and str(need) in _err(L), _err(L)


# ---- decoder_check through vh_ar_decoder_create on host-only descriptors ---------------------------------------------------
def _desc(L, prefix=True, **kw):
    layers = (_lib.VhLayer * 2)()
    for lay in layers:
        lay.wqkv_f = lay.qkv_c1 = lay.qkv_c2 = P
        if prefix:
            lay.kprefix = lay.vprefix = P
    d = _lib.VhArDecoderDesc(B=12, d_model=128, n_heads=2, dff=256, n_layers=2, S_max=64, V=1025, eos=1024, n_split=2,
                             ln_eps=1e-5, layers=layers, proj_w=P, audio_emb=P, audio_pe=P, x=P, q=P, attn=P, hidden=P,
                             logits=P, cache_len=I32, audio_pos=I32, eos_count=I32, codes=P, codes_stride=80, top_k=1,
                             temperature=1.0, n_groups=3, beams_per_group=4, prefix_cap=128, prefix_S=128, prefix_lens=I32,
                             attn_partial=P2, attn_partial_bytes=L.vh_attn_decode_shared_groups_ws_bytes(12, 2, 128, 2))
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = layers
    return d


def _create(L, d):
    h = L.vh_ar_decoder_create(C.byref(d))
    if h:
        L.vh_ar_decoder_destroy(h)
    return bool(h)


def test_decoder_takes_groups_and_names_what_it_refuses(L):
    assert _create(L, _desc(L)), _err(L)
    need = L.vh_attn_decode_shared_groups_ws_bytes(12, 2, 128, 2)
    assert not _create(L, _desc(L, attn_partial_bytes=need - 1))
    assert 'attn_partial' in _err(L) and 'vh_attn_decode_shared_groups_ws_bytes' in _err(L) and str(need) in _err(L), _err(L)
    assert not _create(L, _desc(L, kv_bf16=1)) and 'kv_bf16' in _err(L) and 'n_groups=3' in _err(L), _err(L)
    assert not _create(L, _desc(L, n_heads=1)) and 'head width 128' in _err(L) and 'n_groups=3' in _err(L), _err(L)
    assert not _create(L, _desc(L, beams_per_group=5)) and 'beams_per_group=5' in _err(L), _err(L)
    assert not _create(L, _desc(L, prefix_cap=129)) and 'prefix_cap=129' in _err(L), _err(L)
    assert not _create(L, _desc(L, prefix_lens=None)) and 'prefix_lens' in _err(L), _err(L)
    assert not _create(L, _desc(L, prefix=False)) and 'kprefix' in _err(L), _err(L)
    assert not _create(L, _desc(L, prefix_len=100)) and 'prefix_len=100' in _err(L), _err(L)
    assert not _create(L, _desc(L, prefix_cap=8192, prefix_S=8192, attn_partial_bytes=1 << 30)) and '256 records' in _err(L)
    # n_groups == 0: today's forms, whatever the other new fields hold
    assert _create(L, _desc(L, n_groups=0, beams_per_group=0, prefix_cap=0, prefix_S=0, prefix_lens=None, prefix=False)), _err(L)


# ---- generate_batch(beams=...): the pure-Python refusals, on a CPU model with no device in sight ------------------------
def _cpu_model(**kw):
    from valle2_amd import ConfigValle, get_model_class
    cfg = ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm',
                                  num_beams=4, top_k=1, max_audio_len=8), **kw))
    return get_model_class('ValleAR')(cfg)


@pytest.mark.parametrize('cfg_kw,call_kw,text', [
    ({}, dict(beams=3, shared_prompt=True), 'beams=3 with shared_prompt=True'),
    ({}, dict(beams=3, perf_mode=True), 'beams=3 with perf_mode=True'),
    ({}, dict(beams=3, perf_mode='kv'), "beams=3 with perf_mode='kv'"),
    ({}, dict(beams=3, forced=torch.zeros(8, dtype=torch.int64)), 'beams=3 with forced'),
    (dict(use_kv_cache=False), dict(beams=2), 'beams=2 with use_kv_cache=False'),
    (dict(n_heads=4), dict(beams=2), 'beams=2 with use_kv_cache=True, d_model=128, n_heads=4'),
    ({}, dict(beams=65), 'beams=65'),
    ({}, dict(beams=0), 'beams=0'),
])
def test_generate_batch_refuses_beams_pairs_without_a_device(cfg_kw, call_kw, text):
    m = _cpu_model(**cfg_kw)
    texts, firsts = [torch.arange(5)] * 2, [torch.arange(7)] * 2
    with pytest.raises(ValueError, match=re.escape(text)):
        m.generate_batch(texts, firsts, **call_kw)


def test_signatures():
    import inspect
    from valle2_amd import codec_io, engine
    from valle2_amd.valle_ar import ValleAR
    p = inspect.signature(ValleAR.generate_batch).parameters
    assert p['beams'].default == 1 and p['beams'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[:3] == ['self', 'texts', 'first_codes'] and p['shared_prompt'].default is False
    p = inspect.signature(ValleAR.generate_many).parameters
    assert list(p) == ['self', 'utterances', 'beams'] and p['beams'].default is None
    assert list(inspect.signature(codec_io.synthesize_many).parameters) == ['ar', 'nar', 'items', 'codec', 'greedy_nar']
    # the slot capacity: the longest prompt rounded up to a fixed step, and what fits the merge's 256 records
    assert engine.group_prefix_cap(1) == engine.GROUP_PREFIX_STEP == engine.group_prefix_cap(128) and engine.group_prefix_cap(129) == 256
    assert engine.grouped_prompts_fit(32, 8, 1024) and not engine.grouped_prompts_fit(32, 8, 8192)


def test_synthesize_many_raises_synthesizes_error_for_an_empty_ar_output(monkeypatch):
    from valle2_amd import ConfigValle, codec_io as CIO, get_model_class
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=2)
    ar = get_model_class('ValleAR')(cfg)
    empty = torch.empty(0, dtype=torch.int64)
    monkeypatch.setattr(ar, 'generate_many', lambda utts: [torch.arange(3), empty])
    monkeypatch.setattr(ar, 'generate', lambda *a: empty)
    item = (torch.arange(4), torch.zeros(cfg.num_quantizers, 5, dtype=torch.int64), torch.arange(3))
    with pytest.raises(RuntimeError, match='emitted EOS at its first step') as one:
        CIO.synthesize(ar, None, *item)
    with pytest.raises(RuntimeError, match='emitted EOS at its first step') as many:
        CIO.synthesize_many(ar, None, [item, item])
    assert str(many.value).startswith(str(one.value))
