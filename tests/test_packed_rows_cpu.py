"""NAR decoding over packed rows, the part that needs no device: the packed layout (`engine.pack_plan`), the two C entry
points (`vh_attn_rows_packed`, `vh_transformer_forward_packed`) — declared, bound, versioned, and refusing a bad call before
any GPU work with a message that names the argument — and the Python surface of `ValleNAR.generate_packed`."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest
import torch

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
P, P2, P3, P4, I32 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # "device pointers": 16-byte aligned, never dereferenced
PARENT_ABI = 136                  # VH_VERSION of the commit before this feature
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


# ---- pack_plan ---------------------------------------------------------------------------------------------------------
def test_pack_plan_starts_and_total():
    from valle2_amd.engine import pack_plan
    starts, m, blocks = pack_plan([5, 130, 128, 1])
    assert starts == [0, 5, 135, 263] and m == 264
    assert sorted(blocks) == [(0, 0), (1, 0), (1, 128), (2, 0), (3, 0)]


@pytest.mark.parametrize('lengths', [[5, 130, 128, 1], [1], [129], [256, 257, 3, 1024, 128, 128], [7] * 9])
def test_pack_plan_blocks_cover_every_query_once_longest_first(lengths):
    from valle2_amd.engine import pack_plan
    starts, m, blocks = pack_plan(lengths)
    assert m == sum(lengths) and starts == [sum(lengths[:i]) for i in range(len(lengths))]
    seen = [[0] * n for n in lengths]
    for s, q0 in blocks:
        assert 0 <= s < len(lengths) and 0 <= q0 < lengths[s] and q0 % 128 == 0
        for i in range(q0, min(q0 + 128, lengths[s])):
            seen[s][i] += 1
    assert all(c == 1 for row in seen for c in row), 'every query of every segment exactly once'
    by_len = [lengths[s] for s, _ in blocks]
    assert by_len == sorted(by_len, reverse=True), 'blocks of longer segments come first'


def test_pack_plan_a_130_row_segment_has_blocks_at_0_and_128():
    from valle2_amd.engine import pack_plan
    _, _, blocks = pack_plan([5, 130, 128, 1])
    assert [q0 for s, q0 in blocks if s == 1] == [0, 128]
    assert blocks[:2] == [(1, 0), (1, 128)]                       # the longest segment's blocks lead the table


@pytest.mark.parametrize('lengths', [[], [3, 0, 2], [-1]])
def test_pack_plan_refuses_an_empty_list_and_lengths_below_one(lengths):
    from valle2_amd.engine import pack_plan
    with pytest.raises(ValueError, match='pack_plan'):
        pack_plan(lengths)


# ---- header, bindings, version -----------------------------------------------------------------------------------------
def _declared_params(name):
    m = re.search(r'^int %s\((.*?)\);' % name, HEADER, re.S | re.M)
    assert m, f'{name} is not declared in include/valle_hip.h'
    return [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]


def _ctype_of(param):
    if '*' in param:
        return C.POINTER(_lib.VhForwardDesc) if 'vh_forward_desc' in param else C.c_void_p
    assert param.startswith('int '), param
    return C.c_int


@pytest.mark.parametrize('name', ['vh_attn_rows_packed', 'vh_transformer_forward_packed'])
def test_header_declares_and_bindings_match(L, name):
    params = _declared_params(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert argtypes == [_ctype_of(p) for p in params], f'{name}: {params}'
    assert getattr(L, name).argtypes == argtypes


def test_attn_rows_packed_argument_order():
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params('vh_attn_rows_packed')]
    assert names == ['q', 'ldq', 'kcache', 'vcache', 'out', 'ldo', 'n_heads', 'S_max', 'seg_start', 'seg_len', 'n_seg',
                     'blocks', 'n_blocks', 'stream']
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params('vh_transformer_forward_packed')]
    assert names == ['desc', 'seg_start', 'seg_len', 'n_seg', 'blocks', 'n_blocks', 'stream']


def test_version_is_the_headers_and_above_the_parents(L):
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared >= PARENT_ABI + 1
    assert re.search(r'\b%d\b' % declared, (REPO / 'INTEGRATION.md').read_text()), 'INTEGRATION.md names the new ABI number'


def test_header_states_the_callers_contract_for_the_device_arrays():
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int vh_attn_rows_packed\(', HEADER, re.S)
    text = ' '.join(m.group(1).split())
    assert 'caller vouches' in text and 'disjoint' in text and 'blocks' in text


# ---- refusals of vh_attn_rows_packed -----------------------------------------------------------------------------------
def _attn_args(**kw):
    a = dict(q=P, ldq=128, kcache=P2, vcache=P3, out=P4, ldo=128, n_heads=2, S_max=512, seg_start=I32, seg_len=I32 + 64, n_seg=3,
             blocks=I32 + 128, n_blocks=4, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize('kw,code,text', [
    (dict(q=None), EINVAL, 'null pointer (q'),
    (dict(out=None), EINVAL, 'null pointer (q, kcache, vcache or out)'),
    (dict(kcache=None), EINVAL, 'kcache'),
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(blocks=None), EINVAL, 'blocks'),
    (dict(q=P + 4), EALIGN, 'q must be 16-byte aligned'),
    (dict(out=P4 + 8), EALIGN, 'out must be 16-byte aligned'),
    (dict(kcache=P2 + 4), EALIGN, 'kcache and vcache'),
    (dict(vcache=P3 + 4), EALIGN, 'kcache and vcache'),
    (dict(ldq=126), EINVAL, 'ldq=126'),
    (dict(ldq=64), EINVAL, 'ldq=64'),                  # narrower than n_heads * 64
    (dict(ldo=130), EINVAL, 'ldo=130'),
    (dict(ldo=64), EINVAL, 'ldo=64'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_blocks=0), EINVAL, 'n_blocks=0'),
    (dict(S_max=0), EINVAL, 'S_max=0'),
    (dict(n_heads=0), EINVAL, 'n_heads=0'),
])
def test_attn_rows_packed_refuses_before_any_gpu_work(L, kw, code, text):
    rc = L.vh_attn_rows_packed(*_attn_args(**kw))
    assert rc == code, (rc, _err(L))
    assert 'vh_attn_rows_packed' in _err(L) and text in _err(L), _err(L)


# ---- refusals of vh_transformer_forward_packed -------------------------------------------------------------------------
def _desc(layers, **kw):
    f = dict(B=1, T=300, d_model=128, n_heads=2, dff=256, n_layers=len(layers), S_max=320, mode=0, x_len=0, ln_eps=1e-5,
             layers=layers, x=P, xn=P2, q=P3, attn=P4, hidden=P + 0x100)
    f.update(kw)
    return _lib.VhForwardDesc(**f)


def _layers(n=2, kcache=P2, vcache=P3):
    arr = (_lib.VhLayer * n)()
    for i in range(n):
        arr[i].kcache, arr[i].vcache = kcache, vcache
    return arr


@pytest.mark.parametrize('kw,code,text', [
    (dict(B=2), EINVAL, 'B=2'),
    (dict(S_max=299), EINVAL, 'S_max=299 < T=300'),
    (dict(mode=1), EUNSUPPORTED, 'mode=1'),
    (dict(mode=2), EUNSUPPORTED, 'mode=2'),
    (dict(kv_len=I32), EUNSUPPORTED, 'kv_len is set'),
    (dict(x_len_dev=I32), EUNSUPPORTED, 'x_len_dev is set'),
    (dict(mask=P), EUNSUPPORTED, 'mask is set'),
    (dict(pad=P), EUNSUPPORTED, 'pad is set'),
    (dict(d_model=128, n_heads=4), EUNSUPPORTED, 'd_model=128 != n_heads=4 x 64'),
    (dict(x=None), EINVAL, 'null pointer in desc'),
    (dict(q=P3 + 4), EALIGN, 'q must be 16-byte aligned'),
    (dict(attn=P4 + 4), EALIGN, 'attn must be 16-byte aligned'),
])
def test_forward_packed_refuses_a_bad_descriptor(L, kw, code, text):
    layers = _layers()
    rc = L.vh_transformer_forward_packed(C.byref(_desc(layers, **kw)), I32, I32 + 64, 3, I32 + 128, 4, None)
    assert rc == code, (rc, _err(L))
    assert 'vh_transformer_forward_packed' in _err(L) and text in _err(L), _err(L)


@pytest.mark.parametrize('args,code,text', [
    ((None, I32, 3, I32, 4), EINVAL, 'seg_start'),
    ((I32, None, 3, I32, 4), EINVAL, 'seg_len'),
    ((I32, I32, 3, None, 4), EINVAL, 'blocks'),
    ((I32, I32, 0, I32, 4), EINVAL, 'n_seg=0'),
    ((I32, I32, 3, I32, 0), EINVAL, 'n_blocks=0'),
    # under the composite's own name, before anything is launched (it used to come from vh_attn_rows_packed inside layer 0)
    ((I32, I32, 3, I32, 1 << 30), EUNSUPPORTED, 'vh_transformer_forward_packed: n_blocks=1073741824 x n_heads=2 workgroups'),
])
def test_forward_packed_refuses_bad_segment_arguments(L, args, code, text):
    layers = _layers()
    rc = L.vh_transformer_forward_packed(C.byref(_desc(layers)), *args, None)
    assert rc == code and 'vh_transformer_forward_packed' in _err(L) and text in _err(L), (rc, _err(L))


def test_forward_packed_refuses_a_null_desc_and_misaligned_caches(L):
    assert L.vh_transformer_forward_packed(None, I32, I32, 3, I32, 4, None) == EINVAL and 'null pointer' in _err(L)
    layers = _layers(kcache=P2 + 4)
    rc = L.vh_transformer_forward_packed(C.byref(_desc(layers)), I32, I32, 3, I32, 4, None)
    assert rc == EALIGN and 'kcache and vcache must be 16-byte aligned' in _err(L), (rc, _err(L))
    layers = _layers(vcache=0)
    rc = L.vh_transformer_forward_packed(C.byref(_desc(layers)), I32, I32, 3, I32, 4, None)
    assert rc == EINVAL and 'kcache / vcache' in _err(L), (rc, _err(L))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_signatures():
    from valle2_amd import engine, kernels
    from valle2_amd.valle_nar import ValleNAR
    sig = inspect.signature(ValleNAR.generate_packed)
    assert list(sig.parameters) == ['self', 'texts', 'prompt_codes', 'first_layers', 'greedy', 'seed', 'sampling']
    assert sig.parameters['sampling'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['sampling'].default is None
    assert sig.parameters['greedy'].default is False and sig.parameters['seed'].default is None
    assert 'perf_mode' not in sig.parameters
    assert list(inspect.signature(engine.transformer_forward_packed).parameters) == \
        ['transformer', 'x', 'cache', 'rows', 'embedding', 'scratch']
    assert list(inspect.signature(kernels.attn_rows_packed).parameters) == ['q', 'kcache', 'vcache', 'out', 'n_heads', 'rows']
    assert callable(engine.pack_plan) and inspect.isclass(engine.PackedRows)


def test_generate_packed_names_a_head_width_other_than_64_without_a_device():
    from valle2_amd import ConfigValle
    from valle2_amd.valle_nar import ValleNAR
    cfg = ConfigValle(d_model=128, n_heads=4, dim_feedforward=256, num_layers=1, dropout=0.0, norm='AdaptiveLayerNorm')
    m = ValleNAR(cfg).eval()                                       # CPU-resident; nothing below may touch a device
    g = torch.Generator().manual_seed(0)
    text = torch.randint(0, cfg.vocab_size, (5,), generator=g)
    pc = torch.randint(0, cfg.num_audio_tokens, (4, cfg.num_quantizers), generator=g)
    first = torch.randint(0, cfg.num_audio_tokens, (6,), generator=g)
    with pytest.raises(ValueError, match='head width 32'):
        m.generate_packed([text], [pc], [first], greedy=True)
