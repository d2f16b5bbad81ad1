"""The packed AR prompt pass, the part that needs no device: the two C entry points (`vh_kv_unpack`,
`vh_transformer_forward_packed_lm`) — declared, bound, versioned, and refusing each single fault before any GPU work with the
right code and a message that names the argument — the switch (`ValleAR.packed_prompt`), the pinned signatures of the
generate entry points, the rule that says which calls qualify, and the packed layout of a prompt pass."""
import ctypes as C
import inspect
import itertools
import re
from pathlib import Path

import pytest

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
P, P2, P3, P4, I32 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # "device pointers": 16-byte aligned, never dereferenced
PARENT_ABI = 144                  # VH_VERSION of the commit before this feature
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


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


@pytest.mark.parametrize('name', ['vh_kv_unpack', 'vh_transformer_forward_packed_lm'])
def test_library_exports_and_bindings_match_the_header(L, name):
    params = _declared_params(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert argtypes == [_ctype_of(p) for p in params], f'{name}: {params}'
    assert getattr(L, name).argtypes == argtypes                  # (getattr fails when the library does not export it)


def test_argument_order():
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params('vh_kv_unpack')]
    assert names == ['src', 'dst', 'n_streams', 'n_heads', 'S_src', 'B_dst', 'S_dst', 'seg_start', 'seg_len', 'dst_row', 'n_seg',
                     'stream']
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params('vh_transformer_forward_packed_lm')]
    assert names == ['desc', 'seg_start', 'seg_len', 'seg_x_len', 'n_seg', 'blocks', 'n_blocks', 'lse2', 'stream']


def test_version_is_the_headers_and_above_the_parents(L):
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared >= PARENT_ABI + 1
    assert re.search(r'ABI %d\b' % declared, (REPO / 'INTEGRATION.md').read_text()), 'INTEGRATION.md names the new ABI number'


# ---- refusals of vh_kv_unpack ------------------------------------------------------------------------------------------
def _unpack_args(**kw):
    a = dict(src=P, dst=P2, n_streams=4, n_heads=2, S_src=700, B_dst=8, S_dst=320, seg_start=I32, seg_len=I32 + 64,
             dst_row=I32 + 128, n_seg=8, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize('kw,code,text', [
    (dict(src=None), EINVAL, 'null pointer (src or dst)'),
    (dict(dst=None), EINVAL, 'null pointer (src or dst)'),
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(dst_row=None), EINVAL, 'dst_row'),
    (dict(src=P + 4), EALIGN, 'src and dst must be 16-byte aligned'),
    (dict(dst=P2 + 8), EALIGN, 'src and dst must be 16-byte aligned'),
    (dict(seg_start=I32 + 2), EALIGN, '4-byte aligned'),
    (dict(dst_row=I32 + 129), EALIGN, '4-byte aligned'),
    (dict(n_streams=0), EINVAL, 'n_streams=0'),
    (dict(n_heads=0), EINVAL, 'n_heads=0'),
    (dict(n_heads=-2), EINVAL, 'n_heads=-2'),
    (dict(S_src=0), EINVAL, 'S_src=0'),
    (dict(B_dst=0), EINVAL, 'B_dst=0'),
    (dict(S_dst=-1), EINVAL, 'S_dst=-1'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_seg=-3), EINVAL, 'n_seg=-3'),
    (dict(n_seg=65536), EUNSUPPORTED, 'n_seg=65536'),
    (dict(S_src=(1 << 26) + 1), EUNSUPPORTED, 'S_src=67108865'),
])
def test_kv_unpack_refuses_before_any_gpu_work(L, kw, code, text):
    rc = L.vh_kv_unpack(*_unpack_args(**kw))
    assert rc == code, (rc, _err(L))
    assert 'vh_kv_unpack' in _err(L) and text in _err(L), _err(L)


# ---- refusals of vh_transformer_forward_packed_lm ----------------------------------------------------------------------
def _desc(layers, **kw):
    f = dict(B=1, T=300, d_model=128, n_heads=2, dff=256, n_layers=len(layers), S_max=320, mode=1, x_len=0, ln_eps=1e-5,
             layers=layers, x=P, xn=P2, q=P3, attn=P4, hidden=P + 0x100)
    f.update(kw)
    return _lib.VhForwardDesc(**f)


def _layers(n=2, kcache=P2, vcache=P3):
    arr = (_lib.VhLayer * n)()
    for i in range(n):
        arr[i].kcache, arr[i].vcache = kcache, vcache
    return arr


def _lm(L, desc, seg_start=I32, seg_len=I32 + 64, seg_x_len=I32 + 128, n_seg=3, blocks=I32 + 192, n_blocks=4, lse2=P + 0x200):
    return L.vh_transformer_forward_packed_lm(None if desc is None else C.byref(desc), seg_start, seg_len, seg_x_len, n_seg, blocks,
                                              n_blocks, lse2, None)


@pytest.mark.parametrize('kw,code,text', [
    (dict(mode=0), EUNSUPPORTED, 'mode=0'),                        # the full mask is vh_transformer_forward_packed's
    (dict(mode=2), EUNSUPPORTED, 'mode=2'),
    (dict(B=2), EINVAL, 'B=2'),
    (dict(T=0), EINVAL, 'T=0'),
    (dict(n_layers=0), EINVAL, 'L=0'),
    (dict(S_max=299), EINVAL, 'S_max=299 < T=300'),
    (dict(kv_len=I32), EUNSUPPORTED, 'kv_len is set'),
    (dict(x_len_dev=I32), EUNSUPPORTED, 'x_len_dev is set'),
    (dict(mask=P), EUNSUPPORTED, 'mask is set'),
    (dict(pad=P), EUNSUPPORTED, 'pad is set'),
    (dict(ada=P), EUNSUPPORTED, 'ada is set'),
    (dict(d_model=128, n_heads=4), EUNSUPPORTED, 'd_model=128 != n_heads=4 x 64'),
    (dict(x=None), EINVAL, 'null pointer in desc'),
    (dict(hidden=None), EINVAL, 'null pointer in desc'),
    (dict(q=P3 + 4), EALIGN, 'q must be 16-byte aligned'),
    (dict(attn=P4 + 4), EALIGN, 'attn must be 16-byte aligned'),
])
def test_forward_packed_lm_refuses_a_bad_descriptor(L, kw, code, text):
    layers = _layers()
    rc = _lm(L, _desc(layers, **kw))
    assert rc == code, (rc, _err(L))
    assert 'vh_transformer_forward_packed_lm' in _err(L) and text in _err(L), _err(L)


@pytest.mark.parametrize('kw,code,text', [
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(seg_x_len=None), EINVAL, 'seg_x_len'),
    (dict(blocks=None), EINVAL, 'blocks'),
    (dict(lse2=None), EINVAL, 'lse2'),
    (dict(lse2=P + 0x202), EALIGN, 'lse2 must be 4-byte aligned'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_blocks=0), EINVAL, 'n_blocks=0'),
])
def test_forward_packed_lm_refuses_bad_segment_arguments(L, kw, code, text):
    layers = _layers()
    rc = _lm(L, _desc(layers), **kw)
    assert rc == code and 'vh_transformer_forward_packed_lm' in _err(L) and text in _err(L), (rc, _err(L))


def test_forward_packed_lm_refuses_a_null_desc_and_bad_caches(L):
    assert _lm(L, None) == EINVAL and 'null pointer' in _err(L)
    layers = _layers(kcache=P2 + 4)
    assert _lm(L, _desc(layers)) == EALIGN and 'kcache and vcache must be 16-byte aligned' in _err(L), _err(L)
    layers = _layers(vcache=0)
    assert _lm(L, _desc(layers)) == EINVAL and 'kcache / vcache' in _err(L), _err(L)


def test_forward_packed_still_refuses_the_prefix_mask(L):
    """The full-mask composite is untouched: the prefix mask is the new entry's, not a new mode of the old one."""
    layers = _layers()
    rc = L.vh_transformer_forward_packed(C.byref(_desc(layers, mode=1)), I32, I32 + 64, 3, I32 + 128, 4, None)
    assert rc == EUNSUPPORTED and 'mode=1' in _err(L)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_packed_prompt_is_a_class_attribute_and_none_by_default():
    from valle2_amd import ConfigValle
    from valle2_amd.valle_ar import ValleAR
    assert 'packed_prompt' in vars(ValleAR) and ValleAR.packed_prompt is None
    m = ValleAR(ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0))
    assert m.packed_prompt is None and 'packed_prompt' not in vars(m)


def test_the_switch_reads_the_attribute_then_the_environment(monkeypatch):
    from valle2_amd import generation

    class Model:
        packed_prompt = None
    m = Model()
    monkeypatch.delenv('VALLE2_PACKED_PROMPT', raising=False)
    assert generation.packed_prompt_on(m) is False
    monkeypatch.setenv('VALLE2_PACKED_PROMPT', '1')
    assert generation.packed_prompt_on(m) is True
    monkeypatch.setenv('VALLE2_PACKED_PROMPT', '0')
    assert generation.packed_prompt_on(m) is False
    m.packed_prompt = True
    assert generation.packed_prompt_on(m) is True
    monkeypatch.setenv('VALLE2_PACKED_PROMPT', '1')
    m.packed_prompt = False
    assert generation.packed_prompt_on(m) is False


def test_pinned_signatures_are_unchanged():
    from valle2_amd import codec_io
    from valle2_amd.valle_ar import ValleAR

    def sig(fn):
        return [(n, p.kind.name, p.default) for n, p in inspect.signature(fn).parameters.items()]
    E, KW, PK = inspect.Parameter.empty, 'KEYWORD_ONLY', 'POSITIONAL_OR_KEYWORD'
    assert sig(ValleAR.generate) == [('self', PK, E), ('prompt_tokens', PK, E), ('prompt_codes', PK, E), ('target_tokens', PK, None),
                                     ('perf_mode', KW, False), ('sampling', KW, None)]
    assert sig(ValleAR.generate_many) == [('self', PK, E), ('utterances', PK, E), ('beams', KW, None)]
    assert sig(ValleAR.generate_queued) == [('self', PK, E), ('utterances', PK, E), ('beams', KW, None), ('slots', KW, None)]
    assert sig(ValleAR.generate_batch) == [
        ('self', PK, E), ('texts', PK, E), ('first_codes', PK, E), ('max_new', PK, None), ('use_graph', PK, True),
        ('profile_attn', PK, False), ('perf_mode', PK, False), ('forced', PK, None), ('keep_logits', PK, ()),
        ('shared_prompt', PK, False), ('beams', KW, 1), ('sampling', KW, None)]
    for name in dir(codec_io):
        if name.startswith('synthesize'):
            assert 'packed_prompt' not in inspect.signature(getattr(codec_io, name)).parameters, name


def test_new_python_entry_points():
    from valle2_amd import engine, generation, kernels
    assert list(inspect.signature(engine.transformer_forward_packed_lm).parameters) == ['transformer', 'x', 'cache', 'rows', 'scratch', 'lse2']
    assert list(inspect.signature(kernels.kv_unpack).parameters) == ['src', 'dst', 'seg_start', 'seg_len', 'dst_row']
    assert list(inspect.signature(engine.KVCache.unpack_into).parameters) == ['self', 'dst', 'seg_start', 'seg_len', 'dst_row']
    assert list(inspect.signature(generation.packed_prompt_qualifies).parameters) == \
        ['kind', 'perf_mode', 'head_dim', 'forced', 'ragged', 'no_cache']
    # the full-mask composite keeps its signature
    assert list(inspect.signature(engine.transformer_forward_packed).parameters) == \
        ['transformer', 'x', 'cache', 'rows', 'embedding', 'scratch']


# ---- which calls qualify -----------------------------------------------------------------------------------------------
def test_qualifying_rule_over_every_combination():
    from valle2_amd import generation as G
    kinds = [G.RECOMPUTE_GENERAL, G.ROWS_HD, G.SHARED, G.GROUPED, G.ROWS_PERF_PREFILL, G.ROWS]
    n = 0
    for kind, perf, hd, forced, ragged, no_cache in itertools.product(kinds, (False, True, 'kv'), (16, 32, 64, 128), (False, True),
                                                                      (False, True), (False, True)):
        want = (ragged and perf is False and hd == 64 and not forced and not no_cache and kind in (G.ROWS, G.GROUPED))
        got = G.packed_prompt_qualifies(kind, perf, hd, forced, ragged, no_cache)
        assert got is want, (kind, perf, hd, forced, ragged, no_cache)
        n += got
    assert n == 2                                                  # ragged fp32 width-64 cached rows, and the same grouped


def test_qualifying_rule_on_real_plans():
    """The plans `plan_decode` makes for the calls the issue names: which of them the packed pass takes."""
    from valle2_amd import ConfigValle
    from valle2_amd import generation as G

    def q(cfg, txs, pls, forced=False, **kw):
        plan = G.plan_decode(cfg, txs, pls, max_new=8, **kw)
        return G.packed_prompt_qualifies(plan.kind, plan.perf_mode, cfg.d_model // cfg.n_heads, forced, plan.ragged, plan.no_cache)
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=512, num_layers=2, dropout=0.0)
    assert q(cfg, [5, 9], [7, 4])                                  # ragged rows
    assert q(cfg, [5, 9], [7, 4], beams=2)                         # ragged, grouped
    assert q(cfg, [5, 9], [7, 4], queued=True, cap=128)            # the queue's starting rows
    assert q(cfg, [5, 5], [7, 4])                                  # (a prompt length alone makes a batch ragged)
    assert not q(cfg, [5, 5], [7, 7])                              # equal lengths: nothing to pack
    assert not q(cfg, [5, 5], [7, 7], shared_prompt=True)
    assert not q(cfg, [5, 9], [7, 4], perf_mode=True)
    assert not q(cfg, [5, 9], [7, 4], perf_mode='kv')
    assert not q(cfg, [5, 9], [7, 4], forced=True, by_hand=True)
    cfg32 = ConfigValle(d_model=128, n_heads=4, dim_feedforward=512, num_layers=2, dropout=0.0)
    assert not q(cfg32, [5, 9], [7, 4])                            # head width 32: its own cached decoder, the padded pass
    cfg_nc = ConfigValle(d_model=128, n_heads=2, dim_feedforward=512, num_layers=2, dropout=0.0, use_kv_cache=False)
    assert not q(cfg_nc, [5, 9], [7, 4])                           # every step recomputes: the padded pass

