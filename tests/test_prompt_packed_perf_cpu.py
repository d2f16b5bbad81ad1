"""The packed AR prompt pass in perf mode, the part that needs no device: the three C entry points
(`vh_attn_rows_packed_lm_bf16`, `vh_transformer_forward_packed_lm_bf16`, `vh_kv_unpack_bf16`) — declared, bound, versioned, and
refusing each single fault before any GPU work with the documented code and a message that names the entry point and the
argument — the switch (`ValleAR.packed_prompt_perf`), the rule that says which calls qualify, the Python surface and the
compiled code of `attn16_packed_lm_kernel`."""
import ctypes as C
import inspect
import itertools
import os
import re
import sys
from pathlib import Path

import pytest

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tools'))
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
P, P2, P3, P4, I32 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # "device pointers": 16-byte aligned, never dereferenced
ABI = 146                         # VH_VERSION of this feature
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
ATTN, FORWARD, UNPACK = 'vh_attn_rows_packed_lm_bf16', 'vh_transformer_forward_packed_lm_bf16', 'vh_kv_unpack_bf16'
PADDED_KERNEL, LM_KERNEL = '_Z13attn16_kernel10Attn16Args', '_Z23attn16_packed_lm_kernel10Attn16Args14Packed16LmSegs'


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()                                     # (needs no GPU: tests/test_attn_forms_cpu.py loads it the same way)


def _err(L):
    return (L.vh_last_error() or b'').decode()


# ---- header, bindings, version -----------------------------------------------------------------------------------------
def _declared_params(name):
    m = re.search(r'^int %s\((.*?)\);' % name, HEADER, re.S | re.M)
    assert m, f'{name} is not declared in include/valle_hip.h'
    return [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]


def _ctype_of(param):
    if '*' in param:
        return C.POINTER(_lib.VhForward16Desc) if 'vh_forward16_desc' in param else C.c_void_p
    assert param.startswith('int '), param
    return C.c_int


@pytest.mark.parametrize('name', [ATTN, FORWARD, UNPACK])
def test_header_declares_and_bindings_match(L, name):
    params = _declared_params(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert argtypes == [_ctype_of(p) for p in params], f'{name}: {params}'
    assert getattr(L, name).argtypes == argtypes                  # (getattr fails when the library does not export it)


def test_argument_order():
    names = lambda entry: [re.sub(r'.*[ *]', '', p) for p in _declared_params(entry)]   # noqa: E731
    assert names(ATTN) == ['q', 'ldq', 'kcache16', 'vcache16', 'out', 'ldo', 'n_heads', 'S_max', 'seg_start', 'seg_len', 'seg_x_len',
                           'n_seg', 'blocks', 'n_blocks', 'stream']
    assert names(FORWARD) == ['desc', 'seg_start', 'seg_len', 'seg_x_len', 'n_seg', 'blocks', 'n_blocks', 'stream']
    assert names(UNPACK) == ['src', 'dst', 'n_streams', 'n_heads', 'S_src', 'B_dst', 'S_dst', 'seg_start', 'seg_len', 'dst_row',
                             'n_seg', 'stream']
    assert names(UNPACK) == names('vh_kv_unpack')


def test_version_is_146_and_the_headers(L):
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared == ABI
    text = (REPO / 'INTEGRATION.md').read_text()
    assert re.search(r'ABI %d\b' % ABI, text), 'INTEGRATION.md has a row for the ABI number'
    assert ATTN in text and FORWARD in text and UNPACK in text, 'INTEGRATION.md names the three entry points'
    for name in (ATTN, FORWARD, UNPACK):
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int %s\(' % name, HEADER, re.S)
        assert m and 'ABI %d' % ABI in m.group(1), f'{name}: the header comment names ABI {ABI}'


# ---- refusals of vh_attn_rows_packed_lm_bf16 ---------------------------------------------------------------------------
def _attn_args(**kw):
    a = dict(q=P, ldq=128, kcache=P2, vcache=P3, out=P4, ldo=128, n_heads=2, S_max=512, seg_start=I32, seg_len=I32 + 64,
             seg_x_len=I32 + 128, n_seg=3, blocks=I32 + 192, n_blocks=4, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize('kw,code,text', [
    (dict(q=None), EINVAL, 'null pointer (q'),
    (dict(out=None), EINVAL, 'null pointer (q, kcache16, vcache16 or out)'),
    (dict(kcache=None), EINVAL, 'kcache'),
    (dict(vcache=None), EINVAL, 'vcache'),
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(seg_x_len=None), EINVAL, 'seg_x_len'),
    (dict(blocks=None), EINVAL, 'blocks'),
    (dict(q=P + 4), EALIGN, 'q must be 16-byte aligned'),
    (dict(out=P4 + 8), EALIGN, 'out must be 16-byte aligned'),
    (dict(kcache=P2 + 4), EALIGN, 'kcache16 and vcache16'),
    (dict(vcache=P3 + 4), EALIGN, 'kcache16 and vcache16'),
    (dict(ldq=126), EINVAL, 'ldq=126'),
    (dict(ldq=132), EINVAL, 'ldq=132'),                # a multiple of 4, not of 8
    (dict(ldq=64), EINVAL, 'ldq=64'),                  # narrower than n_heads * 64
    (dict(ldo=130), EINVAL, 'ldo=130'),
    (dict(ldo=64), EINVAL, 'ldo=64'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_seg=-1), EINVAL, 'n_seg=-1'),
    (dict(n_blocks=0), EINVAL, 'n_blocks=0'),
    (dict(S_max=0), EINVAL, 'S_max=0'),
    (dict(n_heads=0), EINVAL, 'n_heads=0'),
    (dict(n_heads=1 << 20, ldq=1 << 26, ldo=1 << 26, n_blocks=1 << 20), EUNSUPPORTED, 'workgroups'),
])
def test_attn_rows_packed_lm_bf16_refuses_before_any_gpu_work(L, kw, code, text):
    rc = L.vh_attn_rows_packed_lm_bf16(*_attn_args(**kw))
    assert rc == code, (rc, _err(L))
    assert ATTN in _err(L) and text in _err(L), _err(L)


# ---- refusals of vh_transformer_forward_packed_lm_bf16 -----------------------------------------------------------------
def _desc(layers, layers16, **kw):
    f = dict(B=1, T=300, d_model=128, n_heads=2, dff=256, n_layers=len(layers), S_max=320, mode=1, x_len=0, ln_eps=1e-5,
             layers=layers, layers16=layers16, x=P, xn16=P2, q16=P3, attn16=P4, hidden16=P + 0x100)
    f.update(kw)
    return _lib.VhForward16Desc(**f)


def _layers(n=2, kcache=P2, vcache=P3, wo=P4, ln2_g=P, b1=P):
    arr, arr16 = (_lib.VhLayer * n)(), (_lib.VhLayer16 * n)()
    for i in range(n):
        arr16[i].wqkv, arr16[i].wo, arr16[i].w1, arr16[i].w2 = P, wo, P, P
        arr16[i].kcache16, arr16[i].vcache16 = kcache, vcache
        arr[i].ln1_g, arr[i].ln1_b, arr[i].ln2_g, arr[i].ln2_b = P, P, ln2_g, P
        arr[i].bo, arr[i].b1, arr[i].b2 = P, b1, P
    return arr, arr16


def _lm(L, desc, seg_start=I32, seg_len=I32 + 64, seg_x_len=I32 + 128, n_seg=3, blocks=I32 + 192, n_blocks=4):
    return L.vh_transformer_forward_packed_lm_bf16(None if desc is None else C.byref(desc), seg_start, seg_len, seg_x_len, n_seg,
                                                   blocks, n_blocks, None)


@pytest.mark.parametrize('kw,code,text', [
    (dict(B=2), EINVAL, 'B=2'),
    (dict(B=0), EINVAL, 'B=0'),
    (dict(S_max=299), EINVAL, 'S_max=299 < T=300'),
    (dict(T=0), EINVAL, 'T=0'),
    (dict(n_layers=0), EINVAL, 'L=0'),
    (dict(mode=0), EUNSUPPORTED, 'mode=0'),                                   # the full mask is vh_transformer_forward_packed_bf16's
    (dict(mode=2), EUNSUPPORTED, 'mode=2'),
    (dict(kv_len=I32), EUNSUPPORTED, 'kv_len is set'),
    (dict(x_len_dev=I32), EUNSUPPORTED, 'x_len_dev is set'),
    (dict(ada=P), EUNSUPPORTED, 'ada is set'),
    (dict(d_model=128, n_heads=4), EUNSUPPORTED, 'd_model=128'),              # head width 32
    (dict(d_model=192, n_heads=3), EUNSUPPORTED, 'd_model=192'),              # n_heads x 64, not a multiple of 128
    (dict(dff=192), EUNSUPPORTED, 'dff=192'),
    (dict(d_model=4224, n_heads=66), EUNSUPPORTED, 'd_model=4224'),
    (dict(x=None), EINVAL, 'null pointer in desc'),
    (dict(q16=None), EINVAL, 'null pointer in desc'),
    (dict(hidden16=None), EINVAL, 'null pointer in desc'),
    (dict(q16=P3 + 4), EALIGN, 'xn16, q16, attn16 and hidden16 must be 16-byte aligned'),
    (dict(attn16=P4 + 4), EALIGN, 'xn16, q16, attn16 and hidden16 must be 16-byte aligned'),
    (dict(x=P + 4), EALIGN, 'x, x_in and ada must be 16-byte aligned'),
    (dict(x_in=P + 8), EALIGN, 'x, x_in and ada must be 16-byte aligned'),
])
def test_forward_packed_lm_bf16_refuses_a_bad_descriptor(L, kw, code, text):
    layers, layers16 = _layers()
    rc = _lm(L, _desc(layers, layers16, **kw))
    assert rc == code, (rc, _err(L))
    assert FORWARD in _err(L) and text in _err(L), _err(L)


@pytest.mark.parametrize('kw,code,text', [
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(seg_x_len=None), EINVAL, 'seg_x_len'),
    (dict(blocks=None), EINVAL, 'blocks'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_blocks=0), EINVAL, 'n_blocks=0'),
    (dict(n_blocks=-2), EINVAL, 'n_blocks=-2'),
])
def test_forward_packed_lm_bf16_refuses_bad_segment_arguments(L, kw, code, text):
    layers, layers16 = _layers()
    rc = _lm(L, _desc(layers, layers16), **kw)
    assert rc == code and FORWARD in _err(L) and text in _err(L), (rc, _err(L))


def test_forward_packed_lm_bf16_refuses_a_null_desc_and_bad_layers(L):
    assert _lm(L, None) == EINVAL and FORWARD in _err(L) and 'null pointer' in _err(L)
    for bad, code, text in ((dict(kcache=P2 + 4), EALIGN, 'kcache16 and vcache16 must be 16-byte aligned'),
                            (dict(vcache=0), EINVAL, 'null bf16 pointer'), (dict(wo=0), EINVAL, 'null bf16 pointer'),
                            (dict(wo=P4 + 2), EALIGN, 'wqkv, wo, w1 and w2'), (dict(ln2_g=0), EINVAL, 'null LayerNorm parameter'),
                            (dict(b1=P + 4), EALIGN, 'LayerNorm parameters and biases')):
        layers, layers16 = _layers(**bad)
        rc = _lm(L, _desc(layers, layers16))
        assert rc == code and FORWARD in _err(L) and text in _err(L), (bad, rc, _err(L))


def test_the_full_mask_composite_still_refuses_the_prefix_mask_under_its_own_name(L):
    layers, layers16 = _layers()
    rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16, mode=1)), I32, I32 + 64, 3, I32 + 128, 4, None)
    assert rc == EUNSUPPORTED and 'vh_transformer_forward_packed_bf16: mode=1' in _err(L), _err(L)
    rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16, mode=0, B=2)), I32, I32 + 64, 3, I32 + 128, 4, None)
    assert rc == EINVAL and 'vh_transformer_forward_packed_bf16: B=2' in _err(L), _err(L)


# ---- refusals of vh_kv_unpack_bf16: those of vh_kv_unpack ----------------------------------------------------------------
def _unpack_args(**kw):
    a = dict(src=P, dst=P2, n_streams=4, n_heads=2, S_src=700, B_dst=8, S_dst=320, seg_start=I32, seg_len=I32 + 64,
             dst_row=I32 + 128, n_seg=8, stream=None)
    a.update(kw)
    return list(a.values())


UNPACK_FAULTS = [
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
    (dict(S_src=0), EINVAL, 'S_src=0'),
    (dict(B_dst=0), EINVAL, 'B_dst=0'),
    (dict(S_dst=-1), EINVAL, 'S_dst=-1'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_seg=-3), EINVAL, 'n_seg=-3'),
    (dict(n_seg=65536), EUNSUPPORTED, 'n_seg=65536'),
    (dict(S_src=(1 << 26) + 1), EUNSUPPORTED, 'S_src=67108865'),
]


@pytest.mark.parametrize('kw,code,text', UNPACK_FAULTS)
def test_kv_unpack_bf16_refuses_what_kv_unpack_refuses(L, kw, code, text):
    rc = L.vh_kv_unpack_bf16(*_unpack_args(**kw))
    assert rc == code, (rc, _err(L))
    assert _err(L).startswith('vh_kv_unpack_bf16:') and text in _err(L), _err(L)
    assert L.vh_kv_unpack(*_unpack_args(**kw)) == code and _err(L).startswith('vh_kv_unpack:'), _err(L)   # the fp32 entry under its own name


# ---- the switch --------------------------------------------------------------------------------------------------------
def test_packed_prompt_perf_is_a_class_attribute_and_none_by_default():
    from valle2_amd import ConfigValle
    from valle2_amd.valle_ar import ValleAR
    assert 'packed_prompt_perf' in vars(ValleAR) and ValleAR.packed_prompt_perf is None
    m = ValleAR(ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0))
    assert m.packed_prompt_perf is None and 'packed_prompt_perf' not in vars(m)
    assert ValleAR.packed_prompt is None                              # the fp32 switch is as it was


def test_the_switch_reads_the_attribute_then_the_environment(monkeypatch):
    from valle2_amd import generation

    class Model:
        packed_prompt_perf = None
        packed_prompt = True                                          # the fp32 switch does not turn this one on
    m = Model()
    monkeypatch.delenv('VALLE2_PACKED_PROMPT_PERF', raising=False)
    monkeypatch.setenv('VALLE2_PACKED_PROMPT', '1')                   # nor does its variable
    assert generation.packed_prompt_perf_on(m) is False
    monkeypatch.setenv('VALLE2_PACKED_PROMPT_PERF', '1')
    assert generation.packed_prompt_perf_on(m) is True
    monkeypatch.setenv('VALLE2_PACKED_PROMPT_PERF', '0')
    assert generation.packed_prompt_perf_on(m) is False
    m.packed_prompt_perf = True
    assert generation.packed_prompt_perf_on(m) is True
    monkeypatch.setenv('VALLE2_PACKED_PROMPT_PERF', '1')
    m.packed_prompt_perf = False
    assert generation.packed_prompt_perf_on(m) is False
    # and the other way round: this switch and its variable leave the fp32 one alone
    m.packed_prompt, m.packed_prompt_perf = None, True
    monkeypatch.delenv('VALLE2_PACKED_PROMPT', raising=False)
    assert generation.packed_prompt_on(m) is False


# ---- which calls qualify -----------------------------------------------------------------------------------------------
def test_qualifying_rule_over_every_combination():
    from valle2_amd import generation as G
    kinds = [G.RECOMPUTE_GENERAL, G.ROWS_HD, G.SHARED, G.GROUPED, G.ROWS_PERF_PREFILL, G.ROWS]
    n = 0
    for kind, perf, hd, forced, ragged, no_cache in itertools.product(kinds, (False, True, 'kv'), (16, 32, 64, 128), (False, True),
                                                                      (False, True), (False, True)):
        want = (ragged and perf is not False and hd == 64 and not forced and not no_cache and kind in (G.ROWS_PERF_PREFILL, G.ROWS))
        got = G.packed_prompt_perf_qualifies(kind, perf, hd, forced, ragged, no_cache)
        assert got is want, (kind, perf, hd, forced, ragged, no_cache)
        # the fp32 rule is unchanged for perf mode: never
        assert not (perf and G.packed_prompt_qualifies(kind, perf, hd, forced, ragged, no_cache))
        n += got
    assert n == 4                                                  # two kinds x perf_mode True / 'kv'


def test_qualifying_rule_on_real_plans():
    from valle2_amd import ConfigValle
    from valle2_amd import generation as G

    def q(cfg, txs, pls, forced=False, **kw):
        plan = G.plan_decode(cfg, txs, pls, max_new=8, **kw)
        return plan.kind, G.packed_prompt_perf_qualifies(plan.kind, plan.perf_mode, cfg.d_model // cfg.n_heads, forced, plan.ragged,
                                                         plan.no_cache)
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=512, num_layers=2, dropout=0.0)
    assert q(cfg, [5, 9], [7, 4], perf_mode=True) == (G.ROWS_PERF_PREFILL, True)
    assert q(cfg, [5, 9], [7, 4], perf_mode='kv') == (G.ROWS, True)
    assert q(cfg, [5, 5], [7, 4], perf_mode=True) == (G.ROWS_PERF_PREFILL, True)     # a prompt length alone makes a batch ragged
    cfg192 = ConfigValle(d_model=128, n_heads=2, dim_feedforward=192, num_layers=2, dropout=0.0)
    assert q(cfg192, [5, 9], [7, 4], perf_mode=True) == (G.ROWS, True)               # the 16-bit stack does not take dff 192: fp32 packed
    assert q(cfg, [5, 9], [7, 4]) == (G.ROWS, False)                                 # fp32: the other switch's
    assert q(cfg, [5, 5], [7, 7], perf_mode=True) == (G.ROWS_PERF_PREFILL, False)    # equal lengths: nothing to pack
    assert q(cfg, [5, 5], [7, 7], perf_mode=True, shared_prompt=True) == (G.SHARED, False)
    assert q(cfg, [5, 9], [7, 4], perf_mode=True, forced=True, by_hand=True) == (G.ROWS_PERF_PREFILL, False)
    assert q(cfg, [5, 9], [7, 4], beams=2) == (G.GROUPED, False)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_new_python_entry_points_and_untouched_signatures():
    from valle2_amd import engine, generation, kernels
    assert list(inspect.signature(kernels.attn_rows_packed_lm_bf16).parameters) == ['q', 'kcache', 'vcache', 'out', 'n_heads', 'rows']
    assert list(inspect.signature(kernels.kv_unpack_bf16).parameters) == ['src', 'dst', 'seg_start', 'seg_len', 'dst_row']
    assert list(inspect.signature(engine.transformer_forward_packed_lm_bf16).parameters) == ['transformer', 'x', 'cache', 'rows', 'scratch']
    assert list(inspect.signature(generation.packed_prompt_perf_qualifies).parameters) == \
        ['kind', 'perf_mode', 'head_dim', 'forced', 'ragged', 'no_cache']
    assert list(inspect.signature(generation.packed_prompt_perf_on).parameters) == ['model']
    # what was there keeps its signature
    assert list(inspect.signature(generation.packed_pass).parameters) == ['model', 'texts', 'txs', 'pls', 'codes', 'into', 'dst_rows']
    assert list(inspect.signature(engine.KVCache.unpack_into).parameters) == ['self', 'dst', 'seg_start', 'seg_len', 'dst_row']
    assert list(inspect.signature(kernels.kv_unpack).parameters) == ['src', 'dst', 'seg_start', 'seg_len', 'dst_row']
    assert list(inspect.signature(engine.transformer_forward_packed_lm).parameters) == ['transformer', 'x', 'cache', 'rows', 'scratch', 'lse2']


def test_generate_signatures_carry_no_new_flag():
    from valle2_amd import codec_io
    from valle2_amd.valle_ar import ValleAR
    for fn in (ValleAR.generate, ValleAR.generate_batch, ValleAR.generate_many, ValleAR.generate_queued):
        assert not any('packed' in name for name in inspect.signature(fn).parameters), fn.__name__
    for name in dir(codec_io):
        if name.startswith('synthesize'):
            assert not any('packed' in p for p in inspect.signature(getattr(codec_io, name)).parameters), name


# ---- the compiled kernel -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bf16_asm():
    import check_isa
    return check_isa.compile_bf16_asm()


def _resources(asm, mangled):
    seg = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(mangled), asm, re.S)
    assert seg, f'{mangled} not found'
    return {k: int(re.search(r'\.amdhsa_%s (\d+)' % k, seg.group(1)).group(1))
            for k in ('next_free_vgpr', 'group_segment_fixed_size', 'private_segment_fixed_size')}


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not installed')
def test_packed_lm_kernel_isa_properties(bf16_asm):
    """No scratch, the loop's wait counts and the M0 writes of the LDS-DMA staging as in the two kernels the body already makes."""
    import check_isa
    assert LM_KERNEL in check_isa.BF16_WAIT_KERNELS
    problems = check_isa.check_no_scratch(bf16_asm, names=['attn16_packed_lm_kernel'])
    problems += check_isa.check_loop_waits(bf16_asm, [LM_KERNEL]) + check_isa.check_m0(bf16_asm, [LM_KERNEL])
    assert not problems, '\n'.join(problems)


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not installed')
def test_packed_lm_kernel_takes_no_more_registers_or_lds_than_the_padded_one(bf16_asm):
    """The padded kernel carries the prefix mask too: the segment form of it must fit the same two workgroups per CU."""
    padded, lm = _resources(bf16_asm, PADDED_KERNEL), _resources(bf16_asm, LM_KERNEL)
    assert lm['private_segment_fixed_size'] == 0
    assert lm['next_free_vgpr'] <= padded['next_free_vgpr'], (lm, padded)
    assert lm['group_segment_fixed_size'] <= padded['group_segment_fixed_size'], (lm, padded)
