"""Packed NAR decoding in perf mode, the part that needs no device: the two C entry points (`vh_attn_rows_packed_bf16`,
`vh_transformer_forward_packed_bf16`) — declared, bound, versioned, and refusing a bad call before any GPU work with a message
that names the entry point and the argument — the Python surface (`ValleNAR.generate_packed_perf`,
`engine.transformer_forward_packed_bf16`, `kernels.attn_rows_packed_bf16`) and the compiled code of `attn16_packed_kernel`."""
import ctypes as C
import inspect
import os
import re
import sys
from pathlib import Path

import pytest
import torch

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tools'))
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
P, P2, P3, P4, I32 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # "device pointers": 16-byte aligned, never dereferenced
ABI = 140                         # VH_VERSION of this feature
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
ATTN, FORWARD = 'vh_attn_rows_packed_bf16', 'vh_transformer_forward_packed_bf16'
PADDED_KERNEL, PACKED_KERNEL = '_Z13attn16_kernel10Attn16Args', '_Z20attn16_packed_kernel10Attn16Args12Packed16Segs'


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
        return C.POINTER(_lib.VhForward16Desc) if 'vh_forward16_desc' in param else C.c_void_p
    assert param.startswith('int '), param
    return C.c_int


@pytest.mark.parametrize('name', [ATTN, FORWARD])
def test_header_declares_and_bindings_match(L, name):
    params = _declared_params(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert argtypes == [_ctype_of(p) for p in params], f'{name}: {params}'
    assert getattr(L, name).argtypes == argtypes


def test_argument_order():
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params(ATTN)]
    assert names == ['q', 'ldq', 'kcache16', 'vcache16', 'out', 'ldo', 'n_heads', 'S_max', 'seg_start', 'seg_len', 'n_seg',
                     'blocks', 'n_blocks', 'stream']
    names = [re.sub(r'.*[ *]', '', p) for p in _declared_params(FORWARD)]
    assert names == ['desc', 'seg_start', 'seg_len', 'n_seg', 'blocks', 'n_blocks', 'stream']


def test_version_is_the_headers_and_integration_names_it(L):
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared >= ABI
    text = (REPO / 'INTEGRATION.md').read_text()
    assert re.search(r'\b%d\b' % declared, text), 'INTEGRATION.md names the ABI number'
    assert ATTN in text and FORWARD in text, 'INTEGRATION.md names the two entry points'


def test_header_states_the_callers_contract_for_the_device_arrays():
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int %s\(' % ATTN, HEADER, re.S)
    text = ' '.join(m.group(1).split())
    assert 'caller vouches' in text and 'disjoint' in text and 'blocks' in text


# ---- refusals of vh_attn_rows_packed_bf16 ------------------------------------------------------------------------------
def _attn_args(**kw):
    a = dict(q=P, ldq=128, kcache=P2, vcache=P3, out=P4, ldo=128, n_heads=2, S_max=512, seg_start=I32, seg_len=I32 + 64, n_seg=3,
             blocks=I32 + 128, n_blocks=4, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize('kw,code,text', [
    (dict(q=None), EINVAL, 'null pointer (q'),
    (dict(out=None), EINVAL, 'null pointer (q, kcache16, vcache16 or out)'),
    (dict(kcache=None), EINVAL, 'kcache'),
    (dict(seg_start=None), EINVAL, 'seg_start'),
    (dict(seg_len=None), EINVAL, 'seg_len'),
    (dict(blocks=None), EINVAL, 'blocks'),
    (dict(q=P + 4), EALIGN, 'q must be 16-byte aligned'),
    (dict(out=P4 + 8), EALIGN, 'out must be 16-byte aligned'),
    (dict(kcache=P2 + 4), EALIGN, 'kcache16 and vcache16'),
    (dict(vcache=P3 + 4), EALIGN, 'kcache16 and vcache16'),
    (dict(ldq=126), EINVAL, 'ldq=126'),
    (dict(ldq=132), EINVAL, 'ldq=132'),                # a multiple of 4, as the fp32 form takes, but not of 8
    (dict(ldq=64), EINVAL, 'ldq=64'),                  # narrower than n_heads * 64
    (dict(ldo=130), EINVAL, 'ldo=130'),
    (dict(ldo=132), EINVAL, 'ldo=132'),
    (dict(ldo=64), EINVAL, 'ldo=64'),
    (dict(n_seg=0), EINVAL, 'n_seg=0'),
    (dict(n_blocks=0), EINVAL, 'n_blocks=0'),
    (dict(S_max=0), EINVAL, 'S_max=0'),
    (dict(n_heads=0), EINVAL, 'n_heads=0'),
    (dict(n_heads=1 << 20, ldq=1 << 26, ldo=1 << 26, n_blocks=1 << 20), EUNSUPPORTED, 'workgroups'),
])
def test_attn_rows_packed_bf16_refuses_before_any_gpu_work(L, kw, code, text):
    rc = L.vh_attn_rows_packed_bf16(*_attn_args(**kw))
    assert rc == code, (rc, _err(L))
    assert ATTN in _err(L) and text in _err(L), _err(L)


# ---- refusals of vh_transformer_forward_packed_bf16 --------------------------------------------------------------------
def _desc(layers, layers16, **kw):
    f = dict(B=1, T=300, d_model=128, n_heads=2, dff=256, n_layers=len(layers), S_max=320, mode=0, x_len=0, ln_eps=1e-5,
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


@pytest.mark.parametrize('kw,code,text', [
    (dict(B=2), EINVAL, 'B=2'),
    (dict(S_max=299), EINVAL, 'S_max=299 < T=300'),
    (dict(T=0), EINVAL, 'T=0'),
    (dict(mode=1), EUNSUPPORTED, 'mode=1'),
    (dict(mode=2), EUNSUPPORTED, 'mode=2'),
    (dict(kv_len=I32), EUNSUPPORTED, 'kv_len is set'),
    (dict(x_len_dev=I32), EUNSUPPORTED, 'x_len_dev is set'),
    (dict(d_model=128, n_heads=4), EUNSUPPORTED, 'd_model=128'),              # head width 32
    (dict(d_model=192, n_heads=3), EUNSUPPORTED, 'd_model=192'),              # n_heads x 64, not a multiple of 128
    (dict(dff=192), EUNSUPPORTED, 'dff=192'),
    (dict(x=None), EINVAL, 'null pointer in desc'),
    (dict(q16=None), EINVAL, 'null pointer in desc'),
    (dict(q16=P3 + 4), EALIGN, 'must be 16-byte aligned'),
    (dict(attn16=P4 + 4), EALIGN, 'must be 16-byte aligned'),
    (dict(x=P + 4), EALIGN, 'x, x_in and ada must be 16-byte aligned'),
    (dict(ada=P + 8), EALIGN, 'x, x_in and ada must be 16-byte aligned'),
    (dict(d_model=4224, n_heads=66), EUNSUPPORTED, 'd_model=4224'),
])
def test_forward_packed_bf16_refuses_a_bad_descriptor(L, kw, code, text):
    layers, layers16 = _layers()
    rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16, **kw)), I32, I32 + 64, 3, I32 + 128, 4, None)
    assert rc == code, (rc, _err(L))
    assert FORWARD in _err(L) and text in _err(L), _err(L)


@pytest.mark.parametrize('args,code,text', [
    ((None, I32, 3, I32, 4), EINVAL, 'seg_start'),
    ((I32, None, 3, I32, 4), EINVAL, 'seg_len'),
    ((I32, I32, 3, None, 4), EINVAL, 'blocks'),
    ((I32, I32, 0, I32, 4), EINVAL, 'n_seg=0'),
    ((I32, I32, 3, I32, 0), EINVAL, 'n_blocks=0'),
])
def test_forward_packed_bf16_refuses_bad_segment_arguments(L, args, code, text):
    layers, layers16 = _layers()
    rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16)), *args, None)
    assert rc == code and FORWARD in _err(L) and text in _err(L), (rc, _err(L))


def test_forward_packed_bf16_refuses_a_null_desc_and_bad_layers(L):
    assert L.vh_transformer_forward_packed_bf16(None, I32, I32, 3, I32, 4, None) == EINVAL and 'null pointer' in _err(L)
    layers, layers16 = _layers(kcache=P2 + 4)
    rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16)), I32, I32, 3, I32, 4, None)
    assert rc == EALIGN and FORWARD in _err(L) and 'kcache16 and vcache16 must be 16-byte aligned' in _err(L), (rc, _err(L))
    for bad in (dict(vcache=0), dict(wo=0)):
        layers, layers16 = _layers(**bad)
        rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16)), I32, I32, 3, I32, 4, None)
        assert rc == EINVAL and FORWARD in _err(L) and 'null bf16 pointer' in _err(L), (rc, _err(L))
    # what an inner launch would refuse for a weight, a LayerNorm parameter or a bias is said under this entry point's name
    for bad, code, text in ((dict(wo=P4 + 2), EALIGN, 'wqkv, wo, w1 and w2'), (dict(ln2_g=0), EINVAL, 'null LayerNorm parameter'),
                            (dict(b1=P + 4), EALIGN, 'LayerNorm parameters and biases')):
        layers, layers16 = _layers(**bad)
        rc = L.vh_transformer_forward_packed_bf16(C.byref(_desc(layers, layers16)), I32, I32, 3, I32, 4, None)
        assert rc == code and FORWARD in _err(L) and text in _err(L), (rc, _err(L))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_signatures():
    from valle2_amd import engine, kernels
    from valle2_amd.valle_nar import ValleNAR
    for fn in (ValleNAR.generate_packed_perf, ValleNAR.generate_packed):            # (generate_packed's is unchanged)
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ['self', 'texts', 'prompt_codes', 'first_layers', 'greedy', 'seed', 'sampling']
        assert sig.parameters['sampling'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['sampling'].default is None
        assert sig.parameters['greedy'].default is False and sig.parameters['seed'].default is None
        assert 'perf_mode' not in sig.parameters
    assert ValleNAR.generate_packed_perf.__name__ == 'generate_packed_perf'
    assert list(inspect.signature(engine.transformer_forward_packed_bf16).parameters) == \
        ['transformer', 'x', 'cache', 'rows', 'embedding', 'scratch']
    assert list(inspect.signature(kernels.attn_rows_packed_bf16).parameters) == ['q', 'kcache', 'vcache', 'out', 'n_heads', 'rows']


def _cpu_model_and_inputs(**kw):
    from valle2_amd import ConfigValle
    from valle2_amd.valle_nar import ValleNAR
    cfg = ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='AdaptiveLayerNorm'),
                             **kw))
    m = ValleNAR(cfg).eval()                                       # CPU-resident; nothing below may touch a device
    g = torch.Generator().manual_seed(0)
    text = torch.randint(0, cfg.vocab_size, (5,), generator=g)
    pc = torch.randint(0, cfg.num_audio_tokens, (4, cfg.num_quantizers), generator=g)
    first = torch.randint(0, cfg.num_audio_tokens, (6,), generator=g)
    return m, ([text], [pc], [first])


def test_generate_packed_perf_names_a_head_width_other_than_64_without_a_device():
    m, args = _cpu_model_and_inputs(n_heads=4)
    with pytest.raises(ValueError, match='generate_packed_perf: head width 32'):
        m.generate_packed_perf(*args, greedy=True)


def test_generate_packed_perf_names_d_model_and_dim_feedforward_without_a_device():
    m, args = _cpu_model_and_inputs(dim_feedforward=192)
    with pytest.raises(ValueError, match=r'generate_packed_perf: d_model=128, dim_feedforward=192'):
        m.generate_packed_perf(*args, greedy=True)
    m, args = _cpu_model_and_inputs(d_model=192, n_heads=3)
    with pytest.raises(ValueError, match=r'd_model=192, dim_feedforward=256'):
        m.generate_packed_perf(*args, greedy=True)


# ---- the compiled kernel -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bf16_asm():
    import check_isa
    return check_isa.compile_bf16_asm()


def _resources(asm, mangled):
    """next_free_vgpr is the UNIFIED register file on gfx950 (architectural VGPRs up to accum_offset, then the AGPRs): no more of
    it is no more VGPRs and no more AGPRs together."""
    seg = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(mangled), asm, re.S)
    assert seg, f'{mangled} not found'
    return {k: int(re.search(r'\.amdhsa_%s (\d+)' % k, seg.group(1)).group(1))
            for k in ('next_free_vgpr', 'group_segment_fixed_size', 'private_segment_fixed_size')}


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not installed')
def test_packed_kernel_isa_properties(bf16_asm):
    import check_isa
    assert PACKED_KERNEL in check_isa.BF16_WAIT_KERNELS
    problems = check_isa.check_no_scratch(bf16_asm, names=['attn16_packed_kernel'])       # exists, no scratch, private segment 0
    problems += check_isa.check_loop_waits(bf16_asm, [PACKED_KERNEL]) + check_isa.check_m0(bf16_asm, [PACKED_KERNEL])
    assert not problems, '\n'.join(problems)


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not installed')
def test_packed_kernel_takes_no_more_registers_or_lds_than_the_padded_one(bf16_asm):
    padded, packed = _resources(bf16_asm, PADDED_KERNEL), _resources(bf16_asm, PACKED_KERNEL)
    assert packed['private_segment_fixed_size'] == 0
    assert packed['next_free_vgpr'] <= padded['next_free_vgpr'], (packed, padded)
    assert packed['group_segment_fixed_size'] <= padded['group_segment_fixed_size'], (packed, padded)
