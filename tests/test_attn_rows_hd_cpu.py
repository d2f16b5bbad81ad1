"""`vh_attn_rows_hd` (many-row flash attention at head widths other than 64) without a GPU: the ABI (header, binding, export,
version), every refusal of the entry point — return code and message, with pointers that are never dereferenced because every
check runs before any launch — and the pure route function `kernels.attn_hd_route` over widths x switch states x mask specs."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
VH_OK, VH_EINVAL, VH_EALIGN, VH_EUNSUPPORTED = 0, -1, -2, -3
MASK_FULL, MASK_PREFIX, MASK_EXPLICIT = 0, 1, 2

CTYPE = {'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p,
         'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float}


def _declaration():
    m = re.search(r'^int vh_attn_rows_hd\((.*?)\);', HEADER, re.S | re.M)
    assert m, 'include/valle_hip.h does not declare vh_attn_rows_hd'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    return [(p.rsplit(' ', 1)[0], p.rsplit(' ', 1)[1]) for p in params]


def test_header_binding_and_library_agree_on_the_entry():
    from valle2_amd import _lib
    decl = _declaration()
    names = [n for _, n in decl]
    assert names[-11:] == ['B', 'n_heads', 'head_dim', 'Tq', 'Tk', 'scale', 'mode', 'x_len', 'x_len_dev', 'kv_len', 'stream']
    assert [n for n in names if n in ('q', 'k', 'v', 'out')] == ['q', 'k', 'v', 'out']
    res, args = _lib.SIGNATURES['vh_attn_rows_hd']
    assert res is ctypes.c_int
    assert args == [CTYPE[t] for t, _ in decl], 'argtypes of the binding differ from the declaration'
    lib = _lib.load_library()
    assert hasattr(lib, 'vh_attn_rows_hd')
    assert lib.vh_attn_rows_hd.argtypes == args


def test_abi_version_stays_and_the_integration_guide_names_the_entry():
    from valle2_amd import _lib
    assert int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1)) == 146
    assert _lib.load_library().vh_version() == 146
    text = (REPO / 'INTEGRATION.md').read_text()
    assert 'vh_attn_rows_hd' in text
    row = next(line for line in text.splitlines() if 'vh_attn_rows_hd' in line)
    assert 'addition' in row                          # a pure addition: said where the entry is listed


# ---- refusals ------------------------------------------------------------------------------------------------------------
B, H, HD, T = 2, 3, 32, 70
LD, LDO = 3 * H * HD, H * HD
Q, K, V, OUT = 0x10000, 0x10000 + 4 * H * HD, 0x10000 + 8 * H * HD, 0x900000        # "device pointers": never dereferenced


def _call(**over):
    """vh_attn_rows_hd on a well-formed call with `over` applied; returns (rc, message)."""
    from valle2_amd import _lib
    lib = _lib.load_library()
    a = dict(q=Q, q_sb=T * LD, q_sh=HD, q_sr=LD, k=K, k_sb=T * LD, k_sh=HD, k_sr=LD, v=V, v_sb=T * LD, v_sh=HD, v_sr=LD,
             out=OUT, o_sb=T * LDO, o_sh=HD, o_sr=LDO, B=B, n_heads=H, head_dim=HD, Tq=T, Tk=T, scale=HD ** -0.5,
             mode=MASK_PREFIX, x_len=33, x_len_dev=None, kv_len=None, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    rc = lib.vh_attn_rows_hd(*a.values())
    return rc, (lib.vh_last_error() or b'').decode()


def _refused(code, needle, **over):
    rc, msg = _call(**over)
    assert rc == code, (over, rc, msg)
    assert 'vh_attn_rows_hd' in msg and needle in msg, (over, msg)


@pytest.mark.parametrize('hd', [12, 18, 132, 256])
def test_refuses_widths_outside_the_served_set(hd):
    _refused(VH_EUNSUPPORTED, f'head_dim={hd}', head_dim=hd)


def test_refuses_the_explicit_mask_mode_and_unknown_modes():
    _refused(VH_EUNSUPPORTED, 'VH_MASK_EXPLICIT', mode=MASK_EXPLICIT)
    _refused(VH_EINVAL, 'mode=7', mode=7)


def test_refuses_more_queries_than_keys():
    _refused(VH_EINVAL, f'Tq={T + 1} Tk={T}', Tq=T + 1)
    _refused(VH_EINVAL, 'Tq=5 Tk=4', Tq=5, Tk=4)


@pytest.mark.parametrize('name,shown', [('B', 'B'), ('n_heads', 'h'), ('Tq', 'Tq')])
@pytest.mark.parametrize('value', [0, -1, -2 ** 31])
def test_refuses_zero_and_negative_dims(name, shown, value):
    _refused(VH_EINVAL, f'{shown}={value}', **{name: value})


@pytest.mark.parametrize('name', ['q', 'k', 'v', 'out'])
def test_refuses_null_and_misaligned_operands(name):
    _refused(VH_EINVAL, 'null pointer', **{name: None})
    base = dict(q=Q, k=K, v=V, out=OUT)[name]
    for off in (4, 8, 12):
        _refused(VH_EALIGN, '16-byte aligned', **{name: base + off})


@pytest.mark.parametrize('name,shown', [('q_sr', 'q row'), ('k_sr', 'k row'), ('v_sr', 'v row'), ('o_sr', 'out row'),
                                        ('k_sh', 'k head'), ('o_sb', 'out batch')])
def test_refuses_a_stride_that_takes_rows_off_the_16_byte_grid(name, shown):
    for off in (1, 2, 3):
        value = LD + off
        _refused(VH_EINVAL, f'{shown} stride={value}', **{name: value})


def test_refuses_key_rows_beyond_the_32_bit_offsets():
    _refused(VH_EUNSUPPORTED, 'k row stride=-288', k_sr=-LD)
    _refused(VH_EUNSUPPORTED, f'v row stride={2 ** 40}', v_sr=2 ** 40)


# ---- the route -----------------------------------------------------------------------------------------------------------
WIDTHS = [12, 16, 20, 32, 48, 64, 96, 128, 132, 256]
SERVED = {16, 20, 32, 48, 96, 128}


@pytest.mark.parametrize('switch,env,on', [(None, None, False), (None, '1', True), (None, '0', False), (True, None, True),
                                           (True, '0', True), (False, None, False), (False, '1', False)])
def test_route_is_flash_exactly_where_the_switch_width_and_mask_allow(monkeypatch, switch, env, on):
    import torch
    from valle2_amd import kernels as K
    monkeypatch.setattr(K, 'ATTN_HD_FLASH', switch)
    if env is None:
        monkeypatch.delenv('VALLE2_ATTN_HD_FLASH', raising=False)
    else:
        monkeypatch.setenv('VALLE2_ATTN_HD_FLASH', env)
    mask = torch.zeros(5, 5, dtype=torch.uint8)
    analytic = [dict(mode=K.MASK_PREFIX, x_len=3, x_len_dev=None, kv_len=None, mask=None, pad=None),
                dict(mode=K.MASK_FULL, x_len=0, x_len_dev=None, kv_len=torch.zeros(2, dtype=torch.int32), mask=None, pad=None),
                dict(mode=K.MASK_FULL)]
    explicit = [dict(mode=K.MASK_EXPLICIT, x_len=0, x_len_dev=None, kv_len=None, mask=mask, pad=None),
                dict(mode=K.MASK_EXPLICIT, x_len=0, x_len_dev=None, kv_len=None, mask=mask, pad=torch.zeros(2, 5, dtype=torch.uint8)),
                dict(mode=K.MASK_FULL, mask=None, pad=torch.zeros(2, 5, dtype=torch.uint8))]
    for hd in WIDTHS:
        for spec in analytic:
            assert K.attn_hd_route(hd, spec) == ('flash' if on and hd in SERVED else 'materialized'), (hd, spec)
        for spec in explicit:
            assert K.attn_hd_route(hd, spec) == 'materialized', (hd, spec)
        if hd == 64:
            assert all(K.attn_hd_route(64, spec) == 'materialized' for spec in analytic + explicit)


def test_call_counts_start_at_zero_and_reset():
    from valle2_amd import kernels as K
    assert set(K.ATTN_HD_CALLS) == {'flash', 'materialized'}
    K.ATTN_HD_CALLS['flash'] += 3
    K.reset_attn_hd_calls()
    assert K.ATTN_HD_CALLS == {'flash': 0, 'materialized': 0}
    assert K.ATTN_HD_FLASH is None                    # default off: the environment decides, and unset means off
