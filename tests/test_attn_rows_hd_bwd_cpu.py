"""`vh_attn_rows_hd_lse`, `vh_attn_rows_hd_bwd` and `vh_attn_rows_hd_bwd_ws_bytes` (training on flash attention at head widths
other than 64) without a GPU: the ABI (header, binding, export, version, integration guide), every refusal of the two entry
points — return code and message, with made-up aligned pointers that are never dereferenced because every check runs before any
launch —, the workspace size, and the backward call counter."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
VH_OK, VH_EINVAL, VH_EALIGN, VH_EUNSUPPORTED = 0, -1, -2, -3
MASK_FULL, MASK_PREFIX, MASK_EXPLICIT = 0, 1, 2

CTYPE = {'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p,
         'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _declaration(name, result='int'):
    m = re.search(r'^%s %s\((.*?)\);' % (result, name), HEADER, re.S | re.M)
    assert m, f'include/valle_hip.h does not declare {name}'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    return [(p.rsplit(' ', 1)[0], p.rsplit(' ', 1)[1]) for p in params]


def _lib():
    from valle2_amd import _lib
    return _lib.load_library()


@pytest.mark.parametrize('name,result', [('vh_attn_rows_hd_lse', 'int'), ('vh_attn_rows_hd_bwd', 'int'),
                                         ('vh_attn_rows_hd_bwd_ws_bytes', 'size_t')])
def test_header_binding_and_library_agree_on_the_entries(name, result):
    from valle2_amd import _lib
    decl = _declaration(name, result)
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if result == 'int' else ctypes.c_size_t)
    assert args == [CTYPE[t] for t, _ in decl], 'argtypes of the binding differ from the declaration'
    lib = _lib.load_library()
    assert hasattr(lib, name)
    assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_the_new_entries_extend_the_forward_entry_s_parameters():
    fwd = _declaration('vh_attn_rows_hd')
    lse = _declaration('vh_attn_rows_hd_lse')
    assert lse[:-2] == fwd[:-1] and lse[-2:] == [('float*', 'lse2'), ('void*', 'stream')]
    names = [n for _, n in _declaration('vh_attn_rows_hd_bwd')]
    assert [n for n in names if n in ('q', 'k', 'v', 'out', 'dout', 'lse2', 'dq', 'dk', 'dv')] == \
        ['q', 'k', 'v', 'out', 'dout', 'lse2', 'dq', 'dk', 'dv']
    assert names[-12:] == ['B', 'n_heads', 'head_dim', 'T', 'scale', 'mode', 'x_len', 'x_len_dev', 'kv_len', 'ws', 'ws_bytes',
                           'stream']


def test_abi_version_stays_and_the_integration_guide_names_the_entries():
    assert int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1)) == 146
    assert _lib().vh_version() == 146
    text = (REPO / 'INTEGRATION.md').read_text()
    for name in ('vh_attn_rows_hd_lse', 'vh_attn_rows_hd_bwd', 'vh_attn_rows_hd_bwd_ws_bytes'):
        row = next((line for line in text.splitlines() if line.startswith('|') and name in line.split('|')[1]), None)
        assert row is not None, f'INTEGRATION.md has no row for {name}'
        assert 'addition' in row                      # a pure addition: said where the entry is listed


# ---- refusals ------------------------------------------------------------------------------------------------------------
B, H, HD, T = 2, 3, 32, 70
LD, LDO = 3 * H * HD, H * HD
# "device pointers": never dereferenced
Q, K, V = 0x10000, 0x10000 + 4 * H * HD, 0x10000 + 8 * H * HD
OUT, DOUT, LSE = 0x900000, 0xa00000, 0xb00000
DQ, DK, DV = 0xc00000, 0xc00000 + 4 * H * HD, 0xc00000 + 8 * H * HD
WS = 0xd00000
WS_BYTES = (B * H * T * 4 + 15) // 16 * 16


def _call_bwd(**over):
    """vh_attn_rows_hd_bwd on a well-formed call with `over` applied; returns (rc, message)."""
    lib = _lib()
    a = dict(q=Q, q_sb=T * LD, q_sh=HD, q_sr=LD, k=K, k_sb=T * LD, k_sh=HD, k_sr=LD, v=V, v_sb=T * LD, v_sh=HD, v_sr=LD,
             out=OUT, o_sb=T * LDO, o_sh=HD, o_sr=LDO, dout=DOUT, d_sb=T * LDO, d_sh=HD, d_sr=LDO, lse2=LSE, dq=DQ, dk=DK, dv=DV,
             g_sb=T * LD, g_sh=HD, g_sr=LD, B=B, n_heads=H, head_dim=HD, T=T, scale=HD ** -0.5, mode=MASK_PREFIX, x_len=33,
             x_len_dev=None, kv_len=None, ws=WS, ws_bytes=WS_BYTES, stream=None)
    assert [n for n in a] == [n for _, n in _declaration('vh_attn_rows_hd_bwd')]
    assert set(over) <= set(a), over
    a.update(over)
    rc = lib.vh_attn_rows_hd_bwd(*a.values())
    return rc, (lib.vh_last_error() or b'').decode()


def _call_lse(**over):
    lib = _lib()
    a = dict(q=Q, q_sb=T * LD, q_sh=HD, q_sr=LD, k=K, k_sb=T * LD, k_sh=HD, k_sr=LD, v=V, v_sb=T * LD, v_sh=HD, v_sr=LD,
             out=OUT, o_sb=T * LDO, o_sh=HD, o_sr=LDO, B=B, n_heads=H, head_dim=HD, Tq=T, Tk=T, scale=HD ** -0.5,
             mode=MASK_PREFIX, x_len=33, x_len_dev=None, kv_len=None, lse2=LSE, stream=None)
    assert [n for n in a] == [n for _, n in _declaration('vh_attn_rows_hd_lse')]
    assert set(over) <= set(a), over
    a.update(over)
    rc = lib.vh_attn_rows_hd_lse(*a.values())
    return rc, (lib.vh_last_error() or b'').decode()


def _refused(call, entry, code, needle, **over):
    rc, msg = call(**over)
    assert rc == code, (over, rc, msg)
    assert f'{entry}:' in msg and needle in msg, (over, msg)


def bwd_refused(code, needle, **over):
    _refused(_call_bwd, 'vh_attn_rows_hd_bwd', code, needle, **over)


def lse_refused(code, needle, **over):
    _refused(_call_lse, 'vh_attn_rows_hd_lse', code, needle, **over)


BWD_POINTERS = dict(q=Q, k=K, v=V, out=OUT, dout=DOUT, lse2=LSE, dq=DQ, dk=DK, dv=DV, ws=WS)


@pytest.mark.parametrize('name', sorted(BWD_POINTERS))
def test_bwd_refuses_null_and_misaligned_pointers(name):
    bwd_refused(VH_EINVAL, 'null pointer', **{name: None})
    for off in (4, 8, 12):
        bwd_refused(VH_EALIGN, '16-byte aligned', **{name: BWD_POINTERS[name] + off})


def test_bwd_refuses_the_explicit_mask_mode_and_unknown_modes():
    bwd_refused(VH_EUNSUPPORTED, 'VH_MASK_EXPLICIT', mode=MASK_EXPLICIT)
    bwd_refused(VH_EINVAL, 'mode=7', mode=7)
    bwd_refused(VH_EINVAL, 'mode=-1', mode=-1)


@pytest.mark.parametrize('name,shown', [('B', 'B'), ('n_heads', 'h'), ('T', 'T')])
@pytest.mark.parametrize('value', [0, -1, -2 ** 31])
def test_bwd_refuses_zero_and_negative_dims(name, shown, value):
    bwd_refused(VH_EINVAL, f'{shown}={value}', **{name: value})


@pytest.mark.parametrize('hd', [0, 12, 18, 132, 256])
def test_bwd_refuses_widths_outside_the_served_set(hd):
    bwd_refused(VH_EUNSUPPORTED, f'head_dim={hd}', head_dim=hd)


@pytest.mark.parametrize('name,shown', [('q_sb', 'q batch'), ('q_sh', 'q head'), ('q_sr', 'q row'), ('k_sb', 'k batch'),
                                        ('k_sh', 'k head'), ('k_sr', 'k row'), ('v_sb', 'v batch'), ('v_sh', 'v head'),
                                        ('v_sr', 'v row'), ('o_sb', 'out batch'), ('o_sh', 'out head'), ('o_sr', 'out row'),
                                        ('d_sb', 'dout batch'), ('d_sh', 'dout head'), ('d_sr', 'dout row'),
                                        ('g_sb', 'grad batch'), ('g_sh', 'grad head'), ('g_sr', 'grad row')])
def test_bwd_refuses_a_stride_that_takes_rows_off_the_16_byte_grid(name, shown):
    for off in (1, 2, 3):
        value = LD + off
        bwd_refused(VH_EINVAL, f'{shown} stride={value}', **{name: value})


@pytest.mark.parametrize('name,shown', [('q_sr', 'q row'), ('k_sr', 'k row'), ('v_sr', 'v row'), ('d_sr', 'dout row')])
def test_bwd_refuses_staged_rows_beyond_the_32_bit_offsets(name, shown):
    bwd_refused(VH_EUNSUPPORTED, f'{shown} stride=-288', **{name: -LD})
    bwd_refused(VH_EUNSUPPORTED, f'{shown} stride={2 ** 40}', **{name: 2 ** 40})
    reach = (2 ** 30 - HD) // (T - 1) // 4 * 4
    assert _call_bwd(**{name: reach + 4})[0] == VH_EUNSUPPORTED


def test_workspace_covers_the_d_vector_and_one_byte_less_is_refused():
    lib = _lib()
    for b, h, t in [(1, 1, 1), (2, 3, 70), (16, 16, 1024), (3, 5, 333)]:
        need = lib.vh_attn_rows_hd_bwd_ws_bytes(b, h, t)
        assert b * h * t * 4 <= need <= b * h * t * 4 + 16
    assert lib.vh_attn_rows_hd_bwd_ws_bytes(2 ** 15, 2 ** 10, 2 ** 10) >= 2 ** 37        # no 32-bit product
    need = lib.vh_attn_rows_hd_bwd_ws_bytes(B, H, T)
    assert need == WS_BYTES
    bwd_refused(VH_EINVAL, f'workspace of {need - 1} bytes, need {need}', ws_bytes=need - 1)
    bwd_refused(VH_EINVAL, 'workspace of 0 bytes', ws_bytes=0)


def test_bwd_refuses_a_grid_that_does_not_fit():
    big = 2 ** 31 - 1
    bwd_refused(VH_EINVAL, 'exceed one grid', B=big, n_heads=big, T=1, ws_bytes=2 ** 63)


# ---- the forward with lse: vh_attn_rows_hd's checks under its own name, plus lse2 -----------------------------------------
def test_lse_refuses_a_null_or_misaligned_lse2():
    lse_refused(VH_EINVAL, 'null pointer', lse2=None)
    for off in (4, 8, 12):
        lse_refused(VH_EALIGN, '16-byte aligned', lse2=LSE + off)


def test_lse_refuses_what_the_forward_entry_refuses():
    for name, base in (('q', Q), ('k', K), ('v', V), ('out', OUT)):
        lse_refused(VH_EINVAL, 'null pointer', **{name: None})
        lse_refused(VH_EALIGN, '16-byte aligned', **{name: base + 4})
    lse_refused(VH_EUNSUPPORTED, 'VH_MASK_EXPLICIT', mode=MASK_EXPLICIT)
    lse_refused(VH_EINVAL, 'mode=7', mode=7)
    for name, shown in (('B', 'B'), ('n_heads', 'h'), ('Tq', 'Tq')):
        for value in (0, -1, -2 ** 31):
            lse_refused(VH_EINVAL, f'{shown}={value}', **{name: value})
    lse_refused(VH_EINVAL, f'Tq={T + 1} Tk={T}', Tq=T + 1)
    for hd in (12, 18, 132, 256):
        lse_refused(VH_EUNSUPPORTED, f'head_dim={hd}', head_dim=hd)
    for name, shown in (('q_sr', 'q row'), ('k_sh', 'k head'), ('v_sb', 'v batch'), ('o_sr', 'out row')):
        lse_refused(VH_EINVAL, f'{shown} stride={LD + 2}', **{name: LD + 2})
    lse_refused(VH_EUNSUPPORTED, 'k row stride=-288', k_sr=-LD)
    lse_refused(VH_EUNSUPPORTED, f'v row stride={2 ** 40}', v_sr=2 ** 40)
    lse_refused(VH_EINVAL, 'exceed one grid', B=2 ** 31 - 1, n_heads=2 ** 31 - 1)


# ---- Python side ---------------------------------------------------------------------------------------------------------
def test_backward_call_counts_start_at_zero_and_reset_with_the_forward_ones():
    from valle2_amd import kernels as K
    assert set(K.ATTN_HD_BWD_CALLS) == {'flash', 'materialized'}
    assert set(K.ATTN_HD_CALLS) == {'flash', 'materialized'}
    K.ATTN_HD_BWD_CALLS['flash'] += 2
    K.ATTN_HD_BWD_CALLS['materialized'] += 1
    K.ATTN_HD_CALLS['materialized'] += 4
    K.reset_attn_hd_calls()
    assert K.ATTN_HD_BWD_CALLS == {'flash': 0, 'materialized': 0}
    assert K.ATTN_HD_CALLS == {'flash': 0, 'materialized': 0}
    assert callable(K.attn_rows_hd_bwd)
