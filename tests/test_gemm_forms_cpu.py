"""Which compiled form a decode GEMM takes, pinned (no GPU: vh_linear_form launches nothing).

tests/golden/gemm_decode_forms.txt is the dispatch of every vh_linear* entry point over a domain of shapes, recorded from the
kernel launches of the commit BEFORE the plan / table refactor (gemm.hip compiled with the launch macro replaced by a
recorder) and reproduced here through vh_linear_form.  A dispatch change shows up as a diff of that file: regenerate it with
`python -m tests.test_gemm_forms_cpu > tests/golden/gemm_decode_forms.txt` (from the repository root) and review the diff.

File format: [forms] and [messages] number the distinct kernels (family<template tuple> and block size) and refusals (return
code and text, with the call's own M / N / K written {M} {N} {K}) in order of first appearance; a [knobs ...] section has one
line per (entry, N or T, K) with the rows M grouped by outcome, `M,M,..=F<form>/<grid x.y.z>` or `=E<message>`.  The
sections of a single non-default knob list only the lines that differ from the default section."""
import ctypes as C
import re
from pathlib import Path

import pytest

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden' / 'gemm_decode_forms.txt'

ROW_GROUPS, TILE_DMA, LN_STATS = 2, 4, 9                     # VH_TUNE_*
KNOB_SETS = [(0, 0, 0), (2, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 1)]     # (ROW_GROUPS, LN_STATS, TILE_DMA): default, each alone
KS = (16, 128, 256, 384, 512, 640, 768, 896, 1024, 1040, 1280, 1536, 1792, 2048, 2304, 2560, 3072, 3584, 4096, 4112)
MS = (1, 16, 17, 32, 33, 48, 49, 64)
TILE_MS, TILE_KS = (65, 129), (48, 512)                      # the tile kernels: LDS-DMA or register staging
NS = (64, 1040)
E = _lib
# label -> (entry, LayerNorm kind, w16); the QKV entries take N = 3 K and, where listed, T in (1, 2)
LINEAR = {'linear': (E.ENTRY_LINEAR, E.LN_NONE, 0), 'linear+ln': (E.ENTRY_LINEAR, E.LN_GAMMA, 0),
          'linear_folded': (E.ENTRY_LINEAR, E.LN_FOLDED, 0), 'linear_w16': (E.ENTRY_LINEAR, E.LN_NONE, 1),
          'linear_ws': (E.ENTRY_LINEAR_WS, E.LN_NONE, 0), 'head_greedy': (E.ENTRY_HEAD_GREEDY, E.LN_NONE, 0)}
QKV_T = {'qkv': (E.ENTRY_QKV, E.LN_NONE, 0), 'qkv+ln': (E.ENTRY_QKV, E.LN_GAMMA, 0), 'qkv_folded': (E.ENTRY_QKV, E.LN_FOLDED, 0)}
QKV_1 = {'qkv_folded_kv16': (E.ENTRY_QKV_KV16, E.LN_FOLDED, 0), 'qkv_folded_kv16_w16': (E.ENTRY_QKV_KV16, E.LN_FOLDED, 1),
         'qkv_hd': (E.ENTRY_QKV_HD, E.LN_NONE, 0), 'qkv_hd+ln': (E.ENTRY_QKV_HD, E.LN_GAMMA, 0),
         'qkv_folded_hd': (E.ENTRY_QKV_HD, E.LN_FOLDED, 0)}
ENTRIES = {**LINEAR, **QKV_T, **QKV_1}
FAMILY = {1: 'fast', 2: 'generic', 3: 'tile_dma', 4: 'tile_reg', 5: 'head'}


TILE_LABELS = ('linear', 'linear_ws', 'linear_w16', 'qkv', 'qkv_hd')


def domain(knobs):
    """(label, N, K, T, [M...]) lines of one knob setting; head_greedy's N is its vocabulary V = N + 1.  The rows above 64
    (tile kernels) are asked at the default knobs and under TILE_DMA only, and only of the entries in TILE_LABELS."""
    decode_ms = () if knobs[2] else MS
    tile_ms = TILE_MS if knobs[:2] == (0, 0) else ()
    for label, (entry, _, _) in ENTRIES.items():
        qkv = entry in (E.ENTRY_QKV, E.ENTRY_QKV_HD, E.ENTRY_QKV_KV16)
        for K in sorted(KS + TILE_KS[:1]):
            if qkv and K % 64:
                continue
            for N in (3 * K,) if qkv else NS:
                for T in (1, 2) if label in QKV_T else (1,):
                    rows = [M for M in (decode_ms if K in KS else ()) + (tile_ms if K in TILE_KS and label in TILE_LABELS and T == 1 else ())
                            if M % T == 0]
                    if rows:
                        yield label, N + (label == 'head_greedy'), K, T, rows


def form_name(f):
    if f.family in (1, 2):
        return f'{FAMILY[f.family]}<{f.mt},{f.nw},{f.epi},{f.pw},{f.ln},{f.nj},{f.w16}> b={f.block}'
    return f'{FAMILY[f.family]}<{f.pw if f.family == 5 else f.epi}> b={f.block}'


def query(L, label, M, N, K, T):
    """('F', form name, grid) or ('E', return code, message) as vh_linear_form has it."""
    entry, ln, w16 = ENTRIES[label]
    info = _lib.VhLinearFormInfo()
    rc = L.vh_linear_form(entry, M, N, K, T, ln, w16, C.byref(info))
    if rc:
        return 'E', rc, (L.vh_last_error() or b'').decode()
    return 'F', form_name(info), tuple(info.grid)


def render(outcome, set_knobs):
    """The fixture's text from outcome(label, M, N, K, T) under every knob setting of KNOB_SETS."""
    forms, messages, sections = {}, {}, []
    default = None
    for knobs in KNOB_SETS:
        set_knobs(knobs)
        lines = {}
        for label, N, K, T, rows in domain(knobs):
            groups = {}
            for M in rows:
                o = outcome(label, M, N, K, T)
                if o[0] == 'F':
                    token = f'F{forms.setdefault(o[1], len(forms))}/' + '.'.join(map(str, o[2]))
                else:
                    text = o[2]
                    for name, v in (('M', M), ('N', N), ('K', K)):          # the call's own numbers, exactly
                        text = re.sub(rf'\b{name}={v}\b', f'{name}={{{name}}}', text)
                    token = f'E{messages.setdefault((o[1], text), len(messages))}'
                groups.setdefault(token, []).append(M)
            key = f'{label} N={N} K={K} T={T}'
            lines[key] = ' '.join(','.join(map(str, ms)) + '=' + t for t, ms in groups.items())
        if default is None:
            default = lines
        else:
            lines = {k: v for k, v in lines.items() if default.get(k) != v}
        sections.append(('[knobs ROW_GROUPS=%d LN_STATS=%d TILE_DMA=%d]' % knobs, lines))
    set_knobs(KNOB_SETS[0])
    out = ['[forms]'] + [f'F{i} {n}' for n, i in forms.items()]
    out += ['[messages]'] + [f'E{i} {rc} {text}' for (rc, text), i in messages.items()]
    for head, lines in sections:
        out += [head] + [f'{k}: {v}' for k, v in lines.items()]
    return '\n'.join(out) + '\n'


def library_render(L):
    def set_knobs(knobs):
        for knob, v in zip((ROW_GROUPS, LN_STATS, TILE_DMA), knobs):
            assert L.vh_set_tuning(knob, v) == 0
    try:
        return render(lambda *call: query(L, *call), set_knobs)
    finally:
        set_knobs(KNOB_SETS[0])


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def test_dispatch_reproduces_the_pinned_table(L):
    want = GOLDEN.read_text()
    assert len(want) < 100_000
    got = library_render(L)
    if got != want:
        diff = [f'{a!r} != {b!r}' for a, b in zip(got.splitlines(), want.splitlines()) if a != b]
        pytest.fail(f'{len(diff)} lines differ (and {len(got.splitlines())} vs {len(want.splitlines())} lines), first: ' + '\n'.join(diff[:5]))


# table rows no shape reaches, each on purpose: {(family, mt, nw, pw, ln, nj, w16, epi): reason}
UNREACHED_ON_PURPOSE = {}
# (the pinned domain has no d_model that is a multiple of 64 but not of 128 below 1024, the one way a QKV product without
# LayerNorm reaches the guarded kernel's eight-wave form: the walk below adds d_model = 192)


def test_plan_stays_inside_the_table_and_reaches_every_row(L):
    rows = set()
    info = _lib.VhLinearFormInfo()
    i = 0
    while L.vh_linear_form_row(i, C.byref(info)) == 0:
        for epi in range(8):
            if info.epis >> epi & 1:
                row = (info.family, info.mt, info.nw, info.pw, info.ln, info.nj, info.w16, epi)
                assert row not in rows, f'row {i} is listed twice: {row}'
                rows.add(row)
        i += 1
    assert i > 0 and 'vh_linear_form_row' in (L.vh_last_error() or b'').decode()
    reached = set()
    try:
        for rg in (0, 2, 3):
            for st in (0, 1):
                assert L.vh_set_tuning(ROW_GROUPS, rg) == 0 and L.vh_set_tuning(LN_STATS, st) == 0
                for label, N, K, T, ms in list(domain((rg, st, 0))) + [(lb, 3 * 192, 192, 1, MS) for lb in ('qkv', 'qkv_hd')]:
                    entry, ln, w16 = ENTRIES[label]
                    for M in ms:
                        if L.vh_linear_form(entry, M, N, K, T, ln, w16, C.byref(info)) == 0 and info.family in (1, 2):
                            reached.add((info.family, info.mt, info.nw, info.pw, info.ln, info.nj, info.w16, info.epi))
    finally:
        L.vh_set_tuning(ROW_GROUPS, 0), L.vh_set_tuning(LN_STATS, 0)
    assert reached <= rows, f'the plan returns forms that are not compiled: {sorted(reached - rows)}'
    assert rows - reached == set(UNREACHED_ON_PURPOSE), f'unreachable rows: {sorted(rows - reached - set(UNREACHED_ON_PURPOSE))}'


def test_form_query_argument_checks(L):
    info = _lib.VhLinearFormInfo()
    assert L.vh_linear_form(99, 1, 64, 128, 1, 0, 0, C.byref(info)) == -1
    assert L.vh_linear_form(E.ENTRY_QKV, 3, 384, 128, 2, 0, 0, C.byref(info)) == -1          # M % T != 0
    assert L.vh_linear_form(E.ENTRY_QKV, 4, 128, 128, 2, 0, 0, C.byref(info)) == -1          # N != 3 K
    assert L.vh_linear_form(E.ENTRY_QKV_KV16, 4, 384, 128, 1, E.LN_NONE, 0, C.byref(info)) == -1
    assert L.vh_linear_form(E.ENTRY_QKV, 4, 384, 128, 1, E.LN_FOLDED, 1, C.byref(info)) == -1   # no such 16-bit-weight entry
    assert L.vh_linear_form(E.ENTRY_LINEAR, 1, 64, 128, 1, 0, 0, None) == -1
    assert L.vh_linear_form(E.ENTRY_LINEAR, 0, 64, 128, 1, 0, 0, C.byref(info)) == 0 and info.family == 0      # nothing to launch
    # the answer is the entry point's own: same code, same text
    P = 0x10000
    assert L.vh_linear_form(E.ENTRY_LINEAR, 4, 64, 384, 1, E.LN_FOLDED, 0, C.byref(info)) == -3
    asked = L.vh_last_error()
    assert L.vh_linear_folded(P, 384, P, P, P, None, 0, P, 64, 4, 64, 384, 0, 1e-5, None) == -3
    assert L.vh_last_error() == asked and b'640,768,896' in asked
    assert info.family == 0 and info.block == 0


def test_version_is_138(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 138
    assert 'ABI 138' in (REPO / 'INTEGRATION.md').read_text()


if __name__ == '__main__':
    print(library_render(_lib.load_library()), end='')
