"""Which kernels a decode-attention call launches, pinned (no GPU: vh_attn_decode_form launches nothing).

tests/golden/attn_decode_forms.txt is the dispatch of the seven vh_attn_decode* entry points over a domain of shapes and the
three decode knobs.  Its launch sections were recorded from the commit BEFORE the call-record / plan / launcher refactor:
attention.hip and attention_hd.hip compiled with the launch calls replaced by a recorder (kernel symbol with template
arguments, grid, block, and the same for the second launch) and driven through `render` below with the entry points themselves
as `launch`; the same recorder build of the refactored files wrote the same sections (18 053 calls, kernel arguments included,
byte for byte).  Here `launch` is vh_attn_decode_form.
The [refusals] section holds, per entry point, one valid call with one argument made wrong at a time: the return codes are the
recorded ones of that commit, the message texts are those of the one check the entry points now share.  Which fault is named
when a call has several is not pinned.  Pointer, len_bias and ldq / ldo faults go through the entry points themselves with
made-up aligned pointers (nothing is dereferenced on a refusal); `out`, the length arrays and the workspace of vh_attn_decode /
vh_attn_decode_hd have never been checked for alignment, so misaligning them is no refusal and not in the domain.

A dispatch change shows up as a diff of the file: regenerate it with
`python -m tests.test_attn_forms_cpu > tests/golden/attn_decode_forms.txt` (from the repository root) and review the diff.

File format: [forms] numbers the distinct launches (first kernel with template arguments and block, `+` second kernel and
block) in order of first appearance, [messages] the refusals (return code and text).  A [knobs ...] section has one line per
(entry, shape) with the n_split values grouped by outcome: `n,n,..=F<form>/<grid x.y.z>[+<second grid>]` or `=E<message>`;
the sections of a single non-default knob list only the lines that differ from the default section."""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import pytest

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden' / 'attn_decode_forms.txt'

VARIANT, WAVES, COMBINE = 0, 1, 12                           # VH_TUNE_DECODE_*
KNOB_SETS = [(0, 0, 0), (1, 0, 0), (0, 4, 0), (0, 8, 0), (0, 16, 0), (0, 0, 1), (0, 0, 2)]   # default, each single value alone
BS = (1, 3, 4, 8, 32, 33, 64, 65)
HS = (1, 2, 8, 16)
SPLITS = (1, 2, 3, 4, 8, 16, 17, 64, 65)                     # (4: 32 x 8 x 4 = 1024 against 32 x 8 x 3)
PREFIXES = (1, 31, 32, 33, 100, 1024, 7680, 7681, 8160, 8192)
BEAMS = (1, 4, 5)
HEAD_DIMS = (12, 16, 20, 32, 36, 64, 68, 128, 132, 192, 196, 256, 260)
ENTRIES = {'decode': _lib.ATTN_ENTRY_DECODE, 'kv16': _lib.ATTN_ENTRY_KV16, 'kv16_split': _lib.ATTN_ENTRY_KV16_SPLIT,
           'shared': _lib.ATTN_ENTRY_SHARED, 'shared_groups': _lib.ATTN_ENTRY_SHARED_GROUPS,
           'shared_kv16': _lib.ATTN_ENTRY_SHARED_KV16, 'hd': _lib.ATTN_ENTRY_HD}
SHARED = ('shared', 'shared_groups', 'shared_kv16')
KERNEL = {1: 'attn_decode_kernel<{nw}>', 2: 'attn_decode_ring_kernel<{nw},{d}>', 3: 'attn_decode_ring16_kernel<{nw},{d}>',
          4: 'attn_decode_ring16_split_kernel<{nw},{d}>', 5: 'attn_decode_hd_kernel<{nw},{d},{lk},{nv}>', 6: 'attn_shared_kernel',
          7: 'attn_shared_groups_kernel', 8: 'attn_shared16_kernel'}
SECOND = {1: 'attn_decode_combine_kernel', 2: 'attn_decode_hd_combine_kernel', 3: 'attn_records_merge_kernel',
          4: 'attn_records_merge_groups_kernel'}
AMPLE = 1 << 40                                              # workspace bytes of the launch domain: never the reason of a refusal


def shape(label, B, h, **kw):
    s = dict(label=label, B=B, h=h, hd=64, S_max=64, prefix=0, prefix_S=0, beams=1)
    s.update(kw)
    return s


def domain():
    """The shapes of one knob setting; each is asked at every n_split of SPLITS (vh_attn_decode_kv16 has none)."""
    for label in ('decode', 'kv16', 'kv16_split'):
        for B in BS:
            for h in HS:
                yield shape(label, B, h)
    for label in SHARED:
        for B in BS:                                         # every row count and head count at one prompt
            for h in HS:
                yield shape(label, B, h, prefix=100, prefix_S=100, beams=4 if label == 'shared_groups' and B % 4 == 0 else 1)
        for B, h in ((4, 8), (64, 16)):                      # every prompt length, once with a cache row to spare
            for p in PREFIXES:
                yield shape(label, B, h, prefix=p, prefix_S=p, beams=4 if label == 'shared_groups' else 1)
            yield shape(label, B, h, prefix=101, prefix_S=100)
            yield shape(label, B, h, prefix=100, prefix_S=101)
    for B in (4, 8, 64, 65):
        for beams in BEAMS:
            yield shape('shared_groups', B, 8, prefix=1024, prefix_S=1024, beams=beams)
    for hd in HEAD_DIMS:
        for B, h in ((1, 1), (4, 8), (64, 16)):
            yield shape('hd', B, h, hd=hd)


def form_text(f):
    """(launch name, grid text) of a vh_attn_decode_form_info."""
    name = KERNEL[f.kernel].format(nw=f.nw, d=f.d, lk=f.lk, nv=f.nv) + f' b={f.block}'
    grid = '.'.join(map(str, f.grid))
    if f.second:
        name += f' + {SECOND[f.second]} b={f.second_block}'
        grid += f'+{f.second_grid}'
    return name, grid


def query(L, s, n_split, nbytes=AMPLE):
    """('F', launch name, grid) or ('E', return code, message) as vh_attn_decode_form has it."""
    info = _lib.VhAttnDecodeFormInfo()
    rc = L.vh_attn_decode_form(ENTRIES[s['label']], s['B'], s['h'], s['hd'], s['S_max'], n_split, s['prefix'], s['prefix_S'],
                               s['beams'], nbytes, C.byref(info))
    if rc:
        return 'E', rc, (L.vh_last_error() or b'').decode()
    return ('F',) + form_text(info)


# ---- the refusal domain: one valid call per entry point, one argument wrong at a time ----------------------------------
P, P2, I32, MIS = 0x10000, 0x20000, 0x30000, 0x10004         # "device pointers": never dereferenced (every call is refused)
BASE = dict(q=P, k=P, v=P, out=P, len=I32, kp=P, vp=P, gl=I32, ws=P2, len_bias=1, B=4, h=8, hd=64, S_max=64, n_split=4,
            prefix=100, prefix_S=128, beams=2, nbytes=AMPLE, ldq=None, ldo=None)
TAKES = {'decode': 'q k v out len ws', 'kv16': 'q k v out len', 'kv16_split': 'q k v out len ws', 'hd': 'q k v out len ws',
         'shared': 'q kp vp k v out len ws', 'shared_groups': 'q kp vp gl k v out len ws', 'shared_kv16': 'q kp vp k v out len ws'}
ALIGNED = {'decode': 'q k v', 'kv16': 'q k v', 'kv16_split': 'q k v ws', 'hd': 'q k v', 'shared': 'q kp vp k v ws',
           'shared_groups': 'q kp vp k v ws', 'shared_kv16': 'q kp vp k v ws'}


def base_args(label, kw):
    return {**BASE, 'hd': 32 if label == 'hd' else 64, **kw}


def entry_call(L, label, **kw):
    """The entry point itself; ldq / ldo default to n_heads * head_dim."""
    a = SimpleNamespace(**base_args(label, kw))
    ldq = a.h * a.hd if a.ldq is None else a.ldq
    ldo = a.h * a.hd if a.ldo is None else a.ldo
    if label == 'decode':
        return L.vh_attn_decode(a.q, ldq, a.k, a.v, a.out, ldo, a.len, a.len_bias, a.B, a.h, a.S_max, a.n_split, a.ws, None)
    if label == 'kv16':
        return L.vh_attn_decode_kv16(a.q, ldq, a.k, a.v, a.out, ldo, a.len, a.len_bias, a.B, a.h, a.S_max, None)
    if label == 'kv16_split':
        return L.vh_attn_decode_kv16_split(a.q, ldq, a.k, a.v, a.out, ldo, a.len, a.len_bias, a.B, a.h, a.S_max, a.n_split, a.ws,
                                           a.nbytes, None)
    if label == 'hd':
        return L.vh_attn_decode_hd(a.q, ldq, a.k, a.v, a.out, ldo, a.len, a.len_bias, a.B, a.h, a.hd, a.S_max, a.hd ** -0.5,
                                   a.n_split, a.ws, a.nbytes, None)
    if label == 'shared_groups':
        return L.vh_attn_decode_shared_groups(a.q, ldq, a.kp, a.vp, a.gl, a.prefix, a.prefix_S, a.k, a.v, a.out, ldo, a.len,
                                              a.len_bias, a.B, a.beams, a.h, a.S_max, a.n_split, a.ws, a.nbytes, None)
    fn = L.vh_attn_decode_shared if label == 'shared' else L.vh_attn_decode_shared_kv16
    return fn(a.q, ldq, a.kp, a.vp, a.prefix, a.prefix_S, a.k, a.v, a.out, ldo, a.len, a.len_bias, a.B, a.h, a.S_max, a.n_split, a.ws,
              a.nbytes, None)


def need_bytes(L, label, **kw):
    a = SimpleNamespace(**base_args(label, kw))
    if label in SHARED:
        return L.vh_attn_decode_shared_ws_bytes(a.B, a.h, a.prefix, a.n_split)
    if label == 'hd':
        return L.vh_attn_decode_hd_ws_bytes(a.B, a.h, a.hd, a.n_split)
    return L.vh_attn_decode_ws_bytes(a.B, a.h, a.n_split)


def refusal_domain(L):
    """(label, fault name, 'entry' or 'query', overrides): the single faults of every entry point."""
    for label in ENTRIES:
        hd = 32 if label == 'hd' else 64
        for p in TAKES[label].split():
            if p != 'ws' or label != 'kv16':
                yield label, f'{p}=null', 'entry', {p: None}
        for p in ALIGNED[label].split():
            yield label, f'{p} misaligned', 'entry', {p: MIS}
        yield label, 'len_bias=2', 'entry', dict(len_bias=2)
        yield label, 'ldq % 4', 'entry', dict(ldq=8 * hd + 2)
        yield label, 'ldq small', 'entry', dict(ldq=8 * hd - 4)
        yield label, 'ldo small', 'entry', dict(ldo=8 * hd - 4)
        if label not in ('decode', 'kv16'):
            yield label, 'ws one byte short', 'query', dict(nbytes=need_bytes(L, label) - 1)
        for dim, bad in (('B', (0,)), ('h', (0,)), ('S_max', (0,)), ('n_split', (0, 17, 65) if label != 'kv16' else ())):
            for v in bad:
                yield label, f'{dim}={v}', 'query', {dim: v}
        if label in SHARED:
            yield label, 'B=65', 'query', dict(B=65)
            for p in (0, 129, 8192):
                yield label, f'prefix={p}', 'query', dict(prefix=p, prefix_S=128 if p < 8192 else 8192)
        if label == 'shared_groups':
            for beams in (0, 3):
                yield label, f'beams={beams}', 'query', dict(beams=beams)
        if label == 'hd':
            for v in (12, 18, 260):
                yield label, f'head_dim={v}', 'query', dict(hd=v)


def refusal_lines(L, call=entry_call, ask=query):
    """`<entry> <fault>: <code> <message>`; an accepted call (n_split = 17 of an fp32 form) is `ok`."""
    out = []
    for label, fault, how, kw in refusal_domain(L):
        if how == 'entry':
            rc = call(L, label, **kw)
        else:
            a = base_args(label, kw)
            o = ask(L, dict(label=label, B=a['B'], h=a['h'], hd=a['hd'], S_max=a['S_max'], prefix=a['prefix'], prefix_S=a['prefix_S'],
                            beams=a['beams']), a['n_split'], a['nbytes'])
            rc = o[1] if o[0] == 'E' else 0
        out.append(f'{label} {fault}: ' + (f'{rc} ' + (L.vh_last_error() or b'').decode() if rc else 'ok'))
    return out


def render(launch, set_knobs, refusals):
    """The fixture's text from launch(shape, n_split) under every knob setting of KNOB_SETS, and the refusal lines."""
    forms, messages, sections = {}, {}, []
    default = None
    for knobs in KNOB_SETS:
        set_knobs(knobs)
        lines = {}
        for s in domain():
            groups = {}
            for n in SPLITS if s['label'] != 'kv16' else (1,):
                o = launch(s, n)
                if o[0] == 'F':
                    token = f'F{forms.setdefault(o[1], len(forms))}/{o[2]}'
                else:
                    token = f'E{messages.setdefault((o[1], o[2].replace(f"n_split={n} ", "n_split={n} ")), len(messages))}'
                groups.setdefault(token, []).append(n)
            key = f'B={s["B"]} h={s["h"]}' + (f' hd={s["hd"]}' if s['label'] == 'hd' else '')
            if s['label'] in SHARED:
                key += f' prefix={s["prefix"]}/{s["prefix_S"]}' + (f' beams={s["beams"]}' if s['label'] == 'shared_groups' else '')
            lines[f'{s["label"]} {key}'] =' '.join(','.join(map(str, ns)) + '=' + t for t, ns in groups.items())
        if default is None:
            default = lines
        else:
            lines = {k: v for k, v in lines.items() if default.get(k) != v}
        sections.append(('[knobs VARIANT=%d WAVES=%d COMBINE=%d]' % knobs, lines))
    set_knobs(KNOB_SETS[0])
    out = ['[forms]'] + [f'F{i} {n}' for n, i in forms.items()]
    out += ['[messages]'] + [f'E{i} {rc} {text}' for (rc, text), i in messages.items()]
    for head, lines in sections:
        out += [head] + [f'{k}: {v}' for k, v in lines.items()]
    out += ['[refusals]'] + refusals()
    return '\n'.join(out) + '\n'


def library_render(L):
    def set_knobs(knobs):
        for knob, v in zip((VARIANT, WAVES, COMBINE), knobs):
            assert L.vh_set_tuning(knob, v) == 0
    try:
        return render(lambda s, n: query(L, s, n), set_knobs, lambda: refusal_lines(L))
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


# compiled kernels no shape reaches, each on purpose: {(kernel, nw, d, lk, nv): reason}
UNREACHED_ON_PURPOSE = {}


def test_plan_stays_inside_the_launcher_and_reaches_every_kernel(L):
    rows = set()
    info = _lib.VhAttnDecodeFormInfo()
    i = 0
    while L.vh_attn_decode_form_row(i, C.byref(info)) == 0:
        row = (info.kernel, info.nw, info.d, info.lk, info.nv)
        assert row not in rows, f'row {i} is listed twice: {row}'
        rows.add(row)
        i += 1
    assert i > 0 and 'vh_attn_decode_form_row' in (L.vh_last_error() or b'').decode()
    reached = set()
    try:
        for knobs in KNOB_SETS:
            for knob, v in zip((VARIANT, WAVES, COMBINE), knobs):
                assert L.vh_set_tuning(knob, v) == 0
            for s in domain():
                for n in SPLITS:
                    if L.vh_attn_decode_form(ENTRIES[s['label']], s['B'], s['h'], s['hd'], s['S_max'], n, s['prefix'], s['prefix_S'],
                                             s['beams'], AMPLE, C.byref(info)) == 0:
                        reached.add((info.kernel, info.nw, info.d, info.lk, info.nv))
    finally:
        for knob in (VARIANT, WAVES, COMBINE):
            L.vh_set_tuning(knob, 0)
    assert reached <= rows, f'the plan returns kernels that are not compiled: {sorted(reached - rows)}'
    assert rows - reached == set(UNREACHED_ON_PURPOSE), f'unreachable rows: {sorted(rows - reached - set(UNREACHED_ON_PURPOSE))}'


@pytest.mark.parametrize('label', list(ENTRIES))
def test_needed_bytes_are_the_ws_bytes_functions(L, label):
    info = _lib.VhAttnDecodeFormInfo()
    for B, h, n_split, prefix, hd in ((1, 1, 1, 1, 16), (4, 8, 2, 100, 32), (4, 8, 8, 1024, 64), (3, 2, 5, 33, 68), (64, 16, 16, 7680, 256)):
        if label == 'kv16':
            n_split = 1
        hd = hd if label == 'hd' else 64
        beams = B if label == 'shared_groups' else 1
        assert L.vh_attn_decode_form(ENTRIES[label], B, h, hd, 64, n_split, prefix, prefix, beams, AMPLE, C.byref(info)) == 0, L.vh_last_error()
        want = need_bytes(L, label, B=B, h=h, n_split=n_split, prefix=prefix, hd=hd)
        assert info.ws_bytes == want, (label, B, h, n_split, prefix, hd)
        assert info.ws_bytes >= info.records * info.record_floats * 4 * B * h
        if info.ws_bytes and label != 'decode':              # exactly enough is taken, one byte less is not
            assert L.vh_attn_decode_form(ENTRIES[label], B, h, hd, 64, n_split, prefix, prefix, beams, want, C.byref(info)) == 0
            assert L.vh_attn_decode_form(ENTRIES[label], B, h, hd, 64, n_split, prefix, prefix, beams, want - 1, C.byref(info)) == -1
            assert 'workspace' in L.vh_last_error().decode()


def test_form_query_argument_checks(L):
    info = _lib.VhAttnDecodeFormInfo()
    assert L.vh_attn_decode_form(7, 4, 8, 64, 64, 1, 0, 0, 1, 0, C.byref(info)) == -1
    assert L.vh_attn_decode_form(-1, 4, 8, 64, 64, 1, 0, 0, 1, 0, C.byref(info)) == -1
    assert L.vh_attn_decode_form(_lib.ATTN_ENTRY_DECODE, 4, 8, 64, 64, 1, 0, 0, 1, 0, None) == -1
    # the answer is the entry point's own: same code, same text
    assert L.vh_attn_decode_form(_lib.ATTN_ENTRY_SHARED_KV16, 4, 8, 64, 32, 16, 7712, 8192, 1, AMPLE, C.byref(info)) == -3
    asked = L.vh_last_error()
    assert entry_call(L, 'shared_kv16', prefix=7712, prefix_S=8192, n_split=16, S_max=32) == -3
    assert L.vh_last_error() == asked and b'256 records' in asked
    assert info.kernel == 0 and info.block == 0
    # a key split of two is combined inside the launch by default: no second launch, ticket words behind the records
    assert L.vh_attn_decode_form(_lib.ATTN_ENTRY_DECODE, 8, 16, 64, 64, 2, 0, 0, 1, 0, C.byref(info)) == 0
    assert info.fused_combine == 1 and info.second == 0 and info.ticket_offset == 8 * 16 * 2 * 72 * 4
    assert info.ws_bytes == info.ticket_offset + 8 * 16 * 4


def test_python_fit_helpers_ask_the_query():
    from valle2_amd import engine
    assert not hasattr(engine, 'SHARED_MAX_RECORDS')
    assert engine.shared_prompt_fits(4, 8, 7680) and not engine.shared_prompt_fits(4, 8, 7681)
    assert engine.grouped_prompts_fit(32, 8, 1024) and not engine.grouped_prompts_fit(32, 8, 8192)


def test_version_is_139(L):
    import re
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 139
    assert 'ABI 139' in (REPO / 'INTEGRATION.md').read_text()


if __name__ == '__main__':
    print(library_render(_lib.load_library()), end='')
