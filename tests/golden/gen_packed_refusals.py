"""The refusal census of the eight entry points that take packed rows: what each refuses, with which code and message,
and — what the single-fault tables of the other tests do not pin — in which ORDER it looks.

    python tests/golden/gen_packed_refusals.py path/to/libvalle_hip.so      (writes tests/golden/packed_refusals.txt)

Needs no device: every call carries at least one fault, so every call ends in a refusal before anything is launched; the
"device pointers" are aligned integers that nothing dereferences.  Per entry there is one representative fault for every
check the entry makes, listed in the order of the checks.  Each fault alone gives a line

    entry | fault | return code | message (vh_last_error)

and every unordered pair of faults a line

    entry | fault A + fault B | the one of the two whose single-fault line the call repeats

The earlier check wins; where both faults change one argument the earlier fault's value stands (n_blocks=0 against
n_blocks=2^30), so that pair carries the earlier fault alone.  A pair that repeats neither line is a mistake in the choice
of faults below, and the script stops there.

The committed file was written by the library as it stood BEFORE the packed front-ends were folded into shared helpers;
tests/test_packed_refusals_cpu.py replays it against the built library line by line.  The one refusal that moved with
that change (vh_transformer_forward_packed: n_blocks x n_heads, which used to come from inside layer 0, behind launches) is
not here but in tests/test_packed_rows_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import itertools
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from valle2_amd import _lib  # noqa: E402

OUT = HERE / 'packed_refusals.txt'
P, P2, P3, P4, P5, I32 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000    # 16-byte aligned, never dereferenced
FULL, PREFIX = 0, 1                                                             # VH_MASK_*
N_LAYERS, BAD_LAYER = 2, 1                                                       # the layer faults sit in the second layer
WORKGROUPS = ('n_blocks=2^30', dict(n_blocks=1 << 30))                          # x n_heads = 2: one past 2^31 - 1


# ---- the four attention entries: arguments in the order of the C signature ---------------------------------------------
def _attn_base(lm=False, lse=False):
    a = dict(q=P, ldq=128, kcache=P2, vcache=P3, out=P4, ldo=128, n_heads=2)
    if lse:
        a.update(M=300)
    a.update(S_max=512)
    if lse:
        a.update(mode=PREFIX)
    a.update(seg_start=I32, seg_len=I32 + 64)
    if lm or lse:
        a.update(seg_x_len=I32 + 128)
    a.update(n_seg=3, blocks=I32 + 192, n_blocks=4)
    if lse:
        a.update(lse2=P5)
    a.update(stream=None)
    return a


_ATTN_SIZES = [('n_seg=0', dict(n_seg=0)), ('n_blocks=0', dict(n_blocks=0)), ('ldq=132', dict(ldq=132)), ('ldo=64', dict(ldo=64))]
_ATTN_FAULTS = ([('kcache=null', dict(kcache=None)), ('blocks=null', dict(blocks=None)), ('S_max=0', dict(S_max=0))] + _ATTN_SIZES +
                [('q+4', dict(q=P + 4)), ('out+8', dict(out=P4 + 8)), ('vcache+4', dict(vcache=P3 + 4)), WORKGROUPS])


def _FP32_LD(faults):
    """16 bytes are 4 floats, not 8 halves: 132 is a good leading dimension there, 130 is not."""
    return [('ldq=130', dict(ldq=130)) if n == 'ldq=132' else (n, kw) for n, kw in faults]


_ATTN_FAULTS_FP32 = _FP32_LD(_ATTN_FAULTS)
_LSE_FAULTS = ([('kcache=null', dict(kcache=None)), ('blocks=null', dict(blocks=None)), ('mode=7', dict(mode=7)),
                ('seg_x_len=null', dict(seg_x_len=None)), ('S_max=299', dict(S_max=299))] +
               _FP32_LD(_ATTN_SIZES) +
               [('out+8', dict(out=P4 + 8)), ('vcache+4', dict(vcache=P3 + 4)), ('lse2+2', dict(lse2=P5 + 2)), WORKGROUPS])


def _call_attn(L, entry, args):
    return getattr(L, entry)(*args.values())


# ---- the four composites: descriptor fields, 'L.' / 'H.' fields of layer BAD_LAYER, and the segment arguments ----------
def _fwd_base(perf, lm):
    a = dict(B=1, T=300, d_model=128, n_heads=2, dff=256, n_layers=N_LAYERS, S_max=320, mode=PREFIX if lm else FULL, x_len=0,
             ln_eps=1e-5, x=P)
    a.update(dict(xn16=P2, q16=P3, attn16=P4, hidden16=P5) if perf else dict(xn=P2, q=P3, attn=P4, hidden=P5))
    a.update(seg_start=I32, seg_len=I32 + 64)
    if lm:
        a.update(seg_x_len=I32 + 128)
    a.update(n_seg=3, blocks=I32 + 192, n_blocks=4)
    if lm and not perf:
        a.update(lse2=P5 + 0x1000)
    return a


_FRONT = [('x=null', dict(x=None)), ('seg_len=null', dict(seg_len=None)), ('B=2', dict(B=2)), ('n_layers=0', dict(n_layers=0)),
          ('S_max=299', dict(S_max=299)), ('n_seg=0', dict(n_seg=0)), ('n_blocks=0', dict(n_blocks=0))]
_MASKS = [('mode=2', dict(mode=2)), ('kv_len', dict(kv_len=I32)), ('x_len_dev', dict(x_len_dev=I32))]
_ADA = ('ada', dict(ada=P))
_FP32_BACK = [('head width 32', dict(n_heads=4)), ('q+4', dict(q=P3 + 4)), ('attn+8', dict(attn=P4 + 8))]
_FP32_LAYERS = [('L.kcache=null', {'L.kcache': 0}), ('L.vcache+4', {'L.vcache': P3 + 4})]
_FP32_NO_MASKS = [('mask', dict(mask=P)), ('pad', dict(pad=P))]
_PERF_BACK = [('d_model=192', dict(d_model=192, n_heads=3)), ('d_model=4224', dict(d_model=4224, n_heads=66)), WORKGROUPS,
              ('x_in+8', dict(x_in=P + 8)), ('q16+4', dict(q16=P3 + 4)), ('H.wo=null', {'H.wo': 0}), ('H.kcache16+4', {'H.kcache16': P2 + 4}),
              ('H.w1+2', {'H.w1': P + 2}), ('L.ln2_g=null', {'L.ln2_g': 0}), ('L.b1+4', {'L.b1': P + 4})]
_FWD_FAULTS = _FRONT + _MASKS + _FP32_NO_MASKS + _FP32_BACK + _FP32_LAYERS       # (its n_blocks x n_heads refusal moved: see above)
_FWD_LM_FAULTS = (_FRONT[:2] + [('lse2=null', dict(lse2=None))] + _FRONT[2:] + _MASKS + _FP32_NO_MASKS + [_ADA] + _FP32_BACK +
                  [('lse2+2', dict(lse2=P5 + 0x1002)), WORKGROUPS] + _FP32_LAYERS)
_FWD16_FAULTS = _FRONT + _MASKS + _PERF_BACK
_FWD16_LM_FAULTS = _FRONT + [('seg_x_len=null', dict(seg_x_len=None))] + _MASKS + [_ADA] + _PERF_BACK


def _call_forward(L, entry, args):
    perf = entry.endswith('_bf16')
    args = dict(args)
    layers, layers16 = (_lib.VhLayer * N_LAYERS)(), (_lib.VhLayer16 * N_LAYERS)()
    for i in range(N_LAYERS):
        for name, _ in _lib.VhLayer._fields_[:13]:                  # LayerNorm parameters, matrices, biases, kcache, vcache
            setattr(layers[i], name, P)
        for name, _ in _lib.VhLayer16._fields_:
            setattr(layers16[i], name, P)
    for key in [k for k in args if k[:2] in ('L.', 'H.')]:
        setattr((layers if key[0] == 'L' else layers16)[BAD_LAYER], key[2:], args.pop(key))
    seg = [args.pop(k) for k in ('seg_start', 'seg_len', 'seg_x_len', 'n_seg', 'blocks', 'n_blocks', 'lse2') if k in args]
    if perf:
        desc = _lib.VhForward16Desc(layers=layers, layers16=layers16, **args)
    else:
        desc = _lib.VhForwardDesc(layers=layers, **args)
    return getattr(L, entry)(C.byref(desc), *seg, None)


# entry -> (how to call it, the arguments nothing is wrong with, its faults in the order of its checks)
ENTRIES = {
    'vh_attn_rows_packed': (_call_attn, _attn_base(), _ATTN_FAULTS_FP32),
    'vh_attn_rows_packed_lse': (_call_attn, _attn_base(lse=True), _LSE_FAULTS),
    'vh_attn_rows_packed_bf16': (_call_attn, _attn_base(), _ATTN_FAULTS),
    'vh_attn_rows_packed_lm_bf16': (_call_attn, _attn_base(lm=True), _ATTN_FAULTS),
    'vh_transformer_forward_packed': (_call_forward, _fwd_base(False, False), _FWD_FAULTS),
    'vh_transformer_forward_packed_lm': (_call_forward, _fwd_base(False, True), _FWD_LM_FAULTS),
    'vh_transformer_forward_packed_bf16': (_call_forward, _fwd_base(True, False), _FWD16_FAULTS),
    'vh_transformer_forward_packed_lm_bf16': (_call_forward, _fwd_base(True, True), _FWD16_LM_FAULTS),
}


def census(L):
    """The lines of packed_refusals.txt as the library L gives them."""
    lines = []
    for entry, (call, base, faults) in ENTRIES.items():
        def refusal(*kws):
            args = dict(base)
            for kw in reversed(kws):                                # the earlier fault's value stands where two meet
                args.update(kw)
            rc = call(L, entry, args)
            assert rc != 0, f'{entry}: a call without a fault ({kws}): it would have launched'
            return '%d | %s' % (rc, (L.vh_last_error() or b'').decode())
        single = {name: refusal(kw) for name, kw in faults}
        assert len(single) == len(faults), f'{entry}: two faults under one name'
        lines += [f'{entry} | {name} | {line}' for name, line in single.items()]
        for (a, kwa), (b, kwb) in itertools.combinations(faults, 2):
            got = refusal(kwa, kwb)
            same = [n for n in (a, b) if single[n] == got]
            assert len(same) == 1, f'{entry}: {a} + {b} gives "{got}", the line of {same or "neither"}'
            lines.append(f'{entry} | {a} + {b} | {same[0]}')
    return lines


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = census(_lib.load_library(sys.argv[1]))
    OUT.write_text('\n'.join(out) + '\n')
    print(f'wrote {OUT} ({len(out)} lines)')
