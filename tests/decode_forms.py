"""The walk over every compiled form of the decode step's two kernel families, shared by tests/test_decode_forms_cpu.py (no
GPU) and tests/test_decode_forms_gpu.py: one case per (FORM_TABLE row, epilogue) of the skinny GEMMs that
test_kernels_gpu._first_shape_of_each_form does not reach, one case per launch form of the seven vh_attn_decode* entry
points, the inputs of both, their float64 references, the bounds, and the plain fp32 emulations (with planted faults) that
show the bounds hold for correct arithmetic and not for a wrong one.

Pure Python at import: the cases come from the two pinned dispatch files (tests/golden/gemm_decode_forms.txt,
tests/golden/attn_decode_forms.txt) and the few shapes those do not hold; no library is loaded.  Which form a case really
takes is asserted against vh_linear_form / vh_attn_decode_form in the CPU file (and again before every GPU launch).

GEMM bounds (u = 2^-24, one fp32 rounding; derivations beside the functions below):
  no LayerNorm, exact rows      every product and partial sum is an integer multiple of 2^-8 below 2^16: the result is exact
  folded LayerNorm, exact rows  2^-21 (|rstd A| + |c2|): five roundings (eps add, rsqrt, product, final add), eight allowed
  LayerNorm in the operand load 6 u sum_k |w| (|x sc| + |sc mean|) + 2 u sum_k |w| (|beta| + |xhat|) + (K + 2) u sum_k |xhat w|
  ordinary rows                 the project's atol 2e-5 / rtol 1e-5; above K = 1024 twice the unfused route's error
"""
import math
import re
from collections import namedtuple
from pathlib import Path

import torch

GOLDEN = Path(__file__).resolve().parent / 'golden'
U = 2.0 ** -24
EPS = 1e-5

# ======================================================================================================================
# GEMM: the cases
# ======================================================================================================================
GEMM_KNOBS = (2, 9, 4)                                      # VH_TUNE_ROW_GROUPS, VH_TUNE_LN_STATS, VH_TUNE_TILE_DMA
# label -> (VH_ENTRY_*, VH_LN_*, w16) as tests/test_gemm_forms_cpu.ENTRIES (numbers of include/valle_hip.h: no import here)
GEMM_ENTRIES = {'linear': (0, 0, 0), 'linear+ln': (0, 1, 0), 'linear_folded': (0, 2, 0), 'linear_w16': (0, 0, 1),
                'linear_ws': (4, 0, 0), 'head_greedy': (5, 0, 0), 'qkv': (1, 0, 0), 'qkv+ln': (1, 1, 0), 'qkv_folded': (1, 2, 0),
                'qkv_folded_kv16': (3, 2, 0), 'qkv_folded_kv16_w16': (3, 2, 1), 'qkv_hd': (2, 0, 0), 'qkv_hd+ln': (2, 1, 0),
                'qkv_folded_hd': (2, 2, 0)}
WALKED_LABELS = ('linear', 'linear_ws', 'qkv', 'qkv_hd')    # test_kernels_gpu._first_shape_of_each_form's
# the pinned domain has no d_model that is a multiple of 64 but not of 128 below 1024: the QKV products without LayerNorm reach
# the guarded kernel's eight-wave forms at d_model = 192 only (tests/test_gemm_forms_cpu adds the same shape to its walk)
GEMM_EXTRA = [(label, M, 576, 192, 1, f'generic<{mt},8,{epi},4,0,0,0> b=512')
              for label, epi in (('qkv', 1), ('qkv_hd', 5)) for M, mt in ((1, 1), (17, 2), (33, 4))]
GemmCase = namedtuple('GemmCase', 'form label M N K T knobs')


def gemm_golden_lines():
    """(knobs, label, N, K, T, [(M, form name)]) of every line of the pinned GEMM dispatch; refusals left out."""
    text = (GOLDEN / 'gemm_decode_forms.txt').read_text().splitlines()
    names = {m.group(1): m.group(2) + ' ' + m.group(3) for m in (re.match(r'(F\d+) (\S+) (b=\d+)$', ln) for ln in text) if m}
    knobs = None
    for ln in text:
        m = re.match(r'\[knobs ROW_GROUPS=(\d) LN_STATS=(\d) TILE_DMA=(\d)\]', ln)
        if m:
            knobs = tuple(map(int, m.groups()))
            continue
        m = re.match(r'(\S+) N=(\d+) K=(\d+) T=(\d+): (.*)', ln)
        if knobs is None or not m:
            continue
        rows = []
        for group in m.group(5).split():
            ms, token = group.split('=')
            if token[0] == 'F':
                rows += [(int(M), names[token.split('/')[0]]) for M in ms.split(',')]
        yield knobs, m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), rows


def is_skinny(form):
    return form.startswith(('fast<', 'generic<'))


def gemm_form_tuple(form):
    """(family, mt, nw, pw, ln, nj, w16, epi) of a skinny form's name: a (FORM_TABLE row, epilogue) pair."""
    fam, args = re.match(r'(fast|generic)<([\d,]+)>', form).groups()
    mt, nw, epi, pw, ln, nj, w16 = map(int, args.split(','))
    return (1 if fam == 'fast' else 2, mt, nw, pw, ln, nj, w16, epi)


def gemm_walked_forms():
    """The skinny forms the existing integer walk runs (the first shape of each form of WALKED_LABELS in the pinned file)."""
    return {form for _, label, _, _, _, rows in gemm_golden_lines() if label in WALKED_LABELS for _, form in rows if is_skinny(form)}


def gemm_head_forms():
    """head<...>: with test_head_greedy_one_launch_equals_head_then_greedy_step."""
    return {form for _, label, _, _, _, rows in gemm_golden_lines() if label == 'head_greedy' for _, form in rows}


def gemm_cases():
    """One case per skinny form outside the existing walk: default knobs before a knob, then the fewest rows, the smallest K."""
    walked, best = gemm_walked_forms(), {}
    lines = [(kn, lb, N, K, T, rows) for kn, lb, N, K, T, rows in gemm_golden_lines() if lb not in WALKED_LABELS + ('head_greedy',)]
    lines += [((0, 0, 0), lb, N, K, T, [(M, form)]) for lb, M, N, K, T, form in GEMM_EXTRA]
    for knobs, label, N, K, T, rows in lines:
        for M, form in rows:
            if not is_skinny(form) or form in walked:
                continue
            rank = (knobs != (0, 0, 0), M, K, N, T, knobs)
            if form not in best or rank < best[form][0]:
                best[form] = (rank, GemmCase(form, label, M, N, K, T, knobs))
    return [c for _, c in sorted(best.values(), key=lambda rc: (rc[1].label, rc[1].form))]


def gemm_case_id(c):
    return f'{c.form.split(" ")[0]}-{c.label}-M{c.M}-K{c.K}-T{c.T}' + ('' if c.knobs == (0, 0, 0) else '-knobs' + ''.join(map(str, c.knobs)))


def gemm_ln(c):
    """0 none, 1 in the operand load, 2 folded with row-resident statistics, 3 folded with fragment statistics."""
    return gemm_form_tuple(c.form)[4]


def gemm_head_dim(c):
    return (48 if c.K == 192 else 32) if '_hd' in c.label else 64


# ======================================================================================================================
# GEMM: inputs, references, bounds
# ======================================================================================================================
def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def exact_rows(M, K, rot, gen):
    """Rows of three kinds, permuted per row (row r is of kind (r + rot) % 3): +-1 (mean 0, variance 1), {-1, +3} in equal
    parts (mean 1, variance 4: a missing mean c1 shows), 5 +- 2^-8 (variance 2^-16, comparable to eps: a missing eps shows)."""
    x = torch.empty(M, K)
    half = torch.arange(K) % 2 == 0
    for r in range(M):
        kind = (r + rot) % 3
        lo, hi = ((-1.0, 1.0), (-1.0, 3.0), (5.0 - 2.0 ** -8, 5.0 + 2.0 ** -8))[kind]
        x[r] = torch.where(half, torch.tensor(lo), torch.tensor(hi))[torch.randperm(K, generator=gen)]
    return x


def gemm_exact_inputs(c, rot):
    """x, w, bias, gamma, beta of the exact rows: small integers everywhere but in x.  Every product x Wf is a multiple of 2^-8
    and sum_k |x Wf| < 2^16 (asserted), so every partial sum of the products, in any order, is exact in fp32; so are the row sums
    (< 2^15 in multiples of 2^-8) and the centred squares (1, 4 or 2^-16)."""
    gen = _gen(11, c.M, c.N, c.K, rot)
    ln = gemm_ln(c)
    x = exact_rows(c.M, c.K, rot, gen)
    w = torch.randint(-2, 3, (c.N, c.K), generator=gen).float()
    w[:, 0] += torch.arange(c.N).float() % 3                     # asymmetric: no column is another's mirror
    has_bias = ln >= 2 or c.label in ('linear+ln', 'linear_w16')
    bias = torch.randint(-2, 3, (c.N,), generator=gen).float() if has_bias else None
    gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (c.K,), generator=gen)] if ln else None
    beta = torch.randint(-1, 2, (c.K,), generator=gen).float() if ln else None
    wf = w * gamma if ln else w
    assert float((x.abs() @ wf.abs().T).max()) < 2.0 ** 16
    return x, w, bias, gamma, beta


def gemm_ordinary_inputs(c):
    """randn + 0.3 rows, weights of the model's scale, a bias where the entry has one and a residual where it takes one."""
    gen = _gen(23, c.M, c.N, c.K)
    ln = gemm_ln(c)
    x = torch.randn(c.M, c.K, generator=gen) + 0.3
    w = 0.05 * torch.randn(c.N, c.K, generator=gen)
    has_bias = ln >= 2 or c.label in ('linear+ln', 'linear_w16')
    bias = torch.randn(c.N, generator=gen) if has_bias else None
    gamma = 1 + 0.1 * torch.randn(c.K, generator=gen) if ln else None
    beta = 0.1 * torch.randn(c.K, generator=gen) if ln else None
    res = torch.randn(c.M, c.N, generator=gen) if c.label in ('linear+ln', 'linear_folded', 'linear_w16') else None
    return x, w, bias, gamma, beta, res


def gemm_takes_act(c):
    return c.label in ('linear+ln', 'linear_folded')


def gelu64(y):
    return 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0)))


def row_stats64(x):
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return mean, var, 1 / torch.sqrt(var + EPS)


def gemm_reference(x, w, bias=None, gamma=None, beta=None, act=False, res=None):
    """float64: LayerNorm (where gamma is given) -> Linear -> GELU -> residual.  w is the matrix as the kernel multiplies by it
    (a 16-bit-weight form: rounded first, by the caller)."""
    y = x.double()
    if gamma is not None:
        mean, _, rstd = row_stats64(x)
        y = (y - mean) * rstd * gamma.double() + beta.double()
    y = y @ w.double().T
    if bias is not None:
        y = y + bias.double()
    if act:
        y = gelu64(y)
    return y if res is None else y + res.double()


def gemm_reference_folded(x, wf, c2, act=False, res=None):
    """The same through a folded matrix wf = W o gamma AS STORED (fp32, or rounded to the 16-bit format) and c2 = beta W^T + bias
    in float64: what a kernel that reads wf is to be measured against."""
    mean, _, rstd = row_stats64(x)
    y = ((x.double() - mean) * rstd) @ wf.double().T + c2.double()
    if act:
        y = gelu64(y)
    return y if res is None else y + res.double()


def folded_exact_bound(x, w, bias, gamma, beta):
    """Per element, for the exact rows through a folded form (LN 2 and LN 3), out = rstd A + c2 with A = (x - mean) Wf^T:
    the statistics (sums of multiples of 2^-8 below 2^15, a division by K whose quotient is representable, centred squares
    1 / 4 / 2^-16), the products and A itself are exact in fp32 — with the shift of the fragment and the 640 / 768 / 896 forms
    too, a multiple of 2^-13 near the mean.  What rounds: var + eps and eps itself (together at most u on the radicand, u / 2 on
    rstd), the hardware reciprocal square root (one unit in the last place: 2 u), the product rstd A (u) and the sum with c2 (u
    of the result): 4.5 u |rstd A| + u |c2| at most.  Allowed: 8 u (|rstd A| + |c2|) = 2^-21 (|rstd A| + |c2|), and the float64
    reference's own error, 2^-45 of the magnitudes it adds."""
    mean, _, rstd = row_stats64(x)
    xn, wf = (x.double() - mean) * rstd, (w * gamma).double()
    ra = xn @ wf.T
    c2 = beta.double() @ w.double().T + (bias.double() if bias is not None else 0)
    own = 2.0 ** -45 * (xn.abs() @ wf.abs().T + c2.abs())          # the float64 reference's own rounding (an element may be 0 exactly)
    return ra + c2, 2.0 ** -21 * (ra.abs() + c2.abs()) + own


def operand_ln_bound(x, w, bias, gamma, beta):
    """Per element, for a form that normalises the operand in its load (LN 1): xhat = x sc + (beta - sc mean), sc = gamma rstd.
    rstd carries 3 u (statistics of these rows are exact, then as above), sc one more, each of x sc and sc mean one more:
    5 u (|x sc| + |sc mean|), the inner difference and the outer sum one each of their results: at most
    d_k = 6 u (|x sc| + |sc mean|) + 2 u (|beta| + |xhat|) on element k — on the 5 +- 2^-8 rows that is 2e-4 of an xhat of 0.8: the
    cancellation of x sc against sc mean is this form's own, and the bound says so.  The product xhat W^T is an fp32 dot product
    of K terms in some order: (K - 1) u sum_k |xhat w|, three more for the bias and the stores: (K + 2) u."""
    mean, _, rstd = row_stats64(x)
    sc = rstd * gamma.double()
    xhat = (x.double() - mean) * sc + beta.double()
    d = 6 * U * ((x.double() * sc).abs() + (sc * mean).abs()) + 2 * U * (beta.double().abs() + xhat.abs())
    wa = w.double().abs()
    ref = xhat @ w.double().T + (bias.double() if bias is not None else 0)
    return ref, d @ wa.T + (x.shape[1] + 2) * U * (xhat.abs() @ wa.T)


def gemm_exact_bound(c, x, w, bias, gamma, beta):
    """(float64 reference, bound per element) of the exact rows of case c; the bound is 0 without a LayerNorm."""
    ln = gemm_ln(c)
    if ln == 0:
        ref = gemm_reference(x, w, bias)
        return ref, torch.zeros_like(ref)
    return (operand_ln_bound if ln == 1 else folded_exact_bound)(x, w, bias, gamma, beta)


def scatter_qkv(y, cache_len, T, h, hd, S, sentinel, ldq, fault=None):
    """What a QKV epilogue leaves of the (B T, 3 d) product y: q in a NaN buffer (B T, ldq), the K / V columns of row (b, t) at
    cache row cache_len[b] + t of sentinel-filled caches (B, h, S, hd)."""
    d = h * hd
    B = y.shape[0] // T
    q = torch.full((B * T, ldq), float('nan'), dtype=y.dtype)
    q[:, :d] = y[:, :d]
    kc = torch.full((B, h, S, hd), float(sentinel[0]), dtype=y.dtype)
    vc = torch.full((B, h, S, hd), float(sentinel[1]), dtype=y.dtype)
    kcols, vcols = (y[:, 2 * d:], y[:, d:2 * d]) if fault == 'kv_swapped' else (y[:, d:2 * d], y[:, 2 * d:])
    if fault == 'head_shifted':                                  # the column groups of a head land one group (4 columns) further on
        kcols, vcols = torch.roll(kcols, 4, 1), torch.roll(vcols, 4, 1)
    for b in range(B):
        for t in range(T):
            at = int(cache_len[b]) + t + (fault == 'row_plus_one')
            kc[b, :, at] = kcols[b * T + t].view(h, hd)
            vc[b, :, at] = vcols[b * T + t].view(h, hd)
    return q, kc, vc


def stored16_outside(got16, want, tol):
    """How many elements of a 16-bit append lie outside what a correct kernel can store.  The kernel rounds an fp32 value y'
    with |y' - want| <= tol once, and rounding is monotonic: round16(want - tol) <= stored <= round16(want + tol).  Where tol is
    below half a unit of the 16-bit format that is "within one unit in the last place of the float64 value rounded to the
    format", the check this replaces; that one cannot hold where the value itself is a cancellation: on the +-1 exact rows
    rstd A + c2 = 10 (1 - rstd) = 5e-5 carries an fp32 error of up to 1e-5, a hundred units of fp16's 6e-8 there (plain fp32
    torch lands 7 units away).  tol == 0 (away from the new row): the bits of `want`."""
    lo, hi = (want.double() - tol.double()).to(got16.dtype).float(), (want.double() + tol.double()).to(got16.dtype).float()
    g = got16.float()
    return int(((g < lo) | (g > hi) | torch.isnan(g)).sum())


def gemm_cache_len(c, S):
    B = c.M // c.T
    return torch.randint(0, S - c.T - 1, (B,), generator=_gen(31, c.M, c.K), dtype=torch.int32)   # (a row to spare: the row_plus_one fault stays inside)


# ---- plain fp32 emulations of the three arithmetics, with the planted faults ---------------------------------------------------
GEMM_FAULTS = ('no_mean_c1', 'no_c2', 'no_eps', 'slab_dropped', 'slab_twice', 'tile2_stats_of_tile1', 'kv_swapped', 'row_plus_one',
               'head_shifted')


def emulate_gemm(ln, x, w, bias, gamma, beta, fault=None, nw=8):
    """fp32 torch: ln 2 two-pass row statistics and the folded epilogue; ln 3 one-pass statistics about the mean of the row's
    first 32 elements, products on x - shift; ln 1 operands normalised before the products.  (torch's own summation order.)"""
    x, w = x.float(), w.float()
    K = x.shape[1]
    eps = 0.0 if fault == 'no_eps' else EPS
    keep = torch.ones(K)
    if fault in ('slab_dropped', 'slab_twice'):                  # one 16 NW slab of K, the second where there is one
        s0 = 16 * nw if K > 16 * nw else 0
        keep[s0:s0 + 16 * nw] = 0.0 if fault == 'slab_dropped' else 2.0
    bias = torch.zeros(w.shape[0]) if bias is None else bias.float()

    def other_tile(t):                                           # rows 16.. take the statistics of rows 0..15
        if fault == 'tile2_stats_of_tile1':
            idx = torch.arange(t.shape[0])
            idx[16:] = idx[16:] % 16
            t = t[idx]
        return t
    if ln == 1:
        mean = x.sum(1, keepdim=True) / K
        var = ((x - mean) ** 2).sum(1, keepdim=True) / K
        rstd = torch.rsqrt(var + eps)
        mean, rstd = other_tile(mean), other_tile(rstd)
        sc = gamma * rstd
        xhat = x * sc + ((beta if fault != 'no_c2' else 0 * beta) - sc * (mean if fault != 'no_mean_c1' else 0 * mean))
        return (xhat * keep) @ w.T + bias
    wf = w * gamma
    c1 = wf.sum(1)
    c2 = (beta @ w.T + bias) if fault != 'no_c2' else torch.zeros(w.shape[0])
    if ln == 2:
        shift = torch.zeros(x.shape[0], 1)
        mean = x.sum(1, keepdim=True) / K
        var = ((x - mean) ** 2).sum(1, keepdim=True) / K
    else:
        shift = x[:, :32].sum(1, keepdim=True) * (1.0 / 32.0)
        t = x - shift
        mean = t.sum(1, keepdim=True) / K                        # mean - shift
        var = torch.clamp((t * t).sum(1, keepdim=True) / K - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + eps)
    mean, rstd = other_tile(mean), other_tile(rstd)
    acc = ((x - shift) * keep) @ wf.T
    if fault != 'no_mean_c1':                                    # (ln 3: the products ran on x - shift, the term is (mean - shift) c1)
        acc = acc - mean * c1
    return acc * rstd + c2


# ======================================================================================================================
# Attention: the cases
# ======================================================================================================================
ATTN_KNOBS = (0, 1, 12)                                     # VH_TUNE_DECODE_VARIANT, _WAVES, _COMBINE
ATTN_ENTRIES = {'decode': 0, 'kv16': 1, 'kv16_split': 2, 'shared': 3, 'shared_groups': 4, 'shared_kv16': 5, 'hd': 6}
SHARED = ('shared', 'shared_groups', 'shared_kv16')
KV16 = ('kv16', 'kv16_split', 'shared_kv16')
AttnCase = namedtuple('AttnCase', 'form entry B h head_dim n_split prefix beams knobs')
PREFIXES = (1, 31, 32, 33, 127, 128, 129, 160)              # the edges of a 32-key block and of a workgroup's four blocks
PREFIX_CAP = 160
LENGTHS = {104: (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 104), 8: (1, 2, 3, 4, 5, 6, 7, 8)}   # S_max -> the rows' lengths, cycled
SCORE_SETS = ('plain', 'peak', 'rising', 'falling', 'plus200', 'minus200')


def attn_golden_lines():
    """(knobs, entry, B, h, head_dim, prefix, prefix_S, beams, [(n_split, launch name)]) of the pinned attention dispatch."""
    text = (GOLDEN / 'attn_decode_forms.txt').read_text().splitlines()
    names = {m.group(1): m.group(2) for m in (re.match(r'(F\d+) (attn_.*)$', ln) for ln in text) if m}
    knobs = None
    for ln in text:
        m = re.match(r'\[knobs VARIANT=(\d+) WAVES=(\d+) COMBINE=(\d+)\]', ln)
        if m:
            knobs = tuple(map(int, m.groups()))
            continue
        if ln.startswith('[refusals]'):
            return
        m = re.match(r'(\w+) B=(\d+) h=(\d+)(?: hd=(\d+))?(?: prefix=(\d+)/(\d+))?(?: beams=(\d+))?: (.*)', ln)
        if knobs is None or not m:
            continue
        launches = []
        for group in m.group(8).split():
            ns, token = group.split('=')
            if token[0] == 'F':
                launches += [(int(n), names[token.split('/')[0]]) for n in ns.split(',')]
        yield (knobs, m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4) or 64), int(m.group(5) or 0), int(m.group(6) or 0),
               int(m.group(7) or 1), launches)


def attn_launch_form(entry, name, n_split):
    """A launch form: entry point, first kernel with its template arguments, and how the split records are added — ' + <second
    kernel>' in the pinned name, or inside the launch (a key split of the burst kernel without a second launch)."""
    fused = ' + in-launch combine' if n_split > 1 and ' + ' not in name and entry == 'decode' else ''
    return f'{entry}: {name}{fused}'


def attn_cases():
    """One case per launch form, default knobs before a knob, then the smallest B h n_split.  The shared-prompt forms take 33
    rows (a second lane pass), two heads and three suffix splits whatever the first pinned shape is: their form does not depend
    on the shape; the groups form takes 36 rows as 9 groups of 4 beams (and runs again as 36 groups of 1)."""
    best = {}
    for knobs, entry, B, h, hd, prefix, prefix_S, beams, launches in attn_golden_lines():
        for n, name in launches:
            form = attn_launch_form(entry, name, n)
            rank = (knobs != (0, 0, 0), B * h * n, B, n, hd, prefix, knobs)
            if form not in best or rank < best[form][0]:
                best[form] = (rank, AttnCase(form, entry, B, h, hd, n, prefix, beams, knobs))
    cases = []
    for _, c in sorted(best.values(), key=lambda rc: rc[0]):
        if c.entry in SHARED:
            c = c._replace(B=36 if c.entry == 'shared_groups' else 33, h=2, n_split=3, prefix=PREFIX_CAP,
                           beams=4 if c.entry == 'shared_groups' else 1)
        cases.append(c)
    return cases


def attn_case_id(c):
    name = c.form.replace('attn_', '').replace('_kernel', '').replace(' b=', '/').replace(': ', '-').replace(' + ', '+').replace(' ', '_')
    return f'{name}-B{c.B}-h{c.h}-hd{c.head_dim}-n{c.n_split}' + ('' if c.knobs == (0, 0, 0) else '-knobs' + '.'.join(map(str, c.knobs)))


def attn_runs(c):
    """The (S_max, len_bias, prefix selector, beams) combinations one case runs, each on every score set.  Without a prompt: both
    caches x both len_bias.  With one: every prefix length of PREFIXES, the cache and len_bias alternating (each pair twice);
    the groups form gives every group its own length (the list rotated by the selector, some groups parked) at 4 beams, at 1 and
    as one group of 36."""
    if c.entry not in SHARED:
        return [(S, bias, None, 1) for S in (104, 8) for bias in (1, 0)]
    if c.entry == 'shared_groups':                                # (36 beams: one group whose beams 32..35 are the second lane pass)
        combos = [(b, S, bias) for b in (c.beams, 1) for S in (104, 8) for bias in (1, 0)] + [(c.B, 104, 1), (c.B, 8, 0)]
        return [(S, bias, i, beams) for i, (beams, S, bias) in enumerate(combos)]
    return [((104, 8)[i % 2], (1, 0)[i // 2 % 2], i, 1) for i in range(len(PREFIXES))]


# ======================================================================================================================
# Attention: inputs, reference, emulations
# ======================================================================================================================
def attn_inputs(c, S, bias, sel, beams, score_set, h16=None):
    """One run's operands on the CPU, fp32 (the 16-bit forms: K / V already rounded to h16, held as fp32).
    rows: R = a multiple of B covering every length of LENGTHS[S]; a launch takes B consecutive rows.  q (R, h, hd);
    k, v (R, h, S, hd) and, with a prompt, kp, vp (G, h, PREFIX_CAP + 32, hd), random everywhere (the GPU copies get NaN / Inf
    beyond the lengths); length (R,) keys attended of the row's own cache (0: an empty suffix, groups form at len_bias 0 only),
    plen (G,) (0: a parked group).
    Score sets: to the row's keys a multiple of q / |q|^2 is added, to a prompt's keys (which every row of the group sees) a
    multiple of a unit vector e on which every q of the head has the same component 4, so that key j's score moves by what is
    asked for: nothing (plain), +6 at the last key but one and +4 at the second (peak), +j / -j over prompt and own keys
    (rising / falling), +200 / -200 everywhere."""
    hd, h, B = c.head_dim, c.h, c.B
    lens = LENGTHS[S]
    R = B * ((len(lens) + B - 1) // B)
    gen = _gen(41, ATTN_ENTRIES[c.entry], B, h, hd, S, bias, -1 if sel is None else sel, beams, SCORE_SETS.index(score_set))
    scale = hd ** -0.5
    q = torch.randn(R, h, hd, generator=gen)
    k = torch.randn(R, h, S, hd, generator=gen)
    v = torch.randn(R, h, S, hd, generator=gen)
    length = torch.tensor([lens[r % len(lens)] for r in range(R)], dtype=torch.int32)
    out = dict(R=R, scale=scale, S=S, bias=bias, beams=beams, hd=hd)
    plen_row = torch.zeros(R, dtype=torch.int64)
    if c.entry in SHARED:
        e = torch.nn.functional.normalize(torch.randn(h, hd, generator=gen), dim=-1)
        q = q - (q * e).sum(-1, keepdim=True) * e + 4.0 * e                      # q . e = 4 in every row
        if c.entry == 'shared_groups':
            G = R // beams
            plen = torch.tensor([PREFIXES[(g + sel) % len(PREFIXES)] for g in range(G)], dtype=torch.int32)
            if G > 1:
                plen[1::7] = 0                                                   # parked groups
            if bias == 0:
                length[0] = 0                                                    # an empty suffix: the prompt's keys only
                plen[0] = max(int(plen[0]), 1)
            grp, lane = torch.arange(R) // beams, torch.arange(R) % beams
        else:
            G, plen, grp, lane = 1, torch.tensor([PREFIXES[sel]], dtype=torch.int32), torch.zeros(R, dtype=torch.int64), torch.arange(R) % B
        kp = torch.randn(G, h, PREFIX_CAP + 32, hd, generator=gen)
        vp = torch.randn(G, h, PREFIX_CAP + 32, hd, generator=gen)
        plen_row = plen.long()[grp]
        out.update(e=e, G=G, plen=plen, grp=grp, lane=lane)
    # the score each key is moved by: positions count over prompt + own keys
    P = PREFIX_CAP + 32 if c.entry in SHARED else 0
    pos_p = torch.arange(P).float()                                              # prompt key j
    pos_s = plen_row[:, None].float() + torch.arange(S).float()[None]            # own key j of row r: after the row's prompt
    total = plen_row + length.long()
    if score_set == 'plain':
        add_p, add_s = torch.zeros(P), torch.zeros(R, S)
    elif score_set in ('rising', 'falling'):
        sign = 1.0 if score_set == 'rising' else -1.0
        add_p, add_s = sign * pos_p, sign * pos_s
    elif score_set in ('plus200', 'minus200'):
        sign = 200.0 if score_set == 'plus200' else -200.0
        add_p, add_s = torch.full((P,), sign), torch.full((R, S), sign)
    else:                                                                        # peak: the last key but one of the row, the second key
        add_p = torch.zeros(P)
        if P:
            add_p[1] = 4.0
        late = torch.clamp(total - 2, min=0)[:, None]
        add_s = 6.0 * (pos_s == late) + (4.0 * (pos_s == 1) if not P else 0.0)
    k = k + (add_s / scale)[:, None, :, None] * (q / (q * q).sum(-1, keepdim=True))[:, :, None, :]
    if P:
        kp = kp + (add_p / (4.0 * scale))[None, None, :, None] * e[None, :, None, :]
    if h16 is not None:
        k, v = k.to(h16).float(), v.to(h16).float()
        if P:
            kp, vp = kp.to(h16).float(), vp.to(h16).float()
    out.update(q=q, k=k, v=v, length=length)
    if P:
        out.update(kp=kp, vp=vp)
    return out


ATTN_FAULTS = ('key_beyond', 'last_key_dropped', 'len_bias_ignored', 'empty_split_max_0', 'no_rescale', 'exp_before_max',
               'prefix_block_whole', 'group0_prefix', 'second_pass_columns')


def _attn_masks(inp, fault=None):
    """(own-key mask (R, S), prompt mask (R, P) or None, rows that attend nothing): what each row attends."""
    S, R = inp['S'], inp['R']
    n = inp['length'].long()
    if fault == 'key_beyond':
        n = torch.clamp(n + 1, max=S)
    if fault == 'last_key_dropped':
        n = torch.clamp(n - 1, min=0)
    if fault == 'len_bias_ignored' and inp['bias'] == 0:         # cache_len + 1 whatever len_bias says
        n = torch.clamp(n + 1, max=S)
    own = torch.arange(S)[None] < n[:, None]
    if 'plen' not in inp:
        return own, None, torch.zeros(R, dtype=torch.bool)
    plen = inp['plen'].long()
    parked = (plen == 0)[inp['grp']]
    if fault == 'group0_prefix':
        plen = torch.where(plen > 0, plen[0].expand_as(plen), plen)
    if fault == 'prefix_block_whole':
        plen = (plen + 31) // 32 * 32
    pm = torch.arange(inp['kp'].shape[2])[None] < plen[inp['grp']][:, None]
    own = own & ~parked[:, None]
    return own, pm & ~parked[:, None], parked


def _scores(inp, dtype, fault=None):
    """(R, h, P + S) scores q . k scale over prompt then own keys, and the matching V (R, h, P + S, hd)."""
    q, k, v = inp['q'].to(dtype), inp['k'].to(dtype), inp['v'].to(dtype)
    s = torch.einsum('rhd,rhsd->rhs', q, k)
    if 'kp' in inp:
        kp, vp, grp = inp['kp'].to(dtype)[inp['grp']], inp['vp'].to(dtype)[inp['grp']], inp['grp']
        qp = q
        if fault == 'second_pass_columns':                       # columns 32.. of a score tile score the prompt with the first pass's queries
            rows = torch.arange(inp['R'])
            qp = q[torch.where(inp['lane'] >= 32, rows - 32, rows)]
        s = torch.cat([torch.einsum('rhd,rhsd->rhs', qp, kp), s], dim=2)
        v = torch.cat([vp, v], dim=2)
    return s * inp['scale'], v


def attn_reference(inp, dtype=torch.float64, fault=None):
    """softmax(q K^T scale) V over the attended keys in `dtype` (float64: the reference; float32: the plain emulation); a row
    that attends nothing (a parked group) is exactly 0."""
    own, pm, parked = _attn_masks(inp, fault)
    mask = own if pm is None else torch.cat([pm, own], dim=1)
    s, v = _scores(inp, dtype, fault)
    s = s.masked_fill(~mask[:, None, :], float('-inf'))
    p = torch.softmax(s, dim=-1)
    p = torch.where(mask[:, None, :], p, torch.zeros_like(p))
    out = torch.einsum('rhs,rhsd->rhd', p, v)
    out[parked | ~mask.any(1)] = 0
    return out


def attn_emulate_chunked(inp, n_split, fault=None):
    """fp32, the kernels' scheme: scores in base 2, an online softmax over 32-key chunks, one record (max, sum, accumulator) per
    32-key block of a prompt and per key split of the row's own keys (ranges of whole chunks, the last splits possibly empty),
    the records merged in order."""
    LOG2E = 1.4426950408889634
    own, pm, parked = _attn_masks(inp, fault)
    s, v = _scores(inp, torch.float32, fault)
    s = s * LOG2E
    R, h, _ = s.shape
    P = 0 if pm is None else pm.shape[1]
    S = own.shape[1]
    pad = (-S) % 32
    mask = own if pm is None else torch.cat([pm, own], dim=1)
    if pad:
        s = torch.cat([s, torch.zeros(R, h, pad)], dim=2)
        v = torch.cat([v, torch.zeros(R, h, pad, v.shape[-1])], dim=2)
        mask = torch.cat([mask, torch.zeros(R, pad, dtype=torch.bool)], dim=1)
    s = s.masked_fill(~mask[:, None, :], float('-inf'))
    v = torch.where(mask[:, None, :, None], v, torch.zeros_like(v))
    n_own = own.sum(1)
    chunks = (n_own + 31) // 32
    per = torch.clamp((chunks + n_split - 1) // n_split, min=1)
    records = []
    for seg in range(P // 32 + n_split):
        m = torch.full((R, h), float('-inf'))
        l = torch.zeros(R, h)
        acc = torch.zeros(R, h, v.shape[-1])
        for ch in range((P + S + pad) // 32):
            if ch < P // 32:
                active = torch.full((R,), ch == seg)
            else:
                active = ((ch - P // 32) // per == seg - P // 32) & torch.tensor(seg >= P // 32)
            active = active & mask[:, ch * 32:ch * 32 + 32].any(1)
            if not bool(active.any()):
                continue
            sc, vc = s[:, :, ch * 32:ch * 32 + 32], v[:, :, ch * 32:ch * 32 + 32]
            m_new = torch.maximum(m, sc.max(-1).values)
            safe = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
            alpha = torch.ones_like(m) if fault == 'no_rescale' else torch.where(torch.isfinite(m), torch.exp2(m - safe), torch.zeros_like(m))
            p = torch.exp2(sc) / torch.exp2(safe)[..., None] if fault == 'exp_before_max' else torch.exp2(sc - safe[..., None])
            l_new = l * alpha + p.sum(-1)
            acc_new = acc * alpha[..., None] + torch.einsum('rhs,rhsd->rhd', p, vc)
            a2 = active[:, None]
            m, l, acc = torch.where(a2, m_new, m), torch.where(a2, l_new, l), torch.where(a2[..., None], acc_new, acc)
        records.append((m, l, acc))
    ms = torch.stack([r[0] for r in records])
    if fault == 'empty_split_max_0':
        ms = torch.where(torch.isfinite(ms), ms, torch.zeros_like(ms))
    top = ms.max(0).values
    safe = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    wgt = torch.where(torch.isfinite(ms), torch.exp2(ms - safe), torch.zeros_like(ms))
    den = sum(r[1] * wgt[i] for i, r in enumerate(records))
    num = sum(r[2] * wgt[i][..., None] for i, r in enumerate(records))
    out = num / den[..., None]
    out[parked] = 0
    return out


def worst(a, b):
    """max |a - b|, infinite where one side is not finite and the other is (or differs)."""
    a, b = a.double(), b.double()
    d = (a - b).abs()
    d = torch.where(torch.isfinite(a) & torch.isfinite(b), d, torch.where((a == b) | (torch.isnan(a) & torch.isnan(b)), torch.zeros_like(d),
                                                                         torch.full_like(d, float('inf'))))
    return float(d.max())


# ======================================================================================================================
# The library's own answer (L: the loaded library; nothing is launched)
# ======================================================================================================================
def set_knobs(L, which, values):
    for knob, v in zip(which, values):
        assert L.vh_set_tuning(knob, v) == 0


def gemm_query_form(L, c, M=None):
    """The form name, as the pinned file writes it, that vh_linear_form returns for case c under the current knobs."""
    import ctypes as C
    from valle2_amd import _lib
    entry, ln, w16 = GEMM_ENTRIES[c.label]
    f = _lib.VhLinearFormInfo()
    if L.vh_linear_form(entry, c.M if M is None else M, c.N, c.K, c.T, ln, w16, C.byref(f)) != 0:
        return 'refused: ' + (L.vh_last_error() or b'').decode()
    family = {1: 'fast', 2: 'generic'}.get(f.family, str(f.family))
    return f'{family}<{f.mt},{f.nw},{f.epi},{f.pw},{f.ln},{f.nj},{f.w16}> b={f.block}'


ATTN_KERNEL = {1: 'attn_decode_kernel<{nw}>', 2: 'attn_decode_ring_kernel<{nw},{d}>', 3: 'attn_decode_ring16_kernel<{nw},{d}>',
               4: 'attn_decode_ring16_split_kernel<{nw},{d}>', 5: 'attn_decode_hd_kernel<{nw},{d},{lk},{nv}>', 6: 'attn_shared_kernel',
               7: 'attn_shared_groups_kernel', 8: 'attn_shared16_kernel'}
ATTN_SECOND = {1: 'attn_decode_combine_kernel', 2: 'attn_decode_hd_combine_kernel', 3: 'attn_records_merge_kernel',
               4: 'attn_records_merge_groups_kernel'}


def attn_info_form(entry, f):
    """The launch form of a vh_attn_decode_form_info, spelt as attn_launch_form spells the pinned file's."""
    name = ATTN_KERNEL[f.kernel].format(nw=f.nw, d=f.d, lk=f.lk, nv=f.nv) + f' b={f.block}'
    if f.second:
        name += f' + {ATTN_SECOND[f.second]} b={f.second_block}'
    return f'{entry}: {name}' + (' + in-launch combine' if f.fused_combine else '')


def attn_query(L, c, S_max, beams=None, prefix=None):
    """(launch form, info) of the launch a run of case c makes, under the current knobs."""
    import ctypes as C
    from valle2_amd import _lib
    f = _lib.VhAttnDecodeFormInfo()
    prefix = (c.prefix if prefix is None else prefix) if c.entry in SHARED else 0
    rc = L.vh_attn_decode_form(ATTN_ENTRIES[c.entry], c.B, c.h, c.head_dim, S_max, c.n_split, prefix, PREFIX_CAP + 32 if prefix else 0,
                               c.beams if beams is None else beams, 1 << 40, C.byref(f))
    if rc != 0:
        return 'refused: ' + (L.vh_last_error() or b'').decode(), None
    return attn_info_form(c.entry, f), f
