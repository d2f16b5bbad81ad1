"""The walk over every path of the training step's matrix products, shared by tests/test_train_gemm_paths_cpu.py (no GPU) and
tests/test_train_gemm_paths_gpu.py: vh_linear_ex (csrc/gemm.hip: tile_epilogue's three bodies + tile_tail_fixup_kernel, six
activations, pre_out / colsum / dropout, both operand stagings), vh_gemm_tn (the pinned schedule's endings and the host's
slices), vh_transpose / vh_transpose_many and vh_gemm_batched.  Here: mirrors of the host planners written from the C source,
the path signature of a shape, one case per signature, seeded inputs (an integer and a float flavour), float64 references,
bounds, and plain fp32 emulations in the kernels' summation order with planted faults that show the bounds bite.

Pure Python + torch at import; no library is loaded (the CPU file compares the mirrors with the library's *_ws_bytes).

Bounds (u = 2^-24, one fp32 rounding; L = contraction length; S = sum_k |a_k b_k|; T = S + |bias| + |residual|):
  derived cap    per element and output, beside `lin_reference` / `tn_cap` / `batched_cap` below
  asserted bound min(SUM_MARGIN x written figure, 1) x cap, per element.  A written figure is the worst error against float64,
                 IN UNITS OF THE CAP, of plain fp32 torch on the CPU and of the fp32 emulation in the kernel's order (32-wide
                 slabs, slices in slice order, the fix-up's slice sum) -- whichever is larger, through `written_figure` (+20 %,
                 two digits), never measured on a kernel.  Where SUM_MARGIN x figure exceeds 1 the bound is the cap itself.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from tests.attn_scores import written_figure          # noqa: F401  (the project's one rounding rule for written figures)
from tests.oracle_runners import SUM_MARGIN

U = 2.0 ** -24
ERF_ABS = 1.2e-7            # csrc/vh_common.h: vh_erf's absolute error
TM = TN = 128
TK = 32
ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_GELU_D, ACT_MUL = 0, 1, 2, 3, 4
KNOB_TILE_DMA, KNOB_TAIL_SPLIT, KNOB_TN_WGS = 4, 10, 11     # include/valle_hip.h VH_TUNE_*
MAX_FLOPS = 2176 * 2048 * 1024                              # the largest product of the walk


def cdiv(a, b):
    return -(-a // b)


def pad4(n):
    return (n + 3) // 4 * 4


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


# ======================================================================================================================
# mirrors of the host planners (csrc/gemm.hip, kernels.py)
# ======================================================================================================================
def n_tiles(M, N):
    return cdiv(M, TM) * cdiv(N, TN)


def tail_plan(M, N, K, tail_split_knob=0):
    """csrc/gemm.hip tail_plan: (K slices per tail tile, whole tiles in front of them); (0, tiles) = no tail split."""
    tiles = n_tiles(M, N)
    r = tiles % 256
    if tiles < 256 or r == 0 or r > 128 or N % TN or K % TK or tail_split_knob == 1:
        return 0, tiles
    split = min(8, 256 // r)
    while split >= 2 and (K % (split * TK) or K // split < 128):
        split -= 1
    return (0, tiles) if split < 2 else (split, tiles - r)


def linear_ex_ws_bytes(M, N, K):
    split, n_whole = tail_plan(M, N, K)
    return (n_tiles(M, N) - n_whole) * split * TM * TN * 4 if split else 0


def staging(M, K, tile_dma, train_epi=True):
    """gemm_plan: which kernel stages the operands.  'skinny': the decode kernels (M <= 64 without a training option)."""
    if M <= 64 and not train_epi:
        return 'skinny'
    return 'dma' if K % TK == 0 and tile_dma != 1 else 'reg'


def tn_plan(M, NI, NJ, wgs=0):
    """csrc/gemm.hip tn_plan + the slice rule of vh_gemm_tn: (planned splits, rows per slice, slices launched)."""
    tiles = n_tiles(NI, NJ)
    slabs = cdiv(M, TK)
    splits = (wgs if wgs > 0 else 256) // tiles
    splits = max(1, min(splits, slabs // 8, 64))
    chunk = cdiv(slabs, splits) * TK
    return splits, chunk, cdiv(M, chunk)


def tn_ws_bytes(M, NI, NJ, wgs=0):
    splits = tn_plan(M, NI, NJ, wgs)[0]
    return splits * NI * pad4(NJ) * 4 if splits > 1 else 0


def batched_splits(M, N, K, nb=1, nh=1):
    """kernels.gemm's split rule."""
    tiles = cdiv(M, 128) * cdiv(N, 128) * nb * nh
    return max(1, min(32, 512 // tiles, K // 512)) if tiles < 256 and K >= 2048 else 1


def batched_chunk(K, splits):
    """vh_gemm_batched's k_chunk (GK = 32: csrc/gemm_general.hip)."""
    return K if splits == 1 else cdiv(cdiv(K, splits), 32) * 32


# ---- path signatures ----------------------------------------------------------------------------------------------------
LinSig = namedtuple('LinSig', 'staging bodies split tail_ragged_m')
TnSig = namedtuple('TnSig', 'slices first last last_ragged ni_end nj_end')


def lin_signature(M, N, K, tile_dma=0, workspace=True, tail_split_knob=0):
    """Which code of csrc/gemm.hip a vh_linear_ex call with a training option runs."""
    st = staging(M, K, tile_dma)
    split, n_whole = tail_plan(M, N, K, tail_split_knob) if (st == 'dma' and workspace) else (0, n_tiles(M, N))
    tn_, bodies, ragged = cdiv(N, TN), set(), False
    for tile in range(n_tiles(M, N)):
        m0, n0 = tile // tn_ * TM, tile % tn_ * TN
        if tile >= n_whole:
            bodies.add('fix-up')
            ragged |= m0 + TM > M
        elif m0 + TM <= M and n0 + TN <= N:
            bodies.add('interior')
        else:
            if min(N, n0 + TN) - n0 >= 4:
                bodies.add('edge-whole')
            if N % 4 and n0 + TN > N:
                bodies.add('ragged-column')
    return LinSig(st, tuple(sorted(bodies)), split, ragged)


def tn_loop_class(rows):
    """The ending of gemm_tile_tn_kernel's schedule for a slice of `rows` contraction rows: (main loop taken, slabs left)."""
    nk, kt = cdiv(rows, TK), 0
    while kt + 3 < nk:
        kt += 2
    return ('loop' if kt else 'noloop') + f'+{nk - kt}'


def _end_class(n):
    return 'chunk' if n % 4 else ('tile' if n % TN else 'whole')     # ends inside a 4-column chunk / inside a tile / on a tile edge


def tn_signature(M, NI, NJ, wgs=0):
    splits, chunk, ny = tn_plan(M, NI, NJ, wgs)
    last = M - (ny - 1) * chunk
    slices = 'one' if ny == 1 else ('all' if ny == splits else 'fewer')
    return TnSig(slices, tn_loop_class(min(M, chunk)), tn_loop_class(last), last % TK != 0, _end_class(NI), _end_class(NJ))


# ======================================================================================================================
# the cases
# ======================================================================================================================
# geometries the walk must hold (M, N, K, what it reaches); K = 1056 is the head's backward: 1025 columns zero-padded to 1056
LIN_REQUIRED = [
    (129, 256, 64, 'interior and edge-whole tiles'), (5, 128, 32, 'a single small tile'), (130, 1025, 64, 'ragged column group'),
    (2176, 2048, 256, 'tail split 2'), (2176, 2048, 384, 'tail split 3'), (2176, 2048, 1024, 'tail split 8'),
    (2139, 2048, 256, 'every tail tile ragged in M'), (3072, 2048, 256, 'r = 128, the last split shape'),
    (9856, 640, 256, 'r = 129, no split'), (2176, 2048, 224, 'K / split < 128, no split'),
    (129, 128, 1056, 'K = 1025 zero-padded to 1056'),
]
LIN_DOMAIN = dict(M=(5, 64, 128, 129, 130, 2139, 2176, 3072, 6619, 9856), N=(2, 128, 130, 256, 640, 1025, 2048),
                  K=(32, 48, 64, 224, 256, 384, 1024))
LinGeom = namedtuple('LinGeom', 'M N K')


def lin_domain():
    d = LIN_DOMAIN
    return [LinGeom(M, N, K) for M in d['M'] for N in d['N'] for K in d['K'] if M * N * K <= MAX_FLOPS]


@functools.lru_cache(None)
def lin_walk():
    """{(signature at TILE_DMA 0, signature at TILE_DMA 1): LinGeom}: the required geometries, then for every other pair of
    signatures the mirrors produce over the domain the smallest shape by flops."""
    key = lambda g: (lin_signature(*g, tile_dma=0), lin_signature(*g, tile_dma=1))
    walk = {}
    for M, N, K, _ in LIN_REQUIRED:
        walk.setdefault(key(LinGeom(M, N, K)), []).append(LinGeom(M, N, K))
    for g in sorted(lin_domain(), key=lambda g: (g.M * g.N * g.K, g)):
        if key(g) not in walk:
            walk[key(g)] = [g]
    return walk


def lin_geoms():
    return [g for gs in lin_walk().values() for g in gs]


# name -> (act, bias, residual kind, pre_out, colsum, dropout); residual kinds: 'res' (added), 'pre' (saved pre-activation),
# 'mul' (saved derivative)
LIN_EPIS = {
    'bias':      (ACT_NONE, True, None, False, False, False),
    'res':       (ACT_NONE, True, 'res', False, False, False),
    'gelu_pre':  (ACT_GELU, True, None, True, False, False),
    'gelu_res':  (ACT_GELU, True, 'res', False, False, False),
    'gelu_d':    (ACT_GELU_D, True, None, True, False, False),
    'gelu_bwd':  (ACT_GELU_BWD, False, 'pre', False, False, False),
    'mul':       (ACT_MUL, False, 'mul', False, False, False),
    'res_cs':    (ACT_NONE, True, 'res', False, True, False),
    'gelu_d_cs': (ACT_GELU_D, True, None, True, True, False),
    'drop_res':  (ACT_NONE, True, 'res', False, False, True),
    'drop_gelu': (ACT_GELU, True, 'res', True, False, True),
    'drop_gelu_d': (ACT_GELU_D, True, None, True, False, True),
    'drop_res_cs': (ACT_NONE, True, 'res', False, True, True),
}
Epi = namedtuple('Epi', 'act bias res pre_out colsum drop')
LinCase = namedtuple('LinCase', 'geom epi tile_dma')


def epi_of(name):
    return Epi(*LIN_EPIS[name])


def epi_accepted(g, name, tile_dma):
    """The VH_REQUIREs of vh_linear_ex; below 65 rows an epilogue without a training option belongs to the decode kernels
    (gemm_plan) and to their walk (tests/decode_forms.py)."""
    e = epi_of(name)
    if e.colsum and g.N % 128:
        return False
    if e.drop and (g.N % 4 or g.K % TK or tile_dma == 1):
        return False
    train = e.pre_out or e.colsum or e.drop or e.act >= ACT_GELU_BWD
    return g.M > 64 or train


def lin_cases():
    return [LinCase(g, name, td) for g in lin_geoms() for td in (0, 1) for name in LIN_EPIS if epi_accepted(g, name, td)]


def lin_case_id(c):
    return f'{c.geom.M}x{c.geom.N}x{c.geom.K}-{c.epi}-dma{c.tile_dma}'


def lin_figure_key(c):
    return f'{c.geom.M}x{c.geom.N}x{c.geom.K}-{c.epi}'


# ---- gemm_tn ----------------------------------------------------------------------------------------------------------------
TN_SHAPES = ((128, 128), (130, 36), (36, 260), (260, 130))
TN_REQUIRED = ([(M, *TN_SHAPES[i % 4], 0) for i, M in enumerate((1, 31, 32, 33, 64, 65, 97, 160, 511, 512, 513))] +
               [(2049, 128, 128, 0), (4321, 128, 128, 0), (4321, 128, 128, 16),      # 16 workgroups: 15 slices of 288 rows + ONE row
                (16385, 256, 256, 0), (800, 260, 130, 12)])                          # 12 workgroups: 2 slices where the default has 3
TN_DOMAIN = dict(M=(1, 31, 32, 33, 64, 65, 96, 97, 128, 160, 257, 511, 512, 513, 544, 545, 577, 608, 800, 2049), wgs=(0, 12))
TnCase = namedtuple('TnCase', 'M NI NJ wgs')


@functools.lru_cache(None)
def tn_walk():
    walk = {}
    for c in TN_REQUIRED:
        walk.setdefault(tn_signature(*c), []).append(TnCase(*c))
    dom = [TnCase(M, NI, NJ, w) for M in TN_DOMAIN['M'] for NI, NJ in TN_SHAPES for w in TN_DOMAIN['wgs']]
    for c in sorted(dom, key=lambda c: (c.M * c.NI * c.NJ, c)):
        if tn_signature(*c) not in walk:
            walk[tn_signature(*c)] = [c]
    return walk


def tn_cases():
    return [c for cs in tn_walk().values() for c in cs]


def tn_case_id(c):
    return f'M{c.M}-{c.NI}x{c.NJ}' + (f'-wgs{c.wgs}' if c.wgs else '')


# ---- transposes --------------------------------------------------------------------------------------------------------------
# (rows, cols, ldo): rows and columns on, below and above multiples of 32, ldo above rows
TRANSPOSE_CASES = [(32, 32, 32), (31, 33, 32), (33, 31, 64), (64, 1, 64), (1, 64, 32), (70, 33, 96), (65, 95, 68), (1025, 36, 1056)]


def plan_shapes(n):
    """(rows, cols, ldo) of a TransposePlan's n items: mixed shapes, items of ONE tile among them (so that an item's first tile
    is the previous item's last + 1), ldo on and above rows."""
    kinds = [(32, 32, 32), (70, 33, 96), (5, 7, 8), (33, 64, 64), (31, 31, 32), (64, 40, 96), (1, 1, 4)]
    return [kinds[(i * 3 + i // 7) % len(kinds)] for i in range(n)]


PLAN_COUNTS = (1, 64, 65, 130)


# ---- gemm_batched --------------------------------------------------------------------------------------------------------------
# (M, N, K, batch, heads): 2-D and a (B, h) strided view, unsplit and the split kernels.gemm picks at K >= 2048, K % 4 != 0
BATCHED_SHAPES = [(70, 37, 131, 1, 1), (37, 64, 131, 2, 3), (70, 37, 2051, 1, 1), (37, 64, 2051, 2, 3)]
BatchedCase = namedtuple('BatchedCase', 'M N K nb nh ak bk')


def batched_cases():
    return [BatchedCase(*s, ak, bk) for s in BATCHED_SHAPES for ak in (False, True) for bk in (False, True)]


def batched_case_id(c):
    return f'{c.M}x{c.N}x{c.K}-b{c.nb}h{c.nh}-{"kT"[c.ak]}{"kT"[c.bk]}'


# ======================================================================================================================
# inputs
# ======================================================================================================================
DROP_SEED, DROP_SITE = 0x1234567890ABCDEF, (3 << 48) | (5 << 8) | 4
DROP_P = {'int': 0.5, 'float': 0.1}          # 1 / (1 - 0.5) = 2: the integer flavour stays exact through the dropout scale


def _ints(shape, gen):
    return torch.randint(-3, 4, shape, generator=gen).float()


@functools.lru_cache(maxsize=2)
def lin_inputs(g, flavour):
    """a (M, K), w (N, K), bias (N), res / saved (M, N).  Integer flavour: values in -3 .. 3, one weight column made asymmetric
    (a row or column permutation shows).  Float flavour: randn operands with a product of unit scale; the bias spreads the
    pre-activation over -6 .. 6 (both erf tails and the centre); the saved pre-activation / derivative handed to GELU_BWD / MUL
    is drawn on its own, independent of the product."""
    M, N, K = g
    gen = _gen(7, M, N, K, flavour == 'int')
    kt = 1025 if K == 1056 else K                                   # true contraction width; the rest is zero padding
    a, w = torch.zeros(M, K), torch.zeros(N, K)
    if flavour == 'int':
        a[:, :kt], w[:, :kt] = _ints((M, kt), gen), _ints((N, kt), gen)
        w[:, 0] += torch.arange(N).float() % 5
        a[:, 1] += torch.arange(M).float() % 3
        bias, res, saved = _ints((N,), gen), _ints((M, N), gen), _ints((M, N), gen)
    else:
        a[:, :kt], w[:, :kt] = torch.randn(M, kt, generator=gen), torch.randn(N, kt, generator=gen) / kt ** 0.5
        bias = torch.linspace(-6, 6, N)[torch.randperm(N, generator=gen)].contiguous()
        res = torch.randn(M, N, generator=gen)
        saved = 12 * torch.rand(M, N, generator=gen) - 6
    return dict(a=a, w=w, bias=bias, res=res, saved=saved)


def residual_of(inp, e):
    return None if e.res is None else inp['res' if e.res == 'res' else 'saved']


@functools.lru_cache(maxsize=4)
def keep_field(flavour, rows, cols):
    """The dropout field of the cases from the CPU oracle (oracle/philox.py), as float 0 / 1."""
    from oracle import philox as P
    return torch.from_numpy(P.keep_field(DROP_SEED, DROP_SITE, DROP_P[flavour], rows, cols).astype(np.float32))


def drop_scale(flavour):
    return float(np.float32(1.0 / (1.0 - np.float64(np.float32(DROP_P[flavour])))))


@functools.lru_cache(maxsize=4)
def tn_inputs(c, flavour):
    """a (M, lda), b (M, ldb) with lda / ldb beyond the 4-column pad and NaN out there; the pad itself holds finite values (the
    kernel multiplies them into rows / columns it never stores)."""
    gen = _gen(9, c.M, c.NI, c.NJ, flavour == 'int')
    lda, ldb = pad4(c.NI) + 8, pad4(c.NJ) + 4
    mk = (lambda *s: _ints(s, gen)) if flavour == 'int' else (lambda *s: torch.randn(*s, generator=gen))
    a, b = mk(c.M, lda), mk(c.M, ldb)
    if flavour == 'int':
        a[:, 0] += torch.arange(c.M).float() % 5
        b[:, c.NJ - 1] += torch.arange(c.M).float() % 3
    a[:, pad4(c.NI):], b[:, pad4(c.NJ):] = float('nan'), float('nan')
    return a, b


def batched_inputs(c, flavour):
    gen = _gen(13, c.M, c.N, c.K, c.nb, flavour == 'int')
    mk = (lambda *s: _ints(s, gen)) if flavour == 'int' else (lambda *s: torch.randn(*s, generator=gen))
    a, b = mk(c.nb, c.nh, c.M, c.K), mk(c.nb, c.nh, c.N, c.K)
    if flavour == 'int':
        b[..., 0] += torch.arange(c.N).float() % 5
    return a, b


# ======================================================================================================================
# vh_linear_ex: float64 reference, derived cap, fp32 emulation
# ======================================================================================================================
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * 0.5 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


@functools.lru_cache(maxsize=2)
def lin_products(g, flavour):
    """(a w^T in float64, sum_k |a_k w_k| in float64) from the fp32 inputs."""
    inp = lin_inputs(g, flavour)
    a, w = inp['a'].double(), inp['w'].double()
    return a @ w.T, a.abs() @ w.abs().T


# Roundings after the sum (the `c` of (L + c) u T), per value the epilogue forms:
#   pre-activation x = acc + bias                  1   -> |x^ - x| <= (L + 1) u (S + |bias|)             =: dx
#   out = x + residual                             2
#   gelu(x) = 0.5 x (1 + erf(x / sqrt 2))          |gelu'| <= 1.13: 1.13 dx; erf: 0.5 |x| (ERF_ABS + u) (its argument's rounding
#                                                  moves erf by < 0.49 u); three roundings of values <= |x|: 3 u |x|
#   gelu'(x) = Phi + x phi                         |gelu''| = |(2 - x^2) phi| <= 0.8: 0.8 dx; Phi: 0.5 ERF_ABS + u; x phi (<= 0.25):
#                                                  exp2 and its argument 4 u, two products 2 u, the sum 1.13 u: 0.5 ERF_ABS + 8 u
#   dropout                                        one rounding of s v: u s |v|; the error of v is scaled by s
#   + residual after activation / dropout          u (|v| + |residual|)
#   GELU_BWD: acc gelu'(p), p exact                1.13 L u S + |acc| (0.5 ERF_ABS + 8 u) + u |acc gelu'(p)|
#   MUL: acc r                                     |r| L u S + u |acc r|
#   colsum                                         sum_m cap(out) + (rows + 8) u sum_m |out|
GRAD_EVAL = 0.5 * ERF_ABS + 8 * U


def lin_reference(c, flavour):
    """{quantity: (float64 reference, derived cap)} of a case: 'out', and 'pre' / 'colsum' where the case has them."""
    g, e = c.geom, epi_of(c.epi)
    inp = lin_inputs(g, flavour)
    P, S = lin_products(g, flavour)
    L = 1025 if g.K == 1056 else g.K
    bias = inp['bias'].double() if e.bias else torch.zeros(g.N, dtype=torch.float64)
    r = residual_of(inp, e)
    r = None if r is None else r.double()
    x, dx = P + bias, (L + 1) * U * (S + bias.abs())
    keep = keep_field(flavour, g.M, g.N).double() * drop_scale(flavour) if e.drop else None
    out = {}
    if e.act == ACT_GELU_BWD:
        d = gelu_grad64(r)
        v, cap = P * d, 1.13 * L * U * S + P.abs() * GRAD_EVAL + U * (P * d).abs()
    elif e.act == ACT_MUL:
        v, cap = P * r, r.abs() * L * U * S + U * (P * r).abs()
    else:
        if e.act == ACT_GELU_D:
            d, dcap = gelu_grad64(x), 0.8 * dx + GRAD_EVAL
            if keep is not None:
                d, dcap = d * keep, keep * (dcap + U * d.abs())
            out['pre'] = (d, dcap)
        elif e.pre_out:
            out['pre'] = (x, dx)
        if e.act == ACT_NONE:
            v, cap = x, dx
        else:
            v, cap = gelu64(x), 1.13 * dx + 0.5 * x.abs() * (ERF_ABS + U) + 3 * U * x.abs()
        if keep is not None:
            cap = keep * (cap + U * v.abs())
            v = v * keep
        if r is not None:
            cap = cap + U * (v.abs() + r.abs())
            v = v + r
    out['out'] = (v, cap)
    if e.colsum:
        out['colsum'] = (v.sum(0), cap.sum(0) + (g.M + 8) * U * v.abs().sum(0))
    return out


def slab_product(a, w):
    """a w^T in fp32, added up slab by slab of 32 as the tile kernels' K loop does."""
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, a.shape[1], TK):
        acc += a[:, k0:k0 + TK] @ w[:, k0:k0 + TK].T
    return acc


def chain_product(a, w):
    """a w^T in fp32 as ONE chain of fused multiply-adds over k, the order of an MFMA accumulator (a product of two fp32 values
    is exact in float64, and the sum of it and an fp32 value rounds once to fp32 up to a double rounding of 2^-29 relative)."""
    acc = torch.zeros(a.shape[0], w.shape[0])
    a64, w64 = a.double(), w.double()
    for k in range(a.shape[1]):
        acc = (acc.double() + a64[:, k:k + 1] * w64[:, k][None, :]).float()
    return acc


CHAIN_ROWS = 96             # rows (spread over M, the last one among them) on which the chain order is emulated


def chain_rows(M):
    return torch.unique(torch.cat([torch.arange(0, M, max(1, M // (CHAIN_ROWS - 1)))[:CHAIN_ROWS - 1], torch.tensor([M - 1])]))


def gelu32(x):
    return 0.5 * x * (1 + torch.erf(x * np.float32(0.70710678118654752440)))


def gelu_grad32(x):
    cdf = 0.5 * (1 + torch.erf(x * np.float32(0.70710678118654752440)))
    return cdf + x * (np.float32(0.39894228040143267794) * torch.exp2(np.float32(-0.72134752044448170368) * x * x))


def tail_mask(g, n_whole):
    """(M, N) bool: the elements of the tail tiles (tile index >= n_whole, tiles numbered n-fastest)."""
    tn_ = cdiv(g.N, TN)
    tile = (torch.arange(g.M)[:, None] // TM) * tn_ + torch.arange(g.N)[None, :] // TN
    return tile >= n_whole


LIN_FAULTS = ('fixup_bias_per_slice', 'drop_after_residual', 'deriv_not_masked', 'pre_out_activated', 'bwd_uses_product',
              'colsum_rows_past_m', 'colsum_misses_fixup')


@functools.lru_cache(maxsize=6)
def _lin_acc(g, flavour, split, n_whole, plain, chain, bias_per_slice=None):
    """The accumulators a w^T of a geometry in fp32 (shared by the epilogues of the geometry): see lin_emulate."""
    inp = lin_inputs(g, flavour)
    a, w = inp['a'], inp['w']
    if plain:
        return a @ w.T
    product = chain_product if chain else slab_product
    if chain:
        a = a[chain_rows(g.M)]
    acc = product(a, w)
    if split:
        kl = g.K // split
        for s in range(split):
            part = product(a[:, s * kl:(s + 1) * kl], w[:, s * kl:(s + 1) * kl])
            tail = part if s == 0 else tail + part
            if bias_per_slice is not None and s:
                tail = tail + bias_per_slice
        mask = tail_mask(g, n_whole)
        acc = torch.where(mask[chain_rows(g.M)] if chain else mask, tail, acc)
    return acc


def lin_emulate(c, flavour, tail_split_knob=0, fault=None, plain=False, chain=False):
    """The case in fp32 on the CPU: plain=True is torch's own product, otherwise the kernels' order (32-wide slabs; with a tail
    split the tail tiles as `split` K slices added in slice order by the fix-up).  chain=True: every slab sum as one chain of
    FMAs over k, on the rows `chain_rows(M)` only (no column sums then).  `fault` plants one of LIN_FAULTS."""
    g, e = c.geom, epi_of(c.epi)
    inp = lin_inputs(g, flavour)
    rows_sel = chain_rows(g.M) if chain else None
    split, n_whole = tail_plan(g.M, g.N, g.K, tail_split_knob) if staging(g.M, g.K, c.tile_dma) == 'dma' else (0, 0)
    bias = inp['bias'] if e.bias else torch.zeros(g.N)
    if fault == 'fixup_bias_per_slice':
        acc = _lin_acc.__wrapped__(g, flavour, split, n_whole, plain, chain, bias)
    else:
        acc = _lin_acc(g, flavour, split, n_whole, plain, chain)
    r = residual_of(inp, e)
    keep = keep_field(flavour, g.M, g.N) * np.float32(drop_scale(flavour)) if e.drop else None
    if chain:
        r, keep = (None if r is None else r[rows_sel]), (None if keep is None else keep[rows_sel])
    out = {}
    if e.act == ACT_GELU_BWD:
        v = acc * gelu_grad32(acc if fault == 'bwd_uses_product' else r)
    elif e.act == ACT_MUL:
        v = acc * r
    else:
        x = acc + bias
        v = x if e.act == ACT_NONE else gelu32(x)
        if e.act == ACT_GELU_D:
            d = gelu_grad32(x)
            out['pre'] = d if keep is None or fault == 'deriv_not_masked' else d * keep
        elif e.pre_out:
            out['pre'] = v if fault == 'pre_out_activated' else x
        if keep is not None and fault != 'drop_after_residual':
            v = v * keep
        if r is not None:
            v = v + r
        if keep is not None and fault == 'drop_after_residual':
            v = v * keep
    out['out'] = v
    if e.colsum and not chain:
        rows = v
        if fault == 'colsum_misses_fixup':
            rows = torch.where(tail_mask(g, n_whole), torch.zeros(()), v)
        # per tile of 128 rows: 8 partial sums of 16 rows, added; then one atomic per tile (any order: here top to bottom)
        cs = torch.zeros(g.N)
        for m0 in range(0, g.M, TM):
            cs += rows[m0:m0 + TM].sum(0)
        if fault == 'colsum_rows_past_m':                 # the operand rows past M are re-reads of row M - 1
            cs += v[g.M - 1] * (cdiv(g.M, TM) * TM - g.M)
        out['colsum'] = cs
    return out


def worst_ratio(got, ref, cap):
    """max |got - ref| / cap; 0 / 0 counts as 0, a NaN as infinitely far."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros((), dtype=torch.float64, device=err.device), err / cap)
    ratio = torch.where(torch.isnan(ratio), torch.full((), float('inf'), dtype=torch.float64, device=err.device), ratio)
    return float(ratio.max())


def lin_measure(c, flavour='float'):
    """{quantity: worst error in units of the cap}: the larger of plain fp32 and the emulations with and without the tail split."""
    ref = lin_reference(c, flavour)
    runs = [lin_emulate(c, flavour, plain=True), lin_emulate(c, flavour, 0), lin_emulate(c, flavour, 1)]
    fig = {q: max(worst_ratio(r[q], *ref[q]) for r in runs) for q in ref}
    sel = chain_rows(c.geom.M)
    for knob in (0, 1):
        for q, t in lin_emulate(c, flavour, knob, chain=True).items():
            fig[q] = max(fig[q], worst_ratio(t, ref[q][0][sel], ref[q][1][sel]))
    return fig


def bound_factor(written):
    """The asserted bound in units of the cap: SUM_MARGIN x the written figure, the cap itself where that exceeds it."""
    return min(SUM_MARGIN * written, 1.0)


# ======================================================================================================================
# vh_gemm_tn
# ======================================================================================================================
def tn_reference(c, flavour):
    a, b = tn_inputs(c, flavour)
    a, b = a[:, :c.NI].double(), b[:, :c.NJ].double()
    return a.T @ b, a.abs().T @ b.abs()


def tn_cap(c, S):
    """(M + ny) u S: M products and adds inside the slices (fp32 FMA chains), ny - 1 adds of the reduce, one to spare."""
    return (c.M + tn_plan(*c)[2]) * U * S


TN_FAULTS = ('ragged_rows_not_zeroed', 'slice_left_out', 'chunk_clamped_early')


def tn_emulate(c, flavour, fault=None, plain=False, chain=False):
    a, b = tn_inputs(c, flavour)
    a, b = a[:, :pad4(c.NI)].clone(), b[:, :pad4(c.NJ)]
    if plain:
        return a[:, :c.NI].T @ b[:, :c.NJ]
    if fault == 'chunk_clamped_early':                    # the last 16-B chunk of every tile's rows of A comes from the chunk before
        for i0 in range(0, c.NI, TM):
            wd = min(TM, pad4(c.NI) - i0)
            if wd >= 8:
                a[:, i0 + wd - 4:i0 + wd] = a[:, i0 + wd - 8:i0 + wd - 4].clone()
    _, chunk, ny = tn_plan(*c)
    total = None
    for s in range(ny):
        lo, hi = s * chunk, min(c.M, (s + 1) * chunk)
        acc = torch.zeros(pad4(c.NI), pad4(c.NJ))
        if chain:
            acc = chain_product(a[lo:hi].T.contiguous(), b[lo:hi].T.contiguous())
        for k0 in range(lo, hi, TK) if not chain else ():
            acc += a[k0:min(hi, k0 + TK)].T @ b[k0:min(hi, k0 + TK)]
        if fault == 'ragged_rows_not_zeroed' and (hi - lo) % TK:      # the rows past the end re-read the slice's last row
            acc += (TK - (hi - lo) % TK) * torch.outer(a[hi - 1], b[hi - 1])
        if fault == 'slice_left_out' and ny > 1 and s == ny // 2:
            continue
        total = acc if total is None else total + acc
    return total[:c.NI, :c.NJ]


def tn_measure(c):
    ref, S = tn_reference(c, 'float')
    cap = tn_cap(c, S)
    return max(worst_ratio(tn_emulate(c, 'float', plain=True), ref, cap), worst_ratio(tn_emulate(c, 'float'), ref, cap),
               worst_ratio(tn_emulate(c, 'float', chain=True), ref, cap))


# ======================================================================================================================
# transposes
# ======================================================================================================================
SENTINEL = -77.0
TRANSPOSE_FAULTS = ('item_off_by_one', 'padding_unwritten')


def transpose_emulate(w, ldo, fault=None):
    """vh_transpose on the CPU: (cols, ldo) = w^T, zero in columns rows .. ldo; what a fault leaves unwritten keeps SENTINEL."""
    rows, cols = w.shape
    out = torch.full((cols, ldo), SENTINEL)
    out[:, :rows] = w.T
    if fault != 'padding_unwritten':
        out[:, rows:] = 0.0
    return out


def plan_emulate(weights, ldos, fault=None):
    """transpose_many_kernel tile by tile: the item of a tile is the last one whose tile0 <= tile ('item_off_by_one': < tile, so
    an item's first tile is taken for a tile past the end of the item before and writes nothing)."""
    tile0, t = [], 0
    for w, ldo in zip(weights, ldos):
        tile0.append(t)
        t += cdiv(w.shape[1], 32) * cdiv(ldo, 32)
    outs = [torch.full((w.shape[1], ldo), SENTINEL) for w, ldo in zip(weights, ldos)]
    for tile in range(t):
        hits = [i for i, t0 in enumerate(tile0) if (t0 < tile if fault == 'item_off_by_one' else t0 <= tile)]
        i = max(hits) if hits else 0
        w, ldo = weights[i], ldos[i]
        rows, cols = w.shape
        local, tiles_x = tile - tile0[i], cdiv(cols, 32)
        r0, c0 = local // tiles_x * 32, local % tiles_x * 32
        r1, c1 = min(r0 + 32, ldo), min(c0 + 32, cols)
        if r0 >= ldo:
            continue
        blk = torch.zeros(c1 - c0, r1 - r0)
        if r0 < rows:
            blk[:, :min(r1, rows) - r0] = w[r0:min(r1, rows), c0:c1].T
        outs[i][c0:c1, r0:r1] = blk
    return outs


def plan_weights(n, seed=0):
    gen = _gen(17, n, seed)
    shapes = plan_shapes(n)
    return [torch.randn(r, c, generator=gen) for r, c, _ in shapes], [ldo for _, _, ldo in shapes]


# ======================================================================================================================
# vh_gemm_batched
# ======================================================================================================================
def batched_reference(c, flavour):
    a, b = batched_inputs(c, flavour)
    a, b = a.double(), b.double()
    return a @ b.transpose(-1, -2), a.abs() @ b.abs().transpose(-1, -2)


def batched_cap(c, S):
    """(K + splits) u S: K products and adds inside the K chunks, one atomic add per chunk into the zeroed output."""
    return (c.K + batched_splits(c.M, c.N, c.K, c.nb, c.nh)) * U * S


def batched_emulate(c, flavour, plain=False, chain=False):
    a, b = batched_inputs(c, flavour)
    if plain:
        return a @ b.transpose(-1, -2)
    if chain:
        return torch.stack([chain_product(x, y) for x, y in zip(a.flatten(0, 1), b.flatten(0, 1))]).view(c.nb, c.nh, c.M, c.N)
    kc = batched_chunk(c.K, batched_splits(c.M, c.N, c.K, c.nb, c.nh))
    out = torch.zeros(c.nb, c.nh, c.M, c.N)
    for k0 in range(0, c.K, kc):
        part = torch.zeros_like(out)
        for k1 in range(k0, min(c.K, k0 + kc), TK):
            k2 = min(c.K, k0 + kc, k1 + TK)
            part += a[..., k1:k2] @ b[..., k1:k2].transpose(-1, -2)
        out += part
    return out


def batched_measure(c):
    ref, S = batched_reference(c, 'float')
    cap = batched_cap(c, S)
    return max(worst_ratio(batched_emulate(c, 'float', **order), ref, cap) for order in
               (dict(plain=True), dict(), dict(chain=True)))


# ======================================================================================================================
# the planted faults and the case each is shown on
# ======================================================================================================================
LIN_FAULT_CASES = {
    'fixup_bias_per_slice': LinCase(LinGeom(2176, 2048, 256), 'res', 0),
    'drop_after_residual': LinCase(LinGeom(129, 256, 64), 'drop_res', 0),
    'deriv_not_masked': LinCase(LinGeom(129, 256, 64), 'drop_gelu_d', 0),
    'pre_out_activated': LinCase(LinGeom(129, 256, 64), 'gelu_pre', 0),
    'bwd_uses_product': LinCase(LinGeom(129, 256, 64), 'gelu_bwd', 0),
    'colsum_rows_past_m': LinCase(LinGeom(129, 256, 64), 'res_cs', 0),
    'colsum_misses_fixup': LinCase(LinGeom(2176, 2048, 256), 'res_cs', 0),
}
TN_FAULT_CASES = {
    'ragged_rows_not_zeroed': TnCase(33, 128, 128, 0),
    'slice_left_out': TnCase(513, 128, 128, 0),
    'chunk_clamped_early': TnCase(65, 130, 36, 0),
}


def describe_signature(sig):
    if isinstance(sig, LinSig):
        return f'{sig.staging}: {"+".join(sig.bodies)}, split {sig.split}' + (', tail ragged in M' if sig.tail_ragged_m else '')
    return (f'slices {sig.slices}, first {sig.first}, last {sig.last}{" ragged" if sig.last_ragged else ""}, '
            f'NI ends {sig.ni_end}, NJ ends {sig.nj_end}')
