"""Many-row attention on adversarial scores, shared by tests/test_attn_scores_cpu.py (no GPU) and tests/test_attn_scores_gpu.py:
the score sets, the operands that realise them on the geometry cases of tests/oracle_runners.py, two tile-wise fp32 emulations
of the kernels' documented schemes (with planted faults), and the tolerances.

Pure Python at import: no library is loaded.

Moving the scores (the construction of decode_forms.attn_inputs): e is a unit vector per head; q's component on e is replaced
by C_Q sign(i) and key j gets add_j / (C_Q / 8) e added, so query i sees its score (q . k / 8, natural-log units) for key j moved
by sign(i) add_j whatever the rest of q and k holds.  The masks, v and dout are the case's own.

Tolerances.  fp32: per element the larger of the geometry tests' tolerance (R.ATTN_TOL's atol + rtol |ref|; lse2: SUM_MARGIN x
ATTN_FP32_ERR) and SUM_MARGIN x the error the same quantity has when fp32 arithmetic computes it on the CPU — the larger of
the plain fp32 reference's and the fault-free tile-wise emulation's worst error against float64, written per (case, set,
quantity) into test_attn_scores_gpu.ATTN_SCORE_FP32_ERR (plus 20 %, two digits, asserted by the CPU file).  A score of 290 in
base 2 is known to 2^-16 in fp32, so the weights carry 1e-5 relative before anything is added up: the fixed tolerances do not
hold there for any fp32 arithmetic.  16-bit: test_bf16_gpu's, see h16_tolerance.  The figures come from the reference's
arithmetic, never from a kernel."""
import functools
import math

import torch

from tests import oracle_runners as R

C_Q = 4.0                               # q . e for every query (times its sign)
LOG2E = 1.4426950408889634
QSCALE = 0.125 * LOG2E                  # what the fp32 kernels multiply q by: scores in base 2
A16_LAZY, A16_NEG = 8.0, -1e30          # csrc/bf16.hip
SCORE_SETS = ('plain', 'peak', 'rising', 'falling', 'rising_slow', 'plus200', 'minus200', 'hidden_peak', 'mixed_drift')
# the smallest shapes that reach one chunk and several, <4> and <8>, the slab reduce, a row without a key, Tq < Tk and both
# explicit-mask entry points
CASES = ('prefix_small', 'prefix_long', 'full_small', 'full_long', 'explicit_shared', 'empty_row_prefix', 'prefix_tq_lt_tk',
         'explicit_bmask')
BWD_CASES = tuple(n for n in CASES if R.ATTN_GEOMETRY_CASES[n][2] == R.ATTN_GEOMETRY_CASES[n][3])
ANALYTIC_CASES = tuple(n for n in CASES if R.ATTN_GEOMETRY_CASES[n][4] != 'explicit')
EPS16 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -8}
SHARP_SETS = ('plain', 'peak')          # held to test_attn_rows_bf16's tolerance; the others to ..._drifting_maximum's


# ---- the operands ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def visible(name):
    """(B, Tq, Tk) bool of the case (R.attn_visible); nobody writes into it."""
    return R.attn_visible(name, R.attn_geometry_inputs(name)[5])


def row_amounts(seen, Tq, score_set):
    """(add (Tk,) float64 in natural-log units, sign (Tq,)) of one sequence whose queries, between them, see the keys `seen`."""
    Tk = seen.shape[0]
    j = torch.arange(Tk, dtype=torch.float64)
    add, sign = torch.zeros(Tk, dtype=torch.float64), torch.ones(Tq)
    if score_set == 'peak':                                      # the row's last visible key but one, and key 1
        keys = seen.nonzero().flatten()
        add[max(int(keys[-2] if len(keys) > 1 else keys[-1]) if len(keys) else Tk - 2, 0)] += 20.0
        add[min(1, Tk - 1)] += 12.0
    elif score_set in ('rising', 'mixed_drift'):
        add = j / 4
    elif score_set == 'falling':
        add = -j / 4
    elif score_set == 'rising_slow':                             # 5 per 64-key tile in base 2: below attn16's threshold of 8
        add = j * (5 * math.log(2.0) / 64)
    elif score_set in ('plus200', 'minus200'):
        add = torch.full((Tk,), 200.0 if score_set == 'plus200' else -200.0, dtype=torch.float64)
    elif score_set == 'hidden_peak':                             # every key no query of the sequence may see
        add = 300.0 * (~seen).double()
    else:
        assert score_set == 'plain', score_set
    if score_set == 'mixed_drift':
        sign[1::2] = -1.0
    return add, sign


def amounts(name, score_set):
    """(add (B, Tk), sign (Tq,)): query i's score for key j of batch row b moves by sign[i] add[b, j]."""
    B, h, Tq, Tk, _ = R.ATTN_GEOMETRY_CASES[name]
    seen = visible(name).any(1)                                  # (B, Tk): keys some query of the batch row sees
    per_row = [row_amounts(seen[b], Tq, score_set) for b in range(B)]
    return torch.stack([a for a, _ in per_row]), per_row[0][1]


def move_scores(q, k, add, sign, seed):
    """q (B, h, Tq, 64), k (B, h, Tk, 64) fp32 with the scores moved by sign[i] add[b, j]: on a seeded unit vector e per head q's
    component becomes C_Q sign(i) and key j gets add_j / (C_Q / 8) e added (in float64, rounded once)."""
    h = q.shape[1]
    gen = torch.Generator().manual_seed(seed)
    e = torch.nn.functional.normalize(torch.randn(h, 64, generator=gen, dtype=torch.float64), dim=-1)[None, :, None, :]
    q64 = q.double()
    q64 = q64 - (q64 * e).sum(-1, keepdim=True) * e + C_Q * sign.double()[None, None, :, None] * e
    k64 = k.double() + (add / (C_Q * 0.125))[:, None, :, None] * e
    return q64.float(), k64.float()


@functools.lru_cache(maxsize=None)
def operands(name, score_set):
    """(q, k, v, dout) fp32 of the case with the scores moved; shared, nobody writes into them."""
    q, k, v, dout, _, _ = R.attn_geometry_inputs(name)
    q, k = move_scores(q, k, *amounts(name, score_set), 9000 + list(R.ATTN_GEOMETRY_CASES).index(name))
    return q, k, v, dout


SEGMENT_LENGTHS = (1, 33, 129, 257, 5)      # of the packed test: one key, one past a 32-key tile, a query block and two, a short tail
SEGMENT_HEADS = 2


@functools.lru_cache(maxsize=None)
def segment(length, score_set, seed):
    """(q (len, 128), k, v (2, len, 64)) fp32 of one packed segment (full mask: every query sees the segment's keys and no
    other, so `hidden_peak` has no key of its own to move — the neighbours' keys are the hidden ones) and its float64
    attention (len, 128)."""
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(1, SEGMENT_HEADS, length, 64, generator=gen) for _ in range(3))
    add, sign = row_amounts(torch.ones(length, dtype=torch.bool), length, score_set)
    q, k = move_scores(q, k, add[None], sign, seed + 1)
    p = torch.softmax(q[0].double() @ k[0].double().transpose(-1, -2) / 8, dim=-1)
    flat = lambda t: t.permute(1, 0, 2).reshape(length, SEGMENT_HEADS * 64)
    return flat(q[0]).contiguous(), k[0].contiguous(), v[0].contiguous(), flat(p @ v[0].double())


@functools.lru_cache(maxsize=None)
def reference(name, score_set, h16=None):
    """float64, over the fp32 operands (h16: over the operands rounded to that format, q pre-scaled first)."""
    return R.attn_geometry_reference(name, h16=h16, operands=operands(name, score_set))


def quantities(name):
    return R.ATTN_QUANTITIES if name in BWD_CASES else ('out', 'lse2')


# ---- the kernels' schemes in fp32 torch, vectorised over rows ---------------------------------------------------------------------
FP32_FAULTS = ('no_rescale', 'max_before_mask', 'rescale_of_first_lane', 'bwd_exp_before_subtract', 'lse2_in_natural_units')
H16_FAULTS = ('no_rescale', 'max_before_mask', 'rescale_of_first_lane', 'ref_point_never_moves', 'delta_unclamped')


def _first_of_wave(t):
    """Along the query axis (the last): every query takes the value of the first query of its 32-query wave."""
    idx = torch.arange(t.shape[-1]) // 32 * 32
    return t[..., idx]


def _any_of_wave(t):
    """Along the query axis: whether any query of the 32-query wave holds True (a ballot)."""
    Tq = t.shape[-1]
    pad = (-Tq) % 32
    w = torch.nn.functional.pad(t, (0, pad)).reshape(*t.shape[:-1], -1, 32).any(-1, keepdim=True)
    return w.expand(*t.shape[:-1], (Tq + pad) // 32, 32).reshape(*t.shape[:-1], Tq + pad)[..., :Tq]


def emulate_fp32(name, ops, fault=None):
    """attn_rows_kernel's scheme and the backward's, fp32: scores in base 2 from q pre-multiplied by 0.125 log2 e, an online
    softmax over 32-key tiles (masked scores -inf, m_use = 0 while nothing is visible), lse2 = m + log2 l, out = acc / l; the
    backward from THIS forward's out and lse2, P = exp2(S - lse2), dS = P (dP - rowsum(dO o out)).  fault:
      'no_rescale'               accumulator and sum keep their scale when the maximum moves
      'max_before_mask'          a visited tile's maximum is taken over its hidden keys too (the weights are masked)
      'rescale_of_first_lane'    a 32-query wave follows its first query: every query takes that query's running maximum, and so
                                 its alpha.  (Consistently — weights and lse2 follow the same maximum; the inconsistent form,
                                 own weights under a foreign alpha, is wrong on any scores and the geometry tests see it.)
      'bwd_exp_before_subtract'  P = exp2(S) / exp2(lse2)
      'lse2_in_natural_units'    the backward takes lse2 for a natural logarithm and converts it: P = exp2(S - lse2 log2 e)"""
    B, h, Tq, Tk, _ = R.ATTN_GEOMETRY_CASES[name]
    q, k, v, dout = (t.float() for t in ops)
    vis = visible(name)[:, None]                                 # (B, 1, Tq, Tk)
    S = (q * QSCALE) @ k.transpose(-1, -2)
    ninf = float('-inf')
    m, l, acc = torch.full((B, h, Tq), ninf), torch.zeros(B, h, Tq), torch.zeros(B, h, Tq, 64)
    for k0 in range(0, Tk, 32):
        vt, st = vis[..., k0:k0 + 32], S[..., k0:k0 + 32]
        sm = st.masked_fill(~vt, ninf)
        tmax = sm.max(-1).values
        if fault == 'max_before_mask':
            tmax = torch.where(vt.any(-1), st.max(-1).values, tmax)
        m_new = torch.maximum(m, tmax)
        if fault == 'rescale_of_first_lane':
            m_new = _first_of_wave(m_new)
        m_use = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
        alpha = torch.ones_like(m) if fault == 'no_rescale' else torch.exp2(m - m_use)
        p = torch.exp2(sm - m_use[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + p @ v[:, :, k0:k0 + 32]
        m = m_new
    out, lse2 = acc / l[..., None], m + torch.log2(l)
    res = dict(out=out, lse2=lse2)
    if Tq != Tk:
        return res
    if fault == 'bwd_exp_before_subtract':
        P = torch.exp2(S) / torch.exp2(lse2)[..., None]
    else:
        P = torch.exp2(S - (lse2 * LOG2E if fault == 'lse2_in_natural_units' else lse2)[..., None])
    zero = torch.zeros(())
    P = torch.where(vis, P, zero)
    dS = torch.where(vis, P * (dout @ v.transpose(-1, -2) - (dout * out).sum(-1, keepdim=True)), zero)
    res.update(dq=dS @ k * 0.125, dk=dS.transpose(-1, -2) @ q * 0.125, dv=P.transpose(-1, -2) @ dout)
    return res


def round16(x, h16):
    """fp32 -> the 16-bit format as the attn16 kernels narrow a weight: fp16 towards zero (v_cvt_pkrtz), bf16 to nearest."""
    y = x.to(h16)
    if h16 == torch.float16:
        over = y.float().abs() > x.abs()                         # rounded away from zero: one step back
        bits = y.view(torch.int16)
        y = torch.where(over, bits - 1, bits).view(torch.float16)
    return y.float()


def emulate_attn16(name, ops, h16, fault=None):
    """attn16_kernel's scheme: operands in the 16-bit format (q pre-scaled by R.ATTN_Q16_PRESCALE, rounded once), fp32 scores in
    base 2, 64-key tiles; a reference point m_ref per query that moves to the row's maximum on tile 0 and afterwards only when
    some query of the 32-query wave has a tile maximum more than A16_LAZY above its own m_ref — then every query of the wave
    moves up to its tile maximum, never down; weights 2^(S - m_ref) rounded to 16 bits; row sums of the rounded weights.  fault:
      'no_rescale', 'max_before_mask'   as emulate_fp32's
      'rescale_of_first_lane'    the wave moves every query's reference point by its FIRST query's delta
      'ref_point_never_moves'    the reference point stays where tile 0 put it
      'delta_unclamped'          when the wave moves, a query whose tile maximum lies below its reference point moves it down"""
    B, h, Tq, Tk, _ = R.ATTN_GEOMETRY_CASES[name]
    q, k, v, _ = ops
    q16, k16, v16 = (q * R.ATTN_Q16_PRESCALE).to(h16).float(), k.to(h16).float(), v.to(h16).float()
    vis = visible(name)[:, None]
    S = q16 @ k16.transpose(-1, -2)
    m_ref, l, acc = torch.zeros(B, h, Tq), torch.zeros(B, h, Tq), torch.zeros(B, h, Tq, 64)
    for it, k0 in enumerate(range(0, Tk, 64)):
        vt = vis[..., k0:k0 + 64]
        x = S[..., k0:k0 + 64] - m_ref[..., None]
        xm = torch.where(vt, x, torch.tensor(A16_NEG))
        mx = xm.max(-1).values
        if fault == 'max_before_mask':
            mx = torch.where(vt.any(-1), x.max(-1).values, mx)
        seen = mx > 0.5 * A16_NEG
        if it == 0:
            move, delta = torch.ones_like(seen), torch.where(seen, mx, torch.zeros_like(mx))
        else:
            move = _any_of_wave(mx > A16_LAZY) & torch.tensor(fault != 'ref_point_never_moves')
            delta = torch.where(seen, mx, torch.zeros_like(mx)) if fault == 'delta_unclamped' else mx.clamp(min=0.0)
        if fault == 'rescale_of_first_lane':
            delta = _first_of_wave(delta)
        delta = torch.where(move, delta, torch.zeros_like(delta))
        m_ref = m_ref + delta
        if it and fault != 'no_rescale':
            alpha = torch.exp2(-delta)
            l, acc = l * alpha, acc * alpha[..., None]
        p = round16(torch.exp2(xm - delta[..., None]), h16)
        l = l + p.sum(-1)
        acc = acc + p @ v16[:, :, k0:k0 + 64]
    out = torch.where(l[..., None] > 0, acc / l[..., None], torch.zeros(()))
    return dict(out=out.to(h16).float())


# ---- tolerances and checks ------------------------------------------------------------------------------------------------------
def written_figure(err):
    """A measured error as it is written into a table: plus 20 %, rounded up to two digits."""
    if err == 0:
        return 0.0
    x = 1.2 * err
    e = math.floor(math.log10(x)) - 1
    return float(f'{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.1e}')


def measure_fp32(name, score_set):
    """{quantity: the larger worst error against float64 of the plain fp32 reference and of the fault-free tile-wise emulation}
    on the kept rows: what ATTN_SCORE_FP32_ERR holds (through written_figure)."""
    ops, ref, kept = operands(name, score_set), reference(name, score_set), R.attn_kept_rows(name)
    plain, tiled = R.attn_geometry_reference(name, torch.float32, operands=ops), emulate_fp32(name, ops)
    sel = lambda t, qn: t[kept] if qn in ('out', 'lse2') else t
    return {qn: max(R.worst(sel(plain[qn], qn), sel(ref[qn], qn)), R.worst(sel(tiled[qn], qn), sel(ref[qn], qn))) for qn in ref}


def fp32_tolerance(quantity, ref, written, lse2_geometry):
    """Per element: the larger of the geometry tests' tolerance and SUM_MARGIN x the written fp32 figure."""
    if quantity == 'lse2':
        old = torch.full_like(ref, R.SUM_MARGIN * lse2_geometry)
    else:
        old = R.ATTN_TOL[quantity][0] + R.ATTN_TOL[quantity][1] * ref.abs()
    return torch.clamp(old, min=R.SUM_MARGIN * written)


def h16_tolerance(score_set, h16, ref, fallback=None):
    """test_bf16_gpu.test_attn_rows_bf16's (plain, peak: atol 1e-3 fp16 / 6e-3 bf16) or test_attn_rows_bf16_drifting_maximum's
    (atol 2e-3 / 1e-2), rtol 2 EPS; fallback: the written error of the fault-free attn16 emulation where that one does not stay
    inside — then SUM_MARGIN x it."""
    fp16 = h16 == torch.float16
    atol = (1e-3 if fp16 else 6e-3) if score_set in SHARP_SETS else (2e-3 if fp16 else 1e-2)
    tol = atol + 2 * EPS16[h16] * ref.abs()
    return tol if fallback is None else torch.clamp(tol, min=R.SUM_MARGIN * fallback)


def miss(got, ref, tol):
    """The largest |got - ref| / tol; <= 1 passes, a NaN or an Inf is infinitely far."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, f'shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    ratio = (got - ref).abs() / tol
    return float(torch.nan_to_num(ratio, nan=float('inf')).max()) if ratio.numel() else 0.0


def fp32_misses(name, got, ref, written, lse2_geometry):
    """{quantity: miss} of the quantities `got` holds; out / lse2 on the kept rows only."""
    kept = R.attn_kept_rows(name)
    res = {}
    for qn in got:
        g_, r_ = (got[qn][kept], ref[qn][kept]) if qn in ('out', 'lse2') else (got[qn], ref[qn])
        res[qn] = miss(g_, r_, fp32_tolerance(qn, r_.double(), written[qn], lse2_geometry))
    return res


def check_fp32(name, got, ref, written, lse2_geometry):
    """Every quantity of `got` against float64; the gradients of a row without a key exactly zero.  Fails once, naming every
    quantity that failed (as R.check_attn does)."""
    failed = []
    for qn, m in fp32_misses(name, got, ref, written, lse2_geometry).items():
        if qn not in ('out', 'lse2'):
            for b in R.ATTN_EMPTY_ROWS.get(name, []):
                if float(got[qn][b].abs().max()) != 0.0:
                    failed.append(f'{qn}: row {b} has no key, its gradient must be exactly zero')
        if not m <= 1.0:
            failed.append(f'{qn}: {m:.3g} x the tolerance')
    assert not failed, 'failed: ' + ' | '.join(failed)
