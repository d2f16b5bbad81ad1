"""Many-row attention, forward and backward, on adversarial scores, against float64.

tests/test_attn_geometry_gpu.py holds this kernel family to float64 on every mask geometry at one score scale (seeded randn:
no row maximum moves by more than a few units).  Here eight of its cases run on the nine score sets of tests/attn_scores.py —
a late peak, maxima that rise or fall with the key, rise below attn16's move threshold, or rise for the even queries of a wave
and fall for the odd ones, every score shifted by +-200 (|S| near 290 in base 2, where the backward's P = exp2(S - lse2)
cancels most), and a peak of +300 on the keys no query may see, which a refilled cache slot or a ragged batch leaves there.

Tolerances (tests/attn_scores.py): fp32 quantities get the larger of the geometry tests' tolerance and SUM_MARGIN = 4 times
the error fp32 arithmetic has on the CPU for the same (case, set, quantity) — ATTN_SCORE_FP32_ERR, the larger of the plain
fp32 reference's and the tile-wise emulation's worst error against float64, plus 20 %, two digits;
tests/test_attn_scores_cpu.py asserts it still holds, that right arithmetic passes and that each planted fault misses by more
than 10 x.  The 16-bit forward keeps test_bf16_gpu's tolerances.  The figures come from the reference's arithmetic, never
from a kernel."""
import pytest
import torch

from tests import attn_scores as A
from tests import oracle_runners as R
from tests import test_attn_geometry_gpu as G
from tests.test_attn_geometry_gpu import DEV, PAD_COLS, Forward, backward_forms, cache, device_spec, heads, rows

pytestmark = pytest.mark.gpu

# the fp32 arithmetic's worst error against float64 per case, set and quantity (A.measure_fp32 through A.written_figure)
ATTN_SCORE_FP32_ERR = {
    'prefix_small': {
        'plain': {'out': 8.8e-07, 'lse2': 1.5e-06, 'dv': 5.7e-06, 'dk': 5.5e-06, 'dq': 1.7e-06},
        'peak': {'out': 3.3e-06, 'lse2': 2.1e-05, 'dv': 2e-05, 'dk': 2.7e-05, 'dq': 4.1e-05},
        'rising': {'out': 8.2e-06, 'lse2': 9.2e-06, 'dv': 1.7e-05, 'dk': 1.1e-05, 'dq': 1.7e-05},
        'falling': {'out': 1.8e-06, 'lse2': 1.6e-06, 'dv': 5.7e-06, 'dk': 5.5e-06, 'dq': 2e-06},
        'rising_slow': {'out': 1.7e-06, 'lse2': 1.6e-06, 'dv': 5.7e-06, 'dk': 5.5e-06, 'dq': 1.7e-06},
        'plus200': {'out': 8.6e-05, 'lse2': 0.00016, 'dv': 8.4e-05, 'dk': 6.8e-05, 'dq': 0.0017},
        'minus200': {'out': 6.9e-05, 'lse2': 0.00021, 'dv': 7.5e-05, 'dk': 6.4e-05, 'dq': 0.0017},
        'hidden_peak': {'out': 8.8e-07, 'lse2': 1.5e-06, 'dv': 5.7e-06, 'dk': 5.5e-06, 'dq': 1.7e-06},
        'mixed_drift': {'out': 6.2e-06, 'lse2': 5.8e-06, 'dv': 8.2e-06, 'dk': 8e-06, 'dq': 1.7e-05},
    },
    'prefix_long': {
        'plain': {'out': 1.9e-06, 'lse2': 1.4e-06, 'dv': 1.9e-06, 'dk': 2e-06, 'dq': 1.2e-06},
        'peak': {'out': 6.3e-06, 'lse2': 2e-05, 'dv': 6e-05, 'dk': 7.2e-05, 'dq': 4.9e-05},
        'rising': {'out': 6e-05, 'lse2': 5.5e-05, 'dv': 0.00016, 'dk': 0.00011, 'dq': 0.00087},
        'falling': {'out': 2.1e-06, 'lse2': 1.7e-06, 'dv': 1.2e-05, 'dk': 1.3e-05, 'dq': 2.9e-06},
        'rising_slow': {'out': 8.9e-06, 'lse2': 1.1e-05, 'dv': 2.1e-05, 'dk': 1.7e-05, 'dq': 2.2e-05},
        'plus200': {'out': 4.4e-05, 'lse2': 4.4e-05, 'dv': 9.5e-05, 'dk': 8.6e-05, 'dq': 0.00063},
        'minus200': {'out': 4.2e-05, 'lse2': 5.4e-05, 'dv': 8.3e-05, 'dk': 7.6e-05, 'dq': 0.00072},
        'hidden_peak': {'out': 1.9e-06, 'lse2': 1.4e-06, 'dv': 1.9e-06, 'dk': 2e-06, 'dq': 1.2e-06},
        'mixed_drift': {'out': 6e-05, 'lse2': 5.5e-05, 'dv': 0.00012, 'dk': 5.9e-05, 'dq': 0.00075},
    },
    'full_small': {
        'plain': {'out': 1.1e-06, 'lse2': 1.5e-06, 'dv': 6.8e-06, 'dk': 5.2e-06, 'dq': 2.4e-06},
        'peak': {'out': 3.9e-06, 'lse2': 2e-05, 'dv': 2.4e-05, 'dk': 2.2e-05, 'dq': 3.3e-05},
        'rising': {'out': 8.4e-06, 'lse2': 1.1e-05, 'dv': 2.2e-05, 'dk': 1.6e-05, 'dq': 2.7e-05},
        'falling': {'out': 1.3e-06, 'lse2': 1.7e-06, 'dv': 6.8e-06, 'dk': 5.2e-06, 'dq': 2.4e-06},
        'rising_slow': {'out': 2.1e-06, 'lse2': 2.5e-06, 'dv': 6.8e-06, 'dk': 5.2e-06, 'dq': 2.4e-06},
        'plus200': {'out': 5.8e-05, 'lse2': 0.00016, 'dv': 9.7e-05, 'dk': 8.6e-05, 'dq': 0.00064},
        'minus200': {'out': 7.2e-05, 'lse2': 0.00011, 'dv': 8.1e-05, 'dk': 9.6e-05, 'dq': 0.00073},
        'hidden_peak': {'out': 1.1e-06, 'lse2': 1.5e-06, 'dv': 6.8e-06, 'dk': 5.2e-06, 'dq': 2.4e-06},
        'mixed_drift': {'out': 8.4e-06, 'lse2': 1.1e-05, 'dv': 1.8e-05, 'dk': 1.4e-05, 'dq': 2.2e-05},
    },
    'full_long': {
        'plain': {'out': 1.4e-06, 'lse2': 1.5e-06, 'dv': 6.7e-06, 'dk': 5e-06, 'dq': 2.1e-06},
        'peak': {'out': 4.1e-06, 'lse2': 1.8e-05, 'dv': 6.2e-05, 'dk': 5.9e-05, 'dq': 6.2e-05},
        'rising': {'out': 7.6e-05, 'lse2': 6.7e-05, 'dv': 0.00026, 'dk': 0.00021, 'dq': 0.0012},
        'falling': {'out': 2.1e-06, 'lse2': 1.9e-06, 'dv': 2.1e-05, 'dk': 1.6e-05, 'dq': 3.1e-06},
        'rising_slow': {'out': 1.2e-05, 'lse2': 1.4e-05, 'dv': 3.5e-05, 'dk': 3.8e-05, 'dq': 4.3e-05},
        'plus200': {'out': 7.7e-05, 'lse2': 6.4e-05, 'dv': 0.00022, 'dk': 0.00018, 'dq': 0.00084},
        'minus200': {'out': 6.7e-05, 'lse2': 8.6e-05, 'dv': 0.00021, 'dk': 0.00018, 'dq': 0.0011},
        'hidden_peak': {'out': 1.4e-06, 'lse2': 1.5e-06, 'dv': 6.7e-06, 'dk': 5e-06, 'dq': 2.1e-06},
        'mixed_drift': {'out': 7.6e-05, 'lse2': 6.7e-05, 'dv': 0.00024, 'dk': 0.00017, 'dq': 0.0008},
    },
    'explicit_shared': {
        'plain': {'out': 9.6e-07, 'lse2': 1.3e-06, 'dv': 1.4e-06, 'dk': 1.6e-06, 'dq': 1.4e-06},
        'peak': {'out': 4.7e-06, 'lse2': 1.8e-05, 'dv': 3.4e-05, 'dk': 3.1e-05, 'dq': 3.8e-05},
        'rising': {'out': 4.2e-05, 'lse2': 4.6e-05, 'dv': 0.00013, 'dk': 7e-05, 'dq': 0.0003},
        'falling': {'out': 1.6e-06, 'lse2': 1.9e-06, 'dv': 9.9e-06, 'dk': 8e-06, 'dq': 2.5e-06},
        'rising_slow': {'out': 6.4e-06, 'lse2': 7.2e-06, 'dv': 1.9e-05, 'dk': 1.4e-05, 'dq': 1.2e-05},
        'plus200': {'out': 4.8e-05, 'lse2': 5.1e-05, 'dv': 6e-05, 'dk': 7.3e-05, 'dq': 0.00053},
        'minus200': {'out': 4.8e-05, 'lse2': 4.2e-05, 'dv': 6.3e-05, 'dk': 6.9e-05, 'dq': 0.00045},
        'hidden_peak': {'out': 9.6e-07, 'lse2': 1.3e-06, 'dv': 1.4e-06, 'dk': 1.6e-06, 'dq': 1.4e-06},
        'mixed_drift': {'out': 4.1e-05, 'lse2': 4.6e-05, 'dv': 9.2e-05, 'dk': 6.3e-05, 'dq': 0.0003},
    },
    'empty_row_prefix': {
        'plain': {'out': 1.3e-06, 'lse2': 1.8e-06, 'dv': 3.3e-06, 'dk': 2e-06, 'dq': 1.1e-06},
        'peak': {'out': 4.3e-06, 'lse2': 1.7e-05, 'dv': 4.2e-05, 'dk': 3.3e-05, 'dq': 3.5e-05},
        'rising': {'out': 2.5e-05, 'lse2': 2.6e-05, 'dv': 5.8e-05, 'dk': 5.9e-05, 'dq': 0.00021},
        'falling': {'out': 2e-06, 'lse2': 2.4e-06, 'dv': 1.8e-05, 'dk': 9e-06, 'dq': 2.2e-06},
        'rising_slow': {'out': 5.5e-06, 'lse2': 6.1e-06, 'dv': 1.3e-05, 'dk': 7.6e-06, 'dq': 6.5e-06},
        'plus200': {'out': 4.3e-05, 'lse2': 6.9e-05, 'dv': 7.5e-05, 'dk': 6.6e-05, 'dq': 0.00093},
        'minus200': {'out': 5.6e-05, 'lse2': 5.1e-05, 'dv': 9.4e-05, 'dk': 0.00013, 'dq': 0.0013},
        'hidden_peak': {'out': 1.3e-06, 'lse2': 1.8e-06, 'dv': 3.3e-06, 'dk': 2e-06, 'dq': 1.1e-06},
        'mixed_drift': {'out': 2.3e-05, 'lse2': 2.5e-05, 'dv': 4.4e-05, 'dk': 3.8e-05, 'dq': 0.00018},
    },
    'prefix_tq_lt_tk': {
        'plain': {'out': 8.1e-07, 'lse2': 1.5e-06},
        'peak': {'out': 5.5e-06, 'lse2': 1.6e-05},
        'rising': {'out': 4.8e-05, 'lse2': 4.9e-05},
        'falling': {'out': 1.8e-06, 'lse2': 1.4e-06},
        'rising_slow': {'out': 6.2e-06, 'lse2': 7.4e-06},
        'plus200': {'out': 3.4e-05, 'lse2': 3.9e-05},
        'minus200': {'out': 2.3e-05, 'lse2': 3.9e-05},
        'hidden_peak': {'out': 8.1e-07, 'lse2': 1.5e-06},
        'mixed_drift': {'out': 4.8e-05, 'lse2': 4.9e-05},
    },
    'explicit_bmask': {
        'plain': {'out': 7.5e-07, 'lse2': 1.1e-06},
        'peak': {'out': 3.6e-06, 'lse2': 1.5e-05},
        'rising': {'out': 2.3e-05, 'lse2': 2.1e-05},
        'falling': {'out': 1.8e-06, 'lse2': 1.1e-06},
        'rising_slow': {'out': 3.4e-06, 'lse2': 4.8e-06},
        'plus200': {'out': 4.8e-05, 'lse2': 5.2e-05},
        'minus200': {'out': 4e-05, 'lse2': 5e-05},
        'hidden_peak': {'out': 7.5e-07, 'lse2': 1.1e-06},
        'mixed_drift': {'out': 1.3e-05, 'lse2': 2.1e-05},
    },
}
# (format, case, set) -> the fault-free attn16 emulation's written error where it leaves test_bf16_gpu's tolerances: nowhere
ATTN_SCORE_H16_ERR = {}
BWD_CASES = list(A.BWD_CASES)
ANALYTIC_CASES = list(A.ANALYTIC_CASES)
SENTINEL = -776.0                                       # (exact in fp32, fp16 and bf16)


def _pairs(cases):
    return [pytest.param(n, s, id=f'{n}-{s}') for n in cases for s in A.SCORE_SETS]


@pytest.mark.parametrize('name,score_set', _pairs(A.CASES))
def test_forward_fp32(name, score_set):
    """attn_rows_kernel (vh_attn_rows / vh_attn_rows_lse / vh_attn_rows_bmask): out and lse2 against float64, out bit-equal with
    and without lse2; K is NaN and V Inf beyond Tk, the keys in [kv_len, Tk) hold the set's values (hidden_peak: +300)."""
    f = Forward(name, A.operands(name, score_set))
    ref = A.reference(name, score_set)
    plain, _ = f.run(False)
    got = dict(out=heads(plain, f.B, f.h))
    if not f.per_row_mask:                         # (a per-row mask is inference only: vh_attn_rows_bmask writes no lse2)
        out, lse2 = f.run(True)
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), 'out differs between the runs with and without lse2'
        got['lse2'] = lse2.cpu()
    kept = R.attn_kept_rows(name)
    print(f'{name} {score_set}: ' + ', '.join(f'{qn} {R.worst(g_[kept], ref[qn][kept]):.3e}' for qn, g_ in got.items()))
    A.check_fp32(name, got, ref, ATTN_SCORE_FP32_ERR[name][score_set], G.ATTN_FP32_ERR[name]['lse2'])


@pytest.mark.parametrize('name,score_set', _pairs(BWD_CASES))
def test_backward(name, score_set):
    """attn_bwd_fused_kernel<4> / <8> + attn_dq_reduce_kernel at every chunk plan, attn_bwd_dq_kernel + attn_bwd_dkv_kernel:
    dq, dk, dv from the forward's own out / lse2; a second run is bit-identical; a row without a key gets exact zeros.
    On the shifted sets P = exp2(S - lse2) is the forward's P only if the recomputed S has the forward's bits: the row sum of dS
    that must vanish is multiplied by a key component of 400 in dq."""
    from valle2_amd import _lib
    L = _lib.lib()
    f = Forward(name, A.operands(name, score_set))
    ref = A.reference(name, score_set)
    out, lse2 = f.run(True)
    d, failed = f.d, []
    for label, form, forced in backward_forms(f):
        L.vh_set_tuning(G.KNOB_ATTN_BWD, form)
        L.vh_set_tuning(G.KNOB_ATTN_BWD_CHUNKS, forced)
        try:
            runs = []
            for _ in range(2):
                g_ = torch.full((f.B * f.Tk, 3 * d), float('nan'), device=DEV)
                f.K.attn_rows_bwd(f.q, f.kc, f.vc, out, f.dout, lse2, g_[:, :d], g_[:, d:2 * d], g_[:, 2 * d:], f.B, f.h, f.Tk,
                                  **f.spec)
                runs.append(g_)
        finally:
            L.vh_set_tuning(G.KNOB_ATTN_BWD, 0)
            L.vh_set_tuning(G.KNOB_ATTN_BWD_CHUNKS, 0)
        got = {qn: heads(runs[0][:, i * d:(i + 1) * d], f.B, f.h) for i, qn in enumerate(('dq', 'dk', 'dv'))}
        print(f'{name} {score_set} {label}: ' + ', '.join(f'{qn} {R.worst(got[qn], ref[qn]):.3e}' for qn in got))
        try:
            assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), 'a second run differs'
            A.check_fp32(name, got, ref, ATTN_SCORE_FP32_ERR[name][score_set], None)
        except AssertionError as e:
            failed.append(f'{label}: {e}')
    assert not failed, ' || '.join(failed)


@pytest.mark.parametrize('name,score_set', _pairs(ANALYTIC_CASES))
def test_forward_16bit(name, score_set):
    """attn16_kernel: operands narrowed to the build's 16-bit format, q pre-scaled as vh_linear_qkv_bf16 leaves it, against
    float64 attention over the same rounded operands."""
    from valle2_amd import kernels as K
    from valle2_amd._lib import h16_dtype
    H16 = h16_dtype()
    B, h, Tq, Tk, mode = R.ATTN_GEOMETRY_CASES[name]
    q, k, v, _ = A.operands(name, score_set)
    spec = R.attn_geometry_inputs(name)[5]
    assert K.Q16_PRESCALE == R.ATTN_Q16_PRESCALE
    d = 64 * h
    qbuf = torch.full((B * Tq, 3 * d), float('nan'), dtype=H16)
    qbuf[:, :d] = (rows(q) * K.Q16_PRESCALE).to(H16)
    obuf = torch.full((B * Tq, d + PAD_COLS), float('nan'), dtype=H16, device=DEV)
    K.attn_rows_bf16(qbuf.to(DEV)[:, :d], cache(k.to(H16), Tk + 9, float('nan'), H16), cache(v.to(H16), Tk + 9, float('inf'), H16),
                     obuf[:, :d], B, h, Tq, Tk, **device_spec(K, mode, spec))
    assert bool(torch.isnan(obuf[:, d:]).all()), 'columns beyond d were written'
    kept = R.attn_kept_rows(name)
    got, ref = heads(obuf[:, :d], B, h).double()[kept], A.reference(name, score_set, H16)['out'][kept]
    fallback = ATTN_SCORE_H16_ERR.get((str(H16), name, score_set))
    m = A.miss(got, ref, A.h16_tolerance(score_set, H16, ref, fallback))
    print(f'{name} {score_set}: out {R.worst(got, ref):.3e} ({m:.3g} x the tolerance)')
    assert m <= 1.0, f'out: {m:.3g} x the tolerance'


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('score_set', A.SCORE_SETS)
def test_packed_segments(score_set):
    """vh_attn_rows_packed and vh_attn_rows_packed_bf16 over segments of 1, 33, 129, 257 and 5 rows, each on a different score
    set (the parameter names the first segment's; the others follow in the order of SCORE_SETS): every segment bit-equal to the
    padded kernel on the segment alone — which the tests above hold to float64 —, finite, and the rows beyond the stream
    untouched.  K is NaN and V Inf from row M on; a neighbour's keys, shifted by up to +-200, are a segment's hidden keys."""
    from valle2_amd import kernels as K
    from valle2_amd._lib import h16_dtype
    from valle2_amd.engine import PackedRows
    H16, H = h16_dtype(), A.SEGMENT_HEADS
    first = A.SCORE_SETS.index(score_set)
    sets = [A.SCORE_SETS[(first + i) % len(A.SCORE_SETS)] for i in range(len(A.SEGMENT_LENGTHS))]
    segs = [A.segment(n, s, 500 + 7 * i) for i, (n, s) in enumerate(zip(A.SEGMENT_LENGTHS, sets))]
    prow = PackedRows(list(A.SEGMENT_LENGTHS), DEV)
    M, S_max = prow.rows, prow.rows + 64
    failed = []
    for label, dt, packed, alone_fn, scale in (('fp32', torch.float32, K.attn_rows_packed, K.attn_rows, 1.0),
                                               ('16-bit', H16, K.attn_rows_packed_bf16, K.attn_rows_bf16, K.Q16_PRESCALE)):
        q = torch.empty(M, H * 64, dtype=dt)
        kc = torch.full((1, H, S_max, 64), float('nan'), dtype=dt)
        vc = torch.full((1, H, S_max, 64), float('inf'), dtype=dt)
        for a, n, (qs, ks, vs, _) in zip(prow.starts, A.SEGMENT_LENGTHS, segs):
            q[a:a + n], kc[0, :, a:a + n], vc[0, :, a:a + n] = (qs * scale).to(dt), ks.to(dt), vs.to(dt)
        out = torch.full((M + 8, H * 64), SENTINEL, device=DEV, dtype=dt)
        q, kc, vc = q.to(DEV), kc.to(DEV), vc.to(DEV)
        packed(q, kc, vc, out[:M], H, prow)
        torch.cuda.synchronize()
        if not bool((out[M:] == SENTINEL).all()):
            failed.append(f'{label}: rows of out at or beyond M must keep the sentinel')
        for a, n, s, (qs, ks, vs, ref) in zip(prow.starts, A.SEGMENT_LENGTHS, sets, segs):
            got = out[a:a + n]
            alone = torch.full((n, H * 64), SENTINEL, device=DEV, dtype=dt)
            alone_fn(q[a:a + n].contiguous(), kc[:, :, a:a + n].contiguous(), vc[:, :, a:a + n].contiguous(), alone, 1, H, n, n,
                     K.MASK_FULL)
            if dt != torch.float32:                     # float64 over the rounded operands
                q64 = (qs * scale).to(dt).double().view(n, H, 64).permute(1, 0, 2) / scale
                p = torch.softmax(q64 @ ks.to(dt).double().transpose(-1, -2) / 8, dim=-1)
                ref = (p @ vs.to(dt).double()).permute(1, 0, 2).reshape(n, H * 64)
            same, finite = torch.equal(_bits(got), _bits(alone)), bool(torch.isfinite(got.float()).all())
            print(f'{label} segment of {n} rows at {a} on {s}: bit-equal to the padded kernel {same}, finite {finite}, '
                  f'out {R.worst(got, ref):.3e}')
            if not (same and finite):
                failed.append(f'{label} segment of {n} rows on {s}: bit-equal {same}, finite {finite}')
    assert not failed, ' || '.join(failed)
