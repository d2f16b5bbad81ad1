"""CPU companion of tests/test_attn_scores_gpu.py: the operands of tests/attn_scores.py move every score by what the set asks
for and leave every kept row a key; the reference is the geometry tests' own; the fp32 error of each (case, set, quantity) is
what the GPU file records; fault-free fp32 and 16-bit arithmetic of the kernels' schemes stays inside the tolerances; and each
planted fault misses float64 by more than 10 x the tolerance on the (case, set) named beside it.  No GPU."""
import pytest
import torch

from tests import attn_scores as A
from tests import oracle_runners as R
from tests import test_attn_geometry_gpu as G
from tests import test_attn_scores_gpu as S

PAIRS = [(n, s) for n in A.CASES for s in A.SCORE_SETS]
H16S = [torch.float16, torch.bfloat16]
ALL = frozenset(A.SCORE_SETS)


# ---- A. the inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,score_set', PAIRS)
def test_inputs_are_valid(name, score_set):
    B, h, Tq, Tk, _ = R.ATTN_GEOMETRY_CASES[name]
    q, k, v, dout = A.operands(name, score_set)
    q0, k0, v0, dout0 = A.operands(name, 'plain')
    assert all(t.dtype == torch.float32 for t in (q, k, v, dout)) and q.shape == (B, h, Tq, 64) and k.shape == (B, h, Tk, 64)
    assert torch.equal(v, v0) and torch.equal(dout, dout0) and torch.equal(v, R.attn_geometry_inputs(name)[2])
    add, sign = A.amounts(name, score_set)
    # every query's score for key j differs from its score for plain's key j by sign(i) add_j (the set's own queries on both
    # sides: where sign(i) = -1 the query itself differs from plain's, by its component on e)
    s, s0 = (q.double() @ kk.double().transpose(-1, -2) / 8 for kk in (k, k0))
    moved = sign.double()[None, None, :, None] * add[:, None, None, :]
    assert float((s - s0 - moved).abs().max()) < 1e-3
    if score_set != 'mixed_drift':
        assert torch.equal(q, q0) and bool((sign == 1).all())
    assert float((q[..., 0::2, :] - q0[..., 0::2, :]).abs().max()) == 0.0       # even queries are plain's in every set
    # every kept row still sees a key, the hidden ones are where the case put them
    has_key = A.visible(name).any(-1)
    for b in range(B):
        assert bool(has_key[b].all()) if b in R.attn_kept_rows(name) else not bool(has_key[b].any())
    ref = A.reference(name, score_set)
    assert set(ref) == set(A.quantities(name))
    kept = R.attn_kept_rows(name)
    assert all(bool(torch.isfinite(t[kept] if qn in ('out', 'lse2') else t).all()) for qn, t in ref.items())
    if score_set == 'hidden_peak':
        plain = A.reference(name, 'plain')
        assert float(add.max()) == 300.0 and not bool((add[:, None, :] * A.visible(name)).any())
        for qn in ref:
            sel = kept if qn in ('out', 'lse2') else slice(None)
            assert torch.equal(ref[qn][sel], plain[qn][sel]), f'{qn}: a hidden key changed the float64 reference'


def test_the_sets_do_what_they_are_for():
    """The late peak is hidden from earlier queries of its own diagonal tile; rising moves the maximum in every 32-key tile and
    falling never after tile 0; rising_slow stays below attn16's threshold per 64-key tile and rising above it; the uniform
    shifts put |S| near 290 in base 2; every case has a hidden key to put a peak on."""
    assert set(A.CASES) <= set(R.ATTN_GEOMETRY_CASES) and len(set(A.SCORE_SETS)) == 9
    name = 'prefix_long'
    add, _ = A.amounts(name, 'peak')
    vis = A.visible(name)
    for b in range(4):
        late = int((add[b] == 20.0).nonzero()[0])
        assert bool(vis[b, :, late].any()) and float(add[b, 1]) == 12.0
    b, late = 0, int((A.amounts(name, 'peak')[0][0] == 20.0).nonzero()[0])
    tile = slice(late // 32 * 32, late // 32 * 32 + 32)
    assert bool(vis[b, tile, late].any()) and not bool(vis[b, tile, late].all())         # queries of the diagonal tile disagree
    rise = A.amounts(name, 'rising')[0][0] * A.LOG2E
    slow = A.amounts(name, 'rising_slow')[0][0] * A.LOG2E
    assert float(rise[64] - rise[0]) > 2 * A.A16_LAZY and abs(float(slow[64] - slow[0]) - 5.0) < 1e-9 < A.A16_LAZY
    assert torch.equal(A.amounts(name, 'falling')[0], -A.amounts(name, 'rising')[0])
    assert abs(200 * A.LOG2E - 288.5) < 0.1
    sign = A.amounts(name, 'mixed_drift')[1]
    assert sign[:32].tolist() == [1.0, -1.0] * 16
    for n in A.CASES:
        assert float(A.amounts(n, 'hidden_peak')[0].max()) == 300.0, n
    assert set(S.BWD_CASES) == set(A.BWD_CASES) == set(A.CASES) - {'prefix_tq_lt_tk', 'explicit_bmask'}
    assert set(S.ANALYTIC_CASES) == set(A.ANALYTIC_CASES) and S.pytestmark.name == 'gpu'


# ---- B. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', A.CASES)
def test_reference_is_unchanged(name):
    """The optional operands argument changes nothing for those who do not pass it, and passing a case's own operands gives
    the same bits: there is one reference."""
    q, k, v, dout, _, _ = R.attn_geometry_inputs(name)
    for kw in ({}, dict(dtype=torch.float32), dict(h16=torch.float16)):
        own, again = R.attn_geometry_reference(name, **kw), R.attn_geometry_reference(name, operands=(q, k, v, dout), **kw)
        assert set(own) == set(again)
        for qn in own:
            assert torch.equal(own[qn].view(torch.int64 if own[qn].dtype == torch.float64 else torch.int32),
                               again[qn].view(torch.int64 if own[qn].dtype == torch.float64 else torch.int32)), (qn, kw)
    # ... and on the `plain` operands it is torch autograd's, as test_attn_geometry_cpu shows for the case's own
    ops, ref, kept = A.operands(name, 'plain'), A.reference(name, 'plain'), R.attn_kept_rows(name)
    leaf = [t[kept].double().requires_grad_() for t in ops[:3]]
    out = torch.nn.functional.scaled_dot_product_attention(*leaf, attn_mask=A.visible(name)[kept][:, None])
    torch.testing.assert_close(ref['out'][kept], out.detach(), rtol=1e-11, atol=1e-12)
    if name in A.BWD_CASES:
        out.backward(ops[3][kept].double())
        for qn, t in zip(('dq', 'dk', 'dv'), leaf):
            torch.testing.assert_close(ref[qn][kept], t.grad, rtol=1e-10, atol=1e-12)


# ---- C. the measured bounds; right arithmetic passes ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,score_set', PAIRS)
def test_fp32_error_is_what_the_gpu_file_says(name, score_set):
    measured, written = A.measure_fp32(name, score_set), S.ATTN_SCORE_FP32_ERR[name][score_set]
    assert set(written) == set(measured) == set(A.quantities(name))
    for qn, err in measured.items():
        print(f'{name} {score_set} {qn}: {err:.3e}')
        assert 0.25 * written[qn] <= err <= written[qn], f'{qn}: measured {err:.3e}, the GPU file says {written[qn]:.3e}'
    ops, ref = A.operands(name, score_set), A.reference(name, score_set)
    for emu in (R.attn_geometry_reference(name, torch.float32, operands=ops), A.emulate_fp32(name, ops)):
        A.check_fp32(name, emu, ref, written, G.ATTN_FP32_ERR[name]['lse2'])


def test_plain_is_tied_to_the_geometry_tolerances():
    """On `plain` the written figure times SUM_MARGIN stays below the fixed tolerance of every quantity: the new inputs are held
    to what the geometry tests hold theirs to.  On the uniform shifts it cannot: a base-2 score of 290 has an fp32 spacing of
    3e-5, and the weights inherit it."""
    for name in A.CASES:
        w = S.ATTN_SCORE_FP32_ERR[name]['plain']
        assert all(R.SUM_MARGIN * w[qn] <= R.ATTN_TOL[qn][0] for qn in w if qn != 'lse2'), name
        assert R.SUM_MARGIN * S.ATTN_SCORE_FP32_ERR[name]['plus200']['out'] > R.ATTN_TOL['out'][0]
    assert set(S.ATTN_SCORE_FP32_ERR) == set(A.CASES) and all(set(v) == ALL for v in S.ATTN_SCORE_FP32_ERR.values())


@pytest.mark.parametrize('h16', H16S, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('name', A.ANALYTIC_CASES)
def test_attn16_scheme_stays_inside_the_16bit_tolerances(name, h16):
    """The fault-free emulation of attn16_kernel's scheme against float64 over the same rounded operands, within
    test_bf16_gpu's tolerances on every set: no (case, set) needs the fall-back, and ATTN_SCORE_H16_ERR is empty."""
    kept = R.attn_kept_rows(name)
    assert S.ATTN_SCORE_H16_ERR == {}
    for score_set in A.SCORE_SETS:
        ref = A.reference(name, score_set, h16)['out'][kept]
        got = A.emulate_attn16(name, A.operands(name, score_set), h16)['out'][kept]
        m = A.miss(got, ref, A.h16_tolerance(score_set, h16, ref))
        print(f'{name} {score_set}: worst error {R.worst(got, ref):.3e}, {m:.3g} x the tolerance')
        assert m <= 1.0, (score_set, m)


# ---- D. planted faults ------------------------------------------------------------------------------------------------------------
# fault -> (case, set, quantities that miss by more than 10 x), and the sets that reject it by more than 10 x on prefix_long
FP32_FAULTS = {
    'no_rescale': ('prefix_long', 'rising', R.ATTN_QUANTITIES, ALL - {'falling'}),
    'max_before_mask': ('prefix_long', 'hidden_peak', R.ATTN_QUANTITIES, {'hidden_peak'}),
    'rescale_of_first_lane': ('prefix_long', 'mixed_drift', R.ATTN_QUANTITIES, {'mixed_drift'}),
    'bwd_exp_before_subtract': ('prefix_long', 'plus200', ('dq', 'dk', 'dv'), {'rising', 'plus200', 'minus200', 'mixed_drift'}),
    'lse2_in_natural_units': ('prefix_long', 'minus200', ('dq', 'dk', 'dv'), ALL),
}
H16_FAULTS = {      # fault -> (case, set, sets that reject it on prefix_long in fp16, in bf16)
    'no_rescale': ('prefix_long', 'rising', {'peak', 'rising', 'rising_slow', 'mixed_drift'}, {'peak', 'rising', 'rising_slow', 'mixed_drift'}),
    'max_before_mask': ('prefix_long', 'hidden_peak', {'rising', 'hidden_peak', 'mixed_drift'}, {'hidden_peak'}),
    'rescale_of_first_lane': ('prefix_long', 'mixed_drift', {'mixed_drift'}, {'mixed_drift'}),
    'ref_point_never_moves': ('prefix_long', 'rising', {'rising', 'rising_slow', 'mixed_drift'}, {'rising', 'mixed_drift'}),
    'delta_unclamped': ('prefix_long', 'mixed_drift', {'mixed_drift'}, {'mixed_drift'}),
}


def _fp32_misses(name, score_set, fault):
    bad = A.emulate_fp32(name, A.operands(name, score_set), fault)
    return A.fp32_misses(name, bad, A.reference(name, score_set), S.ATTN_SCORE_FP32_ERR[name][score_set], G.ATTN_FP32_ERR[name]['lse2'])


def _h16_miss(name, score_set, h16, fault):
    kept = R.attn_kept_rows(name)
    ref = A.reference(name, score_set, h16)['out'][kept]
    return A.miss(A.emulate_attn16(name, A.operands(name, score_set), h16, fault)['out'][kept], ref, A.h16_tolerance(score_set, h16, ref))


@pytest.mark.parametrize('fault', A.FP32_FAULTS)
def test_fp32_fault_is_rejected_with_margin(fault):
    name, score_set, expect, catching = FP32_FAULTS[fault]
    miss = _fp32_misses(name, score_set, fault)
    print(fault, name, score_set, {qn: f'{m:.3g}' for qn, m in miss.items()})
    assert {qn for qn, m in miss.items() if m > 10} == set(expect), miss
    assert all(m <= 1 for qn, m in miss.items() if qn not in expect), miss
    with pytest.raises(AssertionError, match='failed: '):
        A.check_fp32(name, A.emulate_fp32(name, A.operands(name, score_set), fault), A.reference(name, score_set),
                     S.ATTN_SCORE_FP32_ERR[name][score_set], G.ATTN_FP32_ERR[name]['lse2'])
    by_set = {s: max(_fp32_misses(name, s, fault).values()) for s in A.SCORE_SETS}
    assert {s for s, m in by_set.items() if m > 10} == set(catching), by_set


@pytest.mark.parametrize('h16', H16S, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('fault', A.H16_FAULTS)
def test_16bit_fault_is_rejected_with_margin(fault, h16):
    name, score_set, in_fp16, in_bf16 = H16_FAULTS[fault]
    by_set = {s: _h16_miss(name, s, h16, fault) for s in A.SCORE_SETS}
    print(fault, name, {s: f'{m:.3g}' for s, m in by_set.items()})
    assert by_set[score_set] > 10
    assert {s for s, m in by_set.items() if m > 10} == (in_fp16 if h16 == torch.float16 else in_bf16), by_set


def test_faults_that_need_their_set():
    """A fault passes on `plain`, which is why the sets exist — with two exceptions among the fp32 faults, which the geometry
    tests see already and which are kept because they are what the backward's cancellation against lse2 invites:
      'no_rescale'             ordinary scores move a row's maximum too (it passes only on `falling`, whose maximum never moves
                               after tile 0); the 16-bit form of it does pass on plain, where the lazy reference point stays put
      'lse2_in_natural_units'  lse2 of an ordinary row is log2 of a few hundred, not 0: a unit error shows on any scores.
    rescale_of_first_lane is planted in its consistent form for the same reason (see emulate_fp32)."""
    for name in ('prefix_long', 'full_long'):
        for fault in A.FP32_FAULTS:
            worst = max(_fp32_misses(name, 'plain', fault).values())
            assert (worst > 10) if fault in ('no_rescale', 'lse2_in_natural_units') else (worst <= 1), (name, fault, worst)
        assert max(_fp32_misses(name, 'falling', 'no_rescale').values()) <= 1
        for h16 in H16S:
            for fault in A.H16_FAULTS:
                assert _h16_miss(name, 'plain', h16, fault) <= 1, (name, fault, h16)
    # the faults that turn on lanes of a wave disagreeing pass where they agree
    assert max(_fp32_misses('prefix_long', 'rising', 'rescale_of_first_lane').values()) <= 1
    assert _h16_miss('full_long', 'falling', torch.float16, 'delta_unclamped') <= 1
    assert _h16_miss('full_long', 'rising', torch.float16, 'delta_unclamped') <= 1
    # the threshold: below it the reference point lags and the weights grow, which fp16 cannot hold and bf16 can
    assert _h16_miss('full_long', 'rising_slow', torch.float16, 'ref_point_never_moves') > 10
    assert _h16_miss('full_long', 'rising_slow', torch.bfloat16, 'ref_point_never_moves') <= 1
