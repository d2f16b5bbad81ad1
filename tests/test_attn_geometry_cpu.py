"""CPU companion of tests/test_attn_geometry_gpu.py: the float64 reference of the attention geometry cases is torch autograd's
through F.scaled_dot_product_attention; the case table reaches every edge the kernels' tile shortcuts turn on (asserted from
the table, so an edit cannot drop one silently); the fp32 emulation's error is what the GPU file records; and each planted
geometry fault misses the reference by more than 10 x the tolerance of the GPU file on the case named beside it.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import oracle_runners as R
from tests import test_attn_geometry_gpu as G

CASES = R.ATTN_GEOMETRY_CASES
BLOCKS = (32, 64, 128, 256)         # key tile / query wave, attn16's key tile, query block, largest key chunk


def _lengths(key, modes):
    """(case, batch row, value, T) of every per-row length `key` over the cases of `modes`, rows without a key left out."""
    return [(n, b, int(x), CASES[n][3]) for n in CASES if CASES[n][4] in modes and key in R.ATTN_GEOMETRY_LENGTHS[n]
            for b, x in enumerate(R.ATTN_GEOMETRY_LENGTHS[n][key]) if b not in R.ATTN_EMPTY_ROWS.get(n, [])]


# ---- A. the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_reference_is_torch_autograd_in_float64(name):
    B, h, Tq, Tk, mode = CASES[name]
    q, k, v, dout, _, spec = R.attn_geometry_inputs(name)
    kept = R.attn_kept_rows(name)
    vis = R.attn_visible(name, spec)
    assert vis.shape == (B, Tq, Tk) and vis.dtype == torch.bool
    ref = R.attn_geometry_reference(name)
    leaf = [t[kept].double().requires_grad_() for t in (q, k, v)]
    out = F.scaled_dot_product_attention(*leaf, attn_mask=vis[kept][:, None])
    torch.testing.assert_close(ref['out'][kept], out.detach(), rtol=1e-11, atol=1e-12)
    s = (leaf[0].detach() @ leaf[1].detach().transpose(-1, -2)) / 8
    lse2 = torch.log2((torch.exp(s) * vis[kept][:, None]).sum(-1))
    torch.testing.assert_close(ref['lse2'][kept], lse2, rtol=1e-11, atol=1e-11)
    assert set(ref) == set(R.ATTN_QUANTITIES if Tq == Tk else ('out', 'lse2'))
    if Tq == Tk:
        out.backward(dout[kept].double())
        for qn, t in zip(('dq', 'dk', 'dv'), leaf):
            torch.testing.assert_close(ref[qn][kept], t.grad, rtol=1e-10, atol=1e-12, msg=lambda m, qn=qn: f'{qn}: {m}')
            for b in R.ATTN_EMPTY_ROWS.get(name, []):
                assert float(ref[qn][b].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t[kept]).all()) for t in ref.values())


# ---- B. the cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_case_is_valid(name):
    B, h, Tq, Tk, mode = CASES[name]
    q, k, v, dout, mode2, spec = R.attn_geometry_inputs(name)
    assert B <= 4 and h <= 2 and Tq <= Tk <= 640 and mode == mode2
    assert q.shape == dout.shape == (B, h, Tq, 64) and k.shape == v.shape == (B, h, Tk, 64)
    assert all(t.dtype == torch.float32 for t in (q, k, v, dout))
    assert 0.9 < float((q @ k.transpose(-1, -2) / 8).std()) < 1.1                  # scores at the ordinary scale
    for key, dt in (('x_len_dev', torch.int32), ('kv_len', torch.int32), ('mask', torch.uint8), ('pad', torch.uint8)):
        assert key not in spec or (spec[key].dtype == dt and spec[key].shape[0] in (B, Tq))
    has_key = R.attn_visible(name, spec).any(-1)                                   # (B, Tq)
    empty = R.ATTN_EMPTY_ROWS.get(name, [])
    for b in range(B):
        assert bool(has_key[b].all()) if b not in empty else not bool(has_key[b].any()), (name, b)
    assert set(R.ATTN_GEOMETRY_LENGTHS) == set(CASES) == set(G.ATTN_FP32_ERR)


def test_the_table_reaches_every_edge():
    xs, kvs = _lengths('x_len_dev', ('prefix',)), _lengths('kv_len', ('prefix', 'full'))
    for what, vals in (('x_len_dev', xs), ('kv_len', kvs)):
        for m in BLOCKS:
            for r in (0, 1, m - 1):
                # the remainder at THIS block size: not only through a multiple of the next size up
                hit = [x for _, _, x, T in vals if 0 < x <= T and x % m == r and (m == 256 or x % (2 * m) != r)]
                assert hit, f'no {what} with remainder {r if r < 2 else -1} modulo {m}'
    assert {0, 1} <= {x for _, _, x, _ in xs} and any(x == T for _, _, x, T in xs) and any(x > T for _, _, x, T in xs)
    assert any(x == 1 for _, _, x, _ in kvs) and any(x > T for _, _, x, T in kvs)
    for modes in (('prefix',), ('full',)):                       # FULL mode has the same kv_len edges
        own = [x for _, _, x, T in _lengths('kv_len', modes)]
        assert 1 in own and all(any(x % m == r for x in own) for m in (32, 64, 128) for r in (0, 1, m - 1)), modes
        assert any(x > T for _, _, x, T in _lengths('kv_len', modes))
    # kv_len below, at and just above x_len
    pairs = [(x, kv) for (n, b, x, _), (n2, b2, kv, _) in zip(xs, _lengths('kv_len', ('prefix',))) if CASES[n][2] == CASES[n][3]]
    assert [(n, b) for n, b, _, _ in xs] == [(n, b) for n, b, _, _ in _lengths('kv_len', ('prefix',)) if 'x_len_dev' in R.ATTN_GEOMETRY_LENGTHS[n]]
    assert any(kv < x for x, kv in pairs) and any(kv == x for x, kv in pairs) and any(kv == x + 1 for x, kv in pairs)
    # T: partly filled last query block / key tile / chunk, a multiple of 256, the three bands — for each analytic mode
    for mode in ('prefix', 'full'):
        Ts = {c[3] for c in CASES.values() if c[4] == mode and c[2] == c[3]}
        assert any(T % 128 and T % 32 and T % R.attn_chunk_keys(T) for T in Ts if T > 256), mode
        assert any(T % 256 == 0 for T in Ts) and any(T <= 128 for T in Ts) and any(128 < T <= 256 for T in Ts) and any(T > 512 for T in Ts), mode
    # the two fused kernels under FULL: a single chunk of at most 128 keys (<4>) and one above (<8>)
    full_T = {c[3] for c in CASES.values() if c[4] == 'full' and c[2] == c[3]}
    assert any(R.attn_chunk_keys(T) <= 128 for T in full_T) and any(R.attn_chunk_keys(T) > 128 for T in full_T)
    # a prefix end inside a chunk, on a chunk edge, on a 32-key wave edge (chunks as cut at the fewest: the GPU file forces that)
    long = [(x, R.attn_chunk_keys(T)) for n, _, x, T in xs if T > 256 and CASES[n][2] == T and 0 < x < T]
    assert any(x % ck == 0 for x, ck in long) and any(x % 32 and x % ck for x, ck in long) and any(x % 32 == 0 and x % ck for x, ck in long)
    assert CASES['prefix_scalar'][4] == 'prefix' and R.ATTN_GEOMETRY_LENGTHS['prefix_scalar']['x_len'] % 32 == 0
    # explicit: a shared mask with pad (forward and backward) and a per-row one with pad (forward only)
    for n, dims, square in (('explicit_shared', 2, True), ('explicit_bmask', 3, False)):
        spec = R.attn_geometry_inputs(n)[5]
        assert CASES[n][4] == 'explicit' and spec['mask'].dim() == dims and bool(spec['pad'].any()) and (CASES[n][2] == CASES[n][3]) == square
        assert len({bytes(spec['pad'][b].numpy()) for b in range(CASES[n][0])}) > 1
    m3 = R.attn_geometry_inputs('explicit_bmask')[5]['mask']
    assert not torch.equal(m3[0], m3[1])
    # Tq < Tk under PREFIX with queries on both sides of the prefix end (and a q_off that is no multiple of 32), and under FULL
    B, h, Tq, Tk, mode = CASES['prefix_tq_lt_tk']
    assert mode == 'prefix' and Tq < Tk and (Tk - Tq) % 32 and any(Tk - Tq < x < Tk - 1 for x in R.ATTN_GEOMETRY_LENGTHS['prefix_tq_lt_tk']['x_len_dev'])
    assert CASES['full_tq_lt_tk'][4] == 'full' and CASES['full_tq_lt_tk'][2] < CASES['full_tq_lt_tk'][3]
    # a row without a key beside ordinary rows on the slab path, under both analytic masks
    assert {CASES[n][4] for n in R.ATTN_EMPTY_ROWS if CASES[n][3] > 256} == {'full', 'prefix'}
    for n, empty in R.ATTN_EMPTY_ROWS.items():
        assert CASES[n][2] == CASES[n][3] and all(R.ATTN_GEOMETRY_LENGTHS[n]['kv_len'][b] == 0 for b in empty) and len(empty) < CASES[n][0]
    assert set(G.BWD_CASES) == {n for n, c in CASES.items() if c[2] == c[3]} and 'explicit_shared' in G.BWD_CASES
    assert set(G.ANALYTIC_CASES) == {n for n, c in CASES.items() if c[4] != 'explicit'} and G.pytestmark.name == 'gpu'


# ---- C. the measurement behind the lse2 tolerance; a right kernel passes -----------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_fp32_emulation_error_is_what_the_gpu_file_says(name):
    ref, emu = R.attn_geometry_reference(name), R.attn_geometry_reference(name, torch.float32)
    kept = R.attn_kept_rows(name)
    written = G.ATTN_FP32_ERR[name]
    assert set(written) == set(ref)
    for qn in ref:
        err = R.worst(emu[qn][kept], ref[qn][kept])
        print(f'{name} {qn}: {err:.3e}')
        assert 0.25 * written[qn] <= err <= written[qn], f'{qn}: measured {err:.3e}, the GPU file says {written[qn]:.3e}'
    R.check_attn(name, emu, ref, written['lse2'])                  # the same arithmetic in fp32 passes every check
    # ... the large dv of a one-key row included: the rtol term carries it
    if name == 'full_small':
        assert float(ref['dv'].abs().max()) > 20 and written['dv'] < 6e-5 + 1e-4 * 20


def test_16bit_reference_rounds_the_operands_first():
    ref, r16 = R.attn_geometry_reference('prefix_mid'), R.attn_geometry_reference('prefix_mid', h16=torch.float16)
    assert 1e-4 < R.worst(r16['out'], ref['out']) < 1e-2
    q = R.attn_geometry_inputs('prefix_mid')[0]
    assert float(((q * R.ATTN_Q16_PRESCALE).half().double() / R.ATTN_Q16_PRESCALE - q.double()).abs().max()) > 0


# ---- D. planted faults ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fault', list(R.ATTN_FAULTS))
def test_planted_fault_is_rejected_with_margin(fault):
    """The fp32 emulation with the fault misses float64 by more than 10 x the GPU file's tolerance on every quantity named for
    it, on the case named for it; check_attn names those quantities."""
    name, expect = R.ATTN_FAULTS[fault]
    ref, bad = R.attn_geometry_reference(name), R.attn_geometry_reference(name, torch.float32, fault=fault)
    kept = R.attn_kept_rows(name)
    measured = G.ATTN_FP32_ERR[name]['lse2']
    miss = {qn: R.attn_miss(qn, bad[qn][kept], ref[qn][kept], measured) for qn in ref}
    print(fault, name, {qn: f'{m:.3g}' for qn, m in miss.items()})
    assert {qn for qn, m in miss.items() if m > 10} == set(expect), miss
    assert all(m <= 1 for qn, m in miss.items() if qn not in expect), miss
    with pytest.raises(AssertionError, match='failed: ') as e:
        R.check_attn(name, bad, ref, measured)
    assert set(str(e.value).split(' | ')[0][len('failed: '):].split(', ')) == set(expect)


def test_faults_that_need_their_case():
    """Where the geometry a fault turns on is absent the fault cannot show — which is why the case exists."""
    def missed(name, fault):
        ref, bad = R.attn_geometry_reference(name), R.attn_geometry_reference(name, torch.float32, fault=fault)
        return max(R.attn_miss(qn, bad[qn], ref[qn], G.ATTN_FP32_ERR[name]['lse2']) for qn in ref)
    assert missed('prefix_scalar', 'x_len_of_row0') <= 1           # one x_len for all rows
    assert missed('prefix_mid', 'no_q_off') <= 1                   # Tq == Tk
    assert missed('prefix_mid', 'tile_skipped_by_first_query') <= 1    # q_off a multiple of 32: a wave starts on a tile edge
    assert missed('prefix_mid', 'dq_chunk_extra') <= 1             # one chunk, which every row has keys in
    assert missed('explicit_shared', 'mask_of_row0') <= 1          # one mask for all rows
