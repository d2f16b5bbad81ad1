"""tests/train_gemm_paths.py without a GPU: the walk leaves no path signature without a case, the host-plan mirrors agree with
the library's own *_ws_bytes, every written figure of tests/test_train_gemm_paths_gpu.py is reproduced here from fp32 arithmetic
on the CPU, the asserted bounds stay at or below the derived caps, the fault-free emulations pass every case, every planted
fault misses its case's bound by more than ten times, and the integer flavour is exact.  Run with -s for the tables."""
import pytest
import torch

from tests import oracle_runners as R
from tests import test_train_gemm_paths_gpu as G
from tests import train_gemm_paths as P
from valle2_amd import _lib

FAULT_MARGIN = 10.0


def test_sum_margin_and_rounding_rule_are_the_projects():
    from tests import attn_scores
    assert P.SUM_MARGIN is R.SUM_MARGIN and P.written_figure is attn_scores.written_figure and P.written_figure(1.234e-3) == 1.5e-3


# ---- the walks ------------------------------------------------------------------------------------------------------------
def test_linear_ex_walk_leaves_no_signature_without_a_case():
    """Every pair of signatures (LDS-DMA staging, register staging) the mirrors produce over the enumerated domain has a case, the
    required geometries are all there, and the bodies / stagings / split counts of csrc/gemm.hip all occur."""
    walk = P.lin_walk()
    # a denser sweep than the domain the walk was built from: every M / N class around the tile and chunk edges, every K class
    pair = lambda M, N, K: (P.lin_signature(M, N, K, tile_dma=0), P.lin_signature(M, N, K, tile_dma=1))
    rows = sorted(set(range(1, 300, 7)) | {64, 65, 127, 128, 129, 255, 256, 257})
    missing = {pair(M, N, K): (M, N, K) for M in rows for N in range(1, 300) for K in (16, 32, 48, 64)} .keys() - set(walk)
    assert not missing, [P.describe_signature(s[0]) for s in missing]
    # the tail split over whole 17 .. 79 row tiles x K = 128 .. 1024: nothing new but the split counts between the walk's 2, 3 and 8
    # (the same loops of gemm_tile_dma_kernel and tile_tail_fixup_kernel at another trip count)
    walked = {(d._replace(split=0), r) for d, r in walk}
    for m in range(17, 80):
        for d in (0, 37):
            for N in (640, 2048):
                for K in range(128, 1056, 32):
                    dma, reg = pair(m * 128 - d, N, K)
                    assert (dma._replace(split=0), reg) in walked and ((dma, reg) in walk or dma.split in (4, 5, 6, 7)), (m, d, N, K)
    assert {(M, N, K) for M, N, K, _ in P.LIN_REQUIRED} <= {tuple(g) for g in P.lin_geoms()}
    print()
    for (dma, reg), geoms in walk.items():
        print(f'{", ".join("x".join(map(str, g)) for g in geoms):42s} {P.describe_signature(dma)} | {P.describe_signature(reg)}')
    sigs = [s for pair in walk for s in pair]
    assert {b for s in sigs for b in s.bodies} == {'interior', 'edge-whole', 'ragged-column', 'fix-up'}
    assert {s.split for s in sigs} >= {0, 2, 3, 8} and {s.staging for s in sigs} == {'dma', 'reg'}
    assert any(s.tail_ragged_m for s in sigs) and any(s.split and not s.tail_ragged_m for s in sigs)
    # what the issue's table says of its shapes
    assert P.tail_plan(2176, 2048, 256)[0] == 2 and P.tail_plan(2176, 2048, 384)[0] == 3 and P.tail_plan(2176, 2048, 1024)[0] == 8
    assert P.n_tiles(3072, 2048) % 256 == 128 and P.tail_plan(3072, 2048, 256)[0] == 2
    assert P.n_tiles(9856, 640) % 256 == 129 and P.tail_plan(9856, 640, 256)[0] == 0 and P.tail_plan(2176, 2048, 224)[0] == 0
    # every epilogue the entry accepts occurs on every body and both stagings (dropout: LDS-DMA only, whole column groups only)
    for body in ('interior', 'edge-whole', 'ragged-column', 'fix-up'):
        for td in (0, 1):
            have = {c.epi for c in P.lin_cases() if c.tile_dma == td and body in P.lin_signature(*c.geom, tile_dma=td).bodies}
            want = {n for n in P.LIN_EPIS if not (P.epi_of(n).drop and td == 1)}
            if body == 'fix-up':
                want = want if td == 0 else set()
            if body == 'ragged-column':
                want = {n for n in want if not P.epi_of(n).colsum and not P.epi_of(n).drop}
            assert want <= have, (body, td, want - have)


def test_gemm_tn_walk_leaves_no_signature_without_a_case():
    walk = P.tn_walk()
    # every contraction length up to 1400 rows, not only the lengths the walk was built from
    missing = {P.tn_signature(M, NI, NJ, w) for M in range(1, 1400) for NI, NJ in P.TN_SHAPES for w in P.TN_DOMAIN['wgs']} - set(walk)
    assert not missing, [P.describe_signature(s) for s in missing]
    assert {tuple(c) for c in P.TN_REQUIRED} <= {tuple(c) for c in P.tn_cases()}
    print()
    for sig, cases in walk.items():
        print(f'{", ".join(P.tn_case_id(c) for c in cases):40s} {P.describe_signature(sig)}')
    assert {s.first for s in walk} | {s.last for s in walk} == {f'{lp}+{r}' for lp in ('loop', 'noloop') for r in (1, 2, 3)} - {'loop+1'}
    assert {s.slices for s in walk} == {'one', 'all', 'fewer'}
    # what the issue's table says of its shapes
    assert P.tn_plan(511, 128, 128)[1:] == (256, 2) and P.tn_plan(513, 128, 128)[1:] == (288, 2)
    assert P.tn_plan(2049, 128, 128) == (8, 288, 8) and 2049 - 7 * 288 == 33
    assert P.tn_plan(4321, 128, 128, 16) == (16, 288, 16) and 4321 - 15 * 288 == 1            # the last slice is ONE row
    assert P.tn_plan(16385, 256, 256) == (64, 288, 57)
    assert P.tn_plan(800, 260, 130, 12)[0] == 2 and P.tn_plan(800, 260, 130)[0] == 3


def test_loop_tail_never_sees_one_slab_after_the_loop():
    """`for (kt = 0; kt + 3 < nk; kt += 2)` leaves 2 or 3 slabs once taken; 1 slab is left only where nk == 1."""
    for rows in range(1, 40 * 32):
        cls = P.tn_loop_class(rows)
        assert cls != 'loop+1' and (cls == 'noloop+1') == (rows <= 32)


def test_mirrors_agree_with_the_library():
    L = _lib.load_library()                          # host-only entry points: no device needed
    gen = torch.Generator().manual_seed(5)
    shapes = [tuple(g) for g in P.lin_geoms()] + [tuple(int(x) for x in torch.randint(1, 12000, (3,), generator=gen)) for _ in range(300)]
    shapes += [(int(m) * 128 - int(d), int(n) * 128, int(k) * 32) for m, d, n, k in torch.randint(1, 40, (300, 4), generator=gen)]
    for M, N, K in shapes:
        assert L.vh_linear_ex_ws_bytes(M, N, K) == P.linear_ex_ws_bytes(M, N, K), (M, N, K)
    assert sum(1 for s in shapes if P.linear_ex_ws_bytes(*s)) > 20
    tn = [tuple(c) for c in P.tn_cases()]
    tn += [(int(m), int(i), int(j), int(w)) for m, i, j, w in zip(torch.randint(1, 20000, (300,), generator=gen),
                                                                  torch.randint(1, 1100, (300,), generator=gen),
                                                                  torch.randint(1, 2100, (300,), generator=gen),
                                                                  torch.randint(0, 5, (300,), generator=gen) * 100)]
    try:
        for M, NI, NJ, wgs in tn:
            L.vh_set_tuning(P.KNOB_TN_WGS, wgs)
            assert L.vh_gemm_tn_ws_bytes(M, NI, NJ) == P.tn_ws_bytes(M, NI, NJ, wgs), (M, NI, NJ, wgs)
    finally:
        L.vh_set_tuning(P.KNOB_TN_WGS, 0)


# ---- figures, bounds, emulations ------------------------------------------------------------------------------------------------
def test_tables_hold_exactly_the_cases():
    assert set(G.LIN_FP32_ERR) == set(G.lin_keys())
    assert set(G.TN_FP32_ERR) == {P.tn_case_id(c) for c in P.tn_cases()}
    assert set(G.BATCHED_FP32_ERR) == {P.batched_case_id(c) for c in P.batched_cases()}
    for key in G.lin_keys():
        c = next(c for c in P.lin_cases() if P.lin_figure_key(c) == key)
        e = P.epi_of(c.epi)
        assert [f is not None for f in G.LIN_FP32_ERR[key]] == [True, bool(e.pre_out), bool(e.colsum)], key


def still_holds(written, measured, what):
    """The written figure is the measured one through written_figure; a re-measurement on another CPU may land a little lower."""
    assert 0.25 * written <= measured <= written, f'{what}: written {written:.2e}, measured {measured:.2e}'
    assert P.bound_factor(written) <= 1.0            # the asserted bound is at most the derived cap (the cap itself at 1)


@pytest.mark.parametrize('g', P.lin_geoms(), ids=lambda g: 'x'.join(map(str, g)))
def test_linear_ex_figures_emulations_and_integer_flavour(g):
    """Per geometry, every epilogue: the written figures re-measured; the fault-free emulations (plain fp32, slab order with and
    without the tail split, the FMA chain) inside the asserted bound; the integer flavour exact in the emulation."""
    for key in G.lin_keys():
        c = next(c for c in P.lin_cases() if P.lin_figure_key(c) == key)
        if c.geom != g:
            continue
        e, figs = P.epi_of(c.epi), G.lin_figures(key)
        for q, m in P.lin_measure(c).items():
            still_holds(figs[q], m, f'{key} {q}')
            assert m <= P.bound_factor(figs[q]), f'{key} {q}: the correct emulation misses the bound'
        ref = P.lin_reference(c, 'int')
        inp = P.lin_inputs(g, 'int')
        assert float(P.lin_products(g, 'int')[1].max()) + 8 < 2 ** 24          # every partial sum, in any order, is exact
        for knob in (0, 1):
            em = P.lin_emulate(c, 'int', knob)
            for q, (v, cap) in ref.items():
                if G.lin_exact(e, q):
                    if q == 'colsum':
                        assert float(ref['out'][0].abs().sum(0).max()) < 2 ** 24
                    assert torch.equal(em[q].double(), v), f'{key} {q}: integer flavour, knob {knob}'
                else:
                    assert P.worst_ratio(em[q], v, cap) <= 1.0, f'{key} {q}: integer flavour against the cap'
        assert g.N < 16 or inp['w'][:, 0].unique().numel() > 7                 # the asymmetric column


def test_gemm_tn_figures_emulations_and_integer_flavour():
    fell_back = []
    for c in P.tn_cases():
        written, m = G.TN_FP32_ERR[P.tn_case_id(c)], P.tn_measure(c)
        still_holds(written, m, P.tn_case_id(c))
        assert m <= P.bound_factor(written)
        if P.SUM_MARGIN * written > 1:
            fell_back.append(P.tn_case_id(c))
        ref, S = P.tn_reference(c, 'int')
        assert float(S.max()) < 2 ** 24 and torch.equal(P.tn_emulate(c, 'int').double(), ref), P.tn_case_id(c)
    print('\nbound = the derived cap (SUM_MARGIN x figure exceeds it):', ', '.join(fell_back))


def test_gemm_batched_figures_emulations_and_integer_flavour():
    for c in P.batched_cases():
        written, m = G.BATCHED_FP32_ERR[P.batched_case_id(c)], P.batched_measure(c)
        still_holds(written, m, P.batched_case_id(c))
        assert m <= P.bound_factor(written)
        ref, S = P.batched_reference(c, 'int')
        assert float(S.max()) < 2 ** 24 and torch.equal(P.batched_emulate(c, 'int').double(), ref)
    assert {P.batched_splits(c.M, c.N, c.K, c.nb, c.nh) > 1 for c in P.batched_cases()} == {False, True}
    assert all(c.K % 4 for c in P.batched_cases())


# ---- planted faults ----------------------------------------------------------------------------------------------------------
def test_planted_faults_miss_their_bounds():
    """Each fault, emulated in fp32 on its case, is more than FAULT_MARGIN times the asserted bound away from float64."""
    assert set(P.LIN_FAULT_CASES) == set(P.LIN_FAULTS) and set(P.TN_FAULT_CASES) == set(P.TN_FAULTS)
    print()
    for fault, c in P.LIN_FAULT_CASES.items():
        assert c in P.lin_cases()
        ref, figs = P.lin_reference(c, 'float'), G.lin_figures(P.lin_figure_key(c))
        bad, good = P.lin_emulate(c, 'float', fault=fault), P.lin_emulate(c, 'float')
        miss = max(P.worst_ratio(bad[q], *ref[q]) / P.bound_factor(figs[q]) for q in ref)
        ok = max(P.worst_ratio(good[q], *ref[q]) / P.bound_factor(figs[q]) for q in ref)
        print(f'linear_ex {fault:24s} on {P.lin_case_id(c):32s} {miss:12.1f} x the bound (fault-free: {ok:.2f})')
        assert miss > FAULT_MARGIN and ok <= 1.0
    for fault, c in P.TN_FAULT_CASES.items():
        assert c in P.tn_cases()
        ref, S = P.tn_reference(c, 'float')
        cap, factor = P.tn_cap(c, S), P.bound_factor(G.TN_FP32_ERR[P.tn_case_id(c)])
        miss = P.worst_ratio(P.tn_emulate(c, 'float', fault=fault), ref, cap) / factor
        print(f'gemm_tn   {fault:24s} on {P.tn_case_id(c):32s} {miss:12.1f} x the bound')
        assert miss > FAULT_MARGIN
        assert not torch.equal(P.tn_emulate(c, 'int', fault=fault).double(), P.tn_reference(c, 'int')[0])    # and the exact check


def test_planted_transpose_faults_are_seen():
    """The transposes are compared exactly: a fault is seen when any element differs (sentinels where nothing was written)."""
    for rows, cols, ldo in P.TRANSPOSE_CASES:
        w = torch.randn(rows, cols, generator=torch.Generator().manual_seed(1))
        want = torch.zeros(cols, ldo)
        want[:, :rows] = w.T
        assert torch.equal(P.transpose_emulate(w, ldo), want)
        assert (ldo == rows) == torch.equal(P.transpose_emulate(w, ldo, 'padding_unwritten'), want)
    assert any(ldo > rows for rows, _, ldo in P.TRANSPOSE_CASES)
    for n in P.PLAN_COUNTS:
        weights, ldos = P.plan_weights(n)
        want = [P.transpose_emulate(w, ldo) for w, ldo in zip(weights, ldos)]
        good, bad = P.plan_emulate(weights, ldos), P.plan_emulate(weights, ldos, 'item_off_by_one')
        assert all(torch.equal(x, y) for x, y in zip(good, want))
        wrong = [i for i, (x, y) in enumerate(zip(bad, want)) if not torch.equal(x, y)]
        assert wrong == list(range(1, n)), n                # every item but the first loses its first tile
        print(f'transpose_many off by one at a tile0 boundary, {n} items: {len(wrong)} outputs differ')
    shapes = P.plan_shapes(130)
    one_tile = [i for i, (r, c, ldo) in enumerate(shapes) if c <= 32 and ldo <= 32]
    assert one_tile and any(i + 1 in one_tile for i in one_tile)          # first tile == the previous item's last + 1
    assert len(set(shapes)) >= 6


def test_dropout_fields_of_the_cases_are_the_oracles():
    from oracle import philox
    for flavour, p in P.DROP_P.items():
        keep = P.keep_field(flavour, 130, 256)
        assert torch.equal(keep, torch.from_numpy(philox.keep_field(P.DROP_SEED, P.DROP_SITE, p, 130, 256)).float())
        assert abs(float(keep.mean()) - (1 - p)) < 0.02
    assert P.drop_scale('int') == 2.0 and abs(P.drop_scale('float') - 1 / 0.9) < 1e-6
