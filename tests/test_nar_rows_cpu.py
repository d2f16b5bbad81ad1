"""`engine.nar_rows`: the one row layout of ValleNAR's stage loop, padded and packed, against the formulas the two former
loops spelt out (generate_batch: utterance b at row b * max(len); generate_packed: at the running sum).  No device."""
import pytest

from valle2_amd.engine import NarRows, nar_rows, pack_plan

EDGES = [(10, 40, 100), (4, 2, 1), (7, 25, 96), (3, 60, 65), (12, 20, 32)]        # tests/test_packed_rows_gpu.py's EDGES lengths
CASES = {
    'one': [(4, 2, 1)],
    'equal': [(5, 3, 8)] * 3,
    'edges': EDGES,
    'no_prompt': [(6, 0, 9), (3, 5, 2)],
}


def _plan(case, packed):
    txs, tcs, tys = (list(v) for v in zip(*CASES[case]))
    return txs, tcs, tys, nar_rows(txs, tcs, tys, packed)


@pytest.mark.parametrize('case', CASES)
def test_padded_rows_are_the_former_generate_batch_formulas(case):
    txs, tcs, tys, p = _plan(case, False)
    B = len(txs)
    lens = [txs[b] + tcs[b] + tys[b] for b in range(B)]
    total = max(lens)
    assert isinstance(p, NarRows) and p.packed is False and p.lengths == lens
    assert p.starts == [b * total for b in range(B)]
    assert p.rows == B * total
    assert p.t0_prompt == [b * total + txs[b] for b in range(B)]
    assert p.t0_target == [b * total + txs[b] + tcs[b] for b in range(B)]
    assert p.target_rows == [t + (b * total + txs[b] + tcs[b]) for b in range(B) for t in range(tys[b])]
    starts = [0]
    for ty in tys:
        starts.append(starts[-1] + ty)
    assert p.logit_starts == starts
    assert p.kv_len == (lens if len(set(lens)) > 1 else None)


@pytest.mark.parametrize('case', CASES)
def test_packed_rows_are_the_former_generate_packed_formulas(case):
    txs, tcs, tys, p = _plan(case, True)
    B = len(txs)
    lens = [txs[b] + tcs[b] + tys[b] for b in range(B)]
    running, m = [], 0
    for n in lens:
        running.append(m)
        m += n
    assert p.packed is True and p.starts == running and p.rows == m == sum(lens)
    assert p.t0_prompt == [running[b] + txs[b] for b in range(B)]
    assert p.t0_target == [running[b] + txs[b] + tcs[b] for b in range(B)]
    assert p.target_rows == [t + (running[b] + txs[b] + tcs[b]) for b in range(B) for t in range(tys[b])]
    starts = [0]
    for ty in tys:
        starts.append(starts[-1] + ty)
    assert p.logit_starts == starts
    assert p.kv_len is None
    # the segments the packed attention runs over are pack_plan's
    assert p.lengths == lens and (p.starts, p.rows) == pack_plan(lens)[:2]


@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('case', CASES)
def test_every_target_row_lies_in_its_utterance_and_is_used_once(case, packed):
    txs, tcs, tys, p = _plan(case, packed)
    assert len(p.target_rows) == sum(tys) == p.logit_starts[-1] and len(set(p.target_rows)) == len(p.target_rows)
    for b in range(len(txs)):
        run = p.target_rows[p.logit_starts[b]:p.logit_starts[b + 1]]
        lo, hi = p.starts[b] + txs[b] + tcs[b], p.starts[b] + p.lengths[b]
        assert run == list(range(lo, hi)), f'utterance {b}: every row of [{lo}, {hi}) once, frame by frame'
        assert hi <= p.rows and (b + 1 == len(txs) or hi <= p.starts[b + 1])
    assert all(type(v) is int for v in p.starts + p.t0_prompt + p.t0_target + p.target_rows + p.logit_starts + [p.rows])


def test_padded_kv_len_is_none_exactly_when_all_lengths_are_equal():
    assert nar_rows([5, 5, 5], [3, 3, 3], [8, 8, 8], False).kv_len is None
    assert nar_rows([4], [2], [1], False).kv_len is None
    assert nar_rows([6, 5, 5], [3, 4, 3], [7, 7, 8], False).kv_len is None          # other parts, equal sums
    assert nar_rows([6, 3], [0, 5], [9, 2], False).kv_len == [15, 10]
    assert nar_rows([5, 5, 5], [3, 3, 3], [8, 8, 7], False).kv_len == [16, 16, 15]
