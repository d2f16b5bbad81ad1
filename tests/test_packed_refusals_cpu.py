"""The refusal census of the eight packed entry points (tests/golden/gen_packed_refusals.py), replayed against the built
library: every single fault gives the recorded code and message, and of every pair of faults the recorded one is reported
— the order of the checks, which the single-fault tables of the other tests leave open.  Needs no device: every call
carries a fault and ends before anything is launched."""
import pytest

from tests.golden import gen_packed_refusals as G
from valle2_amd import _lib

RECORDED = G.OUT.read_text().splitlines()


@pytest.fixture(scope='module')
def replayed():
    return G.census(_lib.load_library())


def test_the_census_covers_every_entry_fault_and_pair():
    for entry, (_, _, faults) in G.ENTRIES.items():
        n = len(faults)
        lines = [line for line in RECORDED if line.startswith(entry + ' | ')]
        assert len(lines) == n + n * (n - 1) // 2, entry
    assert len(RECORDED) == sum(len(f) * (len(f) + 1) // 2 for _, _, f in G.ENTRIES.values())


def test_no_line_is_missing_or_new(replayed):
    assert len(replayed) == len(RECORDED)


@pytest.mark.parametrize('entry', list(G.ENTRIES))
def test_every_refusal_is_the_recorded_one(replayed, entry):
    mine = lambda lines: [line for line in lines if line.startswith(entry + ' | ')]   # noqa: E731
    differ = [f'{want}   BUT NOW   {got}' for want, got in zip(mine(RECORDED), mine(replayed)) if want != got]
    assert not differ, '\n'.join(differ)
