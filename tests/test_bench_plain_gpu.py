"""A plain `bench.py` run (no --full) at the small shapes: one JSON line with the headline fields and none of the
secondary legs, `--steps` timed steps, and `--dump-outputs` writing the last timed step's tokens, equal from run to run
(seeded weights and utterances)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
SECONDARY = ('prefill', 'decode_step', 'roofline', 'beams', 'default_generate', 'perf_mode', 'rows64', 'config5', 'nar',
             'train', 'cpu_baseline')


def _plain_run(out_dir):
    out = subprocess.run([sys.executable, str(REPO / 'bench.py'), '--small', '--gpus', '1', '--steps', '3', '--warmup', '1',
                          '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.startswith('{')]
    assert len(lines) == 1, out.stdout
    return lines[0]


def test_plain_small_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    r = _plain_run(tmp_path / 'a')
    assert r['steps'] == 3 and r['warmup'] == 1 and r['n_gpus'] == 1
    assert r['unit'] == 'tokens/s' and r['higher_is_better'] is True and r['dtype'] == 'f32'
    rows, new = r['config']['rows_per_gpu'], r['config']['new_tokens']
    assert r['ms_per_step'] > 0 and abs(r['value'] - rows * new / (r['ms_per_step'] * 1e-3)) <= 1e-6 * r['value']
    assert not [k for k in SECONDARY if k in r]
    tok = np.load(tmp_path / 'a' / 'tokens.npy')
    assert tok.dtype == np.float32 and tok.shape == (rows, 63 + 1 + new)      # --small: 63 prompt frames + BOS + new
    assert np.array_equal(tok, np.round(tok)) and tok.min() >= 0
    _plain_run(tmp_path / 'b')
    assert np.array_equal(tok, np.load(tmp_path / 'b' / 'tokens.npy'))
