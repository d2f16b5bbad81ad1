"""The host-side argument checks of the EnCodec encoder's entries (`vh_conv1d_wave`, `vh_conv1d_down`, `vh_rvq_encode`) under
AddressSanitizer + UBSan, CPU only: `make -C valle2_amd/csrc asan` links the stand-alone driver tests/abi/asan_codec_enc.cpp
against the sanitized host build of the library (device code untouched: no GPU sanitizer, no XNACK); the driver hands each entry
one bad argument at a time with "device pointers" into a FREED block, so a host-side dereference is a use-after-free report.
Nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / 'valle2_amd' / 'csrc'


def test_codec_encoder_host_checks_are_clean_under_asan_and_ubsan():
    if shutil.which('make') is None or not Path('/opt/rocm/bin/hipcc').exists():
        pytest.skip('make / hipcc not available')
    build = subprocess.run(['make', '-C', str(CSRC), '-j4', 'asan'], capture_output=True, text=True, timeout=1500)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(CSRC / 'asan' / 'asan_codec_enc')], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-6000:]
    assert 'checks passed' in run.stdout and 'ERROR: AddressSanitizer' not in run.stderr and 'runtime error' not in run.stderr
    assert int(run.stdout.split('asan_codec_enc:')[1].split()[0]) >= 122, run.stdout     # every call the driver makes today
