"""Up to 32 codebooks and audio vocabularies up to 16384, the parts that need no GPU: the CPU oracle against the real
reference's fixture (tests/golden/codebooks.npz, gen_golden_codebooks.py), the library's new entry point and its argument
checks (refused before any device is touched), the header limits, and the compiled code of the new kernel forms."""
import ctypes as C
import os
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests.golden import cases as GC
from tests.golden.gen_golden_codebooks import (NAR_Q, NAR_Q_STAGES, PREP_STRIDE, WIDE_FILTERS, ar_v4096_inputs,
                                               nar_q_inputs, wide_sampling_inputs)
from tests.oracle_runners import load_golden

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize('which', sorted(NAR_Q))
def test_oracle_nar_with_many_codebooks_matches_the_reference(which):
    from oracle import valle_oracle as O
    gold = load_golden('codebooks')
    kw, sd, batch = nar_q_inputs(which)
    cfg = GC.cfg_of(kw)
    assert cfg.num_quantizers > 8
    for stage in NAR_Q_STAGES[which]:
        y, p = O.nar_prepare_audio_codes(sd, cfg, batch['codes'], stage)
        assert p == int(gold[f'{which}_prefix_{stage}'])
        torch.testing.assert_close(y[:, :, ::PREP_STRIDE], gold[f'{which}_prep_{stage}'], rtol=1e-6, atol=1e-6)
        logits, _ = O.nar_stage_logits(sd, cfg, batch, stage)
        torch.testing.assert_close(logits, gold[f'{which}_logits_{stage}'], rtol=1e-5, atol=1e-5)


def test_oracle_greedy_generate_at_4096_audio_tokens_matches_the_reference():
    from oracle import valle_oracle as O
    gold = load_golden('codebooks')
    kw, sd, utt = ar_v4096_inputs()
    trace = {}
    tokens = O.ar_generate(sd, GC.cfg_of(kw), *utt, trace=trace)
    assert torch.equal(tokens, gold['v4096_tokens'])
    torch.testing.assert_close(torch.tensor(trace['margin']), gold['v4096_margin'], atol=2e-5, rtol=2e-5)


@pytest.mark.parametrize('case', range(len(WIDE_FILTERS)))
def test_oracle_filter_at_4097_matches_the_reference(case):
    from oracle import valle_oracle as O
    gold = load_golden('codebooks')
    top_k, top_p, temp = WIDE_FILTERS[case]
    filt = O._top_k_top_p_filter(wide_sampling_inputs() / temp, top_k=top_k, top_p=top_p)
    assert torch.equal(torch.isfinite(filt), gold[f'filter_keep_{case}'])
    torch.testing.assert_close(F.log_softmax(filt, dim=-1), gold[f'filter_logprobs_{case}'], rtol=1e-6, atol=1e-6)
    if case == 0:
        assert int(filt[0].isfinite().sum()) == 51        # row 0 ties at the 50th place: both kept


def _header():
    return (REPO / 'include' / 'valle_hip.h').read_text()


def test_header_limits():
    h = _header()
    assert int(re.search(r'#define VH_MAX_TABLES (\d+)', h).group(1)) >= 32
    assert int(re.search(r'#define VH_SAMPLE_MAX_V (\d+)', h).group(1)) == 16384
    assert int(re.search(r'#define VH_VERSION (\d+)', h).group(1)) >= 129
    assert 'int vh_sample_step_wide(' in h


def _lib():
    from valle2_amd import _lib
    try:
        return _lib.load_library()
    except OSError as e:                                  # (build() makes it)
        pytest.skip(f'libvalle_hip.so not built: {e}')


def test_library_exports_the_wide_sampler():
    lib = _lib()
    assert hasattr(lib, 'vh_sample_step_wide')
    assert lib.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', _header()).group(1))


def test_wide_sampler_refuses_bad_arguments_before_touching_a_device():
    """Every call below is refused by the argument checks (nothing is launched): the pointers are never dereferenced."""
    lib = _lib()
    P = 1 << 20                                           # a 16-byte aligned address that is never read

    def call(V=4097, ldl=4100, temperature=1.0, logits=P, codes=P, x_next=P, B=2, d=64):
        return lib.vh_sample_step_wide(logits, ldl, V, V - 1, 50, 1.0, temperature, 1, codes, 4, P, None, None, P, P, P,
                                       P, x_next, B, d, None)

    for kw, what in [(dict(V=16385, ldl=16388), '16384'), (dict(V=0), 'bad dims'), (dict(ldl=4096), 'bad dims'),
                     (dict(B=0), 'bad dims'), (dict(d=62), 'bad dims'),
                     (dict(logits=None), 'null'), (dict(codes=None), 'null'), (dict(x_next=None), 'null'),
                     (dict(temperature=0.0), 'temperature'), (dict(temperature=-1.0), 'temperature'),
                     (dict(temperature=float('nan')), 'temperature')]:
        rc = call(**kw)
        assert rc != 0, kw
        assert what in lib.vh_last_error().decode(), (kw, lib.vh_last_error())
    # the narrow entry point keeps its limit
    rc = lib.vh_sample_step(P, 4100, 4097, 4096, 50, 1.0, 1.0, 1, P, 4, P, None, None, P, P, P, P, P, 2, 64, None)
    assert rc != 0 and '2048' in lib.vh_last_error().decode()


def test_embedding_sum_refuses_more_than_32_tables_before_touching_a_device():
    lib = _lib()
    P = 1 << 20
    tabs = (C.c_void_p * 33)(*([P] * 33))
    voc = (C.c_int32 * 33)(*([4] * 33))
    rc = lib.vh_embed_sum_pe(P, 1, 1, 1, tabs, voc, 33, P, 0, None, P, 64, 0, 1, 1, 64, None, None, None, None, None)
    assert rc != 0 and '1..32' in lib.vh_last_error().decode()


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not installed')
def test_new_kernel_forms_have_no_scratch():
    sys.path.insert(0, str(REPO / 'tools'))
    import check_isa
    asm = check_isa.compile_elementwise_asm()
    problems = check_isa.check_no_scratch(asm)
    assert not problems, '\n'.join(problems)
