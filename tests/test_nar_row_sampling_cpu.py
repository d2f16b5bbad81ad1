"""Per-request sampling of the NAR stage (ValleNAR.generate_batch(sampling=[...]), codec_io.synthesize_requests,
vh_categorical_rows_keyed), the parts that need no GPU: the float64 mirror of one draw on hand-worked rows, the record a Sampling
hands the stage sampler and the stream its draws run on, what the entry points refuse before any device work, the signatures, the
plumbing of synthesize_requests, and what the C entry point refuses (called through ctypes with made-up, aligned pointers: nothing is
dereferenced)."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import nar_sampling_replay as NR
from tests import sampling_replay as SR
from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced
VH_OK, VH_EINVAL, VH_EALIGN = 0, -1, -2


# ---- 1. the mirror, the record, the stream -----------------------------------------------------------------------------------
def test_mirror_walks_the_whole_row_in_index_order():
    logits = [0.0, 3.0, 1.0, 2.0, -5.0]
    e = np.exp(np.array(logits))
    c = np.cumsum(e) / e.sum()                                           # boundaries after tokens 0, 1, 2, 3
    for u, want in ((0.0, 0), (c[0] - 1e-3, 0), (c[0] + 1e-3, 1), (c[1] - 1e-3, 1), (c[1] + 1e-3, 2), (c[2] + 1e-3, 3),
                    (c[3] + 1e-4, 4), (0.99999994, 4)):
        tok, amb, shares = NR.mirror_draw(logits, 1.0, u)
        assert (tok, amb) == (want, False), (u, tok, amb)
        assert np.allclose(shares, c, rtol=0, atol=1e-12)
    # within delta of an interior boundary: ambiguous on either side of it, not beyond
    assert NR.mirror_draw(logits, 1.0, c[1] + 3e-6)[:2] == (2, True) and NR.mirror_draw(logits, 1.0, c[1] - 3e-6)[:2] == (1, True)
    assert NR.mirror_draw(logits, 1.0, c[1] + 5e-6)[:2] == (2, False)
    # the last index is the fallback when no share exceeds u (the shares end at exactly 1.0, u is below it: forced here)
    assert NR.mirror_draw(logits, 1.0, 1.0)[0] == 4
    # the scale is the fp32 quotient 1.0f / temperature
    x = np.array(logits) * float(np.float32(1.0) / np.float32(0.6))
    c6 = np.cumsum(np.exp(x - x.max()))
    assert np.array_equal(NR.shares(logits, 0.6), c6 / c6[-1])
    # a greedy request: the arg-max of the unscaled logits, the lowest index on ties, never ambiguous
    assert NR.mirror_draw([2.0, 5.0, 5.0], 0.5, 0.9, greedy=True)[:2] == (1, False)
    # hold_rows: equal tokens pass, a neighbour passes only inside the band
    rows = np.array([logits, logits])
    assert NR.hold_rows(rows, [1, 2], [1.0, 1.0], [c[0] + 1e-3, c[1] + 3e-6]) == (1, 0, 0.0)
    amb, excused, worst = NR.hold_rows(rows, [1, 1], [1.0, 1.0], [c[0] + 1e-3, c[1] + 3e-6])
    assert (amb, excused) == (1, 1) and 2.9e-6 < worst < 3.1e-6
    with pytest.raises(AssertionError, match='row 0: the device drew 2, the mirror 1'):
        NR.hold_rows(rows, [2, 2], [1.0, 1.0], [c[0] + 1e-3, c[1] + 3e-6])


def test_nar_record_takes_the_configs_temperature_and_only_the_requests_own_greediness():
    from valle2_amd import ConfigValle, Sampling
    cfg = ConfigValle(top_k=50, tok_p=0.9, temperature=0.7)
    assert Sampling(7).nar_record(cfg) == (7, 0, 0, 1.0, 0.7)                       # None: the config's temperature
    assert Sampling(7, temperature=2).nar_record(cfg) == (7, 0, 0, 1.0, 2.0)
    assert Sampling(2 ** 64 - 1, top_k=1, temperature=0.5).nar_record(cfg) == (2 ** 64 - 1, 0, 1, 1.0, 0.5)
    # the stage has no filter: other top_k values and tok_p do not reach the record, and a greedy CONFIG does not make it greedy
    assert Sampling(7, top_k=8, tok_p=0.5).nar_record(cfg) == (7, 0, 0, 1.0, 0.7)
    assert Sampling(7).nar_record(ConfigValle(top_k=1, temperature=0.7)) == (7, 0, 0, 1.0, 0.7)
    with pytest.raises(ValueError, match='temperature=0.0'):
        Sampling(7).nar_record(ConfigValle(temperature=0.0))
    assert [f.name for f in __import__('dataclasses').fields(Sampling)] == ['seed', 'top_k', 'tok_p', 'temperature']


def test_nar_stream_keeps_the_stages_draws_apart_from_the_ar_stages():
    from valle2_amd.sampling import NAR_STREAM
    assert NAR_STREAM == 0x80000000
    for s in (0, 1, 2 ** 63 + 5):
        assert SR.uniform01(s, 1, 3) != SR.uniform01(s, 1, NAR_STREAM | 3)         # AR (beam 1, position 3) / NAR (frame 1, stage 3)
        assert NR.nar_uniform(s, 1, 3) == SR.uniform01(s, 1, NAR_STREAM | 3)
    # no audio position (< 5000) reaches a NAR stream, whatever the stage
    ar = {SR.uniform01(9, j, p) for j in range(4) for p in range(0, 5000, 7)}
    assert not ar & {NR.nar_uniform(9, t, n) for t in range(4) for n in range(1, 32)}


# ---- 2. refusals on a CPU model, signatures ----------------------------------------------------------------------------------
def _cpu_nar():
    from valle2_amd import ConfigValle, get_model_class
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='AdaptiveLayerNorm')
    return get_model_class('ValleNAR')(cfg)


def test_entry_points_refuse_before_any_device_work():
    """A CPU model: anything that went on to the device would raise VhError (no device) or copy the model there."""
    from valle2_amd import Sampling
    m = _cpu_nar()
    a = Sampling(1)
    texts, pcs, firsts = [torch.arange(5)] * 2, [torch.zeros(4, 8, dtype=torch.int64)] * 2, [torch.arange(7)] * 2
    with pytest.raises(ValueError, match=r'generate_batch: sampling together with seed='):
        m.generate_batch(texts, pcs, firsts, seed=3, sampling=[a, a])
    with pytest.raises(ValueError, match=r'generate_batch: utterance 1 carries no Sampling'):
        m.generate_batch(texts, pcs, firsts, sampling=[a, None])
    with pytest.raises(ValueError, match=r'generate_batch: sampling holds 1 entries for 2 utterances'):
        m.generate_batch(texts, pcs, firsts, sampling=[a])
    with pytest.raises(ValueError, match=r'generate_batch: sampling of utterance 1 is dict, not a valle2_amd.Sampling'):
        m.generate_batch(texts, pcs, firsts, sampling=[a, dict(seed=1)])
    with pytest.raises(ValueError, match=r'generate_batch: sampling is Sampling, not a list'):
        m.generate_batch(texts, pcs, firsts, sampling=a)
    with pytest.raises(ValueError, match=r'generate: sampling is int, not a valle2_amd.Sampling'):
        m.generate(torch.arange(3), pcs[0], torch.arange(2), firsts[0], sampling=5)
    m.config.temperature = 0.0                                                      # the config's value is the request's
    with pytest.raises(ValueError, match=r'temperature=0.0'):
        m.generate_batch(texts, pcs, firsts, sampling=[a, a])


def test_signatures_gain_only_the_keyword_only_sampling():
    from valle2_amd import codec_io as CIO
    from valle2_amd.valle_nar import ValleNAR
    assert list(inspect.signature(ValleNAR.generate).parameters) == \
        ['self', 'prompt_tokens', 'prompt_codes', 'target_tokens', 'target_codes_first_layer', 'greedy', 'sampling']
    assert list(inspect.signature(ValleNAR.generate_batch).parameters) == \
        ['self', 'texts', 'prompt_codes', 'first_layers', 'greedy', 'seed', 'perf_mode', 'sampling']
    for fn in (ValleNAR.generate, ValleNAR.generate_batch):
        ps = inspect.signature(fn).parameters
        assert ps['sampling'].kind is inspect.Parameter.KEYWORD_ONLY and ps['sampling'].default is None
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n, p in ps.items() if n != 'sampling')
        assert ps['greedy'].default is False
    ps = inspect.signature(CIO.synthesize_requests).parameters
    assert list(ps) == ['ar', 'nar', 'items', 'codec', 'queued', 'slots']
    assert ps['codec'].default is None and ps['queued'].default is False and ps['slots'].default is None
    assert all(ps[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ('queued', 'slots'))
    # the entries that hand the fourth element to the AR model only keep their parameter lists
    assert list(inspect.signature(CIO.synthesize_many).parameters) == ['ar', 'nar', 'items', 'codec', 'greedy_nar']
    assert list(inspect.signature(CIO.synthesize_queued).parameters) == ['ar', 'nar', 'items', 'codec', 'greedy_nar', 'slots']


def test_synthesize_requests_hands_the_sampling_to_both_stages(monkeypatch):
    from valle2_amd import ConfigValle, Sampling, codec_io as CIO, get_model_class
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=2)
    ar = get_model_class('ValleAR')(cfg)
    seen = {}

    class Nar:
        def generate_batch(self, texts, prompts, firsts, greedy=False, *, sampling=None):
            seen['nar'] = (len(texts), len(prompts), len(firsts), greedy, sampling)
            return [torch.full((3, cfg.num_quantizers), i, dtype=torch.int64) for i in range(len(texts))]

    def ar_many(utts, **kw):
        seen['ar'] = ('many', kw, [u[3:] for u in utts])
        return [torch.arange(3)] * len(utts)

    def ar_queued(utts, **kw):
        seen['ar'] = ('queued', kw, [u[3:] for u in utts])
        return [torch.arange(3)] * len(utts)
    monkeypatch.setattr(ar, 'generate_many', ar_many)
    monkeypatch.setattr(ar, 'generate_queued', ar_queued)
    a, b = Sampling(1), Sampling(2, top_k=8, temperature=0.8)
    item = (torch.arange(4), torch.zeros(cfg.num_quantizers, 5, dtype=torch.int64), torch.arange(3))
    out = CIO.synthesize_requests(ar, Nar(), [item + (a,), item + (b,)])
    assert seen['ar'] == ('many', {}, [(a,), (b,)]) and seen['nar'] == (2, 2, 2, False, [a, b])
    assert [tuple(o.shape) for o in out] == [(cfg.num_quantizers, 3)] * 2 and int(out[1][0, 0]) == 1     # (Q, Ty), in order
    CIO.synthesize_requests(ar, Nar(), [item + (b,), item + (a,)], queued=True, slots=1)
    assert seen['ar'] == ('queued', dict(slots=1), [(b,), (a,)]) and seen['nar'][4] == [b, a]
    with pytest.raises(ValueError, match=r'synthesize_requests: item 1 carries no valle2_amd.Sampling'):
        CIO.synthesize_requests(ar, Nar(), [item + (a,), item])
    with pytest.raises(ValueError, match=r'synthesize_requests: item 0 carries no valle2_amd.Sampling'):
        CIO.synthesize_requests(ar, Nar(), [item + (None,), item + (a,)])
    with pytest.raises(ValueError, match=r'synthesize_requests: item 0 carries no valle2_amd.Sampling'):
        CIO.synthesize_requests(ar, Nar(), [item + (dict(seed=1),)])


# ---- 3. the C entry point ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


def test_header_declares_and_the_library_exports_the_keyed_launch(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    assert re.search(r'\bint vh_categorical_rows_keyed\(', header)
    assert 'vh_categorical_rows_keyed' in _lib.SIGNATURES
    assert L.vh_categorical_rows_keyed.argtypes == _lib.SIGNATURES['vh_categorical_rows_keyed'][1]
    assert len(_lib.SIGNATURES['vh_categorical_rows_keyed'][1]) == 15
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 136
    assert 'ABI 136' in (REPO / 'INTEGRATION.md').read_text()


def test_keyed_launch_refuses_before_any_gpu_work(L):
    def call(logits=P, ld=1028, V=1025, rows=6, requests=P2, n_requests=3, row_request=I32, row_key=I32, n_keys=70, tokens=P,
             request_stride=560, key_stride=8):
        return L.vh_categorical_rows_keyed(logits, ld, V, rows, requests, n_requests, row_request, row_key, n_keys, 0x80000003,
                                           tokens, request_stride, key_stride, None, None)
    for kw, rc, text in ((dict(logits=None), VH_EINVAL, 'null logits'), (dict(requests=None), VH_EINVAL, 'null requests'),
                         (dict(row_request=None), VH_EINVAL, 'null row_request'), (dict(row_key=None), VH_EINVAL, 'row_key'),
                         (dict(tokens=None), VH_EINVAL, 'null tokens'), (dict(V=0), VH_EINVAL, 'V=0'),
                         (dict(ld=1024), VH_EINVAL, 'ld=1024'), (dict(rows=-1), VH_EINVAL, 'rows=-1'),
                         (dict(n_requests=0), VH_EINVAL, 'n_requests=0'), (dict(n_keys=0), VH_EINVAL, 'n_keys=0'),
                         (dict(request_stride=0), VH_EINVAL, 'request_stride=0'), (dict(key_stride=0), VH_EINVAL, 'key_stride=0'),
                         (dict(requests=P2 + 8), VH_EALIGN, 'requests must be 16-byte aligned')):
        assert call(**kw) == rc and 'vh_categorical_rows_keyed' in _err(L) and text in _err(L), (kw, _err(L))
    assert call(rows=0) == VH_OK                                                    # nothing to draw: no launch
    assert call(rows=0, requests=P2 + 8) == VH_EALIGN                               # ... but the arguments are checked first
