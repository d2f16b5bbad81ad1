"""Per-utterance sampling (valle2_amd.Sampling: seed, top-k, top-p and temperature per request), the parts that need no GPU:
what Sampling and the entry points refuse before any device work, the float64 mirror of the sampler decoding the audit model
under the seeds the GPU cases use (tests/sampling_replay.py), the plan and slot key of a call with row sampling, and the C
ABI: vh_row_sampling, the two `_rows` entry points and the decoder's `row_sampling` field (descriptors checked through ctypes
with made-up, aligned pointers: nothing is dereferenced)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from tests import oracle_runners as R
from tests import sampling_replay as SR
from tests.golden import cases as GC
from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


# ---- 1. Sampling and the entry points, on a CPU model ------------------------------------------------------------------------
def test_sampling_is_exported_and_keeps_what_it_is_given():
    import valle2_amd
    from valle2_amd import ConfigValle, Sampling
    assert 'Sampling' in valle2_amd.__all__
    s = Sampling(7, top_k=8, tok_p=0.9, temperature=0.8)
    assert (s.seed, s.top_k, s.tok_p, s.temperature) == (7, 8, 0.9, 0.8)
    assert Sampling(2 ** 64 - 1).top_k is None and Sampling(0) == Sampling(0)
    cfg = ConfigValle(top_k=50, tok_p=1.0, temperature=0.7)
    assert Sampling(3).resolved(cfg) == (50, 1.0, 0.7)                       # None: the config's value
    assert Sampling(3, top_k=1, temperature=2).resolved(cfg) == (1, 1.0, 2.0)
    # the records of an utterance's rows: beam j carries key j, whatever its place in a call
    assert s.records(cfg, 3) == [(7, 0, 8, 0.9, 0.8), (7, 1, 8, 0.9, 0.8), (7, 2, 8, 0.9, 0.8)]
    assert s.records(cfg, 1, first_key=2) == [(7, 2, 8, 0.9, 0.8)]
    # a plain value: what prints the same compares the same
    assert s == Sampling(7, top_k=8, tok_p=0.9, temperature=0.8) and hash(s) == hash(Sampling(7, 8, 0.9, 0.8))
    assert [f.name for f in __import__('dataclasses').fields(Sampling)] == ['seed', 'top_k', 'tok_p', 'temperature']
    from valle2_amd import sampling as S
    rows = S.beam_rows(s, 3)
    assert [r.records(cfg, 1) for r in rows] == [[rec] for rec in s.records(cfg, 3)] and S.check_list('e', rows, 3) == rows


@pytest.mark.parametrize('kw,text', [
    (dict(seed=-1), 'seed=-1'), (dict(seed=2 ** 64), 'seed='), (dict(seed=1.5), 'seed=1.5'), (dict(seed=True), 'seed=True'),
    (dict(seed=1, top_k=-1), 'top_k=-1'), (dict(seed=1, top_k=2.0), 'top_k=2.0'), (dict(seed=1, top_k=2 ** 31), 'top_k='),
    (dict(seed=1, tok_p=0.0), 'tok_p=0.0'), (dict(seed=1, tok_p=1.5), 'tok_p=1.5'), (dict(seed=1, tok_p='x'), "tok_p='x'"),
    (dict(seed=1, temperature=0.0), 'temperature=0.0'), (dict(seed=1, temperature=-1.0), 'temperature=-1.0'),
    (dict(seed=1, temperature=float('nan')), 'temperature=nan'), (dict(seed=1, temperature=float('inf')), 'temperature=inf'),
])
def test_sampling_validates_the_usual_ranges(kw, text):
    from valle2_amd import Sampling
    with pytest.raises(ValueError, match=re.escape(text)):
        Sampling(**kw)


def _cpu_model(**kw):
    from valle2_amd import ConfigValle, get_model_class
    cfg = ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm',
                                  num_beams=4, top_k=50, max_audio_len=8), **kw))
    return get_model_class('ValleAR')(cfg)


def _utt(sampling=..., n=7):
    pt, codes, tt = torch.arange(5), torch.arange(n * 8).reshape(n, 8) % 1024, torch.arange(10, 13)
    return (pt, codes, tt) if sampling is ... else (pt, codes, tt, sampling)


def test_utterances_of_three_or_four_elements():
    from valle2_amd import Sampling, generation as G
    from valle2_amd import sampling as S
    a, b = Sampling(1), Sampling(2, top_k=8)
    texts, firsts = G.unpack_utterances([_utt(a), _utt(b)])
    plain = G.unpack_utterances([_utt(), _utt()])
    assert all(torch.equal(x, y) for x, y in zip(texts + firsts, plain[0] + plain[1]))
    assert S.of_utterances('e', [_utt(a), _utt(b)]) == [a, b]
    assert S.of_utterances('e', [_utt(), _utt(None)]) is None and S.of_utterances('e', []) is None
    with pytest.raises(ValueError, match='utterance 1 carries no Sampling'):
        S.of_utterances('e', [_utt(a), _utt(), _utt(b)])
    with pytest.raises(ValueError, match='utterance 0 carries no Sampling'):
        S.of_utterances('e', [_utt(None), _utt(a)])
    with pytest.raises(ValueError, match='utterance 0 has 5 elements'):
        S.of_utterances('e', [_utt() + (a, a)])
    with pytest.raises(ValueError, match='not a valle2_amd.Sampling'):
        S.of_utterances('e', [_utt(dict(seed=1))])


def test_entry_points_refuse_before_any_device_work():
    """A CPU model: anything that went on to the device would raise VhError (no device) or copy the model there."""
    from valle2_amd import Sampling
    m = _cpu_model()
    a = Sampling(1)
    texts, firsts = [torch.arange(5)] * 2, [torch.arange(7)] * 2
    with pytest.raises(ValueError, match=r'generate_many: utterance 1 carries no Sampling'):
        m.generate_many([_utt(a), _utt()])
    with pytest.raises(ValueError, match=r'generate_queued: utterance 2 carries no Sampling'):
        m.generate_queued([_utt(a), _utt(a), _utt(None)], beams=2)
    with pytest.raises(ValueError, match=r'generate_batch: utterance 1 carries no Sampling'):
        m.generate_batch(texts, firsts, sampling=[a, None])
    with pytest.raises(ValueError, match=r'generate_batch: sampling holds 1 entries for 2 utterances'):
        m.generate_batch(texts, firsts, beams=2, sampling=[a])
    with pytest.raises(ValueError, match=r'generate_batch: sampling with forced'):
        m.generate_batch(texts, firsts, forced=torch.zeros(8, dtype=torch.int64), sampling=[a, a])
    with pytest.raises(ValueError, match=r'generate: sampling is int, not a valle2_amd.Sampling'):
        m.generate(*_utt(), sampling=5)


def test_signatures_gain_only_keyword_arguments():
    import inspect
    from valle2_amd.valle_ar import ValleAR
    for fn in (ValleAR.generate, ValleAR.generate_batch):
        p = inspect.signature(fn).parameters['sampling']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(ValleAR.generate_many).parameters) == ['self', 'utterances', 'beams']
    assert list(inspect.signature(ValleAR.generate_queued).parameters) == ['self', 'utterances', 'beams', 'slots']


def test_codec_io_hands_the_fourth_element_to_the_ar_model_only(monkeypatch):
    from valle2_amd import ConfigValle, Sampling, codec_io as CIO, get_model_class
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=2)
    ar = get_model_class('ValleAR')(cfg)
    seen = {}

    class Nar:
        def generate_batch(self, texts, prompts, firsts, greedy=False):
            seen['nar'] = (len(texts), len(prompts), len(firsts))
            return [torch.zeros(3, cfg.num_quantizers, dtype=torch.int64)] * len(texts)

    def ar_many(utts, **kw):
        seen['ar'] = [u[3:] for u in utts]
        return [torch.arange(3)] * len(utts)
    monkeypatch.setattr(ar, 'generate_many', ar_many)
    monkeypatch.setattr(ar, 'generate_queued', ar_many)
    a, b = Sampling(1), Sampling(2, top_k=8)
    item = (torch.arange(4), torch.zeros(cfg.num_quantizers, 5, dtype=torch.int64), torch.arange(3))
    for fn in (CIO.synthesize_many, CIO.synthesize_queued):
        assert len(fn(ar, Nar(), [item + (a,), item + (b,)])) == 2
        assert seen['ar'] == [(a,), (b,)] and seen['nar'] == (2, 2, 2)
        assert len(fn(ar, Nar(), [item, item])) == 2 and seen['ar'] == [(), ()]


# ---- 2. the mirror as the sampler -----------------------------------------------------------------------------------------
def test_uniform01_is_the_kernels_generator():
    """splitmix64's finaliser over seed + GOLDEN * ((key << 32) | (pos + 1)), top 24 bits: values worked out by hand from the
    definition (seed 0, key 0, pos 0 is the first output of splitmix64 seeded with 0: 0xE220A8397B1DCDAF)."""
    assert SR.uniform01(0, 0, 0) == (0xE220A8397B1DCDAF >> 40) / 2 ** 24
    assert SR.uniform01(2 ** 64 - 1, 0, 0) != SR.uniform01(0, 0, 0)
    seen = {SR.uniform01(s, k, p) for s in (1, 2 ** 63) for k in range(4) for p in range(60, 70)}
    assert len(seen) == 80 and all(0.0 <= u < 1.0 for u in seen)


def test_mirror_step_walks_the_kept_set_in_index_order_and_flags_what_a_small_error_could_move():
    logits = [0.0, 3.0, 1.0, 2.0, -5.0]                    # top 3: tokens 1, 3, 2; kept in index order: 1, 2, 3
    e = torch.tensor([3.0, 1.0, 2.0]).exp()
    c = (e.cumsum(0) / e.sum()).tolist()
    for u, want in ((0.0, 1), (c[0] - 1e-3, 1), (c[0] + 1e-3, 2), (c[1] - 1e-3, 2), (c[1] + 1e-3, 3), (0.999999, 3)):
        assert SR.mirror_step(logits, 3, 1.0, u, 1e-4) == (want, False, {want})
    tok, amb, cands = SR.mirror_step(logits, 3, 1.0, c[0] + 1e-4, 1e-4)
    assert (tok, amb, cands) == (2, True, {1, 2})         # within 2 delta of the first boundary
    assert SR.mirror_step(logits, 3, 0.5, c[0] + 3e-4, 1e-4)[1] is False      # (another temperature: other boundaries)
    # the threshold: token 0 a hair under token 2 may take its place in the kept set
    tok, amb, cands = SR.mirror_step([1.0 - 1e-4, 3.0, 1.0, 2.0, -5.0], 3, 1.0, 0.5, 1e-4)
    assert amb is True and tok in cands
    assert SR.mirror_step(logits, 1, 1.0, 0.7, 1e-4) == (1, False, {1})       # top_k 1: the arg-max
    assert SR.mirror_step([2.0, 5.0, 5.0], 1, 1.0, 0.7, 1e-4)[0] == 1         # ... the lowest index on ties


@pytest.fixture(scope='module')
def d128():
    kw, sd, utts = R.audit_inputs('d128')
    return GC.cfg_of(kw), sd, utts


@pytest.mark.parametrize('u', range(5))
def test_mirror_decodes_the_audit_model_within_the_cap(d128, u):
    """The oracle's own replayed decode under the seeds and filters of the GPU cases: its rows pass audit_sampled_rows and at
    most AMBIGUOUS_CAP of its steps are ambiguous (a device that agrees with the oracle to AUDIT_DELTA follows the same
    histories except at those steps)."""
    cfg, sd, utts = d128
    pt, pc, tt = utts[u]
    text, s = torch.cat([pt, tt]), SR.replay_request(u)
    rows, scores, counted, ambiguous = SR.mirror_decode(sd, cfg, text, pc[:, 0], SR.REPLAY_BEAMS, R.AUDIT_MAX_NEW, s.seed, s.top_k,
                                                        s.temperature)
    report = R.audit_sampled_rows(sd, cfg, text, rows, scores, pc.shape[0] + 1, R.AUDIT_MAX_NEW, s.top_k, 1.0, s.temperature,
                                  R.AUDIT_DELTA)
    print(f'utterance {u} (top_k {s.top_k}, temperature {s.temperature}): {counted} counted steps, {ambiguous} ambiguous '
          f'({ambiguous / counted:.3f}), rows end {[(r["steps"], r["end"]) for r in report]}')
    assert counted == sum(r['steps'] for r in report) >= R.AUDIT_MAX_NEW
    assert ambiguous <= SR.AMBIGUOUS_CAP * counted
    assert len({tuple(r.tolist()) for r in rows}) == SR.REPLAY_BEAMS, 'beams of one seed must draw different tokens'
    # the replay of its own rows agrees with itself, and a row replayed under another key does not
    assert SR.replay_rows(sd, cfg, text, rows, pc.shape[0] + 1, R.AUDIT_MAX_NEW, s.seed, s.top_k, s.temperature) == (counted, ambiguous)
    with pytest.raises(SR.ReplayError):
        SR.replay_rows(sd, cfg, text, rows, pc.shape[0] + 1, R.AUDIT_MAX_NEW, s.seed, s.top_k, s.temperature, keys=[1, 2, 3, 0])
    with pytest.raises(SR.ReplayError):
        SR.replay_rows(sd, cfg, text, rows, pc.shape[0] + 1, R.AUDIT_MAX_NEW, s.seed + 1, s.top_k, s.temperature)


# ---- 3. the plan, the slot key, the header, the library ----------------------------------------------------------------------
def test_plan_and_slot_key_tell_row_sampling_from_call_sampling():
    from valle2_amd import ConfigValle, generation as G
    cfg = ConfigValle(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm', num_beams=3,
                      top_k=50, max_audio_len=40)
    for kw in ({}, dict(beams=3), dict(beams=3, queued=True, cap=256)):
        call = G.plan_decode(cfg, [9, 12], [18, 62], max_new=40, **kw)
        rows = G.plan_decode(cfg, [9, 12], [18, 62], max_new=40, row_sampling=True, **kw)
        assert call.row_sampling is False and rows.row_sampling is True
        for f in ('kind', 'B', 'prefix_spec', 'rows_spec', 'codes_width', 'cache_len0', 'slot_eligible'):
            assert getattr(call, f) == getattr(rows, f)
        assert G.slot_key(call, cfg, 'cuda:0', ()) != G.slot_key(rows, cfg, 'cuda:0', ())
        assert G.slot_key(rows, cfg, 'cuda:0', ()) == G.slot_key(rows, cfg, 'cuda:0', ())


def test_header_declares_library_exports_and_signatures_bind(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    struct = re.search(r'typedef struct \{([^}]*)\} vh_row_sampling;', header)
    assert struct and [f.split()[-1] for f in struct.group(1).split(';') if f.strip()] == \
        ['seed', 'key', 'top_k', 'top_p', 'temperature', 'reserved[2]']
    for name in ('vh_sample_step_rows', 'vh_sample_step_wide_rows'):
        assert re.search(r'\bint %s\(' % name, header) and name in _lib.SIGNATURES and getattr(L, name) is not None
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r'const vh_row_sampling \*row_sampling;\s*\} vh_ar_decoder_desc;', header), 'the trailing field of the descriptor'
    assert _lib.VhArDecoderDesc._fields_[-1][0] == 'row_sampling'
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 135
    text = (REPO / 'INTEGRATION.md').read_text()
    assert 'ABI 134' in text and 'ABI 135' in text


def test_record_layout_is_the_headers():
    from valle2_amd import kernels
    S = _lib.VhRowSampling
    assert C.sizeof(S) == kernels.ROW_SAMPLING_BYTES == 32
    assert [(getattr(S, n).offset) for n in ('seed', 'key', 'top_k', 'top_p', 'temperature', 'reserved')] == [0, 8, 12, 16, 20, 24]
    packed = kernels.pack_row_sampling([(2 ** 64 - 1, 3, 50, 1.0, 0.8), (5, 0, 0, 0.9, 1.25)])
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (2, 32)
    recs = (S * 2).from_buffer_copy(packed.numpy().tobytes())
    assert (recs[0].seed, recs[0].key, recs[0].top_k, recs[0].top_p) == (2 ** 64 - 1, 3, 50, 1.0)
    assert recs[0].temperature == C.c_float(0.8).value and list(recs[0].reserved) == [0, 0]
    assert (recs[1].seed, recs[1].key, recs[1].top_k, recs[1].temperature) == (5, 0, 0, 1.25) and recs[1].top_p == C.c_float(0.9).value


@pytest.mark.parametrize('name,max_v', [('vh_sample_step_rows', 2048), ('vh_sample_step_wide_rows', 16384)])
def test_rows_entry_points_refuse_before_any_gpu_work(L, name, max_v):
    def call(logits=P, V=1025, rs=P2, codes=P, x_next=P, B=4, d=128):
        return getattr(L, name)(logits, V + 3, V, V - 1, rs, codes, 80, I32, None, P, P, P, I32, I32, x_next, B, d, None)
    for kw, text in ((dict(rs=None), 'null sampling records'), (dict(rs=P2 + 8), 'records must be 16-byte aligned'),
                     (dict(logits=None), 'null pointer'), (dict(V=max_v + 1), f'(<= {max_v})'), (dict(B=0), 'bad dims'),
                     (dict(x_next=P + 4), '16-byte aligned')):
        assert call(**kw) < 0 and text in _err(L), (kw, _err(L))


# ---- 4. the decoder's descriptor ---------------------------------------------------------------------------------------------
def _desc(L, **kw):
    layers = (_lib.VhLayer * 2)()
    for lay in layers:
        lay.wqkv_f = lay.qkv_c1 = lay.qkv_c2 = P
    d = _lib.VhArDecoderDesc(B=12, d_model=128, n_heads=2, dff=256, n_layers=2, S_max=64, V=1025, eos=1024, n_split=1,
                             ln_eps=1e-5, layers=layers, proj_w=P, audio_emb=P, audio_pe=P, x=P, q=P, attn=P, hidden=P,
                             logits=P, cache_len=I32, audio_pos=I32, eos_count=I32, codes=P, codes_stride=80, top_k=50,
                             temperature=1.0, sum_logprobs=P, row_sampling=P2)
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = layers
    return d


def _create(L, d):
    h = L.vh_ar_decoder_create(C.byref(d))
    if h:
        L.vh_ar_decoder_destroy(h)
    return bool(h)


def test_decoder_takes_row_sampling_and_refuses_it_with_the_fused_greedy_head(L):
    assert _create(L, _desc(L)), _err(L)
    assert _create(L, _desc(L, row_sampling=None)), _err(L)                                  # NULL: today's forms
    # the records replace the scalar filter: a greedy config, or no temperature at all, samples per row all the same
    assert _create(L, _desc(L, top_k=1)), _err(L)
    assert _create(L, _desc(L, temperature=0.0)), _err(L)
    assert not _create(L, _desc(L, row_sampling=None, temperature=0.0)) and 'temperature > 0' in _err(L)
    ws = L.vh_head_greedy_ws_bytes(12, 1025)
    assert _create(L, _desc(L, top_k=1, row_sampling=None, head_ws=P, head_ws_bytes=ws)), _err(L)
    assert not _create(L, _desc(L, top_k=1, head_ws=P, head_ws_bytes=ws))
    assert 'row_sampling' in _err(L) and 'head_ws' in _err(L), _err(L)
    assert not _create(L, _desc(L, row_sampling=P2 + 8)) and 'row_sampling must be 16-byte aligned' in _err(L), _err(L)
    # a vocabulary beyond the wide sampler is refused whatever top_k says
    assert not _create(L, _desc(L, top_k=1, V=16385)) and 'row_sampling' in _err(L) and 'VH_SAMPLE_MAX_V' in _err(L), _err(L)
    assert _create(L, _desc(L, top_k=1, V=16385, row_sampling=None)), _err(L)
