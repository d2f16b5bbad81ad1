"""Per-request length bounds (valle2_amd.Bounded: min_new and max_new per utterance), the parts that need no GPU: Bounded's
ranges and what the entry points refuse before any device work, the layout of vh_row_limits, the C ABI (the two `_bounded`
sample entries and vh_ar_decoder_set_row_limits, through ctypes with made-up, aligned pointers: nothing is dereferenced), the
float64 mirror (tests/bounds_replay.py) on hand-worked rows, and the mirror's own decode of the GPU file's model cases."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bounds_replay as BR
from tests import oracle_runners as R
from tests import sampling_replay as SR
from tests.golden import cases as GC
from valle2_amd import Bounded, RepetitionAware, Sampling, _lib, kernels
from valle2_amd import sampling as S

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / 'include' / 'valle_hip.h').read_text()
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": 16-byte aligned, never dereferenced


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


# ---- 1. Bounded and the entry points, on a CPU model -------------------------------------------------------------------------
def test_bounded_is_exported_wraps_both_classes_and_delegates():
    import valle2_amd
    assert 'Bounded' in valle2_amd.__all__
    cfg = GC.cfg_of(dict(GC.AR_TINY, top_k=50, tok_p=1.0, temperature=1.0))
    plain, ras = Sampling(7, top_k=8, temperature=0.8), RepetitionAware(9, top_k=8, window=4, max_repeats=1)
    for inner in (plain, ras):
        b = Bounded(inner, min_new=3, max_new=11)
        assert b.request is inner and (b.seed, b.top_k) == (inner.seed, 8)
        assert b.resolved(cfg) == inner.resolved(cfg) and b.records(cfg, 3, 2) == inner.records(cfg, 3, 2)
        assert b.nar_record(cfg) == inner.nar_record(cfg)
        assert b.limits(3) == [(3, 11)] * 3
    assert Bounded(plain).limits(2) == [(0, 0)] * 2 and Bounded(plain, min_new=0, max_new=None).limits(1) == [(0, 0)]
    assert Bounded(plain, max_new=5).limits(1) == [(0, 5)] and Bounded(plain, min_new=5).limits(1) == [(5, 0)]
    with pytest.raises(Exception):
        Bounded(plain, min_new=1).min_new = 2                     # frozen
    # the pinned field lists of the two classes did not grow
    assert [f for f in Sampling.__dataclass_fields__] == ['seed', 'top_k', 'tok_p', 'temperature']
    assert [f for f in RepetitionAware.__dataclass_fields__][4:] == ['window', 'max_repeats']
    assert S.repetition_aware([Bounded(ras, max_new=3)]) and not S.repetition_aware([Bounded(plain, max_new=3)])
    assert S.bounded([plain, Bounded(ras, min_new=1)]) and not S.bounded([plain, Bounded(plain)]) and not S.bounded(None)
    assert S.row_limits([plain, Bounded(ras, min_new=1, max_new=4)], 2) == [(0, 0), (0, 0), (1, 4), (1, 4)]
    rows = S.beam_rows(Bounded(plain, min_new=2), 3)
    assert [r.records(cfg, 1) for r in rows] == [[rec] for rec in plain.records(cfg, 3)]
    assert S.row_limits(rows, 1) == [(2, 0)] * 3 and S.bounded(rows)


@pytest.mark.parametrize('kw,text', [
    (dict(min_new=-1), 'min_new=-1'), (dict(max_new=2 ** 31), 'max_new=2147483648'), (dict(min_new=1.5), 'min_new=1.5'),
    (dict(max_new=True), 'max_new=True'), (dict(max_new=0), 'max_new=0'), (dict(min_new=6, max_new=5), 'min_new=6 exceeds max_new=5')])
def test_bounded_refuses_what_is_out_of_range(kw, text):
    with pytest.raises(ValueError, match=re.escape(text)):
        Bounded(Sampling(1), **kw)


def test_bounded_refuses_what_is_not_a_sampling():
    with pytest.raises(ValueError, match='request is int'):
        Bounded(5, max_new=3)
    with pytest.raises(ValueError, match='request is Bounded'):
        Bounded(Bounded(Sampling(1)), max_new=3)


def test_every_entry_point_accepts_or_refuses_it_before_any_device_work():
    from valle2_amd import get_model_class, synth
    cfg = GC.cfg_of(dict(GC.AR_TINY, max_audio_len=30, top_k=50, tok_p=1.0, temperature=1.0))
    m = get_model_class('ValleAR')(cfg)                              # on the CPU: anything past the early checks needs a device
    utt = synth.synth_utterance(cfg, 4, 3, 6, seed=1)
    text, first = torch.cat([utt[0], utt[2]]), utt[1][:, 0]
    too_long = Bounded(Sampling(1), min_new=31)
    fine = Bounded(Sampling(1), min_new=30, max_new=10 ** 6)          # a max_new above the cap is allowed
    with pytest.raises(ValueError, match="generate: Bounded min_new=31 exceeds the call's cap of 30"):
        m.generate(*utt, sampling=too_long)
    with pytest.raises(ValueError, match="generate_batch: Bounded min_new=31 exceeds the call's cap of 30"):
        m.generate_batch([text], [first], sampling=[too_long])
    with pytest.raises(ValueError, match="generate_batch: Bounded min_new=30 exceeds the call's cap of 12"):
        m.generate_batch([text], [first], max_new=12, sampling=[fine])
    with pytest.raises(ValueError, match='generate_many: Bounded min_new=31'):
        m.generate_many([utt + (too_long,)])
    with pytest.raises(ValueError, match='generate_queued: Bounded min_new=31'):
        m.generate_queued([utt + (too_long,)], beams=1)
    with pytest.raises(ValueError, match='carries no Sampling and others do'):
        m.generate_many([utt + (fine,), utt])
    with pytest.raises(ValueError, match='greedy'):                   # the wrapped request meets the config as ever
        get_model_class('ValleAR')(GC.cfg_of(dict(GC.AR_TINY, top_k=1))).generate(*utt, sampling=Bounded(RepetitionAware(1), max_new=4))
    # accepted: the early checks pass and return the list (mixed with plain and RepetitionAware requests)
    mixed = [fine, Sampling(2), Bounded(RepetitionAware(3, top_k=8), max_new=5)]
    assert S.check_list('generate_batch', mixed, 3, cfg=cfg) == mixed
    assert S.of_utterances('generate_queued', [utt + (r,) for r in mixed], cfg) == mixed
    from valle2_amd import generation
    assert generation.check_sampling(mixed, 3, None, cfg, 30) == mixed


def test_the_synthesis_entries_and_the_nar_stage_take_it():
    from valle2_amd import codec_io, get_model_class
    cfg = GC.cfg_of(dict(GC.AR_TINY))
    b = Bounded(Sampling(4, temperature=0.7), min_new=2)
    assert b.nar_record(cfg) == Sampling(4, temperature=0.7).nar_record(cfg)      # the NAR stage ignores the bounds
    with pytest.raises(ValueError, match='item 1 carries no valle2_amd.Sampling'):
        codec_io.synthesize_requests(None, None, [(None, None, None, b), (None, None, None, 3)])
    ncfg = GC.cfg_of(dict(GC.AR_TINY, norm='AdaptiveLayerNorm'))
    nar = get_model_class('ValleNAR')(ncfg)
    with pytest.raises(ValueError, match='sampling together with seed='):          # past the type check: a Bounded is a request
        nar.generate_batch([torch.zeros(3, dtype=torch.int64)], [torch.zeros(4, 8, dtype=torch.int64)],
                           [torch.zeros(5, dtype=torch.int64)], seed=1, sampling=[b])


# ---- 2. the records and the C ABI ----------------------------------------------------------------------------------------------
def test_row_limits_layout_and_version(L):
    T = _lib.VhRowLimits
    assert C.sizeof(T) == kernels.ROW_LIMITS_BYTES == 8 and [T.min_new.offset, T.max_new.offset] == [0, 4]
    assert C.sizeof(_lib.VhRowSampling) == 32 and _lib.VhArDecoderDesc._fields_[-1][0] == 'row_sampling'
    packed = kernels.pack_row_limits([(3, 0), (0, 2 ** 31 - 1), (258, 65536)])
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, 8)
    assert packed.numpy().tobytes() == b''.join(int(v).to_bytes(4, 'little') for v in (3, 0, 0, 2 ** 31 - 1, 258, 65536))
    recs = (T * 3).from_buffer_copy(packed.numpy().tobytes())
    assert [(r.min_new, r.max_new) for r in recs] == [(3, 0), (0, 2 ** 31 - 1), (258, 65536)]
    for bad in ([(1,)], [(-1, 0)], [(0, 2 ** 31)], [(1.0, 2)]):
        with pytest.raises(ValueError, match='pack_row_limits: record 0'):
            kernels.pack_row_limits(bad)
    declared = int(re.search(r'#define VH_VERSION (\d+)', HEADER).group(1))
    assert L.vh_version() == declared >= 142
    for name in ('vh_sample_step_rows_bounded', 'vh_sample_step_wide_rows_bounded', 'vh_ar_decoder_set_row_limits'):
        assert hasattr(L, name) and name in HEADER
    comment = HEADER[HEADER.index('PER-ROW LENGTH BOUNDS'):HEADER.index('} vh_row_limits;')]
    for text in ('min_new', 'max_new', 'FORCED', 'OUTSIDE THE SUPPORT', 'sum_logprobs[b] is unchanged', '-inf', '0x40000000', 'finished row'):
        assert text in comment, f'the comment above vh_row_limits does not say {text!r}'
    assert 'ABI 142' in (REPO / 'INTEGRATION.md').read_text()


@pytest.mark.parametrize('name,max_v', [('vh_sample_step_rows_bounded', 2048), ('vh_sample_step_wide_rows_bounded', 16384)])
def test_bounded_entry_points_refuse_before_any_gpu_work(L, name, max_v):
    def call(logits=P, V=1025, rs=P2, limits=P2 + 64, pos_base=I32, B=4):
        return getattr(L, name)(logits, V + 3, V, V - 1, rs, limits, P, 80, I32, pos_base, P, P, P, I32, I32, P, B, 128, None)
    for kw, code, text in ((dict(rs=None), -1, 'null sampling records'), (dict(pos_base=None), -1, 'limits need pos_base'),
                           (dict(V=1), -1, 'limits need V >= 2'), (dict(limits=P2 + 68), -2, 'limits (vh_row_limits records) must be 8-byte aligned'),
                           (dict(logits=None), -1, 'null pointer'), (dict(V=max_v + 1), -1, f'(<= {max_v})'), (dict(B=0), -1, 'bad dims')):
        assert call(**kw) == code and text in _err(L), (kw, _err(L))
    assert name in _err(L) or 'vh_sample_step' in _err(L)


def _desc(**kw):
    layers = (_lib.VhLayer * 2)()
    for lay in layers:
        lay.wqkv_f = lay.qkv_c1 = lay.qkv_c2 = P
    d = _lib.VhArDecoderDesc(B=12, d_model=128, n_heads=2, dff=256, n_layers=2, S_max=64, V=1025, eos=1024, n_split=1,
                             ln_eps=1e-5, layers=layers, proj_w=P, audio_emb=P, audio_pe=P, x=P, q=P, attn=P, hidden=P,
                             logits=P, cache_len=I32, audio_pos=I32, eos_count=I32, pos_base=I32, codes=P, codes_stride=80,
                             top_k=50, temperature=1.0, sum_logprobs=P, row_sampling=P2)
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = layers
    return d


def test_the_decoder_takes_and_refuses_row_limits(L):
    def attempt(limits, **kw):
        d = _desc(**kw)
        h = L.vh_ar_decoder_create(C.byref(d))
        assert h, _err(L)
        try:
            return L.vh_ar_decoder_set_row_limits(h, limits)
        finally:
            L.vh_ar_decoder_destroy(h)
    assert attempt(P2 + 64) == 0 and attempt(None) == 0              # attach, clear
    assert attempt(P2 + 64, row_sampling=None) == -1 and 'without row_sampling' in _err(L)
    assert attempt(P2 + 64, pos_base=None) == -1 and 'without pos_base' in _err(L)
    assert attempt(P2 + 68) == -2 and '8-byte aligned' in _err(L)
    assert attempt(P2 + 64, V=1, eos=0) == -1 and 'V >= 2' in _err(L)
    assert L.vh_ar_decoder_set_row_limits(None, P2) == -1 and 'null decoder' in _err(L)
    # the fused greedy head reads no limits: no decoder with row_sampling has it, so the setter never meets one
    d = _desc(top_k=1, head_ws=P, head_ws_bytes=L.vh_head_greedy_ws_bytes(12, 1025))
    assert not L.vh_ar_decoder_create(C.byref(d)) and 'row_sampling with head_ws' in _err(L)
    assert attempt(P2 + 64, top_k=1, row_sampling=None, head_ws=P, head_ws_bytes=L.vh_head_greedy_ws_bytes(12, 1025)) == -1
    assert 'without row_sampling' in _err(L)
    # (after vh_ar_decoder_capture: VH_ESTATE — capture needs a device, tests/test_length_bounds_gpu.py)


# ---- 3. the mirror on hand-worked rows -----------------------------------------------------------------------------------------
V, EOS, BOS = 9, 8, 9


class _Req:
    def __init__(self, seed=3, top_k=0, tok_p=1.0, temperature=1.0, **ras):
        self.seed, self.top_k, self.tok_p, self.temperature = seed, top_k, tok_p, temperature
        self.__dict__.update(ras)


def test_the_four_cases_in_their_order():
    hist = [BOS, 1, 2, 3, 4, 5]
    assert BR.state(hist, 3, 3, 0, 0, EOS) == BR.FREE
    assert BR.state(hist, 3, 3, 1, 0, EOS) == BR.SUPPRESSED and BR.state(hist, 4, 3, 1, 0, EOS) == BR.FREE
    assert BR.state(hist, 5, 3, 0, 2, EOS) == BR.FORCED and BR.state(hist, 4, 3, 0, 2, EOS) == BR.FREE
    assert BR.state(hist, 5, 3, 9, 2, EOS) == BR.FORCED            # min_new > max_new behaves as its max_new
    assert BR.state([BOS, 1, EOS], 3, 1, 9, 1, EOS) == BR.FINISHED  # a finished row reads neither word


def test_a_dominant_eos_is_drawn_unless_suppressed_and_forced_without_a_score():
    x = np.zeros(V)
    x[EOS], x[2] = 30.0, 5.0                                        # EOS carries all the mass; token 2 all that is left without it
    hist = [BOS, 1, 1, 1]
    for req in (_Req(top_k=0), _Req(top_k=3), _Req(top_k=1), _Req(top_k=0, tok_p=0.9), _Req(top_k=2, window=10, max_repeats=0)):
        tok, case, _, amb, cands, lp = BR.mirror_step_bounded(x, hist, req, 0, 4, 1, 1e-6, EOS, limits=(0, 0))
        assert (tok, case) == (EOS, BR.FREE) and abs(lp) < 1e-9
        tok, case, _, amb, cands, lp = BR.mirror_step_bounded(x, hist, req, 0, 4, 1, 1e-6, EOS, limits=(4, 0))
        assert (tok, case) == (2, BR.SUPPRESSED) and EOS not in cands
        if req.top_k != 1:
            # without EOS token 2 holds e^5 / (e^5 + 7) = 0.955: any top_k keeps the seven ties at 0 beside it, tok_p 0.9
            # drops them (0.045 <= 0.1) and leaves token 2 alone
            want = 0.0 if req.tok_p < 1 else 5.0 - np.log(np.exp(5.0) + 7.0)
            assert abs(lp - want) < 1e-9, (req.__dict__, lp, want)
        else:
            assert lp == 0.0
        tok, case, re_, amb, cands, lp = BR.mirror_step_bounded(x, hist, req, 0, 4, 1, 1e-6, EOS, limits=(9, 3))
        assert (tok, case, re_, amb, cands, lp) == (EOS, BR.FORCED, False, False, {EOS}, None)
    # the redraw under suppression: token 1 fills the history, the redraw over all V entries cannot return EOS either
    x[1] = 6.0
    req = _Req(top_k=1 + 1, window=10, max_repeats=0)
    drew = set()
    for seed in range(40):
        req.seed = seed
        tok, case, re_, _, cands, _ = BR.mirror_step_bounded(x, hist, req, 0, 4, 1, 1e-6, EOS, limits=(4, 0))
        assert tok != EOS and EOS not in cands
        drew.add((tok, re_))
    assert any(re_ for _, re_ in drew), 'no seed redrew'


def test_top_p_cut_keeps_the_largest_and_drops_from_the_smallest():
    x = np.log(np.array([0.5, 0.3, 0.15, 0.05]))
    kept, alts = BR._kept_top_p(x, 0, 0.9, 1e-9)
    assert kept == [0, 1, 2] and not alts                            # dropping 0.05 is <= 0.1; dropping 0.15 more is not
    kept, _ = BR._kept_top_p(x, 0, 0.4, 1e-9)
    assert kept == [0]
    kept, alts = BR._kept_top_p(x, 0, 0.95, 1e-3)                    # the suffix 0.05 sits on 1 - tok_p: ambiguous
    assert alts


# ---- 4. the model cases of the GPU file: the mirror's own decode ---------------------------------------------------------------
def test_the_mirrors_own_decode_of_the_model_cases_stays_within_the_cap_and_the_bounds():
    kw, sd, utts = R.audit_inputs('d128')
    cfg = GC.cfg_of(kw)
    eos = cfg.num_audio_tokens
    total_forced = 0
    for u in range(4):
        req = BR.bounds_request(u)
        text, first = torch.cat([utts[u][0], utts[u][2]]), utts[u][1][:, 0]
        rows, scores, counted, ambiguous, _, forced = BR.mirror_decode(sd, cfg, text, first, BR.BOUNDS_BEAMS, R.AUDIT_MAX_NEW, req)
        print(f'utterance {u}: {counted} counted, {ambiguous} ambiguous, {forced} forced, scores {scores.tolist()}')
        assert ambiguous <= SR.AMBIGUOUS_CAP * counted, f'utterance {u}: {ambiguous} of {counted} steps ambiguous'
        lo, hi = BR.limits_of(req)
        for r in rows:
            gen = r[len(first) + 1:].tolist()
            n = next((i for i, t in enumerate(gen) if t == eos), len(gen))
            assert n >= lo and (hi == 0 or n <= hi)
        total_forced += forced
        # the replay of the mirror's own rows agrees with itself
        assert BR.replay_rows(sd, cfg, text, rows, len(first) + 1, R.AUDIT_MAX_NEW, req)[0] == counted
    assert total_forced > 0
