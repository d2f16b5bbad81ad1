"""Queued decoding (ValleAR.generate_queued: a finished utterance hands its rows to a waiting one), the parts that need no
GPU: the signatures, the three C entry points exported at ABI 134 and what they refuse BEFORE any GPU work (called through
ctypes with made-up, aligned pointers: nothing is dereferenced on a refusal), the schedule (engine.plan_queue) on hand-made
lengths, and generate_queued's pure-Python refusals on a CPU model."""
import inspect
import re
from pathlib import Path

import pytest
import torch

from valle2_amd import _lib

REPO = Path(__file__).resolve().parent.parent
P, P2, I32 = 0x10000, 0x20000, 0x30000            # "device pointers": aligned, never dereferenced (every call is refused)
POLL = 32


@pytest.fixture(scope='module')
def L():
    return _lib.load_library()


def _err(L):
    return (L.vh_last_error() or b'').decode()


# ---- signatures and exports -------------------------------------------------------------------------------------------------
def test_signatures():
    from valle2_amd import codec_io, engine
    from valle2_amd.valle_ar import ValleAR
    p = inspect.signature(ValleAR.generate_queued).parameters
    assert list(p) == ['self', 'utterances', 'beams', 'slots']
    for name in ('beams', 'slots'):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(codec_io.synthesize_queued).parameters
    assert list(p) == ['ar', 'nar', 'items', 'codec', 'greedy_nar', 'slots']
    assert p['slots'].kind is inspect.Parameter.KEYWORD_ONLY and p['slots'].default is None and p['greedy_nar'].default is False
    assert list(inspect.signature(engine.plan_queue).parameters) == ['lengths', 'slots', 'poll', 'max_new']
    assert callable(engine.KVCache.group_view)


def test_header_declares_and_library_exports_the_entry_points(L):
    header = (REPO / 'include' / 'valle_hip.h').read_text()
    for name in ('vh_decode_groups_poll', 'vh_decode_group_reset', 'vh_attn_decode_shared_groups'):
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.vh_version() == int(re.search(r'#define VH_VERSION (\d+)', header).group(1)) >= 134
    assert 'ABI 134' in (REPO / 'INTEGRATION.md').read_text()


# ---- the schedule -----------------------------------------------------------------------------------------------------------
LISTS = [
    ([40, 200, 40, 40, 200, 40], 2, 10 ** 6),
    ([40, 200, 40, 40, 200, 40], 3, 96),
    ([1, 2, 33, 34, 65, 96, 97, 500], 3, 96),
    ([5], 1, 96), ([5, 400], 4, 96), ([33] * 7, 2, 64), ([1000, 1, 1, 1, 1, 1, 1], 2, 10 ** 6),
]


@pytest.mark.parametrize('lengths,slots,max_new', LISTS)
def test_plan_queue_gives_every_utterance_one_interval_on_poll_boundaries(lengths, slots, max_new):
    from valle2_amd import engine
    iv, total = engine.plan_queue(lengths, slots, POLL, max_new)
    assert len(iv) == len(lengths)                                           # exactly one (slot, start, end) each
    used = min(slots, len(lengths))
    for u, (slot, start, end) in enumerate(iv):
        assert 0 <= slot < used and isinstance(start, int) and isinstance(end, int) and 0 <= start < end
        # held for the polls its length needs: the first token comes with the prompt pass, the rest in blocks of POLL
        n = min(lengths[u], max_new)
        assert end - start == max(1, -(-(n - 1) // POLL)) == engine.queue_polls(lengths[u], POLL, max_new)
    for a in range(len(iv)):                                                 # no slot holds two at once
        for b in range(a + 1, len(iv)):
            if iv[a][0] == iv[b][0]:
                assert iv[a][2] <= iv[b][1] or iv[b][2] <= iv[a][1], (iv[a], iv[b])
    assert total == POLL * max(e for _, _, e in iv) and total % POLL == 0    # steps are whole polls up to the latest end
    # utterances are handed out in input order: starts never decrease
    assert [s for _, s, _ in iv] == sorted(s for _, s, _ in iv)
    assert total <= engine.chunk_schedule_steps(lengths, used, POLL, max_new)


@pytest.mark.parametrize('lengths,max_new', [([40, 200, 40], 96), ([7, 64, 65, 66], 10 ** 6), ([1], 96), ([300] * 5, 256)])
def test_plan_queue_is_the_chunk_schedule_when_everything_fits(lengths, max_new):
    from valle2_amd import engine
    for slots in (len(lengths), len(lengths) + 3):
        iv, total = engine.plan_queue(lengths, slots, POLL, max_new)
        assert [(s, st) for s, st, _ in iv] == [(i, 0) for i in range(len(lengths))]
        assert total == engine.chunk_schedule_steps(lengths, len(lengths), POLL, max_new)
        # generate_many's loop: blocks of POLL from step 1 until every row has finished or max_new is reached
        done, longest = 1, min(max(lengths), max_new)
        while done < longest:
            done += POLL
        assert total == max(POLL, done - 1)


def test_plan_queue_beats_three_chunks_of_two():
    from valle2_amd import engine
    lengths = [40, 200, 40, 40, 200, 40]
    iv, total = engine.plan_queue(lengths, 2, POLL, 10 ** 6)
    chunk_maxima = sum(POLL * engine.queue_polls(max(lengths[i:i + 2]), POLL, 10 ** 6) for i in range(0, 6, 2))
    assert chunk_maxima == engine.chunk_schedule_steps(lengths, 2, POLL, 10 ** 6) == (7 + 2 + 7) * POLL
    assert total < chunk_maxima and total == 13 * POLL
    assert iv == [(0, 0, 2), (1, 0, 7), (0, 2, 4), (0, 4, 6), (0, 6, 13), (1, 7, 9)]


def test_queue_schedule_refills_in_slot_order_and_parks_when_nothing_waits():
    from valle2_amd import engine
    s = engine.QueueSchedule(4, 2)
    assert s.holder == [0, 1] and not s.finished
    assert s.retire(1, 1) == 2 and s.retire(0, 3) == 3 and s.refills == 2
    assert s.retire(1, 4) is None and s.holder == [3, None] and not s.finished
    with pytest.raises(ValueError):
        s.retire(1, 5)
    assert s.retire(0, 6) is None and s.finished
    assert s.intervals() == [(0, 0, 3), (1, 0, 1), (1, 1, 4), (0, 3, 6)]
    assert engine.queue_steps_cap(96, POLL) == 96 and engine.queue_steps_cap(97, POLL) == 128 and engine.queue_steps_cap(1, POLL) == 32


# ---- generate_queued: the pure-Python refusals, on a CPU model with no device in sight ------------------------------------
def _cpu_model(**kw):
    from valle2_amd import ConfigValle, get_model_class
    cfg = ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm',
                                  num_beams=4, top_k=1, max_audio_len=8), **kw))
    return get_model_class('ValleAR')(cfg)


@pytest.mark.parametrize('cfg_kw,call_kw,text', [
    ({}, dict(slots=17), 'slots=17 with beams=4'),
    ({}, dict(beams=3, slots=22), 'slots=22 with beams=3'),
    ({}, dict(beams=65), 'slots=None with beams=65'),
    ({}, dict(slots=0), 'slots=0'),
    ({}, dict(slots=-2), 'slots=-2'),
    ({}, dict(beams=0), 'beams=0'),
    (dict(n_heads=4), dict(beams=2), 'beams=2 with use_kv_cache=True, d_model=128, n_heads=4'),
    (dict(use_kv_cache=False), dict(beams=2), 'beams=2 with use_kv_cache=False'),
])
def test_generate_queued_refuses_without_a_device(cfg_kw, call_kw, text):
    m = _cpu_model(**cfg_kw)
    utts = [(torch.arange(5), torch.zeros(7, 8, dtype=torch.int64), None)] * 3
    with pytest.raises(ValueError, match=re.escape(text)) as e:
        m.generate_queued(utts, **call_kw)
    assert 'generate_queued:' in str(e.value)


# ---- the entry points refuse before any GPU work ---------------------------------------------------------------------------
def _poll(L, codes=P, stride=80, width=80, cl=I32, ap=I32, pb=I32, eos=1024, B=12, beams=4, max_new=8, done=I32, steps=I32,
          maxima=I32):
    return L.vh_decode_groups_poll(codes, stride, width, cl, ap, pb, eos, B, beams, max_new, done, steps, maxima, None)


@pytest.mark.parametrize('kw,text', [
    (dict(codes=None), 'null pointer'), (dict(cl=None), 'null pointer'), (dict(ap=None), 'null pointer'),
    (dict(pb=None), 'null pointer'), (dict(done=None), 'null pointer'), (dict(steps=None), 'null pointer'),
    (dict(maxima=None), 'null pointer'),
    (dict(B=13), 'B=13 is not a multiple of beams=4'), (dict(beams=0), 'beams=0'), (dict(B=0), 'B=0'),
    (dict(max_new=-1), 'max_new=-1'), (dict(width=0), 'codes_width=0'), (dict(stride=79), 'codes_stride=79'),
    (dict(codes=P + 4), '8-byte aligned'), (dict(ap=I32 + 2), '4-byte aligned'),
])
def test_poll_refuses_before_any_gpu_work(L, kw, text):
    assert _poll(L, **kw) < 0
    assert 'vh_decode_groups_poll:' in _err(L) and text in _err(L), _err(L)


def _reset(L, codes=P, stride=80, width=80, prompt=P2, prompt_len=5, prefix_len=11, bos=1025, eos=1024, group=1, B=12, beams=4,
           cl=I32, ap=I32, pb=I32, slp=I32, pl=I32):
    return L.vh_decode_group_reset(codes, stride, width, prompt, prompt_len, prefix_len, bos, eos, group, B, beams, cl, ap, pb,
                                   slp, pl, None)


@pytest.mark.parametrize('kw,text', [
    (dict(codes=None), 'null pointer'), (dict(prompt=None), 'null pointer'), (dict(cl=None), 'null pointer'),
    (dict(ap=None), 'null pointer'), (dict(pb=None), 'null pointer'), (dict(slp=None), 'null pointer'),
    (dict(pl=None), 'null pointer'),
    (dict(B=13), 'B=13 is not a multiple of beams=4'), (dict(beams=0), 'beams=0'),
    (dict(group=3), 'group=3 of 3'), (dict(group=-1), 'group=-1'),
    (dict(prompt_len=80), 'prompt_len=80'), (dict(prompt_len=-1), 'prompt_len=-1'),
    (dict(prefix_len=4), 'prefix_len=4 with prompt_len=5'), (dict(prompt_len=0, prefix_len=3), 'prefix_len=3 with prompt_len=0'),
    (dict(width=2, stride=2), 'codes_width=2'),
    (dict(prompt=P2 + 4), '8-byte aligned'), (dict(slp=I32 + 1), '4-byte aligned'),
])
def test_reset_refuses_before_any_gpu_work(L, kw, text):
    assert _reset(L, **kw) < 0
    assert 'vh_decode_group_reset:' in _err(L) and text in _err(L), _err(L)


def test_attention_with_groups_still_refuses_what_it_refused(L):
    """The parked form (prefix_len[g] == 0) is a value in a device array: the host-side checks are unchanged."""
    def call(q=P, plen=I32, B=12, beams=4):
        n = L.vh_attn_decode_shared_groups_ws_bytes(B, 2, 100, 2)
        return L.vh_attn_decode_shared_groups(q, 128, P, P, plen, 100, 128, P, P, P, 128, I32, 1, B, beams, 2, 32, 2, P2, n, None)
    for kw, text in [(dict(q=None), 'null pointer'), (dict(plen=None), 'null pointer'),
                     (dict(B=13), 'B=13 is not a multiple of beams=4')]:
        assert call(**kw) < 0
        assert 'vh_attn_decode_shared_groups:' in _err(L) and text in _err(L), _err(L)
