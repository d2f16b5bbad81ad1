"""generation.plan_decode / slot_key / unpack_utterances, the pure-Python part of AR generation: which caches every kind of
call gets, what its codes and counters look like, which calls may keep a decoder and which of them share one.  No device."""
import pytest
import torch

from valle2_amd import ConfigValle, engine, kernels
from valle2_amd import generation as G

F32, H16 = torch.float32, kernels.H16
TXS, PLS = [9, 12], [18, 62]                       # two utterances: text lengths, BOS + prompt


def _cfg(**kw):
    return ConfigValle(**dict(dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=1, dropout=0.0, norm='LayerNorm',
                                   num_beams=3, top_k=1, max_audio_len=40), **kw))


def _plan(cfg=None, txs=TXS, pls=PLS, max_new=40, **kw):
    return G.plan_decode(cfg or _cfg(), txs, pls, max_new=max_new, **kw)


# s0 = 12 + 62 = 74, pl_max = 62, s_max = roundup32(74 + 40) = 128, suffix = roundup32(41) = 64
@pytest.mark.parametrize('cfg_kw,call_kw,kind,prefix,rows,eligible', [
    # d_model / n_heads = 24 at d_model 120: 120 % 16 != 0, so the cached decoder does not serve it
    (dict(d_model=120, n_heads=5), {}, G.RECOMPUTE_GENERAL, None, None, False),
    (dict(n_heads=4), {}, G.ROWS_HD, None, (2, 128, F32, 32), True),
    ({}, dict(perf_mode=True), G.ROWS_PERF_PREFILL, None, (2, 128, H16, 64), True),
    ({}, {}, G.ROWS, None, (2, 128, F32, 64), True),
    # the two overrides of the table
    (dict(use_kv_cache=False), {}, G.ROWS, None, (2, 128, F32, 64), False),
    ({}, dict(perf_mode='kv'), G.ROWS, None, (2, 74, F32, 64), False),
    # dim_feedforward 192 is no multiple of 128: perf mode without the 16-bit prompt pass is the 'kv' form
    (dict(dim_feedforward=192), dict(perf_mode=True), G.ROWS, None, (2, 74, F32, 64), False),
    ({}, dict(beams=3), G.GROUPED, (2, 128, F32, 64), (6, 64, F32, 64), True),
    # the forms that drive the decoder by hand keep none
    ({}, dict(by_hand=True), G.ROWS, None, (2, 128, F32, 64), False),
])
def test_kinds_caches_codes_and_counters(cfg_kw, call_kw, kind, prefix, rows, eligible):
    cfg = _cfg(**cfg_kw)
    p = _plan(cfg, **call_kw)
    assert p.kind == kind and p.prefix_spec == prefix and p.rows_spec == rows and p.slot_eligible is eligible
    assert (p.s0, p.s_max, p.pl_max, p.ragged, p.fits) == (74, 128, 62, True, True)
    beams = call_kw.get('beams', 1)
    assert (p.G, p.beams, p.B) == (2, beams, 2 * beams)
    if kind == G.GROUPED:
        assert p.cap == engine.group_prefix_cap(74) == 128 and p.codes_width == 128 + 40
        assert p.cache_len0 == [-1] * 6 and p.row_pls == [18, 18, 18, 62, 62, 62]
    else:
        assert p.cap == 0 and p.codes_width == 62 + 40
        assert p.cache_len0 == [9 + 18 - 1, 12 + 62 - 1] and p.row_pls == PLS
    assert p.no_cache is (kind == G.RECOMPUTE_GENERAL or not cfg.use_kv_cache)
    assert (G.slot_key(p, cfg, 'cuda:0', ()) is not None) is eligible


@pytest.mark.parametrize('perf_mode,dtype,prefill_bf16', [(False, F32, False), (True, H16, True), ('kv', H16, False)])
def test_shared_prompt_caches(perf_mode, dtype, prefill_bf16):
    p = _plan(txs=[12] * 4, pls=[62] * 4, shared_prompt=True, perf_mode=perf_mode)
    assert p.kind == G.SHARED and not p.ragged and p.prefill_bf16 is prefill_bf16
    assert p.prefix_spec == (1, 96, dtype, 64) and p.rows_spec == (4, 64, dtype, 64)      # roundup32(74) keys, one row
    assert p.codes_width == 62 + 40 and p.cache_len0 == [-1] * 4 and p.slot_eligible       # ('kv' narrows into the slot's prefix)


def test_refusals_of_the_plan():
    with pytest.raises(ValueError, match='shared_prompt: identical rows'):
        _plan(shared_prompt=True)
    with pytest.raises(Exception, match='sequence exceeds the positional table'):
        _plan(pos_limits=(62 + 39, 5000))
    with pytest.raises(Exception, match='sequence exceeds the positional table'):
        _plan(pos_limits=(5000, 11))
    assert _plan(pos_limits=(62 + 40, 12)).kind == G.ROWS
    # a capacity beyond the records one merge serves: the caller falls back, the plan only says so
    long = _plan(txs=[100], pls=[9000], beams=3)
    assert long.kind == G.GROUPED and not long.fits


def test_the_queue_plans_what_generate_batch_plans_for_the_same_rows():
    cfg = _cfg()
    steps_cap = engine.queue_steps_cap(cfg.max_audio_len, G.EOS_POLL)              # 64
    cap = engine.group_prefix_cap(300)                                             # of a longer utterance further down the list
    queue = _plan(cfg, max_new=steps_cap, beams=3, queued=True, cap=cap)
    many = _plan(cfg, max_new=steps_cap, beams=3, cap=cap)
    for f in ('kind', 'G', 'beams', 'B', 'max_new', 'cap', 's0', 's_max', 'prefix_spec', 'rows_spec', 'cache_len0', 'row_pls',
              'ctx', 'ragged', 'fits', 'prefill_bf16', 'perf_mode', 'no_cache', 'use_graph', 'slot_eligible'):
        assert getattr(queue, f) == getattr(many, f), f
    assert queue.kind == G.GROUPED and queue.cap == 384 and queue.prefix_spec == (2, 384, F32, 64)
    assert queue.rows_spec == (6, 96, F32, 64)                                     # roundup32(steps_cap + 1)
    assert queue.codes_width == many.codes_width + 1 == 384 + 64 + 1               # a row may stand one past its last whole poll
    # one decoder each all the same: the queue's steps re-arm rows, generate_many's never do
    assert G.slot_key(queue, cfg, 'cuda:0', ()) != G.slot_key(many, cfg, 'cuda:0', ())
    # a queue of single beams is GROUPED too
    assert _plan(cfg, max_new=steps_cap, beams=1, queued=True, cap=cap).kind == G.GROUPED


def test_slot_keys_are_shared_and_kept_apart_as_before():
    cfg = _cfg()

    def key(cfg=cfg, device='cuda:0', weights=(1,), **kw):
        return G.slot_key(_plan(cfg, **kw), cfg, device, weights)
    assert key() == key() and hash(key()) == hash(key())
    # grouped prompts of other lengths under one capacity share the decoder; independent rows are keyed on their lengths
    assert key(beams=3) == key(txs=[30, 5], pls=[40, 90], beams=3)
    assert key(beams=3) != key(txs=[30, 5], pls=[40, 130], beams=3)                # capacity 256
    assert key() != key(txs=[30, 5], pls=[40, 90])
    assert key(txs=[12] * 4, pls=[62] * 4, shared_prompt=True) != key(txs=[12] * 4, pls=[62] * 4)
    # must not share: fp32 against perf mode, graph against eager steps, other sampling settings, weights, device, max_new
    assert key() != key(perf_mode=True)
    assert key(txs=[12] * 4, pls=[62] * 4, shared_prompt=True) != key(txs=[12] * 4, pls=[62] * 4, shared_prompt=True, perf_mode=True)
    assert key(txs=[12] * 4, pls=[62] * 4, shared_prompt=True, perf_mode='kv') != key(txs=[12] * 4, pls=[62] * 4, shared_prompt=True, perf_mode=True)
    assert key() != key(use_graph=False)
    for other in (dict(top_k=8), dict(top_k=8, tok_p=0.9), dict(top_k=8, temperature=0.7)):
        assert key() != key(cfg=_cfg(**other))
    assert key(cfg=_cfg(top_k=8)) != key(cfg=_cfg(top_k=8, tok_p=0.9)) != key(cfg=_cfg(top_k=8, temperature=0.7))
    assert key() != key(weights=(2,)) and key() != key(device='cuda:1') and key() != key(max_new=41)


def test_unpack_utterances():
    pt, tt = torch.arange(5), torch.arange(10, 13)
    codes = torch.arange(7 * 8).reshape(7, 8)
    texts, firsts = G.unpack_utterances([(pt, codes, None), (pt, codes, tt)])
    assert texts[0] is pt and torch.equal(texts[1], torch.tensor([0, 1, 2, 3, 4, 10, 11, 12]))
    assert all(torch.equal(f, codes[:, 0]) for f in firsts) and len(firsts) == 2
    assert G.unpack_utterances([]) == ([], [])
    for bad, text in (((pt[None], codes, None), 'Prompt tokens should be 1D tensor.'),
                      ((pt, codes[0], None), 'Prompt codes should be 2D tensor.'),
                      ((pt, codes, tt[None]), 'Target tokens should be 1D tensor.')):
        with pytest.raises(AssertionError) as e:
            G.unpack_utterances([bad])
        assert str(e.value) == text
