"""Per-request sampling of the NAR stage on the device: `vh_categorical_rows_keyed` against `vh_categorical_rows` bit for bit,
its keys (request, frame) against the places of the rows in a launch, its draws against the float64 mirror
(tests/nar_sampling_replay.py) and against the distribution; `ValleNAR.generate_batch(sampling=[...])` / `generate(sampling=)` and
`codec_io.synthesize_requests`: a request's codes are a function of the request alone.

Measured on the MI355X (the mirror case prints its figures): 40 of 6000 draws ambiguous (0.67 %) at V = 1024, 1 of 6000 (0.017 %) at
V = 37, no token that differs from the mirror's."""
import pytest
import torch
import torch.nn.functional as F

from tests import nar_sampling_replay as NR
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _requests(records):
    from valle2_amd import kernels as K
    return K.pack_row_sampling(records).to(DEV)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).to(DEV)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [5, 37, 64, 1024, 1025])
def test_one_request_keyed_by_row_is_categorical_rows_bit_for_bit(V):
    """Empty lanes (V < 64), a last lane that is partly filled (1025), rows that do not fill the four of a workgroup, a padded row
    stride with 100.0 beyond V (never read as a score)."""
    from valle2_amd import kernels as K
    seed, stream_id, temperature = 2 ** 63 + 99, 0x80000003, 0.85
    for rows in (1, 3, 70):
        padded = torch.full((rows, V + 3), 100.0)
        padded[:, :V] = 2.0 * torch.randn(rows, V, generator=torch.Generator().manual_seed(V * 100 + rows))
        logits = padded.to(DEV)[:, :V]
        want, want_lp = torch.empty(rows, device=DEV, dtype=torch.int64), torch.empty(rows, device=DEV)
        K.categorical_rows(logits, want, temperature=temperature, seed=seed, stream_id=stream_id, logprob=want_lp)
        got, got_lp = torch.full((1, rows), -1, device=DEV, dtype=torch.int64), torch.full((rows,), -7.0, device=DEV)
        K.categorical_rows_keyed(logits, got, _requests([(seed, 0, 0, 1.0, temperature)]), _i32([0] * rows), _i32(range(rows)),
                                 stream_id, logprob=got_lp)
        assert int(want.min()) >= 0 and int(want.max()) < V
        assert torch.equal(got[0], want), (V, rows)
        assert torch.equal(got_lp, want_lp), (V, rows)
        # the greedy form too: a record with top_k == 1, whatever its temperature
        K.categorical_rows(logits, want, greedy=True, logprob=want_lp)
        K.categorical_rows_keyed(logits, got, _requests([(seed, 0, 1, 1.0, 0.3)]), _i32([0] * rows), _i32(range(rows)), stream_id,
                                 logprob=got_lp)
        assert torch.equal(got[0], want) and torch.equal(got_lp, torch.zeros_like(got_lp)) and torch.equal(want_lp, got_lp)


def test_draws_follow_the_keys_not_the_places_of_the_rows():
    from valle2_amd import kernels as K
    V, n_keys, stream_id = 1025, 50, 0x80000005
    g = torch.Generator().manual_seed(7)
    logits = 2.0 * torch.randn(3, n_keys, V, generator=g)
    logits[0, 4, 17] = logits[0, 4, 900] = 30.0                          # an exact tie at the top of a greedy row: the lowest index
    logits[0, 9, 1024] = 31.0                                            # the maximum in the last lane's range
    records = [(11, 0, 1, 1.0, 0.9), (12, 0, 0, 1.0, 0.6), (2 ** 64 - 3, 0, 50, 0.5, 1.7)]     # greedy; two temperatures
    # request 1 has 40 frames, request 2 lacks frames 7 and 33: no row names those keys
    named = [(0, t) for t in range(n_keys)] + [(1, t) for t in range(40)] + [(2, t) for t in range(n_keys) if t not in (7, 33)]
    bad = [(-1, 3), (3, 3), (1, -1), (1, n_keys), (2 ** 31 - 1, 0), (0, -(2 ** 31))]       # out of range: nothing read or written
    requests = _requests(records)
    outs = []
    for shuffle in (1, 2):
        pairs = named + bad
        order = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(shuffle)).tolist()
        pairs = [pairs[i] for i in order]
        rows = torch.stack([logits[min(max(gi, 0), 2), min(max(t, 0), n_keys - 1)] for gi, t in pairs]).to(DEV)
        codes = torch.full((3, n_keys, 8), -1, device=DEV, dtype=torch.int64)
        lp = torch.full((len(pairs),), -7.0, device=DEV)
        K.categorical_rows_keyed(rows, codes[:, :, 5], requests, _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs]),
                                 stream_id, logprob=lp)
        codes, lp = codes.cpu(), lp.cpu()
        assert int((codes[:, :, :5] != -1).sum()) == 0 and int((codes[:, :, 6:] != -1).sum()) == 0, 'other codebooks'
        written = torch.zeros(3, n_keys, dtype=torch.bool)
        for gi, t in named:
            written[gi, t] = True
        assert bool((codes[:, :, 5][~written] == -1).all()), 'slots of keys that no row named'
        tok = codes[:, :, 5]
        assert bool(((tok[written] >= 0) & (tok[written] < V)).all())
        is_bad = torch.tensor([p in bad for p in pairs])
        assert bool((lp[is_bad] == -7.0).all()) and bool((lp[~is_bad] <= 0.0).all()), 'log-probabilities follow the packed rows'
        outs.append(tok)
    assert torch.equal(outs[0], outs[1]), 'another packed order must store the same (request, frame) tokens'
    tok = outs[0]
    want0 = torch.argmax(logits[0], dim=-1)
    want0[4] = 17
    assert torch.equal(tok[0], want0) and int(tok[0, 9]) == 1024
    # request 1 alone, unshuffled, through the unkeyed launch with its seed and temperature: row index == frame
    alone = torch.empty(40, device=DEV, dtype=torch.int64)
    K.categorical_rows(logits[1, :40].to(DEV), alone, temperature=0.6, seed=12, stream_id=stream_id)
    assert torch.equal(tok[1, :40], alone.cpu())
    assert not torch.equal(tok[1, :40], tok[2, :40])


@pytest.mark.parametrize('V', [1024, 37])
def test_draws_are_the_mirrors_outside_the_band(V):
    """6000 distinct rows, two requests (temperatures 0.9 and 1.0) of 3000 frames each: every token is the float64 mirror's or the
    draw lies within DELTA of the boundary between the two; at most AMBIGUOUS_CAP of the draws are that close to any boundary."""
    from valle2_amd import kernels as K
    from valle2_amd.sampling import NAR_STREAM
    n, stage = 3000, 3
    seeds, temps = (2 ** 63 + 17, 4242), (0.9, 1.0)
    logits = 2.0 * torch.randn(2 * n, V, generator=torch.Generator().manual_seed(1000 + V))
    tokens = torch.full((2, n), -1, device=DEV, dtype=torch.int64)
    K.categorical_rows_keyed(logits.to(DEV), tokens, _requests([(seeds[0], 0, 0, 1.0, temps[0]), (seeds[1], 0, 0, 1.0, temps[1])]),
                             _i32([0] * n + [1] * n), _i32(list(range(n)) * 2), NAR_STREAM | stage)
    tokens = tokens.cpu().reshape(-1).numpy()
    us = [NR.nar_uniform(seeds[g], t, stage) for g in range(2) for t in range(n)]
    row_temps = [temps[g] for g in range(2) for _ in range(n)]
    ambiguous, excused, worst = NR.hold_rows(logits.numpy(), tokens, row_temps, us)
    print(f'V = {V}: {2 * n} draws, {ambiguous} ambiguous ({ambiguous / (2 * n):.4%}), {excused} disagreements with the mirror, all '
          f'inside the band, the worst {worst:.3e} from the boundary')
    assert ambiguous <= NR.AMBIGUOUS_CAP * 2 * n


def test_keyed_draws_follow_the_distribution_the_stream_and_the_seed():
    from valle2_amd import kernels as K
    V, n, temperature = 1024, 40000, 0.6
    row = 2.0 * torch.randn(V, generator=torch.Generator().manual_seed(V))
    probs = F.softmax(row / temperature, dim=-1)
    logits = row.to(DEV)[None].expand(n, -1).contiguous()
    zeros, keys = _i32([0] * n), _i32(range(n))

    def draw(seed, stream_id, lp=None):
        tok = torch.empty(1, n, device=DEV, dtype=torch.int64)
        K.categorical_rows_keyed(logits, tok, _requests([(seed, 0, 0, 1.0, temperature)]), zeros, keys, stream_id, logprob=lp)
        return tok[0].cpu()
    lp = torch.empty(n, device=DEV)
    tok = draw(99, 0x80000003, lp)
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    freq = torch.bincount(tok, minlength=V).float() / n
    sigma = torch.sqrt(probs * (1 - probs) / n)
    assert bool(((freq - probs).abs() <= 4 * sigma + 1e-4).all()), (freq - probs).abs().max()
    torch.testing.assert_close(lp.cpu(), torch.log(probs[tok]), atol=2e-5, rtol=1e-5)
    assert torch.equal(draw(99, 0x80000003), tok), 'same (seed, frame, stream) must give the same draw'
    assert not torch.equal(draw(99, 0x80000004), tok), 'another stage must draw afresh'
    assert not torch.equal(draw(100, 0x80000003), tok), 'another seed must draw afresh'


def test_binding_refuses_wrong_shapes_and_dtypes():
    from valle2_amd import _lib, kernels as K
    logits = torch.randn(6, 37, device=DEV)
    tok = torch.empty(2, 3, device=DEV, dtype=torch.int64)
    req, rr, rk = _requests([(1, 0, 0, 1.0, 1.0)] * 2), _i32([0, 0, 0, 1, 1, 1]), _i32([0, 1, 2] * 2)
    K.categorical_rows_keyed(logits, tok, req, rr, rk, 1)
    for kw in (dict(tokens=tok.int()), dict(tokens=tok[0]), dict(tokens=tok.cpu()), dict(requests=req[:1]), dict(requests=req.cpu()),
               dict(requests=req.view(torch.int8)), dict(row_request=rr.long()), dict(row_key=rk[:5]), dict(logits=logits.T),
               dict(logprob=torch.empty(5, device=DEV))):
        args = dict(dict(logits=logits, tokens=tok, requests=req, row_request=rr, row_key=rk, stream_id=1), **kw)
        with pytest.raises(_lib.VhError):
            K.categorical_rows_keyed(**args)


# ---- 2. the model ------------------------------------------------------------------------------------------------------------
SHAPES = [(15, 12, 70), (9, 30, 81), (22, 5, 66)]
# why these shapes: every utterance has more than 64 rows (text + prompt + target) and more than 64 target frames, K = d_model and
# dim_feedforward are below 1024 (no split-K) and there are fewer than 256 tiles: every GEMM of a request runs on the same kernel
# alone and in a batch, so its logits — and with them every token — are the same bits in both.


@pytest.fixture(scope='module')
def nar():
    from valle2_amd import get_model_class, synth
    cfg = C.cfg_of(C.NAR_TINY)
    m = get_model_class('ValleNAR')(cfg)
    m.load_state_dict(synth.make_state_dict(cfg, 'ValleNAR', seed=13, rich=True))
    g = torch.Generator().manual_seed(5)
    us = [(torch.randint(0, cfg.vocab_size, (tx,), generator=g).to(DEV),
           torch.randint(0, cfg.num_audio_tokens, (tc, cfg.num_quantizers), generator=g).to(DEV),
           torch.randint(0, cfg.num_audio_tokens, (ty,), generator=g).to(DEV)) for tx, tc, ty in SHAPES]
    return m.to(DEV).eval(), us


def _batch(m, us, order, **kw):
    outs = m.generate_batch([us[i][0] for i in order], [us[i][1] for i in order], [us[i][2] for i in order], **kw)
    return {i: o for i, o in zip(order, outs)}


def test_a_requests_codes_do_not_depend_on_the_batch_the_order_or_torchs_generator(nar):
    from valle2_amd import Sampling
    m, us = nar
    greedy = _batch(m, us, [0, 1, 2], greedy=True)
    for i in range(3):                                     # first: the logits themselves agree between the two forms
        assert torch.equal(_batch(m, us, [i], greedy=True)[i], greedy[i]), f'greedy utterance {i} alone / in the batch'
    ss = [Sampling(2 ** 63 + 11, temperature=0.9), Sampling(12), Sampling(13, top_k=8, tok_p=0.5, temperature=1.3)]
    torch.manual_seed(1)
    batch = _batch(m, us, [0, 1, 2], sampling=ss)
    torch.manual_seed(2)
    again = _batch(m, us, [0, 1, 2], sampling=ss)
    reverse = _batch(m, us, [2, 1, 0], sampling=ss[::-1])
    assert torch.equal(torch.random.get_rng_state(), torch.manual_seed(2).get_state()), 'nothing is drawn from torch\'s generator'
    for i, (text, pc, first) in enumerate(us):
        got = batch[i]
        assert got.shape == (SHAPES[i][2], 8) and got.dtype == torch.int64 and torch.equal(got[:, 0], first)
        assert int(got.min()) >= 0 and int(got.max()) < 1024
        assert not torch.equal(got, greedy[i])
        assert torch.equal(_batch(m, us, [i], sampling=[ss[i]])[i], got), f'utterance {i} alone'
        assert torch.equal(reverse[i], got), f'utterance {i} in the reversed batch'
        assert torch.equal(again[i], got), f'utterance {i} after torch.manual_seed with another value'
        assert torch.equal(m.generate(text[:4], pc, text[4:], first, sampling=ss[i]), got), f'utterance {i} through generate()'
    # another seed: other codes; the same seed on another utterance: its own logits, other codes
    other = _batch(m, us, [0, 1, 2], sampling=[Sampling(2 ** 63 + 12, temperature=0.9), ss[1], ss[2]])
    assert not torch.equal(other[0], batch[0]) and torch.equal(other[1], batch[1]) and torch.equal(other[2], batch[2])
    # a request with top_k == 1 is its greedy run inside a sampled batch; greedy=True makes every request greedy
    mixed = _batch(m, us, [0, 1, 2], sampling=[ss[0], Sampling(5, top_k=1, temperature=0.3), ss[2]])
    assert torch.equal(mixed[1], greedy[1]) and torch.equal(mixed[0], batch[0]) and torch.equal(mixed[2], batch[2])
    flag = _batch(m, us, [0, 1, 2], greedy=True, sampling=ss)
    assert all(torch.equal(flag[i], greedy[i]) for i in range(3))
    # calls without a Sampling keep their own path: seeded from torch's generator
    torch.manual_seed(11)
    a = _batch(m, us, [0, 1])
    torch.manual_seed(11)
    assert all(torch.equal(x, y) for x, y in zip(a.values(), _batch(m, us, [0, 1]).values()))


def test_synthesize_requests_codes_are_a_function_of_the_item_alone():
    """silence_eos and a Sampling with top_k = 8 keep EOS (logit exactly 0) out of the AR stage's kept set, so every utterance runs
    to max_audio_len = 70 frames: more than 64 target frames in the NAR stage, alone or batched."""
    from valle2_amd import ConfigValle, Sampling, codec_io as CIO, get_model_class, synth
    base = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0)
    ar_cfg = ConfigValle(**base, norm='LayerNorm', num_beams=2, top_k=50, max_audio_len=70)
    nar_cfg = ConfigValle(**base, norm='AdaptiveLayerNorm')
    ar = get_model_class('ValleAR')(ar_cfg)
    ar.load_state_dict(synth.silence_eos(synth.make_state_dict(ar_cfg, 'ValleAR', seed=1), ar_cfg))
    nar = get_model_class('ValleNAR')(nar_cfg)
    nar.load_state_dict(synth.make_state_dict(nar_cfg, 'ValleNAR', seed=2))
    ar, nar = ar.to(DEV).eval(), nar.to(DEV).eval()
    items = []
    for i, s in enumerate([Sampling(71, top_k=8, temperature=0.9), Sampling(72, top_k=8), Sampling(73, top_k=8, temperature=1.2)]):
        pt, pc, tt = synth.synth_utterance(ar_cfg, 5 + 2 * i, 7 - i, 9 + 6 * i, seed=60 + i)
        items.append((pt.to(DEV), pc.T.contiguous().to(DEV), tt.to(DEV), s))           # codec layout (Q, T)
    A, B, Cc = items
    torch.manual_seed(3)
    abc = CIO.synthesize_requests(ar, nar, [A, B, Cc])
    torch.manual_seed(4)
    ca = CIO.synthesize_requests(ar, nar, [Cc, A])
    queued = CIO.synthesize_requests(ar, nar, [A, B, Cc], queued=True, slots=2)
    assert len(abc) == 3 and len(ca) == 2 and len(queued) == 3
    a = abc[0]
    assert a.shape[0] == 8 and a.shape[1] > 64 and a.dtype == torch.int64, a.shape
    assert torch.equal(ca[1], a), 'A in [C, A]'
    assert torch.equal(queued[0], a), 'A through the queue with two slots'
    assert torch.equal(ca[0], abc[2]) and torch.equal(queued[2], abc[2]) and torch.equal(queued[1], abc[1])
    first = ar.generate(A[0], CIO.to_prompt_codes(A[1], ar_cfg), A[2], sampling=A[3])
    assert torch.equal(a[0], first), 'the first codebook is the AR model\'s own generate(sampling=)'
    assert not torch.equal(a[1:], abc[1][1:])
