"""CPU companion of tests/test_train_widths_gpu.py: the whole-model cases build and their inputs are well conditioned; the
fp32-versus-float64 error measurements that the GPU file's tolerances for sums over rows rest on; and the comparison helpers
reject fp32 emulations of a wrong kernel — one planted fault each, caught on the quantity it is meant for.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import oracle_runners as R
from tests import test_train_widths_gpu as G
from tests.golden import cases as C

RUN_IDS = [f'{c}-{m[5:]}' for c, m, _ in R.TRAIN_WIDTH_RUNS]


# ---- A. the whole-model cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,cls_name,stage', R.TRAIN_WIDTH_RUNS + [('beyond', 'ValleAR', None)], ids=RUN_IDS + ['beyond-AR'])
def test_whole_model_case_builds_and_its_batch_is_valid(case, cls_name, stage):
    from valle2_amd import get_model_class, synth
    kw, sd, batch = R.train_width_inputs(case, cls_name)
    cfg = C.cfg_of(kw)
    assert (cfg.d_model, cfg.n_heads, cfg.dim_feedforward) == R.TRAIN_WIDTHS[case] and cfg.d_model == 64 * cfg.n_heads
    assert cfg.num_layers == 2 and cfg.dropout == 0.0
    with torch.device('meta'):                                     # shapes only: no second copy of up to 136 M parameters
        model = get_model_class(cls_name)(cfg)
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert have == {k: tuple(v.shape) for k, v in sd.items()} == dict(synth.state_dict_shapes(cfg, cls_name))
    assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in sd.values())
    assert batch['tokens'].shape[0] == 3 and int(batch['tokens'].min()) >= 0 and int(batch['tokens'].max()) < cfg.vocab_size
    if cls_name == 'ValleAR':
        assert 5 <= int(batch['tokens_lens'].min()) and int(batch['tokens_lens'].max()) == batch['tokens'].shape[1] <= 12
        assert 14 <= int(batch['codes_lens'].min()) and int(batch['codes_lens'].max()) <= 31
        assert batch['codes'].shape == batch['target'].shape == (3, int(batch['codes_lens'].max()))
        assert int(batch['codes'].max()) == cfg.bos_token and int(batch['target'].max()) <= cfg.eos_token
        assert bool((batch['codes'][:, 0] == cfg.bos_token).all()) and int(batch['target'].min()) >= 0
    else:
        assert 1 <= stage < cfg.num_quantizers and batch['codes'].shape == (3, 36, cfg.num_quantizers)
        assert int(batch['codes'].min()) >= 0 and int(batch['codes'].max()) < cfg.num_audio_tokens
        assert 0 < min(36 // 3, 3 * cfg.quantization_factor) < 36          # prefix and target frames both exist


@pytest.mark.parametrize('case,cls_name,stage', R.TRAIN_WIDTH_RUNS, ids=RUN_IDS)
def test_float32_oracle_loss_meets_the_tolerance_asked_of_the_gpu(case, cls_name, stage):
    """The oracle's own fp32 loss agrees with its float64 loss to the rtol 1e-5 the GPU test demands: the inputs are not too
    ill-conditioned for that tolerance."""
    kw, sd, batch = R.train_width_inputs(case, cls_name)
    cfg = C.cfg_of(kw)
    l64, _ = R.oracle_training_loss(sd, cfg, batch, cls_name, stage, torch.float64, grads=False)
    l32, _ = R.oracle_training_loss(sd, cfg, batch, cls_name, stage, torch.float32, grads=False)
    print(f'{case} {cls_name}: float64 {float(l64):.9f} float32 {float(l32):.9f}')
    torch.testing.assert_close(l32.double(), l64, rtol=1e-5, atol=1e-6)


# ---- B. the measurements behind the GPU file's tolerances for sums over rows ------------------------------------------------
def ln_measured(key):
    rows, d, ada, mean, dres = key
    inp = R.ln_inputs(rows, d, mean=mean, dres=dres)
    ref, emu = R.ln_reference(inp, ada), R.ln_reference(inp, ada, torch.float32)
    R.check_ln(emu, ref, G.LN_CASES.get(key) or {q: float('inf') for q in R.LN_SUMS if q in ref})    # per-element part; all with the table
    return {q: R.worst(emu[q], ref[q]) for q in R.LN_SUMS if q in ref}


def embed_measured(key):
    d, T, t0 = key
    tabs, ids = R.embed_inputs(d, T)
    dy = torch.randn(3, t0 + T, d, generator=R._g(35))
    ref, emu = (R.embed_reference(ids, dy, t0, tabs[0].shape[0], dt) for dt in (torch.float64, torch.float32))
    return max(R.worst(e, r) for e, r in zip(emu, ref))


def colsum_measured(key):
    x, out0 = R.colsum_inputs(*key)
    return R.worst(R.colsum_reference(x, out0, torch.float32), R.colsum_reference(x, out0))


def test_the_gpu_file_lists_every_case_the_kernels_need():
    ln = set(G.LN_CASES)
    for d in (132, 260, 516, 640, 768, 1028, 1536, 2048):
        assert {(9, d, False, 0.3, False), (9, d, True, 0.3, False)} <= ln
    for rows, d in ((2048, 128), (2053, 512), (4100, 256), (2053, 768), (2600, 1028)):
        assert {(rows, d, False, 0.3, False), (rows, d, True, 0.3, False)} <= ln
    assert (2053, 512, True, 0.3, True) in ln and any(k[3] == 50.0 for k in ln)
    assert {(8192 + 37, 1025, None, None), (45, 4097, None, None), (9, 16384, None, None)} <= set(G.CE_CASES)
    assert any(k[2] == k[1] + 7 for k in G.CE_CASES) and any(k[3] == 80.0 for k in G.CE_CASES)
    assert set(G.EMBED_CASES) == {(132, 37, 0), (768, 107, 5), (2048, 17, 0)}
    assert list(G.COLSUM_CASES) == R.COLSUM_CASES and G.pytestmark.name == 'gpu'


@pytest.mark.parametrize('key', list(G.LN_CASES), ids=lambda k: '-'.join(str(v) for v in k))
def test_layernorm_sums_fp32_error_is_what_the_gpu_file_says(key):
    now = ln_measured(key)
    assert set(now) == set(G.LN_CASES[key])
    for q, err in now.items():
        assert err <= G.LN_CASES[key][q], f'{q}: measured {err:.3e}, the GPU test was written for {G.LN_CASES[key][q]:.3e}'
        assert err >= 0.25 * G.LN_CASES[key][q], f'{q}: measured {err:.3e}: the figure {G.LN_CASES[key][q]:.3e} in the GPU test is stale'


@pytest.mark.parametrize('table,measure', [(G.EMBED_CASES, embed_measured), (G.COLSUM_CASES, colsum_measured)],
                         ids=['embedding', 'colsum'])
def test_row_sums_fp32_error_is_what_the_gpu_file_says(table, measure):
    for key, written in table.items():
        err = measure(key)
        assert 0.25 * written <= err <= written, f'{key}: measured {err:.3e}, the GPU test says {written:.3e}'


def test_layernorm_reference_is_torch_autograd_in_float64():
    """R.ln_reference, written out from the definition, against F.layer_norm differentiated by torch in float64."""
    for rows, d, ada in ((9, 132, True), (9, 516, False), (2053, 512, True)):
        inp = R.ln_inputs(rows, d, dres=True)
        ref = R.ln_reference(inp, ada)
        leaf = {k: inp[k].double().requires_grad_() for k in ('x', 'gamma', 'beta', 'scale', 'shift')}
        y = F.layer_norm(leaf['x'], (d,), leaf['gamma'], leaf['beta'], 1e-5)
        y = leaf['scale'] * y + leaf['shift'] if ada else y
        y.backward(inp['dy'].double())
        pairs = [('y', y), ('dx', leaf['x'].grad + inp['dres'].double()), ('dgamma', leaf['gamma'].grad), ('dbeta', leaf['beta'].grad)]
        pairs += [('dscale', leaf['scale'].grad), ('dshift', leaf['shift'].grad)] if ada else []
        for name, t in pairs:
            torch.testing.assert_close(ref[name], t.detach(), rtol=1e-11, atol=1e-11, msg=lambda m, n=name: f'{n}: {m}')
        torch.testing.assert_close(ref['dcol'], ref['dx'].sum(0), rtol=1e-12, atol=1e-12)


def test_softmax_and_cross_entropy_references_are_torch_autograd_in_float64():
    for name in R.SOFTMAX_CASES:
        S, dP, _, spec = R.softmax_inputs(name)
        s = S.double().requires_grad_()
        p = torch.softmax((s * R.SOFTMAX_SCALE).masked_fill(~R.softmax_visible(name, spec), -float('inf')), -1)
        p.backward(dP.double())
        ref = R.softmax_reference(name)
        R.check_softmax(p, s.grad, ref)
        torch.testing.assert_close(ref['dS'], s.grad, rtol=1e-11, atol=1e-13)
        R.check_softmax(*(R.softmax_reference(name, torch.float32)[k] for k in ('P', 'dS')), ref)     # a right kernel passes
    logits, target = R.ce_inputs(45, 1025, 1032)
    lg = logits.double().requires_grad_()
    loss = F.cross_entropy(lg, target)
    (3.0 * loss).backward()
    ref = R.ce_reference(logits, target, 3.0)
    torch.testing.assert_close(ref['loss'], loss.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(ref['dlogits'], lg.grad, rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize('key', G.CE_CASES, ids=lambda k: '-'.join(str(v) for v in k))
def test_cross_entropy_fp32_emulation_passes_its_check(key):
    """A right kernel — the same arithmetic in fp32, rows added one after the other — passes check_ce at every case (at
    amplitude 80 too: the row maximum comes off before the exponential); a row left out does not."""
    rows, V, ld, amp = key
    logits, target = R.ce_inputs(rows, V, ld, amp)
    ref = R.ce_reference(logits, target, 3.0)
    emu = R.ce_reference(logits, target, 3.0, torch.float32)
    R.check_ce(emu['loss'], emu['dlogits'], ref, rows)
    short = R.ce_reference(logits[:-1], target[:-1], 3.0, torch.float32)
    with pytest.raises(AssertionError, match='failed: loss'):
        R.check_ce(short['loss'] * (rows - 1) / rows, emu['dlogits'], ref, rows)


# ---- C. the helpers reject a wrong kernel -----------------------------------------------------------------------------------
def _failed(excinfo):
    return set(str(excinfo.value).split(' | ')[0][len('failed: '):].split(', '))


@pytest.mark.parametrize('key,fault,expect', [
    ((9, 132, False, 0.3, False), 'tail_unmasked', {'dx', 'dgamma'}),
    ((2053, 768, False, 0.3, False), 'last_row', {'dx', 'dgamma', 'dbeta'}),
    ((2053, 512, True, 0.3, True), 'last_row', {'dx', 'dgamma', 'dbeta', 'dscale', 'dshift', 'dcol'}),
    ((2053, 512, True, 0.3, True), 'stale_ahead', {'dx', 'dgamma', 'dbeta', 'dscale', 'dshift', 'dcol'}),
], ids=['tail_unmasked-132', 'last_row-768', 'last_row-512-dcol', 'stale_ahead-512'])
def test_planted_layernorm_faults_are_rejected(key, fault, expect):
    rows, d, ada, mean, dres = key
    inp = R.ln_inputs(rows, d, mean=mean, dres=dres)
    ref = R.ln_reference(inp, ada)
    R.check_ln(R.ln_reference(inp, ada, torch.float32), ref, G.LN_CASES[key])              # the right emulation passes
    with pytest.raises(AssertionError, match='failed: ') as e:
        R.check_ln(R.ln_reference(inp, ada, torch.float32, fault=fault), ref, G.LN_CASES[key])
    assert _failed(e) == expect, str(e.value)


def test_planted_softmax_fault_dropped_qpos_is_rejected():
    ref = R.softmax_reference('prefix_tq_lt_tk')
    emu = R.softmax_reference('prefix_tq_lt_tk', torch.float32, fault='no_qpos')
    with pytest.raises(AssertionError, match='failed: ') as e:
        R.check_softmax(emu['P'], emu['dS'], ref)
    assert _failed(e) == {'P', 'dS'}
    # where Tq == Tk the offset is zero and the fault cannot show: the case with Tq < Tk is what catches it
    same = R.softmax_reference('prefix_rows', torch.float32, fault='no_qpos')
    R.check_softmax(same['P'], same['dS'], R.softmax_reference('prefix_rows'))


def test_planted_cross_entropy_fault_ld_for_v_is_rejected():
    key = next(k for k in G.CE_CASES if k[2] == k[1] + 7)
    logits, target = R.ce_inputs(*key)
    ref = R.ce_reference(logits, target, 3.0)
    emu = R.ce_reference(logits, target, 3.0, torch.float32, fault='ld_for_V')
    with pytest.raises(AssertionError, match='failed: ') as e:
        R.check_ce(emu['loss'], emu['dlogits'], ref, key[0])
    assert _failed(e) == {'loss', 'dlogits'}
    # on a dense buffer (ld == V) the fault cannot show
    logits, target = R.ce_inputs(45, 1025)
    dense = R.ce_reference(logits, target, 3.0, torch.float32, fault='ld_for_V')
    R.check_ce(dense['loss'], dense['dlogits'], R.ce_reference(logits, target, 3.0), 45)
