"""The codec at the architectures `deep`, `taps` and `flat` (tests/codec_rules.py) without a GPU: the float64 mirror against a
live `transformers` model at those configs (where the package is installed), `EncodecCodec.from_state_dict` on them — hop, the
repacked shapes, the refusal that names `compress` — and the table of compiled forms: a pure-Python restatement of the three
dispatch rules of csrc/codec.hip, every form selected by some parameter list of the codec's device tests, and as many launch
sites in the source as the table has forms, so that a form added later fails here until a case covers it."""
import collections
import re
from pathlib import Path

import pytest
import torch

from tests import codec_enc_mirror as E
from tests import codec_mirror as M
from tests.codec_rules import CONFIGS, HOPS, codec_state_dict, conv_form, lstm_form, rvq_form

REPO = Path(__file__).resolve().parent.parent
NAMES = sorted(CONFIGS)


# ---- the mirror against a live model ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=NAMES)
def live(request):
    pytest.importorskip('transformers')
    from tests.golden.gen_codec_golden import build_model
    cfg = CONFIGS[request.param]
    return request.param, cfg, build_model(3, target_bandwidths=[144.0], **cfg).double()


@pytest.mark.parametrize('T', [1, 2, 11])
def test_mirror_decode_equals_a_live_model(live, T):
    from tests.golden.gen_codec_golden import decoder_state_dict, model_decode
    name, cfg, model = live
    n_q = len(model.quantizer.layers)
    codes = torch.randint(0, cfg['codebook_size'], (2, n_q, T), generator=torch.Generator().manual_seed(T))
    want = model_decode(model, codes)
    got = M.decode(decoder_state_dict(model), codes, **cfg)
    assert tuple(got.shape) == tuple(want.shape) == (2, HOPS[name] * T)
    err = (got - want).abs().max().item()
    print(f'{name} decode T{T}: {n_q} codebooks, max|mirror - model| = {err:.2e}, max|model| = {want.abs().max().item():.3f}')
    assert err <= 1e-10 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('which', ['1', 'hop-1', 'hop+1', '5hop+3'])
def test_mirror_encode_equals_a_live_model(live, which):
    from tests.golden.gen_codec_enc_golden import encoder_state_dict, model_encode
    name, cfg, model = live
    hop = HOPS[name]
    L = {'1': 1, 'hop-1': hop - 1, 'hop+1': hop + 1, '5hop+3': 5 * hop + 3}[which]
    wave = 0.3 * torch.randn(2, L, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    want_codes, want_emb = model_encode(model, wave)
    codes, emb = E.encode(encoder_state_dict(model), wave, **cfg)
    T = -(-L // hop)
    assert tuple(emb.shape) == tuple(want_emb.shape) == (2, T, cfg['hidden_size']) and tuple(codes.shape) == tuple(want_codes.shape)
    err = (emb - want_emb).abs().max().item()
    print(f'{name} encode L{L}: max|mirror - model| = {err:.2e}, max|model| = {want_emb.abs().max().item():.3f}')
    assert err <= 1e-10 * max(1.0, want_emb.abs().max().item())
    assert torch.equal(codes, want_codes)


# ---- the loader, no device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_from_state_dict_repacks_every_config_without_a_device(name, monkeypatch):
    from valle2_amd import EncodecCodec, _lib
    from valle2_amd.codec import state_dict_keys
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('device work in from_state_dict'))
    cfg = M.arch_of(**CONFIGS[name])
    sd = codec_state_dict(21, **CONFIGS[name])
    codec = EncodecCodec.from_state_dict(sd, **CONFIGS[name])
    ratios, nf = cfg['upsampling_ratios'], cfg['num_filters']
    assert codec.hop == codec.encoder.hop == codec.decoder.hop == HOPS[name] == M.hop_of(cfg)
    assert codec.encoder.ratios == tuple(reversed(ratios)) and codec.num_codebooks == 8
    dec, enc = codec.decoder._host, codec.encoder._host
    width = nf * 2 ** len(ratios)
    assert tuple(dec['first'][0].shape) == (width, cfg['kernel_size'], cfg['hidden_size'])
    assert tuple(enc['first'][0].shape) == (nf, cfg['kernel_size'])
    assert len(dec['lstm']) == len(enc['lstm']) == cfg['num_lstm_layers']
    for w_ih, bias, w_hh in dec['lstm'] + enc['lstm']:
        assert tuple(w_ih.shape) == (4 * width, 1, width) and tuple(bias.shape) == (4 * width,) and tuple(w_hh.shape) == (4 * width, width)
    assert len(dec['stages']) == len(enc['stages']) == len(ratios)
    keys = state_dict_keys(cfg)
    for i, (r, stage) in enumerate(zip(ratios, dec['stages'])):
        c_in, c_out = width >> i, width >> (i + 1)
        up, up_b = stage['up']
        assert tuple(up.shape) == (r * c_out, 2, c_in) and tuple(up_b.shape) == (r * c_out,)
        # w[(p, co), 0, ci] = wt[ci, co, p + r] (the frame before), w[(p, co), 1, ci] = wt[ci, co, p]
        wt, bt = M.folded(sd, keys['stages'][i]['up'], torch.float64)
        assert tuple(wt.shape) == (c_in, c_out, 2 * r)
        up4 = up.view(r, c_out, 2, c_in)
        assert torch.equal(up4[:, :, 0], wt[:, :, r:].permute(2, 1, 0).float()) and torch.equal(up4[:, :, 1], wt[:, :, :r].permute(2, 1, 0).float())
        assert torch.equal(up_b.view(r, c_out), bt.float().expand(r, c_out))
        assert [blk['dilation'] for blk in stage['blocks']] == [cfg['dilation_growth_rate'] ** j for j in range(cfg['num_residual_layers'])]
        for blk in stage['blocks']:
            hid = c_out // cfg['compress']
            assert tuple(blk['conv1'][0].shape) == (hid, cfg['residual_kernel_size'], c_out)
            assert tuple(blk['conv2'][0].shape) == (c_out, 1, hid) and tuple(blk['shortcut'][0].shape) == (c_out, 1, c_out)
    for i, (r, stage) in enumerate(zip(reversed(ratios), enc['stages'])):
        c = nf << i
        assert tuple(stage['down'][0].shape) == (2 * c, 2 * r, c) and tuple(stage['down'][1].shape) == (2 * c,)
        assert [blk['dilation'] for blk in stage['blocks']] == [cfg['dilation_growth_rate'] ** j for j in range(cfg['num_residual_layers'])]
        for blk in stage['blocks']:
            assert tuple(blk['conv1'][0].shape) == (c // cfg['compress'], cfg['residual_kernel_size'], c)
    assert tuple(dec['last'][0].shape) == (1, cfg['last_kernel_size'], nf)
    assert tuple(enc['last'][0].shape) == (cfg['hidden_size'], cfg['last_kernel_size'], width)
    assert tuple(enc['e_sq'].shape) == (8, cfg['codebook_size']) and enc['e_sq'].dtype == torch.float32
    assert tuple(dec['codebooks'].shape) == tuple(enc['codebooks'].shape) == (8, cfg['codebook_size'], cfg['hidden_size'])
    assert torch.equal(enc['e_sq'], E.codebooks_of(sd).pow(2).sum(-1).float())


def test_from_state_dict_refuses_four_filters_at_the_taps_config_naming_compress():
    """Three stages halve 32 channels down to 4, whose residual blocks would hold 4 / 2 = 2 hidden channels: not a multiple of 4."""
    from valle2_amd import EncodecCodec, EncodecDecoder, EncodecEncoder
    cfg = dict(CONFIGS['taps'], num_filters=4)
    sd = codec_state_dict(21, **CONFIGS['taps'])
    for cls in (EncodecCodec, EncodecDecoder, EncodecEncoder):
        with pytest.raises(ValueError, match='compress'):
            cls.from_state_dict(sd, **cfg)


# ---- the table of compiled forms -------------------------------------------------------------------------------------------
CONV_FORMS = {(nt, down) for nt in (1, 2, 4) for down in (False, True)}      # conv1d_causal_kernel<NT, DOWN>
LSTM_FORMS = {1, 2, 3, 4}                                                   # lstm_step_kernel<NI>
RVQ_FORMS = {4, 8, 16}                                                      # rvq_encode_kernel<NS>
LAUNCH_SITES = {'rvq_decode_kernel': 1, 'conv1d_causal_kernel': len(CONV_FORMS), 'lstm_step_kernel': len(LSTM_FORMS),
                'conv1d_wave_kernel': 1, 'rvq_encode_kernel': len(RVQ_FORMS)}


def parametrized(fn, name):
    """The values a test function is parametrised with under `name`."""
    return next(m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == name)


def test_form_rules_at_their_thresholds():
    assert [conv_form(c) for c in (1, 4, 32, 36, 64, 68, 132, 512)] == [1, 1, 1, 2, 2, 4, 4, 4]
    assert [lstm_form(h) for h in (4, 256, 260, 512, 516, 768, 772, 1024)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [rvq_form(d) for d in (4, 32, 36, 64, 68, 128)] == [4, 4, 8, 8, 16, 16]


def test_every_compiled_form_is_launched_by_a_device_test():
    from tests import test_codec_enc_gpu as enc_gpu, test_codec_forms_gpu as forms, test_codec_gpu as dec_gpu
    conv = {(conv_form(c_out), False) for _, c_out in forms.CONV_CHANNELS + forms.LENS_CHANNELS + dec_gpu.CHANNELS}
    conv |= {(conv_form(c_out), True) for _, c_out, _ in forms.DOWN + enc_gpu.DOWN}
    assert conv == CONV_FORMS, sorted(CONV_FORMS - conv)
    widths = {H for H, _, _ in forms.LSTM} | set(parametrized(dec_gpu.test_lstm_block_against_the_float64_mirror, 'H'))
    assert {lstm_form(H) for H in widths} == LSTM_FORMS, sorted(widths)
    # a full slice followed by a nearly empty one, and every slice full, at the widest form
    assert {H % 256 for H in widths if lstm_form(H) == 4} >= {0, 4} and 260 in widths
    depths = {case[3] for case in forms.RVQ + enc_gpu.RVQ}
    assert {rvq_form(D) for D in depths} == RVQ_FORMS, sorted(depths)
    assert {rvq_form(D) for _, D in forms.TIES} >= {8, 16}


def test_the_source_has_as_many_launch_sites_as_the_table_has_forms():
    src = (REPO / 'valle2_amd' / 'csrc' / 'codec.hip').read_text()
    sites = collections.Counter(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', src))
    assert dict(sites) == LAUNCH_SITES
    for nt, down in CONV_FORMS:
        assert f'conv1d_causal_kernel<{nt}, {str(down).lower()}>' in src
    for ni in LSTM_FORMS:
        assert f'lstm_step_kernel<{ni}>' in src
    for ns in RVQ_FORMS:
        assert f'rvq_encode_kernel<{ns}>' in src
    # the rules restated in tests/codec_rules.py, as the source writes them
    assert src.count('const int nt = C_out > 64 ? 4 : C_out > 32 ? 2 : 1;') == 2
    assert 'const int ni = (H + 255) / 256;' in src
    assert re.search(r'if \(D <= 32\)\s+hipLaunchKernelGGL\(rvq_encode_kernel<4>', src)
    assert re.search(r'else if \(D <= 64\)\s+hipLaunchKernelGGL\(rvq_encode_kernel<8>', src)
