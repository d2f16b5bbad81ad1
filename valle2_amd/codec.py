"""The DECODER half of the 24 kHz EnCodec family on the device: codes `(Q, T)` -> waveform `(hop T,)`, fp32, in the kernels of
csrc/codec.hip (vh_rvq_decode, vh_conv1d_causal, vh_lstm_layer).  `EncodecDecoder` drops into `codec_io.synthesize*` as the
`codec=` object: the codes never leave the GPU and neither does the waveform.

What is here: the residual vector quantiser's decode and the causal SEANet decoder (first convolution, a 2-layer LSTM with its
skip, per ratio a transposed convolution and residual blocks, the last convolution), weights taken from a state dict in the
key layout of `transformers`' EncodecModel.  What is not: the encoder and RVQ encode (there is no `encode`: prompts come as
codes), the non-causal 48 kHz model, 16-bit arithmetic, streaming, and the `encodec` package's own checkpoint names.  Parity
is pinned against a float64 restatement on RANDOM weights (tests/codec_mirror.py, tests/golden/codec_small.npz); no trained
checkpoint has been run through it.

The decoder is causal — reflect padding on the left only, a one-directional LSTM, transposed convolutions trimmed on the right —
so a ragged batch is right-padded, decoded once and trimmed (`decode_many`), bit for bit what each utterance gives alone.  One
thing is not causal: the reflect padding at the START of an utterance reads forward (xpad[i] = x[pad - i]), so an utterance
shorter than a convolution's padding must not see the batch's padding frames; `decode_many` hands the kernels every
utterance's length and the reflection reads zero beyond it, which is the reference's small-input branch for that utterance."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib

ARCH_DEFAULTS = dict(
    num_filters=32, upsampling_ratios=(8, 5, 4, 2), hidden_size=128, num_residual_layers=1, kernel_size=7, last_kernel_size=7,
    residual_kernel_size=3, dilation_growth_rate=2, num_lstm_layers=2, compress=2, codebook_size=1024,
    # the fields that select another family: only these values are served
    use_causal_conv=True, norm_type='weight_norm', pad_mode='reflect', trim_right_ratio=1.0, audio_channels=1, normalize=False,
    chunk_length_s=None, use_conv_shortcut=True, sampling_rate=24000)
_FAMILY = dict(use_causal_conv=True, norm_type='weight_norm', pad_mode='reflect', trim_right_ratio=1.0, audio_channels=1,
               normalize=False, chunk_length_s=None, use_conv_shortcut=True)


def _check_arch(arch: dict) -> dict:
    unknown = sorted(set(arch) - set(ARCH_DEFAULTS))
    if unknown:
        raise ValueError(f'EncodecDecoder: unknown architecture field(s) {unknown}')
    a = dict(ARCH_DEFAULTS, **arch)
    for name, want in _FAMILY.items():
        if a[name] != want:
            raise ValueError(f'EncodecDecoder: {name}={a[name]!r} is outside the causal 24 kHz family served here ({name}={want!r})')
    a['upsampling_ratios'] = tuple(int(r) for r in a['upsampling_ratios'])
    ints = ('num_filters', 'hidden_size', 'num_residual_layers', 'kernel_size', 'last_kernel_size', 'residual_kernel_size',
            'dilation_growth_rate', 'num_lstm_layers', 'compress', 'codebook_size', 'sampling_rate')
    for name in ints:
        if not isinstance(a[name], int) or a[name] < (0 if name == 'num_residual_layers' else 1):
            raise ValueError(f'EncodecDecoder: {name}={a[name]!r} must be a positive integer')
    if not a['upsampling_ratios'] or any(r < 1 for r in a['upsampling_ratios']):
        raise ValueError(f'EncodecDecoder: upsampling_ratios={a["upsampling_ratios"]!r} must be positive integers')
    # every activation is a (rows, C) matrix whose rows stay on 16-byte boundaries
    if a['hidden_size'] % 4:
        raise ValueError(f'EncodecDecoder: hidden_size={a["hidden_size"]} is not a multiple of 4 (channel counts must be)')
    width = a['num_filters'] * 2 ** len(a['upsampling_ratios'])
    if width > 1024:
        raise ValueError(f'EncodecDecoder: num_filters={a["num_filters"]} x 2^{len(a["upsampling_ratios"])} = {width} LSTM units; '
                         'at most 1024 are served')
    for level in range(len(a['upsampling_ratios']) + 1):
        c = width >> level
        if c % 4:
            raise ValueError(f'EncodecDecoder: num_filters={a["num_filters"]}: the channel count {c} after {level} upsampling '
                             'stage(s) is not a multiple of 4')
    for level in range(len(a['upsampling_ratios']) + 1):
        c = width >> level
        if level and a['num_residual_layers'] and (c % a['compress'] or (c // a['compress']) % 4):
            raise ValueError(f'EncodecDecoder: compress={a["compress"]}: the residual blocks\' hidden channel count '
                             f'{c}/{a["compress"]} is not a multiple of 4')
    return a


def state_dict_keys(arch: dict) -> dict:
    """THE key mapping: role -> prefix (a convolution), key (a tensor) or list, in the layout of `transformers`'
    EncodecModel.state_dict().  decoder.layers: 0 first convolution, 1 LSTM, then per ratio [ELU, transposed convolution,
    residual blocks ...], then [ELU, last convolution]; a residual block is block.[ELU, conv, ELU, conv] + shortcut."""
    p = 'decoder.layers.'
    keys = {'first': p + '0.conv',
            'lstm': [{n: f'{p}1.lstm.{n}_l{layer}' for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')}
                     for layer in range(arch['num_lstm_layers'])],
            'stages': []}
    idx = 2
    for _ in arch['upsampling_ratios']:
        stage = {'up': f'{p}{idx + 1}.conv', 'blocks': []}
        idx += 2
        for _ in range(arch['num_residual_layers']):
            stage['blocks'].append({'conv1': f'{p}{idx}.block.1.conv', 'conv2': f'{p}{idx}.block.3.conv',
                                    'shortcut': f'{p}{idx}.shortcut.conv'})
            idx += 1
        keys['stages'].append(stage)
    keys['last'] = f'{p}{idx + 1}.conv'
    return keys


def codebook_key(q: int) -> str:
    return f'quantizer.layers.{q}.codebook.embed'


def _get(sd, key):
    if key not in sd:
        raise KeyError(f'EncodecDecoder: the state dict has no {key!r} (the key layout of transformers\' EncodecModel is expected)')
    return sd[key].detach().to('cpu')


def _fold(sd, prefix):
    """Weight norm folded in float64: w = g v / ||v||, the norm over every dimension in which g has extent 1."""
    g = _get(sd, prefix + '.parametrizations.weight.original0').double()
    v = _get(sd, prefix + '.parametrizations.weight.original1').double()
    if v.dim() != 3 or g.dim() != 3:
        raise ValueError(f'EncodecDecoder: {prefix}: weight-norm tensors of shapes {tuple(g.shape)} / {tuple(v.shape)}')
    dims = tuple(d for d in range(3) if g.shape[d] == 1)
    return g * v / v.pow(2).sum(dims, keepdim=True).sqrt(), _get(sd, prefix + '.bias').double()


def _expect(name, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'EncodecDecoder: {name} has shape {tuple(t.shape)}, the architecture numbers give {tuple(shape)}')


def _conv(sd, prefix, c_in, c_out, taps):
    """nn.Conv1d (C_out, C_in, taps) -> the kernel's (C_out, taps, C_in), fp32."""
    w, b = _fold(sd, prefix)
    _expect(prefix + ' weight', w, (c_out, c_in, taps))
    _expect(prefix + '.bias', b, (c_out,))
    return w.permute(0, 2, 1).contiguous().float(), b.float()


def _conv_transpose(sd, prefix, c_in, c_out, r):
    """nn.ConvTranspose1d (C_in, C_out, 2 r), stride r, trimmed by r on the right -> a 2-tap window with zero padding over
    N = r C_out columns: w[(p, co), 0, ci] = wt[ci, co, p + r] (the frame before), w[(p, co), 1, ci] = wt[ci, co, p]."""
    w, b = _fold(sd, prefix)
    _expect(prefix + ' weight', w, (c_in, c_out, 2 * r))
    _expect(prefix + '.bias', b, (c_out,))
    taps = torch.stack([w[:, :, r:], w[:, :, :r]])                    # (tap, ci, co, p)
    return taps.permute(3, 2, 0, 1).reshape(r * c_out, 2, c_in).contiguous().float(), b.repeat(r).float()


class EncodecDecoder:
    """codes -> waveform for the causal 24 kHz EnCodec family, on the HIP device the codes live on."""

    def __init__(self, arch: dict, weights: dict):
        self.arch = arch
        self._host = weights            # fp32, on the host, in the kernels' layouts
        self._dev = {}                  # device -> the same on that device
        self.hop = 1
        for r in arch['upsampling_ratios']:
            self.hop *= r

    @classmethod
    def from_state_dict(cls, sd, **arch) -> 'EncodecDecoder':
        """Build from a state dict in `transformers`' EncodecModel key layout (`state_dict_keys`) and the architecture
        numbers (`ARCH_DEFAULTS`: the 24 kHz model).  No device work happens here: an architecture outside the family is a
        ValueError naming the field, a missing tensor a KeyError naming the key."""
        a = _check_arch(arch)
        keys = state_dict_keys(a)
        n_up = len(a['upsampling_ratios'])
        width = a['num_filters'] * 2 ** n_up
        w = {'first': _conv(sd, keys['first'], a['hidden_size'], width, a['kernel_size']), 'lstm': [], 'stages': []}
        for names in keys['lstm']:
            w_ih, w_hh = _get(sd, names['weight_ih']).double(), _get(sd, names['weight_hh']).double()
            bias = _get(sd, names['bias_ih']).double() + _get(sd, names['bias_hh']).double()
            _expect(names['weight_ih'], w_ih, (4 * width, width))
            _expect(names['weight_hh'], w_hh, (4 * width, width))
            _expect(names['bias_ih'], bias, (4 * width,))
            w['lstm'].append((w_ih[:, None, :].contiguous().float(), bias.float(), w_hh.contiguous().float()))
        c = width
        for ratio, stage in zip(a['upsampling_ratios'], keys['stages']):
            blocks = []
            up = _conv_transpose(sd, stage['up'], c, c // 2, ratio)
            c //= 2
            for j, names in enumerate(stage['blocks']):
                hid = c // a['compress']
                blocks.append({'dilation': a['dilation_growth_rate'] ** j,
                               'conv1': _conv(sd, names['conv1'], c, hid, a['residual_kernel_size']),
                               'conv2': _conv(sd, names['conv2'], hid, c, 1),
                               'shortcut': _conv(sd, names['shortcut'], c, c, 1)})
            w['stages'].append({'up': up, 'blocks': blocks})
        w['last'] = _conv(sd, keys['last'], c, 1, a['last_kernel_size'])
        books = []
        while codebook_key(len(books)) in sd:
            books.append(_get(sd, codebook_key(len(books))).float())
        if not books:
            raise KeyError(f'EncodecDecoder: the state dict has no {codebook_key(0)!r}')
        for q, t in enumerate(books):
            _expect(codebook_key(q), t, (a['codebook_size'], a['hidden_size']))
        w['codebooks'] = torch.stack(books).contiguous()
        return cls(a, w)

    # ---- what EncodecPip offers on the decode side --------------------------------------------------------------------
    @property
    def sampling_rate(self) -> int:
        return self.arch['sampling_rate']

    @property
    def num_codebooks(self) -> int:
        return int(self._host['codebooks'].shape[0])

    def validate(self, codes: Tensor, name: str = 'codes', batched: bool = False) -> Tensor:
        """codec_io.validate_codes' checks and messages, against this decoder's codebooks (Q may be smaller than their number)."""
        want = 3 if batched else 2
        if not isinstance(codes, Tensor) or codes.dim() != want:
            raise ValueError(f'{name}: expected a {want}-D tensor in the codec layout {"(B, Q, T)" if batched else "(Q, T)"}, '
                             f'got {tuple(codes.shape) if isinstance(codes, Tensor) else type(codes)}')
        if codes.dtype != torch.int64:
            raise ValueError(f'{name}: codec ids are int64, got {codes.dtype}')
        q = codes.shape[-2]
        if q < 1 or q > self.num_codebooks:
            raise ValueError(f'{name}: {q} codebooks, the decoder holds {self.num_codebooks} '
                             f'(a (T, Q) tensor handed over where (Q, T) is expected?)')
        if codes.shape[-1] < 1 or (batched and codes.shape[0] < 1):
            raise ValueError(f'{name}: no frames to decode in {tuple(codes.shape)}')
        lo, hi = int(codes.min()), int(codes.max())
        if lo < 0 or hi >= self.arch['codebook_size']:
            raise IndexError(f'{name}: ids span [{lo}, {hi}], the codebooks hold {self.arch["codebook_size"]} entries '
                             f'(BOS / EOS never appear inside codec tensors)')
        return codes

    @torch.inference_mode()
    def decode(self, codes: Tensor) -> Tensor:
        """codes (Q, T) -> waveform (hop T,)."""
        return self._run(self.validate(codes)[None])[0]

    @torch.inference_mode()
    def batch_decode(self, codes: Tensor) -> Tensor:
        """codes (B, Q, T) -> waveforms (B, hop T)."""
        return self._run(self.validate(codes, batched=True))

    @torch.inference_mode()
    def decode_many(self, codes_list) -> list:
        """[codes (Q, T_b)] -> [waveform (hop T_b,)]: one right-padded batch, trimmed afterwards.  The decoder is causal, so
        every waveform is bit for bit what `decode` gives for that utterance alone."""
        codes_list = list(codes_list)
        if not codes_list:
            return []
        for i, c in enumerate(codes_list):
            self.validate(c, f'codes[{i}]')
            if c.shape[0] != codes_list[0].shape[0] or c.device != codes_list[0].device:
                raise ValueError(f'codes[{i}]: {c.shape[0]} codebooks on {c.device}, codes[0] has {codes_list[0].shape[0]} on '
                                 f'{codes_list[0].device}')
        T = max(c.shape[1] for c in codes_list)
        batch = codes_list[0].new_zeros(len(codes_list), codes_list[0].shape[0], T)
        for i, c in enumerate(codes_list):
            batch[i, :, :c.shape[1]] = c
        lens = None
        if any(c.shape[1] != T for c in codes_list):
            # the reflect padding at the start of an utterance reads FORWARD: one shorter than the padding must not see the
            # batch's padding frames (vh_conv1d_causal, lens)
            lens = _lib.to_device_async(torch.tensor([c.shape[1] for c in codes_list], dtype=torch.int32), batch.device)
        wave = self._run(batch, lens)
        return [wave[i, :self.hop * c.shape[1]] for i, c in enumerate(codes_list)]

    # ---- the device side ----------------------------------------------------------------------------------------------
    def _weights(self, device):
        key = (device.type, device.index)
        if key not in self._dev:
            def move(o):
                if isinstance(o, Tensor):
                    return o.to(device)
                if isinstance(o, dict):
                    return {k: move(v) for k, v in o.items()}
                if isinstance(o, (list, tuple)):
                    return type(o)(move(v) for v in o)
                return o
            self._dev[key] = move(self._host)
        return self._dev[key]

    def _run(self, codes: Tensor, lens=None) -> Tensor:
        from . import kernels as K
        if not codes.is_cuda:
            raise _lib.VhError(f'EncodecDecoder: codes are on {codes.device}; the decoder runs on a HIP device and there is no '
                               'CPU fallback')
        w = self._weights(codes.device)
        B, Q, T = codes.shape
        x = K.rvq_decode(codes, w['codebooks'])                                             # (B, T, hidden_size)
        x = K.conv1d_causal(x, *w['first'], lens=lens)
        scale = 1
        h = x
        for layer, (w_ih, bias, w_hh) in enumerate(w['lstm']):
            last = layer == len(w['lstm']) - 1
            h = K.lstm_layer(K.conv1d_causal(h, w_ih, bias), w_hh, skip=x if last else None)
        x = h
        for ratio, stage in zip(self.arch['upsampling_ratios'], w['stages']):
            wt, bt = stage['up']
            x = K.conv1d_causal(x, wt, bt, pad_mode=K.PAD_ZERO, elu=True).view(B, x.shape[1] * ratio, wt.shape[0] // ratio)
            scale *= ratio
            for blk in stage['blocks']:
                y = K.conv1d_causal(x, *blk['conv1'], dilation=blk['dilation'], elu=True, lens=lens, len_scale=scale)
                y = K.conv1d_causal(y, *blk['conv2'], elu=True)
                x = K.conv1d_causal(x, *blk['shortcut'], residual=y)
        return K.conv1d_causal(x, *w['last'], elu=True, lens=lens, len_scale=scale).view(B, self.hop * T)
