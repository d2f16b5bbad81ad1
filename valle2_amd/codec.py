"""The 24 kHz EnCodec family on the device, fp32, in the kernels of csrc/codec.hip.  DECODER: codes `(Q, T)` -> waveform
`(hop T,)` (vh_rvq_decode, vh_conv1d_causal, vh_lstm_layer); `EncodecDecoder` drops into `codec_io.synthesize*` as the `codec=`
object: the codes never leave the GPU and neither does the waveform.  ENCODER: waveform `(L,)` -> codes `(Q, ceil(L / hop))`
(vh_conv1d_wave, vh_conv1d_down, vh_rvq_encode over the decoder's stride-1 convolution and LSTM): `EncodecEncoder`, and
`EncodecCodec`, both halves as one `codec=` object, so that a request can be (text, prompt waveform).

What is here: the residual vector quantiser's decode and the causal SEANet decoder (first convolution, a 2-layer LSTM with its
skip, per ratio a transposed convolution and residual blocks, the last convolution), weights taken from a state dict in the
key layout of `transformers`' EncodecModel; and the mirror image, the causal SEANet encoder (first convolution over the raw
waveform, per ratio residual blocks and a strided convolution with the reference's right-hand "extra" reflect padding, the
LSTM, the last convolution) followed by the quantiser's encode (nearest entry per stage, all stages in one launch).  What is
not: the non-causal 48 kHz model, `normalize=True`, chunking, 16-bit arithmetic, streaming, and the `encodec` package's own
checkpoint names.  Parity is pinned against float64 restatements on RANDOM weights (tests/codec_mirror.py,
tests/codec_enc_mirror.py, tests/golden/codec_small.npz, tests/golden/codec_enc_small.npz); no trained checkpoint has been run
through either half.

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


def _check_arch(arch: dict, who: str = 'EncodecDecoder') -> dict:
    unknown = sorted(set(arch) - set(ARCH_DEFAULTS))
    if unknown:
        raise ValueError(f'{who}: unknown architecture field(s) {unknown}')
    a = dict(ARCH_DEFAULTS, **arch)
    for name, want in _FAMILY.items():
        if a[name] != want:
            raise ValueError(f'{who}: {name}={a[name]!r} is outside the causal 24 kHz family served here ({name}={want!r})')
    a['upsampling_ratios'] = tuple(int(r) for r in a['upsampling_ratios'])
    ints = ('num_filters', 'hidden_size', 'num_residual_layers', 'kernel_size', 'last_kernel_size', 'residual_kernel_size',
            'dilation_growth_rate', 'num_lstm_layers', 'compress', 'codebook_size', 'sampling_rate')
    for name in ints:
        if not isinstance(a[name], int) or a[name] < (0 if name == 'num_residual_layers' else 1):
            raise ValueError(f'{who}: {name}={a[name]!r} must be a positive integer')
    if not a['upsampling_ratios'] or any(r < 1 for r in a['upsampling_ratios']):
        raise ValueError(f'{who}: upsampling_ratios={a["upsampling_ratios"]!r} must be positive integers')
    # every activation is a (rows, C) matrix whose rows stay on 16-byte boundaries
    if a['hidden_size'] % 4:
        raise ValueError(f'{who}: hidden_size={a["hidden_size"]} is not a multiple of 4 (channel counts must be)')
    width = a['num_filters'] * 2 ** len(a['upsampling_ratios'])
    if width > 1024:
        raise ValueError(f'{who}: num_filters={a["num_filters"]} x 2^{len(a["upsampling_ratios"])} = {width} LSTM units; '
                         'at most 1024 are served')
    for level in range(len(a['upsampling_ratios']) + 1):
        c = width >> level
        if c % 4:
            raise ValueError(f'{who}: num_filters={a["num_filters"]}: the channel count {c} after {level} upsampling '
                             'stage(s) is not a multiple of 4')
    for level in range(len(a['upsampling_ratios']) + 1):
        c = width >> level
        if level and a['num_residual_layers'] and (c % a['compress'] or (c // a['compress']) % 4):
            raise ValueError(f'{who}: compress={a["compress"]}: the residual blocks\' hidden channel count '
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


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def encoder_state_dict_keys(arch: dict) -> dict:
    """The encoder's key mapping, as `state_dict_keys` is the decoder's.  encoder.layers: 0 first convolution, then per ratio
    in REVERSED upsampling_ratios [residual blocks ..., ELU, downsampling convolution], then [LSTM, ELU, last convolution]."""
    p = 'encoder.layers.'
    keys = {'first': p + '0.conv', 'stages': []}
    idx = 1
    for _ in arch['upsampling_ratios']:
        stage = {'blocks': []}
        for _ in range(arch['num_residual_layers']):
            stage['blocks'].append({'conv1': f'{p}{idx}.block.1.conv', 'conv2': f'{p}{idx}.block.3.conv',
                                    'shortcut': f'{p}{idx}.shortcut.conv'})
            idx += 1
        stage['down'] = f'{p}{idx + 1}.conv'
        idx += 2
        keys['stages'].append(stage)
    keys['lstm'] = [{n: f'{p}{idx}.lstm.{n}_l{layer}' for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')}
                    for layer in range(arch['num_lstm_layers'])]
    keys['last'] = f'{p}{idx + 2}.conv'
    return keys


def _lstm_weights(sd, names, width):
    w_ih, w_hh = _get(sd, names['weight_ih']).double(), _get(sd, names['weight_hh']).double()
    bias = _get(sd, names['bias_ih']).double() + _get(sd, names['bias_hh']).double()
    _expect(names['weight_ih'], w_ih, (4 * width, width))
    _expect(names['weight_hh'], w_hh, (4 * width, width))
    _expect(names['bias_ih'], bias, (4 * width,))
    return w_ih[:, None, :].contiguous().float(), bias.float(), w_hh.contiguous().float()


def _codebooks(sd, a):
    books = []
    while codebook_key(len(books)) in sd:
        books.append(_get(sd, codebook_key(len(books))))
    if not books:
        raise KeyError(f'EncodecDecoder: the state dict has no {codebook_key(0)!r}')
    for q, t in enumerate(books):
        _expect(codebook_key(q), t, (a['codebook_size'], a['hidden_size']))
    return torch.stack([t.float() for t in books]).contiguous()


class EncodecEncoder:
    """waveform -> codes for the causal 24 kHz EnCodec family, on the HIP device the waveform lives on: `transformers`'
    EncodecModel.encoder followed by quantizer.encode, in the kernels of csrc/codec.hip."""
    RVQ_MAX_D, RVQ_MAX_K = 128, 16384           # what vh_rvq_encode serves

    def __init__(self, arch: dict, weights: dict):
        self.arch = arch
        self._host = weights            # fp32, on the host, in the kernels' layouts
        self._dev = {}
        self.ratios = tuple(reversed(arch['upsampling_ratios']))      # the order the encoder downsamples in
        self.hop = 1
        for r in self.ratios:
            self.hop *= r

    @classmethod
    def from_state_dict(cls, sd, **arch) -> 'EncodecEncoder':
        """Build from a state dict in `transformers`' EncodecModel key layout (`encoder_state_dict_keys`, `codebook_key`) and
        the architecture numbers (`ARCH_DEFAULTS`), under the decoder's rules: no device work, an architecture outside the
        family is a ValueError naming the field, a missing tensor a KeyError naming the key."""
        a = _check_arch(arch, 'EncodecEncoder')
        if a['hidden_size'] > cls.RVQ_MAX_D or a['codebook_size'] > cls.RVQ_MAX_K:
            raise ValueError(f'EncodecEncoder: hidden_size={a["hidden_size"]} / codebook_size={a["codebook_size"]}: the quantiser '
                             f'encodes up to hidden_size {cls.RVQ_MAX_D} and codebook_size {cls.RVQ_MAX_K}')
        for r in a['upsampling_ratios']:
            if 2 * r > 64:
                raise ValueError(f'EncodecEncoder: upsampling_ratios={a["upsampling_ratios"]!r}: a downsampling convolution has '
                                 f'2 x ratio taps, at most 64 are served')
        keys = encoder_state_dict_keys(a)
        c = a['num_filters']
        w0, b0 = _conv(sd, keys['first'], 1, c, a['kernel_size'])
        w = {'first': (w0.reshape(c, a['kernel_size']).contiguous(), b0), 'stages': [], 'lstm': []}
        for ratio, stage in zip(reversed(a['upsampling_ratios']), keys['stages']):
            blocks = []
            for j, names in enumerate(stage['blocks']):
                hid = c // a['compress']
                blocks.append({'dilation': a['dilation_growth_rate'] ** j,
                               'conv1': _conv(sd, names['conv1'], c, hid, a['residual_kernel_size']),
                               'conv2': _conv(sd, names['conv2'], hid, c, 1),
                               'shortcut': _conv(sd, names['shortcut'], c, c, 1)})
            w['stages'].append({'blocks': blocks, 'down': _conv(sd, stage['down'], c, 2 * c, 2 * ratio)})
            c *= 2
        for names in keys['lstm']:
            w['lstm'].append(_lstm_weights(sd, names, c))
        w['last'] = _conv(sd, keys['last'], c, a['hidden_size'], a['last_kernel_size'])
        w['codebooks'] = _codebooks(sd, a)
        # |e|^2 of every entry in float64, stored as fp32: the quantiser's score is 2 r.e - |e|^2
        w['e_sq'] = w['codebooks'].double().pow(2).sum(-1).float().contiguous()
        return cls(a, w)

    @property
    def sampling_rate(self) -> int:
        return self.arch['sampling_rate']

    @property
    def num_codebooks(self) -> int:
        return int(self._host['codebooks'].shape[0])

    def frames(self, n_samples: int) -> int:
        """The frame count of n_samples: every downsampling stage takes the ceiling, which is ceil(n_samples / hop)."""
        return -(-int(n_samples) // self.hop)

    # ---- checks, all before any device work ---------------------------------------------------------------------------
    def _check_wave(self, wave, name, rank):
        if not isinstance(wave, Tensor) or not wave.is_floating_point():
            raise ValueError(f'{name}: a floating-point waveform tensor is expected, got '
                             f'{wave.dtype if isinstance(wave, Tensor) else type(wave)}')
        if wave.dim() != rank:
            raise ValueError(f'{name}: expected a {rank}-D waveform {"(B, L)" if rank == 2 else "(L,)"} (mono), got {tuple(wave.shape)}')
        if wave.numel() == 0:
            raise ValueError(f'{name}: an empty waveform {tuple(wave.shape)}')
        return wave

    def _check_q(self, num_codebooks):
        if num_codebooks is None:
            return self.num_codebooks
        if not isinstance(num_codebooks, int) or isinstance(num_codebooks, bool) or not 1 <= num_codebooks <= self.num_codebooks:
            raise ValueError(f'num_codebooks={num_codebooks!r}: the encoder holds {self.num_codebooks} codebooks (1 .. {self.num_codebooks})')
        return num_codebooks

    def _on_device(self, wave):
        if not wave.is_cuda:
            raise _lib.VhError(f'EncodecEncoder: the waveform is on {wave.device}; the encoder runs on a HIP device and there is '
                               'no CPU fallback')
        return wave.float().contiguous()

    # ---- what EncodecPip offers on the encode side --------------------------------------------------------------------
    @torch.inference_mode()
    def embed(self, wave: Tensor) -> Tensor:
        """waveform (L,) -> the encoder's output (T, hidden_size), T = ceil(L / hop): what the quantiser sees."""
        return self._embed(self._on_device(self._check_wave(wave, 'wave', 1))[None])[0]

    @torch.inference_mode()
    def encode(self, wave: Tensor, num_codebooks=None) -> Tensor:
        """waveform (L,) -> codes (Q, T) int64, T = ceil(L / hop); Q = num_codebooks, or every codebook held."""
        self._check_wave(wave, 'wave', 1)
        Q = self._check_q(num_codebooks)
        return self._quantise(self._embed(self._on_device(wave)[None]), Q)[0]

    @torch.inference_mode()
    def batch_encode(self, waves: Tensor, num_codebooks=None) -> Tensor:
        """waveforms (B, L) of one length -> codes (B, Q, T)."""
        self._check_wave(waves, 'waves', 2)
        Q = self._check_q(num_codebooks)
        return self._quantise(self._embed(self._on_device(waves)), Q)

    @torch.inference_mode()
    def encode_many(self, waves, num_codebooks=None, return_embeddings=False):
        """[waveform (L_b,)] -> [codes (Q, T_b)]: one right-padded batch; every level's valid lengths are computed on the host
        and uploaded once, and each utterance's codes (and embeddings (T_b, hidden_size), with return_embeddings) are bit for
        bit what `encode` / `embed` give for it alone."""
        waves = list(waves)
        Q = self._check_q(num_codebooks)
        if not waves:
            return ([], []) if return_embeddings else []
        for i, wv in enumerate(waves):
            self._check_wave(wv, f'waves[{i}]', 1)
            if wv.device != waves[0].device:
                raise ValueError(f'waves[{i}] is on {wv.device}, waves[0] on {waves[0].device}')
        dev = waves[0].device
        if dev.type != 'cuda':
            self._on_device(waves[0])
        lengths = [int(wv.shape[0]) for wv in waves]
        L = max(lengths)
        batch = torch.zeros(len(waves), L, device=dev, dtype=torch.float32)
        for i, wv in enumerate(waves):
            batch[i, :lengths[i]] = wv
        lens = None
        if any(n != L for n in lengths):
            levels = [lengths]
            for r in self.ratios:
                levels.append([-(-n // r) for n in levels[-1]])
            lens = _lib.to_device_async(torch.tensor(levels, dtype=torch.int32), dev)         # (levels, B), one upload
        emb = self._embed(batch, lens)
        codes = self._quantise(emb, Q)
        frames = [self.frames(n) for n in lengths]
        out = [codes[i, :, :t] for i, t in enumerate(frames)]
        return (out, [emb[i, :t] for i, t in enumerate(frames)]) if return_embeddings else out

    # ---- the device side ----------------------------------------------------------------------------------------------
    _weights = EncodecDecoder._weights

    def _embed(self, wave: Tensor, lens=None) -> Tensor:
        """wave (B, L) fp32 on the device -> (B, T, hidden_size); lens (levels, B) int32 on the device, or None."""
        from . import kernels as K
        w = self._weights(wave.device)
        level = 0
        at = (lambda i: None) if lens is None else (lambda i: lens[i])
        x = K.conv1d_wave(wave, *w['first'], lens=at(0))
        for ratio, stage in zip(self.ratios, w['stages']):
            for blk in stage['blocks']:
                y = K.conv1d_causal(x, *blk['conv1'], dilation=blk['dilation'], elu=True, lens=at(level))
                y = K.conv1d_causal(y, *blk['conv2'], elu=True)
                x = K.conv1d_causal(x, *blk['shortcut'], residual=y)
            x = K.conv1d_down(x, *stage['down'], stride=ratio, elu=True, lens=at(level))
            level += 1
        h = x
        for layer, (w_ih, bias, w_hh) in enumerate(w['lstm']):
            last = layer == len(w['lstm']) - 1
            h = K.lstm_layer(K.conv1d_causal(h, w_ih, bias), w_hh, skip=x if last else None)
        return K.conv1d_causal(h, *w['last'], elu=True, lens=at(level))

    def _quantise(self, emb: Tensor, Q: int) -> Tensor:
        from . import kernels as K
        w = self._weights(emb.device)
        return K.rvq_encode(emb, w['codebooks'], w['e_sq'], Q)


class EncodecCodec:
    """Both halves: the `codec=` object of `codec_io.synthesize*` for waveform prompts — `encode` on the prompt, `decode` on
    the synthesised codes, nothing leaving the device."""

    def __init__(self, encoder: EncodecEncoder, decoder: EncodecDecoder):
        if encoder.hop != decoder.hop or encoder.num_codebooks != decoder.num_codebooks or \
                encoder.arch['codebook_size'] != decoder.arch['codebook_size'] or encoder.sampling_rate != decoder.sampling_rate:
            raise ValueError(f'EncodecCodec: the encoder (hop {encoder.hop}, {encoder.num_codebooks} codebooks of '
                             f'{encoder.arch["codebook_size"]}) and the decoder (hop {decoder.hop}, {decoder.num_codebooks} of '
                             f'{decoder.arch["codebook_size"]}) are not two halves of one codec')
        self.encoder, self.decoder = encoder, decoder

    @classmethod
    def from_state_dict(cls, sd, **arch) -> 'EncodecCodec':
        return cls(EncodecEncoder.from_state_dict(sd, **arch), EncodecDecoder.from_state_dict(sd, **arch))

    @property
    def sampling_rate(self) -> int:
        return self.decoder.sampling_rate

    @property
    def num_codebooks(self) -> int:
        return self.decoder.num_codebooks

    @property
    def hop(self) -> int:
        return self.decoder.hop

    def encode(self, wave, num_codebooks=None):
        return self.encoder.encode(wave, num_codebooks)

    def batch_encode(self, waves, num_codebooks=None):
        return self.encoder.batch_encode(waves, num_codebooks)

    def encode_many(self, waves, num_codebooks=None):
        return self.encoder.encode_many(waves, num_codebooks)

    def get_embedding(self, wave):
        """waveform (L,) -> the encoder's output in the reference's layout (hidden_size, T)."""
        return self.encoder.embed(wave).t()

    def decode(self, codes):
        return self.decoder.decode(codes)

    def batch_decode(self, codes):
        return self.decoder.batch_decode(codes)

    def decode_many(self, codes_list):
        return self.decoder.decode_many(codes_list)

    def encode_decode(self, wave, num_codebooks=None):
        """waveform (L,) -> its reconstruction (hop T,), T = ceil(L / hop)."""
        return self.decoder.decode(self.encoder.encode(wave, num_codebooks))
