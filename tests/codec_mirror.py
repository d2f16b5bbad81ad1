"""A functional restatement of the 24 kHz EnCodec decoder (residual vector quantiser decode + causal SEANet decoder) from the
state dict of `transformers`' EncodecModel: plain torch on the CPU, float64 by default (`dtype=torch.float32` runs the same
operations in fp32: the error of the reference's own arithmetic, e_ref, is the distance between the two).  It does not import
`transformers`; tests/golden/codec_small.npz pins it to that model and tests/test_codec_cpu.py to a live one where the package
is installed.  Layout here is torch's (B, C, T); the kernels' is channels-last."""
import torch
import torch.nn.functional as F

ARCH = dict(num_filters=32, upsampling_ratios=(8, 5, 4, 2), hidden_size=128, num_residual_layers=1, kernel_size=7,
            last_kernel_size=7, residual_kernel_size=3, dilation_growth_rate=2, num_lstm_layers=2, compress=2,
            codebook_size=1024)


def arch_of(**over):
    unknown = set(over) - set(ARCH)
    assert not unknown, unknown
    a = dict(ARCH, **over)
    a['upsampling_ratios'] = tuple(a['upsampling_ratios'])
    return a


def hop_of(arch):
    h = 1
    for r in arch['upsampling_ratios']:
        h *= r
    return h


def random_state_dict(seed=0, n_codebooks=8, **over):
    """A seeded state dict of the architecture in `transformers`' key layout (no `transformers` needed): direction tensors
    v ~ N(0, 1), gains g = ||v|| sqrt(2 / fan_in) u with u in [0.8, 1.2] (activations stay O(1) through the stack), LSTM
    weights uniform in +-1 / sqrt(H) as nn.LSTM draws them, codebook entries N(0, 1)."""
    a = arch_of(**over)
    gen = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(prefix, shape, fan_in):
        v = torch.randn(shape, generator=gen)
        norm = v.pow(2).sum((1, 2), keepdim=True).sqrt()
        sd[prefix + '.parametrizations.weight.original0'] = norm * (2.0 / fan_in) ** 0.5 * (0.8 + 0.4 * torch.rand(norm.shape, generator=gen))
        sd[prefix + '.parametrizations.weight.original1'] = v
        n_out = shape[1] if 'transpose' in prefix else shape[0]
        sd[prefix + '.bias'] = 0.1 * torch.randn(n_out, generator=gen)

    p = 'decoder.layers.'
    c = a['num_filters'] * 2 ** len(a['upsampling_ratios'])
    conv(p + '0.conv', (c, a['hidden_size'], a['kernel_size']), a['hidden_size'] * a['kernel_size'])
    for layer in range(a['num_lstm_layers']):
        for n, shape in (('weight_ih', (4 * c, c)), ('weight_hh', (4 * c, c)), ('bias_ih', (4 * c,)), ('bias_hh', (4 * c,))):
            sd[f'{p}1.lstm.{n}_l{layer}'] = (2 * torch.rand(shape, generator=gen) - 1) / c ** 0.5
    idx = 2
    for ratio in a['upsampling_ratios']:
        key = f'{p}{idx + 1}.conv'
        conv(key + '<transpose>', (c, c // 2, 2 * ratio), 2 * c)
        for suffix in ('.parametrizations.weight.original0', '.parametrizations.weight.original1', '.bias'):
            sd[key + suffix] = sd.pop(key + '<transpose>' + suffix)
        c //= 2
        idx += 2
        for _ in range(a['num_residual_layers']):
            hid = c // a['compress']
            conv(f'{p}{idx}.block.1.conv', (hid, c, a['residual_kernel_size']), c * a['residual_kernel_size'])
            conv(f'{p}{idx}.block.3.conv', (c, hid, 1), hid)
            conv(f'{p}{idx}.shortcut.conv', (c, c, 1), c)
            idx += 1
    conv(f'{p}{idx + 1}.conv', (1, c, a['last_kernel_size']), c * a['last_kernel_size'])
    for q in range(n_codebooks):
        sd[f'quantizer.layers.{q}.codebook.embed'] = torch.randn(a['codebook_size'], a['hidden_size'], generator=gen)
    return sd


def folded(sd, prefix, dtype):
    """weight = g v / ||v||, the norm over every dimension in which g has extent 1 (torch's weight_norm, dim 0), in float64."""
    g = sd[prefix + '.parametrizations.weight.original0'].double()
    v = sd[prefix + '.parametrizations.weight.original1'].double()
    dims = tuple(d for d in range(v.dim()) if g.shape[d] == 1)
    w = g * v / v.pow(2).sum(dims, keepdim=True).sqrt()
    return w.to(dtype), sd[prefix + '.bias'].double().to(dtype)


def pad_left(x, pad, mode):
    """EncodecConv1d._pad1d with paddings (pad, 0): reflect, with the small-input branch, or zeros."""
    if pad == 0:
        return x
    if mode != 'reflect':
        return F.pad(x, (pad, 0))
    T = x.shape[-1]
    extra = pad - T + 1 if T <= pad else 0
    if extra:
        x = F.pad(x, (0, extra))
    x = F.pad(x, (pad, 0), mode='reflect')
    return x[..., :x.shape[-1] - extra]


def conv1d_causal(x, w, b, dilation=1, mode='reflect', elu=False, residual=None):
    """x (B, C_in, T), w (C_out, C_in, K): act -> left pad (K - 1) dilation -> conv (+ residual)."""
    if elu:
        x = F.elu(x)
    y = F.conv1d(pad_left(x, (w.shape[-1] - 1) * dilation, mode), w, b, dilation=dilation)
    return y if residual is None else y + residual


def conv_transpose1d_causal(x, w, b, stride, elu=False):
    """x (B, C_in, T), w (C_in, C_out, 2 stride): act -> transposed conv -> trim kernel - stride samples on the right."""
    if elu:
        x = F.elu(x)
    y = F.conv_transpose1d(x, w, b, stride=stride)
    return y[..., :y.shape[-1] - (w.shape[-1] - stride)]


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh):
    """x (T, B, H) -> h (T, B, H): one nn.LSTM layer, zero initial state, gate order i, f, g, o."""
    T, B, H = x.shape
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    pre = x @ w_ih.t() + (b_ih + b_hh)
    out = []
    for t in range(T):
        i, f, g, o = (pre[t] + h @ w_hh.t()).split(H, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out)


def rvq_decode(sd, codes, dtype):
    """codes (B, Q, T) -> (B, D, T): the embeddings added in codebook order from a scalar 0.0, as the reference does."""
    out = torch.zeros((), dtype=dtype)
    for q in range(codes.shape[1]):
        out = out + F.embedding(codes[:, q], sd[f'quantizer.layers.{q}.codebook.embed'].double().to(dtype))
    return out.transpose(1, 2)


def decoder(sd, x, dtype, **over):
    """x (B, hidden_size, T) -> (B, 1, hop T): EncodecDecoder.forward."""
    a = arch_of(**over)
    p = 'decoder.layers.'
    x = conv1d_causal(x, *folded(sd, p + '0.conv', dtype))
    y = x.permute(2, 0, 1)
    h = y
    for layer in range(a['num_lstm_layers']):
        h = lstm_layer(h, *[sd[f'{p}1.lstm.{n}_l{layer}'].double().to(dtype) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')])
    x = (h + y).permute(1, 2, 0)
    idx = 2
    for ratio in a['upsampling_ratios']:
        x = conv_transpose1d_causal(x, *folded(sd, f'{p}{idx + 1}.conv', dtype), stride=ratio, elu=True)
        idx += 2
        for j in range(a['num_residual_layers']):
            d = a['dilation_growth_rate'] ** j
            y = conv1d_causal(x, *folded(sd, f'{p}{idx}.block.1.conv', dtype), dilation=d, elu=True)
            y = conv1d_causal(y, *folded(sd, f'{p}{idx}.block.3.conv', dtype), elu=True)
            x = conv1d_causal(x, *folded(sd, f'{p}{idx}.shortcut.conv', dtype), residual=y)
            idx += 1
    return conv1d_causal(x, *folded(sd, f'{p}{idx + 1}.conv', dtype), elu=True)


def decode(sd, codes, dtype=torch.float64, **over):
    """codes (B, Q, T) int64 -> waveform (B, hop T) in `dtype`."""
    return decoder(sd, rvq_decode(sd, codes, dtype), dtype, **over)[:, 0]
