"""A functional restatement of the 24 kHz EnCodec ENCODER (causal SEANet encoder + the residual vector quantiser's encode) from
the state dict of `transformers`' EncodecModel, beside tests/codec_mirror.py (the decoder): plain torch on the CPU, float64 by
default, the same operations in fp32 with `dtype=torch.float32`.  It does not import `transformers`;
tests/golden/codec_enc_small.npz pins it to that model and tests/test_codec_enc_cpu.py to a live one where the package is
installed.  Layout here is torch's (B, C, T); the kernels' is channels-last.

The quantiser's score of entry k for a residual r is 2 r.e_k - |e_k|^2 — the reference's -(|r|^2 - 2 r.e + |e|^2) without the
term every entry shares — and `rvq_scores` walks the stages along the FLOAT64 codes, which is what the code rules of the device
tests need: per frame the smallest float64 margin between the best and the second-best score, and e_score, the largest
|score_fp32 - score_fp64| when both start from their own input (x32, x64) and subtract the same entries."""
import torch
import torch.nn.functional as F

from tests.codec_mirror import arch_of, conv1d_causal, folded, hop_of, lstm_layer, random_state_dict  # noqa: F401


def random_encoder_state_dict(seed=0, n_codebooks=8, **over):
    """A seeded state dict of the encoder and the codebooks in `transformers`' key layout: direction tensors v ~ N(0, 1), gains
    g = ||v|| sqrt(2 / fan_in) u with u in [0.8, 1.2] (activations, and the embeddings the N(0, 1) codebooks quantise, stay
    O(1); the reference's default init gives embeddings of about 0.1, which every entry is equally far from), LSTM weights
    uniform in +-1 / sqrt(H), codebook entries N(0, 1)."""
    a = arch_of(**over)
    gen = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(prefix, shape, fan_in, gain=2.0):
        v = torch.randn(shape, generator=gen)
        norm = v.pow(2).sum((1, 2), keepdim=True).sqrt()
        sd[prefix + '.parametrizations.weight.original0'] = norm * (gain / fan_in) ** 0.5 * (0.8 + 0.4 * torch.rand(norm.shape, generator=gen))
        sd[prefix + '.parametrizations.weight.original1'] = v
        sd[prefix + '.bias'] = 0.1 * torch.randn(shape[0], generator=gen)

    p = 'encoder.layers.'
    c = a['num_filters']
    conv(p + '0.conv', (c, 1, a['kernel_size']), a['kernel_size'])
    idx = 1
    for ratio in reversed(a['upsampling_ratios']):
        for _ in range(a['num_residual_layers']):
            hid = c // a['compress']
            conv(f'{p}{idx}.block.1.conv', (hid, c, a['residual_kernel_size']), c * a['residual_kernel_size'])
            conv(f'{p}{idx}.block.3.conv', (c, hid, 1), hid, gain=1.0)       # the block's two branches add: half the
            conv(f'{p}{idx}.shortcut.conv', (c, c, 1), c, gain=0.5)          # variance each (the shortcut sees no ELU)
            idx += 1
        conv(f'{p}{idx + 1}.conv', (2 * c, c, 2 * ratio), c * 2 * ratio)
        idx += 2
        c *= 2
    for layer in range(a['num_lstm_layers']):
        for n, shape in (('weight_ih', (4 * c, c)), ('weight_hh', (4 * c, c)), ('bias_ih', (4 * c,)), ('bias_hh', (4 * c,))):
            sd[f'{p}{idx}.lstm.{n}_l{layer}'] = (2 * torch.rand(shape, generator=gen) - 1) / c ** 0.5
    conv(f'{p}{idx + 2}.conv', (a['hidden_size'], c, a['last_kernel_size']), c * a['last_kernel_size'])
    for q in range(n_codebooks):
        sd[f'quantizer.layers.{q}.codebook.embed'] = torch.randn(a['codebook_size'], a['hidden_size'], generator=gen)
    return sd


def pad_causal(x, left, right):
    """EncodecConv1d._pad1d with paddings (left, right), reflect: the small-input branch zero-extends to max(left, right) + 1
    samples, reflects, and cuts the extension off the END of the padded signal."""
    if left == 0 and right == 0:
        return x
    T = x.shape[-1]
    mx = max(left, right)
    extra = mx - T + 1 if T <= mx else 0
    if extra:
        x = F.pad(x, (0, extra))
    x = F.pad(x, (left, right), mode='reflect')
    return x[..., :x.shape[-1] - extra]


def conv1d_down(x, w, b, stride, elu=False):
    """x (B, C_in, T), w (C_out, C_in, K): act -> pad (K - stride, ceil(T / stride) stride - T) -> conv with the stride."""
    if elu:
        x = F.elu(x)
    T = x.shape[-1]
    right = -(-T // stride) * stride - T
    return F.conv1d(pad_causal(x, w.shape[-1] - stride, right), w, b, stride=stride)


def encoder(sd, wave, dtype=torch.float64, **over):
    """wave (B, L) -> (B, hidden_size, ceil(L / hop)): EncodecEncoder.forward."""
    a = arch_of(**over)
    p = 'encoder.layers.'
    x = conv1d_causal(wave.to(dtype)[:, None], *folded(sd, p + '0.conv', dtype))
    idx = 1
    for ratio in reversed(a['upsampling_ratios']):
        for j in range(a['num_residual_layers']):
            d = a['dilation_growth_rate'] ** j
            y = conv1d_causal(x, *folded(sd, f'{p}{idx}.block.1.conv', dtype), dilation=d, elu=True)
            y = conv1d_causal(y, *folded(sd, f'{p}{idx}.block.3.conv', dtype), elu=True)
            x = conv1d_causal(x, *folded(sd, f'{p}{idx}.shortcut.conv', dtype), residual=y)
            idx += 1
        x = conv1d_down(x, *folded(sd, f'{p}{idx + 1}.conv', dtype), stride=ratio, elu=True)
        idx += 2
    y = x.permute(2, 0, 1)
    h = y
    for layer in range(a['num_lstm_layers']):
        h = lstm_layer(h, *[sd[f'{p}{idx}.lstm.{n}_l{layer}'].double().to(dtype) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')])
    x = (h + y).permute(1, 2, 0)
    return conv1d_causal(x, *folded(sd, f'{p}{idx + 2}.conv', dtype), elu=True)


def frames_of(L, arch):
    """The frame count of L samples: every downsampling stage takes the ceiling."""
    for ratio in reversed(arch['upsampling_ratios']):
        L = -(-L // ratio)
    return L


def codebooks_of(sd, dtype=torch.float64):
    books = []
    while f'quantizer.layers.{len(books)}.codebook.embed' in sd:
        books.append(sd[f'quantizer.layers.{len(books)}.codebook.embed'].double().to(dtype))
    return torch.stack(books)


def scores(r, e):
    """r (rows, D), e (K, D) -> (rows, K): 2 r.e - |e|^2 in the operands' dtype."""
    return 2 * (r @ e.t()) - e.pow(2).sum(1)


def rvq_encode(books, x, Q=None):
    """books (n_books, K, D), x (rows, D), same dtype -> codes (Q, rows): the reference's residual quantiser, the first index
    of a maximum."""
    r = x
    out = []
    for q in range(books.shape[0] if Q is None else Q):
        idx = scores(r, books[q]).max(dim=-1).indices
        r = r - F.embedding(idx, books[q])
        out.append(idx)
    return torch.stack(out)


def rvq_scores(books64, x64, x32, Q=None):
    """The stages walked along the FLOAT64 codes -> (codes64 (Q, rows), margin (rows,), e_score): margin is per row the
    smallest float64 gap between the best and the second-best score over the stages (inf where K = 1); e_score the largest
    |score_fp32 - score_fp64|, the fp32 side starting from x32 and subtracting the same entries in fp32."""
    books32 = books64.float()
    r64, r32 = x64, x32
    codes, margin, e_score = [], torch.full((x64.shape[0],), float('inf'), dtype=torch.float64), 0.0
    for q in range(books64.shape[0] if Q is None else Q):
        s64 = scores(r64, books64[q])
        s32 = scores(r32, books32[q])
        e_score = max(e_score, (s32.double() - s64).abs().max().item())
        top = s64.topk(min(2, s64.shape[1]), dim=-1)
        if s64.shape[1] > 1:
            margin = torch.minimum(margin, top.values[:, 0] - top.values[:, 1])
        idx = s64.max(dim=-1).indices
        codes.append(idx)
        r64 = r64 - F.embedding(idx, books64[q])
        r32 = r32 - F.embedding(idx, books32[q])
    return torch.stack(codes), margin, e_score


def chosen_gaps(books64, x64, codes):
    """codes (Q, rows), anyone's: per stage and row the float64 maximum score minus the chosen entry's float64 score, the
    float64 residual rebuilt from those codes' own earlier entries -> (Q, rows), >= 0."""
    r = x64
    gaps = []
    for q in range(codes.shape[0]):
        s = scores(r, books64[q])
        gaps.append(s.max(dim=-1).values - s.gather(1, codes[q][:, None])[:, 0])
        r = r - F.embedding(codes[q], books64[q])
    return torch.stack(gaps)


def encode(sd, wave, dtype=torch.float64, Q=None, **over):
    """wave (B, L) -> (codes (B, Q, T) int64, embeddings (B, T, D) in `dtype`)."""
    emb = encoder(sd, wave, dtype, **over).transpose(1, 2)
    B, T, D = emb.shape
    codes = rvq_encode(codebooks_of(sd, dtype), emb.reshape(B * T, D), Q)
    return codes.view(-1, B, T).transpose(0, 1).contiguous(), emb
