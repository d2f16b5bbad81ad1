"""Records tests/golden/codec_small.npz from `transformers`' EncodecModel (the 24 kHz architecture: causal SEANet decoder +
residual vector quantiser) at a small configuration with seeded random weights:

    python -m tests.golden.gen_codec_golden

The file holds the model's state dict (decoder and codebooks only, keys prefixed 'sd/'), codes (B 2, Q 4, T 9), the waveform
of the model run in float64 ('wave64') and of the same model in fp32 ('wave32').  num_residual_layers = 2 makes dilation 2
occur.  Needs the `transformers` package; the tests that read the file do not."""
from pathlib import Path

import numpy as np
import torch

SMALL = dict(num_filters=8, upsampling_ratios=(4, 2), hidden_size=32, codebook_size=64, num_residual_layers=2)
SMALL_CODEBOOK_DIM = 32
B, Q, T = 2, 4, 9
OUT = Path(__file__).resolve().parent / 'codec_small.npz'


def build_model(seed=0, **over):
    from transformers import EncodecConfig, EncodecModel
    torch.manual_seed(seed)
    kw = dict(over)
    kw['upsampling_ratios'] = list(kw.get('upsampling_ratios', (8, 5, 4, 2)))
    if 'hidden_size' in kw:
        kw.setdefault('codebook_dim', kw['hidden_size'])
    model = EncodecModel(EncodecConfig(**kw)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                   # the codebooks initialise to zeros: give them entries
        for layer in model.quantizer.layers:
            layer.codebook.embed.copy_(torch.randn(layer.codebook.embed.shape, generator=g))
    return model


def decoder_state_dict(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.startswith('decoder.') or k.endswith('codebook.embed')}


@torch.no_grad()
def model_decode(model, codes):
    """codes (B, Q, T) -> (B, hop T) through EncodecModel.decode."""
    return model.decode(codes[None], [None]).audio_values[:, 0]


def main():
    # hop 8 at 24 kHz is 3000 frames per second of 6 bits: 144 kbps makes the model keep 8 codebooks (Q = 4 of them are decoded)
    model = build_model(0, target_bandwidths=[144.0], **SMALL)
    codes = torch.randint(0, SMALL['codebook_size'], (B, Q, T), generator=torch.Generator().manual_seed(2))
    wave32 = model_decode(model, codes)
    sd = decoder_state_dict(model)
    wave64 = model_decode(model.double(), codes)
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    arrays.update(codes=codes.numpy(), wave64=wave64.numpy(), wave32=wave32.numpy())
    np.savez_compressed(OUT, **arrays)
    print(f'{OUT.name}: {OUT.stat().st_size} bytes, {len(sd)} tensors, max|wave64| = {wave64.abs().max():.3f}, '
          f'max|wave32 - wave64| = {(wave32.double() - wave64).abs().max():.2e}')


if __name__ == '__main__':
    main()
