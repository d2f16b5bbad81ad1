"""Records tests/golden/codec_enc_small.npz from `transformers`' EncodecModel (`encoder` followed by `quantizer.encode`) at the
SMALL configuration of gen_codec_golden.py (hop 8) with seeded weights:

    python -m tests.golden.gen_codec_enc_golden

The live model's encoder is loaded with seeded weights of the mirror's scaling (tests/codec_enc_mirror.random_encoder_state_dict): the
default init gives embeddings of about 0.1 against N(0, 1) codebooks, which every entry is equally far from.  The file holds
the state dict (encoder and codebooks, keys prefixed 'sd/') and, per length L in LENGTHS (B = 2 waveforms each): 'wave/L',
'emb64/L' and 'emb32/L' (B, T, D) — the encoder's output in float64 and of the same model in fp32, channels-last —,
'codes64/L' (B, Q, T) from the float64 model, 'codes32/L' from the fp32 one, and 'margin/L' (B, T): per frame the smallest
float64 score margin (best minus second best, of 2 r.e - |e|^2) over the stages.  Needs `transformers`; the tests that read the
file do not."""
from pathlib import Path

import numpy as np
import torch

from tests import codec_enc_mirror as E
from tests.golden.gen_codec_golden import SMALL, build_model

LENGTHS = (1, 5, 8, 9, 67, 72)
B = 2
OUT = Path(__file__).resolve().parent / 'codec_enc_small.npz'


def encoder_state_dict(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.startswith('encoder.') or k.endswith('codebook.embed')}


def rescale(model, seed):
    """Load the live model's encoder with the mirror's seeded weights (every key must exist there with the same shape)."""
    want = E.random_encoder_state_dict(seed, n_codebooks=len(model.quantizer.layers), **SMALL)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in want.items():
            if k.startswith('encoder.'):
                assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
                sd[k].copy_(v)
    assert not [k for k in sd if k.startswith('encoder.') and k not in want]


@torch.no_grad()
def model_encode(model, wave):
    """wave (B, L) -> (codes (B, Q, T), embeddings (B, T, D)) through model.encoder and model.quantizer.encode."""
    emb = model.encoder(wave[:, None])
    codes = model.quantizer.encode(emb)                              # (Q, B, T): every codebook the model holds
    return codes.transpose(0, 1).contiguous(), emb.transpose(1, 2).contiguous()


def main():
    model = build_model(0, target_bandwidths=[144.0], **SMALL)       # 8 codebooks, as gen_codec_golden.py
    rescale(model, 1)
    sd = encoder_state_dict(model)
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    books = E.codebooks_of(sd)
    model64 = build_model(0, target_bandwidths=[144.0], **SMALL)
    model64.load_state_dict(model.state_dict())
    model64 = model64.double()
    for L in LENGTHS:
        wave = torch.randn(B, L, generator=torch.Generator().manual_seed(100 + L)).clamp(-3, 3) * 0.3
        codes32, emb32 = model_encode(model, wave)
        codes64, emb64 = model_encode(model64, wave.double())
        T, D = emb64.shape[1:]
        _, margin, e_score = E.rvq_scores(books, emb64.reshape(B * T, D), emb32.reshape(B * T, D))
        arrays.update({f'wave/{L}': wave.numpy(), f'emb64/{L}': emb64.numpy(), f'emb32/{L}': emb32.numpy(),
                       f'codes64/{L}': codes64.numpy(), f'codes32/{L}': codes32.numpy(), f'margin/{L}': margin.view(B, T).numpy()})
        print(f'L={L}: T={T} max|emb64|={emb64.abs().max():.3f} max|emb32-emb64|={(emb32.double() - emb64).abs().max():.2e} '
              f'codes32==codes64: {torch.equal(codes32, codes64)} min margin={margin.min():.3e} e_score={e_score:.2e}')
    np.savez_compressed(OUT, **arrays)
    print(f'{OUT.name}: {OUT.stat().st_size} bytes, {len(sd)} tensors')


if __name__ == '__main__':
    main()
