"""Seeded inputs of the packed NAR training tests (tests/test_nar_train_packed_cpu.py, tests/test_nar_train_packed_gpu.py):
one small AdaptiveLayerNorm model and one ragged NAR batch in the collate format, zero padded.

Five utterances: text lengths 5, 1, 8, 40, 13 and frame counts 2, 3, 10, 100, 500, so the acoustic prefixes
min(frames // 3, 3 * quantization_factor) are 0, 1, 3, 33 and 150 — no prefix, a one-frame prefix, and the cap, which binds
only from 450 frames on.  The 513-row segment crosses the 256-key chunk of the attention backward twice, and the segment
starts 0, 7, 11, 29, 169 are no multiples of 32."""
import torch

from tests.golden.cases import cfg_of

KW = dict(d_model=128, n_heads=2, dim_feedforward=256, num_layers=2, dropout=0.0, norm='AdaptiveLayerNorm')
MODEL_SEED, DATA_SEED = 71, 7100
TEXT_LENS = [5, 1, 8, 40, 13]
FRAME_LENS = [2, 3, 10, 100, 500]
PREFIXES = [0, 1, 3, 33, 150]
STARTS = [0, 7, 11, 29, 169]
ROWS = 682
STAGES = (1, 7)


def inputs():
    """(config kwargs, state dict, collated NAR batch of the five utterances)."""
    from valle2_amd import synth
    cfg = cfg_of(KW)
    sd = synth.make_state_dict(cfg, 'ValleNAR', seed=MODEL_SEED, rich=True)
    g = torch.Generator(device='cpu').manual_seed(DATA_SEED)
    n = len(TEXT_LENS)
    tokens = torch.zeros(n, max(TEXT_LENS), dtype=torch.int64)
    codes = torch.zeros(n, max(FRAME_LENS), cfg.num_quantizers, dtype=torch.int64)
    for b, (tl, fl) in enumerate(zip(TEXT_LENS, FRAME_LENS)):
        tokens[b, :tl] = torch.randint(0, cfg.vocab_size, (tl,), generator=g)
        codes[b, :fl] = torch.randint(0, cfg.num_audio_tokens, (fl, cfg.num_quantizers), generator=g)
    return KW, sd, {'codes': codes, 'codes_lens': torch.tensor(FRAME_LENS), 'tokens': tokens, 'tokens_lens': torch.tensor(TEXT_LENS)}


def utterance_batch(batch, b):
    """Utterance b of a collated NAR batch alone, as a B = 1 batch with nothing padded."""
    tl, fl = int(batch['tokens_lens'][b]), int(batch['codes_lens'][b])
    return {'tokens': batch['tokens'][b:b + 1, :tl].clone(), 'tokens_lens': batch['tokens_lens'][b:b + 1].clone(),
            'codes': batch['codes'][b:b + 1, :fl].clone(), 'codes_lens': batch['codes_lens'][b:b + 1].clone()}


def weights():
    """The share of each utterance in the mean over target frames: (frames_b - prefix_b) / sum."""
    w = torch.tensor([f - p for f, p in zip(FRAME_LENS, PREFIXES)], dtype=torch.float64)
    return w / w.sum()


def param_names(sd):
    return sorted(k for k in sd if not k.endswith('.pe'))
