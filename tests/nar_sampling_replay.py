"""A float64 mirror of ONE draw of the NAR stage sampler keyed on the request (`vh_categorical_rows_keyed`,
valle2_amd/csrc/elementwise.hip): which token the device must store for a row, given the row's logits, the request's
temperature and the uniform of (seed, frame, stream).  CPU only (tests/test_nar_row_sampling_cpu.py checks it on hand-worked rows,
tests/test_nar_row_sampling_gpu.py holds device rows against it).

What is restated here:
  * x = logits * float32(1 / temperature): the kernel's scale is the fp32 quotient 1.0f / temperature, the product is exact here;
  * the normalised cumulative sums of exp(x - max) in INDEX order (this stage has no filter: the whole vocabulary is kept);
  * the token is the first index whose cumulative share exceeds u, the last index when none does;
  * a request with top_k == 1 takes the arg-max of the unscaled logits, the lowest index on ties.
The uniform is tests.sampling_replay.uniform01 (the generator of every sampler) on the stream NAR_STREAM | stage.

A draw is AMBIGUOUS when u lies within `delta` of an interior boundary of the cumulative shares: the device sums in fp32, lane
by lane, and may put such a u on either side.  DELTA = 4e-6 and the cap are not taken from the device.  An fp32 emulation of the
kernel's arithmetic (64 lane sums over contiguous ranges, the inclusive scan over lanes, the owner lane's walk) was run on the CPU
against this mirror on rows of 2 * randn(V), a fresh row per draw: it never disagreed with the mirror outside the band (0 of 6000
draws at V = 1024, 0 of 3000 at V = 1025, 0 of 6000 at V = 37, 0 of 6000 at V = 5) and the band flagged 0.77 % of the draws at
V = 1024 and 1025, at most 0.05 % at V = 37 and 5.  The device's expf is not numpy's, which the same delta has to absorb; a
disagreement outside the band is a failure, not a reason to widen it.  AMBIGUOUS_CAP: at most 2 % of a case's draws may be
ambiguous (the mirror alone flags 0.77 % at the widest vocabulary tested), so that a case cannot pass while much of it is excused."""
from __future__ import annotations

import numpy as np

from tests.sampling_replay import uniform01

DELTA = 4e-6
AMBIGUOUS_CAP = 0.02


def shares(logits, temperature):
    """The normalised cumulative sums (V,) float64 of softmax(logits * float32(1 / temperature)) in index order."""
    scale = float(np.float32(1.0) / np.float32(temperature))
    x = np.asarray(logits, dtype=np.float64) * scale
    cum = np.cumsum(np.exp(x - x.max()))
    return cum / cum[-1]


def mirror_draw(logits, temperature, u, delta=DELTA, greedy=False):
    """(token, ambiguous, cumulative shares or None) of one draw over `logits` (V,)."""
    if greedy:
        return int(np.argmax(np.asarray(logits, dtype=np.float64))), False, None
    c = shares(logits, temperature)
    hit = np.nonzero(c > u)[0]
    token = int(hit[0]) if len(hit) else len(c) - 1
    ambiguous = bool((np.abs(c[:-1] - u) <= delta).any())              # interior boundaries only: 0 and 1 bound u itself
    return token, ambiguous, c


def nar_uniform(seed, frame, stage):
    """The uniform of frame `frame` of codebook `stage` of a request with `seed`."""
    from valle2_amd.sampling import NAR_STREAM
    return uniform01(seed, frame, NAR_STREAM | stage)


def hold_rows(logits, tokens, temperatures, us, delta=DELTA):
    """Hold device `tokens` (R,) against the mirror over `logits` (R, V), per-row temperatures and uniforms.  Returns (ambiguous
    draws, disagreements inside the band, the worst |share - u| over the boundaries a disagreement crossed — 0.0 without one) and
    raises AssertionError at the first disagreement outside the band."""
    ambiguous = excused = 0
    worst = 0.0
    for r in range(len(tokens)):
        want, amb, c = mirror_draw(logits[r], temperatures[r], us[r], delta)
        got = int(tokens[r])
        ambiguous += amb
        if got == want:
            continue
        lo, hi = min(got, want), max(got, want)
        dist = float(np.abs(c[lo:hi] - us[r]).max()) if 0 <= got < len(c) else float('inf')
        worst = max(worst, dist)
        assert amb and dist <= delta, (f'row {r}: the device drew {got}, the mirror {want}; u = {us[r]:.9f} lies {dist:.3e} from the '
                                       f'farthest boundary between them (delta {delta:g}, temperature {temperatures[r]})')
        excused += 1
    return ambiguous, excused, worst
