"""Deterministic float32 input of the kinds a float caller really sends, for the exact-model tests.

Every float stream the suite fed used to be `pcm.astype(np.float32)`: 16-bit mantissas, no fractions, every channel equally
loud.  Each kind below is what one class of defect needs in order to show (tests/test_cpu_exact_model.py plants each):

  A  uniform in [-1, 1), full float32 mantissa      a window or table staged through a narrower type (float16, bf16)
  B  A x 2^uniform(-24, 0), per sample              a relative error that does not scale: an absolute epsilon somewhere
  C  A with the odd channels x 2^-20 (>= 2 ch)      cross-channel leakage at the 2^-22 level (packed FMAs, row mapping,
                                                    staged stores): 4 u of an equally loud neighbour, inside the bound
  G  A x 2^-20 on alternate passages of 997 frames  quiet passages next to loud ones: a flush or a floor in time
  E  A x 2^100                                      far outside the int16 range: a clamp, or a rounding to integers
  D  A x 2^-125                                     gradual underflow (judged with the bounds' underflow term alone)
  P  A x 12000                                      PCM scale WITH fractions: what an int16 window loses

Seeded with RandomState; `taps` given, the stream carries exact_model.with_silence's stretch of silence.
"""
import numpy as np

import exact_model as em

KINDS = "ABCGEDP"
ROTATION = "ABCGE"      # the kinds the GPU family tests rotate through by case index
PASSAGE = 997


def kind_for(index, channels):
    """the kind of case number `index`: A, B, C, G, E in turn; C needs a channel to be quiet next to, so mono takes G"""
    kind = ROTATION[index % len(ROTATION)]
    return "G" if kind == "C" and channels < 2 else kind


def make(kind, frames, channels, seed, taps=None):
    """-> float32 (frames, channels) of `kind`"""
    assert kind in KINDS and (kind != "C" or channels >= 2), (kind, channels)
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (frames, channels))
    if kind == "B":
        x = x * np.exp2(rng.uniform(-24.0, 0.0, (frames, channels)))
    elif kind == "C":
        x[:, 1::2] *= 2.0 ** -20
    elif kind == "G":
        x[(np.arange(frames) // PASSAGE) % 2 == 1] *= 2.0 ** -20
    elif kind == "E":
        x = x * 2.0 ** 100
    elif kind == "D":
        x = x * 2.0 ** -125
    elif kind == "P":
        x = x * 12000.0
    x = x.astype(np.float32)        # (one rounding of the float64 product: subnormals of kind D included)
    return em.with_silence(x, taps) if taps is not None and frames > 2 * taps + 64 else x


def quiet_frames(frames):
    """the frames of kind G's quiet passages"""
    return (np.arange(frames) // PASSAGE) % 2 == 1
