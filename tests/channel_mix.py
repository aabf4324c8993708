"""The numpy statement of a mixed call's channel mix (include/speexhip_resampler.h): one frame x of n samples times a
row-major matrix M (outputs x n).  Output o is acc = M[o][0] * x[0], then acc = acc + M[o][i] * x[i] for i = 1 .. n-1 in
ascending order, every product and sum in float64 (the product of two float32 values is exact there), then ONE rounding
to float32.  Every term is included; nothing is clamped.  Inputs are expected finite and away from float32 denormals."""
import numpy as np


def mix(M, frames):
    """M: (outputs, n) float32; frames: any array of whole frames of n float32 samples.  Returns (frames, outputs)
    float32."""
    M = np.asarray(M, dtype=np.float32)
    assert M.ndim == 2
    x = np.asarray(frames, dtype=np.float32).reshape(-1, M.shape[1]).astype(np.float64)
    m = M.astype(np.float64)
    acc = x[:, 0:1] * m[None, :, 0]
    for i in range(1, M.shape[1]):
        acc = acc + x[:, i:i + 1] * m[None, :, i]
    return acc.astype(np.float32)


def mix_descending(M, frames):
    """the same sum taken from the last term to the first: NOT the rule -- what test_cpu_mix.py tells it from"""
    M = np.asarray(M, dtype=np.float32)
    x = np.asarray(frames, dtype=np.float32).reshape(-1, M.shape[1]).astype(np.float64)
    m = M.astype(np.float64)
    n = M.shape[1]
    acc = x[:, n - 1:n] * m[None, :, n - 1]
    for i in range(n - 2, -1, -1):
        acc = acc + x[:, i:i + 1] * m[None, :, i]
    return acc.astype(np.float32)


# the three matrices people ask for
STEREO_TO_MONO = np.float32([[0.5, 0.5]])
MONO_TO_STEREO = np.float32([[1.0], [1.0]])
# ITU-R BS.775 style 5.1 (L R C LFE Ls Rs) -> stereo, LFE dropped
SURROUND_TO_STEREO = np.float32([[1.0, 0.0, 0.70710678, 0.0, 0.70710678, 0.0],
                                 [0.0, 1.0, 0.70710678, 0.0, 0.0, 0.70710678]])
