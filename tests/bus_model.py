"""The mix buses restated in numpy (include/speexhip_resampler.h, "Buses"), for the tests to hold the library against.
For the (already gained) float32 samples y'_s of the streams, a stream that has ended supplying +0.0, bus j is

  acc = float64(W[j][0]) * float64(y'_0)
  acc = acc + float64(W[j][s]) * float64(y'_s)        s = 1 .. n_streams - 1, in ascending order
  z   = float32(acc)                                   astype: nearest even

evaluated as written: every product and every add one IEEE operation on float64 in numpy (no fused operations, no pairwise
or blocked summation: a Python loop over the streams), then astype(float32).  Every term is included, a zero weight too.
Nothing here comes from the code under test."""
import numpy as np


def pad(streams, frames, channels):
    """the streams' flat interleaved float32 images (stream s: produced[s] * channels samples) as one (n_streams,
    frames * channels) array, +0.0 behind each stream's end"""
    y = np.zeros((len(streams), frames * channels), np.float32)
    for s, ys in enumerate(streams):
        ys = np.asarray(ys, np.float32).reshape(-1)
        assert ys.size <= y.shape[1] and ys.size % channels == 0
        y[s, : ys.size] = ys
    return y


def buses(weights, y):
    """(n_buses, n) float32: the buses of y (n_streams, n) float32 under weights (n_buses, n_streams) float32"""
    w = np.asarray(weights, np.float32)
    y = np.asarray(y, np.float32)
    assert w.ndim == 2 and y.ndim == 2 and w.shape[1] == y.shape[0]
    y64 = y.astype(np.float64)
    out = np.empty((w.shape[0], y.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(w.shape[0]):
            acc = np.float64(w[j, 0]) * y64[0]
            for s in range(1, w.shape[1]):
                p = np.float64(w[j, s]) * y64[s]
                acc = acc + p
            out[j] = acc.astype(np.float32)
    return out


def mix_minus(n):
    """W = ones - identity: bus j is everybody but stream j"""
    return (np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)).astype(np.float32)
