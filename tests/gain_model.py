"""The per-stream output gain restated in numpy (include/speexhip_resampler.h, "Gain"), for the tests to hold the library
against.  A stream's gain state is (from, to, total, done); the gain of the output frame k frames behind the start of the
ramp is

  step = (float64(to) - float64(from)) / float64(total)
  g(k) = float32( float64(from) + float64(k) * step )   for k <  total
  g(k) = to                                             for k >= total

evaluated as written: every step one IEEE operation on float64 in numpy (no fused operations), then astype(float32), which
rounds to nearest-even.  Every sample of the frame becomes y * g in float32.  The expected bytes of a gained call are
these products of an ungained twin's floats, encoded by the format models; nothing here comes from the code under test."""
import numpy as np


def g(from_gain, to_gain, total, first, n):
    """g(first) .. g(first + n - 1) as float32"""
    frm, to = np.float32(from_gain), np.float32(to_gain)
    k = np.uint64(int(first)) + np.arange(int(n), dtype=np.uint64)
    out = np.full(int(n), to, np.float32)
    if total:
        step = (np.float64(to) - np.float64(frm)) / np.float64(int(total))
        inside = k < np.uint64(int(total))
        with np.errstate(over="ignore", invalid="ignore"):
            p = k[inside].astype(np.float64) * step
            s = np.float64(frm) + p
            out[inside] = s.astype(np.float32)
    return out


def apply(y, gains, c_out):
    """flat interleaved float32 y (frames of c_out samples) times the frames' gains, in float32"""
    y = np.asarray(y, np.float32).reshape(-1, c_out)
    gains = np.asarray(gains, np.float32)
    assert gains.shape == (y.shape[0],)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (y * gains[:, None]).astype(np.float32).reshape(-1)


class State:
    """(from, to, total, done) of one stream, moved as set_gain and the formatted calls move it"""

    def __init__(self):
        self.frm, self.to, self.total, self.done = np.float32(1.0), np.float32(1.0), 0, 0

    def current(self):
        return g(self.frm, self.to, self.total, self.done, 1)[0]

    def set(self, gain, ramp_frames=0):
        self.frm = self.current()
        self.to, self.total, self.done = np.float32(gain), int(ramp_frames), 0

    def off(self):
        return self.to == np.float32(1.0) and (self.total == 0 or self.done == self.total)

    def take(self, frames):
        """the gains of the next `frames` output frames of a formatted call; moves done (saturating at total).  A state
        that is off does not move."""
        out = g(self.frm, self.to, self.total, self.done, frames)
        self.done = min(self.total, self.done + int(frames))
        return out

    def report(self):
        """what get_gain reports: (bits of current, bits of target, remaining)"""
        return (np.float32(self.current()).tobytes(), np.float32(self.to).tobytes(), self.total - self.done)
