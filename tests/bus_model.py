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


ORDER_DEFECTS = ("descending", "tree", "evens_then_odds", "fp32_accumulator")
OTHER_DEFECTS = ("round_each_add", "skip_zero_weight", "zero_plus_first", "skip_ended")
DEFECTS = ORDER_DEFECTS + OTHER_DEFECTS


def _defective(w_row, y64, defect, live):
    """one bus with one planted DEFECT, as float32 -- what a kernel that got the rule wrong in that way would store:
      descending         the streams summed from the last to the first
      tree               pairwise: (p0 + p1) + (p2 + p3) ...
      evens_then_odds    streams 0, 2, 4 ... then 1, 3, 5 ...
      fp32_accumulator   products and sums in float32
      round_each_add     the fp64 sum rounded to float32 after every add (an fp32 fused multiply-add)
      skip_zero_weight   a stream whose weight is 0 contributes no term
      zero_plus_first    the first term is 0.0 + the product
      skip_ended         a stream contributes no term where it has ended (live[s, i] False)
    A sum without any term is +0.0."""
    n_streams = y64.shape[0]
    p = [np.float64(w_row[s]) * y64[s] for s in range(n_streams)]
    if defect == "tree":
        while len(p) > 1:
            p = [p[i] + p[i + 1] if i + 1 < len(p) else p[i] for i in range(0, len(p), 2)]
        return p[0].astype(np.float32)
    order = list(range(n_streams))
    if defect == "descending":
        order.reverse()
    elif defect == "evens_then_odds":
        order = order[0::2] + order[1::2]
    narrow32 = defect in ("fp32_accumulator", "round_each_add")
    if defect == "fp32_accumulator":
        p = [q.astype(np.float32).astype(np.float64) for q in p]
    acc = np.zeros(y64.shape[1], np.float64)
    started = np.zeros(y64.shape[1], bool)
    for s in order:
        if defect == "skip_zero_weight" and w_row[s] == 0:
            continue
        first = np.float64(0.0) + p[s] if defect == "zero_plus_first" else p[s]
        new = np.where(started, acc + p[s], first)
        if narrow32:
            new = new.astype(np.float32).astype(np.float64)
        take = live[s] if defect == "skip_ended" else np.ones_like(started)
        acc = np.where(take, new, acc)
        started = started | take
    return acc.astype(np.float32)


def buses(weights, y, defect=None, live=None):
    """(n_buses, n) float32: the buses of y (n_streams, n) float32 under weights (n_buses, n_streams) float32.
    defect: one of DEFECTS planted (None: the rule); live (n_streams, n) bool, for "skip_ended": where a stream has not
    ended."""
    w = np.asarray(weights, np.float32)
    y = np.asarray(y, np.float32)
    assert w.ndim == 2 and y.ndim == 2 and w.shape[1] == y.shape[0]
    y64 = y.astype(np.float64)
    if defect is not None:
        assert defect in DEFECTS, defect
        live = np.ones(y.shape, bool) if live is None else np.asarray(live, bool)
        assert live.shape == y.shape
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return np.stack([_defective(w[j], y64, defect, live) for j in range(w.shape[0])])
    out = np.empty((w.shape[0], y.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(w.shape[0]):
            acc = np.float64(w[j, 0]) * y64[0]
            for s in range(1, w.shape[1]):
                p = np.float64(w[j, s]) * y64[s]
                acc = acc + p
            out[j] = acc.astype(np.float32)
    return out


def buses_wide(weights, y):
    """buses(weights, y), the rule alone, with the Python loop over the streams only and all buses at once as (n_buses, n)
    float64 arrays: every product and every add still one IEEE operation per element, in the same order -- the same bits,
    at a width (1024 x 1024) where the loop over the buses takes many times as long"""
    w = np.asarray(weights, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32)
    assert w.ndim == 2 and y.ndim == 2 and w.shape[1] == y.shape[0]
    y64 = y.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        acc = w[:, 0:1] * y64[0][None, :]
        for s in range(1, w.shape[1]):
            p = w[:, s: s + 1] * y64[s][None, :]
            acc = acc + p
        return acc.astype(np.float32)


# ---- the mixer's kernel (bus_sum_legs): legs walked in blocks, a block's legs dealt to waves ---------------------------
# What its structure invites, kept apart from ORDER_DEFECTS (the Batch's kernel has neither blocks nor waves):
#   block_partials   each block of `block` legs summed in ascending order into its own fp64 partial (its first term the
#                    product itself), the partials then added in ascending order
#   wave_dealt       one accumulator, but within each block the legs added in the order their waves fetched them: block
#                    slot wave + r * waves -- 0, 4, 8, 12, 1, 5, ... -- a ragged last block leaving out what it lacks
LEG_DEFECTS = ("block_partials", "wave_dealt")
LEG_BLOCK, LEG_WAVES = 16, 4


def wave_dealt_order(n_legs, block=LEG_BLOCK, waves=LEG_WAVES):
    assert block % waves == 0
    order = []
    for b0 in range(0, n_legs, block):
        order += [b0 + wave + r * waves for wave in range(waves) for r in range(block // waves) if b0 + wave + r * waves < n_legs]
    assert sorted(order) == list(range(n_legs))
    return order


def buses_legs(weights, y, defect, block=LEG_BLOCK, waves=LEG_WAVES):
    """(n_buses, n) float32: the buses with one of LEG_DEFECTS planted"""
    assert defect in LEG_DEFECTS, defect
    w = np.asarray(weights, np.float32).astype(np.float64)
    y64 = np.asarray(y, np.float32).astype(np.float64)
    assert w.ndim == 2 and y64.ndim == 2 and w.shape[1] == y64.shape[0]
    n_legs = w.shape[1]
    term = lambda s: w[:, s: s + 1] * y64[s][None, :]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if defect == "wave_dealt":
            order = wave_dealt_order(n_legs, block, waves)
            acc = term(order[0])
            for s in order[1:]:
                acc = acc + term(s)
            return acc.astype(np.float32)
        total = None
        for b0 in range(0, n_legs, block):
            part = term(b0)
            for s in range(b0 + 1, min(n_legs, b0 + block)):
                part = part + term(s)
            total = part if total is None else total + part
        return total.astype(np.float32)


def order_layout_legs(n_legs, pairs, frames, seed=1234):
    """the order layout (below) for any leg count: (n_legs, frames) float32, mono.  Values of 2^12 everywhere; for pair k
    = (a, a + 1) of `pairs` a 2^60-sized value in leg a over stretch k of the frames (len(pairs) equal stretches, the last
    one taking the remainder), and leg a + 1 the exact negation of leg a throughout."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1.0, 1.0, (n_legs, frames)) * 2.0 ** 12).astype(np.float32)
    huge = (rng.uniform(-1.0, 1.0, frames) * 2.0 ** 60).astype(np.float32)
    for lo, hi, (a, b) in zip(*order_stretches(len(pairs), frames), pairs):
        assert b == a + 1 and 0 <= a and b < n_legs
        x[a, lo:hi] = huge[lo:hi]
    for a, b in pairs:
        x[b] = -x[a]
    return x


def order_stretches(n_pairs, frames):
    """(the first frame of each stretch, the frame behind its last)"""
    step = frames // n_pairs
    return [k * step for k in range(n_pairs)], [(k + 1) * step if k + 1 < n_pairs else frames for k in range(n_pairs)]


def order_weights_legs(n_legs, pairs, n_buses, seed=4321):
    """(n_buses, n_legs) float32 for that layout: row 0 all ones, row 1 all minus ones, one row per pair with ones on the
    pair alone (its bus: +0.0, never -0.0), then rows of random weights in [-1.5, 1.5]"""
    assert n_buses >= 2 + len(pairs)
    w = np.random.default_rng(seed).uniform(-1.5, 1.5, (n_buses, n_legs)).astype(np.float32)
    w[0], w[1] = 1.0, -1.0
    for k, (a, b) in enumerate(pairs):
        w[2 + k] = 0.0
        w[2 + k, [a, b]] = 1.0
    return w


# the two order layouts of the mixer's tests: 48 legs -- three blocks; the pair (15, 16) straddles the first block edge, which
# only block_partials can see (15 is the last leg of its block in either order); (46, 47) ends the ragged walk of a wave --
# and the mixer's limits, 1024 x 1024, with a slot that is empty and one that is silent (+0.0 throughout either way)
LEGS_48, PAIRS_48 = 48, ((0, 1), (15, 16), (46, 47))
LIMIT, LIMIT_PAIRS, LIMIT_EMPTY, LIMIT_SILENT = 1024, ((0, 1), (1007, 1008), (1022, 1023)), 500, 501


def limits_layout(frames, seed=1234):
    x = order_layout_legs(LIMIT, LIMIT_PAIRS, frames, seed)
    x[[LIMIT_EMPTY, LIMIT_SILENT]] = 0.0
    return x


def live_of(lengths, n):
    """(n_streams, n) bool: sample i of stream s lies before the stream's end (lengths in samples)"""
    return np.arange(n)[None, :] < np.asarray(lengths)[:, None]


def changed(a, b):
    """share of the samples of one bus whose float32 bits differ; two NaNs count as the same value"""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    return float(((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).mean()) if a.size else 0.0


# The "order" layout: 32 streams whose sum tells every order apart.  A pair of huge values that cancel exactly (2^60: one
# ulp of the fp64 accumulator is 2^8 there) among values of 2^12 -- what the accumulator loses of the small values depends
# on how many of them it holds when the huge one arrives and leaves.  Stream 1 is the negation of stream 0 and stream 31
# of stream 30 throughout; the first half's huge values are in streams 0 and 1, the second half's in streams 30 and 31,
# everything else is 2^12.  Row 0 sums everything, row 1 its negation, rows 2 and 3 one pair alone with zero weights on
# everybody else: +0.0, never -0.0.
ORDER_STREAMS = 32
ORDER_W = np.zeros((4, ORDER_STREAMS), np.float32)
ORDER_W[0], ORDER_W[1] = 1.0, -1.0
ORDER_W[2, :2] = 1.0
ORDER_W[3, -2:] = 1.0


def order_layout(frames, seed=1234):
    """(32, frames) float32, mono: the layout above, its halves frames // 2 long"""
    rng = np.random.default_rng(seed)
    half = frames // 2
    x = (rng.uniform(-1.0, 1.0, (ORDER_STREAMS, frames)) * 2.0 ** 12).astype(np.float32)
    huge = (rng.uniform(-1.0, 1.0, frames) * 2.0 ** 60).astype(np.float32)
    x[0, :half], x[30, half:] = huge[:half], huge[half:]
    x[1], x[31] = -x[0], -x[30]       # (negations throughout, so that a linear filter keeps them negations)
    return x


def mix_minus(n):
    """W = ones - identity: bus j is everybody but stream j"""
    return (np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)).astype(np.float32)
