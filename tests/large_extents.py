"""Calls whose sample indices cross 2^31 and 2^32: a virtual input, the judge of one output window, the windows of a long
call, the planner restated, sentinels and the memory gate.  (tests/test_cpu_large_extents.py, test_gpu_large_extents.py)

Every length of the C ABI is a uint32 count of frames and every stride a uint64, so one call may index many GiB.  The
kernels' index arithmetic mixes 32- and 64-bit types; one missing cast is wrong only beyond 4 GiB.  What is needed to
notice is (1) an input whose value at sample n differs from its value at n - 2^31 and n - 2^32, known on the CPU without
being stored, (2) a judge for a few thousand outputs in the middle of a stream, and (3) the place of the outputs whose
reads or stores cross a power of two.

The virtual input.  Sample n of a stream's interleaved buffer is tile[n % P] with P = 2^24 - 3 samples of noise (int16:
oracle.lcg_pcm; float: float_inputs kind A, full mantissas), except inside a short list of silent frame ranges of
taps + 17 frames (exact_model.with_silence's stretch: single edge taps decide whole samples there).  2^31 % P = 384 and
2^32 % P = 768: a read that wraps at either power lands on other samples.  slice() returns any stretch on the CPU;
fill() writes a device tensor with torch, and the GPU tests read every judged stretch back and compare it with slice().

The judge.  judge_window() is check (a) of exact_model on outputs [K0, K0 + W) of a stream that began at position (0, 0):
Model.segment(head, (0, frac(K0))) with head = the taps - 1 line frames in front of pos(K0) -- no history logic, no new
tolerance.  The CPU parts import without torch and without a GPU.
"""
import bisect
from functools import lru_cache

import numpy as np

import exact_model as em
import float_inputs as fi
import oracle as orc

P = (1 << 24) - 3
SENTINELS = 4096        # elements of sentinel in front of, behind and between everything a call may write
GIB = float(1 << 30)
assert ((1 << 31) % P, (1 << 32) % P) == (384, 768)


def silence_frames(taps):
    return taps + 17


class VirtualInput:
    """kind 'int16' | 'float' | 'ulaw' (mu-law codes, for the formatted calls); silent: [(first frame, frames)] that hold
    the kind's zero."""

    def __init__(self, channels, kind="int16", silent=(), seed=2024):
        assert kind in ("int16", "float", "ulaw")
        self.channels, self.kind = channels, kind
        if kind == "ulaw":      # every code, from the noise's high bytes; silence is the code of zero
            self.tile = (orc.lcg_pcm(P, seed).view(np.uint16) >> 8).astype(np.uint8)
        else:
            self.tile = orc.lcg_pcm(P, seed) if kind == "int16" else fi.make("A", P, 1, seed).reshape(-1)
        self.zero = 0xFF if kind == "ulaw" else 0
        self.silent = sorted((int(a), int(n)) for a, n in silent)
        self._device_tile = None

    @property
    def dtype(self):
        return self.tile.dtype

    def slice(self, n0, count):
        """samples [n0, n0 + count) of the interleaved buffer"""
        n0, count = int(n0), int(count)
        start = n0 % P
        reps = (start + count + P - 1) // P
        x = (np.tile(self.tile, reps) if reps > 1 else self.tile)[start: start + count].copy()
        for a, n in self.silent:
            lo, hi = max(a * self.channels, n0), min((a + n) * self.channels, n0 + count)
            if lo < hi:
                x[lo - n0: hi - n0] = self.zero
        return x

    def frames(self, f0, count):
        return self.slice(int(f0) * self.channels, int(count) * self.channels).reshape(int(count), self.channels)

    def fill(self, tensor):
        """samples [0, tensor.numel()) into a flat device tensor: one expanded copy_ (+ the ragged end), then the silence"""
        import torch
        n = tensor.numel()
        assert tensor.dim() == 1 and tensor.dtype == {"int16": torch.int16, "float": torch.float32, "ulaw": torch.uint8}[self.kind]
        if self._device_tile is None:
            self._device_tile = torch.from_numpy(self.tile).to(tensor.device)
        full = n // P
        if full:
            tensor[: full * P].view(full, P).copy_(self._device_tile.expand(full, P))
        if n - full * P:
            tensor[full * P:].copy_(self._device_tile[: n - full * P])
        for a, cnt in self.silent:
            lo, hi = min(a * self.channels, n), min((a + cnt) * self.channels, n)
            if lo < hi:
                tensor[lo:hi].fill_(self.zero)

    def release(self):
        self._device_tile = None


# ---- the judge -------------------------------------------------------------------------------------------------------
def window_segment(model, vin, k0, w):
    """-> (the model over outputs [k0, k0 + w) of a stream from (0, 0) on `vin`, the frames it is fed, the first of them).
    Output k0 sits at line position pos0 = k0 num // den: line[pos0 + j] is input frame pos0 - (taps - 1) + j."""
    pos0, frac = divmod(int(k0) * model.num, model.den)
    taps = model.taps
    head = np.zeros((taps - 1, model.channels))
    have = min(pos0, taps - 1)
    if have:
        head[taps - 1 - have:] = vin.frames(pos0 - have, have)
    n_fed = (frac + (int(w) - 1) * model.num) // model.den + 1
    return model.segment(head, (0, frac)), vin.frames(pos0, n_fed), pos0


def judge_window(model, bits, vin, k0, got):
    """check (a) on the device's output frames [k0, k0 + len(got)): hard_int16, or judge_float without a yardstick.
    -> failure messages (empty: passed)"""
    got = np.asarray(got)
    seg, fed, pos0 = window_segment(model, vin, k0, got.shape[0])
    truth, mag = seg.truth(fed, got.shape[0])
    if got.dtype == np.int16:
        fails = em.hard_int16(seg, fed, got, truth, mag, bits)
    else:
        fails = em.judge_float(seg, fed, got, truth, mag, bits, None)[0]
    return ["outputs %d + ... (input frame %d + ...): %s" % (k0, pos0, m) for m in fails]


# ---- the windows of a long call --------------------------------------------------------------------------------------
def window_frames(num, den, quality, channels):
    """W: the larger of 8192 frames and three tiles of the plan (lane_periods x den output frames each)"""
    import speexhip
    plan, plan64 = speexhip.debug_plan(num, den, quality, channels), speexhip.debug_plan64(num, den, quality, channels)
    periods = 0
    for p in (plan, plan64):
        if p["fast_path"] in (2, 5):
            periods = max(periods, p["lane_periods"], p.get("w16_lane_periods", 0))
        elif p["fast_path"] in (3, 4):
            # The slide launcher's tile is in no planner hook (debug_launch_shape models period launches alone).  What
            # the plan does report is r_or_p, the periods of a lane block; a workgroup has at most 1024 lanes (the
            # kernels' launch bound, and the hardware's) and a lane block at least one, so no tile the launcher may
            # ever form holds more than 1024 r_or_p periods: a bound, not a guess of its waves and lanes per block.
            periods = max(periods, 1024 * p["r_or_p"])
    return max(8192, 3 * periods * den)


def windows(channels, num, den, taps, in_frames, n_out, w, float_io=False):
    """-> (windows [(name, k0, w)], absent [(name, why)], silent [(first frame, frames)]) of one call of `in_frames` frames
    that makes `n_out`: the first and last w outputs, one window centred on each place where the input or the output
    sample index crosses 2^31 and 2^32 and -- float -- where a byte offset crosses 2^32 (sample 2^30).  One silent range
    lies inside every input-side window (and inside the first and the last)."""
    assert n_out >= 2 * w, (n_out, w)
    sil = silence_frames(taps)
    span = w * num // den                       # input frames the windows of w outputs start in
    assert span > 2 * sil + 2 * taps, "a window of %d outputs is too short for the filter" % w
    wins = [("first", 0, w), ("last", n_out - w, w)]
    silent = [(span // 3, sil), ((n_out - w) * num // den + span // 3, sil)]
    absent = []
    marks = ([(1 << 30, "2^30 (byte 2^32)")] if float_io else []) + [(1 << 31, "2^31"), (1 << 32, "2^32")]
    for x, label in marks:
        f = x // channels                       # the frame that holds input sample x
        kc = f * den // num                     # an output whose window starts there
        if f + sil + taps + 8 < in_frames and kc + w // 2 <= n_out and kc >= w // 2:
            wins.append(("in " + label, kc - w // 2, w))
            silent.append((f + 5, sil))
        else:
            absent.append(("in " + label, "input sample %d is frame %d of %d channels; the call has %d frames" %
                           (x, f, channels, in_frames)))
        kc = x // channels
        if kc + w // 2 <= n_out and kc >= w // 2:
            wins.append(("out " + label, kc - w // 2, w))
        else:
            absent.append(("out " + label, "output sample %d is frame %d of %d channels; the call makes %d frames" %
                           (x, kc, channels, n_out)))
    return wins, absent, silent


def frames_to_cross(channels, num, den, w, in_mark=None, out_mark=None):
    """the odd frame count of a call that crosses input sample `in_mark` and / or output sample `out_mark` and goes three
    windows further"""
    need = 0
    if in_mark:
        need = max(need, in_mark // channels + 3 * (w * num // den + 1))
    if out_mark:
        need = max(need, ((out_mark // channels + 3 * w) * num + den - 1) // den)
    return need | 1


# ---- the planner, restated -------------------------------------------------------------------------------------------
# The reference walks a call in blocks of block_in input frames; the int16 entry point makes at most 1024 outputs per
# block.  One block is a closed form; the blocks of a call are walked as the reference walks them, except that while
# every block is a full one (block_in frames to read, room for all it makes) the position after a block depends on the
# position before it alone -- the positions run into a cycle, and whole blocks are skipped along it.
BLOCK_OUT = 1024


def _block(num, den, last, frac, nin, cap):
    """process_native: outputs while last < nin and fewer than cap; -> (last', frac', frames used, outputs made)"""
    made = 0 if last >= nin else -(-((nin - last) * den - frac) // num)
    if cap is not None and made > cap:
        made = cap
    t = frac + made * num
    at, frac = last + t // den, t % den
    used = min(at, nin)
    return at - used, frac, used, made


@lru_cache(maxsize=None)
def _orbit(num, den, block_in, block_out, last, frac):
    """positions before full blocks 0, 1, ... until one repeats: (states, cumulative frames, cumulative outputs, index of
    the first state of the cycle)"""
    seen, states, cin, cout = {}, [], [0], [0]
    while (last, frac) not in seen:
        seen[(last, frac)] = len(states)
        states.append((last, frac))
        last, frac, used, made = _block(num, den, last, frac, block_in, block_out)
        cin.append(cin[-1] + used)
        cout.append(cout[-1] + made)
    return states, cin, cout, seen[(last, frac)]


def _skip_full_blocks(num, den, block_in, block_out, last, frac, ilen, olen):
    """as many full blocks as leave block_in frames to read and one output of room: -> (last, frac, ilen, olen)"""
    states, cin, cout, i0 = _orbit(num, den, block_in, block_out, last, frac)
    n, cyc = len(states), len(states) - i0

    def after(m):
        if m <= n:
            return cin[m], cout[m]
        q, r = divmod(m - i0, cyc)
        return (cin[i0 + r] + q * (cin[n] - cin[i0]), cout[i0 + r] + q * (cout[n] - cout[i0]))

    lo, hi = 0, 1 << 40
    while lo < hi:      # the largest m with after(m) inside both budgets
        mid = (lo + hi + 1) // 2
        a, b = after(mid)
        if a <= ilen - block_in and b <= olen - 1:
            lo = mid
        else:
            hi = mid - 1
    a, b = after(lo)
    last, frac = states[lo] if lo < n else states[i0 + (lo - i0) % cyc]
    return last, frac, ilen - a, olen - b


def reference_plan(num, den, in_len, out_cap, float_entry=False, block_in=160, last=0, frac=0, magic=0):
    """speex_resampler_process_float / _process_int on one channel, counters only -> (consumed, produced, last', frac',
    magic')"""
    ilen, olen = in_len, out_cap
    if float_entry:
        if magic:
            last, frac, used, made = _block(num, den, last, frac, magic, olen)
            magic -= used
            olen -= made
        if not magic:
            per_block = -(-block_in * den // num) + 1       # no block makes more: the room of a full block
            while ilen and olen:
                if ilen > 2 * block_in and olen > 2 * per_block:
                    last, frac, ilen, olen = _skip_full_blocks(num, den, block_in, None, last, frac, ilen, olen - per_block)
                    olen += per_block
                last, frac, used, made = _block(num, den, last, frac, min(ilen, block_in), olen)
                ilen -= used
                olen -= made
    else:
        while ilen and olen:
            if not magic and ilen > 2 * block_in and olen > 2 * BLOCK_OUT:
                last, frac, ilen, olen = _skip_full_blocks(num, den, block_in, BLOCK_OUT, last, frac, ilen, olen - BLOCK_OUT)
                olen += BLOCK_OUT
            ichunk, ochunk = min(ilen, block_in), min(olen, BLOCK_OUT)
            if magic:
                last, frac, used, made = _block(num, den, last, frac, magic, ochunk)
                magic -= used
                ochunk -= made
                olen -= made
            if not magic:
                last, frac, used, made = _block(num, den, last, frac, ichunk, ochunk)
                ilen -= used
                olen -= made
    return in_len - ilen, out_cap - olen, last, frac, magic


def naive_plan(num, den, in_len, out_cap, float_entry=False, block_in=160, last=0, frac=0, magic=0):
    """the same with the reference's own per-output loop: for calls of a few thousand frames"""
    def native(last, frac, nin, cap):
        made = 0
        while not (last >= nin or made >= cap):
            made += 1
            last += num // den
            frac += num % den
            if frac >= den:
                frac -= den
                last += 1
        used = min(last, nin)
        return last - used, frac, used, made
    ilen, olen = in_len, out_cap
    if float_entry:
        if magic:
            last, frac, used, made = native(last, frac, magic, olen)
            magic -= used
            olen -= made
        if not magic:
            while ilen and olen:
                last, frac, used, made = native(last, frac, min(ilen, block_in), olen)
                ilen -= used
                olen -= made
    else:
        while ilen and olen:
            ichunk, ochunk = min(ilen, block_in), min(olen, BLOCK_OUT)
            if magic:
                last, frac, used, made = native(last, frac, magic, ochunk)
                magic -= used
                ochunk -= made
                olen -= made
            if not magic:
                last, frac, used, made = native(last, frac, ichunk, ochunk)
                ilen -= used
                olen -= made
    return in_len - ilen, out_cap - olen, last, frac, magic


# ---- sentinels -------------------------------------------------------------------------------------------------------
def sentinel_value(dtype_name):
    return {"int16": orc.SENTINEL_I16, "float32": orc.SENTINEL_F32, "uint8": 0xA5}[dtype_name]


def sentinel_ranges(regions, total):
    """regions: [(first element, elements)] a call may write, counted from the pointer the call is given, inside an
    allocation of SENTINELS + total + SENTINELS elements.  -> disjoint [lo, hi) ranges that must stay untouched:
    SENTINELS elements at both ends of the allocation, around every region and around the 32-bit-wrapped alias of every
    region (its offset mod 2^32) -- less the regions themselves."""
    want = [(-SENTINELS, 0), (total, total + SENTINELS)]
    for s, n in regions:
        for a in sorted({s, s % (1 << 32)}):
            want += [(a - SENTINELS, a), (a + n, a + n + SENTINELS)]
    regions = sorted(regions)
    starts = [s for s, _ in regions]
    out = []
    for lo, hi in sorted(set(want)):
        lo, hi = max(lo, -SENTINELS), min(hi, total + SENTINELS)
        i = max(0, bisect.bisect_right(starts, lo) - 1)
        while lo < hi:
            while i < len(regions) and regions[i][0] + regions[i][1] <= lo:
                i += 1
            if i == len(regions) or regions[i][0] >= hi:
                out.append((lo, hi))
                break
            if regions[i][0] > lo:
                out.append((lo, regions[i][0]))
            lo = regions[i][0] + regions[i][1]
    merged = []
    for lo, hi in sorted(out):
        if merged and lo <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(hi, merged[-1][1]))
        else:
            merged.append((lo, hi))
    return merged


class Guarded:
    """An output allocation of `total` elements behind SENTINELS elements, with SENTINELS more behind it: torch.empty,
    untouched but for the sentinel ranges and the regions (pre-filled with the sentinel too, so that what a call leaves
    unwritten inside its region shows)."""

    def __init__(self, torch, dtype, total, regions):
        self.torch, self.total, self.regions = torch, int(total), [(int(s), int(n)) for s, n in regions]
        self.buf = torch.empty(self.total + 2 * SENTINELS, dtype=dtype, device="cuda")
        self.value = sentinel_value(str(dtype).split(".")[-1])
        self.ranges = sentinel_ranges(self.regions, self.total)
        for lo, hi in self.ranges + [(s, s + n) for s, n in self.regions]:
            self.buf[lo + SENTINELS: hi + SENTINELS].fill_(self.value)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + SENTINELS * self.buf.element_size()

    def at(self, first, count):
        """elements [first, first + count) from the call's pointer, as a device tensor"""
        return self.buf[first + SENTINELS: first + count + SENTINELS]

    def untouched(self, lo, hi):
        return hi <= lo or bool((self.at(lo, hi - lo) == self.value).all().item())

    def check(self, what, written=None):
        """every sentinel range, and region i beyond its first written[i] elements"""
        for lo, hi in self.ranges:
            assert self.untouched(lo, hi), "%s: sentinels at elements [%d, %d) of the output were written" % (what, lo, hi)
        for (s, n), w in zip(self.regions, written or ()):
            assert self.untouched(s + w, s + n), "%s: region at %d written past its %d elements" % (what, s, w)

    def free(self):
        self.buf = None


# ---- memory ----------------------------------------------------------------------------------------------------------
def need_bytes(in_samples, in_size, out_samples, out_size, scratch_samples=0, extra=0):
    """device bytes of a long case: its input, its output behind sentinels, the scratch output of the pieces, and what
    the case names besides (a second layout of the input, the library's own images of a formatted call)"""
    return in_samples * in_size + (out_samples + 2 * SENTINELS + scratch_samples) * out_size + extra


def gate(torch, pytest, name, need):
    """skip (with both numbers) only when less than 1.1 x need bytes are free"""
    free, total = torch.cuda.mem_get_info()
    print("\n[large extents] %s: needs %.2f GiB; %.2f GiB free of %.2f" % (name, need / GIB, free / GIB, total / GIB))
    if free < 1.1 * need:
        pytest.skip("%s needs 1.1 x %d bytes, %d are free" % (name, need, free))


def release(torch):
    import speexhip
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    speexhip.release_cached_memory()
