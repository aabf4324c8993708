"""The decision points of every sample encoder, and float streams that make the FIR emit them.

The encoders behind the FIR (csrc/format_device.h, halfbe.h, g711.h) decide: which way a tie goes, where a rail begins,
which half a value rounds to, which G.711 code an int16 gets, where the dither tips a sample over.  FIR output of noise
meets those points by chance or never, so this module makes the FIR output CHOSEN values: a float call fed one non-zero
sample A puts fl32(tap * A) -- one product, nothing added to it but zeros -- wherever that sample lies under a tap.  For
a wanted float32 `target` take a tap, A0 = fl32(target / tap), and search A0 +- 8 ulp for fl32(tap * A) == target.
Impulses at least taps + 3 frames apart do not meet under any window.

  targets(out_fmt, kind, seed)  -> {class name: [float32 | At, ...]}: the decision points of the format's encoder, in
                                   internal units (one int16 step = 1.0)
  craft(model, ch, wanted, ...) -> (x float32 [frames, ch], plan): plan = [(class, output k, channel, target)], and
                                   plan.missed = what no tap of the four tried could make
  encode(fmt, y, ..., defect)   -> the numpy models' bytes, with one planted DEFECT if asked: how the tests show that a
                                   crafted stream sees what noise does not

A big-endian format's decision points are its little-endian twin's (family()); the companded formats have the S16
stage's and their compressor's.  Classes (DESIGN section 4 has the table):

  integer families (u8, s16, s24, s32; v = y * scale, q = floor(v + 0.5), clamped):
    tie / below_tie / above_tie   v = k + 0.5 exactly and its two float32 neighbours, k over 0, +-1, +-2, a spread and
                                  the last two steps before each rail, wherever float32 holds the tie
    rail_in / rail_at / rail_out  per end: the last float32 whose q is inside, the tie at the rail where float32 holds it
                                  (half-up: outside at the top, inside at the bottom), the first whose q is outside.  A
                                  saturating encoder writes the SAME code for all three: what they pin is the code
    far_out                       +-2^31 (in int16 steps) and +-1e30
  ulaw / alaw:  boundary_lo / boundary_hi   for every boundary of the compressor, q = the first int16 of the upper code:
                                  nextafter(q - 0.5, -inf) (-> q - 1, the lower code) and q - 0.5 (-> q, the upper one)
                clip              +-PEAK and the float32 around +-PEAK + 0.5
  f16n (z = y / 32768):  tie_even / tie_odd (+ _below, _above)   halfway between adjacent halfs, the lower one's
                                  mantissa even / odd, normal binades and the subnormal one
                min_sub           2^-25 (-> 0), its upper neighbour (-> 2^-24), 1.5 * 2^-24
                overflow          65520 (-> inf), its lower neighbour and 65504 (-> 0x7BFF)
                z_subnormal       2^-126 <= |y| < 2^-111: z is an fp32 subnormal, y is not
  bf16n:        tie_even / tie_odd (+ _below, _above), carry (a tie that carries into the exponent, one of them at
                2^125: the largest y whose impulse is finite under every filter here), z_subnormal (ties of the bf16
                rounding on fp32-subnormal z).  z = y * 2^-15 <= 2^113 cannot round to 0x7F80 for any finite y: there is
                no overflow class.
  f32n:         z_subnormal_tie (+ _below, _above)   y * 2^-15 is inexact: ties of gradual underflow, y normal
  dithered (kind RECTANGULAR / TRIANGULAR; d = the noise at the designated output's own sample index):
    bracket_lo / bracket_hi       the two adjacent float32 around (k + 0.5 - d) / scale: the closest a float32 comes to
                                  the tie after v + d; for ulaw / alaw with k + 1 = the first int16 of a code
    reassoc  (TRIANGULAR)         y = -2^-75 at an output whose d is exactly -0.5: (v + d) rounds to -0.5, + 0.5 is 0,
                                  floor 0; v + (d + 0.5) = v, floor -1.  The only place the two orders part for any
                                  float32 y (k + 1 = 0: the sum v + d + 0.5 is tiny and exact, v + d is not)."""
import functools

import numpy as np

import dither_model as dm
import exact_model as em
import g711_model as gm
import halfbe_model as hm
import sample_formats as sf

F32 = np.float32
INF32 = np.float32(np.inf)
START = (1 << 32) - 1000      # output frame at which the dithered states of the tests begin: idx crosses 2^32 early on
SEEDS = {dm.RECTANGULAR: 0x0123456789ABCDEF, dm.TRIANGULAR: 0xDEADBEEFCAFEF01C}
ULPS, TAPS_TRIED = 8, 4

INT_FAMILIES = (sf.U8, sf.S16, sf.S24, sf.S32)
# v = y * scale; q = floor(v + 0.5) held to [lo, hi] (U8: before its offset of 128)
INT_RULE = {sf.U8: (1.0 / 256.0, -128, 127), sf.S16: (1.0, -32768, 32767), sf.S24: (256.0, -(1 << 23), (1 << 23) - 1),
            sf.S32: (65536.0, -(1 << 31), (1 << 31) - 1)}


def family(fmt):
    """the format whose encoder decides for fmt: a big-endian format's little-endian twin"""
    return hm.LE_TWIN.get(fmt, fmt)


def stage(fmt):
    """the integer family whose rounding the format's encoder runs (None: a float format)"""
    fam = family(fmt)
    return sf.S16 if fam in gm.COMPANDED else fam if fam in INT_FAMILIES else None


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def below(v):
    return np.nextafter(np.asarray(v, np.float32), -INF32)


def above(v):
    return np.nextafter(np.asarray(v, np.float32), INF32)


def held(v):
    """the float64 values that float32 holds exactly, as float32"""
    v = np.asarray(v, np.float64).reshape(-1)
    return f32(v[f32(v).astype(np.float64) == v])


def bits32(words):
    return np.asarray(words, np.uint32).view(np.float32)


class At:
    """A target that depends on the dither of the output sample it lands on: value(idx) -> float32, for idx = the
    sample's dither index; accept(idx array) -> which indices will do (None: any)."""

    def __init__(self, value, accept=None):
        self.value, self.accept = value, accept


# ---- the classes -----------------------------------------------------------------------------------------------------
def halfup_of(fam, y):
    """floor(v + 0.5) of float32 y in the integer family fam, unclamped, as float64"""
    scale = INT_RULE[fam][0]
    return np.floor(np.asarray(y, np.float32).astype(np.float64) * scale + 0.5)


def _steps(fam):
    """the k of the family's ties: 0, +-1, +-2, a spread, the last two steps before each rail"""
    scale, lo, hi = INT_RULE[fam]
    rng = np.random.RandomState(1000 + fam)
    spread = [int(v) for v in rng.randint(lo // 2, hi // 2, 6)] + [hi // 3, lo // 3]
    return [0, 1, -1, 2, -2] + spread + [hi - 2, hi - 1, lo, lo + 1]


def _rail(fam, top):
    """(rail_in, rail_at or None, rail_out) of one end"""
    scale, lo, hi = INT_RULE[fam]
    edge = (hi + 0.5 if top else lo - 0.5) / scale          # v = the tie at the rail
    inside = lambda y: lo <= halfup_of(fam, y) <= hi
    y = f32(edge)
    step = (above, below) if top else (below, above)          # (outwards, inwards)
    while inside(y):
        y = step[0](y)
    while not inside(step[1](y)):
        y = step[1](y)
    at = held([edge])
    return step[1](y), (at[0] if at.size else None), y


def _int_targets(fam):
    scale, lo, hi = INT_RULE[fam]
    tie = held([(k + 0.5) / scale for k in _steps(fam)])
    out = {"tie": tie, "below_tie": below(tie), "above_tie": above(tie), "rail_in": [], "rail_at": [], "rail_out": []}
    for top in (True, False):
        a, b, c = _rail(fam, top)
        out["rail_in"].append(a)
        out["rail_out"].append(c)
        if b is not None:
            out["rail_at"].append(b)
    out["far_out"] = f32([2.0 ** 31, -(2.0 ** 31), 1e30, -1e30])
    return out


def boundaries(fmt):
    """the first int16 of every code of the compressor but the lowest: 255 of them, both signs"""
    codes = gm.encode(fmt, np.arange(-32768, 32768)).astype(np.int64)
    return np.nonzero(np.diff(codes) != 0)[0] - 32768 + 1


def _g711_targets(fmt):
    q = boundaries(fmt).astype(np.float64)
    peak = float(gm.PEAK[fmt])
    clip = f32([peak, -peak, peak + 0.5, -peak - 0.5])
    return {"boundary_hi": f32(q - 0.5), "boundary_lo": below(f32(q - 0.5)),
            "clip": np.concatenate([clip, below(clip[2:]), above(clip[2:]), f32([32767.5, -32768.5]), below(f32([32767.5, -32768.5]))])}


def _with_neighbours(out, name, z, scale=32768.0):
    y = held(np.asarray(z, np.float32).astype(np.float64) * scale)
    out[name], out[name + "_below"], out[name + "_above"] = y, below(y), above(y)


def _f16_targets():
    # binary16 has 10 fraction bits: in fp32 a tie has fraction bit 12 set and the 12 below it clear
    exps = np.array([127 - 14, 127, 127 + 15], np.uint32)
    out = {}
    for name, mant in (("tie_even", (0, 0x3FE)), ("tie_odd", (1, 0x3FF))):
        z = bits32(((exps[:, None] << np.uint32(23)) | (np.array(mant, np.uint32)[None, :] << np.uint32(13)) | np.uint32(0x1000)).reshape(-1))
        # the subnormal binade: odd multiples of 2^-25 -- between n and n + 1 times 2^-24, n = the kept mantissa
        sub = np.array({"tie_even": (5, 2045), "tie_odd": (3, 2047)}[name], np.float32) * F32(2.0 ** -25)
        z = np.concatenate([z, sub])
        z = z[np.abs(z) < 65520.0]
        _with_neighbours(out, name, np.concatenate([z, -z[:2]]))
    m = F32(2.0 ** -25)
    out["min_sub"] = f32([m, above(m), 1.5 * 2.0 ** -24]) * F32(32768.0)
    out["overflow"] = np.array([65520.0, below(F32(65520.0)), 65504.0], np.float32) * F32(32768.0)
    out["z_subnormal"] = f32([2.0 ** -126, 1.5 * 2.0 ** -120, -(2.0 ** -118), float(below(F32(2.0 ** -111)))])
    return out


def _bf16_targets():
    out = {}
    _with_neighbours(out, "tie_even", bits32([0x3F808000, 0x40008000, 0xBF808000, 0x3EFE8000]))
    _with_neighbours(out, "tie_odd", bits32([0x3F818000, 0x40FD8000, 0xBF818000, 0x3E018000]))
    # mantissa 0x7F: the tie carries into the exponent; 0x6FFF8000 * 2^15 = 2^125 (1 - 2^-9)
    _with_neighbours(out, "carry", bits32([0x3FFF8000, 0xBF7F8000, 0x6FFF8000]))
    # z = n * 2^-149 with n = (hi << 16) | 0x8000, hi < 0x80: bf16 ties on fp32 subnormals; y = z * 2^15 is normal
    out["z_subnormal"] = f32([n * 2.0 ** -134 for n in (0x18000, 0x28000, 0x7F8000, 0x17FFF, 0x18001, -0x38000)])
    return out


def _f32n_targets():
    # y = (2 n + 1) 2^-135: z = (n + 0.5) 2^-149, a tie of the gradual underflow, towards even n
    odd = np.array([2 * n + 1 for n in (256, 257, 1000, 1001, 1 << 21, (1 << 21) + 1)], np.float64)
    tie = f32(np.concatenate([odd, -odd[:2]]) * 2.0 ** -135)
    assert (np.abs(tie) >= 2.0 ** -126).all()
    return {"z_subnormal_tie": tie, "z_subnormal_tie_below": below(tie), "z_subnormal_tie_above": above(tie)}


def straddle(scale, k, d):
    """the two adjacent float32 y around (k + 0.5 - d) / scale whose q = floor((y * scale + d) + 0.5) differ -- the
    arithmetic of dither_model.quantise; -> (lo, hi) with q(lo) <= k < q(hi)"""
    c = f32((k + 0.5 - d) / scale)
    cand = [c]
    for _ in range(3):
        cand = [below(cand[0])] + cand + [above(cand[-1])]
    cand = np.array(cand, np.float32)
    q = np.floor((cand.astype(np.float64) * scale + d) + 0.5)
    i = int(np.nonzero(q <= k)[0][-1])
    assert i + 1 < cand.size and q[i] <= k < q[i + 1], (scale, k, d)
    return cand[i], cand[i + 1]


def _dither_targets(fmt, kind, seed):
    fam = family(fmt)
    st = stage(fmt)
    scale, lo, hi = INT_RULE[st]
    if fam in gm.COMPANDED:
        b = boundaries(fam)
        ks = [int(v) - 1 for v in b[[3, 40, 100, 126, 128, 150, 200, 250]]]
    else:
        ks = [1, -2, 3, -4, hi // 3, lo // 3, hi - 1, lo]
    noise = lambda idx: float(dm.values(kind, seed, idx, 1)[0])
    out = {"bracket_lo": [At(lambda idx, k=k: straddle(scale, k, noise(idx))[0]) for k in ks],
           "bracket_hi": [At(lambda idx, k=k: straddle(scale, k, noise(idx))[1]) for k in ks]}
    return out


def reassoc_target(seed):
    """the one target of class reassoc: TRIANGULAR d == -0.5 exactly at its output (2^-17 of all samples)"""
    def accept(idx):
        w = dm.words(seed, int(idx[0]), idx.size) if idx.size else np.zeros(0, np.uint32)
        return (w & np.uint32(0xFFFF)).astype(np.int64) - (w >> np.uint32(16)).astype(np.int64) == -32768
    return At(lambda idx: F32(-(2.0 ** -75)), accept)


def targets(out_fmt, kind=dm.NONE, seed=0, first_index=0):
    """{class name: [float32 | At, ...]}: the decision points of out_fmt's encoder -- without dither (kind NONE) the
    static classes; with a dither kind the classes that depend on the noise, as At targets (their index is
    first_index + k * channels + c, which craft() knows once it has picked the output).  first_index is the crafter's:
    nothing here depends on it."""
    fam = family(out_fmt)
    if kind != dm.NONE:
        return _dither_targets(out_fmt, kind, seed) if hm.dithered(out_fmt) else {}
    if fam in INT_FAMILIES:
        raw = _int_targets(fam)
    elif fam in gm.COMPANDED:
        raw = _g711_targets(fam)
    elif fam == hm.F16N:
        raw = _f16_targets()
    elif fam == hm.BF16N:
        raw = _bf16_targets()
    elif fam == sf.F32N:
        raw = _f32n_targets()
    else:
        raw = {}
    return {name: [F32(v) for v in np.asarray(vals, np.float32).reshape(-1)] for name, vals in raw.items()}


# classes with one value (or a fixed handful): every one of them must be made; of the others 2 % may be missed
SINGLE = ("rail_in", "rail_at", "rail_out", "far_out", "clip", "min_sub", "overflow", "z_subnormal", "carry", "reassoc")


def wanted_for(formats=hm.ALL, kinds=dm.KINDS):
    """the list craft() takes: [((family name, kind name, class), target)] of every family among `formats`, without
    dither and with each of `kinds`; the few-valued classes first, so that none of them lies in a stream's last tile"""
    items = []
    seen = set()
    for fmt in formats:
        fam = family(fmt)
        if fam in seen:
            continue
        seen.add(fam)
        for kind in (dm.NONE,) + tuple(kinds):
            for name, vals in targets(fmt, kind, SEEDS.get(kind, 0)).items():
                items += [((hm.name(fam), dm.KIND_NAMES[kind], name), v) for v in vals]
    if dm.TRIANGULAR in kinds:
        items.append((("all", dm.KIND_NAMES[dm.TRIANGULAR], "reassoc"), reassoc_target(SEEDS[dm.TRIANGULAR])))
    count = {}
    for label, _ in items:
        count[label] = count.get(label, 0) + 1
    return sorted(items, key=lambda it: (count[it[0]] > 16))      # (stable: the order within each half stays)


def labels_of(fmt, kind):
    """which (family, kind) labels of a plan are decision points of format fmt written with dither kind `kind`"""
    fam, st = family(fmt), stage(fmt)
    own = {(hm.name(fam), dm.KIND_NAMES[dm.NONE])}
    if st is not None:
        own.add((hm.name(st), dm.KIND_NAMES[dm.NONE]))
        if kind != dm.NONE:
            own |= {(hm.name(fam), dm.KIND_NAMES[kind]), (hm.name(st), dm.KIND_NAMES[kind])}
            if kind == dm.TRIANGULAR:
                own.add(("all", dm.KIND_NAMES[kind]))
    return own


# ---- crafting --------------------------------------------------------------------------------------------------------
class Plan(list):
    """[(class, output k, channel, target)] and .missed = [(class, target)] that no tap tried could make"""
    missed = ()


def rows32(model):
    """the taps the fast kernels multiply by: the model's rows rounded once to fp32 (the direct kinds' are fp32 already)"""
    return np.asarray(model.rows, np.float64).astype(np.float32)


def spacing(model):
    """frames between the window starts of consecutive planned outputs: impulses end up taps + 3 apart at least"""
    order = np.argsort(-np.abs(rows32(model)), axis=1, kind="stable")[:, :TAPS_TRIED]
    return model.taps + 3 + int(order.max() - order.min())


def room_for(model, max_frames):
    """how many targets one stream of max_frames frames holds"""
    return max(0, (max_frames - 3 * model.taps - 16) // spacing(model))


def _amplitudes(r32, order, phase, tg):
    """per target: (amplitude, tap index) with fl32(tap * amplitude) == target bit for bit, tap index -1 where none of the
    window's TAPS_TRIED largest taps has one within +- ULPS ulp of fl32(target / tap)"""
    amp = np.zeros(tg.size, np.float32)
    tap_j = np.full(tg.size, -1, np.int64)
    deltas = [0] + [s * u for u in range(1, ULPS + 1) for s in (1, -1)]
    t64 = tg.astype(np.float64)
    with np.errstate(all="ignore"):
        for rank in range(TAPS_TRIED):
            j = order[phase, rank]
            tap = r32[phase, j].astype(np.float64)
            a0 = (t64 / tap).astype(np.float32)
            for dlt in deltas:
                a = (a0.view(np.int32) + np.int32(dlt)).view(np.float32)
                fine = np.isfinite(a) & (np.abs(a) >= F32(2.0 ** -126)) & (tap != 0)
                hit = fine & ((tap * a.astype(np.float64)).astype(np.float32).view(np.uint32) == tg.view(np.uint32)) & (tap_j < 0)
                amp[hit], tap_j[hit] = a[hit], j[hit]
    return amp, tap_j


def craft(model, ch, wanted, first_index=0, search=1 << 22, rounds=3):
    """One impulse per target, taps + 3 frames apart at least, the channels in turn: -> (x float32 [frames, ch], plan).
    wanted: [(class, float32 target | At)].  A target's designated output k is tried under the window's four largest
    taps, +- 8 ulp of fl32(target / tap) each; amplitudes are finite and normal.  What no tap makes is designated another
    output at the stream's end, of another phase where the filter has one (other taps), `rounds` times in all; what is
    left is plan.missed.  An At target with accept() takes the first output accept() allows (looked for over `search`
    sample indices) that can be made."""
    r32 = rows32(model)
    taps, num, den = model.taps, model.num, model.den
    assert model.last0 == 0 and model.frac0 == 0 and ch == model.channels
    order = np.argsort(-np.abs(r32), axis=1, kind="stable")[:, :TAPS_TRIED]
    gap = spacing(model)
    first_k = -(-(taps * den) // num)            # pos(k) >= taps: the impulse lies inside the input under any tap
    value = lambda n, k, c: F32(wanted[n][1].value(first_index + k * ch + c) if isinstance(wanted[n][1], At) else wanted[n][1])
    is_pinned = lambda n: isinstance(wanted[n][1], At) and wanted[n][1].accept is not None
    done = {}                                    # n -> (k, c, target, amplitude, tap index)

    # pinned targets (accept) first: the others fill the outputs around them
    taken = []                                   # window starts of the pinned outputs
    for n in filter(is_pinned, range(len(wanted))):
        idx = np.arange(first_index + first_k * ch, first_index + first_k * ch + search, dtype=np.uint64)
        for i in np.nonzero(wanted[n][1].accept(idx))[0]:
            k, c = int(i) // ch + first_k, int(i) % ch
            pos, t = k * num // den, np.array([value(n, k, c)], np.float32)
            amp, tap_j = _amplitudes(r32, order, np.array([k * num % den]), t)
            if tap_j[0] >= 0 and all(abs(pos - p) >= gap for p in taken):
                taken.append(pos)
                done[n] = (k, c, t[0], amp[0], int(tap_j[0]))
                break

    todo = [n for n in range(len(wanted)) if not is_pinned(n)]
    tried = {}
    free, turn = taps, 0
    for _ in range(rounds):
        where = {}
        for n in todo:
            k = max(first_k, -(-(free * den) // num))
            for _ in range(den):                 # (a phase this target has not been tried at, where there is one)
                if k * num % den not in tried.get(n, ()):
                    break
                k += 1
            pos = k * num // den
            while any(abs(pos - p) < gap for p in taken):      # (step over a pinned output's neighbourhood)
                k = -(-((max(p for p in taken if abs(pos - p) < gap) + gap) * den) // num)
                pos = k * num // den
            where[n] = (k, turn % ch)
            tried.setdefault(n, set()).add(k * num % den)
            turn += 1
            free = pos + gap
        ks = np.array([where[n][0] for n in todo], np.int64)
        tg = np.array([value(n, *where[n]) for n in todo], np.float32)
        amp, tap_j = _amplitudes(r32, order, ks * num % den, tg)
        for i, n in enumerate(todo):
            if tap_j[i] >= 0:
                done[n] = where[n] + (tg[i], amp[i], int(tap_j[i]))
        missed = [(wanted[n][0], tg[i]) for i, n in enumerate(todo) if tap_j[i] < 0]
        todo = [n for i, n in enumerate(todo) if tap_j[i] < 0]
        if not todo:
            break

    ns = sorted(done, key=lambda n: done[n][0])
    ks = np.array([done[n][0] for n in ns], np.int64)
    cs = np.array([done[n][1] for n in ns], np.int64)
    at = ks * num // den + np.array([done[n][4] for n in ns], np.int64) - (taps - 1)      # the impulses' frames
    assert (at >= 0).all()
    x = np.zeros(((int((ks * num // den).max()) if ns else 0) + taps + 8, ch), np.float32)
    x[at, cs] = np.array([done[n][3] for n in ns], np.float32)
    if len(ns) > 1:
        assert np.diff(np.sort(at)).min() >= taps + 3, "impulses closer than taps + 3 frames"
    plan = Plan((wanted[n][0], done[n][0], done[n][1], done[n][2]) for n in ns)
    plan.missed = (missed if todo else []) + [(wanted[n][0], None) for n in range(len(wanted)) if is_pinned(n) and n not in done]
    return x, plan


def streams(model, ch, wanted, first_index=0, max_frames=300000):
    """craft() over as many streams of at most max_frames frames as the targets need: [(x, plan)]; every stream starts a
    fresh state, so first_index is the same for each.  Pinned (accept) targets go to the first stream."""
    per = room_for(model, max_frames) - 40       # (room to step over the pinned outputs, and for second tries)
    assert per > 0
    pinned = [w for w in wanted if isinstance(w[1], At) and w[1].accept is not None]
    rest = [w for w in wanted if not (isinstance(w[1], At) and w[1].accept is not None)]
    size = -(-len(rest) // max(1, -(-len(rest) // per)))      # spread evenly: no stream is a short leftover
    parts = [rest[i: i + size] for i in range(0, len(rest), size)] or [[]]
    out = []
    for i, part in enumerate(parts):
        limit = (size + 4) * spacing(model) * model.den // model.num * ch
        out.append(craft(model, ch, (pinned if i == 0 else []) + part, first_index, search=max(limit, 1)))
        assert out[-1][0].shape[0] <= max_frames
    return out


def chain32_at(model, x, ks, cs):
    """exact_model.chain32 at chosen outputs only: rows rounded once to fp32, one sequential fp32 FMA chain, tap 0 first"""
    r = rows32(model).astype(np.float64)
    line = model.line(x)
    ks, cs = np.asarray(ks, np.int64), np.asarray(cs, np.int64)
    pos, phase = model.where(ks)
    s = np.zeros(ks.size, np.float32)
    for j in range(model.taps):
        s = (r[phase, j] * line[pos + j, cs] + s.astype(np.float64)).astype(np.float32)
    return s


def counts(plan, mask=None):
    """{class: planned points}, over the plan entries mask (a bool per entry) selects"""
    out = {}
    for i, (label, k, c, t) in enumerate(plan):
        if mask is None or mask[i]:
            out[label] = out.get(label, 0) + 1
    return out


# ---- the streams of the tests ------------------------------------------------------------------------------------------
# (channels, in, out, quality), info()["fast_path"], the modes the GPU tests run it in.  The interpolating filter runs in
# the default mode only: exact mode blends four dot products there, so a planned output is no single product.
FILTERS = (((1, 8000, 16000, 7), 3, ("default", "exact")),       # slide, direct
           ((2, 56000, 48000, 7), 2, ("default", "exact")),      # period kernel on the folded view, direct
           ((1, 24000, 48000, 10), 4, ("default", "exact")),     # fp64 slide
           ((2, 44100, 48000, 7), 2, ("default",)))              # period, interpolating
MAX_FRAMES = 300000
CONVERT_TILE, SIDES_TILE = 4096, 1024      # samples per tile of the converting passes, frames per tile of the plane passes


@functools.lru_cache(maxsize=None)
def crafted(cfg):
    """(model, [(x, plan)]) of one filter: every format's decision points, both dither kinds, states that start at
    output frame START; streams of at most MAX_FRAMES frames"""
    model = em.Model(*cfg)
    return model, streams(model, cfg[0], wanted_for(), START * cfg[0], MAX_FRAMES)


def in_whole_tiles(plan, ch, made, tile_samples=None, tile_frames=None):
    """per plan entry: does it lie in a whole tile of a pass over `made` frames -- the 16-bytes-per-lane path of an
    aligned call; the rest of an aligned call and all of an offset one take the element path"""
    k = np.array([p[1] for p in plan], np.int64)
    c = np.array([p[2] for p in plan], np.int64)
    if tile_frames is not None:
        return k < made // tile_frames * tile_frames
    return k * ch + c < made * ch // tile_samples * tile_samples


# ---- the encoders, with planted defects ----------------------------------------------------------------------------------
DEFECTS = ("half_even", "clamp_before_dither", "rail_off_by_one", "f16_toward_zero", "f16_subnormals_flushed",
           "f16_overflow_at_65504", "bf16_truncated", "bf16_half_away", "g711_stage_truncated", "g711_boundary_moved",
           "dither_reassociated", "z_subnormal_flushed")
# the formats (families) a defect can show in, and the dither kind it needs (None: without dither)
DEFECT_SCOPE = {
    # (no A-law byte can tell: every A-law code begins at an even int16, where half-even and half-up agree)
    "half_even": (INT_FAMILIES + (gm.ULAW,), dm.NONE),
    # (without dither the two orders agree; the companded codes are flat for a whole segment below the int16 rails)
    "clamp_before_dither": (INT_FAMILIES, dm.TRIANGULAR),
    "rail_off_by_one": (INT_FAMILIES, dm.NONE),
    "f16_toward_zero": ((hm.F16N,), dm.NONE),
    "f16_subnormals_flushed": ((hm.F16N,), dm.NONE),
    "f16_overflow_at_65504": ((hm.F16N,), dm.NONE),
    "bf16_truncated": ((hm.BF16N,), dm.NONE),
    "bf16_half_away": ((hm.BF16N,), dm.NONE),
    "g711_stage_truncated": (gm.COMPANDED, dm.NONE),
    "g711_boundary_moved": (gm.COMPANDED, dm.NONE),
    "dither_reassociated": (INT_FAMILIES + gm.COMPANDED, dm.TRIANGULAR),
    "z_subnormal_flushed": ((sf.F32N, hm.BF16N), dm.NONE),
}


def _integer_stage(st, y, d, defect):
    """the integer q of float32 y in family st with dither d (float64 array or None), as int64 after the clamp"""
    scale, lo, hi = INT_RULE[st]
    y = np.asarray(y, np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = y.astype(np.float64) * scale
        if defect == "clamp_before_dither":
            v = np.clip(v, lo, hi)
        if d is None:
            t = v
        elif defect == "dither_reassociated":
            t = None
            r = np.floor(v + (np.asarray(d, np.float64) + 0.5))
        else:
            t = v + np.asarray(d, np.float64)
        if t is not None:
            if defect == "half_even":
                r = np.rint(t)
            elif defect == "g711_stage_truncated":
                r = np.trunc(t)
            else:
                r = np.floor(t + 0.5)
        if defect == "rail_off_by_one":         # the upper clamp one too far, the stored integer wraps
            r = np.clip(r, lo, hi + 1)
            r = np.where(r > hi, lo, r)
        r = np.where(np.isnan(r), 0.0, np.clip(r, lo, hi))
    return r.astype(np.int64)


def _f16_bits(z, defect):
    bits = hm.f16_bits(z)
    z = np.asarray(z, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        back = bits.view(np.float16).astype(np.float32)
        if defect == "f16_toward_zero":
            over = np.isfinite(z) & ((np.abs(back) > np.abs(z)) | np.isinf(back))
            bits = np.where(over, bits - np.uint16(1), bits).astype(np.uint16)      # (one code towards zero)
        elif defect == "f16_subnormals_flushed":
            bits = np.where((bits & np.uint16(0x7C00)) == 0, bits & np.uint16(0x8000), bits).astype(np.uint16)
        elif defect == "f16_overflow_at_65504":
            bits = np.where(np.isfinite(z) & (np.abs(z) > 65504.0), np.uint16(0x7C00) | (bits & np.uint16(0x8000)), bits).astype(np.uint16)
    return bits


def _bf16_bits(z, defect):
    if defect not in ("bf16_truncated", "bf16_half_away"):
        return hm.bf16_bits(z)
    z = np.asarray(z, np.float32).reshape(-1)
    u = z.view(np.uint32).astype(np.uint64)
    r = (u if defect == "bf16_truncated" else u + np.uint64(0x8000)) >> np.uint64(16)
    nan = np.uint64(0x7FC0) | ((u >> np.uint64(16)) & np.uint64(0x8000))
    return np.where(np.isnan(z), nan, r).astype(np.uint16)


def encode(fmt, y, kind=dm.NONE, seed=0, position=0, c_out=1, defect=None):
    """The bytes (flat uint8) a call that starts at output frame `position` writes for the float32 frames y in format
    fmt: halfbe_model.from_internal / from_internal_dither restated so that one DEFECT can be planted; defect=None is
    those functions' bytes (test_cpu_decision_points asserts it)."""
    y = np.asarray(y, np.float32).reshape(-1)
    fam = family(fmt)
    if fam == sf.F32:
        return hm.raw(fmt, y.copy())
    if stage(fmt) is None:
        with np.errstate(all="ignore"):
            z = y * F32(1.0 / 32768.0)
            if defect == "z_subnormal_flushed":
                z = np.where(np.abs(z) < F32(2.0 ** -126), np.copysign(F32(0), z), z).astype(np.float32)
        if fam == sf.F32N:
            return hm.raw(fmt, z)
        bits = _f16_bits(z, defect) if fam == hm.F16N else _bf16_bits(z, defect)
        return hm.raw(fmt, bits.view(hm.dtype(fmt)))
    d = None if kind == dm.NONE else dm.values(kind, seed, (int(position) * c_out) & dm.M64, y.size)
    q = _integer_stage(stage(fmt), y, d, defect)
    if fam in gm.COMPANDED:
        codes = gm.encode(fam, q)
        if defect == "g711_boundary_moved":      # one boundary one int16 up: its first int16 still gets the lower code
            b = int(boundaries(fam)[100])
            codes = np.where(q == b, gm.encode(fam, [b - 1])[0], codes).astype(np.uint8)
        return codes
    st = sf.store(fam, q + (128 if fam == sf.U8 else 0))
    return hm.raw(fmt, hm.be_of(fmt, st) if fmt in hm.BIG else st)
