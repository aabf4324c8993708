"""Every device sample encoder at its decision points, through each kernel unit that compiles it.

The other GPU files feed the encoders the FIR of noise: exact ties of the half-up rule, the last value inside a rail, a
binary16 tie, the first int16 of a G.711 code or a dithered sum a few ulp from a tie are met there by chance or never.
Here the float twin's output holds them by construction (tests/decision_points.py: one impulse per wanted value, its
amplitude chosen so that the single product tap * A IS the value), on four filters -- the slide kernel, the period
kernel on a folded view, the fp64 slide kernel and the interpolating period kernel -- and every output format goes
through the convert unit (host form; device form aligned: whole 4096-sample tiles take the 16-bytes-per-lane path; device
form one sample off: the element path), the mix unit, the sides unit (planar output, aligned and one sample off) and the
many-states unit, without dither and with both dither kinds from a position just below 2^32.  Every comparison is
equality of bytes with halfbe_model.from_internal / from_internal_dither of the twin's output; there are no tolerances in
this file.  The only counted conditions are decision_points' own (test_cpu_decision_points.py), asserted again on the
twin's output: every planned output holds its target.  Run with -s for how many planned points of each format and class
each route saw."""
import hashlib

import numpy as np
import pytest

import channel_mix as cm
import decision_points as dp
import dither_model as dm
import halfbe_model as hm
import sample_formats as sf
import speexhip
from test_gpu_halfbe import device_call
from test_gpu_planar import wcap

pytestmark = pytest.mark.gpu

MODES = {"default": None, "exact": speexhip.MODE_EXACT}
CASES = [(cfg, path, mode) for cfg, path, modes in dp.FILTERS for mode in modes]
CASE_IDS = ["%dch-%d-%d-q%d-%s" % (c[0] + (c[2],)) for c in CASES]
SENTINEL = speexhip.Resampler.SENTINEL_BYTE
DITHERED = [f for f in hm.ALL if hm.dithered(f)]
NEGATE = np.float32([[1.0], [-1.0]])      # a mono state's two output rows: every target and its mirror image
IDENTITY = np.float32([[1.0, 0.0], [0.0, 1.0]])
_TWIN, _WANT = {}, {}


class Part:
    """one crafted stream of a filter and what the float twin made of it"""

    def __init__(self, cfg, mode, x, plan):
        ch, fi, fo, q = cfg
        self.cfg, self.mode, self.x, self.plan = cfg, mode, x, plan
        self.frames, self.cap = x.shape[0], wcap(x.shape[0], fi, fo)
        t = speexhip.Resampler(ch, fi, fo, q, mode=MODES[mode])
        rc, used, made, out = t.raw_call("float", x, self.cap)
        assert (rc, used) == (0, self.frames), (cfg, mode, rc, used)
        self.made, self.y = made, out[:made].copy()
        self.fast_path, self.state = t.info()["fast_path"], state_of(t)
        t.close()
        self.digest = hashlib.sha1(self.y.tobytes()).hexdigest()
        self._device = None

    def device_x(self, torch):
        if self._device is None:
            self._device = torch.from_numpy(self.x).cuda()
            assert self._device.data_ptr() % 16 == 0
        return self._device


def state_of(r):
    return r.positions(), r.info()["magic_samples"], r.history().tobytes()


def twin(cfg, mode):
    if (cfg, mode) not in _TWIN:
        _TWIN[(cfg, mode)] = [Part(cfg, mode, x, plan) for x, plan in dp.crafted(cfg)[1]]
    return _TWIN[(cfg, mode)]


def want(part, fmt, kind=dm.NONE, mix=None):
    """the bytes of the twin's output (through the output matrix `mix`) in format fmt, from a state dithered with `kind`
    at decision_points' seed and starting position"""
    key = (part.digest, fmt, kind, None if mix is None else mix.tobytes())
    if key not in _WANT:
        with np.errstate(all="ignore"):
            y = part.y if mix is None else cm.mix(mix, part.y)
            st = hm.from_internal_dither(fmt, y.reshape(-1), kind, dp.SEEDS.get(kind, 0), dp.START, y.shape[1])
        _WANT[key] = hm.raw(fmt, st).tobytes()
    return _WANT[key]


def fresh(part, kind=dm.NONE):
    ch, fi, fo, q = part.cfg
    r = speexhip.Resampler(ch, fi, fo, q, mode=MODES[part.mode])
    if kind != dm.NONE:
        assert r.set_dither(kind, dp.SEEDS[kind], dp.START) == 0
    return r


def finish(r, part, kind, made, what):
    assert state_of(r) == part.state, what
    if kind != dm.NONE:
        assert r.get_dither() == (kind, dp.SEEDS[kind], dp.START + made), what
    r.close()


def produced(out, fmt, made, c_out, what):
    raw = out.view(np.uint8)
    n = made * c_out * hm.nbytes(fmt)
    assert (raw[n:] == SENTINEL).all(), str(what) + ": written past produced"
    return raw[:n].tobytes()


def device_buffer(room, off, torch):
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    return dst, dst.data_ptr() + 16 + off


def device_bytes(dst, off, n, what):
    flat = dst.cpu().numpy()
    lo = 16 + off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), str(what) + ": bytes outside the produced samples written"
    return flat[lo: lo + n].tobytes()


class Seen:
    """planned points of each (format, class) a route saw, by path"""

    def __init__(self, route):
        self.route, self.n = route, {}

    def add(self, part, fmt, kind, path, mask=None):
        own = dp.labels_of(fmt, kind)
        for label, n in dp.counts(part.plan, mask).items():
            if label[:2] in own:
                key = (hm.name(fmt), dm.KIND_NAMES[kind], label[2], path)
                self.n[key] = self.n.get(key, 0) + n

    def report(self, case_id):
        rows = {}
        for (fmt, kind, name, path), n in sorted(self.n.items()):
            rows.setdefault((fmt, kind), []).append("%s@%s=%d" % (name, path, n))
        for (fmt, kind), cells in rows.items():
            print("%s %s %s/%s: %s" % (case_id, self.route, fmt, kind, " ".join(cells)))

    def assert_every_class_on(self, fmts, kinds, paths):
        """each class of each format's decision points lies on each of `paths`"""
        for fmt in fmts:
            for kind in kinds:
                classes = set(k[2] for k in self.n if k[:2] == (hm.name(fmt), dm.KIND_NAMES[kind]))
                assert classes or fmt in (sf.F32,), (self.route, hm.name(fmt), kind)
                for name in classes:
                    for path in paths:
                        assert self.n.get((hm.name(fmt), dm.KIND_NAMES[kind], name, path), 0) > 0, (self.route, hm.name(fmt), kind, name, path)


def case_id(cfg, mode):
    return "%dch-%d-%d-q%d-%s" % (cfg + (mode,))


# ---- the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_float_twin_emits_every_planned_target(cfg, fast_path, mode):
    """the counted conditions of decision_points, on the GPU's own float output: the filter runs on the kernel family it
    stands for, and every planned output IS its target -- a family that does not return the single product fails here"""
    model, parts = dp.crafted(cfg)
    asked = dp.counts([(w[0], 0, 0, 0) for w in dp.wanted_for()])
    made = {}
    for part in twin(cfg, mode):
        assert part.fast_path == fast_path, (cfg, mode, part.fast_path)
        assert part.frames <= dp.MAX_FRAMES
        ks, cs = np.array([p[1] for p in part.plan]), np.array([p[2] for p in part.plan])
        tg = np.array([p[3] for p in part.plan], np.float32)
        assert ks.max() < part.made
        bad = np.nonzero(part.y[ks, cs].view(np.uint32) != tg.view(np.uint32))[0]
        assert bad.size == 0, (cfg, mode, bad.size, [(part.plan[i], part.y[ks[i], cs[i]]) for i in bad[:5]])
        for label, n in dp.counts(part.plan).items():
            made[label] = made.get(label, 0) + n
    for label, n in asked.items():
        assert made.get(label, 0) >= (n if label[2] in dp.SINGLE else 0.98 * n), (label, made.get(label, 0), n)
    print("%s: %d planned outputs hold their targets" % (case_id(cfg, mode), sum(made.values())))


# ---- the convert unit ----------------------------------------------------------------------------------------------------------
def convert_host(part, fmt, kind, seen):
    what = (part.cfg, part.mode, "convert host", hm.name(fmt), kind)
    r = fresh(part, kind)
    rc, used, made, out = r.fmt_call(part.x, sf.F32, fmt, part.cap)
    assert (rc, used, made) == (0, part.frames, part.made), what
    assert produced(out, fmt, made, part.cfg[0], what) == want(part, fmt, kind), what
    finish(r, part, kind, made, what)
    seen.add(part, fmt, kind, "host")


def convert_device(part, fmt, kind, seen, offsets, torch):
    ch = part.cfg[0]
    stream = torch.cuda.current_stream().cuda_stream
    for off in offsets:         # samples off a 16-byte boundary: 0 = whole tiles by 16 bytes per lane, 1 = the element path
        what = (part.cfg, part.mode, "convert device", hm.name(fmt), kind, off)
        r = fresh(part, kind)
        dst, ptr = device_buffer(part.cap * ch * hm.nbytes(fmt), off * hm.nbytes(fmt), torch)
        used, made = r.process_fmt_device(sf.F32, part.device_x(torch).data_ptr(), part.frames, fmt, ptr, part.cap, stream)
        torch.cuda.synchronize()
        assert (used, made) == (part.frames, part.made), what
        assert device_bytes(dst, off * hm.nbytes(fmt), made * ch * hm.nbytes(fmt), what) == want(part, fmt, kind), what
        finish(r, part, kind, made, what)
        tiles = dp.in_whole_tiles(part.plan, ch, made, tile_samples=dp.CONVERT_TILE)
        if off == 0:
            seen.add(part, fmt, kind, "lanes16", tiles)
            seen.add(part, fmt, kind, "element", ~tiles)
        else:
            seen.add(part, fmt, kind, "element")


@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_convert_unit_host_form(cfg, fast_path, mode):
    seen = Seen("convert-host")
    for part in twin(cfg, mode):
        for fmt in hm.ALL:
            convert_host(part, fmt, dm.NONE, seen)
    seen.assert_every_class_on(hm.ALL, (dm.NONE,), ("host",))
    seen.report(case_id(cfg, mode))


@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_convert_unit_device_form_on_both_paths(cfg, fast_path, mode):
    import torch
    seen = Seen("convert-device")
    for part in twin(cfg, mode):
        for fmt in hm.ALL:
            convert_device(part, fmt, dm.NONE, seen, (0, 1), torch)
    seen.assert_every_class_on(hm.ALL, (dm.NONE,), ("lanes16", "element"))
    seen.report(case_id(cfg, mode))


@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_convert_unit_with_dither(cfg, fast_path, mode):
    """rectangular and triangular on every dithered format, states that start at output frame 2^32 - 1000: the host form
    (whole tiles and a tail) and the device form one sample off"""
    import torch
    seen = Seen("convert-dither")
    for part in twin(cfg, mode):
        for kind in dm.KINDS:
            for fmt in DITHERED:
                convert_host(part, fmt, kind, seen)
                convert_device(part, fmt, kind, seen, (1,), torch)
    seen.assert_every_class_on(DITHERED, dm.KINDS, ("host", "element"))
    seen.report(case_id(cfg, mode))


# ---- the mix unit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_mix_unit(cfg, fast_path, mode):
    """a mono state with the output matrix [[1], [-1]]: row 1 is every target negated -- exact negative ties and the
    lower rail's mirror image; a stereo state with the 2 x 2 identity.  The host form and the device form one sample off."""
    import torch
    ch = cfg[0]
    out_mix = NEGATE if ch == 1 else IDENTITY
    c_out = out_mix.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    seen = Seen("mix")
    for part in twin(cfg, mode):
        for fmt in hm.ALL:
            what = (cfg, mode, "mix", hm.name(fmt))
            r = fresh(part)
            rc, used, made, out = r.mix_call(part.x, sf.F32, fmt, None, out_mix, part.cap)
            assert (rc, used, made) == (0, part.frames, part.made), what
            assert produced(out, fmt, made, c_out, what) == want(part, fmt, dm.NONE, out_mix), what
            finish(r, part, dm.NONE, made, what)
            r = fresh(part)
            off = hm.nbytes(fmt)
            dst, ptr = device_buffer(part.cap * c_out * hm.nbytes(fmt), off, torch)
            used, made = r.process_mix_device(sf.F32, part.device_x(torch).data_ptr(), part.frames, fmt, ptr, part.cap, None, out_mix, stream)
            torch.cuda.synchronize()
            assert (used, made) == (part.frames, part.made), what
            assert device_bytes(dst, off, made * c_out * hm.nbytes(fmt), what) == want(part, fmt, dm.NONE, out_mix), what
            finish(r, part, dm.NONE, made, what)
            seen.add(part, fmt, dm.NONE, "host")
            seen.add(part, fmt, dm.NONE, "element")
    seen.assert_every_class_on(hm.ALL, (dm.NONE,), ("host", "element"))
    seen.report(case_id(cfg, mode))


# ---- the sides unit ------------------------------------------------------------------------------------------------------------
def sides_device(part, fmt, kind, seen, offsets, torch):
    """interleaved float in, planes of fmt out: planes at 16-byte multiples (whole 1024-frame tiles by 16 bytes per lane)
    and planes one sample off (the element path)"""
    ch = part.cfg[0]
    bo = hm.nbytes(fmt)
    stream = torch.cuda.current_stream().cuda_stream
    for off in offsets:
        what = (part.cfg, part.mode, "sides", hm.name(fmt), kind, off)
        stride = (part.cap + 15) // 16 * 16 + 16 + off
        d_out = torch.full(((off + ch * stride) * bo + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        a = speexhip.make_side(sf.F32, ch, data=part.device_x(torch).data_ptr())
        b = speexhip.make_side(fmt, ch, speexhip.LAYOUT_PLANAR, None, d_out.data_ptr() + off * bo, stride)
        r = fresh(part, kind)
        used, made = r.process_sides_device(a, part.frames, b, part.cap, stream)
        torch.cuda.synchronize()
        assert (used, made) == (part.frames, part.made), what
        buf = d_out.cpu().numpy()
        touched = np.zeros(buf.size, bool)
        planes = []
        for c in range(ch):
            at = (off + c * stride) * bo
            planes.append(buf[at: at + made * bo].reshape(made, bo))
            touched[at: at + made * bo] = True
        assert np.stack(planes, axis=1).tobytes() == want(part, fmt, kind), what
        assert (buf[~touched] == SENTINEL).all(), what
        finish(r, part, kind, made, what)
        tiles = dp.in_whole_tiles(part.plan, ch, made, tile_frames=dp.SIDES_TILE)
        if off == 0:
            seen.add(part, fmt, kind, "lanes16", tiles)
            seen.add(part, fmt, kind, "element", ~tiles)
        else:
            seen.add(part, fmt, kind, "element")


@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_sides_unit_on_both_paths(cfg, fast_path, mode):
    import torch
    seen = Seen("sides")
    for part in twin(cfg, mode):
        for fmt in hm.ALL:
            sides_device(part, fmt, dm.NONE, seen, (0, 1), torch)
    seen.assert_every_class_on(hm.ALL, (dm.NONE,), ("lanes16", "element"))
    seen.report(case_id(cfg, mode))


@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_sides_unit_with_dither(cfg, fast_path, mode):
    import torch
    seen = Seen("sides-dither")
    for part in twin(cfg, mode):
        for kind in dm.KINDS:
            for fmt in DITHERED:
                sides_device(part, fmt, kind, seen, (0, 1), torch)
    seen.assert_every_class_on(DITHERED, dm.KINDS, ("lanes16", "element"))
    seen.report(case_id(cfg, mode))


# ---- the many-states unit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,fast_path,mode", CASES, ids=CASE_IDS)
def test_many_states_unit(cfg, fast_path, mode):
    """thirteen states of the filter, one per output format, in one speexhip_resampler_process_many_fmt call served by the
    fused passes; then with a dither kind per state, and once more with the kinds swapped, so that every dithered format
    meets both"""
    ch = cfg[0]
    n = len(hm.ALL)
    seen = Seen("many")
    for part in twin(cfg, mode):
        for kinds in ([dm.NONE] * n, [dm.KINDS[i % 2] for i in range(n)], [dm.KINDS[(i + 1) % 2] for i in range(n)]):
            states = [fresh(part, kinds[i]) for i in range(n)]
            outs = [np.full(part.cap * ch * hm.nbytes(f), SENTINEL, np.uint8) for f in hm.ALL]
            c0 = speexhip.many_counters()
            rc, used, made, codes = speexhip.many_fmt_call(states, [sf.F32] * n, [part.x.ctypes.data] * n, [part.frames] * n,
                                                           list(hm.ALL), [o.ctypes.data for o in outs], [part.cap] * n)
            c1 = speexhip.many_counters()
            d = {k: c1[k] - c0[k] for k in c0}
            assert rc == 0 and codes == [0] * n, (cfg, mode, rc, codes)
            assert d["own_calls"] == 0 and d["fir_launches"] >= 1 and d["out_passes"] >= 1, d
            for i, fmt in enumerate(hm.ALL):
                what = (cfg, mode, "many", hm.name(fmt), kinds[i])
                assert (used[i], made[i]) == (part.frames, part.made), what
                assert produced(outs[i], fmt, made[i], ch, what) == want(part, fmt, kinds[i]), what
                finish(states[i], part, kinds[i], made[i], what)
                seen.add(part, fmt, kinds[i] if hm.dithered(fmt) else dm.NONE, "fused")
    seen.assert_every_class_on(hm.ALL, (dm.NONE,), ("fused",))
    seen.assert_every_class_on(DITHERED, dm.KINDS, ("fused",))
    seen.report(case_id(cfg, mode))


# ---- the decoder side ------------------------------------------------------------------------------------------------------------
def wide_codes(bits):
    """integers of a wide format whose conversion to float32 decides something: for 32 bits the int32 -> float ties (the
    dropped bits exactly half, kept mantissas of both parities), their neighbours, and the ends of the range; 24-bit
    integers are all exact in float32 -- the ends, +-1 and a spread"""
    top = 1 << (bits - 1)
    v = [1, -1, top - 1, -top, top - 2, -top + 1, 0x123456 % top, -(0x654321 % top)]
    if bits == 32:
        for p in range(24, 31):
            u = 1 << (p - 23)                  # the spacing of float32 in [2^p, 2^(p+1))
            for m in (2, 3, 1000, 1001, (1 << 23) - 2, (1 << 23) - 1):
                tie = (1 << p) + m * u + u // 2
                v += [tie, tie - 1, tie + 1, -tie, -tie - 1, -tie + 1]
        v += [top - 64, top - 65, top - 63, -top + 64, -top + 65, -top + 63]
    return np.array([w for w in v if -top <= w < top], np.int64)


@pytest.mark.parametrize("fmt", (sf.S24, sf.S32, hm.S24BE, hm.S32BE), ids=["s24", "s32", "s24be", "s32be"])
def test_wide_integer_decoders_at_their_rounding_ties(fmt):
    """one code per impulse, taps + 3 frames apart, F32 out: every output under an impulse is fl32(tap * decoded), so a
    decode that rounds the other way moves the float image by an ulp and the bytes show it.  The host form (whole tiles by
    16 bytes per lane, and a tail) and the device form with the input one sample off (the element path)."""
    import torch
    ch, fi, fo, q = cfg = (1, 8000, 16000, 7)
    le = hm.LE_TWIN.get(fmt, fmt)
    codes = wide_codes(8 * hm.nbytes(fmt))
    codes = np.random.RandomState(24 + fmt).permutation(np.tile(codes, -(-260 // codes.size)))      # (every path holds a mix)
    t = speexhip.Resampler(*cfg)
    gap = t.taps + 3
    values = np.zeros((codes.size + 1) * gap, np.int64)
    values[gap::gap] = codes
    st = sf.store(le, values)
    st = hm.be_of(fmt, st) if fmt in hm.BIG else st
    x = hm.to_internal(fmt, st)
    exact = x.astype(np.float64) * (256.0 if le == sf.S24 else 65536.0) == values
    assert exact.all() if le == sf.S24 else (~exact).sum() >= 200      # (the 32-bit ties and their neighbours are rounded)
    assert values.size % 4096 > 8 * gap
    frames = values.size
    cap = wcap(frames, fi, fo)
    rc_t, used_t, made_t, out_t = t.raw_call("float", x, cap)
    assert rc_t == 0 and used_t == frames and frames > 2 * 4096
    y = out_t[:made_t].reshape(-1)
    r = speexhip.Resampler(*cfg)
    rc, used, made, out = r.fmt_call(st, fmt, sf.F32, cap)
    assert (rc, used, made) == (rc_t, used_t, made_t), hm.name(fmt)
    assert produced(out, sf.F32, made, ch, hm.name(fmt)) == y.tobytes(), hm.name(fmt)
    assert state_of(r) == state_of(t)
    r.close()
    r = speexhip.Resampler(*cfg)
    used, made, got = device_call(r, fmt, st, sf.F32, cap, ch, ch, hm.nbytes(fmt), 0, torch)
    assert (used, made) == (used_t, made_t) and got.tobytes() == y.tobytes(), hm.name(fmt)
    assert state_of(r) == state_of(t)
    r.close()
    t.close()
