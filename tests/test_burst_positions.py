"""Stretch-relative positions above 2^32 in the burst chain (burst resampler, burst AIS, POCSAG and FLEX), through the state
entries (mfm_run*_fetch_state / mfm_run*_store_state) and, without a device, through the host twins, which take their state
from the caller.

The shift.  Call 0 runs from position 0.  In the state it leaves, B is added to the stretch-relative position fields of every
channel that has a stretch (resampler: outs; AIS: outs and the positions its mode uses, pos and r in SEARCH, rd and start in
RECEIVE; POCSAG: outs, its other fields are relative or saturating; FLEX: outs and the position its mode uses, p in SEARCH
and j otherwise, and the ring rotated by B mod 32768; the positions a mode does not use are zero by the canonical form of
the state), and to nothing else.  The later calls must return what the oracle per stretch
(the Checker classes of test_runrs, test_runais, test_runpocsag and test_runflex, run ONCE at base 0) returns, with B added
to first_out of the continuing runs and to sample, start_sample and sync_sample (of a FRAME) of the events of a shifted
stretch, up to that channel's next run that begins a stretch: stretches that begin later are unshifted, and both kinds stand
in one call.  A uniform shift keeps every difference between positions and changes the outcome of every comparison against an
absolute position, so every shifted stretch is at least 4096 outputs old at the shift: more than the 2400 samples of POCSAG
history, the 256 of AIS and the 320 + 311 of FLEX.

The scene: four channels of PCM at the decoders' rate, W = 64, through the ratios 1/1 (4 taps) and 4/5 (41 taps): 0: POCSAG,
2400 baud, two batches (kept and lost sync word) and a transmission soon behind the loss; 1: AIS, busy, with a silent hole;
2: FLEX, a damaged A word, a coding 0 frame, a damaged A word; 3: a 1200 baud POCSAG transmission, then the channel closes
and a fresh stretch begins with AIS packets and a 2400 baud POCSAG transmission.  Channels 0 - 2 stay open across all calls.
The decoders are fed run lists cut by hand from the oracle resampler's output per stretch, so that a call can end at any
output; the burst resampler is fed the gate's calls, and the device chain runs behind it.

Bases: 2^33 + 12345, 2^40 + 1, 2^61 + 1 and 2^32 - d with d read off the Checker's base-0 events (PLACES below).  Each runs as
one call behind call 0 and as ragged calls that end at stretch positions 2^32 - 1, 2^32 and 2^32 + 1.  The guards (no GPU)
assert on the Checker's events alone that every place finds its d and that events lie on both sides of 2^32 in a stretch
that began before it.

The summary skip has a scene of its own (skip_scene): one channel, a transmission, an idle stretch that the POCSAG and the
FLEX walker cross in whole steps of 65 536 samples, a second transmission; 2^32 lies inside a whole step, whose ends are
derived from MFM_RUNPOCSAG_HIST_WORDS and MFM_RUNFLEX_HIST_WORDS as test_burst_scale.py derives them."""
import numpy as np
import pytest

import test_ais as ta
import test_burst_scale as tbs
import test_flex as tf
import test_pocsag as tp
import test_run_bits as trb
import test_runais as tra
import test_runflex as trf
import test_runpocsag as trp
import test_runrs as tr
import test_seek_positions as tsp

T32 = 1 << 32
NCH, W = 4, 64
N = 76000                      # samples per channel at the decoders' rate
L0 = 4321                      # outputs of call 0 (the decoders' crafted calls)
OLD = 4096
RING = 32768
BIGGEST = 20000                # the longest ragged call
RATIOS = [(1, 1, 4), (4, 5, 41)]
RID = lambda r: f"{r[0]}_{r[1]}"
FIXED = {"2^33": (1 << 33) + 12345, "2^40": (1 << 40) + 1, "2^61": (1 << 61) + 1}
STAGES = ["runais", "runpocsag", "runflex"]
MOD = {"runais": tra, "runpocsag": trp, "runflex": trf}
MAIN = {"runais": 1, "runpocsag": 0, "runflex": 2}   # the channel that carries the stage's protocol and stays open
DERIVED = {"runais": ["straddle", "on", "before", "after", "idle"],
           "runpocsag": ["straddle", "on", "before", "after", "syncword", "exact"],
           "runflex": ["bs1", "straddle", "on_sync", "on", "before", "after", "idle"],
           "runrs": ["inside", "first", "last"]}
CUTS = ["one", "ragged"]
EV_POS = {"runais": ("sample", "start_sample"), "runpocsag": ("sample",), "runflex": ("sample", "sync_sample")}
FRAME = 1
FORMS = {"runais": ["pcm", "bits", "alternating"], "runpocsag": ["pcm", "bits", "alternating"], "runflex": ["pcm"]}
POLARITY = {"runais": trb.POS, "runpocsag": trb.NEG}
CASES = [(s, p) for s in STAGES for p in list(FIXED) + DERIVED[s]]
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class _AsIs:
    """in the place of a decoder Checker's resampler checker: the run list is the crafted one"""

    def call(self, runs, payload):
        return runs, payload


# ---- the scene ------------------------------------------------------------------------------------------------------

def scene(pkg, ora, ratio):
    def make():
        sy = pkg.synth
        I, D, _ = ratio
        rng = np.random.RandomState(23)
        x = (rng.randn(NCH, N) * 60).round().astype(np.int16)
        msgs = tp._messages(sy)
        two = sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches(msgs[:2]), preamble_bits=128), 2400, noise=300, seed=1)
        x[0, 5000:5000 + two.size] = two
        q, _ = trp._tx(sy, ora, "short2400", 2)
        at = 5000 + two.size + 700
        x[0, at:at + q.size] = q
        x[1, 1000:] = ta._busy(sy, 31, N - 1000)
        x[1, 30000:34000] = (rng.randn(4000) * 60).round().astype(np.int16)
        bad = sy.flex_pcm([sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)], lead=50, noise=200, seed=5)[:3000]
        f = sy.flex_pcm(tf._frames(sy, 0, 1), noise=300, seed=3)
        x[2, 4400:4400 + bad.size] = bad
        x[2, 9000:9000 + f.size] = f
        x[2, 41000:41000 + bad.size] = bad
        p, _ = trp._tx(sy, ora, "one1200", 1)
        x[3, 4500:4500 + p.size] = p
        x[3, 46500:52500] = ta._busy(sy, 32, 6000)
        q, _ = trp._tx(sy, ora, "short2400", 4)
        x[3, 54000:54000 + q.size] = q
        n_in = N * D // I
        stream = np.ascontiguousarray(np.stack([np.repeat(r, D)[::I][:n_in] for r in x]))
        mask = np.ones((NCH, n_in // W), bool)
        mask[3, 44000 * D // I // W:46000 * D // I // W] = False
        taps = trp.rs_taps(pkg, ora, ratio)
        # the oracle resampler's output per stretch, from the whole stream as one gate call
        whole = tr.gate_calls(pkg, stream, mask, W, 0, [n_in])
        rs = tr.Checker(pkg, ora, taps, I, D, False, W)
        rs.call(*whole[0])
        ys = rs.stretches()
        keys = sorted(ys)
        assert [k[0] for k in keys] == [0, 1, 2, 3, 3] and keys[3][1] == 0
        ny = ys[keys[0]].size
        assert ys[keys[1]].size == ny and ys[keys[2]].size == ny
        ya, yb = ys[keys[3]], ys[keys[4]]
        assert ya.size > L0 + OLD and ya.size + 100 < ny - yb.size
        # (channel, where the stretch lies on the common time line, first window, outputs)
        lay = [(k[0], 0, k[1], ys[k]) for k in keys[:4]] + [(3, ny - yb.size, keys[4][1], yb)]
        return dict(ratio=ratio, stream=stream, mask=mask, n_in=n_in, taps=taps, lay=lay, ny=ny)
    return cached(("scene", ratio), make)


def crafted_calls(pkg, sc, ends):
    """the run lists [(runs, payload)] of calls that end at the time-line positions `ends`"""
    out, t0 = [], 0
    for t1 in ends:
        runs, parts, off = [], [], 0
        for c, g0, win, y in sc["lay"]:
            lo, hi = max(t0, g0), min(t1, g0 + y.size)
            if lo < hi:
                runs.append((win, off, lo - g0, c, hi - lo, int(lo == g0), 0))
                parts.append(y[lo - g0:hi - g0])
                off += hi - lo
        out.append((np.array(runs, pkg.binding.RUNRS_RUN_DTYPE), np.concatenate(parts) if parts else np.zeros(0, np.int16)))
        t0 = t1
    assert t0 == sc["ny"]
    return out


def ends_of(sc, kind, d, biggest=BIGGEST):
    """call 0 ends at L0; behind it one call, or ragged ones with ends at d - 1, d and d + 1"""
    if kind == "one":
        return (L0, sc["ny"])
    rest = [m for m in tsp.ragged(sc["ny"] - L0, (d - 1 - L0, d - L0, d + 1 - L0), biggest, 7) if m]
    ends = (L0 + np.cumsum(rest)).tolist()
    if L0 + 1 < d < sc["ny"] - 1:
        assert d - 1 in ends and d in ends and d + 1 in ends
    return (L0,) + tuple(ends)


def wanted(pkg, ora, sc, stage, ends):
    """(calls, the stage Checker's result per call) at base 0"""
    def make():
        calls = crafted_calls(pkg, sc, ends)
        chk = MOD[stage].Checker(pkg, ora, sc["taps"], sc["ratio"][0], sc["ratio"][1], W)
        chk.rs = _AsIs()
        want = [chk.call(*c)[1] for c in calls]
        chk.stretches()   # each stretch once more through a fresh decoder in one piece
        return calls, want
    return cached(("want", sc.get("name"), sc["ratio"], stage, ends), make)


def events_of(stage, want):
    return np.concatenate([w[0] if stage == "runflex" else w for w in want])


def places(pkg, ora, sc, stage):
    """d per derived place and what the guard reads, from the Checker's events of the stage's own channel at base 0"""
    def make():
        _, want = wanted(pkg, ora, sc, stage, (L0, sc["ny"]))
        ev = events_of(stage, want)
        ev = ev[ev["channel"] == MAIN[stage]]
        s = ev["sample"].astype(np.int64)
        if stage == "runais":
            a = ev["start_sample"].astype(np.int64)
            k = len(ev) // 3
            e = int(s[2 * len(ev) // 3])
            g = int(np.argmax(a[1:] - s[:-1]))
            idle = (int(s[g]), int(a[g + 1]))
            assert idle[1] - idle[0] > 2000 and a[k] > L0
            d = dict(straddle=(int(a[k]) + int(s[k])) // 2, on=e, before=e - 1, after=e + 1, idle=(idle[0] + idle[1]) // 2)
            span = dict(straddle=(int(a[k]), int(s[k])), idle=idle)
        elif stage == "runpocsag":
            t = ev["type"].tolist()
            F, B, K, L = ora.EV_SYNC_FOUND, ora.EV_BATCH, ora.EV_SYNC_KEPT, ora.EV_SYNC_LOST
            assert t[:5] == [F, B, K, B, L] and F in t[5:] and B in t[5:], t
            e = int(s[1])
            assert int(s[5]) - int(s[4]) > trp.HIST   # the search behind the loss outlasts the EXACT span
            d = dict(straddle=(int(s[0]) + int(s[1])) // 2 + 1, on=e, before=e - 1, after=e + 1, syncword=(int(s[1]) + int(s[2])) // 2,
                     exact=int(s[4]) + 1001)
            span = dict(straddle=(int(s[0]), int(s[1])), syncword=(int(s[1]), int(s[2])), exact=(int(s[4]), int(s[4]) + 31 * 75))
        else:
            t = ev["type"].tolist()
            assert t == [trf.BAD_BAUD, FRAME, trf.BAD_BAUD], t
            y, e = int(ev["sync_sample"][1]), int(s[1])
            idle = (int(s[0]) + trf.DEAD, y - 1110 - 400)   # behind the first event's dead time, in front of the frame's BS1
            assert idle[1] - idle[0] > 1000
            d = dict(bs1=y - 600, straddle=(y + e) // 2, on_sync=y, on=e, before=e - 1, after=e + 1, idle=(idle[0] + idle[1]) // 2)
            span = dict(bs1=(y - 1110, y), straddle=(y, e), idle=idle)
        for place in DERIVED[stage]:
            assert place in d, (stage, place)                      # every place finds its d
            assert L0 + 1 < d[place] < sc["ny"] - 1, (stage, place, d[place])
        assert any(v % 2 for v in d.values()) and any(v % 32 for v in d.values())
        return dict(d=d, span=span, on=e, samples=s)
    return cached(("places", sc["ratio"], stage), make)


def base_of(pkg, ora, sc, stage, place):
    return FIXED[place] if place in FIXED else T32 - places(pkg, ora, sc, stage)["d"][place]


def guard(pkg, ora, sc, stage, place, kind):
    """from the Checker alone: where the events of the shifted stretches lie around 2^32; returns (base, ends)"""
    pl = places(pkg, ora, sc, stage)
    base = base_of(pkg, ora, sc, stage, place)
    d = pl["d"].get(place, 0)
    ends = ends_of(sc, kind, d)
    assert all(g0 != 0 or y.size >= L0 + OLD for _, g0, _, y in sc["lay"])   # every shifted stretch is old enough ...
    assert L0 >= OLD
    s = pl["samples"][pl["samples"] >= L0] + base
    if place in FIXED:
        assert s.size >= 3 and (s >= T32).all()
        return base, ends
    assert base + d == T32 and (s < T32).any() and (s >= T32).any(), (stage, place)
    if place in pl["span"]:
        lo, hi = pl["span"][place]
        assert base + lo < T32 <= base + hi, (stage, place)
    if place in ("on", "before", "after"):
        assert base + pl["on"] == T32 + {"on": 0, "before": 1, "after": -1}[place]
    if stage == "runflex" and place == "straddle" and kind == "ragged":
        lo, hi = pl["span"]["straddle"]   # the frame's block lies partly in the ring and partly in the run, 2^32 inside it
        assert sum(lo < e <= hi for e in ends) >= 3
    return base, ends


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("stage,place", CASES)
def test_checker_events_lie_on_both_sides_of_2_to_the_32(pkg, ora, stage, place, ratio, kind):
    sc = scene(pkg, ora, ratio)
    base, ends = guard(pkg, ora, sc, stage, place, kind)
    _, want = wanted(pkg, ora, sc, stage, ends)
    ev = events_of(stage, want)
    fresh = sc["lay"][4][2]
    assert (ev["stretch_window"] == fresh).any() or stage == "runflex"    # the fresh stretch has events of its own
    calls, _ = wanted(pkg, ora, sc, stage, ends)
    both = [r for r, _ in calls[1:] if ((r["flags"] & 1) == 1).any() and ((r["flags"] & 1) == 0).any()]
    assert both                                                            # shifted and fresh stretches in one call


# ---- the shift --------------------------------------------------------------------------------------------------------

def live_of(stage, state):
    if stage == "runrs":
        return state["expected"] != np.uint64(0xffffffffffffffff)
    return state["has_stretch"] == 1


def pos_fields(stage, state):
    """per position field, the channels in which the state's mode uses it"""
    every = np.ones(len(state), bool)
    if stage == "runrs" or stage == "runpocsag":
        return {"outs": every}
    if stage == "runais":
        return {"outs": every, "pos": state["mode"] == 0, "r": state["mode"] == 0, "rd": state["mode"] == 1, "start": state["mode"] == 1}
    return {"outs": every, "p": state["mode"] == 0, "j": state["mode"] != 0}


def shift_state(stage, state, base, on=None, ring=None):
    """B added to the position fields of the channels `on` (default: those with a stretch), the FLEX ring rotated"""
    out = state.copy()
    on = live_of(stage, state) if on is None else on
    for f, used in pos_fields(stage, state).items():
        out[f][on & used] += np.uint64(base)
    if ring is None:
        return out
    ring = ring.copy()
    ring[on] = np.roll(ring[on], base % RING, axis=1)
    return out, ring


class Shift:
    """what the later calls take and must return at base B, from the base-0 lists"""

    def __init__(self, stage, base, on):
        self.stage, self.base, self.on = stage, np.uint64(base), on.copy()

    def runs(self, runs):
        out, flag = runs.copy(), np.zeros(len(runs), bool)
        for i, r in enumerate(runs):
            c = int(r["channel"])
            if int(r["flags"]) & 1:
                self.on[c] = False
            flag[i] = self.on[c]
        out["first_out"][flag] += self.base
        return out, flag

    def events(self, want, flag):
        ev = (want[0] if self.stage == "runflex" else want).copy()
        hit = flag[ev["run"]] if len(ev) else np.zeros(0, bool)
        for f in EV_POS[self.stage]:
            sel = hit & (ev["type"] == FRAME) if f == "sync_sample" else hit
            ev[f][sel] += self.base
        return (ev, want[1]) if self.stage == "runflex" else ev


def final_state(stage, state0, base, on, ring0=None, ring=None):
    """the base-0 state after the last call with B added for the channels whose stretch is still the shifted one; for FLEX the
    got ring is compared here: rotated where the stretch is the shifted one, slot by slot where a fresh stretch wrote it"""
    want = shift_state(stage, state0, base, on=on & live_of(stage, state0))
    if ring0 is not None:
        for c in range(len(state0)):
            if on[c]:
                assert np.array_equal(ring[c], np.roll(ring0[c], base % RING)), c
            else:
                n = min(int(state0["outs"][c]), RING)
                assert np.array_equal(ring[c][:n], ring0[c][:n]) or n == RING and np.array_equal(ring[c], ring0[c]), c
    return want


def twin_call(pkg, stage, state, runs, payload, form):
    b = pkg.binding
    if form == "bits":
        r2, bits = trb.pack(pkg, runs, payload, POLARITY[stage])
        return getattr(b, f"hosttwin_{stage}_call_bits")(state, r2, bits, POLARITY[stage])
    return getattr(b, f"hosttwin_{stage}_call")(state, runs, payload)


def form_of(form, i):
    return ("pcm", "bits")[i % 2] if form == "alternating" else form


def check_state(pkg, stage, state):
    getattr(pkg.binding, f"hosttwin_{stage}_state_check")(state[0] if stage == "runflex" else state)


def twin_run(pkg, stage, calls, want, base, form, collect=None):
    """the twin through all calls, shifted by `base` behind call 0 (None: not at all); returns its final state"""
    b = pkg.binding
    state = getattr(b, f"hosttwin_{stage}_state")(NCH)
    sh = None
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        flag = np.zeros(len(runs), bool)
        if sh is not None:
            runs, flag = sh.runs(runs)
            w = sh.events(w, flag)
        got = twin_call(pkg, stage, state, runs, payload, form_of(form, i))
        MOD[stage].same(got, w, f"{stage} twin at {base}, {form}, call {i}")
        check_state(pkg, stage, state)
        if collect is not None:
            collect.append((stage, (state[0] if stage == "runflex" else state).copy()))
        if i == 0 and base is not None:
            st = state[0] if stage == "runflex" else state
            live = live_of(stage, st)
            assert live.any() and (st["outs"][live] == L0).all()
            sh = Shift(stage, base, live)
            if stage == "runflex":
                state = shift_state(stage, state[0], base, ring=state[1])
            else:
                state = shift_state(stage, state, base)
            check_state(pkg, stage, state)
    return state, (sh.on if sh else None)


def base0(pkg, ora, sc, stage, ends, form="pcm"):
    def make():
        calls, want = wanted(pkg, ora, sc, stage, ends)
        return twin_run(pkg, stage, calls, want, None, form)[0]
    return cached(("base0", sc.get("name"), sc["ratio"], stage, ends, form), make)


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("stage,place", CASES)
def test_hosttwin_decoder_behind_a_shifted_state(pkg, ora, stage, place, ratio, kind):
    """the decoder's twin on the oracle resampler's output per stretch: call 0, the shift, the later calls against the Checker's
    shifted results; PCM form, and for AIS and POCSAG the bits form and both in turn; the state after the last call is the
    base-0 state with B added to the same fields; the validator accepts every state on the way"""
    sc = scene(pkg, ora, ratio)
    base, ends = guard(pkg, ora, sc, stage, place, kind)
    calls, want = wanted(pkg, ora, sc, stage, ends)
    s0 = base0(pkg, ora, sc, stage, ends)
    for form in FORMS[stage]:
        state, on = twin_run(pkg, stage, calls, want, base, form)
        assert on[:3].all() and not on[3]
        if stage == "runflex":
            exp = final_state(stage, s0[0], base, on, s0[1], state[1])
            state = state[0]
        else:
            exp = final_state(stage, s0, base, on)
        assert state.tobytes() == exp.tobytes(), (form, [f for f in exp.dtype.names if not np.array_equal(state[f], exp[f])])


# ---- the summary skip: 2^32 inside a whole step of 65 536 samples ---------------------------------------------------------

SKIP_STAGES = ["runpocsag", "runflex"]
SKIP_BIGGEST = 200000   # a ragged call may hold a whole step


def skip_scene(pkg, ora, stage):
    """one channel, 1/1: a transmission whose events lie behind call 0, an idle stretch of more than two summary steps, a second
    transmission whose first match is the first thing the walker finds.  [e1, e2) is a whole step of the search that opens
    behind the first transmission, 2^32 goes to e1 + 30 001"""
    def make():
        flex = stage == "runflex"
        taps = tbs._taps(ora)
        span = 32500 if flex else 15000
        t0 = 5000 + (8 if flex else 12)
        n = t0 + 2 * span + 3 * 65536
        kinds = [tbs.BAD_BAUD, None] if flex else None
        x = tbs._idle_channel(pkg, ora, stage, taps, n, 31, [t0], kinds=kinds)
        y = ora.Resampler(taps, 1, 1).feed(x)
        p = tbs._searches(ora, stage, y)[1][1]   # where the search opens behind the first transmission's last event
        assert L0 < p < t0 + span
        e1, e2 = tbs.flex_step_ends(L0, p, 2) if flex else tbs.pocsag_step_ends(L0, p, 2, rst=p)
        target = e2 + (2016 + 8 if flex else 4000 + 12)
        x = tbs._idle_channel(pkg, ora, stage, taps, n, 31, [t0, target], kinds=kinds)
        y = ora.Resampler(taps, 1, 1).feed(x)
        ev, searches = tbs._searches(ora, stage, y)
        assert searches[1] == p and tbs._first_hit(stage, y, p) == target and e2 - e1 == 65536 and target + span < y.size
        if flex:
            assert not tbs.flex_m(y)[p:target].any()
        else:   # no summary bit between the search's start and the step's end
            assert not [w for w in tbs.pocsag_flagged(y, L0, y.size - L0) if p <= w < e2]
        d = e1 + 30001
        at = ev["sample"].astype(np.int64)
        assert ((at > L0) & (at < d)).any() and (at > d).any() and e1 < d < e2
        return dict(name="skip " + stage, ratio=(1, 1, 4), taps=taps, lay=[(0, 0, 7, y)], ny=y.size, d=d, step=(e1, e2))
    return cached(("skip", stage), make)


def skip_case(pkg, ora, stage, kind):
    sc = skip_scene(pkg, ora, stage)
    base = T32 - sc["d"]
    ends = ends_of(sc, kind, sc["d"], SKIP_BIGGEST)
    e1, e2 = sc["step"]
    if kind == "one":
        assert base + e1 < T32 < base + e2 and not [e for e in ends if e1 <= e <= e2]   # one call holds the whole step
    calls, want = wanted(pkg, ora, sc, stage, ends)
    return sc, base, ends, calls, want


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("stage", SKIP_STAGES)
def test_hosttwin_summary_step_across_2_to_the_32(pkg, ora, stage, kind):
    sc, base, ends, calls, want = skip_case(pkg, ora, stage, kind)
    s0 = base0(pkg, ora, sc, stage, ends)
    state, on = twin_run(pkg, stage, calls, want, base, "pcm")
    assert on.tolist() == [True, False, False, False]
    if stage == "runflex":
        exp = final_state(stage, s0[0], base, on, s0[1], state[1])
        state = state[0]
    else:
        exp = final_state(stage, s0, base, on)
    assert state.tobytes() == exp.tobytes()


# ---- the burst resampler: the gate's calls ----------------------------------------------------------------------------

RS_CUTS = {"one": (0.1, 1.0), "ragged": (0.1, 0.27, 0.5, 0.5, 0.81, 1.0)}   # call ends as parts of the stream, whole windows


def rs_scene(pkg, ora, sc, kind):
    """the gate's calls and the resampler Checker's results at base 0; d per place from the runs of channel 0"""
    def make():
        n_in = sc["n_in"]
        ends = [int(f * n_in) // W * W + (17 if 0 < f < 1 and kind == "ragged" else 0) for f in RS_CUTS[kind]]
        ends[-1] = n_in
        cuts = np.diff([0] + ends).tolist()
        calls = tr.gate_calls(pkg, sc["stream"], sc["mask"], W, 0, cuts)
        chk = tr.Checker(pkg, ora, sc["taps"], sc["ratio"][0], sc["ratio"][1], False, W)
        want = [chk.call(*c) for c in calls]
        chk.stretches()
        first = want[0][0]
        assert (first["flags"] == 1).all() and (first["nr_out"] >= OLD).all() and len(first) == NCH
        r = [w[0][w[0]["channel"] == 0] for w in want[1:] if len(w[0])]
        r = r[(len(r) - 1) // 2]
        assert len(r) == 1 and int(r["flags"][0]) == 0 and int(r["nr_out"][0]) > 100
        fo, n = int(r["first_out"][0]), int(r["nr_out"][0])
        d = dict(inside=fo + n // 2 + 1, first=fo, last=fo + n - 1)
        both = [w[0] for w in want[1:] if (w[0]["flags"] == 1).any() and (w[0]["flags"] == 0).any()]
        assert both   # shifted and fresh stretches in one call
        return dict(calls=calls, want=want, d=d, run=(fo, n))
    return cached(("rs", sc["ratio"], kind), make)


def rs_shift(want, sh):
    (runs, payload) = want
    runs, _ = sh.runs(runs)
    return runs, payload


def rs_twin_run(pkg, sc, rs, base, dc_pole=None):
    b = pkg.binding
    I, D, _ = sc["ratio"]
    state, pending = b.hosttwin_runrs_state(NCH, len(sc["taps"]), I)
    dc = np.zeros(NCH, b.RUNRS_DC_STATE_DTYPE)
    sh, outs = None, []
    for i, (g, w) in enumerate(zip(rs["calls"], rs["want"])):
        if sh is not None:
            w = rs_shift(w, sh)
        got = b.hosttwin_runrs_call(W, sc["taps"], I, D, state, pending, *g)
        tr.same(got, w, f"resampler twin at {base}, call {i}")
        if dc_pole is not None:
            outs.append(b.hosttwin_runrs_dc_call(dc_pole, dc, got[0], got[1].copy()))
        b.hosttwin_runrs_state_check(state, I, pending.shape[1], dc)
        if i == 0 and base is not None:
            live = live_of("runrs", state)
            assert live.all()
            sh = Shift("runrs", base, live)
            state = shift_state("runrs", state, base)
    return state, pending, dc, outs, (sh.on if sh else None)


RS_CASES = list(FIXED) + DERIVED["runrs"]


def rs_base(rs, place):
    if place in FIXED:
        return FIXED[place]
    fo, n = rs["run"]
    base = T32 - rs["d"][place]
    assert base + fo <= T32 < base + fo + n and (place != "first" or base + fo == T32) and (place != "last" or base + fo + n - 1 == T32)
    return base


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("place", RS_CASES)
def test_hosttwin_resampler_behind_a_shifted_state(pkg, ora, place, ratio, kind):
    """mfm_hosttwin_runrs_call on the gate's calls with `outs` shifted behind call 0: first_out of the continuing runs is B
    further, payload, phase and pending are those of base 0, and so is the DC blocker's output behind it"""
    sc = scene(pkg, ora, ratio)
    rs = rs_scene(pkg, ora, sc, kind)
    base = rs_base(rs, place)
    s0, p0, dc0, outs0, _ = cached(("rs0", ratio, kind), lambda: rs_twin_run(pkg, sc, rs, None, dc_pole=0.999))
    dc_pole = 0.999 if place == "inside" else None
    state, pending, dc, outs, on = rs_twin_run(pkg, sc, rs, base, dc_pole=dc_pole)
    assert on[:3].all() and not on[3]
    exp = final_state("runrs", s0, base, on)
    assert state.tobytes() == exp.tobytes() and np.array_equal(pending, p0)
    if dc_pole is not None:
        assert dc.tobytes() == dc0.tobytes() and len(outs) == len(outs0)
        for a, c in zip(outs, outs0):
            assert np.array_equal(a, c)


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("place", RS_CASES)
def test_hosttwin_chain_behind_a_shifted_resampler(pkg, ora, place, ratio, kind):
    """mfm_hosttwin_runrs_call and the three decoders' twins behind it on the gate's calls, every state shifted by the same B
    behind call 0, against the Checkers' shifted results; at the "inside" place the Checkers' events of every decoder's own
    channel lie on both sides of 2^32"""
    sc = scene(pkg, ora, ratio)
    rs = rs_scene(pkg, ora, sc, kind)
    base = rs_base(rs, place)
    I, D, _ = ratio
    decoders = {s: MOD[s].Checker(pkg, ora, sc["taps"], I, D, W) for s in STAGES}
    _, _, on = gpu_rs_run(pkg, None, sc, rs, base, decoders=decoders)
    assert on[:3].all() and not on[3]
    for s in STAGES if place == "inside" else ():
        parts = [p[0] if isinstance(p, tuple) else p for p in decoders[s].by[(MAIN[s], 0)]]
        at = np.concatenate(parts)["sample"].astype(np.uint64) + np.uint64(base)
        assert (at < T32).any() and (at >= T32).any(), s


# ---- the validators ---------------------------------------------------------------------------------------------------

def _twin_states(pkg, ora):
    """states the twins produce over the scenes of the four stage tests: (stage, state) after every call"""
    b = pkg.binding
    out = []
    for mod, stage, sc_of in ((tra, "runais", lambda r: tra.scene(pkg, r)), (trp, "runpocsag", lambda r: trp.scene(pkg, ora, r, 64)),
                              (trf, "runflex", lambda r: trf.scene(pkg, ora, r, 64))):
        for ratio in mod.RATIOS:
            sc = sc_of(ratio)
            I, D, _ = ratio
            taps = mod.rs_taps(pkg, ora, ratio)
            nw = sc["n_in"] // 64
            rng = np.random.RandomState(3)
            mask = np.ones((mod.NCH, nw), bool)
            for c in range(mod.NCH):   # seeded closed blocks: stretches end and begin in every walker state
                for k in rng.randint(0, nw, 6):
                    mask[c, k:k + 1 + int(rng.randint(0, 4))] = False
            cuts = tr.make_cuts(rng, sc["n_in"], 64, False)
            rstate, pending = b.hosttwin_runrs_state(mod.NCH, len(taps), I)
            state = getattr(b, f"hosttwin_{stage}_state")(mod.NCH)
            for g in tr.gate_calls(pkg, sc["stream"], mask, 64, 0, cuts):
                rs = b.hosttwin_runrs_call(64, taps, I, D, rstate, pending, *g)
                getattr(b, f"hosttwin_{stage}_call")(state, *rs)
                out.append(("runrs", (rstate.copy(), I, pending.shape[1])))
                out.append((stage, (state[0] if stage == "runflex" else state).copy()))
    sc = scene(pkg, ora, RATIOS[0])   # and over this file's scene, whose ragged calls end inside every walker state
    for stage in STAGES:
        for place in DERIVED[stage]:
            calls, want = wanted(pkg, ora, sc, stage, ends_of(sc, "ragged", places(pkg, ora, sc, stage)["d"][place]))
            twin_run(pkg, stage, calls, want, None, "pcm", collect=out)
    return out


def test_validators_accept_what_the_twins_produce(pkg, ora):
    b = pkg.binding
    seen = {}
    for stage, st in cached("twin states", lambda: _twin_states(pkg, ora)):
        if stage == "runrs":
            b.hosttwin_runrs_state_check(*st)
            st = st[0]
        else:
            getattr(b, f"hosttwin_{stage}_state_check")(st)
        if stage != "runrs":
            seen.setdefault(stage, set()).update(int(m) for m in st["mode"][st["has_stretch"] == 1])
    assert seen == {"runais": {0, 1}, "runpocsag": {0, 2, 3}, "runflex": {0, 1, 2}}   # every mode of every walker was checked


def _good(pkg, ora, stage, mode):
    """a state the twin produced with a channel in `mode`, that channel first"""
    for s, st in cached("twin states", lambda: _twin_states(pkg, ora)):
        if s == stage:
            hit = np.flatnonzero((st["has_stretch"] == 1) & (st["mode"] == mode) & (st["outs"] > 3000))
            if hit.size:
                return np.concatenate([st[hit[:1]], st[hit[:1]]])
    raise AssertionError((stage, mode))


BIG = 1 << 62
VIOLATIONS = {
    "runais": [(0, dict(has_stretch=2), "has_stretch"), (0, dict(has_stretch=0), "has_stretch"), (0, dict(reserved=1), "reserved"),
               (0, dict(outs=BIG, pos=BIG), "outs"), (0, dict(pos=BIG), "pos"), (0, dict(rd=BIG), "pos, r, rd and start"),
               (0, dict(start=BIG), "start"), (0, dict(mode=2), "mode"), (1, dict(last_sample=2), "last_sample"), (1, dict(hist8=256), "hist8"),
               (1, dict(cur_bit=1280), "cur_bit"), (0, dict(pos=-1), "pos must not be in front of outs"), (0, dict(r=+1), "r must not be behind pos"),
               (1, dict(rd=-6), "rd must not be in front of outs"), (1, dict(start=+100000), "start must not be behind rd"),
               (0, dict(cur_bit=1), "must be 0 in SEARCH"), (0, dict(rd=+3), "must be 0 in SEARCH"), (1, dict(pos=+5), "pos and r must be 0"),
               (0, dict(packet=1), "packet must be empty"), (1, dict(packet=1 << 31), "packet must hold no bit")],
    "runpocsag": [(0, dict(has_stretch=2), "has_stretch"), (0, dict(has_stretch=0), "has_stretch"), (0, dict(outs=BIG), "outs"),
                  (0, dict(mode=1), "mode"), (0, dict(spb=16), "baud, spb and skip"), (0, dict(skip=1), "baud, spb and skip"),
                  (0, dict(since_reset=2401), "since_reset"), (0, dict(nr_eye=1 << 31), "nr_eye"),
                  (2, dict(spb=17), "spb and baud"), (2, dict(baud=1200, spb=16), "spb and baud"), (2, dict(skip=65536), "skip"),
                  (2, dict(since_reset=1), "since_reset and nr_eye"), (2, dict(nr_eye=1), "since_reset and nr_eye"),
                  (2, dict(batch_word=16), "batch_word"), (2, dict(batch_bit=32), "batch_bit"), (2, dict(batch=1 << 31), "batch must hold no bit"),
                  (3, dict(batch_word=1), "batch_word and batch_bit"), (3, dict(batch=1), "batch must be empty"),
                  (3, dict(nr_sync_bits=32), "nr_sync_bits"), (3, dict(sync_word=0xffffffff), "sync_word"), (2, dict(nr_sync_bits=1), "nr_sync_bits and sync_word")],
    "runflex": [(0, dict(has_stretch=2), "has_stretch"), (0, dict(has_stretch=0), "has_stretch"), (0, dict(outs=BIG, p=BIG), "outs"),
                (0, dict(p=BIG), "p and j"), (0, dict(mode=3), "mode"), (0, dict(coding=1), "outside FRAME"), (0, dict(j=5), "j and eye"),
                (0, dict(eye=3), "j and eye"), (0, dict(p=-1), "p must not be in front of outs"), (0, dict(run=0xffffffff), "run"),
                (1, dict(p=5), "p and run"), (1, dict(eye=2), "eye"), (1, dict(eye=256), "eye"), (1, dict(j=-2000), "j must be in front of outs"),
                (1, dict(j=+4000), "j must be in front of outs"), (2, dict(coding=4), "coding"), (2, dict(sample_range=40000), "sample_range"),
                (2, dict(cycle=16), "cycle"), (2, dict(frame=128), "frame"), (2, dict(j=+1), "j must be in front of outs"),
                (2, dict(outs=+40000), "j must be in front of outs")],
}


def violate(state, change, channel=0):
    """a copy with one field of one channel changed.  A position below 2^61 is relative: to pos for r, to rd for start, to
    outs for the others; packet and batch get a bit set in their first (1) or last word"""
    bad = state.copy()
    for f, v in change.items():
        rel = f in ("outs", "pos", "r", "rd", "start", "p", "j") and v < (1 << 61)
        if f in ("packet", "batch"):
            bad[f][channel][-1 if v > 1 else 0] |= v
        elif f == "nr_eye":
            bad[f][channel][1] = v
        elif rel:
            ref = {"r": "pos", "start": "rd"}.get(f, "outs")
            bad[f][channel] = int(state[ref][channel]) + v
        else:
            bad[f][channel] = v
    return bad


def refused_by_check(pkg, check, state, field):
    with pytest.raises(pkg.MfmError) as ei:
        check(state)
    assert ei.value.code == pkg.binding.MFM_E_INVAL and field in str(ei.value) and "channel 0" in str(ei.value), (field, str(ei.value))


@pytest.mark.parametrize("stage", STAGES)
def test_validators_refuse_each_single_field_violation(pkg, ora, stage):
    check = getattr(pkg.binding, f"hosttwin_{stage}_state_check")
    for mode, change, field in VIOLATIONS[stage]:
        good = _good(pkg, ora, stage, mode)
        check(good)
        refused_by_check(pkg, check, violate(good, change), field)


def test_resampler_validator_refuses_each_single_field_violation(pkg, ora):
    b = pkg.binding
    state, I, plen = next(st for s, st in cached("twin states", lambda: _twin_states(pkg, ora)) if s == "runrs" and live_of("runrs", st[0]).all())
    dc = np.zeros(len(state), b.RUNRS_DC_STATE_DTYPE)
    b.hosttwin_runrs_state_check(state, I, plen, dc)
    for change, field in ((dict(phase=I), "phase"), (dict(pending=plen + 1), "pending"), (dict(outs=BIG), "outs"), (dict(expected=BIG), "expected"),
                          (dict(expected=0xffffffffffffffff), "expected is ~0")):
        bad = state.copy()
        bad["outs"][0] = max(int(bad["outs"][0]), 1)
        for f, v in change.items():
            bad[f][0] = v
        refused_by_check(pkg, lambda s: b.hosttwin_runrs_state_check(s, I, plen, dc), bad, field)
    bad = dc.copy()
    bad["reserved"][0] = 1
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runrs_state_check(state, I, plen, bad)
    assert "reserved" in str(ei.value)
    fresh, _ = b.hosttwin_runrs_state(3, 41, 4)
    b.hosttwin_runrs_state_check(fresh, 4, 12)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _stage_object(pkg, stage, sc):
    return getattr(pkg, {"runais": "RunAis", "runpocsag": "RunPocsag", "runflex": "RunFlex"}[stage])(NCH, 8, NCH * sc["ny"] + 1)


def _fed(pkg, torch, stage, obj, runs, payload, form):
    if form == "bits":
        r2, bits = trb.pack(pkg, runs, payload, POLARITY[stage])
        view, keep = trb._view_of(pkg, torch, r2, bits, POLARITY[stage])
        obj.process_bits_device(view)
        try:
            return obj.fetch()
        finally:
            del keep
    return MOD[stage]._fed(pkg, torch, obj, runs, payload)


def _same_state(stage, got, twin, what):
    if stage == "runflex":
        assert np.array_equal(got[1], twin[1]), what
        got, twin = got[0], twin[0]
    assert got.tobytes() == twin.tobytes(), (what, [f for f in twin.dtype.names if not np.array_equal(got[f], twin[f])])


def _store(stage, obj, state):
    obj.store_state(*state) if stage == "runflex" else obj.store_state(state)


def gpu_run(pkg, torch, stage, sc, calls, want, base, form, move_at=None):
    """the stage on the device beside its twin: call 0, fetch_state against the twin's, the shift, store_state, the later calls
    against the Checker's shifted results and the twin; move_at: the state goes into a fresh object behind that call"""
    b = pkg.binding
    obj = _stage_object(pkg, stage, sc)
    twin = getattr(b, f"hosttwin_{stage}_state")(NCH)
    sh = None
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        what = f"{stage} at {base}, {form}, call {i}"
        if sh is not None:
            runs, flag = sh.runs(runs)
            w = sh.events(w, flag)
        f = form_of(form, i)
        got = _fed(pkg, torch, stage, obj, runs, payload, f)
        MOD[stage].same(got, w, what)
        MOD[stage].same(twin_call(pkg, stage, twin, runs, payload, f), got, f"{what}, against its twin")
        _same_state(stage, obj.fetch_state(), twin, what)
        if i == 0 and base is not None:
            st = twin[0] if stage == "runflex" else twin
            sh = Shift(stage, base, live_of(stage, st))
            twin = shift_state(stage, twin[0], base, ring=twin[1]) if stage == "runflex" else shift_state(stage, twin, base)
            check_state(pkg, stage, twin)   # nothing is stored that the validator would refuse
            _store(stage, obj, twin)
            _same_state(stage, obj.fetch_state(), twin, f"{what}, stored")
            MOD[stage].same(obj.fetch(), got, f"{what}: the last call's events stay readable")
        if i == move_at:
            other = _stage_object(pkg, stage, sc)
            _store(stage, other, obj.fetch_state())
            obj.close()
            obj = other
    out = obj.fetch_state()
    obj.close()
    return out, twin


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("stage,place", CASES)
def test_gpu_decoder_behind_a_stored_shifted_state(pkg, ora, stage, place, ratio, kind):
    """call 0 on the device, fetch_state equal to the twin's, the shift, store_state, the later calls: every fetch against the
    Checker's shifted results and the twin beside it, the state after every call the twin's.  AIS and POCSAG with PCM and
    bits calls in turn"""
    import torch
    sc = scene(pkg, ora, ratio)
    base, ends = guard(pkg, ora, sc, stage, place, kind)
    calls, want = wanted(pkg, ora, sc, stage, ends)
    form = "pcm" if stage == "runflex" else "alternating"
    got, twin = gpu_run(pkg, torch, stage, sc, calls, want, base, form)
    _same_state(stage, got, twin, "after the last call")
    s0 = base0(pkg, ora, sc, stage, ends, form)
    on = np.array([True, True, True, False])
    if stage == "runflex":
        exp = final_state(stage, s0[0], base, on, s0[1], got[1])
        got = got[0]
    else:
        exp = final_state(stage, s0, base, on)
    assert got.tobytes() == exp.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("stage", SKIP_STAGES)
def test_gpu_summary_step_across_2_to_the_32(pkg, ora, stage, kind):
    """the walkers' summary skip with 2^32 inside a whole step of 65 536 samples, behind a stored shifted state"""
    import torch
    sc, base, ends, calls, want = skip_case(pkg, ora, stage, kind)
    got, twin = gpu_run(pkg, torch, stage, sc, calls, want, base, "pcm")
    _same_state(stage, got, twin, "after the last call")


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
def test_gpu_decoder_in_one_form_throughout(pkg, ora, stage):
    """the forms the case above leaves out, at the "on" place, ragged: PCM only and bits only for AIS and POCSAG"""
    import torch
    sc = scene(pkg, ora, RATIOS[1])
    base, ends = guard(pkg, ora, sc, stage, "on", "ragged")
    calls, want = wanted(pkg, ora, sc, stage, ends)
    for form in [f for f in FORMS[stage] if f != "alternating"]:
        got, twin = gpu_run(pkg, torch, stage, sc, calls, want, base, form)
        _same_state(stage, got, twin, form)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
def test_gpu_moving_a_decoders_stream_into_a_fresh_object(pkg, ora, stage):
    """object A runs calls 0 .. 3, its state is fetched and stored into a fresh object that runs the rest: every call's result
    and the final state are one object's (the Checker's and the twin's); store(fetch()) on a live object changes nothing"""
    import torch
    sc = scene(pkg, ora, RATIOS[0])
    ends = ends_of(sc, "ragged", places(pkg, ora, sc, stage)["d"]["on"])
    calls, want = wanted(pkg, ora, sc, stage, ends)
    assert len(calls) > 6
    got, twin = gpu_run(pkg, torch, stage, sc, calls, want, None, "pcm", move_at=3)
    _same_state(stage, got, twin, "after the last call")
    _same_state(stage, got, base0(pkg, ora, sc, stage, ends), "one object's")
    # store(fetch()) on a live object
    obj = _stage_object(pkg, stage, sc)
    twin = getattr(pkg.binding, f"hosttwin_{stage}_state")(NCH)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        got = _fed(pkg, torch, stage, obj, runs, payload, "pcm")
        MOD[stage].same(got, w, f"call {i}")
        st = obj.fetch_state()
        _store(stage, obj, st)
        _same_state(stage, obj.fetch_state(), st, i)
        MOD[stage].same(obj.fetch(), got, f"call {i}, fetched again behind the store")
    obj.close()


def _refused_store(pkg, store, field):
    with pytest.raises(pkg.MfmError) as ei:
        store()
    assert ei.value.code == pkg.binding.MFM_E_INVAL and (field is None or field in str(ei.value)), (field, str(ei.value))


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
def test_gpu_decoder_store_refusals_leave_the_state(pkg, ora, stage):
    """wrong nr_channels, NULL and one invalid field: MFM_E_INVAL, fetch_state unchanged, the next call right.  Only the store
    entry is called with them: no kernel runs on a refused state"""
    import torch
    sc = scene(pkg, ora, RATIOS[0])
    calls, want = wanted(pkg, ora, sc, stage, (L0, sc["ny"]))
    obj = _stage_object(pkg, stage, sc)
    MOD[stage].same(_fed(pkg, torch, stage, obj, *calls[0], "pcm"), want[0], "call 0")
    st = obj.fetch_state()
    state = st[0] if stage == "runflex" else st
    extra = (st[1],) if stage == "runflex" else ()
    _refused_store(pkg, lambda: obj.store_state(state[:3], *(e[:3] for e in extra), nr_channels=3), None)
    _refused_store(pkg, lambda: obj.store_state(None, *extra), None)
    if stage == "runflex":
        _refused_store(pkg, lambda: obj.store_state(state, None), None)
    bad = state.copy()
    bad["outs"][2] = 1 << 62
    _refused_store(pkg, lambda: obj.store_state(bad, *extra), "channel 2")
    bad = state.copy()
    bad["has_stretch"][1] = 2
    _refused_store(pkg, lambda: obj.store_state(bad, *extra), "has_stretch")
    _same_state(stage, obj.fetch_state(), st, "after the refused stores")
    MOD[stage].same(_fed(pkg, torch, stage, obj, *calls[1], "pcm"), want[1], "call 1 after the refused stores")
    obj.close()


# ---- GPU: the burst resampler and the chain behind it -------------------------------------------------------------------

def _rs_object(pkg, sc, dc_pole=None):
    I, D, _ = sc["ratio"]
    rr = pkg.RunResampler(NCH, sc["taps"], I, D, W, max_in_samples=sc["n_in"])
    if dc_pole is not None:
        rr.set_dc_block(dc_pole)
    return rr


def _same_rs_state(got, state, pending, dc, what):
    assert got[0].tobytes() == state.tobytes(), (what, [f for f in state.dtype.names if not np.array_equal(got[0][f], state[f])])
    for c in range(NCH):   # the samples behind `pending` are not part of the state
        k = int(state["pending"][c])
        assert np.array_equal(got[1][c, :k], pending[c, :k]), (what, c)
    if dc is not None:
        assert got[2].tobytes() == dc.tobytes(), what


def gpu_rs_run(pkg, torch, sc, rs, base, dc_pole=None, move_at=None, decoders=None):
    """the burst resampler on the device beside its twin (and the DC twin); decoders: {stage: Checker} for the chain behind its
    device view, every decoder's state shifted by the same B.  torch None: the twins alone, no device"""
    b = pkg.binding
    I, D, _ = sc["ratio"]
    dev = torch is not None
    rr = _rs_object(pkg, sc, dc_pole) if dev else None
    state, pending = b.hosttwin_runrs_state(NCH, len(sc["taps"]), I)
    dc = np.zeros(NCH, b.RUNRS_DC_STATE_DTYPE) if dc_pole is not None else None
    dec = {s: getattr(pkg, {"runais": "RunAis", "runpocsag": "RunPocsag", "runflex": "RunFlex"}[s]).behind(rr) if dev else None
           for s in decoders or {}}
    dtwin = {s: getattr(b, f"hosttwin_{s}_state")(NCH) for s in dec}
    sh, dsh = None, {}
    for i, (g, w) in enumerate(zip(rs["calls"], rs["want"])):
        what = f"resampler at {base}, call {i}"
        dwant = {s: decoders[s].call(*g)[1] for s in dec}   # base 0, from the gate's call
        if sh is not None:
            w = rs_shift(w, sh)
        twin = b.hosttwin_runrs_call(W, sc["taps"], I, D, state, pending, *g)
        if dc_pole is not None:
            twin = (twin[0], b.hosttwin_runrs_dc_call(dc_pole, dc, twin[0], twin[1].copy()))
            w = (w[0], twin[1])   # the DC twin's output: equal to base 0's in the CPU test
        got = tr._fed(pkg, torch, rr, *g) if dev else twin
        tr.same(got, w, what)
        tr.same(got, twin, f"{what}, against its twin")
        for s in dec:
            ww = dwant[s]
            if s in dsh:
                _, flag = dsh[s].runs(rs["want"][i][0])
                ww = dsh[s].events(ww, flag)
            dtw = twin_call(pkg, s, dtwin[s], *twin, "pcm")
            check_state(pkg, s, dtwin[s])
            if dev:
                dec[s].process_device(*rr.device_view())
                dgot = dec[s].fetch()
                MOD[s].same(dgot, ww, f"{what}, {s} behind the device view")
                MOD[s].same(dtw, dgot, f"{what}, {s} against its twin")
                _same_state(s, dec[s].fetch_state(), dtwin[s], f"{what}, {s}")
            else:
                MOD[s].same(dtw, ww, f"{what}, the {s} twin behind the resampler's")
        if dev:
            _same_rs_state(rr.fetch_state(), state, pending, dc, what)
        if i == 0 and base is not None:
            live = live_of("runrs", state)
            sh = Shift("runrs", base, live)
            state = shift_state("runrs", state, base)
            b.hosttwin_runrs_state_check(state, I, pending.shape[1], dc)
            if dev:
                rr.store_state(state, pending, dc)
                _same_rs_state(rr.fetch_state(), state, pending, dc, f"{what}, stored")
                tr.same(rr.fetch(), got, f"{what}: the last call's result stays readable")
            for s in dec:
                t = dtwin[s]
                dsh[s] = Shift(s, base, live)
                dtwin[s] = shift_state(s, t[0], base, ring=t[1]) if s == "runflex" else shift_state(s, t, base)
                check_state(pkg, s, dtwin[s])
                if dev:
                    _store(s, dec[s], dtwin[s])
        if dev and i == move_at:
            other = _rs_object(pkg, sc, dc_pole)
            other.store_state(*rr.fetch_state())
            assert other.dc_block() == rr.dc_block() and other.capacity() == rr.capacity()
            rr.close()
            rr = other
    out = rr.fetch_state() if dev else None
    for o in (list(dec.values()) + [rr] if dev else ()):
        o.close()
    return out, (state, pending, dc), (sh.on if sh else None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
@pytest.mark.parametrize("place", RS_CASES)
def test_gpu_resampler_behind_a_stored_shifted_state(pkg, ora, place, ratio, kind):
    """the gate's calls into a RunResampler whose state was fetched, shifted in `outs` and stored behind call 0: 2^32 inside a
    run, at a run's first output and at its last; the DC blocker on at the "inside" place"""
    import torch
    sc = scene(pkg, ora, ratio)
    rs = rs_scene(pkg, ora, sc, kind)
    base = rs_base(rs, place)
    got, (state, pending, dc), on = gpu_rs_run(pkg, torch, sc, rs, base, dc_pole=0.999 if place == "inside" else None)
    _same_rs_state(got, state, pending, dc, "after the last call")
    assert on[:3].all() and not on[3] and (state["outs"][:3] > np.uint64(base)).all() and state["outs"][3] < T32


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=RID)
def test_gpu_chain_behind_a_stored_shifted_resampler(pkg, ora, ratio):
    """the whole device chain at B = 2^32 - d, 2^32 inside a run: the resampler's own stored `outs` produces the shifted
    first_out, and the three decoders (their states shifted by the same B) consume its device view"""
    import torch
    sc = scene(pkg, ora, ratio)
    rs = rs_scene(pkg, ora, sc, "ragged")
    base = rs_base(rs, "inside")
    I, D, _ = ratio
    decoders = {s: MOD[s].Checker(pkg, ora, sc["taps"], I, D, W) for s in STAGES}
    got, (state, pending, dc), on = gpu_rs_run(pkg, torch, sc, rs, base, decoders=decoders)
    _same_rs_state(got, state, pending, dc, "after the last call")


@pytest.mark.gpu
def test_gpu_moving_a_resamplers_stream_with_the_dc_blocker_on(pkg, ora):
    """object A runs calls 0 .. 2 with the DC blocker on, its state (pending samples and blocker included) goes into a fresh
    object that runs the rest: the results are one object's; store(fetch()) changes nothing"""
    import torch
    sc = scene(pkg, ora, RATIOS[1])
    rs = rs_scene(pkg, ora, sc, "ragged")
    got, (state, pending, dc), _ = gpu_rs_run(pkg, torch, sc, rs, None, dc_pole=0.999, move_at=2)
    _same_rs_state(got, state, pending, dc, "after the last call")
    s0, p0, dc0, _, _ = cached(("rs0", RATIOS[1], "ragged"), lambda: rs_twin_run(pkg, sc, rs, None, dc_pole=0.999))
    _same_rs_state(got, s0, p0, dc0, "one object's")


@pytest.mark.gpu
def test_gpu_resampler_store_refusals_leave_the_state(pkg, ora):
    import torch
    b = pkg.binding
    sc = scene(pkg, ora, RATIOS[1])
    rs = rs_scene(pkg, ora, sc, "ragged")
    rr = _rs_object(pkg, sc)
    tr.same(tr._fed(pkg, torch, rr, *rs["calls"][0]), rs["want"][0], "call 0")
    state, pending = rr.fetch_state()
    _refused_store(pkg, lambda: rr.store_state(state[:3], pending[:3], nr_channels=3), None)
    _refused_store(pkg, lambda: rr.store_state(None, pending), None)
    _refused_store(pkg, lambda: rr.store_state(state, None), None)
    _refused_store(pkg, lambda: rr.store_state(state, pending, np.zeros(NCH, b.RUNRS_DC_STATE_DTYPE)), "DC blocker is off")
    bad = state.copy()
    bad["phase"][1] = sc["ratio"][0]
    _refused_store(pkg, lambda: rr.store_state(bad, pending), "channel 1: phase")
    bad = state.copy()
    bad["pending"][3] = pending.shape[1] + 1
    _refused_store(pkg, lambda: rr.store_state(bad, pending), "channel 3: pending")
    got = rr.fetch_state()
    assert got[0].tobytes() == state.tobytes() and np.array_equal(got[1], pending)
    rr.store_state(state, pending)
    tr.same(rr.fetch(), rs["want"][0], "call 0, fetched again behind the store")
    tr.same(tr._fed(pkg, torch, rr, *rs["calls"][1]), rs["want"][1], "call 1 after the refused stores")
    rr.close()
    rr = _rs_object(pkg, sc, 0.999)
    state, pending, dc = rr.fetch_state()
    _refused_store(pkg, lambda: rr.store_state(state, pending), "DC blocker is on")
    bad = dc.copy()
    bad["reserved"][0] = 7
    _refused_store(pkg, lambda: rr.store_state(state, pending, bad), "reserved")
    rr.store_state(state, pending, dc)
    rr.close()
