"""The burst FLEX stage (mfm_runflex_*, csrc/mfm_runflex.hip): the runs the burst resampler left go through the FLEX front half,
one fresh decoder per stretch.

The expected result is the oracle's, never the code under test: the restated gate (tests/test_gate.py, test_gate_preroll.py),
the oracle resampler per stretch (test_runrs.Checker) and a fresh oracle_lib.Flex() per stretch, fed run by run; every event is
asserted to lie in its run's [first_out, first_out + nr_out).  Every comparison is an equality of every field of every event
and of all 4 x 88 words of every frame."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_flex as tf
import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_runais as tra
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runflex_create", "mfm_runflex_destroy", "mfm_runflex_process_device", "mfm_runflex_fetch",
             "mfm_runflex_device_view", "mfm_runflex_fetch_state", "mfm_hosttwin_runflex_call", "mfm_runflex_store_state",
             "mfm_hosttwin_runflex_state_check"]
RATIOS = [(16, 25, 101), (1, 1, 4)]   # interpolate, decimate, taps
WINDOWS = [7, 64, 500]
NCH = 4
N_OUT = {7: 36000, 64: 100000, 500: 100000}   # samples per channel at 16 000 Hz; W = 7 has a shorter scene, one frame a channel
ORACLE_FIELDS = ("type", "coding", "sample", "sync_sample", "eye", "a", "b", "inv_a", "fiw_raw", "fiw", "fiw_rc", "sample_range",
                 "sample_delta", "cycle", "frame")
FRAME, BAD_BAUD, BAD_FIW = 1, 2, 3
DEAD = 311


def rs_taps(pkg, ora, ratio):
    if ratio[2] == 101:
        return ora.quantize_taps(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16)   # decoder_amd's 16/25 low-pass, shorter
    return ora.quantize_taps([0.1, 0.4, 0.4, 0.1])


def bounds_from_codings(ora):
    """(event spacing, frame spacing), re-derived.  Every event is followed by a reset; behind a reset at x the search looks at
    x + 311 first (310 samples in which a zero-filled register cannot read BS1), a run needs 3 matches, the sample that ends it
    is j >= x + 314, the first sync bit s0 = j + t with t >= 1, the earliest event s0 + 790.  A FRAME lies at its last block
    symbol e = f + step + fudge + sync2 * step + (symbols - 1) * step with f = s0 + 1110."""
    event = DEAD + 3 + 1 + 790
    spans = []
    for i in range(4):
        o = ora.flex_coding(i)
        step = o.sample_skip + 1
        sync2 = 2 * (o.sync_2_samples + 16 // o.sym_bits)
        spans.append(step + o.sample_fudge + sync2 * step + (o.symbols_per_block - 1) * step)
    return event, DEAD + 3 + 1 + 1110 + min(spans)


# ---- the checker --------------------------------------------------------------------------------------------

def to_events(pkg, ora, e, channel, run, window, frame0):
    """RUNFLEX_EVENT_DTYPE records and the words of the frames from the oracle's events of one run"""
    ev = np.zeros(len(e), pkg.binding.RUNFLEX_EVENT_DTYPE)
    for f in ORACLE_FIELDS:
        ev[f] = e[f]
    known = [ora.flex_coding(int(c)) if int(c) < 4 else None for c in e["coding"]]
    ev["baud"] = [o.baud if o else 0 for o in known]
    ev["nr_phases"] = [o.nr_phases if o else 0 for o in known]
    ev["channel"], ev["run"], ev["stretch_window"] = channel, run, window
    is_frame = e["type"] == FRAME
    ev["frame_index"] = np.where(is_frame, frame0 + np.cumsum(is_frame) - 1, 0)
    fw = np.zeros(int(is_frame.sum()), pkg.binding.FLEX_FRAME_DTYPE)
    fw["words"] = e["words"][is_frame]
    return ev, fw


class Checker:
    """what the stage must return for the gate calls of one stream, from the oracle; and what the guards read"""

    def __init__(self, pkg, ora, taps, I, D, W):
        self.pkg, self.ora = pkg, ora
        self.rs = tr.Checker(pkg, ora, taps, I, D, False, W)
        self.chan = {}      # channel -> [decoder, key of the stretch]
        self.by = {}        # (channel, first window) -> [(events, frames)] per run
        self.msgs = {}      # (channel, first window) -> the embedded message layer's messages
        self.pcm = {}       # (channel, first window) -> resampled pieces
        self.bounds = {}    # (channel, first window) -> first_out of every run but the first: the handovers
        self.multi = 0      # calls in which a channel has two runs or more

    def call(self, gate_runs, gate_payload):
        b = self.pkg.binding
        runs, payload = self.rs.call(gate_runs, gate_payload)
        evs, fws, nf = [], [], 0
        ch = [int(c) for c in runs["channel"]]
        self.multi += len(set(ch)) < len(ch)
        for i, r in enumerate(runs):
            c, fo, n = int(r["channel"]), int(r["first_out"]), int(r["nr_out"])
            if int(r["flags"]) & 1:
                key = (c, int(r["first_window"]))
                self.chan[c] = [self.ora.Flex(), key]
                self.by[key], self.pcm[key], self.bounds[key], self.msgs[key] = [], [], [], []
            else:
                self.bounds[self.chan[c][1]].append(fo)
            st = self.chan[c]
            y = payload[int(r["out_offset"]):int(r["out_offset"]) + n]
            e, m = st[0].feed(y)
            assert ((e["sample"] >= fo) & (e["sample"] < fo + n)).all()   # no lag: the oracle reports where the sample is
            ev, fw = to_events(self.pkg, self.ora, e, c, i, st[1][1], nf)
            nf += len(fw)
            self.by[st[1]].append((ev, fw))
            self.msgs[st[1]] += m
            self.pcm[st[1]].append(y)
            evs.append(ev)
            fws.append(fw)
        ev = np.concatenate(evs) if evs else np.zeros(0, b.RUNFLEX_EVENT_DTYPE)
        fw = np.concatenate(fws) if fws else np.zeros(0, b.FLEX_FRAME_DTYPE)
        return (runs, payload), (ev, fw)

    def stretches(self):
        """{(channel, first window): (events without `run` and `frame_index`, frames)}; each stretch once more through a fresh
        decoder in one piece"""
        out = {}
        for key, parts in self.by.items():
            whole, msgs = self.ora.Flex().feed(np.concatenate(self.pcm[key]))
            want, wfw = to_events(self.pkg, self.ora, whole, key[0], 0, key[1], 0)
            ev = np.concatenate([p[0] for p in parts]) if parts else want[:0]
            fw = np.concatenate([p[1] for p in parts]) if parts else wfw[:0]
            ev = ev.copy()
            ev["run"] = 0
            ev["frame_index"] = np.where(ev["type"] == FRAME, np.cumsum(ev["type"] == FRAME) - 1, 0)
            assert ev.tobytes() == want.tobytes() and fw.tobytes() == wfw.tobytes(), key
            assert msgs == self.msgs[key], key
            out[key] = (ev, fw)
        return out


def same(got, want, what):
    (ge, gf), (we, wf) = got, want
    assert ge.dtype == we.dtype and ge.shape == we.shape, (what, ge.shape, we.shape, [(int(e["type"]), int(e["sample"])) for e in ge][:8],
                                                           [(int(e["type"]), int(e["sample"])) for e in we][:8])
    for f in we.dtype.names if len(we) else ():
        bad = np.flatnonzero(ge[f] != we[f])
        assert bad.size == 0, f"{what}: event field {f} differs at {bad[:5].tolist()}: {ge[f][bad[0]]} != {we[f][bad[0]]}"
    assert gf.dtype == wf.dtype and gf.shape == wf.shape, (what, gf.shape, wf.shape)
    assert np.array_equal(gf["words"], wf["words"]), f"{what}: frame words differ in frames {np.flatnonzero((gf['words'] != wf['words']).any(axis=(1, 2)))[:5].tolist()}"


def per_stretch(ev, fw, into):
    """the events of one call with their words, by stretch, without what depends on the cut (run, frame_index)"""
    for e in ev:
        e2 = e.copy()
        words = fw[int(e["frame_index"])]["words"].tobytes() if int(e["type"]) == FRAME else b""
        e2["run"] = e2["frame_index"] = 0
        into.setdefault((int(e["channel"]), int(e["stretch_window"])), []).append((e2.tobytes(), words))


# ---- scenes ---------------------------------------------------------------------------------------------------

_SCENE = {}


def _frames(sy, coding, k, first=0, **kw):
    out = []
    for i in range(first, first + k):
        ph = {p: sy.flex_phase_words([dict(r) for r in tf.RECORDS[: 3 + (i + p) % 5]]) for p in sy.FLEX_CODINGS[coding]["phases"]}
        out.append(sy.flex_frame_levels(coding, (3 + i) % 16, (7 * coding + i) % 128, ph, **kw))
    return out


def scene(pkg, ora, ratio, W):
    """four channels of PCM at the gate's input rate (16 000 * D / I Hz), so that the resampled stretch decodes, and where each
    transmission lies at 16 000 Hz:
    0: the codings 0, 1 and 3 back to back; 1: a damaged A (BAD_BAUD), a damaged FIW (BAD_FIW) and coding 2; 2: the 7000-sample
    1010 tone of test_flex._flex_channels in front of a coding 0 frame, exact silence, a coding 1 frame; 3: codings 2 and 3 at
    low amplitude with a DC offset.  W = 7: shorter, one transmission a channel.  Made once per (ratio, W) and left unchanged"""
    short = W == 7
    key = (ratio, short)
    if key in _SCENE:
        return _SCENE[key]
    sy = pkg.synth
    I, D, _ = ratio
    rate = 16000 * D // I
    n = N_OUT[W]
    tone = [(3 if (k & 1) == 0 else -3, 10) for k in range(700)]
    bad_a = sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)
    bad_fiw = sy.flex_frame_levels(2, 1, 4, {}, fiw_flip=0x00700000)
    ln = lambda fr: sum(r[1] for r in fr)   # samples of a frame at 16 000 Hz
    if short:
        plan = {0: [([_frames(sy, 0, 1)[0]], 400, {})], 1: [([_frames(sy, 1, 1)[0]], 2000, {})],
                2: [([bad_fiw[:400]], 300, {}), ([bad_a[:400]], 9000, {})], 3: [([_frames(sy, 3, 1)[0]], 77, dict(offset=-400, amplitude=5000))]}
    else:
        plan = {0: [([_frames(sy, 0, 1)[0], _frames(sy, 1, 1)[0], _frames(sy, 3, 1)[0]], 400, {})],
                1: [([bad_a, bad_fiw, _frames(sy, 2, 1)[0]], 1200, {})],
                2: [([tone + _frames(sy, 0, 1, first=1)[0]], 50, {}), ([_frames(sy, 1, 1, first=2)[0]], 64000, {})],
                3: [([_frames(sy, 2, 1, first=1)[0], _frames(sy, 3, 1, first=3)[0]], 4099, dict(offset=700, amplitude=5000))]}
    rng = np.random.RandomState(11)
    n_in = n * D // I
    chans, tx = [], {}
    for c in range(NCH):
        x = rng.randint(-300, 300, n_in).astype(np.int16)
        if c == 2:
            x[:] = 0   # exact silence between the transmissions: every bit a one, no swing
        tx[c] = []
        for k, (frames, at, kw) in enumerate(plan[c]):
            p = sy.flex_pcm(frames, noise=300, seed=10 * c + k, rate=rate, **kw)
            a_in = at * D // I
            assert a_in + p.size <= n_in, (c, k, a_in, p.size, n_in)
            x[a_in:a_in + p.size] = p
            pos = at
            for fr in frames:   # one entry per frame: (start, end) at 16 000 Hz
                tx[c].append((pos, pos + ln(fr)))
                pos += ln(fr)
        chans.append(x)
    _SCENE[key] = dict(stream=np.ascontiguousarray(np.stack(chans)), tx=tx, n_in=n_in, D=D, I=I)
    return _SCENE[key]


def make_mask(kind, sc, W, rng):
    """raw squelch verdicts [C][nw] and the (channel, first window) of the stretches a closing window cuts inside a block"""
    nw = sc["n_in"] // W
    m = np.zeros((NCH, nw), bool)
    cut_keys = []
    if kind == "open":
        return ~m, cut_keys
    if kind == "short":   # W = 7: stretches of one or two windows, one channel open all the time
        for c in range(NCH - 1):
            k = int(rng.randint(0, 3))
            while k < nw:
                ln = int(rng.randint(1, 3))
                m[c, k:k + ln] = True
                k += ln + 2 + int(rng.randint(1, 3))
        m[NCH - 1] = True
        return m, cut_keys
    w_of = lambda s16: max(s16, 0) * sc["D"] // sc["I"] // W
    k = 0
    for c in range(NCH):
        for a, b in sc["tx"][c]:
            ka, kb = w_of(a - 250), w_of(b + 700) + 2
            if kind == "cut" and b - a > 20000:
                if k % 3 == 0:
                    kb = w_of(a + 16000)          # closes inside the block: the frame is lost
                    cut_keys.append((c, ka))
                elif k % 3 == 1:
                    ka = w_of(a + (3000 if b - a > 33000 else 120))   # opens inside the BS1 run (the long tone, or sync 1's)
                else:
                    ka = w_of(a + 12000)          # opens mid-block: nothing may be invented
                k += 1
            m[c, ka:min(kb, nw)] = True
    if kind == "cut":   # a run of matches open across closed windows on the tone, and two runs of a channel in one call
        a = sc["tx"][2][0][0]
        if sc["tx"][2][0][1] - a > 33000:
            m[2, w_of(a + 5200):w_of(a + 5600)] = False
            cut_keys = [k if k[0] != 2 else (2, w_of(a + 5600)) for k in cut_keys]

    def start(c, k):   # the first window of the stretch window k lies in
        while k > 0 and m[c, k - 1]:
            k -= 1
        return k

    return m, [(c, start(c, k)) for c, k in cut_keys]


def anchors_of(sc, ev):
    """input positions inside every phase of the first events of the all-open stream (stretch sample = output, the filter's
    delay aside): the open BS1 run, around s0, the sync words, the wait for the FIW, sync 2, the block, the event and the dead
    samples behind it"""
    out = []
    for c in range(NCH):
        for e in [e for e in ev if int(e["channel"]) == c][:3]:
            t, s = int(e["type"]), int(e["sample"])
            s0 = int(e["sync_sample"]) - 1110 if t == FRAME else (s - 1110 if t == BAD_FIW else s - 790)
            marks = [s0 - 150, s0 - 5, s0 + 400, s0 + 950, s, s + 1, s + 150]
            if t == FRAME:
                marks += [s0 + 1110 + 200, s0 + 1110 + 15000]
            out += [max(x, 0) * sc["D"] // sc["I"] for x in marks]
    return sorted(out)


def kinds_of(W):
    return ["open", "fitted", "cut"] + (["short"] if W == 7 else [])


def classify(by, bounds, tally):
    """where the handovers lie, from the oracle's events around each run boundary"""
    for key, (ev, _) in by.items():
        for e in ev:
            t, s = int(e["type"]), int(e["sample"])
            s0 = int(e["sync_sample"]) - 1110 if t == FRAME else (s - 1110 if t == BAD_FIW else s - 790)
            j = s0 - (10 - (int(e["eye"]) // 2) % 10)
            inside = 0
            for b in bounds[key]:   # b: the first sample of a later run
                tally["in_bs1"] += j - int(e["eye"]) < b <= j
                tally["in_sync1"] += s0 < b <= s0 + 790
                tally["in_fiw_wait"] += t != BAD_BAUD and s0 + 790 < b <= s0 + 1110
                tally["dead"] += s < b <= s + DEAD
                if t == FRAME:
                    first = s - 28150 - (5 if int(e["coding"]) & 1 else 0)
                    tally["in_sync2"] += s0 + 1110 < b <= first
                    tally["in_block"] += first < b <= s
                    inside += s0 < b <= s
            tally["three_calls"] += inside >= 2
    return tally


def run_scenes(pkg, ora, W, ratio, make_call, seed, pages=None, guards_only=False):
    """every mask, P = 0 and 2 with the flush, each stream in the seeded cut (a boundary in every phase of a frame, one-window
    calls, nr_in = 0 calls) and as one call; asserts the guards on the oracle's figures before any comparison"""
    I, D, _ = ratio
    sc = scene(pkg, ora, ratio, W)
    taps = rs_taps(pkg, ora, ratio)
    stream, n = sc["stream"], sc["n_in"]
    jobs = []
    tally = dict(in_bs1=0, in_sync1=0, in_fiw_wait=0, in_sync2=0, in_block=0, dead=0, three_calls=0, cut_inside=0, multi=0)
    open_ev, anchors = None, []
    for kind in kinds_of(W):
        for P in (0, 2):
            rng = np.random.RandomState(seed + 10 * kinds_of(W).index(kind) + P)
            mask, cut_keys = make_mask(kind, sc, W, rng)
            for single in (True, False):
                cuts = [n] if single else tra.make_cuts(rng, n, W, anchors)
                calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
                chk = Checker(pkg, ora, taps, I, D, W)
                want = [chk.call(gr, gp) for gr, gp in calls]
                by = chk.stretches()
                emitted = tr.emitted_of(mask, P)[:, :n // W]
                assert sorted(by) == tr.stretches_of_mask(emitted)
                if kind == "open" and single and P == 0:
                    open_ev = np.concatenate([v[0] for v in by.values()])
                    anchors = anchors_of(sc, open_ev)
                if not single:
                    classify(by, chk.bounds, tally)
                tally["multi"] += chk.multi
                if kind == "cut" and P == 0 and single:
                    for k in cut_keys:   # the frame a closing window cut is lost without an event
                        assert k in by and not (by[k][0]["type"] == FRAME).any() and sum(p.size for p in chk.pcm[k]) > 8000, k
                        tally["cut_inside"] += 1
                if kind == "fitted" and pages is not None:
                    pages(chk, by)
                jobs.append((kind, P, single, cuts, mask, calls, want, by))
    # the guards, on the oracle's result alone
    ev = open_ev
    frames = ev[ev["type"] == FRAME]
    if W != 7:
        assert set(frames["coding"].tolist()) == {0, 1, 2, 3} and len(frames) >= 7, frames["coding"].tolist()
        assert (ev["type"] == BAD_BAUD).any() and (ev["type"] == BAD_FIW).any()
        assert tally["cut_inside"] >= 1 and tally["multi"] >= 1, tally
    else:
        assert len(frames) >= 3 and (ev["type"] == BAD_FIW).any() and (ev["type"] == BAD_BAUD).any()
    # the window sets how finely a handover can be placed: 4.5, 41 and 320 outputs at 16/25
    wide = ["in_sync1", "in_block", "three_calls"] + (["in_bs1", "in_fiw_wait", "in_sync2", "dead"] if W <= 64 else [])
    assert all(tally[k] >= 1 for k in wide), tally
    if guards_only:
        return tally
    # the code under test
    for kind, P, single, cuts, mask, calls, want, by in jobs:
        what = f"W {W} {I}/{D} mask {kind} P {P} single {single}"
        call, done = make_call(NCH, W, P, cuts, stream, mask, taps, I, D)
        got_by, want_by = {}, {}
        for i, ((gr, gp), (rs_want, ev_want)) in enumerate(zip(calls, want)):
            got = call(i, gr, gp, rs_want)
            same(got, ev_want, f"{what}, call {i}")
            per_stretch(*got, got_by)
        done()
        for k, (e, fw) in by.items():   # cut independence: per stretch the same events and words however the stream was cut
            per_stretch(e, fw, want_by)
        assert got_by == want_by, what
    return tally


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runflex_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src) and b.MFM_ABI_VERSION == 4
    assert b.RUNFLEX_EVENT_DTYPE.itemsize == 104 and b.RUNFLEX_STATE_DTYPE.itemsize == 88 and C.sizeof(b.RunFlexConfig) == 32
    assert b.RUNFLEX_EVENT_DTYPE.names[:len(b.FLEX_EVENT_DTYPE.names)] == b.FLEX_EVENT_DTYPE.names
    for n in b.FLEX_EVENT_DTYPE.names:   # struct mfm_flex_event in front, field for field
        assert b.RUNFLEX_EVENT_DTYPE.fields[n] == b.FLEX_EVENT_DTYPE.fields[n], n
    assert pkg.RUNFLEX_EVENT_DTYPE is b.RUNFLEX_EVENT_DTYPE and pkg.RunFlex is b.RunFlex and pkg.RunFlexConfig is b.RunFlexConfig
    assert pkg.hosttwin_runflex_call is b.hosttwin_runflex_call and pkg.runflex_to_flex_events is b.runflex_to_flex_events
    assert pkg.RUNFLEX_STATE_DTYPE is b.RUNFLEX_STATE_DTYPE and pkg.hosttwin_runflex_state is b.hosttwin_runflex_state
    assert pkg.runflex_event_bound is b.runflex_event_bound and pkg.runflex_frame_bound is b.runflex_frame_bound
    for struct, names in (("event", b.RUNFLEX_EVENT_DTYPE.names), ("state", b.RUNFLEX_STATE_DTYPE.names),
                          ("config", [n for n, _ in b.RunFlexConfig._fields_])):
        m = re.search(r"struct mfm_runflex_%s \{(.*?)\};" % struct, src, flags=re.S)
        assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == list(names), struct
    for name in ("OVER_RUNS", "OVER_EVENTS", "IN_RUNRS", "IN_OUT_OF_STEP", "IN_BAD_RUNS"):
        m = re.search(r"#define\s+MFM_RUNFLEX_%s\s+(\d+)u\b" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNFLEX_" + name)


def test_bounds_rederived_from_the_oracles_codings(pkg, ora):
    b = pkg.binding
    event, frame = bounds_from_codings(ora)
    assert (event, frame) == (1105, 29985) == (b.RUNFLEX_EVENT_SPACING, b.RUNFLEX_FRAME_SPACING)
    for n in (0, 1, event - 1, event, 3 * event + 7, frame - 1, frame, 10 * frame):
        assert b.runflex_event_bound(n) == n // event + 1 and b.runflex_frame_bound(n) == n // frame + 1
    # what the stage reads back fits its ring: a block's symbols and the sync words
    for i in range(4):
        o = ora.flex_coding(i)
        assert (o.symbols_per_block - 1) * (o.sample_skip + 1) < b.RUNFLEX_RING and 1110 < b.RUNFLEX_RING


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_scene_is_what_it_is_meant_to_be(pkg, ora, W, ratio):
    """from the oracle alone: a FRAME of each coding, both BAD_* types, a stretch a closing window cuts mid-frame, a frame that
    spans three calls or more, and a handover in every phase of a frame the window lets one be placed in"""
    run_scenes(pkg, ora, W, ratio, None, 7 * W + ratio[0], guards_only=True)


def _twin_call(pkg):
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        state = b.hosttwin_runflex_state(nch)

        def call(i, gr, gp, rs_want):
            return b.hosttwin_runflex_call(state, *rs_want)   # max_events, max_frames 0: the defaults never refuse

        return call, lambda: None

    return make_call


def host_pages(pkg, ev, fw):
    """the messages a fresh host FLEX pager assembles from one stretch's events and words, notes included"""
    hp = tf.HostFlex()
    conv = pkg.binding.runflex_to_flex_events(ev)
    half = len(conv) // 2
    hp.on_events(conv[:half], fw)
    hp.on_events(conv[half:], fw)
    hp.close()
    return hp.out


def _pages_check(pkg, found):
    def pages(chk, by):
        for key, (ev, fw) in by.items():
            got = host_pages(pkg, ev, fw)
            assert got == [m[:10] for m in chk.msgs[key]], key
            found[0] += len(tf._pages(got))
    return pages


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_hosttwin_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """csrc/mfm_runflex.h and the twin's decoder on the scenes of the GPU tests; the pages a fresh host pager per stretch
    assembles from the fitted mask's events and words are the oracle's"""
    found = [0]
    run_scenes(pkg, ora, W, ratio, _twin_call(pkg), 7 * W + ratio[0], pages=_pages_check(pkg, found))
    assert found[0] >= 3


_PIECES = {}


def _pieces(pkg, ora):
    """one stretch per channel cut into runs by hand, at any sample: channel 0 carries two frames of the 2-level coding 0,
    channel 1 one of the 4-level coding 3 at 16 000 Hz.  Returns the calls [(runs, payload)] and the oracle's (events, frames)
    per call.  About 60 cuts: inside the open BS1 run, at j and s0 and one sample behind, inside the sync words, between s0 + 790
    and f, at f, inside sync 2, through the block (also more than 28 000 samples behind the sync, so that the frame is built
    from the ring), at e - 1, e, e + 1, inside the dead samples and at their end, as runs of one sample and runs without
    output; channel 1 sits out every third call"""
    if _PIECES:
        return _PIECES["it"]
    b, sy = pkg.binding, pkg.synth
    pcm = [sy.flex_pcm(_frames(sy, 0, 2), lead=500, trail=900, noise=300, seed=1),
           sy.flex_pcm(_frames(sy, 3, 1), lead=901, trail=900, noise=500, seed=2, offset=300)]
    whole = [ora.Flex().feed(x)[0] for x in pcm]
    assert [int(t) for t in whole[0]["type"]] == [FRAME, FRAME] and [int(t) for t in whole[1]["type"]] == [FRAME]
    assert [int(c) for c in whole[0]["coding"]] == [0, 0] and int(whole[1]["coding"][0]) == 3
    marks = []
    for w in whole:
        m = []
        for k, e in enumerate(w):
            f, s = int(e["sync_sample"]), int(e["sample"])
            s0 = f - 1110
            j = s0 - (10 - (int(e["eye"]) // 2) % 10)
            m += [j - 40, j - 1, j, j + 1, s0, s0 + 1, s0 + 333, s0 + 790, s0 + 791, s0 + 1000, f, f + 1, f + 200, f + 410, f + 411,
                  f + 5000, f + 5001, f + 5001, f + 20000, f + 28100, s - 5, s - 1, s, s + 1, s + 2, s + 150, s + DEAD - 1, s + DEAD,
                  s + DEAD + 1]
            if k == 0:
                m += [5, 5, 100, 309, 310, 311]
        marks.append(m)
    assert len(marks[0]) + len(marks[1]) >= 60
    cuts = [sorted(m) + [x.size] for m, x in zip(marks, pcm)]
    calls, want = [], []
    dem = [ora.Flex(), ora.Flex()]
    at, nxt, i = [0, 0], [0, 0], 0
    while nxt[0] < len(cuts[0]) or nxt[1] < len(cuts[1]):
        runs, parts, evs, fws, nf = [], [], [], [], 0
        for c in (0, 1):
            if nxt[c] >= len(cuts[c]) or (c == 1 and i % 3 == 2):   # channel 1 sits out every third call and keeps its state
                continue
            end = cuts[c][nxt[c]]
            nxt[c] += 1
            y = pcm[c][at[c]:end]
            runs.append((7 + c, sum(p.size for p in parts), at[c], c, y.size, int(at[c] == 0 and nxt[c] == 1), 0))
            parts.append(y)
            e = dem[c].feed(y)[0]
            assert ((e["sample"] >= at[c]) & (e["sample"] < end)).all()
            ev, fw = to_events(pkg, ora, e, c, len(runs) - 1, 7 + c, nf)
            nf += len(fw)
            evs.append(ev)
            fws.append(fw)
            at[c] = end
        calls.append((np.array(runs, b.RUNRS_RUN_DTYPE), np.concatenate(parts) if parts else np.zeros(0, np.int16)))
        want.append((np.concatenate(evs) if evs else np.zeros(0, b.RUNFLEX_EVENT_DTYPE),
                     np.concatenate(fws) if fws else np.zeros(0, b.FLEX_FRAME_DTYPE)))
        i += 1
    assert at[0] == pcm[0].size and at[1] == pcm[1].size and sum(len(w[0]) for w in want) == 3 == sum(len(w[1]) for w in want)
    assert any(len(r) and (r["nr_out"] == 0).any() for r, _ in calls) and any(len(r) and (r["nr_out"] == 1).any() for r, _ in calls)
    _PIECES["it"] = (calls, want)
    return _PIECES["it"]


def test_hosttwin_handovers_at_any_sample(pkg, ora):
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    state = b.hosttwin_runflex_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(b.hosttwin_runflex_call(state, runs, payload), w, f"call {i}")


def _refusal_case(pkg, ora):
    """two calls of the hand-cut stretches that both carry runs of both channels, and what is wrong with the second"""
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    ok = [i for i in range(3, len(calls)) if len(calls[i][0]) == 2 and calls[i][0]["nr_out"].min() > 0]
    i = next(i for i in ok if len(want[i][0]))   # a call that ends a frame
    runs, payload = calls[i]
    bound = sum(b.runflex_event_bound(n) for n in runs["nr_out"])
    fbound = sum(b.runflex_frame_bound(n) for n in runs["nr_out"])

    def changed(field, k, value):
        r = runs.copy()
        r[field][k] = value
        return r

    cases = [
        (dict(totals=[2, payload.size, 1, 0]), "overflow or gate error", b.MFM_RUNFLEX_IN_RUNRS << 8),
        (dict(totals=[2, payload.size, 0, 2]), "overflow or gate error", b.MFM_RUNFLEX_IN_RUNRS << 8),
        (dict(runs=changed("first_out", 0, int(runs["first_out"][0]) + 1)), "out of step", b.MFM_RUNFLEX_IN_OUT_OF_STEP << 8),
        (dict(runs=changed("channel", 0, 1)), "out of step", b.MFM_RUNFLEX_IN_OUT_OF_STEP << 8),   # channel 1's second run continues
        (dict(runs=changed("channel", 1, 2)), "does not exist", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),
        (dict(runs=changed("flags", 0, 1)), "does not exist", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),     # begins with first_out != 0
        (dict(runs=runs[::-1].copy()), "does not exist", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),          # channels descend
        (dict(runs=changed("out_offset", 1, payload.size + 1)), "does not exist", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),
        (dict(runs=changed("nr_out", 1, payload.size)), "does not exist", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),
    ]
    capacity = [
        (dict(max_out_samples=payload.size - 1), "max_out_samples", b.MFM_RUNFLEX_IN_BAD_RUNS << 8),
        (dict(max_runs=1), "max_runs", b.MFM_RUNFLEX_OVER_RUNS),
        (dict(max_events=bound - 1), "event bound", b.MFM_RUNFLEX_OVER_EVENTS),
        (dict(max_frames=fbound - 1), "frame bound", b.MFM_RUNFLEX_OVER_EVENTS),
    ]
    return calls, want, i, cases, capacity, (bound, fbound)


def test_hosttwin_refuses_and_leaves_its_state(pkg, ora):
    """once per flag (and per way to raise it): nothing comes out, state and ring stay byte-identical"""
    b = pkg.binding
    calls, want, at, cases, capacity, (bound, fbound) = _refusal_case(pkg, ora)
    state = b.hosttwin_runflex_state(2)
    for i in range(at):
        same(b.hosttwin_runflex_call(state, *calls[i]), want[i], f"call {i}")
    s0, r0 = state[0].copy(), state[1].copy()
    assert s0["has_stretch"].all() and (s0["outs"] > 0).all() and r0.any(axis=1).all()
    runs, payload = calls[at]
    for change, message, flags in cases + capacity:
        kw = dict(runs=runs, payload=payload)
        kw.update(change)
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runflex_call(state, kw.pop("runs"), kw.pop("payload"), **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value))
        assert ei.value.needed == 0 and state[0].tobytes() == s0.tobytes() and state[1].tobytes() == r0.tobytes()
    for kw in (dict(max_out=len(want[at][0]) - 1), dict(max_out_frames=len(want[at][1]) - 1)):   # the caller's arrays are too small
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runflex_call(state, runs, payload, **kw)
        assert ei.value.code == b.MFM_E_NOMEM and (ei.value.needed, ei.value.needed_frames) == (len(want[at][0]), len(want[at][1]))
        assert state[0].tobytes() == s0.tobytes() and state[1].tobytes() == r0.tobytes()
    same(b.hosttwin_runflex_call(state, runs, payload, max_events=bound, max_frames=fbound), want[at], "the same call, right")
    for i in range(at + 1, len(calls)):
        same(b.hosttwin_runflex_call(state, *calls[i]), want[i], f"call {i}")


def test_hosttwin_refuses_by_the_bound_even_without_an_event(pkg):
    """a noise scene with no event at all: max_events or max_frames one below the bound is refused, the bounds and the defaults
    are not"""
    b = pkg.binding
    rng = np.random.RandomState(3)
    ES, FS = b.RUNFLEX_EVENT_SPACING, b.RUNFLEX_FRAME_SPACING
    payload = rng.normal(0, 2000, FS + 2 * ES + 10).round().astype(np.int16)
    sizes = [ES - 1, ES, payload.size - 2 * ES + 1]
    runs = np.array([(c, sum(sizes[:c]), 0, c, n, 1, 0) for c, n in enumerate(sizes)], b.RUNRS_RUN_DTYPE)
    bound = sum(b.runflex_event_bound(n) for n in sizes)
    fbound = sum(b.runflex_frame_bound(n) for n in sizes)
    assert bound == 1 + 2 + (FS + 11) // ES + 1 and fbound == 1 + 1 + 2
    for kw, word in ((dict(max_events=bound - 1), "event bound"), (dict(max_frames=fbound - 1), "frame bound")):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runflex_call(b.hosttwin_runflex_state(3), runs, payload, **kw)
        assert ei.value.code == b.MFM_E_STATE and word in str(ei.value) and ei.value.flags == b.MFM_RUNFLEX_OVER_EVENTS
    for kw in (dict(max_events=bound, max_frames=fbound), dict()):
        ev, fw = b.hosttwin_runflex_call(b.hosttwin_runflex_state(3), runs, payload, **kw)
        assert len(ev) == 0 and len(fw) == 0


REFUSALS = [
    (dict(abi_version=3), "abi_version"),
    (dict(nr_channels=0), "nr_channels"),
    (dict(max_runs=0), "max_runs"),
    (dict(max_out_samples=0), "max_out_samples"),
    (dict(max_runs=1 << 28), "max_runs"),
    (dict(flags=1), "flags must be 0"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_with_a_message(pkg, change, message):
    """every refusal of mfm_runflex_create is decided before a device is looked for"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_out_samples=10000)
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunFlex(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_runflex_to_flex_events_arithmetic(pkg):
    b = pkg.binding
    ev = np.zeros(3, b.RUNFLEX_EVENT_DTYPE)
    rng = np.random.RandomState(1)
    for f in b.RUNFLEX_EVENT_DTYPE.names:
        ev[f] = rng.randint(0, 1 << 31, 3)
    ev["sample"], ev["sync_sample"], ev["stretch_window"] = [1500, 99, (1 << 33) + 7], [390, 0, (1 << 33) - 29000], [0, 3, (1 << 40) + 1]
    ev["sample_delta"] = [-5, 0, 7]
    out = b.runflex_to_flex_events(ev)
    assert out.dtype == b.FLEX_EVENT_DTYPE and out.shape == (3,)
    for f in b.FLEX_EVENT_DTYPE.names:
        assert np.array_equal(out[f], ev[f]), f   # the stretch-relative samples are kept
    assert out.tobytes() == b"".join(e.tobytes()[:88] for e in ev)
    assert b.runflex_to_flex_events(ev[:0]).shape == (0,)


def test_runflex_kernels_use_no_scratch(pkg):
    """the code object's notes of build/mfm_runflex.o (tools/kernel_regs.py): the nine kernels, no private segment, no spilled
    vector register, at most 128 VGPRs, LDS well within 64 KB"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runflex.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    names = ("plan", "slice", "match", "walk", "evscan", "compact", "gather", "ring", "state")
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"rf_{k}_kernel" for k in names), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(5))) == (0, 0) and int(m.group(4)) <= 16384, ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gpu_call(pkg):
    """a real Gate (process_host, flush_device) -> RunResampler -> RunFlex on the device views, no fetch in between; the twin
    runs beside it on the oracle's run lists: same events and words, and the same state and ring after the last call"""
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        cap = max(max(cuts), 1)
        gate = pkg.Gate(nch, cap, W, preroll_windows=P)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P)
        rf = pkg.RunFlex.behind(rr)
        twin = b.hosttwin_runflex_state(nch)
        pos = [0]

        def call(i, gr, gp, rs_want):
            if i < len(cuts):
                m = cuts[i]
                gate.process_host(stream[:, pos[0]:pos[0] + m], tg.records_of(pkg, mask, pos[0] // W, (pos[0] + m) // W))
                pos[0] += m
            else:
                gate.flush_device()
            rr.process_device(*gate.device_view())
            rf.process_device(*rr.device_view())
            ev, fw = rf.fetch()
            d_ev, d_fw, d_tot = rf.device_view()
            tot = tl._d2h(d_tot, 32).view(np.uint64)
            assert tot.tolist() == [len(ev), len(fw), 0, 0], (i, tot.tolist())
            if len(ev):
                assert tl._d2h(d_ev, ev.nbytes).tobytes() == ev.tobytes()
            if len(fw):
                assert tl._d2h(d_fw, fw.nbytes).tobytes() == fw.tobytes()
            tr.same(rr.fetch(), rs_want, f"the resampler's call {i}")
            same(b.hosttwin_runflex_call(twin, *rs_want), (ev, fw), f"the twin's call {i}")
            return ev, fw

        def done():
            state, ring = rf.fetch_state()
            assert state.tobytes() == twin[0].tobytes(), [f for f in state.dtype.names if not np.array_equal(state[f], twin[0][f])]
            assert np.array_equal(ring, twin[1])
            rf.close()
            rr.close()
            gate.close()

        return call, done

    return make_call


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """four channels; all open, windows fitted to the frames, a mask that closes inside a block, opens inside a BS1 run and
    mid-block, at W = 7 stretches of one or two windows; P = 0 and 2 with the flush fed through; cut into calls inside every
    phase of a frame, as one-window and nr_in = 0 calls, and as one call, with identical events and words per stretch;
    device_view totals and bytes, the twin's events, and the twin's state and ring beside it"""
    run_scenes(pkg, ora, W, ratio, _gpu_call(pkg), 7 * W + ratio[0])


def _fed(pkg, torch, rf, runs, payload, totals=None, **kw):
    """one call from uploaded arrays: a burst resampler's result as it would stand in its device view"""
    t = np.array([len(runs), payload.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
    rf.process_device(*(k.data_ptr() for k in keep))
    try:
        return rf.fetch(**kw)
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_handovers_at_any_sample(pkg, ora):
    import torch
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    rf = pkg.RunFlex(2, 4, max(p.size for _, p in calls) + 1)
    twin = b.hosttwin_runflex_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(_fed(pkg, torch, rf, runs, payload), w, f"call {i}")
        b.hosttwin_runflex_call(twin, runs, payload)
        state, ring = rf.fetch_state()
        assert state.tobytes() == twin[0].tobytes() and np.array_equal(ring, twin[1]), i
    rf.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state(pkg, ora):
    """the resampler's flags handed through, out of step, run lists that are not a resampler's, max_runs, the bounds against
    max_events and max_frames: each time nothing comes out and state and ring stay, so the same call fed correctly is right"""
    import torch
    b = pkg.binding
    calls, want, at, cases, _, _ = _refusal_case(pkg, ora)
    runs, payload = calls[at]
    cap = max(p.size for _, p in calls) + 1
    rf = pkg.RunFlex(2, 4, cap)
    for i in range(at):
        same(_fed(pkg, torch, rf, *calls[i]), want[i], f"call {i}")
    s0, r0 = rf.fetch_state()
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rf, change.get("runs", runs), payload, totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == 0 and not ei.value.buffer.view(np.uint8).any() and not ei.value.frame_buffer.view(np.uint8).any()
        s1, r1 = rf.fetch_state()
        assert s1.tobytes() == s0.tobytes() and np.array_equal(r1, r0), change
    got = _fed(pkg, torch, rf, runs, payload)
    same(got, want[at], "the same call, right, after the refused ones")
    for kw in (dict(max_events=len(got[0]) - 1), dict(max_frames=len(got[1]) - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            rf.fetch(**kw)
        assert ei.value.code == b.MFM_E_NOMEM and (ei.value.needed, ei.value.needed_frames) == (len(got[0]), len(got[1]))
        assert not ei.value.buffer.view(np.uint8).any() and not ei.value.frame_buffer.view(np.uint8).any()
    same(rf.fetch(), want[at], "fetched again")
    for i in range(at + 1, len(calls)):
        same(_fed(pkg, torch, rf, *calls[i]), want[i], f"call {i}")
    rf.close()
    # what an object is too small for: the first call, whose runs begin their stretches, against max_runs, max_out_samples,
    # max_events and max_frames; the bounds themselves fit
    runs, payload = calls[0]
    bound = sum(b.runflex_event_bound(n) for n in runs["nr_out"])
    fbound = sum(b.runflex_frame_bound(n) for n in runs["nr_out"])
    assert len(runs) == 2 and (runs["flags"] == 1).all()
    for kw, message in ((dict(max_runs=1), "max_runs"), (dict(max_out_samples=payload.size - 1), "max_out_samples"),
                        (dict(max_events=bound - 1), "event bound"), (dict(max_frames=fbound - 1), "frame bound")):
        args = dict(max_runs=4, max_out_samples=cap, max_events=0, max_frames=0)
        args.update(kw)
        rf = pkg.RunFlex(2, **args)
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rf, runs, payload)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (kw, str(ei.value))
        rf.close()
    rf = pkg.RunFlex(2, 2, payload.size, max_events=bound, max_frames=fbound)
    same(_fed(pkg, torch, rf, runs, payload), want[0], "call 0 on an object made for it")
    rf.close()


CHAIN = dict(fs=1200000, decim=48, offsets=(-150000, 112500), W=100, P=1, blk=300007, hang=6, deviation=2400.0)
_CHAIN = {}


def _chain(pkg, ora):
    """two channels of FM FLEX at 1.2 MS/s (a 4-level 3200 frame on one, a 2-level 1600 frame on the other, noise around them),
    D = 48 -> 25 kHz; the oracle's PCM, the squelch on the PCM energy (a carrier lowers it) with a hang, and the 16/25 resampler
    taps as the scan tool quantises them"""
    if _CHAIN:
        return _CHAIN["it"]
    sy, s = pkg.synth, CHAIN
    fs, decim, W = s["fs"], s["decim"], s["W"]
    taps = sy.design_lpf(128, 12500.0, float(fs))
    parts = []
    for k, o in enumerate(s["offsets"]):
        coding = (2, 0)[k]
        ph = {p: sy.flex_phase_words(tf.RECORDS[k:k + 5]) for p in sy.FLEX_CODINGS[coding]["phases"]}
        gap = sy.synth_iq((3000 + 2500 * k) * fs // 16000, fs, [], seed=10 + k, noise=300).astype(np.float64)
        body = sy.flex_fm_iq([sy.flex_frame_levels(coding, 7, 30 + k, ph)], fs, float(o), deviation_hz=s["deviation"], amplitude=6000.0,
                             noise=300.0, seed=k)
        tail = sy.synth_iq((4500 - 2500 * k) * fs // 16000, fs, [], seed=20 + k, noise=300).astype(np.float64)
        parts.append(np.concatenate([gap, body, tail]))
    n = min(p.shape[0] for p in parts)
    iq = np.clip(np.round(sum(p[:n] for p in parts)), -32768, 32767).astype(np.int16)
    offs = np.array(s["offsets"], np.float64)
    cre = np.stack([ora.make_taps(taps, int(o), fs, 1.0)[0] for o in offs])
    cim = np.stack([ora.make_taps(taps, int(o), fs, 1.0)[1] for o in offs])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm = ora.run_channels(iq, cre, cim, incr, decim)[0]
    e = tl.restate(pkg, pcm, W, tl.PCM)["energy"].astype(np.float64)
    thr = int(np.sqrt(np.percentile(e, 5) * np.percentile(e, 95)))
    mask = tl.restate(pkg, pcm, W, tl.PCM, sense=tl.BELOW, open_thr=thr, close_thr=thr, hang=s["hang"])["open"].astype(bool)
    lpf = [float(x) for x in sy.design_lpf(101, 0.45 / 25, 1.0) * 16]
    rtaps = np.array([int(x * 16384.0) for x in lpf], np.int16)
    _CHAIN["it"] = dict(iq=iq, pcm=pcm, taps=taps, thr=thr, mask=mask, lpf=lpf, rtaps=rtaps, offs=offs)
    return _CHAIN["it"]


def _chain_want(pkg, ora):
    """the checker over the chain scene as the tool runs it: every block, then the flush"""
    sc, s = _chain(pkg, ora), CHAIN
    W, P = s["W"], s["P"]
    chk = Checker(pkg, ora, sc["rtaps"], 16, 25, W)
    n = sc["pcm"].shape[1]
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n))
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True))
    return chk, chk.stretches()


def test_chain_scene_is_what_it_is_meant_to_be(pkg, ora):
    """the recorded scene of the tool test, from the oracle alone: every channel opens and closes, the oracle collects both
    frames from the gated stretches and delivers pages"""
    sc, s = _chain(pkg, ora), CHAIN
    emitted = tgp.dilate(sc["mask"], s["P"])
    assert all(sum(1 for k in tr.stretches_of_mask(emitted) if k[0] == c) >= 1 for c in range(2)) and not emitted.all(axis=1).any()
    chk, by = _chain_want(pkg, ora)
    ev = np.concatenate([v[0] for v in by.values()])
    assert sorted(ev["coding"][ev["type"] == FRAME].tolist()) == [0, 2]
    assert sum(len(tf._pages(m)) for m in chk.msgs.values()) >= 6


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_flex_writes_the_events_and_pages_of_the_oracle(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-out DIR --gate-preroll 1 --gate-resample 16/25 --resample-taps FILE --gate-flex as a fresh child
    process on the chain scene: flex.jsonl holds the oracle's events and pages.jsonl its messages, stretch by stretch"""
    sc, s = _chain(pkg, ora), CHAIN
    fs, decim, W, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 929000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
           str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(sc["thr"]),
           "--hang", str(s["hang"]), "--block", str(s["blk"]), "--gate-out", str(tmp_path / "gated"), "--gate-preroll", str(P),
           "--gate-resample", "16/25", "--resample-taps", str(tmp_path / "filter.json"), "--gate-flex"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    chk, by = _chain_want(pkg, ora)
    fields = ("type", "sample", "sync_sample", "coding", "baud", "eye", "a", "b", "inv_a", "fiw_raw", "fiw", "fiw_rc", "sample_range",
              "sample_delta", "cycle", "frame", "nr_phases")
    want = sorted((int(e["channel"]), k[1] * W) + tuple(int(e[f]) for f in fields) for k, v in by.items() for e in v[0])
    assert len(want) >= 2
    lines = [json.loads(ln) for ln in (tmp_path / "gated" / "flex.jsonl").read_text().splitlines()]
    assert sorted((ln["channel"], ln["first_sample"]) + tuple(ln[f] for f in fields) for ln in lines) == want
    clean = {3: " ", 4: " ", 0x17: " ", 8: "<BKSP>", 12: "<FF>"}
    want_pages = []
    for k, ms in chk.msgs.items():
        for kind, baud, phase, cycle, frame, a0, a1, _a2, cap, text in tf._pages(ms):
            head = (k[0], k[1] * W, baud, frame, cycle, "ABCD"[phase], cap)
            msg = "".join(clean.get(ch, chr(ch)) for ch in text)
            if kind == 1:
                want_pages.append(("alphanumeric",) + head + (bool(a0 & 1), bool(a0 & 2), a0 >> 2, msg))
            elif kind == 2:
                want_pages.append(("numeric",) + head + (msg,))
            elif a0 == 0:
                want_pages.append(("tempAddrActivation",) + head + (a1 & 0x7F, (a1 >> 7) & 0xF))
    assert len(want_pages) >= 6
    pages = [json.loads(ln) for ln in (tmp_path / "gated" / "pages.jsonl").read_text().splitlines()]
    assert all(p["proto"] == "flex" for p in pages)
    got_pages = []
    for p in pages:
        head = (p["type"], p["channel"], p["first_sample"], p["baud"], p["frameNo"], p["cycleNo"], p["phaseNo"], p["capCode"])
        rest = {"alphanumeric": ("fragment", "maildrop", "fragSeq", "message"), "numeric": ("message",),
                "tempAddrActivation": ("startFrameNo", "tempAddressId")}[p["type"]]
        got_pages.append(head + tuple(p[f] for f in rest))
    assert sorted(got_pages, key=repr) == sorted(want_pages, key=repr)
    r = subprocess.run(cmd[:-5] + ["--gate-flex"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-flex needs --gate-resample" in r.stderr
    for other in ("--gate-ais", "--gate-pocsag"):
        r = subprocess.run(cmd + [other], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "exclude each other" in r.stderr
