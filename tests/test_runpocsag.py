"""The burst POCSAG stage (mfm_runpocsag_*, csrc/mfm_runpocsag.hip): the runs the burst resampler left go through the POCSAG
demodulator, one fresh demodulator per stretch.

The expected result is the oracle's, never the code under test: the restated gate (tests/test_gate.py, test_gate_preroll.py),
the oracle resampler per stretch (test_runrs.Checker) and a fresh oracle_lib.Pocsag() per stretch, fed run by run and passed
through the _dedupe rule of tests/test_pocsag.py, so an event belongs to the call and run whose [first_out, first_out + nr_out)
holds its `sample`.  Every comparison is an equality of every field of every event."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_pocsag as tp
import test_runais as tra
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runpocsag_create", "mfm_runpocsag_destroy", "mfm_runpocsag_process_device", "mfm_runpocsag_fetch",
             "mfm_runpocsag_device_view", "mfm_runpocsag_fetch_state", "mfm_hosttwin_runpocsag_call", "mfm_runpocsag_store_state",
             "mfm_hosttwin_runpocsag_state_check"]
RATIOS = [(4, 5, 41), (1, 1, 4)]   # interpolate, decimate, taps
WINDOWS = [7, 64, 500]
NCH = 4
N_OUT = {7: 40000, 64: 120000, 500: 120000}   # samples per channel at 38 400 Hz; W = 7 has a shorter scene, 2400 baud only
EVENT_FIELDS = ("type", "baud", "channel", "aux", "run", "nr_ok", "fail_mask", "reserved", "stretch_window", "sample", "raw", "corrected")
ORACLE_FIELDS = ("type", "baud", "aux", "sample", "nr_ok", "fail_mask", "raw", "corrected")
SPB = {512: 75, 1200: 32, 2400: 16}
HIST = 32 * 75                     # samples a detector looks back, the tail the stage carries
SPACING = 544 * 16


def rs_taps(pkg, ora, ratio):
    if ratio[2] == 41:
        return ora.quantize_taps(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4)   # as test_ais and test_runais
    return ora.quantize_taps([0.1, 0.4, 0.4, 0.1])


def slots(nr_out):
    """the event bound of a run, re-derived: at most nr_out // 8704 + 1 BATCH events (544 bit periods of 16 samples or more
    between two), at most two other events between two of them, in front of the first and behind the last"""
    return 3 * (int(nr_out) // SPACING + 1) + 2


# ---- the checker --------------------------------------------------------------------------------------------

class Checker:
    """what the stage must return for the gate calls of one stream, from the oracle; and what the guards read"""

    def __init__(self, pkg, ora, taps, I, D, W):
        self.pkg, self.ora = pkg, ora
        self.rs = tr.Checker(pkg, ora, taps, I, D, False, W)
        self.chan = {}      # channel -> [decoder, key of the stretch]
        self.by = {}        # (channel, first window) -> events
        self.msgs = {}      # (channel, first window) -> the embedded message layer's messages
        self.pcm = {}       # (channel, first window) -> resampled pieces
        self.bounds = {}    # (channel, first window) -> first_out of every run but the first: the handovers
        self.multi = 0      # calls in which a channel has two runs or more

    def call(self, gate_runs, gate_payload):
        dt = self.pkg.binding.RUNPOCSAG_EVENT_DTYPE
        runs, payload = self.rs.call(gate_runs, gate_payload)
        parts = []
        ch = [int(c) for c in runs["channel"]]
        self.multi += len(set(ch)) < len(ch)
        for i, r in enumerate(runs):
            c, fo, n = int(r["channel"]), int(r["first_out"]), int(r["nr_out"])
            if int(r["flags"]) & 1:
                key = (c, int(r["first_window"]))
                self.chan[c] = [self.ora.Pocsag(), key]
                self.by[key], self.pcm[key], self.bounds[key], self.msgs[key] = [], [], [], []
            else:
                self.bounds[self.chan[c][1]].append(fo)
            st = self.chan[c]
            y = payload[int(r["out_offset"]):int(r["out_offset"]) + n]
            e, m = st[0].feed(y)
            e = tp._dedupe(e, self.ora)
            ev = np.zeros(len(e), dt)
            for f in ORACLE_FIELDS:
                ev[f] = e[f]
            ev["channel"], ev["run"], ev["stretch_window"] = c, i, st[1][1]
            assert ((ev["sample"] >= fo) & (ev["sample"] < fo + n)).all()
            self.by[st[1]].append(ev)
            self.msgs[st[1]] += m
            self.pcm[st[1]].append(y)
            parts.append(ev)
        ev = np.concatenate(parts) if parts else np.zeros(0, dt)
        return (runs, payload), ev

    def stretches(self):
        """{(channel, first window): events without `run`}; each stretch once more through a fresh decoder in one piece"""
        dt = self.pkg.binding.RUNPOCSAG_EVENT_DTYPE
        out = {}
        for key, evs in self.by.items():
            ev = np.concatenate(evs) if evs else np.zeros(0, dt)
            whole, msgs = self.ora.Pocsag().feed(np.concatenate(self.pcm[key]))
            whole = tp._dedupe(whole, self.ora)
            assert len(whole) == len(ev), key
            for f in ORACLE_FIELDS:
                assert np.array_equal(whole[f], ev[f]), (key, f)
            assert msgs == self.msgs[key], key
            ev = ev.copy()
            ev["run"] = 0
            out[key] = ev
        return out


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape,
                                                                 [(int(e["type"]), int(e["sample"])) for e in got][:8],
                                                                 [(int(e["type"]), int(e["sample"])) for e in want][:8])
    for f in EVENT_FIELDS if len(want) else ():
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, f"{what}: event field {f} differs at {bad[:5].tolist()}: {got[f][bad[0]]} != {want[f][bad[0]]}"


# ---- scenes ---------------------------------------------------------------------------------------------------

_SCENE = {}


def _tx(sy, ora, kind, seed):
    """one transmission at 38 400 Hz without lead or trail: (pcm, baud)"""
    msgs = tp._messages(sy)
    first = 576 + 32
    if kind == "long2400":   # four batches or more; the second sync word with 4 flipped bits (kept), the third with 5 (lost)
        bits = sy.pocsag_bits(sy.pocsag_batches(msgs + msgs))
        assert bits.size >= 576 + 4 * 544
        s2, s3 = 576 + 544, 576 + 2 * 544
        flips = [s2 + 1, s2 + 8, s2 + 20, s2 + 31, s3 + 0, s3 + 3, s3 + 9, s3 + 17, s3 + 25]
        return sy.pocsag_pcm(bits, 2400, noise=200, seed=seed, flip=flips), 2400
    if kind == "short2400":
        return sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches(msgs[:1 + seed % 2])), 2400, noise=300, seed=seed), 2400
    if kind == "one1200":
        return sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches([msgs[seed % 2]])), 1200, noise=500, seed=seed), 1200
    assert kind == "one512"   # one batch with single and double errors and one uncorrectable triple
    bits = sy.pocsag_bits(sy.pocsag_batches([msgs[0]]))
    assert bits.size == 576 + 544
    flips = [first + 32 * 1 + 4, first + 32 * 6 + 2, first + 32 * 6 + 29, first + 32 * 7 + 11] + \
        [first + 32 * 9 + b for b in tp._uncorrectable_triple(ora, bits, first + 32 * 9)]
    return sy.pocsag_pcm(bits, 512, noise=400, seed=seed, flip=flips), 512


def scene(pkg, ora, ratio, W):
    """four channels at 38 400 Hz, the input in front of the resampler and where each transmission lies at 38 400 Hz:
    0: 2400 baud, a long transmission (a kept and a lost sync word) with another one soon after the loss, and more behind;
    1: 1200 baud, sparse one-batch transmissions with near silence between them; 2: noise, then uniform random samples;
    3: 512 baud, one one-batch transmission with single, double and one uncorrectable triple error.
    W = 7: shorter, 2400 baud only.  Made once per (ratio, W) and left unchanged"""
    short = W == 7
    key = (ratio, short)
    if key in _SCENE:
        return _SCENE[key]
    sy = pkg.synth
    I, D, _ = ratio
    n = N_OUT[W]
    rng = np.random.RandomState(5)
    plan = {0: [("long2400", 1500)], 1: [("one1200", 2000), ("one1200", 41040), ("one1200", 80080)],
            2: [], 3: [("one512", 6000)]}
    if short:
        plan = {0: [("short2400", 900)], 1: [("short2400", 2500)], 2: [], 3: [("short2400", 300)]}
    chans, tx = [], {}
    for c in range(NCH):
        x = (rng.randn(n) * 60).round().astype(np.int16)   # near silence
        if c == 2:
            x[:n // 2] = rng.normal(0, 2000, n // 2).round().astype(np.int16)
            x[n // 2:] = rng.randint(-32768, 32768, n - n // 2).astype(np.int16)
        tx[c] = []
        at_next = 0
        for k, (kind, at) in enumerate(plan[c]):
            p, baud = _tx(sy, ora, kind, 10 * c + k)
            at = max(at, at_next)
            assert at + p.size <= n, (c, kind, at, p.size, n)
            x[at:at + p.size] = p
            tx[c].append((at, at + p.size, baud))
            at_next = at + p.size
            if kind == "long2400":   # the lost sync word ends at bit 576 + 2 * 544 + 32; one transmission re-synchronises soon after
                lost = at + (576 + 2 * 544 + 32) * 16
                for j in range(2):
                    q, _ = _tx(sy, ora, "short2400", 3 + j)
                    a2 = at_next + 700 + 2600 * j
                    if a2 + q.size + HIST + 600 <= n:
                        x[a2:a2 + q.size] = q
                        tx[c].append((a2, a2 + q.size, 2400))
                        at_next = a2 + q.size
                assert lost < at_next
        chans.append(x)
    x38 = np.stack(chans)
    n_in = n * D // I
    stream = np.stack([np.repeat(x, D)[::I][:n_in] for x in x38])   # for 4/5: np.repeat(x, 5)[::4], as test_runais.scene
    _SCENE[key] = dict(stream=np.ascontiguousarray(stream), tx=tx, n_in=n_in, D=D, I=I)
    return _SCENE[key]


def bit_at(sc, t, bit):
    """input position of bit `bit` of transmission t = (start, end, baud)"""
    return (t[0] + bit * SPB[t[2]]) * sc["D"] // sc["I"]


def make_mask(kind, sc, W, rng):
    """raw squelch verdicts [C][nw]"""
    nw = sc["n_in"] // W
    m = np.zeros((NCH, nw), bool)
    if kind == "open":
        return ~m
    if kind == "short":   # W = 7: stretches of one or two windows, one channel open all the time
        for c in range(NCH - 1):
            k = int(rng.randint(0, 3))
            while k < nw:
                ln = int(rng.randint(1, 3))
                m[c, k:k + ln] = True
                k += ln + 2 + int(rng.randint(1, 3))
        m[NCH - 1] = True
        return m
    lead = 200 * sc["D"] // sc["I"] // W + 1
    behind = (HIST + 400) * sc["D"] // sc["I"] // W + 2   # 32 * 75 samples and more behind a transmission: SYNC_LOST arrives
    k = 0
    for c in range(NCH):
        for t in sc["tx"][c]:
            ka, kb = bit_at(sc, t, 0) // W - lead, t[1] * sc["D"] // sc["I"] // W + behind
            if kind == "cut":
                if k % 3 == 0:
                    kb = bit_at(sc, t, 576 + 32 + 300) // W      # closes inside a batch
                elif k % 3 == 1:
                    ka = bit_at(sc, t, 200) // W                 # opens inside the preamble
                else:
                    ka = bit_at(sc, t, 576 + 32 + 100) // W      # opens inside a batch
            m[c, max(ka, 0):kb] = True
            k += 1
    if kind == "cut":   # the noise channel: seeded blocks, two or more runs of a channel in one call
        k = 0
        while k < nw:
            ln = int(rng.randint(300, 3000)) // W + 1
            m[2, k:k + ln] = True
            k += ln + int(rng.randint(100, 1500)) // W + 1
    return m


def anchors_of(sc, W):
    """input positions inside each walker state of the first transmissions: the preamble (SEARCH), a batch, the sync slot
    behind the first batch, and 1000 outputs behind the end (SEARCH, fewer than 2400 samples behind the reset)"""
    out = []
    for c in range(NCH):
        for t in sc["tx"][c][:2]:
            out += [bit_at(sc, t, 300), bit_at(sc, t, 576 + 32 + 256), bit_at(sc, t, 576 + 544 + 14), (t[1] + 1000) * sc["D"] // sc["I"]]
    return sorted(out)


def kinds_of(W):
    return ["open", "fitted", "cut"] + (["short"] if W == 7 else [])


def classify(ora, by, bounds, tally):
    """where the handovers lie, from the oracle's event times around each run boundary"""
    for key, ev in by.items():
        t = [int(x) for x in ev["type"]]
        s = [int(x) for x in ev["sample"]]
        if t and t[-1] != ora.EV_SYNC_LOST:
            tally["inside_end"] += 1   # the stretch ends inside a transmission: a FOUND without its LOST
        resets = [-1] + [s[i] for i in range(len(t)) if t[i] == ora.EV_SYNC_LOST]
        for b in bounds[key]:
            for i in range(1, len(t)):
                if s[i - 1] < b <= s[i]:
                    tally["in_batch"] += t[i] == ora.EV_BATCH
                    tally["in_sync"] += t[i] in (ora.EV_SYNC_KEPT, ora.EV_SYNC_LOST)
            for r0 in resets:
                nxt = min([x for x in s if x > r0] + [1 << 62])
                tally["in_search"] += r0 < b - 1 < r0 + HIST and b - 1 < nxt and r0 >= 0
    return tally


def run_scenes(pkg, ora, W, ratio, make_call, seed, pages=None):
    """every mask, P = 0 and 2 with the flush, each stream in the seeded cut and as one call; asserts the guards on the
    oracle's figures before any comparison"""
    I, D, _ = ratio
    sc = scene(pkg, ora, ratio, W)
    taps = rs_taps(pkg, ora, ratio)
    stream, n = sc["stream"], sc["n_in"]
    jobs = []
    tally = dict(in_batch=0, in_sync=0, in_search=0, inside_end=0, multi=0)
    open_ev = None
    for kind in kinds_of(W):
        for P in (0, 2):
            rng = np.random.RandomState(seed + 10 * kinds_of(W).index(kind) + P)
            mask = make_mask(kind, sc, W, rng)
            for single in (False, True):
                cuts = [n] if single else tra.make_cuts(rng, n, W, anchors_of(sc, W))
                calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
                chk = Checker(pkg, ora, taps, I, D, W)
                want = [chk.call(gr, gp) for gr, gp in calls]
                by = chk.stretches()
                emitted = tr.emitted_of(mask, P)[:, :n // W]
                assert sorted(by) == tr.stretches_of_mask(emitted)
                if kind == "open" and single:
                    open_ev = np.concatenate(list(by.values()))
                if kind != "open" and not single:
                    classify(ora, by, chk.bounds, tally)
                    tally["multi"] += chk.multi
                if kind == "fitted" and pages is not None:
                    pages(chk, by)
                jobs.append((kind, P, single, cuts, mask, calls, want, by))
    # the guards, on the oracle's result alone
    ev = open_ev
    batches = ev[ev["type"] == ora.EV_BATCH]
    if W != 7:
        assert len(batches) >= 12 and set(batches["baud"].tolist()) == {512, 1200, 2400}, (len(batches), set(batches["baud"].tolist()))
        assert ((ev["type"] == ora.EV_SYNC_KEPT) & (ev["aux"] != tp.SYNC)).any()
        assert (batches["fail_mask"] != 0).any()
        lost_found = False
        for c in range(NCH):
            t = ev["type"][ev["channel"] == c].tolist()
            lost_found |= any(a == ora.EV_SYNC_LOST and b == ora.EV_SYNC_FOUND for a, b in zip(t, t[1:]))
        assert lost_found
    else:
        assert len(batches) >= 3 and set(batches["baud"].tolist()) == {2400}
    assert tally["in_batch"] >= 1 and tally["in_sync"] >= 1 and tally["in_search"] >= 1 and tally["inside_end"] >= 1 and tally["multi"] >= 1, tally
    # the code under test
    for kind, P, single, cuts, mask, calls, want, by in jobs:
        what = f"W {W} {I}/{D} mask {kind} P {P} single {single}"
        call, done = make_call(NCH, W, P, cuts, stream, mask, taps, I, D)
        got_by = {}
        for i, ((gr, gp), (rs_want, ev_want)) in enumerate(zip(calls, want)):
            got = call(i, gr, gp, rs_want)
            same(got, ev_want, f"{what}, call {i}")
            for e in got:
                got_by.setdefault((int(e["channel"]), int(e["stretch_window"])), []).append(e)
        done()
        for k, v in by.items():   # cut independence: per stretch the same events however the stream was cut
            g = got_by.get(k, [])
            assert len(g) == len(v), (what, k)
            for a, b in zip(g, v):
                assert all(np.array_equal(a[f], b[f]) for f in EVENT_FIELDS if f != "run"), (what, k)


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runpocsag_names(pkg):
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
    assert b.RUNPOCSAG_EVENT_DTYPE.itemsize == 176 and C.sizeof(b.RunPocsagEvent) == 176 and C.sizeof(b.RunPocsagConfig) == 28
    assert b.RUNPOCSAG_STATE_DTYPE.itemsize == 432
    assert pkg.RUNPOCSAG_EVENT_DTYPE is b.RUNPOCSAG_EVENT_DTYPE and pkg.RunPocsag is b.RunPocsag
    assert pkg.hosttwin_runpocsag_call is b.hosttwin_runpocsag_call and pkg.runpocsag_to_pocsag_events is b.runpocsag_to_pocsag_events
    assert pkg.RUNPOCSAG_STATE_DTYPE is b.RUNPOCSAG_STATE_DTYPE and pkg.RunPocsagConfig is b.RunPocsagConfig
    m = re.search(r"struct mfm_runpocsag_event \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(uint\d+_t)\s+(\w+)(?:\[16\])?;", m.group(1))] == list(b.RUNPOCSAG_EVENT_DTYPE.names)
    assert list(b.RUNPOCSAG_EVENT_DTYPE.names) == [n for n, _ in b.RunPocsagEvent._fields_]
    for n, _ in b.RunPocsagEvent._fields_:
        assert b.RUNPOCSAG_EVENT_DTYPE.fields[n][1] == getattr(b.RunPocsagEvent, n).offset, n
    m = re.search(r"struct mfm_runpocsag_config \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == [n for n, _ in b.RunPocsagConfig._fields_]
    m = re.search(r"struct mfm_runpocsag_state \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+)(?:\[\d+\])?;", m.group(1))] == list(b.RUNPOCSAG_STATE_DTYPE.names)
    for name in ("OVER_RUNS", "OVER_EVENTS", "IN_RUNRS", "IN_OUT_OF_STEP", "IN_BAD_RUNS"):
        m = re.search(r"#define\s+MFM_RUNPOCSAG_%s\s+(\d+)u\b" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNPOCSAG_" + name)
    assert b.runpocsag_slots(0) == slots(0) == 5 and b.runpocsag_slots(8703) == 5 and b.runpocsag_slots(8704) == slots(8704) == 8


def _twin_call(pkg):
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        state = b.hosttwin_runpocsag_state(nch)

        def call(i, gr, gp, rs_want):
            return b.hosttwin_runpocsag_call(state, *rs_want)   # max_events 0: the default never refuses

        return call, lambda: None

    return make_call


def _pages_check(pkg, found):
    """events converted and fed to a fresh host pager per stretch give the pages of the oracle's embedded message layer"""
    def pages(chk, by):
        for key, ev in by.items():
            hp = tp.HostPager()
            conv = pkg.binding.runpocsag_to_pocsag_events(ev)
            half = len(conv) // 2
            hp.on_events(conv[:half])
            hp.on_events(conv[half:])
            hp.close()
            assert hp.pages == [(m[0], m[1], m[2], m[3], m[4]) for m in chk.msgs[key]], key
            found[0] += len(hp.pages)
    return pages


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_hosttwin_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """csrc/mfm_runpocsag.h and the twin's sample-by-sample decoder on the scenes of the GPU tests; the pages a fresh host
    pager per stretch assembles from the fitted mask's events are the oracle's"""
    found = [0]
    run_scenes(pkg, ora, W, ratio, _twin_call(pkg), 7 * W + ratio[0], pages=_pages_check(pkg, found))
    assert found[0] >= 1


def _pieces(pkg, ora):
    """one stretch per channel cut into runs by hand, at any sample: channel 0 carries the 2400 baud channel of the 1/1 scene
    and channel 1 the 512 baud one, both resampled by the oracle.  Returns the calls [(runs, payload)] and the oracle's events
    per call.  Cuts lie on and around event samples, inside batches and sync slots, as runs of one sample and runs without
    output; channel 1 sits out every third call"""
    b = pkg.binding
    ratio = RATIOS[1]
    sc = scene(pkg, ora, ratio, 64)
    taps = rs_taps(pkg, ora, ratio)
    pcm = [ora.Resampler(taps, 1, 1).feed(sc["stream"][c])[:70000] for c in (0, 3)]
    whole = [tp._dedupe(ora.Pocsag().feed(x)[0], ora) for x in pcm]
    assert len(whole[0]) >= 8 and len(whole[1]) >= 1
    s0 = [int(e["sample"]) for e in whole[0]]
    marks = [[s0[0], s0[0] + 1, s0[0] + 7, s0[1], s0[1] + 1, s0[1] + 3, s0[2], s0[2] + 1, s0[3] - 1, s0[4] + 2400, s0[5] - 100,
              9000, 9001, 9002, 9003, 9003, 9100, 30000, 30001],
             [5, 5, 60, 100, 2399, 2400, 2401, 4800, 20000, int(whole[1][0]["sample"]), int(whole[1][0]["sample"]) + 1, 60000]]
    cuts = [sorted(m) + [x.size] for m, x in zip(marks, pcm)]
    calls, want = [], []
    dem = [ora.Pocsag(), ora.Pocsag()]
    at, nxt, i = [0, 0], [0, 0], 0
    while nxt[0] < len(cuts[0]) or nxt[1] < len(cuts[1]):
        runs, parts, evs = [], [], []
        for c in (0, 1):
            if nxt[c] >= len(cuts[c]) or (c == 1 and i % 3 == 2):   # channel 1 sits out every third call and keeps its state
                continue
            end = cuts[c][nxt[c]]
            nxt[c] += 1
            y = pcm[c][at[c]:end]
            runs.append((7 + c, sum(p.size for p in parts), at[c], c, y.size, int(at[c] == 0 and nxt[c] == 1), 0))
            parts.append(y)
            e = tp._dedupe(dem[c].feed(y)[0], ora)
            ev = np.zeros(len(e), b.RUNPOCSAG_EVENT_DTYPE)
            for f in ORACLE_FIELDS:
                ev[f] = e[f]
            ev["channel"], ev["run"], ev["stretch_window"] = c, len(runs) - 1, 7 + c
            evs.append(ev)
            at[c] = end
        calls.append((np.array(runs, b.RUNRS_RUN_DTYPE), np.concatenate(parts) if parts else np.zeros(0, np.int16)))
        want.append(np.concatenate(evs) if evs else np.zeros(0, b.RUNPOCSAG_EVENT_DTYPE))
        i += 1
    assert at[0] == pcm[0].size and at[1] == pcm[1].size and sum(len(w) for w in want) == len(whole[0]) + len(whole[1])
    assert any(len(r) and (r["nr_out"] == 0).any() for r, _ in calls) and any(len(r) and (r["nr_out"] == 1).any() for r, _ in calls)
    return calls, want


def test_hosttwin_handovers_at_any_sample(pkg, ora):
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    state = b.hosttwin_runpocsag_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(b.hosttwin_runpocsag_call(state, runs, payload), w, f"call {i}")


def _refusal_case(pkg, ora):
    """two calls of the hand-cut stretches that both carry runs of both channels, and what is wrong with the second"""
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    i = next(i for i in range(3, len(calls)) if len(calls[i][0]) == 2 and len(want[i]) and calls[i][0]["nr_out"].min() > 0)
    runs, payload = calls[i]
    bound = sum(slots(n) for n in runs["nr_out"])

    def changed(field, k, value):
        r = runs.copy()
        r[field][k] = value
        return r

    cases = [
        (dict(totals=[2, payload.size, 1, 0]), "overflow or gate error", b.MFM_RUNPOCSAG_IN_RUNRS << 8),
        (dict(totals=[2, payload.size, 0, 2]), "overflow or gate error", b.MFM_RUNPOCSAG_IN_RUNRS << 8),
        (dict(runs=changed("first_out", 0, int(runs["first_out"][0]) + 1)), "out of step", b.MFM_RUNPOCSAG_IN_OUT_OF_STEP << 8),
        (dict(runs=changed("channel", 0, 1)), "out of step", b.MFM_RUNPOCSAG_IN_OUT_OF_STEP << 8),   # channel 1's second run continues
        (dict(runs=changed("channel", 1, 2)), "does not exist", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),
        (dict(runs=changed("flags", 0, 1)), "does not exist", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),     # begins with first_out != 0
        (dict(runs=runs[::-1].copy()), "does not exist", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),          # channels descend
        (dict(runs=changed("out_offset", 1, payload.size + 1)), "does not exist", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),
        (dict(runs=changed("nr_out", 1, payload.size)), "does not exist", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),
    ]
    capacity = [
        (dict(max_out_samples=payload.size - 1), "max_out_samples", b.MFM_RUNPOCSAG_IN_BAD_RUNS << 8),
        (dict(max_runs=1), "max_runs", b.MFM_RUNPOCSAG_OVER_RUNS),
        (dict(max_events=bound - 1), "event bound", b.MFM_RUNPOCSAG_OVER_EVENTS),
    ]
    return calls, want, i, cases, capacity, bound


def test_hosttwin_refuses_and_leaves_its_state(pkg, ora):
    b = pkg.binding
    calls, want, at, cases, capacity, bound = _refusal_case(pkg, ora)
    state = b.hosttwin_runpocsag_state(2)
    for i in range(at):
        same(b.hosttwin_runpocsag_call(state, *calls[i]), want[i], f"call {i}")
    s0 = state.copy()
    assert s0["has_stretch"].all() and (s0["outs"] > 0).all()
    runs, payload = calls[at]
    for change, message, flags in cases + capacity:
        kw = dict(runs=runs, payload=payload)
        kw.update(change)
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runpocsag_call(state, kw.pop("runs"), kw.pop("payload"), **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value))
        assert ei.value.needed == 0 and state.tobytes() == s0.tobytes()
    with pytest.raises(pkg.MfmError) as ei:   # the caller's array is too small: nothing moves either
        b.hosttwin_runpocsag_call(state, runs, payload, max_out=len(want[at]) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(want[at]) and state.tobytes() == s0.tobytes()
    same(b.hosttwin_runpocsag_call(state, runs, payload, max_events=bound), want[at], "the same call, right")   # the bound itself fits
    for i in range(at + 1, len(calls)):
        same(b.hosttwin_runpocsag_call(state, *calls[i]), want[i], f"call {i}")


def test_hosttwin_refuses_by_the_bound_even_without_an_event(pkg):
    """a noise scene with no event at all: max_events one below the bound is refused, the bound and the default are not"""
    b = pkg.binding
    rng = np.random.RandomState(3)
    payload = rng.normal(0, 2000, 3 * SPACING + 10).round().astype(np.int16)
    sizes = [SPACING - 1, SPACING, payload.size - 2 * SPACING + 1]
    runs = np.array([(c, sum(sizes[:c]), 0, c, n, 1, 0) for c, n in enumerate(sizes)], b.RUNRS_RUN_DTYPE)
    bound = sum(slots(n) for n in sizes)
    assert bound == 5 + 8 + 8
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runpocsag_call(b.hosttwin_runpocsag_state(3), runs, payload, max_events=bound - 1)
    assert ei.value.code == b.MFM_E_STATE and "event bound" in str(ei.value) and ei.value.flags == b.MFM_RUNPOCSAG_OVER_EVENTS
    for me in (bound, 0):
        assert len(b.hosttwin_runpocsag_call(b.hosttwin_runpocsag_state(3), runs, payload, max_events=me)) == 0


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
    """every refusal of mfm_runpocsag_create is decided before a device is looked for"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_out_samples=10000)
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunPocsag(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_runpocsag_to_pocsag_events_arithmetic(pkg):
    b = pkg.binding
    ev = np.zeros(3, b.RUNPOCSAG_EVENT_DTYPE)
    ev["type"], ev["baud"], ev["channel"], ev["aux"] = [1, 2, 3], [512, 1200, 2400], [2, 0, 5], [40, 0, 0x7CD215D9]
    ev["run"], ev["nr_ok"], ev["fail_mask"], ev["reserved"] = [9, 8, 7], [0, 12, 0], [0, 0x1000, 0], 0
    ev["stretch_window"], ev["sample"] = [0, 3, (1 << 40) + 1], [1500, 99, (1 << 33) + 7]
    ev["raw"] = np.arange(48).reshape(3, 16) * 0x01010101
    ev["corrected"] = ev["raw"] & 0x7FFFFFFF
    out = b.runpocsag_to_pocsag_events(ev)
    assert out.dtype == b.POCSAG_EVENT_DTYPE and out.shape == (3,)
    for f in ("type", "baud", "channel", "aux", "sample", "nr_ok", "fail_mask", "raw", "corrected"):
        assert np.array_equal(out[f], ev[f]), f   # the stretch-relative sample is kept
    assert b.runpocsag_to_pocsag_events(ev[:0]).shape == (0,)


def test_runpocsag_kernels_use_no_scratch(pkg):
    """the code object's notes of build/mfm_runpocsag.o (tools/kernel_regs.py): the seven kernels, no private segment, no spilled
    vector register, at most 128 VGPRs"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runpocsag.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"rp_{k}_kernel" for k in ("plan", "slice", "match", "walk", "evscan", "compact", "state")), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(5))) == (0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gpu_call(pkg):
    """a real Gate (process_host, flush_device) -> RunResampler -> RunPocsag on the device views, no fetch in between; the
    twin runs beside it on the oracle's run lists: same events, and the same state after the last call"""
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        cap = max(max(cuts), 1)
        gate = pkg.Gate(nch, cap, W, preroll_windows=P)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P)
        rp = pkg.RunPocsag.behind(rr)
        twin = b.hosttwin_runpocsag_state(nch)
        pos = [0]

        def call(i, gr, gp, rs_want):
            if i < len(cuts):
                m = cuts[i]
                gate.process_host(stream[:, pos[0]:pos[0] + m], tg.records_of(pkg, mask, pos[0] // W, (pos[0] + m) // W))
                pos[0] += m
            else:
                gate.flush_device()
            rr.process_device(*gate.device_view())
            rp.process_device(*rr.device_view())
            got = rp.fetch()
            d_ev, d_tot = rp.device_view()
            tot = tl._d2h(d_tot, 32).view(np.uint64)
            assert tot.tolist() == [len(got), len(rs_want[0]), 0, 0], (i, tot.tolist())
            if len(got):
                assert tl._d2h(d_ev, got.nbytes).tobytes() == got.tobytes()
            tr.same(rr.fetch(), rs_want, f"the resampler's call {i}")
            same(b.hosttwin_runpocsag_call(twin, *rs_want), got, f"the twin's call {i}")
            return got

        def done():
            state = rp.fetch_state()
            assert state.tobytes() == twin.tobytes(), [f for f in state.dtype.names if not np.array_equal(state[f], twin[f])]
            rp.close()
            rr.close()
            gate.close()

        return call, done

    return make_call


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """four channels; all open, windows fitted to the transmissions, a mask that closes and opens inside batches and preambles,
    at W = 7 stretches of one or two windows; P = 0 and 2 with the flush fed through; cut into calls inside every walker state,
    as one-window and nr_in = 0 calls, and as one call, with identical events per stretch; device_view totals, the twin's
    events and the twin's state beside it"""
    run_scenes(pkg, ora, W, ratio, _gpu_call(pkg), 7 * W + ratio[0])


def _fed(pkg, torch, rp, runs, payload, totals=None):
    """one call from uploaded arrays: a burst resampler's result as it would stand in its device view"""
    t = np.array([len(runs), payload.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
    rp.process_device(*(k.data_ptr() for k in keep))
    try:
        return rp.fetch()
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_handovers_at_any_sample(pkg, ora):
    import torch
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    rp = pkg.RunPocsag(2, 4, max(p.size for _, p in calls) + 1)
    twin = b.hosttwin_runpocsag_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(_fed(pkg, torch, rp, runs, payload), w, f"call {i}")
        b.hosttwin_runpocsag_call(twin, runs, payload)
        assert rp.fetch_state().tobytes() == twin.tobytes(), i
    rp.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state(pkg, ora):
    """the resampler's flags handed through, out of step, run lists that are not a resampler's, max_runs, the event bound
    against max_events: each time nothing comes out and the state stays, so the same call fed correctly is right"""
    import torch
    b = pkg.binding
    calls, want, at, cases, _, _ = _refusal_case(pkg, ora)
    runs, payload = calls[at]
    cap = max(p.size for _, p in calls) + 1
    rp = pkg.RunPocsag(2, 4, cap)
    for i in range(at):
        same(_fed(pkg, torch, rp, *calls[i]), want[i], f"call {i}")
    s0 = rp.fetch_state()
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rp, change.get("runs", runs), payload, totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == 0 and not ei.value.buffer.view(np.uint8).any()
        assert rp.fetch_state().tobytes() == s0.tobytes(), change
    got = _fed(pkg, torch, rp, runs, payload)
    same(got, want[at], "the same call, right, after the refused ones")
    with pytest.raises(pkg.MfmError) as ei:
        rp.fetch(max_events=len(got) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(got) and not ei.value.buffer.view(np.uint8).any()
    same(rp.fetch(), want[at], "fetched again")
    for i in range(at + 1, len(calls)):
        same(_fed(pkg, torch, rp, *calls[i]), want[i], f"call {i}")
    rp.close()
    # what an object is too small for: the first call, whose runs begin their stretches, against max_runs, max_out_samples and
    # max_events; the event bound itself fits
    runs, payload = calls[0]
    bound = sum(slots(n) for n in runs["nr_out"])
    assert len(runs) == 2 and (runs["flags"] == 1).all()
    for kw, message in ((dict(max_runs=1), "max_runs"), (dict(max_out_samples=payload.size - 1), "max_out_samples"),
                        (dict(max_events=bound - 1), "event bound")):
        args = dict(max_runs=4, max_out_samples=cap, max_events=0)
        args.update(kw)
        rp = pkg.RunPocsag(2, **args)
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rp, runs, payload)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (kw, str(ei.value))
        rp.close()
    rp = pkg.RunPocsag(2, 2, payload.size, max_events=bound)
    same(_fed(pkg, torch, rp, runs, payload), want[0], "call 0 on an object made for it")
    rp.close()


@pytest.mark.gpu
def test_gpu_two_stages_on_two_streams_behind_one_resampler(pkg, ora):
    """two stage objects on streams of their own, ordered behind the resampler's call by a synchronisation, read the same
    device view and give identical results"""
    import torch
    W, ratio = 64, RATIOS[0]
    I, D, _ = ratio
    sc = scene(pkg, ora, ratio, W)
    taps = rs_taps(pkg, ora, ratio)
    stream, n = sc["stream"], sc["n_in"]
    mask = make_mask("cut", sc, W, np.random.RandomState(1))
    cuts = [n // 3 // W * W, n - n // 3 // W * W]
    calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
    chk = Checker(pkg, ora, taps, I, D, W)
    want = [chk.call(gr, gp) for gr, gp in calls]
    assert sum(len(e) for _, e in want) >= 5
    gate = pkg.Gate(NCH, max(cuts), W)
    rr = pkg.RunResampler(NCH, taps, I, D, W, max_in_samples=max(cuts))
    stages = [pkg.RunPocsag.behind(rr), pkg.RunPocsag.behind(rr)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pos = 0
    for i, m in enumerate(cuts):
        gate.process_host(stream[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W))
        pos += m
        rr.process_device(*gate.device_view())
        torch.cuda.synchronize()
        view = rr.device_view()
        for s, st in zip(stages, streams):
            s.process_device(*view, stream=st.cuda_stream)
        got = [s.fetch() for s in stages]
        same(got[0], want[i][1], f"call {i}, the first stage")
        same(got[1], got[0], f"call {i}, the second stage")
    assert stages[0].fetch_state().tobytes() == stages[1].fetch_state().tobytes()
    for o in stages + [rr, gate]:
        o.close()


CHAIN = dict(fs=1200000, decim=25, offsets=(-150000, 100000), W=100, P=1, blk=50021, hang=12)
_CHAIN = {}


def _chain(pkg, ora):
    """two channels of FM POCSAG bursts at 2400 baud (short preambles, one batch each, noise between them) at 1.2 MS/s,
    D = 25 -> 48 kHz; the oracle's PCM, the squelch on the PCM energy (a carrier lowers it) with a hang that outlasts the sync
    slot behind a batch, and the 4/5 resampler taps as the scan tool quantises them"""
    if _CHAIN:
        return _CHAIN["it"]
    sy, s = pkg.synth, CHAIN
    fs, decim, W = s["fs"], s["decim"], s["W"]
    msgs = tp._messages(sy)
    taps = sy.design_lpf(128, 12500.0, float(fs))
    gap = 200 * 250   # 20 windows of PCM: longer than the hang
    parts = []
    for k, o in enumerate(s["offsets"]):
        acc = []
        for j in range(2 - k):
            bits = sy.pocsag_bits(sy.pocsag_batches([msgs[(k + j) % 2]]), preamble_bits=160)
            acc.append(sy.synth_iq(gap + 3000 * (k + j), fs, [], seed=10 * k + j, noise=300).astype(np.int32))
            acc.append(sy.pocsag_fm_iq(bits, 2400, fs, o, amplitude=6000.0, noise=300.0, seed=3 * k + j).astype(np.int32))
        acc.append(sy.synth_iq(gap + (0 if k else 1), fs, [], seed=50 + k, noise=300).astype(np.int32))
        parts.append(np.concatenate(acc))
    n = max(p.shape[0] for p in parts)
    parts = [np.concatenate([p, sy.synth_iq(n - p.shape[0], fs, [], seed=70 + k, noise=300).astype(np.int32)]) if p.shape[0] < n else p
             for k, p in enumerate(parts)]
    iq = np.clip(sum(parts), -32768, 32767).astype(np.int16)
    offs, gains = np.array(s["offsets"], np.float64), np.ones(2)
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm = ora.run_channels(iq, cre, cim, incr, decim)[0]
    e = tl.restate(pkg, pcm, W, tl.PCM)["energy"].astype(np.float64)
    thr = int(np.sqrt(e.min() * e.max()))
    mask = tl.restate(pkg, pcm, W, tl.PCM, sense=tl.BELOW, open_thr=thr, close_thr=thr, hang=s["hang"])["open"].astype(bool)
    lpf = [float(x) for x in sy.design_lpf(41, 0.45 / 5, 1.0) * 4]
    rtaps = np.array([int(x * 16384.0) for x in lpf], np.int16)
    _CHAIN["it"] = dict(iq=iq, pcm=pcm, taps=taps, thr=thr, mask=mask, lpf=lpf, rtaps=rtaps, offs=offs)
    return _CHAIN["it"]


def _chain_want(pkg, ora):
    """the checker over the chain scene as the tool runs it: every block, then the flush"""
    sc, s = _chain(pkg, ora), CHAIN
    W, P = s["W"], s["P"]
    chk = Checker(pkg, ora, sc["rtaps"], 4, 5, W)
    n = sc["pcm"].shape[1]
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n))
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True))
    return chk, chk.stretches()


def test_chain_scene_is_what_it_is_meant_to_be(pkg, ora):
    """the recorded scene of the tool test, from the oracle alone: every channel opens and closes, the oracle finds every
    batch and delivers pages"""
    sc, s = _chain(pkg, ora), CHAIN
    emitted = tgp.dilate(sc["mask"], s["P"])
    assert all(sum(1 for k in tr.stretches_of_mask(emitted) if k[0] == c) >= 1 for c in range(2)) and not emitted.all(axis=1).any()
    chk, by = _chain_want(pkg, ora)
    ev = np.concatenate(list(by.values()))
    assert int((ev["type"] == ora.EV_BATCH).sum()) >= 3 and int((ev["type"] == ora.EV_SYNC_LOST).sum()) >= 3
    assert sum(len(m) for m in chk.msgs.values()) >= 3


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_pocsag_writes_the_events_and_pages_of_the_oracle(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-out DIR --gate-preroll 1 --gate-resample 4/5 --resample-taps FILE --gate-pocsag as a fresh
    child process on the chain scene: pocsag.jsonl holds the oracle's events and pages.jsonl its pages, stretch by stretch"""
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
           "--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-pocsag"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    chk, by = _chain_want(pkg, ora)
    want = sorted((int(e["channel"]), k[1] * W, int(e["type"]), int(e["baud"]), int(e["sample"]), int(e["aux"]), int(e["nr_ok"]),
                   int(e["fail_mask"]), tuple("%08x" % int(w) for w in e["corrected"]) if int(e["type"]) == ora.EV_BATCH else ())
                  for k, v in by.items() for e in v)
    assert len(want) >= 9
    lines = [json.loads(ln) for ln in (tmp_path / "gated" / "pocsag.jsonl").read_text().splitlines()]
    got = sorted((ln["channel"], ln["first_sample"], ln["type"], ln["baud"], ln["sample"], ln["aux"], ln["nr_ok"], ln["fail_mask"],
                  tuple(ln["corrected"])) for ln in lines)
    assert got == want
    text = {2: "alphanumeric", 3: "numeric"}
    clean = {3: " ", 4: " ", 0x17: " "}
    want_pages = sorted((k[0], k[1] * W, text[m[0]], m[1], m[2], m[3], "".join(clean.get(ch, chr(ch)) for ch in m[4]))
                        for k, ms in chk.msgs.items() for m in ms)
    assert len(want_pages) >= 3
    pages = [json.loads(ln) for ln in (tmp_path / "gated" / "pages.jsonl").read_text().splitlines()]
    assert all(p["proto"] == "pocsag" for p in pages)
    assert sorted((p["channel"], p["first_sample"], p["type"], p["baud"], p["capCode"], p["function"], p["message"]) for p in pages) == want_pages
    r = subprocess.run(cmd[:-5] + ["--gate-pocsag"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-pocsag needs --gate-resample" in r.stderr
    r = subprocess.run(cmd + ["--gate-ais"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "exclude each other" in r.stderr
