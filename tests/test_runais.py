"""The burst AIS stage (mfm_runais_*, csrc/mfm_runais.hip): the runs the burst resampler left go through the AIS demodulator,
one fresh demodulator per stretch.

The expected result is the oracle's, never the code under test: the restated gate (tests/test_gate.py, test_gate_preroll.py),
the oracle resampler per stretch (test_runrs.Checker) and a fresh sequential demodulator per stretch (tests/ais_ref.py), fed run
by run, so an event belongs to the call and run whose [first_out, first_out + nr_out) holds its `sample`.  Every comparison
is an equality of every field of every event."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ais_ref
import test_ais as ta
import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runais_create", "mfm_runais_destroy", "mfm_runais_process_device", "mfm_runais_fetch", "mfm_runais_device_view",
             "mfm_runrs_get_capacity", "mfm_hosttwin_runais_call", "mfm_runais_fetch_state", "mfm_runais_store_state",
             "mfm_hosttwin_runais_state_check"]
RATIOS = [(4, 5, 41), (1, 1, 4)]   # interpolate, decimate, taps
WINDOWS = [7, 64, 500]
N48 = 24000                        # samples per channel at 48 kHz: 30 000 at 60 kHz in front of the 4/5 resampler
NCH = 4
SPARSE = (1, 3)                    # the channels that carry known packets with silence between them
EVENT_FIELDS = ("channel", "fcs_valid", "nr_bytes", "run", "stretch_window", "sample", "start_sample", "bytes")


# ---- the checker --------------------------------------------------------------------------------------------

def rs_taps(pkg, ora, ratio):
    if ratio[2] == 41:
        return ora.quantize_taps(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4)   # as test_ais
    return ora.quantize_taps([0.1, 0.4, 0.4, 0.1])


class Checker:
    """what the stage must return for the gate calls of one stream, from the oracle; and the figures the guards read"""

    def __init__(self, pkg, ora, taps, I, D, W):
        self.pkg = pkg
        self.rs = tr.Checker(pkg, ora, taps, I, D, False, W)
        self.chan = {}      # channel -> [demodulator, key of the stretch, sample of the stretch's last event]
        self.by = {}        # (channel, first window) -> events
        self.pcm = {}       # (channel, first window) -> resampled pieces
        self.bounds = {}    # (channel, first window) -> first_out of every run but the first: the handovers
        self.cross = self.close = 0

    def call(self, gate_runs, gate_payload):
        runs, payload = self.rs.call(gate_runs, gate_payload)
        parts = []
        for i, r in enumerate(runs):
            c, fo, n = int(r["channel"]), int(r["first_out"]), int(r["nr_out"])
            if int(r["flags"]) & 1:
                key = (c, int(r["first_window"]))
                self.chan[c] = [ais_ref.Demod(c), key, None]
                self.by[key], self.pcm[key], self.bounds[key] = [], [], []
            else:
                self.bounds[self.chan[c][1]].append(fo)
            st = self.chan[c]
            y = payload[int(r["out_offset"]):int(r["out_offset"]) + n]
            e = st[0].feed(y)
            ev = np.zeros(len(e), self.pkg.binding.RUNAIS_EVENT_DTYPE)
            for f in ("channel", "fcs_valid", "nr_bytes", "sample", "start_sample", "bytes"):
                ev[f] = e[f]
            ev["run"], ev["stretch_window"] = i, st[1][1]
            assert ((ev["sample"] >= fo) & (ev["sample"] < fo + n)).all()
            for x in ev:
                self.cross += int(x["start_sample"]) < fo
                self.close += st[2] is not None and int(x["start_sample"]) - st[2] <= 165
                st[2] = int(x["sample"])
            self.by[st[1]].append(ev)
            self.pcm[st[1]].append(y)
            parts.append(ev)
        ev = np.concatenate(parts) if parts else np.zeros(0, self.pkg.binding.RUNAIS_EVENT_DTYPE)
        return (runs, payload), ev

    def stretches(self):
        """{(channel, first window): events without `run`}; each stretch once more through a fresh demodulator in one piece"""
        out = {}
        for key, evs in self.by.items():
            ev = np.concatenate(evs) if evs else np.zeros(0, self.pkg.binding.RUNAIS_EVENT_DTYPE)
            whole = ais_ref.demod(np.concatenate(self.pcm[key]), key[0])
            assert len(whole) == len(ev), key
            for f in ("channel", "fcs_valid", "nr_bytes", "sample", "start_sample", "bytes"):
                assert np.array_equal(whole[f], ev[f]), (key, f)
            ev = ev.copy()
            ev["run"] = 0
            out[key] = ev
        return out


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in EVENT_FIELDS if len(want) else ():
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, f"{what}: event field {f} differs at {bad[:5].tolist()}: {got[f][bad[0]]} != {want[f][bad[0]]}"


# ---- scenes ---------------------------------------------------------------------------------------------------

_SCENE = {}


def scene(pkg, ratio):
    """four channels at 48 kHz (busy with rejects and back-to-back frames; known packets with near silence between them; a
    frame without end flag, then frames back to back; known packets again), the input in front of the resampler and, for the
    SPARSE channels, where each packet lies in it.  Made once per ratio and left unchanged"""
    if ratio in _SCENE:
        return _SCENE[ratio]
    sy = pkg.synth
    I, D, _ = ratio
    rng = np.random.RandomState(77)
    pl = ta._payloads(sy)
    chans, packets = [], {}
    for c in range(NCH):
        if c == 0:
            x = ta._busy(sy, 61, N48)
        elif c == 2:
            parts = [sy.ais_pcm(sy.ais_frame_bits(bytes(rng.randint(0, 256, 200).astype(np.uint8)), end_flag=False), lead=77, noise=100,
                                trail=300, seed=4),
                     sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(p) for p in (pl[0], pl[1], pl[2], pl[0], pl[0])]), noise=150,
                                phase=3, trail=N48, seed=5)]
            x = np.concatenate(parts)[:N48]
        else:
            x = (rng.randn(N48) * 40).round().astype(np.int16)
            packets[c] = []
            for k in range(6):
                bits = sy.ais_bits([sy.ais_frame_bits(pl[(k + c) % 3])], lead_bits=5, trail_bits=4)   # the bits in front of the preamble must not let it match two bits early
                p = sy.ais_pcm(bits, noise=200, phase=int(rng.randint(0, 5)), seed=10 * c + k)
                a = 1200 + 3700 * k + int(rng.randint(0, 300))
                x[a:a + p.size] = p
                packets[c].append((a * D // I, (a + p.size) * D // I + 1))
        chans.append(x)
    x48 = np.stack(chans)
    n_in = N48 * D // I
    stream = np.stack([np.repeat(x, D)[::I][:n_in] for x in x48])   # for 4/5: np.repeat(x, 5)[::4], as test_ais
    _SCENE[ratio] = dict(stream=np.ascontiguousarray(stream), packets=packets, n_in=n_in)
    return _SCENE[ratio]


def make_mask(kind, sc, W, rng):
    """raw squelch verdicts [C][nw]"""
    nw = sc["n_in"] // W
    m = np.zeros((NCH, nw), bool)
    mg = 150 // W + 1   # windows of margin: the resampler's phase length, the preamble, the end flag
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
    for c in SPARSE:
        for k, (a, b) in enumerate(sc["packets"][c]):
            ka, kb, mid = a // W - mg, b // W + 1 + mg, (a + b) // (2 * W)
            if kind == "cut" and k % 3 == 0:
                kb = mid          # closes in the middle of the packet
            if kind == "cut" and k % 3 == 1:
                ka = mid          # opens in the middle of the packet
            m[c, max(ka, 0):kb] = True
    if kind == "cut":             # the other channels: seeded blocks, whatever they hit
        for c in set(range(NCH)) - set(SPARSE):
            k = 0
            while k < nw:
                ln = int(rng.randint(300, 3000)) // W + 1
                m[c, k:k + ln] = True
                k += ln + int(rng.randint(100, 1500)) // W + 1
    return m


def make_cuts(rng, n, W, anchors):
    """piece lengths that add up to n: an nr_in = 0 call first, a call boundary at every anchor and one window later, a row of
    one-window calls behind the first anchors, an nr_in = 0 call in the middle, otherwise pieces of up to 7000 samples"""
    marks = {n}
    for i, a in enumerate(anchors):
        marks |= {min(a, n), min(a + W, n)}
        if i < 3:
            marks |= {min(a + j * W, n) for j in range(2, 14)}
    pos = 0
    while pos < n:
        pos += int(rng.randint(1, 7001))
        marks.add(min(pos, n))
    marks = sorted(marks - {0})
    out = [0] + [b - a for a, b in zip([0] + marks, marks)]
    out.insert(len(out) // 2, 0)
    assert sum(out) == n
    return out


def anchors_of(sc, ratio, W):
    """input positions near which something happens to a SPARSE packet: its preamble match (about 32 bit periods in), its
    middle, 80 outputs behind its end"""
    out = []
    for c in SPARSE:
        for a, b in sc["packets"][c][:3]:
            out += [a + 165 * ratio[1] // ratio[0], (a + b) // 2, b + 80]
    return sorted(out)


KINDS = ["open", "bursts", "cut", "short"]


def run_scenes(pkg, ora, W, ratio, make_call, seed):
    """every mask (short: W = 7 only), P = 0 and 2 with the flush, each stream in the seeded cut and as one call; returns nothing,
    asserts the guards on the oracle's figures before any comparison"""
    I, D, _ = ratio
    sc = scene(pkg, ratio)
    taps = rs_taps(pkg, ora, ratio)
    stream, n = sc["stream"], sc["n_in"]
    jobs, tally = [], dict(valid=0, invalid=0, full=0, cross=0, close=0, inside=0, behind=0, match=0)
    count = {}
    for kind in KINDS:
        if kind == "short" and W != 7:
            continue
        for P in (0, 2):
            rng = np.random.RandomState(seed + 10 * KINDS.index(kind) + P)
            mask = make_mask(kind, sc, W, rng)
            for single in (False, True):
                cuts = [n] if single else make_cuts(rng, n, W, anchors_of(sc, ratio, W))
                calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
                chk = Checker(pkg, ora, taps, I, D, W)
                want = [chk.call(gr, gp) for gr, gp in calls]
                by = chk.stretches()
                ev = np.concatenate(list(by.values())) if by else np.zeros(0, pkg.binding.RUNAIS_EVENT_DTYPE)
                tally["valid"] += int((ev["fcs_valid"] == 1).sum())
                tally["invalid"] += int((ev["fcs_valid"] == 0).sum())
                tally["full"] += int((ev["nr_bytes"] == 160).sum())
                tally["cross"] += chk.cross
                tally["close"] += chk.close
                count[(kind, P, single)] = len(ev)
                emitted = tr.emitted_of(mask, P)[:, :n // W]
                assert sorted(by) == tr.stretches_of_mask(emitted)
                if kind == "open":   # one stretch from window 0: the row stage's numbering
                    plain = ais_ref.demod_channels(np.stack([ora.Resampler(taps, I, D).feed(x[:n // W * W]) for x in stream]))
                    assert (ev["stretch_window"] == 0).all() and len(ev) == len(plain)
                    ev = ev[np.argsort(ev["channel"], kind="stable")]
                    for f in ais_ref.EVENT_DTYPE.names:
                        if f != "reserved":
                            assert np.array_equal(ev[f], plain[f]), f
                if kind == "bursts":   # every packet whole: exactly one valid event per synthesized packet, nothing else
                    assert len(ev) == sum(len(sc["packets"][c]) for c in SPARSE) and (ev["fcs_valid"] == 1).all()
                    assert sorted(set(ev["channel"].tolist())) == list(SPARSE)
                if not single:   # where the handovers lie
                    hand = [(int(e["start_sample"]), int(e["sample"]), chk.bounds[k]) for k, v in by.items() for e in v]
                    tally["inside"] += any(any(s0 < b <= s1 for b in bs) for s0, s1, bs in hand)            # inside a packet
                    tally["behind"] += any(any(s1 < b <= s1 + 165 for b in bs) for s0, s1, bs in hand)      # just behind its end
                    tally["match"] += any(any(abs(b - s0) <= 3 for b in bs) for s0, s1, bs in hand)         # on the match
                jobs.append((kind, P, single, cuts, mask, calls, want, by))
    # the guards, on the oracle's result alone
    assert tally["valid"] >= 10 and tally["invalid"] >= 1 and tally["full"] >= 1 and tally["cross"] >= 1 and tally["close"] >= 1, tally
    assert tally["inside"] >= 1 and tally["behind"] >= 1 and (tally["match"] >= 1 or W != 7), tally   # W = 7 can place a cut to the sample
    for P in (0, 2):
        assert count[("cut", P, True)] < count[("open", P, True)]   # a packet really was dropped at a stretch end
        for kind in KINDS:
            if (kind, P, True) in count:
                assert count[(kind, P, True)] == count[(kind, P, False)]
    # the code under test
    by_single = {}
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

def test_header_declares_and_library_exports_the_runais_names(pkg):
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
    assert b.RUNAIS_EVENT_DTYPE.itemsize == 200 and C.sizeof(b.RunaisEvent) == 200 and C.sizeof(b.RunaisConfig) == 28
    assert b.RUNAIS_STATE_DTYPE.itemsize == 264
    assert pkg.RUNAIS_EVENT_DTYPE is b.RUNAIS_EVENT_DTYPE and pkg.RunAis is b.RunAis and pkg.hosttwin_runais_call is b.hosttwin_runais_call
    m = re.search(r"struct mfm_runais_event \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+)(?:\[160\])?;", m.group(1)) == [
        ("uint32_t", "channel"), ("uint32_t", "fcs_valid"), ("uint32_t", "nr_bytes"), ("uint32_t", "run"), ("uint64_t", "stretch_window"),
        ("uint64_t", "sample"), ("uint64_t", "start_sample"), ("uint8_t", "bytes")]
    assert list(b.RUNAIS_EVENT_DTYPE.names) == [n for n, _ in b.RunaisEvent._fields_]
    for n, _ in b.RunaisEvent._fields_:
        assert b.RUNAIS_EVENT_DTYPE.fields[n][1] == getattr(b.RunaisEvent, n).offset, n
    m = re.search(r"struct mfm_runais_config \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == [n for n, _ in b.RunaisConfig._fields_]
    m = re.search(r"struct mfm_runais_state \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+)(?:\[\d+\])?;", m.group(1))] == list(b.RUNAIS_STATE_DTYPE.names)
    for name in ("OVER_RUNS", "OVER_EVENTS", "IN_RUNRS", "IN_OUT_OF_STEP", "IN_BAD_RUNS"):
        m = re.search(r"#define\s+MFM_RUNAIS_%s\s+(\d+)u\b" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNAIS_" + name)
    # mfm_runrs_get_capacity wants an object
    assert lib.mfm_runrs_get_capacity(None, None, None) == b.MFM_E_INVAL


def _twin_call(pkg):
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        state = b.hosttwin_runais_state(nch)

        def call(i, gr, gp, rs_want):
            return b.hosttwin_runais_call(state, *rs_want)

        return call, lambda: None

    return make_call


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_hosttwin_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """csrc/mfm_runais.h and the twin's sample-by-sample demodulator on the scenes of the GPU tests"""
    run_scenes(pkg, ora, W, ratio, _twin_call(pkg), 7 * W + ratio[0])


def _pieces(pkg, ora):
    """one stretch per channel cut into runs by hand, at any sample: channel 0 (a SPARSE channel of the 1/1 scene, resampled by
    the oracle) and channel 1 (the busy one).  Returns the calls [(runs, payload)] and the oracle's events per call.  Cuts
    lie on a preamble match, one sample behind it, on a packet end, one behind it, inside packets, as runs of one sample and
    as runs without output"""
    b = pkg.binding
    ratio = RATIOS[1]
    sc = scene(pkg, ratio)
    taps = rs_taps(pkg, ora, ratio)
    pcm = [ora.Resampler(taps, 1, 1).feed(sc["stream"][c]) for c in (SPARSE[0], 0)]
    whole = [ais_ref.demod(x, c) for c, x in enumerate(pcm)]
    assert len(whole[0]) == 6 and len(whole[1]) >= 5
    e0, e1 = whole[0][0], whole[0][1]
    marks = [[int(e0["start_sample"]), int(e0["start_sample"]) + 1, int(e0["start_sample"]) + 4, int(e0["sample"]), int(e0["sample"]) + 1,
              int(e0["sample"]) + 100, int(e1["start_sample"]) - 1, (int(e1["start_sample"]) + int(e1["sample"])) // 2,
              int(e1["sample"]) - 1, int(e1["sample"]) + 165, 9000, 9001, 9002, 9003, 9003, 9100, 9130, 9131],
             [5, 5, 60, 100, 255, 256, 257, 300, 2047, 2048, 2304, 4097, int(whole[1][2]["sample"]), int(whole[1][3]["start_sample"])]]
    cuts = [sorted(m) + [x.size] for m, x in zip(marks, pcm)]
    calls, want = [], []
    dem = [ais_ref.Demod(0), ais_ref.Demod(1)]
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
            e = dem[c].feed(y)
            ev = np.zeros(len(e), b.RUNAIS_EVENT_DTYPE)
            for f in ("channel", "fcs_valid", "nr_bytes", "sample", "start_sample", "bytes"):
                ev[f] = e[f]
            ev["run"], ev["stretch_window"] = len(runs) - 1, 7 + c
            evs.append(ev)
            at[c] = end
        calls.append((np.array(runs, b.RUNRS_RUN_DTYPE), np.concatenate(parts) if parts else np.zeros(0, np.int16)))
        want.append(np.concatenate(evs) if evs else np.zeros(0, b.RUNAIS_EVENT_DTYPE))
        i += 1
    assert at[0] == pcm[0].size and at[1] == pcm[1].size and sum(len(w) for w in want) >= 9
    assert any(len(r) and (r["nr_out"] == 0).any() for r, _ in calls) and any(len(r) and (r["nr_out"] == 1).any() for r, _ in calls)
    return calls, want


def test_hosttwin_handovers_at_any_sample(pkg, ora):
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    state = b.hosttwin_runais_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(b.hosttwin_runais_call(state, runs, payload), w, f"call {i}")


def _refusal_case(pkg, ora):
    """two calls of the hand-cut stretches that both carry runs of both channels, and what is wrong with the second in six ways"""
    b = pkg.binding
    calls, want = _pieces(pkg, ora)
    i = next(i for i in range(3, len(calls)) if len(calls[i][0]) == 2 and len(want[i]) and calls[i][0]["nr_out"].min() > 0)
    runs, payload = calls[i]
    bound = int((runs["nr_out"] // 160 + 1).sum())

    def changed(field, k, value, flags=None):
        r = runs.copy()
        r[field][k] = value
        if flags is not None:
            r["flags"][k] = flags
        return r

    cases = [
        (dict(totals=[2, payload.size, 1, 0]), "overflow or gate error", b.MFM_RUNAIS_IN_RUNRS << 8),
        (dict(totals=[2, payload.size, 0, 2]), "overflow or gate error", b.MFM_RUNAIS_IN_RUNRS << 8),
        (dict(runs=changed("first_out", 0, int(runs["first_out"][0]) + 1)), "out of step", b.MFM_RUNAIS_IN_OUT_OF_STEP << 8),
        (dict(runs=changed("channel", 0, 1)), "out of step", b.MFM_RUNAIS_IN_OUT_OF_STEP << 8),   # channel 1's second run continues
        (dict(runs=changed("channel", 1, 2)), "does not exist", b.MFM_RUNAIS_IN_BAD_RUNS << 8),
        (dict(runs=changed("flags", 0, 1)), "does not exist", b.MFM_RUNAIS_IN_BAD_RUNS << 8),   # begins with first_out != 0
        (dict(runs=runs[::-1].copy()), "does not exist", b.MFM_RUNAIS_IN_BAD_RUNS << 8),   # channels descend
        (dict(runs=changed("out_offset", 1, payload.size + 1)), "does not exist", b.MFM_RUNAIS_IN_BAD_RUNS << 8),
        (dict(runs=changed("nr_out", 1, payload.size)), "does not exist", b.MFM_RUNAIS_IN_BAD_RUNS << 8),
    ]
    capacity = [
        (dict(max_out_samples=payload.size - 1), "max_out_samples", b.MFM_RUNAIS_IN_BAD_RUNS << 8),
        (dict(max_runs=1), "max_runs", b.MFM_RUNAIS_OVER_RUNS),
        (dict(max_events=bound - 1), "event bound", b.MFM_RUNAIS_OVER_EVENTS),
    ]
    return calls, want, i, cases, capacity, bound


def test_hosttwin_refuses_and_leaves_its_state(pkg, ora):
    b = pkg.binding
    calls, want, at, cases, capacity, bound = _refusal_case(pkg, ora)
    cases = cases + capacity
    state = b.hosttwin_runais_state(2)
    for i in range(at):
        same(b.hosttwin_runais_call(state, *calls[i]), want[i], f"call {i}")
    s0 = state.copy()
    assert s0["has_stretch"].all() and (s0["outs"] > 0).all()
    runs, payload = calls[at]
    for change, message, flags in cases:
        kw = dict(runs=runs, payload=payload)
        kw.update(change)
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runais_call(state, kw.pop("runs"), kw.pop("payload"), **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value))
        assert ei.value.needed == 0 and np.array_equal(state, s0)
    with pytest.raises(pkg.MfmError) as ei:   # the caller's array is too small: nothing moves either
        b.hosttwin_runais_call(state, runs, payload, max_out=len(want[at]) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(want[at]) and np.array_equal(state, s0)
    same(b.hosttwin_runais_call(state, runs, payload, max_events=bound), want[at], "the same call, right")   # the bound itself fits
    for i in range(at + 1, len(calls)):
        same(b.hosttwin_runais_call(state, *calls[i]), want[i], f"call {i}")


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
    """every refusal of mfm_runais_create is decided before a device is looked for"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_out_samples=10000)
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunAis(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_runais_to_ais_events_arithmetic(pkg):
    b = pkg.binding
    ev = np.zeros(3, b.RUNAIS_EVENT_DTYPE)
    ev["channel"], ev["fcs_valid"], ev["nr_bytes"], ev["run"] = [2, 0, 5], [1, 0, 1], [23, 160, 4], [9, 8, 7]
    ev["stretch_window"], ev["sample"], ev["start_sample"] = [0, 3, (1 << 40) + 1], [1500, 99, 7], [200, 0, 2]
    ev["bytes"] = np.arange(3 * 160).reshape(3, 160) % 251
    out = b.runais_to_ais_events(ev, 4, 5, 7)
    assert out.dtype == b.AIS_EVENT_DTYPE and not out["reserved"].any()
    base = [0, 3 * 7 * 4 // 5, ((1 << 40) + 1) * 7 * 4 // 5]
    assert out["sample"].tolist() == [base[0] + 1500, base[1] + 99, base[2] + 7]
    assert out["start_sample"].tolist() == [base[0] + 200, base[1], base[2] + 2]
    for f in ("channel", "fcs_valid", "nr_bytes", "bytes"):
        assert np.array_equal(out[f], ev[f])
    assert b.runais_to_ais_events(ev[:0], 1, 1, 64).shape == (0,)


def test_runais_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_runais.o (tools/kernel_regs.py): the six kernels, no private segment, no spilled
    register, at most 128 VGPRs"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runais.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_runais.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"ra_{k}_kernel" for k in ("plan", "slice", "walk", "evscan", "compact", "state")), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gpu_call(pkg):
    """a real Gate (process_host, flush_device) -> RunResampler -> RunAis on the device; the resampler's result is checked on the way"""
    def make_call(nch, W, P, cuts, stream, mask, taps, I, D):
        cap = max(max(cuts), 1)
        gate = pkg.Gate(nch, cap, W, preroll_windows=P)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P)
        ra = pkg.RunAis.behind(rr)
        pos = [0]

        def call(i, gr, gp, rs_want):
            if i < len(cuts):
                m = cuts[i]
                gate.process_host(stream[:, pos[0]:pos[0] + m], tg.records_of(pkg, mask, pos[0] // W, (pos[0] + m) // W))
                pos[0] += m
            else:
                gate.flush_device()
            rr.process_device(*gate.device_view())
            ra.process_device(*rr.device_view())
            got = ra.fetch()
            tr.same(rr.fetch(), rs_want, f"the resampler's call {i}")
            return got

        def done():
            ra.close()
            rr.close()
            gate.close()

        return call, done

    return make_call


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """four channels; all open (equal to the row stage's numbering), windows around each packet, a mask that closes and opens
    inside packets, at W = 7 stretches of one or two windows; P = 0 and 2 with the flush fed through; cut into calls at
    packets' preambles, middles and ends, as one-window and nr_in = 0 calls, and as one call, with identical events per stretch"""
    run_scenes(pkg, ora, W, ratio, _gpu_call(pkg), 7 * W + ratio[0])


def _fed(pkg, torch, ra, runs, payload, totals=None):
    """one call from uploaded arrays: a burst resampler's result as it would stand in its device view"""
    t = np.array([len(runs), payload.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
    ra.process_device(*(k.data_ptr() for k in keep))
    try:
        return ra.fetch()
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_handovers_at_any_sample(pkg, ora):
    import torch
    calls, want = _pieces(pkg, ora)
    ra = pkg.RunAis(2, 4, max(p.size for _, p in calls) + 1)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        same(_fed(pkg, torch, ra, runs, payload), w, f"call {i}")
    ra.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state(pkg, ora):
    """the resampler's flags handed through, out of step, run lists that are not a resampler's, max_runs, the event bound
    against max_events: each time nothing comes out and the state stays, so the same call fed correctly is right"""
    import torch
    b = pkg.binding
    calls, want, at, cases, _, _ = _refusal_case(pkg, ora)
    runs, payload = calls[at]
    cap = max(p.size for _, p in calls) + 1
    ra = pkg.RunAis(2, 4, cap)
    for i in range(at):
        same(_fed(pkg, torch, ra, *calls[i]), want[i], f"call {i}")
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, ra, change.get("runs", runs), payload, totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == 0 and not ei.value.buffer.view(np.uint8).any()
    got = _fed(pkg, torch, ra, runs, payload)
    same(got, want[at], "the same call, right, after the refused ones")
    with pytest.raises(pkg.MfmError) as ei:
        ra.fetch(max_events=len(got) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(got) and not ei.value.buffer.view(np.uint8).any()
    same(ra.fetch(), want[at], "fetched again")
    for i in range(at + 1, len(calls)):
        same(_fed(pkg, torch, ra, *calls[i]), want[i], f"call {i}")
    ra.close()
    # what an object is too small for: the first call, whose runs begin their stretches, against max_runs, max_out_samples and
    # max_events; the event bound itself fits
    runs, payload = calls[0]
    bound = int((runs["nr_out"] // 160 + 1).sum())
    assert len(runs) == 2 and (runs["flags"] == 1).all()
    for kw, message in ((dict(max_runs=1), "max_runs"), (dict(max_out_samples=payload.size - 1), "max_out_samples"),
                        (dict(max_events=bound - 1), "event bound")):
        args = dict(max_runs=4, max_out_samples=cap, max_events=0)
        args.update(kw)
        ra = pkg.RunAis(2, **args)
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, ra, runs, payload)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (kw, str(ei.value))
        ra.close()
    ra = pkg.RunAis(2, 2, payload.size, max_events=bound)
    for i in range(3):
        if len(calls[i][0]) <= 2 and calls[i][1].size <= payload.size and int((calls[i][0]["nr_out"] // 160 + 1).sum()) <= bound:
            same(_fed(pkg, torch, ra, *calls[i]), want[i], f"call {i} on an object made for it")
        else:
            break
    ra.close()


@pytest.mark.gpu
def test_gpu_many_runs_and_many_workgroups(pkg, ora):
    """256 channels, W = 64, 1/1: an alternating mask on most channels (7500 runs in one call: the scans' threads take eight
    runs each, every kernel runs many workgroups), every 16th channel open for the whole call with frames on it (a segment of
    several slicer workgroups), cut into two calls.  Every run of an alternating channel is a stretch of its own"""
    import torch
    W, I, D, nch, nw = 64, 1, 1, 256, 250
    ratio = RATIOS[1]
    taps = rs_taps(pkg, ora, ratio)
    rng = np.random.RandomState(12)
    busy = [ta._busy(pkg.synth, 200 + k, nw * W) for k in range(4)]
    stream = rng.randint(-3000, 3001, size=(nch, nw * W)).astype(np.int16)
    mask = (np.arange(nw)[None, :] + np.arange(nch)[:, None]) % 4 == 0
    for c in range(0, nch, 16):
        stream[c] = busy[(c // 16) % 4]
        mask[c] = True
    cuts = [150 * W, 100 * W]
    calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
    assert len(calls[0][0]) > 7500
    chk = Checker(pkg, ora, taps, I, D, W)
    want = [chk.call(gr, gp) for gr, gp in calls]
    assert sum(len(e) for _, e in want) >= 50 and chk.cross >= 1
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=max(cuts))
    ra = pkg.RunAis.behind(rr)
    assert rr.capacity() == (nch * ((max(cuts) // W + 2) // 2), (nch * (max(cuts) // W + 1) * W + rr.capacity()[0] * 4) * I // D + rr.capacity()[0])
    for i, ((gr, gp), (rs_want, ev_want)) in enumerate(zip(calls, want)):
        t = np.array([len(gr), gp.size, 0, 0], np.uint64)
        keep = (tr._up(torch, gr), tr._up(torch, gp), tr._up(torch, t))
        rr.process_device(*(k.data_ptr() for k in keep))
        ra.process_device(*rr.device_view())
        same(ra.fetch(), ev_want, f"call {i}")
        del keep
    ra.close()
    rr.close()


CHAIN = dict(fs=2400000, decim=50, offsets=(-150000, 100000), W=100, P=1, blk=50021)
_CHAIN = {}


def _chain(pkg, ora):
    """two channels of FM AIS bursts (three packets each, noise between them) at 2.4 MS/s, D = 50 -> 48 kHz; the oracle's PCM,
    the squelch on the PCM energy (a burst lowers it) and the resampler taps as the scan tool quantises them"""
    if _CHAIN:
        return _CHAIN["it"]
    sy, s = pkg.synth, CHAIN
    fs, decim, W = s["fs"], s["decim"], s["W"]
    pl = ta._payloads(sy)
    taps = sy.design_lpf(128, 12500.0, float(fs))
    gap = 40 * 250
    parts = []
    for k, o in enumerate(s["offsets"]):
        acc = []
        for j in range(3):
            bits = sy.ais_bits([sy.ais_frame_bits(pl[(k + j) % 3])], lead_bits=6, trail_bits=6)
            acc.append(sy.synth_iq(gap + 3000 * (k + j), fs, [], seed=10 * k + j, noise=300).astype(np.int32))
            acc.append(sy.ais_fm_iq(bits, fs, o, amplitude=6000.0, noise=300.0, seed=3 * k + j).astype(np.int32))
        acc.append(sy.synth_iq(gap, fs, [], seed=50 + k, noise=300).astype(np.int32))
        parts.append(np.concatenate(acc))
    n = min(p.shape[0] for p in parts)
    iq = np.clip(sum(p[:n] for p in parts), -32768, 32767).astype(np.int16)
    offs, gains = np.array(s["offsets"], np.float64), np.ones(2)
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm = ora.run_channels(iq, cre, cim, incr, decim)[0]
    e = tl.restate(pkg, pcm, W, tl.PCM)["energy"].astype(np.float64)
    thr = int(np.sqrt(e.min() * e.max()))
    mask = tl.restate(pkg, pcm, W, tl.PCM, sense=tl.BELOW, open_thr=thr, close_thr=thr, hang=1)["open"].astype(bool)
    lpf = [0.1, 0.4, 0.4, 0.1]
    rtaps = np.array([int(x * 16384.0) for x in lpf], np.int16)
    # the scene is what it is meant to be: every channel opens and closes three times or more, and the oracle finds the packets
    emitted = tgp.dilate(mask, s["P"])
    assert all(sum(1 for k in tr.stretches_of_mask(emitted) if k[0] == c) >= 3 for c in range(2)) and not emitted.all(axis=1).any()
    _CHAIN["it"] = dict(iq=iq, pcm=pcm, taps=taps, thr=thr, mask=mask, lpf=lpf, rtaps=rtaps, offs=offs)
    return _CHAIN["it"]


@pytest.mark.gpu
def test_gpu_engine_level_gate_runrs_runais_on_device_equals_the_chain_through_the_oracle(pkg, ora):
    """engine -> level (PCM form) -> gate with P = 1 -> burst resampler 1/1 -> burst AIS stage, all queued on the engine's stream
    with no fetch between the stages; every call and the flush against the oracle's PCM through the restated gate, the
    oracle's resampler and a fresh demodulator per stretch"""
    b = pkg.binding
    sc, s = _chain(pkg, ora), CHAIN
    fs, decim, W, P, blk = s["fs"], s["decim"], s["W"], s["P"], s["blk"]
    pcm, mask, iq = sc["pcm"], sc["mask"], sc["iq"]
    eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY)
    for o in sc["offs"]:
        eng.add_channel(int(o), sc["taps"], 1.0)
    eng.commit()
    cap = blk // decim + 8
    lv = pkg.Level(2, cap, W, form=b.MFM_LEVEL_PCM, sense=b.MFM_LEVEL_OPEN_BELOW, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=1)
    gate = pkg.Gate(2, cap, W, elems_per_sample=1, preroll_windows=P)
    rr = pkg.RunResampler(2, sc["rtaps"], 1, 1, W, max_in_samples=cap, preroll_windows=P)
    ra = pkg.RunAis.behind(rr)
    chk = Checker(pkg, ora, sc["rtaps"], 1, 1, W)
    pos, valid = 0, 0
    for at in list(range(0, iq.shape[0], blk)) + [None]:
        if at is not None:
            assert eng.push(iq[at:at + blk]) == 0
            d_pcm, stride, nout, _ = eng.last_output_device()
            lv.process_device(d_pcm, stride, nout, stream=eng.stream)
            d_rec, rec_stride, nw, _ = lv.device_view()
            gate.process_device(d_pcm, stride, nout, d_rec, rec_stride, nw, stream=eng.stream)
            want = chk.call(*tgp.restate_pre(pkg, pcm, mask, W, 1, P, pos, nout))
            pos += nout
        else:
            gate.flush_device(stream=eng.stream)
            want = chk.call(*tgp.restate_pre(pkg, pcm, mask, W, 1, P, pos, 0, flush=True))
        rr.process_device(*gate.device_view(), stream=eng.stream)
        ra.process_device(*rr.device_view(), stream=eng.stream)
        same(ra.fetch(), want[1], f"block at {at}")
        valid += int((want[1]["fcs_valid"] == 1).sum())
    assert pos == pcm.shape[1] and valid >= 5 and chk.cross >= 1
    for o in (ra, rr, gate, lv, eng):
        o.close()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_ais_writes_the_events_of_the_oracle(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-out DIR --gate-preroll 1 --gate-resample 1/1 --resample-taps FILE --gate-ais on the chain
    scene: ais.jsonl holds the oracle's events, stretch by stretch"""
    sc, s = _chain(pkg, ora), CHAIN
    fs, decim, W, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 162000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
           str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(sc["thr"]),
           "--hang", "1", "--block", str(s["blk"]), "--gate-out", str(tmp_path / "gated"), "--gate-preroll", str(P),
           "--gate-resample", "1/1", "--resample-taps", str(tmp_path / "filter.json"), "--gate-ais"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    chk = Checker(pkg, ora, sc["rtaps"], 1, 1, W)
    n = sc["pcm"].shape[1]
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n))
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True))
    want = sorted((int(e["channel"]), k[1] * W, int(e["sample"]), int(e["start_sample"]), int(e["nr_bytes"]), int(e["fcs_valid"]),
                   bytes(e["bytes"][:int(e["nr_bytes"])]).hex()) for k, v in chk.stretches().items() for e in v)
    assert len(want) >= 5
    lines = [json.loads(ln) for ln in (tmp_path / "gated" / "ais.jsonl").read_text().splitlines()]
    got = sorted((ln["channel"], ln["first_sample"], ln["sample"], ln["start_sample"], ln["nr_bytes"], ln["fcs_valid"], ln["bytes"]) for ln in lines)
    assert got == want
    r = subprocess.run(cmd[:-5] + ["--gate-ais"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-ais needs --gate-resample" in r.stderr
