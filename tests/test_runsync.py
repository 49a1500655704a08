"""The burst sync stage (mfm_runsync_*, csrc/mfm_runsync.hip): the burst Mueller-Muller stage's decisions become one bit each, and
wherever the last 32 bits of a stretch are a sync word of the table, or nearly one, an event.

The expected result is never the code under test: a plain restatement of pager/test/test_mueller_muller.c:130-136 (restate
below), extended to several words and the complement, run per stretch over the concatenated decisions.  Every comparison is an
equality of every field of every run record, every bit word and every event."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_runmm as trm
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runsync_create", "mfm_runsync_destroy", "mfm_runsync_process_device", "mfm_runsync_fetch", "mfm_runsync_device_view",
             "mfm_runsync_get_capacity", "mfm_runsync_fetch_state", "mfm_runsync_store_state", "mfm_hosttwin_runsync_call",
             "mfm_hosttwin_runsync_state_check", "mfm_runmm_get_capacity"]
SYNC = 0x7CD215D8        # POCSAG's (test_mueller_muller.c:134)
OTHER = 0xA6C6AAAA       # a second word, as FLEX's sync words stand beside it
NOT_POS, POS = 0, 1
M32 = 0xFFFFFFFF
SEG = 1024               # decisions of a run one wave takes (MFM_RUNSYNC_SEGMENT, csrc/mfm_runsync.h)


# ---- the yardstick ------------------------------------------------------------------------------------------------

def bit_of(d, rule):
    return (0 if d > 0 else 1) if rule == NOT_POS else (1 if d > 0 else 0)


def restate(decisions, words, maxd=3, rule=NOT_POS, either=False):
    """test_mueller_muller.c:130-136 over one stretch: [(n, word index, distance, inverted, register)], and the register after
    every decision"""
    shr, out, regs = 0, [], []
    for n, d in enumerate(decisions):
        shr = ((shr << 1) | bit_of(int(d), rule)) & M32
        regs.append(shr)
        for k, w in enumerate(words):
            dist = bin(w ^ shr).count("1")
            if dist <= maxd:
                out.append((n, k, dist, 0, shr))
                break
            if either and bin((~w & M32) ^ shr).count("1") <= maxd:
                out.append((n, k, bin((~w & M32) ^ shr).count("1"), 1, shr))
                break
    return out, regs


def plant(x, end, word, rule=NOT_POS, lowest=32):
    """the `lowest` low bits of `word` into the decisions so that its last bit is decision `end`"""
    for i in range(lowest):
        bit = (word >> i) & 1
        mag = abs(int(x[end - i])) or 5
        x[end - i] = -mag if (bit == 1) == (rule == NOT_POS) else mag


def make_runs(pkg, rows):
    """RUNMM_RUN_DTYPE from (channel, nr_dec, begins, first_dec, first_window, dec_offset)"""
    runs = np.zeros(len(rows), pkg.binding.RUNMM_RUN_DTYPE)
    for i, (c, n, begins, fd, fw, off) in enumerate(rows):
        runs[i] = (fw, off, fd, c, n, 1 if begins else 0, 0)
    return runs


def pack(bits):
    """one bit per decision, bit j % 32 of word j / 32, the tail 0"""
    w = np.zeros((len(bits) + 31) // 32, np.uint32)
    for j, b in enumerate(bits):
        if b:
            w[j // 32] |= np.uint32(1 << (j % 32))
    return w


class Want:
    """what the stage must return for the burst Mueller-Muller calls of one stream, from the restatement: lines[c] = [(first
    window, decisions)] are channel c's stretches one behind the other, known whole in advance"""

    def __init__(self, pkg, lines, words, maxd=3, rule=NOT_POS, either=False):
        self.pkg, self.rule = pkg, rule
        self.st = {}
        for c, line in enumerate(lines):
            for fw, x in line:
                ev, regs = restate(x, words, maxd, rule, either)
                self.st[(c, fw)] = (x, ev, regs)
        self.state = pkg.binding.hosttwin_runsync_state(len(lines))
        self.cur = {}

    def call(self, runs, decisions):
        b = self.pkg.binding
        out = np.zeros(len(runs), b.RUNSYNC_RUN_DTYPE)
        words, evs, woff = [], [], 0
        for i, r in enumerate(runs):
            c, n, fd, off = int(r["channel"]), int(r["nr_dec"]), int(r["first_dec"]), int(r["dec_offset"])
            if int(r["flags"]) & 1:
                self.cur[c] = (c, int(r["first_window"]))
            key = self.cur[c]
            x, ev, regs = self.st[key]
            assert np.array_equal(decisions[off:off + n], x[fd:fd + n]), "the test's own cutting"
            mine = [e for e in ev if fd <= e[0] < fd + n]
            out[i] = (int(r["first_window"]), woff, fd, c, n, int(r["flags"]) & 1, len(mine))
            w = pack([bit_of(int(d), self.rule) for d in x[fd:fd + n]])
            words.append(w)
            woff += w.size
            evs += [(e[0], c, i, e[4], e[1], e[2], e[3]) for e in mine]
            self.state[c] = (key[1], fd + n, regs[fd + n - 1] if fd + n else 0, 1)
        bits = np.concatenate(words) if words else np.zeros(0, np.uint32)
        return out, bits, np.array(evs, b.RUNSYNC_EVENT_DTYPE) if evs else np.zeros(0, b.RUNSYNC_EVENT_DTYPE)


def same(got, want, what):
    for g, w, name in zip(got, want, ("runs", "bits", "events")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.dtype.names:
            for f in g.dtype.names:
                bad = np.flatnonzero(g[f] != w[f])
                assert bad.size == 0, f"{what}: {name} field {f} differs at {bad[:5].tolist()}: {g[f][bad[0]]} != {w[f][bad[0]]}"
        else:
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{what}: {name} differ at {bad[:5].tolist()}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"
    gr, gb, ge = got
    # consistent in itself: words dense and ascending, a run's events contiguous behind those of the runs in front
    nw = (gr["nr_dec"].astype(np.uint64) + 31) // 32
    assert np.array_equal(gr["word_offset"], np.cumsum(nw, dtype=np.uint64) - nw) and int(nw.sum()) == gb.size, what
    assert int(gr["nr_events"].sum()) == ge.size and np.array_equal(ge["run"], np.repeat(np.arange(len(gr)), gr["nr_events"])), what


def schedule(pkg, lines, cuts):
    """the calls of a stream: cuts[c][k] are the run lengths of channel c's stretch k.  A call takes every channel's next run and
    the beginning runs behind it (only a channel's first run of a call can continue)"""
    flat = []
    for c, line in enumerate(lines):
        runs = []
        for (fw, x), lens in zip(line, cuts[c]):
            assert sum(lens) == x.size
            at = 0
            for j, n in enumerate(lens):
                runs.append((c, n, j == 0, at, fw + j if j else fw, x[at:at + n]))
                at += n
        flat.append(runs)
    calls, p = [], [0] * len(lines)
    while any(p[c] < len(flat[c]) for c in range(len(lines))):
        rows, pieces, off = [], [], 0
        for c in range(len(lines)):
            first = True
            while p[c] < len(flat[c]) and (first or flat[c][p[c]][2]):
                ch, n, begins, fd, fw, x = flat[c][p[c]]
                rows.append((ch, n, begins, fd, fw, off))
                pieces.append(x)
                off += n
                p[c] += 1
                first = False
        calls.append((make_runs(pkg, rows), np.concatenate(pieces).astype(np.int16) if pieces else np.zeros(0, np.int16)))
    return calls


_SCENE = {}


def scene():
    """three channels: one stretch of 700 decisions; two stretches of 100 and 420; one of 64.  Sync words planted so that one
    straddles every seam of the ragged cut, one is complete inside a stretch's first 31 decisions (SYNC has a leading zero), one
    stands inverted, and the second word of the table stands once"""
    if _SCENE:
        return _SCENE["it"]
    rng = np.random.RandomState(7)
    lens = [[700], [100, 420], [64]]
    lines = [[(5 + 30 * k + c, rng.randint(-9000, 9001, n).astype(np.int16)) for k, n in enumerate(row)] for c, row in enumerate(lens)]
    a = lines[0][0][1]
    a[::97] = 0   # zeros among the decisions: the two bit rules part there
    for end in (40, 75, 110, 170, 230, 300):        # across the seams at 32, 64, 97, 160, 224, 289
        plant(a, end, SYNC)
    plant(a, 350, ~SYNC & M32)
    plant(a, 500, OTHER)
    plant(a, 699, SYNC)                             # a stretch's last decision
    plant(lines[1][0][1], 30, SYNC, lowest=31)      # complete at decision 30: zeros above
    plant(lines[1][0][1], 99, SYNC)
    plant(lines[1][1][1], 31, SYNC)
    plant(lines[1][1][1], 70, SYNC)                 # across 64 and the run of nothing behind it
    plant(lines[1][1][1], 400, SYNC ^ 0x00100100)   # two bits off
    plant(lines[2][0][1], 63, OTHER)
    cuts = {
        "ragged": [[[0, 1, 31, 32, 33, 63, 64, 65, 0, 411]], [[33, 67], [64, 0, 65, 291]], [[64]]],
        "three": [[[100, 250, 350]], [[33, 67], [64, 356]], [[64]]],
        "whole": [[[700]], [[100], [420]], [[64]]],
    }
    _SCENE["it"] = (lines, cuts)
    return _SCENE["it"]


CONFIGS = [dict(words=[SYNC], maxd=3, rule=NOT_POS, either=False), dict(words=[OTHER, SYNC], maxd=3, rule=NOT_POS, either=True),
           dict(words=[SYNC, OTHER], maxd=2, rule=POS, either=True)]


def twin_kw(cf, **more):
    return dict(words=cf["words"], max_distance=cf["maxd"], bit_rule=cf["rule"], either=cf["either"], **more)


# ---- names, sizes, create ---------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runsync_names(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    for name in ("BIT_NOT_POS", "BIT_POS", "F_EITHER", "OVER_RUNS", "OVER_DECISIONS", "OVER_EVENTS", "IN_RUNMM", "IN_OUT_OF_STEP", "IN_BAD_RUNS"):
        m = re.search(r"#define MFM_RUNSYNC_%s (\d+)u" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNSYNC_" + name), name
    own = open(os.path.join(ROOT, "tsl-sdr_amd", "csrc", "mfm_runsync.h")).read()
    assert re.search(r"#define MFM_RUNSYNC_SEGMENT %du" % SEG, own) and b.RUNSYNC_SEGMENT == SEG
    assert "test_mueller_muller.c:130-136" in src
    assert pkg.RunSync is b.RunSync and pkg.hosttwin_runsync_call is b.hosttwin_runsync_call and pkg.RUNSYNC_EVENT_DTYPE is b.RUNSYNC_EVENT_DTYPE
    for name in ("behind", "process_device", "fetch", "device_view", "capacity", "fetch_state", "store_state", "close"):
        assert callable(getattr(pkg.RunSync, name)), name
    assert callable(pkg.RunMm.capacity)


def test_struct_sizes_match_the_dtypes(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    for struct_name, dt, size in (("mfm_runsync_run", b.RUNSYNC_RUN_DTYPE, 40), ("mfm_runsync_event", b.RUNSYNC_EVENT_DTYPE, 32),
                                  ("mfm_runsync_state", b.RUNSYNC_STATE_DTYPE, 24)):
        m = re.search(r"struct %s \{(.*?)\};" % struct_name, src, flags=re.S)
        fields = re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1))
        assert [n for _, n in fields] == list(dt.names), struct_name
        width = {"uint64_t": 8, "uint32_t": 4}
        assert sum(width[t] for t, _ in fields) == size == dt.itemsize, struct_name
        assert re.search(r"struct %s \{\s+/\* %d bytes \*/" % (struct_name, size), src), struct_name
    m = re.search(r"struct mfm_runsync_config \{(.*?)\};", src, flags=re.S)
    fields = [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+)(?:\[8\])?;", m.group(1))]
    assert fields == [f[0] for f in b.RunSyncConfig._fields_] and C.sizeof(b.RunSyncConfig) == 72
    # the Mueller-Muller stage's run record is read through the burst resampler's
    assert [n for n in b.RUNMM_RUN_DTYPE.names] == ["first_window", "dec_offset", "first_dec", "channel", "nr_dec", "flags", "reserved"]
    assert [b.RUNMM_RUN_DTYPE.fields[n][1] for n in b.RUNMM_RUN_DTYPE.names] == [b.RUNRS_RUN_DTYPE.fields[n][1] for n in b.RUNRS_RUN_DTYPE.names]


REFUSALS = [
    (dict(abi_version=3), "abi_version"),
    (dict(nr_channels=0), "nr_channels"),
    (dict(words=[]), "nr_words must be 1 .. 8"),
    (dict(words=[SYNC] * 9), "nr_words must be 1 .. 8"),
    (dict(max_distance=16), "max_distance must be at most 15"),
    (dict(bit_rule=2), "bit_rule must be"),
    (dict(flags=2), "flags must be 0 or MFM_RUNSYNC_F_EITHER"),
    (dict(flags=3), "flags must be 0 or MFM_RUNSYNC_F_EITHER"),
    (dict(max_runs=0), "max_runs must be"),
    (dict(max_decisions=0), "max_decisions"),
    (dict(max_runs=1 << 28), "max_runs must be"),
    (dict(max_decisions=1 << 31), "max_decisions"),
    (dict(max_events=1 << 31), "max_events"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_with_a_message(pkg, change, message):
    """every refusal of mfm_runsync_create is decided before a device is looked for; the twin refuses the same"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_decisions=10000, words=[SYNC])
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunSync(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)
    if kw["nr_channels"]:
        tw = {k: v for k, v in kw.items() if k != "nr_channels"}
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runsync_call(b.hosttwin_runsync_state(kw["nr_channels"]), make_runs(pkg, []), np.zeros(0, np.int16), **tw)
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


# ---- the twin against the restatement -----------------------------------------------------------------------------

def test_the_scene_is_what_it_is_meant_to_be(pkg):
    lines, cuts = scene()
    ev, _ = restate(lines[0][0][1], [SYNC])
    assert [e[0] for e in ev] == [40, 75, 110, 170, 230, 300, 699] and all(e[2] == 0 for e in ev)
    ev, _ = restate(lines[0][0][1], [OTHER, SYNC], either=True)
    assert [(e[0], e[1], e[3]) for e in ev] == [(40, 1, 0), (75, 1, 0), (110, 1, 0), (170, 1, 0), (230, 1, 0), (300, 1, 0), (350, 1, 1), (500, 0, 0), (699, 1, 0)]
    ev, _ = restate(lines[1][0][1], [SYNC])
    assert [e[0] for e in ev] == [30, 99]                      # the first inside the first 31 decisions: zeros above
    ev, _ = restate(lines[1][1][1], [SYNC])
    assert [(e[0], e[2]) for e in ev] == [(31, 0), (70, 0), (400, 2)]
    assert (lines[0][0][1] == 0).sum() >= 3
    seams = np.cumsum(cuts["ragged"][0][0])
    assert all(any(e - 31 <= s <= e for e in (40, 75, 110, 170, 230, 300)) for s in seams[2:8])


@pytest.mark.parametrize("cf", CONFIGS, ids=["one", "either", "pos"])
def test_hosttwin_equals_the_restatement_however_the_stream_is_cut(pkg, cf):
    """the scene cut into runs of 0, 1, 31, 32, 33, 63, 64, 65 decisions (a call a run: only a channel's first run continues), into
    three runs and in one piece: every call against the restatement, record by record, word by word, event by event; a run of
    nothing inside a stretch; a beginning run behind a carried stretch in one call"""
    b = pkg.binding
    lines, cuts = scene()
    seen = {}
    for name, cut in cuts.items():
        want, state = Want(pkg, lines, cf["words"], cf["maxd"], cf["rule"], cf["either"]), b.hosttwin_runsync_state(3)
        calls = schedule(pkg, lines, cut)
        assert len(calls) == dict(ragged=10, three=3, whole=1)[name]
        evs = []
        for i, (runs, dec) in enumerate(calls):
            got = b.hosttwin_runsync_call(state, runs, dec, **twin_kw(cf))
            same(got, want.call(runs, dec), f"{name}: call {i}")
            assert state.tobytes() == want.state.tobytes(), (name, i)
            evs += [(int(e["channel"]), int(e["dec"]), int(e["seen"]), int(e["word_index"]), int(e["distance"]), int(e["inverted"]))
                    for e in got[2]]
        seen[name] = sorted(evs)
    assert seen["ragged"] == seen["three"] == seen["whole"] and len(seen["ragged"]) >= 10
    # the ragged cut is what it is meant to be
    calls = schedule(pkg, lines, cuts["ragged"])
    assert [int(r["nr_dec"]) for runs, _ in calls for r in runs if int(r["channel"]) == 0] == cuts["ragged"][0][0]
    second = calls[1][0]
    assert [(int(r["channel"]), int(r["flags"])) for r in second] == [(0, 0), (1, 0), (1, 1)]   # a beginning run behind a carried stretch


def test_a_match_inside_the_first_31_decisions_and_the_complement(pkg):
    """SYNC has a leading zero: its 31 low bits at a stretch's start match at decision 30, as the reference's loop, which tests
    from the first decision on with zeros above, reports it.  An inverted word is a miss without `either` and a hit with it"""
    b = pkg.binding
    rng = np.random.RandomState(3)
    x = rng.randint(1, 9001, 200).astype(np.int16)
    plant(x, 30, SYNC, lowest=31)
    plant(x, 150, ~SYNC & M32)
    runs = make_runs(pkg, [(0, 200, True, 0, 4, 0)])
    r, bits, ev = b.hosttwin_runsync_call(b.hosttwin_runsync_state(1), runs, x, words=[SYNC])
    assert [(int(e["dec"]), int(e["seen"]), int(e["inverted"])) for e in ev] == [(30, SYNC, 0)]
    assert [e[0] for e in restate(x, [SYNC])[0]] == [30]
    r, bits, ev = b.hosttwin_runsync_call(b.hosttwin_runsync_state(1), runs, x, words=[SYNC], either=True)
    assert [(int(e["dec"]), int(e["seen"]), int(e["inverted"]), int(e["distance"])) for e in ev] == [(30, SYNC, 0, 0), (150, ~SYNC & M32, 1, 0)]
    assert [(e[0], e[3]) for e in restate(x, [SYNC], either=True)[0]] == [(30, 0), (150, 1)]


def test_the_lowest_word_index_wins(pkg):
    b = pkg.binding
    near = SYNC ^ 0x3
    x = np.random.RandomState(5).randint(1, 9001, 100).astype(np.int16)
    plant(x, 60, near)
    runs = make_runs(pkg, [(0, 100, True, 0, 4, 0)])
    for words, want in (([SYNC, near], (0, 2)), ([near, SYNC], (0, 0)), ([OTHER, near, SYNC], (1, 0))):
        _, _, ev = b.hosttwin_runsync_call(b.hosttwin_runsync_state(1), runs, x, words=words)
        assert [(int(e["dec"]), int(e["word_index"]), int(e["distance"])) for e in ev] == [(60,) + want], words
        assert [(e[0], e[1], e[2]) for e in restate(x, words)[0]] == [(60,) + want]


def test_bits_are_word_aligned_per_run_with_zero_tails_and_zero_decisions_follow_the_rule(pkg):
    b = pkg.binding
    x = np.array([5, 0, -5, 0, 7] * 20, np.int16)
    lens = [33, 0, 1, 31, 35]
    rows, off = [], 0
    for c, n in enumerate(lens):
        rows.append((c, n, True, 0, c, off))
        off += n
    for rule, zero_bit in ((NOT_POS, 1), (POS, 0)):
        r, bits, _ = b.hosttwin_runsync_call(b.hosttwin_runsync_state(5), make_runs(pkg, rows), x, words=[SYNC], bit_rule=rule)
        assert r["word_offset"].tolist() == [0, 2, 2, 3, 4] and bits.size == 6
        for c, n in enumerate(lens):
            o, w0 = rows[c][5], int(r["word_offset"][c])
            for j in range(32 * ((n + 31) // 32)):
                got = (int(bits[w0 + j // 32]) >> (j % 32)) & 1
                assert got == (bit_of(int(x[o + j]), rule) if j < n else 0), (rule, c, j)
        assert (int(bits[0]) >> 1) & 1 == zero_bit   # d == 0: a one under the reference's rule, where a sign bit has a zero


def refusal_case(pkg):
    """two calls on three channels; the second, whose first run continues channel 0, is the one that is varied"""
    b = pkg.binding
    rng = np.random.RandomState(12)
    d0, d1 = rng.randint(-9000, 9001, 340).astype(np.int16), rng.randint(-9000, 9001, 900).astype(np.int16)
    for end in (20, 200, 349, 380, 500, 899):
        plant(d1, end, SYNC)
    plant(d0, 299, SYNC >> 21, lowest=11)   # the word's first 11 bits end the first call: decision 20 of the second completes it
    first = make_runs(pkg, [(0, 300, True, 0, 1, 0), (2, 40, True, 0, 1, 300)])
    runs = make_runs(pkg, [(0, 350, False, 300, 1, 0), (0, 50, True, 0, 8, 350), (1, 500, True, 0, 4, 400)])

    def changed(i, **kw):
        r = runs.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    IN = 8
    cases = [
        (dict(totals=[3, 900, 1, 0]), "raised overflow or an input error", b.MFM_RUNSYNC_IN_RUNMM << IN),
        (dict(totals=[3, 900, 0, 2]), "raised overflow or an input error", b.MFM_RUNSYNC_IN_RUNMM << IN),
        (dict(runs=changed(0, first_dec=299)), "out of step", b.MFM_RUNSYNC_IN_OUT_OF_STEP << IN),
        (dict(runs=changed(2, flags=0)), "out of step", b.MFM_RUNSYNC_IN_OUT_OF_STEP << IN),                # channel 1 has no stretch
        (dict(runs=changed(1, flags=0, first_dec=650)), "out of step", b.MFM_RUNSYNC_IN_OUT_OF_STEP << IN),  # not its channel's first
        (dict(runs=changed(2, channel=3)), "not a burst Mueller-Muller stage's", b.MFM_RUNSYNC_IN_BAD_RUNS << IN),
        (dict(runs=changed(0, channel=2)), "not a burst Mueller-Muller stage's", (b.MFM_RUNSYNC_IN_BAD_RUNS | b.MFM_RUNSYNC_IN_OUT_OF_STEP) << IN),
        (dict(runs=changed(1, first_dec=5)), "not a burst Mueller-Muller stage's", b.MFM_RUNSYNC_IN_BAD_RUNS << IN),
        (dict(runs=changed(2, nr_dec=501)), "not a burst Mueller-Muller stage's", b.MFM_RUNSYNC_IN_BAD_RUNS << IN),
        (dict(runs=changed(2, dec_offset=401)), "not a burst Mueller-Muller stage's", b.MFM_RUNSYNC_IN_BAD_RUNS << IN),
        (dict(runs=changed(1, dec_offset=349)), "not a burst Mueller-Muller stage's", b.MFM_RUNSYNC_IN_BAD_RUNS << IN),   # not the running sum
        (dict(totals=[3, 1001, 0, 0]), "more decisions than max_decisions", b.MFM_RUNSYNC_OVER_DECISIONS),
        (dict(totals=[5, 900, 0, 0]), "more runs than max_runs", b.MFM_RUNSYNC_OVER_RUNS),
    ]
    return (first, d0), (runs, d1), cases


def refusal_lines(first, d0, runs, d1):
    return [[(1, np.concatenate([d0[:300], d1[:350]])), (8, d1[350:400])], [(4, d1[400:900])], [(1, d0[300:340])]]


def test_hosttwin_refuses_and_leaves_state_and_output(pkg):
    """every flag; each time nothing comes out and the state stays, so the same call fed correctly is right.  max_events goes by
    the count: one below it is refused, the count itself is enough"""
    b = pkg.binding
    (first, d0), (runs, d1), cases = refusal_case(pkg)
    want, state = Want(pkg, refusal_lines(first, d0, runs, d1), [SYNC]), b.hosttwin_runsync_state(3)
    conf = dict(words=[SYNC], max_runs=4, max_decisions=1000)
    same(b.hosttwin_runsync_call(state, first, d0, **conf), want.call(first, d0), "call 0")
    s0 = state.copy()
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runsync_call(state, change.get("runs", runs), d1, totals=change.get("totals"), **conf)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value), ei.value.flags)
        assert ei.value.needed == (0, 0, 0) and state.tobytes() == s0.tobytes(), change
    w = want.call(runs, d1)
    assert w[2].size == 6 and w[2]["dec"].tolist() == [320, 500, 649, 30, 100, 499]
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runsync_call(state, runs, d1, max_events=5, **conf)
    assert ei.value.code == b.MFM_E_STATE and "events exceed max_events" in str(ei.value) and ei.value.flags == b.MFM_RUNSYNC_OVER_EVENTS
    assert state.tobytes() == s0.tobytes()
    for room in (dict(max_out_runs=2), dict(max_out_words=28), dict(max_out_events=5)):   # the caller's buffers too small
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runsync_call(state, runs, d1, **room, **conf)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, 29, 6) and state.tobytes() == s0.tobytes()
    same(b.hosttwin_runsync_call(state, runs, d1, max_events=6, **conf), w, "the same call, right, after the refused ones")
    assert state.tobytes() == want.state.tobytes()


STATE_REFUSALS = [
    (dict(has_stretch=2), "has_stretch must be 0 or 1"),
    (dict(has_stretch=0), "has_stretch is 0 but another field is not 0"),
    (dict(decs=1 << 62), "decs and stretch_window must be below 2^62"),
    (dict(stretch_window=1 << 62), "decs and stretch_window must be below 2^62"),
    (dict(shr=0x20), "shr must hold no bit at or above bit decs"),
    (dict(decs=0), "shr must hold no bit at or above bit decs"),
]


def good_state(pkg, nch=3):
    st = pkg.binding.hosttwin_runsync_state(nch)
    st[1] = (7, 5, 0x1F, 1)
    st[2] = (9, 32, 0xFFFFFFFF, 1)
    return st


@pytest.mark.parametrize("change,message", STATE_REFUSALS, ids=[str(i) for i in range(len(STATE_REFUSALS))])
def test_state_check_names_channel_and_field(pkg, change, message):
    b = pkg.binding
    st = good_state(pkg)
    b.hosttwin_runsync_state_check(st)
    for k, v in change.items():
        st[k][1] = v
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runsync_state_check(st)
    assert ei.value.code == b.MFM_E_INVAL and "channel 1: " + message in str(ei.value), str(ei.value)


def test_hosttwin_is_clean_under_the_address_and_undefined_sanitizers(pkg, tmp_path):
    """tests/hoststub/runsync_twin_main.cpp, a program of its own built with -fsanitize=address,undefined around the stage's host
    code, runs the twin on the ragged cut in buffers of exactly the sizes needed: nothing to report, and the restatement's result"""
    b = pkg.binding
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    exe = tmp_path / "runsync_twin"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "hoststub", "runsync_twin_main.cpp"),
           os.path.join(ROOT, "tsl-sdr_amd", "csrc", "mfm_runsync.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    if re.search(r"lib(a|t|ub|l|m)san", env.get("LD_PRELOAD", "")):   # another sanitizer's runtime does not share a process with this one
        del env["LD_PRELOAD"]
    env.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    lines, cuts = scene()
    cf = CONFIGS[1]
    want = Want(pkg, lines, cf["words"], cf["maxd"], cf["rule"], cf["either"])
    state_file = tmp_path / "state.bin"
    state_file.write_bytes(b.hosttwin_runsync_state(3).tobytes())
    for i, (runs, dec) in enumerate(schedule(pkg, lines, cuts["ragged"])):
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        words = cf["words"] + [0] * (8 - len(cf["words"]))
        fin.write_bytes(struct.pack("<16I", 3, len(runs), dec.size, 0, len(cf["words"]), *words, cf["maxd"], cf["rule"], 1 if cf["either"] else 0)
                        + runs.tobytes() + dec.tobytes())
        r = subprocess.run([str(exe), str(fin), str(state_file), str(fout)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
        raw = fout.read_bytes()
        nr, nw, ne = struct.unpack("<3Q", raw[:24])
        o1, o2 = 24 + 40 * nr, 24 + 40 * nr + 4 * nw
        got = (np.frombuffer(raw[24:o1], b.RUNSYNC_RUN_DTYPE), np.frombuffer(raw[o1:o2], np.uint32), np.frombuffer(raw[o2:o2 + 32 * ne], b.RUNSYNC_EVENT_DTYPE))
        same(got, want.call(runs, dec), f"call {i}")
    assert state_file.read_bytes() == want.state.tobytes()


def test_runmm_capacity_is_the_twins_bound(pkg):
    """what mfm_runmm_get_capacity reports for max_decisions = 0 is max_out_samples / s + max_runs, the bound the twin holds a call
    against; a value given comes back as it is.  Without a device create fails before there is an object to ask: the bound then
    stands by the twin alone"""
    b = pkg.binding
    par = trm.REF
    s = trm.min_step(par)
    max_runs, max_out = 7, 1000
    bound = max_out // s + max_runs
    # the twin's side: 7 runs that share 1000 outputs fit the default exactly as they fit max_decisions = bound, and not bound - 1
    lens = [142] * 6 + [148]
    rows, off = [], 0
    for c, n in enumerate(lens):
        rows.append((c, n, True, 0, c, off))
        off += n
    runs, x = trm.make_runs(pkg, rows), np.zeros(1000, np.int16)
    need = sum(trm.slots(n, s) for n in lens)
    assert need <= bound
    for md in (0, bound, need):
        b.hosttwin_runmm_call(b.hosttwin_runmm_state(7), runs, x, **trm.twin_kw(par, max_runs=max_runs, max_out_samples=max_out, max_decisions=md))
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runmm_call(b.hosttwin_runmm_state(7), runs, x, **trm.twin_kw(par, max_runs=max_runs, max_out_samples=max_out, max_decisions=need - 1))
    assert ei.value.flags == b.MFM_RUNMM_OVER_DECISIONS
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if have:
        for md, want in ((0, bound), (123, 123)):
            rm = pkg.RunMm(7, max_runs, max_out, par["spb"], par["kw"], par["km"], error_min=par["emin"], error_max=par["emax"], max_decisions=md)
            assert rm.capacity() == (max_runs, want)
            rm.close()
    else:
        with pytest.raises(pkg.MfmError) as ei:
            pkg.RunMm(7, max_runs, max_out, par["spb"], par["kw"], par["km"], error_min=par["emin"], error_max=par["emax"])
        assert ei.value.code == b.MFM_E_DEVICE


def test_runsync_kernels_use_no_scratch(pkg):
    """the code object's notes of build/mfm_runsync.o (tools/kernel_regs.py): the five kernels, no private segment, no spilled
    register, at most 128 VGPRs"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runsync.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"rsy_{k}_kernel" for k in ("plan", "match", "scan", "place", "state")), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _fed(pkg, torch, rs, runs, dec, totals=None):
    """one call from uploaded arrays: a burst Mueller-Muller call's result as it would stand in its device view"""
    t = np.array([len(runs), dec.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, dec), tr._up(torch, t))
    rs.process_device(*(k.data_ptr() for k in keep))
    try:
        return rs.fetch()
    finally:
        del keep


def _device_totals(rs):
    return tl._d2h(rs.device_view()[3], 32).view(np.uint64).tolist()


def _make(pkg, nch, max_runs, max_dec, cf, **kw):
    return pkg.RunSync(nch, max_runs, max_dec, cf["words"], max_distance=cf["maxd"], bit_rule=cf["rule"], either=cf["either"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cf", CONFIGS, ids=["one", "either", "pos"])
def test_gpu_equals_twin_and_restatement_on_the_seam_cases(pkg, cf):
    """the CPU scene in its three cuts (ten calls of ragged runs, three calls, one): the restatement call by call, the twin's
    state, the device view"""
    import torch
    b = pkg.binding
    lines, cuts = scene()
    for name, cut in cuts.items():
        rs = _make(pkg, 3, 4, 1300, cf)
        want, twin = Want(pkg, lines, cf["words"], cf["maxd"], cf["rule"], cf["either"]), b.hosttwin_runsync_state(3)
        for i, (runs, dec) in enumerate(schedule(pkg, lines, cut)):
            got = _fed(pkg, torch, rs, runs, dec)
            w = want.call(runs, dec)
            same(got, w, f"{name}: call {i}")
            same(b.hosttwin_runsync_call(twin, runs, dec, **twin_kw(cf)), got, f"{name}: the twin's call {i}")
            assert rs.fetch_state().tobytes() == twin.tobytes() == want.state.tobytes(), (name, i)
            assert _device_totals(rs) == [len(runs), w[2].size, 0, 0]
            d_runs, d_bits, d_ev, _ = rs.device_view()
            assert tl._d2h(d_runs, got[0].nbytes).tobytes() == got[0].tobytes()
            if got[2].size:
                assert tl._d2h(d_ev, got[2].nbytes).tobytes() == got[2].tobytes()
        assert rs.capacity() == (4, 1300 // 32 + 4, 1300)
        rs.close()


@pytest.mark.gpu
def test_gpu_seams_of_the_machine(pkg):
    """words that end on decision 63, 64 and 65 of a run and on the last and first decision of a segment of SEG decisions, in runs
    whose dec_offset is odd and whose word_offset follows a run with nr_dec % 32 != 0; a second call continues them with a word
    across the call seam (the register seeded from the state) and one complete at decision 31"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(21)
    n0 = [1, 2 * SEG + 52, 2 * SEG + 1, SEG + 77, 33, 100]
    n1 = [0, 40, SEG + 1, 64, 0, 31]
    lines = [[(c + 2, rng.randint(-9000, 9001, n0[c] + n1[c]).astype(np.int16))] for c in range(6)]
    for c, ends in ((1, (63, SEG - 1, 2 * SEG, 2 * SEG + 52 + 5)), (2, (64, SEG, 2 * SEG - 1, 2 * SEG + 1 + 31, 3 * SEG + 1)),
                    (3, (65, SEG + 30, SEG + 77 + 63)), (4, (32,)), (5, (99, 130))):
        for e in ends:
            plant(lines[c][0][1], e, SYNC)
    cut = [[[n0[c], n1[c]]] for c in range(6)]
    calls = schedule(pkg, lines, cut)
    assert len(calls) == 2 and [int(o) % 2 for o in calls[0][0]["dec_offset"][1:4]] == [1, 1, 0]
    cf = CONFIGS[0]
    rs = _make(pkg, 6, 6, sum(n0), cf)
    want, twin = Want(pkg, lines, cf["words"]), b.hosttwin_runsync_state(6)
    total = 0
    for i, (runs, dec) in enumerate(calls):
        got = _fed(pkg, torch, rs, runs, dec)
        w = want.call(runs, dec)
        same(got, w, f"call {i}")
        same(b.hosttwin_runsync_call(twin, runs, dec, **twin_kw(cf)), got, f"the twin's call {i}")
        assert rs.fetch_state().tobytes() == twin.tobytes() == want.state.tobytes(), i
        total += w[2].size
    assert total == 15
    rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1025, 2049])
def test_gpu_more_runs_than_lanes_waves_and_the_plan_block(pkg, n):
    """one run of 0 .. 40 decisions per channel, a table that matches about two registers in five; a second call continues every
    third channel, begins every third anew and leaves the rest out"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(n)
    cf = dict(words=[SYNC, OTHER], maxd=15, rule=NOT_POS, either=False)
    l0 = [(7 * i) % 41 for i in range(n)]
    l1 = [(11 * i + 5) % 41 for i in range(n)]
    lines, cut = [], []
    for c in range(n):
        if c % 3 == 0:
            lines.append([(c % 5, rng.randint(-9, 10, l0[c] + l1[c]).astype(np.int16))])
            cut.append([[l0[c], l1[c]]])
        elif c % 3 == 1:
            lines.append([(c % 5, rng.randint(-9, 10, l0[c]).astype(np.int16)), (77, rng.randint(-9, 10, l1[c]).astype(np.int16))])
            cut.append([[l0[c]], [l1[c]]])
        else:
            lines.append([(c % 5, rng.randint(-9, 10, l0[c]).astype(np.int16))])
            cut.append([[l0[c]]])
    # schedule() would put a channel's second stretch into the first call; here it belongs to the second
    want, twin = Want(pkg, lines, cf["words"], cf["maxd"]), b.hosttwin_runsync_state(n)
    first, second, off0, off1, p0, p1 = [], [], 0, 0, [], []
    for c in range(n):
        first.append((c, l0[c], True, 0, c % 5, off0))
        p0.append(lines[c][0][1][:l0[c]])
        off0 += l0[c]
        if c % 3 == 0:
            second.append((c, l1[c], False, l0[c], c % 5 + 1, off1))
            p1.append(lines[c][0][1][l0[c]:])
            off1 += l1[c]
        elif c % 3 == 1:
            second.append((c, l1[c], True, 0, 77, off1))
            p1.append(lines[c][1][1])
            off1 += l1[c]
    calls = [(make_runs(pkg, first), np.concatenate(p0)), (make_runs(pkg, second), np.concatenate(p1))]
    rs = _make(pkg, n, n, max(off0, off1), cf)
    events = 0
    for i, (runs, dec) in enumerate(calls):
        got = _fed(pkg, torch, rs, runs, dec)
        w = want.call(runs, dec)
        same(got, w, f"call {i}")
        same(b.hosttwin_runsync_call(twin, runs, dec, **twin_kw(cf)), got, f"the twin's call {i}")
        assert rs.fetch_state().tobytes() == twin.tobytes(), i
        events += w[2].size
    assert events >= n
    rs.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state_and_a_state_stored_is_a_state_fetched(pkg):
    """every refusal of the twin's test on the device, with the twin's flags in the totals, and max_events one below the call's
    count; each time nothing comes out and the state stays.  The state then moves to a second object mid-stretch (store_state,
    fetched back unchanged; a state that fails is refused with channel and field and changes nothing), where the same input with
    room for its events is right"""
    import torch
    b = pkg.binding
    (first, d0), (runs, d1), cases = refusal_case(pkg)
    want = Want(pkg, refusal_lines(first, d0, runs, d1), [SYNC])
    cf = CONFIGS[0]
    rs = _make(pkg, 3, 4, 1000, cf, max_events=5)
    same(_fed(pkg, torch, rs, first, d0), want.call(first, d0), "call 0")
    s0 = rs.fetch_state()
    twin = s0.copy()
    conf = dict(words=[SYNC], max_runs=4, max_decisions=1000, max_events=5)
    for change, message, flags in cases + [(dict(), "events exceed max_events", b.MFM_RUNSYNC_OVER_EVENTS)]:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rs, change.get("runs", runs), d1, totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == (0, 0, 0)
        assert _device_totals(rs) == [0, 0, flags & 0xff, flags >> 8], (change, _device_totals(rs))
        with pytest.raises(pkg.MfmError) as et:
            b.hosttwin_runsync_call(twin, change.get("runs", runs), d1, totals=change.get("totals"), **conf)
        assert et.value.flags == flags and str(et.value).split(": ", 1)[-1] == str(ei.value).split(": ", 1)[-1]
        assert rs.fetch_state().tobytes() == s0.tobytes() == twin.tobytes(), change
    fits = _make(pkg, 3, 4, 1000, cf, max_events=6)
    bad = s0.copy()
    bad["has_stretch"][2] = 2
    with pytest.raises(pkg.MfmError) as ei:
        fits.store_state(bad)
    assert ei.value.code == b.MFM_E_INVAL and "channel 2: has_stretch must be" in str(ei.value)
    assert not fits.fetch_state().view(np.uint8).any()
    fits.store_state(s0)
    assert fits.fetch_state().tobytes() == s0.tobytes()
    w = want.call(runs, d1)
    assert w[2].size == 6 and int(w[2]["dec"][0]) == 320   # the word across the move: 11 of its bits stand in the state
    got = _fed(pkg, torch, fits, runs, d1)
    same(got, w, "the same call in an object it fits")
    with pytest.raises(pkg.MfmError) as ei:
        fits.fetch(max_runs=3, max_words=29, max_events=5)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, 29, 6)
    same(fits.fetch(), w, "fetched again")
    b.hosttwin_runsync_call(twin, runs, d1, **dict(conf, max_events=6))
    assert fits.fetch_state().tobytes() == twin.tobytes() == want.state.tobytes()
    # and the object that refused takes the next call that fits
    nxt = make_runs(pkg, [(2, 60, False, 40, 1, 0)])
    d2 = np.random.RandomState(1).randint(-9000, 9001, 60).astype(np.int16)
    plant(d2, 50, SYNC)
    got = _fed(pkg, torch, rs, nxt, d2)
    assert got[2]["dec"].tolist() == [90] and int(rs.fetch_state()["decs"][2]) == 100
    for o in (rs, fits):
        o.close()


CHAIN = dict(nch=4, W=256, P=1, n=256 * 100, hang=1, tx=(0, 2), idle=(1, 3))
_CHAIN = {}


def _chain(pkg):
    """four PCM rows at 31 250 Hz (25 kHz behind the 4/5 resampler).  Rows 0 and 2 carry a 1200-baud POCSAG transmission each
    (pkg.synth: a short preamble and one batch), row 1 quiet noise that never opens the squelch, row 3 two loud stretches of a
    random 1200-baud square wave that opens it and holds no sync word; the squelch opens above an rms of 1000"""
    if _CHAIN:
        return _CHAIN["it"]
    s, sy = CHAIN, pkg.synth
    n, W = s["n"], s["W"]
    rng = np.random.RandomState(23)
    rows = (rng.randn(s["nch"], n) * 60).round().astype(np.int16)
    for c, lead, text in ((0, W * 3 + 17, "SYNC IN BURSTS"), (2, W * 8 + 100, "ANOTHER")):
        bits = sy.pocsag_bits(sy.pocsag_batches([(0x12345 + c, 3, 2, sy.pocsag_alpha_words(text))]), preamble_bits=300)
        pcm = sy.pocsag_pcm(bits, 1200, noise=900, seed=c + 1, rate=31250)
        assert lead + pcm.size < n
        rows[c, lead:lead + pcm.size] = pcm
    t = np.arange(n)
    for a, e in ((W * 5 + 3, W * 30 + 40), (W * 50, W * 80 + 9)):
        bits = rng.randint(0, 2, n // 20 + 2) * 2 - 1
        wave = bits[((t[a:e] - a) * 1200.0 / 31250.0).astype(np.int64)] * 7000 + rng.randn(e - a) * 900
        rows[3, a:e] = np.clip(wave, -32768, 32767).round().astype(np.int16)
    thr = W * 1000 * 1000
    mask = tl.restate(pkg, rows, W, tl.PCM, sense=tl.ABOVE, open_thr=thr, close_thr=thr, hang=s["hang"])["open"].astype(bool)
    lpf = [float(x) for x in sy.design_lpf(41, 0.45 / 5, 1.0) * 4]
    rtaps = np.array([int(x * 16384.0) for x in lpf], np.int16)
    cuts = [0, W * 7, W * 1, 3 * W + 5, W - 5]
    while sum(cuts) < n:
        cuts.append(min(W * int(rng.randint(1, 20)), n - sum(cuts)))
    _CHAIN["it"] = dict(rows=np.ascontiguousarray(rows), mask=mask, thr=thr, rtaps=rtaps, cuts=cuts)
    return _CHAIN["it"]


def _chain_calls(pkg, ora):
    """the burst Mueller-Muller stage's calls of the chain scene through the restated level and gate, the oracle's resampler and
    the Mueller-Muller twin: [(runs RUNMM_RUN_DTYPE, decisions)], and the decisions per stretch"""
    if "calls" in _CHAIN:
        return _CHAIN["calls"]
    b = pkg.binding
    sc, s = _chain(pkg), CHAIN
    W, P = s["W"], s["P"]
    rs, mm = tr.Checker(pkg, ora, sc["rtaps"], 4, 5, False, W), b.hosttwin_runmm_state(s["nch"])
    pos, calls = 0, []
    for m in sc["cuts"] + [None]:
        if m is not None:
            want_rs = rs.call(*tgp.restate_pre(pkg, sc["rows"], sc["mask"], W, 1, P, pos, m))
            pos += m
        else:
            want_rs = rs.call(*tgp.restate_pre(pkg, sc["rows"], sc["mask"], W, 1, P, pos, 0, flush=True))
        calls.append((want_rs, b.hosttwin_runmm_call(mm, *want_rs, **trm.twin_kw(trm.REF))))
    by = trm.by_stretch([(rin, out) for (rin, _), out in calls])
    _CHAIN["calls"] = (calls, by)
    return _CHAIN["calls"]


def test_chain_scene_is_what_it_is_meant_to_be(pkg, ora):
    """the restatement finds at least one sync word in the decisions of every transmitting channel and none on the idle ones"""
    calls, by = _chain_calls(pkg, ora)
    found = {c: 0 for c in range(CHAIN["nch"])}
    decs = {c: 0 for c in range(CHAIN["nch"])}
    for (c, fw), d in by.items():
        found[c] += len(restate(d, [SYNC])[0])
        decs[c] += d.size
    assert all(found[c] >= 1 for c in CHAIN["tx"]), found
    assert all(found[c] == 0 for c in CHAIN["idle"]), found
    assert decs[1] == 0 and decs[3] >= 500 and all(decs[c] >= 800 for c in CHAIN["tx"]), decs


@pytest.mark.gpu
def test_gpu_level_gate_runrs_runmm_runsync_on_device_equals_the_chain_through_the_twins(pkg, ora):
    """level -> gate with P = 1 -> burst resampler 4/5 -> burst Mueller-Muller -> burst sync, all on the device views with no fetch
    in between, in ragged calls and the flush: every call against the same chain through the host twins, and every event one the
    restatement finds in its stretch"""
    b = pkg.binding
    sc, s = _chain(pkg), CHAIN
    calls, by = _chain_calls(pkg, ora)
    rows, cuts, W, P, nch = sc["rows"], sc["cuts"], s["W"], s["P"], s["nch"]
    cap = max(cuts)
    lv = pkg.Level(nch, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=s["hang"])
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    rr = pkg.RunResampler(nch, sc["rtaps"], 4, 5, W, max_in_samples=cap, preroll_windows=P)
    rm = pkg.RunMm.behind(rr, trm.REF["spb"], trm.KW, trm.KM, error_min=trm.REF["emin"], error_max=trm.REF["emax"])
    rs = pkg.RunSync.behind(rm, [SYNC])
    max_runs, max_out = rr.capacity()
    assert rm.capacity() == (max_runs, max_out // trm.min_step(trm.REF) + max_runs)   # the default the twin's bound implies
    assert rs.capacity() == (max_runs, rm.capacity()[1] // 32 + max_runs, rm.capacity()[1])
    twin = b.hosttwin_runsync_state(nch)
    pos, seen, cur = 0, [], {}
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gate.process_host(rows[:, pos:pos + m], lv.process_host(rows[:, pos:pos + m]))
            pos += m
        else:
            gate.flush_device()
        rr.process_device(*gate.device_view())
        rm.process_device(*rr.device_view())
        rs.process_device(*rm.device_view())
        got = rs.fetch()
        (_, _), (mruns, mdec) = calls[i]
        trm.same(rm.fetch(), (mruns, mdec), f"the Mueller-Muller call {i}")
        same(b.hosttwin_runsync_call(twin, mruns, mdec, words=[SYNC]), got, f"call {i}")
        for r in got[0]:
            if int(r["flags"]) & 1:
                cur[int(r["channel"])] = int(r["first_window"])
        seen += [(int(e["channel"]), cur[int(e["channel"])], int(e["dec"]), int(e["distance"])) for e in got[2]]
    want = sorted((c, fw, e[0], e[2]) for (c, fw), d in by.items() for e in restate(d, [SYNC])[0])
    assert sorted(seen) == want and {c for c, _, _, _ in want} == set(s["tx"])
    assert rs.fetch_state().tobytes() == twin.tobytes()
    for o in (rs, rm, rr, gate, lv):
        o.close()


def _tool_events(pkg, ora):
    """[(channel, first window, dec, distance, register)] the restatement finds in the tool scene of tests/test_runmm.py"""
    by = trm.tool_want(pkg, ora)
    return sorted((c, fw, e[0], e[2], e[4]) for (c, fw), d in by.items() for e in restate(d, [SYNC])[0]), by


def test_tool_scene_holds_sync_words(pkg, ora):
    ev, by = _tool_events(pkg, ora)
    assert len(ev) >= 2 and {c for c, _, _, _, _ in ev} == {0, 1}


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_sync_writes_the_events_of_the_restatement(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-mm 16 --gate-sync 0x7CD215D8/3 as a fresh child process on the chain scene of
    tests/test_runpocsag.py: sync.jsonl holds the restatement's events and a summary line per stretch; the same command without
    --gate-sync writes byte-identical mm.jsonl and .mm.s16 files and no sync.jsonl"""
    import json
    base = trm.tool_setup(pkg, ora, tmp_path)
    want, by = _tool_events(pkg, ora)
    W = trm.trp.CHAIN["W"]
    common = ["--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-mm", "16"]
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "with")] + common + ["--gate-sync", "0x7CD215D8/3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "without")] + common, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in (tmp_path / "with" / "sync.jsonl").read_text().splitlines()]
    events = [ln for ln in lines if "dec" in ln]
    assert all(set(ln) == {"channel", "first_window", "first_sample", "dec", "word", "distance", "inverted", "seen"} for ln in events)
    assert sorted((ln["channel"], ln["first_window"], ln["dec"], ln["distance"], int(ln["seen"], 16)) for ln in events) == want
    assert all(ln["word"] == "7cd215d8" and ln["inverted"] == 0 and ln["first_sample"] == ln["first_window"] * W for ln in events)
    summaries = {(ln["channel"], ln["first_window"]): ln for ln in lines if "decisions" in ln}
    assert summaries.keys() == by.keys() and len(summaries) + len(events) == len(lines)
    for key, d in by.items():
        assert summaries[key]["decisions"] == d.size and summaries[key]["events"] == {"7cd215d8": sum(1 for e in want if e[:2] == key)}, key
    trm.tool_check(tmp_path / "with", by, W)
    assert not (tmp_path / "without" / "sync.jsonl").exists()
    names = sorted(p.name for p in (tmp_path / "without").iterdir())
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == sorted(names + ["sync.jsonl"])
    for name in names:
        assert (tmp_path / "with" / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), name
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "x"), "--gate-sync", "0x7CD215D8"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-sync needs --gate-mm" in r.stderr


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_a_sync_object_in_an_mm_route(pkg, ora, tmp_path):
    """a route of stage mm that carries "sync": DIR/<name>/sync.jsonl holds the restatement's events with the configuration's
    channel numbers, as --gate-sync writes them"""
    import json
    base = trm.tool_setup(pkg, ora, tmp_path)
    want, by = _tool_events(pkg, ora)
    doc = {"local": True, "routes": [{"name": "sym", "stage": "mm", "resample": "4/5", "taps": str(tmp_path / "filter.json"), "channels": [0, 1],
                                      "mm": {"spb": 16}, "sync": {"words": [OTHER, SYNC], "distance": 3}}]}
    (tmp_path / "routes.json").write_text(json.dumps(doc))
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "routed"), "--gate-route", str(tmp_path / "routes.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in (tmp_path / "routed" / "sym" / "sync.jsonl").read_text().splitlines()]
    two = sorted((c, fw, e[0], e[2], e[4]) for (c, fw), d in by.items() for e in restate(d, [OTHER, SYNC])[0])
    assert sorted((ln["channel"], ln["first_window"], ln["dec"], ln["distance"], int(ln["seen"], 16)) for ln in lines if "dec" in ln) == two
    assert len(two) >= len(want) and {(ln["channel"], ln["first_window"]) for ln in lines if "decisions" in ln} == set(by)
    trm.tool_check(tmp_path / "routed" / "sym", by, trm.trp.CHAIN["W"])


SYNC_REFUSALS = [
    (dict(sync={"distance": 3}), "\"sync\" must be an object with words"),
    (dict(sync={"words": []}), "\"sync\" must be an object with words"),
    (dict(sync={"words": [1 << 32]}), "\"sync\" must be an object with words"),
    (dict(sync={"words": [SYNC], "distance": 16}), "\"sync\" must be an object with words"),
    (dict(sync={"words": [SYNC], "either": 1}), "\"sync\" must be an object with words"),
    (dict(stage="pocsag", sync={"words": [SYNC]}), "\"sync\" belongs to stage mm, not to stage pocsag"),
]


@pytest.mark.parametrize("change,message", SYNC_REFUSALS, ids=[str(i) for i in range(len(SYNC_REFUSALS))])
def test_level_scan_tool_refuses_a_bad_sync_object_and_flag(tmp_path, change, message):
    """what is wrong with a route's "sync" object or with --gate-sync ends the run with a message before anything is set up"""
    import json
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}, {"chanCenterFreq": 928900000}]}))
    route = {"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"spb": 16}}
    route.update(change)
    if route["stage"] != "mm":
        del route["mm"]
    (tmp_path / "routes.json").write_text(json.dumps({"routes": [route]}))
    tool = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", str(tmp_path / "none.bin"),
            "--gate-out", str(tmp_path / "out")]
    r = subprocess.run(tool + ["--gate-route", str(tmp_path / "routes.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "out").exists()
    rs = ["--gate-resample", "4/5", "--resample-taps", "f.json"]
    for flags, text in ((rs + ["--gate-sync", "0x7CD215D8"], "--gate-sync needs --gate-mm"),
                        (rs + ["--gate-mm", "16", "--gate-sync", "sync"], "--gate-sync takes WORD[,WORD...][/DIST][,either]"),
                        (rs + ["--gate-mm", "16", "--gate-sync", "0x7CD215D8/16"], "distance (0 .. 15)")):
        r = subprocess.run(tool + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and text in r.stderr, (flags, r.stderr[-2000:])


@pytest.mark.gpu
def test_gpu_runmm_capacity_is_what_was_given_or_the_default(pkg):
    par = trm.REF
    s = trm.min_step(par)
    for md, want in ((0, 1000 // s + 7), (123, 123)):
        rm = pkg.RunMm(7, 7, 1000, par["spb"], par["kw"], par["km"], error_min=par["emin"], error_max=par["emax"], max_decisions=md)
        assert rm.capacity() == (7, want)
        rm.close()
