"""The burst batch stage (mfm_runbatch_*, csrc/mfm_runbatch.hip): behind a sync event of the burst sync stage, batches of 16
codewords with their BCH verdicts, and sync kept / sync lost in the slot behind every batch.

The expected result is never the code under test: a plain restatement of the rule in include/multifm_hip.h (restate below), run
per stretch over the concatenated decisions, with the sync events of tests/test_runsync.py's restatement and the oracle's
BCH(31,21).  Every comparison is an equality of every field of every event and of the state bytes.  A second yardstick is the
reference decoder's oracle, fed the decisions at 16 samples each."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_level as tl
import test_pocsag as tp
import test_runmm as trm
import test_runrs as tr
import test_runsync as trs

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runbatch_create", "mfm_runbatch_destroy", "mfm_runbatch_process_device", "mfm_runbatch_fetch", "mfm_runbatch_device_view",
             "mfm_runbatch_get_capacity", "mfm_runbatch_fetch_state", "mfm_runbatch_store_state", "mfm_hosttwin_runbatch_call",
             "mfm_hosttwin_runbatch_state_check"]
SYNC, OTHER, M32 = trs.SYNC, trs.OTHER, trs.M32
FOUND, BATCH, LOST, KEPT = 1, 2, 3, 4       # MFM_POCSAG_EV_*
SEARCH, RECEIVE, SLOT = 0, 1, 2             # MFM_RUNBATCH_*
FRAME = 544
NAMES = {FOUND: "FOUND", BATCH: "BATCH", LOST: "LOST", KEPT: "KEPT"}
Z16 = (0,) * 16


# ---- the yardstick ------------------------------------------------------------------------------------------------

_BCH = {}


def bch(ora, w):
    """(corrected, failed) of raw & 0x7fffffff by the oracle's bch_code_decode"""
    w &= 0x7FFFFFFF
    if w not in _BCH:
        rc, out = ora.bch3121_decode(w)
        _BCH[w] = (int(out), int(rc))
    return _BCH[w]


def restate(ora, b, sev, words, keep=4, word_mask=0, payload=True):
    """the rule over the bits b[n] of one stretch and its sync events [(n, word index, distance, inverted, register)]:
    [(type, dec, aux, word_index, inverted, nr_ok, fail_mask, raw, corrected)] and the automaton (mode, mark, word_index, inverted)
    behind the last bit"""
    n, out = len(b), []
    mode, mark, wi, inv = SEARCH, 0, 0, 0
    while True:
        if mode == SEARCH:
            e = next((e for e in sev if mark <= e[0] < n and (word_mask == 0 or (word_mask >> e[1]) & 1)), None)
            if e is None:
                break
            out.append((FOUND, e[0], e[4], e[1], e[3], e[2], 0, Z16, Z16))
            wi, inv = e[1], e[3]
            mark = e[0] + 1
            mode = RECEIVE
        elif mode == RECEIVE:
            if mark + 511 >= n:
                break
            raw, cor, fail = Z16, Z16, 0
            if payload:
                raw = tuple(sum((int(b[mark + 32 * z + i]) ^ inv) << i for i in range(32)) for z in range(16))
                fixed = [bch(ora, w) for w in raw]
                cor = tuple(f[0] for f in fixed)
                fail = sum(1 << z for z in range(16) if fixed[z][1])
            nr_ok = next((z for z in range(16) if (fail >> z) & 1), 16)
            out.append((BATCH, mark + 511, 0, wi, inv, nr_ok, fail, raw, cor))
            mode = SLOT
        else:
            if mark + 543 >= n:
                break
            seen = 0
            for i in range(32):
                seen = (seen << 1) | (int(b[mark + 512 + i]) ^ inv)
            if bin(seen ^ words[wi]).count("1") <= keep:
                out.append((KEPT, mark + 543, seen, wi, inv, 0, 0, Z16, Z16))
                mark += 544
                mode = RECEIVE
            else:
                out.append((LOST, mark + 543, seen, wi, inv, 0, 0, Z16, Z16))
                mark += 575
                mode, wi, inv = SEARCH, 0, 0
    return out, (mode, mark, wi, inv)


def bits_of(x):
    return (np.asarray(x) <= 0).astype(np.uint8)    # MFM_RUNSYNC_BIT_NOT_POS


def pack(b):
    """one bit per decision, bit j % 32 of word j / 32, the tail 0"""
    w = np.zeros(((len(b) + 31) // 32) * 4, np.uint8)
    pb = np.packbits(np.asarray(b, np.uint8), bitorder="little")
    w[:pb.size] = pb
    return w.view("<u4")


class Want:
    """what the sync stage hands over and what the batch stage must return for the calls of one stream, from the restatements:
    lines[c] = [(first window, decisions)] are channel c's stretches one behind the other, known whole in advance"""

    def __init__(self, pkg, ora, lines, words=(SYNC,), maxd=3, either=False, keep=4, word_mask=0):
        self.pkg, self.ora, self.words, self.keep, self.mask = pkg, ora, list(words), keep, word_mask
        self.st = {}
        for c, line in enumerate(lines):
            for fw, x in line:
                b = bits_of(x)
                sev, _ = trs.restate(x, self.words, maxd, trs.NOT_POS, either)
                bev, _ = restate(ora, b, sev, self.words, keep, word_mask)
                self.st[(c, fw)] = (x, b, sev, bev)
        self.state = pkg.binding.hosttwin_runbatch_state(len(lines))
        self.cur = {}

    def state_at(self, key, L):
        """the canonical state of a channel whose stretch `key` has had L decisions"""
        x, b, sev, _ = self.st[key]
        (mode, mark, wi, inv), st = restate(self.ora, b[:L], sev, self.words, self.keep, self.mask, payload=False)[1], \
            np.zeros(1, self.pkg.binding.RUNBATCH_STATE_DTYPE)
        kept = np.zeros(17, np.uint32)
        nk = 0
        if mode != SEARCH:
            nk = L - mark
            w = pack(b[mark:L])
            kept[:w.size] = w
        st[0] = (key[1], L, mark, 1, mode, wi, inv, nk, 0, kept, 0)
        return st[0]

    def call(self, mruns):
        """(sync runs, bit words, sync events), batch events of the call whose burst Mueller-Muller runs are mruns"""
        b_ = self.pkg.binding
        sruns = np.zeros(len(mruns), b_.RUNSYNC_RUN_DTYPE)
        words, sevs, bevs, woff = [], [], [], 0
        for i, r in enumerate(mruns):
            c, n, fd = int(r["channel"]), int(r["nr_dec"]), int(r["first_dec"])
            if int(r["flags"]) & 1:
                self.cur[c] = (c, int(r["first_window"]))
            key = self.cur[c]
            x, b, sev, bev = self.st[key]
            mine = [e for e in sev if fd <= e[0] < fd + n]
            sruns[i] = (int(r["first_window"]), woff, fd, c, n, int(r["flags"]) & 1, len(mine))
            w = pack(b[fd:fd + n])
            words.append(w)
            woff += w.size
            sevs += [(e[0], c, i, e[4], e[1], e[2], e[3]) for e in mine]
            bevs += [(e[0], c, i, e[2], e[3], e[4], e[5], e[6], key[1], e[1], e[7], e[8]) for e in bev if fd <= e[1] < fd + n]
            self.state[c] = self.state_at(key, fd + n)
        bits = np.concatenate(words) if words else np.zeros(0, np.uint32)
        se = np.array(sevs, b_.RUNSYNC_EVENT_DTYPE) if sevs else np.zeros(0, b_.RUNSYNC_EVENT_DTYPE)
        be = np.zeros(len(bevs), b_.RUNBATCH_EVENT_DTYPE)
        for i, e in enumerate(bevs):
            be[i] = e
        return (sruns, bits, se), be


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape, [NAMES[int(t)] for t in got["type"]],
                                                                 [NAMES[int(t)] for t in want["type"]])
    for f in got.dtype.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(got.size, -1).any(axis=1)) if got.size else np.zeros(0, int)
        assert bad.size == 0, f"{what}: field {f} differs at {bad[:5].tolist()}: {got[f][bad[0]]} != {want[f][bad[0]]}"


def twin_kw(w, **more):
    return dict(words=w.words, keep_distance=w.keep, word_mask=w.mask, **more)


def noise(rng, n):
    """decisions without a zero: the two bit rules and the reference's sample < 0 agree on them"""
    return (rng.randint(1, 9001, n) * (rng.randint(0, 2, n) * 2 - 1)).astype(np.int16)


def put(x, at, bits, inverted=False):
    """the bits into the decisions from `at` on: a 1 is a negative decision"""
    bb = np.asarray(bits, np.uint8) ^ (1 if inverted else 0)
    mag = np.abs(x[at:at + bb.size].astype(np.int32))
    x[at:at + bb.size] = np.where(bb == 1, -mag, mag).astype(np.int16)


def flip(x, at):
    x[at] = -x[at]


def random_batches(pkg, rng, n):
    return [[pkg.synth.pocsag_codeword(int(v)) for v in rng.randint(0, 1 << 21, 16)] for _ in range(n)]


def transmission(pkg, batches, pre=32):
    """preamble, then a sync word and 16 words per batch: the first sync word ends at bit pre + 31"""
    return pkg.synth.pocsag_bits(batches, preamble_bits=pre)


_SCENE = {}


def scene(pkg):
    """three channels.  0: one stretch with FOUND BATCH KEPT BATCH LOST (a sync word planted inside the first batch), a sync word
    that ends on mark = p + 575 and is taken, a third batch and a second LOST.  1: the same transmission inverted, with a sync word
    that ends on p + 574 behind its LOST and is ignored; a stretch that ends inside a batch; a stretch that ends inside a slot.  2:
    decisions without a sync word"""
    if _SCENE:
        return _SCENE["it"]
    rng = np.random.RandomState(11)
    b2 = random_batches(pkg, rng, 3)
    t1 = noise(rng, 32 + 2 * FRAME)
    put(t1, 0, transmission(pkg, b2[:2]))
    trs.plant(t1, 260, SYNC)                  # inside the first batch: ignored, and the words it lies in are no codewords
    a = noise(rng, 3000)
    a[40:40 + t1.size] = t1                   # FOUND 103, p = 104, BATCH 615, KEPT 647, p = 648, BATCH 1159, LOST 1191, mark 1223
    trs.plant(a, 1223, SYNC)                  # bits 1192 .. 1223: wholly behind the failed slot
    put(a, 1224, transmission(pkg, b2[2:], pre=0)[32:])   # BATCH 1735, LOST 1767
    b = noise(rng, 1400)
    b[7:7 + t1.size] = -t1                    # FOUND 70, p = 71, BATCH 582, KEPT 614, p = 615, BATCH 1126, LOST 1158, mark 1190
    trs.plant(b, 1189, SYNC)                  # bits 1158 .. 1189: overlaps the failed slot's last bit
    c = noise(rng, 900)
    put(c, 20, transmission(pkg, random_batches(pkg, rng, 2))[:880])      # FOUND 83, BATCH 595, KEPT 627, p = 628: needs 1139
    d = noise(rng, 620)
    put(d, 30, transmission(pkg, random_batches(pkg, rng, 2))[:590])      # FOUND 93, BATCH 605, the slot 606 .. 637
    lines = [[(5, a)], [(9, b), (40, c), (77, d)], [(3, noise(rng, 800))]]
    cuts = {
        "ragged": [[[0, 1, 31, 32, 33, 7, 511, 1, 31, 1, 512, 32, 31, 1, 543, 1, 1232]], [[70, 1, 0, 544, 543, 242], [84, 816], [300, 320]],
                   [[100, 0, 700]]],
        "three": [[[1000, 1000, 1000]], [[700, 700], [900], [310, 310]], [[300, 300, 200]]],
        "whole": [[[3000]], [[1400], [900], [620]], [[800]]],
    }
    _SCENE["it"] = (lines, cuts)
    return _SCENE["it"]


SCENE_KW = dict(words=(SYNC,), maxd=3, either=True, keep=4)


def types(ev):
    return [(NAMES[e[0]], e[1]) for e in ev]


# ---- names, sizes, create ---------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runbatch_names(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    for name in ("SEARCH", "RECEIVE", "SLOT", "OVER_RUNS", "OVER_EVENTS", "IN_RUNSYNC", "IN_OUT_OF_STEP", "IN_BAD_RUNS", "IN_BAD_EVENTS"):
        m = re.search(r"#define MFM_RUNBATCH_%s (\d+)u" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNBATCH_" + name), name
    own = open(os.path.join(ROOT, "tsl-sdr_amd", "csrc", "mfm_runbatch.h")).read()
    assert re.search(r"#define MFM_RUNBATCH_FRAME %du" % FRAME, own) and b.RUNBATCH_FRAME == FRAME
    assert "static_assert" in own and "struct mfm_runsync_run has the field layout of struct mfm_runrs_run" in own
    assert "pager/pager_pocsag.c:468-538" in src
    assert pkg.RunBatch is b.RunBatch and pkg.hosttwin_runbatch_call is b.hosttwin_runbatch_call and pkg.RUNBATCH_EVENT_DTYPE is b.RUNBATCH_EVENT_DTYPE
    assert pkg.hosttwin_runbatch_state is b.hosttwin_runbatch_state and pkg.runbatch_to_pocsag_events is b.runbatch_to_pocsag_events
    for name in ("behind", "process_device", "fetch", "device_view", "capacity", "fetch_state", "store_state", "close"):
        assert callable(getattr(pkg.RunBatch, name)), name
    assert re.search(r"#define MFM_ABI_VERSION 4\b", src)   # a pure addition, as the sync stage was


def test_struct_sizes_match_the_dtypes(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    for struct_name, dt, size in (("mfm_runbatch_event", b.RUNBATCH_EVENT_DTYPE, 176), ("mfm_runbatch_state", b.RUNBATCH_STATE_DTYPE, 120)):
        m = re.search(r"struct %s \{(.*?)\};" % struct_name, src, flags=re.S)
        fields = re.findall(r"(uint\d+_t)\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
        assert [n for _, n, _ in fields] == list(dt.names), struct_name
        width = {"uint64_t": 8, "uint32_t": 4}
        assert sum(width[t] * int(k or 1) for t, _, k in fields) == size == dt.itemsize, struct_name
        assert re.search(r"struct %s \{\s+/\* %d bytes \*/" % (struct_name, size), src), struct_name
    m = re.search(r"struct mfm_runbatch_config \{(.*?)\};", src, flags=re.S)
    fields = [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+)(?:\[8\])?;", m.group(1))]
    assert fields == [f[0] for f in b.RunBatchConfig._fields_] and C.sizeof(b.RunBatchConfig) == 72
    # the sync stage's run record is read through the burst resampler's
    assert [b.RUNSYNC_RUN_DTYPE.fields[n][1] for n in b.RUNSYNC_RUN_DTYPE.names] == [b.RUNRS_RUN_DTYPE.fields[n][1] for n in b.RUNRS_RUN_DTYPE.names]


REFUSALS = [
    (dict(abi_version=3), "abi_version"),
    (dict(nr_channels=0), "nr_channels"),
    (dict(words=[]), "nr_words must be 1 .. 8"),
    (dict(words=[SYNC] * 9), "nr_words must be 1 .. 8"),
    (dict(keep_distance=16), "keep_distance must be at most 15"),
    (dict(word_mask=2), "word_mask must hold no bit at or above nr_words"),
    (dict(words=[SYNC, OTHER], word_mask=4), "word_mask must hold no bit at or above nr_words"),
    (dict(flags=1), "flags must be 0"),
    (dict(max_runs=0), "max_runs must be"),
    (dict(max_decisions=0), "max_decisions"),
    (dict(max_runs=1 << 28), "max_runs must be"),
    (dict(max_decisions=1 << 31), "max_decisions"),
    (dict(max_events=1 << 31), "max_events"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_with_a_message(pkg, change, message):
    """every refusal of mfm_runbatch_create is decided before a device is looked for; the twin refuses the same"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_decisions=10000, words=[SYNC])
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunBatch(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)
    if kw["nr_channels"]:
        tw = {k: v for k, v in kw.items() if k != "nr_channels"}
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(kw["nr_channels"]), np.zeros(0, b.RUNSYNC_RUN_DTYPE), np.zeros(0, np.uint32),
                                     np.zeros(0, b.RUNSYNC_EVENT_DTYPE), **tw)
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def good_state(pkg):
    st = pkg.binding.hosttwin_runbatch_state(4)
    kept = np.zeros(17, np.uint32)
    st[1] = (7, 500, 510, 1, SEARCH, 0, 0, 0, 0, kept, 0)
    kept[0] = 0x1F
    st[2] = (9, 105, 100, 1, RECEIVE, 1, 1, 5, 0, kept, 0)
    kept[:] = M32
    kept[16] = 1
    st[3] = (9, 1513, 1000, 1, SLOT, 0, 0, 513, 0, kept, 0)
    return st


STATE_REFUSALS = [
    (1, dict(has_stretch=2), "has_stretch must be 0 or 1"),
    (1, dict(has_stretch=0), "has_stretch is 0 but another field is not 0"),
    (1, dict(reserved=1), "reserved and reserved2 must be 0"),
    (2, dict(reserved2=1), "reserved and reserved2 must be 0"),
    (1, dict(decs=1 << 62), "decs and stretch_window must be below 2^62"),
    (1, dict(stretch_window=1 << 62), "decs and stretch_window must be below 2^62"),
    (1, dict(mode=3), "mode must be MFM_RUNBATCH_SEARCH, _RECEIVE or _SLOT"),
    (1, dict(mark=532), "mark must be at most decs + 31 in SEARCH"),
    (1, dict(word_index=1), "nr_kept, kept, word_index and inverted must be 0 in SEARCH"),
    (1, dict(nr_kept=1), "nr_kept, kept, word_index and inverted must be 0 in SEARCH"),
    (2, dict(nr_kept=6), "nr_kept must be decs - mark"),
    (2, dict(mark=0, nr_kept=105), "nr_kept must be decs - mark"),
    (2, dict(mark=106), "nr_kept must be decs - mark"),
    (2, dict(mode=SLOT), "nr_kept must be below 512 in RECEIVE and 512 .. 543 in SLOT"),
    (3, dict(mode=RECEIVE), "nr_kept must be below 512 in RECEIVE and 512 .. 543 in SLOT"),
    (3, dict(decs=1544, nr_kept=544), "nr_kept must be below 512 in RECEIVE and 512 .. 543 in SLOT"),
    (2, dict(word_index=8), "word_index must be at most 7 and inverted 0 or 1"),
    (2, dict(inverted=2), "word_index must be at most 7 and inverted 0 or 1"),
    (2, dict(kept0=0x3F), "kept must hold no bit at or above bit nr_kept"),
    (3, dict(kept16=3), "kept must hold no bit at or above bit nr_kept"),
]


@pytest.mark.parametrize("chan,change,message", STATE_REFUSALS, ids=[str(i) for i in range(len(STATE_REFUSALS))])
def test_state_check_names_channel_and_field(pkg, chan, change, message):
    b = pkg.binding
    st = good_state(pkg)
    b.hosttwin_runbatch_state_check(st)
    for k, v in change.items():
        if k.startswith("kept"):
            st["kept"][chan][int(k[4:])] = v
        else:
            st[k][chan] = v
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runbatch_state_check(st)
    assert ei.value.code == b.MFM_E_INVAL and f"burst batch state, channel {chan}: " + message in str(ei.value), str(ei.value)


# ---- the twin against the restatement -----------------------------------------------------------------------------

def test_the_scene_is_what_it_is_meant_to_be(pkg, ora):
    lines, cuts = scene(pkg)
    w = Want(pkg, ora, lines, **SCENE_KW)
    x, b, sev, bev = w.st[(0, 5)]
    assert types(bev) == [("FOUND", 103), ("BATCH", 615), ("KEPT", 647), ("BATCH", 1159), ("LOST", 1191), ("FOUND", 1223), ("BATCH", 1735),
                          ("LOST", 1767)]
    assert [(e[0], e[3]) for e in sev] == [(103, 0), (300, 0), (647, 0), (1223, 0)]      # 300: inside the first batch, ignored
    assert bev[1][6] != 0 and bev[1][5] == next(z for z in range(16) if (bev[1][6] >> z) & 1)   # the planted word broke codewords
    assert bev[3][6] == 0 and bev[3][5] == 16 and all(e[4] == 0 for e in bev)
    x, b, sev, inv = w.st[(1, 9)]
    assert types(inv) == [("FOUND", 70), ("BATCH", 582), ("KEPT", 614), ("BATCH", 1126), ("LOST", 1158)]
    assert [(e[0], e[3]) for e in sev] == [(70, 1), (267, 1), (614, 1), (1189, 0)]       # 1189 = p + 574: ignored
    assert all(e[4] == 1 for e in inv) and inv[0][2] == ~SYNC & M32 and inv[2][2] == SYNC
    for i in (1, 3):   # the inverted transmission's batches equal the upright one's
        assert inv[i][5:] == bev[i][5:] and inv[i][7] != Z16
    # a sync word on p + 575 is taken, one on p + 574 is not
    assert bev[4][1] + 32 == bev[5][1] == 648 + 575 and inv[4][1] + 31 == 1189 == 615 + 574
    assert types(w.st[(1, 40)][3]) == [("FOUND", 83), ("BATCH", 595), ("KEPT", 627)] and 628 < 900 < 628 + 512     # ends inside a batch
    assert types(w.st[(1, 77)][3]) == [("FOUND", 93), ("BATCH", 605)] and 606 <= 620 < 638                        # ends inside a slot
    assert w.st[(2, 3)][2] == [] and w.st[(2, 3)][3] == []                                                        # idle
    assert all((xx != 0).all() for line in lines for _, xx in line)
    for name, cut in cuts.items():
        assert [[sum(k) for k in row] for row in cut] == [[3000], [1400, 900, 620], [800]], name


@pytest.mark.parametrize("cut", ["ragged", "three", "whole"])
def test_hosttwin_equals_the_restatement_however_the_stream_is_cut(pkg, ora, cut):
    """the scene in runs that end on every seam of a frame (in front of and behind p, the batch's last decision, the slot's), in
    three calls and in one: every call against the restatement, event by event, and the state as bytes"""
    b = pkg.binding
    lines, cuts = scene(pkg)
    want, state = Want(pkg, ora, lines, **SCENE_KW), b.hosttwin_runbatch_state(3)
    calls = trs.schedule(pkg, lines, cuts[cut])
    assert len(calls) == dict(ragged=17, three=3, whole=1)[cut]
    seen = []
    for i, (mruns, _) in enumerate(calls):
        sync, w = want.call(mruns)
        got = b.hosttwin_runbatch_call(state, *sync, **twin_kw(want))
        same(got, w, f"{cut}: call {i}")
        assert state.tobytes() == want.state.tobytes(), (cut, i)
        b.hosttwin_runbatch_state_check(state)
        seen += [(int(e["channel"]), int(e["stretch_window"]), int(e["type"]), int(e["dec"])) for e in got]
    assert len(seen) == 8 + 5 + 3 + 2 and sorted(seen) == sorted((c, fw, e[0], e[1]) for (c, fw), v in want.st.items() for e in v[3])


_HAND = {}


def handover(pkg, ora):
    if not _HAND:
        rng = np.random.RandomState(19)
        x = noise(rng, 1200)
        put(x, 10, transmission(pkg, random_batches(pkg, rng, 2)))      # FOUND 73, BATCH 585, KEPT 617, BATCH 1129, LOST 1161
        _HAND["it"] = x
    return _HAND["it"]


def test_the_handover_is_right_at_every_decision(pkg, ora):
    """one transmission cut into two calls at every k from two decisions before the sync word to two behind the LOST: the events,
    their run fields and the final state are the same each time, and the state between the calls is the restatement's"""
    b = pkg.binding
    x = handover(pkg, ora)
    lines = [[(4, x)]]
    want = Want(pkg, ora, lines)
    whole = want.st[(0, 4)][3]
    assert types(whole) == [("FOUND", 73), ("BATCH", 585), ("KEPT", 617), ("BATCH", 1129), ("LOST", 1161)]
    final = None
    for k in range(73 - 31 - 2, 1161 + 3):
        state = b.hosttwin_runbatch_state(1)
        evs = []
        for i, (mruns, _) in enumerate(trs.schedule(pkg, lines, [[[k, x.size - k]]])):
            sync, w = want.call(mruns)
            got = b.hosttwin_runbatch_call(state, *sync, **twin_kw(want))
            same(got, w, f"k = {k}: call {i}")
            assert state.tobytes() == want.state.tobytes(), (k, i)
            evs += [(int(e["type"]), int(e["dec"]), int(e["run"]), i) for e in got]
        assert [(t, d) for t, d, _, _ in evs] == [(e[0], e[1]) for e in whole], k
        assert all(r == 0 and i == (0 if d < k else 1) for _, d, r, i in evs), k      # the call that holds decision dec reports it
        final = final or state.tobytes()
        assert state.tobytes() == final, k


def test_bch_verdicts_equal_the_oracles(pkg, ora):
    """words with 0, 1, 2 and 3 flipped bits at fixed seeded positions: corrected, fail_mask and nr_ok are the oracle's; a failure in
    word 0 gives nr_ok 0, no failure 16"""
    b = pkg.binding
    rng = np.random.RandomState(29)
    batches = random_batches(pkg, rng, 4)
    x = noise(rng, 64 + 4 * FRAME + 40)
    put(x, 0, transmission(pkg, batches))
    p = 64

    def triple(frame, z):
        at = p + frame * FRAME + 32 * z
        for c in tp._uncorrectable_triple(ora, bits_of(x), at):
            flip(x, at + c)

    for z in range(16):          # the first batch: z % 4 flips in word z, among them triples the decoder gives up on or miscorrects
        for k in rng.choice(31, z % 4, replace=False):
            flip(x, p + 32 * z + int(k))
    triple(1, 0)                 # the second: word 0 fails
    flip(x, p + 2 * FRAME + 32 * 5 + 3)    # the third: one and two flips, all corrected
    flip(x, p + 2 * FRAME + 32 * 9 + 30)
    flip(x, p + 2 * FRAME + 32 * 9 + 0)
    triple(3, 7)                 # the fourth: words 7 and 15 fail
    triple(3, 15)
    want = Want(pkg, ora, [[(2, x)]])
    mruns = trs.make_runs(pkg, [(0, x.size, True, 0, 2, 0)])
    sync, w = want.call(mruns)
    got = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, **twin_kw(want))
    same(got, w, "the four batches")
    bat = got[got["type"] == BATCH]
    assert bat.size == 4
    for e, words in zip(bat, batches):
        fixed = [ora.bch3121_decode(int(r) & 0x7FFFFFFF) for r in e["raw"]]
        assert [int(c) for c in e["corrected"]] == [f[1] for f in fixed]
        assert int(e["fail_mask"]) == sum(1 << z for z in range(16) if fixed[z][0])
        assert int(e["nr_ok"]) == next((z for z in range(16) if fixed[z][0]), 16)
    assert int(bat[0]["fail_mask"]) & 0x7777 == 0 and [int(c) for c in bat[0]["corrected"][:3]] == [w_ & 0x7FFFFFFF for w_ in batches[0][:3]]
    assert (int(bat[1]["nr_ok"]), int(bat[1]["fail_mask"]) & 1) == (0, 1)
    assert (int(bat[2]["nr_ok"]), int(bat[2]["fail_mask"])) == (16, 0) and [int(c) for c in bat[2]["corrected"]] == [w_ & 0x7FFFFFFF for w_ in batches[2]]
    assert (int(bat[3]["nr_ok"]), int(bat[3]["fail_mask"])) == (7, (1 << 7) | (1 << 15))


def test_word_mask_chooses_the_words_that_start_a_transmission(pkg, ora):
    """two words in the table: with word_mask 2 a sync event of word 0 is passed over and the next of word 1 is taken, with
    word_mask 1 the other way round; the slot is held against the word that was found"""
    b = pkg.binding
    rng = np.random.RandomState(31)
    x = noise(rng, 1500)
    trs.plant(x, 100, OTHER)
    trs.plant(x, 400, SYNC)
    trs.plant(x, 400 + FRAME, SYNC)
    for mask, first, n_ev in ((0, (100, 0), 6), (1, (100, 0), 3), (2, (400, 1), 5), (3, (100, 0), 6)):
        want = Want(pkg, ora, [[(1, x)]], words=(OTHER, SYNC), word_mask=mask)
        sync, w = want.call(trs.make_runs(pkg, [(0, x.size, True, 0, 1, 0)]))
        got = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, **twin_kw(want))
        same(got, w, f"mask {mask}")
        assert (int(got[0]["dec"]), int(got[0]["word_index"])) == first and got.size == n_ev, mask
    assert [(NAMES[int(e["type"])], int(e["dec"]), int(e["word_index"])) for e in got] == \
        [("FOUND", 100, 0), ("BATCH", 612, 0), ("LOST", 644, 0), ("FOUND", 944, 1), ("BATCH", 1456, 1), ("LOST", 1488, 1)]
    assert [NAMES[int(t)] for t in b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, words=[OTHER, SYNC], word_mask=2)["type"]] == \
        ["FOUND", "BATCH", "KEPT", "BATCH", "LOST"]


# ---- the second yardstick: the reference decoder's oracle ---------------------------------------------------------

_ORA = {}


def oracle_scene(pkg, ora):
    """one stretch: a transmission of two batches (some words with flipped bits), noise in its second slot, noise, then a sync
    word and a third batch.  The oracle's events when every decision is held for 16 samples"""
    if not _ORA:
        rng = np.random.RandomState(37)
        batches = random_batches(pkg, rng, 3)
        x = noise(rng, 2600)
        put(x, 100, transmission(pkg, batches[:2], pre=64))       # the sync word ends at 195
        for at in (196 + 32 * 3 + 5, 196 + 32 * 3 + 17, 196 + FRAME + 32 * 11 + 2):
            flip(x, at)
        for c in tp._uncorrectable_triple(ora, bits_of(x), 196 + FRAME + 32 * 6):
            flip(x, 196 + FRAME + 32 * 6 + c)
        put(x, 1500, transmission(pkg, batches[2:], pre=64))
        pcm = np.repeat(np.where(x > 0, 8000, -8000).astype(np.int16), 16)
        ev, _ = ora.Pocsag().feed(np.concatenate([pcm, np.zeros(4000, np.int16)]))
        _ORA["it"] = (x, ev)
    return _ORA["it"]


def test_the_oracle_alone_sees_the_scene(pkg, ora):
    x, ev = oracle_scene(pkg, ora)
    t = [int(v) for v in ev["type"]]
    assert all(int(v) == 2400 for v in ev["baud"]), sorted(set(int(v) for v in ev["baud"]))
    assert t.count(BATCH) >= 2 and t.count(KEPT) >= 1
    assert any(t[i] == LOST and t[i + 1] == FOUND for i in range(len(t) - 1)), t
    assert (x != 0).all()


def test_the_stage_equals_the_reference_decoders_oracle(pkg, ora):
    """the decisions of a stretch, each held for 16 samples, through the reference decoder's oracle (its 2400-baud detector fires
    once per sync word); sync max_distance 4, keep_distance 4, upright polarity: the sequence of types and every BATCH's raw,
    corrected, nr_ok and fail_mask are the oracle's.  Sample numbers are not compared"""
    b = pkg.binding
    x, ev = oracle_scene(pkg, ora)
    want = Want(pkg, ora, [[(0, x)]], maxd=4, keep=4)
    sync, w = want.call(trs.make_runs(pkg, [(0, x.size, True, 0, 0, 0)]))
    got = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, **twin_kw(want))
    same(got, w, "the restatement")
    assert [NAMES[int(t)] for t in got["type"]] == [NAMES[int(t)] for t in ev["type"]]
    gb, ob = got[got["type"] == BATCH], ev[ev["type"] == BATCH]
    assert gb.size == ob.size == 3
    for f in ("raw", "corrected", "nr_ok", "fail_mask"):
        assert np.array_equal(gb[f], ob[f]), f
    assert [int(v) for v in gb["nr_ok"]] == [16, 6, 16]
    for kind in (LOST, KEPT):
        assert [int(v) for v in got[got["type"] == kind]["aux"]] == [int(v) for v in ev[ev["type"] == kind]["aux"]]


# ---- pages ----------------------------------------------------------------------------------------------------------

def test_pages_of_a_planted_alphanumeric_and_numeric_message(pkg, ora):
    """the stage's events through runbatch_to_pocsag_events and the host pager (pager_pocsag_on_events), a fresh one per stretch:
    the planted text"""
    b = pkg.binding
    sy = pkg.synth
    msgs = tp._messages(sy)
    rng = np.random.RandomState(41)
    bits = transmission(pkg, sy.pocsag_batches(msgs), pre=64)
    x = noise(rng, bits.size + 300)
    put(x, 50, bits)
    want = Want(pkg, ora, [[(6, x)]])
    sync, w = want.call(trs.make_runs(pkg, [(0, x.size, True, 0, 6, 0)]))
    got = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, **twin_kw(want))
    same(got, w, "the messages")
    assert int(got[-1]["type"]) == LOST
    pev = b.runbatch_to_pocsag_events(got, 1200)
    assert pev.dtype == b.POCSAG_EVENT_DTYPE and np.array_equal(pev["sample"], got["dec"]) and (pev["baud"] == 1200).all()
    for f in ("type", "channel", "aux", "nr_ok", "fail_mask", "raw", "corrected"):
        assert np.array_equal(pev[f], got[f]), f
    hp = tp.HostPager()
    hp.on_events(pev)
    hp.close()
    pages = [(k, baud, cap, fn, text.rstrip(b"\x00")) for k, baud, cap, fn, text in hp.pages]
    assert pages[0] == (2, 1200, (0x12345 << 3) | 3, 2, b"HELLO MI355X\x04")
    assert pages[1][:4] == (3, 1200, (0x00777 << 3) | 5, 0) and pages[1][4].startswith(b"0123-456 [9]")
    assert pages[2][:4] == (2, 1200, (0x3FFFF << 3) | 0, 3) and pages[2][4].startswith(b"The quick brown fox jumps over the lazy dog 0123456789")
    assert len(pages) == 3


# ---- refusals ---------------------------------------------------------------------------------------------------------

def refusal_case(pkg, ora):
    """two calls on three channels; the second, whose first run continues channel 0 inside a batch, is the one that is varied:
    (want, first call, second call, [(change, message, flags)])"""
    b = pkg.binding
    rng = np.random.RandomState(43)
    a = noise(rng, 1500)
    put(a, 20, transmission(pkg, random_batches(pkg, rng, 2)))      # FOUND 83, BATCH 595, KEPT 627, BATCH 1139, LOST 1171
    trs.plant(a, 1300, SYNC)                                          # FOUND 1300
    c1 = noise(rng, 700)
    put(c1, 0, transmission(pkg, random_batches(pkg, rng, 1), pre=0))  # FOUND 31, BATCH 543, LOST 575
    lines = [[(1, a), (8, noise(rng, 50))], [(4, c1)], [(1, noise(rng, 40))]]
    want = Want(pkg, ora, lines)
    first = trs.make_runs(pkg, [(0, 300, True, 0, 1, 0), (2, 40, True, 0, 1, 300)])
    second = trs.make_runs(pkg, [(0, 1200, False, 300, 1, 0), (0, 50, True, 0, 8, 1200), (1, 700, True, 0, 4, 1250)])
    IN = 8
    R = lambda i, **kw: ("runs", i, kw)
    E = lambda i, **kw: ("events", i, kw)
    cases = [
        (dict(totals=[3, 3, 1, 0]), "the burst sync stage's call raised overflow or an input error", b.MFM_RUNBATCH_IN_RUNSYNC << IN),
        (dict(totals=[3, 3, 0, 4]), "the burst sync stage's call raised overflow or an input error", b.MFM_RUNBATCH_IN_RUNSYNC << IN),
        (dict(edit=R(0, first_dec=299)), "out of step", b.MFM_RUNBATCH_IN_OUT_OF_STEP << IN),
        (dict(edit=R(2, flags=0)), "out of step", b.MFM_RUNBATCH_IN_OUT_OF_STEP << IN),               # channel 1 has no stretch
        (dict(edit=R(2, channel=3)), "not a burst sync stage's", b.MFM_RUNBATCH_IN_BAD_RUNS << IN),
        (dict(edit=R(1, first_dec=5)), "not a burst sync stage's", b.MFM_RUNBATCH_IN_BAD_RUNS << IN),
        (dict(edit=R(1, word_offset=37)), "not a burst sync stage's", b.MFM_RUNBATCH_IN_BAD_RUNS << IN),     # not the running sum
        (dict(edit=R(2, nr_dec=1 << 20)), "not a burst sync stage's", b.MFM_RUNBATCH_IN_BAD_RUNS << IN),      # more words than the capacity
        (dict(totals=[5, 3, 0, 0]), "more runs than max_runs", b.MFM_RUNBATCH_OVER_RUNS),
        (dict(edit=E(0, dec=299)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),            # in front of its run
        (dict(edit=E(1, dec=1500)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),           # behind its run
        (dict(edit=E(2, dec=700)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),
        (dict(edit=E(1, dec=627)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),            # not ascending: 627, 627
        (dict(edit=E(0, word_index=1)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),
        (dict(edit=E(2, inverted=2)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),
        (dict(totals=[3, 2, 0, 0]), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),           # nr_events past the totals
        (dict(edit=R(0, nr_events=1 << 31)), "the sync events are not", b.MFM_RUNBATCH_IN_BAD_EVENTS << IN),
    ]
    return want, first, second, cases


def edited(sync, change):
    """the second call's arrays with one field of one record changed"""
    runs, bits, ev = (a.copy() for a in sync)
    if "edit" in change:
        what, i, kw = change["edit"]
        for k, v in kw.items():
            (runs if what == "runs" else ev)[k][i] = v
    return runs, bits, ev


REFUSAL_CONF = dict(max_runs=4, max_decisions=2000)


def test_hosttwin_refuses_and_leaves_state_and_output(pkg, ora):
    """every flag; each time nothing comes out and the state stays, so the same call fed correctly is right.  max_events goes by
    the count: one below it is refused, the count itself is enough"""
    b = pkg.binding
    want, first, second, cases = refusal_case(pkg, ora)
    state = b.hosttwin_runbatch_state(3)
    sync0, w0 = want.call(first)
    same(b.hosttwin_runbatch_call(state, *sync0, **twin_kw(want, **REFUSAL_CONF)), w0, "call 0")
    s0 = state.copy()
    assert int(s0["mode"][0]) == RECEIVE and int(s0["nr_kept"][0]) == 300 - 84
    sync, w = want.call(second)
    assert sync[2]["dec"].tolist() == [627, 1300, 31] and sync[0]["nr_events"].tolist() == [2, 0, 1]
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runbatch_call(state, *edited(sync, change), totals=change.get("totals"), **twin_kw(want, **REFUSAL_CONF))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value), ei.value.flags)
        assert ei.value.needed == 0 and state.tobytes() == s0.tobytes(), change
    assert [NAMES[int(t)] for t in w["type"]] == ["BATCH", "KEPT", "BATCH", "LOST", "FOUND", "FOUND", "BATCH", "LOST"]
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runbatch_call(state, *sync, max_events=7, **twin_kw(want, **REFUSAL_CONF))
    assert ei.value.code == b.MFM_E_STATE and "events exceed max_events" in str(ei.value) and ei.value.flags == b.MFM_RUNBATCH_OVER_EVENTS
    assert state.tobytes() == s0.tobytes()
    with pytest.raises(pkg.MfmError) as ei:      # the caller's buffer too small
        b.hosttwin_runbatch_call(state, *sync, max_out_events=7, **twin_kw(want, **REFUSAL_CONF))
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == 8 and state.tobytes() == s0.tobytes()
    same(b.hosttwin_runbatch_call(state, *sync, max_events=8, **twin_kw(want, **REFUSAL_CONF)), w, "the same call, right, after the refused ones")
    assert state.tobytes() == want.state.tobytes()


def test_the_default_max_events_is_the_bound(pkg, ora):
    """70 batches back to back in one run: FOUND, 70 BATCH, 69 KEPT and a LOST; the default capacity, 3 (max_decisions / 544) + 5
    max_runs, holds them with max_decisions the run's own length"""
    b = pkg.binding
    x, want = back_to_back(pkg, ora)
    sync, w = want.call(trs.make_runs(pkg, [(0, x.size, True, 0, 2, 0)]))
    assert w.size == 1 + 2 * 70 and w.size <= 3 * (x.size // FRAME) + 5
    got = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(1), *sync, max_runs=1, max_decisions=x.size, **twin_kw(want))
    same(got, w, "70 batches")


_B2B = {}


def back_to_back(pkg, ora):
    if not _B2B:
        rng = np.random.RandomState(47)
        bits = transmission(pkg, random_batches(pkg, rng, 70), pre=1)
        x = noise(rng, bits.size + 40)
        put(x, 0, bits)
        _B2B["it"] = (x, Want(pkg, ora, [[(2, x)]]))
    return _B2B["it"]


# ---- the host code under the sanitizers, the kernels' registers ---------------------------------------------------

def test_hosttwin_is_clean_under_the_address_and_undefined_sanitizers(pkg, ora, tmp_path):
    """tests/hoststub/runbatch_twin_main.cpp, a program of its own built with -fsanitize=address,undefined around the stage's host
    code (and mfm_pocsag.hip, which owns the BCH tables), runs the twin on the ragged cut in buffers of exactly the sizes needed:
    nothing to report, and the restatement's result"""
    b = pkg.binding
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    exe = tmp_path / "runbatch_twin"
    csrc = os.path.join(ROOT, "tsl-sdr_amd", "csrc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "hoststub", "runbatch_twin_main.cpp"),
           os.path.join(csrc, "mfm_runbatch.hip"), os.path.join(csrc, "mfm_pocsag.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    if re.search(r"lib(a|t|ub|l|m)san", env.get("LD_PRELOAD", "")):   # another sanitizer's runtime does not share a process with this one
        del env["LD_PRELOAD"]
    env.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    lines, cuts = scene(pkg)
    want = Want(pkg, ora, lines, **SCENE_KW)
    state_file = tmp_path / "state.bin"
    state_file.write_bytes(b.hosttwin_runbatch_state(3).tobytes())
    total = 0
    for i, (mruns, _) in enumerate(trs.schedule(pkg, lines, cuts["ragged"])):
        (sruns, bits, sev), w = want.call(mruns)
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        words = want.words + [0] * (8 - len(want.words))
        fin.write_bytes(struct.pack("<16I", 3, len(sruns), bits.size, sev.size, 0, len(want.words), *words, want.mask, want.keep)
                        + sruns.tobytes() + bits.tobytes() + sev.tobytes())
        r = subprocess.run([str(exe), str(fin), str(state_file), str(fout)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
        raw = fout.read_bytes()
        ne, = struct.unpack("<Q", raw[:8])
        assert len(raw) == 8 + 176 * ne
        same(np.frombuffer(raw[8:], b.RUNBATCH_EVENT_DTYPE), w, f"call {i}")
        total += ne
    assert state_file.read_bytes() == want.state.tobytes() and total == 18


def test_runbatch_kernels_use_no_scratch(pkg):
    """the code object's notes of build/mfm_runbatch.o (tools/kernel_regs.py): the five kernels, no private segment, no spilled
    register, at most 128 VGPRs"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runbatch.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"rbt_{k}_kernel" for k in ("plan", "walk", "scan", "decode", "state")), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _fed(pkg, torch, rb, sync, totals=None):
    """one call from uploaded arrays: a burst sync call's result as it would stand in its device view"""
    runs, bits, ev = sync
    t = np.array([len(runs), ev.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, bits if bits.size else np.zeros(1, np.uint32)),
            tr._up(torch, ev if ev.size else np.zeros(1, ev.dtype)), tr._up(torch, t))
    rb.process_device(*(k.data_ptr() for k in keep))
    try:
        return rb.fetch()
    finally:
        del keep


def _device_totals(rb):
    return tl._d2h(rb.device_view()[1], 32).view(np.uint64).tolist()


def _make(pkg, nch, max_runs, max_dec, want, **kw):
    return pkg.RunBatch(nch, max_runs, max_dec, want.words, word_mask=want.mask, keep_distance=want.keep, **kw)


def _both(pkg, torch, rb, want, twin, mruns, what):
    """one call on the device against the restatement, the twin, the twin's state bytes and the device view"""
    b = pkg.binding
    sync, w = want.call(mruns)
    got = _fed(pkg, torch, rb, sync)
    same(got, w, what)
    same(b.hosttwin_runbatch_call(twin, *sync, **twin_kw(want)), got, what + ": the twin")
    assert rb.fetch_state().tobytes() == twin.tobytes() == want.state.tobytes(), what
    assert _device_totals(rb) == [w.size, len(mruns), 0, 0], what
    if got.size:
        assert tl._d2h(rb.device_view()[0], got.nbytes).tobytes() == got.tobytes(), what
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["ragged", "three", "whole"])
def test_gpu_equals_twin_and_restatement_on_the_seam_scene(pkg, ora, cut):
    import torch
    b = pkg.binding
    lines, cuts = scene(pkg)
    want, twin = Want(pkg, ora, lines, **SCENE_KW), b.hosttwin_runbatch_state(3)
    rb = _make(pkg, 3, 6, 6800, want)
    assert rb.capacity() == (6, 3 * (6800 // FRAME) + 30)
    n = 0
    for i, (mruns, _) in enumerate(trs.schedule(pkg, lines, cuts[cut])):
        n += _both(pkg, torch, rb, want, twin, mruns, f"{cut}: call {i}").size
    assert n == 18
    rb.close()


@pytest.mark.gpu
def test_gpu_seams_of_the_machine(pkg, ora):
    """frames that start on bit 0, 1 and 31 of a word of their run; a frame carried over a call seam with 1, 31, 32, 511, 512 and
    543 kept bits (511: the batch is completed by the second run's first decision, 512: by the first run's last); runs whose
    word_offset follows a run with nr_dec % 32 != 0"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(53)
    lines, cut = [], []
    for c, (lead, kept) in enumerate([(0, 1), (1, 31), (31, 32), (0, 511), (1, 512), (31, 543), (5, 0), (17, 544)]):
        x = noise(rng, lead + 32 + 2 * FRAME + 60)
        put(x, lead, transmission(pkg, random_batches(pkg, rng, 2), pre=0))      # p = lead + 32
        lines.append([(c + 2, x)])
        cut.append([[lead + 32 + kept, x.size - (lead + 32 + kept)]])
    want, twin = Want(pkg, ora, lines), b.hosttwin_runbatch_state(len(lines))
    calls = trs.schedule(pkg, lines, cut)
    assert len(calls) == 2 and any(int(r["nr_dec"]) % 32 for r in calls[0][0][:-1])
    rb = _make(pkg, len(lines), len(lines), sum(x.size for [(_, x)] in lines), want)
    got = [_both(pkg, torch, rb, want, twin, mruns, f"call {i}") for i, (mruns, _) in enumerate(calls)]
    st = want.state    # what the first call left is checked in _both; the kept counts it went through:
    # 1 + 32 + 511: completed at a run's last decision; the runs that kept 543 and 544 bits had their batch well inside
    assert [int(e["dec"]) for e in got[0] if int(e["type"]) == BATCH] == [1 + 32 + 511, 31 + 32 + 511, 17 + 32 + 511]
    first = [e for e in got[1] if int(e["type"]) == BATCH and int(e["channel"]) == 3][0]       # ... and at a run's first decision
    assert int(first["dec"]) == 0 + 32 + 511 == int(calls[1][0]["first_dec"][3])
    assert sum(1 for e in got[1] if int(e["type"]) == BATCH) == 2 * 8 - 3 and (st["mode"] == SEARCH).all()
    rb.close()


@pytest.mark.gpu
def test_gpu_seventy_batches_back_to_back(pkg, ora):
    """more batches in one run than the decode kernel's block holds, an odd group of them, and the bound on a run's events met"""
    import torch
    b = pkg.binding
    x, want = back_to_back(pkg, ora)
    want.state[:] = 0
    want.cur.clear()
    rb = _make(pkg, 1, 1, x.size, want)
    got = _both(pkg, torch, rb, want, b.hosttwin_runbatch_state(1), trs.make_runs(pkg, [(0, x.size, True, 0, 2, 0)]), "70 batches")
    assert got.size == 141 and rb.capacity() == (1, 3 * (x.size // FRAME) + 5)
    rb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1025, 2049])
def test_gpu_more_runs_than_lanes_waves_and_the_plan_block(pkg, ora, n):
    """one run of 0 .. 40 decisions per channel, four of them of 1200 decisions that hold a transmission; a second call continues
    every third channel, begins every third anew and leaves the rest out"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(n)
    l0 = [(7 * i) % 41 for i in range(n)]
    l1 = [(11 * i + 5) % 41 for i in range(n)]
    big = [3, n // 3 + 1, n // 2, n - 3]
    for c in big:
        l0[c] = 1200
    lines = []
    for c in range(n):
        if c % 3 == 0:
            lines.append([(c % 5, noise(rng, l0[c] + l1[c]))])
        elif c % 3 == 1:
            lines.append([(c % 5, noise(rng, l0[c])), (77, noise(rng, l1[c]))])
        else:
            lines.append([(c % 5, noise(rng, l0[c]))])
    for c in big:
        put(lines[c][0][1], 30 + c % 29, transmission(pkg, random_batches(pkg, rng, 2), pre=0))
    want, twin = Want(pkg, ora, lines), b.hosttwin_runbatch_state(n)
    first, second, off0, off1 = [], [], 0, 0
    for c in range(n):
        first.append((c, l0[c], True, 0, c % 5, off0))
        off0 += l0[c]
        if c % 3 == 0:
            second.append((c, l1[c], False, l0[c], c % 5 + 1, off1))
            off1 += l1[c]
        elif c % 3 == 1:
            second.append((c, l1[c], True, 0, 77, off1))
            off1 += l1[c]
    rb = _make(pkg, n, n, max(off0, off1), want)
    events = 0
    for i, rows in enumerate((first, second)):
        events += _both(pkg, torch, rb, want, twin, trs.make_runs(pkg, rows), f"call {i}").size
    assert events >= 4 * 5
    rb.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state_and_a_state_stored_is_a_state_fetched(pkg, ora):
    """every refusal of the twin's test on the device, with the twin's flags in the totals, and max_events one below the call's
    count; each time nothing comes out and the state stays.  The state then moves mid-batch to a second object (store_state, fetched
    back unchanged; a state that fails is refused with channel and field and changes nothing), where the same input is right"""
    import torch
    b = pkg.binding
    want, first, second, cases = refusal_case(pkg, ora)
    rb = _make(pkg, 3, 4, 2000, want, max_events=7)
    sync0, w0 = want.call(first)
    same(_fed(pkg, torch, rb, sync0), w0, "call 0")
    s0 = rb.fetch_state()
    twin = s0.copy()
    assert int(s0["mode"][0]) == RECEIVE and int(s0["nr_kept"][0]) == 216
    sync, w = want.call(second)
    conf = dict(REFUSAL_CONF, max_events=7)
    for change, message, flags in cases + [(dict(), "events exceed max_events", b.MFM_RUNBATCH_OVER_EVENTS)]:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rb, edited(sync, change), totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == 0
        assert _device_totals(rb) == [0, 0, flags & 0xff, flags >> 8], (change, _device_totals(rb))
        with pytest.raises(pkg.MfmError) as et:
            b.hosttwin_runbatch_call(twin, *edited(sync, change), totals=change.get("totals"), **twin_kw(want, **conf))
        assert et.value.flags == flags and str(et.value).split(": ", 1)[-1] == str(ei.value).split(": ", 1)[-1]
        assert rb.fetch_state().tobytes() == s0.tobytes() == twin.tobytes(), change
    fits = _make(pkg, 3, 4, 2000, want, max_events=8)
    bad = s0.copy()
    bad["nr_kept"][0] = 215
    with pytest.raises(pkg.MfmError) as ei:
        fits.store_state(bad)
    assert ei.value.code == b.MFM_E_INVAL and "channel 0: nr_kept must be decs - mark" in str(ei.value)
    assert not fits.fetch_state().view(np.uint8).any()
    fits.store_state(s0)
    assert fits.fetch_state().tobytes() == s0.tobytes()
    got = _fed(pkg, torch, fits, sync)
    same(got, w, "the same call in an object it fits")
    assert int(got[0]["type"]) == BATCH and int(got[0]["dec"]) == 595    # the batch across the move: 216 of its bits stood in the state
    with pytest.raises(pkg.MfmError) as ei:
        fits.fetch(max_events=7)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == 8
    same(fits.fetch(), w, "fetched again")
    b.hosttwin_runbatch_call(twin, *sync, **twin_kw(want, **dict(conf, max_events=8)))
    assert fits.fetch_state().tobytes() == twin.tobytes() == want.state.tobytes()
    for o in (rb, fits):
        o.close()


def test_chain_scene_holds_a_batch_on_every_transmitting_channel(pkg, ora):
    calls, by = trs._chain_calls(pkg, ora)
    kinds = {c: [] for c in range(trs.CHAIN["nch"])}
    for (c, fw), d in by.items():
        kinds[c] += [e[0] for e in restate(ora, bits_of(d), trs.restate(d, [SYNC])[0], [SYNC])[0]]
    assert all(kinds[c] == [FOUND, BATCH] for c in trs.CHAIN["tx"]) and all(kinds[c] == [] for c in trs.CHAIN["idle"]), kinds


@pytest.mark.gpu
def test_gpu_level_gate_runrs_runmm_runsync_runbatch_on_device_equals_the_chain_through_the_twins(pkg, ora):
    """level -> gate with P = 1 -> burst resampler 4/5 -> burst Mueller-Muller -> burst sync -> burst batch, all on the device
    views of one stream with no fetch in between until the batch stage's own, in ragged calls and the flush (the small shape of
    tests/test_runsync.py's CHAIN): every call against the same chain through the host twins"""
    b = pkg.binding
    sc, s = trs._chain(pkg), trs.CHAIN
    calls, by = trs._chain_calls(pkg, ora)
    rows, cuts, W, P, nch = sc["rows"], sc["cuts"], s["W"], s["P"], s["nch"]
    cap = max(cuts)
    lv = pkg.Level(nch, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=s["hang"])
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    rr = pkg.RunResampler(nch, sc["rtaps"], 4, 5, W, max_in_samples=cap, preroll_windows=P)
    rm = pkg.RunMm.behind(rr, trm.REF["spb"], trm.KW, trm.KM, error_min=trm.REF["emin"], error_max=trm.REF["emax"])
    rs = pkg.RunSync.behind(rm, [SYNC])
    rb = pkg.RunBatch.behind(rs)
    assert rb.capacity() == (rm.capacity()[0], 3 * (rm.capacity()[1] // FRAME) + 5 * rm.capacity()[0])
    tsync, tbatch = b.hosttwin_runsync_state(nch), b.hosttwin_runbatch_state(nch)
    pos, seen = 0, []
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gate.process_host(rows[:, pos:pos + m], lv.process_host(rows[:, pos:pos + m]))
            pos += m
        else:
            gate.flush_device()
        rr.process_device(*gate.device_view())
        rm.process_device(*rr.device_view())
        rs.process_device(*rm.device_view())
        rb.process_device(*rs.device_view())
        got = rb.fetch()
        (_, _), (mruns, mdec) = calls[i]
        sync = b.hosttwin_runsync_call(tsync, mruns, mdec, words=[SYNC])
        trs.same(rs.fetch(), sync, f"the sync call {i}")
        same(b.hosttwin_runbatch_call(tbatch, *sync, words=[SYNC]), got, f"call {i}")
        assert rb.fetch_state().tobytes() == tbatch.tobytes(), i
        seen += [(int(e["channel"]), int(e["stretch_window"]), int(e["type"]), int(e["dec"])) for e in got]
    want = sorted((c, fw, e[0], e[1]) for (c, fw), d in by.items()
                  for e in restate(ora, bits_of(d), trs.restate(d, [SYNC])[0], [SYNC])[0])
    assert sorted(seen) == want and {c for c, _, _, _ in want} == set(s["tx"]) and any(t == BATCH for _, _, t, _ in want)
    for o in (rb, rs, rm, rr, gate, lv):
        o.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------

def as_events(pkg, tuples, c, fw):
    """RUNBATCH_EVENT_DTYPE records of a stretch's restated events"""
    ev = np.zeros(len(tuples), pkg.binding.RUNBATCH_EVENT_DTYPE)
    for i, e in enumerate(tuples):
        ev[i] = (e[0], c, 0, e[2], e[3], e[4], e[5], e[6], fw, e[1], e[7], e[8])
    return ev


def _tool_batches(pkg, ora, words=(SYNC,), maxd=3, keep=4):
    """{(channel, first window): restated events} of the tool scene of tests/test_runmm.py, and the pages a fresh host pager per
    stretch makes of them at 2400 baud"""
    by = trm.tool_want(pkg, ora)
    W = trm.trp.CHAIN["W"]
    evs, pages = {}, []
    for (c, fw), d in sorted(by.items()):
        evs[(c, fw)] = restate(ora, bits_of(d), trs.restate(d, list(words), maxd)[0], list(words), keep)[0]
        hp = tp.HostPager()
        hp.on_events(pkg.binding.runbatch_to_pocsag_events(as_events(pkg, evs[(c, fw)], c, fw), 2400))
        hp.close()
        pages += [(c, fw * W, kind, baud, cap, fn, text) for kind, baud, cap, fn, text in hp.pages]
    return evs, pages, by


def _tool_lines(out_dir, words=("7cd215d8",)):
    lines = [json.loads(ln) for ln in (out_dir / "batch.jsonl").read_text().splitlines()]
    assert all(set(ln) - {"corrected"} == {"channel", "first_window", "first_sample", "type", "dec", "aux", "word", "inverted", "nr_ok", "fail_mask"}
               for ln in lines)
    assert all(("corrected" in ln) == (ln["type"] == BATCH) and ln["word"] in words for ln in lines)
    got = sorted((ln["channel"], ln["first_window"], ln["type"], ln["dec"], int(ln["aux"], 16), ln["inverted"], ln["nr_ok"], ln["fail_mask"],
                  tuple(int(w, 16) for w in ln.get("corrected", []))) for ln in lines)
    text = {3: " ", 4: " ", 0x17: " ", 8: "<BKSP>", 12: "<FF>"}
    pages = [json.loads(ln) for ln in (out_dir / "pages.jsonl").read_text().splitlines()]
    return got, sorted((p["channel"], p["first_sample"], {"alphanumeric": 2, "numeric": 3}[p["type"]], p["baud"], p["capCode"], p["function"],
                        p["message"]) for p in pages), text


def _tool_compare(pkg, ora, out_dir, evs, pages):
    got, got_pages, text = _tool_lines(out_dir)
    want = sorted((c, fw, e[0], e[1], e[2], e[4], e[5], e[6], e[8] if e[0] == BATCH else ()) for (c, fw), v in evs.items() for e in v)
    assert got == want
    assert got_pages == sorted((c, first, kind, baud, cap, fn, "".join(text.get(ch, chr(ch)) for ch in t)) for c, first, kind, baud, cap, fn, t in pages)


def test_tool_scene_holds_batches_and_pages(pkg, ora):
    evs, pages, by = _tool_batches(pkg, ora)
    kinds = [e[0] for v in evs.values() for e in v]
    assert kinds.count(BATCH) >= 2 and kinds.count(FOUND) >= 2 and {c for (c, _), v in evs.items() if v} == {0, 1}
    assert len(pages) >= 1


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_batch_writes_the_events_and_pages_of_the_restatement(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-mm 16 --gate-sync 0x7CD215D8/3 --gate-batch 4,2400 as a fresh child process on the chain scene
    of tests/test_runpocsag.py: batch.jsonl holds the restatement's events and pages.jsonl the pages a host pager per stretch makes
    of them; the files the command writes without --gate-batch are byte-identical"""
    base = trm.tool_setup(pkg, ora, tmp_path)
    evs, pages, by = _tool_batches(pkg, ora)
    common = ["--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-mm", "16", "--gate-sync", "0x7CD215D8/3"]
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "with")] + common + ["--gate-batch", "4,2400"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "without")] + common, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _tool_compare(pkg, ora, tmp_path / "with", evs, pages)
    names = sorted(p.name for p in (tmp_path / "without").iterdir())
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == sorted(names + ["batch.jsonl", "pages.jsonl"])
    for name in names:
        assert (tmp_path / "with" / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), name


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_a_batch_object_in_an_mm_route(pkg, ora, tmp_path):
    """a route of stage mm that carries "sync" and "batch": DIR/<name>/batch.jsonl and pages.jsonl as --gate-batch writes them, with
    the configuration's channel numbers"""
    base = trm.tool_setup(pkg, ora, tmp_path)
    evs, pages, by = _tool_batches(pkg, ora)
    doc = {"local": True, "routes": [{"name": "sym", "stage": "mm", "resample": "4/5", "taps": str(tmp_path / "filter.json"), "channels": [0, 1],
                                      "mm": {"spb": 16}, "sync": {"words": [SYNC], "distance": 3}, "batch": {"keep": 4, "baud": 2400}}]}
    (tmp_path / "routes.json").write_text(json.dumps(doc))
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "routed"), "--gate-route", str(tmp_path / "routes.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _tool_compare(pkg, ora, tmp_path / "routed" / "sym", evs, pages)
    trm.tool_check(tmp_path / "routed" / "sym", by, trm.trp.CHAIN["W"])


BATCH_REFUSALS = [
    (dict(batch={"keep": 4}), "\"batch\" needs \"sync\""),
    (dict(sync={"words": [SYNC]}, batch={"keep": 16}), "\"batch\" must be an object with optionally keep (0 .. 15) and baud"),
    (dict(sync={"words": [SYNC]}, batch={"keep": 4, "baud": 0}), "\"batch\" must be an object with optionally keep (0 .. 15) and baud"),
    (dict(sync={"words": [SYNC]}, batch={"distance": 4}), "\"batch\" must be an object with optionally keep (0 .. 15) and baud"),
    (dict(sync={"words": [SYNC]}, batch=4), "\"batch\" must be an object with optionally keep (0 .. 15) and baud"),
    (dict(stage="pocsag", batch={"keep": 4}), "\"batch\" belongs to stage mm, not to stage pocsag"),
]


@pytest.mark.parametrize("change,message", BATCH_REFUSALS, ids=[str(i) for i in range(len(BATCH_REFUSALS))])
def test_level_scan_tool_refuses_a_bad_batch_object_and_flag(tmp_path, change, message):
    """what is wrong with a route's "batch" object or with --gate-batch ends the run with a message before anything is set up"""
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
    rs = ["--gate-resample", "4/5", "--resample-taps", "f.json", "--gate-mm", "16"]
    for flags, text in ((rs + ["--gate-batch"], "--gate-batch needs --gate-sync"),
                        (rs + ["--gate-batch", "4"], "--gate-batch needs --gate-sync"),
                        (rs + ["--gate-sync", "0x7CD215D8", "--gate-batch", "four"], "--gate-batch takes [KEEP[,BAUD]]"),
                        (rs + ["--gate-sync", "0x7CD215D8", "--gate-batch", "16"], "keep (0 .. 15)"),
                        (rs + ["--gate-sync", "0x7CD215D8", "--gate-batch", "4,0"], "baud (1 .. 65535)")):
        r = subprocess.run(tool + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and text in r.stderr, (flags, r.stderr[-2000:])
    assert not (tmp_path / "out").exists()
