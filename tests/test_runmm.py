"""The burst Mueller-Muller stage (mfm_runmm_*, csrc/mfm_runmm.hip): the runs the burst resampler left go through the clock
recovery loop, one fresh loop per stretch.

The expected result is the oracle's, never the code under test: a fresh oracle_lib.MuellerMuller (oracle/pocsag_oracle.c's
restatement of pager/mueller_muller.c) per stretch, fed run by run, and where a chain stands in front the restated level and gate
(tests/test_level.py, test_gate_preroll.py) and the oracle resampler per stretch (test_runrs.Checker).  Every comparison is an
equality of every field of every run record and of every decision."""
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
import test_gate_preroll as tgp
import test_level as tl
import test_runpocsag as trp
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runmm_create", "mfm_runmm_destroy", "mfm_runmm_process_device", "mfm_runmm_fetch", "mfm_runmm_device_view",
             "mfm_runmm_fetch_state", "mfm_runmm_store_state", "mfm_hosttwin_runmm_call", "mfm_hosttwin_runmm_state_check"]
KW, KM = 0.0001, 0.000004                              # pager/test/test_mueller_muller.c:85-88, as tests/test_mueller_muller.py
SPB = np.float32(25000.0) / np.float32(1200.0)
MARGIN = np.float32(0.05)
REF = dict(kw=KW, km=KM, spb=float(SPB), emin=float(SPB - MARGIN), emax=float(SPB + MARGIN))
# a loop whose steps leave any small window: |km| * 32768 = 16.4 samples either way, and kw * w_error reaches several samples on
# full-scale input, so the clamp is hit on both sides
WILD = dict(kw=KW, km=0.0005, spb=float(SPB), emin=float(SPB - MARGIN), emax=float(SPB + MARGIN))
U = 512                                                # the walk's staging unit (MFM_RUNMM_STAGING_UNIT, csrc/mfm_runmm.h)
SYNC = 0x7CD215D8


def min_step(par):
    """s = floor(error_min - |km| * 32768) in float: no step is shorter"""
    return int(np.floor(np.float32(par["emin"]) - np.abs(np.float32(par["km"])) * np.float32(32768.0)))


def slots(nr_out, s):
    return int(nr_out) // s + 1


def twin_kw(par, **more):
    return dict(samples_per_bit=par["spb"], kw=par["kw"], km=par["km"], error_min=par["emin"], error_max=par["emax"], **more)


def make_runs(pkg, rows):
    """RUNRS_RUN_DTYPE from (channel, nr_out, begins, first_out, first_window, out_offset)"""
    runs = np.zeros(len(rows), pkg.binding.RUNRS_RUN_DTYPE)
    for i, (c, n, begins, fo, fw, off) in enumerate(rows):
        runs[i] = (fw, off, fo, c, n, 1 if begins else 0, 0)
    return runs


# ---- the checker --------------------------------------------------------------------------------------------

class Checker:
    """what the stage must return for the burst resampler's calls of one stream, from the oracle"""

    def __init__(self, pkg, ora, par):
        self.pkg, self.ora, self.par = pkg, ora, par
        self.chan = {}     # channel -> [oracle loop, key of the stretch, decisions so far]
        self.by = {}       # (channel, first window) -> decisions by run
        self.pcm = {}      # (channel, first window) -> resampled pieces

    def fresh(self):
        p = self.par
        return self.ora.MuellerMuller(p["kw"], p["km"], p["spb"], p["emin"], p["emax"])

    def call(self, runs, payload):
        out = np.zeros(len(runs), self.pkg.binding.RUNMM_RUN_DTYPE)
        parts, off = [], 0
        for i, r in enumerate(runs):
            c, n = int(r["channel"]), int(r["nr_out"])
            if int(r["flags"]) & 1:
                key = (c, int(r["first_window"]))
                self.chan[c] = [self.fresh(), key, 0]
                self.by[key], self.pcm[key] = [], []
            st = self.chan[c]
            y = payload[int(r["out_offset"]):int(r["out_offset"]) + n]
            # the sample behind the piece is never asked for (an index is below the length); a zero stands there
            d = st[0].process(np.concatenate([y, np.zeros(1, np.int16)]), 0, n) if n else np.zeros(0, np.int16)
            out[i] = (int(r["first_window"]), off, st[2], c, d.size, int(r["flags"]) & 1, 0)
            st[2] += d.size
            off += d.size
            parts.append(d)
            self.by[st[1]].append(d)
            self.pcm[st[1]].append(y)
        return out, (np.concatenate(parts) if parts else np.zeros(0, np.int16))

    def stretches(self):
        """{(channel, first window): decisions}; each stretch once more through a fresh loop in one piece"""
        out = {}
        for key, ds in self.by.items():
            d = np.concatenate(ds) if ds else np.zeros(0, np.int16)
            y = np.concatenate(self.pcm[key] + [np.zeros(1, np.int16)])
            whole = self.fresh().process(y, 0, y.size - 1) if y.size > 1 else np.zeros(0, np.int16)
            assert np.array_equal(whole, d), key
            out[key] = d
        return out


def same(got, want, what):
    (gr, gd), (wr, wd) = got, want
    assert gr.dtype == wr.dtype and gr.shape == wr.shape, (what, gr.shape, wr.shape)
    for f in gr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert bad.size == 0, f"{what}: run field {f} differs at {bad[:5].tolist()}: {gr[f][bad[0]]} != {wr[f][bad[0]]}"
    assert gd.dtype == np.int16 and gd.shape == wd.shape, (what, gd.shape, wd.shape)
    bad = np.flatnonzero(gd != wd)
    assert bad.size == 0, f"{what}: decisions differ from {bad[:5].tolist()} on"
    # consistent in itself: dense, ascending, no gaps
    assert np.array_equal(gr["dec_offset"], np.cumsum(gr["nr_dec"], dtype=np.uint64) - gr["nr_dec"]) and int(gr["nr_dec"].sum()) == gd.size, what


def cut_stream(pkg, timelines, edges):
    """the burst resampler's calls of a stream: timelines[c] = [(first window, samples int16)] are channel c's stretches one behind
    the other, and call k takes what lies in [edges[k], edges[k + 1]) of every channel's line, a run per stretch it touches"""
    calls = []
    for t0, t1 in zip(edges[:-1], edges[1:]):
        rows, pieces, off = [], [], 0
        for c, line in enumerate(timelines):
            at = 0
            for fw, x in line:
                lo, hi = max(t0, at), min(t1, at + x.size)
                if lo < hi:
                    rows.append((c, hi - lo, lo == at, lo - at, fw, off))
                    pieces.append(x[lo - at:hi - at])
                    off += hi - lo
                at += x.size
        calls.append((make_runs(pkg, rows), np.concatenate(pieces) if pieces else np.zeros(0, np.int16)))
    return calls


def by_stretch(calls_out):
    """{(channel, first window): decisions} of a list of ((runs in), (runs out, decisions))"""
    out, cur = {}, {}
    for rin, (rout, dec) in calls_out:
        for a, o in zip(rin, rout):
            c = int(a["channel"])
            if int(a["flags"]) & 1:
                cur[c] = (c, int(a["first_window"]))
                out[cur[c]] = []
            assert int(o["first_dec"]) == sum(x.size for x in out[cur[c]])
            out[cur[c]].append(dec[int(o["dec_offset"]):int(o["dec_offset"]) + int(o["nr_dec"])])
    return {k: (np.concatenate(v) if v else np.zeros(0, np.int16)) for k, v in out.items()}


def _timelines(seed=5):
    rng = np.random.RandomState(seed)
    lens = [[3000, 1, 700, 2111], [4999, 813], [0 + 17, 2500, 2500, 795]]
    return [[(100 * k + 7 * c, rng.randint(-9000, 9001, n).astype(np.int16)) for k, n in enumerate(row)] for c, row in enumerate(lens)]


# ---- names, sizes, create ---------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runmm_names(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define MFM_ABI_VERSION %d\b" % b.MFM_ABI_VERSION, src)
    for name in ("OVER_RUNS", "OVER_DECISIONS", "IN_RUNRS", "IN_OUT_OF_STEP", "IN_BAD_RUNS"):
        m = re.search(r"#define MFM_RUNMM_%s (\d+)u" % name, src)
        assert m and int(m.group(1)) == getattr(b, "MFM_RUNMM_" + name), name
    own = open(os.path.join(ROOT, "tsl-sdr_amd", "csrc", "mfm_runmm.h")).read()
    assert re.search(r"#define MFM_RUNMM_STAGING_UNIT %du" % U, own) and b.RUNMM_STAGING_UNIT == U
    assert pkg.RunMm is b.RunMm and pkg.hosttwin_runmm_call is b.hosttwin_runmm_call and pkg.RUNMM_RUN_DTYPE is b.RUNMM_RUN_DTYPE
    for name in ("behind", "process_device", "fetch", "device_view", "fetch_state", "store_state", "close"):
        assert callable(getattr(pkg.RunMm, name)), name


def test_struct_sizes_match_the_dtypes(pkg):
    b = pkg.binding
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    for struct_name, dt, size in (("mfm_runmm_run", b.RUNMM_RUN_DTYPE, 40), ("mfm_runmm_state", b.RUNMM_STATE_DTYPE, 48)):
        m = re.search(r"struct %s \{(.*?)\};" % struct_name, src, flags=re.S)
        fields = re.findall(r"(uint\d+_t|float)\s+(\w+);", m.group(1))
        assert [n for _, n in fields] == list(dt.names), struct_name
        width = {"uint64_t": 8, "uint32_t": 4, "float": 4}
        assert sum(width[t] for t, _ in fields) == size == dt.itemsize, struct_name
        assert re.search(r"struct %s \{\s+/\* %d bytes \*/" % (struct_name, size), src), struct_name
    m = re.search(r"struct mfm_runmm_config \{(.*?)\};", src, flags=re.S)
    fields = [x for _, names in re.findall(r"(u?int\d+_t|float)\s+([\w, ]+);", m.group(1)) for x in names.split(", ")]
    assert fields == [f[0] for f in b.RunMmConfig._fields_] and C.sizeof(b.RunMmConfig) == 48


REFUSALS = [
    (dict(abi_version=3), "abi_version"),
    (dict(nr_channels=0), "nr_channels"),
    (dict(max_runs=0), "max_runs"),
    (dict(max_out_samples=0), "max_out_samples"),
    (dict(max_runs=1 << 28), "max_runs"),
    (dict(max_out_samples=1 << 31), "max_out_samples"),
    (dict(flags=1), "flags must be 0"),
    (dict(kw=float("inf")), "kw must be finite"),
    (dict(kw=float("nan")), "kw must be finite"),
    (dict(error_min=REF["emax"], error_max=REF["emin"]), "error_min must be at most error_max"),
    (dict(samples_per_bit=0.5), "samples_per_bit"),
    (dict(km=0.001), "error_min - |km| * 32768 must be at least 1"),        # 20.78 - 32.8: a step can reach zero
    (dict(km=-0.001), "error_min - |km| * 32768 must be at least 1"),
    (dict(error_max=2.0e6), "error_max + |km| * 32768 must be below 2^20"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_with_a_message(pkg, change, message):
    """every refusal of mfm_runmm_create is decided before a device is looked for; the twin refuses the same"""
    b = pkg.binding
    kw = dict(nr_channels=3, max_runs=100, max_out_samples=10000, samples_per_bit=REF["spb"], kw=KW, km=KM, error_min=REF["emin"],
              error_max=REF["emax"])
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunMm(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)
    if kw["nr_channels"]:
        tw = {k: v for k, v in kw.items() if k != "nr_channels"}
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runmm_call(b.hosttwin_runmm_state(kw["nr_channels"]), make_runs(pkg, []), np.zeros(0, np.int16), **tw)
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


# ---- the twin against the oracle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("par", [REF, WILD], ids=["ref", "wild"])
def test_hosttwin_equals_the_oracle_per_stretch_however_the_stream_is_cut(pkg, ora, par):
    """three channels of three or four stretches each (one of a single sample), cut into calls three ways: every call against
    the oracle, record by record, and the decisions of every stretch identical in the three cuts"""
    b = pkg.binding
    lines = _timelines()
    total = max(sum(x.size for _, x in line) for line in lines)
    rng = np.random.RandomState(2)
    ragged = [0]
    while ragged[-1] < total:
        ragged.append(ragged[-1] + int(rng.randint(1, 1200)))
    seen = []
    for edges in ([0, total], list(range(0, total + 997, 997)), ragged):
        chk, state, outs = Checker(pkg, ora, par), b.hosttwin_runmm_state(3), []
        for i, (runs, payload) in enumerate(cut_stream(pkg, lines, edges)):
            got = b.hosttwin_runmm_call(state, runs, payload, **twin_kw(par))
            same(got, chk.call(runs, payload), f"call {i} of {len(edges) - 1}")
            outs.append((runs, got))
        want = chk.stretches()
        mine = by_stretch(outs)
        assert mine.keys() == want.keys() and len(want) == 10
        for k in want:
            assert np.array_equal(mine[k], want[k]), k
        assert [int(s["outs"]) for s in state] == [line[-1][1].size for line in lines] and (state["has_stretch"] == 1).all()
        assert [int(s["decs"]) for s in state] == [want[(c, line[-1][0])].size for c, line in enumerate(lines)]
        seen.append(mine)
    for k in seen[0]:
        assert np.array_equal(seen[0][k], seen[1][k]) and np.array_equal(seen[0][k], seen[2][k]), k
    assert min_step(par) == (4 if par is WILD else 20)


def test_hosttwin_runs_of_0_1_and_s_minus_1_outputs_before_the_decision_arrives(pkg, ora):
    """two channels fed a call at a time with runs of 0, 1 and s - 1 outputs, several in a row: a run shorter than the distance
    to the next decision produces none and shortens next_offset, a run of nothing changes nothing and still continues"""
    b = pkg.binding
    s = min_step(REF)
    assert s == 20
    rng = np.random.RandomState(9)
    lens = [1, s - 1, 0, 1, 0, 0, s - 1, 1, 1, s - 1, s - 1, 0, 1] * 6
    x = [rng.randint(-9000, 9001, sum(lens) + 40).astype(np.int16) for _ in range(2)]
    chk, state = Checker(pkg, ora, REF), b.hosttwin_runmm_state(2)
    pos, empty, shortened = [0, 0], 0, 0
    for i, n in enumerate(lens):
        n1 = lens[(i + 5) % len(lens)]   # channel 1 walks the same lengths out of phase, and begins with a run of nothing
        rows, pieces, off = [], [], 0
        for c, m in ((0, n), (1, 0 if i == 0 else n1)):
            rows.append((c, m, i == 0, pos[c], 3 + c, off))
            pieces.append(x[c][pos[c]:pos[c] + m])
            pos[c] += m
            off += m
        runs, payload = make_runs(pkg, rows), np.concatenate(pieces)
        before = state.copy()
        got = b.hosttwin_runmm_call(state, runs, payload, **twin_kw(REF))
        same(got, chk.call(runs, payload), f"call {i}")
        for c, m in ((0, n), (1, rows[1][1])):
            if int(got[0]["nr_dec"][c]) == 0 and i > 0:
                empty += 1
                assert int(state["next_offset"][c]) == int(before["next_offset"][c]) - m and state["w"][c] == before["w"][c]
                assert state["m"][c] == before["m"][c] and int(state["decs"][c]) == int(before["decs"][c])
                shortened += m > 0
        assert [int(v) for v in state["outs"]] == pos
    assert empty >= 60 and shortened >= 30
    want = chk.stretches()
    assert all(d.size >= 10 for d in want.values())


def test_hosttwin_a_beginning_run_behind_a_carried_stretch_gets_fresh_state(pkg, ora):
    b = pkg.binding
    rng = np.random.RandomState(4)
    x = rng.randint(-9000, 9001, 900).astype(np.int16)
    state = b.hosttwin_runmm_state(1)
    one = b.hosttwin_runmm_call(state, make_runs(pkg, [(0, 400, True, 0, 2, 0)]), x[:400], **twin_kw(REF))
    carried = state.copy()
    assert int(carried["decs"][0]) == one[1].size >= 15 and carried["w"][0] != np.float32(REF["spb"])
    two = b.hosttwin_runmm_call(state, make_runs(pkg, [(0, 500, True, 0, 9, 0)]), x[400:], **twin_kw(REF))
    fresh = ora.MuellerMuller(KW, KM, REF["spb"], REF["emin"], REF["emax"]).process(np.concatenate([x[400:], [0]]).astype(np.int16), 0, 500)
    assert np.array_equal(two[1], fresh) and int(two[0]["first_dec"][0]) == 0 and int(two[0]["flags"][0]) == 1
    assert int(state["stretch_window"][0]) == 9 and int(state["outs"][0]) == 500 and int(state["decs"][0]) == fresh.size
    # and continuing instead gives the rest of the one stretch
    state = carried.copy()
    three = b.hosttwin_runmm_call(state, make_runs(pkg, [(0, 500, False, 400, 2, 0)]), x[400:], **twin_kw(REF))
    whole = ora.MuellerMuller(KW, KM, REF["spb"], REF["emin"], REF["emax"]).process(np.concatenate([x, [0]]).astype(np.int16), 0, 900)
    assert np.array_equal(np.concatenate([one[1], three[1]]), whole) and int(three[0]["first_dec"][0]) == one[1].size


def _refusal_case(pkg):
    """two calls on three channels; the second, whose first run continues channel 0, is the one that is varied"""
    b = pkg.binding
    rng = np.random.RandomState(12)
    p0, p1 = rng.randint(-9000, 9001, 700).astype(np.int16), rng.randint(-9000, 9001, 900).astype(np.int16)
    first = make_runs(pkg, [(0, 300, True, 0, 1, 0), (2, 400, True, 0, 1, 300)])
    runs = make_runs(pkg, [(0, 350, False, 300, 1, 0), (0, 50, True, 0, 8, 350), (1, 500, True, 0, 4, 400)])

    def changed(i, **kw):
        r = runs.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    IN, O = 8, 0
    cases = [
        (dict(totals=[3, 900, 1, 0]), "raised overflow or gate error", b.MFM_RUNMM_IN_RUNRS << IN),
        (dict(totals=[3, 900, 0, 2]), "raised overflow or gate error", b.MFM_RUNMM_IN_RUNRS << IN),
        (dict(runs=changed(0, first_out=299)), "out of step", b.MFM_RUNMM_IN_OUT_OF_STEP << IN),
        (dict(runs=changed(2, flags=0)), "out of step", b.MFM_RUNMM_IN_OUT_OF_STEP << IN),             # channel 1 has no stretch
        (dict(runs=changed(1, flags=0, first_out=650)), "out of step", b.MFM_RUNMM_IN_OUT_OF_STEP << IN),   # not its channel's first
        (dict(runs=changed(2, channel=3)), "not a burst resampler's", b.MFM_RUNMM_IN_BAD_RUNS << IN),
        (dict(runs=changed(0, channel=2)), "not a burst resampler's", (b.MFM_RUNMM_IN_BAD_RUNS | b.MFM_RUNMM_IN_OUT_OF_STEP) << IN),
        (dict(runs=changed(1, first_out=5)), "not a burst resampler's", b.MFM_RUNMM_IN_BAD_RUNS << IN),
        (dict(runs=changed(2, nr_out=501)), "not a burst resampler's", b.MFM_RUNMM_IN_BAD_RUNS << IN),
        (dict(runs=changed(2, out_offset=901)), "not a burst resampler's", b.MFM_RUNMM_IN_BAD_RUNS << IN),
        (dict(totals=[3, 1001, 0, 0]), "not a burst resampler's", b.MFM_RUNMM_IN_BAD_RUNS << IN),      # beyond max_out_samples
        (dict(totals=[5, 900, 0, 0]), "more runs than max_runs", b.MFM_RUNMM_OVER_RUNS << O),
    ]
    return (first, p0), (runs, p1), cases


def test_hosttwin_refuses_and_leaves_its_state(pkg, ora):
    """every flag: the resampler's flags handed through, out of step, run lists that are not a resampler's, max_runs, the decision
    bound against max_decisions; each time nothing comes out and the state stays, so the same call fed correctly is right"""
    b = pkg.binding
    (first, p0), (runs, p1), cases = _refusal_case(pkg)
    chk, state = Checker(pkg, ora, REF), b.hosttwin_runmm_state(3)
    conf = dict(max_runs=4, max_out_samples=1000)
    same(b.hosttwin_runmm_call(state, first, p0, **twin_kw(REF, **conf)), chk.call(first, p0), "call 0")
    s0 = state.copy()
    for change, message, flags in cases:
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runmm_call(state, change.get("runs", runs), p1, totals=change.get("totals"), **twin_kw(REF, **conf))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value), ei.value.flags)
        assert state.tobytes() == s0.tobytes(), change
    s = min_step(REF)
    bound = sum(slots(n, s) for n in runs["nr_out"])
    assert bound == 17 + 1 + 2 + 1 + 25 + 1
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runmm_call(state, runs, p1, **twin_kw(REF, max_decisions=bound - 1, **conf))
    assert ei.value.code == b.MFM_E_STATE and "decision bound" in str(ei.value) and ei.value.flags == b.MFM_RUNMM_OVER_DECISIONS
    assert state.tobytes() == s0.tobytes()
    # a run of nothing still has a slot: the bound, not the count, decides
    quiet = make_runs(pkg, [(1, 0, True, 0, 0, 0)] * 1)
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runmm_call(b.hosttwin_runmm_state(3), np.concatenate([quiet, quiet]), np.zeros(0, np.int16),
                              **twin_kw(REF, max_runs=4, max_out_samples=10, max_decisions=1))
    assert ei.value.flags == b.MFM_RUNMM_OVER_DECISIONS
    want = chk.call(runs, p1)
    with pytest.raises(pkg.MfmError) as ei:   # the caller's buffers too small: what is needed, and nothing moved
        b.hosttwin_runmm_call(state, runs, p1, max_out_decisions=want[1].size - 1, **twin_kw(REF, **conf))
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, want[1].size) and state.tobytes() == s0.tobytes()
    same(b.hosttwin_runmm_call(state, runs, p1, **twin_kw(REF, max_decisions=bound, **conf)), want, "the same call, right, after the refused ones")
    assert int(state["outs"][0]) == 50 and int(state["stretch_window"][0]) == 8 and int(state["outs"][2]) == 400


STATE_REFUSALS = [
    (dict(has_stretch=2), "has_stretch must be 0 or 1"),
    (dict(has_stretch=0), "has_stretch is 0 but another field is not 0"),
    (dict(outs=1 << 62), "outs and stretch_window must be below 2^62"),
    (dict(stretch_window=1 << 62), "outs and stretch_window must be below 2^62"),
    (dict(decs=101), "decs must be at most outs"),
    (dict(w=float("nan")), "w must be finite"),
    (dict(w=float("-inf")), "w must be finite"),
    (dict(m=-0.5), "m must be at least 0 and below 2^20"),
    (dict(m=float("nan")), "m must be at least 0 and below 2^20"),
    (dict(m=1048576.0), "m must be at least 0 and below 2^20"),
    (dict(last_sample=0.5), "last_sample must be a whole number an int16 holds"),
    (dict(last_sample=32768.0), "last_sample must be a whole number an int16 holds"),
    (dict(last_sample=float("nan")), "last_sample must be a whole number an int16 holds"),
    (dict(next_offset=1 << 21), "next_offset must be below 2^21"),
    (dict(reserved=1), "reserved must be 0"),
]


def good_state(pkg, nch=3):
    st = pkg.binding.hosttwin_runmm_state(nch)
    st[1] = (100, 5, 7, 20.9, 0.25, -1234.0, 3, 1, 0)
    st[2] = (0, 0, 9, REF["spb"], REF["spb"], 0.0, 0, 1, 0)   # a stretch of runs of nothing so far: mm_init's state
    return st


@pytest.mark.parametrize("change,message", STATE_REFUSALS, ids=[str(i) for i in range(len(STATE_REFUSALS))])
def test_state_check_names_channel_and_field(pkg, change, message):
    b = pkg.binding
    st = good_state(pkg)
    b.hosttwin_runmm_state_check(st)
    for k, v in change.items():
        st[k][1] = v
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runmm_state_check(st)
    assert ei.value.code == b.MFM_E_INVAL and "channel 1: " + message in str(ei.value), str(ei.value)


def test_runmm_kernels_use_no_scratch(pkg):
    """the code object's notes of build/mfm_runmm.o (tools/kernel_regs.py): the five kernels, no private segment, no spilled
    vector register, at most 256 VGPRs (two waves a SIMD); the walk's LDS is 16 strips of U samples and the candidate read's 16 bytes"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runmm.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == sorted(f"rm_{k}_kernel" for k in ("plan", "walk", "scan", "compact", "state")), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 256 and (int(m.group(2)), int(m.group(5))) == (0, 0), ln   # two waves a SIMD or more
        if ln.startswith("rm_walk_kernel"):
            assert int(m.group(4)) == 16 * (2 * U + 16), ln


# ---- case (a): steps out of the grid ------------------------------------------------------------------------------

A_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, U - 1, U, U + 1, 2 * U + 3, 5 * U + 77, 3, 40]


def case_a(pkg, full_scale):
    """three calls on three channels, 40 runs: the lengths above in turn, a channel's first run of the second and third call
    continuing its stretch and the others beginning one, and between two runs 0 .. 7 samples nobody owns, so that out_offset
    takes every residue modulo 8 (the payload's address is a multiple of 16 bytes where it is uploaded)"""
    rng = np.random.RandomState(31)
    amp = 32767 if full_scale else 9000
    calls, k, outs, fw = [], 0, {}, {}
    for call in range(3):
        rows, off = [], 0
        for c in range(3):
            for j in range(4 + (c + call) % 2):
                n = A_LENGTHS[k % len(A_LENGTHS)]
                off += (3 * k + 1) % 8
                cont = j == 0 and call > 0 and c != 1 - call % 2 and c in outs
                if not cont:
                    outs[c], fw[c] = 0, 10 * k + c
                rows.append((c, n, not cont, outs[c], fw[c], off))
                outs[c] += n
                off += n
                k += 1
        payload = rng.randint(-amp, amp + 1, off + 5).astype(np.int16)
        calls.append((make_runs(pkg, rows), payload))
    assert sum(len(r) for r, _ in calls) == 40
    assert {int(o) % 8 for r, _ in calls for o in r["out_offset"]} == set(range(8))
    assert {int(n) for r, _ in calls for n in r["nr_out"]} >= set(A_LENGTHS)
    assert sum(int((r["flags"] == 0).sum()) for r, _ in calls) >= 3
    return calls


@pytest.mark.parametrize("par,full_scale", [(REF, False), (WILD, True)], ids=["ref", "wild"])
def test_hosttwin_case_a(pkg, ora, par, full_scale):
    b = pkg.binding
    chk, state = Checker(pkg, ora, par), b.hosttwin_runmm_state(3)
    steps = []
    for i, (runs, payload) in enumerate(case_a(pkg, full_scale)):
        got = b.hosttwin_runmm_call(state, runs, payload, **twin_kw(par))
        same(got, chk.call(runs, payload), f"call {i}")
    chk.stretches()
    if par is WILD:   # the case is what it is meant to be: the clamp on both sides, steps far outside four candidates
        p = {k: np.float32(v) for k, v in par.items()}
        for key, pieces in chk.pcm.items():
            y = np.concatenate(pieces).astype(np.float32)
            # positions of the decisions: where the oracle's decisions were picked is not reported, so walk the loop here
            w, m, last, idx = p["spb"], p["spb"], np.float32(0), 0
            while idx < y.size:
                x = y[idx]
                w = np.float32(w + np.float32(np.float32(np.sign(last) * x) - np.float32(np.sign(x) * last)) * p["kw"])
                lo, hi = w < p["emin"], w > p["emax"]
                w = p["emin"] if lo else p["emax"] if hi else w
                m = np.float32(m + np.float32(w + np.float32(p["km"] * x)))
                st = int(np.floor(m))
                m = np.float32(m - np.float32(st))
                steps.append((st, int(lo) - int(hi)))
                idx += st
                last = x
        assert min(s for s, _ in steps) <= 6 and max(s for s, _ in steps) >= 35 and {c for _, c in steps} == {-1, 0, 1}


def test_hosttwin_is_clean_under_the_address_and_undefined_sanitizers(pkg, ora, tmp_path):
    """tests/hoststub/runmm_twin_main.cpp, a program of its own built with -fsanitize=address,undefined around the stage's host
    code, runs the twin on case (a)'s lists in buffers of exactly the sizes needed: nothing to report, and the oracle's result"""
    b = pkg.binding
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    exe = tmp_path / "runmm_twin"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "hoststub", "runmm_twin_main.cpp"),
           os.path.join(ROOT, "tsl-sdr_amd", "csrc", "mfm_runmm.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    if re.search(r"lib(a|t|ub|l|m)san", env.get("LD_PRELOAD", "")):   # another sanitizer's runtime does not share a process with this one
        del env["LD_PRELOAD"]
    env.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for par, full_scale in ((REF, False), (WILD, True)):
        chk = Checker(pkg, ora, par)
        state_file = tmp_path / "state.bin"
        state_file.write_bytes(b.hosttwin_runmm_state(3).tobytes())
        for i, (runs, payload) in enumerate(case_a(pkg, full_scale)):
            fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
            fin.write_bytes(struct.pack("<4I5f", 3, len(runs), payload.size, 0, par["kw"], par["km"], par["spb"], par["emin"], par["emax"])
                            + runs.tobytes() + payload.tobytes())
            r = subprocess.run([str(exe), str(fin), str(state_file), str(fout)], capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
            raw = fout.read_bytes()
            nr, nd = struct.unpack("<2Q", raw[:16])
            got = (np.frombuffer(raw[16:16 + 40 * nr], b.RUNMM_RUN_DTYPE), np.frombuffer(raw[16 + 40 * nr:16 + 40 * nr + 2 * nd], np.int16))
            same(got, chk.call(runs, payload), f"call {i}")


# ---- GPU ------------------------------------------------------------------------------------------------------

def _fed(pkg, torch, rm, runs, payload, totals=None):
    """one call from uploaded arrays: a burst resampler's result as it would stand in its device view"""
    t = np.array([len(runs), payload.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
    rm.process_device(*(k.data_ptr() for k in keep))
    try:
        return rm.fetch()
    finally:
        del keep


def _device_totals(rm):
    return tl._d2h(rm.device_view()[2], 32).view(np.uint64).tolist()


def _make(pkg, nch, max_runs, max_out, par, **kw):
    return pkg.RunMm(nch, max_runs, max_out, par["spb"], par["kw"], par["km"], error_min=par["emin"], error_max=par["emax"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("par,full_scale", [(REF, False), (WILD, True)], ids=["ref", "wild"])
def test_gpu_case_a_steps_out_of_the_grid(pkg, ora, par, full_scale):
    """(a) runs of 0 .. 17 samples and around the staging unit U = 512 (U - 1, U, U + 1, 2U + 3, 5U + 77) at every alignment of
    out_offset, continuing and beginning; the reference loop, and a loop with steps of 4 .. 37 samples on full-scale input: the
    oracle per run, the twin's state, the device view"""
    import torch
    b = pkg.binding
    calls = case_a(pkg, full_scale)
    rm = _make(pkg, 3, 16, max(p.size for _, p in calls), par)
    chk, twin = Checker(pkg, ora, par), b.hosttwin_runmm_state(3)
    for i, (runs, payload) in enumerate(calls):
        got = _fed(pkg, torch, rm, runs, payload)
        want = chk.call(runs, payload)
        same(got, want, f"call {i}")
        same(b.hosttwin_runmm_call(twin, runs, payload, **twin_kw(par)), got, f"the twin's call {i}")
        assert rm.fetch_state().tobytes() == twin.tobytes(), i
        assert _device_totals(rm) == [len(runs), want[1].size, 0, 0]
        d_runs, d_dec, _ = rm.device_view()
        assert tl._d2h(d_runs, got[0].nbytes).tobytes() == got[0].tobytes()
        if got[1].size:
            assert tl._d2h(d_dec, got[1].nbytes).tobytes() == got[1].tobytes()
    chk.stretches()
    rm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130, 1024, 1025, 2049])
def test_gpu_more_runs_than_lanes_and_waves(pkg, ora, n):
    """(b) one run per channel.  65 and 130 runs of a few hundred samples: more than the 16 walking lanes of a wave, more than the 64
    lanes that stage, more than twice that.  1024, 1025 and 2049
    tiny runs of odd length: the scans' 1024 threads take one run, one or two, two or three each, and every run of a sample or
    more has a decision (its first sample) on those boundaries.  A second call continues every third channel, begins every
    third anew and leaves the rest out"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(n)
    tiny = n >= 1024
    lens = [2 * (i % 23) + 1 for i in range(n)] if tiny else [301 + 14 * (i % 9) for i in range(n)]
    off = np.cumsum([0] + lens[:-1])
    first = make_runs(pkg, [(c, lens[c], True, 0, c % 5, int(off[c])) for c in range(n)])
    p0 = rng.randint(-9000, 9001, sum(lens)).astype(np.int16)
    rows, o = [], 0
    for c in range(n):
        if c % 3 == 2:
            continue
        m = lens[(c + 7) % n] + (0 if tiny else 3 * U)
        rows.append((c, m, c % 3 == 1, 0 if c % 3 == 1 else lens[c], 77 if c % 3 == 1 else c % 5, o))
        o += m
    second = make_runs(pkg, rows)
    p1 = rng.randint(-9000, 9001, o).astype(np.int16)
    rm = _make(pkg, n, n, max(p0.size, p1.size), REF)
    chk, twin = Checker(pkg, ora, REF), b.hosttwin_runmm_state(n)
    for i, (runs, payload) in enumerate(((first, p0), (second, p1))):
        got = _fed(pkg, torch, rm, runs, payload)
        same(got, chk.call(runs, payload), f"call {i}")
        same(b.hosttwin_runmm_call(twin, runs, payload, **twin_kw(REF)), got, f"the twin's call {i}")
        assert rm.fetch_state().tobytes() == twin.tobytes(), i
        assert (got[0]["nr_dec"] >= 1).all() if i == 0 else True
    assert len(chk.stretches()) == n + len([c for c in range(n) if c % 3 == 1])
    rm.close()


_TX = {}


def _transmission(pkg):
    """20 000 samples at 25 kHz of a 1200-baud POCSAG transmission with a short preamble (pkg.synth, as
    tests/test_mueller_muller.py): two batches, so two sync words, inside the piece"""
    if not _TX:
        sy = pkg.synth
        msgs = [(0x12345, 3, 2, sy.pocsag_alpha_words("MUELLER AND MULLER IN BURSTS")), (0x00777, 5, 0, sy.pocsag_numeric_words("0123-456 9")),
                (0x3FFF0, 0, 3, sy.pocsag_alpha_words("The quick brown fox jumps over the lazy dog " * 2))]
        bits = sy.pocsag_bits(sy.pocsag_batches(msgs), preamble_bits=300)
        _TX["pcm"] = sy.pocsag_pcm(bits, 1200, noise=900, lead=300, trail=4000, seed=1, rate=25000)[:20000].copy()
        assert _TX["pcm"].size == 20000
    return _TX["pcm"]


def sync_words(decisions):
    """the reference consumer (pager/test/test_mueller_muller.c:118-121): d > 0 ? 0 : 1 into a shift register, a sync word when
    fewer than 4 bits differ; the decisions at which one is complete"""
    shr, pos = 0, []
    for i, d in enumerate(decisions):
        shr = ((shr << 1) | (0 if d > 0 else 1)) & 0xFFFFFFFF
        if bin(SYNC ^ shr).count("1") < 4:
            pos.append(i)
    return pos


def test_the_transmission_is_what_it_is_meant_to_be(pkg, ora):
    """from the oracle alone: the piece holds two sync words 544 decisions apart, and the loop finds both"""
    pcm = _transmission(pkg)
    d = ora.MuellerMuller(KW, KM, REF["spb"], REF["emin"], REF["emax"]).process(np.concatenate([pcm, np.zeros(1, np.int16)]), 0, pcm.size)
    pos = sync_words(d)
    assert len(pos) == 2 and pos[1] - pos[0] == 544


@pytest.mark.gpu
def test_gpu_a_stretch_of_20000_outputs_cut_into_calls(pkg, ora):
    """(c) one stretch cut into calls of 1 .. 5000 outputs, and once whole: the same decisions, the oracle's, and the reference
    consumer finds every sync word in them"""
    import torch
    pcm = _transmission(pkg)
    rng = np.random.RandomState(8)
    sizes = [1, 5000, 1, 2, 511, 512, 513, 19]
    while sum(sizes) < pcm.size:
        sizes.append(min(int(rng.randint(1, 5001)), pcm.size - sum(sizes)))
    want = ora.MuellerMuller(KW, KM, REF["spb"], REF["emin"], REF["emax"]).process(np.concatenate([pcm, np.zeros(1, np.int16)]), 0, pcm.size)
    for cuts in (sizes, [pcm.size]):
        rm = _make(pkg, 1, 1, 5000 if len(cuts) > 1 else pcm.size, REF)
        chk, parts, pos = Checker(pkg, ora, REF), [], 0
        for i, m in enumerate(cuts):
            runs = make_runs(pkg, [(0, m, pos == 0, pos, 4, 0)])
            got = _fed(pkg, torch, rm, runs, pcm[pos:pos + m])
            same(got, chk.call(runs, pcm[pos:pos + m]), f"call {i} of {len(cuts)}")
            parts.append(got[1])
            pos += m
        dec = np.concatenate(parts)
        assert np.array_equal(dec, want)
        assert sync_words(dec) == sync_words(want) and len(sync_words(dec)) == 2
        st = rm.fetch_state()
        assert int(st["outs"][0]) == pcm.size and int(st["decs"][0]) == want.size
        rm.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state_and_a_state_stored_is_a_state_fetched(pkg, ora):
    """(d) every refusal of the twin's test on the device, with the twin's flags in the totals; a call whose decision bound is one
    above max_decisions; each time nothing comes out and the state stays.  The state then moves to an object the call fits
    (store_state, fetched back unchanged; a state that fails is refused with channel and field and changes nothing), where the
    same input is right"""
    import torch
    b = pkg.binding
    (first, p0), (runs, p1), cases = _refusal_case(pkg)
    s = min_step(REF)
    bound = sum(slots(n, s) for n in runs["nr_out"])
    chk = Checker(pkg, ora, REF)
    rm = _make(pkg, 3, 4, 1000, REF, max_decisions=bound - 1)
    same(_fed(pkg, torch, rm, first, p0), chk.call(first, p0), "call 0")
    s0 = rm.fetch_state()
    twin = s0.copy()
    for change, message, flags in cases + [(dict(), "decision bound", b.MFM_RUNMM_OVER_DECISIONS)]:
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rm, change.get("runs", runs), p1, totals=change.get("totals"))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (change, str(ei.value))
        assert ei.value.needed == (0, 0)
        assert _device_totals(rm) == [0, 0, flags & 0xff, flags >> 8], (change, _device_totals(rm))
        with pytest.raises(pkg.MfmError) as et:
            b.hosttwin_runmm_call(twin, change.get("runs", runs), p1, totals=change.get("totals"),
                                  **twin_kw(REF, max_runs=4, max_out_samples=1000, max_decisions=bound - 1))
        assert et.value.flags == flags and str(et.value).split(": ", 1)[-1] == str(ei.value).split(": ", 1)[-1]
        assert rm.fetch_state().tobytes() == s0.tobytes() == twin.tobytes(), change
    fits = _make(pkg, 3, 4, 1000, REF, max_decisions=bound)
    bad = s0.copy()
    bad["m"][2] = -1.0
    with pytest.raises(pkg.MfmError) as ei:
        fits.store_state(bad)
    assert ei.value.code == b.MFM_E_INVAL and "channel 2: m must be" in str(ei.value)
    assert not fits.fetch_state().view(np.uint8).any()
    fits.store_state(s0)
    assert fits.fetch_state().tobytes() == s0.tobytes()
    want = chk.call(runs, p1)
    got = _fed(pkg, torch, fits, runs, p1)
    same(got, want, "the same call in an object it fits")
    with pytest.raises(pkg.MfmError) as ei:
        fits.fetch(max_runs=3, max_decisions=want[1].size - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, want[1].size)
    same(fits.fetch(), want, "fetched again")
    b.hosttwin_runmm_call(twin, runs, p1, **twin_kw(REF))
    assert fits.fetch_state().tobytes() == twin.tobytes()
    for o in (rm, fits):
        o.close()


CHAIN = dict(nch=4, W=256, P=1, n=256 * 90, hang=1, seed=17)
_CHAIN = {}


def _chain(pkg, ora):
    """four PCM rows at 31 250 Hz (25 kHz behind the 4/5 resampler): quiet noise, and on each row two or three loud stretches of a
    1200-baud square wave of its own phase with noise on it; the squelch opens above an rms of 1000"""
    if _CHAIN:
        return _CHAIN["it"]
    s = CHAIN
    n, W = s["n"], s["W"]
    rng = np.random.RandomState(s["seed"])
    rows = (rng.randn(s["nch"], n) * 60).round().astype(np.int16)
    t = np.arange(n)
    for c in range(s["nch"]):
        for k in range(2 + c % 2):
            a = W * (4 + 27 * k + 2 * c) + 37 * c
            e = a + W * (7 + 3 * k) + 11 * k
            bits = rng.randint(0, 2, n // 20 + 2) * 2 - 1
            wave = bits[((t[a:e] - a) * 1200.0 / 31250.0 + 0.3 * c).astype(np.int64)] * 7000 + rng.randn(e - a) * 900
            rows[c, a:e] = np.clip(wave, -32768, 32767).round().astype(np.int16)
    thr = W * 1000 * 1000
    mask = tl.restate(pkg, rows, W, tl.PCM, sense=tl.ABOVE, open_thr=thr, close_thr=thr, hang=s["hang"])["open"].astype(bool)
    lpf = [float(x) for x in pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4]
    rtaps = np.array([int(x * 16384.0) for x in lpf], np.int16)   # as the scan tool quantises them
    cuts = [0, W * 7, W * 1, 3 * W + 5, W - 5]
    while sum(cuts) < n:
        cuts.append(min(W * int(rng.randint(1, 20)), n - sum(cuts)))
    _CHAIN["it"] = dict(rows=np.ascontiguousarray(rows), mask=mask, thr=thr, lpf=lpf, rtaps=rtaps, cuts=cuts)
    return _CHAIN["it"]


def test_chain_scene_is_what_it_is_meant_to_be(pkg, ora):
    sc, s = _chain(pkg, ora), CHAIN
    emitted = tgp.dilate(sc["mask"], s["P"])
    per = [sum(1 for k in tr.stretches_of_mask(emitted) if k[0] == c) for c in range(s["nch"])]
    assert per == [2, 3, 2, 3] and not emitted.all(axis=1).any()


@pytest.mark.gpu
def test_gpu_level_gate_runrs_runmm_on_device_equals_the_chain_through_the_oracle(pkg, ora):
    """(e) level -> gate with P = 1 -> burst resampler 4/5 -> burst Mueller-Muller, all on the device views with no fetch in
    between, in ragged calls (one of no samples, two that end inside a window) and the flush: every call against the restated
    level and gate, the oracle's resampler and the oracle's loop per stretch; the twin's state at the end"""
    b = pkg.binding
    sc, s = _chain(pkg, ora), CHAIN
    rows, mask, cuts, W, P, nch = sc["rows"], sc["mask"], sc["cuts"], s["W"], s["P"], s["nch"]
    cap = max(cuts)
    lv = pkg.Level(nch, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=s["hang"])
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    rr = pkg.RunResampler(nch, sc["rtaps"], 4, 5, W, max_in_samples=cap, preroll_windows=P)
    rm = pkg.RunMm.behind(rr, REF["spb"], KW, KM, error_min=REF["emin"], error_max=REF["emax"])
    rs, chk, twin = tr.Checker(pkg, ora, sc["rtaps"], 4, 5, False, W), Checker(pkg, ora, REF), b.hosttwin_runmm_state(nch)
    pos, decisions = 0, 0
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gate.process_host(rows[:, pos:pos + m], lv.process_host(rows[:, pos:pos + m]))
            want_rs = rs.call(*tgp.restate_pre(pkg, rows, mask, W, 1, P, pos, m))
            pos += m
        else:
            gate.flush_device()
            want_rs = rs.call(*tgp.restate_pre(pkg, rows, mask, W, 1, P, pos, 0, flush=True))
        rr.process_device(*gate.device_view())
        rm.process_device(*rr.device_view())
        got = rm.fetch()
        tr.same(rr.fetch(), want_rs, f"the resampler's call {i}")
        same(got, chk.call(*want_rs), f"call {i}")
        same(b.hosttwin_runmm_call(twin, *want_rs, **twin_kw(REF)), got, f"the twin's call {i}")
        decisions += got[1].size
    assert pos == rows.shape[1]
    by = chk.stretches()
    assert len(by) == 10 and decisions == sum(d.size for d in by.values()) >= 10 * 80
    assert rm.fetch_state().tobytes() == twin.tobytes()
    for o in (rm, rr, gate, lv):
        o.close()


TOOL_PAR = dict(kw=KW, km=KM, spb=16.0, emin=float(np.float32(16.0) - MARGIN), emax=float(np.float32(16.0) + MARGIN))


def tool_setup(pkg, ora, tmp_path):
    """the chain scene of tests/test_runpocsag.py (two FM channels of 2400-baud bursts, 38 400 Hz behind the 4/5 resampler: 16
    samples per bit) as the files the scan tool reads; the command up to and without --gate-out"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    centre = 929000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": s["fs"], "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": s["decim"],
        "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    return [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
            str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(s["W"]), "--open-thr", str(sc["thr"]),
            "--hang", str(s["hang"]), "--block", str(s["blk"]), "--gate-preroll", str(s["P"])]


def tool_want(pkg, ora):
    """{(channel, first window): decisions} of that scene through the restated gate, the oracle's resampler and the oracle's loop"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    W, P = s["W"], s["P"]
    rs, chk = tr.Checker(pkg, ora, sc["rtaps"], 4, 5, False, W), Checker(pkg, ora, TOOL_PAR)
    n = sc["pcm"].shape[1]
    chk.call(*rs.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n)))
    chk.call(*rs.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True)))
    by = chk.stretches()
    assert len(by) >= 3 and all(d.size >= 500 for d in by.values())
    return by


def tool_check(out_dir, by, W, channels=(0, 1)):
    """chNNNN.mm.s16 under out_dir holds the decisions stretch by stretch, mm.jsonl a line per run that adds up to them"""
    lines = [json.loads(ln) for ln in (out_dir / "mm.jsonl").read_text().splitlines()]
    assert all(set(ln) == {"channel", "first_sample", "first_dec", "nr_dec", "begins", "file_offset"} for ln in lines)
    assert {ln["channel"] for ln in lines} <= set(channels)
    for c in channels:
        keys = sorted(k for k in by if k[0] == c)
        want = np.concatenate([by[k] for k in keys])
        got = np.fromfile(str(out_dir / ("ch%04d.mm.s16" % c)), np.int16)
        assert np.array_equal(got, want), c
        mine = [ln for ln in lines if ln["channel"] == c]
        at, stretch, last = 0, [], -1
        for ln in mine:   # a line per run, in stream order: the file's bytes in order, first_dec counting within the stretch
            if ln["begins"]:
                stretch.append([ln["first_sample"], 0])
            assert ln["file_offset"] == 2 * at and ln["first_dec"] == stretch[-1][1], ln
            assert ln["first_sample"] > last and ln["first_sample"] % W == 0, ln   # the run's own first sample
            at += ln["nr_dec"]
            stretch[-1][1] += ln["nr_dec"]
            last = ln["first_sample"]
        assert stretch == [[k[1] * W, by[k].size] for k in keys]


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_mm_writes_the_decisions_of_the_oracle(pkg, ora, tmp_path):
    """(f) tools/level_scan.py --gate-out DIR --gate-preroll 1 --gate-resample 4/5 --resample-taps FILE --gate-mm SPB as a fresh
    child process on the chain scene of tests/test_runpocsag.py: chNNNN.mm.s16 holds the oracle's decisions stretch by stretch,
    mm.jsonl a line per run that adds up to them"""
    base = tool_setup(pkg, ora, tmp_path)
    cmd = base + ["--gate-out", str(tmp_path / "gated"), "--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"),
                  "--gate-mm", "16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    tool_check(tmp_path / "gated", tool_want(pkg, ora), trp.CHAIN["W"])
    r = subprocess.run(cmd[:-6] + ["--gate-mm", "16"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-mm needs --gate-resample" in r.stderr
    r = subprocess.run(cmd + ["--gate-pocsag"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "exclude each other" in r.stderr


LONG = dict(kw=KW, km=KM, spb=1000.0, emin=float(np.float32(1000.0) - MARGIN), emax=float(np.float32(1000.0) + MARGIN))


def _fed_shifted(pkg, torch, rm, runs, payload, shift):
    """as _fed, the payload standing `shift` samples behind the start of its allocation: an address that is no multiple of 16"""
    t = np.array([len(runs), payload.size, 0, 0], np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, np.concatenate([np.full(shift, 0x7111, np.int16), payload])), tr._up(torch, t))
    assert keep[1].data_ptr() % 16 == 0
    rm.process_device(keep[0].data_ptr(), keep[1].data_ptr() + 2 * shift, keep[2].data_ptr())
    try:
        return rm.fetch()
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_steps_longer_than_the_staging_unit_and_a_payload_off_the_grid(pkg, ora):
    """1000 samples per bit, so every step passes over a unit of U = 512 samples or more (the first of a stretch four): a run that continues starts with
    next_offset >= U (its strip begins at a later unit, nothing in front of it is staged), units go by without a decision, and a
    run's last samples are written in a unit the walk never reads.  The payload's address is 2, 6 and 10 bytes off the 16-byte
    grid in turn.  The state moves to a second object after the first call (store_state with next_offset >= U) and both go on:
    the oracle per run, the twin's state"""
    import torch
    b = pkg.binding
    rng = np.random.RandomState(41)
    lens = [[100, 4000, 1500], [2200, 700, 1500], [1, 2 * U + 3, 1500]]
    fw = [3, 4, 5]
    calls, outs = [], [0, 0, 0]
    for k in range(3):
        rows, off = [], 0
        for c in range(3):
            rows.append((c, lens[c][k], k == 0, outs[c], fw[c], off))
            outs[c] += lens[c][k]
            off += lens[c][k]
        calls.append((make_runs(pkg, rows), rng.randint(-9000, 9001, off).astype(np.int16)))
    cap = max(p.size for _, p in calls)
    one, two = _make(pkg, 3, 3, cap, LONG), _make(pkg, 3, 3, cap, LONG)
    chk, twin = Checker(pkg, ora, LONG), b.hosttwin_runmm_state(3)
    for i, (runs, payload) in enumerate(calls):
        want = chk.call(runs, payload)
        same(b.hosttwin_runmm_call(twin, runs, payload, **twin_kw(LONG)), want, f"the twin's call {i}")
        same(_fed_shifted(pkg, torch, one, runs, payload, (1, 3, 5)[i]), want, f"call {i}")
        assert one.fetch_state().tobytes() == twin.tobytes(), i
        if i == 0:
            st = one.fetch_state()
            assert (st["next_offset"] >= U).all(), st["next_offset"]   # the case is what it is meant to be
            two.store_state(st)
        else:
            same(_fed_shifted(pkg, torch, two, runs, payload, (0, 7, 2)[i]), want, f"call {i} on the object the state moved to")
            assert two.fetch_state().tobytes() == twin.tobytes(), i
    by = chk.stretches()
    assert len(by) == 3 and sum(d.size for d in by.values()) >= 10
    # runs that end without a decision: channel 1's 700 samples lie between two decisions, and channel 2's 2U + 3 behind its one
    # sample are shorter than the first step (2 * spb), so their last samples are staged and never read
    assert chk.by[(1, 4)][1].size == 0 and chk.by[(2, 5)][1].size == 0 and chk.by[(0, 3)][1].size == 3
    for o in (one, two):
        o.close()
