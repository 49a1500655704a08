"""The stretch-end report of the burst stages (mfm_run*_set_end_report and kin, csrc/mfm_run_ends.hip, csrc/mfm_run_ends.h): one
record per stretch that says how the stretch ended and what the closing squelch cut.

What is expected never comes from the code under test.  Which stretches exist, in which call each ends and with how many
outputs is derived here from the run lists alone (stretches_of_runs).  What a record holds is restated here from the state a
fresh plain twin (mfm_hosttwin_run*_call, which tests/test_runais.py, test_runpocsag.py and test_runflex.py check against the
oracle) is left in by that stretch alone, POCSAG's BCH through the oracle library's decoder.  On the device the reference is the
host twin with the report.  Every comparison is an equality."""
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
import test_run_bits as trb
import test_runais as tra
import test_runflex as trf
import test_runpocsag as trp
import test_runrs as tr

ROOT = tg.ROOT
NO_RUN = 0xffffffff
STAGES = ["runais", "runpocsag", "runflex"]
NEW_NAMES = [f"mfm_{s}_{e}" for s in STAGES for e in ("set_end_report", "end_stretches_device", "fetch_ends", "ends_view")] + \
    [f"mfm_hosttwin_{s}_{e}" for s in STAGES for e in ("call_ends", "end_stretches")]
SIZES = {"runais": 48, "runpocsag": 184, "runflex": 64}
# (ratio, W, pre-roll): W = 7 with the stages' first ratio has runs without output (the phase is longer than a window) and
# stretches of one or two windows, many of a channel in one call; W = 64 at 1/1 has the stages' designed "cut" masks
CONFIGS = [(0, 7, 0), (1, 64, 1)]


# ---- the three stages behind one face ----------------------------------------------------------------------------

class Proto:
    def __init__(self, pkg, ora, name):
        b = pkg.binding
        self.pkg, self.ora, self.b, self.name = pkg, ora, b, name
        self.mod = {"runais": tra, "runpocsag": trp, "runflex": trf}[name]
        self.end_dtype = {"runais": b.RUNAIS_END_DTYPE, "runpocsag": b.RUNPOCSAG_END_DTYPE, "runflex": b.RUNFLEX_END_DTYPE}[name]
        self.flex = name == "runflex"
        self.polarity = {"runais": trb.POS, "runpocsag": trb.NEG, "runflex": None}[name]
        self.new_state = getattr(b, f"hosttwin_{name}_state")
        self._call = getattr(b, f"hosttwin_{name}_call")
        self._call_ends = getattr(b, f"hosttwin_{name}_call_ends")
        self.twin_end = getattr(b, f"hosttwin_{name}_end_stretches")
        self.Stage = {"runais": pkg.RunAis, "runpocsag": pkg.RunPocsag, "runflex": pkg.RunFlex}[name]

    def scene(self, ratio, W):
        return self.mod.scene(self.pkg, ratio) if self.name == "runais" else self.mod.scene(self.pkg, self.ora, ratio, W)

    def call(self, state, runs, payload, **kw):
        """the plain twin; the events as a tuple of arrays (FLEX: events and frames)"""
        out = self._call(state, runs, payload, **kw)
        return out if self.flex else (out,)

    def call_ends(self, state, runs, payload, **kw):
        out = self._call_ends(state, runs, payload, **kw)
        return out[:-1], out[-1]

    def states(self, state):
        """the per-channel state array of a twin state"""
        return state[0] if self.flex else state

    def copy(self, state):
        return tuple(x.copy() for x in state) if self.flex else state.copy()

    def fetch(self, st):
        out = st.fetch()
        return out if self.flex else (out,)

    def fetch_states(self, st):
        return st.fetch_state(with_ring=False) if self.flex else st.fetch_state()

    def record(self, s, channel, run):
        """a record restated from one state: the independent statement of the mapping"""
        e = np.zeros((), self.end_dtype)
        e["stretch_window"], e["outs"], e["channel"], e["run"], e["mode"] = s["stretch_window"], s["outs"], channel, run, s["mode"]
        mode = int(s["mode"])
        if self.name == "runais":
            if mode == 1:
                e["start_sample"], e["nr_bits"] = s["start"], s["cur_bit"]
        elif self.name == "runflex":
            if mode:
                e["j"], e["eye"] = s["j"], s["eye"]
            if mode == 2:
                for f in ("coding", "fiw", "cycle", "frame"):
                    e[f] = s[f]
        else:
            e["raw"] = s["batch"]
            if mode:
                e["baud"] = s["baud"]
            if mode == 3:
                e["nr_sync_bits"] = s["nr_sync_bits"]
            if mode == 2:
                nw = int(s["batch_word"])
                e["nr_words"], e["nr_bits"] = nw, s["batch_bit"]
                fail, nr_ok = 0, None
                for z in range(nw):
                    rc, v = self.ora.bch3121_decode(int(s["batch"][z]) & 0x7fffffff)
                    e["corrected"][z] = v
                    if rc:
                        fail |= 1 << z
                        nr_ok = z if nr_ok is None else nr_ok
                e["fail_mask"], e["nr_ok"] = fail, nw if nr_ok is None else nr_ok
        return e


@pytest.fixture(scope="module", params=STAGES)
def proto(request, pkg, ora):
    return Proto(pkg, ora, request.param)


def same_records(got, want, what, fields=None):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in (fields or want.dtype.names) if len(want) else ():
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, f"{what}: record field {f} differs at {bad[:5].tolist()}: {got[f][bad[0]]} != {want[f][bad[0]]}"


def same_events(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


# ---- scenes: the stages' own streams under random open masks, every call cutting ---------------------------------

_CALLS = {}


def random_mask(rng, nch, nw):
    """raw squelch verdicts [C][nw]: per channel open and closed blocks in turn, short ones (1 - 3 windows: many stretches of a
    channel in one call) and long ones mixed; channel 0 opens at window 0, the last channel is closed all the time when there
    are three or more"""
    m = np.zeros((nch, nw), bool)
    for c in range(nch):
        k = 0 if c == 0 else int(rng.randint(0, 6))
        while k < nw:
            ln = int(rng.randint(1, 4)) if rng.rand() < 0.6 else int(rng.randint(4, max(5, nw // 5)))
            m[c, k:k + ln] = True
            k += ln + (int(rng.randint(1, 4)) if rng.rand() < 0.6 else int(rng.randint(4, max(5, nw // 8))))
    if nch >= 3:
        m[nch - 1] = False
    return m


def random_cuts(rng, n, W):
    """piece lengths that add up to n: an nr_in = 0 call first and one in the middle, one-window calls, pieces of up to 120 windows
    (a sixth of a short stream at most) that end anywhere"""
    out, pos, big = [0], 0, max(2, min(120, n // W // 6))
    while pos < n:
        m = min([W, int(rng.randint(1, big * W)), int(rng.randint(1, 6)) * W][int(rng.randint(0, 3))], n - pos)
        out.append(m)
        pos += m
    out.insert(len(out) // 2, 0)
    return out


def rs_calls(pkg, ora, stream, mask, W, P, cuts, taps, I, D):
    """[(runs, payload)]: the restated gate and the oracle's resampler per stretch, as the stages' own tests feed them"""
    chk = tr.Checker(pkg, ora, taps, I, D, False, W)
    return [chk.call(gr, gp) for gr, gp in tr.gate_calls(pkg, stream, mask, W, P, cuts)]


def scene_calls(proto, cfg, nch=4, limit=None, single=False):
    """the calls of one stream in the seeded cut, or as one call that holds everything; made once and left unchanged"""
    key = (proto.name, cfg, nch, limit, single)
    if key not in _CALLS:
        ri, W, P = cfg
        ratio = proto.mod.RATIOS[ri]
        I, D, _ = ratio
        sc = proto.scene(ratio, W)
        n = sc["n_in"] if limit is None else min(sc["n_in"], limit // nch // W * W)
        stream = np.ascontiguousarray(sc["stream"][np.arange(nch) % sc["stream"].shape[0], :n])
        rng = np.random.RandomState(1000 * STAGES.index(proto.name) + 10 * W + nch)
        mask = random_mask(rng, nch, n // W)
        cuts = [n] if single else random_cuts(rng, n, W)
        taps = proto.mod.rs_taps(proto.pkg, proto.ora, ratio)
        _CALLS[key] = dict(calls=rs_calls(proto.pkg, proto.ora, stream, mask, W, P, cuts, taps, I, D), stream=stream, mask=mask, W=W, P=P,
                           taps=taps, I=I, D=D, n=n, nch=nch)
    return _CALLS[key]


def designed_calls(proto, kind="cut"):
    """the stage file's own "cut" mask (closes inside packets, batches and blocks) at W = 64, 1/1, in its own seeded cut"""
    key = (proto.name, "designed", kind)
    if key not in _CALLS:
        mod, pkg, ora = proto.mod, proto.pkg, proto.ora
        ratio, W, P = mod.RATIOS[1], 64, 0
        sc = proto.scene(ratio, W)
        rng = np.random.RandomState(99)
        mask = mod.make_mask(kind, sc, W, rng)
        mask = mask[0] if isinstance(mask, tuple) else mask
        cuts = random_cuts(rng, sc["n_in"], W)
        taps = mod.rs_taps(pkg, ora, ratio)
        _CALLS[key] = dict(calls=rs_calls(pkg, ora, sc["stream"], mask, W, P, cuts, taps, ratio[0], ratio[1]), W=W, nch=4)
    return _CALLS[key]


def stretches_of_runs(calls):
    """from the run lists alone: [(call, channel, stretch_window, outs, run)] in the order the records must come, the end call
    (call = len(calls), run = NO_RUN) last; and the pieces of every stretch, {(channel, stretch_window): [payload slices]}"""
    cur, recs, pieces = {}, [], {}
    for i, (runs, payload) in enumerate(calls):
        for r, run in enumerate(runs):
            c = int(run["channel"])
            if int(run["flags"]) & 1:
                if c in cur:
                    recs.append((i, c, cur[c][0], cur[c][1], r))
                cur[c] = [int(run["first_window"]), 0]
                pieces[(c, cur[c][0])] = []
            assert int(run["first_out"]) == cur[c][1]
            cur[c][1] += int(run["nr_out"])
            pieces[(c, cur[c][0])].append(payload[int(run["out_offset"]):int(run["out_offset"]) + int(run["nr_out"])])
    recs += [(len(calls), c, cur[c][0], cur[c][1], NO_RUN) for c in sorted(cur)]
    return recs, pieces


def twin_stream(proto, calls, nch, **kw):
    """the stream through the twin with the report: ([events per call], [records per call], records of the end call)"""
    state = proto.new_state(nch)
    evs, ends = [], []
    for runs, payload in calls:
        e, r = proto.call_ends(state, runs, payload, **kw)
        evs.append(e)
        ends.append(r)
    last = proto.twin_end(state)
    assert not proto.states(state).view(np.uint8).any()
    return evs, ends, last


def per_run(calls):
    """the same stream with a call boundary at every run boundary"""
    out = []
    for runs, payload in calls:
        for run in runs:
            one = np.array([run], runs.dtype)
            one["out_offset"] = 0
            out.append((one, payload[int(run["out_offset"]):int(run["out_offset"]) + int(run["nr_out"])].copy()))
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib, b = pkg.load_library(), pkg.binding
    for n in NEW_NAMES:
        assert n in declared and hasattr(lib, n) and n in b.ABI_SYMBOLS, n
    for s, dt in (("runais", b.RUNAIS_END_DTYPE), ("runpocsag", b.RUNPOCSAG_END_DTYPE), ("runflex", b.RUNFLEX_END_DTYPE)):
        assert dt.itemsize == SIZES[s]
        m = re.search(r"struct mfm_%s_end \{(.*?)\};" % s, src, flags=re.S)
        fields = re.findall(r"(uint\d+_t)\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
        assert [n for _, n, _ in fields] == list(dt.names)
        assert sum(int(t[4:-2]) // 8 * int(k or 1) for t, _, k in fields) == SIZES[s]   # no padding: the fields add up
        at = 0
        for t, n, k in fields:
            assert dt.fields[n][1] == at, (s, n)
            at += int(t[4:-2]) // 8 * int(k or 1)
    # the sizes the library was compiled with: an end call on one channel with a stretch writes exactly one record
    for s, dt in (("runais", b.RUNAIS_END_DTYPE), ("runpocsag", b.RUNPOCSAG_END_DTYPE), ("runflex", b.RUNFLEX_END_DTYPE)):
        st = getattr(b, f"hosttwin_{s}_state")(2)
        arr = st[0] if s == "runflex" else st
        arr["has_stretch"], arr["outs"], arr["stretch_window"] = 1, [5, 9], [3, 4]
        if s == "runais":
            arr["pos"] = arr["outs"]
        if s == "runflex":
            arr["p"] = arr["outs"]
        guard = np.full(3 * dt.itemsize, 0xa5, np.uint8)
        ends = guard[:2 * dt.itemsize].view(dt)
        nr = C.c_size_t()
        rc = getattr(lib, f"mfm_hosttwin_{s}_end_stretches")(2, arr.ctypes.data, ends.ctypes.data, 2, C.byref(nr))
        assert rc == 0 and nr.value == 2 and (guard[2 * dt.itemsize:] == 0xa5).all()
        assert ends["channel"].tolist() == [0, 1] and ends["outs"].tolist() == [5, 9] and ends["run"].tolist() == [NO_RUN, NO_RUN]
        assert ends["stretch_window"].tolist() == [3, 4] and not arr.view(np.uint8).any()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"r{c[0]}_W{c[1]}_P{c[2]}")
def test_one_record_per_stretch_and_its_content_is_the_state(proto, cfg):
    """the twin's records over the calls and the end call are exactly the stretches of the run lists, in order, and each holds
    what a fresh plain twin fed that stretch alone is left with; the events beside them are the plain twin's"""
    sc = scene_calls(proto, cfg)
    calls, nch = sc["calls"], sc["nch"]
    want, pieces = stretches_of_runs(calls)
    # the scene is what it is meant to be
    assert len(want) >= 20 and max(len(r) for r, _ in calls) >= 3
    assert any(np.unique(r["channel"], return_counts=True)[1].max() >= 3 for r, _ in calls if len(r))   # three runs of a channel in a call
    assert any(w[0] < len(calls) and int(calls[w[0]][0]["channel"][w[4]]) == w[1] and
               (w[4] == 0 or int(calls[w[0]][0]["channel"][w[4] - 1]) != w[1]) for w in want)   # (a): ended by a first run
    if cfg[1] == 7:
        assert any((r["nr_out"] == 0).any() for r, _ in calls if len(r)) and any(w[3] == 0 for w in want)
    evs, ends, last = twin_stream(proto, calls, nch)
    got = np.concatenate(ends + [last])
    got_call = sum(([i] * len(e) for i, e in enumerate(ends + [last])), [])
    assert len(got) == len(want)
    assert got_call == [w[0] for w in want]
    for f, k in (("channel", 1), ("stretch_window", 2), ("outs", 3), ("run", 4)):
        assert got[f].tolist() == [w[k] for w in want], f
    # the events equal the plain twin's, and so does the state on the way
    plain, state = proto.new_state(nch), proto.new_state(nch)
    for i, (runs, payload) in enumerate(calls):
        e, _ = proto.call_ends(state, runs, payload)
        same_events(e, proto.call(plain, runs, payload), f"call {i}")
        same_events(e, evs[i], f"call {i} again")
        assert proto.states(state).tobytes() == proto.states(plain).tobytes()
    # content: the stretch alone through a fresh plain twin, then the mapping restated
    modes = set()
    for rec, w in zip(got, want):
        c, k = w[1], w[2]
        y = np.concatenate(pieces[(c, k)]) if pieces[(c, k)] else np.zeros(0, np.int16)
        fresh = proto.new_state(1)
        proto.call(fresh, np.array([(k, 0, 0, 0, y.size, 1, 0)], proto.b.RUNRS_RUN_DTYPE), y)
        exp = proto.record(proto.states(fresh)[0], c, w[4])
        same_records(np.array([rec]), np.array([exp]), f"stretch {(c, k)}")
        modes.add(int(rec["mode"]))
    assert 0 in modes


def test_designed_masks_cut_something(proto):
    """the stage's own mask that closes inside packets, batches and blocks: records with mode != 0, each equal to the state of the
    stretch alone (POCSAG: whole codewords of the cut batch, corrected)"""
    sc = designed_calls(proto)
    calls = sc["calls"]
    want, pieces = stretches_of_runs(calls)
    _, ends, last = twin_stream(proto, calls, sc["nch"])
    got = np.concatenate(ends + [last])
    assert len(got) == len(want)
    cut = got[got["mode"] != 0]
    assert len(cut) >= 2
    if proto.name == "runpocsag":
        assert (cut["nr_words"] >= 1).any() and (cut["nr_ok"] >= 1).any()
    if proto.name == "runflex":
        assert (cut["mode"] == 2).any()
    for rec, w in zip(got, want):
        y = np.concatenate(pieces[(w[1], w[2])])
        fresh = proto.new_state(1)
        proto.call(fresh, np.array([(w[2], 0, 0, 0, y.size, 1, 0)], proto.b.RUNRS_RUN_DTYPE), y)
        same_records(np.array([rec]), np.array([proto.record(proto.states(fresh)[0], w[1], w[4])]), f"stretch {(w[1], w[2])}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"r{c[0]}_W{c[1]}_P{c[2]}")
def test_records_do_not_depend_on_the_calls(proto, cfg):
    """the same stream in the seeded calls, as one call that holds everything (every stretch one run) and with a call at every
    run boundary: the same records per channel, `run` aside"""
    sc = scene_calls(proto, cfg)
    calls, nch = sc["calls"], sc["nch"]
    fields = [f for f in proto.end_dtype.names if f != "run"]
    whole = scene_calls(proto, cfg, single=True)["calls"]
    assert len(whole) == (2 if cfg[2] else 1) and (whole[0][0]["flags"] & 1).all()   # the second is the gate's flush
    ref = None
    for what, cs in (("seeded", calls), ("one call", whole), ("per run", per_run(calls))):
        _, ends, last = twin_stream(proto, cs, nch)
        got = np.concatenate(ends + [last])
        got = got[np.argsort(got["channel"], kind="stable")]   # per channel, stream order
        if ref is None:
            ref = got
        same_records(got, ref, what, fields)
        assert (np.concatenate(ends)["run"] != NO_RUN).all() and (last["run"] == NO_RUN).all()


def test_refused_calls_leave_no_record_and_no_trace(proto):
    """the refusal cases of the stage's own tests: MFM_E_STATE, no record, the state untouched, and the same input in calls that
    fit gives the records of a stream that was never refused; too small an array for the records moves nothing either"""
    b, mod = proto.b, proto.mod
    case = mod._refusal_case(proto.pkg, proto.ora)
    calls, at, cases, capacity = case[0], case[2], case[3], case[4]
    _, want, want_last = twin_stream(proto, calls, 2)
    assert sum(len(w) for w in want) + len(want_last) >= 2
    state = proto.new_state(2)
    got = []
    for i in range(at):
        got.append(proto.call_ends(state, *calls[i])[1])
    s0 = proto.copy(state)
    runs, payload = calls[at]
    for change, message, flags in list(cases) + list(capacity):
        kw = dict(runs=runs, payload=payload)
        kw.update(change)
        with pytest.raises(proto.pkg.MfmError) as ei:
            proto.call_ends(state, kw.pop("runs"), kw.pop("payload"), **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value))
        assert ei.value.needed_ends == 0 and proto.states(state).tobytes() == proto.states(s0).tobytes()
    for i in range(at, len(calls)):
        got.append(proto.call_ends(state, *calls[i])[1])
    for i, (g, w) in enumerate(zip(got, want)):
        same_records(g, w, f"call {i}")
    with pytest.raises(proto.pkg.MfmError) as ei:
        proto.twin_end(state, max_ends=len(want_last) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed_ends == len(want_last) and proto.states(state)["has_stretch"].any()
    same_records(proto.twin_end(state), want_last, "the end call")
    # a process call with records, into an array too small for them: the count needed, and nothing moves
    sc = scene_calls(proto, CONFIGS[1])
    _, want, _ = twin_stream(proto, sc["calls"], sc["nch"])
    j = next(i for i, w in enumerate(want) if len(w) >= 2)
    state = proto.new_state(sc["nch"])
    for i in range(j):
        proto.call_ends(state, *sc["calls"][i])
    s1 = proto.copy(state)
    with pytest.raises(proto.pkg.MfmError) as ei:
        proto.call_ends(state, *sc["calls"][j], max_ends=len(want[j]) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed_ends == len(want[j]) and proto.states(state).tobytes() == proto.states(s1).tobytes()
    same_records(proto.call_ends(state, *sc["calls"][j])[1], want[j], "the same call, right")


def test_run_ends_kernels_use_no_scratch():
    """the code object's notes of build/mfm_run_ends.o (tools/kernel_regs.py): the report's kernels for the three stages, no
    private segment, no spilled register; and the stages' own objects hold no kernel of the report"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_run_ends.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_run_ends.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    names = sorted(re.sub(r"<.*", "", ln.split()[0]) for ln in lines)
    assert names == sorted(["re_place_kernel"] * 3 + ["re_write_kernel"] * 2 + ["re_write_pocsag_kernel"] + ["re_flush_place_kernel"] * 3 +
                           ["re_flush_write_kernel"] * 2 + ["re_flush_write_pocsag_kernel"]), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ---------------------------------------------------------------------------------------------------------

def _feed(proto, torch, st, runs, payload, totals=None, bits=False):
    """one call from uploaded arrays: a burst resampler's result as it would stand in its device view, PCM or bits form"""
    if bits:
        rb, words = trb.pack(proto.pkg, runs, payload, proto.polarity)
        view, keep = trb._view_of(proto.pkg, torch, rb, words, proto.polarity, totals)
        st.process_bits_device(view)
    else:
        t = np.array([len(runs), payload.size, 0, 0] if totals is None else totals, np.uint64)
        keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
        st.process_device(*(k.data_ptr() for k in keep))
    return keep


def _stage(proto, calls, nch, report=True):
    max_runs = max(max(len(r) for r, _ in calls), 1)
    max_out = max(max(p.size for _, p in calls), 1)
    st = proto.Stage(nch, max_runs, max_out)
    if report:
        st.set_end_report(True)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [1, 3, 65])
def test_gpu_records_equal_the_twin_and_the_report_changes_nothing_else(proto, nch):
    """1, 3 and 65 channels (a second wave of the write kernels, a second block at 65 channels of POCSAG) under the random masks,
    every call cutting, a call without runs, a refused call in the middle: records and the two totals equal the twin's call by
    call; events, totals and state equal those of an object with the report off; the bits entries give the PCM entries' records;
    the end call records exactly the channels with a stretch and leaves every state zero"""
    import torch
    b = proto.b
    sc = scene_calls(proto, CONFIGS[1] if nch > 1 else CONFIGS[0], nch=nch, limit=600000)
    calls = sc["calls"]
    want, _ = stretches_of_runs(calls)
    assert len(want) >= 10 and any(len(r) == 0 for r, _ in calls)
    if nch != 3:   # three or more runs of one channel in a call
        assert any(np.unique(r["channel"], return_counts=True)[1].max() >= 3 for r, _ in calls if len(r))
    _, t_ends, t_last = twin_stream(proto, calls, nch)
    on, off = _stage(proto, calls, nch), _stage(proto, calls, nch, report=False)
    forms = [False] if proto.polarity is None else [False, True]
    twin = proto.new_state(nch)
    refuse_at = len(calls) // 2
    for i, (runs, payload) in enumerate(calls):
        if i == refuse_at:   # the resampler's overflow flag handed through: nothing comes out, nothing moves
            keep = _feed(proto, torch, on, runs, payload, totals=[len(runs), payload.size, 1, 0])
            with pytest.raises(proto.pkg.MfmError) as ei:
                on.fetch_ends()
            assert ei.value.code == b.MFM_E_STATE and "overflow or gate error" in str(ei.value)
            assert proto.fetch_states(on).tobytes() == proto.states(twin).tobytes()
            del keep
        bits = forms[i % len(forms)]
        keep = _feed(proto, torch, on, runs, payload, bits=bits)
        keep2 = _feed(proto, torch, off, runs, payload, bits=bits)
        got = on.fetch_ends()
        same_records(got, t_ends[i], f"call {i}")
        same_events(proto.fetch(on), proto.fetch(off), f"events of call {i}")
        proto.call(twin, runs, payload)
        s_on, s_off = proto.fetch_states(on), proto.fetch_states(off)
        assert s_on.tobytes() == s_off.tobytes() == proto.states(twin).tobytes(), f"state after call {i}"
        d_ends, d_t = on.ends_view()
        assert tl._d2h(d_t, 16).view(np.uint64).tolist() == [len(got), int((got["mode"] != 0).sum())], f"end totals of call {i}"
        if len(got):
            assert tl._d2h(d_ends, got.nbytes).tobytes() == got.tobytes()
        del keep, keep2
    on.end_stretches()
    got = on.fetch_ends()
    same_records(got, t_last, "the end call")
    assert got["channel"].tolist() == [c for c in range(nch) if proto.states(twin)["has_stretch"][c]]
    assert not proto.fetch_states(on).view(np.uint8).any()
    assert all(len(x) == 0 for x in proto.fetch(on))
    for o in (on, off):
        o.close()


@pytest.mark.gpu
def test_gpu_designed_cuts_equal_the_twin(proto):
    """the stage's own "cut" mask: the cut packets, batches and blocks as the twin reports them, POCSAG's corrected words included"""
    import torch
    sc = designed_calls(proto)
    calls, nch = sc["calls"], sc["nch"]
    _, t_ends, t_last = twin_stream(proto, calls, nch)
    assert (np.concatenate(t_ends + [t_last])["mode"] != 0).sum() >= 2
    st = _stage(proto, calls, nch)
    for i, (runs, payload) in enumerate(calls):
        keep = _feed(proto, torch, st, runs, payload)
        same_records(st.fetch_ends(), t_ends[i], f"call {i}")
        del keep
    st.end_stretches()
    same_records(st.fetch_ends(), t_last, "the end call")
    st.close()


@pytest.mark.gpu
def test_gpu_after_the_end_call_a_run_must_begin(proto):
    """behind the end call a continuing run is refused as out of step (the channel has no stretch) and a beginning run decodes
    as on a fresh object"""
    import torch
    b = proto.b
    sc = scene_calls(proto, CONFIGS[1])
    calls, nch = sc["calls"], sc["nch"]
    i = next(i for i, (r, _) in enumerate(calls) if len(r) and not (r["flags"] & 1).all())   # a call with a continuing run
    st = _stage(proto, calls, nch)
    twin = proto.new_state(nch)
    for runs, payload in calls[:i]:
        keep = _feed(proto, torch, st, runs, payload)
        st.fetch_ends()
        proto.call(twin, runs, payload)
        del keep
    st.end_stretches()
    ends = st.fetch_ends()
    assert len(ends) == int(proto.states(twin)["has_stretch"].sum()) >= 1
    runs, payload = calls[i]
    keep = _feed(proto, torch, st, runs, payload)
    with pytest.raises(proto.pkg.MfmError) as ei:
        st.fetch_ends()
    assert ei.value.code == b.MFM_E_STATE and "out of step" in str(ei.value)
    del keep
    # the same outputs as beginning runs: a fresh object's result
    begin = runs.copy()
    begin["flags"] |= 1
    begin["first_out"] = 0
    fresh_state = proto.new_state(nch)
    want_ev, want_ends = proto.call_ends(fresh_state, begin, payload)
    keep = _feed(proto, torch, st, begin, payload)
    same_events(proto.fetch(st), want_ev, "the beginning runs behind the end call")
    same_records(st.fetch_ends(), want_ends, "their records")
    assert proto.fetch_states(st).tobytes() == proto.states(fresh_state).tobytes()
    del keep
    st.close()


@pytest.mark.gpu
def test_gpu_accessors_and_their_order(proto):
    """report off: fetch_ends, end_stretches and ends_view are MFM_E_STATE; before the first call fetch_ends is MFM_E_STATE;
    set_end_report behind a process call is MFM_E_STATE; MFM_E_NOMEM says how many records there are"""
    import torch
    b = proto.b
    sc = scene_calls(proto, CONFIGS[1])
    calls, nch = sc["calls"], sc["nch"]
    _, t_ends, _ = twin_stream(proto, calls, nch)
    st = _stage(proto, calls, nch, report=False)
    for fn in (st.fetch_ends, st.end_stretches, st.ends_view):
        with pytest.raises(proto.pkg.MfmError) as ei:
            fn()
        assert ei.value.code == b.MFM_E_STATE and "report is off" in str(ei.value)
    st.set_end_report(True)
    st.set_end_report(False)
    st.set_end_report(True)
    with pytest.raises(proto.pkg.MfmError) as ei:
        st.fetch_ends()
    assert ei.value.code == b.MFM_E_STATE and "no call yet" in str(ei.value)
    j = next(i for i, e in enumerate(t_ends) if len(e) >= 2)
    for i in range(j + 1):
        keep = _feed(proto, torch, st, *calls[i])
        if i < j:
            st.fetch_ends()
        del keep
    with pytest.raises(proto.pkg.MfmError) as ei:
        st.fetch_ends(max_ends=len(t_ends[j]) - 1)
    assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(t_ends[j]) and not ei.value.buffer.view(np.uint8).any()
    same_records(st.fetch_ends(), t_ends[j], "fetched again")
    for on in (False, True):
        with pytest.raises(proto.pkg.MfmError) as ei:
            st.set_end_report(on)
        assert ei.value.code == b.MFM_E_STATE and "before the first process call" in str(ei.value)
    st.close()


@pytest.mark.gpu
def test_gpu_two_stages_on_two_streams(proto):
    """two objects fed the same calls on two streams of their own: both give the twin's records"""
    import torch
    sc = scene_calls(proto, CONFIGS[1])
    calls, nch = sc["calls"], sc["nch"]
    _, t_ends, t_last = twin_stream(proto, calls, nch)
    sts = [_stage(proto, calls, nch), _stage(proto, calls, nch)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, (runs, payload) in enumerate(calls[:40]):
        t = np.array([len(runs), payload.size, 0, 0], np.uint64)
        keep = (tr._up(torch, runs), tr._up(torch, payload), tr._up(torch, t))
        torch.cuda.synchronize()
        for st, s in zip(sts, streams):
            st.process_device(*(k.data_ptr() for k in keep), stream=s.cuda_stream)
        for st in sts:
            same_records(st.fetch_ends(), t_ends[i], f"call {i}")
        del keep
    for st, s in zip(sts, streams):
        st.end_stretches(stream=s.cuda_stream)
    for st in sts:
        assert len(st.fetch_ends()) >= 1
        st.close()


def _ends_lines(proto_name, ends, W):
    """the lines of ends.jsonl a list of records becomes, restated"""
    fields = {"runais": ("start_sample", "nr_bits"), "runpocsag": ("baud", "nr_words", "nr_bits", "nr_sync_bits", "nr_ok", "fail_mask"),
              "runflex": ("j", "eye", "coding", "fiw", "cycle", "frame")}[proto_name]
    out = []
    for e in ends:
        line = {"channel": int(e["channel"]), "first_sample": int(e["stretch_window"]) * W, "outs": int(e["outs"]), "mode": int(e["mode"])}
        line.update({f: int(e[f]) for f in fields})
        if proto_name == "runpocsag":
            line["corrected"] = ["%08x" % int(w) for w in e["corrected"][:int(e["nr_ok"])]]
        out.append(line)
    return out


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_ends_writes_the_records_of_the_twin(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-pocsag --gate-ends --summary as a fresh child process on the chain scene of
    tests/test_runpocsag.py: ends.jsonl holds the twin's records (per channel in stream order) and the summary its counts; the same
    through --gate-route with a pocsag route for channel 0 and an ais route for channel 1; and without --gate-ends there is no
    ends.jsonl, while every other file and stdout are byte for byte those of the run with it"""
    b = pkg.binding
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    fs, decim, W, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 929000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    route = dict(resample="4/5", taps=str(tmp_path / "filter.json"))
    (tmp_path / "routes.json").write_text(json.dumps({"routes": [dict(route, name="pocsag", stage="pocsag", channels=[0]),
                                                                 dict(route, name="ais", stage="ais", channels=[1])]}))
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
            str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(sc["thr"]),
            "--hang", str(s["hang"]), "--block", str(s["blk"]), "--gate-preroll", str(P)]
    single = ["--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-pocsag"]
    runs = {"plain": base + ["--gate-out", str(tmp_path / "plain")] + single,
            "ends": base + ["--gate-out", str(tmp_path / "ends")] + single + ["--gate-ends", "--summary"],
            "routed": base + ["--gate-out", str(tmp_path / "routed"), "--gate-route", str(tmp_path / "routes.json"), "--gate-ends", "--summary"]}
    out = {}
    for name, cmd in runs.items():
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = r.stdout.splitlines()
    # the twin over the oracle's resampled runs, as the tool's chain sees them: the whole stream, the gate's flush, the end call
    n = sc["pcm"].shape[1]
    rs = tr.Checker(pkg, ora, sc["rtaps"], 4, 5, False, W)
    calls = [rs.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n)), rs.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True))]
    want = {}
    for name in ("runpocsag", "runais"):
        proto = Proto(pkg, ora, name)
        _, ends, last = twin_stream(proto, calls, 2)
        recs = np.concatenate(ends + [last])
        want[name] = recs[np.argsort(recs["channel"], kind="stable")]
    assert len(want["runpocsag"]) >= 3 and len(want["runais"]) == len(want["runpocsag"])
    by_channel = lambda lines: sorted(lines, key=lambda ln: ln["channel"])   # stable: stream order within a channel
    got = [json.loads(ln) for ln in (tmp_path / "ends" / "ends.jsonl").read_text().splitlines()]
    assert by_channel(got) == _ends_lines("runpocsag", want["runpocsag"], W)
    names = {2: "batch", 3: "syncword"}
    cut = [int(m) for m in want["runpocsag"]["mode"] if m]
    summary = [json.loads(ln) for ln in out["ends"] if '"ends": true' in ln]
    assert summary == [{"summary": True, "ends": True, "stretches": len(got), "cut": len(cut),
                        "cut_by_mode": {k: sum(1 for m in cut if names[m] == k) for k in sorted(set(names[m] for m in cut))}}]
    # through the router: every route's stage reports its own channels
    got = [json.loads(ln) for ln in (tmp_path / "routed" / "pocsag" / "ends.jsonl").read_text().splitlines()]
    assert got == [ln for ln in _ends_lines("runpocsag", want["runpocsag"], W) if ln["channel"] == 0] and len(got) >= 1
    got = [json.loads(ln) for ln in (tmp_path / "routed" / "ais" / "ends.jsonl").read_text().splitlines()]
    assert got == [ln for ln in _ends_lines("runais", want["runais"], W) if ln["channel"] == 1] and len(got) >= 1
    routed = [json.loads(ln) for ln in out["routed"] if '"ends": true' in ln]
    assert [ln["route"] for ln in routed] == ["pocsag", "ais"] and routed[0]["stretches"] + routed[1]["stretches"] == len(want["runpocsag"])
    # without the flag: no ends.jsonl, and nothing else differs
    assert not (tmp_path / "plain" / "ends.jsonl").exists()
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(set(os.listdir(tmp_path / "ends")) - {"ends.jsonl"})
    for name in os.listdir(tmp_path / "plain"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "ends" / name).read_bytes(), name
    assert out["plain"] == [ln for ln in out["ends"] if '"summary": true' not in ln]
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "x"), "--gate-ends"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-ends needs" in r.stderr


# ---- designed cuts: one transmission, masks that differ only in where they close ------------------------------------

_DESIGNED = {}


def designed(pkg, ora, name, x, W, closes):
    """one channel, the stage's 1/1 resampler, open from window 0: per name in `closes` the mask closes at that window for good
    (None: never).  Returns {name: (calls, events of the stream, records of the stream with the end call's)}; made once"""
    if name not in _DESIGNED:
        proto = Proto(pkg, ora, name)
        taps = proto.mod.rs_taps(pkg, ora, proto.mod.RATIOS[1])
        nw = x.size // W
        out = {}
        for what, k in closes.items():
            m = np.ones((1, nw), bool)
            if k is not None:
                assert 0 < k < nw
                m[0, k:] = False
            third = nw // 3 * W
            calls = rs_calls(pkg, ora, x[None, :nw * W], m, W, 0, [third, third, nw * W - 2 * third], taps, 1, 1)
            evs, ends, last = twin_stream(proto, calls, 1)
            out[what] = (calls, [np.concatenate([e[i] for e in evs]) for i in range(len(evs[0]))], np.concatenate(ends + [last]))
        _DESIGNED[name] = out
    return _DESIGNED[name]


def ais_designed(pkg, ora):
    sy, W = pkg.synth, 64
    pl = tra.ta._payloads(sy)
    x = (np.random.RandomState(3).randn(12000) * 40).round().astype(np.int16)
    at = []
    for k in range(2):
        p = sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(pl[k])], lead_bits=5, trail_bits=4), noise=200, phase=k, seed=k)
        a = 1500 + 5000 * k
        x[a:a + p.size] = p
        at.append((a, a + p.size))
    assert at[0][1] + 1000 < at[1][0] and at[1][1] + 1000 < x.size
    closes = {"uncut": None, "inside": (at[1][0] + at[1][1]) // 2 // W, "gap": (at[0][1] + at[1][0]) // 2 // W}
    return designed(pkg, ora, "runais", x, W, closes)


def test_designed_ais_cuts(pkg, ora):
    """closed inside the second packet: RECEIVE, with the start_sample the uncut scene's event reports for that packet; closed in
    the gap between the packets: SEARCH"""
    d = ais_designed(pkg, ora)
    ev = d["uncut"][1][0]
    assert len(ev) == 2 and (ev["fcs_valid"] == 1).all() and len(d["uncut"][2]) == 1 and int(d["uncut"][2]["mode"][0]) == 0
    inside, gap = d["inside"][2], d["gap"][2]
    assert len(inside) == 1 and len(d["inside"][1][0]) == 1   # the first packet came, the second did not
    assert int(inside["mode"][0]) == 1 and int(inside["start_sample"][0]) == int(ev["start_sample"][1]) and int(inside["nr_bits"][0]) >= 32
    assert len(gap) == 1 and len(d["gap"][1][0]) == 1 and int(gap["mode"][0]) == 0 and int(gap["start_sample"][0]) == 0
    assert int(inside["outs"][0]) > int(gap["outs"][0]) > 0 and inside["run"][0] == gap["run"][0] == NO_RUN


def pocsag_designed(pkg, ora):
    sy, W, spb = pkg.synth, 64, 32   # 1200 baud at 38 400 Hz
    msgs = trp.tp._messages(sy)
    batches = sy.pocsag_batches(msgs + msgs)
    assert len(batches) >= 2
    bits = sy.pocsag_bits(batches[:2])
    lead = 1000
    x = np.concatenate([sy.pocsag_pcm(bits, 1200, noise=300, lead=lead, trail=6000, seed=4)])
    second = 576 + 544 + 32   # first bit of the second batch's word 0
    at = lambda bit: (lead + bit * spb) // W
    closes = {"uncut": None, "inside": at(second + 32 * 5 + 16), "later": at(second + 32 * 5 + 16) + 32 * spb // W,
              "sync": at(576 + 544 + 16), "idle": at(bits.size) + 4000 // W}
    return designed(pkg, ora, "runpocsag", x, W, closes), [int(w) & 0x7fffffff for w in batches[1]]


def test_designed_pocsag_cuts(pkg, ora):
    """1200 baud, two batches.  Closed inside the second: BATCH with nr_words >= 1 whole words, corrected to the codewords sent;
    closed 32 bit periods later: one word more; closed inside the sync slot behind the first batch: SYNCWORD; closed in the idle
    samples behind the transmission's SYNC_LOST: SEARCH"""
    d, sent = pocsag_designed(pkg, ora)
    ev = d["uncut"][1][0]
    assert int((ev["type"] == ora.EV_BATCH).sum()) == 2
    a, b2 = d["inside"][2], d["later"][2]
    assert len(a) == len(b2) == 1 and int((d["inside"][1][0]["type"] == ora.EV_BATCH).sum()) == 1
    nw = int(a["nr_words"][0])
    assert int(a["mode"][0]) == 2 and int(a["baud"][0]) == 1200 and 1 <= nw < 15
    assert a["corrected"][0][:nw].tolist() == sent[:nw] and not a["corrected"][0][nw:].any()
    assert int(a["nr_ok"][0]) == nw and int(a["fail_mask"][0]) == 0 and (a["raw"][0][:nw] & 0x7fffffff).tolist() == sent[:nw]
    assert int(b2["mode"][0]) == 2 and int(b2["nr_words"][0]) == nw + 1 and b2["corrected"][0][:nw + 1].tolist() == sent[:nw + 1]
    assert int(b2["nr_bits"][0]) == int(a["nr_bits"][0])
    s = d["sync"][2]
    assert len(s) == 1 and int(s["mode"][0]) == 3 and 1 <= int(s["nr_sync_bits"][0]) < 32 and int(s["nr_words"][0]) == 0
    assert not s["corrected"][0].any() and not s["raw"][0].any()
    i = d["idle"][2]
    assert len(i) == 1 and int(i["mode"][0]) == 0 and int(i["baud"][0]) == 0 and int((d["idle"][1][0]["type"] == ora.EV_BATCH).sum()) == 2


def flex_designed(pkg, ora):
    sy, W = pkg.synth, 64
    coding, cycle, frame = 1, 11, 93
    ph = {p: sy.flex_phase_words([dict(r) for r in trf.tf.RECORDS[:3]]) for p in sy.FLEX_CODINGS[coding]["phases"]}
    levels = sy.flex_frame_levels(coding, cycle, frame, ph)
    a = 2000
    x = sy.flex_pcm([levels], noise=300, seed=2, lead=a, trail=4000)
    x[:a] = np.random.RandomState(8).randint(-300, 300, a)
    closes = {"uncut": None, "idle": (a - 600) // W, "sync1": (a + 800) // W, "frame": (a + 12000) // W}
    return designed(pkg, ora, "runflex", x, W, closes), (coding, cycle, frame)


def test_designed_flex_cuts(pkg, ora):
    """closed between the frame information word and the end of the block: FRAME with the cycle and frame sent; closed before
    the FIW: SYNC1; closed in idle: SEARCH"""
    d, (coding, cycle, frame) = flex_designed(pkg, ora)
    ev = d["uncut"][1][0]
    assert len(ev) == 1 and int(ev["type"][0]) == trf.FRAME and (int(ev["cycle"][0]), int(ev["frame"][0])) == (cycle, frame)
    f = d["frame"][2]
    assert len(f) == 1 and len(d["frame"][1][0]) == 0   # the FRAME event never came
    assert (int(f["mode"][0]), int(f["coding"][0]), int(f["cycle"][0]), int(f["frame"][0])) == (2, coding, cycle, frame)
    assert int(f["j"][0]) == int(ev["sync_sample"][0]) and int(f["fiw"][0]) == int(ev["fiw"][0]) and int(f["eye"][0]) == int(ev["eye"][0])
    s = d["sync1"][2]
    assert len(s) == 1 and int(s["mode"][0]) == 1 and int(s["eye"][0]) >= 3 and (int(s["cycle"][0]), int(s["frame"][0]), int(s["fiw"][0])) == (0, 0, 0)
    i = d["idle"][2]
    assert len(i) == 1 and int(i["mode"][0]) == 0 and int(i["j"][0]) == 0 and int(i["eye"][0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGES)
def test_gpu_designed_transmissions_equal_the_twin(pkg, ora, name):
    """the cut, the idle and the uncut variants of the designed transmissions on the device: the twin's records"""
    import torch
    proto = Proto(pkg, ora, name)
    d = {"runais": ais_designed, "runpocsag": lambda p, o: pocsag_designed(p, o)[0], "runflex": lambda p, o: flex_designed(p, o)[0]}[name](pkg, ora)
    for what, (calls, _, want) in d.items():
        st = _stage(proto, calls, 1)
        got = []
        for runs, payload in calls:
            keep = _feed(proto, torch, st, runs, payload)
            got.append(st.fetch_ends())
            del keep
        st.end_stretches()
        got.append(st.fetch_ends())
        same_records(np.concatenate(got), want, what)
        st.close()
