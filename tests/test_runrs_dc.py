"""The burst resampler's DC blocker (mfm_runrs_set_dc_block, csrc/mfm_runrs_dc.hip): with it on, the outputs of a stretch are what
filter/dc_blocker.h returns on a fresh blocker applied to the stretch's resampled PCM, however the stream was cut into calls.

The checker is never the code under test: the restated gate (tests/test_gate.py, test_gate_preroll.py) and, stretch by stretch,
a fresh ora.Resampler(taps, I, D, dc_pole=pole, invert=...) - mfmo_resampler_feed followed by mfmo_dc_blocker_apply on its
blocker, as tests/oracle_lib.py does it - fed run by run, and each stretch once more in one piece to a fresh one.  Every
comparison is an equality."""
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
import test_resampler_forms as trf
import test_runpocsag as trp
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runrs_set_dc_block", "mfm_runrs_get_dc_block", "mfm_hosttwin_runrs_dc_call"]
RATIOS = [(4, 5, 81), (16, 25, 821)]   # interpolate, decimate, taps
WINDOWS = [1, 7, 64, 500]
POLES = [0.999, 0.5]
POLE_P = [(0.9999, 1), (0.999, 16), (0.9, 1638), (0.5, 8192), (0.0, 16384), (-0.99, 32604)]   # filter/dc_blocker.h:56
BAD_POLES = [float("nan"), float("inf"), -float("inf"), 3.5, -1.5]   # (1 - pole) * 16384 is no int16


# ---- the checker --------------------------------------------------------------------------------------------

def dfeed(ora, r, x):
    """mfmo_resampler_feed, then mfmo_dc_blocker_apply on the resampler's own blocker (oracle_lib.Resampler.feed, with room for
    what the pending samples add)"""
    y = tr.ofeed(ora, r, x)
    if y.size:
        ora.lib().mfmo_dc_blocker_apply(r.dc, ora.p16(y), y.size)
    return y


class DcChecker(tr.Checker):
    """test_runrs.Checker with a DC blocker behind every stretch's resampler"""

    def __init__(self, pkg, ora, taps, I, D, invert, W, pole):
        super().__init__(pkg, ora, taps, I, D, invert, W)
        self.pole = pole

    def fresh(self):
        r = self.ora.Resampler(self.taps, self.I, self.D, dc_pole=self.pole, invert=self.invert)
        assert r.dc is not None
        return r

    def call(self, gate_runs, gate_payload):
        runs, pieces, off = [], [], 0
        for g in gate_runs:
            c, k, nw, po = int(g["channel"]), int(g["first_window"]), int(g["nr_windows"]), int(g["payload_offset"])
            x = gate_payload[po:po + nw * self.W]
            st = self.chan.get(c)
            begins = st is None or st[1] != k
            if begins:
                st = self.chan[c] = [self.fresh(), k, 0, (c, k)]
                self.stretch[st[3]] = [[], []]
            y = dfeed(self.ora, st[0], x)
            runs.append((k, off, st[2], c, y.size, int(begins), 0))
            pieces.append(y)
            self.stretch[st[3]][0].append(x)
            self.stretch[st[3]][1].append(y)
            off += y.size
            st[1], st[2] = k + nw, st[2] + y.size
        payload = np.concatenate(pieces) if pieces else np.zeros(0, np.int16)
        return np.array(runs, self.pkg.binding.RUNRS_RUN_DTYPE), payload

    def stretches(self):
        """{(channel, first window): outputs}; each stretch once more through a fresh resampler and blocker in one piece"""
        out = {}
        for key, (xs, ys) in self.stretch.items():
            y = np.concatenate(ys)
            assert np.array_equal(y, dfeed(self.ora, self.fresh(), np.concatenate(xs))), key
            out[key] = y
        return out


def drive(chk, calls, call, what):
    """test_runrs.drive with the checker given: every gate call through call(i, gate_runs, gate_payload) and against the checker;
    returns {(channel, first window): outputs} put together from what the code under test returned"""
    got_by, cur = {}, {}
    for i, (gr, gp) in enumerate(calls):
        want = chk.call(gr, gp)
        got = call(i, gr, gp)
        tr.same(got, want, f"{what}, call {i}")
        for r in got[0]:
            c = int(r["channel"])
            if int(r["flags"]) & 1:
                cur[c] = (c, int(r["first_window"]))
                got_by[cur[c]] = []
            assert int(r["first_out"]) == sum(p.size for p in got_by[cur[c]])   # continues across calls
            got_by[cur[c]].append(got[1][int(r["out_offset"]):int(r["out_offset"]) + int(r["nr_out"])])
    want_by = chk.stretches()
    got_by = {k: (np.concatenate(v) if v else np.zeros(0, np.int16)) for k, v in got_by.items()}
    assert sorted(got_by) == sorted(want_by), what
    for k in want_by:
        assert np.array_equal(got_by[k], want_by[k]), (what, k)
    return got_by


def run_scenes(pkg, ora, W, ratio, pole, channels, make_call, seed):
    """the scenes of test_runrs.run_scenes: every mask, P = 0 and 2, random and full-scale values, invert, each stream in the seeded
    cut and as one call, with identical outputs per stretch"""
    I, D, nr_taps = ratio
    i = 0
    for nch in channels:
        for kind in tr.MASKS:
            if nch == 65 and kind not in ("open", "short"):
                continue
            for P in (0, 2):
                rng = np.random.RandomState(seed + 1000 * nch + 10 * tr.MASKS.index(kind) + P)
                full, invert = bool(i & 1), bool(i & 2)
                i += 1
                stream, mask, n, taps = tr.scene(rng, nch, W, kind, P, full, nr_taps)
                by_cut = []
                for single in (False, True):
                    cuts = tr.make_cuts(rng, n, W, single)
                    calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
                    what = f"W {W} {I}/{D} pole {pole} channels {nch} mask {kind} P {P} full {full} invert {invert} single {single}"
                    call, done = make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert, pole)
                    by_cut.append(drive(DcChecker(pkg, ora, taps, I, D, invert, W, pole), calls, call, what))
                    done()
                assert sorted(by_cut[0]) == sorted(by_cut[1]) == tr.stretches_of_mask(tr.emitted_of(mask, P)[:, :n // W])
                for k in by_cut[0]:
                    assert np.array_equal(by_cut[0][k], by_cut[1][k]), k   # cut independence
                if kind == "open":
                    assert len(by_cut[0]) == nch   # one stretch spanning every call
    assert i >= 4   # a full-scale stream among them


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_dc_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    m = re.search(r"struct mfm_runrs_dc_state \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(u?int\d+_t)\s+([\w, ]+);", m.group(1)) == [("int32_t", "x_n_1, y_n_1, acc"), ("uint32_t", "reserved")]
    assert list(b.RUNRS_DC_STATE_DTYPE.names) == ["x_n_1", "y_n_1", "acc", "reserved"] and b.RUNRS_DC_STATE_DTYPE.itemsize == 16
    assert C.sizeof(b.RunrsConfig) == 48
    assert pkg.RUNRS_DC_STATE_DTYPE is b.RUNRS_DC_STATE_DTYPE and pkg.hosttwin_runrs_dc_call is b.hosttwin_runrs_dc_call
    assert callable(pkg.RunResampler.set_dc_block) and callable(pkg.RunResampler.dc_block)


def _one_run(pkg, n, flags=1):
    return np.array([(0, 0, 0, 0, n, flags, 0)], pkg.binding.RUNRS_RUN_DTYPE)


def twin_p(pkg, pole):
    """the p the twin runs with: after the samples 1, 0 on a fresh blocker acc is -p (dc_blocker.h:82-86 with y_n_1 = 1)"""
    b = pkg.binding
    dc = np.zeros(1, b.RUNRS_DC_STATE_DTYPE)
    y = b.hosttwin_runrs_dc_call(pole, dc, _one_run(pkg, 2), np.array([1, 0], np.int16))
    assert int(y[0]) == 1 and int(dc["x_n_1"][0]) == 0
    return -int(dc["acc"][0])


def test_pole_becomes_the_p_of_the_full_row_resampler(pkg):
    b = pkg.binding
    taps = np.ones(81, np.int16)
    for pole, p in POLE_P:
        assert b.hosttwin_resampler_form(taps, 4, 5, 4096, dc_pole=pole)["dc_p"] == p
        assert twin_p(pkg, pole) == p, pole
    for pole in BAD_POLES:
        dc = np.zeros(1, b.RUNRS_DC_STATE_DTYPE)
        y = np.array([5, 6], np.int16)
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_dc_call(pole, dc, _one_run(pkg, 2), y)
        assert ei.value.code == b.MFM_E_INVAL and "pole" in str(ei.value)
        assert y.tolist() == [5, 6] and not dc.view(np.uint8).any()


def _twin_call(pkg):
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert, pole):
        state, pending = b.hosttwin_runrs_state(nch, len(taps), I)
        dc = np.zeros(nch, b.RUNRS_DC_STATE_DTYPE)

        def call(i, gr, gp):
            runs, payload = b.hosttwin_runrs_call(W, taps, I, D, state, pending, gr, gp, invert=invert)
            return runs, b.hosttwin_runrs_dc_call(pole, dc, runs, payload)

        return call, lambda: None

    return make_call


@pytest.mark.parametrize("pole", POLES)
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_hosttwin_equals_the_oracle_per_stretch(pkg, ora, W, ratio, pole):
    """csrc/mfm_runrs_dc.h through its host twin, behind the resampler's twin, on the scenes of the GPU test; 1 and 3 channels"""
    run_scenes(pkg, ora, W, ratio, pole, (1, 3), _twin_call(pkg), 7 * W + ratio[0])


def test_hosttwin_refuses_and_leaves_state_and_payload(pkg, ora):
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D, pole = 4, 5, 0.9
    calls = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    chk = DcChecker(pkg, ora, taps, I, D, False, W, pole)
    state, pending = b.hosttwin_runrs_state(nch, len(taps), I)
    dc = np.zeros(nch, b.RUNRS_DC_STATE_DTYPE)
    runs, payload = b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[0])
    tr.same((runs, b.hosttwin_runrs_dc_call(pole, dc, runs, payload)), chk.call(*calls[0]), "first call")
    assert dc[1]["y_n_1"] != 0   # a state that a refused call could spoil
    want = chk.call(*calls[1])
    assert [int(f) for f in want[0]["flags"]] == [0, 1, 1] and [int(c) for c in want[0]["channel"]] == [1, 1, 2]
    runs, payload = b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[1])
    assert (runs["nr_out"] > 0).all()
    d0, p0 = dc.copy(), payload.copy()
    cases = []
    bad = runs.copy()
    bad["flags"][1] = 0                       # a continuing run that is not its channel's first
    cases.append((bad, "not its channel's first"))
    bad = runs.copy()
    bad["nr_out"][2] += 1                     # a range beyond nr_elems
    cases.append((bad, "beyond the payload"))
    bad = runs.copy()
    bad["out_offset"][0] = payload.size + 1
    cases.append((bad, "beyond the payload"))
    bad = runs.copy()
    bad["channel"][2] = 0                     # a descending channel
    cases.append((bad, "do not ascend"))
    bad = runs.copy()
    bad["channel"][2] = nch
    cases.append((bad, "does not exist"))
    for bad, message in cases:
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_dc_call(pole, dc, bad, payload)
        assert ei.value.code == b.MFM_E_INVAL and "not a burst resampler's" in str(ei.value) and message in str(ei.value), str(ei.value)
        assert np.array_equal(dc, d0) and np.array_equal(payload, p0)   # a refused call changes nothing
    tr.same((runs, b.hosttwin_runrs_dc_call(pole, dc, runs, payload)), want, "second call")
    chk.stretches()


def test_hosttwin_run_without_output_changes_nothing(pkg):
    """a run with nr_out == 0 that continues leaves the state as it was; one that begins leaves zeros"""
    b = pkg.binding
    dc = np.zeros(2, b.RUNRS_DC_STATE_DTYPE)
    b.hosttwin_runrs_dc_call(0.9, dc, _one_run(pkg, 3), np.array([100, -7, 32767], np.int16))
    assert dc[0]["x_n_1"] == 32767 << 14 and dc[0]["y_n_1"] != 0 and dc[0]["acc"] != 0
    d0 = dc.copy()
    b.hosttwin_runrs_dc_call(0.9, dc, _one_run(pkg, 0, flags=0), np.zeros(0, np.int16))
    assert np.array_equal(dc, d0)
    b.hosttwin_runrs_dc_call(0.9, dc, _one_run(pkg, 0, flags=1), np.zeros(0, np.int16))
    assert not dc.view(np.uint8).any()


def test_dc_kernel_uses_no_scratch(pkg):
    """the code object's notes of build/mfm_runrs_dc.o (tools/kernel_regs.py): the one kernel, no private segment, no LDS, no
    spilled register, at most 128 VGPRs"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runrs_dc.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert [ln.split()[0] for ln in lines] == ["rr_dc_kernel"], out
    m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", lines[0])
    assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))) == (0, 0, 0, 0), lines[0]


# ---- what the feature is for: a paging carrier the receiver is tuned off -------------------------------------------

OFFSET = dict(ratio=(4, 5, 41), W=64, pole=0.999, offset=12000, kinds=("open", "fitted"), seed=64 * 7 + 4)
_OFFSET = {}


def _offset_scene(pkg, ora):
    """the (4, 5) POCSAG scene of tests/test_runpocsag.py at W = 64 with a constant added to the input of every transmission: the
    samples of a transmission are then all positive (+12000 on +-8000 and its noise stays inside int16), as behind a
    discriminator whose receiver is tuned off the carrier by more than the deviation.  Per mask the oracle's chain with the
    DC blocker (pole 0.999) and without it, in the seeded cut.  Made once and left unchanged"""
    if _OFFSET:
        return _OFFSET["it"]
    s = OFFSET
    I, D, _ = s["ratio"]
    W = s["W"]
    sc = dict(trp.scene(pkg, ora, s["ratio"], W))
    stream = sc["stream"].copy()
    for c, txs in sc["tx"].items():
        for t in txs:
            a, e = t[0] * D // I, t[1] * D // I
            x = stream[c, a:e].astype(np.int32) + s["offset"]
            assert x.min() > 0 and x.max() <= 32767   # no sign left to slice, and no clipping
            stream[c, a:e] = x.astype(np.int16)
    sc["stream"] = stream
    taps = trp.rs_taps(pkg, ora, s["ratio"])
    jobs = []
    for kind in s["kinds"]:
        rng = np.random.RandomState(s["seed"] + 10 * trp.kinds_of(W).index(kind))
        mask = trp.make_mask(kind, sc, W, rng)
        cuts = trp.tra.make_cuts(rng, sc["n_in"], W, trp.anchors_of(sc, W))
        calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
        res = {}
        for pole in (s["pole"], None):
            chk = trp.Checker(pkg, ora, taps, I, D, W)
            if pole is not None:
                chk.rs = DcChecker(pkg, ora, taps, I, D, False, W, pole)
            want = [chk.call(gr, gp) for gr, gp in calls]
            res[pole] = (want, chk.stretches())
        jobs.append(dict(kind=kind, mask=mask, cuts=cuts, calls=calls, want=res[s["pole"]][0], by=res[s["pole"]][1], by_plain=res[None][1]))
    _OFFSET["it"] = dict(sc=sc, taps=taps, jobs=jobs)
    return _OFFSET["it"]


def test_offset_scene_is_what_it_is_meant_to_be(pkg, ora):
    """from the oracle alone: with the blocker the chain finds at least three batches under every mask, on every channel that
    carries a transmission; without it there is no sync event at all"""
    it = _offset_scene(pkg, ora)
    sync = (ora.EV_SYNC_FOUND, ora.EV_SYNC_KEPT, ora.EV_SYNC_LOST, ora.EV_BATCH)
    carrying = [c for c, txs in it["sc"]["tx"].items() if txs]
    assert len(carrying) >= 3
    for job in it["jobs"]:
        ev = np.concatenate(list(job["by"].values()))
        assert int((ev["type"] == ora.EV_BATCH).sum()) >= 3, job["kind"]
        assert set(ev["channel"][ev["type"] == ora.EV_BATCH].tolist()) >= set(carrying), job["kind"]
        plain = np.concatenate(list(job["by_plain"].values()))
        assert not np.isin(plain["type"], sync).any(), (job["kind"], plain[["type", "channel", "sample"]][:8])


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gpu_call(pkg):
    """a real Gate (process_host, flush_device) in front of the stage with its blocker on"""
    def make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert, pole):
        cap = max(max(cuts), 1)
        gate = pkg.Gate(nch, cap, W, preroll_windows=P)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P, invert=invert)
        rr.set_dc_block(pole)
        pos = [0]

        def call(i, gr, gp):
            if i < len(cuts):
                m = cuts[i]
                gate.process_host(stream[:, pos[0]:pos[0] + m], tg.records_of(pkg, mask, pos[0] // W, (pos[0] + m) // W))
                pos[0] += m
            else:
                gate.flush_device()
            rr.process_device(*gate.device_view())
            return rr.fetch()

        def done():
            rr.close()
            gate.close()

        return call, done

    return make_call


@pytest.mark.gpu
@pytest.mark.parametrize("pole", POLES)
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_equals_the_oracle_per_stretch(pkg, ora, W, ratio, pole):
    """Gate -> RunResampler with the blocker on the device, on the scenes of the twin's test and with 65 channels (a second wave
    of the DC kernel with one live lane)"""
    run_scenes(pkg, ora, W, ratio, pole, (1, 3, 65), _gpu_call(pkg), 7 * W + ratio[0])


EDGE_NR_OUT = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 1000]
_EDGE = {}


def _edge_scene(pkg):
    """1/1 with the single tap 16384 (phase length 4: a stretch of L samples yields L - 4 outputs), W = 1, 72 channels, the call
    sequence of test_resampler_forms.DC_CALLS.  Channels 0 .. 12 open late in the first call so that their run there has the
    nr_out of EDGE_NR_OUT and continue to the end; 13 .. 33 have one closed sample inside the second call of 1000, at another
    place each: a continuing run and a beginning run of one channel in one call; 34 opens for three samples only; 35 .. 69 are open
    throughout; 70 is a constant +32767 and 71 alternates -32768 / 32767"""
    if _EDGE:
        return _EDGE["it"]
    sizes = [trf.DC_CALLS[0] + 4] + trf.DC_CALLS[1:]
    n, nch = sum(sizes), 72
    starts = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.RandomState(17)
    stream = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
    stream[70] = 32767
    stream[71] = np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    mask = np.ones((nch, n), bool)
    for c, t in enumerate(EDGE_NR_OUT):
        mask[c, :sizes[0] - (t + 4)] = False
    k13 = sizes.index(1000)
    assert k13 == 13 and sizes[k13] == 1000
    for c in range(13, 34):
        mask[c, starts[k13] + 60 + 43 * (c - 13)] = False
    mask[34] = False
    mask[34, starts[2] + 5:starts[2] + 8] = True
    calls = tr.gate_calls(pkg, stream, mask, 1, 0, sizes)
    _EDGE["it"] = dict(sizes=sizes, stream=stream, mask=mask, calls=calls, nch=nch, taps=np.array([16384], np.int16))
    return _EDGE["it"]


@pytest.mark.gpu
@pytest.mark.parametrize("pole,p", POLE_P)
def test_gpu_blocker_alone_at_its_edges(pkg, ora, pole, p):
    import torch
    sc = _edge_scene(pkg)
    chk = DcChecker(pkg, ora, sc["taps"], 1, 1, False, 1, pole)
    rr = pkg.RunResampler(sc["nch"], sc["taps"], 1, 1, 1, max_in_samples=max(sc["sizes"]))
    assert rr.dc_block() == (False, 0)
    rr.set_dc_block(pole)
    assert rr.dc_block() == (True, p)
    seen, residues, long_residues = set(), set(), set()

    def call(i, gr, gp):
        runs, payload = tr._fed(pkg, torch, rr, gr, gp)
        seen.update(int(x) for x in runs["nr_out"])
        residues.update(int(r["out_offset"]) % 8 for r in runs if r["nr_out"])
        long_residues.update(int(r["out_offset"]) % 8 for r in runs if r["nr_out"] >= 63)
        if i == 0:
            assert len(runs) >= 70   # a second wave with few live lanes
        return runs, payload

    by = drive(chk, sc["calls"], call, f"pole {pole}")
    rr.close()
    assert seen >= set(EDGE_NR_OUT), sorted(set(EDGE_NR_OUT) - seen)
    assert residues == set(range(8)) and long_residues == set(range(8))
    assert by[(70, 0)].size == sum(trf.DC_CALLS) and by[(71, 0)].size == sum(trf.DC_CALLS)
    # y leaves int16 on the alternating channel: the stored low 16 bits are not the clipped value
    x = sc["stream"][71].astype(np.int64)
    assert abs(int(x[1]) - int(x[0])) > 32767
    assert len([k for k in by if k[0] == 13]) == 2 and by[(34, int(np.flatnonzero(sc["mask"][34])[0]))].size == 0


@pytest.mark.gpu
def test_gpu_three_runs_of_a_channel_in_one_call(pkg, ora):
    """channel 0 has three runs in the middle call: the first continues the stretch of the call before, the other two begin, and
    the next call continues the third; channel 1 has no run in the middle call; channel 2 is open throughout"""
    import torch
    W, I, D, pole, nch = 16, 4, 5, 0.999, 3
    rng = np.random.RandomState(9)
    taps = rng.randint(-8191, 8192, 81).astype(np.int16)
    stream = rng.randint(-32768, 32768, size=(nch, 30 * W)).astype(np.int16)
    mask = np.zeros((nch, 30), bool)
    mask[0, 6:13] = mask[0, 14:16] = mask[0, 17:25] = True
    mask[1, 3:9] = mask[1, 22:28] = True
    mask[2] = True
    calls = tr.gate_calls(pkg, stream, mask, W, 0, [10 * W] * 3)
    chk = DcChecker(pkg, ora, taps, I, D, False, W, pole)
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=10 * W)
    rr.set_dc_block(pole)
    got = []

    def call(i, gr, gp):
        got.append(tr._fed(pkg, torch, rr, gr, gp))
        return got[-1]

    by = drive(chk, calls, call, "three runs")
    rr.close()
    mid, last = got[1][0], got[2][0]
    assert [(int(r["channel"]), int(r["flags"])) for r in mid] == [(0, 0), (0, 1), (0, 1), (2, 0)] and (mid["nr_out"] > 0).all()
    assert [(int(r["channel"]), int(r["flags"])) for r in last] == [(0, 0), (1, 1), (2, 0)]
    assert sorted(by) == [(0, 6), (0, 14), (0, 17), (1, 3), (1, 22), (2, 0)]


@pytest.mark.gpu
def test_gpu_refusals(pkg, ora):
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D, pole = 4, 5, 0.9
    first, second = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    whole = tr.gate_calls(pkg, stream, mask, W, 0, [30])[0]
    assert whole[1].size == 5 * W and second[1].size == 4 * W
    # an overflowing call raises its flag and writes nothing; the DC state did not move: the next call continues channel 1's stretch
    rr = pkg.RunResampler(nch, taps, I, D, W, max_windows=4, max_runs=8)
    rr.set_dc_block(pole)
    chk = DcChecker(pkg, ora, taps, I, D, False, W, pole)
    want = chk.call(*first)
    assert want[1].size and want[1].any()
    tr.same(tr._fed(pkg, torch, rr, *first), want, "first call")
    with pytest.raises(pkg.MfmError) as ei:
        rr.set_dc_block(0.5)
    assert ei.value.code == b.MFM_E_STATE and "before the first process call" in str(ei.value)
    with pytest.raises(pkg.MfmError) as ei:
        rr.set_dc_block(None)
    assert ei.value.code == b.MFM_E_STATE and rr.dc_block() == (True, 1638)
    for _ in range(2):   # twice: the two state buffers are used in turn
        with pytest.raises(pkg.MfmError) as ei:
            tr._fed(pkg, torch, rr, *whole)
        assert ei.value.code == b.MFM_E_STATE and "max_windows or max_runs" in str(ei.value)
        assert ei.value.needed == (0, 0) and not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
    # a bits call with the blocker on
    keep = (tr._up(torch, second[0]), tr._up(torch, second[1]), tr._up(torch, np.array([len(second[0]), second[1].size, 0, 0], np.uint64)))
    with pytest.raises(pkg.MfmError) as ei:
        rr.process_bits_device(*(k.data_ptr() for k in keep), b.MFM_BITS_NEG)
    assert ei.value.code == b.MFM_E_INVAL and "DC blocker" in str(ei.value)
    del keep
    want = chk.call(*second)
    assert [int(f) for f in want[0]["flags"]] == [0, 1, 1] and int(want[0]["nr_out"][0]) > 0
    tr.same(tr._fed(pkg, torch, rr, *second), want, "second call after the refused ones")
    chk.stretches()
    rr.close()
    # a bad pole
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=30)
    for bad in BAD_POLES:
        with pytest.raises(pkg.MfmError) as ei:
            rr.set_dc_block(bad)
        assert ei.value.code == b.MFM_E_INVAL and "pole" in str(ei.value)
        assert rr.dc_block() == (False, 0)
    # switched on and off again: the bits of an object never touched
    rr.set_dc_block(pole)
    rr.set_dc_block(None)
    assert rr.dc_block() == (False, 0)
    untouched = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=30)
    plain = tr.Checker(pkg, ora, taps, I, D, False, W)
    for i, call in enumerate((first, second)):
        got, ref = tr._fed(pkg, torch, rr, *call), tr._fed(pkg, torch, untouched, *call)
        tr.same(got, ref, f"call {i} beside an object never touched")
        tr.same(got, plain.call(*call), f"call {i} without the blocker")
    rr.close()
    untouched.close()


@pytest.mark.gpu
def test_gpu_offset_carrier_decodes_behind_the_blocker(pkg, ora):
    """Gate -> RunResampler with pole 0.999 -> RunPocsag on the device views, on the scene whose transmissions have no sign left:
    the events are the oracle chain's per stretch (DC-blocked resampler into a fresh POCSAG decoder)"""
    it = _offset_scene(pkg, ora)
    s, sc, taps = OFFSET, it["sc"], it["taps"]
    I, D, _ = s["ratio"]
    W, stream = s["W"], it["sc"]["stream"]
    for job in it["jobs"]:
        cuts, mask = job["cuts"], job["mask"]
        cap = max(max(cuts), 1)
        gate = pkg.Gate(trp.NCH, cap, W)
        rr = pkg.RunResampler(trp.NCH, taps, I, D, W, max_in_samples=cap)
        rr.set_dc_block(s["pole"])
        rp = pkg.RunPocsag.behind(rr)
        pos, got_by = 0, {}
        for i, (m, (rs_want, ev_want)) in enumerate(zip(cuts, job["want"])):
            gate.process_host(stream[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W))
            pos += m
            rr.process_device(*gate.device_view())
            rp.process_device(*rr.device_view())
            got = rp.fetch()
            trp.same(got, ev_want, f"mask {job['kind']}, call {i}")
            tr.same(rr.fetch(), rs_want, f"mask {job['kind']}, the resampler's call {i}")
            for e in got:
                got_by.setdefault((int(e["channel"]), int(e["stretch_window"])), []).append(e)
        for o in (rp, rr, gate):
            o.close()
        assert sum(len(v) for v in got_by.values()) == sum(len(v) for v in job["by"].values())
        for k, v in job["by"].items():
            g = got_by.get(k, [])
            assert len(g) == len(v), (job["kind"], k)
            for a, e in zip(g, v):
                assert all(np.array_equal(a[f], e[f]) for f in trp.EVENT_FIELDS if f != "run"), (job["kind"], k)


def _chain_want_dc(pkg, ora, pole):
    """test_runpocsag._chain_want with the DC blocker behind every stretch's resampler"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    W, P = s["W"], s["P"]
    chk = trp.Checker(pkg, ora, sc["rtaps"], 4, 5, W)
    chk.rs = DcChecker(pkg, ora, sc["rtaps"], 4, 5, False, W, pole)
    n = sc["pcm"].shape[1]
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, 0, n))
    chk.call(*tgp.restate_pre(pkg, sc["pcm"], sc["mask"], W, 1, P, n, 0, flush=True))
    return chk, chk.stretches()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_dc_pole_writes_the_events_of_the_dc_blocked_chain(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-resample 4/5 --gate-dc-pole 0.999 --gate-pocsag as a fresh child process on the chain scene
    of tests/test_runpocsag.py: pocsag.jsonl holds the oracle's events for the DC-blocked chain; with --gate-bits the tool refuses"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    fs, decim, W, P, pole = s["fs"], s["decim"], s["W"], s["P"], 0.999
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
           "--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-dc-pole", str(pole), "--gate-pocsag"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    chk, by = _chain_want_dc(pkg, ora, pole)
    want = sorted((int(e["channel"]), k[1] * W, int(e["type"]), int(e["baud"]), int(e["sample"]), int(e["aux"]), int(e["nr_ok"]),
                   int(e["fail_mask"]), tuple("%08x" % int(w) for w in e["corrected"]) if int(e["type"]) == ora.EV_BATCH else ())
                  for k, v in by.items() for e in v)
    assert len(want) >= 9
    lines = [json.loads(ln) for ln in (tmp_path / "gated" / "pocsag.jsonl").read_text().splitlines()]
    got = sorted((ln["channel"], ln["first_sample"], ln["type"], ln["baud"], ln["sample"], ln["aux"], ln["nr_ok"], ln["fail_mask"],
                  tuple(ln["corrected"])) for ln in lines)
    assert got == want
    # the resampled samples on disk are the blocked ones
    for c in sorted({k[0] for k in chk.rs.stretch}):
        blocked = np.concatenate([np.concatenate(chk.rs.stretch[k][1]) for k in sorted(chk.rs.stretch) if k[0] == c])
        assert np.array_equal(np.fromfile(tmp_path / "gated" / f"ch{c:04d}.rs.s16", np.int16), blocked), c
    r = subprocess.run(cmd + ["--gate-bits"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-dc-pole and --gate-bits exclude each other" in r.stderr
    r = subprocess.run([a for a in cmd if a not in ("--gate-resample", "4/5")], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-dc-pole needs --gate-resample" in r.stderr
