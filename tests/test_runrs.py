"""The burst resampler (mfm_runrs_*, csrc/mfm_runrs.hip): the runs the squelch gate left in its payload go through the rational
resampler, one fresh resampler per stretch of consecutive windows of a channel.

The checker is the numpy restatement of the gate rule (tests/test_gate.py, tests/test_gate_preroll.py) plus the oracle's
mfmo_resampler_feed per stretch through tests/oracle_lib.py: a run that follows on its channel's last run is fed to the same
oracle resampler, any other run to a fresh one, and every stretch is fed once more in one piece to a fresh resampler.  It is
never the code under test, and every comparison is an equality."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runrs_create", "mfm_runrs_destroy", "mfm_runrs_process_device", "mfm_runrs_fetch", "mfm_runrs_device_view",
             "mfm_hosttwin_runrs_plan", "mfm_hosttwin_runrs_call", "mfm_runrs_fetch_state", "mfm_runrs_store_state",
             "mfm_hosttwin_runrs_state_check"]
RATIOS = [(4, 5, 81), (16, 25, 821), (3, 7, 10), (1, 1, 4), (5, 2, 23)]   # interpolate, decimate, taps
WINDOWS = [1, 7, 64, 500]
MASKS = ["closed", "open", "short", "handover", "three"]
KB = 10   # the seeded cut has a call that ends with window KB - 1 and one of 13 windows behind it


# ---- the checker --------------------------------------------------------------------------------------------

def plen_of(nr_taps, I):
    return ((nr_taps + I - 1) // I + 3) & ~3


def ofeed(ora, r, x):
    """mfmo_resampler_feed with room for what the pending samples add (oracle_lib.Resampler.feed sizes for the new ones)"""
    x = np.ascontiguousarray(x, dtype=np.int16).copy()
    if r.invert:
        x = (-x.astype(np.int32)).astype(np.int16)   # decoder.c:624 on int16 storage
    cap = (x.size + r.phase_len()) * r.interp // r.decim + 8
    out = np.zeros(cap, np.int16)
    n = ora.lib().mfmo_resampler_feed(r.h, ora.p16(x), x.size, ora.p16(out), cap)
    assert n < cap
    return out[:n].copy()


class Checker:
    """what the stage must return for the gate calls of one stream, from the oracle"""

    def __init__(self, pkg, ora, taps, I, D, invert, W):
        self.pkg, self.ora, self.taps, self.I, self.D, self.invert, self.W = pkg, ora, taps, I, D, invert, W
        self.chan = {}       # channel -> [oracle resampler, window expected next, outputs so far, key of the stretch]
        self.stretch = {}    # (channel, first window) -> [samples fed, expected outputs by run]

    def call(self, gate_runs, gate_payload):
        runs, pieces, off = [], [], 0
        for g in gate_runs:
            c, k, nw, po = int(g["channel"]), int(g["first_window"]), int(g["nr_windows"]), int(g["payload_offset"])
            x = gate_payload[po:po + nw * self.W]
            st = self.chan.get(c)
            begins = st is None or st[1] != k
            if begins:
                st = self.chan[c] = [self.ora.Resampler(self.taps, self.I, self.D, invert=self.invert), k, 0, (c, k)]
                self.stretch[st[3]] = [[], []]
            y = ofeed(self.ora, st[0], x)
            runs.append((k, off, st[2], c, y.size, int(begins), 0))
            pieces.append(y)
            self.stretch[st[3]][0].append(x)
            self.stretch[st[3]][1].append(y)
            off += y.size
            st[1], st[2] = k + nw, st[2] + y.size
        payload = np.concatenate(pieces) if pieces else np.zeros(0, np.int16)
        return np.array(runs, self.pkg.binding.RUNRS_RUN_DTYPE), payload

    def stretches(self):
        """{(channel, first window): outputs}; each stretch once more through a fresh resampler in one piece"""
        out = {}
        for key, (xs, ys) in self.stretch.items():
            y = np.concatenate(ys)
            whole = ofeed(self.ora, self.ora.Resampler(self.taps, self.I, self.D, invert=self.invert), np.concatenate(xs))
            assert np.array_equal(y, whole), key
            n = sum(x.size for x in xs)
            if n <= plen_of(len(self.taps), self.I):
                assert y.size == 0
            out[key] = y
        return out


def same(got, want, what):
    (gr, gp), (wr, wp) = got, want
    assert gr.shape == wr.shape, (what, gr.shape, wr.shape)
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert bad.size == 0, f"{what}: run field {f} differs at {bad[:5].tolist()}: {gr[f][bad[0]]} != {wr[f][bad[0]]}"
    assert gp.shape == wp.shape, (what, gp.shape, wp.shape)
    bad = np.flatnonzero(gp != wp)
    assert bad.size == 0, f"{what}: payload differs at {bad[:5].tolist()} of {wp.size}: {gp[bad[:5]]} != {wp[bad[:5]]}"


# ---- scenes ---------------------------------------------------------------------------------------------------

def make_taps(rng, nr_taps, full):
    if full:
        return np.where(rng.rand(nr_taps) < 0.5, -32767, 32767).astype(np.int16)
    return rng.randint(-8191, 8192, nr_taps).astype(np.int16)


def make_stream(rng, nch, n, full):
    if full:   # +-32767 and -32768 against taps of +-32767: the int32 sum of a phase wraps
        return rng.choice(np.array([32767, -32767, -32768], np.int16), size=(nch, n))
    return rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)


def make_cuts(rng, n, W, single):
    """piece lengths that add up to n.  single: one call that holds everything.  Otherwise nr_in = 0, three calls in a row
    shorter than W, a call that ends exactly with window KB - 1, one of 13 windows, then zeros, pieces below W and longer ones"""
    if single:
        return [n]
    short = [int(rng.randint(1, W)) if W > 1 else 0 for _ in range(3)]
    out = [0] + short + [KB * W - sum(short), 13 * W]
    assert sum(short) < KB * W
    pos = sum(out)
    while pos < n:
        kind = int(rng.randint(0, 4))
        m = [0, int(rng.randint(1, max(2, W))), W - pos % W, int(rng.randint(W, 9 * W + 1))][kind]
        m = min(m, n - pos)
        out.append(m)
        pos += m
    return out


def make_mask(kind, rng, nch, nw, P):
    """raw squelch verdicts [C][nw]; with pre-roll P the gate emits their dilation.  The seeded cut's fifth call emits the
    windows up to KB - 1 - P and its sixth the 13 windows behind"""
    m = np.zeros((nch, nw), bool)
    if kind == "closed":
        return m
    if kind == "open":
        return ~m
    if kind == "short":   # emitted stretches of 1 - 3 windows (P = 0), closed gaps of 1 - 3 + P
        for c in range(nch):
            k = int(rng.randint(0, 3))
            while k < nw:
                ln = int(rng.randint(1, 4))
                m[c, k:k + ln] = True
                k += ln + P + int(rng.randint(1, 4))
        return m
    c0, c1 = 0, min(1, nch - 1)
    if kind == "handover":   # a stretch ends with the last window one call emits, the neighbour's begins with the next call's first
        m[c0, KB - 2 - P:KB - P] = True
        m[c1, KB + (2 if c1 == c0 else 0):KB + 3] = True
        return m
    assert kind == "three"   # three runs of one channel in the call of 13 windows, and a stretch across its end
    m[nch - 1, [KB + 1, KB + 5, KB + 9]] = True
    m[0, KB + 11:KB + 15] = True
    return m


def emitted_of(mask, P):
    return tgp.dilate(mask, P) if P else mask


def gate_calls(pkg, stream, mask, W, P, cuts):
    """the restated gate result of every call, and of the flush when P > 0"""
    pos, out = 0, []
    for m in cuts:
        out.append(tgp.restate_pre(pkg, stream, mask, W, 1, P, pos, m) if P else tg.restate_call(pkg, stream, mask, W, 1, pos, m))
        pos += m
    if P:
        out.append(tgp.restate_pre(pkg, stream, mask, W, 1, P, pos, 0, flush=True))
    return out


def drive(pkg, ora, calls, taps, I, D, invert, W, call, what):
    """every gate call through call(i, gate_runs, gate_payload) and against the checker; returns {(channel, first window): outputs}
    put together from what the code under test returned"""
    chk = Checker(pkg, ora, taps, I, D, invert, W)
    got_by = {}
    cur = {}
    for i, (gr, gp) in enumerate(calls):
        want = chk.call(gr, gp)
        got = call(i, gr, gp)
        same(got, want, f"{what}, call {i}")
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


def stretches_of_mask(emitted):
    keys = []
    for c in range(emitted.shape[0]):
        e = np.concatenate([[False], emitted[c], [False]])
        keys += [(c, int(k)) for k in np.flatnonzero(e[1:] & ~e[:-1])]
    return sorted(keys)


def scene(rng, nch, W, kind, P, full, nr_taps):
    nw = int(rng.randint(40, 61))
    n = nw * W + W // 2
    stream = make_stream(rng, nch, n, full)
    mask = make_mask(kind, rng, nch, nw, P)
    return stream, mask, n, make_taps(rng, nr_taps, full)


def run_scenes(pkg, ora, W, ratio, channels, make_call, seed):
    """every mask, P = 0 and 2, both kinds of values and invert, each stream in the seeded cut and as one call"""
    I, D, nr_taps = ratio
    i = 0
    for nch in channels:
        for kind in MASKS:
            if nch == 65 and kind not in ("open", "short"):
                continue
            for P in (0, 2):
                rng = np.random.RandomState(seed + 1000 * nch + 10 * MASKS.index(kind) + P)
                full, invert = bool(i & 1), bool(i & 2)
                i += 1
                stream, mask, n, taps = scene(rng, nch, W, kind, P, full, nr_taps)
                by_cut = []
                for single in (False, True):
                    cuts = make_cuts(rng, n, W, single)
                    calls = gate_calls(pkg, stream, mask, W, P, cuts)
                    what = f"W {W} {I}/{D} channels {nch} mask {kind} P {P} full {full} invert {invert} single {single}"
                    call, done = make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert)
                    by_cut.append(drive(pkg, ora, calls, taps, I, D, invert, W, call, what))
                    done()
                # cut independence: the same stretches with the same outputs, and they are the emitted mask's
                assert sorted(by_cut[0]) == sorted(by_cut[1]) == stretches_of_mask(emitted_of(mask, P)[:, :n // W])
                for k in by_cut[0]:
                    assert np.array_equal(by_cut[0][k], by_cut[1][k]), k
                if kind == "closed":
                    assert not by_cut[0]
                if kind == "open":
                    assert len(by_cut[0]) == nch   # one stretch spanning every call
                if kind == "short" and P == 0 and 3 * W <= plen_of(nr_taps, I):
                    assert by_cut[0] and all(v.size == 0 for v in by_cut[0].values())   # stretches shorter than plen + 1 samples
    assert i >= 4


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runrs_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src)
    assert b.RUNRS_RUN_DTYPE.itemsize == 40 and C.sizeof(b.RunrsRun) == 40
    assert b.RUNRS_STATE_DTYPE.itemsize == 24 and C.sizeof(b.RunrsConfig) == 48
    assert pkg.RUNRS_RUN_DTYPE is b.RUNRS_RUN_DTYPE and pkg.RunResampler is b.RunResampler and pkg.hosttwin_runrs_call is b.hosttwin_runrs_call
    m = re.search(r"struct mfm_runrs_run \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [
        ("uint64_t", "first_window"), ("uint64_t", "out_offset"), ("uint64_t", "first_out"), ("uint32_t", "channel"),
        ("uint32_t", "nr_out"), ("uint32_t", "flags"), ("uint32_t", "reserved")]
    assert list(b.RUNRS_RUN_DTYPE.names) == [n for n, _ in b.RunrsRun._fields_]
    m = re.search(r"struct mfm_runrs_config \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == [n for n, _ in b.RunrsConfig._fields_]
    m = re.search(r"struct mfm_runrs_state \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == list(b.RUNRS_STATE_DTYPE.names)
    m = re.search(r"#define\s+MFM_RUNRS_MAX_LDS_BYTES\s+(\d+)u?\b", src)
    assert m and int(m.group(1)) == b.MFM_RUNRS_MAX_LDS_BYTES


def walk(I, D, plen, phase, tot):
    """the oracle's loop (oracle/mfm_oracle.c:616-626) on arrays of cases: (outputs, phase, pending) left behind"""
    phase, tot = phase.astype(np.int64).copy(), tot.astype(np.int64)
    pos, n = np.zeros_like(tot), np.zeros_like(tot)
    while True:
        go = tot - pos > plen
        if not go.any():
            return n, phase, tot - pos
        n += go
        phase = np.where(go, phase + D, phase)
        pos += np.where(go, phase // I, 0)
        phase = np.where(go, phase % I, phase)
        assert (pos <= tot).all()


@pytest.mark.parametrize("plen", [4, 8, 52])
def test_closed_form_equals_a_plain_walk(pkg, ora, plen):
    """nr_out and the state left behind for I, D in 1 .. 9, every starting phase, 0 .. plen pending samples and runs of
    0 .. 3 plen + 2 samples.  The walk depends on phase and pending + run only, so it is done once per pair and compared with
    the closed form of every (pending, run) that adds up to it"""
    b = pkg.binding
    cases = 0
    for I in range(1, 10):
        for D in range(1, 10):
            if (D + I - 1) // I > plen:
                continue
            ph, pe, ns = [a.reshape(-1) for a in np.meshgrid(np.arange(I), np.arange(plen + 1), np.arange(3 * plen + 3), indexing="ij")]
            tph, ttot = [a.reshape(-1) for a in np.meshgrid(np.arange(I), np.arange(4 * plen + 3), indexing="ij")]
            wn, wph, wpe = walk(I, D, plen, tph, ttot)
            at = ph * (4 * plen + 3) + pe + ns
            n, pho, peo = b.hosttwin_runrs_plan(I, D, plen, ph, pe, ns)
            assert np.array_equal(n, wn[at]) and np.array_equal(pho, wph[at]) and np.array_equal(peo, wpe[at]), (I, D)
            assert (peo <= plen).all()
            cases += ph.size
    assert cases > 81 * (plen + 1) * (3 * plen + 3)
    # and the walk is the oracle's: a fresh resampler fed chunk by chunk produces what the chain of closed forms says
    rng = np.random.RandomState(plen)
    for I, D in ((4, 5), (5, 2), (3, 7), (1, 1), (9, 4)):
        taps = rng.randint(-100, 100, I * plen - 1).astype(np.int16)
        r = ora.Resampler(taps, I, D)
        assert r.phase_len() == plen
        phase = pending = 0
        for _ in range(40):
            m = int(rng.randint(0, 3 * plen + 3))
            n, pho, peo = b.hosttwin_runrs_plan(I, D, plen, [phase], [pending], [m])
            assert ofeed(ora, r, rng.randint(-9, 9, m).astype(np.int16)).size == int(n[0])
            phase, pending = int(pho[0]), int(peo[0])


def test_closed_form_refuses_what_is_out_of_range(pkg):
    b = pkg.binding
    for args in ((0, 1, 4, [0], [0], [1]), (1, 0, 4, [0], [0], [1]), (1, 9, 4, [0], [0], [1]), (4, 5, 8, [4], [0], [1]), (4, 5, 8, [0], [9], [1])):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_plan(*args)
        assert ei.value.code == b.MFM_E_INVAL


def _twin_call(pkg):
    b = pkg.binding

    def make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert):
        state, pending = b.hosttwin_runrs_state(nch, len(taps), I)

        def call(i, gr, gp):
            return b.hosttwin_runrs_call(W, taps, I, D, state, pending, gr, gp, invert=invert)

        return call, lambda: None

    return make_call


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_hosttwin_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """csrc/mfm_runrs.h through its host twin on the scenes of the GPU tests, 1 and 3 channels"""
    run_scenes(pkg, ora, W, ratio, (1, 3), _twin_call(pkg), 7 * W + ratio[0])


def _small_case(pkg):
    """W = 5, 4/5 with 9 taps (plen 4): channel 1 has windows 1 - 2 and 4 - 5 open, channel 2 window 3"""
    W, nch = 5, 3
    rng = np.random.RandomState(3)
    stream = rng.randint(-32768, 32768, size=(nch, 30)).astype(np.int16)
    mask = np.zeros((nch, 6), bool)
    mask[1, [1, 2, 4, 5]] = True
    mask[2, 3] = True
    taps = rng.randint(-8191, 8192, 9).astype(np.int16)
    return W, nch, stream, mask, taps


def test_hosttwin_refuses_and_leaves_its_state(pkg, ora):
    b = pkg.binding
    W, nch, stream, mask, taps = _small_case(pkg)
    I, D = 4, 5
    calls = gate_calls(pkg, stream, mask, W, 0, [12, 18])
    chk = Checker(pkg, ora, taps, I, D, False, W)
    state, pending = b.hosttwin_runrs_state(nch, len(taps), I)
    assert pending.shape == (nch, 4) and (state["expected"] == b.MFM_RUNRS_NO_WINDOW).all()
    same(b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[0]), chk.call(*calls[0]), "first call")
    assert int(state["expected"][1]) == 2 and int(state["pending"][1]) <= 4
    s0, p0 = state.copy(), pending.copy()
    want = chk.call(*calls[1])
    assert len(want[0]) == 3 and want[1].size > 0
    for kw in (dict(max_runs=2), dict(max_elems=want[1].size - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[1], **kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, want[1].size)
    gr = calls[1][0].copy()
    for field, value in (("channel", nch), ("payload_offset", calls[1][1].size), ("nr_windows", 7)):
        bad = gr.copy()
        bad[field][1] = value
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_call(W, taps, I, D, state, pending, bad, calls[1][1])
        assert ei.value.code == b.MFM_E_INVAL and "not a gate's" in str(ei.value)
    assert np.array_equal(state, s0) and np.array_equal(pending, p0)   # a refused call changes nothing
    same(b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[1]), want, "second call")
    assert [int(f) for f in want[0]["flags"]] == [0, 1, 1]   # channel 1 goes on, then begins again behind window 3; channel 2 begins


REFUSALS = [
    (dict(abi_version=3), "abi_version"),
    (dict(nr_channels=0), "nr_channels"),
    (dict(nr_channels=65536), "65535"),
    (dict(flags=1), "no DC blocker and no sign-bit output"),
    (dict(interpolate=0), "interpolate and decimate"),
    (dict(decimate=0), "interpolate and decimate"),
    (dict(window_samples=0), "PCM payloads only"),
    (dict(window_samples=(1 << 20) + 1), "PCM payloads only"),
    (dict(coeffs_q14=np.zeros(0, np.int16)), "no taps"),
    (dict(interpolate=1, decimate=9, coeffs_q14=np.ones(4, np.int16)), "more than the 4 taps of a phase"),
    (dict(interpolate=8000, decimate=1, coeffs_q14=np.ones(8000, np.int16)), "MFM_RUNRS_MAX_LDS_BYTES = 49152"),
    (dict(interpolate=1, decimate=60, coeffs_q14=np.ones(64, np.int16)), "MFM_RUNRS_MAX_LDS_BYTES = 49152"),
    (dict(max_in_samples=0), "max_in_samples"),
    (dict(max_in_samples=0, max_windows=8), "max_in_samples"),
    (dict(nr_channels=65535, window_samples=1 << 20, max_in_samples=1 << 24), "2^31"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_with_a_message(pkg, change, message):
    """every refusal of mfm_runrs_create is decided before a device is looked for"""
    b = pkg.binding
    kw = dict(nr_channels=3, coeffs_q14=np.ones(81, np.int16), interpolate=4, decimate=5, window_samples=64, max_in_samples=1000)
    kw.update(change)
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunResampler(**kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_runrs_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_runrs.o (tools/kernel_regs.py): plan, scan, state and the FIR kernel's ten
    instances, no private segment, no spilled register"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runrs.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_runrs.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    fir = [f"rr_fir_kernel<{np_}>" for np_ in range(0, 33, 4)]
    assert sorted(ln.split()[0] for ln in lines) == sorted(fir + ["rr_plan_kernel", "rr_scan_kernel", "rr_state_kernel"]), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gpu_call(pkg):
    """a real Gate (process_host, flush_device) in front of the stage; the gate's own result is checked on the way"""
    def make_call(nch, W, P, cuts, stream, mask, taps, I, D, invert):
        cap = max(max(cuts), 1)
        gate = pkg.Gate(nch, cap, W, preroll_windows=P)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P, invert=invert)
        pos = [0]

        def call(i, gr, gp):
            if i < len(cuts):
                m = cuts[i]
                rec = tg.records_of(pkg, mask, pos[0] // W, (pos[0] + m) // W)
                got = gate.process_host(stream[:, pos[0]:pos[0] + m], rec)
                pos[0] += m
            else:
                gate.flush_device()
                got = gate.fetch()
            tg.same(got, (gr, gp), f"the gate's call {i}")
            rr.process_device(*gate.device_view())
            return rr.fetch()

        def done():
            rr.close()
            gate.close()

        return call, done

    return make_call


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_equals_the_oracle_per_stretch(pkg, ora, W, ratio):
    """1, 3 and 65 channels; all closed, all open, stretches of 1 - 3 windows, a stretch that ends with a call while the
    neighbour's begins with the next, three runs of a channel in one call; P = 0 and 2 with the flush fed through; random and
    full-scale values, invert; 40 - 60 windows cut into calls (nr_in = 0, three calls in a row shorter than W) and as one call,
    with identical outputs per stretch"""
    run_scenes(pkg, ora, W, ratio, (1, 3, 65), _gpu_call(pkg), 11 * W + ratio[0])


def _up(torch, a):
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)
    return torch.from_numpy(raw).cuda()


def _fed(pkg, torch, rr, gr, gp, totals=None):
    """one call from uploaded arrays: a gate's result as it would stand in its device view"""
    t = np.array([len(gr), gp.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (_up(torch, gr), _up(torch, gp), _up(torch, t))
    rr.process_device(*(k.data_ptr() for k in keep))
    out = rr.fetch()
    del keep
    return out


@pytest.mark.gpu
def test_gpu_overflow_and_gate_errors_leave_the_state(pkg, ora):
    """one call of six windows does not fit max_windows = 4 (or max_runs = 2), the gate's overflow and out-of-step flags are
    handed through: each time nothing comes out and the state stays, so the same windows in calls that fit are right"""
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = _small_case(pkg)
    I, D = 4, 5
    first, second = gate_calls(pkg, stream, mask, W, 0, [12, 18])
    whole = gate_calls(pkg, stream, mask, W, 0, [30])[0]
    assert len(whole[0]) == 3 and whole[1].size == 5 * W and len(second[0]) == 3
    for kw, what in ((dict(max_windows=4, max_runs=8), "max_windows"), (dict(max_windows=8, max_runs=2), "max_runs")):
        rr = pkg.RunResampler(nch, taps, I, D, W, **kw)
        chk = Checker(pkg, ora, taps, I, D, False, W)
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rr, *whole)
        assert ei.value.code == b.MFM_E_STATE and "max_windows or max_runs" in str(ei.value), what
        assert ei.value.needed == (0, 0) and not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
        if what == "max_windows":   # two calls that fit
            same(_fed(pkg, torch, rr, *first), chk.call(*first), "first call after the overflow")
            second2 = second
        else:                      # the second call has three runs: as two calls of two and one
            same(_fed(pkg, torch, rr, *first), chk.call(*first), "first call after the overflow")
            gr, gp = second
            cutoff = int(gr["payload_offset"][2])
            a = (gr[:2], gp[:cutoff])
            c = gr[2:].copy()
            c["payload_offset"] -= cutoff
            same(_fed(pkg, torch, rr, *a), chk.call(*a), "second call, two runs")
            second2 = (c, gp[cutoff:])
        same(_fed(pkg, torch, rr, *second2), chk.call(*second2), "last call")
        rr.close()
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=30)
    chk = Checker(pkg, ora, taps, I, D, False, W)
    same(_fed(pkg, torch, rr, *first), chk.call(*first), "first call")
    for totals, message in (([3, second[1].size, 1, 0], "max_open_windows"), ([3, second[1].size, 0, 1], "out of step"),
                            ([3, second[1].size, 1, 1], "out of step")):
        with pytest.raises(pkg.MfmError) as ei:
            _fed(pkg, torch, rr, *second, totals=totals)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value)
        assert ei.value.needed == (0, 0)
    bad = second[0].copy()
    bad["channel"][1] = nch
    with pytest.raises(pkg.MfmError) as ei:
        _fed(pkg, torch, rr, bad, second[1])
    assert ei.value.code == b.MFM_E_STATE and "not a gate's" in str(ei.value)
    want = chk.call(*second)
    same(_fed(pkg, torch, rr, *second), want, "second call after four refused ones")
    for kw in (dict(max_runs=2), dict(max_elems=want[1].size - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            rr.fetch(**kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, want[1].size)
    same(rr.fetch(), want, "fetched again")
    rr.close()


@pytest.mark.gpu
def test_gpu_many_runs_and_many_workgroups(pkg, ora):
    """2100 runs in one call (the scan's threads take three runs each, the last ones fewer) and a run of 5000 outputs (five
    workgroups, the last one partly filled) behind runs without output"""
    import torch
    W, I, D = 8, 4, 5
    rng = np.random.RandomState(8)
    taps = rng.randint(-8191, 8192, 81).astype(np.int16)
    nch, nw = 70, 60
    stream = rng.randint(-32768, 32768, size=(nch, nw * W)).astype(np.int16)
    mask = (np.arange(nw)[None, :] + np.arange(nch)[:, None]) % 2 == 0
    calls = gate_calls(pkg, stream, mask, W, 0, [nw * W])
    assert len(calls[0][0]) == 2100
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=nw * W)
    drive(pkg, ora, calls, taps, I, D, False, W, lambda i, gr, gp: _fed(pkg, torch, rr, gr, gp), "2100 runs")
    rr.close()
    W, nch, nw = 64, 3, 100
    stream = rng.randint(-32768, 32768, size=(nch, nw * W)).astype(np.int16)
    mask = np.zeros((nch, nw), bool)
    mask[0, [1, 3]] = True          # 64 samples: 36 outputs each
    mask[1, 1:99] = True            # 6272 samples: 5001 outputs
    mask[2, 50] = True
    calls = gate_calls(pkg, stream, mask, W, 0, [nw * W])
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=nw * W)
    got = drive(pkg, ora, calls, taps, I, D, False, W, lambda i, gr, gp: _fed(pkg, torch, rr, gr, gp), "long run")
    assert got[(1, 1)].size > 4 * 1024
    rr.close()


CHAIN = dict(nr_channels=3, channel=1, W=500, nr_out=9000, on=(7, 12), amplitude=900.0, noise=512, seed=6)
_CHAIN = {}


def _chain(pkg, ora):
    """3 channels of the 64-channel plan, noise everywhere, and on channel 1 a carrier during windows 7 .. 11"""
    if _CHAIN:
        return _CHAIN["it"]
    sy, s = pkg.synth, CHAIN
    fs, decim, taps, offs, gains = sy.plan("cfg2_64ch", nr_channels=s["nr_channels"])
    W = s["W"]
    n = decim * (s["nr_out"] - 1) + len(taps)
    iq = sy.synth_iq(n, fs, [], seed=s["seed"], noise=s["noise"]).astype(np.int32)
    burst = sy.synth_iq(n, fs, offs[[s["channel"]]], seed=s["seed"], amplitude=s["amplitude"], noise=0).astype(np.int32)
    burst[:decim * s["on"][0] * W] = 0
    burst[decim * s["on"][1] * W:] = 0
    iq = np.clip(iq + burst, -32768, 32767).astype(np.int16)
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm, fiq = ora.run_channels(iq, cre, cim, incr, decim, want_iq=True)
    e = tl.restate(pkg, fiq, W, tl.IQ)["energy"].astype(np.float64)
    on = np.zeros(e.shape, bool)
    on[s["channel"], s["on"][0] + 1:s["on"][1] - 1] = True
    idle = np.ones(e.shape, bool)
    idle[s["channel"], s["on"][0] - 1:s["on"][1] + 1] = False
    thr = int(np.sqrt(e[on].min() * e[idle].max()))
    rec = tl.restate(pkg, fiq, W, tl.IQ, sense=tl.ABOVE, open_thr=thr, close_thr=thr, hang=1)
    mask = rec["open"].astype(bool)
    # the scene is what it is meant to be: a wide margin, one channel that opens and closes again
    assert e[on].min() / e[idle].max() >= 2.0
    assert not np.delete(mask, s["channel"], axis=0).any()
    assert mask[s["channel"], s["on"][0] + 1:s["on"][1] - 1].all() and not mask[s["channel"], :s["on"][0] - 1].any()
    assert not mask[s["channel"], s["on"][1] + 2:].any()
    _CHAIN["it"] = dict(plan=(fs, decim, taps, offs, gains), iq=iq, pcm=pcm, W=W, thr=thr, mask=mask)
    return _CHAIN["it"]


@pytest.mark.gpu
def test_gpu_engine_level_gate_runrs_on_device_equals_the_chain_through_the_oracle(pkg, ora):
    """engine -> level (IQ form) -> gate with P = 1 on the PCM rows -> burst resampler 4/5, all queued on the engine's stream
    with no host copy between the stages; every call and the flush against the oracle's PCM through the restated gate and the
    oracle's resampler"""
    b = pkg.binding
    sc = _chain(pkg, ora)
    (fs, decim, taps, offs, gains), iq, pcm, W, mask, P = sc["plan"], sc["iq"], sc["pcm"], sc["W"], sc["mask"], 1
    nch = pcm.shape[0]
    I, D = 4, 5
    rs_taps = np.random.RandomState(4).randint(-4000, 4001, 81).astype(np.int16)
    blk = 50021
    eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g), want_iq=True)
    eng.commit()
    cap = blk // decim + 8
    lv = pkg.Level(nch, cap, W, form=b.MFM_LEVEL_IQ, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=1)
    gate = pkg.Gate(nch, cap, W, elems_per_sample=1, preroll_windows=P)
    rr = pkg.RunResampler(nch, rs_taps, I, D, W, max_in_samples=cap, preroll_windows=P)
    chk = Checker(pkg, ora, rs_taps, I, D, False, W)
    pos, outs = 0, 0
    for s in range(0, iq.shape[0], blk):
        assert eng.push(iq[s:s + blk]) == 0
        d_pcm, stride, nout, d_iq = eng.last_output_device()
        lv.process_device(d_iq, 2 * stride, nout, stream=eng.stream)
        d_rec, rec_stride, nw, _ = lv.device_view()
        gate.process_device(d_pcm, stride, nout, d_rec, rec_stride, nw, stream=eng.stream)
        rr.process_device(*gate.device_view(), stream=eng.stream)
        got = rr.fetch()
        want = chk.call(*tgp.restate_pre(pkg, pcm, mask, W, 1, P, pos, nout))
        same(got, want, f"block at {pos}")
        outs += got[1].size
        pos += nout
    assert pos == pcm.shape[1]
    gate.flush_device(stream=eng.stream)
    rr.process_device(*gate.device_view(), stream=eng.stream)
    got = rr.fetch()
    same(got, chk.call(*tgp.restate_pre(pkg, pcm, mask, W, 1, P, pos, 0, flush=True)), "flush")
    outs += got[1].size
    by = chk.stretches()
    assert by and outs > 0 and outs == sum(v.size for v in by.values())
    for o in (rr, gate, lv, eng):
        o.close()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_resample_writes_the_stretches_of_the_oracle(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-out DIR --gate-preroll 1 --gate-resample 4/5 --resample-taps FILE on the chain scene, squelch on
    the PCM energy (a carrier lowers it): each chNNNN.rs.s16 is the channel's stretches through the oracle's resampler, and
    resampled.jsonl has one line per run"""
    import json
    sc = _chain(pkg, ora)
    (fs, decim, taps, offs, gains), W, pcm, P = sc["plan"], sc["W"], sc["pcm"], 1
    I, D = 4, 5
    e = tl.restate(pkg, pcm, W, tl.PCM)["energy"].astype(np.float64)
    s = CHAIN
    on = np.zeros(e.shape, bool)
    on[s["channel"], s["on"][0] + 1:s["on"][1] - 1] = True
    idle = np.ones(e.shape, bool)
    idle[s["channel"], s["on"][0] - 1:s["on"][1] + 1] = False
    assert e[idle].min() / e[on].max() >= 2.0
    thr = int(np.sqrt(e[on].max() * e[idle].min()))
    mask = tl.restate(pkg, pcm, W, tl.PCM, sense=tl.BELOW, open_thr=thr, close_thr=thr, hang=1)["open"].astype(bool)
    assert mask[s["channel"]].any() and not mask.all()
    lpf = [float(x) for x in np.hanning(81) * 0.2]
    rs_taps = np.array([int(x * 16384.0) for x in lpf], np.int16)
    centre = 929500000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": lpf}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in taps],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in offs]}))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
           str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(thr),
           "--hang", "1", "--block", "50021", "--gate-out", str(tmp_path / "gated"), "--gate-preroll", str(P),
           "--gate-resample", f"{I}/{D}", "--resample-taps", str(tmp_path / "filter.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    emitted = tgp.dilate(mask, P)
    lines = [json.loads(ln) for ln in (tmp_path / "gated" / "resampled.jsonl").read_text().splitlines()]
    gated = [json.loads(ln) for ln in (tmp_path / "gated" / "index.jsonl").read_text().splitlines()]
    assert len(lines) == len(gated) and [ln["channel"] for ln in lines] == [ln["channel"] for ln in gated]
    assert [ln["first_sample"] for ln in lines] == [ln["first_sample"] for ln in gated]
    assert sorted((ln["channel"], ln["first_sample"] // W) for ln in lines if ln["begins"]) == stretches_of_mask(emitted)
    for c in range(mask.shape[0]):
        path = tmp_path / "gated" / f"ch{c:04d}.rs.s16"
        assert path.exists() == bool(emitted[c].any())
        if not emitted[c].any():
            continue
        want = []
        for _, k0 in [k for k in stretches_of_mask(emitted) if k[0] == c]:
            k1 = k0
            while k1 < emitted.shape[1] and emitted[c, k1]:
                k1 += 1
            want.append(ofeed(ora, ora.Resampler(rs_taps, I, D), pcm[c, k0 * W:k1 * W]))
        assert np.array_equal(np.fromfile(path, np.int16), np.concatenate(want)), c
        mine = [ln for ln in lines if ln["channel"] == c]
        assert sum(ln["nr_out"] for ln in mine) == sum(w.size for w in want)
        at = 0
        for ln in mine:
            assert ln["file_offset"] == at
            at += 2 * ln["nr_out"]
