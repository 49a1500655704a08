"""The run router (mfm_runroute_*, csrc/mfm_runroute.hip): one gate feeds a burst chain per protocol.  Route k's run list is the
gate's runs whose channel has route k, byte for byte and in the gate's order; the payload stays the gate's.

The checker is never the code under test: the partition is restated in numpy (`restate`), and a routed chain is compared with the
chain as it stands without the router on the same gate's view, filtered to the route's channels, and with the oracle Checkers
of tests/test_runpocsag.py, test_runais.py and test_runflex.py on the filtered run list.  Every comparison is an equality."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_runais as tra
import test_runflex as trf
import test_runpocsag as trp
import test_runrs as tr
import test_runrs_dc as trd

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runroute_create", "mfm_runroute_destroy", "mfm_runroute_process_device", "mfm_runroute_device_view", "mfm_runroute_fetch",
             "mfm_runroute_get_capacity", "mfm_hosttwin_runroute_capacity", "mfm_hosttwin_runroute_call"]
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000]   # runs: across a wave, a workgroup's strip and several strips
ROUTES = [1, 3, 8]
TABLES = ["one", "none", "alternating", "random"]
NCH = 97
NONE = 255


# ---- the checker --------------------------------------------------------------------------------------------

def make_table(kind, K, nch=NCH):
    if kind == "one":
        return np.full(nch, K - 1, np.uint8)
    if kind == "none":
        return np.full(nch, NONE, np.uint8)
    if kind == "alternating":
        return (np.arange(nch) % K).astype(np.uint8)
    rng = np.random.RandomState(100 + K)
    t = rng.randint(0, K + 1, nch)
    return np.where(t == K, NONE, t).astype(np.uint8)


_RUNS = {}


def make_runs(pkg, n, nch=NCH):
    """a hand-made gate run list of n runs: channels ascending, a channel's windows ascending, payload offsets that leave holes
    (the router must not care).  Made once per n and left unchanged"""
    if n not in _RUNS:
        rng = np.random.RandomState(7 + n)
        runs = np.zeros(n, pkg.binding.GATE_RUN_DTYPE)
        runs["channel"] = np.sort(rng.randint(0, nch, n))
        runs["nr_windows"] = rng.randint(1, 4, n)
        runs["first_window"] = np.cumsum(runs["nr_windows"] + rng.randint(1, 3, n)) + (1 << 33)
        runs["payload_offset"] = np.cumsum(rng.randint(0, 9, n) * 64)
        _RUNS[n] = runs
    return _RUNS[n]


def totals_of(runs, over=0, oos=0):
    return np.array([len(runs), int(runs["payload_offset"][-1]) + 4 * 64 if len(runs) else 0, over, oos], np.uint64)


def restate(table, K, runs, totals, cap):
    """([runs of route k], [totals of route k]) by the rule of include/multifm_hip.h"""
    over, oos = int(totals[2] != 0), int(totals[3] != 0)
    if not over and not oos and int(totals[0]) > cap:
        over = 1
    if not over and not oos and (runs["channel"] >= len(table)).any():
        oos = 1
    if over or oos:
        return [runs[:0]] * K, [[0, 0, over, oos]] * K
    route = np.asarray(table)[runs["channel"]]
    return [runs[route == k] for k in range(K)], [[int((route == k).sum()), int(totals[1]), 0, 0] for k in range(K)]


def twin(pkg, table, K, runs, totals, cap):
    """the host twin's answer in the shape of restate(), and the raw run rows"""
    rows, t = pkg.hosttwin_runroute_call(table, K, runs, totals, max_runs=cap)
    return [rows[k][:int(t[k][0])] for k in range(K)], [[int(x) for x in t[k]] for k in range(K)], rows


def same_lists(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: route {k} differs ({len(g)} runs, {len(w)} wanted)"


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_runroute_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    m = re.search(r"struct mfm_runroute_config \{(.*?)\};", src, flags=re.S)
    fields = [x for _, names in re.findall(r"(u?int\d+_t)\s+([\w, ]+);", m.group(1)) for x in names.split(", ")]
    assert fields == [f[0] for f in b.RunRouteConfig._fields_] and C.sizeof(b.RunRouteConfig) == 40
    assert re.search(r"#define MFM_RUNROUTE_MAX_ROUTES 8u", src) and re.search(r"#define MFM_ROUTE_NONE 255u", src)
    assert (b.MFM_RUNROUTE_MAX_ROUTES, b.MFM_ROUTE_NONE) == (8, 255) and re.search(r"#define MFM_ABI_VERSION %d\b" % b.MFM_ABI_VERSION, src)
    assert pkg.RunRouter is b.RunRouter and pkg.hosttwin_runroute_call is b.hosttwin_runroute_call
    assert callable(pkg.RunRouter.behind) and callable(pkg.RunRouter.device_view) and callable(pkg.RunRouter.fetch)


@pytest.mark.parametrize("K", ROUTES)
@pytest.mark.parametrize("n", COUNTS)
def test_hosttwin_equals_the_restatement(pkg, n, K):
    runs = make_runs(pkg, n)
    totals = totals_of(runs)
    some = 0
    for kind in TABLES:
        table = make_table(kind, K)
        got_runs, got_totals, _ = twin(pkg, table, K, runs, totals, max(n, 1))
        want_runs, want_totals = restate(table, K, runs, totals, max(n, 1))
        assert got_totals == want_totals, (kind, got_totals, want_totals)
        same_lists(got_runs, want_runs, f"n {n} K {K} table {kind}")
        assert sum(len(r) for r in got_runs) == (0 if kind == "none" else n if kind != "random" else sum(len(r) for r in want_runs))
        some += kind == "random" and 0 < sum(len(r) for r in got_runs) < n
    assert some or n < 63   # the random table drops some runs and keeps some


def test_hosttwin_partition_is_stable_and_channels_ascend(pkg):
    runs = make_runs(pkg, 5000)
    table = make_table("random", 8)
    got, totals, _ = twin(pkg, table, 8, runs, totals_of(runs), 5000)
    assert all(len(g) for g in got)
    for k, g in enumerate(got):
        assert (np.diff(g["channel"].astype(np.int64)) >= 0).all() and (table[g["channel"]] == k).all()
        assert (np.diff(g["first_window"].astype(np.int64)) > 0).all()   # the list's own order, kept


REFUSED = [("the gate's overflow", dict(over=1), [0, 0, 1, 0]), ("the gate's out of step", dict(oos=1), [0, 0, 0, 1]),
           ("both of the gate's flags", dict(over=7, oos=9), [0, 0, 1, 1]), ("runs beyond capacity", dict(cap=256), [0, 0, 1, 0]),
           ("a channel beyond the table", dict(bad=200), [0, 0, 0, 1]), ("a channel beyond the table in the last run", dict(bad=256), [0, 0, 0, 1])]


def refused_case(pkg, change):
    runs = make_runs(pkg, 257).copy()
    if "bad" in change:
        runs["channel"][change["bad"]] = NCH
    return runs, totals_of(runs, change.get("over", 0), change.get("oos", 0)), change.get("cap", 257)


@pytest.mark.parametrize("what,change,want", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_hosttwin_refusals_flag_every_route_and_write_nothing_else(pkg, what, change, want):
    b = pkg.binding
    runs, totals, cap = refused_case(pkg, change)
    for K in ROUTES:
        table = make_table("alternating", K)
        rows = np.zeros((K, cap), b.GATE_RUN_DTYPE)
        rows["channel"] = 0xdeadbeef
        keep = rows.copy()
        _, t = pkg.hosttwin_runroute_call(table, K, runs, totals, max_runs=cap, runs=rows)
        assert [[int(x) for x in q] for q in t] == [want] * K == restate(table, K, runs, totals, cap)[1], what
        assert rows.tobytes() == keep.tobytes(), what


CREATE_REFUSALS = [(dict(nr_routes=0), "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES"), (dict(nr_routes=9), "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES"),
                   (dict(entry=3), "route_of_channel[5] = 3 is neither below nr_routes = 3 nor MFM_ROUTE_NONE"),
                   (dict(entry=254), "route_of_channel[5] = 254"), (dict(flags=1), "flags must be 0"),
                   (dict(abi_version=1), "abi_version"), (dict(max_in_samples=0), "max_in_samples is 0"),
                   (dict(window_samples=0), "window_samples must be 1 .. 2^20")]


@pytest.mark.parametrize("change,message", CREATE_REFUSALS, ids=[str(sorted(c.items())[0]) for c, _ in CREATE_REFUSALS])
def test_create_refuses_with_a_message(pkg, change, message):
    """mfm_runroute_create itself: what it refuses it refuses before it looks for a device"""
    b = pkg.binding
    change = dict(change)
    table = make_table("alternating", 3, 16)
    if "entry" in change:
        table[5] = change.pop("entry")
    kw = dict(nr_routes=3, window_samples=64, max_in_samples=4096)
    kw.update(change)
    K = kw.pop("nr_routes")
    for make in (pkg.RunRouter, pkg.hosttwin_runroute_capacity):
        with pytest.raises(pkg.MfmError) as ei:
            make(table, K, **kw)
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


CAPACITY_CASES = [dict(window_samples=64, max_in_samples=4096), dict(window_samples=64, max_in_samples=4095, preroll_windows=2),
                  dict(window_samples=500, max_in_samples=100, preroll_windows=7), dict(window_samples=1, max_in_samples=1000),
                  dict(window_samples=64, max_in_samples=4096, max_windows=40), dict(window_samples=100, max_in_samples=1 << 20, preroll_windows=63)]


def test_default_capacity_is_the_documented_rule(pkg):
    """max_runs == 0: min(max_windows, nr_channels * ceil(per / 2)) with per = max(max_in_samples / W + 1, P) windows a channel, and
    max_windows == 0 taken as nr_channels * per (include/multifm_hip.h, mfm_runrs_config); a given max_runs is kept"""
    for nch in (1, 3, 1024):
        table = np.zeros(nch, np.uint8)
        for kw in CAPACITY_CASES:
            per = max(kw["max_in_samples"] // kw["window_samples"] + 1, kw.get("preroll_windows", 0))
            want = min(kw.get("max_windows", 0) or nch * per, nch * ((per + 1) // 2))
            assert pkg.hosttwin_runroute_capacity(table, 1, **kw) == want, (nch, kw)
            assert pkg.hosttwin_runroute_capacity(table, 1, max_runs=17, **kw) == 17
    assert pkg.hosttwin_runroute_capacity(np.zeros(4, np.uint8), 1, max_runs=17) == 17   # nothing else is read then


def test_runroute_kernel_uses_no_scratch_and_does_not_spill():
    """the code object's notes of build/mfm_runroute.o (tools/kernel_regs.py): the one kernel, no private segment, no spilled
    register, the LDS of the wave counts alone"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runroute.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert [ln.split()[0] for ln in lines] == ["rt_route_kernel"], out
    m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", lines[0])
    assert m and int(m.group(1)) <= 64 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), lines[0]
    assert int(m.group(4)) == (2 * 8 * 16 + 16) * 4, lines[0]


# ---- GPU: the router alone ------------------------------------------------------------------------------------------

def routed(torch, router, gr, gp, totals=None):
    """one router call from uploaded arrays: a gate's result as it would stand in its device view.  Returns the uploads, which the
    caller keeps while anything reads a route's view: the payload there is this one"""
    t = np.array([len(gr), gp.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, gr), tr._up(torch, gp), tr._up(torch, t))
    router.process_device(*(k.data_ptr() for k in keep))
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("K", ROUTES)
def test_gpu_equals_the_twin(pkg, K):
    """every run count and table of the twin's test through one router per table, the counts in an order that makes most calls
    smaller than the one before: what the totals cover is this call's alone"""
    import torch
    b = pkg.binding
    order = [5000, 1025, 1024, 1023, 257, 256, 255, 65, 64, 63, 1, 0, 5000, 64]
    assert set(order) == set(COUNTS)
    for kind in TABLES:
        table = make_table(kind, K)
        router = pkg.RunRouter(table, K, max_runs=5000)
        assert router.capacity() == 5000 and router.device_view(0)[1] is None
        views = [router.device_view(k) for k in range(K)]
        for n in order:
            runs = make_runs(pkg, n)
            totals = totals_of(runs)
            keep = routed(torch, router, runs, np.zeros(8, np.int16), totals)
            want_runs, want_totals, _ = twin(pkg, table, K, runs, totals, 5000)
            for k in range(K):
                got, nr_elems = router.fetch(k)
                assert got.tobytes() == want_runs[k].tobytes(), (kind, n, k)
                assert nr_elems == want_totals[k][1] == int(totals[1])
                d_runs, d_payload, d_totals = router.device_view(k)
                assert (d_runs, d_totals) == views[k][::2] and d_payload == keep[1].data_ptr()   # fixed at create; the gate's pointer
            del keep
        if kind == "alternating":   # fetch's conventions
            with pytest.raises(pkg.MfmError) as ei:
                router.fetch(0, max_runs=0)
            assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(want_runs[0]) > 0
            with pytest.raises(pkg.MfmError) as ei:
                router.device_view(K)
            assert ei.value.code == b.MFM_E_INVAL
        router.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what,change,want", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_gpu_refusals_equal_the_twin(pkg, what, change, want):
    import torch
    b = pkg.binding
    runs, totals, cap = refused_case(pkg, change)
    good = make_runs(pkg, 255)
    for K in ROUTES:
        table = make_table("alternating", K)
        router = pkg.RunRouter(table, K, max_runs=cap)
        keep = routed(torch, router, runs, np.zeros(8, np.int16), totals)
        for k in range(K):
            with pytest.raises(pkg.MfmError) as ei:
                router.fetch(k)
            assert ei.value.code == b.MFM_E_STATE and ei.value.needed == 0, what
            assert ("out of step" if want[3] else "overflowed") in str(ei.value), (what, str(ei.value))
        keep = routed(torch, router, good, np.zeros(8, np.int16), totals_of(good))   # the router carries no state: the next call is right
        want_runs, _, _ = twin(pkg, table, K, good, totals_of(good), cap)
        for k in range(K):
            assert router.fetch(k)[0].tobytes() == want_runs[k].tobytes()
        del keep
        router.close()


GATE_NUMBERS = [dict(nr_channels=3, window_samples=64, max_in_samples=4096), dict(nr_channels=65, window_samples=7, max_in_samples=700, preroll_windows=2),
                dict(nr_channels=2, window_samples=500, max_in_samples=100, preroll_windows=7),
                dict(nr_channels=9, window_samples=64, max_in_samples=4096, max_windows=40)]


@pytest.mark.gpu
def test_gpu_default_capacity_is_the_burst_resamplers(pkg):
    taps = np.ones(8, np.int16)
    for kw in GATE_NUMBERS:
        kw = dict(kw)
        nch = kw.pop("nr_channels")
        rr = pkg.RunResampler(nch, taps, 4, 5, kw["window_samples"], max_in_samples=kw["max_in_samples"],
                              preroll_windows=kw.get("preroll_windows", 0), max_windows=kw.get("max_windows", 0))
        router = pkg.RunRouter.behind(np.zeros(nch, np.uint8), 1, kw["max_in_samples"], kw["window_samples"],
                                      preroll_windows=kw.get("preroll_windows", 0), max_open_windows=kw.get("max_windows", 0))
        assert router.capacity() == rr.capacity()[0] == pkg.hosttwin_runroute_capacity(np.zeros(nch, np.uint8), 1, **kw), kw
        router.close()
        rr.close()


# ---- GPU: routed chains -----------------------------------------------------------------------------------------------

MIXED = dict(W=64, P=1, hang=2, n=30000, ratio=(4, 5, 41), pole=0.999, seed=21)
_MIXED = {}


def _mixed(pkg, ora):
    """nine PCM rows at one rate: 0 .. 3 the short POCSAG scene of tests/test_runpocsag.py (in front of its 4/5 resampler), 4 .. 7
    the AIS scene of tests/test_runais.py (in front of its 4/5 resampler), 8 a channel of no protocol whose squelch still opens
    (a block of loud noise): its runs go nowhere.  The squelch opens above an rms of 1000.  Made once and left unchanged"""
    if _MIXED:
        return _MIXED["it"]
    s = MIXED
    n, W = s["n"], s["W"]
    pg = trp.scene(pkg, ora, s["ratio"], 7)["stream"][:, :n]
    ai = tra.scene(pkg, s["ratio"])["stream"][:, :n]
    assert pg.shape == ai.shape == (4, n)
    rng = np.random.RandomState(s["seed"])
    idle = (rng.randn(n) * 40).round().astype(np.int16)
    idle[7000:12000] = rng.normal(0, 6000, 5000).round().astype(np.int16)
    rows = np.ascontiguousarray(np.concatenate([pg, ai, idle[None]]))
    table = np.array([0] * 4 + [1] * 4 + [NONE], np.uint8)
    cuts = [0]
    while sum(cuts) < n:
        cuts.append(min(int(rng.randint(1, 7001)), n - sum(cuts)))
    cuts.insert(len(cuts) // 2, 0)
    _MIXED["it"] = dict(rows=rows, table=table, cuts=cuts, thr=W * 1000 * 1000, taps=trp.rs_taps(pkg, ora, s["ratio"]))
    return _MIXED["it"]


def filtered(runs, table, k):
    return runs[np.asarray(table)[runs["channel"]] == k]


def same_but(got, want, skip, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in got.dtype.names:
        if f not in skip:
            assert np.array_equal(got[f], want[f]), (what, f)


def slices(runs, payload, bits):
    out = []
    for r in runs:
        n = (int(r["nr_out"]) + 31) // 32 if bits else int(r["nr_out"])
        out.append(payload[int(r["out_offset"]):int(r["out_offset"]) + n])
    return out


class Chain:
    """burst resampler -> burst stage on the device, behind whatever view it is given"""

    def __init__(self, pkg, nch, taps, ratio, W, cap, P, stage, bits=False, pole=None):
        b = pkg.binding
        self.rr = pkg.RunResampler(nch, taps, ratio[0], ratio[1], W, max_in_samples=cap, preroll_windows=P)
        if pole is not None:
            self.rr.set_dc_block(pole)
        self.st = {"pocsag": pkg.RunPocsag, "ais": pkg.RunAis, "flex": pkg.RunFlex}[stage].behind(self.rr)
        self.polarity = (b.MFM_BITS_POS if stage == "ais" else b.MFM_BITS_NEG) if bits else 0

    def call(self, view):
        """(runs, payload or bit words), events (with the FLEX stage: (events, frames))"""
        if self.polarity:
            self.rr.process_bits_device(*view, self.polarity)
            self.st.process_bits_device(self.rr.bits_view())
            return self.rr.fetch_bits(), self.st.fetch()
        self.rr.process_device(*view)
        self.st.process_device(*self.rr.device_view())
        return self.rr.fetch(), self.st.fetch()

    def close(self):
        self.st.close()
        self.rr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["pcm", "bits_on_the_pocsag_route", "dc_on_the_ais_route"])
def test_gpu_routed_chains_equal_the_unrouted_chains_on_their_channels(pkg, ora, variant):
    """one level and one gate (P = 1) over the nine rows in ragged calls and the flush; route 0 a POCSAG chain at 4/5, route 1 an
    AIS chain at 4/5, the ninth channel routed nowhere.  Per route and call: against the same chain fed the gate's own view,
    filtered to the route's channels, and against the oracle's Checker on the filtered run list"""
    b = pkg.binding
    sc, s = _mixed(pkg, ora), MIXED
    W, P, (I, D, _) = s["W"], s["P"], s["ratio"]
    rows, table, cuts, taps = sc["rows"], sc["table"], sc["cuts"], sc["taps"]
    nch, cap = rows.shape[0], max(cuts)
    bits = [variant.startswith("bits"), False]
    pole = [None, s["pole"] if variant.startswith("dc") else None]
    stages = ["pocsag", "ais"]
    lv = pkg.Level(nch, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=s["hang"])
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    router = pkg.RunRouter.behind(table, 2, cap, W, preroll_windows=P)
    routed_chains = [Chain(pkg, nch, taps, (I, D), W, cap, P, stages[k], bits[k], pole[k]) for k in range(2)]
    plain_chains = [Chain(pkg, nch, taps, (I, D), W, cap, P, stages[k], bits[k], pole[k]) for k in range(2)]
    chk = [trp.Checker(pkg, ora, taps, I, D, W), tra.Checker(pkg, ora, taps, I, D, W)]
    if pole[1] is not None:
        chk[1].rs = trd.DcChecker(pkg, ora, taps, I, D, False, W, pole[1])
    same_ev = [trp.same, tra.same]
    pos, seen, dropped = 0, [0, 0], 0
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gr, gp = gate.process_host(rows[:, pos:pos + m], lv.process_host(rows[:, pos:pos + m]))
            pos += m
        else:
            gate.flush_device()
            gr, gp = gate.fetch()
        router.process_device(*gate.device_view())
        dropped += int((gr["channel"] == 8).sum())
        for k in range(2):
            what = f"{variant}, call {i}, route {k}"
            mine = filtered(gr, table, k)
            assert router.fetch(k)[0].tobytes() == mine.tobytes(), what
            (runs, payload), ev = routed_chains[k].call(router.device_view(k))
            (all_runs, all_payload), all_ev = plain_chains[k].call(gate.device_view())
            keep = np.asarray(table)[all_runs["channel"]] == k
            same_but(runs, all_runs[keep], ("out_offset",), what)
            per = (runs["nr_out"].astype(np.int64) + 31) // 32 if bits[k] else runs["nr_out"].astype(np.int64)
            assert np.array_equal(runs["out_offset"], np.cumsum(per) - per), what   # dense within the route
            for x, y in zip(slices(runs, payload, bits[k]), slices(all_runs[keep], all_payload, bits[k])):
                assert np.array_equal(x, y), what
            same_but(ev, all_ev[np.asarray(table)[all_ev["channel"]] == k], ("run",), what)
            (rs_want, rs_payload), ev_want = chk[k].call(mine, gp)
            same_ev[k](ev, ev_want, what)   # `run` indexes the route's list
            if not bits[k]:
                tr.same((runs, payload), (rs_want, rs_payload), what)
            seen[k] += len(ev)
    assert pos == rows.shape[1] and dropped >= 1 and seen[0] >= 3 and seen[1] >= 3, (dropped, seen)
    by = [c.stretches() for c in chk]   # each stretch once more through a fresh oracle chain in one piece
    assert {key[0] for key in by[0]} <= {0, 1, 2, 3} and {key[0] for key in by[1]} <= {4, 5, 6, 7} and len(by[0]) >= 3 and len(by[1]) >= 3
    for o in routed_chains + plain_chains + [router, gate, lv]:
        o.close()


@pytest.mark.gpu
def test_gpu_flex_route_beside_a_pocsag_route(pkg, ora):
    """the two FM FLEX channels of the chain scene of tests/test_runflex.py on route 1 at 16/25, two POCSAG rows beside them on
    route 0 at 4/5, one gate (P = 1, the scene's mask) in two calls and the flush: the FLEX route returns the events and frames of
    the FLEX chain fed the gate's own view, on those channels, and the oracle's"""
    sc, s = trf._chain(pkg, ora), trf.CHAIN
    W, P = s["W"], s["P"]
    n = sc["pcm"].shape[1] // W * W
    pg = trp.scene(pkg, ora, (4, 5, 41), 7)["stream"][:2]
    reps = -(-n // pg.shape[1])
    rows = np.ascontiguousarray(np.concatenate([np.tile(pg, (1, reps))[:, :n], sc["pcm"][:, :n]]))
    mask = np.concatenate([np.tile(np.array([[True] * 5 + [False] * 3]), (2, n // W // 8 + 1))[:, :n // W], sc["mask"][:, :n // W]])
    table = np.array([0, 0, 1, 1], np.uint8)
    cuts = [n // 3 + 17, n - (n // 3 + 17)]
    cap = max(cuts)
    gate = pkg.Gate(4, cap, W, preroll_windows=P)
    router = pkg.RunRouter.behind(table, 2, cap, W, preroll_windows=P)
    ptaps = trp.rs_taps(pkg, ora, (4, 5, 41))
    routed_chains = [Chain(pkg, 4, ptaps, (4, 5), W, cap, P, "pocsag"), Chain(pkg, 4, sc["rtaps"], (16, 25), W, cap, P, "flex")]
    plain_flex = Chain(pkg, 4, sc["rtaps"], (16, 25), W, cap, P, "flex")
    chk = [trp.Checker(pkg, ora, ptaps, 4, 5, W), trf.Checker(pkg, ora, sc["rtaps"], 16, 25, W)]
    pos, frames, got_by, all_by = 0, 0, {}, {}
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gr, gp = gate.process_host(rows[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W))
            pos += m
        else:
            gate.flush_device()
            gr, gp = gate.fetch()
        router.process_device(*gate.device_view())
        (runs, payload), ev = routed_chains[0].call(router.device_view(0))
        (rs_want, rs_payload), ev_want = chk[0].call(filtered(gr, table, 0), gp)
        tr.same((runs, payload), (rs_want, rs_payload), f"call {i}, the POCSAG route")
        trp.same(ev, ev_want, f"call {i}, the POCSAG route")
        (runs, payload), (ev, fw) = routed_chains[1].call(router.device_view(1))
        (rs_want, rs_payload), want = chk[1].call(filtered(gr, table, 1), gp)
        tr.same((runs, payload), (rs_want, rs_payload), f"call {i}, the FLEX route")
        trf.same((ev, fw), want, f"call {i}, the FLEX route")
        (all_runs, _), (all_ev, all_fw) = plain_flex.call(gate.device_view())
        same_but(runs, all_runs[all_runs["channel"] >= 2], ("out_offset",), f"call {i}")
        trf.per_stretch(ev, fw, got_by)
        trf.per_stretch(all_ev, all_fw, all_by)
        frames += len(fw)
    assert frames == 2 and got_by == {k: v for k, v in all_by.items() if k[0] >= 2} and {k[0] for k in got_by} == {2, 3}
    assert len(chk[0].stretches()) >= 2 and len(chk[1].stretches()) >= 2
    for o in routed_chains + [plain_flex, router, gate]:
        o.close()


@pytest.mark.gpu
def test_gpu_refused_router_call_makes_every_route_refuse_and_keeps_the_state(pkg, ora):
    """a call of three runs through a router made for two, the gate's two flags and a run of a channel that does not exist: each
    route's burst resampler refuses as it does behind a gate, twice (its two state buffers are used in turn), and the same input
    through a router that fits is right afterwards: channel 1's stretch continues"""
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D = 4, 5
    first, second = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    assert len(second[0]) == 3 and [int(c) for c in second[0]["channel"]] == [1, 1, 2]
    table = np.array([0, 1, 0], np.uint8)
    small, fits = pkg.RunRouter(table, 2, max_runs=2), pkg.RunRouter.behind(table, 2, 30, W)
    rrs = [pkg.RunResampler(nch, taps, I, D, W, max_in_samples=30) for _ in range(2)]
    chk = [tr.Checker(pkg, ora, taps, I, D, False, W) for _ in range(2)]

    def through(router, call, totals=None):
        keep = routed(torch, router, call[0], call[1], totals)
        out = []
        for k in range(2):
            rrs[k].process_device(*router.device_view(k))
            try:
                out.append(rrs[k].fetch())
            except pkg.MfmError as err:
                out.append(err)
        del keep
        return out

    for k, got in enumerate(through(fits, first)):
        tr.same(got, chk[k].call(filtered(first[0], table, k), first[1]), f"first call, route {k}")
    bad = second[0].copy()
    bad["channel"][2] = nch
    n2 = second[1].size
    for router, call, totals, message in ((small, second, None, "max_open_windows"), (small, second, None, "max_open_windows"),
                                          (fits, second, [3, n2, 1, 0], "max_open_windows"), (fits, second, [3, n2, 0, 1], "out of step"),
                                          (fits, (bad, second[1]), None, "out of step")):
        for k, err in enumerate(through(router, call, totals)):
            assert isinstance(err, pkg.MfmError) and err.code == b.MFM_E_STATE and message in str(err), (message, k, err)
            assert err.needed == (0, 0) and not err.buffers[0].view(np.uint8).any() and not err.buffers[1].any()
    want = [chk[k].call(filtered(second[0], table, k), second[1]) for k in range(2)]
    assert [int(f) for f in want[1][0]["flags"]] == [0, 1] and int(want[1][0]["nr_out"][0]) > 0   # channel 1 continues on route 1
    for k, got in enumerate(through(fits, second)):
        tr.same(got, want[k], f"second call after five refused ones, route {k}")
    for c in chk:
        c.stretches()
    for o in rrs + [small, fits]:
        o.close()


# ---- GPU: the tool ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_route_writes_what_the_single_chain_run_writes(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-route routes.json as a fresh child process on the chain scene of tests/test_runpocsag.py, channel
    0 on a pocsag route and channel 1 on an ais route: gated/pocsag/pocsag.jsonl and pages.jsonl hold the lines of the
    --gate-resample 4/5 --gate-pocsag run (also run here) that belong to channel 0, in their order"""
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
    (tmp_path / "twice.json").write_text(json.dumps({"routes": [dict(route, name="pocsag", stage="pocsag", channels=[0, 1]),
                                                                dict(route, name="ais", stage="ais", channels=[1])]}))
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
            str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(sc["thr"]),
            "--hang", str(s["hang"]), "--block", str(s["blk"]), "--gate-preroll", str(P)]
    single = base + ["--gate-out", str(tmp_path / "single"), "--gate-resample", "4/5", "--resample-taps", str(tmp_path / "filter.json"), "--gate-pocsag"]
    both = base + ["--gate-out", str(tmp_path / "gated"), "--gate-route", str(tmp_path / "routes.json")]
    outs = []
    for cmd in (single, both):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]   # what goes to stdout does not change
    for name in ("pocsag.jsonl", "pages.jsonl", "resampled.jsonl"):
        want = [ln for ln in (tmp_path / "single" / name).read_text().splitlines() if json.loads(ln)["channel"] == 0]
        got = (tmp_path / "gated" / "pocsag" / name).read_text().splitlines()
        assert got == want and (len(got) >= 3 or name == "pages.jsonl"), name
    assert len((tmp_path / "gated" / "pocsag" / "pages.jsonl").read_text().splitlines()) >= 1
    assert (tmp_path / "gated" / "pocsag" / "ch0000.rs.s16").read_bytes() == (tmp_path / "single" / "ch0000.rs.s16").read_bytes()
    assert not (tmp_path / "gated" / "pocsag" / "ch0001.rs.s16").exists()
    for name in ("index.jsonl", "ch0000.s16", "ch0001.s16"):   # the gate's files, as without the router
        assert (tmp_path / "gated" / name).read_bytes() == (tmp_path / "single" / name).read_bytes(), name
    assert (tmp_path / "gated" / "ais" / "ais.jsonl").exists()
    assert {json.loads(ln)["channel"] for ln in (tmp_path / "gated" / "ais" / "resampled.jsonl").read_text().splitlines()} == {1}
    r = subprocess.run(both + ["--gate-pocsag"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gate-route excludes" in r.stderr
    r = subprocess.run(base + ["--gate-out", str(tmp_path / "bad"), "--gate-route", str(tmp_path / "twice.json")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "channel 1 is in two routes" in r.stderr


BAD_ROUTE_FILES = [
    ([dict(name="a", stage="pocsag", channels=[0, 1]), dict(name="b", stage="ais", channels=[1])], "channel 1 is in two routes"),
    ([dict(name="a", stage="dmr", channels=[0])], "stage 'dmr' is none of ais, pocsag, flex, none"),
    ([dict(name="a", stage="flex", bits=True, channels=[0])], "bits needs stage ais or pocsag"),
    ([dict(name="a", stage="ais", bits=True, dc_pole=0.9, channels=[0])], "dc_pole and bits exclude each other"),
    ([dict(name="r%d" % i, stage="none", channels=[]) for i in range(9)], "9 routes; the run router takes 1 .. 8"),
    ([dict(name="a", stage="ais", channels=[2])], "channel 2 is not one of the configuration's 2"),
    ([dict(name="a", stage="ais", channels=[0]), dict(name="a", stage="none", channels=[1])], "used twice")]


def test_level_scan_tool_refuses_a_bad_route_file_before_it_sets_anything_up(tmp_path):
    """no device needed: the route file is checked before the engine is made"""
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}, {"chanCenterFreq": 929200000}]}))
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", os.devnull,
            "--gate-out", str(tmp_path / "gated"), "--gate-route", str(tmp_path / "routes.json")]
    for routes, message in BAD_ROUTE_FILES:
        (tmp_path / "routes.json").write_text(json.dumps({"routes": [dict(r, resample="4/5", taps="filter.json") for r in routes]}))
        r = subprocess.run(base, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (message, r.stderr[-500:])
    for flag in (["--gate-pocsag"], ["--gate-ais"], ["--gate-flex"], ["--gate-resample", "4/5"]):
        r = subprocess.run(base + flag, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--gate-route excludes" in r.stderr, flag
    r = subprocess.run([x for x in base if x not in ("--gate-out", str(tmp_path / "gated"))], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--gate-route needs --gate-out" in r.stderr
    assert not (tmp_path / "gated").exists()
