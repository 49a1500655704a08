"""The run router's local form (mfm_runroute_create_local, csrc/mfm_runroute_local.hip): PACK's route-local channel numbers and
capacities on the gate's payload in place.  payload_offset stays the gate's, a route's totals carry its own load, and the bound
of the payload ranges goes out through mfm_runroute_bound_view.

The checker is never the code under test: the rules of include/multifm_hip.h are restated in numpy (`restate`), PACK's host twin
is the reference for the relation between the two forms, and the tool's output under "local" is compared with its output under
"pack".  Every comparison is an equality."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_runpocsag as trp
import test_runroute as trr
import test_runroute_sets as trs

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runroute_create_local", "mfm_runroute_bound_view", "mfm_hosttwin_runroute_local_call"]
NCH, K, W = 257, 3, 64
COUNTS = [0, 1, 64, 1025, 1285]   # runs: none, one, a wave, across a strip of 1024, 257 channels x 5


# ---- the checker --------------------------------------------------------------------------------------------

def make_sets(nch=NCH):
    """route 0: every third channel (not contiguous); route 1: channels 100 .. 199; route 2: channels below 40 and above 249;
    channels in two routes and in all three among them, and channels in none"""
    c = np.arange(nch)
    sets = ((c % 3 == 0) * 1 | ((c >= 100) & (c < 200)) * 2 | ((c < 40) | (c >= 250)) * 4).astype(np.uint8)
    counts = {bin(int(s)).count("1") for s in sets}
    assert counts == {0, 1, 2} and int(sets[5]) == 4 and int(sets[1]) == 4 and int(sets[50]) == 0 and int(sets[102]) == 3
    sets[0] = 7
    return sets


_RUNS = {}


def make_runs(pkg, n, nch=NCH):
    """(runs, payload, totals) of a hand-made gate call of n runs, as test_runroute_sets.make_runs makes them.  n == 5 * nch: every
    channel has five runs, so the runs of every channel alternate with closed windows.  Made once per n and left unchanged"""
    if n not in _RUNS:
        rng = np.random.RandomState(31 + n)
        runs = np.zeros(n, pkg.binding.GATE_RUN_DTYPE)
        runs["channel"] = np.repeat(np.arange(nch), 5) if n == 5 * nch else np.sort(rng.randint(0, nch, n))
        runs["nr_windows"] = rng.randint(1, 6, n)
        runs["first_window"] = np.cumsum(runs["nr_windows"] + rng.randint(1, 3, n)) + (1 << 33)
        length = runs["nr_windows"].astype(np.int64) * W
        gap = rng.randint(0, 4, n) * 4
        runs["payload_offset"] = np.cumsum(length + gap) - length
        elems = int(runs["payload_offset"][-1] + length[-1]) + 5 if n else 0
        payload = rng.randint(-32768, 32768, elems).astype(np.int16)
        _RUNS[n] = (runs, payload, np.array([n, elems, 0, 0], np.uint64))
    return _RUNS[n]


def restate(sets, runs, totals, cap, route_caps=None):
    """([runs of route k], [totals of route k], the bound) by the rules of include/multifm_hip.h"""
    sets = np.asarray(sets)
    over, oos = int(totals[2] != 0), int(totals[3] != 0)
    if not over and not oos and int(totals[0]) > cap:
        over = 1
    if not over and not oos and (runs["channel"] >= len(sets)).any():
        oos = 1
    if over or oos:
        return [runs[:0]] * K, [[0, 0, over, oos]] * K, 0
    out_runs, out_totals = [], []
    for k in range(K):
        rk = runs[(sets[runs["channel"]] >> k) & 1 == 1].copy()
        windows = int(rk["nr_windows"].astype(np.int64).sum())
        if route_caps is not None and (len(rk) > route_caps[k][0] or windows > route_caps[k][1]):
            out_runs.append(rk[:0])
            out_totals.append([0, 0, 1, 0])
            continue
        rk["channel"] = np.searchsorted(np.flatnonzero((sets >> k) & 1), rk["channel"])
        out_runs.append(rk)
        out_totals.append([len(rk), windows * W, 0, 0])
    return out_runs, out_totals, int(totals[1])


def twin(pkg, sets, runs, totals, cap, route_caps=None):
    """the host twin's answer in the shape of restate()"""
    kw = {}
    if route_caps is not None:
        kw = dict(route_max_runs=[c[0] for c in route_caps], route_max_windows=[c[1] for c in route_caps])
    rows, t, bound = pkg.hosttwin_runroute_local_call(sets, K, runs, totals, W, max_runs=cap, **kw)
    return [rows[k][:int(t[k][0])] for k in range(K)], [[int(x) for x in t[k]] for k in range(K)], bound


def same(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[2] == want[2], (what, got[2], want[2])
    trr.same_lists(got[0], want[0], what)


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_local_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define MFM_ABI_VERSION 4\b", src) and b.MFM_ABI_VERSION == 4
    assert pkg.hosttwin_runroute_local_call is b.hosttwin_runroute_local_call and callable(pkg.RunRouter.bound_view)


@pytest.mark.parametrize("n", COUNTS)
def test_hosttwin_equals_the_restatement(pkg, n):
    sets = make_sets()
    runs, _, totals = make_runs(pkg, n)
    got = twin(pkg, sets, runs, totals, max(n, 1))
    same(got, restate(sets, runs, totals, max(n, 1)), f"n {n}")
    if n >= 1025:
        assert sum(len(r) for r in got[0]) > int((sets[runs["channel"]] != 0).sum())   # runs of shared channels stand in several lists
        assert all(len(r) > 64 for r in got[0]) and 0 < int((sets[runs["channel"]] == 0).sum())
        for k in range(K):   # stable, channels still ascend, and the numbering inverts
            members = np.flatnonzero((sets >> k) & 1)
            mine = runs[(sets[runs["channel"]] >> k) & 1 == 1]
            assert (np.diff(got[0][k]["channel"].astype(np.int64)) >= 0).all() and np.array_equal(members[got[0][k]["channel"]], mine["channel"])
            assert np.array_equal(got[0][k]["payload_offset"], mine["payload_offset"])


@pytest.mark.parametrize("n", COUNTS)
def test_the_local_twin_and_packs_twin_describe_the_same_windows(pkg, n):
    """for every route: records equal except payload_offset, gate_payload[offset : offset + n] equals PACK's payload slice, totals
    equal, and the bound is the gate's total"""
    sets = make_sets()
    runs, payload, totals = make_runs(pkg, n)
    lists, t, bound = twin(pkg, sets, runs, totals, max(n, 1))
    plists, pt, ppay = trs.twin(pkg, sets, K, runs, payload, totals, max(n, 1), True, W)
    assert t == pt and bound == int(totals[1])
    for k in range(K):
        trr.same_but(lists[k], plists[k], ("payload_offset",), f"n {n}, route {k}")
        for r, p in zip(lists[k], plists[k]):
            m = int(r["nr_windows"]) * W
            assert np.array_equal(payload[int(r["payload_offset"]):int(r["payload_offset"]) + m], ppay[k][int(p["payload_offset"]):int(p["payload_offset"]) + m])
        assert len(lists[k]) > 0 or n < 64


def test_a_route_over_its_own_capacity_is_flagged_alone(pkg):
    """one short in runs and one short in windows: that route gets [0, 0, 1, 0], the others are byte-identical to the call
    without the limit"""
    sets = make_sets()
    runs, _, totals = make_runs(pkg, 1285)
    free = restate(sets, runs, totals, 1285)
    need = [(t[0], t[1] // W) for t in free[1]]   # runs, windows each route carries
    for k, short in ((0, "runs"), (1, "windows"), (2, "runs"), (2, "windows")):
        caps = [list(c) for c in need]
        caps[k][0 if short == "runs" else 1] -= 1
        got = twin(pkg, sets, runs, totals, 1285, route_caps=caps)
        same(got, restate(sets, runs, totals, 1285, route_caps=caps), f"route {k} short of {short}")
        assert got[1][k] == [0, 0, 1, 0] and got[2] == int(totals[1])
        for j in range(K):
            if j != k:
                assert got[1][j] == free[1][j] and got[0][j].tobytes() == free[0][j].tobytes()
    same(twin(pkg, sets, runs, totals, 1285, route_caps=need), free, "capacities that fit exactly")


REFUSED = [("the gate's overflow", dict(over=1), [0, 0, 1, 0]), ("the gate's out of step", dict(oos=1), [0, 0, 0, 1]),
           ("both of the gate's flags", dict(over=7, oos=9), [0, 0, 1, 1]), ("runs beyond capacity", dict(cap=1284), [0, 0, 1, 0]),
           ("a channel beyond the table", dict(bad=1100), [0, 0, 0, 1]), ("a channel beyond the table in the last run", dict(bad=1284), [0, 0, 0, 1])]


def refused_case(pkg, change):
    runs, _, totals = make_runs(pkg, 1285)
    runs, totals = runs.copy(), totals.copy()
    if "bad" in change:
        runs["channel"][change["bad"]] = NCH
    totals[2], totals[3] = change.get("over", 0), change.get("oos", 0)
    return runs, totals, change.get("cap", 1285)


@pytest.mark.parametrize("what,change,want", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_hosttwin_refusals_flag_every_route_and_the_bound_is_zero(pkg, what, change, want):
    sets = make_sets()
    runs, totals, cap = refused_case(pkg, change)
    got = twin(pkg, sets, runs, totals, cap)
    same(got, restate(sets, runs, totals, cap), what)
    assert got[1] == [want] * K and got[2] == 0


def test_a_payload_range_outside_the_gates_elements_is_not_the_routers_to_refuse(pkg):
    """nothing is copied, so nothing is read: the range is the burst resampler's view entry's to check"""
    sets = make_sets()
    runs, _, totals = make_runs(pkg, 1285)
    totals = totals.copy()
    totals[1] -= 6   # the last run now ends past the gate's elements
    got = twin(pkg, sets, runs, totals, 1285)
    same(got, restate(sets, runs, totals, 1285), "a short total")
    assert all(t[2:] == [0, 0] and t[0] for t in got[1]) and got[2] == int(totals[1])


CREATE_REFUSALS = [(dict(entry=8), {}, "routes_of_channel[5] = 0x08 has a bit at or above nr_routes = 3"),
                   (dict(empty=1), {}, "route 1 has no channel: behind mfm_runroute_create_local"),
                   ({}, dict(flags=1), "flags must be 0: mfm_runroute_create_local takes none"), ({}, dict(flags=2), "flags must be 0"),
                   ({}, dict(nr_routes=9), "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES"), ({}, dict(abi_version=1), "abi_version"),
                   ({}, dict(max_in_samples=0), "max_in_samples is 0"),
                   ({}, dict(max_in_samples=0, max_runs=5), "mfm_runroute_create_local with max_in_samples 0 needs max_windows and max_runs"),
                   ({}, dict(max_in_samples=0, max_windows=5), "max_in_samples is 0"),
                   ({}, dict(window_samples=0, max_runs=5), "window_samples must be 1 .. 2^20"),
                   ({}, dict(window_samples=(1 << 20) + 1, max_runs=5), "window_samples must be 1 .. 2^20")]


@pytest.mark.parametrize("table,change,message", CREATE_REFUSALS, ids=[str(sorted({**t, **c}.items())) for t, c, _ in CREATE_REFUSALS])
def test_create_local_refuses_with_a_message(pkg, table, change, message):
    """what mfm_runroute_create_local refuses it refuses before it looks for a device"""
    b = pkg.binding
    sets = trs.make_sets(3, 16)
    if "entry" in table:
        sets[5] = table["entry"]
    if "empty" in table:
        sets &= ~np.uint8(1 << table["empty"])
    kw = dict(nr_routes=3, window_samples=64, max_in_samples=4096)
    kw.update(change)
    nr_routes = kw.pop("nr_routes")
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunRouter(None, nr_routes, sets=sets, local=True, **kw)
    assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_the_binding_keeps_local_apart_from_pack_and_from_the_route_table_form(pkg):
    for kw in (dict(sets=np.ones(4, np.uint8), pack=True, local=True), dict(route_of_channel=np.zeros(4, np.uint8), local=True)):
        with pytest.raises(ValueError):
            pkg.RunRouter(nr_routes=1, window_samples=64, max_in_samples=64, **kw)


def test_the_twin_refuses_a_table_create_refuses(pkg):
    b = pkg.binding
    runs, _, totals = make_runs(pkg, 64)
    for sets, nr_routes, message in ((np.full(NCH, 8, np.uint8), 3, "has a bit at or above nr_routes = 3"), (make_sets(), 9, "nr_routes must be")):
        with pytest.raises(pkg.MfmError) as ei:
            pkg.hosttwin_runroute_local_call(sets, nr_routes, runs, totals, W)
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)


def test_local_kernel_uses_no_scratch_and_does_not_spill():
    """the code object's notes of build/mfm_runroute_local.o (tools/kernel_regs.py): the one partition kernel, no private segment,
    no spilled register, registers for sixteen waves on a compute unit"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runroute_local.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_runroute_local.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert [ln.split()[0] for ln in lines] == ["rt_local_kernel"], out
    m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", lines[0])
    assert m and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), lines[0]
    assert int(m.group(1)) <= 128, lines[0]   # 1024 lanes: sixteen waves on a compute unit's four SIMDs, 512 / 4 registers each
    assert int(m.group(4)) == 2 * 8 * 16 * 4 + 8 * 16 * 8 + 16 * 4 + 8 * 4, lines[0]   # wave counts twice, window sums, bad, capacities


def test_level_scan_tool_reads_local_and_refuses_it_beside_pack_before_it_sets_anything_up(tmp_path):
    """no device needed: the route file is checked before the engine is made"""
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}, {"chanCenterFreq": 929200000}]}))
    route = dict(resample="4/5", taps="filter.json")
    twice = [dict(route, name="a", stage="pocsag", channels=[0, 1]), dict(route, name="b", stage="flex", channels=[1])]
    path = str(tmp_path / "routes.json")
    tool = trs._tool()
    for extra, want in ((dict(shared=True, local=True), (True, False, True)), (dict(shared=True), (True, False, False)),
                        (dict(shared=True, pack=True, local=False), (True, True, False))):
        (tmp_path / "routes.json").write_text(json.dumps(dict(extra, routes=twice)))
        routes, shared, pack = tool.read_routes(path, 2)
        assert (shared, pack, routes.local) == want and [r["channels"] for r in routes] == [[0, 1], [1]]
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", os.devnull,
            "--gate-out", str(tmp_path / "gated"), "--gate-route", path]
    bad = [(dict(routes=twice, shared=True, local=True, pack=True), '"local" and "pack" exclude each other'),
           (dict(routes=twice, local=True), "channel 1 is in two routes"), (dict(routes=twice, shared=True, local="yes"), '"local" must be true or false'),
           (dict(routes=twice + [dict(route, name="c", stage="none", channels=[])], shared=True, local=True), "route c has no channel")]
    for doc, message in bad:
        (tmp_path / "routes.json").write_text(json.dumps(doc))
        r = subprocess.run(base, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (message, r.stderr[-500:])
    assert not (tmp_path / "gated").exists()


# ---- GPU: the router against its twin ---------------------------------------------------------------------------------

def _bound(router):
    """the uint64 behind bound_view(), after the work queued so far"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(1, np.uint64)
    assert hip.hipMemcpy(out.ctypes.data, router.bound_view(), 8, 2) == 0
    return int(out[0])


@pytest.mark.gpu
def test_gpu_equals_the_twin(pkg):
    """forged gate arrays uploaded directly: 1285 runs (the walk crosses a strip: the carried bases and the 64-bit sums), fewer,
    none; each of the gate's flags, more runs than the router holds, a run of channel 257; a route over its own capacity.  Runs,
    totals and the bound of every route, and what the accessors say"""
    import torch
    b = pkg.binding
    sets = make_sets()
    router = pkg.RunRouter(None, K, sets=sets, local=True, window_samples=W, max_runs=1285, max_windows=5 * 1285)
    caps = [router.route_caps(k) for k in range(K)]
    assert router.capacity() == 1285 and caps == [(int(((sets >> k) & 1).sum()), 5 * 1285, 1285) for k in range(K)]
    views, at = [router.device_view(k) for k in range(K)], router.bound_view()
    assert all(v[1] is None for v in views) and at and _bound(router) == 0
    for k in range(K):
        assert np.array_equal(router.route_channels(k), np.flatnonzero((sets >> k) & 1))

    def check(runs, payload, totals, what, refused=None):
        keep = trr.routed(torch, router, runs, payload, totals)
        want = twin(pkg, sets, runs, totals, 1285)
        got = ([], [], None)
        for k in range(K):
            if refused:
                with pytest.raises(pkg.MfmError) as ei:
                    router.fetch(k)
                assert ei.value.code == b.MFM_E_STATE and ei.value.needed == 0 and refused in str(ei.value), (what, str(ei.value))
                assert want[1][k][:2] == [0, 0] and want[1][k][2:] != [0, 0]
            else:
                g, load = router.fetch(k)
                got[0].append(g)
                got[1].append([len(g), load, 0, 0])
            d_runs, d_payload, d_totals = router.device_view(k)
            assert (d_runs, d_totals) == views[k][::2] and d_payload == keep[1].data_ptr()   # fixed at create; the gate's pointer
        assert router.bound_view() == at and _bound(router) == want[2] == (0 if refused else int(totals[1])), what
        if not refused:
            same((got[0], got[1], want[2]), want, what)
        del keep

    for n in (1285, 1025, 64, 1, 0, 1285):
        check(*make_runs(pkg, n), f"n {n}")
        with pytest.raises(pkg.MfmError) as ei:
            router.fetch_payload(0)
        assert ei.value.code == b.MFM_E_INVAL and "MFM_RUNROUTE_F_PACK" in str(ei.value)
    payload = make_runs(pkg, 1285)[1]
    for what, change, want in REFUSED:
        if "cap" in change:
            continue
        runs, totals, _ = refused_case(pkg, change)
        assert twin(pkg, sets, runs, totals, 1285)[1] == [want] * K
        check(runs, payload, totals, what, refused="out of step" if want[3] else "overflowed")
        check(*make_runs(pkg, 1025), "the router carries no state: the next call is right")
    router.close()
    small = pkg.RunRouter(None, K, sets=sets, local=True, window_samples=W, max_runs=1284, max_windows=5 * 1285)
    keep = trr.routed(torch, small, *make_runs(pkg, 1285))
    for k in range(K):
        with pytest.raises(pkg.MfmError) as ei:
            small.fetch(k)
        assert ei.value.code == b.MFM_E_STATE and "overflowed" in str(ei.value)
    assert _bound(small) == 0
    del keep
    small.close()
    for maker in (lambda: pkg.RunRouter(None, K, sets=sets, window_samples=W, max_runs=8, max_windows=8),
                  lambda: pkg.RunRouter(None, K, sets=sets, pack=True, window_samples=W, max_runs=8, max_windows=8),
                  lambda: pkg.RunRouter(np.zeros(NCH, np.uint8), K, max_runs=8)):
        other = maker()
        with pytest.raises(pkg.MfmError) as ei:
            other.bound_view()
        assert ei.value.code == b.MFM_E_INVAL and "mfm_runroute_create_local" in str(ei.value)
        other.close()


@pytest.mark.gpu
def test_gpu_a_route_over_its_own_capacity_is_flagged_alone(pkg):
    """an explicit max_windows one short of what the busiest route carries: that route overflows, the others are the twin's"""
    import torch
    b = pkg.binding
    sets = make_sets()
    runs, payload, totals = make_runs(pkg, 1285)
    need = [(t[0], t[1] // W) for t in restate(sets, runs, totals, 1285)[1]]
    router = pkg.RunRouter(None, K, sets=sets, local=True, window_samples=W, max_runs=1285, max_windows=max(c[1] for c in need) - 1,
                           max_in_samples=5 * W * 1285)
    caps = [router.route_caps(k)[:0:-1] for k in range(K)]   # (runs, windows)
    want = restate(sets, runs, totals, router.capacity(), route_caps=caps)
    over = [t[2] for t in want[1]]
    assert 0 < sum(over) < K, (caps, need)
    same(twin(pkg, sets, runs, totals, router.capacity(), route_caps=caps), want, "the twin")
    keep = trr.routed(torch, router, runs, payload, totals)
    for k in range(K):
        if over[k]:
            with pytest.raises(pkg.MfmError) as ei:
                router.fetch(k)
            assert ei.value.code == b.MFM_E_STATE and "overflowed" in str(ei.value)
        else:
            g, load = router.fetch(k)
            assert g.tobytes() == want[0][k].tobytes() and load == want[1][k][1]
    assert _bound(router) == int(totals[1])
    del keep
    router.close()


# ---- GPU: the tool ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_level_scan_tool_writes_under_local_what_it_writes_under_pack(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-out ... --gate-route on the chain scene of tests/test_runpocsag.py, channel 1 on a POCSAG
    route (4/5) and channels 0 and 1 on a FLEX route (16/25, with the DC blocker), once with "local" and once with "pack": every
    file under both output folders is byte-identical, which covers the true-channel mapping and the stages behind"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    fs, decim, Wt, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 929000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "flex.json").write_text(json.dumps({"lpfCoeffs": [float(t) * 16.0 for t in pkg.synth.design_lpf(101, 0.45 / 25, 1.0)]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    routes = [dict(name="pocsag", stage="pocsag", resample="4/5", taps=str(tmp_path / "filter.json"), channels=[1]),
              dict(name="flex", stage="flex", resample="16/25", taps=str(tmp_path / "flex.json"), dc_pole=0.999, channels=[0, 1])]
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
            str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(Wt), "--open-thr", str(sc["thr"]),
            "--hang", str(s["hang"]), "--block", str(s["blk"]), "--gate-preroll", str(P)]
    outs = []
    for form in ("local", "pack"):
        (tmp_path / (form + ".json")).write_text(json.dumps({"shared": True, form: True, "routes": routes}))
        r = subprocess.run(base + ["--gate-out", str(tmp_path / form), "--gate-route", str(tmp_path / (form + ".json"))], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    files = {}
    for form in ("local", "pack"):
        top = tmp_path / form
        files[form] = {str(p.relative_to(top)): p.read_bytes() for p in sorted(top.rglob("*")) if p.is_file()}
    assert sorted(files["local"]) == sorted(files["pack"])
    for name in files["pack"]:
        assert files["local"][name] == files["pack"][name], name
    lines = [json.loads(ln) for ln in files["local"][os.path.join("pocsag", "pocsag.jsonl")].decode().splitlines()]
    assert len(lines) >= 3 and {ln["channel"] for ln in lines} == {1}   # local channel 0 of the route is channel 1
    both = {json.loads(ln)["channel"] for ln in files["local"][os.path.join("flex", "resampled.jsonl")].decode().splitlines()}
    assert both == {0, 1} and os.path.join("pocsag", "ch0001.rs.s16") in files["local"] and os.path.join("flex", "ch0000.rs.s16") in files["local"]
