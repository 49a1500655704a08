"""The run router's sets form (mfm_runroute_create_sets, csrc/mfm_runroute_sets.hip): a channel's table byte is a set of routes,
and under MFM_RUNROUTE_F_PACK every route gets route-local channel numbers, dense offsets and a payload of its own, so that the
chain behind it is sized to the route (mfm_runroute_route_caps).

The checker is never the code under test: the rules of include/multifm_hip.h are restated in numpy (`restate`), the old form's
host twin is the reference for one-hot tables, and a routed chain is compared with the single-protocol chain that reads the
gate's own view, on the route's channels.  Every comparison is an equality."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_runflex as trf
import test_runpocsag as trp
import test_runroute as trr
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runroute_create_sets", "mfm_runroute_route_channels", "mfm_runroute_route_caps", "mfm_runroute_fetch_payload",
             "mfm_hosttwin_runroute_route_caps", "mfm_hosttwin_runroute_sets_call"]
NCH = 12
ROUTES = [1, 3, 8]
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2500]   # runs: across a wave, a workgroup's strip and several strips
WINDOWS = [1, 64, 100]                                 # W * 2 bytes: never, always and sometimes a multiple of 16


# ---- the checker --------------------------------------------------------------------------------------------

def make_sets(K, nch=NCH):
    """channel c: nowhere, one route, two routes (one when K == 1), all K routes, in turn; every route has a channel"""
    full = (1 << K) - 1
    return np.array([[0, 1 << (c % K), (1 << (c % K)) | (1 << ((c + 1) % K)), full][c % 4] for c in range(nch)], np.uint8)


def one_hot(K, nch=NCH):
    """(sets, the route table it corresponds to): every third channel nowhere"""
    route = np.array([trr.NONE if c % 3 == 2 else c % K for c in range(nch)], np.uint8)
    return np.where(route == trr.NONE, 0, 1 << (route % 8)).astype(np.uint8), route


_RUNS = {}


def make_runs(pkg, n, W, nch=NCH):
    """(runs, payload, totals) of a hand-made gate call of n runs, as test_runroute.make_runs makes them: channels ascending, a
    channel's windows ascending, 1 .. 5 windows a run, payload offsets that leave holes of 0, 4, 8 or 12 elements (so runs begin
    on and off 16 bytes), a random payload.  Made once per (n, W) and left unchanged"""
    if (n, W) not in _RUNS:
        rng = np.random.RandomState(11 + n + 7 * W)
        runs = np.zeros(n, pkg.binding.GATE_RUN_DTYPE)
        runs["channel"] = np.sort(rng.randint(0, nch, n))
        runs["nr_windows"] = rng.randint(1, 6, n)
        runs["first_window"] = np.cumsum(runs["nr_windows"] + rng.randint(1, 3, n)) + (1 << 33)
        length = runs["nr_windows"].astype(np.int64) * W
        gap = rng.randint(0, 4, n) * 4
        runs["payload_offset"] = np.cumsum(length + gap) - length
        elems = int(runs["payload_offset"][-1] + length[-1]) + 5 if n else 0
        payload = rng.randint(-32768, 32768, elems).astype(np.int16)
        _RUNS[(n, W)] = (runs, payload, np.array([n, elems, 0, 0], np.uint64))
    return _RUNS[(n, W)]


def restate(sets, K, runs, payload, totals, cap, pack, W, route_caps=None):
    """([runs of route k], [totals of route k], [payload of route k] or None) by the rules of include/multifm_hip.h"""
    sets = np.asarray(sets)
    over, oos = int(totals[2] != 0), int(totals[3] != 0)
    if not over and not oos and int(totals[0]) > cap:
        over = 1
    if not over and not oos and (runs["channel"] >= len(sets)).any():
        oos = 1
    length = runs["nr_windows"].astype(np.int64) * W
    if not over and not oos and pack and (runs["payload_offset"].astype(np.int64) + length > int(totals[1])).any():
        oos = 1
    if over or oos:
        return [runs[:0]] * K, [[0, 0, over, oos]] * K, [payload[:0]] * K if pack else None
    out_runs, out_totals, out_payloads = [], [], []
    for k in range(K):
        mine = (sets[runs["channel"]] >> k) & 1 == 1
        rk = runs[mine].copy()
        if not pack:
            out_runs.append(rk)
            out_totals.append([len(rk), int(totals[1]), 0, 0])
            continue
        if route_caps is not None and (len(rk) > route_caps[k][0] or int(rk["nr_windows"].sum()) > route_caps[k][1]):
            out_runs.append(rk[:0])
            out_totals.append([0, 0, 1, 0])
            out_payloads.append(payload[:0])
            continue
        members = np.flatnonzero((sets >> k) & 1)
        lk = length[mine]
        pieces = [payload[int(o):int(o) + int(m)] for o, m in zip(rk["payload_offset"], lk)]
        rk["channel"] = np.searchsorted(members, rk["channel"])
        rk["payload_offset"] = np.cumsum(lk) - lk
        out_runs.append(rk)
        out_totals.append([len(rk), int(lk.sum()), 0, 0])
        out_payloads.append(np.concatenate(pieces) if pieces else payload[:0])
    return out_runs, out_totals, out_payloads if pack else None


def twin(pkg, sets, K, runs, payload, totals, cap, pack, W, route_caps=None):
    """the host twin's answer in the shape of restate()"""
    kw = {}
    if route_caps is not None:
        kw = dict(route_max_runs=[c[0] for c in route_caps], route_max_windows=[c[1] for c in route_caps])
    got = pkg.hosttwin_runroute_sets_call(sets, K, runs, totals, max_runs=cap, pack=pack, window_samples=W, gate_payload=payload, **kw)
    rows, t = got[0], got[1]
    lists = [rows[k][:int(t[k][0])] for k in range(K)]
    payloads = [got[2][k][:int(t[k][1])] for k in range(K)] if pack else None
    return lists, [[int(x) for x in t[k]] for k in range(K)], payloads


def same(got, want, what):
    (gr, gt, gp), (wr, wt, wp) = got, want
    assert gt == wt, (what, gt, wt)
    trr.same_lists(gr, wr, what)
    assert (gp is None) == (wp is None), what
    for k in range(len(wr) if wp is not None else 0):
        assert gp[k].dtype == wp[k].dtype and np.array_equal(gp[k], wp[k]), f"{what}: the payload of route {k} differs"


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_sets_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define MFM_RUNROUTE_F_PACK 1u", src) and b.MFM_RUNROUTE_F_PACK == pkg.MFM_RUNROUTE_F_PACK == 1
    assert re.search(r"#define MFM_ABI_VERSION %d\b" % b.MFM_ABI_VERSION, src)
    assert pkg.hosttwin_runroute_sets_call is b.hosttwin_runroute_sets_call and pkg.hosttwin_runroute_route_caps is b.hosttwin_runroute_route_caps
    for name in ("route_channels", "route_caps", "fetch_payload", "behind"):
        assert callable(getattr(pkg.RunRouter, name)), name


@pytest.mark.parametrize("K", ROUTES)
@pytest.mark.parametrize("n", COUNTS)
def test_hosttwin_equals_the_restatement(pkg, n, K):
    sets = make_sets(K)
    bits = {bin(int(s)).count("1") for s in sets}   # nowhere, one route, several, all
    assert bits >= {0, 1, K} and (K < 3 or 2 in bits) and all(((sets >> k) & 1).any() for k in range(K))
    shared = 0
    for W in WINDOWS:
        runs, payload, totals = make_runs(pkg, n, W)
        for pack in (False, True):
            what = f"n {n} K {K} W {W} pack {pack}"
            got = twin(pkg, sets, K, runs, payload, totals, max(n, 1), pack, W)
            same(got, restate(sets, K, runs, payload, totals, max(n, 1), pack, W), what)
            shared += sum(len(r) for r in got[0]) > n
    assert shared or n < 63 or K == 1   # runs of shared channels stand in several lists


@pytest.mark.parametrize("K", ROUTES)
def test_a_one_hot_table_without_pack_equals_the_route_table_form_byte_for_byte(pkg, K):
    sets, route = one_hot(K)
    for n in COUNTS:
        runs, _, totals = make_runs(pkg, n, 64)
        new_rows, new_totals = pkg.hosttwin_runroute_sets_call(sets, K, runs, totals, max_runs=max(n, 1))
        old_rows, old_totals = pkg.hosttwin_runroute_call(route, K, runs, totals, max_runs=max(n, 1))
        assert new_rows.tobytes() == old_rows.tobytes() and new_totals.tobytes() == old_totals.tobytes(), (K, n)
        assert int(new_totals[:, 0].sum()) == int((route[runs["channel"]] != trr.NONE).sum())


def test_under_pack_offsets_are_dense_channels_are_ranks_and_the_payload_is_the_gates_windows(pkg):
    K, W = 3, 100
    sets = make_sets(K)
    runs, payload, totals = make_runs(pkg, 2500, W)
    lists, t, payloads = twin(pkg, sets, K, runs, payload, totals, 2500, True, W)
    for k in range(K):
        members = np.flatnonzero((sets >> k) & 1)   # what mfm_runroute_route_channels returns (the GPU test reads it)
        mine = runs[np.isin(runs["channel"], members)]
        g = lists[k]
        assert len(g) == len(mine) == t[k][0] > 100
        length = g["nr_windows"].astype(np.int64) * W
        assert np.array_equal(g["payload_offset"], np.cumsum(length) - length) and t[k][1] == int(length.sum()) == len(payloads[k])
        assert int(g["channel"].max()) < len(members) and (np.diff(g["channel"].astype(np.int64)) >= 0).all()
        assert np.array_equal(members[g["channel"]], mine["channel"])   # the numbering inverts
        assert np.array_equal(g["first_window"], mine["first_window"]) and np.array_equal(g["nr_windows"], mine["nr_windows"])
        for i in (0, 1, len(g) // 2, len(g) - 1):
            o, m = int(mine["payload_offset"][i]), int(length[i])
            assert np.array_equal(payloads[k][int(g["payload_offset"][i]):int(g["payload_offset"][i]) + m], payload[o:o + m])


CAPS_CASES = [dict(window_samples=64, max_in_samples=4096), dict(window_samples=64, max_in_samples=4095, preroll_windows=2),
              dict(window_samples=500, max_in_samples=100, preroll_windows=7), dict(window_samples=1, max_in_samples=1000),
              dict(window_samples=64, max_in_samples=4096, max_windows=40), dict(window_samples=64, max_in_samples=4096, max_runs=9),
              dict(window_samples=64, max_in_samples=4096, max_windows=100000, max_runs=100000),
              dict(window_samples=100, max_in_samples=1 << 20, preroll_windows=63), dict(window_samples=64, max_in_samples=0, max_windows=77, max_runs=5)]


def test_route_caps_is_the_documented_rule(pkg):
    """include/multifm_hip.h: under PACK, for a route of n channels and per = max(max_in_samples / W + 1, P): n, n * per and no
    more than an explicit max_windows, min(max_windows, n * ceil(per / 2)) and no more than an explicit max_runs; with
    max_in_samples == 0 both as given.  Without PACK the whole gate's: nr_channels, max_windows as given, the router's max_runs"""
    for K in ROUTES:
        sets = make_sets(K)
        for kw in CAPS_CASES:
            for k in range(K):
                n = int(((sets >> k) & 1).sum())
                if kw["max_in_samples"]:
                    per = max(kw["max_in_samples"] // kw["window_samples"] + 1, kw.get("preroll_windows", 0))
                    windows = min(kw.get("max_windows", 0) or n * per, n * per)
                    want = (n, windows, min(kw.get("max_runs", 0) or windows, windows, n * ((per + 1) // 2)))
                else:
                    want = (n, kw["max_windows"], kw["max_runs"])
                assert pkg.hosttwin_runroute_route_caps(sets, K, k, pack=True, **kw) == want, (K, k, kw)
                whole = pkg.hosttwin_runroute_capacity(np.zeros(NCH, np.uint8), 1, **kw)   # the old form's run capacity
                assert pkg.hosttwin_runroute_route_caps(sets, K, k, **kw) == (NCH, kw.get("max_windows", 0), whole), (K, k, kw)
    kw = dict(window_samples=64, max_in_samples=4096)
    assert sum(pkg.hosttwin_runroute_route_caps(make_sets(3), 3, k, pack=True, **kw)[1] for k in range(3)) > NCH * 65   # shared channels count twice


CREATE_REFUSALS = [(dict(entry=8), {}, "routes_of_channel[5] = 0x08 has a bit at or above nr_routes = 3"),
                   (dict(entry=0x81), {}, "routes_of_channel[5] = 0x81 has a bit at or above nr_routes = 3"),
                   (dict(empty=1), dict(pack=True), "route 1 has no channel"), ({}, dict(flags=2), "flags must be 0 or MFM_RUNROUTE_F_PACK"),
                   ({}, dict(flags=4, pack=True), "flags must be 0 or MFM_RUNROUTE_F_PACK"), ({}, dict(nr_routes=9), "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES"),
                   ({}, dict(abi_version=1), "abi_version"), ({}, dict(max_in_samples=0), "max_in_samples is 0"),
                   ({}, dict(max_in_samples=0, max_runs=5, pack=True), "needs max_windows and max_runs"),
                   ({}, dict(window_samples=0, max_runs=5, pack=True), "window_samples must be 1 .. 2^20")]


@pytest.mark.parametrize("table,change,message", CREATE_REFUSALS, ids=[str(sorted({**t, **c}.items())) for t, c, _ in CREATE_REFUSALS])
def test_create_sets_refuses_with_a_message(pkg, table, change, message):
    """mfm_runroute_create_sets itself and its twin: what they refuse they refuse before they look for a device"""
    b = pkg.binding
    sets = make_sets(3, 16)
    if "entry" in table:
        sets[5] = table["entry"]
    if "empty" in table:
        sets &= ~np.uint8(1 << table["empty"])
    kw = dict(nr_routes=3, window_samples=64, max_in_samples=4096)
    kw.update(change)
    K = kw.pop("nr_routes")
    for make in (lambda: pkg.RunRouter(None, K, sets=sets, **kw), lambda: pkg.hosttwin_runroute_route_caps(sets, K, 0, **kw)):
        with pytest.raises(pkg.MfmError) as ei:
            make()
        assert ei.value.code == b.MFM_E_INVAL and message in str(ei.value), str(ei.value)
    # the old entry keeps its own refusal of any flag
    with pytest.raises(pkg.MfmError) as ei:
        pkg.RunRouter(np.zeros(16, np.uint8), 3, window_samples=64, max_in_samples=4096, flags=1)
    assert "flags must be 0" in str(ei.value) and "PACK" not in str(ei.value)


REFUSED = [("the gate's overflow", dict(over=1), [0, 0, 1, 0]), ("the gate's out of step", dict(oos=1), [0, 0, 0, 1]),
           ("both of the gate's flags", dict(over=7, oos=9), [0, 0, 1, 1]), ("runs beyond capacity", dict(cap=256), [0, 0, 1, 0]),
           ("a channel beyond the table", dict(bad=200), [0, 0, 0, 1]), ("a channel beyond the table in the last run", dict(bad=256), [0, 0, 0, 1])]
PACK_REFUSED = REFUSED + [("a payload range beyond the gate's elements", dict(short=1), [0, 0, 0, 1])]


def refused_case(pkg, change, W=64):
    runs, payload, totals = make_runs(pkg, 257, W)
    runs, totals = runs.copy(), totals.copy()
    if "bad" in change:
        runs["channel"][change["bad"]] = NCH
    if "short" in change:
        totals[1] -= 6   # the last run now ends past the gate's elements
    totals[2], totals[3] = change.get("over", 0), change.get("oos", 0)
    return runs, payload, totals, change.get("cap", 257)


@pytest.mark.parametrize("pack", [False, True], ids=["zero_copy", "pack"])
@pytest.mark.parametrize("what,change,want", PACK_REFUSED, ids=[r[0].replace(" ", "_") for r in PACK_REFUSED])
def test_hosttwin_refusals_flag_every_route(pkg, what, change, want, pack):
    runs, payload, totals, cap = refused_case(pkg, change)
    if "short" in change and not pack:
        want = None   # without PACK nothing is copied and the range is the burst resampler's to check: not refused
    for K in ROUTES:
        sets = make_sets(K)
        got = twin(pkg, sets, K, runs, payload, totals, cap, pack, 64)
        same(got, restate(sets, K, runs, payload, totals, cap, pack, 64), what)
        assert got[1] == [want] * K or (want is None and all(t[2:] == [0, 0] and t[0] for t in got[1])), (what, got[1])


def test_a_route_over_its_own_capacity_under_pack_is_flagged_alone(pkg):
    K, W = 3, 64
    sets = make_sets(K)
    runs, payload, totals = make_runs(pkg, 257, W)
    free = restate(sets, K, runs, payload, totals, 257, True, W)
    need = [(t[0], t[1] // W) for t in free[1]]   # runs, windows each route carries
    for k, short in ((0, "runs"), (1, "windows"), (2, "runs")):
        caps = [list(c) for c in need]
        caps[k][0 if short == "runs" else 1] -= 1
        got = twin(pkg, sets, K, runs, payload, totals, 257, True, W, route_caps=caps)
        same(got, restate(sets, K, runs, payload, totals, 257, True, W, route_caps=caps), f"route {k} short of {short}")
        assert [t[2] for t in got[1]] == [int(j == k) for j in range(K)] and got[1][k] == [0, 0, 1, 0]
        for j in range(K):
            if j != k:
                assert got[1][j] == free[1][j] and np.array_equal(got[2][j], free[2][j])
    same(twin(pkg, sets, K, runs, payload, totals, 257, True, W, route_caps=need), free, "capacities that fit exactly")


def test_sets_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_runroute_sets.o (tools/kernel_regs.py): the partition kernel in its two forms and the
    pack copy, no private segment, no spilled register; the router's first object still holds rt_route_kernel alone"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runroute_sets.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object file or no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == ["rt_pack_kernel", "rt_sets_kernel<false>", "rt_sets_kernel<true>"], out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln
        assert int(m.group(1)) <= 128, ln   # 1024 lanes: sixteen waves on a compute unit's four SIMDs, 512 / 4 registers each


def _tool():
    spec = importlib.util.spec_from_file_location("level_scan_for_test", os.path.join(ROOT, "tools", "level_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_level_scan_tool_reads_shared_and_pack_and_refuses_bad_files_before_it_sets_anything_up(tmp_path):
    """no device needed: the route file is checked before the engine is made"""
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}, {"chanCenterFreq": 929200000}]}))
    route = dict(resample="4/5", taps="filter.json")
    twice = [dict(route, name="a", stage="pocsag", channels=[0, 1]), dict(route, name="b", stage="flex", channels=[1])]
    path = str(tmp_path / "routes.json")
    tool = _tool()
    for extra, want in ((dict(shared=True), (True, False)), (dict(shared=True, pack=True), (True, True)), (dict(shared=True, pack=False), (True, False))):
        (tmp_path / "routes.json").write_text(json.dumps(dict(extra, routes=twice)))
        routes, shared, pack = tool.read_routes(path, 2)
        assert (shared, pack) == want and [r["channels"] for r in routes] == [[0, 1], [1]]
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", os.devnull,
            "--gate-out", str(tmp_path / "gated"), "--gate-route", path]
    bad = [(dict(routes=twice), "channel 1 is in two routes"), (dict(routes=twice, shared=False), "channel 1 is in two routes"),
           (dict(routes=twice, pack=True), "channel 1 is in two routes"),
           (dict(routes=[dict(route, name="a", stage="pocsag", channels=[0, 0])], shared=True), "channel 0 is in two routes"),
           (dict(routes=twice, shared=True, pack="yes"), '"pack" must be true or false'), (dict(routes=twice, shared=1), '"shared" must be true or false'),
           (dict(routes=twice + [dict(route, name="c", stage="none", channels=[])], shared=True, pack=True), "route c has no channel")]
    for doc, message in bad:
        (tmp_path / "routes.json").write_text(json.dumps(doc))
        r = subprocess.run(base, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (message, r.stderr[-500:])
    assert not (tmp_path / "gated").exists()


# ---- GPU: the router alone ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("K", ROUTES)
def test_gpu_equals_the_twin(pkg, K):
    """every run count and W of the twin's test through one router per W and form, the counts in an order that makes most calls
    smaller than the one before: runs, totals and packed payloads, and what the accessors say"""
    import torch
    b = pkg.binding
    order = [2500, 1025, 1024, 1023, 65, 64, 63, 1, 0, 2500, 64]
    assert set(order) == set(COUNTS)
    sets = make_sets(K)
    for W in WINDOWS:
        for pack in (False, True):
            router = pkg.RunRouter(None, K, sets=sets, pack=pack, window_samples=W, max_runs=2500, max_windows=12500)
            assert router.capacity() == 2500 and router.route_caps(0) == ((int((sets & 1).sum()) if pack else NCH), 12500, 2500)
            views = [router.device_view(k) for k in range(K)]
            assert all(v[1] is not None for v in views) if pack else all(v[1] is None for v in views)
            assert len({v[1] for v in views}) == K or not pack
            for k in range(K):
                assert np.array_equal(router.route_channels(k), np.flatnonzero((sets >> k) & 1))
            for n in order:
                runs, payload, totals = make_runs(pkg, n, W)
                keep = trr.routed(torch, router, runs, payload, totals)
                want = twin(pkg, sets, K, runs, payload, totals, 2500, pack, W)
                got = ([], [], [] if pack else None)
                for k in range(K):
                    g, nr_elems = router.fetch(k)
                    got[0].append(g)
                    got[1].append([len(g), nr_elems, 0, 0])
                    if pack:
                        got[2].append(router.fetch_payload(k))
                    d_runs, d_payload, d_totals = router.device_view(k)
                    assert (d_runs, d_totals) == views[k][::2] and d_payload == (views[k][1] if pack else keep[1].data_ptr())
                same(got, want, f"K {K} W {W} pack {pack} n {n}")
                del keep
            if pack:
                with pytest.raises(pkg.MfmError) as ei:
                    router.fetch_payload(0, max_elems=0)
                assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == len(want[2][0]) > 0
            else:
                with pytest.raises(pkg.MfmError) as ei:
                    router.fetch_payload(0)
                assert ei.value.code == b.MFM_E_INVAL and "MFM_RUNROUTE_F_PACK" in str(ei.value)
            with pytest.raises(pkg.MfmError) as ei:
                router.route_caps(K)
            assert ei.value.code == b.MFM_E_INVAL
            router.close()


@pytest.mark.gpu
def test_gpu_one_hot_sets_equal_the_route_table_router_and_it_names_its_channels(pkg):
    import torch
    for K in ROUTES:
        sets, route = one_hot(K)
        new, old = pkg.RunRouter(None, K, sets=sets, max_runs=2500), pkg.RunRouter(route, K, max_runs=2500)
        for n in (2500, 1025, 64, 0):
            runs, payload, totals = make_runs(pkg, n, 64)
            keep = trr.routed(torch, new, runs, payload, totals), trr.routed(torch, old, runs, payload, totals)
            for k in range(K):
                assert new.fetch(k)[0].tobytes() == old.fetch(k)[0].tobytes() and new.fetch(k)[1] == old.fetch(k)[1] == int(totals[1])
            del keep
        for k in range(K):
            assert np.array_equal(old.route_channels(k), np.flatnonzero(route == k)) and np.array_equal(new.route_channels(k), np.flatnonzero(route == k))
        assert old.route_caps(0) == new.route_caps(0) == (NCH, 0, 2500)
        new.close()
        old.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [False, True], ids=["zero_copy", "pack"])
def test_gpu_refusals_equal_the_twin(pkg, pack):
    import torch
    b = pkg.binding
    good = make_runs(pkg, 65, 64)
    for what, change, want in PACK_REFUSED if pack else REFUSED:
        runs, payload, totals, cap = refused_case(pkg, change)
        for K in ROUTES:
            sets = make_sets(K)
            router = pkg.RunRouter(None, K, sets=sets, pack=pack, window_samples=64, max_runs=cap, max_windows=5 * 257)
            assert twin(pkg, sets, K, runs, payload, totals, cap, pack, 64)[1] == [want] * K
            keep = trr.routed(torch, router, runs, payload, totals)
            for k in range(K):
                for fetch in [router.fetch] + ([router.fetch_payload] if pack else []):
                    with pytest.raises(pkg.MfmError) as ei:
                        fetch(k)
                    assert ei.value.code == b.MFM_E_STATE and ei.value.needed == 0, what
                    assert ("out of step" if want[3] else "overflowed") in str(ei.value), (what, str(ei.value))
            keep = trr.routed(torch, router, *good)   # the router carries no state: the next call is right
            want_good = twin(pkg, sets, K, *good, cap, pack, 64)
            for k in range(K):
                assert router.fetch(k)[0].tobytes() == want_good[0][k].tobytes()
                assert not pack or np.array_equal(router.fetch_payload(k), want_good[2][k])
            del keep
            router.close()


@pytest.mark.gpu
def test_gpu_a_route_over_its_own_capacity_is_flagged_alone_and_nothing_is_written_past_it(pkg):
    """explicit max_windows / max_runs below what a route of shared channels carries: that route overflows, the others are the
    twin's; the bytes behind the small route's capacity in the shared buffers stay as they were"""
    import torch
    b = pkg.binding
    K, W = 3, 64
    sets = make_sets(K)
    runs, payload, totals = make_runs(pkg, 257, W)
    free = restate(sets, K, runs, payload, totals, 257, True, W)
    need = [(t[0], t[1] // W) for t in free[1]]
    # (a) an explicit max_windows one short of what the busiest route carries; (b) the defaults of a small max_in_samples with
    # three channels in all routes and nine in route 0 alone, and most runs on the three: routes 1 and 2 are short, route 0 is not
    lopsided = np.array([1] * 9 + [7] * 3, np.uint8)
    few = runs[(runs["channel"] >= 9) | (np.arange(len(runs)) % 4 == 0)]
    cases = [(sets, runs, totals, dict(max_runs=257, max_windows=max(c[1] for c in need) - 1, max_in_samples=5 * W * 257), None),
             (lopsided, few, np.array([len(few), int(totals[1]), 0, 0], np.uint64), dict(max_in_samples=40 * W), [0, 1, 1])]
    for sets, runs, totals, limit, flagged in cases:
        router = pkg.RunRouter(None, K, sets=sets, pack=True, window_samples=W, **limit)
        caps = [router.route_caps(k)[:0:-1] for k in range(K)]   # (runs, windows)
        assert len(runs) <= router.capacity()
        want = restate(sets, K, runs, payload, totals, router.capacity(), True, W, route_caps=caps)
        over = [t[2] for t in want[1]]
        assert 0 < sum(over) < K and flagged in (None, over), (limit, caps, need, over)
        same(twin(pkg, sets, K, runs, payload, totals, router.capacity(), True, W, route_caps=caps), want, str(limit))
        keep = trr.routed(torch, router, runs, payload, totals)
        for k in range(K):
            if over[k]:
                with pytest.raises(pkg.MfmError) as ei:
                    router.fetch(k)
                assert ei.value.code == b.MFM_E_STATE and "overflowed" in str(ei.value)
            else:
                assert router.fetch(k)[0].tobytes() == want[0][k].tobytes() and np.array_equal(router.fetch_payload(k), want[2][k])
        del keep
        router.close()


# ---- GPU: sizing and chains ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_a_packed_routes_resampler_is_sized_to_the_route(pkg, ora):
    """3 of 12 channels on a packed route, its burst resampler made from route_caps: it takes a call whose gate payload exceeds
    its own capacity and returns what the unrouted all-channel resampler returns on those channels; the same small resampler behind
    the zero-copy route answers MFM_RUNRS_OVER_OWN"""
    import torch
    b = pkg.binding
    W, cap_in, I, D = 16, 160, 4, 5
    rng = np.random.RandomState(5)
    taps = rng.randint(-8191, 8192, 9).astype(np.int16)
    sets = np.zeros(NCH, np.uint8)
    sets[[2, 5, 11]] = 1
    # every channel open for 3 .. 5 windows, twice: far more payload than three channels' capacity
    runs = np.zeros(2 * NCH, b.GATE_RUN_DTYPE)
    runs["channel"] = np.repeat(np.arange(NCH), 2)
    runs["nr_windows"] = rng.randint(3, 6, 2 * NCH)
    runs["first_window"] = np.tile([10, 20], NCH)
    length = runs["nr_windows"].astype(np.int64) * W
    runs["payload_offset"] = np.cumsum(length + 4) - length
    payload = rng.randint(-32768, 32768, int(runs["payload_offset"][-1] + length[-1])).astype(np.int16)
    totals = np.array([len(runs), payload.size, 0, 0], np.uint64)
    packed = pkg.RunRouter.behind(None, 1, cap_in, W, sets=sets, pack=True)
    zero = pkg.RunRouter.behind(None, 1, cap_in, W, sets=sets)
    caps = packed.route_caps(0)
    assert caps == (3, 3 * (cap_in // W + 1), 3 * ((cap_in // W + 2) // 2)) and zero.route_caps(0) == (NCH, 0, zero.capacity())
    small = [pkg.RunResampler(caps[0], taps, I, D, W, max_in_samples=cap_in, max_windows=caps[1], max_runs=caps[2]) for _ in range(2)]
    whole = pkg.RunResampler(NCH, taps, I, D, W, max_in_samples=cap_in)
    assert payload.size > caps[1] * W   # the gate's payload exceeds the small resampler's cap_elems
    keep = trr.routed(torch, packed, runs, payload, totals), trr.routed(torch, zero, runs, payload, totals)
    small[0].process_device(*packed.device_view(0))
    got_runs, got_payload = small[0].fetch()
    whole.process_device(*(k.data_ptr() for k in keep[1]))
    all_runs, all_payload = whole.fetch()
    mine = np.isin(all_runs["channel"], [2, 5, 11])
    assert len(got_runs) == 6 and np.array_equal(packed.route_channels(0)[got_runs["channel"]], all_runs["channel"][mine])
    trr.same_but(got_runs, all_runs[mine], ("out_offset", "channel"), "the packed route")
    assert int(got_runs["nr_out"].min()) > 0
    for x, y in zip(trr.slices(got_runs, got_payload, False), trr.slices(all_runs[mine], all_payload, False)):
        assert np.array_equal(x, y)
    small[1].process_device(*zero.device_view(0))
    with pytest.raises(pkg.MfmError) as ei:
        small[1].fetch()
    assert ei.value.code == b.MFM_E_STATE and "exceeds max_windows or max_runs" in str(ei.value), str(ei.value)   # MFM_RUNRS_OVER_OWN
    del keep
    for o in small + [whole, packed, zero]:
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [False, True], ids=["zero_copy", "pack"])
def test_gpu_a_shared_channel_feeds_a_pocsag_and_a_flex_chain(pkg, ora, pack):
    """the scene of test_runroute.test_gpu_flex_route_beside_a_pocsag_route with channel 2 in BOTH routes (sets 1, 1, 3, 2): one
    gate (P = 1, the scene's mask) in ragged calls, of which one cuts a stretch, and the flush.  Each chain's runs and events, local
    channels mapped back, equal the single-protocol chain's that reads the gate's own view, on the route's channels"""
    sc, s = trf._chain(pkg, ora), trf.CHAIN
    W, P = s["W"], s["P"]
    n = sc["pcm"].shape[1] // W * W
    pg = trp.scene(pkg, ora, (4, 5, 41), 7)["stream"][:2]
    reps = -(-n // pg.shape[1])
    rows = np.ascontiguousarray(np.concatenate([np.tile(pg, (1, reps))[:, :n], sc["pcm"][:, :n]]))
    mask = np.concatenate([np.tile(np.array([[True] * 5 + [False] * 3]), (2, n // W // 8 + 1))[:, :n // W], sc["mask"][:, :n // W]])
    sets = np.array([1, 1, 3, 2], np.uint8)
    cuts = [n // 5 + 3, 0, n // 3 + 17]
    cuts.append(n - sum(cuts))
    cap = max(cuts)
    gate = pkg.Gate(4, cap, W, preroll_windows=P)
    router = pkg.RunRouter.behind(None, 2, cap, W, preroll_windows=P, sets=sets, pack=pack)
    ptaps = trp.rs_taps(pkg, ora, (4, 5, 41))
    kinds = [("pocsag", ptaps, (4, 5)), ("flex", sc["rtaps"], (16, 25))]
    members = [router.route_channels(k) for k in range(2)]
    assert [m.tolist() for m in members] == [[0, 1, 2], [2, 3]]
    routed, plain = [], []
    for k, (stage, taps, (I, D)) in enumerate(kinds):
        nc, mw, mr = router.route_caps(k)
        assert nc == (len(members[k]) if pack else 4)
        rr = pkg.RunResampler(nc, taps, I, D, W, max_in_samples=cap, preroll_windows=P, max_windows=mw, max_runs=mr)
        routed.append((rr, (pkg.RunPocsag if stage == "pocsag" else pkg.RunFlex).behind(rr)))
        plain.append(trr.Chain(pkg, 4, taps, (I, D), W, cap, P, stage))
    pos, seen, continued, frames, got_by, all_by = 0, [0, 0], 0, 0, {}, {}
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gr, gp = gate.process_host(rows[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W))
            pos += m
        else:
            gate.flush_device()
            gr, gp = gate.fetch()
        router.process_device(*gate.device_view())
        for k in range(2):
            what = f"pack {pack}, call {i}, route {k}"
            rr, st = routed[k]
            rr.process_device(*router.device_view(k))
            st.process_device(*rr.device_view())
            (runs, payload), ev = rr.fetch(), st.fetch()
            (all_runs, all_payload), all_ev = plain[k].call(gate.device_view())
            fw = all_fw = None
            if kinds[k][0] == "flex":
                (ev, fw), (all_ev, all_fw) = ev, all_ev
            runs, ev = runs.copy(), ev.copy()
            if pack:   # local channels back to global ones
                runs["channel"], ev["channel"] = members[k][runs["channel"]], members[k][ev["channel"]]
            keep = np.isin(all_runs["channel"], members[k])
            trr.same_but(runs, all_runs[keep], ("out_offset",), what)
            for x, y in zip(trr.slices(runs, payload, False), trr.slices(all_runs[keep], all_payload, False)):
                assert np.array_equal(x, y), what
            if fw is None:
                trr.same_but(ev, all_ev[np.isin(all_ev["channel"], members[k])], ("run",), what)
            else:   # frame_index counts the call's frames, which the chain of all channels numbers on its own: by stretch, with the words
                assert len(ev) == int(np.isin(all_ev["channel"], members[k]).sum()), what
                trf.per_stretch(ev, fw, got_by)
                trf.per_stretch(all_ev, all_fw, all_by)
                frames += len(fw)
            seen[k] += len(ev)
            continued += int(((runs["flags"] & 1) == 0).sum())
            mine = gr[np.isin(gr["channel"], members[k])]
            assert len(router.fetch(k)[0]) == len(mine) == len(runs), what
    assert pos == n and seen[1] >= 2 and continued >= 1, (seen, continued)   # a stretch continues across a call
    assert frames == 2 and got_by == {key: v for key, v in all_by.items() if key[0] in (2, 3)} and {key[0] for key in got_by} == {2, 3}
    for rr, st in routed:
        st.close()
        rr.close()
    for o in plain + [router, gate]:
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [False, True], ids=["zero_copy", "pack"])
def test_gpu_refused_router_call_keeps_every_routes_chain_state(pkg, ora, pack):
    """as test_runroute's refusal test with channel 1 in both routes: refused calls (the gate's two flags, a channel that does
    not exist, more runs than the router holds) make every route's burst resampler refuse and leave its state where it was: the
    same input through a router that fits is right afterwards, and channel 1's stretch continues"""
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D = 4, 5
    first, second = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    assert len(second[0]) == 3 and [int(c) for c in second[0]["channel"]] == [1, 1, 2]
    sets = np.array([1, 3, 1], np.uint8)
    small = pkg.RunRouter(None, 2, sets=sets, pack=pack, window_samples=W, max_runs=2, max_windows=30)
    fits = pkg.RunRouter.behind(None, 2, 30, W, sets=sets, pack=pack)
    members = [fits.route_channels(k) for k in range(2)]
    rrs = []
    for k in range(2):
        nc, mw, mr = fits.route_caps(k)
        rrs.append(pkg.RunResampler(nc, taps, I, D, W, max_in_samples=30, max_windows=mw, max_runs=mr))
    chk = [tr.Checker(pkg, ora, taps, I, D, False, W) for _ in range(2)]

    def through(router, call, totals=None):
        keep = trr.routed(torch, router, call[0], call[1], totals)
        out = []
        for k in range(2):
            rrs[k].process_device(*router.device_view(k))
            try:
                runs, payload = rrs[k].fetch()
                runs = runs.copy()
                if pack:
                    runs["channel"] = members[k][runs["channel"]]
                out.append((runs, payload))
            except pkg.MfmError as err:
                out.append(err)
        del keep
        return out

    def mine(call, k):
        return call[0][np.isin(call[0]["channel"], members[k])]

    for k, got in enumerate(through(fits, first)):
        tr.same(got, chk[k].call(mine(first, k), first[1]), f"first call, route {k}")
    bad = second[0].copy()
    bad["channel"][2] = nch
    n2 = second[1].size
    for router, call, totals, message in ((small, second, None, "max_open_windows"), (small, second, None, "max_open_windows"),
                                          (fits, second, [3, n2, 1, 0], "max_open_windows"), (fits, second, [3, n2, 0, 1], "out of step"),
                                          (fits, (bad, second[1]), None, "out of step")):
        for k, err in enumerate(through(router, call, totals)):
            assert isinstance(err, pkg.MfmError) and err.code == b.MFM_E_STATE and message in str(err), (message, k, err)
            assert err.needed == (0, 0)
    want = [chk[k].call(mine(second, k), second[1]) for k in range(2)]
    assert [int(f) for f in want[1][0]["flags"]] == [0, 1] and [int(f) for f in want[0][0]["flags"]][:2] == [0, 1]   # channel 1 continues on both
    for k, got in enumerate(through(fits, second)):
        tr.same(got, want[k], f"second call after five refused ones, route {k}")
    for o in rrs + [small, fits]:
        o.close()


# ---- GPU: the tool ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_level_scan_tool_with_a_shared_packed_routes_file_writes_what_the_single_chain_run_writes(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-route routes.json on the chain scene of tests/test_runpocsag.py with "shared" and "pack":
    channel 1 on a pocsag route and channels 0 and 1 on a second pocsag route.  Each route's files hold the lines and bytes of
    the --gate-resample 4/5 --gate-pocsag run that belong to its channels, with true channel numbers"""
    sc, s = trp._chain(pkg, ora), trp.CHAIN
    fs, decim, W, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 929000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))
    route = dict(resample="4/5", taps=str(tmp_path / "filter.json"), stage="pocsag")
    members = {"one": [1], "both": [0, 1]}
    (tmp_path / "routes.json").write_text(json.dumps({"shared": True, "pack": True,
                                                      "routes": [dict(route, name=name, channels=ch) for name, ch in members.items()]}))
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
    some = 0
    for name, ch in members.items():
        for f in ("pocsag.jsonl", "pages.jsonl", "resampled.jsonl"):
            want = [ln for ln in (tmp_path / "single" / f).read_text().splitlines() if json.loads(ln)["channel"] in ch]
            got = (tmp_path / "gated" / name / f).read_text().splitlines()
            assert got == want, (name, f)
            some += len(got)
        for c in range(len(sc["offs"])):
            path = tmp_path / "gated" / name / ("ch%04d.rs.s16" % c)
            assert path.exists() == (c in ch and (tmp_path / "single" / path.name).exists()), (name, c)
            if path.exists():
                assert path.read_bytes() == (tmp_path / "single" / path.name).read_bytes(), (name, c)
    assert some >= 6
    for f in ("index.jsonl", "ch0000.s16", "ch0001.s16"):   # the gate's files, as without the router
        assert (tmp_path / "gated" / f).read_bytes() == (tmp_path / "single" / f).read_bytes(), f
