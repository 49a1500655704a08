"""The burst resampler's view entries (mfm_runrs_process_view_device, mfm_runrs_process_bits_view_device,
csrc/mfm_runrs_view.hip): a resampler sized to one local route of the run router (mfm_runroute_create_local) reads the gate's
payload in place.  A run's payload range is checked against *d_payload_elems, the totals' elements are only the load that must
fit the capacity, and everything else is the rule of the plain entries to the bit.

The checker is never the code under test: a chain behind a local route is compared with the chain behind a packed route
(MFM_RUNROUTE_F_PACK, the plain entries) on the same gate, with the host twins, and the refusals with the oracle's Checker of
tests/test_runrs.py.  Every comparison is an equality."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_runroute as trr
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runrs_process_view_device", "mfm_runrs_process_bits_view_device"]
NCH = 16
SETS = np.array([1, 3] + [0] * 3 + [2] * 11, np.uint8)   # route A = {0, 1}, route B = {1, 5 .. 15}: channel 1 is shared
RATIOS = [(4, 5), (16, 25)]
POLE = 0.999


def _taps(pkg, ora):
    """route A: the 41 taps of the mixed scene at 4/5; route B: 101 taps at 16/25"""
    rng = np.random.RandomState(77)
    return [trr._mixed(pkg, ora)["taps"], rng.randint(-2000, 2001, 101).astype(np.int16)]


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_view_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert callable(pkg.RunResampler.process_view_device) and callable(pkg.RunResampler.process_bits_view_device)
    assert re.search(r"#define MFM_ABI_VERSION 4\b", src)


def test_view_kernel_uses_no_scratch_and_does_not_spill():
    """the code object's notes of build/mfm_runrs_view.o (tools/kernel_regs.py): the one plan kernel, no private segment, no
    spilled register"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_runrs_view.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_runrs_view.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert [ln.split()[0] for ln in lines] == ["rrv_plan_kernel"], out
    m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", lines[0])
    assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), lines[0]


def test_the_runrs_twin_on_local_lists_equals_itself_on_packed_lists_over_a_stream(pkg, ora):
    """mfm_hosttwin_runrs_call is the twin of the view entry: the local route's list with the gate's payload and the gate's total
    as nr_gate_elems, against the same twin on PACK's list with PACK's payload, over a stream of several gate calls (P = 1, the
    flush included): runs but for out_offset's source, payload and state are equal per route, and so is the DC blocker's"""
    b = pkg.binding
    W, P = 16, 1
    rng = np.random.RandomState(9)
    stream = tr.make_stream(rng, NCH, 60 * W, False)
    mask = tr.make_mask("short", rng, NCH, 60, P)
    mask[:, 30:34] = True   # every channel open for a stretch
    cuts = tr.make_cuts(rng, 60 * W, W, False)
    calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
    assert len(calls) >= 8
    taps = _taps(pkg, ora)
    members = [np.flatnonzero((SETS >> k) & 1) for k in range(2)]
    sides = {}
    for side in ("local", "pack"):
        sides[side] = [b.hosttwin_runrs_state(len(members[k]), len(taps[k]), RATIOS[k][0]) + (np.zeros(len(members[k]), b.RUNRS_DC_STATE_DTYPE),)
                       for k in range(2)]
    some, beyond = 0, 0
    for i, (gr, gp) in enumerate(calls):
        totals = np.array([len(gr), gp.size, 0, 0], np.uint64)
        lrows, lt, bound = pkg.hosttwin_runroute_local_call(SETS, 2, gr, totals, W, max_runs=max(len(gr), 1))
        prows, pt, ppay = pkg.hosttwin_runroute_sets_call(SETS, 2, gr, totals, max_runs=max(len(gr), 1), pack=True, window_samples=W, gate_payload=gp)
        assert bound == gp.size and np.array_equal(lt, pt)
        for k in range(2):
            (I, D), what = RATIOS[k], f"call {i}, route {k}"
            ll, pl = lrows[k][:int(lt[k][0])], prows[k][:int(pt[k][0])]
            beyond += int(len(ll) and int(ll["payload_offset"].max()) >= int(lt[k][1]))
            ls, lp, ldc = sides["local"][k]
            ps, pp, pdc = sides["pack"][k]
            got = b.hosttwin_runrs_call(W, taps[k], I, D, ls, lp, ll, gp)
            want = b.hosttwin_runrs_call(W, taps[k], I, D, ps, pp, pl, ppay[k][:int(pt[k][1])])
            tr.same(got, want, what)
            assert np.array_equal(ls, ps) and np.array_equal(lp, pp), what
            got_dc = b.hosttwin_runrs_dc_call(POLE, ldc, got[0], got[1].copy())
            want_dc = b.hosttwin_runrs_dc_call(POLE, pdc, want[0], want[1].copy())
            assert np.array_equal(got_dc, want_dc) and np.array_equal(ldc, pdc), what
            some += got[1].size
    assert some > 1000 and beyond >= 2   # offsets beyond the route's own load: the plain rule would have refused them


# ---- GPU: the chain against PACK, bit for bit ----------------------------------------------------------------------------

CUTS = [0, 5000, 37, 6000, 0, 4500, 63, 7000, 3000, 4400]   # ragged: calls of nothing, calls shorter than W
_SCENE = {}


def _scene(pkg, ora):
    """sixteen PCM rows from the nine of test_runroute's MIXED scene (W = 64, n = 30 000), with every channel loud over samples
    10 000 .. 16 000, so that the squelch of every channel is open for a stretch.  Made once and left unchanged"""
    if not _SCENE:
        sc, s = trr._mixed(pkg, ora), trr.MIXED
        rows = sc["rows"][[c % 9 for c in range(NCH)]].copy()
        rng = np.random.RandomState(5)
        rows[:, 10000:16000] = rng.normal(0, 6000, (NCH, 6000)).round().astype(np.int16)
        assert rows.shape == (NCH, s["n"]) and sum(CUTS) == s["n"] and s["W"] == 64 and min(c for c in CUTS if c) < s["W"]
        _SCENE["it"] = dict(rows=np.ascontiguousarray(rows), thr=sc["thr"])
    return _SCENE["it"]


class Routed:
    """Level -> Gate (pre-roll 1, hang 2) -> a local router and a packed router on the same gate; one call per step"""

    def __init__(self, pkg, ora):
        b, s = pkg.binding, trr.MIXED
        self.pkg, self.sc, self.W, self.P, self.cap = pkg, _scene(pkg, ora), s["W"], s["P"], max(CUTS)
        W, P, cap = self.W, self.P, self.cap
        self.lv = pkg.Level(NCH, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=self.sc["thr"], close_thr=self.sc["thr"], hang_windows=s["hang"])
        self.gate = pkg.Gate(NCH, cap, W, preroll_windows=P)
        self.local = pkg.RunRouter.behind(None, 2, cap, W, preroll_windows=P, sets=SETS, local=True)
        self.pack = pkg.RunRouter.behind(None, 2, cap, W, preroll_windows=P, sets=SETS, pack=True)
        self.caps = [self.local.route_caps(k) for k in range(2)]
        assert self.caps == [self.pack.route_caps(k) for k in range(2)] and [c[0] for c in self.caps] == [2, 12]
        assert [self.local.route_channels(k).tolist() for k in range(2)] == [[0, 1], [1] + list(range(5, 16))]

    def resampler(self, k, taps):
        nc, mw, mr = self.caps[k]
        return self.pkg.RunResampler(nc, taps, RATIOS[k][0], RATIOS[k][1], self.W, max_in_samples=self.cap, preroll_windows=self.P,
                                     max_windows=mw, max_runs=mr)

    def calls(self):
        """per call and the flush: (index, the gate's runs, the gate's payload), both routers run behind the gate"""
        rows, pos = self.sc["rows"], 0
        for i, m in enumerate(CUTS + [None]):
            if m is not None:
                gr, gp = self.gate.process_host(rows[:, pos:pos + m], self.lv.process_host(rows[:, pos:pos + m]))
                pos += m
            else:
                self.gate.flush_device()
                gr, gp = self.gate.fetch()
            view = self.gate.device_view()
            self.local.process_device(*view)
            self.pack.process_device(*view)
            yield i, gr, gp
        assert pos == rows.shape[1]

    def close(self):
        for o in (self.local, self.pack, self.gate, self.lv):
            o.close()


def same_state(got, want, what, valid_only=False):
    """valid_only: the pending samples up to each channel's count only.  What lies behind is whatever an earlier stretch left
    there, and the device, which keeps its state in two buffers used in turn, need not agree with the host twin's one about it"""
    assert len(got) == len(want), what
    if valid_only:
        got, want = list(got), list(want)
        for side in (got, want):
            side[1] = np.where(np.arange(side[1].shape[1])[None, :] < side[0]["pending"][:, None], side[1], 0)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


@pytest.mark.gpu
def test_gpu_a_chain_behind_a_local_route_equals_the_chain_behind_a_packed_route(pkg, ora):
    """route A = {0, 1} at 4/5 with 41 taps and the DC blocker, route B = {1, 5 .. 15} at 16/25, the stream cut raggedly and the
    flush: create_local + the view entry against create_sets(PACK) + the plain entry, both sized by route_caps.  Per call and
    route runs, payload, totals and fetch_state (with the blocker's) are equal, and both equal the host twins.  In at least one
    call the gate's payload exceeds route A's max_windows * W: a view entry that held the gate's total against the capacity
    would refuse it"""
    b = pkg.binding
    rt = Routed(pkg, ora)
    W = rt.W
    taps = _taps(pkg, ora)
    chains = {side: [rt.resampler(k, taps[k]) for k in range(2)] for side in ("local", "pack")}
    twins = []
    for k in range(2):
        for side in chains:
            if k == 0:
                chains[side][k].set_dc_block(POLE)
        twins.append(b.hosttwin_runrs_state(rt.caps[k][0], len(taps[k]), RATIOS[k][0]) + ((np.zeros(rt.caps[k][0], b.RUNRS_DC_STATE_DTYPE),) if k == 0 else ()))
    bound_at = rt.local.bound_view()
    larger, some, continued = 0, [0, 0], 0
    for i, gr, gp in rt.calls():
        totals = np.array([len(gr), gp.size, 0, 0], np.uint64)
        lrows, lt, bound = pkg.hosttwin_runroute_local_call(SETS, 2, gr, totals, W, max_runs=max(len(gr), 1))
        assert bound == gp.size
        larger += int(gp.size > rt.caps[0][1] * W)
        for k in range(2):
            what = f"call {i}, route {k}"
            chains["local"][k].process_view_device(*rt.local.device_view(k), bound_at)
            chains["pack"][k].process_device(*rt.pack.device_view(k))
            lruns, load = rt.local.fetch(k)
            want_list = lrows[k][:int(lt[k][0])]
            assert lruns.tobytes() == want_list.tobytes() and load == int(lt[k][1]) == rt.pack.fetch(k)[1], what
            got, want = chains["local"][k].fetch(), chains["pack"][k].fetch()
            tr.same(got, want, what)   # runs, payload; the totals are their lengths, and a flag would have raised
            same_state(chains["local"][k].fetch_state(), chains["pack"][k].fetch_state(), what)
            tw = twins[k]
            host = b.hosttwin_runrs_call(W, taps[k], RATIOS[k][0], RATIOS[k][1], tw[0], tw[1], want_list, gp)
            if k == 0:
                host = (host[0], b.hosttwin_runrs_dc_call(POLE, tw[2], host[0], host[1].copy()))
            tr.same(got, host, what + ", the host twins")
            same_state(chains["local"][k].fetch_state(), tw, what + ", the host twins' state", valid_only=True)
            some[k] += got[1].size
            continued += int(((got[0]["flags"] & 1) == 0).sum())
    assert larger >= 1, "no call in which the gate's payload elements exceed route A's max_windows * W"
    assert min(some) > 1000 and continued >= 2, (some, continued)
    for side in chains:
        for rr in chains[side]:
            rr.close()
    rt.close()


@pytest.mark.gpu
def test_gpu_the_bits_view_entry_equals_the_bits_entry_behind_a_packed_route(pkg, ora):
    """route A as an AIS route (MFM_BITS_POS), no blocker, through process_bits_view_device against PACK +
    process_bits_device: runs, words, totals and state per call; in one call the local side's object takes PACK's view of the same
    windows through the plain bits entry (view and plain calls alternate on one object), and the stretches go on across it"""
    b = pkg.binding
    rt = Routed(pkg, ora)
    taps = _taps(pkg, ora)[0]
    mine, ref = rt.resampler(0, taps), rt.resampler(0, taps)
    bound_at = rt.local.bound_view()
    words, continued = 0, 0
    for i, gr, gp in rt.calls():
        what = f"call {i}"
        ref.process_bits_device(*rt.pack.device_view(0), b.MFM_BITS_POS)
        want = ref.fetch_bits()
        if i == 5:      # a plain call between view calls, on PACK's view of the same windows
            mine.process_bits_device(*rt.pack.device_view(0), b.MFM_BITS_POS)
        else:
            mine.process_bits_view_device(*rt.local.device_view(0), bound_at, b.MFM_BITS_POS)
        got = mine.fetch_bits()
        tr.same(got, want, what)
        v = mine.bits_view()
        assert v.polarity == b.MFM_BITS_POS
        with pytest.raises(pkg.MfmError) as ei:
            mine.fetch()
        assert ei.value.code == b.MFM_E_STATE and "mfm_runrs_fetch_bits" in str(ei.value)
        same_state(mine.fetch_state(), ref.fetch_state(), what)
        words += got[1].size
        continued += int(((got[0]["flags"] & 1) == 0).sum())
    assert words > 100 and continued >= 1, (words, continued)
    with pytest.raises(pkg.MfmError) as ei:
        mine.process_bits_view_device(*rt.local.device_view(0), bound_at, 3)
    assert ei.value.code == b.MFM_E_INVAL and "polarity" in str(ei.value)
    blocked = rt.resampler(0, taps)
    blocked.set_dc_block(POLE)
    with pytest.raises(pkg.MfmError) as ei:
        blocked.process_bits_view_device(*rt.local.device_view(0), bound_at, b.MFM_BITS_POS)
    assert ei.value.code == b.MFM_E_INVAL and "DC blocker" in str(ei.value)
    for o in (mine, ref, blocked):
        o.close()
    rt.close()


# ---- GPU: refusals ------------------------------------------------------------------------------------------------------

def _viewed(pkg, torch, rr, gr, gp, load, bound, plain=False):
    """one call from uploaded arrays as a local route hands them over: totals[1] is the load, the bound stands apart"""
    t = np.array([len(gr), load, 0, 0], np.uint64)
    keep = (tr._up(torch, gr), tr._up(torch, gp), tr._up(torch, t), tr._up(torch, np.array([bound], np.uint64)))
    if plain:
        rr.process_device(*(k.data_ptr() for k in keep[:3]))
    else:
        rr.process_view_device(*(k.data_ptr() for k in keep))
    try:
        return rr.fetch()   # waits for the queued work, refused or not, before the uploads go
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_view_entry_refusals_leave_the_state_and_a_call_that_fits_is_right(pkg, ora):
    """the small case of tests/test_runrs.py (W = 5, three channels, the second gate call holds channel 1's windows 2 and 4 - 5 at
    payload offsets 0 and 5 and channel 2's window 3 at offset 15), a resampler of three windows: a range that ends one element
    beyond *d_payload_elems is MFM_RUNRS_GATE_BAD_RUNS, a load of four windows MFM_RUNRS_OVER_OWN, a run longer than the capacity
    MFM_RUNRS_GATE_BAD_RUNS, and the local view of channel 2 (offset 15 beyond its load of 5) is refused by the plain entry and
    right through the view entry.  Nothing comes out of a refused call and the state stays"""
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D = 4, 5
    first, second = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    gr, gp = second
    assert [int(c) for c in gr["channel"]] == [1, 1, 2] and [int(o) for o in gr["payload_offset"]] == [0, 5, 15] and gp.size == 20
    rr = pkg.RunResampler(nch, taps, I, D, W, max_windows=3, max_runs=3)
    chk = tr.Checker(pkg, ora, taps, I, D, False, W)
    tr.same(_viewed(pkg, torch, rr, *first, load=first[1].size, bound=first[1].size), chk.call(*first), "first call")
    s0 = rr.fetch_state()
    one, two = gr[:2], gr[2:]
    long = one.copy()
    long["nr_windows"][1] = 4   # 20 elements: within the bound from offset 0, but no run of a load that fits three windows
    long["payload_offset"][1] = 0
    refusals = [("a range one element beyond the bound", dict(gr=one, load=15, bound=14), "not a gate's"),
                ("a range that begins beyond the bound", dict(gr=two, load=5, bound=14), "not a gate's"),
                ("a load one window beyond the capacity", dict(gr=gr, load=20, bound=20), "exceeds max_windows or max_runs"),
                ("a run longer than the capacity", dict(gr=long, load=15, bound=20), "not a gate's"),
                ("the local view of channel 2 through the plain entry", dict(gr=two, load=5, bound=20, plain=True), "not a gate's")]
    for what, kw, message in refusals + refusals[:1]:   # an odd count: both state buffers take a refused call
        with pytest.raises(pkg.MfmError) as ei:
            _viewed(pkg, torch, rr, kw["gr"], gp, kw["load"], kw["bound"], plain=kw.get("plain", False))
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (what, str(ei.value))
        assert ei.value.needed == (0, 0) and not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any(), what
        same_state(rr.fetch_state(), s0, what)
    want = chk.call(one, gp)
    assert [int(f) for f in want[0]["flags"]] == [0, 1] and int(want[0]["nr_out"][0]) > 0   # channel 1 goes on where the first call left it
    tr.same(_viewed(pkg, torch, rr, one, gp, load=15, bound=20), want, "channel 1's local view")
    tr.same(_viewed(pkg, torch, rr, two, gp, load=5, bound=20), chk.call(two, gp), "channel 2's local view")
    tr.same(_viewed(pkg, torch, rr, one, gp, load=15, bound=20, plain=True), chk.call(one, gp), "a view that lies within its load through the plain entry")
    chk.stretches()
    rr.close()
