"""The burst stages at the shapes they were written for: run counts at which the single-block scans change shape, thousands of
runs in one call, and idle runs long enough for the walkers' summary skip (csrc/mfm_runrs.hip, mfm_runais.hip,
mfm_runpocsag.hip, mfm_runflex.hip).

The expected result is the oracle's, never the code under test: the Checker classes of test_runrs.py, test_runais.py,
test_runpocsag.py and test_runflex.py (the oracle resampler per stretch, a fresh oracle decoder per stretch) on gate run lists
that are assembled by hand or restated from a mask.  Every comparison is the `same()` of those files: equality of every field
of every event and of all 4 x 88 words of every frame.  Each scene asserts its guards - run counts, the run indices of the
events, the lengths of the idle spans, how many summary steps a walker has to take - on the oracle's figures when it is built,
so both the host twin's test (no GPU) and the device's test run on a scene that is known to reach the path it is meant for."""
import os
import re

import numpy as np
import pytest

import test_ais as ta
import test_gate as tg
import test_level as tl
import test_pocsag as tp
import test_runais as tra
import test_runflex as trf
import test_runpocsag as trp
import test_runrs as tr

ROOT = tg.ROOT
MOD = {"runrs": tr, "runais": tra, "runpocsag": trp, "runflex": trf}
STAGES = ["runrs", "runais", "runpocsag", "runflex"]
COUNTS = [1024, 1025, 2049]
SCAN_THREADS = 1024     # MFM_RUN_SCAN_THREADS of csrc/mfm_run_stage.h: per = ceil(n / 1024) runs per thread
FRAME, BAD_BAUD = trf.FRAME, trf.BAD_BAUD
FIGURES = {}            # scene -> the figures its guards saw, for a report


def _define(header, name):
    src = open(os.path.join(ROOT, "tsl-sdr_amd", "csrc", header)).read()
    m = re.search(r"#define\s+%s\s+(\d+)u\b" % name, src)
    assert m, name
    return int(m.group(1))


FHW = _define("mfm_runflex.h", "MFM_RUNFLEX_HIST_WORDS")        # history words in front of a run's segment
FDEAD = _define("mfm_runflex.h", "MFM_RUNFLEX_DEAD")            # a search opens at reset + 311 - 1
PHW = _define("mfm_runpocsag.h", "MFM_RUNPOCSAG_HIST_WORDS")
STEP_WORDS = 64 * 32                                            # a summary step: 64 lanes x 32 segment words of 32 samples


def _taps(ora):
    return ora.quantize_taps([0.1, 0.4, 0.4, 0.1])


def _want(pkg, ora, stage, taps, W, calls):
    """the checker and [(the resampler's result, the stage's result)] per gate call, from the oracle; the burst resampler
    itself has no second part"""
    if stage == "runrs":
        chk = tr.Checker(pkg, ora, taps, 1, 1, False, W)
        return chk, [(chk.call(gr, gp), None) for gr, gp in calls]
    chk = MOD[stage].Checker(pkg, ora, taps, 1, 1, W)
    return chk, [chk.call(gr, gp) for gr, gp in calls]


def _same(stage, got, want, what):
    if stage == "runrs":
        tr.same(got, want[0], what)
    else:
        MOD[stage].same(got, want[1], what)


def _events(stage, ev_want):
    return ev_want[0] if stage == "runflex" else ev_want


def _twin(pkg, stage, nch, taps, W):
    """call(gate call, the oracle's resampler result) -> what the host twin returns; and the state it keeps"""
    b = pkg.binding
    if stage == "runrs":
        state, pending = b.hosttwin_runrs_state(nch, len(taps), 1)
        return (lambda g, rs: b.hosttwin_runrs_call(W, taps, 1, 1, state, pending, *g)), (state, pending)
    state = getattr(b, f"hosttwin_{stage}_state")(nch)
    fn = getattr(b, f"hosttwin_{stage}_call")
    return (lambda g, rs: fn(state, *rs)), state


def _device(pkg, torch, stage, nch, taps, W, max_runs, max_in, max_out):
    """a stage object fed from uploaded arrays: call(gate call, the oracle's resampler result) -> what it fetches"""
    if stage == "runrs":
        rr = pkg.RunResampler(nch, taps, 1, 1, W, max_windows=max_in // W, max_runs=max_runs)
        return rr, lambda g, rs: tr._fed(pkg, torch, rr, *g)
    o = {"runais": pkg.RunAis, "runpocsag": pkg.RunPocsag, "runflex": pkg.RunFlex}[stage](nch, max_runs, max_out)
    return o, lambda g, rs: MOD[stage]._fed(pkg, torch, o, *rs)


def _state_is_the_twins(stage, o, twin_state):
    if stage == "runpocsag":
        state = o.fetch_state()
        assert state.tobytes() == twin_state.tobytes(), [f for f in state.dtype.names if not np.array_equal(state[f], twin_state[f])]
    if stage == "runflex":
        state, ring = o.fetch_state()
        assert state.tobytes() == twin_state[0].tobytes(), [f for f in state.dtype.names if not np.array_equal(state[f], twin_state[0][f])]
        assert np.array_equal(ring, twin_state[1])


def _views_match(pkg, stage, o, got, nr_runs):
    """device_view of the burst POCSAG and FLEX stages: the totals and the bytes of what fetch returned"""
    if stage == "runpocsag":
        d_ev, d_tot = o.device_view()
        assert tl._d2h(d_tot, 32).view(np.uint64).tolist() == [len(got), nr_runs, 0, 0]
        if len(got):
            assert tl._d2h(d_ev, got.nbytes).tobytes() == got.tobytes()
    if stage == "runflex":
        ev, fw = got
        d_ev, d_fw, d_tot = o.device_view()
        assert tl._d2h(d_tot, 32).view(np.uint64).tolist() == [len(ev), len(fw), 0, 0]
        if len(ev):
            assert tl._d2h(d_ev, ev.nbytes).tobytes() == ev.tobytes()
        if len(fw):
            assert tl._d2h(d_fw, fw.nbytes).tobytes() == fw.tobytes()


# ---- 1. the run counts at which the scans' partition changes shape ---------------------------------------------------------

_BOUNDARY = {}


def long_indices(n):
    """the runs that carry a transmission: the first, around a thread boundary in the middle of the list (the last run of a scan
    thread, the first of the next, the one behind), runs 1023 and 1024, and the last.  per = ceil(n / 1024) runs per thread"""
    per = (n + SCAN_THREADS - 1) // SCAN_THREADS
    mid = 512 // per * per
    return sorted(i for i in {0, mid - 1, mid, mid + 1, 1023, 1024, n - 1} if 0 <= i < n)


def _long_parts(pkg, stage, k, last, rng):
    """what the k-th long run holds in the first call and how its stretch goes on in the second"""
    sy = pkg.synth
    if stage == "runrs":   # more than 1024 outputs: several FIR workgroups
        return rng.randint(-32768, 32768, 3001 + 2 * k).astype(np.int16), rng.randint(-32768, 32768, 501).astype(np.int16)
    if stage == "runais":
        pl = ta._payloads(sy)
        one = lambda i, seed: sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(pl[i % 3])], lead_bits=5, trail_bits=4), noise=200, lead=61 + k,
                                         trail=201, phase=k % 5, seed=seed)
        return one(k, k), one(k + 1, 50 + k)
    if stage == "runpocsag":
        msgs = tp._messages(sy)
        one = lambda i, seed, lead: sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches([msgs[i % 2]]), preamble_bits=160), 2400, noise=300,
                                                  lead=lead, trail=701, seed=seed)
        return one(k, k, 101 + k), one(k + 1, 50 + k, 300)
    bad_a = sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)[:400]
    if k == 0 or last:     # a whole frame on the first and the last long run, BAD_BAUD on the others
        first = sy.flex_pcm(trf._frames(sy, 3 if last else 0, 1), lead=401 + k, trail=701, noise=300, seed=k)
    else:
        first = sy.flex_pcm([bad_a], lead=351 + 7 * k, trail=400, noise=300, seed=k)
    return first, sy.flex_pcm([bad_a], lead=200, trail=501, noise=300, seed=50 + k)


def boundary_scene(pkg, ora, stage, n):
    """n runs in one call, one channel each, W = 1 so that a gate run is as long as its samples: tiny runs of odd length and
    the long ones of long_indices(n); then a call in which only the long channels go on.  Made once and left unchanged"""
    if (stage, n) in _BOUNDARY:
        return _BOUNDARY[(stage, n)]
    b = pkg.binding
    rng = np.random.RandomState(1000 * STAGES.index(stage) + n)
    taps = _taps(ora)
    long = long_indices(n)
    lens = 2 * rng.randint(17, 45, n) + 1   # 35 .. 89 samples: 31 .. 85 outputs behind the four taps
    g0, p0, g1, p1, off0, off1 = [], [], [], [], 0, 0
    for c in range(n):
        fw = 5 + c % 3
        if c in long:
            x, y = _long_parts(pkg, stage, long.index(c), c == long[-1], rng)
            g1.append((fw + x.size, off1, c, y.size))
            p1.append(y)
            off1 += y.size
        else:
            x = rng.randint(-300, 301, lens[c]).astype(np.int16)
        g0.append((fw, off0, c, x.size))
        p0.append(x)
        off0 += x.size
    calls = [(np.array(g0, b.GATE_RUN_DTYPE), np.concatenate(p0)), (np.array(g1, b.GATE_RUN_DTYPE), np.concatenate(p1))]
    chk, want = _want(pkg, ora, stage, taps, 1, calls)
    # the guards, on the oracle's figures alone
    (runs0, _), ev0 = want[0]
    (runs1, _), ev1 = want[1]
    tiny = np.array([c not in long for c in range(n)])
    assert len(runs0) == n and runs0["channel"].tolist() == list(range(n)) and (runs0["flags"] == 1).all()
    assert (runs0["nr_out"][tiny] % 2 == 1).all() and 30 <= runs0["nr_out"][tiny].min() and runs0["nr_out"][tiny].max() <= 90
    assert len(set((runs0["out_offset"] % 32).tolist())) == 32   # segment bases and payload offsets on every residue
    assert len(runs1) == len(long) >= 5 and int((runs1["flags"] == 0).sum()) >= 4 and runs1["channel"].tolist() == long
    fig = dict(runs=[len(runs0), len(runs1)], long=long, continued=int((runs1["flags"] == 0).sum()))
    if stage == "runrs":
        assert (runs0["nr_out"][long] > 2 * 1024).all()
    else:
        e0, e1 = _events(stage, ev0), _events(stage, ev1)
        assert all((e0["run"] == r).any() for r in long), [int((e0["run"] == r).sum()) for r in long]
        assert len(e1) >= 4
        fig.update(events=[len(e0), len(e1)], runs_with_events=len(set(e0["run"].tolist())), highest_run=int(e0["run"].max()))
    if stage == "runflex":   # both frames, and an event that is no frame in a run between them
        fr = e0[e0["type"] == FRAME]
        assert len(ev0[1]) == 2 and fr["run"].tolist() == [long[0], long[-1]] and fr["frame_index"].tolist() == [0, 1]
        assert ((e0["type"] != FRAME) & (e0["run"] > long[0]) & (e0["run"] < long[-1])).any()
        fig.update(frames=[len(ev0[1]), len(ev1[1])])
    FIGURES[f"boundary {stage} {n}"] = fig
    _BOUNDARY[(stage, n)] = dict(calls=calls, want=want, taps=taps, long=long)
    return _BOUNDARY[(stage, n)]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("stage", STAGES)
def test_hosttwin_boundary_run_counts(pkg, ora, stage, n):
    """the scene's guards and the host twin: 1024, 1025 and 2049 runs in one call, then the long channels alone"""
    sc = boundary_scene(pkg, ora, stage, n)
    call, _ = _twin(pkg, stage, n, sc["taps"], 1)
    for i, (g, w) in enumerate(zip(sc["calls"], sc["want"])):
        _same(stage, call(g, w[0]), w, f"{stage}, {n} runs, call {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("stage", STAGES)
def test_gpu_boundary_run_counts(pkg, ora, stage, n):
    """1024 runs fill every scan thread with one run; at 1025 a thread owns two and threads 513 and up are empty; at 2049 a
    thread owns three and the last busy one ends exactly at n.  Long runs with events sit on the thread boundaries, at runs 1023
    and 1024 and at the end, between tiny runs of odd length; the second call continues the long channels' stretches only, so
    it reads the state of channels whose last run sat on a boundary and leaves the others' alone"""
    import torch
    sc = boundary_scene(pkg, ora, stage, n)
    taps = sc["taps"]
    max_in = max(gp.size for _, gp in sc["calls"]) + 1
    o, call = _device(pkg, torch, stage, n, taps, 1, n, max_in, max_in)
    twin, twin_state = _twin(pkg, stage, n, taps, 1)
    for i, (g, w) in enumerate(zip(sc["calls"], sc["want"])):
        got = call(g, w[0])
        _same(stage, got, w, f"{stage}, {n} runs, call {i}")
        _views_match(pkg, stage, o, got, len(w[0][0]))
        twin(g, w[0])
    _state_is_the_twins(stage, o, twin_state)
    o.close()


# ---- 2. thousands of runs in one call, events scattered over hundreds of them ----------------------------------------------

_MANY = {}
MANY = {"runpocsag": dict(nch=64, nw=1500, cut=800, open=40, period=43), "runflex": dict(nch=128, nw=540, cut=300, open=30, period=32)}
GROUP3 = (3, 5, 9, 11)   # channels c with c % 16 in GROUP3: mid-length runs over a repeating damaged transmission


def _many_stream(pkg, ora, stage, nch, n):
    """every 16th channel busy (all three POCSAG rates back to back / one FLEX frame, the four codings in turn), GROUP3 a short
    transmission that never completes over and over, low noise on the rest"""
    sy = pkg.synth
    rng = np.random.RandomState(21 + len(stage))
    stream = rng.randint(-300, 301, size=(nch, n)).astype(np.int16)
    for c in range(nch):
        if c % 16 == 0 and stage == "runpocsag":
            msgs = tp._messages(sy)
            at = 600 + 37 * (c // 16)
            for k in range(3):
                baud = (512, 1200, 2400)[(k + c // 16) % 3]
                p = sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches([msgs[(k + c) % 2]]), preamble_bits=160), baud, noise=300, seed=10 * c + k)
                assert at + p.size + 2500 <= n, (c, k, at, p.size, n)
                stream[c, at:at + p.size] = p
                at += p.size + 2900
        elif c % 16 == 0:
            # 40 samples of one level in front, so that the noise there cannot open the BS1 run a bit period early
            p = sy.flex_pcm([[(3, 40)] + trf._frames(sy, (c // 16) % 4, 1, first=c // 16)[0]], noise=300, seed=c)
            at = 400 + 37 * (c // 16)
            assert at + p.size + 400 <= n, (c, at, p.size, n)
            stream[c, at:at + p.size] = p
        elif c % 16 in GROUP3 and stage == "runpocsag":
            # 96 bits of preamble, the sync word and 40 bits of a batch: a SYNC_FOUND whose batch never completes
            bits = sy.pocsag_bits(sy.pocsag_batches([tp._messages(sy)[c % 2]]), preamble_bits=96)[:96 + 32 + 40]
            unit = sy.pocsag_pcm(bits, 2400, noise=300, trail=400, seed=c)
            stream[c] = np.roll(np.tile(unit, n // unit.size + 2), 53 * c)[:n]
        elif c % 16 in GROUP3:
            # sync 1 with a damaged A word and nothing behind it: BAD_BAUD
            bad_a = sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)[:112]
            unit = sy.flex_pcm([bad_a], trail=200, noise=300, seed=c)
            stream[c] = np.roll(np.tile(unit, n // unit.size + 2), 53 * c)[:n]
    return np.ascontiguousarray(stream)


def many_scene(pkg, ora, stage):
    """W = 64, 1/1, two calls.  Most channels open every fourth window (every run a stretch of its own), every 16th is open
    throughout and busy, GROUP3 has `open` windows open and the rest of `period` closed.  Made once and left unchanged"""
    if stage in _MANY:
        return _MANY[stage]
    W, s = 64, MANY[stage]
    nch, nw = s["nch"], s["nw"]
    taps = _taps(ora)
    stream = _many_stream(pkg, ora, stage, nch, nw * W)
    k, c = np.arange(nw)[None, :], np.arange(nch)[:, None]
    mask = (k + c) % 4 == 0
    third = np.isin(c % 16, GROUP3)
    mask = np.where(third, (k + 7 * c) % s["period"] < s["open"], mask)
    mask = np.where(c % 16 == 0, True, mask)
    cuts = [s["cut"] * W, (nw - s["cut"]) * W]
    calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
    chk, want = _want(pkg, ora, stage, taps, W, calls)
    by = chk.stretches()   # the oracle agrees with itself however the stretches were cut
    assert sorted(by) == tr.stretches_of_mask(mask)
    # the guards, on the oracle's figures alone
    fig = dict(runs=[], runs_with_events=[], highest_run=[], events=[], frames=[], frame_runs=[], seg_words_max=[], continued=[])
    for (runs, _), ev_want in want:
        ev = _events(stage, ev_want)
        fig["runs"].append(len(runs))
        fig["events"].append(len(ev))
        fig["runs_with_events"].append(len(set(ev["run"].tolist())))
        fig["highest_run"].append(int(ev["run"].max()) if len(ev) else -1)
        fig["seg_words_max"].append(int(runs["nr_out"].max()) // 32)
        ch = runs["channel"]
        first = np.concatenate([[True], ch[1:] != ch[:-1]])
        several = np.isin(ch, ch[~first])
        fig["continued"].append(int((first & several & (runs["flags"] == 0)).sum()))   # goes on from the last call, more runs behind
        if stage == "runflex":
            fr = ev[ev["type"] == FRAME]
            fig["frames"].append(len(ev_want[1]))
            fig["frame_runs"].append(len(set(fr["run"].tolist())))
    assert min(fig["runs"]) > 4096, fig
    assert max(fig["runs_with_events"]) >= 100 and max(fig["highest_run"]) >= 2048, fig
    assert chk.multi >= 1 and fig["continued"][1] >= 1, fig
    assert max(fig["seg_words_max"]) > 256, fig   # several slicer workgroups share a run, next to runs of one partly filled workgroup
    ev_all = np.concatenate([_events(stage, w[1]) for w in want])
    if stage == "runflex":
        assert max(fig["frame_runs"]) >= 8 and set(ev_all["coding"][ev_all["type"] == FRAME].tolist()) == {0, 1, 2, 3}, fig
        t = _events(stage, want[int(np.argmax(fig["frame_runs"]))][1])["type"]
        kinds = (t == FRAME).astype(int)
        assert int((np.diff(kinds) != 0).sum()) >= 8   # FRAME and other events take turns in run order
    else:
        batches = ev_all[ev_all["type"] == ora.EV_BATCH]
        assert set(batches["baud"].tolist()) == {512, 1200, 2400} and len(batches) >= 3 * (nch // 16), (len(batches), fig)
    FIGURES[f"many runs {stage}"] = fig
    _MANY[stage] = dict(calls=calls, want=want, taps=taps, W=W, nch=nch, cuts=cuts, by=by)
    return _MANY[stage]


def _cut_independent(stage, got, by):
    """per stretch the events (and words) the calls returned are those of the stretch fed to a fresh oracle decoder in one piece"""
    if stage == "runflex":
        got_by, want_by = {}, {}
        for ev, fw in got:
            trf.per_stretch(ev, fw, got_by)
        for e, fw in by.values():
            trf.per_stretch(e, fw, want_by)
        assert got_by == want_by
        return
    got_by = {}
    for ev in got:
        for e in ev:
            got_by.setdefault((int(e["channel"]), int(e["stretch_window"])), []).append(e)
    for k, v in by.items():
        g = got_by.get(k, [])
        assert len(g) == len(v), k
        for a, b in zip(g, v):
            assert all(np.array_equal(a[f], b[f]) for f in trp.EVENT_FIELDS if f != "run"), k


@pytest.mark.parametrize("stage", ["runpocsag", "runflex"])
def test_hosttwin_many_runs_and_many_workgroups(pkg, ora, stage):
    """the scene's guards and the host twin on it"""
    sc = many_scene(pkg, ora, stage)
    call, _ = _twin(pkg, stage, sc["nch"], sc["taps"], sc["W"])
    got = []
    for i, (g, w) in enumerate(zip(sc["calls"], sc["want"])):
        got.append(call(g, w[0]))
        _same(stage, got[-1], w, f"{stage}, call {i}")
    _cut_independent(stage, got, sc["by"])


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["runpocsag", "runflex"])
def test_gpu_many_runs_and_many_workgroups(pkg, ora, stage):
    """a real RunResampler fed from uploaded gate calls and the stage behind it on its device view, two calls of more than 4096
    runs: the scans' threads own five runs and more, events lie in hundreds of runs with indices far beyond 1024 (most runs
    have none), slice and match kernels find their run among thousands, a busy run takes several slicer workgroups; the
    device_view totals and bytes, and the twin's state (and ring) after the last call"""
    import torch
    sc = many_scene(pkg, ora, stage)
    nch, W, taps = sc["nch"], sc["W"], sc["taps"]
    rr = pkg.RunResampler(nch, taps, 1, 1, W, max_in_samples=max(sc["cuts"]))
    o = {"runpocsag": pkg.RunPocsag, "runflex": pkg.RunFlex}[stage].behind(rr)
    twin, twin_state = _twin(pkg, stage, nch, taps, W)
    got = []
    for i, ((gr, gp), w) in enumerate(zip(sc["calls"], sc["want"])):
        t = np.array([len(gr), gp.size, 0, 0], np.uint64)
        keep = (tr._up(torch, gr), tr._up(torch, gp), tr._up(torch, t))
        rr.process_device(*(k.data_ptr() for k in keep))
        o.process_device(*rr.device_view())
        got.append(o.fetch())
        del keep
        _same(stage, got[-1], w, f"{stage}, call {i}")
        _views_match(pkg, stage, o, got[-1], len(w[0][0]))
        tr.same(rr.fetch(), w[0], f"the resampler's call {i}")
        twin((gr, gp), w[0])
    _cut_independent(stage, got, sc["by"])
    _state_is_the_twins(stage, o, twin_state)
    o.close()
    rr.close()


# ---- 3. idle runs long enough for the summary skip ---------------------------------------------------------------------------
#
# Both walkers step over idle samples through the summary, one bit per segment word, 64 lanes x 32 bits at a time.  Where a
# step ends follows from the segment layout alone (HIST_WORDS words of history in front of a run's first output), so the
# functions below restate it from the headers' constants and every placement is derived from them.

def flex_step_ends(F, p, count):
    """rf_walk_kernel: a search at stretch sample p of a run whose first output is F looks at the rest of p's segment word
    i = HIST_WORDS + (p - F) / 32, then at the summary words (i + 1) / 32 .. + 63, whose bits stand for the segment words up to
    ((i + 1) / 32 + 64) * 32 - 1.  The next search starts at that bound's first sample.  Returns `count` such bounds in a row"""
    out = []
    for _ in range(count):
        sj = (FHW + ((p - F) >> 5) + 1) >> 5
        p = F + 32 * ((sj << 5) + STEP_WORDS - FHW)
        out.append(p)
    return out


def pocsag_step_ends(F, pos, count, rst=0):
    """rp_walk_kernel: a search at pos first takes steps of 64 words from the word pos lies in (segment bit 0 is stretch sample
    F - 32 * HIST_WORDS), until it is 31 * 75 samples behind a reset at rst > 0; then, with no run of matches pending, it reads
    the summary words (word of pos) / 32 .. + 63 and, with no bit set, goes on at the first sample of segment word
    ((word of pos) / 32 + 64) * 32.  Returns `count` such bounds in a row"""
    ws = F - 32 * PHW
    while True:
        pos = ws + 32 * ((pos - ws) >> 5) + 32 * 64
        if not (rst > 0 and pos < rst + 31 * 75):
            break
    out = []
    for _ in range(count):
        sw0 = ((pos - ws) >> 5) >> 5
        pos = ws + 32 * ((sw0 << 5) + STEP_WORDS)
        out.append(pos)
    return out


def flex_m(y):
    """the FLEX matcher restated (pager_flex.c's BS1 test): a register of the sign bits 10 samples apart, zero-filled before
    the stretch, reads 0xaaaaaaaa - bit k, k = 0 the newest, is set for odd k"""
    bit = y >= 0
    m = np.ones(y.size, bool)
    for k in range(32):
        v = np.zeros(y.size, bool)
        v[10 * k:] = bit[:y.size - 10 * k]
        m &= v if k & 1 else ~v
    return m


def pocsag_m(y, spb):
    """the POCSAG matcher restated (pager_pocsag.c's eye detector): a register of the bits (sample < 0) spb samples apart,
    zero-filled before the stretch, differs from the sync word in four bits at most; bit j is j * spb samples back"""
    bit = y < 0
    wrong = np.zeros(y.size, np.int32)
    for j in range(32):
        v = np.zeros(y.size, bool)
        v[j * spb:] = bit[:y.size - j * spb]
        wrong += v != bool((tp.SYNC >> j) & 1)
    return wrong <= 4


def pocsag_pairs(y):
    """samples at which two matches of one rate next to each other begin"""
    x = np.concatenate([y, np.ones(1, np.int16)])
    hit = np.zeros(y.size, bool)
    for spb in (75, 32, 16):
        m = pocsag_m(x, spb)
        hit |= m[:-1] & m[1:]
    return hit


def pocsag_flagged(y, F, n):
    """the first sample of every segment word of the run [F, F + n) that has its summary bit set, as rp_match_kernel states the
    bit: two matches next to each other of one rate that begin in the word; and, because the next word's first sample is not
    looked at across a wave of 64 words, a match in the last sample of a word whose index is 63 mod 64.  The bits behind the
    run's end are the padding's zeros"""
    x = np.concatenate([y[:F + n], np.ones(64, np.int16)])
    o = np.arange(n)
    last = ((o & 31) == 31) & (((PHW + (o >> 5)) & 63) == 63)
    hit = np.zeros(n, bool)
    for spb in (75, 32, 16):
        m = pocsag_m(x, spb)
        hit |= m[F:F + n] & (m[F + 1:F + n + 1] | last)
    return sorted(set((F + 32 * (np.flatnonzero(hit) >> 5)).tolist()))


_IDLE = {}
IDLE_W = 64


def _searches(ora, stage, y):
    """the oracle's events of a stretch and the samples at which a search opens: the stretch's first (a fresh FLEX decoder
    cannot match before sample 310) and the one behind every event that resets the decoder"""
    if stage == "runflex":
        ev = ora.Flex().feed(y)[0]
        return ev, [FDEAD - 1] + [int(s) + FDEAD for s in ev["sample"]]
    ev = tp._dedupe(ora.Pocsag().feed(y)[0], ora)
    return ev, [0] + [int(e["sample"]) + 1 for e in ev if int(e["type"]) == ora.EV_SYNC_LOST]


def _first_hit(stage, y, p):
    """the first sample at or behind p the matcher fires on (FLEX), or at which two matches in a row begin (POCSAG)"""
    hit = flex_m(y) if stage == "runflex" else pocsag_pairs(y)
    hit[:p] = False
    at = np.flatnonzero(hit)
    return int(at[0]) if at.size else None


def _idle_channel(pkg, ora, stage, taps, n, seed, targets, kinds=None):
    """low noise (+-300) and one transmission per target, each moved until the first hit of the search in front of it is the
    target, to the sample: FRAME or BAD_BAUD (FLEX), a short 2400 baud burst of one batch (POCSAG)"""
    sy = pkg.synth
    x = np.random.RandomState(seed).randint(-300, 301, n).astype(np.int16)
    for i, target in enumerate(targets):
        if stage == "runflex":
            bad_a = sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)[:400]
            fr = bad_a if kinds and kinds[i] == BAD_BAUD else trf._frames(sy, (seed + i) % 4, 1)[0]
            # 40 samples of one level in front: whatever the fill holds there, no register reads BS1 a bit period early
            p = sy.flex_pcm([[(3, 40)] + fr], noise=300, seed=seed + i)
        else:
            p = sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches([tp._messages(sy)[(seed + i) % 2]]), preamble_bits=160), 2400, noise=300,
                              seed=seed + i)
        at, got = target - 300, None
        for _ in range(5):
            assert 0 <= at and at + p.size <= n, (stage, target, at, p.size, n)
            z = x.copy()
            z[at:at + p.size] = p
            y = ora.Resampler(taps, 1, 1).feed(z)
            got = _first_hit(stage, y, _searches(ora, stage, y)[1][i])
            if got == target:
                break
            at += target - got
        assert got == target, (stage, seed, target, got)
        x = z
    return x


def idle_scene(pkg, ora, stage, name):
    """two channels, all open, W = 64, 1/1.  Returns the gate calls, the oracle's results and the figures of the guards.
    The cases, by the number of whole summary steps the walker takes before the transmission's first match (F = 0):
      near_far:  channel 0 (a) none; channel 1 (d) none either, the match in the LAST segment word the first step's summary covers:
                 the last bit of the last lane's summary word, one word short of a whole step
      one_none:  channel 0 (b) one, the match well inside the second step; channel 1 (g) nothing at all, the run ends inside
                 the second step, so the clamp to the run's end follows a real step
      edges:     channel 0 (e) one, the match in the FIRST segment word behind the step (the word the next search begins in);
                 channel 1 the same in the second word behind it (the first bit the next step's summary is asked for)
      two_after: channel 0 (c) two steps; channel 1 (f) a transmission, its event, one whole step from the state that event
                 left, and a second transmission
      two_after_cut: the same stream in two calls, the boundary inside the idle spans: the second call's runs continue their
                 stretches idle, with the history from the carried tail (POCSAG) or the ring (FLEX)
    A FLEX target is the sample of the first match, 8 samples into its segment word; a POCSAG target the sample at which the
    first two matches in a row begin, 12 samples into its word"""
    if (stage, name) in _IDLE:
        return _IDLE[(stage, name)]
    W, taps = IDLE_W, _taps(ora)
    flex = stage == "runflex"
    span = 32500 if flex else 15000      # what a transmission and the events behind it need
    mid = 8 if flex else 12
    near = 2016 if flex else 4000        # a burst's sync word lies 3072 samples behind its start
    if flex:
        e1, e2, e3 = flex_step_ends(0, FDEAD - 1, 3)     # a fresh stretch: the search opens at sample 310
    else:
        e1, e2, e3 = pocsag_step_ends(0, 0, 3)
    assert e2 - e1 == e3 - e2 == 32 * STEP_WORDS == 65536 and e1 % 32 == 0 and near % 32 == 0
    chan = lambda n, seed, targets, kinds=None: _idle_channel(pkg, ora, stage, taps, n, seed, targets, kinds)
    if name == "near_far":
        n = (e1 + span) // W * W + W
        targets, steps = [[near + mid], [e1 - 32 + mid]], [0, 0]
        x = [chan(n, 1, targets[0]), chan(n, 2, targets[1])]
    elif name == "one_none":
        n = (e1 + 3008 + span) // W * W + W
        targets, steps = [[e1 + 3008 + mid], []], [1, None]
        x = [chan(n, 3, targets[0]), chan(n, 4, [])]
    elif name == "edges":
        n = (e1 + span) // W * W + W
        targets, steps = [[e1 + mid], [e1 + 32 + mid]], [1, 1]
        x = [chan(n, 5, targets[0]), chan(n, 6, targets[1])]
    else:
        assert name in ("two_after", "two_after_cut")
        n = (e2 + 2016 + span) // W * W + W
        # (f): the first transmission early (BAD_BAUD for FLEX); where the search behind its event ends its first whole step
        # follows from the event's sample, and the second transmission lies 2016 samples behind that
        probe = ora.Resampler(taps, 1, 1).feed(chan(n, 8, [near + mid], [BAD_BAUD]))
        ev, searches = _searches(ora, stage, probe)
        assert len(searches) == 2 and len(ev) == (1 if flex else 3), ev["type"].tolist()
        after = (flex_step_ends(0, searches[1], 1) if flex else pocsag_step_ends(0, searches[1], 1, rst=searches[1]))[0]
        targets, steps = [[e2 + 2016 + mid], [near + mid, after + 2016 + mid]], [2, 0]
        assert after % 32 == 0 and after - searches[1] <= 65536 + 4096 and targets[1][1] + span <= n
        x = [chan(n, 7, targets[0]), chan(n, 8, targets[1], [BAD_BAUD, FRAME])]
    stream = np.ascontiguousarray(np.stack(x))
    mask = np.ones((2, n // W), bool)
    cuts = [40000 // W * W, n - 40000 // W * W] if name == "two_after_cut" else [n]
    calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
    chk, want = _want(pkg, ora, stage, taps, W, calls)
    by = chk.stretches()
    assert sorted(by) == [(0, 0), (1, 0)] and all(len(w[0][0]) == 2 for w in want)   # one run per channel per call
    # the guards, on the oracle's figures alone: the resampled stretch, its events, the matcher restated
    fig = dict(outs=[], first_hit=[], idle=[], steps=[], events=[])
    for c in (0, 1):
        y = np.concatenate(chk.pcm[(c, 0)])
        ev = by[(c, 0)][0] if flex else by[(c, 0)]
        F = int(want[-1][0][0]["first_out"][c])      # where the last call's run begins: 0 unless the stream is cut
        assert (F > 0) == (len(cuts) == 2) and F < 40000
        ev2, searches = _searches(ora, stage, y)
        assert len(ev2) == len(ev) and [int(s) for s in ev2["sample"]] == [int(s) for s in ev["sample"]]
        types = [int(t) for t in ev["type"]]
        if flex:
            assert types == ([FRAME] * len(targets[c]) if name[:3] != "two" or c == 0 else [BAD_BAUD, FRAME]), (name, c, types)
            for e, t in zip(ev, targets[c]):   # the event is the one the match at the target opens: its BS1 run ends at j
                s0 = int(e["sync_sample"]) - 1110 if int(e["type"]) == FRAME else int(e["sample"]) - 790
                j = s0 - (10 - (int(e["eye"]) // 2) % 10)
                assert t <= j - int(e["eye"]) and j <= t + 400, (name, c, t, j, int(e["eye"]))
            hits = flex_m(y)
        else:
            assert types == [ora.EV_SYNC_FOUND, ora.EV_BATCH, ora.EV_SYNC_LOST] * len(targets[c]), (name, c, types)
            for k, t in enumerate(targets[c]):  # the SYNC_FOUND ends the run of matches that begins at the target
                f, run = int(ev["sample"][3 * k]), int(ev["aux"][3 * k])
                assert t - 1 <= f - run <= t + 1 and (ev["baud"][3 * k:3 * k + 3] == 2400).all(), (name, c, t, f, run)
            flagged = pocsag_flagged(y, 0, F) + pocsag_flagged(y, F, y.size - F) if F else pocsag_flagged(y, 0, y.size)
        assert len(searches) == len(targets[c]) + 1
        fig["outs"].append(y.size)
        fig["events"].append(list(zip(types, [int(s) for s in ev["sample"]])))
        firsts, idle, taken = [], [], []
        for i, p in enumerate(searches):
            # where the search ends: the first hit of the matcher behind p (FLEX: the sample; POCSAG: the segment word with
            # the summary bit, and nothing on the way - the fill sets no summary bit), or the stretch's end
            if flex:
                at = np.flatnonzero(hits[p:])
                stop = p + int(at[0]) if at.size else y.size
            else:
                at = [w for w in flagged if w + 32 > p]
                stop = at[0] if at else y.size
            if i < len(targets[c]):
                t = targets[c][i]
                assert stop == (t if flex else t - mid) or (F and not flex and stop <= t < stop + 32), (name, c, i, stop, t)
                firsts.append(stop)
            else:
                assert stop == y.size or stop > p + 2400, (name, c, i, p, stop)   # nothing right behind the last event
                stop = y.size if not targets[c] else stop
            rst = p if i else 0
            if p < F < stop:   # the first call's run ends idle and short of a whole step; the second call's goes on at F
                assert (flex_step_ends(0, p, 1) if flex else pocsag_step_ends(0, p, 1, rst))[0] >= F
                p, rst = F, 0
            base = F if p >= F else 0
            ends = flex_step_ends(base, p, 4) if flex else pocsag_step_ends(base, p, 4, rst)
            idle.append(stop - p)
            taken.append(sum(1 for e in ends if e <= stop))
        fig["first_hit"].append(firsts)
        fig["idle"].append(idle)
        fig["steps"].append(taken)
        if name == "two_after_cut":
            assert c == 1 or (taken[0] >= 1 and idle[0] > 65536), (name, c, taken, idle)
        elif name == "two_after":
            assert (taken[0] == 2 and idle[0] > 131072) if c == 0 else (taken[:2] == [0, 1] and idle[1] > 65536), (name, c, taken, idle)
        elif steps[c] is None:      # (g): a step, then the clamp to the run's end inside the next one
            assert taken == [1] and e1 < y.size < e2 and not len(ev), (name, c, taken, y.size)
        else:
            # a run's first step is short of 65 536 samples by the history words and the summary word the search begins in
            assert taken[0] == steps[c] and idle[0] >= (65536 - 32 * ((FHW if flex else PHW) + 32)) * steps[c], (name, c, taken, idle)
    if name == "near_far":      # (d) and, in `edges`, (e): the words on either side of the first step's end
        assert e1 - 32 <= fig["first_hit"][1][0] < e1
    if name == "edges":
        assert e1 <= fig["first_hit"][0][0] < e1 + 32 <= fig["first_hit"][1][0] < e1 + 64
    FIGURES[f"idle {stage} {name}"] = fig
    _IDLE[(stage, name)] = dict(calls=calls, want=want, taps=taps, by=by, n=n)
    return _IDLE[(stage, name)]


IDLE_CASES = ["near_far", "one_none", "edges", "two_after", "two_after_cut"]


@pytest.mark.parametrize("name", IDLE_CASES)
@pytest.mark.parametrize("stage", ["runpocsag", "runflex"])
def test_hosttwin_long_idle_runs(pkg, ora, stage, name):
    """the scene's guards and the host twin on it"""
    sc = idle_scene(pkg, ora, stage, name)
    call, _ = _twin(pkg, stage, 2, sc["taps"], IDLE_W)
    got = []
    for i, (g, w) in enumerate(zip(sc["calls"], sc["want"])):
        got.append(call(g, w[0]))
        _same(stage, got[-1], w, f"{stage} {name}, call {i}")
    _cut_independent(stage, got, sc["by"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDLE_CASES)
@pytest.mark.parametrize("stage", ["runpocsag", "runflex"])
def test_gpu_long_idle_runs(pkg, ora, stage, name):
    """the walkers' summary skip inside a run: no, one and two whole steps of 65 536 samples before the first match; the match
    in the last word a step covers, in the first and the second behind it; a step from the state an earlier event left; a run
    that ends inside a step behind a real one; and the longest stream cut inside the idle span, so that a continuing run
    starts idle (idle_scene has the cases and their guards)"""
    import torch
    sc = idle_scene(pkg, ora, stage, name)
    o, call = _device(pkg, torch, stage, 2, sc["taps"], IDLE_W, 4, 0, 2 * sc["n"])
    twin, twin_state = _twin(pkg, stage, 2, sc["taps"], IDLE_W)
    got = []
    for i, (g, w) in enumerate(zip(sc["calls"], sc["want"])):
        got.append(call(g, w[0]))
        _same(stage, got[-1], w, f"{stage} {name}, call {i}")
        _views_match(pkg, stage, o, got[-1], len(w[0][0]))
        twin(g, w[0])
    _cut_independent(stage, got, sc["by"])
    _state_is_the_twins(stage, o, twin_state)
    o.close()
