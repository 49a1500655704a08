"""The level stage's adaptive squelch (mfm_level_set_adaptive; csrc/mfm_level.h, csrc/mfm_level_adaptive.hip): per channel a
noise floor - the smallest (OPEN_ABOVE) or largest (OPEN_BELOW) metric of the last M windows - and a squelch on ratios to it.

Every expected value comes from the plain-Python restatement in this file (Python ints, so no product wraps; slices and min /
max for the floor; a hand-written state machine) on the window sums of tests/test_level.py's restatement; every comparison is
exact equality."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_level as tl

ROOT = tl.ROOT
PCM, IQ, ENERGY, DIFF, ABOVE, BELOW = tl.PCM, tl.IQ, tl.ENERGY, tl.DIFF, tl.ABOVE, tl.BELOW
NEW_NAMES = ["mfm_level_set_adaptive", "mfm_level_get_adaptive", "mfm_level_fetch_floor", "mfm_level_floor_view", "mfm_hosttwin_level_adaptive"]
U64 = (1 << 64) - 1


# ---- the restatement ----------------------------------------------------------------------------------------

def adaptive_run(metrics, sense, open_thr, close_thr, hang, M, open_q8, close_q8, warmup, wrap=False):
    """(floors, opens) of one channel from its first window after create / seek on.  wrap=True takes the products modulo 2^64:
    what a 64-bit multiply would make of them, to show that a case tells the two apart"""
    metrics = [int(m) for m in metrics]
    mask = U64 if wrap else (1 << 200) - 1
    floors, opens, open_, bad = [], [], 0, 0
    for k, m in enumerate(metrics):
        last = metrics[max(0, k - M + 1):k + 1]
        f = max(last) if sense == BELOW else min(last)
        m256, fo, fc = (m * 256) & mask, (f * open_q8) & mask, (f * close_q8) & mask
        if sense == BELOW:
            on_open_side = k >= warmup and m256 <= fo and m <= open_thr
            is_bad = m256 > fc or m > close_thr
        else:
            on_open_side = k >= warmup and m256 >= fo and m >= open_thr
            is_bad = m256 < fc or m < close_thr
        if not open_:
            if on_open_side:
                open_, bad = 1, 0
        elif is_bad:
            bad += 1
            if bad > hang:
                open_, bad = 0, 0
        else:
            bad = 0
        floors.append(f)
        opens.append(open_)
    return floors, opens


def restate_adaptive(plain, metric, sense, open_thr, close_thr, hang, M, open_q8, close_q8, warmup):
    """plain: the records of tests/test_level.py's restate() for the stream from create / seek on; returns (records with the
    adaptive squelch's .open, floors uint64 [C][windows])"""
    rec = plain.copy()
    floor = np.zeros(plain.shape, np.uint64)
    for c in range(plain.shape[0]):
        m = plain["diff_energy" if metric == DIFF else "energy"][c].tolist()
        f, o = adaptive_run(m, sense, open_thr, close_thr, hang, M, open_q8, close_q8, warmup)
        floor[c] = np.array(f, np.uint64) if f else 0
        rec["open"][c] = o
    return rec, floor


def same_floor(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint64, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: floor differs at (channel, window) {bad[:5].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def twin(pkg, metrics, sense, open_thr, close_thr, hang, M, open_q8, close_q8, warmup):
    f, o = pkg.binding.hosttwin_level_adaptive(np.array(metrics, np.uint64), sense, open_thr, close_thr, hang, M, open_q8, close_q8, warmup)
    return [int(v) for v in f], [int(v) for v in o]


# ---- the motivating scene -------------------------------------------------------------------------------------

SCENE = dict(W=256, windows=40, sigmas=(20.0, 200.0, 2000.0), bursts=list(range(10, 15)) + [25, 26],
             M=16, open_q8=1024, close_q8=512, hang=0, warmup=4)


def scene_rows(seed):
    """IQ rows int16 [3][n][2]: Gaussian noise of sigma 20, 200 and 2000 per component, a complex tone of 6 sigma in the burst windows"""
    W, nw = SCENE["W"], SCENE["windows"]
    rng = np.random.RandomState(seed)
    n = W * nw
    t = np.arange(n)
    on = np.zeros(n, bool)
    for k in SCENE["bursts"]:
        on[k * W:(k + 1) * W] = True
    rows = np.zeros((3, n, 2), np.int16)
    for c, sigma in enumerate(SCENE["sigmas"]):
        ph = 2.0 * np.pi * (0.05 * t + rng.rand())
        re = rng.normal(0.0, sigma, n) + on * 6.0 * sigma * np.cos(ph)
        im = rng.normal(0.0, sigma, n) + on * 6.0 * sigma * np.sin(ph)
        rows[c, :, 0] = np.round(re)
        rows[c, :, 1] = np.round(im)
    return rows


def scene_want(pkg, rows):
    plain = tl.restate(pkg, rows, SCENE["W"], IQ)
    return plain, restate_adaptive(plain, ENERGY, ABOVE, 0, 0, SCENE["hang"], SCENE["M"], SCENE["open_q8"], SCENE["close_q8"], SCENE["warmup"])


def scene_mask():
    m = np.zeros(SCENE["windows"], bool)
    m[SCENE["bursts"]] = True
    return m


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_adaptive_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared and hasattr(lib, n) and n in pkg.binding.ABI_SYMBOLS, n
    m = re.search(r"struct mfm_level_adaptive \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["floor_windows", "open_q8", "close_q8", "warmup_windows", "flags", "reserved"]
    import ctypes as C
    assert C.sizeof(pkg.binding.LevelAdaptive) == 24


def _metric_sequence(rng, n, top):
    """an idle level that drifts, bursts of a few windows well off it on both sides, and plain random stretches: both transitions
    of the squelch happen in either sense"""
    idle = top // 64
    m = (idle * np.exp(rng.normal(0.0, 0.15, n) + 0.3 * np.sin(np.arange(n) / 37.0))).astype(np.float64)
    k = 0
    while k < n:
        k += int(rng.randint(3, 40))
        ln = int(rng.randint(1, 12))
        m[k:k + ln] *= float(rng.choice([0.02, 0.1, 0.3, 3.0, 10.0, 50.0]))
        k += ln
    m[n // 2:n // 2 + n // 8] = rng.randint(0, top, size=len(m[n // 2:n // 2 + n // 8]))
    return [int(v) for v in np.clip(m, 0, top)]


@pytest.mark.parametrize("sense", [ABOVE, BELOW])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 1024])
def test_hosttwin_adaptive_equals_python_restatement(pkg, sense, M):
    """random metric sequences; hang 0, 1 and 3, warm-up 0 and 5, with and without the absolute limits"""
    rng = np.random.RandomState(1000 * sense + M)
    opened = closed = 0
    for hang in (0, 1, 3):
        for warmup in (0, 5):
            for limits in (False, True):
                top = 1 << int(rng.choice([20, 40, 61]))
                n = 700 if M < 1024 else 2500
                metrics = _metric_sequence(rng, n, top)
                oq, cq = ((1024, 512), (320, 288), (256, 256))[int(rng.randint(0, 3))]
                if sense == BELOW:
                    oq, cq = 65536 // oq, 65536 // cq
                    open_thr, close_thr = (top // 64, top // 32) if limits else (U64, U64)
                else:
                    open_thr, close_thr = (top // 64, top // 128) if limits else (0, 0)
                args = (sense, open_thr, close_thr, hang, M, oq, cq, warmup)
                want = adaptive_run(metrics, *args)
                got = twin(pkg, metrics, *args)
                assert got[0] == want[0], ("floor", args)
                assert got[1] == want[1], ("open", args)
                assert not any(want[1][:warmup])
                steps = np.diff(np.array([0] + want[1]))
                opened += int((steps == 1).sum())
                closed += int((steps == -1).sum())
    assert opened >= 10 and closed >= 10, (opened, closed)  # the sequences exercise both transitions (M = 1: by the absolute limits alone)


def test_hosttwin_adaptive_on_the_ratio_thresholds(pkg):
    """metric * 256 == floor * q8 opens and is not bad, one less (more) does not open and is bad"""
    def run(sense, metrics, M, oq, cq, hang=0, warmup=0, open_thr=None, close_thr=None):
        none = U64 if sense == BELOW else 0
        args = (sense, none if open_thr is None else open_thr, none if close_thr is None else close_thr, hang, M, oq, cq, warmup)
        want = adaptive_run(metrics, *args)
        assert twin(pkg, metrics, *args) == want
        return want

    # ABOVE, floor 100: opens at 4 x = 400, bad below 2 x = 200
    f, o = run(ABOVE, [100, 399, 400, 200, 199, 400], 8, 1024, 512)
    assert f == [100] * 6 and o == [0, 0, 1, 1, 0, 1]
    f, o = run(ABOVE, [100, 400, 199, 200, 199, 199], 8, 1024, 512, hang=1)
    assert o == [0, 1, 1, 1, 1, 0]
    # the window itself is part of the floor, and a window M back is not
    f, o = run(ABOVE, [100, 400, 400, 400], 3, 1024, 512)
    assert f == [100, 100, 100, 400] and o == [0, 1, 1, 0]
    # warm-up: on the open side counts for nothing, the floor is formed all the same
    f, o = run(ABOVE, [100, 400, 400, 400, 400], 8, 1024, 512, warmup=3)
    assert f == [100] * 5 and o == [0, 0, 0, 1, 1]
    # the absolute limits stay in force: metric 400 passes the ratio, not open_thr 401; and close_thr 300 makes 299 bad
    assert run(ABOVE, [100, 400, 401, 299], 8, 1024, 512, open_thr=401, close_thr=300)[1] == [0, 0, 1, 0]
    # BELOW, floor (the largest) 1000: opens at 1/4 = 250, bad above 1/2 = 500
    f, o = run(BELOW, [1000, 251, 250, 500, 501, 250], 8, 64, 128)
    assert f == [1000] * 6 and o == [0, 0, 1, 1, 0, 1]
    assert run(BELOW, [1000, 250, 249, 400], 8, 64, 128, open_thr=249, close_thr=399)[1] == [0, 0, 1, 0]
    # a silent channel: floor 0, every metric passes the ratio test; open_thr 1 keeps it shut
    assert run(ABOVE, [0, 0, 0, 0], 4, 1024, 512)[1] == [1, 1, 1, 1]
    assert run(ABOVE, [0, 0, 0, 0], 4, 1024, 512, open_thr=1, close_thr=0)[1] == [0, 0, 0, 0]


def test_hosttwin_adaptive_products_do_not_wrap(pkg):
    """metrics near 2^61 with q8 = 65536: floor * 65536 and metric * 256 pass 2^64; the twin follows the Python ints, and a
    product taken modulo 2^64 gives another answer on the same sequences"""
    cases = [(ABOVE, [(1 << 53) - 1, 1 << 61, 1 << 61], 65536, 65536),      # 2^69 >= 2^69 - 65536: opens; wrapped: 0 >= 2^64 - 65536 does not
             (ABOVE, [1 << 60, (1 << 61) - 1, 1 << 60], 65536, 256),        # (2^61 - 1) * 256 < 2^76: stays closed; wrapped it opens
             (BELOW, [(1 << 61) - 1, 1 << 52, 1 << 61], 1, 65536),          # opens at 1/256 of the floor; bad only above 256 floors
             (ABOVE, [(1 << 61) - 1, (1 << 61) - 1, (1 << 61) - 2], 257, 256)]
    differs = 0
    for sense, metrics, oq, cq in cases:
        none = U64 if sense == BELOW else 0
        args = (sense, none, none, 0, 4, oq, cq, 0)
        want = adaptive_run(metrics, *args)
        assert twin(pkg, metrics, *args) == want, (metrics, args)
        differs += adaptive_run(metrics, *args, wrap=True)[1] != want[1]
    assert differs >= 2


def test_motivating_scene_opens_exactly_on_the_bursts_where_no_fixed_threshold_can(pkg):
    """three channels whose noise differs by 40 dB, the same 6-sigma bursts on each: with M = 16, open at 4 floors, bad below 2,
    warm-up 4 every channel is open in exactly the seven burst windows, over 20 seeds; and the weakest burst window of channel 0
    carries less energy than the strongest idle window of channel 2, so no fixed open_thr does the same"""
    mask = scene_mask()
    for seed in range(20):
        rows = scene_rows(seed)
        plain, (rec, floor) = scene_want(pkg, rows)
        for c in range(3):
            assert np.array_equal(rec["open"][c].astype(bool), mask), (seed, c, rec["open"][c].tolist())
            f, o = twin(pkg, plain["energy"][c].tolist(), ABOVE, 0, 0, SCENE["hang"], SCENE["M"], SCENE["open_q8"], SCENE["close_q8"], SCENE["warmup"])
            assert o == rec["open"][c].tolist() and f == floor[c].tolist()
        assert int(plain["energy"][0][mask].min()) < int(plain["energy"][2][~mask].max())


def test_adaptive_kernel_uses_no_scratch_and_does_not_spill():
    """the code object's notes of build/mfm_level_adaptive.o (tools/kernel_regs.py), as tests/test_level.py reads them for
    mfm_level.o: one kernel, no private segment, no spilled register.  It never skips: where the tool cannot read the object
    the test fails"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_level_adaptive.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_level_adaptive.o"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert len(lines) == 1 and "lv_adaptive_finish_kernel" in lines[0], out
    m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", lines[0])
    assert m and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), lines[0]


# ---- GPU ------------------------------------------------------------------------------------------------------

def _gained_rows(rng, nch, n, W, form):
    """random rows whose level changes from window to window (gains spread over 26 dB), so that ratios to a floor open and close;
    with three channels or more: channel 1 silent (floor 0), channel 2 all -32768"""
    nw = n // W + 1
    shape = (nch, n, 2) if form == IQ else (nch, n)
    x = rng.randint(-32768, 32768, size=shape).astype(np.float32)
    gain = np.exp(rng.uniform(np.log(0.05), 0.0, size=(nch, nw))).astype(np.float32)
    g = np.repeat(gain, W, axis=1)[:, :n]
    x *= g[:, :, None] if form == IQ else g
    x = x.astype(np.int16)
    if nch >= 3:
        x[1] = 0
        x[2] = -32768
    return x


def _upload(torch, x, form, in_stride=None, lead=3):
    """x on the device with an odd in_stride behind an odd number of samples: (tensor to keep, address of row 0, in_stride)"""
    E = 2 if form == IQ else 1
    n = x.shape[1]
    in_stride = in_stride or n * E + 1 + (n * E) % 2
    assert in_stride % 2 == 1 and lead % 2 == 1
    d, ptr = tl._on_device(torch, x, in_stride, lead)
    return d, ptr, in_stride


def _run_calls(pkg, dev, nch, W, form, calls, kw, ad, cap=None):
    """the rows of _upload() through one Level with the adaptive squelch `ad`, in process_device calls of `calls` samples; returns
    (records, floors) of all calls side by side and the windows each call completed"""
    _, ptr, in_stride = dev
    E = 2 if form == IQ else 1
    lv = pkg.Level(nch, cap or max(max(calls), 1), W, form=form, **kw)
    lv.set_adaptive(*ad)
    recs, floors, per_call, pos = [], [], [], 0
    for m in calls:
        lv.process_device(ptr + 2 * E * pos, in_stride, m)
        recs.append(lv.fetch())
        floors.append(lv.fetch_floor())
        assert recs[-1].shape == floors[-1].shape == (nch, (pos + m) // W - pos // W)
        per_call.append(recs[-1].shape[1])
        pos += m
    lv.close()
    return np.concatenate(recs, axis=1), np.concatenate(floors, axis=1), per_call


def _settings(plain, i, nch, form):
    """the i-th setting of a test: both senses and, in the PCM form, both metrics come up for every channel count"""
    metric = DIFF if (form == PCM and (i + nch) % 3 == 0) else ENERGY
    sense = BELOW if (i + nch) % 2 else ABOVE
    m = plain["diff_energy" if metric == DIFF else "energy"]
    q = int(np.percentile(m.astype(np.float64), 30 if sense == ABOVE else 70)) if m.size else 0
    if i % 3 == 0:
        open_thr, close_thr = (0, 0) if sense == ABOVE else (U64, U64)
    else:
        open_thr, close_thr = (q, q // 2) if sense == ABOVE else (q, 2 * q)
    oq, cq = (1024, 512) if sense == ABOVE else (64, 128)
    return metric, sense, open_thr, close_thr, (i + nch) % 3, oq, cq, (3 * i) % 7


@pytest.mark.gpu
def test_gpu_motivating_scene_equals_restatement_and_no_fixed_threshold_does_the_same(pkg):
    import torch
    rows = scene_rows(3)
    W, n = SCENE["W"], rows.shape[1]
    plain, (want, want_floor) = scene_want(pkg, rows)
    ad = (SCENE["M"], SCENE["open_q8"], SCENE["close_q8"], SCENE["warmup"])
    rec, floor, _ = _run_calls(pkg, _upload(torch, rows, IQ), 3, W, IQ, [n], dict(sense=ABOVE, hang_windows=SCENE["hang"]), ad)
    tl.same_records(rec, want, "scene")
    same_floor(floor, want_floor, "scene")
    mask = scene_mask()
    assert all(np.array_equal(rec["open"][c].astype(bool), mask) for c in range(3))
    # the same rows with the adaptive squelch off and one fixed threshold from the scene (between channel 1's idle and burst
    # windows): channel 2 is open for good, channel 0 never
    thr = int(np.sqrt(float(plain["energy"][1][mask].min()) * float(plain["energy"][1][~mask].max())))
    lv = pkg.Level(3, n, W, form=IQ, sense=ABOVE, open_thr=thr, close_thr=thr)
    assert lv.get_adaptive() is None
    fixed = lv.process_host(rows)
    lv.close()
    tl.same_records(fixed, tl.restate(pkg, rows, W, IQ, sense=ABOVE, open_thr=thr, close_thr=thr), "fixed threshold")
    assert np.array_equal(fixed["open"][1].astype(bool), mask)
    assert not fixed["open"][0].any() and fixed["open"][2].all()


WINDOWS_PER_CALL = (0, 1, 63, 64, 65, 130)
MS = (1, 2, 63, 64, 65, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [7, 300, 4096, 5000])
@pytest.mark.parametrize("form", [PCM, IQ])
def test_gpu_adaptive_equals_restatement(pkg, form, W):
    """1, 3, 64 and 130 channels; M = 1, 2, 63, 64, 65 and 200; calls that complete 0, 1, 63, 64, 65 and 130 windows - at every W
    with 1 and 3 channels, at W = 7 with every channel count, at W = 300 with 64; where that stream would pass 7 million elements
    per form the calls complete 0, 1 and 65 or 0, 1 and 2 windows (the rounds of 64 windows and the strips are the same code at
    every W and channel count, which wave sums a window is not).  Both senses, both metrics, with and without the absolute limits;
    an odd in_stride and a row pointer offset by an odd number of samples; a silent and a full-scale channel among the random ones"""
    import torch
    for nch in (1, 3, 64, 130):
        per_call = next(pc for pc in (WINDOWS_PER_CALL, (0, 1, 65), (0, 1, 2)) if sum(pc) * W * nch <= 7000000)
        r = max(1, W // 3)  # the first call ends inside window 0; every later one completes whole windows and leaves r samples
        calls = [r] + [k * W for k in per_call[1:]] + [0]
        n = sum(calls)
        rng = np.random.RandomState(W + 7 * nch + form)
        x = _gained_rows(rng, nch, n, W, form)
        plain = tl.restate(pkg, x, W, form)
        dev = _upload(torch, x, form)
        opened = closed = False
        for i, M in enumerate(MS):
            metric, sense, open_thr, close_thr, hang, oq, cq, warmup = _settings(plain, i, nch, form)
            want, want_floor = restate_adaptive(plain, metric, sense, open_thr, close_thr, hang, M, oq, cq, warmup)
            steps = np.diff(want["open"].astype(np.int64), axis=1)
            opened, closed = opened or bool((steps == 1).any()), closed or bool((steps == -1).any())
            kw = dict(metric=metric, sense=sense, open_thr=open_thr, close_thr=close_thr, hang_windows=hang)
            rec, floor, got_per_call = _run_calls(pkg, dev, nch, W, form, calls, kw, (M, oq, cq, warmup))
            what = f"form {form} W {W} channels {nch} M {M} sense {sense} metric {metric}"
            assert got_per_call == list(per_call) + [0], what
            tl.same_records(rec, want, what)
            same_floor(floor, want_floor, what)
            if nch >= 3:
                assert not want_floor[1].any() and int(want["peak"][2].max()) == 32768
        assert (opened and closed) or per_call == (0, 1, 2), (W, nch)  # over the six settings the squelch opens and closes


@pytest.mark.gpu
def test_gpu_adaptive_wide_input_kernel_at_64_channels_across_a_round_edge(pkg):
    """W = 4096 with 64 channels - one wave per slot in the input kernel, a grid of many channels - and a call that completes 65
    windows: the second round of the finish kernel holds one window.  M = 63 (sense ABOVE) and 64 (sense BELOW)"""
    import torch
    W, nch, form = 4096, 64, PCM
    calls = [W // 3, 65 * W, 0]
    rng = np.random.RandomState(4096 + 64)
    x = _gained_rows(rng, nch, sum(calls), W, form)
    plain = tl.restate(pkg, x, W, form)
    dev = _upload(torch, x, form)
    senses = set()
    for i in (2, 3):
        M = MS[i]
        metric, sense, open_thr, close_thr, hang, oq, cq, warmup = _settings(plain, i, nch, form)
        senses.add(sense)
        want, want_floor = restate_adaptive(plain, metric, sense, open_thr, close_thr, hang, M, oq, cq, warmup)
        kw = dict(metric=metric, sense=sense, open_thr=open_thr, close_thr=close_thr, hang_windows=hang)
        rec, floor, per_call = _run_calls(pkg, dev, nch, W, form, calls, kw, (M, oq, cq, warmup))
        assert per_call == [0, 65, 0]
        tl.same_records(rec, want, f"W 4096, 64 channels, M {M}")
        same_floor(floor, want_floor, f"W 4096, 64 channels, M {M}")
        steps = np.diff(want["open"].astype(np.int64), axis=1)
        assert (steps == 1).any() and (steps == -1).any()
    assert senses == {ABOVE, BELOW}


@pytest.mark.gpu
@pytest.mark.parametrize("sense", [ABOVE, BELOW])
@pytest.mark.parametrize("form", [PCM, IQ])
def test_gpu_adaptive_calls_of_more_than_one_strip(pkg, form, sense):
    """the finish kernel holds 1024 windows of a call in LDS at a time.  W = 7, 4 channels: a first call that completes 2137
    windows (two full strips and one of 89) and leaves 4 samples, a second of 300 windows that reads the history the partial last
    strip left, a third of exactly 2048 (the last strip a full one), a fourth of 1025 (a last strip of one window).  M = 1, 200
    and 1024 - the largest strip in LDS, M - 1 + 1024 entries - with a warm-up that ends inside the first strip"""
    import torch
    W, nch = 7, 4
    windows = [2137, 300, 2048, 1025]
    calls = [windows[0] * W + 4] + [k * W for k in windows[1:]]
    rng = np.random.RandomState(2137 + 10 * form + sense)
    x = _gained_rows(rng, nch, sum(calls), W, form)
    plain = tl.restate(pkg, x, W, form)
    assert plain.shape == (nch, sum(windows))
    dev = _upload(torch, x, form)
    oq, cq = (1024, 512) if sense == ABOVE else (64, 128)
    none = 0 if sense == ABOVE else U64
    opened = closed = False
    for M in (1, 200, 1024):
        want, want_floor = restate_adaptive(plain, ENERGY, sense, none, none, 1, M, oq, cq, 5)
        kw = dict(metric=ENERGY, sense=sense, open_thr=none, close_thr=none, hang_windows=1)
        rec, floor, per_call = _run_calls(pkg, dev, nch, W, form, calls, kw, (M, oq, cq, 5))
        assert per_call == windows
        tl.same_records(rec, want, f"strips, form {form} sense {sense} M {M}")
        same_floor(floor, want_floor, f"strips, form {form} sense {sense} M {M}")
        steps = np.diff(want["open"].astype(np.int64), axis=1)
        opened, closed = opened or bool((steps[:, 1024:] == 1).any()), closed or bool((steps[:, 1024:] == -1).any())
    assert opened and closed  # also behind the first strip


@pytest.mark.gpu
@pytest.mark.parametrize("form", [PCM, IQ])
def test_gpu_adaptive_long_windows(pkg, form):
    """W = 4096 * 65: more than 64 slots per window, the wave-per-window branch of the window sums; 3 channels, 3 windows"""
    import torch
    W, nch = 4096 * 65, 3
    calls = [W // 2, W, 2 * W]
    rng = np.random.RandomState(65 + form)
    x = _gained_rows(rng, nch, sum(calls), W, form)
    plain = tl.restate(pkg, x, W, form)
    assert plain.shape == (nch, 3)
    dev = _upload(torch, x, form)
    for i, M in enumerate(MS):
        metric, sense, open_thr, close_thr, hang, oq, cq, _ = _settings(plain, i, nch, form)
        want, want_floor = restate_adaptive(plain, metric, sense, open_thr, close_thr, hang, M, oq, cq, i % 2)
        kw = dict(metric=metric, sense=sense, open_thr=open_thr, close_thr=close_thr, hang_windows=hang)
        rec, floor, _ = _run_calls(pkg, dev, nch, W, form, calls, kw, (M, oq, cq, i % 2))
        tl.same_records(rec, want, f"long windows, form {form} M {M}")
        same_floor(floor, want_floor, f"long windows, form {form} M {M}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [PCM, IQ])
@pytest.mark.parametrize("W", [7, 300])
def test_gpu_adaptive_does_not_depend_on_the_cuts(pkg, form, W):
    """one stream in one call, and cut into seeded random pieces (length 0, length 1, below W, ending exactly on a window edge,
    and at the end four calls in a row that complete no window) through process_device and through process_host: the same records
    and floors, equal to the restatement.  M = 50 is more than the windows of any piece (4 at most), so every floor of a cut run
    reaches into the history the device keeps"""
    import torch
    nch, M = 5, 50
    n = 40 * W + 13 if W >= 300 else 6000 + W + (13 - (6000 + W) % W) % W
    rng = np.random.RandomState(200 + W + form)
    x = _gained_rows(rng, nch, n, W, form)
    E = 2 if form == IQ else 1
    plain = tl.restate(pkg, x, W, form)
    kw = dict(metric=ENERGY, sense=ABOVE, open_thr=0, close_thr=0, hang_windows=1)
    ad = (M, 768, 384, 2)
    want, want_floor = restate_adaptive(plain, ENERGY, ABOVE, 0, 0, 1, *ad)
    rec, floor, _ = _run_calls(pkg, _upload(torch, x, form), nch, W, form, [n], kw, ad)
    tl.same_records(rec, want, "one call")
    same_floor(floor, want_floor, "one call")
    biggest = 3 * W + 2
    tail = n % W
    assert tail >= 6
    cuts = tl._cuts(rng, n - tail, W, biggest) + [2, 0, tail - 5, 3]
    assert sum(cuts) == n
    rec, floor, per_call = _run_calls(pkg, _upload(torch, x, form, in_stride=n * E + 3 + (n * E) % 2, lead=1), nch, W, form, cuts, kw, ad, cap=biggest)
    assert max(per_call) < M and per_call[-4:] == [0, 0, 0, 0]
    tl.same_records(rec, want, "process_device, cut")
    same_floor(floor, want_floor, "process_device, cut")
    host = pkg.Level(nch, biggest, W, form=form, **kw)
    host.set_adaptive(*ad)
    recs, floors, pos = [], [], 0
    for m in cuts:
        recs.append(host.process_host(x[:, pos:pos + m]))
        floors.append(host.fetch_floor())
        pos += m
    host.close()
    tl.same_records(np.concatenate(recs, axis=1), want, "process_host, cut")
    same_floor(np.concatenate(floors, axis=1), want_floor, "process_host, cut")
    steps = np.diff(want["open"].astype(np.int64), axis=1)
    assert (steps == 1).any() and (steps == -1).any()


@pytest.mark.gpu
def test_gpu_adaptive_products_do_not_wrap(pkg):
    """IQ rows of -32768, W = 2^18: a window's energy is 2^49, and with open_q8 = 65536 floor * q8 = 2^65 passes 2^64.  Channel 0:
    all full scale, metric * 256 = 2^57 < 2^65, never opens; a product modulo 2^64 is 0 there and opens.  Channel 1: its first
    window silent, so the floor is 0 and it opens; M = 2 lets the floor come up again in window 2, which is bad"""
    import torch
    W, nch, nw = 1 << 18, 2, 3
    x = np.full((nch, nw * W, 2), -32768, np.int16)
    x[1, :W] = 0
    plain = tl.restate(pkg, x, W, IQ)
    assert int(plain["energy"][0, 0]) == 1 << 49
    ad = (2, 65536, 65536, 0)
    want, want_floor = restate_adaptive(plain, ENERGY, ABOVE, 0, 0, 0, *ad)
    assert want["open"].tolist() == [[0, 0, 0], [1, 1, 0]]
    assert adaptive_run(plain["energy"][0].tolist(), ABOVE, 0, 0, 0, *ad, wrap=True)[1] == [1, 1, 1]
    rec, floor, _ = _run_calls(pkg, _upload(torch, x, IQ), nch, W, IQ, [nw * W], dict(sense=ABOVE), ad)
    tl.same_records(rec, want, "wrap")
    same_floor(floor, want_floor, "wrap")


@pytest.mark.gpu
def test_gpu_adaptive_dead_channel(pkg):
    """a silent channel has floor 0, where every metric passes the ratio test: open_thr = 1 keeps it shut, with open_thr = 0 it
    opens at the first window past the warm-up"""
    W, nch, nw = 100, 2, 12
    x = np.zeros((nch, nw * W), np.int16)
    for open_thr, opens in ((1, [0] * nw), (0, [0] * 3 + [1] * (nw - 3))):
        lv = pkg.Level(nch, nw * W, W, sense=ABOVE, open_thr=open_thr, close_thr=0)
        lv.set_adaptive(8, 1024, 512, 3)
        rec = lv.process_host(x)
        floor = lv.fetch_floor()
        lv.close()
        assert not floor.any() and floor.shape == (nch, nw)
        assert rec["open"].tolist() == [opens] * nch, open_thr
        assert adaptive_run([0] * nw, ABOVE, open_thr, 0, 0, 8, 1024, 512, 3)[1] == opens


@pytest.mark.gpu
def test_gpu_adaptive_seek_starts_history_and_warmup_over_and_keeps_the_setting(pkg):
    nch, W, M = 4, 64, 20
    rng = np.random.RandomState(9)
    a, b = _gained_rows(rng, nch, 30 * W + 10, W, PCM), _gained_rows(rng, nch, 45 * W, W, PCM)
    ad = (M, 768, 384, 3)
    kw = dict(sense=ABOVE, hang_windows=1)
    lv = pkg.Level(nch, 64 * W, W, **kw)
    lv.set_adaptive(*ad)
    setting = dict(floor_windows=M, open_q8=768, close_q8=384, warmup_windows=3)
    assert lv.get_adaptive() == setting
    first = lv.process_host(a)
    want_a, floor_a = restate_adaptive(tl.restate(pkg, a, W, PCM), ENERGY, ABOVE, 0, 0, 1, *ad)
    tl.same_records(first, want_a, "before the seek")
    same_floor(lv.fetch_floor(), floor_a, "before the seek")
    at = 1000
    lv.seek(at * W)
    assert lv.get_adaptive() == setting and lv.fetch_floor().shape == (nch, 0)
    got = np.concatenate([lv.process_host(b[:, :7 * W + 5]), lv.process_host(b[:, 7 * W + 5:])], axis=1)
    want_b, floor_b = restate_adaptive(tl.restate(pkg, b, W, PCM), ENERGY, ABOVE, 0, 0, 1, *ad)
    want_b["window"] += at
    tl.same_records(got, want_b, "after the seek")
    same_floor(lv.fetch_floor(), floor_b[:, 7:], "after the seek, second call")
    assert not want_b["open"][:, :3].any() and want_b["open"].any()
    # the floor of the first windows after the seek is formed from those windows alone
    assert np.array_equal(floor_b[:, 0], want_b["energy"][:, 0])
    lv.close()


@pytest.mark.gpu
def test_gpu_set_adaptive_and_fetch_floor_refusals(pkg):
    b = pkg.binding
    lib = pkg.load_library()
    nch, W = 3, 50
    x = _gained_rows(np.random.RandomState(4), nch, 10 * W, W, PCM)

    def refused(lv, *ad, **kw):
        before = lv.get_adaptive()
        with pytest.raises(pkg.MfmError) as ei:
            lv.set_adaptive(*ad, **kw)
        assert ei.value.code == b.MFM_E_INVAL and lib.mfm_last_error(), (ad, kw)
        assert lv.get_adaptive() == before

    for sense, good, wrong_order in ((ABOVE, (8, 1024, 512, 0), (8, 512, 1024, 0)), (BELOW, (8, 64, 128, 0), (8, 128, 64, 0))):
        lv = pkg.Level(nch, 10 * W, W, sense=sense, open_thr=U64 if sense == BELOW else 0, close_thr=U64 if sense == BELOW else 0)
        for bad in ((0, 512, 256, 0), (1025, 512, 256, 0), (8, 0, 0, 0), (8, 65537, 65537, 0), (8, 65537, 256, 0) if sense == ABOVE else (8, 256, 65537, 0),
                    wrong_order):
            refused(lv, *bad)
        refused(lv, *good, flags=1)
        refused(lv, *good, reserved=1)
        assert b"close_q8" in lib.mfm_last_error() or b"flags" in lib.mfm_last_error()
        # off: no floor to fetch or view
        for fn in (lv.fetch_floor, lv.floor_view):
            with pytest.raises(pkg.MfmError) as ei:
                fn()
            assert ei.value.code == b.MFM_E_INVAL
        lv.set_adaptive(*good)
        lv.set_adaptive(good[0], good[1], good[1], 7)   # equal ratios are in order; a fresh object takes a new setting
        lv.set_adaptive(*good)
        assert lv.fetch_floor().shape == (nch, 0)
        lv.process_host(x[:, :W // 2])                  # a call that completes no window is a call
        refused(lv, *good)
        refused(lv, None)
        lv.process_host(x[:, W // 2:])
        for cap in (0, 1, nch * 10 - 1):
            with pytest.raises(pkg.MfmError) as ei:
                lv.fetch_floor(max_values=cap)
            assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == nch * 10 and not ei.value.buffer.any()
        floor = lv.fetch_floor()
        d_floor, stride = lv.floor_view()
        assert stride >= 10 and floor.shape == (nch, 10)
        raw = tl._d2h(d_floor, nch * stride * 8).view(np.uint64).reshape(nch, stride)[:, :10]
        same_floor(raw, floor, "device view")
        lv.seek(0)
        lv.set_adaptive(None)                           # fresh again: off is accepted, and the fixed squelch is back
        assert lv.get_adaptive() is None
        plain = lv.process_host(x)
        tl.same_records(plain, tl.restate(pkg, x, W, PCM, sense=sense, open_thr=U64 if sense == BELOW else 0,
                                          close_thr=U64 if sense == BELOW else 0), "off again")
        lv.close()


@pytest.mark.gpu
def test_gpu_adaptive_level_to_gate_with_preroll_equals_the_gate_twin_on_the_restatement(pkg):
    """level (adaptive) -> gate with pre-roll 1 on the motivating scene, on the device: runs and payload equal
    mfm_hosttwin_gate_call_preroll fed the restatement's records, for the call and for the flush"""
    import torch
    b = pkg.binding
    rows = scene_rows(5)
    W, n, nch, E, P = SCENE["W"], rows.shape[1], 3, 2, 1
    _, (want, _) = scene_want(pkg, rows)
    flat = np.ascontiguousarray(rows).reshape(nch, n * E)
    hist, bits = np.zeros((nch, (P + 1) * W * E), np.int16), np.zeros(nch, np.uint64)
    want_call = b.hosttwin_gate_call_preroll(W, E, P, 0, flat, hist, bits, want)
    want_flush = b.hosttwin_gate_call_preroll(W, E, P, n, np.zeros((nch, 0), np.int16), hist, bits, np.zeros((nch, 0), b.LEVEL_RECORD_DTYPE),
                                              flush=True)
    d, ptr = tl._on_device(torch, rows, n * E + 1, 3)
    lv = pkg.Level(nch, n, W, form=IQ, sense=ABOVE, hang_windows=SCENE["hang"])
    lv.set_adaptive(SCENE["M"], SCENE["open_q8"], SCENE["close_q8"], SCENE["warmup"])
    gate = pkg.Gate(nch, n, W, elems_per_sample=E, preroll_windows=P)
    lv.process_device(ptr, n * E + 1, n)
    d_rec, rec_stride, nw, _ = lv.device_view()
    gate.process_device(ptr, n * E + 1, n, d_rec, rec_stride, nw)
    got_call = gate.fetch()
    gate.flush_device()
    got_flush = gate.fetch()
    for got, exp, what in ((got_call, want_call, "call"), (got_flush, want_flush, "flush")):
        assert got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]), what
    # the seven burst windows and the one in front of each burst, per channel
    assert sum(int(r["nr_windows"]) for r in got_call[0]) + sum(int(r["nr_windows"]) for r in got_flush[0]) == nch * 9
    gate.close()
    lv.close()
    del d


@pytest.mark.gpu
def test_gpu_level_scan_tool_prints_the_floors_and_is_unchanged_without_the_flags(pkg, ora, tmp_path):
    """tools/level_scan.py on the small capture of tests/test_level.py's tool test, IQ form: with --floor-windows, --open-ratio,
    --close-ratio and --warmup its lines carry the restatement's floor and verdict and --summary the lower median of the floors;
    without them stdout is, byte for byte, the text the tool has always printed for the restatement's records"""
    sy = pkg.synth
    fs, decim, taps, offs, gains = sy.plan("cfg2_64ch", nr_channels=8)
    centre, W = 929500000, 500
    n = decim * 5999 + len(taps)
    iq = sy.synth_iq(n, fs, offs[[1, 5]], seed=4, amplitude=5000.0)
    (tmp_path / "capture.bin").write_bytes(iq.tobytes())
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in taps],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in offs]}))
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    _, fiq = ora.run_channels(iq, cre, cim, incr, decim, want_iq=True)
    plain = tl.restate(pkg, fiq, W, IQ)
    nw = plain.shape[1]
    base = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
            str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "iq", "--window", str(W), "--hang", "1", "--block", "100003", "--summary"]

    def check(stdout, rec, floor):
        """every line is, byte for byte, the tool's text for the restatement's record (the keys in the order the tool has always
        printed them, "floor" and "median_floor" last); records come block by block, so they are matched by (channel, window)"""
        lines = stdout.splitlines()
        recs, sums = lines[:-8], lines[-8:]
        assert len(recs) == rec.size and stdout.endswith("\n")
        want = {}
        for c in range(8):
            for k in range(nw):
                r = rec[c, k]
                ln = {"freq": centre + int(offs[c]), "channel": c, "window": k, "energy": int(r["energy"]),
                      "diff_energy": int(r["diff_energy"]), "peak": int(r["peak"]), "open": int(r["open"])}
                if floor is not None:
                    ln["floor"] = int(floor[c, k])
                want[(c, k)] = json.dumps(ln)
        for text in recs:
            d = json.loads(text)
            assert want.pop((d["channel"], d["window"])) == text
        assert not want
        for c in range(8):
            ow = int(rec["open"][c].sum())
            ln = {"summary": True, "freq": centre + int(offs[c]), "channel": c, "windows": nw, "open_windows": ow, "open_share": ow / nw}
            if floor is not None:
                ln["median_floor"] = sorted(int(v) for v in floor[c])[(nw - 1) // 2]
            assert sums[c] == json.dumps(ln)

    r = subprocess.run(base + ["--floor-windows", "4", "--open-ratio", "1.08", "--close-ratio", "1.03", "--warmup", "2"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the noise channels' windows differ by a few per cent: ratios of 1.08 and 1.03 (276 and 264 in 1/256) open and close on them
    want, want_floor = restate_adaptive(plain, ENERGY, ABOVE, 0, 0, 1, 4, 276, 264, 2)
    check(r.stdout, want, want_floor)
    assert want["open"].any() and not want["open"].all()
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    check(r.stdout, tl.restate(pkg, fiq, W, IQ, sense=ABOVE, hang=1), None)
