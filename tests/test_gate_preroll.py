"""Pre-roll of the squelch gate (mfm_gate_set_preroll, mfm_gate_flush_device, csrc/mfm_gate.hip): with P pre-roll
windows, window k of a channel goes out exactly when any of its records k .. k + P is open, P windows late, and a flush ends
the stream with the P windows still held back.

Every expected value comes from the numpy restatement in this file: dilate the mask, shift by the delay, select as
tests/test_gate.py's restate_call does.  Every comparison is an equality; nothing is compared against the stage itself."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_level as tl

ROOT = tg.ROOT
NEW_NAMES = ["mfm_gate_set_preroll", "mfm_gate_flush_device", "mfm_hosttwin_gate_call_preroll"]
MASKS = tg.MASKS + ["open_at_0"]
PMAX = 63


# ---- the restatement ----------------------------------------------------------------------------------------

def dilate(mask, P):
    """bool [C][K]: window k goes out when any record k .. k + P is open; records at or above K do not exist: closed"""
    out = mask.copy()
    for t in range(1, min(P, mask.shape[1] - 1) + 1):
        out[:, :mask.shape[1] - t] |= mask[:, t:]
    return out


def restate_pre(pkg, stream, mask, W, E, P, pos, nr_in, flush=False):
    """(runs, payload) of the call that takes samples [pos, pos + nr_in), or of the flush at pos"""
    K0, K1 = pos // W, (pos + nr_in) // W
    D = dilate(mask[:, :K1], P)                      # what is known once record K1 - 1 is there
    lo, hi = (max(K1 - P, 0), K1) if flush else (max(K0 - P, 0), K1 - P)
    We = W * E
    runs, pieces, offset = [], [], 0
    for c in range(stream.shape[0]):
        k = lo
        while k < hi:
            if not D[c, k]:
                k += 1
                continue
            e = k
            while e < hi and D[c, e]:
                e += 1
            runs.append((k, offset, c, e - k))
            pieces.append(stream[c, k * We:e * We])
            offset += (e - k) * We
            k = e
    payload = np.concatenate(pieces) if pieces else np.zeros(0, np.int16)
    return np.array(runs, pkg.binding.GATE_RUN_DTYPE), payload


def make_mask(kind, rng, nch, nw):
    if kind == "open_at_0":
        m = np.zeros((nch, nw), bool)
        m[:, 0] = True
        return m
    return tg.make_mask(kind, rng, nch, nw)


def short_cuts(n, W):
    """many calls in a row, each shorter than W (for W = 1 that is no sample at all, every other call): P W is several long"""
    step = max(W // 3, 1)
    out, pos = [], 0
    while pos < n:
        if W == 1:
            out.append(0)
        m = min(step, n - pos)
        out.append(m)
        pos += m
    return out


def drive(pkg, stream, mask, W, E, P, cuts, call, flush, what):
    """feed the cuts through call(pos, rows, records), then flush(pos); every result against the restatement"""
    pos = emitted = 0
    for m in cuts:
        k0, k1 = pos // W, (pos + m) // W
        got = call(pos, stream[:, pos * E:(pos + m) * E], tg.records_of(pkg, mask, k0, k1))
        want = restate_pre(pkg, stream, mask, W, E, P, pos, m)
        tg.same(got, want, f"{what}, call at {pos} of {m}")
        emitted += int(want[0]["nr_windows"].sum())
        pos += m
    assert pos * E == stream.shape[1]
    got = flush(pos)
    want = restate_pre(pkg, stream, mask, W, E, P, pos, 0, flush=True)
    tg.same(got, want, f"{what}, flush at {pos}")
    emitted += int(want[0]["nr_windows"].sum())
    assert emitted == int(dilate(mask[:, :pos // W], P).sum()), what
    return emitted


def twin(pkg, nch, W, E, P):
    """(call, flush) on a fresh host-twin state"""
    b = pkg.binding
    hist = np.zeros((nch, (P + 1) * W * E), np.int16)
    bits = np.zeros(nch, np.uint64)
    none = np.zeros((nch, 0), b.LEVEL_RECORD_DTYPE)

    def call(pos, rows, rec):
        return b.hosttwin_gate_call_preroll(W, E, P, pos, rows, hist, bits, rec)

    def flush(pos):
        return b.hosttwin_gate_call_preroll(W, E, P, pos, np.zeros((nch, 0), np.int16), hist, bits, none, flush=True)

    return call, flush, hist, bits


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_preroll_names(pkg):
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
    assert C.sizeof(b.GateConfig) == 32
    m = re.search(r"#define\s+MFM_GATE_MAX_PREROLL\s+(\d+)u?\b", src)
    assert m and int(m.group(1)) == PMAX == b.MFM_GATE_MAX_PREROLL == pkg.MFM_GATE_MAX_PREROLL <= 63
    assert callable(pkg.Gate.flush_device) and callable(pkg.Gate.set_preroll)


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("W", [1, 2, 7, 8, 511, 4099])
def test_hosttwin_preroll_calls_equal_numpy_restatement(pkg, W, E):
    """csrc/mfm_gate.h through the pre-roll host twin: P 1, 2, 5 and the maximum; 1, 2 and 65 channels; every mask; seeded
    random cuts, and a stream fed in calls shorter than W; a flush ends each"""
    n = tg.stream_len(W)
    for nch in (1, 2, 65):
        rng = np.random.RandomState(2000 * E + 10 * W + nch)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for P in (1, 2, 5, PMAX):
            for kind in MASKS:
                mask = make_mask(kind, rng, nch, n // W)
                for cuts, name in ((tg.make_cuts(rng, n, W, tg.biggest_cut(W)), "seeded"), (short_cuts(n, W), "short")):
                    if name == "short" and (nch == 65 or kind not in ("bernoulli", "single_last", "open_at_0")):
                        continue  # the cut pattern is about the state between calls, not about the channel count
                    if name == "short":
                        assert max(cuts) < max(W, 2) and (W < 7 or P * W >= 3 * max(cuts))
                    call, flush, _, _ = twin(pkg, nch, W, E, P)
                    emitted = drive(pkg, stream, mask, W, E, P, cuts, call, flush, f"W {W} E {E} P {P} channels {nch} mask {kind} {name}")
                    if kind == "closed":
                        assert emitted == 0
                    if kind == "single_last":
                        assert emitted == min(P, (n // W) // 2) + 1
                    if kind == "open_at_0":
                        assert emitted == nch  # nothing exists in front of window 0


@pytest.mark.parametrize("W,E", [(1, 1), (7, 2), (8, 1), (511, 1)])
def test_hosttwin_preroll_zero_is_the_plain_twin_byte_for_byte(pkg, W, E):
    b = pkg.binding
    n, nch = tg.stream_len(W), 3
    rng = np.random.RandomState(77 + W)
    stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
    for kind in tg.MASKS:
        mask = tg.make_mask(kind, rng, nch, n // W)
        call, flush, hist, bits = twin(pkg, nch, W, E, 0)
        carry = np.zeros((nch, W * E), np.int16)
        pos = 0
        for m in tg.make_cuts(rng, n, W, tg.biggest_cut(W)):
            rows, rec = stream[:, pos * E:(pos + m) * E], tg.records_of(pkg, mask, pos // W, (pos + m) // W)
            got, want = call(pos, rows, rec), b.hosttwin_gate_call(W, E, pos, rows, carry, rec)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (kind, pos)
            pos += m
            r = (pos % W) * E
            assert hist[:, :r].tobytes() == carry[:, :r].tobytes() and not bits.any()
        runs, payload = flush(pos)
        assert runs.size == 0 and payload.size == 0


@pytest.mark.parametrize("P", [1, 3])
def test_hosttwin_dilation_across_chunks_of_64_records(pkg, P):
    """200 windows in one call, W = 2: openings at 63, 64, 65, 127 + P and 199.  The pre-roll windows of 63 and of 127 + P lie
    on either side of a chunk edge of 64, those of 199 on either side of the call's end (the flush brings the rest)"""
    W, E, nch, nw = 2, 1, 2, 200
    rng = np.random.RandomState(9)
    stream = rng.randint(-32768, 32768, size=(nch, nw * W)).astype(np.int16)
    mask = np.zeros((nch, nw), bool)
    mask[1, [63, 64, 65, 127 + P, 199]] = True
    call, flush, _, _ = twin(pkg, nch, W, E, P)
    got = call(0, stream, tg.records_of(pkg, mask, 0, nw))
    tg.same(got, restate_pre(pkg, stream, mask, W, E, P, 0, nw * W), "200 windows")
    end = flush(nw * W)
    tg.same(end, restate_pre(pkg, stream, mask, W, E, P, nw * W, 0, flush=True), "flush")
    lengths = [int(x) for x in got[0]["nr_windows"]], [int(x) for x in end[0]["nr_windows"]]
    firsts = [int(x) for x in got[0]["first_window"]], [int(x) for x in end[0]["first_window"]]
    if P == 1:
        assert lengths == ([4, 2, 1], [1]) and firsts == ([62, 127, 198], [199])
    else:
        assert lengths == ([6, 4, 1], [3]) and firsts == ([60, 127, 196], [197])
    assert set(got[0]["channel"]) == {1}


def test_hosttwin_preroll_refuses_and_leaves_its_state(pkg):
    b = pkg.binding
    W, E, nch, stream, mask = tg._crossing_case(pkg)
    P = 1
    call, flush, hist, bits = twin(pkg, nch, W, E, P)
    first = call(0, stream[:, :12], tg.records_of(pkg, mask, 0, 2))
    tg.same(first, restate_pre(pkg, stream, mask, W, E, P, 0, 12), "first call")
    assert hist.any() and bits.tolist() == [0, 1, 0]  # record 1 of channel 1 is open
    h0, b0 = hist.copy(), bits.copy()
    with pytest.raises(pkg.MfmError) as ei:  # 13 samples from 12 complete three windows, not two
        call(12, stream[:, 12:], tg.records_of(pkg, mask, 2, 4))
    assert ei.value.code == b.MFM_E_INVAL
    rec = tg.records_of(pkg, mask, 2, 5)
    rec["window"][2, 1] += 1
    with pytest.raises(pkg.MfmError) as ei:
        call(12, stream[:, 12:], rec)
    assert ei.value.code == b.MFM_E_STATE and "out of step" in str(ei.value)
    want = restate_pre(pkg, stream, mask, W, E, P, 12, 13)
    assert len(want[0]) == 2 and want[1].size == 3 * W   # windows 1 and 2 of channel 1; window 3 of channel 2, in front of 4
    for kw in (dict(max_runs=1), dict(max_elems=3 * W - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_gate_call_preroll(W, E, P, 12, stream[:, 12:], hist, bits, tg.records_of(pkg, mask, 2, 5), **kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (2, 3 * W)
    with pytest.raises(pkg.MfmError) as ei:  # a flush takes no samples
        b.hosttwin_gate_call_preroll(W, E, P, 12, stream[:, 12:], hist, bits, np.zeros((nch, 0), b.LEVEL_RECORD_DTYPE), flush=True)
    assert ei.value.code == b.MFM_E_INVAL
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_gate_call_preroll(W, E, PMAX + 1, 0, stream[:, :0], np.zeros((nch, (PMAX + 2) * W), np.int16), bits,
                                     np.zeros((nch, 0), b.LEVEL_RECORD_DTYPE))
    assert ei.value.code == b.MFM_E_INVAL
    assert np.array_equal(hist, h0) and np.array_equal(bits, b0)  # a refused call changes nothing
    tg.same(call(12, stream[:, 12:], tg.records_of(pkg, mask, 2, 5)), want, "second call")
    tg.same(flush(25), restate_pre(pkg, stream, mask, W, E, P, 25, 0, flush=True), "flush")


def test_preroll_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_gate.o (tools/kernel_regs.py), which holds the gate's one set of kernels, pre-roll
    or not: exactly these five, no private segment, no spilled register"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_gate.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_gate.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert sorted(ln.split()[0] for ln in lines) == ["gt_copy_kernel", "gt_count_kernel", "gt_hist_kernel", "gt_runs_kernel",
                                                     "gt_scan_kernel"], out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# the scene: a carrier that comes up late in a window, so that the squelch opens one window late

SCENE = dict(nr_channels=8, channel=5, W=500, nr_out=6000, window=4, late=25, amplitude=900.0, noise=512, seed=5)
_SCENE = {}


def _scene(pkg, ora):
    if not _SCENE:
        _SCENE["it"] = _make_scene(pkg, ora)
    return _SCENE["it"]


def _make_scene(pkg, ora):
    """8 channels of the 64-channel plan, noise everywhere, and on channel 5 a carrier whose first sample is output sample
    first = 4 W + W - 25 of that channel: the last twentieth of window 4"""
    sy, s = pkg.synth, SCENE
    fs, decim, taps, offs, gains = sy.plan("cfg2_64ch", nr_channels=s["nr_channels"])
    W = s["W"]
    n = decim * (s["nr_out"] - 1) + len(taps)
    first = s["window"] * W + W - s["late"]
    iq = sy.synth_iq(n, fs, [], seed=s["seed"], noise=s["noise"]).astype(np.int32)
    burst = sy.synth_iq(n, fs, offs[[s["channel"]]], seed=s["seed"], amplitude=s["amplitude"], noise=0).astype(np.int32)
    burst[:decim * first + len(taps) - 1] = 0   # output sample i is the filter over inputs decim i .. decim i + taps - 1
    iq = np.clip(iq + burst, -32768, 32767).astype(np.int16)
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm, fiq = ora.run_channels(iq, cre, cim, incr, decim, want_iq=True)
    assert pcm.shape == (s["nr_channels"], s["nr_out"])
    e = tl.restate(pkg, fiq, W, tl.IQ)["energy"].astype(np.float64)
    on = np.zeros(e.shape, bool)
    on[s["channel"], s["window"] + 1:] = True           # the windows the carrier fills
    idle = ~on
    idle[s["channel"], s["window"]] = False             # the window it begins in belongs to neither group
    margin = e[on].min() / e[idle].max()
    thr = int(np.sqrt(e[on].min() * e[idle].max()))     # the geometric mean between the groups, as tests/test_gate.py's scene
    want = tl.restate(pkg, fiq, W, tl.IQ, sense=tl.ABOVE, open_thr=thr, close_thr=thr, hang=1)
    return dict(plan=(fs, decim, taps, offs, gains), iq=iq, pcm=pcm, fiq=fiq, W=W, first=first, thr=thr, margin=margin, records=want,
                mask=want["open"].astype(bool), energy=e)


def _covered(runs, W, c):
    out = set()
    for r in runs:
        if int(r["channel"]) == c:
            out.update(range(int(r["first_window"]) * W, (int(r["first_window"]) + int(r["nr_windows"])) * W))
    return out


def test_scene_on_the_oracle_loses_the_bursts_first_sample_without_preroll_and_keeps_it_with(pkg, ora):
    """why pre-roll exists.  The oracle's filtered IQ of a carrier that comes up in the last twentieth of window 4: the squelch
    (threshold at the geometric mean of carrier and idle window energies) leaves window 4 closed and opens window 5, the plain
    gate's payload begins at sample 5 W and misses the burst's first sample, the gate with P = 1 has it"""
    sc = _scene(pkg, ora)
    s, W, mask, first = SCENE, sc["W"], sc["mask"], sc["first"]
    c, k = s["channel"], s["window"]
    print(f"margin {sc['margin']:.1f}x, energy of window {k}: {sc['energy'][c, k]:.3g}, threshold {sc['thr']:.3g}")
    assert sc["margin"] >= 2.0
    assert k * W + 3 * W // 4 <= first < (k + 1) * W           # the last quarter of window k
    assert not mask[c, :k + 1].any() and mask[c, k + 1:].all()  # window k stays closed, k + 1 opens
    assert not np.delete(mask, c, axis=0).any()
    nch, n = sc["pcm"].shape
    rec = sc["records"]
    got = {}
    for P in (0, 1):
        call, flush, _, _ = twin(pkg, nch, W, 1, P)
        runs = [call(0, sc["pcm"], rec)[0], flush(n)[0]]
        got[P] = _covered(np.concatenate(runs), W, c)
    assert first not in got[0] and min(got[0]) == (k + 1) * W
    assert first in got[1] and min(got[1]) == k * W


# ---- GPU ------------------------------------------------------------------------------------------------------

def _host_gate(pkg, nch, cap, W, E, P, **kw):
    gate = pkg.Gate(nch, cap, W, elems_per_sample=E, preroll_windows=P, **kw)

    def flush(pos):
        gate.flush_device()
        return gate.fetch()

    return gate, (lambda pos, rows, rec: gate.process_host(rows, rec)), flush


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("W", [1, 7, 8, 512, 4099])
def test_gpu_process_host_with_preroll_equals_numpy_restatement(pkg, W, E):
    n = tg.stream_len(W)
    for nch in (3, 65):
        rng = np.random.RandomState(3000 * E + 10 * W + nch)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for P in (1, 3):
            for kind in ("bernoulli", "single_last", "open_at_0", "open"):
                mask = make_mask(kind, rng, nch, n // W)
                for cuts, name in ((tg.make_cuts(rng, n, W, tg.biggest_cut(W)), "seeded"), (short_cuts(n, W), "short")):
                    if name == "short" and (nch == 65 or kind != "bernoulli"):
                        continue  # calls shorter than W: once per (W, E, P)
                    gate, call, flush = _host_gate(pkg, nch, tg.biggest_cut(W), W, E, P)
                    drive(pkg, stream, mask, W, E, P, cuts, call, flush, f"W {W} E {E} P {P} channels {nch} mask {kind}")
                    gate.close()


def _device_calls(pkg, torch, stream, mask, W, E, P, cuts, in_stride, lead, what, cap, **kw):
    d, ptr = tg._to_device(torch, stream, in_stride, lead)
    gate = pkg.Gate(stream.shape[0], cap, W, elems_per_sample=E, preroll_windows=P, **kw)
    keep = []

    def call(pos, rows, rec):
        d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy() if rec.size else np.zeros(8, np.uint8)).cuda()
        keep.append(d_rec)
        gate.process_device(ptr + 2 * E * pos, in_stride, rows.shape[1] // E, d_rec.data_ptr(), rec.shape[1], rec.shape[1])
        return gate.fetch()

    def flush(pos):
        gate.flush_device()
        return gate.fetch()

    drive(pkg, stream, mask, W, E, P, cuts, call, flush, what)
    gate.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [13, 4099])
def test_gpu_process_device_with_preroll_at_every_alignment(pkg, W):
    """rows at offsets of 0 .. 7 elements with an odd stride, P = 2, calls of about 1.5 W (every window they emit lies in the
    history), 3.5 W (one across the seam) and 5 W (some in the rows): history-sourced pieces meet the 16-byte path at all eight
    relative alignments"""
    import torch
    E, P, nch = 1, 2, 3
    cuts = [W + W // 2, 3 * W + W // 2 + 1, W + W // 2 - 3, 5 * W + 3, 2, W + W // 2, W - 1, 3 * W + 5]
    n = sum(cuts)
    in_stride = n + 1 + n % 2
    assert in_stride % 2 == 1
    for lead in range(8):
        rng = np.random.RandomState(W * 7 + lead)
        stream = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
        for kind in ("open", "bernoulli"):
            mask = make_mask(kind, rng, nch, n // W)
            _device_calls(pkg, torch, stream, mask, W, E, P, cuts, in_stride, lead, f"W {W} lead {lead} mask {kind}", max(cuts))


@pytest.mark.gpu
def test_gpu_wide_copy_path_reads_a_window_of_two_pieces_from_the_history(pkg):
    """W E = 10 000 elements: two pieces per window.  P = 1 and an opening at window 2, right behind the edge of a call that ended
    at 2 W: window 1 goes out with the second call and lies wholly in the history"""
    import torch
    W, E, P, nch = 5000, 2, 1, 3
    cuts = [2 * W, 2 * W + 7, W]
    n = sum(cuts)
    rng = np.random.RandomState(51)
    stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
    mask = np.zeros((nch, n // W), bool)
    mask[1, 2] = mask[2, 2:] = True
    for lead, pad in ((0, 8), (3, 1)):
        _device_calls(pkg, torch, stream, mask, W, E, P, cuts, n * E + pad, lead, f"wide lead {lead}", max(cuts))


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [257, 1025])
def test_gpu_channel_scan_edges_with_preroll(pkg, nch):
    import torch
    for W, E in ((5, 1), (8, 2)):
        n = 4 * W + 5
        rng = np.random.RandomState(nch + W)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for kind in ("bernoulli", "single_last"):
            mask = make_mask(kind, rng, nch, n // W)
            _device_calls(pkg, torch, stream, mask, W, E, 1, [W + 2, n - W - 2], n * E + 1, 1, f"channels {nch} W {W} mask {kind}", n)


@pytest.mark.gpu
def test_gpu_overflow_with_preroll_and_the_call_after(pkg):
    """every channel opens at window 3 alone: 4 open windows without pre-roll, with P = 2 the first call (records 0 .. 4) emits
    windows 1 and 2 of each, 8 windows, into a payload of 7"""
    b = pkg.binding
    W, nch, n, P = 6, 4, 60, 2
    rng = np.random.RandomState(22)
    stream = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
    mask = np.zeros((nch, 10), bool)
    mask[:, 3] = True
    gate, call, flush = _host_gate(pkg, nch, 64, W, 1, P, max_open_windows=7)
    with pytest.raises(pkg.MfmError) as ei:
        call(0, stream[:, :31], tg.records_of(pkg, mask, 0, 5))
    assert ei.value.code == b.MFM_E_STATE and "max_open_windows" in str(ei.value)
    assert not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
    d_payload = gate.device_view()[1]
    want = restate_pre(pkg, stream, mask, W, 1, P, 31, 29)
    assert want[1].size == 4 * W
    tg.same(call(31, stream[:, 31:], tg.records_of(pkg, mask, 5, 10)), want, "the call after an overflow")
    tg.same(flush(60), restate_pre(pkg, stream, mask, W, 1, P, 60, 0, flush=True), "flush")
    assert d_payload == gate.device_view()[1]  # a caller-chosen capacity is not regrown
    gate.close()


@pytest.mark.gpu
def test_gpu_preroll_zero_and_a_flush_are_the_plain_gate(pkg):
    b = pkg.binding
    W, E, nch, stream, mask = tg._crossing_case(pkg)
    gate = pkg.Gate(nch, 16, W)
    gate.set_preroll(0)
    first = gate.process_host(stream[:, :12], tg.records_of(pkg, mask, 0, 2))
    second = gate.process_host(stream[:, 12:], tg.records_of(pkg, mask, 2, 5))
    tg._check_crossing(pkg, stream, mask, first, second)
    gate.flush_device()
    runs, payload = gate.fetch()
    assert runs.size == 0 and payload.size == 0
    for again in (lambda: gate.process_host(stream[:, :0], tg.records_of(pkg, mask, 5, 5)), gate.flush_device):
        with pytest.raises(pkg.MfmError) as ei:
            again()
        assert ei.value.code == b.MFM_E_STATE
    gate.close()


@pytest.mark.gpu
def test_gpu_setter_back_to_zero_is_the_plain_gate(pkg):
    """set_preroll(2), then set_preroll(0): the history is sized for P = 0 again.  The crossing case, then windows of two pieces
    with calls that begin deep in the unfinished window (tg._history_case); each ends in a flush that returns nothing"""
    W, E, nch, stream, mask = tg._crossing_case(pkg)
    gate = pkg.Gate(nch, 16, W)
    gate.set_preroll(2)
    gate.set_preroll(0)
    first = gate.process_host(stream[:, :12], tg.records_of(pkg, mask, 0, 2))
    second = gate.process_host(stream[:, 12:], tg.records_of(pkg, mask, 2, 5))
    tg._check_crossing(pkg, stream, mask, first, second)
    gate.flush_device()
    runs, payload = gate.fetch()
    assert runs.size == 0 and payload.size == 0
    gate.close()
    W, E, nch, stream, cuts, masks = tg._history_case(pkg)
    for kind, mask in masks.items():
        gate = pkg.Gate(nch, max(cuts), W, elems_per_sample=E)
        gate.set_preroll(2)
        gate.set_preroll(0)
        tg.drive(pkg, stream, mask, W, E, cuts, lambda pos, rows, rec: gate.process_host(rows, rec), f"back to zero, mask {kind}")
        gate.flush_device()
        runs, payload = gate.fetch()
        assert runs.size == 0 and payload.size == 0
        gate.close()


@pytest.mark.gpu
def test_gpu_setter_and_flush_refusals(pkg):
    b = pkg.binding
    W, E, nch, stream, mask = tg._crossing_case(pkg)
    gate = pkg.Gate(nch, 16, W)
    with pytest.raises(pkg.MfmError) as ei:
        gate.set_preroll(PMAX + 1)
    assert ei.value.code == b.MFM_E_INVAL and str(PMAX) in str(ei.value)
    gate.set_preroll(2)
    gate.set_preroll(1)  # still before the first call
    gate.process_host(stream[:, :12], tg.records_of(pkg, mask, 0, 2))
    with pytest.raises(pkg.MfmError) as ei:
        gate.set_preroll(1)
    assert ei.value.code == b.MFM_E_STATE
    tg.same(gate.process_host(stream[:, 12:], tg.records_of(pkg, mask, 2, 5)), restate_pre(pkg, stream, mask, W, E, 1, 12, 13), "second call")
    gate.flush_device()
    tg.same(gate.fetch(), restate_pre(pkg, stream, mask, W, E, 1, 25, 0, flush=True), "flush")
    for again in (lambda: gate.process_host(stream[:, :0], tg.records_of(pkg, mask, 5, 5)), gate.flush_device):
        with pytest.raises(pkg.MfmError) as ei:
            again()
        assert ei.value.code == b.MFM_E_STATE
    gate.close()
    # 16 channels of 64 windows of 2^20 elements: 2^31 bytes of history, the bound is 2^30
    gate = pkg.Gate(16, 64, 1 << 19, elems_per_sample=2)
    with pytest.raises(pkg.MfmError) as ei:
        gate.set_preroll(PMAX)
    assert ei.value.code == b.MFM_E_INVAL and str(b.MFM_GATE_MAX_HISTORY_BYTES) in str(ei.value)
    gate.close()


@pytest.mark.gpu
def test_gpu_engine_level_gate_with_preroll_on_device_equals_selection_of_the_oracle(pkg, ora):
    """the scene through engine -> level (IQ form) -> gate with P = 1 on the PCM rows, all on the engine's stream: every call and
    the flush equal the restatement's selection of the oracle's PCM, and the payload has the burst's first sample"""
    b = pkg.binding
    sc = _scene(pkg, ora)
    (fs, decim, taps, offs, gains), iq, pcm, W, mask, P = sc["plan"], sc["iq"], sc["pcm"], sc["W"], sc["mask"], 1
    nch = pcm.shape[0]
    blk = 100003
    eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g), want_iq=True)
    eng.commit()
    cap = blk // decim + 8
    lv = pkg.Level(nch, cap, W, form=b.MFM_LEVEL_IQ, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=sc["thr"], close_thr=sc["thr"], hang_windows=1)
    gate = pkg.Gate(nch, cap, W, elems_per_sample=1, preroll_windows=P)
    pos, all_runs = 0, []
    for s in range(0, iq.shape[0], blk):
        assert eng.push(iq[s:s + blk]) == 0
        d_pcm, stride, nout, d_iq = eng.last_output_device()
        lv.process_device(d_iq, 2 * stride, nout, stream=eng.stream)
        d_rec, rec_stride, nw, _ = lv.device_view()
        gate.process_device(d_pcm, stride, nout, d_rec, rec_stride, nw, stream=eng.stream)
        got = gate.fetch()
        tg.same(got, restate_pre(pkg, pcm, mask, W, 1, P, pos, nout), f"block at {pos}")
        all_runs.append(got[0])
        pos += nout
    assert pos == pcm.shape[1]
    gate.flush_device(stream=eng.stream)
    got = gate.fetch()
    tg.same(got, restate_pre(pkg, pcm, mask, W, 1, P, pos, 0, flush=True), "flush")
    all_runs.append(got[0])
    covered = _covered(np.concatenate(all_runs), W, SCENE["channel"])
    assert sc["first"] in covered and len(covered) == int(dilate(mask, P).sum()) * W
    for o in (gate, lv, eng):
        o.close()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_preroll_writes_the_selection_flush_included(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-out DIR --gate-preroll 1 on the scene: each chNNNN.s16 is the dilated mask's selection of the
    oracle's rows, the windows the flush brought included, and index.jsonl keeps its fields"""
    sc = _scene(pkg, ora)
    (fs, decim, taps, offs, gains), W, mask = sc["plan"], sc["W"], sc["mask"]
    centre = 929500000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in taps],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in offs]}))
    flat = np.ascontiguousarray(sc["fiq"]).reshape(mask.shape[0], -1)
    D = dilate(mask, 1)
    assert D[SCENE["channel"], -1] and D.sum() == mask.sum() + 1
    cmd = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
           str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "iq", "--window", str(W), "--open-thr", str(sc["thr"]),
           "--hang", "1", "--block", "100003", "--gate-out", str(tmp_path / "gated"), "--gate-preroll", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    index = [json.loads(ln) for ln in (tmp_path / "gated" / "index.jsonl").read_text().splitlines()]
    seen = np.zeros(D.shape, bool)
    at = {}
    for ln in index:
        assert sorted(ln) == ["channel", "file_offset", "first_sample", "nr_samples"]
        c = ln["channel"]
        assert ln["file_offset"] == at.get(c, 0) and ln["first_sample"] % W == 0 and ln["nr_samples"] % W == 0 and ln["nr_samples"] > 0
        k0, k1 = ln["first_sample"] // W, (ln["first_sample"] + ln["nr_samples"]) // W
        assert not seen[c, k0:k1].any()
        seen[c, k0:k1] = True
        at[c] = at.get(c, 0) + 4 * ln["nr_samples"]
    assert np.array_equal(seen, D)
    for c in range(D.shape[0]):
        path = tmp_path / "gated" / f"ch{c:04d}.s16"
        assert path.exists() == bool(D[c].any())
        if D[c].any():
            sel = np.concatenate([flat[c, k * W * 2:(k + 1) * W * 2] for k in np.flatnonzero(D[c])])
            assert np.array_equal(np.fromfile(path, np.int16), sel), c
