"""The level / squelch stage (mfm_level_*, csrc/mfm_level.hip): per channel and window of W samples the exact integer
sums energy, diff_energy (of the difference wrapped to 16 bits) and peak, and a squelch stepped once per window.

Every expected value comes from the numpy / plain-Python restatement in this file (int64 arithmetic, astype(np.int16)
for the wrapped difference, a hand-written state machine), for the end-to-end test run on the ORACLE's PCM and filtered
IQ; every comparison is exact equality of every record field."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["mfm_level_create", "mfm_level_destroy", "mfm_level_process_device", "mfm_level_process_host", "mfm_level_fetch",
             "mfm_level_device_view", "mfm_hosttwin_level_window", "mfm_hosttwin_squelch_step"]
PCM, IQ = 0, 1
ENERGY, DIFF = 0, 1
ABOVE, BELOW = 0, 1


# ---- the restatement ----------------------------------------------------------------------------------------

def window_sums(x, form, prev=0):
    """(energy, diff_energy, peak) of one window: x int16 [n] (PCM) or [n][2] (IQ)"""
    x = np.asarray(x, np.int16)
    v = x.astype(np.int64)
    energy = int((v * v).sum())
    peak = int(np.abs(v).max()) if v.size else 0
    if form == IQ:
        return energy, 0, peak
    before = np.concatenate([np.array([prev], np.int16), x[:-1]]) if x.size else x
    d = (x.astype(np.int32) - before.astype(np.int32)).astype(np.int16).astype(np.int64)
    return energy, int((d * d).sum()), peak


def squelch_step(open_, bad, sense, open_thr, close_thr, hang, metric):
    if not open_:
        if (metric <= open_thr) if sense == BELOW else (metric >= open_thr):
            return 1, 0
        return 0, bad
    if (metric > close_thr) if sense == BELOW else (metric < close_thr):
        bad += 1
        return (0, 0) if bad > hang else (1, bad)
    return 1, 0


def squelch_run(metrics, sense, open_thr, close_thr, hang):
    open_, bad, out = 0, 0, []
    for m in metrics:
        open_, bad = squelch_step(open_, bad, sense, open_thr, close_thr, hang, int(m))
        out.append(open_)
    return out


def restate(pkg, rows, W, form, metric=ENERGY, sense=ABOVE, open_thr=0, close_thr=0, hang=0):
    """records [C][n // W] of a whole stream: rows int16 [C][n] (PCM) or [C][n][2] (IQ)"""
    rows = np.asarray(rows, np.int16)
    nch, n = rows.shape[0], rows.shape[1]
    nw = n // W
    rec = np.zeros((nch, nw), pkg.binding.LEVEL_RECORD_DTYPE)
    for c0 in range(0, nch, 32):
        x = rows[c0:c0 + 32, :nw * W]
        v = x.astype(np.int64)
        if form == IQ:
            sq, ab = (v * v).sum(axis=2), np.abs(v).max(axis=2)
            dsq = np.zeros_like(sq)
        else:
            before = np.concatenate([np.zeros((x.shape[0], 1), np.int16), x[:, :-1]], axis=1)
            d = (x.astype(np.int32) - before.astype(np.int32)).astype(np.int16).astype(np.int64)
            sq, ab, dsq = v * v, np.abs(v), d * d
        k = x.shape[0]
        rec["energy"][c0:c0 + k] = sq.reshape(k, nw, W).sum(axis=2).astype(np.uint64)
        rec["diff_energy"][c0:c0 + k] = dsq.reshape(k, nw, W).sum(axis=2).astype(np.uint64)
        rec["peak"][c0:c0 + k] = ab.reshape(k, nw, W).max(axis=2).astype(np.uint32) if nw else 0
    rec["window"] = np.arange(nw, dtype=np.uint64)[None, :]
    rec["channel"] = np.arange(nch, dtype=np.uint32)[:, None]
    for c in range(nch):
        m = rec["diff_energy" if metric == DIFF else "energy"][c]
        rec["open"][c] = squelch_run(m, sense, open_thr, close_thr, hang)
    return rec


def same_records(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, f"{what}: field {f} differs at (channel, window) {bad[:5].tolist()}: " \
                              f"{got[f][tuple(bad[0])]} != {want[f][tuple(bad[0])]}"


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_level_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in pkg.binding.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src)
    for name, val in (("MFM_LEVEL_PCM", 0), ("MFM_LEVEL_IQ", 1), ("MFM_LEVEL_METRIC_ENERGY", 0), ("MFM_LEVEL_METRIC_DIFF", 1),
                      ("MFM_LEVEL_OPEN_ABOVE", 0), ("MFM_LEVEL_OPEN_BELOW", 1)):
        assert re.search(r"#define\s+%s\s+%du" % (name, val), src), name
        assert getattr(pkg.binding, name) == val
    b = pkg.binding
    assert C.sizeof(b.LevelRecord) == b.LEVEL_RECORD_DTYPE.itemsize == 40
    assert pkg.LEVEL_RECORD_DTYPE is b.LEVEL_RECORD_DTYPE and C.sizeof(pkg.LevelConfig) == 56
    # the struct in the header, field by field, in the order of the dtype
    m = re.search(r"struct mfm_level_record \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [
        ("uint64_t", "energy"), ("uint64_t", "diff_energy"), ("uint64_t", "window"), ("uint32_t", "peak"), ("uint32_t", "channel"),
        ("uint32_t", "open"), ("uint32_t", "reserved")]
    assert list(b.LEVEL_RECORD_DTYPE.names) == ["energy", "diff_energy", "window", "peak", "channel", "open", "reserved"]


def _patterns(rng, n):
    alt = np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    return {"random": rng.randint(-32768, 32768, n).astype(np.int16), "min": np.full(n, -32768, np.int16),
            "max": np.full(n, 32767, np.int16), "alternating": alt, "alternating2": (-1 - alt.astype(np.int32)).astype(np.int16),
            "zeros": np.zeros(n, np.int16)}


@pytest.mark.parametrize("form", [PCM, IQ])
def test_hosttwin_window_equals_numpy_restatement(pkg, form):
    """csrc/mfm_level.h through its host twin: random rows, all -32768 (a pair of squares sums to 2^31), all 32767,
    alternating -32768 / 32767 both ways, zeros; lengths around the 8-element groups of a 16-byte load; every previous
    sample that matters"""
    rng = np.random.RandomState(5 + form)
    for n in (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 1000, 4097):
        for name, x in _patterns(rng, n * (2 if form == IQ else 1)).items():
            for prev in (0, -32768, 32767, int(rng.randint(-32768, 32768))):
                xs = x.reshape(-1, 2) if form == IQ else x
                want = window_sums(xs, form, prev)
                got = pkg.binding.hosttwin_level_window(xs, form, prev)
                assert got == want, (name, n, prev, got, want)
    e, d, p = pkg.binding.hosttwin_level_window(np.full(4096, -32768, np.int16), PCM, 0)
    assert (e, d, p) == (4096 << 30, 1 << 30, 32768)
    e, d, p = pkg.binding.hosttwin_level_window(np.full((4096, 2), -32768, np.int16), IQ, 0)
    assert (e, d, p) == (8192 << 30, 0, 32768)


def test_hosttwin_window_reads_rows_at_any_alignment(pkg):
    rng = np.random.RandomState(2)
    base = rng.randint(-32768, 32768, 300).astype(np.int16)
    for off in range(9):
        x = base[off:off + 200]
        assert pkg.binding.hosttwin_level_window(x, PCM, int(base[off - 1]) if off else 0) == \
            window_sums(x, PCM, int(base[off - 1]) if off else 0)


@pytest.mark.parametrize("sense", [ABOVE, BELOW])
@pytest.mark.parametrize("hang", [0, 1, 5])
def test_hosttwin_squelch_equals_python_state_machine(pkg, sense, hang):
    rng = np.random.RandomState(10 * hang + sense)
    opened = closed = 0
    for trial in range(20):
        lo, hi = int(rng.randint(300, 500)), int(rng.randint(500, 700))
        open_thr, close_thr = (hi, lo) if sense == ABOVE else (lo, hi)
        metrics = rng.randint(0, 1000, 400)
        if trial % 4 == 0:  # runs on either side, so that the hang count is reached and reset
            metrics = np.repeat(rng.randint(0, 1000, 100), rng.randint(1, 9, 100))[:400]
        want = squelch_run(metrics, sense, open_thr, close_thr, hang)
        open_, bad, got = 0, 0, []
        for m in metrics:
            open_, bad = pkg.binding.hosttwin_squelch_step(sense, open_thr, close_thr, hang, int(m), open_, bad)
            got.append(open_)
        assert got == want, (trial, open_thr, close_thr)
        steps = np.diff(np.array([0] + want))
        opened += int((steps == 1).sum())
        closed += int((steps == -1).sum())
    assert opened >= 20 and closed >= 20  # the sequences exercise both transitions


def test_hosttwin_squelch_on_the_thresholds(pkg):
    """hand-made sequences that sit exactly on open_thr and close_thr"""
    step = pkg.binding.hosttwin_squelch_step

    def run(sense, open_thr, close_thr, hang, metrics):
        o, b, out = 0, 0, []
        for m in metrics:
            o, b = step(sense, open_thr, close_thr, hang, m, o, b)
            out.append(o)
        assert out == squelch_run(metrics, sense, open_thr, close_thr, hang)
        return out

    # ABOVE, open at >= 100, bad at < 50
    assert run(ABOVE, 100, 50, 0, [99, 100, 50, 49, 99, 100]) == [0, 1, 1, 0, 0, 1]
    assert run(ABOVE, 100, 50, 1, [100, 49, 50, 49, 49, 100]) == [1, 1, 1, 1, 0, 1]
    assert run(ABOVE, 100, 50, 5, [100] + [49] * 5 + [50] + [49] * 6 + [49]) == [1] * 12 + [0, 0]
    assert run(ABOVE, 100, 100, 0, [100, 100, 99, 100]) == [1, 1, 0, 1]
    # BELOW, open at <= 50, bad at > 100
    assert run(BELOW, 50, 100, 0, [51, 50, 100, 101, 51, 50]) == [0, 1, 1, 0, 0, 1]
    assert run(BELOW, 50, 100, 1, [50, 101, 100, 101, 101, 50]) == [1, 1, 1, 1, 0, 1]
    assert run(BELOW, 50, 50, 0, [50, 51, 50]) == [1, 0, 1]
    # the full range of the metric
    big = (1 << 64) - 1
    assert run(ABOVE, big, big, 0, [big - 1, big, big - 1]) == [0, 1, 0]
    assert run(BELOW, 0, 0, 0, [1, 0, 1]) == [0, 1, 0]


def test_create_refuses_bad_configurations(pkg):
    """argument checks come before the device is touched: MFM_E_INVAL with or without a GPU"""
    b = pkg.binding
    good = dict(nr_channels=2, max_in_samples=4096, window_samples=64)

    def refused(**kw):
        with pytest.raises(pkg.MfmError) as ei:
            pkg.Level(**dict(good, **kw))
        assert ei.value.code == b.MFM_E_INVAL, kw

    refused(abi_version=b.MFM_ABI_VERSION + 1)
    refused(abi_version=0)
    refused(window_samples=0)
    refused(nr_channels=0)
    refused(max_in_samples=0)
    refused(form=2)
    refused(metric=2)
    refused(sense=2)
    refused(form=IQ, metric=DIFF)
    refused(sense=ABOVE, open_thr=10, close_thr=11)
    refused(sense=BELOW, open_thr=11, close_thr=10)
    lib = pkg.load_library()
    with pytest.raises(pkg.MfmError):
        pkg.Level(sense=BELOW, open_thr=11, close_thr=10, **good)
    assert b"close_thr" in lib.mfm_last_error()
    # ... and the same thresholds the right way round pass the checks (then need a device)
    import torch
    for kw in (dict(sense=ABOVE, open_thr=11, close_thr=10), dict(sense=BELOW, open_thr=10, close_thr=11), dict(open_thr=7, close_thr=7)):
        try:
            pkg.Level(**dict(good, **kw)).close()
            assert torch.cuda.is_available()
        except pkg.MfmError as e:
            assert e.code == b.MFM_E_DEVICE and not torch.cuda.is_available()


def test_level_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_level.o (tools/kernel_regs.py), as tests/test_abi.py reads them for the channel
    kernels: three kernels, no private segment, no spilled register"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_level.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_level.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert len(lines) == 3, out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- GPU ------------------------------------------------------------------------------------------------------

def _rows(rng, nch, n, form):
    shape = (nch, n, 2) if form == IQ else (nch, n)
    x = rng.randint(-32768, 32768, size=shape).astype(np.int16)
    pats = [-32768, None, 32767, 0]  # full-scale rows, the alternating row, a silent one
    for c, p in enumerate(pats):
        if nch >= 3 and c < nch:
            if p is None:
                flat = x[c].reshape(-1)
                flat[:] = np.where(np.arange(flat.size) % 2 == 0, -32768, 32767)
            else:
                x[c] = p
    return x


def _on_device(torch, x, in_stride, lead):
    """rows of x (flattened to elements) laid out [channel][in_stride] behind `lead` elements; returns (tensor, address of row 0)"""
    nch = x.shape[0]
    flat = np.ascontiguousarray(x).reshape(nch, -1)
    host = np.full(lead + nch * in_stride + 8, 0x5555, np.int16)
    view = host[lead:lead + nch * in_stride].reshape(nch, in_stride)
    view[:, :flat.shape[1]] = flat
    d = torch.from_numpy(host).cuda()
    return d, d.data_ptr() + 2 * lead


def _n_for(W, nch):
    if nch <= 64:
        return 3 * W + 17 if W >= 1000 else 20000 + W
    return (2 * W + 100 if W == 4096 else W + 100) if W >= 4096 else 3000 + W


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 7, 64, 1000, 4096, 65536])
@pytest.mark.parametrize("form", [PCM, IQ])
def test_gpu_records_equal_restatement(pkg, form, W):
    """1, 3, 64 and 1024 channels; an odd in_stride and a row pointer offset by an odd number of samples; rows of -32768, of
    32767, alternating and silent among random ones; the squelch on the median window energy"""
    import torch
    for nch in (1, 3, 64, 1024):
        n = _n_for(W, nch)
        rng = np.random.RandomState(W + 7 * nch + form)
        x = _rows(rng, nch, n, form)
        elems = n * (2 if form == IQ else 1)
        in_stride, lead = elems + 1 + (elems % 2), 3
        assert in_stride % 2 == 1
        plain = restate(pkg, x, W, form)
        thr = int(np.median(plain["energy"]))
        kw = dict(metric=DIFF if (form == PCM and nch == 3) else ENERGY, sense=BELOW if nch == 64 else ABOVE, hang=nch % 3)
        if kw["metric"] == DIFF:
            thr = int(np.median(plain["diff_energy"]))
        kw.update(open_thr=thr, close_thr=thr - thr // 4 if kw["sense"] == ABOVE else thr + thr // 4)
        want = restate(pkg, x, W, form, **kw)
        d, ptr = _on_device(torch, x, in_stride, lead)
        lv = pkg.Level(nch, n, W, form=form, metric=kw["metric"], sense=kw["sense"], open_thr=kw["open_thr"], close_thr=kw["close_thr"],
                       hang_windows=kw["hang"])
        lv.process_device(ptr, in_stride, n)
        got = lv.fetch()
        lv.close()
        same_records(got, want, f"form {form} W {W} channels {nch}")
        assert want.shape[1] == n // W >= 1
        if nch >= 3:
            assert int(want["peak"].max()) == 32768 and int(want["energy"][0, 0]) == (W * (2 if form == IQ else 1)) << 30


def _cuts(rng, n, W, biggest):
    """piece lengths that add up to n: zeros, ones, pieces below W, pieces that end exactly on a window edge, longer ones"""
    out, pos, kinds = [], 0, set()
    while pos < n:
        kind = int(rng.randint(0, 6))
        to_edge = W - pos % W
        m = [0, 1, int(rng.randint(1, max(2, W))), to_edge, to_edge + W * int(rng.randint(0, 3)), int(rng.randint(W, 3 * W + 2))][kind]
        if m <= min(n - pos, biggest):
            kinds.add(kind)
        m = min(m, n - pos, biggest)
        out.append(m)
        pos += m
    assert {0, 1, 2, 3, 4, 5} <= kinds
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", [PCM, IQ])
@pytest.mark.parametrize("W", [1, 7, 300, 1000, 4096, 10000])
def test_gpu_records_do_not_depend_on_the_cuts(pkg, form, W):
    """one stream in one call, and cut into seeded random pieces (length 0, length 1, below W, ending exactly on a window
    edge) through process_device and through process_host: the same records, equal to the restatement"""
    import torch
    nch = 5
    n = 40 * W + 13 if W >= 300 else 6000 + W
    rng = np.random.RandomState(100 + W + form)
    x = _rows(rng, nch, n, form)
    E = 2 if form == IQ else 1
    thr = int(np.median(restate(pkg, x, W, form)["energy"]))
    kw = dict(metric=ENERGY, sense=BELOW, open_thr=thr, close_thr=thr + thr // 8, hang=1)
    want = restate(pkg, x, W, form, **kw)
    mk = lambda cap: pkg.Level(nch, cap, W, form=form, metric=ENERGY, sense=BELOW, open_thr=thr, close_thr=kw["close_thr"], hang_windows=1)
    whole = mk(n)
    same_records(whole.process_host(x), want, "one call")
    whole.close()
    biggest = 3 * W + 2
    cuts = _cuts(rng, n, W, biggest)
    d, ptr = _on_device(torch, x, n * E + 3, 1)
    dev, host = mk(biggest), mk(biggest)
    parts_d, parts_h, pos = [], [], 0
    for m in cuts:
        dev.process_device(ptr + 2 * E * pos, n * E + 3, m)
        parts_d.append(dev.fetch())
        parts_h.append(host.process_host(x[:, pos:pos + m]))
        assert parts_d[-1].shape == (nch, (pos + m) // W - pos // W)
        pos += m
    dev.close()
    host.close()
    same_records(np.concatenate(parts_d, axis=1), want, "process_device, cut")
    same_records(np.concatenate(parts_h, axis=1), want, "process_host, cut")
    assert 0 in cuts and 1 in cuts and (W == 1 or any(0 < m < W for m in cuts))


def _d2h(ptr, nbytes):
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipDeviceSynchronize()
    host = np.zeros(nbytes, np.uint8)
    assert rt.hipMemcpy(host.ctypes.data, ptr, nbytes, 2) == 0
    return host


@pytest.mark.gpu
def test_gpu_device_view_and_fetch_agree_and_small_buffers_are_refused(pkg):
    b = pkg.binding
    nch, W, n = 7, 100, 2550
    rng = np.random.RandomState(77)
    x = (rng.randint(-3000, 3000, size=(nch, n)) * (1 + np.arange(nch))[:, None] // 2).astype(np.int16)
    plain = restate(pkg, x, W, PCM)
    thr = int(np.median(plain["energy"][:, -1]))
    want = restate(pkg, x, W, PCM, sense=ABOVE, open_thr=thr, close_thr=thr)
    lv = pkg.Level(nch, 4096, W, sense=ABOVE, open_thr=thr, close_thr=thr)
    assert lv.fetch().shape == (nch, 0)  # nothing processed yet
    rec, stride, nw, d_open = lv.device_view()
    assert nw == 0 and rec and d_open
    assert not _d2h(d_open, 4 * nch).any()  # starts closed
    first = lv.process_host(x[:, :1000])
    lv.process_host(x[:, 1000:])
    # too small a buffer: MFM_E_NOMEM, the needed count, nothing copied
    for cap in (0, 1, nch * 15 - 1):
        with pytest.raises(pkg.MfmError) as ei:
            lv.fetch(max_records=cap)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == nch * 15
        assert not ei.value.buffer.view(np.uint8).any()
    got = lv.fetch()
    same_records(np.concatenate([first, got], axis=1), want, "two calls")
    rec, stride, nw, d_open = lv.device_view()
    assert nw == 15 and stride >= nw
    raw = _d2h(rec, nch * stride * 40).view(b.LEVEL_RECORD_DTYPE).reshape(nch, stride)[:, :nw]
    same_records(raw, got, "device view")
    open_now = _d2h(d_open, 4 * nch).view(np.uint32)
    assert np.array_equal(open_now, got["open"][:, -1]) and 0 < int(open_now.sum()) < nch
    # a call that completes no window leaves the state where it was
    lv.process_host(x[:, :10])
    assert lv.fetch().shape == (nch, 0) and np.array_equal(_d2h(d_open, 4 * nch).view(np.uint32), open_now)
    lv.close()


E2E = dict(nr_out=16000, W=1000, carriers=list(range(3, 64, 8)), amplitude=6000.0, noise=512, seed=11)


def _e2e_input(pkg, ora):
    sy = pkg.synth
    fs, decim, taps, offs, gains = sy.plan("cfg2_64ch")
    n = decim * (E2E["nr_out"] - 1) + len(taps)
    iq = sy.synth_iq(n, fs, offs[E2E["carriers"]], seed=E2E["seed"], amplitude=E2E["amplitude"], noise=E2E["noise"])
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm, fiq = ora.run_channels(iq, cre, cim, incr, decim, threads=8, want_iq=True)
    assert pcm.shape == (64, E2E["nr_out"])
    on = np.zeros(64, bool)
    on[E2E["carriers"]] = True
    return (fs, decim, taps, offs, gains), iq, pcm, fiq, on


def _e2e_thresholds(pkg, pcm, fiq, on):
    """the two groups' window energies in the oracle's output, their margin and the geometric mean between them"""
    W = E2E["W"]
    e_pcm, e_iq = restate(pkg, pcm, W, PCM)["energy"].astype(np.float64), restate(pkg, fiq, W, IQ)["energy"].astype(np.float64)
    m_pcm = e_pcm[~on].min() / e_pcm[on].max()   # a captured carrier LOWERS the discriminator's energy
    m_iq = e_iq[on].min() / e_iq[~on].max()      # and RAISES the filtered IQ's
    return (m_pcm, int(np.sqrt(e_pcm[~on].min() * e_pcm[on].max()))), (m_iq, int(np.sqrt(e_iq[on].min() * e_iq[~on].max())))


def test_e2e_settings_separate_the_groups_in_the_oracle(pkg, ora):
    """The synth settings of the end-to-end test, chosen on the CPU with the oracle alone: 8 carriers (every eighth channel of
    the 64-channel plan, so no two are neighbours), amplitude 6000 in all, uniform noise of +-512, windows of 1000 outputs.
    Margin found in the oracle's window energies (smallest of the one group over largest of the other, all 16 windows):
    PCM form, sense BELOW: 3.81x (the guess from the noise statistics was about 5x; the low-pass in front of the
    discriminator colours the noise of an empty channel and takes some of its energy); IQ form, sense ABOVE: 32.2x.
    16 carriers (every fourth channel) do NOT reach 2x: 1.34x / 0.20x, the neighbours' splatter fills the gaps."""
    _, _, pcm, fiq, on = _e2e_input(pkg, ora)
    (m_pcm, _), (m_iq, _) = _e2e_thresholds(pkg, pcm, fiq, on)
    print(f"margins: PCM form {m_pcm:.2f}x, IQ form {m_iq:.2f}x")
    assert m_pcm >= 2.0 and m_iq >= 2.0


@pytest.mark.gpu
def test_gpu_engine_to_level_stage_on_device_equals_restatement_on_the_oracle(pkg, ora):
    """synth_iq with carriers on 8 of 64 channels -> engine (MFM_F_DEVICE_ONLY, filtered IQ on) -> level stage on the device
    PCM and on the device IQ, on the engine's stream, in blocks that are no multiple of anything: records equal the
    restatement run on the oracle's PCM / IQ, thresholds at the geometric mean of the two groups' window energies in the
    oracle's output, and the channels open at the end are exactly those with carriers, in both forms"""
    b = pkg.binding
    (fs, decim, taps, offs, gains), iq, pcm, fiq, on = _e2e_input(pkg, ora)
    (m_pcm, thr_pcm), (m_iq, thr_iq) = _e2e_thresholds(pkg, pcm, fiq, on)
    assert m_pcm >= 2.0 and m_iq >= 2.0
    W = E2E["W"]
    want_pcm = restate(pkg, pcm, W, PCM, sense=BELOW, open_thr=thr_pcm, close_thr=thr_pcm, hang=1)
    want_iq = restate(pkg, fiq, W, IQ, sense=ABOVE, open_thr=thr_iq, close_thr=thr_iq, hang=1)
    blk = 250007
    eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g), want_iq=True)
    eng.commit()
    cap = blk // decim + 8
    lp = pkg.Level(64, cap, W, form=PCM, sense=BELOW, open_thr=thr_pcm, close_thr=thr_pcm, hang_windows=1)
    li = pkg.Level(64, cap, W, form=IQ, sense=ABOVE, open_thr=thr_iq, close_thr=thr_iq, hang_windows=1)
    got_pcm, got_iq = [], []
    for s in range(0, iq.shape[0], blk):
        assert eng.push(iq[s:s + blk]) == 0
        d_pcm, stride, nout, d_iq = eng.last_output_device()
        assert d_iq
        lp.process_device(d_pcm, stride, nout, stream=eng.stream)
        li.process_device(d_iq, 2 * stride, nout, stream=eng.stream)
        got_pcm.append(lp.fetch())
        got_iq.append(li.fetch())
    same_records(np.concatenate(got_pcm, axis=1), want_pcm, "PCM form")
    same_records(np.concatenate(got_iq, axis=1), want_iq, "IQ form")
    for lv in (lp, li):
        _, _, _, d_open = lv.device_view()
        assert np.array_equal(_d2h(d_open, 4 * 64).view(np.uint32).astype(bool), on)
        lv.close()
    eng.close()
    assert np.array_equal(want_pcm["open"][:, -1].astype(bool), on) and np.array_equal(want_iq["open"][:, -1].astype(bool), on)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pcm", "iq"])
def test_gpu_level_scan_tool_prints_the_records(pkg, ora, tmp_path, form):
    """tools/level_scan.py on a small cs16 capture and a receiver JSON of the reference's shape: its lines parse and equal the
    restatement on the oracle's output, and --summary adds up"""
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
    pcm, fiq = ora.run_channels(iq, cre, cim, incr, decim, want_iq=True)
    rows, f = (fiq, IQ) if form == "iq" else (pcm, PCM)
    e = restate(pkg, rows, W, f)["energy"]
    thr = int(np.sqrt(float(e[[1, 5]].min()) * float(np.delete(e, [1, 5], axis=0).max()))) if form == "iq" else \
        int(np.sqrt(float(e[[1, 5]].max()) * float(np.delete(e, [1, 5], axis=0).min())))
    sense = ABOVE if form == "iq" else BELOW
    want = restate(pkg, rows, W, f, sense=sense, open_thr=thr, close_thr=thr, hang=2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
                        str(tmp_path / "capture.bin"), "--format", "cs16", "--form", form, "--window", str(W), "--open-thr", str(thr),
                        "--hang", "2", "--block", "100003", "--summary"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    recs = [ln for ln in lines if "summary" not in ln]
    sums = [ln for ln in lines if ln.get("summary")]
    assert len(recs) == want.size and len(sums) == 8
    seen = np.zeros(want.shape, bool)
    for ln in recs:
        c, k = ln["channel"], ln["window"]
        w = want[c, k]
        assert not seen[c, k] and ln["freq"] == centre + int(offs[c])
        assert (ln["energy"], ln["diff_energy"], ln["peak"], ln["open"]) == (int(w["energy"]), int(w["diff_energy"]), int(w["peak"]), int(w["open"])), ln
        seen[c, k] = True
    assert seen.all()
    for ln in sums:
        c = ln["channel"]
        assert ln["windows"] == want.shape[1] and ln["open_windows"] == int(want["open"][c].sum())
        assert abs(ln["open_share"] - ln["open_windows"] / ln["windows"]) < 1e-12
    assert 0 < sum(ln["open_windows"] for ln in sums) < want.size
