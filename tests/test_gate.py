"""The squelch gate stage (mfm_gate_*, csrc/mfm_gate.hip): of every channel's rows only the windows whose level record says
`open` go into one dense payload, with a run list that says which channel and which samples each piece is.

Every expected value comes from the numpy restatement in this file: concatenate the stream per channel, cut it into windows,
select by the mask, form runs per call.  Every comparison is an equality."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["mfm_gate_create", "mfm_gate_destroy", "mfm_gate_process_device", "mfm_gate_process_host", "mfm_gate_fetch",
             "mfm_gate_device_view", "mfm_hosttwin_gate_call"]
MASKS = ["closed", "open", "alternating", "single_last", "bernoulli"]


# ---- the restatement ----------------------------------------------------------------------------------------

def restate_call(pkg, stream, mask, W, E, pos, nr_in):
    """(runs, payload) of the call that takes samples [pos, pos + nr_in) of stream int16 [C][n * E]; mask bool [C][n // W]"""
    k0, k1 = pos // W, (pos + nr_in) // W
    We = W * E
    runs, pieces, offset = [], [], 0
    for c in range(stream.shape[0]):
        k = k0
        while k < k1:
            if not mask[c, k]:
                k += 1
                continue
            e = k
            while e < k1 and mask[c, e]:
                e += 1
            runs.append((k, offset, c, e - k))
            pieces.append(stream[c, k * We:e * We])
            offset += (e - k) * We
            k = e
    payload = np.concatenate(pieces) if pieces else np.zeros(0, np.int16)
    return np.array(runs, pkg.binding.GATE_RUN_DTYPE), payload


def records_of(pkg, mask, k0, k1):
    """what the level stage would hand over for windows [k0, k1): only .open and .window matter, the rest is filler"""
    nch = mask.shape[0]
    rec = np.zeros((nch, k1 - k0), pkg.binding.LEVEL_RECORD_DTYPE)
    rec["window"] = np.arange(k0, k1, dtype=np.uint64)[None, :]
    rec["channel"] = np.arange(nch, dtype=np.uint32)[:, None]
    rec["open"] = mask[:, k0:k1]
    rec["energy"] = 0x0123456789ABCDEF
    rec["peak"] = 77
    return rec


def make_mask(kind, rng, nch, nw):
    if kind == "closed":
        return np.zeros((nch, nw), bool)
    if kind == "open":
        return np.ones((nch, nw), bool)
    if kind == "alternating":
        return (np.arange(nw)[None, :] + np.arange(nch)[:, None]) % 2 == 0
    if kind == "single_last":
        m = np.zeros((nch, nw), bool)
        m[nch - 1, nw // 2] = True
        return m
    assert kind == "bernoulli"
    return rng.rand(nch, nw) < 0.3


def make_cuts(rng, n, W, biggest):
    """piece lengths that add up to n: a zero, three pieces in a row shorter than W, then zeros, ones, pieces below W, pieces
    that end exactly on a window edge and longer ones"""
    out = [0] + [min(int(rng.randint(1, W)) if W > 1 else 0, n // 4) for _ in range(3)]
    pos = sum(out)
    assert sum(out[1:]) < max(W, 2) * 3
    while pos < n:
        kind = int(rng.randint(0, 6))
        to_edge = W - pos % W
        m = [0, 1, int(rng.randint(1, max(2, W))), to_edge, to_edge + W * int(rng.randint(0, 3)), int(rng.randint(W, biggest + 1))][kind]
        m = min(m, n - pos, biggest)
        out.append(m)
        pos += m
    return out


def stream_len(W):
    """at least 9 windows and a ragged end; for short windows several hundred, so that one call spans more than one chunk of
    64 records"""
    return 300 * W + W // 2 + 1 if W <= 8 else 9 * W + W // 2 + 3


def biggest_cut(W):
    return 150 * W + 1 if W <= 8 else 3 * W + 2


def same(got, want, what):
    (gr, gp), (wr, wp) = got, want
    assert gr.shape == wr.shape, (what, gr.shape, wr.shape)
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert bad.size == 0, f"{what}: run field {f} differs at {bad[:5].tolist()}: {gr[f][bad[0]]} != {wr[f][bad[0]]}"
    assert gp.shape == wp.shape, (what, gp.shape, wp.shape)
    bad = np.flatnonzero(gp != wp)
    assert bad.size == 0, f"{what}: payload differs at {bad[:5].tolist()} of {wp.size}"


def drive(pkg, stream, mask, W, E, cuts, call, what):
    """feed the cuts through call(pos, rows, records) and compare every call with the restatement; returns windows emitted"""
    pos = emitted = 0
    for m in cuts:
        k0, k1 = pos // W, (pos + m) // W
        got = call(pos, stream[:, pos * E:(pos + m) * E], records_of(pkg, mask, k0, k1))
        want = restate_call(pkg, stream, mask, W, E, pos, m)
        same(got, want, f"{what}, call at {pos} of {m}")
        emitted += int(want[0]["nr_windows"].sum())
        pos += m
    assert pos * E == stream.shape[1] and emitted == int(mask.sum())
    return emitted


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_gate_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in pkg.binding.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src)
    b = pkg.binding
    assert b.GATE_RUN_DTYPE.itemsize == 24 and C.sizeof(b.GateRun) == 24 and C.sizeof(b.GateConfig) == 32
    assert pkg.GATE_RUN_DTYPE is b.GATE_RUN_DTYPE and pkg.Gate is b.Gate
    m = re.search(r"struct mfm_gate_run \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [
        ("uint64_t", "first_window"), ("uint64_t", "payload_offset"), ("uint32_t", "channel"), ("uint32_t", "nr_windows")]
    assert list(b.GATE_RUN_DTYPE.names) == ["first_window", "payload_offset", "channel", "nr_windows"]
    m = re.search(r"struct mfm_gate_config \{(.*?)\};", src, flags=re.S)
    assert m and [n for _, n in re.findall(r"(u?int\d+_t)\s+(\w+);", m.group(1))] == [n for n, _ in b.GateConfig._fields_]


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("W", [1, 2, 3, 7, 8, 511, 512, 4099])
def test_hosttwin_calls_equal_numpy_restatement(pkg, W, E):
    """csrc/mfm_gate.h through its host twin: 1, 2 and 65 channels, every mask, seeded random cuts"""
    n = stream_len(W)
    for nch in (1, 2, 65):
        rng = np.random.RandomState(1000 * E + 10 * W + nch)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for kind in MASKS:
            mask = make_mask(kind, rng, nch, n // W)
            cuts = make_cuts(rng, n, W, biggest_cut(W))
            carry = np.zeros((nch, W * E), np.int16)
            emitted = drive(pkg, stream, mask, W, E, cuts, lambda pos, rows, rec: pkg.binding.hosttwin_gate_call(W, E, pos, rows, carry, rec),
                            f"W {W} E {E} channels {nch} mask {kind}")
            if kind == "closed":
                assert emitted == 0
            if kind == "single_last":
                assert emitted == 1


def _crossing_case(pkg):
    """W = 5, three channels, calls of 12 and 13 samples: windows 1 and 2 of channel 1 are open, window 1 ends the first call's
    windows and window 2 begins the second's"""
    W, E, nch = 5, 1, 3
    rng = np.random.RandomState(3)
    stream = rng.randint(-32768, 32768, size=(nch, 25)).astype(np.int16)
    mask = np.zeros((nch, 5), bool)
    mask[1, 1:3] = True
    mask[2, 4] = True
    return W, E, nch, stream, mask


def _check_crossing(pkg, stream, mask, first, second):
    (r1, p1), (r2, p2) = first, second
    assert len(r1) == 1 and len(r2) == 2
    assert (int(r1[0]["channel"]), int(r1[0]["first_window"]), int(r1[0]["nr_windows"])) == (1, 1, 1)
    assert (int(r2[0]["channel"]), int(r2[0]["first_window"]), int(r2[0]["nr_windows"])) == (1, 2, 1)
    assert int(r2[0]["first_window"]) == int(r1[0]["first_window"]) + int(r1[0]["nr_windows"])  # consecutive windows, two runs
    assert np.array_equal(np.concatenate([p1, p2[:5]]), stream[1, 5:15])
    same(first, restate_call(pkg, stream, mask, 5, 1, 0, 12), "first call")
    same(second, restate_call(pkg, stream, mask, 5, 1, 12, 13), "second call")


def test_hosttwin_run_that_crosses_a_call_boundary_is_two_runs(pkg):
    W, E, nch, stream, mask = _crossing_case(pkg)
    carry = np.zeros((nch, W), np.int16)
    first = pkg.binding.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, records_of(pkg, mask, 0, 2))
    second = pkg.binding.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, records_of(pkg, mask, 2, 5))
    _check_crossing(pkg, stream, mask, first, second)


def test_hosttwin_runs_across_chunks_of_64_records(pkg):
    """one call of 200 windows: runs that begin in one chunk of 64 records and end in the next or the one after, that end
    exactly on a chunk edge, that begin on one, and one that covers everything"""
    W, E, nch, nw = 2, 1, 4, 200
    rng = np.random.RandomState(8)
    stream = rng.randint(-32768, 32768, size=(nch, nw * W)).astype(np.int16)
    mask = np.zeros((nch, nw), bool)
    mask[0, 60:70] = mask[0, 100:128] = mask[0, 128:130] = True   # one run over the 64 edge, one 100 .. 129 over the 128 edge
    mask[1, :] = True                                             # every chunk continues the run
    mask[2, 10:64] = mask[2, 65:128] = mask[2, 192:200] = True    # ends on an edge, begins behind one and ends on the next
    mask[3, 63] = mask[3, 64] = mask[3, 127] = mask[3, 199] = True
    carry = np.zeros((nch, W), np.int16)
    got = pkg.binding.hosttwin_gate_call(W, E, 0, stream, carry, records_of(pkg, mask, 0, nw))
    same(got, restate_call(pkg, stream, mask, W, E, 0, nw * W), "200 windows")
    assert [int(x) for x in got[0]["nr_windows"]] == [10, 30, 200, 54, 63, 8, 2, 1, 1]


def test_hosttwin_refuses_what_the_stage_refuses(pkg):
    b = pkg.binding
    W, E, nch, stream, mask = _crossing_case(pkg)
    carry = np.zeros((nch, W), np.int16)
    with pytest.raises(pkg.MfmError) as ei:  # 12 samples complete two windows, not three
        b.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, records_of(pkg, mask, 0, 3))
    assert ei.value.code == b.MFM_E_INVAL
    rec = records_of(pkg, mask, 0, 2)
    rec["window"][2, 1] += 1
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, rec)
    assert ei.value.code == b.MFM_E_STATE and "out of step" in str(ei.value)
    for kw in (dict(max_runs=0), dict(max_elems=4)):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, records_of(pkg, mask, 0, 2), **kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (1, 5)
    assert not carry.any()  # a refused call changes nothing
    first = b.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, records_of(pkg, mask, 0, 2))
    second = b.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, records_of(pkg, mask, 2, 5))
    _check_crossing(pkg, stream, mask, first, second)


def test_hosttwin_refusals_on_a_later_call_leave_a_filled_carry(pkg):
    """the refusals above at the second call, where the carry holds the two samples the first call left: MFM_E_STATE "out of
    step", MFM_E_NOMEM with the needed sizes, and the carry unchanged after each"""
    b = pkg.binding
    W, E, nch, stream, mask = _crossing_case(pkg)
    carry = np.zeros((nch, W), np.int16)
    first = b.hosttwin_gate_call(W, E, 0, stream[:, :12], carry, records_of(pkg, mask, 0, 2))
    assert np.array_equal(carry[:, :2], stream[:, 10:12]) and carry.any()
    kept = carry.copy()
    with pytest.raises(pkg.MfmError) as ei:  # 13 samples from 12 complete three windows, not two
        b.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, records_of(pkg, mask, 2, 4))
    assert ei.value.code == b.MFM_E_INVAL and np.array_equal(carry, kept)
    rec = records_of(pkg, mask, 2, 5)
    rec["window"][0, 2] -= 1
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, rec)
    assert ei.value.code == b.MFM_E_STATE and "out of step" in str(ei.value) and np.array_equal(carry, kept)
    for kw in (dict(max_runs=1), dict(max_elems=2 * W - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, records_of(pkg, mask, 2, 5), **kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (2, 2 * W) and np.array_equal(carry, kept)
    second = b.hosttwin_gate_call(W, E, 12, stream[:, 12:], carry, records_of(pkg, mask, 2, 5))
    _check_crossing(pkg, stream, mask, first, second)


def _history_case(pkg):
    """W = 5000, E = 2: a window is 10 000 elements, two pieces of the copy kernel.  The first call completes no window and
    leaves 9200 elements of window 0 on the device, so in the second call that window's piece 0 (8192 elements) lies wholly
    in the history and its piece 1 across the seam; the third call begins 9214 elements into window 2"""
    W, E, nch = 5000, 2, 3
    n = 4 * W + 13
    cuts = [4600, 2 * W + 7, n - 4600 - 2 * W - 7]
    assert 4600 * E >= 8192 and all(m > 0 for m in cuts)
    rng = np.random.RandomState(61)
    stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
    masks = {"open": np.ones((nch, 4), bool), "bernoulli": rng.rand(nch, 4) < 0.5}
    first = masks["bernoulli"][:, [0, 2]]
    assert first.any() and not first.all()  # of the windows that begin in the history some go out and some do not
    return W, E, nch, stream, cuts, masks


def test_hosttwin_piece_wholly_in_the_carry(pkg):
    W, E, nch, stream, cuts, masks = _history_case(pkg)
    for kind, mask in masks.items():
        carry = np.zeros((nch, W * E), np.int16)
        drive(pkg, stream, mask, W, E, cuts, lambda pos, rows, rec: pkg.binding.hosttwin_gate_call(W, E, pos, rows, carry, rec),
              f"history case, mask {kind}")


def test_create_refuses_bad_configurations(pkg):
    """argument checks come before the device is touched: MFM_E_INVAL with or without a GPU.  The carry (the history's
    unfinished window) bounds window_samples * elems_per_sample at 2^20"""
    b = pkg.binding
    good = dict(nr_channels=2, max_in_samples=4096, window_samples=64)

    def refused(**kw):
        with pytest.raises(pkg.MfmError) as ei:
            pkg.Gate(**dict(good, **kw))
        assert ei.value.code == b.MFM_E_INVAL, kw

    refused(abi_version=b.MFM_ABI_VERSION + 1)
    refused(nr_channels=0)
    refused(nr_channels=65536)
    refused(max_in_samples=0)
    refused(window_samples=0)
    refused(elems_per_sample=0)
    refused(elems_per_sample=3)
    refused(window_samples=(1 << 20) + 1)
    refused(window_samples=(1 << 19) + 1, elems_per_sample=2)
    assert b"carry" in pkg.load_library().mfm_last_error()
    import torch
    for kw in (dict(window_samples=1 << 20, max_in_samples=1 << 20), dict(window_samples=1 << 19, elems_per_sample=2, max_in_samples=1 << 20)):
        try:
            pkg.Gate(**dict(good, **kw)).close()
            assert torch.cuda.is_available()
        except pkg.MfmError as e:
            assert e.code == b.MFM_E_DEVICE and not torch.cuda.is_available()


def test_gate_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_gate.o (tools/kernel_regs.py): five kernels, no private segment, no spilled register"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_gate.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_gate.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    assert len(lines) == 5, out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# the scene of tests/test_level.py's end-to-end test, gated: squelch on the IQ energy, gate the PCM

_SCENE = {}


def _scene(pkg, ora):
    if not _SCENE:
        _SCENE["it"] = _make_scene(pkg, ora)
    return _SCENE["it"]


def _make_scene(pkg, ora):
    import test_level as tl
    plan, iq, pcm, fiq, on = tl._e2e_input(pkg, ora)
    (_, _), (m_iq, thr_iq) = tl._e2e_thresholds(pkg, pcm, fiq, on)
    W = tl.E2E["W"]
    want = tl.restate(pkg, fiq, W, tl.IQ, sense=tl.ABOVE, open_thr=thr_iq, close_thr=thr_iq, hang=1)
    return plan, iq, pcm, W, m_iq, thr_iq, want


def _scene_is_not_vacuous(m_iq, want):
    opened = want["open"].astype(bool)
    assert m_iq >= 2.0                      # the threshold lies between the two groups' energies
    assert opened.any(axis=1).any()         # a channel with an open window
    assert (~opened.any(axis=1)).any()      # a channel that never opens
    assert 0.0 < opened.mean() < 1.0


def test_scene_thresholds_open_some_channels_and_not_others_in_the_oracle(pkg, ora):
    """the condition the GPU scene test relies on, checked with the oracle alone: a threshold at the geometric mean of the
    carrier and idle IQ window energies (32x apart, tests/test_level.py) opens the 8 carrier channels and no other"""
    _, _, _, _, m_iq, _, want = _scene(pkg, ora)
    print(f"IQ margin {m_iq:.2f}x, open share {want['open'].mean():.4f}")
    _scene_is_not_vacuous(m_iq, want)


# ---- GPU ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("W", [1, 2, 3, 7, 8, 511, 512, 4099])
def test_gpu_process_host_equals_numpy_restatement(pkg, W, E):
    """the CPU matrix through mfm_gate_process_host"""
    n = stream_len(W)
    for nch in (1, 2, 65):
        rng = np.random.RandomState(1000 * E + 10 * W + nch)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for kind in MASKS:
            mask = make_mask(kind, rng, nch, n // W)
            cuts = make_cuts(rng, n, W, biggest_cut(W))
            gate = pkg.Gate(nch, biggest_cut(W), W, elems_per_sample=E)
            drive(pkg, stream, mask, W, E, cuts, lambda pos, rows, rec: gate.process_host(rows, rec), f"W {W} E {E} channels {nch} mask {kind}")
            gate.close()


@pytest.mark.gpu
def test_gpu_run_that_crosses_a_call_boundary_is_two_runs(pkg):
    W, E, nch, stream, mask = _crossing_case(pkg)
    gate = pkg.Gate(nch, 16, W)
    first = gate.process_host(stream[:, :12], records_of(pkg, mask, 0, 2))
    second = gate.process_host(stream[:, 12:], records_of(pkg, mask, 2, 5))
    gate.close()
    _check_crossing(pkg, stream, mask, first, second)


def _to_device(torch, stream, in_stride, lead):
    nch = stream.shape[0]
    host = np.full(lead + nch * in_stride + 8, 0x5555, np.int16)
    host[lead:lead + nch * in_stride].reshape(nch, in_stride)[:, :stream.shape[1]] = stream
    d = torch.from_numpy(host).cuda()
    return d, d.data_ptr() + 2 * lead


def _device_calls(pkg, torch, stream, mask, W, E, cuts, in_stride, lead, what, cap):
    d, ptr = _to_device(torch, stream, in_stride, lead)
    gate = pkg.Gate(stream.shape[0], cap, W, elems_per_sample=E)
    keep = []

    def call(pos, rows, rec):
        d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy() if rec.size else np.zeros(8, np.uint8)).cuda()
        keep.append(d_rec)
        gate.process_device(ptr + 2 * E * pos, in_stride, rows.shape[1] // E, d_rec.data_ptr(), rec.shape[1], rec.shape[1])
        return gate.fetch()

    drive(pkg, stream, mask, W, E, cuts, call, what)
    gate.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [1, 3])
@pytest.mark.parametrize("W,E", [(8, 1), (4, 2), (7, 1), (3, 2), (512, 1), (511, 1), (515, 2), (4099, 1)])
def test_gpu_process_device_at_every_alignment(pkg, W, E, lead):
    """rows in device memory with an odd in_stride and a base offset by 1 and by 3 elements; W E a multiple of 8 and not"""
    import torch
    n = stream_len(W)
    nch = 5
    rng = np.random.RandomState(W * 31 + E + lead)
    stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
    in_stride = n * E + 1 + (n * E) % 2
    assert in_stride % 2 == 1
    for kind in ("open", "bernoulli", "alternating"):
        mask = make_mask(kind, rng, nch, n // W)
        cuts = make_cuts(rng, n, W, biggest_cut(W))
        _device_calls(pkg, torch, stream, mask, W, E, cuts, in_stride, lead, f"W {W} E {E} lead {lead} mask {kind}", biggest_cut(W))


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [1, 63, 64, 65, 257, 1024])
def test_gpu_channel_scan_crosses_wave_and_block_edges(pkg, nch):
    import torch
    for W, E in ((5, 1), (8, 2)):
        n = 4 * W + 5
        rng = np.random.RandomState(nch + W)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        for kind in ("bernoulli", "open", "single_last"):
            mask = make_mask(kind, rng, nch, n // W)
            _device_calls(pkg, torch, stream, mask, W, E, [W + 2, n - W - 2], n * E + 1, 1, f"channels {nch} W {W} mask {kind}", n)


@pytest.mark.gpu
def test_gpu_many_channels_with_more_than_a_scan_thread_each(pkg):
    """2500 channels: a scan thread sums three channels"""
    nch, W = 2500, 2
    rng = np.random.RandomState(12)
    stream = rng.randint(-32768, 32768, size=(nch, 9)).astype(np.int16)
    mask = rng.rand(nch, 4) < 0.4
    gate = pkg.Gate(nch, 16, W)
    drive(pkg, stream, mask, W, 1, [3, 6], lambda pos, rows, rec: gate.process_host(rows, rec), "2500 channels")
    gate.close()


@pytest.mark.gpu
def test_gpu_wide_copy_path(pkg):
    """W = 4096, nr_in = 3 * 4096 + 17 in one call, then the rest: whole pieces of 16-byte stores, and IQ rows whose window is
    two pieces"""
    import torch
    W, n = 4096, 5 * 4096 + 40
    for E in (1, 2, 3):
        E, We_odd = (E, False) if E < 3 else (2, True)
        nch = 6
        rng = np.random.RandomState(40 + E)
        stream = rng.randint(-32768, 32768, size=(nch, n * E)).astype(np.int16)
        mask = rng.rand(nch, n // W) < 0.6
        mask[0, :] = True
        lead = 3 if We_odd else 0
        _device_calls(pkg, torch, stream, mask, W, E, [3 * 4096 + 17, n - 3 * 4096 - 17], n * E + (1 if We_odd else 8), lead,
                      f"wide E {E} lead {lead}", 3 * 4096 + 17)


@pytest.mark.gpu
def test_gpu_piece_wholly_in_the_history_without_preroll(pkg):
    """_history_case on the device: a piece that lies wholly in the history takes the 16-byte loop from the history's pointer, the
    next one the loop across the seam; rows 16-byte aligned with a stride that is a multiple of 8, and off by 3 with an odd one"""
    import torch
    W, E, nch, stream, cuts, masks = _history_case(pkg)
    for lead, pad in ((0, 8), (3, 1)):
        for kind, mask in masks.items():
            _device_calls(pkg, torch, stream, mask, W, E, cuts, stream.shape[1] + pad, lead, f"history case lead {lead} mask {kind}", max(cuts))


@pytest.mark.gpu
def test_gpu_overflow_small_buffers_and_out_of_step_records(pkg):
    b = pkg.binding
    W, nch, n = 6, 4, 60
    rng = np.random.RandomState(21)
    stream = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
    mask = np.zeros((nch, 10), bool)
    mask[:, :5] = True            # the first call: 20 open windows
    mask[1, 6:8] = mask[3, 9] = True
    gate = pkg.Gate(nch, 64, W, max_open_windows=19)
    assert gate.fetch()[0].size == 0 and gate.fetch()[1].size == 0  # nothing processed yet
    # a wrong nr_windows: MFM_E_INVAL, and the stage stays where it was
    with pytest.raises(pkg.MfmError) as ei:
        gate.process_host(stream[:, :31], records_of(pkg, mask, 0, 4))
    assert ei.value.code == b.MFM_E_INVAL
    # 20 open windows do not fit 19: MFM_E_STATE at fetch, nothing copied
    with pytest.raises(pkg.MfmError) as ei:
        gate.process_host(stream[:, :31], records_of(pkg, mask, 0, 5))
    assert ei.value.code == b.MFM_E_STATE and "max_open_windows" in str(ei.value)
    assert not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
    # the following call fits and is right: the position and the carry moved on
    got = gate.process_host(stream[:, 31:], records_of(pkg, mask, 5, 10))
    want = restate_call(pkg, stream, mask, W, 1, 31, 29)
    same(got, want, "the call after an overflow")
    assert len(want[0]) == 2 and want[1].size == 3 * W
    # too small a buffer: MFM_E_NOMEM, the needed sizes, nothing copied; then the retry
    for kw in (dict(max_runs=1, max_elems=3 * W), dict(max_runs=2, max_elems=3 * W - 1), dict(max_runs=0, max_elems=0)):
        with pytest.raises(pkg.MfmError) as ei:
            gate.fetch(**kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (2, 3 * W)
        assert not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
    same(gate.fetch(max_runs=2, max_elems=3 * W), want, "retry")
    # the device view shows the same
    d_runs, d_payload, d_totals = gate.device_view()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    tot, pay, runs = np.zeros(4, np.uint64), np.zeros(3 * W, np.int16), np.zeros(2, b.GATE_RUN_DTYPE)
    for host, dev in ((tot, d_totals), (pay, d_payload), (runs, d_runs)):
        assert rt.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2) == 0
    assert tot.tolist() == [2, 3 * W, 0, 0]
    same((runs, pay), want, "device view")
    gate.close()
    # records with a wrong .window: MFM_E_STATE
    gate = pkg.Gate(nch, 64, W)
    rec = records_of(pkg, mask, 0, 5)
    rec["window"][2, 3] = 7
    with pytest.raises(pkg.MfmError) as ei:
        gate.process_host(stream[:, :31], rec)
    assert ei.value.code == b.MFM_E_STATE and "level and gate out of step" in str(ei.value)
    gate.close()
    # records of windows 1 .. 5 where 0 .. 4 are due (a level object one call ahead)
    gate = pkg.Gate(nch, 64, W)
    with pytest.raises(pkg.MfmError) as ei:
        gate.process_host(stream[:, :31], records_of(pkg, mask, 1, 6))
    assert ei.value.code == b.MFM_E_STATE
    gate.close()


@pytest.mark.gpu
def test_gpu_engine_level_gate_on_device_equals_selection_of_the_oracle(pkg, ora):
    """synth_iq with carriers on 8 of 64 channels -> engine (filtered IQ on) -> level stage in the IQ form -> gate on the PCM
    rows, all on the engine's stream, in blocks that are no multiple of anything: runs and payload equal the oracle's PCM
    selected by the numpy squelch over the oracle's IQ energies"""
    b = pkg.binding
    (fs, decim, taps, offs, gains), iq, pcm, W, m_iq, thr_iq, want = _scene(pkg, ora)
    _scene_is_not_vacuous(m_iq, want)
    mask = want["open"].astype(bool)
    blk = 250007
    eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g), want_iq=True)
    eng.commit()
    cap = blk // decim + 8
    lv = pkg.Level(64, cap, W, form=b.MFM_LEVEL_IQ, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr_iq, close_thr=thr_iq, hang_windows=1)
    gate = pkg.Gate(64, cap, W, elems_per_sample=1)
    pos = windows = 0
    for s in range(0, iq.shape[0], blk):
        assert eng.push(iq[s:s + blk]) == 0
        d_pcm, stride, nout, d_iq = eng.last_output_device()
        lv.process_device(d_iq, 2 * stride, nout, stream=eng.stream)
        d_rec, rec_stride, nw, _ = lv.device_view()
        gate.process_device(d_pcm, stride, nout, d_rec, rec_stride, nw, stream=eng.stream)
        got = gate.fetch()
        same(got, restate_call(pkg, pcm, mask, W, 1, pos, nout), f"block at {pos}")
        windows += int(got[0]["nr_windows"].sum())
        pos += nout
    assert pos == pcm.shape[1] and windows == int(mask.sum()) > 0
    for o in (gate, lv, eng):
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pcm", "iq"])
def test_gpu_level_scan_tool_writes_the_gated_samples(pkg, ora, tmp_path, form):
    """tools/level_scan.py --gate-out on a small cs16 capture: each chNNNN.s16 is the numpy selection of the oracle's rows, and
    index.jsonl agrees with the files; stdout is what it is without the option"""
    import test_level as tl
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
    rows, f, E = (fiq, tl.IQ, 2) if form == "iq" else (pcm, tl.PCM, 1)
    e = tl.restate(pkg, rows, W, f)["energy"]
    thr = int(np.sqrt(float(e[[1, 5]].min()) * float(np.delete(e, [1, 5], axis=0).max()))) if form == "iq" else \
        int(np.sqrt(float(e[[1, 5]].max()) * float(np.delete(e, [1, 5], axis=0).min())))
    want = tl.restate(pkg, rows, W, f, sense=tl.ABOVE if form == "iq" else tl.BELOW, open_thr=thr, close_thr=thr, hang=2)
    mask = want["open"].astype(bool)
    assert mask.any() and not mask.all()
    flat = np.ascontiguousarray(rows).reshape(8, -1)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
           str(tmp_path / "capture.bin"), "--format", "cs16", "--form", form, "--window", str(W), "--open-thr", str(thr),
           "--hang", "2", "--block", "100003", "--summary"]
    r = subprocess.run(cmd + ["--gate-out", str(tmp_path / "gated")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and plain.stdout == r.stdout
    index = [json.loads(ln) for ln in (tmp_path / "gated" / "index.jsonl").read_text().splitlines()]
    sizes = {}
    for c in range(8):
        path = tmp_path / "gated" / f"ch{c:04d}.s16"
        sel = np.concatenate([flat[c, k * W * E:(k + 1) * W * E] for k in np.flatnonzero(mask[c])]) if mask[c].any() else None
        assert path.exists() == (sel is not None)
        if sel is not None:
            assert np.array_equal(np.fromfile(path, np.int16), sel), c
            sizes[c] = 2 * sel.size
    at = {c: 0 for c in sizes}
    seen = np.zeros(mask.shape, bool)
    for ln in index:
        c = ln["channel"]
        assert ln["file_offset"] == at[c] and ln["first_sample"] % W == 0 and ln["nr_samples"] % W == 0 and ln["nr_samples"] > 0
        k0, k1 = ln["first_sample"] // W, (ln["first_sample"] + ln["nr_samples"]) // W
        assert mask[c, k0:k1].all() and not seen[c, k0:k1].any()
        seen[c, k0:k1] = True
        at[c] += 2 * E * ln["nr_samples"]
    assert at == sizes and np.array_equal(seen, mask)
