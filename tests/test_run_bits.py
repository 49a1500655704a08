"""The sign-bit path of the burst chain: mfm_runrs_process_bits_device (csrc/mfm_run_bits.hip, csrc/mfm_runrs_kernels.h) writes one
predicate bit per output, every run's bits starting on a 32-bit word, and mfm_runais_process_bits_device /
mfm_runpocsag_process_bits_device copy those words in the place of their slicers.

The checker of the resampler's bits is the PCM form, which tests/test_runrs.py checks against the oracle: the bits are the
predicate of its outputs, packed here with numpy.  The checkers of the stages are the PCM entries (tests/test_runais.py,
tests/test_runpocsag.py) and, on the device, the oracle chain of those files.  Every comparison is an equality.

What a run of whole windows can produce.  The gate emits whole windows, so a stretch of n windows through a fresh resampler has
total(n) = ((n W - plen) I - 1) // D + 1 outputs (0 while n W <= plen), and a run that continues a stretch across a call
boundary has total(a + b) - total(a).  At W = 64 that rules some run lengths out.  Five windows of 4/5 add exactly 256 outputs
and 25 windows of 16/25 exactly 1024, so the run lengths modulo 64 take a few values only (32, 20, 7, 58, 45 and their
differences for 4/5): no run has a length of 1 or 63 modulo 64, none has 1025 (1024 is reached only as 20 resp. 25 windows behind
a handover, and the next window adds 51 resp. 41).  With 4/5 and 81 taps no run has 1 .. 31 outputs (one window already gives
32), and a run has 0 outputs only where plen >= W (the 269 taps).  plan_case() finds, for each shape, a run for every edge the
shape can produce and says which it cannot (an exhaustive search, checked against CANNOT below); with W = 1 a run can have any
length and one call holds every edge, so the edges that W = 64 lacks are not dropped, they are checked there."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_runais as tra
import test_runpocsag as trp
import test_runrs as tr

ROOT = tg.ROOT
NEW_NAMES = ["mfm_runrs_process_bits_device", "mfm_runrs_bits_view", "mfm_runrs_fetch_bits", "mfm_runrs_get_bits_capacity",
             "mfm_runais_process_bits_device", "mfm_runpocsag_process_bits_device", "mfm_hosttwin_runrs_call_bits",
             "mfm_hosttwin_runais_call_bits", "mfm_hosttwin_runpocsag_call_bits"]
NEG, POS = 1, 2   # MFM_BITS_NEG, MFM_BITS_POS


def pack(pkg, runs, payload, polarity):
    """the bits form of a PCM result, restated: per run the predicate of its outputs, LSB first, padded with zeros to a word;
    out_offset the exclusive scan of (nr_out + 31) // 32"""
    out = runs.copy()
    words, at = [], 0
    for i, r in enumerate(runs):
        o, n = int(r["out_offset"]), int(r["nr_out"])
        y = payload[o:o + n]
        bit = (y < 0) if polarity == NEG else (y > 0)
        padded = np.zeros((n + 31) // 32 * 32, np.uint8)
        padded[:n] = bit
        words.append(np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32))
        out["out_offset"][i] = at
        at += (n + 31) // 32
    return out, (np.concatenate(words) if words else np.zeros(0, np.uint32))


def same_bits(got, want, what):
    (gr, gb), (wr, wb) = got, want
    assert gr.shape == wr.shape, (what, gr.shape, wr.shape)
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert bad.size == 0, f"{what}: run field {f} differs at {bad[:5].tolist()}: {gr[f][bad[0]]} != {wr[f][bad[0]]}"
    assert gb.dtype == np.uint32 and gb.shape == wb.shape, (what, gb.shape, wb.shape)
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, f"{what}: bit words differ at {bad[:5].tolist()} of {wb.size}: {gb[bad[:5]]} != {wb[bad[:5]]}"


# ---- CPU: names, sizes ----------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_bits_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    b = pkg.binding
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in b.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src) and b.MFM_ABI_VERSION == 4
    assert (b.MFM_BITS_NEG, b.MFM_BITS_POS) == (NEG, POS)
    m = re.search(r"struct mfm_runrs_bits_view \{(.*?)\};", src, flags=re.S)
    assert m and re.findall(r"(\w+)\s*\*?\s*(\w+);", m.group(1)) == [("mfm_runrs_run", "d_runs"), ("uint32_t", "d_bits"), ("uint64_t", "d_totals"),
                                                                    ("uint32_t", "polarity"), ("uint32_t", "reserved")]
    assert [n for n, _ in b.RunrsBitsView._fields_] == ["d_runs", "d_bits", "d_totals", "polarity", "reserved"]
    assert C.sizeof(b.RunrsBitsView) == 32 and pkg.RunrsBitsView is b.RunrsBitsView
    # no existing struct changed its size
    assert b.RUNRS_RUN_DTYPE.itemsize == 40 and C.sizeof(b.RunrsRun) == 40 and b.RUNRS_STATE_DTYPE.itemsize == 24
    assert C.sizeof(b.RunrsConfig) == 48 and C.sizeof(b.RunaisConfig) == 28 and C.sizeof(b.RunPocsagConfig) == 28
    assert b.RUNAIS_EVENT_DTYPE.itemsize == 200 and b.RUNAIS_STATE_DTYPE.itemsize == 264
    assert b.RUNPOCSAG_EVENT_DTYPE.itemsize == 176 and b.RUNPOCSAG_STATE_DTYPE.itemsize == 432
    assert C.sizeof(b.BitsView) == 32 and C.sizeof(b.GateRun) == b.GATE_RUN_DTYPE.itemsize == 24
    for name in ("hosttwin_runrs_call_bits", "hosttwin_runais_call_bits", "hosttwin_runpocsag_call_bits"):
        assert getattr(pkg, name) is getattr(b, name)
    for cls, names in ((b.RunResampler, ("process_bits_device", "bits_view", "fetch_bits", "bits_capacity")),
                       (b.RunAis, ("process_bits_device",)), (b.RunPocsag, ("process_bits_device",))):
        for n in names:
            assert callable(getattr(cls, n))
    # the entries want an object
    assert lib.mfm_runrs_get_bits_capacity(None, None, None) == b.MFM_E_INVAL
    assert lib.mfm_runrs_bits_view(None, None) == b.MFM_E_INVAL


def test_bits_kernels_use_no_scratch_and_do_not_spill():
    """the code object's notes of build/mfm_run_bits.o (tools/kernel_regs.py): the bits form's scan, the FIR kernel's nine
    instances and the stages' word-copy slicer; no private segment, no spilled register, at most 128 VGPRs.  The PCM forms'
    objects keep exactly their kernels (tests/test_runrs.py, test_runais.py, test_runpocsag.py)"""
    obj = os.path.join(ROOT, "tsl-sdr_amd", "build", "mfm_run_bits.o")
    assert os.path.exists(obj), "the build leaves tsl-sdr_amd/build/mfm_run_bits.o"
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm tools here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "vgpr" in ln]
    fir = [f"rrb_fir_kernel<{np_}>" for np_ in range(0, 33, 4)]
    assert sorted(ln.split()[0] for ln in lines) == sorted(fir + ["rrb_scan_kernel", "rb_slice_kernel"]), out
    for ln in lines:
        m = re.search(r"vgpr\s+(\d+) agpr\s+\d+ spill\s+(\d+) \| sgpr\s+\d+ spill\s+(\d+) \| lds\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(1)) <= 128 and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (0, 0, 0), ln


# ---- CPU: the resampler's twin --------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", tr.RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", tr.WINDOWS)
def test_hosttwin_bits_are_the_predicate_of_the_pcm_twin(pkg, W, ratio):
    """the ratios, windows, masks and cuts of tests/test_runrs.py, 1 and 3 channels, P = 0 and 2, invert, both polarities: every
    run's words are the packed predicate of the PCM twin's outputs (so the tail bits are 0), the word offsets the exclusive scan
    of (nr_out + 31) // 32; and a state that goes through PCM and bits calls in turn gives the same stream as either alone"""
    b = pkg.binding
    I, D, nr_taps = ratio
    i = 0
    for nch in (1, 3):
        for kind in tr.MASKS:
            for P in (0, 2):
                rng = np.random.RandomState(5 * W + I + 1000 * nch + 10 * tr.MASKS.index(kind) + P)
                full, invert = bool(i & 1), bool(i & 2)
                polarity = (NEG, POS)[(i >> 2) & 1]
                i += 1
                stream, mask, n, taps = tr.scene(rng, nch, W, kind, P, full, nr_taps)
                calls = tr.gate_calls(pkg, stream, mask, W, P, tr.make_cuts(rng, n, W, False))
                st = [b.hosttwin_runrs_state(nch, len(taps), I) for _ in range(3)]   # PCM alone, bits alone, in turn
                outs = words = 0
                for k, (gr, gp) in enumerate(calls):
                    what = f"W {W} {I}/{D} channels {nch} mask {kind} P {P} full {full} invert {invert} polarity {polarity}, call {k}"
                    pcm = b.hosttwin_runrs_call(W, taps, I, D, st[0][0], st[0][1], gr, gp, invert=invert)
                    want = pack(pkg, pcm[0], pcm[1], polarity)
                    assert want[0]["out_offset"].tolist() == np.concatenate([[0], np.cumsum((pcm[0]["nr_out"].astype(np.int64) + 31) // 32)])[:-1].tolist()
                    got = b.hosttwin_runrs_call_bits(W, taps, I, D, st[1][0], st[1][1], gr, gp, polarity, invert=invert)
                    same_bits(got, want, what)
                    for r in got[0]:   # the tail of a run's last word, stated on its own
                        nr = int(r["nr_out"])
                        if nr % 32:
                            assert int(got[1][int(r["out_offset"]) + nr // 32]) >> (nr % 32) == 0, what
                    if k % 2:
                        same_bits(b.hosttwin_runrs_call_bits(W, taps, I, D, st[2][0], st[2][1], gr, gp, polarity, invert=invert), want, what + " in turn")
                    else:
                        tr.same(b.hosttwin_runrs_call(W, taps, I, D, st[2][0], st[2][1], gr, gp, invert=invert), pcm, what + " in turn")
                    for s in st[1:]:
                        assert s[0].tobytes() == st[0][0].tobytes() and s[1].tobytes() == st[0][1].tobytes(), what
                    outs += pcm[1].size
                    words += got[1].size
                if kind == "open" and n // W * W > tr.plen_of(nr_taps, I):   # the stretch is long enough for an output
                    assert outs > 0 and words > 0
    assert i >= 8


def test_hosttwin_bits_refusals_leave_the_state(pkg):
    """a polarity that is none, a caller's array too small, a run list that is not a gate's: nothing is written, the state
    included, and the same input is right afterwards"""
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D = 4, 5
    calls = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    ref = b.hosttwin_runrs_state(nch, len(taps), I)
    state, pending = b.hosttwin_runrs_state(nch, len(taps), I)
    want = [pack(pkg, *b.hosttwin_runrs_call(W, taps, I, D, ref[0], ref[1], gr, gp), NEG) for gr, gp in calls]
    same_bits(b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *calls[0], NEG), want[0], "first call")
    s0, p0 = state.copy(), pending.copy()
    for polarity in (0, 3, 4):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *calls[1], polarity)
        assert ei.value.code == b.MFM_E_INVAL and "MFM_BITS_NEG or MFM_BITS_POS" in str(ei.value)
    assert len(want[1][0]) == 3 and want[1][1].size > 0
    for kw in (dict(max_runs=2), dict(max_words=want[1][1].size - 1)):
        with pytest.raises(pkg.MfmError) as ei:
            b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *calls[1], NEG, **kw)
        assert ei.value.code == b.MFM_E_NOMEM and ei.value.needed == (3, want[1][1].size)
    bad = calls[1][0].copy()
    bad["channel"][1] = nch
    with pytest.raises(pkg.MfmError) as ei:
        b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, bad, calls[1][1], NEG)
    assert ei.value.code == b.MFM_E_INVAL and "not a gate's" in str(ei.value)
    assert np.array_equal(state, s0) and np.array_equal(pending, p0)
    same_bits(b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *calls[1], NEG), want[1], "second call")


# ---- CPU: the stages' twins -----------------------------------------------------------------------------------

def _stage_scenes(pkg, W, stream, n, masks, taps, I, D, cuts_of, polarity, state_of, call_pcm, call_bits, same, what0):
    """every mask with P = 0 and 2 in the seeded cut: the resampler's and the stage's twins in the PCM form, in the bits form,
    and a third pair that takes the forms in turn.  Events equal call by call, and so does the stage's carried state"""
    b = pkg.binding
    events = 0
    for kind, mask_of in masks:
        for P in (0, 2):
            rng = np.random.RandomState(7 * W + I + 10 * len(kind) + P)
            mask = mask_of(rng)
            calls = tr.gate_calls(pkg, stream, mask, W, P, cuts_of(rng))
            rs = [b.hosttwin_runrs_state(stream.shape[0], len(taps), I) for _ in range(3)]
            st = [state_of(stream.shape[0]) for _ in range(3)]
            for k, (gr, gp) in enumerate(calls):
                what = f"{what0} mask {kind} P {P}, call {k}"
                pcm = b.hosttwin_runrs_call(W, taps, I, D, rs[0][0], rs[0][1], gr, gp)
                bits = b.hosttwin_runrs_call_bits(W, taps, I, D, rs[1][0], rs[1][1], gr, gp, polarity)
                want = call_pcm(st[0], *pcm)
                same(call_bits(st[1], *bits), want, what + ", bits")
                if k % 2:
                    turn = call_pcm(st[2], *b.hosttwin_runrs_call(W, taps, I, D, rs[2][0], rs[2][1], gr, gp))
                else:
                    turn = call_bits(st[2], *b.hosttwin_runrs_call_bits(W, taps, I, D, rs[2][0], rs[2][1], gr, gp, polarity))
                same(turn, want, what + ", in turn")
                assert st[1].tobytes() == st[0].tobytes() and st[2].tobytes() == st[0].tobytes(), what
                events += len(want)
    return events


@pytest.mark.parametrize("ratio", tra.RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", tra.WINDOWS)
def test_hosttwin_runais_bits_equal_the_pcm_twin(pkg, ora, W, ratio):
    """the scenes, masks and cuts of tests/test_runais.py"""
    b = pkg.binding
    I, D, _ = ratio
    sc = tra.scene(pkg, ratio)
    kinds = [k for k in tra.KINDS if k != "short" or W == 7]
    masks = [(k, (lambda rng, k=k: tra.make_mask(k, sc, W, rng))) for k in kinds]
    events = _stage_scenes(pkg, W, sc["stream"], sc["n_in"], masks, tra.rs_taps(pkg, ora, ratio), I, D,
                           lambda rng: tra.make_cuts(rng, sc["n_in"], W, tra.anchors_of(sc, ratio, W)), POS, b.hosttwin_runais_state,
                           b.hosttwin_runais_call, b.hosttwin_runais_call_bits, tra.same, f"AIS W {W} {I}/{D}")
    assert events >= 20


@pytest.mark.parametrize("ratio", trp.RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("W", trp.WINDOWS)
def test_hosttwin_runpocsag_bits_equal_the_pcm_twin(pkg, ora, W, ratio):
    """the scenes, masks and cuts of tests/test_runpocsag.py"""
    b = pkg.binding
    I, D, _ = ratio
    sc = trp.scene(pkg, ora, ratio, W)
    masks = [(k, (lambda rng, k=k: trp.make_mask(k, sc, W, rng))) for k in trp.kinds_of(W)]
    events = _stage_scenes(pkg, W, sc["stream"], sc["n_in"], masks, trp.rs_taps(pkg, ora, ratio), I, D,
                           lambda rng: tra.make_cuts(rng, sc["n_in"], W, trp.anchors_of(sc, W)), NEG, b.hosttwin_runpocsag_state,
                           b.hosttwin_runpocsag_call, b.hosttwin_runpocsag_call_bits, trp.same, f"POCSAG W {W} {I}/{D}")
    assert events >= 6


def test_hosttwin_runais_bits_handovers_at_any_sample(pkg, ora):
    """the hand-cut stretches of tests/test_runais.py (cuts on a preamble match, a packet end, runs of one sample and without
    output) in the bits form, against the oracle's events; the state equals the PCM twin's after every call"""
    b = pkg.binding
    calls, want = tra._pieces(pkg, ora)
    state, ref = b.hosttwin_runais_state(2), b.hosttwin_runais_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        tra.same(b.hosttwin_runais_call_bits(state, *pack(pkg, runs, payload, POS)), w, f"call {i}")
        b.hosttwin_runais_call(ref, runs, payload)
        assert state.tobytes() == ref.tobytes(), i


def test_hosttwin_runpocsag_bits_handovers_at_any_sample(pkg, ora):
    b = pkg.binding
    calls, want = trp._pieces(pkg, ora)
    state, ref = b.hosttwin_runpocsag_state(2), b.hosttwin_runpocsag_state(2)
    for i, ((runs, payload), w) in enumerate(zip(calls, want)):
        trp.same(b.hosttwin_runpocsag_call_bits(state, *pack(pkg, runs, payload, NEG)), w, f"call {i}")
        b.hosttwin_runpocsag_call(ref, runs, payload)
        assert state.tobytes() == ref.tobytes(), i


def _stage_refusals(pkg, calls, want, at, state_of, call_bits, same, right, wrong, bad_runs, slots_of):
    """the refusals of a stage's bits entry on the call `at` of hand-cut stretches: each leaves the state, and the same call is
    right afterwards"""
    b = pkg.binding
    state = state_of(2)
    for i in range(at):
        same(call_bits(state, *pack(pkg, *calls[i], right)), want[i], f"call {i}")
    s0 = state.copy()
    runs, bits = pack(pkg, *calls[at], right)
    nout = int(runs["nr_out"].sum())
    with pytest.raises(pkg.MfmError) as ei:   # the other stage's polarity, and none
        call_bits(state, runs, bits, polarity=wrong)
    assert ei.value.code == b.MFM_E_INVAL and "needs MFM_BITS_" in str(ei.value)
    with pytest.raises(pkg.MfmError) as ei:
        call_bits(state, runs, bits, polarity=0)
    assert ei.value.code == b.MFM_E_INVAL and "needs MFM_BITS_" in str(ei.value)

    def changed(field, k, value):
        r = runs.copy()
        r[field][k] = value
        return r

    last_words = (int(runs["nr_out"][1]) + 31) // 32
    assert len(runs) == 2 and int(runs["out_offset"][1]) + last_words == bits.size
    cases = [
        # a word range beyond the totals: by offset, by one word through nr_out, and with totals that leave the last word out;
        # in the last case the bit array handed over ends where the totals say, so a read of the refused range would be seen
        (dict(runs=changed("out_offset", 1, int(runs["out_offset"][1]) + 1)), bits, "does not exist", bad_runs << 8),
        (dict(runs=changed("nr_out", 1, 32 * last_words + 1)), bits, "does not exist", bad_runs << 8),
        (dict(totals=[2, bits.size - 1, 0, 0]), bits[:-1], "does not exist", bad_runs << 8),
        (dict(totals=[2, bits.size, 1, 0]), bits, "overflow or gate error", 1 << 8),
        (dict(runs=changed("first_out", 0, int(runs["first_out"][0]) + 1)), bits, "out of step", 2 << 8),
        (dict(max_out_samples=nout - 1), bits, "max_out_samples", bad_runs << 8),       # the sum of nr_out is still bounded
        (dict(totals=[2, nout // 32 + 3, 0, 0]), bits, "max_out_samples", bad_runs << 8),   # totals[1] beyond max_out_samples / 32 + max_runs
        (dict(max_runs=1, max_out_samples=nout + 64), bits, "max_runs", 1),
        (dict(max_events=slots_of(runs) - 1), bits, "event bound", 2),
    ]
    for change, bw, message, flags in cases:
        kw = dict(runs=runs)
        kw.update(change)
        with pytest.raises(pkg.MfmError) as ei:
            call_bits(state, kw.pop("runs"), bw, **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value) and ei.value.flags == flags, (change, str(ei.value), ei.value.flags)
        assert ei.value.needed == 0 and state.tobytes() == s0.tobytes()
    same(call_bits(state, runs, bits, max_events=slots_of(runs)), want[at], "the same call, right")
    for i in range(at + 1, len(calls)):
        same(call_bits(state, *pack(pkg, *calls[i], right)), want[i], f"call {i}")


def test_hosttwin_runais_bits_refuses_and_leaves_its_state(pkg, ora):
    b = pkg.binding
    calls, want, at, _, _, _ = tra._refusal_case(pkg, ora)
    _stage_refusals(pkg, calls, want, at, b.hosttwin_runais_state, b.hosttwin_runais_call_bits, tra.same, POS, NEG, b.MFM_RUNAIS_IN_BAD_RUNS,
                    lambda runs: int((runs["nr_out"] // 160 + 1).sum()))


def test_hosttwin_runpocsag_bits_refuses_and_leaves_its_state(pkg, ora):
    b = pkg.binding
    calls, want, at, _, _, _ = trp._refusal_case(pkg, ora)
    _stage_refusals(pkg, calls, want, at, b.hosttwin_runpocsag_state, b.hosttwin_runpocsag_call_bits, trp.same, NEG, POS,
                    b.MFM_RUNPOCSAG_IN_BAD_RUNS, lambda runs: sum(trp.slots(n) for n in runs["nr_out"]))


# ---- the edges of the resampler's bits kernel -------------------------------------------------------------------

EDGES = ("zero", "lt32", "mod64_0", "mod64_1", "mod64_63", "n1024", "n1025", "gt2048", "two_runs", "continues")
EDGE_OF = {
    "zero": lambda n: n == 0,
    "lt32": lambda n: 1 <= n <= 31,
    "mod64_0": lambda n: n > 0 and n % 64 == 0 and n % 1024 != 0,
    "mod64_1": lambda n: n % 64 == 1 and n % 1024 != 1,
    "mod64_63": lambda n: n % 64 == 63,
    "n1024": lambda n: n == 1024,
    "n1025": lambda n: n == 1025,
    "gt2048": lambda n: n > 2048 and n % 1024 != 0,   # several workgroups and a partial last one
}
# interpolate, decimate, taps, W: the issue's shape with the taps of tests/test_runrs.py, a tap count whose phase is too long
# for registers (plen 68: the LDS instance), and W = 1, where a run of whole windows can have any number of outputs
SHAPES = [(4, 5, 81, 64), (16, 25, 821, 64), (4, 5, 269, 64), (4, 5, 81, 1), (16, 25, 821, 1)]
# what a run of whole windows cannot be at W = 64 (the module's docstring); everything else must be there
CANNOT = {(4, 5, 81, 64): {"zero", "lt32", "mod64_1", "mod64_63", "n1025"}, (16, 25, 821, 64): {"zero", "mod64_1", "mod64_63", "n1025"},
          (4, 5, 269, 64): {"lt32", "mod64_1", "mod64_63", "n1025"}, (4, 5, 81, 1): set(), (16, 25, 821, 1): set()}
FIR_INSTANCE = {(4, 5, 81): 12, (16, 25, 821): 28, (4, 5, 269): 0}   # NP of rr_geometry: register pairs, 0 = pairs read from LDS


def total(I, D, plen, W, n):
    """outputs of a stretch of n whole windows through a fresh resampler (csrc/mfm_runrs.h, restated)"""
    s = n * W
    return 0 if s <= plen else ((s - plen) * I - 1) // D + 1


def edges_of(nr_outs, channels, continues):
    have = {e for e, pred in EDGE_OF.items() if any(pred(int(n)) for n in nr_outs)}
    if len(set(channels)) < len(channels):
        have.add("two_runs")
    if continues:
        have.add("continues")
    return have


def plan_case(shape):
    """a mask [3][A + B] and the cut [A W, B W]: the second call holds a run for every edge the shape can produce.  An edge is
    looked for as a run that begins in the second call (n windows) and, failing that, as one that continues a stretch of `a`
    windows of the first call (at most one per channel); exhaustively up to 5200 samples per run, which is past every edge"""
    I, D, nr_taps, W = shape
    plen = tr.plen_of(nr_taps, I)
    nmax = 5200 // W
    begin, cont, cannot = [], [], set()
    for e in EDGES[:8]:
        n = next((n for n in range(1, nmax + 1) if EDGE_OF[e](total(I, D, plen, W, n))), None)
        if n is not None:
            begin.append(n)
            continue
        ab = next(((a, bb) for a in range(1, 41) for bb in range(1, nmax + 1)
                   if EDGE_OF[e](total(I, D, plen, W, a + bb) - total(I, D, plen, W, a))), None)
        if ab is None or len(cont) == 3:
            cannot.add(e)
        else:
            cont.append(ab)
    if not cont:
        cont.append((2, 3))
    A = max(a for a, _ in cont) + 2
    at = [A] * 3   # next free window of each channel in the second call
    spans = []
    for c, (a, bb) in enumerate(cont):
        spans.append((c, A - a, A + bb))
        at[c] = A + bb + 1
    for n in sorted(begin, reverse=True):   # the longest first, each on the channel that is shortest so far
        c = int(np.argmin(at))
        spans.append((c, at[c], at[c] + n))
        at[c] += n + 1
    spans.append((0, at[0], at[0] + 1))   # and one window more behind the runs of channel 0: two runs of one channel for certain
    at[0] += 2
    B = max(at) - A
    mask = np.zeros((3, A + B), bool)
    for c, k0, k1 in spans:
        mask[c, k0:k1] = True
    return mask, [A * W, B * W], cannot


def test_the_planned_calls_hold_every_edge_the_shapes_can_produce(pkg):
    """plan_case on every shape, through the PCM twin: the second call's runs show every edge but those the docstring rules out
    for W = 64, each W = 1 shape shows all of them in one call, and the tap counts pick the instances they are meant to"""
    b = pkg.binding
    for shape in SHAPES:
        I, D, nr_taps, W = shape
        mask, cuts, cannot = plan_case(shape)
        assert cannot == CANNOT[shape], (shape, cannot)
        rng = np.random.RandomState(nr_taps + W)
        stream = rng.randint(-32768, 32768, size=(3, sum(cuts))).astype(np.int16)
        taps = rng.randint(-8191, 8192, nr_taps).astype(np.int16)
        calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
        state, pending = b.hosttwin_runrs_state(3, nr_taps, I)
        b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[0])
        runs, _ = b.hosttwin_runrs_call(W, taps, I, D, state, pending, *calls[1])
        have = edges_of(runs["nr_out"], runs["channel"].tolist(), bool(((runs["flags"] & 1) == 0).any()))
        assert have == set(EDGES) - cannot, (shape, sorted(set(EDGES) - cannot - have))
    assert set().union(*[set(EDGES) - CANNOT[s] for s in SHAPES if s[3] == 64]) == set(EDGES) - {"n1025", "mod64_1", "mod64_63"}
    for (I, D, nr_taps), np_ in FIR_INSTANCE.items():
        plen = tr.plen_of(nr_taps, I)
        assert ((plen // 2 + 3) // 4 * 4 if (256 * D) % I == 0 and plen // 2 <= 32 else 0) == np_


# ---- GPU ------------------------------------------------------------------------------------------------------

def _hip():
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return rt


@pytest.mark.gpu
@pytest.mark.parametrize("polarity", [NEG, POS], ids=["neg", "pos"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}_{s[1]}_taps{s[2]}_W{s[3]}")
def test_gpu_resampler_bits_equal_the_twin_bit_for_bit(pkg, shape, polarity):
    """3 channels through a real Gate; the first call leaves stretches open, the second holds the planned edges (asserted on what
    the device returned).  The bit payload is filled with 0xFF before the second call: every word a run owns is compared whole,
    which checks the zero tails, and every word behind totals[1] is still 0xFF.  invert is on for the 16/25 shapes"""
    b = pkg.binding
    I, D, nr_taps, W = shape
    invert = I == 16
    mask, cuts, cannot = plan_case(shape)
    rng = np.random.RandomState(nr_taps + W)
    stream = rng.randint(-32768, 32768, size=(3, sum(cuts))).astype(np.int16)
    taps = rng.randint(-8191, 8192, nr_taps).astype(np.int16)
    calls = tr.gate_calls(pkg, stream, mask, W, 0, cuts)
    state, pending = b.hosttwin_runrs_state(3, nr_taps, I)
    gate = pkg.Gate(3, max(cuts), W)
    rr = pkg.RunResampler(3, taps, I, D, W, max_in_samples=max(cuts), invert=invert)
    max_runs, max_words = rr.bits_capacity()
    assert (max_runs, max_words) == (rr.capacity()[0], rr.capacity()[1] // 32 + rr.capacity()[0])
    rt, pos = _hip(), 0
    for i, m in enumerate(cuts):
        want = b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *calls[i], polarity, invert=invert)
        tg.same(gate.process_host(stream[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W)), calls[i], f"the gate's call {i}")
        pos += m
        if i == 1:
            view = rr.bits_view()   # the payload's address, from the first call; that call has been fetched, so nothing is queued
            assert rt.hipMemset(view.d_bits, 0xff, max_words * 4) == 0 and rt.hipDeviceSynchronize() == 0
        rr.process_bits_device(*gate.device_view(), polarity)
        got = rr.fetch_bits()
        same_bits(got, want, f"call {i}")
        view = rr.bits_view()
        assert view.polarity == polarity and view.reserved == 0
        assert tl._d2h(view.d_totals, 32).view(np.uint64).tolist() == [len(want[0]), want[1].size, 0, 0]
    whole = tl._d2h(view.d_bits, max_words * 4).view(np.uint32)
    assert np.array_equal(whole[:want[1].size], want[1]) and want[1].size < max_words
    assert (whole[want[1].size:] == 0xffffffff).all()
    runs = got[0]
    have = edges_of(runs["nr_out"], runs["channel"].tolist(), bool(((runs["flags"] & 1) == 0).any()))
    assert have == set(EDGES) - CANNOT[shape], (shape, sorted(set(EDGES) - CANNOT[shape] - have))
    assert runs["out_offset"].tolist() == np.concatenate([[0], np.cumsum((runs["nr_out"].astype(np.int64) + 31) // 32)])[:-1].tolist()
    for e in (rr, gate):
        e.close()


def _fed_bits(pkg, torch, rr, gr, gp, polarity, totals=None):
    """one bits call from uploaded arrays: a gate's result as it would stand in its device view"""
    t = np.array([len(gr), gp.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, gr), tr._up(torch, gp), tr._up(torch, t))
    rr.process_bits_device(*(k.data_ptr() for k in keep), polarity)
    try:
        return rr.fetch_bits()
    finally:
        del keep


@pytest.mark.gpu
def test_gpu_resampler_bits_refusals_and_accessors(pkg):
    """a polarity that is none is refused at the call; a call that does not fit max_windows raises the flag, writes nothing and
    leaves the state, so the same windows in calls that fit are right; after a bits call the PCM accessors answer MFM_E_STATE and
    after a PCM call the bits accessors do; PCM and bits calls in turn continue one stretch"""
    import torch
    b = pkg.binding
    W, nch, stream, mask, taps = tr._small_case(pkg)
    I, D = 4, 5
    first, second = tr.gate_calls(pkg, stream, mask, W, 0, [12, 18])
    whole = tr.gate_calls(pkg, stream, mask, W, 0, [30])[0]
    state, pending = b.hosttwin_runrs_state(nch, len(taps), I)
    rr = pkg.RunResampler(nch, taps, I, D, W, max_windows=4, max_runs=8)
    with pytest.raises(pkg.MfmError) as ei:   # before any call there is no bits result to look at
        rr.bits_view()
    assert ei.value.code == b.MFM_E_STATE
    for polarity in (0, 3):
        with pytest.raises(pkg.MfmError) as ei:
            rr.process_bits_device(1, 1, 1, polarity)
        assert ei.value.code == b.MFM_E_INVAL and "MFM_BITS_NEG or MFM_BITS_POS" in str(ei.value)
    with pytest.raises(pkg.MfmError) as ei:
        _fed_bits(pkg, torch, rr, *whole, NEG)
    assert ei.value.code == b.MFM_E_STATE and "max_windows or max_runs" in str(ei.value)
    assert ei.value.needed == (0, 0) and not ei.value.buffers[0].view(np.uint8).any() and not ei.value.buffers[1].any()
    same_bits(_fed_bits(pkg, torch, rr, *first, NEG), b.hosttwin_runrs_call_bits(W, taps, I, D, state, pending, *first, NEG), "first call")
    for fn in (rr.fetch, rr.device_view):   # no PCM was written
        with pytest.raises(pkg.MfmError) as ei:
            fn()
        assert ei.value.code == b.MFM_E_STATE and "mfm_runrs_fetch_bits or mfm_runrs_bits_view" in str(ei.value)
    # the stretch of channel 1 goes on in a PCM call
    want = b.hosttwin_runrs_call(W, taps, I, D, state, pending, *second)
    assert [int(f) for f in want[0]["flags"]] == [0, 1, 1]
    t = np.array([len(second[0]), second[1].size, 0, 0], np.uint64)
    keep = (tr._up(torch, second[0]), tr._up(torch, second[1]), tr._up(torch, t))
    rr.process_device(*(k.data_ptr() for k in keep))
    tr.same(rr.fetch(), want, "second call, PCM")
    assert len(rr.device_view()) == 3
    for fn in (rr.fetch_bits, rr.bits_view):
        with pytest.raises(pkg.MfmError) as ei:
            fn()
        assert ei.value.code == b.MFM_E_STATE and "mfm_runrs_fetch or mfm_runrs_device_view" in str(ei.value)
    del keep
    rr.close()


def _chains(pkg, stage, nch, taps, I, D, W, P, cap, polarity):
    """three chains burst resampler -> stage behind one gate: PCM, bits, and the two forms in turn"""
    rrs = [pkg.RunResampler(nch, taps, I, D, W, max_in_samples=cap, preroll_windows=P) for _ in range(3)]
    sts = [stage.behind(rr) for rr in rrs]

    def run(i, view):
        out = []
        for k, (rr, st) in enumerate(zip(rrs, sts)):
            if k == 0 or (k == 2 and i % 2 == 0):
                rr.process_device(*view)
                st.process_device(*rr.device_view())
            else:
                rr.process_bits_device(*view, polarity)
                st.process_bits_device(rr.bits_view())
            out.append(st.fetch())
        return out

    def close():
        for o in sts + rrs:
            o.close()

    return run, close, sts


def _gpu_stage_chain(pkg, ora, Checker, same, stage, polarity, stream, n, mask, W, P, taps, I, D, cuts, what):
    """gate -> burst resampler -> stage on the device in the three chains, every call against the oracle chain"""
    calls = tr.gate_calls(pkg, stream, mask, W, P, cuts)
    chk = Checker(pkg, ora, taps, I, D, W)
    want = [chk.call(gr, gp) for gr, gp in calls]
    chk.stretches()
    nch, cap = stream.shape[0], max(max(cuts), 1)
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    run, close, sts = _chains(pkg, stage, nch, taps, I, D, W, P, cap, polarity)
    pos, events = 0, 0
    for i, (_, ev_want) in enumerate(want):
        if i < len(cuts):
            m = cuts[i]
            gate.process_host(stream[:, pos:pos + m], tg.records_of(pkg, mask, pos // W, (pos + m) // W))
            pos += m
        else:
            gate.flush_device()
        for name, got in zip(("PCM", "bits", "in turn"), run(i, gate.device_view())):
            same(got, ev_want, f"{what}, call {i}, {name}")
        events += len(ev_want)
    if hasattr(sts[0], "fetch_state"):
        states = [s.fetch_state().tobytes() for s in sts]
        assert states[1] == states[0] and states[2] == states[0]
    close()
    gate.close()
    return events


@pytest.mark.gpu
def test_gpu_chain_runais_bits_equals_the_pcm_chain_and_the_oracle(pkg, ora):
    """the 1/1 scene of tests/test_runais.py at W = 64 with the mask that closes and opens inside packets, P = 2 with the flush, in
    the seeded cut: the PCM chain, the bits chain and a chain that takes the forms call by call in turn give the oracle's events"""
    ratio, W, P = tra.RATIOS[1], 64, 2
    sc = tra.scene(pkg, ratio)
    rng = np.random.RandomState(41)
    mask = tra.make_mask("cut", sc, W, rng)
    cuts = tra.make_cuts(rng, sc["n_in"], W, tra.anchors_of(sc, ratio, W))
    events = _gpu_stage_chain(pkg, ora, tra.Checker, tra.same, pkg.RunAis, POS, sc["stream"], sc["n_in"], mask, W, P, tra.rs_taps(pkg, ora, ratio),
                              1, 1, cuts, "AIS")
    assert events >= 5 and len(cuts) >= 10


@pytest.mark.gpu
def test_gpu_chain_runpocsag_bits_equals_the_pcm_chain_and_the_oracle(pkg, ora):
    """the 1/1 scene of tests/test_runpocsag.py at W = 7 (its shortest) with the mask that closes and opens inside batches, P = 2
    with the flush, in the seeded cut; the three chains also leave the same per-channel state"""
    ratio, W, P = trp.RATIOS[1], 7, 2
    sc = trp.scene(pkg, ora, ratio, W)
    rng = np.random.RandomState(43)
    mask = trp.make_mask("cut", sc, W, rng)
    cuts = tra.make_cuts(rng, sc["n_in"], W, trp.anchors_of(sc, W))
    events = _gpu_stage_chain(pkg, ora, trp.Checker, trp.same, pkg.RunPocsag, NEG, sc["stream"], sc["n_in"], mask, W, P,
                              trp.rs_taps(pkg, ora, ratio), 1, 1, cuts, "POCSAG")
    assert events >= 3 and len(cuts) >= 10


def _view_of(pkg, torch, runs, bits, polarity, totals=None):
    t = np.array([len(runs), bits.size, 0, 0] if totals is None else totals, np.uint64)
    keep = (tr._up(torch, runs), tr._up(torch, bits), tr._up(torch, t))
    return pkg.RunrsBitsView(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), polarity, 0), keep


@pytest.mark.gpu
@pytest.mark.parametrize("proto", ["ais", "pocsag"])
def test_gpu_stage_bits_refusals_leave_the_state(pkg, ora, proto):
    """the other stage's polarity is refused at the call; a word range beyond the totals and the resampler's flags come back as
    the PCM entry's flags with nothing written; the state stays, so the same call fed right is right, and so are the calls
    behind it, PCM and bits in turn"""
    import torch
    b = pkg.binding
    mod, stage, right, wrong = (tra, pkg.RunAis, POS, NEG) if proto == "ais" else (trp, pkg.RunPocsag, NEG, POS)
    calls, want, at, _, _, _ = mod._refusal_case(pkg, ora)
    st = stage(2, 4, max(p.size for _, p in calls) + 1)

    def fed(i, form, **kw):
        runs, payload = calls[i]
        if form == "pcm":
            return mod._fed(pkg, torch, st, runs, payload)
        runs, bits = pack(pkg, runs, payload, right)
        view, keep = _view_of(pkg, torch, kw.get("runs", runs), bits, kw.get("polarity", right), kw.get("totals"))
        st.process_bits_device(view)
        try:
            return st.fetch()
        finally:
            del keep

    for i in range(at):
        mod.same(fed(i, "bits" if i % 2 else "pcm"), want[i], f"call {i}")
    with pytest.raises(pkg.MfmError) as ei:
        fed(at, "bits", polarity=wrong)
    assert ei.value.code == b.MFM_E_INVAL and "needs MFM_BITS_" in str(ei.value)
    runs, bits = pack(pkg, *calls[at], right)
    beyond = runs.copy()
    beyond["out_offset"][1] += 1
    longer = runs.copy()
    longer["nr_out"][1] = 32 * ((int(runs["nr_out"][1]) + 31) // 32) + 1
    for kw, message in ((dict(runs=beyond), "does not exist"), (dict(runs=longer), "does not exist"),
                        (dict(totals=[2, bits.size - 1, 0, 0]), "does not exist"), (dict(totals=[2, bits.size, 0, 2]), "overflow or gate error")):
        with pytest.raises(pkg.MfmError) as ei:
            fed(at, "bits", **kw)
        assert ei.value.code == b.MFM_E_STATE and message in str(ei.value), (kw, str(ei.value))
        assert ei.value.needed == 0 and not ei.value.buffer.view(np.uint8).any()
    for i in range(at, len(calls)):
        mod.same(fed(i, "pcm" if i % 2 else "bits"), want[i], f"call {i} behind the refused ones")
    st.close()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_gate_bits_writes_the_same_events(pkg, ora, tmp_path):
    """tools/level_scan.py ... --gate-ais --gate-bits on the chain scene of tests/test_runais.py writes the ais.jsonl of the run
    without --gate-bits, the same lines in resampled.jsonl but for file_offset, and no resampled PCM; --gate-bits is refused
    without a stage that reads bits and beside --gate-flex"""
    sc, s = tra._chain(pkg, ora), tra.CHAIN
    fs, decim, W, P = s["fs"], s["decim"], s["W"], s["P"]
    centre = 162000000
    (tmp_path / "capture.bin").write_bytes(sc["iq"].tobytes())
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": sc["lpf"]}))
    (tmp_path / "rx.json").write_text(json.dumps({
        "device": {"type": "file", "filename": str(tmp_path / "capture.bin"), "fileFormat": "cs16"},
        "sampleRateHz": fs, "centerFreqHz": centre, "nrSampBufs": 16, "decimationFactor": decim, "lpfTaps": [float(t) for t in sc["taps"]],
        "channels": [{"outFifo": "/dev/null", "chanCenterFreq": centre + int(o)} for o in sc["offs"]]}))

    def cmd(out, *more):
        return [sys.executable, os.path.join(ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input",
                str(tmp_path / "capture.bin"), "--format", "cs16", "--form", "pcm", "--window", str(W), "--open-thr", str(sc["thr"]),
                "--hang", "1", "--block", str(s["blk"]), "--gate-out", str(tmp_path / out), "--gate-preroll", str(P),
                "--gate-resample", "1/1", "--resample-taps", str(tmp_path / "filter.json")] + list(more)

    for out, more in (("pcm", ("--gate-ais",)), ("bits", ("--gate-ais", "--gate-bits"))):
        r = subprocess.run(cmd(out, *more), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    ais = [(tmp_path / d / "ais.jsonl").read_text() for d in ("pcm", "bits")]
    assert ais[0] == ais[1] and len(ais[0].splitlines()) >= 5
    lines = [[json.loads(ln) for ln in (tmp_path / d / "resampled.jsonl").read_text().splitlines()] for d in ("pcm", "bits")]
    assert [{k: v for k, v in ln.items() if k != "file_offset"} for ln in lines[0]] == lines[1] and lines[1]
    assert (tmp_path / "pcm" / "index.jsonl").read_text() == (tmp_path / "bits" / "index.jsonl").read_text()
    assert any(f.endswith(".rs.s16") for f in os.listdir(tmp_path / "pcm")) and not any(f.endswith(".rs.s16") for f in os.listdir(tmp_path / "bits"))
    for more, message in ((("--gate-bits",), "--gate-bits needs --gate-ais or --gate-pocsag"),
                          (("--gate-flex", "--gate-bits"), "--gate-bits and --gate-flex exclude each other")):
        r = subprocess.run(cmd("refused", *more), capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
