"""The sign-bit path from the resampler to the POCSAG and AIS stages: mfm_resampler_process_bits_* leaves one packed
predicate bit per output (sample < 0 for POCSAG, sample > 0 for AIS) instead of PCM, mfm_pocsag_process_bits_device /
mfm_ais_process_bits_device splice those bits into the stage's window in the place of the slicer.

Expected values come from the oracles (oracle_lib.Resampler / oracle_lib.Pocsag, ais_ref), never from the PCM path of
the code under test; everything is compared bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ais_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tsl-sdr_amd", "host")
NEW_NAMES = ["mfm_resampler_process_bits_device", "mfm_resampler_process_bits_host_to_device", "mfm_resampler_process_bits_host",
             "mfm_pocsag_process_bits_device", "mfm_ais_process_bits_device", "mfm_hosttwin_splice_bits"]
NEG, POS = 1, 2


# ---- CPU ---------------------------------------------------------------------------------------------------

def _bits_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")


def _words_of(bits):
    pad = (-len(bits)) % 32
    return np.packbits(np.concatenate([bits, np.zeros(pad, np.uint8)]), bitorder="little").view("<u4")


@pytest.mark.parametrize("nr_bits", [0, 1, 31, 32, 33, 511, 512, 513, 4097])
def test_hosttwin_splice_equals_numpy_restatement(pkg, nr_bits):
    """the per-word splice the kernel runs (csrc/mfm_bits.h), through its host twin: bits below off0 kept, bits in
    [off0, off0 + nr_bits) from the source, the rest of the last touched word zero, no word beyond it touched"""
    rng = np.random.RandomState(nr_bits)
    for base in (0, 64, 4096):
        for r in range(32):
            off0 = base + r
            src_bits = rng.randint(0, 2, nr_bits).astype(np.uint8)
            src = _words_of(src_bits) if nr_bits else np.zeros(0, "<u4")
            if src.size:  # what lies behind the last bit of the source must not matter
                junk = src.copy()
                if nr_bits % 32:
                    junk[-1] |= np.uint32((0xFFFFFFFF << (nr_bits % 32)) & 0xFFFFFFFF)
            else:
                junk = src
            nwin = (off0 + nr_bits + 31) // 32 + 3
            window = np.full(nwin, 0xFFFFFFFF, "<u4")
            want_bits = _bits_of(window)
            if nr_bits:
                last = (off0 + nr_bits - 1) // 32
                want_bits = np.concatenate([want_bits[:off0], src_bits, np.zeros(32 * (last + 1) - off0 - nr_bits, np.uint8),
                                            want_bits[32 * (last + 1):]])
            want = _words_of(want_bits)
            for s in (src, junk):
                got = pkg.binding.hosttwin_splice_bits(window, off0, s, nr_bits)
                assert np.array_equal(got, want), (off0, nr_bits)


def test_header_declares_and_library_exports_the_new_names(pkg):
    src = open(os.path.join(ROOT, "include", "multifm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load_library()
    for n in NEW_NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in pkg.binding.ABI_SYMBOLS
    assert re.search(r"#define\s+MFM_BITS_NEG\s+1u", src) and re.search(r"#define\s+MFM_BITS_POS\s+2u", src)
    assert re.search(r"#define\s+MFM_ABI_VERSION\s+4\b", src)
    assert (pkg.binding.MFM_BITS_NEG, pkg.binding.MFM_BITS_POS) == (NEG, POS)
    assert C.sizeof(pkg.BitsView) == 32


@pytest.mark.parametrize("tool,extra", [("decoder_amd", ["-m", "POCSAG", "-b"]), ("aisdecoder_amd", ["-b"]),
                                        ("decoder_amd", ["-m", "FLEX"]), ("decoder_amd", [])])
def test_programs_refuse_sign_bits_with_dc_blocker_or_flex(tmp_path, tool, extra):
    """-s with -b (the DC blocker filters the resampled PCM) or with FLEX (four-level slicer, the default protocol of
    decoder_amd): a fatal message and a non-zero exit, before any device is touched"""
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": [0.25, 0.5, 0.25]}))
    (tmp_path / "in.pcm").write_bytes(b"\0" * 64)
    r = subprocess.run([os.path.join(HOST_DIR, tool), "-I", "1", "-D", "1", "-S", "48000", "-F", str(tmp_path / "filter.json"),
                        "-f", "929612500", "-s"] + extra + [str(tmp_path / "in.pcm")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "BAD-SIGN-BIT-PATH" in r.stdout + r.stderr and "(-s)" in r.stdout + r.stderr


# ---- GPU: the resampler's second output form ------------------------------------------------------------------

def _design(pkg, ntaps, interp, decim):
    return pkg.synth.design_lpf(ntaps, 0.45 / max(interp, decim), 1.0) * interp


def _input_with_runs(rng, nch, n):
    """full-range noise with runs of exact zeros and of -32768 in every channel, so that the resampled stream holds
    zeros, negatives and positives: < 0, > 0 and >= 0 are three different planes"""
    x = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
    for c in range(nch):
        for k in range(3):
            a = int(rng.randint(0, n - n // 8))
            x[c, a:a + n // 10] = 0 if (k + c) % 2 == 0 else -32768
    x[:, n // 2:n // 2 + n // 12] = 0
    x[:, n // 4:n // 4 + n // 16] = -32768
    return x


def _planes(y):
    return (y < 0), (y > 0), (y >= 0)


def _pack_rows(pred):
    return np.stack([_words_of(row.astype(np.uint8)) for row in pred]) if pred.shape[1] else np.zeros((pred.shape[0], 0), "<u4")


SIZES = [1, 1000, 1, 1, 1, 1, 7, 4096, 100, 8192, 2048, 33, 517, 6001]
UNITY_TAPS = [0.25, 0.5, 0.25]  # the filter tests/test_ais.py gives aisdecoder_amd at 1/1


@pytest.mark.gpu
@pytest.mark.parametrize("interp,decim,ntaps,force_dot2", [(4, 5, 81, False), (4, 5, 81, True), (16, 25, 821, False),
                                                           (16, 25, 821, True), (1, 1, 3, False), (1, 1, 3, True), (3, 7, 60, False)])
def test_gpu_resampler_bits_equal_packed_oracle_predicates(pkg, ora, interp, decim, ntaps, force_dot2):
    """4/5 (POCSAG, the AIS device-path test), 16/25, 1/1 (aisdecoder test) on the matrix form and again on the v_dot2 form,
    3/7 which the matrix form does not take; 1, 3, 64 and 1024 channels; invert on and off; ragged calls with 0 outputs,
    1 output, counts that are no multiple of 32 or 256; bits behind the last output of a call are 0"""
    taps = ora.quantize_taps(UNITY_TAPS if (interp, decim) == (1, 1) else _design(pkg, ntaps, interp, decim))
    for nch in (1, 3, 64, 1024):
        n = 40000 if nch <= 64 else 12000
        rng = np.random.RandomState(1000 * interp + decim + nch)
        x = _input_with_runs(rng, nch, n)
        for invert, pol in ((False, NEG), (False, POS), (True, NEG), (True, POS)):
            if nch >= 64 and invert != (pol == POS):
                continue  # the wide shapes: one polarity each way
            want = np.stack([ora.Resampler(taps, interp, decim, invert=invert).feed(x[c]) for c in range(nch)])
            neg, pos, nonneg = _planes(want)
            assert (neg != ~nonneg).sum() == 0 and (pos != nonneg).any() and (neg != pos).any() and neg.any() and pos.any(), \
                "the oracle's PCM must tell the three predicates apart"
            gpu = pkg.Resampler(nch, taps, interp, decim, 8192, device=0, invert=invert, force_dot2=force_dot2)
            pos_in, pos_out, k, counts = 0, 0, 0, []
            while pos_in < n:
                m = min(SIZES[k % len(SIZES)], n - pos_in)
                words, nb = gpu.process_bits_host(x[:, pos_in:pos_in + m], pol)
                seg = want[:, pos_out:pos_out + nb]
                assert seg.shape[1] == nb, "more outputs than the oracle has"
                exp = _pack_rows(seg < 0 if pol == NEG else seg > 0)
                assert words.shape == exp.shape and np.array_equal(words, exp), \
                    f"{nch} channels, invert={invert}, polarity={pol}, call {k} ({m} in, {nb} out)"
                counts.append(nb)
                pos_in += m
                pos_out += nb
                k += 1
            gpu.close()
            assert pos_out == want.shape[1]
            assert 0 in counts and 1 in counts and any(c % 32 for c in counts) and any(c % 256 and c > 256 for c in counts)


def _device_rows(ptr, stride_elems, n_elems, nch, dtype):
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    rt.hipDeviceSynchronize()
    host = np.zeros((nch, max(n_elems, 1)), dtype)
    isz = host.itemsize
    if n_elems:
        assert rt.hipMemcpy2D(host.ctypes.data, host.shape[1] * isz, ptr, stride_elems * isz, n_elems * isz, nch, 2) == 0
    return host[:, :n_elems]


@pytest.mark.gpu
@pytest.mark.parametrize("interp,decim,ntaps,force_dot2", [(4, 5, 81, False), (4, 5, 81, True), (3, 7, 60, False)])
def test_gpu_pcm_calls_and_bits_calls_alternate_on_one_resampler(pkg, ora, interp, decim, ntaps, force_dot2):
    import torch
    nch, n = 5, 60000
    rng = np.random.RandomState(9)
    x = _input_with_runs(rng, nch, n)
    taps = ora.quantize_taps(_design(pkg, ntaps, interp, decim))
    want = np.stack([ora.Resampler(taps, interp, decim).feed(x[c]) for c in range(nch)])
    gpu = pkg.Resampler(nch, taps, interp, decim, 8192, device=0, force_dot2=force_dot2)
    d = torch.from_numpy(x).cuda()
    pos_in, pos_out, k, kinds = 0, 0, 0, rng.randint(0, 3, 1000)
    while pos_in < n:
        m = min(int(rng.choice([1, 5, 333, 4096, 8192, 1000])), n - pos_in)
        if kinds[k] == 0:
            yptr, ystride, ny = gpu.process_device(d.data_ptr() + 2 * pos_in, n, m)
            got = _device_rows(yptr, ystride, ny, nch, np.int16)
            assert np.array_equal(got, want[:, pos_out:pos_out + ny]), f"PCM call {k}"
        else:
            pol = NEG if kinds[k] == 1 else POS
            v = gpu.process_bits_device(d.data_ptr() + 2 * pos_in, n, m, pol)
            ny = v.nr_bits
            assert v.polarity == pol and v.reserved == 0
            got = _device_rows(v.d_bits, v.stride_words, (ny + 31) // 32, nch, np.uint32)
            seg = want[:, pos_out:pos_out + ny]
            assert seg.shape[1] == ny and np.array_equal(got, _pack_rows(seg < 0 if pol == NEG else seg > 0)), f"bits call {k}"
        pos_in += m
        pos_out += ny
        k += 1
    gpu.close()
    assert pos_out == want.shape[1] and len(set(kinds[:k])) == 3


@pytest.mark.gpu
def test_gpu_refusals_leave_the_objects_usable(pkg, ora):
    import torch
    b = pkg.binding
    lib = pkg.load_library()
    taps = ora.quantize_taps(_design(pkg, 81, 4, 5))
    nch, n = 2, 6000
    x = np.random.RandomState(3).randint(-20000, 20000, size=(nch, n)).astype(np.int16)
    d = torch.from_numpy(x).cuda()
    # a resampler with the DC blocker refuses the bits form, says why, and goes on with PCM as if nothing had been asked
    rs = pkg.Resampler(nch, taps, 4, 5, 4096, device=0, dc_pole=0.999)
    ref = [ora.Resampler(taps, 4, 5, dc_pole=0.999) for _ in range(nch)]
    first = rs.process_host(x[:, :3000])
    with pytest.raises(pkg.MfmError) as ei:
        rs.process_bits_host(x[:, 3000:], NEG)
    assert ei.value.code == b.MFM_E_INVAL and b"DC blocker" in lib.mfm_last_error()
    with pytest.raises(pkg.MfmError) as ei:
        rs.process_bits_device(d.data_ptr(), n, 100, POS)
    assert ei.value.code == b.MFM_E_INVAL
    second = rs.process_host(x[:, 3000:])
    want = np.stack([np.concatenate([r.feed(x[c, :3000]), r.feed(x[c, 3000:])]) for c, r in enumerate(ref)])
    assert np.array_equal(np.concatenate([first, second], axis=1), want)
    rs.close()
    # unknown polarity; wrong polarity into either stage
    rs = pkg.Resampler(nch, taps, 4, 5, 4096, device=0)
    for pol in (0, 3, 0x80000001):
        with pytest.raises(pkg.MfmError) as ei:
            rs.process_bits_device(d.data_ptr(), n, 100, pol)
        assert ei.value.code == b.MFM_E_INVAL and b"polarity" in lib.mfm_last_error()
    pg, ai = pkg.Pocsag(nch, rs.max_out()), pkg.Ais(nch, rs.max_out())
    want = np.stack([ora.Resampler(taps, 4, 5).feed(x[c]) for c in range(nch)])
    v = rs.process_bits_device(d.data_ptr(), n, 3000, POS)
    with pytest.raises(pkg.MfmError) as ei:
        pg.process_bits_device(v)
    assert ei.value.code == b.MFM_E_INVAL and b"MFM_BITS_NEG" in lib.mfm_last_error()
    ai.process_bits_device(v)
    ai.fetch_events()
    n1 = v.nr_bits
    v = rs.process_bits_device(d.data_ptr() + 2 * 3000, n, 3000, NEG)
    with pytest.raises(pkg.MfmError) as ei:
        ai.process_bits_device(v)
    assert ei.value.code == b.MFM_E_INVAL and b"MFM_BITS_POS" in lib.mfm_last_error()
    pg.process_bits_device(v)
    pg.fetch_events()
    got = _device_rows(v.d_bits, v.stride_words, (v.nr_bits + 31) // 32, nch, np.uint32)
    assert np.array_equal(got, _pack_rows(want[:, n1:n1 + v.nr_bits] < 0))  # the refused calls consumed nothing
    for o in (rs, pg, ai):
        o.close()


# ---- GPU: the stages behind it --------------------------------------------------------------------------------

def _sorted_by_channel(parts):
    ev = np.concatenate(parts)
    return ev[np.argsort(ev["channel"], kind="stable")]


def _chain(pkg, rs, stage, x, pol, cuts, mode):
    """x [C][n] through resampler -> stage on the device, cut into calls at `cuts`; mode 'bits', 'pcm' or 'mixed'
    (alternating at random on the same two objects).  Returns (events per call, outputs after each call)."""
    import torch
    nch, n = x.shape
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rng = np.random.RandomState(len(cuts))
    bounds = [0] + list(cuts) + [n]
    parts, outs, total, used = [], [], 0, set()
    for a, b in zip(bounds, bounds[1:]):
        bits = mode == "bits" or (mode == "mixed" and rng.randint(0, 2) == 1)
        used.add(bits)
        if bits:
            v = rs.process_bits_device(d.data_ptr() + 2 * a, n, b - a, pol)
            stage.process_bits_device(v)
            total += v.nr_bits
        else:
            yptr, ystride, ny = rs.process_device(d.data_ptr() + 2 * a, n, b - a)
            stage.process_device(yptr, ystride, ny)
            total += ny
        parts.append(stage.fetch_events())
        outs.append(total)
    assert mode != "mixed" or used == {True, False}
    return parts, outs


def _random_cuts(rng, n, biggest, count):
    cuts = set(rng.choice(np.arange(1, n), count, replace=False).tolist())
    cuts |= set(range(biggest, n, biggest))  # no call longer than the objects take
    return sorted(cuts)


@pytest.mark.gpu
def test_gpu_pocsag_events_through_the_sign_bits_equal_the_oracle(pkg, ora):
    """48 kS/s PCM -> 4/5 -> bits -> POCSAG stage: events equal, field for field, to oracle resampler -> oracle POCSAG;
    512 / 1200 / 2400 baud, noise-only and silent channels, random cuts, and PCM / bits calls alternating on one stage
    across window slides"""
    from test_pocsag import _compare_events, _messages
    sy = pkg.synth
    msgs = _messages(sy)
    reps = 1
    while sy.pocsag_bits(sy.pocsag_batches(msgs * reps)).size < 576 + 544 * 11:
        reps += 1
    bits = sy.pocsag_bits(sy.pocsag_batches(msgs * reps))
    n = 1300000  # the 512 baud transmission: 93.75 input samples per bit
    rng = np.random.RandomState(21)
    chans = []
    for baud, seed, noise in ((512, 1, 600), (1200, 2, 900), (2400, 3, 1500)):
        parts, size = [], 0
        while size < n:
            parts.append(sy.pocsag_pcm(bits, baud, noise=noise, lead=5000 + 777 * seed, trail=25000, seed=seed + 10 * len(parts), rate=48000))
            size += parts[-1].size
        chans.append(np.concatenate(parts)[:n])
    chans.append(rng.normal(0, 2000, n).round().astype(np.int16))
    chans.append(np.zeros(n, np.int16))
    chans.append(rng.randint(-32768, 32768, n).astype(np.int16))
    x = np.stack(chans)
    nch = x.shape[0]
    rtaps = ora.quantize_taps(sy.design_lpf(81, 0.45 / 5, 1.0) * 4)
    want = []
    for c in range(nch):
        ev, _ = ora.Pocsag().feed(ora.Resampler(rtaps, 4, 5).feed(x[c]))
        want.append(ev)
    for c in range(3):  # the condition on the inputs, on the oracle alone
        assert int((want[c]["type"] == ora.EV_BATCH).sum()) >= 10, c
        assert int((want[c]["type"] == ora.EV_SYNC_LOST).sum()) >= 1, c
    blk = 40000
    for mode, count in (("bits", 0), ("bits", 60), ("mixed", 90)):
        rs = pkg.Resampler(nch, rtaps, 4, 5, blk, device=0)
        pg = pkg.Pocsag(nch, rs.max_out(), device=0)
        # the stage's window holds 65536 + 2048 + 2 * (max_in rounded up to 2048) samples and slides when a call would not
        # fit: with calls of at most max_in that is at least twice in any stretch of three windows
        window = 65536 + 2048 + 2 * ((rs.max_out() + 2047) // 2048 * 2048)
        assert n * 4 // 5 > 3 * window
        parts, _ = _chain(pkg, rs, pg, x, NEG, _random_cuts(rng, n, blk, count) if count else list(range(blk, n, blk)), mode)
        got = _sorted_by_channel(parts)
        for c in range(nch):
            _compare_events(got[got["channel"] == c], want[c], ora, f"{mode}/{count} channel {c}")
        rs.close()
        pg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
def test_gpu_ais_events_through_the_sign_bits_equal_the_restatement(pkg, ora, invert):
    """60 kS/s PCM -> 4/5 -> bits -> AIS stage against oracle resampler -> tests/ais_ref.py: packets of types 1, 4, 5 back
    to back, CRC rejects, a packet that straddles a call boundary, noise and silence; bits only and alternating with PCM"""
    from test_ais import _busy, _payloads, _same
    sy = pkg.synth
    n_out, n_in, blk = 200000, 250000, 30000
    p1, p4, p5 = _payloads(sy)
    back_to_back = sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(p) for p in (p1, p4, p5) * 12]), noise=300, trail=n_out, seed=5)[:n_out]
    rng = np.random.RandomState(31)
    chans = [_busy(sy, 60, n_out), _busy(sy, 61, n_out, noise=1500.0), back_to_back,
             (rng.randn(n_out) * 2000).round().astype(np.int16), np.zeros(n_out, np.int16)]
    x60 = np.stack([np.repeat(c, 5)[::4][:n_in] for c in chans])
    x_in = (-x60.astype(np.int32)).clip(-32768, 32767).astype(np.int16) if invert else x60
    rtaps = ora.quantize_taps(sy.design_lpf(41, 0.45 / 5, 1.0) * 4)
    want = ais_ref.demod_channels(np.stack([ora.Resampler(rtaps, 4, 5, invert=invert).feed(r) for r in x_in]))
    for c in range(3):
        assert int((want["channel"] == c).sum()) >= 20, c
    assert (want["fcs_valid"] == 0).any() and (want["fcs_valid"] == 1).any()
    nch = x_in.shape[0]
    for mode, count in (("bits", 0), ("bits", 80), ("mixed", 120)):
        rs = pkg.Resampler(nch, rtaps, 4, 5, blk, device=0, invert=invert)
        st = pkg.Ais(nch, rs.max_out())
        cuts = _random_cuts(rng, n_in, blk, count) if count else list(range(blk, n_in, blk))
        parts, outs = _chain(pkg, rs, st, x_in, POS, cuts, mode)
        # some packet begins in one call and ends in a later one
        assert any(((want["start_sample"] < o) & (want["sample"] >= o)).any() for o in outs[:-1])
        _same(_sorted_by_channel(parts), want)
        rs.close()
        st.close()


@pytest.mark.gpu
def test_gpu_chain_engine_to_bits_to_pocsag_stays_on_device(pkg, ora):
    """etc/pocsag_rtlsdr.json geometry (fs 1.2 MS/s, D 25 -> 48 kS/s): Engine -> mfm_engine_last_output_device -> resampler
    bits -> POCSAG stage on the engine's stream, against oracle engine -> oracle resampler -> oracle POCSAG"""
    from test_pocsag import _compare_events, _messages
    sy = pkg.synth
    fs, decim, taps, offs, gains = sy.plan("pocsag_rtlsdr")
    assert decim == 25
    bits = sy.pocsag_bits(sy.pocsag_batches(_messages(sy)[:2]))
    n, lead = 3 << 20, 60000
    iq = np.zeros((n, 2), np.int64)
    for o, baud, seed in zip(offs, (1200, 512), (1, 2)):
        b = bits if baud == 1200 else bits[:576 + 544]
        burst = sy.pocsag_fm_iq(b, baud, fs, float(o), lead=lead, trail=0, amplitude=7000.0, noise=150.0, seed=seed)
        m = min(n, burst.shape[0])
        iq[:m] += burst[:m]
        if m < n:
            ph = 2 * np.pi * float(o) * np.arange(m, n) / fs
            iq[m:, 0] += (7000.0 * np.cos(ph)).round().astype(np.int64)
            iq[m:, 1] += (7000.0 * np.sin(ph)).round().astype(np.int64)
    iq = np.clip(iq, -32768, 32767).astype(np.int16)
    blk = 1 << 19
    eng = pkg.Engine(fs, decim, blk, device=0, flags=pkg.binding.MFM_F_DEVICE_ONLY)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g))
    eng.commit()
    rtaps = ora.quantize_taps(sy.design_lpf(81, 0.45 / 5, 1.0) * 4)
    rs = pkg.Resampler(len(offs), rtaps, 4, 5, blk // decim + 8, device=0)
    pg = pkg.Pocsag(len(offs), rs.max_out(), device=0)
    got = []
    for b in range(n // blk):
        assert eng.push(iq[b * blk:(b + 1) * blk]) == 0
        dptr, stride, nout, _ = eng.last_output_device()
        v = rs.process_bits_device(dptr, stride, nout, NEG, stream=eng.stream)
        pg.process_bits_device(v, stream=eng.stream)
        got.append(pg.fetch_events())
    got = _sorted_by_channel(got)
    for o in (eng, rs, pg):
        o.close()
    cre = np.stack([ora.make_taps(taps, int(o), fs, float(g))[0] for o, g in zip(offs, gains)])
    cim = np.stack([ora.make_taps(taps, int(o), fs, float(g))[1] for o, g in zip(offs, gains)])
    incr = np.stack([ora.rot_incr(int(o), fs, decim) for o in offs])
    pcm, _ = ora.run_channels(iq, cre, cim, incr, decim)
    for c in range(len(offs)):
        want, pages = ora.Pocsag().feed(ora.Resampler(rtaps, 4, 5).feed(pcm[c]))
        assert int((want["type"] == ora.EV_BATCH).sum()) >= 1
        _compare_events(got[got["channel"] == c], want, ora, f"chain channel {c}")
        if c == 0:
            assert [m[4].rstrip(b"\x00") for m in pages][:1] == [b"HELLO MI355X\x04"]


# ---- GPU: the decoder programs ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
def test_decoder_amd_sign_bit_option_prints_the_same_lines(tmp_path, ora, pkg, invert):
    """decoder_amd -m POCSAG -s: JSON lines byte-equal to the run without -s and to what the oracle chain's pages print as"""
    from test_pocsag import _json_lines, _messages
    sy = pkg.synth
    msgs = _messages(sy) + [(0x2AAAA, 7, 1, sy.pocsag_alpha_words('quote " slash / back \\ tab\t nl\n bell\x07 end\x17'))]
    bits = sy.pocsag_bits(sy.pocsag_batches(msgs))
    total = 900000
    chans = []
    for baud, seed in ((1200, 1), (2400, 2), (512, 3)):
        x = sy.pocsag_pcm(bits, baud, noise=900, lead=9000 + 111 * seed, trail=40000, seed=seed, rate=48000)
        chans.append(np.concatenate([x, np.random.RandomState(seed).normal(0, 900, total).round().astype(np.int16)])[:total])
    taps = sy.design_lpf(81, 0.45 / 5, 1.0) * 4
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": [float(t) for t in taps]}))
    paths = []
    for c, x in enumerate(chans):
        p = tmp_path / f"ch{c}.pcm"
        p.write_bytes(((-x.astype(np.int32)).astype(np.int16) if invert else x).tobytes())
        paths.append(str(p))
    env = dict(os.environ, MFM_DECODER_FIXED_TIME="1")
    for name, opt in (("bits", ["-s"]), ("pcm", [])):
        r = subprocess.run([os.path.join(HOST_DIR, "decoder_amd"), "-I", "4", "-D", "5", "-S", "48000", "-F", str(tmp_path / "filter.json"),
                            "-f", "929612500", "-m", "POCSAG", "-c", "-o", str(tmp_path / name), "-B", "100000"] + opt +
                           (["-i"] if invert else []) + paths, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
    rtaps = ora.quantize_taps(taps)
    for c, x in enumerate(chans):
        xin = (-x.astype(np.int32)).astype(np.int16) if invert else x
        _, pages = ora.Pocsag().feed(ora.Resampler(rtaps, 4, 5, invert=invert).feed(xin))
        assert len(pages) >= 3
        got = (tmp_path / f"bits.{c}").read_text()
        assert got == _json_lines(pages), f"channel {c}"
        assert got == (tmp_path / f"pcm.{c}").read_text(), f"channel {c}"


@pytest.mark.gpu
def test_aisdecoder_amd_sign_bit_option_prints_the_same_lines(tmp_path, ora, pkg):
    """aisdecoder_amd -s, 1/1 through a three-tap filter and 4/5 from 60 kS/s: lines byte-equal to the run without -s and
    to the restatement's on the oracle resampler's PCM"""
    from test_ais import _busy
    sy = pkg.synth
    n = 150000
    chans = [_busy(sy, 80 + c, n) for c in range(3)]
    env = dict(os.environ, MFM_DECODER_FIXED_TIME="1")
    for tag, interp, decim, coeffs, data in (
            ("unity", 1, 1, [0.25, 0.5, 0.25], chans),
            ("fourfifths", 4, 5, [float(t) for t in sy.design_lpf(41, 0.45 / 5, 1.0) * 4], [np.repeat(c, 5)[::4] for c in chans])):
        (tmp_path / f"{tag}.json").write_text(json.dumps({"lpfCoeffs": coeffs}))
        paths = []
        for c, x in enumerate(data):
            (tmp_path / f"{tag}{c}.pcm").write_bytes(np.ascontiguousarray(x, np.int16).tobytes())
            paths.append(str(tmp_path / f"{tag}{c}.pcm"))
        for name, opt in (("bits", ["-s"]), ("pcm", [])):
            r = subprocess.run([os.path.join(HOST_DIR, "aisdecoder_amd"), "-I", str(interp), "-D", str(decim), "-S", "48000", "-F",
                                str(tmp_path / f"{tag}.json"), "-f", "162000000", "-c", "-o", str(tmp_path / f"{tag}_{name}"),
                                "-B", "10000"] + opt + paths, capture_output=True, text=True, timeout=180, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
        rtaps = ora.quantize_taps(coeffs)
        lines = 0
        for c, x in enumerate(data):
            want, st = ais_ref.json_lines(ais_ref.demod(ora.Resampler(rtaps, interp, decim).feed(np.ascontiguousarray(x, np.int16))))
            lines += st["lines"]
            got = (tmp_path / f"{tag}_bits.{c}").read_text()
            assert got == want, f"{tag} channel {c}"
            assert got == (tmp_path / f"{tag}_pcm.{c}").read_text(), f"{tag} channel {c}"
        assert lines >= 10
