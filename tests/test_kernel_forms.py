"""Which kernel form the channel engine picks at commit, and parity of every form it picks.

The engine's planner (csrc/mfm_plan.hip, plan_channel_kernel) chooses among the v_dot2 kernel, the first-generation matrix
kernel, the second generation's layouts on 64-channel slices, and the long-filter kernel (mfm_kernel_v3l.hip) with one or two
row blocks per wave; PCM stores go through with system scope ("write-through") from 512 channels on unless MFM_F_PCM_WRITE_BACK.  A
PCM block is bit-exact only if the form that ran is, so:
  1. a selection table pins, for each configuration, the form the planner picks - on the host through
     mfm_hosttwin_kernel_form, and as stats() reports it after commit on the GPU (no kernel runs) - with the expected values
     written out from the documented rules: a form that quietly falls back to another fails here;
  2. every form the table selects runs against the oracle, bit-exact, with its form asserted first."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_parity import _ingest_8bit, _mk_engine, _oracle_tables

# the oracle's thread pool: a job on the GPU machines may use 16 CPUs, whatever os.cpu_count() says
THREADS = min(16, os.cpu_count() or 8)

ETC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_etc")
FLAG = {"V1": 0x8, "DOT2": 0x4, "ONE_RB": 0x400, "S128": 0x800, "S64": 0x1000}


def _etc(config, filter_file):
    """(fs, D, taps, offsets, gains) of a reference configuration file and the filter file that goes with it; a channel's
    gain is its "dBGain" key (multifm/receiver.c reads that key only: a misspelt one leaves 0 dB)"""
    with open(os.path.join(ETC, config)) as f:
        cfg = json.load(f)
    with open(os.path.join(ETC, filter_file)) as f:
        taps = np.array(json.load(f)["lpfTaps"], np.float64)
    offs = np.array([c["chanCenterFreq"] - cfg["centerFreqHz"] for c in cfg["channels"]], np.int64)
    gains = np.array([10.0 ** (c.get("dBGain", 0.0) / 10.0) for c in cfg["channels"]])
    return cfg["sampleRateHz"], cfg["decimationFactor"], taps, offs, gains


def _lpf(decim, ntaps, nch, scale=1.0, fs=2400000, cutoff=9000.0):
    def make(pkg):
        return fs, decim, pkg.synth.design_lpf(ntaps, cutoff, fs) * scale, pkg.synth.channel_offsets(nch, fs), None
    return make


def _plan(name, nch):
    return lambda pkg: pkg.synth.plan(name, nr_channels=nch)


def _planes(n_hi, nch=512):
    """the cfg3 geometry (2.4 MS/s, D = 96, 128 taps: four k-steps of 32 taps) with taps scaled so that n_hi k-steps have a
    tap beyond one signed byte: /8 none; as designed the two middle ones; x4 all four; x4 with the first k-step's taps /8
    three"""
    def make(pkg):
        fs, decim, taps, offs, gains = pkg.synth.plan("cfg3_1024ch", nr_channels=nch)
        t = {0: taps / 8.0, 2: taps, 4: taps * 4.0}.get(n_hi)
        if n_hi == 3:
            t = taps * 4.0
            t[:32] = taps[:32] / 8.0
        return fs, decim, t, offs, None
    return make


def _big_taps(pkg):
    fs = 2400000
    return fs, 96, pkg.synth.design_lpf(128, 400000.0, fs), [0, 37500], [6.275, 1.0]   # peak tap 32705 > 32639


# Selection table: (id, geometry, flags, expected stats).  Expected: kernel_variant (0 v_dot2, 1 first generation, 2 second),
# slice_channels, taps_resident, outputs_per_tile, k_steps, popcount(tap_hi_mask) (None: not pinned).  The rules they follow
# (mfm_plan.hip plan_channel_kernel, the mfm_stats comments in include/multifm_hip.h, mfm3l_fits / mfm3l_instance_ptr in
# mfm_kernel_v3l.hip), in the order the planner applies them (each may replace what the ones before it chose):
#   [dot2]  the v_dot2 kernel: MFM_F_FORCE_DOT2, a tap beyond 32639, or a padded filter beyond 16 k-steps; 128 outputs per
#           tile (two per lane) where the tile fits 53 KiB of LDS
#   [v1]    the first generation: 62-output tiles (two 31-output iterations) where they fit, else 31
#   [sub]   D % 32 == 0, <= 4 k-steps: second generation, sub-plane layout, slices of 64, taps not "resident" (layout 3 only)
#   [crow]  D % 8 == 0, D % 32 != 0, <= 4 k-steps: the chunk-row layout, slices of 64
#   [pad25] D = 25, <= 150 taps: padded-row layout 2, six k-steps, slices of 64
#   [shift] D = 1, 2, 4: the long-filter kernel's shifted copies, one row block per wave (slices of 64), taps resident
#   [v3l]   8..16 k-steps (first generation's power of two): the long-filter kernel, candidates (rb, ng) = (2, 1), (1, 4),
#           (1, 2) in order; rb = 2 needs more than 8 row blocks (> 64 channels) and 8 (kq + nh) <= 128 and is built with
#           quarter-tile images (ng = 1) only; split-row instances (D % 4 != 0) are built with rb = 1, ng = 4, <= 4 chunks only
#   [s128]  the [sub] geometry with 4 k-steps at >= 512 channels (kSlice128MinChannels) or MFM_F_SLICE_128, not with
#           MFM_F_SLICE_64 / MFM_F_FORCE_MFMA_V1: the long-filter kernel with rb = 2, ng = 4 (whole-tile images, built for
#           KQ = 4 with 0, 2 and 4 held high planes: 8 (4 + nh) + 16 <= 128 holds for all) - unless <= 64 channels (one row block)
SELECTION = [
    # ---- every channel-engine configuration under tests/golden/reference_etc/ (multifm_decimate.json configures the
    #      rational resampler only), with its own filter file and channel list
    ("etc_multifm", lambda p: _etc("multifm.json", "flex_25khz_lpf.json"), 0, (2, 64, 0, 64, 4, 2)),        # [crow] D 40
    ("etc_multifm_1ch", lambda p: _etc("multifm_1ch.json", "flex_25khz_lpf.json"), 0, (2, 64, 0, 64, 4, 2)),  # [crow]
    ("etc_multifm_airspy", lambda p: _etc("multifm_airspy.json", "flex_25khz_lpf_3mhz.json"), 0,
     (2, 64, 1, 64, 16, 0)),   # [v3l] D 120, 512 taps: one channel = one row block, (1, 4)
    ("etc_multifm_usrp", lambda p: _etc("multifm_usrp.json", "flex_25khz_lpf_3mhz.json"), 0, (2, 64, 1, 64, 16, 0)),  # [v3l]
    ("etc_multifm_file", lambda p: _etc("multifm_file.json", "flex_25khz_lpf.json"), 0, (2, 64, 1, 64, 4, None)),  # [shift] D 1
    ("etc_pocsag_rtlsdr", lambda p: _etc("pocsag_rtlsdr.json", "pocsag_1200khz_fs.json"), 0,
     (2, 64, 1, 64, 16, None)),   # [v3l] D 25, 256 taps: 11 k-steps used, split rows -> (1, 4)
    ("etc_pocsag_airspy", lambda p: _etc("pocsag_airspy.json", "pocsag_narrow.json"), 0, (2, 64, 1, 64, 16, None)),  # [v3l]
    # ---- bench shapes
    ("cfg2_64", _plan("cfg2_64ch", 64), 0, (2, 64, 0, 64, 4, 2)),            # [sub] D 96
    ("cfg3_511", _plan("cfg3_1024ch", 511), 0, (2, 64, 0, 64, 4, 2)),        # [sub] below kSlice128MinChannels
    ("cfg3_512", _plan("cfg3_1024ch", 512), 0, (2, 128, 1, 64, 4, 2)),       # [s128] at kSlice128MinChannels
    ("cfg3_513", _plan("cfg3_1024ch", 513), 0, (2, 128, 1, 64, 4, 2)),       # [s128] partial last slice (1 channel)
    ("cfg3_1000", _plan("cfg3_1024ch", 1000), 0, (2, 128, 1, 64, 4, 2)),     # [s128] partial last slice (104 channels)
    ("cfg3_1024", _plan("cfg3_1024ch", 1024), 0, (2, 128, 1, 64, 4, 2)),     # [s128] north-star shape
    ("cfg5_64", _plan("cfg5_airspy", 64), 0, (2, 64, 1, 64, 16, 0)),         # [v3l] 8 row blocks: no rb = 2; D 400 needs
                                                                             # half-tile images, (1, 2)
    ("cfg5_130", _plan("cfg5_airspy", 130), 0, (2, 128, 1, 64, 16, 0)),      # [v3l] (2, 1)
    ("cfg5_256", _plan("cfg5_airspy", 256), 0, (2, 128, 1, 64, 16, 0)),      # [v3l] (2, 1)
    ("cfg5_2048", _plan("cfg5_airspy", 2048), 0, (2, 128, 1, 64, 16, 0)),    # [v3l] (2, 1)
    # ---- cfg3's 128-tap filters with the slice flags
    ("s128_65", _plan("cfg3_1024ch", 65), FLAG["S128"], (2, 128, 1, 64, 4, 2)),     # [s128] forced, 9 row blocks
    ("s128_128", _plan("cfg3_1024ch", 128), FLAG["S128"], (2, 128, 1, 64, 4, 2)),   # [s128] forced
    ("s128_129", _plan("cfg3_1024ch", 129), FLAG["S128"], (2, 128, 1, 64, 4, 2)),   # [s128] forced
    ("s128_200", _plan("cfg3_1024ch", 200), FLAG["S128"], (2, 128, 1, 64, 4, 2)),   # [s128] forced
    ("s128_64", _plan("cfg3_1024ch", 64), FLAG["S128"], (2, 64, 0, 64, 4, 2)),      # [s128] <= 64 channels: stays [sub]
    ("s128_8", _plan("cfg3_1024ch", 8), FLAG["S128"], (2, 64, 0, 64, 4, 2)),        # [s128] one row block: stays [sub]
    ("s64_1024", _plan("cfg3_1024ch", 1024), FLAG["S64"], (2, 64, 0, 64, 4, 2)),    # [s128] MFM_F_SLICE_64: [sub]
    ("s64_s128_1024", _plan("cfg3_1024ch", 1024), FLAG["S64"] | FLAG["S128"], (2, 64, 0, 64, 4, 2)),  # SLICE_64 wins
    ("v1_1024", _plan("cfg3_1024ch", 1024), FLAG["V1"], (1, 64, 0, 62, 4, 2)),      # [v1] 128 taps: nothing to hold resident
    ("one_rb_1024", _plan("cfg3_1024ch", 1024), FLAG["ONE_RB"], (2, 64, 0, 64, 4, 2)),  # [s128] asks for rb = 2, which
                                                                                      # MFM_F_V3L_ONE_ROW_BLOCK rules out: [sub]
    # ---- the other [s128] geometries: D % 32 == 0, four k-steps (129 .. 256 padded elements)
    ("d32_t128_512", _lpf(32, 128, 512), 0, (2, 128, 1, 64, 4, 2)),
    ("d32_t100_1024", _lpf(32, 100, 1024), 0, (2, 128, 1, 64, 4, 3)),
    ("d64_t128_512", _lpf(64, 128, 512), 0, (2, 128, 1, 64, 4, 2)),
    ("d64_t72_1024", _lpf(64, 72, 1024), 0, (2, 128, 1, 64, 4, 2)),
    ("d128_t128_1024", _lpf(128, 128, 1024), 0, (2, 128, 1, 64, 4, 2)),
    ("d128_t128_512", _lpf(128, 128, 512), 0, (2, 128, 1, 64, 4, 2)),
    ("d96_t110_512", _lpf(96, 110, 512), 0, (2, 128, 1, 64, 4, 3)),
    ("d32_t64_1024", _lpf(32, 64, 1024), 0, (2, 64, 0, 64, 2, 2)),     # two k-steps: not [s128], stays [sub]
    ("d25_t128_1024", _lpf(25, 128, 1024), 0, (2, 64, 0, 64, 6, None)),  # [pad25]: D % 32 != 0, slices of 64 at any count
    # ---- high-byte tap planes on the [s128] geometry (512 channels): 0, 2, 3 and 4 planes, all on rb = 2 (built for
    #      held-plane counts 0, 2 and 4; the sub-plane fallback for "more than two planes" of the engine comment does not arise)
    ("planes0", _planes(0), 0, (2, 128, 1, 64, 4, 0)),
    ("planes2", _planes(2), 0, (2, 128, 1, 64, 4, 2)),
    ("planes3", _planes(3), 0, (2, 128, 1, 64, 4, 3)),
    ("planes4", _planes(4), 0, (2, 128, 1, 64, 4, 4)),
    # ---- fallbacks: what runs now where the preferred form is not built
    ("d25_t170_130", _lpf(25, 170, 130), 0, (2, 64, 1, 64, 8, 3)),   # [v3l] D % 4 != 0: split rows, rb = 1 only
    ("d30_t150_130", _lpf(30, 150, 130), 0, (2, 64, 1, 64, 8, 3)),   # [v3l] D % 4 != 0: split rows, rb = 1 only
    ("d24_t140_130", _lpf(24, 140, 130), 0, (2, 128, 1, 64, 8, 3)),  # [v3l] D % 4 == 0: (2, 1) is built and fits
    ("d150_t300_130", _lpf(150, 300, 130), 0, (1, 64, 1, 31, 16, 2)),  # [v3l] D % 4 != 0 needs a half-tile image (> 4 chunks
                                                                      # for a whole tile): no split instance -> [v1]; resident:
                                                                      # recorded (first-generation instance table)
    ("d96_t256_130", _lpf(96, 256, 130), 0, (2, 128, 1, 64, 8, 2)),              # [v3l] (2, 1)
    ("d96_t256_130_one_rb", _lpf(96, 256, 130), FLAG["ONE_RB"], (2, 64, 1, 64, 8, 2)),  # [v3l] rb = 1 forced: (1, 4)
    ("force_dot2", _plan("cfg3_1024ch", 1024), FLAG["DOT2"], (0, 0, 0, 128, 0, 0)),  # [dot2]
    ("taps_beyond_byte_split", _big_taps, 0, (0, 0, 0, 128, 0, 0)),                 # [dot2]
]


FORM_FIELDS = ("kernel_variant", "slice_channels", "taps_resident", "outputs_per_tile", "k_steps", "tap_hi_mask", "lds_bytes",
               "rot_exact_channels", "rot_fast_slices")


def _selection_engine(pkg, row):
    """the row's engine with its channels added, not committed"""
    name, geom, flags, want = row
    fs, decim, taps, offs, gains = geom(pkg)
    eng = pkg.Engine(fs, decim, 1 << 16, device=0, flags=flags)
    gains = gains if gains is not None else [1.0] * len(offs)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g))
    return eng


def _check_form(row, st):
    name, _, _, want = row
    got = (st["kernel_variant"], st["slice_channels"], st["taps_resident"], st["outputs_per_tile"], st["k_steps"],
           bin(st["tap_hi_mask"]).count("1"))
    want = tuple(g if w is None else w for w, g in zip(want, got))
    assert got == want, f"{name}: (variant, slice, resident, outputs/tile, k-steps, high planes) {got}, expected {want}"


@pytest.mark.parametrize("row", SELECTION, ids=[r[0] for r in SELECTION])
def test_selection_table_host(pkg, row):
    """the planner on the host, without a device (mfm_hosttwin_kernel_form)"""
    eng = _selection_engine(pkg, row)
    st = eng.kernel_form()
    eng.close()
    _check_form(row, st)


@pytest.mark.gpu
@pytest.mark.parametrize("row", SELECTION, ids=[r[0] for r in SELECTION])
def test_selection_table(pkg, row):
    """what commit chose, as stats() reports it - and that it is what the host twin planned"""
    eng = _selection_engine(pkg, row)
    twin = eng.kernel_form()
    eng.commit()
    st = eng.stats()
    eng.close()
    _check_form(row, st)
    assert {k: st[k] for k in FORM_FIELDS} == {k: twin[k] for k in FORM_FIELDS}, row[0]


# ---------------------------------------------------------------------------------------------------------------- parity

# ragged blocks: single samples, one block shorter than the 128-tap filter, odd lengths, front-end buffer sizes
SIZES = [50000, 1, 100, 4096, 7919, 1, 127, 30001, 96 * 64 + 5, 12345]


def _form(eng, variant, slices):
    st = eng.stats()
    assert (st["kernel_variant"], st["slice_channels"]) == (variant, slices), st
    return st


def _stream(pkg, eng, iq, sizes=SIZES):
    """push iq in blocks of the given (cycled) sizes, fetch everything; (PCM, filtered IQ or None)"""
    pcm, q, pos, k = [], [], 0, 0
    n = iq.shape[0]
    while pos < n:
        m = min(sizes[k % len(sizes)], n - pos)
        rc = eng.push(iq[pos:pos + m])
        if rc == pkg.binding.MFM_E_BUSY:
            got = eng.fetch()
            pcm.append(got[1])
            q.append(got[2])
            continue
        assert rc == 0, eng.lib.mfm_last_error()
        pos += m
        k += 1
    eng.sync()
    while True:
        got = eng.fetch()
        if got is None:
            break
        pcm.append(got[1])
        q.append(got[2])
    return np.concatenate(pcm, axis=1), (np.concatenate(q, axis=1) if q and q[0] is not None else None)


def _assert_equal(pcm, ref, what):
    assert pcm.shape == ref.shape, (what, pcm.shape, ref.shape)
    if not np.array_equal(pcm, ref):
        bad = np.argwhere(pcm != ref)
        raise AssertionError(f"{what}: {len(bad)} PCM samples differ from the oracle; first at (chan, n) = {bad[0]}, "
                             f"channels {np.unique(bad[:, 0])[:8]}")


def _mixed_offsets(pkg, nch, fs=2400000, decim=96):
    """channel_offsets with two channels in five on the 12.5 kHz grid (exact rotators): the engine orders rows by rotator
    class, so the class boundary falls inside a 128-channel slice"""
    offs = pkg.synth.channel_offsets(nch, fs).astype(np.int64)
    grid = pkg.synth.grid_offsets(nch, fs, decim)
    sel = np.arange(nch) % 5 < 2
    offs[sel] = grid[sel]
    return offs


def _run_parity(pkg, ora, fs, decim, taps, offs, iq, flags, variant, slices, gains=None, sizes=SIZES):
    eng = _mk_engine(pkg, fs, decim, taps, offs, gains, max_block=max(sizes), flags=flags)
    st = _form(eng, variant, slices)
    cre, cim, incr = _oracle_tables(eng, len(offs))
    pcm, _ = _stream(pkg, eng, iq, sizes)
    eng.close()
    ref, _ = ora.run_channels(iq, cre, cim, incr, decim, threads=THREADS)
    _assert_equal(pcm, ref, f"flags {flags:#x}, {len(offs)} channels")
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [512, 513, 1000, 1024])
def test_slice128_by_default(pkg, ora, nch):
    """From kSlice128MinChannels on, 128-tap filters run on 128-channel slices; partial last slices (513: one channel, 1000:
    104) and a rotator-class boundary inside a slice, int16 blocks of ragged lengths."""
    fs, decim, taps, _, gains = pkg.synth.plan("cfg3_1024ch", nr_channels=nch)
    offs = _mixed_offsets(pkg, nch)
    iq = pkg.synth.synth_iq(sum(SIZES), fs, offs[::max(1, nch // 5)][:5], seed=nch)
    st = _run_parity(pkg, ora, fs, decim, taps, offs, iq, 0, 2, 128)
    assert 0 < st["rot_exact_channels"] < nch


@pytest.mark.gpu
@pytest.mark.parametrize("nch,iq_chan", [(129, None), (200, 77), (384, None)])
def test_slice128_forced(pkg, ora, nch, iq_chan):
    """MFM_F_SLICE_128 below 512 channels; with a filtered-IQ consumer on one channel the rb = 2 instance keeps running (its
    epilogue's IQ store is a run-time switch) and that channel's filtered IQ is the oracle's as well."""
    b = pkg.binding
    fs, decim, taps, _, gains = pkg.synth.plan("cfg3_1024ch", nr_channels=nch)
    offs = _mixed_offsets(pkg, nch)
    iq = pkg.synth.synth_iq(sum(SIZES), fs, offs[::max(1, nch // 5)][:5], seed=nch + 1)
    eng = pkg.Engine(fs, decim, max(SIZES), device=0, flags=b.MFM_F_SLICE_128)
    for c, o in enumerate(offs):
        eng.add_channel(int(o), taps, 1.0, want_iq=(c == iq_chan))
    eng.commit()
    _form(eng, 2, 128)
    cre, cim, incr = _oracle_tables(eng, nch)
    pcm, q = _stream(pkg, eng, iq)
    eng.close()
    ref, refq = ora.run_channels(iq, cre, cim, incr, decim, threads=THREADS, want_iq=iq_chan is not None)
    _assert_equal(pcm, ref, f"SLICE_128, {nch} channels")
    if iq_chan is not None:
        assert q is not None and np.array_equal(q[iq_chan], refq[iq_chan]), "filtered IQ differs"


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [512, 1024])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_slice128_on_bytes(pkg, ora, fmt, nch):
    """The north-star shape as an RTL-SDR deployment runs it: 8-bit blocks read as bytes by the rb = 2 instance, full-range
    bytes (0x00, 0x7f, 0x80, 0xff), ragged (even: cu8) block lengths, one shorter than the filter."""
    fs, decim, taps, offs, _ = pkg.synth.plan("cfg3_1024ch", nr_channels=nch)
    rng = np.random.RandomState(300 + fmt + nch)
    blocks = []
    for m in (40000, 96, 4096, 30002, 2, 12346):
        raw = rng.randint(0, 256, size=(m, 2)).astype(np.uint8)
        raw[:4] = [[0, 255], [127, 128], [128, 127], [255, 0]][:min(4, m)]
        blocks.append((raw, fmt))
    got, want, st = _ingest_8bit(pkg, ora, fs, decim, taps, offs, blocks, 40000)
    assert (st["kernel_variant"], st["slice_channels"]) == (2, 128), st
    assert st["launches_8bit"] == st["launches"] > 0, st
    _assert_equal(got, want, f"bytes fmt {fmt}, {nch} channels")


@pytest.mark.gpu
@pytest.mark.parametrize("n_hi", [0, 2, 3, 4])
def test_slice128_high_byte_planes(pkg, ora, n_hi):
    """Tap sets with 0, 2, 3 and 4 high-byte k-steps on 128-channel slices (instances for 0, 2 and 4 held planes)."""
    fs, decim, taps, offs, _ = _planes(n_hi)(pkg)
    iq = pkg.synth.random_iq(sum(SIZES), seed=n_hi)
    eng = _mk_engine(pkg, fs, decim, taps, offs, max_block=max(SIZES))
    st = _form(eng, 2, 128)
    eng.close()
    assert bin(st["tap_hi_mask"]).count("1") == n_hi, hex(st["tap_hi_mask"])
    _run_parity(pkg, ora, fs, decim, taps, offs, iq, 0, 2, 128)


def _device_only(pkg, eng, iq, block):
    """MFM_F_DEVICE_ONLY: push, sync, copy the device view of each block's PCM out"""
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    outs = []
    for lo in range(0, iq.shape[0], block):
        assert eng.push(iq[lo:lo + block]) == 0, eng.lib.mfm_last_error()
        eng.sync()
        dptr, stride, nout, _ = eng.last_output_device()
        host = np.empty((eng.nr_channels, stride), np.int16)
        assert rt.hipMemcpy(host.ctypes.data, dptr, host.nbytes, 2) == 0
        outs.append(host[:, :nout].copy())
    return np.concatenate(outs, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["cfg3", "cfg5"])
def test_pcm_store_policy(pkg, ora, geom):
    """At 512 channels (kPcmWriteThroughMinChannels) PCM stores go through with system scope unless MFM_F_PCM_WRITE_BACK:
    {slices of 64, slices of 128} x {write-through, write-back} on the 128-tap geometry, write-back against the default on
    the long-filter kernel (cfg5, D 400, 512 taps) - consumed through the host mirror and, device-only, from the device view
    (write-back PCM must be visible to the next consumer without a system-scope store)."""
    b = pkg.binding
    name = {"cfg3": "cfg3_1024ch", "cfg5": "cfg5_airspy"}[geom]
    fs, decim, taps, offs, gains = pkg.synth.plan(name, nr_channels=512)
    block = 96 * 333 + 17 if geom == "cfg3" else 400 * 120 + 7
    iq = pkg.synth.random_iq(3 * block + len(taps), seed=512)
    slicings = [(b.MFM_F_SLICE_64, 64), (0, 128)] if geom == "cfg3" else [(0, 128)]
    ref = None
    for slice_flag, slices in slicings:
        for store in (0, b.MFM_F_PCM_WRITE_BACK):
            flags = slice_flag | store
            eng = _mk_engine(pkg, fs, decim, taps, offs, gains, max_block=block, flags=flags)
            _form(eng, 2, slices)
            if ref is None:
                cre, cim, incr = _oracle_tables(eng, len(offs))
                ref, _ = ora.run_channels(iq, cre, cim, incr, decim, threads=THREADS)
            pcm, _ = eng.run(iq, block)
            eng.close()
            _assert_equal(pcm, ref, f"{geom} host mirror, flags {flags:#x}")
            eng = _mk_engine(pkg, fs, decim, taps, offs, gains, max_block=block, flags=flags | b.MFM_F_DEVICE_ONLY)
            _form(eng, 2, slices)
            pcm = _device_only(pkg, eng, iq, block)
            eng.close()
            _assert_equal(pcm, ref, f"{geom} device view, flags {flags:#x}")

@pytest.mark.gpu

def test_slice128_gathered_and_overlapped(pkg, ora):
    """MFM_F_GATHER | MFM_F_OVERLAP with coalesce_samples on 128-channel slices: launch boundaries at the gathered counts, each
    launch recomputing the output in front of it.  The launches stay on ONE stream (at most 38 tiles on 4 slices, against the
    256 slots of one workgroup per CU: overlapped_launches == 0 below) - this is the flag's bookkeeping on the long-filter
    kernel; launches of that kernel that do alternate are in tests/test_overlap_forms.py."""
    b = pkg.binding
    fs, decim, taps, _, _ = pkg.synth.plan("cfg3_1024ch", nr_channels=512)
    offs = _mixed_offsets(pkg, 512)
    sizes = [1, 100, 4096, 4096, 16384, 7919, 5, 127, 128, 129, 60000, 1000, 131072]
    n = 400000
    iq = pkg.synth.synth_iq(n, fs, offs[::100], seed=5120)
    eng = pkg.Engine(fs, decim, 131072, device=0, flags=b.MFM_F_GATHER | b.MFM_F_OVERLAP, coalesce_samples=100000)
    for o in offs:
        eng.add_channel(int(o), taps, 1.0)
    eng.commit()
    _form(eng, 2, 128)
    cre, cim, incr = _oracle_tables(eng, len(offs))
    parts, pos, k = [], 0, 0

    def drain():
        while True:
            got = eng.fetch()
            if got is None:
                return
            assert not parts or got[0] == parts[-1][0] + parts[-1][1].shape[1]
            parts.append((got[0], got[1]))
    while pos < n:
        m = min(sizes[k % len(sizes)], n - pos)
        rc = eng.push(iq[pos:pos + m])
        if rc == b.MFM_E_BUSY:
            drain()
            continue
        assert rc == 0, eng.lib.mfm_last_error()
        pos += m
        k += 1
    while eng.flush() == b.MFM_E_BUSY:
        drain()
    eng.sync()
    drain()
    st = eng.stats()
    eng.close()
    pcm = np.concatenate([p[1] for p in parts], axis=1)
    ref, _ = ora.run_channels(iq, cre, cim, incr, decim, threads=THREADS)
    _assert_equal(pcm, ref, "gathered + overlapped, 512 channels")
    assert st["submits"] == k and st["pending_samples"] == 0 and 2 <= st["launches"] <= n // 100000 + 1, st
    assert st["overlapped_launches"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["d25_t170_130", "d30_t150_130", "d24_t140_130", "d150_t300_130", "d96_t256_130_one_rb"])
def test_fallback_geometries(pkg, ora, row):
    """Parity of the fallback rows of the selection table, in the form the table pins."""
    name, geom, flags, want = next(r for r in SELECTION if r[0] == row)
    fs, decim, taps, offs, gains = geom(pkg)
    sizes = [decim * 400 + 3, 1, len(taps) - 7, 20011, decim * 64 + 9]
    iq = pkg.synth.synth_iq(sum(sizes) * 2, fs, offs[::40][:4], seed=decim)
    _run_parity(pkg, ora, fs, decim, taps, offs, iq, flags, want[0], want[1], sizes=sizes)
