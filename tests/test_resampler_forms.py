"""Which kernel the PCM resampler picks at create, and parity of every instance it picks.

mfm_resampler_create (csrc/mfm_resampler.hip, planned by rs_plan in csrc/mfm_rs_plan.h) chooses between the matrix-core kernel
with KS = 1 .. 4 k-steps and the v_dot2 kernel with a phase's coefficient pairs in registers (NP = 4, 8, ..., 32) or in LDS
(NP = 0), in two LDS regimes (up to 48 KB, and above it with the kernel's limit raised), with four fallbacks from the matrix
form and refusals.  All the decoders consume its PCM, so a wrong sample here is one they would all agree on.  So:
  (a) a selection table pins, for each configuration, the form the planner picks - on the host through
      mfm_hosttwin_resampler_form and, on the GPU, as get_form reports it after create (no kernel runs);
  (b) the tables of the matrix form (A fragments in lane order, row constants, the padded-row layout) are evaluated on the CPU
      for every carried phase (mfm_hosttwin_resampler_matrix_block) against the oracle;
  (c) every row of the table, and every NP instance forced, runs against the oracle with its form asserted first;
  (d) the DC blocker alone (the resampler as an identity), at poles that make its multiplier's operands wide, on two lane blocks;
  (e) input rows that start at odd samples of a larger buffer, strides far beyond the row, and the max_in_samples bound.
Every comparison is bit-exact.

The rules the table's expected values are written out from (head of mfm_resampler.hip; filter/polyphase_fir.c:70-83 for the
phase length), in the order the planner applies them:
  [plen]   phase length = ceil(T / I), rounded up to a multiple of 4
  [walk]   refused: ceil(D / I) > plen (an output would consume more samples than a phase holds)
  [lds]    v_dot2 LDS = 2 I plen + 2 (floor(1024 D / I) + plen + 32) bytes, rounded up to 16; refused above 150 KB
  [np]     coefficient pairs in registers when 256 D % I == 0, plen / 2 <= 32 and that LDS is at most 48 KB: the instance is
           NP = plen / 2 rounded up to 4; else NP = 0 (pairs in LDS) - above 48 KB always, with the kernel's limit raised
  [matrix] not forced (MFM_RS_FORCE_DOT2), 16 D / I an integer R ("ratio"), R <= 240 ("block"), K <= 256 ("window") where
           K = (last / R) rp + last % R + 1 rounded up to 64, rp = R rounded up to 16, last = floor((I - 1 + 15 D) / I) + plen - 1,
           and every tap within +-32639 ("tap range"); KS = K / 64; LDS = 2 planes of (256 + ceil(K / rp)) rp bytes, each
           rounded up to 64
"""
import ctypes as C

import numpy as np
import pytest

DOT2, MATRIX = 0, 1
FB = {"none": 0, "ratio": 1, "window": 2, "block": 3, "tap range": 4, "forced": 5}


def _taps(ntaps, kind, seed):
    """random taps within +-32639 (the int32 sums wrap), with the peak the row asks for"""
    rng = np.random.RandomState(seed)
    t = rng.randint(-32639, 32640, size=ntaps).astype(np.int16)
    if kind == "beyond":
        t[ntaps // 3] = 32640
    elif kind == "peak":
        t[ntaps // 3] = 32639
        t[ntaps // 2] = -32639
    return t


# (id, I, D, taps, tap kind, natural form: (form, KS, fallback, LDS bytes or None), NP when forced to v_dot2, phase length)
# or (..., None, None, None) for a refusal.  Worked out by hand from the rules above, e.g. 4/5 with 81 taps: plen = ceil(81 / 4)
# = 21 -> 24; R = 20, rp = 32, last = floor((3 + 75) / 4) + 23 = 42, K = 2 * 32 + 2 + 1 = 67 -> 128, KS = 2; 12 pairs -> NP 12.
SELECTION = [
    ("4_5_t8", 4, 5, 8, "random", (MATRIX, 1, "none", None), 4, 4),
    ("4_5_t40", 4, 5, 40, "random", (MATRIX, 1, "none", None), 8, 12),
    ("4_5_t81", 4, 5, 81, "random", (MATRIX, 2, "none", None), 12, 24),
    ("4_5_t100", 4, 5, 100, "random", (MATRIX, 2, "none", None), 16, 28),
    ("4_5_t160", 4, 5, 160, "random", (MATRIX, 2, "none", None), 20, 40),
    ("2_3_t96", 2, 3, 96, "random", (MATRIX, 2, "none", None), 24, 48),
    ("16_25_t821", 16, 25, 821, "random", (MATRIX, 2, "none", None), 28, 52),
    ("4_5_t256", 4, 5, 256, "random", (MATRIX, 3, "none", None), 32, 64),
    ("4_5_t260", 4, 5, 260, "random", (MATRIX, 3, "none", None), 0, 68),           # 34 pairs: more than the registers hold
    ("1_2_t200", 1, 2, 200, "random", (MATRIX, 4, "none", None), 0, 200),
    ("1_1_t240", 1, 1, 240, "random", (MATRIX, 4, "none", None), 0, 240),
    ("1_8_t136", 1, 8, 136, "random", (MATRIX, 4, "none", 66048), 0, 136),         # matrix LDS beyond 64 KB
    ("1_10_t60", 1, 10, 60, "random", (MATRIX, 4, "none", 82560), 32, 60),
    ("1_15_t16", 1, 15, 16, "random", (MATRIX, 4, "none", 123904), 8, 16),
    ("1_1_t242", 1, 1, 242, "random", (DOT2, 0, "window", None), 0, 244),          # last = 15 + 243: K = 259 -> 320
    ("1_2_t250", 1, 2, 250, "random", (DOT2, 0, "window", None), 0, 252),
    ("1_8_t140", 1, 8, 140, "random", (DOT2, 0, "window", None), 0, 140),
    ("1_16_t16", 1, 16, 16, "random", (DOT2, 0, "block", None), 8, 16),            # R = 256
    ("2_31_t40", 2, 31, 40, "random", (DOT2, 0, "block", None), 12, 20),           # R = 248 (its window is too long as well)
    ("3_2_t41", 3, 2, 41, "random", (DOT2, 0, "ratio", None), 0, 16),
    ("7_3_t50", 7, 3, 50, "random", (DOT2, 0, "ratio", None), 0, 8),
    ("3_7_t60", 3, 7, 60, "random", (DOT2, 0, "ratio", None), 0, 20),
    ("25_40_t821", 25, 40, 821, "random", (DOT2, 0, "ratio", None), 0, 36),        # multifm_decimate.json, unreduced
    ("1_30_t64", 1, 30, 64, "random", (DOT2, 0, "block", 61760), 0, 64),           # v_dot2 LDS above 48 KB (R = 480)
    ("1_73_t80", 1, 73, 80, "random", (DOT2, 0, "block", 149888), 0, 80),          # just under the 150 KB refusal
    ("1_100_t128", 1, 100, 128, "random", None, None, None),                      # refused [lds]: 205 376 bytes
    ("1_9_t5", 1, 9, 5, "random", None, None, None),                              # refused [walk]: plen 8 < 9
    ("4_5_t81_beyond", 4, 5, 81, "beyond", (DOT2, 0, "tap range", None), 12, 24),  # one tap 32640
    ("4_5_t81_peak", 4, 5, 81, "peak", (MATRIX, 2, "none", None), 12, 24),         # peak taps exactly +-32639
]
IDS = [r[0] for r in SELECTION]
ROW = {r[0]: r for r in SELECTION}
RUNNABLE = [r[0] for r in SELECTION if r[5] is not None]
# one row per v_dot2 instance when forced: NP = 4, 8, ..., 32 and 0
FORCED = ["4_5_t8", "4_5_t40", "4_5_t81", "4_5_t100", "4_5_t160", "2_3_t96", "16_25_t821", "4_5_t256", "4_5_t260"]
# one row per matrix instance KS = 1 .. 4 (natural form): with FORCED, the 14 instances that also give sign bits
MATRIX_KS = {"4_5_t40": 1, "4_5_t81": 2, "4_5_t256": 3, "1_2_t200": 4}


def _row_taps(row):
    return _taps(row[3], row[4], seed=1000 * row[1] + 10 * row[2] + row[3])


def _expect(row, forced):
    """the form dict entries the row pins"""
    _, interp, decim, ntaps, _, natural, forced_np, plen = row
    form, ks, fb, lds = natural
    if forced:
        form, ks, fb, lds = DOT2, 0, "forced", None
    want = {"form": form, "k_steps": ks, "fallback": FB[fb], "phase_len": plen}
    if form == DOT2:
        want.update(reg_pairs=forced_np, block_samples=0, row_bytes=0, window_bytes=0)
    else:
        r = 16 * decim // interp
        want.update(reg_pairs=0, block_samples=r, row_bytes=(r + 15) // 16 * 16, window_bytes=64 * ks)
    if lds is not None:
        want["lds_bytes"] = lds
    return want


def _check_form(name, got, want):
    sub = {k: got[k] for k in want}
    assert sub == want, f"{name}: form {sub}, expected {want}"


def test_selection_table_covers_every_instance():
    """the table is only worth its rows: all four KS, all nine NP, every fallback, both refusals, both LDS regimes of each form"""
    rows = [r for r in SELECTION if r[5] is not None]
    assert {r[5][1] for r in rows if r[5][0] == MATRIX} == {1, 2, 3, 4}
    assert {ROW[n][6] for n in FORCED} == {0, 4, 8, 12, 16, 20, 24, 28, 32}
    assert {r[5][2] for r in rows} == {"none", "ratio", "window", "block", "tap range"}
    assert sum(r[5] is None for r in SELECTION) == 2
    assert any(r[5][0] == MATRIX and (r[5][3] or 0) > 65536 for r in rows)
    assert any(r[5][0] == DOT2 and (r[5][3] or 0) > 49152 for r in rows)
    assert {ROW[n][5][1] for n in MATRIX_KS} == {1, 2, 3, 4} and all(ROW[n][5][1] == k for n, k in MATRIX_KS.items())


@pytest.mark.parametrize("name", IDS)
def test_selection_table_host(pkg, name):
    """the planner on the host, without a device (mfm_hosttwin_resampler_form): natural and forced"""
    b = pkg.binding
    row = ROW[name]
    taps = _row_taps(row)
    for forced in (False, True):
        if row[5] is None:
            with pytest.raises(pkg.MfmError) as ei:
                b.hosttwin_resampler_form(taps, row[1], row[2], 4096, force_dot2=forced)
            assert ei.value.code == b.MFM_E_INVAL
            continue
        got = b.hosttwin_resampler_form(taps, row[1], row[2], 4096, force_dot2=forced)
        _check_form(f"{name} forced={forced}", got, _expect(row, forced))
        # max_out as documented: (max_in + plen + 64) I / D + 8, rounded up to 8
        assert got["max_out"] == (((4096 + row[7] + 64) * row[1]) // row[2] + 8 + 7) // 8 * 8
        assert got["dc_p"] == 0


def test_host_twin_refuses_what_create_refuses(pkg):
    """create's argument checks, answered without a device: MFM_E_INVAL, whatever device the configuration names"""
    b = pkg.binding
    lib = pkg.load_library()
    taps = _taps(81, "random", 1)
    good = dict(abi_version=b.MFM_ABI_VERSION, device=12345, nr_channels=3, interpolate=4, decimate=5, max_in_samples=4096)
    f = b.ResamplerForm()

    def call(nr=taps.size, co=taps, **kw):
        cfg = b.ResamplerConfig(**dict(good, **kw))
        return lib.mfm_hosttwin_resampler_form(C.byref(cfg), co.ctypes.data_as(C.POINTER(C.c_int16)), nr, C.byref(f))

    assert call() == 0 and f.form == MATRIX and f.k_steps == 2   # a device that does not exist is not looked for
    for bad in (dict(abi_version=b.MFM_ABI_VERSION + 1), dict(interpolate=0), dict(decimate=0), dict(nr_channels=0),
                dict(max_in_samples=0)):
        assert call(**bad) == b.MFM_E_INVAL, bad
    assert call(nr=0) == b.MFM_E_INVAL
    assert lib.mfm_hosttwin_resampler_form(None, taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, C.byref(f)) == b.MFM_E_INVAL
    # a call whose phase walk does not fit 32 bits: out_cap * D >= 2^32
    assert call(max_in_samples=1 << 30) == b.MFM_E_INVAL
    # the DC blocker's p = (int16)((1 - pole) * 16384), filter/dc_blocker.h:56
    for pole, p in ((0.9999, 1), (0.999, 16), (0.9, 1638), (0.5, 8192), (0.0, 16384), (-0.99, 32604)):
        assert b.hosttwin_resampler_form(taps, 4, 5, 4096, dc_pole=pole)["dc_p"] == p
    # the matrix block twin has nothing to evaluate where the matrix form is not chosen, or for a phase that does not exist
    x = np.zeros(64, np.int16)
    with pytest.raises(pkg.MfmError):
        b.hosttwin_resampler_matrix_block(_taps(41, "random", 2), 3, 2, 0, x)
    with pytest.raises(pkg.MfmError):
        b.hosttwin_resampler_matrix_block(taps, 4, 5, 4, x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_selection_table(pkg, name):
    """what create chose, as get_form reports it - and that it is what the host twin planned; no kernel runs"""
    b = pkg.binding
    row = ROW[name]
    taps = _row_taps(row)
    for forced in (False, True):
        if row[5] is None:
            with pytest.raises(pkg.MfmError) as ei:
                pkg.Resampler(3, taps, row[1], row[2], 4096, device=0, force_dot2=forced)
            assert ei.value.code == b.MFM_E_INVAL
            continue
        twin = b.hosttwin_resampler_form(taps, row[1], row[2], 4096, nr_channels=3, force_dot2=forced)
        gpu = pkg.Resampler(3, taps, row[1], row[2], 4096, device=0, force_dot2=forced)
        got = gpu.form()
        assert got["max_out"] == gpu.max_out()
        gpu.close()
        _check_form(f"{name} forced={forced}", got, _expect(row, forced))
        assert got == twin, name


# ------------------------------------------------------------------------------------------------ (b) tables on the CPU

@pytest.mark.parametrize("name", ["4_5_t40", "4_5_t81", "4_5_t256", "1_2_t200", "16_25_t821"])
def test_matrix_tables_match_the_oracle_at_every_phase(pkg, ora, name):
    """one block of 16 outputs from the tables the matrix kernel reads (A fragments in lane order, row constants, byte planes
    in padded rows), for every carried phase phi < I, against the oracle started at that phase: after a prefix that makes it
    produce m outputs it stands at sample floor(m D / I) with phase m D % I.  Full-scale random input plus rows of +32767 and
    -32768; random taps within +-32639, so the int32 sums wrap."""
    b = pkg.binding
    _, interp, decim, ntaps, _, natural, _, plen = ROW[name]
    taps = _row_taps(ROW[name])
    form = b.hosttwin_resampler_form(taps, interp, decim, 4096)
    assert (form["form"], form["k_steps"]) == (MATRIX, natural[1])
    rng = np.random.RandomState(ntaps)
    window = (15 * decim + interp - 1) // interp + plen   # the samples a block's 16 outputs can touch, from its first
    n = ((interp + 16) * decim) // interp + plen + 64
    rows = [rng.randint(-32768, 32768, size=n).astype(np.int16), np.full(n, 32767, np.int16), np.full(n, -32768, np.int16)]
    wants = [ora.Resampler(taps, interp, decim).feed(x) for x in rows]
    seen = set()
    for m in range(interp):
        phi, pos = (m * decim) % interp, (m * decim) // interp
        seen.add(phi)
        for x, w in zip(rows, wants):
            want = w[m:m + 16]
            assert want.size == 16
            got = b.hosttwin_resampler_matrix_block(taps, interp, decim, phi, x[pos:])
            assert np.array_equal(got, want), f"{name}: phase {phi}: {got} != {want}"
            # nothing past the block's window is read: the same outputs from the window alone (samples behind it count as 0)
            got = b.hosttwin_resampler_matrix_block(taps, interp, decim, phi, x[pos:pos + window])
            assert np.array_equal(got, want), f"{name}: phase {phi}, window only"
    assert seen == set(range(interp))   # I and D are coprime in these rows: the first I outputs start at every phase once


# ------------------------------------------------------------------------------------------- (c) every instance on the GPU

def _three_channels(rng, n):
    x = rng.randint(-32768, 32768, size=(3, n)).astype(np.int16)
    x[1] = 32767
    x[2] = -32768
    return x


def _bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _run_instance(pkg, ora, row, forced, with_bits):
    b = pkg.binding
    _, interp, decim, ntaps, _, natural, _, plen = row
    taps = _row_taps(row)
    want_form = _expect(row, forced)
    # more than two workgroups of outputs in one call, the last one partial: a workgroup is 4096 outputs of the matrix form,
    # 1024 of v_dot2
    outputs = 9000 if want_form["form"] == MATRIX else 2500
    max_in = -(-outputs * decim // interp)
    # ragged calls: fewer samples than a phase (no output), nothing, 1, 7, one whole max_in_samples, 1, nothing, the rest
    sizes = [plen - 1, 0, 1, 7, max_in, 1, 0, max_in // 3 + 5]
    rng = np.random.RandomState(ntaps + decim)
    x = _three_channels(rng, sum(sizes))
    for invert, pol in ((False, b.MFM_BITS_NEG), (True, b.MFM_BITS_POS)):
        gpu = pkg.Resampler(3, taps, interp, decim, max_in, device=0, invert=invert, force_dot2=forced)
        _check_form(f"{row[0]} forced={forced}", gpu.form(), want_form)   # first: a quiet fallback fails here
        gbits = pkg.Resampler(3, taps, interp, decim, max_in, device=0, invert=invert, force_dot2=forced) if with_bits else None
        refs = [ora.Resampler(taps, interp, decim, invert=invert) for _ in range(3)]
        pos, total = 0, 0
        for k, m in enumerate(sizes):
            want = np.stack([r.feed(x[c, pos:pos + m]) for c, r in enumerate(refs)])
            got = gpu.process_host(x[:, pos:pos + m])
            what = f"{row[0]} forced={forced} invert={invert} call {k} ({m} samples)"
            assert got.shape == want.shape, (what, got.shape, want.shape)
            if k == 0:
                assert got.shape[1] == 0, what
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                raise AssertionError(f"{what}: {len(bad)} samples differ from the oracle; first at (chan, n) = {bad[0]}")
            if gbits is not None:
                words, nbits = gbits.process_bits_host(x[:, pos:pos + m], pol)
                assert nbits == want.shape[1] and words.shape[1] == (nbits + 31) // 32, what
                pred = (want < 0) if pol == b.MFM_BITS_NEG else (want > 0)
                if nbits:
                    assert np.array_equal(_bits_of(words, nbits), pred.astype(np.uint8)), f"{what}: sign bits"
                if nbits % 32:
                    assert not (words[:, -1] >> np.uint32(nbits % 32)).any(), f"{what}: bits behind the last output"
            pos += m
            total += got.shape[1]
        gpu.close()
        if gbits is not None:
            gbits.close()
        assert total > outputs


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNNABLE)
def test_every_row_matches_oracle_in_its_natural_form(pkg, ora, name):
    """every row of the table that is not a refusal: KS = 1 .. 4 (ids 4_5_t40, 4_5_t81, 4_5_t256, 1_2_t200 also give sign
    bits), matrix LDS up to 124 KB, every fallback to v_dot2, v_dot2 LDS above 48 KB"""
    _run_instance(pkg, ora, ROW[name], False, name in MATRIX_KS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FORCED, ids=[f"np{ROW[n][6]}_{n}" for n in FORCED])
def test_every_dot2_instance_matches_oracle(pkg, ora, name):
    """MFM_RS_FORCE_DOT2 on the rows whose phase gives NP = 4, 8, ..., 32 and 0: PCM and sign bits"""
    _run_instance(pkg, ora, ROW[name], True, True)


# ---------------------------------------------------------------------------------------------------- (d) the DC blocker

# outputs per call: the edges of the blocker's 64-sample trips (63/64/65, 127/128/129: i + 128 <= n_out decides the prefetch)
DC_CALLS = [1000, 1, 64, 7, 129, 63, 128, 65, 127, 200, 64, 1, 128, 1000, 7, 65]


@pytest.mark.gpu
@pytest.mark.parametrize("pole", [0.9999, 0.999, 0.9, 0.5, 0.0, -0.99])
def test_dc_blocker_alone(pkg, ora, pole):
    """1/1 with the single tap 16384 makes the resampler an identity (r14(16384 x) = x), so the DC blocker alone is under test:
    70 channels (a second 64-lane block with 6 lanes live), p = 1, 16, 1638, 8192, 16384, 32604 on the multiplier, state
    carried over calls whose output counts sit on the edges of the 64-sample trips.  A constant +32767 and an alternating
    -32768 / 32767 row take y beyond int16, so the carried y_(n-1) is the unclipped one."""
    nch = 70
    taps = np.array([16384], np.int16)
    sizes = [DC_CALLS[0] + 4] + DC_CALLS[1:]   # the first call keeps one phase length (4) back
    n = sum(sizes)
    rng = np.random.RandomState(int(abs(pole) * 10000))
    x = rng.randint(-32768, 32768, size=(nch, n)).astype(np.int16)
    x[1] = 32767
    x[2, 0::2] = -32768
    x[2, 1::2] = 32767
    x[68] = 32767
    x[69, 0::2] = 32767
    x[69, 1::2] = -32768
    gpu = pkg.Resampler(nch, taps, 1, 1, max(sizes), device=0, dc_pole=pole)
    form = gpu.form()
    assert (form["form"], form["k_steps"], form["phase_len"]) == (MATRIX, 1, 4)
    assert form["dc_p"] == {0.9999: 1, 0.999: 16, 0.9: 1638, 0.5: 8192, 0.0: 16384, -0.99: 32604}[pole]
    refs = [ora.Resampler(taps, 1, 1, dc_pole=pole) for _ in range(nch)]
    plain = ora.Resampler(taps, 1, 1)
    assert np.array_equal(plain.feed(x[0]), x[0, :n - 4])   # the identity the test rests on
    pos = 0
    for k, m in enumerate(sizes):
        got = gpu.process_host(x[:, pos:pos + m])
        want = np.stack([r.feed(x[c, pos:pos + m]) for c, r in enumerate(refs)])
        assert got.shape == want.shape and got.shape[1] == DC_CALLS[k], (k, got.shape, want.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"pole {pole}, call {k} ({DC_CALLS[k]} outputs): {len(bad)} samples differ; first at (chan, n) = "
                                 f"{bad[0]}, channels {np.unique(bad[:, 0])[:8]}")
        pos += m
    gpu.close()


# ---------------------------------------------------------------------------------------------------- (e) input placement

class _Hip:
    def __init__(self):
        rt = C.CDLL("libamdhip64.so")
        rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        rt.hipFree.argtypes = [C.c_void_p]
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        self.rt = rt

    def upload(self, a):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def rows(self, ptr, stride, n, nch):
        host = np.zeros((nch, max(n, 1)), np.int16)
        if n:
            assert self.rt.hipMemcpy2D(host.ctypes.data, host.shape[1] * 2, ptr, stride * 2, n * 2, nch, 2) == 0
        return host[:, :n]

    def free(self, p):
        assert self.rt.hipFree(p) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,forced", [("4_5_t81", False), ("4_5_t81", True), ("1_2_t200", False)],
                         ids=["4_5_t81_matrix", "4_5_t81_dot2", "1_2_t200_matrix"])
def test_input_rows_anywhere_in_a_larger_buffer(pkg, ora, name, forced):
    """process_device with rows that start 0, 1, 3 and 7 samples into a larger device buffer (the matrix form reads 16 bytes
    at a time from rows that are then only 2-byte aligned, the v_dot2 staging single samples) and strides of nr_in + 5 and
    3 nr_in; everything around the rows is full-scale noise that must not be read as samples.  Then the bound: nr_in =
    max_in_samples is accepted, max_in_samples + 1 is MFM_E_INVAL and leaves the stream where it was."""
    b = pkg.binding
    row = ROW[name]
    _, interp, decim, ntaps, _, _, _, plen = row
    taps = _row_taps(row)
    nch, max_in = 3, 6000
    hip = _Hip()
    rng = np.random.RandomState(ntaps + 77)
    gpu = pkg.Resampler(nch, taps, interp, decim, max_in, device=0, force_dot2=forced)
    _check_form(name, gpu.form(), _expect(row, forced))
    refs = [ora.Resampler(taps, interp, decim) for _ in range(nch)]
    calls = [(off, stride_of) for off in (0, 1, 3, 7) for stride_of in (lambda n: n + 5, lambda n: 3 * n)]
    nr = [5001, 777, 5999, 1234, 4096, 33, 6000, 2501]   # one of them = max_in_samples
    for k, ((off, stride_of), n) in enumerate(zip(calls, nr)):
        stride = stride_of(n)
        buf = rng.randint(-32768, 32768, size=off + nch * stride + 16).astype(np.int16)
        x = np.stack([buf[off + c * stride:off + c * stride + n] for c in range(nch)])
        d = hip.upload(buf)
        yptr, ystride, ny = gpu.process_device(d + 2 * off, stride, n)
        got = hip.rows(yptr, ystride, ny, nch)   # (the copy waits for the kernels on the default stream)
        hip.free(d)
        want = np.stack([r.feed(x[c]) for c, r in enumerate(refs)])
        assert got.shape == want.shape and ny > 0, (k, got.shape, want.shape)
        assert np.array_equal(got, want), f"{name} forced={forced}: call {k}, row offset {off}, stride {stride}, {n} samples"
    # one sample too many: refused, and the stream goes on as if the call had not been made
    buf = rng.randint(-32768, 32768, size=nch * (max_in + 1)).astype(np.int16)
    d = hip.upload(buf)
    with pytest.raises(pkg.MfmError) as ei:
        gpu.process_device(d, max_in + 1, max_in + 1)
    assert ei.value.code == b.MFM_E_INVAL
    yptr, ystride, ny = gpu.process_device(d, max_in + 1, max_in)
    got = hip.rows(yptr, ystride, ny, nch)
    hip.free(d)
    want = np.stack([r.feed(buf[c * (max_in + 1):c * (max_in + 1) + max_in]) for c, r in enumerate(refs)])
    assert got.shape == want.shape and np.array_equal(got, want)
    gpu.close()
