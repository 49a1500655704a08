"""Two-stream launches and the early carry on every form they run on (include/multifm_hip.h: MFM_F_OVERLAP,
mfm_engine_stream; mfm_launch_plan.h launch_plan, which mfm_engine.hip's launch_locked queues; mfm_kernel_v3.hip, the `L.head_n != 0 && tile == 0` block).

tests/test_launch_overlap.py runs the path on one form (D 96, 128 taps, one slice, the sub-plane layout, no filtered IQ).  Here:
the three layouts of the second-generation kernel at every k-step count, 64 and 65 channels, several slices, filtered IQ, the
copy-back fallback (more first chunks than workgroup slots), MFM_F_OVERLAP host-fed, with 8-bit blocks and format changes, on the
long-filter kernel (layout 3) and with three input buffers, reset() and seek() per layout.

A launch goes to the other stream only when it fills the workgroup slots more than once, so every case restates the engine's
rule from stats() and sizes its blocks from it -

    slots   = 256 * max(1, min(2, 163840 // lds_bytes))           (layout 3: 256, one workgroup per CU)
    nslices = ceil(nr_channels / slice_channels)
    ntiles  = ceil(n_new / outputs_per_tile)
    a launch alternates iff ntiles * nslices > slots and n_new * D >= tail + D

- and asserts that overlapped_launches, launches, launches_8bit and pinned EQUAL what the rule predicts for the blocks fed (at
least four alternating launches in every case): an engine that stays on one stream fails.  The big block B gives
slots / nslices + 3 tiles (about 33 000 channel-tiles whatever the geometry); the seam sequence B, B-1, B-2, B-3, one tile,
B, 1 sample, B-D-1, B carries lengths of every residue mod 4 - also among those the kernel's patch reads - and enters and
leaves the path twice.

Every comparison is bit-exact against the oracle, fed the engine's own Q14 tables (mfm_engine_get_channel), on ALL channels and
ALL outputs: at these sizes a whole oracle run is 1-3 G complex multiply-adds, a second or less on the oracle's thread pool.
Channels are programmed with add_channel_q14: seeded random taps, even channels within one byte (|tap| <= 127), odd channels up
to 32639; every fourth channel an exact rotator, +(16384, 0) and -(16384, 0) in turn, the others an increment drawn (seeded)
from four general ones - 101 kHz, 777 Hz, an eighth turn, a quarter turn at 2.4 MS/s / 96 - because the engine keeps one
rotator table per distinct increment (up to 53 000 entries each): thousands of distinct ones would be a test of commit()."""
import concurrent.futures
import os
import time

import numpy as np
import pytest

from test_gpu_parity import _oracle_tables
from test_launch_overlap import D2H, H2D, _hip

pytestmark = pytest.mark.gpu

# the oracle's thread pool: a job on the GPU machines may use 16 CPUs, whatever os.cpu_count() says
THREADS = min(16, os.cpu_count() or 8)
FS = 2400000
LDS_PER_CU = 163840
CS16, CS8, RTLSDR_U8 = 0, 1, 3


# ------------------------------------------------------------------------------------------------ the rule, restated

def _rule(st, nch):
    """(slots, nslices, outputs per tile) of launch_plan()'s alternation rule (mfm_launch_plan.h), from stats() alone"""
    slots = 256 * max(1, min(2, LDS_PER_CU // st["lds_bytes"]))
    return slots, -(-nch // st["slice_channels"]), st["outputs_per_tile"]


def _big_block(slots, nslices, ot, D):
    """the smallest round block with three tiles more than one per slot and slice: B-3 and B-D-1 still alternate"""
    return (slots // nslices + 3) * ot * D


def _patched(pred):
    """carried lengths that the KERNEL reads from the ring: left by an alternating launch to a launch that alternates too (a
    launch that does not takes its head back to the buffer's front with mfm_carry_kernel first)"""
    return [a[2] for a, b in zip(pred, pred[1:]) if a[1] and b[1]]


def _seam_sizes(rule, D, T):
    """B, B-1, B-2, B-3, one tile's worth, B, 1 sample, B-D-1, B.  The ninth block is there for the head the eighth leaves:
    with it the carried lengths D + tail that the kernel's patch reads - not only those a copy takes back - take every residue
    mod 4 (the tails go t, t-1, t-3 and, behind the eighth block, t-6).  That holds for the round B wherever D % 4 == 0; at
    D = 25 with 150 taps it does not, and B gives way by the fewest samples (at most 3: the tile count stays) for which it does."""
    for r in range(4):
        B = _big_block(*rule, D) - r
        sizes = [B, B - 1, B - 2, B - 3, rule[2] * D, B, 1, B - D - 1, B]
        if {n % 4 for n in _patched(_predict([(n, False) for n in sizes], D, T, rule))} == {0, 1, 2, 3}:
            return sizes
    raise AssertionError(f"no block size near {B} carries every residue mod 4")


def _predict(launches, D, T, rule, alternates=lambda raw8: True):
    """launches: (samples, read as bytes) per launch_locked() pass.  Per pass: (outputs, alternates, carried length D + tail)."""
    slots, nslices, ot = rule
    tail, out = 0, []
    for n, raw8 in launches:
        avail = tail + n
        n_new = (avail - T) // D + 1 if avail >= T else 0
        ntiles = -(-n_new // ot)
        two = n_new > 0 and alternates(raw8) and ntiles * nslices > slots and n_new * D >= tail + D
        tail = avail - n_new * D
        out.append((n_new, two, D + tail))
    return out


def _assert_counts(st, pred, raw8=()):
    """the engine's counters against the prediction; at least four alternating launches, or the case proves nothing"""
    want_two = sum(1 for p in pred if p[1])
    want_launches = sum(1 for p in pred if p[0])
    want_8bit = sum(1 for p, r in zip(pred, raw8) if p[0] and r)
    assert want_two >= 4, pred
    assert st["overlapped_launches"] == want_two, (st["overlapped_launches"], want_two, pred)
    assert st["launches"] == want_launches and st["launches_8bit"] == want_8bit and st["pinned"] == 0, (st, pred)
    assert st["outputs"] == sum(p[0] for p in pred)


# ------------------------------------------------------------------------------------------------ channels, oracle

_cache = {}


def _incr_pool(ora):
    if "pool" not in _cache:
        _cache["pool"] = [tuple(int(v) for v in ora.rot_incr(o, 2400000, 96)) for o in (101000, 777, 3125, -6250)]
        assert _cache["pool"][3] == (0, 16384) and all(abs(p[0]) != 16384 for p in _cache["pool"])
    return _cache["pool"]


def _q14_engine(pkg, ora, D, T, nch, block, flags, want_iq=False, seed=0, exact_slice=False, commit=True, **kw):
    """(engine, its stats).  exact_slice: the first 64 channels are exact rotators too, so that one slice holds nothing else.
    commit=False: the engine with its channels added and what the planner says it will run (mfm_hosttwin_kernel_form) - the
    block size follows from the form, and the engine wants its largest block at creation."""
    rng = np.random.default_rng(1000 * D + T + seed)
    pool = _incr_pool(ora)
    eng = pkg.Engine(FS, D, block, device=0, flags=flags, **kw)
    nexact = 0
    for c in range(nch):
        lim = 127 if c % 2 == 0 else 32639
        cre = rng.integers(-lim, lim + 1, size=T).astype(np.int16)
        cim = rng.integers(-lim, lim + 1, size=T).astype(np.int16)
        if c % 4 == 0 or (exact_slice and c < 64):
            incr = (16384, 0) if (c // 4) % 2 == 0 else (-16384, 0)
            nexact += 1
        else:
            incr = pool[int(rng.integers(len(pool)))]
            nexact += 1 if incr == (0, 16384) else 0   # the quarter turn is a rotator class of its own, and counted as exact
        eng.add_channel_q14(cre, cim, incr, want_iq=want_iq)
    if not commit:
        st = eng.kernel_form()
        eng.close()
        assert st["rot_exact_channels"] == nexact >= 1
        return None, st
    eng.commit()
    st = eng.stats()
    assert st["rot_exact_channels"] == nexact >= 1 and st["nr_channels"] == nch
    return eng, st


def _form(st, k_steps, slice_channels=64):
    """a quiet fallback to another kernel form fails here"""
    assert (st["kernel_variant"], st["slice_channels"], st["k_steps"], st["outputs_per_tile"]) == (2, slice_channels, k_steps, 64), st


def _oracle(ora, eng, nch, iq, D, want_iq=False, before=0):
    """the oracle on the engine's own tables, every channel, the whole stream; before: the stream starts at that output"""
    cre, cim, incr = _oracle_tables(eng, nch)
    if 0 == before:
        return ora.run_channels(iq, cre, cim, incr, D, threads=THREADS, want_iq=want_iq)

    def one(c):
        ch = ora.Channel(cre[c], cim[c], D, incr[c])
        ch.skip_outputs(before)
        pcm, q = ch.feed(iq)
        ch.close()
        return pcm, q
    with concurrent.futures.ThreadPoolExecutor(THREADS) as ex:
        got = list(ex.map(one, range(nch)))
    return np.stack([g[0] for g in got]), (np.stack([g[1] for g in got]) if want_iq else None)


def _random_s16(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(n, 2), dtype=np.int16)


def _assert_exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ from the oracle; first at {bad[0]}, channels "
                             f"{np.unique(bad[:, 0])[:8]}, outputs {np.unique(bad[:, 1])[:8]}")


# ------------------------------------------------------------------------------------------------ feeding

class _Dev:
    """Device-resident blocks through acquire_input[_bytes] / submit, two launches in flight: the PCM (and filtered IQ) of a
    pair of launches is read from the two output slots after the second has been submitted."""

    def __init__(self, eng, nch, D, T, want_iq=False, before=0):
        self.eng, self.hip, self.nch, self.D, self.T, self.want_iq = eng, _hip(), nch, D, T, want_iq
        self.tail, self.produced, self.pending, self.pcm, self.q = 0, before, [], [], []

    def put(self, blk, fmt=CS16):
        """blk: [n][2] int16, or uint8 for an 8-bit format"""
        n = blk.shape[0]
        ptr, cap = self.eng.acquire_input() if fmt == CS16 else self.eng.acquire_input_bytes(fmt)
        assert cap >= n and blk.flags["C_CONTIGUOUS"] and blk.nbytes == n * (4 if fmt == CS16 else 2)
        assert self.hip.hipMemcpy(ptr, blk.ctypes.data, blk.nbytes, H2D) == 0
        self.eng.submit(n, producer_stream=0, wait_producer=False)
        avail = self.tail + n
        want = (avail - self.T) // self.D + 1 if avail >= self.T else 0
        self.tail = avail - want * self.D
        if want:
            dptr, stride, nout, qptr = self.eng.last_output_device()
            assert nout == want
            self.pending.append((dptr, qptr, nout, stride))
            self.produced += nout
        if len(self.pending) == 2:
            self.collect()

    def collect(self):
        self.eng.sync()
        for dptr, qptr, nout, stride in self.pending:
            pcm = np.empty((self.nch, stride), np.int16)
            assert self.hip.hipMemcpy(pcm.ctypes.data, dptr, pcm.nbytes, D2H) == 0
            self.pcm.append(pcm[:, :nout].copy())
            if self.want_iq:
                assert qptr
                q = np.empty((self.nch, stride, 2), np.int16)
                assert self.hip.hipMemcpy(q.ctypes.data, qptr, q.nbytes, D2H) == 0
                self.q.append(q[:, :nout].copy())
        self.pending = []

    def result(self):
        self.collect()
        return np.concatenate(self.pcm, axis=1), (np.concatenate(self.q, axis=1) if self.want_iq else None)


def _feed_s16(dev, iq, sizes):
    pos = 0
    for n in sizes:
        dev.put(iq[pos:pos + n])
        pos += n
    assert pos == iq.shape[0]


def _seam_case(pkg, ora, D, T, nch, k_steps, flags, want_iq=False, exact_slice=False, fallback=False, slots=None):
    """the seam sequence, device-resident, on one geometry: form, counters and every output of every channel"""
    t0 = time.perf_counter()
    _, st = _q14_engine(pkg, ora, D, T, nch, 1 << 16, flags, want_iq, exact_slice=exact_slice, commit=False)
    rule = _rule(st, nch)
    assert slots is None or rule[0] == slots, (st["lds_bytes"], slots)
    sizes = _seam_sizes(rule, D, T)
    eng, st = _q14_engine(pkg, ora, D, T, nch, sizes[0], flags, want_iq, exact_slice=exact_slice)
    _form(st, k_steps)
    assert _rule(st, nch) == rule
    if exact_slice:
        assert st["rot_fast_slices"] >= 1, st
    if fallback:
        # more first chunks (eight per slice, dealt over the XCDs) than workgroup slots: a workgroup would come to a first
        # chunk as its second item, which the kernel's patch does not handle - the engine copies the head back instead
        assert 8 * rule[1] > rule[0], rule
    pred = _predict([(n, False) for n in sizes], D, T, rule)
    assert {p[2] % 4 for p in pred} == {0, 1, 2, 3} == {n % 4 for n in _patched(pred)}, pred
    iq = _random_s16(sum(sizes), 7 * D + T + nch)
    dev = _Dev(eng, nch, D, T, want_iq)
    _feed_s16(dev, iq, sizes)
    pcm, q = dev.result()
    st = eng.stats()
    ref, refq = _oracle(ora, eng, nch, iq, D, want_iq)
    eng.close()
    _assert_counts(st, pred)
    if fallback:
        assert st["grid_last"] == rule[0], (st["grid_last"], rule)
    _assert_exact(pcm, ref, f"PCM, D {D}, {T} taps, {nch} channels, flags {flags:#x}")
    if want_iq:
        _assert_exact(q.reshape(nch, -1), refq.reshape(nch, -1), f"filtered IQ, D {D}, {T} taps, {nch} channels")
    print(f"D {D} T {T} ch {nch}: B {sizes[0]}, rule {rule}, {sum(p[1] for p in pred)} alternating launches, "
          f"{time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ 1. layouts and k-steps

# (D, taps, channels, k-steps, workgroups per CU the LDS image leaves room for)
LAYOUTS = [
    # [sub]: D % 32 == 0
    (32, 32, 64, 1, 2), (32, 128, 64, 4, 2),   # (32, 128): a window crosses four rows, extra = 3
    (64, 64, 64, 2, 2), (96, 96, 64, 4, 2),
    (128, 128, 64, 4, 1), (128, 128, 65, 4, 1),   # 94 208 bytes of LDS: one workgroup per CU, 256 slots
    # [crow]: D % 8 == 0, D % 32 != 0
    (8, 128, 64, 4, 2), (24, 64, 64, 2, 2), (40, 128, 64, 4, 2), (40, 128, 65, 4, 2),
    (120, 128, 64, 4, 1),                         # 102 400 bytes: one workgroup per CU
    # [pad25]: six k-steps whatever the tap count
    (25, 128, 64, 6, 2), (25, 128, 65, 6, 2), (25, 150, 64, 6, 2),
]


@pytest.mark.parametrize("D,T,nch,k_steps,wg_per_cu", LAYOUTS, ids=[f"d{r[0]}_t{r[1]}_c{r[2]}" for r in LAYOUTS])
def test_seams_on_every_layout_and_k_step_count(pkg, ora, D, T, nch, k_steps, wg_per_cu):
    """The head patch indexes the ring through stage_index, which differs per layout (chunk rows on [crow]; on [pad25] the
    alignment term and the clamp for chunks in front of the buffer) and with the staging chunks per thread.  Default flags:
    a device-only engine alternates by itself.  65 channels: a second slice of one channel, with its own tile-0 workgroup."""
    _seam_case(pkg, ora, D, T, nch, k_steps, pkg.binding.MFM_F_DEVICE_ONLY, slots=256 * wg_per_cu)


def test_sub_layout_at_decimation_160_does_not_exist(pkg):
    """[sub] takes at most four k-steps (128 taps) and the engine refuses taps < decimation (the reference dereferences NULL
    there, direct_fir.c:394-398): D = 160 with 128 taps cannot be committed, so there is no such form to alternate.  The
    geometries that land on one workgroup per CU are (128, 128) and (120, 128) above."""
    b = pkg.binding
    eng = pkg.Engine(FS, 160, 1 << 16, device=0, flags=b.MFM_F_DEVICE_ONLY)
    with pytest.raises(b.MfmError) as err:
        eng.add_channel_q14(np.ones(128, np.int16), np.ones(128, np.int16), (16384, 0))
    eng.close()
    assert err.value.args and "decimation" in str(err.value)


# ------------------------------------------------------------------------------------------------ 2. slices

SLICES = [
    # (D, taps, channels, slices, k-steps, MFM_F_SLICE_64)
    (96, 128, 192, 3, 4, False), (96, 128, 320, 5, 4, False), (96, 128, 511, 8, 4, False),
    (96, 128, 768, 12, 4, True),    # from 512 channels on 128-tap filters run on slices of 128 unless MFM_F_SLICE_64
    (32, 64, 1024, 16, 2, False),
    (96, 128, 1024, 16, 4, True),
]


@pytest.mark.parametrize("D,T,nch,nslices,k_steps,slice64", SLICES, ids=[f"d{r[0]}_t{r[1]}_c{r[2]}" for r in SLICES])
def test_seams_on_several_slices(pkg, ora, D, T, nch, nslices, k_steps, slice64):
    """Every slice has a tile-0 workgroup of its own that reads the ring: slice counts that leave holes in the dealing over the
    eight XCDs (3, 5, 12), a partial last slice (511: 63 channels), 16 slices; one slice of exact rotators only."""
    b = pkg.binding
    assert -(-nch // 64) == nslices
    _seam_case(pkg, ora, D, T, nch, k_steps, b.MFM_F_DEVICE_ONLY | (b.MFM_F_SLICE_64 if slice64 else 0), exact_slice=True)


# ------------------------------------------------------------------------------------------------ 3. filtered IQ

@pytest.mark.parametrize("D,T,k_steps", [(96, 128, 4), (40, 128, 4), (25, 128, 6)], ids=["sub", "crow", "pad25"])
def test_seams_with_filtered_iq(pkg, ora, D, T, k_steps):
    """want_iq on every channel: other kernel instances; PCM and filtered IQ against the oracle."""
    _seam_case(pkg, ora, D, T, 64, k_steps, pkg.binding.MFM_F_DEVICE_ONLY, want_iq=True)


# ------------------------------------------------------------------------------------------------ 4. copy-back fallback

@pytest.mark.parametrize("D,T,nch,k_steps,slots,slice64", [(32, 64, 4160, 2, 512, False), (128, 128, 2112, 4, 256, True)],
                         ids=["d32_t64_c4160", "d128_t128_c2112"])
def test_copy_back_when_first_chunks_exceed_the_slots(pkg, ora, D, T, nch, k_steps, slots, slice64):
    """4160 channels (65 slices) of 64 taps at D = 32: 8 * 65 = 520 first-chunk items on 512 slots; 2112 channels (33 slices of
    64, MFM_F_SLICE_64) at (128, 128), one workgroup per CU: 264 on 256.  The launches still alternate and the carry still goes
    to the ring, but mfm_carry_kernel copies it back to the buffer's front and the kernel does not patch: exact on every
    channel, counters as predicted, a grid of exactly the slots."""
    b = pkg.binding
    _seam_case(pkg, ora, D, T, nch, k_steps, b.MFM_F_DEVICE_ONLY | (b.MFM_F_SLICE_64 if slice64 else 0), fallback=True, slots=slots)


# ------------------------------------------------------------------------------------------------ 5. MFM_F_OVERLAP, host-fed

def _host_fed(eng, iq, sizes, busy, want_iq=False):
    """push / fetch / release through the host mirror, MFM_E_BUSY drained; [(first output, pcm, iq)] per launch"""
    parts, pos = [], 0

    def drain():
        while True:
            got = eng.fetch()
            if got is None:
                return
            assert got[0] == (parts[-1][0] + parts[-1][1].shape[1] if parts else 0)
            parts.append(got)
    for n in sizes:
        while True:
            rc = eng.push(iq[pos:pos + n])
            if rc == 0:
                break
            assert rc == busy, eng.lib.mfm_last_error()
            drain()
        pos += n
    assert pos == iq.shape[0]
    while eng.flush() == busy:
        drain()
    eng.sync()
    drain()
    return parts


@pytest.mark.parametrize("D,T,nch,k_steps", [(32, 64, 1024, 2), (40, 128, 256, 4)], ids=["sub_1024", "crow_256"])
def test_overlap_flag_host_fed(pkg, ora, D, T, nch, k_steps):
    """MFM_F_OVERLAP on an engine with a host mirror: the H2D copies and the early carry's copy share the copy stream, the PCM
    is mirrored out of four slots.  The seam sequence."""
    b = pkg.binding
    _, st = _q14_engine(pkg, ora, D, T, nch, 1 << 16, b.MFM_F_OVERLAP, commit=False)
    rule = _rule(st, nch)
    sizes = _seam_sizes(rule, D, T)
    eng, st = _q14_engine(pkg, ora, D, T, nch, sizes[0], b.MFM_F_OVERLAP)
    _form(st, k_steps)
    pred = _predict([(n, False) for n in sizes], D, T, rule)
    assert {p[2] % 4 for p in pred} == {0, 1, 2, 3} == {n % 4 for n in _patched(pred)}, pred
    iq = _random_s16(sum(sizes), 5 * D + nch)
    parts = _host_fed(eng, iq, sizes, b.MFM_E_BUSY)
    st = eng.stats()
    ref, _ = _oracle(ora, eng, nch, iq, D)
    eng.close()
    _assert_counts(st, pred)
    assert [p[1].shape[1] for p in parts] == [p[0] for p in pred if p[0]]
    _assert_exact(np.concatenate([p[1] for p in parts], axis=1), ref, f"host-fed, D {D}, {nch} channels")


# ------------------------------------------------------------------------------------------------ 6. 8-bit blocks

@pytest.mark.parametrize("overlap_flag", [True, False], ids=["overlap", "default"])
@pytest.mark.parametrize("fmt", [RTLSDR_U8, CS8], ids=["rtlsdr_u8", "cs8"])
def test_8bit_blocks_and_format_changes(pkg, ora, fmt, overlap_flag):
    """[sub] 512 channels, 96 taps, D = 96 (MFM_F_SLICE_64: by default this many channels of four k-steps run on slices of 128),
    blocks u8 B, u8 B-2, int16 B-1, int16 B-3, u8 B, u8 B.  Bytes cannot follow an int16 history - acquire_input_bytes must
    refuse, and the caller widens those blocks as the reference's front end does - so two launches read bytes.  With
    MFM_F_OVERLAP they alternate with the carry copied on the next launch's stream; with default flags they stay on one stream.
    Either way the first int16 block finds a byte history at its buffer's front, which submit() widens in place on the stream
    of that buffer's launch, and then starts the early carry."""
    b = pkg.binding
    D, T, nch = 96, 96, 512
    flags = b.MFM_F_DEVICE_ONLY | b.MFM_F_SLICE_64 | (b.MFM_F_OVERLAP if overlap_flag else 0)
    _, st = _q14_engine(pkg, ora, D, T, nch, 1 << 16, flags, commit=False)
    rule = _rule(st, nch)
    B = _big_block(*rule, D)
    eng, st = _q14_engine(pkg, ora, D, T, nch, B, flags)
    _form(st, 4)
    blocks = [(B, True), (B - 2, True), (B - 1, False), (B - 3, False), (B, True), (B, True)]   # (samples, 8-bit source)
    as_bytes = [True, True, False, False, False, False]   # what the engine can read as bytes: no int16 history in front
    pred = _predict(list(zip([n for n, _ in blocks], as_bytes)), D, T, rule, alternates=lambda raw8: overlap_flag or not raw8)
    rng = np.random.default_rng(600 + fmt)
    dev = _Dev(eng, nch, D, T)
    iq = []
    for (n, src8), raw8 in zip(blocks, as_bytes):
        if src8:
            raw = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
            raw[:4] = [[0, 255], [127, 128], [128, 127], [255, 0]]
            wide = ora.unpack_bytes(raw, fmt).reshape(-1, 2)
            if raw8:
                dev.put(raw, fmt)
            else:
                with pytest.raises(b.MfmError):
                    eng.acquire_input_bytes(fmt)
                dev.put(wide)
        else:
            wide = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
            dev.put(wide)
        iq.append(wide)
    pcm, _ = dev.result()
    st = eng.stats()
    ref, _ = _oracle(ora, eng, nch, np.concatenate(iq), D)
    eng.close()
    _assert_counts(st, pred, as_bytes)
    assert st["launches_8bit"] == 2 and st["overlapped_launches"] == (6 if overlap_flag else 4)
    _assert_exact(pcm, ref, f"8-bit format {fmt}, overlap flag {overlap_flag}")


# ------------------------------------------------------------------------------------------------ 7. layout 3

@pytest.mark.parametrize("plan,nch", [("cfg3_1024ch", 512), ("cfg5_airspy", 130)])
def test_overlap_flag_on_the_long_filter_kernel(pkg, ora, plan, nch):
    """mfm_kernel_v3l.hip (128-tap filters on slices of 128 channels; 512 taps at D = 400) alternates under MFM_F_OVERLAP
    without the ring: the carry is copied on the next launch's stream.  Its launches are sized for one workgroup per CU
    (plan_layout3 sets v_wg_per_cu = 1; mfm_v3l_wg_per_cu says 2 only for byte blocks on shifted copies), and its LDS image is
    beyond half a CU's, so the restated rule gives the same 256 slots - asserted.  Designed filters; one channel in five on
    the grid of half the output rate (exact rotators)."""
    b = pkg.binding
    fs, D, taps, offs, _ = pkg.synth.plan(plan, nr_channels=nch)
    offs = np.array(offs, np.int64)
    offs[::5] = pkg.synth.grid_offsets(nch, fs, D)[::5]
    T = len(taps)

    def make(block, commit=True):
        eng = pkg.Engine(fs, D, block, device=0, flags=b.MFM_F_DEVICE_ONLY | b.MFM_F_OVERLAP)
        for o in offs:
            eng.add_channel(int(o), taps, 1.0)
        if not commit:
            st = eng.kernel_form()
            eng.close()
            return None, st
        eng.commit()
        return eng, eng.stats()
    _, st = make(1 << 16, commit=False)
    assert (st["kernel_variant"], st["slice_channels"], st["taps_resident"]) == (2, 128, 1), st
    assert LDS_PER_CU // st["lds_bytes"] == 1 and 0 < st["rot_exact_channels"] < nch, st
    rule = _rule(st, nch)
    assert rule[0] == 256
    sizes = _seam_sizes(rule, D, T)
    eng, st = make(sizes[0])
    pred = _predict([(n, False) for n in sizes], D, T, rule)
    iq = _random_s16(sum(sizes), nch)
    dev = _Dev(eng, nch, D, T)
    _feed_s16(dev, iq, sizes)
    pcm, _ = dev.result()
    st = eng.stats()
    ref, _ = _oracle(ora, eng, nch, iq, D)
    eng.close()
    _assert_counts(st, pred)
    _assert_exact(pcm, ref, f"{plan}, {nch} channels")


# ------------------------------------------------------------------------------------------------ 8. three buffers

def test_three_buffers_gathered(pkg, ora):
    """coalesce_samples with MFM_F_GATHER | MFM_F_OVERLAP: three input buffers, a carry ring of four slots, slot
    (pass + 1) % 4.  Ragged blocks of 1..8192 samples gathered into launches of 80 000 and more - 40 tiles on 16 slices, 512
    slots - ten launches and the flush: every ring slot is reused twice."""
    b = pkg.binding
    D, T, nch, co = 32, 64, 1024, 80000
    rng = np.random.default_rng(88)
    sizes = [int(v) for v in rng.integers(1, 8193, size=220)]
    launches, pend = [], 0
    for n in sizes:     # MFM_F_GATHER: a launch once coalesce_samples have gathered, and the flush at the end
        pend += n
        if pend >= co:
            launches.append(pend)
            pend = 0
    if pend:
        launches.append(pend)
    assert len(launches) >= 10
    eng, st = _q14_engine(pkg, ora, D, T, nch, 8192, b.MFM_F_GATHER | b.MFM_F_OVERLAP, coalesce_samples=co)
    _form(st, 2)
    rule = _rule(st, nch)
    pred = _predict([(n, False) for n in launches], D, T, rule)
    assert sum(1 for p in pred if p[1]) >= 9, pred
    iq = _random_s16(sum(sizes), 89)
    parts = _host_fed(eng, iq, sizes, b.MFM_E_BUSY)
    st = eng.stats()
    ref, _ = _oracle(ora, eng, nch, iq, D)
    eng.close()
    _assert_counts(st, pred)
    assert st["submits"] == len(sizes) and st["pending_samples"] == 0
    assert [p[1].shape[1] for p in parts] == [p[0] for p in pred if p[0]]
    _assert_exact(np.concatenate([p[1] for p in parts], axis=1), ref, "three buffers, gathered")


# ------------------------------------------------------------------------------------------------ 9. reset / seek

@pytest.mark.parametrize("how", ["reset", "seek"])
@pytest.mark.parametrize("D,T,k_steps", [(40, 128, 4), (25, 128, 6)], ids=["crow", "pad25"])
def test_reset_and_seek_with_a_head_in_the_ring(pkg, ora, D, T, k_steps, how):
    """Three alternating blocks, then reset() or seek(2^32 + 12345) while the third block's carry is in the ring, then four
    more: the stream that follows is exact from its first output (the oracle stepped there with skip_outputs)."""
    b = pkg.binding
    nch = 64
    _, st = _q14_engine(pkg, ora, D, T, nch, 1 << 16, b.MFM_F_DEVICE_ONLY, commit=False)
    rule = _rule(st, nch)
    sizes = _seam_sizes(rule, D, T)[:4]
    eng, st = _q14_engine(pkg, ora, D, T, nch, sizes[0], b.MFM_F_DEVICE_ONLY)
    _form(st, k_steps)
    iq = _random_s16(sum(sizes), 31 * D)
    first = _Dev(eng, nch, D, T)
    _feed_s16(first, iq[:sum(sizes[:3])], sizes[:3])
    pcm, _ = first.result()
    ref, _ = _oracle(ora, eng, nch, iq[:sum(sizes[:3])], D)
    _assert_exact(pcm, ref, f"before {how}, D {D}")
    assert eng.stats()["overlapped_launches"] == 3
    before = 0 if how == "reset" else (1 << 32) + 12345
    eng.reset() if how == "reset" else eng.seek(before)
    second = _Dev(eng, nch, D, T, before=before)
    _feed_s16(second, iq, sizes)
    pcm, _ = second.result()
    st = eng.stats()
    ref2, _ = _oracle(ora, eng, nch, iq, D, before=before)
    eng.close()
    pred = _predict([(n, False) for n in sizes], D, T, rule)
    assert all(p[1] for p in pred) and len(pred) == 4 and st["overlapped_launches"] == 7 and st["launches"] == 7 and st["pinned"] == 0
    assert st["outputs"] == before + sum(p[0] for p in pred)
    _assert_exact(pcm, ref2, f"after {how}, D {D}")
    if how == "reset":
        assert np.array_equal(ref2[:, :ref.shape[1]], ref)
