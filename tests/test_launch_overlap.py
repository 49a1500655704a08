"""Consecutive launches on two compute streams with an early carry (include/multifm_hip.h: mfm_engine_stream, MFM_F_OVERLAP).

The headline's geometry kept small: 2.4 MS/s, decimation 96, the 128-tap low-pass, 64 channels, blocks of 2^22 samples -
683 tiles on 512 workgroup slots, so a launch fills the slots more than once and the engine alternates (2^21 would give 341
tiles and would not).  A launch that alternates leaves the next launch's [last consumed row | unconsumed tail] in the engine's
carry ring, and the next launch's first workgroup reads it from there sample by sample.

Everything is compared bit-exact with the oracle, never with the engine itself: four channels spread over the rows in full,
and for every channel the first and last 2048 outputs of each block.  One random stream and one oracle run serve every test
(the output stream does not depend on the blocking, so each test feeds a prefix of that stream cut its own way)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 1 << 22
NCH = 64
FULL = (0, 21, 42, 63)      # channels compared over the whole stream
EDGE = 2048                 # outputs compared at each end of every block, on every channel
SEAMS = [BLOCK - d for d in (0, 1, 2, 3, 5, 96, 97, 191)]   # the carried length takes every residue mod 4
INOUT = [BLOCK, BLOCK, 1 << 15, BLOCK, 1 << 12, BLOCK]      # the small ones are under a tile per slot: one stream
H2D, D2H, D2D = 1, 2, 3

_cache = {}


def _hip():
    if "hip" not in _cache:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _cache["hip"] = hip
    return _cache["hip"]


def _stream(kind):
    """the test stream: sum(SEAMS) random samples, as int16 pairs or as RTL-SDR bytes"""
    if ("iq", kind) not in _cache:
        rng = np.random.default_rng(20 if kind == "s16" else 21)
        n = sum(SEAMS)
        if kind == "s16":
            _cache["iq", kind] = (rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16), None)
        else:
            raw = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
            _cache["iq", kind] = (None, raw)
    return _cache["iq", kind]


def _engine(pkg, flags, block=BLOCK, **kw):
    fs, decim, taps, offs, gains = pkg.synth.plan("cfg2_64ch", nr_channels=NCH)
    assert (fs, decim, len(taps)) == (2400000, 96, 128)
    eng = pkg.Engine(fs, decim, block, device=0, flags=flags, **kw)
    for o, g in zip(offs, gains):
        eng.add_channel(int(o), taps, float(g))
    eng.commit()
    if "tables" not in _cache:
        _cache["tables"] = [eng.get_channel(c) for c in range(NCH)]
    return eng


class _Ref:
    """the oracle on the test stream from output `before` on: FULL channels whole, any channel by windows"""

    def __init__(self, ora, pkg, kind, before=0):
        s16, raw = _stream(kind)
        self.ora, self.before = ora, before
        self.iq = s16 if raw is None else ora.unpack_bytes(raw, pkg.binding.MFM_IN_RTLSDR_U8).reshape(-1, 2)
        self.full = {}

    def channel(self, c, nout):
        """outputs [0, nout) of channel c"""
        if c not in self.full or self.full[c].size < nout:
            cre, cim, incr = _cache["tables"][c]
            ch = self.ora.Channel(cre, cim, 96, incr)
            ch.skip_outputs(self.before)
            self.full[c] = ch.feed(self.iq[: (nout - 1) * 96 + 128])[0]
            ch.close()
        return self.full[c][:nout]

    def window(self, c, lo, hi):
        """outputs [lo, hi) of channel c, lo >= 1"""
        cre, cim, incr = _cache["tables"][c]
        return self.ora.window_pcm(self.iq, cre, cim, 96, incr, self.before, lo, hi - lo)


def _ref(ora, pkg, kind="s16", before=0):
    if ("ref", kind, before) not in _cache:
        _cache["ref", kind, before] = _Ref(ora, pkg, kind, before)
    return _cache["ref", kind, before]


class _Feed:
    """Blocks of the test stream through acquire_input / submit on device-resident data, two launches in flight: the PCM of
    a pair of blocks is read back from the two output slots after the second has been submitted."""

    def __init__(self, eng, kind="s16", fmt=None, before=0):
        self.eng, self.hip, self.fmt = eng, _hip(), fmt
        s16, raw = _stream(kind)
        self.src = s16 if raw is None else raw
        self.pos, self.outs, self.pending = 0, [], []
        self.tail, self.produced = 0, before  # the engine's bookkeeping, restated (stats() may wait for the device)

    def put(self, n, then=None):
        """default producer: a synchronous copy into the acquired buffer.  then: called right behind the submit"""
        ptr, cap = self.eng.acquire_input() if self.fmt is None else self.eng.acquire_input_bytes(self.fmt)
        assert cap >= n
        blk = self.src[self.pos:self.pos + n]
        assert self.hip.hipMemcpy(ptr, blk.ctypes.data, blk.nbytes, H2D) == 0
        self.eng.submit(n, producer_stream=0, wait_producer=False)
        if then:
            then()
        self.submitted(n)

    def submitted(self, n):
        self.pos += n
        avail = self.tail + n
        want = (avail - 128) // 96 + 1 if avail >= 128 else 0
        self.tail = avail - want * 96
        if want:
            dptr, stride, nout, _ = self.eng.last_output_device()
            assert nout == want
            self.pending.append((dptr, nout, stride, self.produced))
            self.produced += nout
        if len(self.pending) == 2:
            self.collect()

    def collect(self):
        self.eng.sync()
        for dptr, nout, stride, first in self.pending:
            pcm = np.empty((NCH, stride), np.int16)
            assert self.hip.hipMemcpy(pcm.ctypes.data, dptr, pcm.nbytes, D2H) == 0
            self.outs.append((first, pcm[:, :nout].copy()))
        self.pending = []

    def check(self, ref, base=0):
        """every block collected so far against the oracle; base: the stream's output count at the start of this feed"""
        self.collect()
        assert self.outs
        for first, pcm in self.outs:
            lo, n = first - base, pcm.shape[1]
            for c in FULL:
                want = ref.channel(c, lo + n)[lo:lo + n]
                assert np.array_equal(pcm[c], want), (c, first, int(np.argmax(pcm[c] != want)))
            wins = sorted(set([(max(lo, 1), min(lo + EDGE, lo + n)), (max(lo + n - EDGE, lo, 1), lo + n)]))
            for c in range(NCH):
                for a, z in wins:
                    if z > a:
                        want = ref.window(c, a, z)
                        assert np.array_equal(pcm[c, a - lo:z - lo], want), (c, first, a, int(np.argmax(pcm[c, a - lo:z - lo] != want)))
        last = self.outs[-1]
        return last[0] + last[1].shape[1]


def test_seam_at_every_alignment(pkg, ora):
    """Eight device-resident blocks of 2^22 - {0, 1, 2, 3, 5, 96, 97, 191} samples, default flags: the carried length takes every
    residue mod 4, the seam between ring and buffer falls inside, at the start of and at the end of a 16-byte chunk."""
    b = pkg.binding
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY)
    f = _Feed(eng)
    carried = set()
    for n in SEAMS:
        f.put(n)
        carried.add((96 + f.tail) % 4)
    total = f.check(_ref(ora, pkg))
    st = eng.stats()
    eng.close()
    assert carried == {0, 1, 2, 3}
    assert total == st["outputs"] == (sum(SEAMS) - 128) // 96 + 1
    assert st["launches"] == 8 and st["overlapped_launches"] >= 6 and st["pinned"] == 0


@pytest.mark.parametrize("timing", [False, True])
def test_into_and_out_of_the_path(pkg, ora, timing):
    """Blocks of 2^22, 2^22, 2^15, 2^22, 2^12, 2^22 samples: the small ones run on one stream with the carry in the kernel, and
    take their own [hist | tail] out of the ring first.  Exact across both transitions, with and without sparse timing."""
    b = pkg.binding
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY | ((b.MFM_F_TIMING | b.MFM_F_TIMING_SPARSE) if timing else 0))
    f = _Feed(eng)
    for n in INOUT:
        f.put(n)
    f.check(_ref(ora, pkg))
    st = eng.stats()
    eng.close()
    assert st["launches"] == 6 and st["overlapped_launches"] == 4
    if timing:
        assert st["timed_launches"] == 2 and st["kernel_ms"] > 0  # launches 0 and 4 of 6


@pytest.mark.parametrize("when", ["before_first_submit", "after_third_block", "overlap_flag"])
def test_pinning(pkg, ora, when):
    """mfm_engine_stream() pins: asked before the first submit no launch overlaps; asked after the third block the later
    launches all go to the returned stream, and a consumer enqueued there sees the finished PCM; MFM_F_OVERLAP alternates
    regardless."""
    b = pkg.binding
    hip = _hip()
    import torch
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY | (b.MFM_F_OVERLAP if when == "overlap_flag" else 0))
    f = _Feed(eng)
    s = eng.stream if when != "after_third_block" else None
    copies, seen = [], set()
    spare = [torch.empty(NCH * (BLOCK // 96 + 4096), dtype=torch.int16, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    def consumer():
        # a copy queued behind the launch on the engine's stream, no host synchronisation in between
        dptr, st_, nout, _ = eng.last_output_device()
        assert NCH * st_ <= spare[0].numel()
        t = spare[len(copies)]
        assert hip.hipMemcpyAsync(t.data_ptr(), dptr, NCH * st_ * 2, D2D, s) == 0
        copies.append((t, st_, nout, f.produced))

    for k, n in enumerate(SEAMS[:6]):
        if when == "after_third_block" and k == 3:
            s = eng.stream
            assert eng.stats()["overlapped_launches"] == 3
        f.put(n, then=consumer if when == "after_third_block" and k >= 3 else None)
        if s is not None:
            seen.add(eng.stream)
    f.check(_ref(ora, pkg))
    st = eng.stats()
    eng.close()
    assert st["launches"] == 6
    if when == "before_first_submit":
        assert st["overlapped_launches"] == 0 and st["pinned"] == 1 and seen == {s}
    elif when == "after_third_block":
        assert st["overlapped_launches"] == 3 and st["pinned"] == 1 and seen == {s}
        torch.cuda.synchronize()
        ref = _ref(ora, pkg)
        assert len(copies) == 3
        for t, st_, nout, first in copies:
            got = t.cpu().numpy().reshape(-1)[: NCH * st_].reshape(NCH, st_)[:, :nout]
            for c in FULL:
                assert np.array_equal(got[c], ref.channel(c, first + nout)[first:first + nout]), (c, first)
    else:
        assert st["overlapped_launches"] == 6 and st["pinned"] == 0 and len(seen) == 2


def test_producer_ordering(pkg, ora):
    """The natural flow: every block is written into the acquired buffer by an asynchronous copy on a torch stream, without a
    host synchronisation, and submitted with wait_producer; the next acquire_input() is followed at once by the next
    overwrite.  The carry's copy must come behind the producer, the producer behind the launch and the copy that read the
    buffer before.  Ten blocks."""
    import torch
    b = pkg.binding
    lib = pkg.load_library()
    in_bytes = lib.mfm_engine_input_bytes(BLOCK, 128)
    bufs = [torch.empty(in_bytes // 2, dtype=torch.int16, device="cuda") for _ in range(2)]
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY, ext_input=(bufs[0].data_ptr(), bufs[1].data_ptr()))
    f = _Feed(eng)
    if "pinned" not in _cache:
        _cache["pinned"] = torch.from_numpy(f.src.reshape(-1)).pin_memory()
    host = _cache["pinned"]
    ps = torch.cuda.Stream()
    n = 3300003  # 538 tiles: still more than the 512 slots
    for _ in range(10):
        ptr, cap = eng.acquire_input()
        assert cap >= n
        which = 0 if bufs[0].data_ptr() <= ptr < bufs[0].data_ptr() + in_bytes else 1
        off = (ptr - bufs[which].data_ptr()) // 2
        with torch.cuda.stream(ps):
            bufs[which][off:off + 2 * n].copy_(host[2 * f.pos:2 * (f.pos + n)], non_blocking=True)
        eng.submit(n, producer_stream=ps.cuda_stream, wait_producer=True)
        f.submitted(n)
    f.check(_ref(ora, pkg))
    st = eng.stats()
    eng.close()
    assert st["launches"] == 10 and st["overlapped_launches"] == 10


@pytest.mark.parametrize("how", ["reset", "seek"])
def test_reset_and_seek_mid_stream(pkg, ora, how):
    """reset() and seek() (to an output count beyond 2^32) in the middle of an alternating stream, a head still in the ring:
    the stream that follows is exact from its first output."""
    b = pkg.binding
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY)
    f = _Feed(eng)
    for n in SEAMS[:3]:
        f.put(n)
    f.check(_ref(ora, pkg))
    before = 0 if how == "reset" else (1 << 32) + 12345
    eng.reset() if how == "reset" else eng.seek(before)
    g = _Feed(eng, before=before)
    for n in SEAMS[:4]:
        g.put(n)
    total = g.check(_ref(ora, pkg, before=before), base=before)
    st = eng.stats()
    eng.close()
    assert total == st["outputs"] == before + (sum(SEAMS[:4]) - 128) // 96 + 1
    assert st["overlapped_launches"] == 7


def test_last_launch_input_after_an_overlapped_launch(pkg, ora):
    """mfm_engine_last_launch_input() promises [carried tail | block] contiguous at the returned address, also when the launch
    took its head from the ring."""
    b = pkg.binding
    hip = _hip()
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY)
    f = _Feed(eng)
    for n in SEAMS[:3]:
        f.put(n)
    iptr, n_in, fmt = eng.last_launch_input()
    got = np.empty((n_in, 2), np.int16)
    assert hip.hipMemcpy(got.ctypes.data, iptr, got.nbytes, D2H) == 0
    f.check(_ref(ora, pkg))
    st = eng.stats()
    eng.close()
    end = sum(SEAMS[:3])
    assert fmt == 0 and st["overlapped_launches"] == 3 and n_in > SEAMS[2]
    assert np.array_equal(got, f.src[end - n_in:end])


def test_8bit_blocks_keep_one_stream(pkg, ora):
    """RTL-SDR bytes through acquire_input_bytes, the block sizes of the seam test: exact, and no launch overlaps - the path
    is for int16 blocks."""
    b = pkg.binding
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY)
    f = _Feed(eng, kind="u8", fmt=b.MFM_IN_RTLSDR_U8)
    for n in SEAMS:
        f.put(n)
    f.check(_ref(ora, pkg, kind="u8"))
    st = eng.stats()
    eng.close()
    assert st["launches"] == st["launches_8bit"] == 8 and st["overlapped_launches"] == 0


def test_timing_by_the_kernels_own_stamps(pkg, ora):
    """MFM_F_TIMING on an alternating engine: no event pairs; launch_ms() of the last k launches is launch_cycles()'s 100 MHz
    reference ticks / 1e5 for the same launches, and kernel_ms their sum."""
    b = pkg.binding
    eng = _engine(pkg, b.MFM_F_DEVICE_ONLY | b.MFM_F_TIMING)
    f = _Feed(eng)
    for n in SEAMS[:6]:
        f.put(n)
    f.check(_ref(ora, pkg))
    st = eng.stats()
    ms = eng.launch_ms(6)
    _, ref_ticks = eng.launch_cycles(6)
    eng.close()
    assert st["overlapped_launches"] == 6 and st["timed_launches"] == 6 and ms.size == 6 and ref_ticks.size == 6
    assert (ref_ticks > 0).all()
    assert np.array_equal(ms, (ref_ticks.astype(np.float64) / 1e5).astype(np.float32))
    assert st["kernel_ms"] == float(ms.astype(np.float64).sum())
    # a 2^22-sample launch of this geometry takes 7-9 us of matrix work per tile round: between 5 us and 5 ms whatever the clock
    assert 0.005 < ms.min() and ms.max() < 5.0
