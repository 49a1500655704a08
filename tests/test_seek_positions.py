"""Stream positions above 2^32 in the stages that report them, through their seek entries (mfm_pocsag_seek, mfm_flex_seek,
mfm_ais_seek, mfm_level_seek, mfm_gate_seek): a seeked object is a fresh one whose next sample has index `samples_before`.

Every expected value is the reference's that the stage's own test file uses - ora.Pocsag().feed with test_pocsag._dedupe,
ora.Flex().feed as in test_flex._check_channel, tests/ais_ref.py, test_level.restate, test_gate.restate_call /
test_gate_preroll.restate_pre - run ONCE on the short stream from position 0; the base is added here (to `sample`,
`sync_sample` of a FRAME, `start_sample`; base / W to `window` and `first_window`).  Every comparison is the exact one of
those files.

Bases per stage: 0 and 53 000 (controls), 2^33 + 12345 and 2^40 + 1, and 2^32 - d with d read off the reference's event
list, so that 2^32 falls between a match and its event, on / one before / one behind an event's sample, and into the idle
search between two transmissions.  For the level and gate stages a base is a multiple of W (so d = 2^32 mod W plus whole
windows: W = 100 is the case where a window straddles 2^32, and no d is odd there by construction); 2^32 is put into a
window that opens a channel, one inside an open stretch and one that closes a channel.  Each base runs as one call and as a ragged list of calls
that has calls ending at absolute 2^32 - 1, 2^32 and 2^32 + 1.  The guards (no GPU) assert, on the reference's list alone,
that every 2^32 - d case has events on both sides and that the straddling event straddles; a GPU case asserts its guard
first.  Every GPU case feeds the object another stream with a transmission in it before it seeks.

Behind them, window numbers above 2^32 through the burst chain (gate -> burst resampler -> burst POCSAG, AIS, FLEX): the host
twins at pos = base, and on the device behind a seeked level stage and gate, against the oracle per stretch.  Stretch-relative
positions above 2^32 in the burst stages are test_burst_positions.py's, through the stages' state entries."""
import numpy as np
import pytest

import ais_ref
import test_ais as ta
import test_flex as tf
import test_gate as tg
import test_gate_preroll as tgp
import test_level as tl
import test_pocsag as tp
import test_runais as tra
import test_runflex as trf
import test_runpocsag as trp
import test_runrs as tr

T32 = 1 << 32
FIXED = {"zero": 0, "control": 53000, "2^33": (1 << 33) + 12345, "2^40": (1 << 40) + 1}
DERIVED = ["straddle", "on", "before", "after", "idle"]
PLACES = list(FIXED) + DERIVED
CUTS = ["one", "ragged"]
FRAME = 1
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ragged(n, marks, biggest, seed):
    """piece lengths that add up to n: a call of no sample, seeded ends, an end at every mark inside the stream, no piece
    above `biggest`"""
    rng = np.random.RandomState(seed)
    ends = sorted({int(x) for x in rng.randint(1, n, 12)} | {int(m) for m in marks if 0 < m < n} | {n})
    out, pos = [0], 0
    for e in ends:
        while e - pos > biggest:
            out.append(biggest)
            pos += biggest
        out.append(e - pos)
        pos = e
    assert sum(out) == n and max(out) <= biggest
    return out


def cuts_of(kind, n, d, biggest, seed):
    if kind == "one":
        return [n]
    cuts = ragged(n, (d - 1, d, d + 1), biggest, seed)
    if 1 < d < n - 1:
        ends = np.cumsum(cuts).tolist()
        assert d - 1 in ends and d in ends and d + 1 in ends
    return cuts


# ---- the three decoders: scenes and what the reference says about them -----------------------------------------------

def _pocsag_scene(pkg, ora):
    """five channels of 100 000 samples at 38 400 Hz: 0: 1200 baud, two clean transmissions with noise between them; 1: 512
    baud, two batches with single, double and one uncorrectable triple error; 2: 2400 baud in heavy noise, three times;
    3: noise; 4: a transmission that starts at sample 0.  And another stream that ends inside a batch, for the object to forget"""
    sy = pkg.synth
    n = 100000
    rng = np.random.RandomState(41)
    msgs = tp._messages(sy)
    one = sy.pocsag_bits(sy.pocsag_batches(msgs[:1]))
    two = sy.pocsag_bits(sy.pocsag_batches(msgs[:2]), preamble_bits=128)
    assert one.size == 576 + 544 and two.size == 128 + 2 * 544

    def place(parts):
        x = np.concatenate(parts)
        assert x.size <= n, x.size
        return np.concatenate([x, rng.normal(0, 900, n - x.size).round().astype(np.int16)])

    first = 128 + 32
    flips = [first + 32 * 1 + 4, first + 32 * 6 + 2, first + 32 * 6 + 29, first + 32 * 7 + 11] + \
        [first + 32 * 9 + b for b in tp._uncorrectable_triple(ora, two, first + 32 * 9)]
    pcm = np.stack([
        place([sy.pocsag_pcm(one, 1200, noise=700, lead=4000, trail=8000, seed=1), sy.pocsag_pcm(one, 1200, noise=700, lead=100, seed=2)]),
        place([sy.pocsag_pcm(two, 512, noise=500, lead=2000, seed=3, flip=flips)]),
        place([sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches(msgs[:2])), 2400, amplitude=6000, noise=3000, lead=900 + 700 * k, trail=3000,
                             seed=10 + k) for k in range(3)]),
        rng.normal(0, 2000, n).round().astype(np.int16),
        place([sy.pocsag_pcm(one, 1200, noise=300, lead=0, seed=20)]),
    ])
    want = [tp._dedupe(ora.Pocsag().feed(row)[0], ora) for row in pcm]
    pre = sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches(msgs[:1]), preamble_bits=64), 2400, noise=300, lead=500, seed=5)[:6000]
    pre = np.stack([pre] * 2 + [rng.normal(0, 2000, pre.size).round().astype(np.int16)] * 3)
    # where 2^32 goes
    F, B, L = ora.EV_SYNC_FOUND, ora.EV_BATCH, ora.EV_SYNC_LOST
    t1, s1 = want[1]["type"].tolist(), want[1]["sample"].tolist()
    assert t1[:2] == [F, B] and (want[1]["type"] == B).sum() == 2 and (want[1]["fail_mask"] != 0).any()
    t0, s0 = want[0]["type"].tolist(), want[0]["sample"].tolist()
    assert t0.count(F) == 2 and t0.count(L) == 2 and t0.index(L) < len(t0) - 1 and t0[t0.index(L) + 1] == F
    assert int(want[4]["sample"][0]) < 32 * 700 and len(want[2]) >= 6 and len(want[3]) == 0
    e = int(s0[t0.index(B)])
    lost, found = int(s0[t0.index(L)]), int(s0[t0.index(L) + 1])
    d = dict(straddle=(int(s1[0]) + int(s1[1])) // 2 + 1, on=e, before=e - 1, after=e + 1, idle=(lost + found) // 2)
    return dict(pcm=pcm, want=want, pre=pre, d=d, straddles=(int(s1[0]), int(s1[1])), idle=(lost, found), on=e, fields=("sample",))


def _flex_scene(pkg, ora):
    """four channels at 16 000 Hz, one per coding, two frames each with 2000 idle samples between them; the last one behind
    the sync part of a frame with a damaged A word (a BAD_BAUD event, whose sync_sample is 0 at any base)"""
    sy = pkg.synth
    rng = np.random.RandomState(42)
    bad = sy.flex_pcm([sy.flex_frame_levels(1, 1, 3, {}, a_flip=0x0F0F0000)], lead=50, noise=200, seed=5)[:3000]
    chans = [sy.flex_pcm(tf._frames(sy, 0, 2), lead=333, trail=900, noise=300, seed=1, gap=2000),
             sy.flex_pcm(tf._frames(sy, 1, 2), lead=1, trail=900, noise=1500, seed=2, gap=2000),
             sy.flex_pcm(tf._frames(sy, 2, 2), lead=4099, trail=900, noise=500, seed=3, offset=700, gap=2000),
             np.concatenate([bad, sy.flex_pcm(tf._frames(sy, 3, 2), lead=77, trail=900, noise=500, seed=4, offset=-400, amplitude=5000, gap=2000)])]
    n = max(len(c) for c in chans)
    pcm = np.stack([np.concatenate([c, rng.randint(-300, 300, n - len(c)).astype(np.int16)]) for c in chans])
    assert n <= 72000
    want = [ora.Flex().feed(row)[0] for row in pcm]
    pre = sy.flex_pcm(tf._frames(sy, 0, 1), lead=100, noise=300, seed=9)[:6000]   # ends inside the frame's block
    pre = np.stack([pre] * 4)
    for c in range(4):
        fr = want[c][want[c]["type"] == FRAME]
        assert len(fr) == 2 and set(fr["coding"].tolist()) == {c}, c
    assert [int(t) for t in want[3]["type"]] == [2, FRAME, FRAME] and int(want[3]["sync_sample"][0]) == 0
    f0, f1, f2 = want[0][0], want[1][0], want[2][want[2]["type"] == FRAME]
    e = int(f1["sample"])
    idle = (int(f2["sample"][0]), int(f2["sync_sample"][1]))
    assert idle[1] - idle[0] > 2000
    d = dict(straddle=(int(f0["sync_sample"]) + int(f0["sample"])) // 2, on=e, before=e - 1, after=e + 1, idle=idle[0] + 1001)
    return dict(pcm=pcm, want=want, pre=pre, d=d, straddles=(int(f0["sync_sample"]), int(f0["sample"])), idle=idle, on=e,
                fields=("sample", "sync_sample"))


def _ais_scene(pkg, ora):
    """four busy channels of 30 000 samples at 48 000 Hz (test_ais._busy: all message types, back-to-back packets, CRC rejects,
    a missing end flag)"""
    sy = pkg.synth
    n = 30000
    pcm = np.stack([ta._busy(sy, 60 + c, n, noise=400.0 if c != 1 else 2500.0) for c in range(4)])
    want = [ais_ref.demod(row, c) for c, row in enumerate(pcm)]
    assert all(len(w) >= 8 for w in want) and sum(int((w["fcs_valid"] == 0).sum()) for w in want) >= 1
    pre = np.stack([ta._busy(sy, 70, 4000, flips=False)[:3600]] * 4)
    w0, w1, w2 = want[0], want[1], want[2]
    k = len(w0) // 2
    e = int(w1["sample"][len(w1) // 2])
    gaps = w2["start_sample"][1:].astype(np.int64) - w2["sample"][:-1].astype(np.int64)
    g = int(np.argmax(gaps))
    idle = (int(w2["sample"][g]), int(w2["start_sample"][g + 1]))
    assert idle[1] - idle[0] >= 4
    d = dict(straddle=(int(w0["start_sample"][k]) + int(w0["sample"][k])) // 2, on=e, before=e - 1, after=e + 1,
             idle=(idle[0] + idle[1]) // 2)
    return dict(pcm=pcm, want=want, pre=pre, d=d, straddles=(int(w0["start_sample"][k]), int(w0["sample"][k])), idle=idle, on=e,
                fields=("sample", "start_sample"))


DECODERS = {"pocsag": _pocsag_scene, "flex": _flex_scene, "ais": _ais_scene}
SMALL_IN = {"pocsag": 4096, "flex": 16384, "ais": 2048}   # the ragged cut's max_in_samples: the bit window slides several times


def decoder_scene(pkg, ora, stage):
    return cached(stage, lambda: DECODERS[stage](pkg, ora))


def base_of(sc, place):
    return FIXED[place] if place in FIXED else T32 - sc["d"][place]


def shifted(sc, c, base):
    """the reference's events of channel c at `base`"""
    w = sc["want"][c].copy()
    for f in sc["fields"]:
        add = np.where(w["type"] == FRAME, base, 0) if f == "sync_sample" else base   # sync_sample is 0 in every other event
        w[f] = (w[f].astype(np.uint64) + np.asarray(add).astype(np.uint64)).astype(w[f].dtype)
    return w


def guard_decoder(sc, place):
    """on the reference's events alone: where they lie around absolute 2^32 at this base"""
    base = base_of(sc, place)
    n = sc["pcm"].shape[1]
    at = np.concatenate([shifted(sc, c, base)["sample"] for c in range(len(sc["want"]))]).astype(np.uint64)
    assert at.size and int(at.min()) >= base and int(at.max()) < base + n
    if place in ("zero", "control"):
        assert int(at.max()) < T32
        return base
    if place in FIXED:
        assert int(at.min()) >= T32
        return base
    d = sc["d"][place]
    assert 1 < d < n - 1 and base + d == T32
    assert (at < T32).any() and (at >= T32).any(), (place, d)
    lo, hi = sc["straddles"]
    if place == "straddle":
        assert base + lo < T32 <= base + hi, (lo, hi, d)
    if place in ("on", "before", "after"):
        assert base + sc["on"] == T32 + {"on": 0, "before": 1, "after": -1}[place]
    if place == "idle":
        assert base + sc["idle"][0] < T32 < base + sc["idle"][1]
    return base


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("stage", list(DECODERS))
def test_reference_events_lie_on_both_sides_of_2_to_the_32(pkg, ora, stage, place):
    sc = decoder_scene(pkg, ora, stage)
    guard_decoder(sc, place)
    assert any(sc["d"][p] % 2 for p in DERIVED)   # no alignment of the stage (groups of 2048, words of 32, rings) meets 2^32
    for kind in CUTS:
        biggest = sc["pcm"].shape[1] if kind == "one" else SMALL_IN[stage]
        cuts_of(kind, sc["pcm"].shape[1], sc["d"].get(place, 0), biggest, 7)


def _feed(st, rows, biggest, collect):
    pos = 0
    while pos < rows.shape[1]:
        m = min(biggest, rows.shape[1] - pos)
        collect(st.process_host(rows[:, pos:pos + m]))
        pos += m


def _run_pocsag(pkg, ora, sc, base, cuts, biggest):
    nch = sc["pcm"].shape[0]
    st = pkg.Pocsag(nch, biggest)
    seen = []
    _feed(st, sc["pre"], biggest, seen.append)
    seen = np.concatenate(seen)
    assert (seen["type"] == ora.EV_SYNC_FOUND).any() and not (seen["type"] == ora.EV_BATCH).any()   # it forgets a batch half collected
    if base is not None:
        st.seek(base)
        assert st.fetch_events().size == 0
    got, pos = [], 0
    for m in cuts:
        got.append(st.process_host(sc["pcm"][:, pos:pos + m]))
        pos += m
    st.close()
    got = np.concatenate(got)
    return [got[got["channel"] == c] for c in range(nch)]


def _run_ais(pkg, ora, sc, base, cuts, biggest):
    nch = sc["pcm"].shape[0]
    st = pkg.Ais(nch, biggest)
    seen = []
    _feed(st, sc["pre"], biggest, seen.append)
    assert np.concatenate(seen).size >= 1
    if base is not None:
        st.seek(base)
        assert st.fetch_events().size == 0
    got, pos = [], 0
    for m in cuts:
        got.append(st.process_host(sc["pcm"][:, pos:pos + m]))
        pos += m
    st.close()
    got = np.concatenate(got)
    return [got[got["channel"] == c] for c in range(nch)]


def _run_flex(pkg, ora, sc, base, cuts, biggest):
    """per channel (events with frame_index into the second part, frame words)"""
    nch = sc["pcm"].shape[0]
    st = pkg.binding.Flex(nch, biggest)
    _feed(st, sc["pre"], biggest, lambda r: None)   # sync 1 and the FIW are through, the block is not: state FRAME
    if base is not None:
        st.seek(base)
        ev, fw = st.fetch_events()
        assert ev.size == 0 and fw.size == 0
    evs, words, pos = [[] for _ in range(nch)], [], 0
    for m in cuts:
        ev, fw = st.process_host(sc["pcm"][:, pos:pos + m])
        for e in ev:
            e = e.copy()
            if int(e["type"]) == FRAME:
                words.append(fw[int(e["frame_index"])])
                e["frame_index"] = len(words) - 1
            evs[int(e["channel"])].append(e)
        pos += m
    st.close()
    b = pkg.binding
    return [(np.array(v, b.FLEX_EVENT_DTYPE), np.array(words, b.FLEX_FRAME_DTYPE)) for v in evs]


def _compare(pkg, ora, stage, sc, got, base, what):
    for c in range(len(sc["want"])):
        want = shifted(sc, c, base)
        tag = f"{what}, channel {c}"
        if stage == "pocsag":
            tp._compare_events(got[c], want, ora, tag)
        elif stage == "ais":
            assert (got[c]["channel"] == c).all(), tag
            ta._same(got[c], want)
        else:
            tf._check_channel(ora, pkg.synth, got[c][0], got[c][1], want, tag)


RUN = {"pocsag": _run_pocsag, "flex": _run_flex, "ais": _run_ais}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("stage", list(DECODERS))
def test_gpu_seeked_decoder_reports_the_references_events_at_the_base(pkg, ora, stage, place, kind):
    """after another stream and a seek: the events of a fresh object, `samples_before` added.  The ragged cut runs with a small
    max_in_samples, so the POCSAG and AIS bit windows slide (pg_begin / ai_begin's new_ws) several times - above 2^32 at
    every base but the controls - and the FLEX ring wraps"""
    sc = decoder_scene(pkg, ora, stage)
    base = guard_decoder(sc, place)
    n = sc["pcm"].shape[1]
    biggest = n if kind == "one" else SMALL_IN[stage]
    cuts = cuts_of(kind, n, sc["d"].get(place, 0), biggest, 7)
    got = RUN[stage](pkg, ora, sc, base, cuts, biggest)
    _compare(pkg, ora, stage, sc, got, base, f"{stage} base {base} ({place}) cut {kind}")


# ---- level and gate -------------------------------------------------------------------------------------------------

WINDOWS = [64, 100, 4096]
NCH, NWIN = 5, 40
LEVEL_PLACES = list(FIXED) + ["opening", "inside", "closing"]
GATE_PLACES = list(FIXED) + ["run_start", "mid"]
GATE_KINDS = [(1, 0, "alternating"), (1, 0, "bernoulli"), (2, 0, "bernoulli"), (1, 3, "bernoulli"), (2, 3, "bernoulli")]   # E, P, mask


def window_base(W, place, k):
    """a multiple of W: the fixed bases rounded down; otherwise the one at which 2^32 lies in relative window k"""
    if place in FIXED:
        return FIXED[place] // W * W
    return (T32 // W - k) * W


def level_scene(pkg, W, form):
    """five channels, 40 windows and a ragged end: noise with bursts that are not aligned to windows; energy squelch with a
    hang of one window"""
    def make():
        rng = np.random.RandomState(W + form)
        n = NWIN * W + W // 2 + 3
        shape = (NCH, n, 2) if form == tl.IQ else (NCH, n)
        x = rng.randint(-100, 101, size=shape).astype(np.int16)
        for c in range(NCH - 1):   # the last channel stays closed
            k = 1 + c
            while k < NWIN - 2:
                ln = int(rng.randint(1, 5))
                a, b = k * W + int(rng.randint(0, W)), (k + ln) * W + int(rng.randint(0, W))
                x[c, a:b] = rng.randint(-32768, 32768, size=x[c, a:b].shape).astype(np.int16)
                k += ln + 2 + int(rng.randint(1, 4))
        e = 2 if form == tl.IQ else 1
        kw = dict(metric=tl.ENERGY, sense=tl.ABOVE, open_thr=W * e * 10 ** 6, close_thr=W * e * 10 ** 5, hang=1)
        want = tl.restate(pkg, x, W, form, **kw)
        op = want["open"].astype(bool)
        rise = np.flatnonzero((op[:, 1:] & ~op[:, :-1]).any(axis=0)) + 1
        stay = np.flatnonzero((op[:, 1:] & op[:, :-1]).any(axis=0)) + 1
        fall = np.flatnonzero((~op[:, 1:] & op[:, :-1]).any(axis=0)) + 1
        mid = lambda a: int(a[np.argmin(np.abs(a - NWIN // 2))])
        pre = rng.randint(-32768, 32768, size=(NCH, 3 * W + W // 2) + shape[2:]).astype(np.int16)
        return dict(x=x, want=want, kw=kw, k=dict(opening=mid(rise), inside=mid(stay), closing=mid(fall)), pre=pre, n=n)
    return cached(("level", W, form), make)


def guard_level(sc, W, place):
    base = window_base(W, place, sc["k"].get(place, 0))
    assert base % W == 0
    op = sc["want"]["open"].astype(bool)
    kabs = sc["want"]["window"][op].astype(np.uint64) + np.uint64(base // W)   # windows of the records that say open
    assert kabs.size
    if place in FIXED:
        assert (int(kabs.max()) + 1) * W <= T32 if place in ("zero", "control") else int(kabs.min()) * W >= T32
        return base, 0
    d = T32 - base
    k = sc["k"][place]
    assert k * W <= d < (k + 1) * W and (d % W != 0) == (W == 100)   # W = 100: the window straddles 2^32
    assert (kabs < T32 // W).any() and (kabs >= T32 // W).any()
    col = op[:, k]
    if place == "opening":
        assert (col & ~op[:, k - 1]).any()
    if place == "inside":
        assert (col & op[:, k - 1]).any()
    if place == "closing":
        assert (~col & op[:, k - 1]).any() and not op[NCH - 1].any()
    return base, d


LEVEL_CASES = [(W, tl.PCM) for W in WINDOWS] + [(100, tl.IQ)]


@pytest.mark.parametrize("place", LEVEL_PLACES)
@pytest.mark.parametrize("W,form", LEVEL_CASES)
def test_reference_records_lie_on_both_sides_of_2_to_the_32(pkg, W, form, place):
    sc = level_scene(pkg, W, form)
    _, d = guard_level(sc, W, place)
    cuts_of("ragged", sc["n"], d, 7 * W + 5, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("place", LEVEL_PLACES)
@pytest.mark.parametrize("W,form", LEVEL_CASES)
def test_gpu_seeked_level_reports_the_restated_records_at_the_base(pkg, W, form, place, kind):
    sc = level_scene(pkg, W, form)
    base, d = guard_level(sc, W, place)
    n = sc["n"]
    biggest = n if kind == "one" else 7 * W + 5
    kw = sc["kw"]
    lv = pkg.Level(NCH, biggest, W, form=form, metric=kw["metric"], sense=kw["sense"], open_thr=kw["open_thr"], close_thr=kw["close_thr"],
                   hang_windows=kw["hang"])
    seen = lv.process_host(sc["pre"])   # every channel open, half a window carried
    assert seen.shape[1] == 3 and seen["open"].all()
    lv.seek(base)
    assert lv.fetch().shape == (NCH, 0)
    parts, pos = [], 0
    for m in cuts_of(kind, n, d, biggest, 3):
        parts.append(lv.process_host(sc["x"][:, pos:pos + m]))
        pos += m
    lv.close()
    want = sc["want"].copy()
    want["window"] += np.uint64(base // W)
    tl.same_records(np.concatenate(parts, axis=1), want, f"level W {W} form {form} base {base} ({place}) cut {kind}")


def gate_scene(pkg, W, E, P, mask_kind):
    def make():
        rng = np.random.RandomState(1000 * E + 10 * W + P)
        n = NWIN * W + W // 2 + 3
        stream = rng.randint(-32768, 32768, size=(NCH, n * E)).astype(np.int16)
        mask = tg.make_mask(mask_kind, rng, NCH, NWIN)
        runs = _gate_want(pkg, dict(stream=stream, mask=mask), W, E, P, [n])[0][0]   # as one call: the emitted stretches
        starts = np.sort(runs["first_window"][runs["first_window"] >= 3].astype(np.int64))
        k = int(starts[np.argmin(np.abs(starts - NWIN // 2))])
        pre = rng.randint(-32768, 32768, size=(NCH, (4 * W + W // 2) * E)).astype(np.int16)
        return dict(stream=stream, mask=mask, n=n, k=dict(run_start=k, mid=NWIN // 2 + 1), pre=pre)
    return cached(("gate", W, E, P, mask_kind), make)


def _gate_want(pkg, sc, W, E, P, cuts):
    """the restated (runs, payload) of every call, and of the flush when P > 0, at base 0"""
    out, pos = [], 0
    for m in cuts:
        out.append(tgp.restate_pre(pkg, sc["stream"], sc["mask"], W, E, P, pos, m) if P else tg.restate_call(pkg, sc["stream"], sc["mask"], W, E, pos, m))
        pos += m
    if P:
        out.append(tgp.restate_pre(pkg, sc["stream"], sc["mask"], W, E, P, pos, 0, flush=True))
    return out


def guard_gate(pkg, sc, W, E, P, place, kind):
    base = window_base(W, place, sc["k"].get(place, 0))
    d = 0 if place in FIXED else T32 - base
    biggest = sc["n"] if kind == "one" else 7 * W + 5
    cuts = cuts_of(kind, sc["n"], d, biggest, 3)
    want = _gate_want(pkg, sc, W, E, P, cuts)
    first = np.concatenate([r["first_window"] for r, _ in want]).astype(np.uint64) + np.uint64(base // W)
    assert first.size
    if place in FIXED:
        assert int(first.max()) * W < T32 if place in ("zero", "control") else int(first.min()) * W >= T32
    else:
        assert (first < T32 // W).any() and (first >= T32 // W).any(), (place, kind)
        assert (d % W != 0) == (W == 100)
        if place == "run_start":
            assert (first == T32 // W).any()
    return base, cuts, biggest, want


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("place", GATE_PLACES)
@pytest.mark.parametrize("E,P,mask_kind", GATE_KINDS)
@pytest.mark.parametrize("W", WINDOWS)
def test_reference_runs_lie_on_both_sides_of_2_to_the_32(pkg, W, E, P, mask_kind, place, kind):
    guard_gate(pkg, gate_scene(pkg, W, E, P, mask_kind), W, E, P, place, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("place", GATE_PLACES)
@pytest.mark.parametrize("E,P,mask_kind", GATE_KINDS)
@pytest.mark.parametrize("W", WINDOWS)
def test_gpu_seeked_gate_reports_the_restated_runs_at_the_base(pkg, W, E, P, mask_kind, place, kind):
    """the records carry the window numbers a seeked level stage writes; with P = 3 the gate has a history and, in the ragged
    cut, a flush to forget, and emits no window in front of the base"""
    sc = gate_scene(pkg, W, E, P, mask_kind)
    base, cuts, biggest, want = guard_gate(pkg, sc, W, E, P, place, kind)
    gate = pkg.Gate(NCH, max(biggest, sc["pre"].shape[1] // E), W, elems_per_sample=E, preroll_windows=P)
    runs, _ = gate.process_host(sc["pre"], tg.records_of(pkg, np.ones((NCH, 4), bool), 0, 4))
    assert len(runs) == (NCH if P < 4 else 0)
    if P and kind == "ragged":
        gate.flush_device()
        assert len(gate.fetch()[0]) == NCH
    gate.seek(base)
    assert len(gate.fetch()[0]) == 0
    pos = 0
    for i, m in enumerate(cuts):
        rec = tg.records_of(pkg, sc["mask"], pos // W, (pos + m) // W)
        rec["window"] += np.uint64(base // W)
        got = gate.process_host(sc["stream"][:, pos * E:(pos + m) * E], rec)
        wr = want[i][0].copy()
        wr["first_window"] += np.uint64(base // W)
        tg.same(got, (wr, want[i][1]), f"gate W {W} E {E} P {P} {mask_kind} base {base} ({place}) cut {kind}, call {i} at {pos}")
        pos += m
    if P:
        gate.flush_device()
        wr = want[-1][0].copy()
        wr["first_window"] += np.uint64(base // W)
        tg.same(gate.fetch(), (wr, want[-1][1]), f"gate W {W} E {E} P {P} base {base} ({place}) cut {kind}, flush")
    gate.close()


# ---- refusals -------------------------------------------------------------------------------------------------------

def _refused(pkg, fn, *needles):
    with pytest.raises(pkg.MfmError) as ei:
        fn()
    assert ei.value.code == pkg.binding.MFM_E_INVAL
    for s in needles:
        assert s in str(ei.value), str(ei.value)


@pytest.mark.gpu
def test_gpu_refused_seeks_say_why_and_leave_the_stream_as_it_was(pkg, ora):
    """no object, samples_before >= 2^62, and for level and gate a position inside a window: MFM_E_INVAL with a message, and the
    object goes on with its stream exactly as one that never saw the call"""
    b = pkg.binding
    lib = pkg.load_library()
    for name in ("pocsag", "flex", "ais", "level", "gate"):
        assert getattr(lib, f"mfm_{name}_seek")(None, 0) == b.MFM_E_INVAL
        assert f"mfm_{name}_seek: no object" in lib.mfm_last_error().decode()
    # the decoders: half the stream, the refused call on one of two objects, the other half
    for stage in DECODERS:
        sc = decoder_scene(pkg, ora, stage)
        n = sc["pcm"].shape[1]
        make = {"pocsag": lambda: pkg.Pocsag(5, n), "flex": lambda: b.Flex(4, n), "ais": lambda: pkg.Ais(4, n)}[stage]
        out = []
        for refuse in (True, False):
            st = make()
            first = st.process_host(sc["pcm"][:, :n // 2])
            if refuse:
                _refused(pkg, lambda: st.seek(1 << 62), f"mfm_{stage}_seek", "2^62")
                _refused(pkg, lambda: st.seek((1 << 64) - 1), "2^62")
                again = st.fetch_events()   # the last call's result is still there
                assert all(np.array_equal(a, f) for a, f in zip(again, first)) if stage == "flex" else np.array_equal(again, first)
            out.append((first, st.process_host(sc["pcm"][:, n // 2:])))
            st.close()
        flat = lambda r: [x.tobytes() for part in r for x in (part if isinstance(part, tuple) else (part,))]
        assert flat(out[0]) == flat(out[1]), stage
        assert sum(len(p[0]) if isinstance(p, tuple) else len(p) for p in out[0]) == sum(len(w) for w in sc["want"])
    # level and gate
    W = 100
    lsc = level_scene(pkg, W, tl.PCM)
    kw = lsc["kw"]
    n = lsc["n"]
    half = 17 * W + 30   # inside a window
    recs = []
    for refuse in (True, False):
        lv = pkg.Level(NCH, n, W, open_thr=kw["open_thr"], close_thr=kw["close_thr"], hang_windows=kw["hang"])
        a = lv.process_host(lsc["x"][:, :half])
        if refuse:
            _refused(pkg, lambda: lv.seek(1 << 62), "mfm_level_seek", "2^62")
            _refused(pkg, lambda: lv.seek(T32 + 1), "mfm_level_seek", "multiple of window_samples")
            _refused(pkg, lambda: lv.seek(W - 1), "multiple of window_samples")
            assert np.array_equal(lv.fetch(), a)
        recs.append(np.concatenate([a, lv.process_host(lsc["x"][:, half:])], axis=1))
        lv.close()
    assert recs[0].tobytes() == recs[1].tobytes()
    tl.same_records(recs[0], lsc["want"], "level, a refused seek in between")
    gsc = gate_scene(pkg, W, 1, 3, "bernoulli")
    res = []
    for refuse in (True, False):
        gate = pkg.Gate(NCH, gsc["n"], W, preroll_windows=3)
        a = gate.process_host(gsc["stream"][:, :half], tg.records_of(pkg, gsc["mask"], 0, half // W))
        if refuse:
            _refused(pkg, lambda: gate.seek(1 << 62), "mfm_gate_seek", "2^62")
            _refused(pkg, lambda: gate.seek(T32), "mfm_gate_seek", "multiple of window_samples")   # 2^32 = 96 mod 100
            again = gate.fetch()
            assert np.array_equal(again[0], a[0]) and np.array_equal(again[1], a[1])
        bb = gate.process_host(gsc["stream"][:, half:], tg.records_of(pkg, gsc["mask"], half // W, gsc["n"] // W))
        gate.flush_device()
        res.append((a, bb, gate.fetch()))
        gate.close()
    for x, y in zip(res[0], res[1]):
        tg.same(x, y, "gate, a refused seek in between")
    for got, want in zip(res[0], _gate_want(pkg, gsc, W, 1, 3, [half, gsc["n"] - half])):
        tg.same(got, want, "gate, a refused seek in between, against the restatement")


@pytest.mark.gpu
def test_gpu_gate_seeked_without_its_level_stage_is_out_of_step(pkg):
    """the gate stands at 2^32 + 4 windows, the level stage that writes its records at 0: the record check against `.window`
    (all 64 bits of it) raises the flag; seeked to the same place the pair agrees, and 2^32 windows apart is caught too"""
    W = 64
    sc = level_scene(pkg, W, tl.PCM)
    kw = sc["kw"]
    rows = sc["x"][:, :10 * W]
    for level_at, gate_at, ok in ((0, T32 + 4 * W, False), (T32 + 4 * W, T32 + 4 * W, True), (4 * W, T32 * W + 4 * W, False)):
        lv = pkg.Level(NCH, 10 * W, W, open_thr=kw["open_thr"], close_thr=kw["close_thr"], hang_windows=kw["hang"])
        gate = pkg.Gate(NCH, 10 * W, W)
        lv.seek(level_at)
        gate.seek(gate_at)
        rec = lv.process_host(rows)
        assert int(rec["window"][0, 0]) == level_at // W
        if ok:
            runs, _ = gate.process_host(rows, rec)
            assert (runs["first_window"] >= np.uint64(gate_at // W)).all()
        else:
            with pytest.raises(pkg.MfmError) as ei:
                gate.process_host(rows, rec)
            assert ei.value.code == pkg.binding.MFM_E_STATE and "out of step" in str(ei.value)
        gate.close()
        lv.close()


# ---- window numbers above 2^32 through the burst chain -------------------------------------------------------------------

CH_W, CH_P, CH_N = 100, 2, 48000
CH_CUTS = [16033, 17744, CH_N - 16033 - 17744]   # 2^32 of the "inside" base lies in the second call
CHAIN_PLACES = list(FIXED) + ["inside"]
CH_K = 260                                       # the window of the scene that 2^32 is put into
STAGES = ["runpocsag", "runais", "runflex"]
CH_MOD = {"runpocsag": trp, "runais": tra, "runflex": trf}


def chain_scene(pkg, ora):
    """four channels of 48 000 samples, near silence around: 0: two 2400 baud POCSAG transmissions; 1: AIS packets back to back
    with a silent hole; 2: one FLEX frame; 3: one 1200 baud POCSAG transmission.  Resampled 1 : 1, so every burst decoder reads
    the same samples.  The mask is the level restatement's squelch (energy, hang 2), the gate has a pre-roll of 2; the wanted
    results of every call come from the oracle per stretch (the Checker classes of test_runpocsag, test_runais and
    test_runflex), once, at base 0"""
    def make():
        sy = pkg.synth
        rng = np.random.RandomState(8)
        x = (rng.randn(4, CH_N) * 60).round().astype(np.int16)
        at = 1500
        for seed in (0, 2):
            p, _ = trp._tx(sy, ora, "short2400", seed)
            x[0, at:at + p.size] = p
            at += p.size + 3000
        assert at - 3000 <= CH_N
        busy = ta._busy(sy, 31, CH_N - 1000)
        x[1, 1000:] = busy
        x[1, 20000:24000] = (rng.randn(4000) * 60).round().astype(np.int16)
        f = sy.flex_pcm(tf._frames(sy, 0, 1), noise=300, seed=3)
        x[2, 2050:2050 + f.size] = f
        p, _ = trp._tx(sy, ora, "one1200", 1)
        x[3, 2000:2000 + p.size] = p
        W, P = CH_W, CH_P
        kw = dict(metric=tl.ENERGY, sense=tl.ABOVE, open_thr=W * 10 ** 7, close_thr=W * 10 ** 6, hang=2)
        records = tl.restate(pkg, x, W, tl.PCM, **kw)
        mask = records["open"].astype(bool)
        # the host twin of the gate knows no stream start but window 0: with pre-roll it would emit the windows in front of
        # a base whose first P records are open.  The device gate is held to that in the gate cases above (window 0 open)
        assert not mask[:, :P + 1].any()
        taps = trp.rs_taps(pkg, ora, (1, 1, 4))
        calls = tr.gate_calls(pkg, x, mask, W, P, CH_CUTS)
        chk = {s: CH_MOD[s].Checker(pkg, ora, taps, 1, 1, W) for s in STAGES}
        want = {s: [chk[s].call(gr, gp) for gr, gp in calls] for s in STAGES}
        sc = dict(x=x, mask=mask, records=records, kw=kw, taps=taps, calls=calls, want=want)
        # the guards
        rs = [w[0][0] for w in want["runpocsag"]]
        begins = sum(int((r["flags"] & 1).sum()) for r in rs)
        ev_p = np.concatenate([w[1] for w in want["runpocsag"]])
        ev_a = np.concatenate([w[1] for w in want["runais"]])
        ev_f = np.concatenate([w[1][0] for w in want["runflex"]])
        assert begins >= 6 and (ev_p["type"] == ora.EV_BATCH).sum() >= 3 and len(ev_a) >= 5 and (ev_f["type"] == FRAME).sum() >= 1
        second = calls[1][0]
        inside = (second["first_window"] <= CH_K) & (CH_K < second["first_window"] + second["nr_windows"])
        assert inside.sum() >= 3                      # 2^32 falls into runs of three channels, in the second call
        for ev in (ev_p, ev_a, ev_f):   # 1 : 1, so an event lies near input sample stretch_window * W + sample: every decoder
            at = ev["stretch_window"].astype(np.int64) * W + ev["sample"].astype(np.int64)   # has one behind 2^32 in a stretch
            assert ((ev["stretch_window"] < CH_K) & (at > (CH_K + 1) * W)).any()            # that began in front of it
            assert (at < CH_K * W).any() or ev is ev_f                                     # (one frame: nothing in front)
        sc["state0"] = _twin_chain(pkg, sc, 0)
        return sc
    return cached("chain", make)


def chain_base(place):
    return window_base(CH_W, place, CH_K)


def _shift(stage, want, kb):
    """a call's wanted (burst resampler result, stage result) with base / W added to every window number"""
    (runs, payload), ev = want
    runs = runs.copy()
    runs["first_window"] += np.uint64(kb)
    if stage == "runflex":
        e = ev[0].copy()
        e["stretch_window"] += np.uint64(kb)
        return (runs, payload), (e, ev[1])
    ev = ev.copy()
    ev["stretch_window"] += np.uint64(kb)
    return (runs, payload), ev


def _shift_gate(call, kb):
    runs = call[0].copy()
    runs["first_window"] += np.uint64(kb)
    return runs, call[1]


def _records_at(pkg, sc, k0, k1, kb):
    rec = sc["records"][:, k0:k1].copy()
    rec["window"] += np.uint64(kb)
    return rec


def _twin_chain(pkg, sc, base):
    """the gate's, the burst resampler's and the three decoders' host twins, call by call, against the wanted results at `base`;
    returns the burst resampler's state after the flush"""
    b = pkg.binding
    W, P, kb = CH_W, CH_P, base // CH_W
    hist, bits = np.zeros((4, (P + 1) * W), np.int16), np.zeros(4, np.uint64)
    state, pending = b.hosttwin_runrs_state(4, len(sc["taps"]), 1)
    twin = {s: getattr(b, f"hosttwin_{s}_state")(4) for s in STAGES}
    pos = 0
    for i in range(len(CH_CUTS) + 1):
        if i < len(CH_CUTS):
            m = CH_CUTS[i]
            g = b.hosttwin_gate_call_preroll(W, 1, P, base + pos, sc["x"][:, pos:pos + m], hist, bits, _records_at(pkg, sc, pos // W, (pos + m) // W, kb))
            pos += m
        else:
            g = b.hosttwin_gate_call_preroll(W, 1, P, base + pos, np.zeros((4, 0), np.int16), hist, bits, np.zeros((4, 0), b.LEVEL_RECORD_DTYPE),
                                             flush=True)
        what = f"twin chain at {base}, call {i}"
        tg.same(g, _shift_gate(sc["calls"][i], kb), what)
        rs = b.hosttwin_runrs_call(W, sc["taps"], 1, 1, state, pending, *g)
        for s in STAGES:
            want = _shift(s, sc["want"][s][i], kb)
            tr.same(rs, want[0], what)
            CH_MOD[s].same(getattr(b, f"hosttwin_{s}_call")(twin[s], *rs), want[1], f"{what}, {s}")
    return state.copy()


@pytest.mark.parametrize("place", CHAIN_PLACES)
def test_hosttwin_burst_chain_carries_window_numbers_above_2_to_the_32(pkg, ora, place):
    """mfm_hosttwin_gate_call_preroll at pos = base, then the burst resampler's and the three burst decoders' twins: events and
    payload are those of base 0 (the oracle's, per stretch), every first_window and stretch_window is base / W further, and
    so is mfm_runrs_state.expected"""
    sc = chain_scene(pkg, ora)
    base = chain_base(place)
    b = pkg.binding
    if place == "inside":
        assert base + CH_CUTS[0] < T32 < base + CH_CUTS[0] + CH_CUTS[1] and base // CH_W + CH_K == T32 // CH_W and T32 % CH_W
    state = _twin_chain(pkg, sc, base)
    s0 = sc["state0"]
    live = s0["expected"] != b.MFM_RUNRS_NO_WINDOW
    assert live.any()
    assert np.array_equal(state["expected"][live], s0["expected"][live] + np.uint64(base // CH_W))
    assert (state["expected"][~live] == b.MFM_RUNRS_NO_WINDOW).all()
    for f in ("outs", "phase", "pending"):
        assert np.array_equal(state[f], s0[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("place", CHAIN_PLACES)
def test_gpu_burst_chain_behind_a_seeked_level_and_gate(pkg, ora, place):
    """Level.seek + Gate.seek after another stream, then Level -> Gate -> RunResampler -> RunPocsag, RunAis, RunFlex on the
    device views, three calls (2^32 inside the second at the "inside" base) and the flush: every stage's fetch against the
    level restatement, the gate restatement and the oracle per stretch, with base / W added to the window numbers; the
    decoders' twins run beside them on the wanted run lists"""
    import torch
    sc = chain_scene(pkg, ora)
    base = chain_base(place)
    b = pkg.binding
    W, P, kb = CH_W, CH_P, base // CH_W
    cap = max(CH_CUTS)
    kw = sc["kw"]
    lv = pkg.Level(4, cap, W, open_thr=kw["open_thr"], close_thr=kw["close_thr"], hang_windows=kw["hang"])
    gate = pkg.Gate(4, cap, W, preroll_windows=P)
    rr = pkg.RunResampler(4, sc["taps"], 1, 1, W, max_in_samples=cap, preroll_windows=P)
    dec = {"runpocsag": pkg.RunPocsag.behind(rr), "runais": pkg.RunAis.behind(rr), "runflex": pkg.RunFlex.behind(rr)}
    twin = {s: getattr(b, f"hosttwin_{s}_state")(4) for s in STAGES}
    # something to forget: five loud windows and a half through level and gate
    loud = np.random.RandomState(1).randint(-32768, 32768, size=(4, 5 * W + W // 2)).astype(np.int16)
    rec = lv.process_host(loud)
    assert rec["open"].all()
    assert len(gate.process_host(loud, rec)[0]) == 4
    lv.seek(base)
    gate.seek(base)
    pos = 0
    for i in range(len(CH_CUTS) + 1):
        what = f"chain at {base} ({place}), call {i}"
        if i < len(CH_CUTS):
            m = CH_CUTS[i]
            d, ptr = tl._on_device(torch, sc["x"][:, pos:pos + m], m + 1, 3)
            lv.process_device(ptr, m + 1, m)
            d_rec, rec_stride, nwin, _ = lv.device_view()
            gate.process_device(ptr, m + 1, m, d_rec, rec_stride, nwin)
            tl.same_records(lv.fetch(), _records_at(pkg, sc, pos // W, (pos + m) // W, kb), what)
            pos += m
        else:
            gate.flush_device()
        rr.process_device(*gate.device_view())
        got = {}
        for s in STAGES:
            dec[s].process_device(*rr.device_view())
            got[s] = dec[s].fetch()
        tg.same(gate.fetch(), _shift_gate(sc["calls"][i], kb), what)
        rs = rr.fetch()
        for s in STAGES:
            want = _shift(s, sc["want"][s][i], kb)
            tr.same(rs, want[0], what)
            CH_MOD[s].same(got[s], want[1], f"{what}, {s}")
            CH_MOD[s].same(getattr(b, f"hosttwin_{s}_call")(twin[s], *want[0]), got[s], f"{what}, {s} against its twin")
        d = None   # the call's rows were read: every fetch above waited for its stage
    for o in list(dec.values()) + [rr, gate, lv]:
        o.close()
