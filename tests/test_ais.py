"""The AIS stage: the sequential restatement (tests/ais_restatement.c) pinned to what the protocol and the reference's
decoder say, the host message layer (tsl-sdr_amd/host/mfm_ais.c) against it on the CPU, aisdecoder_amd's command line,
then bit-exact GPU parity of mfm_ais (every event field) alone, behind the resampler and in the full chain
multifm_amd -> aisdecoder_amd."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ais_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tsl-sdr_amd", "host")
HOST_SO = os.path.join(HOST_DIR, "libmfm_host.so")
TOOL = os.path.join(HOST_DIR, "aisdecoder_amd")

T1 = dict(mmsi=123456789, nav_stat=5, rot=-12, sog=123, pos_acc=1, lon=-7234567, lat=2345678, course=1234, heading=234,
          seconds=45)
T4 = dict(mmsi=111222333, year=2026, month=10, day=16, hour=1, minute=2, second=3, lon=1234567, lat=-2345678, epfd=7)
T5 = dict(mmsi=987654321, version=1, imo=9876543, callsign='AB"1', ship_name="SEA \\SPRITE/", ship_type=70, bow=100,
          stern=20, port=10, starboard=12, fix=1, eta_month=10, eta_day=16, eta_hour=12, eta_minute=30, draught=123,
          destination="BREST")


def _payloads(sy):
    return [sy.ais_type1(**T1), sy.ais_type4(**T4), sy.ais_type5(**T5)]


def _check_fields(line, kind):
    assert line.startswith('{"proto":"ais","type":"') and '"timestamp":"1970-01-01 00:00:00 UTC"' in line
    d = json.loads(line.replace("\\/", "/")) if kind < 2 else None
    if kind == 0:
        assert d["type"] == "positionReport"
        assert (d["mmsi"], d["navStat"], d["rateOfTurn"], d["positionAcc"], d["course"], d["heading"], d["seconds"]) == \
            (T1["mmsi"], T1["nav_stat"], T1["rot"], T1["pos_acc"], T1["course"], T1["heading"], T1["seconds"])
        assert d["speedOverGround"] == pytest.approx(T1["sog"] / 10, abs=1e-5)
        assert d["geoPosition"]["lon"] == pytest.approx(T1["lon"] / 600000.0, abs=2e-6)
        assert d["geoPosition"]["lat"] == pytest.approx(T1["lat"] / 600000.0, abs=2e-6)
    elif kind == 1:
        assert d["type"] == "baseStationReport" and d["mmsi"] == T4["mmsi"]
        assert d["baseStationDate"] == "2026-10-16 01:02:03 UTC" and d["fixType"] == "Surveyed"
        assert d["geoPosition"]["lon"] == pytest.approx(T4["lon"] / 600000.0, abs=2e-6)
    else:
        # callsign / ship name / destination are printed unescaped (decoder.c:372), so this line is not strict JSON
        assert '"type":"staticAndVoyageData"' in line and '"mmsi":987654321,"version":1,"imoNumber":9876543,' in line
        assert '"callsign":"AB"1@@@","shipName":"SEA \\SPRITE/@@@@@@@@"' in line
        assert '"dimensions":{"toBow":100,"toStern":20,"toPort":10,"toStarboard":12},"fixType":"GPS"' in line
        assert '"eta":"10-16 12:30","draught":12.300000,"destination":"BREST@@@@@@@@@@@@@@@"' in line


# ---- the restatement ---------------------------------------------------------------------------------------

def test_restatement_crc_is_crc16_x25():
    assert ais_ref.crc16(b"123456789") == 0x906E


def test_synth_fcs_matches_restatement(pkg):
    rng = np.random.RandomState(1)
    for n in (0, 1, 21, 53, 158):
        data = bytes(rng.randint(0, 256, n).astype(np.uint8))
        assert pkg.synth.ais_crc16(data) == ais_ref.crc16(data)


@pytest.mark.parametrize("phase", range(5))
def test_restatement_decodes_synth_frames_at_every_phase(pkg, phase):
    sy = pkg.synth
    for kind, payload in enumerate(_payloads(sy)):
        bits = sy.ais_bits([sy.ais_frame_bits(payload)], lead_bits=7, trail_bits=11)
        pcm = sy.ais_pcm(bits, noise=300, lead=333, trail=50, phase=phase, seed=phase)
        ev = ais_ref.demod(pcm)
        assert len(ev) == 1 and ev[0]["fcs_valid"] == 1 and ev[0]["nr_bytes"] == len(payload) + 2
        assert bytes(ev[0]["bytes"][:len(payload)]) == payload
        text, st = ais_ref.json_lines(ev)
        assert st == {"crc_rejects": 0, "short": 0, "lines": 1}
        _check_fields(text, kind)


# ---- the host message layer on the CPU ---------------------------------------------------------------------

class PositionReport(C.Structure):
    _fields_ = [("mmsi", C.c_uint32), ("nav_stat", C.c_uint32), ("position_acc", C.c_uint32), ("course", C.c_uint32),
                ("heading", C.c_uint32), ("timestamp", C.c_uint32), ("longitude", C.c_float), ("latitude", C.c_float),
                ("rate_of_turn", C.c_int32), ("speed_over_ground", C.c_float)]


class BaseStationReport(C.Structure):
    _fields_ = [("mmsi", C.c_uint32), ("year", C.c_uint32), ("month", C.c_uint32), ("day", C.c_uint32),
                ("hour", C.c_uint32), ("minute", C.c_uint32), ("second", C.c_uint32), ("longitude", C.c_float),
                ("latitude", C.c_float), ("epfd_type", C.c_uint32), ("epfd_name", C.c_char_p)]


class StaticVoyageData(C.Structure):
    _fields_ = [("mmsi", C.c_uint32), ("version", C.c_uint32), ("imo_number", C.c_uint32), ("ship_type", C.c_uint32),
                ("dim_to_bow", C.c_uint32), ("dim_to_stern", C.c_uint32), ("dim_to_port", C.c_uint32),
                ("dim_to_starboard", C.c_uint32), ("fix_type", C.c_uint32), ("epfd_name", C.c_char_p),
                ("eta_month", C.c_uint32), ("eta_day", C.c_uint32), ("eta_hour", C.c_uint32), ("eta_minute", C.c_uint32),
                ("draught", C.c_float), ("callsign", C.c_char * 8), ("ship_name", C.c_char * 21),
                ("destination", C.c_char * 21)]


def _escape(s):
    """decoder.c:121-166"""
    out = []
    for ch in s:
        out.append({"\n": "\\n", "\r": "\\n", '"': '\\"', "\\": "\\\\", "/": "\\/", "\b": "<BKSP>", "\f": "<FF>",
                    "\t": "\\t", "\x03": " ", "\x04": " ", "\x17": " "}.get(ch, ch if 0x20 <= ord(ch) < 0x7F else
                                                                          "\\u%04x" % ord(ch)))
    return "".join(out)


TS = '"timestamp":"1970-01-01 00:00:00 UTC",'


def _host_decode(events):
    """feed events to ais_decode_on_events in libmfm_host.so; JSON lines formatted from what the callbacks got, with
    decoder.c:320-394's layout"""
    if not os.path.exists(HOST_SO):
        pytest.fail(f"{HOST_SO} missing: run make -C tsl-sdr_amd")
    L = C.CDLL(HOST_SO)
    lines = []
    F1 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PositionReport), C.c_char_p)
    F4 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BaseStationReport), C.c_char_p)
    F5 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(StaticVoyageData), C.c_char_p)

    def raw(r):
        return _escape(r.decode("latin-1")) + '"}\n'

    def on1(d, st, p, r):
        p = p.contents
        lines.append('{"proto":"ais","type":"positionReport",' + TS +
                     '"mmsi":%u,"navStat":%u,"rateOfTurn":%d,"speedOverGround":%f,"positionAcc":%u,'
                     '"geoPosition":{"lon":%f,"lat":%f},"course":%u,"heading":%u,"seconds":%u,"rawAscii":"'
                     % (p.mmsi, p.nav_stat, p.rate_of_turn, p.speed_over_ground, p.position_acc, p.longitude, p.latitude,
                        p.course, p.heading, p.timestamp) + raw(r))
        return 0

    def on4(d, st, b, r):
        b = b.contents
        lines.append('{"proto":"ais","type":"baseStationReport",' + TS +
                     '"mmsi":%u,"baseStationDate":"%04u-%02u-%02u %02u:%02u:%02u UTC",'
                     '"geoPosition":{"lon":%f,"lat":%f},"fixType":"%s","rawAscii":"'
                     % (b.mmsi, b.year, b.month, b.day, b.hour, b.minute, b.second, b.longitude, b.latitude,
                        b.epfd_name.decode()) + raw(r))
        return 0

    def on5(d, st, s, r):
        s = s.contents
        lines.append('{"proto":"ais","type":"staticAndVoyageData",' + TS +
                     '"mmsi":%u,"version":%u,"imoNumber":%u,"callsign":"%s","shipName":"%s",'
                     '"shipType":%u,"dimensions":{"toBow":%u,"toStern":%u,"toPort":%u,"toStarboard":%u},'
                     '"fixType":"%s","eta":"%02u-%02u %02u:%02u","draught":%f,"destination":"%s","rawAscii":"'
                     % (s.mmsi, s.version, s.imo_number, s.callsign.decode("latin-1"), s.ship_name.decode("latin-1"),
                        s.ship_type, s.dim_to_bow, s.dim_to_stern, s.dim_to_port, s.dim_to_starboard,
                        s.epfd_name.decode(), s.eta_month, s.eta_day, s.eta_hour, s.eta_minute, s.draught,
                        s.destination.decode("latin-1")) + raw(r))
        return 0

    cbs = (F1(on1), F4(on4), F5(on5))
    L.ais_decode_new.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, F1, F4, F5]
    L.ais_decode_on_events.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ais_decode_crc_rejects.argtypes = [C.c_void_p]
    L.ais_decode_crc_rejects.restype = C.c_size_t
    L.ais_decode_short_packets.argtypes = [C.c_void_p]
    L.ais_decode_short_packets.restype = C.c_size_t
    L.ais_decode_set_user.argtypes = [C.c_void_p, C.c_void_p]
    L.ais_decode_get_user.argtypes = [C.c_void_p]
    L.ais_decode_get_user.restype = C.c_void_p
    L.ais_decode_delete.argtypes = [C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.ais_decode_new(C.byref(h), 161975000, *cbs) == 0
    L.ais_decode_set_user(h, C.c_void_p(0x1234))
    assert L.ais_decode_get_user(h) == 0x1234
    ev = np.ascontiguousarray(events, dtype=ais_ref.EVENT_DTYPE)
    # one call with everything and, on a second object, one call per event: same result
    assert L.ais_decode_on_events(h, ev.ctypes.data, len(ev)) == 0
    stats = {"crc_rejects": L.ais_decode_crc_rejects(h), "short": L.ais_decode_short_packets(h), "lines": len(lines)}
    assert L.ais_decode_delete(C.byref(h)) == 0 and not h.value
    return "".join(lines), stats


def test_host_decode_matches_restatement(pkg):
    sy = pkg.synth
    p1, p4, p5 = _payloads(sy)
    rng = np.random.RandomState(3)
    long1 = p1 + bytes(rng.randint(0, 256, 158 - len(p1)).astype(np.uint8))  # 160 bytes with the FCS: rawAscii cap
    ev = np.concatenate([
        ais_ref.event(p1),                                  # 21 bytes: len % 3 == 0
        ais_ref.event(p4 + b"\x5c"),                        # 22: % 3 == 1
        ais_ref.event(p5),                                  # 53: % 3 == 2
        ais_ref.event(sy.ais_type1(**dict(T1, msg_type=3)) + b"\xff\x00"),  # 23: % 3 == 2, type 3
        ais_ref.event(p1, fcs=0x1234),                      # CRC reject: counted, not printed
        ais_ref.event(p5[:40]),                             # valid FCS, type 5, too short: dropped and counted
        ais_ref.event(p1[:17]),                             # type 1 one byte short
        ais_ref.event(p4[:18]),                             # type 4, exactly long enough
        ais_ref.event(b"\x24" + p1[1:]),                    # type 9: nothing
        ais_ref.event(b"\x04\x00"),                         # 4 bytes with the FCS, the shortest candidate
        ais_ref.event(long1),
        ais_ref.event(long1[:148]), ais_ref.event(long1[:147]), ais_ref.event(long1[:146]),
    ])
    want, wst = ais_ref.json_lines(ev)
    got, gst = _host_decode(ev)
    assert wst == {"crc_rejects": 1, "short": 3, "lines": 9}
    assert gst == wst
    assert got == want
    lines = want.splitlines()
    _check_fields(lines[0], 0)
    _check_fields(lines[1], 1)
    _check_fields(lines[2], 2)
    raws = [json.loads(x.replace("\\/", "/"))["rawAscii"] for x in lines if "positionReport" in x]
    assert [len(r) for r in raws[-4:]] == [196, 196, 196, 196]   # 158, 148, 147 bytes -> 49 groups; 146 -> 49 too
    assert len(raws[0]) == 28
    # a last group of one byte: its value sits in the low bits, the first two characters are '0'
    r4 = json.loads(lines[1].replace("\\/", "/"))["rawAscii"]
    assert len(r4) == 32 and r4[-4:-2] == "00"


def test_aisdecoder_parses_reference_options_and_refuses_without_a_gpu(tmp_path):
    """aisdecoder_amd takes decoder_amd's command line; missing pieces stop it with the reference's messages, and
    without a device it stops at the GPU resampler instead of falling back to anything on the CPU"""
    if not os.path.exists(TOOL):
        pytest.fail(f"{TOOL} missing: run make -C tsl-sdr_amd")
    (tmp_path / "f.json").write_text(json.dumps({"lpfCoeffs": [1.0]}))
    (tmp_path / "in.pcm").write_bytes(np.zeros(4096, np.int16).tobytes())
    inp = str(tmp_path / "in.pcm")
    base = [TOOL, "-I", "1", "-D", "1", "-S", "48000", "-F", str(tmp_path / "f.json"), "-f", "161975000"]

    def run(args):
        return subprocess.run(args, capture_output=True, text=True, timeout=60)

    r = run([TOOL, "-h"])
    assert r.returncode == 0 and "USAGE" in r.stderr
    r = run(base)
    assert r.returncode != 0 and "MISSING-SRC-DEST" in r.stderr
    r = run([TOOL, "-I", "1", "-D", "1", "-f", "161975000", inp])
    assert r.returncode != 0 and "BAD-FILTER-FILE" in r.stderr
    r = run([TOOL, "-F", str(tmp_path / "f.json"), inp])
    assert r.returncode != 0 and "BAD-PAGER-FREQ" in r.stderr
    r = run(base + ["-D", "0", inp])
    assert r.returncode != 0 and "BAD-DECIMATION" in r.stderr
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    full = base + ["-b", "-p", "0.999", "-i", "-c", "-o", str(tmp_path / "out.json"), "-B", "1024", "-g", "0", inp]
    r = run(full)
    assert "Resampling: 1/1 from 48000 to 48000.000000" in r.stderr
    if has_gpu:
        assert r.returncode == 0 and (tmp_path / "out.json").read_text() == "", r.stderr[-2000:]
    else:
        assert r.returncode != 0 and "NO-RESAMPLER" in r.stderr, r.stderr[-2000:]


# ---- the GPU stage -----------------------------------------------------------------------------------------

def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ais_ref.EVENT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f


def _run(pkg, pcm2d, cuts=None):
    """events of [C][n] PCM through mfm_ais, in one call or cut into calls at `cuts`"""
    pcm2d = np.ascontiguousarray(pcm2d, np.int16)
    C_, n = pcm2d.shape
    bounds = [0] + list(cuts or []) + [n]
    biggest = max(max(b - a for a, b in zip(bounds, bounds[1:])), 1)
    st = pkg.Ais(C_, biggest)
    parts = []
    for a, b in zip(bounds, bounds[1:]):
        parts.append(st.process_host(pcm2d[:, a:b]))
    st.close()
    ev = np.concatenate(parts)
    # fetch order is per call, channels ascending; the restatement's is per channel: compare channel by channel
    return ev[np.argsort(ev["channel"], kind="stable")]


def _busy(sy, seed, n, noise=400.0, flips=True):
    """a channel with frames of all three types, back-to-back ones, CRC rejects and a missing end flag"""
    rng = np.random.RandomState(seed)
    pl = _payloads(sy)
    frames = []
    while sum(len(f) for f in frames) * 5 < n - 3000:
        k = rng.randint(0, 6)
        if k < 3:
            frames.append(sy.ais_frame_bits(pl[k]))
        elif k == 3:
            frames.append(sy.ais_frame_bits(pl[rng.randint(0, 3)], fcs=int(rng.randint(0, 65536))))
        elif k == 4:
            frames.append(sy.ais_frame_bits(bytes(rng.randint(0, 256, 30).astype(np.uint8))))
        else:
            frames.append(np.ones(int(rng.randint(1, 400)), np.uint8))
    bits = sy.ais_bits(frames, gap_bits=int(rng.randint(0, 4)))
    flip = rng.choice(bits.size, bits.size // 400, replace=False) if flips else None
    x = sy.ais_pcm(bits, noise=noise, lead=int(rng.randint(0, 50)), phase=int(rng.randint(0, 5)), seed=seed, flip=flip)
    x = np.concatenate([x, (rng.randn(max(0, n - x.size)) * noise).round().astype(np.int16)])[:n]
    return x


@pytest.mark.gpu
def test_gpu_clean_frames_all_types_every_phase(pkg):
    sy = pkg.synth
    chans = []
    for payload in _payloads(sy):
        for phase in range(5):
            bits = sy.ais_bits([sy.ais_frame_bits(payload)], lead_bits=3, trail_bits=9)
            chans.append(sy.ais_pcm(bits, noise=200, lead=1000 + 37 * phase, trail=3000, phase=phase, seed=phase))
    n = min(x.size for x in chans)
    pcm = np.stack([x[:n] for x in chans])
    want = ais_ref.demod_channels(pcm)
    assert len(want) == 15 and want["fcs_valid"].all()
    got = _run(pkg, pcm)
    _same(got, want)
    for c in range(15):
        text, _ = ais_ref.json_lines(got[got["channel"] == c])
        _check_fields(text, c // 5)


@pytest.mark.gpu
def test_gpu_noise_errors_back_to_back_stream_start_and_1280_bit_cut(pkg):
    sy = pkg.synth
    rng = np.random.RandomState(11)
    p1, p4, p5 = _payloads(sy)
    n = 120000
    chans = [
        _busy(sy, 1, n), _busy(sy, 2, n, noise=2500.0), _busy(sy, 3, n, flips=False),
        # a preamble at sample 0, then packets back to back: the second preamble lies in the reset window
        sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(p) for p in (p1, p4, p5, p1, p1)]), trail=n),
        sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(p) for p in (p5, p4)], gap_bits=1), phase=3, trail=n),
        # no end flag: stuffed data never holds 0x7e, so the packet is cut at 1280 bits
        sy.ais_pcm(sy.ais_frame_bits(bytes(rng.randint(0, 256, 200).astype(np.uint8)), end_flag=False), lead=77,
                   noise=100, trail=n, seed=4),
        # after a preamble only 1s: the receiver never ends (nr_ones >= 5 writes nothing)
        sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(p1)[:40]], trail_bits=20000), lead=5, trail=n),
        (rng.randn(n) * 3000).round().astype(np.int16),
        np.zeros(n, np.int16),
    ]
    pcm = np.stack([x[:n] for x in chans])
    want = ais_ref.demod_channels(pcm)
    assert (want["fcs_valid"] == 0).sum() >= 3 and (want["fcs_valid"] == 1).sum() >= 10
    assert (want["nr_bytes"] == 160).any()
    assert (want["start_sample"] < 300).any()
    _same(_run(pkg, pcm), want)


@pytest.mark.gpu
def test_gpu_events_do_not_depend_on_how_the_stream_is_cut(pkg):
    sy = pkg.synth
    n = 60000
    pcm = np.stack([_busy(sy, 20 + c, n) for c in range(4)] + [np.zeros(n, np.int16)])
    want = ais_ref.demod_channels(pcm)
    assert len(want) >= 10
    rng = np.random.RandomState(5)
    tiny = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 100, 101, 102]  # 1-sample calls at the very start
    cuts_list = [
        tiny + sorted(rng.choice(np.arange(200, n), 40, replace=False).tolist()),
        sorted(set(rng.choice(np.arange(1, n), 300, replace=False).tolist())),
        list(range(4999, n, 4999)),
    ]
    # 1-sample calls right around a packet end and a preamble
    e0 = int(want["sample"][0])
    cuts_list.append(sorted(set(range(e0 - 3, e0 + 4)) | set(range(int(want["start_sample"][1]) - 2,
                                                                      int(want["start_sample"][1]) + 3))))
    for cuts in cuts_list:
        _same(_run(pkg, pcm, cuts), want)


@pytest.mark.gpu
@pytest.mark.parametrize("nr_channels", [64, 1024])
def test_gpu_many_channels_idle_and_busy(pkg, nr_channels):
    sy = pkg.synth
    n = 40000
    rng = np.random.RandomState(nr_channels)
    busy = [_busy(sy, 100 + k, n) for k in range(8)]
    pcm = np.zeros((nr_channels, n), np.int16)
    kinds = rng.randint(0, 3, nr_channels)
    for c in range(nr_channels):
        if kinds[c] == 0:
            pcm[c] = busy[c % 8]
        elif kinds[c] == 1:
            pcm[c] = (rng.randn(n) * 1000).round().astype(np.int16)
    want = ais_ref.demod_channels(pcm)
    assert (want["fcs_valid"] == 1).sum() > nr_channels // 8
    _same(_run(pkg, pcm, [n // 3, n // 3 + 1]), want)


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
def test_gpu_device_path_behind_the_resampler(pkg, ora, invert):
    """mfm_resampler_process_device -> mfm_ais_process_device on one stream, PCM never leaving HBM, 4/5 from 60 kHz
    with -i; must equal the oracle resampler followed by the restatement"""
    import torch
    sy = pkg.synth
    n_in, blk = 150000, 25000
    chans = [_busy(sy, 40 + c, n_in * 4 // 5) for c in range(6)]
    # 60 kHz input whose 4/5 resampling is close to the 48 kHz frames (the filter smooths; the comparison is exact)
    x60 = np.stack([np.repeat(x, 5)[::4][:n_in] for x in chans])
    x_in = (-x60.astype(np.int32)).clip(-32768, 32767).astype(np.int16) if invert else x60
    taps = sy.design_lpf(41, 0.45 / 5, 1.0) * 4
    rtaps = ora.quantize_taps(taps)
    rs = pkg.Resampler(len(chans), rtaps, 4, 5, blk, device=0, invert=invert)
    st = pkg.Ais(len(chans), rs.max_out())
    d = torch.from_numpy(np.ascontiguousarray(x_in)).cuda()
    parts = []
    for a in range(0, n_in, blk):
        yptr, ystride, ny = rs.process_device(d.data_ptr() + 2 * a, n_in, min(blk, n_in - a))
        st.process_device(yptr, ystride, ny)
        parts.append(st.fetch_events())
    got = np.concatenate(parts)
    got = got[np.argsort(got["channel"], kind="stable")]
    want = ais_ref.demod_channels(np.stack([ora.Resampler(rtaps, 4, 5, invert=invert).feed(x) for x in x_in]))
    assert (want["fcs_valid"] == 1).sum() >= 6
    _same(got, want)
    st.close()
    rs.close()


@pytest.mark.gpu
def test_gpu_chain_multifm_amd_to_aisdecoder_amd(tmp_path, ora, pkg):
    """IQ at 2.4 MS/s -> multifm_amd (D 50 -> 48 kHz, two channels) -> PCM files -> aisdecoder_amd -> JSON lines;
    equal to the restatement's lines on the same PCM through the oracle resampler, time fixed"""
    sy = pkg.synth
    fs, decim = 2400000, 50
    center = 162000000
    offs = (-150000.0, 100000.0)  # clear of the capture's DC at the tuner centre
    pl = _payloads(sy)
    n = 4096 * 600 + 777
    acc = np.zeros((n, 2), np.float64)
    for k, o in enumerate(offs):
        frames = [sy.ais_frame_bits(pl[(k + j) % 3]) for j in range(4)]
        bits = sy.ais_bits(frames, gap_bits=200, lead_bits=100 + 37 * k, trail_bits=0)
        burst = sy.ais_fm_iq(bits, fs, o, amplitude=40.0, noise=1.5, seed=k)
        m = min(n, burst.shape[0])
        acc[:m] += burst[:m]
    raw = np.clip(np.round(acc + 127.0), 0, 255).astype(np.uint8)
    cap = tmp_path / "capture.cu8"
    cap.write_bytes(raw.tobytes())
    lpf = sy.design_lpf(128, 12500.0, float(fs))
    (tmp_path / "taps.json").write_text(json.dumps({"lpfTaps": [float(t) for t in lpf]}))
    cfg = {"device": {"type": "file", "filename": str(cap), "fileFormat": "cu8"}, "sampleRateHz": fs,
           "centerFreqHz": center, "nrSampBufs": 32, "decimationFactor": decim,
           "channels": [{"outFifo": str(tmp_path / f"ch{c}.pcm"), "chanCenterFreq": int(center + o), "dBGain": 6.0}
                        for c, o in enumerate(offs)]}
    for c in range(len(offs)):
        (tmp_path / f"ch{c}.pcm").write_bytes(b"")
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    r = subprocess.run([os.path.join(HOST_DIR, "multifm_amd"), str(tmp_path / "cfg.json"), str(tmp_path / "taps.json")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    (tmp_path / "filter.json").write_text(json.dumps({"lpfCoeffs": [0.25, 0.5, 0.25]}))
    env = dict(os.environ, MFM_DECODER_FIXED_TIME="1")
    r = subprocess.run([TOOL, "-I", "1", "-D", "1", "-S", "48000", "-F", str(tmp_path / "filter.json"), "-f", str(center),
                        "-c", "-o", str(tmp_path / "ais.json"), "-B", "10000"] +
                       [str(tmp_path / f"ch{c}.pcm") for c in range(len(offs))],
                       capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rtaps = ora.quantize_taps([0.25, 0.5, 0.25])
    total = 0
    for c in range(len(offs)):
        pcm = np.frombuffer((tmp_path / f"ch{c}.pcm").read_bytes(), dtype=np.int16)
        want, st = ais_ref.json_lines(ais_ref.demod(ora.Resampler(rtaps, 1, 1).feed(pcm)))
        total += st["lines"]
        assert (tmp_path / f"ais.json.{c}").read_text() == want, f"channel {c}"
    assert total >= 6
