"""ctypes wrapper around tests/ais_restatement.c: the sequential AIS demod, decode and JSON lines the GPU stage,
the host message layer and aisdecoder_amd are compared against.  Compiled with gcc into a temporary directory on
first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# struct mfm_ais_event (192 bytes)
EVENT_DTYPE = np.dtype([("channel", "<u4"), ("fcs_valid", "<u4"), ("nr_bytes", "<u4"), ("reserved", "<u4"),
                        ("sample", "<u8"), ("start_sample", "<u8"), ("bytes", "u1", (160,))])
assert EVENT_DTYPE.itemsize == 192

_lib = None
_tmp = None


def lib():
    global _lib, _tmp
    if _lib is not None:
        return _lib
    _tmp = tempfile.TemporaryDirectory(prefix="ais_restatement_")
    so = os.path.join(_tmp.name, "libais_restatement.so")
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "ais_restatement.c")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building ais_restatement.c failed:\n" + r.stderr)
    L = C.CDLL(so)
    L.ais_r_crc16.restype = C.c_uint16
    L.ais_r_crc16.argtypes = [C.c_char_p, C.c_size_t]
    L.ais_r_new.restype = C.c_void_p
    L.ais_r_free.argtypes = [C.c_void_p]
    L.ais_r_free.restype = None
    L.ais_r_crc_rejects.restype = C.c_uint64
    L.ais_r_crc_rejects.argtypes = [C.c_void_p]
    L.ais_r_feed.restype = C.c_size_t
    L.ais_r_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t]
    L.ais_r_json.restype = C.c_size_t
    L.ais_r_json.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def crc16(data):
    data = bytes(data)
    return lib().ais_r_crc16(data, len(data))


class Demod:
    """one channel of the sequential demodulator; feed() can be called with any cut of the stream"""

    def __init__(self, channel=0):
        self.L = lib()
        self.h = self.L.ais_r_new()
        self.channel = channel

    def feed(self, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        cap = a.size // 160 + 16
        out = np.zeros(cap, EVENT_DTYPE)
        n = self.L.ais_r_feed(self.h, a.ctypes.data, a.size, self.channel, out.ctypes.data, cap)
        assert n <= cap
        return out[:n].copy()

    @property
    def crc_rejects(self):
        return self.L.ais_r_crc_rejects(self.h)

    def __del__(self):
        try:
            self.L.ais_r_free(self.h)
        except Exception:
            pass


def demod(pcm, channel=0):
    """events of one whole channel stream"""
    return Demod(channel).feed(pcm)


def demod_channels(pcm2d):
    """events of [C][n] PCM, channels ascending (the order mfm_ais_fetch_events uses)"""
    parts = [demod(row, c) for c, row in enumerate(np.asarray(pcm2d))]
    return np.concatenate(parts) if parts else np.zeros(0, EVENT_DTYPE)


def json_lines(events):
    """(text, {"crc_rejects", "short", "lines"}) for the events of one channel, time fixed at the epoch"""
    ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    stats = (C.c_uint64 * 3)()
    need = lib().ais_r_json(ev.ctypes.data, len(ev), None, 0, stats)
    buf = C.create_string_buffer(need + 1)
    stats = (C.c_uint64 * 3)()
    lib().ais_r_json(ev.ctypes.data, len(ev), buf, need + 1, stats)
    return buf.value.decode("latin-1"), {"crc_rejects": stats[0], "short": stats[1], "lines": stats[2]}


def event(payload, fcs=None, channel=0, sample=0, start_sample=0, fcs_valid=None, nr_bytes=None):
    """an mfm_ais_event built in Python: payload bytes, then the FCS (computed unless given)"""
    payload = bytes(payload)
    if fcs is None:
        fcs = crc16(payload)
    body = payload + bytes([fcs & 0xFF, fcs >> 8])
    e = np.zeros(1, EVENT_DTYPE)
    e["channel"], e["sample"], e["start_sample"] = channel, sample, start_sample
    e["nr_bytes"] = len(body) if nr_bytes is None else nr_bytes
    e["fcs_valid"] = int(crc16(payload) == fcs) if fcs_valid is None else fcs_valid
    e["bytes"][0, :len(body)] = np.frombuffer(body, np.uint8)
    return e
