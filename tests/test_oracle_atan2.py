"""Pin the oracle's fast_atan2f against the reference's own object code and golden vectors.

oracle/_ref/libref_fast_atan2f.so is the reference's multifm/fast_atan2f.c compiled unmodified
(oracle/Makefile).  tests/golden/atan2_ref.npz holds (y, x) -> bits it returned; tests/golden/atan2_ref_dense.npz the
bits it returned for the inputs below, so that the pin holds where the reference tree (and with it oracle/_ref) is absent.
"""
import os

import numpy as np


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def dense_inputs():
    """the operands the discriminator produces: int32 values converted to float"""
    rng = np.random.RandomState(1234)
    n = 60000
    return np.concatenate([
        rng.randint(-(1 << 31), (1 << 31) - 1, size=(n // 3, 2)).astype(np.float32),
        rng.randint(-(1 << 16), 1 << 16, size=(n // 3, 2)).astype(np.float32),
        rng.randint(-300, 300, size=(n // 3, 2)).astype(np.float32),
    ])


def knot_inputs():
    """(7, 7), then (k, 255) for every inner table knot k = 1 .. 254"""
    return np.array([[7.0, 7.0]] + [[float(k), 255.0] for k in range(1, 255)], np.float32)


def _reference_bits(ora, golden_dir, name, yx):
    """What the reference's own fast_atan2f returns for yx, as bits: the stored answers (tests/golden/make_golden.py), checked
    against the object code itself wherever oracle/_ref is built."""
    want = np.load(os.path.join(golden_dir, "atan2_ref_dense.npz"))[name]
    assert want.shape == (len(yx),)
    ref = ora.ref_atan2()
    if ref is not None:
        live = _bits([ref.fast_atan2f(float(y), float(x)) for y, x in yx])
        assert np.array_equal(live, want), f"{int((live != want).sum())} stored answers differ from oracle/_ref"
    return want


def test_oracle_matches_golden_vectors_from_reference(ora, golden_dir):
    g = np.load(os.path.join(golden_dir, "atan2_ref.npz"))
    yx, want = g["yx"], g["bits"]
    got = np.array([ora.lib().mfmo_fast_atan2f(float(y), float(x)) for y, x in yx], dtype=np.float32)
    assert np.array_equal(_bits(got), want), f"{int((_bits(got) != want).sum())} of {len(want)} differ"


def test_oracle_matches_reference_object_code_dense(ora, golden_dir):
    yx = dense_inputs()
    want = _reference_bits(ora, golden_dir, "dense", yx)
    o = ora.lib()
    got = _bits([o.mfmo_fast_atan2f(float(y), float(x)) for y, x in yx])
    bad = int((got != want).sum())
    assert bad == 0


def test_table_is_the_reference_table(ora, golden_dir):
    """T[i] read back through the reference function: for y = T-knot exact ratios the reference returns
    T[k] + (T[k+1]-T[k])*alpha with alpha in [0,1); at x=255,y=k it must land within the k-th segment."""
    tbl = ora.atan_table()
    assert tbl.shape == (257,)
    assert tbl[0] == 0.0 and tbl[255] == tbl[256] == np.float32(7.853982e-01)
    assert np.all(np.diff(tbl[:256]) > 0)
    ref_out = _reference_bits(ora, golden_dir, "knots", knot_inputs()).view(np.float32)
    # z == 1 hits index 255 with alpha 0: the reference returns pi/2 - T[255] for y >= x > 0
    v = ref_out[0]
    assert v == np.float32(np.float32(1.57079632679489661923) - tbl[255])
    # every knot: the returned angle lies inside [T[k-1], T[k+1]] (alpha rounding may move one segment)
    for k in range(1, 255):
        a = ref_out[k]
        assert tbl[k - 1] <= a <= tbl[k + 1]


def test_fused_variant_differs_by_at_most_one_pcm_lsb(ora):
    rng = np.random.RandomState(5)
    s = rng.randint(-(1 << 30), 1 << 30, size=(200000, 2)).astype(np.int32)
    sre, sim = np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(s[:, 1])
    import ctypes as C
    a = np.zeros(len(s), np.int16)
    b = np.zeros(len(s), np.int16)
    p32 = C.POINTER(C.c_int32)
    ora.lib().mfmo_discriminate_batch(sre.ctypes.data_as(p32), sim.ctypes.data_as(p32), len(s), ora.p16(a), 0)
    ora.lib().mfmo_discriminate_batch(sre.ctypes.data_as(p32), sim.ctypes.data_as(p32), len(s), ora.p16(b), 1)
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert d.max() <= 1
