/*
 * mfm_level.h - the arithmetic of the signal-level / squelch stage (mfm_level_*, include/multifm_hip.h), stated once for
 * the kernels and for the host twins (mfm_hosttwin_level_window, mfm_hosttwin_squelch_step) the CPU tests run.
 *
 * A row is a run of int16 ELEMENTS: one per sample in the PCM form, two (re, im) in the IQ form.  Everything here works on
 * pairs of consecutive elements packed in a dword (lower half = the earlier element), which is how a 16-byte load
 * delivers them, and in packed 16-bit arithmetic:
 *
 *   |x|      max(x, 0 - x) as int16; -32768 stays 0x8000, which READ AS uint16 is 32768
 *   energy   |lo|^2 + |hi|^2 <= 2^31 fits a uint32 (a signed 32-bit sum of two squares would not: two -32768 give 2^31);
 *            the pair sums are added up in 64 bits
 *   diff     d = x[n] - x[n-1] in uint16 arithmetic IS the difference wrapped to 16 bits; then |d|^2 as above
 *   peak     a packed maximum of |x|; the larger half is taken once at the end
 *
 * All of it is exact integer arithmetic: sums do not depend on the order in which pairs, lanes or waves are added up.
 */
#ifndef MFM_LEVEL_H
#define MFM_LEVEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t mfm_u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t mfm_i16x2 __attribute__((ext_vector_type(2)));

struct mfm_level_acc {
    uint64_t energy, diff;
    mfm_u16x2 peak;
};

/* eight elements as a 16-byte load takes them off a row of any alignment */
struct __attribute__((packed, aligned(2))) mfm_level_x8 {
    uint32_t d[4];
};

__host__ __device__ inline mfm_u16x2 mfm_level_abs2(mfm_u16x2 x)
{
    const mfm_u16x2 nx = (mfm_u16x2)(0) - x;
    return __builtin_bit_cast(mfm_u16x2, __builtin_elementwise_max(__builtin_bit_cast(mfm_i16x2, x), __builtin_bit_cast(mfm_i16x2, nx)));
}

__host__ __device__ inline uint32_t mfm_level_sq2(mfm_u16x2 a)
{
    return (uint32_t)a.x * (uint32_t)a.x + (uint32_t)a.y * (uint32_t)a.y;
}

/*
 * One pair of elements.  x2: the pair; prev2: the pair one element earlier (its lower half is the element before x2's
 * lower half, its upper half is x2's lower half); dmask: 0xffff per half whose difference counts (an element behind the
 * end of a range has none).  with_diff is 0 in the IQ form.
 */
__host__ __device__ inline void mfm_level_step2(mfm_level_acc &a, uint32_t x2, uint32_t prev2, uint32_t dmask, bool with_diff)
{
    const mfm_u16x2 x = __builtin_bit_cast(mfm_u16x2, x2);
    const mfm_u16x2 ax = mfm_level_abs2(x);
    a.energy += mfm_level_sq2(ax);
    a.peak = __builtin_elementwise_max(a.peak, ax);
    if (with_diff) {
        const mfm_u16x2 d = (x - __builtin_bit_cast(mfm_u16x2, prev2)) & __builtin_bit_cast(mfm_u16x2, dmask);
        a.diff += mfm_level_sq2(mfm_level_abs2(d));
    }
}

/* eight elements d[0..3] of which the first `valid` exist (the others read as 0); up: the dword whose UPPER half is the
 * element in front of d[0]'s lower half */
__host__ __device__ inline void mfm_level_step8(mfm_level_acc &a, const uint32_t d[4], uint32_t up, uint32_t valid, bool with_diff)
{
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t before = q ? d[q - 1] : up;
        const uint32_t m = valid >= 2 * q + 2 ? 0xffffffffu : (valid == 2 * q + 1 ? 0xffffu : 0u);
        mfm_level_step2(a, d[q], (d[q] << 16) | (before >> 16), m, with_diff);
    }
}

__host__ __device__ inline uint32_t mfm_level_peak(const mfm_level_acc &a)
{
    return a.peak.x > a.peak.y ? a.peak.x : a.peak.y;
}

/*
 * The three sums over nr_elems elements at x (any alignment), prev = the element in front of x[0].  Adds to `a`.
 * Whole groups of eight go through one 16-byte load each, the rest element by element.
 */
__host__ __device__ inline void mfm_level_window(mfm_level_acc &a, const int16_t *x, uint32_t nr_elems, int16_t prev, bool with_diff)
{
    uint32_t up = (uint32_t)(uint16_t)prev << 16;
    uint32_t i = 0;
    for (; i + 8 <= nr_elems; i += 8) {
        const mfm_level_x8 v = *reinterpret_cast<const mfm_level_x8 *>(x + i);
        mfm_level_step8(a, v.d, up, 8, with_diff);
        up = v.d[3];
    }
    if (i < nr_elems) {
        uint32_t d[4] = { 0, 0, 0, 0 };
        for (uint32_t k = 0; i + k < nr_elems; k++) {
            d[k >> 1] |= (uint32_t)(uint16_t)x[i + k] << (16 * (k & 1));
        }
        mfm_level_step8(a, d, up, nr_elems - i, with_diff);
    }
}

/*
 * One step of the squelch, once per completed window.  below = 0: a carrier RAISES the metric (opens at metric >=
 * open_thr, a window is bad when metric < close_thr); below = 1: it LOWERS it (<= open_thr, bad when > close_thr).
 * hang + 1 bad windows in a row close; a good one resets the count.
 */
__host__ __device__ inline void mfm_level_squelch_step(uint32_t &open, uint32_t &bad, uint32_t below, uint64_t open_thr, uint64_t close_thr,
                                                       uint32_t hang, uint64_t metric)
{
    if (!open) {
        if (below ? metric <= open_thr : metric >= open_thr) {
            open = 1;
            bad = 0;
        }
    } else if (below ? metric > close_thr : metric < close_thr) {
        if (++bad > hang) {
            open = 0;
            bad = 0;
        }
    } else {
        bad = 0;
    }
}

#endif /* MFM_LEVEL_H */
