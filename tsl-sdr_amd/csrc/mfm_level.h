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

/*
 * ---- The adaptive squelch (mfm_level_set_adaptive): thresholds as ratios to the channel's own noise floor ----
 *
 * Per channel, over completed windows in stream order, k_s the first window after create or the last seek:
 *
 *   floor[k]   the extremum of metric[j], j in [max(k_s, k - M + 1), k] (window k included): the MINIMUM for OPEN_ABOVE (a carrier
 *              raises the metric, the idle level is the low side), the MAXIMUM for OPEN_BELOW.  A minimum-statistics estimate: it
 *              does not depend on the squelch state, so all floors of a call are computed in parallel.  A transmission longer
 *              than M windows drags it along, and the squelch closes.
 *   KEY        both senses run ONE sliding minimum: of metric for OPEN_ABOVE, of ~metric for OPEN_BELOW (the complement turns
 *              the order round); a window in front of k_s has the key UINT64_MAX, the minimum's identity.
 *   ratios     open_q8, close_q8 in 1/256.  metric * 256 against floor * q8 needs more than 64 bits (the metric reaches 2^61, a
 *              ratio 2^16): mfm_level_mul32 forms the exact product of a 64-bit and a 32-bit factor as top * 2^32 + low.
 *   open side  ABOVE: metric * 256 >= floor * open_q8 and metric >= open_thr;  BELOW: <= and <=.  False during the first
 *              warmup_windows windows after k_s.
 *   bad        ABOVE: metric * 256 < floor * close_q8 or metric < close_thr;  BELOW: > or >.
 *
 * The fixed thresholds of the config stay in force as absolute limits (a silent channel has floor 0, and every metric passes
 * the ratio test there).  Only the two predicates feed the state machine, which is mfm_level_squelch_step's.
 */
struct mfm_level_wide {
    uint64_t top;  /* the product >> 32 */
    uint32_t low;  /* its low 32 bits */
};

/* a * b exactly: b < 2^32 and, so that `top` cannot wrap, b <= 2^31 (the callers' factors are 256 and a ratio <= 65536) */
__host__ __device__ inline mfm_level_wide mfm_level_mul32(uint64_t a, uint32_t b)
{
    const uint64_t lo = (a & 0xffffffffull) * b, hi = (a >> 32) * b;
    mfm_level_wide w;
    w.top = hi + (lo >> 32);
    w.low = (uint32_t)lo;
    return w;
}

__host__ __device__ inline bool mfm_level_wide_ge(const mfm_level_wide &a, const mfm_level_wide &b)
{
    return a.top > b.top || (a.top == b.top && a.low >= b.low);
}

__host__ __device__ inline uint64_t mfm_level_floor_key(uint32_t below, uint64_t metric)
{
    return below ? ~metric : metric;
}

/* the two predicates of one window; warm: the window is one of the first warmup_windows */
__host__ __device__ inline void mfm_level_adaptive_predicates(uint32_t below, uint64_t metric, uint64_t floor, uint32_t open_q8, uint32_t close_q8,
                                                              uint64_t open_thr, uint64_t close_thr, bool warm, bool &on_open_side, bool &is_bad)
{
    const mfm_level_wide m = mfm_level_mul32(metric, 256u);
    const mfm_level_wide fo = mfm_level_mul32(floor, open_q8), fc = mfm_level_mul32(floor, close_q8);
    if (below) {
        on_open_side = !warm && mfm_level_wide_ge(fo, m) && metric <= open_thr;
        is_bad = !mfm_level_wide_ge(fc, m) || metric > close_thr;
    } else {
        on_open_side = !warm && mfm_level_wide_ge(m, fo) && metric >= open_thr;
        is_bad = !mfm_level_wide_ge(m, fc) || metric < close_thr;
    }
}

/* One step of the squelch on the two predicates: mfm_level_squelch_step itself, on a metric of 1 or 0 against thresholds of
 * 1 (closed, only "on the open side" is looked at: 1 >= 1 opens; open, only "bad": 0 < 1 is bad). */
__host__ __device__ inline void mfm_level_squelch_step_bits(uint32_t &open, uint32_t &bad, uint32_t hang, bool on_open_side, bool is_bad)
{
    const uint64_t metric = open ? (is_bad ? 0u : 1u) : (on_open_side ? 1u : 0u);
    mfm_level_squelch_step(open, bad, 0u, 1u, 1u, hang, metric);
}

#endif /* MFM_LEVEL_H */
