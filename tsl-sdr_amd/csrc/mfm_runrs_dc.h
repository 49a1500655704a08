/*
 * mfm_runrs_dc.h - the arithmetic of the burst resampler's DC blocker (mfm_runrs_set_dc_block, include/multifm_hip.h), stated
 * once for the kernel (rr_dc_kernel, mfm_runrs.hip) and for the host twin (mfm_hosttwin_runrs_dc_call) the CPU tests run: the
 * pole's fixed-point form, what a run starts from, one sample of the recurrence, and what a run leaves behind.
 *
 * filter/dc_blocker.h:80-90 per sample, in the reference's variables (int32, wrapping, p = (int16)((1 - pole) * 16384)):
 *     acc -= x_n_1;  x_n_1 = x << 14;  acc += x_n_1 - p * y_n_1;  y_n_1 = acc >> 14;  sample = (int16)y_n_1
 * With r = acc - x_n_1 (what is left of acc once the previous sample is taken out) that is
 *     r -= p * y_n_1;  acc = (x << 14) + r;  y_n_1 = acc >> 14
 * which is the form mfm_dc_block_kernel (mfm_resampler.hip) runs.  The carried y_n_1 is the unclipped value, |y_n_1| <= 2^17.
 */
#ifndef MFM_RUNRS_DC_H
#define MFM_RUNRS_DC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

/* filter/dc_blocker.h:56, the conversion mfm_resampler_create makes (mfm_rs_plan.h); false where that conversion is not
 * defined: a pole that is not a number, or whose (1 - pole) * 16384 does not fit the int16 it is cut to */
inline bool mfm_runrs_dc_pole(double pole, int32_t *p)
{
    const double v = (1.0 - pole) * 16384.0;
    if (!(v > -32769.0 && v < 32768.0)) {
        return false;
    }
    *p = (int16_t)v;
    return true;
}

/* a blocker between two samples: r = acc - x_n_1, and x_n_1 itself (Q30), which only the state that is left needs */
struct mfm_runrs_dc_carry {
    uint32_t r, xq;
    int32_t yp;
};

/* what a run starts from: its channel's state where it continues a stretch (the channel's first run of the call, with
 * MFM_RUNRS_BEGINS clear), a fresh blocker otherwise */
__host__ __device__ inline mfm_runrs_dc_carry mfm_runrs_dc_start(const mfm_runrs_dc_state *old, bool first_in_channel, uint32_t run_flags)
{
    mfm_runrs_dc_carry k;
    const bool cont = first_in_channel && 0u == (run_flags & MFM_RUNRS_BEGINS);
    k.xq = cont ? (uint32_t)old->x_n_1 : 0u;
    k.r = cont ? (uint32_t)old->acc - (uint32_t)old->x_n_1 : 0u;
    k.yp = cont ? old->y_n_1 : 0;
    return k;
}

/* one sample, singly (the kernel's 16-byte groups run the same three steps on packed words and set xq once per group) */
__host__ __device__ inline int16_t mfm_runrs_dc_sample(mfm_runrs_dc_carry &k, int32_t p, int16_t x)
{
    k.r -= (uint32_t)p * (uint32_t)k.yp;
    k.xq = (uint32_t)(int32_t)x << 14;
    k.yp = (int32_t)(k.xq + k.r) >> 14;
    return (int16_t)k.yp;
}

/* the state a run leaves; a run without outputs leaves exactly what it started from */
__host__ __device__ inline mfm_runrs_dc_state mfm_runrs_dc_leave(const mfm_runrs_dc_carry &k)
{
    mfm_runrs_dc_state s;
    s.x_n_1 = (int32_t)k.xq;
    s.y_n_1 = k.yp;
    s.acc = (int32_t)(k.xq + k.r);
    s.reserved = 0;
    return s;
}

#endif /* MFM_RUNRS_DC_H */
