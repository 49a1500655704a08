/*
 * mfm_runmm.h - what the kernels of the burst Mueller-Muller stage (mfm_runmm_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runmm_call) must state once: the loop's parameters, what a run starts from, one decision of the loop, what a run
 * leaves behind and what a stored state must satisfy.  The checks a run has to pass before anything of the payload is read are
 * mfm_run_stage.h's.
 *
 * The position.  The reference keeps the position of the next decision as a float (cur_sample, pager/mueller_muller.c:56-66,
 * :96, :108-109).  It starts at 0 and only ever has floorf() of something added and the whole block length taken away, so it
 * holds whole numbers only, and it holds them exactly while block + one step stays below 2^23: with blocks of fewer than 2^22
 * samples and steps below 2^20 + 1 (the create condition) it always does.  (size_t)(cur_sample + 0.5f) is then cur_sample, and
 * "cur_sample < nr_samples_f" is "index < nr_samples": how the stretch was cut into blocks does not enter.  The stage therefore
 * keeps the position as an integer - next_offset in the state, an index into the run on the device - and w, m and last_sample
 * as the floats they are.
 */
#ifndef MFM_RUNMM_H
#define MFM_RUNMM_H

#include <hip/hip_runtime.h>
#include <cmath>
#include <math.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"

#define MFM_RUNMM_STAGING_UNIT 512u /* samples of a run the walk holds in LDS at a time (rm_walk_kernel, mfm_runmm.hip) */
#define MFM_RUNMM_MAX_STEP (1u << 21) /* no step reaches this: floor(m + w + km * x) < 1 + 2^20 (and 2^20 more for a stored m) */

/* the loop's constants, as mm_init takes them, and the shortest step any accepted configuration can take */
struct mfm_runmm_params {
    float kw, km, spb, error_min, error_max;
    uint32_t s;
};

/* mfm_mm_create's conditions; NULL when they hold, else what is wrong.  s = floor(error_min - |km| * 32768): rounding is
 * monotone, so w + km * x >= error_min - |km| * 32768 in float as it is in the reals, m >= 0 is added to it and floorf taken */
inline const char *mfm_runmm_params_check(float kw, float km, float spb, float error_min, float error_max, mfm_runmm_params *out)
{
    if (!std::isfinite(kw)) {
        return "kw must be finite";
    }
    if (!(error_max >= error_min)) {
        return "error_min must be at most error_max";
    }
    if (!(spb >= 1.0f) || !(spb < 1048576.0f)) {
        return "samples_per_bit must be at least 1 and below 2^20";
    }
    if (!(error_min - fabsf(km) * 32768.0f >= 1.0f)) {
        return "error_min - |km| * 32768 must be at least 1: a step that can fall below one sample never leaves the loop";
    }
    if (!(error_max + fabsf(km) * 32768.0f < 1048576.0f)) {
        return "error_max + |km| * 32768 must be below 2^20";
    }
    if (out) {
        out->kw = kw;
        out->km = km;
        out->spb = spb;
        out->error_min = error_min;
        out->error_max = error_max;
        out->s = (uint32_t)floorf(error_min - fabsf(km) * 32768.0f);
    }
    return nullptr;
}

/* decision slots of a run: decisions are at least s samples apart and all lie in [0, nr_out) */
__host__ __device__ inline uint32_t mfm_runmm_slots(uint32_t nr_out, uint32_t s)
{
    return nr_out / s + 1u;
}

/*
 * What a state handed in from outside (mfm_runmm_store_state) must satisfy before a kernel reads it; NULL when it does, else a
 * message that names the field.  From what the walk does with it: outs and stretch_window are positions; every decision but a
 * stretch's first follows a step of at least one sample, so decs <= outs; w is clamped before it is used and only has to be a
 * number; floorf(m + ...) is the step, at least 1 for m >= 0 and below MFM_RUNMM_MAX_STEP for m < 2^20 (m is samples_per_bit
 * before the first decision and a fraction afterwards); last_sample is a sample; next_offset is what is left of a step.
 */
inline const char *mfm_runmm_state_check(const mfm_runmm_state &st)
{
    if (st.has_stretch > 1u) {
        return "has_stretch must be 0 or 1";
    }
    if (!st.has_stretch) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&st);
        for (uint32_t i = 0; i < sizeof(st) / 4u; i++) {
            if (w[i]) {
                return "has_stretch is 0 but another field is not 0";
            }
        }
        return nullptr;
    }
    if (st.outs >= MFM_RUN_POS_LIMIT || st.stretch_window >= MFM_RUN_POS_LIMIT) {
        return "outs and stretch_window must be below 2^62";
    }
    if (st.decs > st.outs) {
        return "decs must be at most outs";
    }
    if (!std::isfinite(st.w)) {
        return "w must be finite";
    }
    if (!(st.m >= 0.0f && st.m < 1048576.0f)) {
        return "m must be at least 0 and below 2^20";
    }
    if (!(st.last_sample >= -32768.0f && st.last_sample <= 32767.0f) || st.last_sample != (float)(int32_t)st.last_sample) {
        return "last_sample must be a whole number an int16 holds";
    }
    if (st.next_offset >= MFM_RUNMM_MAX_STEP) {
        return "next_offset must be below 2^21";
    }
    if (st.reserved) {
        return "reserved must be 0";
    }
    return nullptr;
}

/* the loop between two decisions: the reference's w, m and last_sample, and sign(last_sample), which :76 takes again */
struct mfm_runmm_carry {
    float w, m, last_sample, last_sign;
};

__host__ __device__ inline float mfm_runmm_sign(float v) /* _mm_get_sign, :34-38 */
{
    return (float)(v > 0.0f) - (float)(v < 0.0f);
}

/* what a run starts from: its channel's state where it continues a stretch, mm_init's (:17-26) where it begins one */
__host__ __device__ inline mfm_runmm_state mfm_runmm_start(const mfm_runmm_state &old, const mfm_runrs_run &run, float spb)
{
    if (!(run.flags & MFM_RUNRS_BEGINS)) {
        return old;
    }
    mfm_runmm_state st;
    st.outs = 0;
    st.decs = 0;
    st.stretch_window = run.first_window;
    st.w = spb;
    st.m = spb;
    st.last_sample = 0.0f;
    st.next_offset = 0;
    st.has_stretch = 1;
    st.reserved = 0;
    return st;
}

/*
 * One decision on sample x (:66-101): returns the whole-sample distance to the next one.  The float operations are the
 * reference's in the reference's order - mul, mul, sub; mul, add; clamp; mul, add, add; floorf; sub - and this file is compiled
 * without contraction on both sides.  w is finite and error_min <= error_max, so the median of three is the if / else if of
 * :86-90.
 */
__host__ __device__ inline uint32_t mfm_runmm_step(mfm_runmm_carry &k, const mfm_runmm_params &P, int32_t x)
{
    const float sample = (float)x;
    const float sc = (float)(x > 0 ? 1 : (x < 0 ? -1 : 0));           /* _mm_get_sign(sample) */
    const float w_error = k.last_sign * sample - sc * k.last_sample;  /* :76 */
    const float w1 = k.w + w_error * P.kw;                            /* :79 */
#if defined(__HIP_DEVICE_COMPILE__)
    k.w = __builtin_amdgcn_fmed3f(w1, P.error_min, P.error_max);      /* :86-90 */
#else
    k.w = P.error_min > w1 ? P.error_min : (P.error_max < w1 ? P.error_max : w1);
#endif
    k.m += k.w + P.km * sample;                                       /* :92 */
    const float fl = floorf(k.m);
    k.m -= fl;                                                        /* :97 */
    k.last_sample = sample;                                           /* :100 */
    k.last_sign = sc;
    return (uint32_t)fl;                                              /* :95 */
}

/* the state a run of nr_out outputs leaves: idx is where the walk stopped (>= nr_out), nr_dec what it decided */
__host__ __device__ inline void mfm_runmm_leave(mfm_runmm_state &st, const mfm_runmm_carry &k, uint32_t idx, uint32_t nr_out, uint32_t nr_dec)
{
    st.w = k.w;
    st.m = k.m;
    st.last_sample = k.last_sample;
    st.next_offset = idx - nr_out;
    st.outs += nr_out;
    st.decs += nr_dec;
    st.has_stretch = 1;
    st.reserved = 0;
}

#endif /* MFM_RUNMM_H */
