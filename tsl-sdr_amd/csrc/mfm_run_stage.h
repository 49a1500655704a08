/*
 * mfm_run_stage.h - what the four burst stages behind the burst resampler (mfm_runais_*, mfm_runpocsag_*, mfm_runflex_*,
 * mfm_runmm_*, include/multifm_hip.h) state once: the rule a run has to pass before anything of the payload is read, the
 * one-block scan their plan, scan and place kernels are built on, the head of a plan kernel, and the host code around a call
 * that does not depend on what a stage decodes: leaving a message, the create-time bounds, the messages of a refused call, the
 * host twin's plan pass, the order of calls on streams and the state entries.
 *
 * Plain inline functions and duck-typed templates, as mfm_run_ends.h: every kernel stays in its stage's own object under its
 * own name and hands its arrays to the functions below; the walk, slice, match and state kernels are the stages' alone.  Obj
 * is a stage's object: cfg, have_call, last_stream, d_chan[2], cur.
 */
#ifndef MFM_RUN_STAGE_H
#define MFM_RUN_STAGE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/multifm_hip.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);

constexpr uint32_t MFM_RUN_SCAN_THREADS = 1024; /* the one block of a plan, scan or place kernel */
constexpr uint32_t MFM_RUN_NONE = 0xffffffffu;  /* d_chan_last: the channel has no run in this call */
constexpr uint32_t MFM_RUN_RS_RUNS = 0, MFM_RUN_RS_ELEMS = 1, MFM_RUN_RS_OVERFLOW = 2, MFM_RUN_RS_GATE = 3; /* the resampler's totals */
constexpr uint32_t MFM_RUN_T_OVERFLOW = 2, MFM_RUN_T_INPUT = 3; /* d_totals[] of every stage; [0] and [1] are the stage's own */
constexpr uint64_t MFM_RUN_MAX_RUNS = 1ull << 28, MFM_RUN_MAX_OUT = 1ull << 31; /* per call: segment words and slots stay below 2^32 */
#define MFM_RUN_POS_LIMIT (1ull << 62) /* positions a stored state may hold stay below this, as the seek entries demand */

/* the flags the shared code raises; the stages keep their public names for them */
constexpr uint32_t MFM_RUN_IN_RUNRS = 1u, MFM_RUN_IN_OUT_OF_STEP = 2u, MFM_RUN_IN_BAD_RUNS = 4u, MFM_RUN_OVER_RUNS = 1u;
#define MFM_RUN_SAME_FLAG(name)                                                                                          \
    static_assert(MFM_RUNAIS_##name == MFM_RUN_##name && MFM_RUNPOCSAG_##name == MFM_RUN_##name &&                     \
                      MFM_RUNFLEX_##name == MFM_RUN_##name && MFM_RUNMM_##name == MFM_RUN_##name,                       \
                  "the burst stages share the value of " #name)
MFM_RUN_SAME_FLAG(IN_RUNRS);
MFM_RUN_SAME_FLAG(IN_OUT_OF_STEP);
MFM_RUN_SAME_FLAG(IN_BAD_RUNS);
MFM_RUN_SAME_FLAG(OVER_RUNS);
#undef MFM_RUN_SAME_FLAG

/* ---- host and device ------------------------------------------------------------------------------------------------ */

/*
 * The input-error flags of run `run` (0: it may be read).  prev: the run in front of it in the list (NULL for the first),
 * nr_elems: the resampler's total of output elements, state: the per-channel state the call started from.  words: the
 * resampler's bits form (AIS and POCSAG), where out_offset and nr_elems count 32-bit words and the run owns (nr_out + 31) / 32
 * of them.
 */
template <class State>
__host__ __device__ inline uint32_t mfm_run_check_run(const mfm_runrs_run &run, const mfm_runrs_run *prev, uint32_t nr_channels,
                                                      uint64_t nr_elems, const State *state, bool words = false)
{
    const uint64_t owned = words ? ((uint64_t)run.nr_out + 31u) / 32u : run.nr_out;
    if (run.channel >= nr_channels || (prev && prev->channel > run.channel) || run.out_offset > nr_elems ||
        owned > nr_elems - run.out_offset) {
        return MFM_RUN_IN_BAD_RUNS;
    }
    if (run.flags & MFM_RUNRS_BEGINS) {
        return run.first_out != 0 ? MFM_RUN_IN_BAD_RUNS : 0u;
    }
    /* only a channel's first run of a call can continue: a later one has a closed window in front of it */
    const bool first = !prev || prev->channel != run.channel;
    const State &st = state[run.channel];
    return first && st.has_stretch && st.outs == run.first_out ? 0u : MFM_RUN_IN_OUT_OF_STEP;
}

/* what the resampler's totals say before a run is read: the call's runs and elements, and the flags of a call of which nothing
 * may be read.  cap_elems: what the payload may hold in the form it has (the bits form allows cap_out / 32 + cap_runs words) */
__host__ __device__ inline void mfm_run_totals_check(const uint64_t *rtotals, uint64_t cap_elems, uint64_t cap_runs, uint64_t *n,
                                                     uint64_t *E, uint64_t *over, uint64_t *err)
{
    *n = rtotals[MFM_RUN_RS_RUNS];
    *E = rtotals[MFM_RUN_RS_ELEMS];
    *over = *err = 0;
    if (rtotals[MFM_RUN_RS_OVERFLOW] || rtotals[MFM_RUN_RS_GATE]) {
        *err = MFM_RUN_IN_RUNRS;
    } else if (*E > cap_elems) {
        *err = MFM_RUN_IN_BAD_RUNS;
    } else if (*n > cap_runs) {
        *over = MFM_RUN_OVER_RUNS;
    }
}

/* ---- device --------------------------------------------------------------------------------------------------------- */

/* scan over the block (1024 threads); returns this thread's EXCLUSIVE prefix, *total = the block's sum */
__device__ __forceinline__ uint64_t mfm_run_block_scan(uint64_t v, uint64_t *lds, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)inc, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), o);
        if (lane >= (uint32_t)o) {
            inc += ((uint64_t)hi << 32) | lo;
        }
    }
    if (lane == 63) {
        lds[wave] = inc;
    }
    __syncthreads();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < MFM_RUN_SCAN_THREADS / 64; i++) {
        const uint64_t t = lds[i];
        base += i < wave ? t : 0u;
        all += t;
    }
    __syncthreads();
    *total = all;
    return base + inc - v;
}

/* this thread's slice [*r0, *r1) of a list of n the block's 1024 threads share: ceil(n / 1024) entries each */
template <class T>
__device__ __forceinline__ void mfm_run_slice(T n, T *r0, T *r1)
{
    const T per = (n + MFM_RUN_SCAN_THREADS - 1) / MFM_RUN_SCAN_THREADS;
    *r0 = threadIdx.x * per < n ? threadIdx.x * per : n;
    *r1 = *r0 + per < n ? *r0 + per : n;
}

/* the head of a plan kernel: mfm_run_totals_check; false when nothing may be read, with the zeroed totals, the flags and the
 * nr_ctl zeroed control words written */
__device__ __forceinline__ bool mfm_run_plan_head(const uint64_t *rtotals, uint64_t cap_elems, uint64_t cap_runs, uint64_t *totals,
                                                  uint32_t *ctl, uint32_t nr_ctl, uint64_t *n, uint64_t *E, uint64_t *over, uint64_t *err)
{
    mfm_run_totals_check(rtotals, cap_elems, cap_runs, n, E, over, err);
    if (*over || *err) {
        if (threadIdx.x == 0) {
            totals[0] = 0;
            totals[1] = 0;
            totals[MFM_RUN_T_OVERFLOW] = *over;
            totals[MFM_RUN_T_INPUT] = *err;
            for (uint32_t i = 0; i < nr_ctl; i++) {
                ctl[i] = 0;
            }
        }
        return false;
    }
    return true;
}

/* one block: the n counts into their exclusive scan; returns the total */
__device__ __forceinline__ uint64_t mfm_run_count_scan(const uint32_t *count, uint32_t *base_of, uint64_t n, uint64_t *lds)
{
    uint64_t r0, r1;
    mfm_run_slice(n, &r0, &r1);
    uint64_t s = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        s += count[r];
    }
    uint64_t total;
    uint64_t base = mfm_run_block_scan(s, lds, &total);
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        base_of[r] = (uint32_t)base;
        base += count[r];
    }
    return total;
}

/* one workgroup: a run's *count records of `each` words from its slot range into the dense list */
__device__ __forceinline__ void mfm_run_copy_words(const uint32_t *src, uint32_t *dst, const uint32_t *count, uint32_t each)
{
    for (uint32_t i = threadIdx.x; i < *count * each; i += blockDim.x) {
        dst[i] = src[i];
    }
}

/* ---- host ----------------------------------------------------------------------------------------------------------- */

inline int mfm_run_fail(int code, const char *msg)
{
    mfm_internal_set_error(msg);
    return code;
}

inline int mfm_run_hip_failed(const char *what, hipError_t e)
{
    char msg[256];
    snprintf(msg, sizeof(msg), "%s failed: %s", what, hipGetErrorString(e));
    mfm_internal_set_error(msg);
    return e == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;
}

#define MFM_RUN_TRY(expr)                                                                                    \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            return mfm_run_hip_failed(#expr, err_);                                                          \
        }                                                                                                    \
    } while (0)

/* what every stage's create checks without a device, in front of its own conditions and capacity defaults */
template <class Cfg>
inline int mfm_run_geometry(const Cfg &cfg)
{
    if (cfg.abi_version != MFM_ABI_VERSION) {
        return mfm_run_fail(MFM_E_INVAL, "abi_version is not MFM_ABI_VERSION");
    }
    if (0 == cfg.nr_channels) {
        return mfm_run_fail(MFM_E_INVAL, "nr_channels must be at least 1");
    }
    if (0 == cfg.max_runs || 0 == cfg.max_out_samples || cfg.max_runs >= MFM_RUN_MAX_RUNS || cfg.max_out_samples >= MFM_RUN_MAX_OUT) {
        return mfm_run_fail(MFM_E_INVAL, "max_runs must be 1 .. 2^28 - 1 and max_out_samples 1 .. 2^31 - 1: the burst resampler's capacities (mfm_runrs_get_capacity)");
    }
    if (cfg.flags != 0) {
        return mfm_run_fail(MFM_E_INVAL, "flags must be 0");
    }
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it; own: the stage's, of its own capacity */
inline const char *mfm_run_refusal(uint64_t over, uint64_t err, const char *own)
{
    if (err & MFM_RUN_IN_RUNRS) {
        return "the burst resampler's call raised overflow or gate error";
    }
    if (err & MFM_RUN_IN_BAD_RUNS) {
        return "the run list is not a burst resampler's: a run names a channel or an output range that does not exist, or more than max_out_samples";
    }
    if (err & MFM_RUN_IN_OUT_OF_STEP) {
        return "out of step with the burst resampler: a continuing run does not follow on its channel's stretch";
    }
    if (over & MFM_RUN_OVER_RUNS) {
        return "the call has more runs than max_runs";
    }
    return own;
}

/*
 * The host twin's plan pass: the totals, then every run (mfm_run_check_run) and the sum of the outputs; slots(nr_out) is called
 * for every run of a list that may be read, for the stage's own sums, which it holds against its capacities afterwards (they stay
 * 0 where the totals refuse the call).  false: a list or a payload that is needed is missing (MFM_E_INVAL).
 */
template <class State, class Slots>
inline bool mfm_run_twin_plan(const uint64_t *totals, uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, const State *state,
                              const mfm_runrs_run *runs, const void *payload, bool words, Slots slots, uint64_t *n, uint64_t *over,
                              uint64_t *err)
{
    uint64_t E;
    mfm_run_totals_check(totals, words ? (uint64_t)max_out_samples / 32u + max_runs : (uint64_t)max_out_samples, max_runs, n, &E, over, err);
    if (*over || *err) {
        return true;
    }
    if ((*n && !runs) || (E && !payload)) {
        return false;
    }
    uint64_t to = 0;
    for (uint64_t r = 0; r < *n; r++) {
        *err |= mfm_run_check_run(runs[r], r ? &runs[r - 1] : nullptr, nr_channels, E, state, words);
        to += runs[r].nr_out;
        slots(runs[r].nr_out);
    }
    if (to > max_out_samples) {
        *err |= MFM_RUN_IN_BAD_RUNS;
    }
    return true;
}

/* ... and how the twin leaves a refused call: the flags as the device's totals hold them, the message, MFM_E_STATE */
inline int mfm_run_twin_refuse(uint64_t over, uint64_t err, uint32_t *flags, const char *why)
{
    if (flags) {
        *flags = (uint32_t)(over | (err << 8));
    }
    return mfm_run_fail(MFM_E_STATE, why);
}

/* a process call in front of its launches: the device, and the stream order (state lives on the device; keep calls ordered) */
template <class Obj>
inline int mfm_run_call_begin(Obj *o, hipStream_t s)
{
    MFM_RUN_TRY(hipSetDevice(o->cfg.device));
    if (o->have_call && o->last_stream != s) {
        MFM_RUN_TRY(hipStreamSynchronize(o->last_stream));
    }
    return MFM_OK;
}

/* ... and behind them: the call wrote d_chan[cur ^ 1], which the next one reads */
template <class Obj>
inline void mfm_run_call_end(Obj *o, hipStream_t s)
{
    o->cur ^= 1u;
    o->last_stream = s;
    o->have_call = true;
}

/* mfm_hosttwin_run*_state_check: check(state) is the stage's rule (NULL or what is wrong), noun its name in the message */
template <class State, class Check>
inline int mfm_run_state_check(uint32_t nr_channels, const State *state, const char *noun, Check check)
{
    if (!state || !nr_channels) {
        return MFM_E_INVAL;
    }
    for (uint32_t c = 0; c < nr_channels; c++) {
        if (const char *why = check(state[c])) {
            char msg[224];
            snprintf(msg, sizeof(msg), "burst %s state, channel %u: %s", noun, c, why);
            return mfm_run_fail(MFM_E_INVAL, msg);
        }
    }
    return MFM_OK;
}

/* the per-channel states the next process call reads, once the queued work has run */
template <class Obj, class State>
inline int mfm_run_fetch_state(Obj *o, State *state, size_t nr_channels)
{
    if (!o || !state || nr_channels != o->cfg.nr_channels) {
        return MFM_E_INVAL;
    }
    MFM_RUN_TRY(hipSetDevice(o->cfg.device));
    if (o->have_call) {
        MFM_RUN_TRY(hipStreamSynchronize(o->last_stream));
    }
    MFM_RUN_TRY(hipMemcpy(state, o->d_chan[o->cur], nr_channels * sizeof(State), hipMemcpyDeviceToHost));
    return MFM_OK;
}

/* ... and put in their place; check: the stage's mfm_hosttwin_run*_state_check, before a kernel reads them */
template <class Obj, class State, class Check>
inline int mfm_run_store_state(Obj *o, const State *state, size_t nr_channels, Check check)
{
    if (!o || !state || nr_channels != o->cfg.nr_channels) {
        return MFM_E_INVAL;
    }
    const int ok = check(o->cfg.nr_channels, state);
    if (ok != MFM_OK) {
        return ok;
    }
    MFM_RUN_TRY(hipSetDevice(o->cfg.device));
    if (o->have_call) {
        MFM_RUN_TRY(hipStreamSynchronize(o->last_stream));
    }
    MFM_RUN_TRY(hipMemcpy(o->d_chan[o->cur], state, nr_channels * sizeof(State), hipMemcpyHostToDevice));
    return MFM_OK;
}

#endif /* MFM_RUN_STAGE_H */
