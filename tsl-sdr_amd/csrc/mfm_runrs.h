/*
 * mfm_runrs.h - the arithmetic of the burst resampler (mfm_runrs_*, include/multifm_hip.h), stated once for the kernels
 * and for the host twin (mfm_hosttwin_runrs_call) the CPU tests run: whether a run of the gate continues its channel's
 * stretch, how many outputs it produces and what it leaves behind, and where a sample of the run lies.
 *
 * A run's input is the virtual stream "the channel's pending samples, then the run's payload samples": `pending` of the
 * first and nsamp = nr_windows * W of the second.  Output j of the run reads plen samples from position
 * floor((p0 + j D) / I) of that stream with the taps of phase (p0 + j D) % I, where p0 < I is the phase the stretch had
 * reached (filter/polyphase_fir.c:206-211 unrolled), and exists only while strictly more than plen samples are unconsumed
 * (polyphase_fir.c:184).
 */
#ifndef MFM_RUNRS_H
#define MFM_RUNRS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

#define MFM_RUNRS_NO_WINDOW (~0ull) /* `expected` of a channel that has no stretch to continue */

/* per-channel state between calls: struct mfm_runrs_state (include/multifm_hip.h); the pending samples stand beside it,
 * plen per channel, stored as received (inversion is applied on use) */

#ifndef MFM_RUN_POS_LIMIT
#define MFM_RUN_POS_LIMIT (1ull << 62) /* positions a stored state may hold stay below this, as the seek entries demand */
#endif

/*
 * What a state handed in from outside (mfm_runrs_store_state) must satisfy before a kernel reads it; NULL when it does, else a
 * message that names the field.  From what reads the state: mfm_runrs_plan_run needs phase < I (its numerator stays
 * non-negative) and pending <= plen (the state kernel copies `pending` samples of a channel's plen); outs + nr_out and
 * expected + nr_windows must not wrap; a channel without a stretch (expected = ~0) carries nothing.
 */
inline const char *mfm_runrs_state_check(const mfm_runrs_state &st, uint32_t I, uint32_t plen)
{
    if (st.expected == MFM_RUNRS_NO_WINDOW) {
        return st.outs || st.phase || st.pending ? "expected is ~0 (no stretch) but outs, phase or pending is not 0" : nullptr;
    }
    if (st.expected >= MFM_RUN_POS_LIMIT) {
        return "expected must be below 2^62 or ~0 (no stretch)";
    }
    if (st.outs >= MFM_RUN_POS_LIMIT) {
        return "outs must be below 2^62";
    }
    if (st.phase >= I) {
        return "phase must be below interpolate";
    }
    if (st.pending > plen) {
        return "pending must be at most the phase length";
    }
    return nullptr;
}

/* the DC blocker's state is wrapping arithmetic throughout: only the reserved word is constrained */
inline const char *mfm_runrs_dc_state_check(const mfm_runrs_dc_state &dc)
{
    return dc.reserved ? "the DC blocker's reserved must be 0" : nullptr;
}

/*
 * What one gate call can hand over, in windows and in runs, from the numbers of mfm_runrs_config (the run router,
 * mfm_runroute.hip, sizes itself by the same rule): max_windows and max_runs as given, and for a 0 the gate's own default.
 * false when a default is asked for and max_in_samples, which it is formed from, is 0.
 */
struct mfm_runrs_caps {
    uint64_t windows, runs;
};

inline bool mfm_runrs_caps_of(uint32_t nr_channels, uint32_t window_samples, uint32_t max_windows, uint32_t max_runs, uint32_t max_in_samples,
                              uint32_t preroll_windows, mfm_runrs_caps &c)
{
    const uint64_t max_win = max_in_samples ? (uint64_t)max_in_samples / window_samples + 1u : 0u;
    const uint64_t per_chan = max_win > preroll_windows ? max_win : preroll_windows; /* a flush emits up to P windows */
    if ((0 == max_windows || 0 == max_runs) && 0 == max_in_samples) {
        return false;
    }
    c.windows = max_windows ? max_windows : (uint64_t)nr_channels * per_chan;
    if (max_runs) {
        c.runs = max_runs;
    } else {
        const uint64_t most = (uint64_t)nr_channels * ((per_chan + 1u) / 2u); /* two runs of a channel have a closed window between them */
        c.runs = c.windows < most ? c.windows : most;
    }
    return true;
}

/* what a run starts from */
struct mfm_runrs_start {
    uint64_t first_out;
    uint32_t phase, pending;
    uint32_t begins; /* 1: a new stretch (fresh resampler) */
};

/* first_in_channel: the run is the channel's first of this call.  Only that one can continue: the gate's runs within a call
 * are maximal, so a later run of the channel has a closed window in front of it */
__host__ __device__ inline mfm_runrs_start mfm_runrs_start_of(const mfm_runrs_state &st, bool first_in_channel, uint64_t first_window)
{
    mfm_runrs_start s;
    const bool cont = first_in_channel && st.expected != MFM_RUNRS_NO_WINDOW && st.expected == first_window;
    s.first_out = cont ? st.outs : 0ull;
    s.phase = cont ? st.phase : 0u;
    s.pending = cont ? st.pending : 0u;
    s.begins = cont ? 0u : 1u;
    return s;
}

struct mfm_runrs_step {
    uint64_t nr_out;  /* outputs of the run */
    uint64_t pos_end; /* samples of the virtual stream consumed */
    uint32_t phase;   /* left behind */
    uint32_t pending; /* left behind: tot - pos_end, never more than plen */
};

/* The number of j >= 0 with floor((p0 + j D) / I) <= tot - plen - 1, in closed form: with M = tot - plen - 1 >= 0 that is
 * p0 + j D <= M I + I - 1, so j <= ((M + 1) I - 1 - p0) / D; p0 < I keeps the numerator non-negative.  The walk then stands
 * at t = p0 + nr_out D: position t / I >= M + 1, so at most plen samples stay pending; a ratio that mfm_rs_plan.h accepts
 * (ceil(D / I) <= plen) keeps the position at or below tot. */
__host__ __device__ inline mfm_runrs_step mfm_runrs_plan_run(uint32_t I, uint32_t D, uint32_t plen, uint32_t p0, uint32_t pending, uint64_t nsamp)
{
    mfm_runrs_step r;
    const uint64_t tot = (uint64_t)pending + nsamp;
    if (tot <= plen) {
        r.nr_out = 0;
        r.pos_end = 0;
        r.phase = p0;
        r.pending = (uint32_t)tot;
        return r;
    }
    r.nr_out = ((tot - plen) * I - 1u - p0) / D + 1u;
    const uint64_t t = p0 + r.nr_out * D;
    r.pos_end = t / I;
    r.phase = (uint32_t)(t - r.pos_end * I);
    r.pending = (uint32_t)(tot - r.pos_end);
    return r;
}

/* sample v of the run's virtual stream; outside it (the zero-padded taps of a phase read there) 0.  `invert` negates on
 * int16 storage (decoder/decoder.c:624) */
__host__ __device__ inline int16_t mfm_runrs_sample(const int16_t *pend, uint32_t pending, const int16_t *run, uint64_t nsamp, int64_t v, bool invert)
{
    int16_t s = 0;
    if (v >= 0 && v < (int64_t)pending) {
        s = pend[v];
    } else if (v >= (int64_t)pending && (uint64_t)(v - pending) < nsamp) {
        s = run[v - pending];
    }
    return invert ? (int16_t)(-s) : s;
}

/* ---- the bits form (mfm_runrs_process_bits_device): one predicate bit per output in the place of the int16 ---- */

/* words a run of nr_out outputs owns in the bits payload: output j is bit j % 32 of word out_offset + j / 32 */
__host__ __device__ inline uint32_t mfm_runrs_bit_words(uint32_t nr_out)
{
    return (nr_out + 31u) / 32u;
}

/* the predicate of the Q14-rounded output: sample < 0 (MFM_BITS_NEG) or sample > 0 (MFM_BITS_POS) */
__host__ __device__ inline bool mfm_runrs_bit(int16_t y, uint32_t polarity)
{
    return polarity == MFM_BITS_NEG ? y < 0 : y > 0;
}

#endif /* MFM_RUNRS_H */
