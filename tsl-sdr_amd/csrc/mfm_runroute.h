/*
 * mfm_runroute.h - the arithmetic of the run router (mfm_runroute_*, include/multifm_hip.h), stated once for the kernel and
 * for the host twin (mfm_hosttwin_runroute_call) the CPU tests run: which route a run of the gate belongs to, and when a call
 * is refused and with which flags.  The partition itself is a stable one: route k's list is the gate's runs whose channel has
 * route k, in the gate's order.
 */
#ifndef MFM_RUNROUTE_H
#define MFM_RUNROUTE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_runrs.h"

/* d_totals[], the gate's and each route's */
#define MFM_RUNROUTE_T_RUNS 0
#define MFM_RUNROUTE_T_ELEMS 1
#define MFM_RUNROUTE_T_OVERFLOW 2
#define MFM_RUNROUTE_T_OUT_OF_STEP 3

/* a run that names a channel the table does not have is not a gate's run: the call is refused (out of step) */
__host__ __device__ inline bool mfm_runroute_bad_channel(uint32_t channel, uint32_t nr_channels)
{
    return channel >= nr_channels;
}

/* the route of a run's channel: the table's byte, MFM_ROUTE_NONE for a channel that does not exist */
__host__ __device__ inline uint32_t mfm_runroute_of(const uint8_t *route_of_channel, uint32_t nr_channels, uint32_t channel)
{
    return mfm_runroute_bad_channel(channel, nr_channels) ? MFM_ROUTE_NONE : route_of_channel[channel];
}

/* what can be told from the gate's totals alone: its own flags are passed on as 0 / 1, and a call with more runs than the
 * router holds is an overflow.  true: the call is refused, every route gets these two flags with 0 runs and 0 elements */
__host__ __device__ inline bool mfm_runroute_refused(const uint64_t *gate_totals, uint64_t cap_runs, uint64_t &overflow, uint64_t &out_of_step)
{
    overflow = gate_totals[MFM_RUNROUTE_T_OVERFLOW] ? 1u : 0u;
    out_of_step = gate_totals[MFM_RUNROUTE_T_OUT_OF_STEP] ? 1u : 0u;
    if (!overflow && !out_of_step && gate_totals[MFM_RUNROUTE_T_RUNS] > cap_runs) {
        overflow = 1u;
    }
    return overflow || out_of_step;
}

/*
 * ---- the sets form (mfm_runroute_create_sets): a channel's byte is a SET of routes, bit k = route k; under
 * MFM_RUNROUTE_F_PACK each route gets route-local channel numbers, dense offsets and a payload of its own.  Stated once for
 * the kernels of mfm_runroute_sets.hip and for mfm_hosttwin_runroute_sets_call.
 */

/* the routes of a run's channel: the table's byte, the empty set for a channel that does not exist */
__host__ __device__ inline uint32_t mfm_runroute_set_of(const uint8_t *routes_of_channel, uint32_t nr_channels, uint32_t channel)
{
    return mfm_runroute_bad_channel(channel, nr_channels) ? 0u : routes_of_channel[channel];
}

__host__ __device__ inline bool mfm_runroute_in_route(uint32_t set, uint32_t route)
{
    return ((set >> route) & 1u) != 0;
}

/* Route-local channel numbers: the rank of channel c in route k is the number of channels below c whose set has bit k, so a
 * route's local numbers ascend with the global ones.  The ranks of all channels stand in one table [nr_channels][nr_routes],
 * built once per object by mfm_runroute_build_ranks (count[k] = the route's channels) and read by mfm_runroute_rank_of. */
inline void mfm_runroute_build_ranks(const uint8_t *routes_of_channel, uint32_t nr_channels, uint32_t nr_routes, uint32_t *rank, uint32_t *count)
{
    for (uint32_t k = 0; k < nr_routes; k++) {
        count[k] = 0;
    }
    for (uint32_t c = 0; c < nr_channels; c++) {
        for (uint32_t k = 0; k < nr_routes; k++) {
            rank[(size_t)c * nr_routes + k] = count[k];
            count[k] += mfm_runroute_in_route(routes_of_channel[c], k) ? 1u : 0u;
        }
    }
}

__host__ __device__ inline uint32_t mfm_runroute_rank_of(const uint32_t *rank, uint32_t nr_routes, uint32_t channel, uint32_t route)
{
    return rank[(size_t)channel * nr_routes + route];
}

/* PACK copies a run's windows, so a run whose payload range does not lie within the gate's payload elements is not a gate's
 * run: the call is refused (out of step), as a bad channel is.  Written so that nothing wraps. */
__host__ __device__ inline bool mfm_runroute_bad_range(uint64_t payload_offset, uint32_t nr_windows, uint32_t window_samples, uint64_t gate_elems)
{
    const uint64_t len = (uint64_t)nr_windows * window_samples; /* < 2^52 */
    return payload_offset > gate_elems || len > gate_elems - payload_offset;
}

/* PACK: a route whose runs or windows of one call exceed the capacities mfm_runroute_route_caps gives for it gets overflow = 1
 * with 0 runs and 0 elements; the other routes are unaffected */
__host__ __device__ inline bool mfm_runroute_route_over(uint64_t runs, uint64_t windows, uint64_t cap_runs, uint64_t cap_windows)
{
    return runs > cap_runs || windows > cap_windows;
}

/*
 * What mfm_runroute_route_caps returns under PACK for a route of n channels (n >= 1): mfm_runrs_caps_of applied to n, never
 * above an explicit max_windows / max_runs.  With max_in_samples == 0 there is no default to form and both must be explicit:
 * they are returned as given.  false: max_in_samples is 0 and one of the two is 0.
 */
inline bool mfm_runroute_pack_caps(uint32_t n, uint32_t window_samples, uint32_t max_windows, uint32_t max_runs, uint32_t max_in_samples,
                                   uint32_t preroll_windows, mfm_runrs_caps &c)
{
    if (0 == max_in_samples) {
        c.windows = max_windows;
        c.runs = max_runs;
        return max_windows && max_runs;
    }
    mfm_runrs_caps own;
    (void)mfm_runrs_caps_of(n, window_samples, 0u, 0u, max_in_samples, preroll_windows, own);
    c.windows = max_windows && max_windows < own.windows ? max_windows : own.windows;
    (void)mfm_runrs_caps_of(n, window_samples, (uint32_t)(c.windows < 0xffffffffull ? c.windows : 0xffffffffull), 0u, max_in_samples,
                            preroll_windows, own);
    c.runs = max_runs && max_runs < own.runs ? max_runs : own.runs;
    return true;
}

/*
 * ---- the local form (mfm_runroute_create_local): PACK's route-local channel numbers, capacities and per-route overflow on the
 * gate's payload in place.  The set lookup, the rank, mfm_runroute_route_over and mfm_runroute_pack_caps above are its rules
 * too; a payload range is not looked at (nothing is copied: it is the burst resampler's view entry that checks it, against the
 * bound the router hands on).  Stated once for the kernel of mfm_runroute_local.hip and for mfm_hosttwin_runroute_local_call.
 */

/* the kernel's form of a routed record's channel: the record's third 64-bit word (channel | nr_windows << 32) with the channel
 * replaced by its rank in the route */
__host__ __device__ inline uint64_t mfm_runroute_local_word(uint64_t word, uint32_t local_channel)
{
    return (word & 0xffffffff00000000ull) | local_channel;
}

/* a route's load, its totals' elements: the windows of its records times W; below 2^52 for a route within its capacity */
__host__ __device__ inline uint64_t mfm_runroute_load(uint64_t windows, uint32_t window_samples)
{
    return windows * window_samples;
}

/* the bound the router hands to the burst resampler's view entry: the gate's payload elements, 0 for a call refused for the
 * whole router */
__host__ __device__ inline uint64_t mfm_runroute_bound(bool refused, uint64_t gate_elems)
{
    return refused ? 0u : gate_elems;
}

#endif /* MFM_RUNROUTE_H */
