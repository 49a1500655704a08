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

#endif /* MFM_RUNROUTE_H */
