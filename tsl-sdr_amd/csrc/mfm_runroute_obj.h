/*
 * mfm_runroute_obj.h - the run router's object, shared by its three objects: mfm_runroute.hip (create from a route table, the
 * zero-copy partition kernel and the accessors), mfm_runroute_sets.hip (create from a table of route sets, the partition
 * kernel of that form and the pack copy) and mfm_runroute_local.hip (mfm_runroute_create_local: route-local channel numbers on
 * the gate's payload in place, its partition kernel).  Private to the library.
 */
#ifndef MFM_RUNROUTE_OBJ_H
#define MFM_RUNROUTE_OBJ_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

struct mfm_runroute {
    mfm_runroute_config cfg{};
    uint64_t cap_runs = 0;
    uint8_t *d_table = nullptr;
    mfm_gate_run *d_runs = nullptr; /* [K][cap_runs] */
    uint64_t *d_totals = nullptr;   /* [K][4] */
    const int16_t *d_payload = nullptr; /* the last call's: the gate's */
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    /* the sets form (mfm_runroute_create_sets) */
    bool sets = false, pack = false;
    uint8_t *h_table = nullptr;     /* [C] the sets, for mfm_runroute_route_channels */
    uint32_t nr_of[MFM_RUNROUTE_MAX_ROUTES] = { 0 };       /* channels of route k */
    /* the local form (mfm_runroute_create_local): sets is true as well, d_rank and d_caps are PACK's */
    bool local = false;
    uint64_t *d_bound = nullptr;    /* [1] the gate's payload elements of the last call, 0 for a refused one */
    /* PACK and the local form */
    uint64_t cap_route_runs[MFM_RUNROUTE_MAX_ROUTES] = { 0 };    /* what mfm_runroute_route_caps returns */
    uint64_t cap_route_windows[MFM_RUNROUTE_MAX_ROUTES] = { 0 };
    uint64_t pack_base[MFM_RUNROUTE_MAX_ROUTES + 1] = { 0 };     /* route k's payload within d_pack, in elements, multiples of 8 */
    uint32_t tile_base[MFM_RUNROUTE_MAX_ROUTES + 1] = { 0 };     /* route k's first workgroup of the copy kernel */
    uint32_t *d_rank = nullptr;     /* [C][K] route-local channel numbers; the local form too */
    uint64_t *d_caps = nullptr;     /* [K][2] cap_route_runs, cap_route_windows; the local form too */
    uint64_t *d_src = nullptr;      /* [K][cap_runs] the gate's payload_offset of each routed run */
    int16_t *d_pack = nullptr;      /* the routes' dense payloads */
};

/* mfm_runroute_sets.hip: the call of an object made by mfm_runroute_create_sets, and what its destroy frees besides */
extern "C" __attribute__((visibility("hidden"))) int mfm_runroute_sets_process(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs,
                                                                              const int16_t *d_payload, const uint64_t *d_totals, hipStream_t s);
extern "C" __attribute__((visibility("hidden"))) void mfm_runroute_sets_free(struct mfm_runroute *rt);
/* mfm_runroute_sets.hip: what mfm_runroute_create_sets checks and derives under MFM_RUNROUTE_F_PACK, for the local form, which
 * refuses the same and sizes its routes by the same rule: cfg->flags must be 0 here.  NULL, or the message (err is room for it);
 * nr_of, route_runs and route_windows are [MFM_RUNROUTE_MAX_ROUTES] */
extern "C" __attribute__((visibility("hidden"))) const char *mfm_runroute_local_geometry(const struct mfm_runroute_config *cfg,
                                                                                        const uint8_t *routes_of_channel, uint64_t *cap_runs,
                                                                                        uint32_t *nr_of, uint64_t *route_runs,
                                                                                        uint64_t *route_windows, char *err, size_t cap);
/* mfm_runroute_local.hip: the call of an object made by mfm_runroute_create_local */
extern "C" __attribute__((visibility("hidden"))) int mfm_runroute_local_process(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs,
                                                                               const int16_t *d_payload, const uint64_t *d_totals, hipStream_t s);

#endif /* MFM_RUNROUTE_OBJ_H */
