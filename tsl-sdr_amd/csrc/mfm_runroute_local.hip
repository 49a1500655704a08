/*
 * mfm_runroute_local.hip - the run router's local form (mfm_runroute_create_local): route-local channel numbers, as under
 * MFM_RUNROUTE_F_PACK, on the gate's payload IN PLACE.  payload_offset stays the gate's, nothing is copied, and every route
 * reports its own load, so that a burst resampler sized to the route reads the gate's payload through its view entry
 * (mfm_runrs_process_view_device) with the bound this router hands on.  See include/multifm_hip.h for the boundary and
 * mfm_runroute.h for the arithmetic.  An object of its own, as mfm_runroute_sets.hip is, so that every other object keeps the
 * kernels it had; the router's struct is shared through mfm_runroute_obj.h.
 *
 *   rt_local_kernel  the strip walk of rt_sets_kernel: ONE workgroup of 1024 lanes, one lane per run, strips of 1024 runs in
 *                    order.  A lane reads its run and its channel's set; for each route k the wave ballots bit k of the set,
 *                    the lane's rank within the wave is the count of set bits below it, the wave counts go through LDS and
 *                    lanes 0 .. K - 1 turn them into exclusive offsets from the route's running base.  A lane then writes its
 *                    record once per route it is in, with the channel's rank in the route (a table lookup) and nothing else
 *                    changed.  The route's load needs a SUM of nr_windows, not a prefix (no offset is rewritten): every lane
 *                    keeps a 64-bit sum per route over all its strips, and once behind the walk a wave reduction per route
 *                    and the 16 wave sums in LDS give the route's windows.  At the end lanes 0 .. K - 1 write their route's
 *                    totals - a route over its own capacity gets overflow alone - and lane 0 stores the bound.
 *
 * No float, no atomics, no scratch, no host synchronisation: counts are read on the device.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/multifm_hip.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);
#include "mfm_runroute.h"
#include "mfm_runroute_obj.h"
#include "mfm_runrs.h"

namespace {

constexpr uint32_t RL_THREADS = 1024, RL_WAVES = RL_THREADS / 64u, RL_K = MFM_RUNROUTE_MAX_ROUTES;

static_assert(sizeof(mfm_gate_run) == 24 && offsetof(mfm_gate_run, channel) == 16, "the kernel copies a run as three 64-bit words");
static_assert(RL_K <= 8, "a channel's set is one byte");

struct RlCall {
    const mfm_gate_run *gruns;
    const uint64_t *gtotals;
    const uint8_t *table;  /* [C] sets */
    const uint32_t *rank;  /* [C][K] */
    const uint64_t *caps;  /* [K][2] runs, windows a route may carry */
    mfm_gate_run *runs;    /* [K][cap_runs] */
    uint64_t *totals;      /* [K][4] */
    uint64_t *bound;       /* [1] */
    uint64_t cap_runs;
    uint32_t C, K, W;
};

/* the sum over the wave's lanes, in every lane */
__device__ __forceinline__ uint64_t rl_wave_total(uint64_t v)
{
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        v += __shfl_xor(v, d, 64);
    }
    return v;
}

__global__ __launch_bounds__(RL_THREADS) void rt_local_kernel(const RlCall A)
{
    __shared__ uint32_t s_cnt[2][RL_K][RL_WAVES];
    __shared__ uint64_t s_win[RL_K][RL_WAVES];
    __shared__ uint32_t s_bad[RL_WAVES];
    __shared__ uint32_t s_cap[RL_K]; /* the routes' own run capacities, below 2^31; read behind a strip's barriers */
    const uint32_t tid = threadIdx.x, wave = tid / 64u, lane = tid % 64u;
    uint64_t cap_r = 0, cap_w = 0; /* lanes 0 .. K - 1: the route's own capacities, read once, beside the gate's totals */
    if (tid < A.K) {
        cap_r = A.caps[2u * tid];
        cap_w = A.caps[2u * tid + 1u];
        s_cap[tid] = (uint32_t)cap_r;
    }
    uint64_t over, oos;
    if (mfm_runroute_refused(A.gtotals, A.cap_runs, over, oos)) {
        if (tid < A.K) {
            uint64_t *t = A.totals + 4u * tid;
            t[MFM_RUNROUTE_T_RUNS] = 0;
            t[MFM_RUNROUTE_T_ELEMS] = 0;
            t[MFM_RUNROUTE_T_OVERFLOW] = over;
            t[MFM_RUNROUTE_T_OUT_OF_STEP] = oos;
        }
        if (tid == 0) {
            *A.bound = mfm_runroute_bound(true, 0u);
        }
        return;
    }
    const uint64_t n = A.gtotals[MFM_RUNROUTE_T_RUNS]; /* <= cap_runs < 2^31 */
    uint32_t base = 0;     /* lanes 0 .. K - 1: runs of route tid in the strips so far */
    uint64_t wsum[RL_K];   /* windows of this lane's runs in route k: fewer than 2^21 strips of less than 2^32 windows */
#pragma unroll
    for (uint32_t k = 0; k < RL_K; k++) {
        wsum[k] = 0;
    }
    int bad = 0;
    uint32_t par = 0;
#pragma unroll 1
    for (uint64_t r0 = 0; r0 < n; r0 += RL_THREADS, par ^= 1u) {
        const uint64_t r = r0 + tid;
        uint64_t g0 = 0, g1 = 0, g2 = 0; /* the run as three 64-bit words, as in rt_route_kernel */
        uint32_t set = 0;
        if (r < n) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(A.gruns + r);
            g0 = src[0];
            g1 = src[1];
            g2 = src[2];
            const uint32_t channel = (uint32_t)g2;
            bad |= mfm_runroute_bad_channel(channel, A.C) ? 1 : 0;
            set = mfm_runroute_set_of(A.table, A.C, channel);
        }
        const uint32_t nw = (uint32_t)(g2 >> 32);
        uint32_t rank[RL_K];
#pragma unroll
        for (uint32_t k = 0; k < RL_K; k++) { /* unrolled: rank and wsum stay registers.  All eight routes: no set has a bit at
                                               * or above K (create checked the table), so those ballots are empty */
            const bool in = mfm_runroute_in_route(set, k);
            const uint64_t m = __ballot(in);
            rank[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            wsum[k] += in ? nw : 0u;
            if (lane == 0) {
                s_cnt[par][k][wave] = (uint32_t)__builtin_popcountll(m);
            }
        }
        __syncthreads();
        if (tid < A.K) { /* the route's 16 wave counts become exclusive offsets from its base */
            uint32_t sum = base;
#pragma unroll
            for (uint32_t w = 0; w < RL_WAVES; w++) {
                const uint32_t c = s_cnt[par][tid][w];
                s_cnt[par][tid][w] = sum;
                sum += c;
            }
            base = sum;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < RL_K; k++) {
            if (mfm_runroute_in_route(set, k)) { /* k < K, and the channel exists: create checked the table, and a channel beyond
                                                  * it has the empty set */
                const uint64_t pos = (uint64_t)s_cnt[par][k][wave] + rank[k]; /* < n <= cap_runs: at most n of a route */
                if (pos < s_cap[k]) { /* nothing past the route's own capacity: its totals will say overflow */
                    uint64_t *dst = reinterpret_cast<uint64_t *>(A.runs + (uint64_t)k * A.cap_runs + pos);
                    dst[0] = g0;
                    dst[1] = g1; /* the gate's payload_offset: the payload stays where it is */
                    dst[2] = mfm_runroute_local_word(g2, mfm_runroute_rank_of(A.rank, A.K, (uint32_t)g2, k));
                }
            }
        }
    }
    /* the routes' windows: once, behind the walk */
#pragma unroll
    for (uint32_t k = 0; k < RL_K; k++) {
        /* a wave without a window of the route has nothing to sum: the routes at and above K, and every route of an idle call */
        const uint64_t t = __ballot(wsum[k] != 0) ? rl_wave_total(wsum[k]) : 0u;
        if (lane == 0) {
            s_win[k][wave] = t;
        }
    }
    const uint64_t wave_bad = __ballot(bad);
    if (lane == 0) {
        s_bad[wave] = wave_bad != 0;
    }
    __syncthreads();
    uint32_t wrong = 0;
#pragma unroll
    for (uint32_t w = 0; w < RL_WAVES; w++) {
        wrong |= s_bad[w];
    }
    if (tid < A.K) {
        uint64_t windows = 0;
#pragma unroll
        for (uint32_t w = 0; w < RL_WAVES; w++) {
            windows += s_win[tid][w];
        }
        const bool route_over = !wrong && mfm_runroute_route_over(base, windows, cap_r, cap_w);
        const bool none = wrong || route_over;
        uint64_t *t = A.totals + 4u * tid;
        t[MFM_RUNROUTE_T_RUNS] = none ? 0u : base;
        t[MFM_RUNROUTE_T_ELEMS] = none ? 0u : mfm_runroute_load(windows, A.W); /* <= the route's window capacity * W */
        t[MFM_RUNROUTE_T_OVERFLOW] = route_over ? 1u : 0u;
        t[MFM_RUNROUTE_T_OUT_OF_STEP] = wrong ? 1u : 0u;
    }
    if (tid == 0) {
        *A.bound = mfm_runroute_bound(wrong != 0, A.gtotals[MFM_RUNROUTE_T_ELEMS]);
    }
}

thread_local char g_rl_error[256] = "";

int rl_fail(int code, const char *msg)
{
    snprintf(g_rl_error, sizeof(g_rl_error), "%s", msg);
    mfm_internal_set_error(g_rl_error);
    return code;
}

} /* namespace */

#define RL_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_rl_error, sizeof(g_rl_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_rl_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

extern "C" {

int mfm_runroute_local_process(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                               hipStream_t s)
{
    const RlCall A{ d_runs,      d_totals,     rt->d_table,         rt->d_rank,        rt->d_caps,            rt->d_runs,
                    rt->d_totals, rt->d_bound, rt->cap_runs,        rt->cfg.nr_channels, rt->cfg.nr_routes, rt->cfg.window_samples };
    /* one workgroup whatever the capacity, as rt_route_kernel */
    hipLaunchKernelGGL(rt_local_kernel, dim3(1), dim3(RL_THREADS), 0, s, A);
    RL_TRY(hipGetLastError());
    rt->d_payload = d_payload; /* only handed on: nothing is read here */
    rt->last_stream = s;
    rt->have_call = true;
    return MFM_OK;
}

int mfm_runroute_create_local(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel)
{
    if (!prt || !cfg) {
        return MFM_E_INVAL;
    }
    *prt = nullptr;
    char err[192];
    uint64_t cap_runs = 0, route_runs[RL_K], route_windows[RL_K];
    uint32_t nr_of[RL_K];
    if (const char *m = mfm_runroute_local_geometry(cfg, routes_of_channel, &cap_runs, nr_of, route_runs, route_windows, err, sizeof(err))) {
        return rl_fail(MFM_E_INVAL, m);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    mfm_runroute *rt = new (std::nothrow) mfm_runroute();
    if (!rt) {
        return MFM_E_NOMEM;
    }
    rt->cfg = *cfg;
    rt->cap_runs = cap_runs;
    rt->sets = true; /* the table is one of sets: what mfm_runroute_route_channels reads */
    rt->local = true;
    const size_t K = cfg->nr_routes, C = cfg->nr_channels, nruns = (size_t)(cap_runs ? cap_runs : 1);
    *prt = rt; /* from here on the caller's destroy frees what was allocated */
    rt->h_table = new (std::nothrow) uint8_t[C];
    if (!rt->h_table) {
        return MFM_E_NOMEM;
    }
    memcpy(rt->h_table, routes_of_channel, C);
    uint64_t caps[RL_K][2];
    for (size_t k = 0; k < K; k++) {
        rt->nr_of[k] = nr_of[k];
        rt->cap_route_runs[k] = caps[k][0] = route_runs[k];
        rt->cap_route_windows[k] = caps[k][1] = route_windows[k];
    }
    uint32_t *rank = new (std::nothrow) uint32_t[C * K];
    if (!rank) {
        return MFM_E_NOMEM;
    }
    uint32_t count[RL_K];
    mfm_runroute_build_ranks(routes_of_channel, cfg->nr_channels, cfg->nr_routes, rank, count);
    hipError_t e = hipSetDevice(cfg->device);
    if (e == hipSuccess) {
        e = hipMalloc(&rt->d_rank, C * K * sizeof(uint32_t));
    }
    if (e == hipSuccess) {
        e = hipMemcpy(rt->d_rank, rank, C * K * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    delete[] rank;
    RL_TRY(e);
    RL_TRY(hipMalloc(&rt->d_table, C));
    RL_TRY(hipMemcpy(rt->d_table, routes_of_channel, C, hipMemcpyHostToDevice));
    RL_TRY(hipMalloc(&rt->d_runs, K * nruns * sizeof(mfm_gate_run)));
    RL_TRY(hipMalloc(&rt->d_totals, K * 4 * 8));
    RL_TRY(hipMemset(rt->d_totals, 0, K * 4 * 8));
    RL_TRY(hipMalloc(&rt->d_caps, K * 2 * 8));
    RL_TRY(hipMemcpy(rt->d_caps, caps, K * 2 * 8, hipMemcpyHostToDevice));
    RL_TRY(hipMalloc(&rt->d_bound, 8));
    RL_TRY(hipMemset(rt->d_bound, 0, 8));
    RL_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

int mfm_runroute_bound_view(struct mfm_runroute *rt, const uint64_t **d_payload_elems)
{
    if (!rt || !d_payload_elems) {
        return MFM_E_INVAL;
    }
    *d_payload_elems = nullptr;
    if (!rt->local) {
        return rl_fail(MFM_E_INVAL, "the router was not made by mfm_runroute_create_local: its routes' totals carry the bound of the payload "
                                    "ranges themselves (the gate's payload elements, or under MFM_RUNROUTE_F_PACK the route's own)");
    }
    *d_payload_elems = rt->d_bound;
    return MFM_OK;
}

int mfm_hosttwin_runroute_local_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *routes_of_channel, uint32_t window_samples,
                                     size_t max_runs, const uint32_t *route_max_runs, const uint32_t *route_max_windows,
                                     const struct mfm_gate_run *gate_runs, const uint64_t *gate_totals, struct mfm_gate_run *runs,
                                     uint64_t *totals, uint64_t *payload_elems)
{
    if (!gate_totals || !totals || !payload_elems || !route_max_runs || !route_max_windows || (!gate_runs && gate_totals[MFM_RUNROUTE_T_RUNS]) ||
        (!runs && max_runs)) {
        return MFM_E_INVAL;
    }
    mfm_runroute_config cfg{};
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = nr_channels;
    cfg.nr_routes = nr_routes;
    cfg.window_samples = window_samples;
    cfg.max_windows = 1; /* the table, nr_routes and window_samples are what is checked here: the capacities are the caller's */
    cfg.max_runs = 1;
    char err[192];
    uint64_t cap_runs = 0, rr[RL_K], rw[RL_K];
    uint32_t nr_of[RL_K];
    if (const char *m = mfm_runroute_local_geometry(&cfg, routes_of_channel, &cap_runs, nr_of, rr, rw, err, sizeof(err))) {
        return rl_fail(MFM_E_INVAL, m);
    }
    for (uint32_t k = 0; k < nr_routes; k++) {
        if (route_max_runs[k] > max_runs) {
            return rl_fail(MFM_E_INVAL, "a route's capacity exceeds the row it is given: max_runs records");
        }
    }
    uint32_t *rank = new (std::nothrow) uint32_t[(size_t)nr_channels * nr_routes];
    if (!rank) {
        return MFM_E_NOMEM;
    }
    uint32_t members[RL_K];
    mfm_runroute_build_ranks(routes_of_channel, nr_channels, nr_routes, rank, members);
    uint64_t over, oos;
    bool refused = mfm_runroute_refused(gate_totals, max_runs, over, oos);
    const uint64_t n = refused ? 0u : gate_totals[MFM_RUNROUTE_T_RUNS];
    for (uint64_t r = 0; r < n && !refused; r++) {
        if (mfm_runroute_bad_channel(gate_runs[r].channel, nr_channels)) {
            refused = true;
            oos = 1u;
        }
    }
    *payload_elems = mfm_runroute_bound(refused, gate_totals[MFM_RUNROUTE_T_ELEMS]);
    for (uint32_t k = 0; k < nr_routes; k++) {
        uint64_t *t = totals + 4u * k;
        t[MFM_RUNROUTE_T_RUNS] = 0;
        t[MFM_RUNROUTE_T_ELEMS] = 0;
        t[MFM_RUNROUTE_T_OVERFLOW] = refused ? over : 0u;
        t[MFM_RUNROUTE_T_OUT_OF_STEP] = refused ? oos : 0u;
        if (refused) {
            continue;
        }
        uint64_t count = 0, windows = 0;
        for (uint64_t r = 0; r < n; r++) { /* what the route would carry, before anything is written */
            if (mfm_runroute_in_route(mfm_runroute_set_of(routes_of_channel, nr_channels, gate_runs[r].channel), k)) {
                count++;
                windows += gate_runs[r].nr_windows;
            }
        }
        if (mfm_runroute_route_over(count, windows, route_max_runs[k], route_max_windows[k])) {
            t[MFM_RUNROUTE_T_OVERFLOW] = 1u;
            continue;
        }
        mfm_gate_run *row = runs + (size_t)k * max_runs;
        uint64_t at = 0;
        for (uint64_t r = 0; r < n; r++) {
            const mfm_gate_run &g = gate_runs[r];
            if (!mfm_runroute_in_route(mfm_runroute_set_of(routes_of_channel, nr_channels, g.channel), k)) {
                continue;
            }
            row[at] = g; /* first_window, nr_windows and payload_offset are the gate's */
            row[at].channel = mfm_runroute_rank_of(rank, nr_routes, g.channel, k);
            at++;
        }
        t[MFM_RUNROUTE_T_RUNS] = count;
        t[MFM_RUNROUTE_T_ELEMS] = mfm_runroute_load(windows, window_samples);
    }
    delete[] rank;
    return MFM_OK;
}

} /* extern "C" */
