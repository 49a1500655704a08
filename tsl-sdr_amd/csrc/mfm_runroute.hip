/*
 * mfm_runroute.hip - the run router: the run list of one squelch-gate call is partitioned by a per-channel route table, so that
 * each protocol's burst chain (burst resampler -> burst AIS / POCSAG / FLEX) reads only the runs of its own channels.  See
 * include/multifm_hip.h for the boundary and mfm_runroute.h for the arithmetic.  An object of its own, as mfm_runrs_dc.hip is, so
 * that every other object keeps the kernels it had.
 *
 * Zero-copy: the payload stays the gate's; what is written is one run list of the full capacity and one totals quad per route,
 * at addresses fixed at create.  How many runs a call carries is read on the device, so the host never waits.
 *
 *   rt_route_kernel  ONE workgroup of 1024 lanes walks the gate's run list in strips of 1024 runs, one lane per run.  A lane
 *                    reads its run and its channel's byte of the route table.  For each route k the wave ballots
 *                    route == k: the lane's rank within the wave is the count of set bits below it, the wave's count goes to
 *                    LDS.  Lanes 0 .. K - 1 then turn the 16 wave counts of their route into exclusive offsets from the
 *                    route's running base (which they carry from strip to strip in a register), and every lane copies its run
 *                    to base + wave offset + rank of its route's list.  Strips are taken in order, so the partition is stable.
 *                    The LDS counts are kept twice and used in turn, which makes it two barriers per strip.  At the end lanes
 *                    0 .. K - 1 write their route's totals.
 *
 * The other cross-workgroup form, a count / scan / scatter triple over many workgroups, is three launches where this is one;
 * DESIGN.md section 3.3 has the measurement this form was kept on.
 *
 * No float, no atomics, no scratch.
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

constexpr uint32_t RT_THREADS = 1024, RT_WAVES = RT_THREADS / 64u;
constexpr uint64_t RT_MAX_RUNS = 1ull << 31; /* as the burst resampler's */

static_assert(sizeof(mfm_gate_run) == 24 && offsetof(mfm_gate_run, channel) == 16, "the kernel copies a run as three 64-bit words");

struct RtCall {
    const mfm_gate_run *gruns;
    const uint64_t *gtotals;
    const uint8_t *table; /* [C] */
    mfm_gate_run *runs;   /* [K][cap_runs] */
    uint64_t *totals;     /* [K][4] */
    uint64_t cap_runs;
    uint32_t C, K;
};

__global__ __launch_bounds__(RT_THREADS) void rt_route_kernel(const RtCall A)
{
    __shared__ uint32_t s_cnt[2][MFM_RUNROUTE_MAX_ROUTES][RT_WAVES];
    __shared__ uint32_t s_bad[RT_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid / 64u, lane = tid % 64u;
    uint64_t over, oos;
    if (mfm_runroute_refused(A.gtotals, A.cap_runs, over, oos)) {
        if (tid < A.K) {
            uint64_t *t = A.totals + 4u * tid;
            t[MFM_RUNROUTE_T_RUNS] = 0;
            t[MFM_RUNROUTE_T_ELEMS] = 0;
            t[MFM_RUNROUTE_T_OVERFLOW] = over;
            t[MFM_RUNROUTE_T_OUT_OF_STEP] = oos;
        }
        return;
    }
    const uint64_t n = A.gtotals[MFM_RUNROUTE_T_RUNS]; /* <= cap_runs < 2^31 */
    uint32_t base = 0;                                  /* lanes 0 .. K - 1: runs of route tid in the strips so far */
    int bad = 0;
    uint32_t par = 0;
#pragma unroll 1
    for (uint64_t r0 = 0; r0 < n; r0 += RT_THREADS, par ^= 1u) {
        const uint64_t r = r0 + tid;
        /* the run as three 64-bit words (first_window, payload_offset, channel | nr_windows << 32): a struct that is loaded under
         * a condition and stored behind the barriers is otherwise given a place in LDS */
        uint64_t g0 = 0, g1 = 0, g2 = 0;
        uint32_t route = MFM_ROUTE_NONE;
        if (r < n) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(A.gruns + r);
            g0 = src[0];
            g1 = src[1];
            g2 = src[2];
            const uint32_t channel = (uint32_t)g2;
            bad |= mfm_runroute_bad_channel(channel, A.C) ? 1 : 0;
            route = mfm_runroute_of(A.table, A.C, channel);
        }
        uint32_t rank = 0;
        for (uint32_t k = 0; k < A.K; k++) { /* K uniform: scalar work but for the rank */
            const uint64_t m = __ballot(route == k);
            if (route == k) {
                rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            }
            if (lane == 0) {
                s_cnt[par][k][wave] = (uint32_t)__builtin_popcountll(m);
            }
        }
        __syncthreads();
        if (tid < A.K) { /* the route's 16 wave counts become exclusive offsets from its base */
            uint32_t c[RT_WAVES];
#pragma unroll
            for (uint32_t w = 0; w < RT_WAVES; w++) {
                c[w] = s_cnt[par][tid][w];
            }
            uint32_t sum = base;
#pragma unroll
            for (uint32_t w = 0; w < RT_WAVES; w++) {
                s_cnt[par][tid][w] = sum;
                sum += c[w];
            }
            base = sum;
        }
        __syncthreads();
        if (route < A.K) { /* route < K or MFM_ROUTE_NONE: create checked the table */
            const uint64_t at = (uint64_t)route * A.cap_runs + s_cnt[par][route][wave] + rank; /* < (route + 1) * cap_runs: at most n of a route */
            uint64_t *dst = reinterpret_cast<uint64_t *>(A.runs + at);
            dst[0] = g0;
            dst[1] = g1;
            dst[2] = g2;
        }
    }
    const uint64_t wave_bad = __ballot(bad);
    if (lane == 0) {
        s_bad[wave] = wave_bad != 0;
    }
    __syncthreads();
    if (tid < A.K) {
        uint32_t wrong = 0;
#pragma unroll
        for (uint32_t w = 0; w < RT_WAVES; w++) {
            wrong |= s_bad[w];
        }
        uint64_t *t = A.totals + 4u * tid;
        t[MFM_RUNROUTE_T_RUNS] = wrong ? 0u : base;
        t[MFM_RUNROUTE_T_ELEMS] = wrong ? 0u : A.gtotals[MFM_RUNROUTE_T_ELEMS];
        t[MFM_RUNROUTE_T_OVERFLOW] = 0;
        t[MFM_RUNROUTE_T_OUT_OF_STEP] = wrong ? 1u : 0u;
    }
}

thread_local char g_rt_error[256] = "";

int rt_fail(int code, const char *msg)
{
    snprintf(g_rt_error, sizeof(g_rt_error), "%s", msg);
    mfm_internal_set_error(g_rt_error);
    return code;
}

/* what create checks of the route table and derives from the configuration, without a device; NULL or the message */
const char *rt_table_check(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *route_of_channel, char *err, size_t cap)
{
    if (0 == nr_channels || nr_channels > 65535u) {
        return "nr_channels must be 1 .. 65535";
    }
    if (0 == nr_routes || nr_routes > MFM_RUNROUTE_MAX_ROUTES) {
        snprintf(err, cap, "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES = %u", MFM_RUNROUTE_MAX_ROUTES);
        return err;
    }
    if (!route_of_channel) {
        return "no route table";
    }
    for (uint32_t c = 0; c < nr_channels; c++) {
        if (route_of_channel[c] >= nr_routes && route_of_channel[c] != MFM_ROUTE_NONE) {
            snprintf(err, cap, "route_of_channel[%u] = %u is neither below nr_routes = %u nor MFM_ROUTE_NONE (255)", c, route_of_channel[c],
                     nr_routes);
            return err;
        }
    }
    return nullptr;
}

const char *rt_geometry(const mfm_runroute_config &cfg, const uint8_t *route_of_channel, uint64_t &cap_runs, char *err, size_t cap)
{
    if (cfg.abi_version != MFM_ABI_VERSION) {
        return "abi_version is not MFM_ABI_VERSION";
    }
    if (cfg.flags != 0) {
        return "flags must be 0";
    }
    if (const char *m = rt_table_check(cfg.nr_channels, cfg.nr_routes, route_of_channel, err, cap)) {
        return m;
    }
    cap_runs = cfg.max_runs;
    if (0 == cfg.max_runs) { /* the burst resampler's default for the same numbers, by its rule */
        if (0 == cfg.window_samples || cfg.window_samples > (1u << 20)) {
            return "window_samples must be 1 .. 2^20, the gate's";
        }
        mfm_runrs_caps caps;
        if (!mfm_runrs_caps_of(cfg.nr_channels, cfg.window_samples, cfg.max_windows, 0u, cfg.max_in_samples, cfg.preroll_windows, caps)) {
            return "max_runs is 0 (the burst resampler's default) and max_in_samples is 0: give the gate's max_in_samples";
        }
        cap_runs = caps.runs;
    }
    if (cap_runs >= RT_MAX_RUNS) {
        return "max_runs must stay below 2^31";
    }
    return nullptr;
}

} /* namespace */

#define RT_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_rt_error, sizeof(g_rt_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_rt_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

extern "C" {

int mfm_hosttwin_runroute_capacity(const struct mfm_runroute_config *cfg, const uint8_t *route_of_channel, uint32_t *max_runs)
{
    if (!cfg) {
        return MFM_E_INVAL;
    }
    char err[192];
    uint64_t cap = 0;
    if (const char *m = rt_geometry(*cfg, route_of_channel, cap, err, sizeof(err))) {
        return rt_fail(MFM_E_INVAL, m);
    }
    if (max_runs) {
        *max_runs = (uint32_t)cap;
    }
    return MFM_OK;
}

int mfm_runroute_create(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *route_of_channel)
{
    if (!prt || !cfg) {
        return MFM_E_INVAL;
    }
    *prt = nullptr;
    char err[192];
    uint64_t cap = 0;
    if (const char *m = rt_geometry(*cfg, route_of_channel, cap, err, sizeof(err))) {
        return rt_fail(MFM_E_INVAL, m);
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
    rt->cap_runs = cap;
    const size_t K = cfg->nr_routes, nruns = (size_t)(cap ? cap : 1);
    *prt = rt; /* from here on the caller's destroy frees what was allocated */
    rt->h_table = new (std::nothrow) uint8_t[cfg->nr_channels]; /* for mfm_runroute_route_channels */
    if (!rt->h_table) {
        return MFM_E_NOMEM;
    }
    memcpy(rt->h_table, route_of_channel, cfg->nr_channels);
    RT_TRY(hipSetDevice(cfg->device));
    RT_TRY(hipMalloc(&rt->d_table, cfg->nr_channels));
    RT_TRY(hipMemcpy(rt->d_table, route_of_channel, cfg->nr_channels, hipMemcpyHostToDevice));
    RT_TRY(hipMalloc(&rt->d_runs, K * nruns * sizeof(mfm_gate_run)));
    RT_TRY(hipMalloc(&rt->d_totals, K * 4 * 8));
    RT_TRY(hipMemset(rt->d_totals, 0, K * 4 * 8));
    RT_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runroute_destroy(struct mfm_runroute **prt)
{
    if (!prt || !*prt) {
        return;
    }
    mfm_runroute *rt = *prt;
    (void)hipSetDevice(rt->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(rt->d_table);
    (void)hipFree(rt->d_runs);
    (void)hipFree(rt->d_totals);
    (void)hipFree(rt->d_bound);
    mfm_runroute_sets_free(rt);
    delete rt;
    *prt = nullptr;
}

int mfm_runroute_process_device(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                                void *stream)
{
    if (!rt || !d_runs || !d_payload || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    RT_TRY(hipSetDevice(rt->cfg.device));
    if (rt->have_call && rt->last_stream != s) {
        RT_TRY(hipStreamSynchronize(rt->last_stream)); /* the result buffers are reused: keep calls ordered */
    }
    if (rt->local) { /* made by mfm_runroute_create_local: the kernel of mfm_runroute_local.hip */
        return mfm_runroute_local_process(rt, d_runs, d_payload, d_totals, s);
    }
    if (rt->sets) { /* made by mfm_runroute_create_sets: the kernels of mfm_runroute_sets.hip */
        return mfm_runroute_sets_process(rt, d_runs, d_payload, d_totals, s);
    }
    const RtCall A{ d_runs, d_totals, rt->d_table, rt->d_runs, rt->d_totals, rt->cap_runs, rt->cfg.nr_channels, rt->cfg.nr_routes };
    /* one workgroup whatever the capacity: it walks as many strips as the gate's run count, read on the device, asks for */
    hipLaunchKernelGGL(rt_route_kernel, dim3(1), dim3(RT_THREADS), 0, s, A);
    RT_TRY(hipGetLastError());
    rt->d_payload = d_payload;
    rt->last_stream = s;
    rt->have_call = true;
    return MFM_OK;
}

int mfm_runroute_device_view(struct mfm_runroute *rt, uint32_t route, const struct mfm_gate_run **d_runs, const int16_t **d_payload,
                             const uint64_t **d_totals)
{
    if (!rt) {
        return MFM_E_INVAL;
    }
    if (route >= rt->cfg.nr_routes) {
        return rt_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    if (d_runs) {
        *d_runs = rt->d_runs + (size_t)route * (size_t)(rt->cap_runs ? rt->cap_runs : 1);
    }
    if (d_payload) {
        *d_payload = rt->pack ? rt->d_pack + rt->pack_base[route] : rt->d_payload; /* PACK: the route's own, fixed at create */
    }
    if (d_totals) {
        *d_totals = rt->d_totals + 4u * route;
    }
    return MFM_OK;
}

int mfm_runroute_fetch(struct mfm_runroute *rt, uint32_t route, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, size_t *nr_elems)
{
    if (!rt || !nr_runs || !nr_elems || (!runs && max_runs)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_elems = 0;
    if (route >= rt->cfg.nr_routes) {
        return rt_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    if (!rt->have_call) {
        return MFM_OK;
    }
    RT_TRY(hipSetDevice(rt->cfg.device));
    RT_TRY(hipStreamSynchronize(rt->last_stream));
    uint64_t t[4];
    RT_TRY(hipMemcpy(t, rt->d_totals + 4u * route, sizeof(t), hipMemcpyDeviceToHost));
    *nr_runs = (size_t)t[MFM_RUNROUTE_T_RUNS];
    *nr_elems = (size_t)t[MFM_RUNROUTE_T_ELEMS];
    if (t[MFM_RUNROUTE_T_OUT_OF_STEP]) {
        return rt_fail(MFM_E_STATE, "the gate's call was out of step with its level stage, or its run list names a channel that does not exist");
    }
    if (t[MFM_RUNROUTE_T_OVERFLOW]) {
        return rt_fail(MFM_E_STATE, "the gate's call overflowed its max_open_windows or carries more runs than the router's max_runs");
    }
    if (t[MFM_RUNROUTE_T_RUNS] > max_runs) {
        return MFM_E_NOMEM;
    }
    if (t[MFM_RUNROUTE_T_RUNS]) {
        const mfm_gate_run *src = rt->d_runs + (size_t)route * (size_t)(rt->cap_runs ? rt->cap_runs : 1);
        RT_TRY(hipMemcpy(runs, src, (size_t)t[MFM_RUNROUTE_T_RUNS] * sizeof(mfm_gate_run), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runroute_get_capacity(struct mfm_runroute *rt, uint32_t *max_runs)
{
    if (!rt) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = (uint32_t)rt->cap_runs;
    }
    return MFM_OK;
}

int mfm_hosttwin_runroute_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *route_of_channel, size_t max_runs,
                               const struct mfm_gate_run *gate_runs, const uint64_t *gate_totals, struct mfm_gate_run *runs, uint64_t *totals)
{
    if (!gate_totals || !totals || (!gate_runs && gate_totals[MFM_RUNROUTE_T_RUNS]) || (!runs && max_runs)) {
        return MFM_E_INVAL;
    }
    char err[192];
    if (const char *m = rt_table_check(nr_channels, nr_routes, route_of_channel, err, sizeof(err))) {
        return rt_fail(MFM_E_INVAL, m);
    }
    uint64_t over, oos;
    bool refused = mfm_runroute_refused(gate_totals, max_runs, over, oos);
    const uint64_t n = refused ? 0u : gate_totals[MFM_RUNROUTE_T_RUNS];
    for (uint64_t r = 0; r < n && !refused; r++) {
        if (mfm_runroute_bad_channel(gate_runs[r].channel, nr_channels)) {
            refused = true;
            oos = 1u;
        }
    }
    uint64_t count[MFM_RUNROUTE_MAX_ROUTES] = { 0 };
    if (!refused) {
        for (uint64_t r = 0; r < n; r++) {
            const uint32_t k = mfm_runroute_of(route_of_channel, nr_channels, gate_runs[r].channel);
            if (k < nr_routes) {
                runs[(size_t)k * max_runs + count[k]++] = gate_runs[r];
            }
        }
    }
    for (uint32_t k = 0; k < nr_routes; k++) {
        uint64_t *t = totals + 4u * k;
        t[MFM_RUNROUTE_T_RUNS] = refused ? 0u : count[k];
        t[MFM_RUNROUTE_T_ELEMS] = refused ? 0u : gate_totals[MFM_RUNROUTE_T_ELEMS];
        t[MFM_RUNROUTE_T_OVERFLOW] = refused ? over : 0u;
        t[MFM_RUNROUTE_T_OUT_OF_STEP] = refused ? oos : 0u;
    }
    return MFM_OK;
}

} /* extern "C" */
