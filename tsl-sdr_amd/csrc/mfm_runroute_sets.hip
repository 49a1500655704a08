/*
 * mfm_runroute_sets.hip - the run router's sets form (mfm_runroute_create_sets): a channel's table byte is a SET of routes, so
 * a channel that time-shares two protocols reaches both chains, and under MFM_RUNROUTE_F_PACK every route gets route-local
 * channel numbers, dense offsets and a payload of its own, so that the burst chain behind it is sized to the route.  See
 * include/multifm_hip.h for the boundary and mfm_runroute.h for the arithmetic.  An object of its own, as mfm_runroute.hip is,
 * so that every other object keeps the kernels it had; the router's struct is shared through mfm_runroute_obj.h.
 *
 *   rt_sets_kernel  the strip walk of rt_route_kernel: ONE workgroup of 1024 lanes, one lane per run, strips of 1024 runs in
 *                   order.  A lane reads its run and its channel's set.  For each route k the wave ballots bit k of the set:
 *                   the lane's rank within the wave is the count of set bits below it, and a lane may rank in several routes.
 *                   Under PACK the same walk carries a second sum per route, the 64-bit running count of nr_windows: a wave
 *                   prefix sum over the lanes of the route (skipped by a wave that has none), the wave totals beside the
 *                   wave counts in LDS, and lanes 0 .. K - 1 turn both into exclusive offsets from the route's two running
 *                   bases.  A lane then writes its record once per route it is in; under PACK with the channel's rank in the
 *                   route, the dense offset, and the gate's payload_offset into a side list for the copy.  At the end lanes
 *                   0 .. K - 1 write their route's totals; under PACK a route over its own capacity gets overflow alone.
 *   rt_pack_kernel  PACK only, memory-bound: workgroup b owns RT_TILE elements of one route's dense payload.  It finds the run
 *                   its first element lies in by a binary search over the route's dense offsets and walks the runs its tile
 *                   meets; a lane moves eight elements as one 16-byte access where source and destination are both aligned
 *                   to 16 bytes (a route's payload begins on 16 bytes and so does every eighth element of it; the source is
 *                   wherever the gate put the run), and element by element otherwise.  The grid is the sum of the routes'
 *                   tile capacities; a workgroup beyond its route's elements returns after reading the totals.
 *
 * The other form of the window sums, a partition without them and a scan kernel with one workgroup per route behind it, is one
 * launch more; DESIGN.md section 3.3 has the measurement the walk with the sums in it was kept on.
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

constexpr uint32_t RS_THREADS = 1024, RS_WAVES = RS_THREADS / 64u, RS_K = MFM_RUNROUTE_MAX_ROUTES;
constexpr uint64_t RS_MAX_RUNS = 1ull << 31;        /* as mfm_runroute_create's */
constexpr uint32_t RT_COPY_THREADS = 256, RT_TILE = 8192; /* elements a workgroup copies: four 16-byte accesses a lane */

static_assert(sizeof(mfm_gate_run) == 24 && offsetof(mfm_gate_run, channel) == 16, "the kernel copies a run as three 64-bit words");
static_assert(RS_K <= 8, "a channel's set is one byte");

struct RsCall {
    const mfm_gate_run *gruns;
    const uint64_t *gtotals;
    const uint8_t *table;  /* [C] sets */
    const uint32_t *rank;  /* [C][K], PACK */
    const uint64_t *caps;  /* [K][2] runs, windows a route may carry, PACK */
    mfm_gate_run *runs;    /* [K][cap_runs] */
    uint64_t *src;         /* [K][cap_runs] the gate's payload_offset of each routed run, PACK */
    uint64_t *totals;      /* [K][4] */
    uint64_t cap_runs;
    uint32_t C, K, W;
};

/* inclusive sum over the wave's lanes */
__device__ __forceinline__ uint64_t rs_wave_sum(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        v += lane >= d ? o : 0u;
    }
    return v;
}

template <bool PACK>
__global__ __launch_bounds__(RS_THREADS) void rt_sets_kernel(const RsCall A)
{
    __shared__ uint32_t s_cnt[2][RS_K][RS_WAVES];
    __shared__ uint64_t s_win[PACK ? 2 : 1][PACK ? RS_K : 1][PACK ? RS_WAVES : 1];
    __shared__ uint32_t s_bad[RS_WAVES];
    __shared__ uint32_t s_cap[RS_K]; /* PACK: the routes' own run capacities, below 2^31; read behind a strip's barriers */
    const uint32_t tid = threadIdx.x, wave = tid / 64u, lane = tid % 64u;
    if (PACK && tid < A.K) {
        s_cap[tid] = (uint32_t)A.caps[2u * tid];
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
        return;
    }
    const uint64_t n = A.gtotals[MFM_RUNROUTE_T_RUNS]; /* <= cap_runs < 2^31 */
    const uint64_t gate_elems = A.gtotals[MFM_RUNROUTE_T_ELEMS];
    uint32_t base = 0;  /* lanes 0 .. K - 1: runs of route tid in the strips so far */
    uint64_t wbase = 0; /* and their windows: below 2^31 * 2^32 */
    int bad = 0;
    uint32_t par = 0;
#pragma unroll 1
    for (uint64_t r0 = 0; r0 < n; r0 += RS_THREADS, par ^= 1u) {
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
            if (PACK) {
                bad |= mfm_runroute_bad_range(g1, (uint32_t)(g2 >> 32), A.W, gate_elems) ? 1 : 0;
            }
            set = mfm_runroute_set_of(A.table, A.C, channel);
        }
        const uint32_t nw = (uint32_t)(g2 >> 32);
        uint32_t rank[RS_K];
        uint64_t wpre[RS_K]; /* windows of the route's lanes below this one in the wave */
#pragma unroll
        for (uint32_t k = 0; k < RS_K; k++) { /* unrolled: rank and wpre stay registers.  All eight routes: no set has a bit at
                                               * or above K (create checked the table), so those ballots are empty */
            const bool in = mfm_runroute_in_route(set, k);
            const uint64_t m = __ballot(in);
            rank[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            wpre[k] = 0;
            uint64_t incl = 0;
            if (PACK && m) { /* a wave without a lane of the route has nothing to sum */
                const uint64_t v = in ? nw : 0u;
                incl = rs_wave_sum(v, lane);
                wpre[k] = incl - v;
            }
            if (lane == 63u) {
                s_cnt[par][k][wave] = (uint32_t)__builtin_popcountll(m);
                if (PACK) {
                    s_win[par][k][wave] = incl;
                }
            }
        }
        __syncthreads();
        if (tid < A.K) { /* the route's 16 wave counts (and window sums) become exclusive offsets from its bases */
            uint32_t sum = base;
            uint64_t wsum = wbase;
#pragma unroll
            for (uint32_t w = 0; w < RS_WAVES; w++) {
                const uint32_t c = s_cnt[par][tid][w];
                s_cnt[par][tid][w] = sum;
                sum += c;
                if (PACK) {
                    const uint64_t x = s_win[par][tid][w];
                    s_win[par][tid][w] = wsum;
                    wsum += x;
                }
            }
            base = sum;
            wbase = wsum;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < RS_K; k++) {
            if (mfm_runroute_in_route(set, k)) { /* k < K: create checked the table */
                const uint64_t pos = (uint64_t)s_cnt[par][k][wave] + rank[k]; /* < n <= cap_runs: at most n of a route */
                uint64_t *dst = reinterpret_cast<uint64_t *>(A.runs + (uint64_t)k * A.cap_runs + pos);
                if (!PACK) {
                    dst[0] = g0;
                    dst[1] = g1;
                    dst[2] = g2;
                } else if (pos < s_cap[k]) { /* nothing past the route's own capacity: its totals will say overflow */
                    dst[0] = g0;
                    dst[1] = (s_win[par][k][wave] + wpre[k]) * A.W;
                    dst[2] = (g2 & 0xffffffff00000000ull) | mfm_runroute_rank_of(A.rank, A.K, (uint32_t)g2, k);
                    A.src[(uint64_t)k * A.cap_runs + pos] = g1;
                }
            }
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
        for (uint32_t w = 0; w < RS_WAVES; w++) {
            wrong |= s_bad[w];
        }
        uint64_t route_over = 0;
        uint64_t elems = gate_elems;
        if (PACK) {
            route_over = !wrong && mfm_runroute_route_over(base, wbase, A.caps[2u * tid], A.caps[2u * tid + 1u]) ? 1u : 0u;
            elems = wbase * A.W; /* <= the route's window capacity * W */
        }
        const bool none = wrong || route_over;
        uint64_t *t = A.totals + 4u * tid;
        t[MFM_RUNROUTE_T_RUNS] = none ? 0u : base;
        t[MFM_RUNROUTE_T_ELEMS] = none ? 0u : elems;
        t[MFM_RUNROUTE_T_OVERFLOW] = route_over;
        t[MFM_RUNROUTE_T_OUT_OF_STEP] = wrong ? 1u : 0u;
    }
}

/* eight samples as one 16-byte access */
struct __attribute__((aligned(16))) rt_x8 {
    uint32_t d[4];
};

struct CpCall {
    const mfm_gate_run *runs; /* [K][cap_runs] the routes' records: dense payload_offset */
    const uint64_t *src;      /* [K][cap_runs] the gate's payload_offset */
    const uint64_t *totals;   /* [K][4] */
    const int16_t *gpayload;
    int16_t *pack;
    uint64_t cap_runs;
    uint64_t pack_base[RS_K]; /* in elements, multiples of 8 */
    uint32_t tile_base[RS_K]; /* route k's first workgroup */
    uint32_t K, W;
};

__global__ __launch_bounds__(RT_COPY_THREADS) void rt_pack_kernel(const CpCall A)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    uint32_t k = 0, tb = A.tile_base[0];
    uint64_t pb = A.pack_base[0];
#pragma unroll
    for (uint32_t j = 1; j < RS_K; j++) { /* constant indices: the by-value arrays stay in scalar registers */
        if (j < A.K && b >= A.tile_base[j]) {
            k = j;
            tb = A.tile_base[j];
            pb = A.pack_base[j];
        }
    }
    const uint64_t *t = A.totals + 4u * k;
    const uint64_t n = t[MFM_RUNROUTE_T_RUNS], elems = t[MFM_RUNROUTE_T_ELEMS];
    const uint64_t t0 = (uint64_t)(b - tb) * RT_TILE;
    if (t0 >= elems || 0 == n) {
        return; /* a refused call, a route over its capacity, or a tile beyond what this call carries */
    }
    const uint64_t t1 = t0 + RT_TILE < elems ? t0 + RT_TILE : elems; /* <= the route's capacity: the partition flagged more */
    const mfm_gate_run *runs = A.runs + (uint64_t)k * A.cap_runs;
    const uint64_t *src = A.src + (uint64_t)k * A.cap_runs;
    /* the run element t0 lies in: the last r with payload_offset <= t0 (offsets are dense and begin at 0) */
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint64_t mid = (lo + hi) >> 1;
        if (runs[mid].payload_offset <= t0) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    int16_t *dst = A.pack + pb;
    const uint64_t gp8 = (uint64_t)(reinterpret_cast<uintptr_t>(A.gpayload) >> 1); /* the gate payload's address in elements */
#pragma unroll 1
    for (uint64_t r = lo; r < n; r++) {
        const uint64_t off = runs[r].payload_offset;
        if (off >= t1) {
            break;
        }
        const uint64_t len = (uint64_t)runs[r].nr_windows * A.W;
        const uint64_t d0 = off > t0 ? off : t0, d1 = off + len < t1 ? off + len : t1;
        if (d1 <= d0) {
            continue;
        }
        const uint64_t so = src[r];
        const int16_t *s = A.gpayload + so; /* element e of the route's payload is s[e - off] */
        /* dst + e is on 16 bytes when e % 8 == 0; s + (e - off) then is when the two addresses agree modulo 8 elements */
        const bool vec = ((gp8 + so) & 7u) == (off & 7u);
        const uint64_t g1 = (d1 + 7u) / 8u;
        for (uint64_t g = d0 / 8u + tid; g < g1; g += RT_COPY_THREADS) {
            const uint64_t e0 = g * 8u, e1 = e0 + 8u;
            if (vec && e0 >= d0 && e1 <= d1) {
                *reinterpret_cast<rt_x8 *>(dst + e0) = *reinterpret_cast<const rt_x8 *>(s + (e0 - off));
            } else {
                const uint64_t a = e0 > d0 ? e0 : d0, z = e1 < d1 ? e1 : d1;
                for (uint64_t e = a; e < z; e++) {
                    dst[e] = s[e - off];
                }
            }
        }
    }
}

thread_local char g_rs_error[256] = "";

int rs_fail(int code, const char *msg)
{
    snprintf(g_rs_error, sizeof(g_rs_error), "%s", msg);
    mfm_internal_set_error(g_rs_error);
    return code;
}

const char *rs_table_check(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *routes_of_channel, char *err, size_t cap)
{
    if (0 == nr_channels || nr_channels > 65535u) {
        return "nr_channels must be 1 .. 65535";
    }
    if (0 == nr_routes || nr_routes > MFM_RUNROUTE_MAX_ROUTES) {
        snprintf(err, cap, "nr_routes must be 1 .. MFM_RUNROUTE_MAX_ROUTES = %u", MFM_RUNROUTE_MAX_ROUTES);
        return err;
    }
    if (!routes_of_channel) {
        return "no route table";
    }
    for (uint32_t c = 0; c < nr_channels; c++) {
        if (routes_of_channel[c] >> nr_routes) {
            snprintf(err, cap, "routes_of_channel[%u] = 0x%02x has a bit at or above nr_routes = %u", c, routes_of_channel[c], nr_routes);
            return err;
        }
    }
    return nullptr;
}

/* what the object is made from, derived without a device */
struct RsGeometry {
    uint64_t cap_runs = 0;
    uint32_t nr_of[RS_K] = { 0 };
    mfm_runrs_caps route[RS_K] = {}; /* PACK */
};

/* local: for mfm_runroute_create_local, which takes no flag and whose routes are sized as PACK's are, without a payload of
 * their own */
const char *rs_geometry(const mfm_runroute_config &cfg, const uint8_t *routes_of_channel, RsGeometry &G, char *err, size_t cap, bool local = false)
{
    if (cfg.abi_version != MFM_ABI_VERSION) {
        return "abi_version is not MFM_ABI_VERSION";
    }
    if (local && cfg.flags != 0) {
        return "flags must be 0: mfm_runroute_create_local takes none, and MFM_RUNROUTE_F_PACK belongs to mfm_runroute_create_sets";
    }
    if (cfg.flags & ~MFM_RUNROUTE_F_PACK) {
        return "flags must be 0 or MFM_RUNROUTE_F_PACK";
    }
    const bool pack = local || (cfg.flags & MFM_RUNROUTE_F_PACK) != 0; /* the routes are sized to their channels */
    const char *form = local ? "behind mfm_runroute_create_local" : "under MFM_RUNROUTE_F_PACK";
    if (const char *m = rs_table_check(cfg.nr_channels, cfg.nr_routes, routes_of_channel, err, cap)) {
        return m;
    }
    if ((0 == cfg.max_runs || pack) && (0 == cfg.window_samples || cfg.window_samples > (1u << 20))) {
        return "window_samples must be 1 .. 2^20, the gate's";
    }
    G.cap_runs = cfg.max_runs;
    if (0 == cfg.max_runs) { /* the burst resampler's default for the same numbers, as mfm_runroute_create */
        mfm_runrs_caps caps;
        if (!mfm_runrs_caps_of(cfg.nr_channels, cfg.window_samples, cfg.max_windows, 0u, cfg.max_in_samples, cfg.preroll_windows, caps)) {
            return "max_runs is 0 (the burst resampler's default) and max_in_samples is 0: give the gate's max_in_samples";
        }
        G.cap_runs = caps.runs;
    }
    if (G.cap_runs >= RS_MAX_RUNS) {
        return "max_runs must stay below 2^31";
    }
    for (uint32_t c = 0; c < cfg.nr_channels; c++) {
        for (uint32_t k = 0; k < cfg.nr_routes; k++) {
            G.nr_of[k] += mfm_runroute_in_route(routes_of_channel[c], k) ? 1u : 0u;
        }
    }
    if (!pack) {
        return nullptr;
    }
    uint64_t tiles = 0;
    for (uint32_t k = 0; k < cfg.nr_routes; k++) {
        if (0 == G.nr_of[k]) {
            snprintf(err, cap, "route %u has no channel: %s a route's stages are sized to its channels", k, form);
            return err;
        }
        if (!mfm_runroute_pack_caps(G.nr_of[k], cfg.window_samples, cfg.max_windows, cfg.max_runs, cfg.max_in_samples, cfg.preroll_windows,
                                    G.route[k])) {
            return local ? "mfm_runroute_create_local with max_in_samples 0 needs max_windows and max_runs"
                         : "MFM_RUNROUTE_F_PACK with max_in_samples 0 needs max_windows and max_runs";
        }
        if (G.route[k].runs > G.cap_runs) { /* a route's list is a row of the router's capacity; the rule never gives more */
            G.route[k].runs = G.cap_runs;
        }
        if (G.route[k].windows > 0xffffffffull) {
            return "a route's window capacity must stay below 2^32";
        }
        tiles += (G.route[k].windows * cfg.window_samples + RT_TILE - 1u) / RT_TILE;
    }
    if (!local && tiles >= (1ull << 31)) { /* the local form copies nothing */
        return "the routes' payload capacities together must stay below 2^31 tiles of 8192 elements";
    }
    return nullptr;
}

} /* namespace */

#define RS_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_rs_error, sizeof(g_rs_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_rs_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

extern "C" {

const char *mfm_runroute_local_geometry(const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel, uint64_t *cap_runs,
                                        uint32_t *nr_of, uint64_t *route_runs, uint64_t *route_windows, char *err, size_t cap)
{
    RsGeometry G;
    if (const char *m = rs_geometry(*cfg, routes_of_channel, G, err, cap, true)) {
        return m;
    }
    *cap_runs = G.cap_runs;
    for (uint32_t k = 0; k < RS_K; k++) {
        nr_of[k] = G.nr_of[k];
        route_runs[k] = G.route[k].runs;
        route_windows[k] = G.route[k].windows;
    }
    return nullptr;
}

void mfm_runroute_sets_free(struct mfm_runroute *rt)
{
    (void)hipFree(rt->d_rank);
    (void)hipFree(rt->d_caps);
    (void)hipFree(rt->d_src);
    (void)hipFree(rt->d_pack);
    delete[] rt->h_table;
    rt->h_table = nullptr;
}

int mfm_runroute_sets_process(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                              hipStream_t s)
{
    const RsCall A{ d_runs,      d_totals,     rt->d_table,         rt->d_rank,        rt->d_caps, rt->d_runs, rt->d_src, rt->d_totals,
                    rt->cap_runs, rt->cfg.nr_channels, rt->cfg.nr_routes, rt->cfg.window_samples };
    /* one workgroup whatever the capacity, as rt_route_kernel */
    if (rt->pack) {
        hipLaunchKernelGGL(rt_sets_kernel<true>, dim3(1), dim3(RS_THREADS), 0, s, A);
    } else {
        hipLaunchKernelGGL(rt_sets_kernel<false>, dim3(1), dim3(RS_THREADS), 0, s, A);
    }
    RS_TRY(hipGetLastError());
    if (rt->pack) {
        CpCall B{};
        B.runs = rt->d_runs;
        B.src = rt->d_src;
        B.totals = rt->d_totals;
        B.gpayload = d_payload;
        B.pack = rt->d_pack;
        B.cap_runs = rt->cap_runs;
        for (uint32_t k = 0; k < RS_K; k++) {
            B.pack_base[k] = rt->pack_base[k < rt->cfg.nr_routes ? k : rt->cfg.nr_routes];
            B.tile_base[k] = rt->tile_base[k < rt->cfg.nr_routes ? k : rt->cfg.nr_routes];
        }
        B.K = rt->cfg.nr_routes;
        B.W = rt->cfg.window_samples;
        const uint32_t tiles = rt->tile_base[rt->cfg.nr_routes]; /* from the capacities: what a call carries is read on the device */
        if (tiles) {
            hipLaunchKernelGGL(rt_pack_kernel, dim3(tiles), dim3(RT_COPY_THREADS), 0, s, B);
            RS_TRY(hipGetLastError());
        }
    }
    rt->d_payload = d_payload;
    rt->last_stream = s;
    rt->have_call = true;
    return MFM_OK;
}

int mfm_runroute_create_sets(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel)
{
    if (!prt || !cfg) {
        return MFM_E_INVAL;
    }
    *prt = nullptr;
    char err[192];
    RsGeometry G;
    if (const char *m = rs_geometry(*cfg, routes_of_channel, G, err, sizeof(err))) {
        return rs_fail(MFM_E_INVAL, m);
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
    rt->cap_runs = G.cap_runs;
    rt->sets = true;
    rt->pack = (cfg->flags & MFM_RUNROUTE_F_PACK) != 0;
    const size_t K = cfg->nr_routes, C = cfg->nr_channels, nruns = (size_t)(G.cap_runs ? G.cap_runs : 1);
    *prt = rt; /* from here on the caller's destroy frees what was allocated */
    rt->h_table = new (std::nothrow) uint8_t[C];
    if (!rt->h_table) {
        return MFM_E_NOMEM;
    }
    memcpy(rt->h_table, routes_of_channel, C);
    for (size_t k = 0; k < K; k++) {
        rt->nr_of[k] = G.nr_of[k];
    }
    RS_TRY(hipSetDevice(cfg->device));
    RS_TRY(hipMalloc(&rt->d_table, C));
    RS_TRY(hipMemcpy(rt->d_table, routes_of_channel, C, hipMemcpyHostToDevice));
    RS_TRY(hipMalloc(&rt->d_runs, K * nruns * sizeof(mfm_gate_run)));
    RS_TRY(hipMalloc(&rt->d_totals, K * 4 * 8));
    RS_TRY(hipMemset(rt->d_totals, 0, K * 4 * 8));
    if (rt->pack) {
        uint32_t *rank = new (std::nothrow) uint32_t[C * K];
        if (!rank) {
            return MFM_E_NOMEM;
        }
        uint32_t count[RS_K];
        mfm_runroute_build_ranks(routes_of_channel, cfg->nr_channels, cfg->nr_routes, rank, count);
        hipError_t e = hipMalloc(&rt->d_rank, C * K * sizeof(uint32_t));
        if (e == hipSuccess) {
            e = hipMemcpy(rt->d_rank, rank, C * K * sizeof(uint32_t), hipMemcpyHostToDevice);
        }
        delete[] rank;
        RS_TRY(e);
        uint64_t caps[RS_K][2];
        for (size_t k = 0; k < K; k++) {
            rt->cap_route_runs[k] = caps[k][0] = G.route[k].runs;
            rt->cap_route_windows[k] = caps[k][1] = G.route[k].windows;
            const uint64_t elems = G.route[k].windows * cfg->window_samples;
            rt->pack_base[k + 1] = rt->pack_base[k] + ((elems + 7u) & ~7ull); /* every route's payload begins on 16 bytes */
            rt->tile_base[k + 1] = rt->tile_base[k] + (uint32_t)((elems + RT_TILE - 1u) / RT_TILE);
        }
        RS_TRY(hipMalloc(&rt->d_caps, K * 2 * 8));
        RS_TRY(hipMemcpy(rt->d_caps, caps, K * 2 * 8, hipMemcpyHostToDevice));
        RS_TRY(hipMalloc(&rt->d_src, K * nruns * sizeof(uint64_t)));
        RS_TRY(hipMalloc(&rt->d_pack, (size_t)(rt->pack_base[K] ? rt->pack_base[K] : 8u) * sizeof(int16_t)));
    }
    RS_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

int mfm_runroute_route_channels(struct mfm_runroute *rt, uint32_t route, uint32_t *channels, size_t max, size_t *nr)
{
    if (!rt || !nr || (!channels && max)) {
        return MFM_E_INVAL;
    }
    *nr = 0;
    if (route >= rt->cfg.nr_routes) {
        return rs_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    size_t n = 0;
    for (uint32_t c = 0; c < rt->cfg.nr_channels; c++) {
        const bool in = rt->sets ? mfm_runroute_in_route(rt->h_table[c], route) : rt->h_table[c] == route;
        if (in) {
            if (n < max) {
                channels[n] = c;
            }
            n++;
        }
    }
    *nr = n;
    return n > max ? MFM_E_NOMEM : MFM_OK;
}

int mfm_runroute_route_caps(struct mfm_runroute *rt, uint32_t route, uint32_t *nr_channels, uint32_t *max_windows, uint32_t *max_runs)
{
    if (!rt) {
        return MFM_E_INVAL;
    }
    if (route >= rt->cfg.nr_routes) {
        return rs_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    const bool sized = rt->pack || rt->local; /* the route's own numbers */
    if (nr_channels) {
        *nr_channels = sized ? rt->nr_of[route] : rt->cfg.nr_channels;
    }
    if (max_windows) {
        *max_windows = sized ? (uint32_t)rt->cap_route_windows[route] : rt->cfg.max_windows;
    }
    if (max_runs) {
        *max_runs = (uint32_t)(sized ? rt->cap_route_runs[route] : rt->cap_runs);
    }
    return MFM_OK;
}

int mfm_runroute_fetch_payload(struct mfm_runroute *rt, uint32_t route, int16_t *payload, size_t max_elems, size_t *nr_elems)
{
    if (!rt || !nr_elems || (!payload && max_elems)) {
        return MFM_E_INVAL;
    }
    *nr_elems = 0;
    if (!rt->pack) {
        return rs_fail(MFM_E_INVAL, "the router was not made with MFM_RUNROUTE_F_PACK: its routes have no payload of their own, it stays the gate's");
    }
    if (route >= rt->cfg.nr_routes) {
        return rs_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    if (!rt->have_call) {
        return MFM_OK;
    }
    RS_TRY(hipSetDevice(rt->cfg.device));
    RS_TRY(hipStreamSynchronize(rt->last_stream));
    uint64_t t[4];
    RS_TRY(hipMemcpy(t, rt->d_totals + 4u * route, sizeof(t), hipMemcpyDeviceToHost));
    *nr_elems = (size_t)t[MFM_RUNROUTE_T_ELEMS];
    if (t[MFM_RUNROUTE_T_OUT_OF_STEP]) {
        return rs_fail(MFM_E_STATE, "the gate's call was out of step with its level stage, or its run list is not a gate's");
    }
    if (t[MFM_RUNROUTE_T_OVERFLOW]) {
        return rs_fail(MFM_E_STATE, "the gate's call overflowed, or carries more runs or windows than the router or this route holds");
    }
    if (t[MFM_RUNROUTE_T_ELEMS] > max_elems) {
        return MFM_E_NOMEM;
    }
    if (t[MFM_RUNROUTE_T_ELEMS]) {
        RS_TRY(hipMemcpy(payload, rt->d_pack + rt->pack_base[route], (size_t)t[MFM_RUNROUTE_T_ELEMS] * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_hosttwin_runroute_route_caps(const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel, uint32_t route,
                                     uint32_t *nr_channels, uint32_t *max_windows, uint32_t *max_runs)
{
    if (!cfg) {
        return MFM_E_INVAL;
    }
    char err[192];
    RsGeometry G;
    if (const char *m = rs_geometry(*cfg, routes_of_channel, G, err, sizeof(err))) {
        return rs_fail(MFM_E_INVAL, m);
    }
    if (route >= cfg->nr_routes) {
        return rs_fail(MFM_E_INVAL, "route must be below nr_routes");
    }
    const bool pack = (cfg->flags & MFM_RUNROUTE_F_PACK) != 0;
    if (nr_channels) {
        *nr_channels = pack ? G.nr_of[route] : cfg->nr_channels;
    }
    if (max_windows) {
        *max_windows = pack ? (uint32_t)G.route[route].windows : cfg->max_windows;
    }
    if (max_runs) {
        *max_runs = (uint32_t)(pack ? G.route[route].runs : G.cap_runs);
    }
    return MFM_OK;
}

int mfm_hosttwin_runroute_sets_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *routes_of_channel, uint32_t flags,
                                    uint32_t window_samples, size_t max_runs, const uint32_t *route_max_runs, const uint32_t *route_max_windows,
                                    const struct mfm_gate_run *gate_runs, const int16_t *gate_payload, const uint64_t *gate_totals,
                                    struct mfm_gate_run *runs, uint64_t *totals, int16_t *payloads, size_t max_elems)
{
    if (!gate_totals || !totals || (!gate_runs && gate_totals[MFM_RUNROUTE_T_RUNS]) || (!runs && max_runs)) {
        return MFM_E_INVAL;
    }
    if (flags & ~MFM_RUNROUTE_F_PACK) {
        return rs_fail(MFM_E_INVAL, "flags must be 0 or MFM_RUNROUTE_F_PACK");
    }
    const bool pack = (flags & MFM_RUNROUTE_F_PACK) != 0;
    char err[192];
    if (const char *m = rs_table_check(nr_channels, nr_routes, routes_of_channel, err, sizeof(err))) {
        return rs_fail(MFM_E_INVAL, m);
    }
    uint32_t *rank = nullptr;
    if (pack) {
        if (!route_max_runs || !route_max_windows || (!gate_payload && gate_totals[MFM_RUNROUTE_T_ELEMS]) || (!payloads && max_elems)) {
            return MFM_E_INVAL;
        }
        if (0 == window_samples || window_samples > (1u << 20)) {
            return rs_fail(MFM_E_INVAL, "window_samples must be 1 .. 2^20, the gate's");
        }
        for (uint32_t k = 0; k < nr_routes; k++) {
            if ((uint64_t)route_max_windows[k] * window_samples > max_elems || route_max_runs[k] > max_runs) {
                return rs_fail(MFM_E_INVAL, "a route's capacity exceeds the row it is given: max_runs records, max_elems elements");
            }
        }
        rank = new (std::nothrow) uint32_t[(size_t)nr_channels * nr_routes];
        if (!rank) {
            return MFM_E_NOMEM;
        }
        uint32_t count[RS_K];
        mfm_runroute_build_ranks(routes_of_channel, nr_channels, nr_routes, rank, count);
    }
    uint64_t over, oos;
    bool refused = mfm_runroute_refused(gate_totals, max_runs, over, oos);
    const uint64_t n = refused ? 0u : gate_totals[MFM_RUNROUTE_T_RUNS];
    for (uint64_t r = 0; r < n && !refused; r++) {
        if (mfm_runroute_bad_channel(gate_runs[r].channel, nr_channels) ||
            (pack && mfm_runroute_bad_range(gate_runs[r].payload_offset, gate_runs[r].nr_windows, window_samples, gate_totals[MFM_RUNROUTE_T_ELEMS]))) {
            refused = true;
            oos = 1u;
        }
    }
    for (uint32_t k = 0; k < nr_routes; k++) {
        uint64_t *t = totals + 4u * k;
        t[MFM_RUNROUTE_T_RUNS] = 0;
        t[MFM_RUNROUTE_T_ELEMS] = refused || pack ? 0u : gate_totals[MFM_RUNROUTE_T_ELEMS];
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
        if (pack && mfm_runroute_route_over(count, windows, route_max_runs[k], route_max_windows[k])) {
            t[MFM_RUNROUTE_T_OVERFLOW] = 1u;
            continue;
        }
        mfm_gate_run *row = runs + (size_t)k * max_runs;
        int16_t *pay = pack ? payloads + (size_t)k * max_elems : nullptr;
        uint64_t at = 0, elems = 0;
        for (uint64_t r = 0; r < n; r++) {
            const mfm_gate_run &g = gate_runs[r];
            if (!mfm_runroute_in_route(mfm_runroute_set_of(routes_of_channel, nr_channels, g.channel), k)) {
                continue;
            }
            row[at] = g;
            if (pack) {
                const uint64_t len = (uint64_t)g.nr_windows * window_samples;
                row[at].channel = mfm_runroute_rank_of(rank, nr_routes, g.channel, k);
                row[at].payload_offset = elems;
                if (len) {
                    memcpy(pay + elems, gate_payload + g.payload_offset, len * sizeof(int16_t));
                }
                elems += len;
            }
            at++;
        }
        t[MFM_RUNROUTE_T_RUNS] = count;
        if (pack) {
            t[MFM_RUNROUTE_T_ELEMS] = elems;
        }
    }
    delete[] rank;
    return MFM_OK;
}

} /* extern "C" */
