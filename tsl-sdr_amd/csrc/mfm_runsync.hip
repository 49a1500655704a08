/*
 * mfm_runsync.hip - the burst sync stage: the decisions the burst Mueller-Muller stage left in its dense payload become one bit
 * each, and wherever the last 32 bits of a stretch are a sync word of the table, or nearly one, an event
 * (pager/test/test_mueller_muller.c:130-136, with a table and the complement).  See include/multifm_hip.h for the boundary and
 * the result, mfm_runsync.h for the bit, the register and the match, and mfm_run_stage.h for the checks of a run.
 *
 * The input is what mfm_runmm_device_view returns; how many runs and decisions a call carries is read on the device, so the host
 * never waits and every launch is sized from the capacities fixed at create.  There is no feedback: the verdict on a decision
 * needs the 31 decisions before it and nothing else, so the parallelism is the number of decisions.
 *
 *   rsy_plan_kernel    one block.  Every run is checked (mfm_run_check_run, and dec_offset against the running sum) before a
 *                      decision is read; exclusive scans of the runs' bit words and of their segments of MFM_RUNSYNC_SEGMENT
 *                      decisions; the run records but for nr_events; a channel's last run leaves its index for the state kernel.
 *   rsy_match_kernel   one wave per segment, found by bisection in the segment scan.  64 consecutive decisions a step, two bytes
 *                      a lane in one coalesced load: the wave's ballot over the bit is the run's next two words as they stand in
 *                      the result.  A lane's register is a funnel of those two words and the word in front, reversed; the word in
 *                      front of a run is the carried register or 0, the word in front of a later segment a ballot over the run's
 *                      32 decisions before it.  Every lane holds its register against the table; the segment's count of matches.
 *   rsy_scan_kernel    one block: exclusive scan of the segments' counts, the events of every run, the total against max_events.
 *   rsy_place_kernel   one wave per segment that has a match: the registers again, from the bit words this time (1/16 of the
 *                      bytes), and every match to the segment's base plus its rank among the wave's matches.
 *   rsy_state_kernel   one lane per channel: the register after the last decision of the channel's last run, from the bit words,
 *                      into the OTHER of two state buffers; a channel without a run, and every channel of a refused call, copies
 *                      its state over.
 *
 * No atomic decides a placement, nothing is a float and nothing is read behind a run.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_runsync.h"

static_assert(sizeof(mfm_runsync_run) == 40 && offsetof(mfm_runsync_run, first_dec) == 16 && offsetof(mfm_runsync_run, nr_events) == 36,
              "struct mfm_runsync_run is 40 bytes");
static_assert(sizeof(mfm_runsync_event) == 32 && offsetof(mfm_runsync_event, channel) == 8 && offsetof(mfm_runsync_event, inverted) == 28,
              "struct mfm_runsync_event is 32 bytes");

namespace {

constexpr uint32_t RSY_T_RUNS = 0, RSY_T_EVENTS = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RSY_SEG = MFM_RUNSYNC_SEGMENT;    /* decisions of a run one wave takes */
constexpr uint32_t RSY_CTL_RUNS = 0, RSY_CTL_SEGS = 1, RSY_CTL_WORDS = 2, RSY_NR_CTL = 3; /* 0 for a refused call */
static_assert(RSY_SEG % 64u == 0, "a segment is whole steps of the wave, and begins on a word of its run");

struct RsyCall {
    const mfm_runsync_in_run *runs;
    const int16_t *decs;
    const uint64_t *mtotals;
    const mfm_runsync_state *chan_old;
    mfm_runsync_state *chan_new;
    mfm_runsync_run *out_runs;  /* [cap_runs] */
    uint32_t *seg_base;         /* [cap_runs] first segment of a run */
    uint32_t *chan_last;        /* [C] */
    uint32_t *ctl;              /* [RSY_NR_CTL] */
    uint64_t *totals;
    uint32_t *bits;             /* [cap_decs / 32 + cap_runs] */
    uint32_t *count;            /* [cap_segs] matches of a segment */
    uint32_t *ev_base;          /* [cap_segs + 1] first event of a segment */
    mfm_runsync_event *events;  /* [cap_events] */
    uint32_t C, cap_runs, cap_decs, cap_events;
    mfm_runsync_params P;
};

__device__ __forceinline__ uint32_t rsy_words(uint32_t nr_dec)
{
    return (nr_dec + 31u) / 32u; /* nr_dec < 2^31 (the capacity) */
}

__device__ __forceinline__ uint32_t rsy_segs(uint32_t nr_dec)
{
    return (nr_dec + RSY_SEG - 1u) / RSY_SEG;
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rsy_plan_kernel(const RsyCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t n, E, over, err, r0, r1;
    mfm_runsync_totals_check(A.mtotals, A.cap_decs, A.cap_runs, &n, &E, &over, &err);
    if (over || err) { /* nothing may be read */
        if (threadIdx.x == 0) {
            A.totals[RSY_T_RUNS] = 0;
            A.totals[RSY_T_EVENTS] = 0;
            A.totals[MFM_RUN_T_OVERFLOW] = over;
            A.totals[MFM_RUN_T_INPUT] = err;
            for (uint32_t i = 0; i < RSY_NR_CTL; i++) {
                A.ctl[i] = 0;
            }
        }
        return;
    }
    mfm_run_slice(n, &r0, &r1);
    const mfm_runsync_state_outs *state = reinterpret_cast<const mfm_runsync_state_outs *>(A.chan_old);
    uint64_t sd = 0, sw = 0, sg = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        const mfm_runrs_run run = A.runs[r];
        bad |= mfm_run_check_run(run, r ? &A.runs[r - 1] : nullptr, A.C, E, state);
        sd += run.nr_out;
        /* a run that passed the check has at most E <= cap_decs < 2^31 decisions; one that did not is never packed */
        sw += ((uint64_t)run.nr_out + 31u) / 32u;
        sg += ((uint64_t)run.nr_out + RSY_SEG - 1u) / RSY_SEG;
    }
    /* fewer than 2^28 runs of fewer than 2^32 decisions: every sum stays below 2^63 */
    uint64_t td, tw, tg;
    uint64_t bd = mfm_run_block_scan(sd, lds, &td);
    uint64_t bw = mfm_run_block_scan(sw, lds, &tw);
    uint64_t bg = mfm_run_block_scan(sg, lds, &tg);
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) { /* the payload is dense: a run's decisions stand behind those of the runs in front */
        bad |= A.runs[r].out_offset != bd ? MFM_RUNSYNC_IN_BAD_RUNS : 0u;
        bd += A.runs[r].nr_out;
    }
    if (__syncthreads_or((bad & MFM_RUNSYNC_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNSYNC_IN_OUT_OF_STEP;
    }
    if (__syncthreads_or((bad & MFM_RUNSYNC_IN_BAD_RUNS) != 0)) {
        err |= MFM_RUNSYNC_IN_BAD_RUNS;
    }
    const bool refused = err != 0;
    if (!refused) { /* the ranges are the running sum and end within E: td <= E <= cap_decs, so words and segments fit 32 bits */
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t nr_dec = A.runs[r].nr_out, c = A.runs[r].channel;
            mfm_runsync_run *o = &A.out_runs[r];
            o->first_window = A.runs[r].first_window;
            o->word_offset = bw;
            o->first_dec = A.runs[r].first_out;
            o->channel = c;
            o->nr_dec = nr_dec;
            o->flags = A.runs[r].flags & MFM_RUNRS_BEGINS;
            o->nr_events = 0; /* the event scan */
            A.seg_base[r] = (uint32_t)bg;
            bw += rsy_words(nr_dec);
            bg += rsy_segs(nr_dec);
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RSY_T_RUNS] = refused ? 0u : n;
        A.totals[RSY_T_EVENTS] = 0; /* the event scan */
        A.totals[MFM_RUN_T_OVERFLOW] = 0;
        A.totals[MFM_RUN_T_INPUT] = err;
        A.ctl[RSY_CTL_RUNS] = refused ? 0u : (uint32_t)n;
        A.ctl[RSY_CTL_SEGS] = refused ? 0u : (uint32_t)tg;
        A.ctl[RSY_CTL_WORDS] = refused ? 0u : (uint32_t)tw;
    }
}

/* the run of segment s: the last r with seg_base[r] <= s (a run without a decision has no segment and shares its base with the
 * run behind it) */
__device__ __forceinline__ uint32_t rsy_run_of(const uint32_t *seg_base, uint32_t n_runs, uint32_t s)
{
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_base[mid] <= s) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

/* the word in front of a run's first: the carried register as packed bits, or nothing */
__device__ __forceinline__ uint32_t rsy_seed(const mfm_runsync_state *chan_old, const mfm_runsync_run &run)
{
    return (run.flags & MFM_RUNRS_BEGINS) ? 0u : mfm_runsync_reverse(chan_old[run.channel].shr);
}

/* lane's register after its decision of a step: prev is the word in front of the step's two words lo and hi */
__device__ __forceinline__ uint32_t rsy_lane_register(uint32_t prev, uint32_t lo, uint32_t hi, uint32_t lane)
{
    const uint32_t win = lane < 32u ? mfm_runsync_window(prev, lo, lane + 1u) : mfm_runsync_window(lo, hi, lane - 31u);
    return mfm_runsync_reverse(win);
}

__global__ __launch_bounds__(64) void rsy_match_kernel(const RsyCall A)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= A.ctl[RSY_CTL_SEGS]) { /* surplus waves: the launch is sized from the capacity; 0 for a refused call */
        return;
    }
    const uint32_t r = rsy_run_of(A.seg_base, A.ctl[RSY_CTL_RUNS], s);
    const mfm_runsync_run run = A.out_runs[r];
    const uint32_t nd = run.nr_dec, nw = rsy_words(nd);
    const uint32_t j0 = (s - A.seg_base[r]) * RSY_SEG; /* below nd: the segment exists */
    const int16_t *d = A.decs + A.runs[r].out_offset; /* [out_offset, out_offset + nd) lies within the totals (the plan) */
    uint32_t *bits = A.bits + run.word_offset;
    const mfm_runsync_params P = A.P;
    uint32_t prev;
    if (j0 == 0u) {
        prev = rsy_seed(A.chan_old, run);
    } else { /* the 32 decisions in front of the segment: j0 >= RSY_SEG */
        const bool b = lane < 32u && mfm_runsync_bit(d[j0 - 32u + lane], P.bit_rule) != 0u;
        prev = (uint32_t)__ballot(b);
    }
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint32_t jb = j0; jb < j0 + RSY_SEG && jb < nd; jb += 64u) {
        const uint32_t j = jb + lane;
        const bool in = j < nd;
        const bool b = in && mfm_runsync_bit(d[in ? j : jb], P.bit_rule) != 0u;
        const uint64_t m = __ballot(b);
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        const uint32_t wi = jb / 32u + lane;
        if (lane < 2u && wi < nw) { /* the bits at and above nd are 0: `in` */
            bits[wi] = lane ? hi : lo;
        }
        const uint32_t shr = rsy_lane_register(prev, lo, hi, lane);
        uint32_t k, dist, inv;
        const bool hit = in && mfm_runsync_match(shr, P, &k, &dist, &inv);
        cnt += (uint32_t)__popcll(__ballot(hit));
        prev = hi;
    }
    if (lane == 0u) {
        A.count[s] = cnt;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rsy_scan_kernel(const RsyCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    const uint32_t n = A.ctl[RSY_CTL_RUNS], nseg = A.ctl[RSY_CTL_SEGS]; /* 0 for a refused call */
    const uint64_t total = mfm_run_count_scan(A.count, A.ev_base, nseg, lds); /* at most one a decision: below 2^31 */
    if (threadIdx.x == 0) {
        A.ev_base[nseg] = (uint32_t)total;
    }
    __threadfence_block();
    __syncthreads(); /* every thread has read ctl, and the bases stand */
    const bool over = total > A.cap_events;
    if (!over) {
        uint32_t r0, r1;
        mfm_run_slice(n, &r0, &r1);
#pragma unroll 1
        for (uint32_t r = r0; r < r1; r++) { /* a run's segments are consecutive, and so are their events */
            const uint32_t s0 = A.seg_base[r], s1 = r + 1u < n ? A.seg_base[r + 1u] : nseg;
            A.out_runs[r].nr_events = A.ev_base[s1] - A.ev_base[s0];
        }
    }
    if (threadIdx.x == 0 && n != 0u) {
        if (over) { /* by the count, before an event is placed */
            A.totals[RSY_T_RUNS] = 0;
            A.totals[MFM_RUN_T_OVERFLOW] = MFM_RUNSYNC_OVER_EVENTS;
            for (uint32_t i = 0; i < RSY_NR_CTL; i++) {
                A.ctl[i] = 0;
            }
        } else {
            A.totals[RSY_T_EVENTS] = total;
        }
    }
}

__global__ __launch_bounds__(64) void rsy_place_kernel(const RsyCall A)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= A.ctl[RSY_CTL_SEGS] || A.count[s] == 0u) { /* surplus waves, a refused call, a segment without a match */
        return;
    }
    const uint32_t r = rsy_run_of(A.seg_base, A.ctl[RSY_CTL_RUNS], s);
    const mfm_runsync_run run = A.out_runs[r];
    const uint32_t nd = run.nr_dec, nw = rsy_words(nd);
    const uint32_t j0 = (s - A.seg_base[r]) * RSY_SEG;
    const uint32_t *bits = A.bits + run.word_offset;
    const mfm_runsync_params P = A.P;
    uint32_t prev = j0 == 0u ? rsy_seed(A.chan_old, run) : bits[j0 / 32u - 1u];
    uint32_t at = A.ev_base[s]; /* at + the segment's count <= the total <= cap_events (the scan) */
#pragma unroll 1
    for (uint32_t jb = j0; jb < j0 + RSY_SEG && jb < nd; jb += 64u) {
        const uint32_t j = jb + lane, w = jb / 32u;
        const uint32_t lo = bits[w], hi = w + 1u < nw ? bits[w + 1u] : 0u; /* w < nw: jb < nd */
        const uint32_t shr = rsy_lane_register(prev, lo, hi, lane);
        uint32_t k = 0, dist = 0, inv = 0;
        const bool hit = j < nd && mfm_runsync_match(shr, P, &k, &dist, &inv);
        const uint64_t h = __ballot(hit);
        if (hit) {
            mfm_runsync_event e;
            e.dec = run.first_dec + j;
            e.channel = run.channel;
            e.run = r;
            e.seen = shr;
            e.word_index = k;
            e.distance = dist;
            e.inverted = inv;
            A.events[at + (uint32_t)__popcll(h & ((1ull << lane) - 1ull))] = e;
        }
        at += (uint32_t)__popcll(h);
        prev = hi;
    }
}

__global__ __launch_bounds__(256) void rsy_state_kernel(const RsyCall A)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= A.C) {
        return;
    }
    const uint32_t last = A.chan_last[c];
    A.chan_last[c] = MFM_RUN_NONE; /* for the next call */
    const bool refused = A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0;
    const mfm_runsync_state old = A.chan_old[c];
    mfm_runsync_state st = old; /* a channel without a run, a refused call: the state stays */
    if (last != MFM_RUN_NONE && !refused) {
        const mfm_runsync_run run = A.out_runs[last];
        st = mfm_runsync_start(old, run.first_window, run.flags);
        if (run.nr_dec) {
            const uint32_t seed = (run.flags & MFM_RUNRS_BEGINS) ? 0u : mfm_runsync_reverse(old.shr);
            st.shr = mfm_runsync_register_at(A.bits + run.word_offset, rsy_words(run.nr_dec), seed, run.nr_dec - 1u);
            st.decs += run.nr_dec;
        }
    }
    A.chan_new[c] = st;
}

/* what create checks without a device; the table and the event capacity with the default filled in */
int rsy_geometry(const mfm_runsync_config &cfg, mfm_runsync_params *P, uint64_t *cap_events)
{
    struct { /* what the burst stages share of their configurations; the capacities are held against the limits below */
        uint32_t abi_version, nr_channels, max_runs, max_out_samples, flags;
    } common = { cfg.abi_version, cfg.nr_channels, 1u, 1u, 0u };
    const int rc = mfm_run_geometry(common);
    if (rc != MFM_OK) {
        return rc;
    }
    if (const char *why = mfm_runsync_params_check(cfg, P)) {
        return mfm_run_fail(MFM_E_INVAL, why);
    }
    if (0 == cfg.max_runs || 0 == cfg.max_decisions || cfg.max_runs >= MFM_RUN_MAX_RUNS || cfg.max_decisions >= MFM_RUN_MAX_OUT ||
        cfg.max_events >= MFM_RUN_MAX_OUT) {
        return mfm_run_fail(MFM_E_INVAL, "max_runs must be 1 .. 2^28 - 1, max_decisions 1 .. 2^31 - 1 and max_events below 2^31: the burst Mueller-Muller stage's capacities (mfm_runmm_get_capacity)");
    }
    *cap_events = cfg.max_events ? cfg.max_events : cfg.max_decisions;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *rsy_refusal(uint64_t over, uint64_t err)
{
    if (err & MFM_RUNSYNC_IN_RUNMM) {
        return "the burst Mueller-Muller stage's call raised overflow or an input error";
    }
    if (err & MFM_RUNSYNC_IN_BAD_RUNS) {
        return "the run list is not a burst Mueller-Muller stage's: a run names a channel that does not exist, channels do not ascend, or a dec_offset is not the running sum of nr_dec or ends past the totals";
    }
    if (err & MFM_RUNSYNC_IN_OUT_OF_STEP) {
        return "out of step with the burst Mueller-Muller stage: a continuing run does not follow on its channel's stretch";
    }
    if (over & MFM_RUNSYNC_OVER_RUNS) {
        return "the call has more runs than max_runs";
    }
    if (over & MFM_RUNSYNC_OVER_DECISIONS) {
        return "the call has more decisions than max_decisions";
    }
    return "the call's events exceed max_events";
}

} /* namespace */

struct mfm_runsync {
    mfm_runsync_config cfg{};
    mfm_runsync_params P{};
    uint64_t cap_events = 0, cap_words = 0, cap_segs = 0;
    mfm_runsync_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    mfm_runsync_run *d_out_runs = nullptr;
    uint32_t *d_seg_base = nullptr, *d_chan_last = nullptr, *d_ctl = nullptr, *d_bits = nullptr, *d_count = nullptr, *d_ev_base = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runsync_event *d_events = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
};

extern "C" {

int mfm_runsync_create(struct mfm_runsync **ps, const struct mfm_runsync_config *cfg)
{
    if (!ps || !cfg) {
        return MFM_E_INVAL;
    }
    *ps = nullptr;
    mfm_runsync_params P{};
    uint64_t cap_events = 0;
    const int rc = rsy_geometry(*cfg, &P, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    mfm_runsync *o = new (std::nothrow) mfm_runsync();
    if (!o) {
        return MFM_E_NOMEM;
    }
    o->cfg = *cfg;
    o->P = P;
    o->cap_events = cap_events;
    /* a run owns at most nr_dec / 32 + 1 words and nr_dec / MFM_RUNSYNC_SEGMENT + 1 segments */
    o->cap_words = (uint64_t)cfg->max_decisions / 32u + cfg->max_runs;
    o->cap_segs = (uint64_t)cfg->max_decisions / RSY_SEG + cfg->max_runs;
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    *ps = o; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&o->d_chan[i], C * sizeof(mfm_runsync_state)));
        MFM_RUN_TRY(hipMemset(o->d_chan[i], 0, C * sizeof(mfm_runsync_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&o->d_out_runs, nruns * sizeof(mfm_runsync_run)));
    MFM_RUN_TRY(hipMalloc(&o->d_seg_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(o->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_ctl, 4 * 4));
    MFM_RUN_TRY(hipMemset(o->d_ctl, 0, 4 * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(o->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&o->d_bits, (size_t)o->cap_words * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_count, (size_t)o->cap_segs * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_ev_base, ((size_t)o->cap_segs + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_events, (size_t)cap_events * sizeof(mfm_runsync_event)));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runsync_destroy(struct mfm_runsync **ps)
{
    if (!ps || !*ps) {
        return;
    }
    mfm_runsync *o = *ps;
    (void)hipSetDevice(o->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(o->d_chan[0]);
    (void)hipFree(o->d_chan[1]);
    (void)hipFree(o->d_out_runs);
    (void)hipFree(o->d_seg_base);
    (void)hipFree(o->d_chan_last);
    (void)hipFree(o->d_ctl);
    (void)hipFree(o->d_totals);
    (void)hipFree(o->d_bits);
    (void)hipFree(o->d_count);
    (void)hipFree(o->d_ev_base);
    (void)hipFree(o->d_events);
    delete o;
    *ps = nullptr;
}

int mfm_runsync_process_device(struct mfm_runsync *o, const struct mfm_runmm_run *d_runs, const int16_t *d_decisions, const uint64_t *d_totals,
                               void *stream)
{
    if (!o || !d_runs || !d_decisions || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(o, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = o->cur;
    const RsyCall A{ reinterpret_cast<const mfm_runsync_in_run *>(d_runs), d_decisions, d_totals, o->d_chan[cur], o->d_chan[cur ^ 1u],
                     o->d_out_runs, o->d_seg_base, o->d_chan_last, o->d_ctl, o->d_totals, o->d_bits, o->d_count, o->d_ev_base, o->d_events,
                     o->cfg.nr_channels, o->cfg.max_runs, o->cfg.max_decisions, (uint32_t)o->cap_events, o->P };
    hipLaunchKernelGGL(rsy_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsy_match_kernel, dim3((uint32_t)o->cap_segs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsy_scan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsy_place_kernel, dim3((uint32_t)o->cap_segs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsy_state_kernel, dim3((o->cfg.nr_channels + 255u) / 256u), dim3(256), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(o, s);
    return MFM_OK;
}

int mfm_runsync_fetch(struct mfm_runsync *o, struct mfm_runsync_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits, size_t max_words,
                      size_t *nr_words, struct mfm_runsync_event *events, size_t max_events, size_t *nr_events)
{
    if (!o || !nr_runs || !nr_words || !nr_events || (!runs && max_runs) || (!bits && max_words) || (!events && max_events)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_words = 0;
    *nr_events = 0;
    if (!o->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(o->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(o->last_stream));
    uint64_t t[4];
    uint32_t ctl[RSY_NR_CTL];
    MFM_RUN_TRY(hipMemcpy(t, o->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, rsy_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    MFM_RUN_TRY(hipMemcpy(ctl, o->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    *nr_runs = (size_t)t[RSY_T_RUNS];
    *nr_words = ctl[RSY_CTL_WORDS];
    *nr_events = (size_t)t[RSY_T_EVENTS];
    if (*nr_runs > max_runs || *nr_words > max_words || *nr_events > max_events) {
        return MFM_E_NOMEM;
    }
    if (*nr_runs) {
        MFM_RUN_TRY(hipMemcpy(runs, o->d_out_runs, *nr_runs * sizeof(mfm_runsync_run), hipMemcpyDeviceToHost));
    }
    if (*nr_words) {
        MFM_RUN_TRY(hipMemcpy(bits, o->d_bits, *nr_words * 4, hipMemcpyDeviceToHost));
    }
    if (*nr_events) {
        MFM_RUN_TRY(hipMemcpy(events, o->d_events, *nr_events * sizeof(mfm_runsync_event), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runsync_device_view(struct mfm_runsync *o, const struct mfm_runsync_run **d_runs, const uint32_t **d_bits,
                            const struct mfm_runsync_event **d_events, const uint64_t **d_totals)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (d_runs) {
        *d_runs = o->d_out_runs;
    }
    if (d_bits) {
        *d_bits = o->d_bits;
    }
    if (d_events) {
        *d_events = o->d_events;
    }
    if (d_totals) {
        *d_totals = o->d_totals;
    }
    return MFM_OK;
}

int mfm_runsync_get_capacity(struct mfm_runsync *o, uint32_t *max_runs, uint64_t *max_words, uint64_t *max_events)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = o->cfg.max_runs;
    }
    if (max_words) {
        *max_words = o->cap_words;
    }
    if (max_events) {
        *max_events = o->cap_events;
    }
    return MFM_OK;
}

int mfm_runsync_fetch_state(struct mfm_runsync *o, struct mfm_runsync_state *state, size_t nr_channels)
{
    return mfm_run_fetch_state(o, state, nr_channels);
}

int mfm_hosttwin_runsync_state_check(uint32_t nr_channels, const struct mfm_runsync_state *state)
{
    return mfm_run_state_check(nr_channels, state, "sync", mfm_runsync_state_check);
}

int mfm_runsync_store_state(struct mfm_runsync *o, const struct mfm_runsync_state *state, size_t nr_channels)
{
    return mfm_run_store_state(o, state, nr_channels, mfm_hosttwin_runsync_state_check);
}

/* ---- the host twin: the same plan, the reference's loop one decision at a time ---- */

int mfm_hosttwin_runsync_call(const struct mfm_runsync_config *cfg, struct mfm_runsync_state *state, const struct mfm_runmm_run *mruns,
                              const int16_t *decisions, const uint64_t *totals, struct mfm_runsync_run *out_runs, size_t max_out_runs,
                              size_t *nr_runs, uint32_t *bits, size_t max_out_words, size_t *nr_words, struct mfm_runsync_event *events,
                              size_t max_out_events, size_t *nr_events, uint32_t *flags)
{
    if (!cfg || !state || !totals || !nr_runs || !nr_words || !nr_events || (!out_runs && max_out_runs) || (!bits && max_out_words) ||
        (!events && max_out_events)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_words = 0;
    *nr_events = 0;
    if (flags) {
        *flags = 0;
    }
    mfm_runsync_params P{};
    uint64_t cap_events = 0;
    const int rc = rsy_geometry(*cfg, &P, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    const mfm_runsync_in_run *runs = reinterpret_cast<const mfm_runsync_in_run *>(mruns);
    uint64_t n, E, over, err; /* the plan pass */
    mfm_runsync_totals_check(totals, cfg->max_decisions, cfg->max_runs, &n, &E, &over, &err);
    if (!over && !err) {
        if (!mfm_run_twin_plan(totals, cfg->nr_channels, cfg->max_runs, cfg->max_decisions, reinterpret_cast<const mfm_runsync_state_outs *>(state),
                               runs, decisions, false, [](uint32_t) {}, &n, &over, &err)) {
            return MFM_E_INVAL;
        }
        uint64_t sum = 0; /* the payload is dense */
        for (uint64_t r = 0; r < n; r++) {
            err |= runs[r].out_offset != sum ? MFM_RUNSYNC_IN_BAD_RUNS : 0u;
            sum += runs[r].nr_out;
        }
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, rsy_refusal(over, err));
    }
    /* every run from the state the call started with (only a channel's first run reads it); the state its last run leaves */
    std::vector<mfm_runsync_run> recs(n);
    std::vector<mfm_runsync_state> left(n);
    std::vector<uint32_t> words;
    std::vector<mfm_runsync_event> evs;
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        mfm_runsync_state st = mfm_runsync_start(state[run.channel], run.first_window, run.flags);
        const int16_t *d = decisions + run.out_offset;
        mfm_runsync_run &o = recs[r];
        o.first_window = run.first_window;
        o.word_offset = words.size();
        o.first_dec = st.decs;
        o.channel = run.channel;
        o.nr_dec = run.nr_out;
        o.flags = run.flags & MFM_RUNRS_BEGINS;
        o.nr_events = 0;
        words.resize(words.size() + ((size_t)run.nr_out + 31u) / 32u, 0u);
        for (uint32_t j = 0; j < run.nr_out; j++) {
            const uint32_t bit = mfm_runsync_bit(d[j], P.bit_rule);
            words[(size_t)o.word_offset + j / 32u] |= bit << (j % 32u);
            st.shr = (st.shr << 1) | bit; /* :132 */
            mfm_runsync_event e;
            if (mfm_runsync_match(st.shr, P, &e.word_index, &e.distance, &e.inverted)) { /* :134 */
                e.dec = st.decs + j;
                e.channel = run.channel;
                e.run = (uint32_t)r;
                e.seen = st.shr;
                evs.push_back(e);
                o.nr_events++;
            }
        }
        st.decs += run.nr_out;
        left[r] = st;
    }
    if (evs.size() > cap_events) {
        return mfm_run_twin_refuse(MFM_RUNSYNC_OVER_EVENTS, 0, flags, rsy_refusal(MFM_RUNSYNC_OVER_EVENTS, 0));
    }
    *nr_runs = (size_t)n;
    *nr_words = words.size();
    *nr_events = evs.size();
    if (n > max_out_runs || words.size() > max_out_words || evs.size() > max_out_events) {
        return MFM_E_NOMEM; /* nothing written, the state included */
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            state[runs[r].channel] = left[r];
        }
    }
    if (n) {
        memcpy(out_runs, recs.data(), (size_t)n * sizeof(mfm_runsync_run));
    }
    if (!words.empty()) {
        memcpy(bits, words.data(), words.size() * 4);
    }
    if (!evs.empty()) {
        memcpy(events, evs.data(), evs.size() * sizeof(mfm_runsync_event));
    }
    return MFM_OK;
}

} /* extern "C" */
