/*
 * mfm_run_ends.hip - the stretch-end report of the burst stages: which of the states a call holds are the end of a stretch
 * (mfm_run_ends.h states the rule and the records), as one dense list in run order.  Launched only with the report on, behind a
 * stage's walk kernel and in front of its state kernel; the stages' own launches and buffers are untouched.
 *
 *   re_place_kernel   one block.  A run's records (0, 1 or 2) from runs[r], runs[r + 1] and the state its channel started the
 *                     call with, a run per thread and step, left in base[r]; then a thread sums a stretch of them, the
 *                     exclusive scan gives every run its first record and the sums the two totals (the records with
 *                     mode != 0 ride in the upper half of the scanned word).
 *   re_write_kernel   AIS and FLEX: one thread per run writes the run's records at its base.
 *   re_write_pocsag_kernel   one wave per run: lane z < 16 corrects batch word z with the stage's BCH tables, a ballot gives
 *                     fail_mask and nr_ok, lane 0 writes the rest of the record.
 *   re_flush_place_kernel, re_flush_write_kernel, re_flush_write_pocsag_kernel   the end call, the same over the channels
 *                     with a stretch; the write kernel zeroes the channel's state behind its record, the place kernel the
 *                     stage's totals.
 *
 * Every launch is sized from the capacities fixed at create; surplus threads return after reading the control words.  Nothing
 * is floating point, no atomic is used, and a record's place is the scan's.
 */
#include <hip/hip_runtime.h>


#include "mfm_run_ends.h"

static_assert(sizeof(mfm_runais_end) == 48 && sizeof(mfm_runpocsag_end) == 184 && sizeof(mfm_runflex_end) == 64, "the stretch-end records");
static_assert(offsetof(mfm_runpocsag_end, raw) == 56 && offsetof(mfm_runpocsag_end, corrected) == 120, "struct mfm_runpocsag_end");

namespace {

constexpr uint32_t RE_WRITE_THREADS = 256;

template <class State>
struct ReCall {
    const mfm_runrs_run *runs;
    const State *chan_old;
    const State *run_state;
    const uint32_t *ctl;
    const MfmBchTables *bch;
    uint32_t *base;
    void *ends;
    uint64_t *end_totals;
    uint32_t C, cap_runs;
};

template <class State>
struct ReFlush {
    State *chan;
    uint64_t *totals;
    const MfmBchTables *bch;
    uint32_t *base;
    void *ends;
    uint64_t *end_totals;
    uint32_t C;
};

/* records of run r in the low half, those with mode != 0 in the high half */
template <class State>
__device__ __forceinline__ uint64_t re_count(const ReCall<State> &A, uint64_t r, uint64_t n)
{
    const uint32_t c = A.runs[r].channel; /* < C: the plan checked the list */
    const State *old = &A.chan_old[c];
    const uint32_t what = mfm_run_ends_of_run(A.runs, r, n, old->has_stretch);
    uint64_t k = 0;
    if (what & MFM_RUN_ENDS_A) {
        k += 1u + ((uint64_t)(old->mode != 0u) << 32);
    }
    if (what & MFM_RUN_ENDS_B) {
        k += 1u + ((uint64_t)(A.run_state[r].mode != 0u) << 32);
    }
    return k;
}

template <class State>
__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void re_place_kernel(const ReCall<State> A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    const uint32_t n = A.ctl[1]; /* 0 for a refused call; at most cap_runs */
    /* the counts, a run per thread and step (neighbouring threads read neighbouring runs, no step waits for another): they wait
     * in base[r], records in bits 0 - 1 and those with mode != 0 in bits 2 - 3 */
    for (uint32_t r = threadIdx.x; r < n; r += MFM_RUN_SCAN_THREADS) {
        const uint64_t k = re_count(A, r, n);
        A.base[r] = (uint32_t)k | ((uint32_t)(k >> 32) << 2);
    }
    __syncthreads(); /* one block: what it wrote is what it reads */
    uint32_t r0, r1;
    mfm_run_slice(n, &r0, &r1);
    uint64_t s = 0;
#pragma unroll 1
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t k = A.base[r];
        s += (k & 3u) | ((uint64_t)(k >> 2) << 32);
    }
    uint64_t total;
    uint64_t base = mfm_run_block_scan(s, lds, &total); /* fewer than 2^28 runs of two records: the halves do not meet */
#pragma unroll 1
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t k = A.base[r];
        A.base[r] = (uint32_t)base;
        base += k & 3u;
    }
    if (threadIdx.x == 0) {
        A.end_totals[0] = total & 0xffffffffull; /* at most n: a channel's first run has no (b) of a run in front of it */
        A.end_totals[1] = total >> 32;
    }
}

__device__ __forceinline__ void re_record(const mfm_runais_state &s, uint32_t c, uint32_t run, mfm_runais_end &e)
{
    mfm_runais_end_of(s, c, run, e);
}

__device__ __forceinline__ void re_record(const mfm_runflex_state &s, uint32_t c, uint32_t run, mfm_runflex_end &e)
{
    mfm_runflex_end_of(s, c, run, e);
}

template <class State, class End>
__global__ __launch_bounds__(RE_WRITE_THREADS) void re_write_kernel(const ReCall<State> A)
{
    const uint32_t n = A.ctl[1];
    const uint32_t r = blockIdx.x * RE_WRITE_THREADS + threadIdx.x;
    if (r >= n) { /* surplus threads, and every thread of a refused call */
        return;
    }
    const uint32_t c = A.runs[r].channel;
    const uint32_t what = mfm_run_ends_of_run(A.runs, r, n, A.chan_old[c].has_stretch);
    End *out = static_cast<End *>(A.ends) + A.base[r]; /* base + records <= n <= the capacity */
    if (what & MFM_RUN_ENDS_A) {
        re_record(A.chan_old[c], c, r, *out);
        out++;
    }
    if (what & MFM_RUN_ENDS_B) {
        re_record(A.run_state[r], c, r + 1u, *out);
    }
}

/* one wave, one record: lane z < 16 holds word z */
__device__ __forceinline__ void re_pocsag_record(const MfmBchTables *bch, const mfm_runpocsag_state &s, uint32_t c, uint32_t run,
                                                 mfm_runpocsag_end *e)
{
    const uint32_t lane = threadIdx.x;
    uint32_t fail = 0, fixed = 0;
    if (lane < 16u) {
        fixed = mfm_runpocsag_end_word(bch, s, lane, &fail);
    }
    const uint32_t mask = (uint32_t)__ballot(fail != 0u); /* lanes 0 .. 15 only */
    if (lane < 16u) {
        e->raw[lane] = s.batch[lane];
        e->corrected[lane] = fixed;
    }
    if (lane == 0) {
        mfm_runpocsag_end_head(s, c, run, mask, *e);
    }
}

__global__ __launch_bounds__(64) void re_write_pocsag_kernel(const ReCall<mfm_runpocsag_state> A)
{
    const uint32_t n = A.ctl[1];
    const uint32_t r = blockIdx.x;
    if (r >= n) {
        return;
    }
    const uint32_t c = A.runs[r].channel;
    const uint32_t what = mfm_run_ends_of_run(A.runs, r, n, A.chan_old[c].has_stretch);
    mfm_runpocsag_end *out = static_cast<mfm_runpocsag_end *>(A.ends) + A.base[r];
    if (what & MFM_RUN_ENDS_A) {
        re_pocsag_record(A.bch, A.chan_old[c], c, r, out);
        out++;
    }
    if (what & MFM_RUN_ENDS_B) {
        re_pocsag_record(A.bch, A.run_state[r], c, r + 1u, out);
    }
}

/* ---- the end call --------------------------------------------------------------------------------------------------- */

template <class State>
__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void re_flush_place_kernel(const ReFlush<State> A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t c0, c1;
    mfm_run_slice<uint64_t>(A.C, &c0, &c1);
    uint64_t s = 0;
#pragma unroll 1
    for (uint64_t c = c0; c < c1; c++) {
        s += A.chan[c].has_stretch ? 1u + ((uint64_t)(A.chan[c].mode != 0u) << 32) : 0u;
    }
    uint64_t total;
    uint64_t base = mfm_run_block_scan(s, lds, &total);
#pragma unroll 1
    for (uint64_t c = c0; c < c1; c++) {
        A.base[c] = (uint32_t)base;
        base += A.chan[c].has_stretch ? 1u : 0u;
    }
    if (threadIdx.x < 4) { /* the end call replaces the previous result: no event, no flag */
        A.totals[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) {
        A.end_totals[0] = total & 0xffffffffull;
        A.end_totals[1] = total >> 32;
    }
}

template <class State, class End>
__global__ __launch_bounds__(RE_WRITE_THREADS) void re_flush_write_kernel(const ReFlush<State> A)
{
    const uint32_t c = blockIdx.x * RE_WRITE_THREADS + threadIdx.x;
    if (c >= A.C) {
        return;
    }
    State *st = &A.chan[c];
    if (!st->has_stretch) { /* all zero already (the stages' state checks say so) */
        return;
    }
    re_record(*st, c, MFM_RUN_ENDS_NO_RUN, static_cast<End *>(A.ends)[A.base[c]]);
    *st = State{};
}

__global__ __launch_bounds__(64) void re_flush_write_pocsag_kernel(const ReFlush<mfm_runpocsag_state> A)
{
    const uint32_t c = blockIdx.x; /* the grid is C */
    mfm_runpocsag_state *st = &A.chan[c];
    if (!st->has_stretch) {
        return;
    }
    re_pocsag_record(A.bch, *st, c, MFM_RUN_ENDS_NO_RUN, static_cast<mfm_runpocsag_end *>(A.ends) + A.base[c]);
    __syncthreads(); /* one wave: every lane has read what it needs of the state */
    uint32_t *w = reinterpret_cast<uint32_t *>(st);
    for (uint32_t i = threadIdx.x; i < sizeof(mfm_runpocsag_state) / 4u; i += 64u) {
        w[i] = 0;
    }
}

size_t re_record_bytes(int stage)
{
    return stage == MFM_RUN_ENDS_AIS ? sizeof(mfm_runais_end) : stage == MFM_RUN_ENDS_POCSAG ? sizeof(mfm_runpocsag_end) : sizeof(mfm_runflex_end);
}

template <class State, class End>
void re_launch_process(const MfmRunEnds *e, const MfmRunEndsCall *c, hipStream_t s)
{
    const ReCall<State> A{ c->runs, static_cast<const State *>(c->chan_old), static_cast<const State *>(c->run_state), c->ctl, c->bch,
                           e->d_base, e->d_ends, e->d_end_totals, c->C, c->cap_runs };
    hipLaunchKernelGGL(re_place_kernel<State>, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    if constexpr (sizeof(End) == sizeof(mfm_runpocsag_end)) {
        hipLaunchKernelGGL(re_write_pocsag_kernel, dim3(c->cap_runs), dim3(64), 0, s, A);
    } else {
        hipLaunchKernelGGL((re_write_kernel<State, End>), dim3((c->cap_runs + RE_WRITE_THREADS - 1u) / RE_WRITE_THREADS), dim3(RE_WRITE_THREADS), 0,
                           s, A);
    }
}

template <class State, class End>
void re_launch_flush(const MfmRunEnds *e, void *chan, uint64_t *totals, const MfmBchTables *bch, uint32_t C, hipStream_t s)
{
    const ReFlush<State> A{ static_cast<State *>(chan), totals, bch, e->d_base, e->d_ends, e->d_end_totals, C };
    hipLaunchKernelGGL(re_flush_place_kernel<State>, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    if constexpr (sizeof(End) == sizeof(mfm_runpocsag_end)) {
        hipLaunchKernelGGL(re_flush_write_pocsag_kernel, dim3(C), dim3(64), 0, s, A);
    } else {
        hipLaunchKernelGGL((re_flush_write_kernel<State, End>), dim3((C + RE_WRITE_THREADS - 1u) / RE_WRITE_THREADS), dim3(RE_WRITE_THREADS), 0, s, A);
    }
}

} /* namespace */

extern "C" {

int mfm_internal_run_ends_set(MfmRunEnds *e, int stage, bool on, size_t max_runs, size_t nr_channels)
{
    if (on == e->on) {
        return MFM_OK;
    }
    if (!on) {
        (void)hipFree(e->d_ends);
        (void)hipFree(e->d_end_totals);
        (void)hipFree(e->d_base);
        *e = MfmRunEnds{};
        return MFM_OK;
    }
    /* a process call holds at most max_runs records, an end call at most nr_channels */
    e->cap = max_runs > nr_channels ? max_runs : nr_channels;
    MFM_RUN_TRY(hipMalloc(&e->d_ends, e->cap * re_record_bytes(stage)));
    MFM_RUN_TRY(hipMalloc(&e->d_end_totals, 2 * 8));
    MFM_RUN_TRY(hipMemset(e->d_end_totals, 0, 2 * 8));
    MFM_RUN_TRY(hipMalloc(&e->d_base, e->cap * 4));
    MFM_RUN_TRY(hipDeviceSynchronize());
    e->on = true;
    return MFM_OK;
}

int mfm_internal_run_ends_process(MfmRunEnds *e, int stage, const MfmRunEndsCall *call, hipStream_t s)
{
    if (stage == MFM_RUN_ENDS_AIS) {
        re_launch_process<mfm_runais_state, mfm_runais_end>(e, call, s);
    } else if (stage == MFM_RUN_ENDS_POCSAG) {
        re_launch_process<mfm_runpocsag_state, mfm_runpocsag_end>(e, call, s);
    } else {
        re_launch_process<mfm_runflex_state, mfm_runflex_end>(e, call, s);
    }
    MFM_RUN_TRY(hipGetLastError());
    return MFM_OK;
}

int mfm_internal_run_ends_flush(MfmRunEnds *e, int stage, void *chan, uint64_t *totals, const MfmBchTables *bch, uint32_t C, hipStream_t s)
{
    if (stage == MFM_RUN_ENDS_AIS) {
        re_launch_flush<mfm_runais_state, mfm_runais_end>(e, chan, totals, bch, C, s);
    } else if (stage == MFM_RUN_ENDS_POCSAG) {
        re_launch_flush<mfm_runpocsag_state, mfm_runpocsag_end>(e, chan, totals, bch, C, s);
    } else {
        re_launch_flush<mfm_runflex_state, mfm_runflex_end>(e, chan, totals, bch, C, s);
    }
    MFM_RUN_TRY(hipGetLastError());
    return MFM_OK;
}

int mfm_internal_run_ends_fetch(MfmRunEnds *e, int stage, void *out, size_t max, size_t *nr)
{
    uint64_t t[2];
    MFM_RUN_TRY(hipMemcpy(t, e->d_end_totals, sizeof(t), hipMemcpyDeviceToHost));
    *nr = (size_t)t[0];
    if (t[0] > max) {
        return MFM_E_NOMEM;
    }
    if (t[0]) {
        MFM_RUN_TRY(hipMemcpy(out, e->d_ends, (size_t)t[0] * re_record_bytes(stage), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

} /* extern "C" */
