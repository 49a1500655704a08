/*
 * mfm_runbatch.hip - the burst batch stage: behind a sync event of the burst sync stage the bit words become POCSAG batches of
 * 16 codewords with their BCH verdicts, and the sync slot behind every batch says whether the transmission goes on
 * (pager/pager_pocsag.c:468-538 at one sample per bit).  See include/multifm_hip.h for the boundary and the result,
 * mfm_runbatch.h for the automaton, the window a word is cut from and the bound on a run's events, and mfm_run_stage.h for the
 * checks of a run.
 *
 * The input is what mfm_runsync_device_view returns; how many runs and events a call carries is read on the device, so the host
 * never waits and every launch is sized from the capacities fixed at create.  The automaton is sequential only in frames, at
 * most nr_dec / 544 + 2 steps a run; what a frame holds is cut and corrected in parallel.
 *
 *   rbt_plan_kernel    one block.  Every run is checked (mfm_run_check_run, and word_offset against the running sum of words)
 *                      before a bit is read; exclusive scans of the runs' sync events and of their slot ranges; a channel's last
 *                      run leaves its index for the state kernel.
 *   rbt_walk_kernel    one wave per run.  The run's sync events are checked, 64 a step; then the automaton
 *                      (mfm_runbatch_walk): SEARCH is a ballot over the events for the first dec >= mark, a slot one window
 *                      and a popcount.  It leaves one descriptor per event in the run's slot range, their count and the
 *                      automaton behind the run's last decision.
 *   rbt_scan_kernel    one block: exclusive scan of the runs' counts, the total against max_events.
 *   rbt_decode_kernel  16 lanes an event, 16 events a block.  A lane of a BATCH cuts its word with the window, from the bit
 *                      words or from `kept` where the frame began in an earlier call; BCH from the tables in LDS; a ballot is
 *                      fail_mask and its trailing zeros nr_ok.  Events go to their scan positions.
 *   rbt_state_kernel   one lane per channel: the automaton its last run left, `kept` packed again from the stream the run
 *                      started with, into the OTHER of two state buffers; a channel without a run, and every channel of a
 *                      refused call, copies its state over.
 *
 * No atomic decides a placement, nothing is a float and nothing is read behind a run.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_bch.h"
#include "mfm_runbatch.h"

namespace {

constexpr uint32_t RBT_T_EVENTS = 0, RBT_T_RUNS = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RBT_CTL_RUNS = 0, RBT_CTL_SLOTS = 1, RBT_CTL_BAD = 2, RBT_NR_CTL = 3; /* 0 for a refused call */
constexpr uint32_t RBT_DECODE_THREADS = 256, RBT_PER_BLOCK = RBT_DECODE_THREADS / 16;

/* what the walk leaves of an event: the decode kernel makes the event of it */
struct RbtSlot {
    uint64_t dec;
    uint32_t type, aux, word_index, inverted, nr_ok, reserved;
};

/* the automaton behind a run's last decision */
struct RbtLeft {
    uint64_t mark;
    uint32_t mode, word_index, inverted, reserved;
};

struct RbtCall {
    const mfm_runbatch_in_run *runs;
    const uint32_t *bits;
    const mfm_runsync_event *sev;
    const uint64_t *stotals;
    const mfm_runbatch_state *chan_old;
    mfm_runbatch_state *chan_new;
    uint32_t *in_base;   /* [cap_runs] first sync event of a run */
    uint32_t *slot_base; /* [cap_runs] first slot of a run */
    uint32_t *count;     /* [cap_runs] events of a run */
    uint32_t *ev_base;   /* [cap_runs + 1] first event of a run */
    RbtLeft *left;       /* [cap_runs] */
    RbtSlot *slots;      /* [cap_slots] */
    uint32_t *chan_last; /* [C] */
    uint32_t *ctl;       /* [RBT_NR_CTL] */
    uint64_t *totals;
    mfm_runbatch_event *events; /* [cap_events] */
    const MfmBchTables *bch;
    uint32_t C, cap_runs, cap_decs, cap_events;
    mfm_runbatch_params P;
};

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rbt_plan_kernel(const RbtCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    /* the sync stage's totals are { runs, events, overflow, input error }: mfm_run_totals_check without a bound on the events,
     * which are no payload of this stage's */
    const uint64_t n = A.stotals[MFM_RUN_RS_RUNS], E = A.stotals[MFM_RUN_RS_ELEMS];
    const bool flagged = A.stotals[MFM_RUN_RS_OVERFLOW] != 0 || A.stotals[MFM_RUN_RS_GATE] != 0;
    const uint64_t over = !flagged && n > A.cap_runs ? MFM_RUNBATCH_OVER_RUNS : 0u;
    uint64_t err = flagged ? MFM_RUNBATCH_IN_RUNSYNC : 0u, r0, r1;
    if (over || err) { /* nothing may be read */
        if (threadIdx.x == 0) {
            A.totals[RBT_T_EVENTS] = 0;
            A.totals[RBT_T_RUNS] = 0;
            A.totals[MFM_RUN_T_OVERFLOW] = over;
            A.totals[MFM_RUN_T_INPUT] = err;
            for (uint32_t i = 0; i < RBT_NR_CTL; i++) {
                A.ctl[i] = 0;
            }
        }
        return;
    }
    const uint64_t cap_words = (uint64_t)A.cap_decs / 32u + A.cap_runs;
    const uint64_t cap_slots = 3u * (uint64_t)(A.cap_decs / MFM_RUNBATCH_FRAME) + 5u * (uint64_t)A.cap_runs;
    mfm_run_slice(n, &r0, &r1);
    const mfm_runbatch_state_outs *state = reinterpret_cast<const mfm_runbatch_state_outs *>(A.chan_old);
    uint64_t sw = 0, se = 0, ss = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        const mfm_runrs_run run = A.runs[r];
        bad |= mfm_run_check_run(run, r ? &A.runs[r - 1] : nullptr, A.C, cap_words, state, true);
        sw += ((uint64_t)run.nr_out + 31u) / 32u;
        se += run.reserved; /* nr_events */
        ss += mfm_runbatch_slots(run.nr_out);
    }
    /* fewer than 2^28 runs of fewer than 2^32 decisions or events: every sum stays below 2^63 */
    uint64_t tw, te, ts;
    uint64_t bw = mfm_run_block_scan(sw, lds, &tw);
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) { /* the bit words are dense: a run's words stand behind those of the runs in front */
        bad |= A.runs[r].out_offset != bw ? MFM_RUNBATCH_IN_BAD_RUNS : 0u;
        bw += ((uint64_t)A.runs[r].nr_out + 31u) / 32u;
    }
    /* the bases are written whatever the checks say (r < n <= cap_runs): a refused call never reads them */
    uint64_t be = mfm_run_block_scan(se, lds, &te);
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        A.in_base[r] = (uint32_t)be;
        be += A.runs[r].reserved;
    }
    uint64_t bs = mfm_run_block_scan(ss, lds, &ts);
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        A.slot_base[r] = (uint32_t)bs;
        bs += mfm_runbatch_slots(A.runs[r].nr_out);
    }
    if (tw > cap_words || ts > cap_slots) { /* more than the sync stage's capacities hold: what is sized from them would not do */
        bad |= MFM_RUNBATCH_IN_BAD_RUNS;
    }
    if (te > E || E >= MFM_RUN_MAX_OUT) { /* the events of the runs are the sync stage's, and those fit 31 bits */
        bad |= MFM_RUNBATCH_IN_BAD_EVENTS;
    }
    if (__syncthreads_or((bad & MFM_RUNBATCH_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNBATCH_IN_OUT_OF_STEP;
    }
    if (__syncthreads_or((bad & MFM_RUNBATCH_IN_BAD_RUNS) != 0)) {
        err |= MFM_RUNBATCH_IN_BAD_RUNS;
    }
    if (__syncthreads_or((bad & MFM_RUNBATCH_IN_BAD_EVENTS) != 0)) {
        err |= MFM_RUNBATCH_IN_BAD_EVENTS;
    }
    const bool refused = err != 0;
    if (!refused) { /* ts <= cap_slots < 2^31 and te <= E < 2^31: the bases stand as they are */
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t c = A.runs[r].channel;
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RBT_T_EVENTS] = 0; /* the event scan */
        A.totals[RBT_T_RUNS] = refused ? 0u : n;
        A.totals[MFM_RUN_T_OVERFLOW] = 0;
        A.totals[MFM_RUN_T_INPUT] = err;
        A.ctl[RBT_CTL_RUNS] = refused ? 0u : (uint32_t)n;
        A.ctl[RBT_CTL_SLOTS] = refused ? 0u : (uint32_t)ts;
        A.ctl[RBT_CTL_BAD] = 0;
    }
}

/* the stream a run starts with: its channel's kept bits where it continues a frame, and its own words */
struct RbtStream {
    const uint32_t *kept, *bits;
    uint32_t nr_kept, nr_dec;
    uint64_t base, end; /* the stream's first decision within the stretch, and the decision behind the run's last */
    uint64_t stretch_window;
    mfm_runbatch_auto a;
};

__device__ __forceinline__ RbtStream rbt_stream(const RbtCall &A, const mfm_runrs_run &run)
{
    RbtStream s;
    const mfm_runbatch_state *old = &A.chan_old[run.channel];
    mfm_runbatch_start(old, run.flags, &s.a, &s.nr_kept);
    s.kept = old->kept; /* read only below nr_kept, which is 0 where the run begins a stretch */
    s.bits = A.bits + run.out_offset;
    s.nr_dec = run.nr_out;
    s.base = run.first_out - s.nr_kept;
    s.end = run.first_out + run.nr_out;
    s.stretch_window = (run.flags & MFM_RUNRS_BEGINS) ? run.first_window : old->stretch_window;
    return s;
}

__global__ __launch_bounds__(64) void rbt_walk_kernel(const RbtCall A)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    if (r >= A.ctl[RBT_CTL_RUNS]) { /* surplus waves: the launch is sized from the capacity; 0 for a refused call */
        return;
    }
    const mfm_runrs_run run = A.runs[r];
    const mfm_runsync_event *ev = A.sev + A.in_base[r]; /* [in_base, in_base + nr_events) lies within the sync stage's total (the plan) */
    const uint32_t ne = run.reserved;
    const mfm_runbatch_params P = A.P;
    bool bad = false;
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < ne; i0 += 64u) { /* before the automaton follows an event */
        const uint32_t i = i0 + lane;
        if (i < ne) {
            const mfm_runsync_event e = ev[i];
            bad = bad || !mfm_runbatch_event_ok(e, i ? &ev[i - 1u] : nullptr, run.first_out, run.nr_out, P.nr_words);
        }
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0u) {
            A.count[r] = 0;
            A.ctl[RBT_CTL_BAD] = 1; /* every wave that writes it writes the same: the scan refuses the call */
        }
        return;
    }
    RbtStream s = rbt_stream(A, run);
    RbtSlot *slots = A.slots + A.slot_base[r];
    const uint32_t room = (uint32_t)mfm_runbatch_slots(run.nr_out);
    uint32_t cursor = 0, at = 0;
    auto find = [&](uint64_t mark, mfm_runsync_event *out) -> bool {
#pragma unroll 1
        while (cursor < ne) { /* the marks ascend, and so does the cursor */
            const uint32_t i = cursor + lane;
            bool hit = false;
            if (i < ne) {
                hit = ev[i].dec >= mark && mfm_runbatch_enabled(P, ev[i].word_index);
            }
            const uint64_t m = __ballot(hit);
            if (m != 0ull) {
                cursor += (uint32_t)__ffsll((unsigned long long)m) - 1u;
                *out = ev[cursor]; /* the same address in every lane */
                cursor++;
                return true;
            }
            cursor += 64u;
        }
        return false;
    };
    auto emit = [&](uint32_t type, uint64_t dec, uint32_t aux, uint32_t word_index, uint32_t inverted, uint32_t nr_ok) {
        if (lane == 0u && at < room) { /* at < room: the bound on a run's events (mfm_runbatch.h) */
            RbtSlot o;
            o.dec = dec;
            o.type = type;
            o.aux = aux;
            o.word_index = word_index;
            o.inverted = inverted;
            o.nr_ok = nr_ok;
            o.reserved = 0;
            slots[at] = o;
        }
        at++;
    };
    const uint32_t cnt = mfm_runbatch_walk(&s.a, s.base, s.end, s.kept, s.nr_kept, s.bits, s.nr_dec, P, find, emit);
    if (lane == 0u) {
        A.count[r] = cnt < room ? cnt : room;
        RbtLeft l;
        l.mark = s.a.mark;
        l.mode = s.a.mode;
        l.word_index = s.a.word_index;
        l.inverted = s.a.inverted;
        l.reserved = 0;
        A.left[r] = l;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rbt_scan_kernel(const RbtCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    const uint32_t n = A.ctl[RBT_CTL_RUNS]; /* 0 for a refused call */
    const bool bad = A.ctl[RBT_CTL_BAD] != 0u;
    const uint64_t total = mfm_run_count_scan(A.count, A.ev_base, n, lds); /* at most the slots: below 2^32 */
    if (threadIdx.x == 0) {
        A.ev_base[n] = (uint32_t)total;
    }
    __threadfence_block();
    __syncthreads(); /* every thread has read ctl */
    const bool over = !bad && total > A.cap_events;
    if (threadIdx.x == 0 && n != 0u) {
        if (bad || over) { /* by the check and by the count, before an event is placed or a state moves */
            A.totals[RBT_T_RUNS] = 0;
            A.totals[MFM_RUN_T_OVERFLOW] = over ? MFM_RUNBATCH_OVER_EVENTS : 0u;
            A.totals[MFM_RUN_T_INPUT] = bad ? MFM_RUNBATCH_IN_BAD_EVENTS : 0u;
            for (uint32_t i = 0; i < RBT_NR_CTL; i++) {
                A.ctl[i] = 0;
            }
        } else {
            A.totals[RBT_T_EVENTS] = total;
        }
    }
}

/* the run of slot s: the last r with slot_base[r] <= s (every run has at least five slots) */
__device__ __forceinline__ uint32_t rbt_run_of(const uint32_t *slot_base, uint32_t n_runs, uint32_t s)
{
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (slot_base[mid] <= s) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__global__ __launch_bounds__(RBT_DECODE_THREADS) void rbt_decode_kernel(const RbtCall A)
{
    __shared__ MfmBchTables T;
    const uint32_t z = threadIdx.x & 15u, g = (threadIdx.x & 63u) >> 4;
    const uint32_t s = blockIdx.x * RBT_PER_BLOCK + threadIdx.x / 16u;
    const uint32_t n = A.ctl[RBT_CTL_RUNS], nslots = A.ctl[RBT_CTL_SLOTS]; /* 0 for a refused call */
    if (blockIdx.x * RBT_PER_BLOCK >= nslots) { /* surplus blocks */
        return;
    }
    uint32_t r = 0, idx = 0;
    bool have = false;
    if (s < nslots) {
        r = rbt_run_of(A.slot_base, n, s);
        idx = s - A.slot_base[r];
        have = idx < A.count[r];
    }
    RbtSlot o{};
    if (have) {
        o = A.slots[s];
    }
    const bool batch = have && o.type == MFM_POCSAG_EV_BATCH;
    if (!__syncthreads_or(batch)) { /* no batch in the block: the tables stay where they are */
        if (!have) {
            return;
        }
    } else {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(A.bch);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&T);
        for (uint32_t i = threadIdx.x; i < sizeof(MfmBchTables) / 4; i += RBT_DECODE_THREADS) {
            dst[i] = src[i];
        }
        __syncthreads();
    }
    uint32_t raw = 0, fixed = 0, rc = 0;
    uint64_t stretch_window = 0;
    mfm_runrs_run run{};
    if (have) {
        run = A.runs[r];
        const RbtStream st = rbt_stream(A, run);
        stretch_window = st.stretch_window;
        if (batch) {
            raw = mfm_runbatch_raw(st.kept, st.nr_kept, st.bits, st.nr_dec, st.base, o.dec, z, o.inverted);
            fixed = mfm_bch_fix(&T, raw & 0x7fffffffu, &rc); /* pager_pocsag.c:332-334 */
        }
    }
    const uint32_t fail = (uint32_t)(__ballot(batch && rc != 0u) >> (16u * g)) & 0xffffu;
    if (!have) {
        return;
    }
    mfm_runbatch_event *e = &A.events[A.ev_base[r] + idx]; /* below the total, which is at most cap_events (the scan) */
    if (z == 0u) {
        e->type = o.type;
        e->channel = run.channel;
        e->run = r;
        e->aux = o.aux;
        e->word_index = o.word_index;
        e->inverted = o.inverted;
        e->nr_ok = batch ? (fail ? (uint32_t)__ffs((int)fail) - 1u : 16u) : o.nr_ok;
        e->fail_mask = fail;
        e->stretch_window = stretch_window;
        e->dec = o.dec;
    }
    e->raw[z] = raw;
    e->corrected[z] = fixed;
}

__global__ __launch_bounds__(256) void rbt_state_kernel(const RbtCall A)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= A.C) {
        return;
    }
    const uint32_t last = A.chan_last[c];
    A.chan_last[c] = MFM_RUN_NONE; /* for the next call */
    const bool refused = A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0;
    const mfm_runbatch_state *old = &A.chan_old[c];
    mfm_runbatch_state *st = &A.chan_new[c];
    if (last == MFM_RUN_NONE || refused) { /* a channel without a run, a refused call: the state stays */
        const uint32_t *src = reinterpret_cast<const uint32_t *>(old);
        uint32_t *dst = reinterpret_cast<uint32_t *>(st);
#pragma unroll 1
        for (uint32_t i = 0; i < sizeof(mfm_runbatch_state) / 4; i++) {
            dst[i] = src[i];
        }
        return;
    }
    const mfm_runrs_run run = A.runs[last];
    const RbtStream s = rbt_stream(A, run);
    const RbtLeft l = A.left[last];
    const uint32_t left = l.mode == MFM_RUNBATCH_SEARCH ? 0u : (uint32_t)(s.end - l.mark); /* below 544: the walk went as far as the run */
    st->stretch_window = s.stretch_window;
    st->decs = s.end;
    st->mark = l.mark;
    st->has_stretch = 1;
    st->mode = l.mode;
    st->word_index = l.word_index;
    st->inverted = l.inverted;
    st->nr_kept = left;
    st->reserved = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < MFM_RUNBATCH_KEPT_WORDS; w++) {
        st->kept[w] = mfm_runbatch_keep(s.kept, s.nr_kept, s.bits, s.nr_dec, s.base, l.mark, left, w);
    }
    st->reserved2 = 0;
}

/* what create checks without a device; the table and the event capacity with the default filled in */
int rbt_geometry(const mfm_runbatch_config &cfg, mfm_runbatch_params *P, uint64_t *cap_events)
{
    struct { /* what the burst stages share of their configurations; the capacities are held against the limits below */
        uint32_t abi_version, nr_channels, max_runs, max_out_samples, flags;
    } common = { cfg.abi_version, cfg.nr_channels, 1u, 1u, cfg.flags };
    const int rc = mfm_run_geometry(common);
    if (rc != MFM_OK) {
        return rc;
    }
    if (const char *why = mfm_runbatch_params_check(cfg, P)) {
        return mfm_run_fail(MFM_E_INVAL, why);
    }
    if (0 == cfg.max_runs || 0 == cfg.max_decisions || cfg.max_runs >= MFM_RUN_MAX_RUNS || cfg.max_decisions >= MFM_RUN_MAX_OUT ||
        cfg.max_events >= MFM_RUN_MAX_OUT) {
        return mfm_run_fail(MFM_E_INVAL, "max_runs must be 1 .. 2^28 - 1, max_decisions 1 .. 2^31 - 1 and max_events below 2^31: the burst sync stage's capacities");
    }
    /* 3 * 2^31 / 544 + 5 * 2^28 stays below 2^31 */
    *cap_events = cfg.max_events ? cfg.max_events : 3u * (uint64_t)(cfg.max_decisions / MFM_RUNBATCH_FRAME) + 5u * (uint64_t)cfg.max_runs;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *rbt_refusal(uint64_t over, uint64_t err)
{
    if (err & MFM_RUNBATCH_IN_RUNSYNC) {
        return "the burst sync stage's call raised overflow or an input error";
    }
    if (err & MFM_RUNBATCH_IN_BAD_RUNS) {
        return "the run list is not a burst sync stage's: a run names a channel that does not exist, channels do not ascend, a word_offset is not the running sum of the runs' words, or the runs hold more than max_decisions and max_runs allow";
    }
    if (err & MFM_RUNBATCH_IN_OUT_OF_STEP) {
        return "out of step with the burst sync stage: a continuing run does not follow on its channel's stretch";
    }
    if (err & MFM_RUNBATCH_IN_BAD_EVENTS) {
        return "the sync events are not a burst sync stage's: a dec outside its run, events that do not ascend, a word_index or inverted that cannot be, or more events than the totals hold";
    }
    if (over & MFM_RUNBATCH_OVER_RUNS) {
        return "the call has more runs than max_runs";
    }
    return "the call's events exceed max_events";
}

} /* namespace */

struct mfm_runbatch {
    mfm_runbatch_config cfg{};
    mfm_runbatch_params P{};
    uint64_t cap_events = 0, cap_slots = 0;
    mfm_runbatch_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    uint32_t *d_in_base = nullptr, *d_slot_base = nullptr, *d_count = nullptr, *d_ev_base = nullptr, *d_chan_last = nullptr, *d_ctl = nullptr;
    RbtLeft *d_left = nullptr;
    RbtSlot *d_slots = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runbatch_event *d_events = nullptr;
    MfmBchTables *d_bch = nullptr; /* owned by mfm_pocsag.hip, one per device */
    hipStream_t last_stream = nullptr;
    bool have_call = false;
};

extern "C" {

int mfm_runbatch_create(struct mfm_runbatch **pb, const struct mfm_runbatch_config *cfg)
{
    if (!pb || !cfg) {
        return MFM_E_INVAL;
    }
    *pb = nullptr;
    mfm_runbatch_params P{};
    uint64_t cap_events = 0;
    const int rc = rbt_geometry(*cfg, &P, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    MfmBchTables *d_bch = nullptr;
    const int rb = mfm_internal_bch_device_tables(cfg->device, &d_bch);
    if (rb != MFM_OK) {
        return rb;
    }
    mfm_runbatch *o = new (std::nothrow) mfm_runbatch();
    if (!o) {
        return MFM_E_NOMEM;
    }
    o->cfg = *cfg;
    o->P = P;
    o->d_bch = d_bch;
    o->cap_events = cap_events;
    o->cap_slots = 3u * (uint64_t)(cfg->max_decisions / MFM_RUNBATCH_FRAME) + 5u * (uint64_t)cfg->max_runs; /* the sum of mfm_runbatch_slots */
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    *pb = o; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&o->d_chan[i], C * sizeof(mfm_runbatch_state)));
        MFM_RUN_TRY(hipMemset(o->d_chan[i], 0, C * sizeof(mfm_runbatch_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&o->d_in_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_slot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_count, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_ev_base, (nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_left, nruns * sizeof(RbtLeft)));
    MFM_RUN_TRY(hipMalloc(&o->d_slots, (size_t)o->cap_slots * sizeof(RbtSlot)));
    MFM_RUN_TRY(hipMalloc(&o->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(o->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_ctl, 4 * 4));
    MFM_RUN_TRY(hipMemset(o->d_ctl, 0, 4 * 4));
    MFM_RUN_TRY(hipMalloc(&o->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(o->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&o->d_events, (size_t)cap_events * sizeof(mfm_runbatch_event)));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runbatch_destroy(struct mfm_runbatch **pb)
{
    if (!pb || !*pb) {
        return;
    }
    mfm_runbatch *o = *pb;
    (void)hipSetDevice(o->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(o->d_chan[0]);
    (void)hipFree(o->d_chan[1]);
    (void)hipFree(o->d_in_base);
    (void)hipFree(o->d_slot_base);
    (void)hipFree(o->d_count);
    (void)hipFree(o->d_ev_base);
    (void)hipFree(o->d_left);
    (void)hipFree(o->d_slots);
    (void)hipFree(o->d_chan_last);
    (void)hipFree(o->d_ctl);
    (void)hipFree(o->d_totals);
    (void)hipFree(o->d_events);
    delete o;
    *pb = nullptr;
}

int mfm_runbatch_process_device(struct mfm_runbatch *o, const struct mfm_runsync_run *d_runs, const uint32_t *d_bits,
                                const struct mfm_runsync_event *d_events, const uint64_t *d_totals, void *stream)
{
    if (!o || !d_runs || !d_bits || !d_events || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(o, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = o->cur;
    const RbtCall A{ reinterpret_cast<const mfm_runbatch_in_run *>(d_runs), d_bits, d_events, d_totals, o->d_chan[cur], o->d_chan[cur ^ 1u],
                     o->d_in_base, o->d_slot_base, o->d_count, o->d_ev_base, o->d_left, o->d_slots, o->d_chan_last, o->d_ctl, o->d_totals,
                     o->d_events, o->d_bch, o->cfg.nr_channels, o->cfg.max_runs, o->cfg.max_decisions, (uint32_t)o->cap_events, o->P };
    hipLaunchKernelGGL(rbt_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rbt_walk_kernel, dim3(o->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rbt_scan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rbt_decode_kernel, dim3((uint32_t)((o->cap_slots + RBT_PER_BLOCK - 1u) / RBT_PER_BLOCK)), dim3(RBT_DECODE_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rbt_state_kernel, dim3((o->cfg.nr_channels + 255u) / 256u), dim3(256), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(o, s);
    return MFM_OK;
}

int mfm_runbatch_fetch(struct mfm_runbatch *o, struct mfm_runbatch_event *events, size_t max_events, size_t *nr_events)
{
    if (!o || !nr_events || (!events && max_events)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (!o->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(o->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(o->last_stream));
    uint64_t t[4];
    MFM_RUN_TRY(hipMemcpy(t, o->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, rbt_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    *nr_events = (size_t)t[RBT_T_EVENTS];
    if (*nr_events > max_events) {
        return MFM_E_NOMEM;
    }
    if (*nr_events) {
        MFM_RUN_TRY(hipMemcpy(events, o->d_events, *nr_events * sizeof(mfm_runbatch_event), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runbatch_device_view(struct mfm_runbatch *o, const struct mfm_runbatch_event **d_events, const uint64_t **d_totals)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (d_events) {
        *d_events = o->d_events;
    }
    if (d_totals) {
        *d_totals = o->d_totals;
    }
    return MFM_OK;
}

int mfm_runbatch_get_capacity(struct mfm_runbatch *o, uint32_t *max_runs, uint64_t *max_events)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (max_runs) {
        *max_runs = o->cfg.max_runs;
    }
    if (max_events) {
        *max_events = o->cap_events;
    }
    return MFM_OK;
}

int mfm_runbatch_fetch_state(struct mfm_runbatch *o, struct mfm_runbatch_state *state, size_t nr_channels)
{
    return mfm_run_fetch_state(o, state, nr_channels);
}

int mfm_hosttwin_runbatch_state_check(uint32_t nr_channels, const struct mfm_runbatch_state *state)
{
    return mfm_run_state_check(nr_channels, state, "batch", mfm_runbatch_state_check);
}

int mfm_runbatch_store_state(struct mfm_runbatch *o, const struct mfm_runbatch_state *state, size_t nr_channels)
{
    return mfm_run_store_state(o, state, nr_channels, mfm_hosttwin_runbatch_state_check);
}

/* ---- the host twin: the same plan, the same automaton one run after the other ---- */

int mfm_hosttwin_runbatch_call(const struct mfm_runbatch_config *cfg, struct mfm_runbatch_state *state, const struct mfm_runsync_run *sruns,
                               const uint32_t *bits, const struct mfm_runsync_event *sev, const uint64_t *totals,
                               struct mfm_runbatch_event *events, size_t max_out_events, size_t *nr_events, uint32_t *flags)
{
    if (!cfg || !state || !totals || !nr_events || (!events && max_out_events)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (flags) {
        *flags = 0;
    }
    mfm_runbatch_params P{};
    uint64_t cap_events = 0;
    const int rc = rbt_geometry(*cfg, &P, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    const mfm_runbatch_in_run *runs = reinterpret_cast<const mfm_runbatch_in_run *>(sruns);
    const mfm_runbatch_state_outs *souts = reinterpret_cast<const mfm_runbatch_state_outs *>(state);
    uint64_t n, E, over, err; /* the plan pass */
    mfm_run_totals_check(totals, ~0ull, cfg->max_runs, &n, &E, &over, &err);
    if (!over && !err) {
        const uint64_t cap_words = (uint64_t)cfg->max_decisions / 32u + cfg->max_runs;
        const uint64_t cap_slots = 3u * (uint64_t)(cfg->max_decisions / MFM_RUNBATCH_FRAME) + 5u * (uint64_t)cfg->max_runs;
        uint64_t tw = 0, te = 0, ts = 0;
        if (n && !runs) {
            return MFM_E_INVAL;
        }
        for (uint64_t r = 0; r < n; r++) {
            err |= mfm_run_check_run(runs[r], r ? &runs[r - 1] : nullptr, cfg->nr_channels, cap_words, souts, true);
            err |= runs[r].out_offset != tw ? MFM_RUNBATCH_IN_BAD_RUNS : 0u;
            tw += ((uint64_t)runs[r].nr_out + 31u) / 32u;
            ts += mfm_runbatch_slots(runs[r].nr_out);
            te += runs[r].reserved;
        }
        if (tw > cap_words || ts > cap_slots) {
            err |= MFM_RUNBATCH_IN_BAD_RUNS;
        }
        if (te > E || E >= MFM_RUN_MAX_OUT) {
            err |= MFM_RUNBATCH_IN_BAD_EVENTS;
        }
        if (!err && ((tw && !bits) || (te && !sev))) {
            return MFM_E_INVAL;
        }
    }
    if (!over && !err) { /* the sync events, before the automaton follows one */
        uint64_t at = 0;
        for (uint64_t r = 0; r < n; r++) {
            for (uint32_t i = 0; i < runs[r].reserved; i++) {
                if (!mfm_runbatch_event_ok(sev[at + i], i ? &sev[at + i - 1] : nullptr, runs[r].first_out, runs[r].nr_out, P.nr_words)) {
                    err |= MFM_RUNBATCH_IN_BAD_EVENTS;
                }
            }
            at += runs[r].reserved;
        }
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, rbt_refusal(over, err));
    }
    /* every run from the state the call started with (only a channel's first run reads it); the state its last run leaves */
    const MfmBchTables *T = mfm_internal_bch_host_tables();
    std::vector<mfm_runbatch_state> left(n);
    std::vector<mfm_runbatch_event> evs;
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        const mfm_runbatch_state &old = state[run.channel];
        const mfm_runsync_event *ev = sev + at;
        const uint32_t ne = run.reserved, nd = run.nr_out;
        at += ne;
        mfm_runbatch_auto a;
        uint32_t nr_kept;
        mfm_runbatch_start(&old, run.flags, &a, &nr_kept);
        const uint32_t *kept = old.kept, *rb = nd ? bits + run.out_offset : nullptr;
        const uint64_t base = run.first_out - nr_kept, end = run.first_out + nd;
        const uint64_t stretch_window = (run.flags & MFM_RUNRS_BEGINS) ? run.first_window : old.stretch_window;
        uint32_t cursor = 0;
        auto find = [&](uint64_t mark, mfm_runsync_event *out) -> bool {
            for (; cursor < ne; cursor++) {
                if (ev[cursor].dec >= mark && mfm_runbatch_enabled(P, ev[cursor].word_index)) {
                    *out = ev[cursor++];
                    return true;
                }
            }
            return false;
        };
        auto emit = [&](uint32_t type, uint64_t dec, uint32_t aux, uint32_t word_index, uint32_t inverted, uint32_t nr_ok) {
            mfm_runbatch_event e;
            memset(&e, 0, sizeof(e));
            e.type = type;
            e.channel = run.channel;
            e.run = (uint32_t)r;
            e.aux = aux;
            e.word_index = word_index;
            e.inverted = inverted;
            e.nr_ok = nr_ok;
            e.stretch_window = stretch_window;
            e.dec = dec;
            if (type == MFM_POCSAG_EV_BATCH) {
                e.nr_ok = 16;
                for (uint32_t z = 0; z < 16u; z++) {
                    uint32_t bad = 0;
                    e.raw[z] = mfm_runbatch_raw(kept, nr_kept, rb, nd, base, dec, z, inverted);
                    e.corrected[z] = mfm_bch_fix(T, e.raw[z] & 0x7fffffffu, &bad); /* pager_pocsag.c:332-334 */
                    if (bad) {
                        e.fail_mask |= 1u << z;
                        e.nr_ok = e.nr_ok == 16u ? z : e.nr_ok;
                    }
                }
            }
            evs.push_back(e);
        };
        mfm_runbatch_walk(&a, base, end, kept, nr_kept, rb, nd, P, find, emit);
        mfm_runbatch_state &st = left[r];
        memset(&st, 0, sizeof(st));
        const uint32_t keep = a.mode == MFM_RUNBATCH_SEARCH ? 0u : (uint32_t)(end - a.mark);
        st.stretch_window = stretch_window;
        st.decs = end;
        st.mark = a.mark;
        st.has_stretch = 1;
        st.mode = a.mode;
        st.word_index = a.word_index;
        st.inverted = a.inverted;
        st.nr_kept = keep;
        for (uint32_t w = 0; w < MFM_RUNBATCH_KEPT_WORDS; w++) {
            st.kept[w] = mfm_runbatch_keep(kept, nr_kept, rb, nd, base, a.mark, keep, w);
        }
    }
    if (evs.size() > cap_events) {
        return mfm_run_twin_refuse(MFM_RUNBATCH_OVER_EVENTS, 0, flags, rbt_refusal(MFM_RUNBATCH_OVER_EVENTS, 0));
    }
    *nr_events = evs.size();
    if (evs.size() > max_out_events) {
        return MFM_E_NOMEM; /* nothing written, the state included */
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            state[runs[r].channel] = left[r];
        }
    }
    if (!evs.empty()) {
        memcpy(events, evs.data(), evs.size() * sizeof(mfm_runbatch_event));
    }
    return MFM_OK;
}

} /* extern "C" */
