/*
 * mfm_run_ends.h - the stretch-end records of the three burst stages (mfm_runais_*, mfm_runpocsag_*, mfm_runflex_*,
 * include/multifm_hip.h): what the kernels of mfm_run_ends.hip and the host twins must state once.
 *
 * A record is a pure function of one per-channel state, the channel and the run that ended the stretch: the three
 * mfm_run*_end_of below.  Which states are the end of a stretch is one rule for all three stages (mfm_run_ends_of_run): run r
 * of a call that is not refused yields
 *   (a) a record of the state the call started from, when r is its channel's first run of the call, begins a stretch and
 *       that state has a stretch: run = r;
 *   (b) a record of the state r's walk ended in, when run r + 1 is of the same channel (it necessarily begins): run = r + 1;
 * (a) in front of (b), runs in list order.  The end call records every channel with a stretch, run = MFM_RUN_ENDS_NO_RUN.
 *
 * The stage files hold no kernel of this: they hand their buffers to the launchers below, which live in mfm_run_ends.hip.
 */
#ifndef MFM_RUN_ENDS_H
#define MFM_RUN_ENDS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/multifm_hip.h"
#include "mfm_bch.h"
#include "mfm_runais.h"
#include "mfm_runflex.h"
#include "mfm_runpocsag.h"

#define MFM_RUN_ENDS_NO_RUN 0xffffffffu /* mfm_run*_end.run of a record the end call wrote */
#define MFM_RUN_ENDS_A 1u               /* mfm_run_ends_of_run: the carried stretch ends in front of run r */
#define MFM_RUN_ENDS_B 2u               /* the stretch run r belongs to ends behind it */

enum { MFM_RUN_ENDS_AIS = 0, MFM_RUN_ENDS_POCSAG = 1, MFM_RUN_ENDS_FLEX = 2 };

/* which records run r of a list of n yields; has_stretch: of the state the call started from, r's channel.  The first-run test
 * is the one of the stages' check_run */
__host__ __device__ inline uint32_t mfm_run_ends_of_run(const mfm_runrs_run *runs, uint64_t r, uint64_t n, uint32_t has_stretch)
{
    const bool first = r == 0 || runs[r - 1].channel != runs[r].channel;
    uint32_t k = 0;
    if (first && (runs[r].flags & MFM_RUNRS_BEGINS) && has_stretch) {
        k |= MFM_RUN_ENDS_A;
    }
    if (r + 1 < n && runs[r + 1].channel == runs[r].channel) {
        k |= MFM_RUN_ENDS_B;
    }
    return k;
}

__host__ __device__ inline void mfm_runais_end_of(const mfm_runais_state &s, uint32_t channel, uint32_t run, mfm_runais_end &e)
{
    e.stretch_window = s.stretch_window;
    e.outs = s.outs;
    e.start_sample = s.mode == MFM_RUNAIS_RECEIVE ? s.start : 0u;
    e.channel = channel;
    e.run = run;
    e.mode = s.mode;
    e.nr_bits = s.mode == MFM_RUNAIS_RECEIVE ? s.cur_bit : 0u;
    e.reserved[0] = e.reserved[1] = 0;
}

__host__ __device__ inline void mfm_runflex_end_of(const mfm_runflex_state &s, uint32_t channel, uint32_t run, mfm_runflex_end &e)
{
    e.stretch_window = s.stretch_window;
    e.outs = s.outs;
    e.j = s.j;
    e.channel = channel;
    e.run = run;
    e.mode = s.mode;
    e.eye = s.eye;
    e.coding = s.coding;
    e.fiw = s.fiw;
    e.cycle = s.cycle;
    e.frame = s.frame;
    e.reserved[0] = e.reserved[1] = 0;
}

/* POCSAG, word z (0 .. 15) of the batch the squelch cut: corrected[z], and *fail = 1 when the stage's BCH decoder gives the
 * word up.  Words from batch_word on are not whole: 0, no failure */
template <class T>
__host__ __device__ inline uint32_t mfm_runpocsag_end_word(const T *bch, const mfm_runpocsag_state &s, uint32_t z, uint32_t *fail)
{
    *fail = 0;
    if (s.mode != MFM_RUNPOCSAG_BATCH || z >= s.batch_word) {
        return 0;
    }
    return mfm_bch_fix(bch, s.batch[z] & 0x7fffffffu, fail);
}

/* POCSAG, all of a record but raw[] and corrected[]; fail_mask: bit z = what mfm_runpocsag_end_word said of word z */
__host__ __device__ inline void mfm_runpocsag_end_head(const mfm_runpocsag_state &s, uint32_t channel, uint32_t run, uint32_t fail_mask,
                                                       mfm_runpocsag_end &e)
{
    const bool batch = s.mode == MFM_RUNPOCSAG_BATCH;
    e.stretch_window = s.stretch_window;
    e.outs = s.outs;
    e.channel = channel;
    e.run = run;
    e.mode = s.mode;
    e.baud = s.baud;
    e.nr_words = batch ? s.batch_word : 0u;
    e.nr_bits = batch ? s.batch_bit : 0u;
    e.nr_sync_bits = s.mode == MFM_RUNPOCSAG_SYNCWORD ? s.nr_sync_bits : 0u;
    e.reserved = 0;
    uint32_t first = 0; /* the BATCH event's rule: words accepted in front of the first failure */
    while (first < e.nr_words && !((fail_mask >> first) & 1u)) {
        first++;
    }
    e.nr_ok = first;
    e.fail_mask = fail_mask;
}

template <class T>
inline void mfm_runpocsag_end_of(const T *bch, const mfm_runpocsag_state &s, uint32_t channel, uint32_t run, mfm_runpocsag_end &e)
{
    uint32_t mask = 0;
    for (uint32_t z = 0; z < 16u; z++) {
        uint32_t fail;
        e.raw[z] = s.batch[z];
        e.corrected[z] = mfm_runpocsag_end_word(bch, s, z, &fail);
        mask |= fail << z;
    }
    mfm_runpocsag_end_head(s, channel, run, mask, e);
}

/*
 * Host twin of the records of one process call that is not refused: state is what the call started from, left[r] what run r's
 * walk ended in; of(state, channel, run, end) is the stage's record.  Returns the number of records; writes at most max of them.
 */
template <class State, class End, class Of>
inline size_t mfm_run_ends_host_call(const mfm_runrs_run *runs, uint64_t n, const State *state, const State *left, End *ends, size_t max, Of of)
{
    size_t k = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint32_t c = runs[r].channel;
        const uint32_t what = mfm_run_ends_of_run(runs, r, n, state[c].has_stretch);
        if (what & MFM_RUN_ENDS_A) {
            if (k < max) {
                of(state[c], c, (uint32_t)r, ends[k]);
            }
            k++;
        }
        if (what & MFM_RUN_ENDS_B) {
            if (k < max) {
                of(left[r], c, (uint32_t)r + 1u, ends[k]);
            }
            k++;
        }
    }
    return k;
}

/* Host twin of the end call: MFM_E_NOMEM (nothing written, *nr = needed) or MFM_OK with the records written and every state zero */
template <class State, class End, class Of>
inline int mfm_run_ends_host_flush(uint32_t nr_channels, State *state, End *ends, size_t max, size_t *nr, Of of)
{
    if (!state || !nr || !nr_channels || (!ends && max)) {
        return MFM_E_INVAL;
    }
    size_t k = 0;
    for (uint32_t c = 0; c < nr_channels; c++) {
        k += state[c].has_stretch ? 1u : 0u;
    }
    *nr = k;
    if (k > max) {
        return MFM_E_NOMEM;
    }
    k = 0;
    for (uint32_t c = 0; c < nr_channels; c++) {
        if (state[c].has_stretch) {
            of(state[c], c, MFM_RUN_ENDS_NO_RUN, ends[k++]);
        }
    }
    memset(state, 0, (size_t)nr_channels * sizeof(State));
    return MFM_OK;
}

/* ---- the device side, in mfm_run_ends.hip ----------------------------------------------------------------------------- */

/* what a stage object keeps for the report; all NULL while it is off */
struct MfmRunEnds {
    bool on = false;
    void *d_ends = nullptr;           /* [cap] records of the stage's type */
    uint64_t *d_end_totals = nullptr; /* { records, records with mode != 0 } */
    uint32_t *d_base = nullptr;       /* [cap] first record of a run (process call) or of a channel (end call) */
    size_t cap = 0;                   /* max(max_runs, nr_channels) */
};

/* the buffers of one process call: the stage's own, as its walk kernel left them */
struct MfmRunEndsCall {
    const mfm_runrs_run *runs;
    const void *chan_old;  /* [C] the state the call started from */
    const void *run_state; /* [cap_runs] what a run's walk ended in */
    const uint32_t *ctl;   /* ctl[1]: the call's runs, 0 when it is refused */
    const MfmBchTables *bch; /* POCSAG */
    uint32_t C, cap_runs;
};

#define MFM_RUN_ENDS_HIDDEN extern "C" __attribute__((visibility("hidden")))
/* switch the report on (allocate) or off (free) on the current device; MFM_OK or an MFM_E_* code with the message set */
MFM_RUN_ENDS_HIDDEN int mfm_internal_run_ends_set(MfmRunEnds *e, int stage, bool on, size_t max_runs, size_t nr_channels);
/* the count-and-place and the write launch of a process call, queued on s */
MFM_RUN_ENDS_HIDDEN int mfm_internal_run_ends_process(MfmRunEnds *e, int stage, const MfmRunEndsCall *call, hipStream_t s);
/* the end call: records of the channels with a stretch out of chan [C], which is zeroed, as are the stage's totals[4] */
MFM_RUN_ENDS_HIDDEN int mfm_internal_run_ends_flush(MfmRunEnds *e, int stage, void *chan, uint64_t *totals, const MfmBchTables *bch,
                                                    uint32_t C, hipStream_t s);
/* copy the records out once the queued work has run: MFM_E_NOMEM with *nr = needed when max is too small */
MFM_RUN_ENDS_HIDDEN int mfm_internal_run_ends_fetch(MfmRunEnds *e, int stage, void *out, size_t max, size_t *nr);

/*
 * The four entries of a stage, stated once: Obj is the stage's object (cfg, have_call, last_stream, d_chan[2], cur, d_totals,
 * ends), fail(code, msg) its way to leave a message, refusal(over, err) the message of a refused call.
 */
template <class Obj, class Fail>
inline int mfm_run_ends_entry_set(Obj *o, int stage, int on, Fail fail)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (o->have_call) {
        return fail(MFM_E_STATE, "the stretch-end report is switched before the first process call only");
    }
    if (hipSetDevice(o->cfg.device) != hipSuccess) {
        return fail(MFM_E_DEVICE, "hipSetDevice failed");
    }
    return mfm_internal_run_ends_set(&o->ends, stage, on != 0, o->cfg.max_runs, o->cfg.nr_channels);
}

template <class Obj, class Fail>
inline int mfm_run_ends_entry_flush(Obj *o, int stage, const MfmBchTables *bch, void *stream, Fail fail)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (!o->ends.on) {
        return fail(MFM_E_STATE, "the stretch-end report is off (set_end_report before the first process call)");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipSetDevice(o->cfg.device) != hipSuccess) {
        return fail(MFM_E_DEVICE, "hipSetDevice failed");
    }
    if (o->have_call && o->last_stream != s && hipStreamSynchronize(o->last_stream) != hipSuccess) {
        return fail(MFM_E_DEVICE, "hipStreamSynchronize failed"); /* state lives on the device; keep calls ordered */
    }
    /* the buffer the next process call reads */
    const int rc = mfm_internal_run_ends_flush(&o->ends, stage, o->d_chan[o->cur], o->d_totals, bch, o->cfg.nr_channels, s);
    if (rc != MFM_OK) {
        return rc;
    }
    o->last_stream = s;
    o->have_call = true;
    return MFM_OK;
}

template <class Obj, class Fail, class Refusal>
inline int mfm_run_ends_entry_fetch(Obj *o, int stage, void *ends, size_t max_ends, size_t *nr_ends, Fail fail, Refusal refusal)
{
    if (!o || !nr_ends || (!ends && max_ends)) {
        return MFM_E_INVAL;
    }
    *nr_ends = 0;
    if (!o->ends.on) {
        return fail(MFM_E_STATE, "the stretch-end report is off (set_end_report before the first process call)");
    }
    if (!o->have_call) {
        return fail(MFM_E_STATE, "no call yet: there are no stretch-end records to fetch");
    }
    uint64_t t[4];
    if (hipSetDevice(o->cfg.device) != hipSuccess || hipStreamSynchronize(o->last_stream) != hipSuccess ||
        hipMemcpy(t, o->d_totals, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) {
        return fail(MFM_E_DEVICE, "waiting for the last call failed");
    }
    if (t[2] || t[3]) { /* overflow, input error */
        return fail(MFM_E_STATE, refusal(t[2], t[3]));
    }
    return mfm_internal_run_ends_fetch(&o->ends, stage, ends, max_ends, nr_ends);
}

template <class Obj, class End, class Fail>
inline int mfm_run_ends_entry_view(Obj *o, const End **d_ends, const uint64_t **d_end_totals, Fail fail)
{
    if (!o) {
        return MFM_E_INVAL;
    }
    if (!o->ends.on) {
        return fail(MFM_E_STATE, "the stretch-end report is off (set_end_report before the first process call)");
    }
    if (d_ends) {
        *d_ends = static_cast<const End *>(o->ends.d_ends);
    }
    if (d_end_totals) {
        *d_end_totals = o->ends.d_end_totals;
    }
    return MFM_OK;
}

#endif /* MFM_RUN_ENDS_H */
