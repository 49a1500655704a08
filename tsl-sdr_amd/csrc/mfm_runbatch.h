/*
 * mfm_runbatch.h - what the kernels of the burst batch stage (mfm_runbatch_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runbatch_call) must state once: the automaton that follows a POCSAG transmission behind a sync event
 * (pager/pager_pocsag.c:468-538 at one sample per bit), where the bits of a frame come from, what a run starts from and leaves
 * behind, and what a stored state must satisfy.  The checks a run has to pass before a bit is read are mfm_run_stage.h's: struct
 * mfm_runsync_run has the field layout of struct mfm_runrs_run (word_offset for out_offset, first_dec for first_out, nr_dec for
 * nr_out, nr_events where it has reserved) and the state below that of a state with `outs` where it has `decs`, so
 * mfm_run_check_run reads both as they stand.
 *
 * The bits.  Decision j of a run is bit j % 32 of the run's word j / 32 (the sync stage's packing).  A frame that began in an
 * earlier call has its first bits in the state: `kept` holds the decisions [mark, decs) of the stretch, LSB first.  Behind one
 * another the two are one stream of nr_kept + nr_dec bits whose bit 0 is decision `decs - nr_kept` of the stretch, and every word
 * of a batch and every sync slot is one 32-bit window of that stream (mfm_runbatch_window): a funnel of two neighbouring words of
 * `kept`, of the run's bits, or one of each where the window lies across the seam.
 *
 * The bound on a run's events.  Two BATCH events are at least 544 decisions apart (the 512 of the batch behind the 32 of a sync
 * slot), so a run of nr_dec decisions holds at most nr_dec / 544 + 1 of them.  Between two of them lie at most two others (KEPT,
 * or LOST and the next FOUND), in front of the first at most two (a slot's verdict and a FOUND) and behind the last at most two:
 * 3 B + 2 events for B batches, at most 3 (nr_dec / 544) + 5; a run without a batch has at most two.  Summed over a call that is
 * at most 3 (max_decisions / 544) + 5 max_runs, the default of max_events and the size of the walk's slot ranges.
 */
#ifndef MFM_RUNBATCH_H
#define MFM_RUNBATCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"
#include "mfm_runsync.h"

#define MFM_RUNBATCH_BATCH 512u /* decisions of a batch: 16 codewords */
#define MFM_RUNBATCH_FRAME 544u /* ... and of a batch with the sync slot behind it */
#define MFM_RUNBATCH_KEPT_WORDS 17u

static_assert(MFM_RUNBATCH_IN_RUNSYNC == MFM_RUN_IN_RUNRS && MFM_RUNBATCH_IN_OUT_OF_STEP == MFM_RUN_IN_OUT_OF_STEP &&
                  MFM_RUNBATCH_IN_BAD_RUNS == MFM_RUN_IN_BAD_RUNS && MFM_RUNBATCH_OVER_RUNS == MFM_RUN_OVER_RUNS,
              "the burst stages share the values of their flags");
static_assert(sizeof(mfm_runsync_run) == sizeof(mfm_runrs_run) && offsetof(mfm_runsync_run, first_window) == offsetof(mfm_runrs_run, first_window) &&
                  offsetof(mfm_runsync_run, word_offset) == offsetof(mfm_runrs_run, out_offset) &&
                  offsetof(mfm_runsync_run, first_dec) == offsetof(mfm_runrs_run, first_out) &&
                  offsetof(mfm_runsync_run, channel) == offsetof(mfm_runrs_run, channel) &&
                  offsetof(mfm_runsync_run, nr_dec) == offsetof(mfm_runrs_run, nr_out) && offsetof(mfm_runsync_run, flags) == offsetof(mfm_runrs_run, flags) &&
                  offsetof(mfm_runsync_run, nr_events) == offsetof(mfm_runrs_run, reserved),
              "struct mfm_runsync_run has the field layout of struct mfm_runrs_run");

/* struct mfm_runbatch_state as mfm_run_check_run reads a state: the decisions are the stretch's outputs so far */
struct __attribute__((may_alias)) mfm_runbatch_state_outs {
    uint64_t stretch_window, outs, mark;
    uint32_t has_stretch, mode, word_index, inverted, nr_kept, reserved;
    uint32_t kept[MFM_RUNBATCH_KEPT_WORDS];
    uint32_t reserved2;
};
static_assert(sizeof(mfm_runbatch_state) == 120 && sizeof(mfm_runbatch_state_outs) == 120 &&
                  offsetof(mfm_runbatch_state, decs) == offsetof(mfm_runbatch_state_outs, outs) &&
                  offsetof(mfm_runbatch_state, has_stretch) == offsetof(mfm_runbatch_state_outs, has_stretch) &&
                  offsetof(mfm_runbatch_state, kept) == 48,
              "struct mfm_runbatch_state is 120 bytes");
static_assert(sizeof(mfm_runbatch_event) == 176 && offsetof(mfm_runbatch_event, stretch_window) == 32 && offsetof(mfm_runbatch_event, raw) == 48,
              "struct mfm_runbatch_event is 176 bytes");
typedef mfm_runrs_run __attribute__((may_alias)) mfm_runbatch_in_run; /* a struct mfm_runsync_run, read through the shared checks */

/* the table and the two settings of the automaton, as create takes them */
struct mfm_runbatch_params {
    uint32_t words[8];
    uint32_t nr_words, word_mask, keep_distance;
};

/* the automaton between two events: what of struct mfm_runbatch_state the walk moves */
struct mfm_runbatch_auto {
    uint64_t mark;
    uint32_t mode, word_index, inverted;
};

/* create's conditions on the table; NULL when they hold, else what is wrong */
inline const char *mfm_runbatch_params_check(const mfm_runbatch_config &cfg, mfm_runbatch_params *out)
{
    if (cfg.nr_words < 1u || cfg.nr_words > 8u) {
        return "nr_words must be 1 .. 8";
    }
    if (cfg.keep_distance > 15u) {
        return "keep_distance must be at most 15";
    }
    if (cfg.word_mask >> cfg.nr_words) {
        return "word_mask must hold no bit at or above nr_words";
    }
    if (out) {
        for (uint32_t k = 0; k < 8u; k++) {
            out->words[k] = k < cfg.nr_words ? cfg.words[k] : 0u;
        }
        out->nr_words = cfg.nr_words;
        out->word_mask = cfg.word_mask;
        out->keep_distance = cfg.keep_distance;
    }
    return nullptr;
}

/* the slots the walk keeps for a run of nr_dec decisions: the bound on its events (above) */
__host__ __device__ inline uint64_t mfm_runbatch_slots(uint32_t nr_dec)
{
    return 3u * (uint64_t)(nr_dec / MFM_RUNBATCH_FRAME) + 5u;
}

/* may a sync event of word k start a transmission */
__host__ __device__ inline bool mfm_runbatch_enabled(const mfm_runbatch_params &P, uint32_t k)
{
    return P.word_mask == 0u || ((P.word_mask >> k) & 1u) != 0u;
}

/* word k of the table without addressing a place of it */
__host__ __device__ inline uint32_t mfm_runbatch_word_of(const mfm_runbatch_params &P, uint32_t k)
{
    uint32_t w = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        w = i == k ? P.words[i] : w;
    }
    return w;
}

/*
 * 32 bits of the stream "kept, then the run's bits" from bit s on, LSB first, 0 where the stream has no bit: kept holds nr_kept
 * bits and is 0 above them, bits holds the run's nr_dec and is 0 above them in the run's last word.  Nothing is read behind
 * either.
 */
__host__ __device__ inline uint32_t mfm_runbatch_window(const uint32_t *kept, uint32_t nr_kept, const uint32_t *bits, uint32_t nr_dec, uint64_t s)
{
    uint32_t v = 0;
    if (s < nr_kept) { /* nr_kept < 544: 17 words */
        const uint32_t w = (uint32_t)s >> 5;
        const uint32_t hi = w + 1u < MFM_RUNBATCH_KEPT_WORDS ? kept[w + 1u] : 0u;
        v = mfm_runsync_window(kept[w], hi, (uint32_t)s & 31u);
    }
    if (nr_dec != 0u && s + 32u > nr_kept) {
        if (s >= nr_kept) {
            const uint64_t t = s - nr_kept;
            if (t < nr_dec) {
                const uint32_t w = (uint32_t)(t >> 5), nw = (nr_dec + 31u) / 32u;
                const uint32_t hi = w + 1u < nw ? bits[w + 1u] : 0u;
                v |= mfm_runsync_window(bits[w], hi, (uint32_t)t & 31u);
            }
        } else { /* across the seam: the run's first bit is bit nr_kept - s of the window, 1 .. 31 */
            v |= bits[0] << (nr_kept - (uint32_t)s);
        }
    }
    return v;
}

/* what a run starts from: its channel's state where it continues a stretch, a fresh automaton where it begins one */
__host__ __device__ inline void mfm_runbatch_start(const mfm_runbatch_state *old, uint32_t flags, mfm_runbatch_auto *a, uint32_t *nr_kept)
{
    if (flags & MFM_RUNRS_BEGINS) {
        a->mark = 0;
        a->mode = MFM_RUNBATCH_SEARCH;
        a->word_index = 0;
        a->inverted = 0;
        *nr_kept = 0;
    } else {
        a->mark = old->mark;
        a->mode = old->mode;
        a->word_index = old->word_index;
        a->inverted = old->inverted;
        *nr_kept = old->nr_kept;
    }
}

/*
 * The automaton over one run.  The stream (kept, nr_kept, bits, nr_dec) begins at decision `base` of the stretch and the run
 * ends in front of decision `end`.  find(mark, &ev) gives the run's first sync event with dec >= mark whose word is enabled,
 * emit(type, dec, aux, word_index, inverted, nr_ok) takes the events in ascending dec.  Returns how many there were.
 */
template <class Find, class Emit>
__host__ __device__ inline uint32_t mfm_runbatch_walk(mfm_runbatch_auto *a, uint64_t base, uint64_t end, const uint32_t *kept, uint32_t nr_kept,
                                                      const uint32_t *bits, uint32_t nr_dec, const mfm_runbatch_params &P, Find find, Emit emit)
{
    uint32_t n = 0;
#pragma unroll 1
    for (;;) {
        if (a->mode == MFM_RUNBATCH_SEARCH) {
            mfm_runsync_event ev;
            if (!find(a->mark, &ev)) {
                break;
            }
            emit(MFM_POCSAG_EV_SYNC_FOUND, ev.dec, ev.seen, ev.word_index, ev.inverted, ev.distance);
            n++;
            a->word_index = ev.word_index;
            a->inverted = ev.inverted;
            a->mark = ev.dec + 1u;
            a->mode = MFM_RUNBATCH_RECEIVE;
        } else if (a->mode == MFM_RUNBATCH_RECEIVE) {
            if (a->mark + MFM_RUNBATCH_BATCH > end) {
                break;
            }
            emit(MFM_POCSAG_EV_BATCH, a->mark + MFM_RUNBATCH_BATCH - 1u, 0u, a->word_index, a->inverted, 0u);
            n++;
            a->mode = MFM_RUNBATCH_SLOT;
        } else {
            if (a->mark + MFM_RUNBATCH_FRAME > end) {
                break;
            }
            const uint32_t win = mfm_runbatch_window(kept, nr_kept, bits, nr_dec, a->mark + MFM_RUNBATCH_BATCH - base);
            const uint32_t seen = mfm_runsync_reverse(win) ^ (a->inverted ? 0xffffffffu : 0u);
            const bool keep = mfm_runsync_popcount(seen ^ mfm_runbatch_word_of(P, a->word_index)) <= P.keep_distance;
            emit(keep ? MFM_POCSAG_EV_SYNC_KEPT : MFM_POCSAG_EV_SYNC_LOST, a->mark + MFM_RUNBATCH_FRAME - 1u, seen, a->word_index, a->inverted, 0u);
            n++;
            if (keep) {
                a->mark += MFM_RUNBATCH_FRAME;
                a->mode = MFM_RUNBATCH_RECEIVE;
            } else { /* the next sync lies wholly behind the failed slot; polarity is decided anew */
                a->mark += MFM_RUNBATCH_FRAME + 31u;
                a->mode = MFM_RUNBATCH_SEARCH;
                a->word_index = 0;
                a->inverted = 0;
            }
        }
    }
    return n;
}

/* word z of the batch whose last decision is `dec`, as collected: LSB first, upright */
__host__ __device__ inline uint32_t mfm_runbatch_raw(const uint32_t *kept, uint32_t nr_kept, const uint32_t *bits, uint32_t nr_dec, uint64_t base,
                                                     uint64_t dec, uint32_t z, uint32_t inverted)
{
    const uint64_t p = dec + 1u - MFM_RUNBATCH_BATCH;
    return mfm_runbatch_window(kept, nr_kept, bits, nr_dec, p + 32u * z - base) ^ (inverted ? 0xffffffffu : 0u);
}

/* word w of the `kept` a run leaves: the decisions [mark, end) of the stretch from the stream the run started with */
__host__ __device__ inline uint32_t mfm_runbatch_keep(const uint32_t *kept, uint32_t nr_kept, const uint32_t *bits, uint32_t nr_dec, uint64_t base,
                                                      uint64_t mark, uint32_t left, uint32_t w)
{
    if (32u * w >= left) {
        return 0u;
    }
    const uint32_t v = mfm_runbatch_window(kept, nr_kept, bits, nr_dec, mark + 32u * w - base);
    return left - 32u * w >= 32u ? v : v & ((1u << (left - 32u * w)) - 1u);
}

/* a sync event of a run must be the run's own before the automaton follows it; prev: the run's event in front of it */
__host__ __device__ inline bool mfm_runbatch_event_ok(const mfm_runsync_event &e, const mfm_runsync_event *prev, uint64_t first_dec, uint32_t nr_dec,
                                                      uint32_t nr_words)
{
    return e.dec >= first_dec && e.dec - first_dec < nr_dec && (!prev || prev->dec < e.dec) && e.word_index < nr_words && e.inverted <= 1u;
}

/* What a state handed in from outside (mfm_runbatch_store_state) must satisfy before a kernel reads it; NULL when it does, else
 * a message that names the field.  The form is canonical: a device's and a twin's state of the same stream are the same bytes. */
inline const char *mfm_runbatch_state_check(const mfm_runbatch_state &st)
{
    if (st.has_stretch > 1u) {
        return "has_stretch must be 0 or 1";
    }
    if (st.reserved || st.reserved2) {
        return "reserved and reserved2 must be 0";
    }
    bool any = false;
    for (uint32_t w = 0; w < MFM_RUNBATCH_KEPT_WORDS; w++) {
        any = any || st.kept[w] != 0u;
    }
    if (!st.has_stretch) {
        return st.stretch_window || st.decs || st.mark || st.mode || st.word_index || st.inverted || st.nr_kept || any
                   ? "has_stretch is 0 but another field is not 0"
                   : nullptr;
    }
    if (st.decs >= MFM_RUN_POS_LIMIT || st.stretch_window >= MFM_RUN_POS_LIMIT) {
        return "decs and stretch_window must be below 2^62";
    }
    if (st.mode > MFM_RUNBATCH_SLOT) {
        return "mode must be MFM_RUNBATCH_SEARCH, _RECEIVE or _SLOT";
    }
    if (st.mode == MFM_RUNBATCH_SEARCH) {
        if (st.mark > st.decs + 31u) {
            return "mark must be at most decs + 31 in SEARCH";
        }
        return st.nr_kept || any || st.word_index || st.inverted ? "nr_kept, kept, word_index and inverted must be 0 in SEARCH" : nullptr;
    }
    if (st.mark == 0u || st.mark > st.decs || st.decs - st.mark != st.nr_kept) {
        return "nr_kept must be decs - mark, and mark 1 .. decs, in RECEIVE and SLOT";
    }
    if (st.mode == MFM_RUNBATCH_RECEIVE ? st.nr_kept >= MFM_RUNBATCH_BATCH : (st.nr_kept < MFM_RUNBATCH_BATCH || st.nr_kept >= MFM_RUNBATCH_FRAME)) {
        return "nr_kept must be below 512 in RECEIVE and 512 .. 543 in SLOT";
    }
    if (st.word_index > 7u || st.inverted > 1u) {
        return "word_index must be at most 7 and inverted 0 or 1";
    }
    for (uint32_t w = 0; w < MFM_RUNBATCH_KEPT_WORDS; w++) {
        const uint32_t have = st.nr_kept > 32u * w ? st.nr_kept - 32u * w : 0u;
        if (have < 32u && (st.kept[w] >> have) != 0u) {
            return "kept must hold no bit at or above bit nr_kept";
        }
    }
    return nullptr;
}

#endif /* MFM_RUNBATCH_H */
