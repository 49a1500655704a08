/*
 * mfm_runpocsag.h - what the kernels of the burst POCSAG stage (mfm_runpocsag_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runpocsag_call) must state once: the layout of a run's bit segment, its share of the event slots and the
 * bits a stretch leaves behind.  The checks a run has to pass before anything of the payload is read are mfm_run_stage.h's.
 *
 * A run's segment is MFM_RUNPOCSAG_HIST_WORDS words of history, then its nr_out sample bits (bit = sample < 0), then one
 * word of padding: segment bit 2400 + j is output j of the run, i.e. stretch sample first_out + j.  The history is the
 * channel's carried tail when the run continues a stretch and zeros when it begins one: exactly the reference's zero-filled
 * eye registers (pager/pager_pocsag.c:119-126), with the detector reset at stretch sample 0.
 *
 * The tail.  A detector of samples_per_bit S visits one of its S registers per sample, each register every S samples, and a
 * register holds the 32 bits shifted in last: what the detectors do at sample n depends on the sample bits n - j * S, j = 0 ..
 * 31, on their nr_eye_matches (carried in the state) and on nothing older.  The slowest detector has S = 75, so at most
 * 32 * 75 = 2400 samples before the current one matter (31 * 75 = 2325 are read): 75 whole words.
 *
 * The EXACT span.  A reset (stretch start or SYNC_LOST) zero-fills the registers, so a register's bit j is zero, whatever the
 * bit stream holds, while n - j * S lies before the reset: for n < reset + 31 * 75 the walker masks those bits off, from
 * there on the registers equal the free-running shifted views.  The span is the row stage's 31 bit periods of the slowest
 * rate; it is measured from the carried since_reset when a run continues a stretch.
 */
#ifndef MFM_RUNPOCSAG_H
#define MFM_RUNPOCSAG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"

#define MFM_RUNPOCSAG_HIST_WORDS 75u /* 32 bits * 75 samples per bit of register history = 2400 samples, whole words */
#define MFM_RUNPOCSAG_HIST_BITS (32u * MFM_RUNPOCSAG_HIST_WORDS)
#define MFM_RUNPOCSAG_SLOW_SPAN (31u * 75u)    /* samples after a reset during which some register bit is zero-filled */
#define MFM_RUNPOCSAG_MIN_SPACING (544u * 16u) /* samples between two BATCH events of a stretch at least (see the header) */
#define MFM_RUNPOCSAG_SYNC 0x7cd215d8u         /* pager_pocsag_priv.h:40 */

enum { MFM_RUNPOCSAG_SEARCH = 0, MFM_RUNPOCSAG_BATCH = 2, MFM_RUNPOCSAG_SYNCWORD = 3 };

/*
 * What a state handed in from outside (mfm_runpocsag_store_state) must satisfy before a kernel reads it; NULL when it does,
 * else a message that names the field.  From what the walker does with it: outs is the only position (the others are relative
 * to it); the reset lies at outs - since_reset, which must exist and is tracked for 2400 samples; nr_eye counts matches of the
 * stretch and is added to 32-bit run lengths; in BATCH and SYNCWORD the next bit is taken (spb - 1 - skip) mod 2^16 samples
 * on, bit batch_word * 32 + batch_bit of 512 or bit nr_sync_bits of 32 comes next, and the words collected hold nothing from
 * there on.  Fields a mode does not use are zero, as the walker leaves them.
 */
inline const char *mfm_runpocsag_state_check(const mfm_runpocsag_state &st)
{
    if (st.has_stretch > 1u) {
        return "has_stretch must be 0 or 1";
    }
    if (!st.has_stretch) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&st);
        for (uint32_t i = 0; i < sizeof(st) / 4u; i++) {
            if (w[i]) {
                return "has_stretch is 0 but another field is not 0";
            }
        }
        return nullptr;
    }
    if (st.outs >= MFM_RUN_POS_LIMIT || st.stretch_window >= MFM_RUN_POS_LIMIT) {
        return "outs and stretch_window must be below 2^62";
    }
    if (st.mode != MFM_RUNPOCSAG_SEARCH && st.mode != MFM_RUNPOCSAG_BATCH && st.mode != MFM_RUNPOCSAG_SYNCWORD) {
        return "mode must be 0 (SEARCH), 2 (BATCH) or 3 (SYNCWORD)";
    }
    if (st.mode == MFM_RUNPOCSAG_SEARCH) {
        if (st.baud || st.spb || st.skip) {
            return "baud, spb and skip must be 0 in SEARCH";
        }
        if (st.since_reset > MFM_RUNPOCSAG_HIST_BITS || st.since_reset > st.outs) {
            return "since_reset must be at most 2400 and at most outs";
        }
        for (int d = 0; d < 3; d++) {
            if (st.nr_eye[d] >= (1u << 31) || st.nr_eye[d] > st.outs) {
                return "nr_eye must be below 2^31 and at most outs";
            }
        }
    } else {
        if (!((st.spb == 75u && st.baud == 512u) || (st.spb == 32u && st.baud == 1200u) || (st.spb == 16u && st.baud == 2400u))) {
            return "spb and baud must be 75 / 512, 32 / 1200 or 16 / 2400 in BATCH and SYNCWORD";
        }
        if (st.skip > 0xffffu) {
            return "skip must fit 16 bits";
        }
        if (st.since_reset || st.nr_eye[0] || st.nr_eye[1] || st.nr_eye[2]) {
            return "since_reset and nr_eye must be 0 in BATCH and SYNCWORD";
        }
    }
    if (st.mode == MFM_RUNPOCSAG_BATCH) {
        if (st.batch_word >= 16u || st.batch_bit >= 32u) {
            return "batch_word must be below 16 and batch_bit below 32";
        }
        for (uint32_t b = st.batch_word * 32u + st.batch_bit; b < 512u; b++) {
            if ((st.batch[b >> 5] >> (b & 31u)) & 1u) {
                return "batch must hold no bit from batch_word * 32 + batch_bit on";
            }
        }
    } else {
        if (st.batch_word || st.batch_bit) {
            return "batch_word and batch_bit must be 0 outside BATCH";
        }
        for (uint32_t i = 0; i < 16u; i++) {
            if (st.batch[i]) {
                return "batch must be empty outside BATCH";
            }
        }
    }
    if (st.mode == MFM_RUNPOCSAG_SYNCWORD) {
        if (st.nr_sync_bits >= 32u || (st.sync_word >> st.nr_sync_bits) != 0u) {
            return "nr_sync_bits must be below 32 and sync_word hold no more bits than that";
        }
    } else if (st.nr_sync_bits || st.sync_word) {
        return "nr_sync_bits and sync_word must be 0 outside SYNCWORD";
    }
    return nullptr;
}

/* words of a run's segment: history, bits, one word of padding (the tail is cut out with a funnel shift over two words) */
__host__ __device__ inline uint32_t mfm_runpocsag_seg_words(uint32_t nr_out)
{
    return MFM_RUNPOCSAG_HIST_WORDS + (nr_out + 31u) / 32u + 1u;
}

/* event slots of a run: at most nr_out / 8704 + 1 BATCH events, at most two other events between two of them, in front of
 * the first and behind the last (the derivation is in the header) */
__host__ __device__ inline uint32_t mfm_runpocsag_slots(uint32_t nr_out)
{
    return 3u * (nr_out / MFM_RUNPOCSAG_MIN_SPACING + 1u) + 2u;
}

/* word k (0 .. 74) of the tail a run leaves: segment bits [nr_out + 32 k, nr_out + 32 k + 32), which end with the run's last
 * sample and begin in the carried history when the run is shorter than 2400 samples */
__host__ __device__ inline uint32_t mfm_runpocsag_tail_word(const uint32_t *seg, uint32_t nr_out, uint32_t k)
{
    const uint32_t q = (nr_out >> 5) + k, s = nr_out & 31u;
    return s ? (seg[q] >> s) | (seg[q + 1] << (32u - s)) : seg[q];
}

#endif /* MFM_RUNPOCSAG_H */
