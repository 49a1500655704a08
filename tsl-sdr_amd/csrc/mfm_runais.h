/*
 * mfm_runais.h - what the kernels of the burst AIS stage (mfm_runais_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runais_call) must state once: the layout of a run's bit segment, its share of the event slots and the bits a
 * stretch leaves behind.  The checks a run has to pass before anything of the payload is read are mfm_run_stage.h's.
 *
 * A run's segment is MFM_RUNAIS_HIST_WORDS words of history, then its nr_out sample bits (bit = sample > 0), then one word
 * of padding: segment bit 256 + j is output j of the run, i.e. stretch sample first_out + j.  The history is the channel's
 * carried tail when the run continues a stretch and zeros when it begins one: exactly the reference's zero-filled
 * prior_sample slots and registers (ais/ais_demod.c:44-50).
 */
#ifndef MFM_RUNAIS_H
#define MFM_RUNAIS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"

#define MFM_RUNAIS_HIST_WORDS 8u  /* (160 + 5) samples of register history, rounded to words */
#define MFM_RUNAIS_HIST_BITS (32u * MFM_RUNAIS_HIST_WORDS)
#define MFM_RUNAIS_MIN_SPACING 160u /* samples between two packet ends of a stretch at least (see the header) */

enum { MFM_RUNAIS_SEARCH = 0, MFM_RUNAIS_RECEIVE = 1 };

/* the state a run leaves, in the one form both the device and the host twin write: fields its mode does not use are zero
 * (a search that finds a preamble sets rd, start, last_sample, hist8 and cur_bit; a packet's end sets pos and r) */
__host__ __device__ inline void mfm_runais_canon(mfm_runais_state &s)
{
    if (s.mode == MFM_RUNAIS_SEARCH) {
        s.rd = s.start = 0;
        s.last_sample = s.hist8 = s.cur_bit = 0;
    } else {
        s.pos = s.r = 0;
    }
}

/*
 * What a state handed in from outside (mfm_runais_store_state) must satisfy before a kernel reads it; NULL when it does, else
 * a message that names the field.  From what the walker indexes with: a continuing run has first_out == outs and its segment
 * begins 256 samples in front of that, so the word index (pos - ws) >> 5 of the search and the bit index rd - ws of the
 * receiver are unsigned and in range only for pos >= outs and rd >= outs; the receiver writes packet bit cur_bit + k - 1 and
 * stops at 1280, so cur_bit <= 1279 and the packet holds nothing from cur_bit on; r is where the search last restarted, at or
 * in front of pos; start is the preamble in front of rd.  Fields the mode does not use are zero (mfm_runais_canon).
 */
inline const char *mfm_runais_state_check(const mfm_runais_state &st)
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
    if (st.reserved) {
        return "reserved must be 0";
    }
    if (st.outs >= MFM_RUN_POS_LIMIT || st.stretch_window >= MFM_RUN_POS_LIMIT) {
        return "outs and stretch_window must be below 2^62";
    }
    if (st.pos >= MFM_RUN_POS_LIMIT || st.r >= MFM_RUN_POS_LIMIT || st.rd >= MFM_RUN_POS_LIMIT || st.start >= MFM_RUN_POS_LIMIT) {
        return "pos, r, rd and start must be below 2^62";
    }
    if (st.mode > MFM_RUNAIS_RECEIVE) {
        return "mode must be 0 (SEARCH) or 1 (RECEIVE)";
    }
    if (st.last_sample > 1u) {
        return "last_sample must be 0 or 1";
    }
    if (st.hist8 > 0xffu) {
        return "hist8 must be below 256";
    }
    if (st.cur_bit >= 1280u) {
        return "cur_bit must be below 1280";
    }
    if (st.mode == MFM_RUNAIS_SEARCH) {
        if (st.rd || st.start || st.last_sample || st.hist8 || st.cur_bit) {
            return "rd, start, last_sample, hist8 and cur_bit must be 0 in SEARCH";
        }
        if (st.pos < st.outs) {
            return "pos must not be in front of outs in SEARCH";
        }
        if (st.r > st.pos) {
            return "r must not be behind pos in SEARCH";
        }
        for (uint32_t i = 0; i < 40u; i++) {
            if (st.packet[i]) {
                return "packet must be empty in SEARCH";
            }
        }
    } else {
        if (st.pos || st.r) {
            return "pos and r must be 0 in RECEIVE";
        }
        if (st.rd < st.outs) {
            return "rd must not be in front of outs in RECEIVE";
        }
        if (st.start > st.rd) {
            return "start must not be behind rd in RECEIVE";
        }
        for (uint32_t b = st.cur_bit; b < 1280u; b++) {
            if ((st.packet[b >> 5] >> (b & 31u)) & 1u) {
                return "packet must hold no bit from cur_bit on";
            }
        }
    }
    return nullptr;
}

/* words of a run's segment: history, bits, one word of padding (the tail is cut out with a funnel shift over two words) */
__host__ __device__ inline uint32_t mfm_runais_seg_words(uint32_t nr_out)
{
    return MFM_RUNAIS_HIST_WORDS + (nr_out + 31u) / 32u + 1u;
}

/* event slots of a run: packet ends are MFM_RUNAIS_MIN_SPACING samples apart, and one packet may be carried in */
__host__ __device__ inline uint32_t mfm_runais_slots(uint32_t nr_out)
{
    return nr_out / MFM_RUNAIS_MIN_SPACING + 1u;
}

/* word k (0 .. 7) of the tail a run leaves: segment bits [nr_out + 32 k, nr_out + 32 k + 32), which end with the run's last
 * sample and begin in the carried history when the run is shorter than 256 samples */
__host__ __device__ inline uint32_t mfm_runais_tail_word(const uint32_t *seg, uint32_t nr_out, uint32_t k)
{
    const uint32_t q = (nr_out >> 5) + k, s = nr_out & 31u;
    return s ? (seg[q] >> s) | (seg[q + 1] << (32u - s)) : seg[q];
}

#endif /* MFM_RUNAIS_H */
