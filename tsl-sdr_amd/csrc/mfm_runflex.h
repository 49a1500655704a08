/*
 * mfm_runflex.h - what the kernels of the burst FLEX stage (mfm_runflex_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runflex_call) must state once: the layout of a run's bit segment, where a PCM sample of a stretch lives, a
 * run's share of the event and frame slots, the coding table and the 4-level slicer, and the canonical form of the state a run
 * leaves.  The checks a run has to pass before anything of the payload is read are mfm_run_stage.h's.
 *
 * A run's segment is MFM_RUNFLEX_HIST_WORDS words of history, then its nr_out sample bits (bit = sample >= 0), then one word
 * of padding: segment bit 320 + j is output j of the run, i.e. stretch sample first_out + j.  The history is the sign of the
 * 320 stretch samples in front of the run, taken from the channel's ring when the run continues a stretch, and zeros when it
 * begins one or where the stretch has no sample (below 0).  The ten BS1 registers take every tenth sample and hold 32 bits, so
 * "a register reads 0xaaaaaaaa at sample n" looks at n, n - 10, ..., n - 310 and at nothing older.
 *
 * The ring.  PCM sample s of a stretch is output s - first_out of the run while s >= first_out and lives in the channel's ring
 * at s & 32767 below that.  The ring is written last, from the channel's last run of a call (its last 32 768 outputs at most).
 * A frame's end looks back over its block symbols, 5631 * 5 = 28 155 samples at most, the frame information word's arrival over
 * the 112 sync samples, 1 110: all within the ring.  A run that begins a stretch never reads the ring: no sample below 0 exists, and the search
 * opens at sample 310 (the registers are zero-filled at the stretch start as after every reset), so a stale ring is harmless.
 *
 * The bounds.  Every event is followed by a reset, and after a reset at sample x (the event's) the next event needs: the 310
 * samples in which no zero-filled register can match (the search looks at x + 311 first), a run of three matches or more
 * (x + 311 .. x + 313), the sample that ends it (j >= x + 314), t = 1 .. 10 samples to the first sync bit (s0 >= x + 315) and 790
 * more to the earliest event (BAD_BAUD at s0 + 790): two events of a stretch are at least 1105 samples apart, so a run of
 * nr_out samples holds at most nr_out / 1105 + 1 of them.  A FRAME event lies at the last block symbol e, which is
 * step + fudge + sync2 * step + (symbols - 1) * step >= 28 560 samples (the four codings: 28 560, 28 562, 28 560, 28 562) behind
 * the last FIW bit f = s0 + 1110: two FRAME events are at least 315 + 1110 + 28 560 = 29 985 samples apart and a run holds at
 * most nr_out / 29985 + 1 of them.
 */
#ifndef MFM_RUNFLEX_H
#define MFM_RUNFLEX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_stage.h"

#define MFM_RUNFLEX_HIST_WORDS 10u  /* 310 samples of register history, whole words */
#define MFM_RUNFLEX_HIST_BITS (32u * MFM_RUNFLEX_HIST_WORDS)
#define MFM_RUNFLEX_RING 32768u     /* PCM samples per channel the stage keeps */
#define MFM_RUNFLEX_DEAD 311u       /* first sample after a reset at r that can complete a BS1 register: r + 311 */
#define MFM_RUNFLEX_EVENT_SPACING 1105u  /* samples between two events of a stretch at least */
#define MFM_RUNFLEX_FRAME_SPACING 29985u /* samples between two FRAME events of a stretch at least */

enum { MFM_RUNFLEX_SEARCH = 0, MFM_RUNFLEX_SYNC1 = 1, MFM_RUNFLEX_FRAME = 2 };

#define MFM_RUNFLEX_SYNC1_WAIT 1120u  /* SYNC1 waits while j + (1 .. 10) + 1110 >= outs: j is at most this far behind outs */
#define MFM_RUNFLEX_FRAME_WAIT 28562u /* FRAME waits while the last block symbol, at most this far behind j, is >= outs */

/*
 * What a state handed in from outside (mfm_runflex_store_state) must satisfy before a kernel reads it; NULL when it does, else
 * a message that names the field.  From what the walker indexes with: a continuing run has first_out == outs, and the search
 * indexes the match plane with the unsigned p - first_out, so p >= outs; SYNC1 and FRAME read samples from j on out of the
 * ring and the run, j a sample the stretch has seen and recent enough that the wait is not over yet (which keeps everything
 * read within the ring's 32 768 samples); coding selects one of four rows; the swing values are int16 and cycle and frame the
 * FIW's 4 and 7 bits.  Fields a mode does not use are zero (mfm_runflex_canon).  The ring is PCM: any value is a sample.
 */
inline const char *mfm_runflex_state_check(const mfm_runflex_state &st)
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
    if (st.p >= MFM_RUN_POS_LIMIT || st.j >= MFM_RUN_POS_LIMIT) {
        return "p and j must be below 2^62";
    }
    if (st.mode > MFM_RUNFLEX_FRAME) {
        return "mode must be 0 (SEARCH), 1 (SYNC1) or 2 (FRAME)";
    }
    if (st.mode != MFM_RUNFLEX_FRAME) {
        if (st.coding || st.a || st.b || st.inv_a || st.fiw_raw || st.fiw || st.cycle || st.frame || st.sample_range || st.sample_delta) {
            return "coding, a, b, inv_a, fiw_raw, fiw, sample_range, sample_delta, cycle and frame must be 0 outside FRAME";
        }
    } else {
        if (st.coding >= 4u) {
            return "coding must be below 4 in FRAME";
        }
        if (st.sample_range != (int16_t)st.sample_range || st.sample_delta != (int16_t)st.sample_delta) {
            return "sample_range and sample_delta must fit int16";
        }
        if (st.cycle >= 16u || st.frame >= 128u) {
            return "cycle must be below 16 and frame below 128";
        }
    }
    if (st.mode == MFM_RUNFLEX_SEARCH) {
        if (st.j || st.eye) {
            return "j and eye must be 0 in SEARCH";
        }
        if (st.p < st.outs) {
            return "p must not be in front of outs in SEARCH";
        }
        if (st.run > st.outs || (st.run && st.p != st.outs)) {
            return "run must be at most outs, and 0 unless p is outs";
        }
    } else {
        if (st.p || st.run) {
            return "p and run must be 0 outside SEARCH";
        }
        if (st.eye < 3u || st.eye > 255u) {
            return "eye must be 3 .. 255 in SYNC1 and FRAME";
        }
        const uint64_t wait = st.mode == MFM_RUNFLEX_SYNC1 ? MFM_RUNFLEX_SYNC1_WAIT : MFM_RUNFLEX_FRAME_WAIT;
        if (st.j >= st.outs || st.outs - st.j > wait) {
            return st.mode == MFM_RUNFLEX_SYNC1 ? "j must be in front of outs by 1 .. 1120 samples in SYNC1"
                                                : "j must be in front of outs by 1 .. 28562 samples in FRAME";
        }
    }
    return nullptr;
}

/* words of a run's segment: history, bits, one word of padding (the views are cut out with a funnel shift over two words) */
__host__ __device__ inline uint32_t mfm_runflex_seg_words(uint32_t nr_out)
{
    return MFM_RUNFLEX_HIST_WORDS + (nr_out + 31u) / 32u + 1u;
}

/* event and frame slots of a run (the derivation is above) */
__host__ __device__ inline uint32_t mfm_runflex_event_slots(uint32_t nr_out)
{
    return nr_out / MFM_RUNFLEX_EVENT_SPACING + 1u;
}

__host__ __device__ inline uint32_t mfm_runflex_frame_slots(uint32_t nr_out)
{
    return nr_out / MFM_RUNFLEX_FRAME_SPACING + 1u;
}

/* _pager_codings[] (pager_flex.c:46-96) as mfm_flex.hip's fx_codings states it, in selects: no table, so host and device share
 * it; sync2 = 2 * (sync_2_samples + 16 / sym_bits) symbols (:460-525) */
struct MfmRunflexCoding {
    uint32_t seq_a, baud, levels, skip, fudge, nr_phases, sync2, symbols;
};

__host__ __device__ inline MfmRunflexCoding mfm_runflex_coding(uint32_t i)
{
    const bool fast = (i & 1u) != 0, four = (i & 2u) != 0; /* 3200 symbols per second; 4-level */
    MfmRunflexCoding c;
    c.seq_a = i == 0 ? 0x78f3u : (i == 1 ? 0x84e7u : (i == 2 ? 0x4f97u : 0x215fu));
    c.levels = four ? 4u : 2u;
    c.skip = fast ? 4u : 9u;
    c.fudge = fast ? 2u : 0u;
    c.nr_phases = (fast ? 2u : 1u) * (four ? 2u : 1u);
    c.baud = 1600u * c.nr_phases;
    c.sync2 = fast ? 80u : 40u;
    c.symbols = fast ? 5632u : 2816u;
    return c;
}

/* the coding whose A code differs from the upper half of `a` in fewer than 4 bits, 0xffffffff for none (:264-287) */
__host__ __device__ inline uint32_t mfm_runflex_find_coding(uint32_t a)
{
    for (uint32_t i = 0; i < 4; i++) {
#if defined(__HIP_DEVICE_COMPILE__)
        if (__popc(mfm_runflex_coding(i).seq_a ^ (a >> 16)) < 4) {
#else
        if (__builtin_popcount(mfm_runflex_coding(i).seq_a ^ (a >> 16)) < 4) {
#endif
            return i;
        }
    }
    return 0xffffffffu;
}

/* pager_flex.c:107-119 */
__host__ __device__ inline uint32_t mfm_runflex_checksum(uint32_t w)
{
    w &= 0x1fffffu;
    uint32_t s = 0;
    for (int n = 0; n < 6; n++) {
        s += (w >> (4 * n)) & 0xfu;
    }
    return s & 0xfu;
}

/* _pager_flex_slice_4fsk, pager_flex.c:148-171 */
__host__ __device__ inline uint32_t mfm_runflex_slice4(int v, int delta, int range)
{
    const int s = (int16_t)(v - delta);
    if (s < 0) {
        return (-s > range / 4) ? 0u : 1u;
    }
    return (s > range / 4) ? 2u : 3u;
}

/* which symbol of the block and which bit of it carries bit n of phase q (:1242-1285); false: the coding has no phase q */
__host__ __device__ inline bool mfm_runflex_phase_map(const MfmRunflexCoding &cd, uint32_t q, uint32_t *mul, uint32_t *add, uint32_t *sel)
{
    const bool four = cd.levels == 4u;
    *mul = 1;
    *add = 0;
    *sel = 0;
    if (cd.nr_phases == 1u) {
        return q == 0;
    }
    if (cd.nr_phases == 2u) {
        if (four) {
            *sel = q == 0;
        } else {
            *mul = 2;
            *add = q >> 1;
        }
        return q == 0 || q == 2;
    }
    *mul = 2;
    *add = q >> 1;
    *sel = (q & 1u) == 0;
    return true;
}

/* the state a run leaves, in the one form both the device and the host twin write: fields its mode does not use are zero */
__host__ __device__ inline void mfm_runflex_canon(mfm_runflex_state &s)
{
    if (s.mode != MFM_RUNFLEX_FRAME) {
        s.coding = s.a = s.b = s.inv_a = s.fiw_raw = s.fiw = s.cycle = s.frame = 0;
        s.sample_range = s.sample_delta = 0;
    }
    if (s.mode == MFM_RUNFLEX_SEARCH) {
        s.j = 0;
        s.eye = 0;
    } else {
        s.p = 0;
        s.run = 0;
    }
}

#endif /* MFM_RUNFLEX_H */
