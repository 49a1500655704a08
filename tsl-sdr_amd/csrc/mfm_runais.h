/*
 * mfm_runais.h - what the kernels of the burst AIS stage (mfm_runais_*, include/multifm_hip.h) and its host twin
 * (mfm_hosttwin_runais_call) must state once: the layout of a run's bit segment, its share of the event slots, the checks
 * a run has to pass before anything of the payload is read, and the bits a stretch leaves behind.
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

#define MFM_RUNAIS_HIST_WORDS 8u  /* (160 + 5) samples of register history, rounded to words */
#define MFM_RUNAIS_HIST_BITS (32u * MFM_RUNAIS_HIST_WORDS)
#define MFM_RUNAIS_MIN_SPACING 160u /* samples between two packet ends of a stretch at least (see the header) */

enum { MFM_RUNAIS_SEARCH = 0, MFM_RUNAIS_RECEIVE = 1 };

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

/*
 * The input-error flags of run `run` (0: it may be read).  prev: the run in front of it in the list (NULL for the first),
 * nr_elems: the resampler's total of output elements, state: the per-channel state the call started from.  words: the
 * resampler's bits form, where out_offset and nr_elems count 32-bit words and the run owns (nr_out + 31) / 32 of them.
 */
__host__ __device__ inline uint32_t mfm_runais_check_run(const mfm_runrs_run &run, const mfm_runrs_run *prev, uint32_t nr_channels,
                                                         uint64_t nr_elems, const mfm_runais_state *state, bool words = false)
{
    const uint64_t owned = words ? ((uint64_t)run.nr_out + 31u) / 32u : run.nr_out;
    if (run.channel >= nr_channels || (prev && prev->channel > run.channel) || run.out_offset > nr_elems ||
        owned > nr_elems - run.out_offset) {
        return MFM_RUNAIS_IN_BAD_RUNS;
    }
    if (run.flags & MFM_RUNRS_BEGINS) {
        return run.first_out != 0 ? MFM_RUNAIS_IN_BAD_RUNS : 0u;
    }
    /* only a channel's first run of a call can continue: a later one has a closed window in front of it */
    const bool first = !prev || prev->channel != run.channel;
    const mfm_runais_state &st = state[run.channel];
    return first && st.has_stretch && st.outs == run.first_out ? 0u : MFM_RUNAIS_IN_OUT_OF_STEP;
}

/* word k (0 .. 7) of the tail a run leaves: segment bits [nr_out + 32 k, nr_out + 32 k + 32), which end with the run's last
 * sample and begin in the carried history when the run is shorter than 256 samples */
__host__ __device__ inline uint32_t mfm_runais_tail_word(const uint32_t *seg, uint32_t nr_out, uint32_t k)
{
    const uint32_t q = (nr_out >> 5) + k, s = nr_out & 31u;
    return s ? (seg[q] >> s) | (seg[q + 1] << (32u - s)) : seg[q];
}

#endif /* MFM_RUNAIS_H */
