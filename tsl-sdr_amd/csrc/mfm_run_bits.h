/*
 * mfm_run_bits.h - what the burst AIS and POCSAG stages hand to the slicer of the sign-bit path (mfm_run_bits.hip): their
 * PCM slicers' arguments with the bit payload in the place of the PCM, and the two numbers in which the stages differ.
 */
#ifndef MFM_RUN_BITS_H
#define MFM_RUN_BITS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"

#define MFM_RUN_BITS_SLICE_NT 256u /* threads = segment words per workgroup, as the PCM slicers (their blk_base is shared) */

struct mfm_run_bits_slice {
    const struct mfm_runrs_run *runs;
    const uint32_t *bits;     /* the resampler's bits payload */
    const uint32_t *chan_old; /* the per-channel state the call started from, as words */
    const uint32_t *blk_base; /* [runs + 1] first slicer workgroup of a run */
    const uint32_t *seg_base; /* [runs] first word of a run's segment */
    const uint32_t *ctl;      /* [0] workgroups of the slicer, [1] runs */
    uint32_t *seg;
    uint32_t state_words;     /* words of one channel's state */
    uint32_t tail_word0;      /* where its tail begins */
    uint32_t hist_words;      /* words of the tail = of a segment's history */
};

/* queues the slicer on s; max_blocks as the PCM slicer's launch */
extern "C" __attribute__((visibility("hidden"))) int mfm_internal_run_bits_slice(const struct mfm_run_bits_slice *args, uint32_t max_blocks,
                                                                                hipStream_t s);

#endif /* MFM_RUN_BITS_H */
