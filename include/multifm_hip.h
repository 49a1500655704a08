/*
 * multifm_hip.h - C ABI of the MI355X multifm channel engine (libmultifm_hip.so).
 *
 * This is the drop-in boundary for multifm's per-channel hot path.  In the reference
 * (pvachon/tsl-sdr) every channel is a pthread that runs
 *
 *     demod_thread_process()            multifm/demod.c:48-121
 *       direct_fir_push_sample_buf()    filter/direct_fir.c:118-146
 *       direct_fir_process()            filter/direct_fir.c:422-453   (complex-tap decimating FIR
 *                                                                      + Q14 derotator)
 *       multifm_fm_demod_process()      multifm/fm_demod.c:36-85      (fast_atan2f discriminator)
 *       write(fifo_fd, pcm)             multifm/demod.c:93
 *
 * on every struct sample_buf that receiver_sample_buf_deliver() (multifm/receiver.c:78-98) hands it.
 * Here ONE engine object owns all channels of a receiver and runs that whole loop as one fused HIP
 * kernel per block of wideband samples.  The entry points below are what a reference-side
 * replacement of demod.c / receiver.c binds:
 *
 *   reference call                                   engine call
 *   ------------------------------------------------ -----------------------------------------
 *   demod_thread_new(.., offset_hz, samp_hz,         mfm_engine_add_channel()
 *       out_fifo, decimation, lpf_taps, nr_taps,
 *       fir_debug_output, gain)   demod.h:104-116
 *   (receiver_start)              receiver.c:268      mfm_engine_commit()
 *   receiver_sample_buf_deliver() receiver.c:78-98    mfm_engine_push() | acquire_input()+submit()
 *   write(fifo_fd, ...)           demod.c:93          mfm_engine_fetch() / mfm_engine_release()
 *   demod_thread_delete()         demod.c:163-190     mfm_engine_destroy()
 *
 * Conventions follow the reference's aresult_t style: every call returns an int, 0 (MFM_OK) on
 * success and a negative MFM_E_* on failure; nothing throws; handles are opaque; plain pointers and
 * sizes only.  All sample data is interleaved int16 I,Q exactly as in struct sample_buf::data_buf
 * (filter/sample_buf.h:59-102).  Output PCM is the same int16 stream a channel thread writes to its
 * FIFO; optional filtered IQ is the signalDebugFile stream (demod.c:75-81).
 *
 * The library has no CPU fallback: without a usable HIP device mfm_engine_create() fails with
 * MFM_E_DEVICE.
 */
#ifndef MULTIFM_HIP_H
#define MULTIFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFM_OK 0
#define MFM_E_INVAL (-1)  /* bad argument (TSL_ASSERT_ARG failures in the reference) */
#define MFM_E_NOMEM (-2)  /* host or device allocation failed */
#define MFM_E_BUSY (-3)   /* no free output slot / input buffer (direct_fir.c:136 A_E_BUSY analogue) */
#define MFM_E_DEVICE (-4) /* HIP runtime error or no device */
#define MFM_E_STATE (-5)  /* call not valid in this state (e.g. add_channel after commit) */
#define MFM_E_DONE (-6)   /* nothing to fetch (A_E_DONE analogue) */

#define MFM_ABI_VERSION 4 /* 2: mfm_resampler_config grew flags + reserved; mfm_flex_*, mfm_group_* added
                             3: mfm_stats grew timed_launches, rot_exact_channels, rot_fast_slices, k_steps, tap_hi_mask, taps_resident; MFM_F_TIMING_SPARSE, MFM_F_STREAM_TAPS;
                                mfm_group_config.exchange
                             4: mfm_engine_config / mfm_group_config grew coalesce_samples (+ a third ext_input); mfm_stats grew submits,
                                pending_samples; mfm_engine_flush, mfm_group_flush, mfm_engine_input_bytes_cfg, mfm_engine_replay,
                                mfm_engine_last_launch_input, mfm_engine_seek, mfm_host_alloc/free, mfm_*_push_pinned,
                                mfm_*_copy_done/_wait, mfm_devtest_discriminate; MFM_F_GATHER, MFM_F_OVERLAP */

/* flags for mfm_engine_config::flags */
#define MFM_F_DEVICE_ONLY 0x1u /* keep outputs in HBM; no host mirror, fetch() unavailable */
#define MFM_F_TIMING 0x2u      /* bracket every kernel launch with HIP events (an engine with two compute streams reads the
                                  kernel's own stamps instead: mfm_stats::kernel_ms) */
#define MFM_F_FORCE_DOT2 0x4u  /* run the v_dot2 (packed int16 VALU) kernel even where the matrix-core kernel applies:
                                  both produce the same bits; parity tests and A/B timing select it here */
#define MFM_F_FORCE_MFMA_V1 0x8u /* where both matrix-core kernels apply, run the first-generation one (31-output column
                                  blocks, 2-byte PCM stores) instead of the second (64-output tiles, 8-byte stores) */

#define MFM_F_TIMING_SPARSE 0x20u /* with MFM_F_TIMING: bracket one launch in four only (a back-to-back stream then runs
                                     without an event pair between most kernels; mfm_stats.timed_launches says how many
                                     durations kernel_ms sums) */
#define MFM_F_GROUP_SHARED_DEVICE 0x40u /* mfm_group_config only, a TEST AID: the same device may be listed several times, so that
                                           a group of several shards runs on a one-GPU box (real RCCL refuses such a communicator;
                                           tests/hoststub/fake_rccl.cpp stands in for it) */
#define MFM_F_STREAM_TAPS 0x80u /* filters of 129..512 taps on the matrix kernel: re-read the taps from L2 in every iteration
                                  (the round-1 form: 128 registers, two workgroups per CU) instead of keeping all of them in
                                  registers (256 registers, one workgroup per CU); same bits; parity tests and A/B timing */
#define MFM_F_GATHER 0x100u    /* with coalesce_samples: launch only once coalesce_samples have gathered, or on mfm_engine_flush() /
                                  mfm_engine_sync() - never because the device happens to be idle (a producer that knows when
                                  its backlog ends and flushes then; deterministic launch boundaries for tests) */
#define MFM_F_OVERLAP 0x200u   /* second-generation kernel: consecutive launches alternate between two compute streams.  A launch
                                  depends on the one before it through input samples only (it recomputes the output in front of
                                  it and finds its rotator position from the stream's output count), so the next launch's
                                  workgroups take the slots the current one's shorter chunks free up instead of waiting for
                                  its last tile and a dispatch.  mfm_engine_stream() then returns the stream of the most
                                  recent launch, and the engine goes on alternating after the stream has been handed out
                                  (without the flag it alternates only until then: mfm_engine_stream).  The carry of an
                                  alternating launch of int16 blocks on mfm_kernel_v3.hip is copied at submit time, behind the
                                  block's producer and behind no channel kernel, into a ring of the engine's own from which the
                                  next launch reads it; 8-bit blocks and the long-filter kernels copy it on the next launch's
                                  stream.  Per-launch durations (MFM_F_TIMING) of an engine with two streams are the kernel's
                                  own stamps (mfm_stats::kernel_ms).  Ignored by the other kernels. */
#define MFM_F_V3L_ONE_ROW_BLOCK 0x400u /* long filters on the second generation (mfm_kernel_v3l.hip): one row block (8 channels) per
                                  wave - slices of 64 channels - also where two would fit (slices of 128: the default for more
                                  than 64 channels when two row blocks' taps fit 128 registers); same bits; parity tests, A/B timing */
#define MFM_F_SLICE_128 0x800u  /* 128-tap filters (filter/direct_fir.c:363-384 at multifm's 2.4 MS/s -> 25 kS/s geometry) on slices of
                                  128 channels - two row blocks per wave share every B fragment and every staged image
                                  (mfm_kernel_v3l.hip) - whatever the channel count; the default takes them from 512 channels on,
                                  where they measured faster than slices of 64 (by 0.6-1.4 %).  Same bits; parity tests, A/B timing */
#define MFM_F_SLICE_64 0x1000u  /* ... never: slices of 64 channels (mfm_kernel_v3.hip) at any channel count */
#define MFM_F_PCM_WRITE_BACK 0x2000u /* second-generation kernels: PCM stores never go through to memory with system scope (the default does
                                  that for launches of 512 channels and more: less L2-miss traffic there); same bits; parity tests, A/B timing */
#define MFM_F_WIDEN_8BIT 0x10u /* mfm_engine_push_bytes: always widen 8-bit blocks to int16 in HBM first, also where the
                                  matrix kernel could read the bytes themselves (same bits; parity tests and A/B timing) */

struct mfm_engine_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    uint32_t sample_rate_hz;    /* receiver sampleRateHz, receiver.c:138 */
    uint32_t decimation;        /* decimationFactor, receiver.c:160-172 */
    uint32_t max_block_samples; /* largest block one push()/submit() may carry */
    uint32_t flags;             /* MFM_F_* */
    /* Optional caller-owned device memory for the input staging buffers (two; three with coalesce_samples), each at
     * least mfm_engine_input_bytes_cfg() bytes (lets a caller hand in torch/RCCL-registered memory).
     * NULL = the engine allocates. */
    void *ext_input[3];
    /*
     * Backlog coalescing.  A channel thread of the reference takes whatever its work queue holds - up to 128 queued
     * sample_bufs (multifm/demod.c:297) - and runs them back to back (demod.c:134-150): its cost per sample does not depend
     * on the size of the buffers a front end delivers (4096 samples from file_if.c:18, 131072 from rtl_sdr_if.c:46).  A
     * kernel launch has a fixed cost, so the engine does the same with launches: with coalesce_samples > 0 a submitted block
     * is APPENDED to the input buffer being filled, and the buffer is launched as one pass
     *   - at once when the device has nothing to do (a live stream keeps its latency),
     *   - with one launch in flight, as soon as a quarter of that launch's samples have gathered (the device never runs dry),
     *   - otherwise when coalesce_samples have gathered, or on mfm_engine_flush() / mfm_engine_sync().
     * The output stream is the same in every case (it never depended on the blocking: filter/direct_fir.c:328-417 walks
     * sample by sample); mfm_engine_fetch() returns one block per LAUNCH.  0 = every submit is a launch (rounds 1-3).
     */
    uint32_t coalesce_samples;
    uint32_t reserved;          /* 0 */
};

struct mfm_engine; /* opaque */

struct mfm_block {
    uint64_t first_output; /* stream index of pcm[.][0] */
    size_t nr_outputs;     /* outputs per channel in this block */
    size_t stride;         /* elements between consecutive channels */
    const int16_t *pcm;    /* [nr_channels][stride] host memory, valid until release() */
    const int16_t *iq;     /* [nr_channels][2*stride] filtered I,Q or NULL */
};

struct mfm_stats {
    uint64_t samples_in;       /* wideband samples accepted */
    uint64_t outputs;          /* outputs produced per channel */
    uint64_t launches;         /* kernel launches */
    double kernel_ms;          /* sum of the durations of `timed_launches` launches (MFM_F_TIMING): HIP event pairs on an engine
                                  with one compute stream.  On an engine with two (MFM_F_OVERLAP, or by itself:
                                  mfm_engine_stream) no event pairs are recorded - a pair around a launch that shares the chip
                                  with the one before it measures its wait for workgroup slots - and a duration is what the
                                  kernel stamped itself: the 100 MHz reference ticks of its LONGEST WORKGROUP'S own run time
                                  (mfm_engine_get_launch_cycles), not a span on a stream.  Consecutive launches overlap by
                                  their ragged ends, so the mean of these may exceed the step period; a speed claim rests on
                                  the step time (bench.py: ms_per_step), not on kernel_ms.  A stamp that left the readable
                                  half of the stamp ring before it was folded is not counted in timed_launches. */
    uint32_t nr_channels;
    uint32_t nr_taps;
    uint32_t outputs_per_tile; /* kernel geometry, informational */
    uint32_t lds_bytes;
    uint32_t grid_last;        /* workgroups of the last launch */
    uint32_t tail_samples;     /* unconsumed samples carried to the next block */
    uint64_t rot_table_entries;
    uint32_t kernel_variant;   /* 0 = v_dot2 kernel, 1 = int8-MFMA (FIR-as-GEMM) kernel, 2 = its second generation */
    uint32_t pending_blocks;   /* finished or in-flight blocks not yet fetched + released */
    uint64_t launches_8bit;    /* of `launches`: those that read an 8-bit block as bytes (mfm_engine_push_bytes) */
    uint64_t timed_launches;   /* launches whose duration is in kernel_ms: all of them with MFM_F_TIMING, one in four
                                  with MFM_F_TIMING_SPARSE as well */
    uint32_t rot_exact_channels; /* channels whose rotator (filter/direct_fir.c:151-172) is exactly +-(16384, 0) for ever:
                                    offsets at multiples of half the output rate; their derotation is the identity or a
                                    sign flip */
    uint32_t rot_fast_slices;  /* 64-channel slices of the second-generation kernel made of such channels only */
    uint32_t k_steps;          /* matrix kernels: k-steps of 64 int16 elements (32 complex taps) per output, padded */
    uint32_t tap_hi_mask;      /* matrix kernels: bit k set = k-step k has taps beyond one byte, so its two products with
                                  the high-byte tap plane are issued (4 matrix instructions for that k-step, else 2) */
    uint32_t taps_resident;    /* first-generation matrix kernel, filters of 129..512 taps: 1 = int16 blocks run an instance that
                                  keeps every k-step of taps in registers, 0 = the taps are streamed from L2 (MFM_F_STREAM_TAPS,
                                  or no resident instance for the geometry) */
    uint32_t slice_channels;   /* matrix kernels: channels whose workgroup shares one staged image: 64, or 128 on the long-filter kernel with
                                  two row blocks per wave (129..512 taps at more than 64 channels; 128 taps from 512 channels on or with
                                  MFM_F_SLICE_128); 0: the v_dot2 kernel */
    uint64_t submits;          /* blocks accepted (mfm_engine_submit / push); with coalesce_samples several of them share a launch */
    uint64_t pending_samples;  /* samples accepted and not yet launched (coalesce_samples; mfm_engine_flush launches them) */
    uint64_t overlapped_launches; /* of `launches`: those that went to the other compute stream than the launch before them
                                  and left their carry to a copy of the engine's own, so that the next launch's workgroups
                                  moved into their ragged end (MFM_F_OVERLAP, or by itself: mfm_engine_stream) */
    uint32_t pinned;           /* 1: the engine's stream has been handed out (mfm_engine_stream) or the engine belongs to a
                                  device group, and MFM_F_OVERLAP is not set: one compute stream */
    uint32_t reserved2;        /* 0 */
};

/* Size in bytes of one input staging buffer for this configuration and tap count (coalesce_samples = 0). */
size_t mfm_engine_input_bytes(uint32_t max_block_samples, uint32_t nr_taps);
/* The same for a configuration with coalesce_samples; also how many buffers the engine uses (2, or 3 when it coalesces:
 * one being read, one queued behind it, one being filled), i.e. how many ext_input pointers it wants. */
size_t mfm_engine_input_bytes_cfg(const struct mfm_engine_config *cfg, uint32_t nr_taps, uint32_t *nr_buffers);

int mfm_engine_create(struct mfm_engine **pe, const struct mfm_engine_config *cfg);
void mfm_engine_destroy(struct mfm_engine **pe);

/*
 * Register a channel the way demod_thread_new() does (multifm/demod.h:104-116): real low-pass taps
 * are rotated to offset_hz and quantised to Q14 (demod.c:204-269), the derotator increment is
 * derived from offset_hz and the decimation (direct_fir.c:72-79).  want_iq != 0 asks for the
 * filtered-IQ stream too (fir_debug_output).  Returns the channel index (>= 0) or MFM_E_*.
 * All channels of one engine share nr_taps (the reference shares lpfTaps, receiver.c:175-184).
 */
int mfm_engine_add_channel(struct mfm_engine *e, int32_t offset_hz, const double *lpf_taps, size_t nr_taps,
                           double channel_gain, int want_iq);

/* Same, from already-quantised Q14 taps and rotator increment (fixtures, tests). */
int mfm_engine_add_channel_q14(struct mfm_engine *e, const int16_t *coeff_re, const int16_t *coeff_im,
                               size_t nr_taps, int16_t rot_incr_re, int16_t rot_incr_im, int want_iq);

/* Read back what a channel was programmed with (Q14 taps, rotator increment as {re, im}). */
int mfm_engine_get_channel(struct mfm_engine *e, uint32_t chan, int16_t *coeff_re, int16_t *coeff_im,
                           int16_t rot_incr[2]);

/* Freeze the channel set: build tap/rotator tables, allocate device buffers. */
int mfm_engine_commit(struct mfm_engine *e);

/*
 * Zero-copy ingest.  acquire_input() returns device memory where the caller (an H2D copy, an RCCL
 * broadcast, a generator kernel) must write the next block; submit() then processes nr_samples of
 * it.  With wait_producer != 0, producer_stream is the hipStream_t the data was produced on (NULL is
 * the legacy default stream, which is what torch's default stream is): the engine's compute stream
 * waits for the work queued there so far (no host sync).  With wait_producer == 0 the caller
 * guarantees the data is already in place.  Blocks are processed in submit order.
 */
int mfm_engine_acquire_input(struct mfm_engine *e, void **d_dst, size_t *capacity_samples);
int mfm_engine_submit(struct mfm_engine *e, size_t nr_samples, void *producer_stream, int wait_producer);

/* Host ingest: copies nr_samples interleaved int16 IQ pairs (any count <= max_block_samples) and
 * submits them.  Returns as soon as the copy has been staged; never blocks longer than a memcpy. */
int mfm_engine_push(struct mfm_engine *e, const int16_t *iq, size_t nr_samples);

/*
 * Host ingest of 8-bit captures: the byte pairs are staged as they are (half the
 * PCIe bytes of mfm_engine_push).  Where a matrix-core kernel runs and no channel asked for its filtered IQ they stay
 * bytes in HBM and the kernel's GEMM takes them as its one sample plane (same bits as the widened path); otherwise - and
 * for a cu8 block of odd length, or behind a history of another format - they are widened to int16 on the device exactly
 * as the reference's front ends do on the host.  nr_samples IQ pairs = 2 * nr_samples bytes.
 */
#define MFM_IN_CS16 0       /* interleaved int16, same as mfm_engine_push (multifm/file_if.c:46-64) */
#define MFM_IN_CS8 1        /* signed bytes, sign-extended (multifm/file_if.c:66-111) */
#define MFM_IN_CU8 2        /* file_if's "cu8": bytes read as SIGNED, minus 127; after an odd number of samples the
                               last one is stored without the subtraction (multifm/file_if.c:113-157) */
#define MFM_IN_RTLSDR_U8 3  /* unsigned bytes, (b - 127) << 7 (multifm/rtl_sdr_if.c:146-158) */
int mfm_engine_push_bytes(struct mfm_engine *e, const void *bytes, size_t nr_samples, int format);
/*
 * Host ingest without the staging copy.  The reference's sample_bufs come from a fixed pool (frame_alloc_new,
 * multifm/receiver.c:154-157); when that pool is page-locked memory (mfm_host_alloc) the H2D copy reads data_buf where
 * the front end wrote it.  mfm_engine_push_pinned() is mfm_engine_push_bytes() (any MFM_IN_* format) on such memory: it
 * returns at once with a ticket, and the buffer must stay untouched until mfm_engine_copy_done(ticket) says 1 (or
 * mfm_engine_copy_wait returns) - that is when the reference would sample_buf_decref() it (filter/direct_fir.c:395).
 */
void *mfm_host_alloc(size_t bytes); /* page-locked host memory (hipHostMalloc); NULL on failure */
/* The host <-> device link by itself, as a yardstick for host-fed throughput (bench.py `link`): total_bytes leave an arena of
 * page-locked memory in pieces of piece_bytes (one hipMemcpyAsync each on one stream, as the engine's pinned pushes do per
 * sample_buf), while d2h_per_h2d bytes per input byte come back on a second stream (the PCM mirror; 0: none).  Rates in
 * GB/s over the second of two passes. */
int mfm_link_probe(int device, size_t piece_bytes, size_t total_bytes, double d2h_per_h2d, double *h2d_GBps, double *d2h_GBps);
/* the same with the pieces gap_bytes apart in the arena (a sample_buf's header between the data of two frames) and
 * pieces_per_command of them per copy command - one strided hipMemcpy2DAsync that packs them on the device, what
 * mfm_engine_push_pinned_run() issues for a run of adjacent frames */
int mfm_link_probe_runs(int device, size_t piece_bytes, size_t gap_bytes, size_t pieces_per_command, size_t total_bytes,
                        double d2h_per_h2d, double *h2d_GBps, double *d2h_GBps);
void mfm_host_free(void *p);
int mfm_engine_push_pinned(struct mfm_engine *e, const void *data, size_t nr_samples, int format, uint64_t *ticket);
int mfm_engine_copy_done(struct mfm_engine *e, uint64_t ticket); /* 1: read, 0: not yet, < 0: error */
int mfm_engine_copy_wait(struct mfm_engine *e, uint64_t ticket);
/* The same for a producer on the device (a collective, a capture card's DMA): where the next block's BYTES go, two per
 * sample, when the engine's kernel can read them as they are - the second-generation matrix kernel, and no history of
 * another format in front (MFM_E_STATE otherwise: widen the block as the reference does and use
 * mfm_engine_acquire_input).  Then mfm_engine_submit() as for int16 blocks; a cu8 block must be of even length. */
int mfm_engine_acquire_input_bytes(struct mfm_engine *e, int format, void **d_dst, size_t *capacity_samples);

/* Oldest finished block, in submit order (blocks with zero outputs are skipped).  Waits for the
 * device.  MFM_E_DONE when nothing is pending.  The block stays valid until release(). */
int mfm_engine_fetch(struct mfm_engine *e, struct mfm_block *blk);
int mfm_engine_release(struct mfm_engine *e);

/* Device-resident view of the most recent submit's outputs (MFM_F_DEVICE_ONLY users). */
int mfm_engine_last_output_device(struct mfm_engine *e, void **d_pcm, size_t *stride, size_t *nr_outputs,
                                  void **d_iq);

/* What the most recent launch read: device address of its [history tail | blocks] and the sample count (self-checks that
 * re-run a launch's input through a reference; valid until nbuf - 1 further launches have been queued).  A launch that took
 * its first samples from the engine's carry ring (MFM_F_OVERLAP) leaves the buffer's front stale: the call then waits for that
 * launch and puts them there before it returns.  Producer-side call. */
int mfm_engine_last_launch_input(struct mfm_engine *e, void **d_in, size_t *nr_samples, int *format);

/* coalesce_samples: launch what has been accepted and not yet launched (MFM_E_BUSY when every output slot holds an
 * unfetched block: fetch / release and call again).  Producer side: the thread that submits.  No-op otherwise. */
int mfm_engine_flush(struct mfm_engine *e);

/* Wait for everything submitted so far (launches pending samples first, as mfm_engine_flush, and returns its MFM_E_BUSY).
 * Threading: push / stage / acquire_input / submit / flush / sync / seek / reset are PRODUCER-side calls and belong to one
 * thread at a time; fetch / release (and get_stats, copy_done / copy_wait) may run on another.  A flush that finds nothing
 * gathered is safe from any thread (it tests under the engine's lock). */
int mfm_engine_sync(struct mfm_engine *e);

/*
 * A producer loop in C, for measurements: `nr_blocks` times { acquire_input(); submit(block_samples, no producer) } on
 * whatever the input buffers hold (the caller pre-fills them), exactly what a C host does per delivered sample_buf
 * without the per-call cost of a scripting language in between.  Stops at the first error and returns it.
 */
int mfm_engine_replay(struct mfm_engine *e, size_t block_samples, size_t nr_blocks);

/* Forget the stream: history tail, rotator phase and discriminator state go back to a fresh
 * stream (what restarting the reference does). Pending blocks are dropped. */
int mfm_engine_reset(struct mfm_engine *e);

/*
 * Resume a stream that had produced outputs_before outputs per channel (a receiver restarted from a checkpoint): as
 * mfm_engine_reset(), except that the derotators stand where outputs_before steps of their recurrence leave them
 * (filter/direct_fir.c:151-172 carries rot_phase across buffers; the recurrence is input independent) and
 * mfm_block::first_output goes on counting from there.  The filter history and the discriminator's last sample start
 * empty, as after a restart of the reference.
 */
int mfm_engine_seek(struct mfm_engine *e, uint64_t outputs_before);

int mfm_engine_get_stats(struct mfm_engine *e, struct mfm_stats *st);

/* MFM_F_TIMING: durations (ms; HIP events on the compute stream, or - on an engine with two compute streams - the kernel's
 * own stamps, mfm_stats::kernel_ms) of the most recent timed launches, oldest first; at most `cap` and at most the last
 * 4096.  Returns how many were written. */
size_t mfm_engine_get_launch_ms(struct mfm_engine *e, float *dst, size_t cap);
/* MFM_F_TIMING, second-generation kernels: the last launches' durations in the shader's own clocks, oldest first - the
 * longest workgroup's s_memtime (shader-clock ticks) and s_memrealtime (100 MHz reference ticks) difference, stamped by the
 * kernel itself.  shader / ref * 100 MHz is the clock the launch really ran at; shader ticks against the kernel's issue
 * cycles is how much of the launch the SIMDs were issuing (bench.py: roofline.issue_model).  Waits for the launches issued so
 * far and nothing else: samples that were accepted and not yet launched stay where they are (no flush - the call is read-only,
 * also on a device group's shard engines).  At most the last 512 launches.  0 entries for launches that left no stamp; returns the number of entries written (0 without MFM_F_TIMING or on the other
 * kernels).  Either array may be NULL. */
size_t mfm_engine_get_launch_cycles(struct mfm_engine *e, uint64_t *shader_ticks, uint64_t *ref_ticks, size_t cap);

/* The engine's compute stream (hipStream_t), for callers that order their own work after it: THE stream every later launch
 * is ordered on (with MFM_F_OVERLAP: the one the most recent launch went to, and the next call may return the other).
 *
 * Handing the stream out PINS the engine.  An engine alternates its launches between two compute streams without being
 * asked (as MFM_F_OVERLAP does, early carry included) while nobody can tell: int16 blocks on mfm_kernel_v3.hip,
 * MFM_F_DEVICE_ONLY, two input buffers (no coalesce_samples), a launch that fills the workgroup slots more than once, not a
 * member of a device group - and this function not called yet.  Such an engine can only be observed through
 * mfm_engine_sync(), fetch and the stats calls, which wait for both streams.  The first call here joins the two (the stream
 * returned waits for the other one's last launch), and from then on the engine launches on that one stream, with the carry
 * in the kernel.  A caller that asks before its first submit gets an engine that never alternated; mfm_stats::pinned and
 * ::overlapped_launches tell.  (mfm_engine_last_output_device() returns no stream and pins nothing: order consumers through
 * this call.)  Producer-side call. */
void *mfm_engine_stream(struct mfm_engine *e);

const char *mfm_strerror(int err);
const char *mfm_last_error(void); /* thread-local detail of the last failure */

/*
 * ---- one channel set on several GPUs of a node (SURVEY.md section 8b "set_devices", section 8e) -----------------
 * The reference fans every delivered sample_buf out to all channel threads (multifm/receiver.c:78-98).  A device
 * group does the same across GPUs: channels are cut into contiguous shards (mfm_shard_range), one engine per device;
 * mfm_group_push() stages a block on the first device and exchanges it with RCCL over xGMI (ncclBroadcast, or a scatter
 * plus ncclAllGather: MFM_X_*), in place into every other engine's input buffer, then every engine runs its shard - all
 * shards take a block or none does; a failure after the first shard has taken it makes every later call fail with
 * MFM_E_DEVICE rather than let the shards drift apart.  No other exchange.  Blocks come back per
 * shard: mfm_group_fetch() fills one mfm_block per shard, all for the same stream position; channel c of the group is
 * row c - first_channel of its shard's block (mfm_group_shard_info).  One host thread at a time may push, another one
 * fetch/release (as for a single engine).  RCCL (librccl.so) is loaded at run time, and only by groups that exchange.
 */
#define MFM_GROUP_MAX_DEVICES 16
#define MFM_X_AUTO 0u /* one device: direct staging, no RCCL; several: RCCL broadcast */
#define MFM_X_RCCL 1u /* always through the RCCL broadcast path (exercises the call sequence on a one-GPU box) */
#define MFM_X_RCCL_ALLGATHER 2u /* RCCL, large-block form for point-to-point xGMI: the root sends 1/S of the block to each of
                                   its S - 1 peers (ncclSend/ncclRecv, S - 1 links at once), then ncclAllGather in place -
                                   no single link carries the whole block, as it does along a broadcast's ring */

struct mfm_group_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    uint32_t nr_devices;        /* 1..MFM_GROUP_MAX_DEVICES; devices beyond the channel count stay idle */
    int32_t devices[MFM_GROUP_MAX_DEVICES]; /* HIP device ordinals; devices[0] ingests and is the broadcast root */
    uint32_t sample_rate_hz;
    uint32_t decimation;
    uint32_t max_block_samples;
    uint32_t flags;             /* MFM_F_* handed to every engine (MFM_F_DEVICE_ONLY: see mfm_group_submit) */
    uint32_t exchange;          /* MFM_X_* */
    uint32_t coalesce_samples;  /* as mfm_engine_config::coalesce_samples; the shards launch or defer together */
    uint32_t reserved;          /* 0 */
};

struct mfm_group; /* opaque */

/* channels [first, first + count) of nr_channels belong to shard `shard` of nr_shards: contiguous ranges whose sizes
 * differ by at most one (empty only when there are fewer channels than shards).  Pure function. */
void mfm_shard_range(uint32_t nr_channels, uint32_t nr_shards, uint32_t shard, uint32_t *first, uint32_t *count);

int mfm_group_create(struct mfm_group **pg, const struct mfm_group_config *cfg);
void mfm_group_destroy(struct mfm_group **pg);
/* as mfm_engine_add_channel(); returns the channel's index in the group */
int mfm_group_add_channel(struct mfm_group *g, int32_t offset_hz, const double *lpf_taps, size_t nr_taps, double channel_gain,
                          int want_iq);
/* cut the shards, create and commit one engine per non-empty shard, set up the RCCL communicators */
int mfm_group_commit(struct mfm_group *g);
int mfm_group_nr_shards(struct mfm_group *g); /* >= 1 after commit */
int mfm_group_shard_info(struct mfm_group *g, uint32_t shard, uint32_t *first_channel, uint32_t *nr_channels, int32_t *device);
/* Blocks that are in device memory already (a producer kernel, a peer copy, another library's collective wrote them): the
 * ROOT's input buffer is where they go - acquire_input() names the address, as mfm_engine_acquire_input() - and submit()
 * exchanges the nr_samples int16 samples there to the other shards and submits them on every shard, in the same order and
 * under the same all-or-nothing rules as a host block (mfm_group_push).  The caller has made sure the block is complete
 * before it submits.  With MFM_F_DEVICE_ONLY in the group's flags the shards keep their outputs in HBM (no host mirror, no
 * mfm_group_fetch): a throughput measurement, or a consumer that works on the device. */
int mfm_group_acquire_input(struct mfm_group *g, void **d_dst, size_t *capacity_samples);
int mfm_group_submit(struct mfm_group *g, size_t nr_samples);
/* shard `shard`'s engine, for the READ-ONLY engine calls (get_stats, get_launch_ms / _cycles, last_output_device,
 * last_launch_input, get_channel with the shard's own channel numbers); NULL when there is no such shard */
struct mfm_engine *mfm_group_shard_engine(struct mfm_group *g, uint32_t shard);
/* host ingest of one block in any MFM_IN_* format.  MFM_E_BUSY when a shard's output ring is full (nothing was
 * staged on any shard: fetch/release and retry). */
int mfm_group_push(struct mfm_group *g, const void *data, size_t nr_samples, int format);
/* the same out of page-locked memory (mfm_host_alloc), without the staging copy: as mfm_engine_push_pinned() */
int mfm_group_push_pinned(struct mfm_group *g, const void *data, size_t nr_samples, int format, uint64_t *ticket);
/* A RUN of page-locked buffers of nr_samples_each samples that lie stride_bytes apart in one arena - a pool that hands its
 * frames out in address order delivers neighbours one after the other (host/mfm_tsl.c frame_alloc, host/mfm_receiver.c) - goes
 * to the device as ONE strided copy command and is accepted as one block.  One command per 512 KiB sample_buf runs at half the
 * link's rate, one per 16 KiB file_if buffer at a ninth (bench.py end_to_end.link).  *accepted (>= 1 on MFM_OK) = how many
 * buffers of the run were taken: fewer than `count` when less fits the buffer being filled or the gathering policy would have
 * launched in between; the caller offers the rest again.  One ticket covers the accepted buffers. */
int mfm_engine_push_pinned_run(struct mfm_engine *e, const void *first, size_t stride_bytes, size_t nr_samples_each, size_t count,
                               int format, uint64_t *ticket, size_t *accepted);
int mfm_group_push_pinned_run(struct mfm_group *g, const void *first, size_t stride_bytes, size_t nr_samples_each, size_t count,
                              int format, uint64_t *ticket, size_t *accepted);
size_t mfm_engine_input_room(struct mfm_engine *e); /* samples the buffer being filled still takes */
/* mfm_group_replay_pinned() over one arena of buffers stride_bytes apart, in runs of up to max_run neighbours (measurements) */
int mfm_group_replay_arena(struct mfm_group *g, const void *arena, size_t stride_bytes, size_t nr_bufs, size_t buf_samples, int format,
                           size_t nr_pushes, size_t max_run, uint64_t *outputs_per_channel, uint64_t *copy_commands);
int mfm_group_copy_done(struct mfm_group *g, uint64_t ticket);
/* A host loop in C, for measurements (bench.py end_to_end): nr_pushes buffers of buf_samples samples, taken in turn from the
 * caller's nr_bufs page-locked buffers, pushed with mfm_group_push_pinned(); blocks are fetched and released whenever the
 * output rings are full, everything is flushed and drained at the end.  *outputs_per_channel = outputs fetched. */
int mfm_group_replay_pinned(struct mfm_group *g, const void *const *bufs, size_t nr_bufs, size_t buf_samples, int format,
                            size_t nr_pushes, uint64_t *outputs_per_channel);
int mfm_group_copy_wait(struct mfm_group *g, uint64_t ticket);
/* oldest finished block of every shard into blks[0 .. nr_shards); MFM_E_DONE when nothing is pending */
int mfm_group_fetch(struct mfm_group *g, struct mfm_block *blks);
int mfm_group_release(struct mfm_group *g);
/* coalesce_samples: launch, on every shard, what has been pushed and not yet launched (MFM_E_BUSY: fetch / release first) */
int mfm_group_flush(struct mfm_group *g);
/* flush, then wait for every shard (MFM_E_BUSY from the flush is returned as it is: it is not a failure).  Producer-side
 * like the pushes: a host with a submit thread lets THAT thread flush and waits for mfm_stats::pending_samples == 0 and
 * pending_blocks == 0 instead (host/mfm_receiver.c receiver_drain). */
int mfm_group_sync(struct mfm_group *g);
int mfm_group_get_stats(struct mfm_group *g, uint32_t shard, struct mfm_stats *st);
/* whether blocks travel through RCCL, how many blocks were pushed through it and how many bytes it moved to
 * non-root devices */
int mfm_group_exchange_info(struct mfm_group *g, int *uses_rccl, uint64_t *blocks, uint64_t *bytes_exchanged);
/* One shard of the exchange, as measured: what a scaling figure needs to be read (is a step bound by the exchange of the block -
 * multifm/receiver.c:89-95's fan-out, here over xGMI - or by the shard's kernel?).  With MFM_F_TIMING the group brackets the
 * RCCL calls of one block in four with an event pair on every shard's exchange stream. */
struct mfm_exchange_detail {
    int32_t device;            /* HIP device of the shard */
    int32_t rccl_ranks;        /* ncclCommCount of the shard's communicator; 0: the group does not exchange; -1: the library has no such call */
    char pci_bus_id[32];       /* hipDeviceGetPCIBusId of the device */
    uint64_t timed_exchanges;  /* exchanges whose duration is in exchange_ms */
    double exchange_ms;        /* sum of their durations on this shard's exchange stream */
    uint64_t timed_launches;   /* the shard engine's mfm_stats::timed_launches ... */
    double kernel_ms;          /* ... and ::kernel_ms */
    uint32_t bound;            /* MFM_BOUND_KERNEL / MFM_BOUND_EXCHANGE: the larger of the two means; MFM_BOUND_UNKNOWN without both */
    uint32_t reserved0;
};
#define MFM_BOUND_UNKNOWN 0u
#define MFM_BOUND_KERNEL 1u
#define MFM_BOUND_EXCHANGE 2u
int mfm_group_exchange_detail(struct mfm_group *g, uint32_t shard, struct mfm_exchange_detail *out);
/* Which RCCL a device group of more than one GPU uses: loads it as mfm_group_commit() would - the file the environment variable
 * MFM_RCCL_LIBRARY names, if it is set (nothing else is tried then); else a librccl that is mapped into the
 * process already (PyTorch brings its own), else the loader's search for the bare name (LD_LIBRARY_PATH, the cache), then
 * $ROCM_PATH/lib/librccl.so and /opt/rocm/lib/librccl.so - and writes the file's path.  MFM_E_DEVICE when none can be loaded. */
int mfm_group_rccl_library(char *path, size_t cap);

/*
 * ---- PCM stage behind the FIFO -------------------------------------------
 * The decoder / resampler processes read a channel's PCM FIFO and run it through a real-valued rational
 * resampler and an optional DC blocker before the protocol decoders (decoder/decoder.c:580-673):
 *
 *   polyphase_fir_new(&fir, nr_coeffs, q14_coeffs, interpolate, decimate)   filter/polyphase_fir.c:47-105
 *   polyphase_fir_push_sample_buf / polyphase_fir_process                    filter/polyphase_fir.c:162-233
 *   dc_blocker_init(pole) / dc_blocker_apply                                 filter/dc_blocker.h:45-93
 *
 * mfm_resampler does that for ALL channels of an engine at once, on PCM that is still in HBM (the output
 * of mfm_engine_submit) or handed in from the host.  Same arithmetic, bit for bit: int16 x int16 -> wrapping
 * int32 dot product of one phase filter with consecutive samples, Q14 rounding, phase walk
 * phase += D; consumed = phase / I; phase %= I, an output only while MORE than one phase length of
 * unconsumed samples exists (polyphase_fir.c:184).
 */
struct mfm_resampler; /* opaque */

struct mfm_resampler_config {
    uint32_t abi_version;    /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t interpolate;    /* I */
    uint32_t decimate;       /* D */
    uint32_t max_in_samples; /* most PCM samples per channel one process call may carry */
    uint32_t invert;         /* decoder -i: negate the input samples (decoder.c:621-626) */
    uint32_t dc_block;       /* decoder -b */
    double dc_pole;          /* decoder -p, only with dc_block */
    uint32_t flags;          /* MFM_RS_* */
    uint32_t reserved;       /* 0 */
};

#define MFM_RS_FORCE_DOT2 1u /* the v_dot2 kernel even where the matrix-core form applies (A/B timing; same bits out) */

/* coeffs are the Q14 int16 taps (decoder.c:530-533 quantises lpfCoeffs with (int16_t)(c * 16384)) */
int mfm_resampler_create(struct mfm_resampler **pr, const struct mfm_resampler_config *cfg, const int16_t *coeffs,
                         size_t nr_coeffs);
void mfm_resampler_destroy(struct mfm_resampler **pr);
/* Upper bound of outputs per channel one process call can produce. */
size_t mfm_resampler_max_out(const struct mfm_resampler *r);
/*
 * Consume nr_in PCM samples per channel from device memory laid out [channel][in_stride] (for instance the
 * pointer/stride of mfm_engine_last_output_device) and produce *nr_out resampled samples per channel at
 * *d_out, laid out [channel][*out_stride], valid until the next call.  Work is queued on `stream` (a
 * hipStream_t, NULL = legacy default stream); no host synchronisation.
 */
int mfm_resampler_process_device(struct mfm_resampler *r, const int16_t *d_pcm, size_t in_stride, size_t nr_in,
                                 void *stream, int16_t **d_out, size_t *out_stride, size_t *nr_out);
/* Host in, device out: the PCM is staged to the device on `stream` (what a decoder-shaped host reading FIFOs
 * uses, so that only the input crosses PCIe); otherwise as mfm_resampler_process_device. */
int mfm_resampler_process_host_to_device(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                         void *stream, int16_t **d_out, size_t *out_stride, size_t *nr_out);
/* Host convenience (tests, harnesses): same, host in / host out, synchronous; out is [channel][out_stride]. */
int mfm_resampler_process_host(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                               int16_t *out, size_t out_stride, size_t *nr_out);

/*
 * Sign-bit form of the output.  The POCSAG and AIS stages look at one predicate of every resampled sample and at
 * nothing else (pager/pager_pocsag.c:91,476,516: sample < 0; ais/ais_demod.c:126,172: sample > 0), so a chain
 * that ends in one of them does not need the resampled PCM in memory: the calls below consume input exactly as
 * their PCM counterparts do (same phase walk, same carried tail, same `invert`), write NO PCM and leave one packed
 * bit per output, taken from the Q14-rounded sample in the kernel that computes it.  PCM calls and bits calls may
 * alternate on one resampler; the stream of outputs continues across them.  A resampler created with dc_block
 * answers them with MFM_E_INVAL (the DC blocker is a sequential filter over the resampled PCM in memory), as it does
 * an unknown polarity.
 */
#define MFM_BITS_NEG 1u /* bit = (sample < 0)  - POCSAG */
#define MFM_BITS_POS 2u /* bit = (sample > 0)  - AIS    */

struct mfm_bits_view {          /* valid until the resampler's next process call */
    const uint32_t *d_bits;     /* device memory, [channel][stride_words]; output j of THIS call is bit j % 32 of word j / 32 */
    size_t stride_words;
    size_t nr_bits;             /* outputs per channel of this call (what nr_out would have been); 0 is a valid result */
    uint32_t polarity;          /* MFM_BITS_NEG or MFM_BITS_POS */
    uint32_t reserved;          /* 0 */
};

/* Bits at positions >= nr_bits of a row's last word are 0; words behind it are not defined. */
int mfm_resampler_process_bits_device(struct mfm_resampler *r, const int16_t *d_pcm, size_t in_stride, size_t nr_in,
                                      void *stream, uint32_t polarity, struct mfm_bits_view *view);
/* Host in, device out (what the decoder programs use with -s). */
int mfm_resampler_process_bits_host_to_device(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                              void *stream, uint32_t polarity, struct mfm_bits_view *view);
/* Host convenience (tests): host in, bits out to host memory laid out [channel][bits_stride_words], synchronous. */
int mfm_resampler_process_bits_host(struct mfm_resampler *r, const int16_t *pcm, size_t in_stride, size_t nr_in,
                                    uint32_t polarity, uint32_t *bits, size_t bits_stride_words, size_t *nr_bits);

/*
 * Which kernel a resampler runs.  mfm_resampler_create() picks between two forms - the matrix-core kernel with 1 to 4 k-steps
 * and the v_dot2 kernel with a phase's coefficient pairs in registers (instances of 4, 8, ..., 32 pairs) or in LDS - from the
 * ratio, the number of taps, their range and the flags alone (the rules are at the head of csrc/mfm_resampler.hip); all of them
 * give the same bits.  The form is decided on the host, so it can be asked of a live object and of a configuration that has
 * none (mfm_hosttwin_resampler_form, no device needed).
 */
#define MFM_RS_FB_NONE 0u      /* the matrix form runs */
#define MFM_RS_FB_RATIO 1u     /* 16 D / I is not an integer */
#define MFM_RS_FB_WINDOW 2u    /* the window of a block of 16 outputs is longer than 256 bytes of padded rows */
#define MFM_RS_FB_BLOCK 3u     /* R = 16 D / I > 240 */
#define MFM_RS_FB_TAP_RANGE 4u /* a tap beyond +-32639 does not split into two signed bytes */
#define MFM_RS_FB_FORCED 5u    /* MFM_RS_FORCE_DOT2 */

struct mfm_resampler_form {
    uint32_t form;          /* 0 v_dot2, 1 matrix */
    uint32_t fallback;      /* MFM_RS_FB_*: why the matrix form was not taken */
    uint32_t reg_pairs;     /* v_dot2: the instance's coefficient pairs held in registers (4, 8, ..., 32), 0 = pairs in LDS; matrix: 0 */
    uint32_t k_steps;       /* matrix: k-steps of 64 window bytes (1 .. 4); v_dot2: 0 */
    uint32_t block_samples; /* matrix: R = 16 D / I, the samples a block of 16 outputs consumes; v_dot2: 0 */
    uint32_t row_bytes;     /* matrix: R rounded up to a multiple of 16, a row of the LDS image; v_dot2: 0 */
    uint32_t window_bytes;  /* matrix: bytes of padded rows the window of one block spans, a multiple of 64; v_dot2: 0 */
    uint32_t lds_bytes;     /* dynamic LDS of the kernel that will launch */
    uint32_t phase_len;     /* taps per phase, a multiple of 4 (filter/polyphase_fir.c:70-83) */
    uint32_t max_out;       /* = mfm_resampler_max_out() */
    int32_t dc_p;           /* the DC blocker's (1 - pole) in Q14 (filter/dc_blocker.h:56); 0 without dc_block */
    uint32_t reserved;      /* 0 */
};

int mfm_resampler_get_form(const struct mfm_resampler *r, struct mfm_resampler_form *form);

/*
 * ---- Pager stage: POCSAG slicer / sync / batch collection + BCH(31,21) -----
 * Replaces, for ALL channels at once and on PCM that is still in HBM (38 400 Hz, i.e. the resampler's output):
 *
 *   pager_pocsag_on_pcm            pager/pager_pocsag.c:434-543   state machine SEARCH -> SYNCHRONIZED ->
 *                                                                  BATCH_RECEIVE -> SEARCH_SYNCWORD
 *   _pager_pocsag_baud_on_sample   pager/pager_pocsag.c:81-117    three eye detectors (75 / 32 / 16 samples/bit)
 *   bch_code_decode                pager/bch_code.c:307-398       on the 16 words of every batch (:332-334)
 *
 * Output is an event list per channel (sync found, batch of 16 raw + corrected words with the BCH verdicts, sync
 * kept / lost) - everything _pager_pocsag_process_batch (:319-432) needs to assemble pages.  That last step is
 * a byte-serial walk over at most 16 words per batch and stays on the host (tsl-sdr_amd/host/mfm_pager_pocsag.c,
 * same callback signatures as pager/pager_pocsag.h:29-46).
 *
 * Conventions kept: bit = (sample < 0); sync = popcount(word ^ 0x7cd215d8) <= 4; eye open when more than
 * samples_per_bit/2 consecutive matches, sampling offset = matches/2; batch words filled LSB first; the word is
 * masked with 0x7fffffff before BCH; a word that fails BCH ends the batch for the message layer (nr_ok).
 */
#define MFM_POCSAG_EV_SYNC_FOUND 1u
#define MFM_POCSAG_EV_BATCH      2u
#define MFM_POCSAG_EV_SYNC_LOST  3u
#define MFM_POCSAG_EV_SYNC_KEPT  4u

struct mfm_pocsag_event {
    uint32_t type;          /* MFM_POCSAG_EV_* */
    uint32_t baud;          /* 512 / 1200 / 2400 */
    uint32_t channel;
    uint32_t aux;           /* SYNC_FOUND: eye matches; SYNC_LOST / SYNC_KEPT: the 32 bits seen in the sync slot */
    uint64_t sample;        /* index (per channel, since creation) of the PCM sample that completed the event */
    uint32_t nr_ok;         /* BATCH: words accepted before the first BCH failure (16 = whole batch) */
    uint32_t fail_mask;     /* BATCH: bit z set when word z is uncorrectable */
    uint32_t raw[16];       /* BATCH: words as collected */
    uint32_t corrected[16]; /* BATCH: (raw & 0x7fffffff) after BCH correction */
};

struct mfm_pocsag; /* opaque */

struct mfm_pocsag_config {
    uint32_t abi_version;    /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_in_samples; /* most PCM samples per channel one process call may carry */
    uint32_t max_events;     /* per channel and call; 0 = max_in_samples / 2048 + 16 (cannot overflow) */
    uint32_t flags;          /* 0 */
};

int mfm_pocsag_create(struct mfm_pocsag **pp, const struct mfm_pocsag_config *cfg);
void mfm_pocsag_destroy(struct mfm_pocsag **pp);
/*
 * Consume nr_in PCM samples per channel, laid out [channel][in_stride] in device memory (for instance the
 * output of mfm_resampler_process_device).  Work is queued on `stream`; no host synchronisation.  The events of
 * THIS call replace those of the previous one.
 */
int mfm_pocsag_process_device(struct mfm_pocsag *p, const int16_t *d_pcm, size_t in_stride, size_t nr_in,
                              void *stream);
/* Host convenience: same from host memory, synchronous. */
int mfm_pocsag_process_host(struct mfm_pocsag *p, const int16_t *pcm, size_t in_stride, size_t nr_in);
/* As mfm_pocsag_process_device with nr_in = view->nr_bits, from the resampler's sign bits (polarity MFM_BITS_NEG; any
 * other is MFM_E_INVAL) instead of PCM: the bits are spliced into the window in the place of the slicer.  PCM calls and
 * bits calls may alternate on one stage object. */
int mfm_pocsag_process_bits_device(struct mfm_pocsag *p, const struct mfm_bits_view *view, void *stream);
/*
 * Wait for the last process call and copy its events: channels ascending, stream order within a channel.
 * MFM_E_NOMEM when `max_events` is too small (nothing copied, *nr_events = needed), MFM_E_STATE when a channel
 * overflowed its device-side event list (only possible with a caller-chosen max_events).
 */
int mfm_pocsag_fetch_events(struct mfm_pocsag *p, struct mfm_pocsag_event *out, size_t max_events,
                            size_t *nr_events);
/*
 * Resume a stream at a position (the stage behind an engine that mfm_engine_seek() put there): afterwards the object is
 * what mfm_pocsag_create() with the same configuration returns, except that the next sample it consumes has index
 * samples_before.  Events are those of a fresh object for the same input with samples_before added to `sample`; the
 * detector reset lies at samples_before (the registers read zero-filled in front of it, as at sample 0).  Everything the
 * stream so far left is forgotten: walker state, bit window, the last call's events.  Waits for the object's queued work;
 * synchronous, not for the hot path.  MFM_E_INVAL with a message, the object unchanged: no object, or samples_before >=
 * 2^62 (the walk forms int64 differences of positions).  mfm_flex_seek, mfm_ais_seek, mfm_level_seek and mfm_gate_seek
 * below mean the same for their stages.
 */
int mfm_pocsag_seek(struct mfm_pocsag *p, uint64_t samples_before);

/*
 * ---- Pager stage: FLEX sync 1 / frame information word / sync 2 / block de-interleave -------
 * Replaces, for ALL channels at once and on PCM that is still in HBM (16 000 Hz, pager_flex_priv.h:231):
 *
 *   pager_flex_on_pcm              pager/pager_flex.c:1401-1455   SYNC_1 -> SYNC_2 -> BLOCK, sample skipping
 *   _pager_flex_sync_update        pager/pager_flex.c:295-458     ten-phase BS1 search, eye run, A / B / inverted A,
 *                                                                  frame information word, swing of the signal
 *   _pager_flex_handle_fiw         pager/pager_flex.c:1312-1345   BCH(31,21) + checksum of the FIW, cycle / frame
 *   _pager_flex_sync2_update       pager/pager_flex.c:460-525     counts the 25 ms of sync 2
 *   _pager_flex_block_update       pager/pager_flex.c:1224-1310   2- / 4-level slicer, phase split, block de-interleave
 *
 * Output per channel: an event list (frame collected / unknown A code / bad FIW) and, for every frame, the 88 words
 * of each phase exactly as _pager_flex_phase_append_bit (:1200-1222) leaves them.  What follows in the reference,
 * _pager_flex_phase_process (:1088-1198: BIW, addresses, vectors, message bodies), is a serial walk over at most
 * 88 words with in-place corrections; it stays on the host (tsl-sdr_amd/host/mfm_pager_flex.c, same callback
 * signatures as pager/pager_flex.h:16-87).
 *
 * Conventions kept: bit = (sample >= 0); BS1 = 0xaaaaaaaa seen by one of ten registers that take every tenth
 * sample; a run of three or more consecutive matching samples opens the eye and the sampling clock is set to half
 * the run length (the run counter is 8 bits wide, as in the reference); only the upper half of A is compared, with
 * fewer than 4 differing bits (the inverted-A comparison of :278 can never succeed and is not evaluated); swing =
 * mean of the positive minus mean of the non-positive samples over the 112 sync bits, all in int16 arithmetic;
 * registers are zero-filled after every reset, so no match is possible for the next 310 samples.
 * A sync run without a positive or without a non-positive sample (the reference divides by zero) is reported as
 * MFM_FLEX_EV_BAD_FIW with fiw_rc 3.
 */
#define MFM_FLEX_EV_FRAME    1u
#define MFM_FLEX_EV_BAD_BAUD 2u
#define MFM_FLEX_EV_BAD_FIW  3u
#define MFM_FLEX_PHASE_WORDS 88u /* pager_flex_priv.h:175 */

struct mfm_flex_event {
    uint32_t type;          /* MFM_FLEX_EV_* */
    uint32_t channel;
    uint64_t sample;        /* index (per channel, since creation) of the PCM sample that completed the event */
    uint64_t sync_sample;   /* FRAME: sample of the last FIW bit */
    uint32_t coding;        /* index into _pager_codings[] (pager_flex.c:46-96); 0xffffffff for BAD_BAUD */
    uint32_t baud;          /* 1600 / 3200 / 6400; 0 for BAD_BAUD */
    uint32_t eye;           /* length of the BS1 run (sync->bit_counter at :339) */
    uint32_t a, b, inv_a;   /* the sync words as collected */
    uint32_t fiw_raw;       /* the 32 FIW bits as collected */
    uint32_t fiw;           /* (fiw_raw & 0x7fffffff) after BCH correction */
    uint32_t fiw_rc;        /* 0 accepted, 1 uncorrectable, 2 checksum, 3 no swing */
    int32_t sample_range;   /* flex->sample_range / sample_delta (:441-442) */
    int32_t sample_delta;
    uint32_t cycle, frame;  /* FIW fields (:1337-1338) */
    uint32_t frame_index;   /* FRAME: index of this frame's words in the array the same fetch call fills */
    uint32_t nr_phases;     /* 1 / 2 / 4 */
    uint32_t reserved;
};

/* phase_words[] of phases A..D of one frame; phases the coding does not carry are zero */
struct mfm_flex_frame_words {
    uint32_t words[4][MFM_FLEX_PHASE_WORDS];
};

struct mfm_flex; /* opaque */

struct mfm_flex_config {
    uint32_t abi_version;    /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_in_samples; /* most PCM samples per channel one process call may carry (<= 2^26) */
    uint32_t max_events;     /* per channel and call; 0 = max_in_samples / 1024 + 8 (cannot overflow) */
    uint32_t flags;          /* 0 */
};

int mfm_flex_create(struct mfm_flex **pf, const struct mfm_flex_config *cfg);
void mfm_flex_destroy(struct mfm_flex **pf);
/*
 * Consume nr_in PCM samples per channel, laid out [channel][in_stride] in device memory (for instance the output of
 * mfm_resampler_process_device).  Work is queued on `stream`; no host synchronisation; d_pcm is read until the
 * queued work has run.  The events of THIS call replace those of the previous one.
 */
int mfm_flex_process_device(struct mfm_flex *f, const int16_t *d_pcm, size_t in_stride, size_t nr_in, void *stream);
/* Host convenience: same from host memory, synchronous. */
int mfm_flex_process_host(struct mfm_flex *f, const int16_t *pcm, size_t in_stride, size_t nr_in);
/*
 * Wait for the last process call and copy its events (channels ascending, stream order within a channel) and the
 * words of its frames.  MFM_E_NOMEM when either array is too small (nothing copied, *nr_events / *nr_frames =
 * needed), MFM_E_STATE when a channel overflowed its device-side lists (only with a caller-chosen max_events).
 */
int mfm_flex_fetch_events(struct mfm_flex *f, struct mfm_flex_event *events, size_t max_events, size_t *nr_events,
                          struct mfm_flex_frame_words *frames, size_t max_frames, size_t *nr_frames);
/* As mfm_pocsag_seek: samples_before is added to `sample` and, in FRAME events, to `sync_sample` (0 in the others at any
 * position); the history ring is emptied and the BS1 registers read zero-filled in front of samples_before, so the search
 * opens at samples_before + 310. */
int mfm_flex_seek(struct mfm_flex *f, uint64_t samples_before);

/*
 * ---- AIS stage: slicer / preamble detector / NRZI + HDLC bit recovery / FCS check ------------------------------
 * Replaces, for ALL channels at once and on PCM that is still in HBM (48 000 Hz, i.e. the resampler's output):
 *
 *   ais_demod_on_pcm                  ais/ais_demod.c:215-258   state machine SEARCH_SYNC -> RECEIVING
 *   _ais_demod_detect_handle_sample   ais/ais_demod.c:114-158   five preamble registers, 3 of 5 within 2 bits
 *   _ais_demod_packet_rx_sample       ais/ais_demod.c:160-213   NRZI, unstuffing, end flag / 1280-bit cut
 *   _ais_crc16                        ais/ais_demod.c:19-36     CRC-16, reflected 0x8408, init 0xffff, inverted
 *
 * Output is one event per candidate packet, i.e. per packet end with current_bit / 8 >= 4 (:190-191), whether its
 * FCS holds or not.  Decoding the message (ais/ais_decode.c) stays on the host (tsl-sdr_amd/host/mfm_ais.c).
 *
 * Conventions kept: bit = (sample > 0); detector bit = !(b[s] ^ b[s-5]); the first packet bit is read four samples
 * after the matching sample, then one every five; packet bits LSB first into bytes; the FCS is the little-endian
 * pair after nr_bytes - 2 bytes of data.
 */
struct mfm_ais_event {
    uint32_t channel;
    uint32_t fcs_valid;     /* 1: the CRC over bytes[0 .. nr_bytes - 2) equals bytes[nr_bytes - 2] | bytes[nr_bytes - 1] << 8 */
    uint32_t nr_bytes;      /* current_bit / 8 at the packet end, the two FCS bytes included (4 .. 160) */
    uint32_t reserved;      /* 0 */
    uint64_t sample;        /* index (per channel, since creation) of the PCM sample that ended the packet */
    uint64_t start_sample;  /* index of the sample where the preamble matched */
    uint8_t bytes[160];     /* the packet buffer as the reference holds it (a partial last byte included, zeros after) */
};

struct mfm_ais; /* opaque */

struct mfm_ais_config {
    uint32_t abi_version;    /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_in_samples; /* most PCM samples per channel one process call may carry */
    uint32_t max_events;     /* per channel and call; 0 = max_in_samples / 160 + 16 (cannot overflow) */
    uint32_t flags;          /* 0 */
};

int mfm_ais_create(struct mfm_ais **pp, const struct mfm_ais_config *cfg);
void mfm_ais_destroy(struct mfm_ais **pp);
/*
 * Consume nr_in PCM samples per channel, laid out [channel][in_stride] in device memory (for instance the
 * output of mfm_resampler_process_device).  Work is queued on `stream`; no host synchronisation.  The events of
 * THIS call replace those of the previous one.  A packet that is still being received at the end of a call is
 * carried over on the device: events do not depend on how a stream is cut into calls.
 */
int mfm_ais_process_device(struct mfm_ais *p, const int16_t *d_pcm, size_t in_stride, size_t nr_in, void *stream);
/* Host convenience: same from host memory, synchronous. */
int mfm_ais_process_host(struct mfm_ais *p, const int16_t *pcm, size_t in_stride, size_t nr_in);
/* As mfm_ais_process_device with nr_in = view->nr_bits, from the resampler's sign bits (polarity MFM_BITS_POS; any
 * other is MFM_E_INVAL) instead of PCM.  PCM calls and bits calls may alternate on one stage object. */
int mfm_ais_process_bits_device(struct mfm_ais *p, const struct mfm_bits_view *view, void *stream);
/*
 * Wait for the last process call and copy its events: channels ascending, stream order within a channel.
 * MFM_E_NOMEM when `max_events` is too small (nothing copied, *nr_events = needed), MFM_E_STATE when a channel
 * overflowed its device-side event list (only possible with a caller-chosen max_events).
 */
int mfm_ais_fetch_events(struct mfm_ais *p, struct mfm_ais_event *out, size_t max_events, size_t *nr_events);
/* As mfm_pocsag_seek: samples_before is added to `sample` and `start_sample`; a packet that was being received is dropped. */
int mfm_ais_seek(struct mfm_ais *p, uint64_t samples_before);

/*
 * ---- Level stage: per-channel signal level and squelch -----------------------------------------------------------
 * The reference has no counterpart: every channel thread demodulates all the time (multifm/demod.c:48-121) and an empty
 * channel's discriminator noise runs through every decoder behind it.  This stage answers "which channels carry a signal
 * right now" for ALL channels at once, on rows that are still in HBM, in one of two forms chosen at create:
 *
 *   MFM_LEVEL_PCM   one int16 per sample: the engine's PCM or the resampler's output, rows [channel][in_stride]
 *   MFM_LEVEL_IQ    two per sample, re, im interleaved: the engine's filtered IQ.  in_stride counts int16 ELEMENTS
 *                   here as well, so for the engine's IQ rows it is 2 * stride
 *
 * Samples are numbered per channel from 0 at create; window k covers samples [k W, (k + 1) W), W = window_samples.  A
 * window that straddles calls is carried on the device, and a call completes floor((pos + nr_in) / W) - floor(pos / W)
 * windows, the same number for every channel: records do not depend on how a stream is cut into calls (nr_in = 0 and
 * nr_in < W included).  All arithmetic is integer and exact.  Per channel and completed window one record:
 *
 *   energy       sum of x * x (PCM) or of re * re + im * im (IQ); -32768 squares to 2^30, nothing wraps
 *   diff_energy  PCM form only, else 0: sum of d * d, d = (int16_t)(x[n] - x[n-1]) - the difference WRAPPED to 16 bits,
 *                because the discriminator's output is an angle; x[-1] = 0 at stream start, the previous sample is
 *                carried across windows and calls
 *   peak         largest |x|, over both components in the IQ form; |-32768| = 32768
 *   open         squelch state after this window
 *
 * Squelch, per channel, stepped once per completed window in stream order on `metric` (the window's energy or
 * diff_energy, compared with the thresholds as it is, no division).  It starts closed.  Closed: opens when the metric is
 * on the open side of open_thr (>= for MFM_LEVEL_OPEN_ABOVE: a carrier raises the IQ energy; <= for
 * MFM_LEVEL_OPEN_BELOW: a captured FM carrier lowers the discriminator's energy).  Open: a window is bad when the metric
 * is strictly on the closed side of close_thr; hang_windows + 1 bad windows in a row close, a good one resets the count.
 * The current state of every channel also stands in device memory as one uint32 per channel (d_open of
 * mfm_level_device_view()): a channel mask for stages that can skip idle channels.
 */
#define MFM_LEVEL_PCM 0u
#define MFM_LEVEL_IQ 1u
#define MFM_LEVEL_METRIC_ENERGY 0u
#define MFM_LEVEL_METRIC_DIFF 1u   /* PCM form only */
#define MFM_LEVEL_OPEN_ABOVE 0u
#define MFM_LEVEL_OPEN_BELOW 1u

struct mfm_level_record {   /* 40 bytes */
    uint64_t energy;
    uint64_t diff_energy;
    uint64_t window;        /* k */
    uint32_t peak;
    uint32_t channel;
    uint32_t open;          /* 0 / 1 */
    uint32_t reserved;      /* 0 */
};

struct mfm_level; /* opaque */

struct mfm_level_config {
    uint32_t abi_version;    /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_in_samples; /* most samples per channel one process call may carry (<= 2^28) */
    uint32_t form;           /* MFM_LEVEL_PCM / MFM_LEVEL_IQ */
    uint32_t window_samples; /* W >= 1 */
    uint32_t metric;         /* MFM_LEVEL_METRIC_* */
    uint32_t sense;          /* MFM_LEVEL_OPEN_* */
    uint64_t open_thr;
    uint64_t close_thr;      /* MFM_E_INVAL unless close_thr <= open_thr (OPEN_ABOVE) / close_thr >= open_thr (OPEN_BELOW) */
    uint32_t hang_windows;
    uint32_t flags;          /* 0 */
};

int mfm_level_create(struct mfm_level **pp, const struct mfm_level_config *cfg);
void mfm_level_destroy(struct mfm_level **pp);
/*
 * Consume nr_in samples per channel from device memory laid out [channel][in_stride] (int16 elements; for instance
 * the pointers and stride of mfm_engine_last_output_device(), or the resampler's output).  Work is queued on `stream`;
 * no host synchronisation; the rows are read until the queued work has run.  The records of THIS call replace those of
 * the previous one.
 */
int mfm_level_process_device(struct mfm_level *p, const int16_t *d_rows, size_t in_stride, size_t nr_in, void *stream);
/* Host convenience: same from host memory, synchronous. */
int mfm_level_process_host(struct mfm_level *p, const int16_t *rows, size_t in_stride, size_t nr_in);
/*
 * Wait for the last process call and copy its records: channels ascending, windows ascending within a channel,
 * nr_channels * *nr_windows of them (*nr_windows = windows per channel that call completed; 0 is a valid result).
 * MFM_E_NOMEM when max_records is smaller than that (nothing copied; *nr_windows says what is needed).
 */
int mfm_level_fetch(struct mfm_level *p, struct mfm_level_record *out, size_t max_records, size_t *nr_windows);
/* For callers that stay on the device: the last call's records at d_records[channel * record_stride + i],
 * i < *nr_windows, and the squelch state d_open[channel]; both are written by work queued on that call's stream and
 * stay valid (d_open: current) until the next call.  Any of the four may be NULL. */
int mfm_level_device_view(struct mfm_level *p, const struct mfm_level_record **d_records, size_t *record_stride, size_t *nr_windows,
                          const uint32_t **d_open);
/* As mfm_pocsag_seek: samples_before / W is added to `window`; the sums of an unfinished window, x[-1] and the squelch
 * (closed again, d_open included) are forgotten, and the last call's records.  Also MFM_E_INVAL when samples_before is not a
 * multiple of window_samples: no fresh stage stands inside a window. */
int mfm_level_seek(struct mfm_level *p, uint64_t samples_before);

/*
 * The adaptive squelch: open_thr / close_thr of the config are two numbers for every channel, but across the channels of one
 * wide-band capture the idle level differs (filter roll-off, gain slope, neighbours) and on a live stream it drifts.  With this
 * setting every channel's squelch follows the channel's own noise floor, scanner-style.  Per channel, over completed windows in
 * stream order, k_s the first window after create or the last mfm_level_seek, metric[k] the window's energy or diff_energy as
 * the config's `metric` says:
 *
 *   floor[k]   the extremum of metric[j] for j in [max(k_s, k - M + 1), k], window k included, M = floor_windows: the MINIMUM for
 *              MFM_LEVEL_OPEN_ABOVE (the idle level is the low side), the MAXIMUM for MFM_LEVEL_OPEN_BELOW.  It does not depend on
 *              the squelch state.  A transmission longer than M windows drags the floor along and the squelch closes.
 *   open side  ABOVE: metric * 256 >= floor * open_q8 and metric >= open_thr;  BELOW: metric * 256 <= floor * open_q8 and
 *              metric <= open_thr.  False for the first warmup_windows windows after k_s.
 *   bad        ABOVE: metric * 256 < floor * close_q8 or metric < close_thr;  BELOW: metric * 256 > floor * close_q8 or
 *              metric > close_thr.
 *
 * The products are exact (no wrap).  The state machine is the one above, fed these two predicates: it starts closed, opens on an
 * open-side window, hang_windows + 1 bad windows in a row close it, a window that is not bad resets the count.  The config's
 * thresholds stay in force as absolute limits: a silent channel has floor 0, where every metric passes the ratio test, and a
 * non-zero open_thr keeps it shut.  No limit is open_thr = close_thr = 0 (ABOVE) or UINT64_MAX (BELOW).  Like everything in this
 * stage the result does not depend on how the stream is cut into calls.  Records, d_open and mfm_level_device_view are what they
 * were: the gate and everything behind it take the adaptive verdict as it is.
 */
struct mfm_level_adaptive {      /* 24 bytes */
    uint32_t floor_windows;      /* M, 1 .. 1024 */
    uint32_t open_q8;            /* 1 .. 65536: ratio to the floor in 1/256 */
    uint32_t close_q8;           /* 1 .. 65536; <= open_q8 for OPEN_ABOVE, >= open_q8 for OPEN_BELOW */
    uint32_t warmup_windows;
    uint32_t flags, reserved;    /* 0 */
};
/* Switch the adaptive squelch on (a) or off (NULL).  Only on a fresh object - after create or mfm_level_seek, before the next
 * process call - else MFM_E_INVAL; MFM_E_INVAL with a mfm_last_error() message and the object unchanged for values out of range,
 * ratios in the wrong order or non-zero flags / reserved.  mfm_level_seek keeps the setting and forgets the history of the floor
 * and the warm-up count. */
int mfm_level_set_adaptive(struct mfm_level *p, const struct mfm_level_adaptive *a);
/* *on = 1 and *a = the setting, or *on = 0 and *a zeroed; either may be NULL */
int mfm_level_get_adaptive(struct mfm_level *p, uint32_t *on, struct mfm_level_adaptive *a);
/* The floors of the last call's windows, as mfm_level_fetch copies its records: nr_channels * *nr_windows values, channels
 * ascending; MFM_E_NOMEM when max_values is smaller (nothing copied), 0 windows is a valid result.  mfm_level_floor_view is the
 * device form, d_floor[channel * floor_stride + i], valid like mfm_level_device_view's records.  MFM_E_INVAL with the adaptive
 * squelch off. */
int mfm_level_fetch_floor(struct mfm_level *p, uint64_t *out, size_t max_values, size_t *nr_windows);
int mfm_level_floor_view(struct mfm_level *p, const uint64_t **d_floor, size_t *floor_stride);

/*
 * ---- Gate stage: only open windows of a channel leave the GPU -------------------------------------------------------
 * The consumer of the level stage's verdict: of rows that are still in HBM it packs the windows whose record says
 * `open` into one dense payload, with a run list that says which channel and which samples each piece is.  One short
 * device-to-host copy (mfm_gate_fetch) or a consumer on the device (mfm_gate_device_view) then carries what is worth
 * carrying.  The reference has no counterpart.
 *
 * Samples are numbered per channel from 0 at create and window k is [k W, (k + 1) W): the level stage's numbers.  A call
 * with nr_in samples completes floor((pos + nr_in) / W) - floor(pos / W) windows, so the gate is fed the same nr_in
 * sequence as the level object whose records it reads; the rows may be others than those the level was measured on
 * (squelch on the IQ energy, gate the PCM) as long as the numbering matches.  The samples of an unfinished window are
 * carried on the device, at most W - 1 per channel: output does not depend on how a stream is cut into calls (nr_in = 0
 * and several calls in a row shorter than W included).  Create refuses W * elems_per_sample above 2^20 (the carry is
 * one window of int16 per channel, kept twice: it is the history below with P = 0) with MFM_E_INVAL and a message.
 *
 * Window k of channel c goes out exactly when the record of (c, k) has open != 0: the opening window is among them (the
 * squelch is stepped after it), the tail is what hang_windows gives; no closed window in front of an opening is emitted.
 * The payload is dense: channels ascending, windows ascending within a channel, each W * elems_per_sample int16, so
 * consecutive open windows of one channel are contiguous.  Each maximal stretch of consecutive open windows WITHIN ONE
 * CALL is one mfm_gate_run; a stretch that goes on into the next call begins a new run there (first_window of the one
 * follows the last window of the other).  Runs stand in payload order.  Order and offsets are deterministic.
 *
 * Pre-roll (mfm_gate_set_preroll; off by default, and with it off everything above holds to the byte).  The squelch is
 * stepped on a whole window, so a burst that begins late in window k opens only window k + 1 and the rule above drops the
 * burst's first samples.  With P = preroll_windows (0 .. MFM_GATE_MAX_PREROLL) window k of channel c goes out exactly
 * when any record (c, j) with k <= j <= k + P has open != 0.  That cannot be known before record k + P exists, so the
 * gate's output is DELAYED BY P WINDOWS: a process call that brings the total of completed windows from K0 to K1 emits
 * those of the windows max(K0 - P, 0) .. K1 - P - 1 that satisfy the rule (the first P completed windows of a stream emit
 * nothing), from a history of the last P windows and the unfinished one that the gate keeps per channel on the device:
 * (P + 1) * W * elems_per_sample int16 per channel, twice (two buffers used in turn).  nr_windows keeps its meaning (what
 * this call completes: the records handed over are those of windows K0 .. K1 - 1).  Runs, payload order, first_window
 * (the true k), payload_offset, "a stretch that goes on into the next call begins a new run there", overflow and
 * out-of-step are as above, over the range of windows the call emits; output does not depend on how the stream is cut
 * into calls.  mfm_gate_flush_device ends the stream: it emits, by the same rule with every missing future record taken
 * as closed, the up to P completed windows not yet decided, as a normal call result; the unfinished window is dropped.
 */
#define MFM_GATE_MAX_PREROLL 63u
#define MFM_GATE_MAX_HISTORY_BYTES (1ull << 30) /* one history buffer: nr_channels * (P + 1) * W * elems_per_sample * 2 at most */

struct mfm_gate_run {           /* 24 bytes */
    uint64_t first_window;      /* k of the run's first window; its first sample is k * W */
    uint64_t payload_offset;    /* in int16 elements, a multiple of W * elems_per_sample */
    uint32_t channel;
    uint32_t nr_windows;
};

struct mfm_gate; /* opaque */

struct mfm_gate_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;       /* 1 .. 65535 */
    uint32_t max_in_samples;    /* most samples per channel one process call may carry (<= 2^28) */
    uint32_t window_samples;    /* W, the level stage's W */
    uint32_t elems_per_sample;  /* 1: PCM rows, 2: filtered-IQ rows (re, im interleaved) */
    uint32_t max_open_windows;  /* payload capacity per call over all channels, in windows;
                                   0 = nr_channels * (max_in_samples / W + 1), which cannot overflow */
    uint32_t flags;             /* 0 */
};

int mfm_gate_create(struct mfm_gate **pg, const struct mfm_gate_config *cfg);
void mfm_gate_destroy(struct mfm_gate **pg);
/*
 * Consume nr_in samples per channel from device memory laid out [channel][in_stride] (in_stride in int16 ELEMENTS, as in
 * the level stage; any 2-byte alignment of rows and stride).  d_records, record_stride and nr_windows are what
 * mfm_level_device_view() returns for the level call on the same block; only .open and .window are read.  nr_windows
 * other than what this call completes is MFM_E_INVAL (nothing is queued, the position stays).  Work is queued on
 * `stream`; no host synchronisation; rows and records are read until the queued work has run.  Runs and payload of THIS
 * call replace those of the previous one.  A record whose .window is not the k the gate expects raises a flag on the
 * device that mfm_gate_fetch reports.
 */
int mfm_gate_process_device(struct mfm_gate *g, const int16_t *d_rows, size_t in_stride, size_t nr_in, const struct mfm_level_record *d_records,
                            size_t record_stride, size_t nr_windows, void *stream);
/* Host convenience: the same from host memory (rows [channel][in_stride], records [channel][record_stride]), synchronous. */
int mfm_gate_process_host(struct mfm_gate *g, const int16_t *rows, size_t in_stride, size_t nr_in, const struct mfm_level_record *records,
                          size_t record_stride, size_t nr_windows);
/*
 * Wait for the last process call, read its two totals into *nr_runs and *nr_elems and copy the used part of both arrays.
 * MFM_E_NOMEM when max_runs or max_elems is too small (nothing copied, the totals say what is needed); MFM_E_STATE when
 * the call's open windows exceeded a caller-chosen max_open_windows (nothing copied, nothing was written past the
 * capacity; the stream position and the carry moved on, so a following call that fits is right again) or when level and
 * gate were out of step.
 */
int mfm_gate_fetch(struct mfm_gate *g, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                   size_t *nr_elems);
/* For consumers that stay on the device: the last call's runs, payload and d_totals[4] = { runs, payload elements,
 * overflow (0 / 1), out of step (0 / 1) }, written by work queued on that call's stream and valid until the next call.
 * Any of the three may be NULL. */
int mfm_gate_device_view(struct mfm_gate *g, const struct mfm_gate_run **d_runs, const int16_t **d_payload, const uint64_t **d_totals);
/*
 * Pre-roll of P = preroll_windows windows (see above).  Valid only before the first process call: MFM_E_STATE afterwards.
 * MFM_E_INVAL with a message that names the bound when P exceeds MFM_GATE_MAX_PREROLL or one history buffer,
 * nr_channels * (P + 1) * W * elems_per_sample int16 (each channel's part rounded up to 16 bytes), would exceed
 * MFM_GATE_MAX_HISTORY_BYTES.  Allocates the history, and where the default capacity (max_open_windows == 0) would not
 * hold a flush of P windows per channel regrows payload and runs to nr_channels * P windows.  P = 0 is the plain gate.
 */
int mfm_gate_set_preroll(struct mfm_gate *g, uint32_t preroll_windows);
/*
 * End of the stream.  Queues on `stream`, without host synchronisation, the emission of the up to P completed windows
 * not yet decided (every missing future record taken as closed); the result is read like a process call's, with
 * mfm_gate_fetch (which waits for it: there is no separate synchronous flush) or mfm_gate_device_view.  With P = 0 that
 * result is empty.  Afterwards mfm_gate_process_* and a second flush return MFM_E_STATE.
 */
int mfm_gate_flush_device(struct mfm_gate *g, void *stream);
/* As mfm_pocsag_seek: samples_before / W is added to `first_window`.  The gate keeps its preroll_windows; history and open
 * bits are emptied, a flush is undone, and the windows in front of samples_before do not exist (pre-roll emits none of
 * them, as it emits none in front of window 0).  Also MFM_E_INVAL when samples_before is not a multiple of window_samples.
 * A gate that was put elsewhere than the level stage it reads raises out-of-step on fetch, as any wrong `.window` does. */
int mfm_gate_seek(struct mfm_gate *g, uint64_t samples_before);

/*
 * ---- Burst resampler: the gate's runs through the rational resampler, on the device ----------------------------------
 * The first stage that takes the gate's output rather than full rows: its input is what mfm_gate_device_view returns (the
 * run list, the dense payload, the totals) and its work is proportional to what the squelch left open.  The arithmetic is
 * the resampler's above (filter/polyphase_fir.c:162-233), bit for bit: int16 x int16 -> wrapping int32 sum over one phase,
 * Q14 rounding (a >> 14) + ((a >> 13) & 1) cut to int16, phase walk phase += D; pos += phase / I; phase %= I, an output
 * only while strictly MORE than plen unconsumed samples exist; `invert` negates the input on int16 storage.
 *
 * Stretch.  A stretch of channel c is a maximal sequence of consecutive window numbers k that the gate emitted for c over
 * the whole stream; it does not depend on how the stream was cut into calls.  The gate begins a new mfm_gate_run at every
 * call boundary, so a stretch is one or more runs whose first_window values follow on.
 *
 * Rule.  The outputs of a stretch are the concatenation of the outputs of its runs, and they are exactly what a fresh
 * resampler (phase 0, nothing pending) returns when fed the stretch's samples.  The at most plen samples pending at the
 * end of a stretch produce nothing, as at the end of a stream in the reference; a stretch shorter than plen + 1 samples
 * produces no output, and its runs still appear, with nr_out = 0.
 *
 * State.  Per channel, on the device: the window number expected next, the phase, the outputs so far, the pending count
 * and plen pending samples; with the DC blocker on, the blocker's x_(n-1), y_(n-1) and acc as well.  A run continues its
 * channel's stretch exactly when its first_window equals the expected number; otherwise it resets the state and begins a new
 * stretch.  Within one call only a channel's first run can continue (the gate's runs within a call are maximal).  A channel
 * without a run in a call keeps its state.
 *
 * DC blocker (decoder -b, decoder/decoder.c:580-673: resample, then dc_blocker_apply).  Off at create; switched on with
 * mfm_runrs_set_dc_block before the first call.  With it on, the outputs of a stretch are exactly what
 * filter/dc_blocker.h:72-93 returns on a fresh struct dc_blocker - dc_blocker_init(pole): p = (int16)((1 - pole) * 16384),
 * x_n_1 = y_n_1 = acc = 0 - applied to the stretch's resampled PCM in stretch order, that PCM being the concatenation of the
 * outputs of the stretch's runs.  The arithmetic is the reference's int32 arithmetic, wrapping, with the truncating shift;
 * the carried y_(n-1) is the unclipped value, the stored sample its low 16 bits.  The result does not depend on how the
 * stream was cut into calls, and everything else in a call's result (run list, out_offset, first_out, nr_out, flags, totals,
 * refusals) is as without the blocker.  A run with nr_out == 0 changes nothing: it still begins a stretch with zero state,
 * or continues one and leaves the state as it was.
 *
 * Result.  It replaces the previous call's: one mfm_runrs_run per input run, in the gate's order; a dense int16 payload in
 * that order (out_offset ascending, no gaps); d_totals[4] = { runs, output elements, overflow, gate error }.  Order and
 * offsets are deterministic.  When the gate's totals carry overflow or out-of-step, or the call does not fit max_windows /
 * max_runs, the call produces nothing (output elements = 0), raises the flag and leaves the per-channel state untouched:
 *   overflow    MFM_RUNRS_OVER_OWN: more runs or payload than max_runs / max_windows; MFM_RUNRS_OVER_GATE: the gate's
 *   gate error  MFM_RUNRS_GATE_OUT_OF_STEP: the gate's; MFM_RUNRS_GATE_BAD_RUNS: a run names a channel or payload range that
 *               does not exist (not a gate's run list)
 *
 * Refusals at create (MFM_E_INVAL with a message, never a fallback): the stage takes PCM payloads only (a gate with
 * elems_per_sample == 1); its DC blocker (mfm_runrs_set_dc_block) and its sign-bit output (below) are entries of their own,
 * so `flags` must be 0; a ratio whose walk steps past a phase (mfm_rs_plan.h's rule, as mfm_resampler_create); a coefficient
 * image I * plen int16 that, with the input window of one workgroup, exceeds MFM_RUNRS_MAX_LDS_BYTES.
 */
#define MFM_RUNRS_MAX_LDS_BYTES 49152u /* coefficient image + one workgroup's input window */
#define MFM_RUNRS_BEGINS 1u            /* mfm_runrs_run.flags bit 0: the run begins a stretch */
#define MFM_RUNRS_OVER_OWN 1u
#define MFM_RUNRS_OVER_GATE 2u
#define MFM_RUNRS_GATE_OUT_OF_STEP 1u
#define MFM_RUNRS_GATE_BAD_RUNS 2u

struct mfm_runrs_run {          /* 40 bytes */
    uint64_t first_window;      /* the gate run's */
    uint64_t out_offset;        /* in int16 elements of the output payload */
    uint64_t first_out;         /* index of the run's first output within its stretch */
    uint32_t channel;
    uint32_t nr_out;
    uint32_t flags;             /* MFM_RUNRS_BEGINS */
    uint32_t reserved;          /* 0 */
};

struct mfm_runrs; /* opaque */

struct mfm_runrs_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;       /* 1 .. 65535 */
    uint32_t interpolate;       /* I */
    uint32_t decimate;          /* D */
    uint32_t window_samples;    /* W, the gate's */
    uint32_t max_windows;       /* the gate's payload capacity per call, in windows (its max_open_windows); 0 = the gate's own
                                   default, nr_channels * max(max_in_samples / W + 1, preroll_windows), which cannot overflow */
    uint32_t max_runs;          /* 0 = a bound that cannot overflow: two runs of a channel have a closed window between them */
    uint32_t invert;            /* decoder -i */
    uint32_t flags;             /* 0 */
    uint32_t max_in_samples;    /* the gate's; read only where max_windows or max_runs is 0 */
    uint32_t preroll_windows;   /* the gate's P (its flush emits up to P windows per channel); likewise */
};

/* coeffs are the Q14 int16 taps, as in mfm_resampler_create */
int mfm_runrs_create(struct mfm_runrs **prr, const struct mfm_runrs_config *cfg, const int16_t *coeffs, size_t nr_coeffs);
void mfm_runrs_destroy(struct mfm_runrs **prr);
/*
 * Resample the runs of one gate call: d_runs, d_payload and d_totals are what mfm_gate_device_view returned after
 * mfm_gate_process_device or mfm_gate_flush_device.  Work is queued on `stream` (the gate call's, or one ordered behind it);
 * no host synchronisation: run count and payload length are read on the device, launches are sized from the capacities
 * fixed at create.  The three arrays are read until the queued work has run.
 */
int mfm_runrs_process_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                             void *stream);
/*
 * Wait for the last call, read its totals into *nr_runs and *nr_elems and copy the used part of both arrays.  MFM_E_NOMEM
 * when max_runs or max_elems is too small (nothing copied, the totals say what is needed); MFM_E_STATE with a message when
 * the call raised overflow or gate error (nothing copied, nothing was written past the capacity, the state did not move:
 * the same input in calls that fit is right again).
 */
int mfm_runrs_fetch(struct mfm_runrs *rr, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                    size_t *nr_elems);
/* For consumers that stay on the device: the last call's runs, payload and d_totals[4], written by work queued on that
 * call's stream and valid until the next call.  Any of the three may be NULL. */
int mfm_runrs_device_view(struct mfm_runrs *rr, const struct mfm_runrs_run **d_runs, const int16_t **d_payload, const uint64_t **d_totals);
/* The capacities fixed at create, which a stage behind sizes itself from: the most runs and the most output elements one call
 * can produce (max_runs as given or its default; ((max_windows * W + max_runs * plen) * I) / D + max_runs). */
int mfm_runrs_get_capacity(struct mfm_runrs *rr, uint32_t *max_runs, uint64_t *max_out_elems);
/*
 * The DC blocker of the rule above, one fresh blocker per stretch.  Valid only before the first process call (MFM_E_STATE
 * with a message afterwards).  on == 0 switches it off (the pole is not read): the object then queues the launches and
 * returns the bits of one never touched.  Otherwise the pole is converted as mfm_resampler_create converts dc_pole,
 * p = (int16)((1 - pole) * 16384); a pole for which that is not defined (not a number, or a product outside int16) is
 * MFM_E_INVAL with a message.  With the blocker on mfm_runrs_process_bits_device returns MFM_E_INVAL with a message and the
 * state does not move, as mfm_resampler_process_bits_device does with dc_block: the blocker filters the PCM the predicate
 * would be taken from.
 */
int mfm_runrs_set_dc_block(struct mfm_runrs *rr, uint32_t on, double pole);
/* The setting: *on 0 / 1, *dc_p the Q14 (1 - pole) in use (0 when off).  Either may be NULL. */
int mfm_runrs_get_dc_block(struct mfm_runrs *rr, uint32_t *on, int32_t *dc_p);

/*
 * The bits form: the sign-bit path of the burst chain.  The burst AIS stage looks only at sample > 0 and the burst POCSAG
 * stage only at sample < 0, so for them the resampler can write one predicate bit per output in the place of the int16.
 *
 * Input.  The call consumes its input exactly as mfm_runrs_process_device does: the same plan, stretch rule, refusals and
 * per-channel state.  PCM calls and bits calls may alternate on one object, and a stretch continues across them.  `polarity`
 * is MFM_BITS_NEG or MFM_BITS_POS (anything else: MFM_E_INVAL with a message).  `invert` applies to the input as in the PCM
 * form; the predicate is taken from the Q14-rounded int16 output, so the bits are exactly the predicate of what the PCM form
 * writes.
 *
 * Result.  It replaces the previous call's, of either form.  The run list is as in the PCM form except that out_offset counts
 * 32-bit WORDS of the bits payload: a run owns (nr_out + 31) / 32 words, ascending, no gaps (a run with nr_out == 0 owns
 * none); output j of a run is bit j % 32 of word out_offset + j / 32; bits at and above nr_out in a run's last word are 0.
 * d_totals[4] = { runs, payload words, overflow, gate error }.  Every run's bits start on a word, which is what lets the
 * stages behind copy words instead of slicing samples.  A refused call writes nothing and leaves the state where it was.
 *
 * Which accessor.  After a bits call mfm_runrs_fetch and mfm_runrs_device_view answer MFM_E_STATE with a message (no PCM was
 * written); after a PCM call, and before the first call of either form (mfm_runrs_bits_view), the bits accessors do.
 *
 * Capacity.  The bits payload is allocated at create: max_out_elems / 32 + max_runs words (mfm_runrs_get_bits_capacity).
 */
int mfm_runrs_process_bits_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload,
                                  const uint64_t *d_totals, uint32_t polarity, void *stream);
struct mfm_runrs_bits_view {    /* valid until the resampler's next process call of either form */
    const struct mfm_runrs_run *d_runs;
    const uint32_t *d_bits;
    const uint64_t *d_totals;
    uint32_t polarity;          /* MFM_BITS_NEG or MFM_BITS_POS */
    uint32_t reserved;          /* 0 */
};
/* For consumers that stay on the device: the last (bits) call's runs, bit payload, d_totals[4] and polarity. */
int mfm_runrs_bits_view(struct mfm_runrs *rr, struct mfm_runrs_bits_view *view);
/* As mfm_runrs_fetch for a bits call: the runs and the used words of the bit payload; *nr_words = the call's total. */
int mfm_runrs_fetch_bits(struct mfm_runrs *rr, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits, size_t max_words,
                         size_t *nr_words);
/* The capacities of the bits form: max_runs as mfm_runrs_get_capacity gives it, and max_out_elems / 32 + max_runs words. */
int mfm_runrs_get_bits_capacity(struct mfm_runrs *rr, uint32_t *max_runs, uint64_t *max_words);
/*
 * The state between calls, for moving a stream between objects and for tests that place a stretch at a chosen position.
 * struct mfm_runrs_state and struct mfm_runrs_dc_state are declared with the host twins below, which carry the same.
 * mfm_runrs_fetch_state waits for the queued work and copies state [nr_channels], the pending samples [nr_channels][plen]
 * (plen = ((nr_coeffs + interpolate - 1) / interpolate + 3) & ~3; NULL: not wanted) and the DC blocker's dc [nr_channels] (NULL:
 * not wanted; MFM_E_STATE with a message when it is wanted and the blocker is off).
 * mfm_runrs_store_state waits likewise and writes what the next process call reads: state and pending are required, dc is
 * required with the blocker on and must be NULL with it off.  Every channel is validated first (csrc/mfm_runrs.h states the
 * conditions: phase < interpolate, pending <= plen, outs and expected below 2^62 or expected = ~0 with the rest zero, the
 * blocker's reserved 0); a state that fails gets MFM_E_INVAL with a message naming channel and field, and nothing is written.
 * Capacities, the blocker's setting and the result of the last call (PCM or bits) stay as they were.  nr_channels must be the
 * configuration's (MFM_E_INVAL).
 */
struct mfm_runrs_state;
struct mfm_runrs_dc_state;
int mfm_runrs_fetch_state(struct mfm_runrs *rr, struct mfm_runrs_state *state, int16_t *pending, struct mfm_runrs_dc_state *dc,
                          size_t nr_channels);
int mfm_runrs_store_state(struct mfm_runrs *rr, const struct mfm_runrs_state *state, const int16_t *pending,
                          const struct mfm_runrs_dc_state *dc, size_t nr_channels);
/*
 * The view entries: a resampler sized to a part of a payload reads that payload in place.  They are
 * mfm_runrs_process_device and mfm_runrs_process_bits_device with the two meanings of d_totals[1] taken apart.  The plain
 * entries read it as how much payload exists (the bound of every run's range payload_offset .. + nr_windows * W) and as the load
 * that must fit max_windows * W.  Here *d_payload_elems, one uint64 on the device, is how much payload exists, and d_totals[1] is
 * read only as the load (MFM_RUNRS_OVER_OWN when it exceeds max_windows * W).  That is what a local route of the run router
 * hands over (mfm_runroute_create_local below): mfm_runroute_device_view's three addresses and mfm_runroute_bound_view's.
 *
 * Everything else is the rule of the plain entries, to the bit: stretches, the per-channel state and its two buffers, the
 * refusals and their flags, the DC blocker (mfm_runrs_set_dc_block works with the PCM view entry), the bits entry's MFM_E_INVAL
 * with the blocker on, and mfm_runrs_fetch, _device_view, _bits_view, _fetch_bits, _fetch_state and _store_state.  View calls and
 * plain calls may alternate on one object, and a stretch continues across them.  A run longer than max_windows * W cannot
 * belong to a load that fits and is refused as a range that does not exist is (MFM_RUNRS_GATE_BAD_RUNS).
 *
 * Safe misuse.  A local route's view handed to the PLAIN entries is either refused (MFM_RUNRS_GATE_BAD_RUNS: a run whose range
 * ends beyond the route's load) or right; it never reads outside the gate's payload, because the load is at most the gate's
 * total.
 */
int mfm_runrs_process_view_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                                  const uint64_t *d_payload_elems, void *stream);
int mfm_runrs_process_bits_view_device(struct mfm_runrs *rr, const struct mfm_gate_run *d_runs, const int16_t *d_payload,
                                       const uint64_t *d_totals, const uint64_t *d_payload_elems, uint32_t polarity, void *stream);

/*
 * ---- Run router: one gate feeds a burst chain per protocol ---------------------------------------------------------------
 * A burst resampler has one ratio and one set of taps for all channels, and a burst decoder reads all of its runs.  A capture
 * that carries several protocols (POCSAG at 38 400 Hz beside FLEX at 16 000 Hz in one paging band) therefore needs one burst
 * chain per protocol, and each chain should see only the runs of its own channels.  The router stands between the gate and the
 * burst resamplers: it partitions the gate's run list by a per-channel route table and leaves the payload where it is.  The
 * burst resampler never assumes that payload_offset values are dense, so nothing is copied.  The reference has no counterpart.
 *
 * Input.  What mfm_gate_device_view returned after mfm_gate_process_device or mfm_gate_flush_device, and
 * route_of_channel [nr_channels] given at create: a route 0 .. nr_routes - 1 per channel, or MFM_ROUTE_NONE for a channel
 * whose runs go nowhere.
 *
 * Result per route k.  It replaces the previous call's.  The run list is the gate's mfm_gate_run records whose channel has
 * route k: byte for byte, payload_offset untouched, in the gate's order (the partition is stable, so channels still ascend
 * and a channel's runs keep their order).  d_payload is the gate's pointer.  d_totals[4] = { runs of route k, the gate's
 * payload elements unchanged (the burst resampler uses them as the bound of the payload ranges), overflow (0 / 1), out of
 * step (0 / 1) }.  Order and content are deterministic: no atomic decides a position.
 *
 * Refused calls.  When the gate's totals carry overflow or out-of-step the flag is passed on to every route; when the gate
 * has more runs than the router's max_runs every route gets overflow = 1; when a run names a channel >= nr_channels (not a
 * gate's run list) every route gets out of step = 1.  In all three cases every route gets 0 runs and 0 elements, and the
 * burst resamplers behind refuse as they do behind a gate (MFM_RUNRS_OVER_GATE, MFM_RUNRS_GATE_OUT_OF_STEP) and keep their
 * state.  The router itself carries no state between calls.
 *
 * Sizing what stands behind.  Channel numbers stay global, so events keep true channel numbers and stretch_window; a route's
 * burst resampler is therefore created with the WHOLE gate's numbers (the same nr_channels, max_windows and max_runs), and its
 * state and output buffers are sized for all channels.  Packing a dense payload per route would let the stages behind be
 * sized to the route, at the price of a copy of every open window; a router made by mfm_runroute_create does not do that, one made
 * by mfm_runroute_create_sets with MFM_RUNROUTE_F_PACK (below) does.
 *
 * Refusals at create (MFM_E_INVAL with a message, never a fallback): nr_routes outside 1 .. MFM_RUNROUTE_MAX_ROUTES, a table
 * entry that is neither below nr_routes nor MFM_ROUTE_NONE, non-zero flags, nr_channels or window_samples out of range, a
 * default capacity asked for without max_in_samples.
 */
#define MFM_RUNROUTE_MAX_ROUTES 8u
#define MFM_ROUTE_NONE 255u

struct mfm_runroute; /* opaque */

struct mfm_runroute_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;       /* 1 .. 65535, the gate's */
    uint32_t nr_routes;         /* K: 1 .. MFM_RUNROUTE_MAX_ROUTES */
    uint32_t window_samples;    /* W, the gate's; read only for the defaults below */
    uint32_t max_windows;       /* as mfm_runrs_config.max_windows; read only where max_runs is 0 */
    uint32_t max_runs;          /* most runs one gate call may carry; 0 = exactly the default of a burst resampler made from
                                   the same numbers (mfm_runrs_config.max_runs) */
    uint32_t max_in_samples;    /* the gate's; read only where max_runs is 0 */
    uint32_t preroll_windows;   /* the gate's P; likewise */
    uint32_t flags;             /* 0 */
};

int mfm_runroute_create(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *route_of_channel);
void mfm_runroute_destroy(struct mfm_runroute **prt);
/*
 * Partition the runs of one gate call.  Work is queued on `stream` (the gate call's, or one ordered behind it); no host
 * synchronisation and no count is read on the host: the launch is sized from the capacity, and lanes that have no run return
 * after reading the totals.  d_runs and d_totals are read until the queued work has run; d_payload is only handed on.
 */
int mfm_runroute_process_device(struct mfm_runroute *rt, const struct mfm_gate_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                                void *stream);
/*
 * For the burst resampler of route `route`: what it takes in the place of the gate's view.  d_runs (a buffer of max_runs
 * records per route) and d_totals are fixed at create, so they are known without waiting; d_payload is the pointer the last
 * mfm_runroute_process_device call was given (NULL before the first).  Any of the three may be NULL.  MFM_E_INVAL for a
 * route >= nr_routes.
 */
int mfm_runroute_device_view(struct mfm_runroute *rt, uint32_t route, const struct mfm_gate_run **d_runs, const int16_t **d_payload,
                             const uint64_t **d_totals);
/*
 * Wait for the last call, read route `route`'s totals into *nr_runs and *nr_elems (the gate's payload elements) and copy its
 * runs.  MFM_E_NOMEM when max_runs is too small (nothing copied, *nr_runs says what is needed); MFM_E_STATE with a message
 * when the call was refused (nothing copied).
 */
int mfm_runroute_fetch(struct mfm_runroute *rt, uint32_t route, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, size_t *nr_elems);
/* The run capacity fixed at create: max_runs as given or its default. */
int mfm_runroute_get_capacity(struct mfm_runroute *rt, uint32_t *max_runs);

/*
 * ---- Run router, the sets form: shared channels, and packed routes sized to the route ---------------------------------
 * Paging carriers time-share one frequency between POCSAG and FLEX, so a channel may have to reach two chains; and a route's
 * chain behind the zero-copy router is sized for all channels.  mfm_runroute_create_sets takes the same configuration and
 * returns the same object type: mfm_runroute_process_device, _device_view, _fetch, _get_capacity and _destroy work on it
 * unchanged.  mfm_runroute_create and what it refuses stay as they are.
 *
 * Input.  routes_of_channel [nr_channels]: a SET per channel, bit k set = the channel's runs go to route k, 0 = nowhere.  A
 * bit at or above nr_routes is MFM_E_INVAL with a message that names the channel.  cfg->flags is 0 or MFM_RUNROUTE_F_PACK.
 *
 * Without PACK the router stays zero-copy with global channel numbers: route k's list is the gate's records whose channel's
 * set has bit k, byte for byte, as a stable partition; a run of a shared channel stands in several lists.  Totals and the
 * three refusals are those of the section above, and a table with one bit per channel gives byte for byte what
 * mfm_runroute_create gives for the corresponding route table.
 *
 * With PACK every route gets route-local channel numbers and a dense payload of its own.  Route k's record i is the gate's
 * record with `channel` replaced by the channel's rank among the route's channels (ascending: the numbering is fixed for the
 * object's life, channels still ascend, and mfm_runroute_route_channels inverts it) and `payload_offset` replaced by the sum of
 * nr_windows * W over the route's earlier records; first_window and nr_windows are untouched.  The route's payload holds
 * exactly those windows, copied from the gate's payload at the gate's payload_offset (which need not be dense).  d_totals[4] =
 * { runs, the route's payload elements, overflow, out of step }.  mfm_runroute_device_view returns the route's own payload
 * buffer, fixed at create.  The list beyond the totals' runs and the payload beyond the totals' elements are not defined.
 *
 * Refused calls.  The gate's two flags, more runs than the router's max_runs and a run of a channel >= nr_channels flag every
 * route as above.  Under PACK a run whose payload range does not lie within the gate's payload elements does the same (out of
 * step: the copy would read it), and a route whose runs or windows in one call exceed its own capacity (below) gets
 * overflow = 1 with 0 runs and 0 elements: nothing is written past the capacity and the other routes are unaffected.
 *
 * Sizing what stands behind: mfm_runroute_route_caps returns the three numbers to create route k's burst resampler with
 * (mfm_runrs_config.nr_channels, max_windows, max_runs).  Without PACK, and for an object of mfm_runroute_create, these are the
 * whole gate's: nr_channels, cfg->max_windows as given (0 stays 0, the burst resampler's default) and the router's max_runs.
 * With PACK, for a route of n channels and per = max(max_in_samples / W + 1, preroll_windows):
 *   nr_channels = n
 *   max_windows = n * per, and no more than an explicit cfg->max_windows
 *   max_runs    = min(max_windows, n * ((per + 1) / 2)), and no more than an explicit cfg->max_runs
 * which is the burst resampler's own rule (mfm_runrs_config) for n channels.  With max_in_samples == 0 there is no default to
 * form: max_windows and max_runs must both be given and are returned as given.  A burst resampler made from the three numbers
 * never answers MFM_RUNRS_OVER_OWN to a call the router did not flag; with the defaults no route can overflow at all.
 *
 * Refusals at create (MFM_E_INVAL with a message): those of mfm_runroute_create, flags other than 0 or MFM_RUNROUTE_F_PACK,
 * a set with a bit at or above nr_routes; under PACK a route without a channel, window_samples out of range, and
 * max_in_samples == 0 without both max_windows and max_runs.
 */
#define MFM_RUNROUTE_F_PACK 1u

int mfm_runroute_create_sets(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel);
/* The global channel numbers of route `route`, ascending: under PACK local channel i is channels[i].  Valid for every router
 * object.  *nr = the route's channels; MFM_E_NOMEM when max is too small (the first max are written). */
int mfm_runroute_route_channels(struct mfm_runroute *rt, uint32_t route, uint32_t *channels, size_t max, size_t *nr);
/* The numbers to create route `route`'s burst resampler with, by the rule above.  Any of the three may be NULL. */
int mfm_runroute_route_caps(struct mfm_runroute *rt, uint32_t route, uint32_t *nr_channels, uint32_t *max_windows, uint32_t *max_runs);
/*
 * PACK only (MFM_E_INVAL with a message otherwise): wait for the last call as mfm_runroute_fetch does and copy route `route`'s
 * payload.  *nr_elems = the route's payload elements; MFM_E_NOMEM when max_elems is too small (nothing copied); MFM_E_STATE
 * with a message when the call or the route was refused.
 */
int mfm_runroute_fetch_payload(struct mfm_runroute *rt, uint32_t route, int16_t *payload, size_t max_elems, size_t *nr_elems);

/*
 * ---- Run router, the local form: route-local channel numbers on the gate's payload in place -----------------------------
 * The two forms above each pay for what the other avoids: the zero-copy forms keep global channel numbers, so every route's
 * chain is sized for all channels; PACK sizes the chain to the route and copies every open window to do so.  The local form
 * gives PACK's channel numbers and capacities without the copy: the payload stays the gate's and payload_offset stays the
 * gate's, and the burst resampler behind reads it through its view entries (mfm_runrs_process_view_device below), which take
 * the bound of the payload ranges apart from the load.  mfm_runroute_create_local is a creator of its own, not a flag, and
 * returns the same object type: mfm_runroute_process_device, _device_view, _fetch, _get_capacity, _route_channels, _route_caps
 * and _destroy work on it; mfm_runroute_fetch_payload answers MFM_E_INVAL as for every object without PACK.  The other two
 * creators and what they refuse stay as they are.
 *
 * Input.  routes_of_channel [nr_channels], a SET per channel exactly as for mfm_runroute_create_sets (bit k = route k, 0 =
 * nowhere, a channel may stand in several routes).  cfg->flags must be 0.
 *
 * Result per route k.  Record i is the gate's record with `channel` replaced by the channel's rank among the route's channels
 * (PACK's numbering: fixed for the object's life, ascending, inverted by mfm_runroute_route_channels); first_window, nr_windows
 * and payload_offset are untouched; the partition is stable.  mfm_runroute_device_view returns as d_payload the gate's pointer
 * handed to the last call.  d_totals[4] = { runs, the route's LOAD = the sum of nr_windows * W over its records, overflow, out
 * of step }, and mfm_runroute_fetch's *nr_elems is that load.  The load is what the route's resampler must hold; it is NOT a
 * bound of the payload offsets, which range over the gate's whole payload.  That bound is mfm_runroute_bound_view's: one uint64
 * at an address fixed at create, which every process call writes with the gate's payload elements (d_totals[1] of the gate), or
 * with 0 when the call is refused for the whole router.  On objects of the other two creators mfm_runroute_bound_view is
 * MFM_E_INVAL with a message: their totals carry the bound themselves.
 *
 * Refused calls.  The gate's two flags, more runs than the router's max_runs and a run of a channel >= nr_channels flag every
 * route, as above.  A route whose runs or windows in one call exceed its own capacity gets overflow = 1 with 0 runs and 0
 * elements, and the other routes are unaffected, as under PACK.  A payload range outside the gate's elements is left to the
 * resampler's view entry, as in the zero-copy forms: nothing is copied, so nothing is read here.
 *
 * Sizing what stands behind: mfm_runroute_route_caps returns PACK's rule (n channels, n * per windows, the run bound of the
 * burst resampler's own rule for n channels).  A burst resampler made from the three numbers never answers MFM_RUNRS_OVER_OWN
 * through its view entry to a call the router did not flag.
 *
 * Refusals at create (MFM_E_INVAL with a message): those of mfm_runroute_create_sets under PACK - a route without a channel,
 * window_samples out of range, max_in_samples == 0 without both max_windows and max_runs, a set with a bit at or above
 * nr_routes - and non-zero flags.
 */
int mfm_runroute_create_local(struct mfm_runroute **prt, const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel);
/* The address of the bound, for mfm_runrs_process_view_device's d_payload_elems: fixed at create, written by every process
 * call on its stream. */
int mfm_runroute_bound_view(struct mfm_runroute *rt, const uint64_t **d_payload_elems);

/*
 * ---- Burst AIS stage: the burst resampler's runs through the AIS demodulator, on the device -----------------------------
 * The AIS stage above (mfm_ais_*) on ragged runs instead of full rows: its input is what mfm_runrs_device_view returns (the
 * run list, the dense resampled payload, the totals), all read on the device, and its output is AIS packet events.
 *
 * Stretch means what it means for the burst resampler; this stage does not track windows.  Run r continues its channel's
 * stretch exactly when MFM_RUNRS_BEGINS is clear in runs[r].flags, otherwise it begins a new one.  Sample numbers are
 * stretch-relative: sample first_out + j is output j of the run.
 *
 * Rule.  The events of a stretch are exactly what a fresh reference demodulator (ais_demod_on_pcm, ais/ais_demod.c:215-258,
 * SEARCH_SYNC, all registers and prior samples zero) returns when fed the stretch's resampled PCM, with the conventions of
 * mfm_ais: bit = (sample > 0); the first packet bit is read four samples after the matching sample, then one every five; an
 * event at each packet end with current_bit / 8 >= 4; the FCS as there.  A packet still being received when its stretch ends
 * is dropped without an event.  A run with nr_out == 0 produces no event and still begins or continues its stretch.  Events
 * do not depend on how the stream was cut into calls.
 *
 * State.  Per channel, on the device (struct mfm_runais_state below, which the host twin carries too): the walker's state of
 * the stretch in progress (mode, positions, NRZI and flag history, the packet so far), the outputs seen, the stretch's first
 * window, and the last 256 sample bits of the stretch: (160 + 5) samples of register history, rounded to words.  Two state
 * buffers are used in turn: a channel's first run reads the old state, its last run leaves the new one.  A channel without a
 * run in a call keeps its state.
 *
 * Result.  It replaces the previous call's: one dense list of mfm_runais_event in run order, stream order within a run;
 * d_totals[4] = { events, runs, overflow, input error }.  Order and content are deterministic: the walk of a run writes into a
 * slot range given by a scan, and the ranges are packed afterwards.
 *
 * Event bound.  The first packet bit is read 4 samples after the preamble match, one more every 5, and an event needs 32
 * kept bits, so a packet ends at least 4 + 5 * 31 = 159 samples after its match, which lies behind the previous packet end:
 * two packet ends of a stretch are at least 160 samples apart.  A run of nr_out samples therefore ends at most
 * nr_out / 160 + 1 packets (the + 1: a packet carried in ends anywhere), and a call at most the sum of that over its runs.
 *
 * Refused calls produce nothing, leave the per-channel state untouched and raise a flag that mfm_runais_fetch reports as
 * MFM_E_STATE with a message:
 *   overflow     MFM_RUNAIS_OVER_RUNS: more runs than max_runs; MFM_RUNAIS_OVER_EVENTS: the call's event bound exceeds
 *                max_events (by the bound, not by the count, so "does it fit" does not depend on the signal)
 *   input error  MFM_RUNAIS_IN_RUNRS: the resampler's totals carry overflow or gate error; MFM_RUNAIS_IN_OUT_OF_STEP: a
 *                continuing run's first_out is not the channel's output count, the channel has no stretch, or the run is not
 *                its channel's first of the call; MFM_RUNAIS_IN_BAD_RUNS: a run names a channel >= nr_channels, channels do
 *                not ascend, a beginning run's first_out is not 0, an output range lies beyond the resampler's totals or the
 *                totals beyond max_out_samples.  These are checked before anything of the payload is read.
 */
#define MFM_RUNAIS_OVER_RUNS 1u
#define MFM_RUNAIS_OVER_EVENTS 2u
#define MFM_RUNAIS_IN_RUNRS 1u
#define MFM_RUNAIS_IN_OUT_OF_STEP 2u
#define MFM_RUNAIS_IN_BAD_RUNS 4u

struct mfm_runais_event {       /* 200 bytes */
    uint32_t channel;
    uint32_t fcs_valid;
    uint32_t nr_bytes;          /* 4 .. 160, FCS bytes included */
    uint32_t run;               /* index, in this call's run list, of the run in which the packet ended */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
    uint64_t sample;            /* stretch-relative index of the resampled sample that ended the packet */
    uint64_t start_sample;      /* stretch-relative index of the sample where the preamble matched */
    uint8_t bytes[160];         /* as mfm_ais_event.bytes */
};

struct mfm_runais; /* opaque */

struct mfm_runais_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst resampler's capacities (mfm_runrs_get_capacity) */
    uint32_t max_out_samples;
    uint32_t max_events;        /* per call, all channels; 0 = max_out_samples / 160 + max_runs, cannot overflow */
    uint32_t flags;             /* 0 */
};

int mfm_runais_create(struct mfm_runais **pa, const struct mfm_runais_config *cfg);
void mfm_runais_destroy(struct mfm_runais **pa);
/*
 * Demodulate the runs of one burst resampler call: d_runs, d_payload and d_totals are what mfm_runrs_device_view returned.
 * Work is queued on `stream` (the resampler call's, or one ordered behind it); no host synchronisation and no count read on
 * the host: launches are sized from the capacities fixed at create, surplus workgroups return after reading the totals.  The
 * three arrays are read until the queued work has run.
 */
int mfm_runais_process_device(struct mfm_runais *a, const struct mfm_runrs_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                              void *stream);
/*
 * The same call on the burst resampler's bits form (mfm_runrs_bits_view after mfm_runrs_process_bits_device with
 * MFM_BITS_POS; any other polarity: MFM_E_INVAL with a message at the call).  Events, state, bounds and refusals are exactly
 * those of the PCM entry on the same stretches; PCM and bits calls may alternate on one object (the carried tail is bits in
 * both).  Only the slicer differs: word k of a run's sample bits is payload word out_offset + k, a 4-byte copy per 32
 * samples.  The range check reads out_offset + (nr_out + 31) / 32 <= totals[1] (totals[1] itself at most max_out_samples / 32
 * + max_runs), runs before anything of the payload is read, and the sum of nr_out is still bounded by max_out_samples.
 */
int mfm_runais_process_bits_device(struct mfm_runais *a, const struct mfm_runrs_bits_view *view, void *stream);
/*
 * Wait for the last call and copy its events (the copy is sized by the call's events).  MFM_E_NOMEM when max_events is too
 * small (nothing copied, *nr_events = needed); MFM_E_STATE with a message when the call was refused (nothing copied, the
 * state did not move: the same input in a call that is right is right again).
 */
int mfm_runais_fetch(struct mfm_runais *a, struct mfm_runais_event *events, size_t max_events, size_t *nr_events);
/* For consumers that stay on the device: the last call's events and d_totals[4], valid until the next call.  Either may be
 * NULL. */
int mfm_runais_device_view(struct mfm_runais *a, const struct mfm_runais_event **d_events, const uint64_t **d_totals);
/* The per-channel state (struct mfm_runais_state, declared with the host twin below), for moving a stream between objects:
 * fetch_state waits for the queued work and copies it out; store_state waits likewise, validates every channel
 * (csrc/mfm_runais.h states the conditions) and writes what the next process call reads.  A state that fails gets MFM_E_INVAL
 * with a message naming channel and field, and nothing is written.  The events of the last call stay readable. */
struct mfm_runais_state;
int mfm_runais_fetch_state(struct mfm_runais *a, struct mfm_runais_state *state, size_t nr_channels);
int mfm_runais_store_state(struct mfm_runais *a, const struct mfm_runais_state *state, size_t nr_channels);
/*
 * Stretch-end records: how each stretch ended and what the closing squelch cut.  Off at create; with the report on, one record
 * per stretch over the whole stream.  Events, totals and state are those of an object with the report off, and with it off a
 * process call queues exactly the launches it queued before the report existed.
 *
 * Rule.  A stretch of channel c ends in one of three ways.
 *   (a) A call that is not refused holds a run r that is c's first run of the call and has MFM_RUNRS_BEGINS, and the state the
 *       call started from has has_stretch == 1.  The record is taken from that carried state; run = r.
 *   (b) A call that is not refused holds a run r of c whose successor r + 1 in the list is also of channel c (that successor
 *       necessarily begins a stretch).  The record is taken from the state r's walk ended in; run = r + 1.
 *   (c) The end call below, at the end of a stream behind the gate's flush: every channel with has_stretch == 1 gets a record,
 *       channels ascending, run = 0xffffffff, and afterwards every channel's state is all zero.  The end call replaces the
 *       previous result: the event list is empty and the totals read { 0, 0, 0, 0 }.  After it a continuing run is
 *       MFM_RUNAIS_IN_OUT_OF_STEP (the channel has no stretch) and a beginning run is fine.
 * The records of a process call follow run-list order, (a) in front of (b) where a run yields both: channels ascending, stream
 * order within a channel.  A refused call writes no record and moves no state; the same input in calls that fit yields the
 * right records.  A record's content does not depend on how the stream was cut into calls, only the call it appears in does.
 * A run with nr_out == 0 begins or continues its stretch as before, and a stretch of such runs alone still gets a record, with
 * outs = 0 and mode SEARCH.  A process call holds at most max_runs records and an end call at most nr_channels: the capacity
 * allocated when the report is switched on is the larger of the two.
 *
 * mode 1 (RECEIVE) says a packet was cut: its preamble matched at start_sample and nr_bits bits had been kept.
 */
struct mfm_runais_end {         /* 48 bytes */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
    uint64_t outs;              /* resampled outputs of the whole stretch */
    uint64_t start_sample;      /* RECEIVE: as the event of the packet would have reported it; 0 in SEARCH */
    uint32_t channel;
    uint32_t run;               /* index, in this call's run list, of the run that begins the next stretch; 0xffffffff: end call */
    uint32_t mode;              /* 0 SEARCH, 1 RECEIVE */
    uint32_t nr_bits;           /* RECEIVE: bits of the packet kept so far */
    uint32_t reserved[2];       /* 0 */
};
/* Switch the report on or off.  Valid only before the first process call: MFM_E_STATE with a message afterwards. */
int mfm_runais_set_end_report(struct mfm_runais *a, int on);
/* (c) above, queued on `stream` like a process call.  MFM_E_STATE with a message when the report is off. */
int mfm_runais_end_stretches_device(struct mfm_runais *a, void *stream);
/* Wait for the last call (process or end) and copy its records.  MFM_E_NOMEM when max_ends is too small (nothing copied,
 * *nr_ends = needed); MFM_E_STATE with a message when the report is off, before the first call, or when the last call was
 * refused. */
int mfm_runais_fetch_ends(struct mfm_runais *a, struct mfm_runais_end *ends, size_t max_ends, size_t *nr_ends);
/* For consumers that stay on the device: the last call's records and d_end_totals[2] = { records, records with mode != 0 },
 * valid until the next call.  Either may be NULL.  MFM_E_STATE with a message when the report is off. */
int mfm_runais_ends_view(struct mfm_runais *a, const struct mfm_runais_end **d_ends, const uint64_t **d_end_totals);

/*
 * ---- Burst POCSAG stage: the burst resampler's runs through the POCSAG demodulator, on the device -----------------------
 * The pager stage above (mfm_pocsag_*) on ragged runs instead of full rows: its input is what mfm_runrs_device_view returns
 * (the run list, the dense resampled payload, the totals), all read on the device, and its output is POCSAG events.  The
 * stage assumes 38 400 Hz, as mfm_pocsag does.
 *
 * Stretch means what it means for the burst resampler; this stage does not track windows.  Run r continues its channel's
 * stretch exactly when MFM_RUNRS_BEGINS is clear in runs[r].flags, otherwise it begins a new one.  Sample numbers are
 * stretch-relative: sample first_out + j is output j of the run.
 *
 * Rule.  The events of a stretch are exactly what a fresh reference decoder (pager_pocsag_on_pcm, pager/pager_pocsag.c:434-543,
 * with the three detectors of :81-117; state SEARCH, all eye registers, counters and batch words zero) returns when fed the
 * stretch's resampled PCM, with the conventions of mfm_pocsag: bit = (sample < 0); sync = popcount(word ^ 0x7cd215d8) <= 4;
 * the eye fires when a run of more than samples_per_bit / 2 matches ends, with offset matches / 2; batch words are filled LSB
 * first and masked with 0x7fffffff before BCH, nr_ok / fail_mask / raw / corrected as there; when two detectors fire on one
 * sample the later one (2400 after 1200 after 512) wins and only the winner is reported.  A batch or sync word still being
 * collected when its stretch ends is dropped without an event, as the reference drops it at the end of a stream.  A run with
 * nr_out == 0 produces no event and still begins or continues its stretch.  Events do not depend on how the stream was cut
 * into calls.
 *
 * No lag.  An event is reported by the call and run whose [first_out, first_out + nr_out) holds its `sample`: the partly
 * collected batch travels in the per-channel state, as it does in the reference's struct pager_pocsag_batch.
 *
 * State.  Per channel, on the device (struct mfm_runpocsag_state below, which the host twin carries too): the walker's mode,
 * baud and samples per bit, the sample-skip counter, the batch so far, the sync word so far, the three nr_eye_matches, the
 * outputs seen, the stretch's first window, the distance back to the last detector reset (saturating) and the last 2400
 * sample bits of the stretch: the slowest detector keeps 32 bits 75 samples apart.  Two state buffers are used in turn: a
 * channel's first run reads the old state, its last run leaves the new one.  A channel without a run in a call keeps its
 * state.  Only a channel's first run of a call can continue a stretch, so every run of a call is walked independently.
 *
 * Result.  It replaces the previous call's: one dense list of mfm_runpocsag_event in run order, stream order within a run;
 * d_totals[4] = { events, runs, overflow, input error }.  Order and content are deterministic: the walk of a run writes into a
 * slot range given by a scan, and the ranges are packed afterwards.
 *
 * Event bound.  Within a stretch the events follow (FOUND BATCH (KEPT BATCH)* LOST)*.  A BATCH event needs 512 bits after the
 * previous sync slot's 32, so two BATCH events are at least 544 bit periods = 544 * 16 = 8704 samples apart: a run of nr_out
 * samples holds at most nr_out / 8704 + 1 of them.  Between two consecutive BATCH events lie at most two others (KEPT, or LOST
 * FOUND), in front of a run's first at most two (a transmission carried in: LOST FOUND) and behind its last at most two, so a
 * run holds at most 3 * (nr_out / 8704 + 1) + 2 events and a call at most the sum of that over its runs.
 *
 * Refused calls produce nothing, leave the per-channel state untouched and raise a flag that mfm_runpocsag_fetch reports as
 * MFM_E_STATE with a message:
 *   overflow     MFM_RUNPOCSAG_OVER_RUNS: more runs than max_runs; MFM_RUNPOCSAG_OVER_EVENTS: the call's event bound exceeds
 *                max_events (by the bound, not by the count, so "does it fit" does not depend on the signal)
 *   input error  MFM_RUNPOCSAG_IN_RUNRS: the resampler's totals carry overflow or gate error; MFM_RUNPOCSAG_IN_OUT_OF_STEP: a
 *                continuing run's first_out is not the channel's output count, the channel has no stretch, or the run is not
 *                its channel's first of the call; MFM_RUNPOCSAG_IN_BAD_RUNS: a run names a channel >= nr_channels, channels
 *                do not ascend, a beginning run's first_out is not 0, an output range lies beyond the resampler's totals or
 *                the totals beyond max_out_samples.  These are checked before anything of the payload is read.
 */
#define MFM_RUNPOCSAG_OVER_RUNS 1u
#define MFM_RUNPOCSAG_OVER_EVENTS 2u
#define MFM_RUNPOCSAG_IN_RUNRS 1u
#define MFM_RUNPOCSAG_IN_OUT_OF_STEP 2u
#define MFM_RUNPOCSAG_IN_BAD_RUNS 4u

struct mfm_runpocsag_event {    /* 176 bytes */
    uint32_t type;              /* MFM_POCSAG_EV_* */
    uint32_t baud;              /* 512 / 1200 / 2400 */
    uint32_t channel;
    uint32_t aux;               /* as mfm_pocsag_event.aux */
    uint32_t run;               /* index, in this call's run list, of the run that holds `sample` */
    uint32_t nr_ok;             /* BATCH: as mfm_pocsag_event */
    uint32_t fail_mask;
    uint32_t reserved;          /* 0 */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
    uint64_t sample;            /* stretch-relative index of the resampled sample that completed the event */
    uint32_t raw[16];
    uint32_t corrected[16];
};

struct mfm_runpocsag; /* opaque */

struct mfm_runpocsag_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst resampler's capacities (mfm_runrs_get_capacity) */
    uint32_t max_out_samples;
    uint32_t max_events;        /* per call, all channels; 0 = 3 * (max_out_samples / 8704) + 5 * max_runs, cannot overflow */
    uint32_t flags;             /* 0 */
};

int mfm_runpocsag_create(struct mfm_runpocsag **pp, const struct mfm_runpocsag_config *cfg);
void mfm_runpocsag_destroy(struct mfm_runpocsag **pp);
/*
 * Decode the runs of one burst resampler call: d_runs, d_payload and d_totals are what mfm_runrs_device_view returned.
 * Work is queued on `stream` (the resampler call's, or one ordered behind it); no host synchronisation and no count read on
 * the host: launches are sized from the capacities fixed at create, surplus workgroups return after reading the totals.  The
 * three arrays are read until the queued work has run.
 */
int mfm_runpocsag_process_device(struct mfm_runpocsag *p, const struct mfm_runrs_run *d_runs, const int16_t *d_payload,
                                 const uint64_t *d_totals, void *stream);
/*
 * The same call on the burst resampler's bits form (mfm_runrs_bits_view after mfm_runrs_process_bits_device with
 * MFM_BITS_NEG; any other polarity: MFM_E_INVAL with a message at the call).  Events, state, bounds and refusals are exactly
 * those of the PCM entry on the same stretches; PCM and bits calls may alternate on one object (the carried tail is bits in
 * both).  Only the slicer differs: word k of a run's sample bits is payload word out_offset + k, a 4-byte copy per 32
 * samples.  The range check reads out_offset + (nr_out + 31) / 32 <= totals[1] (totals[1] itself at most max_out_samples / 32
 * + max_runs), runs before anything of the payload is read, and the sum of nr_out is still bounded by max_out_samples.
 */
int mfm_runpocsag_process_bits_device(struct mfm_runpocsag *p, const struct mfm_runrs_bits_view *view, void *stream);
/*
 * Wait for the last call and copy its events (the copy is sized by the call's events).  MFM_E_NOMEM when max_events is too
 * small (nothing copied, *nr_events = needed); MFM_E_STATE with a message when the call was refused (nothing copied, the
 * state did not move: the same input in a call that is right is right again).
 */
int mfm_runpocsag_fetch(struct mfm_runpocsag *p, struct mfm_runpocsag_event *events, size_t max_events, size_t *nr_events);
/* For consumers that stay on the device: the last call's events and d_totals[4], valid until the next call.  Either may be
 * NULL. */
int mfm_runpocsag_device_view(struct mfm_runpocsag *p, const struct mfm_runpocsag_event **d_events, const uint64_t **d_totals);
struct mfm_runpocsag_state;
/* Wait for the last call and copy the per-channel state it left, state[nr_channels] (for tests and for moving a stream
 * between objects: it is what the host twin carries). */
int mfm_runpocsag_fetch_state(struct mfm_runpocsag *p, struct mfm_runpocsag_state *state, size_t nr_channels);
/* The way back: waits for the queued work, validates every channel (csrc/mfm_runpocsag.h states the conditions) and writes
 * what the next process call reads.  A state that fails gets MFM_E_INVAL with a message naming channel and field, and nothing
 * is written.  The events of the last call stay readable. */
int mfm_runpocsag_store_state(struct mfm_runpocsag *p, const struct mfm_runpocsag_state *state, size_t nr_channels);
/*
 * Stretch-end records, as the burst AIS stage's: off at create, one record per stretch over the whole stream, and nothing
 * else changes with the report on or off.
 *
 * Rule.  A stretch of channel c ends (a) in front of a run r that is c's first of a call that is not refused and has
 * MFM_RUNRS_BEGINS while the state the call started from has has_stretch == 1 (the record of that carried state, run = r);
 * (b) behind a run r of such a call whose successor r + 1 is also of channel c (the record of the state r's walk ended in,
 * run = r + 1); (c) at the end call: every channel with has_stretch == 1, channels ascending, run = 0xffffffff, after which
 * every state is all zero, the event list is empty, the totals read { 0, 0, 0, 0 }, a continuing run is
 * MFM_RUNPOCSAG_IN_OUT_OF_STEP and a beginning run is fine.  Records follow run-list order, (a) in front of (b).  A refused
 * call writes no record and moves no state.  Content does not depend on how the stream was cut into calls.  A stretch of runs
 * with nr_out == 0 alone gets a record with outs = 0 and mode SEARCH.  At most max_runs records per process call and
 * nr_channels per end call.
 *
 * The cut batch.  Every codeword of a batch is BCH-protected on its own, so the whole words of a batch the squelch cut
 * (mode 2, words 0 .. nr_words - 1) are corrected here exactly as a BATCH event's are: masked with 0x7fffffff, the stage's own
 * decoder, nr_ok the words accepted in front of the first failure (at most nr_words), fail_mask with bits below nr_words only.
 * raw[] is the batch as collected, the nr_bits bits of the word in progress included; corrected[z] is 0 from nr_words on.
 */
struct mfm_runpocsag_end {      /* 184 bytes */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
    uint64_t outs;              /* resampled outputs of the whole stretch */
    uint32_t channel;
    uint32_t run;               /* index, in this call's run list, of the run that begins the next stretch; 0xffffffff: end call */
    uint32_t mode;              /* 0 SEARCH, 2 BATCH, 3 SYNCWORD */
    uint32_t baud;              /* BATCH / SYNCWORD: 512 / 1200 / 2400 */
    uint32_t nr_words;          /* BATCH: whole words collected */
    uint32_t nr_bits;           /* BATCH: bits of the word in progress */
    uint32_t nr_sync_bits;      /* SYNCWORD: bits of the sync slot collected */
    uint32_t reserved;          /* 0 */
    uint32_t nr_ok;
    uint32_t fail_mask;
    uint32_t raw[16];
    uint32_t corrected[16];
};
/* Switch the report on or off.  Valid only before the first process call: MFM_E_STATE with a message afterwards. */
int mfm_runpocsag_set_end_report(struct mfm_runpocsag *p, int on);
/* (c) above, queued on `stream` like a process call.  MFM_E_STATE with a message when the report is off. */
int mfm_runpocsag_end_stretches_device(struct mfm_runpocsag *p, void *stream);
/* Wait for the last call (process or end) and copy its records.  MFM_E_NOMEM when max_ends is too small (nothing copied,
 * *nr_ends = needed); MFM_E_STATE with a message when the report is off, before the first call, or when the last call was
 * refused. */
int mfm_runpocsag_fetch_ends(struct mfm_runpocsag *p, struct mfm_runpocsag_end *ends, size_t max_ends, size_t *nr_ends);
/* The last call's records and d_end_totals[2] = { records, records with mode != 0 } on the device, valid until the next call.
 * Either may be NULL.  MFM_E_STATE with a message when the report is off. */
int mfm_runpocsag_ends_view(struct mfm_runpocsag *p, const struct mfm_runpocsag_end **d_ends, const uint64_t **d_end_totals);

/*
 * ---- Burst FLEX stage: the burst resampler's runs through the FLEX front half, on the device ------------------------------
 * The pager stage above (mfm_flex_*) on ragged runs instead of full rows: its input is what mfm_runrs_device_view returns
 * (the run list, the dense resampled payload, the totals), all read on the device, and its output is FLEX events and the
 * words of the frames collected.  The stage assumes 16 000 Hz, as mfm_flex does.
 *
 * Stretch means what it means for the burst resampler; this stage does not track windows.  Run r continues its channel's
 * stretch exactly when MFM_RUNRS_BEGINS is clear in runs[r].flags, otherwise it begins a new one.  Only a channel's first run
 * of a call can continue.  Sample numbers are stretch-relative: sample first_out + j is output j of the run.
 *
 * Rule.  The events and frame words of a stretch are exactly what a fresh reference decoder (pager_flex_on_pcm in state
 * SYNC_1, registers, counters and phase words zero) returns when fed the stretch's resampled PCM, with every convention the
 * mfm_flex_* comment lists: bit = (sample >= 0); ten BS1 registers; the eye is a run of three or more matching samples,
 * counted modulo 256; only the upper half of A is compared, with fewer than 4 differing bits; the swing in int16 arithmetic;
 * registers zero-filled after every reset, so nothing matches for 310 samples, and the stretch start is such a reset; a sync
 * run without swing is MFM_FLEX_EV_BAD_FIW with fiw_rc 3.  A sync, FIW or block still being collected when its stretch ends
 * is dropped without an event.  A run with nr_out == 0 produces nothing and still begins or continues its stretch.  Events
 * do not depend on how the stream was cut into calls.
 *
 * No lag.  An event is reported by the call and run whose [first_out, first_out + nr_out) holds its `sample`: BAD_BAUD at
 * s0 + 790 (s0 the first sync bit), BAD_FIW at f = s0 + 1110, FRAME at the last block symbol.
 *
 * State.  Per channel, on the device (struct mfm_runflex_state below, which the host twin carries too): the walker's mode and
 * what it has of the frame so far, positions stretch-relative, the outputs seen and the stretch's first window; and a ring
 * of the last 32 768 PCM samples of the stretch, indexed by stretch sample & 32767: the sync words are read again when the
 * FIW arrives and a block's symbols when its last one does, up to 28 155 samples later.  Two state buffers are used in turn;
 * the ring is written in place and last, from the channel's last run of a call, and not at all by a refused call.  A run that
 * begins a stretch never reads the ring.  A channel without a run in a call keeps its state.
 *
 * Result.  It replaces the previous call's: one dense list of mfm_runflex_event in run order, stream order within a run, and
 * one dense list of mfm_flex_frame_words, indexed by the FRAME events' frame_index, in event order;
 * d_totals[4] = { events, frames, overflow, input error }.  Order and content are deterministic: the walk of a run writes into
 * slot ranges given by a scan, and the ranges are packed afterwards.
 *
 * Bounds.  Every event is followed by a reset, and after a reset the next event needs 311 dead samples, a run of 3 matches,
 * the sample that ends it, 1 sample or more to the first sync bit and 790 more: two events of a stretch are at least 1105
 * samples apart, so a run holds at most nr_out / 1105 + 1 events.  A FRAME's last symbol lies at least 28 560 samples behind
 * its last FIW bit, which lies 1110 behind the first sync bit: two FRAME events are at least 315 + 1110 + 28 560 = 29 985
 * samples apart, so a run holds at most nr_out / 29985 + 1 frames.  A call holds at most the sums over its runs.
 *
 * Refused calls produce nothing, leave the per-channel state and the ring untouched and raise a flag that mfm_runflex_fetch
 * reports as MFM_E_STATE with a message:
 *   overflow     MFM_RUNFLEX_OVER_RUNS: more runs than max_runs; MFM_RUNFLEX_OVER_EVENTS: the call's event bound exceeds
 *                max_events or its frame bound max_frames (by the bound, not by the count)
 *   input error  MFM_RUNFLEX_IN_RUNRS, MFM_RUNFLEX_IN_OUT_OF_STEP, MFM_RUNFLEX_IN_BAD_RUNS: as the burst POCSAG stage's,
 *                checked before anything of the payload is read.
 */
#define MFM_RUNFLEX_OVER_RUNS 1u
#define MFM_RUNFLEX_OVER_EVENTS 2u
#define MFM_RUNFLEX_IN_RUNRS 1u
#define MFM_RUNFLEX_IN_OUT_OF_STEP 2u
#define MFM_RUNFLEX_IN_BAD_RUNS 4u

struct mfm_runflex_event {      /* 104 bytes: struct mfm_flex_event, then the run and the stretch */
    uint32_t type;              /* MFM_FLEX_EV_* */
    uint32_t channel;
    uint64_t sample;            /* stretch-relative index of the resampled sample that completed the event */
    uint64_t sync_sample;       /* FRAME: stretch-relative sample of the last FIW bit */
    uint32_t coding;            /* as mfm_flex_event, field for field */
    uint32_t baud;
    uint32_t eye;
    uint32_t a;
    uint32_t b;
    uint32_t inv_a;
    uint32_t fiw_raw;
    uint32_t fiw;
    uint32_t fiw_rc;
    int32_t sample_range;
    int32_t sample_delta;
    uint32_t cycle;
    uint32_t frame;
    uint32_t frame_index;       /* FRAME: index of this frame's words in the call's list of frames */
    uint32_t nr_phases;
    uint32_t reserved;          /* 0 */
    uint32_t run;               /* index, in this call's run list, of the run that holds `sample` */
    uint32_t reserved2;         /* 0 */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
};

struct mfm_runflex; /* opaque */

struct mfm_runflex_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst resampler's capacities (mfm_runrs_get_capacity) */
    uint32_t max_out_samples;
    uint32_t max_events;        /* per call, all channels; 0 = max_out_samples / 1105 + max_runs, cannot overflow */
    uint32_t max_frames;        /* per call, all channels; 0 = max_out_samples / 29985 + max_runs, cannot overflow */
    uint32_t flags;             /* 0 */
};

int mfm_runflex_create(struct mfm_runflex **pf, const struct mfm_runflex_config *cfg);
void mfm_runflex_destroy(struct mfm_runflex **pf);
/*
 * Decode the runs of one burst resampler call: d_runs, d_payload and d_totals are what mfm_runrs_device_view returned.
 * Work is queued on `stream` (the resampler call's, or one ordered behind it); no host synchronisation and no count read on
 * the host: launches are sized from the capacities fixed at create, surplus workgroups return after reading the totals.  The
 * three arrays are read until the queued work has run.
 */
int mfm_runflex_process_device(struct mfm_runflex *f, const struct mfm_runrs_run *d_runs, const int16_t *d_payload,
                               const uint64_t *d_totals, void *stream);
/*
 * Wait for the last call and copy its events and the words of its frames (the copies are sized by the call's counts).
 * MFM_E_NOMEM when either array is too small (nothing copied, *nr_events / *nr_frames = needed); MFM_E_STATE with a message
 * when the call was refused (nothing copied, the state did not move: the same input in a call that is right is right again).
 */
int mfm_runflex_fetch(struct mfm_runflex *f, struct mfm_runflex_event *events, size_t max_events, size_t *nr_events,
                      struct mfm_flex_frame_words *frames, size_t max_frames, size_t *nr_frames);
/* For consumers that stay on the device: the last call's events, frames and d_totals[4], valid until the next call.  Each may
 * be NULL. */
int mfm_runflex_device_view(struct mfm_runflex *f, const struct mfm_runflex_event **d_events,
                            const struct mfm_flex_frame_words **d_frames, const uint64_t **d_totals);
struct mfm_runflex_state;
/* Wait for the last call and copy the per-channel state it left, state[nr_channels], and, unless ring is NULL, the rings,
 * ring[nr_channels][32768] (for tests and for moving a stream between objects: it is what the host twin carries). */
int mfm_runflex_fetch_state(struct mfm_runflex *f, struct mfm_runflex_state *state, int16_t *ring, size_t nr_channels);
/* The way back: waits for the queued work, validates every channel (csrc/mfm_runflex.h states the conditions) and writes the
 * state and the ring [nr_channels][32768] (both required) that the next process call reads.  A state that fails gets
 * MFM_E_INVAL with a message naming channel and field, and nothing is written.  The events and frames of the last call stay
 * readable. */
int mfm_runflex_store_state(struct mfm_runflex *f, const struct mfm_runflex_state *state, const int16_t *ring, size_t nr_channels);
/*
 * Stretch-end records, as the burst AIS stage's: off at create, one record per stretch over the whole stream, and nothing
 * else changes with the report on or off.
 *
 * Rule.  A stretch of channel c ends (a) in front of a run r that is c's first of a call that is not refused and has
 * MFM_RUNRS_BEGINS while the state the call started from has has_stretch == 1 (the record of that carried state, run = r);
 * (b) behind a run r of such a call whose successor r + 1 is also of channel c (the record of the state r's walk ended in,
 * run = r + 1); (c) at the end call: every channel with has_stretch == 1, channels ascending, run = 0xffffffff, after which
 * every state is all zero (the rings stay: a beginning run never reads one), the event and frame lists are empty, the totals
 * read { 0, 0, 0, 0 }, a continuing run is MFM_RUNFLEX_IN_OUT_OF_STEP and a beginning run is fine.  Records follow run-list
 * order, (a) in front of (b).  A refused call writes no record and moves no state.  Content does not depend on how the stream
 * was cut into calls.  A stretch of runs with nr_out == 0 alone gets a record with outs = 0 and mode SEARCH.  At most max_runs
 * records per process call and nr_channels per end call.
 *
 * mode 1 (SYNC1): the squelch closed between the end of the BS1 run at sample j and the frame information word; mode 2
 * (FRAME): between the FIW, whose last bit lay at j, and the last block symbol, and cycle / frame / coding / fiw are the FRAME
 * event's that never came.
 */
struct mfm_runflex_end {        /* 64 bytes */
    uint64_t stretch_window;    /* first window of the stretch: its first input sample is stretch_window * W */
    uint64_t outs;              /* resampled outputs of the whole stretch */
    uint64_t j;                 /* as mfm_runflex_state.j; 0 in SEARCH */
    uint32_t channel;
    uint32_t run;               /* index, in this call's run list, of the run that begins the next stretch; 0xffffffff: end call */
    uint32_t mode;              /* 0 SEARCH, 1 SYNC1, 2 FRAME */
    uint32_t eye;               /* SYNC1 / FRAME */
    uint32_t coding;            /* FRAME, as are fiw, cycle and frame */
    uint32_t fiw;
    uint32_t cycle;
    uint32_t frame;
    uint32_t reserved[2];       /* 0 */
};
/* Switch the report on or off.  Valid only before the first process call: MFM_E_STATE with a message afterwards. */
int mfm_runflex_set_end_report(struct mfm_runflex *f, int on);
/* (c) above, queued on `stream` like a process call.  MFM_E_STATE with a message when the report is off. */
int mfm_runflex_end_stretches_device(struct mfm_runflex *f, void *stream);
/* Wait for the last call (process or end) and copy its records.  MFM_E_NOMEM when max_ends is too small (nothing copied,
 * *nr_ends = needed); MFM_E_STATE with a message when the report is off, before the first call, or when the last call was
 * refused. */
int mfm_runflex_fetch_ends(struct mfm_runflex *f, struct mfm_runflex_end *ends, size_t max_ends, size_t *nr_ends);
/* The last call's records and d_end_totals[2] = { records, records with mode != 0 } on the device, valid until the next call.
 * Either may be NULL.  MFM_E_STATE with a message when the report is off. */
int mfm_runflex_ends_view(struct mfm_runflex *f, const struct mfm_runflex_end **d_ends, const uint64_t **d_end_totals);

/*
 * ---- Mueller-Muller clock recovery (BASELINE.json configs[3]: "mueller_muller slicer") -------------------------
 *   mm_init      pager/mueller_muller.c:10-33
 *   mm_process   pager/mueller_muller.c:41-115
 * for all channels of a PCM block at once, one loop state per channel, same float operations in the same order
 * (decisions are bit-identical to a build of the reference without FP contraction).  The reference's live decoder
 * does not call it (pager_pocsag.c has its own eye detectors); its consumer is pager/test/test_mueller_muller.c:
 * decisions[i] > 0 ? 0 : 1 shifted into a 32-bit register and compared with the POCSAG sync word.
 * As in the reference (:66-67) the index of a decision can reach nr_in: when in_stride > nr_in that sample is read
 * (the next block's first one, if the caller slices a longer buffer as the reference's test does), otherwise the
 * last sample stands in for it.
 */
struct mfm_mm; /* opaque */

struct mfm_mm_config {
    uint32_t abi_version; /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_in_samples; /* < 2^22: the reference's float sample position stays a whole number it holds exactly */
    float kw, km, samples_per_bit, error_min, error_max; /* mm_init's arguments; MFM_E_INVAL unless kw is finite,
                                                          * error_min <= error_max, error_min - |km| * 32768 >= 1 (a
                                                          * step cannot reach zero) and error_max + |km| * 32768 < 2^20 */
};

int mfm_mm_create(struct mfm_mm **pm, const struct mfm_mm_config *cfg);
void mfm_mm_destroy(struct mfm_mm **pm);
size_t mfm_mm_max_decisions(const struct mfm_mm *m);
/* decisions: [channel][*dec_stride] int16 (the samples picked, :71), counts: [channel] decisions of this call;
 * both in device memory, valid until the next call; queued on `stream`.  A row holds mfm_mm_max_decisions()
 * decisions (sized so that no configuration create accepts can exceed it); what lies behind them in the row is
 * scratch. */
int mfm_mm_process_device(struct mfm_mm *m, const int16_t *d_pcm, size_t in_stride, size_t nr_in, void *stream,
                          int16_t **d_decisions, size_t *dec_stride, uint32_t **d_counts);
/* Host convenience: synchronous; MFM_E_NOMEM if a channel produced more than dec_stride decisions. */
int mfm_mm_process_host(struct mfm_mm *m, const int16_t *pcm, size_t in_stride, size_t nr_in, int16_t *decisions,
                        size_t dec_stride, uint32_t *counts);

/*
 * ---- Burst Mueller-Muller stage: the burst resampler's runs through the clock recovery loop, on the device ----------------
 * The stage above (mfm_mm_*) on ragged runs instead of full rows: its input is what mfm_runrs_device_view returns (the run
 * list, the dense resampled payload, the totals), all read on the device, and its output is the decisions of every run: the
 * clock-recovered symbols of a burst, for a consumer of its own (a 2-FSK channel none of the burst decoders understands).
 *
 * Stretch means what it means for the burst resampler; this stage does not track windows.  Run r continues its channel's
 * stretch exactly when MFM_RUNRS_BEGINS is clear in runs[r].flags, otherwise it begins a new one.
 *
 * Rule.  The decisions of a stretch are the concatenation of the decisions of its runs, and they are exactly what a fresh
 * struct mueller_muller, initialised by mm_init(kw, km, samples_per_bit, error_min, error_max) (pager/mueller_muller.c:10-33),
 * returns when the stretch's resampled PCM is fed through mm_process (:41-115) in pieces of fewer than 2^22 samples each: the
 * same float operations in the same order, without contraction, bit-identical to oracle/pocsag_oracle.c's restatement.  The
 * reference's float sample position only ever holds whole numbers there (csrc/mfm_runmm.h), so the result does not depend on
 * the cutting and the stage keeps the position as an integer.  A decision is the sample picked (:71); its index is always
 * below the stretch's length so far, and no sample behind a run is read: there is no look-ahead column here.  The next
 * decision may lie beyond the end of a run, or of several short ones: the whole-sample distance still to skip travels in the
 * state (next_offset); a run shorter than it produces no decision and shortens it.  A run with nr_out == 0 changes nothing
 * and still begins or continues its stretch.  Decisions do not depend on how the stream was cut into calls.
 *
 * No lag.  A decision never looks ahead: it is reported by the call and run that holds its sample, and nothing is pending at
 * a stretch's end.
 *
 * State.  Per channel, on the device (struct mfm_runmm_state below, which the host twin carries too): the loop's w, m and
 * last_sample, the distance to the next decision, the outputs and the decisions of the stretch so far and the stretch's first
 * window.  Two state buffers are used in turn: a channel's first run reads the old state, its last run leaves the new one.  A
 * channel without a run in a call keeps its state.  Only a channel's first run of a call can continue a stretch, so every run
 * of a call is walked independently: the runs, not the arithmetic, are the stage's parallelism.
 *
 * Result.  It replaces the previous call's: one struct mfm_runmm_run per input run, in the resampler's order, and one dense
 * int16 payload of decisions in run order; dec_offset ascends and there are no gaps.  d_totals[4] = { runs, decisions,
 * overflow, input error }.  Order and offsets are deterministic: the walk of a run writes into a slot range given by a scan,
 * and the ranges are packed afterwards.
 *
 * Decision bound.  No step is shorter than s = floor(error_min - |km| * 32768) >= 1 samples (:86-96), so a run holds at most
 * nr_out / s + 1 decisions and a call at most the sum of that over its runs.
 *
 * Refused calls produce nothing, leave the per-channel state untouched and raise a flag that mfm_runmm_fetch reports as
 * MFM_E_STATE with a message:
 *   overflow     MFM_RUNMM_OVER_RUNS: more runs than max_runs; MFM_RUNMM_OVER_DECISIONS: the call's decision bound exceeds
 *                max_decisions (by the bound, not by the count, so "does it fit" does not depend on the signal)
 *   input error  MFM_RUNMM_IN_RUNRS, MFM_RUNMM_IN_OUT_OF_STEP, MFM_RUNMM_IN_BAD_RUNS: the burst POCSAG stage's conditions of
 *                the same names, checked before anything of the payload is read.
 *
 * Refusals at create (MFM_E_INVAL with a message, before a device is looked for): mfm_mm_create's conditions on the five
 * floats (kw finite, error_min <= error_max, samples_per_bit >= 1 - and below 2^20, it is the first step -, s >= 1, error_max
 * + |km| * 32768 < 2^20), capacities that are zero or reach 2^28 runs or 2^31 samples, flags other than 0.  max_in_samples has
 * no counterpart: the position is an integer per run.
 */
#define MFM_RUNMM_OVER_RUNS 1u
#define MFM_RUNMM_OVER_DECISIONS 2u
#define MFM_RUNMM_IN_RUNRS 1u
#define MFM_RUNMM_IN_OUT_OF_STEP 2u
#define MFM_RUNMM_IN_BAD_RUNS 4u

struct mfm_runmm_run {          /* 40 bytes */
    uint64_t first_window;      /* the resampler run's */
    uint64_t dec_offset;        /* in int16 elements of the decision payload */
    uint64_t first_dec;         /* index of the run's first decision within its stretch */
    uint32_t channel;
    uint32_t nr_dec;
    uint32_t flags;             /* MFM_RUNRS_BEGINS, copied */
    uint32_t reserved;          /* 0 */
};

struct mfm_runmm; /* opaque */

struct mfm_runmm_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst resampler's capacities (mfm_runrs_get_capacity) */
    uint32_t max_out_samples;
    uint32_t max_decisions;     /* per call, all channels; 0 = max_out_samples / s + max_runs, cannot overflow */
    uint32_t flags;             /* 0 */
    float kw, km, samples_per_bit, error_min, error_max; /* mm_init's arguments */
};

int mfm_runmm_create(struct mfm_runmm **pm, const struct mfm_runmm_config *cfg);
void mfm_runmm_destroy(struct mfm_runmm **pm);
/*
 * Recover the clock of the runs of one burst resampler call: d_runs, d_payload and d_totals are what mfm_runrs_device_view
 * returned.  Work is queued on `stream` (the resampler call's, or one ordered behind it); no host synchronisation and no count
 * read on the host: launches are sized from the capacities fixed at create, surplus workgroups return after reading the
 * totals.  The three arrays are read until the queued work has run.
 */
int mfm_runmm_process_device(struct mfm_runmm *m, const struct mfm_runrs_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                             void *stream);
/*
 * Wait for the last call, read its totals into *nr_runs and *nr_decisions and copy the used part of both arrays.  MFM_E_NOMEM
 * when max_runs or max_decisions is too small (nothing copied, the totals say what is needed); MFM_E_STATE with a message when
 * the call was refused (nothing copied, the state did not move: the same input in a call that is right is right again).
 */
int mfm_runmm_fetch(struct mfm_runmm *m, struct mfm_runmm_run *runs, size_t max_runs, size_t *nr_runs, int16_t *decisions,
                    size_t max_decisions, size_t *nr_decisions);
/* For consumers that stay on the device: the last call's runs, decisions and d_totals[4], valid until the next call.  Any of the
 * three may be NULL. */
int mfm_runmm_device_view(struct mfm_runmm *m, const struct mfm_runmm_run **d_runs, const int16_t **d_decisions, const uint64_t **d_totals);
struct mfm_runmm_state;
/* Wait for the last call and copy the per-channel state it left, state[nr_channels] (for tests and for moving a stream
 * between objects: it is what the host twin carries). */
int mfm_runmm_fetch_state(struct mfm_runmm *m, struct mfm_runmm_state *state, size_t nr_channels);
/* The way back: waits for the queued work, validates every channel (csrc/mfm_runmm.h states the conditions) and writes what
 * the next process call reads.  A state that fails gets MFM_E_INVAL with a message naming channel and field, and nothing is
 * written.  The result of the last call stays readable. */
int mfm_runmm_store_state(struct mfm_runmm *m, const struct mfm_runmm_state *state, size_t nr_channels);
/* The capacities fixed at create: max_runs as given, and max_decisions with the default filled in (max_out_samples / s +
 * max_runs where the configuration said 0).  What a stage behind this one sizes itself from.  Either pointer may be NULL. */
int mfm_runmm_get_capacity(struct mfm_runmm *m, uint32_t *max_runs, uint64_t *max_decisions);

/*
 * ---- Burst sync stage: sync words in the burst Mueller-Muller stage's decisions, on the device ------------------------------
 * The consumer of the stage above: its input is what mfm_runmm_device_view returns (the run records, the dense int16 decisions,
 * the totals), all read on the device, and its output is one bit per decision and one event wherever the last 32 bits of a
 * stretch are a sync word of a small table, or nearly one.  One pass says per stretch which word was seen, where and in which
 * polarity; the bits let a consumer cut the frames behind a sync out of 1/16 of the bytes.
 *
 * Stretch means what it means for the burst Mueller-Muller stage.  Run r continues its channel's stretch exactly when
 * MFM_RUNRS_BEGINS is clear in runs[r].flags, otherwise it begins a new one.
 *
 * Rule.  The reference's only consumer of mm_process, pager/test/test_mueller_muller.c:130-136, with a table and the
 * complement.  Per stretch a fresh register shr = 0; for every decision d of the stretch, in order, shr = (shr << 1) | bit,
 * where bit = !(d > 0) with MFM_RUNSYNC_BIT_NOT_POS (the reference's, :132) and bit = (d > 0) with MFM_RUNSYNC_BIT_POS.
 * MFM_RUNSYNC_BIT_NOT_POS is not the sign bit MFM_BITS_NEG takes: d == 0 is the one value where the two differ (bit 1 here, 0
 * there).  After decision number n (counted from 0 within the stretch) the lowest word index k that matches is looked for, the
 * word itself before its complement: words[k] matches when popcount(words[k] ^ shr) <= max_distance, and with
 * MFM_RUNSYNC_F_EITHER its complement when popcount(~words[k] ^ shr) <= max_distance.  max_distance <= 15 keeps a register from
 * matching a word and its complement at once.  A match is one event; there is at most one event per decision.  The reference
 * compares with "< 4": max_distance = 3.
 *
 * The register is tested from the stretch's first decision on, with zeros above the bits shifted in so far, exactly as the
 * reference's loop tests it: there is no warm-up of 32 decisions, and a word with leading zeros can match before 32 decisions
 * have passed.
 *
 * No lag.  Events do not depend on how the stream was cut into calls or runs; an event is reported by the call and run that
 * holds decision n.
 *
 * State.  Per channel, on the device (struct mfm_runsync_state below, which the host twin carries too): the register, the
 * decisions of the stretch so far and the stretch's first window.  Two state buffers are used in turn: a channel's first run of
 * a call reads the old state, its last run leaves the new one.  A channel without a run keeps its state.  A run with nr_dec == 0
 * changes nothing and still begins or continues its stretch.
 *
 * Result.  It replaces the previous call's.
 *   run records  one struct mfm_runsync_run per input run, in the Mueller-Muller stage's order
 *   bits         one bit per decision: decision j of a run is bit j % 32 of word word_offset + j / 32.  A run owns (nr_dec + 31) /
 *                32 words, ascending and without gaps; a run with nr_dec == 0 owns none; the bits at and above nr_dec in a run's
 *                last word are 0 - the convention of mfm_runrs_process_bits_device.  Capacity: max_decisions / 32 + max_runs words.
 *   events       struct mfm_runsync_event, dense, in run order and ascending in dec within a run; a run's events are contiguous
 *                (nr_events of them, behind those of the runs in front).  Order and offsets come from a scan, never from atomics.
 *   totals       d_totals[4] = { runs, events, overflow, input error }
 *
 * Refused calls produce nothing, leave the per-channel state untouched and raise a flag that mfm_runsync_fetch reports as
 * MFM_E_STATE with a message:
 *   overflow     MFM_RUNSYNC_OVER_RUNS: more runs than max_runs; MFM_RUNSYNC_OVER_DECISIONS: more decisions than max_decisions;
 *                MFM_RUNSYNC_OVER_EVENTS: the call's events exceed a caller-chosen max_events - by the count, which is known
 *                before an event is placed, so nothing is written past the capacity
 *   input error  MFM_RUNSYNC_IN_RUNMM: the Mueller-Muller stage's totals carry overflow or an input error;
 *                MFM_RUNSYNC_IN_OUT_OF_STEP: a continuing run that is not its channel's first of the call, or whose first_dec is
 *                not the state's decs, or whose channel has no stretch; MFM_RUNSYNC_IN_BAD_RUNS: a channel >= nr_channels,
 *                channels not ascending, a beginning run whose first_dec is not 0, a dec_offset that is not the running sum of
 *                nr_dec or a range that ends past the totals.  All of these are checked before a decision is read.
 *
 * Refusals at create (MFM_E_INVAL with a message, before a device is looked for): nr_words of 0 or above 8, max_distance above
 * 15, an unknown bit_rule, flags other than MFM_RUNSYNC_F_EITHER, capacities that are zero or reach 2^28 runs or 2^31 decisions
 * or events.
 */
#define MFM_RUNSYNC_BIT_NOT_POS 0u     /* bit = !(d > 0): test_mueller_muller.c:132 */
#define MFM_RUNSYNC_BIT_POS 1u         /* bit = (d > 0) */
#define MFM_RUNSYNC_F_EITHER 1u        /* mfm_runsync_config.flags: the complement of every word is tested too */
#define MFM_RUNSYNC_OVER_RUNS 1u
#define MFM_RUNSYNC_OVER_DECISIONS 2u
#define MFM_RUNSYNC_OVER_EVENTS 4u
#define MFM_RUNSYNC_IN_RUNMM 1u
#define MFM_RUNSYNC_IN_OUT_OF_STEP 2u
#define MFM_RUNSYNC_IN_BAD_RUNS 4u

struct mfm_runsync_run {        /* 40 bytes */
    uint64_t first_window;      /* the Mueller-Muller run's */
    uint64_t word_offset;       /* in 32-bit words of the bits */
    uint64_t first_dec;         /* index of the run's first decision within its stretch */
    uint32_t channel;
    uint32_t nr_dec;
    uint32_t flags;             /* MFM_RUNRS_BEGINS, copied */
    uint32_t nr_events;
};

struct mfm_runsync_event {      /* 32 bytes */
    uint64_t dec;               /* the decision that completed the word, counted within its stretch */
    uint32_t channel;
    uint32_t run;               /* index in this call's run list */
    uint32_t seen;              /* the register */
    uint32_t word_index;
    uint32_t distance;          /* bits that differ from the word, or from its complement */
    uint32_t inverted;          /* 0: the word, 1: its complement */
};

/* the per-channel state, on the device and in the host twin: all zero at the start of a stream.  What a stored state must
 * satisfy: csrc/mfm_runsync.h (mfm_runsync_state_check) */
struct mfm_runsync_state {      /* 24 bytes */
    uint64_t stretch_window;    /* first window of the stretch */
    uint64_t decs;              /* decisions of the stretch so far */
    uint32_t shr;               /* the register after the last of them */
    uint32_t has_stretch;       /* 0: nothing to continue */
};

struct mfm_runsync; /* opaque */

struct mfm_runsync_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst Mueller-Muller stage's capacities (mfm_runmm_get_capacity) */
    uint32_t max_decisions;
    uint32_t max_events;        /* per call, all channels; 0 = max_decisions, cannot overflow: at most one event per decision */
    uint32_t nr_words;          /* 1 .. 8 */
    uint32_t words[8];
    uint32_t max_distance;      /* 0 .. 15 */
    uint32_t bit_rule;          /* MFM_RUNSYNC_BIT_NOT_POS or MFM_RUNSYNC_BIT_POS */
    uint32_t flags;             /* 0 or MFM_RUNSYNC_F_EITHER */
};

int mfm_runsync_create(struct mfm_runsync **ps, const struct mfm_runsync_config *cfg);
void mfm_runsync_destroy(struct mfm_runsync **ps);
/*
 * Search the decisions of one burst Mueller-Muller call: d_runs, d_decisions and d_totals are what mfm_runmm_device_view
 * returned.  Work is queued on `stream` (the Mueller-Muller call's, or one ordered behind it); no host synchronisation and no
 * count read on the host: launches are sized from the capacities fixed at create, surplus workgroups return after reading the
 * totals.  The three arrays are read until the queued work has run.
 */
int mfm_runsync_process_device(struct mfm_runsync *s, const struct mfm_runmm_run *d_runs, const int16_t *d_decisions, const uint64_t *d_totals,
                               void *stream);
/*
 * Wait for the last call, read its totals and copy the used part of the three arrays.  MFM_E_NOMEM when max_runs, max_words or
 * max_events is too small (nothing copied, *nr_runs, *nr_words and *nr_events say what is needed); MFM_E_STATE with a message
 * when the call was refused (nothing copied, the state did not move: the same input in a call that is right is right again).
 */
int mfm_runsync_fetch(struct mfm_runsync *s, struct mfm_runsync_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits, size_t max_words,
                      size_t *nr_words, struct mfm_runsync_event *events, size_t max_events, size_t *nr_events);
/* For consumers that stay on the device: the last call's run records, bits, events and d_totals[4], valid until the next call.
 * Any of the four may be NULL. */
int mfm_runsync_device_view(struct mfm_runsync *s, const struct mfm_runsync_run **d_runs, const uint32_t **d_bits,
                            const struct mfm_runsync_event **d_events, const uint64_t **d_totals);
/* The capacities fixed at create: runs, bit words (max_decisions / 32 + max_runs) and events.  Any pointer may be NULL. */
int mfm_runsync_get_capacity(struct mfm_runsync *s, uint32_t *max_runs, uint64_t *max_words, uint64_t *max_events);
/* Wait for the last call and copy the per-channel state it left, state[nr_channels]: what the host twin carries. */
int mfm_runsync_fetch_state(struct mfm_runsync *s, struct mfm_runsync_state *state, size_t nr_channels);
/* The way back: waits for the queued work, validates every channel (csrc/mfm_runsync.h states the conditions) and writes what
 * the next process call reads.  A state that fails gets MFM_E_INVAL with a message naming channel and field, and nothing is
 * written.  The result of the last call stays readable. */
int mfm_runsync_store_state(struct mfm_runsync *s, const struct mfm_runsync_state *state, size_t nr_channels);

/*
 * ---- Burst batch stage: POCSAG batches behind the burst sync stage's events, on the device ----------------------------------
 * The consumer of the stage above: its input is what mfm_runsync_device_view returns (the run records, the bit words, the
 * events, the totals), all read on the device.  Behind a sync event it cuts batches of 16 codewords out of the bit words, runs
 * BCH(31,21) on them and follows sync kept / sync lost exactly as pager/pager_pocsag.c:468-538 does at one sample per bit; the
 * events carry the types the host pager consumes (MFM_POCSAG_EV_*), so the clock-recovery branch of the burst chain reaches
 * pages at any symbol rate the Mueller-Muller stage follows.
 *
 * Rule.  Per stretch (the sync stage's: MFM_RUNRS_BEGINS decides where one begins).  Let b[n] be the sync stage's bit of
 * decision n of the stretch.  A fresh automaton starts every stretch in SEARCH with mark = 0.
 *   SEARCH   the stretch's first sync event with dec >= mark whose word is enabled (word_mask bit word_index set, or word_mask
 *            == 0), at decision n0: FOUND with dec = n0, aux = seen, word_index, the distance in nr_ok, inverted.  The automaton
 *            keeps word_index and inverted for this transmission; mark = p = n0 + 1; RECEIVE.
 *   RECEIVE  word z (0 .. 15) of the batch is filled LSB first (the reference's bit << bit_count): bit i of word z is
 *            b[p + 32 z + i] ^ inverted, the sync stage's own packing.  When decision p + 511 exists: BATCH with dec = p + 511
 *            and raw[16], corrected[z] = BCH(raw[z] & 0x7fffffff), fail_mask (bit z: word z is uncorrectable) and nr_ok (the
 *            words in front of the first failure) - struct mfm_pocsag_event's convention.  SLOT.
 *   SLOT     the 32 bits of decisions p + 512 .. p + 543 as a register, shifted in MSB first as the sync stage's, complemented
 *            when inverted: seen.  popcount(seen ^ words[word_index]) <= keep_distance (the reference: 4): KEPT with dec = p +
 *            543 and aux = seen, p += 544, RECEIVE.  Otherwise LOST with the same dec and aux, mark = p + 575, SEARCH: the next
 *            sync lies wholly behind the failed slot, as the reference searches from scratch after
 *            _pager_pocsag_baud_search_reset, and the next FOUND decides the polarity anew.
 * Sync events seen in RECEIVE or SLOT are ignored.  A batch or slot still being collected when its stretch ends is dropped
 * without an event.  A run with nr_dec == 0 changes nothing and still begins or continues its stretch.
 *
 * No lag.  Events do not depend on how the stream was cut into calls or runs; an event is reported by the call and run that
 * holds decision dec.
 *
 * State.  Per channel, on the device (struct mfm_runbatch_state below, which the host twin carries too), two buffers used in
 * turn.  In RECEIVE and SLOT kept holds the bits of the decisions [mark, decs), nr_kept = decs - mark < 544 of them, LSB first
 * and zero above: the previous call's bit words are gone by then.  In SEARCH nr_kept, kept, word_index and inverted are 0; a
 * channel without a stretch is all zero.  The form is canonical: device and twin states compare as bytes.
 *
 * Result.  It replaces the previous call's: struct mfm_runbatch_event, dense, in run order and ascending in dec within a run,
 * placed by a scan and never by atomics; d_totals[4] = { events, runs, overflow, input error }.  A run of nr_dec decisions has
 * at most 3 (nr_dec / 544) + 5 events (derived in csrc/mfm_runbatch.h), so the default max_events cannot overflow.
 *
 * Refused calls produce nothing, leave every state untouched and raise a flag that mfm_runbatch_fetch reports as MFM_E_STATE
 * with a message:
 *   overflow     MFM_RUNBATCH_OVER_RUNS: more runs than max_runs; MFM_RUNBATCH_OVER_EVENTS: the call's events exceed a
 *                caller-chosen max_events - by the count, which is known before an event is placed
 *   input error  MFM_RUNBATCH_IN_RUNSYNC: the sync stage's totals carry a flag; MFM_RUNBATCH_IN_OUT_OF_STEP and _IN_BAD_RUNS: the
 *                burst stages' shared run checks, a word_offset that is not the running sum of the runs' words, or runs
 *                that hold more bit words or event slots than max_decisions and max_runs allow; MFM_RUNBATCH_IN_BAD_EVENTS: an event whose dec lies outside its run, events not
 *                ascending, word_index >= nr_words, inverted > 1, or the sum of nr_events past the sync stage's totals.  All of
 *                these are checked before any state moves.
 *
 * Refusals at create (MFM_E_INVAL with a message, before a device is looked for): nr_words of 0 or above 8, keep_distance above
 * 15, word_mask bits at or above nr_words, flags other than 0, capacities that are zero or reach 2^28 runs or 2^31 decisions or
 * events.
 */
#define MFM_RUNBATCH_SEARCH 0u         /* mfm_runbatch_state.mode */
#define MFM_RUNBATCH_RECEIVE 1u
#define MFM_RUNBATCH_SLOT 2u
#define MFM_RUNBATCH_OVER_RUNS 1u
#define MFM_RUNBATCH_OVER_EVENTS 2u
#define MFM_RUNBATCH_IN_RUNSYNC 1u
#define MFM_RUNBATCH_IN_OUT_OF_STEP 2u
#define MFM_RUNBATCH_IN_BAD_RUNS 4u
#define MFM_RUNBATCH_IN_BAD_EVENTS 8u

struct mfm_runbatch_event {     /* 176 bytes */
    uint32_t type;              /* MFM_POCSAG_EV_* */
    uint32_t channel;
    uint32_t run;               /* index in this call's run list */
    uint32_t aux;               /* SYNC_FOUND: the sync stage's register; SYNC_KEPT / SYNC_LOST: the 32 bits seen in the slot, upright */
    uint32_t word_index;        /* the transmission's sync word */
    uint32_t inverted;          /* ... and polarity */
    uint32_t nr_ok;             /* SYNC_FOUND: the sync event's distance; BATCH: words in front of the first BCH failure (16: all) */
    uint32_t fail_mask;         /* BATCH: bit z set when word z is uncorrectable */
    uint64_t stretch_window;    /* first window of the stretch */
    uint64_t dec;               /* the decision that completed the event, counted within its stretch */
    uint32_t raw[16];           /* BATCH: the words as collected, upright */
    uint32_t corrected[16];     /* BATCH: (raw & 0x7fffffff) after BCH correction */
};

/* the per-channel state, on the device and in the host twin: all zero at the start of a stream.  What a stored state must
 * satisfy: csrc/mfm_runbatch.h (mfm_runbatch_state_check) */
struct mfm_runbatch_state {     /* 120 bytes */
    uint64_t stretch_window;    /* first window of the stretch */
    uint64_t decs;              /* decisions of the stretch so far */
    uint64_t mark;              /* SEARCH: the first decision a sync may end on; RECEIVE / SLOT: p, the frame's first decision */
    uint32_t has_stretch;       /* 0: nothing to continue */
    uint32_t mode;              /* MFM_RUNBATCH_SEARCH / _RECEIVE / _SLOT */
    uint32_t word_index;
    uint32_t inverted;
    uint32_t nr_kept;           /* decs - mark in RECEIVE and SLOT, else 0 */
    uint32_t reserved;          /* 0 */
    uint32_t kept[17];          /* the bits of the decisions [mark, decs), LSB first, 0 above */
    uint32_t reserved2;         /* 0 */
};

struct mfm_runbatch; /* opaque */

struct mfm_runbatch_config {
    uint32_t abi_version;       /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t nr_channels;
    uint32_t max_runs;          /* the burst sync stage's (its max_runs and max_decisions) */
    uint32_t max_decisions;
    uint32_t max_events;        /* per call, all channels; 0 = 3 * (max_decisions / 544) + 5 * max_runs, cannot overflow */
    uint32_t nr_words;          /* 1 .. 8: the sync stage's table */
    uint32_t words[8];
    uint32_t word_mask;         /* the words that start a transmission; 0 = all */
    uint32_t keep_distance;     /* 0 .. 15; the reference: 4 */
    uint32_t flags;             /* 0 */
};

int mfm_runbatch_create(struct mfm_runbatch **pb, const struct mfm_runbatch_config *cfg);
void mfm_runbatch_destroy(struct mfm_runbatch **pb);
/*
 * Follow the sync events of one burst sync call: the four arrays are what mfm_runsync_device_view returned.  Work is queued on
 * `stream` (the sync call's, or one ordered behind it); no host synchronisation and no count read on the host: launches are
 * sized from the capacities fixed at create, surplus workgroups return after reading the totals.  The arrays are read until the
 * queued work has run.
 */
int mfm_runbatch_process_device(struct mfm_runbatch *b, const struct mfm_runsync_run *d_runs, const uint32_t *d_bits,
                                const struct mfm_runsync_event *d_events, const uint64_t *d_totals, void *stream);
/*
 * Wait for the last call, read its totals and copy its events.  MFM_E_NOMEM when max_events is too small (nothing copied,
 * *nr_events says what is needed); MFM_E_STATE with a message when the call was refused (nothing copied, no state moved: the
 * same input in a call that is right is right again).
 */
int mfm_runbatch_fetch(struct mfm_runbatch *b, struct mfm_runbatch_event *events, size_t max_events, size_t *nr_events);
/* For consumers that stay on the device: the last call's events and d_totals[4], valid until the next call.  Either may be
 * NULL. */
int mfm_runbatch_device_view(struct mfm_runbatch *b, const struct mfm_runbatch_event **d_events, const uint64_t **d_totals);
/* The capacities fixed at create: runs and events (the default filled in).  Either pointer may be NULL. */
int mfm_runbatch_get_capacity(struct mfm_runbatch *b, uint32_t *max_runs, uint64_t *max_events);
/* Wait for the last call and copy the per-channel state it left, state[nr_channels]: what the host twin carries. */
int mfm_runbatch_fetch_state(struct mfm_runbatch *b, struct mfm_runbatch_state *state, size_t nr_channels);
/* The way back: waits for the queued work, validates every channel (csrc/mfm_runbatch.h states the conditions) and writes what
 * the next process call reads.  A state that fails gets MFM_E_INVAL with a message naming channel and field, and nothing is
 * written.  The result of the last call stays readable. */
int mfm_runbatch_store_state(struct mfm_runbatch *b, const struct mfm_runbatch_state *state, size_t nr_channels);

/* bch_code_decode (pager/bch_code.c:307-398) on n words in place; rc[i] = its return value (0 or 1). */
int mfm_bch3121_decode_device(uint32_t *d_words, uint8_t *d_rc, size_t n, int device, void *stream);
int mfm_bch3121_decode_host(uint32_t *words, uint8_t *rc, size_t n, int device);

/*
 * ---- Floating-point IQ path (BASELINE.json configs[4] "fp32 vs int16 IQ path") ---------
 * The reference has no floating-point channel path.  This is multifm's per-channel loop
 *
 *   _demod_fir_prepare               multifm/demod.c:204-269       taps = (gain * cexp(j f_offs i)) * h[i], NOT quantised
 *   direct_fir_process               filter/direct_fir.c:328-453   complex FIR, decimation D, derotation by
 *                                                                  cexp(-j 2 pi off D n / fs) (closed form of :151-172)
 *   multifm_fm_demod_process         multifm/fm_demod.c:36-85      s = o[n] conj(o[n-1]), fast_atan2f, phi/pi*16384
 *
 * on float32 interleaved IQ (any scale) in fp32 arithmetic.  Parity target: oracle/f32_oracle.c (the same in fp64),
 * 1e-5 relative (tests/test_f32_path.py).  PCM comes out as float and, truncated like fm_demod.c:72, as int16 laid
 * out like the integer engine's ([channel][stride]) so that mfm_resampler_* / mfm_pocsag_* take it unchanged.
 * All channels of an engine share one filter length (>= the decimation).
 */
struct mfm_f32_engine; /* opaque */

#define MFM_F32_WANT_IQ 1u /* also keep the derotated filtered samples (signalDebugFile analogue) */
#define MFM_F32_PACKED_FMA 2u /* multiply with v_pk_fma_f32 instead of the fp32 matrix instructions (A/B timing) */
#define MFM_F32_TILE_KERNEL 4u /* the round-1 kernel, one workgroup per tile, instead of the persistent one (A/B timing) */

struct mfm_f32_config {
    uint32_t abi_version; /* MFM_ABI_VERSION */
    int32_t device;
    uint32_t sample_rate_hz;
    uint32_t decimation;
    uint32_t max_block_samples; /* most IQ samples one process call may carry */
    uint32_t flags;             /* MFM_F32_* */
};

struct mfm_f32_block {
    float *d_pcm_f32;     /* device, [channel][stride] */
    int16_t *d_pcm_i16;   /* device, [channel][stride] */
    float *d_iq_f32;      /* device, [channel][stride] (re, im) pairs, NULL without MFM_F32_WANT_IQ */
    size_t stride;        /* elements between channels */
    size_t nr_out;        /* outputs per channel of this call */
    uint32_t nr_channels;
    uint32_t reserved;
};

int mfm_f32_create(struct mfm_f32_engine **pe, const struct mfm_f32_config *cfg);
/* same arguments as demod_thread_new's offset / taps / gain (multifm/demod.h:104-110); returns the channel index */
int mfm_f32_add_channel(struct mfm_f32_engine *e, int32_t offset_hz, const double *lpf_taps, size_t nr_taps,
                        double gain);
int mfm_f32_commit(struct mfm_f32_engine *e);
void mfm_f32_destroy(struct mfm_f32_engine **pe);
size_t mfm_f32_max_out(const struct mfm_f32_engine *e);
/* nr_samples float IQ pairs in device memory; work is queued on `stream`, the block's pointers are valid until the
 * next call.  The stream position (unconsumed samples, output phase, discriminator history) carries over. */
int mfm_f32_process_device(struct mfm_f32_engine *e, const float *d_iq, size_t nr_samples, void *stream,
                           struct mfm_f32_block *out);
/* Host convenience (tests): synchronous, any of the three outputs may be NULL; out_stride in elements. */
int mfm_f32_process_host(struct mfm_f32_engine *e, const float *iq, size_t nr_samples, float *pcm_f32,
                         int16_t *pcm_i16, float *iq_f32, size_t out_stride, size_t *nr_out);

/*
 * Host twins of the kernel's scalar numerics (compiled from the same header the kernel uses).
 * They exist so the test-suite can check, on the CPU, that the device formulas reproduce the
 * reference's expressions bit for bit; they are not a compute path.
 */
int32_t mfm_hosttwin_discriminate(int32_t s_re, int32_t s_im);
void mfm_hosttwin_discriminate_batch(const int32_t *s_re, const int32_t *s_im, size_t n, int16_t *out);
int16_t mfm_hosttwin_r14(int32_t a);
/* out[i] = pcm of the non-negative angle whose float bit pattern is first_bits + i */
void mfm_hosttwin_pcm_range(uint32_t first_bits, uint32_t count, int16_t *out);
void mfm_hosttwin_atan_table(float tbl[257]);
int mfm_hosttwin_atan_table_ok(void); /* 1 if the generated table matches the pinned hash */
/* The discriminator (multifm/fm_demod.c:68-72 on fast_atan2f.c:101-174) exactly as the channel kernel of `variant`
 * (mfm_stats::kernel_variant: 0, 1, 2) computes it ON THE DEVICE, for caller-supplied products s = q conj(prev): the three
 * kernels carry three renderings of it (scalar, packed, four at a time), and tests run the hard cases of its division
 * through each (tools/div_proof.c).  Host arrays in and out; not a compute path. */
int mfm_devtest_discriminate(int variant, const int32_t *s_re, const int32_t *s_im, size_t n, int16_t *pcm_out, int device);
/* What v_rcp_f32 returns on `device` for all 2^23 binary32 significands, as a hash (+ how many reciprocals are one ulp low /
 * correctly rounded / one ulp high / anything else), and optionally the discriminator's division against the IEEE quotient
 * on 2^28 significand pairs.  mfm_engine_commit() compares the hash with MFM_RCP_TABLE_HASH_GFX950 - the table the
 * division's correctness proof (tools/div_proof.c) enumerated - once per device, and falls back to the sweep when it
 * differs: a device with another reciprocal table is accepted only if not one quotient is off. */
#define MFM_RCP_TABLE_HASH_GFX950 0x706d94bc005bcc1aull /* (read off an MI355X: tests/test_gpu_parity.py checks it there) */
int mfm_devtest_rcp_table(int device, uint64_t *hash, uint64_t counts[4], uint64_t *sweep_bad, uint64_t *sweep_tried);
/* The kernel form mfm_engine_commit() would choose for this engine's channels, planned on the host without a device: the
 * fields kernel_variant, slice_channels, taps_resident, outputs_per_tile, k_steps, tap_hi_mask, lds_bytes, rot_exact_channels
 * and rot_fast_slices as mfm_engine_get_stats() reports them after commit, the others 0.  Before commit only; a plan that
 * commit would refuse returns the same error. */
int mfm_hosttwin_kernel_form(struct mfm_engine *e, struct mfm_stats *st);
/* the device's table-driven BCH(31,21) decode (syndrome bytes -> 1024-entry flip table), on the host */
int mfm_hosttwin_bch3121_decode(uint32_t *word);
/* host twin of the splice that stands in the place of the slicers on the sign-bit path (csrc/mfm_bits.h, the same inline the
 * kernel runs per word): bits [off0, off0 + nr_bits) of `window` from bits [0, nr_bits) of `src`, bits below off0 kept, the rest
 * of the last touched word zero, no word behind it touched */
void mfm_hosttwin_splice_bits(uint32_t *window, uint64_t off0, const uint32_t *src, uint64_t nr_bits);
/* host twins of the level stage's arithmetic (csrc/mfm_level.h, the inlines its kernels run): the three sums of one window of
 * nr_samples samples at x (form MFM_LEVEL_PCM: nr_samples int16; MFM_LEVEL_IQ: 2 * nr_samples, and *diff_energy = 0), prev = the
 * sample in front of x[0]; and one step of the squelch on *open / *bad (sense MFM_LEVEL_OPEN_*), which returns the new *open */
void mfm_hosttwin_level_window(const int16_t *x, size_t nr_samples, uint32_t form, int16_t prev, uint64_t *energy, uint64_t *diff_energy,
                               uint32_t *peak);
uint32_t mfm_hosttwin_squelch_step(uint32_t sense, uint64_t open_thr, uint64_t close_thr, uint32_t hang_windows, uint64_t metric,
                                   uint32_t *open, uint32_t *bad);
/* host twin of the adaptive squelch (mfm_level_set_adaptive; csrc/mfm_level.h, the inlines the kernel runs) for ONE channel:
 * metric[0 .. nr_windows) are the windows from the first one after create or seek on; floor[k] and open[k] (either may be NULL)
 * get window k's floor and the squelch state after it.  The floor is formed by its definition, window by window.  Nothing is
 * checked and nothing is reported: the caller passes a setting mfm_level_set_adaptive would accept (with metric or the setting NULL,
 * or floor_windows 0, the call returns with floor and open untouched). */
void mfm_hosttwin_level_adaptive(const uint64_t *metric, size_t nr_windows, uint32_t sense, uint64_t open_thr, uint64_t close_thr,
                                 uint32_t hang_windows, const struct mfm_level_adaptive *a, uint64_t *floor, uint32_t *open);
/* host twin of one call of the gate stage (csrc/mfm_gate.h, the arithmetic its kernels run: the window cut of a call, run
 * formation, offsets), on the CPU with no device: pos = samples per channel consumed before the call, rows [channel][in_stride],
 * carry [channel][W * elems_per_sample] read and then updated, records [channel][record_stride].  0 with runs and payload filled;
 * MFM_E_INVAL for a wrong nr_windows, MFM_E_STATE for a record with a wrong .window, MFM_E_NOMEM when max_runs or max_elems is
 * too small (*nr_runs and *nr_elems say what is needed); on any error nothing is written, the carry included. */
int mfm_hosttwin_gate_call(uint32_t nr_channels, uint32_t window_samples, uint32_t elems_per_sample, uint64_t pos, const int16_t *rows,
                           size_t in_stride, size_t nr_in, int16_t *carry, const struct mfm_level_record *records, size_t record_stride,
                           size_t nr_windows, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                           size_t *nr_elems);
/* host twin of one call (flush == 0) or of the flush (flush != 0: nr_in and nr_windows 0, rows and records unused) of a
 * gate with pre-roll, with the state the stage carries made explicit: history int16 [nr_channels][(P + 1) * W *
 * elems_per_sample] (linear, oldest first; the last min(K, P) complete windows and the unfinished one, K = pos / W),
 * open_bits uint64 [nr_channels] (bit i = the open bit of record K - P + i, 0 where no such record exists), both zero at
 * pos 0 and updated in place, and pos.  Error rules of mfm_hosttwin_gate_call: on any error nothing is written, history
 * and bits included.  With preroll_windows = 0 it is mfm_hosttwin_gate_call to the byte (history = carry). */
int mfm_hosttwin_gate_call_preroll(uint32_t nr_channels, uint32_t window_samples, uint32_t elems_per_sample, uint32_t preroll_windows,
                                   uint64_t pos, int flush, const int16_t *rows, size_t in_stride, size_t nr_in, int16_t *history,
                                   uint64_t *open_bits, const struct mfm_level_record *records, size_t record_stride, size_t nr_windows,
                                   struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                                   size_t *nr_elems);
/* host twin of the burst resampler's closed form (csrc/mfm_runrs.h, what its plan and state kernels run), n cases at once:
 * a run of nr_samples[i] samples met with phase[i] (< interpolate) and pending[i] (<= plen) unconsumed samples produces
 * nr_out[i] outputs and leaves phase_out[i] and pending_out[i].  MFM_E_INVAL for a ratio the stage refuses or a case out of
 * range. */
int mfm_hosttwin_runrs_plan(uint32_t interpolate, uint32_t decimate, uint32_t plen, const uint32_t *phase, const uint32_t *pending,
                            const uint64_t *nr_samples, size_t n, uint64_t *nr_out, uint32_t *phase_out, uint32_t *pending_out);
/* the per-channel state of the burst resampler, on the device and in the host twin: zero-filled except expected = ~0 (no
 * stretch) at the start of a stream.  What a stored state must satisfy: csrc/mfm_runrs.h (mfm_runrs_state_check) */
struct mfm_runrs_state {        /* 24 bytes */
    uint64_t expected;          /* window number that continues the channel's stretch */
    uint64_t outs;              /* outputs of the stretch so far */
    uint32_t phase;
    uint32_t pending;           /* samples in the channel's part of `pending` */
};
/* host twin of one mfm_runrs_process_device call, no device needed: gate_runs / gate_payload are one gate call's result
 * (nr_gate_runs, nr_gate_elems: its totals), state [nr_channels] and pending [nr_channels][plen] are updated in place, plen =
 * ((nr_coeffs + interpolate - 1) / interpolate + 3) & ~3.  MFM_E_INVAL for what create refuses and for a run list that is not a
 * gate's, MFM_E_NOMEM when max_runs or max_elems is too small (*nr_runs / *nr_elems say what is needed); on any error nothing
 * is written, the state included.  It is the twin of mfm_runrs_process_view_device as well: nr_gate_elems is a bound of the
 * payload ranges only and there is no capacity test, so a local route's run list (mfm_runroute_create_local) goes in with the
 * gate's payload and the gate's total as nr_gate_elems. */
int mfm_hosttwin_runrs_call(uint32_t nr_channels, uint32_t window_samples, uint32_t interpolate, uint32_t decimate, uint32_t invert,
                            const int16_t *coeffs, size_t nr_coeffs, struct mfm_runrs_state *state, int16_t *pending,
                            const struct mfm_gate_run *gate_runs, size_t nr_gate_runs, const int16_t *gate_payload, size_t nr_gate_elems,
                            struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                            size_t *nr_elems);
/* host twin of one mfm_runrs_process_bits_device call: as mfm_hosttwin_runrs_call on the same state (the two may alternate on
 * it), with the predicate words of `polarity` in `bits` and out_offset, max_words and *nr_words in 32-bit words.  It runs the
 * inlines the kernels run (csrc/mfm_runrs.h). */
int mfm_hosttwin_runrs_call_bits(uint32_t nr_channels, uint32_t window_samples, uint32_t interpolate, uint32_t decimate, uint32_t invert,
                                 uint32_t polarity, const int16_t *coeffs, size_t nr_coeffs, struct mfm_runrs_state *state, int16_t *pending,
                                 const struct mfm_gate_run *gate_runs, size_t nr_gate_runs, const int16_t *gate_payload,
                                 size_t nr_gate_elems, struct mfm_runrs_run *runs, size_t max_runs, size_t *nr_runs, uint32_t *bits,
                                 size_t max_words, size_t *nr_words);
/* the per-channel state of the burst resampler's DC blocker (filter/dc_blocker.h's fields), on the device and in the host
 * twin: all zero at the start of a stream */
struct mfm_runrs_dc_state {     /* 16 bytes */
    int32_t x_n_1, y_n_1, acc;
    uint32_t reserved;          /* 0 */
};
/* host twin of the DC blocker of a burst resampler with mfm_runrs_set_dc_block(rr, 1, pole), no device needed: applies the rule
 * in place to the result of one mfm_hosttwin_runrs_call (runs, nr_runs, payload, nr_elems = its *nr_elems); dc [nr_channels] is
 * updated in place.  It runs the inlines the kernel runs (csrc/mfm_runrs_dc.h).  MFM_E_INVAL with a message for a pole
 * mfm_runrs_set_dc_block refuses and for a run list that is not a burst resampler's: a channel >= nr_channels or channels not
 * ascending, a run with MFM_RUNRS_BEGINS clear that is not its channel's first, a range beyond nr_elems; on any error nothing
 * is written, the state included. */
int mfm_hosttwin_runrs_dc_call(uint32_t nr_channels, double pole, struct mfm_runrs_dc_state *dc, const struct mfm_runrs_run *runs,
                               size_t nr_runs, int16_t *payload, size_t nr_elems);
/* the validation mfm_runrs_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runrs.h).  plen as in mfm_hosttwin_runrs_call; dc may be NULL. */
int mfm_hosttwin_runrs_state_check(uint32_t nr_channels, uint32_t interpolate, uint32_t plen, const struct mfm_runrs_state *state,
                                   const struct mfm_runrs_dc_state *dc);
/* what mfm_runroute_create checks and derives, no device needed: MFM_OK with *max_runs = the router's run capacity (max_runs
 * as given, or the burst resampler's default for the same numbers: one rule, csrc/mfm_runrs.h), or MFM_E_INVAL with the
 * message create gives.  max_runs may be NULL. */
int mfm_hosttwin_runroute_capacity(const struct mfm_runroute_config *cfg, const uint8_t *route_of_channel, uint32_t *max_runs);
/* host twin of one mfm_runroute_process_device call, no device needed (csrc/mfm_runroute.h, the route lookup and the refusal
 * predicate its kernel runs): gate_runs / gate_totals[4] are one gate call's result, max_runs the router's capacity.  Route
 * k's list goes to runs + k * max_runs and its totals to totals + 4 * k (runs [nr_routes * max_runs], totals [nr_routes * 4]).
 * A refused call returns MFM_OK as the device does, with the flags in every route's totals and `runs` untouched.
 * MFM_E_INVAL with a message for a table or a nr_routes that create refuses. */
int mfm_hosttwin_runroute_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *route_of_channel, size_t max_runs,
                               const struct mfm_gate_run *gate_runs, const uint64_t *gate_totals, struct mfm_gate_run *runs, uint64_t *totals);
/* what mfm_runroute_create_sets checks and mfm_runroute_route_caps then returns for `route`, no device needed: MFM_OK with the
 * three numbers (any may be NULL), or MFM_E_INVAL with create's message */
int mfm_hosttwin_runroute_route_caps(const struct mfm_runroute_config *cfg, const uint8_t *routes_of_channel, uint32_t route,
                                     uint32_t *nr_channels, uint32_t *max_windows, uint32_t *max_runs);
/* host twin of one mfm_runroute_process_device call on an object of mfm_runroute_create_sets, no device needed
 * (csrc/mfm_runroute.h: the set lookup, the rank and the refusal predicates its kernels run).  flags is 0 or
 * MFM_RUNROUTE_F_PACK; max_runs is the router's capacity.  Route k's list goes to runs + k * max_runs and its totals to
 * totals + 4 * k.  Under PACK route_max_runs [nr_routes] and route_max_windows [nr_routes] are the routes' own capacities
 * (what mfm_runroute_route_caps returns; none may exceed max_runs, or max_elems / window_samples), gate_payload is the gate's
 * payload of gate_totals[1] elements, and route k's payload goes to payloads + k * max_elems; without PACK the four and
 * window_samples are not read.  A refused call, or a refused route, returns MFM_OK as the device does, with the flags in the
 * totals and nothing else written for it. */
int mfm_hosttwin_runroute_sets_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *routes_of_channel, uint32_t flags,
                                    uint32_t window_samples, size_t max_runs, const uint32_t *route_max_runs, const uint32_t *route_max_windows,
                                    const struct mfm_gate_run *gate_runs, const int16_t *gate_payload, const uint64_t *gate_totals,
                                    struct mfm_gate_run *runs, uint64_t *totals, int16_t *payloads, size_t max_elems);
/* host twin of one mfm_runroute_process_device call on an object of mfm_runroute_create_local, no device needed
 * (csrc/mfm_runroute.h: the set lookup, the rank and the refusal predicates its kernel runs).  max_runs is the router's
 * capacity, route_max_runs [nr_routes] and route_max_windows [nr_routes] the routes' own (what mfm_runroute_route_caps returns;
 * no route_max_runs may exceed max_runs).  Route k's list goes to runs + k * max_runs and its totals to totals + 4 * k;
 * *payload_elems is what the call leaves behind mfm_runroute_bound_view.  The gate's payload is not an argument: nothing of it
 * is read.  A refused call, or a refused route, returns MFM_OK as the device does, with the flags in the totals and nothing else
 * written for it.  MFM_E_INVAL with a message for a table, a nr_routes or a window_samples that create refuses. */
int mfm_hosttwin_runroute_local_call(uint32_t nr_channels, uint32_t nr_routes, const uint8_t *routes_of_channel, uint32_t window_samples,
                                     size_t max_runs, const uint32_t *route_max_runs, const uint32_t *route_max_windows,
                                     const struct mfm_gate_run *gate_runs, const uint64_t *gate_totals, struct mfm_gate_run *runs,
                                     uint64_t *totals, uint64_t *payload_elems);
/* the per-channel state of the burst AIS stage, on the device and in the host twin: all zero at the start of a stream.
 * Fields a mode does not use are zero.  What a stored state must satisfy: csrc/mfm_runais.h (mfm_runais_state_check) */
struct mfm_runais_state {       /* 264 bytes */
    uint64_t outs;              /* outputs of the stretch so far */
    uint64_t stretch_window;    /* first window of the stretch */
    uint64_t pos;               /* SEARCH: next sample to look at (all positions stretch-relative) */
    uint64_t r;                 /* SEARCH: first sample after the last detector reset */
    uint64_t rd;                /* RECEIVE: next sample to read a bit from */
    uint64_t start;             /* RECEIVE: sample where the preamble matched */
    uint32_t mode;              /* 0 SEARCH, 1 RECEIVE */
    uint32_t last_sample;       /* RECEIVE: the bit read last (NRZI) */
    uint32_t hist8;             /* RECEIVE: the eight decoded bits read last, newest in bit 7 */
    uint32_t cur_bit;           /* RECEIVE: bits kept so far */
    uint32_t has_stretch;       /* 0: nothing to continue */
    uint32_t reserved;          /* 0 */
    uint32_t packet[40];        /* the packet so far, LSB first */
    uint32_t tail[8];           /* the last 256 sample bits of the stretch, the newest in bit 31 of tail[7]; zeros in front of
                                   a stretch shorter than that */
};
/* host twin of one mfm_runais_process_device call and its fetch, no device needed: runs / payload / totals are one burst
 * resampler call's result (totals[4] as its d_totals), state [nr_channels] is read and updated in place, max_runs,
 * max_out_samples and max_events are the configuration's (max_events 0 = its default).  Same refusals: MFM_E_STATE with the
 * message mfm_runais_fetch gives and *flags = overflow | input error << 8; MFM_E_NOMEM when max_out is too small (*nr_events
 * = needed); on any error nothing is written, the state included. */
int mfm_hosttwin_runais_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                             struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                             const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events, uint32_t *flags);
/* the same on the burst resampler's bits form: runs / bits / totals are one mfm_runrs_process_bits_device call's result (or
 * mfm_hosttwin_runrs_call_bits'), polarity its polarity (MFM_E_INVAL with a message unless MFM_BITS_POS).  PCM and bits calls may
 * alternate on one state. */
int mfm_hosttwin_runais_call_bits(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                  struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const uint32_t *bits, uint32_t polarity,
                                  const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events,
                                  uint32_t *flags);
/* the validation mfm_runais_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runais.h) */
int mfm_hosttwin_runais_state_check(uint32_t nr_channels, const struct mfm_runais_state *state);
/* mfm_hosttwin_runais_call with the stretch-end records of the call (mfm_runais_fetch_ends' of an object with the report on):
 * at most max_ends are written, *nr_ends is their number; MFM_E_NOMEM when max_ends is too small (*nr_ends = needed), and on
 * any error nothing is written, the state included.  There is no twin for the bits form: records do not depend on the form. */
int mfm_hosttwin_runais_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                  struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                  const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events, uint32_t *flags,
                                  struct mfm_runais_end *ends, size_t max_ends, size_t *nr_ends);
/* host twin of mfm_runais_end_stretches_device and its fetch: a record for every channel with a stretch, then state
 * [nr_channels] all zero; MFM_E_NOMEM when max_ends is too small (*nr_ends = needed, nothing written) */
int mfm_hosttwin_runais_end_stretches(uint32_t nr_channels, struct mfm_runais_state *state, struct mfm_runais_end *ends, size_t max_ends,
                                      size_t *nr_ends);
/* the per-channel state of the burst POCSAG stage, on the device and in the host twin: all zero at the start of a stream.
 * Fields a mode does not use are zero.  What a stored state must satisfy: csrc/mfm_runpocsag.h (mfm_runpocsag_state_check) */
struct mfm_runpocsag_state {    /* 432 bytes */
    uint64_t outs;              /* outputs of the stretch so far */
    uint64_t stretch_window;    /* first window of the stretch */
    uint32_t mode;              /* 0 SEARCH, 2 BATCH, 3 SYNCWORD */
    uint32_t baud;              /* BATCH / SYNCWORD: 512 / 1200 / 2400 */
    uint32_t spb;               /* BATCH / SYNCWORD: samples per bit (the reference's sample_skip) */
    uint32_t skip;              /* BATCH / SYNCWORD: the reference's 16-bit cur_sample_skip after the last output */
    uint32_t batch_word;        /* BATCH: words complete */
    uint32_t batch_bit;         /* BATCH: bits of the word in progress */
    uint32_t sync_word;         /* SYNCWORD: the bits of the sync slot so far, the newest in bit 0 */
    uint32_t nr_sync_bits;
    uint32_t nr_eye[3];         /* SEARCH: nr_eye_matches of the 512 / 1200 / 2400 detector after the last output */
    uint32_t since_reset;       /* SEARCH: outputs since the last detector reset (stretch start or SYNC_LOST), at most 2400 */
    uint32_t has_stretch;       /* 0: nothing to continue */
    uint32_t batch[16];         /* BATCH: the batch so far, LSB first */
    uint32_t tail[75];          /* the last 2400 sample bits of the stretch, the newest in bit 31 of tail[74]; zeros in front
                                   of a stretch shorter than that */
};
/* host twin of one mfm_runpocsag_process_device call and its fetch, no device needed: runs / payload / totals are one burst
 * resampler call's result (totals[4] as its d_totals), state [nr_channels] is read and updated in place, max_runs,
 * max_out_samples and max_events are the configuration's (max_events 0 = its default).  Same refusals: MFM_E_STATE with the
 * message mfm_runpocsag_fetch gives and *flags = overflow | input error << 8; MFM_E_NOMEM when max_out is too small
 * (*nr_events = needed); on any error nothing is written, the state included. */
int mfm_hosttwin_runpocsag_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out, size_t *nr_events,
                                uint32_t *flags);
/* the same on the burst resampler's bits form: runs / bits / totals are one mfm_runrs_process_bits_device call's result (or
 * mfm_hosttwin_runrs_call_bits'), polarity its polarity (MFM_E_INVAL with a message unless MFM_BITS_NEG).  PCM and bits calls may
 * alternate on one state. */
int mfm_hosttwin_runpocsag_call_bits(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                     struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const uint32_t *bits,
                                     uint32_t polarity, const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out,
                                     size_t *nr_events, uint32_t *flags);
/* the validation mfm_runpocsag_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runpocsag.h) */
int mfm_hosttwin_runpocsag_state_check(uint32_t nr_channels, const struct mfm_runpocsag_state *state);
/* mfm_hosttwin_runpocsag_call with the stretch-end records of the call, as mfm_hosttwin_runais_call_ends */
int mfm_hosttwin_runpocsag_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                     struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                     const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out, size_t *nr_events,
                                     uint32_t *flags, struct mfm_runpocsag_end *ends, size_t max_ends, size_t *nr_ends);
/* host twin of mfm_runpocsag_end_stretches_device and its fetch, as mfm_hosttwin_runais_end_stretches */
int mfm_hosttwin_runpocsag_end_stretches(uint32_t nr_channels, struct mfm_runpocsag_state *state, struct mfm_runpocsag_end *ends,
                                         size_t max_ends, size_t *nr_ends);
/* the per-channel state of the burst FLEX stage, on the device and in the host twin, beside the channel's ring of 32 768 PCM
 * samples: all zero at the start of a stream.  Positions are stretch-relative.  Fields a mode does not use are zero.  What a
 * stored state must satisfy: csrc/mfm_runflex.h (mfm_runflex_state_check) */
struct mfm_runflex_state {      /* 88 bytes */
    uint64_t outs;              /* outputs of the stretch so far */
    uint64_t stretch_window;    /* first window of the stretch */
    uint64_t p;                 /* SEARCH: next sample to look at (behind a reset: 311 samples behind it, maybe beyond outs) */
    uint64_t j;                 /* SYNC1: the sample that ended the BS1 run; FRAME: the sample of the last FIW bit */
    uint32_t mode;              /* 0 SEARCH, 1 SYNC1 (waiting for the sync words or the FIW), 2 FRAME (waiting for the block) */
    uint32_t run;               /* SEARCH: matches counted in the run that is open at p */
    uint32_t eye;               /* SYNC1 / FRAME: the run length modulo 256 that opened the eye */
    uint32_t coding;            /* FRAME: what the FRAME event will carry, as mfm_flex_event */
    uint32_t a;
    uint32_t b;
    uint32_t inv_a;
    uint32_t fiw_raw;
    uint32_t fiw;
    int32_t sample_range;
    int32_t sample_delta;
    uint32_t cycle;
    uint32_t frame;
    uint32_t has_stretch;       /* 0: nothing to continue */
};
/* host twin of one mfm_runflex_process_device call and its fetch, no device needed: runs / payload / totals are one burst
 * resampler call's result (totals[4] as its d_totals), state [nr_channels] and ring [nr_channels][32768] are read and updated
 * in place, max_runs, max_out_samples, max_events and max_frames are the configuration's (0 = the default).  Same refusals:
 * MFM_E_STATE with the message mfm_runflex_fetch gives and *flags = overflow | input error << 8; MFM_E_NOMEM when max_out or
 * max_out_frames is too small (*nr_events, *nr_frames = needed); on any error nothing is written, state and ring included. */
int mfm_hosttwin_runflex_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                              uint32_t max_frames, struct mfm_runflex_state *state, int16_t *ring, const struct mfm_runrs_run *runs,
                              const int16_t *payload, const uint64_t *totals, struct mfm_runflex_event *events, size_t max_out,
                              size_t *nr_events, struct mfm_flex_frame_words *frames, size_t max_out_frames, size_t *nr_frames,
                              uint32_t *flags);
/* the validation mfm_runflex_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runflex.h) */
int mfm_hosttwin_runflex_state_check(uint32_t nr_channels, const struct mfm_runflex_state *state);
/* mfm_hosttwin_runflex_call with the stretch-end records of the call, as mfm_hosttwin_runais_call_ends */
int mfm_hosttwin_runflex_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                   uint32_t max_frames, struct mfm_runflex_state *state, int16_t *ring, const struct mfm_runrs_run *runs,
                                   const int16_t *payload, const uint64_t *totals, struct mfm_runflex_event *events, size_t max_out,
                                   size_t *nr_events, struct mfm_flex_frame_words *frames, size_t max_out_frames, size_t *nr_frames,
                                   uint32_t *flags, struct mfm_runflex_end *ends, size_t max_ends, size_t *nr_ends);
/* host twin of mfm_runflex_end_stretches_device and its fetch, as mfm_hosttwin_runais_end_stretches (the rings are not touched) */
int mfm_hosttwin_runflex_end_stretches(uint32_t nr_channels, struct mfm_runflex_state *state, struct mfm_runflex_end *ends,
                                       size_t max_ends, size_t *nr_ends);
/* the per-channel state of the burst Mueller-Muller stage, on the device and in the host twin: all zero at the start of a
 * stream.  What a stored state must satisfy: csrc/mfm_runmm.h (mfm_runmm_state_check) */
struct mfm_runmm_state {        /* 48 bytes */
    uint64_t outs;              /* outputs of the stretch so far */
    uint64_t decs;              /* decisions of the stretch so far */
    uint64_t stretch_window;    /* first window of the stretch */
    float w;                    /* the reference's w, m and last_sample after the last decision (mm_init's before the first) */
    float m;
    float last_sample;
    uint32_t next_offset;       /* whole samples from the stretch's end so far to the next decision */
    uint32_t has_stretch;       /* 0: nothing to continue */
    uint32_t reserved;          /* 0 */
};
/* host twin of one mfm_runmm_process_device call and its fetch, no device needed (cfg->device is not read): runs / payload /
 * totals are one burst resampler call's result (totals[4] as its d_totals), state [cfg->nr_channels] is read and updated in
 * place.  Same refusals: MFM_E_INVAL with the message create gives; MFM_E_STATE with the message mfm_runmm_fetch gives and
 * *flags = overflow | input error << 8; MFM_E_NOMEM when max_out_runs or max_out_decisions is too small (*nr_runs,
 * *nr_decisions = needed); on any error nothing is written, the state included. */
int mfm_hosttwin_runmm_call(const struct mfm_runmm_config *cfg, struct mfm_runmm_state *state, const struct mfm_runrs_run *runs,
                            const int16_t *payload, const uint64_t *totals, struct mfm_runmm_run *out_runs, size_t max_out_runs,
                            size_t *nr_runs, int16_t *decisions, size_t max_out_decisions, size_t *nr_decisions, uint32_t *flags);
/* the validation mfm_runmm_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runmm.h) */
int mfm_hosttwin_runmm_state_check(uint32_t nr_channels, const struct mfm_runmm_state *state);
/* host twin of one mfm_runsync_process_device call and its fetch, no device needed (cfg->device is not read): runs / decisions /
 * totals are one burst Mueller-Muller call's result (totals[4] as its d_totals), state [cfg->nr_channels] is read and updated in
 * place.  Same refusals: MFM_E_INVAL with the message create gives; MFM_E_STATE with the message mfm_runsync_fetch gives and
 * *flags = overflow | input error << 8; MFM_E_NOMEM when max_out_runs, max_out_words or max_out_events is too small (*nr_runs,
 * *nr_words, *nr_events = needed); on any error nothing is written, the state included. */
int mfm_hosttwin_runsync_call(const struct mfm_runsync_config *cfg, struct mfm_runsync_state *state, const struct mfm_runmm_run *runs,
                              const int16_t *decisions, const uint64_t *totals, struct mfm_runsync_run *out_runs, size_t max_out_runs,
                              size_t *nr_runs, uint32_t *bits, size_t max_out_words, size_t *nr_words, struct mfm_runsync_event *events,
                              size_t max_out_events, size_t *nr_events, uint32_t *flags);
/* the validation mfm_runsync_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runsync.h) */
int mfm_hosttwin_runsync_state_check(uint32_t nr_channels, const struct mfm_runsync_state *state);
/* host twin of one mfm_runbatch_process_device call and its fetch, no device needed (cfg->device is not read): runs / bits /
 * sync_events / totals are one burst sync call's result as mfm_runsync_fetch gives it, with its four totals; state[nr_channels]
 * is read and, where the call is right and fits, updated in place.  Same refusals: MFM_E_INVAL with the message create gives;
 * MFM_E_STATE with the message mfm_runbatch_fetch gives and *flags = overflow | input error << 8; MFM_E_NOMEM with *nr_events
 * what is needed.  Either way nothing is written and no state moves. */
int mfm_hosttwin_runbatch_call(const struct mfm_runbatch_config *cfg, struct mfm_runbatch_state *state, const struct mfm_runsync_run *runs,
                               const uint32_t *bits, const struct mfm_runsync_event *sync_events, const uint64_t *totals,
                               struct mfm_runbatch_event *events, size_t max_out_events, size_t *nr_events, uint32_t *flags);
/* the validation mfm_runbatch_store_state applies, no device needed: MFM_OK, or MFM_E_INVAL with a message naming the first
 * channel and field that fail (csrc/mfm_runbatch.h) */
int mfm_hosttwin_runbatch_state_check(uint32_t nr_channels, const struct mfm_runbatch_state *state);
/* The form mfm_resampler_create() would choose for this configuration and these taps, planned on the host by the same function
 * and without looking for a device (cfg->device is not read).  MFM_E_INVAL for what create refuses: its argument checks, a ratio
 * whose walk steps past a phase (ceil(D / I) > phase length), a call whose phase walk does not fit 32 bits, more than 150 KB
 * of LDS per workgroup. */
int mfm_hosttwin_resampler_form(const struct mfm_resampler_config *cfg, const int16_t *coeffs, size_t nr_coeffs,
                                struct mfm_resampler_form *form);
/* One block of 16 outputs of the matrix form, evaluated on the CPU from the tables its kernel reads and indexed the way its
 * lanes index them: the A fragments of G for the carried phase `phase` (< I) in the matrix instruction's lane order, the row
 * constants, the input as two byte planes (x = 256 Xh + Xl + 128) in rows of R samples padded to row_bytes (the padding holds
 * a non-zero filler: G must be zero over it), the sums ll + (md << 8) + (hh << 16) + krow wrapping in 32 bits, Q14 rounding.
 * x[0] is the first sample of the block, samples from nr_x on count as 0.  A check of the tables and of the layout arithmetic,
 * not of the instruction; MFM_E_INVAL where create would not choose the matrix form. */
int mfm_hosttwin_resampler_matrix_block(const struct mfm_resampler_config *cfg, const int16_t *coeffs, size_t nr_coeffs,
                                        uint32_t phase, const int16_t *x, size_t nr_x, int16_t y16[16]);

#ifdef __cplusplus
}
#endif

#endif /* MULTIFM_HIP_H */
