/*
 * mfm_runpocsag.hip - the burst POCSAG stage: the runs the burst resampler left in its dense payload go through the POCSAG
 * demodulator (pager/pager_pocsag.c:81-117,434-543) on the device, one fresh demodulator per stretch.  See
 * include/multifm_hip.h for the boundary and the event format, mfm_runpocsag.h for the segment layout, the tail, the slot
 * bound, mfm_run_stage.h for the checks of a run, and mfm_pocsag.hip for the row stage whose bit-sliced correlator, segmented eye scan and
 * strided gathers this file restates.
 *
 * The input is what mfm_runrs_device_view returns; how many runs and samples a call carries is read on the device, so the
 * host never waits and every launch is sized from the capacities fixed at create.
 *
 *   rp_plan_kernel     one block.  One pass over the runs: every run is checked (mfm_run_check_run) before anything of
 *                      the payload is read; exclusive scans of the runs' segment words, event slots and slicer workgroups; a
 *                      channel's last run leaves its index for the state kernel; the totals and the flags.
 *   rp_slice_kernel    payload int16 -> 1 bit per sample (sample < 0).  A workgroup takes 256 words of one run's segment,
 *                      which it finds from its index by binary search in the scanned workgroup counts: the 75 history words
 *                      (the channel's carried tail, or zeros), then 32 samples per lane as four 16-byte loads, the run's end
 *                      one by one.
 *                      On the resampler's bits form (mfm_runpocsag_process_bits_device) rb_slice_kernel of mfm_run_bits.hip
 *                      runs in its place: the 32 sample bits of a word are one payload word, a 4-byte copy.
 *   rp_match_kernel    the free-running match words m[d] of the three rates over every segment, data parallel: a workgroup
 *                      takes the same 256 segment words as in the slicer, puts them and the 76 words in front (the
 *                      correlators reach 31 * 75 samples back) into LDS and every thread computes the three match words of
 *                      its own segment word, bit-sliced (carry-save adders over 32 shifted views, every shift a constant);
 *                      and a summary, one bit per segment word: "a run of two or more matches touches this word".
 *   rp_walk_kernel     one wave per run: mfm_pocsag.hip's SEARCH / BATCH / SYNCWORD loop in segment coordinates, from the
 *                      carried state or a fresh one.  SEARCH takes 64 segment words (2048 samples) per step from the three
 *                      planes, the segmented wave scan finds the first "run of more than spb / 2 matches ends", and with
 *                      nothing pending the summary skips 65 536 samples per step.  For 31 * 75 samples behind a SYNC_LOST
 *                      the walker recomputes the words itself from LDS with the pre-reset bits masked off ("EXACT"); a reset
 *                      at stretch sample 0 needs none of that, the history in front of it is zeros already.  BATCH and
 *                      SYNCWORD are strided gathers with ballots that stop at the run's end; the partial batch stays in
 *                      the per-run record.  BCH by the syndrome -> flip-mask table in LDS (mfm_bch.h).  Events go to the
 *                      run's slot range.
 *   rp_evscan_kernel   one block: exclusive scan of the runs' event counts, the total.
 *   rp_compact_kernel  one wave per run: its events from the slot range into the dense list.
 *   rp_state_kernel    one block per channel: the record of the channel's last run and the last 2400 bits of its segment
 *                      go into the OTHER of two state buffers; a channel without a run, and every channel of a refused
 *                      call, copies its state over.
 *
 * Nothing is floating point and no atomic decides a placement. The block scan, a thread's slice of the runs, the plan's head, the count scan and
 * the word copy of the compaction, and the host code around a call are mfm_run_stage.h's, shared with the other burst stages.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_bch.h"
#include "mfm_run_bits.h"
#include "mfm_run_ends.h"
#include "mfm_runpocsag.h"

static_assert(sizeof(mfm_runpocsag_event) == 176 && offsetof(mfm_runpocsag_event, run) == 16 &&
                  offsetof(mfm_runpocsag_event, stretch_window) == 32 && offsetof(mfm_runpocsag_event, sample) == 40 &&
                  offsetof(mfm_runpocsag_event, raw) == 48 && offsetof(mfm_runpocsag_event, corrected) == 112,
              "struct mfm_runpocsag_event is 176 bytes");
static_assert(sizeof(mfm_runpocsag_state) == 432 && offsetof(mfm_runpocsag_state, batch) == 68 && offsetof(mfm_runpocsag_state, tail) == 132,
              "struct mfm_runpocsag_state");

namespace {

constexpr uint32_t RP_SLICE_NT = MFM_RUN_BITS_SLICE_NT;         /* slicer: threads = segment words per workgroup */
constexpr uint32_t RP_T_EVENTS = 0, RP_T_RUNS = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RP_SYNC = MFM_RUNPOCSAG_SYNC;
constexpr uint32_t RP_BACK = 76;              /* 31 * 75 bits = 72.7 words of history, plus the funnel-shift neighbour */
constexpr uint32_t RP_TILE = RP_BACK + 64 + 2;
constexpr uint32_t RP_STATE_WORDS = sizeof(mfm_runpocsag_state) / 4, RP_TAIL_WORD0 = offsetof(mfm_runpocsag_state, tail) / 4;
static_assert(MFM_RUNPOCSAG_HIST_WORDS + 1 >= RP_BACK, "a step's tile starts at most one word in front of the segment");

/* ---- bit-sliced sync-word correlator, after pg_count_le4 and pg_match32 of mfm_pocsag.hip --------------------------------- */

#define RP_FA(a, b, c, s, cy)                                                                                \
    do {                                                                                                     \
        const uint32_t x_ = (a) ^ (b);                                                                       \
        const uint32_t s_ = x_ ^ (c);                                                                        \
        const uint32_t c_ = (x_ & (c)) | ((a) & (b));                                                        \
        (s) = s_;                                                                                            \
        (cy) = c_;                                                                                           \
    } while (0)
#define RP_HA(a, b, s, cy)                                                                                   \
    do {                                                                                                     \
        const uint32_t s_ = (a) ^ (b);                                                                       \
        const uint32_t c_ = (a) & (b);                                                                       \
        (s) = s_;                                                                                            \
        (cy) = c_;                                                                                           \
    } while (0)

/* y[0..31]: 32 one-bit-per-sample mismatch vectors; returns, per sample, "at most 4 of them are set" */
__device__ __forceinline__ uint32_t rp_count_le4(const uint32_t *y)
{
    uint32_t s[12], c[16];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        RP_FA(y[3 * i], y[3 * i + 1], y[3 * i + 2], s[i], c[i]);
    }
    s[10] = y[30];
    s[11] = y[31];
    uint32_t t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        RP_FA(s[3 * i], s[3 * i + 1], s[3 * i + 2], t[i], c[10 + i]);
    }
    uint32_t u0, bit0;
    RP_FA(t[0], t[1], t[2], u0, c[14]);
    RP_HA(u0, t[3], bit0, c[15]);
    /* weight 2: 16 inputs */
    uint32_t v[6], d[8];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        RP_FA(c[3 * i], c[3 * i + 1], c[3 * i + 2], v[i], d[i]);
    }
    v[5] = c[15];
    uint32_t w0, w1, bit1;
    RP_FA(v[0], v[1], v[2], w0, d[5]);
    RP_FA(v[3], v[4], v[5], w1, d[6]);
    RP_HA(w0, w1, bit1, d[7]);
    /* weight 4: 8 inputs */
    uint32_t x0, x1, e0, e1, e2, e3, z0, bit2;
    RP_FA(d[0], d[1], d[2], x0, e0);
    RP_FA(d[3], d[4], d[5], x1, e1);
    RP_FA(x0, x1, d[6], z0, e2);
    RP_HA(z0, d[7], bit2, e3);
    const uint32_t ge8 = e0 | e1 | e2 | e3;
    return ~ge8 & ~(bit2 & (bit1 | bit0));
}

/*
 * m word of rate SPB for the 32 samples of tile word RP_BACK + lane: register bit j is the sample bit j * SPB samples back, so
 * every view is the tile at a constant word and bit offset from the lane's own word (the free-running map).
 */
template <int SPB>
__device__ __forceinline__ uint32_t rp_match32(const uint32_t *tile, uint32_t lane)
{
    uint32_t y[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int32_t back = -j * SPB;                 /* <= 0 */
        const int32_t qo = back >> 5;                  /* floor */
        const uint32_t sh = (uint32_t)back & 31u;
        const uint32_t q = (uint32_t)((int32_t)(RP_BACK + lane) + qo);
        const uint32_t x = sh == 0 ? tile[q] : __builtin_amdgcn_alignbit(tile[q + 1], tile[q], sh);
        y[j] = ((RP_SYNC >> j) & 1u) ? ~x : x;
    }
    return rp_count_le4(y);
}

/*
 * The same word with the bits of samples before r_t (tile bit index of the reset) read as zero, which is what the
 * reference's zero-filled registers hold (pager_pocsag.c:119-126): "EXACT".  Only the two steps behind a SYNC_LOST take it, so
 * it is a rolled loop with a saturating bit-sliced counter and costs the walker no registers.
 */
__device__ __forceinline__ uint32_t rp_match32_exact(const uint32_t *tile, uint32_t lane, int32_t r_t, uint32_t spb)
{
    uint32_t c0 = 0, c1 = 0, c2 = 0, ov = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < 32; j++) {
        const int32_t P = 32 * (int32_t)(RP_BACK + lane) - (int32_t)(j * spb); /* tile bit of the view's bit 0: >= 32 * 76 - 2325 */
        const uint32_t q = (uint32_t)P >> 5, sh = (uint32_t)P & 31u;
        uint32_t x = __builtin_amdgcn_alignbit(tile[q + 1], tile[q], sh);
        const int32_t th = r_t - P; /* first bit of the view that is a real one */
        x &= th <= 0 ? 0xffffffffu : (th >= 32 ? 0u : (0xffffffffu << th));
        const uint32_t y = ((RP_SYNC >> j) & 1u) ? ~x : x;
        const uint32_t t0 = c0 & y;
        c0 ^= y;
        const uint32_t t1 = c1 & t0;
        c1 ^= t0;
        ov |= c2 & t1; /* eight or more */
        c2 ^= t1;
    }
    return ~ov & ~(c2 & (c1 | c0)); /* at most four mismatches */
}

/* ---- the call ------------------------------------------------------------------------------------------------------- */

struct RpCall {
    const mfm_runrs_run *runs;
    const int16_t *payload;
    const uint32_t *bits; /* the resampler's bits form: the payload of predicate words, and payload is NULL */
    const uint64_t *rtotals;
    const mfm_runpocsag_state *chan_old;
    mfm_runpocsag_state *chan_new;
    mfm_runpocsag_state *run_state; /* [cap_runs] what a run's walk ends in (all but the tail) */
    uint32_t *seg;                  /* the runs' bit segments, one behind the other */
    uint32_t *plane;                /* the match words: plane d (512 / 1200 / 2400) at plane + d * seg_cap, laid out as seg */
    uint32_t *summ;                 /* the summary: a run's words from (seg_base >> 5) + run index on, one bit per segment word */
    uint32_t *seg_base;             /* [cap_runs] first word of a run's segment */
    uint32_t *slot_base;            /* [cap_runs] first event slot of a run */
    uint32_t *blk_base;             /* [cap_runs + 1] first slicer workgroup of a run */
    uint32_t *count;                /* [cap_runs] events of a run */
    uint32_t *ev_base;              /* [cap_runs] their exclusive scan */
    uint32_t *chan_last;            /* [C] */
    uint32_t *ctl;                  /* [0] workgroups of the slicer, [1] runs */
    uint64_t *totals;
    mfm_runpocsag_event *slots;     /* [cap_events] */
    mfm_runpocsag_event *events;    /* [cap_events] */
    const MfmBchTables *bch;
    uint32_t C, cap_runs, cap_out, cap_events, seg_cap;
};

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rp_plan_kernel(const RpCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    const bool words = A.bits != nullptr; /* E and out_offset count words of the bits payload */
    uint64_t n, E, over, err, r0, r1;
    if (!mfm_run_plan_head(A.rtotals, words ? (uint64_t)A.cap_out / 32u + A.cap_runs : (uint64_t)A.cap_out, A.cap_runs, A.totals, A.ctl, 2, &n, &E, &over, &err)) {
        return; /* nothing may be read */
    }
    mfm_run_slice(n, &r0, &r1);
    uint64_t so = 0, sw = 0, ss = 0, sb = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        const mfm_runrs_run run = A.runs[r];
        bad |= mfm_run_check_run(run, r ? &A.runs[r - 1] : nullptr, A.C, E, A.chan_old, words);
        const uint32_t w = mfm_runpocsag_seg_words(run.nr_out);
        so += run.nr_out;
        sw += w;
        ss += mfm_runpocsag_slots(run.nr_out);
        sb += (w + RP_SLICE_NT - 1u) / RP_SLICE_NT;
    }
    /* fewer than 2^28 runs of fewer than 2^32 outputs: every sum stays below 2^63 */
    uint64_t to, tws, tb;
    (void)mfm_run_block_scan(so, lds, &to);
    /* a call that is not refused has fewer than 2^32 segment words and fewer than 2^32 slots (rp_geometry): they share a scan */
    const uint64_t bws = mfm_run_block_scan((sw & 0xffffffffull) | (ss << 32), lds, &tws);
    uint64_t bw = bws & 0xffffffffull, bs = bws >> 32, ts = tws >> 32;
    uint64_t bb = mfm_run_block_scan(sb, lds, &tb);
    if (__syncthreads_or((bad & MFM_RUNPOCSAG_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNPOCSAG_IN_OUT_OF_STEP;
    }
    /* ranges that overlap could ask for more than the segments hold */
    if (__syncthreads_or((bad & MFM_RUNPOCSAG_IN_BAD_RUNS) != 0) || to > A.cap_out) {
        err |= MFM_RUNPOCSAG_IN_BAD_RUNS;
    }
    if (!err && ts > A.cap_events) {
        over = MFM_RUNPOCSAG_OVER_EVENTS;
    }
    const bool refused = over || err;
    if (!refused) { /* within the capacities: segment words, slots and workgroups all fit 32 bits (rp_geometry) */
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t nr_out = A.runs[r].nr_out, c = A.runs[r].channel;
            const uint32_t w = mfm_runpocsag_seg_words(nr_out);
            A.seg_base[r] = (uint32_t)bw;
            A.slot_base[r] = (uint32_t)bs;
            A.blk_base[r] = (uint32_t)bb;
            bw += w;
            bs += mfm_runpocsag_slots(nr_out);
            bb += (w + RP_SLICE_NT - 1u) / RP_SLICE_NT;
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RP_T_EVENTS] = 0; /* the event scan */
        A.totals[RP_T_RUNS] = refused ? 0u : n;
        A.totals[MFM_RUN_T_OVERFLOW] = over;
        A.totals[MFM_RUN_T_INPUT] = err;
        if (!refused) {
            A.blk_base[n] = (uint32_t)tb;
        }
        A.ctl[0] = refused ? 0u : (uint32_t)tb;
        A.ctl[1] = refused ? 0u : (uint32_t)n;
    }
}

struct __attribute__((packed, aligned(2))) RpPcm8 { /* eight samples as one 16-byte access */
    uint32_t d[4];
};

__device__ __forceinline__ uint32_t rp_neg2(uint32_t d) /* the sign bits of two samples (pager_pocsag.c:91) */
{
    return ((d >> 15) & 1u) | ((d >> 30) & 2u);
}

__global__ __launch_bounds__(RP_SLICE_NT) void rp_slice_kernel(const RpCall A)
{
    const uint32_t b = blockIdx.x;
    if (b >= A.ctl[0]) { /* surplus workgroups: the launch is sized from the capacity */
        return;
    }
    /* the run of workgroup b: the last r with blk_base[r] <= b (every run has at least one) */
    uint32_t lo = 0, hi = A.ctl[1];
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.blk_base[mid] <= b) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    const uint32_t r = lo;
    const mfm_runrs_run run = A.runs[r];
    const uint32_t w = (b - A.blk_base[r]) * RP_SLICE_NT + threadIdx.x;
    if (w >= mfm_runpocsag_seg_words(run.nr_out)) {
        return;
    }
    uint32_t word = 0;
    if (w < MFM_RUNPOCSAG_HIST_WORDS) {
        word = (run.flags & MFM_RUNRS_BEGINS) ? 0u : A.chan_old[run.channel].tail[w];
    } else {
        const uint32_t j0 = (w - MFM_RUNPOCSAG_HIST_WORDS) * 32u;
        const int16_t *x = A.payload + run.out_offset; /* [out_offset, out_offset + nr_out) lies within the totals (the plan) */
        if (j0 < run.nr_out && run.nr_out - j0 >= 32u) {
#pragma unroll
            for (uint32_t g = 0; g < 4; g++) {
                const RpPcm8 v = *reinterpret_cast<const RpPcm8 *>(x + j0 + 8u * g);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    word |= rp_neg2(v.d[q]) << (8u * g + 2u * q);
                }
            }
        } else { /* the run's last samples; the padding word stays zero */
            for (uint32_t i = 0; i < 32u && j0 + i < run.nr_out; i++) {
                word |= (x[j0 + i] < 0 ? 1u : 0u) << i;
            }
        }
    }
    A.seg[A.seg_base[r] + w] = word;
}

/* m[0..2] and the summary of the 256 segment words the slicer's workgroup of the same index wrote */
__global__ __launch_bounds__(RP_SLICE_NT) void rp_match_kernel(const RpCall A)
{
    __shared__ uint32_t tile[RP_BACK + RP_SLICE_NT + 2];
    const uint32_t b = blockIdx.x;
    if (b >= A.ctl[0]) {
        return;
    }
    uint32_t lo = 0, hi = A.ctl[1];
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.blk_base[mid] <= b) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    const uint32_t r = lo;
    const uint32_t nw = mfm_runpocsag_seg_words(A.runs[r].nr_out);
    const uint32_t w_blk = (b - A.blk_base[r]) * RP_SLICE_NT; /* < nw: the run has ceil(nw / 256) workgroups */
    const uint32_t base = A.seg_base[r];
    const uint32_t *bits = A.seg + base;
    for (uint32_t k = threadIdx.x; k < RP_BACK + RP_SLICE_NT + 2u; k += RP_SLICE_NT) {
        const int64_t q = (int64_t)w_blk - (int64_t)RP_BACK + (int64_t)k;
        tile[k] = q >= 0 && q < (int64_t)nw ? bits[q] : 0u; /* in front of the segment: the zeros a fresh stretch has there */
    }
    __syncthreads();
    const uint32_t w = w_blk + threadIdx.x;
    const bool in = w < nw;
    const uint32_t ms[3] = { rp_match32<75>(tile, threadIdx.x), rp_match32<32>(tile, threadIdx.x), rp_match32<16>(tile, threadIdx.x) };
    if (in) {
        A.plane[base + w] = ms[0];
        A.plane[(size_t)A.seg_cap + base + w] = ms[1];
        A.plane[2 * (size_t)A.seg_cap + base + w] = ms[2];
    }
    /* summary bit: two adjacent matches inside the word, or its last sample and the next word's first both match (across a
     * wave boundary: assume they do).  A detector fires only after more than 8 matches in a row, so with nothing pending the
     * walker skips words without the bit */
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t flag = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const uint32_t nxt = (uint32_t)__shfl_down((int)ms[d], 1);
        const uint32_t next_first = lane == 63 ? 1u : (nxt & 1u);
        flag |= (ms[d] & (ms[d] >> 1)) | ((ms[d] >> 31) & next_first);
    }
    const unsigned long long any = __ballot(in && flag != 0u);
    if ((lane == 0 || lane == 32) && in) {
        A.summ[(base >> 5) + r + (w >> 5)] = (uint32_t)(any >> lane);
    }
}

__device__ __forceinline__ uint32_t rp_wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o < v ? o : v;
    }
    return v;
}

/* one wave per run: pager_pocsag_on_pcm (pager_pocsag.c:434-543) from event to event, positions stretch-relative */
__global__ __launch_bounds__(64) void rp_walk_kernel(const RpCall A)
{
    __shared__ MfmBchTables T;
    __shared__ uint32_t tile[RP_TILE];
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) { /* surplus waves, and every wave of a refused call */
        return;
    }
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(A.bch);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&T);
        for (uint32_t i = lane; i < sizeof(MfmBchTables) / 4; i += 64u) {
            dst[i] = src[i];
        }
    }
    __syncthreads();
    const mfm_runrs_run run = A.runs[r];
    const bool begins = (run.flags & MFM_RUNRS_BEGINS) != 0;
    const mfm_runpocsag_state *old = &A.chan_old[run.channel];
    /* a fresh decoder: SEARCH at sample 0, reset at 0, nothing collected.  b0 is the sample that carries the next bit to
     * collect (BATCH / SYNCWORD), nb / ns the bits of the batch / sync slot so far, sacc the sync bits in their final places
     * (the first in bit 31); lane w < 16 holds batch word w */
    uint64_t pos = run.first_out, b0 = 0, stretch_window = run.first_window;
    int64_t rst = 0;
    uint32_t mode = MFM_RUNPOCSAG_SEARCH, S = 0, baud = 0, nb = 0, ns = 0, sacc = 0, myraw = 0;
    uint32_t nr[3] = { 0, 0, 0 };
    if (!begins) {
        mode = old->mode;
        S = old->spb;
        baud = old->baud;
        nb = old->batch_word * 32u + old->batch_bit;
        ns = old->nr_sync_bits;
        sacc = ns ? old->sync_word << (32u - ns) : 0u;
        nr[0] = old->nr_eye[0];
        nr[1] = old->nr_eye[1];
        nr[2] = old->nr_eye[2];
        myraw = lane < 16u ? old->batch[lane] : 0u;
        rst = (int64_t)run.first_out - (int64_t)old->since_reset;
        b0 = run.first_out + ((S - 1u - old->skip) & 0xffffu); /* ++skip == S there (16-bit counter) */
        stretch_window = old->stretch_window;
    }
    const uint32_t *bits = A.seg + A.seg_base[r];
    const uint32_t *planes = A.plane + A.seg_base[r];
    const uint32_t *summ = A.summ + (A.seg_base[r] >> 5) + r;
    const int64_t ws = (int64_t)run.first_out - (int64_t)MFM_RUNPOCSAG_HIST_BITS; /* stretch sample of segment bit 0 */
    const uint64_t end = run.first_out + run.nr_out;
    const uint32_t max_ev = mfm_runpocsag_slots(run.nr_out), nw = mfm_runpocsag_seg_words(run.nr_out);
    const uint32_t nsumm = (nw + 31u) / 32u;
    mfm_runpocsag_event *ev = A.slots + A.slot_base[r];
    uint32_t nev = 0;
    auto getbit = [&](uint64_t n) { /* n in [first_out, end) */
        const uint32_t o = (uint32_t)((int64_t)n - ws);
        return (bits[o >> 5] >> (o & 31u)) & 1u;
    };
    auto emit = [&](uint32_t type, uint32_t aux, uint64_t sample, uint32_t nr_ok, uint32_t fail_mask, uint32_t raw, uint32_t fixed) {
        if (nev < max_ev) { /* always: the slot bound (mfm_runpocsag_slots) */
            mfm_runpocsag_event *e = &ev[nev];
            if (lane == 0) {
                e->type = type;
                e->baud = baud;
                e->channel = run.channel;
                e->aux = aux;
                e->run = r;
                e->nr_ok = nr_ok;
                e->fail_mask = fail_mask;
                e->reserved = 0;
                e->stretch_window = stretch_window;
                e->sample = sample;
            }
            if (lane < 16u) {
                e->raw[lane] = raw;
                e->corrected[lane] = fixed;
            }
            nev++;
        }
    };

    for (;;) {
        if (mode == MFM_RUNPOCSAG_SEARCH) {
            if (pos >= end) {
                break;
            }
            /* ---- one step: the 64 segment words from the one that holds pos, all three detectors ---- */
            const uint32_t w0 = (uint32_t)((int64_t)pos - ws) >> 5; /* >= 75: pos lies behind the history */
            /* the planes are the free-running map; behind a SYNC_LOST the registers differ from it for 31 * 75 samples.  A
             * reset at stretch sample 0 has zeros in front of it in the segment: there the map is exact as it stands */
            const bool exact = rst > 0 && (int64_t)pos < rst + (int64_t)MFM_RUNPOCSAG_SLOW_SPAN;
            if (exact) {
                __syncthreads();
                for (uint32_t k = lane; k < RP_TILE; k += 64u) {
                    const int64_t q = (int64_t)w0 - (int64_t)RP_BACK + (int64_t)k;
                    tile[k] = q >= 0 && q < (int64_t)nw ? bits[q] : 0u;
                }
                __syncthreads();
            }
            const int64_t cb = ws + 32 * (int64_t)w0;
            const int64_t lane_base = cb + 32 * (int64_t)lane;
            const int64_t lo64 = (int64_t)pos - lane_base, hi64 = (int64_t)end - lane_base;
            const int lo = lo64 < 0 ? 0 : (lo64 > 32 ? 32 : (int)lo64);
            const int hi = hi64 < 0 ? 0 : (hi64 > 32 ? 32 : (int)hi64);
            const bool active = hi > lo;
            const uint32_t rm = active ? (((hi == 32) ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
            /* the reset as a bit index of the tile (tile word 0 is segment word w0 - RP_BACK); only looked at while it is near */
            int64_t r_t64 = rst - (cb - 32 * (int64_t)RP_BACK);
            r_t64 = r_t64 < -8192 ? -8192 : (r_t64 > 8192 ? 8192 : r_t64);
            const int32_t r_t = (int32_t)r_t64;
            uint32_t bestkey = 0xffffffffu, bestrun = 0;
            uint32_t endrun[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const uint32_t spb = d == 0 ? 75u : (d == 1 ? 32u : 16u);
                uint32_t m;
                if (exact) {
                    m = rp_match32_exact(tile, lane, r_t, spb);
                } else {
                    m = w0 + lane < nw ? planes[(size_t)d * A.seg_cap + w0 + lane] : 0u;
                }
                const uint32_t z = ~m & rm; /* non-matching samples of my word that are in range */
                /* run of matches reaching the end of my range, and whether my whole range matches */
                uint32_t full = (z == 0u) ? 1u : 0u;
                uint32_t val = active ? ((z == 0u) ? (uint32_t)(hi - lo) : (uint32_t)(hi - 1 - (31 - __clz((int)z)))) : 0u;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t pv = (uint32_t)__shfl_up((int)val, off);
                    const uint32_t pf = (uint32_t)__shfl_up((int)full, off);
                    if ((int)lane >= off) {
                        val = full ? val + pv : val;
                        full = full & pf;
                    }
                }
                uint32_t c_in = (uint32_t)__shfl_up((int)val, 1);
                uint32_t f_in = (uint32_t)__shfl_up((int)full, 1);
                if (lane == 0) {
                    c_in = 0;
                    f_in = 1;
                }
                c_in += f_in ? nr[d] : 0u; /* nr_eye_matches when the detector reaches my range */
                const uint32_t v63 = (uint32_t)__shfl((int)val, 63), f63 = (uint32_t)__shfl((int)full, 63);
                endrun[d] = v63 + (f63 ? nr[d] : 0u);
                if (active) {
                    /* a detector fires on a non-matching sample that ends a run of more than spb/2 matches
                     * (pager_pocsag.c:96-108); only samples right behind a match can qualify */
                    uint32_t cand = z & (((m & rm) << 1) | ((c_in > 0u) ? (1u << lo) : 0u));
                    while (cand) {
                        const int k = __ffs((int)cand) - 1;
                        cand &= cand - 1u;
                        const uint32_t zb = z & ((1u << k) - 1u);
                        const uint32_t run_len = zb ? (uint32_t)(k - 1 - (31 - __clz((int)zb))) : (uint32_t)(k - lo) + c_in;
                        if (run_len > spb / 2u) {
                            const uint32_t key = ((lane * 32u + (uint32_t)k) << 2) | (uint32_t)(2 - d);
                            if (key < bestkey) {
                                bestkey = key;
                                bestrun = run_len;
                            }
                            break;
                        }
                    }
                }
            }
            const uint32_t minkey = rp_wave_min(bestkey);
            if (minkey != 0xffffffffu) {
                /* earliest sample wins; on the same sample the detector run last (2400 after 1200 after 512)
                 * leaves its settings behind (pager_pocsag.c:452-457) */
                const unsigned long long who = __ballot(bestkey == minkey);
                const uint32_t run_len = (uint32_t)__shfl((int)bestrun, __ffsll((long long)who) - 1);
                const int d = 2 - (int)(minkey & 3u);
                const uint64_t f = (uint64_t)(cb + (int64_t)(minkey >> 2));
                S = d == 0 ? 75u : (d == 1 ? 32u : 16u);
                baud = d == 0 ? 512u : (d == 1 ? 1200u : 2400u);
                emit(MFM_POCSAG_EV_SYNC_FOUND, run_len, f, 0, 0, 0, 0);
                /* batch.cur_sample_skip = matches / 2 (uint16), a bit is taken when ++skip == sample_skip */
                const uint32_t c0 = (run_len >> 1) & 0xffffu;
                b0 = f + (c0 < S ? S - c0 : 65536u + S - c0);
                mode = MFM_RUNPOCSAG_BATCH;
                nb = 0;
                myraw = 0;
                nr[0] = nr[1] = nr[2] = 0;
            } else {
                nr[0] = endrun[0];
                nr[1] = endrun[1];
                nr[2] = endrun[2];
                const uint64_t nxt = (uint64_t)(cb + 32 * 64);
                pos = nxt < end ? nxt : end;
                /* nothing pending and the map exact: jump to the next word with any run of matches in it */
                while ((nr[0] | nr[1] | nr[2]) == 0u && pos < end && !(rst > 0 && (int64_t)pos < rst + (int64_t)MFM_RUNPOCSAG_SLOW_SPAN)) {
                    const uint32_t wp = (uint32_t)((int64_t)pos - ws) >> 5; /* the segment word of pos */
                    const uint32_t sw0 = wp >> 5;
                    const uint32_t sidx = sw0 + lane;
                    uint32_t sv = sidx < nsumm ? summ[sidx] : 0xffffffffu;
                    if (lane == 0) {
                        sv &= 0xffffffffu << (wp & 31u); /* words in front of pos are done with */
                    }
                    const unsigned long long nz = __ballot(sv != 0u);
                    if (nz == 0ull) {
                        const uint64_t far = (uint64_t)(ws + 1024 * (int64_t)(sw0 + 64u));
                        pos = far < end ? far : end;
                        continue;
                    }
                    const int l1 = __ffsll((long long)nz) - 1;
                    const uint32_t svw = (uint32_t)__shfl((int)sv, l1);
                    const int64_t hit = ws + 32 * (int64_t)((sw0 + (uint32_t)l1) * 32u + (uint32_t)(__ffs((int)svw) - 1));
                    pos = hit <= (int64_t)pos ? pos : ((uint64_t)hit < end ? (uint64_t)hit : end);
                    break;
                }
            }
        } else if (mode == MFM_RUNPOCSAG_BATCH) {
            /* the bits of the batch still to come, one every S samples, LSB first into 16 words (pager_pocsag.c:472-481),
             * as far as the run holds them */
            if (b0 >= end) {
                break;
            }
            const uint64_t avail = (end - 1 - b0) / S + 1;
            const uint32_t want = 512u - nb;
            const uint32_t take = avail < want ? (uint32_t)avail : want;
#pragma unroll
            for (uint32_t g = 0; g < 8; g++) {
                const uint32_t i = 64u * g + lane; /* bit of the batch */
                const bool valid = i >= nb && i - nb < take;
                const uint32_t bit = valid ? getbit(b0 + (uint64_t)(i - nb) * S) : 0u;
                const unsigned long long bl = __ballot((int)bit);
                if (lane == 2 * g) {
                    myraw |= (uint32_t)bl;
                }
                if (lane == 2 * g + 1) {
                    myraw |= (uint32_t)(bl >> 32);
                }
            }
            if (take == want) {
                const uint64_t at = b0 + (uint64_t)(want - 1u) * S;
                uint32_t rc = 0;
                const uint32_t fixed = mfm_bch_fix(&T, myraw & 0x7fffffffu, &rc); /* pager_pocsag.c:332-334 */
                const uint32_t fail = (uint32_t)__ballot(lane < 16u && rc) & 0xffffu;
                const uint32_t nr_ok = fail ? (uint32_t)(__ffs((int)fail) - 1) : 16u;
                emit(MFM_POCSAG_EV_BATCH, 0, at, nr_ok, fail, myraw, fixed);
                myraw = 0;
                nb = 0;
                b0 = at + S;
                mode = MFM_RUNPOCSAG_SYNCWORD;
                ns = 0;
                sacc = 0;
            } else {
                nb += take;
                b0 += (uint64_t)take * S; /* >= end */
            }
        } else {
            /* the 32 bits of the sync slot, the first ending up in bit 31 (pager_pocsag.c:506-513) */
            if (b0 >= end) {
                break;
            }
            const uint64_t avail = (end - 1 - b0) / S + 1;
            const uint32_t want = 32u - ns;
            const uint32_t take = avail < want ? (uint32_t)avail : want;
            const bool valid = lane < 32u && lane >= ns && lane - ns < take;
            const uint32_t bit = valid ? getbit(b0 + (uint64_t)(lane - ns) * S) : 0u;
            sacc |= __brev((uint32_t)__ballot((int)bit));
            if (take == want) {
                const uint64_t at = b0 + (uint64_t)(want - 1u) * S;
                const uint32_t sw = sacc;
                ns = 0;
                sacc = 0;
                if (__popc(sw ^ RP_SYNC) <= 4) {
                    emit(MFM_POCSAG_EV_SYNC_KEPT, sw, at, 0, 0, 0, 0);
                    b0 = at + S;
                    mode = MFM_RUNPOCSAG_BATCH;
                    nb = 0;
                    myraw = 0;
                } else {
                    emit(MFM_POCSAG_EV_SYNC_LOST, sw, at, 0, 0, 0, 0);
                    mode = MFM_RUNPOCSAG_SEARCH; /* pager_pocsag.c:517-523: all three detectors start from zero */
                    pos = at + 1;
                    rst = (int64_t)(at + 1);
                    nr[0] = nr[1] = nr[2] = 0;
                    S = 0;
                    baud = 0;
                }
            } else {
                ns += take;
                b0 += (uint64_t)take * S; /* >= end */
            }
        }
    }
    /* every lane holds the whole state but the batch words; fields the mode does not use are zero */
    mfm_runpocsag_state *dst = &A.run_state[r];
    const bool search = mode == MFM_RUNPOCSAG_SEARCH;
    if (lane < 16u) {
        dst->batch[lane] = mode == MFM_RUNPOCSAG_BATCH ? myraw : 0u;
    }
    if (lane == 0) {
        const int64_t since = (int64_t)end - rst;
        dst->outs = end;
        dst->stretch_window = stretch_window;
        dst->mode = mode;
        dst->baud = baud;
        dst->spb = S;
        dst->skip = search ? 0u : (S - 1u - (uint32_t)(b0 - end)) & 0xffffu;
        dst->batch_word = mode == MFM_RUNPOCSAG_BATCH ? nb >> 5 : 0u;
        dst->batch_bit = mode == MFM_RUNPOCSAG_BATCH ? nb & 31u : 0u;
        dst->sync_word = mode == MFM_RUNPOCSAG_SYNCWORD && ns ? sacc >> (32u - ns) : 0u;
        dst->nr_sync_bits = mode == MFM_RUNPOCSAG_SYNCWORD ? ns : 0u;
        dst->nr_eye[0] = search ? nr[0] : 0u;
        dst->nr_eye[1] = search ? nr[1] : 0u;
        dst->nr_eye[2] = search ? nr[2] : 0u;
        dst->since_reset = search ? (since < (int64_t)MFM_RUNPOCSAG_HIST_BITS ? (uint32_t)since : MFM_RUNPOCSAG_HIST_BITS) : 0u;
        dst->has_stretch = 1;
        A.count[r] = nev;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rp_evscan_kernel(const RpCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    /* 0 runs for a refused call; the total is at most the sum of the slots: within cap_events */
    const uint64_t total = mfm_run_count_scan(A.count, A.ev_base, A.ctl[1], lds);
    if (threadIdx.x == 0) {
        A.totals[RP_T_EVENTS] = total;
    }
}

__global__ __launch_bounds__(64) void rp_compact_kernel(const RpCall A)
{
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) {
        return;
    }
    constexpr uint32_t EW = sizeof(mfm_runpocsag_event) / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.slots + A.slot_base[r]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(A.events + A.ev_base[r]);
    mfm_run_copy_words(src, dst, &A.count[r], EW);
}

__global__ __launch_bounds__(128) void rp_state_kernel(const RpCall A)
{
    __shared__ uint32_t s_last;
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_last = A.chan_last[c];
        A.chan_last[c] = MFM_RUN_NONE; /* for the next call */
    }
    __syncthreads();
    const uint32_t last = s_last;
    const bool refused = A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0;
    uint32_t *nw = reinterpret_cast<uint32_t *>(&A.chan_new[c]);
    if (last == MFM_RUN_NONE || refused) { /* the state stays */
        const uint32_t *old = reinterpret_cast<const uint32_t *>(&A.chan_old[c]);
        for (uint32_t i = tid; i < RP_STATE_WORDS; i += blockDim.x) {
            nw[i] = old[i];
        }
        return;
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&A.run_state[last]);
    const uint32_t *seg = A.seg + A.seg_base[last];
    const uint32_t nr_out = A.runs[last].nr_out;
    for (uint32_t i = tid; i < RP_STATE_WORDS; i += blockDim.x) {
        nw[i] = i < RP_TAIL_WORD0 ? src[i] : mfm_runpocsag_tail_word(seg, nr_out, i - RP_TAIL_WORD0);
    }
}

/* what create checks without a device; the capacities with the default filled in */
int rp_geometry(const mfm_runpocsag_config &cfg, uint64_t *cap_events)
{
    const int rc = mfm_run_geometry(cfg);
    if (rc != MFM_OK) {
        return rc;
    }
    /* the sum of mfm_runpocsag_slots over max_runs runs that share max_out_samples outputs, at most */
    *cap_events = cfg.max_events ? cfg.max_events : 3ull * (cfg.max_out_samples / MFM_RUNPOCSAG_MIN_SPACING) + 5ull * cfg.max_runs;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *rp_refusal(uint64_t over, uint64_t err)
{
    return mfm_run_refusal(over, err, "the call's event bound (the sum of 3 * (nr_out / 8704 + 1) + 2 over its runs) exceeds max_events");
}

} /* namespace */

struct mfm_runpocsag {
    mfm_runpocsag_config cfg{};
    uint64_t cap_events = 0, seg_words = 0, max_blocks = 0;
    mfm_runpocsag_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    mfm_runpocsag_state *d_run_state = nullptr;
    uint32_t *d_plane = nullptr, *d_summ = nullptr;
    uint32_t *d_seg = nullptr, *d_seg_base = nullptr, *d_slot_base = nullptr, *d_blk_base = nullptr, *d_count = nullptr, *d_ev_base = nullptr;
    uint32_t *d_chan_last = nullptr, *d_ctl = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runpocsag_event *d_slots = nullptr, *d_events = nullptr;
    MfmBchTables *d_bch = nullptr; /* owned by mfm_pocsag.hip, one per device */
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    MfmRunEnds ends; /* the stretch-end report (mfm_run_ends.h); off at create */
};

extern "C" {

int mfm_runpocsag_create(struct mfm_runpocsag **pp, const struct mfm_runpocsag_config *cfg)
{
    if (!pp || !cfg) {
        return MFM_E_INVAL;
    }
    *pp = nullptr;
    uint64_t cap_events = 0;
    const int rc = rp_geometry(*cfg, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    MfmBchTables *d_bch = nullptr;
    const int rb = mfm_internal_bch_device_tables(cfg->device, &d_bch);
    if (rb != MFM_OK) {
        return rb; /* no CPU path */
    }
    mfm_runpocsag *p = new (std::nothrow) mfm_runpocsag();
    if (!p) {
        return MFM_E_NOMEM;
    }
    p->cfg = *cfg;
    p->cap_events = cap_events;
    p->d_bch = d_bch;
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    /* a run's segment has at most nr_out / 32 + 77 words and (that + 255) / 256 slicer workgroups */
    p->seg_words = (uint64_t)cfg->max_out_samples / 32u + (MFM_RUNPOCSAG_HIST_WORDS + 2ull) * nruns;
    p->max_blocks = p->seg_words / RP_SLICE_NT + nruns;
    if (p->seg_words >= (1ull << 32) || p->max_blocks >= (1ull << 31)) {
        delete p;
        return mfm_run_fail(MFM_E_INVAL, "max_runs and max_out_samples together ask for 2^32 segment words or more");
    }
    *pp = p; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&p->d_chan[i], C * sizeof(mfm_runpocsag_state)));
        MFM_RUN_TRY(hipMemset(p->d_chan[i], 0, C * sizeof(mfm_runpocsag_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&p->d_run_state, nruns * sizeof(mfm_runpocsag_state)));
    MFM_RUN_TRY(hipMalloc(&p->d_seg, (size_t)p->seg_words * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_plane, (size_t)p->seg_words * 12));
    MFM_RUN_TRY(hipMalloc(&p->d_summ, ((size_t)p->seg_words / 32 + 2 * nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_seg_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_slot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_blk_base, (nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_count, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_ev_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(p->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_ctl, 2 * 4));
    MFM_RUN_TRY(hipMemset(p->d_ctl, 0, 2 * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(p->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&p->d_slots, (size_t)cap_events * sizeof(mfm_runpocsag_event)));
    MFM_RUN_TRY(hipMalloc(&p->d_events, (size_t)cap_events * sizeof(mfm_runpocsag_event)));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runpocsag_destroy(struct mfm_runpocsag **pp)
{
    if (!pp || !*pp) {
        return;
    }
    mfm_runpocsag *p = *pp;
    (void)hipSetDevice(p->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->d_chan[0]);
    (void)hipFree(p->d_chan[1]);
    (void)hipFree(p->d_run_state);
    (void)hipFree(p->d_seg);
    (void)hipFree(p->d_plane);
    (void)hipFree(p->d_summ);
    (void)hipFree(p->d_seg_base);
    (void)hipFree(p->d_slot_base);
    (void)hipFree(p->d_blk_base);
    (void)hipFree(p->d_count);
    (void)hipFree(p->d_ev_base);
    (void)hipFree(p->d_chan_last);
    (void)hipFree(p->d_ctl);
    (void)hipFree(p->d_totals);
    (void)hipFree(p->d_slots);
    (void)hipFree(p->d_events);
    (void)mfm_internal_run_ends_set(&p->ends, MFM_RUN_ENDS_POCSAG, false, 0, 0);
    delete p;
    *pp = nullptr;
}

} /* extern "C" */

namespace {

/* one call in either form: d_payload (PCM) or d_bits (the resampler's bits form), the other NULL */
int rp_process(mfm_runpocsag *p, const mfm_runrs_run *d_runs, const int16_t *d_payload, const uint32_t *d_bits, const uint64_t *d_totals,
               void *stream)
{
    if (!p || !d_runs || (!d_payload && !d_bits) || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(p, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = p->cur;
    const RpCall A{ d_runs,         d_payload,     d_bits,         d_totals,       p->d_chan[cur], p->d_chan[cur ^ 1u], p->d_run_state,
                    p->d_seg,       p->d_plane,    p->d_summ,      p->d_seg_base, p->d_slot_base, p->d_blk_base,  p->d_count,          p->d_ev_base,
                    p->d_chan_last, p->d_ctl,      p->d_totals,    p->d_slots,     p->d_events,         p->d_bch,
                    p->cfg.nr_channels, p->cfg.max_runs, p->cfg.max_out_samples, (uint32_t)p->cap_events, (uint32_t)p->seg_words };
    hipLaunchKernelGGL(rp_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    if (d_bits) { /* the word copy of mfm_run_bits.hip in the place of the slicer */
        const mfm_run_bits_slice B{ d_runs, d_bits, reinterpret_cast<const uint32_t *>(p->d_chan[cur]), p->d_blk_base, p->d_seg_base, p->d_ctl,
                                    p->d_seg, RP_STATE_WORDS, RP_TAIL_WORD0, MFM_RUNPOCSAG_HIST_WORDS };
        if (mfm_internal_run_bits_slice(&B, (uint32_t)p->max_blocks, s) != MFM_OK) {
            MFM_RUN_TRY(hipGetLastError());
            return MFM_E_DEVICE;
        }
    } else {
        hipLaunchKernelGGL(rp_slice_kernel, dim3((uint32_t)p->max_blocks), dim3(RP_SLICE_NT), 0, s, A);
        MFM_RUN_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(rp_match_kernel, dim3((uint32_t)p->max_blocks), dim3(RP_SLICE_NT), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rp_walk_kernel, dim3(p->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rp_evscan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rp_compact_kernel, dim3(p->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    if (p->ends.on) { /* behind the walk, in front of the state kernel */
        const MfmRunEndsCall E{ d_runs, p->d_chan[cur], p->d_run_state, p->d_ctl, p->d_bch, p->cfg.nr_channels, p->cfg.max_runs };
        const int re = mfm_internal_run_ends_process(&p->ends, MFM_RUN_ENDS_POCSAG, &E, s);
        if (re != MFM_OK) {
            return re;
        }
    }
    hipLaunchKernelGGL(rp_state_kernel, dim3(p->cfg.nr_channels), dim3(128), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(p, s);
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_runpocsag_process_device(struct mfm_runpocsag *p, const struct mfm_runrs_run *d_runs, const int16_t *d_payload,
                                 const uint64_t *d_totals, void *stream)
{
    if (!d_payload) {
        return MFM_E_INVAL;
    }
    return rp_process(p, d_runs, d_payload, nullptr, d_totals, stream);
}

int mfm_runpocsag_process_bits_device(struct mfm_runpocsag *p, const struct mfm_runrs_bits_view *view, void *stream)
{
    if (!p || !view || !view->d_bits) {
        return MFM_E_INVAL;
    }
    if (view->polarity != MFM_BITS_NEG) {
        return mfm_run_fail(MFM_E_INVAL, "the burst POCSAG stage needs MFM_BITS_NEG bits (bit = sample < 0)");
    }
    return rp_process(p, view->d_runs, nullptr, view->d_bits, view->d_totals, stream);
}

int mfm_runpocsag_fetch(struct mfm_runpocsag *p, struct mfm_runpocsag_event *events, size_t max_events, size_t *nr_events)
{
    if (!p || !nr_events || (!events && max_events)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (!p->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(p->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(p->last_stream));
    uint64_t t[4];
    MFM_RUN_TRY(hipMemcpy(t, p->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, rp_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    *nr_events = (size_t)t[RP_T_EVENTS];
    if (t[RP_T_EVENTS] > max_events) {
        return MFM_E_NOMEM;
    }
    if (t[RP_T_EVENTS]) {
        MFM_RUN_TRY(hipMemcpy(events, p->d_events, (size_t)t[RP_T_EVENTS] * sizeof(mfm_runpocsag_event), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runpocsag_device_view(struct mfm_runpocsag *p, const struct mfm_runpocsag_event **d_events, const uint64_t **d_totals)
{
    if (!p) {
        return MFM_E_INVAL;
    }
    if (d_events) {
        *d_events = p->d_events;
    }
    if (d_totals) {
        *d_totals = p->d_totals;
    }
    return MFM_OK;
}

int mfm_hosttwin_runpocsag_state_check(uint32_t nr_channels, const struct mfm_runpocsag_state *state)
{
    return mfm_run_state_check(nr_channels, state, "POCSAG", mfm_runpocsag_state_check);
}

int mfm_runpocsag_fetch_state(struct mfm_runpocsag *p, struct mfm_runpocsag_state *state, size_t nr_channels)
{
    return mfm_run_fetch_state(p, state, nr_channels);
}

int mfm_runpocsag_store_state(struct mfm_runpocsag *p, const struct mfm_runpocsag_state *state, size_t nr_channels)
{
    return mfm_run_store_state(p, state, nr_channels, mfm_hosttwin_runpocsag_state_check);
}

/* ---- the stretch-end report: kernels and launchers in mfm_run_ends.hip ---- */

int mfm_runpocsag_set_end_report(struct mfm_runpocsag *p, int on)
{
    return mfm_run_ends_entry_set(p, MFM_RUN_ENDS_POCSAG, on, mfm_run_fail);
}

int mfm_runpocsag_end_stretches_device(struct mfm_runpocsag *p, void *stream)
{
    return mfm_run_ends_entry_flush(p, MFM_RUN_ENDS_POCSAG, p ? p->d_bch : nullptr, stream, mfm_run_fail);
}

int mfm_runpocsag_fetch_ends(struct mfm_runpocsag *p, struct mfm_runpocsag_end *ends, size_t max_ends, size_t *nr_ends)
{
    return mfm_run_ends_entry_fetch(p, MFM_RUN_ENDS_POCSAG, ends, max_ends, nr_ends, mfm_run_fail, rp_refusal);
}

int mfm_runpocsag_ends_view(struct mfm_runpocsag *p, const struct mfm_runpocsag_end **d_ends, const uint64_t **d_end_totals)
{
    return mfm_run_ends_entry_view(p, d_ends, d_end_totals, mfm_run_fail);
}

} /* extern "C" */

/* ---- the host twin: the same plan, segments and tail, the decoder one sample at a time in the reference's own terms ------ */

namespace {

/* one run through the decoder from state st (updated in place, all but the tail); events appended */
void rp_host_walk(mfm_runpocsag_state &st, const uint32_t *seg, const mfm_runrs_run &run, uint32_t r, std::vector<mfm_runpocsag_event> &out)
{
    static const uint32_t SPB[3] = { 75, 32, 16 }, BAUD[3] = { 512, 1200, 2400 };
    const MfmBchTables *T = mfm_internal_bch_host_tables();
    const int64_t ws = (int64_t)run.first_out - (int64_t)MFM_RUNPOCSAG_HIST_BITS;
    const uint64_t end = (uint64_t)run.first_out + run.nr_out;
    int64_t rst = (int64_t)run.first_out - (int64_t)st.since_reset;
    auto raw = [&](int64_t x) {
        const uint64_t o = (uint64_t)(x - ws);
        return (seg[o >> 5] >> (o & 31u)) & 1u;
    };
    auto event = [&](uint32_t type, uint32_t aux, uint64_t sample) {
        mfm_runpocsag_event e;
        memset(&e, 0, sizeof(e));
        e.type = type;
        e.baud = st.baud;
        e.channel = run.channel;
        e.aux = aux;
        e.run = r;
        e.stretch_window = st.stretch_window;
        e.sample = sample;
        return e;
    };
    for (uint64_t n = run.first_out; n < end; n++) {
        const uint32_t bit = raw((int64_t)n);
        if (st.mode == MFM_RUNPOCSAG_SEARCH) {
            int fired = -1;
            uint32_t matches = 0;
            for (int d = 0; d < 3; d++) { /* pager_pocsag.c:455-460, :81-117 */
                uint32_t reg = 0;
                for (int j = 0; j < 32; j++) {
                    const int64_t s = (int64_t)n - (int64_t)j * SPB[d];
                    if (s >= rst) { /* the registers were zero-filled at the reset */
                        reg |= raw(s) << j;
                    }
                }
                if (__builtin_popcount(reg ^ MFM_RUNPOCSAG_SYNC) <= 4) {
                    st.nr_eye[d]++;
                } else if (st.nr_eye[d] > SPB[d] / 2u) {
                    fired = d; /* the later detector wins */
                    matches = st.nr_eye[d];
                } else {
                    st.nr_eye[d] = 0;
                }
            }
            if (fired >= 0) {
                st.mode = MFM_RUNPOCSAG_BATCH;
                st.baud = BAUD[fired];
                st.spb = SPB[fired];
                st.skip = (matches / 2u) & 0xffffu;
                st.batch_word = st.batch_bit = 0;
                memset(st.batch, 0, sizeof(st.batch));
                st.nr_eye[0] = st.nr_eye[1] = st.nr_eye[2] = 0;
                out.push_back(event(MFM_POCSAG_EV_SYNC_FOUND, matches, n));
            }
        } else if (st.mode == MFM_RUNPOCSAG_BATCH) {
            st.skip = (st.skip + 1u) & 0xffffu;
            if (st.skip == st.spb) { /* :474-481 */
                st.skip = 0;
                st.batch[st.batch_word] |= bit << st.batch_bit;
                if (++st.batch_bit == 32u) {
                    st.batch_bit = 0;
                    if (++st.batch_word == 16u) {
                        mfm_runpocsag_event e = event(MFM_POCSAG_EV_BATCH, 0, n);
                        e.nr_ok = 16;
                        for (uint32_t z = 0; z < 16; z++) { /* :332-334 */
                            uint32_t rc = 0;
                            e.raw[z] = st.batch[z];
                            e.corrected[z] = mfm_bch_fix(T, st.batch[z] & 0x7fffffffu, &rc);
                            if (rc) {
                                e.fail_mask |= 1u << z;
                                if (e.nr_ok == 16u) {
                                    e.nr_ok = z;
                                }
                            }
                        }
                        out.push_back(e);
                        memset(st.batch, 0, sizeof(st.batch));
                        st.batch_word = 0;
                        st.mode = MFM_RUNPOCSAG_SYNCWORD;
                        st.sync_word = st.nr_sync_bits = 0;
                    }
                }
            }
        } else {
            st.skip = (st.skip + 1u) & 0xffffu;
            if (st.skip == st.spb) { /* :511-534 */
                st.skip = 0;
                st.sync_word = (st.sync_word << 1) | bit;
                if (++st.nr_sync_bits == 32u) {
                    const uint32_t sw = st.sync_word;
                    st.sync_word = st.nr_sync_bits = 0;
                    if (__builtin_popcount(sw ^ MFM_RUNPOCSAG_SYNC) <= 4) {
                        out.push_back(event(MFM_POCSAG_EV_SYNC_KEPT, sw, n));
                        st.mode = MFM_RUNPOCSAG_BATCH;
                    } else {
                        out.push_back(event(MFM_POCSAG_EV_SYNC_LOST, sw, n));
                        st.mode = MFM_RUNPOCSAG_SEARCH;
                        st.baud = st.spb = 0;
                        rst = (int64_t)n + 1;
                    }
                }
            }
        }
    }
    const int64_t since = (int64_t)end - rst;
    st.since_reset = st.mode == MFM_RUNPOCSAG_SEARCH ? (since < (int64_t)MFM_RUNPOCSAG_HIST_BITS ? (uint32_t)since : MFM_RUNPOCSAG_HIST_BITS) : 0u;
    st.outs = end;
    st.has_stretch = 1;
}

} /* namespace */

namespace {

/* a stretch-end record on the host: the BCH through the host copy of the stage's tables */
void rp_end_of(const mfm_runpocsag_state &s, uint32_t channel, uint32_t run, mfm_runpocsag_end &e)
{
    mfm_runpocsag_end_of(mfm_internal_bch_host_tables(), s, channel, run, e);
}

/* the host twin of one call in either form: bits != NULL is the resampler's bits form (totals[1] and out_offset in words) */
int rp_twin_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events, struct mfm_runpocsag_state *state,
                 const struct mfm_runrs_run *runs, const int16_t *payload, const uint32_t *bits, bool words, const uint64_t *totals,
                 struct mfm_runpocsag_event *events, size_t max_out, size_t *nr_events, uint32_t *flags,
                 struct mfm_runpocsag_end *ends = nullptr, size_t max_ends = 0, size_t *nr_ends = nullptr) /* nr_ends: with the records */
{
    if (!state || !totals || !nr_events || (!events && max_out) || (nr_ends && !ends && max_ends)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (nr_ends) {
        *nr_ends = 0;
    }
    if (flags) {
        *flags = 0;
    }
    mfm_runpocsag_config cfg{};
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = nr_channels;
    cfg.max_runs = max_runs;
    cfg.max_out_samples = max_out_samples;
    cfg.max_events = max_events;
    uint64_t cap_events = 0;
    const int rc = rp_geometry(cfg, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    uint64_t n, over, err, ts = 0; /* the plan pass */
    if (!mfm_run_twin_plan(totals, nr_channels, max_runs, max_out_samples, state, runs, words ? (const void *)bits : (const void *)payload, words,
                           [&](uint32_t nr_out) { ts += mfm_runpocsag_slots(nr_out); }, &n, &over, &err)) {
        return MFM_E_INVAL;
    }
    if (!err && ts > cap_events) {
        over = MFM_RUNPOCSAG_OVER_EVENTS;
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, rp_refusal(over, err));
    }
    /* every run from the state the call started with (only a channel's first run reads it); the state its last run leaves */
    std::vector<mfm_runpocsag_event> out;
    std::vector<mfm_runpocsag_state> left(n);
    std::vector<uint32_t> seg;
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        mfm_runpocsag_state st;
        memset(&st, 0, sizeof(st));
        st.stretch_window = run.first_window;
        if (!(run.flags & MFM_RUNRS_BEGINS)) {
            st = state[run.channel];
        }
        seg.assign(mfm_runpocsag_seg_words(run.nr_out), 0u);
        for (uint32_t k = 0; k < MFM_RUNPOCSAG_HIST_WORDS; k++) {
            seg[k] = st.tail[k]; /* zeros for a beginning run */
        }
        if (words) { /* the slicer's word copy */
            for (uint32_t k = 0; k < (run.nr_out + 31u) / 32u; k++) {
                seg[MFM_RUNPOCSAG_HIST_WORDS + k] = bits[run.out_offset + k];
            }
        } else {
            for (uint32_t j = 0; j < run.nr_out; j++) {
                if (payload[run.out_offset + j] < 0) {
                    seg[MFM_RUNPOCSAG_HIST_WORDS + (j >> 5)] |= 1u << (j & 31u);
                }
            }
        }
        rp_host_walk(st, seg.data(), run, (uint32_t)r, out);
        for (uint32_t k = 0; k < MFM_RUNPOCSAG_HIST_WORDS; k++) {
            st.tail[k] = mfm_runpocsag_tail_word(seg.data(), run.nr_out, k);
        }
        left[r] = st;
    }
    *nr_events = out.size();
    if (out.size() > max_out) {
        return MFM_E_NOMEM; /* nothing written, the state included */
    }
    if (nr_ends) { /* from the state the call started with, before it moves */
        *nr_ends = mfm_run_ends_host_call(runs, n, state, left.data(), ends, 0, rp_end_of);
        if (*nr_ends > max_ends) {
            return MFM_E_NOMEM;
        }
        (void)mfm_run_ends_host_call(runs, n, state, left.data(), ends, max_ends, rp_end_of);
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            state[runs[r].channel] = left[r];
        }
    }
    if (!out.empty()) {
        memcpy(events, out.data(), out.size() * sizeof(mfm_runpocsag_event));
    }
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_hosttwin_runpocsag_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out, size_t *nr_events,
                                uint32_t *flags)
{
    return rp_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, payload, nullptr, false, totals, events, max_out,
                        nr_events, flags);
}

int mfm_hosttwin_runpocsag_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                     struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                     const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out, size_t *nr_events,
                                     uint32_t *flags, struct mfm_runpocsag_end *ends, size_t max_ends, size_t *nr_ends)
{
    if (!nr_ends) {
        return MFM_E_INVAL;
    }
    return rp_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, payload, nullptr, false, totals, events, max_out,
                        nr_events, flags, ends, max_ends, nr_ends);
}

int mfm_hosttwin_runpocsag_end_stretches(uint32_t nr_channels, struct mfm_runpocsag_state *state, struct mfm_runpocsag_end *ends,
                                         size_t max_ends, size_t *nr_ends)
{
    return mfm_run_ends_host_flush(nr_channels, state, ends, max_ends, nr_ends, rp_end_of);
}

int mfm_hosttwin_runpocsag_call_bits(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                     struct mfm_runpocsag_state *state, const struct mfm_runrs_run *runs, const uint32_t *bits,
                                     uint32_t polarity, const uint64_t *totals, struct mfm_runpocsag_event *events, size_t max_out,
                                     size_t *nr_events, uint32_t *flags)
{
    if (polarity != MFM_BITS_NEG) {
        return mfm_run_fail(MFM_E_INVAL, "the burst POCSAG stage needs MFM_BITS_NEG bits (bit = sample < 0)");
    }
    return rp_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, nullptr, bits, true, totals, events, max_out,
                        nr_events, flags);
}

} /* extern "C" */
