/*
 * mfm_runais.hip - the burst AIS stage: the runs the burst resampler left in its dense payload go through the AIS
 * demodulator (ais/ais_demod.c:114-258) on the device, one fresh demodulator per stretch.  See include/multifm_hip.h for the
 * boundary and the event format, mfm_runais.h for the segment layout and the slot bound, mfm_run_stage.h for the checks of a
 * run, and mfm_ais.hip for the row stage whose bit-sliced correlator and RECEIVE step this file restates.
 *
 * The input is what mfm_runrs_device_view returns; how many runs and samples a call carries is read on the device, so the
 * host never waits and every launch is sized from the capacities fixed at create.
 *
 *   ra_plan_kernel     one block.  One pass over the runs: every run is checked (mfm_run_check_run) before anything of the
 *                      payload is read; exclusive scans of the runs' segment words, event slots and slicer workgroups; a
 *                      channel's last run leaves its index for the state kernel; the totals and the flags.
 *   ra_slice_kernel    payload int16 -> 1 bit per sample.  A workgroup takes 256 words of one run's segment, which it finds
 *                      from its index by binary search in the scanned workgroup counts: the 8 history words (the channel's
 *                      carried tail, or zeros), then 32 samples per lane as four 16-byte loads, the run's end one by one.
 *                      On the resampler's bits form (mfm_runais_process_bits_device) rb_slice_kernel of mfm_run_bits.hip
 *                      runs in its place: the 32 sample bits of a word are one payload word, a 4-byte copy.
 *   ra_walk_kernel     one wave per run: mfm_ais.hip's SEARCH / RECEIVE loop in segment coordinates.  SEARCH computes the M
 *                      words in the walker, a segment word per lane and 63 words (2016 samples) per step (a lane gets the
 *                      words in front of its own by lane shifts, so every shift of the correlator is a constant), with the
 *                      samples before the last reset masked off while the reset is near ("EXACT"): a beginning run has its
 *                      reset at stretch sample 0.
 *                      There is no free-running match plane: runs are short and each has a wave of its own.  Events go to
 *                      the run's slot range, the state the run ends in to a per-run record.
 *   ra_evscan_kernel   one block: exclusive scan of the runs' event counts, the total.
 *   ra_compact_kernel  one wave per run: its events from the slot range into the dense list.
 *   ra_state_kernel    one block per channel: the record of the channel's last run and the last 256 bits of its segment
 *                      go into the OTHER of two state buffers; a channel without a run, and every channel of a refused
 *                      call, copies its state over.
 *
 * Nothing is floating point and no atomic decides a placement (the packet bits of one RECEIVE step are OR-ed into LDS). The block scan, a thread's slice of the runs, the plan's head, the count scan and
 * the word copy of the compaction, and the host code around a call are mfm_run_stage.h's, shared with the other burst stages.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_run_bits.h"
#include "mfm_run_ends.h"
#include "mfm_runais.h"

static_assert(sizeof(mfm_runais_event) == 200, "struct mfm_runais_event is 200 bytes");
static_assert(sizeof(mfm_runais_state) == 264 && offsetof(mfm_runais_state, packet) == 72 && offsetof(mfm_runais_state, tail) == 232,
              "struct mfm_runais_state");

namespace {

constexpr uint32_t RA_SLICE_NT = MFM_RUN_BITS_SLICE_NT;         /* slicer: threads = segment words per workgroup */
constexpr uint32_t RA_T_EVENTS = 0, RA_T_RUNS = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RA_PREAMBLE = 0x5555557eu; /* ais_demod.c:136 */
constexpr uint32_t RA_SLOW_SPAN = 165;        /* samples after a reset during which M differs from the free-running map */
constexpr uint32_t RA_MAX_BITS = 5 * 256;     /* ais_demod.c:186 */
constexpr uint32_t RA_PACKET_WORDS = RA_MAX_BITS / 32;
constexpr uint32_t RA_STATE_WORDS = sizeof(mfm_runais_state) / 4, RA_TAIL_WORD0 = offsetof(mfm_runais_state, tail) / 4;

/* ---- bit-sliced preamble correlator, after ai_q32 and ai_m32 of mfm_ais.hip ----------------------------------------------- */

/*
 * q word for the 32 samples of one word, restated in coordinates relative to that word so that every shift is a constant:
 * v[d] is bit-stream word (mine - d), d = 0 .. 5 ((160 + 5) samples of register history).  EXACT: samples before r_loc
 * (index of the reset relative to my word's first sample) read as zero in the slicer history and in the registers, which
 * is what the reference's zero-filled prior_sample slots and preamble registers hold (ais_demod.c:44-50).
 */
template <bool EXACT>
__device__ __forceinline__ uint32_t ra_q32(const uint32_t (&v)[6], int32_t r_loc)
{
    auto mask_before = [&](int32_t P) {
        const int32_t th = r_loc - P; /* samples of the word that lie before the reset */
        return th <= 0 ? 0xffffffffu : (th >= 32 ? 0u : (0xffffffffu << th));
    };
    auto bview = [&](int32_t P) { /* P <= 0, a constant once the loop is unrolled */
        const int32_t d = -(P >> 5);
        uint32_t x = (P & 31) == 0 ? v[d] : __builtin_amdgcn_alignbit(v[d - 1], v[d], (uint32_t)P & 31u);
        if (EXACT) {
            x &= mask_before(P);
        }
        return x;
    };
    uint32_t s0 = 0, s1 = 0, ov = 0;
    uint32_t cur = bview(0);
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const int32_t P = -5 * k;
        const uint32_t prev = bview(P - 5);
        uint32_t n = ~(cur ^ prev); /* ais_demod.c:133 */
        if (EXACT) {
            n &= mask_before(P);
        }
        cur = prev;
        const uint32_t y = ((RA_PREAMBLE >> k) & 1u) ? ~n : n;
        const uint32_t c0 = s0 & y;
        s0 ^= y;
        const uint32_t c1 = s1 & c0;
        s1 ^= c0;
        ov |= c1;
    }
    uint32_t q = ~ov & ~(s0 & s1); /* at most two mismatches (ais_demod.c:40) */
    if (EXACT) {
        q &= mask_before(0); /* registers not updated since the reset are zero: no match */
    }
    return q;
}

/* M word from the q words of samples [32 wi, 32 wi + 32) and the word before: three or more of five */
__device__ __forceinline__ uint32_t ra_m32(uint32_t qc, uint32_t qp)
{
    uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t v = j == 0 ? qc : ((qc << j) | (qp >> (32 - j)));
        const uint32_t c0 = s0 & v;
        s0 ^= v;
        const uint32_t c1 = s1 & c0;
        s1 ^= c0;
        s2 |= c1;
    }
    return s2 | (s1 & s0);
}

/* ---- the call ------------------------------------------------------------------------------------------------------- */

struct RaCall {
    const mfm_runrs_run *runs;
    const int16_t *payload;
    const uint32_t *bits; /* the resampler's bits form: the payload of predicate words, and payload is NULL */
    const uint64_t *rtotals;
    const mfm_runais_state *chan_old;
    mfm_runais_state *chan_new;
    mfm_runais_state *run_state; /* [cap_runs] what a run's walk ends in (all but the tail) */
    uint32_t *seg;               /* the runs' bit segments, one behind the other */
    uint32_t *seg_base;          /* [cap_runs] first word of a run's segment */
    uint32_t *slot_base;         /* [cap_runs] first event slot of a run */
    uint32_t *blk_base;          /* [cap_runs + 1] first slicer workgroup of a run */
    uint32_t *count;             /* [cap_runs] events of a run */
    uint32_t *ev_base;           /* [cap_runs] their exclusive scan */
    uint32_t *chan_last;         /* [C] */
    uint32_t *ctl;               /* [0] workgroups of the slicer, [1] runs */
    uint64_t *totals;
    mfm_runais_event *slots;     /* [cap_events] */
    mfm_runais_event *events;    /* [cap_events] */
    uint32_t C, cap_runs, cap_out, cap_events;
};

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void ra_plan_kernel(const RaCall A)
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
        const uint32_t w = mfm_runais_seg_words(run.nr_out);
        so += run.nr_out;
        sw += w;
        ss += mfm_runais_slots(run.nr_out);
        sb += (w + RA_SLICE_NT - 1u) / RA_SLICE_NT;
    }
    /* fewer than 2^31 runs of fewer than 2^32 outputs: every sum stays below 2^63 */
    uint64_t to, tws, tb;
    (void)mfm_run_block_scan(so, lds, &to);
    /* a call that is not refused has fewer than 2^32 segment words and fewer than 2^32 slots (ra_geometry): they share a scan */
    const uint64_t bws = mfm_run_block_scan((sw & 0xffffffffull) | (ss << 32), lds, &tws);
    uint64_t bw = bws & 0xffffffffull, bs = bws >> 32, ts = tws >> 32;
    uint64_t bb = mfm_run_block_scan(sb, lds, &tb);
    if (__syncthreads_or((bad & MFM_RUNAIS_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNAIS_IN_OUT_OF_STEP;
    }
    /* ranges that overlap could ask for more than the segments hold */
    if (__syncthreads_or((bad & MFM_RUNAIS_IN_BAD_RUNS) != 0) || to > A.cap_out) {
        err |= MFM_RUNAIS_IN_BAD_RUNS;
    }
    if (!err && ts > A.cap_events) {
        over = MFM_RUNAIS_OVER_EVENTS;
    }
    const bool refused = over || err;
    if (!refused) {
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t nr_out = A.runs[r].nr_out, c = A.runs[r].channel;
            const uint32_t w = mfm_runais_seg_words(nr_out);
            A.seg_base[r] = (uint32_t)bw;
            A.slot_base[r] = (uint32_t)bs;
            A.blk_base[r] = (uint32_t)bb;
            bw += w;
            bs += mfm_runais_slots(nr_out);
            bb += (w + RA_SLICE_NT - 1u) / RA_SLICE_NT;
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RA_T_EVENTS] = 0; /* the event scan */
        A.totals[RA_T_RUNS] = refused ? 0u : n;
        A.totals[MFM_RUN_T_OVERFLOW] = over;
        A.totals[MFM_RUN_T_INPUT] = err;
        if (!refused) {
            A.blk_base[n] = (uint32_t)tb;
        }
        A.ctl[0] = refused ? 0u : (uint32_t)tb;
        A.ctl[1] = refused ? 0u : (uint32_t)n;
    }
}

struct __attribute__((packed, aligned(2))) RaPcm8 { /* eight samples as one 16-byte access */
    uint32_t d[4];
};

__device__ __forceinline__ uint32_t ra_pos2(uint32_t d)
{
    const int16_t lo = (int16_t)(d & 0xffffu), hi = (int16_t)(d >> 16);
    return (lo > 0 ? 1u : 0u) | (hi > 0 ? 2u : 0u);
}

__global__ __launch_bounds__(RA_SLICE_NT) void ra_slice_kernel(const RaCall A)
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
    const uint32_t w = (b - A.blk_base[r]) * RA_SLICE_NT + threadIdx.x;
    if (w >= mfm_runais_seg_words(run.nr_out)) {
        return;
    }
    uint32_t word = 0;
    if (w < MFM_RUNAIS_HIST_WORDS) {
        word = (run.flags & MFM_RUNRS_BEGINS) ? 0u : A.chan_old[run.channel].tail[w];
    } else {
        const uint32_t j0 = (w - MFM_RUNAIS_HIST_WORDS) * 32u;
        const int16_t *x = A.payload + run.out_offset; /* [out_offset, out_offset + nr_out) lies within the totals (the plan) */
        if (j0 < run.nr_out && run.nr_out - j0 >= 32u) {
#pragma unroll
            for (uint32_t g = 0; g < 4; g++) {
                const RaPcm8 v = *reinterpret_cast<const RaPcm8 *>(x + j0 + 8u * g);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    word |= ra_pos2(v.d[q]) << (8u * g + 2u * q);
                }
            }
        } else { /* the run's last samples; the padding word stays zero */
            for (uint32_t i = 0; i < 32u && j0 + i < run.nr_out; i++) {
                word |= (x[j0 + i] > 0 ? 1u : 0u) << i;
            }
        }
    }
    A.seg[A.seg_base[r] + w] = word;
}

/* one wave per run: ais_demod_on_pcm (ais_demod.c:215-258) from event to event, positions stretch-relative */
__global__ __launch_bounds__(64) void ra_walk_kernel(const RaCall A)
{
    __shared__ uint16_t crc_tab[256];
    __shared__ uint32_t pk[RA_PACKET_WORDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) { /* surplus waves, and every wave of a refused call */
        return;
    }
    /* CRC-16 table, reflected polynomial 0x8408 (ais_demod.c:19-36) */
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        uint32_t v = lane + 64u * j;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            v = (v & 1u) ? ((v >> 1) ^ 0x8408u) : (v >> 1);
        }
        crc_tab[lane + 64u * j] = (uint16_t)v;
    }
    const mfm_runrs_run run = A.runs[r];
    const bool begins = (run.flags & MFM_RUNRS_BEGINS) != 0;
    const mfm_runais_state *old = &A.chan_old[run.channel];
    /* a fresh demodulator: SEARCH at sample 0, reset at 0, nothing received */
    uint64_t pos = 0, rst = 0, rd = 0, start = 0, stretch_window = run.first_window;
    uint32_t mode = MFM_RUNAIS_SEARCH, last_sample = 0, hist8 = 0, cur_bit = 0;
    if (!begins) {
        pos = old->pos;
        rst = old->r;
        rd = old->rd;
        start = old->start;
        stretch_window = old->stretch_window;
        mode = old->mode;
        last_sample = old->last_sample;
        hist8 = old->hist8;
        cur_bit = old->cur_bit;
    }
    if (lane < RA_PACKET_WORDS) {
        pk[lane] = begins ? 0u : old->packet[lane];
    }
    __syncthreads();
    const uint32_t *bits = A.seg + A.seg_base[r];
    const int64_t ws = (int64_t)run.first_out - (int64_t)MFM_RUNAIS_HIST_BITS; /* stretch sample of segment bit 0 */
    const uint64_t end = run.first_out + run.nr_out;
    const uint32_t max_ev = mfm_runais_slots(run.nr_out), nw = mfm_runais_seg_words(run.nr_out);
    mfm_runais_event *ev = A.slots + A.slot_base[r];
    uint32_t nev = 0;
    auto getbit = [&](uint64_t n) {
        const uint32_t o = (uint32_t)((int64_t)n - ws);
        return (bits[o >> 5] >> (o & 31u)) & 1u;
    };

    for (;;) {
        if (mode == MFM_RUNAIS_SEARCH) {
            if (pos >= end) {
                break;
            }
            /* ---- one step: the word in front of pos (its q only) and the 63 from pos on, a word per lane ---- */
            const uint32_t w0 = (uint32_t)((int64_t)pos - ws) >> 5; /* >= 8: pos lies behind the history */
            const uint32_t wrel = w0 - 1u + lane;
            const int64_t cb = ws + 32 * (int64_t)(w0 - 1u);
            const int64_t lane_base = cb + 32 * (int64_t)lane;
            const int64_t lo64 = (int64_t)pos - lane_base, hi64 = (int64_t)end - lane_base;
            const int lo = lo64 < 0 ? 0 : (lo64 > 32 ? 32 : (int)lo64);
            const int hi = hi64 < 0 ? 0 : (hi64 > 32 ? 32 : (int)hi64);
            const uint32_t rm = hi > lo ? (((hi == 32) ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
            /* v[d] = segment word wrel - d: mine and my neighbours' by lane shifts, the first lanes' from the eight words in front */
            const uint32_t mine = wrel < nw ? bits[wrel] : 0u;
            const uint32_t front = lane < 8u && w0 + lane >= 9u ? bits[w0 - 9u + lane] : 0u;
            uint32_t v[6];
            v[0] = mine;
#pragma unroll
            for (uint32_t d = 1; d < 6; d++) {
                const uint32_t a = (uint32_t)__shfl_up((int)mine, d), f = (uint32_t)__shfl((int)front, (int)((8u - d + lane) & 63u));
                v[d] = lane >= d ? a : f;
            }
            /* M differs from the free-running map for 165 samples after a reset: there the samples before it are masked off */
            uint32_t qc;
            if (pos < rst + RA_SLOW_SPAN) {
                int64_t r_loc = (int64_t)rst - lane_base;
                r_loc = r_loc < -1024 ? -1024 : (r_loc > 1024 ? 1024 : r_loc);
                qc = ra_q32<true>(v, (int32_t)r_loc);
            } else {
                qc = ra_q32<false>(v, 0);
            }
            const uint32_t qp = (uint32_t)__shfl_up((int)qc, 1); /* lane 0 has nothing to look at (rm == 0) */
            const uint32_t m = ra_m32(qc, qp) & rm;
            const unsigned long long hit = __ballot(m != 0u);
            if (hit) {
                /* SEARCH_SYNC -> RECEIVING (ais_demod.c:147-155): first bit read at i + 4, then every 5 samples */
                const int l1 = __ffsll((long long)hit) - 1;
                const uint32_t ml = (uint32_t)__shfl((int)m, l1);
                const uint64_t i = (uint64_t)(cb + 32 * (int64_t)l1 + (int64_t)(__ffs((int)ml) - 1));
                mode = MFM_RUNAIS_RECEIVE;
                start = i;
                rd = i + 4;
                last_sample = getbit(i);
                hist8 = 0;
                cur_bit = 0;
            } else {
                const uint64_t nxt = (uint64_t)(cb + 32 * 64);
                pos = nxt < end ? nxt : end;
            }
        } else {
            /* ---- RECEIVING: 64 bit periods per step (ais_demod.c:160-213) ---- */
            if (rd >= end) {
                break;
            }
            const uint64_t avail = (end - 1 - rd) / 5 + 1;
            const uint32_t V = avail < 64 ? (uint32_t)avail : 64u;
            const bool valid = lane < V;
            const uint32_t raw = valid ? getbit(rd + 5ull * lane) : 0u;
            uint32_t prev = (uint32_t)__shfl_up((int)raw, 1);
            if (lane == 0) {
                prev = last_sample;
            }
            const uint32_t bit = valid ? ((prev ^ raw) ^ 1u) : 0u; /* NRZI: no transition = 1 (:170) */
            const unsigned long long B = __ballot((int)bit);
            /* the eight decoded bits ending at mine, oldest in bit 0; hist8 holds those before this step */
            const uint32_t w = lane >= 7 ? (uint32_t)(B >> (lane - 7)) & 0xffu
                                         : (uint32_t)((B << (7 - lane)) | (unsigned long long)(hist8 >> (lane + 1))) & 0xffu;
            const bool flag = valid && w == 0x7eu; /* :186 */
            /* a bit is written only while fewer than five 1s precede it since the rx reset (:175-184); hist8
             * starts at zero at that reset, so "the five bits before are all 1" says the same */
            const bool keep = valid && ((w >> 2) & 31u) != 31u;
            const unsigned long long K = __ballot(keep);
            const uint32_t kept_through = (uint32_t)__popcll(K & ((2ull << lane) - 1ull));
            const bool ends = valid && (flag || cur_bit + kept_through >= RA_MAX_BITS);
            const unsigned long long E = __ballot(ends);
            const uint32_t e = E ? (uint32_t)(__ffsll((long long)E) - 1) : V - 1;
            if (keep && bit && lane <= e) {
                const uint32_t p = cur_bit + kept_through - 1u; /* < 1280: e is the first lane to reach it */
                atomicOr(&pk[p >> 5], 1u << (p & 31u));
            }
            __syncthreads();
            if (E) {
                const uint32_t nbits = cur_bit + (uint32_t)__shfl((int)kept_through, (int)e);
                const uint32_t nr_bytes = nbits / 8u;
                const uint64_t at = rd + 5ull * e;
                if (nr_bytes >= 4u) { /* :190-206 */
                    const uint8_t *pb = reinterpret_cast<const uint8_t *>(pk);
                    uint32_t crc = 0xffffu;
                    for (uint32_t k = 0; k < nr_bytes - 2u; k++) {
                        crc = (crc >> 8) ^ crc_tab[(crc ^ pb[k]) & 0xffu];
                    }
                    crc = ~crc & 0xffffu;
                    const uint32_t rx_crc = (uint32_t)pb[nr_bytes - 2u] | ((uint32_t)pb[nr_bytes - 1u] << 8);
                    if (nev < max_ev) { /* always: the slot bound (mfm_runais_slots) */
                        mfm_runais_event *o = &ev[nev];
                        if (lane == 0) {
                            o->channel = run.channel;
                            o->fcs_valid = crc == rx_crc ? 1u : 0u;
                            o->nr_bytes = nr_bytes;
                            o->run = r;
                            o->stretch_window = stretch_window;
                            o->sample = at;
                            o->start_sample = start;
                        }
                        if (lane < RA_PACKET_WORDS) {
                            reinterpret_cast<uint32_t *>(o->bytes)[lane] = pk[lane];
                        }
                        nev++;
                    }
                }
                __syncthreads();
                if (lane < RA_PACKET_WORDS) {
                    pk[lane] = 0; /* :53-59 */
                }
                __syncthreads();
                mode = MFM_RUNAIS_SEARCH; /* :207-210: the detector restarts from zero at the next sample */
                pos = rst = at + 1;
            } else {
                cur_bit += (uint32_t)__popcll(K);
                hist8 = (uint32_t)__shfl((int)w, (int)(V - 1));
                last_sample = (uint32_t)__shfl((int)raw, (int)(V - 1));
                rd += 5ull * V;
            }
        }
    }
    /* every lane holds the whole state; lanes write their share of it */
    mfm_runais_state *dst = &A.run_state[r];
    if (lane < RA_PACKET_WORDS) {
        dst->packet[lane] = pk[lane];
    }
    if (lane == 0) { /* in the canonical form (mfm_runais_canon): what the mode does not use is zero */
        mfm_runais_state s;
        s.outs = end;
        s.stretch_window = stretch_window;
        s.pos = pos;
        s.r = rst;
        s.rd = rd;
        s.start = start;
        s.mode = mode;
        s.last_sample = last_sample;
        s.hist8 = hist8;
        s.cur_bit = cur_bit;
        mfm_runais_canon(s);
        dst->outs = s.outs;
        dst->stretch_window = s.stretch_window;
        dst->pos = s.pos;
        dst->r = s.r;
        dst->rd = s.rd;
        dst->start = s.start;
        dst->mode = s.mode;
        dst->last_sample = s.last_sample;
        dst->hist8 = s.hist8;
        dst->cur_bit = s.cur_bit;
        dst->has_stretch = 1;
        dst->reserved = 0;
        A.count[r] = nev;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void ra_evscan_kernel(const RaCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    /* 0 runs for a refused call; the total is at most the sum of the slots: within cap_events */
    const uint64_t total = mfm_run_count_scan(A.count, A.ev_base, A.ctl[1], lds);
    if (threadIdx.x == 0) {
        A.totals[RA_T_EVENTS] = total;
    }
}

__global__ __launch_bounds__(64) void ra_compact_kernel(const RaCall A)
{
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) {
        return;
    }
    constexpr uint32_t EW = sizeof(mfm_runais_event) / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.slots + A.slot_base[r]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(A.events + A.ev_base[r]);
    mfm_run_copy_words(src, dst, &A.count[r], EW);
}

__global__ __launch_bounds__(64) void ra_state_kernel(const RaCall A)
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
        for (uint32_t i = tid; i < RA_STATE_WORDS; i += blockDim.x) {
            nw[i] = old[i];
        }
        return;
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&A.run_state[last]);
    const uint32_t *seg = A.seg + A.seg_base[last];
    const uint32_t nr_out = A.runs[last].nr_out;
    for (uint32_t i = tid; i < RA_STATE_WORDS; i += blockDim.x) {
        nw[i] = i < RA_TAIL_WORD0 ? src[i] : mfm_runais_tail_word(seg, nr_out, i - RA_TAIL_WORD0);
    }
}

/* what create checks without a device; the capacities with the default filled in */
int ra_geometry(const mfm_runais_config &cfg, uint64_t *cap_events)
{
    const int rc = mfm_run_geometry(cfg);
    if (rc != MFM_OK) {
        return rc;
    }
    *cap_events = cfg.max_events ? cfg.max_events : (uint64_t)cfg.max_out_samples / MFM_RUNAIS_MIN_SPACING + cfg.max_runs;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *ra_refusal(uint64_t over, uint64_t err)
{
    return mfm_run_refusal(over, err, "the call's event bound (the sum of nr_out / 160 + 1 over its runs) exceeds max_events");
}

} /* namespace */

struct mfm_runais {
    mfm_runais_config cfg{};
    uint64_t cap_events = 0, seg_words = 0, max_blocks = 0;
    mfm_runais_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    mfm_runais_state *d_run_state = nullptr;
    uint32_t *d_seg = nullptr, *d_seg_base = nullptr, *d_slot_base = nullptr, *d_blk_base = nullptr, *d_count = nullptr, *d_ev_base = nullptr;
    uint32_t *d_chan_last = nullptr, *d_ctl = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runais_event *d_slots = nullptr, *d_events = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    MfmRunEnds ends; /* the stretch-end report (mfm_run_ends.h); off at create */
};

extern "C" {

int mfm_runais_create(struct mfm_runais **pa, const struct mfm_runais_config *cfg)
{
    if (!pa || !cfg) {
        return MFM_E_INVAL;
    }
    *pa = nullptr;
    uint64_t cap_events = 0;
    const int rc = ra_geometry(*cfg, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    mfm_runais *a = new (std::nothrow) mfm_runais();
    if (!a) {
        return MFM_E_NOMEM;
    }
    a->cfg = *cfg;
    a->cap_events = cap_events;
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    /* a run's segment has at most nr_out / 32 + 10 words and (that + 255) / 256 slicer workgroups */
    a->seg_words = (uint64_t)cfg->max_out_samples / 32u + 10ull * nruns;
    a->max_blocks = a->seg_words / RA_SLICE_NT + nruns;
    *pa = a; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&a->d_chan[i], C * sizeof(mfm_runais_state)));
        MFM_RUN_TRY(hipMemset(a->d_chan[i], 0, C * sizeof(mfm_runais_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&a->d_run_state, nruns * sizeof(mfm_runais_state)));
    MFM_RUN_TRY(hipMalloc(&a->d_seg, (size_t)a->seg_words * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_seg_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_slot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_blk_base, (nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_count, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_ev_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(a->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_ctl, 2 * 4));
    MFM_RUN_TRY(hipMemset(a->d_ctl, 0, 2 * 4));
    MFM_RUN_TRY(hipMalloc(&a->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(a->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&a->d_slots, (size_t)cap_events * sizeof(mfm_runais_event)));
    MFM_RUN_TRY(hipMalloc(&a->d_events, (size_t)cap_events * sizeof(mfm_runais_event)));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runais_destroy(struct mfm_runais **pa)
{
    if (!pa || !*pa) {
        return;
    }
    mfm_runais *a = *pa;
    (void)hipSetDevice(a->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(a->d_chan[0]);
    (void)hipFree(a->d_chan[1]);
    (void)hipFree(a->d_run_state);
    (void)hipFree(a->d_seg);
    (void)hipFree(a->d_seg_base);
    (void)hipFree(a->d_slot_base);
    (void)hipFree(a->d_blk_base);
    (void)hipFree(a->d_count);
    (void)hipFree(a->d_ev_base);
    (void)hipFree(a->d_chan_last);
    (void)hipFree(a->d_ctl);
    (void)hipFree(a->d_totals);
    (void)hipFree(a->d_slots);
    (void)hipFree(a->d_events);
    (void)mfm_internal_run_ends_set(&a->ends, MFM_RUN_ENDS_AIS, false, 0, 0);
    delete a;
    *pa = nullptr;
}

} /* extern "C" */

namespace {

/* one call in either form: d_payload (PCM) or d_bits (the resampler's bits form), the other NULL */
int ra_process(mfm_runais *a, const mfm_runrs_run *d_runs, const int16_t *d_payload, const uint32_t *d_bits, const uint64_t *d_totals, void *stream)
{
    if (!a || !d_runs || (!d_payload && !d_bits) || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(a, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = a->cur;
    const RaCall A{ d_runs,        d_payload,      d_bits,         d_totals,       a->d_chan[cur], a->d_chan[cur ^ 1u], a->d_run_state,
                    a->d_seg,      a->d_seg_base,  a->d_slot_base, a->d_blk_base,  a->d_count,          a->d_ev_base,
                    a->d_chan_last, a->d_ctl,      a->d_totals,    a->d_slots,     a->d_events,         a->cfg.nr_channels,
                    a->cfg.max_runs, a->cfg.max_out_samples, (uint32_t)a->cap_events };
    hipLaunchKernelGGL(ra_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    if (d_bits) { /* the word copy of mfm_run_bits.hip in the place of the slicer */
        const mfm_run_bits_slice B{ d_runs, d_bits, reinterpret_cast<const uint32_t *>(a->d_chan[cur]), a->d_blk_base, a->d_seg_base, a->d_ctl,
                                    a->d_seg, RA_STATE_WORDS, RA_TAIL_WORD0, MFM_RUNAIS_HIST_WORDS };
        if (mfm_internal_run_bits_slice(&B, (uint32_t)a->max_blocks, s) != MFM_OK) {
            MFM_RUN_TRY(hipGetLastError());
            return MFM_E_DEVICE;
        }
    } else {
        hipLaunchKernelGGL(ra_slice_kernel, dim3((uint32_t)a->max_blocks), dim3(RA_SLICE_NT), 0, s, A);
        MFM_RUN_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ra_walk_kernel, dim3(a->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(ra_evscan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(ra_compact_kernel, dim3(a->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    if (a->ends.on) { /* behind the walk, in front of the state kernel */
        const MfmRunEndsCall E{ d_runs, a->d_chan[cur], a->d_run_state, a->d_ctl, nullptr, a->cfg.nr_channels, a->cfg.max_runs };
        const int re = mfm_internal_run_ends_process(&a->ends, MFM_RUN_ENDS_AIS, &E, s);
        if (re != MFM_OK) {
            return re;
        }
    }
    hipLaunchKernelGGL(ra_state_kernel, dim3(a->cfg.nr_channels), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(a, s);
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_runais_process_device(struct mfm_runais *a, const struct mfm_runrs_run *d_runs, const int16_t *d_payload, const uint64_t *d_totals,
                              void *stream)
{
    if (!d_payload) {
        return MFM_E_INVAL;
    }
    return ra_process(a, d_runs, d_payload, nullptr, d_totals, stream);
}

int mfm_runais_process_bits_device(struct mfm_runais *a, const struct mfm_runrs_bits_view *view, void *stream)
{
    if (!a || !view || !view->d_bits) {
        return MFM_E_INVAL;
    }
    if (view->polarity != MFM_BITS_POS) {
        return mfm_run_fail(MFM_E_INVAL, "the burst AIS stage needs MFM_BITS_POS bits (bit = sample > 0)");
    }
    return ra_process(a, view->d_runs, nullptr, view->d_bits, view->d_totals, stream);
}

int mfm_runais_fetch(struct mfm_runais *a, struct mfm_runais_event *events, size_t max_events, size_t *nr_events)
{
    if (!a || !nr_events || (!events && max_events)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    if (!a->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(a->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(a->last_stream));
    uint64_t t[4];
    MFM_RUN_TRY(hipMemcpy(t, a->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, ra_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    *nr_events = (size_t)t[RA_T_EVENTS];
    if (t[RA_T_EVENTS] > max_events) {
        return MFM_E_NOMEM;
    }
    if (t[RA_T_EVENTS]) {
        MFM_RUN_TRY(hipMemcpy(events, a->d_events, (size_t)t[RA_T_EVENTS] * sizeof(mfm_runais_event), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runais_device_view(struct mfm_runais *a, const struct mfm_runais_event **d_events, const uint64_t **d_totals)
{
    if (!a) {
        return MFM_E_INVAL;
    }
    if (d_events) {
        *d_events = a->d_events;
    }
    if (d_totals) {
        *d_totals = a->d_totals;
    }
    return MFM_OK;
}

int mfm_hosttwin_runais_state_check(uint32_t nr_channels, const struct mfm_runais_state *state)
{
    return mfm_run_state_check(nr_channels, state, "AIS", mfm_runais_state_check);
}

int mfm_runais_fetch_state(struct mfm_runais *a, struct mfm_runais_state *state, size_t nr_channels)
{
    return mfm_run_fetch_state(a, state, nr_channels);
}

int mfm_runais_store_state(struct mfm_runais *a, const struct mfm_runais_state *state, size_t nr_channels)
{
    return mfm_run_store_state(a, state, nr_channels, mfm_hosttwin_runais_state_check);
}

/* ---- the stretch-end report: kernels and launchers in mfm_run_ends.hip ---- */

int mfm_runais_set_end_report(struct mfm_runais *a, int on)
{
    return mfm_run_ends_entry_set(a, MFM_RUN_ENDS_AIS, on, mfm_run_fail);
}

int mfm_runais_end_stretches_device(struct mfm_runais *a, void *stream)
{
    return mfm_run_ends_entry_flush(a, MFM_RUN_ENDS_AIS, nullptr, stream, mfm_run_fail);
}

int mfm_runais_fetch_ends(struct mfm_runais *a, struct mfm_runais_end *ends, size_t max_ends, size_t *nr_ends)
{
    return mfm_run_ends_entry_fetch(a, MFM_RUN_ENDS_AIS, ends, max_ends, nr_ends, mfm_run_fail, ra_refusal);
}

int mfm_runais_ends_view(struct mfm_runais *a, const struct mfm_runais_end **d_ends, const uint64_t **d_end_totals)
{
    return mfm_run_ends_entry_view(a, d_ends, d_end_totals, mfm_run_fail);
}

} /* extern "C" */

/* ---- the host twin: the same plan, segments and tail, the demodulator one sample at a time ---------------------------- */

namespace {

struct RaHostRun {
    const uint32_t *seg;
    int64_t ws;
    uint64_t rst;
    uint32_t raw(int64_t x) const /* the slicer's bit of stretch sample x */
    {
        const uint64_t o = (uint64_t)(x - ws);
        return (seg[o >> 5] >> (o & 31u)) & 1u;
    }
    uint32_t bit(int64_t x) const /* as the detector holds it: zero before the reset (ais_demod.c:44-50) */
    {
        return x < (int64_t)rst ? 0u : raw(x);
    }
    uint32_t q(int64_t u) const /* the register updated at u matches the preamble within two bits (:135-145) */
    {
        if (u < (int64_t)rst) {
            return 0;
        }
        uint32_t reg = 0;
        for (int k = 0; k < 32; k++) {
            const int64_t s = u - 5 * k;
            if (s >= (int64_t)rst) {
                reg |= ((bit(s) ^ bit(s - 5)) ^ 1u) << k;
            }
        }
        return __builtin_popcount(reg ^ RA_PREAMBLE) <= 2 ? 1u : 0u;
    }
};

uint16_t ra_host_crc(const uint8_t *p, size_t n) /* ais_demod.c:19-36 */
{
    uint32_t crc = 0xffffu;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int b = 0; b < 8; b++) {
            crc = (crc & 1u) ? ((crc >> 1) ^ 0x8408u) : (crc >> 1);
        }
    }
    return (uint16_t)(~crc & 0xffffu);
}

/* one run through the demodulator from state st (updated in place, all but the tail); events appended */
void ra_host_walk(mfm_runais_state &st, const uint32_t *seg, const mfm_runrs_run &run, uint32_t r, std::vector<mfm_runais_event> &out)
{
    RaHostRun h{ seg, (int64_t)run.first_out - (int64_t)MFM_RUNAIS_HIST_BITS, st.r };
    const uint64_t end = run.first_out + run.nr_out;
    for (;;) {
        if (st.mode == MFM_RUNAIS_SEARCH) {
            if (st.pos >= end) {
                break;
            }
            h.rst = st.r;
            uint32_t qh = 0;
            for (int j = 4; j >= 1; j--) {
                qh = (qh << 1) | h.q((int64_t)st.pos - j);
            }
            uint64_t t = st.pos;
            for (; t < end; t++) {
                qh = ((qh << 1) | h.q((int64_t)t)) & 31u;
                if (__builtin_popcount(qh) >= 3) {
                    break;
                }
            }
            if (t == end) {
                st.pos = end;
                continue;
            }
            st.mode = MFM_RUNAIS_RECEIVE; /* :147-155 */
            st.start = t;
            st.rd = t + 4;
            st.last_sample = h.raw((int64_t)t);
            st.hist8 = 0;
            st.cur_bit = 0;
        } else {
            if (st.rd >= end) {
                break;
            }
            const uint32_t raw = h.raw((int64_t)st.rd);
            const uint32_t bit = (st.last_sample ^ raw) ^ 1u; /* :170 */
            const uint32_t w = (st.hist8 >> 1) | (bit << 7);
            const bool flag = w == 0x7eu;
            if (((w >> 2) & 31u) != 31u) { /* :175-184 */
                if (bit) {
                    st.packet[st.cur_bit >> 5] |= 1u << (st.cur_bit & 31u);
                }
                st.cur_bit++;
            }
            if (flag || st.cur_bit >= RA_MAX_BITS) {
                const uint32_t nr_bytes = st.cur_bit / 8u;
                if (nr_bytes >= 4u) { /* :190-206 */
                    mfm_runais_event e;
                    memset(&e, 0, sizeof(e));
                    memcpy(e.bytes, st.packet, sizeof(e.bytes));
                    e.channel = run.channel;
                    e.fcs_valid = ra_host_crc(e.bytes, nr_bytes - 2u) == ((uint32_t)e.bytes[nr_bytes - 2u] | ((uint32_t)e.bytes[nr_bytes - 1u] << 8));
                    e.nr_bytes = nr_bytes;
                    e.run = r;
                    e.stretch_window = st.stretch_window;
                    e.sample = st.rd;
                    e.start_sample = st.start;
                    out.push_back(e);
                }
                memset(st.packet, 0, sizeof(st.packet));
                st.mode = MFM_RUNAIS_SEARCH;
                st.pos = st.r = st.rd + 1;
            } else {
                st.hist8 = w;
                st.last_sample = raw;
                st.rd += 5;
            }
        }
    }
    st.outs = end;
    st.has_stretch = 1;
    mfm_runais_canon(st);
}

} /* namespace */

namespace {

/* the host twin of one call in either form: bits != NULL is the resampler's bits form (totals[1] and out_offset in words) */
int ra_twin_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events, struct mfm_runais_state *state,
                 const struct mfm_runrs_run *runs, const int16_t *payload, const uint32_t *bits, bool words, const uint64_t *totals,
                 struct mfm_runais_event *events, size_t max_out, size_t *nr_events, uint32_t *flags,
                 struct mfm_runais_end *ends = nullptr, size_t max_ends = 0, size_t *nr_ends = nullptr) /* nr_ends: with the records */
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
    mfm_runais_config cfg{};
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = nr_channels;
    cfg.max_runs = max_runs;
    cfg.max_out_samples = max_out_samples;
    cfg.max_events = max_events;
    uint64_t cap_events = 0;
    const int rc = ra_geometry(cfg, &cap_events);
    if (rc != MFM_OK) {
        return rc;
    }
    uint64_t n, over, err, ts = 0; /* the plan pass */
    if (!mfm_run_twin_plan(totals, nr_channels, max_runs, max_out_samples, state, runs, words ? (const void *)bits : (const void *)payload, words,
                           [&](uint32_t nr_out) { ts += mfm_runais_slots(nr_out); }, &n, &over, &err)) {
        return MFM_E_INVAL;
    }
    if (!err && ts > cap_events) {
        over = MFM_RUNAIS_OVER_EVENTS;
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, ra_refusal(over, err));
    }
    /* every run from the state the call started with (only a channel's first run reads it); the state its last run leaves */
    std::vector<mfm_runais_event> out;
    std::vector<mfm_runais_state> left(n);
    std::vector<uint32_t> seg;
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        mfm_runais_state st;
        memset(&st, 0, sizeof(st));
        st.stretch_window = run.first_window;
        if (!(run.flags & MFM_RUNRS_BEGINS)) {
            st = state[run.channel];
        }
        seg.assign(mfm_runais_seg_words(run.nr_out), 0u);
        for (uint32_t k = 0; k < MFM_RUNAIS_HIST_WORDS; k++) {
            seg[k] = st.tail[k]; /* zeros for a beginning run */
        }
        if (words) { /* the slicer's word copy */
            for (uint32_t k = 0; k < (run.nr_out + 31u) / 32u; k++) {
                seg[MFM_RUNAIS_HIST_WORDS + k] = bits[run.out_offset + k];
            }
        } else {
            for (uint32_t j = 0; j < run.nr_out; j++) {
                if (payload[run.out_offset + j] > 0) {
                    seg[MFM_RUNAIS_HIST_WORDS + (j >> 5)] |= 1u << (j & 31u);
                }
            }
        }
        ra_host_walk(st, seg.data(), run, (uint32_t)r, out);
        for (uint32_t k = 0; k < MFM_RUNAIS_HIST_WORDS; k++) {
            st.tail[k] = mfm_runais_tail_word(seg.data(), run.nr_out, k);
        }
        left[r] = st;
    }
    *nr_events = out.size();
    if (out.size() > max_out) {
        return MFM_E_NOMEM; /* nothing written, the state included */
    }
    if (nr_ends) { /* from the state the call started with, before it moves */
        *nr_ends = mfm_run_ends_host_call(runs, n, state, left.data(), ends, 0, mfm_runais_end_of);
        if (*nr_ends > max_ends) {
            return MFM_E_NOMEM;
        }
        (void)mfm_run_ends_host_call(runs, n, state, left.data(), ends, max_ends, mfm_runais_end_of);
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            state[runs[r].channel] = left[r];
        }
    }
    if (!out.empty()) {
        memcpy(events, out.data(), out.size() * sizeof(mfm_runais_event));
    }
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_hosttwin_runais_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                             struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                             const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events, uint32_t *flags)
{
    return ra_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, payload, nullptr, false, totals, events, max_out,
                        nr_events, flags);
}

int mfm_hosttwin_runais_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                  struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const int16_t *payload,
                                  const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events, uint32_t *flags,
                                  struct mfm_runais_end *ends, size_t max_ends, size_t *nr_ends)
{
    if (!nr_ends) {
        return MFM_E_INVAL;
    }
    return ra_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, payload, nullptr, false, totals, events, max_out,
                        nr_events, flags, ends, max_ends, nr_ends);
}

int mfm_hosttwin_runais_end_stretches(uint32_t nr_channels, struct mfm_runais_state *state, struct mfm_runais_end *ends, size_t max_ends,
                                      size_t *nr_ends)
{
    return mfm_run_ends_host_flush(nr_channels, state, ends, max_ends, nr_ends, mfm_runais_end_of);
}

int mfm_hosttwin_runais_call_bits(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                  struct mfm_runais_state *state, const struct mfm_runrs_run *runs, const uint32_t *bits, uint32_t polarity,
                                  const uint64_t *totals, struct mfm_runais_event *events, size_t max_out, size_t *nr_events,
                                  uint32_t *flags)
{
    if (polarity != MFM_BITS_POS) {
        return mfm_run_fail(MFM_E_INVAL, "the burst AIS stage needs MFM_BITS_POS bits (bit = sample > 0)");
    }
    return ra_twin_call(nr_channels, max_runs, max_out_samples, max_events, state, runs, nullptr, bits, true, totals, events, max_out,
                        nr_events, flags);
}

} /* extern "C" */
