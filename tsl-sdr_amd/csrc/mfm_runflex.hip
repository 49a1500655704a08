/*
 * mfm_runflex.hip - the burst FLEX stage: the runs the burst resampler left in its dense payload go through the FLEX front
 * half (pager/pager_flex.c:129-171,264-525,1200-1345,1401-1455) on the device, one fresh decoder per stretch.  See
 * include/multifm_hip.h for the boundary and the event format, mfm_runflex.h for the segment layout, the ring, the slot
 * bounds, mfm_run_stage.h for the checks of a run, and mfm_flex.hip for the row stage whose match words, walk from event to event and frame
 * gather this file restates on ragged runs.
 *
 * The input is what mfm_runrs_device_view returns; how many runs and samples a call carries is read on the device, so the
 * host never waits and every launch is sized from the capacities fixed at create.
 *
 *   rf_plan_kernel     one block.  One pass over the runs: every run is checked (mfm_run_check_run) before anything of
 *                      the payload is read; exclusive scans of the runs' segment words, event slots, frame slots and slicer
 *                      workgroups; a channel's last run leaves its index for the ring and state kernels; the totals and flags.
 *   rf_slice_kernel    PCM int16 -> 1 bit per sample (sample >= 0).  A workgroup takes 256 words of one run's segment, which
 *                      it finds from its index by binary search in the scanned workgroup counts: the 10 history words (from
 *                      the channel's ring, or zeros), then 32 samples per lane as four 16-byte loads, the run's end one by one.
 *   rf_match_kernel    m, "a BS1 register reads 0xaaaaaaaa at this sample", over every segment: fx_match_kernel's arithmetic,
 *                      an AND of 32 funnel-shifted views 10 samples apart, the segment words and the 10 in front in LDS; and a
 *                      summary, one bit per segment word: "m is not zero here".
 *   rf_walk_kernel     one wave per run: fx_walk_kernel's SEARCH / SYNC1 / FRAME loop, positions stretch-relative, from the
 *                      carried state or a fresh one (SEARCH at sample 310).  With no run of matches open the summary steps
 *                      over 65 536 samples at a time.  The 112 sync samples are gathered with two ballots, from the payload
 *                      or, below the run's first output, from the ring.  Events go to the run's slot range, a frame leaves a
 *                      descriptor in the run's frame slot range.
 *   rf_evscan_kernel   one block: exclusive scans of the runs' event and frame counts, the totals.
 *   rf_compact_kernel  one wave per run: its events (frame_index made call-wide) and frame descriptors into the dense lists.
 *   rf_gather_kernel   one workgroup per frame found: every block symbol sliced once into an LDS byte (5632 at most), then the
 *                      88 x phases words built from LDS, as fx_gather_kernel does; samples from the payload or the ring.
 *   rf_ring_kernel     the last 32 768 outputs at most of a channel's last run into the channel's ring; not for a refused call.
 *   rf_state_kernel    one block per channel: the record of the channel's last run goes into the OTHER of two state buffers;
 *                      a channel without a run, and every channel of a refused call, copies its state over.
 *
 * Nothing is floating point and no atomic decides a placement.  The block scan, a thread's slice of the runs, the plan's head and the
 * host code around a call are mfm_run_stage.h's, shared with the other burst stages.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_bch.h"
#include "mfm_run_ends.h"
#include "mfm_runflex.h"

static_assert(sizeof(mfm_flex_event) == 88 && sizeof(mfm_runflex_event) == 104 && offsetof(mfm_runflex_event, run) == 88 &&
                  offsetof(mfm_runflex_event, stretch_window) == 96 && offsetof(mfm_runflex_event, frame_index) == 76,
              "struct mfm_runflex_event is struct mfm_flex_event and 16 bytes");
static_assert(sizeof(mfm_runflex_state) == 88 && offsetof(mfm_runflex_state, mode) == 32, "struct mfm_runflex_state");

namespace {

constexpr uint32_t RF_SLICE_NT = 256;         /* slicer: threads = segment words per workgroup */
constexpr uint32_t RF_GATHER_THREADS = 256;
constexpr uint32_t RF_RING_BLOCKS = 8;        /* workgroups per channel of the ring kernel */
constexpr uint32_t RF_T_EVENTS = 0, RF_T_FRAMES = 1; /* d_totals[], in front of MFM_RUN_T_OVERFLOW and MFM_RUN_T_INPUT */
constexpr uint32_t RF_HW = MFM_RUNFLEX_HIST_WORDS;
constexpr uint32_t RF_STATE_WORDS = sizeof(mfm_runflex_state) / 4;

/* a collected frame, as the walk leaves it for the gather kernel */
struct RfFrameDesc {
    uint64_t first;    /* stretch sample of the block's first symbol */
    uint32_t coding;
    int32_t range, delta;
    uint32_t run;      /* the run whose walk found it */
};

struct RfCall {
    const mfm_runrs_run *runs;
    const int16_t *payload;
    const uint64_t *rtotals;
    const mfm_runflex_state *chan_old;
    mfm_runflex_state *chan_new;
    mfm_runflex_state *run_state; /* [cap_runs] what a run's walk ends in */
    int16_t *ring;                /* [C][32768] */
    uint32_t *seg;                /* the runs' bit segments, one behind the other */
    uint32_t *plane;              /* m, laid out as seg */
    uint32_t *summ;               /* the summary: a run's words from (seg_base >> 5) + run index on, one bit per segment word */
    uint32_t *seg_base;           /* [cap_runs] first word of a run's segment */
    uint32_t *slot_base;          /* [cap_runs] first event slot of a run */
    uint32_t *fslot_base;         /* [cap_runs] first frame slot of a run */
    uint32_t *blk_base;           /* [cap_runs + 1] first slicer workgroup of a run */
    uint32_t *count;              /* [cap_runs][2] events, frames of a run */
    uint32_t *ev_base;            /* [cap_runs][2] their exclusive scans */
    uint32_t *chan_last;          /* [C] */
    uint32_t *ctl;                /* [0] workgroups of the slicer, [1] runs */
    uint64_t *totals;
    mfm_runflex_event *slots;     /* [cap_events] */
    mfm_runflex_event *events;    /* [cap_events] */
    RfFrameDesc *fslots;          /* [cap_frames] */
    RfFrameDesc *fdesc;           /* [cap_frames] dense */
    mfm_flex_frame_words *frames; /* [cap_frames] */
    const MfmBchTables *bch;
    uint32_t C, cap_runs, cap_out, cap_events, cap_frames;
};

/* PCM sample s of the stretch run `run` belongs to: the payload from the run's first output on, the channel's ring below */
__device__ __forceinline__ int rf_sample(const RfCall &A, const mfm_runrs_run &run, uint64_t s)
{
    /* one load either way: pick the address, not the value */
    const int16_t *in_run = A.payload + run.out_offset + (s - run.first_out);
    const int16_t *in_ring = A.ring + (size_t)run.channel * MFM_RUNFLEX_RING + (size_t)(s & (MFM_RUNFLEX_RING - 1u));
    return *(s >= run.first_out ? in_run : in_ring);
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rf_plan_kernel(const RfCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t n, E, over, err, r0, r1;
    if (!mfm_run_plan_head(A.rtotals, A.cap_out, A.cap_runs, A.totals, A.ctl, 2, &n, &E, &over, &err)) {
        return; /* nothing may be read */
    }
    mfm_run_slice(n, &r0, &r1);
    uint64_t so = 0, sw = 0, ss = 0, sf = 0, sb = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        const mfm_runrs_run run = A.runs[r];
        bad |= mfm_run_check_run(run, r ? &A.runs[r - 1] : nullptr, A.C, E, A.chan_old);
        const uint32_t w = mfm_runflex_seg_words(run.nr_out);
        so += run.nr_out;
        sw += w;
        ss += mfm_runflex_event_slots(run.nr_out);
        sf += mfm_runflex_frame_slots(run.nr_out);
        sb += (w + RF_SLICE_NT - 1u) / RF_SLICE_NT;
    }
    /* fewer than 2^28 runs of fewer than 2^32 outputs: every sum stays below 2^63 */
    uint64_t to, tws, tfb;
    (void)mfm_run_block_scan(so, lds, &to);
    /* a call that is not refused has fewer than 2^32 segment words, slots and workgroups (rf_geometry): two share a scan */
    const uint64_t bws = mfm_run_block_scan((sw & 0xffffffffull) | (ss << 32), lds, &tws);
    const uint64_t bfb = mfm_run_block_scan((sf & 0xffffffffull) | (sb << 32), lds, &tfb);
    uint64_t bw = bws & 0xffffffffull, bs = bws >> 32, bf = bfb & 0xffffffffull, bb = bfb >> 32;
    const uint64_t ts = tws >> 32, tf = tfb & 0xffffffffull, tb = tfb >> 32;
    if (__syncthreads_or((bad & MFM_RUNFLEX_IN_OUT_OF_STEP) != 0)) {
        err |= MFM_RUNFLEX_IN_OUT_OF_STEP;
    }
    /* ranges that overlap could ask for more than the segments hold */
    if (__syncthreads_or((bad & MFM_RUNFLEX_IN_BAD_RUNS) != 0) || to > A.cap_out) {
        err |= MFM_RUNFLEX_IN_BAD_RUNS;
    }
    if (!err && (ts > A.cap_events || tf > A.cap_frames)) {
        over = MFM_RUNFLEX_OVER_EVENTS;
    }
    const bool refused = over || err;
    if (!refused) { /* within the capacities: segment words, slots and workgroups all fit 32 bits (rf_geometry) */
#pragma unroll 1
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t nr_out = A.runs[r].nr_out, c = A.runs[r].channel;
            const uint32_t w = mfm_runflex_seg_words(nr_out);
            A.seg_base[r] = (uint32_t)bw;
            A.slot_base[r] = (uint32_t)bs;
            A.fslot_base[r] = (uint32_t)bf;
            A.blk_base[r] = (uint32_t)bb;
            bw += w;
            bs += mfm_runflex_event_slots(nr_out);
            bf += mfm_runflex_frame_slots(nr_out);
            bb += (w + RF_SLICE_NT - 1u) / RF_SLICE_NT;
            if (r + 1 == n || A.runs[r + 1].channel != c) {
                A.chan_last[c] = (uint32_t)r;
            }
        }
    }
    if (threadIdx.x == 0) {
        A.totals[RF_T_EVENTS] = 0; /* the event scan */
        A.totals[RF_T_FRAMES] = 0;
        A.totals[MFM_RUN_T_OVERFLOW] = over;
        A.totals[MFM_RUN_T_INPUT] = err;
        if (!refused) {
            A.blk_base[n] = (uint32_t)tb;
        }
        A.ctl[0] = refused ? 0u : (uint32_t)tb;
        A.ctl[1] = refused ? 0u : (uint32_t)n;
    }
}

struct __attribute__((packed, aligned(2))) RfPcm8 { /* eight samples as one 16-byte access */
    uint32_t d[4];
};

__device__ __forceinline__ uint32_t rf_pos2(uint32_t d) /* the bits of two samples: sample >= 0 (pager_flex.c:137) */
{
    return ((~d >> 15) & 1u) | ((~d >> 30) & 2u);
}

/* the run of slicer workgroup b: the last r with blk_base[r] <= b (every run has at least one) */
__device__ __forceinline__ uint32_t rf_run_of_block(const RfCall &A, uint32_t b)
{
    uint32_t lo = 0, hi = A.ctl[1];
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.blk_base[mid] <= b) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__global__ __launch_bounds__(RF_SLICE_NT) void rf_slice_kernel(const RfCall A)
{
    const uint32_t b = blockIdx.x;
    if (b >= A.ctl[0]) { /* surplus workgroups: the launch is sized from the capacity */
        return;
    }
    const uint32_t r = rf_run_of_block(A, b);
    const mfm_runrs_run run = A.runs[r];
    const uint32_t w = (b - A.blk_base[r]) * RF_SLICE_NT + threadIdx.x;
    if (w >= mfm_runflex_seg_words(run.nr_out)) {
        return;
    }
    uint32_t word = 0;
    if (w < RF_HW) {
        if (!(run.flags & MFM_RUNRS_BEGINS)) { /* the 320 stretch samples in front of the run, as far as they exist */
            const int16_t *ring = A.ring + (size_t)run.channel * MFM_RUNFLEX_RING;
            for (uint32_t i = 0; i < 32u; i++) {
                const uint64_t back = MFM_RUNFLEX_HIST_BITS - (32u * w + i); /* 320 .. 1 */
                if (run.first_out >= back) {
                    word |= (ring[(run.first_out - back) & (MFM_RUNFLEX_RING - 1u)] >= 0 ? 1u : 0u) << i;
                }
            }
        }
    } else {
        const uint32_t j0 = (w - RF_HW) * 32u;
        const int16_t *x = A.payload + run.out_offset; /* [out_offset, out_offset + nr_out) lies within the totals (the plan) */
        if (j0 < run.nr_out && run.nr_out - j0 >= 32u) {
#pragma unroll
            for (uint32_t g = 0; g < 4; g++) {
                const RfPcm8 v = *reinterpret_cast<const RfPcm8 *>(x + j0 + 8u * g);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    word |= rf_pos2(v.d[q]) << (8u * g + 2u * q);
                }
            }
        } else { /* the run's last samples; the padding word stays zero */
            for (uint32_t i = 0; i < 32u && j0 + i < run.nr_out; i++) {
                word |= (x[j0 + i] >= 0 ? 1u : 0u) << i;
            }
        }
    }
    A.seg[A.seg_base[r] + w] = word;
}

/* m and the summary of the 256 segment words the slicer's workgroup of the same index wrote */
__global__ __launch_bounds__(RF_SLICE_NT) void rf_match_kernel(const RfCall A)
{
    __shared__ uint32_t tile[RF_HW + RF_SLICE_NT + 2];
    const uint32_t b = blockIdx.x;
    if (b >= A.ctl[0]) {
        return;
    }
    const uint32_t r = rf_run_of_block(A, b);
    const uint32_t nr_out = A.runs[r].nr_out;
    const uint32_t nw = mfm_runflex_seg_words(nr_out);
    const uint32_t w_blk = (b - A.blk_base[r]) * RF_SLICE_NT; /* < nw: the run has ceil(nw / 256) workgroups */
    const uint32_t base = A.seg_base[r];
    const uint32_t *bits = A.seg + base;
    for (uint32_t k = threadIdx.x; k < RF_HW + RF_SLICE_NT + 2u; k += RF_SLICE_NT) {
        const int64_t q = (int64_t)w_blk - (int64_t)RF_HW + (int64_t)k;
        tile[k] = q >= 0 && q < (int64_t)nw ? bits[q] : 0u;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x, w = w_blk + t;
    const bool in = w < nw;
    /* register bit k (k = 0 newest) is the sign bit 10 k samples back; BS1 wants a one at every odd k */
    uint32_t m = 0xffffffffu;
#pragma unroll
    for (uint32_t k = 0; k < 32; k++) {
        const uint32_t off = 32u * RF_HW + 32u * t - 10u * k;
        const uint32_t v = __funnelshift_r(tile[off >> 5], tile[(off >> 5) + 1], off & 31u);
        m &= (k & 1u) ? v : ~v;
    }
    /* only the run's own samples: not the history words, not the bits behind its last output */
    const int64_t j0 = 32 * ((int64_t)w - (int64_t)RF_HW);
    if (j0 < 0 || j0 >= (int64_t)nr_out) {
        m = 0;
    } else if ((int64_t)nr_out - j0 < 32) {
        m &= 0xffffffffu >> (32u - (uint32_t)((int64_t)nr_out - j0));
    }
    if (in) {
        A.plane[base + w] = m;
    }
    const uint32_t lane = t & 63u;
    const unsigned long long any = __ballot(in && m != 0u);
    if ((lane == 0 || lane == 32) && in) {
        A.summ[(base >> 5) + r + (w >> 5)] = (uint32_t)(any >> lane);
    }
}

__device__ __forceinline__ int rf_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v += __shfl_xor(v, d);
    }
    return v;
}

/* one wave per run: pager_flex_on_pcm from event to event as fx_walk_kernel walks it, positions stretch-relative */
__global__ __launch_bounds__(64) void rf_walk_kernel(const RfCall A)
{
    __shared__ MfmBchTables bch_s;
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) { /* surplus waves, and every wave of a refused call */
        return;
    }
    const mfm_runrs_run run = A.runs[r];
    const uint32_t c = run.channel;
    const uint64_t F = run.first_out, end = F + run.nr_out;
    const uint32_t nw = mfm_runflex_seg_words(run.nr_out), nsumm = (nw + 31u) / 32u;
    const uint32_t *M = A.plane + A.seg_base[r];
    const uint32_t *summ = A.summ + (A.seg_base[r] >> 5) + r;
    const uint32_t max_ev = mfm_runflex_event_slots(run.nr_out), max_fw = mfm_runflex_frame_slots(run.nr_out);
    mfm_runflex_event *ev = A.slots + A.slot_base[r];
    RfFrameDesc *fd = A.fslots + A.fslot_base[r];
    bool have_bch = false;
    /* a fresh decoder: the registers zero-filled "before sample 0", so the search opens at sample 310 (pager_flex_new) */
    mfm_runflex_state S;
    if (run.flags & MFM_RUNRS_BEGINS) {
        S = mfm_runflex_state{};
        S.p = MFM_RUNFLEX_DEAD - 1u;
        S.stretch_window = run.first_window;
    } else {
        S = A.chan_old[c];
    }
    uint32_t nev = 0, nfw = 0;
    auto emit = [&](uint32_t type, uint64_t sample, uint32_t fiw_rc, uint32_t frame_index) {
        if (nev < max_ev && lane == 0) { /* always: the slot bound (mfm_runflex_event_slots) */
            const bool known = S.coding < 4u;
            mfm_runflex_event e;
            e.type = type;
            e.channel = c;
            e.sample = sample;
            e.sync_sample = type == MFM_FLEX_EV_FRAME ? S.j : 0;
            e.coding = S.coding;
            e.baud = known ? mfm_runflex_coding(S.coding).baud : 0;
            e.eye = S.eye;
            e.a = S.a;
            e.b = S.b;
            e.inv_a = S.inv_a;
            e.fiw_raw = S.fiw_raw;
            e.fiw = S.fiw;
            e.fiw_rc = fiw_rc;
            e.sample_range = S.sample_range;
            e.sample_delta = S.sample_delta;
            e.cycle = S.cycle;
            e.frame = S.frame;
            e.frame_index = frame_index;
            e.nr_phases = known ? mfm_runflex_coding(S.coding).nr_phases : 0;
            e.reserved = 0;
            e.run = r;
            e.reserved2 = 0;
            e.stretch_window = S.stretch_window;
            ev[nev] = e;
        }
        nev++;
    };

    for (;;) {
        if (S.mode == MFM_RUNFLEX_SEARCH) {
            bool opened = false;
            while (S.p < end) { /* p >= F: a search never falls behind the outputs seen */
                if (S.run == 0) {
                    /* nothing open: go to the next set bit of m.  First the rest of the word p is in ... */
                    const uint32_t o = (uint32_t)(S.p - F);
                    const uint32_t i = RF_HW + (o >> 5);
                    const uint32_t head = M[i] & (0xffffffffu << (o & 31u));
                    if (head != 0) {
                        S.p = F + (o & ~31u) + ((uint32_t)__ffs((int)head) - 1u); /* < end: m is masked there */
                    } else {
                        /* ... then whole words through the summary, 64 x 32 words = 65 536 samples per step */
                        const uint32_t j = i + 1u, sj = j >> 5;
                        uint32_t v = sj + lane < nsumm ? summ[sj + lane] : 0u;
                        if (lane == 0) {
                            v &= 0xffffffffu << (j & 31u);
                        }
                        const unsigned long long nz = __ballot(v != 0u);
                        if (nz == 0) {
                            const uint64_t next = F + 32ull * (((uint64_t)(sj + 64u) << 5) - RF_HW);
                            S.p = next < end ? next : end; /* what lies beyond `end` belongs to the next run */
                            continue;
                        }
                        const int fl = __ffsll((long long)nz) - 1;
                        const uint32_t fv = (uint32_t)__shfl((int)v, fl);
                        const uint32_t wi = ((sj + (uint32_t)fl) << 5) + ((uint32_t)__ffs((int)fv) - 1u);
                        S.p = F + 32ull * (wi - RF_HW) + ((uint32_t)__ffs((int)M[wi]) - 1u);
                    }
                }
                /* count the run on from p, one word at a time */
                const uint32_t o = (uint32_t)(S.p - F), sh = o & 31u;
                const uint32_t inv = ~(M[RF_HW + (o >> 5)] >> sh);
                uint32_t avail = 32u - sh;
                if (end - S.p < avail) {
                    avail = (uint32_t)(end - S.p);
                }
                uint32_t ones = inv == 0 ? 32u : (uint32_t)__ffs((int)inv) - 1u;
                if (ones > avail) {
                    ones = avail;
                }
                S.run += ones;
                S.p += ones;
                if (ones < avail) {
                    /* sample p does not match: the run is over (pager_flex.c:328-344) */
                    const uint32_t cnt = S.run & 255u;
                    S.run = 0;
                    if (cnt >= 3) {
                        S.mode = MFM_RUNFLEX_SYNC1;
                        S.j = S.p;
                        S.eye = cnt;
                        opened = true;
                        break;
                    }
                    S.p += 1;
                }
            }
            if (!opened) {
                break; /* out of samples; a run that is still open goes on in the next call */
            }
        }

        if (S.mode == MFM_RUNFLEX_SYNC1) {
            /* the sample counter was set to run / 2 at j and a bit is taken whenever it wraps to 0 (:339,:348) */
            const uint64_t s0 = S.j + (10u - ((S.eye / 2u) % 10u));
            if (s0 + 790 >= end) {
                break;
            }
            const bool have_fiw = s0 + 1110 < end;
            const int v0 = rf_sample(A, run, s0 + 10 * lane); /* bits 0..63 */
            const uint32_t k1 = 64 + lane;                    /* bits 64..111 */
            const bool use1 = k1 < 80 || (have_fiw && k1 < 112);
            const int v1 = use1 ? rf_sample(A, run, s0 + 10 * k1) : 0;
            const uint64_t bal0 = __ballot(v0 >= 0), bal1 = __ballot(use1 && v1 >= 0);
            S.a = __brev((uint32_t)bal0);                                   /* shifted in MSB first (:349) */
            S.b = __brev((uint32_t)(bal0 >> 32) & 0xffffu) >> 16;
            S.inv_a = __brev((uint32_t)(bal0 >> 48) | ((uint32_t)bal1 << 16));
            S.fiw_raw = 0;
            S.fiw = 0;
            S.sample_range = 0;
            S.sample_delta = 0;
            S.cycle = 0;
            S.frame = 0;
            S.coding = mfm_runflex_find_coding(S.a);
            if (S.coding == 0xffffffffu) {
                emit(MFM_FLEX_EV_BAD_BAUD, s0 + 790, 0, 0);
                S.mode = MFM_RUNFLEX_SEARCH;
                S.run = 0;
                S.p = s0 + 790 + MFM_RUNFLEX_DEAD;
                continue;
            }
            if (!have_fiw) {
                break;
            }
            S.fiw_raw = (uint32_t)(bal1 >> 16); /* shifted in LSB first (:422) */
            /* swing of the 112 sync samples (:352-358, :438-442) */
            const bool in1 = k1 < 112;
            const int sum_hi = rf_wave_sum((v0 > 0 ? v0 : 0) + (in1 && v1 > 0 ? v1 : 0));
            const int sum_lo = rf_wave_sum((v0 <= 0 ? v0 : 0) + (in1 && v1 <= 0 ? v1 : 0));
            const int n_hi = rf_wave_sum((v0 > 0) + (in1 && v1 > 0));
            const int n_lo = rf_wave_sum((v0 <= 0) + (in1 && v1 <= 0));
            const uint64_t f = s0 + 1110;
            uint32_t rc;
            if (n_hi == 0 || n_lo == 0) {
                rc = 3;
            } else {
                const int high = (int16_t)(sum_hi / n_hi), low = (int16_t)(sum_lo / n_lo);
                S.sample_range = (int16_t)(high - low);
                S.sample_delta = (int16_t)(high - S.sample_range / 2);
                uint32_t bad;
                if (!have_bch) { /* copied on the first frame information word of the run */
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.bch);
                    uint32_t *dst = reinterpret_cast<uint32_t *>(&bch_s);
                    for (uint32_t i = lane; i < sizeof(MfmBchTables) / 4u; i += 64u) {
                        dst[i] = src[i];
                    }
                    have_bch = true; /* one wave: its LDS writes are visible to its later reads in program order */
                }
                S.fiw = mfm_bch_fix(&bch_s, S.fiw_raw & 0x7fffffffu, &bad); /* :1319-1327 */
                if (bad) {
                    rc = 1;
                } else if (mfm_runflex_checksum(S.fiw) != 0xfu) {
                    rc = 2;
                } else {
                    rc = 0;
                    S.cycle = (S.fiw >> 4) & 0xfu;
                    S.frame = (S.fiw >> 8) & 0x7fu;
                }
            }
            if (rc != 0) {
                emit(MFM_FLEX_EV_BAD_FIW, f, rc, 0);
                S.mode = MFM_RUNFLEX_SEARCH;
                S.run = 0;
                S.p = f + MFM_RUNFLEX_DEAD;
                continue;
            }
            S.mode = MFM_RUNFLEX_FRAME;
            S.j = f;
        }

        if (S.mode == MFM_RUNFLEX_FRAME) {
            const MfmRunflexCoding cd = mfm_runflex_coding(S.coding);
            const uint32_t step = cd.skip + 1u;
            /* first processed sample after f is f + skip + fudge + 1 (:1421-1423, :1410-1451), then one per `step` */
            const uint64_t first = S.j + step + cd.fudge + (uint64_t)cd.sync2 * step;
            const uint64_t e = first + (uint64_t)(cd.symbols - 1u) * step;
            if (e >= end) {
                break;
            }
            if (nfw < max_fw && lane == 0) { /* always: the slot bound (mfm_runflex_frame_slots) */
                fd[nfw] = RfFrameDesc{ first, S.coding, S.sample_range, S.sample_delta, r };
            }
            emit(MFM_FLEX_EV_FRAME, e, 0, nfw);
            nfw++;
            S.mode = MFM_RUNFLEX_SEARCH; /* _pager_flex_reset_sync (:1308) */
            S.run = 0;
            S.p = e + MFM_RUNFLEX_DEAD;
        }
    }

    if (lane == 0) {
        S.outs = end;
        S.has_stretch = 1;
        mfm_runflex_canon(S);
        A.run_state[r] = S;
        A.count[2 * r] = nev < max_ev ? nev : max_ev;
        A.count[2 * r + 1] = nfw < max_fw ? nfw : max_fw;
    }
}

__global__ __launch_bounds__(MFM_RUN_SCAN_THREADS) void rf_evscan_kernel(const RfCall A)
{
    __shared__ uint64_t lds[MFM_RUN_SCAN_THREADS / 64];
    uint64_t r0, r1;
    mfm_run_slice<uint64_t>(A.ctl[1], &r0, &r1); /* 0 runs for a refused call */
    uint64_t s = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        s += (uint64_t)A.count[2 * r] | ((uint64_t)A.count[2 * r + 1] << 32);
    }
    uint64_t total;
    uint64_t base = mfm_run_block_scan(s, lds, &total); /* at most the sums of the slots: within cap_events and cap_frames */
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        A.ev_base[2 * r] = (uint32_t)base;
        A.ev_base[2 * r + 1] = (uint32_t)(base >> 32);
        base += (uint64_t)A.count[2 * r] | ((uint64_t)A.count[2 * r + 1] << 32);
    }
    if (threadIdx.x == 0) {
        A.totals[RF_T_EVENTS] = total & 0xffffffffull;
        A.totals[RF_T_FRAMES] = total >> 32;
    }
}

__global__ __launch_bounds__(64) void rf_compact_kernel(const RfCall A)
{
    const uint32_t r = blockIdx.x;
    if (r >= A.ctl[1]) {
        return;
    }
    constexpr uint32_t EW = sizeof(mfm_runflex_event) / 4, FI = offsetof(mfm_runflex_event, frame_index) / 4;
    const uint32_t fbase = A.ev_base[2 * r + 1];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.slots + A.slot_base[r]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(A.events + A.ev_base[2 * r]);
    for (uint32_t i = threadIdx.x; i < A.count[2 * r] * EW; i += blockDim.x) {
        const uint32_t k = i % EW;
        /* frame_index goes from the run's list to the call's; `type` is an event's first word */
        dst[i] = src[i] + (k == FI && src[i - k] == MFM_FLEX_EV_FRAME ? fbase : 0u);
    }
    for (uint32_t i = threadIdx.x; i < A.count[2 * r + 1]; i += blockDim.x) {
        A.fdesc[fbase + i] = A.fslots[A.fslot_base[r] + i];
    }
}

/*
 * The words of the frames the walks found, one workgroup per frame.  Every symbol of the block is sliced once (consecutive
 * threads take consecutive symbols, 10 or 20 bytes apart) into one LDS byte, then the 88 x phases words are built from LDS:
 * bit jb of word 8 b + i of a phase is bit 256 b + 8 jb + i of that phase.
 */
__global__ __launch_bounds__(RF_GATHER_THREADS) void rf_gather_kernel(const RfCall A)
{
    __shared__ uint8_t sym[5632];
    const uint32_t g = blockIdx.x;
    if (g >= A.totals[RF_T_FRAMES]) { /* surplus workgroups; a refused call has no frame */
        return;
    }
    const RfFrameDesc d = A.fdesc[g];
    const mfm_runrs_run run = A.runs[d.run];
    const MfmRunflexCoding cd = mfm_runflex_coding(d.coding);
    const uint32_t step = cd.skip + 1u;
    const bool four = cd.levels == 4u;
    uint32_t *out = &A.frames[g].words[0][0];
#pragma unroll 4
    for (uint32_t k = threadIdx.x; k < cd.symbols; k += RF_GATHER_THREADS) {
        const int v = rf_sample(A, run, d.first + (uint64_t)k * step);
        sym[k] = (uint8_t)(four ? mfm_runflex_slice4(v, d.delta, d.range) : (uint32_t)(v >= 0)); /* 2-level: 1 == symbol (:1246) */
    }
    __syncthreads();
    for (uint32_t item = threadIdx.x; item < 4 * MFM_FLEX_PHASE_WORDS; item += RF_GATHER_THREADS) {
        const uint32_t q = item / MFM_FLEX_PHASE_WORDS, w = item % MFM_FLEX_PHASE_WORDS;
        uint32_t mul, add, sel;
        const bool present = mfm_runflex_phase_map(cd, q, &mul, &add, &sel);
        uint32_t word = 0;
        if (present) {
            const uint32_t n0 = (w >> 3) * 256 + (w & 7);
#pragma unroll
            for (uint32_t jb = 0; jb < 32; jb++) {
                word |= (((uint32_t)sym[(n0 + 8 * jb) * mul + add] >> sel) & 1u) << jb;
            }
        }
        out[item] = word;
    }
}

/* grid (RF_RING_BLOCKS, C): the last min(nr_out, 32768) outputs of the channel's last run into the channel's ring */
__global__ __launch_bounds__(256) void rf_ring_kernel(const RfCall A)
{
    const uint32_t c = blockIdx.y;
    const uint32_t last = A.chan_last[c];
    if (last == MFM_RUN_NONE || A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0) {
        return; /* a refused call wrote no chan_last; the test on the totals states the rule */
    }
    const mfm_runrs_run run = A.runs[last];
    const uint32_t cnt = run.nr_out < MFM_RUNFLEX_RING ? run.nr_out : MFM_RUNFLEX_RING;
    int16_t *ring = A.ring + (size_t)c * MFM_RUNFLEX_RING;
    const int16_t *x = A.payload + run.out_offset;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < cnt; k += RF_RING_BLOCKS * 256u) {
        const uint32_t off = run.nr_out - cnt + k;
        ring[(run.first_out + off) & (MFM_RUNFLEX_RING - 1u)] = x[off];
    }
}

__global__ __launch_bounds__(64) void rf_state_kernel(const RfCall A)
{
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t last = A.chan_last[c];
    const bool refused = A.totals[MFM_RUN_T_OVERFLOW] != 0 || A.totals[MFM_RUN_T_INPUT] != 0;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(last == MFM_RUN_NONE || refused ? &A.chan_old[c] : &A.run_state[last]);
    uint32_t *nw = reinterpret_cast<uint32_t *>(&A.chan_new[c]);
    if (tid < RF_STATE_WORDS) {
        nw[tid] = src[tid];
    }
    if (tid == 0) {
        A.chan_last[c] = MFM_RUN_NONE; /* for the next call */
    }
}

/* what create checks without a device; the capacities with the defaults filled in */
int rf_geometry(const mfm_runflex_config &cfg, uint64_t *cap_events, uint64_t *cap_frames)
{
    const int rc = mfm_run_geometry(cfg);
    if (rc != MFM_OK) {
        return rc;
    }
    /* the sums of the slots over max_runs runs that share max_out_samples outputs, at most */
    *cap_events = cfg.max_events ? cfg.max_events : (uint64_t)cfg.max_out_samples / MFM_RUNFLEX_EVENT_SPACING + cfg.max_runs;
    *cap_frames = cfg.max_frames ? cfg.max_frames : (uint64_t)cfg.max_out_samples / MFM_RUNFLEX_FRAME_SPACING + cfg.max_runs;
    return MFM_OK;
}

/* the message of a refused call, as fetch and the host twin give it */
const char *rf_refusal(uint64_t over, uint64_t err)
{
    return mfm_run_refusal(over, err, "the call's event bound (the sum of nr_out / 1105 + 1 over its runs) exceeds max_events, or its frame bound (nr_out / 29985 + 1) max_frames");
}

} /* namespace */

struct mfm_runflex {
    mfm_runflex_config cfg{};
    uint64_t cap_events = 0, cap_frames = 0, seg_words = 0, max_blocks = 0;
    mfm_runflex_state *d_chan[2] = { nullptr, nullptr }; /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint32_t cur = 0;
    mfm_runflex_state *d_run_state = nullptr;
    int16_t *d_ring = nullptr;
    uint32_t *d_seg = nullptr, *d_plane = nullptr, *d_summ = nullptr;
    uint32_t *d_seg_base = nullptr, *d_slot_base = nullptr, *d_fslot_base = nullptr, *d_blk_base = nullptr, *d_count = nullptr, *d_ev_base = nullptr;
    uint32_t *d_chan_last = nullptr, *d_ctl = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_runflex_event *d_slots = nullptr, *d_events = nullptr;
    RfFrameDesc *d_fslots = nullptr, *d_fdesc = nullptr;
    mfm_flex_frame_words *d_frames = nullptr;
    MfmBchTables *d_bch = nullptr; /* owned by mfm_pocsag.hip, one per device */
    hipStream_t last_stream = nullptr;
    bool have_call = false;
    MfmRunEnds ends; /* the stretch-end report (mfm_run_ends.h); off at create */
};

extern "C" {

int mfm_runflex_create(struct mfm_runflex **pf, const struct mfm_runflex_config *cfg)
{
    if (!pf || !cfg) {
        return MFM_E_INVAL;
    }
    *pf = nullptr;
    uint64_t cap_events = 0, cap_frames = 0;
    const int rc = rf_geometry(*cfg, &cap_events, &cap_frames);
    if (rc != MFM_OK) {
        return rc;
    }
    MfmBchTables *d_bch = nullptr;
    const int rb = mfm_internal_bch_device_tables(cfg->device, &d_bch);
    if (rb != MFM_OK) {
        return rb; /* no CPU path */
    }
    mfm_runflex *p = new (std::nothrow) mfm_runflex();
    if (!p) {
        return MFM_E_NOMEM;
    }
    p->cfg = *cfg;
    p->cap_events = cap_events;
    p->cap_frames = cap_frames;
    p->d_bch = d_bch;
    const size_t C = cfg->nr_channels, nruns = cfg->max_runs;
    /* a run's segment has at most nr_out / 32 + 12 words and (that + 255) / 256 slicer workgroups */
    p->seg_words = (uint64_t)cfg->max_out_samples / 32u + (MFM_RUNFLEX_HIST_WORDS + 2ull) * nruns;
    p->max_blocks = p->seg_words / RF_SLICE_NT + nruns;
    if (p->seg_words >= (1ull << 32) || p->max_blocks >= (1ull << 31) || cap_events >= (1ull << 32) || cap_frames >= (1ull << 31)) {
        delete p;
        return mfm_run_fail(MFM_E_INVAL, "max_runs and max_out_samples together ask for 2^32 segment words or more");
    }
    *pf = p; /* from here on the caller's destroy frees what was allocated */
    MFM_RUN_TRY(hipSetDevice(cfg->device));
    for (int i = 0; i < 2; i++) {
        MFM_RUN_TRY(hipMalloc(&p->d_chan[i], C * sizeof(mfm_runflex_state)));
        MFM_RUN_TRY(hipMemset(p->d_chan[i], 0, C * sizeof(mfm_runflex_state))); /* no stretch */
    }
    MFM_RUN_TRY(hipMalloc(&p->d_ring, C * MFM_RUNFLEX_RING * sizeof(int16_t)));
    MFM_RUN_TRY(hipMemset(p->d_ring, 0, C * MFM_RUNFLEX_RING * sizeof(int16_t)));
    MFM_RUN_TRY(hipMalloc(&p->d_run_state, nruns * sizeof(mfm_runflex_state)));
    MFM_RUN_TRY(hipMalloc(&p->d_seg, (size_t)p->seg_words * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_plane, (size_t)p->seg_words * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_summ, ((size_t)p->seg_words / 32 + 2 * nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_seg_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_slot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_fslot_base, nruns * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_blk_base, (nruns + 1) * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_count, nruns * 8));
    MFM_RUN_TRY(hipMalloc(&p->d_ev_base, nruns * 8));
    MFM_RUN_TRY(hipMalloc(&p->d_chan_last, C * 4));
    MFM_RUN_TRY(hipMemset(p->d_chan_last, 0xff, C * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_ctl, 2 * 4));
    MFM_RUN_TRY(hipMemset(p->d_ctl, 0, 2 * 4));
    MFM_RUN_TRY(hipMalloc(&p->d_totals, 4 * 8));
    MFM_RUN_TRY(hipMemset(p->d_totals, 0, 4 * 8));
    MFM_RUN_TRY(hipMalloc(&p->d_slots, (size_t)cap_events * sizeof(mfm_runflex_event)));
    MFM_RUN_TRY(hipMalloc(&p->d_events, (size_t)cap_events * sizeof(mfm_runflex_event)));
    MFM_RUN_TRY(hipMalloc(&p->d_fslots, (size_t)cap_frames * sizeof(RfFrameDesc)));
    MFM_RUN_TRY(hipMalloc(&p->d_fdesc, (size_t)cap_frames * sizeof(RfFrameDesc)));
    MFM_RUN_TRY(hipMalloc(&p->d_frames, (size_t)cap_frames * sizeof(mfm_flex_frame_words)));
    MFM_RUN_TRY(hipDeviceSynchronize());
    return MFM_OK;
}

void mfm_runflex_destroy(struct mfm_runflex **pf)
{
    if (!pf || !*pf) {
        return;
    }
    mfm_runflex *p = *pf;
    (void)hipSetDevice(p->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->d_chan[0]);
    (void)hipFree(p->d_chan[1]);
    (void)hipFree(p->d_ring);
    (void)hipFree(p->d_run_state);
    (void)hipFree(p->d_seg);
    (void)hipFree(p->d_plane);
    (void)hipFree(p->d_summ);
    (void)hipFree(p->d_seg_base);
    (void)hipFree(p->d_slot_base);
    (void)hipFree(p->d_fslot_base);
    (void)hipFree(p->d_blk_base);
    (void)hipFree(p->d_count);
    (void)hipFree(p->d_ev_base);
    (void)hipFree(p->d_chan_last);
    (void)hipFree(p->d_ctl);
    (void)hipFree(p->d_totals);
    (void)hipFree(p->d_slots);
    (void)hipFree(p->d_events);
    (void)hipFree(p->d_fslots);
    (void)hipFree(p->d_fdesc);
    (void)hipFree(p->d_frames);
    (void)mfm_internal_run_ends_set(&p->ends, MFM_RUN_ENDS_FLEX, false, 0, 0);
    delete p;
    *pf = nullptr;
}

int mfm_runflex_process_device(struct mfm_runflex *p, const struct mfm_runrs_run *d_runs, const int16_t *d_payload,
                               const uint64_t *d_totals, void *stream)
{
    if (!p || !d_runs || !d_payload || !d_totals) {
        return MFM_E_INVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rb = mfm_run_call_begin(p, s);
    if (rb != MFM_OK) {
        return rb;
    }
    const uint32_t cur = p->cur;
    const RfCall A{ d_runs,        d_payload,      d_totals,        p->d_chan[cur], p->d_chan[cur ^ 1u], p->d_run_state, p->d_ring,
                    p->d_seg,      p->d_plane,     p->d_summ,       p->d_seg_base,  p->d_slot_base,      p->d_fslot_base, p->d_blk_base,
                    p->d_count,    p->d_ev_base,   p->d_chan_last,  p->d_ctl,       p->d_totals,         p->d_slots,     p->d_events,
                    p->d_fslots,   p->d_fdesc,     p->d_frames,     p->d_bch,       p->cfg.nr_channels,  p->cfg.max_runs,
                    p->cfg.max_out_samples, (uint32_t)p->cap_events, (uint32_t)p->cap_frames };
    hipLaunchKernelGGL(rf_plan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_slice_kernel, dim3((uint32_t)p->max_blocks), dim3(RF_SLICE_NT), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_match_kernel, dim3((uint32_t)p->max_blocks), dim3(RF_SLICE_NT), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_walk_kernel, dim3(p->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_evscan_kernel, dim3(1), dim3(MFM_RUN_SCAN_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_compact_kernel, dim3(p->cfg.max_runs), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    /* the frames' words read the ring as the call found it: before the ring kernel */
    hipLaunchKernelGGL(rf_gather_kernel, dim3((uint32_t)p->cap_frames), dim3(RF_GATHER_THREADS), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    hipLaunchKernelGGL(rf_ring_kernel, dim3(RF_RING_BLOCKS, p->cfg.nr_channels), dim3(256), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    if (p->ends.on) { /* behind the walk, in front of the state kernel */
        const MfmRunEndsCall E{ d_runs, p->d_chan[cur], p->d_run_state, p->d_ctl, p->d_bch, p->cfg.nr_channels, p->cfg.max_runs };
        const int re = mfm_internal_run_ends_process(&p->ends, MFM_RUN_ENDS_FLEX, &E, s);
        if (re != MFM_OK) {
            return re;
        }
    }
    hipLaunchKernelGGL(rf_state_kernel, dim3(p->cfg.nr_channels), dim3(64), 0, s, A);
    MFM_RUN_TRY(hipGetLastError());
    mfm_run_call_end(p, s);
    return MFM_OK;
}

int mfm_runflex_fetch(struct mfm_runflex *p, struct mfm_runflex_event *events, size_t max_events, size_t *nr_events,
                      struct mfm_flex_frame_words *frames, size_t max_frames, size_t *nr_frames)
{
    if (!p || !nr_events || !nr_frames || (!events && max_events) || (!frames && max_frames)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    *nr_frames = 0;
    if (!p->have_call) {
        return MFM_OK;
    }
    MFM_RUN_TRY(hipSetDevice(p->cfg.device));
    MFM_RUN_TRY(hipStreamSynchronize(p->last_stream));
    uint64_t t[4];
    MFM_RUN_TRY(hipMemcpy(t, p->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    if (t[MFM_RUN_T_OVERFLOW] || t[MFM_RUN_T_INPUT]) {
        return mfm_run_fail(MFM_E_STATE, rf_refusal(t[MFM_RUN_T_OVERFLOW], t[MFM_RUN_T_INPUT]));
    }
    *nr_events = (size_t)t[RF_T_EVENTS];
    *nr_frames = (size_t)t[RF_T_FRAMES];
    if (t[RF_T_EVENTS] > max_events || t[RF_T_FRAMES] > max_frames) {
        return MFM_E_NOMEM;
    }
    if (t[RF_T_EVENTS]) {
        MFM_RUN_TRY(hipMemcpy(events, p->d_events, (size_t)t[RF_T_EVENTS] * sizeof(mfm_runflex_event), hipMemcpyDeviceToHost));
    }
    if (t[RF_T_FRAMES]) {
        MFM_RUN_TRY(hipMemcpy(frames, p->d_frames, (size_t)t[RF_T_FRAMES] * sizeof(mfm_flex_frame_words), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runflex_device_view(struct mfm_runflex *p, const struct mfm_runflex_event **d_events,
                            const struct mfm_flex_frame_words **d_frames, const uint64_t **d_totals)
{
    if (!p) {
        return MFM_E_INVAL;
    }
    if (d_events) {
        *d_events = p->d_events;
    }
    if (d_frames) {
        *d_frames = p->d_frames;
    }
    if (d_totals) {
        *d_totals = p->d_totals;
    }
    return MFM_OK;
}

int mfm_hosttwin_runflex_state_check(uint32_t nr_channels, const struct mfm_runflex_state *state)
{
    return mfm_run_state_check(nr_channels, state, "FLEX", mfm_runflex_state_check);
}

/* the states as the other stages', and the ring behind them */
int mfm_runflex_fetch_state(struct mfm_runflex *p, struct mfm_runflex_state *state, int16_t *ring, size_t nr_channels)
{
    const int rc = mfm_run_fetch_state(p, state, nr_channels);
    if (rc != MFM_OK) {
        return rc;
    }
    if (ring) {
        MFM_RUN_TRY(hipMemcpy(ring, p->d_ring, nr_channels * MFM_RUNFLEX_RING * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_runflex_store_state(struct mfm_runflex *p, const struct mfm_runflex_state *state, const int16_t *ring, size_t nr_channels)
{
    if (!ring) {
        return MFM_E_INVAL;
    }
    const int rc = mfm_run_store_state(p, state, nr_channels, mfm_hosttwin_runflex_state_check);
    if (rc != MFM_OK) {
        return rc;
    }
    MFM_RUN_TRY(hipMemcpy(p->d_ring, ring, nr_channels * MFM_RUNFLEX_RING * sizeof(int16_t), hipMemcpyHostToDevice));
    return MFM_OK;
}

/* ---- the stretch-end report: kernels and launchers in mfm_run_ends.hip ---- */

int mfm_runflex_set_end_report(struct mfm_runflex *p, int on)
{
    return mfm_run_ends_entry_set(p, MFM_RUN_ENDS_FLEX, on, mfm_run_fail);
}

int mfm_runflex_end_stretches_device(struct mfm_runflex *p, void *stream)
{
    return mfm_run_ends_entry_flush(p, MFM_RUN_ENDS_FLEX, p ? p->d_bch : nullptr, stream, mfm_run_fail);
}

int mfm_runflex_fetch_ends(struct mfm_runflex *p, struct mfm_runflex_end *ends, size_t max_ends, size_t *nr_ends)
{
    return mfm_run_ends_entry_fetch(p, MFM_RUN_ENDS_FLEX, ends, max_ends, nr_ends, mfm_run_fail, rf_refusal);
}

int mfm_runflex_ends_view(struct mfm_runflex *p, const struct mfm_runflex_end **d_ends, const uint64_t **d_end_totals)
{
    return mfm_run_ends_entry_view(p, d_ends, d_end_totals, mfm_run_fail);
}

} /* extern "C" */

/* ---- the host twin: the same plan, ring and state, the decoder one sample at a time through the search ------------------ */

namespace {

struct RfHostIn {
    const mfm_runrs_run *run;
    const int16_t *payload, *ring; /* the channel's ring */
    int at(uint64_t s) const
    {
        return s >= run->first_out ? payload[run->out_offset + (s - run->first_out)] : ring[s & (MFM_RUNFLEX_RING - 1u)];
    }
};

/* "the register sample n goes to reads BS1": bits n, n - 10, ..., n - 310, the newest a zero (n >= 310) */
bool rf_host_match(const RfHostIn &I, uint64_t n)
{
    for (uint32_t k = 0; k < 32; k++) {
        if ((I.at(n - 10u * k) >= 0) != ((k & 1u) != 0)) {
            return false;
        }
    }
    return true;
}

void rf_host_words(const RfHostIn &I, uint64_t first, uint32_t coding, int range, int delta, mfm_flex_frame_words *fw)
{
    const MfmRunflexCoding cd = mfm_runflex_coding(coding);
    const uint32_t step = cd.skip + 1u;
    std::vector<uint8_t> sym(cd.symbols);
    for (uint32_t k = 0; k < cd.symbols; k++) {
        const int v = I.at(first + (uint64_t)k * step);
        sym[k] = (uint8_t)(cd.levels == 4u ? mfm_runflex_slice4(v, delta, range) : (uint32_t)(v >= 0));
    }
    memset(fw, 0, sizeof(*fw));
    for (uint32_t q = 0; q < 4; q++) {
        uint32_t mul, add, sel;
        if (!mfm_runflex_phase_map(cd, q, &mul, &add, &sel)) {
            continue;
        }
        for (uint32_t w = 0; w < MFM_FLEX_PHASE_WORDS; w++) {
            const uint32_t n0 = (w >> 3) * 256 + (w & 7);
            for (uint32_t jb = 0; jb < 32; jb++) {
                fw->words[q][w] |= (((uint32_t)sym[(n0 + 8 * jb) * mul + add] >> sel) & 1u) << jb;
            }
        }
    }
}

/* one run through the decoder from state S (updated in place); events and frames appended, frame_index call-wide */
void rf_host_walk(mfm_runflex_state &S, const RfHostIn &I, uint32_t r, std::vector<mfm_runflex_event> &out,
                  std::vector<mfm_flex_frame_words> &frames)
{
    const MfmBchTables *T = mfm_internal_bch_host_tables();
    const mfm_runrs_run &run = *I.run;
    const uint64_t end = run.first_out + run.nr_out;
    auto emit = [&](uint32_t type, uint64_t sample, uint32_t fiw_rc, uint32_t frame_index) {
        const bool known = S.coding < 4u;
        mfm_runflex_event e;
        memset(&e, 0, sizeof(e));
        e.type = type;
        e.channel = run.channel;
        e.sample = sample;
        e.sync_sample = type == MFM_FLEX_EV_FRAME ? S.j : 0;
        e.coding = S.coding;
        e.baud = known ? mfm_runflex_coding(S.coding).baud : 0;
        e.eye = S.eye;
        e.a = S.a;
        e.b = S.b;
        e.inv_a = S.inv_a;
        e.fiw_raw = S.fiw_raw;
        e.fiw = S.fiw;
        e.fiw_rc = fiw_rc;
        e.sample_range = S.sample_range;
        e.sample_delta = S.sample_delta;
        e.cycle = S.cycle;
        e.frame = S.frame;
        e.frame_index = frame_index;
        e.nr_phases = known ? mfm_runflex_coding(S.coding).nr_phases : 0;
        e.run = r;
        e.stretch_window = S.stretch_window;
        out.push_back(e);
    };
    for (;;) {
        if (S.mode == MFM_RUNFLEX_SEARCH) {
            bool opened = false;
            while (S.p < end) {
                if (rf_host_match(I, S.p)) {
                    S.run++;
                    S.p++;
                    continue;
                }
                const uint32_t cnt = S.run & 255u; /* the reference's counter is a uint8_t */
                S.run = 0;
                if (cnt >= 3) {
                    S.mode = MFM_RUNFLEX_SYNC1;
                    S.j = S.p;
                    S.eye = cnt;
                    opened = true;
                    break;
                }
                S.p++;
            }
            if (!opened) {
                break;
            }
        }
        if (S.mode == MFM_RUNFLEX_SYNC1) {
            const uint64_t s0 = S.j + (10u - ((S.eye / 2u) % 10u));
            if (s0 + 790 >= end) {
                break;
            }
            const bool have_fiw = s0 + 1110 < end;
            uint32_t a = 0, b = 0, inv_a = 0, fiw_raw = 0;
            for (uint32_t k = 0; k < (have_fiw ? 112u : 80u); k++) {
                const uint32_t bit = I.at(s0 + 10u * k) >= 0;
                if (k < 32) {
                    a = (a << 1) | bit;
                } else if (k < 48) {
                    b = (b << 1) | bit;
                } else if (k < 80) {
                    inv_a = (inv_a << 1) | bit;
                } else {
                    fiw_raw |= bit << (k - 80u);
                }
            }
            S.a = a;
            S.b = b;
            S.inv_a = inv_a;
            S.fiw_raw = S.fiw = 0;
            S.sample_range = S.sample_delta = 0;
            S.cycle = S.frame = 0;
            S.coding = mfm_runflex_find_coding(a);
            if (S.coding == 0xffffffffu) {
                emit(MFM_FLEX_EV_BAD_BAUD, s0 + 790, 0, 0);
                S.mode = MFM_RUNFLEX_SEARCH;
                S.run = 0;
                S.p = s0 + 790 + MFM_RUNFLEX_DEAD;
                continue;
            }
            if (!have_fiw) {
                break;
            }
            S.fiw_raw = fiw_raw;
            int sum_hi = 0, sum_lo = 0, n_hi = 0, n_lo = 0;
            for (uint32_t k = 0; k < 112; k++) {
                const int v = I.at(s0 + 10u * k);
                if (v > 0) {
                    sum_hi += v;
                    n_hi++;
                } else {
                    sum_lo += v;
                    n_lo++;
                }
            }
            const uint64_t f = s0 + 1110;
            uint32_t rc;
            if (n_hi == 0 || n_lo == 0) {
                rc = 3;
            } else {
                const int high = (int16_t)(sum_hi / n_hi), low = (int16_t)(sum_lo / n_lo);
                S.sample_range = (int16_t)(high - low);
                S.sample_delta = (int16_t)(high - S.sample_range / 2);
                uint32_t bad;
                S.fiw = mfm_bch_fix(T, S.fiw_raw & 0x7fffffffu, &bad);
                if (bad) {
                    rc = 1;
                } else if (mfm_runflex_checksum(S.fiw) != 0xfu) {
                    rc = 2;
                } else {
                    rc = 0;
                    S.cycle = (S.fiw >> 4) & 0xfu;
                    S.frame = (S.fiw >> 8) & 0x7fu;
                }
            }
            if (rc != 0) {
                emit(MFM_FLEX_EV_BAD_FIW, f, rc, 0);
                S.mode = MFM_RUNFLEX_SEARCH;
                S.run = 0;
                S.p = f + MFM_RUNFLEX_DEAD;
                continue;
            }
            S.mode = MFM_RUNFLEX_FRAME;
            S.j = f;
        }
        if (S.mode == MFM_RUNFLEX_FRAME) {
            const MfmRunflexCoding cd = mfm_runflex_coding(S.coding);
            const uint32_t step = cd.skip + 1u;
            const uint64_t first = S.j + step + cd.fudge + (uint64_t)cd.sync2 * step;
            const uint64_t e = first + (uint64_t)(cd.symbols - 1u) * step;
            if (e >= end) {
                break;
            }
            emit(MFM_FLEX_EV_FRAME, e, 0, (uint32_t)frames.size());
            frames.emplace_back();
            rf_host_words(I, first, S.coding, S.sample_range, S.sample_delta, &frames.back());
            S.mode = MFM_RUNFLEX_SEARCH;
            S.run = 0;
            S.p = e + MFM_RUNFLEX_DEAD;
        }
    }
    S.outs = end;
    S.has_stretch = 1;
    mfm_runflex_canon(S);
}

} /* namespace */

namespace {

/* the host twin of one call; nr_ends != NULL: with the stretch-end records */
int rf_twin_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events, uint32_t max_frames,
                 struct mfm_runflex_state *state, int16_t *ring, const struct mfm_runrs_run *runs, const int16_t *payload,
                 const uint64_t *totals, struct mfm_runflex_event *events, size_t max_out, size_t *nr_events,
                 struct mfm_flex_frame_words *frames, size_t max_out_frames, size_t *nr_frames, uint32_t *flags,
                 struct mfm_runflex_end *ends, size_t max_ends, size_t *nr_ends)
{
    if (!state || !ring || !totals || !nr_events || !nr_frames || (!events && max_out) || (!frames && max_out_frames) ||
        (nr_ends && !ends && max_ends)) {
        return MFM_E_INVAL;
    }
    *nr_events = 0;
    *nr_frames = 0;
    if (nr_ends) {
        *nr_ends = 0;
    }
    if (flags) {
        *flags = 0;
    }
    mfm_runflex_config cfg{};
    cfg.abi_version = MFM_ABI_VERSION;
    cfg.nr_channels = nr_channels;
    cfg.max_runs = max_runs;
    cfg.max_out_samples = max_out_samples;
    cfg.max_events = max_events;
    cfg.max_frames = max_frames;
    uint64_t cap_events = 0, cap_frames = 0;
    const int rc = rf_geometry(cfg, &cap_events, &cap_frames);
    if (rc != MFM_OK) {
        return rc;
    }
    uint64_t n, over, err, ts = 0, tf = 0; /* the plan pass */
    if (!mfm_run_twin_plan(totals, nr_channels, max_runs, max_out_samples, state, runs, payload, false,
                           [&](uint32_t nr_out) { ts += mfm_runflex_event_slots(nr_out); tf += mfm_runflex_frame_slots(nr_out); }, &n, &over, &err)) {
        return MFM_E_INVAL;
    }
    if (!err && (ts > cap_events || tf > cap_frames)) {
        over = MFM_RUNFLEX_OVER_EVENTS;
    }
    if (over || err) {
        return mfm_run_twin_refuse(over, err, flags, rf_refusal(over, err));
    }
    /* every run from the state and the ring the call started with (only a channel's first run reads them) */
    std::vector<mfm_runflex_event> out;
    std::vector<mfm_flex_frame_words> fw;
    std::vector<mfm_runflex_state> left(n);
    for (uint64_t r = 0; r < n; r++) {
        const mfm_runrs_run &run = runs[r];
        mfm_runflex_state st;
        memset(&st, 0, sizeof(st));
        if (run.flags & MFM_RUNRS_BEGINS) {
            st.p = MFM_RUNFLEX_DEAD - 1u;
            st.stretch_window = run.first_window;
        } else {
            st = state[run.channel];
        }
        const RfHostIn I{ &run, payload, ring + (size_t)run.channel * MFM_RUNFLEX_RING };
        rf_host_walk(st, I, (uint32_t)r, out, fw);
        left[r] = st;
    }
    *nr_events = out.size();
    *nr_frames = fw.size();
    if (out.size() > max_out || fw.size() > max_out_frames) {
        return MFM_E_NOMEM; /* nothing written, state and ring included */
    }
    if (nr_ends) { /* from the state the call started with, before it moves */
        *nr_ends = mfm_run_ends_host_call(runs, n, state, left.data(), ends, 0, mfm_runflex_end_of);
        if (*nr_ends > max_ends) {
            return MFM_E_NOMEM;
        }
        (void)mfm_run_ends_host_call(runs, n, state, left.data(), ends, max_ends, mfm_runflex_end_of);
    }
    for (uint64_t r = 0; r < n; r++) {
        if (r + 1 == n || runs[r + 1].channel != runs[r].channel) {
            const mfm_runrs_run &run = runs[r];
            state[run.channel] = left[r];
            const uint32_t cnt = run.nr_out < MFM_RUNFLEX_RING ? run.nr_out : MFM_RUNFLEX_RING;
            int16_t *rg = ring + (size_t)run.channel * MFM_RUNFLEX_RING;
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t off = run.nr_out - cnt + k;
                rg[(run.first_out + off) & (MFM_RUNFLEX_RING - 1u)] = payload[run.out_offset + off];
            }
        }
    }
    if (!out.empty()) {
        memcpy(events, out.data(), out.size() * sizeof(mfm_runflex_event));
    }
    if (!fw.empty()) {
        memcpy(frames, fw.data(), fw.size() * sizeof(mfm_flex_frame_words));
    }
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_hosttwin_runflex_call(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                              uint32_t max_frames, struct mfm_runflex_state *state, int16_t *ring, const struct mfm_runrs_run *runs,
                              const int16_t *payload, const uint64_t *totals, struct mfm_runflex_event *events, size_t max_out,
                              size_t *nr_events, struct mfm_flex_frame_words *frames, size_t max_out_frames, size_t *nr_frames,
                              uint32_t *flags)
{
    return rf_twin_call(nr_channels, max_runs, max_out_samples, max_events, max_frames, state, ring, runs, payload, totals, events, max_out,
                        nr_events, frames, max_out_frames, nr_frames, flags, nullptr, 0, nullptr);
}

int mfm_hosttwin_runflex_call_ends(uint32_t nr_channels, uint32_t max_runs, uint32_t max_out_samples, uint32_t max_events,
                                   uint32_t max_frames, struct mfm_runflex_state *state, int16_t *ring, const struct mfm_runrs_run *runs,
                                   const int16_t *payload, const uint64_t *totals, struct mfm_runflex_event *events, size_t max_out,
                                   size_t *nr_events, struct mfm_flex_frame_words *frames, size_t max_out_frames, size_t *nr_frames,
                                   uint32_t *flags, struct mfm_runflex_end *ends, size_t max_ends, size_t *nr_ends)
{
    if (!nr_ends) {
        return MFM_E_INVAL;
    }
    return rf_twin_call(nr_channels, max_runs, max_out_samples, max_events, max_frames, state, ring, runs, payload, totals, events, max_out,
                        nr_events, frames, max_out_frames, nr_frames, flags, ends, max_ends, nr_ends);
}

int mfm_hosttwin_runflex_end_stretches(uint32_t nr_channels, struct mfm_runflex_state *state, struct mfm_runflex_end *ends,
                                       size_t max_ends, size_t *nr_ends)
{
    return mfm_run_ends_host_flush(nr_channels, state, ends, max_ends, nr_ends, mfm_runflex_end_of);
}

} /* extern "C" */
