/*
 * mfm_gate.hip - the squelch gate: of rows that are still in HBM (the engine's PCM or filtered IQ, the resampler's output)
 * only the windows the level stage left OPEN, and the P pre-roll windows in front of every opening, go into one dense
 * payload, with a run list that says which channel and which samples each piece is.  See include/multifm_hip.h for the
 * boundary, mfm_gate.h for the arithmetic.
 *
 * The reference has no such stage (nor a squelch).  What the stage computes is an exact copy, so a numpy restatement is the
 * yardstick (tests/test_gate.py, tests/test_gate_preroll.py).
 *
 * Layout of the work.  A row is a run of int16 ELEMENTS (E per sample), a window is We = W * E of them.  Window k of a
 * channel goes out when any of its records k .. k + P is open (P = preroll_windows, 0 unless mfm_gate_set_preroll said
 * otherwise), so a call that brings the records K0 .. K1 - 1 decides the windows K0 - P .. K1 - P - 1, its candidates, whose
 * samples may lie in earlier calls.  The device therefore keeps per channel
 *
 *   the history   a LINEAR buffer of at most (P + 1) * We elements: the last min(K, P) complete windows and the unfinished
 *                 one, oldest first.  It stands as a virtual prefix in front of the call's rows; mfm_gate_src gives a signed
 *                 index, the row when >= 0, otherwise counted back from the history's end.  There are two buffers used in
 *                 turn: a call reads one and gt_hist_kernel, behind the copy, writes the other from (old history ++ rows),
 *                 so a call shorter than the history is a move between buffers and nothing is read after it was written.
 *                 (A ring would save that move; it would also put a second seam into the copy's source.  The move is
 *                 (P + 1) * We elements per channel and call at most.)
 *   the bits      one 64-bit word: the open bits of the P records in front of the next call.  Two words used in turn as
 *                 well: the count pass writes the next one, the runs pass still reads the current one.
 *
 * With P = 0 the history is the unfinished window alone and the word stays 0; nothing in this file asks whether P is 0.
 *
 *   gt_count_kernel  one WAVE per channel walks the channel's candidates 64 at a time: one ballot of the record bits per
 *                    chunk (the word behind it is the next chunk's), dilated by shift-and-OR (mfm_gate_dilate); the open
 *                    windows and the run starts are popcounts of that mask.  A record whose .window is not the expected k
 *                    marks the channel.
 *   gt_scan_kernel   one block: exclusive scan of both counts over all channels (a thread sums a stretch of channels, the
 *                    waves scan by lane shifts, the 16 wave sums go through LDS), the totals, the overflow and
 *                    out-of-step flags.
 *   gt_runs_kernel   one wave per channel again: with the channel's base from the scan every candidate gets its slot in the
 *                    payload (or MFM_GATE_CLOSED) and every run start writes its descriptor (first_window is the true k);
 *                    on overflow nothing does.
 *   gt_copy_kernel   the hot path.  A group of G lanes (G = 1 .. 256, a power of two chosen from We) copies one piece of
 *                    at most 8192 elements of one open window; the group of a closed window returns after reading its
 *                    slot.  The piece is cut where the DESTINATION reaches 16-byte alignment: up to 7 elements one by
 *                    one, then 16-byte stores, each fed by one 16-byte load from wherever the source lies (aligned when
 *                    source and destination agree modulo 16 bytes, otherwise an unaligned load, which the memory path
 *                    splits), up to four of them in flight per lane, then up to 7 elements again.  The body of a piece lies
 *                    wholly in the rows, wholly in the history or across the seam; the first two take that loop from their
 *                    base pointer, the third a plainer loop whose one chunk of eight on the seam is put together singly.
 *   gt_hist_kernel   the history's update, behind the copy, which read the old one.
 *
 * A flush is a call with no rows and no records that decides the P windows left.  Nothing is floating point, nothing goes
 * through an atomic (order and offsets are a count, a scan and a rank), and the host never waits: how many windows a call
 * completes follows from the stream position alone.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_gate.h"

extern "C" __attribute__((visibility("hidden"))) void mfm_internal_set_error(const char *msg);

struct mfm_gate {
    mfm_gate_config cfg{};
    uint32_t W = 0, E = 1, We = 0;
    uint32_t max_win = 0;      /* windows per channel a process call completes at most */
    uint64_t cap_windows = 0;  /* payload capacity, windows */
    uint64_t cap_runs = 0;
    uint32_t log2g = 0, npieces = 1;
    uint64_t pos = 0;          /* samples per channel consumed so far */
    uint64_t k_first = 0;      /* the stream's first window: 0, or where mfm_gate_seek put it; no window in front of it exists */
    uint32_t *d_cnt_open = nullptr, *d_cnt_runs = nullptr, *d_bad = nullptr, *d_base_runs = nullptr, *d_base_open = nullptr, *d_slot = nullptr;
    uint64_t *d_totals = nullptr;
    mfm_gate_run *d_runs = nullptr;
    int16_t *d_payload = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_call = false, flushed = false;
    uint32_t P = 0;
    uint32_t slot_stride = 0;  /* of d_slot: candidates per channel and call at most, max(max_win, largest P set) */
    uint32_t hist_stride = 0;  /* elements per channel of either history buffer */
    int16_t *d_hist[2] = { nullptr, nullptr };  /* used in turn: a call reads [cur] and writes [cur ^ 1] */
    uint64_t *d_bits[2] = { nullptr, nullptr }; /* the open bits of the P records in front of the next call, likewise */
    uint32_t cur = 0;
};

namespace {

constexpr uint32_t GT_PIECE = 8192;  /* elements one group copies at most: 256 lanes, 4 chunks of 8 each */
constexpr uint32_t GT_SCAN_THREADS = 1024;
constexpr uint32_t GT_T_RUNS = 0, GT_T_ELEMS = 1, GT_T_OVERFLOW = 2, GT_T_OUT_OF_STEP = 3; /* d_totals[] */

/* eight elements as one 16-byte access; the load may lie at any 2-byte alignment */
struct __attribute__((packed, aligned(2))) gt_x8u {
    uint32_t d[4];
};
struct __attribute__((aligned(16))) gt_x8 {
    uint32_t d[4];
};

struct GtRecs {
    const mfm_level_record *rec;
    size_t rec_stride;
    uint64_t k0;    /* the call's first record */
    uint64_t kf;    /* the stream's first window (mfm_gate::k_first) */
    uint32_t nrec;  /* records the call brings */
    uint32_t nemit; /* candidates: nrec, at a flush P */
    uint32_t P;
    uint32_t nr_channels;
};

/* 64 bits of the channel's sequence S from bit i0 on (mfm_gate.h): prev below P, then the call's records, then closed.
 * `wrong` collects out-of-step records. */
__device__ __forceinline__ uint64_t gt_word(const GtRecs &R, const mfm_level_record *rc, uint64_t prev, uint32_t i0, uint32_t lane, uint32_t &wrong)
{
    const uint32_t i = i0 + lane;
    bool open = false;
    if (i < R.P) {
        open = (prev >> i) & 1ull;
    } else if (i - R.P < R.nrec) {
        const uint32_t j = i - R.P;
        open = rc[j].open != 0;
        wrong |= rc[j].window != R.k0 + j ? 1u : 0u;
    }
    return __ballot(open);
}

__global__ __launch_bounds__(256) void gt_count_kernel(const GtRecs R, const uint64_t *__restrict__ bits_in, uint64_t *__restrict__ bits_out,
                                                      uint32_t *__restrict__ cnt_open, uint32_t *__restrict__ cnt_runs, uint32_t *__restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (c >= R.nr_channels) {
        return;
    }
    const mfm_level_record *rc = R.rec + (size_t)c * R.rec_stride;
    const uint64_t prev = bits_in[c];
    const uint32_t skip = mfm_gate_pre_skip(R.k0 - R.kf, R.P);
    mfm_gate_walk w{};
    uint32_t wrong = 0;
    uint64_t lo = gt_word(R, rc, prev, 0, lane, wrong);
    for (uint32_t e0 = 0; e0 < R.nemit; e0 += 64) {
        const uint32_t cnt = R.nemit - e0 < 64u ? R.nemit - e0 : 64u;
        const uint64_t hi = gt_word(R, rc, prev, e0 + 64, lane, wrong);
        const uint64_t mask = mfm_gate_dilate(lo, hi, R.P, e0, cnt, skip);
        uint32_t dr, dl;
        (void)mfm_gate_walk_step(w, mask, cnt, e0 + 64 >= R.nemit, dr, dl);
        lo = hi;
    }
    /* the P records in front of the next call: S[nrec .. nrec + P - 1] */
    uint32_t unused = 0;
    const uint64_t next = gt_word(R, rc, prev, R.nrec, lane, unused) & mfm_gate_below(R.P);
    const bool any_wrong = __ballot(wrong != 0) != 0;
    if (lane == 0) {
        cnt_open[c] = w.opens;
        cnt_runs[c] = w.runs;
        bad[c] = any_wrong ? 1u : 0u;
        bits_out[c] = next;
    }
}

/* scan over the block (1024 threads); returns this thread's EXCLUSIVE prefix, *total = the block's sum.  Every sum is a
 * count of windows of one call, below 2^32 (mfm_gate_create) */
__device__ __forceinline__ uint32_t gt_block_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= (uint32_t)o) {
            inc += up;
        }
    }
    if (lane == 63) {
        lds[wave] = inc;
    }
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < GT_SCAN_THREADS / 64; i++) {
        const uint32_t t = lds[i];
        base += i < wave ? t : 0u;
        all += t;
    }
    __syncthreads();
    *total = all;
    return base + inc - v;
}

__global__ __launch_bounds__(GT_SCAN_THREADS) void gt_scan_kernel(uint32_t nr_channels, uint32_t per, const uint32_t *__restrict__ cnt_open,
                                                                  const uint32_t *__restrict__ cnt_runs, const uint32_t *__restrict__ bad,
                                                                  uint32_t *__restrict__ base_open, uint32_t *__restrict__ base_runs,
                                                                  uint64_t *__restrict__ totals, uint32_t We, uint64_t cap_windows)
{
    __shared__ uint32_t lds[GT_SCAN_THREADS / 64];
    const uint32_t c0 = threadIdx.x * per;
    const uint32_t c1 = c0 + per < nr_channels ? c0 + per : nr_channels;
    uint32_t so = 0, sr = 0, sb = 0;
#pragma unroll 1
    for (uint32_t c = c0; c < c1; c++) {
        so += cnt_open[c];
        sr += cnt_runs[c];
        sb += bad[c];
    }
    uint32_t to, tr, tb;
    uint32_t bo = gt_block_scan(so, lds, &to);
    uint32_t br = gt_block_scan(sr, lds, &tr);
    (void)gt_block_scan(sb, lds, &tb);
#pragma unroll 1
    for (uint32_t c = c0; c < c1; c++) {
        base_open[c] = bo;
        base_runs[c] = br;
        bo += cnt_open[c];
        br += cnt_runs[c];
    }
    if (threadIdx.x == 0) {
        totals[GT_T_RUNS] = tr;
        totals[GT_T_ELEMS] = (uint64_t)to * We;
        totals[GT_T_OVERFLOW] = to > cap_windows ? 1ull : 0ull;
        totals[GT_T_OUT_OF_STEP] = tb ? 1ull : 0ull;
    }
}

__global__ __launch_bounds__(256) void gt_runs_kernel(const GtRecs R, const uint64_t *__restrict__ bits_in, const uint32_t *__restrict__ base_open,
                                                     const uint32_t *__restrict__ base_runs, const uint64_t *__restrict__ totals,
                                                     mfm_gate_run *__restrict__ runs, uint32_t *__restrict__ slot, uint32_t slot_stride, uint32_t We)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (c >= R.nr_channels) {
        return;
    }
    const mfm_level_record *rc = R.rec + (size_t)c * R.rec_stride;
    uint32_t *sc = slot + (size_t)c * slot_stride;
    if (totals[GT_T_OVERFLOW]) { /* the payload cannot take the call: nothing goes out */
        for (uint32_t m = lane; m < R.nemit; m += 64) {
            sc[m] = MFM_GATE_CLOSED;
        }
        return;
    }
    const uint64_t prev = bits_in[c];
    const uint32_t skip = mfm_gate_pre_skip(R.k0 - R.kf, R.P);
    const uint32_t bo = base_open[c];
    mfm_gate_run *rr = runs + base_runs[c];
    mfm_gate_walk w{};
    uint32_t wrong = 0;
    uint64_t lo = gt_word(R, rc, prev, 0, lane, wrong);
    for (uint32_t e0 = 0; e0 < R.nemit; e0 += 64) {
        const uint32_t cnt = R.nemit - e0 < 64u ? R.nemit - e0 : 64u;
        const bool last = e0 + 64 >= R.nemit;
        const uint64_t hi = gt_word(R, rc, prev, e0 + 64, lane, wrong);
        const uint64_t mask = mfm_gate_dilate(lo, hi, R.P, e0, cnt, skip);
        const uint64_t starts = mfm_gate_starts(w, mask);
        if (lane < cnt) {
            const bool open = (mask >> lane) & 1ull;
            const uint32_t at = bo + mfm_gate_slot(w, mask, lane); /* < cap_windows <= 2^32 - 2 */
            sc[e0 + lane] = open ? at : MFM_GATE_CLOSED;
            if ((starts >> lane) & 1ull) {
                uint32_t rank, len;
                bool whole;
                mfm_gate_run_at(w, mask, starts, lane, cnt, last, rank, len, whole);
                rr[rank].first_window = R.k0 + e0 + lane - R.P; /* an open candidate lies at or above skip: k >= kf */
                rr[rank].payload_offset = (uint64_t)at * We;
                rr[rank].channel = c;
                if (whole) {
                    rr[rank].nr_windows = len;
                }
            }
        }
        uint32_t done_run = 0, done_len = 0;
        if (mfm_gate_walk_step(w, mask, cnt, last, done_run, done_len) && lane == 0) {
            rr[done_run].nr_windows = done_len;
        }
        lo = hi;
    }
}

struct GtCopy {
    size_t stride;        /* of rows, elements */
    uint32_t hist_stride; /* elements */
    uint32_t slot_stride;
    uint32_t We, nemit;
    uint32_t back;        /* P * We + r0: elements of the virtual stream between candidate 0's first and the row's first */
    uint32_t hlen;        /* elements the history holds */
    uint32_t log2g;       /* lanes per piece = 1 << log2g */
    uint32_t npieces;     /* pieces per window */
};

__global__ __launch_bounds__(256) void gt_copy_kernel(const GtCopy K, const int16_t *__restrict__ rows, const int16_t *__restrict__ hist,
                                                     const uint32_t *__restrict__ slot, int16_t *__restrict__ payload)
{
    const uint32_t G = 1u << K.log2g;
    const uint32_t lane = threadIdx.x & (G - 1u);
    const uint32_t u = blockIdx.x * (256u >> K.log2g) + (threadIdx.x >> K.log2g); /* piece of the channel */
    const uint32_t c = blockIdx.y;
    const uint32_t m = K.npieces == 1 ? u : u / K.npieces; /* the candidate */
    if (m >= K.nemit) {
        return;
    }
    const uint32_t at = slot[(size_t)c * K.slot_stride + m];
    if (at == MFM_GATE_CLOSED) { /* a closed window is neither read nor written */
        return;
    }
    const uint32_t p0 = (u - m * K.npieces) * GT_PIECE; /* the piece: elements [p0, p0 + len) of the window */
    const uint32_t len = K.We - p0 < GT_PIECE ? K.We - p0 : GT_PIECE;
    const int16_t *xr = rows + (size_t)c * K.stride;
    /* xlow[g] for g < 0: the history, counted back from its end (an open candidate is a window that exists, g >= -hlen) */
    const int16_t *xlow = hist + (size_t)c * K.hist_stride + K.hlen;
    const uint64_t d0 = (uint64_t)at * K.We + p0;
    int16_t *dst = payload + d0;
    const int64_t g0 = mfm_gate_src(m, p0, K.We, K.back);
    auto one = [&](uint32_t j) {
        const int64_t g = g0 + j;
        dst[j] = g >= 0 ? xr[g] : xlow[g];
    };
    const uint32_t mis = (uint32_t)d0 & 7u; /* the payload itself is 16-byte aligned */
    uint32_t head = (8u - mis) & 7u;
    head = head < len ? head : len;
    const uint32_t nbody = (len - head) >> 3;
    const int64_t gb = g0 + head;
    if (gb >= 0 || gb + (int64_t)(8u * nbody) <= 0) { /* all of the body in the row, or all of it in the history */
        const int16_t *src = (gb >= 0 ? xr : xlow) + gb;
        int16_t *out = dst + head;
        auto ld = [&](uint32_t t) { return *reinterpret_cast<const gt_x8u *>(src + 8u * t); };
        auto st = [&](uint32_t t, const gt_x8u &v) {
            gt_x8 o;
            o.d[0] = v.d[0];
            o.d[1] = v.d[1];
            o.d[2] = v.d[2];
            o.d[3] = v.d[3];
            *reinterpret_cast<gt_x8 *>(out + 8u * t) = o;
        };
        uint32_t t = lane;
        for (; t + 3u * G < nbody; t += 4u * G) {
            const gt_x8u v0 = ld(t), v1 = ld(t + G), v2 = ld(t + 2u * G), v3 = ld(t + 3u * G);
            st(t, v0);
            st(t + G, v1);
            st(t + 2u * G, v2);
            st(t + 3u * G, v3);
        }
        for (; t + G < nbody; t += 2u * G) {
            const gt_x8u v0 = ld(t), v1 = ld(t + G);
            st(t, v0);
            st(t + G, v1);
        }
        if (t < nbody) {
            st(t, ld(t));
        }
    } else {
        /* the body begins in the history and ends in the row.  The one chunk whose eight elements lie on both sides, if
         * any, is put together singly */
        const uint32_t ts = (-gb & 7) ? (uint32_t)(-gb >> 3) : ~0u;
        for (uint32_t t = lane; t < nbody; t += G) {
            const int64_t g = gb + 8u * t;
            if (t != ts) {
                const gt_x8u v = *reinterpret_cast<const gt_x8u *>(g >= 0 ? xr + g : xlow + g);
                gt_x8 o;
                o.d[0] = v.d[0];
                o.d[1] = v.d[1];
                o.d[2] = v.d[2];
                o.d[3] = v.d[3];
                *reinterpret_cast<gt_x8 *>(dst + head + 8u * t) = o;
            } else {
                for (uint32_t e = 0; e < 8; e++) {
                    one(head + 8u * t + e);
                }
            }
        }
    }
    for (uint32_t j = lane; j < head; j += G) {
        one(j);
    }
    for (uint32_t j = head + 8u * nbody + lane; j < len; j += G) {
        one(j);
    }
}

/* the history after the call: its hlen1 elements are the last hlen1 of (old history of hlen0 ++ the row's N) */
__global__ __launch_bounds__(256) void gt_hist_kernel(const int16_t *__restrict__ rows, size_t stride, const int16_t *__restrict__ hist_in,
                                                     int16_t *__restrict__ hist_out, uint32_t hist_stride, uint32_t hlen0, uint32_t hlen1,
                                                     uint32_t N)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (i < hlen1) {
        const int64_t g = mfm_gate_hist_src(i, hlen1, N);
        hist_out[(size_t)c * hist_stride + i] = g >= 0 ? rows[(size_t)c * stride + g] : hist_in[(size_t)c * hist_stride + hlen0 + g];
    }
}

thread_local char g_gt_error[256] = "";

int gt_fail(int code, const char *msg)
{
    snprintf(g_gt_error, sizeof(g_gt_error), "%s", msg);
    mfm_internal_set_error(g_gt_error);
    return code;
}

#define GT_TRY(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_gt_error, sizeof(g_gt_error), "%s failed: %s", #expr, hipGetErrorString(err_));       \
            mfm_internal_set_error(g_gt_error);                                                              \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

/* what depends on P: d_slot, d_runs and d_payload grow where a flush of P windows per channel needs more than they hold
 * (they never shrink), history and bits are made anew, zeroed.  The object changes only where a step succeeded, and P
 * with the last one; the caller has checked P and set the device. */
int gt_size_for(mfm_gate *g, uint32_t P)
{
    const uint32_t C = g->cfg.nr_channels;
    const uint32_t per_ch = g->max_win > P ? g->max_win : P; /* candidates per channel and call at most: a flush has P */
    const uint64_t all = (uint64_t)C * per_ch;
    if (per_ch > g->slot_stride) {
        uint32_t *slot = nullptr;
        GT_TRY(hipMalloc(&slot, (size_t)all * 4));
        (void)hipFree(g->d_slot);
        g->d_slot = slot;
        g->slot_stride = per_ch;
    }
    /* the default capacity holds any call, and a flush is one; a caller-chosen capacity stays, but the run list must hold
     * what fits it: a flush has up to (P + 1) / 2 runs per channel */
    const uint64_t cap_windows = 0 == g->cfg.max_open_windows && all > g->cap_windows ? all : g->cap_windows;
    const uint64_t most_runs = (uint64_t)C * ((per_ch + 1) / 2); /* two runs of a channel have a closed window between them */
    const uint64_t cap_runs = cap_windows < most_runs ? cap_windows : most_runs;
    if (cap_runs > g->cap_runs) {
        mfm_gate_run *runs = nullptr;
        GT_TRY(hipMalloc(&runs, (size_t)cap_runs * sizeof(mfm_gate_run)));
        (void)hipFree(g->d_runs);
        g->d_runs = runs;
        g->cap_runs = cap_runs;
    }
    if (cap_windows > g->cap_windows) {
        int16_t *payload = nullptr;
        GT_TRY(hipMalloc(&payload, (size_t)cap_windows * g->We * 2));
        (void)hipFree(g->d_payload);
        g->d_payload = payload;
        g->cap_windows = cap_windows;
    }
    const uint32_t hist_stride = ((P + 1u) * g->We + 7u) & ~7u; /* <= 64 * 2^20 + 7 */
    const size_t bytes[4] = { (size_t)C * hist_stride * 2, (size_t)C * hist_stride * 2, (size_t)C * 8, (size_t)C * 8 };
    void *fresh[4] = { nullptr, nullptr, nullptr, nullptr };
    hipError_t history_alloc = hipSuccess;
    for (int i = 0; i < 4 && history_alloc == hipSuccess; i++) {
        history_alloc = hipMalloc(&fresh[i], bytes[i]);
        history_alloc = history_alloc == hipSuccess ? hipMemset(fresh[i], 0, bytes[i]) : history_alloc;
    }
    history_alloc = history_alloc == hipSuccess ? hipDeviceSynchronize() : history_alloc;
    if (history_alloc != hipSuccess) {
        for (void *p : fresh) {
            (void)hipFree(p);
        }
        GT_TRY(history_alloc);
    }
    for (int i = 0; i < 2; i++) {
        (void)hipFree(g->d_hist[i]);
        (void)hipFree(g->d_bits[i]);
        g->d_hist[i] = static_cast<int16_t *>(fresh[i]);
        g->d_bits[i] = static_cast<uint64_t *>(fresh[2 + i]);
    }
    g->hist_stride = hist_stride;
    g->cur = 0;
    g->P = P;
    return MFM_OK;
}

/* one process call (flush == 0) or the flush: count, scan, runs and copy where the call has candidates, the history.
 * Arguments checked by the caller */
int gt_call(mfm_gate *g, const int16_t *d_rows, size_t in_stride, size_t nr_in, const mfm_level_record *d_records, size_t record_stride,
            const mfm_gate_cut &cut, int flush, hipStream_t s)
{
    const uint32_t C = g->cfg.nr_channels, P = g->P, We = g->We;
    const uint32_t nemit = flush ? P : cut.nwin;
    const uint32_t hlen0 = mfm_gate_hist_len(cut.k0 - g->k_first, cut.r0, P, We);
    const GtRecs R{ d_records, record_stride, cut.k0, g->k_first, cut.nwin, nemit, P, C };
    const int16_t *hin = g->d_hist[g->cur];
    hipLaunchKernelGGL(gt_count_kernel, dim3((C + 3) / 4), dim3(256), 0, s, R, g->d_bits[g->cur], g->d_bits[g->cur ^ 1u], g->d_cnt_open,
                       g->d_cnt_runs, g->d_bad);
    GT_TRY(hipGetLastError());
    hipLaunchKernelGGL(gt_scan_kernel, dim3(1), dim3(GT_SCAN_THREADS), 0, s, C, (C + GT_SCAN_THREADS - 1) / GT_SCAN_THREADS, g->d_cnt_open,
                       g->d_cnt_runs, g->d_bad, g->d_base_open, g->d_base_runs, g->d_totals, We, g->cap_windows);
    GT_TRY(hipGetLastError());
    if (nemit) {
        hipLaunchKernelGGL(gt_runs_kernel, dim3((C + 3) / 4), dim3(256), 0, s, R, g->d_bits[g->cur], g->d_base_open, g->d_base_runs, g->d_totals,
                           g->d_runs, g->d_slot, g->slot_stride, We);
        GT_TRY(hipGetLastError());
        const GtCopy K{ in_stride, g->hist_stride, g->slot_stride, We, nemit, P * We + cut.r0, hlen0, g->log2g, g->npieces };
        const uint64_t pieces = (uint64_t)nemit * g->npieces;
        const uint32_t per_block = 256u >> g->log2g;
        hipLaunchKernelGGL(gt_copy_kernel, dim3((uint32_t)((pieces + per_block - 1) / per_block), C), dim3(256), 0, s, K, d_rows, hin, g->d_slot,
                           g->d_payload);
        GT_TRY(hipGetLastError());
    }
    if (flush) {
        g->flushed = true; /* the history is of no more use; the unfinished window is dropped */
    } else if (nr_in) {    /* nr_in == 0 leaves the history as it is, and the bits: S[0 .. P - 1] is prev */
        const uint32_t hlen1 = mfm_gate_hist_len(cut.k0 + cut.nwin - g->k_first, cut.r1, P, We);
        if (hlen1) {
            hipLaunchKernelGGL(gt_hist_kernel, dim3((hlen1 + 255) / 256, C), dim3(256), 0, s, d_rows, in_stride, hin, g->d_hist[g->cur ^ 1u],
                               g->hist_stride, hlen0, hlen1, (uint32_t)nr_in * g->E);
            GT_TRY(hipGetLastError());
        }
        g->cur ^= 1u; /* both the bits (written by the count pass) and the history */
    }
    g->pos += nr_in;
    g->last_stream = s;
    g->have_call = true;
    return MFM_OK;
}

} /* namespace */

extern "C" {

int mfm_gate_create(struct mfm_gate **pg, const struct mfm_gate_config *cfg)
{
    if (!pg || !cfg) {
        return MFM_E_INVAL;
    }
    *pg = nullptr;
    if (cfg->abi_version != MFM_ABI_VERSION || 0 == cfg->nr_channels || cfg->nr_channels > 65535u || 0 == cfg->max_in_samples ||
        cfg->max_in_samples > (1u << 28) || cfg->flags != 0) {
        return gt_fail(MFM_E_INVAL, "abi_version, nr_channels (1 .. 65535), max_in_samples (1 .. 2^28) or flags (0) out of range");
    }
    if (cfg->elems_per_sample != 1 && cfg->elems_per_sample != 2) {
        return gt_fail(MFM_E_INVAL, "elems_per_sample must be 1 (PCM rows) or 2 (filtered-IQ rows)");
    }
    if (0 == cfg->window_samples || (uint64_t)cfg->window_samples * cfg->elems_per_sample > MFM_GATE_MAX_WINDOW_ELEMS) {
        return gt_fail(MFM_E_INVAL, "window_samples * elems_per_sample must be 1 .. 2^20: the carry buffer holds one window per channel");
    }
    const uint32_t C = cfg->nr_channels;
    const uint32_t max_win = cfg->max_in_samples / cfg->window_samples + 1;
    const uint64_t all = (uint64_t)C * max_win;
    if (all > 0xfffffffeull) {
        return gt_fail(MFM_E_INVAL, "nr_channels * (max_in_samples / window_samples + 1) must stay below 2^32 - 1");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        return MFM_E_DEVICE; /* no CPU path */
    }
    GT_TRY(hipSetDevice(cfg->device));
    mfm_gate *g = new (std::nothrow) mfm_gate();
    if (!g) {
        return MFM_E_NOMEM;
    }
    g->cfg = *cfg;
    g->W = cfg->window_samples;
    g->E = cfg->elems_per_sample;
    g->We = g->W * g->E;
    g->max_win = max_win;
    g->slot_stride = max_win;
    g->cap_windows = cfg->max_open_windows && cfg->max_open_windows < all ? cfg->max_open_windows : all;
    const uint64_t most_runs = (uint64_t)C * ((max_win + 1) / 2); /* two runs of a channel have a closed window between them */
    g->cap_runs = g->cap_windows < most_runs ? g->cap_windows : most_runs;
    const uint32_t chunks = (g->We + 7u) / 8u;
    while ((1u << g->log2g) < chunks && g->log2g < 8) {
        g->log2g++;
    }
    g->npieces = (g->We + GT_PIECE - 1) / GT_PIECE;
    *pg = g;
    GT_TRY(hipMalloc(&g->d_cnt_open, (size_t)C * 4));
    GT_TRY(hipMalloc(&g->d_cnt_runs, (size_t)C * 4));
    GT_TRY(hipMalloc(&g->d_bad, (size_t)C * 4));
    GT_TRY(hipMalloc(&g->d_base_runs, (size_t)C * 4));
    GT_TRY(hipMalloc(&g->d_base_open, (size_t)C * 4));
    GT_TRY(hipMalloc(&g->d_slot, (size_t)C * max_win * 4));
    GT_TRY(hipMalloc(&g->d_totals, 4 * 8));
    GT_TRY(hipMemset(g->d_totals, 0, 4 * 8));
    GT_TRY(hipMalloc(&g->d_runs, (size_t)g->cap_runs * sizeof(mfm_gate_run)));
    GT_TRY(hipMalloc(&g->d_payload, (size_t)g->cap_windows * g->We * 2));
    return gt_size_for(g, 0); /* the history of P = 0 is the carry: one window per channel (twice) */
}

void mfm_gate_destroy(struct mfm_gate **pg)
{
    if (!pg || !*pg) {
        return;
    }
    mfm_gate *g = *pg;
    (void)hipSetDevice(g->cfg.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(g->d_cnt_open);
    (void)hipFree(g->d_cnt_runs);
    (void)hipFree(g->d_bad);
    (void)hipFree(g->d_base_runs);
    (void)hipFree(g->d_base_open);
    (void)hipFree(g->d_slot);
    (void)hipFree(g->d_totals);
    (void)hipFree(g->d_runs);
    (void)hipFree(g->d_payload);
    for (int i = 0; i < 2; i++) {
        (void)hipFree(g->d_hist[i]);
        (void)hipFree(g->d_bits[i]);
    }
    delete g;
    *pg = nullptr;
}

int mfm_gate_set_preroll(struct mfm_gate *g, uint32_t preroll_windows)
{
    if (!g) {
        return MFM_E_INVAL;
    }
    if (g->have_call || g->flushed) {
        return gt_fail(MFM_E_STATE, "mfm_gate_set_preroll comes before the first process call");
    }
    const uint32_t P = preroll_windows, C = g->cfg.nr_channels;
    char msg[200];
    if (P > MFM_GATE_MAX_PREROLL) {
        snprintf(msg, sizeof(msg), "preroll_windows above MFM_GATE_MAX_PREROLL = %u", MFM_GATE_MAX_PREROLL);
        return gt_fail(MFM_E_INVAL, msg);
    }
    const uint64_t hist_bytes = (uint64_t)C * (((P + 1u) * g->We + 7u) & ~7u) * 2u;
    if (P && hist_bytes > MFM_GATE_MAX_HISTORY_BYTES) { /* P = 0 is what create made: one window, bounded there */
        snprintf(msg, sizeof(msg), "the history, (P + 1) windows of int16 per channel = %llu bytes, exceeds MFM_GATE_MAX_HISTORY_BYTES = %llu",
                 (unsigned long long)hist_bytes, (unsigned long long)MFM_GATE_MAX_HISTORY_BYTES);
        return gt_fail(MFM_E_INVAL, msg);
    }
    if ((uint64_t)C * P > 0xfffffffeull) {
        return gt_fail(MFM_E_INVAL, "nr_channels * preroll_windows must stay below 2^32 - 1");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || g->cfg.device >= ndev) {
        return MFM_E_DEVICE;
    }
    GT_TRY(hipSetDevice(g->cfg.device));
    return gt_size_for(g, P);
}

int mfm_gate_seek(struct mfm_gate *g, uint64_t samples_before)
{
    if (!g) {
        return gt_fail(MFM_E_INVAL, "mfm_gate_seek: no object");
    }
    if (samples_before >= (1ull << 62)) {
        return gt_fail(MFM_E_INVAL, "mfm_gate_seek: samples_before must stay below 2^62");
    }
    if (samples_before % g->W) {
        return gt_fail(MFM_E_INVAL, "mfm_gate_seek: samples_before must be a multiple of window_samples (no fresh stage stands inside a window)");
    }
    GT_TRY(hipSetDevice(g->cfg.device));
    if (g->have_call) {
        GT_TRY(hipStreamSynchronize(g->last_stream));
    }
    /* what create and mfm_gate_set_preroll(P) leave: history and open bits empty, no result to fetch; the windows in front
     * of samples_before do not exist, as those in front of 0 do not in a fresh stream */
    const uint32_t C = g->cfg.nr_channels;
    for (int i = 0; i < 2; i++) {
        GT_TRY(hipMemset(g->d_hist[i], 0, (size_t)C * g->hist_stride * 2));
        GT_TRY(hipMemset(g->d_bits[i], 0, (size_t)C * 8));
    }
    GT_TRY(hipMemset(g->d_totals, 0, 4 * 8));
    GT_TRY(hipDeviceSynchronize());
    g->cur = 0;
    g->pos = samples_before;
    g->k_first = samples_before / g->W;
    g->last_stream = nullptr;
    g->have_call = false;
    g->flushed = false;
    return MFM_OK;
}

int mfm_gate_process_device(struct mfm_gate *g, const int16_t *d_rows, size_t in_stride, size_t nr_in, const struct mfm_level_record *d_records,
                            size_t record_stride, size_t nr_windows, void *stream)
{
    if (!g || (!d_rows && nr_in) || nr_in > g->cfg.max_in_samples || (nr_in && in_stride < nr_in * g->E && g->cfg.nr_channels > 1)) {
        return MFM_E_INVAL;
    }
    const mfm_gate_cut cut = mfm_gate_cut_of(g->pos, nr_in, g->W, g->E);
    if (nr_windows != cut.nwin) {
        return gt_fail(MFM_E_INVAL, "nr_windows is not what this call completes: feed the gate the level stage's nr_in sequence");
    }
    if (cut.nwin && (!d_records || record_stride < cut.nwin)) {
        return MFM_E_INVAL;
    }
    if (cut.nwin > g->max_win) {
        return gt_fail(MFM_E_INVAL, "internal: window count exceeds the plan");
    }
    if (g->flushed) {
        return gt_fail(MFM_E_STATE, "the gate was flushed: the stream has ended");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GT_TRY(hipSetDevice(g->cfg.device));
    if (g->have_call && g->last_stream != s) {
        GT_TRY(hipStreamSynchronize(g->last_stream)); /* state lives on the device; keep calls ordered */
    }
    return gt_call(g, d_rows, in_stride, nr_in, d_records, record_stride, cut, 0, s);
}

int mfm_gate_flush_device(struct mfm_gate *g, void *stream)
{
    if (!g) {
        return MFM_E_INVAL;
    }
    if (g->flushed) {
        return gt_fail(MFM_E_STATE, "the gate was flushed: the stream has ended");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GT_TRY(hipSetDevice(g->cfg.device));
    if (g->have_call && g->last_stream != s) {
        GT_TRY(hipStreamSynchronize(g->last_stream));
    }
    return gt_call(g, nullptr, 0, 0, nullptr, 0, mfm_gate_cut_of(g->pos, 0, g->W, g->E), 1, s);
}

int mfm_gate_process_host(struct mfm_gate *g, const int16_t *rows, size_t in_stride, size_t nr_in, const struct mfm_level_record *records,
                          size_t record_stride, size_t nr_windows)
{
    if (!g || (!rows && nr_in) || (!records && nr_windows) || record_stride < nr_windows) {
        return MFM_E_INVAL;
    }
    GT_TRY(hipSetDevice(g->cfg.device));
    const uint32_t C = g->cfg.nr_channels;
    const size_t ne = nr_in * g->E;
    int16_t *d_in = nullptr;
    mfm_level_record *d_rec = nullptr;
    GT_TRY(hipMalloc(&d_in, (size_t)C * (ne ? ne : 1) * 2));
    if (hipMalloc(&d_rec, (size_t)C * (nr_windows ? nr_windows : 1) * sizeof(mfm_level_record)) != hipSuccess) {
        (void)hipFree(d_in);
        return MFM_E_NOMEM;
    }
    int rc = MFM_OK;
    if (ne && hipMemcpy2D(d_in, ne * 2, rows, in_stride * 2, ne * 2, C, hipMemcpyHostToDevice) != hipSuccess) {
        rc = MFM_E_DEVICE;
    }
    const size_t rrow = nr_windows * sizeof(mfm_level_record);
    if (rc == MFM_OK && nr_windows &&
        hipMemcpy2D(d_rec, rrow, records, record_stride * sizeof(mfm_level_record), rrow, C, hipMemcpyHostToDevice) != hipSuccess) {
        rc = MFM_E_DEVICE;
    }
    if (rc == MFM_OK) {
        rc = mfm_gate_process_device(g, d_in, ne, nr_in, d_rec, nr_windows, nr_windows, nullptr);
    }
    (void)hipDeviceSynchronize();
    (void)hipFree(d_in);
    (void)hipFree(d_rec);
    return rc;
}

int mfm_gate_fetch(struct mfm_gate *g, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                   size_t *nr_elems)
{
    if (!g || !nr_runs || !nr_elems || (!runs && max_runs) || (!payload && max_elems)) {
        return MFM_E_INVAL;
    }
    *nr_runs = 0;
    *nr_elems = 0;
    if (!g->have_call) {
        return MFM_OK;
    }
    GT_TRY(hipSetDevice(g->cfg.device));
    GT_TRY(hipStreamSynchronize(g->last_stream));
    uint64_t t[4];
    GT_TRY(hipMemcpy(t, g->d_totals, sizeof(t), hipMemcpyDeviceToHost));
    *nr_runs = (size_t)t[GT_T_RUNS];
    *nr_elems = (size_t)t[GT_T_ELEMS];
    if (t[GT_T_OUT_OF_STEP]) {
        return gt_fail(MFM_E_STATE, "level and gate out of step");
    }
    if (t[GT_T_OVERFLOW]) {
        return gt_fail(MFM_E_STATE, "the call's open windows exceed max_open_windows");
    }
    if (t[GT_T_RUNS] > max_runs || t[GT_T_ELEMS] > max_elems) {
        return MFM_E_NOMEM;
    }
    if (t[GT_T_RUNS]) {
        GT_TRY(hipMemcpy(runs, g->d_runs, (size_t)t[GT_T_RUNS] * sizeof(mfm_gate_run), hipMemcpyDeviceToHost));
        GT_TRY(hipMemcpy(payload, g->d_payload, (size_t)t[GT_T_ELEMS] * 2, hipMemcpyDeviceToHost));
    }
    return MFM_OK;
}

int mfm_gate_device_view(struct mfm_gate *g, const struct mfm_gate_run **d_runs, const int16_t **d_payload, const uint64_t **d_totals)
{
    if (!g) {
        return MFM_E_INVAL;
    }
    if (d_runs) {
        *d_runs = g->d_runs;
    }
    if (d_payload) {
        *d_payload = g->d_payload;
    }
    if (d_totals) {
        *d_totals = g->d_totals;
    }
    return MFM_OK;
}

int mfm_hosttwin_gate_call_preroll(uint32_t nr_channels, uint32_t window_samples, uint32_t elems_per_sample, uint32_t preroll_windows,
                                   uint64_t pos, int flush, const int16_t *rows, size_t in_stride, size_t nr_in, int16_t *history,
                                   uint64_t *open_bits, const struct mfm_level_record *records, size_t record_stride, size_t nr_windows,
                                   struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                                   size_t *nr_elems)
{
    if (!nr_channels || !window_samples || (elems_per_sample != 1 && elems_per_sample != 2) || preroll_windows > MFM_GATE_MAX_PREROLL ||
        !history || !open_bits || !nr_runs || !nr_elems || (!rows && nr_in) || (!runs && max_runs) || (!payload && max_elems) ||
        (flush && (nr_in || nr_windows))) {
        return MFM_E_INVAL;
    }
    const uint32_t P = preroll_windows, We = window_samples * elems_per_sample;
    const size_t hstride = (size_t)(P + 1u) * We;
    const mfm_gate_cut cut = mfm_gate_cut_of(pos, nr_in, window_samples, elems_per_sample);
    if (nr_windows != cut.nwin || (cut.nwin && (!records || record_stride < cut.nwin))) {
        return MFM_E_INVAL;
    }
    const uint32_t nrec = cut.nwin, nemit = flush ? P : nrec;
    const uint32_t skip = mfm_gate_pre_skip(cut.k0, P);
    const uint32_t hlen0 = mfm_gate_hist_len(cut.k0, cut.r0, P, We);
    bool wrong = false;
    auto word = [&](uint32_t c, uint32_t i0) { /* gt_word */
        const mfm_level_record *rc = records + c * record_stride;
        uint64_t v = 0;
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t i = i0 + l;
            bool open = false;
            if (i < P) {
                open = (open_bits[c] >> i) & 1ull;
            } else if (i - P < nrec) {
                open = rc[i - P].open != 0;
                wrong |= rc[i - P].window != cut.k0 + (i - P);
            }
            v |= open ? 1ull << l : 0ull;
        }
        return v;
    };
    /* the count pass and the scan */
    uint64_t open_total = 0, run_total = 0;
    for (uint32_t c = 0; c < nr_channels; c++) {
        mfm_gate_walk w{};
        uint64_t lo = word(c, 0);
        for (uint32_t e0 = 0; e0 < nemit; e0 += 64) {
            const uint32_t cnt = nemit - e0 < 64u ? nemit - e0 : 64u;
            const uint64_t hi = word(c, e0 + 64);
            uint32_t dr, dl;
            (void)mfm_gate_walk_step(w, mfm_gate_dilate(lo, hi, P, e0, cnt, skip), cnt, e0 + 64 >= nemit, dr, dl);
            lo = hi;
        }
        open_total += w.opens;
        run_total += w.runs;
    }
    *nr_runs = (size_t)run_total;
    *nr_elems = (size_t)(open_total * We);
    if (wrong) {
        return gt_fail(MFM_E_STATE, "level and gate out of step");
    }
    if (run_total > max_runs || open_total * We > max_elems) {
        return MFM_E_NOMEM; /* nothing written, history and bits included: the caller may call again */
    }
    /* runs and payload */
    uint64_t bo = 0, br = 0;
    for (uint32_t c = 0; c < nr_channels; c++) {
        const int16_t *xr = rows + c * in_stride;
        const int16_t *xlow = history + c * hstride + hlen0;
        mfm_gate_walk w{};
        uint64_t lo = word(c, 0);
        for (uint32_t e0 = 0; e0 < nemit; e0 += 64) {
            const uint32_t cnt = nemit - e0 < 64u ? nemit - e0 : 64u;
            const bool last = e0 + 64 >= nemit;
            const uint64_t hi = word(c, e0 + 64);
            const uint64_t mask = mfm_gate_dilate(lo, hi, P, e0, cnt, skip);
            const uint64_t starts = mfm_gate_starts(w, mask);
            for (uint32_t i = 0; i < cnt; i++) {
                if (!((mask >> i) & 1ull)) {
                    continue;
                }
                const uint64_t at = bo + mfm_gate_slot(w, mask, i);
                for (uint32_t j = 0; j < We; j++) {
                    const int64_t g = mfm_gate_src(e0 + i, j, We, P * We + cut.r0);
                    payload[at * We + j] = g >= 0 ? xr[g] : xlow[g];
                }
                if ((starts >> i) & 1ull) {
                    uint32_t rank, len;
                    bool whole;
                    mfm_gate_run_at(w, mask, starts, i, cnt, last, rank, len, whole);
                    mfm_gate_run &r = runs[br + rank];
                    r.first_window = cut.k0 + e0 + i - P;
                    r.payload_offset = at * We;
                    r.channel = c;
                    if (whole) {
                        r.nr_windows = len;
                    }
                }
            }
            uint32_t done_run = 0, done_len = 0;
            if (mfm_gate_walk_step(w, mask, cnt, last, done_run, done_len)) {
                runs[br + done_run].nr_windows = done_len;
            }
            lo = hi;
        }
        bo += w.opens;
        br += w.runs;
    }
    if (flush) {
        return MFM_OK;
    }
    /* the bits and the history, behind the copy that read them */
    const uint32_t N = (uint32_t)nr_in * elems_per_sample;
    const uint32_t hlen1 = mfm_gate_hist_len(cut.k0 + nrec, cut.r1, P, We);
    std::vector<int16_t> next(hlen1 ? hlen1 : 1);
    for (uint32_t c = 0; c < nr_channels; c++) {
        open_bits[c] = word(c, nrec) & mfm_gate_below(P);
        int16_t *h = history + c * hstride;
        const int16_t *xr = rows + c * in_stride;
        for (uint32_t i = 0; i < hlen1; i++) {
            const int64_t g = mfm_gate_hist_src(i, hlen1, N);
            next[i] = g >= 0 ? xr[g] : h[hlen0 + g];
        }
        memcpy(h, next.data(), (size_t)hlen1 * 2);
    }
    return MFM_OK;
}

/* the twin without pre-roll: P = 0, where the history is the carry, [channel][We], and the bits stay 0.  Every argument
 * check and return code is the one above */
int mfm_hosttwin_gate_call(uint32_t nr_channels, uint32_t window_samples, uint32_t elems_per_sample, uint64_t pos, const int16_t *rows,
                           size_t in_stride, size_t nr_in, int16_t *carry, const struct mfm_level_record *records, size_t record_stride,
                           size_t nr_windows, struct mfm_gate_run *runs, size_t max_runs, size_t *nr_runs, int16_t *payload, size_t max_elems,
                           size_t *nr_elems)
{
    if (!nr_channels) {
        return MFM_E_INVAL;
    }
    std::vector<uint64_t> bits(nr_channels, 0);
    return mfm_hosttwin_gate_call_preroll(nr_channels, window_samples, elems_per_sample, 0, pos, 0, rows, in_stride, nr_in, carry, bits.data(),
                                          records, record_stride, nr_windows, runs, max_runs, nr_runs, payload, max_elems, nr_elems);
}

} /* extern "C" */
