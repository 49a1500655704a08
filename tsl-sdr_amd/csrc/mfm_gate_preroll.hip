/*
 * mfm_gate_preroll.hip - the pre-roll mode of the squelch gate (mfm_gate_set_preroll, mfm_gate_flush_device): window k of a
 * channel goes out when any of its records k .. k + P is open, so that the samples in front of an opening, where a burst
 * begins, are not lost.  See include/multifm_hip.h for the contract, mfm_gate.h for the arithmetic, mfm_gate.hip for the
 * gate itself: with P = 0 none of this file's kernels is launched.
 *
 * What changes against the plain gate.  A call that brings the records K0 .. K1 - 1 decides the windows K0 - P .. K1 - P - 1
 * (its candidates), whose samples earlier calls brought.  So the device keeps per channel
 *
 *   the history   a LINEAR buffer of at most (P + 1) * We elements: the last min(K, P) complete windows and the unfinished
 *                 one, oldest first.  It stands as a virtual prefix in front of the call's rows; mfm_gate_src gives a signed
 *                 index, the row when >= 0, otherwise counted back from the history's end.  There are two buffers used in
 *                 turn: a call reads one and gtp_hist_kernel, behind the copy, writes the other from (old history ++ rows),
 *                 so a call shorter than the history is a move between buffers and nothing is read after it was written.
 *                 (A ring would save that move; it would also put a second seam into the copy's source.  The move is
 *                 (P + 1) * We elements per channel and call at most.)
 *   the bits      one 64-bit word: the open bits of the P records in front of the next call.  Two words used in turn as
 *                 well: the count pass writes the next one, the runs pass still reads the current one.
 *
 *   gtp_count_kernel  one wave per channel: per chunk of 64 candidates one ballot of the record bits (the word behind it
 *                     is the next chunk's), dilated by shift-and-OR (mfm_gate_dilate); counts as in gt_count_kernel.
 *   gtp_runs_kernel   the same walk with the channel's base: slots and run descriptors; first_window is the true k.
 *   gtp_copy_kernel   the hot path, gt_copy_kernel's shape: destination-aligned 16-byte stores fed by 16-byte loads at any
 *                     2-byte source alignment, four in flight per lane, scalar head and tail.  The body of a piece lies
 *                     wholly in the rows, wholly in the history (every window in front of an opening does) or across the
 *                     seam; the first two take the fast loop from their base pointer, the third the plain loop whose one
 *                     chunk of eight on the seam is put together singly.  A closed candidate is neither read nor written.
 *   gtp_hist_kernel   the history's update, behind the copy.
 *
 * The scan between count and runs is gt_scan_kernel (mfm_gate.hip).  A flush is a call with no rows and no records that
 * decides the P windows left.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/multifm_hip.h"

#include "mfm_gate.h"
#include "mfm_gate_internal.h"

namespace {

struct __attribute__((packed, aligned(2))) gtp_x8u {
    uint32_t d[4];
};
struct __attribute__((aligned(16))) gtp_x8 {
    uint32_t d[4];
};

struct GtpRecs {
    const mfm_level_record *rec;
    size_t rec_stride;
    uint64_t k0;    /* the call's first record */
    uint32_t nrec;  /* records the call brings */
    uint32_t nemit; /* candidates: nrec, at a flush P */
    uint32_t P;
    uint32_t nr_channels;
};

/* 64 bits of the channel's sequence S from bit i0 on (mfm_gate.h): prev below P, then the call's records, then closed */
__device__ __forceinline__ uint64_t gtp_word(const GtpRecs &R, const mfm_level_record *rc, uint64_t prev, uint32_t i0, uint32_t lane,
                                             uint32_t &wrong)
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

__global__ __launch_bounds__(256) void gtp_count_kernel(const GtpRecs R, const uint64_t *__restrict__ bits_in, uint64_t *__restrict__ bits_out,
                                                       uint32_t *__restrict__ cnt_open, uint32_t *__restrict__ cnt_runs, uint32_t *__restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (c >= R.nr_channels) {
        return;
    }
    const mfm_level_record *rc = R.rec + (size_t)c * R.rec_stride;
    const uint64_t prev = bits_in[c];
    const uint32_t skip = mfm_gate_pre_skip(R.k0, R.P);
    mfm_gate_walk w{};
    uint32_t wrong = 0;
    uint64_t lo = gtp_word(R, rc, prev, 0, lane, wrong);
    for (uint32_t e0 = 0; e0 < R.nemit; e0 += 64) {
        const uint32_t cnt = R.nemit - e0 < 64u ? R.nemit - e0 : 64u;
        const uint64_t hi = gtp_word(R, rc, prev, e0 + 64, lane, wrong);
        const uint64_t mask = mfm_gate_dilate(lo, hi, R.P, e0, cnt, skip);
        uint32_t dr, dl;
        (void)mfm_gate_walk_step(w, mask, cnt, e0 + 64 >= R.nemit, dr, dl);
        lo = hi;
    }
    /* the P records in front of the next call: S[nrec .. nrec + P - 1] */
    uint32_t unused = 0;
    const uint64_t next = gtp_word(R, rc, prev, R.nrec, lane, unused) & mfm_gate_below(R.P);
    const bool any_wrong = __ballot(wrong != 0) != 0;
    if (lane == 0) {
        cnt_open[c] = w.opens;
        cnt_runs[c] = w.runs;
        bad[c] = any_wrong ? 1u : 0u;
        bits_out[c] = next;
    }
}

__global__ __launch_bounds__(256) void gtp_runs_kernel(const GtpRecs R, const uint64_t *__restrict__ bits_in, const uint32_t *__restrict__ base_open,
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
    if (totals[MFM_GT_T_OVERFLOW]) { /* the payload cannot take the call: nothing goes out */
        for (uint32_t m = lane; m < R.nemit; m += 64) {
            sc[m] = MFM_GATE_CLOSED;
        }
        return;
    }
    const uint64_t prev = bits_in[c];
    const uint32_t skip = mfm_gate_pre_skip(R.k0, R.P);
    const uint32_t bo = base_open[c];
    mfm_gate_run *rr = runs + base_runs[c];
    mfm_gate_walk w{};
    uint32_t wrong = 0;
    uint64_t lo = gtp_word(R, rc, prev, 0, lane, wrong);
    for (uint32_t e0 = 0; e0 < R.nemit; e0 += 64) {
        const uint32_t cnt = R.nemit - e0 < 64u ? R.nemit - e0 : 64u;
        const bool last = e0 + 64 >= R.nemit;
        const uint64_t hi = gtp_word(R, rc, prev, e0 + 64, lane, wrong);
        const uint64_t mask = mfm_gate_dilate(lo, hi, R.P, e0, cnt, skip);
        const uint64_t starts = mfm_gate_starts(w, mask);
        if (lane < cnt) {
            const bool open = (mask >> lane) & 1ull;
            const uint32_t at = bo + mfm_gate_slot(w, mask, lane);
            sc[e0 + lane] = open ? at : MFM_GATE_CLOSED;
            if ((starts >> lane) & 1ull) {
                uint32_t rank, len;
                bool whole;
                mfm_gate_run_at(w, mask, starts, lane, cnt, last, rank, len, whole);
                rr[rank].first_window = R.k0 + e0 + lane - R.P; /* an open candidate lies at or above skip: k >= 0 */
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

struct GtpCopy {
    size_t stride;        /* of rows, elements */
    uint32_t hist_stride; /* elements */
    uint32_t slot_stride;
    uint32_t We, nemit;
    uint32_t back;        /* P * We + r0: elements of the virtual stream between candidate 0's first and the row's first */
    uint32_t hlen;        /* elements the history holds */
    uint32_t log2g;       /* lanes per piece = 1 << log2g */
    uint32_t npieces;     /* pieces per window */
};

__global__ __launch_bounds__(256) void gtp_copy_kernel(const GtpCopy K, const int16_t *__restrict__ rows, const int16_t *__restrict__ hist,
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
    const uint32_t p0 = (u - m * K.npieces) * MFM_GT_PIECE; /* the piece: elements [p0, p0 + len) of the window */
    const uint32_t len = K.We - p0 < MFM_GT_PIECE ? K.We - p0 : MFM_GT_PIECE;
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
        auto ld = [&](uint32_t t) { return *reinterpret_cast<const gtp_x8u *>(src + 8u * t); };
        auto st = [&](uint32_t t, const gtp_x8u &v) {
            gtp_x8 o;
            o.d[0] = v.d[0];
            o.d[1] = v.d[1];
            o.d[2] = v.d[2];
            o.d[3] = v.d[3];
            *reinterpret_cast<gtp_x8 *>(out + 8u * t) = o;
        };
        uint32_t t = lane;
        for (; t + 3u * G < nbody; t += 4u * G) {
            const gtp_x8u v0 = ld(t), v1 = ld(t + G), v2 = ld(t + 2u * G), v3 = ld(t + 3u * G);
            st(t, v0);
            st(t + G, v1);
            st(t + 2u * G, v2);
            st(t + 3u * G, v3);
        }
        for (; t + G < nbody; t += 2u * G) {
            const gtp_x8u v0 = ld(t), v1 = ld(t + G);
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
                const gtp_x8u v = *reinterpret_cast<const gtp_x8u *>(g >= 0 ? xr + g : xlow + g);
                gtp_x8 o;
                o.d[0] = v.d[0];
                o.d[1] = v.d[1];
                o.d[2] = v.d[2];
                o.d[3] = v.d[3];
                *reinterpret_cast<gtp_x8 *>(dst + head + 8u * t) = o;
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
__global__ __launch_bounds__(256) void gtp_hist_kernel(const int16_t *__restrict__ rows, size_t stride, const int16_t *__restrict__ hist_in,
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

thread_local char g_gtp_error[256] = "";

} /* namespace */

#define GTP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t err_ = (expr);                                                                            \
        if (err_ != hipSuccess) {                                                                            \
            snprintf(g_gtp_error, sizeof(g_gtp_error), "%s failed: %s", #expr, hipGetErrorString(err_));     \
            mfm_internal_set_error(g_gtp_error);                                                             \
            return err_ == hipErrorOutOfMemory ? MFM_E_NOMEM : MFM_E_DEVICE;                                 \
        }                                                                                                    \
    } while (0)

extern "C" {

int mfm_gate_internal_preroll_call(struct mfm_gate *g, const int16_t *d_rows, size_t in_stride, size_t nr_in, const struct mfm_level_record *d_records,
                                   size_t record_stride, uint32_t nwin, int flush, hipStream_t s)
{
    const uint32_t C = g->cfg.nr_channels, P = g->P, We = g->We;
    const mfm_gate_cut cut = mfm_gate_cut_of(g->pos, nr_in, g->W, g->E);
    const uint32_t nemit = flush ? P : nwin;
    const uint32_t hlen0 = mfm_gate_hist_len(cut.k0, cut.r0, P, We);
    const GtpRecs R{ d_records, record_stride, cut.k0, nwin, nemit, P, C };
    const int16_t *hin = g->d_hist[g->cur];
    int16_t *hout = g->d_hist[g->cur ^ 1u];
    hipLaunchKernelGGL(gtp_count_kernel, dim3((C + 3) / 4), dim3(256), 0, s, R, g->d_bits[g->cur], g->d_bits[g->cur ^ 1u], g->d_cnt_open,
                       g->d_cnt_runs, g->d_bad);
    GTP_TRY(hipGetLastError());
    const int rc = mfm_gate_internal_scan(g, s);
    if (rc != MFM_OK) {
        return rc;
    }
    if (nemit) {
        hipLaunchKernelGGL(gtp_runs_kernel, dim3((C + 3) / 4), dim3(256), 0, s, R, g->d_bits[g->cur], g->d_base_open, g->d_base_runs, g->d_totals,
                           g->d_runs, g->d_slot, g->slot_stride, We);
        GTP_TRY(hipGetLastError());
        const GtpCopy K{ in_stride, g->hist_stride, g->slot_stride, We, nemit, P * We + cut.r0, hlen0, g->log2g, g->npieces };
        const uint64_t pieces = (uint64_t)nemit * g->npieces;
        const uint32_t per_block = 256u >> g->log2g;
        hipLaunchKernelGGL(gtp_copy_kernel, dim3((uint32_t)((pieces + per_block - 1) / per_block), C), dim3(256), 0, s, K, d_rows, hin, g->d_slot,
                           g->d_payload);
        GTP_TRY(hipGetLastError());
    }
    if (flush) {
        g->flushed = true; /* the history is of no more use; the unfinished window is dropped */
    } else if (nr_in) {    /* nr_in == 0 leaves the history as it is (and the bits: S[0 .. P - 1] is prev) */
        const uint32_t N = (uint32_t)nr_in * g->E;
        const uint32_t hlen1 = mfm_gate_hist_len(cut.k0 + nwin, cut.r1, P, We);
        if (hlen1) {
            hipLaunchKernelGGL(gtp_hist_kernel, dim3((hlen1 + 255) / 256, C), dim3(256), 0, s, d_rows, in_stride, hin, hout, g->hist_stride, hlen0,
                               hlen1, N);
            GTP_TRY(hipGetLastError());
        }
    }
    if (!flush && nr_in) {
        g->cur ^= 1u; /* both the bits (written by the count pass) and the history; with no sample both stay as they are */
    }
    g->pos += nr_in;
    g->last_stream = s;
    g->have_call = true;
    return MFM_OK;
}

int mfm_gate_set_preroll(struct mfm_gate *g, uint32_t preroll_windows)
{
    if (!g) {
        return MFM_E_INVAL;
    }
    if (g->have_call || g->flushed) {
        return mfm_gate_internal_fail(MFM_E_STATE, "mfm_gate_set_preroll comes before the first process call");
    }
    const uint32_t P = preroll_windows, C = g->cfg.nr_channels;
    char msg[200];
    if (P > MFM_GATE_MAX_PREROLL) {
        snprintf(msg, sizeof(msg), "preroll_windows above MFM_GATE_MAX_PREROLL = %u", MFM_GATE_MAX_PREROLL);
        return mfm_gate_internal_fail(MFM_E_INVAL, msg);
    }
    const uint32_t hist_stride = ((P + 1u) * g->We + 7u) & ~7u; /* <= 64 * 2^20 + 7 */
    const uint64_t hist_bytes = (uint64_t)C * hist_stride * 2u;
    if (P && hist_bytes > MFM_GATE_MAX_HISTORY_BYTES) {
        snprintf(msg, sizeof(msg), "the history, (P + 1) windows of int16 per channel = %llu bytes, exceeds MFM_GATE_MAX_HISTORY_BYTES = %llu",
                 (unsigned long long)hist_bytes, (unsigned long long)MFM_GATE_MAX_HISTORY_BYTES);
        return mfm_gate_internal_fail(MFM_E_INVAL, msg);
    }
    const uint32_t per_ch = g->max_win > P ? g->max_win : P; /* candidates per channel and call at most: a flush has P */
    const uint64_t all = (uint64_t)C * per_ch;
    if (all > 0xfffffffeull) {
        return mfm_gate_internal_fail(MFM_E_INVAL, "nr_channels * preroll_windows must stay below 2^32 - 1");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || g->cfg.device >= ndev) {
        return MFM_E_DEVICE;
    }
    GTP_TRY(hipSetDevice(g->cfg.device));
    for (int i = 0; i < 2; i++) {
        (void)hipFree(g->d_hist[i]);
        (void)hipFree(g->d_bits[i]);
        g->d_hist[i] = nullptr;
        g->d_bits[i] = nullptr;
    }
    g->P = 0;
    if (!P) {
        return MFM_OK;
    }
    const uint32_t have = g->slot_stride ? g->slot_stride : g->max_win; /* what d_slot holds per channel */
    if (per_ch > have) {
        uint32_t *slot = nullptr;
        GTP_TRY(hipMalloc(&slot, (size_t)C * per_ch * 4));
        (void)hipFree(g->d_slot);
        g->d_slot = slot;
    }
    g->slot_stride = per_ch > have ? per_ch : have;
    /* the default capacity holds any call, and a flush is one; a caller-chosen capacity stays, but the run list must hold
     * what fits it: a flush has up to (P + 1) / 2 runs per channel */
    const uint64_t cap_windows = 0 == g->cfg.max_open_windows && all > g->cap_windows ? all : g->cap_windows;
    const uint64_t most_runs = (uint64_t)C * ((per_ch + 1) / 2);
    const uint64_t cap_runs = cap_windows < most_runs ? cap_windows : most_runs;
    if (cap_runs > g->cap_runs) {
        mfm_gate_run *runs = nullptr;
        GTP_TRY(hipMalloc(&runs, (size_t)cap_runs * sizeof(mfm_gate_run)));
        (void)hipFree(g->d_runs);
        g->d_runs = runs;
        g->cap_runs = cap_runs;
    }
    if (cap_windows > g->cap_windows) {
        int16_t *payload = nullptr;
        GTP_TRY(hipMalloc(&payload, (size_t)cap_windows * g->We * 2));
        (void)hipFree(g->d_payload);
        g->d_payload = payload;
        g->cap_windows = cap_windows;
    }
    for (int i = 0; i < 2; i++) {
        GTP_TRY(hipMalloc(&g->d_hist[i], (size_t)hist_bytes));
        GTP_TRY(hipMalloc(&g->d_bits[i], (size_t)C * 8));
        GTP_TRY(hipMemset(g->d_hist[i], 0, (size_t)hist_bytes));
        GTP_TRY(hipMemset(g->d_bits[i], 0, (size_t)C * 8));
    }
    GTP_TRY(hipDeviceSynchronize());
    g->hist_stride = hist_stride;
    g->cur = 0;
    g->P = P;
    return MFM_OK;
}

int mfm_gate_flush_device(struct mfm_gate *g, void *stream)
{
    if (!g) {
        return MFM_E_INVAL;
    }
    if (g->flushed) {
        return mfm_gate_internal_fail(MFM_E_STATE, "the gate was flushed: the stream has ended");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GTP_TRY(hipSetDevice(g->cfg.device));
    if (g->have_call && g->last_stream != s) {
        GTP_TRY(hipStreamSynchronize(g->last_stream));
    }
    if (g->P) {
        return mfm_gate_internal_preroll_call(g, nullptr, 0, 0, nullptr, 0, 0, 1, s);
    }
    /* P = 0: nothing is left to decide; the call's result is empty */
    GTP_TRY(hipMemsetAsync(g->d_totals, 0, 4 * 8, s));
    g->flushed = true;
    g->last_stream = s;
    g->have_call = true;
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
    auto word = [&](uint32_t c, uint32_t i0) { /* gtp_word */
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
        return mfm_gate_internal_fail(MFM_E_STATE, "level and gate out of step");
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

} /* extern "C" */
