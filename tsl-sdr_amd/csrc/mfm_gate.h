/*
 * mfm_gate.h - the arithmetic of the squelch gate stage (mfm_gate_*, include/multifm_hip.h), stated once for the kernels
 * and for the host twin (mfm_hosttwin_gate_call_preroll) the CPU tests run: how a call is cut into windows, which windows go
 * out, how they form runs, and where each window lies in the payload, in the call's rows and in the history.
 *
 * A row is a run of int16 ELEMENTS (E per sample); a window is We = W * E of them.  A channel's records of one call are
 * walked 64 at a time: `mask` has bit i set when window i of the chunk goes out (mfm_gate_dilate of the record bits), and everything
 * below is popcounts and trailing-zero counts on that mask plus four numbers carried from chunk to chunk.
 */
#ifndef MFM_GATE_H
#define MFM_GATE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define MFM_GATE_MAX_WINDOW_ELEMS (1u << 20) /* W * elems_per_sample at most: the history is up to 64 of these per channel */
#define MFM_GATE_CLOSED 0xffffffffu          /* payload slot of a window that does not go out */

/* what a call of nr_in samples at stream position pos (samples) covers */
struct mfm_gate_cut {
    uint64_t k0;   /* window the call's first sample lies in */
    uint32_t nwin; /* windows the call completes: k0 .. k0 + nwin - 1 */
    uint32_t r0;   /* ELEMENTS of window k0 that earlier calls left: the carry, the history's last part */
    uint32_t r1;   /* elements of the unfinished window k0 + nwin that this call leaves there */
};

__host__ __device__ inline mfm_gate_cut mfm_gate_cut_of(uint64_t pos, uint64_t nr_in, uint32_t W, uint32_t E)
{
    mfm_gate_cut c;
    const uint64_t k1 = (pos + nr_in) / W;
    c.k0 = pos / W;
    c.nwin = (uint32_t)(k1 - c.k0);
    c.r0 = (uint32_t)(pos - c.k0 * W) * E;
    c.r1 = (uint32_t)(pos + nr_in - k1 * W) * E;
    return c;
}

/* element j of candidate m of the call, whose first element lies `back` = P * We + r0 elements in front of the row's: its
 * index in the call's row when >= 0, else counted back from the history's end */
__host__ __device__ inline int64_t mfm_gate_src(uint32_t m, uint32_t j, uint32_t We, uint32_t back)
{
    return (int64_t)((uint64_t)m * We + j) - (int64_t)back;
}

__host__ __device__ inline uint64_t mfm_gate_below(uint32_t i) /* bits 0 .. i - 1 */
{
    return i >= 64 ? ~0ull : ((1ull << i) - 1ull);
}

/* consecutive set bits of mask from bit i upwards */
__host__ __device__ inline uint32_t mfm_gate_ones_from(uint64_t mask, uint32_t i)
{
    const uint64_t z = ~(mask >> i);
    return z ? (uint32_t)__builtin_ctzll(z) : 64u; /* mask >> i shifts zeros in: only i = 0 with all 64 set has no zero */
}

/* a channel's walk through its records, between chunks */
struct mfm_gate_walk {
    uint32_t opens;    /* open windows before this chunk */
    uint32_t runs;     /* runs begun before this chunk */
    uint32_t pend_run; /* rank of the run that reaches this chunk's first window ... */
    uint32_t pend_len; /* ... and its windows so far; 0: none does */
};

/* bit i: window i begins a run (open, and the window in front of it in THIS call is not) */
__host__ __device__ inline uint64_t mfm_gate_starts(const mfm_gate_walk &w, uint64_t mask)
{
    return mask & ~((mask << 1) | (w.pend_len ? 1ull : 0ull));
}

/* window i of the chunk, open: its slot in the channel's part of the payload (in windows) */
__host__ __device__ inline uint32_t mfm_gate_slot(const mfm_gate_walk &w, uint64_t mask, uint32_t i)
{
    return w.opens + (uint32_t)__builtin_popcountll(mask & mfm_gate_below(i));
}

/* window i of the chunk begins a run: its rank among the channel's runs, its windows inside this chunk, and whether that
 * is all of it (it ends inside the chunk, or the chunk is the call's last) */
__host__ __device__ inline void mfm_gate_run_at(const mfm_gate_walk &w, uint64_t mask, uint64_t starts, uint32_t i, uint32_t cnt, bool last,
                                                uint32_t &rank, uint32_t &len, bool &whole)
{
    rank = w.runs + (uint32_t)__builtin_popcountll(starts & mfm_gate_below(i));
    len = mfm_gate_ones_from(mask, i);
    whole = last || i + len < cnt;
}

/*
 * Step the walk over a chunk of cnt windows (mask has no bit at or above cnt).  When the run that reached into the chunk
 * ends in it (or with the call), returns true with its rank and full length: the one descriptor field that the lane
 * which began it could not write.
 */
__host__ __device__ inline bool mfm_gate_walk_step(mfm_gate_walk &w, uint64_t mask, uint32_t cnt, bool last, uint32_t &done_run, uint32_t &done_len)
{
    const uint64_t starts = mfm_gate_starts(w, mask);
    bool done = false;
    if (w.pend_len) {
        const uint32_t lead = mfm_gate_ones_from(mask, 0);
        w.pend_len += lead;
        if (last || lead < cnt) {
            done = true;
            done_run = w.pend_run;
            done_len = w.pend_len;
            w.pend_len = 0;
        }
    }
    if (!last && starts && ((mask >> (cnt - 1)) & 1ull)) { /* the chunk's last run began in it and goes on */
        const uint32_t top = 63u - (uint32_t)__builtin_clzll(starts);
        w.pend_run = w.runs + (uint32_t)__builtin_popcountll(starts) - 1u;
        w.pend_len = cnt - top;
    }
    w.opens += (uint32_t)__builtin_popcountll(mask);
    w.runs += (uint32_t)__builtin_popcountll(starts);
    return done;
}

/*
 * ---- which windows go out, and where their samples are (P = preroll_windows >= 0, mfm_gate_set_preroll) ----------------
 * Window k goes out when any of the records k .. k + P is open, so a call that brings the records K0 .. K1 - 1 decides the
 * windows K0 - P .. K1 - P - 1: its CANDIDATES, e = 0 .. nemit - 1 with k = K0 - P + e (a flush brings no record and
 * decides the P windows left, the missing records taken as closed).  A channel's record bits of the call are one sequence
 * S: bits 0 .. P - 1 are the P records in front of the call (carried as one 64-bit word per channel, bit i = record
 * K0 - P + i, zero where no such record exists), bit P + j is record j of the call, everything behind is closed.  The bit
 * of candidate e is the OR of S[e] .. S[e + P]; for a chunk of 64 candidates that is a shift-and-OR over two words of S.
 * That mask is what the walk above takes.  With P = 0 it is the record bits themselves, no candidate is skipped, and the
 * history below is the carry alone.
 *
 * The samples of the candidates lie in front of the call's rows: the history, a linear buffer per channel that holds the
 * last min(K, P) complete windows and the r elements of the unfinished one, oldest first.  It stands as a virtual prefix
 * in front of the rows, so mfm_gate_src with back = r0 + P * We is the signed source index: the row when >= 0,
 * otherwise counted back from the history's end.  P is at most MFM_GATE_MAX_PREROLL = 63 (include/multifm_hip.h): S[e] ..
 * S[e + P] of 64 candidates then lie in two words.
 */

/* candidates below this one are windows in front of the stream's first (k < 0; after mfm_gate_seek: in front of the window
 * it names): they do not exist and never go out.  k0 and, below, K count from the stream's first window */
__host__ __device__ inline uint32_t mfm_gate_pre_skip(uint64_t k0, uint32_t P)
{
    return k0 < P ? P - (uint32_t)k0 : 0u;
}

/* what the history holds once K windows are complete and r elements of the next one have come */
__host__ __device__ inline uint32_t mfm_gate_hist_len(uint64_t K, uint32_t r, uint32_t P, uint32_t We)
{
    return (uint32_t)(K < P ? K : P) * We + r;
}

/* the mask of the 64 candidates whose record bits begin at lo bit 0 (lo = S[e0 .. e0 + 63], hi = S[e0 + 64 .. e0 + 127]);
 * bits at or above cnt and candidates below skip (counted from candidate 0, the chunk begins at e0) are cleared */
__host__ __device__ inline uint64_t mfm_gate_dilate(uint64_t lo, uint64_t hi, uint32_t P, uint32_t e0, uint32_t cnt, uint32_t skip)
{
    uint64_t d = lo;
    for (uint32_t t = 1; t <= P; t++) { /* P <= 63: both shifts stay below 64 */
        d |= (lo >> t) | (hi << (64u - t));
    }
    d &= mfm_gate_below(cnt);
    if (skip > e0) {
        d &= ~mfm_gate_below(skip - e0);
    }
    return d;
}

/* element i of the history after a call of N elements, as an index into (old history of hlen0 elements ++ the call's row):
 * the row when >= 0, otherwise counted back from the old history's end */
__host__ __device__ inline int64_t mfm_gate_hist_src(uint32_t i, uint32_t hlen1, uint32_t N)
{
    return (int64_t)N - (int64_t)hlen1 + (int64_t)i;
}

#endif /* MFM_GATE_H */
