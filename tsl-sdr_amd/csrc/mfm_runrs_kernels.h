/*
 * mfm_runrs_kernels.h - the device code of the burst resampler's plan, scan and FIR kernels (see mfm_runrs.hip for the four
 * kernels and what each does), as bodies with the form as a template parameter: mfm_runrs.hip instantiates the PCM form
 * (rr_scan_kernel, rr_fir_kernel<NP>), mfm_run_bits.hip the bits form (rrb_scan_kernel, rrb_fir_kernel<NP>), so the two
 * forms share every line but the store and neither pays for the other; the plan body is rr_plan_kernel's there and, with the
 * bound of the payload ranges taken apart from the load, rrv_plan_kernel's in mfm_runrs_view.hip (the view entries).
 */
#ifndef MFM_RUNRS_KERNELS_H
#define MFM_RUNRS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multifm_hip.h"
#include "mfm_numerics.h"
#include "mfm_run_stage.h"
#include "mfm_runrs.h"

namespace {

constexpr uint32_t RR_NT = 256, RR_OPT = 4, RR_OPB = RR_NT * RR_OPT; /* FIR kernel: threads, outputs per thread / per workgroup */
constexpr uint32_t RR_SCAN_THREADS = MFM_RUN_SCAN_THREADS; /* the block scan and a thread's slice are mfm_run_stage.h's */
constexpr uint32_t RR_NONE = 0xffffffffu;                            /* d_chan_last: the channel has no run in this call */
constexpr uint32_t RR_T_RUNS = 0, RR_T_ELEMS = 1, RR_T_OVERFLOW = 2, RR_T_GATE = 3; /* d_totals[], ours and the gate's */

struct RrPlan { /* what the plan pass found for a run and the FIR and state kernels need again */
    uint32_t p0, pending;
};

struct RrCall {
    const mfm_gate_run *gruns;
    const int16_t *gpayload;
    const uint64_t *gtotals;
    const mfm_runrs_state *chan_old;
    mfm_runrs_state *chan_new;
    const int16_t *pend_old; /* [C][pend_stride] */
    int16_t *pend_new;
    const int16_t *phase;    /* [I][plen] */
    mfm_runrs_run *runs;
    RrPlan *plan;
    uint32_t *nblk;          /* [cap_runs] workgroups per run */
    uint32_t *blk_base;      /* [cap_runs + 1] their exclusive scan */
    uint32_t *bad;           /* [cap_runs] */
    uint32_t *chan_last;     /* [C] */
    uint32_t *ctl;           /* [0] workgroups of the FIR kernel, [1] runs */
    uint64_t *totals;
    int16_t *y;
    uint64_t cap_runs, cap_elems, out_cap;
    uint32_t C, W, I, D, plen, pend_stride, invert, coef_bytes;
    uint32_t *bits;          /* the bits form: the payload of predicate words */
    uint32_t polarity;       /* the bits form: MFM_BITS_NEG or MFM_BITS_POS */
    const mfm_runrs_dc_state *dc_old; /* [C] the DC blocker's state, NULL with the blocker off */
    mfm_runrs_dc_state *dc_new;
    int32_t dc_p;
};

/* 1 / 2 when the gate's totals say that nothing may be read: its own flags, or more than this object was made for */
__device__ __forceinline__ bool rr_refused(const RrCall &A, uint64_t &over, uint64_t &gate)
{
    over = A.gtotals[RR_T_OVERFLOW] ? MFM_RUNRS_OVER_GATE : 0u;
    gate = A.gtotals[RR_T_GATE] ? MFM_RUNRS_GATE_OUT_OF_STEP : 0u;
    if (!over && !gate && (A.gtotals[RR_T_RUNS] > A.cap_runs || A.gtotals[RR_T_ELEMS] > A.cap_elems)) {
        over = MFM_RUNRS_OVER_OWN;
    }
    return over || gate;
}

/*
 * The plan pass, one lane per run (mfm_runrs.hip describes it).  VIEW is the one difference between rr_plan_kernel and the view
 * entries' rrv_plan_kernel (mfm_runrs_view.hip): what a run's payload range is checked against.  Without it that is the totals'
 * own elements, the payload being the gate's whole; with it *payload_elems, how much payload exists, while the totals' elements
 * are only the load rr_refused holds against the capacity (a local route's of the run router).  The FIR and the state kernel read
 * a run's range only from runs this pass let through, so the bound here is the bound of every read.
 */
template <bool VIEW>
__device__ __forceinline__ void rr_plan_body(const RrCall &A, const uint64_t *payload_elems)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t over, gate;
    if (rr_refused(A, over, gate) || r >= A.gtotals[RR_T_RUNS]) { /* surplus lanes, and every lane of a refused call */
        return;
    }
    const uint64_t n = A.gtotals[RR_T_RUNS];
    const uint64_t exists = VIEW ? *payload_elems : A.gtotals[RR_T_ELEMS];
    const mfm_gate_run g = A.gruns[r];
    const uint64_t nsamp = (uint64_t)g.nr_windows * A.W;
    /* VIEW: the load is within cap_elems (rr_refused), so a run of the list it belongs to is; one that is longer is not of that
     * list, and everything behind counts on a run's samples being within the capacity, as they are without VIEW */
    if (g.channel >= A.C || g.payload_offset > exists || nsamp > exists - g.payload_offset || (VIEW && nsamp > A.cap_elems)) {
        A.bad[r] = 1; /* not a gate's run: the scan raises the flag and nothing goes out */
        A.nblk[r] = 0;
        A.runs[r].nr_out = 0;
        return;
    }
    const bool first = r == 0 || A.gruns[r - 1].channel != g.channel;
    const bool last = r + 1 == n || A.gruns[r + 1].channel != g.channel;
    const mfm_runrs_start s = mfm_runrs_start_of(A.chan_old[g.channel], first, g.first_window);
    const mfm_runrs_step st = mfm_runrs_plan_run(A.I, A.D, A.plen, s.phase, s.pending, nsamp);
    mfm_runrs_run o;
    o.first_window = g.first_window;
    o.out_offset = 0; /* the scan */
    o.first_out = s.first_out;
    o.channel = g.channel;
    o.nr_out = (uint32_t)st.nr_out; /* below 2^31: nsamp is within the capacity */
    o.flags = s.begins ? MFM_RUNRS_BEGINS : 0u;
    o.reserved = 0;
    A.runs[r] = o;
    A.plan[r] = RrPlan{ s.phase, s.pending };
    A.nblk[r] = (uint32_t)((st.nr_out + RR_OPB - 1u) / RR_OPB);
    A.bad[r] = 0;
    if (last) {
        A.chan_last[g.channel] = (uint32_t)r;
    }
}

/* BITS: out_offset and the total count 32-bit words of the bits payload (mfm_runrs_bit_words per run), not int16 elements */
template <bool BITS>
__device__ __forceinline__ void rr_scan_body(const RrCall &A)
{
    __shared__ uint64_t lds[RR_SCAN_THREADS / 64];
    uint64_t over, gate;
    if (rr_refused(A, over, gate)) {
        if (threadIdx.x == 0) {
            A.totals[RR_T_RUNS] = 0;
            A.totals[RR_T_ELEMS] = 0;
            A.totals[RR_T_OVERFLOW] = over;
            A.totals[RR_T_GATE] = gate;
            A.ctl[0] = 0;
            A.ctl[1] = 0;
        }
        return;
    }
    const uint64_t n = A.gtotals[RR_T_RUNS]; /* <= cap_runs < 2^32 */
    uint64_t r0, r1;
    mfm_run_slice(n, &r0, &r1);
    uint64_t so = 0, sb = 0, sq = 0;
    uint32_t sw = 0;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        so += A.runs[r].nr_out;
        sq += mfm_runrs_bit_words(A.runs[r].nr_out);
        sb += A.nblk[r];
        sw |= A.bad[r];
    }
    /* the workgroup counts ride in the scan of the outputs: a run has at most nr_out / 1024 + 1 of them, so their sum over
     * fewer than 2^31 runs of fewer than 2^31 outputs stays below 2^32, and the outputs' sum below 2^62 */
    uint64_t to, tb, tq = 0;
    uint64_t bo = mfm_run_block_scan(so, lds, &to);
    uint64_t bb;
    if (BITS) {
        /* the words ride with the workgroup counts: both sums stay below 2^32 (at most to / 32 + n words, which is also why
         * they fit the bits payload when to is within out_cap; a sum beyond that is a refused call and never used) */
        bb = mfm_run_block_scan((sb & 0xffffffffull) | (sq << 32), lds, &tb);
        bo = bb >> 32;
        tq = tb >> 32;
        bb &= 0xffffffffull;
        tb &= 0xffffffffull;
    } else {
        bb = mfm_run_block_scan(sb, lds, &tb);
    }
    /* run lists that are not a gate's (overlapping payload ranges) could ask for more than the output holds */
    const bool wrong = __syncthreads_or(sw != 0) != 0 || to > A.out_cap;
#pragma unroll 1
    for (uint64_t r = r0; r < r1; r++) {
        A.runs[r].out_offset = bo;
        A.blk_base[r] = (uint32_t)bb;
        bo += BITS ? mfm_runrs_bit_words(A.runs[r].nr_out) : A.runs[r].nr_out;
        bb += A.nblk[r];
    }
    if (threadIdx.x == 0) {
        A.blk_base[n] = (uint32_t)tb;
        A.totals[RR_T_RUNS] = wrong ? 0u : n;
        A.totals[RR_T_ELEMS] = wrong ? 0u : (BITS ? tq : to);
        A.totals[RR_T_OVERFLOW] = 0;
        A.totals[RR_T_GATE] = wrong ? MFM_RUNRS_GATE_BAD_RUNS : 0u;
        A.ctl[0] = wrong ? 0u : (uint32_t)tb;
        A.ctl[1] = wrong ? 0u : (uint32_t)n;
    }
}

/* eight samples as one 16-byte access */
struct __attribute__((aligned(16))) rr_x8 {
    uint32_t d[4];
};

__device__ __forceinline__ uint32_t rr_neg2(uint32_t w) /* both int16 halves negated on int16 storage */
{
    return ((0u - (w & 0xffffu)) & 0xffffu) | ((0u - (w >> 16)) << 16);
}

/* one output: the dot product of the samples from x32 position pos on with the pairs of phase ph (in cw when NP > 0, else
 * read from ph_s), Q14-rounded */
template <int NP>
__device__ __forceinline__ int16_t rr_fir_output(const uint32_t *x32, const uint32_t *ph_s, const uint32_t (&cw)[NP > 0 ? NP : 1], uint32_t npairs,
                                                 uint32_t pos, uint32_t ph)
{
    const uint32_t *xw = x32 + (pos >> 1);
    const uint32_t sh = (pos & 1u) * 16u;
    int32_t acc = 0; /* filter/utils.c:94-103, int32 wrap-around */
    uint32_t lo2 = xw[0];
    if (NP > 0) {
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)NP; i++) {
            const uint32_t hi2 = xw[i + 1];
            const uint32_t pr = __builtin_amdgcn_alignbit(hi2, lo2, sh); /* samples pos + 2i, pos + 2i + 1 */
            asm("v_dot2_i32_i16 %0, %1, %2, %0" : "+v"(acc) : "v"(pr), "v"(cw[i]));
            lo2 = hi2;
        }
    } else {
        const uint32_t *cp = ph_s + ph * npairs;
        for (uint32_t i = 0; i < npairs; i++) {
            const uint32_t hi2 = xw[i + 1];
            const uint32_t pr = __builtin_amdgcn_alignbit(hi2, lo2, sh);
            asm("v_dot2_i32_i16 %0, %1, %2, %0" : "+v"(acc) : "v"(pr), "v"(cp[i]));
            lo2 = hi2;
        }
    }
    asm volatile("s_nop 2" : "+v"(acc)); /* a DOT result needs 3 wait states before other VALU code reads it */
    return (int16_t)mfm_r14_wide(acc);   /* utils.c:112 */
}

/* NP > 0: coefficient pairs of the thread's phase in registers, NP = pairs per phase rounded up to a multiple of 4 (the
 * padding pairs are zero); NP = 0: pairs read from LDS, any phase length.  BITS: the predicate of each output goes out as one
 * bit, a wave's 64 outputs as two words, in the place of the int16 store */
template <int NP, bool BITS>
__device__ __forceinline__ void rr_fir_body(const RrCall &A)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rr_smem[];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b >= A.ctl[0]) { /* surplus workgroups: the launch is sized from the capacity */
        return;
    }
    /* the run of workgroup b: the last r with blk_base[r] <= b (runs without output have no workgroup) */
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
    const mfm_gate_run g = A.gruns[r];
    const RrPlan P = A.plan[r];
    const uint32_t n_out = A.runs[r].nr_out, c = A.runs[r].channel;
    const uint64_t y0 = A.runs[r].out_offset;
    const uint32_t j0 = (b - A.blk_base[r]) * RR_OPB;
    const uint32_t cnt = n_out - j0 < RR_OPB ? n_out - j0 : RR_OPB;
    const uint64_t nsamp = (uint64_t)g.nr_windows * A.W;
    const int16_t *run = A.gpayload + g.payload_offset;
    const int16_t *pend = A.pend_old + (size_t)c * A.pend_stride;
    const bool invert = A.invert != 0;

    uint32_t *ph_s = reinterpret_cast<uint32_t *>(rr_smem); /* [I][plen / 2] coefficient pairs */
    const uint32_t npairs = A.plen / 2u;                    /* plen is a multiple of 4 */
    int16_t *x_s = reinterpret_cast<int16_t *>(rr_smem + A.coef_bytes);
    /* filter/polyphase_fir.c:206-211 unrolled to output j of the run: position (p0 + j D) / I, phase (p0 + j D) % I.  One
     * 64-bit division per workgroup; within it everything is relative and fits 32 bits (1024 D + I < 2^31) */
    const uint64_t t0 = P.p0 + (uint64_t)j0 * A.D;
    const uint64_t pos0 = t0 / A.I;
    const uint32_t ph0 = (uint32_t)(t0 - pos0 * A.I);
    /* x_s[0] is the sample `adj` in front of position pos0, where the payload is 16-byte aligned */
    const int64_t e0 = (int64_t)pos0 - (int64_t)P.pending; /* position pos0 as an index into the run's samples */
    const uint32_t adj = (uint32_t)((reinterpret_cast<uintptr_t>(run) / 2u + (uint64_t)e0) & 7u);
    const uint32_t last_rel = (ph0 + (cnt - 1u) * A.D) / A.I;
    const uint32_t nwin = (adj + last_rel + A.plen + 16u + 7u) & ~7u; /* <= x_cap (rr_geometry) */
    for (uint32_t i = tid; i < A.I * npairs; i += RR_NT) {
        ph_s[i] = reinterpret_cast<const uint32_t *>(A.phase)[i];
    }
    for (uint32_t k = tid; k < nwin / 8u; k += RR_NT) {
        const int64_t e = e0 - (int64_t)adj + 8 * (int64_t)k;
        if (e >= 0 && (uint64_t)e + 8u <= nsamp) {
            rr_x8 w = *reinterpret_cast<const rr_x8 *>(run + e);
            if (invert) {
                w.d[0] = rr_neg2(w.d[0]);
                w.d[1] = rr_neg2(w.d[1]);
                w.d[2] = rr_neg2(w.d[2]);
                w.d[3] = rr_neg2(w.d[3]);
            }
            *reinterpret_cast<rr_x8 *>(x_s + 8u * k) = w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                x_s[8u * k + i] = mfm_runrs_sample(pend, P.pending, run, nsamp, e + (int64_t)P.pending + i, invert);
            }
        }
    }
    __syncthreads();
    const uint32_t *x32 = reinterpret_cast<const uint32_t *>(x_s);

    /* one division per thread: its outputs are RR_NT apart, so position and phase advance by constants */
    const uint32_t t_first = ph0 + tid * A.D;
    uint32_t pos = adj + t_first / A.I, ph = t_first % A.I;
    const uint32_t step_pos = (RR_NT * A.D) / A.I, step_ph = (RR_NT * A.D) % A.I;
    constexpr bool REGCOEF = NP > 0;
    uint32_t cw[REGCOEF ? NP : 1];
    if (REGCOEF) {
        /* 256 D is a multiple of I: outputs tid, tid + 256, ... of this workgroup have the same phase */
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)NP; i++) {
            cw[i] = i < npairs ? ph_s[ph * npairs + i] : 0u;
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < RR_OPT; u++) {
        const uint32_t j = tid + u * RR_NT;
        if (BITS) {
            /* the wave's 64 outputs start at wj (uniform over the wave): it leaves together, and its lanes past cnt stay for
             * the ballot and contribute 0 */
            const uint32_t wj = (tid & ~63u) + u * RR_NT;
            if (wj >= cnt) {
                break;
            }
            bool pred = false;
            if (j < cnt) {
                pred = mfm_runrs_bit(rr_fir_output<NP>(x32, ph_s, cw, npairs, pos, ph), A.polarity);
            }
            const unsigned long long word2 = __ballot(pred);
            if ((tid & 63u) == 0u) { /* y0 counts words here; j0 and wj are multiples of 64 */
                uint32_t *dst = A.bits + y0 + (j0 + wj) / 32u;
                dst[0] = (uint32_t)word2;
                if (wj + 32u < cnt) {
                    dst[1] = (uint32_t)(word2 >> 32);
                }
            }
        } else {
            if (j >= cnt) {
                break;
            }
            A.y[y0 + j0 + j] = rr_fir_output<NP>(x32, ph_s, cw, npairs, pos, ph);
        }
        pos += step_pos;
        ph += step_ph;
        if (ph >= A.I) {
            ph -= A.I;
            pos += 1u;
        }
    }
}

} /* namespace */

#endif /* MFM_RUNRS_KERNELS_H */
