/*
 * mfm_runrs_dc.hip - the kernel of the burst resampler's DC blocker (include/multifm_hip.h: mfm_runrs_set_dc_block), an object of
 * its own as mfm_run_bits.hip is, so that mfm_runrs.o keeps the kernels it had.  mfm_runrs.hip queues it between its FIR and its
 * state kernel and holds the two state buffers; the arithmetic is mfm_runrs_dc.h's, which the host twin runs too.
 */
#include <hip/hip_runtime.h>

#include "../../include/multifm_hip.h"
#include "mfm_runrs_dc.h"
#include "mfm_runrs_kernels.h"

namespace {

typedef uint32_t rr_u32x4 __attribute__((ext_vector_type(4))); /* (HIP's uint4 is a struct of unions: arrays of it end up in scratch) */

/* eight samples of the recurrence on one 16-byte group: per sample the three-instruction chain of mfm_dc_block_kernel
 * (mfm_resampler.hip; read that comment first) - the multiply-add of the leak r += y * -p, (x << 14) + r as ONE v_mad_i32_i16
 * that picks the sample's half of the packed word itself, the arithmetic shift - and half a v_perm to pack */
__device__ __forceinline__ rr_u32x4 rr_dc_group(const rr_u32x4 w, uint32_t &r, int32_t &yp, int32_t np)
{
    rr_u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t acc;
        r += (uint32_t)__mul24(yp, np); /* |np| <= 2^15 and |y| <= 2^17: the product fits the 24-bit multiplier */
        asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,0,0,0]" : "=v"(acc) : "v"(w[d]), "s"(16384), "v"(r));
        yp = (int32_t)acc >> 14;
        const uint32_t lo = (uint32_t)yp;
        r += (uint32_t)__mul24(yp, np);
        asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(acc) : "v"(w[d]), "s"(16384), "v"(r));
        yp = (int32_t)acc >> 14;
        o[d] = __builtin_amdgcn_perm((uint32_t)yp, lo, 0x05040100u); /* low halves of (lo, yp) */
    }
    return o;
}

/*
 * The DC blocker, one lane per run, in place on the run's outputs y[out_offset .. out_offset + nr_out).  out_offset has any
 * 2-byte alignment (it is a sum of earlier runs' counts): at most 7 samples singly up to the 16-byte grid, then 16-byte groups
 * - 64 samples per trip with the next 64 requested before the current 64 are worked on, as in mfm_dc_block_kernel (a lane's
 * run is its own cache lines, and a load that is waited for costs a full memory round trip), then the whole groups that are
 * left one at a time, the next requested before the current - then the tail singly.  A wave runs as long as its longest run.
 * No float, no atomics, no LDS, no scratch.
 */
__global__ __launch_bounds__(64) void rr_dc_kernel(const RrCall A)
{
    const uint64_t r_idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_runs = A.totals[RR_T_RUNS]; /* ours, from the scan: 0 when the call was refused */
    if (A.totals[RR_T_OVERFLOW] != 0 || A.totals[RR_T_GATE] != 0 || r_idx >= n_runs) {
        return; /* surplus lanes: the launch is sized from the capacity */
    }
    const mfm_runrs_run run = A.runs[r_idx];
    const bool first = r_idx == 0 || A.runs[r_idx - 1].channel != run.channel;
    const bool last = r_idx + 1 == n_runs || A.runs[r_idx + 1].channel != run.channel;
    mfm_runrs_dc_carry k = mfm_runrs_dc_start(A.dc_old + run.channel, first, run.flags);
    const int32_t p = A.dc_p, np = -p;
    const uint32_t n = run.nr_out;
    int16_t *yy = A.y + run.out_offset; /* out_offset + nr_out <= the call's elements <= out_cap (the scan) */
    uint32_t i = 0;
    uint32_t head = (uint32_t)((8u - ((reinterpret_cast<uintptr_t>(yy) >> 1) & 7u)) & 7u);
    head = head < n ? head : n;
    for (; i < head; i++) {
        yy[i] = mfm_runrs_dc_sample(k, p, yy[i]);
    }
    const uint32_t ng = (n - head) / 8u; /* whole 16-byte groups */
    if (ng) {
        rr_u32x4 *grp = reinterpret_cast<rr_u32x4 *>(yy + head);
        uint32_t r = k.r, g = 0;
        int32_t yp = k.yp, xl = 0; /* xl: the last sample read, x_(n-1) of whatever follows */
        constexpr uint32_t V = 8;
        if (ng >= V) {
            /* two sets of eight groups used in turn, the loop unrolled by two: with one set copied into the other at the end of
             * a trip the compiler moves the copies, and the wait for the loads with them, to the front of the trip */
            rr_u32x4 ga[V], gb[V];
#pragma unroll
            for (uint32_t v = 0; v < V; v++) {
                ga[v] = grp[v];
            }
            for (;;) {
                /* the next 64 samples; behind the last whole trip the same ones again (a valid address, nobody uses them) */
                const rr_u32x4 *pb = grp + (g + 2u * V <= ng ? g + V : g);
#pragma unroll
                for (uint32_t v = 0; v < V; v++) {
                    gb[v] = pb[v];
                }
#pragma unroll
                for (uint32_t v = 0; v < V; v++) {
                    grp[g + v] = rr_dc_group(ga[v], r, yp, np);
                }
                xl = (int32_t)ga[V - 1u][3] >> 16;
                g += V;
                if (g + V > ng) {
                    break;
                }
                const rr_u32x4 *pa = grp + (g + 2u * V <= ng ? g + V : g);
#pragma unroll
                for (uint32_t v = 0; v < V; v++) {
                    ga[v] = pa[v];
                }
#pragma unroll
                for (uint32_t v = 0; v < V; v++) {
                    grp[g + v] = rr_dc_group(gb[v], r, yp, np);
                }
                xl = (int32_t)gb[V - 1u][3] >> 16;
                g += V;
                if (g + V > ng) {
                    break;
                }
            }
        }
        if (g < ng) {
            rr_u32x4 cur = grp[g];
            for (; g < ng; g++) {
                const rr_u32x4 nxt = grp[g + 1u < ng ? g + 1u : g];
                grp[g] = rr_dc_group(cur, r, yp, np);
                xl = (int32_t)cur[3] >> 16;
                cur = nxt;
            }
        }
        k.r = r;
        k.yp = yp;
        k.xq = (uint32_t)xl << 14;
        i = head + 8u * ng;
    }
    for (; i < n; i++) {
        yy[i] = mfm_runrs_dc_sample(k, p, yy[i]);
    }
    if (last) {
        A.dc_new[run.channel] = mfm_runrs_dc_leave(k);
    }
}

} /* namespace */

extern "C" __attribute__((visibility("hidden"))) int mfm_internal_runrs_dc_launch(const void *call, uint32_t cap_runs, hipStream_t s)
{
    const RrCall &A = *static_cast<const RrCall *>(call);
    /* run count and flags are read on the device: the launch is sized from the capacity */
    hipLaunchKernelGGL(rr_dc_kernel, dim3((cap_runs + 63u) / 64u), dim3(64), 0, s, A);
    return hipPeekAtLastError() == hipSuccess ? MFM_OK : MFM_E_DEVICE;
}
