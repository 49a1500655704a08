/*
 * mfm_run_bits.hip - the kernels of the burst chain's sign-bit path (include/multifm_hip.h: mfm_runrs_process_bits_device,
 * mfm_runais_process_bits_device, mfm_runpocsag_process_bits_device), in an object of their own beside the PCM forms'.
 *
 *   rrb_scan_kernel   the burst resampler's scan with out_offset and the total in words of the bits payload
 *                     (mfm_runrs_kernels.h, rr_scan_body<true>).
 *   rrb_fir_kernel    the burst resampler's FIR kernel with the int16 store replaced by a wave-wide ballot of the predicate:
 *                     two finished words per 64 outputs (rr_fir_body<NP, true>), NP as in mfm_runrs.hip.
 *   rb_slice_kernel   the slicer of the burst AIS and POCSAG stages on that payload.  A run's bits start on a payload word, so
 *                     word HIST_WORDS + k of its segment is payload word out_offset + k: a 4-byte copy per 32 samples; the
 *                     history words (the channel's carried tail, or zeros) and the padding word as in the PCM slicers.  The
 *                     two stages differ in the length of the history and in where the tail lies in their state, which are
 *                     arguments.
 *
 * Nothing is floating point and nothing goes through an atomic.
 */
#include <hip/hip_runtime.h>

#include "../../include/multifm_hip.h"
#include "mfm_run_bits.h"
#include "mfm_runrs_kernels.h"

namespace {

__global__ __launch_bounds__(RR_SCAN_THREADS) void rrb_scan_kernel(const RrCall A)
{
    rr_scan_body<true>(A);
}

template <int NP>
__global__ __launch_bounds__(RR_NT) void rrb_fir_kernel(const RrCall A)
{
    rr_fir_body<NP, true>(A);
}

__global__ __launch_bounds__(MFM_RUN_BITS_SLICE_NT) void rb_slice_kernel(const mfm_run_bits_slice A)
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
    const uint32_t w = (b - A.blk_base[r]) * MFM_RUN_BITS_SLICE_NT + threadIdx.x;
    const uint32_t nbw = mfm_runrs_bit_words(run.nr_out);
    if (w >= A.hist_words + nbw + 1u) { /* history, bits, one word of padding */
        return;
    }
    uint32_t word = 0;
    if (w < A.hist_words) {
        word = (run.flags & MFM_RUNRS_BEGINS) ? 0u : A.chan_old[(size_t)run.channel * A.state_words + A.tail_word0 + w];
    } else if (w - A.hist_words < nbw) {
        /* [out_offset, out_offset + nbw) lies within the totals (the plan); bits past nr_out are zero there */
        word = A.bits[run.out_offset + (w - A.hist_words)];
    }
    A.seg[A.seg_base[r] + w] = word;
}

} /* namespace */

extern "C" {

__attribute__((visibility("hidden"))) int mfm_internal_runrs_bits_launch(const void *call, uint32_t np, uint32_t max_blocks, uint32_t lds_bytes,
                                                                         hipStream_t s)
{
    const RrCall &A = *static_cast<const RrCall *>(call);
    hipLaunchKernelGGL(rrb_scan_kernel, dim3(1), dim3(RR_SCAN_THREADS), 0, s, A);
    if (hipPeekAtLastError() != hipSuccess) {
        return MFM_E_DEVICE;
    }
    if (max_blocks) {
        const dim3 grid(max_blocks);
        switch (np / 4u) {
        case 1: hipLaunchKernelGGL((rrb_fir_kernel<4>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 2: hipLaunchKernelGGL((rrb_fir_kernel<8>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 3: hipLaunchKernelGGL((rrb_fir_kernel<12>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 4: hipLaunchKernelGGL((rrb_fir_kernel<16>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 5: hipLaunchKernelGGL((rrb_fir_kernel<20>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 6: hipLaunchKernelGGL((rrb_fir_kernel<24>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 7: hipLaunchKernelGGL((rrb_fir_kernel<28>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        case 8: hipLaunchKernelGGL((rrb_fir_kernel<32>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        default: hipLaunchKernelGGL((rrb_fir_kernel<0>), grid, dim3(RR_NT), lds_bytes, s, A); break;
        }
        if (hipPeekAtLastError() != hipSuccess) {
            return MFM_E_DEVICE;
        }
    }
    return MFM_OK;
}

__attribute__((visibility("hidden"))) int mfm_internal_run_bits_slice(const struct mfm_run_bits_slice *args, uint32_t max_blocks, hipStream_t s)
{
    hipLaunchKernelGGL(rb_slice_kernel, dim3(max_blocks), dim3(MFM_RUN_BITS_SLICE_NT), 0, s, *args);
    return hipPeekAtLastError() == hipSuccess ? MFM_OK : MFM_E_DEVICE;
}

} /* extern "C" */
